// lift_batch.hpp -- the lifting transform for a BATCH of slices resident in HBM, over LoD structures the caller
// already holds (what gpcc_dev_lod_build leaves: predictor order, indices slice relative).
//
// lift_kernels.hpp takes a level of detail of ONE slice as a parallel step, so a slice of L levels is about 7 L
// launches and a batch of S slices S times that.  Slices are independent, so their levels can be taken together:
// a STEP is one LoD transition of every slice at once,
//   forward and quantisation weights   step t takes level num_lods_s - 1 - t of slice s (finest first)
//   inverse                            step t takes level t + 1                         (coarsest first)
// and a slice with fewer levels is idle in the later steps; an empty LoD is an empty range.  Per step and
// direction two prefix tables [num_slices + 1] say where each slice's refinement range (the predictors of the
// level) and coarser range (the receivers of the update, [0, npl[l - 1])) start among the step's threads: thread g
// finds its slice with find_slice over the prefix, its predictor is lo_s + (g - prefix[s]).  A step that is empty
// for every slice is not launched.
//
// Launches of one call, L the largest num_lods of the batch -- none depends on num_slices:
//   forward   at most 7 + 7 (L - 1):  check, init, [scalable weights], (L - 1) weights, 3 (L - 1) forward steps,
//                                     [LCP sums, LCP resolve], quantise, 3 (L - 1) inverse steps, write-back
//   inverse   at most 5 + 4 (L - 1):  check, init, [scalable weights], (L - 1) weights, quantise,
//                                     3 (L - 1) inverse steps, write-back
//
// The per-slice facts (LiftSlice: base, sizes, the ranges of lift_replay_ranges, QP layers, flags, region boxes)
// are a table in device memory, built on the host by lift_batch_plan and uploaded once per call with the prefix
// tables; never a kernel argument, its size follows num_slices.  All working-array indices are base_s + i, the
// neighbour indices stay slice relative.  The arithmetic is that of lift_kernels.hpp: the kernels here call its
// __device__ bodies with the arrays of the predictor's slice.  Update sums are 64-bit integer atomics, so results
// do not depend on the order of execution.
//
// The structure is the caller's memory: lift_batch_check_kernel runs first and states what check_neighbour_tables
// states on the host (counts in 0..3, point indices in [0, n_s), every neighbour in [0, npl[l - 1]) of its
// predictor's level); it sets the verdict word, and every later kernel reads that word first and does nothing when
// it is set.  No kernel dereferences an index the check has not passed.
//
// The plan and launch functions are what the library (gpcc_dev_lift_forward / _inverse) and the emulator harness
// (tests/emu/lift_batch_emu_harness.cpp) both call.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include <hip/hip_runtime.h>

#include "gpcc_attr_mi355.h"
#include "lift_kernels.hpp"
#include "raht_marshal.hpp"

namespace gpcc {

constexpr int kLiftBatchBlock = 256;
constexpr int32_t kLiftBatchMaxSlices = 1 << 18;  // (slice, LoD) keys stay far inside an int

// what the kernels know about one slice
struct LiftSlice {
  int32_t base, n;                 // first point of the slice in the batch, its points
  int32_t num_lods;
  int32_t npl[GPCC_MAX_LODS];      // cumulative LoD sizes
  int32_t num_ranges;              // lift_replay_ranges
  int32_t range_start[kMaxLodRanges];
  int32_t range_qlayer[kMaxLodRanges];
  int32_t range_lcp[kMaxLodRanges];
  int32_t lcp_enabled;             // the flag, and three components
  int32_t scalable;                // quantisation weights of the scalable structure
  int32_t bitdepth;
  int32_t layer_qp[GPCC_MAX_QP_LAYERS][2];
  int32_t max_qp, fixed_point_qp_offset;
  gpcc_qp_regions regions;         // num_qp_regions == 0: no offsets
};

// the batch as the kernels see it (pointers into device memory)
struct LiftBatch {
  int32_t num_slices, n, c;
  int32_t* verdict;                // 0: the structure passed the check
  const int32_t* pt_off;           // [num_slices + 1] the batch's offsets
  const LiftSlice* slice;          // [num_slices]
  const int32_t* nc;               // [n]     the caller's structure
  const int32_t* ni;               // [n][3]
  const int32_t* nw;               // [n][3]
  const int32_t* indexes;          // [n]
  const int32_t* xyz;              // [n][3] point order (read only by slices with regions)
  int32_t* attrs;                  // [n][c] point order
  int32_t* coeffs;                 // [n][c] coding order
  int8_t* lcp;                     // [num_slices][GPCC_MAX_LODS]
  int64_t* a;                      // [n][c] working values, coding order
  unsigned long long* qw;          // [n] quantisation weights
  unsigned long long* uw;          // [n] update weight sums
  unsigned long long* up;          // [n][c] update sums
  long long* lcp_sums;             // [num_slices][GPCC_MAX_LODS][2]
  const RsqrtLut* rsqrt;
};

// one step: the prefix of its threads over the slices, its direction
struct LiftStep {
  const int32_t* prefix;  // [num_slices + 1]
  int32_t total;          // prefix[num_slices]
  int32_t t, inverse;
};

// ---- the host's plan -------------------------------------------------------------------------------------------
// `meta` is one block, uploaded as it stands: the verdict word (zero), the offsets, the slice table, the four
// prefix tables [steps][num_slices + 1] and the slices' LCP coefficients (the decoder's input, the encoder's
// output).  The at_* are byte offsets into it.
struct LiftBatchPlan {
  std::vector<char> meta;
  size_t at_pt_off = 0, at_slice = 0, at_prefix[2][2] = {{0, 0}, {0, 0}} /* [inverse][coarse] */, at_lcp = 0;
  int32_t num_slices = 0, c = 0, steps = 0;  // steps: the largest num_lods - 1
  int64_t n = 0;
  bool any_lcp = false, any_scalable = false, all_scalable = true, any_region = false;

  const int32_t* prefix(int inverse, int coarse, int t) const
  {
    return (const int32_t*)(meta.data() + at_prefix[inverse][coarse]) + (size_t)t * (num_slices + 1);
  }
  int32_t total(int inverse, int coarse, int t) const { return prefix(inverse, coarse, t)[num_slices]; }
};

// level of slice `sl` in step t, 0: the slice is idle
inline int
lift_step_level_host(int num_lods, int t, int inverse)
{
  const int l = inverse ? t + 1 : num_lods - 1 - t;
  return l >= 1 && l < num_lods ? l : 0;
}

// lift [num_slices] as the entry takes them (checked by the caller); lcp_in: the decoder's coefficients
// [num_slices][GPCC_MAX_LODS] or null
inline void
lift_batch_plan(
  LiftBatchPlan& plan, const gpcc_lift_params* lift, int32_t num_slices, const int64_t* offsets, int32_t c,
  const int8_t* lcp_in)
{
  const size_t S = (size_t)num_slices;
  plan.num_slices = num_slices;
  plan.c = c;
  plan.n = offsets[num_slices];
  plan.steps = 0;
  for (size_t s = 0; s < S; s++) {
    plan.steps = plan.steps < lift[s].num_lods - 1 ? lift[s].num_lods - 1 : plan.steps;
    const bool scalable = lift[s].scalable_lifting_enabled_flag != 0;
    plan.any_scalable = plan.any_scalable || scalable;
    plan.all_scalable = plan.all_scalable && scalable;
    plan.any_lcp = plan.any_lcp || (c == 3 && lift[s].last_component_prediction_enabled_flag);
    plan.any_region = plan.any_region || lift[s].num_qp_regions > 0;
  }
  size_t at = 16;  // the verdict word
  plan.at_pt_off = at;
  at += sizeof(int32_t) * (S + 1);
  plan.at_slice = at;
  at += sizeof(LiftSlice) * S;
  for (int inverse = 0; inverse < 2; inverse++)
    for (int coarse = 0; coarse < 2; coarse++) {
      plan.at_prefix[inverse][coarse] = at;
      at += sizeof(int32_t) * (S + 1) * (size_t)plan.steps;
    }
  plan.at_lcp = at;
  at += S * GPCC_MAX_LODS;
  plan.meta.assign(at, 0);

  int32_t* pt_off = (int32_t*)(plan.meta.data() + plan.at_pt_off);
  LiftSlice* tab = (LiftSlice*)(plan.meta.data() + plan.at_slice);
  for (size_t s = 0; s <= S; s++)
    pt_off[s] = (int32_t)offsets[s];
  for (size_t s = 0; s < S; s++) {
    const gpcc_lift_params& p = lift[s];
    LiftSlice& sl = tab[s];
    sl.base = (int32_t)offsets[s];
    sl.n = (int32_t)(offsets[s + 1] - offsets[s]);
    sl.num_lods = p.num_lods;
    for (int l = 0; l < p.num_lods; l++)
      sl.npl[l] = p.num_points_in_lod[l];
    sl.num_ranges = lift_replay_ranges(&p, sl.n, sl.range_start, sl.range_qlayer, sl.range_lcp);
    sl.lcp_enabled = p.last_component_prediction_enabled_flag && c == 3;
    sl.scalable = p.scalable_lifting_enabled_flag != 0;
    sl.bitdepth = p.bitdepth;
    memcpy(sl.layer_qp, p.layer_qp, sizeof(sl.layer_qp));
    sl.max_qp = p.max_qp;
    sl.fixed_point_qp_offset = p.fixed_point_qp_offset;
    sl.regions.num_qp_regions = p.num_qp_regions;
    memcpy(sl.regions.qp_region_min, p.qp_region_min, sizeof(p.qp_region_min));
    memcpy(sl.regions.qp_region_max, p.qp_region_max, sizeof(p.qp_region_max));
    memcpy(sl.regions.qp_region_offset, p.qp_region_offset, sizeof(p.qp_region_offset));
  }
  for (int inverse = 0; inverse < 2; inverse++)
    for (int t = 0; t < plan.steps; t++) {
      int32_t* fine = (int32_t*)plan.prefix(inverse, 0, t);
      int32_t* coarse = (int32_t*)plan.prefix(inverse, 1, t);
      fine[0] = coarse[0] = 0;
      for (size_t s = 0; s < S; s++) {
        const int l = lift_step_level_host(lift[s].num_lods, t, inverse);
        const int32_t* npl = lift[s].num_points_in_lod;
        const int32_t cnt = l ? npl[l] - npl[l - 1] : 0;
        fine[s + 1] = fine[s] + cnt;
        coarse[s + 1] = coarse[s] + (cnt ? npl[l - 1] : 0);  // (an empty LoD updates nobody)
      }
    }
  if (lcp_in)
    memcpy(plan.meta.data() + plan.at_lcp, lcp_in, S * GPCC_MAX_LODS);
}

// the kernels' view, `d_meta` where plan.meta has been uploaded to; the caller adds its own buffers
inline void
lift_batch_view(LiftBatch& b, const LiftBatchPlan& plan, char* d_meta)
{
  b.num_slices = plan.num_slices;
  b.n = (int32_t)plan.n;
  b.c = plan.c;
  b.verdict = (int32_t*)d_meta;
  b.pt_off = (const int32_t*)(d_meta + plan.at_pt_off);
  b.slice = (const LiftSlice*)(d_meta + plan.at_slice);
  b.lcp = (int8_t*)(d_meta + plan.at_lcp);
}

inline LiftStep
lift_batch_step(const LiftBatchPlan& plan, const char* d_meta, int inverse, int coarse, int t)
{
  LiftStep st;
  st.prefix = (const int32_t*)(d_meta + plan.at_prefix[inverse][coarse]) + (size_t)t * (plan.num_slices + 1);
  st.total = plan.total(inverse, coarse, t);
  st.t = t;
  st.inverse = inverse;
  return st;
}

// ---- device side -------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool
lift_batch_refused(const LiftBatch& b)
{
  return __hip_atomic_load(b.verdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

// level of detail of predictor i of a slice
__device__ __forceinline__ int
lift_level_of(const LiftSlice& sl, int i)
{
  int l = 0;
  while (l < sl.num_lods - 1 && i >= sl.npl[l])
    l++;
  return l;
}

// thread g of a step -> its slice and, slice relative, its predictor (refinement range) or receiver (coarser range)
__device__ __forceinline__ int
lift_step_slice(const LiftBatch& b, const LiftStep& st, int g, bool coarse, int& i)
{
  const int s = find_slice(st.prefix, b.num_slices, g);
  const LiftSlice& sl = b.slice[s];
  const int l = st.inverse ? st.t + 1 : sl.num_lods - 1 - st.t;
  i = (coarse ? 0 : sl.npl[l - 1]) + (g - st.prefix[s]);
  return s;
}

// what check_neighbour_tables states on the host, for every predictor of the batch
__global__ __launch_bounds__(kLiftBatchBlock) void
lift_batch_check_kernel(LiftBatch b)
{
  for (int g = blockIdx.x * kLiftBatchBlock + threadIdx.x; g < b.n; g += gridDim.x * kLiftBatchBlock) {
    const int s = find_slice(b.pt_off, b.num_slices, g);
    const LiftSlice& sl = b.slice[s];
    const int i = g - sl.base;
    const int cnt = b.nc[g], pt = b.indexes[g];
    bool bad = cnt < 0 || cnt > 3 || pt < 0 || pt >= sl.n;
    if (!bad) {
      const int l = lift_level_of(sl, i);
      const int coarser = l ? sl.npl[l - 1] : 0;  // where the predictor's level starts
      for (int j = 0; j < cnt; j++) {
        const int v = b.ni[3 * (size_t)g + j];
        bad = bad || v < 0 || v >= coarser;
      }
    }
    if (bad)
      atomicOr(b.verdict, 1);
  }
}

__global__ __launch_bounds__(kLiftBatchBlock) void
lift_batch_init_kernel(LiftBatch b, int encoder)
{
  if (lift_batch_refused(b))
    return;
  for (int g = blockIdx.x * kLiftBatchBlock + threadIdx.x; g < b.n; g += gridDim.x * kLiftBatchBlock) {
    const int s = find_slice(b.pt_off, b.num_slices, g);
    const size_t base = (size_t)b.slice[s].base;
    lift_init_point(
      b.c, encoder, b.attrs + base * b.c, b.indexes + base, b.a + base * b.c, b.qw + base, b.uw + base,
      b.up + base * b.c, (int)(g - base));
  }
  const int sums = b.num_slices * 2 * GPCC_MAX_LODS;
  for (int k = blockIdx.x * kLiftBatchBlock + threadIdx.x; k < sums; k += gridDim.x * kLiftBatchBlock)
    b.lcp_sums[k] = 0;
}

// the slices with the scalable structure: their weights in closed form
__global__ __launch_bounds__(kLiftBatchBlock) void
lift_batch_quant_weights_scalable_kernel(LiftBatch b)
{
  if (lift_batch_refused(b))
    return;
  for (int g = blockIdx.x * kLiftBatchBlock + threadIdx.x; g < b.n; g += gridDim.x * kLiftBatchBlock) {
    const int s = find_slice(b.pt_off, b.num_slices, g);
    const LiftSlice& sl = b.slice[s];
    if (sl.scalable)
      b.qw[g] = quant_weight_scalable_point(sl.n, sl.num_lods, sl.npl, g - sl.base);
  }
}

// ... and the others: one step of PCCComputeQuantizationWeights
__global__ __launch_bounds__(kLiftBatchBlock) void
lift_batch_quant_weights_kernel(LiftBatch b, LiftStep st)
{
  if (lift_batch_refused(b))
    return;
  for (int g = blockIdx.x * kLiftBatchBlock + threadIdx.x; g < st.total; g += gridDim.x * kLiftBatchBlock) {
    int i;
    const int s = lift_step_slice(b, st, g, false, i);
    const LiftSlice& sl = b.slice[s];
    if (sl.scalable)
      continue;
    const size_t base = (size_t)sl.base;
    lift_quant_weights_point(b.nc + base, b.ni + 3 * base, b.nw + 3 * base, b.qw + base, i);
  }
}

template<int C>
__global__ __launch_bounds__(kLiftBatchBlock) void
lift_batch_predict_kernel(LiftBatch b, LiftStep st, int direct)
{
  if (lift_batch_refused(b))
    return;
  for (int g = blockIdx.x * kLiftBatchBlock + threadIdx.x; g < st.total; g += gridDim.x * kLiftBatchBlock) {
    int i;
    const size_t base = (size_t)b.slice[lift_step_slice(b, st, g, false, i)].base;
    lift_predict_point<C>(b.nc + base, b.ni + 3 * base, b.nw + 3 * base, b.a + base * C, i, direct);
  }
}

template<int C>
__global__ __launch_bounds__(kLiftBatchBlock) void
lift_batch_update_scatter_kernel(LiftBatch b, LiftStep st)
{
  if (lift_batch_refused(b))
    return;
  for (int g = blockIdx.x * kLiftBatchBlock + threadIdx.x; g < st.total; g += gridDim.x * kLiftBatchBlock) {
    int i;
    const size_t base = (size_t)b.slice[lift_step_slice(b, st, g, false, i)].base;
    lift_update_scatter_point<C>(
      b.nc + base, b.ni + 3 * base, b.nw + 3 * base, b.qw + base, b.uw + base, b.up + base * C, b.a + base * C, i);
  }
}

// st: the step's COARSER ranges
template<int C>
__global__ __launch_bounds__(kLiftBatchBlock) void
lift_batch_update_apply_kernel(LiftBatch b, LiftStep st, int direct)
{
  if (lift_batch_refused(b))
    return;
  for (int g = blockIdx.x * kLiftBatchBlock + threadIdx.x; g < st.total; g += gridDim.x * kLiftBatchBlock) {
    int i;
    const size_t base = (size_t)b.slice[lift_step_slice(b, st, g, true, i)].base;
    lift_update_apply_point<C>(b.uw + base, b.up + base * C, b.a + base * C, i, direct);
  }
}

// per-slice, per-LoD sums of computeLastComponentPredictionCoeff (three components)
__global__ __launch_bounds__(kLiftBatchBlock) void
lift_batch_lcp_sums_kernel(LiftBatch b)
{
  if (lift_batch_refused(b))
    return;
  const int lane = threadIdx.x & 63;
  // wave-uniform loop: every lane of a wavefront takes part in the shuffles
  for (int64_t first = (int64_t)blockIdx.x * kLiftBatchBlock + (threadIdx.x & ~63); first < b.n;
       first += (int64_t)gridDim.x * kLiftBatchBlock) {
    const int g = (int)first + lane;
    long long m12 = 0, m11 = 0;
    int key = -1;  // slice and LoD; -1: nothing to add (behind the batch, or a slice without the flag)
    if (g < b.n) {
      const int s = find_slice(b.pt_off, b.num_slices, g);
      const LiftSlice& sl = b.slice[s];
      if (sl.lcp_enabled) {
        const int i = g - sl.base;
        lift_lcp_products(b.a + (size_t)sl.base * 3, i, m12, m11);
        key = s * GPCC_MAX_LODS + lift_level_of(sl, i);
      }
    }
    // one atomic pair per wavefront when its lanes share slice and LoD (almost always in a batch of large
    // slices: indices are LoD-ordered); integer sums, order irrelevant
    const int key0 = __shfl(key, 0);
    if (__all(key < 0 || key == key0)) {
      long long s12 = m12, s11 = m11;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        s12 += __shfl_xor(s12, d);
        s11 += __shfl_xor(s11, d);
      }
      if (lane == 0 && key0 >= 0) {
        atomicAdd((unsigned long long*)&b.lcp_sums[2 * (size_t)key0], (unsigned long long)s12);
        atomicAdd((unsigned long long*)&b.lcp_sums[2 * (size_t)key0 + 1], (unsigned long long)s11);
      }
    } else if (key >= 0) {
      atomicAdd((unsigned long long*)&b.lcp_sums[2 * (size_t)key], (unsigned long long)m12);
      atomicAdd((unsigned long long*)&b.lcp_sums[2 * (size_t)key + 1], (unsigned long long)m11);
    }
  }
}

// one thread per slice
__global__ __launch_bounds__(kLiftBatchBlock) void
lift_batch_lcp_resolve_kernel(LiftBatch b)
{
  if (lift_batch_refused(b))
    return;
  for (int s = blockIdx.x * kLiftBatchBlock + threadIdx.x; s < b.num_slices; s += gridDim.x * kLiftBatchBlock) {
    const LiftSlice& sl = b.slice[s];
    if (sl.lcp_enabled)
      lift_lcp_resolve(
        sl.num_lods, sl.npl, b.lcp_sums + (size_t)s * 2 * GPCC_MAX_LODS, b.lcp + (size_t)s * GPCC_MAX_LODS);
  }
}

template<int C>
__global__ __launch_bounds__(kLiftBatchBlock) void
lift_batch_quantise_kernel(LiftBatch b, int encoder)
{
  GPCC_VGPR_FLOOR_64();
  __shared__ RsqrtLut lut;
  if (lift_batch_refused(b))  // (the word is final since the check kernel ended: the same for every thread)
    return;
  for (int i = threadIdx.x; i < 96; i += kLiftBatchBlock) {
    lut.r3[i] = b.rsqrt->r3[i];
    lut.rc[i] = b.rsqrt->rc[i];
  }
  __syncthreads();
  for (int g = blockIdx.x * kLiftBatchBlock + threadIdx.x; g < b.n; g += gridDim.x * kLiftBatchBlock) {
    const int s = find_slice(b.pt_off, b.num_slices, g);
    const LiftSlice& sl = b.slice[s];
    const int i = g - sl.base;
    const int r = lift_range_of(sl.num_ranges, sl.range_start, i);
    const int lcpc = (C == 3 && sl.lcp_enabled) ? b.lcp[(size_t)s * GPCC_MAX_LODS + sl.range_lcp[r]] : 0;
    int32_t o0 = 0, o1 = 0;
    if (sl.regions.num_qp_regions > 0) {
      // the offsets of the coefficient's POINT, from its own position (raht_marshal.hpp does the same)
      const int32_t* q = b.xyz + 3 * ((size_t)sl.base + b.indexes[g]);
      marshal_region_offset(sl.regions, q[0], q[1], q[2], o0, o1);
    }
    lift_quantise_point<C>(
      encoder, sl.layer_qp[sl.range_qlayer[r]], o0, o1, sl.max_qp, sl.fixed_point_qp_offset, lcpc, b.qw[g], lut,
      &b.a[(size_t)g * C], &b.coeffs[(size_t)g * C]);
  }
}

__global__ __launch_bounds__(kLiftBatchBlock) void
lift_batch_writeback_kernel(LiftBatch b)
{
  if (lift_batch_refused(b))
    return;
  for (int g = blockIdx.x * kLiftBatchBlock + threadIdx.x; g < b.n; g += gridDim.x * kLiftBatchBlock) {
    const int s = find_slice(b.pt_off, b.num_slices, g);
    const LiftSlice& sl = b.slice[s];
    const size_t base = (size_t)sl.base;
    lift_writeback_point(
      b.c, ((int64_t)1 << sl.bitdepth) - 1, b.a + base * b.c, b.indexes + base, b.attrs + base * b.c, (int)(g - base));
  }
}

// ---- the launch sequence ---------------------------------------------------------------------------------------
// span(name): an object that lives as long as the ONE launch it names (the library's per-kernel timer, so the
// number of spans is the number of launches).  b: lift_batch_view plus the caller's buffers; d_meta: the uploaded
// plan.meta.  Enqueues only.
template<int C, class Span>
inline hipError_t
lift_batch_launch_c(
  hipStream_t st, const LiftBatch& b, const LiftBatchPlan& plan, const char* d_meta, bool encoder, Span&& span)
{
  const dim3 block(kLiftBatchBlock);
  auto grid = [](int64_t items) { return dim3(marshal_grid(items)); };
  {
    auto t = span("lift_batch_check");
    hipLaunchKernelGGL(lift_batch_check_kernel, grid(b.n), block, 0, st, b);
  }
  {
    auto t = span("lift_batch_init");
    hipLaunchKernelGGL(lift_batch_init_kernel, grid(b.n), block, 0, st, b, encoder ? 1 : 0);
  }
  if (plan.any_scalable) {
    auto t = span("lift_batch_quant_weights_scalable");
    hipLaunchKernelGGL(lift_batch_quant_weights_scalable_kernel, grid(b.n), block, 0, st, b);
  }
  if (!plan.all_scalable)
    for (int k = 0; k < plan.steps; k++) {
      const LiftStep fine = lift_batch_step(plan, d_meta, 0, 0, k);
      if (!fine.total)
        continue;
      auto t = span("lift_batch_quant_weights");
      hipLaunchKernelGGL(lift_batch_quant_weights_kernel, grid(fine.total), block, 0, st, b, fine);
    }
  if (encoder) {
    for (int k = 0; k < plan.steps; k++) {
      const LiftStep fine = lift_batch_step(plan, d_meta, 0, 0, k), coarse = lift_batch_step(plan, d_meta, 0, 1, k);
      if (!fine.total)
        continue;
      {
        auto t = span("lift_batch_predict");
        hipLaunchKernelGGL((lift_batch_predict_kernel<C>), grid(fine.total), block, 0, st, b, fine, 1);
      }
      {
        auto t = span("lift_batch_update_scatter");
        hipLaunchKernelGGL((lift_batch_update_scatter_kernel<C>), grid(fine.total), block, 0, st, b, fine);
      }
      {
        auto t = span("lift_batch_update_apply");
        hipLaunchKernelGGL((lift_batch_update_apply_kernel<C>), grid(coarse.total), block, 0, st, b, coarse, 1);
      }
    }
    if (C == 3 && plan.any_lcp) {
      {
        auto t = span("lift_batch_lcp_sums");
        hipLaunchKernelGGL(lift_batch_lcp_sums_kernel, grid(b.n), block, 0, st, b);
      }
      {
        auto t = span("lift_batch_lcp_resolve");
        hipLaunchKernelGGL(lift_batch_lcp_resolve_kernel, grid(b.num_slices), block, 0, st, b);
      }
    }
  }
  {
    auto t = span("lift_batch_quantise");
    hipLaunchKernelGGL((lift_batch_quantise_kernel<C>), grid(b.n), block, 0, st, b, encoder ? 1 : 0);
  }
  for (int k = 0; k < plan.steps; k++) {
    const LiftStep fine = lift_batch_step(plan, d_meta, 1, 0, k), coarse = lift_batch_step(plan, d_meta, 1, 1, k);
    if (!fine.total)
      continue;
    {
      auto t = span("lift_batch_update_scatter");
      hipLaunchKernelGGL((lift_batch_update_scatter_kernel<C>), grid(fine.total), block, 0, st, b, fine);
    }
    {
      auto t = span("lift_batch_update_apply");
      hipLaunchKernelGGL((lift_batch_update_apply_kernel<C>), grid(coarse.total), block, 0, st, b, coarse, 0);
    }
    {
      auto t = span("lift_batch_predict");
      hipLaunchKernelGGL((lift_batch_predict_kernel<C>), grid(fine.total), block, 0, st, b, fine, 0);
    }
  }
  {
    auto t = span("lift_batch_writeback");
    hipLaunchKernelGGL(lift_batch_writeback_kernel, grid(b.n), block, 0, st, b);
  }
  return hipGetLastError();
}

template<class Span>
inline hipError_t
lift_batch_launch(
  hipStream_t st, const LiftBatch& b, const LiftBatchPlan& plan, const char* d_meta, bool encoder, Span&& span)
{
  switch (b.c) {
  case 1: return lift_batch_launch_c<1>(st, b, plan, d_meta, encoder, span);
  case 2: return lift_batch_launch_c<2>(st, b, plan, d_meta, encoder, span);
  default: return lift_batch_launch_c<3>(st, b, plan, d_meta, encoder, span);
  }
}

}  // namespace gpcc
