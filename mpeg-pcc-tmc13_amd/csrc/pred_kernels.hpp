// pred_kernels.hpp -- the predicting transform on gfx950, given the LoD
// structure (predictors in coding order).
//
// The reference walks the predictors one by one
// (encode/decode{Colors,Reflectances}Pred, tmc3/AttributeEncoder.cpp:749-853,
// 1075-1210, tmc3/AttributeDecoder.cpp:328-523): a point is predicted from the
// RECONSTRUCTED values of up to three neighbours that precede it in coding
// order -- of coarser levels of detail and, unless
// intra_lod_prediction_skip_layers excludes it, of its own.  That is a
// dependency DAG over the points, not a level-synchronous structure, so:
//   * quantisation weights (computeQuantizationWeights, PCCTMC3Common.h:
//     895-922): the DAG walked from the last predictor to the first; a point
//     is final once every later point that references it has added its share
//     (in-degree counted up front, 64-bit atomic adds commute);
//   * reconstruction: the DAG walked forward; wavefronts claim 64 consecutive
//     predictors in coding order (a ticket, so everything a claim waits for is
//     owned by a wavefront that is already running), a lane publishes its
//     reconstruction as ONE write-through granule {values, tag} that doubles
//     as the done flag, neighbours inside the claim are handed over lane to
//     lane (ds_bpermute) without touching memory.
// The decoder is complete (prediction modes hidden in the coefficient
// parities, inter-component prediction, QP layers, region offsets).  The
// encoder's choice among direct predictors reads a running rate model that
// every EARLIER point has updated (PCCResidualsEncoder::resStatUpdate*,
// AttributeEncoder.cpp:136-159): that is one serial scan over the slice with a
// double-precision log2 per candidate, so the device encoder covers
// max_num_direct_predictors == 0 and returns GPCC_ERR_UNSUPPORTED otherwise
// (the caller keeps the reference's loop).
#pragma once

#include <algorithm>
#include <vector>

#include "lift_kernels.hpp"

namespace gpcc {

struct PredCtx {
  int32_t n, c;
  int32_t num_lods;
  int32_t npl[GPCC_MAX_LODS];
  // the reference's running counters per range between distinct LoD
  // boundaries (replayed on the host): quantLayer, the `lod` of the coding
  // loop (icpCoeffs[lod]) and the `lod` of the coefficient estimation
  int32_t num_ranges;
  int32_t range_start[kMaxLodRanges];
  int32_t range_qlayer[kMaxLodRanges];
  int32_t range_lod[kMaxLodRanges];
  int32_t range_est[kMaxLodRanges];
  int32_t est_resolved;  // estimation: LoDs [0, est_resolved) reach their boundary
  int32_t max_levels;
  int32_t bitdepth;
  int32_t num_qp_layers;
  int32_t layer_qp[GPCC_MAX_QP_LAYERS][2];
  int32_t max_qp;
  int32_t max_direct, avg_disabled, threshold, icp_enabled;
  int32_t qnw[3];
  const int32_t* nc;
  const int32_t* ni;
  const int32_t* nw;
  const int32_t* indexes;
  const int32_t* qp_off;
  int32_t* attrs;   // [n][c] point order
  int32_t* values;  // [n][c] coding order
  int8_t* icp;      // [GPCC_MAX_LODS][3]
  int32_t* indeg;   // [n]
  int32_t* recv;    // [n]
  unsigned long long* acc;  // [n]
  unsigned long long* qw;   // [n]
  // [n][4] {r, g, b, tag}: one 16-byte granule per predictor.  HARDWARE ASSUMPTION
  // (as for the granules of lod_kernels.hpp and raht_subnode.hpp): a naturally
  // aligned 16-byte sc1 store / load is observed whole -- a reader that sees the tag
  // sees the three values of the same store (MI355X_MICROARCH.md, hand-off section);
  // there is no release / acquire pair around it.
  uint32_t* rec;
  uint32_t tag;       // tag of this pass's granules (the encoder's mode decision iterates passes)
  // encoder with direct predictors (pred_rate_* below)
  const int32_t* src;       // [n][c] source attributes, point order (attrs then only takes the reconstruction)
  const int32_t* rm;        // [n][6] rate model before every predictor: probResGt0[3], probResGt1[3]
  const double* log2tab;    // [2^20 + 1] log2 of every integer, computed by the HOST's libm
  int32_t* ticket;  // [2]
  int32_t* wide;    // set by pred_indegree_kernel: an in-degree >= 2^20
  int32_t packed_ok;  // quant_neigh_weight >= 0 and their sum < 256
  int32_t* error;
  unsigned long long* icp_sums;  // [GPCC_MAX_LODS][18]: 8 weights x {k=1,2}, orig x {1,2}
  // attribute inter prediction (pred_dag_kernel<.., true>, one component): a neighbour index
  // >= n names entry (index - n) of the reference frame; its value is always there
  // (predictReflectance PCCTMC3Common.h:555-585, predModeEligibleRefl
  // AttributeCommon.cpp:176-210, decidePredModeRefl AttributeEncoder.cpp:663-717 all read the
  // frame's reflectance for such a neighbour).  indeg / recv / acc / qw have n_frame spare
  // entries behind the n predictors: the shares such a neighbour would be skipped for
  // (computeQuantizationWeights :913-914) land there.
  const int32_t* frame_attr;  // [n_frame]
};

// The reference's running counters step when the predictor index meets
// numPointsInLod[counter] (one step per index, so a repeated boundary
// stalls them): quantLayer and `lod` of the coding loops
// (AttributeEncoder.cpp:1108-1121, AttributeDecoder.cpp:476-501) before the
// index is processed, `lod` of computeInterComponentPredictionCoeffs
// (:1033-1056) after index npl[lod] - 1.  Replayed over the distinct
// boundaries.
inline void
pred_fill_ranges(PredCtx& cx, const int32_t* npl, int num_lods, int num_qp_layers, int n)
{
  int ql = 0, lod = 0, est = 0, nr = 1;
  std::vector<int> bs(npl, npl + num_lods);
  std::sort(bs.begin(), bs.end());
  bs.erase(std::unique(bs.begin(), bs.end()), bs.end());
  cx.range_start[0] = 0;
  for (int b : bs) {
    if (b >= n)
      break;
    if (ql < num_lods && b == npl[ql])
      ql = std::min(num_qp_layers - 1, ql + 1);
    if (lod < num_lods && b == npl[lod])
      lod++;
    if (b > 0 && est < num_lods && b == npl[est])
      est++;
    if (b > 0) {
      cx.range_start[nr] = b;
      nr++;
    }
    cx.range_qlayer[nr - 1] = ql;
    cx.range_lod[nr - 1] = std::min(lod, GPCC_MAX_LODS - 1);
    cx.range_est[nr - 1] = std::min(est, GPCC_MAX_LODS - 1);
  }
  cx.num_ranges = nr;
  cx.est_resolved = est < num_lods && npl[est] == n ? est + 1 : est;
}

__device__ __forceinline__ int
pred_range_of(const PredCtx& cx, int i)
{
  int r = 0;
  for (int k = 1; k < cx.num_ranges; k++)
    r += i >= cx.range_start[k];
  return r;
}

constexpr int kPredCountShift = 44;  // packed share word: (count << 44) | sum

__global__ __launch_bounds__(256) void
pred_indegree_kernel(PredCtx cx)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cx.n; i += gridDim.x * blockDim.x) {
    const int cnt = cx.nc[i];
    for (int j = 0; j < cnt; j++)
      if (atomicAdd(&cx.indeg[cx.ni[3 * (size_t)i + j]], 1) + 1 >= (1 << (64 - kPredCountShift)))
        atomicExch(cx.wide, 1);  // a count that does not fit the packed word
  }
}

// computeQuantizationWeights: predictors from the last to the first.  A
// wavefront claims 64 consecutive predictors (descending).  A point's shares
// and the number of referrers that have delivered travel in ONE 64-bit word,
// (count << 44) | sum, so a delivery is a single fire-and-forget atomic add
// and the word a consumer polls is complete when its count is (no fence, no
// wait on the producer's side).  44 bits hold every sum when the three
// quant_neigh_weights are non-negative and add up to < 256: the shares a point
// hands on are then less than its own weight, so all weights together stay
// below 2^16 n.  Shares for a point of the same claim go through the
// wavefront's LDS slots, the rest through memory; a lane polls memory only
// until the referrers OUTSIDE its claim have delivered (the in-degree minus the
// referrers counted inside the claim), after that the claim iterates on LDS
// alone.  In-degrees of 2^20 or more, or other weights: kWide, separate sum and
// count words with release / acquire ordering.
template<bool kWide>
__device__ __forceinline__ void
pred_quant_weights_body(const PredCtx& cx)
{
  __shared__ unsigned long long lacc[4][64];
  __shared__ int lrecv[4][64];
  __shared__ int lneed[4][64];
  constexpr unsigned long long kOne = 1ull << kPredCountShift, kSumMask = kOne - 1;
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  for (;;) {
    int tk = 0;
    if (lane == 0)
      tk = atomicAdd(&cx.ticket[0], 1);
    tk = __shfl(tk, 0);
    const int64_t base = (int64_t)tk * 64;
    if (base >= cx.n)
      break;
    if (__hip_atomic_load(cx.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      break;
    const int i = cx.n - 1 - (int)(base + lane);
    bool pending = i >= 0;
    int cnt = 0, need = 0;
    int nb[3] = {0, 0, 0};
    int tl[3] = {64, 64, 64};  // lane of a neighbour inside the claim (> own lane), 64 = outside
    __hip_atomic_store(&lacc[wv][lane], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_store(&lrecv[wv][lane], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_store(&lneed[wv][lane], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (pending) {
      cnt = cx.nc[i];
      need = cx.indeg[i];
      for (int j = 0; j < 3; j++)
        if (j < cnt) {
          nb[j] = cx.ni[3 * (size_t)i + j];
          const int64_t t = (int64_t)(cx.n - 1 - nb[j]) - base;
          // (t < 0: a neighbour in the reference frame, addressed behind the n predictors --
          // its share goes the memory way, into an entry nobody reads)
          tl[j] = t >= 0 && t < 64 ? (int)t : 64;
        }
    }
    // (the wavefront is in lock step here: every slot is cleared before a lane counts into
    // another lane's, every count is in before a lane reads its own -- said to the compiler,
    // and to the CPU emulator of tests/emu, with wave barriers; no instruction on the device)
    __builtin_amdgcn_wave_barrier();
    for (int j = 0; j < 3; j++)
      if (tl[j] < 64)
        __hip_atomic_fetch_add(&lneed[wv][tl[j]], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __builtin_amdgcn_wave_barrier();
    const int need_l = __hip_atomic_load(&lneed[wv][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const int need_g = need - need_l;
    bool gdone = !pending || need_g == 0;
    unsigned long long gsum = 0;
    unsigned spins = 0;
    while (__any(pending)) {
      if (pending && !gdone) {
        if (kWide) {
          gdone = __hip_atomic_load(&cx.recv[i], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == need_g;
          if (gdone)
            gsum = __hip_atomic_load(&cx.acc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          const unsigned long long v =
            __hip_atomic_load(&cx.acc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          gdone = (int)(v >> kPredCountShift) == need_g;
          gsum = v & kSumMask;
        }
      }
      bool ready = false;
      unsigned long long lsum = 0;
      if (pending && gdone) {
        if (kWide) {
          ready = __hip_atomic_load(&lrecv[wv][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == need_l;
          if (ready)
            lsum = __hip_atomic_load(&lacc[wv][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
          const unsigned long long v =
            __hip_atomic_load(&lacc[wv][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          ready = (int)(v >> kPredCountShift) == need_l;
          lsum = v & kSumMask;
        }
      }
      if (ready) {
        const uint64_t w = 256 + gsum + lsum;
        cx.qw[i] = w;
        for (int j = 0; j < 3; j++) {
          if (j >= cnt)
            continue;
          // int32 * uint64 -> uint64 in the reference: the unsigned overload of
          // divExp2RoundHalfInf (PCCMath.h:678-685), modular product, logical shift
          unsigned long long share = ((unsigned long long)(long long)cx.qnw[j] * w + 128ull) >> 8;
          if (!kWide)
            share += kOne;
          if (tl[j] < 64)
            __hip_atomic_fetch_add(&lacc[wv][tl[j]], share, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          else
            atomicAdd(&cx.acc[nb[j]], share);
        }
        if (kWide)
          for (int j = 0; j < 3; j++) {
            if (j >= cnt)
              continue;
            if (tl[j] < 64)
              __hip_atomic_fetch_add(&lrecv[wv][tl[j]], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            else
              __hip_atomic_fetch_add(&cx.recv[nb[j]], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          }
        pending = false;
      }
      if (++spins > (1u << 24)) {
        if (lane == 0)
          atomicExch(cx.error, 1);
        break;
      }
    }
  }
}

__global__ __launch_bounds__(256) void
pred_quant_weights_kernel(PredCtx cx)
{
  // uniform: the flag was written by the kernel before this one
  if (cx.packed_ok && !*cx.wide)
    pred_quant_weights_body<false>(cx);
  else
    pred_quant_weights_body<true>(cx);
}

// ---- computeInterComponentPredictionCoeffs (encoder) -----------------------
__global__ __launch_bounds__(256) void
pred_icp_sums_kernel(PredCtx cx)
{
  __shared__ unsigned long long s[GPCC_MAX_LODS][18];
  for (int t = threadIdx.x; t < GPCC_MAX_LODS * 18; t += blockDim.x)
    (&s[0][0])[t] = 0;
  __syncthreads();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cx.n; i += gridDim.x * blockDim.x) {
    const int lod = cx.range_est[pred_range_of(cx, i)];
    int32_t resid[3];
    const int32_t* me = &cx.attrs[3 * (size_t)cx.indexes[i]];
    const bool has = cx.nc[i] >= 1;
    const int32_t* nbp = has ? &cx.attrs[3 * (size_t)cx.indexes[cx.ni[3 * (size_t)i]]] : me;
    for (int k = 0; k < 3; k++)
      resid[k] = me[k] - (has ? nbp[k] : 0);
    for (int w = 0; w < 8; w++)
      for (int k = 1; k < 3; k++)
        atomicAdd(
          &s[lod][2 * w + k - 1],
          (unsigned long long)abs(resid[k] - (((w + 1) * resid[0] + 2) >> 2)));
    for (int k = 1; k < 3; k++)
      atomicAdd(&s[lod][16 + k - 1], (unsigned long long)abs(resid[k]));
  }
  __syncthreads();
  for (int t = threadIdx.x; t < GPCC_MAX_LODS * 18; t += blockDim.x)
    if ((&s[0][0])[t])
      atomicAdd(&cx.icp_sums[t], (&s[0][0])[t]);
}

__global__ void
pred_icp_resolve_kernel(PredCtx cx)
{
  const int lod = threadIdx.x;
  if (lod >= GPCC_MAX_LODS)
    return;
  int8_t out[3] = {0, 0, 0};
  if (lod < cx.est_resolved && lod < cx.max_levels) {
    const unsigned long long* s = &cx.icp_sums[18 * lod];
    for (int k = 1; k < 3; k++) {
      int best = 0;
      for (int w = 1; w < 8; w++)
        if (s[2 * w + k - 1] < s[2 * best + k - 1])
          best = w;
      out[k] = s[2 * best + k - 1] > s[16 + k - 1] ? 0 : (int8_t)(1 + best);
    }
  }
  for (int k = 0; k < 3; k++)
    cx.icp[3 * lod + k] = out[k];
}

// ---- the encoder's rate model (PCCResidualsEncoder, AttributeEncoder.cpp:81-222) -------
// The choice among direct predictors (decidePredModeRefl :663-745, decidePredModeColor
// :896-985) scores every candidate with an estimate of its coded size from two running
// probabilities per component, updated after every predictor in coding order
// (resStatUpdate :137-165): the one loop-carried state of the encoder that is not a
// neighbour value.  Here the state BEFORE every predictor is an input of the DAG pass
// (cx.rm), recomputed from the pass's values by pred_rate_scan_kernel, and the two are
// iterated: a pass whose values equal the previous pass's has used exactly the states the
// sequential coder would have had (induction over the coding order), so the fixed point IS
// the reference's result.  Each pass is exact up to its first wrong decision, and a wrong
// state decays by 1/64 per predictor, so a handful of passes settle a slice.
// The estimate takes log2 of integers below 2^20: the table is filled by the host's libm
// (the reference's own log2), and every term is added in the reference's order without
// contraction: bitsPtColor (:163-199) carries ONE running sum through the three components,
// so pred_rate_component takes that sum and returns it.  (Double addition is not
// associative: with a sum per component, added afterwards, two direct predictors of equal
// distortion and nearly equal rate -- modes that only swap a parity bit between the second
// and the third component -- were ranked the other way round from 12 bits upwards.)
// Identical doubles, identical decisions.
constexpr int kRateScale = 1 << 20, kRateWindowLog2 = 6;

__device__ __forceinline__ double
pred_log2i(const PredCtx& cx, int64_t v)
{
  return v >= 0 && v <= kRateScale ? cx.log2tab[v] : log2((double)v);
}

__device__ __forceinline__ double
pred_rate_component(const PredCtx& cx, const int32_t* rm, int k, int32_t value, double bits)
{
#pragma clang fp contract(off)
  const int l2 = 20;  // ilog2(scaleRes)
  bits += value ? l2 - pred_log2i(cx, rm[k]) : l2 - pred_log2i(cx, kRateScale - rm[k]);
  const int mag = value < 0 ? -value : value;
  if (mag) {
    bits += mag > 1 ? l2 - pred_log2i(cx, rm[3 + k]) : l2 - pred_log2i(cx, kRateScale - rm[3 + k]);
    bits += 1;
    if (mag > 1)
      bits += 2.0 * pred_log2i(cx, (int64_t)mag - 1) + 1.0;
  }
  return bits;
}

// bitsPtRefl (:203-222)
__device__ __forceinline__ double
pred_rate_refl(const PredCtx& cx, const int32_t* rm, int avail, int32_t value, int mode)
{
#pragma clang fp contract(off)
  const int a = value < 0 ? -value : value;
  if (avail == 4) {
    value = (a << 2) + mode;
  } else if (avail == 3) {
    int v = a;
    if (mode > 0)
      v = (v << 1) + (mode - 1);
    value = (v << 1) + (mode > 0);
  } else if (avail == 2) {
    value = (a << 1) + (mode & 1);
  }
  double bits = 0;
  bits = pred_rate_component(cx, rm, 0, value, bits);
  return bits;
}

// bitsPtColor (:168-199)
__device__ __forceinline__ double
pred_rate_colour(const PredCtx& cx, const int32_t* rm, int avail, const int64_t r[3], int mode)
{
#pragma clang fp contract(off)
  int32_t v[3] = {(int32_t)r[0], (int32_t)r[1], (int32_t)r[2]};
  const int a1 = v[1] < 0 ? -v[1] : v[1], a2 = v[2] < 0 ? -v[2] : v[2];
  if (avail == 4) {
    v[1] = 2 * a1 + (mode >> 1);
    v[2] = 2 * a2 + (mode & 1);
  } else if (avail == 3) {
    v[1] = 2 * a1 + (mode > 0);
    if (mode > 0)
      v[2] = 2 * a2 + (mode - 1);
  } else if (avail == 2) {
    v[1] = 2 * a1 + (mode & 1);
  }
  double bits = 0;
  for (int k = 0; k < 3; k++)
    bits = pred_rate_component(cx, rm, k, v[k], bits);
  return bits;
}

__device__ __forceinline__ int64_t
pred_half_up8(int64_t x)
{
  return (x + 128) >> 8;
}

// computeColorResiduals (:858-890)
__device__ __forceinline__ void
pred_colour_residuals(
  bool icp_on, const int32_t col[3], const int64_t pred[3], const int8_t icp[3], const Quantizer q[2],
  int64_t r[3])
{
  r[0] = quantize(q[0], ((int64_t)col[0] - pred[0]) << 8);
  const int64_t residual0 = pred_half_up8(mul_i64_u32(r[0], q[0].step));
  for (int k = 1; k < 3; k++) {
    int64_t err = (int64_t)col[k] - pred[k];
    if (icp_on)
      err -= ((int64_t)icp[k] * residual0 + 2) >> 2;
    r[k] = quantize(q[1], err << 8);
  }
}

// computeColorDistortions (:792-823)
__device__ __forceinline__ int
pred_colour_distortion(int64_t clip_max, const int32_t col[3], const int64_t pred[3], const Quantizer q[2])
{
  int d = 0;
  for (int k = 0; k < 3; k++) {
    const Quantizer qq = q[k ? 1 : 0];
    const int64_t rq = quantize(qq, ((int64_t)col[k] - pred[k]) << 8);
    int64_t rec = pred[k] + pred_half_up8(mul_i64_u32(rq, qq.step));
    rec = rec < 0 ? 0 : (rec > clip_max ? clip_max : rec);
    const int e = (int)((int64_t)col[k] - (int64_t)(uint16_t)rec);
    d += e < 0 ? -e : e;
  }
  return d;
}

__device__ __forceinline__ int
pred_rate_step(int x, bool up)
{
  return up ? x + ((kRateScale - x) >> kRateWindowLog2) : x - (x >> kRateWindowLog2);
}

__global__ __launch_bounds__(256) void
pred_rate_init_kernel(int32_t* rm, int n)
{
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n * 6; i += (size_t)gridDim.x * blockDim.x)
    rm[i] = kRateScale >> 1;
}

// The states before every predictor from the values of a pass.  probResGt0 steps at
// every predictor (up when the value is non-zero); probResGt1 only at the non-zero
// values (up when the magnitude exceeds 1), so its recurrence runs over the COMPACTED
// list of those events (flags -> ranks by a scan -> events) and a predictor reads the
// state in front of the first event at or behind it.  A recurrence is cut into chunks of
// kRateChunk events, one thread each: a thread does not know the state at its chunk's
// start, so it runs the recurrence from the two EXTREME reachable states (63 and
// 2^20 - 63: the fixed points of the two steps) over a warm-up window in front of the
// chunk -- every step is monotone in the state, the true state lies between the two
// runs, and where they have met it is known exactly.  A warm-up that has not met is
// quadrupled (at worst back to the first event, where the state is the initial one).
constexpr int kRateChunk = 256;
constexpr int kRateMin = 63, kRateMax = kRateScale - 63;

// rank[i + 1] = (value of component k at predictor i is non-zero); rank[0] = 0
__global__ __launch_bounds__(256) void
pred_rate_flags_kernel(const int32_t* __restrict__ values, int n, int c, int k, int32_t* __restrict__ rank)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    rank[i + 1] = values[(size_t)i * c + k] != 0;
    if (i == 0)
      rank[0] = 0;
  }
}

// after the inclusive scan rank[i] = non-zero values before predictor i
__global__ __launch_bounds__(256) void
pred_rate_events_kernel(
  const int32_t* __restrict__ values, int n, int c, int k, const int32_t* __restrict__ rank,
  uint8_t* __restrict__ ev)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int32_t v = values[(size_t)i * c + k];
    if (v)
      ev[rank[i]] = (v < 0 ? -v : v) > 1;
  }
}

// One recurrence over `m` events (up[e] from the values for probResGt0: stride c,
// non-zero test; from the event bytes for probResGt1); state[e] = the state in front of
// event e, state[m] behind the last (m is read from *m_ptr when given).
// One wavefront per 64 chunks.  The wavefront first packs the flags of ITS events -- the 1024 of the first
// chunk's warm-up and the 64 x 256 of the chunks -- into bit words in LDS with coalesced loads and ballots; the
// threads then run their recurrences on the words, stage the states in LDS and the wavefront writes them out
// 64 consecutive events per store.  (Until round 5 a thread read its 1 280 flags itself, sixteen loads at a
// time, every lane in a different cache line, and stored its 256 states the same way: 1.07 ms per call for
// 1 M events, 8.6 ms of a predicting encode.)  A warm-up that has not met after 1024 events is continued from
// global memory with quadrupled windows, as before.
constexpr int kRateWarm = 1024;
constexpr int kRateHalf = kRateChunk / 2;

__global__ __launch_bounds__(64) void
pred_rate_scan_kernel(
  const int32_t* __restrict__ values, int stride, const uint8_t* __restrict__ ev, int m_max,
  const int32_t* __restrict__ m_ptr, int32_t* __restrict__ state, int state_stride, int write_final)
{
  __shared__ unsigned long long wbits[(kRateWarm + 64 * kRateChunk) / 64];
  __shared__ int32_t stage[64 * (kRateHalf + 1)];
  const int m = m_ptr ? *m_ptr : m_max;
  const int lane = threadIdx.x;
  const long long wave_start = (long long)blockIdx.x * 64 * kRateChunk;
  if (wave_start > m || (wave_start == m && m > 0))
    return;  // (no chunk of this wavefront holds an event, and state[m] is another wavefront's)
  auto up = [&](long long e) -> bool { return values ? values[(size_t)e * stride] != 0 : ev[e] != 0; };
  // ---- the flags of events [base, last) as bit words: bit (e - base) ----
  const long long base = wave_start - kRateWarm;
  const long long last = wave_start + 64 * kRateChunk < m ? wave_start + 64 * kRateChunk : m;
  const int nwords = (int)((last - base + 63) >> 6);
  // (sixteen words per batch: the sixteen loads are unconditional -- the index clamped into the range, the range
  // test applied to the loaded flag -- so that they are in flight together; behind a test per event every load
  // waited for its predecessor's ballot: 272 round trips to memory per wavefront)
  if (last > 0) {
    auto pack = [&](auto flag_at) {
      for (int w0 = 0; w0 < nwords; w0 += 16) {
        int f[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
          const long long e = base + (long long)(w0 + j) * 64 + lane;
          const long long ec = e < 0 ? 0 : (e >= last ? last - 1 : e);
          f[j] = flag_at(ec);
        }
#pragma unroll
        for (int j = 0; j < 16; j++) {
          const long long e = base + (long long)(w0 + j) * 64 + lane;
          const unsigned long long b = __ballot((f[j] != 0) & (e >= 0) & (e < last));
          if (lane == 0 && w0 + j < nwords)
            wbits[w0 + j] = b;
        }
      }
    };
    if (values)
      pack([&](long long e) -> int { return values[(size_t)e * stride]; });
    else
      pack([&](long long e) -> int { return ev[e]; });
  } else {
    for (int w = lane; w < nwords; w += 64)
      wbits[w] = 0;
  }
  __syncthreads();
  const long long start = wave_start + (long long)lane * kRateChunk;
  const bool active = !(start > m || (start == m && m > 0));
  const int end = !active ? 0 : (start + kRateChunk < m ? (int)(start + kRateChunk) : m);
  int x = kRateScale >> 1;
  if (active && start > 0) {
    // warm-up over [b, start): b = start - 1024 or 0
    const int b = start - kRateWarm > 0 ? (int)(start - kRateWarm) : 0;
    int lo = b == 0 ? kRateScale >> 1 : kRateMin, hi = b == 0 ? kRateScale >> 1 : kRateMax;
    for (long long e = b; e < start;) {
      const int bit = (int)(e - base);
      const int b1 = start - (e - (bit & 63)) < 64 ? (int)(start - (e - (bit & 63))) : 64;
      unsigned long long w = wbits[bit >> 6] >> (bit & 63);
      for (int q = bit & 63; q < b1; q++, w >>= 1) {
        lo = pred_rate_step(lo, w & 1);
        hi = pred_rate_step(hi, w & 1);
      }
      e += b1 - (bit & 63);
    }
    x = lo;
    if (lo != hi) {
      for (long long w = 4 * kRateWarm;; w *= 4) {
        const int bb = start - w > 0 ? (int)(start - w) : 0;
        lo = bb == 0 ? kRateScale >> 1 : kRateMin;
        hi = bb == 0 ? kRateScale >> 1 : kRateMax;
        for (int e = bb; e < (int)start; e++) {
          const bool u = up(e);
          lo = pred_rate_step(lo, u);
          hi = pred_rate_step(hi, u);
        }
        x = lo;
        if (lo == hi)
          break;
      }
    }
  }
  // ---- the chunk, in two halves: states staged in LDS (row of a lane: kRateHalf + 1 words, so that the lanes'
  // stores fall into different banks), written out 64 consecutive events at a time ----
  for (int h = 0; h < 2; h++) {
    const long long h0 = start + (long long)h * kRateHalf;
    if (active) {
      for (int q = 0; q < kRateHalf; q += 64) {
        const long long e0 = h0 + q;
        if (e0 >= end)
          break;
        const int bit = (int)(e0 - base);  // (a multiple of 64)
        unsigned long long w = wbits[bit >> 6];
        const int cnt = end - e0 < 64 ? (int)(end - e0) : 64;
        for (int t = 0; t < cnt; t++, w >>= 1) {
          stage[lane * (kRateHalf + 1) + q + t] = x;
          x = pred_rate_step(x, w & 1);
        }
      }
    }
    __syncthreads();
    for (int i = 0; i < kRateHalf; i++) {
      const int idx = i * 64 + lane;
      const int c = idx / kRateHalf, t = idx % kRateHalf;
      const long long e = wave_start + (long long)c * kRateChunk + (long long)h * kRateHalf + t;
      if (e < m)
        state[(size_t)e * state_stride] = stage[c * (kRateHalf + 1) + t];
    }
    __syncthreads();
  }
  if (active && write_final && end == m)
    state[(size_t)m * state_stride] = x;
}

// probResGt1 of every predictor: the state in front of the first event at or behind it
__global__ __launch_bounds__(256) void
pred_rate_gather_kernel(
  const int32_t* __restrict__ rank, const int32_t* __restrict__ evstate, int n, int k, int32_t* __restrict__ rm)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    rm[(size_t)i * 6 + 3 + k] = evstate[rank[i]];
}

// did this pass change a value?  (and keep the values for the next comparison)
__global__ __launch_bounds__(256) void
pred_values_diff_kernel(const int32_t* __restrict__ values, int32_t* __restrict__ prev, size_t count, int32_t* flag)
{
  bool diff = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const int32_t v = values[i];
    diff |= v != prev[i];
    prev[i] = v;
  }
  if (__any(diff) && (threadIdx.x & 63) == 0)
    atomicOr(flag, 1);
}

// One predictor, from its neighbours' reconstructions to its coded values and its own
// reconstruction: eligibility for direct prediction, the mode (decoder: unfolded from the value
// parities; encoder: decided with the rate model `rm` -- the six words in front of THIS predictor),
// prediction, residual, reconstruction and, in the encoder, the mode folded into the values.
// The one statement of the per-predictor step: pred_dag_kernel runs it for a lane of a claim,
// pred_walk_kernel for the predictor its walk stands at.
template<int C, bool ENC>
__device__ __forceinline__ void
pred_point(
  const PredCtx& cx, const int32_t* rm, int cnt, const int32_t (&nbv)[3][C], const int32_t (&nwt)[3],
  const int32_t (&col)[3], const Quantizer (&q)[2], const int64_t (&wgt)[2], const int8_t (&icpc)[3], int maxcand,
  int64_t clip_max, int32_t (&val)[3], int32_t (&myrec)[C])
{
  // predModeEligibleColor / ...Refl
  bool elig = false;
  if (cnt > 1 && cx.max_direct) {
    int32_t best = 0;
    for (int k = 0; k < C; k++) {
      int32_t lo = nbv[0][k], hi = nbv[0][k];
      for (int j = 1; j < 3; j++)
        if (j < cnt) {
          lo = min(lo, nbv[j][k]);
          hi = max(hi, nbv[j][k]);
        }
      best = k == 0 ? hi - lo : max(best, hi - lo);
    }
    elig = best >= cx.threshold;
  }
  int mode = 0;
  if (!ENC && elig) {
    if (C == 1) {
      // decodePredModeRefl
      int a = abs(val[0]);
      const int sg = val[0] < 0 ? -1 : 1;
      if (maxcand == 4) {
        mode = a & 3;
        a >>= 2;
      } else if (maxcand == 3) {
        mode = a & 1;
        a >>= 1;
        if (mode > 0) {
          mode += a & 1;
          a >>= 1;
        }
      } else if (maxcand == 2) {
        mode = a & 1;
        a >>= 1;
      }
      val[0] = sg * a;
    } else {
      // decodePredModeColor
      const int s1 = val[1 % C] < 0 ? -1 : 1, s2 = val[2 % C] < 0 ? -1 : 1;
      const int a1 = abs(val[1 % C]), a2 = abs(val[2 % C]);
      if (maxcand == 4) {
        val[1 % C] = s1 * (a1 >> 1);
        val[2 % C] = s2 * (a2 >> 1);
        mode = ((a1 & 1) << 1) + (a2 & 1);
      } else if (maxcand == 3) {
        val[1 % C] = s1 * (a1 >> 1);
        mode = a1 & 1;
        if (a1 & 1) {
          val[2 % C] = s2 * (a2 >> 1);
          mode += a2 & 1;
        }
      } else if (maxcand == 2) {
        val[1 % C] = s1 * (a1 >> 1);
        mode = a1 & 1;
      }
    }
    mode += cx.avg_disabled;
  }
  if (ENC && elig) {
    // decidePredModeRefl / decidePredModeColor with the rate model as it is
    // before this predictor
#pragma clang fp contract(off)
    const int dis = cx.avg_disabled;
    mode = dis;
    int64_t p0[3] = {0, 0, 0};
    if (dis) {
      for (int k = 0; k < C; k++)
        p0[k] = nbv[0][k];
    } else {
      for (int k = 0; k < C; k++) {
        int64_t s = 0;
        for (int j = 0; j < 3; j++)
          if (j < cnt)
            s += (int64_t)(uint32_t)nwt[j] * nbv[j][k];
        p0[k] = (uint16_t)div_exp2_round_half_inf(s, 8);
      }
    }
    if (C == 1) {
      int64_t rq = quantize(q[0], ((int64_t)col[0] - p0[0]) << 8);
      int64_t best = (int64_t)pred_rate_refl(cx, rm, maxcand, (int32_t)rq, mode - dis);
      for (int j = 0; j < 3; j++) {
        if (j < dis || j >= cnt || j >= cx.max_direct)
          continue;
        rq = quantize(q[0], ((int64_t)col[0] - (int64_t)nbv[j][0]) << 8);
        const int64_t score = (int64_t)pred_rate_refl(cx, rm, maxcand, (int32_t)rq, j + !dis);
        if (score < best) {
          best = score;
          mode = j + 1;
        }
      }
    } else {
      int32_t c3[3] = {col[0], col[1 % C], col[2 % C]};
      int64_t r[3];
      pred_colour_residuals(cx.icp_enabled != 0, c3, p0, icpc, q, r);
      int dist = pred_colour_distortion(clip_max, c3, p0, q);
      double rate = pred_rate_colour(cx, rm, maxcand, r, 0);
      double best = dist + rate * 0.14 * (q[0].step >> 8);
      for (int j = 0; j < 3; j++) {
        if (j < dis || j >= cnt || j >= cx.max_direct)
          continue;
        const int64_t np[3] = {nbv[j][0], nbv[j][1 % C], nbv[j][2 % C]};
        pred_colour_residuals(cx.icp_enabled != 0, c3, np, icpc, q, r);
        dist = pred_colour_distortion(clip_max, c3, np, q);
        rate = pred_rate_colour(cx, rm, maxcand, r, j + !dis);
        const double score = dist + rate * 0.14 * (q[0].step >> 8);
        if (score < best) {
          best = score;
          mode = j + 1;
        }
      }
    }
  }
  // PCCPredictor::predictColor / predictReflectance
  int64_t pr[C];
  for (int k = 0; k < C; k++)
    pr[k] = 0;
  if (mode > cnt) {
  } else if (mode > 0) {
    // (the three values first, the choice among VALUES: a choice among the loads becomes one load at a
    // computed address, and the neighbour block then lives in scratch)
    for (int k = 0; k < C; k++) {
      const int32_t v0 = nbv[0][k], v1 = nbv[1][k], v2 = nbv[2][k];
      pr[k] = mode == 1 ? v0 : (mode == 2 ? v1 : v2);
    }
  } else {
    for (int k = 0; k < C; k++) {
      int64_t s = 0;
      for (int j = 0; j < 3; j++)
        if (j < cnt)
          s += (int64_t)(uint32_t)nwt[j] * nbv[j][k];
      pr[k] = (uint16_t)div_exp2_round_half_inf(s, 8);
    }
  }
  int64_t residual0 = 0;
  for (int k = 0; k < C; k++) {
    const Quantizer qq = k ? q[1] : q[0];
    const int64_t weight = k ? wgt[1] : wgt[0];
    const int64_t icpterm = C == 3 ? ((int64_t)icpc[k] * residual0 + 2) >> 2 : 0;
    int64_t rr;
    if (ENC) {
      int64_t residual = col[k] - pr[k];
      int64_t rq = quantize(qq, (residual * weight) << 8);
      rr = ((mul_i64_u32(rq, qq.step) + 128) >> 8) / weight;
      if (C == 3 && cx.icp_enabled && k > 0) {
        residual -= icpterm;
        rq = quantize(qq, (residual * weight) << 8);
        rr = ((mul_i64_u32(rq, qq.step) + 128) >> 8) / weight;
        rr += icpterm;
      }
      val[k] = (int32_t)rq;
      if (k == 0)
        residual0 = rr;
    } else {
      rr = ((mul_i64_u32((int64_t)val[k], qq.step) + 128) >> 8) / weight;
      const int64_t residual = rr;
      rr += icpterm;
      if (!k && cx.icp_enabled)
        residual0 = residual;
    }
    int64_t v = pr[k] + rr;
    v = v < 0 ? 0 : (v > clip_max ? clip_max : v);
    myrec[k] = (int32_t)(uint16_t)v;
  }
  if (ENC && elig) {
    // encodePredModeRefl (:749-772) / encodePredModeColor (:988-1016): the mode
    // travels in the low bits of the coded magnitudes
    const int m = mode - cx.avg_disabled;
    if (C == 1) {
      const int sg = val[0] < 0 ? -1 : 1;
      int a = val[0] < 0 ? -val[0] : val[0];
      if (maxcand == 4) {
        a = (a << 2) + m;
      } else if (maxcand == 3) {
        if (m > 0)
          a = (a << 1) + (m - 1);
        a = (a << 1) + (m > 0);
      } else if (maxcand == 2) {
        a = (a << 1) + m;
      }
      val[0] = sg * a;
    } else {
      const int s1 = val[1 % C] < 0 ? -1 : 1, s2 = val[2 % C] < 0 ? -1 : 1;
      const int a1 = val[1 % C] < 0 ? -val[1 % C] : val[1 % C];
      const int a2 = val[2 % C] < 0 ? -val[2 % C] : val[2 % C];
      if (maxcand == 4) {
        val[1 % C] = s1 * ((a1 << 1) + (m >> 1));
        val[2 % C] = s2 * ((a2 << 1) + (m & 1));
      } else if (maxcand == 3) {
        const int p1 = m ? 1 : 0;
        val[1 % C] = s1 * ((a1 << 1) + p1);
        if (p1)
          val[2 % C] = s2 * ((a2 << 1) + (m - p1));
      } else if (maxcand == 2) {
        val[1 % C] = s1 * ((a1 << 1) + m);
      }
    }
  }
}

// ---- reconstruction: the DAG walked forward --------------------------------
template<int C, bool ENC, bool INTER = false>
__global__ __launch_bounds__(256) void
pred_dag_kernel(PredCtx cx)
{
  GPCC_VGPR_FLOOR_64();
  const int lane = lane_id();
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(
    cx.rec, 0, (int)((size_t)cx.n * 16), 0x00020000);
  const int maxcand = cx.max_direct + !cx.avg_disabled;
  const int64_t clip_max = ((int64_t)1 << cx.bitdepth) - 1;
  for (;;) {
    int tk = 0;
    if (lane == 0)
      tk = atomicAdd(&cx.ticket[1], 1);
    tk = __shfl(tk, 0);
    const int64_t base64 = (int64_t)tk * 64;
    if (base64 >= cx.n)
      break;
    if (__hip_atomic_load(cx.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      break;
    const int base = (int)base64;
    const int i = base + lane;
    const bool live = i < cx.n;
    int cnt = 0, pt = 0;
    int nidx[3] = {0, 0, 0};
    int32_t nwt[3] = {0, 0, 0};
    int32_t val[3] = {0, 0, 0};
    int32_t col[3] = {0, 0, 0};
    int64_t wgt[2] = {1, 1};
    Quantizer q[2] = {make_quantizer(4), make_quantizer(4)};
    int8_t icpc[3] = {0, 0, 0};
    if (live) {
      cnt = cx.nc[i];
      pt = cx.indexes[i];
      for (int j = 0; j < 3; j++) {
        nidx[j] = j < cnt ? cx.ni[3 * (size_t)i + j] : 0;
        nwt[j] = j < cnt ? cx.nw[3 * (size_t)i + j] : 0;
      }
      const int r = pred_range_of(cx, i);
      const int layer = cx.range_qlayer[r];
      const int o0 = cx.qp_off ? cx.qp_off[2 * (size_t)pt] : 0;
      const int o1 = cx.qp_off ? cx.qp_off[2 * (size_t)pt + 1] : 0;
      const int qp0 = clip(cx.layer_qp[layer][0] + o0, 4, cx.max_qp);
      const int qp1 = clip(cx.layer_qp[layer][1] + o1 + qp0, 4, cx.max_qp);
      q[0] = make_quantizer(qp0);
      q[1] = make_quantizer(qp1);
      const int64_t w = (int64_t)cx.qw[i];
      wgt[0] = (w < q[0].step ? w : (int64_t)q[0].step) >> 8;
      wgt[1] = (w < q[1].step ? w : (int64_t)q[1].step) >> 8;
      if (C == 3 && cx.icp_enabled) {
        const int l = cx.range_lod[r];
        for (int k = 0; k < 3; k++)
          icpc[k] = cx.icp[3 * l + k];
      }
      for (int k = 0; k < C; k++) {
        if (ENC)
          col[k] = (cx.src ? cx.src : cx.attrs)[(size_t)pt * C + k];
        else
          val[k] = cx.values[(size_t)i * C + k];
      }
    }
    int32_t nbv[3][C];
    for (int j = 0; j < 3; j++)
      for (int k = 0; k < C; k++)
        nbv[j][k] = 0;
    uint32_t have = 0;  // neighbours received
    const uint32_t want = live ? (1u << cnt) - 1 : 0;
    if (INTER) {
      // neighbours in the reference frame: their values do not wait for anybody
      for (int j = 0; j < 3; j++)
        if (j < cnt && nidx[j] >= cx.n) {
          nbv[j][0] = cx.frame_attr[nidx[j] - cx.n];
          have |= 1u << j;
        }
    }
    int32_t myrec[C];
    for (int k = 0; k < C; k++)
      myrec[k] = 0;
    int mydone = 0;
    bool pending = live;
    unsigned spins = 0;
    while (__any(pending)) {
      // neighbours inside the claim: lane to lane
      for (int j = 0; j < 3; j++) {
        const int src = nidx[j] - base;
        const bool inw = j < cnt && src >= 0 && (!INTER || nidx[j] < cx.n);
        const int sl = inw ? src : lane;
        const int d = __shfl(mydone, sl);
        int32_t v[C];
        for (int k = 0; k < C; k++)
          v[k] = __shfl(myrec[k], sl);
        if (inw && d && !((have >> j) & 1)) {
          for (int k = 0; k < C; k++)
            nbv[j][k] = v[k];
          have |= 1u << j;
        }
      }
      // neighbours of earlier claims: poll their granules, loads first
      {
        const uint32_t todo = pending ? want & ~have : 0;
        u32x4 g[3];
        for (int j = 0; j < 3; j++) {
          g[j] = u32x4{0, 0, 0, 0};
          if (((todo >> j) & 1) && nidx[j] < base)
            g[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, nidx[j] * 16, 0, /*sc1*/ 16);
        }
        for (int j = 0; j < 3; j++)
          if (((todo >> j) & 1) && nidx[j] < base && g[j].w == cx.tag) {
            nbv[j][0] = (int32_t)g[j].x;
            nbv[j][1 % C] = C > 1 ? (int32_t)g[j].y : nbv[j][1 % C];
            nbv[j][2 % C] = C > 2 ? (int32_t)g[j].z : nbv[j][2 % C];
            have |= 1u << j;
          }
      }
      const bool ready = pending && have == want;
      if (ready) {
        pred_point<C, ENC>(
          cx, ENC ? cx.rm + (size_t)i * 6 : nullptr, cnt, nbv, nwt, col, q, wgt, icpc, maxcand, clip_max, val, myrec);
        {
          const u32x4 st = {(uint32_t)myrec[0], (uint32_t)myrec[1 % C], (uint32_t)myrec[2 % C], cx.tag};
          __builtin_amdgcn_raw_buffer_store_b128(st, rsrc, i * 16, 0, /*sc1*/ 16);
        }
        for (int k = 0; k < C; k++) {
          cx.attrs[(size_t)pt * C + k] = myrec[k];
          if (ENC)
            cx.values[(size_t)i * C + k] = val[k];
        }
        mydone = 1;
        pending = false;
      }
      if (!__any(ready)) {
        if (++spins > (1u << 22)) {
          if (lane == 0)
            atomicExch(cx.error, 1);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
    }
  }
}

// ---- the encoder's finish: an ordered walk over what the passes left undecided --------------
// The passes above remove almost every wrong decision within a few rounds; after that a pass
// recomputes the whole slice to move the first wrong decision a few dozen predictors ahead, and
// whether it ever stops is chance.  What a pass leaves behind is enough to finish exactly.  Let V'
// be the values of the pass before the last, R (cx.rm) the trajectory computed from V', V the last
// pass's values and D = { i : V_i != V'_i } in ascending order.  Everything is causal in coding
// order, so on [0, min D) V is the sequential coder's result, and R at d = min D is the exact
// state in front of d.  pred_walk_kernel takes it from there: ONE wavefront walks the predictors
// in coding order from d with the state in registers, pred_point per predictor, and compares as
// it goes.  Once the state behind a predictor equals R's (all 2C words) and the next predictor
// is not in D, everything ahead up to the next element of D is the sequential coder's as well
// (same state, same values, so the same recurrence) -- PROVIDED its neighbours' reconstructions
// are the pass's.  The walk marks every predictor whose reconstruction it changed (w.changed),
// and from a point of agreement it looks ahead, 256 predictors per step across the lanes, for the
// first predictor that is in D or has a marked neighbour; before it has changed a reconstruction
// that is simply the next element of D.  The walk resumes there with R's state, which is exact
// there by the same induction.  It ends at n: every value, every reconstruction and both
// reconstruction copies (attrs, rec) are then the sequential coder's.  No polling, no wait on
// another workgroup; every loop is bounded by n.
struct PredWalk {
  const int32_t* rank;  // [n + 1] rank[i] = elements of D below i (inclusive scan of the flags)
  const int32_t* list;  // [rank[n]] D, ascending
  uint8_t* changed;     // [n] cleared; 1 where the walk changed a reconstruction
  int32_t* out;         // [4] predictors walked, stretches walked, longest stretch, 1 = reached n
};

// flags for the scan: rank[i + 1] = (predictor i's values differ from the previous pass's);
// prev == nullptr (after the very first pass there is nothing to compare with): every predictor
__global__ __launch_bounds__(256) void
pred_diff_flags_kernel(
  const int32_t* __restrict__ values, const int32_t* __restrict__ prev, int n, int c, int32_t* __restrict__ rank)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    bool diff = !prev;
    if (prev)
      for (int k = 0; k < c; k++)
        diff |= values[(size_t)i * c + k] != prev[(size_t)i * c + k];
    rank[i + 1] = diff;
    if (i == 0)
      rank[0] = 0;
  }
}

// after the inclusive scan: D as a list
__global__ __launch_bounds__(256) void
pred_diff_list_kernel(const int32_t* __restrict__ rank, int n, int32_t* __restrict__ list)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    if (rank[i + 1] != rank[i])
      list[rank[i]] = i;
}

constexpr int kWalkBlock = 64;  // predictors staged in LDS per refill
constexpr int kWalkAhead = 4;   // look-ahead: this many wavefront-wide groups per step

template<int C, bool INTER>
__global__ __launch_bounds__(64) void
pred_walk_kernel(PredCtx cx, PredWalk w)
{
  // the records of predictors [i0, i0 + 64): everything a step reads except the log2 table
  __shared__ int32_t s_cnt[kWalkBlock], s_pt[kWalkBlock], s_ni[kWalkBlock][3], s_nw[kWalkBlock][3];
  __shared__ int32_t s_col[kWalkBlock][3], s_old[kWalkBlock][3], s_val[kWalkBlock][3], s_nb[kWalkBlock][3][3];
  __shared__ int32_t s_rec[kWalkBlock][3], s_rm[kWalkBlock + 1][6], s_in_d[kWalkBlock + 1];
  __shared__ int32_t s_next[4];
  __shared__ Quantizer s_q[kWalkBlock][2];
  __shared__ int64_t s_wgt[kWalkBlock][2];
  __shared__ int8_t s_icp[kWalkBlock][3];
  const int lane = threadIdx.x;
  const int n = cx.n;
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(cx.rec, 0, (int)((size_t)n * 16), 0x00020000);
  const int maxcand = cx.max_direct + !cx.avg_disabled;
  const int64_t clip_max = ((int64_t)1 << cx.bitdepth) - 1;
  const int total = w.rank[n];
  int i0 = total > 0 ? w.list[0] : n;
  int32_t st[6] = {0, 0, 0, 0, 0, 0};  // (lane 0's: the state in front of the predictor the walk stands at)
  bool fresh = true;                   // the state is to be taken from R
  int dirty = 0;                       // the walk has changed a reconstruction
  int walked = 0, stretches = 0, longest = 0, run = 0;
  while (i0 < n) {
    // what this wavefront stored (reconstructions, marks) is read back below: complete the stores first
    __threadfence();
    {
      const int i = i0 + lane;
      const bool live = i < n;
      int cnt = 0, pt = 0;
      if (live) {
        cnt = cx.nc[i];
        pt = cx.indexes[i];
        const int r = pred_range_of(cx, i);
        const int layer = cx.range_qlayer[r];
        const int o0 = cx.qp_off ? cx.qp_off[2 * (size_t)pt] : 0;
        const int o1 = cx.qp_off ? cx.qp_off[2 * (size_t)pt + 1] : 0;
        const int qp0 = clip(cx.layer_qp[layer][0] + o0, 4, cx.max_qp);
        const int qp1 = clip(cx.layer_qp[layer][1] + o1 + qp0, 4, cx.max_qp);
        const int64_t qw = (int64_t)cx.qw[i];
        const Quantizer q0 = make_quantizer(qp0), q1 = make_quantizer(qp1);
        s_q[lane][0] = q0;
        s_q[lane][1] = q1;
        s_wgt[lane][0] = (qw < q0.step ? qw : (int64_t)q0.step) >> 8;
        s_wgt[lane][1] = (qw < q1.step ? qw : (int64_t)q1.step) >> 8;
        for (int k = 0; k < 3; k++)
          s_icp[lane][k] = C == 3 && cx.icp_enabled ? cx.icp[3 * cx.range_lod[r] + k] : 0;
        u32x4 g[3];
        for (int j = 0; j < 3; j++) {
          const int nb = j < cnt ? cx.ni[3 * (size_t)i + j] : 0;
          s_ni[lane][j] = nb;
          s_nw[lane][j] = j < cnt ? cx.nw[3 * (size_t)i + j] : 0;
          g[j] = u32x4{0, 0, 0, 0};
          if (j < cnt && INTER && nb >= n)
            g[j].x = (uint32_t)cx.frame_attr[nb - n];
          else if (j < cnt && nb < i0)
            g[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, nb * 16, 0, /*sc1*/ 16);
        }
        for (int j = 0; j < 3; j++) {
          s_nb[lane][j][0] = (int32_t)g[j].x;
          s_nb[lane][j][1] = (int32_t)g[j].y;
          s_nb[lane][j][2] = (int32_t)g[j].z;
        }
        for (int k = 0; k < 3; k++) {
          s_col[lane][k] = k < C ? cx.src[(size_t)pt * C + k] : 0;
          s_old[lane][k] = k < C ? cx.attrs[(size_t)pt * C + k] : 0;
          s_val[lane][k] = k < C ? cx.values[(size_t)i * C + k] : 0;
        }
        for (int k = 0; k < 6; k++)
          s_rm[lane][k] = cx.rm[(size_t)i * 6 + k];
        s_in_d[lane] = w.rank[i + 1] != w.rank[i];
      }
      s_cnt[lane] = cnt;
      s_pt[lane] = pt;
      if (lane == 0) {
        const int e = i0 + kWalkBlock;
        s_in_d[kWalkBlock] = e < n ? w.rank[e + 1] != w.rank[e] : 0;
        for (int k = 0; k < 6; k++)
          s_rm[kWalkBlock][k] = e < n ? cx.rm[(size_t)e * 6 + k] : 0;
      }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- the walk through the block: one lane, the state in its registers ----
    if (lane == 0) {
      int next = i0 + kWalkBlock < n ? i0 + kWalkBlock : n, seek = 0;
      for (int t = 0; t < kWalkBlock && i0 + t < n; t++) {
        const int i = i0 + t;
        if (fresh) {
          for (int k = 0; k < 6; k++)
            st[k] = s_rm[t][k];
          fresh = false;
          stretches++;
          run = 0;
        }
        const int cnt = s_cnt[t], pt = s_pt[t];
        int32_t nbv[3][C];
        int32_t nwt[3], col[3], val[3] = {0, 0, 0}, myrec[C];
        int8_t icpc[3];
        for (int j = 0; j < 3; j++) {
          const int nb = s_ni[t][j];
          const bool mine = j < cnt && nb >= i0 && (!INTER || nb < n);  // walked in this block
          for (int k = 0; k < C; k++)
            nbv[j][k] = j < cnt ? (mine ? s_rec[nb - i0][k] : s_nb[t][j][k]) : 0;
          nwt[j] = s_nw[t][j];
          col[j] = s_col[t][j];
          icpc[j] = s_icp[t][j];
        }
        const Quantizer q[2] = {s_q[t][0], s_q[t][1]};
        const int64_t wgt[2] = {s_wgt[t][0], s_wgt[t][1]};
        pred_point<C, true>(cx, st, cnt, nbv, nwt, col, q, wgt, icpc, maxcand, clip_max, val, myrec);
        bool rchg = false;
        for (int k = 0; k < C; k++) {
          rchg |= myrec[k] != s_old[t][k];
          s_rec[t][k] = myrec[k];
          cx.attrs[(size_t)pt * C + k] = myrec[k];
          cx.values[(size_t)i * C + k] = val[k];
        }
        {
          const u32x4 gr = {(uint32_t)myrec[0], (uint32_t)myrec[1 % C], (uint32_t)myrec[2 % C], cx.tag};
          __builtin_amdgcn_raw_buffer_store_b128(gr, rsrc, i * 16, 0, /*sc1*/ 16);
        }
        if (rchg) {
          w.changed[i] = 1;
          dirty = 1;
        }
        // resStatUpdate
        bool same = true;
        for (int k = 0; k < C; k++) {
          st[k] = pred_rate_step(st[k], val[k] != 0);
          if (val[k])
            st[3 + k] = pred_rate_step(st[3 + k], (val[k] < 0 ? -val[k] : val[k]) > 1);
          same &= st[k] == s_rm[t + 1][k] && st[3 + k] == s_rm[t + 1][3 + k];
        }
        walked++;
        run++;
        longest = run > longest ? run : longest;
        if (i + 1 < n && same && !s_in_d[t + 1]) {
          next = i + 1;
          seek = 1;
          break;
        }
      }
      s_next[0] = next;
      s_next[1] = seek;
      s_next[2] = dirty;
    }
    __builtin_amdgcn_wave_barrier();
    i0 = s_next[0];
    const int seek = s_next[1], any_dirty = s_next[2];
    __builtin_amdgcn_wave_barrier();
    if (!seek)
      continue;
    // ---- agreement at i0: the first predictor at or behind it that has to be walked ----
    fresh = true;
    const int r0 = w.rank[i0];
    const int next_d = r0 < total ? w.list[r0] : n;
    if (!any_dirty) {
      i0 = next_d;
      continue;
    }
    __threadfence();  // (the marks)
    int found = next_d;
    for (int b = i0; b < next_d; b += 64 * kWalkAhead) {
      int cnt[kWalkAhead], nb[kWalkAhead][3];
#pragma unroll
      for (int u = 0; u < kWalkAhead; u++) {
        const int i = b + u * 64 + lane;
        cnt[u] = i < next_d ? cx.nc[i] : 0;
        for (int j = 0; j < 3; j++)
          nb[u][j] = i < next_d ? cx.ni[3 * (size_t)i + j] : 0;
      }
      int hit[kWalkAhead];
#pragma unroll
      for (int u = 0; u < kWalkAhead; u++) {
        hit[u] = 0;
        for (int j = 0; j < 3; j++)
          if (j < cnt[u] && nb[u][j] < n)
            hit[u] |= w.changed[nb[u][j]];
      }
      int first = -1;
#pragma unroll
      for (int u = 0; u < kWalkAhead; u++) {
        const unsigned long long m = __ballot(hit[u] != 0);
        if (first < 0 && m)
          first = b + u * 64 + __ffsll((long long)m) - 1;
      }
      if (first >= 0) {
        found = first;
        break;
      }
    }
    i0 = found;
  }
  if (lane == 0) {
    w.out[0] = walked;
    w.out[1] = stretches;
    w.out[2] = longest;
    w.out[3] = 1;
  }
}

}  // namespace gpcc
