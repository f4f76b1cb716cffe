// quantize_positions.hpp -- what the encoder does to the input cloud in front of the geometry coder
// (PCCTMC3Encoder3::quantization, encoder.cpp:1554-1577) and what it hands to recolouring per slice
// (getPartition with a map, encoder.cpp:1611-1659):
//   quantizePositions      pointset_processing.cpp:170-194   mode 0: every point quantised, duplicates kept
//   quantizePositionsUniq  :143-159                          mode 1: ... merged where the results are equal
//   samplePositionsUniq    :113-134                          mode 2: ... merged where a coarser key is equal
//   reducePointSet         :53-103                           the merge: one std::map insertion per point, last first
//
// reducePointSet restated.  Points with equal keys form a group i0 < i1 < ... < ik of source indices;
// srcIdxDupList[ij] = i(j+1), the last one points to itself; the destination cloud holds one point per group, in
// the order of the groups' first source indices, positioned at Q(src[i0]); idxToSrcIdx[d] = i0.
//
//   qz_init        the bounding box's identity, the sort's tile table
//   qz_quantize    one lane per point: key and position in float exactly as the reference forms them
//                  (__fmul_rn / __fsub_rn / roundf, nothing to contract); the keys' bounding box by a butterfly
//                  over the wavefront, one LDS word per wavefront, six device-scope atomics per workgroup
//   qz_plan        one thread: the bit widths of the three biased key coordinates, one or two sort rounds, how
//                  many 8-bit passes each -- the PLAN stays on the device, the host never waits for the box
//   qz_pack        the biased coordinates packed into a 64-bit key (all three when the widths sum to <= 64,
//                  else y and z: the low word), value = source index
//   qz_sort_*      morton_sort.hpp's passes (stable, 8-bit digits), the digit's shift and the ping-pong
//                  buffers taken from the plan; the host launches as many as its own bound on the widths allows
//                  (the clamp box in modes 0 / 1, 32 bits an axis in mode 2), a pass the plan does not need
//                  returns at once.  qz_rekey between the rounds replaces the key by x: the high word
//   qz_link        over the sorted order: next[] and a head flag per source index.  Stability gives ascending
//                  source indices inside a group
//   qz_head_count  \  ordered compaction of the heads in source order, ref_crop.hpp's shape: a count per tile of
//   kd_scan        |  1 024 source indices, the scan of recolour_kdtree.hpp, the emit with ranks from ballots.
//   qz_emit        /  No atomic decides a position and no workgroup waits for another
// and for the partition, over ALL listed indices of ALL slices at once:
//   part_count     one lane per listed destination index: the length of its chain, validating as it walks
//   kd_scan        one scan over the batch; part_offsets gathers the slices' offsets for the host
//   part_emit      the walk again, positions and c attributes gathered behind the scanned offset
// A chain is a dependent walk by one lane: a group of g points costs g dependent loads, twice.
//
// Domain: every float that the reference converts to int must lie in [-2^31, 2^31) (the conversion is undefined
// outside); a point outside sets the sticky error word to kQzErrorRange.  A listed index outside [0, n_dst), a map
// entry outside [0, n_src) or a next[] entry that does not ascend sets kQzErrorMap; the walk stops there, so it
// never leaves the arrays and always ends.
//
// Launches are written with hipLaunchKernelGGL and the HIP runtime calls are plain, so that the header also
// compiles for the CPU wavefront emulator (tests/emu).
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "morton_sort.hpp"
#include "recolour_kdtree.hpp"

#ifdef GPCC_EMU
// (the emulator's compiler targets a CPU without fused multiply-add: one rounding per operation as written)
inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
inline float __fsub_rn(float a, float b) { volatile float r = a - b; return r; }
#endif

namespace gpcc {

constexpr int kQzBlock = 256;
constexpr int kQzTile = 1024;      // source indices per workgroup of the compaction: four per thread
constexpr int kQzErrorRange = 8;   // the sticky error word's codes (check_device_error)
constexpr int kQzErrorMap = 9;
constexpr int kQzGridMax = 2048;

// the plan: int32 words on the device
enum {
  kQzMin = 0,        // [3] the keys' bounding box
  kQzMax = 3,        // [3]
  kQzWidth = 6,      // [3] bits of max - min per axis
  kQzTwoRounds = 9,  // the widths sum to more than 64
  kQzPasses1 = 10,   // passes of the first (or only) round
  kQzPasses2 = 11,   // passes of the second round
  kQzPlanWords = 16
};

struct QzArgs {
  const int32_t* src;  // [n][3]
  int32_t* key;        // [n][3] what is compared
  int32_t* pos;        // [n][3] what is emitted; == key in modes 0 and 1
  int32_t* plan;       // [kQzPlanWords]
  int32_t* error;      // the context's sticky error word
  int32_t n;
  int32_t mode;
  float scale;         // scaleFactor / quantScale
  float diff_scale;    // mode 2: sampleScale / quantScale, divided on the host as the reference does
  int32_t offset[3];
  int32_t clamp_min[3], clamp_max[3];
};

// the sort's buffers and tables, the map, the compaction's counts
struct QzWork {
  int64_t* skey[2];     // [n] ping-pong
  int32_t* sval[2];     // [n]
  int32_t* pt_off;      // [2]
  int32_t* tile_first;  // [sort tiles]
  int32_t* tile_count;
  int32_t* tile_slice;
  uint32_t* hist;       // [256][sort tiles]
  int32_t* next;        // [n] out: srcIdxDupList
  uint8_t* head;        // [n] 1: the first point of its group
  int32_t* counts;      // [compaction tiles + 1]; tile t at t + 1, [0] = 0
  long long* sums;      // the scan's block sums
  int32_t* idx_to_src;  // [n] out (the first num_dst entries)
  int32_t* dst;         // [n][3] out (the first num_dst points)
  int32_t num_sort_tiles;
  int32_t num_tiles;    // of the compaction
};

inline int
qz_sort_tiles(int64_t n)
{
  return (int)((n + kSortTile - 1) / kSortTile);
}
inline int
qz_tiles(int64_t n)
{
  return (int)((n + kQzTile - 1) / kQzTile);
}
inline size_t
qz_sum_entries(size_t count_entries)
{
  return count_entries / kKdScanBlock + 2;
}
inline int
qz_grid(int64_t items)
{
  const int64_t g = (items + kQzBlock - 1) / kQzBlock;
  return (int)(g < 1 ? 1 : g > kQzGridMax ? kQzGridMax : g);
}

// take(bytes) -> char*: the library's arena, or the emulator harness's guarded allocations.  mode 0 needs only
// args.key; modes 1 and 2 the rest (mode 2 a second position array).
template<class Take>
inline void
qz_carve(Take&& take, int64_t n, int mode, QzArgs& a, QzWork& w)
{
  const size_t N = (size_t)n;
  a.plan = (int32_t*)take(sizeof(int32_t) * kQzPlanWords);
  a.key = (int32_t*)take(sizeof(int32_t) * 3 * N);
  a.pos = mode == 2 ? (int32_t*)take(sizeof(int32_t) * 3 * N) : a.key;
  if (mode == 0)
    return;
  w.num_sort_tiles = qz_sort_tiles(n);
  w.num_tiles = qz_tiles(n);
  for (int b = 0; b < 2; b++) {
    w.skey[b] = (int64_t*)take(sizeof(int64_t) * N);
    w.sval[b] = (int32_t*)take(sizeof(int32_t) * N);
  }
  w.pt_off = (int32_t*)take(sizeof(int32_t) * 2);
  w.tile_first = (int32_t*)take(sizeof(int32_t) * w.num_sort_tiles);
  w.tile_count = (int32_t*)take(sizeof(int32_t) * w.num_sort_tiles);
  w.tile_slice = (int32_t*)take(sizeof(int32_t) * w.num_sort_tiles);
  w.hist = (uint32_t*)take(sizeof(uint32_t) * 256 * (size_t)w.num_sort_tiles);
  w.next = (int32_t*)take(sizeof(int32_t) * N);
  w.head = (uint8_t*)take(N);
  w.counts = (int32_t*)take(sizeof(int32_t) * ((size_t)w.num_tiles + 1));
  w.sums = (long long*)take(sizeof(long long) * qz_sum_entries((size_t)w.num_tiles + 1));
  w.idx_to_src = (int32_t*)take(sizeof(int32_t) * N);
  w.dst = (int32_t*)take(sizeof(int32_t) * 3 * N);
}

// The host's bound on the passes of the two rounds, from what it knows without looking at a point: the clamp
// box in modes 0 / 1, the whole int32 range in mode 2.  The plan on the device never asks for more.
inline void
qz_pass_bounds(int mode, const int32_t* clamp_min, const int32_t* clamp_max, int* max1, int* max2)
{
  int wb[3], sum = 0;
  for (int k = 0; k < 3; k++) {
    const uint32_t span = mode == 2 ? 0xffffffffu : (uint32_t)clamp_max[k] - (uint32_t)clamp_min[k];
    wb[k] = 0;
    while (wb[k] < 32 && (span >> wb[k]))
      wb[k]++;
    sum += wb[k];
  }
  if (sum <= 64) {
    *max1 = (sum + 7) / 8;
    *max2 = 0;
  } else {
    *max1 = 8;  // (the data may still fit one 64-bit key)
    *max2 = (wb[0] + 7) / 8;
  }
}

__global__ __launch_bounds__(kQzBlock) void
qz_init_kernel(QzArgs a, QzWork w)
{
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (t0 == 0) {
    for (int k = 0; k < 3; k++) {
      a.plan[kQzMin + k] = INT32_MAX;
      a.plan[kQzMax + k] = INT32_MIN;
    }
    for (int k = kQzWidth; k < kQzPlanWords; k++)
      a.plan[k] = 0;
    if (a.mode != 0) {
      w.pt_off[0] = 0;
      w.pt_off[1] = a.n;
      w.counts[0] = 0;
    }
  }
  if (a.mode == 0)
    return;
  for (int t = t0; t < w.num_sort_tiles; t += gridDim.x * blockDim.x) {
    const int64_t first = (int64_t)t * kSortTile;
    w.tile_first[t] = (int32_t)first;
    w.tile_count[t] = (int32_t)(a.n - first < kSortTile ? a.n - first : kSortTile);
    w.tile_slice[t] = 0;
  }
}

__device__ __forceinline__ bool
qz_in_int32(float f)
{
  return f >= -2147483648.0f && f < 2147483648.0f;  // (false for a NaN)
}

__global__ __launch_bounds__(kQzBlock) void
qz_quantize_kernel(QzArgs a)
{
  __shared__ int32_t wave_box[6][kQzBlock / 64];
  const int tid = threadIdx.x;
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * kQzBlock + tid; i < a.n; i += (int64_t)gridDim.x * kQzBlock) {
    int32_t key[3], pos[3];
    bool ok = true;
    for (int k = 0; k < 3; k++) {
      // int -> float rounds to nearest even; std::round(float) is roundf: halves away from zero
      const float t = roundf(__fmul_rn((float)a.src[3 * i + k], a.scale));
      if (a.mode == 2) {
        const float u = roundf(__fmul_rn(t, a.diff_scale));
        ok = ok && qz_in_int32(t) && qz_in_int32(u);
        key[k] = ok ? (int32_t)u : 0;
        pos[k] = ok ? (int32_t)((uint32_t)(int32_t)t - (uint32_t)a.offset[k]) : 0;  // (an integer subtraction)
      } else {
        const float f = __fsub_rn(t, (float)a.offset[k]);
        ok = ok && qz_in_int32(f);
        const int32_t q = ok ? (int32_t)f : 0;
        key[k] = q < a.clamp_min[k] ? a.clamp_min[k] : q > a.clamp_max[k] ? a.clamp_max[k] : q;
        pos[k] = key[k];
      }
    }
    bad = bad || !ok;
    for (int k = 0; k < 3; k++) {
      a.key[3 * i + k] = key[k];
      if (a.mode == 2)
        a.pos[3 * i + k] = pos[k];
      lo[k] = key[k] < lo[k] ? key[k] : lo[k];
      hi[k] = key[k] > hi[k] ? key[k] : hi[k];
    }
  }
  if (bad)
    atomicCAS(a.error, 0, kQzErrorRange);
  // (every lane of the workgroup is here: the collectives below are convergent)
  for (int k = 0; k < 3; k++) {
    int32_t mn = lo[k], mx = hi[k];
    for (int m = 32; m >= 1; m >>= 1) {
      const int32_t on = __shfl_xor(mn, m, 64), ox = __shfl_xor(mx, m, 64);
      mn = on < mn ? on : mn;
      mx = ox > mx ? ox : mx;
    }
    if ((tid & 63) == 0) {
      wave_box[k][tid >> 6] = mn;
      wave_box[3 + k][tid >> 6] = mx;
    }
  }
  __syncthreads();
  if (tid < 6) {
    int32_t v = wave_box[tid][0];
    for (int w = 1; w < kQzBlock / 64; w++) {
      const int32_t o = wave_box[tid][w];
      v = tid < 3 ? (o < v ? o : v) : (o > v ? o : v);
    }
    if (tid < 3)
      atomicMin(a.plan + kQzMin + tid, v);
    else
      atomicMax(a.plan + kQzMin + tid, v);
  }
}

__global__ void
qz_plan_kernel(int32_t* plan)
{
  if (blockIdx.x != 0 || threadIdx.x != 0)
    return;
  int w[3], sum = 0;
  for (int k = 0; k < 3; k++) {
    const uint32_t span = (uint32_t)plan[kQzMax + k] - (uint32_t)plan[kQzMin + k];
    w[k] = span ? 32 - __clz((int)span) : 0;
    plan[kQzWidth + k] = w[k];
    sum += w[k];
  }
  const int two = sum > 64;
  plan[kQzTwoRounds] = two;
  plan[kQzPasses1] = ((two ? w[1] + w[2] : sum) + 7) / 8;
  plan[kQzPasses2] = two ? (w[0] + 7) / 8 : 0;
}

// the biased coordinate of axis k: 0 .. 2^width - 1
__device__ __forceinline__ uint64_t
qz_biased(const int32_t* __restrict__ key, const int32_t* __restrict__ plan, int64_t i, int k)
{
  return (uint32_t)key[3 * i + k] - (uint32_t)plan[kQzMin + k];
}

__global__ __launch_bounds__(kQzBlock) void
qz_pack_kernel(QzArgs a, QzWork w)
{
  const int wy = a.plan[kQzWidth + 1], wz = a.plan[kQzWidth + 2];
  const bool two = a.plan[kQzTwoRounds] != 0;
  for (int64_t i = (int64_t)blockIdx.x * kQzBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kQzBlock) {
    // (a shift by the full width only where the shifted value is zero anyway: guarded)
    uint64_t k = qz_biased(a.key, a.plan, i, 2) | (wz < 64 ? qz_biased(a.key, a.plan, i, 1) << wz : 0);
    if (!two && wy + wz < 64)
      k |= qz_biased(a.key, a.plan, i, 0) << (wy + wz);
    w.skey[0][i] = (int64_t)k;
    w.sval[0][i] = (int32_t)i;
  }
}

// Pass j of a round as the plan has it: false when the plan does not need it.  Passes 0 .. passes1 - 1 of the
// first round read buffer j & 1; the second round goes on from where the first one stopped.
__device__ __forceinline__ bool
qz_sort_ctx(const QzArgs& a, const QzWork& w, int round, int j, SortCtx* cx)
{
  const int p1 = a.plan[kQzPasses1], p2 = a.plan[kQzPasses2];
  if (j >= (round ? p2 : p1))
    return false;
  const int b = (round ? p1 + j : j) & 1;
  cx->n = a.n;
  cx->num_tiles = w.num_sort_tiles;
  cx->num_slices = 1;
  cx->pt_off = w.pt_off;
  cx->tile_first = w.tile_first;
  cx->tile_count = w.tile_count;
  cx->tile_slice = w.tile_slice;
  cx->hist = w.hist;
  cx->key_in = w.skey[b];
  cx->val_in = w.sval[b];
  cx->key_out = w.skey[b ^ 1];
  cx->val_out = w.sval[b ^ 1];
  cx->shift = 8 * j;
  return true;
}

__global__ __launch_bounds__(kSortThreads) void
qz_sort_hist_kernel(QzArgs a, QzWork w, int round, int j)
{
  SortCtx cx;
  if (qz_sort_ctx(a, w, round, j, &cx))  // (uniform over the grid)
    sort_hist_pass(cx);
}

__global__ __launch_bounds__(1024) void
qz_sort_scan_kernel(QzArgs a, QzWork w, int round, int j)
{
  SortCtx cx;
  if (qz_sort_ctx(a, w, round, j, &cx))
    sort_scan_pass(cx);
}

__global__ __launch_bounds__(kSortThreads) void
qz_sort_scatter_kernel(QzArgs a, QzWork w, int round, int j)
{
  SortCtx cx;
  if (qz_sort_ctx(a, w, round, j, &cx))
    sort_scatter_pass(cx);
}

// between the rounds: the high word (x) of the point at each sorted place, in place
__global__ __launch_bounds__(kQzBlock) void
qz_rekey_kernel(QzArgs a, QzWork w)
{
  if (!a.plan[kQzTwoRounds])
    return;
  const int b = a.plan[kQzPasses1] & 1;
  for (int64_t i = (int64_t)blockIdx.x * kQzBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kQzBlock)
    w.skey[b][i] = (int64_t)qz_biased(a.key, a.plan, w.sval[b][i], 0);
}

// Sorted place i holds source index s, place i + 1 holds t: equal keys make t the next of s, else s ends its
// chain and t is a head.  Every source index is written once to next[] and once to head[].
__global__ __launch_bounds__(kQzBlock) void
qz_link_kernel(QzArgs a, QzWork w)
{
  const int32_t* order = w.sval[(a.plan[kQzPasses1] + a.plan[kQzPasses2]) & 1];
  for (int64_t i = (int64_t)blockIdx.x * kQzBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kQzBlock) {
    const int32_t s = order[i];
    if (i == 0)
      w.head[s] = 1;
    if (i + 1 == a.n) {
      w.next[s] = s;
      continue;
    }
    const int32_t t = order[i + 1];
    const bool same = a.key[3 * (int64_t)s] == a.key[3 * (int64_t)t] && a.key[3 * (int64_t)s + 1] == a.key[3 * (int64_t)t + 1]
      && a.key[3 * (int64_t)s + 2] == a.key[3 * (int64_t)t + 2];
    w.next[s] = same ? t : s;
    w.head[t] = same ? 0 : 1;
  }
}

// bit k: source index p0 + k exists and is a head
__device__ __forceinline__ unsigned
qz_head_flags(const uint8_t* __restrict__ head, int64_t p0, int64_t n)
{
  unsigned in = 0;
  for (int k = 0; k < 4; k++)
    if (p0 + k < n && head[p0 + k])
      in |= 1u << k;
  return in;
}

// grid: the compaction's tiles
__global__ __launch_bounds__(kQzBlock) void
qz_head_count_kernel(QzArgs a, QzWork w)
{
  __shared__ int32_t wave_cnt[kQzBlock / 64];
  const int tid = threadIdx.x;
  const unsigned in = qz_head_flags(w.head, (int64_t)blockIdx.x * kQzTile + 4 * tid, a.n);
  int cnt = 0;
  for (int k = 0; k < 4; k++)
    cnt += __popcll(__ballot((in >> k) & 1));
  if ((tid & 63) == 0)
    wave_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int sum = 0;
    for (int v = 0; v < kQzBlock / 64; v++)
      sum += wave_cnt[v];
    w.counts[(size_t)blockIdx.x + 1] = sum;
  }
}

// counts: scanned.  The rank inside the wavefront from the ballots, the wavefronts' bases through LDS, the tile's
// base from the scan: heads leave in source order.
__global__ __launch_bounds__(kQzBlock) void
qz_emit_kernel(QzArgs a, QzWork w)
{
  __shared__ int32_t wave_cnt[kQzBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t p0 = (int64_t)blockIdx.x * kQzTile + 4 * tid;
  const unsigned in = qz_head_flags(w.head, p0, a.n);
  const unsigned long long below = (1ull << lane) - 1;
  int cnt = 0, before = 0;
  // (a thread's four indices are consecutive: ranks count whole threads below, then the thread's own flags)
  for (int k = 0; k < 4; k++) {
    const unsigned long long m = __ballot((in >> k) & 1);
    cnt += __popcll(m);
    before += __popcll(m & below);
  }
  if (lane == 0)
    wave_cnt[wave] = cnt;
  __syncthreads();
  int64_t at = (int64_t)w.counts[blockIdx.x] + before;
  for (int v = 0; v < wave; v++)
    at += wave_cnt[v];
  for (int k = 0; k < 4; k++) {
    if (!((in >> k) & 1))
      continue;
    w.idx_to_src[at] = (int32_t)(p0 + k);
    for (int j = 0; j < 3; j++)
      w.dst[3 * at + j] = a.pos[3 * (p0 + k) + j];
    at++;
  }
}

// Everything in front of the host's one wait.  max1 / max2: qz_pass_bounds().  span(name): an object that lives as
// long as the launch it names (the library's per-kernel timer).  Mode 0 ends behind the quantiser.
template<class Span>
inline hipError_t
qz_count_launch(hipStream_t st, const QzArgs& a, const QzWork& w, int max1, int max2, Span&& span)
{
  {
    auto t = span("qz_init");
    hipLaunchKernelGGL(qz_init_kernel, dim3(qz_grid(a.mode ? w.num_sort_tiles : 1)), dim3(kQzBlock), 0, st, a, w);
  }
  {
    auto t = span("qz_quantize");
    hipLaunchKernelGGL(qz_quantize_kernel, dim3(qz_grid(a.n)), dim3(kQzBlock), 0, st, a);
  }
  if (a.mode == 0)
    return hipGetLastError();
  {
    auto t = span("qz_plan");
    hipLaunchKernelGGL(qz_plan_kernel, dim3(1), dim3(64), 0, st, a.plan);
  }
  {
    auto t = span("qz_pack");
    hipLaunchKernelGGL(qz_pack_kernel, dim3(qz_grid(a.n)), dim3(kQzBlock), 0, st, a, w);
  }
  const int sort_grid = w.num_sort_tiles < kQzGridMax ? w.num_sort_tiles : kQzGridMax;
  for (int round = 0; round < 2; round++) {
    if (round == 1 && max2 > 0) {
      auto t = span("qz_rekey");
      hipLaunchKernelGGL(qz_rekey_kernel, dim3(qz_grid(a.n)), dim3(kQzBlock), 0, st, a, w);
    }
    for (int j = 0; j < (round ? max2 : max1); j++) {
      {
        auto t = span("qz_sort_hist");
        hipLaunchKernelGGL(qz_sort_hist_kernel, dim3(sort_grid), dim3(kSortThreads), 0, st, a, w, round, j);
      }
      {
        auto t = span("qz_sort_scan");
        hipLaunchKernelGGL(qz_sort_scan_kernel, dim3(1), dim3(1024), 0, st, a, w, round, j);
      }
      {
        auto t = span("qz_sort_scatter");
        hipLaunchKernelGGL(qz_sort_scatter_kernel, dim3(sort_grid), dim3(kSortThreads), 0, st, a, w, round, j);
      }
    }
  }
  {
    auto t = span("qz_link");
    hipLaunchKernelGGL(qz_link_kernel, dim3(qz_grid(a.n)), dim3(kQzBlock), 0, st, a, w);
  }
  {
    auto t = span("qz_head_count");
    hipLaunchKernelGGL(qz_head_count_kernel, dim3(w.num_tiles), dim3(kQzBlock), 0, st, a, w);
  }
  {
    auto t = span("qz_scan");
    hipError_t e = kd_scan(st, w.counts, (size_t)w.num_tiles + 1, w.sums);
    if (e != hipSuccess)
      return e;
  }
  return hipGetLastError();
}

// behind the wait: w.counts[w.num_tiles] is the number of destination points
template<class Span>
inline hipError_t
qz_emit_launch(hipStream_t st, const QzArgs& a, const QzWork& w, Span&& span)
{
  auto t = span("qz_emit");
  hipLaunchKernelGGL(qz_emit_kernel, dim3(w.num_tiles), dim3(kQzBlock), 0, st, a, w);
  return hipGetLastError();
}

// ---- the source points of a batch of slices (getPartition with a map) -------------------------------------------

struct PartArgs {
  const int32_t* src_xyz;        // [n_src][3]
  const int32_t* src_attrs;      // [n_src][c], or null
  const int32_t* idx_to_src;     // [n_dst]
  const int32_t* next;           // [n_src]
  const int32_t* indexes;        // [listed] destination indices of all slices, slice after slice
  const int32_t* index_offsets;  // [num_slices + 1]
  int32_t* counts;               // [listed + 1]; listed index j at j + 1, [0] = 0
  unsigned long long* total;     // the chains' lengths summed in 64 bits (the scan's entries are int32)
  int32_t* offsets;              // [num_slices + 1] out
  int32_t* out_xyz;              // [offsets[num_slices]][3]
  int32_t* out_attrs;            // [offsets[num_slices]][c], or null
  int32_t* error;
  int32_t n_src, n_dst, c;
  int32_t listed, num_slices;
};

// The first source point of listed index j, or -1 with the error word set.
__device__ __forceinline__ int32_t
part_head(const PartArgs& a, int64_t j)
{
  const int32_t d = a.indexes[j];
  if (d < 0 || d >= a.n_dst)
    return -1;
  const int32_t s = a.idx_to_src[d];
  return s < 0 || s >= a.n_src ? -1 : s;
}

__global__ __launch_bounds__(kQzBlock) void
part_count_kernel(PartArgs a)
{
  __shared__ long long wave_sum[kQzBlock / 64];
  const int tid = threadIdx.x;
  long long mine = 0;
  bool bad = false;
  if (blockIdx.x == 0 && tid == 0) {
    a.counts[0] = 0;
  }
  for (int64_t j = (int64_t)blockIdx.x * kQzBlock + tid; j < a.listed; j += (int64_t)gridDim.x * kQzBlock) {
    int32_t len = 0;
    int32_t s = part_head(a, j);
    bad = bad || s < 0;
    while (s >= 0) {
      len++;
      const int32_t t = a.next[s];
      if (t == s)
        break;
      // (strictly ascending and inside the array: the walk ends after at most n_src steps)
      if (t < s || t >= a.n_src) {
        bad = true;
        break;
      }
      s = t;
    }
    a.counts[j + 1] = len;
    mine += len;
  }
  if (bad)
    atomicCAS(a.error, 0, kQzErrorMap);
  for (int m = 32; m >= 1; m >>= 1)
    mine += __shfl_xor(mine, m, 64);
  if ((tid & 63) == 0)
    wave_sum[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    long long s = 0;
    for (int v = 0; v < kQzBlock / 64; v++)
      s += wave_sum[v];
    if (s)
      atomicAdd(a.total, (unsigned long long)s);
  }
}

__global__ __launch_bounds__(256) void
part_offsets_kernel(PartArgs a)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= a.num_slices)
    a.offsets[s] = a.counts[a.index_offsets[s]];
}

// counts: scanned; the map has been validated by the count pass
__global__ __launch_bounds__(kQzBlock) void
part_emit_kernel(PartArgs a)
{
  for (int64_t j = (int64_t)blockIdx.x * kQzBlock + threadIdx.x; j < a.listed; j += (int64_t)gridDim.x * kQzBlock) {
    int64_t at = a.counts[j];
    const int64_t end = a.counts[j + 1];
    int32_t s = part_head(a, j);
    while (s >= 0 && at < end) {
      for (int k = 0; k < 3; k++)
        a.out_xyz[3 * at + k] = a.src_xyz[3 * (int64_t)s + k];
      if (a.out_attrs)
        for (int k = 0; k < a.c; k++)
          a.out_attrs[a.c * at + k] = a.src_attrs[(int64_t)a.c * s + k];
      at++;
      s = a.next[s];
    }
  }
}

inline size_t
part_sum_entries(int64_t listed)
{
  return qz_sum_entries((size_t)listed + 1);
}

// in front of the host's wait: a.total cleared, the counts, their scan, the slices' offsets
template<class Span>
inline hipError_t
part_count_launch(hipStream_t st, const PartArgs& a, long long* sums, Span&& span)
{
  hipError_t e = hipMemsetAsync(a.total, 0, sizeof(unsigned long long), st);
  if (e != hipSuccess)
    return e;
  {
    auto t = span("part_count");
    hipLaunchKernelGGL(part_count_kernel, dim3(qz_grid(a.listed)), dim3(kQzBlock), 0, st, a);
  }
  {
    auto t = span("part_scan");
    e = kd_scan(st, a.counts, (size_t)a.listed + 1, sums);
    if (e != hipSuccess)
      return e;
  }
  {
    auto t = span("part_offsets");
    hipLaunchKernelGGL(part_offsets_kernel, dim3(a.num_slices / 256 + 1), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

template<class Span>
inline hipError_t
part_emit_launch(hipStream_t st, const PartArgs& a, Span&& span)
{
  auto t = span("part_emit");
  hipLaunchKernelGGL(part_emit_kernel, dim3(qz_grid(a.listed)), dim3(kQzBlock), 0, st, a);
  return hipGetLastError();
}

}  // namespace gpcc
