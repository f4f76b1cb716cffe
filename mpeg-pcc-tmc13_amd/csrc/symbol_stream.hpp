// symbol_stream.hpp -- the entropy front end of the device tier: a batch of coefficient streams in HBM to the
// (run, values) symbols of the entropy loops and to the binary decisions of PCCResidualsEncoder (residual_bins.hpp),
// and back: a batch of symbol streams to dense coefficients.
//
// The symbol syntax is the same for the three coders (AttributeEncoder.cpp:1279-1291, 1458-1474, 829-853): a zero
// run over the positions whose components are all zero, then the values of the next position; a last run when the
// stream ends in zeros.  Per slice, nothing is carried from one slice to the next.
//
// Coefficients to symbols and bins.  The work is a (slice, tile) table as in spherical.hpp (RplArgs): tiles of
// 1 024 positions that never straddle a slice, one workgroup per tile, the four wavefronts of it 256 consecutive
// positions each in four rows of 64, so that a ballot IS the row's coded mask.
//   sym_tile_summary  the coded flag of every position (any component non-zero, either layout); the 16 mask words of
//                     the tile, its number of coded positions, its last coded position (as an index into the batch)
//   scan              exclusive, over the tiles of ALL slices: the sum of the counts (a tile's first symbol) and the
//                     running maximum of the last coded positions (a tile's predecessor).  Neither is segmented: a
//                     slice subtracts the sum at its first tile, and a maximum below its first point is "none"
//   sym_count         every coded position finds its predecessor -- in its row's mask, in the masks of the rows in
//                     front of it, in the scanned maximum -- and so its run; writes the symbol when asked to; counts
//                     its decisions; the tile's sum, the slice's last tile with the trailing run's decisions
//   scan              the tiles' decision sums, 64 bit
//   sym_slices        per slice: the offset of its decisions, its number of symbols, its trailing run -- what the
//                     host reads in its one wait, because it has to know the total before anything is written
//   sym_emit          the runs and the counts again; every coded position writes its decisions at its offset
// The zero coefficients are read once (the summary); the other passes read the masks and the coded values.
//
// Symbols to coefficients.  Symbol k of a slice lies at sum_{j <= k} (runs[j] + 1) - 1.  Tiles of 1 024 symbols that
// never straddle a slice:
//   memset            the batch's coefficients
//   sym_unpack_sums   64-bit tile sums (adversarial runs do not wrap: 2^29 symbols of 2^31 at the most)
//   scan              exclusive over the tiles of all slices; a slice subtracts the sum at its first tile
//   sym_unpack_scatter the scan inside the tile again; values[k][0 .. c) to the slice's layout
// A negative run, or a position outside the slice, is not written and sets the context's sticky error word to
// kSymUnpackErrorRange.
//
// No atomic decides a position and no workgroup waits for another: plain multi-pass scans, as in ref_crop.hpp.
// The number of launches does not depend on the number of slices.
//
// Launches are written with hipLaunchKernelGGL and the HIP runtime calls are plain, so that the header also compiles
// for the CPU wavefront emulator (tests/emu).
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "residual_bins.hpp"
#include "spherical.hpp"

namespace gpcc {

constexpr int kSymBlock = 256;
constexpr int kSymTile = kRplTile;        // positions (symbols, for the unpack) per workgroup
constexpr int kSymWords = kSymTile / 64;  // mask words per tile
constexpr int kSymScanBlock = 2048;       // entries per workgroup of the scan
constexpr int kSymUnpackErrorRange = 7;   // the sticky error word's code (check_device_error)

static_assert(kSymTile == 4 * kSymBlock && kSymWords == 16, "four rows of 64 per wavefront");

struct SymArgs {
  const int32_t* coeffs;        // slice s at coeffs + c * pt_off[s]: planar [c][n_s] or [n_s][c]
  const int32_t* pt_off;        // [num_slices + 1]
  const int32_t* tile_off;      // [num_slices + 1]
  unsigned long long* mask;     // [num_tiles][kSymWords]
  int32_t* tile_cnt;            // [num_tiles] coded positions
  int32_t* tile_last;           // [num_tiles] last coded position as an index into the batch, -1: none
  long long* sym_base;          // [num_tiles + 1] scanned tile_cnt
  long long* prev;              // [num_tiles + 1] scanned tile_last: the last coded position in front of the tile
  int32_t* tile_bins;           // [num_tiles] decisions
  long long* bin_base;          // [num_tiles + 1] scanned tile_bins
  long long* scan_sums;         // [sym_scan_blocks(num_tiles)] each
  long long* scan_maxs;
  long long* bin_offsets;       // [num_slices + 1]
  int32_t* num_symbols;         // [num_slices]
  int32_t* trailing_run;        // [num_slices]
  int32_t* runs;                // slice s at runs + pt_off[s]; nullptr: no symbol output
  int32_t* values;              // slice s at values + c * pt_off[s], [num_symbols][c]; nullptr: no symbol output
  uint8_t* bins;
  int32_t c;
  int32_t planar;
  int32_t num_slices;
  int32_t num_tiles;
};

struct SymUnpackArgs {
  const int32_t* runs;          // symbols of slice s: [sym_off[s], sym_off[s + 1])
  const int32_t* values;        // [symbols][c]
  const int32_t* pt_off;        // [num_slices + 1]
  const int32_t* sym_off;       // [num_slices + 1]
  const int32_t* tile_off;      // [num_slices + 1] tiles of symbols; a slice without symbols has none
  long long* tile_sum;          // [num_tiles]
  long long* tile_base;         // [num_tiles + 1] scanned tile_sum
  long long* scan_sums;         // [sym_scan_blocks(num_tiles)]
  int32_t* coeffs;              // out, layout as SymArgs::coeffs; every position is written
  int32_t* error;               // the context's sticky error word
  int32_t c;
  int32_t planar;
  int32_t num_slices;
  int32_t num_tiles;
};

inline size_t
sym_scan_blocks(size_t n)
{
  return (n + kSymScanBlock - 1) / kSymScanBlock + 1;
}

// ---- exclusive scan of one or two arrays: sums of a (64 bit) and, when b is given, running maxima of b (-1 in
// front of the first entry).  out[n] is the total.  Three launches, no workgroup waits for another. ----
template<class In>
__global__ __launch_bounds__(256) void
sym_scan_sums_kernel(
  const In* __restrict__ a, const int32_t* __restrict__ b, size_t n, long long* __restrict__ sums,
  long long* __restrict__ maxs)
{
  __shared__ long long ws[4], wm[4];
  const size_t base = (size_t)blockIdx.x * kSymScanBlock;
  long long s = 0, m = -1;
  for (int k = 0; k < kSymScanBlock / 256; k++) {
    const size_t i = base + (size_t)k * 256 + threadIdx.x;
    if (i < n) {
      s += (long long)a[i];
      if (b)
        m = b[i] > m ? b[i] : m;
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    s += __shfl_xor(s, d);
    const long long o = __shfl_xor(m, d);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0) {
    ws[threadIdx.x >> 6] = s;
    wm[threadIdx.x >> 6] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long mm = wm[0];
    for (int w = 1; w < 4; w++)
      mm = wm[w] > mm ? wm[w] : mm;
    sums[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
    if (b)
      maxs[blockIdx.x] = mm;
  }
}

// (one workgroup: a thread takes its share of the block totals, the shares are scanned by shuffles and across the
// sixteen wavefronts through LDS)
__global__ __launch_bounds__(1024) void
sym_scan_blocks_kernel(long long* sums, long long* maxs, int nblocks)
{
  __shared__ long long wtot[16], wmax[16];
  const int per = (nblocks + 1023) / 1024;
  const int b0 = threadIdx.x * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
  long long s = 0, m = -1;
  for (int b = b0; b < b1; b++) {
    s += sums[b];
    if (maxs)
      m = maxs[b] > m ? maxs[b] : m;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long inc = s, incm = m;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl_up(inc, d);
    const long long om = __shfl_up(incm, d);
    if (lane >= d) {
      inc += o;
      incm = om > incm ? om : incm;
    }
  }
  // (the maximum in front of this thread's share: of the lanes below)
  long long runm = __shfl_up(incm, 1);
  if (lane == 0)
    runm = -1;
  if (lane == 63) {
    wtot[wave] = inc;
    wmax[wave] = incm;
  }
  __syncthreads();
  long long run = inc - s;
  for (int w = 0; w < wave; w++) {
    run += wtot[w];
    runm = wmax[w] > runm ? wmax[w] : runm;
  }
  for (int b = b0; b < b1; b++) {
    const long long v = sums[b];
    sums[b] = run;
    run += v;
    if (maxs) {
      const long long vm = maxs[b];
      maxs[b] = runm;
      runm = vm > runm ? vm : runm;
    }
  }
}

template<class In>
__global__ __launch_bounds__(256) void
sym_scan_apply_kernel(
  const In* __restrict__ a, const int32_t* __restrict__ b, size_t n, const long long* __restrict__ sums,
  const long long* __restrict__ maxs, long long* __restrict__ out_sum, long long* __restrict__ out_max)
{
  GPCC_VGPR_FLOOR_64();  // (50 registers otherwise: the fenced 49..56 class, gpcc_primitives.hpp)
  __shared__ long long ws[4], wm[4];
  const size_t base = (size_t)blockIdx.x * kSymScanBlock;
  long long run = sums[blockIdx.x], runm = b ? maxs[blockIdx.x] : -1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = 0; k < kSymScanBlock / 256; k++) {
    const size_t i = base + (size_t)k * 256 + threadIdx.x;
    const long long v = i < n ? (long long)a[i] : 0;
    const long long vm = (b && i < n) ? (long long)b[i] : -1;
    long long inc = v, incm = vm;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long o = __shfl_up(inc, d);
      const long long om = __shfl_up(incm, d);
      if (lane >= d) {
        inc += o;
        incm = om > incm ? om : incm;
      }
    }
    long long exm = __shfl_up(incm, 1);
    if (lane == 0)
      exm = -1;
    __syncthreads();  // (ws / wm of the previous turn have been read)
    if (lane == 63) {
      ws[wave] = inc;
      wm[wave] = incm;
    }
    __syncthreads();
    long long off = run, offm = runm > exm ? runm : exm;
    for (int w = 0; w < wave; w++) {
      off += ws[w];
      offm = wm[w] > offm ? wm[w] : offm;
    }
    // entry i in front of which `off` has been summed; the total behind the last entry
    if (i < n) {
      out_sum[i] = off + inc - v;
      if (b)
        out_max[i] = offm;
      if (i == n - 1) {
        out_sum[n] = off + inc;
        if (b)
          out_max[n] = vm > offm ? vm : offm;
      }
    }
    run += ws[0] + ws[1] + ws[2] + ws[3];
    for (int w = 0; w < 4; w++)
      runm = wm[w] > runm ? wm[w] : runm;
  }
}

// a: [n] entries, n >= 1; b: nullptr or [n]; sums / maxs: sym_scan_blocks(n) words; out_*: [n + 1]
template<class In>
inline hipError_t
sym_scan(
  hipStream_t st, const In* a, const int32_t* b, size_t n, long long* sums, long long* maxs, long long* out_sum,
  long long* out_max)
{
  const int nblk = (int)((n + kSymScanBlock - 1) / kSymScanBlock);
  hipLaunchKernelGGL(sym_scan_sums_kernel<In>, dim3(nblk), dim3(256), 0, st, a, b, n, sums, maxs);
  hipLaunchKernelGGL(sym_scan_blocks_kernel, dim3(1), dim3(1024), 0, st, sums, b ? maxs : (long long*)nullptr, nblk);
  hipLaunchKernelGGL(
    sym_scan_apply_kernel<In>, dim3(nblk), dim3(256), 0, st, a, b, n, (const long long*)sums, (const long long*)maxs,
    out_sum, out_max);
  return hipGetLastError();
}

// ---- coefficients to symbols and bins ----------------------------------------------------------------------------

// the tile of this workgroup
struct SymTile {
  int s;             // slice
  int64_t b;         // the slice's first point in the batch
  int32_t n;         // points of the slice
  int32_t first;     // the tile's first position in the slice
  bool last_tile;    // of the slice
};

__device__ __forceinline__ SymTile
sym_tile(const int32_t* __restrict__ pt_off, const int32_t* __restrict__ tile_off, int num_slices, int t)
{
  SymTile r;
  r.s = rpl_slice_of_tile(tile_off, num_slices, t);
  r.b = pt_off[r.s];
  r.n = pt_off[r.s + 1] - pt_off[r.s];
  r.first = (t - tile_off[r.s]) * kSymTile;
  r.last_tile = t + 1 == tile_off[r.s + 1];
  return r;
}

// component j of position p of the slice
__device__ __forceinline__ int32_t
sym_coeff(const SymArgs& a, const SymTile& ti, int32_t p, int j)
{
  const int64_t at = a.planar ? (int64_t)j * ti.n + p : (int64_t)a.c * p + j;
  return a.coeffs[(int64_t)a.c * ti.b + at];
}

// grid: num_tiles workgroups
__global__ __launch_bounds__(kSymBlock) void
sym_tile_summary_kernel(SymArgs a)
{
  __shared__ unsigned long long words[kSymWords];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x;
  const SymTile ti = sym_tile(a.pt_off, a.tile_off, a.num_slices, t);
  for (int k = 0; k < 4; k++) {
    const int32_t p = ti.first + wave * 256 + k * 64 + lane;
    bool coded = false;
    if (p < ti.n)
      for (int j = 0; j < a.c; j++)
        coded = coded || sym_coeff(a, ti, p, j) != 0;
    const unsigned long long m = __ballot(coded);
    if (lane == 0)
      words[wave * 4 + k] = m;
  }
  __syncthreads();
  if (tid < kSymWords)
    a.mask[(size_t)t * kSymWords + tid] = words[tid];
  if (tid == 0) {
    int cnt = 0, last = -1;
    for (int w = 0; w < kSymWords; w++) {
      cnt += __popcll(words[w]);
      if (words[w])
        last = w * 64 + 63 - __clzll((long long)words[w]);
    }
    a.tile_cnt[t] = cnt;
    a.tile_last[t] = last < 0 ? -1 : (int32_t)(ti.b + ti.first + last);
  }
}

// What a coded position needs of its tile, from the tile's mask words (the same for every lane of a row): the coded
// positions in front of the row and the last of them (position in the tile, -1: none).
__device__ __forceinline__ void
sym_row_front(const unsigned long long* __restrict__ words, int row, int* before, int* last)
{
  int cnt = 0, l = -1;
  for (int w = 0; w < row; w++) {
    const unsigned long long m = words[w];
    cnt += __popcll(m);
    if (m)
      l = w * 64 + 63 - __clzll((long long)m);
  }
  *before = cnt;
  *last = l;
}

// the last coded position of the slice in front of tile t (position in the slice, -1: none)
__device__ __forceinline__ int32_t
sym_carry(const SymArgs& a, const SymTile& ti, int t)
{
  const long long g = a.prev[t];
  return g < ti.b ? -1 : (int32_t)(g - ti.b);
}

// The symbol of the coded position `lane` of row `row`: its run, its values, its rank among the tile's symbols.
__device__ __forceinline__ void
sym_symbol(
  const SymArgs& a, const SymTile& ti, const unsigned long long* __restrict__ words, int row, int lane, int32_t carry,
  int32_t* run, int32_t* v, int* rank)
{
  int before, last;
  sym_row_front(words, row, &before, &last);
  const unsigned long long below = words[row] & ((1ull << lane) - 1);
  const int in_tile = row * 64 + lane;
  int32_t prev;  // position in the slice
  if (below)
    prev = ti.first + row * 64 + 63 - __clzll((long long)below);
  else
    prev = last >= 0 ? ti.first + last : carry;
  *run = ti.first + in_tile - prev - 1;
  *rank = before + __popcll(below);
  for (int j = 0; j < a.c; j++)
    v[j] = sym_coeff(a, ti, ti.first + in_tile, j);
}

__device__ __forceinline__ int
sym_bins_of(int32_t run, const int32_t* v, int c)
{
  BinSink s{nullptr, 0};
  bins_run_length(s, run);
  bins_values(s, v, c);
  return s.n;
}

// the trailing run of the slice whose last tile this is: behind the tile's last coded position, or behind the
// carry when the tile has none
__device__ __forceinline__ int32_t
sym_trailing(const SymTile& ti, const unsigned long long* __restrict__ words, int32_t carry)
{
  int before, last;
  sym_row_front(words, kSymWords, &before, &last);
  const int32_t l = last >= 0 ? ti.first + last : carry;
  return ti.n - 1 - l;
}

// grid: num_tiles workgroups
__global__ __launch_bounds__(kSymBlock) void
sym_count_kernel(SymArgs a)
{
  __shared__ int wsum[kSymBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x;
  const SymTile ti = sym_tile(a.pt_off, a.tile_off, a.num_slices, t);
  const unsigned long long* words = a.mask + (size_t)t * kSymWords;
  const int32_t carry = sym_carry(a, ti, t);
  // the slice's symbols in front of the tile
  const int64_t base = a.sym_base[t] - a.sym_base[a.tile_off[ti.s]];
  int sum = 0;
  for (int k = 0; k < 4; k++) {
    const int row = wave * 4 + k;
    if (!((words[row] >> lane) & 1))
      continue;
    int32_t run, v[3];
    int rank;
    sym_symbol(a, ti, words, row, lane, carry, &run, v, &rank);
    if (a.runs) {
      const int64_t at = base + rank;
      a.runs[ti.b + at] = run;
      for (int j = 0; j < a.c; j++)
        a.values[a.c * (ti.b + at) + j] = v[j];
    }
    sum += sym_bins_of(run, v, a.c);
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
    sum += __shfl_xor(sum, d);
  if (lane == 0)
    wsum[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (ti.last_tile) {
      const int32_t trailing = sym_trailing(ti, words, carry);
      if (trailing > 0) {
        BinSink s{nullptr, 0};
        bins_run_length(s, trailing);
        total += s.n;
      }
    }
    a.tile_bins[t] = total;
  }
}

// what the host reads: grid over the slices
__global__ __launch_bounds__(256) void
sym_slices_kernel(SymArgs a)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > a.num_slices)
    return;
  const int t0 = a.tile_off[s];  // (tile_off[num_slices] == num_tiles: the total)
  a.bin_offsets[s] = a.bin_base[t0];
  if (s == a.num_slices)
    return;
  const int t1 = a.tile_off[s + 1];
  a.num_symbols[s] = (int32_t)(a.sym_base[t1] - a.sym_base[t0]);
  // the last coded position in front of the next slice's first tile: this slice's, if it has one
  const long long g = a.prev[t1];
  const int32_t b = a.pt_off[s], e = a.pt_off[s + 1];
  a.trailing_run[s] = g < b ? e - b : (int32_t)(e - 1 - g);
}

// grid: num_tiles workgroups
__global__ __launch_bounds__(kSymBlock) void
sym_emit_kernel(SymArgs a)
{
  __shared__ int wsum[kSymBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x;
  const long long out0 = a.bin_base[t], out1 = a.bin_base[t + 1];
  if (out0 == out1)
    return;  // (nothing of this tile is coded and no trailing run ends here: uniform over the workgroup)
  const SymTile ti = sym_tile(a.pt_off, a.tile_off, a.num_slices, t);
  const unsigned long long* words = a.mask + (size_t)t * kSymWords;
  const int32_t carry = sym_carry(a, ti, t);
  int32_t run[4], v[4][3];
  int cnt[4], off[4];
  int mine = 0;  // this wavefront's decisions in front of the row, then of the whole wavefront
  for (int k = 0; k < 4; k++) {
    const int row = wave * 4 + k;
    cnt[k] = 0;
    if ((words[row] >> lane) & 1) {
      int rank;
      sym_symbol(a, ti, words, row, lane, carry, &run[k], v[k], &rank);
      cnt[k] = sym_bins_of(run[k], v[k], a.c);
    }
    int inc = cnt[k];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d)
        inc += o;
    }
    off[k] = mine + inc - cnt[k];
    mine += __shfl(inc, 63);
  }
  if (lane == 0)
    wsum[wave] = mine;
  __syncthreads();
  long long at = out0;
  for (int w = 0; w < wave; w++)
    at += wsum[w];
  for (int k = 0; k < 4; k++) {
    if (!cnt[k])
      continue;
    BinSink s{a.bins + at + off[k], 0};
    bins_run_length(s, run[k]);
    bins_values(s, v[k], a.c);
  }
  if (tid == 0 && ti.last_tile) {
    const int32_t trailing = sym_trailing(ti, words, carry);
    if (trailing > 0) {
      BinSink n{nullptr, 0};
      bins_run_length(n, trailing);
      BinSink s{a.bins + out1 - n.n, 0};
      bins_run_length(s, trailing);
    }
  }
}

// The launches in front of the host's one wait.  span(name): an object that lives as long as the launch it names
// (the library's per-kernel timer).
template<class Span>
inline hipError_t
sym_count_launch(hipStream_t st, const SymArgs& a, Span&& span)
{
  const size_t nt = (size_t)a.num_tiles;
  {
    auto t = span("sym_tile_summary");
    hipLaunchKernelGGL(sym_tile_summary_kernel, dim3(a.num_tiles), dim3(kSymBlock), 0, st, a);
  }
  {
    auto t = span("sym_tile_scan");
    hipError_t e = sym_scan<int32_t>(
      st, (const int32_t*)a.tile_cnt, (const int32_t*)a.tile_last, nt, a.scan_sums, a.scan_maxs, a.sym_base, a.prev);
    if (e != hipSuccess)
      return e;
  }
  {
    auto t = span("sym_count");
    hipLaunchKernelGGL(sym_count_kernel, dim3(a.num_tiles), dim3(kSymBlock), 0, st, a);
  }
  {
    auto t = span("sym_bin_scan");
    hipError_t e = sym_scan<int32_t>(
      st, (const int32_t*)a.tile_bins, (const int32_t*)nullptr, nt, a.scan_sums, a.scan_maxs, a.bin_base,
      (long long*)nullptr);
    if (e != hipSuccess)
      return e;
  }
  {
    auto t = span("sym_slices");
    hipLaunchKernelGGL(sym_slices_kernel, dim3(a.num_slices / 256 + 1), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

template<class Span>
inline hipError_t
sym_emit_launch(hipStream_t st, const SymArgs& a, Span&& span)
{
  auto t = span("sym_emit");
  hipLaunchKernelGGL(sym_emit_kernel, dim3(a.num_tiles), dim3(kSymBlock), 0, st, a);
  return hipGetLastError();
}

// ---- symbols to coefficients -------------------------------------------------------------------------------------

// what a symbol adds to the position; a negative run is an error, counted as no run
__device__ __forceinline__ long long
sym_step(int32_t run)
{
  return run < 0 ? 1 : (long long)run + 1;
}

// grid: num_tiles workgroups; thread i of a tile owns its symbols 4 i .. 4 i + 3
__global__ __launch_bounds__(kSymBlock) void
sym_unpack_sums_kernel(SymUnpackArgs a)
{
  __shared__ long long ws[kSymBlock / 64];
  const int tid = threadIdx.x;
  const int t = blockIdx.x;
  const int s = rpl_slice_of_tile(a.tile_off, a.num_slices, t);
  const int64_t first = (int64_t)a.sym_off[s] + (int64_t)(t - a.tile_off[s]) * kSymTile, end = a.sym_off[s + 1];
  long long sum = 0;
  bool bad = false;
  for (int k = 0; k < 4; k++) {
    const int64_t g = first + 4 * tid + k;
    if (g < end) {
      const int32_t run = a.runs[g];
      bad = bad || run < 0;
      sum += sym_step(run);
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
    sum += __shfl_xor(sum, d);
  if ((tid & 63) == 0)
    ws[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0)
    a.tile_sum[t] = ws[0] + ws[1] + ws[2] + ws[3];
  if (bad)
    atomicCAS(a.error, 0, kSymUnpackErrorRange);
}

// grid: num_tiles workgroups
__global__ __launch_bounds__(kSymBlock) void
sym_unpack_scatter_kernel(SymUnpackArgs a)
{
  __shared__ long long ws[kSymBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x;
  const int s = rpl_slice_of_tile(a.tile_off, a.num_slices, t);
  const int64_t first = (int64_t)a.sym_off[s] + (int64_t)(t - a.tile_off[s]) * kSymTile, end = a.sym_off[s + 1];
  const int64_t b = a.pt_off[s];
  const int64_t n = a.pt_off[s + 1] - b;
  int32_t run[4];
  long long mine = 0;
  for (int k = 0; k < 4; k++) {
    const int64_t g = first + 4 * tid + k;
    run[k] = g < end ? a.runs[g] : 0;
    mine += g < end ? sym_step(run[k]) : 0;
  }
  long long inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl_up(inc, d);
    if (lane >= d)
      inc += o;
  }
  if (lane == 63)
    ws[wave] = inc;
  __syncthreads();
  // the steps of the slice in front of this thread's symbols
  long long at = a.tile_base[t] - a.tile_base[a.tile_off[s]] + inc - mine;
  for (int w = 0; w < wave; w++)
    at += ws[w];
  bool bad = false;
  for (int k = 0; k < 4; k++) {
    const int64_t g = first + 4 * tid + k;
    if (g >= end)
      break;
    at += sym_step(run[k]);
    const long long p = at - 1;
    if (run[k] < 0 || p >= n) {
      bad = true;
      continue;
    }
    for (int j = 0; j < a.c; j++) {
      const int64_t o = a.planar ? (int64_t)j * n + p : (int64_t)a.c * p + j;
      a.coeffs[a.c * b + o] = a.values[a.c * g + j];
    }
  }
  if (bad)
    atomicCAS(a.error, 0, kSymUnpackErrorRange);
}

// words: the int32 of the batch's coefficients (c times its points).  Nothing is waited for.
template<class Span>
inline hipError_t
sym_unpack_launch(hipStream_t st, const SymUnpackArgs& a, int64_t words, Span&& span)
{
  {
    auto t = span("sym_unpack_clear");
    hipError_t e = hipMemsetAsync(a.coeffs, 0, sizeof(int32_t) * (size_t)words, st);
    if (e != hipSuccess)
      return e;
  }
  if (a.num_tiles == 0)
    return hipSuccess;  // (no slice has a symbol)
  {
    auto t = span("sym_unpack_sums");
    hipLaunchKernelGGL(sym_unpack_sums_kernel, dim3(a.num_tiles), dim3(kSymBlock), 0, st, a);
  }
  {
    auto t = span("sym_unpack_scan");
    hipError_t e = sym_scan<long long>(
      st, (const long long*)a.tile_sum, (const int32_t*)nullptr, (size_t)a.num_tiles, a.scan_sums, (long long*)nullptr,
      a.tile_base, (long long*)nullptr);
    if (e != hipSuccess)
      return e;
  }
  {
    auto t = span("sym_unpack_scatter");
    hipLaunchKernelGGL(sym_unpack_scatter_kernel, dim3(a.num_tiles), dim3(kSymBlock), 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace gpcc
