// spherical.hpp -- attribute positions in the pseudo-spherical domain (spherical_coord_flag):
// what the reference does to a slice's positions in front of attrEncoder->encode /
// _attrDecoder->decode (encoder.cpp:1148-1197, decoder.cpp:871-920):
//   convertXyzToRpl  (coordinate_conversion.cpp:44-69)  xyz -> (r, phi, laser) and their bounding box,
//   offsetAndScale   (coordinate_conversion.cpp:109-118) ((v - min) * attr_coord_scale + 128) >> 8,
// with findLaser (geometry_octree.cpp:856-872), isqrt and iatan2 (misc.cpp:139-147, :279-309).
//
// Two streaming kernels over the points of a batch of slices.  The first converts and reduces each
// slice's bounding box into a [num_slices][6] device array; the second reads the minimum from that
// array (or from the parameter block), so no host wait lies between them.
//
// Integer widths, as the reference has them, for the domain |x|, |y|, |z| < 2^22 after the laser
// origin has been subtracted:
//   * pos << 8 is an int shift there (below 2^30 in magnitude); the squares and their sum are 64-bit
//     (below 2^61);
//   * findLaser multiplies z by the reciprocal square root as int64 (below 2^54 in magnitude: the
//     reciprocal square root of a non-zero sum is at most 2^32), shifts by 14 and TRUNCATES to int;
//   * iatan2 takes the shifted values as int.
// One reciprocal square root of x^2 + y^2 serves findLaser, iatan2Core and the low branch of isqrt:
// the reference evaluates irsqrt three times with the same 64-bit argument there (iatan2Core squares
// the absolute values, in either order), so the bits are the same.  The high branch of isqrt
// (x^2 + y^2 > 2^46) takes the reciprocal square root of another argument and keeps its own.
//
// A point outside the domain, or a scaled coordinate outside [0, 2^21) -- what the Morton sort and the
// LoD build accept --, sets the context's sticky error word to kRplErrorDomain.
//
// Launches are written with hipLaunchKernelGGL and the HIP runtime calls are plain, so that the
// header also compiles for the CPU wavefront emulator (tests/emu).
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "gpcc_attr_mi355.h"
#include "gpcc_primitives.hpp"

namespace gpcc {

constexpr int kRplBlock = 256;
constexpr int kRplTile = 1024;      // points per tile: one 48-byte group of four points per thread
constexpr int kRplGridMax = 2048;   // 256 CUs x 8 workgroups
constexpr int kRplErrorDomain = 5;  // the sticky error word's code (check_device_error)
constexpr int32_t kRplPosLimit = 1 << 22;
constexpr int32_t kRplOutLimit = 1 << 21;

// one 16-byte word; four points are three of them
struct alignas(16) RplQuad {
  int32_t v[4];
};

// Tiles never straddle a slice: slice s owns the tiles tile_off[s] .. tile_off[s + 1] - 1, tile t of
// it the points pt_off[s] + (t - tile_off[s]) * kRplTile onwards.
struct RplArgs {
  const int32_t* src;       // [n][3]
  int32_t* dst;             // [n][3]; may be src
  int32_t* bbox;            // [num_slices][6]: min, max of the unscaled (r, phi, laser)
  const int32_t* pt_off;    // [num_slices + 1]
  const int32_t* tile_off;  // [num_slices + 1]
  int32_t* error;           // the context's sticky error word
  int32_t num_slices;
  int32_t num_tiles;
  int32_t origin[3];
  int32_t num_lasers;
  int32_t scale[3];
  int32_t min_pos_mode;
  int32_t min_pos[3];
  int32_t theta[GPCC_MAX_LASERS];
};

inline int
rpl_tiles(int64_t n)
{
  return (int)((n + kRplTile - 1) / kRplTile);
}

inline int
rpl_grid(int64_t num_tiles)
{
  return (int)(num_tiles < 1 ? 1 : num_tiles > kRplGridMax ? kRplGridMax : num_tiles);
}

// findLaser (geometry_octree.cpp:856-872) with rinv == irsqrt((x << 8)^2 + (y << 8)^2).
// std::upper_bound over theta[1 .. num - 2] as a bisection of at most log2(GPCC_MAX_LASERS) steps: `it`
// is the first entry of that range above theta32, or theta[num - 1] when there is none (and when the
// range is empty, num == 2); a tie between `it` and its predecessor picks the predecessor.
// The two differences wrap like the machine's int subtraction does.
GPCC_HD int
find_laser(int32_t z, uint64_t rinv, const int32_t* theta, int num)
{
  if (num == 1)
    return 0;
  const int32_t theta32 = (int32_t)(((int64_t)z * (int64_t)rinv) >> 14);
  int lo = 1, hi = num - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (theta[mid] > theta32)
      hi = mid;
    else
      lo = mid + 1;
  }
  const int32_t below = (int32_t)((uint32_t)theta32 - (uint32_t)theta[lo - 1]);
  const int32_t above = (int32_t)((uint32_t)theta[lo] - (uint32_t)theta32);
  return below <= above ? lo - 1 : lo;
}

// one point of convertXyzToRpl (coordinate_conversion.cpp:56-63); p: xyz in, (r, phi, laser) out.
// false: outside the domain (p is left as it was)
GPCC_HD bool
rpl_convert_point(
  int32_t* p, const int32_t* origin, const int32_t* theta, int num_lasers, const RsqrtLut& rs, const AsinLut& as)
{
  const int64_t x64 = (int64_t)p[0] - origin[0], y64 = (int64_t)p[1] - origin[1], z64 = (int64_t)p[2] - origin[2];
  if (x64 <= -kRplPosLimit || x64 >= kRplPosLimit || y64 <= -kRplPosLimit || y64 >= kRplPosLimit
      || z64 <= -kRplPosLimit || z64 >= kRplPosLimit)
    return false;
  const int32_t xl = (int32_t)x64 * 256, yl = (int32_t)y64 * 256;
  const uint64_t r2 = (uint64_t)((int64_t)xl * xl) + (uint64_t)((int64_t)yl * yl);
  const uint64_t rinv = irsqrt(r2, rs);
  const int laser = find_laser((int32_t)z64, rinv, theta, num_lasers);
  uint32_t r;
  if (r2 <= ((uint64_t)1 << 46)) {
    r = (uint32_t)(1 + ((r2 * rinv) >> 40));
  } else {
    const uint64_t x0 = (r2 + 65536) >> 16;
    r = (uint32_t)(1 + ((x0 * irsqrt(x0, rs)) >> 32));
  }
  p[0] = (int32_t)(r >> 8);
  p[1] = (iatan2(yl, xl, rinv, as) + 3294199) >> 8;
  p[2] = laser;
  return true;
}

// one coordinate of offsetAndScale (coordinate_conversion.cpp:116-117), the product in 64 bits
GPCC_HD int64_t
rpl_scale_coord(int32_t v, int32_t mn, int32_t scale)
{
  return (((int64_t)v - mn) * (int64_t)scale + 128) >> 8;
}

// the last slice whose first tile is not behind tile t
__device__ __forceinline__ int
rpl_slice_of_tile(const int32_t* __restrict__ tile_off, int num_slices, int t)
{
  int lo = 0, hi = num_slices - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_off[mid] <= t)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// The points [first, end) of a tile, four at a time where a whole 48-byte group lies inside the tile and
// the arrays are 16-byte aligned, one at a time at the tile's two edges and otherwise.  Groups are counted
// from the start of the ARRAY (a slice may begin at any point), so a group at the edge of a tile is shared
// with the neighbouring tile, each side handling its own points: every point is read and written by one
// thread only, which is what makes dst == src safe.
template<bool kStore, class Op>
__device__ __forceinline__ void
rpl_tile_points(const int32_t* src, int32_t* dst, bool wide, int64_t first, int64_t end, Op&& op)
{
  const int64_t g1 = (end - 1) >> 2;
  for (int64_t g = (first >> 2) + threadIdx.x; g <= g1; g += kRplBlock) {
    const int64_t p0 = g << 2;
    if (wide && p0 >= first && p0 + 4 <= end) {
      const RplQuad* s4 = reinterpret_cast<const RplQuad*>(src) + 3 * g;
      RplQuad w[3] = {s4[0], s4[1], s4[2]};
      int32_t* v = &w[0].v[0];  // (the three words are contiguous: 12 values, four points)
      for (int k = 0; k < 4; k++)
        op(v + 3 * k);
      if (kStore) {
        RplQuad* d4 = reinterpret_cast<RplQuad*>(dst) + 3 * g;
        d4[0] = w[0];
        d4[1] = w[1];
        d4[2] = w[2];
      }
    } else {
      for (int k = 0; k < 4; k++) {
        const int64_t p = p0 + k;
        if (p < first || p >= end)
          continue;
        int32_t v[3] = {src[3 * p], src[3 * p + 1], src[3 * p + 2]};
        op(v);
        if (kStore) {
          dst[3 * p] = v[0];
          dst[3 * p + 1] = v[1];
          dst[3 * p + 2] = v[2];
        }
      }
    }
  }
}

__device__ __forceinline__ bool
rpl_wide(const void* a, const void* b)
{
  return (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

__global__ __launch_bounds__(256) void
rpl_bbox_init_kernel(int32_t* bbox, int32_t num_slices)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 6 * num_slices)
    bbox[i] = i % 6 < 3 ? INT32_MAX : INT32_MIN;
}

// kConvert: xyz -> (r, phi, laser), written to dst, and the bounding box of the result;
// otherwise the input is spherical already (predictive geometry's own positions) and only its
// bounding box is taken.
// A workgroup walks its tiles in ascending order, so the tiles of a slice come together: the lanes keep
// their minima and maxima in registers until the slice changes, then a butterfly over the wavefront, one
// LDS word per wavefront and component, and six device-scope atomics per workgroup and slice.
template<bool kConvert>
__global__ __launch_bounds__(kRplBlock) void
rpl_convert_kernel(RplArgs a)
{
  __shared__ RsqrtLut rs;
  __shared__ AsinLut as;
  __shared__ int32_t theta[GPCC_MAX_LASERS];
  __shared__ int32_t wave_box[6][kRplBlock / 64];
  const int tid = threadIdx.x;
  if (kConvert) {
    constexpr uint16_t r3[96] = {GPCC_RSQRT_R3};
    constexpr uint32_t rc[96] = {GPCC_RSQRT_RC};
    constexpr uint32_t asin_lut[kAsinLutSize] = {GPCC_ASIN_LUT};
    for (int i = tid; i < 96; i += kRplBlock) {
      rs.r3[i] = r3[i];
      rs.rc[i] = rc[i];
    }
    for (int i = tid; i < kAsinLutSize; i += kRplBlock)
      as.v[i] = asin_lut[i];
    for (int i = tid; i < GPCC_MAX_LASERS; i += kRplBlock)
      theta[i] = a.theta[i < a.num_lasers ? i : a.num_lasers - 1];
    __syncthreads();
  }
  const bool wide = rpl_wide(a.src, a.dst);
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  bool bad = false;
  int cur = -1;
  auto flush = [&](int slice) {
    for (int k = 0; k < 3; k++) {
      int32_t mn = lo[k], mx = hi[k];
      for (int m = 32; m >= 1; m >>= 1) {
        const int32_t omn = __shfl_xor(mn, m, 64);
        const int32_t omx = __shfl_xor(mx, m, 64);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
      }
      if ((tid & 63) == 0) {
        wave_box[k][tid >> 6] = mn;
        wave_box[3 + k][tid >> 6] = mx;
      }
      lo[k] = INT32_MAX;
      hi[k] = INT32_MIN;
    }
    __syncthreads();
    if (tid < 6) {
      int32_t v = wave_box[tid][0];
      for (int w = 1; w < kRplBlock / 64; w++) {
        const int32_t o = wave_box[tid][w];
        v = (tid < 3 ? o < v : o > v) ? o : v;
      }
      if (tid < 3)
        atomicMin(a.bbox + 6 * slice + tid, v);
      else
        atomicMax(a.bbox + 6 * slice + tid, v);
    }
    __syncthreads();  // (wave_box is written again at the next change of slice)
  };
  // (every lane of the workgroup takes the same turns of this loop and the grid is never larger than the
  // number of tiles: the collectives and barriers of flush() are convergent)
  for (int t = blockIdx.x; t < a.num_tiles; t += gridDim.x) {
    const int s = rpl_slice_of_tile(a.tile_off, a.num_slices, t);
    if (cur >= 0 && s != cur)
      flush(cur);
    cur = s;
    const int64_t first = (int64_t)a.pt_off[s] + (int64_t)(t - a.tile_off[s]) * kRplTile;
    const int64_t last = first + kRplTile, slice_end = a.pt_off[s + 1];
    rpl_tile_points<kConvert>(a.src, a.dst, wide, first, last < slice_end ? last : slice_end, [&](int32_t* p) {
      if (kConvert && !rpl_convert_point(p, a.origin, theta, a.num_lasers, rs, as)) {
        bad = true;
        p[0] = p[1] = p[2] = 0;
      }
      for (int k = 0; k < 3; k++) {
        lo[k] = p[k] < lo[k] ? p[k] : lo[k];
        hi[k] = p[k] > hi[k] ? p[k] : hi[k];
      }
    });
  }
  if (cur >= 0)
    flush(cur);
  if (bad)
    atomicCAS(a.error, 0, kRplErrorDomain);
}

// offsetAndScale with the slice's minimum read where the first kernel left it (min_pos_mode 0), taken
// from the parameter block (1), or the smaller of the two per component (2)
__global__ __launch_bounds__(kRplBlock) void
rpl_scale_kernel(RplArgs a)
{
  const bool wide = rpl_wide(a.src, a.dst);
  bool bad = false;
  for (int t = blockIdx.x; t < a.num_tiles; t += gridDim.x) {
    const int s = rpl_slice_of_tile(a.tile_off, a.num_slices, t);
    int32_t mn[3];
    for (int k = 0; k < 3; k++) {
      const int32_t b = a.min_pos_mode == 1 ? a.min_pos[k] : a.bbox[6 * s + k];
      mn[k] = a.min_pos_mode == 2 && a.min_pos[k] < b ? a.min_pos[k] : b;
    }
    const int64_t first = (int64_t)a.pt_off[s] + (int64_t)(t - a.tile_off[s]) * kRplTile;
    const int64_t last = first + kRplTile, slice_end = a.pt_off[s + 1];
    rpl_tile_points<true>(a.src, a.dst, wide, first, last < slice_end ? last : slice_end, [&](int32_t* p) {
      for (int k = 0; k < 3; k++) {
        const int64_t v = rpl_scale_coord(p[k], mn[k], a.scale[k]);
        if (v < 0 || v >= kRplOutLimit)
          bad = true;
        p[k] = (int32_t)v;
      }
    });
  }
  if (bad)
    atomicCAS(a.error, 0, kRplErrorDomain);
}

// the three launches of a batch on `st`; a.src / a.dst as the caller gave them.  span(name): an object that
// lives as long as the launch it names (the library's per-kernel timer)
template<class Span>
inline hipError_t
rpl_launch(hipStream_t st, RplArgs a, bool convert, Span&& span)
{
  const dim3 grid(rpl_grid(a.num_tiles)), block(kRplBlock);
  {
    auto t = span("rpl_bbox_init");
    hipLaunchKernelGGL(
      rpl_bbox_init_kernel, dim3((6 * a.num_slices + 255) / 256), dim3(256), 0, st, a.bbox, a.num_slices);
  }
  {
    auto t = span(convert ? "rpl_convert" : "rpl_bbox");
    if (convert)
      hipLaunchKernelGGL(rpl_convert_kernel<true>, grid, block, 0, st, a);
    else
      hipLaunchKernelGGL(rpl_convert_kernel<false>, grid, block, 0, st, a);
  }
  if (convert)
    a.src = a.dst;  // (the unscaled result is what is offset and scaled)
  {
    auto t = span("rpl_scale");
    hipLaunchKernelGGL(rpl_scale_kernel, grid, block, 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace gpcc
