// raht_marshal.hpp -- the marshalling around the RAHT transform for a BATCH of slices resident in HBM: what
// encode/decode{Colors,Reflectances}TransformRaht do in front of and behind the transform (AttributeEncoder.cpp:
// 1331-1338 / 1364-1375, 1262 / 1336; AttributeDecoder.cpp:585 / 648, 600-609 / 663-674).
//
//   gather        attributes from point order into the order of the sorted Morton codes, and, for the slices that
//                 name QP regions, the two region offsets of every point (QpSet::regionQpOffset, quantization.cpp:
//                 195-204: the FIRST box that contains the point, bounds inclusive) formed on the spot from the
//                 point's own position -- no [n][2] array in point order, no second gather
//   clip-scatter  the reconstruction clipped to [0, clip_max] back to point order
//
// Both kernels walk the SORTED side, which is contiguous: thread e owns word e of the [n][C] array in sorted
// order, so a wave's accesses to it are 64 consecutive dwords.  The point-order side is the random one; the C
// words of a row are touched by C neighbouring lanes.  The slice of a sorted position comes from find_slice over
// the batch's offsets; the source row is base + order[i].  The slices' region blocks are a table in device
// memory (sizeof(gpcc_qp_regions) bytes per slice), never a kernel argument.
//
// The launch functions are what the library (gpcc_dev_raht_encode_attr / _decode_attr) and the emulator harness
// (tests/emu/raht_marshal_emu_harness.cpp) both call.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "gpcc_attr_mi355.h"
#include "raht_common.hpp"

namespace gpcc {

constexpr int kMarshalBlock = 256;
constexpr int kMarshalGridMax = 2048;  // 256 CUs x 8 workgroups of 256 threads

struct MarshalArgs {
  const int32_t* pt_off;           // [num_slices + 1] the batch's offsets
  const gpcc_qp_regions* regions;  // [num_slices] device table; null: no slice names a region
  const int32_t* order;            // [n] slice-local original index of the i-th sorted point
  const int32_t* xyz;              // [n][3] point order (read only where regions != null)
  int32_t* point;                  // [n][c] point order: the gather's source, the scatter's destination
  int32_t* sorted;                 // [n][c] sorted order: the gather's destination, the scatter's source
  int32_t* qp_off;                 // [n][2] sorted order, written by the gather where regions != null
  int32_t n, c, num_slices;
  int32_t clip_max;                // clip-scatter: 2^bitdepth - 1
  int32_t attrs;                   // gather: 0 = the region offsets only (the decoder)
};

inline int
marshal_grid(int64_t items)
{
  const int64_t g = (items + kMarshalBlock - 1) / kMarshalBlock;
  return (int)(g < 1 ? 1 : (g > kMarshalGridMax ? kMarshalGridMax : g));
}

// the offsets of the first box of `r` that holds (x, y, z); none: zero
__device__ __forceinline__ void
marshal_region_offset(const gpcc_qp_regions& r, int x, int y, int z, int32_t& o0, int32_t& o1)
{
  o0 = o1 = 0;
  const int nr = r.num_qp_regions < GPCC_MAX_QP_REGIONS ? r.num_qp_regions : GPCC_MAX_QP_REGIONS;
  for (int b = 0; b < nr; b++) {
    const bool in = !(x < r.qp_region_min[b][0] || x > r.qp_region_max[b][0] || y < r.qp_region_min[b][1]
                      || y > r.qp_region_max[b][1] || z < r.qp_region_min[b][2] || z > r.qp_region_max[b][2]);
    if (in) {
      o0 = r.qp_region_offset[b][0];
      o1 = r.qp_region_offset[b][1];
      return;
    }
  }
}

// C words per sorted position (C == 1 with a.attrs == 0: one thread per position, offsets only)
template<int C>
__global__ __launch_bounds__(kMarshalBlock) void
raht_gather_kernel(MarshalArgs a)
{
  const int64_t total = (int64_t)a.n * C;
  for (int64_t e = (int64_t)blockIdx.x * kMarshalBlock + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kMarshalBlock) {
    const int i = (int)(e / C), k = (int)(e - (int64_t)i * C);
    const int s = find_slice(a.pt_off, a.num_slices, i);
    const int64_t row = (int64_t)a.pt_off[s] + a.order[i];
    if (a.attrs)
      a.sorted[e] = a.point[row * C + k];
    if (k == 0 && a.regions) {
      int32_t o0, o1;
      marshal_region_offset(a.regions[s], a.xyz[3 * row], a.xyz[3 * row + 1], a.xyz[3 * row + 2], o0, o1);
      a.qp_off[2 * (int64_t)i] = o0;
      a.qp_off[2 * (int64_t)i + 1] = o1;
    }
  }
}

template<int C>
__global__ __launch_bounds__(kMarshalBlock) void
raht_clip_scatter_kernel(MarshalArgs a)
{
  const int64_t total = (int64_t)a.n * C;
  for (int64_t e = (int64_t)blockIdx.x * kMarshalBlock + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kMarshalBlock) {
    const int i = (int)(e / C), k = (int)(e - (int64_t)i * C);
    const int s = find_slice(a.pt_off, a.num_slices, i);
    const int64_t row = (int64_t)a.pt_off[s] + a.order[i];
    const int32_t v = a.sorted[e];
    a.point[row * C + k] = v < 0 ? 0 : (v > a.clip_max ? a.clip_max : v);
  }
}

// span(name): an object that lives as long as the launch it names (the library's per-kernel timer).
// One launch whatever num_slices is; none when there is nothing to do (a decoder without regions).
template<class Span>
inline hipError_t
raht_gather_launch(hipStream_t st, const MarshalArgs& a, Span&& span)
{
  if (!a.attrs && !a.regions)
    return hipSuccess;
  auto t = span("raht_gather");
  const int c = a.attrs ? a.c : 1;
  const dim3 grid(marshal_grid((int64_t)a.n * c)), block(kMarshalBlock);
  switch (c) {
  case 1:
    hipLaunchKernelGGL((raht_gather_kernel<1>), grid, block, 0, st, a);
    break;
  case 2:
    hipLaunchKernelGGL((raht_gather_kernel<2>), grid, block, 0, st, a);
    break;
  default:
    hipLaunchKernelGGL((raht_gather_kernel<3>), grid, block, 0, st, a);
    break;
  }
  return hipGetLastError();
}

template<class Span>
inline hipError_t
raht_clip_scatter_launch(hipStream_t st, const MarshalArgs& a, Span&& span)
{
  auto t = span("raht_clip_scatter");
  const dim3 grid(marshal_grid((int64_t)a.n * a.c)), block(kMarshalBlock);
  switch (a.c) {
  case 1:
    hipLaunchKernelGGL((raht_clip_scatter_kernel<1>), grid, block, 0, st, a);
    break;
  case 2:
    hipLaunchKernelGGL((raht_clip_scatter_kernel<2>), grid, block, 0, st, a);
    break;
  default:
    hipLaunchKernelGGL((raht_clip_scatter_kernel<3>), grid, block, 0, st, a);
    break;
  }
  return hipGetLastError();
}

}  // namespace gpcc
