// ref_crop.hpp -- the reference frame of an inter-predicted LoD slice: what the reference does to the previous
// frame in front of the lifting and predicting coders (encoder.cpp:1215-1236, decoder.cpp:926-947):
//   computeBoundingBox of the current slice's attribute-domain positions (PCCPointCloud.h),
//   Box3::contains (PCCMath.h:469-474, inclusive on all six faces) over the whole previous frame,
//   the points inside appended in order, with their attributes: an ordered (stable) compaction.
//
// For a batch of slices against one frame, the cropped frames back to back:
//   slice_bbox        rpl_convert_kernel<false> of spherical.hpp: tiles of 1 024 points that never straddle a
//                     slice, a butterfly over the wavefront, six device-scope atomics per workgroup and slice
//   ref_crop_count    one workgroup per (slice, tile of the frame): the points of the tile inside the slice's
//                     box, by ballots; one count per (slice, tile)
//   scan              kd_scan (recolour_kdtree.hpp) over the counts of ALL slices, slice-major: the cropped
//                     frames lie back to back, so the scanned count of (slice, tile) is the tile's first output
//                     position and the scanned count of (slice, tile 0) is the slice's offset
//   ref_crop_offsets  the slices' offsets gathered for the host, which has to know the total before anything
//                     is written (the caller's capacity)
//   ref_crop_scatter  the flags again; the rank inside the wavefront from the ballots, the wavefronts' bases
//                     through LDS, the tile's base from the scan
// No atomic decides a position and no workgroup waits for another: the order is the contract.
//
// A frame coordinate or a slice's box outside [0, 2^21) -- what the Morton sort and the LoD build accept -- sets
// the context's sticky error word to kRefCropErrorRange.
//
// Launches are written with hipLaunchKernelGGL and the HIP runtime calls are plain, so that the header also
// compiles for the CPU wavefront emulator (tests/emu).
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "recolour_kdtree.hpp"
#include "spherical.hpp"

namespace gpcc {

constexpr int kRefCropBlock = 256;
constexpr int kRefCropTile = 1024;       // frame points per workgroup: one 48-byte group of four points per thread
constexpr int kRefCropErrorRange = 6;    // the sticky error word's code (check_device_error)
constexpr int32_t kRefCropPosLimit = 1 << 21;
constexpr int64_t kRefCropMaxPairs = (int64_t)1 << 27;  // (slice, tile) pairs of one call

struct RefCropArgs {
  const int32_t* xyz_frame;    // [n_frame][3]
  const int32_t* attrs_frame;  // [n_frame][c]
  const int32_t* bbox;         // [num_slices][6]: min, max of the current slices
  int32_t* counts;             // [num_slices * num_tiles + 1]; (slice, tile) at slice * num_tiles + tile + 1, [0] = 0
  int32_t* offsets;            // [num_slices + 1]
  int32_t* xyz_ref;            // out [offsets[num_slices]][3]
  int32_t* attrs_ref;          // out [offsets[num_slices]][c]
  int32_t* error;              // the context's sticky error word
  int32_t n_frame;
  int32_t c;
  int32_t num_slices;
  int32_t num_tiles;           // of the frame
};

inline int
ref_crop_tiles(int64_t n_frame)
{
  return (int)((n_frame + kRefCropTile - 1) / kRefCropTile);
}

// entries of RefCropArgs::counts, and of the scan's block sums
inline size_t
ref_crop_count_entries(int num_slices, int64_t n_frame)
{
  return (size_t)num_slices * ref_crop_tiles(n_frame) + 1;
}

inline size_t
ref_crop_sum_entries(int num_slices, int64_t n_frame)
{
  return ref_crop_count_entries(num_slices, n_frame) / kKdScanBlock + 2;
}

// The four points p0 .. p0 + 3 of the calling thread (p0 a multiple of four): three 16-byte loads where the whole
// group lies inside the frame and the array is 16-byte aligned, scalar loads otherwise.  Bit k of the result: point
// p0 + k exists and lies inside the box (inclusive on all six faces); *bad: a coordinate outside [0, 2^21).
__device__ __forceinline__ unsigned
ref_crop_flags(const int32_t* __restrict__ xyz, bool wide, int64_t p0, int64_t n, const int32_t* box, int32_t* v, bool* bad)
{
  unsigned have = 0;
  if (wide && p0 + 4 <= n) {
    const RplQuad* s4 = reinterpret_cast<const RplQuad*>(xyz) + 3 * (p0 >> 2);
    const RplQuad w0 = s4[0], w1 = s4[1], w2 = s4[2];
    for (int i = 0; i < 4; i++) {
      v[i] = w0.v[i];
      v[4 + i] = w1.v[i];
      v[8 + i] = w2.v[i];
    }
    have = 15;
  } else {
    for (int k = 0; k < 4; k++) {
      if (p0 + k >= n)
        continue;
      for (int j = 0; j < 3; j++)
        v[3 * k + j] = xyz[3 * (p0 + k) + j];
      have |= 1u << k;
    }
  }
  unsigned in = 0;
  for (int k = 0; k < 4; k++) {
    if (!((have >> k) & 1))
      continue;
    bool inside = true;
    for (int j = 0; j < 3; j++) {
      const int32_t x = v[3 * k + j];
      inside = inside && x >= box[j] && x <= box[3 + j];
      if (x < 0 || x >= kRefCropPosLimit)
        *bad = true;
    }
    in |= inside ? 1u << k : 0u;
  }
  return in;
}

// grid: num_slices * num_tiles workgroups, slice-major
__global__ __launch_bounds__(kRefCropBlock) void
ref_crop_count_kernel(RefCropArgs a)
{
  __shared__ int32_t wave_cnt[kRefCropBlock / 64];
  const int tid = threadIdx.x;
  const int s = (int)(blockIdx.x / (unsigned)a.num_tiles), t = (int)(blockIdx.x % (unsigned)a.num_tiles);
  int32_t box[6];
  bool bad = false;
  for (int k = 0; k < 6; k++)
    box[k] = a.bbox[6 * s + k];
  if (t == 0)
    for (int k = 0; k < 3; k++)
      bad = bad || box[k] < 0 || box[3 + k] >= kRefCropPosLimit;
  int32_t v[12];
  bool bad_frame = false;
  const unsigned in = ref_crop_flags(
    a.xyz_frame, rpl_wide(a.xyz_frame, a.xyz_frame), (int64_t)t * kRefCropTile + 4 * tid, a.n_frame, box, v, &bad_frame);
  int cnt = 0;
  for (int k = 0; k < 4; k++)
    cnt += __popcll(__ballot((in >> k) & 1));
  if ((tid & 63) == 0)
    wave_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int sum = 0;
    for (int w = 0; w < kRefCropBlock / 64; w++)
      sum += wave_cnt[w];
    a.counts[(size_t)blockIdx.x + 1] = sum;
    if (blockIdx.x == 0)
      a.counts[0] = 0;
  }
  // (the frame is the same for every slice: the first one reports it; a slice's box by one thread)
  if ((bad && tid == 0) || (s == 0 && bad_frame))
    atomicCAS(a.error, 0, kRefCropErrorRange);
}

__global__ __launch_bounds__(256) void
ref_crop_offsets_kernel(RefCropArgs a)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= a.num_slices)
    a.offsets[s] = a.counts[(size_t)s * a.num_tiles];
}

// counts: scanned (inclusive over the shifted array, i.e. exclusive per pair)
__global__ __launch_bounds__(kRefCropBlock) void
ref_crop_scatter_kernel(RefCropArgs a)
{
  __shared__ int32_t wave_cnt[kRefCropBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = (int)(blockIdx.x / (unsigned)a.num_tiles), t = (int)(blockIdx.x % (unsigned)a.num_tiles);
  const int32_t base = a.counts[blockIdx.x];
  if (a.counts[(size_t)blockIdx.x + 1] == base)
    return;  // (nothing of this tile is kept: uniform over the workgroup)
  int32_t box[6];
  for (int k = 0; k < 6; k++)
    box[k] = a.bbox[6 * s + k];
  int32_t v[12];
  bool bad = false;
  const int64_t p0 = (int64_t)t * kRefCropTile + 4 * tid;
  const unsigned in = ref_crop_flags(a.xyz_frame, rpl_wide(a.xyz_frame, a.xyz_frame), p0, a.n_frame, box, v, &bad);
  const unsigned long long below = (1ull << lane) - 1;
  int cnt = 0, before = 0;
  for (int k = 0; k < 4; k++) {
    const unsigned long long m = __ballot((in >> k) & 1);
    cnt += __popcll(m);
    before += __popcll(m & below);
  }
  if (lane == 0)
    wave_cnt[wave] = cnt;
  __syncthreads();
  int64_t at = (int64_t)base + before;
  for (int w = 0; w < wave; w++)
    at += wave_cnt[w];
  for (int k = 0; k < 4; k++) {
    if (!((in >> k) & 1))
      continue;
    for (int j = 0; j < 3; j++)
      a.xyz_ref[3 * at + j] = v[3 * k + j];
    for (int j = 0; j < a.c; j++)
      a.attrs_ref[a.c * at + j] = a.attrs_frame[(int64_t)a.c * (p0 + k) + j];
    at++;
  }
}

// A reference frame that is already on the device, in front of the LoD build: any coordinate outside [0, 2^21)
// sets the sticky error word (the host tier checks the same in a loop over the caller's array).  xyz is the build's
// own copy of the frame: such a coordinate is replaced there, so that no kernel behind this one meets a value the
// host tier would have refused.
__global__ __launch_bounds__(256) void
ref_frame_range_kernel(int32_t* __restrict__ xyz, int64_t words, int32_t* error)
{
  // (the library caps its grids: a grid-stride loop)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x)
    if (xyz[i] < 0 || xyz[i] >= kRefCropPosLimit) {
      xyz[i] = 0;
      atomicCAS(error, 0, kRefCropErrorRange);
    }
}

// ... and its attributes for the lifting coder: int32 to fixed point (<< kFixedPointAttributeShift), written behind
// the coder's n working values
__global__ __launch_bounds__(256) void
frame_stage_lift_kernel(const int32_t* __restrict__ attrs, int64_t count, int64_t* __restrict__ a)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x)
    a[i] = (int64_t)attrs[i] * 256;
}

// The launches in front of the host's one wait: the current slices' boxes into `bbox`, the counts, their scan
// and a.offsets.  slices: the RplArgs of the current slices (src, pt_off, tile_off, num_slices, num_tiles);
// sums: ref_crop_sum_entries() words for the scan.  span(name): an object that lives as long as the launch it
// names (the library's per-kernel timer).
template<class Span>
inline hipError_t
ref_crop_count_launch(hipStream_t st, RplArgs slices, const RefCropArgs& a, long long* sums, Span&& span)
{
  slices.dst = const_cast<int32_t*>(slices.src);  // (never written: the kernel only takes the box)
  slices.bbox = const_cast<int32_t*>(a.bbox);
  slices.error = a.error;
  {
    auto t = span("rpl_bbox_init");
    hipLaunchKernelGGL(
      rpl_bbox_init_kernel, dim3((6 * a.num_slices + 255) / 256), dim3(256), 0, st, slices.bbox, a.num_slices);
  }
  {
    auto t = span("slice_bbox");
    hipLaunchKernelGGL(rpl_convert_kernel<false>, dim3(rpl_grid(slices.num_tiles)), dim3(kRplBlock), 0, st, slices);
  }
  const unsigned pairs = (unsigned)a.num_slices * (unsigned)a.num_tiles;
  {
    auto t = span("ref_crop_count");
    hipLaunchKernelGGL(ref_crop_count_kernel, dim3(pairs), dim3(kRefCropBlock), 0, st, a);
  }
  {
    auto t = span("ref_crop_scan");
    hipError_t e = kd_scan(st, a.counts, (size_t)pairs + 1, sums);
    if (e != hipSuccess)
      return e;
  }
  {
    auto t = span("ref_crop_offsets");
    hipLaunchKernelGGL(ref_crop_offsets_kernel, dim3(a.num_slices / 256 + 1), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

template<class Span>
inline hipError_t
ref_crop_scatter_launch(hipStream_t st, const RefCropArgs& a, Span&& span)
{
  auto t = span("ref_crop_scatter");
  hipLaunchKernelGGL(
    ref_crop_scatter_kernel, dim3((unsigned)a.num_slices * (unsigned)a.num_tiles), dim3(kRefCropBlock), 0, st, a);
  return hipGetLastError();
}

}  // namespace gpcc
