// slice_rdo.hpp -- the slice-level inter / intra decision of the reflectance coders
// (attrInterIntraSliceRDO, AttributeEncoder.cpp:501-585): the distortion estimate of each
// candidate,
//   distEstimate = sum over the points of |reconstructed - original|
// (AttributeEncoder.cpp:825-827 predicting, :1645-1646 lifting), and the re-addressing of the
// neighbours that live in the reference frame, which lets the inter candidate's structure stay
// on the device between gpcc's LoD build and its transforms.
//
// The reference accumulates the sum in a double that only ever receives integers: below 2^53 it
// is exact and independent of the order (2^29 points x 2^16 = 2^45).  The sum here is an int64,
// so the result does not depend on how the workgroups are scheduled either.
//
// Launches are written with hipLaunchKernelGGL and the HIP runtime calls are plain, so that
// the header also compiles for the CPU wavefront emulator (tests/emu).
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace gpcc {

// one 16-byte load of four attributes (the arrays the kernel reads are 16-byte aligned:
// carved from the arena in 256-byte units)
struct alignas(16) RdoQuad {
  int32_t v[4];
};

struct SliceDistArgs {
  const int32_t* rec[2];    // [n] each candidate's clipped reconstruction, point order
  const int32_t* orig;      // [n] the source attributes, shared by the candidates
  unsigned long long* out;  // [num] one sum per candidate, cleared by the caller
  int32_t n;
  int32_t num;  // candidates: 1 or 2
};

constexpr int kSliceDistBlock = 256;
// workgroups: enough to keep every CU's memory pipeline busy (256 CUs x 8), never more than
// there are 16-byte loads for
inline int
slice_distortion_grid(int64_t n)
{
  const int64_t quads = (n + 3) / 4;
  const int64_t g = (quads + kSliceDistBlock - 1) / kSliceDistBlock;
  return (int)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}

__device__ __forceinline__ long long
rdo_abs_diff(int32_t a, int32_t b)
{
  const long long d = (long long)a - (long long)b;
  return d < 0 ? -d : d;
}

// Streaming: a grid-stride loop over 16-byte loads (the last n % 4 values by the first lanes
// of workgroup 0), a butterfly over the 64 lanes of the wavefront, one LDS word per wavefront
// and candidate, one device-scope 64-bit atomic add per workgroup and candidate.  No workgroup
// waits for another.
__global__ __launch_bounds__(kSliceDistBlock) void
slice_distortion_kernel(SliceDistArgs a)
{
  __shared__ long long wave_sum[2][kSliceDistBlock / 64];
  const int tid = threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kSliceDistBlock;
  const int64_t quads = a.n >> 2;
  long long acc[2] = {0, 0};
  const RdoQuad* o4 = reinterpret_cast<const RdoQuad*>(a.orig);
  const RdoQuad* r4[2] = {
    reinterpret_cast<const RdoQuad*>(a.rec[0]), reinterpret_cast<const RdoQuad*>(a.rec[a.num > 1 ? 1 : 0])};
  for (int64_t q = (int64_t)blockIdx.x * kSliceDistBlock + tid; q < quads; q += stride) {
    const RdoQuad o = o4[q];
    const RdoQuad x = r4[0][q];
    acc[0] += rdo_abs_diff(x.v[0], o.v[0]) + rdo_abs_diff(x.v[1], o.v[1]) + rdo_abs_diff(x.v[2], o.v[2])
      + rdo_abs_diff(x.v[3], o.v[3]);
    if (a.num > 1) {
      const RdoQuad y = r4[1][q];
      acc[1] += rdo_abs_diff(y.v[0], o.v[0]) + rdo_abs_diff(y.v[1], o.v[1]) + rdo_abs_diff(y.v[2], o.v[2])
        + rdo_abs_diff(y.v[3], o.v[3]);
    }
  }
  if (blockIdx.x == 0) {
    const int64_t i = (quads << 2) + tid;
    if (tid < 4 && i < a.n) {
      acc[0] += rdo_abs_diff(a.rec[0][i], a.orig[i]);
      if (a.num > 1)
        acc[1] += rdo_abs_diff(a.rec[1][i], a.orig[i]);
    }
  }
  // (every lane of the workgroup is here: the collectives below are convergent)
  for (int k = 0; k < 2; k++) {
    long long s = acc[k];
    for (int m = 32; m >= 1; m >>= 1)
      s += __shfl_xor(s, m, 64);
    if ((tid & 63) == 0)
      wave_sum[k][tid >> 6] = s;
  }
  __syncthreads();
  if (tid < a.num) {
    long long s = 0;
    for (int w = 0; w < kSliceDistBlock / 64; w++)
      s += wave_sum[tid][w];
    if (s)
      atomicAdd(a.out + tid, (unsigned long long)s);
  }
}

// The inter candidate's structure as the transforms read it: a neighbour that lives in the
// reference frame is addressed BEHIND the n predictors (launch_lift / launch_pred: entry n + r
// holds the frame's attribute r).  gpcc_lod_build_inter hands out the frame's own index and the
// flag; the host entries add n on the host (frame_neighbours_behind), this does it where the
// structure is.
__global__ __launch_bounds__(256) void
rdo_frame_neighbours_kernel(
  int32_t n, const int32_t* __restrict__ count, const int32_t* __restrict__ inter_ref,
  const int32_t* __restrict__ neigh_index, int32_t* __restrict__ out)
{
  const int64_t total = (int64_t)n * 3;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)(t / 3), j = (int32_t)(t - (int64_t)i * 3);
    const int32_t v = neigh_index[t];
    out[t] = (j < count[i] && inter_ref[t]) ? v + n : v;
  }
}

}  // namespace gpcc
