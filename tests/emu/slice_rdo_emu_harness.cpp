// tests/emu/slice_rdo_emu_harness.cpp -- TEST INFRASTRUCTURE: slice_distortion_kernel and
// rdo_frame_neighbours_kernel (slice_rdo.hpp) under the CPU wavefront emulator, launched as
// rdo_attr_driver (gpcc_attr_mi355.hip) launches them.
#include <stdlib.h>
#include <string.h>

#include "hip/hip_runtime.h"

#include "slice_rdo.hpp"

using namespace gpcc;

namespace {
// the library hands the kernel arrays carved in 256-byte units
int32_t*
aligned_copy(const int32_t* src, size_t n)
{
  const size_t bytes = (sizeof(int32_t) * (n ? n : 1) + 255) & ~size_t(255);
  int32_t* p = (int32_t*)aligned_alloc(256, bytes);
  memset(p, 0xCD, bytes);
  if (src)
    memcpy(p, src, sizeof(int32_t) * n);
  return p;
}
}  // namespace

// rec [num][n], orig [n] -> out [num]; grid <= 0: the library's choice
extern "C" int
slice_distortion_emu(const int32_t* rec, const int32_t* orig, int32_t n, int32_t num, int32_t grid, int64_t* out)
{
  if (n <= 0 || num < 1 || num > 2)
    return -1;
  int32_t* d_rec[2] = {aligned_copy(rec, n), num > 1 ? aligned_copy(rec + n, n) : nullptr};
  int32_t* d_orig = aligned_copy(orig, n);
  unsigned long long sums[2] = {0, 0};
  SliceDistArgs a{};
  a.rec[0] = d_rec[0];
  a.rec[1] = d_rec[1];
  a.orig = d_orig;
  a.out = sums;
  a.n = n;
  a.num = num;
  hipLaunchKernelGGL(
    slice_distortion_kernel, dim3(grid > 0 ? grid : slice_distortion_grid(n)), dim3(kSliceDistBlock), 0, nullptr, a);
  for (int k = 0; k < num; k++)
    out[k] = (int64_t)sums[k];
  free(d_rec[0]);
  free(d_rec[1]);
  free(d_orig);
  return 0;
}

extern "C" int
rdo_frame_neighbours_emu(
  int32_t n, const int32_t* count, const int32_t* inter_ref, const int32_t* neigh_index, int32_t* out)
{
  if (n <= 0)
    return -1;
  hipLaunchKernelGGL(
    rdo_frame_neighbours_kernel, dim3((3 * n + 255) / 256), dim3(256), 0, nullptr, n, count, inter_ref, neigh_index, out);
  return 0;
}
