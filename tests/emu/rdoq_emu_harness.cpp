// tests/emu/rdoq_emu_harness.cpp -- TEST INFRASTRUCTURE: rdoq_resolve_kernel (raht_rdoq.hpp) under the CPU wavefront
// emulator, driven as gpcc_debug_rdoq_resolve (gpcc_attr_mi355.hip) drives it on the device: the same plan
// (rdoq_probe_plan), the same start of state and slice_l, one launch per level from the top one down through
// rdoq_resolve_launch.  The threshold functions of raht_levels.hpp run through their probe kernel as well.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip/hip_runtime.h"

#include "raht_rdoq.hpp"

using namespace gpcc;

// Arguments of gpcc_debug_rdoq_resolve; *error is the word the kernel sets when a look-back wait expires.
// Returns -1 for arguments the plan refuses, -2 when a guard word around the coefficients has changed.
extern "C" int
rdoq_emu_resolve(
  int32_t num_slices, const int64_t* offsets, const int32_t* cut_off, const int32_t* cuts, const uint32_t* desc,
  int32_t c, int32_t* coeffs, int32_t* slice_l_out, int32_t* error)
{
  RdoqProbePlan pl;
  if (num_slices < 1 || c < 1 || c > 3 || !rdoq_probe_plan(offsets, num_slices, cut_off, cuts, &pl))
    return -1;
  const int s = num_slices;
  const size_t n = (size_t)offsets[s], row = (size_t)s + 1;
  const size_t guard = 64;
  std::vector<int32_t> co(n * c + 2 * guard, (int32_t)0xCDCDCDCD);
  memcpy(co.data() + guard, coeffs, n * c * sizeof(int32_t));
  std::vector<unsigned long long> state((size_t)pl.num_tiles + 1, 0);
  std::vector<int32_t> slice_l(s, -1);
  *error = 0;

  RdoqCtx rc{};
  rc.tv.nlev = pl.nlev + 1;
  rc.tv.num_slices = s;
  rc.tv.n_total = (int32_t)n;
  rc.tv.pt_off = pl.pt_off.data();
  for (int li = 0; li <= pl.nlev; li++)
    rc.tv.soff[li] = pl.soff.data() + (size_t)li * row;
  rc.tv.error = error;
  rc.sched = pl.sched.data();
  rc.tile_base = pl.tile_base.data();
  rc.num_tiles = pl.num_tiles;
  rc.desc = desc;
  rc.coeffs = co.data() + guard;
  rc.slice_l = slice_l.data();
  rc.state = state.data();
  rc.c = c;
  if (pl.num_tiles > 0)
    for (int li = pl.nlev - 1; li >= 0; li--) {
      rc.li = li;
      rdoq_resolve_launch(rc, nullptr);
    }
  for (size_t i = 0; i < guard; i++)
    if (co[i] != (int32_t)0xCDCDCDCD || co[guard + n * c + i] != (int32_t)0xCDCDCDCD)
      return -2;
  memcpy(coeffs, co.data() + guard, n * c * sizeof(int32_t));
  memcpy(slice_l_out, slice_l.data(), s * sizeof(int32_t));
  return 0;
}

extern "C" int
rdoq_emu_threshold(
  const int64_t* dist2, const int64_t* lambda, const int32_t* rate_coeff, const uint32_t* limit, int64_t count,
  uint32_t* out_div, uint32_t* out_recip)
{
  if (count < 1)
    return -1;
  hipLaunchKernelGGL(
    rdoq_threshold_probe_kernel, dim3(1), dim3(64), 0, nullptr, dist2, lambda, rate_coeff, limit, count, out_div,
    out_recip);
  return 0;
}
