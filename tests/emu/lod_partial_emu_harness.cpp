// tests/emu/lod_partial_emu_harness.cpp -- TEST INFRASTRUCTURE: the scalable-lifting LoD build of a
// PARTIALLY decoded slice (lod_scalable_levels with a first level m > 0 and the count of points the
// decode skipped) and the quantisation weights of such a slice
// (quant_weights_scalable_partial_kernel) under the CPU wavefront emulator.  Workspace, gather,
// level loop and finalise / weights are the library's text (lod_levels.hpp, lod_scalable.hpp); the
// Morton sort is std::sort.
#include <algorithm>
#include <vector>

#include "hip/hip_runtime.h"

#include "lod_scalable.hpp"
#include "lift_kernels.hpp"
#include "lod_emu_blocks.hpp"

using namespace gpcc;

// outputs as gpcc_lod_build_partial
extern "C" int
lod_emu_partial_build(
  const gpcc_lod_params* lp, const int32_t* xyz, int32_t n, int32_t min_geom_node_size_log2,
  int32_t geom_num_points, int32_t* neigh_count, int32_t* neigh_index, int32_t* neigh_weight,
  int32_t* indexes, int32_t* num_points_in_lod, int32_t* num_lods)
{
  if (!lp->scalable_lifting_enabled_flag || n <= 0 || geom_num_points < n)
    return -1;
  EmuBlocks blocks;
  EmuLodHost host;
  LodWork w{};
  emu_lod_workspace(blocks, w, xyz, n, nullptr, 0, true);
  lod_prepare(lp, w, nullptr, host);
  std::vector<int32_t> npl;
  int scan_epoch = 0;
  if (lod_scalable_levels(lp, w, nullptr, &npl, &scan_epoch, min_geom_node_size_log2, (int64_t)geom_num_points - n) != hipSuccess
      || lod_finish(lp, w, nullptr, nullptr, host) != hipSuccess)
    return -5;
  if (!blocks.intact())
    return EmuBlocks::kOverrun;
  emu_lod_results(w, npl, neigh_count, neigh_index, neigh_weight, indexes, num_points_in_lod, num_lods);
  return 0;
}

// computeQuantizationWeightsScalable of a partially decoded slice, as launch_lift launches it:
// qw [n] out (8 fractional bits)
extern "C" int
quant_weights_emu_partial(
  int32_t n, int32_t min_geom_node_size_log2, int32_t geom_num_points,
  const int32_t* num_points_in_lod, int32_t num_lods, uint64_t* qw)
{
  if (n <= 0 || num_lods < 1 || num_lods > GPCC_MAX_LODS || num_points_in_lod[num_lods - 1] != n)
    return -1;
  LodSizes t{};
  t.num_lods = num_lods;
  for (int l = 0; l < num_lods; l++)
    t.npl[l] = num_points_in_lod[l];
  hipLaunchKernelGGL(
    quant_weights_scalable_partial_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n,
    (long long)geom_num_points, (int)(min_geom_node_size_log2 == 0), t, (unsigned long long*)qw);
  return 0;
}
