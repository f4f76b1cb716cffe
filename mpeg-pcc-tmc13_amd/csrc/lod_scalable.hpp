// lod_scalable.hpp -- the level loop of the LoD build under
// aps.scalable_lifting_enabled_flag (buildPredictorsFast,
// tmc3/PCCTMC3Common.h:2300-2469 with the scalable branches :1174-1176,
// :1232-1236, :1918-1939, :2230-2235, :2377-2448), for whole slices and for
// the partial decode (minGeomNodeSizeLog2 = m > 0: the octree stopped m levels
// early, the cloud holds fewer points than the slice header counts).
//
// What changes against lod_plain_levels (lod_levels.hpp), whose pieces this loop shares:
//   * levels m .. 20 (AttributeParameterSet::maxNumDetailLevels, hls.h:835-839):
//     node size, walk direction, corner mask, cell shift and prune distance
//     take the absolute level, the entries of `npl` count from m;
//   * sub-sampling is the octree one (lod_centroid_* kernels): node size = LoD
//     index, every node is a group, the walk direction alternates;
//   * the search of LoD l sees all positions at the corner of their node of
//     size 2^l (lod_node_corner_bpos_kernel), in cells of 2^(l+1), and drops
//     neighbours beyond max_neigh_range (lod_nn_search_kernel<true>);
//   * while a new refinement layer is larger than all finer layers together the
//     finer layers are searched AGAIN against the new retained set
//     ("concatenateLayers"; the points the partial decode never saw count among
//     the finer ones).  A predictor's slot depends on its position in the
//     coding order only, so a repeated search simply overwrites its results.
//
// Like lod_levels.hpp this text also runs under the CPU wavefront emulator
// (tests/emu) -- the LoD structure of this file is pinned there against the
// oracle, which is pinned against the compiled reference.
#pragma once

#include <algorithm>
#include <vector>

#include "lod_levels.hpp"

namespace gpcc {

// -> cumulative sizes in `npl` as the reference pushes them (n first, then the
// retained count of every level that retains); *scan_epoch is the partition
// kernel's epoch counter of the build.  Partial decode: `first_level` is
// minGeomNodeSizeLog2 (0..20, checked by the caller) and `skipped` >= 0 the
// slice's points that the cloud lacks (geom_num_points_minus1 + 1 - n).
inline hipError_t
lod_scalable_levels(
  const gpcc_lod_params* lp, const LodWork& w, hipStream_t st, std::vector<int32_t>* npl,
  int* scan_epoch, int first_level = 0, int64_t skipped = 0)
{
  constexpr int kLevels = 21;
  const int n = w.n;
  const bool unit_bias =
    lp->lod_neigh_bias[0] == 1 && lp->lod_neigh_bias[1] == 1 && lp->lod_neigh_bias[2] == 1;
  LodQuietHost host;

  // nearest neighbours of the layer [s, e) of the coding-order list at LoD `l`
  // against the retained list `ret`
  auto search = [&](int l, int s, int e, const int32_t* ret, int n_ret) -> hipError_t {
    if (e - s <= 0)
      return hipSuccess;
    NnCtx nc{};
    nc.node_mask = l ? 0xffffffffu << l : 0xffffffffu;
    nc.bpos = w.bpos;
    if (l) {
      hipLaunchKernelGGL(
        lod_node_corner_bpos_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, st, n, (const int32_t*)w.pos,
        nc.node_mask, lp->lod_neigh_bias[0], lp->lod_neigh_bias[1], lp->lod_neigh_bias[2], w.bpos_lod);
      nc.bpos = w.bpos_lod;
    }
    nc.shift3 = 3 * (1 + l);
    nc.boundary = std::min(63, nc.shift3 + kAtlasBits);
    nc.range_inter = lp->inter_lod_search_range;
    nc.range_intra = lp->intra_lod_search_range;
    nc.pos = w.pos;
    nc.unit_bias = unit_bias;
    nc.prune_dist = (int64_t)(3ll * (lp->max_neigh_range_minus1 + 1)) << (2 * l);
    return lod_search_layer(nc, lp, w, l, s, e - s, ret, n_ret, true, false, st, host);
  };

  npl->clear();
  npl->push_back(n);
  int32_t* d_input = w.list_a;
  int32_t* d_ret = w.list_b;
  int n_in = n, n_idx = 0;
  bool concatenate = true;
  for (int lod = first_level; n_in > 0 && lod < kLevels; lod++) {
    const int start = n_idx;
    int n_ret = 0, n_ref = 0;
    if (lod == kLevels - 1 || n_in == 1) {
      GPCC_LODS_TRY(hipMemcpyAsync(
        w.refine + start, d_input, sizeof(int32_t) * n_in, hipMemcpyDeviceToDevice, st));
      n_ref = n_in;
    } else {
      // subsampleByOctree (:2146-2194) with octreeNodeSizeLog2 = lod, no minimum
      // group size (period 1 = every node closes a group), direction = lod & 1
      LodCtx lc{};
      lc.code = w.code;
      lc.pos = w.pos;
      lc.input = d_input;
      lc.n_in = n_in;
      lc.shift3 = 3 * (lod + 1);
      lc.flags = w.flags;
      GPCC_LODS_TRY(lod_centroid_flags(w, lc, 1, lod, lod & 1, st, host));
      // retained / refinement lists
      GPCC_LODS_TRY(
        lod_partition(w, n_in, w.flags, d_input, d_ret, w.refine + start, st, scan_epoch, &n_ret, host));
      n_ref = n_in - n_ret;
    }
    n_idx += n_ref;

    if (concatenate && n_ref > 0) {
      if (n_ref <= start + skipped)
        concatenate = false;
      else
        for (int l = 0; l < lod - first_level; l++)
          GPCC_LODS_TRY(
            search(first_level + l, n - (*npl)[l], n - (*npl)[l + 1], d_ret, n_ret));
    }
    GPCC_LODS_TRY(search(lod, start, n_idx, d_ret, n_ret));
    if (n_ret > 0)
      npl->push_back(n_ret);
    std::swap(d_input, d_ret);
    n_in = n_ret;
  }
  return hipSuccess;
}

#undef GPCC_LODS_TRY

}  // namespace gpcc
