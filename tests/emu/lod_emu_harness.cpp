// tests/emu/lod_emu_harness.cpp -- TEST INFRASTRUCTURE: the LoD build for scalable
// lifting (mpeg-pcc-tmc13_amd/csrc/lod_scalable.hpp + the kernels of lod_kernels.hpp)
// under the CPU wavefront emulator.  What lod_build_core (gpcc_attr_mi355.hip) does
// around the level loop -- Morton sort, gather, finalise, weights -- is repeated here
// with the same kernels; the sort itself is std::sort.
#include <algorithm>
#include <vector>

#include "hip/hip_runtime.h"

#include "lod_scalable.hpp"

using namespace gpcc;

namespace {
template<class T>
T*
carve(std::vector<void*>* blocks, size_t count)
{
  const size_t bytes = (sizeof(T) * std::max<size_t>(count, 1) + 255) & ~size_t(255);
  void* p = malloc(bytes + 256);
  memset(p, 0xCD, bytes + 256);  // the arena of the library is not cleared either
  blocks->push_back(p);
  return (T*)p;
}

int64_t
morton_of(const int32_t* p)
{
  int64_t m = 0;
  for (int b = 0; b < 21; b++)
    m |= ((int64_t)((p[0] >> b) & 1) << (3 * b + 2)) | ((int64_t)((p[1] >> b) & 1) << (3 * b + 1))
      | ((int64_t)((p[2] >> b) & 1) << (3 * b));
  return m;
}
}  // namespace

// outputs as gpcc_lod_build
extern "C" int
lod_emu_scalable_build(
  const gpcc_lod_params* lp, const int32_t* xyz, int32_t n, int32_t* neigh_count,
  int32_t* neigh_index, int32_t* neigh_weight, int32_t* indexes, int32_t* num_points_in_lod,
  int32_t* num_lods)
{
  if (!lp->scalable_lifting_enabled_flag || n <= 0)
    return -1;
  std::vector<void*> blocks;
  const size_t N = (size_t)n;
  const int nb0 = (n + 31) >> 5, nb1 = (nb0 + 31) >> 5, nb2 = (nb1 + 31) >> 5;
  int64_t* d_code = carve<int64_t>(&blocks, N);
  int32_t* d_order = carve<int32_t>(&blocks, N);
  {
    std::vector<std::pair<int64_t, int32_t>> v(N);
    for (int i = 0; i < n; i++)
      v[i] = {morton_of(xyz + 3 * (size_t)i), i};
    std::sort(v.begin(), v.end());
    for (int i = 0; i < n; i++) {
      d_code[i] = v[i].first;
      d_order[i] = v[i].second;
    }
  }
  int32_t* d_pos = carve<int32_t>(&blocks, 3 * N);
  int32_t* d_bpos = carve<int32_t>(&blocks, 3 * N);
  LodWork w{};
  w.n = n;
  w.code = d_code;
  w.order = d_order;
  w.pos = d_pos;
  w.bpos = d_bpos;
  w.bpos_lod = carve<int32_t>(&blocks, 3 * N);
  w.list_a = carve<int32_t>(&blocks, N + 1);
  w.list_b = carve<int32_t>(&blocks, N + 1);
  w.refine = carve<int32_t>(&blocks, N + 1);
  w.flags = carve<uint8_t>(&blocks, N + 1);
  w.heads = carve<uint8_t>(&blocks, N + 1);
  w.nxt0 = carve<int32_t>(&blocks, N + 2);
  w.nj0 = carve<int32_t>(&blocks, N + 2);
  w.nj1 = carve<int32_t>(&blocks, N + 2);
  w.ret_key = carve<int64_t>(&blocks, N + 1);
  w.counts = carve<int32_t>(&blocks, 64);
  w.scan = carve<unsigned long long>(&blocks, 1024);
  memset(w.counts, 0, sizeof(int32_t) * 64);
  memset(w.scan, 0, sizeof(unsigned long long) * 1024);
  w.atlas_limit = carve<long long>(&blocks, 1);
  {
    int32_t* p = carve<int32_t>(&blocks, (size_t)2 * 2 * 3 * (nb0 + nb1 + nb2 + 3));
    const int cnt[3] = {nb0 + 1, nb1 + 1, nb2 + 1};
    for (int l = 0; l < 2; l++)
      for (int lev = 0; lev < 3; lev++)
        for (int m = 0; m < 2; m++) {
          w.box[l][lev][m] = p;
          p += 3 * cnt[lev];
        }
  }
  w.pred_count = carve<int32_t>(&blocks, N);
  w.pred_point = carve<int32_t>(&blocks, 3 * N);
  w.pred_dist2 = carve<uint64_t>(&blocks, 3 * N);
  w.pt2pred = carve<int32_t>(&blocks, N);
  w.indexes = carve<int32_t>(&blocks, N);
  int32_t* d_neigh_index = carve<int32_t>(&blocks, 3 * N);
  int32_t* d_weight = carve<int32_t>(&blocks, 3 * N);

  hipLaunchKernelGGL(
    lod_gather_pos_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n, xyz,
    (const int32_t*)d_order, lp->lod_neigh_bias[0], lp->lod_neigh_bias[1], lp->lod_neigh_bias[2],
    d_pos, d_bpos, w.list_a);
  std::vector<int32_t> npl;
  int scan_epoch = 0;
  hipError_t e = lod_scalable_levels(lp, w, nullptr, &npl, &scan_epoch);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(
      lod_finalise_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n, 0, w.pred_count,
      (const int32_t*)w.pred_point, (const int32_t*)w.pt2pred, w.pred_dist2, d_neigh_index);
    hipLaunchKernelGGL(
      lod_compute_weights_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n, w.pred_count,
      (const uint64_t*)w.pred_dist2, d_weight);
    if (lp->attr_encoding == 1 && lp->pred_weight_blending_enabled_flag)
      hipLaunchKernelGGL(
        lod_blend_weights_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n,
        (const int32_t*)w.pred_count, (const int32_t*)w.pred_point, xyz, d_weight);
    memcpy(neigh_count, w.pred_count, sizeof(int32_t) * N);
    memcpy(neigh_index, d_neigh_index, sizeof(int32_t) * 3 * N);
    memcpy(neigh_weight, d_weight, sizeof(int32_t) * 3 * N);
    memcpy(indexes, w.indexes, sizeof(int32_t) * N);
    *num_lods = (int)npl.size();
    for (size_t i = 0; i < npl.size(); i++)
      num_points_in_lod[i] = npl[npl.size() - 1 - i];
  }
  for (void* p : blocks)
    free(p);
  return e == hipSuccess ? 0 : -5;
}

// ---- attribute inter prediction ---------------------------------------------------------
// lod_nn_search_kernel<false, true> + lod_finalise_inter_kernel + the frame preparation, as
// lod_build_core launches them, with all three sub-samplers.  The level loop below is this
// harness' own (the library's is HIP host code inside gpcc_attr_mi355.hip).
extern "C" int
lod_emu_inter_build(
  const gpcc_lod_params* lp, const int32_t* xyz, int32_t n, const int32_t* xyz_ref, int32_t n_ref,
  int32_t search_range, int32_t frame_distance, int32_t* neigh_count, int32_t* neigh_index,
  int32_t* neigh_weight, int32_t* indexes, int32_t* num_points_in_lod, int32_t* num_lods,
  int32_t* inter_ref)
{
  if (lp->scalable_lifting_enabled_flag || lp->lod_decimation_type < 0 || lp->lod_decimation_type > 2 || n <= 0 || n_ref < 0)
    return -1;
  // n_ref == 0: the intra build (lod_nn_search_kernel<false, false>, lod_finalise_kernel, the
  // block's own search ranges)
  const bool inter = n_ref > 0;
  std::vector<void*> blocks;
  const size_t N = (size_t)n, NF = (size_t)n_ref;
  auto sorted = [&](const int32_t* p, size_t cnt, int64_t* code, int32_t* order) {
    std::vector<std::pair<int64_t, int32_t>> v(cnt);
    for (size_t i = 0; i < cnt; i++)
      v[i] = {morton_of(p + 3 * i), (int32_t)i};
    std::sort(v.begin(), v.end());
    for (size_t i = 0; i < cnt; i++) {
      code[i] = v[i].first;
      order[i] = v[i].second;
    }
  };
  auto boxes_of = [&](int cnt, int32_t* box[3][2]) {
    const int b0 = (cnt + 31) >> 5, b1 = (b0 + 31) >> 5, b2 = (b1 + 31) >> 5;
    int32_t* p = carve<int32_t>(&blocks, (size_t)2 * 3 * (b0 + b1 + b2 + 3));
    const int c3[3] = {b0 + 1, b1 + 1, b2 + 1};
    for (int lev = 0; lev < 3; lev++)
      for (int m = 0; m < 2; m++) {
        box[lev][m] = p;
        p += 3 * c3[lev];
      }
  };
  auto build_boxes = [&](int32_t* box[3][2], const int32_t* list, int cnt, const int32_t* bpos) {
    const int c0 = (cnt + 31) >> 5, c1 = (c0 + 31) >> 5;
    hipLaunchKernelGGL(lod_box0_kernel, dim3(lod_grid(std::max(c0, 1), 256)), dim3(256), 0, nullptr, cnt, list, bpos,
                       box[0][0], box[0][1]);
    hipLaunchKernelGGL(lod_box_up_kernel, dim3(lod_grid(std::max(c1, 1), 256)), dim3(256), 0, nullptr, c0,
                       (const int32_t*)box[0][0], (const int32_t*)box[0][1], box[1][0], box[1][1]);
    hipLaunchKernelGGL(lod_box_up_kernel, dim3(1), dim3(256), 0, nullptr, c1, (const int32_t*)box[1][0],
                       (const int32_t*)box[1][1], box[2][0], box[2][1]);
  };

  int64_t* d_code = carve<int64_t>(&blocks, N);
  int32_t* d_order = carve<int32_t>(&blocks, N);
  sorted(xyz, N, d_code, d_order);
  int32_t* d_pos = carve<int32_t>(&blocks, 3 * N);
  int32_t* d_bpos = carve<int32_t>(&blocks, 3 * N);
  int32_t* d_list_a = carve<int32_t>(&blocks, N + 1);
  int32_t* d_list_b = carve<int32_t>(&blocks, N + 1);
  int32_t* d_refine = carve<int32_t>(&blocks, N + 1);
  uint8_t* d_flags = carve<uint8_t>(&blocks, N + 1);
  uint8_t* d_heads = carve<uint8_t>(&blocks, N + 1);
  int32_t* d_nxt0 = carve<int32_t>(&blocks, N + 2);
  int32_t* d_nj[2] = {carve<int32_t>(&blocks, N + 2), carve<int32_t>(&blocks, N + 2)};
  int64_t* d_ret_key = carve<int64_t>(&blocks, N + 1);
  int32_t* d_counts = carve<int32_t>(&blocks, 64);
  unsigned long long* d_scan = carve<unsigned long long>(&blocks, 1024);
  memset(d_counts, 0, sizeof(int32_t) * 64);
  memset(d_scan, 0, sizeof(unsigned long long) * 1024);
  long long* d_atlas_limit = carve<long long>(&blocks, 1);
  // the distance sub-sampler's cells
  int32_t* d_cell_first = carve<int32_t>(&blocks, N + 2);
  int32_t* d_positions = carve<int32_t>(&blocks, N + 1);
  int64_t* d_cell_key = carve<int64_t>(&blocks, N + 1);
  uint32_t* d_cell_state = carve<uint32_t>(&blocks, 4 * (N + 1));
  memset(d_cell_state, 0, sizeof(uint32_t) * 4 * (N + 1));
  int32_t* d_small = carve<int32_t>(&blocks, 64);
  memset(d_small, 0, sizeof(int32_t) * 64);
  int32_t* box_ret[3][2];
  int32_t* box_ref[3][2];
  int32_t* box_frame[3][2];
  boxes_of(n, box_ret);
  boxes_of(n, box_ref);
  boxes_of(inter ? n_ref : 1, box_frame);
  int32_t* d_pred_count = carve<int32_t>(&blocks, N);
  int32_t* d_pred_point = carve<int32_t>(&blocks, 3 * N);
  uint64_t* d_pred_dist2 = carve<uint64_t>(&blocks, 3 * N);
  int32_t* d_pt2pred = carve<int32_t>(&blocks, N);
  int32_t* d_indexes = carve<int32_t>(&blocks, N);
  int32_t* d_neigh_index = carve<int32_t>(&blocks, 3 * N);
  int32_t* d_weight = carve<int32_t>(&blocks, 3 * N);
  int32_t* d_inter_ref = carve<int32_t>(&blocks, 3 * N);
  // the reference frame
  int64_t* d_fcode = carve<int64_t>(&blocks, NF);
  int32_t* d_forder = carve<int32_t>(&blocks, NF);
  if (inter)
    sorted(xyz_ref, NF, d_fcode, d_forder);
  int32_t* d_fpos = carve<int32_t>(&blocks, 3 * NF);
  int32_t* d_fbpos = carve<int32_t>(&blocks, 3 * NF);
  int32_t* d_flist = carve<int32_t>(&blocks, NF + 1);

  const int b0 = lp->lod_neigh_bias[0], b1 = lp->lod_neigh_bias[1], b2 = lp->lod_neigh_bias[2];
  hipLaunchKernelGGL(lod_gather_pos_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n, xyz,
                     (const int32_t*)d_order, b0, b1, b2, d_pos, d_bpos, d_list_a);
  if (inter) {
    hipLaunchKernelGGL(lod_gather_pos_kernel, dim3(lod_grid(n_ref, 256)), dim3(256), 0, nullptr, n_ref, xyz_ref,
                       (const int32_t*)d_forder, b0, b1, b2, d_fpos, d_fbpos, d_flist);
    build_boxes(box_frame, d_flist, n_ref, d_fbpos);
  }

  std::vector<int32_t> npl;
  npl.push_back(n);
  int32_t* d_input = d_list_a;
  int32_t* d_ret = d_list_b;
  int n_in = n, n_idx = 0, scan_epoch = 0;
  const int max_levels = lp->num_detail_levels_minus1 + 1;
  for (int lod = 0; n_in > 0 && lod < max_levels; lod++) {
    const int start = n_idx;
    int n_ret = 0, n_ref_l = 0;
    const int shift_bits0 = lp->dist2 + lp->attr_dist2_delta + lod;
    if (lod == max_levels - 1 || (lp->lod_decimation_type != 1 && n_in == 1)) {
      memcpy(d_refine + start, d_input, sizeof(int32_t) * n_in);
      n_ref_l = n_in;
    } else {
      const int period = lp->lod_sampling_period[lod];
      if (lp->lod_decimation_type == 0) {
        // subsampleByDistance as lod_build_core launches it; its workgroups (eight ticket
        // classes) wait for one another: they run together here (no LDS in that kernel)
        LodCtx lc{};
        lc.n = n;
        lc.code = d_code;
        lc.order = d_order;
        lc.pos = d_pos;
        lc.bpos = d_bpos;
        lc.input = d_input;
        lc.n_in = n_in;
        lc.shift3 = 3 * (shift_bits0 + 1);
        lc.boundary = std::min(63, lc.shift3 + 21);
        lc.radius2 = (int64_t)3 << (shift_bits0 << 1);
        lc.cell_first = d_cell_first;
        lc.cell_key = d_cell_key;
        lc.cell_state = d_cell_state;
        lc.ticket = d_small;
        lc.error = d_small + 8;
        lc.epoch = lod + 1;
        lc.flags = d_flags;
        hipLaunchKernelGGL(lod_flag_cell_heads_kernel, dim3(lod_grid(n_in, 256)), dim3(256), 0, nullptr, lc, d_heads, d_positions);
        scan_epoch++;
        const int g0 = (int)std::min<int64_t>(1024, ((int64_t)n_in + 1023) / 1024);
        hipLaunchKernelGGL(lod_partition_kernel, dim3(std::max(g0, 1)), dim3(256), 0, nullptr, n_in, (const uint8_t*)d_heads,
                           (const int32_t*)d_positions, d_cell_first, (int32_t*)nullptr, d_counts, d_scan, scan_epoch);
        const int ncell = d_counts[0];
        d_cell_first[ncell] = n_in;
        memset(d_small, 0, sizeof(int32_t) * 8);
        lc.ncell = ncell;
        hipLaunchKernelGGL(lod_cell_keys_kernel, dim3(lod_grid(ncell, 256)), dim3(256), 0, nullptr, lc);
        emu::set_concurrent_blocks(8);
        hipLaunchKernelGGL(lod_subsample_distance_kernel, dim3(8), dim3(256), 0, nullptr, lc);
        emu::set_concurrent_blocks(1);
        if (d_small[8])
          return -7;
      } else if (lp->lod_decimation_type == 1) {
        hipLaunchKernelGGL(lod_flag_periodic_kernel, dim3(lod_grid(n_in, 256)), dim3(256), 0, nullptr, n_in, period, d_flags);
      } else {
        LodCtx lc{};
        lc.code = d_code;
        lc.pos = d_pos;
        lc.input = d_input;
        lc.n_in = n_in;
        lc.shift3 = 3 * (shift_bits0 + 1);
        lc.flags = d_flags;
        hipLaunchKernelGGL(lod_centroid_next_kernel, dim3(lod_grid(n_in + 1, 256)), dim3(256), 0, nullptr, lc, period, d_nxt0);
        memset(d_heads, 0, (size_t)n_in + 1);
        d_heads[0] = 1;
        const int32_t* cur = d_nxt0;
        for (int r = 0, reach = 1; reach < n_in; r++, reach *= 2) {
          hipLaunchKernelGGL(lod_centroid_jump_kernel, dim3(lod_grid(n_in + 1, 256)), dim3(256), 0, nullptr, n_in, cur,
                             d_nj[r & 1], d_heads);
          cur = d_nj[r & 1];
        }
        hipLaunchKernelGGL(lod_centroid_pick_kernel, dim3(lod_grid(n_in, 256)), dim3(256), 0, nullptr, lc, shift_bits0,
                           (const int32_t*)d_nxt0, (const uint8_t*)d_heads, 1);
      }
      scan_epoch++;
      const int grid = (int)std::min<int64_t>(1024, ((int64_t)n_in + 1023) / 1024);
      hipLaunchKernelGGL(lod_partition_kernel, dim3(std::max(grid, 1)), dim3(256), 0, nullptr, n_in,
                         (const uint8_t*)d_flags, (const int32_t*)d_input, d_ret, d_refine + start, d_counts, d_scan,
                         scan_epoch);
      n_ret = d_counts[0];
      n_ref_l = n_in - n_ret;
    }
    n_idx += n_ref_l;
    if (n_ref_l > 0) {
      NnCtx nc{};
      nc.n = n;
      nc.code = d_code;
      nc.order = d_order;
      nc.bpos = d_bpos;
      nc.retained = d_ret;
      nc.ret_key = d_ret_key;
      nc.n_ret = n_ret;
      nc.refine = d_refine + start;
      nc.n_ref = n_ref_l;
      nc.start = start;
      nc.shift3 = 3 * (1 + shift_bits0);
      nc.boundary = std::min(63, nc.shift3 + 21);
      nc.distribution = lp->prediction_with_distribution_enabled;
      nc.range_inter = inter ? search_range : lp->inter_lod_search_range;
      nc.range_intra = inter ? search_range : lp->intra_lod_search_range;
      nc.intra = lod >= lp->intra_lod_prediction_skip_layers;
      nc.max_neigh = lp->num_pred_nearest_neighbours_minus1 + 1;
      for (int lev = 0; lev < 3; lev++)
        for (int m = 0; m < 2; m++) {
          nc.box_ret[lev][m] = box_ret[lev][m];
          nc.box_ref[lev][m] = box_ref[lev][m];
          nc.box_frame[lev][m] = box_frame[lev][m];
        }
      nc.atlas_limit = d_atlas_limit;
      nc.pred_count = d_pred_count;
      nc.pred_point = d_pred_point;
      nc.pred_dist2 = d_pred_dist2;
      nc.pt2pred = d_pt2pred;
      nc.indexes = d_indexes;
      nc.frame_code = d_fcode;
      nc.frame_order = d_forder;
      nc.frame_bpos = d_fbpos;
      nc.frame_identity = d_flist;
      nc.n_frame = n_ref;
      nc.frame_range = search_range;
      nc.frame_boundary = std::min(63, nc.shift3 + 9);
      if (n_ret > 0) {
        hipLaunchKernelGGL(lod_ret_keys_kernel, dim3(lod_grid(n_ret, 256)), dim3(256), 0, nullptr, n_ret,
                           (const int32_t*)d_ret, (const int64_t*)d_code, nc.shift3, d_ret_key);
        build_boxes(box_ret, d_ret, n_ret, d_bpos);
      }
      if (nc.intra)
        build_boxes(box_ref, d_refine + start, n_ref_l, d_bpos);
      *d_atlas_limit = INT64_MAX;
      if (n_ret > 0)
        hipLaunchKernelGGL(lod_atlas_limit_kernel, dim3(lod_grid(n_ret, 256)), dim3(256), 0, nullptr, nc, d_atlas_limit);
      if (inter)
        hipLaunchKernelGGL((lod_nn_search_kernel<false, true>), dim3(lod_grid(n_ref_l, 256)), dim3(256), 0, nullptr, nc);
      else
        hipLaunchKernelGGL((lod_nn_search_kernel<false, false>), dim3(lod_grid(n_ref_l, 256)), dim3(256), 0, nullptr, nc);
    }
    if (n_ret > 0)
      npl.push_back(n_ret);
    std::swap(d_input, d_ret);
    n_in = n_ret;
  }
  if (inter)
    hipLaunchKernelGGL(lod_finalise_inter_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n, d_pred_count,
                       (const int32_t*)d_pred_point, (const int32_t*)d_pt2pred, d_pred_dist2, d_neigh_index, d_inter_ref,
                       frame_distance);
  else {
    hipLaunchKernelGGL(lod_finalise_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n, 0, d_pred_count,
                       (const int32_t*)d_pred_point, (const int32_t*)d_pt2pred, d_pred_dist2, d_neigh_index);
    memset(d_inter_ref, 0, sizeof(int32_t) * 3 * N);
  }
  hipLaunchKernelGGL(lod_compute_weights_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n, d_pred_count,
                     (const uint64_t*)d_pred_dist2, d_weight);
  if (lp->attr_encoding == 1 && lp->pred_weight_blending_enabled_flag) {
    if (inter)
      hipLaunchKernelGGL(lod_blend_weights_inter_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n,
                         (const int32_t*)d_pred_count, (const int32_t*)d_pred_point, xyz, xyz_ref, d_weight);
    else
      hipLaunchKernelGGL(lod_blend_weights_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n,
                         (const int32_t*)d_pred_count, (const int32_t*)d_pred_point, xyz, d_weight);
  }
  memcpy(neigh_count, d_pred_count, sizeof(int32_t) * N);
  memcpy(neigh_index, d_neigh_index, sizeof(int32_t) * 3 * N);
  memcpy(neigh_weight, d_weight, sizeof(int32_t) * 3 * N);
  memcpy(indexes, d_indexes, sizeof(int32_t) * N);
  memcpy(inter_ref, d_inter_ref, sizeof(int32_t) * 3 * N);
  *num_lods = (int)npl.size();
  for (size_t i = 0; i < npl.size(); i++)
    num_points_in_lod[i] = npl[npl.size() - 1 - i];
  for (void* p : blocks)
    free(p);
  return 0;
}

// ---- reflectance lifting with neighbours in a reference frame -----------------------------
// The arrangement host_lod_coder / launch_lift (gpcc_attr_mi355.hip) use for attribute inter
// prediction: the frame's attributes in fixed point BEHIND the n working values, flagged
// neighbours pointed there, the intra kernels unchanged.  One QP layer, one component.
extern "C" int
lift_emu_inter(
  const gpcc_lift_params* p, int32_t encoder, int32_t n, const int32_t* nc, const int32_t* ni,
  const int32_t* nw, const int32_t* inter_ref, const int32_t* indexes, int32_t* attrs,
  const int32_t* attrs_ref, int32_t n_ref, int32_t* coeffs)
{
  if (p->num_qp_layers != 1 || p->scalable_lifting_enabled_flag || n <= 0 || n_ref <= 0)
    return -1;
  std::vector<void*> blocks;
  const size_t N = (size_t)n, NE = N + (size_t)n_ref;
  int32_t* d_ni = carve<int32_t>(&blocks, 3 * N);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < 3; j++)
      d_ni[3 * i + j] = ni[3 * i + j] + (j < nc[i] && inter_ref[3 * i + j] ? n : 0);
  RsqrtLut* lut = (RsqrtLut*)carve<char>(&blocks, sizeof(RsqrtLut));
  {
    const uint16_t r3[96] = {GPCC_RSQRT_R3};
    const uint32_t rc[96] = {GPCC_RSQRT_RC};
    memcpy(lut->r3, r3, sizeof(r3));
    memcpy(lut->rc, rc, sizeof(rc));
  }
  LiftCtx cx{};
  cx.n = n;
  cx.c = 1;
  cx.num_lods = p->num_lods;
  for (int l = 0; l < p->num_lods; l++)
    cx.npl[l] = p->num_points_in_lod[l];
  cx.num_ranges = 1;
  cx.lcp_enabled = 0;
  cx.bitdepth = p->bitdepth;
  cx.num_qp_layers = 1;
  memcpy(cx.layer_qp, p->layer_qp, sizeof(cx.layer_qp));
  cx.max_qp = p->max_qp;
  cx.fixed_point_qp_offset = p->fixed_point_qp_offset;
  cx.nc = nc;
  cx.ni = d_ni;
  cx.nw = nw;
  cx.indexes = indexes;
  cx.qp_off = nullptr;
  cx.attrs = attrs;
  cx.coeffs = coeffs;
  cx.lcp = carve<int8_t>(&blocks, GPCC_MAX_LODS);
  cx.a = carve<int64_t>(&blocks, NE);
  cx.qw = carve<unsigned long long>(&blocks, NE);
  cx.uw = carve<unsigned long long>(&blocks, NE);
  cx.up = carve<unsigned long long>(&blocks, NE);
  cx.lcp_sums = carve<long long>(&blocks, 2 * GPCC_MAX_LODS);
  cx.rsqrt = lut;
  for (int r = 0; r < n_ref; r++)
    cx.a[N + r] = (int64_t)attrs_ref[r] * 256;
  const int* npl = cx.npl;
  auto grid = [&](int items) { return dim3(lod_grid(std::max(items, 1), 256)); };
  hipLaunchKernelGGL(lift_init_kernel, grid(n), dim3(256), 0, nullptr, cx, encoder);
  for (int l = p->num_lods - 1; l >= 1; l--)
    if (npl[l] > npl[l - 1])
      hipLaunchKernelGGL(lift_quant_weights_kernel, grid(npl[l] - npl[l - 1]), dim3(256), 0, nullptr, cx, npl[l - 1], npl[l]);
  if (encoder)
    for (int l = p->num_lods - 1; l >= 1; l--) {
      if (npl[l] == npl[l - 1])
        continue;
      const int cnt = npl[l] - npl[l - 1];
      hipLaunchKernelGGL(lift_predict_kernel<1>, grid(cnt), dim3(256), 0, nullptr, cx, npl[l - 1], npl[l], 1);
      hipLaunchKernelGGL(lift_update_scatter_kernel<1>, grid(cnt), dim3(256), 0, nullptr, cx, npl[l - 1], npl[l]);
      hipLaunchKernelGGL(lift_update_apply_kernel<1>, grid(npl[l - 1]), dim3(256), 0, nullptr, cx, npl[l - 1], 1);
    }
  hipLaunchKernelGGL(lift_quantise_kernel<1>, grid(n), dim3(256), 0, nullptr, cx, encoder);
  for (int l = 1; l < p->num_lods; l++) {
    if (npl[l] == npl[l - 1])
      continue;
    const int cnt = npl[l] - npl[l - 1];
    hipLaunchKernelGGL(lift_update_scatter_kernel<1>, grid(cnt), dim3(256), 0, nullptr, cx, npl[l - 1], npl[l]);
    hipLaunchKernelGGL(lift_update_apply_kernel<1>, grid(npl[l - 1]), dim3(256), 0, nullptr, cx, npl[l - 1], 0);
    hipLaunchKernelGGL(lift_predict_kernel<1>, grid(cnt), dim3(256), 0, nullptr, cx, npl[l - 1], npl[l], 0);
  }
  hipLaunchKernelGGL(lift_writeback_kernel, grid(n), dim3(256), 0, nullptr, cx);
  for (void* b : blocks)
    free(b);
  return 0;
}

// ---- the reflectance predicting transform with neighbours in a reference frame ---------------
// pred_dag_kernel<1, ENC, true> with the arrangement host_lod_coder / launch_pred use: flagged
// neighbours point behind the n predictors (PredCtx::frame_attr), the share arrays have spare
// entries there.  Decoder and encoder, the latter's iteration over the rate model included.  One
// QP layer.  The persistent kernels run as ONE workgroup here.
#include "pred_kernels.hpp"

extern "C" int
pred_emu_inter(
  const gpcc_pred_params* p, int32_t encoder, int32_t n, const int32_t* nc, const int32_t* ni,
  const int32_t* nw, const int32_t* inter_ref, const int32_t* indexes, int32_t* attrs,
  const int32_t* attrs_ref, int32_t n_ref, int32_t* values)
{
  if (p->num_qp_layers != 1 || p->scalable_lifting_enabled_flag || n <= 0 || n_ref <= 0)
    return -1;
  std::vector<void*> blocks;
  const size_t N = (size_t)n, NE = N + (size_t)n_ref;
  int32_t* d_ni = carve<int32_t>(&blocks, 3 * N);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < 3; j++)
      d_ni[3 * i + j] = ni[3 * i + j] + (j < nc[i] && inter_ref[3 * i + j] ? n : 0);
  PredCtx cx{};
  cx.n = n;
  cx.c = 1;
  cx.num_lods = p->num_lods;
  for (int l = 0; l < p->num_lods; l++)
    cx.npl[l] = p->num_points_in_lod[l];
  cx.num_ranges = 1;
  cx.max_levels = p->max_num_detail_levels;
  cx.bitdepth = p->bitdepth;
  cx.num_qp_layers = 1;
  memcpy(cx.layer_qp, p->layer_qp, sizeof(cx.layer_qp));
  cx.max_qp = p->max_qp;
  cx.max_direct = p->max_num_direct_predictors;
  cx.avg_disabled = p->direct_avg_predictor_disabled_flag != 0;
  cx.threshold = p->adaptive_prediction_threshold;
  cx.icp_enabled = 0;
  for (int k = 0; k < 3; k++)
    cx.qnw[k] = p->quant_neigh_weight[k];
  cx.nc = nc;
  cx.ni = d_ni;
  cx.nw = nw;
  cx.indexes = indexes;
  cx.qp_off = nullptr;
  cx.attrs = attrs;
  cx.values = values;
  cx.icp = carve<int8_t>(&blocks, GPCC_MAX_LODS * 3);
  cx.indeg = carve<int32_t>(&blocks, NE);
  cx.recv = carve<int32_t>(&blocks, NE);
  cx.acc = carve<unsigned long long>(&blocks, NE);
  cx.qw = carve<unsigned long long>(&blocks, NE);
  cx.rec = carve<uint32_t>(&blocks, 4 * N);
  memset(cx.indeg, 0, sizeof(int32_t) * NE);
  memset(cx.recv, 0, sizeof(int32_t) * NE);
  memset(cx.acc, 0, sizeof(unsigned long long) * NE);
  memset(cx.qw, 0, sizeof(unsigned long long) * NE);
  memset(cx.rec, 0, sizeof(uint32_t) * 4 * N);
  int32_t* small = carve<int32_t>(&blocks, 64);
  memset(small, 0, sizeof(int32_t) * 64);
  cx.ticket = small;
  cx.error = small + 8;
  cx.wide = small + 16;
  cx.packed_ok = cx.qnw[0] >= 0 && cx.qnw[1] >= 0 && cx.qnw[2] >= 0 && cx.qnw[0] + cx.qnw[1] + cx.qnw[2] < 256;
  cx.icp_sums = carve<unsigned long long>(&blocks, GPCC_MAX_LODS * 18);
  cx.tag = 1;
  cx.frame_attr = attrs_ref;
  hipLaunchKernelGGL(pred_indegree_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, cx);
  if (cx.qnw[0] || cx.qnw[1] || cx.qnw[2])
    hipLaunchKernelGGL(pred_quant_weights_kernel, dim3(1), dim3(256), 0, nullptr, cx);
  else
    for (int i = 0; i < n; i++)
      cx.qw[i] = 256;
  int unsettled = 0;
  if (encoder && cx.max_direct > 0) {
    // the encoder with direct predictors, as launch_pred iterates it (gpcc_attr_mi355.hip): the
    // DAG pass with the rate model before every predictor, then that model's trajectory from the
    // values the pass produced, until the values stop changing.  The inclusive scan the library
    // runs on the device (rc_scan) is a host loop here.
    std::vector<double> log2tab((size_t)kRateScale + 1);
    for (int v = 0; v <= kRateScale; v++)
      log2tab[v] = log2((double)v);
    int32_t* rm = carve<int32_t>(&blocks, 6 * N);
    int32_t* src_copy = carve<int32_t>(&blocks, N);
    int32_t* prev_values = carve<int32_t>(&blocks, N);
    int32_t* ev_rank = carve<int32_t>(&blocks, N + 1);
    uint8_t* ev_up = carve<uint8_t>(&blocks, N + 1);
    int32_t* ev_state = carve<int32_t>(&blocks, N + 1);
    int32_t* flag = small + 24;
    memcpy(src_copy, attrs, sizeof(int32_t) * N);
    memset(prev_values, 0, sizeof(int32_t) * N);
    cx.src = src_copy;
    cx.rm = rm;
    cx.log2tab = log2tab.data();
    hipLaunchKernelGGL(pred_rate_init_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, rm, n);
    bool settled = false;
    for (int pass = 0; pass < 64 && !settled; pass++) {
      cx.tag = (uint32_t)(pass + 1);
      memset(cx.ticket, 0, 8 * sizeof(int32_t));
      *flag = 0;
      hipLaunchKernelGGL((pred_dag_kernel<1, true, true>), dim3(1), dim3(256), 0, nullptr, cx);
      hipLaunchKernelGGL(pred_values_diff_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, (const int32_t*)cx.values,
                         prev_values, N, flag);
      if (pass > 0 && !*flag) {
        settled = true;
        break;
      }
      const int chunks = n / kRateChunk + 1;
      hipLaunchKernelGGL(pred_rate_scan_kernel, dim3((chunks + 63) / 64), dim3(64), 0, nullptr, (const int32_t*)cx.values, 1,
                         (const uint8_t*)nullptr, n, (const int32_t*)nullptr, rm, 6, 0);
      hipLaunchKernelGGL(pred_rate_flags_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, (const int32_t*)cx.values, n, 1, 0, ev_rank);
      for (size_t i = 1; i <= N; i++)
        ev_rank[i] += ev_rank[i - 1];
      hipLaunchKernelGGL(pred_rate_events_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, (const int32_t*)cx.values, n, 1, 0,
                         (const int32_t*)ev_rank, ev_up);
      hipLaunchKernelGGL(pred_rate_scan_kernel, dim3((chunks + 63) / 64), dim3(64), 0, nullptr, (const int32_t*)nullptr, 0,
                         (const uint8_t*)ev_up, n, (const int32_t*)(ev_rank + n), ev_state, 1, 1);
      hipLaunchKernelGGL(pred_rate_gather_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, (const int32_t*)ev_rank,
                         (const int32_t*)ev_state, n, 0, rm);
    }
    unsettled = !settled;
  } else if (encoder)
    hipLaunchKernelGGL((pred_dag_kernel<1, true, true>), dim3(1), dim3(256), 0, nullptr, cx);
  else
    hipLaunchKernelGGL((pred_dag_kernel<1, false, true>), dim3(1), dim3(256), 0, nullptr, cx);
  const int err = *cx.error ? 1 : (unsettled ? 2 : 0);
  for (void* b : blocks)
    free(b);
  return err ? -6 - err : 0;
}

// pred_rate_scan_kernel alone, launched as the library launches it (one thread per chunk of 256 events, `m_max`
// sizing the grid, the event count read from memory when m >= 0): values (stride) or event bytes in, states out
extern "C" int
lod_emu_rate_scan(
  const int32_t* values, int32_t stride, const uint8_t* ev, int32_t m_max, int32_t m, int32_t* state,
  int32_t state_stride, int32_t write_final)
{
  const int chunks = m_max / kRateChunk + 1;
  int32_t m_mem = m;
  hipLaunchKernelGGL(
    pred_rate_scan_kernel, dim3((chunks + 63) / 64), dim3(64), 0, nullptr, values, stride, ev, m_max,
    m >= 0 ? (const int32_t*)&m_mem : (const int32_t*)nullptr, state, state_stride, write_final);
  return 0;
}
