// tests/emu/lod_partial_emu_harness.cpp -- TEST INFRASTRUCTURE: the scalable-lifting LoD build of a
// PARTIALLY decoded slice (lod_scalable_levels with a first level m > 0 and the count of points the
// decode skipped) and the quantisation weights of such a slice
// (quant_weights_scalable_partial_kernel) under the CPU wavefront emulator.  Around the level loop
// it does what lod_build_core (gpcc_attr_mi355.hip) does -- Morton sort (std::sort here), gather,
// finalise, weights -- with the library's kernels.
#include <algorithm>
#include <vector>

#include "hip/hip_runtime.h"

#include "lod_scalable.hpp"
#include "lift_kernels.hpp"

using namespace gpcc;

namespace {
struct Blocks {
  std::vector<void*> all;
  ~Blocks()
  {
    for (void* p : all)
      free(p);
  }
  template<class T>
  T* carve(size_t count)
  {
    const size_t bytes = (sizeof(T) * std::max<size_t>(count, 1) + 255) & ~size_t(255);
    void* p = malloc(bytes + 256);
    memset(p, 0xCD, bytes + 256);  // the arena of the library is not cleared either
    all.push_back(p);
    return (T*)p;
  }
};

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

// outputs as gpcc_lod_build_partial
extern "C" int
lod_emu_partial_build(
  const gpcc_lod_params* lp, const int32_t* xyz, int32_t n, int32_t min_geom_node_size_log2,
  int32_t geom_num_points, int32_t* neigh_count, int32_t* neigh_index, int32_t* neigh_weight,
  int32_t* indexes, int32_t* num_points_in_lod, int32_t* num_lods)
{
  if (!lp->scalable_lifting_enabled_flag || n <= 0 || geom_num_points < n)
    return -1;
  Blocks b;
  const size_t N = (size_t)n;
  const int nb0 = (n + 31) >> 5, nb1 = (nb0 + 31) >> 5, nb2 = (nb1 + 31) >> 5;
  int64_t* d_code = b.carve<int64_t>(N);
  int32_t* d_order = b.carve<int32_t>(N);
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
  int32_t* d_pos = b.carve<int32_t>(3 * N);
  int32_t* d_bpos = b.carve<int32_t>(3 * N);
  LodWork w{};
  w.n = n;
  w.code = d_code;
  w.order = d_order;
  w.pos = d_pos;
  w.bpos = d_bpos;
  w.bpos_lod = b.carve<int32_t>(3 * N);
  w.list_a = b.carve<int32_t>(N + 1);
  w.list_b = b.carve<int32_t>(N + 1);
  w.refine = b.carve<int32_t>(N + 1);
  w.flags = b.carve<uint8_t>(N + 1);
  w.heads = b.carve<uint8_t>(N + 1);
  w.nxt0 = b.carve<int32_t>(N + 2);
  w.nj0 = b.carve<int32_t>(N + 2);
  w.nj1 = b.carve<int32_t>(N + 2);
  w.ret_key = b.carve<int64_t>(N + 1);
  w.counts = b.carve<int32_t>(64);
  w.scan = b.carve<unsigned long long>(1024);
  memset(w.counts, 0, sizeof(int32_t) * 64);
  memset(w.scan, 0, sizeof(unsigned long long) * 1024);
  w.atlas_limit = b.carve<long long>(1);
  {
    int32_t* p = b.carve<int32_t>((size_t)2 * 2 * 3 * (nb0 + nb1 + nb2 + 3));
    const int cnt[3] = {nb0 + 1, nb1 + 1, nb2 + 1};
    for (int l = 0; l < 2; l++)
      for (int lev = 0; lev < 3; lev++)
        for (int m = 0; m < 2; m++) {
          w.box[l][lev][m] = p;
          p += 3 * cnt[lev];
        }
  }
  w.pred_count = b.carve<int32_t>(N);
  w.pred_point = b.carve<int32_t>(3 * N);
  w.pred_dist2 = b.carve<uint64_t>(3 * N);
  w.pt2pred = b.carve<int32_t>(N);
  w.indexes = b.carve<int32_t>(N);
  int32_t* d_neigh_index = b.carve<int32_t>(3 * N);
  int32_t* d_weight = b.carve<int32_t>(3 * N);

  hipLaunchKernelGGL(
    lod_gather_pos_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n, xyz,
    (const int32_t*)d_order, lp->lod_neigh_bias[0], lp->lod_neigh_bias[1], lp->lod_neigh_bias[2],
    d_pos, d_bpos, w.list_a);
  std::vector<int32_t> npl;
  int scan_epoch = 0;
  if (lod_scalable_levels(
        lp, w, nullptr, &npl, &scan_epoch, min_geom_node_size_log2,
        (int64_t)geom_num_points - n)
      != hipSuccess)
    return -5;
  hipLaunchKernelGGL(
    lod_finalise_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n, 0, w.pred_count,
    (const int32_t*)w.pred_point, (const int32_t*)w.pt2pred, w.pred_dist2, d_neigh_index);
  hipLaunchKernelGGL(
    lod_compute_weights_kernel, dim3(lod_grid(n, 256)), dim3(256), 0, nullptr, n, w.pred_count,
    (const uint64_t*)w.pred_dist2, d_weight);
  memcpy(neigh_count, w.pred_count, sizeof(int32_t) * N);
  memcpy(neigh_index, d_neigh_index, sizeof(int32_t) * 3 * N);
  memcpy(neigh_weight, d_weight, sizeof(int32_t) * 3 * N);
  memcpy(indexes, w.indexes, sizeof(int32_t) * N);
  *num_lods = (int)npl.size();
  for (size_t i = 0; i < npl.size(); i++)
    num_points_in_lod[i] = npl[npl.size() - 1 - i];
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
