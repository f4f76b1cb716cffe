// lod_levels.hpp -- the host side of the LoD build (AttributeLods::generate /
// buildPredictorsFast, tmc3/PCCTMC3Common.h:2300-2469) around the kernels of
// lod_kernels.hpp: the device workspace of one build, stated once (lod_carve), and
// the build's stages -- gather, the level loop with its three sub-samplers and the
// nearest-neighbour search of every level, finalise / weights / blend.  The level
// loop under scalable lifting is lod_scalable.hpp's, over the same pieces.
//
// Launches are written with hipLaunchKernelGGL and the HIP runtime calls are the
// plain ones, nothing here knows a context: the library (lod_build_core) and the CPU
// wavefront emulator (tests/emu) compile this same text, so what the CPU tier pins
// against the oracle is the library's own loop.
//
// What differs between the two is a small policy object `host`:
//   host.span(name, level = -1)      an RAII timing scope (the library's Timer, with the
//                                    level in the name when one is given; nothing under
//                                    the emulator)
//   host.grid(items)                 workgroups of 256 threads for `items` work items
//   host.launch_subsample(lc, ncell) launches lod_subsample_distance_kernel, whose
//                                    workgroups wait for one another: resident ones on
//                                    the device, fibers that run together under the emulator
#pragma once

#include <algorithm>
#include <vector>

#include "gpcc_attr_mi355.h"
#include "lod_kernels.hpp"

namespace gpcc {

// device workspace of one LoD build: every array, carved by lod_carve
struct LodWork {
  int32_t n, n_frame;
  const int32_t* xyz;        // [n][3] positions in POINT order: xyz_own, or the caller's device copy
  int32_t* xyz_own;          // [n][3]
  int64_t* code;             // [n] sorted Morton codes
  int32_t* order;            // [n] point index of each sorted entry
  int32_t* pos;              // [n][3] sorted positions
  int32_t* bpos;             // [n][3] sorted positions * lodNeighBias
  int32_t* bpos_lod;         // [n][3] scalable lifting: node-corner positions of the LoD searched
  int32_t *list_a, *list_b;  // [n + 1] input / retained, ping-pong
  int32_t* refine;           // [n + 1] coding-order list of packed indices
  uint8_t *flags, *heads;    // [n + 1]
  // cells of the distance sub-sampler
  int32_t* positions;        // [n + 1]
  int32_t* cell_first;       // [n + 2]
  int32_t* cent_tmp;         // [n + 2]
  int64_t* cell_key;         // [n + 1]
  uint32_t* cell_state;      // [n + 1][4]
  // group pointers of the centroid / octree sub-samplers (next, and the two squared pointers): no level
  // runs both kinds of sub-sampler, so lod_carve lays them over cell_first, positions and cent_tmp
  int32_t *nxt0, *nj0, *nj1;
  int64_t* ret_key;          // [n + 1]
  int32_t* small;            // [64] words, see kLodTicket ..
  int32_t* counts;           // [2] of the partition kernel: small + kLodCounts
  unsigned long long* scan;  // [1024]
  long long* atlas_limit;
  int32_t* box[2][3][2];     // [list 0 = retained, 1 = refine][level][min/max]
  int32_t *pred_count, *pred_point;
  uint64_t* pred_dist2;
  int32_t *pt2pred, *indexes;
  // results
  int32_t* neigh_index;      // [n][3]
  int32_t* weight;           // [n][3]
  int32_t* inter_ref;        // [n][3] with a frame
  // the reference frame of attribute inter prediction, sorted as the points are
  int32_t* fxyz;             // [n_frame][3] point order
  int64_t* fcode;
  int32_t *forder, *fpos, *fbpos, *flist;
  int32_t* fbox[3][2];
};

// words of LodWork::small
constexpr int kLodTicket = 0;  // [8] of the distance sub-sampler
constexpr int kLodError = 8;   // its sticky error word
constexpr int kLodCounts = 16; // [2] of the partition kernel
constexpr int kLodMoved = 24;  // points out of Morton order (lod_count_moved_kernel)

// search parameters of an inter build (null = intra)
struct LodFrameParams {
  int32_t search_range;    // abh.attrInterPredSearchRange: replaces both LoD search ranges
  int32_t frame_distance;  // AttributeInterPredParams::frameDistance
};

inline int
lod_grid(int64_t items, int per_block)
{
  int64_t g = (items + per_block - 1) / per_block;
  g = std::min<int64_t>(std::max<int64_t>(g, 1), 1 << 16);
  return (int)g;
}

// the loop under scalable lifting times itself as a whole
struct LodQuietHost {
  struct Span {};
  Span span(const char*, int = -1) const { return {}; }
  int grid(int64_t items) const { return lod_grid(items, 256); }
};

#define GPCC_LODS_TRY(expr)     \
  do {                          \
    hipError_t e_ = (expr);     \
    if (e_ != hipSuccess)       \
      return e_;                \
  } while (0)

// three box levels (32 entries, 32 x 32, the rest) over a list of up to `cnt` entries: [level][min/max][3]
inline size_t
lod_box_words(int cnt)
{
  const int b0 = (cnt + 31) >> 5, b1 = (b0 + 31) >> 5, b2 = (b1 + 31) >> 5;
  return (size_t)2 * 3 * (b0 + b1 + b2 + 3);
}

inline int32_t*
lod_box_layout(int32_t* p, int cnt, int32_t* box[3][2])
{
  const int b0 = (cnt + 31) >> 5, b1 = (b0 + 31) >> 5, b2 = (b1 + 31) >> 5;
  const int per[3] = {b0 + 1, b1 + 1, b2 + 1};
  size_t o = 0;
  for (int lev = 0; lev < 3; lev++)
    for (int m = 0; m < 2; m++) {
      box[lev][m] = p ? p + o : nullptr;
      o += (size_t)3 * per[lev];
    }
  return p ? p + o : nullptr;
}

// The arrays of a build and their sizes.  take(bytes) -> char* (null while a caller only measures).
template<class Take>
void
lod_carve(Take&& take, LodWork& w, int n, int n_frame, bool scalable)
{
  const size_t N = (size_t)n, NF = (size_t)n_frame;
  w.n = n;
  w.n_frame = n_frame;
#define GPCC_LOD_TAKE(field, count) w.field = (decltype(w.field))take(sizeof(*w.field) * (count))
  GPCC_LOD_TAKE(xyz_own, 3 * N);
  GPCC_LOD_TAKE(code, N);
  GPCC_LOD_TAKE(order, N);
  GPCC_LOD_TAKE(pos, 3 * N);
  GPCC_LOD_TAKE(bpos, 3 * N);
  GPCC_LOD_TAKE(list_a, N + 1);
  GPCC_LOD_TAKE(list_b, N + 1);
  GPCC_LOD_TAKE(refine, N + 1);
  GPCC_LOD_TAKE(flags, N + 1);
  GPCC_LOD_TAKE(heads, N + 1);
  GPCC_LOD_TAKE(positions, N + 1);
  GPCC_LOD_TAKE(cell_first, N + 2);
  GPCC_LOD_TAKE(cent_tmp, N + 2);
  GPCC_LOD_TAKE(cell_key, N + 1);
  GPCC_LOD_TAKE(ret_key, N + 1);
  GPCC_LOD_TAKE(cell_state, 4 * (N + 1));
  GPCC_LOD_TAKE(small, 64);
  GPCC_LOD_TAKE(scan, 1024);
  GPCC_LOD_TAKE(atlas_limit, 1);
  int32_t* boxes = (int32_t*)take(sizeof(int32_t) * 2 * lod_box_words(n));
  lod_box_layout(lod_box_layout(boxes, n, w.box[0]), n, w.box[1]);
  GPCC_LOD_TAKE(pred_count, N);
  GPCC_LOD_TAKE(pred_point, 3 * N);
  GPCC_LOD_TAKE(pred_dist2, 3 * N);
  GPCC_LOD_TAKE(pt2pred, N);
  GPCC_LOD_TAKE(indexes, N);
  GPCC_LOD_TAKE(neigh_index, 3 * N);
  GPCC_LOD_TAKE(weight, 3 * N);
  GPCC_LOD_TAKE(bpos_lod, scalable ? 3 * N : 1);
  GPCC_LOD_TAKE(fxyz, 3 * NF + 1);
  GPCC_LOD_TAKE(fcode, NF + 1);
  GPCC_LOD_TAKE(forder, NF + 1);
  GPCC_LOD_TAKE(fpos, 3 * NF + 1);
  GPCC_LOD_TAKE(fbpos, 3 * NF + 1);
  GPCC_LOD_TAKE(flist, NF + 1);
  lod_box_layout((int32_t*)take(sizeof(int32_t) * (lod_box_words(n_frame) + 1)), n_frame, w.fbox);
  GPCC_LOD_TAKE(inter_ref, n_frame ? 3 * N : 1);
#undef GPCC_LOD_TAKE
  w.xyz = w.xyz_own;
  w.nxt0 = w.cell_first;
  w.nj0 = w.positions;
  w.nj1 = w.cent_tmp;
  w.counts = w.small ? w.small + kLodCounts : nullptr;
}
constexpr int kLodCarveTakes = 36;  // take() calls above: as many guard bands per build

template<class Host>
void
lod_build_boxes(
  int32_t* const box[3][2], const int32_t* list, int cnt, const int32_t* bpos, hipStream_t st, Host& host)
{
  const int c0 = (cnt + 31) >> 5, c1 = (c0 + 31) >> 5;
  {
    auto tm = host.span("lod_boxes");
    hipLaunchKernelGGL(
      lod_box0_kernel, dim3(host.grid(std::max(c0, 1))), dim3(256), 0, st, cnt, list, bpos, box[0][0], box[0][1]);
  }
  {
    auto tm = host.span("lod_boxes");
    hipLaunchKernelGGL(
      lod_box_up_kernel, dim3(host.grid(std::max(c1, 1))), dim3(256), 0, st, c0, (const int32_t*)box[0][0],
      (const int32_t*)box[0][1], box[1][0], box[1][1]);
  }
  {
    auto tm = host.span("lod_boxes");
    hipLaunchKernelGGL(
      lod_box_up_kernel, dim3(1), dim3(256), 0, st, c1, (const int32_t*)box[1][0], (const int32_t*)box[1][1],
      box[2][0], box[2][1]);
  }
}

// list[0, cnt) split by flags into out_true / out_false (either may be null) -> *n_true
template<class Host>
hipError_t
lod_partition(
  const LodWork& w, int cnt, const uint8_t* flags, const int32_t* list, int32_t* out_true, int32_t* out_false,
  hipStream_t st, int* scan_epoch, int* n_true, Host& host)
{
  (*scan_epoch)++;
  const int grid = (int)std::min<int64_t>(1024, ((int64_t)cnt + 1023) / 1024);
  {
    auto tm = host.span("lod_partition");
    hipLaunchKernelGGL(
      lod_partition_kernel, dim3(std::max(grid, 1)), dim3(256), 0, st, cnt, flags, list, out_true, out_false,
      w.counts, w.scan, *scan_epoch);
  }
  int32_t h = 0;
  GPCC_LODS_TRY(hipMemcpyAsync(&h, w.counts, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  GPCC_LODS_TRY(hipStreamSynchronize(st));
  *n_true = h;
  return hipSuccess;
}

// subsampleByCentroid (:2088-2143) / subsampleByOctree (:2146-2194) -> lc.flags: groups of `period`
// nodes of size 2^node_log2; group starts = orbit of 0 under next(), by pointer doubling
template<class Host>
hipError_t
lod_centroid_flags(
  const LodWork& w, const LodCtx& lc, int period, int node_log2, int backward, hipStream_t st, Host& host)
{
  const int n_in = lc.n_in;
  int32_t* nj[2] = {w.nj0, w.nj1};  // squared pointers
  auto tm = host.span("lod_centroid");
  hipLaunchKernelGGL(
    lod_centroid_next_kernel, dim3(host.grid(n_in + 1)), dim3(256), 0, st, lc, period, w.nxt0);
  GPCC_LODS_TRY(hipMemsetAsync(w.heads, 0, (size_t)n_in + 1, st));
  GPCC_LODS_TRY(hipMemsetAsync(w.heads, 1, 1, st));
  const int32_t* cur = w.nxt0;
  for (int r = 0, reach = 1; reach < n_in; r++, reach *= 2) {
    hipLaunchKernelGGL(
      lod_centroid_jump_kernel, dim3(host.grid(n_in + 1)), dim3(256), 0, st, n_in, cur, nj[r & 1], w.heads);
    cur = nj[r & 1];
  }
  hipLaunchKernelGGL(
    lod_centroid_pick_kernel, dim3(host.grid(n_in)), dim3(256), 0, st, lc, node_log2,
    (const int32_t*)w.nxt0, (const uint8_t*)w.heads, backward);
  return hipSuccess;
}

// Nearest neighbours of the layer [start, start + n_ref) of the coding-order list at LoD `level`
// against the retained list `ret`.  The caller has set nc.shift3, .boundary, the search ranges,
// with a frame .frame_range and .frame_boundary, and under scalable lifting .bpos, .pos,
// .node_mask, .unit_bias and .prune_dist; the rest comes from the workspace and `lp`.
template<class Host>
hipError_t
lod_search_layer(
  NnCtx nc, const gpcc_lod_params* lp, const LodWork& w, int level, int start, int n_ref, const int32_t* ret,
  int n_ret, bool scalable, bool inter, hipStream_t st, Host& host)
{
  nc.n = w.n;
  nc.code = w.code;
  nc.order = w.order;
  if (!nc.bpos)
    nc.bpos = w.bpos;
  nc.retained = ret;
  nc.ret_key = w.ret_key;
  nc.n_ret = n_ret;
  nc.refine = w.refine + start;
  nc.n_ref = n_ref;
  nc.start = start;
  nc.distribution = lp->prediction_with_distribution_enabled;
  nc.intra = level >= lp->intra_lod_prediction_skip_layers;
  nc.max_neigh = lp->num_pred_nearest_neighbours_minus1 + 1;
  for (int lev = 0; lev < 3; lev++)
    for (int m = 0; m < 2; m++) {
      nc.box_ret[lev][m] = w.box[0][lev][m];
      nc.box_ref[lev][m] = w.box[1][lev][m];
      if (inter)
        nc.box_frame[lev][m] = w.fbox[lev][m];
    }
  if (inter) {
    nc.frame_code = w.fcode;
    nc.frame_order = w.forder;
    nc.frame_bpos = w.fbpos;
    nc.frame_identity = w.flist;
    nc.n_frame = w.n_frame;
  }
  nc.atlas_limit = w.atlas_limit;
  nc.pred_count = w.pred_count;
  nc.pred_point = w.pred_point;
  nc.pred_dist2 = w.pred_dist2;
  nc.pt2pred = w.pt2pred;
  nc.indexes = w.indexes;
  if (n_ret > 0) {
    hipLaunchKernelGGL(
      lod_ret_keys_kernel, dim3(host.grid(n_ret)), dim3(256), 0, st, n_ret, ret, (const int64_t*)w.code, nc.shift3,
      w.ret_key);
    lod_build_boxes(w.box[0], ret, n_ret, nc.bpos, st, host);
  }
  if (nc.intra)
    lod_build_boxes(w.box[1], w.refine + start, n_ref, nc.bpos, st, host);
  // (the host value is read when the call returns only for pageable memory of
  // this size: a stack variable is copied before hipMemcpyAsync returns)
  const long long inf = INT64_MAX;
  GPCC_LODS_TRY(hipMemcpyAsync(w.atlas_limit, &inf, sizeof(inf), hipMemcpyHostToDevice, st));
  if (n_ret > 0) {
    auto tm = host.span("lod_atlas_limit");
    hipLaunchKernelGGL(lod_atlas_limit_kernel, dim3(host.grid(n_ret)), dim3(256), 0, st, nc, w.atlas_limit);
  }
  {
    auto tm = host.span("lod_nn_search", level);
    if (scalable)
      hipLaunchKernelGGL(lod_nn_search_kernel<true>, dim3(host.grid(n_ref)), dim3(256), 0, st, nc);
    else if (inter)
      hipLaunchKernelGGL(
        HIP_KERNEL_NAME(lod_nn_search_kernel<false, true>), dim3(host.grid(n_ref)), dim3(256), 0, st, nc);
    else
      hipLaunchKernelGGL(lod_nn_search_kernel<false>, dim3(host.grid(n_ref)), dim3(256), 0, st, nc);
  }
  return hipGetLastError();
}

// The level loop without scalable lifting: sub-sampling by distance (lod_decimation_type 0),
// periodic (1) or by centroid (2), then the search of the level's refinement points.
// -> cumulative sizes in `npl` as the reference pushes them (n first, then the retained count of
// every level that retains).  `npl` left empty: a lod_sampling_period < 1 at a level the loop
// came to, which the caller refuses.
template<class Host>
hipError_t
lod_plain_levels(
  const gpcc_lod_params* lp, const LodWork& w, const LodFrameParams* frame, hipStream_t st,
  std::vector<int32_t>* npl, int* scan_epoch, Host& host)
{
  const int n = w.n;
  const int max_levels = lp->num_detail_levels_minus1 + 1;
  npl->clear();
  npl->push_back(n);
  int32_t* d_input = w.list_a;
  int32_t* d_ret = w.list_b;
  int n_in = n, n_idx = 0;
  for (int lod = 0; n_in > 0 && lod < max_levels; lod++) {
    const int start = n_idx;
    int n_ret = 0, n_ref = 0;
    const int shift_bits0 = lp->dist2 + lp->attr_dist2_delta + lod;
    if (lod == max_levels - 1 || (lp->lod_decimation_type != 1 && n_in == 1)) {
      GPCC_LODS_TRY(
        hipMemcpyAsync(w.refine + start, d_input, sizeof(int32_t) * n_in, hipMemcpyDeviceToDevice, st));
      n_ref = n_in;
    } else {
      if (lp->lod_decimation_type == 1) {
        const int period = lp->lod_sampling_period[lod];
        if (period < 1) {
          npl->clear();
          return hipSuccess;
        }
        hipLaunchKernelGGL(
          lod_flag_periodic_kernel, dim3(host.grid(n_in)), dim3(256), 0, st, n_in, period, w.flags);
      } else if (lp->lod_decimation_type == 2) {
        const int period = lp->lod_sampling_period[lod];
        if (period < 1) {
          npl->clear();
          return hipSuccess;
        }
        LodCtx lc{};
        lc.code = w.code;
        lc.pos = w.pos;
        lc.input = d_input;
        lc.n_in = n_in;
        lc.shift3 = 3 * (shift_bits0 + 1);
        lc.flags = w.flags;
        GPCC_LODS_TRY(lod_centroid_flags(w, lc, period, shift_bits0, 1, st, host));
      } else {
        LodCtx lc{};
        lc.n = n;
        lc.code = w.code;
        lc.order = w.order;
        lc.pos = w.pos;
        lc.bpos = w.bpos;
        lc.input = d_input;
        lc.n_in = n_in;
        lc.shift3 = 3 * (shift_bits0 + 1);
        lc.boundary = std::min(63, lc.shift3 + 21);
        lc.radius2 = (int64_t)3 << (shift_bits0 << 1);
        lc.cell_first = w.cell_first;
        lc.cell_key = w.cell_key;
        lc.cell_state = w.cell_state;
        lc.ticket = w.small + kLodTicket;
        lc.error = w.small + kLodError;
        lc.epoch = lod + 1;
        lc.flags = w.flags;
        {
          auto tm = host.span("lod_cell_heads");
          hipLaunchKernelGGL(
            lod_flag_cell_heads_kernel, dim3(host.grid(n_in)), dim3(256), 0, st, lc, w.heads, w.positions);
        }
        int ncell = 0;
        GPCC_LODS_TRY(lod_partition(
          w, n_in, w.heads, w.positions, w.cell_first, (int32_t*)nullptr, st, scan_epoch, &ncell, host));
        GPCC_LODS_TRY(
          hipMemcpyAsync(w.cell_first + ncell, &n_in, sizeof(int32_t), hipMemcpyHostToDevice, st));
        GPCC_LODS_TRY(hipMemsetAsync(w.small + kLodTicket, 0, sizeof(int32_t) * 8, st));
        lc.ncell = ncell;
        hipLaunchKernelGGL(lod_cell_keys_kernel, dim3(host.grid(ncell)), dim3(256), 0, st, lc);
        {
          auto tm = host.span("lod_subsample", lod);
          host.launch_subsample(lc, ncell);
        }
      }
      GPCC_LODS_TRY(
        lod_partition(w, n_in, w.flags, d_input, d_ret, w.refine + start, st, scan_epoch, &n_ret, host));
      n_ref = n_in - n_ret;
    }
    n_idx += n_ref;

    // nearest neighbours of this LoD's refinement points
    if (n_ref > 0) {
      NnCtx nc{};
      nc.shift3 = 3 * (1 + shift_bits0);
      nc.boundary = std::min(63, nc.shift3 + 21);
      nc.range_inter = frame ? frame->search_range : lp->inter_lod_search_range;
      nc.range_intra = frame ? frame->search_range : lp->intra_lod_search_range;
      if (frame) {
        nc.frame_range = frame->search_range;
        nc.frame_boundary = std::min(63, nc.shift3 + 9);
      }
      GPCC_LODS_TRY(
        lod_search_layer(nc, lp, w, lod, start, n_ref, d_ret, n_ret, false, frame != nullptr, st, host));
    }
    if (n_ret > 0)
      npl->push_back(n_ret);
    std::swap(d_input, d_ret);
    n_in = n_ret;
  }
  return hipSuccess;
}

// sorted and biased positions and the list 0, 1, 2, ... of the points (w.code / w.order hold their Morton order)
template<class Host>
void
lod_prepare(const gpcc_lod_params* lp, const LodWork& w, hipStream_t st, Host& host)
{
  auto tm = host.span("lod_gather");
  hipLaunchKernelGGL(
    lod_gather_pos_kernel, dim3(host.grid(w.n)), dim3(256), 0, st, w.n, w.xyz, (const int32_t*)w.order,
    lp->lod_neigh_bias[0], lp->lod_neigh_bias[1], lp->lod_neigh_bias[2], w.pos, w.bpos, w.list_a);
}

// the same of the reference frame (w.fxyz, w.fcode / w.forder) and one box hierarchy over it
// (buildPredictorsFast :2352-2376, computeNearestNeighbors :1270-1292) -- the same at every level of detail
template<class Host>
void
lod_prepare_frame(const gpcc_lod_params* lp, const LodWork& w, hipStream_t st, Host& host)
{
  hipLaunchKernelGGL(
    lod_gather_pos_kernel, dim3(host.grid(w.n_frame)), dim3(256), 0, st, w.n_frame, (const int32_t*)w.fxyz,
    (const int32_t*)w.forder, lp->lod_neigh_bias[0], lp->lod_neigh_bias[1], lp->lod_neigh_bias[2], w.fpos, w.fbpos,
    w.flist);
  lod_build_boxes(w.fbox, w.flist, w.n_frame, w.fbpos, st, host);
}

// predictor order, weights and -- predicting transform with pred_weight_blending -- their blend
template<class Host>
hipError_t
lod_finish(const gpcc_lod_params* lp, const LodWork& w, const LodFrameParams* frame, hipStream_t st, Host& host)
{
  const int n = w.n;
  const dim3 grid(host.grid(n));
  {
    auto tm = host.span("lod_finalise");
    if (frame)
      hipLaunchKernelGGL(
        lod_finalise_inter_kernel, grid, dim3(256), 0, st, n, w.pred_count, (const int32_t*)w.pred_point,
        (const int32_t*)w.pt2pred, w.pred_dist2, w.neigh_index, w.inter_ref, frame->frame_distance);
    else
      hipLaunchKernelGGL(
        lod_finalise_kernel, grid, dim3(256), 0, st, n, 0, w.pred_count, (const int32_t*)w.pred_point,
        (const int32_t*)w.pt2pred, w.pred_dist2, w.neigh_index);
  }
  hipLaunchKernelGGL(
    lod_compute_weights_kernel, grid, dim3(256), 0, st, n, w.pred_count, (const uint64_t*)w.pred_dist2, w.weight);
  if (lp->attr_encoding == 1 && lp->pred_weight_blending_enabled_flag) {
    if (frame)
      hipLaunchKernelGGL(
        lod_blend_weights_inter_kernel, grid, dim3(256), 0, st, n, (const int32_t*)w.pred_count,
        (const int32_t*)w.pred_point, w.xyz, (const int32_t*)w.fxyz, w.weight);
    else
      hipLaunchKernelGGL(
        lod_blend_weights_kernel, grid, dim3(256), 0, st, n, (const int32_t*)w.pred_count,
        (const int32_t*)w.pred_point, w.xyz, w.weight);
  }
  return hipGetLastError();
}

}  // namespace gpcc
