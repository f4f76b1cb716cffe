// tests/emu/pred_repair_emu_harness.cpp -- TEST INFRASTRUCTURE: the predicting encoder with direct
// predictors as launch_pred (gpcc_attr_mi355.hip) runs it -- whole-slice passes, then the ordered
// walk of pred_walk_kernel over what they left undecided -- under the CPU wavefront emulator.
// The kernels are the library's (pred_kernels.hpp); the host-side decisions (when the walk takes
// over, whether it is complete) are the library's too (pred_repair.hpp).  One or three
// components, neighbours in a reference frame or not, any number of LoDs, one QP layer,
// per-point QP offsets.  The persistent kernels run as ONE workgroup; the inclusive scan the
// library runs on the device (rc_scan) is a host loop here.
#include <algorithm>
#include <cmath>
#include <vector>

#include "hip/hip_runtime.h"

#include "lod_scalable.hpp"
#include "pred_kernels.hpp"
#include "pred_repair.hpp"

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

const double*
log2_table()
{
  static std::vector<double> t;
  if (t.empty()) {
    t.resize((size_t)kRateScale + 1);
    for (int v = 0; v <= kRateScale; v++)
      t[v] = log2((double)v);
  }
  return t.data();
}

template<int C>
int
run(
  const gpcc_pred_params* p, int32_t n, const int32_t* nc, const int32_t* ni, const int32_t* nw, const int32_t* inter_ref,
  const int32_t* indexes, int32_t* attrs, const int32_t* attrs_ref, int32_t n_ref, int32_t repair_after, int32_t* values,
  int8_t* icp, int64_t* stats, const int32_t* qp_off)
{
  std::vector<void*> blocks;
  const size_t N = (size_t)n, NE = N + (size_t)n_ref;
  int32_t* d_ni = carve<int32_t>(&blocks, 3 * N);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < 3; j++)
      d_ni[3 * i + j] = ni[3 * i + j] + (n_ref > 0 && j < nc[i] && inter_ref[3 * i + j] ? n : 0);
  PredCtx cx{};
  cx.n = n;
  cx.c = C;
  cx.num_lods = p->num_lods;
  for (int l = 0; l < p->num_lods; l++)
    cx.npl[l] = p->num_points_in_lod[l];
  pred_fill_ranges(cx, p->num_points_in_lod, p->num_lods, p->num_qp_layers, n);
  cx.max_levels = p->max_num_detail_levels;
  cx.bitdepth = p->bitdepth;
  cx.num_qp_layers = p->num_qp_layers;
  memcpy(cx.layer_qp, p->layer_qp, sizeof(cx.layer_qp));
  cx.max_qp = p->max_qp;
  cx.max_direct = p->max_num_direct_predictors;
  cx.avg_disabled = p->direct_avg_predictor_disabled_flag != 0;
  cx.threshold = p->adaptive_prediction_threshold;
  cx.icp_enabled = C == 3 && p->inter_component_prediction_enabled_flag;
  for (int k = 0; k < 3; k++)
    cx.qnw[k] = p->quant_neigh_weight[k];
  cx.nc = nc;
  cx.ni = d_ni;
  cx.nw = nw;
  cx.indexes = indexes;
  cx.qp_off = qp_off;
  cx.attrs = attrs;
  cx.values = values;
  cx.icp = carve<int8_t>(&blocks, GPCC_MAX_LODS * 3);
  memset(cx.icp, 0, GPCC_MAX_LODS * 3);
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
  memset(cx.icp_sums, 0, sizeof(unsigned long long) * GPCC_MAX_LODS * 18);
  cx.tag = 1;
  cx.frame_attr = attrs_ref;
  auto grid = [&](int items) { return dim3(lod_grid(std::max(items, 1), 256)); };
  hipLaunchKernelGGL(pred_indegree_kernel, grid(n), dim3(256), 0, nullptr, cx);
  if (cx.qnw[0] || cx.qnw[1] || cx.qnw[2])
    hipLaunchKernelGGL(pred_quant_weights_kernel, dim3(1), dim3(256), 0, nullptr, cx);
  else
    for (int i = 0; i < n; i++)
      cx.qw[i] = 256;
  if (cx.icp_enabled) {
    hipLaunchKernelGGL(pred_icp_sums_kernel, dim3(std::min(lod_grid(n, 256), 1024)), dim3(256), 0, nullptr, cx);
    hipLaunchKernelGGL(pred_icp_resolve_kernel, dim3(1), dim3(64), 0, nullptr, cx);
  }
  int32_t* rm = carve<int32_t>(&blocks, 6 * N);
  int32_t* src_copy = carve<int32_t>(&blocks, N * C);
  int32_t* prev_values = carve<int32_t>(&blocks, N * C);
  int32_t* ev_rank = carve<int32_t>(&blocks, N + 1);
  uint8_t* ev_up = carve<uint8_t>(&blocks, N + 1);
  int32_t* ev_state = carve<int32_t>(&blocks, N + 1);
  int32_t* flag = small + 24;
  memcpy(src_copy, attrs, sizeof(int32_t) * N * C);
  cx.src = src_copy;
  cx.rm = rm;
  cx.log2tab = log2_table();
  auto dag = [&]() {
    if (n_ref > 0)
      hipLaunchKernelGGL((pred_dag_kernel<C, true, true>), dim3(1), dim3(256), 0, nullptr, cx);
    else
      hipLaunchKernelGGL((pred_dag_kernel<C, true, false>), dim3(1), dim3(256), 0, nullptr, cx);
  };
  auto scan = [&]() {
    for (size_t i = 1; i <= N; i++)
      ev_rank[i] += ev_rank[i - 1];
  };
  hipLaunchKernelGGL(pred_rate_init_kernel, grid(n), dim3(256), 0, nullptr, rm, n);
  // ---- launch_pred's loop ----
  const int after = repair_after > 0 ? std::min<int>(repair_after, kPredMaxPasses) : kPredRepairAfterDefault;
  bool settled = false;
  int passes = 0, differences = 0;
  for (int pass = 0; !settled && !differences; pass++) {
    passes++;
    cx.tag = (uint32_t)(pass + 1);
    memset(cx.ticket, 0, 8 * sizeof(int32_t));
    *flag = 0;
    dag();
    if (pred_repair_pass_lists(pass, after)) {
      hipLaunchKernelGGL(pred_diff_flags_kernel, grid(n), dim3(256), 0, nullptr, (const int32_t*)cx.values,
                         pass > 0 ? (const int32_t*)prev_values : (const int32_t*)nullptr, n, C, ev_rank);
      scan();
      differences = ev_rank[n];
      settled = differences == 0;
      break;
    }
    hipLaunchKernelGGL(pred_values_diff_kernel, grid(n), dim3(256), 0, nullptr, (const int32_t*)cx.values, prev_values,
                       N * C, flag);
    if (pass > 0 && !*flag) {
      settled = true;
      break;
    }
    const int chunks = n / kRateChunk + 1;
    for (int k = 0; k < C; k++) {
      hipLaunchKernelGGL(pred_rate_scan_kernel, dim3((chunks + 63) / 64), dim3(64), 0, nullptr, (const int32_t*)cx.values + k,
                         C, (const uint8_t*)nullptr, n, (const int32_t*)nullptr, rm + k, 6, 0);
      hipLaunchKernelGGL(pred_rate_flags_kernel, grid(n), dim3(256), 0, nullptr, (const int32_t*)cx.values, n, C, k, ev_rank);
      scan();
      hipLaunchKernelGGL(pred_rate_events_kernel, grid(n), dim3(256), 0, nullptr, (const int32_t*)cx.values, n, C, k,
                         (const int32_t*)ev_rank, ev_up);
      hipLaunchKernelGGL(pred_rate_scan_kernel, dim3((chunks + 63) / 64), dim3(64), 0, nullptr, (const int32_t*)nullptr, 0,
                         (const uint8_t*)ev_up, n, (const int32_t*)(ev_rank + n), ev_state, 1, 1);
      hipLaunchKernelGGL(pred_rate_gather_kernel, grid(n), dim3(256), 0, nullptr, (const int32_t*)ev_rank,
                         (const int32_t*)ev_state, n, k, rm);
    }
  }
  int rc = 0;
  stats[0] = passes;
  stats[1] = stats[2] = stats[3] = stats[4] = 0;
  stats[5] = stats[6] = -1;
  if (!settled) {
    PredWalk w{};
    w.rank = ev_rank;
    w.list = ev_state;
    w.changed = ev_up;
    w.out = small + 32;
    memset(ev_up, 0, N);
    memset(w.out, 0, 4 * sizeof(int32_t));
    hipLaunchKernelGGL(pred_diff_list_kernel, grid(n), dim3(256), 0, nullptr, (const int32_t*)ev_rank, n, ev_state);
    if (n_ref > 0)
      hipLaunchKernelGGL((pred_walk_kernel<C, true>), dim3(1), dim3(64), 0, nullptr, cx, w);
    else
      hipLaunchKernelGGL((pred_walk_kernel<C, false>), dim3(1), dim3(64), 0, nullptr, cx, w);
    if (!pred_repair_walk_complete(w.out, n, differences))
      rc = -9;
    stats[1] = differences;
    stats[2] = w.out[0];
    stats[3] = w.out[1];
    stats[4] = w.out[2];
    stats[5] = ev_state[0];
    stats[6] = ev_state[differences - 1];
  }
  if (*cx.error)
    rc = -7;
  memcpy(icp, cx.icp, GPCC_MAX_LODS * 3);
  for (void* b : blocks)
    free(b);
  return rc;
}
}  // namespace

// attrs [n][c] in: source, out: reconstruction (point order); values [n][c] out (coding order); icp [32][3] out;
// inter_ref / attrs_ref: null / n_ref = 0 without a reference frame; repair_after <= 0: the library's default;
// stats [7] out: passes, differences the walk started from, predictors walked, stretches, longest stretch, the first
// and the last difference (-1: the walk was not needed); qp_off [n][2] in point order: the per-point QP offsets of
// the slice's regions, or null
extern "C" int
pred_repair_emu_encode(
  const gpcc_pred_params* p, int32_t n, int32_t c, const int32_t* nc, const int32_t* ni, const int32_t* nw,
  const int32_t* inter_ref, const int32_t* indexes, int32_t* attrs, const int32_t* attrs_ref, int32_t n_ref,
  int32_t repair_after, int32_t* values, int8_t* icp, int64_t* stats, const int32_t* qp_off)
{
  if (n <= 0 || (c != 1 && c != 3) || p->max_num_direct_predictors < 1 || p->scalable_lifting_enabled_flag
      || (n_ref > 0 && c != 1))
    return -1;
  return c == 1 ? run<1>(p, n, nc, ni, nw, inter_ref, indexes, attrs, attrs_ref, n_ref, repair_after, values, icp, stats,
                         qp_off)
                : run<3>(p, n, nc, ni, nw, inter_ref, indexes, attrs, attrs_ref, n_ref, repair_after, values, icp, stats,
                         qp_off);
}

// the switch as the library reads it from its environment text
extern "C" int
pred_repair_emu_after_from_text(const char* s)
{
  return pred_repair_after_from_text(s);
}
