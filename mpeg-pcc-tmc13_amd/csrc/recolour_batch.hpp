// recolour_batch.hpp -- a batch of slices recoloured in one call, everything resident on the device
// (gpcc_dev_recolour_attrs): the k-d trees of all slices built as two FORESTS (recolour_kdtree.hpp:
// kd_init_forest_kernel, KdLevelLoop::begin_forest -- the sources' on the call's stream, the targets' on a second
// one, as the two trees of the host tier), the searches, lists and blends over the concatenated slices.
//
// The number of launches and of host waits does not depend on the number of slices.  A lane finds its slice in a
// small device table (RcBatchTab); what the reference has per slice is per slice here: target_to_source_offset,
// 1 / pointCountSource, 1 / pointCountTarget and, under a finite max_geometry_dist2_fwd, the first limited target
// (one word per slice: a limited target shrinks the results of the later targets of ITS slice only).  All
// arithmetic goes through the device functions of recolour_kernels.hpp / recolour_kdtree.hpp; neighbour indices
// are indices into the concatenated arrays, so the gathers need no translation.
//
// rcb_check (the argument checks, host only) and rcb_run (the stage sequence) are what the library entry
// (gpcc_attr_mi355.hip) and the emulator harness (tests/emu/rc_batch_emu_harness.cpp) both call; what differs
// between them -- where blocks come from, the second stream, pinned memory, profiling spans -- is the `Host`.
#pragma once

#include <string>
#include <vector>

#include "recolour_kernels.hpp"

namespace gpcc {

// the device's view of the batch's R non-empty slices
struct RcBatchTab {
  const int32_t* src_off;  // [R + 1] slice r's sources are [src_off[r], src_off[r + 1]) of the concatenated array
  const int32_t* tgt_off;  // [R + 1]
  const int32_t* off;      // [R][3] target_to_source_offset of every slice
  const double* src_box;   // [R][6] root box of slice r's source tree (root r of the source forest): lo[3], hi[3]
  const double* tgt_box;   // [R][6]
  int32_t R;
};

// The slice of element i of one side: looked up for the FIRST element of the lane's wavefront (the same loads in
// every lane: a wavefront that lies inside one slice stays uniform), then advanced lane by lane where a slice
// boundary falls inside the wavefront.  i < off[R].
__device__ __forceinline__ int
rc_slice_of(const int32_t* __restrict__ off, int R, int i)
{
  const int i0 = i & ~63;
  int lo = 0, hi = R;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i0)
      lo = mid;
    else
      hi = mid;
  }
  while (i >= off[lo + 1])
    lo++;
  return lo;
}

// rc_forward_attrs_kernel over the concatenated targets: the search starts at the root of the slice's source tree
template<int K, bool ALIMIT>
__global__ __launch_bounds__(256) GPCC_RC_OCCUPANCY void
rcb_forward_attrs_kernel(RcCtx cx, RcBatchTab tb, RcAttrs at)
{
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cx.tgt.n)
    return;
  const int sl = rc_slice_of(tb.tgt_off, tb.R, t);
  const gpcc_recolour_params& p = cx.p;
  const int kf = p.num_neighbours_fwd;
  const double max_a = rc_limit(p.max_attribute_dist2_fwd);
  const int32_t off[3] = {tb.off[3 * sl], tb.off[3 * sl + 1], tb.off[3 * sl + 2]};
  double q[3];
  rc_forward_query(cx.tgt.xyz, t, off, cx.t2s, q);
  RcKnn<K> r;
  rc_kd_search_from<K>(cx.src, sl, tb.src_box + 6 * sl, tb.src_box + 6 * sl + 3, q, kf, r);
  if (cx.nearest) {
    cx.nearest[t] = r.i[0];
    if (rc_worst(r, kf) > rc_limit(p.max_geometry_dist2_fwd))
      atomicMin(&cx.fwd_first[sl], t);
  }
  for (int a = 0; a < at.n; a++) {
    const RcAttr& A = at.a[a];
    if (A.c == 3)
      rc_forward_tail<3, K, ALIMIT>(p, r, A.src, A.ref1 + (size_t)t * 3, max_a, (double)A.clip_max);
    else
      rc_forward_tail<1, K, ALIMIT>(p, r, A.src, A.ref1 + t, max_a, (double)A.clip_max);
  }
}

// rc_forward_limit_attrs_kernel with the first limited target of the lane's OWN slice (cx.fwd_first: [R])
__global__ __launch_bounds__(256) void
rcb_forward_limit_attrs_kernel(RcCtx cx, RcBatchTab tb, RcAttrs at)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cx.tgt.n)
    return;
  const int sl = rc_slice_of(tb.tgt_off, tb.R, t);
  if (t < cx.fwd_first[sl])
    return;
  const int32_t s = cx.nearest[t];
  for (int a = 0; a < at.n; a++) {
    const RcAttr& A = at.a[a];
    for (int k = 0; k < A.c; k++)
      A.ref1[(size_t)t * A.c + k] = A.src[(size_t)s * A.c + k];
  }
}

// rc_backward_kernel over the concatenated sources: the search starts at the root of the slice's target tree
template<int K>
__global__ __launch_bounds__(256) GPCC_RC_OCCUPANCY void
rcb_backward_kernel(RcCtx cx, RcBatchTab tb)
{
#pragma clang fp contract(off)
  GPCC_VGPR_FLOOR_64();  // (<2> arrives at 50 registers: the 49..56 class of gpcc_primitives.hpp)
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cx.src.n)
    return;
  const int sl = rc_slice_of(tb.src_off, tb.R, s);
  const int kb = cx.p.num_neighbours_bwd;
  const double max_g = rc_limit(cx.p.max_geometry_dist2_bwd);
  const int32_t off[3] = {tb.off[3 * sl], tb.off[3 * sl + 1], tb.off[3 * sl + 2]};
  double q[3];
  rc_backward_query(cx.src.xyz, s, off, cx.s2t, q);
  RcKnn<K> r;
  rc_kd_search_from<K>(cx.tgt, sl, tb.tgt_box + 6 * sl, tb.tgt_box + 6 * sl + 3, q, kb, r);
#pragma unroll
  for (int i = 0; i < K; i++) {
    if (i < kb) {
      const bool ok = i < r.count && r.d[i] <= max_g;
      cx.bt[(size_t)s * kb + i] = ok ? r.i[i] : -1;
      cx.bd[(size_t)s * kb + i] = ok ? r.d[i] : 0.0;
      if (ok)
        atomicAdd(&cx.lstart[r.i[i] + 1], 1);
    }
  }
}

// rc_blend_attrs_kernel with the slice's own point counts (the lists themselves are global: a target's entries are
// sources of its own slice, rc_list_fill_kernel serves the batch as it is)
__global__ __launch_bounds__(256) void
rcb_blend_attrs_kernel(RcCtx cx, RcBatchTab tb, RcAttrs at)
{
#pragma clang fp contract(off)
  GPCC_VGPR_FLOOR_64();
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cx.tgt.n)
    return;
  const int l0 = cx.lstart[t];
  const int n = cx.lstart[t + 1] - l0;
  double* ld = cx.ldist + l0;
  int32_t* ls = cx.lsrc + l0;
  if (n == 0) {
    for (int a = 0; a < at.n; a++) {
      const RcAttr& A = at.a[a];
      for (int k = 0; k < A.c; k++)
        A.out[(size_t)t * A.c + k] = A.ref1[(size_t)t * A.c + k];
    }
    return;
  }
  rc_list_order(ld, ls, n);
  const int sl = rc_slice_of(tb.tgt_off, tb.R, t);
  const double r_source = 1.0 / (double)(tb.src_off[sl + 1] - tb.src_off[sl]);
  const double r_target = 1.0 / (double)(tb.tgt_off[sl + 1] - tb.tgt_off[sl]);
  for (int a = 0; a < at.n; a++) {
    const RcAttr& A = at.a[a];
    if (A.c == 3)
      rc_blend_tail<3>(cx.p, ld, ls, n, A.src, A.ref1 + (size_t)t * 3, A.out + (size_t)t * 3, (double)A.clip_max, r_source,
                       r_target);
    else
      rc_blend_tail<1>(cx.p, ld, ls, n, A.src, A.ref1 + t, A.out + t, (double)A.clip_max, r_source, r_target);
  }
}

// ---- host ----------------------------------------------------------------------------------
// the arguments of gpcc_dev_recolour_attrs
struct RcBatchIn {
  int32_t num_slices;
  const int64_t* src_off;  // host [S + 1]
  const int64_t* tgt_off;  // host [S + 1]
  const int32_t* d_src_xyz;
  const int32_t* d_tgt_xyz;
  const gpcc_dev_recolour_attr* attrs;
  int32_t num_attrs;
  float scale;
  const int32_t* offsets;  // host [S][3]
};

// The argument checks, from the offsets alone and ahead of any launch -> GPCC_OK or the refusal with its reason.
// GPCC_ERR_UNSUPPORTED (a slice with fewer points than neighbours asked for) only when nothing is invalid.
inline int
rcb_check(const gpcc_recolour_params* p, const RcBatchIn& in, std::string* why)
{
  auto refuse = [&](int code, const char* msg) {
    *why = msg;
    return code;
  };
  if (!in.attrs || in.num_attrs < 1 || in.num_attrs > GPCC_RC_MAX_ATTRS)
    return refuse(GPCC_ERR_INVALID_ARG, "attribute table is null or does not hold 1 .. GPCC_RC_MAX_ATTRS attributes");
  for (int a = 0; a < in.num_attrs; a++) {
    const gpcc_dev_recolour_attr& A = in.attrs[a];
    if (!A.d_src || !A.d_tgt || (A.c != 1 && A.c != 3))
      return refuse(GPCC_ERR_INVALID_ARG, "null attribute buffer or attribute count not 1 / 3");
    if (A.bitdepth < 1 || A.bitdepth > 16)
      return refuse(GPCC_ERR_INVALID_ARG, "bitdepth must be 1..16");
  }
  if (!p || !in.src_off || !in.tgt_off || !in.d_src_xyz || !in.d_tgt_xyz || !in.offsets || in.num_slices < 1)
    return refuse(GPCC_ERR_INVALID_ARG, "null buffer or no slice");
  const int kf = p->num_neighbours_fwd, kb = p->num_neighbours_bwd;
  if (kf < 1 || kf > kRcMaxK || kb < 1 || kb > kRcMaxK || p->search_range < 0 || !(in.scale > 0))
    return refuse(GPCC_ERR_INVALID_ARG, "neighbour counts must be 1..8, search range >= 0, scale > 0");
  const int S = in.num_slices;
  if (in.src_off[0] != 0 || in.tgt_off[0] != 0)
    return refuse(GPCC_ERR_INVALID_ARG, "offsets do not start at 0");
  for (int s = 0; s < S; s++)
    if (in.src_off[s + 1] < in.src_off[s] || in.tgt_off[s + 1] < in.tgt_off[s])
      return refuse(GPCC_ERR_INVALID_ARG, "offsets are not ascending");
  const int64_t ns = in.src_off[S], nt = in.tgt_off[S];
  if (ns > (1 << 27) || nt > (1 << 27))
    return refuse(GPCC_ERR_INVALID_ARG, "more than 2^27 points");
  if (ns <= 0 || nt <= 0)
    return refuse(GPCC_ERR_INVALID_ARG, "empty batch");
  for (int s = 0; s < S; s++)
    if ((in.src_off[s + 1] == in.src_off[s]) != (in.tgt_off[s + 1] == in.tgt_off[s]))
      return refuse(GPCC_ERR_INVALID_ARG, "a slice is empty on one side only");
  for (int a = 0; a < in.num_attrs; a++) {
    const uintptr_t a0 = (uintptr_t)in.attrs[a].d_tgt, a1 = a0 + sizeof(int32_t) * (size_t)in.attrs[a].c * (size_t)nt;
    for (int b = 0; b < a; b++) {
      const uintptr_t b0 = (uintptr_t)in.attrs[b].d_tgt, b1 = b0 + sizeof(int32_t) * (size_t)in.attrs[b].c * (size_t)nt;
      if (a0 < b1 && b0 < a1)
        return refuse(GPCC_ERR_INVALID_ARG, "two attributes name overlapping output buffers");
    }
    for (int b = 0; b < in.num_attrs; b++)
      if (in.attrs[a].d_tgt == in.attrs[b].d_src)
        return refuse(GPCC_ERR_INVALID_ARG, "an output buffer is a source buffer");
  }
  for (int s = 0; s < S; s++) {
    const int64_t n_s = in.src_off[s + 1] - in.src_off[s], n_t = in.tgt_off[s + 1] - in.tgt_off[s];
    if (n_s > 0 && (n_s < kf || n_t < kb))
      return refuse(GPCC_ERR_UNSUPPORTED, "a slice has fewer points than neighbours asked for");
  }
  return GPCC_OK;
}

// one forest's build: index array and nodes stay (work = false), the level loop's working set ends with the build.
// The sizes are one tree's (recolour_impl's kd_alloc) with the forest's capacities, derived at kd_forest_node_capacity.
template<class Host>
hipError_t
rcb_kd_carve(Host& host, KdBuild& b, const int32_t* d_xyz, int n, int roots)
{
  const size_t N = (size_t)n, M = 2 * N + 2;
  const size_t node_cap = kd_forest_node_capacity(N, (size_t)roots);
  b.t.xyz = d_xyz;
  b.t.n = n;
  b.roots = roots;
  b.node_cap = (int32_t)node_cap;
  struct Want {
    void** p;
    size_t bytes;
    bool work;
  };
  const Want want[] = {
    {(void**)&b.t.vind, sizeof(int32_t) * N, false},
    {(void**)&b.t.nodes, sizeof(KdNode) * node_cap, false},
    {(void**)&b.pnode, sizeof(int32_t) * N, true},
    {(void**)&b.rng, sizeof(int32_t) * 2 * M, true},
    {(void**)&b.parent, sizeof(int32_t) * M, true},
    {(void**)&b.box, sizeof(double) * 6 * M, true},
    {(void**)&b.mm, sizeof(int32_t) * 6 * M, true},
    {(void**)&b.cut, sizeof(double) * M, true},
    {(void**)&b.lim, sizeof(int32_t) * 2 * M, true},
    {(void**)&b.split, sizeof(int32_t) * M, true},
    {(void**)&b.flag, sizeof(int32_t) * (N + 1), true},
    {(void**)&b.tmp_l, sizeof(int32_t) * N, true},
    {(void**)&b.tmp_r, sizeof(int32_t) * N, true},
    {(void**)&b.sums, sizeof(long long) * ((N + 1) / kKdScanBlock + 2), true},
    {(void**)&b.counters, sizeof(int32_t) * 4, true},
    {(void**)&b.sub_list, sizeof(int32_t) * 2 * kd_forest_sub_capacity(N, (size_t)roots), true},
  };
  for (const Want& w : want) {
    const hipError_t e = host.take(w.bytes, w.p, w.work);
    if (e != hipSuccess)
      return e;
  }
  return hipSuccess;
}

// The stage sequence of a checked batch (rcb_check returned GPCC_OK).  Host:
//   hipError_t take(size_t bytes, void** out, bool work)   a device block; work: until end_work()
//   void end_work()
//   hipError_t upload(void* dst, const void* src, size_t bytes)   host table -> device, on the call's stream
//   hipError_t fork(hipStream_t* second) / join()   the second stream starts behind the call's stream / the
//                                                    call's stream goes on behind the second one
//   int32_t* counters()              host memory the device can copy to: 2 x 4 ints
//   int32_t* boxes(size_t ints)      ... the slices' bounding boxes
//   int fail(int code, const char* msg)
//   auto span(const char* name)      a profiling span that ends with the returned object
// Waits: one per level of the deeper forest, none behind the trees -- the blend is enqueued and the call returns.
// Nothing writes an output before the last check has passed.
template<class Host>
int
rcb_run(Host& host, const gpcc_recolour_params& p, const RcBatchIn& in, hipStream_t st)
{
#define RCB_TRY(expr)                                              \
  do {                                                             \
    const hipError_t e_ = (expr);                                  \
    if (e_ != hipSuccess)                                          \
      return host.fail(GPCC_ERR_HIP, hipGetErrorString(e_));       \
  } while (0)
  const int S = in.num_slices;
  const int ns = (int)in.src_off[S], nt = (int)in.tgt_off[S];
  const int kf = p.num_neighbours_fwd, kb = p.num_neighbours_bwd;
  // the non-empty slices: an empty one takes no room in the concatenated arrays
  int R = 0;
  for (int s = 0; s < S; s++)
    R += in.src_off[s + 1] > in.src_off[s] ? 1 : 0;
  std::vector<int32_t> h_tab(2 * ((size_t)R + 1) + 3 * (size_t)R);
  {
    int32_t *so = h_tab.data(), *to = so + R + 1, *off = to + R + 1;
    int r = 0;
    for (int s = 0; s < S; s++)
      if (in.src_off[s + 1] > in.src_off[s]) {
        so[r] = (int32_t)in.src_off[s];
        to[r] = (int32_t)in.tgt_off[s];
        for (int k = 0; k < 3; k++)
          off[3 * r + k] = in.offsets[3 * s + k];
        r++;
      }
    so[R] = ns;
    to[R] = nt;
  }
  int32_t *d_tab = nullptr, *d_bbox = nullptr;
  double* d_box = nullptr;
  RCB_TRY(host.take(sizeof(int32_t) * h_tab.size(), (void**)&d_tab, false));
  RCB_TRY(host.take(sizeof(double) * 12 * (size_t)R, (void**)&d_box, false));
  RCB_TRY(host.take(sizeof(int32_t) * 12 * (size_t)R, (void**)&d_bbox, false));
  RCB_TRY(host.upload(d_tab, h_tab.data(), sizeof(int32_t) * h_tab.size()));
  RcBatchTab tb{};
  tb.src_off = d_tab;
  tb.tgt_off = d_tab + R + 1;
  tb.off = d_tab + 2 * (R + 1);
  tb.src_box = d_box;
  tb.tgt_box = d_box + 6 * (size_t)R;
  tb.R = R;

  RcCtx cx{};
  cx.p = p;
  cx.s2t = (double)in.scale;
  cx.t2s = 1.0 / (double)in.scale;

  // ---- the two forests, built together: the sources' on the call's stream, the targets' on the second one ----
  {
    auto span = host.span("rc_kdtree");
    KdBuild ks{}, kt{};
    RCB_TRY(rcb_kd_carve(host, ks, in.d_src_xyz, ns, R));
    RCB_TRY(rcb_kd_carve(host, kt, in.d_tgt_xyz, nt, R));
    hipStream_t st2 = nullptr;
    RCB_TRY(host.fork(&st2));
    int32_t* h_cnt = host.counters();
    int32_t* h_bbox = host.boxes(12 * (size_t)R);
    if (!h_cnt || !h_bbox)
      return host.fail(GPCC_ERR_OUT_OF_MEMORY, "no host memory for the slices' bounding boxes");
    KdLevelLoop loop[2];
    RCB_TRY(loop[0].begin_forest(ks, tb.src_off, R, d_box, d_bbox, st, h_cnt));
    RCB_TRY(hipMemcpyAsync(h_bbox, d_bbox, sizeof(int32_t) * 6 * (size_t)R, hipMemcpyDeviceToHost, st));
    RCB_TRY(loop[1].begin_forest(kt, tb.tgt_off, R, d_box + 6 * (size_t)R, d_bbox + 6 * (size_t)R, st2, h_cnt + 4));
    RCB_TRY(hipMemcpyAsync(h_bbox + 6 * (size_t)R, d_bbox + 6 * (size_t)R, sizeof(int32_t) * 6 * (size_t)R,
                           hipMemcpyDeviceToHost, st2));
    bool first_wait = true;
    while (!loop[0].done() || !loop[1].done()) {
      for (int w = 0; w < 2; w++)
        if (!loop[w].done())
          RCB_TRY(loop[w].launch());
      for (int w = 0; w < 2; w++)
        if (!loop[w].done())
          RCB_TRY(loop[w].finish());
      if (first_wait) {
        // the build's first wait: every slice's bounding boxes have come down with the counters
        first_wait = false;
        for (size_t k = 0; k < 12 * (size_t)R; k++)
          if (h_bbox[k] <= -(1 << 30) || h_bbox[k] >= (1 << 30)) {
            host.join();
            return host.fail(GPCC_ERR_INVALID_ARG, "coordinates outside (-2^30, 2^30)");
          }
      }
    }
    RCB_TRY(host.join());
    for (int w = 0; w < 2; w++)
      if (loop[w].tree_depth() > kKdMaxDepth)
        return host.fail(GPCC_ERR_UNSUPPORTED, "a k-d tree deeper than 64 levels: the batch stays on the reference CPU path");
    cx.src = ks.t;
    cx.tgt = kt.t;
    host.end_work();
  }

  RcAttrs at{};
  at.n = in.num_attrs;
  for (int a = 0; a < in.num_attrs; a++) {
    at.a[a].src = (const int32_t*)in.attrs[a].d_src;
    at.a[a].out = (int32_t*)in.attrs[a].d_tgt;
    at.a[a].c = in.attrs[a].c;
    at.a[a].clip_max = (1 << in.attrs[a].bitdepth) - 1;
    RCB_TRY(host.take(sizeof(int32_t) * (size_t)in.attrs[a].c * nt, (void**)&at.a[a].ref1, false));
  }
  const size_t total_cap = (size_t)ns * kb;
  long long* d_sums = nullptr;
  RCB_TRY(host.take(sizeof(int32_t) * total_cap, (void**)&cx.bt, false));
  RCB_TRY(host.take(sizeof(double) * total_cap, (void**)&cx.bd, false));
  RCB_TRY(host.take(sizeof(int32_t) * ((size_t)nt + 1), (void**)&cx.lstart, false));
  RCB_TRY(host.take(sizeof(int32_t) * (size_t)nt, (void**)&cx.lcur, false));
  RCB_TRY(host.take(sizeof(double) * total_cap, (void**)&cx.ldist, false));
  RCB_TRY(host.take(sizeof(int32_t) * total_cap, (void**)&cx.lsrc, false));
  RCB_TRY(host.take(sizeof(long long) * (((size_t)nt + 1) / kKdScanBlock + 2), (void**)&d_sums, false));
  if (p.max_geometry_dist2_fwd < 512) {
    // finite forward geometry limit: nearest source point per target, the first limited target PER SLICE
    RCB_TRY(host.take(sizeof(int32_t) * ((size_t)nt + R), (void**)&cx.nearest, false));
    cx.fwd_first = cx.nearest + nt;
    RCB_TRY(hipMemsetAsync(cx.fwd_first, 0x7f, sizeof(int32_t) * (size_t)R, st));
  }

  // ---- forward, backward, lists, blend: one launch each for the batch ------------------------
  const int fgrid = (nt + 255) / 256, bgrid = (ns + 255) / 256;
  {
    auto span = host.span("rc_forward");
    const bool alimit = p.max_attribute_dist2_fwd < 512;
#define RCB_FWD(KK)                                                                                                          \
  do {                                                                                                                       \
    if (alimit)                                                                                                              \
      hipLaunchKernelGGL(HIP_KERNEL_NAME(rcb_forward_attrs_kernel<KK, true>), dim3(fgrid), dim3(256), 0, st, cx, tb, at);   \
    else                                                                                                                     \
      hipLaunchKernelGGL(HIP_KERNEL_NAME(rcb_forward_attrs_kernel<KK, false>), dim3(fgrid), dim3(256), 0, st, cx, tb, at);  \
  } while (0)
    switch (kf <= 1 ? 1 : kf <= 2 ? 2 : kf <= 4 ? 4 : 8) {
    case 1: RCB_FWD(1); break;
    case 2: RCB_FWD(2); break;
    case 4: RCB_FWD(4); break;
    default: RCB_FWD(8); break;
    }
#undef RCB_FWD
    if (cx.nearest)
      hipLaunchKernelGGL(rcb_forward_limit_attrs_kernel, dim3(fgrid), dim3(256), 0, st, cx, tb, at);
  }
  RCB_TRY(hipMemsetAsync(cx.lstart, 0, sizeof(int32_t) * ((size_t)nt + 1), st));
  RCB_TRY(hipMemsetAsync(cx.lcur, 0, sizeof(int32_t) * (size_t)nt, st));
  {
    auto span = host.span("rc_backward");
    switch (kb <= 1 ? 1 : kb <= 2 ? 2 : kb <= 4 ? 4 : 8) {
    case 1: hipLaunchKernelGGL(HIP_KERNEL_NAME(rcb_backward_kernel<1>), dim3(bgrid), dim3(256), 0, st, cx, tb); break;
    case 2: hipLaunchKernelGGL(HIP_KERNEL_NAME(rcb_backward_kernel<2>), dim3(bgrid), dim3(256), 0, st, cx, tb); break;
    case 4: hipLaunchKernelGGL(HIP_KERNEL_NAME(rcb_backward_kernel<4>), dim3(bgrid), dim3(256), 0, st, cx, tb); break;
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(rcb_backward_kernel<8>), dim3(bgrid), dim3(256), 0, st, cx, tb); break;
    }
  }
  {
    auto span = host.span("rc_lists");
    RCB_TRY(kd_scan(st, cx.lstart, (size_t)nt + 1, d_sums));
    hipLaunchKernelGGL(rc_list_fill_kernel, dim3(bgrid), dim3(256), 0, st, cx);
  }
  {
    auto span = host.span("rc_blend");
    hipLaunchKernelGGL(rcb_blend_attrs_kernel, dim3(fgrid), dim3(256), 0, st, cx, tb, at);
  }
  RCB_TRY(hipGetLastError());
  return GPCC_OK;
#undef RCB_TRY
}

}  // namespace gpcc
