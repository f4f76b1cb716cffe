// tests/emu/raht_marshal_emu_harness.cpp -- TEST INFRASTRUCTURE: the kernels of raht_marshal.hpp under the CPU
// wavefront emulator, launched through the launch functions dev_raht_attr (gpcc_attr_mi355.hip) calls, with the same
// tables: the batch's offsets as int32, the slices' region blocks as an array.  Guard bytes surround every array
// the kernels read or write.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip/hip_runtime.h"

#include "raht_marshal.hpp"

using namespace gpcc;

namespace {

constexpr size_t kGuardBytes = 64;  // in front of and behind every array
constexpr unsigned char kGuardByte = 0xCD;

// `bytes` bytes between two bands of guard bytes; an input is copied in
struct Guarded {
  unsigned char* raw;
  size_t bytes;
  explicit Guarded(size_t b, const void* init = nullptr) : bytes(b)
  {
    raw = (unsigned char*)aligned_alloc(256, (b + 2 * kGuardBytes + 255) & ~size_t(255));
    memset(raw, kGuardByte, b + 2 * kGuardBytes);
    if (init)
      memcpy(data(), init, b);
  }
  ~Guarded() { free(raw); }
  unsigned char* data() { return raw + kGuardBytes; }
  bool bands_intact() const
  {
    for (size_t i = 0; i < kGuardBytes; i++)
      if (raw[i] != kGuardByte || raw[kGuardBytes + bytes + i] != kGuardByte)
        return false;
    return true;
  }
  // an input: the bands and the content
  bool unchanged(const void* init) const { return bands_intact() && memcmp(raw + kGuardBytes, init, bytes) == 0; }
  // an array no launch may touch
  bool untouched() const
  {
    for (size_t i = 0; i < bytes; i++)
      if (raw[kGuardBytes + i] != kGuardByte)
        return false;
    return bands_intact();
  }
};

std::vector<int32_t>
table_of(int32_t num_slices, const int64_t* offsets)
{
  std::vector<int32_t> t((size_t)num_slices + 1);
  for (int s = 0; s <= num_slices; s++)
    t[s] = (int32_t)offsets[s];
  return t;
}

}  // namespace

// order [n]: slice-local; xyz [n][3], attrs [n][c]: point order; regions [num_slices] or null; attrs_too == 0: the
// decoder's launch (region offsets only).  out_sorted [n][c], out_qp [n][2].  Returns -2 when a guard byte has
// changed, an input has been written, or an output that this launch does not own has been touched.
extern "C" int
raht_marshal_emu_gather(
  int32_t num_slices, const int64_t* offsets, const gpcc_qp_regions* regions, const int32_t* order, const int32_t* xyz,
  const int32_t* attrs, int32_t c, int32_t attrs_too, int32_t* out_sorted, int32_t* out_qp)
{
  if (num_slices < 1 || c < 1 || c > 3)
    return -1;
  const size_t S = (size_t)num_slices, N = (size_t)offsets[num_slices];
  const std::vector<int32_t> pt = table_of(num_slices, offsets);
  Guarded g_pt(4 * (S + 1), pt.data()), g_reg(regions ? S * sizeof(gpcc_qp_regions) : 4, regions), g_order(4 * N, order),
    g_xyz(12 * N, xyz), g_attrs(4 * N * c, attrs), g_sorted(4 * N * c), g_qp(8 * N);
  MarshalArgs a{};
  a.pt_off = (const int32_t*)g_pt.data();
  a.regions = regions ? (const gpcc_qp_regions*)g_reg.data() : nullptr;
  a.order = (const int32_t*)g_order.data();
  a.xyz = (const int32_t*)g_xyz.data();
  a.point = (int32_t*)g_attrs.data();
  a.sorted = (int32_t*)g_sorted.data();
  a.qp_off = (int32_t*)g_qp.data();
  a.n = (int32_t)N;
  a.c = c;
  a.num_slices = num_slices;
  a.attrs = attrs_too;
  auto span = [](const char*) { return 0; };
  raht_gather_launch(nullptr, a, span);
  bool ok = g_pt.unchanged(pt.data()) && g_order.unchanged(order) && g_xyz.unchanged(xyz) && g_attrs.unchanged(attrs)
    && (regions ? g_reg.unchanged(regions) : g_reg.untouched());
  ok = ok && (attrs_too ? g_sorted.bands_intact() : g_sorted.untouched());
  ok = ok && (regions ? g_qp.bands_intact() : g_qp.untouched());
  memcpy(out_sorted, g_sorted.data(), 4 * N * c);
  memcpy(out_qp, g_qp.data(), 8 * N);
  return ok ? 0 : -2;
}

// sorted [n][c] in Morton order -> out_point [n][c] in point order, clipped to [0, clip_max]
extern "C" int
raht_marshal_emu_clip_scatter(
  int32_t num_slices, const int64_t* offsets, const int32_t* order, const int32_t* sorted, int32_t c, int32_t clip_max,
  int32_t* out_point)
{
  if (num_slices < 1 || c < 1 || c > 3)
    return -1;
  const size_t S = (size_t)num_slices, N = (size_t)offsets[num_slices];
  const std::vector<int32_t> pt = table_of(num_slices, offsets);
  Guarded g_pt(4 * (S + 1), pt.data()), g_order(4 * N, order), g_sorted(4 * N * c, sorted), g_point(4 * N * c);
  MarshalArgs a{};
  a.pt_off = (const int32_t*)g_pt.data();
  a.order = (const int32_t*)g_order.data();
  a.point = (int32_t*)g_point.data();
  a.sorted = (int32_t*)g_sorted.data();
  a.n = (int32_t)N;
  a.c = c;
  a.num_slices = num_slices;
  a.clip_max = clip_max;
  auto span = [](const char*) { return 0; };
  raht_clip_scatter_launch(nullptr, a, span);
  const bool ok = g_pt.unchanged(pt.data()) && g_order.unchanged(order) && g_sorted.unchanged(sorted) && g_point.bands_intact();
  memcpy(out_point, g_point.data(), 4 * N * c);
  return ok ? 0 : -2;
}
