// tests/emu/ref_crop_emu_harness.cpp -- TEST INFRASTRUCTURE: the kernels of ref_crop.hpp (with the bounding-box
// kernel of spherical.hpp and the scan of recolour_kdtree.hpp) under the CPU wavefront emulator, launched as
// dev_ref_crop (gpcc_attr_mi355.hip) launches them: the same tables, the same two launch functions with the
// host's look at the offsets between them.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip/hip_runtime.h"

#include "ref_crop.hpp"

using namespace gpcc;

// xyz [offsets[num_slices]][3]: the current slices; frame_xyz [n_frame][3], frame_attrs [n_frame][c];
// out_xyz [capacity][3], out_attrs [capacity][c]; ref_offsets [num_slices + 1]; bbox [num_slices][6];
// *error: the sticky word.  misalign: the frame's and the output's arrays start this many int32 behind a
// 16-byte boundary (0: the wide loads are taken).  Returns 1 when the capacity is too small (nothing written),
// -2 when a guard word around the outputs has changed.
extern "C" int
ref_crop_emu(
  int32_t num_slices, const int64_t* offsets, const int32_t* xyz, int32_t n_frame, const int32_t* frame_xyz,
  const int32_t* frame_attrs, int32_t c, int32_t* out_xyz, int32_t* out_attrs, int64_t capacity, int64_t* ref_offsets,
  int32_t* bbox, int32_t* error, int32_t misalign)
{
  if (num_slices < 1 || n_frame < 1 || c < 1 || c > 3 || misalign < 0 || misalign > 3)
    return -1;
  std::vector<int32_t> meta(2 * ((size_t)num_slices + 1));
  int32_t* h_pt = meta.data();
  int32_t* h_tile = meta.data() + num_slices + 1;
  h_tile[0] = 0;
  for (int s = 0; s <= num_slices; s++)
    h_pt[s] = (int32_t)offsets[s];
  for (int s = 0; s < num_slices; s++)
    h_tile[s + 1] = h_tile[s] + rpl_tiles(offsets[s + 1] - offsets[s]);

  // guard words around the arrays: a store outside shows
  auto alloc = [&](size_t words) {
    const size_t bytes = ((sizeof(int32_t) * (words + 4 + 16)) + 255) & ~size_t(255);
    int32_t* p = (int32_t*)aligned_alloc(256, bytes);
    memset(p, 0xCD, bytes);
    return p;
  };
  const size_t cap = (size_t)capacity;
  int32_t* raw_fx = alloc(3 * (size_t)n_frame);
  int32_t* raw_ox = alloc(3 * cap);
  int32_t* raw_oa = alloc((size_t)c * cap);
  int32_t* d_fx = raw_fx + misalign;
  int32_t* d_ox = raw_ox + misalign;
  int32_t* d_oa = raw_oa + misalign;
  memcpy(d_fx, frame_xyz, sizeof(int32_t) * 3 * n_frame);

  std::vector<int32_t> counts(ref_crop_count_entries(num_slices, n_frame), -1), off32((size_t)num_slices + 1, -1);
  std::vector<long long> sums(ref_crop_sum_entries(num_slices, n_frame));
  RplArgs sl{};
  sl.src = xyz;
  sl.pt_off = h_pt;
  sl.tile_off = h_tile;
  sl.num_slices = num_slices;
  sl.num_tiles = h_tile[num_slices];
  RefCropArgs a{};
  a.xyz_frame = d_fx;
  a.attrs_frame = frame_attrs;
  a.bbox = bbox;
  a.counts = counts.data();
  a.offsets = off32.data();
  a.xyz_ref = d_ox;
  a.attrs_ref = d_oa;
  a.error = error;
  a.n_frame = n_frame;
  a.c = c;
  a.num_slices = num_slices;
  a.num_tiles = ref_crop_tiles(n_frame);
  auto span = [](const char*) { return 0; };
  ref_crop_count_launch(nullptr, sl, a, sums.data(), span);
  for (int s = 0; s <= num_slices; s++)
    ref_offsets[s] = off32[s];
  int rc = 0;
  if (ref_offsets[num_slices] > capacity)
    rc = 1;
  else if (ref_offsets[num_slices] > 0)
    ref_crop_scatter_launch(nullptr, a, span);

  const size_t kept = rc ? 0 : (size_t)ref_offsets[num_slices];
  for (int i = 0; i < 16; i++)
    if (d_ox[3 * (rc ? 0 : cap) + i] != (int32_t)0xCDCDCDCD || d_oa[c * (rc ? 0 : cap) + i] != (int32_t)0xCDCDCDCD)
      rc = rc == 1 ? -2 : (rc ? rc : -2);
  // (behind the points kept nothing is written either)
  for (size_t i = 3 * kept; i < 3 * cap; i++)
    if (d_ox[i] != (int32_t)0xCDCDCDCD)
      rc = -2;
  for (size_t i = c * kept; i < c * cap; i++)
    if (d_oa[i] != (int32_t)0xCDCDCDCD)
      rc = -2;
  for (int i = 0; i < misalign; i++)
    if (raw_ox[i] != (int32_t)0xCDCDCDCD || raw_oa[i] != (int32_t)0xCDCDCDCD)
      rc = -2;
  memcpy(out_xyz, d_ox, sizeof(int32_t) * 3 * kept);
  memcpy(out_attrs, d_oa, sizeof(int32_t) * c * kept);
  free(raw_fx);
  free(raw_ox);
  free(raw_oa);
  return rc;
}
