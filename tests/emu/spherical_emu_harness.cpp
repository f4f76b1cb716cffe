// tests/emu/spherical_emu_harness.cpp -- TEST INFRASTRUCTURE: rpl_bbox_init_kernel, rpl_convert_kernel and
// rpl_scale_kernel (spherical.hpp) under the CPU wavefront emulator, launched as dev_to_spherical
// (gpcc_attr_mi355.hip) launches them: the same tile tables, the same rpl_launch.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip/hip_runtime.h"

#include "spherical.hpp"

using namespace gpcc;

// xyz, pos_out [n][3] (pos_out may be xyz: the in-place form); bbox [num_slices][6]; *error: the sticky word.
// misalign: the device arrays start this many int32 behind a 16-byte boundary (0: the wide loads are taken).
extern "C" int
spherical_emu(
  const gpcc_spherical_params* sp, int32_t num_slices, const int64_t* offsets, const int32_t* xyz, int32_t* pos_out,
  int32_t* bbox, int32_t* error, int32_t misalign)
{
  if (!sp || num_slices < 1 || sp->num_lasers < 1 || sp->num_lasers > GPCC_MAX_LASERS || misalign < 0 || misalign > 3)
    return -1;
  const int64_t n = offsets[num_slices];
  std::vector<int32_t> meta(2 * ((size_t)num_slices + 1));
  int32_t* h_pt = meta.data();
  int32_t* h_tile = meta.data() + num_slices + 1;
  h_tile[0] = 0;
  for (int s = 0; s <= num_slices; s++)
    h_pt[s] = (int32_t)offsets[s];
  for (int s = 0; s < num_slices; s++)
    h_tile[s + 1] = h_tile[s] + rpl_tiles(offsets[s + 1] - offsets[s]);

  // guard words behind the arrays: a store past the end shows
  const size_t bytes = ((sizeof(int32_t) * (3 * n + 4 + 16)) + 255) & ~size_t(255);
  int32_t* raw_in = (int32_t*)aligned_alloc(256, bytes);
  int32_t* raw_out = (int32_t*)aligned_alloc(256, bytes);
  memset(raw_in, 0xCD, bytes);
  memset(raw_out, 0xCD, bytes);
  int32_t* d_in = raw_in + misalign;
  const bool in_place = pos_out == xyz;
  int32_t* d_out = in_place ? d_in : raw_out + misalign;
  memcpy(d_in, xyz, sizeof(int32_t) * 3 * n);

  RplArgs a{};
  a.src = d_in;
  a.dst = d_out;
  a.bbox = bbox;
  a.pt_off = h_pt;
  a.tile_off = h_tile;
  a.error = error;
  a.num_slices = num_slices;
  a.num_tiles = h_tile[num_slices];
  a.num_lasers = sp->num_lasers;
  a.min_pos_mode = sp->min_pos_mode;
  for (int k = 0; k < 3; k++) {
    a.origin[k] = sp->laser_origin[k];
    a.scale[k] = sp->attr_coord_scale[k];
    a.min_pos[k] = sp->min_pos[k];
  }
  for (int i = 0; i < sp->num_lasers; i++)
    a.theta[i] = sp->laser_theta[i];
  rpl_launch(nullptr, a, sp->convert != 0, [](const char*) { return 0; });

  int rc = 0;
  for (int i = 0; i < 16; i++)
    if (d_out[3 * n + i] != (int32_t)0xCDCDCDCD || d_in[3 * n + i] != (int32_t)0xCDCDCDCD)
      rc = -2;
  for (int i = 0; i < misalign; i++)
    if (raw_out[i] != (int32_t)0xCDCDCDCD || raw_in[i] != (int32_t)0xCDCDCDCD)
      rc = -2;
  memcpy(pos_out, d_out, sizeof(int32_t) * 3 * n);
  free(raw_in);
  free(raw_out);
  return rc;
}

// the two primitives on their own (host side of the GPCC_HD functions)
extern "C" int
spherical_emu_iatan2(int y, int x)
{
  static RsqrtLut rs;
  static AsinLut as;
  static bool ready = false;
  if (!ready) {
    const uint16_t r3[96] = {GPCC_RSQRT_R3};
    const uint32_t rc[96] = {GPCC_RSQRT_RC};
    const uint32_t asin_lut[kAsinLutSize] = {GPCC_ASIN_LUT};
    for (int i = 0; i < 96; i++) {
      rs.r3[i] = r3[i];
      rs.rc[i] = rc[i];
    }
    for (int i = 0; i < kAsinLutSize; i++)
      as.v[i] = asin_lut[i];
    ready = true;
  }
  return iatan2(y, x, rs, as);
}

extern "C" int
spherical_emu_find_laser(int32_t z, uint64_t rinv, const int32_t* theta, int num)
{
  return find_laser(z, rinv, theta, num);
}
