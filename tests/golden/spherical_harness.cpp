// tests/golden/spherical_harness.cpp -- TEST INFRASTRUCTURE: the reference's own convertXyzToRpl,
// offsetAndScale and normalisedAxesWeights (tmc3/coordinate_conversion.cpp) behind a C interface, for
// make_spherical_golden.py and test_shim_spherical.py.  Compiled in a temporary directory together with
// the reference's coordinate_conversion.cpp, geometry_octree.cpp, misc.cpp and tables.cpp; it runs only
// where the reference tree exists.
#include <stdint.h>
#include <string.h>

#include <chrono>

#include "coordinate_conversion.h"

using namespace pcc;

// scale [3] = normalisedAxesWeights({0, {rmax, two_pi, max_laser}}, forced_max_log2) (encoder.cpp:208-212)
extern "C" void
spherical_ref_scale(int32_t rmax, int32_t two_pi, int32_t max_laser, int32_t forced_max_log2, int32_t* scale)
{
  Box3<int> box{0, {rmax, two_pi, max_laser}};
  auto w = normalisedAxesWeights(box, forced_max_log2);
  for (int k = 0; k < 3; k++)
    scale[k] = w[k];
}

// One slice as encoder.cpp:1148-1197 treats it.  convert: convertXyzToRpl first; otherwise `xyz` holds
// spherical positions already and only their bounding box is taken (the predictive-geometry branch).
// mode 0: the minimum is the box's; 1: min_pos as given; 2: the smaller of the two per component.
// rpl [n][3]: the unscaled positions; bbox [6]: their min, max; pos [n][3]: offset and scaled.
// Returns the nanoseconds the two reference calls took.
extern "C" int64_t
spherical_ref_slice(
  const int32_t* origin, const int32_t* theta, int32_t num_theta, const int32_t* xyz, int32_t n, int32_t convert,
  int32_t mode, const int32_t* min_pos, const int32_t* scale, int32_t* rpl, int32_t* bbox, int32_t* pos,
  int32_t* min_used)
{
  static_assert(sizeof(Vec3<int>) == 12, "Vec3<int> is three ints");
  const Vec3<int>* src = reinterpret_cast<const Vec3<int>*>(xyz);
  Vec3<int>* dst = reinterpret_cast<Vec3<int>*>(pos);
  Box3<int> box;
  const auto t0 = std::chrono::steady_clock::now();
  if (convert) {
    box = convertXyzToRpl(Vec3<int>{origin[0], origin[1], origin[2]}, theta, num_theta, src, src + n, dst);
  } else {
    memcpy(pos, xyz, sizeof(int32_t) * 3 * n);
    box = Box3<int>(dst, dst + n);
  }
  const auto t1 = std::chrono::steady_clock::now();
  memcpy(rpl, pos, sizeof(int32_t) * 3 * n);
  Vec3<int> mn = box.min;
  for (int k = 0; k < 3; k++) {
    bbox[k] = box.min[k];
    bbox[3 + k] = box.max[k];
    if (mode == 1)
      mn[k] = min_pos[k];
    else if (mode == 2)
      mn[k] = mn[k] < min_pos[k] ? mn[k] : min_pos[k];
    min_used[k] = mn[k];
  }
  const auto t2 = std::chrono::steady_clock::now();
  offsetAndScale(mn, Vec3<int>{scale[0], scale[1], scale[2]}, dst, dst + n);
  const auto t3 = std::chrono::steady_clock::now();
  return std::chrono::duration_cast<std::chrono::nanoseconds>((t1 - t0) + (t3 - t2)).count();
}
