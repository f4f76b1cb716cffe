// coordinate_conversion_mi355.cpp -- drop-in replacement for the reference's
//   pcc::convertXyzToRpl   (tmc3/coordinate_conversion.cpp:44-69,   declared coordinate_conversion.h)
//   pcc::offsetAndScale    (tmc3/coordinate_conversion.cpp:109-118)
// the two calls that move a slice's positions into the pseudo-spherical domain in front of the
// attribute coders (encoder.cpp:1181-1194, decoder.cpp:871-920; aps.spherical_coord_flag).
//
// Both are free functions, so the link seam is made like seam 1: the integrator compiles
// tmc3/coordinate_conversion.cpp with
//   -DconvertXyzToRpl=convertXyzToRplCpu -DoffsetAndScale=offsetAndScaleCpu
// (offsetAndScaleShift and normalisedAxesWeights are other tokens and keep their names) and adds this
// translation unit, which defines the two original names with the original signatures over
// gpcc_attr_to_spherical.  Whenever the entry declines -- no GPU, more than GPCC_MAX_LASERS lasers, a point
// outside the entry's domain -- the renamed reference function runs instead; the caller's arrays are
// untouched until the entry has succeeded.
//
// Built against the reference's headers; contains no reference code.
#include <cstdio>
#include <cstring>
#include <vector>

#include "coordinate_conversion.h"

#include "shim_common.hpp"

namespace pcc {
// the renamed reference bodies
Box3<int> convertXyzToRplCpu(
  Vec3<int> laserOrigin, const int* laserThetaList, int numTheta, const Vec3<int>* begin, const Vec3<int>* end,
  Vec3<int>* dst);
void offsetAndScaleCpu(const Vec3<int>& minPos, const Vec3<int>& axisWeight, Vec3<int>* begin, Vec3<int>* end);
}  // namespace pcc

namespace gpcc_shim {
// what this TU did (gpcc_shim_spherical_counters)
long long g_sph_device_calls = 0, g_sph_cpu_calls = 0;

static_assert(sizeof(pcc::Vec3<int>) == 3 * sizeof(int32_t), "Vec3<int> is three ints");

inline void
declined(int rc, const char* what)
{
  if (rc != GPCC_ERR_UNSUPPORTED)
    std::fprintf(stderr, "gpcc: %s; %s falls back to the CPU\n", gpcc_last_error(), what);
}
}  // namespace gpcc_shim

namespace pcc {

Box3<int>
convertXyzToRpl(
  Vec3<int> laserOrigin, const int* laserThetaList, int numTheta, const Vec3<int>* begin, const Vec3<int>* end,
  Vec3<int>* dst)
{
  const long long n = end - begin;
  gpcc_ctx* ctx = gpcc_shim::process_context("the spherical coordinate conversion");
  if (ctx && n > 0 && n <= GPCC_MAX_POINTS && numTheta >= 1 && numTheta <= GPCC_MAX_LASERS) {
    // offsetAndScale as the identity: minimum zero, scale 1.0 in its 8-bit fixed point
    gpcc_spherical_params sp;
    std::memset(&sp, 0, sizeof(sp));
    for (int k = 0; k < 3; k++) {
      sp.laser_origin[k] = laserOrigin[k];
      sp.attr_coord_scale[k] = 256;
    }
    sp.num_lasers = numTheta;
    for (int i = 0; i < numTheta; i++)
      sp.laser_theta[i] = laserThetaList[i];
    sp.min_pos_mode = 1;
    sp.convert = 1;
    int32_t box[6];
    const int rc = gpcc_attr_to_spherical(
      ctx, &sp, reinterpret_cast<const int32_t*>(begin), int32_t(n), reinterpret_cast<int32_t*>(dst), box);
    if (rc == GPCC_OK) {
      gpcc_shim::g_sph_device_calls++;
      return Box3<int>(Vec3<int>{box[0], box[1], box[2]}, Vec3<int>{box[3], box[4], box[5]});
    }
    gpcc_shim::declined(rc, "convertXyzToRpl");
  }
  gpcc_shim::g_sph_cpu_calls++;
  gpcc_shim::strict_check("convertXyzToRpl");
  return convertXyzToRplCpu(laserOrigin, laserThetaList, numTheta, begin, end, dst);
}

void
offsetAndScale(const Vec3<int>& minPos, const Vec3<int>& axisWeight, Vec3<int>* begin, Vec3<int>* end)
{
  const long long n = end - begin;
  gpcc_ctx* ctx = gpcc_shim::process_context("the spherical coordinate conversion");
  if (ctx && n > 0 && n <= GPCC_MAX_POINTS) {
    gpcc_spherical_params sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.num_lasers = 1;  // (not read: the positions are spherical already)
    for (int k = 0; k < 3; k++) {
      sp.attr_coord_scale[k] = axisWeight[k];
      sp.min_pos[k] = minPos[k];
    }
    sp.min_pos_mode = 1;
    sp.convert = 0;
    int32_t* p = reinterpret_cast<int32_t*>(begin);
    const int rc = gpcc_attr_to_spherical(ctx, &sp, p, int32_t(n), p, nullptr);
    if (rc == GPCC_OK) {
      gpcc_shim::g_sph_device_calls++;
      return;
    }
    gpcc_shim::declined(rc, "offsetAndScale");
  }
  gpcc_shim::g_sph_cpu_calls++;
  gpcc_shim::strict_check("offsetAndScale");
  offsetAndScaleCpu(minPos, axisWeight, begin, end);
}

}  // namespace pcc

// {calls that ran on the device, calls handed to the reference's CPU bodies}
extern "C" void
gpcc_shim_spherical_counters(long long out[2])
{
  out[0] = gpcc_shim::g_sph_device_calls;
  out[1] = gpcc_shim::g_sph_cpu_calls;
}
