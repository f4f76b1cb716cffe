// tests/golden/quantize_harness.cpp -- TEST INFRASTRUCTURE: the reference's quantizePositions,
// quantizePositionsUniq and samplePositionsUniq (pointset_processing.h) behind a C interface for
// make_quantize_golden.py, and the walk over the returned map that getPartition (encoder.cpp:1611-1659, which cannot
// be compiled on its own) does.  Compiled in a temporary directory together with the reference's
// pointset_processing.cpp; it runs only where the reference tree exists.
#include <stdint.h>

#include <chrono>

#include "PCCMath.h"
#include "PCCPointSet.h"
#include "pointset_processing.h"

using namespace pcc;

// mode 0 quantizePositions, 1 quantizePositionsUniq, 2 samplePositionsUniq.  src [n][3]; dst_xyz [n][3],
// idx_to_src [n], dup_next [n] out (modes 1, 2); part [n] out: the source indices getPartition visits for the list
// of every destination index in order.  *ns: the nanoseconds of the reference's call alone.  Returns the number of
// destination points.
extern "C" int32_t
quantize_ref(
  int32_t mode, float scale, float sample_scale, const int32_t* offset, const int32_t* clamp_min,
  const int32_t* clamp_max, const int32_t* src, int32_t n, int32_t* dst_xyz, int32_t* idx_to_src, int32_t* dup_next,
  int32_t* part, int64_t* ns)
{
  PCCPointSet3 cloud;
  cloud.resize(n);
  for (int i = 0; i < n; i++)
    cloud[i] = Vec3<int32_t>{src[3 * i], src[3 * i + 1], src[3 * i + 2]};
  const Vec3<int> off{offset[0], offset[1], offset[2]};
  const Box3<int> clamp{
    Vec3<int>{clamp_min[0], clamp_min[1], clamp_min[2]}, Vec3<int>{clamp_max[0], clamp_max[1], clamp_max[2]}};

  if (mode == 0) {
    PCCPointSet3 dst;
    const auto t0 = std::chrono::steady_clock::now();
    quantizePositions(scale, off, clamp, cloud, &dst);
    const auto t1 = std::chrono::steady_clock::now();
    *ns = std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
    for (int i = 0; i < n; i++)
      for (int k = 0; k < 3; k++)
        dst_xyz[3 * i + k] = dst[i][k];
    return n;
  }

  const auto t0 = std::chrono::steady_clock::now();
  SrcMappedPointSet map =
    mode == 1 ? quantizePositionsUniq(scale, off, clamp, cloud) : samplePositionsUniq(sample_scale, scale, off, cloud);
  const auto t1 = std::chrono::steady_clock::now();
  *ns = std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();

  const int32_t num_dst = (int32_t)map.cloud.getPointCount();
  for (int i = 0; i < num_dst; i++) {
    idx_to_src[i] = map.idxToSrcIdx[i];
    for (int k = 0; k < 3; k++)
      dst_xyz[3 * i + k] = map.cloud[i][k];
  }
  for (int i = 0; i < n; i++)
    dup_next[i] = map.srcIdxDupList[i];

  // getPartition's loop: each linked list until an element points to itself
  int32_t at = 0;
  for (int idx = 0; idx < num_dst; idx++) {
    int prev_idx, src_idx = map.idxToSrcIdx[idx];
    do {
      part[at++] = src_idx;
      prev_idx = src_idx;
      src_idx = map.srcIdxDupList[src_idx];
    } while (src_idx != prev_idx);
  }
  return num_dst;
}
