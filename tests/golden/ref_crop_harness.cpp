// tests/golden/ref_crop_harness.cpp -- TEST INFRASTRUCTURE: the crop of the previous frame to the current slice's
// bounding box, stated with the reference's own PCCPointSet3::computeBoundingBox and Box3::contains behind a C
// interface for make_ref_crop_golden.py: the box of the slice, then every frame point the box contains, appended to
// the output arrays in the frame's order with its attributes.  Compiled in a temporary directory against the
// reference's headers; it runs only where the reference tree exists.
#include <stdint.h>

#include <chrono>

#include "PCCMath.h"
#include "PCCPointSet.h"

using namespace pcc;

// xyz [n][3]: the current slice; frame_xyz [n_frame][3], frame_attrs [n_frame][c], c in 1..3.  bbox [6] out: min,
// max; out_xyz / out_attrs: the kept points.  *ns: the nanoseconds of the box and the walk over the frame (this
// restatement's, not the reference encoder's).  Returns the number of points kept.
extern "C" int32_t
ref_crop_ref(
  const int32_t* xyz, int32_t n, const int32_t* frame_xyz, const int32_t* frame_attrs, int32_t n_frame, int32_t c,
  int32_t* bbox, int32_t* out_xyz, int32_t* out_attrs, int64_t* ns)
{
  PCCPointSet3 slice;
  slice.resize(n);
  for (int i = 0; i < n; i++)
    slice[i] = Vec3<int32_t>{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};

  const auto t0 = std::chrono::steady_clock::now();
  const Box3<int32_t> box = slice.computeBoundingBox();
  int32_t kept = 0;
  for (int32_t i = 0; i < n_frame; i++) {
    const int32_t* q = frame_xyz + 3 * i;
    if (!box.contains(Vec3<int32_t>{q[0], q[1], q[2]}))
      continue;
    for (int k = 0; k < 3; k++)
      out_xyz[3 * kept + k] = q[k];
    for (int k = 0; k < c; k++)
      out_attrs[c * kept + k] = frame_attrs[c * i + k];
    kept++;
  }
  const auto t1 = std::chrono::steady_clock::now();
  *ns = std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();

  for (int k = 0; k < 3; k++) {
    bbox[k] = box.min[k];
    bbox[3 + k] = box.max[k];
  }
  return kept;
}
