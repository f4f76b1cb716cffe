// tests/emu/quantize_emu_harness.cpp -- TEST INFRASTRUCTURE: the kernels of quantize_positions.hpp (with the sort
// passes of morton_sort.hpp and the scan of recolour_kdtree.hpp) under the CPU wavefront emulator, launched as
// host_quantize_positions / host_src_partition (gpcc_attr_mi355.hip) launch them: the same carving, the same launch
// functions with the host's look at the count between them.  Every work and output array is an allocation of its
// own between guard words.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip/hip_runtime.h"

#include "quantize_positions.hpp"

using namespace gpcc;

namespace {

constexpr size_t kGuardWords = 16;
constexpr int32_t kGuard = (int32_t)0xCDCDCDCD;

struct Guarded {
  std::vector<char*> raw;
  std::vector<size_t> bytes;
  char* take(size_t n)
  {
    const size_t padded = (n + 3) & ~size_t(3);
    char* p = (char*)malloc(padded + 2 * kGuardWords * 4);
    memset(p, 0xCD, padded + 2 * kGuardWords * 4);
    raw.push_back(p);
    bytes.push_back(n);
    return p + kGuardWords * 4;
  }
  // every byte in front of and behind every array still holds the fill
  bool intact() const
  {
    for (size_t i = 0; i < raw.size(); i++) {
      const size_t total = ((bytes[i] + 3) & ~size_t(3)) + 2 * kGuardWords * 4;
      for (size_t b = 0; b < kGuardWords * 4; b++)
        if ((unsigned char)raw[i][b] != 0xCD)
          return false;
      for (size_t b = kGuardWords * 4 + bytes[i]; b < total; b++)
        if ((unsigned char)raw[i][b] != 0xCD)
          return false;
    }
    return true;
  }
  ~Guarded()
  {
    for (char* p : raw)
      free(p);
  }
};

}  // namespace

// params: mode, then offset[3], clamp_min[3], clamp_max[3]; scales: scale, sample_scale.  src [n][3];
// dst_xyz [n][3], idx_to_src [n], dup_next [n] out; plan [kQzPlanWords] out: the device's plan; *error: the sticky
// word.  max1 / max2 < 0: the host's own bound (qz_pass_bounds).  Returns the number of destination points, -2
// when a guard word has changed, -3 when an array behind the kept entries was written.
extern "C" int
quantize_emu(
  const int32_t* params, const float* scales, const int32_t* src, int32_t n, int32_t* dst_xyz, int32_t* idx_to_src,
  int32_t* dup_next, int32_t* plan, int32_t* error, int32_t max1, int32_t max2)
{
  if (n < 1)
    return -1;
  QzArgs a{};
  QzWork w{};
  a.n = n;
  a.mode = params[0];
  a.scale = scales[0];
  a.diff_scale = a.mode == 2 ? scales[1] / scales[0] : 0;
  for (int k = 0; k < 3; k++) {
    a.offset[k] = params[1 + k];
    a.clamp_min[k] = params[4 + k];
    a.clamp_max[k] = params[7 + k];
  }
  int b1 = 0, b2 = 0;
  qz_pass_bounds(a.mode, a.clamp_min, a.clamp_max, &b1, &b2);
  if (max1 >= 0)
    b1 = max1;
  if (max2 >= 0)
    b2 = max2;
  Guarded g;
  qz_carve([&](size_t bytes) { return g.take(bytes); }, n, a.mode, a, w);
  a.error = error;
  a.src = src;
  auto span = [](const char*) { return 0; };
  qz_count_launch(nullptr, a, w, b1, b2, span);
  memcpy(plan, a.plan, sizeof(int32_t) * kQzPlanWords);
  int kept = n;
  if (a.mode == 0) {
    memcpy(dst_xyz, a.key, sizeof(int32_t) * 3 * n);
  } else {
    kept = w.counts[w.num_tiles];
    if (kept < 1 || kept > n)
      return -4;
    qz_emit_launch(nullptr, a, w, span);
    memcpy(dst_xyz, w.dst, sizeof(int32_t) * 3 * kept);
    memcpy(idx_to_src, w.idx_to_src, sizeof(int32_t) * kept);
    memcpy(dup_next, w.next, sizeof(int32_t) * n);
    for (size_t i = kept; i < (size_t)n; i++)
      if (w.idx_to_src[i] != kGuard || w.dst[3 * i] != kGuard || w.dst[3 * i + 2] != kGuard)
        return -3;
  }
  return g.intact() ? kept : -2;
}

// One call of the partition's launches.  src_attrs may be null (positions only).  capacity: the points the output
// arrays hold; out_offsets [num_slices + 1] is filled in every case.  Returns 0, 1 when the capacity is too small
// (nothing written), -2 / -3 as above.
extern "C" int
partition_emu(
  const int32_t* src_xyz, const int32_t* src_attrs, int32_t n_src, int32_t c, const int32_t* idx_to_src, int32_t n_dst,
  const int32_t* dup_next, const int32_t* indexes, const int32_t* index_offsets, int32_t num_slices, int32_t* out_xyz,
  int32_t* out_attrs, int64_t capacity, int64_t* out_offsets, int32_t* error)
{
  const int32_t listed = index_offsets[num_slices];
  if (listed < 1)
    return -1;
  Guarded g;
  PartArgs a{};
  a.counts = (int32_t*)g.take(sizeof(int32_t) * ((size_t)listed + 1));
  long long* sums = (long long*)g.take(sizeof(long long) * part_sum_entries(listed));
  a.total = (unsigned long long*)g.take(sizeof(unsigned long long));
  a.offsets = (int32_t*)g.take(sizeof(int32_t) * ((size_t)num_slices + 1));
  a.out_xyz = (int32_t*)g.take(sizeof(int32_t) * 3 * (size_t)capacity);
  a.out_attrs = src_attrs ? (int32_t*)g.take(sizeof(int32_t) * c * (size_t)capacity) : nullptr;
  a.src_xyz = src_xyz;
  a.src_attrs = src_attrs;
  a.idx_to_src = idx_to_src;
  a.next = dup_next;
  a.indexes = indexes;
  a.index_offsets = index_offsets;
  a.error = error;
  a.n_src = n_src;
  a.n_dst = n_dst;
  a.c = c;
  a.listed = listed;
  a.num_slices = num_slices;
  auto span = [](const char*) { return 0; };
  part_count_launch(nullptr, a, sums, span);
  for (int s = 0; s <= num_slices; s++)
    out_offsets[s] = a.offsets[s];
  int rc = 0;
  if (*error)
    return g.intact() ? 0 : -2;
  const long long total = (long long)*a.total;
  if (total != a.offsets[num_slices])
    return -4;
  if (total > capacity) {
    rc = 1;
  } else {
    part_emit_launch(nullptr, a, span);
    memcpy(out_xyz, a.out_xyz, sizeof(int32_t) * 3 * total);
    if (src_attrs)
      memcpy(out_attrs, a.out_attrs, sizeof(int32_t) * c * total);
  }
  const size_t kept = rc ? 0 : (size_t)total;
  for (size_t i = 3 * kept; i < 3 * (size_t)capacity; i++)
    if (a.out_xyz[i] != kGuard)
      return -3;
  if (src_attrs)
    for (size_t i = c * kept; i < (size_t)c * capacity; i++)
      if (a.out_attrs[i] != kGuard)
        return -3;
  return g.intact() ? rc : -2;
}
