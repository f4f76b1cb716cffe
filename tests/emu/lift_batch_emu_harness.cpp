// tests/emu/lift_batch_emu_harness.cpp -- TEST INFRASTRUCTURE: the kernels of lift_batch.hpp under the CPU wavefront
// emulator, driven by the plan and launch functions dev_lift_batch (gpcc_attr_mi355.hip) calls, with the same
// tables: plan.meta "uploaded" as one block, the working arrays beside it.  Guard bytes surround every array the
// kernels read or write.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip/hip_runtime.h"

#include "lift_batch.hpp"

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

}  // namespace

// The arguments of gpcc_dev_lift_forward / _inverse, in host memory.  attrs, coeffs [N][c] and lcp
// [num_slices][GPCC_MAX_LODS] are read and written in place (lcp as the library does it: the encoder's rows of the
// slices with the flag).  *verdict: the check kernel's word; *launches: the launches of the call.
// Returns 0, or -2 when a guard byte has changed, an input has been written, or -- with the verdict set -- any
// output or working array has been touched.
extern "C" int
lift_batch_emu(
  const gpcc_lift_params* lift, int32_t num_slices, const int64_t* offsets, int32_t c, int32_t encoder,
  const int32_t* nc, const int32_t* ni, const int32_t* nw, const int32_t* indexes, const int32_t* xyz,
  int32_t* attrs, int32_t* coeffs, int8_t* lcp, int32_t* verdict, int32_t* launches)
{
  if (num_slices < 1 || c < 1 || c > 3)
    return -1;
  LiftBatchPlan plan;
  lift_batch_plan(plan, lift, num_slices, offsets, c, encoder ? nullptr : lcp);
  const size_t S = (size_t)num_slices, N = (size_t)plan.n;
  RsqrtLut lut;
  {
    const uint16_t r3[96] = {GPCC_RSQRT_R3};
    const uint32_t rc[96] = {GPCC_RSQRT_RC};
    memcpy(lut.r3, r3, sizeof(r3));
    memcpy(lut.rc, rc, sizeof(rc));
  }
  Guarded g_meta(plan.meta.size(), plan.meta.data()), g_nc(4 * N, nc), g_ni(12 * N, ni), g_nw(12 * N, nw),
    g_ix(4 * N, indexes), g_xyz(xyz ? 12 * N : 4, xyz), g_attrs(4 * N * c, attrs), g_coeffs(4 * N * c, coeffs),
    g_a(8 * N * c), g_qw(8 * N), g_uw(8 * N), g_up(8 * N * c), g_sums(16 * GPCC_MAX_LODS * S), g_lut(sizeof(lut), &lut);
  char* d_meta = (char*)g_meta.data();
  LiftBatch b{};
  lift_batch_view(b, plan, d_meta);
  b.nc = (const int32_t*)g_nc.data();
  b.ni = (const int32_t*)g_ni.data();
  b.nw = (const int32_t*)g_nw.data();
  b.indexes = (const int32_t*)g_ix.data();
  b.xyz = xyz ? (const int32_t*)g_xyz.data() : nullptr;
  b.attrs = (int32_t*)g_attrs.data();
  b.coeffs = (int32_t*)g_coeffs.data();
  b.a = (int64_t*)g_a.data();
  b.qw = (unsigned long long*)g_qw.data();
  b.uw = (unsigned long long*)g_uw.data();
  b.up = (unsigned long long*)g_up.data();
  b.lcp_sums = (long long*)g_sums.data();
  b.rsqrt = (const RsqrtLut*)g_lut.data();
  int count = 0;
  auto span = [&](const char*) { return ++count; };
  lift_batch_launch(nullptr, b, plan, d_meta, encoder != 0, span);
  *launches = count;
  *verdict = *b.verdict;

  bool ok = g_nc.unchanged(nc) && g_ni.unchanged(ni) && g_nw.unchanged(nw) && g_ix.unchanged(indexes)
    && (xyz ? g_xyz.unchanged(xyz) : g_xyz.untouched()) && g_lut.unchanged(&lut) && g_meta.bands_intact()
    && g_attrs.bands_intact() && g_coeffs.bands_intact() && g_a.bands_intact() && g_qw.bands_intact()
    && g_uw.bands_intact() && g_up.bands_intact() && g_sums.bands_intact();
  // the tables are inputs: all of the block but the verdict word and the encoder's LCP rows
  ok = ok && memcmp(d_meta + 16, plan.meta.data() + 16, plan.at_lcp - 16) == 0;
  if (!encoder)
    ok = ok && g_coeffs.unchanged(coeffs) && memcmp(d_meta + plan.at_lcp, plan.meta.data() + plan.at_lcp, S * GPCC_MAX_LODS) == 0;
  if (*verdict) {
    ok = ok && g_attrs.unchanged(attrs) && g_coeffs.unchanged(coeffs) && g_a.untouched() && g_qw.untouched()
      && g_uw.untouched() && g_up.untouched() && g_sums.untouched()
      && memcmp(d_meta + plan.at_lcp, plan.meta.data() + plan.at_lcp, S * GPCC_MAX_LODS) == 0;
    return ok ? 0 : -2;
  }
  memcpy(attrs, g_attrs.data(), 4 * N * c);
  memcpy(coeffs, g_coeffs.data(), 4 * N * c);
  if (encoder && plan.any_lcp)
    for (size_t s = 0; s < S; s++)
      if (lift[s].last_component_prediction_enabled_flag)
        memcpy(lcp + s * GPCC_MAX_LODS, d_meta + plan.at_lcp + s * GPCC_MAX_LODS, GPCC_MAX_LODS);
  return ok ? 0 : -2;
}
