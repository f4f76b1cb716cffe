// tests/emu/symbol_stream_emu_harness.cpp -- TEST INFRASTRUCTURE: the kernels of symbol_stream.hpp (with the
// binarisation of residual_bins.hpp) under the CPU wavefront emulator, launched as dev_residual_bins and
// dev_zero_run_unpack (gpcc_attr_mi355.hip) launch them: the same tables, the same launch functions with the host's
// look at the offsets between counting and emitting; and the scan all passes share, on its own.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip/hip_runtime.h"

#include "symbol_stream.hpp"

using namespace gpcc;

namespace {

constexpr int kGuardWords = 16;  // in front of and behind every output
constexpr unsigned char kGuardByte = 0xCD;

// an output of `bytes` bytes between two bands of guard bytes
struct Guarded {
  unsigned char* raw;
  size_t bytes;
  explicit Guarded(size_t b) : bytes(b)
  {
    raw = (unsigned char*)aligned_alloc(256, (b + 2 * 4 * kGuardWords + 255) & ~size_t(255));
    memset(raw, kGuardByte, b + 2 * 4 * kGuardWords);
  }
  ~Guarded() { free(raw); }
  unsigned char* data() { return raw + 4 * kGuardWords; }
  // the bands, and of the output itself everything from `used` on
  bool intact(size_t used) const
  {
    for (size_t i = 0; i < 4 * kGuardWords; i++)
      if (raw[i] != kGuardByte || raw[4 * kGuardWords + bytes + i] != kGuardByte)
        return false;
    for (size_t i = used; i < bytes; i++)
      if (raw[4 * kGuardWords + i] != kGuardByte)
        return false;
    return true;
  }
};

}  // namespace

// coeffs: the batch, slice s at coeffs + c * offsets[s] in the layout `planar` says; bins [bins_capacity] out;
// bin_offsets [num_slices + 1], num_symbols / trailing_run [num_slices] out; runs [n] / values [n][c] out, slice s at
// its points' offset (both or neither).  Returns 1 when the capacity is too small (bins untouched), -2 when a guard
// byte around an output, or a symbol slot behind a slice's last symbol, has changed.
extern "C" int
symbol_stream_emu_bins(
  int32_t num_slices, const int64_t* offsets, const int32_t* coeffs, int32_t c, int32_t planar, uint8_t* bins,
  int64_t bins_capacity, int64_t* bin_offsets, int32_t* runs, int32_t* values, int32_t* num_symbols,
  int32_t* trailing_run)
{
  if (num_slices < 1 || (c != 1 && c != 3) || bins_capacity < 0 || (runs == nullptr) != (values == nullptr))
    return -1;
  const size_t S = (size_t)num_slices, N = (size_t)offsets[num_slices];
  std::vector<int32_t> meta(3 * (S + 1), 0);
  int32_t* h_pt = meta.data();
  int32_t* h_tile = meta.data() + 2 * (S + 1);
  for (size_t s = 0; s <= S; s++)
    h_pt[s] = (int32_t)offsets[s];
  for (size_t s = 0; s < S; s++)
    h_tile[s + 1] = h_tile[s] + rpl_tiles(offsets[s + 1] - offsets[s]);
  const size_t nt = (size_t)h_tile[S];

  Guarded g_bins((size_t)bins_capacity), g_runs(4 * N), g_vals(4 * N * c), g_off(8 * (S + 1)), g_sym(4 * S), g_trail(4 * S);
  Guarded g_mask(8 * nt * kSymWords), g_cnt(4 * nt), g_last(4 * nt), g_tbins(4 * nt), g_base(8 * (nt + 1)),
    g_prev(8 * (nt + 1)), g_bbase(8 * (nt + 1));
  std::vector<long long> sums(sym_scan_blocks(nt)), maxs(sym_scan_blocks(nt));
  SymArgs a{};
  a.coeffs = coeffs;
  a.pt_off = h_pt;
  a.tile_off = h_tile;
  a.mask = (unsigned long long*)g_mask.data();
  a.tile_cnt = (int32_t*)g_cnt.data();
  a.tile_last = (int32_t*)g_last.data();
  a.sym_base = (long long*)g_base.data();
  a.prev = (long long*)g_prev.data();
  a.tile_bins = (int32_t*)g_tbins.data();
  a.bin_base = (long long*)g_bbase.data();
  a.scan_sums = sums.data();
  a.scan_maxs = maxs.data();
  a.bin_offsets = (long long*)g_off.data();
  a.num_symbols = (int32_t*)g_sym.data();
  a.trailing_run = (int32_t*)g_trail.data();
  a.runs = runs ? (int32_t*)g_runs.data() : nullptr;
  a.values = runs ? (int32_t*)g_vals.data() : nullptr;
  a.bins = g_bins.data();
  a.c = c;
  a.planar = planar != 0;
  a.num_slices = num_slices;
  a.num_tiles = (int32_t)nt;
  auto span = [](const char*) { return 0; };
  sym_count_launch(nullptr, a, span);
  memcpy(bin_offsets, a.bin_offsets, 8 * (S + 1));
  memcpy(num_symbols, a.num_symbols, 4 * S);
  memcpy(trailing_run, a.trailing_run, 4 * S);
  int rc = 0;
  if (bin_offsets[num_slices] > bins_capacity)
    rc = 1;
  else if (bin_offsets[num_slices] > 0)
    sym_emit_launch(nullptr, a, span);

  bool ok = g_bins.intact(rc ? 0 : (size_t)bin_offsets[num_slices]) && g_off.intact(g_off.bytes)
    && g_sym.intact(g_sym.bytes) && g_trail.intact(g_trail.bytes) && g_mask.intact(g_mask.bytes)
    && g_cnt.intact(g_cnt.bytes) && g_last.intact(g_last.bytes) && g_tbins.intact(g_tbins.bytes)
    && g_base.intact(g_base.bytes) && g_prev.intact(g_prev.bytes) && g_bbase.intact(g_bbase.bytes);
  if (runs) {
    ok = ok && g_runs.intact(g_runs.bytes) && g_vals.intact(g_vals.bytes);
    // (behind a slice's symbols nothing is written)
    const int32_t* r = (const int32_t*)g_runs.data();
    const int32_t* v = (const int32_t*)g_vals.data();
    for (size_t s = 0; s < S; s++) {
      for (int64_t k = offsets[s] + num_symbols[s]; k < offsets[s + 1]; k++) {
        ok = ok && r[k] == (int32_t)0xCDCDCDCD;
        for (int j = 0; j < c; j++)
          ok = ok && v[c * k + j] == (int32_t)0xCDCDCDCD;
      }
    }
    memcpy(runs, r, 4 * N);
    memcpy(values, v, 4 * N * c);
  }
  if (!rc)
    memcpy(bins, g_bins.data(), (size_t)bin_offsets[num_slices]);
  return ok ? rc : -2;
}

// runs / values: slice s owns the symbols [sym_offsets[s], sym_offsets[s + 1]); coeffs_out [c * n]: the batch;
// *error: the sticky word.  Returns -2 when a guard byte around the coefficients has changed.
extern "C" int
symbol_stream_emu_unpack(
  int32_t num_slices, const int64_t* offsets, const int64_t* sym_offsets, const int32_t* runs, const int32_t* values,
  int32_t* coeffs_out, int32_t c, int32_t planar, int32_t* error)
{
  if (num_slices < 1 || c < 1 || c > 3)
    return -1;
  const size_t S = (size_t)num_slices, N = (size_t)offsets[num_slices];
  std::vector<int32_t> meta(3 * (S + 1), 0);
  int32_t* h_pt = meta.data();
  int32_t* h_sym = meta.data() + (S + 1);
  int32_t* h_tile = meta.data() + 2 * (S + 1);
  for (size_t s = 0; s <= S; s++) {
    h_pt[s] = (int32_t)offsets[s];
    h_sym[s] = (int32_t)sym_offsets[s];
  }
  for (size_t s = 0; s < S; s++)
    h_tile[s + 1] = h_tile[s] + rpl_tiles(sym_offsets[s + 1] - sym_offsets[s]);
  const size_t nt = (size_t)h_tile[S];

  Guarded g_co(4 * N * c), g_sum(8 * (nt + 1)), g_base(8 * (nt + 1));
  std::vector<long long> sums(sym_scan_blocks(nt));
  SymUnpackArgs a{};
  a.runs = runs;
  a.values = values;
  a.pt_off = h_pt;
  a.sym_off = h_sym;
  a.tile_off = h_tile;
  a.tile_sum = (long long*)g_sum.data();
  a.tile_base = (long long*)g_base.data();
  a.scan_sums = sums.data();
  a.coeffs = (int32_t*)g_co.data();
  a.error = error;
  a.c = c;
  a.planar = planar != 0;
  a.num_slices = num_slices;
  a.num_tiles = (int32_t)nt;
  auto span = [](const char*) { return 0; };
  sym_unpack_launch(nullptr, a, (int64_t)c * (int64_t)N, span);
  const bool ok = g_co.intact(g_co.bytes) && g_sum.intact(g_sum.bytes) && g_base.intact(g_base.bytes);
  memcpy(coeffs_out, g_co.data(), 4 * N * c);
  return ok ? 0 : -2;
}

// the scan on its own: a [n] (64-bit entries when wide), b [n] or null; out_sum / out_max [n + 1]
extern "C" int
symbol_stream_emu_scan(int64_t n, const void* a, int32_t wide, const int32_t* b, long long* out_sum, long long* out_max)
{
  if (n < 1)
    return -1;
  const size_t N = (size_t)n;
  Guarded g_sum(8 * (N + 1)), g_max(8 * (N + 1)), g_s(8 * sym_scan_blocks(N)), g_m(8 * sym_scan_blocks(N));
  long long* sums = (long long*)g_s.data();
  long long* maxs = (long long*)g_m.data();
  long long* os = (long long*)g_sum.data();
  long long* om = b ? (long long*)g_max.data() : nullptr;
  if (wide)
    sym_scan<long long>(nullptr, (const long long*)a, b, N, sums, maxs, os, om);
  else
    sym_scan<int32_t>(nullptr, (const int32_t*)a, b, N, sums, maxs, os, om);
  const bool ok = g_sum.intact(g_sum.bytes) && g_max.intact(b ? g_max.bytes : 0) && g_s.intact(g_s.bytes) && g_m.intact(g_m.bytes);
  memcpy(out_sum, os, 8 * (N + 1));
  if (b)
    memcpy(out_max, om, 8 * (N + 1));
  return ok ? 0 : -2;
}
