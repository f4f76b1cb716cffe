// tests/emu/rc_batch_emu_harness.cpp -- TEST INFRASTRUCTURE: gpcc_dev_recolour_attrs under the CPU wavefront
// emulator.  It runs rcb_check and rcb_run of mpeg-pcc-tmc13_amd/csrc/recolour_batch.hpp -- the text the library
// entry runs -- with a Host made of malloc: EVERY block the driver takes (the slice table, the forests' index
// arrays, nodes, level arrays and subtree lists, the lists, the forward values) and every input and output array
// stands between guard bytes that are compared after the run, so the capacities derived for R roots are checked
// here.
#include <string>
#include <vector>

#include "hip/hip_runtime.h"

#include "recolour_batch.hpp"

using namespace gpcc;

namespace {
constexpr size_t kGuard = 256;
constexpr unsigned char kGuardByte = 0xA7;

// `bytes` between two bands of guard bytes, tight against both
struct Guarded {
  unsigned char* base = nullptr;
  size_t bytes = 0, lead = 0;
  void* data() const { return base + lead; }
  void make(size_t n, const void* init)
  {
    bytes = n;
    lead = kGuard;
    base = (unsigned char*)malloc(lead + bytes + kGuard);
    memset(base, kGuardByte, lead + bytes + kGuard);
    if (init)
      memcpy(data(), init, bytes);
    else
      memset(data(), 0xCD, bytes);  // the pool of the library is not cleared either
  }
  bool intact() const
  {
    for (size_t i = 0; i < lead; i++)
      if (base[i] != kGuardByte)
        return false;
    for (size_t i = 0; i < kGuard; i++)
      if (base[lead + bytes + i] != kGuardByte)
        return false;
    return true;
  }
};

struct NoSpan {
  ~NoSpan() {}
};

struct EmuHost {
  std::vector<Guarded> blocks;
  std::vector<int32_t> h_boxes;
  int32_t h_counters[8] = {};
  std::string why;
  ~EmuHost()
  {
    for (Guarded& g : blocks)
      free(g.base);
  }
  hipError_t take(size_t bytes, void** out, bool)
  {
    Guarded g;
    g.make(bytes, nullptr);
    blocks.push_back(g);
    *out = g.data();
    return hipSuccess;
  }
  void end_work() {}  // (kept until the end: their guard bytes are compared with the others)
  hipError_t upload(void* dst, const void* src, size_t bytes)
  {
    memcpy(dst, src, bytes);
    return hipSuccess;
  }
  hipError_t fork(hipStream_t* second)
  {
    *second = nullptr;
    return hipSuccess;
  }
  hipError_t join() { return hipSuccess; }
  int32_t* counters() { return h_counters; }
  int32_t* boxes(size_t ints)
  {
    h_boxes.assign(ints, 0);
    return h_boxes.data();
  }
  int fail(int code, const char* msg)
  {
    why = msg;
    return code;
  }
  NoSpan span(const char*) { return NoSpan(); }
  bool intact() const
  {
    for (const Guarded& g : blocks)
      if (!g.intact())
        return false;
    return true;
  }
};
}  // namespace

// The arguments of gpcc_dev_recolour_attrs with host arrays in the place of the device's; the kernels see guarded
// copies.  -> the library's return code (0, GPCC_ERR_*), or -104 where a guard band or an input array was written
// (the outputs are still copied back).
extern "C" int
rc_batch_emu_recolour(
  const gpcc_recolour_params* p, int32_t num_slices, const int64_t* src_off, const int32_t* src_xyz, const int64_t* tgt_off,
  const int32_t* tgt_xyz, const gpcc_dev_recolour_attr* attrs, int32_t num_attrs, float scale, const int32_t* offsets)
{
  RcBatchIn in = {num_slices, src_off, tgt_off, src_xyz, tgt_xyz, attrs, num_attrs, scale, offsets};
  std::string why;
  int rc = rcb_check(p, in, &why);
  if (rc != GPCC_OK)
    return rc;
  const size_t ns = (size_t)src_off[num_slices], nt = (size_t)tgt_off[num_slices];
  Guarded g_sx, g_tx, g_src[GPCC_RC_MAX_ATTRS], g_out[GPCC_RC_MAX_ATTRS];
  gpcc_dev_recolour_attr table[GPCC_RC_MAX_ATTRS];
  g_sx.make(sizeof(int32_t) * 3 * ns, src_xyz);
  g_tx.make(sizeof(int32_t) * 3 * nt, tgt_xyz);
  in.d_src_xyz = (const int32_t*)g_sx.data();
  in.d_tgt_xyz = (const int32_t*)g_tx.data();
  for (int a = 0; a < num_attrs; a++) {
    g_src[a].make(sizeof(int32_t) * attrs[a].c * ns, attrs[a].d_src);
    g_out[a].make(sizeof(int32_t) * attrs[a].c * nt, attrs[a].d_tgt);
    table[a] = attrs[a];
    table[a].d_src = g_src[a].data();
    table[a].d_tgt = g_out[a].data();
  }
  in.attrs = table;
  {
    EmuHost host;
    rc = rcb_run(host, *p, in, nullptr);
    if (!host.intact())
      rc = -104;
  }
  if (!g_sx.intact() || !g_tx.intact() || memcmp(g_sx.data(), src_xyz, g_sx.bytes) != 0
      || memcmp(g_tx.data(), tgt_xyz, g_tx.bytes) != 0)
    rc = -104;
  for (int a = 0; a < num_attrs; a++) {
    memcpy(attrs[a].d_tgt, g_out[a].data(), g_out[a].bytes);
    if (!g_src[a].intact() || !g_out[a].intact() || memcmp(g_src[a].data(), attrs[a].d_src, g_src[a].bytes) != 0)
      rc = -104;
    free(g_src[a].base);
    free(g_out[a].base);
  }
  free(g_sx.base);
  free(g_tx.base);
  return rc;
}
