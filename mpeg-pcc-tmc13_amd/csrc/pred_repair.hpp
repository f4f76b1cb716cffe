// pred_repair.hpp -- the host-side decisions of the predicting encoder's finish (pred_walk_kernel,
// pred_kernels.hpp), stated once: launch_pred (gpcc_attr_mi355.hip) and the emulator harness
// (tests/emu/pred_repair_emu_harness.cpp) both include this file, so the harness runs the
// library's sequence and not a copy of it.  Plain C++, no device code.
#pragma once

#include <cstdint>
#include <cstdlib>

namespace gpcc {

// Whole-slice passes pay off while they remove wrong decisions by large factors; the walk's cost
// follows the number of decisions that are left.  The switch point cannot change the result
// (both are exact), only the time: GPCC_PRED_REPAIR_AFTER=<passes>.  The default follows the counts of
// profiles/pred_repair_emu_switch.jsonl (40 000 noisy lidar points, QP 10 / QP 4: 15 658 / 29 815 predictors
// left to walk after 8 passes, 10 274 / 17 598 after 16, 4 942 / 6 310 after 32) and the cost of a pass, about
// 4 ns per predictor (1 M points, 3 passes, 12.8 ms): a pass over n predictors costs what
// walking n / 250 of them costs if a walked predictor takes 1 us of the one wavefront, so the 24 passes between
// 8 and 32 pay for themselves many times over; slices that settle within 32 passes never enter the walk.
constexpr int kPredRepairAfterDefault = 32;
// no slice runs more whole-slice passes than this, whatever the switch says
constexpr int kPredMaxPasses = 64;

// the switch from its environment text (null / empty / not a positive number: the default)
inline int
pred_repair_after_from_text(const char* s)
{
  if (!s || !*s)
    return kPredRepairAfterDefault;
  char* end = nullptr;
  const long v = strtol(s, &end, 10);
  if (end == s || *end || v < 1)
    return kPredRepairAfterDefault;
  return v > kPredMaxPasses ? kPredMaxPasses : (int)v;
}

// after `passes_done` passes that have not settled: go on with passes, or finish with the walk?
inline bool
pred_repair_due(int passes_done, int after)
{
  return passes_done >= after || passes_done >= kPredMaxPasses;
}

// the pass whose values are compared as a list (the walk's input) instead of as one flag
inline bool
pred_repair_pass_lists(int pass, int after)
{
  return pred_repair_due(pass + 1, after);
}

// What the walk reports (PredWalk::out): it has to have reached the end of the slice, having
// walked at least the first difference and no more than the slice.  Anything else is a defect of
// the library, reported instead of looped on.
inline bool
pred_repair_walk_complete(const int32_t out[4], int n, int differences)
{
  return out[3] == 1 && out[0] >= (differences > 0 ? 1 : 0) && out[0] <= n && out[1] <= out[0] && out[2] <= out[0];
}

}  // namespace gpcc
