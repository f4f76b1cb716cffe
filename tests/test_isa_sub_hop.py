"""What one productive iteration of the sub-node level kernels' dependency loop is made of
(mpeg-pcc-tmc13_amd/csrc/raht_subnode.hpp), pinned on the gfx950 ISA so that it does not erode:

* the granule poll is issued at the top of an iteration and its `s_waitcnt vmcnt` does not sit in the stage body
  that follows it: a group fed from the wavefront's mailbox computes while the round trip is in flight, and the
  answer is taken in front of the iteration's first store;
* the lossy encoder's RDOQ threshold is a multiplication by the reciprocal of lambda, computed before the loop:
  no double division (v_div_* / v_rcp_f64) between the poll and the idle sleep;
* the per-slot tables (awaited row, prediction weight) are read from LDS where a lane's slot changes;
* the double-precision butterfly stages are branch-free, and the loop region of the two headline kernels stays
  within a few per cent of its instruction count.

Same listing as tests/test_isa_chain_discipline.py (GPCC_ISA_LISTING, else tests/isa/sub_kernels.hip compiled
here) -- no GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa_hop") / "gpcc.s")
    csrc = os.path.join(ROOT, "mpeg-pcc-tmc13_amd", "csrc")
    src = os.path.join(ROOT, "tests", "isa", "sub_kernels.hip")
    pre = os.environ.get("GPCC_ISA_LISTING")
    if pre and os.path.exists(pre) and os.path.getmtime(pre) >= max(
            os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc)):
        out = pre
    else:
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-w",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        "-S", "--cuda-device-only", "-o", out, src], check=True, timeout=900)
    bodies, cur = {}, None
    for ln in open(out):
        m = re.match(r"^(_Z\w+):\s*; @", ln)
        if m:
            cur = m.group(1)
            bodies[cur] = []
        elif cur:
            s = ln.strip()
            if s and not s.startswith((";", ".")) and not s.endswith(":"):
                bodies[cur].append(s)
            if ln.startswith(".Lfunc_end"):
                cur = None
    return bodies


def loop_region(body):
    """instructions from the first granule poll to the idle sleep of the staged loop"""
    polls = [i for i, s in enumerate(body) if s.startswith("buffer_load_dwordx4") and "sc1" in s]
    assert polls, "no granule poll found"
    sleeps = [i for i, s in enumerate(body) if s.startswith("s_sleep") and i > polls[0]]
    assert sleeps
    return body[polls[0]:sleeps[0]]


def kernel_name(c, mode, arith, rec=0):
    return f"_ZN4gpcc21raht_level_sub_kernelILi{c}ELi{mode}ENS_8Arith{arith}ELb0ELb{rec}EEEvNS_8LevelCtxE"


LOSSY = [(1, "I64", 0), (1, "F64", 0), (3, "I64", 0), (3, "F64", 0), (1, "I64", 1), (1, "F64", 1)]


@pytest.mark.parametrize("c,arith,rec", LOSSY)
def test_no_double_division_on_the_chain(kernels, c, arith, rec):
    region = loop_region(kernels[kernel_name(c, 3, arith, rec)])
    bad = [s for s in region if re.match(r"v_(div_\w*f64|rcp_f64)", s)]
    assert not bad, bad


def vm_wait_distances(region):
    """for the loop region: how many instructions lie between the poll and (a) the first vector-memory wait,
    (b) the first vector-memory wait that has at least one DPP move (a butterfly stage) in front of it"""
    waits = [i for i, s in enumerate(region) if s.startswith("s_waitcnt") and "vmcnt" in s]
    dpp = [i for i, s in enumerate(region) if "_dpp" in s]
    stores = [i for i, s in enumerate(region) if re.match(r"(buffer|global)_store", s)]
    return waits, dpp, stores


@pytest.mark.parametrize("arith", ["F64", "I64"])
def test_decoder_poll_is_taken_behind_the_butterflies(kernels, arith):
    """decoder: one wait right behind the poll (the waiting iteration), the other behind all six butterfly
    stages and in front of the granule's store -- none in between"""
    region = loop_region(kernels[kernel_name(1, 1, arith)])
    waits, dpp, stores = vm_wait_distances(region)
    assert len(waits) == 2, [region[i] for i in waits]
    assert waits[0] < dpp[0], "the waiting iteration looks at the answer before any stage body"
    assert waits[1] > dpp[-1], "a vector-memory wait inside the butterflies waits for the poll in flight"
    assert stores and waits[1] < stores[0], "the answer is taken in front of the iteration's first store"


@pytest.mark.parametrize("arith", ["F64", "I64"])
def test_lossy_prediction_stage_has_no_memory_wait(kernels, arith):
    """lossy encoder: behind the waiting iteration's wait, the next vector-memory wait comes after the three forward
    butterfly stages of (P) -- they are the first DPP moves of the region"""
    region = loop_region(kernels[kernel_name(1, 3, arith)])
    waits, dpp, stores = vm_wait_distances(region)
    assert waits[0] < dpp[0]
    fwd = dpp[:6]  # three stages, two 32-bit halves each
    assert waits[1] > fwd[-1], (waits[:3], fwd)


@pytest.mark.parametrize("c,mode,arith", [(1, 1, "F64"), (1, 3, "F64"), (1, 1, "I64"), (1, 3, "I64"), (1, 2, "I64")])
def test_slot_tables_are_read_from_lds(kernels, c, mode, arith):
    """the awaited row and the prediction weight of a lane's slot: two ds_read_b32 in front of the poll, no
    12-deep select chain"""
    body = kernels[kernel_name(c, mode, arith)]
    polls = [i for i, s in enumerate(body) if s.startswith("buffer_load_dwordx4") and "sc1" in s]
    before = body[polls[0] - 12:polls[0]]
    assert sum(s.startswith("ds_read_b32") for s in before) >= 2, before
    assert sum(s.startswith("v_cndmask") for s in before) <= 2, before


# instructions between the poll and the idle sleep: the build that introduced this file has 277 / 996 (346 / 1068
# before it: the double-precision butterfly stages are one straight line for the whole group, no branch per side)
@pytest.mark.parametrize("mode,bound", [(1, 290), (3, 1040)])
def test_loop_region_size_of_the_headline_kernels(kernels, mode, bound):
    region = loop_region(kernels[kernel_name(1, mode, "F64")])
    assert len(region) <= bound, len(region)
