"""The in-wavefront hand-over at the top of the sub-node level kernels' staged loop
(mpeg-pcc-tmc13_amd/csrc/raht_subnode.hpp, stage X: children of blocks claimed by the same wavefront are taken
from the wavefront's LDS mailbox), pinned on the gfx950 ISA:

* it is indexed by producer group: the only loop around the mailbox value read (ds_read_b64) is the scalar loop over
  the groups that have committed since it last ran -- no per-slot walk over what the lanes still await;
* the section from the top of the staged loop to the first granule poll stays within 5 % of its instruction count.

Same listing as tests/test_isa_sub_hop.py (GPCC_ISA_LISTING, else tests/isa/sub_kernels.hip compiled here) -- no GPU
needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """kernel name -> its instructions and labels in listing order; a label keeps the compiler's note on the loop its
    block belongs to (`name: ; in Loop: Header=BB0_1 Depth=2`)"""
    out = str(tmp_path_factory.mktemp("isa_mailbox") / "gpcc.s")
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
            if ln.startswith(".Lfunc_end"):
                cur = None
                continue
            s = ln.split(";")[0].strip()
            if s.endswith(":"):
                bodies[cur].append(s + " ;" + ln.partition(";")[2].rstrip())
            elif s and not s.startswith("."):
                bodies[cur].append(s)
    return bodies


def kernel_name(c, mode, arith):
    return f"_ZN4gpcc21raht_level_sub_kernelILi{c}ELi{mode}ENS_8Arith{arith}ELb0ELb0EEEvNS_8LevelCtxE"


def is_label(s):
    return ": ;" in s


def successors(body):
    """index -> indices control can go to next (labels are entries of their own)"""
    at = {s.split(":")[0]: i for i, s in enumerate(body) if is_label(s)}
    succ = []
    for i, s in enumerate(body):
        m = re.match(r"(s_c?branch\w*)\s+(\S+)", s)
        nxt = [i + 1] if i + 1 < len(body) and not s.startswith(("s_endpgm", "s_branch")) else []
        if m and m.group(2) in at:
            nxt.append(at[m.group(2)])
        succ.append(nxt)
    return succ


def reach(start, succ, stop):
    """what control reaches from `start` without going on from a line in `stop`"""
    seen, todo = set(), [start]
    while todo:
        i = todo.pop()
        if i in seen:
            continue
        seen.add(i)
        if i not in stop:
            todo.extend(succ[i])
    return seen


def hand_over(body):
    """-> (lines, succ): the hand-over section -- every line on a path from the top of the staged loop to its first granule
    poll.  The compiler places blocks of the section anywhere in the kernel, so paths are followed, not the listing
    order; the top is the header of the loop of depth 2 that holds the poll, as the compiler's notes name it."""
    polls = [i for i, s in enumerate(body) if s.startswith("buffer_load_dwordx4") and "sc1" in s]
    assert polls, "no granule poll found"
    poll = polls[0]
    succ = successors(body)
    at = {s.split(":")[0]: i for i, s in enumerate(body) if is_label(s)}
    note = next(body[i] for i in range(poll, -1, -1) if is_label(body[i]))
    m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=2", note)
    assert m, note
    top = at[".L" + m.group(1)]
    pred = [[] for _ in body]
    for i, nxt in enumerate(succ):
        for n in nxt:
            pred[n].append(i)
    # (a path that leaves the staged loop enters a block of the loop over the rounds, or of none: the prologue stays out)
    outer = {i for i, s in enumerate(body) if is_label(s) and (re.search(r"Header[=:] ?\S* ?Depth=1$", s) or "Loop" not in s)}
    assert top not in outer and len(outer) > 2
    lines = reach(top, succ, {poll} | outer) & reach(poll, pred, {top} | outer)
    return sorted(lines - {poll}), succ


def instructions(body, lines):
    return [body[i] for i in lines if not is_label(body[i])]


KERNELS = [(1, 1, "F64"), (1, 1, "I64"), (1, 3, "F64"), (1, 3, "I64"), (1, 2, "I64")]


@pytest.mark.parametrize("c,mode,arith", KERNELS)
def test_mailbox_read_sits_in_the_scalar_loop_over_new_groups_only(kernels, c, mode, arith):
    body = kernels[kernel_name(c, mode, arith)]
    lines, succ = hand_over(body)
    inside = set(lines)
    sub = [[n for n in succ[i] if n in inside] if i in inside else [] for i in range(len(body))]
    back = [[] for _ in body]
    for i, nxt in enumerate(sub):
        for n in nxt:
            back[n].append(i)
    reads = [i for i in lines if body[i].startswith("ds_read_b64")]
    assert reads, "the mailbox value read is not in the hand-over section"
    for r in reads:
        # every line that lies on a cycle through the read
        cycle = {i for n in sub[r] for i in reach(n, sub, set())} & {i for n in back[r] for i in reach(n, back, set())}
        if r not in cycle:
            continue
        # a branch that decides whether the cycle goes round once more: the wave-uniform set of newly committed groups
        # lives in scalar registers, so the trip condition is a scalar compare -- never lanes' state (vcc / exec)
        exits = [i for i in cycle if len(succ[i]) == 2 and len([n for n in succ[i] if n in cycle]) == 1]
        assert exits
        for i in exits:
            assert re.match(r"s_cbranch_scc[01]\s", body[i]), body[i]


# instructions on the paths from the top of the staged loop to the first granule poll: the build that introduced this file
# has the counts below (bound: + 5 %).  With the per-slot walk it replaced: 79 / 84 / 84 / 85 / 83 (the second and the
# last in listing order: there the compiler had folded the staged loop into the loop over the rounds).
@pytest.mark.parametrize("c,mode,arith,count", [k + (n,) for k, n in zip(KERNELS, (59, 61, 64, 66, 61))])
def test_hand_over_section_size(kernels, c, mode, arith, count):
    body = kernels[kernel_name(c, mode, arith)]
    n = len(instructions(body, hand_over(body)[0]))
    print(f"hand-over section of <{c},{mode},Arith{arith}>: {n} instructions")
    assert n <= count + count // 20, n
