"""GPU tier: the in-wavefront hand-over of the sub-node level kernels (mpeg-pcc-tmc13_amd/csrc/raht_subnode.hpp) on the
shapes of tests/test_emu_sub_mailbox.py -- Morton octets whose last group awaits seven groups of its own round, rounds
that are not octet-aligned, two slices in one round, a partly dead last round -- forward and inverse through the device
tier, equal to the oracle, and ctx.synchronize() clean: no bounded wait of the dependency loop expired."""
import numpy as np
import pytest

import oracle_loader as ol
from test_emu_sub_mailbox import grid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    yield c
    c.close()


# (a level goes to the per-level kernels where a slice has more than 256 parents -- kSweepDefaultParents, raht_sweep.hpp --
# so the fully occupied cube is 16 x 16 x 16 here: 512 octets at the finest level; the finest level of the grids has
# about 480 and 512 parents)
def cube(c):
    return [grid(16, 1.0, 5, c)]


def sparse30(c):
    return [grid(16, 0.3, 11, c)]


def sparse60(c):
    return [grid(16, 0.6, 21, c)]


def two_slices(c):
    return [grid(16, 0.3, 31, c), grid(8, 1.0, 32, c)]


def partly_dead(c):
    m, a = grid(16, 0.6, 41, c)
    return [(m[:1496], a[:1496])]


# shape, components, double-precision back end where it is exact (else int64), params
CASES = [(cube, 1, True, dict(qp=28)), (cube, 3, False, dict(qp=34)), (cube, 1, False, dict(qp=28, extension=False)),
         (sparse30, 3, True, dict(qp=28)), (sparse30, 1, False, dict(qp=22)),
         (sparse60, 1, True, dict(qp=22)), (sparse60, 3, False, dict(qp=28, extension=False)),
         (two_slices, 1, True, dict(qp=28)), (two_slices, 1, False, dict(qp=28)),
         (partly_dead, 1, True, dict(qp=34)),
         (two_slices, 1, False, dict(haar=True, qp=4, chroma_offset=0))]


@pytest.mark.parametrize("shape,c,fast,kw", CASES, ids=[
    f"{s.__name__}-c{c}-{'f64' if f else 'i64'}-" + "-".join(f"{k}{v}" for k, v in kw.items()) for s, c, f, kw in CASES])
def test_device_tier_equals_the_oracle(shape, c, fast, kw, ctx):
    import torch
    from mpeg_pcc_tmc13_amd import raht_params
    p = raht_params(**kw)
    slices = shape(c)
    offsets = np.concatenate([[0], np.cumsum([len(m) for m, _ in slices])]).astype(np.int64)
    dev = torch.device("cuda:0")
    d_m = torch.from_numpy(np.concatenate([m for m, _ in slices])).to(dev)
    d_a = torch.from_numpy(np.concatenate([a for _, a in slices]).reshape(-1)).to(dev)
    d_c = torch.zeros(c * int(offsets[-1]), dtype=torch.int32, device=dev)
    d_inv = torch.zeros_like(d_a)
    torch.cuda.synchronize()
    ctx.set_fast_arith(fast)
    ctx.set_morton_bits(12)
    try:
        ctx.dev_raht_forward(p, offsets, d_m.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), c)
        ctx.synchronize()
        ctx.dev_raht_inverse(p, offsets, d_m.data_ptr(), d_inv.data_ptr(), d_c.data_ptr(), c)
        ctx.synchronize()
    finally:
        ctx.set_morton_bits(0)
        ctx.set_fast_arith(True)
    co, rec, inv = d_c.cpu().numpy(), d_a.cpu().numpy().reshape(-1, c), d_inv.cpu().numpy().reshape(-1, c)
    for i, (m, a) in enumerate(slices):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        o_co, o_rec = ol.oracle().raht_forward(p, m, a)
        np.testing.assert_array_equal(co[c * lo:c * hi], o_co, err_msg=f"slice {i} coefficients")
        np.testing.assert_array_equal(rec[lo:hi], o_rec, err_msg=f"slice {i} encoder reconstruction")
        np.testing.assert_array_equal(inv[lo:hi], o_rec, err_msg=f"slice {i} decoder")
