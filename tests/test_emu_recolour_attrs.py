"""CPU tier: gpcc_recolour_attrs' kernels (recolour_kernels.hpp: rc_forward_attrs / rc_forward_limit_attrs /
rc_blend_attrs around the attribute-free backward and list kernels) under the CPU wavefront emulator.  One
emulated call with several attributes on the same positions against what pcc::recolour gives for each attribute
ALONE (the compiled reference where present, else the oracle restatement), ties included; every attribute array and
every output stands between guard bytes that the harness compares after the run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recolour_attrs_cases as rac
from mpeg_pcc_tmc13_amd import RecolourAttr, recolour_params, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", EMU_DIR, "-f", "recolour_attrs.mk", "librc_attrs_emu.so"], check=True,
                       stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(EMU_DIR, "librc_attrs_emu.so"))
        _lib.rc_attrs_emu_recolour.restype = C.c_int
        _lib.rc_attrs_emu_recolour.argtypes = [C.c_void_p, _i32p, C.c_int32, _i32p, C.c_int32, C.POINTER(RecolourAttr),
                                               C.c_int32, C.c_float, _i32p]
    return _lib


def emu_recolour_attrs(p, xyz, attrs, tgt, scale=1.0, offset=(0, 0, 0)):
    """-> the outputs; asserts the harness's return code: 0 means every guard band is intact too"""
    xyz = np.ascontiguousarray(xyz, dtype=np.int32)
    tgt = np.ascontiguousarray(tgt, dtype=np.int32)
    table = (RecolourAttr * len(attrs))()
    srcs, outs = [], []
    for i, (a, bitdepth) in enumerate(attrs):
        sa = np.ascontiguousarray(a, dtype=np.int32).reshape(len(xyz), -1)
        out = np.full((len(tgt), sa.shape[1]), -77, dtype=np.int32)
        srcs.append(sa)
        outs.append(out)
        table[i].src, table[i].tgt, table[i].c, table[i].bitdepth = sa.ctypes.data, out.ctypes.data, sa.shape[1], bitdepth
    rc = lib().rc_attrs_emu_recolour(C.addressof(p), xyz.reshape(-1), len(xyz), tgt.reshape(-1), len(tgt), table,
                                     len(attrs), scale, np.asarray(offset, dtype=np.int32))
    assert rc == 0, f"harness returned {rc} (-4: a guard band or a source array was written)"
    return outs


@pytest.mark.parametrize("kind,scale,kw", rac.MATRIX)
def test_one_emulated_call_gives_each_attribute_its_own_result(kind, scale, kw):
    """[colour(8), reflectance(10)] on a colour cloud, [reflectance(8), colour(8)] on a lidar sweep"""
    rac.check_orders(lambda p, xyz, attrs, tgt, s: emu_recolour_attrs(p, xyz, attrs, tgt, scale=s), kind, scale, kw,
                     rac.TWO)


@pytest.mark.parametrize("kind,scale,kw", rac.NEIGHBOUR_CASES)
def test_an_attribute_does_not_depend_on_its_neighbours_in_the_call(kind, scale, kw):
    """the two attributes reversed, and four: colour, reflectance, colour + 9 mod 256, reflectance reversed"""
    rac.check_orders(lambda p, xyz, attrs, tgt, s: emu_recolour_attrs(p, xyz, attrs, tgt, scale=s), kind, scale, kw,
                     rac.REVERSED_AND_FOUR)


def test_the_two_limits_trim_the_attributes_of_a_call_differently():
    """the inputs do exercise it: under both attribute limits most targets differ from the result without limits,
    for either attribute"""
    _, _, _, _, limited = rac.case("dense", 0.37, rac.key(dict(max_attr_fwd=200.0, max_attr_bwd=300.0)))
    _, _, _, _, free = rac.case("dense", 0.37, rac.key({}))
    for a in (0, 1):
        assert np.any(limited[a] != free[a], axis=1).mean() > 0.5


def test_duplicates_offset_and_small_clouds():
    xyz, a = synth.dense_cloud(3000, seed=5, bits=6)
    xyz = np.concatenate([xyz, xyz[::3], xyz[::7]])
    a = np.concatenate([a, (a[::3] + 9) % 256, (a[::7] + 31) % 256]).astype(np.int32)
    b = np.random.default_rng(77).integers(0, 1024, (len(xyz), 1)).astype(np.int32)
    p = recolour_params(bitdepth=8)
    for scale, off in ((1.0, (0, 0, 0)), (0.5, (3, -2, 5))):
        tgt = np.unique(np.rint(xyz.astype(np.float64) * scale).astype(np.int32) - np.array(off, dtype=np.int32), axis=0)
        got = emu_recolour_attrs(p, xyz, [(a, 8), (b, 10)], tgt, scale=scale, offset=off)
        np.testing.assert_array_equal(got[0], rac.alone(p, xyz, a, 8, tgt, scale=scale, offset=off))
        np.testing.assert_array_equal(got[1], rac.alone(p, xyz, b, 10, tgt, scale=scale, offset=off))
    # as many points as forward neighbours on identical clouds, then a single target
    xyz, a = synth.random_cloud(8, seed=2, bits=3, c=3)
    b = np.random.default_rng(77).integers(0, 1024, (8, 1)).astype(np.int32)
    assert p.num_neighbours_fwd == 8 == len(xyz)
    for tgt in (xyz, xyz[:1]):
        got = emu_recolour_attrs(p, xyz, [(b, 10), (a, 8)], tgt)
        np.testing.assert_array_equal(got[0], rac.alone(p, xyz, b, 10, tgt))
        np.testing.assert_array_equal(got[1], rac.alone(p, xyz, a, 8, tgt))
