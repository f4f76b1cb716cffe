"""The C ABI of the device tier's RAHT slice coder (gpcc_dev_raht_encode_attr, gpcc_dev_raht_decode_attr): both symbols
are declared, exported and mirrored, the ABI version is unchanged, and every refusal -- null pointers, the slice
table, the component count, the parameter block, the bit depth, a slice's region count -- returns
GPCC_ERR_INVALID_ARG ahead of the context with the caller's guard-patterned buffers unchanged.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mpeg_pcc_tmc13_amd import raht_params
from mpeg_pcc_tmc13_amd.params import QpRegions, qp_regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpcc_dev_raht_encode_attr", "gpcc_dev_raht_decode_attr"]
GPCC_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from mpeg_pcc_tmc13_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_entries_declared_exported_and_mirrored(lib):
    from mpeg_pcc_tmc13_amd import _lib, raht
    h = open(os.path.join(ROOT, "include", "gpcc_attr_mi355.h")).read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", h, re.M), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.ABI_SYMBOLS
        assert getattr(lib, name).argtypes, f"{name} has no argtypes"
    assert int(re.search(r"#define GPCC_ABI_VERSION (\d+)", h).group(1)) == 6 == lib.gpcc_abi_version() == _lib.ABI_VERSION
    assert hasattr(raht.Context, "dev_raht_attr")


def ptr(a):
    return None if a is None else a.ctypes.data


class Call:
    """valid-looking arguments (never read: the calls fail before); the "device" pointers are host arrays"""

    def __init__(self, encode):
        self.encode = encode
        self.params = raht_params()
        self.slices, self.off = 2, (C.c_int64 * 3)(0, 3, 5)
        self.xyz = np.full(15, -7, np.int32)
        self.attrs = np.full(15, -7, np.int32)
        self.co = np.full(15, -7, np.int32)
        self.order = np.full(5, -7, np.int32)
        self.regions = None
        self.c, self.bitdepth = 3, 8

    def call(self, lib):
        fn = lib.gpcc_dev_raht_encode_attr if self.encode else lib.gpcc_dev_raht_decode_attr
        reg = None if self.regions is None else C.cast(self.regions, C.c_void_p)
        return fn(None, None if self.params is None else C.byref(self.params), reg, self.slices, self.off, ptr(self.xyz),
                  ptr(self.attrs), ptr(self.co), ptr(self.order), self.c, self.bitdepth)

    def untouched(self):
        return all(a is None or (a == -7).all() for a in (self.xyz, self.attrs, self.co, self.order))


def reached_the_context(lib, rc):
    return rc == GPCC_ERR_INVALID_ARG and b"ctx is null" in lib.gpcc_last_error()


def refused(lib, encode, **change):
    a = Call(encode)
    for k, v in change.items():
        setattr(a, k, v)
    rc = a.call(lib)
    assert rc == GPCC_ERR_INVALID_ARG and not reached_the_context(lib, rc), change
    assert lib.gpcc_last_error()
    assert a.untouched()


def reaches(lib, encode, **change):
    a = Call(encode)
    for k, v in change.items():
        setattr(a, k, v)
    assert reached_the_context(lib, a.call(lib)), change
    assert a.untouched()


def region_table(*counts):
    arr = (QpRegions * len(counts))()
    for s, k in enumerate(counts):
        if 0 <= k <= 8:
            arr[s] = qp_regions([((0, 0, 0), (3, 3, 3), (1, -1))] * k)
        else:
            arr[s].num_qp_regions = k
    return arr


def bad_params():
    for field, value in (("num_qp_layers", 0), ("num_qp_layers", 99), ("num_ac_qp_layers", -1), ("num_ac_qp_layers", 99)):
        p = raht_params()
        setattr(p, field, value)
        yield p


@pytest.mark.parametrize("encode", [True, False])
def test_refusals_need_no_context(lib, encode):
    for null in ("params", "off", "xyz", "attrs", "co"):
        refused(lib, encode, **{null: None})
    refused(lib, encode, slices=0)
    refused(lib, encode, slices=-1)
    for off in ((1, 3, 5), (0, 0, 5), (0, 3, 3), (0, 3, 2), (0, 3, (1 << 29) + 1)):
        refused(lib, encode, off=(C.c_int64 * 3)(*off))
    for c in (0, -1, 4):
        refused(lib, encode, c=c)
    for p in bad_params():
        refused(lib, encode, params=p)
    for bitdepth in (0, -1, 17, 32):
        refused(lib, encode, bitdepth=bitdepth)
    for counts in ((-1, 0), (0, 9), (8, 1 << 20)):
        refused(lib, encode, regions=region_table(*counts))


@pytest.mark.parametrize("encode", [True, False])
def test_valid_arguments_reach_the_context_check(lib, encode):
    for change in (dict(), dict(order=None), dict(c=1), dict(c=2), dict(bitdepth=1), dict(bitdepth=16),
                   dict(regions=region_table(0, 0)), dict(regions=region_table(8, 0)),
                   dict(slices=1, off=(C.c_int64 * 2)(0, 5)), dict(off=(C.c_int64 * 3)(0, 1, 1 << 29))):
        reaches(lib, encode, **change)
