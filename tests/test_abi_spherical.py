"""The C ABI of the spherical-domain attribute positions (spherical_coord_flag): the two entries are declared,
exported and mirrored, the ABI version is unchanged, the parameter block has the size of its ctypes mirror, and
every argument error is refused ahead of the context.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gpcc_attr_to_spherical", "gpcc_dev_attr_to_spherical"]
GPCC_ERR_INVALID_ARG, GPCC_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    from mpeg_pcc_tmc13_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def header():
    return open(os.path.join(ROOT, "include", "gpcc_attr_mi355.h")).read()


def test_entries_declared_exported_and_mirrored(lib):
    from mpeg_pcc_tmc13_amd import _lib, raht, params, synth
    h = header()
    for name in ENTRIES:
        assert re.search(r"^int " + name + r"\(", h, re.M), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.ABI_SYMBOLS
        assert getattr(lib, name).argtypes, f"{name} has no argtypes"
    assert int(re.search(r"#define GPCC_ABI_VERSION (\d+)", h).group(1)) == 6 == lib.gpcc_abi_version()
    for name in ("attr_to_spherical", "dev_attr_to_spherical", "dev_attr_morton_sort"):
        assert hasattr(raht.Context, name)
    assert int(re.search(r"#define GPCC_MAX_LASERS (\d+)", h).group(1)) == params.GPCC_MAX_LASERS >= 64
    origin, thetas = synth.lidar_lasers()
    assert origin.shape == (3,) and len(thetas) == 64 and (np.diff(thetas) > 0).all()
    # the table belongs to lidar_cloud's rings: tan(-24.8 deg) and tan(+2 deg) in 18-bit fixed point
    assert thetas[0] == round(np.tan(np.deg2rad(-24.8)) * 2**18) and thetas[-1] == round(np.tan(np.deg2rad(2.0)) * 2**18)


def test_struct_size_equals_the_mirror():
    """sizeof(gpcc_spherical_params) as the C compiler sees it"""
    from mpeg_pcc_tmc13_amd import SphericalParams
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "size.c"), os.path.join(tmp, "size")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "gpcc_attr_mi355.h"\n'
                    'int main(void) { printf("%zu %zu %zu\\n", sizeof(gpcc_spherical_params), '
                    'offsetof(gpcc_spherical_params, attr_coord_scale), offsetof(gpcc_spherical_params, convert)); return 0; }\n')
        subprocess.run([os.environ.get("CC", "gcc"), "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        size, off_scale, off_convert = (int(v) for v in subprocess.run([exe], check=True, capture_output=True).stdout.split())
    assert size == C.sizeof(SphericalParams) == 4 * (3 + 1 + 128 + 3 + 1 + 3 + 1)
    assert off_scale == SphericalParams.attr_coord_scale.offset and off_convert == SphericalParams.convert.offset


class Args:
    """valid-looking buffers of a 4-point slice (never read: the calls fail before)"""

    def __init__(self):
        from mpeg_pcc_tmc13_amd import spherical_params
        self.p = spherical_params((0, 0, 0), [-100, 0, 100], (256, 256, 256))
        self.n = 4
        self.xyz = np.array([[10, 0, 0], [0, 10, 0], [-10, 0, 1], [3, 4, 5]], np.int32)
        self.out = np.full((4, 3), -7, np.int32)
        self.bbox = np.full(6, -7, np.int32)
        self.off = (C.c_int64 * 2)(0, 4)
        self.slices = 1

    def host(self, lib, ctx=None, **null):
        def ptr(name, a):
            return None if null.get(name) else a.ctypes.data
        return lib.gpcc_attr_to_spherical(ctx, None if null.get("params") else C.byref(self.p), ptr("xyz", self.xyz), self.n,
                                          ptr("out", self.out), ptr("bbox", self.bbox))

    def dev(self, lib, ctx=None, **null):
        def ptr(name, a):
            return None if null.get(name) else a.ctypes.data
        return lib.gpcc_dev_attr_to_spherical(ctx, None if null.get("params") else C.byref(self.p), self.slices,
                                              None if null.get("off") else self.off, ptr("xyz", self.xyz),
                                              ptr("out", self.out), ptr("bbox", self.bbox))


def bad_params():
    """(what, a change of the parameter block, the code)"""
    def lasers(n):
        def f(p):
            p.num_lasers = n
        return f

    def descending(p):
        p.laser_theta[2] = -1

    def mode(v):
        def f(p):
            p.min_pos_mode = v
        return f

    def convert(p):
        p.convert = 2
    return [("no lasers", lasers(0), GPCC_ERR_INVALID_ARG), ("negative lasers", lasers(-1), GPCC_ERR_INVALID_ARG),
            ("too many lasers", lasers(129), GPCC_ERR_UNSUPPORTED), ("thetas not ascending", descending, GPCC_ERR_INVALID_ARG),
            ("mode 3", mode(3), GPCC_ERR_INVALID_ARG), ("mode -1", mode(-1), GPCC_ERR_INVALID_ARG),
            ("convert 2", convert, GPCC_ERR_INVALID_ARG)]


@pytest.mark.parametrize("tier", ["host", "dev"])
def test_argument_refusals_need_no_context(lib, tier):
    def call(a, **null):
        return getattr(a, tier)(lib, **null)
    for null in ("params", "xyz", "out") + (("off",) if tier == "dev" else ()):
        assert call(Args(), **{null: True}) == GPCC_ERR_INVALID_ARG, null
    for what, change, code in bad_params():
        a = Args()
        change(a.p)
        assert call(a) == code, what
        assert lib.gpcc_last_error()
    if tier == "host":
        for n in (0, -3, (1 << 29) + 1):
            a = Args()
            a.n = n
            assert call(a) == GPCC_ERR_INVALID_ARG, n
    else:
        a = Args()
        a.slices = 0
        assert call(a) == GPCC_ERR_INVALID_ARG
        for off in ((1, 4), (0, 0), (0, -2), (0, (1 << 29) + 1)):
            a = Args()
            a.off = (C.c_int64 * 2)(*off)
            assert call(a) == GPCC_ERR_INVALID_ARG, off
            assert b"ctx" not in lib.gpcc_last_error()
    # valid arguments reach the context check (a null bounding box is allowed), and nothing was written above
    a = Args()
    assert call(a, bbox=True) == GPCC_ERR_INVALID_ARG
    assert b"ctx" in lib.gpcc_last_error()
    assert (a.out == -7).all() and (a.bbox == -7).all()
    # equal neighbours in the table are ascending enough for std::upper_bound
    a = Args()
    a.p.laser_theta[1] = a.p.laser_theta[0]
    assert call(a) == GPCC_ERR_INVALID_ARG and b"ctx" in lib.gpcc_last_error()
