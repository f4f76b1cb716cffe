"""GPU parity: the HIP path through the C ABI against (a) the committed
golden vectors of the compiled reference and (b) the CPU oracle on the same
seeded inputs.  Integer path: bit-exact."""
import numpy as np
import pytest

import oracle_loader as ol
import raht_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "raht_golden.npz"))


@pytest.mark.parametrize("name", rc.CASE_NAMES)
def test_case_vs_golden_and_oracle(name, ctx, golden):
    """Every intra parameter combination runs on the device, forward and inverse."""
    case = rc.CASES[rc.CASE_NAMES.index(name)]
    p, morton, attrs, qp = rc.make_inputs(case)
    n, c = attrs.shape
    coeffs, rec = ctx.raht_forward(p, morton, attrs, qp)
    inv = ctx.raht_inverse(p, morton, coeffs, c, qp)
    assert str(golden[name + "/sha"]) == rc.digest(coeffs) + rc.digest(rec) + rc.digest(inv)
    o_coeffs, o_rec = ol.oracle().raht_forward(p, morton, attrs, qp)
    np.testing.assert_array_equal(coeffs, o_coeffs)
    np.testing.assert_array_equal(rec, o_rec)
    np.testing.assert_array_equal(inv, o_rec)


@pytest.mark.parametrize("seed", range(4))
def test_random_flags_vs_oracle(seed, ctx):
    from mpeg_pcc_tmc13_amd import raht_params, synth
    rng = np.random.default_rng(5000 + seed)
    o = ol.oracle()
    for _ in range(10):
        n = int(rng.integers(1, 4000))
        c = int(rng.choice([1, 2, 3]))
        xyz, attrs = synth.random_cloud(n, seed=int(rng.integers(1 << 30)), bits=int(rng.integers(1, 8)),
                                        c=c, dup_fraction=float(rng.choice([0.0, 0.25])))
        haar = bool(rng.integers(2))
        p = raht_params(
            qp=4 if haar else int(rng.integers(4, 52)), chroma_offset=0 if haar else int(rng.integers(-3, 3)),
            haar=haar, prediction=bool(rng.integers(4) > 0), subnode=bool(rng.integers(2)),
            extension=bool(rng.integers(4) > 0), search_range=int(rng.choice([4, 64, 50000])),
            threshold0=int(rng.integers(0, 6)), threshold1=int(rng.integers(0, 12)))
        morton, a, order = synth.sort_by_morton(xyz, attrs)
        qp_off = rng.integers(-4, 5, size=(n, 2)).astype(np.int32) if rng.integers(3) == 0 else None
        co, rec = ctx.raht_forward(p, morton, a, qp_off)
        o_co, o_rec = o.raht_forward(p, morton, a, qp_off)
        np.testing.assert_array_equal(co, o_co)
        np.testing.assert_array_equal(rec, o_rec)
        np.testing.assert_array_equal(ctx.raht_inverse(p, morton, o_co, c, qp_off), o_rec)


def test_batched_slices_device_tier(ctx):
    """Several ragged slices in one batch == each slice on its own."""
    import torch
    from mpeg_pcc_tmc13_amd import raht_params, synth
    sizes = [1, 7, 3000, 1, 20000, 513, 2]
    p = raht_params(qp=30, subnode=False)
    ms, as_ = [], []
    for i, n in enumerate(sizes):
        xyz, col = synth.random_cloud(n, seed=40 + i, bits=5 if n > 100 else 2, dup_fraction=0.1 if n > 10 else 0.0)
        m, a, _ = synth.sort_by_morton(xyz, col)
        ms.append(m)
        as_.append(a)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    dev = torch.device("cuda:0")
    d_m = torch.from_numpy(np.concatenate(ms)).to(dev)
    d_a = torch.from_numpy(np.concatenate(as_).reshape(-1)).to(dev)
    d_c = torch.zeros(3 * int(offsets[-1]), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.set_morton_bits(15)
    ctx.dev_raht_forward(p, offsets, d_m.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), 3)
    ctx.synchronize()
    rec = d_a.cpu().numpy()
    co = d_c.cpu().numpy()
    d_a2 = torch.zeros_like(d_a)
    ctx.dev_raht_inverse(p, offsets, d_m.data_ptr(), d_a2.data_ptr(), d_c.data_ptr(), 3)
    ctx.synchronize()
    ctx.set_morton_bits(0)
    inv = d_a2.cpu().numpy()
    for i, n in enumerate(sizes):
        o_co, o_rec = ol.oracle().raht_forward(p, ms[i], as_[i])
        b = int(offsets[i])
        np.testing.assert_array_equal(co[3 * b:3 * (b + n)], o_co)
        np.testing.assert_array_equal(rec[3 * b:3 * (b + n)].reshape(n, 3), o_rec)
        np.testing.assert_array_equal(inv[3 * b:3 * (b + n)].reshape(n, 3), o_rec)


def test_full_size_roundtrip_properties(ctx):
    """BASELINE config sizes (1M points): size-independent properties --
    decoder(encoder coefficients) == encoder reconstruction; integer Haar at
    qp 4 is lossless; results are deterministic run to run."""
    from mpeg_pcc_tmc13_amd import raht_params, synth
    xyz, refl = synth.lidar_cloud(1_000_000, seed=3)
    morton, attrs, _ = synth.sort_by_morton(xyz, refl)
    p = raht_params(qp=34, subnode=False, search_range=2500)
    co, rec = ctx.raht_forward(p, morton, attrs)
    co2, rec2 = ctx.raht_forward(p, morton, attrs)
    assert rc.digest(co) == rc.digest(co2) and rc.digest(rec) == rc.digest(rec2)
    np.testing.assert_array_equal(ctx.raht_inverse(p, morton, co, 1), rec)
    ph = raht_params(qp=4, haar=True, chroma_offset=0, subnode=False, search_range=2500)
    co, rec = ctx.raht_forward(ph, morton, attrs)
    np.testing.assert_array_equal(rec, attrs)
    np.testing.assert_array_equal(ctx.raht_inverse(ph, morton, co, 1), attrs)


def test_error_paths(ctx):
    from mpeg_pcc_tmc13_amd import raht_params
    from mpeg_pcc_tmc13_amd._lib import GpccError
    p = raht_params(subnode=False)
    with pytest.raises(GpccError) as ei:
        ctx.raht_forward(p, np.array([5, 3], dtype=np.int64), np.zeros((2, 3), np.int32))
    assert ei.value.code == -6  # unsorted
    with pytest.raises(GpccError):
        ctx.raht_forward(p, np.array([1, 2], dtype=np.int64), np.zeros((2, 4), np.int32))


def test_point_count_limit(ctx):
    """More than GPCC_MAX_POINTS points: refused before any buffer is read."""
    import ctypes as C
    from mpeg_pcc_tmc13_amd import lod_params, raht_params
    lib, h = ctx._lib, ctx._h
    big = (1 << 29) + 1
    buf = np.zeros(16, np.int64)
    ptr = buf.ctypes.data
    p, lp = raht_params(), lod_params()
    assert lib.gpcc_raht_forward(h, C.byref(p), ptr, None, ptr, ptr, big, 1) == -1
    assert b"2^29" in lib.gpcc_last_error()
    assert lib.gpcc_attr_morton_sort(h, ptr, big, ptr, ptr) == -1
    assert lib.gpcc_lod_build(h, C.byref(lp), ptr, big, ptr, ptr, ptr, ptr, ptr, C.byref(C.c_int32())) == -1
    assert lib.gpcc_lod_compute_weights(h, big, ptr, ptr, ptr) == -1


@pytest.mark.parametrize("seed", range(3))
def test_subnode_inverse_random_vs_oracle(seed, ctx):
    """CTC-default flags (sub-node prediction on): decoder on the device."""
    from mpeg_pcc_tmc13_amd import raht_params, synth
    rng = np.random.default_rng(7000 + seed)
    o = ol.oracle()
    for _ in range(8):
        n = int(rng.integers(2, 6000))
        c = int(rng.choice([1, 3]))
        xyz, attrs = synth.random_cloud(n, seed=int(rng.integers(1 << 30)), bits=int(rng.integers(2, 7)),
                                        c=c, dup_fraction=float(rng.choice([0.0, 0.2])))
        p = raht_params(qp=int(rng.integers(10, 46)), subnode=True, extension=bool(rng.integers(4) > 0),
                        search_range=int(rng.choice([8, 50000])))
        morton, a, _ = synth.sort_by_morton(xyz, attrs)
        o_co, o_rec = o.raht_forward(p, morton, a)
        np.testing.assert_array_equal(ctx.raht_inverse(p, morton, o_co, c), o_rec)


def test_subnode_full_size_decode(ctx):
    """1M-point lidar frame, CTC flags: device decode of the reference's
    (oracle's) coefficients equals the encoder reconstruction."""
    from mpeg_pcc_tmc13_amd import raht_params, synth
    xyz, refl = synth.lidar_cloud(300_000, seed=5)
    morton, attrs, _ = synth.sort_by_morton(xyz, refl)
    p = raht_params(qp=34, subnode=True, search_range=2500)
    o_co, o_rec = ol.oracle().raht_forward(p, morton, attrs)
    np.testing.assert_array_equal(ctx.raht_inverse(p, morton, o_co, 1), o_rec)


@pytest.mark.parametrize("kind,n", [("dense", 60000), ("lidar", 90000)])
@pytest.mark.parametrize("qp", [4, 10, 16, 22, 28, 40, 51])
def test_subnode_lossy_qp_sweep(kind, n, qp, ctx):
    """Lossy encoder with sub-node prediction across the rate range: the
    share of coefficients whose RDOQ decision depends on the zero-run state
    (and the reach of their thresholds) changes by orders of magnitude."""
    from mpeg_pcc_tmc13_amd import raht_params, synth
    xyz, attrs = synth.dense_cloud(n, seed=21, bits=9) if kind == "dense" else synth.lidar_cloud(n, seed=21)
    morton, attrs, _ = synth.sort_by_morton(xyz, attrs)
    p = raht_params(qp=qp, subnode=True, search_range=2500 if kind == "lidar" else 50000)
    chk = ol.ref() if ol.ref_available() else ol.oracle()
    want_co, want_rec = chk.raht_forward(p, morton, attrs)
    co, rec = ctx.raht_forward(p, morton, attrs)
    np.testing.assert_array_equal(co, want_co)
    np.testing.assert_array_equal(rec, want_rec)
    np.testing.assert_array_equal(ctx.raht_inverse(p, morton, co, attrs.shape[1]), want_rec)


def _longest_zero_run(co, c):
    nz = np.flatnonzero((co.reshape(c, -1) != 0).any(axis=0))
    return int(np.diff(np.concatenate([[-1], nz, [co.size // c]])).max() - 1)


@pytest.mark.parametrize("subnode", [False, True], ids=["level", "subnode"])
@pytest.mark.parametrize("qp", [28, 40])
def test_sparse_perturbation_long_zero_runs(qp, subnode, ctx):
    """A flat cloud with one point in 5000 perturbed: a few dozen non-zero coefficients with all-zero runs of many
    2048-coefficient tiles between them, so the zero-run state is carried through chains of transparent tiles (and
    through the carriers of the same state in the sub-node, sweep, compact and tile kernels) where natural clouds
    reset it every few coefficients."""
    from mpeg_pcc_tmc13_amd import raht_params, synth
    xyz, attrs = synth.dense_cloud(150000, seed=21, bits=9)
    attrs = np.full_like(attrs, 100)
    n, c = attrs.shape
    rng = np.random.default_rng(1)
    pick = rng.choice(n, n // 5000, replace=False)
    attrs[pick] += rng.integers(1, 40, (len(pick), c)).astype(attrs.dtype)
    morton, attrs, _ = synth.sort_by_morton(xyz, attrs)
    p = raht_params(qp=qp, subnode=subnode, search_range=50000)
    o_co, o_rec = ol.oracle().raht_forward(p, morton, attrs)
    if qp == 28:   # (the data keeps meaning what it means today)
        assert _longest_zero_run(o_co, c) >= 16384
    want_co, want_rec = ol.ref().raht_forward(p, morton, attrs) if ol.ref_available() else (o_co, o_rec)
    co, rec = ctx.raht_forward(p, morton, attrs)
    np.testing.assert_array_equal(co, want_co)
    np.testing.assert_array_equal(rec, want_rec)
    np.testing.assert_array_equal(ctx.raht_inverse(p, morton, co, c), want_rec)


def test_subnode_lossy_multi_slice_levels(ctx):
    """Several slices of different depth in one batch: the zero-run state is
    carried per slice from level to level."""
    import torch
    from mpeg_pcc_tmc13_amd import raht_params, synth
    p = raht_params(qp=28, subnode=True, search_range=50000)
    frames = [synth.sort_by_morton(*synth.dense_cloud(n, seed=31 + i, bits=b)) for i, (n, b) in
              enumerate([(20000, 8), (300, 5), (45000, 9), (1, 4), (9000, 7)])]
    c = frames[0][1].shape[1]
    offsets = np.concatenate([[0], np.cumsum([len(f[0]) for f in frames])]).astype(np.int64)
    dev = torch.device("cuda", 0)
    d_m = torch.from_numpy(np.concatenate([f[0] for f in frames])).to(dev)
    d_a = torch.from_numpy(np.concatenate([f[1] for f in frames]).reshape(-1)).to(dev)
    d_c = torch.zeros(c * int(offsets[-1]), dtype=torch.int32, device=dev)
    ctx.set_morton_bits(27)
    ctx.dev_raht_forward(p, offsets, d_m.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), c)
    ctx.synchronize()
    ctx.set_morton_bits(0)
    co, rec = d_c.cpu().numpy(), d_a.cpu().numpy().reshape(-1, c)
    chk = ol.ref() if ol.ref_available() else ol.oracle()
    for i, f in enumerate(frames):
        a, b = int(offsets[i]), int(offsets[i + 1])
        wco, wrec = chk.raht_forward(p, f[0], f[1])
        np.testing.assert_array_equal(co[c * a:c * b], wco, err_msg=f"slice {i}")
        np.testing.assert_array_equal(rec[a:b], wrec, err_msg=f"slice {i}")


@pytest.mark.parametrize("subnode", [False, True])
def test_neighbour_links_opt_in(subnode, ctx, monkeypatch):
    """GPCC_LINKS=1 (csrc/raht_links.hpp, round 5): the level kernels take their neighbours from the top-down link
    records instead of bisecting -- measured slower on the MI355X (profiles/r05_links_ab.txt) and therefore off by
    default, but bit-exact: the golden cases that use the RAHT extension, multi-slice batches, several search ranges
    (the window is an index distance at the consumer)"""
    from mpeg_pcc_tmc13_amd import _lib, build, raht_params, synth
    if not _lib.load().gpcc_debug_has_experiments():
        # the product library leaves the experiments' branches out (they cost the headline kernel 1.6 %): this test
        # runs in a fresh process on the experiments build that build() makes next to it
        import os
        import subprocess
        import sys
        assert _lib.LIB_PATH != build.LIB_EXPERIMENTS, "the experiments build lacks the experiments"
        assert os.path.exists(build.LIB_EXPERIMENTS), build.LIB_EXPERIMENTS + " is missing: run build()"
        r = subprocess.run([sys.executable, "-m", "pytest", f"{__file__}::test_neighbour_links_opt_in[{subnode}]", "-q",
                            "-m", "gpu"], env=dict(os.environ, GPCC_LIB_PATH=build.LIB_EXPERIMENTS),
                           capture_output=True, text=True, timeout=900, cwd=os.path.dirname(os.path.dirname(__file__)))
        assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
        return
    monkeypatch.setenv("GPCC_LINKS", "1")   # (read by the library at every call)
    o = ol.oracle()
    for kind, n, c, sr in (("dense", 60000, 3, 50000), ("lidar", 90000, 1, 2500), ("dense", 30000, 1, 8), ("lidar", 50000, 1, 8)):
        xyz, attrs = (synth.dense_cloud(n, seed=17, bits=9) if kind == "dense" else synth.lidar_cloud(n, seed=17))
        attrs = np.ascontiguousarray(attrs[:, :c])
        morton, a, _ = synth.sort_by_morton(xyz, attrs)
        p = raht_params(qp=34, subnode=subnode, search_range=sr, chroma_offset=-1 if c == 3 else 0)
        co, rec = ctx.raht_forward(p, morton, a)
        o_co, o_rec = o.raht_forward(p, morton, a)
        np.testing.assert_array_equal(co, o_co)
        np.testing.assert_array_equal(rec, o_rec)
        np.testing.assert_array_equal(ctx.raht_inverse(p, morton, co, c), o_rec)
    monkeypatch.setenv("GPCC_LINKS", "0")
    co0, _ = ctx.raht_forward(p, morton, a)
    np.testing.assert_array_equal(co0, o_co)
