"""K4 (dr_msac_score) and K4r (dr_rigid_residual) on every launch path, byte for byte: the outputs are slices of sentinel-filled
guarded buffers, compared with the f64 reference of tests/msac_ref.py under its mask, score, sentinel and guard rules.  Every
case first asserts, through the restated launch rule, the path it is meant to reach.  (The trace helper of
test_gpu_launch_trace.py records entry points, not kernel names, so the kernel is named by the restated rule alone.)

Measured (one MI355X, docs/LOG.md, "K4 / K4r launch-path tests"): worst score error / tolerance 0.088 over all paths, worst excluded share
of a case 3.3e-4 of its bytes and 6.1e-3 of its inliers (caps 1e-3, 1e-2), no differing byte outside the exclusion; 63 tests in 3.4 s."""
import pytest
import torch

from tests import msac_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
STATS = {}      # group:kernel -> the worst excluded shares and score error / tolerance of the run


@pytest.fixture(scope="module", autouse=True)
def _report():
    """after the module's last test: the worst figures per launch path (shown by pytest -s)"""
    yield
    for k in sorted(STATS):
        print("STATS", k, STATS[k])


def _cases(group, **kw):
    return [c for c in R.gpu_cases() if c["group"] == group and all(c[k] == v for k, v in kw.items())]


def _thr(c, dev):
    return torch.full((c["P"],), c["thr"], dtype=c["dtype"], device=dev)


def _run(dev, c, expect=None, gate=None, gated=None, want_masks=None, models_scale=None):
    """one case under the sentinel harness -> (buffers, expectation, valid, dispatch)"""
    P, M, N = c["P"], c["M"], c["N"]
    want_masks = c["want_masks"] if want_masks is None else want_masks
    d = R.dispatch(P, M, N, c["dtype"], c["offset"] % 16 == 0 or not want_masks)
    if expect is not None:
        assert d[:len(expect)] == expect, (c, d)
    mt, md, valid, refs = R.case_inputs(c)
    sel = torch.arange(P) % mt.shape[0]
    mtd, mdd = mt.to(dev)[sel.to(dev)], md.to(dev)[sel.to(dev)]
    if models_scale is not None:
        mdd = mdd * models_scale
    vd = None if valid is None else valid.to(dev)
    bufs = R.call_with_sentinels(mtd, mdd, _thr(c, dev), vd, want_masks, c["offset"], gate)
    exp = R.stack_refs(refs, R.c_red(d[3], d[2]), R.unit(c["dtype"]))
    st = R.compare(*bufs, exp, P, valid=vd, gated=gated, stats=STATS.setdefault(c["group"] + ":" + d[0] + str(d[1]), {}))
    print(c["group"], d, (P, M, N), c["offset"], c["pattern"], c["special"], st)
    return bufs, exp, vd, d


def _outputs(bufs, P, M, N):
    mb, m0, sb, s0 = bufs
    return sb[s0:s0 + P * M].clone(), (None if mb is None else mb[m0:m0 + P * M * N].clone())


@pytest.mark.parametrize("N", R.SHORT_N)
def test_short_rows(dev, N):
    kernel = "small1" if N <= 64 else "small2" if N <= 128 else "small4"
    cs = _cases("short", N=N)
    assert len(cs) == len(R.SHORT_M) + 4 and {c["offset"] for c in cs} == {0, 1, 2}
    for c in cs:
        _run(dev, c, (kernel,))


@pytest.mark.parametrize("N", R.F16S_N)
def test_fast16_with_16_slot_halves(dev, N):
    cs = _cases("f16s", N=N)
    assert len(cs) == len(R.F16S_P) * len(R.F16S_M)
    ny = 2 if N > 2048 else 1
    for c in cs:
        _run(dev, c, ("fast16", 16, ny, 1, ny > 1))


@pytest.mark.parametrize("P,M,N", R.F16L)
def test_fast16_with_64_slot_halves(dev, P, M, N):
    (c,) = _cases("f16l", P=P, M=M)
    _run(dev, c, ("fast16", 64, 1, 1, False))


@pytest.mark.parametrize("shape,expect", [(R.F16L_ATOMIC, ("fast16", 64, 2, 1, True)),      # point range split over blocks, atomic scores
                                          (R.F16L_RELOAD, ("fast16", 64, 1, 2, False)),     # two chunks inside the block: the reload path
                                          (R.F16S_CHUNKS, ("fast16", 16, 2, 2, True))])
def test_fast16_point_range_walks(dev, shape, expect):
    (c,) = _cases("f16x", P=shape[0])
    _run(dev, c, expect)


@pytest.mark.parametrize("N", R.F8_N + R.F8_N16)
def test_eight_point_kernel(dev, N):
    cs = _cases("f8", N=N)
    assert {c["offset"] for c in cs} == ({8} if N % 16 == 0 else {0, 1})
    for c in cs:
        _run(dev, c, ("fast8", 64, 2 if N > 2048 else 1, 1))


@pytest.mark.parametrize("N", R.F64_N)
def test_f64_generic_kernel(dev, N):
    cs = _cases("f64", N=N)
    assert len(cs) == 2 * len(R.F64_M)
    for c in cs:
        _run(dev, c, ("generic", 32, 2 if N > 2048 else 1, 1))


@pytest.mark.parametrize("P,N,expect", [(3, 272, ("fast16", 16)), (512, 272, ("fast16", 64)), (3, 257, ("fast8", 64)),
                                        (3, 255, ("small4", 16))])
def test_validity_patterns_with_special_models(dev, P, N, expect):
    cs = _cases("patterns", P=P, N=N)
    assert [c["pattern"] for c in cs] == [None] + list(R.VALID_PATTERNS) and all(c["special"] for c in cs)
    for c in cs:
        _run(dev, c, expect)


@pytest.mark.parametrize("P,N", [(3, 272), (512, 272), (3, 2064)])
def test_huge_and_tiny_thresholds(dev, P, N):
    for c in _cases("props", P=P, N=N):
        bufs, exp, _, _ = _run(dev, c)
        s, k = _outputs(bufs, P, c["M"], N)
        if c["thr"] == R.THR_HUGE:
            assert (k == 1).all()                       # every row all ones
        else:
            assert (k == 0).all() and (s == 0).all()    # every row empty


@pytest.mark.parametrize("shape", [(3, 70, 272), (512, 70, 272), (3, 70, 257), (3, 33, 255), R.F16L_ATOMIC])
def test_scores_without_masks_repeats_and_model_scale(dev, shape):
    P, M, N = shape
    c = (_cases("patterns", P=P, N=N, pattern="alternating") + _cases("f16x", P=P))[0]
    b1, exp, vd, d = _run(dev, c)
    s1, k1 = _outputs(b1, P, M, N)
    s2, k2 = _outputs(_run(dev, c)[0], P, M, N)
    s3, _ = _outputs(_run(dev, dict(c, offset=0), want_masks=False)[0], P, M, N)     # (scores alone pass the score rule in _run)
    assert torch.equal(k1, k2)
    if d[2] == 1:   # ny == 1: one block owns a score, nothing is accumulated across blocks
        assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(s1.view(torch.int32), s3.view(torch.int32))
    assert d[2] <= 2    # ny == 2: two atomic adds onto a zeroed score, (0 + a) + b == (0 + b) + a: the order cannot show
    for scale in (2.0 ** 20, 2.0 ** -20):
        s4, k4 = _outputs(_run(dev, c, models_scale=scale)[0], P, M, N)
        assert torch.equal(k1, k4)
        assert torch.equal(s1.view(torch.int32), s4.view(torch.int32))


@pytest.mark.parametrize("P", [3, 512])
def test_gate_leaves_terminated_pairs_untouched(dev, P):
    (c,) = _cases("patterns", P=P, N=272, pattern="all_but_one")
    gated = (torch.arange(P) % 3 == 1).to(dev)
    iters = torch.where(gated, 100, 99).to(torch.int32)
    gate = (iters, torch.full((P,), 100.0, dtype=F64, device=dev))
    _run(dev, c, ("fast16",), gate=gate, gated=gated)


# ---- K4r ---------------------------------------------------------------------------------------------------------------------
_RIGID = {}


def _rigid(dev, P, M, N, threshold, accumulate, dtype=F32):
    """pair p takes set p % 3 of the three distinct (points, models) sets"""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    kernel, tile, ny, cpb = R.rigid_dispatch(P, M, N, threshold, dtype, True, cus)
    mmax = max(max(R.RIGID_M), M)
    key = (N, dtype, mmax)
    if key not in _RIGID:
        pts, md = R.rigid_sets(3, mmax, N, 3000 + N, dtype)
        _RIGID[key] = (pts, md, {})
    pts, md, refs = _RIGID[key]
    thr = threshold if dtype == F64 else float(torch.tensor(threshold, dtype=F32))
    if threshold not in refs:
        refs[threshold] = [R.rigid_ref(pts[s], md[s], thr, R.unit(dtype)) for s in range(3)]
    rs = [{k: (v[:M] if torch.is_tensor(v) else v) for k, v in r.items()} for r in refs[threshold][:min(P, 3)]]
    sel = torch.arange(P) % len(rs)
    bufs = R.call_rigid_with_sentinels(pts[sel].to(dev), md[sel, :M].contiguous().to(dev), threshold, accumulate)
    exp = R.stack_refs(rs, R.c_red_rigid(cpb, ny), R.unit(dtype))
    st = R.compare(*bufs, exp, P, stats=STATS.setdefault("rigid:" + kernel + (":tile%d" % tile if kernel == "pk8" else ""), {}))
    print("rigid", (kernel, tile, ny, cpb), (P, M, N), threshold, accumulate, st)
    return kernel, tile


@pytest.mark.parametrize("N", R.RIGID_N)
def test_rigid_residual_packed_kernel(dev, N):
    for P in R.RIGID_P:
        for M in R.RIGID_M:
            for acc in (False, True):
                kernel, tile = _rigid(dev, P, M, N, 9e-4, acc)
                assert (kernel, tile) == ("pk8", 4)     # (the smallest tile: these grids are far below one round of resident blocks)


@pytest.mark.parametrize("shape,tile256", [(R.RIGID_TILE6, 6), (R.RIGID_TILE34, 34), (R.RIGID_TILE64, 64)])
def test_rigid_residual_packed_kernel_larger_tiles(dev, shape, tile256):
    """the tile follows the device's compute units; with 256 of them these shapes get 6, 34 and kR16MaxTile = 64, each with a partial
    last tile"""
    P, M, N = shape
    assert R.rigid_dispatch(P, M, N, 9e-4)[:2] == ("pk8", tile256) and M % tile256 != 0
    for acc in (False, True):
        kernel, tile = _rigid(dev, P, M, N, 9e-4, acc)
        assert kernel == "pk8"
        if torch.cuda.get_device_properties(dev).multi_processor_count == 256:
            assert tile == tile256


@pytest.mark.parametrize("N,threshold,dtype", [(2064, 1e-12, F32), (2063, 9e-4, F32), (2047, 9e-4, F64)])
def test_rigid_residual_general_kernel(dev, N, threshold, dtype):
    for P in R.RIGID_P:
        for M in (1, 33, 70):
            for acc in ((False, True) if dtype == F32 else (False,)):
                assert _rigid(dev, P, M, N, threshold, acc, dtype)[0] == "general"
