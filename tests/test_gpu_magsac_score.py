"""dr_magsac_score against the f64 gamma-function oracle (tests/magsac_ref.py), through ctypes on sentinel-filled guarded buffers:
every launch path, the slot rules, validity patterns, extreme thresholds, gated pairs, bit-repeatability, and the hand-over to
dr_ransac_update.  Tolerances and caps are magsac_ref's / msac_ref's (derived, not measured on the kernel)."""
import pytest
import torch

from tests import magsac_ref as G
from tests import msac_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
INL_SENTINEL = -77


def launch(matches, models, thr, valid=None, want_inliers=True, gate=None):
    """-> (score buffer, start, inlier buffer | None, start): outputs between guards, all sentinel before the call"""
    from differentiable_ransac_amd import _lib as L
    P, N, _ = matches.shape
    M = models.shape[1]
    _, _, sb, s0 = R.new_buffers(P, M, N, matches.dtype, matches.device, want_masks=False)
    ib, i0 = None, 16
    if want_inliers:
        ib = torch.full((2 * i0 + P * M,), INL_SENTINEL, dtype=torch.int32, device=matches.device)
    v = None if valid is None else valid.contiguous().view(torch.uint8)
    gates = [L.ptr(None), L.ptr(None)] if gate is None else [L.ptr(gate[0]), L.ptr(gate[1])]
    L.call(f"dr_magsac_score_{L.suffix(matches.dtype)}", L.ptr(matches.contiguous()), L.ptr(models.contiguous()), L.ptr(v),
           L.ptr(thr.contiguous()), L.c_int(P), L.c_int(M), L.c_int(N), L.ptr(sb[s0:s0 + P * M]),
           L.ptr(None if ib is None else ib[i0:i0 + P * M]), *gates, L.stream())
    return sb, s0, ib, i0


def check(bufs, refs, P, M, valid=None, gated=None, stats=None):
    sb, s0, ib, i0 = bufs
    S = len(refs)
    sel = torch.arange(P) % S
    ref = {k: torch.stack([r[k][:M] for r in refs])[sel].to(DEV) for k in ("scores", "inliers", "excl", "tol", "nan")}
    live = torch.ones(P, M, dtype=torch.bool, device=DEV) if valid is None else valid.to(DEV).bool()
    open_ = torch.ones(P, dtype=torch.bool, device=DEV) if gated is None else ~gated.to(DEV)
    sent = torch.tensor(R.SCORE_SENTINEL, dtype=sb.dtype, device=DEV)
    scores = sb[s0:s0 + P * M].view(P, M)
    assert (sb[:s0] == sent).all() and (sb[s0 + P * M:] == sent).all(), "score guard overwritten"
    assert (scores[~open_] == sent).all(), "score of a gated pair written"
    nan = ref["nan"] & live
    ev = live & ~nan & open_[:, None]
    so = scores[open_]
    assert not (so == sent).any(), "score left unwritten"
    assert (so[~live[open_]] == 0).all(), "invalid slot: score not exactly 0"
    assert torch.isnan(scores[nan & open_[:, None]]).all(), "non-finite or all-zero model: score not NaN"
    err = (scores.double() - ref["scores"]).abs()
    ratio = torch.where(ev, err / ref["tol"].clamp(min=1e-300), torch.zeros_like(err))
    worst = float(ratio.max())
    assert not torch.isnan(scores[ev]).any() and worst <= 1.0, f"score rule: worst |error| / tolerance = {worst}"
    n_ex, n_in = int((ref["excl"] * ev).sum()), int((ref["inliers"] * ev).sum())
    if ib is not None:
        inl = ib[i0:i0 + P * M].view(P, M)
        assert (ib[:i0] == INL_SENTINEL).all() and (ib[i0 + P * M:] == INL_SENTINEL).all(), "inlier guard overwritten"
        assert (inl[~open_] == INL_SENTINEL).all(), "count of a gated pair written"
        assert (inl[open_][~(ev[open_])] == 0).all(), "invalid / NaN slot: count not 0"
        off = (inl.long() - ref["inliers"]).abs()
        assert (off[ev] <= ref["excl"][ev]).all(), "inlier count differs outside the points with |d2 - thr2| <= 2 bound"
    if stats is not None:
        stats["ratio"] = max(stats.get("ratio", 0.0), worst)
        stats["excl"] = stats.get("excl", 0) + n_ex
        stats["inl"] = stats.get("inl", 0) + n_in
        stats["slots"] = stats.get("slots", 0) + int(ev.sum())
    return n_ex, n_in, int(ev.sum())


def caps(n_ex, n_in, points):
    assert G.within_caps(n_ex, n_in, points), f"excluded points {n_ex}: {n_in} reference inliers, {points} points"


def inputs(mt, md, M, P, thr, dtype):
    S = mt.shape[0]
    sel = torch.arange(P) % S
    return (mt[sel].to(DEV).contiguous(), md[sel][:, :M].to(DEV).contiguous(),
            torch.full((P,), float(thr), dtype=dtype, device=DEV))


def test_every_launch_path_is_reached():
    assert {G.dispatch(*s) for s in G.score_shapes()} == G.intended_paths()


@pytest.mark.parametrize("N,dtype", [(n, torch.float32) for n in G.SCORE_N + (G.SCORE_CHUNKS[2],)] + [(n, torch.float64) for n in G.F64_N],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_shapes(N, dtype):
    mt, md, refs = G.sweep_inputs(N, dtype)
    shapes = [s for s in G.score_shapes() if s[2] == N and s[3] == dtype]
    assert shapes
    stats = {}
    for i, (P, M, _, _) in enumerate(shapes):
        m, d, thr = inputs(mt, md, M, P, R.THR, dtype)
        bufs = launch(m, d, thr, want_inliers=i % 2 == 0)
        n_ex, n_in, slots = check(bufs, refs, P, M, stats=stats)
        caps(n_ex, n_in, slots * N)
        again = launch(m, d, thr, want_inliers=i % 2 == 0)
        assert torch.equal(bufs[0].view(torch.uint8), again[0].view(torch.uint8)), "two launches differ in a bit"
        if bufs[2] is not None:
            assert torch.equal(bufs[2], again[2])
    print(f"N={N} {dtype}: worst |error| / tolerance {stats['ratio']:.3g}, excluded {stats['excl']} of {stats['inl']} inliers")


@pytest.mark.parametrize("N", G.PATTERN_N)
def test_validity_patterns(N):
    """all seven patterns on every launch path: the three wave variants (N = 64, 128, 256) and the block kernel"""
    cases = [c for c in G.gpu_cases() if c["pattern"] is not None and c["N"] == N]
    assert [c["pattern"] for c in cases] == list(R.VALID_PATTERNS)
    assert G.dispatch(3, 70, N)[0] == {64: "wave1", 128: "wave2", 256: "wave4"}.get(N, "block")
    for c in cases:
        mt, md, refs, valid = G.case_inputs(c)
        m, d, thr = inputs(mt, md, c["M"], c["P"], c["thr"], c["dtype"])
        n_ex, n_in, slots = check(launch(m, d, thr, valid=valid.to(DEV)), refs, c["P"], c["M"], valid=valid)
        caps(n_ex, n_in, slots * N)


@pytest.mark.parametrize("N", G.PATTERN_N)
def test_gated_pairs_keep_their_contents(N):
    """a closed gate on every launch path, with and without a validity tensor and counts"""
    P, M, _ = G.PATTERN_SHAPE
    mt, md, refs = G.sweep_inputs(N, torch.float32)
    m, d, thr = inputs(mt, md, M, P, R.THR, torch.float32)
    iters = torch.tensor([0, 500, 10], dtype=torch.int32, device=DEV)
    max_iters = torch.tensor([100.0, 500.0, 9.5], dtype=torch.float64, device=DEV)
    gated = torch.tensor([False, True, True])
    check(launch(m, d, thr, gate=(iters, max_iters)), refs, P, M, gated=gated)
    valid = R.valid_pattern("alternating", P, M)
    check(launch(m, d, thr, valid=valid.to(DEV), gate=(iters, max_iters), want_inliers=False), refs, P, M, valid=valid, gated=gated)
    open_all = torch.full((3,), 1e9, dtype=torch.float64, device=DEV)
    check(launch(m, d, thr, gate=(iters, open_all)), refs, P, M)


@pytest.mark.parametrize("thr,seed,mmax", [(R.THR_HUGE, 1000 + G.PROPS_SHAPE[2], G.MMAX), (R.THR_TINY, R.TINY_SEED, G.TINY_M)],
                         ids=["huge", "tiny"])
def test_extreme_thresholds(thr, seed, mmax):
    P, M, N = G.PROPS_SHAPE
    M = min(M, mmax)
    mt, md, refs = G.case_refs(3, N, seed, torch.float32, False, thr, mmax)
    m, d, t = inputs(mt, md, M, P, thr, torch.float32)
    bufs = launch(m, d, t)
    n_ex, n_in, slots = check(bufs, refs, P, M)
    caps(n_ex, n_in, slots * N)
    if thr == R.THR_HUGE:
        inl = bufs[2][bufs[3]:bufs[3] + P * M]
        assert (inl == N).all(), "a huge threshold: every point inside"


def test_scores_feed_ransac_update():
    """host-made models: ops.magsac_score then ops.ransac_update picks the oracle's arg-max where the top-two margin exceeds twice the
    tolerance (at most 10 % of the pairs may fall outside that rule)"""
    from differentiable_ransac_amd import ops
    P, M, N = G.K6_SHAPE
    mt, md, refs = G.case_refs(P, N, G.K6_SEED, torch.float32, True, R.THR, M)      # P distinct sets
    m, d, thr = inputs(mt, md, M, P, R.THR, torch.float32)
    scores, _ = ops.magsac_score(m, d, thr)
    st, thr_t = ops.ransac_init(P, N, 1000, R.THR, None, None, m.device, torch.float32)
    ops.ransac_update(st, m, d, None, scores, thr_t, M, 5)
    torch.cuda.synchronize()
    decided = 0
    for p in range(P):
        r = refs[p]
        sc = r["scores"][:M].clone()
        sc[r["nan"][:M]] = -float("inf")
        top = torch.argsort(sc, descending=True, stable=True)
        a, b = int(top[0]), int(top[1])
        tol = float(max(r["tol"][a], r["tol"][b]))
        assert abs(float(st.best_score[p]) - float(sc[a])) <= 2 * tol or float(sc[a] - sc[b]) <= 2 * tol
        if float(sc[a] - sc[b]) > 2 * tol:
            decided += 1
            assert torch.equal(st.best_model[p].cpu(), md[p][a]), f"pair {p}: not the oracle's arg-max"
            assert abs(float(st.best_score[p]) - float(sc[a])) <= tol
            assert int(st.best_inliers[p]) == int(st.best_mask[p].sum())
    assert decided >= 0.9 * P, f"only {decided} of {P} pairs decided by more than twice the tolerance"
