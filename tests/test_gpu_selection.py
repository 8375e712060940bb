"""The kernels that end every test-mode call, against the f64 restatement of tests/selection_ref.py: dr_ransac_update (arg-max,
better-test, best mask / inlier count, adaptive stop, the sub-batch walk), dr_select_best and dr_refit_accept, each through
its _f32 and _f64 entry.

Scores are set by hand, independently of the models, so that the winner is known exactly; the models are real (the
synthetic ground truth, perturbed), so that masks and inlier counts mean something.  Exact: winner, iteration counter,
best score and model (bit for bit), and the best mask against the dr_msac_score mask row of the same model (the same
arithmetic per (model, point) is claimed for both).  Against f64: the mask outside the rounding margin of
selection_ref.sampson, the adaptive bound to 1e-12, the refit candidates' scores within the bound of selection_ref.msac64."""
import math

import pytest
import torch

from differentiable_ransac_amd import synth
from oracle import cpu_ref as O
from tests import selection_ref as S

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
STATE = ("best_score", "best_model", "best_mask", "best_inliers", "iters", "max_iters")
# every dr_msac_score family: f32 short rows (<= 64, <= 128, <= 256), fast16 (N % 16 == 0), fast (N % 16 != 0); f64 kernel
POINTS = [1, 50, 100, 200, 256, 257, 512, 1000, 2000, 2050, 4096]
SENTINEL_MODEL = (torch.arange(9, dtype=torch.float64) * 0.25 + 0.5).reshape(3, 3)


def bits(t):
    t = t.contiguous().reshape(-1)
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


def problem(P, M, N, dt, seed, spread=(1e-4, 0.3)):
    """P synthetic pairs of N points, M models per pair (ground truth perturbed by a relative sigma log-uniform in `spread`),
    a threshold per pair (the normalised 0.75 px, times 0.5 .. 2 across the pairs) and scores uniform in [0, 100)"""
    d = synth.batch_two_view(P, N, seed0=seed, inlier_ratio=0.6)
    g = torch.Generator().manual_seed(seed)
    gt = d["gt_E"].double()
    lo, hi = math.log10(spread[0]), math.log10(spread[1])
    sig = 10 ** (lo + (hi - lo) * torch.rand(P, M, 1, 1, generator=g, dtype=torch.float64))
    models = (gt[:, None] * (1 + sig * torch.randn(P, M, 3, 3, generator=g, dtype=torch.float64))).to(dt)
    base = torch.tensor([float(O.normalized_threshold(0.75, d["K1"][p].double(), d["K2"][p].double(), False))
                         for p in range(P)], dtype=torch.float64)
    fac = torch.linspace(0.5, 2.0, P, dtype=torch.float64) if P > 1 else torch.ones(1, dtype=torch.float64)
    scores = (100 * torch.rand(P, M, generator=g, dtype=torch.float64)).to(dt)
    return dict(matches=d["matches"].to(dt), models=models, thr=(base * fac).to(dt), scores=scores, gt=gt.to(dt), g=g)


def device_masks(dev, pb, idx):
    """dr_msac_score mask rows [P,R,N] of the models at slots idx [P,R] (-1: any slot, unused)"""
    from differentiable_ransac_amd import ops
    P = idx.shape[0]
    sel = pb["models"][torch.arange(P)[:, None], idx.clamp_min(0)]
    _, masks = ops.msac_score(pb["matches"].to(dev), sel.to(dev), pb["thr"].to(dev))
    return masks.cpu()


def check_mask_f64(mask, pb, p, m):
    """the mask of slot m's model against f64 Sampson, outside the rounding margin (and the margin is not everything)"""
    q, rel = S.sampson(pb["matches"][p], pb["models"][p, m], pb["thr"][p], pb["matches"].dtype)
    sure = S.sure(q, rel)
    assert int(sure.sum()) >= 0.95 * q.numel(), (p, m, int(sure.sum()))
    assert torch.equal(mask[sure], S.mask64(q)[sure]), (p, m)


# ------------------------------------------------------------------------------------------------ dr_ransac_update
def run_update(dev, pb, B, k=5, conf=0.999, eps=1e-5, max_iterations=5000, sub_models=0, valid=None, iters=None,
               max_iters=None, best=None):
    """one dr_ransac_update launch from a sentinel state (mask of ones, non-identity model, odd inlier count), checked pair by
    pair against selection_ref.update.  Returns the restatement's result per pair."""
    from differentiable_ransac_amd import ops
    P, M = pb["scores"].shape
    N = pb["matches"].shape[1]
    dt = pb["matches"].dtype
    iters = torch.zeros(P, dtype=torch.int32) if iters is None else iters
    max_iters = torch.full((P,), float(max_iterations), dtype=torch.float64) if max_iters is None else max_iters
    best = torch.zeros(P, dtype=dt) if best is None else best
    st = ops.RansacState(P, N, max_iterations, dev, dt)
    st.best_score.copy_(best)
    st.best_model.copy_(SENTINEL_MODEL.to(dt).expand(P, 3, 3))
    st.best_mask.fill_(True)
    st.best_inliers.fill_(777)
    st.iters.copy_(iters)
    st.max_iters.copy_(max_iters)
    before = {key: getattr(st, key).cpu().clone() for key in STATE}
    md, thd = pb["matches"].to(dev), pb["thr"].to(dev)
    ops.ransac_update(st, md, pb["models"].to(dev), None if valid is None else valid.to(dev), pb["scores"].to(dev), thd, B, k,
                      conf, eps, sub_models=sub_models)
    torch.cuda.synchronize()
    after = {key: getattr(st, key).cpu() for key in STATE}
    vrow = (lambda p: None) if valid is None else (lambda p: valid[p])
    cands = torch.tensor([S.sub_batch_argmax(pb["scores"][p], vrow(p), sub_models) for p in range(P)])
    dmask = device_masks(dev, pb, cands)
    refs = []
    for p in range(P):
        row = {int(c): r for r, c in enumerate(cands[p].tolist()) if c >= 0}
        ref = S.update(pb["scores"][p], vrow(p), int(iters[p]), float(max_iters[p]), best[p], B, k, conf, eps, max_iterations,
                       sub_models, lambda m: int(dmask[p, row[m]].sum()), N)
        refs.append(ref)
        if int(iters[p]) >= float(max_iters[p]):
            # a pair that had stopped before the call: all six state tensors bit for bit
            for key in STATE:
                assert torch.equal(bits(after[key][p]) if after[key].is_floating_point() else after[key][p],
                                   bits(before[key][p]) if before[key].is_floating_point() else before[key][p]), (p, key)
            continue
        if ref["ambiguous"]:
            # a stop test met a computed bound within 1e-9 of the iteration count: f64 rounding of pow / log10 may decide it
            # either way, so this pair's stop decision is not checked
            continue
        assert int(after["iters"][p]) == ref["it"], (p, int(after["iters"][p]), ref)
        if ref["winner"] < 0:
            for key in ("best_score", "best_model", "best_mask", "best_inliers", "max_iters"):
                assert torch.equal(bits(after[key][p]) if after[key].is_floating_point() else after[key][p],
                                   bits(before[key][p]) if before[key].is_floating_point() else before[key][p]), (p, key)
            continue
        w = ref["winner"]
        assert same_bits(after["best_score"][p], pb["scores"][p, w]), (p, w, float(after["best_score"][p]))
        assert same_bits(after["best_model"][p], pb["models"][p, w]), (p, w)
        mk = after["best_mask"][p]
        assert torch.equal(mk, dmask[p, row[w]]), (p, w, int((mk != dmask[p, row[w]]).sum()))
        check_mask_f64(mk, pb, p, w)
        assert int(after["best_inliers"][p]) == int(mk.sum()), p
        want = S.bound(int(mk.sum()), N, k, conf, eps, max_iterations)
        assert abs(float(after["max_iters"][p]) - want) <= 1e-12 * max(1.0, want), (p, float(after["max_iters"][p]), want)
    return refs


def _mixed_state(P, dt):
    """pair 0: first batch; pair 1: stopped before the call; pair 2: 16 iterations, best 50; pair 3: best 99.9; the rest first batch"""
    iters = torch.zeros(P, dtype=torch.int32)
    max_iters = torch.full((P,), 5000.0, dtype=torch.float64)
    best = torch.zeros(P, dtype=dt)
    if P > 1:
        iters[1], max_iters[1], best[1] = 65, 40.5, 3.0
    if P > 2:
        iters[2], best[2] = 16, 50.0
    if P > 3:
        iters[3], best[3] = 16, 99.9
    return dict(iters=iters, max_iters=max_iters, best=best)


@pytest.mark.parametrize("N", POINTS)
@pytest.mark.parametrize("dt", DTYPES)
def test_update_point_counts(dev, dt, N):
    pb = problem(7, 65, N, dt, seed=1000 + N)
    valid = torch.rand(7, 65, generator=pb["g"]) < 0.7
    refs = run_update(dev, pb, B=65, valid=valid, **_mixed_state(7, dt))
    assert refs[0]["winner"] >= 0


@pytest.mark.parametrize("M", [1, 10, 63, 65, 10240])
@pytest.mark.parametrize("dt", DTYPES)
def test_update_model_counts(dev, dt, M):
    P = 2 if M == 10240 else 5
    pb = problem(P, M, 300, dt, seed=2000 + M)
    run_update(dev, pb, B=M, **_mixed_state(P, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_update_many_pairs(dev, dt):
    P = 300
    pb = problem(P, 10, 100, dt, seed=3000)
    valid = torch.rand(P, 10, generator=pb["g"]) < 0.8
    iters = torch.randint(0, 3, (P,), generator=pb["g"], dtype=torch.int32) * 10
    best = torch.where(iters > 0, torch.full((P,), 90.0), torch.zeros(P)).to(dt)
    refs = run_update(dev, pb, B=10, valid=valid, iters=iters, best=best)
    assert sum(r["winner"] >= 0 for r in refs) > P // 2


# equal maxima (lower index, higher index) inside one sub-batch, the lower one where the kernel's scan meets it later or in
# another thread: same lane of the 4-way unroll (stride 4 step, step = 64 x waves per sub-batch) and of the next unroll slot,
# lanes of one wave, different waves (>= 64), beyond one block pass (>= 1024)
TIES = [(10, 10 + 4 * 1024), (10, 10 + 1024), (3, 40), (62, 65), (1000, 1030), (63, 64 + 1024), (5, 9000), (3000, 4097),
        (10, 10 + 4 * 256), (200, 300), (0, 19), (3, 17)]


@pytest.mark.parametrize("sub_models", [0, 2560, 20])
@pytest.mark.parametrize("dt", DTYPES)
def test_update_ties_take_the_first_index(dev, dt, sub_models):
    M = 10240
    msub = sub_models or M
    R = M // msub
    ties = [(a, b) for a, b in TIES if b < msub]
    P = len(ties) + 1
    # badly perturbed models: few inliers, the bound stays at max_iterations and the whole walk runs (B = 1)
    pb = problem(P, M, 200, dt, seed=4000 + sub_models, spread=(0.05, 0.3))
    for p, (a, b) in enumerate(ties):
        j = (p % R) if R > 1 else 0            # the tied sub-batch: first, last, and in between
        pb["scores"][p, j * msub + a] = 1000.0
        pb["scores"][p, j * msub + b] = 1000.0
    # a tie across sub-batches: the later one equals the best and must not replace it
    last = P - 1
    pb["scores"][last, 7] = 1000.0
    pb["scores"][last, min(M - 1, msub + 7)] = 1000.0
    refs = run_update(dev, pb, B=1, sub_models=sub_models)
    for p, (a, b) in enumerate(ties):
        j = (p % R) if R > 1 else 0
        assert refs[p]["winner"] == j * msub + a and refs[p]["walked"] == R, (p, refs[p])
    assert refs[last]["winner"] == 7


@pytest.mark.parametrize("sub_models", [0, 40])
@pytest.mark.parametrize("dt", DTYPES)
def test_update_scores_that_must_not_win(dev, dt, sub_models):
    P, M = 10, 120
    pb = problem(P, M, 256, dt, seed=5000 + sub_models)
    g = pb["g"]
    sc = pb["scores"]
    valid = torch.rand(P, M, generator=g) < 0.7
    valid[:, 50] = True
    iters = torch.zeros(P, dtype=torch.int32)
    best = torch.zeros(P, dtype=dt)
    sc[0, 30] = float("nan"); valid[0, 30] = True; sc[0, 50] = 500.0            # NaN where the maximum would be
    sc[1, 31] = 1e6; valid[1, 31] = False; sc[1, 50] = 500.0                    # the largest score in an invalid slot
    valid[2] = False                                                             # nothing valid
    sc[3] = float("nan")                                                         # everything NaN
    iters[4] = 16                                                                # a score equal to the best ...
    best[4] = sc[4][valid[4]].max()
    best[5] = sc[5][valid[5]].max()                                              # ... is taken on the first batch only
    sc[6] = 0.0                                                                  # first batch, all scores 0: still taken
    iters[7], best[7] = 16, 1e5                                                  # nothing better
    valid[8, :40] = False                                                        # first sub-batch empty; the next one is
    sc[9, 40:] = 0.0                                                             # later sub-batches of zeros
    refs = run_update(dev, pb, B=8, valid=valid, iters=iters, best=best, sub_models=sub_models)
    R = 3 if sub_models else 1
    assert refs[0]["winner"] == 50 and refs[1]["winner"] == 50
    assert refs[2]["winner"] == -1 and refs[3]["winner"] == -1
    assert refs[4]["winner"] == -1
    assert refs[5]["winner"] >= 0
    assert refs[6]["winner"] == int(torch.nonzero(valid[6])[0, 0])
    assert refs[7]["winner"] == -1
    assert (refs[8]["winner"] >= 40) if sub_models else (refs[8]["winner"] >= 0)
    assert refs[2]["it"] == 8 * R and refs[3]["it"] == 8 * R


R_SUBS = {2: 5120, 3: 3414, 5: 2048, 15: 683, 16: 640, 17: 603, 64: 160, 512: 20}


@pytest.mark.parametrize("sub_models", [0, 10240, 10245] + list(R_SUBS.values()))
@pytest.mark.parametrize("dt", DTYPES)
def test_update_sub_batch_walk(dev, dt, sub_models):
    M = 10240
    R = -(-M // sub_models) if 0 < sub_models < M else 1
    assert R == 1 or R_SUBS[R] == sub_models
    pb = problem(3, M, 300, dt, seed=6000 + sub_models)
    # pair 0: a winner early in the walk, the ground truth itself: ~60 % inliers, bound ~85 iterations, so the walk (16 per
    # sub-batch) ends after ~6 sub-batches
    pb["models"][0, 5] = pb["gt"][0]
    pb["thr"][0] *= 4
    pb["scores"][0, 5] = 1000.0
    st = dict(iters=torch.tensor([0, 32, 48], dtype=torch.int32), max_iters=torch.tensor([5000.0, 5000.0, 47.5], dtype=torch.float64),
              best=torch.tensor([0.0, 99.0, 1.0], dtype=dt))
    refs = run_update(dev, pb, B=16, sub_models=sub_models, **st)
    assert refs[0]["winner"] == 5
    if R >= 15:
        assert refs[0]["walked"] < R, refs[0]


@pytest.mark.parametrize("dt", DTYPES)
def test_update_refuses_513_sub_batches(dev, dt):
    from differentiable_ransac_amd import _lib as L
    from differentiable_ransac_amd import ops
    pb = problem(1, 513, 64, dt, seed=6500)
    st = ops.RansacState(1, 64, 5000, dev, dt)
    with pytest.raises(L.DransacError):
        ops.ransac_update(st, pb["matches"].to(dev), pb["models"].to(dev), None, pb["scores"].to(dev), pb["thr"].to(dev), 1, 5,
                          sub_models=1)


@pytest.mark.parametrize("eps", [1e-5, 0.0])
@pytest.mark.parametrize("conf", [0.99, 0.999])
@pytest.mark.parametrize("k", [3, 5, 7, 8])
@pytest.mark.parametrize("dt", DTYPES)
def test_update_adaptive_bound_edges(dev, dt, k, conf, eps):
    P, M, B, max_iterations = 6, 48, 48, 1000     # (max_iterations not a multiple of B)
    pb = problem(P, M, 200, dt, seed=7000 + k)
    pb["thr"][0] = 1e-12                              # no inlier: the bound is max_iterations
    pb["thr"][2] = 1e-12
    pb["thr"][1] = 100.0                              # every point an inlier: bound 0.6, the pair stops after this sub-batch
    iters = torch.tensor([0, 0, 960, 0, 0, 0], dtype=torch.int32)
    max_iters = torch.full((P,), float(max_iterations), dtype=torch.float64)
    if eps == 0.0:
        # (with every point an inlier the reference's math.log10(0) raises: that pair is left out, as stopped)
        iters[1], max_iters[1] = 10, 5.0
    refs = run_update(dev, pb, B=B, k=k, conf=conf, eps=eps, max_iterations=max_iterations, sub_models=16, iters=iters,
                      max_iters=max_iters)
    assert refs[0]["max_it"] == max_iterations and refs[0]["it"] == 3 * B
    assert refs[2]["it"] == 1008                      # 960 < 1000 walks one sub-batch, 1008 stops
    if eps:
        # ratio 1: log10(1 - confidence) / log10(eps), 0.6 or 0.4
        assert abs(refs[1]["max_it"] - math.log10(1 - conf) / math.log10(eps)) < 1e-12
        assert refs[1]["it"] == B and refs[1]["walked"] == 1


# ------------------------------------------------------------------------------------------------ dr_select_best
def check_select(dev, pb, valid):
    from differentiable_ransac_amd import ops
    P, M = pb["scores"].shape
    N = pb["matches"].shape[1]
    dt = pb["matches"].dtype
    out = ops.select_best(pb["matches"].to(dev), pb["models"].to(dev), pb["scores"].to(dev), pb["thr"].to(dev),
                          valid=None if valid is None else valid.to(dev))
    idx, sc, mo, mk, inl = (t.cpu() for t in out)
    want = torch.tensor([S.first_argmax(pb["scores"][p], None if valid is None else valid[p])[0] for p in range(P)])
    assert torch.equal(idx.long(), want)
    dmask = device_masks(dev, pb, want[:, None])
    for p in range(P):
        w = int(want[p])
        if w < 0:
            assert float(sc[p]) == 0.0 and torch.equal(mo[p], torch.eye(3, dtype=dt)), p
            assert not bool(mk[p].any()) and int(inl[p]) == 0, p
            continue
        assert same_bits(sc[p], pb["scores"][p, w]) and same_bits(mo[p], pb["models"][p, w]), p
        assert torch.equal(mk[p], dmask[p, 0]), (p, int((mk[p] != dmask[p, 0]).sum()))
        check_mask_f64(mk[p], pb, p, w)
        assert int(inl[p]) == int(mk[p].sum()), p
    return want


def _select_specials(pb, valid):
    sc = pb["scores"]
    M = sc.shape[1]
    valid[0] = False                                   # nothing valid: -1, score 0, eye(3), empty mask, no inliers
    sc[1] = float("nan")                               # everything NaN: the same
    if M > 300:
        sc[2, 300] = sc[2, 44] = 1000.0                 # one thread, two passes
        sc[3, 256] = sc[3, 255] = 1000.0                # thread 0 and thread 255
        valid[3, 255] = valid[3, 256] = True
        valid[2, 44] = valid[2, 300] = True
    if M > 64:
        sc[5, 64] = sc[5, 3] = 1000.0                   # different waves
        valid[5, 3] = valid[5, 64] = True
    if M > 5:
        sc[4, 3] = float("nan"); valid[4, 3] = True     # NaN where the maximum would be ...
        sc[4, 1] = 1e6; valid[4, 1] = False             # ... and the largest score in an invalid slot
        sc[4, 5] = 500.0; valid[4, 5] = True


@pytest.mark.parametrize("valid_null", [False, True])
@pytest.mark.parametrize("N", POINTS)
@pytest.mark.parametrize("dt", DTYPES)
def test_select_best_point_counts(dev, dt, N, valid_null):
    pb = problem(7, 65, N, dt, seed=8000 + N)
    valid = torch.rand(7, 65, generator=pb["g"]) < 0.7
    _select_specials(pb, valid)
    want = check_select(dev, pb, None if valid_null else valid)
    if not valid_null:
        assert want[0] == -1 and want[4] == 5
    assert want[1] == -1 and want[5] == 3


@pytest.mark.parametrize("P,M", [(1, 1), (7, 10), (300, 10), (6, 10240), (5, 63)])
@pytest.mark.parametrize("dt", DTYPES)
def test_select_best_shapes(dev, dt, P, M):
    pb = problem(P, M, 257, dt, seed=9000 + P + M)
    valid = torch.rand(P, M, generator=pb["g"]) < 0.8
    valid[:, 0] = True
    if P >= 6:
        _select_specials(pb, valid)
    if M > 5000:
        pb["scores"][5, 5000] = pb["scores"][5, 1] = 1000.0
        valid[5, 1] = valid[5, 5000] = True
    want = check_select(dev, pb, valid)
    if M > 5000:
        assert want[2] == 44 and want[3] == 255 and want[5] == 1


# ------------------------------------------------------------------------------------------------ dr_refit_accept
def _candidates(pb, P, Sn, dt):
    """candidate 0 near the ground truth; the last one (S >= 2) twice candidate 0 -- the same Sampson distances, an exact tie
    at a later index; in between (and, for S = 1, at odd pairs) NaN, inf and all-zero candidates, and perturbed ones"""
    g = pb["g"]
    gt = pb["gt"].double()
    cand = gt[:, None] * (1 + 0.05 * torch.randn(P, Sn, 3, 3, generator=g, dtype=torch.float64))
    cand[:, 0] = gt * (1 + 1e-4 * torch.randn(P, 3, 3, generator=g, dtype=torch.float64))
    cand = cand.to(dt)
    if Sn >= 2:
        cand[:, Sn - 1] = 2 * cand[:, 0]
    for p in range(P):
        slots = range(1, Sn - 1) if Sn >= 2 else ([0] if p % 2 else [])
        for c in slots:
            kind = (c + p) % 4
            if kind == 0:
                cand[p, c, 1, 2] = float("nan")
            elif kind == 1:
                cand[p, c, 2, 2] = float("inf")
            elif kind == 2:
                cand[p, c] = 0.0
    return cand


def _accept(dev, pb, cand, cv, best, model):
    from differentiable_ransac_amd import ops
    bs, bm = best.to(dev).clone(), model.to(dev).clone()
    ops.refit_accept(pb["matches"].to(dev), cand.to(dev), None if cv is None else cv.to(dev), pb["thr"].to(dev), bs, bm)
    torch.cuda.synchronize()
    return bs.cpu(), bm.cpu()


@pytest.mark.parametrize("cv_mixed", [False, True])
@pytest.mark.parametrize("N", [8, 255, 2000, 5000])
@pytest.mark.parametrize("Sn", [1, 4, 10])
@pytest.mark.parametrize("dt", DTYPES)
def test_refit_accept(dev, dt, Sn, N, cv_mixed):
    P = 8
    pb = problem(P, 1, N, dt, seed=10000 + 10 * N + Sn)
    cand = _candidates(pb, P, Sn, dt)
    cv = None
    if cv_mixed:
        cv = torch.rand(P, Sn, generator=pb["g"]) < 0.6
        cv[:, 0] = True
        cv[:, Sn - 1] = True
    sentinel = SENTINEL_MODEL.to(dt).expand(P, 3, 3).contiguous()
    # every candidate on its own, from best_score = -1: the kernel's own score (or no replacement)
    ksc = [[None] * Sn for _ in range(P)]
    for c in range(Sn):
        bs, bm = _accept(dev, pb, cand[:, c:c + 1], None if cv is None else cv[:, c:c + 1], torch.full((P,), -1.0, dtype=dt),
                         sentinel)
        for p in range(P):
            m = cand[p, c]
            competes = (cv is None or bool(cv[p, c])) and bool(torch.isfinite(m).all()) and bool((m != 0).any())
            if not competes:
                assert float(bs[p]) == -1.0 and same_bits(bm[p], sentinel[p]), (p, c)
                continue
            assert float(bs[p]) >= 0.0 and same_bits(bm[p], m), (p, c)
            ksc[p][c] = bs[p]
            q, rel = S.sampson(pb["matches"][p], m, pb["thr"][p], dt)
            want, tol = S.msac64(q, rel, dt, N)
            assert abs(float(bs[p]) - want) <= tol, (p, c, float(bs[p]), want, tol)
    # the duplicate scores exactly as its original
    if Sn >= 2:
        for p in range(P):
            assert same_bits(ksc[p][0], ksc[p][Sn - 1]), (p, float(ksc[p][0]), float(ksc[p][Sn - 1]))
    # all candidates at once, against a best score below all of them, above, EQUAL to the top (kept: strict) and one ulp below
    # the top (replaced)
    best = torch.empty(P, dtype=dt)
    for p in range(P):
        top = max((float(s) for s in ksc[p] if s is not None), default=5.0)
        topt = torch.tensor(top, dtype=dt)
        best[p] = [torch.tensor(-1.0, dtype=dt), topt + 1e3, topt, torch.nextafter(topt, torch.tensor(-math.inf, dtype=dt))][p % 4]
    bs, bm = _accept(dev, pb, cand, cv, best, sentinel)
    for p in range(P):
        w = S.refit_accept([None if s is None else float(s) for s in ksc[p]], [s is not None for s in ksc[p]], float(best[p]))
        competes = any(s is not None for s in ksc[p])
        assert (w >= 0) == (competes and p % 4 in (0, 3)), (p, w)
        if w < 0:
            assert same_bits(bs[p], best[p]) and same_bits(bm[p], sentinel[p]), p
        else:
            assert w == 0, (p, w)                      # the near-exact candidate, the first of the two equal maxima
            assert same_bits(bs[p], ksc[p][w]) and same_bits(bm[p], cand[p, w]), p
