"""dr_homography_magsac_score, dr_homography_irls and BatchedHomography(scoring="magsac") against the f64 oracle
tests/homography_magsac_ref.py, in f32 and f64.

Score shapes: N = 4 (fewer than a lane's 8 points), 257 (one past the 256-lane stride), 2049 (one past the 2048-point chunk); M = 1, 17,
33 (a partial 16-slot tile, one tile plus one, two tiles plus one).  IRLS shapes: four pairs of N = 4, 257, 2049.  Every tolerance is
the oracle module's (derived there, never from a kernel's output); the conditions a comparison rests on -- the share of cells in the
guard band, decision margins above the tolerance, no row of a polish step in the band -- are asserted on the oracle's side first
(tests/test_homography_magsac_host.py holds the oracle alone to them on these inputs).  Every test prints its worst err / tol."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import homography_magsac_ref as MR
from tests import homography_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
NAME = {torch.float32: "float32", torch.float64: "float64"}
THR = R.THRESHOLD
F32_STEPS = 5


def _bytes(t):
    return t.contiguous().view(torch.uint8)


# ------------------------------------------------------------------------------------------------ dr_homography_magsac_score
@functools.lru_cache(maxsize=None)
def _score_case(N, M, name):
    m, models, valid = MR.score_case(N, M, name)
    inband, cells = MR.band_share(m, models, valid, THR, name)
    return m, models, valid, inband, cells


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MR.SCORE_M)
@pytest.mark.parametrize("N", MR.SCORE_N)
def test_score_against_oracle(dev, dt, N, M):
    from differentiable_ransac_amd import ops
    name = NAME[dt]
    m, models, valid, inband, cells = _score_case(N, M, name)
    assert cells > 0 and inband <= R.BAND_SHARE_MAX * cells           # the condition on the input
    P = len(m)
    args = (torch.from_numpy(m).to(dev, dt), torch.from_numpy(models).to(dev, dt), THR, torch.from_numpy(valid).to(dev))
    scores, inl = ops.homography_magsac_score(*args)
    s_only, none = ops.homography_magsac_score(*args, want_inliers=False)
    assert none is None and torch.equal(_bytes(s_only), _bytes(scores))
    sk, ik = scores.double().cpu().numpy(), inl.cpu().numpy()
    worst, top = 0.0, 0.0
    for p in range(P):
        for j in range(M):
            if not valid[p, j]:
                assert sk[p, j] == 0.0 and ik[p, j] == 0, (p, j)
                continue
            so, io = MR.magsac(m[p], models[p, j], THR)
            tol = MR.score_tolerance(m[p], models[p, j], THR, name)
            nb = int(R.in_band(R.ratio2(models[p, j], m[p], THR), name).sum())
            assert abs(sk[p, j] - so) <= tol, (p, j, sk[p, j], so, tol)
            assert abs(int(ik[p, j]) - io) <= nb, (p, j, ik[p, j], io, nb)     # equal, except for the cell's points inside the band
            worst, top = max(worst, abs(sk[p, j] - so) / tol), max(top, so)
    print(f"magsac score {name} N={N} M={M}: worst err/tol {worst:.3g}, band cells {inband}/{cells}, best score {top:.4f}")


@pytest.mark.parametrize("dt", DTYPES)
def test_score_edge_rows(dev, dt):
    """one pair, four points, five slots.  H_p has the vanishing line x = 320: point 0 (x = 100) is transferred exactly and lies in
    front, point 1 (x = 500) is transferred exactly and lies behind the camera, point 2 is far off, point 3 is a fixed point of the
    identity (d2 = 0 exactly there) and far off under H_p.  Slots: H_p, a NaN entry, a rank-one matrix of integers (det = 0 exactly),
    H_p flagged invalid, the identity."""
    from differentiable_ransac_amd import ops
    name = NAME[dt]
    Hp = R.canonical(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0 / 320.0, 0.0, 1.0]]))
    x1 = np.array([[100.0, 50.0], [500.0, 80.0], [10.0, 10.0], [200.0, 300.0]])
    y = np.concatenate([x1, np.ones((4, 1))], 1) @ Hp.T
    x2 = y[:, :2] / y[:, 2:]
    x2[2], x2[3] = (600.0, 600.0), x1[3]
    m = MR.rounded(np.concatenate([x1, x2], 1), name)
    nan = Hp.copy()
    nan[1, 1] = np.nan
    models = MR.rounded(np.stack([Hp, nan, np.outer([1.0, 2.0, 3.0], [1.0, -1.0, 2.0]), Hp, np.eye(3)]), name)
    valid = np.array([True, True, True, False, True])
    args = (torch.from_numpy(m[None]).to(dev, dt), torch.from_numpy(models[None]).to(dev, dt), THR, torch.from_numpy(valid[None]).to(dev))
    scores, inl = ops.homography_magsac_score(*args)
    again, inl2 = ops.homography_magsac_score(*args)
    assert torch.equal(_bytes(scores), _bytes(again)) and torch.equal(inl, inl2)          # two launches, the same bytes
    s, n = scores[0].double().cpu().numpy(), inl[0].cpu().numpy()
    print(f"edge rows {name}: scores {s.tolist()}, inliers {n.tolist()}")
    so, io = MR.magsac(m, models[0], THR)
    assert io == 1 and abs(so - 1.0) < 1e-6                         # the oracle: point 0 alone, the point behind the camera adds nothing
    assert abs(s[0] - so) <= MR.score_tolerance(m, models[0], THR, name) and n[0] == 1
    assert math.isnan(s[1]) and n[1] == 0 and math.isnan(s[2]) and n[2] == 0
    assert s[3] == 0.0 and n[3] == 0
    assert MR.magsac(m, models[4], THR) == (1.0, 1)                  # the point at d2 = 0 adds 1
    assert abs(s[4] - 1.0) <= MR.score_tolerance(m, models[4], THR, name) and n[4] == 1


# ------------------------------------------------------------------------------------------------ dr_homography_irls
@functools.lru_cache(maxsize=None)
def _irls_case(N, name, iters, claimed=None):
    return MR.irls_case(N, name, iters, claimed)


def _run_irls(dev, dt, N, iters, claimed=None):
    """-> (state after the launch, fits, the oracle's per-pair results, start models, start scores); the fields the kernel must leave
    alone are filled with noise and compared bytewise"""
    from differentiable_ransac_amd import ops
    m, start, score, oracle = _irls_case(N, NAME[dt], iters, claimed)
    st = ops.HomographyState(4, N, 1000, dev, dt)
    rng = np.random.default_rng(1)
    st.best_model.copy_(torch.from_numpy(start))
    st.best_score.copy_(torch.from_numpy(score))
    st.best_mask.copy_(torch.from_numpy(rng.uniform(size=(4, N)) < 0.5))
    st.best_inliers.copy_(torch.from_numpy(rng.integers(0, N, 4)))
    st.iters.copy_(torch.from_numpy(rng.integers(0, 900, 4)))
    st.max_iters.copy_(torch.from_numpy(rng.uniform(1.0, 1000.0, 4)))
    keep = {k: getattr(st, k).clone() for k in ("best_mask", "best_inliers", "iters", "max_iters")}
    tm = torch.from_numpy(m).to(dev, dt)
    fits = torch.full((4,), 7, device=dev, dtype=torch.int32)          # (added to)
    ops.homography_irls(st, tm, ops.thr2_tensor(THR, 4, tm), iters, fits)
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(_bytes(getattr(st, k)), _bytes(v)), k
    return st, fits.cpu().numpy() - 7, oracle, start, score


def _compare_irls(what, st, fits, oracle, start, score, dt):
    """a pair that meets homography_magsac_ref.irls_clear: equal fits; the state untouched bit for bit where no candidate was taken,
    else score and model within their bounds.  Any other pair is left out.  -> (pairs left out, pairs that took a candidate)"""
    name = NAME[dt]
    skipped, took, worst_s, worst_m = 0, 0, 0.0, 0.0
    for p, o in enumerate(oracle):
        final = float(st.best_score[p])
        got = st.best_model[p].cpu().double().numpy()
        print(f"{what} pair {p}: fits {fits[p]} (oracle {o['fits']}), score {score[p]:.9g} -> {final:.9g} (oracle {o['score']:.9g}), margins "
              f"{[f'{g:.3g}' for g in o['margins']]}, tolerance {o['tol']:.3g}")
        assert final >= score[p], p      # exact: a candidate is taken on a strictly higher score only
        if not MR.irls_clear(o, name):
            skipped += 1
            continue
        assert fits[p] == o["fits"], p
        if not any(g > 0 for g in o["margins"]):
            assert np.array_equal(got, start[p], equal_nan=True) and final == score[p], p
            continue
        took += 1
        assert abs(final - o["score"]) <= o["tol"], (p, final, o["score"], o["tol"])
        worst_s = max(worst_s, abs(final - o["score"]) / o["tol"])
        last = [t for t, g in zip(o["trace"], o["margins"]) if g > 0][-1]
        err, mtol = np.abs(got - o["model"]).max(), R.refit_tolerance(last["sv"], name)
        worst_m = max(worst_m, err / mtol)
        assert err <= mtol, (p, err, mtol)
        assert abs(np.linalg.norm(got) - 1.0) <= 4 * R.eps_of(name) and np.linalg.det(got) > 0
    print(f"{what}: pairs left out {skipped}/4, pairs that took a candidate {took}, worst score err/tol {worst_s:.3g}, worst model "
          f"err/tol {worst_m:.3g}")
    return skipped, took


@pytest.mark.parametrize("N", MR.IRLS_N)
def test_irls_against_oracle_f64(dev, N):
    """IRLS_STEPS[N] steps (one at N = 4, where the first fit is exact and a second gains exactly 0; five otherwise).  Every margin of
    the oracle exceeds the f64 tolerance and no row lies in the band (asserted: no pair is left out)"""
    dt, iters = torch.float64, MR.IRLS_STEPS[N]
    st, fits, oracle, start, score = _run_irls(dev, dt, N, iters)
    skipped, took = _compare_irls(f"irls f64 N={N}", st, fits, oracle, start, score, dt)
    assert skipped == 0 and took == 2                                # the condition on the input
    assert fits.tolist() == [iters, iters, 0, 0]


@pytest.mark.parametrize("N", MR.IRLS_N)
def test_irls_f32_one_step(dev, N):
    """ONE step: the first fit of a perturbed start gains 2 to 400 against an f32 score tolerance of 0.006 to 1.4, so the pairs that take
    a candidate are compared with the oracle -- fits, score and model.  The row decision and the weights are f64 in the kernel, so the
    model bound is the refit's own (eps32 for the output rounding + the f64 term).  At most one pair in four may be left out."""
    dt = torch.float32
    st, fits, oracle, start, score = _run_irls(dev, dt, N, 1)
    skipped, took = _compare_irls(f"irls f32 N={N} one step", st, fits, oracle, start, score, dt)
    assert skipped <= 1 and took >= 1
    assert fits[2] == 0 and fits[3] == 0


@pytest.mark.parametrize("N", MR.IRLS_N)
def test_irls_f32_several_steps_never_lower_the_score(dev, N):
    """the later fits gain less than the f32 tolerance, so only what holds exactly is asserted: the score is not below the one-step
    result, the models stay finite, 0 <= fits <= iters (the other state fields are compared bytewise in _run_irls)"""
    dt = torch.float32
    one, _, _, _, _ = _run_irls(dev, dt, N, 1)
    st, fits, oracle, start, score = _run_irls(dev, dt, N, F32_STEPS)
    for p in range(4):
        print(f"irls f32 N={N} pair {p}: fits {fits[p]}, score {score[p]:.6g} -> {float(one.best_score[p]):.6g} (one step) -> "
              f"{float(st.best_score[p]):.6g} (oracle after {F32_STEPS}: {oracle[p]['score']:.6g})")
        assert float(st.best_score[p]) >= float(one.best_score[p]) >= score[p], p
        assert 0 <= fits[p] <= F32_STEPS
        assert p == 3 or np.isfinite(st.best_model[p].cpu().numpy()).all()
    assert fits[0] >= 1 and fits[1] >= 1 and fits[2] == 0 and fits[3] == 0
    # a repeated launch from the same state gives the same bits
    again, fits2, _, _, _ = _run_irls(dev, dt, N, F32_STEPS)
    assert torch.equal(_bytes(again.best_model), _bytes(st.best_model)) and torch.equal(_bytes(again.best_score), _bytes(st.best_score))
    assert np.array_equal(fits, fits2)


@pytest.mark.parametrize("dt", DTYPES)
def test_irls_losing_candidate_leaves_the_state(dev, dt):
    """pairs 0 and 1 claim a best_score no fit reaches (1e6, and N: a score is below the number of points): one fit each, which loses by
    more than any tolerance; model and score stay as they were, bit for bit"""
    N = 257
    st, fits, oracle, start, score = _run_irls(dev, dt, N, 4, claimed=(1e6, float(N)))
    skipped, took = _compare_irls(f"irls {NAME[dt]} losing candidate", st, fits, oracle, start, score, dt)
    assert skipped == 0 and took == 0 and fits.tolist() == [1, 1, 0, 0]
    assert torch.equal(st.best_score.cpu().double(), torch.from_numpy(score))
    assert np.array_equal(st.best_model.cpu().double().numpy(), start, equal_nan=True)


# ------------------------------------------------------------------------------------------------ BatchedHomography
DRV = MR.DRV
KEYS = ("model", "mask", "score", "inliers", "iterations", "irls_fits")


@functools.lru_cache(maxsize=None)
def _driver_inputs():
    from differentiable_ransac_amd import synth
    rounds = math.ceil(DRV["max_iterations"] / DRV["B"])
    sc = MR.driver_scenes()
    noise = [synth.gumbel_noise((DRV["P"], DRV["B"], DRV["N"]), seed=1000 + r, dtype=torch.float64) for r in range(rounds)]
    return sc, np.stack([s["matches"] for s in sc]), noise


def _driver(**kw):
    from differentiable_ransac_amd.ransac import BatchedHomography
    return BatchedHomography(ransac_batch_size=DRV["B"], threshold=THR, max_iterations=DRV["max_iterations"], **kw)


def test_driver_against_oracle(dev):
    """f64, explicit noise, irls_iters = 3.  The oracle's loop runs on the models the solver kernel returned for the pinned index sets
    (the validity flags equal the closed form's; the solver's models are test_gpu_homography.py's subject), so that a last-bit
    difference of a model is not a score difference.  The condition on the input: every round's decision margin and every IRLS margin
    exceeds the tolerance."""
    from differentiable_ransac_amd import ops
    P, N, B = DRV["P"], DRV["N"], DRV["B"]
    sc, m, noise = _driver_inputs()
    dt, name = torch.float64, "float64"
    tm = torch.from_numpy(m).to(dev)
    logits = torch.zeros(P, N, device=dev, dtype=dt)
    g = [x.to(dev) for x in noise]
    out = {k: v.cpu() for k, v in _driver(scoring="magsac", irls_iters=DRV["irls_iters"])(tm, logits, gumbels=g).items()}
    assert set(out) == set(KEYS) and out["irls_fits"].dtype == torch.int32 and out["irls_fits"].shape == (P,)
    idx = [ops.gumbel_topk(logits, B, 4, 1.0, x, 0, soft=False)["idx"] for x in g]
    kern = [ops.homography4_gather(tm, i) for i in idx]
    idx = [i.cpu().numpy() for i in idx]
    for p in range(P):
        hyp = []
        for r, i in enumerate(idx):
            _, va, co = R.hypotheses(m[p], i[p])
            mk, vk = kern[r][0][p].cpu().numpy(), kern[r][1][p].cpu().numpy()
            assert np.array_equal(vk, va), (p, r)
            hyp.append((mk, va, co))
        o = MR.run(m[p], [i[p] for i in idx], THR, max_iterations=DRV["max_iterations"], irls_iters=DRV["irls_iters"], dtype_name=name,
                   hyp_per_round=hyp)
        tol = max(o["tols"] + [MR.score_tolerance(m[p], t["cand"], THR, name) for t in o["irls_trace"] if t["cand"] is not None])
        margin = min(o["gaps"] + [abs(x) for x in o["irls_margins"]])
        band = R.in_band(o["ratio2"], name)
        print(f"magsac driver pair {p}: rounds {o['rounds']}, iterations {o['iterations']}, inliers {o['inliers']}, score {o['score']:.6f} "
              f"(kernel {float(out['score'][p]):.6f}), irls fits {o['irls_fits']} margins {[f'{x:.3g}' for x in o['irls_margins']]}, "
              f"smallest margin {margin:.3g} vs tolerance {tol:.3g}")
        assert margin > tol, (p, margin, tol)                       # the conditions on the input
        assert not any(R.in_band(t["ratio2"], name).any() for t in o["irls_trace"]), p
        assert int(out["iterations"][p]) == o["iterations"] and int(out["inliers"][p]) == o["inliers"], p
        assert int(out["irls_fits"][p]) == o["irls_fits"], p
        assert np.array_equal(out["mask"][p].numpy()[~band], o["mask"][~band]), p
        assert abs(float(out["score"][p]) - o["score"]) <= tol, p
        taken = [t for t, x in zip(o["irls_trace"], o["irls_margins"]) if x > 0]
        got = out["model"][p].numpy()
        if taken:
            err, mtol = np.abs(got - o["model"]).max(), R.refit_tolerance(taken[-1]["sv"], name)
        else:
            err, mtol = np.abs(got - o["model"]).max(), 0.0        # the RANSAC winner itself: the solver's model, bit for bit
        print(f"   score err/tol {abs(float(out['score'][p]) - o['score']) / tol:.3g}, model err {err:.3g} tolerance {mtol:.3g}, mean transfer "
              f"error on the true inliers {R.mean_transfer_error(got, m[p], sc[p]['inlier']):.4f}")
        assert err <= mtol, (p, err, mtol)


@pytest.mark.parametrize("dt", DTYPES)
def test_driver_msac_default_and_no_polish(dev, dt):
    P, N = DRV["P"], DRV["N"]
    _, m, noise = _driver_inputs()
    tm = torch.from_numpy(m).to(dev, dt)
    logits = torch.zeros(P, N, device=dev, dtype=dt)
    g = [x.to(dev, dt) for x in noise]
    # scoring="msac" is the default path, bit for bit and key for key
    a, b = _driver()(tm, logits, gumbels=g), _driver(scoring="msac")(tm, logits, gumbels=g)
    assert set(a) == set(b) == {"model", "mask", "score", "inliers", "iterations"}
    assert all(torch.equal(_bytes(a[k]), _bytes(b[k])) for k in a)
    # no polish: the RANSAC winner, no fit counted
    host = _driver(scoring="magsac")(tm, logits, gumbels=g)
    assert set(host) == set(KEYS)
    plain = _driver(scoring="magsac", irls_iters=0)(tm, logits, gumbels=g)
    norefit = _driver(scoring="magsac", refit=False)(tm, logits, gumbels=g)
    for o in (plain, norefit):
        assert int(o["irls_fits"].sum()) == 0 and torch.equal(o["mask"], host["mask"]) and bool((o["score"] <= host["score"]).all())
    print(f"magsac driver {NAME[dt]}: iterations {host['iterations'].cpu().tolist()}, fits {host['irls_fits'].cpu().tolist()}, score "
          f"{plain['score'].cpu().tolist()} -> {host['score'].cpu().tolist()}")
    assert int(host["irls_fits"].sum()) >= 1 and bool((host["irls_fits"] <= 10).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_driver_prosac_with_magsac(dev, dt):
    P, N = DRV["P"], DRV["N"]
    sc, m, _ = _driver_inputs()
    tm = torch.from_numpy(m).to(dev, dt)
    logits = torch.from_numpy(np.stack([np.where(s["inlier"], 1.0, -1.0) for s in sc])).to(dev, torch.float32)
    logits = logits + 1e-3 * torch.rand(P, N, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    out = _driver(scoring="magsac", sampling="prosac", seed=2)(tm, logits)
    assert set(out) == set(KEYS)
    model = out["model"].cpu().double().numpy()
    print(f"prosac + magsac {NAME[dt]}: iterations {out['iterations'].cpu().tolist()}, inliers {out['inliers'].cpu().tolist()}, fits "
          f"{out['irls_fits'].cpu().tolist()}")
    assert np.isfinite(model).all() and bool(torch.isfinite(out["score"]).all())
    assert out["irls_fits"].dtype == torch.int32 and bool((out["irls_fits"] >= 0).all()) and bool((out["irls_fits"] <= 10).all())
    assert int(out["inliers"][0]) >= 0.4 * N          # the 60 % pair, sampled from its best-ranked points, finds its plane
