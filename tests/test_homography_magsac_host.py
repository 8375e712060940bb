"""MAGSAC++ scoring and IRLS polish of the homography path without a GPU: the properties of the oracle
tests/homography_magsac_ref.py, the conditions on the oracle's side that tests/test_gpu_homography_magsac.py rests on (its seeds were
chosen here), the ABI of dr_homography_magsac_score / dr_homography_irls (declared, exported, DR_EINVAL before any device work) and the
constructor checks of BatchedHomography(scoring=, irls_iters=)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from tests import homography_magsac_ref as MR
from tests import homography_ref as R

SYMBOLS = ["dr_homography_magsac_score_f32", "dr_homography_magsac_score_f64", "dr_homography_irls_f32", "dr_homography_irls_f64"]
THR = R.THRESHOLD
SCENES = [(60, 300, 0.6), (61, 300, 0.35), (62, 120, 0.5), (63, 700, 0.35), (64, 64, 0.6)]


# ------------------------------------------------------------------------------------------------ weight and loss
def _simpson(f, a, b, n=2000):
    x = np.linspace(a, b, 2 * n + 1)
    y = f(x)
    return float((b - a) / (6.0 * n) * (y[0] + y[-1] + 4.0 * y[1:-1:2].sum() + 2.0 * y[2:-1:2].sum()))


def test_loss_is_the_normalised_integral_of_x_w():
    """rho(d) = int_0^d x w(x^2 / thr^2) dx, l = rho(d) / rho(thr): by Simpson's rule in x on 4001 nodes (w is smooth on [0, thr]; the
    rule's error is below 1e-12 here), at 25 distances.  And d rho / d(d^2) = w / 2, by central differences of the oracle's loss."""
    f = lambda x: x * MR.weight(x * x / (THR * THR))
    rho1 = _simpson(f, 0.0, THR)
    worst = 0.0
    for d in np.linspace(0.04, 0.999, 25) * THR:
        worst = max(worst, abs(_simpson(f, 0.0, d) / rho1 - float(MR.loss(d * d / (THR * THR)))))
    print(f"largest |quadrature - loss| = {worst:.3g}")
    assert worst <= 1e-10
    s = np.linspace(0.02, 0.98, 49)
    h = 1e-6
    slope = (MR.loss(s + h) - MR.loss(s - h)) / (2.0 * h)            # d l / d s = w(s) thr^2 / (2 rho(thr))
    err = np.abs(slope - MR.weight(s) * THR * THR / (2.0 * rho1)).max()
    print(f"largest |d loss / d s - w thr^2 / (2 rho(thr))| = {err:.3g}")
    assert err <= 1e-8


def test_loss_and_weight_shapes_and_constants():
    assert MR.K2 == 13.276704135987622 and MR.UK == 0.5 * MR.K2
    s = np.linspace(0.0, 1.0, 20001)[:-1]
    l, w = MR.loss(s), MR.weight(s)
    assert l[0] == 0.0 and float(MR.weight(0.0)) == 1.0
    assert float(MR.weight(1.0)) == 0.0 and float(MR.weight(3.0)) == 0.0 and float(MR.weight(np.nextafter(1.0, 0.0))) < 1e-12
    assert float(MR.loss(1.0)) == 1.0 and float(MR.loss(7.0)) == 1.0 and abs(float(MR.loss(np.nextafter(1.0, 0.0))) - 1.0) < 1e-12
    assert (np.diff(1.0 - l) < 0).all() and (1.0 - l > 0).all()       # 1 - l falls monotonically from 1 to 0
    assert (w >= 0).all() and (np.diff(w) < 0).all()
    # L is the largest slope of 1 - l: at s = 0, by a one-sided difference
    h = 1e-7
    assert abs(float(MR.loss(h)) / h - MR.L) < 1e-4 and (np.diff(l) / np.diff(s) <= MR.L * (1 + 1e-9)).all()


def test_score_on_exact_matches_is_n_and_edge_points_add_nothing():
    H = R.random_h(np.random.default_rng(0))
    x1 = np.random.default_rng(1).uniform(0.0, 640.0, (37, 2))
    y = np.concatenate([x1, np.ones((37, 1))], 1) @ H.T
    m = np.concatenate([x1, y[:, :2] / y[:, 2:]], 1)
    s, n = MR.magsac(m, H, THR)
    assert n == 37 and abs(s - 37.0) < 1e-9
    m[1, 2] += 10.0 * THR                     # an outlier
    m[2, 3] = np.nan                          # a NaN point
    s, n = MR.magsac(m, H, THR)
    assert n == 35 and abs(s - 35.0) < 1e-9
    assert MR.magsac(m, np.full((3, 3), np.nan), THR)[1] == 0 and math.isnan(MR.magsac(m, np.zeros((3, 3)), THR)[0])
    for name in ("float32", "float64"):
        assert MR.score_tolerance(m, H, THR, name) >= 37 * MR.e_term(name)


# ------------------------------------------------------------------------------------------------ irls
@pytest.mark.parametrize("seed,N,share", SCENES)
def test_irls_never_lowers_the_score_and_lowers_the_error(seed, N, share):
    sc = R.scene(seed, N, share)
    m = sc["matches"]
    H0 = MR.perturbed(sc["H"], np.random.default_rng(seed))
    s0 = MR.magsac(m, H0, THR)[0]
    trace = []
    H1, s1, fits, margins = MR.irls(m, H0, THR, 10, trace=trace)
    e0, e1 = R.mean_transfer_error(H0, m, sc["inlier"]), R.mean_transfer_error(H1, m, sc["inlier"])
    print(f"N={N} share={share}: score {s0:.4f} -> {s1:.4f}, fits {fits}, mean transfer error {e0:.4f} -> {e1:.4f}, margins "
          f"{[f'{x:.2e}' for x in margins]}")
    assert s1 > s0 and 1 <= fits <= 10 and len(trace) == fits
    assert all(x > 0 for x in margins[:-1])
    assert s1 == MR.magsac(m, H1, THR)[0]
    assert e1 < e0
    # from the converged result: at most one further fit, which does not win by more than the rounding of a score
    Hc, sc_, _, _ = MR.irls(m, H0, THR, 300)
    H2, s2, fits2, _ = MR.irls(m, Hc, THR, 10)
    assert s2 >= sc_ and s2 - sc_ < 1e-9 * max(sc_, 1.0)


def test_irls_stops_without_four_rows_and_on_a_bad_model():
    sc = R.scene(70, 100, 0.5)
    far = R.canonical(np.array([[1.0, 0.0, 1e4], [0.0, 1.0, 1e4], [0.0, 0.0, 1.0]]))
    assert MR.magsac(sc["matches"], far, THR) == (0.0, 0)
    H, s, fits, margins = MR.irls(sc["matches"], far, THR, 10)
    assert fits == 0 and s == 0.0 and margins == [] and np.array_equal(H, far)
    H, s, fits, _ = MR.irls(sc["matches"], np.full((3, 3), np.nan), THR, 10, score=0.0)
    assert fits == 0 and s == 0.0
    # a claimed score no fit reaches: one fit, which loses
    H0 = MR.perturbed(sc["H"], np.random.default_rng(3))
    H, s, fits, margins = MR.irls(sc["matches"], H0, THR, 10, score=1e6)
    assert fits == 1 and s == 1e6 and margins[0] < 0 and np.array_equal(H, H0)


# ------------------------------------------------------------------------------------------------ the GPU tests' conditions
@pytest.mark.parametrize("name", ["float32", "float64"])
def test_the_score_cases_keep_the_band_share(name):
    for N in MR.SCORE_N:
        for M in MR.SCORE_M:
            m, models, valid = MR.score_case(N, M, name)
            inband, cells = MR.band_share(m, models, valid, THR, name)
            assert cells > 0 and inband <= R.BAND_SHARE_MAX * cells, (N, M, inband, cells)
            best = max(MR.magsac(m[p], models[p, j], THR)[0] for p in range(len(m)) for j in range(M) if valid[p, j])
            assert best > 0.15 * N or M == 1, (N, M, best)         # the cases score real models too (a sanity check, not a bound)


@pytest.mark.parametrize("N", MR.IRLS_N)
def test_the_irls_cases_are_clear_of_their_tolerances(N):
    """f64 at IRLS_STEPS[N] steps: every pair; f32 at one step: every pair (the GPU test allows one of four to fail this)"""
    for name, iters in (("float64", MR.IRLS_STEPS[N]), ("float32", 1)):
        _, _, _, out = MR.irls_case(N, name, iters)
        assert all(MR.irls_clear(o, name) for o in out), (N, name)
        assert [o["fits"] for o in out] == [iters, iters, 0, 0] and all(o["margins"][0] > 0 for o in out[:2])
    for name in ("float32", "float64"):
        _, _, _, out = MR.irls_case(257, name, 4, claimed=(1e6, 257.0))
        assert [o["fits"] for o in out] == [1, 1, 0, 0] and all(MR.irls_clear(o, name) for o in out)


def test_the_driver_case_is_clear_of_its_tolerances():
    """the driver test's scenes and noise, with the index sets as the top four of the noise (what the sampler returns for zero logits)
    and the oracle's own closed-form models: every decision margin and every IRLS margin exceeds the tolerance"""
    from differentiable_ransac_amd import synth
    D = MR.DRV
    rounds = math.ceil(D["max_iterations"] / D["B"])
    noise = [synth.gumbel_noise((D["P"], D["B"], D["N"]), seed=1000 + r, dtype=torch.float64) for r in range(rounds)]
    idx = [torch.topk(x, 4, dim=-1).indices.numpy() for x in noise]
    for p, sc in enumerate(MR.driver_scenes()):
        m = sc["matches"]
        o = MR.run(m, [i[p] for i in idx], THR, max_iterations=D["max_iterations"], irls_iters=D["irls_iters"], dtype_name="float64")
        tol = max(o["tols"] + [MR.score_tolerance(m, o["model"], THR, "float64")])
        margin = min(o["gaps"] + [abs(x) for x in o["irls_margins"]])
        print(f"pair {p}: rounds {o['rounds']} inliers {o['inliers']} fits {o['irls_fits']} margin {margin:.3g} tolerance {tol:.3g}")
        assert margin > tol and o["irls_fits"] == D["irls_iters"]
        assert not any(R.in_band(t["ratio2"], "float64").any() for t in o["irls_trace"])
        assert o["inliers"] > 4                                      # every pair's winner holds more than its own sample


# ------------------------------------------------------------------------------------------------ library and driver
def test_header_declares_and_library_exports_the_entries():
    declared = set(L.entries())
    assert not [s for s in SYMBOLS if s not in declared]
    lib = L.lib()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]


def test_entries_refuse_bad_arguments_without_a_gpu():
    lib = L.lib()
    buf = (ctypes.c_char * 256)()
    for sfx in ("f32", "f64"):
        score = getattr(lib, "dr_homography_magsac_score_" + sfx)

        def call_score(matches=buf, models=buf, thr2=buf, P=1, M=1, N=1, scores=buf):
            return score(matches, models, None, thr2, P, M, N, scores, None, None)

        for name in ("matches", "models", "thr2", "scores"):
            assert call_score(**{name: None}) == -1 and b"null" in lib.dr_last_error(), name
        for kw in (dict(P=0), dict(M=0), dict(N=-1), dict(P=65536)):
            assert call_score(**kw) == -1 and b"dr_homography_magsac_score" in lib.dr_last_error(), kw
        irls = getattr(lib, "dr_homography_irls_" + sfx)

        def call_irls(matches=buf, thr2=buf, P=1, N=1, iters=1, score=buf, model=buf, fits=buf):
            return irls(matches, thr2, P, N, iters, score, model, fits, None)

        for name in ("matches", "thr2", "score", "model", "fits"):
            assert call_irls(**{name: None}) == -1 and b"null" in lib.dr_last_error(), name
        for kw in (dict(P=0), dict(N=0), dict(N=-3)):
            assert call_irls(**kw) == -1 and b"dr_homography_irls" in lib.dr_last_error(), kw
        for it in (0, -1):
            assert call_irls(iters=it) == -1 and b"irls_iters" in lib.dr_last_error()


def test_constructor_checks():
    from differentiable_ransac_amd.ransac import BatchedHomography
    d = BatchedHomography()
    assert d.scoring == "msac" and d.irls_iters == 10
    m = BatchedHomography(scoring="magsac", irls_iters=0)
    assert m.scoring == "magsac" and m.irls_iters == 0
    with pytest.raises(ValueError, match="scoring must be"):
        BatchedHomography(scoring="lmeds")
    with pytest.raises(ValueError, match="train"):
        BatchedHomography(scoring="magsac", train=True)
    with pytest.raises(ValueError, match="irls_iters"):
        BatchedHomography(scoring="magsac", irls_iters=-1)
    with pytest.raises(TypeError):
        BatchedHomography(scoring="magsac", lo=1)           # local optimisation is not an argument of this driver
    assert BatchedHomography(scoring="msac", train=True).train
    assert BatchedHomography(scoring="magsac", sampling="prosac").sampling == "prosac"


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes(monkeypatch):
    from differentiable_ransac_amd import ops
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    st = ops.HomographyState(2, 16, 100, "cpu", torch.float32)
    with pytest.raises(L.DransacError):
        ops.homography_irls(st, torch.rand(2, 16, 4), torch.full((2,), 9.0), 4, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(L.DransacError, match="matches"):
        ops.homography_magsac_score(torch.rand(2, 16, 6), torch.rand(2, 3, 3, 3), 3.0)
    with pytest.raises(L.DransacError, match="models"):
        ops.homography_magsac_score(torch.rand(2, 16, 4), torch.rand(2, 3, 4, 4), 3.0)
    assert calls == []
