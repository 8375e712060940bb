"""MAGSAC++ scoring and IRLS polish of the registration path without a GPU: the properties of the oracle
tests/registration_magsac_ref.py, the ABI of dr_rigid_magsac_score / dr_registration_irls (declared, exported, DR_EINVAL before any
device work) and the constructor checks of BatchedRegistration(scoring=, irls_iters=)."""
import ctypes

import numpy as np
import pytest

from differentiable_ransac_amd import _lib as L
from tests import registration_magsac_ref as MR
from tests import registration_ref as R

SYMBOLS = ["dr_rigid_magsac_score_f32", "dr_rigid_magsac_score_f64", "dr_registration_irls_f32", "dr_registration_irls_f64"]
THR = R.THRESHOLD
IRLS_ITERS = 10
SCENES = [(60, 300, 0.6), (61, 300, 0.35), (62, 300, 0.15), (63, 120, 0.5), (64, 700, 0.35), (65, 64, 0.6)]
POLISH_SEEDS = list(range(200, 210))      # ten scenes of 30 % inliers, noise 0.005
POLISH_THR = 0.5


# ------------------------------------------------------------------------------------------------ weight and loss
def test_constants():
    assert MR.K2 == 11.344866730144373 and MR.UK == 0.5 * MR.K2 and MR.C == np.exp(-MR.UK)
    assert 5.7 < MR.L < 5.9
    # L is the largest slope of 1 - l: at s = 0, by a one-sided difference
    h = 1e-7
    assert abs(float(MR.loss(h)) / h - MR.L) < 1e-5


def test_loss_and_weight_shapes():
    s = np.linspace(0.0, 1.0, 20001)[:-1]
    l, w = MR.loss(s), MR.weight(s)
    assert l[0] == 0.0 and MR.weight(0.0) == 1.0
    assert abs(float(MR.loss(np.nextafter(1.0, 0.0))) - 1.0) < 1e-12 and float(MR.loss(1.0)) == 1.0 and float(MR.loss(7.0)) == 1.0
    assert (np.diff(l) > 0).all()
    assert (w >= 0).all() and (np.diff(w) < 0).all()
    assert float(MR.weight(np.nextafter(1.0, 0.0))) < 1e-12 and float(MR.weight(1.0)) == 0.0 and float(MR.weight(3.0)) == 0.0
    assert float(MR.weight(np.nan)) == 0.0 and float(MR.loss(np.nan)) == 1.0


def test_weight_is_the_derivative_of_rho():
    """rho(d) = int_0^d x w(x) dx: d rho / d(d^2) = w / 2, by central differences in d^2; and the loss is rho over rho(threshold)"""
    thr = THR
    d2 = np.linspace(0.02, 0.98, 49) * thr * thr
    h = 1e-5 * thr * thr
    num = (MR.rho(d2 + h, thr) - MR.rho(d2 - h, thr)) / (2.0 * h)
    err = np.abs(num - 0.5 * MR.weight(d2 / (thr * thr))).max()
    print(f"largest |d rho / d d2 - w / 2| = {err:.3g}")
    assert err <= 1e-8
    assert np.abs(MR.rho(d2, thr) / MR.rho(thr * thr, thr) - MR.loss(d2 / (thr * thr))).max() < 1e-14


def test_score_of_the_identity_on_identical_clouds_is_n():
    p = np.random.default_rng(0).uniform(0.0, 1.0, (37, 3))
    assert MR.magsac(np.concatenate([p, p], 1), np.eye(4), THR) == (37.0, 37)
    # a point at the cutoff and a NaN point contribute nothing
    m = np.concatenate([p, p], 1)[:3].copy()
    m[1, 3] += THR
    m[2, 4] = np.nan
    s, n = MR.magsac(m, np.eye(4), THR)
    assert n == 1 and s == 1.0


# ------------------------------------------------------------------------------------------------ irls
def _start(sc, rng, deg=2.0, shift=0.02):
    """the generating pose turned by `deg` degrees about a random axis and moved by `shift`"""
    ax = rng.standard_normal(3)
    ax *= np.radians(deg) / np.linalg.norm(ax)
    W = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    M = np.eye(4)
    M[:3, :3] = R._nearest_rotation(np.eye(3) + W + 0.5 * W @ W) @ sc["R"]
    d = rng.standard_normal(3)
    M[:3, 3] = sc["t"] + shift * d / np.linalg.norm(d)
    return M


@pytest.mark.parametrize("seed,N,share", SCENES)
def test_irls_never_lowers_the_score_stops_and_is_a_fixed_point(seed, N, share):
    sc = R.scene(seed, N, share)
    m = sc["matches"]
    M0 = _start(sc, np.random.default_rng(seed))
    s0 = MR.magsac(m, M0, THR)[0]
    M1, s1, fits, margins = MR.irls(m, M0, THR, IRLS_ITERS)
    print(f"N={N} share={share}: score {s0:.4f} -> {s1:.4f}, fits {fits}, margins {[f'{x:.2e}' for x in margins]}")
    assert s1 >= s0 and 1 <= fits <= IRLS_ITERS
    assert all(x > 0 for x in margins[:-1])
    assert s1 == MR.magsac(m, M1, THR)[0]
    # run to convergence, then start from the result: at most one fit, which does not win
    Mc, sc_, _, _ = MR.irls(m, M0, THR, 200)
    M2, s2, fits2, margins2 = MR.irls(m, Mc, THR, IRLS_ITERS)
    assert fits2 <= 1 and s2 == sc_ and np.array_equal(M2, Mc), (fits2, margins2)


def test_irls_stops_without_three_weighted_points_and_on_a_bad_model():
    sc = R.scene(70, 100, 0.5)
    far = np.eye(4)                                   # (q_hat = p: the translation of norm >= 1 leaves no point inside)
    assert MR.magsac(sc["matches"], far, THR) == (0.0, 0)
    M, s, fits, margins = MR.irls(sc["matches"], far, THR, IRLS_ITERS)
    assert fits == 0 and s == 0.0 and margins == [] and np.array_equal(M, far)
    bad = np.full((4, 4), np.nan)
    M, s, fits, _ = MR.irls(sc["matches"], bad, THR, IRLS_ITERS)
    assert fits == 0 and s == 0.0


def _polish_errors(seed, thr):
    sc = R.scene(seed, 300, 0.3, noise=0.005)
    m = sc["matches"]
    rng = np.random.default_rng(seed)
    idx = [np.stack([rng.permutation(300)[:3] for _ in range(64)]) for _ in range(4)]
    o = MR.run(m, idx, thr, max_iterations=256, irls_iters=IRLS_ITERS)
    ref = R.refit(m, o["mask"])
    assert o["inliers"] >= 30 and ref["valid"], seed     # a winner worth polishing
    return o, R.rotation_error_deg(o["model"], sc["R"]), R.rotation_error_deg(ref["model"], sc["R"])


def test_polish_is_no_worse_than_the_inlier_refit_on_most_scenes():
    """30 % inliers, noise 0.005, seeds POLISH_SEEDS: from the RANSAC winner of 4 x 64 random triplets, the rotation error of the IRLS
    result against that of registration_ref.refit on the winner's mask.
    The cutoff is POLISH_THR = 0.5 = 100 sigma, the loose threshold MAGSAC++ is made for: the outliers are uniform in a cube of side 4,
    so a ball of that radius holds 0.8 % of them and a winner's mask carries one to five, which pull the unweighted fit while their
    weight exp(-u_k s) is small.  At the path's default 0.05 = 10 sigma the same ball holds 8e-6 of the outliers: the mask is the
    Gaussian inliers alone, for which the unweighted fit is the maximum-likelihood estimate, and no re-weighting can be expected to
    beat it (measured on these seeds: IRLS is no worse on 4 of 10, with errors within 15 % of each other; printed below, not asserted)."""
    wins = 0
    for seed in POLISH_SEEDS:
        o, e_irls, e_refit = _polish_errors(seed, POLISH_THR)
        _, t_irls, t_refit = _polish_errors(seed, THR)
        print(f"seed {seed}: inliers {o['inliers']}, fits {o['irls_fits']}, rotation error irls {e_irls:.4f} refit {e_refit:.4f} deg "
              f"(at threshold {THR}: {t_irls:.4f} / {t_refit:.4f})")
        wins += e_irls <= e_refit
    print(f"irls no worse on {wins} of {len(POLISH_SEEDS)} seeds")
    assert len(POLISH_SEEDS) >= 8 and 2 * wins > len(POLISH_SEEDS)


# ------------------------------------------------------------------------------------------------ library and driver
def test_header_declares_and_library_exports_the_entries():
    declared = set(L.entries()) | {"dr_version", "dr_last_error"}
    assert not [s for s in SYMBOLS if s not in declared]
    lib = L.lib()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    assert lib.dr_version() == 1


def test_entries_refuse_bad_arguments_without_a_gpu():
    lib = L.lib()
    buf = (ctypes.c_char * 256)()
    for sfx in ("f32", "f64"):
        score = getattr(lib, "dr_rigid_magsac_score_" + sfx)

        def call_score(matches=buf, models=buf, thr2=buf, P=1, M=1, N=1, scores=buf, gi=None, gm=None):
            return score(matches, models, None, thr2, P, M, N, scores, None, gi, gm, None)

        for name in ("matches", "models", "thr2", "scores"):
            assert call_score(**{name: None}) == -1 and b"null" in lib.dr_last_error(), name
        for kw in (dict(P=0), dict(M=0), dict(N=-1), dict(P=65536)):
            assert call_score(**kw) == -1 and b"dr_rigid_magsac_score" in lib.dr_last_error(), kw
        assert call_score(gi=buf) == -1 and b"gate" in lib.dr_last_error()
        irls = getattr(lib, "dr_registration_irls_" + sfx)

        def call_irls(matches=buf, thr2=buf, P=1, N=1, iters=1, score=buf, model=buf, fits=buf):
            return irls(matches, thr2, P, N, iters, score, model, fits, None)

        for name in ("matches", "thr2", "score", "model", "fits"):
            assert call_irls(**{name: None}) == -1 and b"null" in lib.dr_last_error(), name
        for kw in (dict(P=0), dict(N=0), dict(N=-3)):
            assert call_irls(**kw) == -1 and b"registration_irls" in lib.dr_last_error(), kw
        for it in (0, -1):
            assert call_irls(iters=it) == -1 and b"irls_iters" in lib.dr_last_error()


def test_constructor_checks():
    from differentiable_ransac_amd.ransac import BatchedRegistration
    d = BatchedRegistration()
    assert d.scoring == "msac" and d.irls_iters == 10
    m = BatchedRegistration(scoring="magsac", irls_iters=0)
    assert m.scoring == "magsac" and m.irls_iters == 0
    with pytest.raises(ValueError, match="scoring must be"):
        BatchedRegistration(scoring="lmeds")
    for lo in (1, 2):
        with pytest.raises(ValueError, match="MSAC"):
            BatchedRegistration(scoring="magsac", lo=lo)
    with pytest.raises(ValueError, match="train"):
        BatchedRegistration(scoring="magsac", train=True)
    with pytest.raises(ValueError, match="irls_iters"):
        BatchedRegistration(scoring="magsac", irls_iters=-1)
    assert BatchedRegistration(scoring="msac", lo=2, lo_iters=4).lo == 2 and BatchedRegistration(scoring="msac", train=True).train


def test_wrapper_refuses_cpu_tensors(monkeypatch):
    import torch
    from differentiable_ransac_amd import ops
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    st = ops.RegistrationState(2, 16, 100, "cpu", torch.float32)
    with pytest.raises(L.DransacError):
        ops.registration_irls(st, torch.rand(2, 16, 6), torch.full((2,), 0.0025), 4, torch.zeros(2, dtype=torch.int32))
    assert calls == []
