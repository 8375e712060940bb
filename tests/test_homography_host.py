"""The f64 oracle of the homography path (tests/homography_ref.py) checked against itself and against an SVD, the conditions its GPU
cases must meet, and the constructor's refusals -- no GPU."""
import math

import numpy as np
import pytest

from tests import homography_ref as R
from differentiable_ransac_amd.ransac import BatchedHomography

EPS = R.eps_of("float64")


def _project(H, x1):
    y = np.concatenate([x1, np.ones((len(x1), 1))], 1) @ H.T
    return y[:, :2] / y[:, 2:]


def test_closed_form_equals_the_svd_dlt_on_well_conditioned_samples():
    rng = np.random.default_rng(0)
    seen = 0
    for s in range(4):
        m = R.scene(s, 300, 0.6)["matches"]
        for _ in range(64):
            smp = m[rng.choice(300, 4, replace=False)]
            o = R.closed_form(smp)
            if not (o["valid"] and o["conditioning"] > R.WELL):
                continue
            d = R.dlt(smp)
            assert d["valid"]
            # the closed form's bound plus the SVD's own: eps sigma_1 / (sigma_8 - sigma_9) per rounding, 64 of them as in the refit
            tol = R.model_tolerance(o["conditioning"], "float64") + 64.0 * EPS * d["sv"][0] / (d["sv"][7] - d["sv"][8])
            err = np.abs(o["model"] - d["model"]).max()
            assert err <= tol, (err, tol, o["conditioning"])
            seen += 1
    assert seen >= 40


def test_a_noise_free_homography_is_recovered():
    rng = np.random.default_rng(1)
    for s in range(8):
        H = R.random_h(rng)
        x1 = rng.uniform(0.0, 640.0, (4, 2))
        o = R.closed_form(np.concatenate([x1, _project(H, x1)], 1))
        if o["conditioning"] <= R.WELL:
            continue
        assert o["valid"]
        assert abs(np.linalg.norm(o["model"]) - 1.0) < 4 * EPS and np.linalg.det(o["model"]) > 0
        # (the projected x2 carry their own rounding, half an ulp of 640 over a unit scale: inside the same bound)
        assert np.abs(o["model"] - H).max() <= R.model_tolerance(o["conditioning"], "float64") + 64 * EPS / o["conditioning"]


def test_collinear_and_orientation_flipped_samples_are_rejected():
    x1 = np.array([[10.0, 20.0], [30.0, 40.0], [50.0, 60.0], [400.0, 100.0]])       # three points on a line (integers: exactly)
    x2 = np.array([[15.0, 25.0], [200.0, 40.0], [80.0, 300.0], [410.0, 120.0]])
    assert not R.closed_form(np.concatenate([x1, x2], 1))["valid"]
    assert not R.closed_form(np.concatenate([x2, x1], 1))["valid"]
    sq = np.array([[0.0, 0.0], [100.0, 0.0], [100.0, 100.0], [0.0, 100.0]])
    assert R.closed_form(np.concatenate([sq, sq + 5.0], 1))["valid"]
    flip = sq[[1, 0, 2, 3]]                                                           # two corners swapped: a triangle changes its turn
    assert not R.closed_form(np.concatenate([sq, flip], 1))["valid"]
    mirror = sq * np.array([-1.0, 1.0])                                               # a reflection: every triangle does
    assert not R.closed_form(np.concatenate([sq, mirror], 1))["valid"]
    bad = np.concatenate([sq, sq], 1)
    bad[2, 1] = np.nan
    assert not R.closed_form(bad)["valid"]


def test_points_behind_the_vanishing_line_are_outliers():
    # y_w = 1 - x / 320: the vanishing line x = 320 crosses the points
    H = R.canonical(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0 / 320.0, 0.0, 1.0]]))
    rng = np.random.default_rng(2)
    x1 = rng.uniform(0.0, 640.0, (200, 2))
    x1 = x1[np.abs(x1[:, 0] - 320.0) > 5.0]
    m = np.concatenate([x1, _project(H, x1)], 1)                                      # every point fits H exactly...
    score, inl, r = R.msac(m, H, 3.0)
    front = x1[:, 0] < 320.0
    assert front.any() and (~front).any()
    assert inl == int(front.sum()) and np.array_equal(r < 1.0, front)                # ...and only those in front count
    assert abs(score - front.sum()) < 1e-6
    assert R.msac(m, -H, 3.0)[:2] == (score, inl)                                     # the sign rule is applied by the residual
    assert math.isnan(R.msac(m, np.zeros((3, 3)), 3.0)[0])


@pytest.mark.parametrize("share", [0.6, 0.35])
def test_run_recovers_the_homography(share):
    N, B = 300, 256
    sc = R.scene(5 if share > 0.5 else 6, N, share)
    rng = np.random.default_rng(7)
    idx = [np.stack([rng.choice(N, 4, replace=False) for _ in range(B)]) for _ in range(8)]
    out = R.run(sc["matches"], idx, max_iterations=B * 8)
    assert out["inliers"] >= 0.9 * sc["inlier"].sum()
    assert (out["mask"] & ~sc["inlier"]).sum() <= 0.05 * N
    err = R.mean_transfer_error(out["model"], sc["matches"], sc["inlier"])
    truth = R.mean_transfer_error(sc["H"], sc["matches"], sc["inlier"])
    print(f"share {share}: rounds {out['rounds']} inliers {out['inliers']} / {sc['inlier'].sum()} error {err:.3f} (truth {truth:.3f})")
    assert err < 1.5 * truth + 0.1
    assert out["iterations"] == out["rounds"] * B


@pytest.mark.parametrize("case", R.GPU_CASES, ids=[f"P{c[0]}-N{c[1]}-B{c[2]}" for c in R.GPU_CASES])
@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
def test_the_caps_hold_for_the_gpu_cases(case, dtype_name):
    c = R.gpu_case(*case, dtype_name=dtype_name)
    well, band = R.caps(list(c["matches"]), list(c["idx"]), [None] * len(c["matches"]), R.THRESHOLD, dtype_name)
    print(f"{case} {dtype_name}: well-conditioned {well:.3f} in band {band:.5f}")
    assert well >= R.WELL_SHARE_MIN
    assert band <= R.BAND_SHARE_MAX


def test_the_constructor_refuses_what_it_must():
    for kw in (dict(sampling="prosac", train=True), dict(sampling="other"), dict(max_iterations=0), dict(ransac_batch_size=0),
               dict(prosac_draws=0)):
        with pytest.raises(ValueError):
            BatchedHomography(**kw)
    import torch
    drv = BatchedHomography()
    with pytest.raises(ValueError, match=r"\[P,N,4\]"):
        drv(torch.zeros(1, 8, 6), torch.zeros(1, 8))
    with pytest.raises(ValueError, match="prosac"):
        BatchedHomography(sampling="prosac")(torch.zeros(1, 8, 4), torch.zeros(1, 8), gumbels=[torch.zeros(1, 4, 8)])
    import differentiable_ransac_amd
    assert differentiable_ransac_amd.BatchedHomography is BatchedHomography
