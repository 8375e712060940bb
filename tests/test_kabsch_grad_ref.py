"""Host-side checks of the Kabsch gradient references (tests/kabsch_grad_ref.py) -- that the two agree, how far apart they are (the
tolerance constant of tests/test_gpu_kabsch_grad.py), that the tolerance rejects wrong closed forms -- and of what train mode adds to
the header, the built library and ransac.BatchedRegistration.  No GPU."""

import numpy as np
import pytest

from differentiable_ransac_amd import _lib as L
from tests import kabsch_grad_ref as G
from tests import registration_ref as R

SYMBOLS = [f"dr_{n}_{s}" for n in ("kabsch", "kabsch_bwd", "refit_rigid_bwd") for s in ("f32", "f64")]


def _fit_inputs(n, seed):
    rng = np.random.default_rng(seed)
    x = R.scene(seed, max(n, 8), 0.6)["matches"][:n]
    return x, rng.uniform(0.25, 1.25, n), rng.standard_normal((3, 3)), rng.standard_normal(3)


@pytest.mark.parametrize("n", [3, 4, 8, 50])
def test_the_two_references_agree(n):
    """weighted and unweighted fits of 3, 4, 8 and 50 rows: autograd through the SVD against the closed form, to 1e-10 relative
    (measured: 1e-12) where kappa is moderate"""
    seen = 0
    for seed in range(12):
        x, w, gR, gt = _fit_inputs(n, 40 + seed)
        for wt in (None, w):
            if G.kappa(x, wt) > 100:
                continue
            seen += 1
            ax, aw = G.autograd(x[None], None if wt is None else wt[None], gR[None], gt[None])
            bx, bw = G.closed_form(x, wt, gR, gt)
            assert np.abs(ax[0] - bx).max() <= 1e-10 * np.abs(bx).max()
            assert np.abs(aw[0] - bw).max() <= 1e-10 * G.weight_grad_magnitude(x, wt, gR, gt)
    assert seen >= 12


def test_reference_gradient_against_finite_differences():
    """neither reference is trusted on the other's word alone: central differences of L = sum gR o R + gt . t through
    registration_ref.kabsch"""
    x, w, gR, gt = _fit_inputs(5, 77)

    def loss(xx, ww):
        M = R.kabsch(xx[:, :3], xx[:, 3:], ww)["model"]
        return float((M[:3, :3] * gR).sum() + M[:3, 3] @ gt)
    bx, bw = G.closed_form(x, w, gR, gt)
    h = 1e-6
    for n, d in ((0, 0), (2, 4), (4, 5)):
        e = np.zeros_like(x)
        e[n, d] = h
        assert (loss(x + e, w) - loss(x - e, w)) / (2 * h) == pytest.approx(bx[n, d], rel=1e-6, abs=1e-8)
    for n in (1, 3):
        e = np.zeros_like(w)
        e[n] = h
        assert (loss(x, w + e) - loss(x, w - e)) / (2 * h) == pytest.approx(bw[n], rel=1e-6, abs=1e-8)


def test_tolerance_constant_and_input_conditioning():
    """c per sample size and for the pair cases (printed: docs/LOG.md records it), and the properties of the GPU tests' inputs that
    the tolerance rule asks for: at most 1 % of a case above KAPPA_MAX, and c eps64 kappa <= eps32 on what is compared in f32"""
    c = G.tolerance_constant()
    print("tolerance constants (10 x the largest (a)-(b) distance in units of eps64 kappa mag):", {k: round(float(v), 1) for k, v in c.items()})
    for k in G.SAMPLE_K:
        assert 10.0 <= c[k] < 1e4
        for Bt in G.SAMPLE_BT:
            for weighted in (False, True):
                cs = G.sample_case(Bt, k, weighted, np.float32)
                kap = np.array([G.kappa(cs["x"][s], None if cs["w"] is None else cs["w"][s]) for s in range(Bt)])
                assert (kap > G.KAPPA_MAX).sum() <= 0.01 * Bt, (k, Bt, weighted)
                assert c[k] * G.EPS64 * kap[kap <= G.KAPPA_MAX].max() <= G.EPS32
    assert 10.0 <= c["pair"] < 1e4
    assert c["pair"] * G.EPS64 * G.KAPPA_MAX <= G.EPS32


@pytest.mark.parametrize("wrong", ["flip_gH", "drop_gw_centroid"])
def test_a_wrong_closed_form_misses_the_tolerance(wrong):
    """the sign of gH flipped, and the centroid term of g_w dropped: both are outside c eps64 kappa mag on every sample tried"""
    c = G.tolerance_constant()
    for k in G.SAMPLE_K:
        cs = G.sample_case(65, k, True)
        for s in range(0, 65, 8):
            x, w, gR, gt = cs["x"][s], cs["w"][s], cs["gR"][s], cs["gt"][s]
            if G.kappa(x, w) > G.KAPPA_MAX:
                continue
            assert G.distance_units(x, w, gR, gt) <= c[k]
            assert G.distance_units(x, w, gR, gt, other=G.closed_form(x, w, gR, gt, **{wrong: True})) > c[k]


def test_reflection_sample_is_a_reflection():
    x = G.reflection_sample()
    o = R.kabsch(x[:, :3], x[:, 3:])
    S = np.linalg.svd((x[:, :3] - x[:, :3].mean(0)).T @ (x[:, 3:] - x[:, 3:].mean(0)), compute_uv=False)
    assert o["valid"] and o["flipped"] and S[1] > 2 * S[2] and G.kappa(x) < 100


def test_header_declares_and_library_exports_the_train_entries():
    declared = set(L.entries()) | {"dr_version", "dr_last_error"}
    assert not [s for s in SYMBOLS if s not in declared]
    lib = L.lib()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    assert lib.dr_version() == 1


def test_train_entries_refuse_bad_arguments_without_a_gpu():
    import ctypes
    lib = L.lib()
    buf = (ctypes.c_char * 64)()
    assert lib.dr_kabsch_f32(None, None, 1, 3, None, None, None) == -1 and b"null" in lib.dr_last_error()
    assert lib.dr_kabsch_f64(buf, None, 1, 2, buf, buf, None) == -1                       # k = 2
    assert lib.dr_kabsch_bwd_f32(buf, None, buf, 1, 9, buf, None, None) == -1             # k = 9
    assert lib.dr_kabsch_bwd_f64(buf, None, None, 1, 3, buf, None, None) == -1            # no upstream gradient
    assert lib.dr_refit_rigid_bwd_f32(buf, None, None, buf, 1, 3, None, None, None) == -1  # nothing to write
    assert lib.dr_refit_rigid_bwd_f64(buf, None, None, buf, 0, 3, buf, None, None) == -1


def test_train_mode_constructs():
    from differentiable_ransac_amd import ops
    from differentiable_ransac_amd.ransac import BatchedRegistration
    assert BatchedRegistration().train is False
    drv = BatchedRegistration(ransac_batch_size=65, max_iterations=130, num_samples=4, train=True)
    assert drv.train is True and drv.rounds == 2 and drv.k == 4
    assert callable(ops.kabsch) and callable(ops.weighted_kabsch)
