"""Host-side checks of the homography training loss: the f64 reference tests/homography_loss_ref.py against the maths it states and
against the MSAC score of tests/homography_ref.py, the rules its inputs must satisfy, the C header and the built library,
loss.HomographyLoss's refusals and loss.homography_errors.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from tests import homography_loss_ref as HL
from tests import homography_ref as HR

SYMBOLS = [f"dr_homography_{n}_{s}" for n in ("loss_fused", "loss_scale", "loss_fwd", "gt_mask") for s in ("f32", "f64")]


@pytest.mark.parametrize("N,M", HL.CASES)
def test_closed_form_gradient_equals_autograd(N, M):
    cs = HL.case(N, M)
    for use_mask, use_keep, pairs in HL.VARIANTS:
        thr2 = HL.thr2_of(HL.threshold_of(pairs), "float64")
        ref = HL.reference(cs, thr2, use_mask, use_keep)
        g = HL.closed_form_gradient(cs, thr2, ref)
        unit, _ = HL.gradient_units(cs, thr2, ref, use_mask, "float64")
        # both are f64 evaluations of the same sums in different orders: within the worst-case weights, and exactly 0 where nothing is live
        assert (np.abs(g - ref["grad"]) <= unit).all()
        assert not ref["grad"][~ref["keep"]].any() and not g[~ref["keep"]].any()
        assert 0.0 <= ref["mean"] <= 1.0 and abs(ref["mean"] - ref["per_pair"].mean()) < 1e-15


@pytest.mark.parametrize("N,M", HL.CASES)
def test_extended_reference_agrees_with_autograd_and_both_are_orthogonal_to_the_model(N, M):
    """the long-double closed form (g_ref of the f64 GPU tests) against f64 autograd: the autograd reference is a correct f64
    evaluation, so it has to meet the bound c = 4 w that an f64 kernel has to meet against the same g_ref; <grad, H> = 0"""
    cs = HL.case(N, M)
    c = HL.tolerance_constant()[N]
    for use_mask, use_keep, pairs in HL.GRAD_VARIANTS:
        thr2 = HL.thr2_of(HL.threshold_of(pairs), "float64")
        ref = HL.reference(cs, thr2, use_mask, use_keep)
        unit, compared = HL.gradient_units(cs, thr2, ref, use_mask, "float64")
        g = HL.extended_gradient(cs, thr2, ref)
        assert g.dtype == np.longdouble and np.finfo(np.longdouble).eps <= 2.0 ** -63
        assert HL.worst_ratio(ref["grad"], g, unit, compared) <= c
        assert HL.worst_ratio(HL.closed_form_gradient(cs, thr2, ref), g, unit, compared) <= c
        assert HL.inner_ratio(ref["grad"], cs, unit, compared) <= c
        assert HL.inner_ratio(g.astype(np.float64), cs, unit, compared) <= c
        assert np.abs(ref["grad"][ref["keep"]]).max() > 0 or N == 1


def test_loss_is_invariant_under_scale_and_sign_of_the_models():
    cs = HL.case(257, 65)
    thr2 = HL.thr2_of(HL.THRESHOLD_PAIRS, "float64")
    base = HL.reference(cs, thr2)
    rng = np.random.default_rng(5)
    factor = rng.uniform(0.25, 4.0, (HL.P, 65, 1, 1)) * rng.choice([-1.0, 1.0], (HL.P, 65, 1, 1))
    other = HL.reference(dict(cs, models=cs["models"] * factor), thr2)
    assert np.allclose(other["sums"], base["sums"], rtol=1e-9, atol=1e-9) and abs(other["mean"] - base["mean"]) < 1e-12
    assert np.allclose(other["grad"] * factor, base["grad"], rtol=1e-6, atol=1e-9 * np.abs(base["grad"]).max())


def test_sums_are_the_msac_score_on_the_masked_points():
    for N, M in ((257, 65), (65, 65), (1, 65)):
        cs = HL.case(N, M)
        ref = HL.reference(cs, HL.thr2_of(HL.THRESHOLD, "float64"), True, False)
        for p in range(HL.P):
            rows = cs["matches"][p][cs["mask"][p]]
            for m in range(M):
                score = HR.msac(rows, cs["models"][p, m], HL.THRESHOLD)[0] if len(rows) else 0.0
                assert abs((len(rows) - ref["sums"][p, m]) - score) <= 1e-9 * max(1, len(rows)), (N, p, m)


@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
def test_inputs_respect_the_band_cap_and_the_rounding_margin(dtype_name):
    for N, M in HL.CASES:
        cs = HL.case(N, M, dtype_name)
        HL.check_inputs(cs, dtype_name)                    # (also asserted when the case is built)
        for use_mask, _, pairs in HL.GRAD_VARIANTS:
            near = HL.near_boundary(cs, HL.thr2_of(HL.threshold_of(pairs), dtype_name), use_mask, dtype_name)
            assert near.sum() <= HL.BAND_CAP * near.size
        assert cs["keep"].any(1).all() and (N < 63 or cs["mask"].any(1).all())
        assert np.array_equal(cs["models"], cs["models"].astype(dtype_name).astype(np.float64))
        norms = np.linalg.norm(cs["models"].reshape(HL.P, M, 9), axis=-1)
        assert norms.min() >= 0.25 * (1 - 1e-6) and norms.max() <= 4.0 * (1 + 1e-6)
        assert M < 63 or ((np.linalg.det(cs["models"]) < 0).any() and (np.linalg.det(cs["models"]) > 0).any())
    # both branches of the truncation occur in most models of a case with more than a handful of points
    cs = HL.case(257, 65, dtype_name)
    ref = HL.reference(cs, HL.thr2_of(HL.THRESHOLD, dtype_name), True, False)
    both = ref["live"].any(-1) & (ref["masked"][:, None, :] & ~ref["live"]).any(-1)
    assert both.mean() > 0.5


def test_tolerance_constant_is_measured_and_finite():
    w, c = HL.worst_plain_ratio(), HL.tolerance_constant()
    print("homography loss: worst plain f32 ratio w[N] =", {k: round(v, 4) for k, v in w.items()})
    assert set(c) == set(HL.N_SWEEP) and all(0 < v < math.inf for v in c.values()) and c == {N: 4.0 * v for N, v in w.items()}
    # the tolerance separates a wrong formula: the gradient without the truncation (every masked point in front live) is far outside it
    cs = HL.case(257, 65, "float32")
    thr2 = HL.thr2_of(HL.THRESHOLD, "float32")
    ref = HL.reference(cs, thr2, True, True)
    unit, compared = HL.gradient_units(cs, thr2, ref, True, "float32")
    g = HL.closed_form_gradient(cs, thr2 * 1e6, ref) * 1e6          # thr2 -> huge: nothing is truncated; same 2 / thr2 factor
    assert HL.worst_ratio(g, ref["grad"], unit, compared) > 100 * c[257]


def test_header_declares_and_library_exports_the_loss_entries():
    entries = L.entries()
    assert not [s for s in SYMBOLS if s not in entries]
    lib = L.lib()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    assert lib.dr_version() == 1
    ptr, i = L.c_pointer, L.c_int
    for sfx in ("f32", "f64"):
        assert entries[f"dr_homography_loss_fused_{sfx}"] == [ptr] * 5 + [i] * 3 + [ptr] * 6
        assert entries[f"dr_homography_loss_fwd_{sfx}"] == [ptr] * 5 + [i] * 3 + [ptr] * 5
        assert entries[f"dr_homography_loss_scale_{sfx}"] == [ptr] * 3 + [i] * 2 + [ptr] * 2
        assert entries[f"dr_homography_gt_mask_{sfx}"] == [ptr] * 3 + [i] * 2 + [ptr] * 3
        for kind in ("loss_fused", "loss_fwd", "loss_scale", "gt_mask"):      # the registration entries' argument shapes
            assert entries[f"dr_homography_{kind}_{sfx}"] == entries[f"dr_registration_{kind}_{sfx}"]


def test_entries_refuse_bad_arguments_without_a_gpu():
    lib = L.lib()
    buf = (ctypes.c_char * 256)()
    for sfx in ("f32", "f64"):
        fused, fwd = getattr(lib, f"dr_homography_loss_fused_{sfx}"), getattr(lib, f"dr_homography_loss_fwd_{sfx}")
        scale, gtm = getattr(lib, f"dr_homography_loss_scale_{sfx}"), getattr(lib, f"dr_homography_gt_mask_{sfx}")
        assert fused(None, None, buf, None, buf, 1, 1, 1, buf, buf, buf, buf, buf, None) == -1 and b"null" in lib.dr_last_error()
        assert fused(buf, None, buf, None, buf, 1, 1, 1, buf, None, buf, buf, buf, None) == -1       # no gradient buffer
        assert fwd(buf, None, buf, None, None, 1, 1, 1, buf, buf, buf, buf, None) == -1              # no thr2
        assert scale(buf, buf, None, 1, 1, buf, None) == -1 and b"null" in lib.dr_last_error()
        assert gtm(buf, None, buf, 1, 1, buf, buf, None) == -1 and b"null" in lib.dr_last_error()
        for P, M, N in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (65536, 1, 1), (1 << 11, 1 << 11, 1)):
            assert fused(buf, None, buf, None, buf, P, M, N, buf, buf, buf, buf, buf, None) == -1 and b"dr_homography_loss_fused" in lib.dr_last_error()
            assert fwd(buf, None, buf, None, buf, P, M, N, buf, buf, buf, buf, None) == -1
        assert scale(buf, buf, buf, 0, 1, buf, None) == -1 and scale(buf, buf, buf, 1, 0, buf, None) == -1
        assert gtm(buf, buf, buf, 0, 1, buf, buf, None) == -1 and gtm(buf, buf, buf, 1, 0, buf, buf, None) == -1


def test_homography_errors_on_constructed_homographies():
    from differentiable_ransac_amd.loss import homography_errors
    gt = torch.tensor(HR.scene(7, 8, 1.0)["H"])
    assert float(homography_errors(-3.5 * gt, gt, (480, 640))) < 1e-9                          # any scale, either sign
    # a shift by (3, 4) moves every corner by 5; a scale of 2 about the origin moves (0,0), (w,0), (w,h), (0,h) by 0, w, |(w,h)|, h
    eye = torch.eye(3, dtype=torch.float64)
    shift = eye.clone()
    shift[0, 2], shift[1, 2] = 3.0, 4.0
    zoom = torch.diag(torch.tensor([2.0, 2.0, 1.0], dtype=torch.float64))
    err = homography_errors(torch.stack([shift, zoom]), eye, (30, 40))
    assert torch.allclose(err, torch.tensor([5.0, (0.0 + 40.0 + 50.0 + 30.0) / 4.0], dtype=torch.float64), atol=1e-12)
    err = homography_errors(torch.stack([shift, zoom]).reshape(1, 2, 3, 3).float(), eye.float(), (30, 40))      # leading dimensions, f32
    assert err.shape == (1, 2) and not err.requires_grad and torch.allclose(err[0], torch.tensor([5.0, 30.0]), atol=1e-4)


def test_loss_refuses_mismatched_arguments_before_any_launch():
    from differentiable_ransac_amd import ops
    from differentiable_ransac_amd.loss import HomographyLoss
    m, mod = torch.zeros(2, 5, 4), torch.zeros(2, 3, 3, 3)
    with pytest.raises(L.DransacError):
        ops.homography_loss_mean(m, None, mod.double(), 3.0)
    with pytest.raises(L.DransacError):
        ops.homography_loss_mean(torch.zeros(2, 5, 6), None, mod, 3.0)
    with pytest.raises(L.DransacError):
        ops.homography_loss_sums(m, torch.zeros(2, 4, dtype=torch.bool), mod, 3.0)
    with pytest.raises(L.DransacError):
        ops.homography_gt_mask(m, torch.zeros(2, 4, 4), 3.0)
    with pytest.raises(L.DransacError, match="models only"):          # no gradient to the matches: refused, not dropped
        HomographyLoss(3.0)(mod.requires_grad_(True), m.clone().requires_grad_(True))
