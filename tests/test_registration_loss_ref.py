"""Host-side checks of the registration training loss: the f64 reference tests/registration_loss_ref.py against the maths it states
and against the MSAC score of tests/registration_ref.py, the rules its inputs must satisfy, the C header and the built library, and
loss.registration_errors.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from tests import registration_loss_ref as RL
from tests import registration_ref as R

SYMBOLS = [f"dr_registration_{n}_{s}" for n in ("loss_fused", "loss_scale", "loss_fwd", "gt_mask") for s in ("f32", "f64")]


@pytest.mark.parametrize("N,M", RL.CASES)
def test_closed_form_gradient_equals_autograd(N, M):
    cs = RL.case(N, M)
    for use_mask, use_keep, pairs in RL.VARIANTS:
        thr2 = RL.thr2_of(RL.threshold_of(pairs), "float64")
        ref = RL.reference(cs, thr2, use_mask, use_keep)
        g = RL.closed_form_gradient(cs, thr2, ref)
        unit, _ = RL.gradient_units(cs, thr2, ref, use_mask, "float64")
        # both are f64 evaluations of the same sums in different orders: a few units of eps n mag, and exactly 0 where nothing is live
        assert (np.abs(g - ref["grad"]).max((-1, -2)) <= 4.0 * unit).all()
        assert not ref["grad"][..., 3, :].any() and not g[..., 3, :].any()
        assert not ref["grad"][~ref["keep"]].any()
        assert 0.0 <= ref["mean"] <= 1.0 and abs(ref["mean"] - ref["per_pair"].mean()) < 1e-15


def test_sums_are_the_msac_score_on_the_masked_points():
    for N, M in ((257, 65), (65, 65), (1, 65)):
        cs = RL.case(N, M)
        ref = RL.reference(cs, RL.thr2_of(RL.THRESHOLD, "float64"), True, False)
        for p in range(RL.P):
            rows = cs["matches"][p][cs["mask"][p]]
            for m in range(M):
                score = R.msac(rows, cs["models"][p, m], RL.THRESHOLD)[0] if len(rows) else 0.0
                assert abs((len(rows) - ref["sums"][p, m]) - score) <= 1e-12 * max(1, len(rows)), (N, p, m)


@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
def test_inputs_respect_the_band_cap_and_the_rounding_margin(dtype_name):
    for N, M in RL.CASES:
        cs = RL.case(N, M, dtype_name)
        RL.check_inputs(cs, dtype_name)                    # (also asserted when the case is built)
        for use_mask, _, pairs in RL.GRAD_VARIANTS:
            near = RL.near_boundary(cs, RL.thr2_of(RL.threshold_of(pairs), dtype_name), use_mask, dtype_name)
            assert near.sum() <= RL.BAND_CAP * near.size
        assert cs["mask"].any(1).all() and cs["keep"].any(1).all()
    # both branches of the truncation occur in most models of a case with more than a handful of points
    cs = RL.case(257, 65, dtype_name)
    ref = RL.reference(cs, RL.thr2_of(RL.THRESHOLD, dtype_name), True, False)
    both = ref["live"].any(-1) & (ref["masked"][:, None, :] & ~ref["live"]).any(-1)
    assert both.mean() > 0.5


def test_tolerance_constant_is_measured_and_finite():
    w, c = RL.worst_plain_ratio(), RL.tolerance_constant()
    print("registration loss: worst plain f32 ratio w[N] =", {k: round(v, 4) for k, v in w.items()})
    assert set(c) == set(RL.N_SWEEP) and all(0 < v < math.inf for v in c.values()) and c == {N: 4.0 * v for N, v in w.items()}
    # the tolerance separates a wrong formula: the gradient without the truncation (every masked point live) is far outside it
    cs = RL.case(257, 65, "float32")
    thr2 = RL.thr2_of(RL.THRESHOLD, "float32")
    ref = RL.reference(cs, thr2, True, True)
    unit, compared = RL.gradient_units(cs, thr2, ref, True, "float32")
    g = RL.closed_form_gradient(cs, thr2 * 1e6, ref) * 1e6          # thr2 -> huge: nothing is truncated; same 2 / thr2 factor
    assert RL.worst_ratio(g, ref["grad"], unit, compared) > 100 * c[257]


@pytest.mark.parametrize("N,M", RL.CASES)
def test_extended_reference_agrees_with_autograd(N, M):
    """the long-double closed form (g_ref of the f64 GPU tests) against f64 autograd: the autograd reference is a correct f64
    evaluation, so it has to meet the bound c = 4 w that an f64 kernel has to meet against the same g_ref"""
    cs = RL.case(N, M)
    c = RL.tolerance_constant()[N]
    for use_mask, use_keep, pairs in RL.GRAD_VARIANTS:
        thr2 = RL.thr2_of(RL.threshold_of(pairs), "float64")
        ref = RL.reference(cs, thr2, use_mask, use_keep)
        unit, compared = RL.gradient_units(cs, thr2, ref, use_mask, "float64")
        g = RL.extended_gradient(cs, thr2, ref)
        assert g.dtype == np.longdouble and np.finfo(np.longdouble).eps <= 2.0 ** -63
        assert RL.worst_ratio(ref["grad"], g, unit, compared) <= c


def test_header_declares_and_library_exports_the_loss_entries():
    declared = set(L.entries()) | {"dr_version", "dr_last_error"}
    assert not [s for s in SYMBOLS if s not in declared]
    lib = L.lib()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    assert lib.dr_version() == 1


def test_entries_refuse_bad_arguments_without_a_gpu():
    lib = L.lib()
    buf = (ctypes.c_char * 256)()
    for sfx in ("f32", "f64"):
        fused, fwd = getattr(lib, f"dr_registration_loss_fused_{sfx}"), getattr(lib, f"dr_registration_loss_fwd_{sfx}")
        scale, gtm = getattr(lib, f"dr_registration_loss_scale_{sfx}"), getattr(lib, f"dr_registration_gt_mask_{sfx}")
        assert fused(None, None, buf, None, buf, 1, 1, 1, buf, buf, buf, buf, buf, None) == -1 and b"null" in lib.dr_last_error()
        assert fused(buf, None, buf, None, buf, 1, 1, 1, buf, None, buf, buf, buf, None) == -1       # no gradient buffer
        assert fwd(buf, None, buf, None, None, 1, 1, 1, buf, buf, buf, buf, None) == -1              # no thr2
        assert scale(buf, buf, None, 1, 1, buf, None) == -1 and b"null" in lib.dr_last_error()
        assert gtm(buf, None, buf, 1, 1, buf, buf, None) == -1 and b"null" in lib.dr_last_error()
        for P, M, N in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
            assert fused(buf, None, buf, None, buf, P, M, N, buf, buf, buf, buf, buf, None) == -1 and b"dr_registration_loss_fused" in lib.dr_last_error()
            assert fwd(buf, None, buf, None, buf, P, M, N, buf, buf, buf, buf, None) == -1
        assert scale(buf, buf, buf, 0, 1, buf, None) == -1 and scale(buf, buf, buf, 1, 0, buf, None) == -1
        assert gtm(buf, buf, buf, 0, 1, buf, buf, None) == -1 and gtm(buf, buf, buf, 1, 0, buf, buf, None) == -1


def test_registration_errors_on_constructed_poses():
    from differentiable_ransac_amd.loss import registration_errors

    def pose(deg, axis, t):
        a = math.radians(deg)
        c, s = math.cos(a), math.sin(a)
        Rm = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
        M = torch.eye(4, dtype=torch.float64)
        M[:3, :3], M[:3, 3] = torch.tensor(Rm, dtype=torch.float64), torch.tensor(t, dtype=torch.float64)
        return M
    gt = pose(30.0, "z", [1.0, 2.0, 3.0])
    models = torch.stack([gt @ pose(d, ax, [0.0, 0.0, 0.0]) for d, ax in ((0.0, "x"), (90.0, "y"), (180.0, "x"))])
    models[:, :3, 3] = gt[:3, 3] + torch.tensor([3.0, 0.0, 4.0], dtype=torch.float64)          # |dt| = 5
    rre, rte = registration_errors(models, gt)
    assert torch.allclose(rre, torch.tensor([0.0, 90.0, 180.0], dtype=torch.float64), atol=1e-6)
    assert torch.allclose(rte, torch.full((3,), 5.0, dtype=torch.float64), atol=1e-12)
    rre, rte = registration_errors(models.reshape(1, 3, 4, 4).float(), gt.float())            # leading dimensions, f32, broadcast
    assert rre.shape == (1, 3) and rte.shape == (1, 3) and not rre.requires_grad
    assert torch.allclose(rre[0], torch.tensor([0.0, 90.0, 180.0]), atol=0.05)


def test_loss_refuses_mismatched_arguments_before_any_launch():
    from differentiable_ransac_amd import ops
    m, mod = torch.zeros(2, 5, 6), torch.zeros(2, 3, 4, 4)
    with pytest.raises(L.DransacError):
        ops.registration_loss_mean(m, None, mod.double(), 0.05)
    with pytest.raises(L.DransacError):
        ops.registration_loss_mean(m[..., :4], None, mod, 0.05)
    with pytest.raises(L.DransacError):
        ops.registration_loss_sums(m, torch.zeros(2, 4, dtype=torch.bool), mod, 0.05)
    with pytest.raises(L.DransacError):
        ops.registration_gt_mask(m, torch.zeros(2, 3, 3), 0.05)
    from differentiable_ransac_amd.loss import RegistrationLoss
    with pytest.raises(L.DransacError, match="models only"):          # no gradient to the correspondences: refused, not dropped
        RegistrationLoss(0.05)(mod.requires_grad_(True), m.clone().requires_grad_(True))
