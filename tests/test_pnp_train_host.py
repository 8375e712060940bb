"""The trainable absolute-pose path without a GPU: the reference tests/pnp_grad_ref.py against finite differences of pnp_ref.p3p and
against f64 torch autograd of the loss written in plain CPU torch, the ABI of the new entries (declared in include/dransac.h, exported,
bound), and the refusals of BatchedPnP.hypotheses before any launch."""
import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from tests import pnp_grad_ref as G
from tests import pnp_ref as R

SYMBOLS = [f"dr_{n}_{s}" for n in ("p3p", "p3p_bwd", "pnp_gt_mask", "pnp_loss_fused", "pnp_loss_fwd", "pnp_loss_scale")
           for s in ("f32", "f64")]
FD_H = 1e-6
FD_BOUND = 1e-6


def _nearest(sol, T):
    return min(sol, key=lambda s: sum(R.pose_error(s, T)))


def test_p3p_vjp_against_central_differences_of_the_reference_p3p():
    """L = <G, T> of the pose that continues T: (L(m3 + h e) - L(m3 - h e)) / 2h, h = 1e-6, following the nearest pose.  The bound 1e-6
    is relative to the largest entry of the sample's derivative; the truncation of the difference (h^2 L''' / 6) and its rounding
    (eps |L| / h ~ 1e-10) are what the margin is for."""
    m, idx = R.solver_case(1, 64, 33)
    rng = np.random.default_rng(0)
    worst, models = 0.0, 0
    for b in range(33):
        m3 = m[0][idx[0][b]]
        sol, info = R.p3p(m3)
        assert R.comparable(info) and info["tri"] > 0.0, b            # none is left out
        for T in sol:
            Gm = rng.normal(size=(4, 4))
            got = G.p3p_vjp(m3, T, Gm)
            fd = np.zeros((3, 5))
            for i in range(3):
                for d in range(5):
                    L2 = []
                    for sgn in (1.0, -1.0):
                        mp = m3.copy()
                        mp[i, d] += sgn * FD_H
                        L2.append(float(np.sum(Gm[:3] * _nearest(R.p3p(mp)[0], T)[:3])))
                    fd[i, d] = (L2[0] - L2[1]) / (2.0 * FD_H)
            err = float(np.abs(got - fd).max() / np.abs(fd).max())
            worst, models = max(worst, err), models + 1
            assert err <= FD_BOUND, (b, err)
    print(f"p3p_vjp against central differences: {models} models, worst relative error {worst:.3g} (bound {FD_BOUND:g})")
    assert models == 51


def test_p3p_vjp_ignores_row_3_and_the_normal_part_of_the_rotation_gradient():
    m, idx = R.solver_case(1, 64, 33)
    m3 = m[0][idx[0][0]]
    T = R.p3p(m3)[0][0]
    rng = np.random.default_rng(1)
    Gm = rng.normal(size=(4, 4))
    base = G.p3p_vjp(m3, T, Gm)
    other = Gm.copy()
    other[3] = rng.normal(size=4)
    S = rng.normal(size=(3, 3))
    other[:3, :3] += (S + S.T) @ T[:3, :3]                           # d R = [w]x R is orthogonal to S R for a symmetric S
    again = G.p3p_vjp(m3, T, other)
    assert np.abs(again - base).max() <= 1e-9 * np.abs(base).max()
    Gs = np.stack([Gm] * 4)
    out, valid, _ = G.p3p_vjp_slots(m[0], idx[0][:1], np.where(np.arange(4)[:, None, None] < valid_count(m3), Gs, np.nan))
    assert np.isfinite(out).all() and valid.sum() == valid_count(m3)


def test_root_pose_lands_on_the_root_and_barely_moves_the_pose():
    m, idx = R.solver_case(1, 64, 33)
    worst_move = worst_res = 0.0
    for b in range(33):
        m3 = m[0][idx[0][b]]
        for T in R.p3p(m3)[0]:
            Tr = G.root_pose(m3, T)
            worst_move = max(worst_move, float(np.abs(Tr - T).max()))
            worst_res = max(worst_res, float(np.sqrt(R.residual(m3, Tr)[0].max())))
            assert np.abs(Tr[:3, :3] @ Tr[:3, :3].T - np.eye(3)).max() < 1e-14 and np.array_equal(Tr[3], [0, 0, 0, 1])
    print(f"root_pose: largest move of a pose entry {worst_move:.3g}, largest sample residual afterwards {worst_res:.3g}")
    # (evaluated in f64 on the pose rounded to f64: that rounding alone moves x_c / z_c by a few eps |x_c| / z_c)
    assert worst_move < 1e-11 and worst_res < 1e-13


def valid_count(m3):
    return len(R.p3p(m3)[0])


def _torch_loss(m, mask, models, keep, thr):
    """the loss in plain f64 torch, for autograd: the same expression, no formula of the gradient"""
    P = m.shape[0]
    thr2 = torch.as_tensor(np.broadcast_to(np.asarray(thr, np.float64) ** 2, (P,)).copy())
    finite = torch.isfinite(models[:, :, :3]).all(-1).all(-1)
    safe = torch.where(finite[:, :, None, None], models, torch.zeros_like(models))
    xc = torch.einsum("pmij,pnj->pmni", safe[:, :, :3, :3], m[:, :, :3]) + safe[:, :, None, :3, 3]
    front = xc[..., 2] > 0
    z = torch.where(front, xc[..., 2], torch.ones_like(xc[..., 2]))
    d2 = (xc[..., 0] / z - m[:, None, :, 3]) ** 2 + (xc[..., 1] / z - m[:, None, :, 4]) ** 2
    live = front & (d2 < thr2[:, None, None]) & finite[:, :, None]
    term = torch.where(live, d2 / thr2[:, None, None], torch.ones_like(d2))
    sums = (term * mask[:, None, :]).sum(-1) * keep
    den = (mask.sum(1) * keep.sum(1)).clamp(min=1.0)
    return sums, sums.sum(1) / den, (sums.sum(1) / den).mean()


@pytest.mark.parametrize("thr", [R.THRESHOLD, (R.THRESHOLD, 0.8 * R.THRESHOLD, 1.25 * R.THRESHOLD)])
def test_pnp_loss_against_f64_torch_autograd(thr):
    m, models, valid, poses = R.score_case(7)
    thr_p = np.broadcast_to(np.asarray(thr, np.float64), (3,))
    mask = np.stack([R.inlier_mask(m[p], poses[p], thr_p[p]) for p in range(3)])
    mask[:, -1] = True                                                # the point behind the camera is among the masked ones
    assert np.isnan(models[:, 130]).all() and valid[:, 130].all() and not valid[:, 131].any() and mask.sum(1).min() >= 3
    sums, per_pair, mean, grad = G.pnp_loss(m, mask, models, valid, thr)
    tm = torch.tensor(models, requires_grad=True)
    ts, tp, tmean = _torch_loss(torch.tensor(m), torch.tensor(mask).double(), tm, torch.tensor(valid).double(), thr)
    tmean.backward()
    want = tm.grad.numpy()
    assert np.abs(sums - ts.detach().numpy()).max() <= 1e-12 * max(1.0, sums.max())
    assert np.abs(per_pair - tp.detach().numpy()).max() <= 1e-13 and abs(mean - float(tmean.detach())) <= 1e-13
    assert np.isfinite(want).all() and np.abs(grad).max() > 0.0
    err = float(np.abs(grad - want).max() / np.abs(want).max())
    print(f"pnp_loss gradient against torch autograd: relative error {err:.3g}, |grad| max {np.abs(want).max():.3g}")
    # two f64 evaluations in different orders.  e = x_c / z_c - u cancels from |x_c / z_c| <= 2.3 to below the threshold (0.004 at the
    # least): a rounding is eps 2.3 / 0.004 = 1.3e-13 of a term, ten roundings per term, up to five live points: 1e-11 with a margin
    assert err <= 1e-11
    assert not grad[:, 130].any() and not grad[:, 131].any() and not grad[:, :, 3].any()
    assert (sums[:, 130] == mask.sum(1)).all() and not sums[:, 131].any()
    # the point behind the camera counts 1 under the generating pose and passes nothing: the same gradient with a far outlier in its place
    moved = m.copy()
    moved[:, -1, 3:] += 1.0
    s2, _, _, g2 = G.pnp_loss(moved, mask, models, valid, thr)
    assert np.array_equal(s2[:, 128], sums[:, 128]) and np.array_equal(g2[:, 128], grad[:, 128])


def test_header_declares_and_library_exports_and_binds_the_entries():
    declared = L.entries()
    assert not [s for s in SYMBOLS if s not in declared]
    lib = L.lib()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    buf = (__import__("ctypes").c_char * 256)()
    for sfx in ("f32", "f64"):
        fwd, bwd = getattr(lib, "dr_p3p_" + sfx), getattr(lib, "dr_p3p_bwd_" + sfx)
        assert fwd(None, 1, buf, buf, None) == -1 and b"null" in lib.dr_last_error()
        assert fwd(buf, 0, buf, buf, None) == -1 and b"dr_p3p" in lib.dr_last_error()
        assert bwd(buf, None, 1, buf, None) == -1 and b"null" in lib.dr_last_error()
        assert bwd(buf, buf, 1 << 29, buf, None) == -1 and b"dr_p3p_bwd" in lib.dr_last_error()
        fused = getattr(lib, "dr_pnp_loss_fused_" + sfx)
        assert fused(buf, None, buf, None, buf, 1, 1, 1, buf, None, buf, buf, buf, None) == -1 and b"null" in lib.dr_last_error()
        assert fused(buf, None, buf, None, buf, 1, 0, 1, buf, buf, buf, buf, buf, None) == -1 and b"dr_pnp_loss_fused" in lib.dr_last_error()


def test_wrappers_and_hypotheses_refuse_before_any_launch(monkeypatch):
    from differentiable_ransac_amd import BatchedPnP, loss, ops
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    with pytest.raises(NotImplementedError, match="DESIGN.md"):
        BatchedPnP(train=True)
    assert issubclass(loss.PnPLoss, loss._PairLoss) and loss.PnPLoss(0.005).threshold == 0.005
    m, lg = torch.rand(2, 16, 5), torch.zeros(2, 16)
    with pytest.raises(ValueError, match="prosac"):
        BatchedPnP(sampling="prosac").hypotheses(m, lg)
    with pytest.raises(ValueError, match=r"\[P,N,5\]"):
        BatchedPnP().hypotheses(torch.rand(2, 16, 4), lg)
    with pytest.raises(ValueError, match=r"\[P,N,5\]"):
        BatchedPnP().hypotheses(torch.rand(16, 5), lg)
    with pytest.raises(ValueError, match="dtype"):
        BatchedPnP().hypotheses(m, lg.double())
    d = BatchedPnP(ransac_batch_size=64, max_iterations=256)
    d.device_termination = True
    with pytest.raises(ValueError, match="device_termination"):
        d.hypotheses(m, lg)
    with pytest.raises(L.DransacError, match="GPU tensors"):
        ops.p3p(torch.rand(4, 3, 5))
    with pytest.raises(L.DransacError, match="samples"):
        ops.p3p(torch.rand(4, 4, 5))
    with pytest.raises(L.DransacError, match="float32 or float64"):
        ops.p3p(torch.zeros(4, 3, 5, dtype=torch.int32))
    mo = torch.rand(2, 8, 4, 4)
    for fn in (lambda: ops.pnp_gt_mask(torch.rand(2, 16, 6), mo[:, 0], 0.005), lambda: ops.pnp_loss_mean(torch.rand(2, 16, 4), None, mo, 0.005),
               lambda: ops.pnp_loss_sums(torch.rand(16, 5), None, mo, 0.005)):
        with pytest.raises(L.DransacError, match="matches"):
            fn()
    with pytest.raises(L.DransacError, match="detach"):
        ops.pnp_loss_mean(m.clone().requires_grad_(True), None, mo, 0.005)
    with pytest.raises(L.DransacError, match="pose"):
        ops.pnp_gt_mask(m, torch.rand(2, 3, 3), 0.005)
    assert calls == []
