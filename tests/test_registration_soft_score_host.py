"""The differentiable soft-inlier score of the registration path and loss.RegistrationExpectedLoss without a GPU: the two forms of the
reference tests/registration_soft_score_ref.py against each other and against central differences, the ABI of the new entries, the
refusals of ops.registration_soft_score before any launch, the loss's arithmetic with the score op replaced by the reference's scores,
and PnPExpectedLoss's value through the base the two losses now share."""
import ctypes

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from tests import pnp_ref as R
from tests import pnp_soft_score_ref as PS
from tests import registration_soft_score_ref as S

SYMBOLS = [f"dr_{n}_{s}" for n in ("registration_soft_score", "registration_soft_score_bwd") for s in ("f32", "f64")]


def _torch_grads(c, gs):
    tm, to = torch.tensor(c["m"], requires_grad=True), torch.tensor(c["models"], requires_grad=True)
    mask = None if c["mask"] is None else torch.tensor(c["mask"])
    ts = S.torch_soft_score(tm, mask, to, torch.tensor(c["keep"]), c["thr"], S.BETA)
    (ts * torch.tensor(np.where(c["keep"], gs, 0.0))).sum().backward()
    return ts.detach().numpy(), to.grad.numpy(), tm.grad.numpy()


@pytest.mark.parametrize("cs", S.CASES[:2], ids=str)
def test_the_closed_form_equals_f64_torch_autograd(cs):
    """Two evaluations in different orders, autograd's in f64.  d = R p + t - q cancels from |q| <= 3.5 to a fraction of the threshold's
    0.04: a rounding is eps 3.5 / 0.01 = 8e-14 of a term, some ten roundings per term; a gradient row is a signed sum of up to 300 such
    terms that may itself cancel by two orders: 1e-9 of the case's largest entry with a margin.  A score is a sum of at most n_scored
    weights, each moved by at most |dw / da| |da| = 0.25 x 2000 x 2 |d| x 4e-16 x 10 roundings < 1e-12."""
    c = S.case(*cs)
    gs = np.random.default_rng(1).normal(size=c["keep"].shape)
    s, gm, gx = S.soft_score(c["m"], c["mask"], c["models"], c["keep"], c["thr"], S.BETA, gs)
    ts, tgm, tgx = _torch_grads(c, gs)
    P, N, M = cs
    n_scored = N if c["mask"] is None else c["mask"].sum(1).max()
    es, em, ex = np.abs(s - ts).max(), np.abs(gm - tgm).max() / np.abs(gm).max(), np.abs(gx - tgx).max() / np.abs(gx).max()
    print(f"closed form against autograd {cs}: scores {es:.3g}, grad_models {em:.3g}, grad_matches {ex:.3g} (relative)")
    assert np.isfinite(tgm).all() and np.isfinite(tgx).all() and np.isfinite(gm).all() and np.isfinite(gx).all()
    assert es <= 1e-12 * n_scored and em <= 1e-9 and ex <= 1e-9
    assert not s[~c["keep"]].any() and not gm[~c["keep"]].any() and not s[:, M - 1].any() and not gm[:, M - 1].any()
    assert not s[1].any() and not gm[1].any() and not gx[1].any() and c["thr"][1] == 0.0        # the pair without a threshold
    assert not gm[:, :, 3].any() and s[0, M - 4] > 0.9 * 0.6 * (n_scored if c["mask"] is None else c["mask"][0].sum()) * 0.9
    if c["mask"] is not None:
        assert not gx[~c["mask"]].any() and (~c["mask"]).any()
    # the weights span (0, 1), and part of the inliers lies beyond the cutoff under the moved pose
    G = S._grid(c["m"][0], c["models"][0, [M - 2]], c["thr"][0] ** 2, S.BETA)
    inl = G["a"][0] > -400.0
    assert (G["a"][0][inl] < S.CUTOFF).any() and (G["a"][0][inl] > S.CUTOFF).any()
    w = S._grid(c["m"][0], c["models"][0][c["keep"][0]][:-1], c["thr"][0] ** 2, S.BETA)["w"]
    assert ((w > 0.05) & (w < 0.3)).any() and ((w > 0.4) & (w < 0.6)).any() and (w > 0.9).any()


def test_central_differences_of_the_reference_agree_with_its_gradient():
    """L = <gs, scores>: (L(x + h) - L(x - h)) / 2h, h = 1e-7, on 40 entries of the matches and 40 of the models, relative to the
    largest derivative of its kind.  The truncation is (h / l)^2 with l the length over which a weight changes, thr / sqrt(beta) ~ 0.02
    in the distance (a rotation entry moves a point by |p| <= 1.8 of its change): 1e-10.  The rounding is eps sum |gs s| / h =
    1e-16 x 1e3 / 1e-7 = 1e-6 against derivatives of the order of 100: 1e-8.  Bound: 1e-6."""
    c = S.case(3, 70, 80)
    gs = np.where(c["keep"], np.random.default_rng(2).normal(size=c["keep"].shape), 0.0)
    _, gm, gx = S.soft_score(c["m"], c["mask"], c["models"], c["keep"], c["thr"], S.BETA, gs)
    L0 = lambda m, mo: float((gs * S.soft_score(m, c["mask"], mo, c["keep"], c["thr"], S.BETA)).sum())
    rng, h, worst = np.random.default_rng(3), 1e-7, 0.0
    use = np.argwhere(c["keep"] & np.isfinite(c["models"][:, :, 1, 2]) & (c["thr"] > 0)[:, None])
    for k in range(40):
        p, n, d = (0, 2)[rng.integers(2)], rng.integers(70), rng.integers(6)
        a, b = c["m"].copy(), c["m"].copy()
        a[p, n, d] += h
        b[p, n, d] -= h
        worst = max(worst, abs((L0(a, c["models"]) - L0(b, c["models"])) / (2 * h) - gx[p, n, d]) / np.abs(gx).max())
        (p, j), r, q = use[rng.integers(len(use))], rng.integers(3), rng.integers(4)
        a, b = c["models"].copy(), c["models"].copy()
        a[p, j, r, q] += h
        b[p, j, r, q] -= h
        worst = max(worst, abs((L0(c["m"], a) - L0(c["m"], b)) / (2 * h) - gm[p, j, r, q]) / np.abs(gm).max())
    print(f"central differences against the closed form: worst relative error {worst:.3g} (bound 1e-6)")
    assert np.abs(gx).max() > 0 and np.abs(gm).max() > 0 and worst <= 1e-6


def test_header_declares_and_library_exports_and_checks_the_entries():
    declared = L.entries()
    assert not [s for s in SYMBOLS if s not in declared]
    # the f32 and f64 signatures match, float for double, and are the PnP entries'
    text = lambda e: str(e).replace("float", "T").replace("double", "T").replace("f32", "").replace("f64", "")
    for n in ("soft_score", "soft_score_bwd"):
        assert text(declared[f"dr_registration_{n}_f32"]) == text(declared[f"dr_registration_{n}_f64"])
    lib = L.lib()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    for n in ("soft_score", "soft_score_bwd"):
        for sfx in ("f32", "f64"):
            assert getattr(lib, f"dr_registration_{n}_{sfx}").argtypes == getattr(lib, f"dr_pnp_{n}_{sfx}").argtypes
    buf = (ctypes.c_char * 256)()
    for sfx in ("f32", "f64"):
        fwd, bwd = getattr(lib, "dr_registration_soft_score_" + sfx), getattr(lib, "dr_registration_soft_score_bwd_" + sfx)
        assert fwd(buf, None, buf, None, buf, 5.0, 1, 1, 1, None, None) == -1 and b"null" in lib.dr_last_error()
        assert fwd(buf, None, buf, None, buf, 5.0, 1, 0, 1, buf, None) == -1 and b"dr_registration_soft_score" in lib.dr_last_error()
        assert fwd(buf, None, buf, None, buf, 0.0, 1, 1, 1, buf, None) == -1 and b"beta" in lib.dr_last_error()
        assert fwd(buf, None, buf, None, buf, float("nan"), 1, 1, 1, buf, None) == -1 and b"beta" in lib.dr_last_error()
        assert bwd(buf, None, buf, None, buf, 5.0, None, 1, 1, 1, buf, None, None) == -1 and b"null" in lib.dr_last_error()
        assert bwd(buf, None, buf, None, buf, 5.0, buf, 1 << 12, 1 << 12, 1, buf, None, None) == -1 and b"2^22" in lib.dr_last_error()
        assert bwd(buf, None, buf, None, buf, -1.0, buf, 1, 1, 1, buf, buf, None) == -1 and b"beta" in lib.dr_last_error()


def test_the_wrapper_refuses_before_any_launch(monkeypatch):
    from differentiable_ransac_amd import ops
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    m, mo = torch.rand(2, 16, 6), torch.rand(2, 8, 4, 4)
    with pytest.raises(L.DransacError, match=r"\[P,N,6\]"):
        ops.registration_soft_score(torch.rand(2, 16, 5), mo, 0.05)                  # wrong width
    with pytest.raises(L.DransacError, match=r"\[P,N,6\]"):
        ops.registration_soft_score(torch.rand(16, 6), mo, 0.05)
    for bad in (torch.rand(2, 8, 3, 3), torch.rand(2, 8, 16), torch.rand(3, 8, 4, 4)):    # wrong model shape
        with pytest.raises(L.DransacError, match="models"):
            ops.registration_soft_score(m, bad, 0.05)
    with pytest.raises(L.DransacError, match="dtype"):
        ops.registration_soft_score(m, mo.double(), 0.05)                            # dtype mix
    with pytest.raises(L.DransacError, match="dtype"):
        ops.registration_soft_score(m.half(), mo.half(), 0.05)
    for beta in (0.0, -1.0, float("nan"), float("inf"), torch.tensor(5.0)):
        with pytest.raises(L.DransacError, match="beta"):
            ops.registration_soft_score(m, mo, 0.05, beta)
    with pytest.raises(L.DransacError, match="mask"):
        ops.registration_soft_score(m, mo, 0.05, mask=torch.ones(2, 15, dtype=torch.bool))
    with pytest.raises(L.DransacError, match="keep"):
        ops.registration_soft_score(m, mo, 0.05, keep=torch.ones(2, 9, dtype=torch.bool))
    with pytest.raises(L.DransacError, match="bool"):
        ops.registration_soft_score(m, mo, 0.05, keep=torch.ones(2, 8))
    with pytest.raises(L.DransacError):
        ops.registration_soft_score(m, mo, torch.full((3,), 0.05))                   # a threshold that is neither a float nor [P]
    with pytest.raises(L.DransacError, match="GPU tensors"):
        ops.registration_soft_score(m, mo, 0.05)                                     # CPU tensors
    assert calls == []


def test_the_loss_arithmetic_matches_the_reference_on_stubbed_scores(monkeypatch):
    """RegistrationExpectedLoss with ops.registration_soft_score replaced by the reference's scores (as a differentiable leaf), on the
    CPU in f64: the soft-max over the kept slots, the pairs without a usable slot, both clamps.  Against the reference's pair-by-pair
    form."""
    from differentiable_ransac_amd import loss, ops
    c = S.case(3, 70, 80)
    P, N, M = 3, 70, 80
    keep = c["keep"].copy()
    keep[2, : M // 2] = False
    thr = np.abs(c["thr"]) + 0.04 * (c["thr"] == 0)                                  # every pair scored here; pair 1 loses its slots:
    keep[1] = False                                                                  # a pair without a kept slot
    models = c["models"].copy()
    models[0, M - 3, :3, :3] = R.rot([0.0, 2.5, 0.0]) @ models[0, M - 3, :3, :3]      # 143 degrees: above max_loss
    scores = torch.tensor(S.soft_score(c["m"], None, models, keep, thr), requires_grad=True)
    seen = []
    monkeypatch.setattr(ops, "registration_soft_score", lambda *a, **k: seen.append(a) or scores)
    to, gt = torch.tensor(models, requires_grad=True), torch.tensor(c["poses"])
    crit = loss.RegistrationExpectedLoss(thr)
    got = crit(to, torch.tensor(c["m"]), gt, keep=torch.tensor(keep))
    got.backward()
    assert len(seen) == 1 and seen[0][3] == 5.0 and seen[0][4] is None               # (matches, models, threshold, beta, mask, keep)
    assert (crit.beta, crit.alpha, crit.trans_weight, crit.max_loss) == (5.0, 100.0, 50.0, 100.0) and S.LOSS["trans_weight"] == 50.0
    s2, t2 = scores.detach().clone().requires_grad_(True), torch.tensor(models, requires_grad=True)
    want, per_pair, probs = S.expected_loss(t2, s2, N, gt, torch.tensor(keep), **S.LOSS)
    want.backward()
    assert abs(float(got.detach()) - float(want.detach())) <= 1e-12 * float(want.detach())
    assert torch.allclose(crit.per_pair, per_pair.detach(), rtol=1e-12, atol=0)
    assert torch.allclose(crit.probs, probs.detach(), rtol=1e-12, atol=1e-300) and float(crit.per_pair[1]) == 0.0
    assert torch.equal(crit.scores, scores.detach())
    assert not bool(crit.probs[~torch.tensor(keep)].any()) and not bool(crit.probs[:, M - 1].any())
    assert torch.isfinite(to.grad).all() and torch.isfinite(scores.grad).all()
    assert torch.allclose(to.grad, t2.grad, rtol=1e-9, atol=1e-12 * float(t2.grad.abs().max()))
    assert torch.allclose(scores.grad, s2.grad, rtol=1e-9, atol=1e-12 * float(s2.grad.abs().max()))
    assert not bool(to.grad[1].any()) and not bool(scores.grad[1].any()) and not bool(to.grad[~torch.tensor(keep)].any())
    # the clamps: the generating pose sits on the arc-cosine's clamp (finite, zero gradient), the far pose on max_loss
    errs = S.pose_errors(torch.tensor(models[:1, [M - 4, M - 3]]), gt[:1], S.LOSS["trans_weight"], S.LOSS["max_loss"])[0]
    assert abs(float(errs[0]) - np.degrees(2.0 * np.arcsin(np.sqrt(0.5e-6)))) < 1e-9 and float(errs[1]) == S.LOSS["max_loss"]
    assert not bool(to.grad[0, M - 4].any()) and not bool(to.grad[0, M - 3].any())


def test_pnp_expected_loss_keeps_its_signature_and_value_through_the_shared_base(monkeypatch):
    """A fixed input with the formulae written out here in numpy (nothing of loss.py or of the reference modules): two pairs, four
    slots, one dropped, scores given; l = min(max(RRE deg, 100 RTE), 100), probs = softmax(100 s / N) over the kept slots."""
    import inspect

    from differentiable_ransac_amd import loss, ops
    assert issubclass(loss.PnPExpectedLoss, loss._ExpectedLoss) and issubclass(loss.RegistrationExpectedLoss, loss._ExpectedLoss)
    sig = inspect.signature(loss.PnPExpectedLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == [("beta", 5.0), ("alpha", 100.0), ("trans_weight", 100.0),
                                                                            ("max_loss", 100.0)]
    assert list(inspect.signature(loss.PnPExpectedLoss.forward).parameters) == ["self", "models", "matches", "gt_pose", "keep", "mask"]
    N = 50
    angles = np.radians([[1.0, 3.0, 0.5, 20.0], [2.0, 0.25, 170.0, 4.0]])
    shifts = np.array([[0.002, 0.05, 0.03, 0.1], [0.5, 0.001, 0.2, 2.0]])
    sc = np.array([[30.0, 29.5, 30.2, 12.0], [20.0, 20.6, 3.0, 20.3]])
    keep = np.array([[True, True, False, True], [True, True, True, True]])
    gt = np.stack([R.pose(R.rot([0.3, -0.2, 0.1]), [0.1, 0.2, 3.0]), R.pose(R.rot([-0.5, 0.4, 0.2]), [0.0, -0.3, 4.0])])
    models = np.empty((2, 4, 4, 4))
    for p in range(2):
        for j in range(4):
            axis = np.array([1.0, 2.0, -1.0 + j]) / np.linalg.norm([1.0, 2.0, -1.0 + j])
            models[p, j] = R.pose(R.rot(axis * angles[p, j]) @ gt[p][:3, :3], gt[p][:3, 3] + shifts[p, j] * np.array([0.6, 0.0, 0.8]))
    models[0, 2] = np.nan
    ell = np.minimum(np.maximum(np.degrees(angles), 100.0 * shifts), 100.0)
    want = []
    for p in range(2):
        z = 100.0 * sc[p, keep[p]] / N
        q = np.exp(z - z.max())
        want.append(float((q / q.sum() * ell[p, keep[p]]).sum()))
    monkeypatch.setattr(ops, "pnp_soft_score", lambda *a, **k: torch.tensor(np.where(keep, sc, 0.0)))
    crit = loss.PnPExpectedLoss(0.005)
    got = crit(torch.tensor(models), torch.zeros(2, N, 5, dtype=torch.float64), torch.tensor(gt), keep=torch.tensor(keep))
    assert np.allclose(crit.per_pair.numpy(), want, rtol=1e-9, atol=0) and abs(float(got) - np.mean(want)) <= 1e-9 * np.mean(want)
