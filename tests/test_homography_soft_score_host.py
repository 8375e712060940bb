"""The differentiable soft-inlier score of the homography path and loss.HomographyExpectedLoss without a GPU: the two forms of the
reference tests/homography_soft_score_ref.py against each other and against central differences, the score's invariance under the
scale and the sign of a model, the reference's corner errors against loss.homography_errors and loss.homography_corner_errors, the
entries in the header and the library, the refusals of ops.homography_soft_score before any launch, and the loss's arithmetic with the
score op replaced by the reference's scores."""
import ctypes

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from tests import homography_soft_score_ref as S

SYMBOLS = [f"dr_{n}_{s}" for n in ("homography_soft_score", "homography_soft_score_bwd") for s in ("f32", "f64")]
SMALL = (3, 70, 80)


def _torch_grads(c, gs):
    tm, to = torch.tensor(c["m"], requires_grad=True), torch.tensor(c["models"], requires_grad=True)
    mask = None if c["mask"] is None else torch.tensor(c["mask"])
    ts = S.torch_soft_score(tm, mask, to, torch.tensor(c["keep"]), c["thr"], S.BETA)
    (ts * torch.tensor(np.where(c["keep"], gs, 0.0))).sum().backward()
    return ts.detach().numpy(), np.nan_to_num(to.grad.numpy()), tm.grad.numpy()


@pytest.mark.parametrize("cs", S.CASES[:2], ids=str)
def test_the_closed_form_equals_f64_torch_autograd(cs):
    """Two evaluations in different orders, autograd's in f64.  e = x2 - y_xy / y_w cancels from |x2| <= 700 px to a fraction of a pixel:
    a rounding is eps 700 / 0.1 = 2e-12 of a term, some ten roundings per term, and a gradient row is a signed sum of up to 300 such
    terms that may itself cancel by two orders: 1e-8 of the case's largest entry with a margin.  A score is a sum of at most n_scored
    weights, each moved by at most |dw / da| |da| = 0.25 x (5 / 5.8) x 2 |e| x 700 x 1e-16 x 10 roundings < 1e-11."""
    c = S.case(*cs)
    gs = np.random.default_rng(1).normal(size=c["keep"].shape)
    s, gm, gx = S.soft_score(c["m"], c["mask"], c["models"], c["keep"], c["thr"], S.BETA, gs)
    ts, tgm, tgx = _torch_grads(c, gs)
    P, N, M = cs
    n_scored = N if c["mask"] is None else c["mask"].sum(1).max()
    es, em, ex = np.abs(s - ts).max(), np.abs(gm - tgm).max() / np.abs(gm).max(), np.abs(gx - tgx).max() / np.abs(gx).max()
    print(f"closed form against autograd {cs}: scores {es:.3g}, grad_models {em:.3g}, grad_matches {ex:.3g} (relative)")
    assert np.isfinite(tgm).all() and np.isfinite(tgx).all() and np.isfinite(gm).all() and np.isfinite(gx).all()
    assert es <= 1e-11 * n_scored and em <= 1e-8 and ex <= 1e-8
    for j in (S.BAD, S.SINGULAR):                                                    # kept, but not usable
        assert c["keep"][:, j].all() and not s[:, j].any() and not gm[:, j].any()
    assert not s[~c["keep"]].any() and not gm[~c["keep"]].any()
    assert not s[1].any() and not gm[1].any() and not gx[1].any() and c["thr"][1] == 0.0        # the pair without a threshold
    n0 = n_scored if c["mask"] is None else c["mask"][0].sum()
    assert s[0, S.GEN] > 0.45 * n0 and s[0, S.FAR] < 0.01 * n0
    if c["mask"] is not None:
        assert not gx[~c["mask"]].any() and (~c["mask"]).any()
    # the weights span (0, 1), and part of the inliers lies beyond the cutoff under the shifted model
    G = S._grid(c["m"][0], c["models"][0, [M + S.FAR]], c["thr"][0] ** 2, S.BETA)
    inl = G["a"][0] > -400.0
    assert (G["a"][0][inl] < S.CUTOFF).any() and (G["a"][0][inl] > S.CUTOFF).any()
    ok = c["keep"][0] & S.usable_models(c["models"][0])
    w = S._grid(c["m"][0], c["models"][0][ok], c["thr"][0] ** 2, S.BETA)["w"]
    assert ((w > 0.05) & (w < 0.3)).any() and ((w > 0.4) & (w < 0.6)).any() and (w > 0.9).any()


def test_central_differences_of_the_reference_agree_with_its_gradient():
    """L = <gs, scores>: (L(x + h) - L(x - h)) / 2h on 40 entries of the matches (h = 1e-5 px, relative to the largest derivative of
    its kind) and 40 of the models.  A model's entries span six orders (the perspective terms of a unit-norm H in pixels are 1e-6) and
    so do its derivatives, the other way: the step is 1e-6 of the entry and the derivative is taken times the entry (d L / d log |H_rq|),
    relative to the largest such product.  Such a step moves a point by 1e-6 x 640 px; the truncation is (h / l)^2 with l the length
    over which a weight changes, a pixel: 1e-10 for the matches, 4e-7 for the models.  The rounding is eps sum |gs s| / h =
    1e-16 x 1e2 / 1e-5 = 1e-9 against derivatives of the order of 1 for the matches, 1e-8 against products of the order of 100 for the
    models.  Bound: 1e-5."""
    c = S.case(*SMALL)
    gs = np.where(c["keep"], np.random.default_rng(2).normal(size=c["keep"].shape), 0.0)
    _, gm, gx = S.soft_score(c["m"], c["mask"], c["models"], c["keep"], c["thr"], S.BETA, gs)
    L0 = lambda p, m, mo: float((gs[p] * S.soft_score(m[None], None, mo[None], c["keep"][p:p + 1], c["thr"][p:p + 1], S.BETA)).sum())
    rng, worst = np.random.default_rng(3), 0.0
    use = np.argwhere(c["keep"] & S.usable_models(c["models"]) & (c["thr"] > 0)[:, None])
    scale = np.abs(gm * np.nan_to_num(c["models"])).max()
    for k in range(40):
        p, n, d, h = (0, 2)[rng.integers(2)], rng.integers(70), rng.integers(4), 1e-5
        a, b = c["m"][p].copy(), c["m"][p].copy()
        a[n, d] += h
        b[n, d] -= h
        worst = max(worst, abs((L0(p, a, c["models"][p]) - L0(p, b, c["models"][p])) / (2 * h) - gx[p, n, d]) / np.abs(gx).max())
        (p, j), r, q = use[rng.integers(len(use))], rng.integers(3), rng.integers(3)
        a, b = c["models"][p].copy(), c["models"][p].copy()
        h = 1e-6 * abs(a[j, r, q])
        a[j, r, q] += h
        b[j, r, q] -= h
        fd = (L0(p, c["m"][p], a) - L0(p, c["m"][p], b)) / (2 * h)
        worst = max(worst, abs(fd - gm[p, j, r, q]) * abs(c["models"][p, j, r, q]) / scale)
    print(f"central differences against the closed form: worst relative error {worst:.3g} (bound 1e-5)")
    assert np.abs(gx).max() > 0 and scale > 0 and worst <= 1e-5


def test_the_score_ignores_the_scale_and_the_sign_of_a_model():
    """score(c H) = score(H) for c = -3 and c = 0.5 (1e-12 of the scored points: the reference's own rounding), the gradient of c H is
    that of H over c, and by Euler's relation for a function of degree 0 the gradient is orthogonal to the model: sum H o grad_H = 0
    to 1e-9 of sum |H o grad_H|."""
    c = S.case(*SMALL)
    gs = np.ones(c["keep"].shape)
    s, gm, _ = S.soft_score(c["m"], None, c["models"], c["keep"], c["thr"], S.BETA, gs)
    use = c["keep"] & S.usable_models(c["models"]) & (c["thr"] > 0)[:, None]
    assert abs(s[0, S.SCALED] - s[0, S.NEAR]) <= 1e-12 * 70 and s[0, S.NEAR] > 10.0
    assert np.abs(gm[0, S.SCALED] * -3.0 - gm[0, S.NEAR]).max() <= 1e-9 * np.abs(gm[0, S.NEAR]).max()
    for k in (-3.0, 0.5):
        sk, gk, _ = S.soft_score(c["m"], None, k * c["models"], c["keep"], c["thr"], S.BETA, gs)
        assert np.abs(sk - s).max() <= 1e-12 * 70
        assert np.abs(gk[use] * k - gm[use]).max() <= 1e-9 * np.abs(gm[use]).max()
    dot, mag = (c["models"][use] * gm[use]).sum((-1, -2)), np.abs(c["models"][use] * gm[use]).sum((-1, -2))
    assert mag.max() > 0 and (np.abs(dot) <= 1e-9 * np.maximum(mag, mag.max() * 1e-6)).all()


def test_corner_errors_are_homography_errors_and_the_package_form_agrees():
    from differentiable_ransac_amd import loss
    c = S.case(*SMALL)
    use = c["keep"][0] & S.usable_models(c["models"][0])
    models, gt = torch.tensor(c["models"][:1, use]), torch.tensor(c["gt"][:1])
    want = loss.homography_errors(models, gt[:, None], S.SIZE)                       # [1,k], unclamped, plain norm
    ref = S.corner_errors(models, gt, S.SIZE, 1e9)
    got = loss.homography_corner_errors(models.clone().requires_grad_(True), gt, S.SIZE, 1e9)
    # (sqrt(d^2 + 1e-12) - d <= 1e-6 at d = 0 and 5e-13 / d elsewhere; the smallest distance here is that of GEN, 0)
    assert torch.allclose(ref, want, rtol=1e-12, atol=1e-6) and torch.allclose(got, ref, rtol=1e-12, atol=1e-11)
    assert float(want.max()) > 100.0 > float(want.min())                             # both sides of the default clamp
    assert torch.equal(loss.homography_corner_errors(models, gt, S.SIZE, 100.0), got.detach().clamp(max=100.0))
    # the long-double closed form that the reference's expected loss uses, against the torch form and its autograd
    tr = models.clone().requires_grad_(True)
    clamped = S.corner_errors(tr, gt, S.SIZE, 100.0)
    clamped.sum().backward()
    ell, dell = S.corner_errors_closed_form(models[0].numpy(), gt[0].numpy(), S.SIZE, 100.0)
    assert np.allclose(ell, clamped.detach().numpy()[0], rtol=1e-12, atol=1e-11) and (ell == 100.0).any() and (ell < 100.0).any()
    scale = np.abs(dell).max((1, 2), keepdims=True)                                  # (d / |d| of a 1e-3 px error: 1e-13 / 1e-3)
    assert (np.abs(dell - tr.grad.numpy()[0]) <= 1e-9 * scale).all() and scale.max() > 0
    # the sign and the scale of a model do not matter; a model that sends a corner through infinity takes max_loss and no gradient
    flipped = loss.homography_corner_errors(-3.0 * models, gt, S.SIZE, 1e9)
    assert torch.allclose(flipped, got.detach(), rtol=1e-12, atol=1e-11)
    bad = torch.stack([torch.tensor(c["models"][0, S.NEAR]), torch.eye(3, dtype=torch.float64)])[None]
    bad[0, 1, 2, 0] = -1.0 / 320.0                                                    # w = 1 - x / 320: the corners at x = 640 get w = -1
    bad.requires_grad_(True)
    ell = loss.homography_corner_errors(bad, gt, S.SIZE, 100.0)
    ell.sum().backward()
    ell = ell.detach()
    assert float(ell[0, 1]) == 100.0 and not bool(bad.grad[0, 1].any()) and bool(torch.isfinite(bad.grad).all())
    assert 0.0 < float(ell[0, 0]) < 1.0 and bool(bad.grad[0, 0].any())                # the model moved by 0.3 px
    assert float(S.corner_errors(bad.detach(), gt, S.SIZE, 100.0)[0, 1]) == 100.0


def test_header_declares_and_library_exports_and_checks_the_entries():
    declared = L.entries()
    assert not [s for s in SYMBOLS if s not in declared]
    text = lambda e: str(e).replace("float", "T").replace("double", "T").replace("f32", "").replace("f64", "")
    for n in ("soft_score", "soft_score_bwd"):
        assert text(declared[f"dr_homography_{n}_f32"]) == text(declared[f"dr_homography_{n}_f64"])
    lib = L.lib()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    for n in ("soft_score", "soft_score_bwd"):
        for sfx in ("f32", "f64"):
            assert getattr(lib, f"dr_homography_{n}_{sfx}").argtypes == getattr(lib, f"dr_registration_{n}_{sfx}").argtypes
    buf = (ctypes.c_char * 256)()
    for sfx in ("f32", "f64"):
        fwd, bwd = getattr(lib, "dr_homography_soft_score_" + sfx), getattr(lib, "dr_homography_soft_score_bwd_" + sfx)
        assert fwd(buf, None, buf, None, buf, 5.0, 1, 1, 1, None, None) == -1 and b"null" in lib.dr_last_error()
        assert fwd(buf, None, buf, None, buf, 5.0, 1, 0, 1, buf, None) == -1 and b"dr_homography_soft_score" in lib.dr_last_error()
        assert fwd(buf, None, buf, None, buf, 0.0, 1, 1, 1, buf, None) == -1 and b"beta" in lib.dr_last_error()
        assert fwd(buf, None, buf, None, buf, float("nan"), 1, 1, 1, buf, None) == -1 and b"beta" in lib.dr_last_error()
        assert bwd(buf, None, buf, None, buf, 5.0, None, 1, 1, 1, buf, None, None) == -1 and b"null" in lib.dr_last_error()
        assert bwd(buf, None, buf, None, buf, 5.0, buf, 1 << 12, 1 << 12, 1, buf, None, None) == -1 and b"2^22" in lib.dr_last_error()
        assert bwd(buf, None, buf, None, buf, -1.0, buf, 1, 1, 1, buf, buf, None) == -1 and b"beta" in lib.dr_last_error()


def test_the_wrapper_refuses_before_any_launch(monkeypatch):
    from differentiable_ransac_amd import ops
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    m, mo = torch.rand(2, 16, 4), torch.rand(2, 8, 3, 3)
    with pytest.raises(L.DransacError, match=r"\[P,N,4\]"):
        ops.homography_soft_score(torch.rand(2, 16, 5), mo, 3.0)                     # wrong width
    with pytest.raises(L.DransacError, match=r"\[P,N,4\]"):
        ops.homography_soft_score(torch.rand(16, 4), mo, 3.0)
    for bad in (torch.rand(2, 8, 4, 4), torch.rand(2, 8, 9), torch.rand(3, 8, 3, 3)):    # wrong model shape
        with pytest.raises(L.DransacError, match="models"):
            ops.homography_soft_score(m, bad, 3.0)
    with pytest.raises(L.DransacError, match="dtype"):
        ops.homography_soft_score(m, mo.double(), 3.0)                               # dtype mix
    with pytest.raises(L.DransacError, match="dtype"):
        ops.homography_soft_score(m.half(), mo.half(), 3.0)
    for beta in (0.0, -1.0, float("nan"), float("inf"), torch.tensor(5.0)):
        with pytest.raises(L.DransacError, match="beta"):
            ops.homography_soft_score(m, mo, 3.0, beta)
    with pytest.raises(L.DransacError, match="mask"):
        ops.homography_soft_score(m, mo, 3.0, mask=torch.ones(2, 15, dtype=torch.bool))
    with pytest.raises(L.DransacError, match="keep"):
        ops.homography_soft_score(m, mo, 3.0, keep=torch.ones(2, 9, dtype=torch.bool))
    with pytest.raises(L.DransacError, match="bool"):
        ops.homography_soft_score(m, mo, 3.0, keep=torch.ones(2, 8))
    with pytest.raises(L.DransacError):
        ops.homography_soft_score(m, mo, torch.full((3,), 3.0))                      # a threshold that is neither a float nor [P]
    with pytest.raises(L.DransacError, match="GPU tensors"):
        ops.homography_soft_score(m, mo, 3.0)                                        # CPU tensors
    assert calls == []


def test_the_loss_has_the_stated_defaults_and_its_arithmetic_matches_the_reference_on_stubbed_scores(monkeypatch):
    """HomographyExpectedLoss with ops.homography_soft_score replaced by the reference's scores (as a differentiable leaf), on the CPU
    in f64: the soft-max over the usable slots, a pair without a kept slot, the clamp.  Against the reference's pair-by-pair form."""
    import inspect

    from differentiable_ransac_amd import loss, ops
    sig = inspect.signature(loss.HomographyExpectedLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[3:]] == [("beta", 5.0), ("alpha", 100.0), ("max_loss", 100.0)]
    assert list(sig.parameters)[1:3] == ["threshold", "size"]
    assert list(inspect.signature(loss.HomographyExpectedLoss.forward).parameters) == ["self", "models", "matches", "gt_H", "keep", "mask"]
    assert issubclass(loss.HomographyExpectedLoss, loss._ExpectedLoss) and loss.HomographyExpectedLoss._tail_f64
    c = S.case(*SMALL)
    P, N, M = SMALL
    keep = c["keep"].copy()
    keep[2, : M // 2] = False
    thr = np.abs(c["thr"]) + 3.0 * (c["thr"] == 0)                                   # every pair scored here; pair 1 loses its slots:
    keep[1] = False                                                                  # a pair without a kept slot
    scores = torch.tensor(S.soft_score(c["m"], None, c["models"], keep, thr), requires_grad=True)
    seen = []
    monkeypatch.setattr(ops, "homography_soft_score", lambda *a, **k: seen.append(a) or scores)
    # (a ground truth that no slot equals: at a zero corner error the two forms' gradients are their own rounding over 1e-6 px)
    rng = np.random.default_rng(5)
    to, gt = torch.tensor(c["models"], requires_grad=True), torch.tensor(np.stack([S._moved(H, rng, 0.05) for H in c["gt"]]))
    crit = loss.HomographyExpectedLoss(thr, S.SIZE)
    got = crit(to, torch.tensor(c["m"]), gt, keep=torch.tensor(keep))
    got.backward()
    assert len(seen) == 1 and seen[0][3] == 5.0 and seen[0][4] is None               # (matches, models, threshold, beta, mask, keep)
    assert (crit.beta, crit.alpha, crit.max_loss, crit.size) == (5.0, 100.0, 100.0, S.SIZE)
    s2, t2 = scores.detach().clone().requires_grad_(True), torch.tensor(c["models"], requires_grad=True)
    want, per_pair, probs = S.expected_loss(t2, s2, N, gt, torch.tensor(keep), **S.LOSS)
    want.backward()
    assert abs(float(got.detach()) - float(want.detach())) <= 1e-12 * float(want.detach())
    assert torch.allclose(crit.per_pair, per_pair.detach(), rtol=1e-12, atol=0)
    assert torch.allclose(crit.probs, probs.detach(), rtol=1e-12, atol=1e-300) and float(crit.per_pair[1]) == 0.0
    assert torch.equal(crit.scores, scores.detach())
    tk = torch.tensor(keep)
    assert not bool(crit.probs[~tk].any()) and not bool(crit.probs[:, S.BAD].any()) and not bool(crit.probs[:, S.SINGULAR].any())
    assert torch.allclose(crit.probs.sum(1), torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64), atol=1e-12)
    g2 = torch.nan_to_num(t2.grad)
    assert torch.isfinite(to.grad).all() and torch.isfinite(scores.grad).all()
    assert torch.allclose(to.grad, g2, rtol=1e-9, atol=1e-12 * float(g2.abs().max()))
    assert torch.allclose(scores.grad, s2.grad, rtol=1e-9, atol=1e-12 * float(s2.grad.abs().max()))
    assert not bool(to.grad[1].any()) and not bool(scores.grad[1].any()) and not bool(to.grad[~tk].any())
    assert not bool(to.grad[:, S.BAD].any()) and not bool(to.grad[:, S.SINGULAR].any())
