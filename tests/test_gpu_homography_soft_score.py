"""The differentiable soft-inlier score and the expected corner loss of the homography path (dr_homography_soft_score,
dr_homography_soft_score_bwd; ops.homography_soft_score, loss.HomographyExpectedLoss) against the reference
tests/homography_soft_score_ref.py, in f32 and f64.

Protocol (tests/test_gpu_registration_soft_score.py's): per score, per model and per point the bound is TOL_FACTOR = 8 times what the
reference measures on itself -- its run on inputs as the kernel receives them (pnp_ref.as_kernel_input), its result rounded the same
way, against its run on the inputs the comparison uses -- with a floor of one eps of the type times the number of scored points
(scores) or times the row's largest entry (gradients), plus the own terms of the points within that deviation of the a = -40 cutoff
or of y_w = 0, z_w = 0.  No case and no row is excluded.  The measured figures are printed next to each bound; docs/LOG.md records
them.

Measured on one MI355X (worst error / bound over the cases (3,70,80), (2,300,260), (1,257,550); docs/LOG.md, 34): scores f32
0.361 / 0.189 / 0.563, f64 0.125 / 0.125 / 0.0625; grad_models f32 0.14 / 0.132 / 0.211, f64 0.531 / 0.015 / 0.375; grad_matches f32
0.129 / 0.133 / 0.147, f64 0.003 / 0.004 / 0.010; the loss's value and per-pair values at most 0.125; its grad_models f32 0.135 /
0.138 / 0.515, f64 0.094 / 0.013 / 0.037; its grad_matches f32 0.133 / 0.13 / 0.152, f64 0.026 / 0.004 / 0.005.  With the residual
in the type's own arithmetic (the loss kernel's treatment) the scores stood at 1.96 (f32, first case) and 1.12 / 1.69 / 1.5 (f64),
and the f64 grad_models at 13.9 / 0.39 / 38.3; with the loss's corner difference in plain f64 its f64 grad_models stood at 4.37 on
the first case (LOG 34)."""
import functools

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import ops
from differentiable_ransac_amd.loss import HomographyExpectedLoss
from differentiable_ransac_amd.ransac import BatchedHomography
from tests import homography_ref as G
from tests import homography_soft_score_ref as S
from tests import pnp_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.float64]
IDS = [f"P{c[0]}-N{c[1]}-M{c[2]}" for c in S.CASES]
LOSS = S.LOSS


def _name(dt):
    return "float32" if dt == torch.float32 else "float64"


def _dev(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dt is None else t.to(dt)


def _np(t):
    return t.detach().double().cpu().numpy()


def _bytes(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8)


def _all_zero_bytes(t):
    return t.numel() > 0 and not bool(t.any()) and not bool(torch.signbit(t).any())      # (+0.0 everywhere, no -0.0)


def _given(a, name):
    """what a kernel of type `name` is handed, in f64: the f32 rounding, or the f64 values themselves"""
    return a.astype(np.float32).astype(np.float64) if name == "float32" else a


def _kernel_models(models, name, seed):
    """the models as a kernel of type `name` receives them: a non-finite entry stays (one ulp below inf is a finite number), and so
    does the singular slot (one ulp off a zero is not a zero row)"""
    ok = np.where(np.isfinite(models), R.as_kernel_input(models, name, seed), models)
    ok[:, S.SINGULAR] = models[:, S.SINGULAR]
    return ok


@functools.lru_cache(maxsize=None)
def _ref(cs, name):
    """the case, the upstream gradient, the reference on the originals, on the inputs as the kernel receives them, and the bands"""
    c = S.case(*cs)
    P, N, M = cs
    gs = _given(np.random.default_rng(M).normal(size=(P, M)), name)
    ref = S.soft_score(c["m"], c["mask"], c["models"], c["keep"], c["thr"], S.BETA, gs)
    mk, tk, gk = (R.as_kernel_input(a, name, 3 + i) for i, a in enumerate((c["m"], c["thr"], gs)))
    ok = _kernel_models(c["models"], name, 6)
    tk = np.where(c["thr"] > 0, tk, c["thr"])                     # (a threshold of 0 stays 0)
    dev = tuple(R.as_kernel_input(a, name, 9) for a in S.soft_score(mk, c["mask"], ok, c["keep"], tk, S.BETA, gk))
    widths = S.cutoff_widths(c["m"], mk, c["models"], ok, c["keep"], c["thr"], tk, S.BETA)
    band = S.bands(c["m"], c["mask"], c["models"], c["keep"], c["thr"], S.BETA, gs, *widths)
    n_scored = np.full(P, N) if c["mask"] is None else c["mask"].sum(1)
    return dict(c, gs=gs, ref=ref, dev=dev, band=band, widths=widths, n_scored=n_scored, kin=(mk, ok, tk))


def _tensors(c, dt):
    mask = None if c["mask"] is None else _dev(c["mask"])
    return _dev(c["m"], dt), _dev(c["models"], dt), _dev(c["keep"]), mask, _dev(c["thr"], dt)


def _upstream(c, dt):
    g = _dev(c["gs"], dt).clone()
    g[~_dev(c["keep"])] = float("nan")                        # a dropped slot's upstream gradient is never read
    return g


@functools.lru_cache(maxsize=None)
def _run_once(cs, dt):
    return _run(_ref(cs, _name(dt)), dt)


def _run(c, dt, with_matches=True):
    tm, tmo, tk, tmask, thr = _tensors(c, dt)
    tm.requires_grad_(with_matches)
    tmo.requires_grad_(True)
    scores = ops.homography_soft_score(tm, tmo, thr, S.BETA, tmask, tk)
    scores.backward(_upstream(c, dt))
    return scores.detach(), tmo.grad, tm.grad


def _bounds(c, cs, name):
    """per score, per model row, per point row: max(TOL_FACTOR x measured, floor) + band, as `compare` forms it"""
    P, N, M = cs
    eps = R.eps_of(name)
    out = []
    for k, rows, floor in ((0, P * M, np.repeat(eps * c["n_scored"], M)), (1, P * M, None), (2, P * N, None)):
        ref, dev = (np.asarray(a, np.float64).reshape(rows, -1) for a in (c["ref"][k], c["dev"][k]))
        fl = eps * np.abs(ref).max(1) if floor is None else floor
        out.append(np.maximum(R.TOL_FACTOR * np.abs(dev - ref).max(1), fl) + c["band"][k].reshape(-1))
    return out


# ---- 1-2. forward and backward against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cs", S.CASES, ids=IDS)
def test_scores_match_the_reference(cs, dt):
    name, (P, N, M) = _name(dt), cs
    c = _ref(cs, name)
    scores, _, _ = _run_once(cs, dt)
    assert scores.shape == (P, M) and scores.dtype == dt
    floor = np.repeat(R.eps_of(name) * c["n_scored"], M)
    worst = S.compare(_np(scores), c["ref"][0], c["dev"][0], floor, c["band"][0].reshape(-1), f"homography soft score {cs} {name}")
    assert worst <= 1.0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cs", S.CASES, ids=IDS)
def test_gradients_match_the_reference(cs, dt):
    name, (P, N, M) = _name(dt), cs
    c = _ref(cs, name)
    scores, gm, gx = _run_once(cs, dt)
    assert gm.shape == (P, M, 3, 3) and gx.shape == (P, N, 4) and gm.dtype == dt and gx.dtype == dt
    assert bool(torch.isfinite(gm).all()) and bool(torch.isfinite(gx).all())
    eps = R.eps_of(name)
    _, gm0, gx0 = c["ref"]
    wm = S.compare(_np(gm), gm0, c["dev"][1], eps * np.abs(gm0).reshape(P * M, -1).max(1), c["band"][1].reshape(-1),
                   f"homography soft score grad_models {cs} {name}")
    wx = S.compare(_np(gx), gx0, c["dev"][2], eps * np.abs(gx0).reshape(P * N, -1).max(1), c["band"][2].reshape(-1),
                   f"homography soft score grad_matches {cs} {name}")
    assert wm <= 1.0 and wx <= 1.0


# ---- 3-7. exact zeros, the scaled twin, the size of a score, repeatability, the skipped launch --------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cs", S.CASES, ids=IDS)
def test_zero_rules_the_scaled_twin_repeatability_and_the_absent_match_gradient(cs, dt):
    name, (P, N, M) = _name(dt), cs
    c = _ref(cs, name)
    scores, gm, gx = _run_once(cs, dt)                        # (the upstream gradient of every dropped slot is NaN)
    keep = _dev(c["keep"])
    assert bool((~keep).any()) and bool(keep[:, S.BAD].all()) and bool(keep[:, S.SINGULAR].all())
    for t in (scores[~keep], gm[~keep], scores[:, S.BAD], gm[:, S.BAD], scores[:, S.SINGULAR], gm[:, S.SINGULAR]):
        assert _all_zero_bytes(t)                             # dropped slots, the non-finite kept one, the singular kept one
    if P > 1:                                                 # the pair without a threshold: nothing scored, nothing passed
        assert float(c["thr"][1]) == 0.0
        for t in (scores[1], gm[1], gx[1]):
            assert _all_zero_bytes(t)
    live = [p for p in range(P) if c["thr"][p] > 0]
    s, g = _np(scores), _np(gm)
    bs, bm, _ = (b.reshape(P, -1) for b in _bounds(c, cs, name))
    for p in live:
        assert s[p, S.GEN] > 0.45 * c["n_scored"][p]          # the generating H collects its 60 % inliers at weights above 0.9
        assert 0.0 <= s[p, S.FAR] < 0.01 * c["n_scored"][p]   # three thresholds away: the inliers sit at the cutoff, w < e^-34
        assert float(gm[p, S.NEAR].abs().max()) > 0.0 and float(gx[p].abs().max()) > 0.0
        # -3 H scores as H does and its gradient is that of H over -3: both within their bounds of the reference, in which they agree
        assert abs(s[p, S.SCALED] - s[p, S.NEAR]) <= bs[p, S.SCALED] + bs[p, S.NEAR]
        us, un = abs(c["gs"][p, S.SCALED]), abs(c["gs"][p, S.NEAR])      # (each row carries its own upstream gradient)
        assert np.abs(g[p, S.SCALED] * -3.0 / c["gs"][p, S.SCALED] - g[p, S.NEAR] / c["gs"][p, S.NEAR]).max() \
            <= 3.0 * bm[p, S.SCALED] / us + bm[p, S.NEAR] / un
        assert s[p, S.NEAR] > 0.45 * c["n_scored"][p]
    if c["mask"] is not None:
        off = ~_dev(c["mask"])
        assert bool(off.any()) and _all_zero_bytes(gx[off])   # unmasked points: exact zeros
    # repeatability: forward and backward, bit for bit
    again = _run(c, dt)
    assert all(torch.equal(_bytes(a), _bytes(b)) for a, b in zip((scores, gm, gx), again))
    # matches that need no gradient: none is returned, grad_models has the same bytes
    s1, gm1, gx1 = _run(c, dt, with_matches=False)
    assert gx1 is None and torch.equal(_bytes(gm1), _bytes(gm)) and torch.equal(_bytes(s1), _bytes(scores))


# ---- 8-9. a NaN threshold, no second derivative -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_nan_thresholds_nan_models_in_dropped_slots_and_second_derivatives(dt):
    c = _ref(S.CASES[0], _name(dt))
    tm, tmo, tk, tmask, thr = _tensors(c, dt)
    thr = thr.clone()
    thr[2] = float("nan")
    assert bool(torch.isnan(tmo[~tk]).all())                  # every dropped slot holds NaN
    tm.requires_grad_(True), tmo.requires_grad_(True)
    scores = ops.homography_soft_score(tm, tmo, thr, S.BETA, tmask, tk)
    (gm, gx) = torch.autograd.grad(scores, (tmo, tm), _upstream(c, dt), create_graph=True)
    for t in (scores[1:], gm[1:], gx[1:]):
        assert _all_zero_bytes(t)
    assert bool(scores[0].any()) and bool(gm[0].any()) and bool(gx[0].any())
    assert bool(torch.isfinite(gm).all()) and bool(torch.isfinite(gx).all())
    with pytest.raises(RuntimeError):                         # the backward is a kernel result: no second derivative
        gm.sum().backward()


# ---- 10. the loss -------------------------------------------------------------------------------------------------------------------------
def _loss_f64(m, mask, models, keep, thr, gt, name=None):
    """the reference's loss on numpy inputs -> (loss, per_pair, grad_models, grad_matches): the expected loss in f64 torch on the
    reference's scores, its gradient to the scores carried to models and matches by the reference's closed form.  With `name` (the
    run on inputs as the kernels receive them) the scores enter the loss as the op returns them, a tensor of that type, and the
    upstream gradient d loss / d scores is handed to the closed form as the backward kernel receives it."""
    scores = S.soft_score(m, mask, models, keep, thr, S.BETA)
    ts = torch.tensor(scores if name is None else R.as_kernel_input(scores, name, 15), requires_grad=True)
    to, tk = torch.tensor(models, requires_grad=True), torch.tensor(keep)
    n = m.shape[1] if mask is None else mask.sum(1)
    loss, per_pair, _ = S.expected_loss(to, ts, n, torch.tensor(gt), tk, **LOSS)
    loss.backward()
    up = np.nan_to_num(ts.grad.numpy())
    _, gm, gx = S.soft_score(m, mask, models, keep, thr, S.BETA, up if name is None else R.as_kernel_input(up, name, 14))
    return float(loss.detach()), per_pair.detach().numpy(), np.nan_to_num(to.grad.numpy()) + gm, gx


@functools.lru_cache(maxsize=None)
def _loss_ref(cs, name):
    c = _ref(cs, name)
    mk, ok, tk = c["kin"]
    ref = _loss_f64(c["m"], c["mask"], c["models"], c["keep"], c["thr"], c["gt"])
    dev = _loss_f64(mk, c["mask"], ok, c["keep"], tk, R.as_kernel_input(c["gt"], name, 12), name)
    return ref, tuple(R.as_kernel_input(np.asarray(a), name, 13) for a in dev)


@functools.lru_cache(maxsize=None)
def _loss_grad_scores(cs, name):
    """d loss / d scores [P,M] of the reference on the case"""
    c = _ref(cs, name)
    ts = torch.tensor(S.soft_score(c["m"], c["mask"], c["models"], c["keep"], c["thr"], S.BETA), requires_grad=True)
    n = cs[1] if c["mask"] is None else c["mask"].sum(1)
    S.expected_loss(torch.tensor(c["models"]), ts, n, torch.tensor(c["gt"]), torch.tensor(c["keep"]), **LOSS)[0].backward()
    return ts.grad.numpy()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cs", S.CASES, ids=IDS)
def test_expected_loss_matches_the_reference(cs, dt):
    name, (P, N, M) = _name(dt), cs
    c = _ref(cs, name)
    ref, dev = _loss_ref(cs, name)
    tm, tmo, tk, tmask, _ = _tensors(c, dt)
    tm.requires_grad_(True), tmo.requires_grad_(True)
    crit = HomographyExpectedLoss(_dev(c["thr"], dt), S.SIZE, S.BETA, **LOSS)
    loss = crit(tmo, tm, _dev(c["gt"], dt), keep=tk, mask=tmask)
    loss.backward()
    assert loss.dim() == 0 and crit.per_pair.shape == (P,) and crit.probs.shape == (P, M) and crit.scores.shape == (P, M)
    usable = tk & _dev(S.usable_models(c["models"]))
    assert not bool(crit.probs[~usable].any()) and torch.allclose(crit.probs.sum(1), torch.ones(P, device=DEV, dtype=dt), atol=1e-5)
    eps = R.eps_of(name)
    # a point in a band moves a score by at most its own weight, e^-40 next to scores of tens: nothing of that reaches the soft-max
    # in either type.  Its gradient terms enter the rows' bounds with the loss's own upstream gradient, d loss / d score
    _, bm, bx = S.bands(c["m"], c["mask"], c["models"], c["keep"], c["thr"], S.BETA, np.nan_to_num(_loss_grad_scores(cs, name)),
                        *c["widths"])
    bm, bx = bm.reshape(-1), bx.reshape(-1)
    # floors: a pair's value is a convex combination of errors <= max_loss, each rounded once; the mean likewise
    wv = S.compare(np.array([[float(loss.detach())]]), np.array([[ref[0]]]), np.array([[dev[0]]]), np.array([eps * LOSS["max_loss"]]),
                   np.zeros(1), f"homography expected loss {cs} {name}: value {ref[0]:.6g}")
    wp = S.compare(_np(crit.per_pair)[:, None], ref[1][:, None], dev[1][:, None], np.full(P, eps * LOSS["max_loss"]), np.zeros(P),
                   f"homography expected loss {cs} {name}: per pair")
    wm = S.compare(_np(tmo.grad), ref[2], dev[2], eps * np.abs(ref[2]).reshape(P * M, -1).max(1), bm,
                   f"homography expected loss {cs} {name}: grad_models")
    wx = S.compare(_np(tm.grad), ref[3], dev[3], eps * np.abs(ref[3]).reshape(P * N, -1).max(1), bx,
                   f"homography expected loss {cs} {name}: grad_matches")
    assert bool(torch.isfinite(tmo.grad).all()) and bool(torch.isfinite(tm.grad).all())
    assert not bool(tmo.grad[~usable].any())
    assert max(wv, wp, wm, wx) <= 1.0


@pytest.mark.parametrize("dt", DTYPES)
def test_expected_loss_of_a_pair_without_a_kept_slot_is_zero(dt):
    c = _ref(S.CASES[0], _name(dt))
    tm, tmo, tk, tmask, thr = _tensors(c, dt)
    tk = tk.clone()
    tk[2] = False
    tm.requires_grad_(True), tmo.requires_grad_(True)
    crit = HomographyExpectedLoss(thr, S.SIZE)
    loss = crit(tmo, tm, _dev(c["gt"], dt), keep=tk)
    loss.backward()
    assert float(crit.per_pair[2]) == 0.0 and bool(torch.isfinite(loss)) and crit.max_loss == 100.0
    assert not bool(tmo.grad[2].any()) and not bool(tm.grad[2].any()) and bool(tm.grad[0].any())
    # pair 1 has no threshold: its scores are 0, the soft-max is uniform over its usable slots, the gradient comes from the corner errors
    usable = tk[1] & _dev(S.usable_models(c["models"][1]))
    pr = crit.probs[1][usable]
    assert not bool(crit.scores[1].any()) and not bool(tm.grad[1].any()) and bool(tmo.grad[1].any())
    assert torch.allclose(pr, torch.full_like(pr, 1.0 / int(usable.sum())), rtol=1e-6, atol=0) and not bool(crit.probs[1][~usable].any())
    assert bool(torch.isfinite(tmo.grad).all()) and bool(torch.isfinite(tm.grad).all())


# ---- 11. end to end -----------------------------------------------------------------------------------------------------------------------
def _one_ulp(a, name, seed):
    """every finite entry one ulp OF THE TYPE up or down, in f64: the driver's outputs are exact in the type, so rounding them to it
    measures nothing; the smallest change the format can express is what as_kernel_input makes for f64, here for either type"""
    t = np.float32 if name == "float32" else np.float64
    a = np.asarray(a, np.float64).astype(t)
    up = np.random.default_rng(seed).random(a.shape) < 0.5
    return np.where(up, np.nextafter(a, t(np.inf)), np.nextafter(a, t(-np.inf))).astype(np.float64)


@pytest.mark.parametrize("dt", DTYPES)
def test_dsac_train_step(dt):
    name, P, N = _name(dt), 2, 200
    pairs = [G.scene(70 + p, N, 0.6) for p in range(P)]
    gt = _dev(np.stack([s["H"] for s in pairs]), dt)
    tm = _dev(np.stack([s["matches"] for s in pairs]), dt).requires_grad_()
    logits = torch.zeros(P, N, device=DEV, dtype=dt).requires_grad_()
    drv = BatchedHomography(ransac_batch_size=64, max_iterations=128, threshold=3.0, train=True)
    out = drv(tm, logits)
    crit = HomographyExpectedLoss(3.0, S.SIZE)
    loss = crit(out["models"], tm, gt, keep=out["keep"])
    loss.backward()
    assert out["models"].shape == (P, 128, 3, 3) and bool(torch.isfinite(loss)) and 0.0 <= float(loss) <= crit.max_loss
    for g in (logits.grad, tm.grad):
        assert g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any())
    # on the models the driver returned, the loss is the reference's: the bound is 8 x what one ulp of the type in every input moves
    # the reference's loss, with the floor of one eps of max_loss (a convex combination of errors <= max_loss)
    m, mo, kp, gts = _np(tm), _np(out["models"]), out["keep"].cpu().numpy(), _np(gt)
    thr = 3.0

    def ref_loss(m, mo, gts, thr=thr):
        ts = torch.tensor(S.soft_score(m, None, mo, kp, thr, S.BETA))
        return S.expected_loss(torch.tensor(mo), ts, N, torch.tensor(gts), torch.tensor(kp), **LOSS)[:2]
    want, want_pp = ref_loss(m, mo, gts)
    moved, moved_pp = ref_loss(_one_ulp(m, name, 1), np.where(np.isfinite(mo), _one_ulp(mo, name, 2), mo), _one_ulp(gts, name, 3),
                                float(_one_ulp(thr, name, 4)))
    eps = R.eps_of(name)
    wv = S.compare(np.array([[float(loss)]]), np.array([[float(want)]]), np.array([[float(moved)]]), np.array([eps * LOSS["max_loss"]]),
                   np.zeros(1), f"homography dsac step {name}: loss {float(want):.6g}")
    wp = S.compare(_np(crit.per_pair)[:, None], want_pp.numpy()[:, None], moved_pp.numpy()[:, None], np.full(P, eps * LOSS["max_loss"]),
                   np.zeros(P), f"homography dsac step {name}: per pair")
    print(f"homography dsac step {name}: loss {float(loss):.4f}, kept {int(out['keep'].sum())} of {P * 128}, |grad logits| "
          f"{float(logits.grad.abs().sum()):.3g}, |grad matches| {float(tm.grad.abs().sum()):.3g}")
    assert max(wv, wp) <= 1.0
