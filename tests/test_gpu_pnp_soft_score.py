"""The differentiable soft-inlier score and the expected pose loss of the absolute-pose path (dr_pnp_soft_score, dr_pnp_soft_score_bwd;
ops.pnp_soft_score, loss.PnPExpectedLoss) against the f64 reference tests/pnp_soft_score_ref.py, in f32 and f64.

Protocol (the reference's docstring): per score, per model and per point the bound is TOL_FACTOR = 8 times what the reference measures
on itself -- its run on inputs as the kernel receives them (pnp_ref.as_kernel_input), its result rounded the same way, against its run
on the inputs the comparison uses -- with a floor of one eps of the type times the number of scored points (scores) or times the row's
largest entry (gradients), plus the own terms of the points within that deviation of the a = -40 cutoff or of z_c = 0.  No case and no
row is excluded.  The measured figures are printed next to each bound; docs/LOG.md records them.

Measured on one MI355X (worst error / bound over the cases (3,70,80), (2,300,260), (1,257,1100); docs/LOG.md, 29): scores f32
0.184 / 0.231 / 0.397, f64 0.281 / 0.625 / 0.375; grad_models f32 0.151 / 0.131 / 0.132, f64 0.402 / 0.249 / 0.32; grad_matches f32
0.175 / 0.14 / 0.142, f64 0.321 / 0.514 / 0.305; the loss's value at most 0.11, its gradients at most 0.51 (f32) and 0.64 (f64).  With
the type's own arithmetic for the residual and a plain sum the same checks stood at up to 2.3 (LOG 29 has the causes)."""
import functools

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import ops, synth
from differentiable_ransac_amd.loss import PnPExpectedLoss
from differentiable_ransac_amd.ransac import BatchedPnP
from tests import pnp_ref as R
from tests import pnp_soft_score_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.float64]
IDS = [f"P{c[0]}-N{c[1]}-M{c[2]}" for c in S.CASES]
LOSS = dict(alpha=100.0, trans_weight=100.0, max_loss=100.0)


def _name(dt):
    return "float32" if dt == torch.float32 else "float64"


def _dev(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dt is None else t.to(dt)


def _np(t):
    return t.detach().double().cpu().numpy()


def _bytes(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8)


def _given(a, name):
    """what a kernel of type `name` is handed, in f64: the f32 rounding, or the f64 values themselves"""
    return a.astype(np.float32).astype(np.float64) if name == "float32" else a


@functools.lru_cache(maxsize=None)
def _ref(cs, name):
    """the case, the upstream gradient, the reference on the originals, on the inputs as the kernel receives them, and the bands"""
    c = S.case(*cs)
    P, N, M = cs
    gs = _given(np.random.default_rng(M).normal(size=(P, M)), name)
    ref = S.soft_score(c["m"], c["mask"], c["models"], c["keep"], c["thr"], S.BETA, gs)
    mk, ok, tk, gk = (R.as_kernel_input(a, name, 3 + i) for i, a in enumerate((c["m"], c["models"], c["thr"], gs)))
    ok = np.where(np.isfinite(c["models"]), ok, c["models"])     # (one ulp below inf is a finite number: a non-finite entry stays)
    dev = tuple(R.as_kernel_input(a, name, 9) for a in S.soft_score(mk, c["mask"], ok, c["keep"], tk, S.BETA, gk))
    wa, wz = S.cutoff_widths(c["m"], mk, c["models"], ok, c["keep"], c["thr"], tk, S.BETA)
    band = S.bands(c["m"], c["mask"], c["models"], c["keep"], c["thr"], S.BETA, gs, wa, wz)
    n_scored = np.full(P, N) if c["mask"] is None else c["mask"].sum(1)
    return dict(c, gs=gs, ref=ref, dev=dev, band=band, n_scored=n_scored, kin=(mk, ok, tk))


def _tensors(c, dt):
    mask = None if c["mask"] is None else _dev(c["mask"])
    return _dev(c["m"], dt), _dev(c["models"], dt), _dev(c["keep"]), mask, _dev(c["thr"], dt)


def _upstream(c, dt):
    g = _dev(c["gs"], dt).clone()
    g[~_dev(c["keep"])] = float("nan")                        # a dropped slot's upstream gradient is never read
    return g


def _run(c, dt, with_matches=True):
    tm, tmo, tk, tmask, thr = _tensors(c, dt)
    tm.requires_grad_(with_matches)
    tmo.requires_grad_(True)
    scores = ops.pnp_soft_score(tm, tmo, thr, S.BETA, tmask, tk)
    scores.backward(_upstream(c, dt))
    return scores.detach(), tmo.grad, tm.grad


# ---- 1-3. forward, backward, repeatability --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cs", S.CASES, ids=IDS)
def test_scores_match_the_reference(cs, dt):
    name, (P, N, M) = _name(dt), cs
    c = _ref(cs, name)
    scores, _, _ = _run(c, dt)
    assert scores.shape == (P, M) and scores.dtype == dt
    floor = np.repeat(R.eps_of(name) * c["n_scored"], M)
    worst = S.compare(_np(scores), c["ref"][0], c["dev"][0], floor, c["band"][0].reshape(-1), f"soft score {cs} {name}")
    assert worst <= 1.0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cs", S.CASES, ids=IDS)
def test_gradients_match_the_reference(cs, dt):
    name, (P, N, M) = _name(dt), cs
    c = _ref(cs, name)
    scores, gm, gx = _run(c, dt)
    assert gm.shape == (P, M, 4, 4) and gx.shape == (P, N, 5) and gm.dtype == dt and gx.dtype == dt
    assert bool(torch.isfinite(gm).all()) and bool(torch.isfinite(gx).all())
    eps = R.eps_of(name)
    _, gm0, gx0 = c["ref"]
    wm = S.compare(_np(gm), gm0, c["dev"][1], eps * np.abs(gm0).reshape(P * M, -1).max(1), c["band"][1].reshape(-1),
                   f"soft score grad_models {cs} {name}")
    wx = S.compare(_np(gx), gx0, c["dev"][2], eps * np.abs(gx0).reshape(P * N, -1).max(1), c["band"][2].reshape(-1),
                   f"soft score grad_matches {cs} {name}")
    assert wm <= 1.0 and wx <= 1.0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cs", S.CASES, ids=IDS)
def test_zero_rules_repeatability_and_the_absent_match_gradient(cs, dt):
    name, (P, N, M) = _name(dt), cs
    c = _ref(cs, name)
    scores, gm, gx = _run(c, dt)
    s = _np(scores)
    assert not s[~c["keep"]].any() and not s[:, M - 1].any()               # dropped slots and the non-finite kept one: score exactly 0
    assert (s[:, M - 4] > 0.3 * c["n_scored"]).all()                      # the generating pose collects its 60 % inliers
    assert (s[:, M - 2] < s[:, M - 4]).all()                              # the pose with points behind the camera
    zero = torch.zeros((), device=DEV, dtype=dt)
    keep = _dev(c["keep"])
    assert torch.equal(_bytes(gm[~keep]), _bytes(zero.expand_as(gm[~keep])))                  # dropped slots: exact zeros, row 3 too
    assert torch.equal(_bytes(gm[:, M - 1]), _bytes(zero.expand_as(gm[:, M - 1])))            # the non-finite kept slot
    assert torch.equal(_bytes(gm[:, :, 3]), _bytes(zero.expand_as(gm[:, :, 3])))              # row 3 of every slot
    assert float(gm[:, M - 3].abs().max()) > 0.0 and float(gx.abs().max()) > 0.0
    if c["mask"] is not None:
        off = ~_dev(c["mask"])
        assert bool(off.any()) and torch.equal(_bytes(gx[off]), _bytes(zero.expand_as(gx[off])))      # unmasked points: exact zeros
    # repeatability: forward and backward, bit for bit
    again = _run(c, dt)
    assert all(torch.equal(_bytes(a), _bytes(b)) for a, b in zip((scores, gm, gx), again))
    # matches that need no gradient: none is returned, grad_models has the same bytes
    s1, gm1, gx1 = _run(c, dt, with_matches=False)
    assert gx1 is None and torch.equal(_bytes(gm1), _bytes(gm)) and torch.equal(_bytes(s1), _bytes(scores))


@pytest.mark.parametrize("dt", DTYPES)
def test_a_pair_without_a_threshold_scores_zero_and_passes_nothing(dt):
    c = _ref(S.CASES[0], _name(dt))
    tm, tmo, tk, tmask, thr = _tensors(c, dt)
    thr = thr.clone()
    thr[1] = 0.0
    tm.requires_grad_(True), tmo.requires_grad_(True)
    scores = ops.pnp_soft_score(tm, tmo, thr, S.BETA, tmask, tk)
    scores.backward(_upstream(c, dt))
    assert not bool(scores[1].any()) and not bool(tmo.grad[1].any()) and not bool(tm.grad[1].any())
    assert bool(scores[0].any()) and bool(tmo.grad[0].any()) and bool(tm.grad[2].any())


# ---- 4. the loss -----------------------------------------------------------------------------------------------------------------------
def _loss_f64(m, mask, models, keep, thr, poses):
    """tests/pnp_soft_score_ref.py's loss on numpy inputs -> (loss, per_pair, grad_models, grad_matches): the expected loss in f64 torch
    on the reference's scores, its gradient to the scores carried to models and matches by the reference's closed form (which the host
    tests hold against f64 autograd; plain f64 autograd through the residual carries the error described at pnp_soft_score_ref._grid)"""
    ts = torch.tensor(S.soft_score(m, mask, models, keep, thr, S.BETA), requires_grad=True)
    to, tk = torch.tensor(models, requires_grad=True), torch.tensor(keep)
    n = m.shape[1] if mask is None else mask.sum(1)
    loss, per_pair, _ = S.expected_loss(to, ts, n, torch.tensor(poses), tk, **LOSS)
    loss.backward()
    _, gm, gx = S.soft_score(m, mask, models, keep, thr, S.BETA, np.nan_to_num(ts.grad.numpy()))
    return float(loss.detach()), per_pair.detach().numpy(), to.grad.numpy() + gm, gx


@functools.lru_cache(maxsize=None)
def _loss_ref(cs, name):
    c = _ref(cs, name)
    mk, ok, tk = c["kin"]
    ref = _loss_f64(c["m"], c["mask"], c["models"], c["keep"], c["thr"], c["poses"])
    dev = _loss_f64(mk, c["mask"], ok, c["keep"], tk, R.as_kernel_input(c["poses"], name, 12))
    return ref, tuple(R.as_kernel_input(np.asarray(a), name, 13) for a in dev)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cs", S.CASES, ids=IDS)
def test_expected_loss_matches_the_reference(cs, dt):
    name, (P, N, M) = _name(dt), cs
    c = _ref(cs, name)
    assert not c["band"][0].any() and not c["band"][1].any() and not c["band"][2].any()      # no point of these cases sits in a band
    ref, dev = _loss_ref(cs, name)
    tm, tmo, tk, tmask, _ = _tensors(c, dt)
    tm.requires_grad_(True), tmo.requires_grad_(True)
    crit = PnPExpectedLoss(_dev(c["thr"], dt), S.BETA, **LOSS)
    loss = crit(tmo, tm, _dev(c["poses"], dt), keep=tk, mask=tmask)
    loss.backward()
    assert loss.dim() == 0 and crit.per_pair.shape == (P,) and crit.probs.shape == (P, M) and crit.scores.shape == (P, M)
    assert not bool(crit.probs[~tk].any()) and torch.allclose(crit.probs.sum(1), torch.ones(P, device=DEV, dtype=dt), atol=1e-5)
    eps = R.eps_of(name)
    # floors: a pair's value is a convex combination of errors <= max_loss, each rounded once; the mean likewise
    wv = S.compare(np.array([[float(loss)]]), np.array([[ref[0]]]), np.array([[dev[0]]]), np.array([eps * LOSS["max_loss"]]),
                   np.zeros(1), f"expected loss {cs} {name}: value {ref[0]:.6g}")
    wp = S.compare(_np(crit.per_pair)[:, None], ref[1][:, None], dev[1][:, None], np.full(P, eps * LOSS["max_loss"]), np.zeros(P),
                   f"expected loss {cs} {name}: per pair")
    wm = S.compare(_np(tmo.grad), ref[2], dev[2], eps * np.abs(ref[2]).reshape(P * M, -1).max(1), np.zeros(P * M),
                   f"expected loss {cs} {name}: grad_models")
    wx = S.compare(_np(tm.grad), ref[3], dev[3], eps * np.abs(ref[3]).reshape(P * N, -1).max(1), np.zeros(P * N),
                   f"expected loss {cs} {name}: grad_matches")
    assert bool(torch.isfinite(tmo.grad).all()) and bool(torch.isfinite(tm.grad).all())
    assert not bool(tmo.grad[~tk].any()) and not bool(tmo.grad[:, M - 1].any())
    assert max(wv, wp, wm, wx) <= 1.0


@pytest.mark.parametrize("dt", DTYPES)
def test_expected_loss_of_a_pair_without_a_kept_slot_is_zero(dt):
    c = _ref(S.CASES[0], _name(dt))
    tm, tmo, tk, tmask, thr = _tensors(c, dt)
    tk = tk.clone()
    tk[1] = False
    tm.requires_grad_(True), tmo.requires_grad_(True)
    crit = PnPExpectedLoss(thr, S.BETA, **LOSS)
    loss = crit(tmo, tm, _dev(c["poses"], dt), keep=tk)
    loss.backward()
    assert float(crit.per_pair[1]) == 0.0 and bool(torch.isfinite(loss))
    assert not bool(tmo.grad[1].any()) and not bool(tm.grad[1].any()) and bool(tm.grad[0].any())
    assert bool(torch.isfinite(tmo.grad).all()) and bool(torch.isfinite(tm.grad).all())


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------
def _close(a, b):
    # the gradients of the logits and of the matches leave through the sampler's backward, which adds with float atomics
    # (csrc/gumbel_topk.hip): its last bits depend on the order of arrival, as in tests/test_gpu_graphs.py
    return torch.allclose(a, b, rtol=1e-3, atol=1e-6 * float(a.abs().max()))


@pytest.mark.parametrize("dt", DTYPES)
def test_dsac_train_step(dt):
    P, N, B, iters = 2, 70, 16, 32
    sc = [R.scene(60 + p, N, 0.6) for p in range(P)]
    gumbels = [synth.gumbel_noise((P, B, N), seed=80 + r).to(DEV, dt) for r in range(iters // B)]
    gt = _dev(np.stack([s["pose"] for s in sc]), dt)

    def step():
        tm = _dev(np.stack([s["matches"] for s in sc]), dt).requires_grad_(True)
        logits = _dev(np.stack([np.where(s["inlier"], 1.0, -1.0) for s in sc]), dt).requires_grad_(True)
        drv = BatchedPnP(ransac_batch_size=B, threshold=R.THRESHOLD, max_iterations=iters, seed=3)
        out = drv.hypotheses(tm, logits, gumbels=gumbels)
        out["models"].retain_grad()
        crit = PnPExpectedLoss(R.THRESHOLD)
        loss = crit(out["models"], tm, gt, keep=out["keep"])
        loss.backward()
        return loss.detach(), out["models"].detach(), out["models"].grad, logits.grad, tm.grad, crit

    loss, models, gmod, gl, gx, crit = step()
    assert models.shape == (P, 2 * 4 * B, 4, 4) and bool(torch.isfinite(loss)) and 0.0 <= float(loss) <= crit.max_loss
    for g in (gl, gx):
        assert g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any())
    print(f"dsac step {_name(dt)}: loss {float(loss):.4f}, per pair {[f'{float(x):.3g}' for x in crit.per_pair]}, |grad logits| "
          f"{float(gl.abs().sum()):.3g}, |grad matches| {float(gx.abs().sum()):.3g}")
    loss2, models2, gmod2, gl2, gx2, _ = step()
    assert torch.equal(_bytes(loss), _bytes(loss2)) and torch.equal(_bytes(models), _bytes(models2))
    assert torch.equal(_bytes(gmod), _bytes(gmod2))            # the loss, the hypotheses, the score's and the loss's gradient: the same bytes
    assert _close(gl, gl2) and _close(gx, gx2)


# ---- 6. capture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_forward_and_backward_replay_from_a_graph(dev, dt):
    from differentiable_ransac_amd.graphs import GraphedStep
    c = S.case(2, 70, 80)
    tm, tmo, tk, _, thr = _tensors(c, dt)
    g_up = torch.where(tk, _dev(np.random.default_rng(5).normal(size=(2, 80)), dt), torch.zeros((), device=DEV, dtype=dt))
    tm.requires_grad_(True), tmo.requires_grad_(True)

    def fn():
        tm.grad = tmo.grad = None
        scores = ops.pnp_soft_score(tm, tmo, thr, S.BETA, None, tk)
        scores.backward(g_up)
        return scores.detach(), tmo.grad, tm.grad

    want = [t.clone() for t in fn()]
    step = GraphedStep(fn, warmup=1)
    got = [t.clone() for t in step()]
    assert all(torch.equal(_bytes(a), _bytes(b)) for a, b in zip(want, got))
    assert bool(want[1].any()) and bool(want[2].any())
