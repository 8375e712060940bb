"""The trainable absolute-pose path (dr_p3p, dr_p3p_bwd, dr_pnp_loss_*, dr_pnp_gt_mask; ops.p3p, loss.PnPLoss, BatchedPnP.hypotheses)
against the f64 references tests/pnp_ref.py and tests/pnp_grad_ref.py, in f32 and f64.

Tolerances follow tests/test_gpu_pnp.py: TOL_FACTOR = 8 times a figure the reference measures on itself -- its run on inputs as the
kernel receives them (pnp_ref.as_kernel_input), its result rounded the same way, against its run on the inputs the comparison uses --
never anything a kernel returned.  For the P3P reverse pass the figure is taken per sample (the conditioning of a minimal sample varies
by orders of magnitude across a case), with a floor of one eps of the type on the sample's largest derivative: the kernel rounds its
result to the type once.  A point whose d2 / thr^2 lies within the band of 1 that the reference's own d2 deviation spans may be live on
one side and truncated on the other: it moves a sum by at most the band's width and a gradient by its own term, which the reference
adds to the bound (pnp_grad_ref.pnp_loss_bands).  The measured figures are printed next to each bound; docs/LOG.md records them."""
import functools

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from differentiable_ransac_amd import ops
from differentiable_ransac_amd.loss import PnPLoss
from differentiable_ransac_amd.ransac import BatchedPnP
from tests import pnp_grad_ref as G
from tests import pnp_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.float64]
THR = R.THRESHOLD
THR_PAIRS = (1.0, 0.8, 1.25)          # the per-pair thresholds of the loss tests, in units of THR
F = R.TOL_FACTOR
SENTINEL = 777.0
KEYS = {"model", "mask", "score", "inliers", "iterations"}
ptr, stream = L.ptr, L.stream


def _name(dt):
    return "float32" if dt == torch.float32 else "float64"


def _dev(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dt is None else t.to(dt)


def _np(t):
    return t.detach().double().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()


def _bytes(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8)


def _given(a, name):
    """what a kernel of type `name` is handed, in f64: the f32 rounding, or the f64 values themselves"""
    return a.astype(np.float32).astype(np.float64) if name == "float32" else a


def _samples(tm, ti):
    """matches [P,N,5], idx [P,B,3] -> matches[idx] [P,B,3,5]"""
    return tm[torch.arange(tm.shape[0], device=tm.device)[:, None, None], ti.long()].contiguous()


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", R.GPU_CASES, ids=[f"P{c[0]}-N{c[1]}-B{c[2]}" for c in R.GPU_CASES])
def test_p3p_on_explicit_samples_equals_the_gather_form(case, dt):
    m, idx = R.solver_case(*case)
    tm, ti = _dev(m, dt), _dev(idx)
    models, keep = ops.p3p(_samples(tm, ti))
    want, valid = ops.p3p_gather(tm, ti)
    P, _, B = case
    assert models.shape == (P, B, 4, 4, 4) and keep.shape == (P, B, 4) and keep.dtype == torch.bool and models.dtype == dt
    assert torch.equal(_bytes(models.reshape(P, 4 * B, 4, 4)), _bytes(want)) and torch.equal(keep.reshape(P, 4 * B), valid)
    assert bool(valid.any())


# ---- 2. backward -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vjp_ref(case, name):
    """the case, the upstream gradients, per pair the reference's derivative on the inputs the kernel is given with the samples that
    may be compared, and per sample the measured figure: the reference on as_kernel_input inputs, its result rounded the same way,
    against that run"""
    m, idx = R.solver_case(*case)
    P, _, B = case
    up = _given(np.random.default_rng(case[2]).normal(size=(P, 4 * B, 4, 4)), name)
    mg, mk, uk = _given(m, name), R.as_kernel_input(m, name, 1), R.as_kernel_input(up, name, 8)
    ref, skipped = [], 0
    for p in range(P):
        g0, va, infos = G.p3p_vjp_slots(mg[p], idx[p], up[p])
        g1, va1, infos1 = G.p3p_vjp_slots(mk[p], idx[p], uk[p])
        g1 = R.as_kernel_input(g1, name, 9)
        keep = np.array([R.comparable(a) and R.comparable(b) for a, b in zip(infos, infos1)])
        skipped += int((~keep).sum())
        assert np.array_equal(va.reshape(B, 4)[keep], va1.reshape(B, 4)[keep])       # (the separation rule keeps the reference's own count stable)
        fig = np.abs(g1 - g0).reshape(B, -1).max(1)
        floor = R.eps_of(name) * np.abs(g0).reshape(B, -1).max(1)
        ref.append((g0, va, keep, fig, floor))
    return m, idx, up, ref, skipped


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", R.GPU_CASES, ids=[f"P{c[0]}-N{c[1]}-B{c[2]}" for c in R.GPU_CASES])
def test_p3p_backward_matches_the_reference(case, dt):
    """Both sides evaluate the derivative at the ROOT of the sample's reprojection equations: the reference through
    pnp_grad_ref.root_pose, the kernel through its Gauss-Newton step (pnp.hip, 1b).  At the poses as P3P returns them neither meets
    this bound on ill-conditioned samples in f64 (docs/LOG.md, 28).  Measured worst error / bound: 0.04-0.06 in f32, 0.10 / 0.68 / 0.58
    in f64."""
    name = _name(dt)
    m, idx, up, ref, skipped = _vjp_ref(case, name)
    P, _, B = case
    assert skipped <= R.EXCLUDED_MAX * P * B, (skipped, P * B)
    samples = _samples(_dev(m, dt), _dev(idx)).requires_grad_(True)
    models, keep = ops.p3p(samples)
    g_up = _dev(up, dt).reshape(P, B, 4, 4, 4).clone()
    g_up[~keep] = float("nan")                                 # an invalid slot's gradient is never read
    g_up[..., 3, :] = 7e30                                     # nor is row 3 of any
    (got,) = torch.autograd.grad(models, samples, g_up, retain_graph=True)
    (again,) = torch.autograd.grad(models, samples, g_up)
    assert torch.equal(_bytes(got), _bytes(again))             # a repeated backward: the same bytes
    assert got.shape == samples.shape and got.dtype == dt and bool(torch.isfinite(got).all())
    gk, vk = _np(got), keep.cpu().numpy().reshape(P, 4 * B)
    worst = (0.0, 0.0, 0.0, 0.0)
    for p, (g0, va, ok, fig, floor) in enumerate(ref):
        for b in np.flatnonzero(ok):
            assert np.array_equal(vk[p, 4 * b:4 * b + 4], va[4 * b:4 * b + 4]), (p, b)
            err, bound = float(np.abs(gk[p, b] - g0[b]).max()), F * max(fig[b], floor[b])
            if bound > 0.0 and err / bound >= worst[0]:
                worst = (err / bound, err, fig[b], bound)
            assert err <= bound, (p, b, err, fig[b], floor[b], float(np.abs(g0[b]).max()))
    print(f"p3p backward {case} {name}: worst error / bound {worst[0]:.3g} (error {worst[1]:.3g}, measured {worst[2]:.3g}, bound "
          f"{worst[3]:.3g}); left out {skipped} of {P * B}")


@pytest.mark.parametrize("dt", DTYPES)
def test_p3p_backward_zero_rules(dt):
    m = R.scene(2, 16, 1.0)["matches"].copy()
    m[2, :3] = m[0, :3] + 2.0 * (m[1, :3] - m[0, :3])        # rows 0, 1, 2: collinear world points
    m[4, 3:] = m[3, 3:]                                      # rows 3, 4: coincident bearings
    idx = np.array([[[0, 1, 2], [5, 6, 6], [3, 4, 7], [8, 9, 10]]], np.int32)
    samples = _samples(_dev(m[None], dt), _dev(idx)).requires_grad_(True)
    models, keep = ops.p3p(samples)
    assert not bool(keep[0, :3].any()) and bool(keep[0, 3].any())
    up = _dev(np.random.default_rng(4).normal(size=(1, 4, 4, 4, 4)), dt)
    (g,) = torch.autograd.grad(models, samples, up)
    assert not bool(g[0, :3].any())                          # exact zeros: collinear, a repeated index, coincident bearings
    assert bool(torch.isfinite(g[0, 3]).all()) and float(g[0, 3].abs().max()) > 0.0
    assert torch.equal(_bytes(g[0, :3]), _bytes(torch.zeros_like(g[0, :3])))
    assert ops._P3P.backward(None, None, None) is None      # no upstream gradient: none is returned, nothing is launched


# ---- 3. loss ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loss_ref(N, name):
    """the case (pnp_ref.score_case; the mask = the reference's inliers of the generating pose at the pair's threshold, plus the point
    behind the camera), the reference on the f64 originals, its deviation on as_kernel_input inputs, the band of the live decision
    (test_gpu_pnp._score_ref's width) and what a decision inside it moves"""
    m, models, valid, poses = R.score_case(N)
    thr = THR * np.array(THR_PAIRS)
    mask = np.stack([R.inlier_mask(m[p], poses[p], thr[p]) for p in range(3)])
    mask[:, -1] = True
    mk, ok, tk = R.as_kernel_input(m, name, 3), R.as_kernel_input(models, name, 4), R.as_kernel_input(thr, name, 5)
    ref, dev = G.pnp_loss(m, mask, models, valid, thr), G.pnp_loss(mk, mask, ok, valid, tk)
    width = 0.0
    for p in range(3):
        for j in np.flatnonzero(valid[p] & np.isfinite(models[p, :, 0, 0])):
            a, b = R.residual(m[p][mask[p]], models[p, j])[0], R.residual(mk[p][mask[p]], ok[p, j])[0]
            near = a < 4 * thr[p] ** 2
            if near.any():
                width = max(width, float(np.abs(a / thr[p] ** 2 - b / tk[p] ** 2)[near].max()))
    width *= F
    count, size = G.pnp_loss_bands(m, mask, models, valid, thr, width)
    # the gradient's figure is the case's, as test_gpu_pnp's figures are (the largest deviation of any slot), over the slots no live
    # decision can turn.  A figure per slot was tried first and is too tight for honest f32 arithmetic: on P3P slots whose only live
    # points are their own sample (gradient ~ 0 in f64) the f32 kernel sat at 1.11 (N = 7) and 1.97 (N = 2049) of 8 x the slot's own
    # figure, its error being the rounding of three fma per coordinate against the reference's rounding of the inputs (docs/LOG.md)
    slot_dev = np.abs(R.as_kernel_input(dev[3], name, 6) - ref[3]).reshape(3, R.M_SLOTS, -1).max(2)
    fig_g = float(slot_dev[count == 0].max())
    figs = dict(sums=float(np.abs(dev[0] - ref[0]).max()), per_pair=float(np.abs(dev[1] - ref[1]).max()), mean=abs(dev[2] - ref[2]),
                grad=fig_g, grad_slots=slot_dev)
    den = np.maximum(mask.sum(1) * valid.sum(1), 1)
    tol = dict(sums=F * figs["sums"] + count * width, per_pair=F * figs["per_pair"] + count.sum(1) * width / den,
               mean=F * figs["mean"] + float((count.sum(1) * width / den).mean()), grad=(F * fig_g + size)[:, :, None, None])
    return dict(m=m, models=models, valid=valid, poses=np.stack(poses), thr=thr, mask=mask, ref=ref, figs=figs, tol=tol, width=width,
                count=count)


def _raw(kind, matches, mask, models, keep, thr2):
    """the C entries on sentinel-filled outputs -> dict(sums, grad | None, per_pair, coef, mean)"""
    (P, N, _), M, dt = matches.shape, models.shape[1], matches.dtype
    new = lambda *shape: torch.full(shape, SENTINEL, device=matches.device, dtype=dt)
    out = dict(sums=new(P, M), grad=new(P, M, 4, 4) if kind == "fused" else None, per_pair=new(P), coef=new(P), mean=new(1))
    grad = (ptr(out["grad"]),) if kind == "fused" else ()
    L.call(f"dr_pnp_loss_{kind}_{L.suffix(dt)}", ptr(matches), ptr(mask.view(torch.uint8)), ptr(models), ptr(keep.view(torch.uint8)),
           ptr(thr2), P, M, N, ptr(out["sums"]), *grad, ptr(out["per_pair"]), ptr(out["coef"]), ptr(out["mean"]), stream())
    return out


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", R.SCORE_N)
def test_loss_value_gradient_and_mask_match_the_reference(N, dt):
    name = _name(dt)
    c = _loss_ref(N, name)
    sums0, pp0, mean0, grad0 = c["ref"]
    tol, figs = c["tol"], c["figs"]
    tm, tmo, tk, tmask, thr = _dev(c["m"], dt), _dev(c["models"], dt), _dev(c["valid"]), _dev(c["mask"]), _dev(c["thr"], dt)
    assert tmo.shape == (3, R.M_SLOTS, 4, 4)
    thr2 = ops.thr2_tensor(thr, 3, tm)
    fwd, fused, again = (_raw(k, tm, tmask, tmo, tk, thr2) for k in ("fwd", "fused", "fused"))
    for out in (fwd, fused):                                  # value: from both entries
        assert all(not bool((v == SENTINEL).any()) for v in out.values() if v is not None)
        es, ep, em = np.abs(_np(out["sums"]) - sums0), np.abs(_np(out["per_pair"]) - pp0), abs(float(out["mean"]) - mean0)
        print(f"loss N={N} {name}: sums {es.max():.3g} (measured {figs['sums']:.3g}, bound {tol['sums'].min():.3g}+), per_pair "
              f"{ep.max():.3g} (measured {figs['per_pair']:.3g}, bound {tol['per_pair'].min():.3g}+), mean {em:.3g} (measured "
              f"{figs['mean']:.3g}, bound {tol['mean']:.3g}); band width {c['width']:.3g}, points in it {int(c['count'].sum())}")
        assert (es <= tol["sums"]).all() and (ep <= tol["per_pair"]).all() and em <= tol["mean"]
    for key in ("sums", "grad", "per_pair", "coef", "mean"):  # a repeated call: the same bytes; the value-only entry: the fused one's
        assert torch.equal(_bytes(fused[key]), _bytes(again[key])), key
        assert key == "grad" or torch.equal(_bytes(fused[key]), _bytes(fwd[key])), key
    # the wrappers: the same entries
    s_w, pp_w = ops.pnp_loss_sums(tm, tmask, tmo, thr, tk, want_pairs=True)
    assert torch.equal(_bytes(s_w), _bytes(fwd["sums"])) and torch.equal(_bytes(pp_w), _bytes(fwd["per_pair"]))
    assert torch.equal(_bytes(ops.pnp_loss_mean(tm, tmask, tmo, thr, tk)), _bytes(fwd["mean"][0]))
    # gradient: loss.PnPLoss -> backward
    mg = tmo.clone().requires_grad_(True)
    loss = PnPLoss(thr)(mg, tm, gt_mask=tmask, keep=tk)
    assert torch.equal(_bytes(loss), _bytes(fused["mean"][0]))
    loss.backward()
    g = _np(mg.grad)
    eg = np.abs(g - grad0)
    ratio = (eg / np.maximum(tol["grad"], 1e-300)).reshape(3, R.M_SLOTS, -1).max(2)
    p, j = np.unravel_index(ratio.argmax(), ratio.shape)
    own = (eg.reshape(3, R.M_SLOTS, -1).max(2) / np.maximum(F * figs["grad_slots"], 1e-300))[c["valid"] & (c["count"] == 0)].max()
    print(f"loss N={N} {name}: gradient, worst error / bound {ratio[p, j]:.3g} at slot {(int(p), int(j))}: error {eg[p, j].max():.3g}, "
          f"measured {figs['grad']:.3g}, bound {tol['grad'][p, j, 0, 0]:.3g}, |grad| max {np.abs(grad0).max():.3g}; for information, the "
          f"worst error over 8 x the SLOT's own figure {own:.3g}")
    assert np.isfinite(g).all() and (eg <= tol["grad"]).all()
    assert not g[:, 131].any() and not g[:, 130].any() and not g[:, :, 3].any()          # the dropped slot, the NaN slot, row 3
    assert not _np(fused["sums"])[:, 131].any() and np.array_equal(_np(fused["sums"])[:, 130], c["mask"].sum(1))
    assert np.abs(g[:, 129]).max() > 0.0
    # the ground-truth mask: the reference's, except inside the band
    gt = _dev(c["poses"], dt)
    mk, count = ops.pnp_gt_mask(tm, gt, thr)
    assert mk.dtype == torch.bool and count.dtype == torch.int32 and torch.equal(count.long(), mk.sum(1))
    for p in range(3):
        want = R.inlier_mask(c["m"][p], c["poses"][p], c["thr"][p])
        off = mk[p].cpu().numpy() != want
        d2 = R.residual(c["m"][p], c["poses"][p])[0]
        assert (np.abs(d2[off] / c["thr"][p] ** 2 - 1.0) <= c["width"]).all(), (p, int(off.sum()))
        assert int(off.sum()) <= R.band_counts(c["m"][p], c["poses"][p][None], [True], c["thr"][p], c["width"])[0]
    crit = PnPLoss(thr)
    assert torch.equal(_bytes(crit(tmo, tm, gt_pose=gt, keep=tk)), _bytes(crit(tmo, tm, gt_mask=mk, keep=tk)))
    # contract: no gradient for the matches
    with pytest.raises(L.DransacError, match="detach"):
        crit(mg, tm.clone().requires_grad_(True), gt_mask=tmask, keep=tk)


# ---- 4. driver -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_hypotheses_train_step(dt):
    D = R.DRV
    P, N, B = D["P"], D["N"], D["B"]
    rounds = D["max_iterations"] // B
    sc = R.driver_scenes()
    tm = _dev(np.stack([s["matches"] for s in sc]), dt)
    base = _dev(np.stack([np.where(s["inlier"], 1.0, -1.0) for s in sc]), dt)
    logits = base.clone().requires_grad_(True)
    drv = BatchedPnP(ransac_batch_size=B, threshold=THR, max_iterations=D["max_iterations"], seed=3)
    out = drv.hypotheses(tm, logits)
    assert set(out) == {"models", "keep"} and rounds == 4
    assert out["models"].shape == (P, rounds * 4 * B, 4, 4) == (3, 1024, 4, 4) and out["keep"].shape == (3, 1024)
    assert out["keep"].dtype == torch.bool and out["models"].dtype == dt
    twin = BatchedPnP(ransac_batch_size=B, threshold=THR, max_iterations=D["max_iterations"], seed=3)
    by_hand = []
    for _ in range(rounds):
        samples, _, _ = ops.SampleGather.apply(tm, base, B, 3, 1.0, None, twin._seeds.next())
        mo, kp = ops.p3p(samples)
        by_hand.append((mo.reshape(P, 4 * B, 4, 4), kp.reshape(P, 4 * B)))
    assert torch.equal(_bytes(out["models"]), _bytes(torch.cat([b[0] for b in by_hand], 1)))
    assert torch.equal(out["keep"], torch.cat([b[1] for b in by_hand], 1))
    loss = PnPLoss(THR)(out["models"], tm.detach(), gt_pose=_dev(np.stack([s["pose"] for s in sc]), dt), keep=out["keep"])
    loss.backward()
    g = logits.grad
    assert g is not None and bool(torch.isfinite(g).all()) and bool((g.abs().sum(1) > 0).all())
    print(f"hypotheses {_name(dt)}: kept {int(out['keep'].sum())} / {out['keep'].numel()}, loss {float(loss):.4f}, |grad| per pair "
          f"{[f'{float(x):.3g}' for x in g.abs().sum(1)]}")
    # the method leaves no state behind: a test-mode call afterwards is a fresh driver's at the same call number
    fresh = BatchedPnP(ransac_batch_size=B, threshold=THR, max_iterations=D["max_iterations"], seed=3)
    fresh.calls = drv.calls
    assert drv.calls == rounds
    a, b = drv(tm, base), fresh(tm, base)
    assert set(a) == KEYS and all(torch.equal(_bytes(a[k]), _bytes(b[k])) for k in KEYS)
