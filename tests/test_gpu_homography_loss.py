"""dr_homography_loss_{fused,scale,fwd} and dr_homography_gt_mask (ops.homography_loss_mean / _sums, ops.homography_gt_mask,
loss.HomographyLoss) against the f64 reference of tests/homography_loss_ref.py, in f32 and f64.  Inputs, the band rule, the
tolerances and the gradient constant are that module's; the worst observed ratio of every case is printed."""
import functools

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from differentiable_ransac_amd import ops
from differentiable_ransac_amd.loss import HomographyLoss
from tests import homography_loss_ref as HL

pytestmark = pytest.mark.gpu

DTYPES = {"f32": (torch.float32, "float32"), "f64": (torch.float64, "float64")}
SENTINEL = 777.0
c_int, ptr, stream = L.c_int, L.ptr, L.stream


@functools.lru_cache(maxsize=None)
def _reference(N, M, name, use_mask, use_keep, pairs):
    cs = HL.case(N, M, name)
    thr2 = HL.thr2_of(HL.threshold_of(pairs), name)
    return cs, thr2, HL.reference(cs, thr2, use_mask, use_keep)


def _inputs(cs, dev, tdt, use_mask=True, use_keep=True):
    t = lambda a: torch.tensor(a, dtype=tdt, device=dev)
    mask = torch.tensor(cs["mask"], device=dev) if use_mask else None
    keep = torch.tensor(cs["keep"], device=dev) if use_keep else None
    return t(cs["matches"]), mask, t(cs["models"]), keep


def _threshold(pairs, dev, tdt):
    return torch.tensor(HL.THRESHOLD_PAIRS, dtype=tdt, device=dev) if pairs else HL.THRESHOLD


def _raw(kind, matches, mask, models, keep, thr2):
    """the C entries on sentinel-filled outputs -> dict(sums, grad | None, per_pair, coef, mean)"""
    (P, N, _), M, dt = matches.shape, models.shape[1], matches.dtype
    new = lambda *shape: torch.full(shape, SENTINEL, device=matches.device, dtype=dt)
    out = dict(sums=new(P, M), grad=new(P, M, 3, 3) if kind == "fused" else None, per_pair=new(P), coef=new(P), mean=new(1))
    mk = None if mask is None else mask.view(torch.uint8)
    kp = None if keep is None else keep.view(torch.uint8)
    grad = (ptr(out["grad"]),) if kind == "fused" else ()
    L.call(f"dr_homography_loss_{kind}_{L.suffix(dt)}", ptr(matches), ptr(mk), ptr(models), ptr(kp), ptr(thr2), c_int(P), c_int(M),
           c_int(N), ptr(out["sums"]), *grad, ptr(out["per_pair"]), ptr(out["coef"]), ptr(out["mean"]), stream())
    return out


def _written(out):
    return all(not (v == SENTINEL).any() for v in out.values() if v is not None)


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("N,M", HL.CASES)
def test_values_against_the_reference(dev, N, M, name):
    tdt, np_name = DTYPES[name]
    worst = 0.0
    for use_mask, use_keep, pairs in HL.VARIANTS:
        cs, thr2, ref = _reference(N, M, np_name, use_mask, use_keep, pairs)
        matches, mask, models, keep = _inputs(cs, dev, tdt, use_mask, use_keep)
        thr = _threshold(pairs, dev, tdt)
        sums, per_pair = ops.homography_loss_sums(matches, mask, models, thr, keep, want_pairs=True)
        mean = ops.homography_loss_mean(matches, mask, models, thr, keep)
        assert torch.equal(ops.thr2_tensor(thr, HL.P, matches).double().cpu(), torch.tensor(thr2))   # the reference's thr2 is the kernel's
        tol_s, tol_p, tol_m = HL.value_tolerances(cs, thr2, ref, np_name)
        es = np.abs(sums.double().cpu().numpy() - ref["sums"])
        ep = np.abs(per_pair.double().cpu().numpy() - ref["per_pair"])
        em = abs(float(mean) - ref["mean"])
        worst = max(worst, float((es / np.maximum(tol_s, 1e-300)).max()), float((ep / tol_p).max()), em / tol_m)
        assert (es <= tol_s).all() and (ep <= tol_p).all() and em <= tol_m, (use_mask, use_keep, pairs)
        assert 0.0 <= float(mean) <= 1.0
    print(f"homography loss values N={N} M={M} {name}: worst error / tolerance {worst:.3g}")


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("N,M", HL.CASES)
def test_gradient_against_the_reference(dev, N, M, name):
    tdt, np_name = DTYPES[name]
    c = HL.tolerance_constant()[N]
    worst = worst_inner = 0.0
    for use_mask, use_keep, pairs in HL.GRAD_VARIANTS:
        cs, thr2, ref = _reference(N, M, np_name, use_mask, use_keep, pairs)
        matches, mask, models, keep = _inputs(cs, dev, tdt, use_mask, use_keep)
        models.requires_grad_(True)
        loss = ops.homography_loss_mean(matches, mask, models, _threshold(pairs, dev, tdt), keep)
        (loss * HL.UPSTREAM).backward()
        g = models.grad.double().cpu().numpy()
        assert np.isfinite(g).all()
        assert not g[~ref["keep"]].any(), "a dropped slot gets an exact-zero gradient"
        unit, compared = HL.gradient_units(cs, thr2, ref, use_mask, np_name)
        g_ref = HL.extended_gradient(cs, thr2, ref) if name == "f64" else ref["grad"]      # (the f64 reference errs like an f64 kernel)
        ratio, inner = HL.worst_ratio(g, g_ref, unit, compared), HL.inner_ratio(g, cs, unit, compared)
        worst, worst_inner = max(worst, ratio), max(worst_inner, inner)
        print(f"  variant {(use_mask, use_keep, pairs)}: |g - g_ref| / (eps W) = {ratio:.4g}, |<g, H>| / (eps <W, |H|>) = {inner:.4g}")
        assert ratio <= c, (use_mask, use_keep, pairs, ratio, c)
        assert inner <= c, (use_mask, use_keep, pairs, inner, c)
    print(f"homography loss gradient N={N} M={M} {name}: worst ratio {worst:.4g}, worst <g, H> ratio {worst_inner:.4g}, c = {c:.4g}")


@pytest.mark.parametrize("name", list(DTYPES))
def test_rules_empty_mask_no_kept_model_bad_slots_and_zero_threshold(dev, name):
    tdt, np_name = DTYPES[name]
    cs = HL.case(257, 65, np_name)
    matches, mask, models, keep = _inputs(cs, dev, tdt)
    thr2 = ops.thr2_tensor(HL.THRESHOLD, HL.P, matches)
    base = _raw("fused", matches, mask, models, keep, thr2)
    assert _written(base)
    # pair 1 with an empty mask / with keep all false: per_pair 0, zero gradients, the other pairs bit for bit as before
    for which in ("mask", "keep"):
        mk, kp = mask.clone(), keep.clone()
        (mk if which == "mask" else kp)[1] = False
        out = _raw("fused", matches, mk, models, kp, thr2)
        assert _written(out)
        assert float(out["per_pair"][1]) == 0.0 and not out["grad"][1].any() and not out["sums"][1].any() and float(out["coef"][1]) == 1.0
        for p in (0, 2):
            for key in ("sums", "grad", "per_pair", "coef"):
                assert torch.equal(out[key][p], base[key][p]), (which, key, p)
        assert torch.isfinite(out["mean"]).all()
    # NaN models in dropped slots are never read: sums 0, gradient 0, everything else bit for bit the run with those slots zeroed
    dropped = ~keep
    assert dropped.any()
    nan_models, zero_models = models.clone(), models.clone()
    nan_models[dropped] = float("nan")
    zero_models[dropped] = 0.0
    a, b = _raw("fused", matches, mask, nan_models, keep, thr2), _raw("fused", matches, mask, zero_models, keep, thr2)
    for key in a:
        assert torch.isfinite(a[key]).all() and torch.equal(a[key], b[key]) and torch.equal(a[key], base[key]), key
    assert not a["sums"][dropped].any() and not a["grad"][dropped].any()
    lf = ops.homography_loss_mean(matches, mask, nan_models.requires_grad_(True), HL.THRESHOLD, keep)
    lf.backward()
    assert torch.isfinite(lf) and torch.isfinite(nan_models.grad).all() and not nan_models.grad[dropped].any()
    # KEPT models with an inf entry, a NaN entry and det == 0 (a zero row): sums = #mask, zero gradient, the other models untouched
    bad = models.clone()
    bad[0, 0, 1, 2] = float("inf")
    bad[1, 0, 2, 0] = float("nan")
    bad[2, 0, 2] = 0.0
    out = _raw("fused", matches, mask, bad, keep, thr2)
    for p in range(3):
        assert float(out["sums"][p, 0]) == float(mask[p].sum()) and not out["grad"][p, 0].any()
    assert torch.equal(out["sums"][:, 1:], base["sums"][:, 1:]) and torch.equal(out["grad"][:, 1:], base["grad"][:, 1:])
    assert torch.isfinite(out["mean"]).all() and torch.isfinite(out["grad"]).all()
    # thr2 = 0 (pair 0) and NaN (pair 2): nothing is below it -- sums = #mask for the kept models, zero gradients, pair 1 as before
    t0 = thr2.clone()
    t0[0], t0[2] = 0.0, float("nan")
    out = _raw("fused", matches, mask, models, keep, t0)
    for p in (0, 2):
        assert torch.equal(out["sums"][p], keep[p].to(tdt) * mask[p].sum()) and not out["grad"][p].any() and float(out["per_pair"][p]) == 1.0
    assert torch.equal(out["sums"][1], base["sums"][1]) and torch.equal(out["grad"][1], base["grad"][1])
    # a model and its negation: the same sums bit for bit, the negated gradient bit for bit
    out = _raw("fused", matches, mask, -models, keep, thr2)
    assert torch.equal(out["sums"], base["sums"]) and torch.equal(out["grad"], -base["grad"]) and torch.equal(out["mean"], base["mean"])


@pytest.mark.parametrize("name", list(DTYPES))
def test_constructed_boundary_points_are_decided_exactly(dev, name):
    tdt, _ = DTYPES[name]
    # under the identity e = x2 - x1 and f = -e.  Point 0: e = (1, 0): d2 = 1 + 1 = 2 = thr2 exactly -> truncated.  Point 1: e = (0.5, 0):
    # d2 = 0.5, live.  Model 1 shifts x by 0.5: e = (0.5, 0) and 0, both live.  Every value is a dyadic rational, exact in both dtypes.
    matches = torch.tensor([[[8.0, 16.0, 9.0, 16.0], [4.0, 2.0, 4.5, 2.0]]], dtype=tdt, device=dev)
    models = torch.eye(3, dtype=tdt, device=dev).repeat(1, 2, 1, 1)
    models[0, 1, 0, 2] = 0.5
    thr2 = torch.tensor([2.0], dtype=tdt, device=dev)
    out = _raw("fused", matches, None, models, None, thr2)
    assert out["sums"].tolist() == [[1.0 + 0.5 / 2.0, 0.5 / 2.0 + 0.0]]
    # model 0: only point 1 is live, y_w = z_w = 1, 2 / thr2 = 1: d sums / d h = (-e_0, -e_1, e . t) (x1, 1)^T with e = (0.5, 0),
    # t = x1 = (4, 2); the adjugate half: f = (-0.5, 0), s = x2 = (4.5, 2) -> (-f_0, -f_1, f . s) (x2, 1)^T, brought back by J^T at h = I
    gh = np.outer([-0.5, 0.0, 2.0], [4.0, 2.0, 1.0])
    ga = np.outer([0.5, 0.0, -2.25], [4.5, 2.0, 1.0]).reshape(9)
    want = gh + HL.adj_vjp(np.eye(3).reshape(9), ga, np.stack).reshape(3, 3)
    assert np.array_equal(out["grad"][0, 0].double().cpu().numpy(), want)
    # a truncated point passes nothing: model 0's gradient is point 1's alone, bit for bit
    alone = _raw("fused", matches[:, 1:].contiguous(), None, models, None, thr2)
    assert torch.equal(alone["grad"][0, 0], out["grad"][0, 0]) and float(alone["sums"][0, 0]) == float(out["sums"][0, 0]) - 1.0
    # the ground-truth mask has the same strict test: at threshold 2 a point with e = (1, 1), d2 = 4 = thr2, is out
    edge = torch.tensor([[[8.0, 16.0, 9.0, 17.0], [4.0, 2.0, 4.5, 2.0]]], dtype=tdt, device=dev)
    mask, count = ops.homography_gt_mask(edge, models[:, 0].contiguous(), 2.0)
    assert mask.tolist() == [[False, True]] and count.tolist() == [1]
    # a point behind the camera with d2 = 0: H = diag(-1, 1, -1) has det > 0 and sends x1 = (3, 0) to y = (-3, 0, -1): y_w < 0,
    # t = (3, 0) = x2, and adj(H) = diag(-1, 1, -1) gives z_w < 0, s = x1.  It counts 1 and passes nothing; under the identity it is live
    Hb = torch.diag(torch.tensor([-1.0, 1.0, -1.0], dtype=tdt, device=dev))
    assert float(torch.linalg.det(Hb.double())) > 0
    mb = torch.tensor([[[3.0, 0.0, 3.0, 0.0]]], dtype=tdt, device=dev)
    out = _raw("fused", mb, None, Hb[None, None].contiguous(), None, thr2)
    assert out["sums"].tolist() == [[1.0]] and not out["grad"].any() and out["mean"].tolist() == [1.0]
    front = _raw("fused", mb, None, torch.eye(3, dtype=tdt, device=dev)[None, None].contiguous(), None, thr2)
    assert front["sums"].tolist() == [[0.0]]
    mask, count = ops.homography_gt_mask(mb, Hb[None].contiguous(), 3.0)
    assert mask.tolist() == [[False]] and count.tolist() == [0]
    # the backward is a kernel result: a second derivative through it is refused, not returned wrong
    mg = models.clone().requires_grad_(True)
    (g1,) = torch.autograd.grad(ops.homography_loss_mean(matches, None, mg, 2.0), mg, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("N,M", [(1, 65), (65, 65), (257, 130), (1000, 65)])
def test_paths_agree_and_repeat_bit_for_bit(dev, N, M, name):
    tdt, np_name = DTYPES[name]
    cs = HL.case(N, M, np_name)
    for use_mask, use_keep in ((True, True), (False, False)):
        matches, mask, models, keep = _inputs(cs, dev, tdt, use_mask, use_keep)
        thr2 = ops.thr2_tensor(_threshold(True, dev, tdt), HL.P, matches)
        fused, again, fwd = (_raw(k, matches, mask, models, keep, thr2) for k in ("fused", "fused", "fwd"))
        assert _written(fused) and _written(fwd)
        for key in ("sums", "grad", "per_pair", "coef", "mean"):
            assert torch.equal(fused[key], again[key]), key
            if key != "grad":
                assert torch.equal(fused[key], fwd[key]), key
        # the backward: every element written, bit-repeatable, = grad_unscaled x coef x upstream / P
        up = torch.tensor([HL.UPSTREAM], dtype=tdt, device=dev)
        gm = [torch.full_like(fused["grad"], SENTINEL) for _ in range(2)]
        for g in gm:
            L.call(f"dr_homography_loss_scale_{L.suffix(tdt)}", ptr(fused["grad"]), ptr(fused["coef"]), ptr(up), c_int(HL.P), c_int(M),
                   ptr(g), stream())
        assert torch.equal(gm[0], gm[1]) and not (gm[0] == SENTINEL).any()
        want = fused["grad"] * (fused["coef"] * up / HL.P)[:, None, None, None]
        assert torch.allclose(gm[0], want, rtol=4 * HL.eps_of(np_name), atol=0.0)


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("N", HL.N_SWEEP)
def test_gt_mask_is_the_references_and_the_state_steps(dev, N, name):
    tdt, np_name = DTYPES[name]
    cs = HL.case(N, HL.M_AT_N, np_name)            # (check_inputs: no point within the band or the rounding margin of the ground truth)
    matches = torch.tensor(cs["matches"], dtype=tdt, device=dev)
    gt_H = torch.tensor(cs["gt_H"], dtype=tdt, device=dev)
    geo = HL.geometry(cs["matches"], cs["gt_H"][:, None])
    for pairs in (False, True):
        thr2 = HL.thr2_of(HL.threshold_of(pairs), np_name)
        want = (geo["front"] & (geo["d2"] / thr2[:, None, None] < 1.0))[:, 0]
        mask, count = ops.homography_gt_mask(matches, gt_H, _threshold(pairs, dev, tdt))
        assert mask.dtype == torch.bool and count.dtype == torch.int32
        assert np.array_equal(mask.cpu().numpy(), want) and count.tolist() == want.sum(1).tolist()
        assert count.tolist() == mask.sum(1).tolist()
        assert pairs or np.array_equal(want, cs["mask"])
        # the mask dr_homography_update writes for the same model and threshold, bit for bit
        st = ops.HomographyState(HL.P, N, 100, dev, tdt)
        ops.homography_update(st, matches, gt_H[:, None].contiguous(), None, torch.ones(HL.P, 1, dtype=tdt, device=dev),
                              _threshold(pairs, dev, tdt), 1)
        assert torch.equal(st.best_mask, mask) and torch.equal(st.best_inliers, count)
    # the loss takes the homography in place of the mask, and [P,3,3] models
    crit = HomographyLoss(HL.THRESHOLD)
    models = torch.tensor(cs["models"], dtype=tdt, device=dev)
    by_H = crit(models, matches, gt_H=gt_H)
    by_mask = crit(models, matches, gt_mask=torch.tensor(cs["mask"], device=dev))
    assert torch.equal(by_H, by_mask)
    assert torch.equal(crit(models[:, 0], matches, gt_H=gt_H), crit(models[:, :1], matches, gt_mask=torch.tensor(cs["mask"], device=dev)))


def _train_step(dev, seed, device_seeds):
    from differentiable_ransac_amd.ransac import BatchedHomography
    from tests import homography_ref as HR
    P, N = 2, 257
    scenes = [HR.scene(40 + p, N, 0.6) for p in range(P)]
    matches = torch.tensor(np.stack([s["matches"] for s in scenes]), dtype=torch.float32, device=dev)
    gt_H = torch.tensor(np.stack([s["H"] for s in scenes]), dtype=torch.float32, device=dev)
    logits = torch.linspace(-1.0, 1.0, N, device=dev).repeat(P, 1).clone().requires_grad_(True)
    drv = BatchedHomography(train=True, ransac_batch_size=64, max_iterations=128, threshold=HR.THRESHOLD, seed=seed)
    if device_seeds:
        drv.device_seeds(dev)
    crit = HomographyLoss(HR.THRESHOLD)
    with torch.no_grad():
        gt_mask = ops.homography_gt_mask(matches, gt_H, HR.THRESHOLD)[0]

    def step():
        logits.grad = None
        out = drv(matches, logits)
        out["models"].retain_grad()
        loss = crit(out["models"], matches, gt_mask=gt_mask, keep=out["keep"])
        loss.backward()
        return loss, out["models"].grad, logits.grad

    def by_gt_H():
        out = drv(matches, logits)
        return crit(out["models"], matches, gt_H=gt_H, keep=out["keep"])
    step.by_gt_H = by_gt_H
    return step


def _close(a, b):
    # the logit gradient leaves the loss through the sampler's backward, which adds the rows' terms with float atomics
    # (csrc/gumbel_topk.hip): its last bits depend on the order of arrival, as in tests/test_gpu_graphs.py
    return torch.allclose(a, b, rtol=1e-3, atol=1e-6 * float(a.abs().max()))


def test_end_to_end_train_step_and_graph_replay(dev):
    """BatchedHomography(train=True) -> HomographyLoss(keep) -> backward on 2 pairs x 257 points, two rounds of 64 hypotheses.
    Bit for bit: the loss and its gradient w.r.t. the models (this path has no atomics).  The logit gradient is finite, non-zero
    and equal up to the summation order of the sampler's atomic backward."""
    from differentiable_ransac_amd.graphs import GraphedStep
    first_step = _train_step(dev, 11, False)
    loss, gm, grad = (t.clone() for t in first_step())
    assert torch.isfinite(loss) and 0.0 < float(loss.detach()) <= 1.0 and gm.shape == (2, 128, 3, 3)
    assert torch.isfinite(gm).all() and torch.isfinite(grad).all() and (grad != 0).any()
    loss2, gm2, grad2 = _train_step(dev, 11, False)()
    assert torch.equal(loss, loss2) and torch.equal(gm, gm2) and _close(grad, grad2), "the same seed gives the same bits"
    assert torch.equal(_train_step(dev, 11, False).by_gt_H(), loss), "gt_H gives the mask that ops.homography_gt_mask gives"
    # captured with device seeds: replay r equals eager call warmup + r of a driver with the same base seed
    warm = 2
    eager = _train_step(dev, 11, True)
    for _ in range(warm):
        eager()
    want = [t.clone() for t in eager()]
    step = GraphedStep(_train_step(dev, 11, True), warmup=warm)
    first = [t.clone() for t in step()]
    assert torch.equal(first[0], want[0]) and torch.equal(first[1], want[1]), "the first replay equals the eager step of the same seed"
    assert torch.isfinite(first[2]).all() and (first[2] != 0).any() and _close(first[2], want[2])
    second = [t.clone() for t in step()]
    assert torch.isfinite(second[2]).all() and not torch.equal(first[1], second[1]), "the second replay draws new samples: the seed advanced"
