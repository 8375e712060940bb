"""dr_registration_loss_{fused,scale,fwd} and dr_registration_gt_mask (ops.registration_loss_mean / _sums, ops.registration_gt_mask,
loss.RegistrationLoss) against the f64 reference of tests/registration_loss_ref.py, in f32 and f64.  Inputs, the band rule, the
tolerances and the gradient constant are that module's; the worst observed ratio of every case is printed."""
import functools

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from differentiable_ransac_amd import ops
from differentiable_ransac_amd.loss import RegistrationLoss
from tests import registration_loss_ref as RL

pytestmark = pytest.mark.gpu

DTYPES = {"f32": (torch.float32, "float32"), "f64": (torch.float64, "float64")}
SENTINEL = 777.0
c_int, ptr, stream = L.c_int, L.ptr, L.stream


@functools.lru_cache(maxsize=None)
def _reference(N, M, name, use_mask, use_keep, pairs):
    cs = RL.case(N, M, name)
    thr2 = RL.thr2_of(RL.threshold_of(pairs), name)
    return cs, thr2, RL.reference(cs, thr2, use_mask, use_keep)


def _inputs(cs, dev, tdt, use_mask=True, use_keep=True):
    t = lambda a: torch.tensor(a, dtype=tdt, device=dev)
    mask = torch.tensor(cs["mask"], device=dev) if use_mask else None
    keep = torch.tensor(cs["keep"], device=dev) if use_keep else None
    return t(cs["matches"]), mask, t(cs["models"]), keep


def _threshold(pairs, dev, tdt):
    return torch.tensor(RL.THRESHOLD_PAIRS, dtype=tdt, device=dev) if pairs else RL.THRESHOLD


def _raw(kind, matches, mask, models, keep, thr2):
    """the C entries on sentinel-filled outputs -> dict(sums, grad | None, per_pair, coef, mean)"""
    (P, N, _), M, dt = matches.shape, models.shape[1], matches.dtype
    new = lambda *shape: torch.full(shape, SENTINEL, device=matches.device, dtype=dt)
    out = dict(sums=new(P, M), grad=new(P, M, 4, 4) if kind == "fused" else None, per_pair=new(P), coef=new(P), mean=new(1))
    mk = None if mask is None else mask.view(torch.uint8)
    kp = None if keep is None else keep.view(torch.uint8)
    grad = (ptr(out["grad"]),) if kind == "fused" else ()
    L.call(f"dr_registration_loss_{kind}_{L.suffix(dt)}", ptr(matches), ptr(mk), ptr(models), ptr(kp), ptr(thr2), c_int(P), c_int(M),
           c_int(N), ptr(out["sums"]), *grad, ptr(out["per_pair"]), ptr(out["coef"]), ptr(out["mean"]), stream())
    return out


def _written(out):
    return all(not (v == SENTINEL).any() for v in out.values() if v is not None)


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("N,M", RL.CASES)
def test_values_against_the_reference(dev, N, M, name):
    tdt, np_name = DTYPES[name]
    worst = 0.0
    for use_mask, use_keep, pairs in RL.VARIANTS:
        cs, thr2, ref = _reference(N, M, np_name, use_mask, use_keep, pairs)
        matches, mask, models, keep = _inputs(cs, dev, tdt, use_mask, use_keep)
        thr = _threshold(pairs, dev, tdt)
        sums, per_pair = ops.registration_loss_sums(matches, mask, models, thr, keep, want_pairs=True)
        mean = ops.registration_loss_mean(matches, mask, models, thr, keep)
        assert torch.equal(ops.thr2_tensor(thr, RL.P, matches).double().cpu(), torch.tensor(thr2))   # the reference's thr2 is the kernel's
        tol_s, tol_p, tol_m = RL.value_tolerances(cs, thr2, ref, np_name)
        es = np.abs(sums.double().cpu().numpy() - ref["sums"])
        ep = np.abs(per_pair.double().cpu().numpy() - ref["per_pair"])
        em = abs(float(mean) - ref["mean"])
        worst = max(worst, float((es / np.maximum(tol_s, 1e-300)).max()), float((ep / tol_p).max()), em / tol_m)
        assert (es <= tol_s).all() and (ep <= tol_p).all() and em <= tol_m, (use_mask, use_keep, pairs)
        assert 0.0 <= float(mean) <= 1.0
    print(f"registration loss values N={N} M={M} {name}: worst error / tolerance {worst:.3g}")


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("N,M", RL.CASES)
def test_gradient_against_the_reference(dev, N, M, name):
    tdt, np_name = DTYPES[name]
    c = RL.tolerance_constant()[N]
    worst = 0.0
    for use_mask, use_keep, pairs in RL.GRAD_VARIANTS:
        cs, thr2, ref = _reference(N, M, np_name, use_mask, use_keep, pairs)
        matches, mask, models, keep = _inputs(cs, dev, tdt, use_mask, use_keep)
        models.requires_grad_(True)
        loss = ops.registration_loss_mean(matches, mask, models, _threshold(pairs, dev, tdt), keep)
        (loss * RL.UPSTREAM).backward()
        g = models.grad.double().cpu().numpy()
        assert np.isfinite(g).all() and not g[..., 3, :].any(), "the last row of the gradient is written as zeros"
        assert not g[~ref["keep"]].any(), "a dropped slot gets an exact-zero gradient"
        unit, compared = RL.gradient_units(cs, thr2, ref, use_mask, np_name)
        g_ref = RL.extended_gradient(cs, thr2, ref) if name == "f64" else ref["grad"]      # (the f64 reference errs like an f64 kernel)
        ratio = RL.worst_ratio(g, g_ref, unit, compared)
        worst = max(worst, ratio)
        assert ratio <= c, (use_mask, use_keep, pairs, ratio, c)
    print(f"registration loss gradient N={N} M={M} {name}: worst |g - g_ref| / (eps n mag) = {worst:.4g}, c = {c:.4g}")


@pytest.mark.parametrize("name", list(DTYPES))
def test_rules_empty_mask_no_kept_model_nan_and_inf_slots(dev, name):
    tdt, np_name = DTYPES[name]
    cs = RL.case(257, 65, np_name)
    matches, mask, models, keep = _inputs(cs, dev, tdt)
    thr2 = ops.thr2_tensor(RL.THRESHOLD, RL.P, matches)
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
    # NaN models in dropped slots: everything finite and equal to the run with those slots zeroed, bit for bit
    dropped = ~keep
    assert dropped.any()
    nan_models, zero_models = models.clone(), models.clone()
    nan_models[dropped] = float("nan")
    zero_models[dropped] = 0.0
    a, b = _raw("fused", matches, mask, nan_models, keep, thr2), _raw("fused", matches, mask, zero_models, keep, thr2)
    for key in a:
        assert torch.isfinite(a[key]).all() and torch.equal(a[key], b[key]), key
    lf = ops.registration_loss_mean(matches, mask, nan_models.requires_grad_(True), RL.THRESHOLD, keep)
    lf.backward()
    assert torch.isfinite(lf) and torch.isfinite(nan_models.grad).all() and not nan_models.grad[dropped].any()
    # a KEPT model with an inf entry: sums = #mask, zero gradient, the other models untouched
    inf_models = models.clone()
    inf_models[0, 0, 1, 2] = float("inf")
    inf_models[2, 0, 0, 3] = float("nan")
    out = _raw("fused", matches, mask, inf_models, keep, thr2)
    for p in (0, 2):
        assert float(out["sums"][p, 0]) == float(mask[p].sum()) and not out["grad"][p, 0].any()
    assert torch.equal(out["sums"][:, 1:], base["sums"][:, 1:]) and torch.equal(out["grad"][:, 1:], base["grad"][:, 1:])
    assert torch.isfinite(out["mean"]).all() and torch.isfinite(out["grad"]).all()


@pytest.mark.parametrize("name", list(DTYPES))
def test_a_point_exactly_at_the_threshold_takes_the_truncated_branch(dev, name):
    tdt, _ = DTYPES[name]
    # R = I, t = (0.25, 0, 0), q = p + (0.75, 0, 0): r = (-0.5, 0, 0), d2 = 0.25 = thr2 exactly (powers of two in both dtypes);
    # the second point sits at d2 = 0.0625 and is live, the second model moves the first point inside
    p = torch.tensor([[1.0, 2.0, 4.0], [0.5, 1.0, 2.0]], dtype=tdt, device=dev)
    q = p + torch.tensor([[0.75, 0.0, 0.0], [0.5, 0.0, 0.0]], dtype=tdt, device=dev)
    matches = torch.cat([p, q], -1)[None]
    models = torch.eye(4, dtype=tdt, device=dev).repeat(1, 2, 1, 1)
    models[0, 0, 0, 3], models[0, 1, 0, 3] = 0.25, 0.5
    models.requires_grad_(True)
    sums = ops.registration_loss_sums(matches, None, models, 0.5)
    assert sums.tolist() == [[1.0 + 0.25, 0.25 + 0.0]]
    ops.registration_loss_mean(matches, None, models, 0.5).backward()
    g = models.grad[0]
    # model 0: only point 1 (r = (-0.25, 0, 0)) is live: d sums / d t = (2 / 0.25) r = (-2, 0, 0), x coef = 1 / 4
    assert g[0, :3, 3].tolist() == [-0.5, 0.0, 0.0] and g[0, 0, :3].tolist() == [-0.25, -0.5, -1.0]
    # model 1: point 0 (r = (-0.25, 0, 0)) is live, point 1 has r = 0
    assert g[1, :3, 3].tolist() == [-0.5, 0.0, 0.0] and g[1, 0, :3].tolist() == [-0.5, -1.0, -2.0]
    mask, count = ops.registration_gt_mask(matches, models.detach()[:, 0].contiguous(), 0.5)
    assert mask.tolist() == [[False, True]] and count.tolist() == [1]
    # the backward is a kernel result: a second derivative through it is refused, not returned wrong
    (g1,) = torch.autograd.grad(ops.registration_loss_mean(matches, None, models, 0.5), models, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("N,M", [(1, 65), (65, 65), (257, 130), (1000, 65)])
def test_paths_agree_and_repeat_bit_for_bit(dev, N, M, name):
    tdt, np_name = DTYPES[name]
    cs = RL.case(N, M, np_name)
    for use_mask, use_keep in ((True, True), (False, False)):
        matches, mask, models, keep = _inputs(cs, dev, tdt, use_mask, use_keep)
        thr2 = ops.thr2_tensor(_threshold(True, dev, tdt), RL.P, matches)
        fused, again, fwd = (_raw(k, matches, mask, models, keep, thr2) for k in ("fused", "fused", "fwd"))
        assert _written(fused) and _written(fwd)
        for key in ("sums", "grad", "per_pair", "coef", "mean"):
            assert torch.equal(fused[key], again[key]), key
            if key != "grad":
                assert torch.equal(fused[key], fwd[key]), key
        # the backward: every element written, bit-repeatable, = grad_unscaled x coef x upstream / P
        up = torch.tensor([RL.UPSTREAM], dtype=tdt, device=dev)
        gm = [torch.full_like(fused["grad"], SENTINEL) for _ in range(2)]
        for g in gm:
            L.call(f"dr_registration_loss_scale_{L.suffix(tdt)}", ptr(fused["grad"]), ptr(fused["coef"]), ptr(up), c_int(RL.P), c_int(M),
                   ptr(g), stream())
        assert torch.equal(gm[0], gm[1]) and not (gm[0] == SENTINEL).any()
        want = fused["grad"] * (fused["coef"] * up / RL.P)[:, None, None, None]
        assert torch.allclose(gm[0], want, rtol=4 * RL.eps_of(np_name), atol=0.0)


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("N", RL.N_SWEEP)
def test_gt_mask_is_the_references(dev, N, name):
    tdt, np_name = DTYPES[name]
    cs = RL.case(N, RL.M_AT_N, np_name)            # (check_inputs: no point within the band or the rounding margin of the pose)
    matches = torch.tensor(cs["matches"], dtype=tdt, device=dev)
    pose = torch.tensor(cs["pose"], dtype=tdt, device=dev)
    for pairs in (False, True):
        want = RL.ratio(cs, cs["pose"][:, None], RL.thr2_of(RL.threshold_of(pairs), np_name))[:, 0] < 1.0
        mask, count = ops.registration_gt_mask(matches, pose, _threshold(pairs, dev, tdt))
        assert mask.dtype == torch.bool and count.dtype == torch.int32
        assert np.array_equal(mask.cpu().numpy(), want) and count.tolist() == want.sum(1).tolist()
        assert pairs or np.array_equal(want, cs["mask"])
    # the loss takes the pose in place of the mask, and [P,4,4] models
    crit = RegistrationLoss(RL.THRESHOLD)
    models = torch.tensor(cs["models"], dtype=tdt, device=dev)
    by_pose = crit(models, matches, gt_pose=pose)
    by_mask = crit(models, matches, gt_mask=torch.tensor(cs["mask"], device=dev))
    assert torch.equal(by_pose, by_mask)
    assert torch.equal(crit(models[:, 0], matches, gt_pose=pose), crit(models[:, :1], matches, gt_mask=torch.tensor(cs["mask"], device=dev)))


def _train_step(dev, seed, device_seeds):
    from differentiable_ransac_amd.ransac import BatchedRegistration
    from tests import registration_ref as R
    P, N = 2, 200
    scenes = [R.scene(40 + p, N, 0.6) for p in range(P)]
    matches = torch.tensor(np.stack([s["matches"] for s in scenes]), dtype=torch.float32, device=dev)
    pose = torch.eye(4, device=dev).repeat(P, 1, 1)
    for p, s in enumerate(scenes):
        pose[p, :3, :3], pose[p, :3, 3] = torch.tensor(s["R"], dtype=torch.float32), torch.tensor(s["t"], dtype=torch.float32)
    logits = torch.linspace(-1.0, 1.0, N, device=dev).repeat(P, 1).clone().requires_grad_(True)
    drv = BatchedRegistration(train=True, ransac_batch_size=64, max_iterations=128, threshold=R.THRESHOLD, seed=seed)
    if device_seeds:
        drv.device_seeds(dev)
    crit = RegistrationLoss(R.THRESHOLD)
    with torch.no_grad():
        gt_mask = ops.registration_gt_mask(matches, pose, R.THRESHOLD)[0]

    def step():
        logits.grad = None
        out = drv(matches, logits)
        out["models"].retain_grad()
        loss = crit(out["models"], matches, gt_mask=gt_mask, keep=out["keep"])
        loss.backward()
        return loss, out["models"].grad, logits.grad
    return step


def _close(a, b):
    # the logit gradient leaves the loss through the sampler's backward, which adds the rows' terms with float atomics
    # (csrc/gumbel_topk.hip): its last bits depend on the order of arrival, as in tests/test_gpu_graphs.py
    return torch.allclose(a, b, rtol=1e-3, atol=1e-6 * float(a.abs().max()))


def test_end_to_end_train_step_and_graph_replay(dev):
    """BatchedRegistration(train=True) -> RegistrationLoss(keep) -> backward on 2 pairs x 200 points, two rounds of 64 hypotheses.
    Bit for bit: the loss and its gradient w.r.t. the models (this path has no atomics).  The logit gradient is finite, non-zero
    and equal up to the summation order of the sampler's atomic backward."""
    from differentiable_ransac_amd.graphs import GraphedStep
    loss, gm, grad = (t.clone() for t in _train_step(dev, 11, False)())
    assert torch.isfinite(loss) and 0.0 < float(loss.detach()) <= 1.0 and gm.shape == (2, 128, 4, 4)
    assert torch.isfinite(grad).all() and (grad != 0).any()
    loss2, gm2, grad2 = _train_step(dev, 11, False)()
    assert torch.equal(loss, loss2) and torch.equal(gm, gm2) and _close(grad, grad2), "the same seed gives the same bits"
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
