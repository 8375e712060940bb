"""dr_kabsch, dr_kabsch_bwd and dr_refit_rigid_bwd (ops.kabsch, ops.weighted_kabsch) and BatchedRegistration(train=True) against
the f64 references of tests/kabsch_grad_ref.py, in f32 and f64.  Inputs, tolerance rule and its constant are that module's:
per sample (or pair) |g - g_ref|_inf <= c eps kappa_eff mag, samples with kappa > KAPPA_MAX checked for finiteness only."""
import functools

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from differentiable_ransac_amd import ops
from tests import kabsch_grad_ref as G

pytestmark = pytest.mark.gpu

DTYPES = {"f32": (torch.float32, np.float32, G.EPS32), "f64": (torch.float64, np.float64, G.EPS64)}
SENTINEL = 777.0


def _dev(a, dev, tdt):
    return None if a is None else torch.tensor(a, dtype=tdt, device=dev)


def _upstream(case, dev, tdt):
    """the [.,4,4] gradient whose top rows are (gR, gt) and whose last row -- never read -- is NaN"""
    g = torch.full(case["gR"].shape[:1] + (4, 4), float("nan"), dtype=tdt, device=dev)
    g[:, :3, :3] = _dev(case["gR"], dev, tdt)
    g[:, :3, 3] = _dev(case["gt"], dev, tdt)
    return g


def _bound(err, scale, kap, c, eps, f32):
    """-> (ok, worst ratio): err, scale, kap per sample; kappa_eff = 1 in f32 after checking c eps64 kappa <= eps32"""
    if f32:
        assert (c * G.EPS64 * kap <= G.EPS32).all()
    tol = c * eps * (1.0 if f32 else kap) * scale
    return bool((err <= tol).all()), float((err / tol).max())


@functools.lru_cache(maxsize=None)
def _sample_reference(Bt, k, weighted, dt):
    cs = G.sample_case(Bt, k, weighted, DTYPES[dt][1])
    gx, gw = G.autograd(cs["x"], cs["w"], cs["gR"], cs["gt"])
    rows = [(cs["x"][s], None if cs["w"] is None else cs["w"][s]) for s in range(Bt)]
    kap = np.array([G.kappa(x, w) for x, w in rows])
    mag = np.array([G.weight_grad_magnitude(x, w, cs["gR"][s], cs["gt"][s]) for s, (x, w) in enumerate(rows)])
    return cs, gx, gw, kap, mag


def _kabsch_grads(dev, tdt, x, w, upstream):
    xs = _dev(x, dev, tdt).requires_grad_(True)
    ws = None if w is None else _dev(w, dev, tdt).requires_grad_(True)
    models, valid = ops.kabsch(xs, ws)
    models.backward(upstream)
    return models.detach(), valid, xs.grad, None if ws is None else ws.grad


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("k", G.SAMPLE_K)
def test_kabsch_forward_is_kabsch_gather_bit_for_bit(dev, dt, k):
    tdt, ndt, _ = DTYPES[dt]
    P, N, B = 2, 200, 65
    g = torch.Generator().manual_seed(5 + k)
    matches = torch.tensor(np.stack([G.scene_matches(p, N, ndt) for p in range(P)]), dtype=tdt, device=dev)
    idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(B)]) for _ in range(P)]).to(torch.int32)
    idx[0, 3, 1] = idx[0, 3, 0]                                  # a repeated row: degenerate for k = 3
    idx = idx.to(dev)
    want_m, want_v = ops.kabsch_gather(matches, idx)
    samples = torch.stack([matches[p][idx[p].long()] for p in range(P)])
    got_m, got_v = ops.kabsch(samples)
    assert got_m.shape == (P, B, 4, 4) and got_v.shape == (P, B) and got_v.dtype == torch.bool
    assert torch.equal(got_m, want_m) and torch.equal(got_v, want_v)
    assert bool(got_v.any()) and (k > 3 or not bool(got_v[0, 3]))
    # unit weights are the same fit, bit for bit
    got_w, _ = ops.kabsch(samples, torch.ones(P, B, k, dtype=tdt, device=dev))
    assert torch.equal(got_w, want_m)


# ------------------------------------------------------------------------------------------------------------ kabsch backward
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k", G.SAMPLE_K)
@pytest.mark.parametrize("Bt", G.SAMPLE_BT)
def test_kabsch_backward_against_f64_autograd(dev, Bt, k, weighted, dt):
    tdt, _, eps = DTYPES[dt]
    cs, rx, rw, kap, mag = _sample_reference(Bt, k, weighted, dt)
    _, valid, gx, gw = _kabsch_grads(dev, tdt, cs["x"], cs["w"], _upstream(cs, dev, tdt))
    gx = gx.cpu().double().numpy()
    assert bool(valid.all()) and np.isfinite(gx).all() and gx.shape == (Bt, k, 6)
    use = kap <= G.KAPPA_MAX
    assert (~use).sum() <= 0.01 * Bt
    c = G.tolerance_constant()[k]
    ok, worst = _bound(np.abs(gx - rx).max((1, 2))[use], np.abs(rx).max((1, 2))[use], kap[use], c, eps, dt == "f32")
    print(f"samples Bt={Bt} k={k} weighted={weighted} {dt}: worst error / tolerance = {worst:.3g}")
    assert ok, worst
    if weighted:
        gw = gw.cpu().double().numpy()
        assert np.isfinite(gw).all() and gw.shape == (Bt, k)
        ok, worst = _bound(np.abs(gw - rw).max(1)[use], mag[use], kap[use], c, eps, dt == "f32")
        print(f"   weight gradient: worst error / tolerance = {worst:.3g}")
        assert ok, worst
    else:
        assert gw is None


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_kabsch_backward_degenerate_samples_get_exact_zeros(dev, dt):
    tdt = DTYPES[dt][0]
    good = G.sample_case(1, 3, False, DTYPES[dt][1])["x"][0]
    line = np.concatenate([np.array([[0, 0, 0], [1, 2, 3], [2, 4, 6]], float), good[:, 3:]], 1)      # collinear p
    twin = good.copy()
    twin[1] = twin[0]                                                                                # a repeated row
    x = np.stack([good, line, twin, good])
    up = torch.randn(4, 4, 4, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(dev, tdt)
    up[3] = up[0]                                          # the two good samples: same bits next to a degenerate neighbour or not
    w = np.full((4, 3), 0.5)
    for weights in (None, w):
        models, valid, gx, gw = _kabsch_grads(dev, tdt, x, weights, up)
        assert valid.tolist() == [True, False, False, True]
        assert torch.equal(models[1], torch.eye(4, dtype=tdt, device=dev)) and torch.equal(models[2], models[1])
        assert bool((gx[1:3] == 0).all()) and bool((gx[0] != 0).any()) and torch.equal(gx[0], gx[3])
        if weights is not None:
            assert bool((gw[1:3] == 0).all()) and bool((gw[0] != 0).any())


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_kabsch_backward_on_a_reflection_sample(dev, dt):
    """d = det(V U^T) = -1 with s2 well above s3: K = tr(A) I - A carries the sign through A = R H, nothing else changes"""
    tdt, ndt, eps = DTYPES[dt]
    x = G.reflection_sample().astype(ndt).astype(np.float64)
    assert G._svd_parts(x, None)[-1] == -1.0
    rng = np.random.default_rng(4)
    cs = dict(gR=rng.standard_normal((1, 3, 3)).astype(ndt).astype(np.float64), gt=rng.standard_normal((1, 3)).astype(ndt).astype(np.float64))
    rx, _ = G.autograd(x[None], None, cs["gR"], cs["gt"])
    models, valid, gx, _ = _kabsch_grads(dev, tdt, x[None], None, _upstream(cs, dev, tdt))
    assert bool(valid[0]) and float(torch.linalg.det(models[0, :3, :3].double())) == pytest.approx(1.0, abs=1e-5)
    kap = np.array([G.kappa(x)])
    err = np.abs(gx.cpu().double().numpy() - rx).max((1, 2))
    ok, worst = _bound(err, np.abs(rx).max((1, 2)), kap, G.tolerance_constant()[4], eps, dt == "f32")
    assert ok, worst


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_kabsch_backward_zero_weight_row(dev, dt):
    tdt, ndt, eps = DTYPES[dt]
    cs = G.sample_case(1, 4, True, ndt)
    w = cs["w"].copy()
    w[0, 2] = 0.0
    rx, rw = G.autograd(cs["x"], w, cs["gR"], cs["gt"])
    _, valid, gx, gw = _kabsch_grads(dev, tdt, cs["x"], w, _upstream(cs, dev, tdt))
    assert bool(valid[0]) and bool((gx[0, 2] == 0).all()) and bool(torch.isfinite(gw).all()) and float(gw[0, 2]) != 0.0
    kap = np.array([G.kappa(cs["x"][0], w[0])])
    assert kap[0] <= G.KAPPA_MAX
    c = G.tolerance_constant()[4]
    mag = np.array([G.weight_grad_magnitude(cs["x"][0], w[0], cs["gR"][0], cs["gt"][0])])
    assert _bound(np.abs(gx.cpu().double().numpy() - rx).max((1, 2)), np.abs(rx).max((1, 2)), kap, c, eps, dt == "f32")[0]
    assert _bound(np.abs(gw.cpu().double().numpy() - rw).max(1), mag, kap, c, eps, dt == "f32")[0]


# ------------------------------------------------------------------------------------------------------------ weighted_kabsch backward
@functools.lru_cache(maxsize=None)
def _pair_reference(N, kind, weighted, dt):
    cs = G.pair_case(N, kind, weighted, DTYPES[dt][1])
    return (cs,) + G.pair_reference(cs)


def _raw_refit_bwd(dev, tdt, cs, want_m=True, want_w=True):
    """dr_refit_rigid_bwd on buffers pre-filled with a sentinel -> (grad_matches | None, grad_weights | None)"""
    m = _dev(cs["x"], dev, tdt)
    P, N, _ = m.shape
    mask = None if cs["mask"] is None else torch.tensor(cs["mask"], device=dev)
    w = _dev(cs["w"], dev, tdt)
    gm = torch.full((P, N, 6), SENTINEL, dtype=tdt, device=dev) if want_m else None
    gw = torch.full((P, N), SENTINEL, dtype=tdt, device=dev) if want_w else None
    L.call(f"dr_refit_rigid_bwd_{L.suffix(tdt)}", L.ptr(m), L.ptr(None if mask is None else mask.view(torch.uint8)), L.ptr(w),
           L.ptr(_upstream(cs, dev, tdt)), L.c_int(P), L.c_int(N), L.ptr(gm), L.ptr(gw), L.stream())
    return gm, gw


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N,kind,weighted", G.PAIR_CASES)
def test_weighted_kabsch_backward_against_f64_autograd(dev, N, kind, weighted, dt):
    tdt, _, eps = DTYPES[dt]
    cs, rx, rw, kap, mag = _pair_reference(N, kind, weighted, dt)
    assert (kap <= G.KAPPA_MAX).all()
    gm, gw = _raw_refit_bwd(dev, tdt, cs)
    gm2, gw2 = _raw_refit_bwd(dev, tdt, cs)
    assert torch.equal(gm, gm2) and torch.equal(gw, gw2)                      # a repeated launch gives the same bits
    gm, gw = gm.cpu().double().numpy(), gw.cpu().double().numpy()
    if cs["mask"] is not None:
        assert (gm[~cs["mask"]] == 0).all() and (gw[~cs["mask"]] == 0).all()  # exact zeros over the sentinel
        assert all((gm[p][cs["mask"][p]] != 0).any() for p in range(len(gm)))
    c = G.tolerance_constant()["pair"]
    ok, worst = _bound(np.abs(gm - rx).max((1, 2)), np.abs(rx).max((1, 2)), kap, c, eps, dt == "f32")
    print(f"pairs N={N} mask={kind} weighted={weighted} {dt}: worst error / tolerance = {worst:.3g}")
    assert ok, worst
    ok, worst = _bound(np.abs(gw - rw).max(1), mag, kap, c, eps, dt == "f32")
    print(f"   weight gradient: worst error / tolerance = {worst:.3g}")
    assert ok, worst


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N,weighted", [(1000, True), (257, False), (3, True)])
def test_weighted_kabsch_backward_two_rows_is_zero_everywhere(dev, N, weighted, dt):
    tdt = DTYPES[dt][0]
    cs = G.pair_case(N, "two", weighted, DTYPES[dt][1])
    gm, gw = _raw_refit_bwd(dev, tdt, cs)
    assert bool((gm == 0).all()) and bool((gw == 0).all())
    _, valid = ops.weighted_kabsch(_dev(cs["x"], dev, tdt), _dev(cs["w"], dev, tdt), torch.tensor(cs["mask"], device=dev))
    assert not bool(valid.any())


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_weighted_kabsch_autograd_outputs(dev, dt):
    """ops.weighted_kabsch: forward = refit_rigid; gradients to the matches alone, the weights alone and both are the entry's bits"""
    tdt = DTYPES[dt][0]
    cs = G.pair_case(1000, "ragged", True, DTYPES[dt][1])
    mask = torch.tensor(cs["mask"], device=dev)
    up = torch.nan_to_num(_upstream(cs, dev, tdt), nan=0.0)
    want_m, want_w = _raw_refit_bwd(dev, tdt, cs)
    for need_m, need_w in ((True, True), (True, False), (False, True)):
        m = _dev(cs["x"], dev, tdt).requires_grad_(need_m)
        w = _dev(cs["w"], dev, tdt).requires_grad_(need_w)
        model, valid = ops.weighted_kabsch(m, w, mask)
        ref_model, ref_valid = ops.refit_rigid(m.detach(), mask, w.detach())
        assert torch.equal(model, ref_model) and torch.equal(valid, ref_valid) and bool(valid.all()) and not valid.requires_grad
        model.backward(up)
        assert (m.grad is not None) == need_m and (w.grad is not None) == need_w
        assert not need_m or torch.equal(m.grad, want_m)
        assert not need_w or torch.equal(w.grad, want_w)
    # no weights: gradient to the matches, of the unit-weight fit
    m = _dev(cs["x"], dev, tdt).requires_grad_(True)
    ops.weighted_kabsch(m, None, mask)[0].backward(up)
    cs1 = dict(cs, w=None)
    assert torch.equal(m.grad, _raw_refit_bwd(dev, tdt, cs1, want_w=False)[0])


# ------------------------------------------------------------------------------------------------------------ driver
def test_registration_train_logits_gradient_f64(dev):
    """BatchedRegistration(train=True), explicit noise, P = 2, N = 300, B = 65, k = 3, two rounds; loss = mean over the kept
    hypotheses of |R - R_gt|_F^2 + |t - t_gt|^2; logits.grad against CPU f64 autograd over oracle/cpu_ref.py's sampler and gather and
    reference (a)'s Kabsch.

    Tolerance (inf-norm over the logits), from the error the sample gradients are allowed: the logit gradient is
    sum_b sum_r a_br dy_soft[b, i_r] / dlogit with a_br = <g_samples[b, r], matches[i_r]> and |dy_i / dl_n| <= y_i / tau, so
    c eps64 sum_b kappa_b |g_samples_b|_inf 6 |matches|_inf sum_r y[b, i_r] / tau  (the kernel's share)
    + 64 eps64 sum_b sum_r |a_br| y[b, i_r] / tau                                   (the soft-max and the sums, both sides)."""
    from differentiable_ransac_amd import synth
    from differentiable_ransac_amd.ransac import BatchedRegistration
    from oracle import cpu_ref as O
    from tests import registration_ref as R
    P, N, B, k, rounds, tau = 2, 300, 65, 3, 2, 1.0
    scenes = [R.scene(100 + p, N, 0.6) for p in range(P)]
    m64 = torch.tensor(np.stack([s["matches"] for s in scenes]))
    gt = torch.eye(4, dtype=torch.float64).repeat(P, 1, 1)
    for p in range(P):
        gt[p, :3, :3], gt[p, :3, 3] = torch.tensor(scenes[p]["R"]), torch.tensor(scenes[p]["t"])
    logits = torch.randn(P, N, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    noise = [synth.gumbel_noise((P, B, N), seed=300 + r, dtype=torch.float64) for r in range(rounds)]

    def pose_loss(models, keep, gt_):
        d = models[..., :3, :] - gt_[:, None, :3, :]
        per = (d * d).sum((-1, -2))
        return torch.where(keep, per, torch.zeros_like(per)).sum() / keep.sum()

    drv = BatchedRegistration(ransac_batch_size=B, max_iterations=B * rounds, num_samples=k, tau=tau, train=True)
    lg = logits.to(dev).requires_grad_(True)
    out = drv(m64.to(dev), lg, gumbels=[g.to(dev) for g in noise])
    assert out["models"].shape == (P, rounds * B, 4, 4) and out["keep"].shape == (P, rounds * B)
    keep = out["keep"].cpu()
    # CPU side: the same index sets first
    l64 = logits.clone().requires_grad_(True)
    models, samples, ys = [], [], []
    for r in range(rounds):
        idx_gpu = ops.gumbel_topk(logits.to(dev), B, k, tau, noise[r].to(dev), 0, soft=False)["idx"].cpu().long()
        per_pair = []
        for p in range(P):
            idx, ret, y_soft = O.gumbel_topk(l64[p], noise[r][p], tau, k)
            assert torch.equal(idx, torch.sort(idx_gpu[p], -1).values)
            s = O.gather_samples(m64[p], ret)
            s.retain_grad()
            samples.append((s, idx, y_soft.detach()))
            per_pair.append(G.torch_kabsch(s))
        models.append(torch.stack(per_pair))
    models = torch.cat(models, 1)
    assert float((models.detach() - out["models"].detach().cpu()).abs().max()) < 1e-9
    loss_ref = pose_loss(models, keep, gt)
    loss_ref.backward()
    loss = pose_loss(out["models"], out["keep"], gt.to(dev))
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(loss_ref.detach()), rel=1e-12)
    c = G.tolerance_constant()[k]
    mmax = float(m64.abs().max())
    tol = 0.0
    for s, idx, y in samples:
        gs = s.grad.detach()
        ysel = torch.gather(y, 1, idx)                                       # [B,k]
        kap = torch.tensor([G.kappa(x.detach().numpy()) for x in s])
        live = torch.isfinite(kap)
        a = (gs * s.detach()).sum(-1).abs()                                  # [B,k]
        tol += float((c * G.EPS64 * kap[live] * gs.abs().amax((1, 2))[live] * 6 * mmax * ysel.sum(1)[live]).sum() / tau)
        tol += float(64 * G.EPS64 * (a * ysel).sum() / tau)
    err = float((lg.grad.cpu() - l64.grad).abs().max())
    print(f"driver: |dlogits - ref|_inf = {err:.3g}, tolerance {tol:.3g}, |ref|_inf = {float(l64.grad.abs().max()):.3g}")
    assert float(l64.grad.abs().max()) > 0 and tol < 1e-6 * float(l64.grad.abs().max())
    assert err <= tol
