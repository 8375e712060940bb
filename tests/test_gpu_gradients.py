"""The backward kernels that produce the training signal, against torch autograd through the f64 oracle on the same inputs
(and the same explicit Gumbel noise where a sampler is involved): rigid solver, rigid residual, the 3-D train path end to
end, the weighted 8-point solver, MSAC scoring and the pose error in f32.  tests/test_oracle_gradients.py checks, on the
CPU, that each arbiter's autograd is the derivative.

Tolerances are derived from f32 rounding, u = 2^-24: each is u times a bound on the sizes of the terms the kernel adds up
(the f64 sum of |per-point contributions|, times the accumulation depth) or times the conditioning of the sample, with a
stated safety factor; never u times max|grad| alone."""
import math

import pytest
import torch

from oracle import cpu_ref as O
from tests.conftest import load_golden
from tests.test_oracle_gradients import f8_batch, rigid_batch, rigid_branch_neg, rigid_gap

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
F64 = torch.float64


def rigid_gap_t(data):
    """[Bt] gap_t = min_{i != j} |lambda_i - lambda_j| / lambda_max of cov^T cov, the conditioning of the SVD that
    O.rigid_svd(flag=True) differentiates."""
    d = data - data.mean(1, keepdim=True)
    cov = d[..., :3].transpose(-1, -2) @ d[..., 3:]
    lam = torch.linalg.eigvalsh(cov.transpose(-1, -2) @ cov)
    return torch.minimum(lam[:, 2] - lam[:, 1], lam[:, 1] - lam[:, 0]) / lam[:, 2]


def _excess(err, tol):
    """max of err / tol (<= 1 passes), for the assertion messages"""
    return float((err / tol).max())


# ------------------------------------------------------------------------------------------------------- K3r backward
GAP_MIN = 1e-3


@pytest.mark.parametrize("Bt", [1, 63, 65, 4097])
@pytest.mark.parametrize("n", [3, 4, 10, 100])
@pytest.mark.parametrize("flag", [True, False])
def test_rigid_solver_backward_against_f64_autograd(dev, flag, n, Bt):
    """dr_solve_rigid_bwd_f32 (rigid_bwd_kernel): random upstream gradients on model (all 16 entries), R, t and all three.

    Tolerance per sample (the kernel works in f64 from the f32 samples; what is f32 is the R it reads back from the model,
    relative error <= u per entry, and its output):
      flag=False -- the polar factor's derivative solves Y Z + Z Y = skew(W), W = R^T (G_R - 1 (g_t o c0)^T), Y = sc R^T cov,
        so perturbing R by u moves G_cov = 2 sc R Z by about u sc |W| / (gap s_max), gap = min(s_i + s_j) / s_max; a point
        receives G_cov (or its transpose) times dq (dp): T_cov = 2 sc |W| max(|dp|, |dq|) / (gap s_max);
      the centroid term g_c0 = -g_t colsum(R) / n: T_c = 4 |g_t| / n;
      the f32 store: max|g_ref|.
    tol = 64 u (T_cov + T_c + max|g_ref|); samples with gap < GAP_MIN are not compared (asserted finite).
      flag=True -- R = I whatever the data (Q9) and the kernel's R path is exactly zero, while the arbiter differentiates
        the SVD of sc^2 cov^T cov, which it resolves only to eps_64 / gap_t, gap_t = min(lambda_i - lambda_j) / lambda_max:
        tol = 64 u (T_c + max|g_ref|) + 64 eps_64 sc |W| max(|dp|, |dq|) / gap_t, and samples with gap_t < GAP_MIN (where the
        arbiter's R itself is not I to 1e-3: nearly repeated singular values) are not compared."""
    from differentiable_ransac_amd import ops
    data = rigid_batch(Bt, n, seed=1000 * n + Bt + 7 * flag, dtype=torch.float32)
    x64 = data.double()
    neg = rigid_branch_neg(x64, flag)
    if Bt > 1 and (not flag or n == 3):   # flag=True, n > 3: cov^T cov is positive definite, det(V U^T) = 1 always
        assert 0 < int(neg.sum()) < Bt, int(neg.sum())
    g = torch.Generator().manual_seed(Bt + n)
    Gm = torch.randn(Bt, 4, 4, generator=g, dtype=F64)
    GR = torch.randn(Bt, 3, 3, generator=g, dtype=F64)
    Gt = torch.randn(Bt, 3, generator=g, dtype=F64)

    s = data.to(dev).requires_grad_(True)
    model, R, t, _, valid = ops.solve_rigid_autograd(s, None, flag)
    assert bool(valid.all())
    xo = x64.clone().requires_grad_(True)
    mo, Ro, to, _, oko = O.rigid_svd(xo, flag=flag)
    assert bool(oko.all())

    d = x64 - x64.mean(1, keepdim=True)
    dp, dq = d[..., :3], d[..., 3:]
    c0 = x64[..., :3].mean(1)
    Rd = Ro.detach()
    cov = dp.transpose(-1, -2) @ dq
    sc = 3.0 * n * n / (dp.norm(dim=-1).sum(1) * dq.norm(dim=-1).sum(1))
    reach = torch.maximum(dp.norm(dim=-1).amax(1), dq.norm(dim=-1).amax(1))
    if flag:
        gap_t = rigid_gap_t(x64)
        compare = gap_t >= GAP_MIN
        assert int(compare.sum()) >= max(1, int(0.8 * Bt)), (int(compare.sum()), Bt)
    else:
        gap = rigid_gap(x64, Rd)
        compare = gap >= GAP_MIN
        assert int(compare.sum()) >= max(1, int(0.9 * Bt)), (int(compare.sum()), Bt)
        s_max = torch.linalg.eigvalsh(sc[:, None, None] * 0.5 * (Rd.transpose(-1, -2) @ cov + cov.transpose(-1, -2) @ Rd)
                                      ).abs().amax(-1)
    assert float((R.detach().cpu().double() - Ro.detach()).abs().amax((1, 2))[compare].max()) < 1e-3

    zero = torch.zeros(Bt, 4, 4, dtype=F64)
    bottom = zero.clone()
    bottom[:, 3] = Gm[:, 3]
    modes = {"model": (Gm, None, None), "R": (None, GR, None), "t": (None, None, Gt), "all": (Gm, GR, Gt),
             "bottom_row": (bottom, None, None)}
    for mode, (gm_, gr_, gt_) in modes.items():
        lg = 0
        lo = 0
        if gm_ is not None:
            lg = lg + (model * gm_.float().to(dev)).sum()
            lo = lo + (mo * gm_).sum()
        if gr_ is not None:
            lg = lg + (R * gr_.float().to(dev)).sum()
            lo = lo + (Ro * gr_).sum()
        if gt_ is not None:
            lg = lg + (t * gt_.float().to(dev)).sum()
            lo = lo + (to * gt_).sum()
        gk, = torch.autograd.grad(lg, s, retain_graph=True)
        go, = torch.autograd.grad(lo, xo, retain_graph=True)
        gk = gk.cpu().double()
        assert bool(torch.isfinite(gk).all()), mode
        if mode == "bottom_row":        # the constant row (0, 0, 0, 1) contributes nothing
            assert float(gk.abs().max()) == 0.0 and float(go.abs().max()) < 1e-12
            continue
        gme = zero if gm_ is None else gm_
        g_t = gme[:, :3, 3] + (0 if gt_ is None else gt_)
        G_R = gme[:, :3, :3] + (0 if gr_ is None else gr_)
        T = 4 * g_t.norm(dim=-1) / n + go.abs().amax((1, 2))
        W = Rd.transpose(-1, -2) @ (G_R - torch.ones(Bt, 3, 1, dtype=F64) * (g_t * c0)[:, None, :])
        if not flag:
            T = T + 2 * sc * W.norm(dim=(-1, -2)) * reach / (gap.clamp(min=GAP_MIN) * s_max)
            tol = 64 * U32 * T
        else:       # + the arbiter's own rounding through the SVD of cov^T cov (the kernel's R path is exactly zero here)
            tol = 64 * U32 * T + 64 * 2.0 ** -52 * sc * W.norm(dim=(-1, -2)) * reach / gap_t.clamp(min=GAP_MIN)
        err = (gk - go).abs().amax((1, 2))
        bad = compare & ~(err <= tol)
        assert not bool(bad.any()), (mode, int(bad.sum()), _excess(err[compare], tol[compare]))


def test_rigid_solver_backward_refuses_f64(dev):
    from differentiable_ransac_amd import ops
    from differentiable_ransac_amd._lib import DransacError
    s = rigid_batch(8, 4, seed=3).to(dev).requires_grad_(True)
    model, _, _, _, _ = ops.solve_rigid_autograd(s, None, True)
    with pytest.raises(DransacError):
        model.sum().backward()


# ------------------------------------------------------------------------------------------------------- K4r backward
def _residual_grad_and_bound(pts, models, g_res, chunk=64):
    """f64 torch on pts.device: d(sum_pm g_res[p,m] res[p,m]) / d models [P,M,4,4] by autograd of the plain residual
    sum_n |q_n - (A p_n + t)|^2, and the f32 error bound of rigid_residual_bwd_kernel [P,M,4,4]:
      each residual component e_ni is three fmas and a subtraction: |de| <= 4u (|q_ni| + sum_k |m_ik| |x_nk|);
      each product 2 e x rounds once, and the sum runs through 8 points per lane, 6 wave levels, 4 waves and one
      partial per 2048-point chunk: depth = 8 + 6 + 2 + ceil(N / 2048), |dsum| <= (depth + 2) u sum_n |e_ni x_nk|.
    bound = 2 |g| (4 sum_n (|q| + |m||x|) |x| + (depth + 2) sum_n |e x|) (times u by the caller)."""
    P, N, _ = pts.shape
    M = models.shape[1]
    depth = 8 + 6 + 2 + math.ceil(N / 2048)
    grad = torch.zeros(P, M, 4, 4, dtype=F64, device=pts.device)
    bound = torch.zeros(P, M, 4, 4, dtype=F64, device=pts.device)
    for p in range(P):
        x = pts[p].double()
        xh = torch.cat((x[:, :3], torch.ones(N, 1, dtype=F64, device=x.device)), 1)
        for m0 in range(0, M, chunk):
            mm = models[p, m0:m0 + chunk].double().requires_grad_(True)
            gp = g_res[p, m0:m0 + chunk].double()
            e = x[None, :, 3:] - xh[None] @ mm[:, :3, :].transpose(-1, -2)          # [c,N,3]
            gm, = torch.autograd.grad(((e * e).sum((1, 2)) * gp).sum(), mm)
            grad[p, m0:m0 + chunk] = gm
            with torch.no_grad():
                eb = x[None, :, 3:].abs() + xh.abs()[None] @ mm[:, :3, :].abs().transpose(-1, -2)
                b = 4 * torch.einsum("cni,nk->cik", eb, xh.abs()) + (depth + 2) * torch.einsum("cni,nk->cik", e.abs(), xh.abs())
                bound[p, m0:m0 + chunk, :3] = 2 * gp.abs()[:, None, None] * b
    return grad, bound


def _rigid_models(P, M, seed):
    g = torch.Generator().manual_seed(seed)
    Q, _ = torch.linalg.qr(torch.eye(3, dtype=F64) + 0.2 * torch.randn(P, M, 3, 3, generator=g, dtype=F64))
    Q = Q * torch.sign(torch.linalg.det(Q))[..., None, None]
    m = torch.zeros(P, M, 4, 4, dtype=F64)
    m[..., :3, :3] = Q
    m[..., :3, 3] = 0.3 * torch.randn(P, M, 3, generator=g, dtype=F64)
    m[..., 3, 3] = 1
    return m.float()


@pytest.mark.parametrize("N", [1, 7, 2047, 2048, 2049, 5000])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("P", [1, 3])
def test_rigid_residual_backward_against_f64(dev, P, M, N):
    """dr_rigid_residual_bwd_f32: 16-model tiles and 2048-point chunks, with and without tails."""
    _check_rigid_residual(dev, P, M, N)


def test_rigid_residual_backward_config4_size(dev):
    """BASELINE configs[3]-sized: one pair, 2048 models, 50 000 points (the f64 reference runs on the device, in chunks)."""
    _check_rigid_residual(dev, 1, 2048, 50000)


def _check_rigid_residual(dev, P, M, N):
    from differentiable_ransac_amd import ops, synth
    pts = torch.stack([synth.rigid_pair(100 * P + p + N, N)["matches"] for p in range(P)]).to(dev)
    models = _rigid_models(P, M, seed=M + N).to(dev).requires_grad_(True)
    g_res = torch.randn(P, M, generator=torch.Generator().manual_seed(P * M + N), dtype=F64)
    res, _ = ops.rigid_residual_autograd(pts, models, 0.03)
    gk, = torch.autograd.grad((res * g_res.float().to(dev)).sum(), models)
    ref, bound = _residual_grad_and_bound(pts, models.detach(), g_res.to(dev))
    assert float(gk[..., 3, :].abs().max()) == 0.0           # the constant bottom row
    err = (gk.double() - ref).abs()
    tol = 2 * U32 * bound + 1e-30                               # safety factor 2 on the bound of the docstring
    assert bool((err <= tol).all()), _excess(err, tol)


# ------------------------------------------------------------------------------------------------------- 3-D train path
def _logit_grad_scale(logits64, gumbels64, contrib, tau=1.0, k=3):
    """sum over (batch sample b, slot j) of c_bj y_bj (delta_{sel_bj, n} + y_bn) / tau: the f64 sum of |per-sample
    contributions| to the logits gradient through the straight-through estimator; contrib(b, idx [B,k]) -> c [B,k] >= 0
    (the magnitude of the upstream a_bj = <dL/dsample_bj, point sel_bj> (+ dL/dweight_bj), or a bound on its error)."""
    S = torch.zeros_like(logits64)
    for b, gb in enumerate(gumbels64):
        idx, _, y = O.gumbel_topk(logits64, gb, tau, k)
        a = contrib(b, idx)
        ysel = torch.gather(y, 1, idx)
        S += ((a * ysel).sum(1)[:, None] * y).sum(0) / tau
        S.index_add_(0, idx.reshape(-1), (a * ysel).reshape(-1) / tau)
    return S


def _ransac3d_oracle(matches, logits, gumbels, flag, Wm, Wr):
    """f64 autograd of O.ransac3d_train_batch over the batches: loss = mean over batches of the mean residual + <Wm, models>
    + <Wr, residuals>.  -> (logits grad, chosen models, and a tolerance scale per logit)."""
    m64, l64 = matches.double(), logits.double().requires_grad_(True)
    loss, chosen, per = 0, [], []
    nb = len(gumbels)
    for b, gb in enumerate(gumbels):
        model, res, mean_res, _, _ = O.ransac3d_train_batch(m64, l64, gb.double(), flag=flag)
        assert model.shape[0] == res.shape[0]
        loss = loss + mean_res / nb + (model * Wm[b]).sum() + (res * Wr[b]).sum()
        chosen.append(model.detach())
    loss.backward()
    # tolerance: per sample the f32 model gradient carries (residual-kernel bound + rounding of the upstream) relative error
    # kappa_b; through the solver's backward (linear in the model gradient, flag=True; conditioned by 1/gap, flag=False) it
    # reaches the sample gradient and, through the straight-through estimator, the logits
    N = matches.shape[0]
    B = gumbels[0].shape[0]
    pts = matches.double()[None]
    kap = []
    for b in range(nb):
        g_res = (1.0 / (nb * B * N) + Wr[b])[None]
        ref, bound = _residual_grad_and_bound(pts, chosen[b][None], g_res)
        gmod = ref[0] + Wm[b]
        k_b = (U32 * bound[0] + U32 * Wm[b].abs()).norm(dim=(-1, -2)) / gmod.norm(dim=(-1, -2))
        if not flag:
            idx = O.gumbel_topk(logits.double(), gumbels[b].double(), 1.0, 3)[0]
            k_b = k_b / rigid_gap(matches.double()[idx], chosen[b][:, :3, :3]).clamp(min=1e-6)
        kap.append(k_b)

    def contrib(b, idx):
        x = m64[idx].clone().requires_grad_(True)
        model, _, _, _, _ = O.rigid_svd(x, flag=flag)
        res = O.rigid_squared_residual(m64[:, :3], m64[:, 3:], model[:, :3, :].transpose(-1, -2))[0]
        l = (res * (1.0 / (nb * B * N) + Wr[b])).sum() + (model * Wm[b]).sum()
        gx, = torch.autograd.grad(l, x)
        # |a| (the f32 rounding of the store and of the estimator) + the error bound of a, in units of u
        return (gx.abs() * m64[idx].abs()).sum(-1) * (1 + kap[b][:, None] / U32)
    scale = _logit_grad_scale(l64.detach(), [gb.double() for gb in gumbels], contrib)
    return l64.grad, torch.cat(chosen), scale


def _drop_in_3d(dev, matches, logits, gumbels, flag, Wm, Wr):
    from differentiable_ransac_amd.estimators import RigidTransformationSVDBasedSolver
    from differentiable_ransac_amd.ransac import RANSAC3D
    from differentiable_ransac_amd.samplers import GumbelSoftmaxSampler
    from differentiable_ransac_amd.scorings import MSACScore
    B = gumbels[0].shape[0]
    r3 = RANSAC3D(RigidTransformationSVDBasedSolver(device="cuda"), GumbelSoftmaxSampler(B, 3, device="cuda"),
                  MSACScore("cuda"), train=True, ransac_batch_size=B, sampler_id=2, max_iterations=B * len(gumbels), flag=flag)
    lg = logits.to(dev).requires_grad_(True)
    models, residuals, means, _, _ = r3(matches.to(dev), lg, None, gumbels=[x.to(dev) for x in gumbels])
    keys = sorted(models)
    assert len(keys) == len(gumbels) and all(models[k].shape[0] == B for k in keys)
    loss = sum(means.values()) / len(means)
    for b, k in enumerate(keys):
        loss = loss + (models[k] * Wm[b].float().to(dev)).sum() + (residuals[k] * Wr[b].float().to(dev)).sum()
    loss.backward()
    return lg.grad.cpu().double(), torch.cat([models[k] for k in keys]).detach().cpu().double()


def _functional(nb, B, seed):
    g = torch.Generator().manual_seed(seed)
    return ([1e-2 * torch.randn(B, 4, 4, generator=g, dtype=F64) for _ in range(nb)],
            [1e-3 * torch.randn(B, generator=g, dtype=F64) for _ in range(nb)])


def test_ransac3d_train_logits_gradient_on_the_reference_run(dev):
    """RANSAC3D (flag=True) on the reference's ransac3d_train fixture: the reference's loss (mean of avg_residuals) plus a
    random linear functional of the models and residuals, logits gradient against f64 autograd over the same gumbels."""
    gd = load_golden("ransac3d_train")
    gumbels = list(gd["gumbels"])
    Wm, Wr = _functional(len(gumbels), gumbels[0].shape[0], 3)
    gk, mk = _drop_in_3d(dev, gd["matches"], gd["logits"], gumbels, True, Wm, Wr)
    go, mo, scale = _ransac3d_oracle(gd["matches"], gd["logits"], gumbels, True, Wm, Wr)
    assert float((mk - mo).abs().max()) < 1e-3                 # same index sets
    tol = 16 * U32 * scale
    err = (gk - go).abs()
    assert bool((err <= tol).all()), _excess(err, tol)
    assert float(go.abs().max()) > 0


@pytest.mark.parametrize("flag", [True, False])
def test_ransac3d_train_logits_gradient_on_synthetic_pairs(dev, flag):
    """RANSAC3D on synth.rigid_pair data with explicit noise, both flags; and BatchedRANSAC3D(train=True) with P = 3 gives
    each pair the gradient the per-pair drop-in gives."""
    from differentiable_ransac_amd import synth
    from differentiable_ransac_amd.ransac import BatchedRANSAC3D
    P, N, B, rounds = 3, 400, 32, 2
    pairs = [synth.rigid_pair(50 + p, N) for p in range(P)]
    gumbels = [synth.gumbel_noise((P, B, N), seed=70 + r) for r in range(rounds)]
    Wm, Wr = _functional(rounds, B, 5)
    drop = []
    for p in range(P):
        gk, mk = _drop_in_3d(dev, pairs[p]["matches"], pairs[p]["logits"], [g_[p] for g_ in gumbels], flag, Wm, Wr)
        go, mo, scale = _ransac3d_oracle(pairs[p]["matches"], pairs[p]["logits"], [g_[p] for g_ in gumbels], flag, Wm, Wr)
        assert float((mk - mo).abs().max()) < 1e-3
        tol = 16 * U32 * scale
        err = (gk - go).abs()
        assert bool((err <= tol).all()), (p, _excess(err, tol))
        drop.append((gk, tol))
    br = BatchedRANSAC3D(ransac_batch_size=B, train=True, max_iterations=B * rounds, flag=flag)
    lg = torch.stack([pp["logits"] for pp in pairs]).to(dev).requires_grad_(True)
    out = br(torch.stack([pp["matches"] for pp in pairs]).to(dev), lg, gumbels=[g_.to(dev) for g_ in gumbels])
    assert bool(out["keep"].all())
    W_m = torch.cat(Wm, 0).float().to(dev)
    W_r = torch.cat(Wr, 0).float().to(dev)
    loss = out["mean_residuals"].mean(1).sum() + (out["models"] * W_m).sum() + (out["residuals"] * W_r).sum()
    loss.backward()
    for p in range(P):
        err = (lg.grad[p].cpu().double() - drop[p][0]).abs()
        assert bool((err <= drop[p][1]).all()), (p, _excess(err, drop[p][1]))


# ------------------------------------------------------------------------------------------------------- K3f8 weighted
@pytest.mark.parametrize("n", [8, 9, 12, 20])
@pytest.mark.parametrize("Bt", [1, 65])
def test_weighted_f8_solver_backward_against_f64_autograd(dev, n, Bt):
    """dr_solve_f8_bwd_f32 with weights: grad_samples and grad_weights against f64 autograd of O.fundamental_8pt, moderate
    weights (0.2 .. 1), loss ((F . W).sum())^2 (F's sign is LAPACK's).  The kernel solves again in f64 from the f32 inputs
    and uses the stored F only for its sign; what is f32 is the upstream gradient 2 (F . W) W, whose relative error is
    u sum|F o W| / |sum F o W| (kappa), and the stored output.  tol = 8 u (1 + kappa) |g_ref|_max per sample, plus the
    f64 solve's own rounding amplified by the eigen-gap of A^T A (below 1e-9 relative here).  n = 8: the null vector
    ignores row scaling, the weights receive nothing (asserted as such)."""
    from differentiable_ransac_amd import ops
    pts, w = f8_batch(Bt, n, seed=n + Bt, dtype=torch.float32)
    Wl = torch.randn(Bt, 3, 3, generator=torch.Generator().manual_seed(n), dtype=F64)
    s, wd = pts.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    F, valid = ops.solve_fundamental8(s, wd)
    assert bool(valid.all())
    (((F * Wl.float().to(dev)).sum((1, 2))) ** 2).sum().backward()
    x, wt = pts.double().requires_grad_(True), w.double().requires_grad_(True)
    Fo = O.fundamental_8pt(x, wt)
    (((Fo * Wl).sum((1, 2))) ** 2).sum().backward()
    kappa = (Fo * Wl).abs().sum((1, 2)) / (Fo * Wl).sum((1, 2)).abs()
    scale = torch.maximum(x.grad.abs().amax((1, 2)), wt.grad.abs().amax(1))
    tol = 8 * U32 * (1 + kappa) * scale + 1e-9 * scale
    ex = (s.grad.cpu().double() - x.grad).abs().amax((1, 2))
    ew = (wd.grad.cpu().double() - wt.grad).abs().amax(1)
    assert bool((ex <= tol).all()), _excess(ex, tol)
    assert bool((ew <= tol).all()), _excess(ew, tol)
    if n > 8:
        assert float((wt.grad.abs().amax(1) / scale).min()) > 1e-4


def _weighted_train(dev, dtype):
    from differentiable_ransac_amd import estimators, samplers, scorings
    from differentiable_ransac_amd.ransac import RANSAC
    gd = load_golden("ransac_train_f8_weighted")
    B = gd["gumbels"].shape[1]
    r = RANSAC(estimators.FundamentalMatrixEstimatorNew("cuda"), samplers.GumbelSoftmaxSampler(B, 8, device="cuda", data_type=dtype),
               scorings.MSACScore("cuda"), train=True, ransac_batch_size=B, fmat=True, sampler_id=3, weighted=1,
               threshold=0.75, max_iterations=100)
    eye = torch.eye(3, dtype=dtype, device=dev)
    logits = gd["logits"].to(dev, dtype).requires_grad_(True)
    models, _, _, _ = r(gd["matches"].to(dev, dtype), logits, eye, eye, None, gumbels=[x.to(dev, dtype) for x in gd["gumbels"]])
    return gd, logits, torch.cat([models[k] for k in sorted(models)])


def test_weighted_f8_train_f32_chosen_models(dev):
    """The drop-in weighted train call (-fmat 1 -sam 3 -wei 1 -tr 1) in f32 on the reference's ransac_train_f8_weighted run.

    The soft weights of this run span 1e-5 .. 0.76, so the weighted normal equations are ill-conditioned: the reference's
    f32 LAPACK answer and the f64 one differ by O(1) on some samples (the f64 oracle differs from the fixture by 2.2).  The
    kernel solves in f64 from the f32 samples, so its models are held to the f64 oracle on the same f32 inputs, and to the
    reference's chosen models up to the reference's own f32 error (u times the conditioning of its normal equations)."""
    gd, _, chosen = _weighted_train(dev, torch.float32)
    c = chosen.detach().cpu().double()
    assert c.shape == gd["chosen"].shape
    m64 = gd["matches"].double()
    o64 = torch.cat([O.ransac_train_batch(m64, gd["logits"].double(), x.double(), None, "f8", weighted=True)[0]
                     for x in gd["gumbels"]])

    def aligned(a, ref):
        s = torch.sign((a * ref).sum((-1, -2)))
        return (a * s[:, None, None] - ref).abs().amax((-1, -2)) / ref.abs().amax((-1, -2))
    # per sample: the kernel's inputs (samples times the straight-through value, soft weights) are f32, i.e. the rows of
    # the weighted design matrix A carry a relative error u; the null vector moves by u sigma_max / (sigma_8 - sigma_9) of
    # A, i.e. u sqrt(lambda_max / (lambda_8 - lambda_9)) of the normal matrix A^T A: tol = 64 u sqrt(kappa)
    kap = []
    for x in gd["gumbels"]:
        _, ret, y = O.gumbel_topk(gd["logits"].double(), x.double(), 1.0, 8)
        smp, w = O.gather_samples(m64, ret, y)
        nrm, _, _ = O.hartley_normalize(smp)
        A = O._f_rows(nrm, w)
        lam = torch.linalg.eigvalsh(A.transpose(-1, -2) @ A)
        kap.append(lam[:, -1] / (lam[:, 1] - lam[:, 0]))
    tol = 64 * U32 * torch.cat(kap).sqrt()
    err64 = aligned(c, o64)
    assert bool((err64 <= tol).all()), _excess(err64, tol)
    # against the reference: it solved the normal equations in f32, whose error is u kappa (not u sqrt(kappa)): so
    # |kernel - reference| <= tol + 64 u kappa (+ 1e-4, and 10 % for the two normalisations).  On this run kappa >= 975,
    # so the bound is at least 4e-3: a loose check; the f32 LAPACK answer itself depends on the CPU
    # library, so the oracle run in f32 is no fixed yardstick either: the tight check is the one against o64 above
    ref = gd["chosen"].double()
    bound = 1.1 * (tol + 64 * U32 * torch.cat(kap)) + 1e-4
    err_ref = aligned(c, ref)
    assert bool((err_ref <= bound).all()), _excess(err_ref, bound)


def test_weighted_f8_train_f64_logits_gradient(dev):
    """The same call in f64 (-pr 2): logits gradient against f64 autograd of the oracle, to a rounding-level tolerance (as
    test_gpu_round4's unweighted check).  Not compared in f32: there the ill-conditioned weighted solve (see the test above)
    makes the f32 reference and the f64 arbiter disagree at O(1)."""
    gd, logits, chosen = _weighted_train(dev, torch.float64)
    assert chosen.dtype == F64
    l64 = gd["logits"].double().requires_grad_(True)
    o64 = torch.cat([O.ransac_train_batch(gd["matches"].double(), l64, x.double(), None, "f8", weighted=True)[0]
                     for x in gd["gumbels"]])
    s = torch.sign((chosen.detach().cpu() * o64.detach()).sum((-1, -2)))
    rel = (chosen.detach().cpu() * s[:, None, None] - o64.detach()).abs().amax((-1, -2)) / o64.detach().abs().amax((-1, -2))
    assert rel.max() < 1e-6, float(rel.max())
    w = torch.randn(o64.shape, generator=torch.Generator().manual_seed(11), dtype=F64)
    (o64 * w).sum().backward()
    (chosen * (w * s[:, None, None]).to(dev)).sum().backward()
    gl = logits.grad.cpu()
    assert bool(torch.isfinite(gl).all()) and float(l64.grad.abs().max()) > 0
    assert (gl - l64.grad).abs().max() <= 1e-8 * l64.grad.abs().max(), (float((gl - l64.grad).abs().max()),
                                                                         float(l64.grad.abs().max()))


# ------------------------------------------------------------------------------------------------------- K4 backward
def _msac_data(P, N, M, seed):
    """normalised two-view matches [P,N,4], models near the ground truth [P,M,3,3] and per-pair thresholds (about 40 % of
    the (model, point) pairs inliers), with every point that lies within a relative 1e-3 of (1.5 thr)^2 for some model
    replaced by a fresh random one (repeated until there are none): the f32 kernel and the f64 arbiter then agree on
    every inlier decision."""
    from differentiable_ransac_amd import synth
    from tests.test_oracle_gradients import _d2_ratio
    g = torch.Generator().manual_seed(seed)
    data = synth.batch_two_view(P, max(N, 8), seed0=seed, dtype=F64)
    matches = data["matches"][:, :N].clone()
    models = data["gt_E"][:, None] + 0.02 * torch.randn(P, M, 3, 3, generator=g, dtype=F64)
    models = models.float().double()
    thr = torch.empty(P, dtype=F64)
    replaced = 0
    for p in range(P):
        thr[p] = float(_d2_ratio(matches[p], models[p], 1.0).sqrt().flatten().quantile(0.4))
        thr[p] = float(thr[p].float())
        for _ in range(50):
            m32 = matches[p].float().double()
            near = ((_d2_ratio(m32, models[p], float(thr[p])) - 1).abs() < 1e-3).any(0)
            if not bool(near.any()):
                break
            replaced += int(near.sum())
            matches[p, near] = torch.rand(int(near.sum()), 4, generator=g, dtype=F64) * 0.5 - 0.25
        else:
            raise AssertionError("could not clear the threshold band")
    return matches.float(), models.float(), thr.float(), replaced


def _msac_bound(matches, models, thr, g):
    """f32 error bound of msac_bwd_kernel per model entry [M,3,3], in units of u.  Per inlier point the kernel adds
    c1 X2 X1^T - c2 (X2 a^T + b X1^T), c1 = 2 r / jj, c2 = 2 r^2 / jj^2, with a = F^T x2, b = F x1 (first two entries),
    r = x1 . a, jj = |a|^2 + |b|^2 each a chain of 2-3 fmas:
        |da| <= 4 |F|^T |x2|, |db| <= 4 |F| |x1|, |dr| <= 4 rho (rho = sum |x1_j F_ij x2_i|), |djj| <= 2 (|a| |da| + |b| |db|),
        |dc1| <= 2 |dr| / jj + 2 |r| |djj| / jj^2,  |dc2| <= 4 |r| |dr| / jj^2 + 4 r^2 |djj| / jj^3,
    plus (depth + 3) |term| for the products and the sum (8 points a lane, 6 wave levels, 4 waves, one partial per
    2048-point chunk); all times |g| / (1.5 thr)^2."""
    N = matches.shape[0]
    depth = 8 + 6 + 2 + math.ceil(N / 2048)
    one = torch.ones(N, 1, dtype=F64)
    X1, X2 = torch.cat((matches[:, :2], one), 1), torch.cat((matches[:, 2:], one), 1)      # [N,3]
    Fa = models.abs()
    a = (X2 @ models)[..., :2]                        # [M,N,2]: a_j = sum_i x2_i F_ij
    b = (X1 @ models.transpose(-1, -2))[..., :2]      # [M,N,2]: b_i = sum_j F_ij x1_j
    da = 4 * (X2.abs() @ Fa)[..., :2]
    db = 4 * (X1.abs() @ Fa.transpose(-1, -2))[..., :2]
    r = (X1[None] * (X2 @ models)).sum(-1)            # [M,N]
    dr = 4 * (X1.abs()[None] * (X2.abs() @ Fa)).sum(-1)
    jj = (a * a).sum(-1) + (b * b).sum(-1)
    djj = 2 * ((a.abs() * da).sum(-1) + (b.abs() * db).sum(-1))
    t2 = (1.5 * thr) ** 2
    inl = (r * r / jj < t2).to(F64)
    c1, c2 = 2 * r.abs() / jj * inl, 2 * r * r / jj ** 2 * inl
    dc1 = (2 * dr / jj + 2 * r.abs() * djj / jj ** 2) * inl
    dc2 = (4 * r.abs() * dr / jj ** 2 + 4 * r * r * djj / jj ** 3) * inl
    z = torch.zeros_like(a[..., :1])
    A, Bv, dA, dB = (torch.cat((v, z), -1) for v in (a.abs(), b.abs(), da, db))
    X1a, X2a = X1.abs(), X2.abs()

    def outer(cc, u, v, u_m=False, v_m=False):
        return torch.einsum("mn,%s,%s->mij" % ("mni" if u_m else "ni", "mnj" if v_m else "nj"), cc, u, v)
    term = outer(c1, X2a, X1a) + outer(c2, X2a, A, v_m=True) + outer(c2, Bv, X1a, u_m=True)
    dterm = outer(dc1, X2a, X1a) + outer(dc2, X2a, A, v_m=True) + outer(dc2, Bv, X1a, u_m=True) \
        + outer(c2, X2a, dA, v_m=True) + outer(c2, dB, X1a, u_m=True)
    return (dterm + (depth + 3) * term) * g.abs()[:, None, None] / t2


@pytest.mark.parametrize("N", [1, 7, 2047, 2048, 2049, 5000])
@pytest.mark.parametrize("M", [1, 16, 17, 40])
@pytest.mark.parametrize("P", [1, 3])
def test_msac_score_backward_against_f64_autograd(dev, P, M, N):
    """dr_msac_score_bwd_f32 (ops.msac_score_autograd) against f64 autograd of O.msac_score, per-pair thresholds; an
    all-zero and a NaN model row (M >= 17) leave the other rows' gradients bit-identical and receive exactly zero (their
    Sampson distance is 0/0 = NaN, which the kernel's `d2 < thr^2` test counts as an outlier for every point)."""
    from differentiable_ransac_amd import ops
    matches, models, thr, _ = _msac_data(P, N, M, seed=N + M)
    G = torch.randn(P, M, generator=torch.Generator().manual_seed(P + M + N), dtype=F64)
    md = models.to(dev).requires_grad_(True)
    sc, _ = ops.msac_score_autograd(matches.to(dev), md, thr.to(dev))
    gk, = torch.autograd.grad((sc * G.float().to(dev)).sum(), md)
    gk = gk.cpu().double()
    assert bool(torch.isfinite(gk).all())
    for p in range(P):
        x = models[p].double().requires_grad_(True)
        so, _ = O.msac_score(matches[p].double(), x, float(thr[p]))
        go, = torch.autograd.grad((so * G[p]).sum(), x)
        tol = U32 * _msac_bound(matches[p].double(), models[p].double(), float(thr[p]), G[p]) + 1e-30
        err = (gk[p] - go).abs()
        assert bool((err <= tol).all()), (p, _excess(err, tol))
    if M >= 17:
        bad = models.clone()
        bad[:, 3] = 0.0
        bad[:, 16] = float("nan")
        mb = bad.to(dev).requires_grad_(True)
        sb, _ = ops.msac_score_autograd(matches.to(dev), mb, thr.to(dev))
        gb, = torch.autograd.grad((sb * G.float().to(dev)).sum(), mb)
        gb = gb.cpu().double()
        keep = torch.ones(M, dtype=torch.bool)
        keep[[3, 16]] = False
        assert torch.equal(gb[:, keep], gk[:, keep])
        assert float(gb[:, 3].abs().max()) == 0.0 and float(gb[:, 16].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------- pose error f32
def test_pose_loss_backward_f32_against_f64_autograd(dev):
    """PoseLoss (Horn, keep mask) in f32, P = 3, M = 60, against f64 autograd of O.pose_loss over each pair's kept models
    (on the f32 values of the models).  pose_error_bwd_kernel<float> differentiates in f64 dual numbers from the f32 models;
    what is f32 is the upstream (keep / count / P / 2: one rounding) and the store: tol = 4 u |g_ref| per entry, plus
    1e-9 |g_ref|_model for the f64 evaluation.  Compared: kept models whose kernel candidate equals the oracle's (the vote
    is made from f32 points) and that lie away from the ground truth (err_R > 1e-3, arccos singular there); the models that
    are not kept receive exactly zero."""
    from differentiable_ransac_amd import ops, synth
    from differentiable_ransac_amd.loss import PoseLoss
    P, N, M = 3, 500, 60
    data = synth.batch_two_view(P, N, seed0=90, dtype=F64)
    g = torch.Generator().manual_seed(90)
    models = (data["gt_E"][:, None] + 0.1 * torch.randn(P, M, 3, 3, generator=g, dtype=F64)).float()
    keep = torch.rand(P, M, generator=g) > 0.3
    m32 = data["matches"].float()
    md = models.to(dev).requires_grad_(True)
    loss = PoseLoss()(md, m32[..., :2].to(dev), m32[..., 2:].to(dev), data["R"].float().to(dev), data["t"].float().to(dev),
                      keep=keep.to(dev))
    loss.backward()
    gk = md.grad.cpu().double()
    _, _, which_k, _ = ops.pose_error(m32.to(dev), models.to(dev), data["R"].float().to(dev), data["t"].float().to(dev))
    which_k = which_k.cpu()
    assert float(gk[~keep].abs().max()) == 0.0
    compared = 0
    mo = [models[p][keep[p]].double().requires_grad_(True) for p in range(P)]
    O.pose_loss(mo, m32.double(), data["R"].float().double(), data["t"].float().double()).backward()
    for p in range(P):
        eq, _, wo = O.pose_error(mo[p].detach(), m32[p].double(), data["R"][p].float().double(), data["t"][p].float().double())
        sel = (which_k[p][keep[p]].long() == wo) & (eq > 1e-3)
        ref = mo[p].grad
        tol = 4 * U32 * ref.abs() + 1e-9 * ref.abs().amax((1, 2), keepdim=True)
        err = (gk[p][keep[p]] - ref).abs()
        assert bool((err[sel] <= tol[sel]).all()), (p, _excess(err[sel], tol[sel]))
        compared += int(sel.sum())
    assert compared >= 0.8 * int(keep.sum()), (compared, int(keep.sum()))
