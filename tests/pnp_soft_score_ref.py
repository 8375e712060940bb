"""f64 reference of the differentiable soft-inlier score of the absolute-pose path (dr_pnp_soft_score, dr_pnp_soft_score_bwd;
ops.pnp_soft_score) and of loss.PnPExpectedLoss, written from the definition and not from the kernels.  Scenes and P3P poses come from
tests/pnp_ref.py.

    x_c = R X + t,  d2 = (x_c / z_c - u)^2 + (y_c / z_c - v)^2,  a = beta (1 - d2 / thr^2)
    live = z_c > 0 and d2 finite and a >= -40,   w = live ? 1 / (1 + exp(-a)) : 0,   score[p,m] = sum over the masked points of w
    g = grad_scores[p,m] (-beta / thr^2) w (1 - w),   h = (e_0 i, e_1 i, -(e_0 x + e_1 y) i),   i = 1 / z_c
    d / d t = sum_n 2 g h,  d / d R = sum_n 2 g h X^T (row 3 zero);   d / d X = sum_m R^T (2 g h),  d / d (u, v) = sum_m -2 g e

A slot keep drops scores 0 and has no gradient; so does a kept model with a non-finite entry, and a pair whose threshold is not > 0.
The definition is written twice: closed form in numpy (value and both gradients) and as a plain f64 torch expression for autograd;
tests/test_pnp_soft_score_host.py holds one against the other and against central differences.

The expected loss (loss.PnPExpectedLoss) in f64 torch: probs = softmax(alpha score / N_p) over the usable slots (kept, finite),
l = min(max(RRE in degrees, trans_weight RTE), max_loss) with acos's argument clamped to +-(1 - 1e-6) and RTE = sqrt(|dt|^2 + 1e-24),
loss = mean over the pairs of sum_m probs l.

Tolerances (tests/test_gpu_pnp_soft_score.py).  As in tests/pnp_ref.py no bound comes from a kernel: `compare` measures, per score / per
model / per point, the reference on inputs as the kernel receives them (pnp_ref.as_kernel_input), its result rounded the same way,
against the reference on the originals, and allows TOL_FACTOR = 8 times that with a floor of one eps of the type times the number of
scored points (scores) or times the row's largest entry (gradients).  A point within that measured deviation of the a = -40 cutoff or
of z_c = 0 may be live on one side only: `bands` adds its own term to the bound of whatever it enters."""
import numpy as np
import torch

from tests import pnp_ref as R

BETA = 5.0
CUTOFF = -40.0
ACOS_MAX = 1.0 - 1e-6
RTE_EPS2 = 1e-24
# (P, N, M) of the GPU tests: a lane block plus a ragged tail both ways; across the 256-point tile (with a mask); across the 512-model
# tile of the transposed pass (twice, and ragged)
CASES = [(3, 70, 80), (2, 300, 260), (1, 257, 1100)]
THR_PAIRS = (1.0, 0.8, 1.25)


# ------------------------------------------------------------------------------------------------ the cases
def case(P, N, M, seed=41):
    """-> dict(m [P,N,5], models [P,M,4,4], keep [P,M], mask [P,N] | None, thr [P], poses [P,4,4]).  Slots: the P3P poses of random
    samples (60 % inliers: good and wild ones; a sample's unused slots are dropped), every seventh of them dropped too; then the
    generating pose, a slightly perturbed one, the generating pose moved 5 back along the axis (points at depth 3..7: part of them
    behind the camera) and a kept model with a NaN entry.  Every dropped slot holds NaN.  The mask (the second case only) drops about a
    third of the points."""
    rng = np.random.default_rng(seed + 1000 * N + M)
    B = (M - 4 + 3) // 4
    ms, mo, kp, poses = [], [], [], []
    for p in range(P):
        sc = R.scene(seed + 17 * p + N, N, 0.6)
        m, T = sc["matches"], sc["pose"]
        idx = np.stack([rng.permutation(N)[:3] for _ in range(B)])
        models, valid, _ = R.slots(m, idx)
        models, valid = models[:M - 4].copy(), valid[:M - 4].copy()
        valid[::7] = False
        back = T.copy()
        back[2, 3] -= 5.0
        bad = T.copy()
        bad[1, 2] = np.inf if p % 2 else np.nan
        models = np.concatenate([models, np.stack([T, R.perturbed(T, rng, 0.2, 0.002), back, bad])])
        valid = np.concatenate([valid, [True] * 4])
        models[~valid] = np.nan
        ms.append(m), mo.append(models), kp.append(valid), poses.append(T)
    thr = R.THRESHOLD * np.array([THR_PAIRS[p % 3] for p in range(P)])
    mask = (rng.random((P, N)) < 0.67) if (P, N, M) == CASES[1] else None
    return dict(m=np.stack(ms), models=np.stack(mo), keep=np.stack(kp), mask=mask, thr=thr, poses=np.stack(poses))


# ------------------------------------------------------------------------------------------------ closed form
def _grid(m, T, thr2, beta):
    """one pair's points m [n,5] under models T [k,4,4] (finite) -> dict of [k,n] arrays, nothing gated by `live` except w.  Evaluated in
    numpy.longdouble: e = x_c / z_c - u cancels by two to three orders and a / thr2 multiplies what is left by 2e5, so in f64 the reference
    itself would carry as much error as the one-ulp change of the inputs that it is used to measure (and more than an f64 kernel with
    a compensated residual has); the sums are rounded to f64 by the callers"""
    LD = np.longdouble
    m, T, thr2, beta = np.asarray(m, LD), np.asarray(T, LD), LD(thr2), LD(beta)
    with np.errstate(all="ignore"):
        xc = np.einsum("kij,nj->kni", T[:, :3, :3], m[:, :3]) + T[:, None, :3, 3]
        iz = LD(1) / xc[..., 2]
        x, y = xc[..., 0] * iz, xc[..., 1] * iz
        e0, e1 = x - m[None, :, 3], y - m[None, :, 4]
        d2 = e0 * e0 + e1 * e1
        a = beta * (LD(1) - d2 / thr2)
        live = (xc[..., 2] > 0) & np.isfinite(d2) & (a >= CUTOFF)
        sig = LD(1) / (LD(1) + np.exp(-np.where(np.isfinite(a), np.maximum(a, LD(-700)), LD(-700))))      # the weight WITHOUT the cutoff
        h = np.stack([e0 * iz, e1 * iz, -(e0 * x + e1 * y) * iz], -1)
    return dict(zc=xc[..., 2], a=a, live=live, sig=sig, w=np.where(live, sig, 0.0), e=np.stack([e0, e1], -1), h=h)


def _usable(models, keep, thr, P, M):
    keep = np.ones((P, M), bool) if keep is None else np.asarray(keep, bool)
    thr2 = np.broadcast_to(np.asarray(thr, np.float64) ** 2, (P,))
    with np.errstate(invalid="ignore"):
        return keep & np.isfinite(models[:, :, :3]).all((2, 3)) & (thr2 > 0)[:, None], thr2


def soft_score(m, mask, models, keep, thr, beta=BETA, grad_scores=None):
    """m [P,N,5], mask [P,N] bool | None, models [P,M,4,4], keep [P,M] bool | None, thr = distance (scalar or [P]) -> scores [P,M];
    with grad_scores [P,M] (entries of unusable slots are never read) -> (scores, grad_models [P,M,4,4], grad_matches [P,N,5])"""
    (P, N, _), M = m.shape, models.shape[1]
    mask = np.ones((P, N), bool) if mask is None else np.asarray(mask, bool)
    use, thr2 = _usable(models, keep, thr, P, M)
    scores, gm, gx = np.zeros((P, M)), np.zeros((P, M, 4, 4)), np.zeros((P, N, 5))
    for p in range(P):
        js, ns = np.flatnonzero(use[p]), np.flatnonzero(mask[p])
        if not len(js) or not len(ns):
            continue
        T, pts = models[p, js], m[p, ns]
        G = _grid(pts, T, thr2[p], beta)
        scores[p, js] = G["w"].sum(1)
        if grad_scores is None:
            continue
        g2 = 2.0 * grad_scores[p, js][:, None] * (-beta / thr2[p]) * G["w"] * (1.0 - G["w"])
        with np.errstate(invalid="ignore"):                                                       # (0 x inf behind the gate)
            gh = np.where(G["live"][..., None], g2[..., None] * G["h"], 0.0)                      # [k,n,3]
            ge = np.where(G["live"][..., None], -g2[..., None] * G["e"], 0.0)
        gm[p, js, :3, 3] = gh.sum(1)
        gm[p, js, :3, :3] = np.einsum("kni,nj->kij", gh, pts[:, :3])
        gx[p, ns, :3] = np.einsum("kij,kni->nj", T[:, :3, :3], gh)
        gx[p, ns, 3:] = ge.sum(0)
    return scores if grad_scores is None else (scores, gm, gx)


def bands(m, mask, models, keep, thr, beta, grad_scores, width_a, width_z):
    """what the points whose `live` decision a deviation of width_a in a (at the cutoff) or of width_z in z_c (at 0) can turn move at
    most: (scores [P,M], grad_models rows [P,M], grad_matches rows [P,N]): the sum of the points' own terms, evaluated without the gate
    (the largest |entry| of the term for the gradients)"""
    (P, N, _), M = m.shape, models.shape[1]
    mask = np.ones((P, N), bool) if mask is None else np.asarray(mask, bool)
    use, thr2 = _usable(models, keep, thr, P, M)
    bs, bm, bx = np.zeros((P, M)), np.zeros((P, M)), np.zeros((P, N))
    for p in range(P):
        js, ns = np.flatnonzero(use[p]), np.flatnonzero(mask[p])
        if not len(js) or not len(ns):
            continue
        T, pts = models[p, js], m[p, ns]
        G = _grid(pts, T, thr2[p], beta)
        with np.errstate(all="ignore"):
            near = ((np.abs(G["a"] - CUTOFF) <= width_a) & (G["zc"] > -width_z)) | (np.abs(G["zc"]) <= width_z)
            g2 = np.abs(2.0 * grad_scores[p, js][:, None] * (beta / thr2[p]) * G["sig"] * (1.0 - G["sig"]))
            gh = np.nan_to_num(g2[..., None] * np.abs(G["h"]), nan=0.0, posinf=0.0)
            tm = gh.max(-1) * np.maximum(1.0, np.abs(pts[:, :3]).max(1))[None]
            tx = np.maximum(np.abs(np.einsum("kij,kni->knj", np.abs(T[:, :3, :3]), gh)).max(-1),
                            np.nan_to_num(g2[..., None] * np.abs(G["e"]), nan=0.0, posinf=0.0).max(-1))
        bs[p, js] = np.where(near, G["sig"], 0.0).sum(1)
        bm[p, js] = np.where(near, tm, 0.0).sum(1)
        bx[p, ns] = np.where(near, tx, 0.0).sum(0)
    return bs, bm, bx


def cutoff_widths(m, mk, models, ok, keep, thr, tk, beta):
    """the reference's own deviation of a (among the points within 20 of the cutoff) and of z_c between the originals and the inputs as
    the kernel receives them, times TOL_FACTOR: the widths `bands` takes"""
    (P, _, _), M = m.shape, models.shape[1]
    use, thr2 = _usable(models, keep, thr, P, M)
    t2k = np.broadcast_to(np.asarray(tk, np.float64) ** 2, (P,))
    wa = wz = 0.0
    for p in range(P):
        js = np.flatnonzero(use[p])
        if not len(js):
            continue
        A, B = _grid(m[p], models[p, js], thr2[p], beta), _grid(mk[p], ok[p, js], t2k[p], beta)
        with np.errstate(all="ignore"):
            da = np.abs(A["a"] - B["a"])[np.isfinite(A["a"]) & np.isfinite(B["a"]) & (np.abs(A["a"] - CUTOFF) < 20.0)]
        wa, wz = max(wa, float(da.max()) if da.size else 0.0), max(wz, float(np.abs(A["zc"] - B["zc"]).max()))
    return R.TOL_FACTOR * wa, R.TOL_FACTOR * wz


# ------------------------------------------------------------------------------------------------ f64 torch, for autograd
def torch_soft_score(m, mask, models, keep, thr, beta=BETA):
    """the definition as a plain f64 torch expression (no formula of a gradient): tensors m [P,N,5], models [P,M,4,4]; mask, keep bool
    tensors or None; thr a float or a [P] array -> scores [P,M]"""
    (P, N, _), M = m.shape, models.shape[1]
    thr2 = torch.as_tensor(np.broadcast_to(np.asarray(thr, np.float64) ** 2, (P,)).copy())
    use = torch.isfinite(models[:, :, :3]).all(-1).all(-1) & (thr2 > 0)[:, None]
    if keep is not None:
        use = use & keep
    safe = torch.where(use[:, :, None, None], models, torch.zeros_like(models))
    xc = torch.einsum("pmij,pnj->pmni", safe[:, :, :3, :3], m[:, :, :3]) + safe[:, :, None, :3, 3]
    front = xc[..., 2] > 0
    z = torch.where(front, xc[..., 2], torch.ones_like(xc[..., 2]))
    d2 = (xc[..., 0] / z - m[:, None, :, 3]) ** 2 + (xc[..., 1] / z - m[:, None, :, 4]) ** 2
    t2 = torch.where(thr2 > 0, thr2, torch.ones_like(thr2))[:, None, None]
    a = beta * (1.0 - d2 / t2)
    live = front & torch.isfinite(d2) & (a >= CUTOFF) & use[:, :, None]
    w = torch.where(live, torch.sigmoid(torch.where(live, a, torch.zeros_like(a))), torch.zeros_like(a))
    if mask is not None:
        w = w * mask[:, None, :].to(w.dtype)
    return w.sum(-1)


def pose_errors(models, gt_pose, trans_weight, max_loss):
    Rm, Rg = models[..., :3, :3], gt_pose[:, None, :3, :3]
    c = ((Rg * Rm).sum((-1, -2)) - 1.0) / 2.0
    rre = torch.rad2deg(torch.acos(c.clamp(-ACOS_MAX, ACOS_MAX)))
    d = models[..., :3, 3] - gt_pose[:, None, :3, 3]
    rte = torch.sqrt((d * d).sum(-1) + RTE_EPS2)
    return torch.maximum(rre, trans_weight * rte).clamp(max=max_loss)


def expected_loss(models, scores, n_scored, gt_pose, keep, alpha, trans_weight, max_loss):
    """f64 torch: models [P,M,4,4], scores [P,M], n_scored [P] (or an int), gt_pose [P,4,4], keep [P,M] bool | None ->
    (loss, per_pair [P], probs [P,M])"""
    use = torch.isfinite(models[:, :, :3]).all(-1).all(-1)
    if keep is not None:
        use = use & keep
    n = torch.as_tensor(n_scored, dtype=scores.dtype).reshape(-1, 1).clamp(min=1.0)
    per_pair, probs = [], []
    for p in range(models.shape[0]):                       # pair by pair over the usable slots only: no -inf, no NaN to mask
        js = torch.nonzero(use[p])[:, 0]
        pr = torch.zeros_like(scores[p])
        if len(js) == 0:
            per_pair.append(scores[p].sum() * 0.0), probs.append(pr)
            continue
        q = torch.softmax(alpha * scores[p, js] / n[p if n.shape[0] > 1 else 0], 0)
        ell = pose_errors(models[p:p + 1, js], gt_pose[p:p + 1], trans_weight, max_loss)[0]
        per_pair.append((q * ell).sum()), probs.append(pr.index_put((js,), q))
    per_pair = torch.stack(per_pair)
    return per_pair.mean(), per_pair, torch.stack(probs)


# ------------------------------------------------------------------------------------------------ the comparison
def compare(got, ref, dev, floor, band, what):
    """got, ref, dev [rows, k]: the kernel's rows, the reference's and the reference's on the kernel's inputs (rounded as the kernel
    rounds); floor, band [rows] -> the worst error / bound after printing it; the caller asserts <= 1"""
    got, ref, dev = (np.asarray(a, np.float64).reshape(len(floor), -1) for a in (got, ref, dev))
    err, fig = np.abs(got - ref).max(1), np.abs(dev - ref).max(1)
    bound = np.maximum(R.TOL_FACTOR * fig, floor) + band
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    r = int(ratio.argmax())
    print(f"{what}: worst error / bound {ratio[r]:.3g} at row {r} (error {err[r]:.3g}, measured {fig[r]:.3g}, floor {floor[r]:.3g}, "
          f"band {band[r]:.3g}); rows above the bound {int((ratio > 1).sum())} of {len(ratio)}; in a band {int((band > 0).sum())}")
    return float(ratio[r])
