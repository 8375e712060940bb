"""f64 reference of the differentiable soft-inlier score of the registration path (dr_registration_soft_score,
dr_registration_soft_score_bwd; ops.registration_soft_score) and of loss.RegistrationExpectedLoss, written from the definition and not
from the kernels.  Scenes come from tests/registration_ref.py.

    d = R p + t - q,  d2 = |d|^2,  a = beta (1 - d2 / thr^2)
    live = d2 finite and a >= -40,   w = live ? 1 / (1 + exp(-a)) : 0,   score[p,m] = sum over the masked points of w
    g = 2 grad_scores[p,m] (-beta / thr^2) w (1 - w) per live term
    d / d t = sum_n g d,  d / d R = sum_n g d p^T (row 3 zero);   d / d p = sum_m R^T (g d),  d / d q = sum_m -g d

A slot keep drops scores 0 and has no gradient; so does a kept model with a non-finite entry, and a pair whose threshold is not > 0.
The definition is written twice: closed form in numpy (value and both gradients) and as a plain f64 torch expression for autograd;
tests/test_registration_soft_score_host.py holds one against the other and against central differences.

The expected loss (loss.RegistrationExpectedLoss) is PnPExpectedLoss's definition on these scores, in f64 torch: probs =
softmax(alpha score / N_p) over the usable slots (kept, finite), l = min(max(RRE in degrees, trans_weight RTE), max_loss) with the
arc-cosine's argument clamped to +-(1 - 1e-6) and RTE = sqrt(|dt|^2 + 1e-24), loss = mean over the pairs of sum_m probs l;
trans_weight = 50 is the default here.  The slots of these cases come within 1e-3 rad of the pose, where acos(c) itself loses
eps / (1 - c) = 4e-10 of the angle: `pose_errors` takes the half-angle from 1 - c = |R - R_gt|^2_F / 4 (see there).

Tolerances (tests/test_gpu_registration_soft_score.py): the protocol of tests/pnp_soft_score_ref.py.  No bound comes from a kernel:
`compare` measures, per score / per model / per point, the reference on inputs as the kernel receives them (pnp_ref.as_kernel_input),
its result rounded the same way, against the reference on the originals, and allows TOL_FACTOR = 8 times that with a floor of one eps
of the type times the number of scored points (scores) or times the row's largest entry (gradients).  A point within that measured
deviation of the a = -40 cutoff may be live on one side only: `bands` adds its own term to the bound of whatever it enters."""
import numpy as np
import torch

from tests import pnp_ref as R
from tests import registration_ref as G
from tests.pnp_soft_score_ref import ACOS_MAX, RTE_EPS2, compare  # noqa: F401  (one protocol for both families)

BETA = 5.0
CUTOFF = -40.0
THRESHOLD = G.THRESHOLD
LOSS = dict(alpha=100.0, trans_weight=50.0, max_loss=100.0)
# (P, N, M) of the GPU tests: a lane block plus a ragged tail both ways; across the 256-point tile by 44 (with a mask) and by 1; across
# the 512-model tile of the transposed pass (twice, and ragged)
CASES = [(3, 70, 80), (2, 300, 260), (1, 257, 1100)]
THR_PAIRS = (1.0, 0.8, 1.25)


# ------------------------------------------------------------------------------------------------ the cases
def _moved(T, rng, angle, shift):
    """the pose turned by `angle` rad about a random axis and moved by `shift` in a random direction"""
    w, d = rng.normal(size=3), rng.normal(size=3)
    return R.pose(R.rot(w * angle / np.linalg.norm(w)) @ T[:3, :3], T[:3, 3] + d * shift / np.linalg.norm(d))


def case(P, N, M, seed=43):
    """-> dict(m [P,N,6], models [P,M,4,4], keep [P,M], mask [P,N] | None, thr [P], poses [P,4,4]).  Points of unit scale under a
    random pose (registration_ref.scene: 60 % inliers with 5 mm of noise, outliers in a 4 m cube), threshold 0.05 times THR_PAIRS; the
    second pair of a case with P > 1 has threshold 0.  Slots: the generating pose turned and moved by 10^U(-3, -0.7) (rad and length:
    displacements from a fiftieth of the threshold to four times it, so that the weights span (0, 1) and part of the inliers falls
    beyond the cutoff at three thresholds), every eighth a random pose, every seventh dropped; then the generating pose, a slightly
    moved one, one moved by three thresholds (the cutoff: inliers on both sides of it) and a kept model with a NaN or inf entry.  Every dropped slot
    holds NaN.  The mask (the second case only) drops about a third of the points."""
    rng = np.random.default_rng(seed + 1000 * N + M)
    ms, mo, kp, poses = [], [], [], []
    for p in range(P):
        sc = G.scene(seed + 17 * p + N, N, 0.6)
        T = R.pose(sc["R"], sc["t"])
        models = np.empty((M, 4, 4))
        for j in range(M - 4):
            s = 10.0 ** rng.uniform(-3.0, -0.7)
            models[j] = R.pose(G.random_rotation(rng), rng.standard_normal(3)) if j % 8 == 5 else _moved(T, rng, s, s)
        valid = np.ones(M, bool)
        valid[:M - 4:7] = False
        bad = T.copy()
        bad[1, 2] = np.inf if p % 2 else np.nan
        models[M - 4:] = np.stack([T, _moved(T, rng, 0.004, 0.004), _moved(T, rng, 0.0, 3.0 * THRESHOLD * THR_PAIRS[p % 3]), bad])
        models[~valid] = np.nan
        ms.append(sc["matches"]), mo.append(models), kp.append(valid), poses.append(T)
    thr = THRESHOLD * np.array([THR_PAIRS[p % 3] for p in range(P)])
    if P > 1:
        thr[1] = 0.0
    mask = (rng.random((P, N)) < 0.67) if (P, N, M) == CASES[1] else None
    return dict(m=np.stack(ms), models=np.stack(mo), keep=np.stack(kp), mask=mask, thr=thr, poses=np.stack(poses))


# ------------------------------------------------------------------------------------------------ closed form
def _grid(m, T, thr2, beta):
    """one pair's points m [n,6] under models T [k,4,4] (finite) -> dict of [k,n] arrays, nothing gated by `live` except w.  Evaluated in
    numpy.longdouble: d = R p + t - q cancels from |q| ~ 2 to a fraction of the threshold and a / thr2 multiplies what is left by
    2000, so in f64 the reference itself would carry as much error as the one-ulp change of the inputs that it is used to measure (and
    more than an f64 kernel with a compensated residual has); the sums are rounded to f64 by the callers"""
    LD = np.longdouble
    m, T, thr2, beta = np.asarray(m, LD), np.asarray(T, LD), LD(thr2), LD(beta)
    with np.errstate(all="ignore"):
        d = np.einsum("kij,nj->kni", T[:, :3, :3], m[:, :3]) + T[:, None, :3, 3] - m[None, :, 3:]
        d2 = (d * d).sum(-1)
        a = beta * (LD(1) - d2 / thr2)
        live = np.isfinite(d2) & (a >= CUTOFF)
        sig = LD(1) / (LD(1) + np.exp(-np.where(np.isfinite(a), np.maximum(a, LD(-700)), LD(-700))))      # the weight WITHOUT the cutoff
    return dict(a=a, live=live, sig=sig, w=np.where(live, sig, 0.0), d=d)


def _usable(models, keep, thr, P, M):
    keep = np.ones((P, M), bool) if keep is None else np.asarray(keep, bool)
    thr2 = np.broadcast_to(np.asarray(thr, np.float64) ** 2, (P,))
    with np.errstate(invalid="ignore"):
        return keep & np.isfinite(models[:, :, :3]).all((2, 3)) & (thr2 > 0)[:, None], thr2


def soft_score(m, mask, models, keep, thr, beta=BETA, grad_scores=None):
    """m [P,N,6], mask [P,N] bool | None, models [P,M,4,4], keep [P,M] bool | None, thr = distance (scalar or [P]) -> scores [P,M];
    with grad_scores [P,M] (entries of unusable slots are never read) -> (scores, grad_models [P,M,4,4], grad_matches [P,N,6])"""
    (P, N, _), M = m.shape, models.shape[1]
    mask = np.ones((P, N), bool) if mask is None else np.asarray(mask, bool)
    use, thr2 = _usable(models, keep, thr, P, M)
    scores, gm, gx = np.zeros((P, M)), np.zeros((P, M, 4, 4)), np.zeros((P, N, 6))
    for p in range(P):
        js, ns = np.flatnonzero(use[p]), np.flatnonzero(mask[p])
        if not len(js) or not len(ns):
            continue
        T, pts = models[p, js], m[p, ns]
        G_ = _grid(pts, T, thr2[p], beta)
        scores[p, js] = G_["w"].sum(1)
        if grad_scores is None:
            continue
        g2 = 2.0 * grad_scores[p, js][:, None] * (-beta / thr2[p]) * G_["w"] * (1.0 - G_["w"])
        with np.errstate(invalid="ignore"):                                                       # (0 x inf behind the gate)
            gd = np.where(G_["live"][..., None], g2[..., None] * G_["d"], 0.0)                    # [k,n,3]
        gm[p, js, :3, 3] = gd.sum(1)
        gm[p, js, :3, :3] = np.einsum("kni,nj->kij", gd, pts[:, :3])
        gx[p, ns, :3] = np.einsum("kij,kni->nj", T[:, :3, :3], gd)
        gx[p, ns, 3:] = -gd.sum(0)
    return scores if grad_scores is None else (scores, gm, gx)


def bands(m, mask, models, keep, thr, beta, grad_scores, width_a):
    """what the points whose `live` decision a deviation of width_a in a (at the cutoff) can turn move at most: (scores [P,M],
    grad_models rows [P,M], grad_matches rows [P,N]): the sum of the points' own terms, evaluated without the gate (the largest
    |entry| of the term for the gradients)"""
    (P, N, _), M = m.shape, models.shape[1]
    mask = np.ones((P, N), bool) if mask is None else np.asarray(mask, bool)
    use, thr2 = _usable(models, keep, thr, P, M)
    bs, bm, bx = np.zeros((P, M)), np.zeros((P, M)), np.zeros((P, N))
    for p in range(P):
        js, ns = np.flatnonzero(use[p]), np.flatnonzero(mask[p])
        if not len(js) or not len(ns):
            continue
        T, pts = models[p, js], m[p, ns]
        G_ = _grid(pts, T, thr2[p], beta)
        with np.errstate(all="ignore"):
            near = np.abs(G_["a"] - CUTOFF) <= width_a
            g2 = np.abs(2.0 * grad_scores[p, js][:, None] * (beta / thr2[p]) * G_["sig"] * (1.0 - G_["sig"]))
            gd = np.nan_to_num(g2[..., None] * np.abs(G_["d"]), nan=0.0, posinf=0.0)
            tm = gd.max(-1) * np.maximum(1.0, np.abs(pts[:, :3]).max(1))[None]
            tx = np.maximum(np.einsum("kij,kni->knj", np.abs(T[:, :3, :3]), gd).max(-1), gd.max(-1))
        bs[p, js] = np.where(near, G_["sig"], 0.0).sum(1)
        bm[p, js] = np.where(near, tm, 0.0).sum(1)
        bx[p, ns] = np.where(near, tx, 0.0).sum(0)
    return bs, bm, bx


def cutoff_widths(m, mk, models, ok, keep, thr, tk, beta):
    """the reference's own deviation of a (among the points within 20 of the cutoff) between the originals and the inputs as the
    kernel receives them, times TOL_FACTOR: the width `bands` takes"""
    (P, _, _), M = m.shape, models.shape[1]
    use, thr2 = _usable(models, keep, thr, P, M)
    t2k = np.broadcast_to(np.asarray(tk, np.float64) ** 2, (P,))
    wa = 0.0
    for p in range(P):
        js = np.flatnonzero(use[p])
        if not len(js) or not t2k[p] > 0:
            continue
        A, B = _grid(m[p], models[p, js], thr2[p], beta), _grid(mk[p], ok[p, js], t2k[p], beta)
        with np.errstate(all="ignore"):
            da = np.abs(A["a"] - B["a"])[np.isfinite(A["a"]) & np.isfinite(B["a"]) & (np.abs(A["a"] - CUTOFF) < 20.0)]
        wa = max(wa, float(da.max()) if da.size else 0.0)
    return R.TOL_FACTOR * wa


# ------------------------------------------------------------------------------------------------ f64 torch, for autograd
def torch_soft_score(m, mask, models, keep, thr, beta=BETA):
    """the definition as a plain f64 torch expression (no formula of a gradient): tensors m [P,N,6], models [P,M,4,4]; mask, keep bool
    tensors or None; thr a float or a [P] array -> scores [P,M]"""
    (P, N, _), M = m.shape, models.shape[1]
    thr2 = torch.as_tensor(np.broadcast_to(np.asarray(thr, np.float64) ** 2, (P,)).copy())
    use = torch.isfinite(models[:, :, :3]).all(-1).all(-1) & (thr2 > 0)[:, None]
    if keep is not None:
        use = use & keep
    safe = torch.where(use[:, :, None, None], models, torch.zeros_like(models))
    d = torch.einsum("pmij,pnj->pmni", safe[:, :, :3, :3], m[:, :, :3]) + safe[:, :, None, :3, 3] - m[:, None, :, 3:]
    d2 = (d * d).sum(-1)
    t2 = torch.where(thr2 > 0, thr2, torch.ones_like(thr2))[:, None, None]
    a = beta * (1.0 - d2 / t2)
    live = torch.isfinite(d2) & (a >= CUTOFF) & use[:, :, None]
    w = torch.where(live, torch.sigmoid(torch.where(live, a, torch.zeros_like(a))), torch.zeros_like(a))
    if mask is not None:
        w = w * mask[:, None, :].to(w.dtype)
    return w.sum(-1)


# ------------------------------------------------------------------------------------------------ the expected loss
def pose_errors(models, gt_pose, trans_weight, max_loss):
    """l [P,M] in f64 torch.  RRE = acos(c), c = (tr(Rg^T R) - 1) / 2 clamped to +-ACOS_MAX, evaluated without the cancellation of c at a
    small angle: for two rotations 1 - c = |R - Rg|_F^2 / 4 =: q (clamped to 1 -+ ACOS_MAX), sin^2(theta / 2) = q / 2 and
    cos^2(theta / 2) = 1 - q / 2, so theta = 2 atan2(sqrt(q / 2), sqrt(1 - q / 2)), each factor good to an eps of itself"""
    D = models[..., :3, :3] - gt_pose[:, None, :3, :3]
    q = ((D * D).sum((-1, -2)) / 4.0).clamp(1.0 - ACOS_MAX, 1.0 + ACOS_MAX)
    rre = torch.rad2deg(2.0 * torch.atan2(torch.sqrt(q / 2.0), torch.sqrt(1.0 - q / 2.0)))
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
