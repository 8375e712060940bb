"""f64 reference of the differentiable soft-inlier score of the homography path (dr_homography_soft_score,
dr_homography_soft_score_bwd; ops.homography_soft_score) and of loss.HomographyExpectedLoss, written from the definition and not from
the kernels.  Scenes come from tests/homography_ref.py (640-pixel square, 0.5 px of noise, 60 % inliers).

    h = sign(det H) H,  A = adj(H),  y = h (x1, 1),  z = A (x2, 1),  e = x2 - y_xy / y_w,  f = x1 - z_xy / z_w,  d2 = |e|^2 + |f|^2
    a = beta (1 - d2 / thr^2),   live = y_w > 0 and z_w > 0 and d2 finite and a >= -40,   w = live ? 1 / (1 + exp(-a)) : 0
    score[p,m] = sum over the masked points of w
    g = grad_scores[p,m] (-beta / thr^2) w (1 - w) per live term;  with t = y_xy / y_w:  d d2 / d y = (2 / y_w) (-e_0, -e_1, e . t),
    d d2 / d h = that (x) (x1, 1);  the same for z, f, A and x2;  <G, adj(H)> has the derivative eps_jab eps_icd G_ij H_bd at H_ac
    d / d H = sum_n g (sign d d2 / d h + J_adj(H)^T d d2 / d A);   d / d x1 = sum_m g (2 f + h[:, :2]^T d d2 / d y),
    d / d x2 = sum_m g (2 e + A[:, :2]^T d d2 / d z)

A slot keep drops scores 0 and has no gradient; so does a kept model with a non-finite entry or with det = 0, and a pair whose
threshold is not > 0.  The definition is written twice: closed form in numpy (value and both gradients) and as a plain f64 torch
expression for autograd; tests/test_homography_soft_score_host.py holds one against the other and against central differences.

The expected loss (loss.HomographyExpectedLoss) in f64 torch: probs = softmax(alpha score / N_p) over the usable slots (kept, finite,
det != 0), l = min(mean over the four corners of the first image of sqrt(|image under H - image under gt_H|^2 + 1e-12), max_loss), and
max_loss for a model that sends a corner to w <= 0 under the det > 0 sign; loss = mean over the pairs of sum_m probs l.  The corner
errors are written twice as well: `corner_errors` in f64 torch, and `corner_errors_closed_form` (value and gradient in
numpy.longdouble), which `expected_loss` uses.

Tolerances (tests/test_gpu_homography_soft_score.py): the protocol of tests/pnp_soft_score_ref.py.  No bound comes from a kernel:
`compare` measures, per score / per model / per point, the reference on inputs as the kernel receives them (pnp_ref.as_kernel_input),
its result rounded the same way, against the reference on the originals, and allows TOL_FACTOR = 8 times that with a floor of one eps
of the type times the number of scored points (scores) or times the row's largest entry (gradients).  A point within that measured
deviation of the a = -40 cutoff, or of y_w = 0 or z_w = 0, may be live on one side only: `bands` adds its own term to the bound of
whatever it enters."""
import numpy as np
import torch

from tests import homography_ref as G
from tests import pnp_ref as R
from tests.pnp_soft_score_ref import compare  # noqa: F401  (one protocol for the three families)

BETA = 5.0
CUTOFF = -40.0
THRESHOLD = G.THRESHOLD
SIDE = 640.0
SIZE = (SIDE, SIDE)
CORNER_EPS2 = 1e-12
LOSS = dict(alpha=100.0, max_loss=100.0)
MODEL_TILE = 256
# (P, N, M) of the GPU tests: a lane block plus a ragged tail both ways; across the 256-point tile by 44 (with a mask) and by 1; across
# the 256-model tile of the transposed pass (twice, and ragged)
CASES = [(3, 70, 80), (2, 300, 260), (1, 257, 2 * MODEL_TILE + 38)]
THR_PAIRS = (1.0, 0.8, 1.25)
TAIL = 6                                                  # the named slots at the end of every pair (case)
GEN, NEAR, FAR, BAD, SINGULAR, SCALED = -6, -5, -4, -3, -2, -1

_EPS3 = np.zeros((3, 3, 3))
_EPS3[0, 1, 2] = _EPS3[1, 2, 0] = _EPS3[2, 0, 1] = 1.0
_EPS3[0, 2, 1] = _EPS3[2, 1, 0] = _EPS3[1, 0, 2] = -1.0


# ------------------------------------------------------------------------------------------------ the cases
def _moved(H, rng, px):
    """H followed by a rigid motion of the second image that displaces its points by about `px` pixels: a shift of px in a random
    direction and a turn of px / 320 rad about the centre"""
    a, phi, c = rng.choice([-1.0, 1.0]) * px / (0.5 * SIDE), rng.uniform(0.0, 2.0 * np.pi), 0.5 * SIDE
    S = np.array([[np.cos(a), -np.sin(a), px * np.cos(phi)], [np.sin(a), np.cos(a), px * np.sin(phi)], [0.0, 0.0, 1.0]])
    C = np.array([[1.0, 0.0, c], [0.0, 1.0, c], [0.0, 0.0, 1.0]])
    return G.canonical(C @ S @ np.linalg.inv(C) @ H)


def _shifted(H, px):
    return G.canonical(np.array([[1.0, 0.0, px], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) @ H)


def case(P, N, M, seed=47):
    """-> dict(m [P,N,4], models [P,M,3,3], keep [P,M], mask [P,N] | None, thr [P], gt [P,3,3]).  Matches in pixels under a random
    homography (homography_ref.scene: 60 % inliers with 0.5 px of noise, outliers uniform in the square), threshold 3 px times
    THR_PAIRS; the second pair of a case with P > 1 has threshold 0.  Slots: the generating H moved by 3 x 10^U(log10(1/50), log10(4))
    pixels (displacements from a fiftieth of the threshold to four times it, so that the weights span (0, 1) and part of the inliers
    falls beyond the cutoff at three thresholds), every eighth a random homography, every seventh dropped; then the generating H
    (GEN), a slightly moved one (NEAR), one shifted by three thresholds of transfer DISTANCE (FAR: the second image moved by
    3 thr / sqrt(2), which the two transfers see once each, so d2 ~ 9 thr^2 and a ~ -40: inliers on both sides of the cutoff), a kept
    model with a NaN or inf entry (BAD), a kept model with a zero third row (SINGULAR: det = 0 in any arithmetic) and -3 x NEAR (SCALED).
    Every dropped slot holds NaN.  The mask (the second case only) drops about a third of the points."""
    rng = np.random.default_rng(seed + 1000 * N + M)
    ms, mo, kp, gts = [], [], [], []
    for p in range(P):
        sc = G.scene(seed + 17 * p + N, N, 0.6)
        H = sc["H"]
        t = THRESHOLD * THR_PAIRS[p % 3]
        models = np.empty((M, 3, 3))
        for j in range(M - TAIL):
            s = THRESHOLD * 10.0 ** rng.uniform(np.log10(1.0 / 50.0), np.log10(4.0))
            models[j] = G.random_h(rng) if j % 8 == 5 else _moved(H, rng, s)
        valid = np.ones(M, bool)
        valid[:M - TAIL:7] = False
        near = _moved(H, rng, 0.3)
        bad = H.copy()
        bad[1, 2] = np.inf if p % 2 else np.nan
        sing = H.copy()
        sing[2] = 0.0
        models[M - TAIL:] = np.stack([H, near, _shifted(H, 3.0 * t / np.sqrt(2.0)), bad, sing, -3.0 * near])
        models[~valid] = np.nan
        ms.append(sc["matches"]), mo.append(models), kp.append(valid), gts.append(H)
    thr = THRESHOLD * np.array([THR_PAIRS[p % 3] for p in range(P)])
    if P > 1:
        thr[1] = 0.0
    mask = (rng.random((P, N)) < 0.67) if (P, N, M) == CASES[1] else None
    return dict(m=np.stack(ms), models=np.stack(mo), keep=np.stack(kp), mask=mask, thr=thr, gt=np.stack(gts))


# ------------------------------------------------------------------------------------------------ closed form
def det3(H):
    return (H[..., 0, 0] * (H[..., 1, 1] * H[..., 2, 2] - H[..., 1, 2] * H[..., 2, 1])
            - H[..., 0, 1] * (H[..., 1, 0] * H[..., 2, 2] - H[..., 1, 2] * H[..., 2, 0])
            + H[..., 0, 2] * (H[..., 1, 0] * H[..., 2, 1] - H[..., 1, 1] * H[..., 2, 0]))


def _grid(m, H, thr2, beta, terms=True):
    """one pair's matches m [n,4] under models H [k,3,3] (finite, det != 0) -> dict of arrays, nothing gated by `live` except w:
    a, live, sig, w, yw, zw [k,n]; with `terms` tH [k,n,3,3] = d d2 / d H and tx [k,n,4] = d d2 / d match of every term.  Evaluated in
    numpy.longdouble: e = x2 - y_xy / y_w cancels from hundreds of pixels to a fraction of one, so in f64 the reference itself would
    carry as much error as the one-ulp change of the inputs that it is used to measure; the sums are rounded to f64 by the callers"""
    LD = np.longdouble
    m, H, thr2, beta, E3 = np.asarray(m, LD), np.asarray(H, LD), LD(thr2), LD(beta), _EPS3.astype(LD)
    with np.errstate(all="ignore"):
        sgn = np.where(det3(H) < 0, LD(-1), LD(1))
        h = H * sgn[:, None, None]
        A = LD(0.5) * np.einsum("jab,icd,kac,kbd->kij", E3, E3, H, H)
        one = np.ones((len(m), 1), LD)
        X1, X2 = np.concatenate([m[:, :2], one], 1), np.concatenate([m[:, 2:], one], 1)
        y, z = np.einsum("kij,nj->kni", h, X1), np.einsum("kij,nj->kni", A, X2)
        ry, rz = LD(1) / y[..., 2], LD(1) / z[..., 2]
        ty, tz = y[..., :2] * ry[..., None], z[..., :2] * rz[..., None]
        e, f = m[None, :, 2:] - ty, m[None, :, :2] - tz
        d2 = (e * e).sum(-1) + (f * f).sum(-1)
        a = beta * (LD(1) - d2 / thr2)
        live = (y[..., 2] > 0) & (z[..., 2] > 0) & np.isfinite(d2) & (a >= CUTOFF)
        sig = LD(1) / (LD(1) + np.exp(-np.where(np.isfinite(a), np.maximum(a, LD(-700)), LD(-700))))      # the weight WITHOUT the cutoff
        out = dict(a=a, live=live, sig=sig, w=np.where(live, sig, 0.0), yw=y[..., 2], zw=z[..., 2])
        if not terms:
            return out
        dy = 2 * ry[..., None] * np.concatenate([-e, (e * ty).sum(-1, keepdims=True)], -1)                # d d2 / d y [k,n,3]
        dz = 2 * rz[..., None] * np.concatenate([-f, (f * tz).sum(-1, keepdims=True)], -1)
        gA = dz[..., :, None] * X2[None, :, None, :]                                                      # d d2 / d A [k,n,3,3]
        tH = sgn[:, None, None, None] * dy[..., :, None] * X1[None, :, None, :] + np.einsum("knij,kijac->knac", gA, np.einsum("jab,icd,kbd->kijac", E3, E3, H))
        tx = np.concatenate([2 * f + np.einsum("kij,kni->knj", h[:, :, :2], dy), 2 * e + np.einsum("kij,kni->knj", A[:, :, :2], dz)], -1)
    return dict(out, tH=tH, tx=tx)


def usable_models(models):
    """[...,3,3] -> bool: finite, with a finite non-zero determinant (the score kernel's usable set)"""
    with np.errstate(all="ignore"):
        d = det3(models)
        return np.isfinite(models).all((-1, -2)) & np.isfinite(d) & (d != 0)


def _usable(models, keep, thr, P, M):
    keep = np.ones((P, M), bool) if keep is None else np.asarray(keep, bool)
    thr2 = np.broadcast_to(np.asarray(thr, np.float64) ** 2, (P,))
    with np.errstate(invalid="ignore"):
        return keep & usable_models(models) & (thr2 > 0)[:, None], thr2


def soft_score(m, mask, models, keep, thr, beta=BETA, grad_scores=None):
    """m [P,N,4], mask [P,N] bool | None, models [P,M,3,3], keep [P,M] bool | None, thr = distance (scalar or [P]) -> scores [P,M];
    with grad_scores [P,M] (entries of unusable slots are never read) -> (scores, grad_models [P,M,3,3], grad_matches [P,N,4])"""
    (P, N, _), M = m.shape, models.shape[1]
    mask = np.ones((P, N), bool) if mask is None else np.asarray(mask, bool)
    use, thr2 = _usable(models, keep, thr, P, M)
    scores, gm, gx = np.zeros((P, M)), np.zeros((P, M, 3, 3)), np.zeros((P, N, 4))
    for p in range(P):
        js, ns = np.flatnonzero(use[p]), np.flatnonzero(mask[p])
        if not len(js) or not len(ns):
            continue
        G_ = _grid(m[p, ns], models[p, js], thr2[p], beta, grad_scores is not None)
        scores[p, js] = G_["w"].sum(1)
        if grad_scores is None:
            continue
        g = grad_scores[p, js][:, None] * (-beta / thr2[p]) * G_["w"] * (1.0 - G_["w"])
        with np.errstate(invalid="ignore"):                                                       # (0 x inf behind the gate)
            gm[p, js] = np.where(G_["live"][..., None, None], g[..., None, None] * G_["tH"], 0.0).sum(1)
            gx[p, ns] = np.where(G_["live"][..., None], g[..., None] * G_["tx"], 0.0).sum(0)
    return scores if grad_scores is None else (scores, gm, gx)


def bands(m, mask, models, keep, thr, beta, grad_scores, width_a, width_w):
    """what the points whose `live` decision a deviation of width_a in a (at the cutoff) or of width_w in y_w or z_w (at 0) can turn
    move at most: (scores [P,M], grad_models rows [P,M], grad_matches rows [P,N]): the sum of the points' own terms, evaluated without
    the gate (the largest |entry| of the term for the gradients)"""
    (P, N, _), M = m.shape, models.shape[1]
    mask = np.ones((P, N), bool) if mask is None else np.asarray(mask, bool)
    use, thr2 = _usable(models, keep, thr, P, M)
    bs, bm, bx = np.zeros((P, M)), np.zeros((P, M)), np.zeros((P, N))
    for p in range(P):
        js, ns = np.flatnonzero(use[p]), np.flatnonzero(mask[p])
        if not len(js) or not len(ns):
            continue
        G_ = _grid(m[p, ns], models[p, js], thr2[p], beta)
        with np.errstate(all="ignore"):
            near = ((np.abs(G_["a"] - CUTOFF) <= width_a) & (G_["yw"] > -width_w) & (G_["zw"] > -width_w)) | \
                (np.abs(G_["yw"]) <= width_w) | (np.abs(G_["zw"]) <= width_w)
            g = np.abs(grad_scores[p, js][:, None] * (beta / thr2[p]) * G_["sig"] * (1.0 - G_["sig"]))
            tm = np.nan_to_num(g * np.abs(G_["tH"]).max((-1, -2)), nan=0.0, posinf=0.0)
            tx = np.nan_to_num(g * np.abs(G_["tx"]).max(-1), nan=0.0, posinf=0.0)
        bs[p, js] = np.where(near, G_["sig"], 0.0).sum(1)
        bm[p, js] = np.where(near, tm, 0.0).sum(1)
        bx[p, ns] = np.where(near, tx, 0.0).sum(0)
    return bs, bm, bx


def cutoff_widths(m, mk, models, ok, keep, thr, tk, beta):
    """the reference's own deviation of a (among the points within 20 of the cutoff) and of y_w, z_w between the originals and the
    inputs as the kernel receives them, times TOL_FACTOR: the widths `bands` takes"""
    (P, _, _), M = m.shape, models.shape[1]
    use, thr2 = _usable(models, keep, thr, P, M)
    t2k = np.broadcast_to(np.asarray(tk, np.float64) ** 2, (P,))
    wa = ww = 0.0
    for p in range(P):
        js = np.flatnonzero(use[p])
        if not len(js) or not t2k[p] > 0:
            continue
        A, B = _grid(m[p], models[p, js], thr2[p], beta, False), _grid(mk[p], ok[p, js], t2k[p], beta, False)
        with np.errstate(all="ignore"):
            da = np.abs(A["a"] - B["a"])[np.isfinite(A["a"]) & np.isfinite(B["a"]) & (np.abs(A["a"] - CUTOFF) < 20.0)]
        wa = max(wa, float(da.max()) if da.size else 0.0)
        ww = max(ww, float(np.abs(A["yw"] - B["yw"]).max()), float(np.abs(A["zw"] - B["zw"]).max()))
    return R.TOL_FACTOR * wa, R.TOL_FACTOR * ww


# ------------------------------------------------------------------------------------------------ f64 torch, for autograd
def _torch_det3(H):
    return (H[..., 0, 0] * (H[..., 1, 1] * H[..., 2, 2] - H[..., 1, 2] * H[..., 2, 1])
            - H[..., 0, 1] * (H[..., 1, 0] * H[..., 2, 2] - H[..., 1, 2] * H[..., 2, 0])
            + H[..., 0, 2] * (H[..., 1, 0] * H[..., 2, 1] - H[..., 1, 1] * H[..., 2, 0]))


def torch_usable(models):
    with torch.no_grad():
        d = _torch_det3(models)
        return torch.isfinite(models).all(-1).all(-1) & torch.isfinite(d) & (d != 0)


def torch_soft_score(m, mask, models, keep, thr, beta=BETA):
    """the definition as a plain f64 torch expression (no formula of a gradient; the adjugate as the cross products of the columns):
    tensors m [P,N,4], models [P,M,3,3]; mask, keep bool tensors or None; thr a float or a [P] array -> scores [P,M]"""
    (P, N, _), M = m.shape, models.shape[1]
    thr2 = torch.as_tensor(np.broadcast_to(np.asarray(thr, np.float64) ** 2, (P,)).copy())
    use = torch_usable(models) & (thr2 > 0)[:, None]
    if keep is not None:
        use = use & keep
    H = torch.where(use[:, :, None, None], models, torch.eye(3, dtype=models.dtype).expand_as(models))
    A = torch.stack([torch.linalg.cross(H[..., :, 1], H[..., :, 2]), torch.linalg.cross(H[..., :, 2], H[..., :, 0]),
                     torch.linalg.cross(H[..., :, 0], H[..., :, 1])], -2)
    h = H * torch.where(_torch_det3(H.detach()) < 0, -1.0, 1.0)[..., None, None]
    one = torch.ones_like(m[..., :1])
    y = torch.einsum("pmij,pnj->pmni", h, torch.cat([m[..., :2], one], -1))
    z = torch.einsum("pmij,pnj->pmni", A, torch.cat([m[..., 2:], one], -1))
    front = (y[..., 2] > 0) & (z[..., 2] > 0)
    yw, zw = torch.where(front, y[..., 2], torch.ones_like(y[..., 2])), torch.where(front, z[..., 2], torch.ones_like(z[..., 2]))
    e, f = m[:, None, :, 2:] - y[..., :2] / yw[..., None], m[:, None, :, :2] - z[..., :2] / zw[..., None]
    d2 = (e * e).sum(-1) + (f * f).sum(-1)
    t2 = torch.where(thr2 > 0, thr2, torch.ones_like(thr2))[:, None, None]
    a = beta * (1.0 - d2 / t2)
    live = front & torch.isfinite(d2) & (a >= CUTOFF) & use[:, :, None]
    w = torch.where(live, torch.sigmoid(torch.where(live, a, torch.zeros_like(a))), torch.zeros_like(a))
    if mask is not None:
        w = w * mask[:, None, :].to(w.dtype)
    return w.sum(-1)


# ------------------------------------------------------------------------------------------------ the expected loss
def corner_errors(models, gt, size, max_loss):
    """l [P,M] in f64 torch for usable models [P,M,3,3] against gt [P,3,3]; size = (h, w) of the first image"""
    hh, ww = float(size[0]), float(size[1])
    c = torch.tensor([[0.0, 0.0, 1.0], [ww, 0.0, 1.0], [ww, hh, 1.0], [0.0, hh, 1.0]], dtype=models.dtype)
    out = []
    for p in range(models.shape[0]):                       # pair by pair, model by model: nothing shared with loss.py's batched form
        row = []
        for H in models[p]:
            Hs = H if float(_torch_det3(H.detach())) > 0 else -H
            y, g = c @ Hs.T, c @ gt[p].T
            if bool((y[:, 2] <= 0).any()):
                row.append(H.sum() * 0.0 + max_loss)
                continue
            d = y[:, :2] / y[:, 2:] - g[:, :2] / g[:, 2:]
            row.append(torch.sqrt((d * d).sum(-1) + CORNER_EPS2).mean().clamp(max=max_loss))
        out.append(torch.stack(row) if row else models.new_zeros(0))
    return torch.stack(out)


def corner_errors_closed_form(models, gt, size, max_loss):
    """numpy: usable models [k,3,3] against gt [3,3] -> (l [k], d l / d H [k,3,3]), evaluated in numpy.longdouble and rounded once.
    d = (image under H) - (image under gt) cancels from hundreds of pixels to the error itself, and the gradient's direction d / |d|
    carries that loss: in f64 (`corner_errors` and autograd) this reference would carry as much error as the one-ulp change of the
    inputs that it is used to measure.  With y = s H X_c, t = y_xy / y_w, r = sqrt(|d|^2 + eps2):
    d l / d H = s / 4 sum_c (d_0, d_1, -(d . t)) / (r y_w) (x) X_c; 0 for a clamped model and for one that sends a corner to w <= 0"""
    LD = np.longdouble
    H, g = np.asarray(models, LD), np.asarray(gt, LD)
    hh, ww = LD(size[0]), LD(size[1])
    X = np.array([[0, 0, 1], [ww, 0, 1], [ww, hh, 1], [0, hh, 1]], LD)
    sgn = np.where(det3(H) < 0, LD(-1), LD(1))
    y, gy = np.einsum("kij,cj->kci", H * sgn[:, None, None], X), X @ g.T
    front = (y[..., 2] > 0).all(1)
    yw = np.where(y[..., 2] > 0, y[..., 2], LD(1))
    t = y[..., :2] / yw[..., None]
    d = t - (gy[:, :2] / gy[:, 2:])[None]
    r = np.sqrt((d * d).sum(-1) + LD(CORNER_EPS2))
    ell = r.mean(1)
    u = np.concatenate([d, -(d * t).sum(-1, keepdims=True)], -1) / (r * yw)[..., None]
    grad = sgn[:, None, None] * np.einsum("kci,cj->kij", u, X) / LD(4)
    flat = ~front | (ell >= max_loss)
    return (np.where(flat, LD(max_loss), ell).astype(np.float64), np.where(flat[:, None, None], LD(0), grad).astype(np.float64))


class _CornerErrors(torch.autograd.Function):
    """corner_errors_closed_form as a node of the f64 torch graph of `expected_loss`"""

    @staticmethod
    def forward(ctx, models, gt, size, max_loss):
        ell, grad = corner_errors_closed_form(models.detach().numpy(), gt.detach().numpy(), size, max_loss)
        ctx.save_for_backward(torch.from_numpy(grad))
        return torch.from_numpy(ell)

    @staticmethod
    def backward(ctx, g):
        return g[:, None, None] * ctx.saved_tensors[0], None, None, None


def expected_loss(models, scores, n_scored, gt, keep, alpha, max_loss, size=SIZE):
    """f64 torch: models [P,M,3,3], scores [P,M], n_scored [P] (or an int), gt [P,3,3], keep [P,M] bool | None ->
    (loss, per_pair [P], probs [P,M])"""
    use = torch_usable(models)
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
        ell = _CornerErrors.apply(models[p, js], gt[p], size, max_loss)
        per_pair.append((q * ell).sum()), probs.append(pr.index_put((js,), q))
    per_pair = torch.stack(per_pair)
    return per_pair.mean(), per_pair, torch.stack(probs)
