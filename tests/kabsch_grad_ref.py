"""Two independent f64 references of the gradient of the weighted Kabsch fit (csrc/registration.hip: kabsch3_bwd, dr_kabsch_bwd,
dr_refit_rigid_bwd), the conditioning number the tolerance carries, and the inputs the host and GPU tests share.

The fit (tests/registration_ref.kabsch): rows (p_n, q_n), weights w_n >= 0, W = sum w, c0 = sum w p / W, c1 = sum w q / W,
H = sum w (p - c0)(q - c1)^T = U S V^T, R = V diag(1, 1, d) U^T with d = det(V U^T), t = c1 - R c0.  The functional is
L = sum gR o R + gt . t for given gR [3,3], gt [3]; wanted are dL/dp, dL/dq, dL/dw.

  (a) autograd      torch f64 autograd through torch.linalg.svd on the CPU, batched over samples.
  (b) closed_form   numpy.longdouble, no SVD derivative: on the rotation polished by registration_ref._polish_rotation, the condition
                    "A = R H is symmetric" is differentiated -- G = gR - gt c0^T, K = tr(A) I - A, Y = G R^T,
                    a = (Y21 - Y12, Y02 - Y20, Y10 - Y01), z = K^-1 a, gH = -R^T [z]x, g_c0 = -R^T gt, g_c1 = gt, and per row
                    g_p = w gH dq + (w / W) g_c0, g_q = w gH^T dp + (w / W) g_c1, g_w = dp^T gH dq + (dp . g_c0 + dq . g_c1) / W.

kappa = (s1 + s2) / (s2 + d s3), the condition number of K: it blows up for near-collinear samples and at the reflection tie
d = -1, s2 ~ s3.

Tolerance of the GPU tests, per sample (or pair) and per output (the [k,6] sample gradient, the [k] weight gradient):
    |g - g_ref|_inf <= c eps(dtype) kappa_eff mag,
mag = |g_ref|_inf for the sample gradient.  The weight gradient is a sum of three terms that cancel (its |g_ref|_inf is up to 1e3 times
smaller than its terms on these inputs, and both references lose exactly that), so its mag is counted, not fitted: the largest over
the rows of |dp|^T |gH| |dq| + (|dp| . |g_c0| + |dq| . |g_c1|) / W, the sum of the absolute values of what is added (weight_grad_magnitude,
from reference (b)).  kappa_eff = kappa in f64 and 1 in f32 (where c eps64 kappa <= eps32 is asserted on the inputs: both sides see the same rounded
inputs, and the kernels work in f64).  c = 10 x the largest distance between (a) and (b) in units of eps64 kappa |g_ref|_inf over
the inputs of the GPU tests (tolerance_constant below; printed by the host test, recorded in docs/LOG.md) -- a property of the
references, never fitted to a kernel's output.  Samples with kappa > KAPPA_MAX are left out of the comparison (finiteness only), at
most one per cent of a case."""
import functools

import numpy as np
import torch

from tests import registration_ref as R

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
KAPPA_MAX = 1e3
SAMPLE_BT = (1, 63, 64, 65, 130)
SAMPLE_K = (3, 4, 8)
PAIR_N = (3, 255, 256, 257, 1000)


# ------------------------------------------------------------------------------------------------------------------ references
def _torch_fit(x, w):
    """x [B,n,6], w [B,n] (torch f64) -> R [B,3,3], t [B,3], with autograd through the SVD"""
    W = w.sum(-1, keepdim=True)
    c = (w[..., None] * x).sum(-2) / W
    dp = x[..., :3] - c[:, None, :3]
    dq = x[..., 3:] - c[:, None, 3:]
    H = (w[..., None] * dp).transpose(-1, -2) @ dq
    U, S, Vh = torch.linalg.svd(H)
    V = Vh.transpose(-1, -2)
    d = torch.sign(torch.linalg.det(V @ U.transpose(-1, -2))).detach()
    D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], -1))
    Rm = V @ D @ U.transpose(-1, -2)
    t = c[:, 3:] - (Rm @ c[:, :3, None])[..., 0]
    return Rm, t


def torch_kabsch(x, w=None):
    """reference (a)'s forward as a differentiable torch function: x [B,n,6], w [B,n] | None -> models [B,4,4]"""
    w = torch.ones(x.shape[:-1], dtype=x.dtype) if w is None else w
    Rm, t = _torch_fit(x, w)
    top = torch.cat([Rm, t[..., None]], -1)
    last = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=x.dtype).expand(x.shape[0], 1, 4)
    return torch.cat([top, last], -2)


def autograd(x, w, gR, gt):
    """(a): x [B,n,6], w [B,n] | None, gR [B,3,3], gt [B,3] (numpy f64) -> (gx [B,n,6], gw [B,n])"""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    wt = torch.tensor(np.ones(np.shape(x)[:-1]) if w is None else np.asarray(w, np.float64), requires_grad=True)
    Rm, t = _torch_fit(xt, wt)
    loss = (Rm * torch.tensor(np.asarray(gR, np.float64))).sum() + (t * torch.tensor(np.asarray(gt, np.float64))).sum()
    gx, gw = torch.autograd.grad(loss, (xt, wt))
    return gx.numpy(), gw.numpy()


def _svd_parts(x, w):
    """-> (c0, c1, dp, dq, H, W) in longdouble, (U, S, V, d) of the f64 SVD"""
    x = np.asarray(x, np.float64).astype(LD)
    w = (np.ones(len(x)) if w is None else np.asarray(w, np.float64)).astype(LD)
    W = w.sum()
    c0 = (w[:, None] * x[:, :3]).sum(0) / W
    c1 = (w[:, None] * x[:, 3:]).sum(0) / W
    dp, dq = x[:, :3] - c0, x[:, 3:] - c1
    H = ((w[:, None] * dp)[:, :, None] * dq[:, None, :]).sum(0)
    U, S, Vt = np.linalg.svd(H.astype(np.float64))
    d = 1.0 if np.linalg.det(Vt.T @ U.T) > 0 else -1.0
    return c0, c1, dp, dq, H, W, w, U, S, Vt.T, d


def kappa(x, w=None):
    """(s1 + s2) / (s2 + d s3) of one sample x [n,6]; inf for a degenerate one"""
    *_, S, _, d = _svd_parts(x, w)
    den = S[1] + d * S[2]
    return float((S[0] + S[1]) / den) if den > 0 and S[1] > 1e-12 * S[0] else float("inf")


def closed_form(x, w, gR, gt, flip_gH=False, drop_gw_centroid=False, want_mag=False):
    """(b) for one sample: x [n,6], w [n] | None, gR [3,3], gt [3] -> (gx [n,6], gw [n]) as f64.  The two switches produce the
    deliberately WRONG forms the host test uses to show that the tolerance separates them.  want_mag: -> the magnitude of the weight
    gradient's terms per row instead (see the module docstring)."""
    c0, c1, dp, dq, H, W, w, U, S, V, d = _svd_parts(x, w)
    Rm = R._polish_rotation(V @ np.diag([1.0, 1.0, d]) @ U.T, H)
    gR, gt = np.asarray(gR, np.float64).astype(LD), np.asarray(gt, np.float64).astype(LD)
    G = gR - np.outer(gt, c0)
    g_c1, g_c0 = gt, -Rm.T @ gt
    A = Rm @ H
    A = LD(0.5) * (A + A.T)
    K = np.trace(A) * np.eye(3, dtype=LD) - A
    Y = G @ Rm.T
    a = np.array([Y[2, 1] - Y[1, 2], Y[0, 2] - Y[2, 0], Y[1, 0] - Y[0, 1]], dtype=LD)
    # K^-1 a by the adjugate, in longdouble (numpy.linalg has no extended-precision solve)
    cof = np.array([[K[1, 1] * K[2, 2] - K[1, 2] * K[2, 1], K[0, 2] * K[2, 1] - K[0, 1] * K[2, 2], K[0, 1] * K[1, 2] - K[0, 2] * K[1, 1]],
                    [K[1, 2] * K[2, 0] - K[1, 0] * K[2, 2], K[0, 0] * K[2, 2] - K[0, 2] * K[2, 0], K[0, 2] * K[1, 0] - K[0, 0] * K[1, 2]],
                    [K[1, 0] * K[2, 1] - K[1, 1] * K[2, 0], K[0, 1] * K[2, 0] - K[0, 0] * K[2, 1], K[0, 0] * K[1, 1] - K[0, 1] * K[1, 0]]],
                   dtype=LD)
    det = K[0, 0] * cof[0, 0] + K[0, 1] * cof[1, 0] + K[0, 2] * cof[2, 0]
    z = cof @ a / det
    gH = -Rm.T @ R._cross_matrix(z)
    if want_mag:
        return (np.einsum("ni,ij,nj->n", np.abs(dp), np.abs(gH), np.abs(dq))
                + (np.abs(dp) @ np.abs(g_c0) + np.abs(dq) @ np.abs(g_c1)) / W).astype(np.float64)
    if flip_gH:
        gH = -gH
    gp = w[:, None] * (dq @ gH.T) + (w / W)[:, None] * g_c0
    gq = w[:, None] * (dp @ gH) + (w / W)[:, None] * g_c1
    gw = np.einsum("ni,ij,nj->n", dp, gH, dq)
    if not drop_gw_centroid:
        gw = gw + (dp @ g_c0 + dq @ g_c1) / W
    return np.concatenate([gp, gq], 1).astype(np.float64), gw.astype(np.float64)


def weight_grad_magnitude(x, w, gR, gt):
    """max over the rows of one sample of the summed absolute values of the weight gradient's terms"""
    return float(closed_form(x, w, gR, gt, want_mag=True).max())


def distance_units(x, w, gR, gt, other=None):
    """the distance between (a) and (b) -- or between (a) and `other` = (gx, gw) -- of one sample, in units of
    eps64 kappa mag, the larger of the two outputs"""
    ax, aw = autograd(x[None], None if w is None else w[None], gR[None], gt[None])
    bx, bw = closed_form(x, w, gR, gt) if other is None else other
    k = kappa(x, w)
    return max(np.abs(ax[0] - bx).max() / np.abs(ax[0]).max(),
               np.abs(aw[0] - bw).max() / weight_grad_magnitude(x, w, gR, gt)) / (EPS64 * k)


# ---------------------------------------------------------------------------------------------------------------------- inputs
def scene_matches(p, N, dtype=np.float64):
    """registration_ref.scene(100 + p, N, 0.6), rounded to `dtype` (so that f32 kernels and the f64 references see the same numbers)"""
    return R.scene(100 + p, N, 0.6)["matches"].astype(dtype).astype(np.float64)


def sample_case(Bt, k, weighted, dtype=np.float64):
    """the inputs of one dr_kabsch_bwd case: samples [Bt,k,6] drawn by seeded randperm index sets from scene_matches(p, 200) with
    p = sample number mod 4, weights [Bt,k] in [0.25, 1.25) | None, upstream gradients gR [Bt,3,3], gt [Bt,3]; all f64 arrays holding
    values exact in `dtype`"""
    g = torch.Generator().manual_seed(1000 * k + Bt + (500 if weighted else 0))
    N = 200
    scenes = [scene_matches(p, N, dtype) for p in range(4)]
    idx = torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(Bt)]).numpy()
    x = np.stack([scenes[s % 4][idx[s]] for s in range(Bt)])
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64).numpy().astype(dtype).astype(np.float64)
    w = (0.25 + torch.rand(Bt, k, generator=g, dtype=torch.float64).numpy()).astype(dtype).astype(np.float64) if weighted else None
    return dict(x=x, w=w, gR=rnd(Bt, 3, 3), gt=rnd(Bt, 3), idx=idx)


def pair_mask(kind, P, N, seed):
    """the masks of the dr_refit_rigid_bwd cases, a different one per pair: None | "ragged" (60 % of the rows) | "stride" (rows with
    n % 256 == 5 only, thinned differently per pair) | "two" (two rows: no fit)"""
    if kind is None:
        return None
    rng = np.random.default_rng(seed)
    m = np.zeros((P, N), dtype=bool)
    for p in range(P):
        if kind == "ragged":
            m[p] = rng.uniform(size=N) < 0.6
        elif kind == "stride":
            rows = np.arange(5, N, 256)
            m[p, (rows, rows[1:], rows[:-1])[p % 3]] = True
        elif kind == "two":
            m[p, rng.permutation(N)[:2]] = True
    return m


def pair_case(N, mask_kind, weighted, dtype=np.float64, P=3):
    """the inputs of one dr_refit_rigid_bwd case: matches [P,N,6] = scene_matches(p, N), mask [P,N] | None, weights [P,N] in
    [0.25, 1.25) | None, gR [P,3,3], gt [P,3]"""
    g = torch.Generator().manual_seed(7 * N + (3 if weighted else 0) + len(str(mask_kind)))
    x = np.stack([scene_matches(p, N, dtype) for p in range(P)])
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64).numpy().astype(dtype).astype(np.float64)
    w = (0.25 + torch.rand(P, N, generator=g, dtype=torch.float64).numpy()).astype(dtype).astype(np.float64) if weighted else None
    return dict(x=x, w=w, mask=pair_mask(mask_kind, P, N, N + 11), gR=rnd(P, 3, 3), gt=rnd(P, 3))


def pair_reference(case):
    """(a) on the selected rows of every pair, scattered back: -> (gx [P,N,6], gw [P,N], kappa [P], weight_grad_magnitude [P]);
    zeros and kappa = inf for a pair with fewer than three rows"""
    x, w, mask = case["x"], case["w"], case["mask"]
    P, N, _ = x.shape
    gx, gw, kap, mag = np.zeros((P, N, 6)), np.zeros((P, N)), np.full(P, np.inf), np.zeros(P)
    for p in range(P):
        sel = np.ones(N, bool) if mask is None else mask[p]
        if sel.sum() < 3:
            continue
        wp = None if w is None else w[p, sel]
        ax, aw = autograd(x[p, sel][None], None if wp is None else wp[None], case["gR"][p][None], case["gt"][p][None])
        gx[p, sel], gw[p, sel], kap[p] = ax[0], aw[0], kappa(x[p, sel], wp)
        mag[p] = weight_grad_magnitude(x[p, sel], wp, case["gR"][p], case["gt"][p])
    return gx, gw, kap, mag


PAIR_CASES = [(N, None, wt) for N in PAIR_N for wt in (False, True)] + [(1000, "ragged", True), (1000, "stride", True),
                                                                         (257, "ragged", False), (1000, "stride", False)]


@functools.lru_cache(maxsize=None)
def tolerance_constant():
    """-> dict(k -> c for the sample cases, "pair" -> c for the pair cases), each 10 x the largest (a)-(b) distance over the GPU
    tests' f64 inputs with kappa <= KAPPA_MAX, and at least 10 (one unit is the least two correct f64 evaluations can differ by)"""
    out = {}
    for k in SAMPLE_K:
        worst = 1.0
        for Bt in SAMPLE_BT:
            for weighted in (False, True):
                cs = sample_case(Bt, k, weighted)
                for s in range(Bt):
                    w = None if cs["w"] is None else cs["w"][s]
                    if kappa(cs["x"][s], w) <= KAPPA_MAX:
                        worst = max(worst, distance_units(cs["x"][s], w, cs["gR"][s], cs["gt"][s]))
        out[k] = 10.0 * worst
    worst = 1.0
    for N, kind, weighted in PAIR_CASES:
        cs = pair_case(N, kind, weighted)
        for p in range(cs["x"].shape[0]):
            sel = np.ones(N, bool) if cs["mask"] is None else cs["mask"][p]
            w = None if cs["w"] is None else cs["w"][p, sel]
            if sel.sum() >= 3 and kappa(cs["x"][p, sel], w) <= KAPPA_MAX:
                worst = max(worst, distance_units(cs["x"][p, sel], w, cs["gR"][p], cs["gt"][p]))
    out["pair"] = 10.0 * worst
    return out


def reflection_sample():
    """a constructed sample of four rows whose best orthogonal fit is a reflection (d = -1) with well separated s2 > s3:
    q = mirror image of p in the z = 0 plane, rotated and shifted -> x [4,6]"""
    rng = np.random.default_rng(17)
    p = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.2], [0.2, 0.9, -0.1], [0.3, 0.2, 0.5]])
    Rr = R.random_rotation(rng)
    q = (p * np.array([1.0, 1.0, -1.0])) @ Rr.T + np.array([0.3, -0.2, 0.7])
    return np.concatenate([p, q], 1)
