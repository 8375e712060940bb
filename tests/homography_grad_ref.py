"""Two independent f64 references of the gradient of the weighted normalised DLT (csrc/homography.hip: dr_refit_homography_bwd,
ops.weighted_homography), the conditioning number the tolerance carries, and the inputs the host and GPU tests share.

The fit (tests/homography_ref.dlt; csrc/homography.hip (4)): rows (X1_n, X2_n) in pixels, weights w_n >= 0.  Per image c = mean X_n,
q_n = X_n - c, D = sum |q_n|, s = sqrt(2) R / D (Hartley's transform of the R selected rows, UNWEIGHTED), T = [[s, 0, -s cx],
[0, s, -s cy], [0, 0, 1]]; (x, y) = s q1_n, (u, v) = s q2_n, X = (x, y, 1), a = (0, -X, v X), b = (X, 0, -u X),
G = sum w (a a^T + b b^T), h = the eigenvector of G's smallest eigenvalue lambda_0, H0 = T2^-1 mat(h) T1, H = sigma H0 / |H0|_F,
sigma = sign det H0.  The functional is L = <gH, H> for a given gH [3,3]; wanted are dL/dX [n,4] and dL/dw [n].

  (a) autograd      torch f64 autograd on the CPU through that definition and torch.linalg.eigh.
  (b) closed_form   numpy.longdouble, no eigenvector autograd: a cyclic Jacobi in longdouble gives every eigenpair (lambda_i, v_i);
                    g0 = (sigma / |H0|) (gH - H <H, gH>), g_h = T2^-T g0 T1^T, the direct gradients of (c, s) of each image from
                    the derivative matrices of T1 and T2^-1; z = sum_{i != 0} v_i (v_i . g_h) / (lambda_i - lambda_0), so that
                    dL = -z^T dG h; per row f_n = -[(a . z)(a . h) + (b . z)(b . h)] = dL/dw_n, gx_n = w_n df_n/d(x, y, u, v) through
                    da, db; per image g_c = -s sum gx_n + direct, g_s = sum (gx_n . x_n) / s + direct, g_D = -g_s s / D,
                    g_c -= g_D sum q_n / |q_n|, and dL/dX_n = s gx_n + g_D q_n / |q_n| + g_c / R.

kappa = (lambda_8 - lambda_0) / (lambda_1 - lambda_0) of the normalised Gram matrix: the amplification of a perturbation of G into h.

Tolerance of the GPU tests, per pair and per output (the [n,4] matches gradient, the [n] weight gradient):
    |g - g_ref|_inf <= c eps(dtype) kappa_eff mag,
mag = |g_ref|_inf for the matches gradient.  The weight gradient is a cancelling sum: on a near-exact inlier a . h and b . h are
differences of O(1) products that leave the residual, and both references lose exactly that.  Its mag is therefore counted, not
fitted: the largest over the rows of (|a| . |z|)(|a| . |h|) + (|b| . |z|)(|b| . |h|), the sum of the absolute values of the products
that are added (weight_grad_magnitude, from reference (b)); it is never below |g_ref|_inf.  kappa_eff = kappa in f64 and 1 in f32
(where c eps64 kappa <= eps32 is asserted on the inputs: both sides see the same rounded inputs and the kernel works in f64).
c = 10 x the largest distance between (a) and (b) in those units over the f64 inputs of the GPU tests, and at least 10
(tolerance_constant below; printed by the host test, recorded in docs/LOG.md): a property of the two references, never fitted to the
kernel's output; the factor 10 is for the kernel's different summation order.  Pairs with kappa > KAPPA_MAX are compared for
finiteness only; they may be at most one per cent of a case -- with at most three pairs per case: none.  KAPPA_MAX comes from the
inputs' own distribution: over the GPU tests' inputs kappa lies between 9 and 3.5e3 (the host test prints the range; the largest values
belong to the minimal fits N = 4, 5, where lambda_0 = 0 and lambda_1 is set by how close the rows are to a degenerate
configuration), and KAPPA_MAX = 1e5 leaves a factor of thirty above that while c eps64 KAPPA_MAX stays below eps32."""
import functools
import math

import numpy as np
import torch

from tests import homography_ref as HR

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
KAPPA_MAX = 1e5
PAIR_N = (4, 5, 255, 256, 257, 1000)
PAIR_P = (1, 3)
INLIER_SHARE = 0.7
PAIR_CASES = [(N, P, weighted, masked) for N in PAIR_N for P in PAIR_P for weighted in (False, True) for masked in (False, True)]


# ------------------------------------------------------------------------------------------------------------------ reference (a)
def _norms(q):
    """|q_n| with the zero subgradient at q_n = 0"""
    d2 = (q * q).sum(-1)
    pos = d2 > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))


def torch_fit(x, w=None, want_eig=False):
    """reference (a)'s forward as a differentiable torch function: x [n,4], w [n] | None (f64) -> H [3,3], unit norm, det > 0"""
    n = x.shape[0]
    w = torch.ones(n, dtype=x.dtype) if w is None else w
    one, zero = torch.ones(n, 1, dtype=x.dtype), torch.zeros(n, 3, dtype=x.dtype)
    parts = []
    for img in (x[:, :2], x[:, 2:]):
        c = img.mean(0)
        q = img - c
        s = math.sqrt(2.0) * n / _norms(q).sum()
        parts.append((c, s, q * s))
    (c1, s1, p1), (c2, s2, p2) = parts
    X = torch.cat([p1, one], 1)
    A = torch.cat([torch.cat([zero, -X, p2[:, 1:2] * X], 1), torch.cat([X, zero, -p2[:, 0:1] * X], 1)], 0)
    G = A.T @ (torch.cat([w, w])[:, None] * A)
    lam, V = torch.linalg.eigh(G)
    Hn = V[:, 0].reshape(3, 3)
    o, z = torch.ones((), dtype=x.dtype), torch.zeros((), dtype=x.dtype)
    T1 = torch.stack([torch.stack([s1, z, -s1 * c1[0]]), torch.stack([z, s1, -s1 * c1[1]]), torch.stack([z, z, o])])
    T2i = torch.stack([torch.stack([1 / s2, z, c2[0]]), torch.stack([z, 1 / s2, c2[1]]), torch.stack([z, z, o])])
    H0 = T2i @ Hn @ T1
    H = H0 / torch.linalg.norm(H0)
    H = H * torch.sign(torch.linalg.det(H)).detach()
    return (H, lam.detach().numpy()) if want_eig else H


def autograd(x, w, gH):
    """(a): x [n,4], w [n] | None, gH [3,3] (numpy f64) -> (gx [n,4], gw [n])"""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    wt = torch.tensor(np.ones(len(x)) if w is None else np.asarray(w, np.float64), requires_grad=True)
    loss = (torch_fit(xt, wt) * torch.tensor(np.asarray(gH, np.float64))).sum()
    gx, gw = torch.autograd.grad(loss, (xt, wt))
    return gx.numpy(), gw.numpy()


def kappa(x, w=None):
    """(lambda_8 - lambda_0) / (lambda_1 - lambda_0) of one pair's normalised Gram matrix; inf for a degenerate one"""
    with torch.no_grad():
        _, lam = torch_fit(torch.tensor(np.asarray(x, np.float64)), None if w is None else torch.tensor(np.asarray(w, np.float64)),
                           want_eig=True)
    gap = lam[1] - lam[0]
    return float((lam[8] - lam[0]) / gap) if np.isfinite(lam).all() and gap > 1e-14 * lam[8] else float("inf")


# ------------------------------------------------------------------------------------------------------------------ reference (b)
def jacobi_eigh(G):
    """cyclic Jacobi of a symmetric matrix in longdouble -> (eigenvalues ascending, eigenvectors as columns)"""
    A = np.array(G, dtype=LD)
    n = len(A)
    V = np.eye(n, dtype=LD)
    for _ in range(60):
        off = np.sqrt(((A - np.diag(np.diag(A))) ** 2).sum())
        if off <= LD(1e-22) * np.sqrt((np.diag(A) ** 2).sum()):
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                if A[p, q] == 0:
                    continue
                with np.errstate(over="ignore"):      # (a tiny A[p, q]: theta = inf, t = 0)
                    theta = (A[q, q] - A[p, p]) / (2 * A[p, q])
                t = (1 if theta >= 0 else -1) / (abs(theta) + np.hypot(theta, LD(1)))
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                for M in (A, V):
                    mp, mq = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * mp - s * mq, s * mp + c * mq
                rp, rq = A[p].copy(), A[q].copy()
                A[p], A[q] = c * rp - s * rq, s * rp + c * rq
    order = np.argsort(np.diag(A))
    return np.diag(A)[order], V[:, order]


def _unit(i, j):
    E = np.zeros((3, 3), dtype=LD)
    E[i, j] = 1
    return E


def closed_form(x, w, gH, want_mag=False):
    """(b) for one pair: x [n,4], w [n] | None, gH [3,3] -> (gx [n,4], gw [n]) as f64.  want_mag: -> (gx, gw, mag [n]), mag = the
    summed absolute values of the weight gradient's terms per row (module docstring)."""
    x = np.asarray(x, np.float64).astype(LD)
    n = len(x)
    w = (np.ones(n) if w is None else np.asarray(w, np.float64)).astype(LD)
    gH = np.asarray(gH, np.float64).astype(LD)
    img = []
    for k in (0, 2):
        c = x[:, k:k + 2].sum(0) / n
        q = x[:, k:k + 2] - c
        r = np.sqrt((q * q).sum(1))
        D = r.sum()
        s = np.sqrt(LD(2)) * n / D
        with np.errstate(all="ignore"):
            dirs = np.where(r[:, None] > 0, q / np.where(r > 0, r, 1)[:, None], 0)
        img.append(dict(c=c, q=q, D=D, s=s, p=q * s, dirs=dirs))
    i1, i2 = img
    xx, yy, uu, vv = i1["p"][:, 0], i1["p"][:, 1], i2["p"][:, 0], i2["p"][:, 1]
    one, zero = np.ones(n, dtype=LD), np.zeros(n, dtype=LD)
    X = np.stack([xx, yy, one], 1)
    Z3 = np.zeros((n, 3), dtype=LD)
    a = np.concatenate([Z3, -X, vv[:, None] * X], 1)
    b = np.concatenate([X, Z3, -uu[:, None] * X], 1)
    G = a.T @ (w[:, None] * a) + b.T @ (w[:, None] * b)
    lam, V = jacobi_eigh(G)
    h = V[:, 0]
    T1 = np.array([[i1["s"], 0, -i1["s"] * i1["c"][0]], [0, i1["s"], -i1["s"] * i1["c"][1]], [0, 0, 1]], dtype=LD)
    T2i = np.array([[1 / i2["s"], 0, i2["c"][0]], [0, 1 / i2["s"], i2["c"][1]], [0, 0, 1]], dtype=LD)
    Hn = h.reshape(3, 3)
    H0 = T2i @ Hn @ T1
    nrm = np.sqrt((H0 * H0).sum())
    det = H0[0, 0] * (H0[1, 1] * H0[2, 2] - H0[1, 2] * H0[2, 1]) - H0[0, 1] * (H0[1, 0] * H0[2, 2] - H0[1, 2] * H0[2, 0]) \
        + H0[0, 2] * (H0[1, 0] * H0[2, 1] - H0[1, 1] * H0[2, 0])
    sigma = 1 if det > 0 else -1
    H = sigma * H0 / nrm
    g0 = (sigma / nrm) * (gH - H * (H * gH).sum())
    gh = (T2i.T @ g0 @ T1.T).reshape(9)
    s1, s2 = i1["s"], i2["s"]
    dT1 = [-s1 * _unit(0, 2), -s1 * _unit(1, 2), _unit(0, 0) + _unit(1, 1) - i1["c"][0] * _unit(0, 2) - i1["c"][1] * _unit(1, 2)]
    dT2i = [_unit(0, 2), _unit(1, 2), -(_unit(0, 0) + _unit(1, 1)) / (s2 * s2)]
    direct = [np.array([(g0 * (T2i @ Hn @ d)).sum() for d in dT1], dtype=LD), np.array([(g0 * (d @ Hn @ T1)).sum() for d in dT2i], dtype=LD)]
    z = np.zeros(9, dtype=LD)
    for i in range(1, 9):
        z += V[:, i] * (V[:, i] @ gh) / (lam[i] - lam[0])
    ah, az, bh, bz = a @ h, a @ z, b @ h, b @ z
    aa, ab = np.abs(a), np.abs(b)
    mag = (aa @ np.abs(z)) * (aa @ np.abs(h)) + (ab @ np.abs(z)) * (ab @ np.abs(h))
    gw = -(az * ah + bz * bh)
    # da / d(x, y, u, v) and db / d(x, y, u, v), [4][n,9]
    col = lambda k, v: np.concatenate([np.zeros((n, k), dtype=LD), v[:, None], np.zeros((n, 8 - k), dtype=LD)], 1)
    da = [col(3, -one) + col(6, vv), col(4, -one) + col(7, vv), np.zeros((n, 9), dtype=LD), col(6, xx) + col(7, yy) + col(8, one)]
    db = [col(0, one) + col(6, -uu), col(1, one) + col(7, -uu), col(6, -xx) + col(7, -yy) + col(8, -one), np.zeros((n, 9), dtype=LD)]
    gp = np.stack([-w * ((da[k] @ z) * ah + az * (da[k] @ h) + (db[k] @ z) * bh + bz * (db[k] @ h)) for k in range(4)], 1)
    out = np.zeros((n, 4), dtype=LD)
    for k, im in enumerate((i1, i2)):
        g = gp[:, 2 * k:2 * k + 2]
        s = im["s"]
        g_c = -s * g.sum(0) + direct[k][:2]
        g_s = (g * im["p"]).sum() / s + direct[k][2]
        g_D = -g_s * s / im["D"]
        g_c = g_c - g_D * im["dirs"].sum(0)
        out[:, 2 * k:2 * k + 2] = s * g + g_D * im["dirs"] + g_c / n
    res = (out.astype(np.float64), gw.astype(np.float64))
    return res + (mag.astype(np.float64),) if want_mag else res


def weight_grad_magnitude(x, w, gH):
    """max over the rows of one pair of the summed absolute values of the weight gradient's terms"""
    return float(closed_form(x, w, gH, want_mag=True)[2].max())


def distance_units(x, w, gH, other=None, a=None):
    """the distance between (a) and (b) -- or between (a) and `other` = (gx, gw) -- of one pair in units of eps64 kappa mag, the
    larger of the two outputs; a = (gx, gw) of reference (a) where the caller has them"""
    ax, aw = autograd(x, w, gH) if a is None else a
    bx, bw, mag = closed_form(x, w, gH, want_mag=True)
    if other is not None:
        bx, bw = other
    return max(np.abs(ax - bx).max() / np.abs(ax).max(), np.abs(aw - bw).max() / mag.max()) / (EPS64 * kappa(x, w))


# ---------------------------------------------------------------------------------------------------------------------- inputs
def _round(a, dtype):
    return np.asarray(a).astype(dtype).astype(np.float64)


def scene_matches(p, N, dtype=np.float64):
    """homography_ref.scene(300 + p, N, 0.7) in pixels, rounded to `dtype` (so that f32 kernels and the f64 references see the same
    numbers)"""
    return _round(HR.scene(300 + p, N, INLIER_SHARE)["matches"], dtype)


def pair_case(N, P, weighted, masked, dtype=np.float64):
    """the inputs of one dr_refit_homography_bwd case: x [P,N,4] = scene_matches(p, N), mask [P,N] (about half the rows, another
    half per pair) | None, w [P,N] in [0.25, 1.25) | None, gH [P,3,3] standard normal, its component along H left in; f64 arrays
    holding values exact in `dtype`"""
    g = torch.Generator().manual_seed(11 * N + 5 * P + (3 if weighted else 0) + (1 if masked else 0))
    x = np.stack([scene_matches(p, N, dtype) for p in range(P)])
    w = _round(0.25 + torch.rand(P, N, generator=g, dtype=torch.float64).numpy(), dtype) if weighted else None
    gH = _round(torch.randn(P, 3, 3, generator=g, dtype=torch.float64).numpy(), dtype)
    mask = (np.random.default_rng(N + 13 * P).uniform(size=(P, N)) < 0.5) if masked else None
    return dict(x=x, w=w, mask=mask, gH=gH)


def selected(case, p):
    """-> (rows mask [N] bool, x of the selected rows, w of them | None) of pair p"""
    N = case["x"].shape[1]
    sel = np.ones(N, bool) if case["mask"] is None else case["mask"][p]
    return sel, case["x"][p, sel], None if case["w"] is None else case["w"][p, sel]


def pair_reference(case):
    """(a) on the selected rows of every pair, scattered back: -> dict(gx [P,N,4], gw [P,N], kappa [P], mag_x [P], mag_w [P],
    rows [P]); zeros and kappa = inf for a pair with fewer than four rows"""
    P, N, _ = case["x"].shape
    out = dict(gx=np.zeros((P, N, 4)), gw=np.zeros((P, N)), kappa=np.full(P, np.inf), mag_x=np.zeros(P), mag_w=np.zeros(P),
               rows=np.zeros(P, int))
    for p in range(P):
        sel, xs, ws = selected(case, p)
        out["rows"][p] = sel.sum()
        if sel.sum() < 4:
            continue
        ax, aw = autograd(xs, ws, case["gH"][p])
        out["gx"][p, sel], out["gw"][p, sel], out["kappa"][p] = ax, aw, kappa(xs, ws)
        out["mag_x"][p], out["mag_w"][p] = np.abs(ax).max(), weight_grad_magnitude(xs, ws, case["gH"][p])
    return out


@functools.lru_cache(maxsize=None)
def cached_case(N, P, weighted, masked, dtype_name="float64"):
    """-> (pair_case, pair_reference of it), computed once and shared by the tests: do not modify"""
    cs = pair_case(N, P, weighted, masked, np.dtype(dtype_name))
    return cs, pair_reference(cs)


def exact_case(dtype=np.float64):
    """four exact correspondences of a homography with small integer entries on integer points (every product exact in f32):
    -> dict(x [1,4,4], w None, mask None, gH [1,3,3])"""
    x1 = np.array([[0.0, 0.0], [8.0, 1.0], [7.0, 9.0], [-1.0, 6.0]])
    Hm = np.array([[2.0, 0.0, 1.0], [0.0, 2.0, -3.0], [0.0, 0.0, 1.0]])
    y = np.concatenate([x1, np.ones((4, 1))], 1) @ Hm.T
    x = np.concatenate([x1, y[:, :2] / y[:, 2:]], 1)
    gH = _round(np.random.default_rng(5).standard_normal((1, 3, 3)), dtype)
    return dict(x=_round(x, dtype)[None], w=None, mask=None, gH=gH)


@functools.lru_cache(maxsize=None)
def input_units():
    """-> list of (case key, pair, kappa, (a)-(b) distance in units) over the f64 inputs of the GPU tests with at least four rows"""
    out = []
    for key in PAIR_CASES:
        cs, ref = cached_case(*key)
        for p in range(key[1]):
            if ref["rows"][p] < 4:
                continue
            sel, xs, ws = selected(cs, p)
            k = ref["kappa"][p]
            a = (ref["gx"][p, sel], ref["gw"][p, sel])
            out.append((key, p, k, distance_units(xs, ws, cs["gH"][p], a=a) if k <= KAPPA_MAX else float("nan")))
    return out


@functools.lru_cache(maxsize=None)
def tolerance_constant():
    """10 x the largest (a)-(b) distance over the GPU tests' f64 inputs with kappa <= KAPPA_MAX, and at least 10 (one unit is the
    least two correct f64 evaluations can differ by)"""
    return 10.0 * max([1.0] + [u for _, _, k, u in input_units() if k <= KAPPA_MAX])


def tolerances(ref, p, dtype_name):
    """-> (tolerance of the matches gradient, of the weight gradient) of pair p of a reference, or None for a pair with
    kappa > KAPPA_MAX (finiteness only)"""
    k = ref["kappa"][p]
    if not k <= KAPPA_MAX:
        return None
    unit = tolerance_constant() * (EPS64 * k if dtype_name == "float64" else EPS32)
    return unit * ref["mag_x"][p], unit * ref["mag_w"][p]
