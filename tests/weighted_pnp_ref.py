"""f64 reference of the differentiable weighted PnP fit (ops.weighted_pnp, ops.pnp_dlt; dr_refit_pnp_weighted, dr_refit_pnp_bwd,
dr_pnp_dlt), written from the formulas with numpy and CPU torch autograd and not from the kernels.

  minimiser   weighted Levenberg-Marquardt with the kernels' acceptance rule (`lm`, what a forward of `iters` passes is compared with
              from the same start), then Newton steps with the full Hessian onto the stationary point (`minimiser`).
  gradient    the implicit function theorem at that point (`ift`): the cost c(theta) = 1/2 sum w |r|^2 in the left-multiplied chart
              theta = (w, d), x_c' = exp([w]x) x_c + d, is plain torch; its gradient g and Hessian H (torch.autograd.functional.hessian)
              come from autograd, lambda = H^-1 g_theta, and the gradients to rows and weights are -d (lambda . g) / d (rows, weights),
              again by autograd.  No formula of the derivative is written down here.  gauss_newton=True puts J^T J in H's place: what a
              backward without the residual terms would return.
  DLT         `dlt`: the null vector of the weighted equations by numpy.linalg.svd, the nearest rotation by another.

Tolerances (pnp_ref's rule): `deviation` of a quantity = the reference on inputs as the kernel receives them (rounded to float32; for
float64 moved by one ulp) against the reference on the f64 originals; a test allows TOL_FACTOR = 8 times the largest figure of its case.
The forward follows tests/test_gpu_pnp.py's refit test: the compared result is `lm` at the kernel's number of passes, and its figures are
that run on the kernel's inputs with its pose rounded the same way, and that run with twice the passes (its own convergence error: the
loop takes a step only on a strictly lower cost, and where it stalls depends on roundings) -- `forward_figures`.  The backward's figures are
the largest over SEEDS one-ulp moves (one rounding for float32) -- `backward_figures`."""
import math

import numpy as np
import torch

from tests import pnp_ref as R

TOL_FACTOR = R.TOL_FACTOR
NOISE = 0.02               # image noise of the gradient scenes: residuals at which the second-order terms of H matter (test asserts it)
COND_MAX = 1e8             # a pair is compared only if cond(H) is below this; at most EXCLUDED_MAX of a case may be left out
EXCLUDED_MAX = 0.10
DLT_GAP = 1e-10            # the header's rule: lambda_1 - lambda_0 <= DLT_GAP lambda_max -> no pose
SHAPES = [(1, 3), (3, 4), (1, 6), (3, 7), (1, 257), (3, 300)]      # (P, N)
ITERS = 20


def scene(seed, N, noise=NOISE):
    """pnp_ref.scene without outliers at image noise `noise`, weights in [0.2, 1], a start 2 degrees / 1 % of the depth off the truth"""
    sc = R.scene(seed, N, 1.0, noise)
    rng = np.random.default_rng(seed + 977)
    sc["weights"] = rng.uniform(0.2, 1.0, N)
    sc["start"] = R.perturbed(sc["pose"], rng, 2.0, 0.01)
    return sc


def case(P, N, seed=3, noise=NOISE, ragged=False):
    """-> dict(m [P,N,5], w [P,N], start [P,4,4], gt [P,4,4], mask [P,N] bool): `ragged` drops a different number of rows per pair"""
    scs = [scene(seed + 13 * p + N, N, noise) for p in range(P)]
    mask = np.ones((P, N), bool)
    if ragged:
        for p in range(P):
            drop = np.random.default_rng(seed + p).permutation(N)[:min(N - 6, 1 + 2 * p + N // 5)] if N > 6 else []
            mask[p, drop] = False
    return dict(m=np.stack([s["matches"] for s in scs]), w=np.stack([s["weights"] for s in scs]), start=np.stack([s["start"] for s in scs]),
                gt=np.stack([s["pose"] for s in scs]), mask=mask)


# ------------------------------------------------------------------------------------------------ the fit
def _rows(m, sel, T):
    with np.errstate(all="ignore"):
        xc = m[:, :3] @ T[:3, :3].T + T[:3, 3]
        r = np.stack([xc[:, 0] / xc[:, 2] - m[:, 3], xc[:, 1] / xc[:, 2] - m[:, 4]], 1)
    return xc, r, sel & (xc[:, 2] > 0) & np.isfinite(r).all(1)


def _jac(xc):
    iz = 1.0 / xc[:, 2]
    x, y, z0 = xc[:, 0] * iz, xc[:, 1] * iz, np.zeros(len(xc))
    return (np.stack([-x * y, 1 + x * x, -y, iz, z0, -x * iz], 1), np.stack([-1 - y * y, x * y, x, z0, iz, -y * iz], 1))


def lm(m, w, mask, init, iters=ITERS):
    """pnp_ref.lm_refit with a weight on every row's terms -> (pose, valid)"""
    T = np.array(init, np.float64)
    sel = np.ones(len(m), bool) if mask is None else np.asarray(mask, bool)
    w = np.ones(len(m)) if w is None else np.asarray(w, np.float64)
    if not np.isfinite(T[:3]).all() or _rows(m, sel, T)[2].sum() < 3:
        return np.eye(4), False
    lam = 1e-3
    for _ in range(iters):
        xc, r, rows = _rows(m, sel, T)
        Ju, Jv = _jac(xc[rows])
        wr = w[rows]
        A = Ju.T @ (wr[:, None] * Ju) + Jv.T @ (wr[:, None] * Jv)
        g = Ju.T @ (wr * r[rows, 0]) + Jv.T @ (wr * r[rows, 1])
        cost = float(np.sum(wr[:, None] * r[rows] ** 2))
        try:
            Lc = np.linalg.cholesky(A + lam * np.diag(np.diag(A)))
            s = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
            ok = bool(np.isfinite(s).all())
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            E = R.rot(s[:3])
            Tc = R.pose(E @ T[:3, :3], E @ T[:3, 3] + s[3:])
            _, rc, rows_c = _rows(m, sel, Tc)
            ok = bool(rows_c[rows].all()) and float(np.sum(wr[:, None] * rc[rows] ** 2)) < cost
        if ok:
            T, lam = Tc, max(lam * 0.1, 1e-12)
        else:
            lam *= 10.0
    if not np.isfinite(T).all():
        return np.eye(4), False
    return T, True


def _skew(v):
    z = torch.zeros((), dtype=torch.float64)
    return torch.stack([torch.stack([z, -v[2], v[1]]), torch.stack([v[2], z, -v[0]]), torch.stack([-v[1], v[0], z])])


def _moved(theta, T):
    """(exp([w]x) R, exp([w]x) t + d) to second order in theta: all the derivatives at theta = 0 that are taken here"""
    K = _skew(theta[:3])
    E = torch.eye(3, dtype=torch.float64) + K + 0.5 * K @ K
    return E @ T[:3, :3], E @ T[:3, 3] + theta[3:]


def _cost(theta, T, m, w):
    Rm, t = _moved(theta, T)
    xc = m[:, :3] @ Rm.T + t
    r = xc[:, :2] / xc[:, 2:] - m[:, 3:]
    return 0.5 * (w[:, None] * r ** 2).sum()


def _grad_hess(T, m, w):
    z = torch.zeros(6, dtype=torch.float64)
    H = torch.autograd.functional.hessian(lambda th: _cost(th, T, m, w), z)
    g = torch.autograd.functional.jacobian(lambda th: _cost(th, T, m, w), z)
    return g.numpy(), H.numpy()


def minimiser(m, w, mask, init, iters=200):
    """the stationary point: `lm` until it stalls, then Newton steps with the full Hessian over the rows of its result
    -> (pose, valid, rows [N] bool, H [6,6])"""
    T, ok = lm(m, w, mask, init, iters)
    sel = np.ones(len(m), bool) if mask is None else np.asarray(mask, bool)
    if not ok:
        return T, False, np.zeros(len(m), bool), np.eye(6)
    rows = _rows(m, sel, T)[2]
    w = np.ones(len(m)) if w is None else np.asarray(w, np.float64)
    mt, wt = torch.tensor(m[rows]), torch.tensor(w[rows])
    for _ in range(4):
        g, H = _grad_hess(torch.tensor(T), mt, wt)
        s = -np.linalg.solve(H, g)
        E = R.rot(s[:3])
        T = R.pose(E @ T[:3, :3], E @ T[:3, 3] + s[3:])
    g, H = _grad_hess(torch.tensor(T), mt, wt)
    return T, True, rows, H


def ift(m, w, rows, T, G, gauss_newton=False):
    """the vjp of the minimiser T over the fixed row set: G [4,4] (rows 0-2 read) -> (grad_m [N,5], grad_w [N], cond(H), lambda_min(H));
    zeros outside `rows`"""
    N = len(m)
    w = np.ones(N) if w is None else np.asarray(w, np.float64)
    Tt = torch.tensor(T)
    mt, wt = torch.tensor(m[rows], requires_grad=True), torch.tensor(w[rows], requires_grad=True)
    z = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    Rm, t = _moved(z, Tt)
    up = (torch.tensor(G[:3, :3]) * Rm).sum() + (torch.tensor(G[:3, 3]) * t).sum()
    (gth,) = torch.autograd.grad(up, z)
    _, H = _grad_hess(Tt, mt.detach(), wt.detach())
    ev = np.linalg.eigvalsh(H)
    if gauss_newton:
        xc = m[rows, :3] @ T[:3, :3].T + T[:3, 3]
        Ju, Jv = _jac(xc)
        H = Ju.T @ (w[rows, None] * Ju) + Jv.T @ (w[rows, None] * Jv)
    lam = torch.tensor(np.linalg.solve(H, gth.numpy()))
    z2 = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(_cost(z2, Tt, mt, wt), z2, create_graph=True)
    gm, gw = torch.autograd.grad(-(g * lam).sum(), (mt, wt))
    out_m, out_w = np.zeros((N, 5)), np.zeros(N)
    out_m[rows], out_w[rows] = gm.numpy(), gw.numpy()
    return out_m, out_w, float(ev.max() / ev.min()) if ev.min() > 0 else math.inf, float(ev.min())


def solve_and_grad(m, w, mask, init, G, gauss_newton=False, iters=200):
    """minimiser + ift of one pair -> dict(T, valid, rows, gm, gw, cond)"""
    T, ok, rows, H = minimiser(m, w, mask, init, iters)
    if not ok:
        return dict(T=T, valid=False, rows=rows, gm=np.zeros((len(m), 5)), gw=np.zeros(len(m)), cond=math.inf)
    gm, gw, cond, _ = ift(m, w, rows, T, G, gauss_newton)
    return dict(T=T, valid=True, rows=rows, gm=gm, gw=gw, cond=cond)


SEEDS = 4                  # one-ulp moves tried for a float64 figure (float32 has one rounding)


def _seeds(name):
    return range(SEEDS if name == "float64" else 1)


def backward_figures(m, w, mask, start, G, name):
    """-> (a = solve_and_grad on the f64 originals, figure of grad_m, figure of grad_w): the largest deviation of the reference on
    inputs as a kernel of type `name` receives them, over the seeds of as_kernel_input (those runs start from a's pose: the stationary
    point does not depend on the start)"""
    a = solve_and_grad(m, w, mask, start, G)
    fm = fw = 0.0
    for s in _seeds(name):
        k = lambda x, j: R.as_kernel_input(x, name, 10 * s + j)
        b = solve_and_grad(k(m, 1), k(w, 2), mask, a["T"], k(G, 4), iters=10)
        fm, fw = max(fm, deviation(a["gm"], b["gm"])), max(fw, deviation(a["gw"], b["gw"]))
    return a, fm, fw


def forward_figures(m, w, mask, start, name, iters=ITERS, other_starts=()):
    """-> (Tr = lm at `iters` passes on the f64 originals, figure): the largest of |Tr - lm on the kernel's inputs, its pose rounded as the
    kernel's is| over the seeds, |Tr - lm at twice the passes|, and |Tr - lm from each of `other_starts`| (a start the minimiser must
    not depend on)"""
    Tr, ok = lm(m, w, mask, start, iters)
    assert ok
    fig = deviation(Tr, lm(m, w, mask, start, 2 * iters)[0])
    for s in _seeds(name):
        k = lambda x, j: R.as_kernel_input(x, name, 10 * s + j)
        fig = max(fig, deviation(Tr, k(lm(k(m, 1), k(w, 2), mask, k(start, 3), iters)[0], 5)))
    for T0 in other_starts:
        fig = max(fig, deviation(Tr, lm(m, w, mask, T0, iters)[0]))
    return Tr, fig


# ------------------------------------------------------------------------------------------------ DLT
def dlt(m, w=None, mask=None):
    """-> (pose, valid): Hartley-normalised world points, the right singular vector of the smallest singular value of the weighted
    equations, the sign that puts the weighted majority in front, the nearest rotation, t = m / mean singular value"""
    sel = np.ones(len(m), bool) if mask is None else np.asarray(mask, bool)
    w = (np.ones(len(m)) if w is None else np.asarray(w, np.float64))[sel]
    X, uv = m[sel, :3], m[sel, 3:]
    bad = (np.eye(4), False)
    if sel.sum() < 6 or not np.isfinite(m[sel]).all() or not w.sum() > 0:
        return bad
    c = (w[:, None] * X).sum(0) / w.sum()
    s = math.sqrt(3.0) * w.sum() / float((w * np.linalg.norm(X - c, axis=1)).sum())
    Xn = np.concatenate([s * (X - c), np.ones((len(X), 1))], 1)
    z = np.zeros_like(Xn)
    A = np.concatenate([np.concatenate([Xn, z, -uv[:, :1] * Xn], 1), np.concatenate([z, Xn, -uv[:, 1:] * Xn], 1)])
    A *= np.sqrt(np.concatenate([w, w]))[:, None]
    sv, Vt = np.linalg.svd(A, full_matrices=True)[1:]
    sv = np.concatenate([sv, np.zeros(12 - len(sv))]) ** 2
    if not (sv[-2] - sv[-1]) > DLT_GAP * sv[0]:
        return bad
    Pn = Vt[-1].reshape(3, 4)
    if float((w * np.sign(Xn @ Pn[2])).sum()) < 0:
        Pn = -Pn
    M, mt = s * Pn[:, :3], Pn[:, 3] - s * Pn[:, :3] @ c
    U, S, Vt3 = np.linalg.svd(M)
    d = np.sign(np.linalg.det(U @ Vt3))
    Rm = U @ np.diag([1.0, 1.0, d]) @ Vt3
    scale = (S[0] + S[1] + d * S[2]) / 3.0
    if not scale > 0:
        return bad
    T = R.pose(Rm, mt / scale)
    return (T, True) if np.isfinite(T).all() else bad


def coplanar_case(N, seed=5):
    """a scene whose world points lie on a tilted plane in front of the camera (exact observations)"""
    rng = np.random.default_rng(seed)
    sc = R.scene(seed, N, 1.0, 0.0)
    T = sc["pose"]
    a, b = rng.uniform(-1.5, 1.5, N), rng.uniform(-1.5, 1.5, N)
    Xc = np.stack([a, b, 5.0 + 0.3 * a - 0.2 * b], 1)
    X = (Xc - T[:3, 3]) @ T[:3, :3]
    return np.concatenate([X, Xc[:, :2] / Xc[:, 2:]], 1)


def deviation(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
