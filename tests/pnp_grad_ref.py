"""f64 numpy reference of the trainable absolute-pose path (dr_p3p_bwd, dr_pnp_loss_*; ops.p3p, loss.PnPLoss), written from the
formulas and not from the kernels.  The poses come from tests/pnp_ref.py.

The P3P reverse pass.  A valid pose T = [[R, t], [0, 1]] of a sample m3 [3,5] is a root of r(theta; m3) = 0, the six reprojection
residuals r_i = (x_c / z_c - u_i, y_c / z_c - v_i) at x_c = R X_i + t.  With the left-multiplied step theta = (w, d) of pnp_ref.lm_refit
(R' = exp([w]x) R, t' = exp([w]x) t + d) and J = d r / d theta the implicit function theorem gives d theta / d m3 = -J^-1 d r / d m3, so
for an incoming G = d L / d T (rows 0-2):
    g_theta = (sum_j R[:,j] x G_R[:,j] + t x G_t, G_t),   J^T lambda = g_theta,
    d L / d X_i = -(A_i R)^T lambda_i,   d L / d (u, v)_i = lambda_i,   A_i = (1 / z_c) [[1, 0, -x], [0, 1, -y]].
test_pnp_train_host.py checks it against central differences of pnp_ref.p3p.
The theorem holds at the root.  pnp_ref.p3p's pose lies a few ulp times the sample's conditioning away from it, and on an
ill-conditioned sample the derivative evaluated there is off by more than the GPU test allows a kernel (a derivative evaluated exactly
at the root would miss 8 x the per-sample figure by a factor of two on samples of the test's cases).  p3p_vjp_slots therefore moves every
pose onto the root first (root_pose: Gauss-Newton with the residual in extended precision), so that its own error stays below the bound
it is used to enforce.

The loss.  d2 = (x_c / z_c - u)^2 + (y_c / z_c - v)^2, term = d2 / thr^2 if z_c > 0 and d2 < thr^2 else 1, sums[p,m] over the masked
points, per_pair[p] = sum over kept m / max(#kept #mask, 1), mean over the pairs; a slot keep drops has sums 0 and no gradient, a kept
model with a non-finite entry (or a threshold that is not > 0) counts 1 per masked point and has no gradient."""
import numpy as np

from tests import pnp_ref as R


def _jacobian(m3, T):
    """-> (J [6,6], A [3,2,3]): rows 2 i, 2 i + 1 = d r_i / d (w, d) at x_c = R X_i + t"""
    Rm, t = T[:3, :3], T[:3, 3]
    J, A = np.zeros((6, 6)), np.zeros((3, 2, 3))
    for i in range(3):
        xc = Rm @ m3[i, :3] + t
        iz = 1.0 / xc[2]
        x, y = xc[0] * iz, xc[1] * iz
        A[i] = iz * np.array([[1.0, 0.0, -x], [0.0, 1.0, -y]])
        skew = np.array([[0.0, -xc[2], xc[1]], [xc[2], 0.0, -xc[0]], [-xc[1], xc[0], 0.0]])
        J[2 * i:2 * i + 2] = A[i] @ np.concatenate([-skew, np.eye(3)], 1)
    return J, A


def p3p_vjp(m3, T, G):
    """m3 [3,5], one of its poses T [4,4], G [4,4] = d L / d T (row 3 is not read) -> d L / d m3 [3,5]"""
    m3, T, G = (np.asarray(a, np.float64) for a in (m3, T, G))
    Rm, t = T[:3, :3], T[:3, 3]
    gw = np.cross(t, G[:3, 3]) + sum(np.cross(Rm[:, j], G[:3, j]) for j in range(3))
    J, A = _jacobian(m3, T)
    lam = np.linalg.solve(J.T, np.concatenate([gw, G[:3, 3]]))
    out = np.zeros((3, 5))
    for i in range(3):
        out[i, :3] = -(A[i] @ Rm).T @ lam[2 * i:2 * i + 2]
        out[i, 3:] = lam[2 * i:2 * i + 2]
    return out


def root_pose(m3, T, iters=3):
    """the pose moved onto the root of the sample's six reprojection equations: Gauss-Newton steps delta = -J^-1 r with r evaluated in
    numpy.longdouble (J and the solve in f64: iterative refinement), applied on the left, exp([w]x) to second order (|w| ~ 1e-14)"""
    LD = np.longdouble
    m3 = np.asarray(m3, np.float64)
    Rm, t = np.asarray(T[:3, :3], LD), np.asarray(T[:3, 3], LD)
    X, uv = m3[:, :3].astype(LD), m3[:, 3:].astype(LD)
    for _ in range(iters):
        xc = X @ Rm.T + t
        r = np.stack([xc[:, 0] / xc[:, 2] - uv[:, 0], xc[:, 1] / xc[:, 2] - uv[:, 1]], 1).reshape(6)
        d = np.linalg.solve(_jacobian(m3, R.pose(Rm.astype(np.float64), t.astype(np.float64)))[0], -r.astype(np.float64)).astype(LD)
        K = np.array([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]], LD)
        E = np.eye(3, dtype=LD) + K + K @ K / 2
        Rm, t = E @ Rm, E @ t + d[3:]
    return R.pose(Rm.astype(np.float64), t.astype(np.float64))


def p3p_vjp_slots(m, idx, G):
    """m [N,5], idx [B,3], G [4B,4,4] in the contract's layout (slots 4 b + j, the valid ones first) -> (grad [B,3,5] = the sum of
    p3p_vjp over each sample's valid slots, each at root_pose of the slot's pose, valid [4B], infos); the gradient of an invalid slot is
    never read"""
    models, valid, infos = R.slots(m, idx)
    out = np.zeros((len(idx), 3, 5))
    for b in range(len(idx)):
        for j in range(4 * b, 4 * b + 4):
            if valid[j]:
                out[b] += p3p_vjp(m[idx[b]], root_pose(m[idx[b]], models[j]), G[j])
    return out, valid, infos


# ------------------------------------------------------------------------------------------------ the loss
def _thr2(thr, P):
    return np.broadcast_to(np.asarray(thr, np.float64) ** 2, (P,))


def _point_grads(m, T, thr2):
    """one model on the points m [n,5] -> (d2 [n], front [n], g [n,4,4]): the derivative of d2 / thr2 with respect to T at EVERY point,
    h = (2 / thr2) (e_0 i, e_1 i, -(e_0 x + e_1 y) i), d / dt = h, d / dR = h X^T, row 3 zero"""
    with np.errstate(all="ignore"):
        xc = m[:, :3] @ T[:3, :3].T + T[:3, 3]
        iz = 1.0 / xc[:, 2]
        x, y = xc[:, 0] * iz, xc[:, 1] * iz
        e0, e1 = x - m[:, 3], y - m[:, 4]
        d2 = e0 * e0 + e1 * e1
        h = (2.0 / thr2) * np.stack([e0 * iz, e1 * iz, -(e0 * x + e1 * y) * iz], 1)
    g = np.zeros((len(m), 4, 4))
    g[:, :3, :3] = h[:, :, None] * m[:, None, :3]
    g[:, :3, 3] = h
    return d2, xc[:, 2] > 0, g


def point_terms(m, T, thr2):
    """-> (term [n], live [n], d term / d T [n,4,4]: zeros at a point that is not live)"""
    d2, front, g = _point_grads(m, T, thr2)
    with np.errstate(all="ignore"):
        live = front & (d2 < thr2)
    g[~live] = 0.0
    return np.where(live, d2 / thr2, 1.0), live, g


def pnp_loss(m, mask, models, keep, thr):
    """m [P,N,5], mask [P,N] bool | None, models [P,M,4,4], keep [P,M] bool | None, thr = distance, scalar or [P] ->
    (sums [P,M], per_pair [P], mean, grad_models [P,M,4,4] = d mean / d models)"""
    P, N, M = m.shape[0], m.shape[1], models.shape[1]
    mask = np.ones((P, N), bool) if mask is None else np.asarray(mask, bool)
    keep = np.ones((P, M), bool) if keep is None else np.asarray(keep, bool)
    thr2 = _thr2(thr, P)
    sums, grad, per_pair = np.zeros((P, M)), np.zeros((P, M, 4, 4)), np.zeros(P)
    for p in range(P):
        coef = 1.0 / max(int(mask[p].sum()) * int(keep[p].sum()), 1)
        for j in np.flatnonzero(keep[p]):
            if not (np.isfinite(models[p, j, :3]).all() and thr2[p] > 0):
                sums[p, j] = mask[p].sum()
                continue
            term, _, g = point_terms(m[p][mask[p]], models[p, j], thr2[p])
            sums[p, j] = term.sum()
            grad[p, j] = g.sum(0) * coef / P
        per_pair[p] = sums[p].sum() * coef
    return sums, per_pair, float(per_pair.mean()), grad


def pnp_loss_bands(m, mask, models, keep, thr, width):
    """per slot (count [P,M], size [P,M]): the masked points whose d2 / thr^2 lies within `width` of 1 in front of the camera -- the
    points whose `live` decision a relative error of `width` in d2 can turn -- and the sum over them of the largest |entry| of the
    point's term in grad_models (what one such decision moves the gradient by; it moves sums by at most `width`)"""
    P, N, M = m.shape[0], m.shape[1], models.shape[1]
    mask = np.ones((P, N), bool) if mask is None else np.asarray(mask, bool)
    keep = np.ones((P, M), bool) if keep is None else np.asarray(keep, bool)
    thr2 = _thr2(thr, P)
    count, size = np.zeros((P, M), int), np.zeros((P, M))
    for p in range(P):
        coef = 1.0 / max(int(mask[p].sum()) * int(keep[p].sum()), 1)
        for j in np.flatnonzero(keep[p]):
            if not np.isfinite(models[p, j, :3]).all():
                continue
            pts = m[p][mask[p]]
            d2, ok = R.residual(pts, models[p, j])
            band = ok & (np.abs(d2 / thr2[p] - 1.0) <= width)
            if band.any():
                g = _point_grads(pts[band], models[p, j], thr2[p])[2]
                count[p, j], size[p, j] = int(band.sum()), float(np.abs(g).reshape(len(g), -1).max(1).sum()) * coef / P
    return count, size

