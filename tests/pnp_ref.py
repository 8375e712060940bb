"""f64 numpy reference of the absolute-pose path (csrc/pnp.hip, ransac.BatchedPnP), written from the formulas and not from the
kernels: P3P through numpy.roots on the quartic and an SVD alignment, the reprojection residual with MSAC score and inlier count, the
per-pair state step, a Levenberg-Marquardt refit with the kernels' acceptance rule, a scene generator and the shapes the GPU tests use.

matches [N,5] = (X, Y, Z, u, v), (u, v) normalised; a pose is [4,4] = [[R, t], [0,0,0,1]], x_c = R X + t;
d2 = (x_c/z_c - u)^2 + (y_c/z_c - v)^2, a point with z_c <= 0 or a non-finite d2 never counts; inlier iff d2 < threshold^2.

Tolerances.  No bound here comes from a kernel's output.  For a compared quantity the tests measure `deviation`: the reference run on
inputs as the kernel receives them (`as_kernel_input`: rounded to float32, or for float64 moved by one ulp in a seeded random direction --
the smallest change of the inputs the format can express) against the reference run on the f64 originals, and allow TOL_FACTOR = 8 times
the largest figure of the case: a solver's conditioning varies by about that much across a few hundred samples, and the device rounds
its model to the type once more."""
import math

import numpy as np

THRESHOLD = 0.005          # inlier distance, normalised units (2.5 px at f = 500)
NOISE = 0.0008             # sigma of the Gaussian image noise on inliers, normalised units
TOL_FACTOR = 8.0
SEP_MIN = 1e-3             # a sample is compared only if the quartic's four complex roots are pairwise at least this far apart (relative)
TRI_MIN = 1e-4             # ... and sin^2 of the world triangle's angle at point 0 and of every angle between two bearings is at least this
DEGENERATE = 1e-12         # below this sin^2 (1e-6 rad) a sample has no solution at all: the header's rule (coincident points give 0 / 0 -> none)
EXCLUDED_MAX = 0.05        # at most this share of a case's samples may be left out
GPU_CASES = [(1, 64, 1), (1, 64, 65), (3, 64, 33)]          # (P, N, B) of the solver test
SCORE_N = (7, 300, 2049)
M_SLOTS = 132
DRV = dict(P=3, N=257, B=64, max_iterations=256, shares=(0.2, 0.35, 0.7), seed=5)


def eps_of(name):
    return float(np.finfo(np.float32 if name == "float32" else np.float64).eps)


def as_kernel_input(a, name, seed=0):
    """the array as a kernel of type `name` sees it, in f64: rounded to float32, or every entry one float64 ulp up or down"""
    a = np.asarray(a, np.float64)
    if name == "float32":
        return a.astype(np.float32).astype(np.float64)
    up = np.random.default_rng(seed).random(a.shape) < 0.5
    return np.where(up, np.nextafter(a, np.inf), np.nextafter(a, -np.inf))


# ------------------------------------------------------------------------------------------------ poses
def rot(w):
    """exp([w]x), Rodrigues"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def rot_angle(Ra, Rb):
    """the angle of Ra^T Rb in radians, from the skew part below 0.1 rad (acos loses half the digits there)"""
    D = Ra.T @ Rb
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    c = 0.5 * (np.trace(D) - 1.0)
    return float(math.atan2(s, c))


def pose_error(Ta, Tb):
    return rot_angle(Ta[:3, :3], Tb[:3, :3]), float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3]))


def scene(seed, N, share, noise=NOISE):
    """a random pose, N points in a box in front of the camera, round(share N) inliers with Gaussian image noise, uniform outliers"""
    rng = np.random.default_rng(seed)
    R, t = rot(rng.normal(0, 0.4, 3)), np.concatenate([rng.uniform(-0.5, 0.5, 2), [0.0]])
    Xc = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.5, 1.5, N), rng.uniform(3.0, 7.0, N)], 1)
    X = (Xc - t) @ R                                   # R^T (Xc - t), row-wise
    uv = Xc[:, :2] / Xc[:, 2:]
    inl = np.zeros(N, bool)
    inl[rng.permutation(N)[:int(round(share * N))]] = True
    uv = np.where(inl[:, None], uv + rng.normal(0, noise, (N, 2)), rng.uniform(-0.6, 0.6, (N, 2)))
    return dict(matches=np.concatenate([X, uv], 1), pose=pose(R, t), inlier=inl)


# ------------------------------------------------------------------------------------------------ P3P
def _align(X, Y):
    """the proper rotation and translation with Y_i ~ R X_i + t (Kabsch by SVD)"""
    xm, ym = X.mean(0), Y.mean(0)
    U, _, Vt = np.linalg.svd((Y - ym).T @ (X - xm))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, ym - R @ xm


def p3p(m3):
    """m3 [3,5] -> (poses [k,4,4] in ascending order of the quartic's root, info): Grunert's P3P in the ratio form.  With bearings f_i,
    depths s_1 = x s_0, s_2 = v s_0 and g(v) = 1 + v^2 - 2 v cb: x = p(v) / q(v), p = (K-1) v^2 - 2 K cb v + K + 1, q = 2 (cg - v ca),
    K = (a^2 - c^2) / b^2, and p^2 - 2 cg p q + q^2 (1 - c^2 / b^2 g) = 0.  info: sep = the smallest relative distance between two of the
    quartic's complex roots, tri = the smallest sin^2 among the world triangle's angle at point 0 and the bearings' angles."""
    m3 = np.asarray(m3, np.float64)
    X = m3[:, :3]
    f = np.concatenate([m3[:, 3:], np.ones((3, 1))], 1)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    a2, b2, c2 = np.sum((X[1] - X[2]) ** 2), np.sum((X[0] - X[2]) ** 2), np.sum((X[0] - X[1]) ** 2)
    none = np.zeros((0, 4, 4))
    with np.errstate(all="ignore"):
        tri = [np.sum(np.cross(X[1] - X[0], X[2] - X[0]) ** 2) / (b2 * c2)]
        tri += [np.sum(np.cross(f[i], f[j]) ** 2) for i, j in ((0, 1), (0, 2), (1, 2))]
    tri = min(float(x) if np.isfinite(x) else 0.0 for x in tri)
    if not (min(a2, b2, c2) > 0 and tri > DEGENERATE):
        return none, dict(sep=np.inf, tri=0.0)
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    K = (a2 - c2) / b2
    p = np.array([K - 1.0, -2.0 * K * cb, K + 1.0])                 # descending, as numpy's polynomials are
    q = np.array([-2.0 * ca, 2.0 * cg])
    g = np.array([1.0, -2.0 * cb, 1.0])
    quartic = np.polyadd(np.polysub(np.polymul(p, p), 2.0 * cg * np.polymul(p, q)),
                         np.polymul(np.polymul(q, q), np.polysub([1.0], c2 / b2 * g)))
    roots = np.roots(quartic)
    sep = np.inf
    for i in range(len(roots)):
        for j in range(i + 1, len(roots)):
            sep = min(sep, abs(roots[i] - roots[j]) / (1.0 + max(abs(roots[i]), abs(roots[j]))))
    if len(roots) < 4:
        sep = 0.0                                                      # a vanishing leading coefficient: a root at infinity
    out = []
    for v in sorted(float(r.real) for r in roots if abs(r.imag) < 1e-8 * (1.0 + abs(r.real))):
        if not v > 0:
            continue
        x = np.polyval(p, v) / np.polyval(q, v)
        s = np.sqrt(b2 / np.polyval(g, v)) * np.array([1.0, x, v])
        for _ in range(6):                                             # Newton on the three law-of-cosines equations
            F = np.array([s[1] ** 2 + s[2] ** 2 - 2 * s[1] * s[2] * ca - a2, s[0] ** 2 + s[2] ** 2 - 2 * s[0] * s[2] * cb - b2,
                          s[0] ** 2 + s[1] ** 2 - 2 * s[0] * s[1] * cg - c2])
            J = 2.0 * np.array([[0, s[1] - s[2] * ca, s[2] - s[1] * ca], [s[0] - s[2] * cb, 0, s[2] - s[0] * cb],
                                [s[0] - s[1] * cg, s[1] - s[0] * cg, 0]])
            try:
                d = np.linalg.solve(J, F)
            except np.linalg.LinAlgError:
                break
            if not np.isfinite(d).all():
                break
            s = s - d
        if not (np.isfinite(s).all() and (s > 0).all()):
            continue
        R, t = _align(X, s[:, None] * f)
        if np.isfinite(R).all() and np.isfinite(t).all() and ((X @ R.T + t)[:, 2] > 0).all():
            out.append(pose(R, t))
    return (np.stack(out) if out else none), dict(sep=float(sep), tri=tri)


def comparable(info):
    """may a device result be compared on this sample: the reference alone decides, from its own roots and triangle"""
    return info["tri"] == 0.0 or (info["sep"] >= SEP_MIN and info["tri"] >= TRI_MIN)


def slots(m, idx):
    """the contract's layout for index sets idx [B,3]: (models [4B,4,4], valid [4B], infos): valid slots first, identity elsewhere"""
    B = len(idx)
    models, valid, infos = np.tile(np.eye(4), (4 * B, 1, 1)), np.zeros(4 * B, bool), []
    for b in range(B):
        sol, info = p3p(m[idx[b]])
        infos.append(info)
        models[4 * b:4 * b + len(sol)], valid[4 * b:4 * b + len(sol)] = sol, True
    return models, valid, infos


# ------------------------------------------------------------------------------------------------ residual, score
def residual(m, T):
    """-> (d2 [N], counts [N] bool: in front of the camera with a finite d2)"""
    with np.errstate(all="ignore"):
        xc = m[:, :3] @ T[:3, :3].T + T[:3, 3]
        d2 = (xc[:, 0] / xc[:, 2] - m[:, 3]) ** 2 + (xc[:, 1] / xc[:, 2] - m[:, 4]) ** 2
        return d2, (xc[:, 2] > 0) & np.isfinite(d2)


def msac(m, T, thr):
    """-> (score, inliers); a non-finite model scores NaN with 0 inliers"""
    if not np.isfinite(T[:3]).all():
        return math.nan, 0
    d2, ok = residual(m, T)
    inl = ok & (d2 < thr * thr)
    return float(np.sum(1.0 - d2[inl] / (thr * thr))), int(inl.sum())


def inlier_mask(m, T, thr):
    if not np.isfinite(T[:3]).all():
        return np.zeros(len(m), bool)
    d2, ok = residual(m, T)
    return ok & (d2 < thr * thr)


def score_all(m, models, valid, thr):
    """-> (scores [M], inliers [M]): an invalid slot scores exactly 0"""
    out = [(0.0, 0) if not v else msac(m, T, thr) for T, v in zip(models, valid)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def band_counts(m, models, valid, thr, width):
    """per slot the number of points whose d2 / thr^2 lies within `width` of 1: the points whose inlier decision a relative error of
    `width` in d2 can turn"""
    out = np.zeros(len(models), int)
    for j, (T, v) in enumerate(zip(models, valid)):
        if v and np.isfinite(T[:3]).all():
            d2, ok = residual(m, T)
            out[j] = int((ok & (np.abs(d2 / (thr * thr) - 1.0) <= width)).sum())
    return out


# ------------------------------------------------------------------------------------------------ the state step
def adaptive_max_iters(inliers, N, k, confidence, eps, max_iterations):
    rk = (inliers / N) ** k
    if 1.0 - rk >= 1.0 - eps:
        return float(max_iterations)
    return min(float(max_iterations), max(0.0, math.log10(1.0 - confidence) / math.log10(1.0 - rk + eps)))


def new_state(N, max_iterations):
    return dict(score=0.0, model=np.eye(4), mask=np.zeros(N, bool), inliers=0, iters=0, max_iters=float(max_iterations))


def step(st, m, models, valid, scores, thr, B, confidence=0.999, eps=1e-5, max_iterations=5000):
    """one round on a pair's state, in place: nothing for a terminated pair; the FIRST arg-max over valid, non-NaN scores replaces the
    state on a STRICTLY higher score; the adaptive bound with sample size 3; iters += B"""
    if st["iters"] >= st["max_iters"]:
        return st
    cand = [j for j in range(len(scores)) if valid[j] and not math.isnan(scores[j])]
    if cand:
        j = max(cand, key=lambda q: (scores[q], -q))
        if scores[j] > st["score"]:
            mask = inlier_mask(m, models[j], thr)
            st.update(score=float(scores[j]), model=models[j].copy(), mask=mask, inliers=int(mask.sum()),
                      max_iters=adaptive_max_iters(int(mask.sum()), len(m), 3, confidence, eps, max_iterations))
    st["iters"] += B
    return st


# ------------------------------------------------------------------------------------------------ LM refit
def lm_refit(m, mask, init, iters=10):
    """Levenberg-Marquardt on the reprojection error over the mask's rows in front of the camera under the current iterate, from `init`:
    (J^T J + lambda diag) step = -J^T r, step = (w, d) applied on the left (R' = exp(w) R, t' = exp(w) t + d), taken only on a strictly
    lower cost over the same rows with none of them lost (lambda / 10, floor 1e-12), else lambda x 10; lambda starts at 1e-3.
    -> (pose, valid, cost of the result over its own rows)"""
    T = np.array(init, np.float64)
    sel = np.ones(len(m), bool) if mask is None else np.asarray(mask, bool)

    def rows_of(T):
        with np.errstate(all="ignore"):
            xc = m[:, :3] @ T[:3, :3].T + T[:3, 3]
            r = np.stack([xc[:, 0] / xc[:, 2] - m[:, 3], xc[:, 1] / xc[:, 2] - m[:, 4]], 1)
        return xc, r, sel & (xc[:, 2] > 0) & np.isfinite(r).all(1)

    if not np.isfinite(T[:3]).all() or rows_of(T)[2].sum() < 3:
        return np.eye(4), False, math.nan
    lam = 1e-3
    for _ in range(iters):
        xc, r, rows = rows_of(T)
        iz = 1.0 / xc[rows, 2]
        x, y, z0 = xc[rows, 0] * iz, xc[rows, 1] * iz, np.zeros(rows.sum())
        Ju = np.stack([-x * y, 1 + x * x, -y, iz, z0, -x * iz], 1)
        Jv = np.stack([-1 - y * y, x * y, x, z0, iz, -y * iz], 1)
        A = Ju.T @ Ju + Jv.T @ Jv
        g = Ju.T @ r[rows, 0] + Jv.T @ r[rows, 1]
        cost = float(np.sum(r[rows] ** 2))
        try:
            L = np.linalg.cholesky(A + lam * np.diag(np.diag(A)))
            s = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            ok = bool(np.isfinite(s).all())
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            E = rot(s[:3])
            Tc = pose(E @ T[:3, :3], E @ T[:3, 3] + s[3:])
            _, rc, rows_c = rows_of(Tc)
            ok = bool(rows_c[rows].all()) and float(np.sum(rc[rows] ** 2)) < cost
        if ok:
            T, lam = Tc, max(lam * 0.1, 1e-12)
        else:
            lam *= 10.0
    if not np.isfinite(T).all():
        return np.eye(4), False, math.nan
    _, r, rows = rows_of(T)
    return T, True, float(np.sum(r[rows] ** 2))


def cost_over(m, rows, T):
    """sum |r|^2 of pose T over the given rows (inf where one of them is not in front of the camera)"""
    d2, ok = residual(m[rows], T)
    return float(d2.sum()) if ok.all() else math.inf


def perturbed(T, rng, deg=3.0, depth=0.03):
    """the pose turned by `deg` degrees about a random axis and moved by `depth` of the scene's depth (5)"""
    w = rng.normal(size=3)
    w *= math.radians(deg) / np.linalg.norm(w)
    d = rng.normal(size=3)
    d *= depth * 5.0 / np.linalg.norm(d)
    return pose(rot(w) @ T[:3, :3], T[:3, 3] + d)


# ------------------------------------------------------------------------------------------------ the whole call
def run(m, idx_rounds, thr, B, max_iterations, confidence=0.999, eps=1e-5, refit=True, refit_iters=10):
    """the driver on one pair with the given index sets per round [B,3]: -> dict(model, mask, score, inliers, iterations, rounds)"""
    st, rounds = new_state(len(m), max_iterations), 0
    for idx in idx_rounds:
        if st["iters"] >= st["max_iters"]:
            break
        models, valid, _ = slots(m, idx)
        scores, _ = score_all(m, models, valid, thr)
        step(st, m, models, valid, scores, thr, B, confidence, eps, max_iterations)
        rounds += 1
    model, score = st["model"], st["score"]
    if refit:
        cand, ok, _ = lm_refit(m, st["mask"], st["model"], refit_iters)
        cs = msac(m, cand, thr)[0] if ok else 0.0
        if cs > score:
            model, score = cand, cs
    return dict(model=model, mask=st["mask"], score=score, inliers=st["inliers"], iterations=st["iters"], rounds=rounds, state=st)


# ------------------------------------------------------------------------------------------------ the GPU tests' cases
def solver_case(P, N, B, seed=11):
    """-> (matches [P,N,5], idx [P,B,3] int32): scenes at 60 % inliers, distinct random triples"""
    rng = np.random.default_rng(seed + 7 * B)
    m = np.stack([scene(seed + p, N, 0.6)["matches"] for p in range(P)])
    idx = np.stack([np.stack([rng.permutation(N)[:3] for _ in range(B)]) for _ in range(P)]).astype(np.int32)
    return m, idx


def score_case(N, seed=21):
    """-> (matches [3,N,5], models [3,M_SLOTS,4,4], valid [3,M_SLOTS], poses): P3P slots of 32 random samples per pair, then slot 128 =
    the generating pose, 129 = a perturbed one, 130 = a NaN model (valid), 131 = a pose claimed invalid; the last point of every pair lies
    BEHIND the camera of the generating pose on the ray of its own observation (d2 = 0 there, and it must add nothing)"""
    P, rng = 3, np.random.default_rng(seed + N)
    ms, mo, va, poses = [], [], [], []
    for p in range(P):
        sc = scene(seed + 31 * p + N, N, 0.6)
        m, T = sc["matches"].copy(), sc["pose"]
        xc = -2.0 * np.array([m[-1, 3], m[-1, 4], 1.0])
        m[-1, :3] = T[:3, :3].T @ (xc - T[:3, 3])
        idx = np.stack([rng.permutation(N)[:3] for _ in range(32)])
        models, valid, _ = slots(m, idx)
        extra = np.stack([T, perturbed(T, rng, 0.2, 0.002), np.full((4, 4), np.nan), T])
        ms.append(m), mo.append(np.concatenate([models, extra])), va.append(np.concatenate([valid, [True, True, True, False]]))
        poses.append(T)
    return np.stack(ms), np.stack(mo), np.stack(va), poses


def deviation(fn, args_f64, args_in):
    """max |fn(inputs as the kernel receives them) - fn(f64 originals)| over the entries both runs give finite"""
    a, b = np.asarray(fn(*args_f64), np.float64), np.asarray(fn(*args_in), np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.abs(a - b)[ok].max()) if ok.any() else 0.0


def pose_sigma(m, rows, T, noise):
    """first-order standard deviations (rotation angle in rad, translation) of the least-squares pose over `rows` under image noise of
    sigma `noise` per coordinate: C = noise^2 (J^T J)^-1 at T in the left-multiplied step (w, d) of lm_refit; the rotation error is |w|,
    the translation moves by w x t + d, so sigma_rot = sqrt(tr C_ww), sigma_t <= sqrt(tr C_dd) + |t| sigma_rot"""
    xc = m[rows, :3] @ T[:3, :3].T + T[:3, 3]
    iz = 1.0 / xc[:, 2]
    x, y, z0 = xc[:, 0] * iz, xc[:, 1] * iz, np.zeros(len(xc))
    Ju = np.stack([-x * y, 1 + x * x, -y, iz, z0, -x * iz], 1)
    Jv = np.stack([-1 - y * y, x * y, x, z0, iz, -y * iz], 1)
    C = noise ** 2 * np.linalg.inv(Ju.T @ Ju + Jv.T @ Jv)
    srot = math.sqrt(np.trace(C[:3, :3]))
    return srot, math.sqrt(np.trace(C[3:, 3:])) + float(np.linalg.norm(T[:3, 3])) * srot


def driver_scenes():
    return [scene(DRV["seed"] + 100 * p, DRV["N"], s) for p, s in enumerate(DRV["shares"])]
