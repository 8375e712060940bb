"""f64 numpy oracle of the homography path (csrc/homography.hip, ransac.BatchedHomography), written from the maths of the kernels and
not from their code, the scene generator its tests share, and the tolerances those tests use.

Conventions: matches [N,4] = (x1, y1, x2, y2) in pixels; a model is the 3x3 H with x2 ~ H x1, unit Frobenius norm, det H > 0.
Residual: y = H (x1, 1), z = adj(H) (x2, 1), d2 = |x2 - y_xy / y_w|^2 + |x1 - z_xy / z_w|^2 under the det > 0 sign; a point with
y_w <= 0 or z_w <= 0, or a non-finite d2, is an outlier.  `threshold` is a DISTANCE: inlier iff d2 < threshold^2, MSAC score =
sum_n max(0, 1 - d2_n / threshold^2).

  closed_form   four matches -> H.  Per image q_i = x_i - centroid, s = sqrt(2) / mean |q_i|, p_i = (s q_i, 1); the orientation
                determinants D_3 = [q0 q1 q2], D_0 = [q3 q1 q2], D_1 = [q0 q3 q2], D_2 = [q0 q1 q3]; lambda_i = D_i / D_3;
                A = [lambda_i p_i]; H = T2^-1 A2 adj(A1) T1, unit norm, det > 0.  Valid iff every D is non-zero with the same sign in
                both images and H is finite with det != 0.  conditioning = min |lambda| / max |lambda| over both images.
  dlt           the normalised DLT by SVD (numpy.linalg.svd of the 2n x 9 system): the refit, and the closed form's cross-check.
  ratio2, msac, update, stop_rule (sample size 4), refit, run: as tests/registration_ref.py has them, on this residual; `update`
                replaces the state only on a strictly higher score.

Tolerances (eps = the machine epsilon of the kernel's type; eps32 = 1.19e-7, eps64 = 2.22e-16), each from the operations as written:

  model_tolerance    max |H_kernel - H_oracle| entrywise on unit-norm models.  The solver works in f64 for either type.  Its longest
                path -- centroid, q, |q|, s, a determinant (7 operations), lambda, a column of A, an adjugate entry, a row of A2 adj(A1),
                the two similarity products, the norm and the scaling -- is 64 roundings of half an ulp each.  H is
                P2 diag(lambda2_i / lambda1_i) P1^-1 up to scale, so a relative error of a lambda reaches H amplified by at most
                max |lambda| / min |lambda| = 1 / conditioning, once per image: 64 x 1/2 x 2 / conditioning = 64 eps64 / conditioning.
                A determinant is a sum of three signed products, so its own relative error is not a rounding but a rounding times
                its condition number sum |terms| / |D| >= 1; `cancellation` is the largest of the eight (closed_form returns it),
                and every lambda = D_i / D_3 inherits it.  Safety factor 2:
                tol64 = 128 eps64 cancellation / conditioning   (2.8e-12 x cancellation at the well-conditioned limit 1e-2).
                An f32 caller sees that plus the rounding of the output, eps32 / 2 per entry of magnitude <= 1; safety factor 2:
                tol32 = eps32 + tol64 = 1.19e-7.
  d2_bound      per point, from the magnitudes of that point (see the function): two roundings per linear form, two per adjugate
                entry, one per reciprocal (v_rcp_f32: 1 ulp) and product, four for the sum of squares; safety factor 2.
  BAND          |d2 / thr2 - 1| < BAND[dtype]: inside it an inlier decision may differ.  At the cutoff sum |e| <= 2 thr over the four
                residual components, so delta d2 / thr2 <= 4 delta_e / thr; delta_e <= X rho eps with X = 1024 the bound of a
                coordinate here (640-pixel square, shifts and scale included) and rho = 16 relative roundings of a transfer (two per
                linear form for numerator and denominator, each with |terms| / |sum| <= 2; the adjugate's two; reciprocal, product
                and subtraction): 4 x 1024 x 16 eps / 3, safety factor 2:   BAND = 131072 eps / 3 = 5.2e-3 (f32), 9.7e-12 (f64).
  score_tolerance    the d2_bound of every point at or inside the band's outer edge, over thr2, plus the reduction: `depth` = 8
                (a lane's points) + 6 (the wave tree) + chunks + 4 (waves) additions of partial sums <= score, half an ulp each;
                safety factor 2 (d2_bound's own included).
  grad_tolerance     |<g_kernel - g_autograd, delta>| <= tol |g_autograd| |delta|.  The reverse pass is twice the forward's length
                (128 roundings) and divides by D_3 once more: 128 x 1/2 x 2 / conditioning^2, safety factor 2:
                tol64 = 256 eps64 / conditioning^2 (5.7e-10 at 1e-2); f32 adds the rounding of the 16 outputs, eps32 / 2 each
                (Cauchy-Schwarz: eps32 / 2 |g| |delta|), safety factor 2: tol32 = eps32 + tol64.
  refit_tolerance    the smallest eigenvector of the Gram matrix G = A^T A (Jacobi, converged to 2e-30 in the off-diagonal mass): a
                perturbation of eps |G| turns it by eps sigma_1^2 / (sigma_8^2 - sigma_9^2).  64 roundings of half an ulp on a Gram
                entry's path and through the rotations' accumulated product (30 sweeps at most, 4 needed), safety factor 2:
                tol64 = 64 eps64 sigma_1^2 / (sigma_8^2 - sigma_9^2), with the oracle's singular values; tol32 = eps32 + tol64."""
import math

import numpy as np

THRESHOLD = 3.0
WELL = 1e-2                                                      # a sample is well conditioned above this
BAND = {"float32": 131072.0 * float(np.finfo(np.float32).eps) / 3.0, "float64": 131072.0 * float(np.finfo(np.float64).eps) / 3.0}
WELL_SHARE_MIN = 0.8                                             # cap: well-conditioned samples, of P B
BAND_SHARE_MAX = 0.01                                            # cap: cells inside the guard band


def eps_of(dtype_name):
    return float(np.finfo(dtype_name).eps)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def random_h(rng, side=640.0):
    """rotation <= 0.4 rad, scale 0.8-1.25, shift <= 40 px about the centre, perspective terms <= 3e-4 (about the centre too)"""
    a, s = rng.uniform(-0.4, 0.4), rng.uniform(0.8, 1.25)
    c = 0.5 * side
    S = np.array([[s * math.cos(a), -s * math.sin(a), rng.uniform(-40, 40)], [s * math.sin(a), s * math.cos(a), rng.uniform(-40, 40)],
                  [rng.uniform(-3e-4, 3e-4), rng.uniform(-3e-4, 3e-4), 1.0]])
    C = np.array([[1, 0, c], [0, 1, c], [0, 0, 1.0]])
    return canonical(C @ S @ np.linalg.inv(C))


def scene(seed, N, inlier_share, noise=0.5, side=640.0):
    """-> dict(matches [N,4], H, inlier [N] bool): x1 uniform in the square; inliers x2 = H x1 + N(0, noise^2), outliers uniform"""
    rng = np.random.default_rng(seed)
    H = random_h(rng, side)
    x1 = rng.uniform(0.0, side, (N, 2))
    y = np.concatenate([x1, np.ones((N, 1))], 1) @ H.T
    x2 = y[:, :2] / y[:, 2:]
    n_in = int(round(inlier_share * N))
    inlier = np.zeros(N, dtype=bool)
    inlier[rng.permutation(N)[:n_in]] = True
    x2 = np.where(inlier[:, None], x2 + noise * rng.standard_normal((N, 2)), rng.uniform(0.0, side, (N, 2)))
    return dict(matches=np.concatenate([x1, x2], 1), H=H, inlier=inlier)


# ---- models ------------------------------------------------------------------------------------------------------------------------
def identity():
    return np.eye(3)


def canonical(H):
    """unit Frobenius norm, det > 0; None for a non-finite or singular matrix"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    if not np.isfinite(H).all():
        return None
    n = np.linalg.norm(H)
    if not (n > 0 and np.isfinite(n)):
        return None
    H = H / n
    d = np.linalg.det(H)
    if not np.isfinite(d) or d == 0.0:
        return None
    return H if d > 0 else -H


def adjugate(H):
    H = np.asarray(H, np.float64).reshape(3, 3)
    return np.array([np.cross(H[:, 1], H[:, 2]), np.cross(H[:, 2], H[:, 0]), np.cross(H[:, 0], H[:, 1])])


def _tri(q, i, j, k):
    return q[i, 0] * (q[j, 1] - q[k, 1]) - q[j, 0] * (q[i, 1] - q[k, 1]) + q[k, 0] * (q[i, 1] - q[j, 1])


def _tri_abs(q, i, j, k):
    """the sum of the absolute values of the determinant's three terms"""
    return abs(q[i, 0] * (q[j, 1] - q[k, 1])) + abs(q[j, 0] * (q[i, 1] - q[k, 1])) + abs(q[k, 0] * (q[i, 1] - q[j, 1]))


def _image(x):
    c = x.mean(0)
    q = x - c
    s = math.sqrt(2.0) / np.linalg.norm(q, axis=1).mean() if np.linalg.norm(q, axis=1).mean() > 0 else math.inf
    D = np.array([_tri(q, 3, 1, 2), _tri(q, 0, 3, 2), _tri(q, 0, 1, 3), _tri(q, 0, 1, 2)])
    with np.errstate(all="ignore"):
        lam = D[:3] / D[3]
        A = np.stack([lam * s * q[:3, 0], lam * s * q[:3, 1], lam])
    T = np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    with np.errstate(all="ignore"):
        canc = np.array([_tri_abs(q, 3, 1, 2), _tri_abs(q, 0, 3, 2), _tri_abs(q, 0, 1, 3), _tri_abs(q, 0, 1, 2)]) / np.abs(D)
    return D, lam, A, T, float(np.max(canc))


def closed_form(sample):
    """sample [4,4] -> dict(model [3,3], valid, conditioning, cancellation)"""
    x = np.asarray(sample, np.float64).reshape(4, 4)
    bad = dict(model=identity(), valid=False, conditioning=0.0, cancellation=math.inf)
    if not np.isfinite(x).all():
        return bad
    D1, l1, A1, T1, c1 = _image(x[:, :2])
    D2, l2, A2, T2, c2 = _image(x[:, 2:])
    if D1[3] == 0.0 or D2[3] == 0.0:
        return bad
    # (the conditioning of the two basis solves is a property of the sample, whether or not the orientation test then keeps it)
    cond = float(min(np.abs(l1).min() / np.abs(l1).max(), np.abs(l2).min() / np.abs(l2).max()))
    canc = max(c1, c2)
    bad = dict(model=identity(), valid=False, conditioning=cond, cancellation=canc)
    if not (((D1 > 0) & (D2 > 0)) | ((D1 < 0) & (D2 < 0))).all():
        return bad
    with np.errstate(all="ignore"):
        H = canonical(np.linalg.inv(T2) @ A2 @ adjugate(A1) @ T1)
    if H is None:
        return bad
    return dict(model=H, valid=True, conditioning=cond, cancellation=canc)


def hartley(x):
    c = x.mean(0)
    s = math.sqrt(2.0) / np.linalg.norm(x - c, axis=1).mean()
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def dlt(matches, weights=None):
    """the normalised DLT by SVD -> dict(model, valid, sv = singular values of the weighted system); the weight of a point multiplies
    its two rows' terms in A^T A (its rows are scaled by sqrt(w))"""
    m = np.asarray(matches, np.float64).reshape(-1, 4)
    bad = dict(model=identity(), valid=False, sv=None)
    if len(m) < 4 or not np.isfinite(m).all():
        return bad
    w = np.ones(len(m)) if weights is None else np.asarray(weights, np.float64)
    T1, T2 = hartley(m[:, :2]), hartley(m[:, 2:])
    if not (np.isfinite(T1).all() and np.isfinite(T2).all()):
        return bad
    X = np.concatenate([m[:, :2], np.ones((len(m), 1))], 1) @ T1.T
    U = np.concatenate([m[:, 2:], np.ones((len(m), 1))], 1) @ T2.T
    Z = np.zeros_like(X)
    rw = np.sqrt(np.maximum(w, 0.0))[:, None]
    A = np.concatenate([np.concatenate([Z, -X, U[:, 1:2] * X], 1) * rw, np.concatenate([X, Z, -U[:, 0:1] * X], 1) * rw], 0)
    if not np.isfinite(A).all():
        return bad
    _, sv, Vt = np.linalg.svd(A, full_matrices=len(A) < 9)
    sv = np.concatenate([sv, np.zeros(9 - len(sv))])
    H = canonical(np.linalg.inv(T2) @ Vt[-1].reshape(3, 3) @ T1)
    if H is None:
        return bad
    return dict(model=H, valid=True, sv=sv)


def refit(matches, mask=None, weights=None):
    m = np.asarray(matches, np.float64)
    sel = np.ones(len(m), bool) if mask is None else np.asarray(mask, bool)
    return dlt(m[sel], None if weights is None else np.asarray(weights, np.float64)[sel])


def hypotheses(matches, idx, want_cancellation=False):
    """idx [B,4] -> (models [B,3,3], valid [B], conditioning [B]) (+ cancellation [B])"""
    out = [closed_form(matches[np.asarray(i)]) for i in np.asarray(idx)]
    res = (np.stack([o["model"] for o in out]), np.array([o["valid"] for o in out]), np.array([o["conditioning"] for o in out]))
    return res + (np.array([o["cancellation"] for o in out]),) if want_cancellation else res


# ---- residual, score, state ----------------------------------------------------------------------------------------------------------
def model_kind(H):
    """'scored', or 'nan' for a non-finite model or det == 0"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    if not np.isfinite(H).all():
        return "nan"
    d = np.linalg.det(H)
    return "scored" if (np.isfinite(d) and d != 0.0) else "nan"


def transfer(H, matches):
    """-> (d2 [N] with inf where a third coordinate is not positive or d2 is not finite, y [N,3], z [N,3]) under the det > 0 sign"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    if np.linalg.det(H) < 0:
        H = -H
    m = np.asarray(matches, np.float64)
    one = np.ones((len(m), 1))
    y = np.concatenate([m[:, :2], one], 1) @ H.T
    z = np.concatenate([m[:, 2:], one], 1) @ adjugate(H).T
    with np.errstate(all="ignore"):
        e = m[:, 2:] - y[:, :2] / y[:, 2:]
        f = m[:, :2] - z[:, :2] / z[:, 2:]
        d2 = (e * e).sum(1) + (f * f).sum(1)
    d2 = np.where((y[:, 2] > 0) & (z[:, 2] > 0) & np.isfinite(d2), d2, np.inf)
    return d2, y, z


def ratio2(H, matches, thr=THRESHOLD):
    return transfer(H, matches)[0] / (float(thr) * float(thr))


def msac(matches, H, thr=THRESHOLD):
    """-> (score, inliers, ratio2 [N]); NaN score for a model that scores NaN"""
    if model_kind(H) == "nan":
        return math.nan, 0, np.full(len(matches), np.inf)
    r = ratio2(H, matches, thr)
    return float(np.maximum(0.0, 1.0 - r[r < 1.0]).sum()), int((r < 1.0).sum()), r


def d2_bound(H, matches, dtype_name):
    """per point, a bound of |d2_kernel - d2_oracle| in the kernel's arithmetic for a model given in that type.  With X = (x, y, 1):
    a linear form sum_j c_j X_j from two fma carries eps sum |c_j X_j| (two roundings of half an ulp on partial sums no larger than
    that); an adjugate entry h h - h h carries eps (|h h| + |h h|), which the form inherits; t = num / den from a reciprocal (1 ulp)
    and a product: |t| (d num / |num| + d den / |den| + 3/2 eps); a residual component e = x - t one more half ulp of |e|... and
    d2 = sum e^2: 2 sum |e| d e + 2 eps d2.  Safety factor 2."""
    eps = eps_of(dtype_name)
    H = np.asarray(H, np.float64).reshape(3, 3)
    if np.linalg.det(H) < 0:
        H = -H
    m = np.asarray(matches, np.float64)
    one = np.ones((len(m), 1))
    X1, X2 = np.concatenate([m[:, :2], one], 1), np.concatenate([m[:, 2:], one], 1)
    Ad = adjugate(H)
    aH = np.abs(H)
    # |a b| + |c d| of every adjugate entry a b - c d (row r of adj(H) = the cross product of two columns of H)
    P = np.zeros((3, 3))
    cols = [(1, 2), (2, 0), (0, 1)]
    for r, (u, v) in enumerate(cols):
        for k in range(3):
            k1, k2 = (k + 1) % 3, (k + 2) % 3
            P[r, k] = aH[k1, u] * aH[k2, v] + aH[k2, u] * aH[k1, v]
    dAd = eps * P
    out = np.zeros(len(m))
    d2 = np.zeros(len(m))
    for (Mx, dM, Xa, tgt) in ((H, np.zeros((3, 3)), X1, m[:, 2:]), (Ad, dAd, X2, m[:, :2])):
        v = Xa @ Mx.T
        dv = eps * (np.abs(Xa) @ np.abs(Mx).T) + np.abs(Xa) @ dM.T
        with np.errstate(all="ignore"):
            for k in range(2):
                t = v[:, k] / v[:, 2]
                dt = np.abs(t) * (dv[:, k] / np.abs(v[:, k]) + dv[:, 2] / np.abs(v[:, 2]) + 1.5 * eps)
                dt = np.where(v[:, k] == 0, dv[:, k] / np.abs(v[:, 2]), dt)
                e = tgt[:, k] - t
                de = dt + 0.5 * eps * np.abs(e)
                out += 2.0 * np.abs(e) * de + de * de
                d2 += e * e
    return 2.0 * (out + 2.0 * eps * d2)


def score_tolerance(matches, H, thr, dtype_name):
    eps = eps_of(dtype_name)
    t2 = float(thr) * float(thr)
    r = ratio2(H, matches, thr)
    near = np.isfinite(r) & (r < 1.0 + BAND[dtype_name])
    if not near.any():
        return 0.0
    db = d2_bound(H, matches, dtype_name)
    depth = 8 + 6 + 4 + math.ceil(len(r) / 2048)
    score = float(np.maximum(0.0, 1.0 - r[near]).sum())
    # an inlier's term also carries the rounding of 1 / thr2 and of the fma: 3/2 eps
    return float((db[near] / t2).sum() + 1.5 * eps * near.sum() + 2.0 * depth * 0.5 * eps * max(score, 1.0))


def in_band(r, dtype_name):
    return np.abs(np.asarray(r) - 1.0) < BAND[dtype_name]


def model_tolerance(conditioning, dtype_name, cancellation=1.0):
    tol64 = 128.0 * eps_of("float64") * max(cancellation, 1.0) / conditioning
    return tol64 if dtype_name == "float64" else eps_of("float32") + tol64


def grad_tolerance(conditioning, dtype_name):
    tol64 = 256.0 * eps_of("float64") / (conditioning * conditioning)
    return tol64 if dtype_name == "float64" else eps_of("float32") + tol64


def refit_tolerance(sv, dtype_name):
    tol64 = 64.0 * eps_of("float64") * sv[0] ** 2 / (sv[7] ** 2 - sv[8] ** 2)
    return tol64 if dtype_name == "float64" else eps_of("float32") + tol64


def stop_rule(inliers, N, confidence=0.999, eps=1e-5, max_iterations=5000, sample_size=4):
    rk = (float(inliers) / float(N)) ** sample_size
    if 1.0 - rk >= 1.0 - eps:
        return float(max_iterations)
    return min(float(max_iterations), max(0.0, math.log10(1.0 - confidence) / math.log10(1.0 - rk + eps)))


def new_state(N, max_iterations):
    return dict(best_score=0.0, best_model=identity(), best_mask=np.zeros(N, dtype=bool), best_inliers=0, iters=0,
                max_iters=float(max_iterations), best_ratio2=np.full(N, np.inf))


def update(state, matches, models, valid, scores, thr, B, confidence=0.999, eps=1e-5, max_iterations=5000):
    """one state step, in place; -> the winner's index or None.  Strictly higher scores only."""
    if not state["iters"] < state["max_iters"]:
        return None
    scores = np.asarray(scores, np.float64)
    ok = ~np.isnan(scores)
    if valid is not None:
        ok &= np.asarray(valid, bool)
    win = None
    if ok.any():
        win = int(np.argmax(np.where(ok, scores, -np.inf)))      # numpy's argmax is the first maximum
        if scores[win] > state["best_score"]:
            r = ratio2(models[win], matches, thr) if model_kind(models[win]) == "scored" else np.full(len(matches), np.inf)
            state.update(best_score=float(scores[win]), best_model=np.array(models[win], np.float64).reshape(3, 3),
                         best_mask=r < 1.0, best_inliers=int((r < 1.0).sum()), best_ratio2=r)
            state["max_iters"] = stop_rule(state["best_inliers"], len(r), confidence, eps, max_iterations)
        else:
            win = None
    state["iters"] += B
    return win


def decision_margin(first, best, second, prev):
    """tests/registration_ref.py's: by how much the scores of a round may move before its outcome can change (here the first round
    has no special rule: prev = 0 from the start)"""
    if best > prev:
        return min(best - second, best - prev)
    return prev - best


def run(matches, idx_per_round, thr=THRESHOLD, confidence=0.999, eps=1e-5, max_iterations=5000, do_refit=True, dtype_name=None,
        hyp_per_round=None):
    """the whole loop for one pair; idx_per_round: list of [B,4] index sets.  dtype_name: round every model to that type before it is
    scored, as the kernels store it.  hyp_per_round (optional): (models, valid, conditioning) per round in place of hypotheses() --
    a caller that has checked a solver's output against hypotheses() can run the rest of the loop on exactly those models.  -> dict(model, mask, score, inliers, iterations, ratio2, rounds, gaps = decision_margin of
    every round, tols = the score tolerance of that round's best model, refit_gap, refit_tol, conditioning of the winner)"""
    N = len(matches)
    st = new_state(N, max_iterations)
    cast = (lambda M: M) if dtype_name is None else (lambda M: np.asarray(M, dtype_name).astype(np.float64))
    gaps, tols, win_cond, rounds = [], [], 1.0, 0
    for rnd, idx in enumerate(idx_per_round):
        if not st["iters"] < st["max_iters"]:
            break
        rounds += 1
        models, valid, conds = hypotheses(matches, idx) if hyp_per_round is None else hyp_per_round[rnd]
        models = cast(models)
        scores = np.array([msac(matches, M, thr)[0] if v else 0.0 for M, v in zip(models, valid)])
        ok = valid & ~np.isnan(scores)
        order = np.argsort(-scores[ok], kind="stable")
        top = scores[ok][order]
        if len(top):
            gaps.append(decision_margin(st["iters"] == 0, float(top[0]), float(top[1]) if len(top) > 1 else -math.inf,
                                        st["best_score"]))
            if dtype_name is not None:
                lead = np.flatnonzero(ok)[order[:2]]
                tols.append(max(score_tolerance(matches, models[j], thr, dtype_name) for j in lead))
        w = update(st, matches, models, valid, scores, thr, len(idx), confidence, eps, max_iterations)
        if w is not None:
            win_cond = float(conds[w])
    model, score, refit_gap, refit_tol, refit_sv = st["best_model"], st["best_score"], math.inf, 0.0, None
    refitted = False
    if do_refit:
        cand = refit(matches, st["best_mask"])
        if cand["valid"]:
            cm = cast(cand["model"])
            s = msac(matches, cm, thr)[0]
            refit_gap = abs(s - score)
            refit_sv = cand["sv"]
            if dtype_name is not None:
                refit_tol = score_tolerance(matches, cm, thr, dtype_name)
            if s > score:
                model, score, refitted = cm, s, True
    return dict(model=model, mask=st["best_mask"], score=score, inliers=st["best_inliers"], iterations=st["iters"],
                ratio2=st["best_ratio2"], rounds=rounds, gaps=gaps, tols=tols, refit_gap=refit_gap, refit_tol=refit_tol,
                refit_sv=refit_sv, refitted=refitted, conditioning=win_cond)


def mean_transfer_error(H, matches, sel):
    """mean sqrt(d2) over the rows `sel` picks"""
    d2 = transfer(H, np.asarray(matches, np.float64)[sel])[0]
    return float(np.sqrt(d2).mean())


def caps(matches_list, idx_list, models_list, thr, dtype_name):
    """the two conditions a GPU case must meet on the oracle's side: -> (share of well-conditioned samples among the valid-or-not
    P B samples, share of (model, point) cells inside the guard band)"""
    well = total = cells = inband = 0
    for m, idx, models in zip(matches_list, idx_list, models_list):
        mo, va, co = hypotheses(m, idx) if models is None else models
        well += int((co > WELL).sum())
        total += len(co)
        for M, v in zip(mo, va):
            if v:
                r = ratio2(M, m, thr)
                cells += len(r)
                inband += int(in_band(r, dtype_name).sum())
    return well / max(total, 1), inband / max(cells, 1)


# ---- the closed form restated in torch (f64 autograd reference of dr_homography4_bwd) --------------------------------------------------
def closed_form_torch(samples):
    """samples [..., 4, 4] (f64 torch) -> H [..., 3, 3] unit norm, det > 0; differentiable; no validity test"""
    import torch

    def image(x):
        c = x.mean(-2, keepdim=True)
        q = x - c
        s = math.sqrt(2.0) / q.norm(dim=-1).mean(-1)

        def tri(i, j, k):
            return (q[..., i, 0] * (q[..., j, 1] - q[..., k, 1]) - q[..., j, 0] * (q[..., i, 1] - q[..., k, 1])
                    + q[..., k, 0] * (q[..., i, 1] - q[..., j, 1]))
        D3 = tri(0, 1, 2)
        lam = torch.stack([tri(3, 1, 2), tri(0, 3, 2), tri(0, 1, 3)], -1) / D3[..., None]
        A = torch.stack([lam * s[..., None] * q[..., :3, 0], lam * s[..., None] * q[..., :3, 1], lam], -2)
        T = torch.zeros(x.shape[:-2] + (3, 3), dtype=x.dtype, device=x.device)
        T[..., 0, 0] = s
        T[..., 1, 1] = s
        T[..., 0, 2] = -s * c[..., 0, 0]
        T[..., 1, 2] = -s * c[..., 0, 1]
        T[..., 2, 2] = 1.0
        return A, T
    A1, T1 = image(samples[..., :2])
    A2, T2 = image(samples[..., 2:])
    adj = torch.stack([torch.linalg.cross(A1[..., :, 1], A1[..., :, 2]), torch.linalg.cross(A1[..., :, 2], A1[..., :, 0]),
                       torch.linalg.cross(A1[..., :, 0], A1[..., :, 1])], -2)
    H = torch.linalg.solve(T2, A2 @ adj @ T1)
    H = H / H.flatten(-2).norm(dim=-1)[..., None, None]
    return H * torch.sign(torch.linalg.det(H))[..., None, None]


# ---- the explicit-index cases of tests/test_gpu_homography.py (and, for the caps, of tests/test_homography_host.py) ---------------------
# (P, N, B = M, inlier share, seed): P in {1, 3}; N = 4 (one possible sample), 7, 300, 2049 (one point past a 2048-point chunk and
# past the 256-thread stride); B = M in {1, 33, 64} around the 64-sample solver block and the 16-slot score tile
GPU_CASES = [(1, 4, 1, 1.0, 3), (3, 7, 33, 1.0, 11), (3, 300, 64, 0.6, 21), (1, 2049, 33, 0.5, 31), (1, 300, 1, 0.6, 41)]


def gpu_case(P, N, B, share, seed, dtype_name="float64"):
    """-> dict(matches [P,N,4] (values of `dtype_name`, held as f64), idx [P,B,4] int32, inlier [P,N]): every other sample is drawn
    from the inliers alone, so that a case scores real models too"""
    rng = np.random.default_rng(1000 + seed)
    ms, ii, inl = [], [], []
    for p in range(P):
        sc = scene(seed * 16 + p, N, share)
        ins = np.flatnonzero(sc["inlier"])
        idx = np.stack([rng.choice(ins if (b % 2 == 0 and len(ins) >= 4) else N, 4, replace=False) for b in range(B)])
        ms.append(np.asarray(sc["matches"], dtype_name).astype(np.float64))
        ii.append(idx.astype(np.int32))
        inl.append(sc["inlier"])
    return dict(matches=np.stack(ms), idx=np.stack(ii), inlier=np.stack(inl))
