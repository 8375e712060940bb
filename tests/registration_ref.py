"""f64 numpy oracle of the robust 3-D registration path (csrc/registration.hip, ransac.BatchedRegistration), written from the
maths of the four kernels and not from their code, and the scene generator its tests share.

Conventions: matches [N,6] = (p, q); a model is the 4x4 [[R, t], [0, 0, 0, 1]]; the prediction is q_hat = R p + t and
d2 = |q - q_hat|^2.  `threshold` is a DISTANCE: a point is an inlier iff d2 < threshold^2.  The MSAC score of a model is
sum_n max(0, 1 - d2_n / threshold^2).

  kabsch   c0, c1 = (weighted) means; H = sum w (p - c0)(q - c1)^T = U S V^T (numpy.linalg.svd);
           R = V diag(1, 1, det(V U^T)) U^T, polished in extended precision (_polish_rotation); t = c1 - R c0; degenerate when
           sigma_2 <= 1e-12 sigma_1 or anything is non-finite.
  msac     score, inlier count, d2 / threshold^2 per point.
  update   the state step: first arg-max over valid, non-NaN scores; taken when score > best_score or iters == 0; mask, inlier count
           and stop bound of the winner; iters += B.
  refit    kabsch over the rows a mask selects (with optional row weights), at least three rows.
  run      the whole loop on given index sets, with the final refit."""
import math

import numpy as np

THRESHOLD = 0.05
BAND = {"float32": 1e-3, "float64": 1e-9}      # |d2 / threshold^2 - 1| inside which a kernel's inlier decision may differ


def eps_of(dtype_name):
    return float(np.finfo(dtype_name).eps)


def random_rotation(rng):
    Q, Rr = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = Q * np.sign(np.diag(Rr))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


def scene(seed, N, inlier_share, noise=0.005, outlier_side=4.0):
    """a random rotation, a translation of norm 1-2, p uniform in the unit cube; the first round(share N) rows (then shuffled) are
    q = R p + t + N(0, noise^2), the others uniform in a cube of side `outlier_side` centred on the inliers' cube.
    -> dict(matches [N,6], R, t, inlier [N] bool)"""
    rng = np.random.default_rng(seed)
    R = random_rotation(rng)
    t = rng.standard_normal(3)
    t *= rng.uniform(1.0, 2.0) / np.linalg.norm(t)
    p = rng.uniform(0.0, 1.0, (N, 3))
    q = p @ R.T + t
    n_in = int(round(inlier_share * N))
    inlier = np.zeros(N, dtype=bool)
    inlier[rng.permutation(N)[:n_in]] = True
    centre = np.full(3, 0.5) @ R.T + t
    out = centre + rng.uniform(-0.5 * outlier_side, 0.5 * outlier_side, (N, 3))
    q = np.where(inlier[:, None], q + noise * rng.standard_normal((N, 3)), out)
    return dict(matches=np.concatenate([p, q], 1), R=R, t=t, inlier=inlier)


def _nearest_rotation(A):
    """the rotation nearest to an almost orthogonal A"""
    U, _, Vt = np.linalg.svd(A)
    return U @ Vt


def boundary_scene(seed, N, M, thr=THRESHOLD):
    """every row q = R p + t + e with |e| uniform in [0, 2 thr], so that many points sit near the inlier decision of a model close
    to the pose; M such models: the pose times a rotation by N(0, (thr / 4)^2) rad per axis, plus N(0, (thr / 4)^2) per
    translation entry.  -> (matches [N,6], models [M,4,4])"""
    rng = np.random.default_rng(seed)
    R, t = random_rotation(rng), rng.standard_normal(3)
    p = rng.uniform(0.0, 1.0, (N, 3))
    e = rng.standard_normal((N, 3))
    e *= rng.uniform(0.0, 2.0 * thr, (N, 1)) / np.linalg.norm(e, axis=1, keepdims=True)
    models = np.tile(np.eye(4), (M, 1, 1))
    for j in range(M):
        W = _cross_matrix(0.25 * thr * rng.standard_normal(3)).astype(np.float64)
        models[j, :3, :3] = _nearest_rotation(np.eye(3) + W + 0.5 * W @ W) @ R
        models[j, :3, 3] = t + 0.25 * thr * rng.standard_normal(3)
    return np.concatenate([p, p @ R.T + t + e], 1), models


def best_gap(values, largest):
    """relative gap between the best and the second-best of `values` (inf for a single value): a reduction-order rounding, far
    below it, cannot change the winner"""
    v = np.sort(np.asarray(values, np.float64))
    if len(v) < 2:
        return math.inf
    a, b = (v[-1], v[-2]) if largest else (v[0], v[1])
    return abs(a - b) / abs(a)


LD = np.longdouble


def _cross_matrix(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=LD)


def _polish_rotation(R0, H):
    """LAPACK's U and V are orthogonal to some ten eps each, and V D U^T inherits that: measured against a 40-digit SVD the plain
    product is off by up to 18 eps sigma_1 / sigma_2 -- more than the 16 the kernels are allowed.  The optimum is characterised by
    R H = V D S V^T being symmetric; starting from the SVD's rotation (which fixes the branch, reflection included), Newton steps in
    extended precision solve for the small rotation exp([w]x) that removes the skew part of R H.  -> R in longdouble"""
    R = R0.astype(LD)
    for _ in range(3):
        # re-orthonormalise (first order is enough: R0 is orthogonal to 1e-15), then the Newton step
        R = (LD(1.5) * np.eye(3, dtype=LD) - LD(0.5) * (R @ R.T)) @ R
        A = R @ H
        K = A - A.T
        rhs = -np.array([K[2, 1], K[0, 2], K[1, 0]], dtype=LD)
        L = np.zeros((3, 3), dtype=LD)
        for k in range(3):
            W = _cross_matrix(np.eye(3, dtype=LD)[k])
            F = W @ A + A.T @ W
            L[:, k] = [F[2, 1], F[0, 2], F[1, 0]]
        w = np.linalg.solve(L.astype(np.float64), rhs.astype(np.float64)).astype(LD)   # (a correction of 1e-15: f64 solve is plenty)
        W = _cross_matrix(w)
        R = (np.eye(3, dtype=LD) + W + LD(0.5) * (W @ W)) @ R
    return (LD(1.5) * np.eye(3, dtype=LD) - LD(0.5) * (R @ R.T)) @ R


def identity():
    return np.eye(4)


def kabsch(p, q, w=None):
    """p, q [n,3], w [n] or None -> dict(model [4,4], valid, ratio = sigma_2 / sigma_1, flipped = det(V U^T) < 0)"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    w = np.ones(len(p)) if w is None else np.asarray(w, np.float64)
    bad = dict(model=identity(), valid=False, ratio=0.0, flipped=False)
    if len(p) < 3 or not (np.isfinite(p).all() and np.isfinite(q).all() and np.isfinite(w).all()) or not w.sum() > 0:
        return bad
    # means and H in extended precision (numpy.longdouble: 64-bit mantissa on x86), so that the oracle's own error is the SVD's
    pl, ql, wl = p.astype(LD), q.astype(LD), w.astype(LD)
    c0 = (wl[:, None] * pl).sum(0) / wl.sum()
    c1 = (wl[:, None] * ql).sum(0) / wl.sum()
    Hl = ((wl[:, None] * (pl - c0))[:, :, None] * (ql - c1)[:, None, :]).sum(0)
    H = Hl.astype(np.float64)
    if not np.isfinite(H).all():
        return bad
    U, S, Vt = np.linalg.svd(H)
    if not S[1] > 1e-12 * S[0]:
        return bad
    V = Vt.T
    d = np.linalg.det(V @ U.T)
    R = _polish_rotation(V @ np.diag([1.0, 1.0, 1.0 if d > 0 else -1.0]) @ U.T, Hl)
    M = identity()
    M[:3, :3] = R.astype(np.float64)
    M[:3, 3] = (c1 - R @ c0).astype(np.float64)
    return dict(model=M, valid=True, ratio=float(S[1] / S[0]), flipped=bool(d < 0))


def ratio2(model, matches, thr):
    """d2 / threshold^2 per point, f64"""
    m = np.asarray(matches, np.float64)
    M = np.asarray(model, np.float64).reshape(4, 4)
    e = m[:, 3:] - (m[:, :3] @ M[:3, :3].T + M[:3, 3])
    return (e * e).sum(1) / (float(thr) * float(thr))


def msac(matches, model, thr):
    """-> (score, inliers, ratio2 [N])"""
    r = ratio2(model, matches, thr)
    return float(np.maximum(0.0, 1.0 - r).sum()), int((r < 1.0).sum()), r


def score_tolerance(matches, model, thr, dtype_name):
    """16 eps N max_n(|q_hat| + |q|)^2 / threshold^2: about ten roundings per term, every term continuous at the threshold"""
    m = np.asarray(matches, np.float64)
    M = np.asarray(model, np.float64).reshape(4, 4)
    qh = m[:, :3] @ M[:3, :3].T + M[:3, 3]
    mag = (np.linalg.norm(qh, axis=1) + np.linalg.norm(m[:, 3:], axis=1)).max()
    return 16.0 * eps_of(dtype_name) * len(m) * mag * mag / (float(thr) * float(thr))


def stop_rule(inliers, N, confidence=0.999, eps=1e-5, max_iterations=5000, sample_size=3):
    """min(max_iterations, log(1 - confidence) / log(1 - ratio^3 + eps)), max_iterations when 1 - ratio^3 >= 1 - eps"""
    rk = (float(inliers) / float(N)) ** sample_size
    if 1.0 - rk >= 1.0 - eps:
        return float(max_iterations)
    return min(float(max_iterations), max(0.0, math.log10(1.0 - confidence) / math.log10(1.0 - rk + eps)))


def new_state(N, max_iterations):
    return dict(best_score=0.0, best_model=identity(), best_mask=np.zeros(N, dtype=bool), best_inliers=0, iters=0,
                max_iters=float(max_iterations), best_ratio2=np.full(N, np.inf))


def update(state, matches, models, valid, scores, thr, B, confidence=0.999, eps=1e-5, max_iterations=5000):
    """one state step, in place; -> the winner's index or None"""
    if not state["iters"] < state["max_iters"]:
        return None
    scores = np.asarray(scores, np.float64)
    ok = ~np.isnan(scores)
    if valid is not None:
        ok &= np.asarray(valid, bool)
    win = None
    if ok.any():
        win = int(np.argmax(np.where(ok, scores, -np.inf)))      # numpy's argmax is the first maximum
        if scores[win] > state["best_score"] or state["iters"] == 0:
            r = ratio2(models[win], matches, thr)
            state.update(best_score=float(scores[win]), best_model=np.array(models[win], np.float64).reshape(4, 4),
                         best_mask=r < 1.0, best_inliers=int((r < 1.0).sum()), best_ratio2=r)
            state["max_iters"] = stop_rule(state["best_inliers"], len(r), confidence, eps, max_iterations)
        else:
            win = None
    state["iters"] += B
    return win


def refit(matches, mask=None, weights=None):
    m = np.asarray(matches, np.float64)
    sel = np.ones(len(m), bool) if mask is None else np.asarray(mask, bool)
    w = None if weights is None else np.asarray(weights, np.float64)[sel]
    return kabsch(m[sel, :3], m[sel, 3:], w)


def hypotheses(matches, idx):
    """idx [B,k] -> (models [B,4,4], valid [B], ratio [B])"""
    out = [kabsch(matches[i, :3], matches[i, 3:]) for i in np.asarray(idx)]
    return (np.stack([o["model"] for o in out]), np.array([o["valid"] for o in out]), np.array([o["ratio"] for o in out]))


def decision_margin(first, best, second, prev):
    """By how much the scores of a round may move before its outcome can change.  A round that can replace the state (the first
    round always does; a later one when its best score beats the state's `prev`) must single out its winner: margin = min(best -
    second, best - prev).  A round whose best score stays below the state's changes nothing whichever model wins its arg-max -- in
    a pair with few inliers most rounds are of this kind, many with every score exactly 0 -- and its margin is prev - best."""
    if first:
        return best - second
    if best > prev:
        return min(best - second, best - prev)
    return prev - best


def run(matches, idx_per_round, thr=THRESHOLD, confidence=0.999, eps=1e-5, max_iterations=5000, do_refit=True):
    """the whole loop for one pair; idx_per_round: list of [B,k] index sets.  -> dict(model, mask, score, inliers, iterations,
    ratio2 = the RANSAC winner's d2 / thr^2 per point, rounds = rounds run, gaps = decision_margin of every round run, refit_gap = |refit score - RANSAC score| (inf without a valid refit), model_ratio = sigma_2 /
    sigma_1 of the fit the returned model came from)"""
    N = len(matches)
    st = new_state(N, max_iterations)
    gaps, win_ratio, rounds = [], 1.0, 0
    for idx in idx_per_round:
        if not st["iters"] < st["max_iters"]:
            break
        rounds += 1
        models, valid, ratios = hypotheses(matches, idx)
        scores = np.array([msac(matches, M, thr)[0] if v else -1.0 for M, v in zip(models, valid)])
        top = np.sort(scores[valid])[::-1]
        if len(top):
            gaps.append(decision_margin(st["iters"] == 0, float(top[0]), float(top[1]) if len(top) > 1 else -math.inf,
                                        st["best_score"]))
        w = update(st, matches, models, valid, scores, thr, len(idx), confidence, eps, max_iterations)
        if w is not None:
            win_ratio = float(ratios[w])
    model, score, refit_gap = st["best_model"], st["best_score"], math.inf
    if do_refit:
        cand = refit(matches, st["best_mask"])
        if cand["valid"]:
            s = msac(matches, cand["model"], thr)[0]
            refit_gap = abs(s - score)
            if s > score:
                model, score, win_ratio = cand["model"], s, cand["ratio"]
    return dict(model=model, mask=st["best_mask"], score=score, inliers=st["best_inliers"], iterations=st["iters"],
                ratio2=st["best_ratio2"], rounds=rounds, gaps=gaps, refit_gap=refit_gap, model_ratio=win_ratio)


def rotation_error_deg(R, R_true):
    c = (np.trace(np.asarray(R, np.float64)[:3, :3].T @ R_true) - 1.0) / 2.0
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))


def model_error(M, Mo):
    """(|dR|_inf entrywise, |dt| / max(1, |t|_inf))"""
    M, Mo = np.asarray(M, np.float64).reshape(4, 4), np.asarray(Mo, np.float64).reshape(4, 4)
    dR = np.abs(M[:3, :3] - Mo[:3, :3]).max()
    dt = np.abs(M[:3, 3] - Mo[:3, 3]).max() / max(1.0, np.abs(Mo[:3, 3]).max())
    return float(dR), float(dt)
