"""f64 host restatement of the kernels that end every test-mode call: the update step of dr_ransac_update (ransac.py:109-144
with the deviations include/dransac.h documents: first arg-max over valid, non-NaN scores, and the sub-batch walk),
dr_select_best and the acceptance rule of dr_refit_accept (ransac.py:173-185).  It is the arbiter of
tests/test_gpu_selection.py, as lo_ref.py is of the local optimisation.

The Sampson ratio q = d^2 / (1.5 thr)^2 is computed in f64; a point is an inlier when q < 1.  A kernel computes d^2 in its own
precision, so `sampson` also returns, per point, a relative bound `rel` on the error of the kernel's q (derived below): a point
whose q lies within that margin of 1 may fall on either side, and only those points are exempt from the mask comparisons."""
import math

import torch

from oracle import cpu_ref as O


def sampson(matches, model, thr, dt):
    """matches [N,4], model [3,3] (any dtype), thr: the pair's threshold as the kernel holds it (dt) -> (q [N] f64, rel [N] f64).

    The kernel forms a = M^T x2, b = M x1 (x homogeneous, nested FMAs), r = x1 . a, jj = a0^2 + a1^2 + b0^2 + b1^2,
    d^2 = r^2 * rcp(jj), s = fma(d^2, 1/(1.5 thr)^2, -1).  Each of a, b, r is a short dot product: its rounding error is at most
    a few ulp of the sum of the magnitudes of its terms, so |dr| / |r| <= 5 u rabs / |r| with rabs = |x1|.(|M|^T |x2|), and
    jj, a sum of squares of such dot products, has |djj| / jj <= 6 u jabs / jj (jabs: the same sum over |M|, |x|).  With the
    reciprocal, the threshold's three roundings and the final FMA: |dq| / q <= u (10 rabs / |r| + 6 jabs / jj + 8).  `rel`
    is twice that (u = unit roundoff of dt); a zero residual (rabs / 0) or jj = 0 gives an infinite margin."""
    x = matches.double()
    M = model.double().reshape(3, 3)
    one = torch.ones_like(x[:, 0])
    x1 = torch.stack([x[:, 0], x[:, 1], one], -1)
    x2 = torch.stack([x[:, 2], x[:, 3], one], -1)
    a = x2 @ M                      # a_j = sum_i x2_i M_ij  (M^T x2)
    b = x1 @ M.T                    # b_i = sum_j M_ij x1_j  (M x1)
    r = (x1 * a).sum(-1)
    jj = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
    Ma = M.abs()
    aa = x2.abs() @ Ma
    ba = x1.abs() @ Ma.T
    rabs = (x1.abs() * aa).sum(-1)
    jabs = aa[:, 0] ** 2 + aa[:, 1] ** 2 + ba[:, 0] ** 2 + ba[:, 1] ** 2
    t = float(torch.tensor(1.5, dtype=dt) * torch.tensor(float(thr), dtype=dt))
    q = (r * r / jj) / (t * t)
    u = torch.finfo(dt).eps / 2
    rel = 2 * u * (10 * rabs / r.abs() + 6 * jabs / jj + 8)
    rel = torch.where(torch.isnan(rel), torch.full_like(rel, math.inf), rel)
    return q, rel


def mask64(q):
    return q < 1.0                  # (NaN: no inlier)


def sure(q, rel):
    """points whose side of the threshold no rounding of the kernel can change"""
    return (q - 1.0).abs() > rel * q.abs().clamp_min(1.0)


def msac64(q, rel, dt, n_terms):
    """MSAC score sum(max(0, 1 - q)) in f64 and the bound on the kernel's error.

    Per point the kernel's term has error <= q rel (the margin above; a point that flips lies within it of 1, so its term is
    at most q rel too).  The kernel then sums its terms in dt: a thread ceil(N / 256) of them in order, a 64-lane tree (6
    levels) and four wave partials, so the summation adds at most (ceil(N / 256) + 10) u sum(terms).  The returned bound is
    twice the sum of both parts, plus a few ulp of the result."""
    u = torch.finfo(dt).eps / 2
    ok = ~torch.isnan(q)
    term = torch.where(ok & (q < 1), 1.0 - q, torch.zeros_like(q))
    near = ok & (q < 1.0 + rel * q.abs().clamp_min(1.0))
    per_point = torch.where(near, q.abs() * torch.where(torch.isinf(rel), torch.ones_like(rel), rel) + u, torch.zeros_like(q))
    s = float(term.sum())
    tol = 2 * (float(per_point.sum()) + (math.ceil(n_terms / 256) + 10) * u * s) + 8 * u * max(1.0, s)
    return s, tol


def first_argmax(scores, valid=None):
    """first index of the maximum over the valid, non-NaN entries of scores [M] -> (index, value) or (-1, None)"""
    s = scores.double()
    ok = ~torch.isnan(s)
    if valid is not None:
        ok &= valid.bool()
    if not bool(ok.any()):
        return -1, None
    best = float(s[ok].max())
    idx = int(torch.nonzero(ok & (s == best))[0, 0])
    return idx, scores[idx]


def bound(inliers, N, k, confidence, eps, max_iterations):
    """max_iters after a replacement: min(max_iterations, adaptive_iteration_number) (ransac.py:135-142), via math"""
    return min(float(max_iterations), float(O.adaptive_iteration_number(inliers, N, k, confidence, eps, max_iterations)))


def update(scores, valid, it, max_it, best, B, k, confidence, eps, max_iterations, sub_models, inliers_of, N):
    """The update step on one pair.  scores [M] (dt), valid [M] bool or None; (it, max_it) the counters before the call;
    best: the best score before the call (dt scalar).  inliers_of(m) -> inlier count of slot m's model.

    Walks the ceil(M / msub) sub-batches in order (msub = sub_models if 0 < sub_models < M, else M: one batch); before each,
    the loop's stop test it >= max_it.  A sub-batch's first arg-max over valid, non-NaN scores replaces the best when it is
    greater than the best or it == 0; then max_it = bound(...).  Every walked sub-batch adds B.
    Returns dict(it, max_it, winner (slot of the last replacement or -1), score, ambiguous, walked): `ambiguous` marks a stop
    test whose computed bound lies within 1e-9 (relative) of the iteration count, where f64 rounding may decide."""
    M = scores.shape[0]
    msub = sub_models if 0 < sub_models < M else M
    R = -(-M // msub)
    winner, bs, ambiguous, walked = -1, best, False, 0
    computed = False
    for j in range(R):
        if computed and abs(it - max_it) <= 1e-9 * max(1.0, max_it):
            ambiguous = True
        if it >= max_it:
            break
        lo, hi = j * msub, min(M, (j + 1) * msub)
        i, v = first_argmax(scores[lo:hi], None if valid is None else valid[lo:hi])
        if i >= 0 and (float(v) > float(bs) or it == 0):
            winner, bs = lo + i, v
            max_it = bound(inliers_of(lo + i), N, k, confidence, eps, max_iterations)
            computed = True
        it += B
        walked += 1
    return dict(it=it, max_it=max_it, winner=winner, score=bs, ambiguous=ambiguous, walked=walked)


def sub_batch_argmax(scores, valid, sub_models):
    """first arg-max of every sub-batch (slot index, -1 for none): the only slots the walk can take"""
    M = scores.shape[0]
    msub = sub_models if 0 < sub_models < M else M
    out = []
    for lo in range(0, M, msub):
        i, _ = first_argmax(scores[lo:lo + msub], None if valid is None else valid[lo:lo + msub])
        out.append(lo + i if i >= 0 else -1)
    return out


def refit_accept(cand_scores, cand_ok, best):
    """the acceptance of ransac.py:173-185 on one pair: first arg-max over the valid, finite candidates, kept only when it is
    STRICTLY greater than the best.  cand_scores: the candidates' scores as the kernel computes them.  -> index or -1"""
    idx, top = -1, None
    for c, (s, ok) in enumerate(zip(cand_scores, cand_ok)):
        if ok and (top is None or s > top):
            idx, top = c, s
    return idx if idx >= 0 and top > best else -1
