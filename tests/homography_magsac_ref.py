"""f64 numpy oracle of the MAGSAC++ scoring and IRLS polish of the homography path (dr_homography_magsac_score, dr_homography_irls,
ransac.BatchedHomography(scoring="magsac")), written from the maths and not from the kernels' code.  Scenes, the transfer error, the
normalised DLT (plain and weighted), the state step and the stop rule are tests/homography_ref.py's; the weight, the loss and their
constants are tests/magsac_ref.py's 4-degrees-of-freedom forms (torch.special.gammainc / gammaincc: the definitions, not the closed
form the kernels evaluate), since the symmetric transfer error is a 4-vector like the residual behind the Sampson distance.

`threshold` is the cutoff DISTANCE, read as k sigma_max with k^2 = chi2.ppf(0.99, 4); s = d2 / threshold^2:

  score   = sum_n (1 - l(s_n)) over the points with s_n < 1 in front of both cameras; inliers = their number; a model that
            homography_ref.model_kind calls 'nan' scores NaN with 0 inliers
  irls    from (model, score), up to `iters` times: rows = the points with s_n < 1 under the current model, each with the weight w(s_n);
            homography_ref.refit(m, mask=rows, weights=w) (Hartley's transforms unweighted over the rows, the weight in the Gram sums);
            the candidate rounded to the kernel's type; its score over all points; taken only on a STRICTLY higher score.  Ends before a
            fit when the current model scores NaN or has fewer than four rows, on an invalid or non-finite candidate (or one that scores
            NaN), on a candidate that does not win, and at the step limit.

Tolerance of a score (score_tolerance), three parts, none of them tuned:
  L x sum_n d2_bound_n / thr2   over the points at or inside the band's outer edge (s_n < 1 + BAND): the error of d2 in the kernel's
                  arithmetic (homography_ref.d2_bound, safety factor 2 included) through the Lipschitz constant L of 1 - l in s
                  (magsac_ref.L = u_k (Gamma_0 - Gamma_k) / rho_1, attained at s = 0).  The term is continuous across the cutoff
                  (l(1) = 1: 1 - l ends at 0, what a point outside adds), so s -> the term is Lipschitz with L on the whole line and a
                  point that the kernel and the oracle put on different sides of the cutoff is covered by its own d2_bound: only the
                  inlier COUNT of such a cell can differ, and the GPU tests leave cells with a point in the band out of that comparison.
  depth eps max(score, 1)       the reduction: homography_ref.score_tolerance's depth = 8 (a lane's points) + 6 (the wave tree) + chunks + 4
                  (waves) additions of partial sums <= score, half an ulp each, safety factor 2.
  N x e_term(dtype)             the evaluation of 1 - l at an exact s by the closed form of csrc/magsac_device.hpp, from the ulp bounds of
                  the device library's sqrt, exp and erfc: magsac_ref.e_term, derived there (14 / 16 unit roundoffs per term).
Tolerance of the model of a polish step: homography_ref.refit_tolerance(sv, dtype) with the oracle's singular values of the weighted
system.  The kernel evaluates the row decision and the weights of a step in f64 for either type, from the model and the rows as stored,
so the weights carry no f32 error; what remains is the f64 rounding of d2 (relative 1e-13 at most, far below the refit tolerance) and a
row whose s lies in the f64 band, which the GPU tests exclude by a condition on the oracle's side."""
import math

import numpy as np
import torch

from tests import homography_ref as R
from tests import magsac_ref as M4

L = M4.L
K2, UK = M4.K2, M4.UK
_TORCH = {"float32": torch.float32, "float64": torch.float64}


def weight(s):
    return M4.weight(torch.as_tensor(np.asarray(s, np.float64))).numpy()


def loss(s):
    return M4.loss(torch.as_tensor(np.asarray(s, np.float64))).numpy()


def e_term(dtype_name):
    return M4.e_term(_TORCH[dtype_name])


def magsac(matches, H, thr=R.THRESHOLD):
    """-> (score, inliers); NaN score, 0 inliers for a model that scores NaN"""
    if R.model_kind(H) == "nan":
        return math.nan, 0
    r = R.ratio2(H, matches, thr)
    live = np.isfinite(r) & (r < 1.0)
    return float((1.0 - loss(r[live])).sum()), int(live.sum())


def score_tolerance(matches, H, thr, dtype_name):
    eps = R.eps_of(dtype_name)
    t2 = float(thr) * float(thr)
    r = R.ratio2(H, matches, thr)
    n = len(r)
    near = np.isfinite(r) & (r < 1.0 + R.BAND[dtype_name])
    depth = 8 + 6 + 4 + math.ceil(n / 2048)
    slack, score = 0.0, 0.0
    if near.any():
        slack = float((R.d2_bound(H, matches, dtype_name)[near] / t2).sum())
        score = float((1.0 - loss(r[near & (r < 1.0)])).sum())
    return L * slack + 2.0 * depth * 0.5 * eps * max(score, 1.0) + n * e_term(dtype_name)


def rounded(a, dtype_name):
    """the values a kernel of that type stores, as f64"""
    return a if dtype_name is None else np.asarray(a, dtype_name).astype(np.float64)


def irls(matches, model, thr, iters, score=None, trace=None, dtype_name=None):
    """-> (model, score, fits, margins): margins[i] = candidate score - current score of fit i (only for fits whose candidate was
    scored).  trace (a list, optional) receives a dict per fit run: homography_ref.dlt's (model, valid, sv) + rows = the row mask,
    ratio2 = s of every point under the model the fit started from, cand = the rounded candidate (None when the fit is not valid)"""
    m = np.asarray(matches, np.float64)
    model = np.array(model, np.float64).reshape(3, 3)
    score = magsac(m, model, thr)[0] if score is None else float(score)
    fits, margins = 0, []
    for _ in range(iters):
        if R.model_kind(model) == "nan":
            break
        r = R.ratio2(model, m, thr)
        rows = np.isfinite(r) & (r < 1.0)
        if rows.sum() < 4:
            break
        w = np.zeros(len(m))
        w[rows] = weight(r[rows])
        fit = dict(R.refit(m, mask=rows, weights=w), rows=rows, ratio2=r, cand=None)
        fits += 1
        if trace is not None:
            trace.append(fit)
        if not fit["valid"]:
            break
        cand = rounded(fit["model"], dtype_name)
        if not np.isfinite(cand).all() or R.model_kind(cand) == "nan":
            break
        fit["cand"] = cand
        s = magsac(m, cand, thr)[0]
        margins.append(s - score)
        if not s > score:
            break
        model, score = cand, s
    return model, score, fits, margins


def run(matches, idx_per_round, thr=R.THRESHOLD, confidence=0.999, eps=1e-5, max_iterations=5000, do_refit=True, irls_iters=10,
        dtype_name=None, hyp_per_round=None):
    """homography_ref.run with this score and this polish (its arguments; hyp_per_round = (models, valid, conditioning) per round in
    place of homography_ref.hypotheses).  -> dict(model, mask, score, inliers, iterations, ratio2, rounds, gaps = decision_margin of
    every round run, tols = the score tolerance of that round's two leading models, irls_fits, irls_margins, irls_trace)"""
    N = len(matches)
    st = R.new_state(N, max_iterations)
    gaps, tols, rounds = [], [], 0
    for rnd, idx in enumerate(idx_per_round):
        if not st["iters"] < st["max_iters"]:
            break
        rounds += 1
        models, valid, _ = R.hypotheses(matches, idx) if hyp_per_round is None else hyp_per_round[rnd]
        models = rounded(models, dtype_name)
        scores = np.array([magsac(matches, M, thr)[0] if v else 0.0 for M, v in zip(models, valid)])
        ok = np.asarray(valid, bool) & ~np.isnan(scores)
        order = np.argsort(-scores[ok], kind="stable")
        top = scores[ok][order]
        if len(top):
            gaps.append(R.decision_margin(st["iters"] == 0, float(top[0]), float(top[1]) if len(top) > 1 else -math.inf,
                                          st["best_score"]))
            if dtype_name is not None:
                lead = np.flatnonzero(ok)[order[:2]]
                tols.append(max(score_tolerance(matches, models[j], thr, dtype_name) for j in lead))
        R.update(st, matches, models, valid, scores, thr, len(idx), confidence, eps, max_iterations)
    model, score, fits, margins, trace = st["best_model"], st["best_score"], 0, [], []
    if do_refit and irls_iters > 0:
        model, score, fits, margins = irls(matches, model, thr, irls_iters, score, trace, dtype_name)
    return dict(model=model, mask=st["best_mask"], score=score, inliers=st["best_inliers"], iterations=st["iters"],
                ratio2=st["best_ratio2"], rounds=rounds, gaps=gaps, tols=tols, irls_fits=fits, irls_margins=margins, irls_trace=trace)


# ---- the inputs of tests/test_gpu_homography_magsac.py, made here so that tests/test_homography_magsac_host.py can hold the oracle
# alone to the conditions those tests rest on ------------------------------------------------------------------------------------------
SCORE_N, SCORE_M = (4, 257, 2049), (1, 17, 33)
SCORE_P = 2


def score_case(N, M, dtype_name):
    """-> (matches [P,N,4], models [P,M,3,3], valid [P,M]): homography_ref.gpu_case scenes (60 % inliers; N = 4: inliers alone) and
    the closed-form hypotheses of their index sets, values of `dtype_name` held as f64"""
    c = R.gpu_case(SCORE_P, N, M, 1.0 if N == 4 else 0.6, 500 + N + M, dtype_name)
    hyp = [R.hypotheses(m, i) for m, i in zip(c["matches"], c["idx"])]
    return c["matches"], rounded(np.stack([h[0] for h in hyp]), dtype_name), np.stack([h[1] for h in hyp])


def band_share(matches, models, valid, thr, dtype_name):
    """(cells inside the guard band, cells) over the valid slots"""
    inband = cells = 0
    for p in range(len(matches)):
        for H, v in zip(models[p], valid[p]):
            if v and R.model_kind(H) == "scored":
                r = R.ratio2(H, matches[p], thr)
                cells += len(r)
                inband += int(R.in_band(r, dtype_name).sum())
    return inband, cells


IRLS_N = (4, 257, 2049)
# f64 steps per N: the oracle's margins fall by about 7 per fit and stay far above the f64 score tolerance (3e-9 at most) for these;
# four points are fitted exactly by the first step, so a second one gains exactly 0
IRLS_STEPS = {4: 1, 257: 5, 2049: 5}
IRLS_SEED = {4: 700, 257: 700, 2049: 700}


def perturbed(H, rng, px=1.5, side=640.0):
    """H with its action on the square's corners moved by up to `px` pixels: the DLT of the moved corners"""
    c = np.array([[0.0, 0.0], [side, 0.0], [side, side], [0.0, side]])
    y = np.concatenate([c, np.ones((4, 1))], 1) @ np.asarray(H).T
    y = y[:, :2] / y[:, 2:] + rng.uniform(-px, px, (4, 2))
    return R.closed_form(np.concatenate([c, y], 1))["model"]


def irls_case(N, dtype_name, iters, claimed=None, thr=R.THRESHOLD):
    """four pairs: 0 and 1 the generating H of two scenes (60 % inliers; N = 4: inliers alone), each perturbed; 2 a start model that
    leaves no point inside the cutoff (a shift by 10^4 pixels); 3 a NaN model.  claimed: best_score values in the place of the start
    models' own scores for pairs 0 and 1.  -> (matches [4,N,4], start [4,3,3], score [4], per pair dict(model, score, fits, margins,
    trace, tol = the largest score tolerance among the start model and the candidates scored))"""
    sc = [R.scene(IRLS_SEED[N] + 10 * N + p, N, 1.0 if N == 4 else 0.6) for p in range(4)]
    m = rounded(np.stack([s["matches"] for s in sc]), dtype_name)
    rng = np.random.default_rng(N)
    far = R.canonical(np.array([[1.0, 0.0, 1e4], [0.0, 1.0, 1e4], [0.0, 0.0, 1.0]]))
    start = np.stack([perturbed(sc[0]["H"], rng), perturbed(sc[1]["H"], rng), far, np.full((3, 3), np.nan)])
    start = rounded(start, dtype_name)
    score = np.array([magsac(m[p], start[p], thr)[0] for p in range(4)])
    score[3] = 0.0                                          # (a NaN model is never the state's own: the state starts at score 0)
    if claimed is not None:
        score[:2] = claimed
    score = rounded(score, dtype_name)
    out = []
    for p in range(4):
        trace = []
        model, s, fits, margins = irls(m[p], start[p], thr, iters, score[p], trace, dtype_name)
        scored = [t["cand"] for t in trace if t["cand"] is not None] + ([start[p]] if R.model_kind(start[p]) == "scored" else [])
        out.append(dict(model=model, score=s, fits=fits, margins=margins, trace=trace,
                        tol=max([score_tolerance(m[p], c, thr, dtype_name) for c in scored] + [0.0])))
    return m, start, score, out


def irls_clear(o, dtype_name):
    """the condition a pair's comparison rests on: every margin of the oracle exceeds the score tolerance, and no point lies in the
    f64 band of a step's row decision (the kernel takes that decision in f64 for either type)"""
    rows_clear = all(not R.in_band(t["ratio2"], "float64").any() for t in o["trace"])
    return rows_clear and min([abs(g) for g in o["margins"]] + [math.inf]) > o["tol"]


DRV = dict(P=3, N=300, B=64, max_iterations=256, irls_iters=3, shares=(0.6, 0.35, 0.15), seed=940)


def driver_scenes():
    return [R.scene(DRV["seed"] + p, DRV["N"], s) for p, s in enumerate(DRV["shares"])]
