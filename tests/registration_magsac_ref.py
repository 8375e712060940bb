"""f64 numpy oracle of the MAGSAC++ scoring and IRLS polish of the registration path (dr_rigid_magsac_score, dr_registration_irls,
ransac.BatchedRegistration(scoring="magsac")), written from the maths and not from the kernels' code.  Scenes, the Kabsch fit, the
state step and the stop rule are tests/registration_ref.py's.

`threshold` is the cutoff DISTANCE, read as k sigma_max with k^2 = the 0.99 quantile of chi^2 with 3 degrees of freedom (the residual
q - (R p + t) is a 3-vector), the noise scale uniform in [0, sigma_max].  With s = d2 / threshold^2, u_k = k^2 / 2, c = exp(-u_k):

  weight  w(s) = (exp(-u_k s) - c) / (1 - c)                       for s < 1, else 0
  loss    l(s) = (1 - exp(-u_k s) - c u_k s) / (1 - c (1 + u_k))   for s < 1, else 1:  rho(d) = int_0^d x w(x) dx over rho(threshold)
  score        = sum_n (1 - l(s_n)) in [0, N];  inliers = #{s_n < 1};  a non-finite d2 contributes nothing
  irls         from (model, score), up to `iters` times: w(s_n) under the current model, the weighted Kabsch fit over all points, the
               candidate's score; taken only on a STRICTLY higher score.  Ends before a fit when fewer than three points have s < 1,
               on an invalid or non-finite fit, on a candidate that does not win, and at the step limit.

Tolerance of a score: L x registration_ref.score_tolerance + E.  The first term carries the error of s (registration_ref's bound is
that of sum_n s_n: 16 eps mag^2 / threshold^2 per point, of which rigid_d2 uses about ten roundings; the two roundings of the folded
factor u_k / threshold^2 and of its product with d2 are relative errors of s and fit into the rest) through the Lipschitz constant
L = max |d(1 - l)/ds| = u_k (1 - c) / (1 - c (1 + u_k)), attained at s = 0.  E carries the exponential itself: a relative error of
EXP_ULPS ulps in e = exp(-u_k s) moves a term by EXP_ULPS ulp(e) / (1 - c (1 + u_k)), and ulp(e) <= eps e for e < 1 (eps / 2 in
[0.5, 1), and exp(0) = 1 is exact), which is below eps (1 - c) for every s: so E = N EXP_ULPS eps L / u_k, L / u_k = (1 - c) / (1 - c (1 + u_k)).
EXP_ULPS: f32 uses v_exp_f32, 1 ulp (the V_EXP_F32 entry of AMD's CDNA instruction-set guides); f64 uses
the device library's exp, 1 ulp (the double-precision table of the HIP math API reference)."""
import math

import numpy as np

from tests import registration_ref as R

K2 = 11.344866730144373                 # chi2.ppf(0.99, df=3)
UK = 0.5 * K2
C = math.exp(-UK)
D = 1.0 - C * (1.0 + UK)                # the loss's normaliser: l(1) = 1
L = UK * (1.0 - C) / D                  # Lipschitz constant of 1 - l in s
EXP_ULPS = {"float32": 1.0, "float64": 1.0}


def weight(s):
    s = np.asarray(s, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(s < 1.0, (np.exp(-UK * s) - C) / (1.0 - C), 0.0)


def loss(s):
    s = np.asarray(s, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(s < 1.0, (1.0 - np.exp(-UK * s) - C * UK * s) / D, 1.0)


def rho(d2, thr):
    """int_0^d x w(x) dx as a function of d^2 (not normalised): threshold^2 / (2 u_k (1 - c)) x (1 - exp(-u_k s) - c u_k s)"""
    s = np.asarray(d2, np.float64) / (thr * thr)
    return thr * thr / (2.0 * UK * (1.0 - C)) * (1.0 - np.exp(-UK * s) - C * UK * s)


def magsac(matches, model, thr):
    """-> (score, inliers)"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = R.ratio2(model, matches, thr)
    live = np.isfinite(r) & (r < 1.0)
    return float((1.0 - loss(r[live])).sum()), int(live.sum())


def score_tolerance(matches, model, thr, dtype_name):
    n = len(matches)
    return L * R.score_tolerance(matches, model, thr, dtype_name) + n * EXP_ULPS[dtype_name] * R.eps_of(dtype_name) * L / UK


def irls(matches, model, thr, iters, score=None, trace=None):
    """-> (model, score, fits, margins): margins[i] = candidate score - current score of fit i (only for fits that gave a valid model).
    trace (a list, optional) receives registration_ref.kabsch's dict of every fit run"""
    m = np.asarray(matches, np.float64)
    model = np.array(model, np.float64).reshape(4, 4)
    score = magsac(m, model, thr)[0] if score is None else float(score)
    fits, margins = 0, []
    for _ in range(iters):
        with np.errstate(invalid="ignore", over="ignore"):
            r = R.ratio2(model, m, thr)
        live = np.isfinite(r) & (r < 1.0)
        if live.sum() < 3:
            break
        w = weight(r[live])
        cand = R.kabsch(m[live, :3], m[live, 3:], w)
        fits += 1
        if trace is not None:
            trace.append(cand)
        if not cand["valid"] or not np.isfinite(cand["model"]).all():
            break
        s = magsac(m, cand["model"], thr)[0]
        margins.append(s - score)
        if not s > score:
            break
        model, score = cand["model"], s
    return model, score, fits, margins


def run(matches, idx_per_round, thr=R.THRESHOLD, confidence=0.999, eps=1e-5, max_iterations=5000, do_refit=True, irls_iters=10):
    """registration_ref.run with this score and this polish.  -> dict(model, mask, score, inliers, iterations, ratio2, rounds, gaps =
    decision_margin of every round run, irls_fits, irls_margins, model_ratio = sigma_2 / sigma_1 of the fit the returned model came from)"""
    N = len(matches)
    st = R.new_state(N, max_iterations)
    gaps, rounds, win_ratio = [], 0, 1.0
    for idx in idx_per_round:
        if not st["iters"] < st["max_iters"]:
            break
        rounds += 1
        models, valid, ratios = R.hypotheses(matches, idx)
        scores = np.array([magsac(matches, M, thr)[0] if v else -1.0 for M, v in zip(models, valid)])
        top = np.sort(scores[valid])[::-1]
        if len(top):
            gaps.append(R.decision_margin(st["iters"] == 0, float(top[0]), float(top[1]) if len(top) > 1 else -math.inf,
                                          st["best_score"]))
        w = R.update(st, matches, models, valid, scores, thr, len(idx), confidence, eps, max_iterations)
        if w is not None:
            win_ratio = float(ratios[w])
    model, score, fits, margins = st["best_model"], st["best_score"], 0, []
    if do_refit and irls_iters > 0:
        trace = []
        model, score, fits, margins = irls(matches, model, thr, irls_iters, score, trace)
        taken = [t for t, g in zip(trace, margins) if g > 0]
        if taken:
            win_ratio = taken[-1]["ratio"]
    return dict(model=model, mask=st["best_mask"], score=score, inliers=st["best_inliers"], iterations=st["iters"],
                ratio2=st["best_ratio2"], rounds=rounds, gaps=gaps, irls_fits=fits, irls_margins=margins, model_ratio=win_ratio)
