"""f64 numpy restatement of local optimisation in the robust 3-D registration path (dr_registration_local_opt,
ransac.BatchedRegistration(lo = 1 / 2)), built on tests/registration_ref.py (kabsch through refit, msac, stop_rule, update) and
written from the rules, not from the kernel:

  gate     `seen` [17] = (best_score, best_model) of the last visit, NaN at first; equal bytes -> nothing happens.
  few      best_inliers < 3 -> only the snapshot is stored.
  loop     once (lo = 1) or up to lo_iters times (lo = 2): the Kabsch fit over best_mask; stop on an invalid or non-finite fit; the
           candidate's MSAC score and inliers over all points; taken only when score > best_score (strict), and then score, model, mask
           (the candidate's own) and inlier count are replaced; stop when the candidate loses or the accepted mask equals the old one.
  after    max_iters = stop_rule(best_inliers, N, 3); the snapshot; lo_refits += fits run.

lo_step returns one record per fit run, with what decides whether a kernel in another precision can be held to this trajectory:
margin = |candidate score - best score| (the acceptance decision) and band = min_n |d2_n / thr^2 - 1| (the inlier decisions)."""
import math

import numpy as np

from tests import registration_ref as R


def new_seen():
    return np.full(17, np.nan)


def _snapshot(state):
    return np.concatenate([[state["best_score"]], np.asarray(state["best_model"], np.float64).reshape(16)])


def lo_step(state, matches, thr, lo, lo_iters, seen, confidence=0.999, eps=1e-5, max_iterations=5000):
    """in place on `state` (a registration_ref.new_state dict; gains "lo_refits") and `seen`; -> None when the gate skipped the pair,
    else the list of dict(valid, accepted, margin, band, ratio, score) of the fits run"""
    if _snapshot(state).tobytes() == seen.tobytes():
        return None
    fits = []
    if state["best_inliers"] >= 3:
        for _ in range(1 if lo == 1 else lo_iters):
            cand = R.refit(matches, state["best_mask"])
            if not cand["valid"] or not np.isfinite(cand["model"]).all():
                fits.append(dict(valid=False, accepted=False, margin=math.inf, band=math.inf, ratio=0.0, score=-1.0))
                break
            s, n, r = R.msac(matches, cand["model"], thr)
            rec = dict(valid=True, accepted=s > state["best_score"], margin=abs(s - state["best_score"]),
                       band=float(np.abs(r - 1.0).min()), ratio=cand["ratio"], score=s)
            fits.append(rec)
            if not rec["accepted"]:
                break
            mask = r < 1.0
            unchanged = np.array_equal(mask, state["best_mask"])
            state.update(best_score=s, best_model=cand["model"], best_mask=mask, best_inliers=n, best_ratio2=r, model_ratio=cand["ratio"])
            if unchanged:
                break
        state["max_iters"] = R.stop_rule(state["best_inliers"], len(matches), confidence, eps, max_iterations)
    seen[:] = _snapshot(state)
    state["lo_refits"] = state.get("lo_refits", 0) + len(fits)
    return fits


def run_lo(matches, idx_per_round, lo, lo_iters, thr=R.THRESHOLD, confidence=0.999, eps=1e-5, max_iterations=5000, do_refit=True):
    """registration_ref.run with lo_step after every update.  -> its dict, plus lo_refits, lo_fits = every fit record of the call,
    and gaps = the decision margins of the rounds AND the acceptance margins of the fits"""
    N = len(matches)
    st = R.new_state(N, max_iterations)
    st["model_ratio"] = 1.0
    seen = new_seen()
    gaps, lo_fits, rounds = [], [], 0
    for idx in idx_per_round:
        if not st["iters"] < st["max_iters"]:
            break
        rounds += 1
        models, valid, ratios = R.hypotheses(matches, idx)
        scores = np.array([R.msac(matches, M, thr)[0] if v else -1.0 for M, v in zip(models, valid)])
        top = np.sort(scores[valid])[::-1]
        if len(top):
            gaps.append(R.decision_margin(st["iters"] == 0, float(top[0]), float(top[1]) if len(top) > 1 else -math.inf,
                                          st["best_score"]))
        w = R.update(st, matches, models, valid, scores, thr, len(idx), confidence, eps, max_iterations)
        if w is not None:
            st["model_ratio"] = float(ratios[w])
        fits = lo_step(st, matches, thr, lo, lo_iters, seen, confidence, eps, max_iterations)
        lo_fits += fits or []
    gaps += [f["margin"] for f in lo_fits]
    model, score, refit_gap, ratio = st["best_model"], st["best_score"], math.inf, st["model_ratio"]
    if do_refit:
        cand = R.refit(matches, st["best_mask"])
        if cand["valid"] and np.array_equal(cand["model"], model):
            pass      # LO ended on an unchanged mask: the final refit repeats its last fit -- the same model whichever way it goes
        elif cand["valid"]:
            s = R.msac(matches, cand["model"], thr)[0]
            refit_gap = abs(s - score)
            if s > score:
                model, score, ratio = cand["model"], s, cand["ratio"]
    return dict(model=model, mask=st["best_mask"], score=score, inliers=st["best_inliers"], iterations=st["iters"],
                ratio2=st["best_ratio2"], rounds=rounds, gaps=gaps, refit_gap=refit_gap, model_ratio=ratio,
                lo_refits=st.get("lo_refits", 0), lo_fits=lo_fits)


# ------------------------------------------------------------------------------------------------ the cases of the GPU test
LO_P, LO_NS, LO_ITERS, LO_NOISE = 6, (3, 255, 256, 257, 1000), 8, 0.02
LO_SHARES = (0.6, 0.35, 0.15)
LO_MAX_ITERATIONS = 5000


def rounded(a, dtype_name):
    """the values a kernel of that dtype is handed, as f64"""
    return np.asarray(a, np.float64).astype(dtype_name).astype(np.float64)


def lo_scene(N, p):
    return R.scene(LO_SCENE_SEED[N] + p, N, LO_SHARES[p % 3], noise=LO_NOISE)


# scene seeds per N; the state of pair p is seeded from three TRUE inliers drawn with a fixed seed (N = 3: the one possible sample).
# What the exclusion rule leaves out of these cases is counted and bounded by tests/test_registration_lo_host.py
LO_SCENE_SEED = {3: 4000, 255: 4100, 256: 4200, 257: 4300, 1000: 4400}


def seed_rows(N, p, sc):
    if N == 3:
        return np.arange(3)
    inl = np.flatnonzero(sc["inlier"])
    rng = np.random.default_rng(7000 + 10 * N + p)
    return np.sort(rng.choice(inl, 3, replace=False))


def seeded_state(m, rows, thr):
    """the state one oracle `update` leaves from the single hypothesis fitted to `rows`"""
    st = R.new_state(len(m), LO_MAX_ITERATIONS)
    models, valid, ratios = R.hypotheses(m, rows[None])
    scores = np.array([R.msac(m, models[0], thr)[0] if valid[0] else -1.0])
    R.update(st, m, models, valid, scores, thr, 64, max_iterations=LO_MAX_ITERATIONS)
    st["model_ratio"] = float(ratios[0])
    return st


def build_case(N, lo, dtype_name):
    """-> list over the P pairs of dict(matches = rounded inputs, seed = the seeded state (a copy), after = the state lo_step leaves,
    fits, tol = score tolerance at the final model, excluded)"""
    thr = float(np.asarray(R.THRESHOLD, dtype_name))
    out = []
    for p in range(LO_P):
        sc = lo_scene(N, p)
        m = rounded(sc["matches"], dtype_name)
        st = seeded_state(m, seed_rows(N, p, sc), thr)
        seed = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
        fits = lo_step(st, m, thr, lo, LO_ITERS, new_seen(), max_iterations=LO_MAX_ITERATIONS)
        tol = R.score_tolerance(m, st["best_model"], thr, dtype_name)
        excluded = any(f["valid"] and (f["margin"] < 2.0 * tol or f["band"] < R.BAND[dtype_name]) for f in fits)
        out.append(dict(matches=m, scene=sc, seed=seed, after=st, fits=fits, tol=tol, excluded=excluded, thr=thr))
    return out
