"""f64 oracle of the two-view MAGSAC++ scoring and IRLS polish (dr_magsac_score, dr_magsac_irls, BatchedRANSAC(scoring="magsac")),
written from the definitions with torch.special.gammainc / gammaincc -- not from the closed form the kernels evaluate.  The Sampson
distance, its forward bound and the inputs are tests/msac_ref.py's.  The weighted fits of the IRLS oracle are NOT restated here: they are
oracle/cpu_ref.py's f64 solvers (fundamental_8pt, nister_5pt) handed the row weights -- independent of the kernels, like refit_ref.py's.

d2 = the squared Sampson distance, thr2 = (1.5 thr)^2 read as (k sigma_max)^2, k^2 = chi2.ppf(0.99, 4); s = d2 / thr2, u = u_k s:
  weight  w(s) = (Gamma(3/2, u) - Gamma_k) / (Gamma_0 - Gamma_k)                  for s < 1, else 0
  loss    l(s) = (u Gamma(3/2, u) + gamma(5/2, u) - u Gamma_k) / rho_1            for s < 1, else 1
  score        = sum_n (1 - l(s_n)),  inliers = #{s_n < 1};  a non-finite d2 contributes nothing.

Tolerance of a score:  SAFETY x ( L sum_n bound_n / thr2  +  C_RED u ref  +  N E_term ).
  L = u_k (Gamma_0 - Gamma_k) / rho_1, the Lipschitz constant of 1 - l in s (attained at s = 0); bound_n = msac_ref.sampson_ref's forward
  bound of d2, summed over the points that can hold a non-zero term.
  C_RED, from the kernels' reduction: 8 sequential adds of a lane's points (the wave-per-model path: at most 4), 6 steps of the wave
  tree, one accumulation per 2048-point chunk onto the wave's LDS partial, 3 adds of the four waves, 1 for the term's last FMA.
  E_term = the absolute error of evaluating 1 - l at an exact s with the closed form of csrc/magsac_device.hpp,
      u = u_k s;  x = sqrt(u);  F = Gamma_0 erfc(x);  G = x exp(-u) + F;  rho = u (F - Gamma_k) + (3 sqrt(pi)/4 - 1.5 G);  1 - rho / rho_1,
  from the ulp bounds of the device library's functions: sqrt 1, exp 1, erfc 4 (f32) / 5 (f64) ulp (the single- and double-precision
  tables of the HIP math API reference), one unit roundoff per operation as written and per rounded constant, and the conditioning
  x erfc'(x) / erfc(x) of erfc for the error of its argument; term_error_bound() evaluates that first-order bound at an s, E_TERM is
  its ceiling over [0, 1) (tests/test_magsac_host.py recomputes it on a dense grid).  1 ulp = 2 unit roundoffs."""
import math

import torch

from oracle import cpu_ref as O
from tests import msac_ref as R

F64 = torch.float64
K2 = 13.276704135987622                  # chi2.ppf(0.99, df=4)
UK = 0.5 * K2
G0 = math.sqrt(math.pi) / 2.0            # Gamma(3/2)
G52 = 0.75 * math.sqrt(math.pi)          # Gamma(5/2)


def _upper32(u):
    return torch.special.gammaincc(torch.full_like(u, 1.5), u) * G0


def _lower52(u):
    return torch.special.gammainc(torch.full_like(u, 2.5), u) * G52


GK = float(_upper32(torch.tensor([UK], dtype=F64)))
RHO1 = float(_lower52(torch.tensor([UK], dtype=F64)))
L = UK * (G0 - GK) / RHO1
FUNC_ULPS = {"sqrt": 1.0, "exp": 1.0, "erfc": {torch.float32: 4.0, torch.float64: 5.0}}
# ceilings of term_error_bound over [0, 1), in unit roundoffs (13.3 / 15.3 on 10^5 points; the host test holds them)
E_TERM_UNITS = {torch.float32: 14.0, torch.float64: 16.0}
SAFETY = R.SAFETY


def e_term(dtype):
    return E_TERM_UNITS[dtype] * R.unit(dtype)


def weight(s):
    s = torch.as_tensor(s, dtype=F64)
    u = UK * s.clamp(min=0.0, max=1.0)
    return torch.where(s < 1.0, (_upper32(u) - GK) / (G0 - GK), torch.zeros_like(s))


def loss(s):
    s = torch.as_tensor(s, dtype=F64)
    u = UK * s.clamp(min=0.0, max=1.0)
    return torch.where(s < 1.0, (u * _upper32(u) + _lower52(u) - u * GK) / RHO1, torch.ones_like(s))


def closed_form(s):
    """(1 - l, w) by the closed form the issue states, f64"""
    s = torch.as_tensor(s, dtype=F64)
    u = UK * s
    x = torch.sqrt(u)
    F = G0 * torch.special.erfc(x)
    q = x * torch.exp(-u)
    rho = (u - 1.5) * F - 1.5 * q + G52 - u * GK
    return 1.0 - rho / RHO1, (F + q - GK) / (G0 - GK)


def term_error_bound(s, dtype):
    """first-order bound of |computed (1 - l)(s) - exact|, in unit roundoffs (module docstring), s in [0, 1)"""
    s = torch.as_tensor(s, dtype=F64)
    u = UK * s
    x = torch.sqrt(u)
    ec = torch.special.erfc(x)
    F = G0 * ec
    q = x * torch.exp(-u)
    G = F + q
    cond = 2.0 * x * x * torch.exp(-u) / (math.sqrt(math.pi) * ec)            # |x erfc'(x) / erfc(x)|
    rel_F = 2.0 * FUNC_ULPS["erfc"][dtype] + cond * 2.0 * FUNC_ULPS["sqrt"] + 2.0   # + Gamma_0 rounded, the product
    rel_q = 2.0 * FUNC_ULPS["sqrt"] + 2.0 * FUNC_ULPS["exp"] + 1.0
    err_G = F * rel_F + q * rel_q + G
    err_Fk = F * rel_F + (F - GK).abs() + GK
    inner = G52 - 1.5 * G
    err_inner = 1.5 * err_G + inner.abs() + G52
    rho = u * (F - GK) + inner
    err_rho = u * err_Fk + err_inner + rho.abs()
    gain = 1.0 - rho / RHO1
    return (err_rho + rho.abs()) / RHO1 + gain.abs() + 2.0 * L * s             # u = s u_k: u_k rounded, the product


# --------------------------------------------------------------------------------------------- the launch paths, restated
def dispatch(P, M, N, dtype=torch.float32):
    """magsac_score_launch -> (kernel, chunks): 'wave1' / 'wave2' / 'wave4' (N <= 256, a wave per model, both types) or 'block'
    (32-slot tiles, 8 points per lane, the block walks `chunks` 2048-point chunks)"""
    if N <= 256:
        return ("wave1" if N <= 64 else "wave2" if N <= 128 else "wave4"), 1
    return "block", (N + 2047) // 2048


def c_red(N):
    return 8 + 6 + 3 + 1 + (N + 2047) // 2048


SCORE_N, SCORE_M, SCORE_P = (1, 63, 64, 65, 255, 256, 257, 272, 2047, 2064), (1, 15, 16, 17, 65), (1, 3)
SCORE_CHUNKS = (3, 17, 4112)
F64_N, F64_M = (1, 7, 2049), (1, 33)
MMAX = 70        # models are made once per (N, dtype) and cut to a case's M (msac_ref.two_view_sets: a model does not depend on M)
PATTERN_SHAPE, PROPS_SHAPE, TINY_M = (3, 70, 272), (3, 65, 272), R.TINY_M
PATTERN_N = (64, 128, 256, 257, 272)     # one row length per wave variant and two of the block kernel: slot rules and gate on every path
K6_SHAPE, K6_SEED = (8, 65, 272), 3039     # the seed: every pair's top-two margin exceeds twice the tolerance (host test)


def score_shapes():
    """[(P, M, N, dtype)] of test_gpu_magsac_score's shape sweep"""
    out = [(p, m, n, torch.float32) for n in SCORE_N for m in SCORE_M for p in SCORE_P]
    out.append(SCORE_CHUNKS + (torch.float32,))
    out += [(3, m, n, torch.float64) for n in F64_N for m in F64_M]
    return out


def intended_paths():
    """{(kernel, chunks)} the sweep is meant to reach: every launch path, one and several chunks"""
    return {("wave1", 1), ("wave2", 1), ("wave4", 1), ("block", 1), ("block", 2), ("block", 3)}


# --------------------------------------------------------------------------------------------- score reference
_REFS = {}


def score_ref(matches, models, thr, dtype):
    """matches [N,4], models [M,3,3] (values of `dtype`), thr as handed to the kernel -> dict(scores [M] (NaN: non-finite / all-zero
    model), inliers [M], excl [M] = points with |d2 - thr2| <= 2 bound, tol [M], nan [M])"""
    r = R.sampson_ref(matches, models, thr, R.unit(dtype))
    s = r["d2"] / r["thr2"]
    live = r["masks"]
    term = torch.where(live, 1.0 - loss(torch.where(live, s, torch.zeros_like(s))), torch.zeros_like(s))
    scores = term.sum(-1)
    scores[r["nan"]] = float("nan")
    N = matches.shape[0]
    tol = SAFETY * (L * r["score_slack"] + c_red(N) * R.unit(dtype) * scores.abs().nan_to_num() + N * e_term(dtype))
    return dict(scores=scores, inliers=live.sum(-1), excl=r["excl"].sum(-1), tol=tol, nan=r["nan"])


def case_refs(S, N, seed, dtype, special, thr, mmax=MMAX):
    """(matches [S,N,4], models [S,mmax,3,3], [score_ref per set]) of a shape group, made once"""
    key = (S, N, seed, dtype, special, thr, mmax)
    if key not in _REFS:
        mt, md = R.two_view_sets(S, mmax, N, seed, dtype, R.SPECIALS if special else ())
        t = thr if dtype == torch.float64 else float(torch.tensor(thr, dtype=torch.float32))
        _REFS[key] = (mt, md, [score_ref(mt[s], md[s], t, dtype) for s in range(S)])
    return _REFS[key]


def gpu_cases():
    """every (P, M, N, dtype, thr, seed, mmax, special, pattern) test_gpu_magsac_score holds to the caps, so that the host test can hold
    the reference alone to them on exactly these inputs (the gated run shares the pattern runs' inputs)"""
    out = [dict(P=p, M=m, N=n, dtype=dt, thr=R.THR, seed=1000 + n, mmax=MMAX, special=True, pattern=None) for p, m, n, dt in score_shapes()]
    P, M, _ = PATTERN_SHAPE
    out += [dict(P=P, M=M, N=n, dtype=torch.float32, thr=R.THR, seed=1000 + n, mmax=MMAX, special=True, pattern=pat)
            for n in PATTERN_N for pat in R.VALID_PATTERNS]
    P, M, N = PROPS_SHAPE
    out.append(dict(P=P, M=M, N=N, dtype=torch.float32, thr=R.THR_HUGE, seed=1000 + N, mmax=MMAX, special=False, pattern=None))
    out.append(dict(P=P, M=TINY_M, N=N, dtype=torch.float32, thr=R.THR_TINY, seed=R.TINY_SEED, mmax=TINY_M, special=False, pattern=None))
    return out


def case_inputs(c):
    """-> (matches [3,N,4], models [3,mmax,3,3], per-set references, valid [P,M] | None) of a gpu_cases() entry"""
    mt, md, refs = case_refs(3, c["N"], c["seed"], c["dtype"], c["special"], c["thr"], c["mmax"])
    return mt, md, refs, (None if c["pattern"] is None else R.valid_pattern(c["pattern"], c["P"], c["M"]))


def within_caps(n_ex, n_in, points):
    """the two caps of the GPU tests: conditions on the inputs, not measurements"""
    return (n_ex <= R.CAP_INLIERS * n_in or n_ex == 0) and n_ex <= R.CAP_BYTES * max(points, 1)


def sweep_inputs(N, dtype):
    return case_refs(3, N, 1000 + N, dtype, True, R.THR)


def reference_cap(refs, M, P, valid=None):
    """(excluded points, reference inliers, points) over the evaluated slots of a case, from the reference alone"""
    S = len(refs)
    sel = torch.arange(P) % S
    live = ~torch.stack([r["nan"][:M] for r in refs])[sel]
    if valid is not None:
        live = live & valid
    ex = torch.stack([r["excl"][:M] for r in refs])[sel]
    inl = torch.stack([r["inliers"][:M] for r in refs])[sel]
    return int((ex * live).sum()), int((inl * live).sum()), int(live.sum())


def magsac(matches, model, thr):
    """matches [N,4], one model, thr -> (score, inliers) in f64"""
    r = score_ref(matches, torch.as_tensor(model, dtype=F64).reshape(1, 3, 3), thr, torch.float64)
    return float(r["scores"][0]), int(r["inliers"][0])


def score_tolerance(matches, model, thr, dtype):
    model = torch.as_tensor(model).to(dtype).reshape(1, 3, 3)
    return float(score_ref(matches.to(dtype), model, thr, dtype)["tol"][0])


# --------------------------------------------------------------------------------------------- IRLS oracle
def _ratio(matches, model, thr):
    r = R.sampson_ref(matches, model.reshape(1, 3, 3), thr, R.U64)
    return (r["d2"] / r["thr2"])[0]


def weighted_fit(matches, w, fundamental):
    """the row-weighted refit over ALL points, rows scaled by sqrt(w): F = Hartley-normalised LSQ 8-point (normalisation unweighted);
    E = the five-point solve on the weighted Gram matrix -> (candidates [S,3,3] f64, usable [S] bool)"""
    m = matches.to(F64)[None]
    rw = torch.sqrt(w.to(F64))[None]
    if fundamental:
        F = O.fundamental_8pt(m, rw)
        F = F[0]
        return F.reshape(1, 3, 3), torch.isfinite(F).all().reshape(1)
    E, ok, real = O.nister_5pt(m, rw)
    return E[0], real[0] & ok[0] & torch.isfinite(E[0]).all(-1).all(-1)


def irls(matches, model, thr, iters, fundamental, score=None, dtype=F64):
    """dtype: the type the state and the candidates are stored in (every candidate is rounded to it before it is scored, as the kernel's
    are: over ten steps an unrounded f64 sequence drifts from an f32 state by more than one output rounding).
    -> (model [3,3], score, fits, margins): margins[i] = |best candidate score - current score| of fit i and, for E, also the gap
    between its two best candidates (what a rounding would have to cross to change the step)"""
    m = matches.to(F64)
    model = torch.as_tensor(model, dtype=F64).reshape(3, 3).clone()
    score = magsac(m, model, thr)[0] if score is None else float(score)
    kmin = 8 if fundamental else 5
    fits, margins = 0, []
    for _ in range(iters):
        s = _ratio(m, model, thr)
        live = torch.isfinite(s) & (s < 1.0)
        if int(live.sum()) < kmin:
            break
        w = torch.where(live, weight(torch.where(live, s, torch.zeros_like(s))), torch.zeros_like(s))
        cand, ok = weighted_fit(m, w, fundamental)
        cand = cand.to(dtype).to(F64)
        fits += 1
        sc = [magsac(m, cand[c], thr)[0] if bool(ok[c]) else -math.inf for c in range(cand.shape[0])]
        if not any(bool(o) for o in ok):
            break
        order = sorted(range(len(sc)), key=lambda c: -sc[c])
        best = order[0]
        margins.append(abs(sc[best] - score))
        if len(order) > 1 and sc[order[1]] > -math.inf:
            margins.append(sc[best] - sc[order[1]])
        if not sc[best] > score:
            break
        model, score = cand[best].clone(), sc[best]
    return model, score, fits, margins


IRLS_P, IRLS_N, IRLS_THR, IRLS_ITERS, IRLS_SIGMA = 4, (8, 64, 300), (R.THR, 4 * R.THR), (1, 10), 1e-3


# scene seeds, chosen on the host (test_magsac_host.py holds the condition): a ten-step sequence that converges ends with margins below
# the f32 score tolerance, and with these seeds at most 2 of a shape's 16 cases do (4 are allowed)
IRLS_SEEDS = {(True, 64): 536, (True, 300): 504, (False, 64): 519, (False, 300): 503}


def irls_outside(N, fundamental, dtype):
    """cases of a shape whose oracle margins do not all exceed the score tolerance (of the oracle's final model), of 16"""
    mt, md = irls_inputs(N, fundamental)
    mt, md = mt.to(dtype), md.to(dtype)
    out = 0
    for thr in IRLS_THR:
        for iters in IRLS_ITERS:
            for p in range(IRLS_P):
                m, _, _, margins = irls(mt[p].double(), md[p].double(), thr, iters, fundamental, dtype=dtype)
                out += bool(margins) and min(margins) <= score_tolerance(mt[p], m, thr, dtype)
    return out


def irls_inputs(N, fundamental, seed=None):
    """P pairs of N inlier rows (normalised coordinates; noise 1e-3 of synth.two_view_pair) and start models gt + sigma randn, f64"""
    from differentiable_ransac_amd import synth
    seed = IRLS_SEEDS.get((bool(fundamental), N), 500) if seed is None else seed
    mts, mds = [], []
    for p in range(IRLS_P):
        d = synth.two_view_pair(seed + p, 2 * max(N, 8), dtype=F64)
        g = torch.Generator().manual_seed(seed * 31 + p)
        mts.append(d["matches"][-N:].to(F64))
        mds.append(d["gt_E"].to(F64) + IRLS_SIGMA * torch.randn(3, 3, generator=g, dtype=F64))
    return torch.stack(mts), torch.stack(mds)
