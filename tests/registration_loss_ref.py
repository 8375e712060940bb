"""f64 reference of the registration training loss (csrc/registration_loss.hip, ops.registration_loss_mean, loss.RegistrationLoss),
written from its definition, the seeded inputs the host and GPU tests share, and the rules the comparisons follow.

Definition.  matches [P,N,6] = (p, q); models [P,M,4,4] = [[R, t], [0,0,0,1]]; mask [P,N] (the ground-truth inliers; None = all);
keep [P,M] (None = all); thr2 [P] = threshold^2, computed in the dtype under test as ops.thr2_tensor does.  With r = R p + t - q:

    d2 = |r|^2,  e = d2 / thr2 if d2 < thr2 else 1,  sums[p,m] = sum_{n in mask} e  (0 for a slot keep drops)
    per_pair[p] = sum_{m kept} sums[p,m] / max(#kept_p #mask_p, 1),  loss = mean_p per_pair[p]

`reference` evaluates this in torch f64 and differentiates it by autograd; `closed_form_gradient` is the hand-written gradient
d sums / d R = (2 / thr2) sum r p^T, d sums / d t = (2 / thr2) sum r over the masked points with d2 < thr2 (host test: the two agree).

Inputs.  Pair p of a case is kabsch_grad_ref.scene_matches(p, N) (registration_ref.scene(100 + p, N, 0.6): 60 % inliers with 5 mm of
noise, outliers in a 4 m cube), its pose the scene's, its mask the points within the threshold of that pose.  Three of four models
are the pose disturbed by a rotation of N(0, 0.03^2) rad per axis and a shift of N(0, 0.02^2) per axis -- displacements of the order
of the 5 cm threshold, so that both branches of the truncation occur in most of them -- and every fourth is a random pose.

Band rule.  The truncation is a step in the gradient (not in the value): a model is *near the boundary* if any masked point of it has
|d2 / thr2 - 1| < band = 64 eps(dtype under test).  Such models are left out of the gradient comparison (finiteness only), at most
2 % of the models of a case (`check_inputs`, asserted for every case when it is built).  Values are compared for all models.

Rounding margin.  Evaluated in the dtype under test, d2 carries the cancellation of q - (R p + t): three fused multiply-adds of
magnitude S_i = sum_j |R_ij||p_j| + |t_i| per component, a subtraction, three more for the square, so
|delta(d2 / thr2)| <= eps (3 sum_i |e_i| S_i + 2.5 d2) / thr2 =: margin (about 400 eps32 at the threshold, with |q| ~ 2 and thr = 0.05).
A point with band <= |d2 / thr2 - 1| <= margin could be decided either way by a correct f32 evaluation and would move the gradient by
a whole term.  The band is not widened for it: the model seeds of the cases (SEEDS) are chosen so that NO point of any model, and no
point under the ground-truth pose, lies in that zone in either dtype -- a property of the inputs and of the number format, found and
asserted with this module alone (`check_inputs`).

Tolerances.
  gradient, per model:  |g - g_ref|_inf <= c eps n mag x (coef_p |upstream| / P), n = #masked points of the pair, mag = (2 / thr2) sum |r||p|
      over the model's masked points with d2 < thr2, coef_p = 1 / max(#kept_p #mask_p, 1).  c = 4 w for both dtypes, with w the worst
      such ratio of a plain f32 torch evaluation of the closed form (einsum, (R p + t) - q) against the f64 reference, over the
      cases that share N (`worst_plain_ratio`).  The error is the cancellation above, per point about |S| / |r| eps of its term: in
      these units it is largest, about |S| / (|r| n), for the models with one or two points inside the threshold (random poses), it
      falls with n, and one constant per N is the tight choice.  4 x covers another order of summation.
      The f64 autograd reference is itself a plain evaluation, off by up to w in units of eps64, which is a quarter of what an f64
      kernel is allowed: with f64 under test g_ref is `extended_gradient`, the closed form in numpy.longdouble (64-bit mantissa),
      whose own error is 2^-11 of that.  The host test ties the two references together.
  sums, per model:  sum over the masked points with d2 < thr2 of the margin above (the truncated points contribute exactly 1), plus
      eps n_live sum e for the accumulation, plus eps.  per_pair: sum_{m kept} of those / den + eps M per_pair; mean: their mean + eps P."""
import functools

import numpy as np
import torch

from tests import kabsch_grad_ref as K
from tests import registration_ref as R

P = 3
N_SWEEP, M_AT_N = (1, 63, 64, 65, 257, 1000), 65
M_SWEEP, N_AT_M = (1, 63, 64, 65, 130), 257
CASES = [(N, M_AT_N) for N in N_SWEEP] + [(N_AT_M, M) for M in M_SWEEP if M != M_AT_N]
THRESHOLD = R.THRESHOLD
THRESHOLD_PAIRS = (0.05, 0.04, 0.06)
UPSTREAM = 1.75                       # the non-unit upstream scalar of the gradient tests
ROT_NOISE, SHIFT_NOISE = 0.03, 0.02
BAND_EPS, BAND_CAP = 64.0, 0.02
VARIANTS = [(um, uk, pairs) for um in (True, False) for uk in (True, False) for pairs in (False, True)]
GRAD_VARIANTS = [(True, True, True), (False, False, False)]
# model seed of a case where seed 0 leaves a point in the rounding-margin zone: one for which check_inputs holds in both dtypes (it is
# asserted when a case is built, so a seed that does not hold fails every test that uses the case)
SEEDS = {(1000, 65): 4, (257, 63): 1, (257, 130): 5}


def eps_of(dtype_name):
    return float(np.finfo(dtype_name).eps)


def thr2_of(threshold, dtype_name):
    """threshold^2 [P] as ops.thr2_tensor computes it: rounded to the dtype, squared in the dtype -> f64 array"""
    t = np.broadcast_to(np.asarray(threshold, np.float64), (P,)).astype(dtype_name)
    return (t * t).astype(np.float64)


def threshold_of(pairs):
    return THRESHOLD_PAIRS if pairs else THRESHOLD


@functools.lru_cache(maxsize=None)
def case(N, M, dtype_name="float64"):
    """-> dict(matches [P,N,6], pose [P,4,4], mask [P,N], models [P,M,4,4], keep [P,M]): f64 arrays holding values exact in the dtype"""
    rnd = lambda a: np.asarray(a, np.float64).astype(dtype_name).astype(np.float64)
    rng = np.random.default_rng(1000003 * SEEDS.get((N, M), 0) + 31 * N + M)
    matches = np.stack([K.scene_matches(p, N, np.dtype(dtype_name)) for p in range(P)])
    pose = np.tile(np.eye(4), (P, 1, 1))
    models = np.tile(np.eye(4), (P, M, 1, 1))
    for p in range(P):
        sc = R.scene(100 + p, N, 0.6)
        pose[p, :3, :3], pose[p, :3, 3] = sc["R"], sc["t"]
        for m in range(M):
            if m % 4 == 3:
                models[p, m, :3, :3], models[p, m, :3, 3] = R.random_rotation(rng), rng.standard_normal(3)
            else:
                W = R._cross_matrix(ROT_NOISE * rng.standard_normal(3)).astype(np.float64)
                models[p, m, :3, :3] = R._nearest_rotation(np.eye(3) + W + 0.5 * W @ W) @ sc["R"]
                models[p, m, :3, 3] = sc["t"] + SHIFT_NOISE * rng.standard_normal(3)
    keep = rng.uniform(size=(P, M)) < 0.8
    keep[:, 0] = True
    cs = dict(matches=matches, pose=rnd(pose), models=rnd(models), keep=keep, N=N, M=M)
    cs["mask"] = ratio(cs, cs["pose"][:, None], thr2_of(THRESHOLD, dtype_name))[:, 0] < 1.0
    check_inputs(cs, dtype_name)
    return cs


def residual(cs, models):
    """r = R p + t - q for models [P,M,4,4] -> [P,M,N,3] (f64)"""
    p, q = cs["matches"][..., :3], cs["matches"][..., 3:]
    return np.einsum("pmij,pnj->pmni", models[..., :3, :3], p) + models[..., None, :3, 3] - q[:, None]


def ratio(cs, models, thr2):
    """d2 / thr2 [P,M,N]"""
    r = residual(cs, models)
    return (r * r).sum(-1) / thr2[:, None, None]


def rounding_margin(cs, models, thr2, dtype_name):
    """the bound of the module docstring on the rounding error of d2 / thr2 evaluated in the dtype, [P,M,N]"""
    p = np.abs(cs["matches"][..., :3])
    S = np.einsum("pmij,pnj->pmni", np.abs(models[..., :3, :3]), p) + np.abs(models[..., None, :3, 3])
    e = np.abs(residual(cs, models))
    return eps_of(dtype_name) * (3.0 * (e * S).sum(-1) + 2.5 * (e * e).sum(-1)) / thr2[:, None, None]


def selection(cs, use_mask):
    return cs["mask"] if use_mask else np.ones(cs["matches"].shape[:2], bool)


def near_boundary(cs, thr2, use_mask, dtype_name):
    """the band rule -> [P,M] bool"""
    d = np.abs(ratio(cs, cs["models"], thr2) - 1.0) < BAND_EPS * eps_of(dtype_name)
    return (d & selection(cs, use_mask)[:, None, :]).any(-1)


def check_inputs(cs, dtype_name):
    """the cap of the band rule and the emptiness of the rounding-margin zone (module docstring), for both threshold forms, over
    ALL points (a superset of every mask) and with the ground-truth pose as one more model"""
    band = BAND_EPS * eps_of(dtype_name)
    models = np.concatenate([cs["models"], cs["pose"][:, None]], 1)
    for pairs in (False, True):
        thr2 = thr2_of(threshold_of(pairs), dtype_name)
        d = np.abs(ratio(cs, models, thr2) - 1.0)
        near = (d < band).any(-1)
        assert not near[:, -1].any(), "a point within the band of the ground-truth pose"
        assert near[:, :-1].sum() <= BAND_CAP * P * cs["M"], (cs["N"], cs["M"], dtype_name, int(near.sum()))
        gray = (d >= band) & (d <= rounding_margin(cs, models, thr2, dtype_name))
        assert not gray.any(), (cs["N"], cs["M"], dtype_name, pairs, int(gray.sum()))


def _loss(matches, models, mask, keep, thr2):
    """the definition, in torch: differentiable w.r.t. models -> (loss, per_pair, sums, d2)"""
    p, q = matches[..., :3], matches[..., 3:]
    r = torch.einsum("pmij,pnj->pmni", models[..., :3, :3], p) + models[..., None, :3, 3] - q[:, None]
    d2 = (r * r).sum(-1)
    t2 = thr2[:, None, None]
    e = torch.where(d2 < t2, d2 / t2, torch.ones_like(d2))
    sums = torch.where(mask[:, None, :], e, torch.zeros_like(e)).sum(-1)
    sums = torch.where(keep, sums, torch.zeros_like(sums))
    den = (keep.sum(1) * mask.sum(1)).clamp(min=1).to(sums.dtype)
    per_pair = sums.sum(1) / den
    return per_pair.mean(), per_pair, sums, d2


def reference(cs, thr2, use_mask=True, use_keep=True, upstream=UPSTREAM):
    """-> dict(mean, per_pair [P], sums [P,M], grad [P,M,4,4] = d (upstream x loss) / d models by autograd, coef [P],
    n [P] = #masked points, mag [P,M], live [P,M,N] = masked and d2 < thr2, masked [P,N], keep [P,M] as used); numpy"""
    mask = torch.tensor(selection(cs, use_mask))
    keep = torch.tensor(cs["keep"] if use_keep else np.ones_like(cs["keep"]))
    models = torch.tensor(cs["models"], requires_grad=True)
    t2 = torch.tensor(thr2)
    loss, per_pair, sums, d2 = _loss(torch.tensor(cs["matches"]), models, mask, keep, t2)
    (grad,) = torch.autograd.grad(loss * upstream, models)
    live = (mask[:, None, :] & (d2 < t2[:, None, None])).numpy()
    r = residual(cs, cs["models"])
    pn = np.linalg.norm(cs["matches"][..., :3], axis=-1)
    mag = (2.0 / thr2)[:, None] * (np.linalg.norm(r, axis=-1) * pn[:, None, :] * live).sum(-1)
    n = mask.sum(1).numpy()
    coef = 1.0 / np.maximum(keep.sum(1).numpy() * n, 1)
    return dict(mean=float(loss.detach()), per_pair=per_pair.detach().numpy(), sums=sums.detach().numpy(), grad=grad.numpy(), coef=coef, n=n,
                mag=mag, live=live, keep=keep.numpy(), masked=mask.numpy())


def closed_form_gradient(cs, thr2, ref, upstream=UPSTREAM, dtype=np.float64):
    """the hand-written gradient of upstream x loss, evaluated in `dtype` with plain torch ops (f64: against autograd in the host
    test; f32: the plain evaluation worst_plain_ratio measures) -> [P,M,4,4] f64"""
    tt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    m, x, t2 = torch.tensor(cs["models"]).to(tt), torch.tensor(cs["matches"]).to(tt), torch.tensor(thr2).to(tt)
    p, q = x[..., :3], x[..., 3:]
    r = torch.einsum("pmij,pnj->pmni", m[..., :3, :3], p) + m[..., None, :3, 3] - q[:, None]
    live = torch.tensor(ref["masked"])[:, None, :] & ((r * r).sum(-1) < t2[:, None, None])
    rl = r * live[..., None].to(tt)
    g = torch.zeros(m.shape, dtype=tt)
    g[..., :3, :3] = torch.einsum("pmni,pnj->pmij", rl, p)
    g[..., :3, 3] = rl.sum(2)
    scale = (2.0 / t2) * torch.tensor(ref["coef"] * upstream / P).to(tt)
    return (g * scale[:, None, None, None] * torch.tensor(ref["keep"]).to(tt)[..., None, None]).double().numpy()


def gradient_units(cs, thr2, ref, use_mask, dtype_name, upstream=UPSTREAM):
    """-> (unit [P,M] = eps n mag coef |upstream| / P: the tolerance is c x unit; compared [P,M] bool = kept, not near the boundary)"""
    unit = eps_of(dtype_name) * (ref["n"] * ref["coef"])[:, None] * ref["mag"] * abs(upstream) / P
    return unit, ref["keep"] & ~near_boundary(cs, thr2, use_mask, dtype_name)


def extended_gradient(cs, thr2, ref, upstream=UPSTREAM):
    """the closed form in numpy.longdouble on the reference's live set -> [P,M,4,4] longdouble: g_ref when f64 is under test"""
    LD = np.longdouble
    m, x = cs["models"].astype(LD), cs["matches"].astype(LD)
    p, q = x[..., :3], x[..., 3:]
    r = np.einsum("pmij,pnj->pmni", m[..., :3, :3], p) + m[..., None, :3, 3] - q[:, None]
    rl = r * ref["live"][..., None]
    g = np.zeros(m.shape, LD)
    g[..., :3, :3] = np.einsum("pmni,pnj->pmij", rl, p)
    g[..., :3, 3] = rl.sum(2)
    scale = (LD(2) / thr2.astype(LD)) * (ref["coef"].astype(LD) * LD(upstream) / P)
    return g * scale[:, None, None, None] * ref["keep"][..., None, None]


def worst_ratio(g, g_ref, unit, compared):
    """max over the compared models of |g - g_ref|_inf / unit (models whose unit is 0 must match exactly: inf otherwise)"""
    err = np.abs(g.astype(np.longdouble) - g_ref).max((-1, -2)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(unit > 0, err / unit, np.where(err > 0, np.inf, 0.0))
    return float(ratio[compared].max()) if compared.any() else 0.0


@functools.lru_cache(maxsize=None)
def worst_plain_ratio():
    """-> dict(N -> w): the worst ratio of the plain f32 evaluation of the closed form against the f64 reference, on the f32 inputs of
    the cases with that N, both gradient variants"""
    out = {}
    for N, M in CASES:
        cs = case(N, M, "float32")
        for use_mask, use_keep, pairs in GRAD_VARIANTS:
            thr2 = thr2_of(threshold_of(pairs), "float32")
            ref = reference(cs, thr2, use_mask, use_keep)
            unit, compared = gradient_units(cs, thr2, ref, use_mask, "float32")
            g = closed_form_gradient(cs, thr2, ref, dtype=np.float32)
            out[N] = max(out.get(N, 0.0), worst_ratio(g, ref["grad"], unit, compared))
    return out


def tolerance_constant():
    """-> dict(N -> c = 4 w), for both dtypes"""
    return {N: 4.0 * w for N, w in worst_plain_ratio().items()}


def value_tolerances(cs, thr2, ref, dtype_name):
    """-> (sums [P,M], per_pair [P], mean): module docstring"""
    eps = eps_of(dtype_name)
    marg = (rounding_margin(cs, cs["models"], thr2, dtype_name) * ref["live"]).sum(-1)
    n_live = ref["live"].sum(-1)
    tol = np.where(ref["keep"], marg + eps * n_live * ref["sums"] + eps, 0.0)
    pair = tol.sum(1) * ref["coef"] + eps * cs["M"] * ref["per_pair"] + eps
    return tol, pair, float(pair.mean() + eps * P)
