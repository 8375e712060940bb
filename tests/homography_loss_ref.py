"""f64 reference of the homography training loss (csrc/homography_loss.hip, ops.homography_loss_mean, loss.HomographyLoss), written
from its definition, the seeded inputs the host and GPU tests share, and the rules the comparisons follow.

Definition.  matches [P,N,4] = (x1, x2) in pixels; models [P,M,3,3] of any scale and either sign; mask [P,N] (the ground-truth
inliers; None = all); keep [P,M] (None = all); thr2 [P] = threshold^2, computed in the dtype under test as ops.thr2_tensor does.
With h = sign(det H) H, a = adj(H), X1 = (x1, 1), X2 = (x2, 1), y = h X1, z = a X2, t = y_xy / y_w, s = z_xy / z_w:

    e = x2 - t,  f = x1 - s,  d2 = |e|^2 + |f|^2,  live = y_w > 0 and z_w > 0 and d2 < thr2,  term = d2 / thr2 if live else 1
    sums[p,m] = sum_{n in mask} term  (0 for a slot keep drops)
    per_pair[p] = sum_{m kept} sums[p,m] / max(#kept_p #mask_p, 1),  loss = mean_p per_pair[p]

`reference` evaluates this in torch f64 and differentiates it by autograd; `closed_form_gradient` is the hand-written gradient the
kernel implements (host test: the two agree):

    d sums / d h = (2 / thr2) sum u X1^T,  u = (-e_0, -e_1, e . t) / y_w;   d sums / d a = (2 / thr2) sum v X2^T,  v = (-f_0, -f_1, f . s) / z_w
    d sums / d H = sign(det H) (d sums / d h + J^T d sums / d a),  J = d adj(h) / d h (linear in h; ADJ / adj_vjp below)

over the masked live points.  d2 does not change under H -> c H, c > 0, so <d sums / d H, H> = 0.

Inputs.  Pair p of a case is homography_ref.scene(100 + p, N, 0.6) (60 % inliers with 0.5 px of noise, outliers uniform in the 640 px
square), its mask the points live under the scene's H.  Three of four models are that H re-solved (homography_ref.closed_form) from
the four corners of the square and their images displaced by N(0, CORNER_NOISE^2) px per coordinate -- of the order of the 3 px
threshold, so that both branches of the truncation occur in most of them -- and every fourth is homography_ref.random_h.  Every
model is then multiplied by a scale drawn from [0.25, 4] and a random sign.

Band rule.  The decisions are steps in the gradient (not in the value): a model is *near a boundary* if a masked point of it has
|d2 / thr2 - 1| < band = 64 eps(dtype under test), or |y_w| (|z_w|) below 64 eps of the magnitude of its terms, sum_j |h_2j X1_j|
(sum_j Q_2j |X2_j| with Q the |products| of the adjugate's entries).  Such models are checked for finiteness only in the gradient
comparison, at most 2 % of the models of a case.  Values are compared for all models.

Rounding margin.  In the dtype under test a transferred coordinate t_k = y_k / y_w carries, per unit of eps,
    D_k = Y_k + |t_k| (Y_w + 3/2),   Y_k = sum_j |h_kj X1_j| / |y_w|
-- the numerator's two fused multiply-adds round partial sums no larger than sum_j |h_kj X1_j| (half an ulp each), the denominator's
the same relative to y_w and multiplied by |t_k|, the reciprocal one ulp and the final fma half an ulp of |t_k|.  On the other side the
adjugate's entries a = h h - h h are themselves rounded to eps (|h h| + |h h|) = eps Q (their own cancellation), which the linear forms
inherit on top of their own roundings: Z_k = 2 sum_j Q_kj |X2_j| / |z_w| takes Y_k's place.  Then
    |delta d2| <= eps (2 sum_k |e_k| D^y_k + 2 sum_k |f_k| D^z_k + 5/2 d2),   margin = that / thr2
(about 2e3 eps at the threshold for coordinates of some hundred pixels: 2e-4 in f32).  A point with band <= |d2 / thr2 - 1| <= margin
could be decided either way by a correct evaluation in the dtype and would move the gradient by a whole term.  The band is not
widened for it: NO point of any model, and no point under the ground-truth homography, lies in that zone, for either threshold form,
in the dtype of the case.  With M N ~ 10^5 (model, point) pairs and an f32 margin of 2e-4 a case drawn blindly has some tens of such
points whatever its seed, so the condition is met where it can be: model by model, a drawn model with a point in the zone is
drawn again (the generator's next draw) until it has none -- about one model in ten in f32, practically none in f64.  The scenes are
fixed; no point of theirs lies in the zone under the ground truth (SEEDS would move a case's model stream if a later change needed
it).  `check_inputs` asserts the cap and the emptiness of the zone whenever a case is built, with this module alone.  |y_w|, |z_w|:
their margin, eps times the terms' magnitude, lies inside the band, so there is no such zone for them.

Tolerances.
  gradient, per model and ENTRY:  |g - g_ref|[q] <= c eps W[q] x (2 / thr2) (coef_p |upstream| / P), coef_p = 1 / max(#kept_p #mask_p, 1).  W is
      the gradient's own formula with every cancelling quantity replaced by the magnitude of its rounding: e_k by D^y_k (e = x2 - t
      cancels from hundreds of pixels to a few, so eps D is hundreds of ulps of e: the whole error), hence
          U = (D_0, D_1, (|t_0| + |e_0|) D_0 + (|t_1| + |e_1|) D_1) / |y_w|,   W_h = sum_live U |X1|^T,   W_a likewise from D^z, s, f, z_w, X2,
          W = W_h + |J|^T W_a   (adj_vjp on |h| with every sign +: the transpose-Jacobian moves W_a's errors and adds none of weight)
      The accumulation itself adds eps n_live sum |u| |X|, smaller than W by the same |e| / D, and is left to the constant.  c = 4 w for
      both dtypes, with w the worst such ratio of a plain f32 torch evaluation of the closed form (matmul, true division) against the
      f64 reference over the cases that share N (`worst_plain_ratio`); 4 x covers another order of summation and the fused
      multiply-adds' different roundings.  It is measured from the reference, never from the kernel.  Found (x86-64, torch 2.10): W_FOUND below,
      0.10 to 0.20, so c = 0.4 to 0.8: the plain evaluation stays a fifth and less under the worst-case weights W.
      The f64 autograd reference is itself a plain evaluation, off by up to w in units of eps64: with f64 under test g_ref is
      `extended_gradient`, the closed form in numpy.longdouble (64-bit mantissa) on the reference's live set.
      <g, H> = 0 is checked against the same bound: |<g, H>| <= sum_q tol[q] |H[q]|.
  sums, per model:  sum over the masked live points of the margin above (the others contribute exactly 1), plus eps n_live sums for
      the accumulation, plus eps.  per_pair: sum_{m kept} of those x coef + eps M per_pair + eps; mean: their mean + eps P."""
import functools

import numpy as np
import torch

from tests import homography_ref as HR

P = 3
TILE = 256                            # kHLTile of csrc/homography_loss.hip: the sweep brackets it
N_SWEEP, M_AT_N = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 1000), 65
M_SWEEP, N_AT_M = (1, 63, 64, 65, 130), 257
CASES = [(N, M_AT_N) for N in N_SWEEP] + [(N_AT_M, M) for M in M_SWEEP if M != M_AT_N]
THRESHOLD = HR.THRESHOLD
THRESHOLD_PAIRS = (3.0, 2.5, 3.5)
UPSTREAM = 1.75                       # the non-unit upstream scalar of the gradient tests
CORNER_NOISE, SIDE = 1.5, 640.0
BAND_EPS, BAND_CAP = 64.0, 0.02
VARIANTS = [(um, uk, pairs) for um in (True, False) for uk in (True, False) for pairs in (False, True)]
GRAD_VARIANTS = [(True, True, True), (False, False, False)]
SEEDS = {}                            # (N, M) -> another model stream for a case; none is needed (module docstring)
# worst_plain_ratio() as found when this module was written (the host test prints the current values)
W_FOUND = {1: 0.199, 63: 0.097, 64: 0.145, 65: 0.130, 255: 0.099, 256: 0.118, 257: 0.175, 1000: 0.153}

# adj(H)[r][c] = the cofactor of H[c][r]: entry k = 3 r + c as (i, j, i', j') with a_k = h_i h_j - h_i' h_j'
ADJ = []
for _r in range(3):
    for _c in range(3):
        _rows, _cols = [i for i in range(3) if i != _c], [j for j in range(3) if j != _r]
        _q = (3 * _rows[0] + _cols[0], 3 * _rows[1] + _cols[1], 3 * _rows[0] + _cols[1], 3 * _rows[1] + _cols[0])
        ADJ.append(_q if (_r + _c) % 2 == 0 else (_q[2], _q[3], _q[0], _q[1]))


def adjugate9(h, stack):
    """h [...,9] -> adj [...,9] (numpy or torch: `stack` is the library's)"""
    return stack([h[..., i] * h[..., j] - h[..., k] * h[..., l] for i, j, k, l in ADJ], -1)


def adj_products9(h, stack):
    """|h_i h_j| + |h_i' h_j'| of every adjugate entry: the magnitude its rounding is relative to"""
    a = abs(h)
    return stack([a[..., i] * a[..., j] + a[..., k] * a[..., l] for i, j, k, l in ADJ], -1)


def adj_vjp(h, g, stack, absolute=False):
    """J^T g for a = adj(h): out[q] = sum_k g[k] d a_k / d h_q -> [...,9]; absolute: every sign + (a bound's propagation)"""
    out = [0] * 9
    neg = 1.0 if absolute else -1.0
    for k, (i, j, i2, j2) in enumerate(ADJ):
        out[i] = out[i] + g[..., k] * h[..., j]
        out[j] = out[j] + g[..., k] * h[..., i]
        out[i2] = out[i2] + neg * g[..., k] * h[..., j2]
        out[j2] = out[j2] + neg * g[..., k] * h[..., i2]
    return stack(out, -1)


def eps_of(dtype_name):
    return float(np.finfo(dtype_name).eps)


def thr2_of(threshold, dtype_name):
    """threshold^2 [P] as ops.thr2_tensor computes it: rounded to the dtype, squared in the dtype -> f64 array"""
    t = np.broadcast_to(np.asarray(threshold, np.float64), (P,)).astype(dtype_name)
    return (t * t).astype(np.float64)


def threshold_of(pairs):
    return THRESHOLD_PAIRS if pairs else THRESHOLD


def _homogeneous(x):
    return np.concatenate([x, np.ones(x.shape[:-1] + (1,), x.dtype)], -1)


def geometry(matches, models, dtype=np.float64):
    """matches [P,N,4], models [P,M,3,3] -> dict of [P,M,N(,k)] arrays in `dtype` (f64 or longdouble): yw, zw, t, s, e, f, d2, front,
    and per unit of eps Dy, Dz [..,2] (module docstring), Syw, Szw (the magnitude of y_w's and z_w's terms)"""
    x, H = matches.astype(dtype), models.astype(dtype).reshape(models.shape[:2] + (9,))
    det = H[..., 0] * (H[..., 4] * H[..., 8] - H[..., 5] * H[..., 7]) - H[..., 1] * (H[..., 3] * H[..., 8] - H[..., 5] * H[..., 6]) \
        + H[..., 2] * (H[..., 3] * H[..., 7] - H[..., 4] * H[..., 6])
    sign = np.where(det < 0, -1.0, 1.0).astype(dtype)
    h = (H * sign[..., None]).reshape(H.shape[:2] + (3, 3))
    a = adjugate9(H, np.stack).reshape(h.shape)
    Q = adj_products9(H, np.stack).reshape(h.shape)
    X1, X2 = _homogeneous(x[..., :2]), _homogeneous(x[..., 2:])
    y, z = np.einsum("pmij,pnj->pmni", h, X1), np.einsum("pmij,pnj->pmni", a, X2)
    Sy, Sz = np.einsum("pmij,pnj->pmni", np.abs(h), np.abs(X1)), 2.0 * np.einsum("pmij,pnj->pmni", Q, np.abs(X2))
    with np.errstate(all="ignore"):
        t, s = y[..., :2] / y[..., 2:], z[..., :2] / z[..., 2:]
        e, f = x[:, None, :, 2:] - t, x[:, None, :, :2] - s
        d2 = (e * e).sum(-1) + (f * f).sum(-1)
        yw, zw = y[..., 2], z[..., 2]
        Dy = Sy[..., :2] / np.abs(yw)[..., None] + np.abs(t) * (Sy[..., 2:] / np.abs(yw)[..., None] + 1.5)
        Dz = Sz[..., :2] / np.abs(zw)[..., None] + np.abs(s) * (Sz[..., 2:] / np.abs(zw)[..., None] + 1.5)
    return dict(sign=sign, h=h, a=a, X1=X1, X2=X2, yw=yw, zw=zw, t=t, s=s, e=e, f=f, d2=d2, front=(yw > 0) & (zw > 0), Dy=Dy, Dz=Dz,
                Syw=Sy[..., 2], Szw=Sz[..., 2])


def rounding_margin(geo, thr2, dtype_name):
    """the bound of the module docstring on the rounding error of d2 / thr2 evaluated in the dtype, [P,M,N]"""
    with np.errstate(all="ignore"):
        d = 2.0 * (np.abs(geo["e"]) * geo["Dy"]).sum(-1) + 2.0 * (np.abs(geo["f"]) * geo["Dz"]).sum(-1) + 2.5 * geo["d2"]
    return eps_of(dtype_name) * d / thr2[:, None, None]


def zones(geo, thr2, dtype_name):
    """-> (band [P,M,N]: inside a decision's band; gray [P,M,N]: between the band and the rounding margin)"""
    band = BAND_EPS * eps_of(dtype_name)
    with np.errstate(all="ignore"):
        d = np.abs(geo["d2"] / thr2[:, None, None] - 1.0)
        near_w = (np.abs(geo["yw"]) < band * geo["Syw"]) | (np.abs(geo["zw"]) < band * geo["Szw"])
        in_band = (geo["front"] & (d < band)) | near_w
        gray = geo["front"] & ~in_band & (d <= rounding_margin(geo, thr2, dtype_name))
    return in_band, gray


def _draw_model(rng, H):
    """one model of a case: the scene's H re-solved from displaced corners, or (the caller's every fourth) a random one; any scale, sign"""
    while True:
        if H is None:
            model = HR.random_h(rng, SIDE)
        else:
            c1 = np.array([[0.0, 0.0], [SIDE, 0.0], [SIDE, SIDE], [0.0, SIDE]])
            y = _homogeneous(c1) @ H.T
            c2 = y[:, :2] / y[:, 2:] + CORNER_NOISE * rng.standard_normal((4, 2))
            out = HR.closed_form(np.concatenate([c1, c2], 1))
            if not out["valid"]:
                continue
            model = out["model"]
        return model * rng.uniform(0.25, 4.0) * (1.0 if rng.uniform() < 0.5 else -1.0)


def _clean(matches_p, models, dtype_name):
    """-> [M] bool: the model has no point in the gray zone, for either threshold form"""
    geo = geometry(matches_p[None], models[None])
    ok = np.ones(len(models), bool)
    for pairs in (False, True):
        for thr2 in np.unique(thr2_of(threshold_of(pairs), dtype_name)):
            ok &= ~zones(geo, np.array([thr2]), dtype_name)[1][0].any(-1)
    return ok


@functools.lru_cache(maxsize=None)
def case(N, M, dtype_name="float64"):
    """-> dict(matches [P,N,4], gt_H [P,3,3], mask [P,N], models [P,M,3,3], keep [P,M]): f64 arrays holding values exact in the dtype"""
    rnd = lambda a: np.asarray(a, np.float64).astype(dtype_name).astype(np.float64)
    rng = np.random.default_rng(1000003 * SEEDS.get((N, M), 0) + 31 * N + M)
    scenes = [HR.scene(100 + p, N, 0.6) for p in range(P)]
    matches = rnd(np.stack([sc["matches"] for sc in scenes]))
    gt_H = rnd(np.stack([sc["H"] for sc in scenes]))
    models = np.zeros((P, M, 3, 3))
    for p in range(P):
        todo = np.arange(M)
        while len(todo):
            models[p, todo] = rnd(np.stack([_draw_model(rng, None if m % 4 == 3 else scenes[p]["H"]) for m in todo]))
            todo = todo[~_clean(matches[p], models[p, todo], dtype_name)]
    keep = rng.uniform(size=(P, M)) < 0.8
    keep[:, 0] = True
    cs = dict(matches=matches, gt_H=gt_H, models=models, keep=keep, N=N, M=M)
    geo = geometry(matches, gt_H[:, None])
    cs["mask"] = (geo["front"] & (geo["d2"] / thr2_of(THRESHOLD, dtype_name)[:, None, None] < 1.0))[:, 0]
    check_inputs(cs, dtype_name)
    return cs


def selection(cs, use_mask):
    return cs["mask"] if use_mask else np.ones(cs["matches"].shape[:2], bool)


def near_boundary(cs, thr2, use_mask, dtype_name):
    """the band rule -> [P,M] bool"""
    in_band, _ = zones(geometry(cs["matches"], cs["models"]), thr2, dtype_name)
    return (in_band & selection(cs, use_mask)[:, None, :]).any(-1)


def check_inputs(cs, dtype_name):
    """the cap of the band rule and the emptiness of the rounding-margin zone (module docstring), for both threshold forms, over
    ALL points (a superset of every mask) and with the ground-truth homography as one more model"""
    geo = geometry(cs["matches"], np.concatenate([cs["models"], cs["gt_H"][:, None]], 1))
    for pairs in (False, True):
        in_band, gray = zones(geo, thr2_of(threshold_of(pairs), dtype_name), dtype_name)
        near = in_band.any(-1)
        assert not near[:, -1].any(), "a point within the band of the ground-truth homography"
        assert near[:, :-1].sum() <= BAND_CAP * P * cs["M"], (cs["N"], cs["M"], dtype_name, int(near.sum()))
        assert not gray.any(), (cs["N"], cs["M"], dtype_name, pairs, int(gray.sum()))


def _transfer(matches, models, xp):
    """the definition's y, z, e, f, d2 in numpy or torch (`xp`), models [P,M,3,3] -> dict ([P,M,N,..])"""
    H9 = models.reshape(models.shape[:2] + (9,))
    det = H9[..., 0] * (H9[..., 4] * H9[..., 8] - H9[..., 5] * H9[..., 7]) - H9[..., 1] * (H9[..., 3] * H9[..., 8] - H9[..., 5] * H9[..., 6]) \
        + H9[..., 2] * (H9[..., 3] * H9[..., 7] - H9[..., 4] * H9[..., 6])
    sign = xp.where(det < 0, -xp.ones_like(det), xp.ones_like(det))
    h = models * sign[..., None, None]
    a = adjugate9(H9, xp.stack).reshape(models.shape)
    one = xp.ones_like(matches[..., :1])
    X1, X2 = xp.concatenate([matches[..., :2], one], -1), xp.concatenate([matches[..., 2:], one], -1)
    y, z = xp.einsum("pmij,pnj->pmni", h, X1), xp.einsum("pmij,pnj->pmni", a, X2)
    t, s = y[..., :2] / y[..., 2:], z[..., :2] / z[..., 2:]
    e, f = matches[:, None, :, 2:] - t, matches[:, None, :, :2] - s
    return dict(sign=sign, h=h, X1=X1, X2=X2, yw=y[..., 2], zw=z[..., 2], t=t, s=s, e=e, f=f, d2=(e * e).sum(-1) + (f * f).sum(-1))


def _loss(matches, models, mask, keep, thr2):
    """the definition, in torch: differentiable w.r.t. models -> (loss, per_pair, sums, live)"""
    g = _transfer(matches, models, torch)
    t2 = thr2[:, None, None]
    live = (g["yw"] > 0) & (g["zw"] > 0) & (g["d2"] < t2)
    term = torch.where(live, g["d2"] / t2, torch.ones_like(g["d2"]))
    sums = torch.where(mask[:, None, :], term, torch.zeros_like(term)).sum(-1)
    sums = torch.where(keep, sums, torch.zeros_like(sums))
    den = (keep.sum(1) * mask.sum(1)).clamp(min=1).to(sums.dtype)
    per_pair = sums.sum(1) / den
    return per_pair.mean(), per_pair, sums, live


def reference(cs, thr2, use_mask=True, use_keep=True, upstream=UPSTREAM):
    """-> dict(mean, per_pair [P], sums [P,M], grad [P,M,3,3] = d (upstream x loss) / d models by autograd, coef [P], n [P] = #masked
    points, W [P,M,3,3] (module docstring), live [P,M,N] = masked and live, masked [P,N], keep [P,M] as used, margin [P,M,N]); numpy"""
    mask = torch.tensor(selection(cs, use_mask))
    keep = torch.tensor(cs["keep"] if use_keep else np.ones_like(cs["keep"]))
    models = torch.tensor(cs["models"], requires_grad=True)
    loss, per_pair, sums, live = _loss(torch.tensor(cs["matches"]), models, mask, keep, torch.tensor(thr2))
    (grad,) = torch.autograd.grad(loss * upstream, models)
    live = (live & mask[:, None, :]).numpy()
    n = mask.sum(1).numpy()
    coef = 1.0 / np.maximum(keep.sum(1).numpy() * n, 1)
    geo = geometry(cs["matches"], cs["models"])
    lv = live[..., None].astype(np.float64)
    with np.errstate(all="ignore"):
        def weights(D, tt, ee, w, X):
            U = np.concatenate([D, ((np.abs(tt) + np.abs(ee)) * D).sum(-1, keepdims=True)], -1) / np.abs(w)[..., None]
            return np.einsum("pmnk,pnj->pmkj", np.where(lv > 0, U, 0.0), np.abs(X))
        Wh = weights(geo["Dy"], geo["t"], geo["e"], geo["yw"], geo["X1"])
        Wa = weights(geo["Dz"], geo["s"], geo["f"], geo["zw"], geo["X2"])
    W = Wh + adj_vjp(np.abs(geo["h"]).reshape(P, -1, 9), Wa.reshape(P, -1, 9), np.stack, absolute=True).reshape(Wh.shape)
    return dict(mean=float(loss.detach()), per_pair=per_pair.detach().numpy(), sums=sums.detach().numpy(), grad=grad.numpy(), coef=coef, n=n,
                W=W, live=live, keep=keep.numpy(), masked=mask.numpy(), margin=rounding_margin(geo, thr2, "float64") / eps_of("float64"))


def _closed_form(g, live, thr2, scale, keep, xp):
    """the hand-written gradient from _transfer's quantities on the live set -> [P,M,3,3]"""
    lv = xp.stack([live] * 3, -1)

    def half(ee, tt, w, X):
        u = xp.concatenate([-ee, (ee * tt).sum(-1)[..., None]], -1) / w[..., None]
        return xp.einsum("pmnk,pnj->pmkj", xp.where(lv, u, xp.zeros_like(u)), X)
    gh, ga = half(g["e"], g["t"], g["yw"], g["X1"]), half(g["f"], g["s"], g["zw"], g["X2"])
    shape = gh.shape
    back = adj_vjp(g["h"].reshape(shape[:2] + (9,)), ga.reshape(shape[:2] + (9,)), xp.stack).reshape(shape)
    return (gh + back) * (g["sign"] * scale[:, None] * keep)[..., None, None]


def closed_form_gradient(cs, thr2, ref, upstream=UPSTREAM, dtype=np.float64):
    """the hand-written gradient of upstream x loss, evaluated in `dtype` with plain torch ops (f64: against autograd in the host
    test; f32: the plain evaluation worst_plain_ratio measures), the live set decided in that dtype -> [P,M,3,3] f64"""
    tt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    m, x, t2 = torch.tensor(cs["models"]).to(tt), torch.tensor(cs["matches"]).to(tt), torch.tensor(thr2).to(tt)
    g = _transfer(x, m, torch)
    live = torch.tensor(ref["masked"])[:, None, :] & (g["yw"] > 0) & (g["zw"] > 0) & (g["d2"] < t2[:, None, None])
    scale = (2.0 / t2) * torch.tensor(ref["coef"] * upstream / P).to(tt)
    return _closed_form(g, live, t2, scale, torch.tensor(ref["keep"]).to(tt), torch).double().numpy()


def extended_gradient(cs, thr2, ref, upstream=UPSTREAM):
    """the closed form in numpy.longdouble on the reference's live set -> [P,M,3,3] longdouble: g_ref when f64 is under test"""
    LD = np.longdouble
    g = _transfer(cs["matches"].astype(LD), cs["models"].astype(LD), np)
    scale = (LD(2) / thr2.astype(LD)) * (ref["coef"].astype(LD) * LD(upstream) / P)
    with np.errstate(all="ignore"):
        return _closed_form(g, ref["live"], thr2, scale, ref["keep"].astype(LD), np)


def gradient_units(cs, thr2, ref, use_mask, dtype_name, upstream=UPSTREAM):
    """-> (unit [P,M,3,3] = eps W (2 / thr2) coef |upstream| / P: the tolerance is c x unit, entry by entry; compared [P,M] bool = kept,
    not near a boundary)"""
    unit = eps_of(dtype_name) * ref["W"] * ((2.0 / thr2) * ref["coef"] * abs(upstream) / P)[:, None, None, None]
    return unit, ref["keep"] & ~near_boundary(cs, thr2, use_mask, dtype_name)


def worst_ratio(g, g_ref, unit, compared):
    """max over the compared models and their entries of |g - g_ref| / unit (entries whose unit is 0 must match exactly: inf otherwise)"""
    err = np.abs(g.astype(np.longdouble) - g_ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(unit > 0, err / unit, np.where(err > 0, np.inf, 0.0))
    return float(ratio[compared].max()) if compared.any() else 0.0


def inner_ratio(g, cs, unit, compared):
    """max over the compared models of |<g, H>| / sum_q unit[q] |H[q]| (0 / 0 = 0)"""
    inner = np.abs((g * cs["models"]).sum((-1, -2)))
    bound = (unit * np.abs(cs["models"])).sum((-1, -2))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, inner / bound, np.where(inner > 0, np.inf, 0.0))
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
    marg = np.where(ref["live"], ref["margin"] * eps, 0.0).sum(-1)
    n_live = ref["live"].sum(-1)
    tol = np.where(ref["keep"], marg + eps * n_live * ref["sums"] + eps, 0.0)
    pair = tol.sum(1) * ref["coef"] + eps * cs["M"] * ref["per_pair"] + eps
    return tol, pair, float(pair.mean() + eps * P)
