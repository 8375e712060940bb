"""dr_refit_pnp_weighted, dr_refit_pnp_bwd and dr_pnp_dlt (ops.weighted_pnp, ops.pnp_dlt) against the f64 reference
tests/weighted_pnp_ref.py, in f32 and f64.  Every tolerance is TOL_FACTOR = 8 times a figure the reference measures on itself (its run on
inputs as the kernel receives them against its run on the f64 originals), plus, where stated, a rounding bound written down in the
reference -- never anything a kernel returned.  The measured figures are printed next to each bound; docs/LOG.md records them.

Figures of the last run on an MI355X are in docs/LOG.md ("Differentiable weighted PnP")."""
import functools

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import loss, ops
from differentiable_ransac_amd.ops import L, ptr, stream
from differentiable_ransac_amd.ransac import BatchedPnP
from tests import pnp_ref as R
from tests import weighted_pnp_ref as W

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.float64]
F = W.TOL_FACTOR


def _name(dt):
    return "float32" if dt == torch.float32 else "float64"


def _dev(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dt is None else t.to(dt)


def _np(t):
    return t.double().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _upstream(P):
    return np.stack([np.random.default_rng(100 + p).normal(size=(4, 4)) for p in range(P)])


@functools.lru_cache(maxsize=None)
def _ref(P, N, name, ragged=False):
    """the case's inputs, the upstream gradients, per pair dict(a = the reference's stationary point and gradients on the f64 originals,
    gn = the same with J^T J in the Hessian's place, Tr = its LM at ITERS passes) and the case's figures (the largest of its pairs):
    fm, fw of the gradients and fT of the forward, each measured by the reference on itself for a kernel of type `name`"""
    cs = W.case(P, N, ragged=ragged)
    G = _upstream(P)
    out, fig = [], dict(fm=0.0, fw=0.0, fT=0.0)
    for p in range(P):
        mask = cs["mask"][p] if ragged else None
        a, fm, fw = W.backward_figures(cs["m"][p], cs["w"][p], mask, cs["start"][p], G[p], name)
        gn = W.solve_and_grad(cs["m"][p], cs["w"][p], mask, a["T"], G[p], gauss_newton=True, iters=10)
        Tr, fT = W.forward_figures(cs["m"][p], cs["w"][p], mask, cs["start"][p], name)
        fig = dict(fm=max(fig["fm"], fm), fw=max(fig["fw"], fw), fT=max(fig["fT"], fT))
        out.append(dict(a=a, gn=gn, Tr=Tr))
    return cs, G, out, fig


def _raw_refit(tm, mask, w, init, iters):
    P, N, _ = tm.shape
    model, valid = torch.empty((P, 4, 4), device=DEV, dtype=tm.dtype), torch.empty((P,), device=DEV, dtype=torch.bool)
    L.call(f"dr_refit_pnp_weighted_{L.suffix(tm.dtype)}", ptr(tm), ptr(None if mask is None else mask.view(torch.uint8)), ptr(w), ptr(init),
           P, N, iters, ptr(model), ptr(valid), stream())
    return model, valid


CASES = [(P, N, False) for P, N in W.SHAPES] + [(3, 7, True), (3, 300, True)]


# ---- forward ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_forward_bits_without_weights_and_values_with_them(dt):
    name = _name(dt)
    for P, N, ragged in CASES:
        cs, _, ref, fig = _ref(P, N, name, ragged)
        tm, tw, init = _dev(cs["m"], dt), _dev(cs["w"], dt), _dev(cs["start"], dt)
        mask = _dev(cs["mask"]) if ragged else None
        plain, pv = ops.refit_pnp(tm, mask, init, W.ITERS)
        mo, va = _raw_refit(tm, mask, None, init, W.ITERS)
        assert torch.equal(_bytes(mo), _bytes(plain)) and torch.equal(va, pv), (P, N, ragged)
        mo, va = ops.weighted_pnp(tm, tw, init, mask, W.ITERS)
        again = ops.weighted_pnp(tm, tw, init, mask, W.ITERS)
        assert torch.equal(_bytes(mo), _bytes(again[0])) and bool(va.all())
        got, tol = _np(mo), F * fig["fT"]
        errs = [W.deviation(got[p], r["Tr"]) for p, r in enumerate(ref)]
        print(f"forward {name} P={P} N={N} ragged={ragged}: errors {[float(f'{e:.3g}') for e in errs]}, measured {fig['fT']:.3g}, "
              f"bound {tol:.3g}")
        assert max(errs) <= tol, (P, N, ragged)


@pytest.mark.parametrize("dt", DTYPES)
def test_weights_of_exactly_one_give_the_bits_of_the_plain_refit(dt):
    """the weighted instantiation writes its sums with fma in the shape the unweighted ones compile to (csrc/pnp.hip says how): w = 1
    multiplies exactly, so every sum, every step and the model repeat the plain refit's bits"""
    shapes = []
    for P, N, ragged in CASES:
        cs = W.case(P, N, ragged=ragged)
        tm, init = _dev(cs["m"], dt), _dev(cs["start"], dt)
        mask = _dev(cs["mask"]) if ragged else None
        plain, pv = ops.refit_pnp(tm, mask, init, W.ITERS)
        mo, va = _raw_refit(tm, mask, torch.ones(P, N, device=DEV, dtype=dt), init, W.ITERS)
        if not (torch.equal(_bytes(mo), _bytes(plain)) and torch.equal(va, pv)):
            shapes.append((P, N, ragged, float((mo - plain).abs().max())))
    print(f"weights of one {_name(dt)}: shapes whose bits differ (P, N, ragged, max |difference|): {shapes}")
    assert not shapes


@pytest.mark.parametrize("dt", DTYPES)
def test_weight_zero_on_a_gross_outlier_is_the_masked_fit(dt):
    """the outlier is one in the OBSERVATION (its point stays in front of every candidate): weight 0 adds exact zeros to every sum, so
    the bits are those of the fit with the row masked out"""
    for P, N in [(3, 7), (3, 300)]:
        cs = W.case(P, N)
        m, w = cs["m"].copy(), cs["w"].copy()
        m[:, 1, 3:] += 0.5
        w[:, 1] = 0.0
        keep = np.ones((P, N), bool)
        keep[:, 1] = False
        tm, tw, init = _dev(m, dt), _dev(w, dt), _dev(cs["start"], dt)
        a, va = ops.weighted_pnp(tm, tw, init, None, W.ITERS)
        b, vb = ops.weighted_pnp(tm, tw, init, _dev(keep), W.ITERS)
        assert bool(va.all()) and bool(vb.all()) and torch.equal(_bytes(a), _bytes(b))
        c, _ = ops.weighted_pnp(tm, torch.where(tw == 0, torch.ones_like(tw), tw), init, None, W.ITERS)
        assert not torch.equal(_bytes(a), _bytes(c))          # (the outlier does move the fit when it counts)


# ---- backward -----------------------------------------------------------------------------------------------------------------------------
def _backward(tm, tw, init, mask, G, iters=W.ITERS):
    tm, tw = tm.clone().requires_grad_(True), tw.clone().requires_grad_(True)
    model, valid = ops.weighted_pnp(tm, tw, init, mask, iters)
    model.backward(G)
    return model.detach(), valid, tm.grad, tw.grad


@pytest.mark.parametrize("dt", DTYPES)
def test_backward_matches_the_implicit_function_theorem_of_the_reference(dt):
    """gradients to rows and weights for a random grad_model on noisy scenes.  Tolerance: 8 x the case's figures, the reference's own
    deviation on the kernel's inputs (the largest over the seeds of the one-ulp move and the pairs of the case).  On N >= 7 the
    reference with J^T J in H's place must lie outside that tolerance: a backward without the second-order terms fails here."""
    name = _name(dt)
    worst = 0.0
    for P, N, ragged in CASES:
        cs, G, ref, fig = _ref(P, N, name, ragged)
        tm, tw, init = _dev(cs["m"], dt), _dev(cs["w"], dt), _dev(cs["start"], dt)
        mask = _dev(cs["mask"]) if ragged else None
        model, valid, gm, gw = _backward(tm, tw, init, mask, _dev(G, dt))
        _, _, gm2, gw2 = _backward(tm, tw, init, mask, _dev(G, dt))
        assert torch.equal(_bytes(gm), _bytes(gm2)) and torch.equal(_bytes(gw), _bytes(gw2))          # two launches, the same bits
        assert bool(valid.all()) and bool(torch.isfinite(gm).all()) and bool(torch.isfinite(gw).all())
        gm, gw = _np(gm), _np(gw)
        tol_m, tol_w = F * fig["fm"], F * fig["fw"]
        left_out = 0
        for p, r in enumerate(ref):
            a, gn = r["a"], r["gn"]
            if a["cond"] > W.COND_MAX:
                left_out += 1
                continue
            em, ew = W.deviation(gm[p], a["gm"]), W.deviation(gw[p], a["gw"])
            print(f"backward {name} P={P} N={N} ragged={ragged} pair {p}: cond {a['cond']:.3g}; rows {em:.3g} / {tol_m:.3g}, weights "
                  f"{ew:.3g} / {tol_w:.3g}; J^T J off by {W.deviation(gn['gm'], a['gm']):.3g}, {W.deviation(gn['gw'], a['gw']):.3g}")
            worst = max(worst, em / tol_m, ew / tol_w)
            assert em <= tol_m and ew <= tol_w, (P, N, ragged, p)
            if N >= 7:
                assert W.deviation(gn["gm"], a["gm"]) > tol_m and W.deviation(gn["gw"], a["gw"]) > tol_w
            if ragged:
                off = ~cs["mask"][p]
                assert not gm[p][off].any() and not gw[p][off].any()
        assert left_out <= W.EXCLUDED_MAX * P
    print(f"backward {name}: worst error / tolerance {worst:.3g}")


@pytest.mark.parametrize("dt", DTYPES)
def test_exact_fit_of_three_rows_agrees_with_the_p3p_backward(dt):
    name = _name(dt)
    cs, G, ref, fig = _ref(1, 3, name)
    tm, tw, init = _dev(cs["m"], dt), _dev(cs["w"], dt), _dev(cs["start"], dt)
    model, valid, gm, gw = _backward(tm, tw, init, None, _dev(G, dt))
    assert bool(valid.all())
    ts = tm.clone().requires_grad_(True)
    slots, keep = ops.p3p(ts)
    d = (slots[0] - model[0]).abs().amax((-1, -2)) + (~keep[0]) * 1e9
    j = int(d.argmin())
    up = torch.zeros_like(slots)
    up[0, j] = _dev(G, dt)[0]
    slots.backward(up)
    err = W.deviation(_np(gm), _np(ts.grad))
    print(f"exact fit {name}: slot {j}; weighted_pnp against p3p backward {err:.3g} / {F * fig['fm']:.3g}; |grad w| max "
          f"{float(gw.abs().max()):.3g} / {F * fig['fw']:.3g}")
    assert float(d[j].detach()) < 1e-3 and err <= F * fig["fm"]
    assert float(gw.abs().max()) <= F * fig["fw"]


@pytest.mark.parametrize("dt", DTYPES)
def test_backward_zero_rules(dt):
    P, N = 3, 7
    cs = W.case(P, N, ragged=True)
    m, mask, start = cs["m"].copy(), cs["mask"].copy(), cs["start"].copy()
    mask[1] = True
    m[~mask] = np.nan                                         # pair 0, 2: masked rows are never read
    T = cs["gt"][1]                                           # pair 1: row 2 behind the camera, on the ray of its own observation
    m[1, 2, :3] = T[:3, :3].T @ (-2.0 * np.array([m[1, 2, 3], m[1, 2, 4], 1.0]) - T[:3, 3])
    start[2] = np.nan                                         # pair 2: no fit
    tm, tw = _dev(m, dt), _dev(cs["w"], dt)
    model, valid, gm, gw = _backward(tm, tw, _dev(start, dt), _dev(mask), _dev(_upstream(P), dt))
    assert valid.cpu().tolist() == [True, True, False] and torch.equal(model[2], torch.eye(4, device=DEV, dtype=dt))
    gm, gw = _np(gm), _np(gw)
    assert np.isfinite(gm).all() and np.isfinite(gw).all()
    assert not gm[~mask].any() and not gw[~mask].any()
    assert not gm[1, 2].any() and gw[1, 2] == 0.0
    assert not gm[2].any() and not gw[2].any()
    live = mask.copy()
    live[1, 2] = False
    live[2] = False
    assert (np.abs(gm[live]).sum(1) > 0).all() and (gw[live] != 0).all()
    # only one of the two gradients asked for: the same bits
    t1 = tm.clone().requires_grad_(True)
    ops.weighted_pnp(t1, tw, _dev(start, dt), _dev(mask), W.ITERS)[0].backward(_dev(_upstream(P), dt))
    assert np.array_equal(_np(t1.grad), gm)


@pytest.mark.parametrize("dt", DTYPES)
def test_composition_with_sigmoid_weights_and_the_pnp_loss(dt):
    P, N = 3, 300
    scs = [R.scene(40 + p, N, 0.7) for p in range(P)]
    tm = _dev(np.stack([s["matches"] for s in scs]), dt)
    gt = _dev(np.stack([s["pose"] for s in scs]), dt)
    logits = _dev(np.stack([np.where(s["inlier"], 2.0, -2.0) for s in scs]), dt).requires_grad_(True)
    model, valid = ops.weighted_pnp(tm, torch.sigmoid(logits))
    assert bool(valid.all())
    value = loss.PnPLoss(0.05).forward(model, tm, gt_pose=gt)
    value.backward()
    assert bool(torch.isfinite(logits.grad).all()) and float(logits.grad.abs().sum()) > 0


# ---- DLT ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_dlt_matches_the_reference_and_starts_the_fit(dt):
    name = _name(dt)
    for P, N, ragged in CASES:
        if N < 6:
            continue
        cs = W.case(P, N, ragged=ragged)
        tm, tw = _dev(cs["m"], dt), _dev(cs["w"], dt)
        mask = _dev(cs["mask"]) if ragged else None
        mo, va = ops.pnp_dlt(tm, tw, mask)
        again = ops.pnp_dlt(tm, tw, mask)
        assert bool(va.all()) and torch.equal(_bytes(mo), _bytes(again[0]))
        got, refs, starts, fig = _np(mo), [], [], 0.0
        for p in range(P):
            mk = cs["mask"][p] if ragged else None
            a, oka = W.dlt(cs["m"][p], cs["w"][p], mk)
            assert oka
            for s in W._seeds(name):                       # the reference on the kernel's inputs, its pose rounded as the kernel's is
                k = lambda x, j: R.as_kernel_input(x, name, 10 * s + j)
                b, okb = W.dlt(k(cs["m"][p], 1), k(cs["w"][p], 2), mk)
                assert okb
                fig = max(fig, W.deviation(a, k(b, 5)))
            refs.append(a)
        errs = [W.deviation(got[p], refs[p]) for p in range(P)]
        print(f"dlt {name} P={P} N={N} ragged={ragged}: errors {[float(f'{e:.3g}') for e in errs]}, measured {fig:.3g}, bound {F * fig:.3g}")
        assert max(errs) <= F * fig, (P, N, ragged)
        # without a start: what the fit reaches from the truth.  The figure includes the reference's own LM from its own DLT
        free, vf = ops.weighted_pnp(tm, tw, None, mask, W.ITERS)
        assert bool(vf.all())
        figs, errs = [], []
        for p in range(P):
            mk = cs["mask"][p] if ragged else None
            Tg, f = W.forward_figures(cs["m"][p], cs["w"][p], mk, cs["gt"][p], name, other_starts=(refs[p],))
            figs.append(f)
            errs.append(W.deviation(_np(free)[p], Tg))
        print(f"no start {name} P={P} N={N} ragged={ragged}: errors {[float(f'{e:.3g}') for e in errs]}, measured {max(figs):.3g}, "
              f"bound {F * max(figs):.3g}")
        assert max(errs) <= F * max(figs), (P, N, ragged)


@pytest.mark.parametrize("dt", DTYPES)
def test_dlt_refuses_planes_short_sets_and_empty_masks(dt):
    N = 12
    flat, good = W.coplanar_case(N), R.scene(3, N, 1.0, 0.0)["matches"]
    tm = _dev(np.stack([flat, good, good, good]), dt)
    mask = np.ones((4, N), bool)
    mask[2, 5:] = False                                        # five rows
    mask[3] = False
    mo, va = ops.pnp_dlt(tm, None, _dev(mask))
    assert va.cpu().tolist() == [False, True, False, False]
    eye = torch.eye(4, device=DEV, dtype=dt)
    assert all(torch.equal(mo[p], eye) for p in (0, 2, 3))
    mo, va = ops.weighted_pnp(tm, None, None, _dev(mask))      # no start, no fit: pass one
    assert va.cpu().tolist() == [False, True, False, False] and all(torch.equal(mo[p], eye) for p in (0, 2, 3))
    mo, va = ops.weighted_pnp(tm[:1], None, _dev(R.scene(5, N, 1.0, 0.0)["pose"][None], dt))
    assert bool(va.all())


# ---- untouched paths ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_the_driver_still_issues_the_plain_refit(dt):
    D = R.DRV
    P, N, B = D["P"], D["N"], D["B"]
    tm = _dev(np.stack([s["matches"] for s in R.driver_scenes()]), dt)
    logits = torch.zeros(P, N, device=DEV, dtype=dt)
    kw = dict(ransac_batch_size=B, threshold=R.THRESHOLD, max_iterations=D["max_iterations"], seed=3)
    out, plain = BatchedPnP(**kw)(tm, logits), BatchedPnP(refit=False, **kw)(tm, logits)
    cand, ok = ops.refit_pnp(tm, plain["mask"], plain["model"], 10)
    score = ops.pnp_score(tm, cand[:, None], R.THRESHOLD, want_inliers=False)[0][:, 0]
    take = ok & (score > plain["score"])
    want = torch.where(take[:, None, None], cand, plain["model"])
    assert torch.equal(_bytes(out["model"]), _bytes(want)) and bool(take.any())
    raw, rv = _raw_refit(tm, plain["mask"], None, plain["model"], 10)
    assert torch.equal(_bytes(raw), _bytes(cand)) and torch.equal(rv, ok)
