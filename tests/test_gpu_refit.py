"""The refit kernels (dr_refit_fundamental, dr_refit_essential, and dr_local_opt which calls both) against the f64 restatements of
tests/refit_ref.py, where they can go wrong: selections that hold outliers (the two smallest eigenvalues of the Gram matrix
close to each other), row weights, point counts around the wave and block sizes, selections that live in one thread / one wave /
the last rows, the minimal and sub-minimal counts, an exactly singular Gram matrix, both launch forms of the E refit, and local
optimisation started from a contaminated mask.

The F tolerance is refit_ref.f_tolerance: ten times what the two f64 references (eigh of A^T A, svd of A) differ by, as a multiple
of eps64 * cond, floored at 1e-11; for f32 the inputs are rounded first, the reference is f64 on the rounded inputs and 8 eps32 is
added for the rounded output.  Every test prints its figures before it asserts."""
import functools

import pytest
import torch

from oracle import cpu_ref as O
from tests import lo_ref
from tests import refit_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
E_TOL = {torch.float64: 1e-6, torch.float32: 1e-4}   # solution sets, as in test_batched_refit_kernels


def _round(t, dt):
    """the values the kernel is handed, as f64"""
    return None if t is None else t.to(dt).double()


def _check_f(F, valid, cases, dt, what):
    """cases: [(label, matches, mask, weights)] in f64, one per pair of the launch"""
    F, valid = F.cpu().double(), valid.cpu()
    bad = []
    for p, (lab, m, k, w) in enumerate(cases):
        Fo, ok, cond, ratio = R.f_refit(_round(m, dt), k, _round(w, dt))
        assert ok, lab
        err, tol = R.rel_err(F[p], Fo), R.f_tolerance(cond, dt)
        print(f"{what} {lab}: ratio {ratio:.3f} cond {cond:.3g} err {err:.3g} tol {tol:.3g}")
        if not (bool(valid[p]) and torch.isfinite(F[p]).all() and err <= tol):
            bad.append((lab, round(ratio, 3), err, tol))
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _sweep():
    cases = R.sweep_cases()
    return cases, torch.stack([m for _, m, _ in cases]), torch.stack([k for _, _, k in cases])


@pytest.mark.parametrize("dt", DTYPES)
def test_f_eigen_gap_sweep(dev, dt):
    """every contaminated selection as one pair of one launch, ragged through the mask"""
    from differentiable_ransac_amd import ops
    cases, m, k = _sweep()
    F, valid = ops.refit_fundamental(m.to(dev, dt), k.to(dev))
    _check_f(F, valid, [(lab, mm, kk, None) for lab, mm, kk in cases], dt, "sweep")


@pytest.mark.parametrize("dt", DTYPES)
def test_f_weighted_sweep(dev, dt):
    """the same selections with row weights 0.2 + 0.8 u, and one pair whose weights span 1e-5 ... 1"""
    from differentiable_ransac_amd import ops
    cases, m, k = _sweep()
    w = R.moderate_weights(len(cases), R.SWEEP_N)
    wm, wk, ww = R.wide_weight_case()
    m, k, w = torch.cat((m, wm[None])), torch.cat((k, wk[None])), torch.cat((w, ww[None]))
    labelled = [("w:" + lab, m[i], k[i], w[i]) for i, (lab, _, _) in enumerate(cases)] + [("wide_weights", wm, wk, ww)]
    F, valid = ops.refit_fundamental(m.to(dev, dt), k.to(dev), w.to(dev, dt))
    _check_f(F, valid, labelled, dt, "weighted")
    # weights of exactly one are the unweighted kernel, bit for bit
    F1, _ = ops.refit_fundamental(m.to(dev, dt), k.to(dev), torch.ones_like(w).to(dev, dt))
    F0, _ = ops.refit_fundamental(m.to(dev, dt), k.to(dev))
    assert torch.equal(F1, F0)


@pytest.mark.parametrize("dt", DTYPES)
def test_f_point_counts(dev, dt):
    """N around the wave (64) and the block (256), no mask; an all-true mask is the same computation, bit for bit"""
    from differentiable_ransac_amd import ops
    for N in (8,) + R.EDGE_NS:
        m = R.clean_pair(11, N, True)[0]
        F, valid = ops.refit_fundamental(m[None].to(dev, dt))
        Fm, vm = ops.refit_fundamental(m[None].to(dev, dt), torch.ones(1, N, dtype=torch.bool, device=dev))
        assert torch.equal(F, Fm) and torch.equal(valid, vm), N
        _check_f(F, valid, [(f"N={N}", m, None, None)], dt, "count")


@pytest.mark.parametrize("dt", DTYPES)
def test_f_mask_layouts(dev, dt):
    """N = 1000, selections confined to one thread, one wave, the last wave's first stride, the last rows; 8 and 9 rows; 7, 4, 0"""
    from differentiable_ransac_amd import ops
    m = R.clean_pair(12, R.LAYOUT_N, True)[0]
    masks = R.layout_masks(8)
    names = list(masks)
    k = torch.stack([masks[n] for n in names])
    F, valid = ops.refit_fundamental(m[None].expand(len(names), -1, -1).contiguous().to(dev, dt), k.to(dev))
    assert torch.isfinite(F).all()
    enough = [i for i, n in enumerate(names) if int(masks[n].sum()) >= 8]
    few = [i for i in range(len(names)) if i not in enough]
    assert {names[i] for i in few} == {"one_thread", "below_min", "none"} and int(masks["below_min"].sum()) == 7
    for i in few:   # below 8 rows: not valid, and exactly the identity
        assert not bool(valid[i]) and torch.equal(F[i].cpu(), torch.eye(3, dtype=dt)), names[i]
    _check_f(F[enough], valid[enough], [("layout:" + names[i], m, masks[names[i]], None) for i in enough], dt, "layout")
    # ten rows, all of them thread 0's (indices = 0 mod 256): every other lane of the block contributes zeros
    ml = R.long_pair()
    kl = torch.arange(R.ONE_THREAD_LONG_N) % 256 == 0
    F, valid = ops.refit_fundamental(ml[None].to(dev, dt), kl[None].to(dev))
    _check_f(F, valid, [("one_thread_long", ml, kl, None)], dt, "layout")


def test_f_exactly_singular_gram_matrix(dev):
    """noise-free inliers in f64: the smallest eigenvalue is zero to rounding; F stays finite and is the ground truth"""
    from differentiable_ransac_amd import ops
    for N in (8, 200):
        m, gt = R.clean_pair(21, N, True, noise=False)
        F, valid = ops.refit_fundamental(m[None].to(dev))
        F = F[0].cpu()
        assert bool(valid[0]) and torch.isfinite(F).all()
        d = float((O.canonical(F) - O.canonical(gt.double())).abs().max())
        print(f"singular N={N}: |F - gt| {d:.3g}")
        assert d < 1e-6, (N, d)


# ------------------------------------------------------------------------------------------------------------ E
def _check_e(E, valid, cases, dt, what):
    bad = []
    for p, (lab, m, k) in enumerate(cases):
        Eo, real = R.e_refit(_round(m, dt), k)
        d, n, no = R.set_distance(E[p], valid[p], Eo, real)
        print(f"{what} {lab}: {n} solutions (reference {no}), worst distance {d:.3g}")
        if not (torch.isfinite(E[p]).all() and n >= 1 and d < E_TOL[dt]):
            bad.append((lab, n, no, d))
    assert not bad, bad


def _invalid_slots_are_identity(E, valid):
    E, valid = E.cpu(), valid.cpu()
    return bool((E[~valid] == torch.eye(3, dtype=E.dtype)).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_e_point_counts(dev, dt):
    from differentiable_ransac_amd import ops
    for N in (5,) + R.EDGE_NS:
        m = R.clean_pair(11, N, False)[0]
        E, valid = ops.refit_essential(m[None].to(dev, dt))
        Em, vm = ops.refit_essential(m[None].to(dev, dt), torch.ones(1, N, dtype=torch.bool, device=dev))
        assert torch.equal(E, Em) and torch.equal(valid, vm), N
        assert _invalid_slots_are_identity(E, valid)
        _check_e(E, valid, [(f"N={N}", m, None)], dt, "count")


@pytest.mark.parametrize("dt", DTYPES)
def test_e_mask_layouts(dev, dt):
    from differentiable_ransac_amd import ops
    m = R.clean_pair(12, R.LAYOUT_N, False)[0]
    masks = R.layout_masks(5)
    names = list(masks)
    k = torch.stack([masks[n] for n in names])
    md = m[None].expand(len(names), -1, -1).contiguous().to(dev, dt)
    E, valid = ops.refit_essential(md, k.to(dev))
    # whatever is selected, fewer than five rows included (the kernel solves what it is given; the drivers never hand it fewer than
    # five rows, see test_local_opt_leaves_pairs_below_the_minimum_alone): finite, and the solver's identity in the unused slots
    assert torch.isfinite(E).all() and _invalid_slots_are_identity(E, valid)
    enough = [i for i, n in enumerate(names) if int(masks[n].sum()) >= 5]
    assert {names[i] for i in range(len(names)) if i not in enough} == {"one_thread", "below_min", "none"}
    _check_e(E[enough], valid[enough], [("layout:" + names[i], m, masks[names[i]]) for i in enough], dt, "layout")
    # exactly five rows: the per-sample minimal solver on the gathered rows
    i = names.index("exactly_min")
    Es, vs = ops.solve_nister5(md[0][masks["exactly_min"].to(dev)][None])
    d, n, ns = R.set_distance(E[i], valid[i], Es[0], vs[0])
    print(f"exactly five rows against solve_nister5: {n} / {ns} solutions, distance {d:.3g}")
    assert n == ns and d < E_TOL[dt]
    ml = R.long_pair_normalised()
    kl = torch.arange(R.ONE_THREAD_LONG_N) % 256 == 0
    E, valid = ops.refit_essential(ml[None].to(dev, dt), kl[None].to(dev))
    _check_e(E, valid, [("one_thread_long", ml, kl)], dt, "layout")


@pytest.mark.parametrize("dt", DTYPES)
def test_e_both_launch_forms(dev, dt):
    """the same 16 pairs as one launch (wave-cooperative final stage) and as two launches of 8 (the light one); half of the pairs
    are selections with outliers: close eigenvalues for the Jacobi"""
    from differentiable_ransac_amd import ops
    cases = R.e_form_cases()
    assert len(cases) == 16
    m = torch.stack([c[1] for c in cases]).to(dev, dt)
    k = torch.stack([c[2] for c in cases]).to(dev)
    E16, v16 = ops.refit_essential(m, k)
    halves = [ops.refit_essential(m[i:i + 8], k[i:i + 8]) for i in (0, 8)]
    E8, v8 = torch.cat([h[0] for h in halves]), torch.cat([h[1] for h in halves])
    assert _invalid_slots_are_identity(E16, v16) and _invalid_slots_are_identity(E8, v8)
    _check_e(E16, v16, cases, dt, "cooperative")
    _check_e(E8, v8, cases, dt, "light")
    for p, (lab, _, _) in enumerate(cases):
        d, a, b = R.set_distance(E16[p], v16[p], E8[p], v8[p])
        print(f"forms {lab}: {a} / {b} solutions, distance {d:.3g}")
        assert a == b and d < E_TOL[dt], (lab, a, b, d)


# ------------------------------------------------------------------------------------------------------------ local optimisation
def _state(dev, dt, m, thr, model, mask):
    """a test-mode state: the given model, ITS MSAC score, the given mask"""
    from differentiable_ransac_amd import ops
    P, N = mask.shape
    st = ops.RansacState(P, N, 5000, dev, dt)
    score = torch.tensor([float(O.msac_score(m[p], model[p:p + 1], float(thr[p]))[0][0]) for p in range(P)], dtype=torch.float64)
    st.best_score.copy_(score.to(dt))
    st.best_model.copy_(model)
    st.best_mask.copy_(mask)
    st.best_inliers.copy_(mask.sum(-1).int())
    st.iters.fill_(16)
    return st, st.best_score.cpu().double()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("lo", [1, 2])
def test_local_opt_from_a_bad_start(dev, lo, dt):
    """F, P = 8, N = 256: the state mask is 60 % inliers + 40 % outliers and the state model a poor one, so the first refit
    runs on close eigenvalues and wins.  The rules and tolerances of test_gpu_local_opt.test_one_launch_matches_the_restatement."""
    from differentiable_ransac_amd import ops
    P, N, lo_iters, k = 8, 256, 8, 7
    pairs = [R.lo_bad_start(400 + p, N) for p in range(P)]
    m = torch.stack([q[0] for q in pairs]).to(dt)
    mask0 = torch.stack([q[1] for q in pairs])
    # 3 px: the pairs' inliers carry about 1 px of noise, and a model refitted on a contaminated mask keeps a few tens of them --
    # at 0.75 px it keeps two to seven, and the f32 MSAC score of so few rows is not good to the 1e-4 asserted below
    thr = torch.stack([torch.tensor(float(O.normalized_threshold(3.0, q[2], q[3], True))) for q in pairs]).to(dt)
    model0 = torch.stack([R.poor_model(q[4], 400 + p) for p, q in enumerate(pairs)]).to(dt)
    st, score0 = _state(dev, dt, m, thr, model0, mask0)
    seen = torch.full((P, 10), float("nan"), device=dev, dtype=dt)
    refits = torch.zeros(P, device=dev, dtype=torch.int32)
    ops.local_optimize(st, m.to(dev), thr.to(dev), True, lo, lo_iters, k, 0.999, 1e-5, 5000, seen, refits)
    torch.cuda.synchronize()
    changed = 0
    for p in range(P):
        ratio = R.f_refit(m[p].double(), mask0[p])[3]
        sc, mk, mo, n = lo_ref.lo_step(m[p].double(), float(thr[p]), True, lo, lo_iters, float(score0[p]), mask0[p],
                                       model0[p].double())
        gs, gm = float(st.best_score[p]), st.best_mask[p].cpu()
        dm = float((O.canonical(st.best_model[p].cpu().double()) - O.canonical(mo.double())).abs().max())
        print(f"lo={lo} pair {p}: first refit at ratio {ratio:.3f}; score {gs:.6g} (restatement {sc:.6g}, start {float(score0[p]):.6g}), "
              f"mask differs in {int((gm != mk).sum())}, model {dm:.3g}, refits {int(refits[p])} ({n})")
        assert abs(gs - sc) <= (1e-4 if dt == torch.float32 else 1e-9) * max(1.0, sc), (p, gs, sc)
        assert int((gm != mk).sum()) <= (1 if dt == torch.float32 else 0), p
        assert int(st.best_inliers[p]) == int(gm.sum())
        assert dm < (1e-4 if dt == torch.float32 else 1e-7), p
        want_mi = min(5000, O.adaptive_iteration_number(int(gm.sum()), N, k, 0.999, max_iterations=5000))
        assert abs(float(st.max_iters[p]) - want_mi) <= 1e-9 * max(1.0, want_mi), p
        assert 1 <= int(refits[p]) <= (1 if lo == 1 else lo_iters)
        if dt == torch.float64:
            assert int(refits[p]) == n, p
        changed += int(not torch.equal(gm, mask0[p]))
        assert torch.equal(seen[p, 0].cpu(), st.best_score[p].cpu())
        assert torch.equal(seen[p, 1:].cpu(), st.best_model[p].reshape(9).cpu())
    assert changed == P             # every refit beat the poor start


@pytest.mark.parametrize("fmat", [False, True])
def test_local_opt_leaves_pairs_below_the_minimum_alone(dev, fmat):
    """the drivers' guard (include/dransac.h, K7b): with fewer than 8 (F) / 5 (E) rows in the mask nothing is refitted"""
    from differentiable_ransac_amd import ops
    kmin, N, dt = (8, 5)[not fmat], R.LAYOUT_N, torch.float64
    m, gt = R.clean_pair(12, N, fmat)
    masks = R.layout_masks(kmin)
    names = ["one_thread", "below_min", "none", "exactly_min"]
    P = len(names)
    mask = torch.stack([masks[n] for n in names])
    mm = m[None].expand(P, -1, -1).contiguous()
    thr = torch.full((P,), 1e-3 if not fmat else 1.0, dtype=dt)
    model = torch.stack([R.poor_model(gt, 7)] * P)
    st, _ = _state(dev, dt, mm, thr, model, mask)
    before = {key: getattr(st, key).clone() for key in ("best_score", "best_model", "best_mask", "best_inliers", "max_iters")}
    seen = torch.full((P, 10), float("nan"), device=dev, dtype=dt)
    refits = torch.zeros(P, device=dev, dtype=torch.int32)
    ops.local_optimize(st, mm.to(dev), thr.to(dev), fmat, 2, 4, 7 if fmat else 5, 0.999, 1e-5, 5000, seen, refits)
    torch.cuda.synchronize()
    assert refits.cpu().tolist()[:3] == [0, 0, 0] and int(refits[3]) >= 1
    for key, v in before.items():
        assert torch.equal(getattr(st, key)[:3], v[:3]), key
    assert torch.isfinite(st.best_model).all() and torch.isfinite(st.best_score).all()
