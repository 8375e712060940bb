"""The absolute-pose kernels (csrc/pnp.hip) and ransac.BatchedPnP against the f64 reference tests/pnp_ref.py, in f32 and f64.
Every tolerance is TOL_FACTOR = 8 times a figure the reference measures on itself (pnp_ref's docstring): its run on inputs as the kernel
receives them, its result rounded as the kernel's is, against its run on the f64 originals -- never anything a kernel returned.  The
measured figures are printed next to each bound; docs/LOG.md records them."""
import functools
import math

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import ops, synth
from differentiable_ransac_amd.ops import L, ptr, stream
from differentiable_ransac_amd.ransac import BatchedPnP
from tests import pnp_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.float64]
THR = R.THRESHOLD
F = R.TOL_FACTOR
KEYS = {"model", "mask", "score", "inliers", "iterations"}


def _name(dt):
    return "float32" if dt == torch.float32 else "float64"


def _dev(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dt is None else t.to(dt)


def _np(t):
    return t.double().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _given(a, name):
    """what a kernel of type `name` is handed, in f64: the f32 rounding, or the f64 values themselves"""
    return a.astype(np.float32).astype(np.float64) if name == "float32" else a


def _pair_up(ref, got):
    """the rotation distances of the one-to-one nearest-rotation matching of two solution sets of equal size -> [(i, j)]"""
    left, out = list(range(len(got))), []
    for i, s in enumerate(ref):
        j = min(left, key=lambda q: R.rot_angle(s[:3, :3], got[q][:3, :3]))
        left.remove(j)
        out.append((i, j))
    return out


# ---- 1. solver -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solver_ref(case, name):
    """per pair the reference slots on the inputs the kernel is given; the samples it leaves out; and the measured figures: the largest
    rotation / translation deviation and the largest sample residual of the reference on as_kernel_input inputs, its poses rounded the
    same way, against its f64 run"""
    m, idx = R.solver_case(*case)
    mg, mk = _given(m, name), R.as_kernel_input(m, name, 1)
    ref, fig_a, fig_t, fig_r, skipped, total = [], 0.0, 0.0, 0.0, 0, 0
    for p in range(case[0]):
        mo, va, infos = R.slots(mg[p], idx[p])
        mo2, va2, infos2 = R.slots(mk[p], idx[p])
        keep = np.array([R.comparable(a) and R.comparable(b) for a, b in zip(infos, infos2)])
        skipped, total = skipped + int((~keep).sum()), total + len(keep)
        for b in np.flatnonzero(keep):
            a, c = mo[4 * b:4 * b + 4][va[4 * b:4 * b + 4]], mo2[4 * b:4 * b + 4][va2[4 * b:4 * b + 4]]
            assert len(a) == len(c), (p, b)           # (the separation rule is what makes the reference's own count stable)
            for i, j in _pair_up(a, c):
                cj = R.as_kernel_input(c[j], name, 2)
                ea, et = R.pose_error(a[i], cj)
                fig_a, fig_t = max(fig_a, ea), max(fig_t, et)
                fig_r = max(fig_r, math.sqrt(R.residual(mg[p][idx[p][b]], cj)[0].max()))
        ref.append((mo, va, keep))
    return m, idx, ref, (fig_a, fig_t, fig_r), skipped, total


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", R.GPU_CASES, ids=[f"P{c[0]}-N{c[1]}-B{c[2]}" for c in R.GPU_CASES])
def test_solver_matches_the_reference(case, dt):
    name = _name(dt)
    m, idx, ref, (fig_a, fig_t, fig_r), skipped, total = _solver_ref(case, name)
    assert skipped <= max(R.EXCLUDED_MAX * total, 0), (skipped, total)
    tm, ti = _dev(m, dt), _dev(idx)
    models, valid = ops.p3p_gather(tm, ti)
    again = ops.p3p_gather(tm, ti)
    assert torch.equal(_bytes(models), _bytes(again[0])) and torch.equal(valid, again[1])          # a repeated launch: the same bytes
    assert models.shape == (case[0], 4 * case[2], 4, 4) and valid.shape == (case[0], 4 * case[2]) and valid.dtype == torch.bool
    mk, vk, mg = _np(models), valid.cpu().numpy(), _given(m, name)
    e = R.eps_of(name)
    worst = [0.0, 0.0, 0.0]
    for p, (mo, va, keep) in enumerate(ref):
        assert np.array_equal(mk[p][~vk[p]], np.broadcast_to(np.eye(4), mk[p][~vk[p]].shape))   # every invalid slot is the identity
        for b in range(case[2]):
            got_v = vk[p, 4 * b:4 * b + 4]
            assert np.array_equal(got_v, np.sort(got_v)[::-1]), (p, b)                            # the valid slots come first
            got = mk[p, 4 * b:4 * b + 4][got_v]
            # the contract, of every valid slot.  R = sum_k e'_k e_k^T of two frames whose vectors have unit norm to 2 eps each and
            # are orthogonal to 2 eps (the second Gram-Schmidt pass): an entry of R R^T - I collects (2 + 2 + 2) eps per frame, 3 eps from
            # the products and 2 eps from storing R in the type -- 17 eps; 32 eps is allowed
            for T in got:
                assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() <= 32 * e and np.linalg.det(T[:3, :3]) > 0
                assert np.array_equal(T[3], [0, 0, 0, 1])
                d2, front = R.residual(mg[p][idx[p][b]], T)
                assert front.all(), (p, b)
            if not keep[b]:
                continue
            want = mo[4 * b:4 * b + 4][va[4 * b:4 * b + 4]]
            assert len(got) == len(want), (p, b, len(got), len(want))
            for i, j in _pair_up(want, got):
                ea, et = R.pose_error(want[i], got[j])
                er = math.sqrt(R.residual(mg[p][idx[p][b]], got[j])[0].max())
                worst = [max(worst[0], ea), max(worst[1], et), max(worst[2], er)]
                assert ea <= F * fig_a and et <= F * fig_t and er <= F * fig_r, (p, b, ea, et, er)
    print(f"solver {case} {name}: rotation {worst[0]:.3g} (measured {fig_a:.3g}, bound {F * fig_a:.3g}), translation {worst[1]:.3g} "
          f"(measured {fig_t:.3g}, bound {F * fig_t:.3g}), sample residual {worst[2]:.3g} (measured {fig_r:.3g}, bound {F * fig_r:.3g}); "
          f"left out {skipped} of {total}")


@pytest.mark.parametrize("dt", DTYPES)
def test_solver_degenerate_samples_have_four_invalid_identity_slots(dt):
    m = R.scene(2, 16, 1.0)["matches"].copy()
    m[2, :3] = m[0, :3] + 2.0 * (m[1, :3] - m[0, :3])        # rows 0, 1, 2: collinear world points
    m[4, 3:] = m[3, 3:]                                      # rows 3, 4: coincident bearings
    idx = np.array([[[0, 1, 2], [5, 6, 6], [3, 4, 7], [8, 9, 10], [0, 1, 99], [-1, 2, 3]]], np.int32)
    models, valid = ops.p3p_gather(_dev(m[None], dt), _dev(idx))
    vk, mk = valid.cpu().numpy()[0].reshape(6, 4), _np(models)[0].reshape(6, 4, 4, 4)
    assert not vk[[0, 1, 2, 4, 5]].any() and vk[3].any()
    assert np.array_equal(mk[[0, 1, 2, 4, 5]], np.broadcast_to(np.eye(4), (5, 4, 4, 4)))


# ---- 2. score ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _score_ref(N, name):
    """the case, the reference's scores and counts on the f64 originals, the measured score figure per pair, and per slot the number of
    points inside the band a relative d2 error of `width` can turn: width = TOL_FACTOR x the largest |d2' - d2| / thr^2 between the two
    reference runs over the points with d2 < 4 thr^2"""
    m, models, valid, poses = R.score_case(N)
    mk, ok = R.as_kernel_input(m, name, 3), R.as_kernel_input(models, name, 4)
    want, figs, width = [], [], 0.0
    for p in range(len(m)):
        s0, n0 = R.score_all(m[p], models[p], valid[p], THR)
        s1, _ = R.score_all(mk[p], ok[p], valid[p], THR)
        good = np.isfinite(s0)
        figs.append(float(np.abs(s1 - s0)[good].max()))
        for j in np.flatnonzero(valid[p] & good):
            a, b = R.residual(m[p], models[p, j])[0], R.residual(mk[p], ok[p, j])[0]
            near = a < 4 * THR * THR
            if near.any():
                width = max(width, float(np.abs(a - b)[near].max()) / (THR * THR))
        want.append((s0, n0))
    width *= F
    bands = [R.band_counts(m[p], models[p], valid[p], THR, width) for p in range(len(m))]
    return m, models, valid, want, figs, bands, width


def _score_raw(tm, tmo, tv, thr2, scores, inliers, gate=None):
    P, N, _ = tm.shape
    g = (ptr(None), ptr(None)) if gate is None else (ptr(gate.iters), ptr(gate.max_iters))
    L.call(f"dr_pnp_score_{L.suffix(tm.dtype)}", ptr(tm), ptr(tmo), ptr(tv.view(torch.uint8)), ptr(thr2), P, tmo.shape[1], N,
           ptr(scores), ptr(inliers), *g, stream())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", R.SCORE_N)
def test_score_matches_the_reference(N, dt):
    name = _name(dt)
    m, models, valid, want, figs, bands, width = _score_ref(N, name)
    tm, tmo, tv = _dev(m, dt), _dev(models, dt), _dev(valid)
    scores, inl = ops.pnp_score(tm, tmo, THR, valid=tv)
    s2, i2 = ops.pnp_score(tm, tmo, THR, valid=tv)
    assert torch.equal(_bytes(scores), _bytes(s2)) and torch.equal(inl, i2)
    assert scores.shape == (3, R.M_SLOTS) and inl.dtype == torch.int32
    sk, ik = _np(scores), inl.cpu().numpy()
    worst = 0.0
    for p, (s0, n0) in enumerate(want):
        assert (sk[p][~valid[p]] == 0.0).all() and (ik[p][~valid[p]] == 0).all()                 # invalid slots: exactly 0
        assert math.isnan(sk[p, 130]) and ik[p, 130] == 0                                        # a NaN model scores NaN
        good = valid[p] & np.isfinite(s0)
        # a point inside the band may fall on either side: it moves the count by one and the score by at most `width`
        err = np.abs(sk[p] - s0)[good]
        tol = F * max(figs) + bands[p][good] * width              # the case's figure: the largest of its pairs
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all(), (p, err.max(), figs[p])
        assert (np.abs(ik[p] - n0)[good] <= bands[p][good]).all(), (p, np.abs(ik[p] - n0)[good].max())
        assert s0[128] > 0.3 * N * 0.6                                                           # the generating pose scores (sanity)
    print(f"score N={N} {name}: worst error / bound {worst:.3f}; measured score figures {[f'{x:.3g}' for x in figs]}, bound "
          f"{F}x; band width {width:.3g}, largest band {max(int(b.max()) for b in bands)} points")
    # the point behind the camera (last row; d2 = 0 under slot 128) adds nothing: a far outlier in its place gives the same bytes
    moved = tm.clone()
    moved[:, -1, 3:] += 1.0
    s3, i3 = ops.pnp_score(moved, tmo, THR, valid=tv)
    assert torch.equal(_bytes(s3[:, 128]), _bytes(scores[:, 128])) and torch.equal(i3[:, 128], inl[:, 128])
    assert bool((inl[:, 128] <= N - 1).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_score_gate_keeps_the_rows_of_a_closed_pair(dt):
    m, models, valid, *_ = _score_ref(300, _name(dt))
    tm, tmo, tv = _dev(m, dt), _dev(models, dt), _dev(valid)
    thr2 = ops.thr2_tensor(THR, 3, tm)
    st = ops.PnPState(3, 300, 100, DEV, dt)
    st.iters[1] = 100                                        # pair 1 has terminated
    open_s, open_i = ops.pnp_score(tm, tmo, THR, valid=tv)
    scores = torch.full((3, R.M_SLOTS), -7.0, device=DEV, dtype=dt)
    inl = torch.full((3, R.M_SLOTS), -7, device=DEV, dtype=torch.int32)
    _score_raw(tm, tmo, tv, thr2, scores, inl, st)
    assert bool((scores[1] == -7.0).all()) and bool((inl[1] == -7).all())
    assert torch.equal(_bytes(scores[[0, 2]]), _bytes(open_s[[0, 2]])) and torch.equal(inl[[0, 2]], open_i[[0, 2]])
    gated = ops.pnp_score(tm, tmo, THR, valid=tv, gate=ops.PnPState(3, 300, 100, DEV, dt))       # an open gate changes nothing
    assert torch.equal(_bytes(gated[0]), _bytes(open_s))


# ---- 3. update ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_update_follows_the_reference_state_step(dt):
    name = _name(dt)
    P, N, B, MI = 3, 300, 33, 5000
    m = np.stack([R.scene(70 + p, N, s)["matches"] for p, s in enumerate((0.6, 0.3, 0.6))])
    mg, tm = _given(m, name), _dev(m, dt)
    rng = np.random.default_rng(9)
    st = ops.PnPState(P, N, MI, DEV, dt)
    st.iters[2] = 64
    st.max_iters[2] = 60.0                                   # pair 2 terminated in advance: untouched, iters included
    ref = [R.new_state(N, MI) for _ in range(P)]
    ref[2].update(iters=64, max_iters=60.0)
    _, _, _, _, _, _, width = _score_ref(300, name)          # the band of the inlier decision, measured by the reference
    want = [float(MI), float(MI), 60.0]
    for r in range(3):
        idx = np.stack([np.stack([rng.permutation(N)[:3] for _ in range(B)]) for _ in range(P)]).astype(np.int32)
        models, valid = ops.p3p_gather(tm, _dev(idx))
        scores, _ = ops.pnp_score(tm, models, THR, valid=valid)
        ops.pnp_update(st, tm, models, valid, scores, THR, B)
        mk, vk, sk = _np(models), valid.cpu().numpy(), _np(scores)
        for p in range(P):
            before = ref[p]["score"]
            R.step(ref[p], mg[p], mk[p], vk[p], sk[p], THR, B, max_iterations=MI)
            assert int(st.iters[p]) == ref[p]["iters"]
            assert np.array_equal(_np(st.best_model[p]), ref[p]["model"]) and float(st.best_score[p]) == ref[p]["score"]
            mask = st.best_mask[p].cpu().numpy()
            assert int(st.best_inliers[p]) == int(mask.sum())
            d2, _ = R.residual(mg[p], ref[p]["model"])
            off = mask != ref[p]["mask"]                     # only points inside the band may sit on the other side
            assert (np.abs(d2[off] / (THR * THR) - 1.0) <= width).all(), (r, p, int(off.sum()))
            if ref[p]["score"] != before:                    # replaced this round: the bound of the mask's own count, in f64
                want[p] = R.adaptive_max_iters(int(mask.sum()), N, 3, 0.999, 1e-5, MI)
            assert abs(float(st.max_iters[p]) - want[p]) <= 1e-12 * want[p], (r, p)
            ref[p].update(max_iters=float(st.max_iters[p]), inliers=int(mask.sum()), mask=mask)       # (a band point: follow the device)
    assert float(st.best_score[2]) == 0.0 and not bool(st.best_mask[2].any())
    assert int(st.best_inliers[0]) > 100


# ---- 4. refit ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _refit_ref(N, name):
    """three pairs: scene, inlier mask, perturbed start; the reference's result on the f64 originals; the measured figures: its run on
    as_kernel_input inputs with its pose rounded the same way, and its run with twice the passes (its own convergence error)"""
    rng = np.random.default_rng(N)
    out = []
    for p in range(3):
        sc = R.scene(80 + N + p, N, 0.6)
        m, rows = sc["matches"], sc["inlier"]
        T0 = R.perturbed(sc["pose"], rng)
        Tr, ok, cost = R.lm_refit(m, rows, T0, 10)
        T1 = R.as_kernel_input(R.lm_refit(R.as_kernel_input(m, name, 5), rows, R.as_kernel_input(T0, name, 6), 10)[0], name, 7)
        T2, _, cost2 = R.lm_refit(m, rows, T0, 20)
        fa, ft = (max(x) for x in zip(R.pose_error(Tr, T1), R.pose_error(Tr, T2)))
        fc = max(abs(R.cost_over(m, rows, T1) - cost), abs(cost2 - cost))
        assert ok
        out.append(dict(m=m, rows=rows, T0=T0, Tr=Tr, cost=cost, fig=(fa, ft, fc)))
    return out


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", R.SCORE_N)
def test_refit_matches_the_reference(N, dt):
    name = _name(dt)
    ref = _refit_ref(N, name)
    tm = _dev(np.stack([r["m"] for r in ref]), dt)
    mask, init = _dev(np.stack([r["rows"] for r in ref])), _dev(np.stack([r["T0"] for r in ref]), dt)
    model, valid = ops.refit_pnp(tm, mask, init, 10)
    again = ops.refit_pnp(tm, mask, init, 10)
    assert torch.equal(_bytes(model), _bytes(again[0])) and torch.equal(valid, again[1]) and bool(valid.all())
    fa, ft, fc = (max(r["fig"][q] for r in ref) for q in range(3))          # the case's figures: the largest of its pairs
    for p, r in enumerate(ref):
        T = _np(model[p])
        ea, et = R.pose_error(T, r["Tr"])
        cost = R.cost_over(r["m"], r["rows"], T)
        print(f"refit N={N} {name} pair {p}: rotation {ea:.3g} (measured {fa:.3g}, bound {F * fa:.3g}), translation {et:.3g} (measured "
              f"{ft:.3g}, bound {F * ft:.3g}), cost {cost:.9g} against {r['cost']:.9g} (measured {fc:.3g}, margin {F * fc:.3g})")
        assert cost <= r["cost"] + F * fc
        assert ea <= F * fa and et <= F * ft
    # iters = 0 returns the start; fewer than three rows and a NaN start are invalid identities
    same, v0 = ops.refit_pnp(tm, mask, init, 0)
    assert torch.equal(_bytes(same), _bytes(init)) and bool(v0.all())
    few = torch.zeros_like(mask)
    few[:, :2] = True
    few[2, :3] = True
    bad = init.clone()
    bad[1, 0, 0] = float("nan")
    mo, va = ops.refit_pnp(tm, few, init, 10)
    assert va.cpu().tolist() == [False, False, True] and torch.equal(mo[:2], torch.eye(4, device=DEV, dtype=dt).expand(2, 4, 4))
    mo, va = ops.refit_pnp(tm, mask, bad, 10)
    assert va.cpu().tolist() == [True, False, True] and torch.equal(mo[1], torch.eye(4, device=DEV, dtype=dt))


# ---- 5. driver ---------------------------------------------------------------------------------------------------------------------------
def _driver(**kw):
    D = R.DRV
    return BatchedPnP(ransac_batch_size=D["B"], threshold=THR, max_iterations=D["max_iterations"], **kw)


@functools.lru_cache(maxsize=None)
def _driver_inputs():
    D = R.DRV
    sc = R.driver_scenes()
    rounds = math.ceil(D["max_iterations"] / D["B"])
    noise = [synth.gumbel_noise((D["P"], D["B"], D["N"]), seed=1000 + r, dtype=torch.float64) for r in range(rounds)]
    return sc, np.stack([s["matches"] for s in sc]), noise


@pytest.mark.parametrize("dt", DTYPES)
def test_driver(dt):
    D = R.DRV
    P, N, B = D["P"], D["N"], D["B"]
    sc, m, noise = _driver_inputs()
    tm, logits, g = _dev(m, dt), torch.zeros(P, N, device=DEV, dtype=dt), [x.to(DEV, dt) for x in noise]
    out = _driver()(tm, logits, gumbels=g)
    assert set(out) == KEYS
    assert out["model"].shape == (P, 4, 4) and out["model"].dtype == dt and out["score"].shape == (P,) and out["score"].dtype == dt
    assert out["mask"].shape == (P, N) and out["mask"].dtype == torch.bool
    assert out["inliers"].shape == (P,) and out["inliers"].dtype == torch.int32 and out["iterations"].dtype == torch.int32
    its = out["iterations"].cpu().tolist()
    assert all(i % B == 0 and B <= i <= D["max_iterations"] for i in its) and len(set(its)) == 3, its     # three different rounds
    assert torch.equal(out["inliers"].long(), out["mask"].sum(1))
    # the 70 % pair against the generating pose: five first-order standard deviations of the least-squares pose under the image noise
    srot, strans = R.pose_sigma(m[2], sc[2]["inlier"], sc[2]["pose"], R.NOISE)
    ea, et = R.pose_error(_np(out["model"][2]), sc[2]["pose"])
    print(f"driver {_name(dt)}: iterations {its}, inliers {out['inliers'].cpu().tolist()}; 70 % pair: {ea:.3g} rad (sigma {srot:.3g}), "
          f"{et:.3g} (sigma {strans:.3g})")
    assert ea <= 5 * srot and et <= 5 * strans
    assert int(out["inliers"][2]) >= 0.9 * int(sc[2]["inlier"].sum())
    # refit = False returns the state's model; the refit only ever raises the score, and never touches mask or counters
    plain = _driver(refit=False)(tm, logits, gumbels=g)
    assert bool((plain["score"] <= out["score"]).all())
    for k in ("mask", "inliers", "iterations"):
        assert torch.equal(plain[k], out[k])
    idx = [ops.gumbel_topk(logits, B, 3, 1.0, x, 0, soft=False)["idx"] for x in g]
    st = ops.PnPState(P, N, D["max_iterations"], DEV, dt)
    for i in idx[:max(its) // B]:
        models, valid = ops.p3p_gather(tm, i)
        ops.pnp_update(st, tm, models, valid, ops.pnp_score(tm, models, THR, valid=valid)[0], THR, B)
    assert torch.equal(_bytes(plain["model"]), _bytes(st.best_model)) and torch.equal(plain["iterations"], st.iters)
    # device_termination: every round issued, gated on the device -- the host loop's bytes
    d = _driver()
    d.device_termination = True
    gated = d(tm, logits, gumbels=g)
    assert all(torch.equal(_bytes(gated[k]), _bytes(out[k])) for k in KEYS)


@pytest.mark.parametrize("dt", DTYPES)
def test_driver_seeded_and_prosac(dt):
    D = R.DRV
    P, N, B = D["P"], D["N"], D["B"]
    sc, m, _ = _driver_inputs()
    tm = _dev(m, dt)
    logits = torch.zeros(P, N, device=DEV, dtype=dt)
    a, b = _driver(seed=3)(tm, logits), _driver(seed=3)(tm, logits)
    assert all(torch.equal(_bytes(a[k]), _bytes(b[k])) for k in KEYS)
    # PROSAC on logits that rank the inliers first, 70 % inliers in every pair: the first round finds the model and its bound ends the call
    easy = [R.scene(300 + p, N, 0.7) for p in range(P)]
    te = _dev(np.stack([s["matches"] for s in easy]), dt)
    ranked = _dev(np.stack([np.where(s["inlier"], 5.0, -5.0) + 1e-3 * np.arange(N)[::-1] for s in easy]), dt)
    out = _driver(sampling="prosac", seed=3)(te, ranked)
    assert out["iterations"].cpu().tolist() == [B] * P, out["iterations"].cpu().tolist()
    for p in range(P):
        assert int(out["inliers"][p]) >= 0.9 * int(easy[p]["inlier"].sum()), (p, int(out["inliers"][p]))
        srot, strans = R.pose_sigma(easy[p]["matches"], easy[p]["inlier"], easy[p]["pose"], R.NOISE)
        ea, et = R.pose_error(_np(out["model"][p]), easy[p]["pose"])
        assert ea <= 5 * srot and et <= 5 * strans, (p, ea, srot, et, strans)
    with pytest.raises(ValueError, match="prosac"):
        _driver(sampling="prosac")(te, ranked, gumbels=[ranked])
