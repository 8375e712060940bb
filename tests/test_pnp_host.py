"""The absolute-pose path without a GPU: the properties of the reference tests/pnp_ref.py, the conditions on the reference's side that
tests/test_gpu_pnp.py rests on (its caps and seeds were chosen here), the ABI of the four entries (declared, exported, DR_EINVAL before
any device work), the wrappers' refusals and the constructor checks of BatchedPnP."""
import ctypes
import math

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from tests import pnp_ref as R

SYMBOLS = [f"dr_{n}_{s}" for n in ("p3p_gather", "pnp_score", "pnp_update", "refit_pnp") for s in ("f32", "f64")]
THR = R.THRESHOLD


# ------------------------------------------------------------------------------------------------ the reference alone
def test_p3p_recovers_the_generating_pose_on_noise_free_samples():
    sc = R.scene(1, 200, 1.0, noise=0.0)
    m, T = sc["matches"], sc["pose"]
    rng = np.random.default_rng(0)
    worst = worst_res = 0.0
    for _ in range(200):
        idx = rng.permutation(200)[:3]
        sol, info = R.p3p(m[idx])
        assert 1 <= len(sol) <= 4
        for s in sol:                                   # every solution reprojects its own sample exactly, in front of the camera
            d2, ok = R.residual(m[idx], s)
            assert ok.all()
            worst_res = max(worst_res, float(d2.max()))
            assert abs(np.linalg.det(s[:3, :3]) - 1.0) < 1e-12 and np.abs(s[:3, :3] @ s[:3, :3].T - np.eye(3)).max() < 1e-12
        if R.comparable(info):
            worst = max(worst, min(sum(R.pose_error(s, T)) for s in sol))
    print(f"largest distance of the closest solution from the generating pose {worst:.3g}, largest sample d2 {worst_res:.3g}")
    assert worst < 1e-8 and worst_res < 1e-20


def test_p3p_degenerate_samples_have_no_solution():
    m = R.scene(2, 16, 1.0)["matches"]
    col = m[:3].copy()
    col[2, :3] = col[0, :3] + 2.0 * (col[1, :3] - col[0, :3])                # collinear world points
    same = m[[0, 1, 1]]                                                       # a repeated index
    ray = m[:3].copy()
    ray[1, 3:] = ray[0, 3:]                                                   # coincident bearings
    for s in (col, same, ray):
        sol, info = R.p3p(s)
        assert len(sol) == 0 and info["tri"] == 0.0 and R.comparable(info)


@pytest.mark.parametrize("case", R.GPU_CASES)
def test_the_solver_cases_stay_inside_the_exclusion_cap(case):
    m, idx = R.solver_case(*case)
    infos = [i for p in range(case[0]) for i in R.slots(m[p], idx[p])[2]]
    out = sum(not R.comparable(i) for i in infos)
    print(f"{case}: {out} of {len(infos)} samples left out")
    assert out <= R.EXCLUDED_MAX * len(infos) or (len(infos) == 1 and out == 0)


def test_score_rules():
    sc = R.scene(3, 50, 1.0, noise=0.0)
    m, T = sc["matches"].copy(), sc["pose"]
    s, n = R.msac(m, T, THR)
    assert n == 50 and abs(s - 50.0) < 1e-9
    xc = -2.0 * np.array([m[0, 3], m[0, 4], 1.0])                              # on the ray of its observation, behind the camera
    m[0, :3] = T[:3, :3].T @ (xc - T[:3, 3])
    assert R.residual(m, T)[0][0] < 1e-20 and not R.residual(m, T)[1][0]
    m[1, 4] = np.nan
    s, n = R.msac(m, T, THR)
    assert n == 48 and abs(s - 48.0) < 1e-9
    assert math.isnan(R.msac(m, np.full((4, 4), np.nan), THR)[0]) and R.msac(m, np.full((4, 4), np.nan), THR)[1] == 0
    sco, inl = R.score_all(m, np.stack([T, T]), np.array([True, False]), THR)
    assert sco[1] == 0.0 and inl[1] == 0 and inl[0] == 48


def test_state_step_rules():
    sc = R.scene(4, 100, 0.5)
    m, T = sc["matches"], sc["pose"]
    far = R.perturbed(T, np.random.default_rng(0), 20.0, 0.3)
    models, valid = np.stack([far, T, T, np.full((4, 4), np.nan)]), np.array([True, True, True, True])
    scores = R.score_all(m, models, valid, THR)[0]
    st = R.step(R.new_state(100, 5000), m, models, valid, scores, THR, 64)
    assert st["iters"] == 64 and np.array_equal(st["model"], T) and st["inliers"] == 50 == int(st["mask"].sum())     # the FIRST arg-max
    assert st["max_iters"] == R.adaptive_max_iters(50, 100, 3, 0.999, 1e-5, 5000) < 64
    before = dict(st)
    R.step(st, m, models, valid, scores, THR, 64)                             # terminated: untouched, iters included
    assert st["iters"] == 64 and st["score"] == before["score"]
    st = R.new_state(100, 5000)
    st["score"] = scores[1]
    R.step(st, m, models, valid, scores, THR, 64)                             # an equal score does not replace
    assert st["inliers"] == 0 and st["iters"] == 64
    st = R.step(R.new_state(100, 5000), m, models, np.zeros(4, bool), scores, THR, 64)
    assert st["score"] == 0.0 and st["iters"] == 64                           # no valid slot: only iters moves


@pytest.mark.parametrize("N", R.SCORE_N)
def test_lm_refit_lowers_the_cost_and_converges(N):
    sc = R.scene(40 + N, N, 0.6)
    m, T, rows = sc["matches"], sc["pose"], sc["inlier"]
    T0 = R.perturbed(T, np.random.default_rng(N))
    Tr, ok, cost = R.lm_refit(m, rows, T0, 10)
    assert ok and cost < R.cost_over(m, rows, T0) and cost <= R.cost_over(m, rows, T) * (1 + 1e-9)
    T2, _, cost2 = R.lm_refit(m, rows, T0, 20)
    da, dt = R.pose_error(Tr, T2)
    print(f"N={N}: cost {R.cost_over(m, rows, T0):.4g} -> {cost:.6g}; 10 vs 20 passes: {da:.3g} rad, {dt:.3g}, cost {cost - cost2:.3g}")
    assert da < 1e-9 and dt < 1e-9
    assert R.lm_refit(m, np.arange(N) < 2, T0, 10)[1] is False               # fewer than three rows
    assert R.lm_refit(m, rows, np.full((4, 4), np.nan), 10)[1] is False


def test_the_driver_case_stops_its_pairs_in_three_different_rounds():
    from differentiable_ransac_amd import synth
    D = R.DRV
    rounds = math.ceil(D["max_iterations"] / D["B"])
    noise = [synth.gumbel_noise((D["P"], D["B"], D["N"]), seed=1000 + r, dtype=torch.float64) for r in range(rounds)]
    idx = [torch.topk(x, 3, dim=-1).indices.numpy() for x in noise]          # what the sampler returns for zero logits
    out = [R.run(sc["matches"], [i[p] for i in idx], THR, D["B"], D["max_iterations"]) for p, sc in enumerate(R.driver_scenes())]
    print([(o["rounds"], o["inliers"], o["iterations"]) for o in out])
    assert len({o["rounds"] for o in out}) == 3 and all(o["iterations"] % D["B"] == 0 for o in out)
    sc = R.driver_scenes()[2]
    srot, st = R.pose_sigma(sc["matches"], sc["inlier"], sc["pose"], R.NOISE)
    ea, et = R.pose_error(out[2]["model"], sc["pose"])
    print(f"70 % pair: {ea:.3g} rad (sigma {srot:.3g}), {et:.3g} (sigma {st:.3g})")
    assert ea <= 5 * srot and et <= 5 * st


# ------------------------------------------------------------------------------------------------ library, wrappers, driver
def test_header_declares_and_library_exports_the_entries():
    declared = set(L.entries())
    assert not [s for s in SYMBOLS if s not in declared]
    lib = L.lib()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]


def test_entries_refuse_bad_arguments_without_a_gpu():
    lib = L.lib()
    buf = (ctypes.c_char * 256)()
    for sfx in ("f32", "f64"):
        gather = getattr(lib, "dr_p3p_gather_" + sfx)

        def call_gather(matches=buf, idx=buf, P=1, B=1, N=3, models=buf, valid=buf):
            return gather(matches, idx, P, B, N, models, valid, None)

        for name in ("matches", "idx", "models", "valid"):
            assert call_gather(**{name: None}) == -1 and b"null" in lib.dr_last_error(), name
        for kw in (dict(P=0), dict(B=0), dict(N=-1), dict(P=1 << 15, B=1 << 15)):
            assert call_gather(**kw) == -1 and b"dr_p3p_gather" in lib.dr_last_error(), kw
        score = getattr(lib, "dr_pnp_score_" + sfx)

        def call_score(matches=buf, models=buf, thr2=buf, P=1, M=1, N=1, scores=buf, gi=None, gm=None):
            return score(matches, models, None, thr2, P, M, N, scores, None, gi, gm, None)

        for name in ("matches", "models", "thr2", "scores"):
            assert call_score(**{name: None}) == -1 and b"null" in lib.dr_last_error(), name
        for kw in (dict(P=0), dict(M=0), dict(N=-1), dict(P=65536)):
            assert call_score(**kw) == -1 and b"dr_pnp_score" in lib.dr_last_error(), kw
        assert call_score(gi=buf) == -1 and b"gate" in lib.dr_last_error()
        update = getattr(lib, "dr_pnp_update_" + sfx)
        names = ("matches", "models", "scores", "thr2", "best_score", "best_model", "best_mask", "best_inliers", "iters", "max_iters")

        def call_update(P=1, M=4, N=1, B=1, max_iterations=10, **kw):
            a = {n: kw.get(n, buf) for n in names}
            return update(a["matches"], a["models"], None, a["scores"], a["thr2"], P, M, N, B, 0.999, 1e-5, max_iterations,
                          a["best_score"], a["best_model"], a["best_mask"], a["best_inliers"], a["iters"], a["max_iters"], None)

        for name in names:
            assert call_update(**{name: None}) == -1 and b"null" in lib.dr_last_error(), name
        for kw in (dict(P=0), dict(M=0), dict(N=0), dict(B=0), dict(max_iterations=0)):
            assert call_update(**kw) == -1 and b"dr_pnp_update" in lib.dr_last_error(), kw
        refit = getattr(lib, "dr_refit_pnp_" + sfx)

        def call_refit(matches=buf, init=buf, P=1, N=3, iters=1, model=buf, valid=buf):
            return refit(matches, None, init, P, N, iters, model, valid, None)

        for name in ("matches", "init", "model", "valid"):
            assert call_refit(**{name: None}) == -1 and b"null" in lib.dr_last_error(), name
        for kw in (dict(P=0), dict(N=0), dict(iters=-1)):
            assert call_refit(**kw) == -1 and b"dr_refit_pnp" in lib.dr_last_error(), kw


def test_constructor_checks():
    from differentiable_ransac_amd import BatchedPnP, ransac
    d = BatchedPnP()
    assert (d.k, d.B, d.threshold, d.refit, d.refit_iters, d.sampling, d.scoring, d.lo, d.train) == \
        (3, 1024, 0.005, True, 10, "gumbel", "msac", 0, False)
    assert d.rounds == 5 and BatchedPnP is ransac.BatchedPnP and BatchedPnP._State.__name__ == "PnPState"
    for kw in (dict(train=True), dict(scoring="magsac"), dict(lo=1), dict(lo=2)):
        with pytest.raises(NotImplementedError, match="DESIGN.md"):
            BatchedPnP(**kw)
    for kw in (dict(sampling="uniform"), dict(max_iterations=0), dict(ransac_batch_size=0), dict(refit_iters=-1), dict(refit_iters=2.5),
               dict(refit_iters=True)):
        with pytest.raises(ValueError):
            BatchedPnP(**kw)
    assert BatchedPnP(sampling="prosac", prosac_draws=1000).sampling == "prosac" and BatchedPnP(refit_iters=0).refit_iters == 0
    d = BatchedPnP(ransac_batch_size=64, max_iterations=256)
    d.device_termination = True
    assert d.device_termination
    with pytest.raises(ValueError, match="16 rounds"):
        BatchedPnP(ransac_batch_size=64, max_iterations=5000).device_termination = True
    with pytest.raises(ValueError, match=r"\[P,N,5\]"):
        d(torch.rand(2, 16, 4), torch.zeros(2, 16))


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes(monkeypatch):
    from differentiable_ransac_amd import ops
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    m, idx, mo = torch.rand(2, 16, 5), torch.zeros(2, 4, 3, dtype=torch.int32), torch.rand(2, 16, 4, 4)
    st = ops.PnPState(2, 16, 100, "cpu", torch.float32)
    assert st.best_model.shape == (2, 4, 4)
    for fn in (lambda: ops.p3p_gather(m, idx), lambda: ops.pnp_score(m, mo, THR), lambda: ops.refit_pnp(m, None, mo[:, 0]),
               lambda: ops.pnp_update(st, m, mo, None, torch.rand(2, 16), THR, 4)):
        with pytest.raises(L.DransacError, match="GPU tensors"):
            fn()
    assert calls == []
    # the shape checks, on tensors that claim to be on the device (nothing is launched: call is patched)
    monkeypatch.setattr(ops, "_gpu_only", lambda *a, **k: None)
    with pytest.raises(L.DransacError, match="matches"):
        ops.p3p_gather(torch.rand(2, 16, 6), idx)
    with pytest.raises(L.DransacError, match="index sets"):
        ops.p3p_gather(m, idx.long())
    with pytest.raises(L.DransacError, match="index sets"):
        ops.p3p_gather(m, torch.zeros(2, 4, 4, dtype=torch.int32))
    with pytest.raises(L.DransacError, match="models"):
        ops.pnp_score(m, torch.rand(2, 16, 3, 3), THR)
    with pytest.raises(L.DransacError, match="models"):
        ops.pnp_score(m, mo.double(), THR)
    with pytest.raises(L.DransacError, match="valid"):
        ops.pnp_score(m, mo, THR, valid=torch.ones(2, 15, dtype=torch.bool))
    with pytest.raises(L.DransacError, match="scores"):
        ops.pnp_update(st, m, mo, None, torch.rand(2, 15), THR, 4)
    with pytest.raises(L.DransacError, match="PnPState"):
        ops.pnp_update(ops.PnPState(2, 17, 100, "cpu", torch.float32), m, mo, None, torch.rand(2, 16), THR, 4)
    with pytest.raises(L.DransacError, match="init_model"):
        ops.refit_pnp(m, None, torch.rand(2, 3, 3))
    with pytest.raises(L.DransacError, match="mask"):
        ops.refit_pnp(m, torch.ones(2, 15, dtype=torch.bool), mo[:, 0])
    with pytest.raises(L.DransacError, match="iters"):
        ops.refit_pnp(m, None, mo[:, 0], iters=-1)
    assert calls == []
