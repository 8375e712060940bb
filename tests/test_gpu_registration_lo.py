"""dr_registration_local_opt and BatchedRegistration(lo = 1 / 2) against the f64 restatement tests/registration_lo_ref.py.

One launch: P = 6 pairs, N in {3, 255, 256, 257, 1000} (the 256-thread stride's edges and a multi-pass row), lo in {1, 2}, lo_iters = 8,
scenes with noise 0.02 and 0.6 / 0.35 / 0.15 inliers, the state seeded by one oracle update from three true inliers.  A case (pair) is
compared with the oracle -- fits run and mask exactly, score within registration_ref.score_tolerance, model within the bound of
tests/test_gpu_registration.py (_model_tol), inlier count exactly, stop bound to that file's 1e-12 -- unless a fit of the oracle's
trajectory has an acceptance margin below twice the score tolerance or a point inside registration_ref.BAND; what that leaves out is
counted and bounded in tests/test_registration_lo_host.py (no f64 case; 42 of 60 f32 cases, see there why).  EVERY case, left out or
not, is held to what no decision can change: the state is the one dr_registration_update writes for the final model (mask, count and
stop bound bit for bit), the score is the MSAC score of that model within the tolerance and not below the seed's, the fits run are
within 1..lo_iters.  Every test prints its figures before it asserts."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import registration_lo_ref as LR
from tests import registration_ref as R
from tests.test_gpu_registration import DRV, NAME, THR, _driver_inputs, _model_tol

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
KEYS = ("best_score", "best_model", "best_mask", "best_inliers", "iters", "max_iters")
MAXIT = LR.LO_MAX_ITERATIONS


@functools.lru_cache(maxsize=None)
def _case(N, lo, name):
    return LR.build_case(N, lo, name)


def _device_state(seeds, matches, dev, dt, guard=False):
    """seeds: list of oracle states -> (RegistrationState, lo_seen, lo_refits, padded buffers or None); with `guard` the mask, the model
    and the snapshot live inside sentinel-filled buffers one row longer at each end"""
    from differentiable_ransac_amd import ops
    P, N = len(seeds), matches.shape[1]
    st = ops.RegistrationState(P, N, MAXIT, dev, dt)
    seen = torch.full((P, 17), float("nan"), device=dev, dtype=dt)
    pads = None
    if guard:
        pads = dict(best_mask=torch.full((P + 2, N), 0x5A, device=dev, dtype=torch.uint8),
                    best_model=torch.full((P + 2, 4, 4), -7.5, device=dev, dtype=dt), seen=torch.full((P + 2, 17), -7.5, device=dev, dtype=dt))
        st.best_mask = pads["best_mask"][1:P + 1].view(torch.bool)
        st.best_model = pads["best_model"][1:P + 1]
        seen = pads["seen"][1:P + 1]
        seen.fill_(float("nan"))
    st.best_score.copy_(torch.tensor([s["best_score"] for s in seeds], dtype=torch.float64))
    st.best_model.copy_(torch.from_numpy(np.stack([s["best_model"] for s in seeds])))
    st.best_mask.copy_(torch.from_numpy(np.stack([s["best_mask"] for s in seeds])))
    st.best_inliers.copy_(torch.tensor([s["best_inliers"] for s in seeds], dtype=torch.int32))
    st.iters.copy_(torch.tensor([s["iters"] for s in seeds], dtype=torch.int32))
    st.max_iters.copy_(torch.tensor([s["max_iters"] for s in seeds], dtype=torch.float64))
    return st, seen, torch.zeros(P, device=dev, dtype=torch.int32), pads


def _snap(st):
    return {k: getattr(st, k).clone() for k in KEYS}


def _launch(st, tm, lo, seen, refits, lo_iters=LR.LO_ITERS):
    from differentiable_ransac_amd import ops
    ops.registration_local_optimize(st, tm, ops.thr2_tensor(THR, tm.shape[0], tm), lo, lo_iters, 0.999, 1e-5, MAXIT, seen, refits)


# ------------------------------------------------------------------------------------------------ one launch
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("lo", [1, 2])
@pytest.mark.parametrize("N", LR.LO_NS)
def test_one_launch_against_the_restatement(dev, dt, lo, N):
    from differentiable_ransac_amd import ops
    name = NAME[dt]
    cases = _case(N, lo, name)
    P = len(cases)
    m = np.stack([c["matches"] for c in cases])
    tm = torch.from_numpy(m).to(dev, dt)
    st, seen, refits, _ = _device_state([c["seed"] for c in cases], m, dev, dt)
    before = {k: v.cpu() for k, v in _snap(st).items()}
    _launch(st, tm, lo, seen, refits)
    after = {k: v.cpu() for k, v in _snap(st).items()}
    refits, seen = refits.cpu(), seen.cpu()
    # what dr_registration_update writes for the final models (a fresh state takes any valid model)
    ref = ops.RegistrationState(P, N, MAXIT, dev, dt)
    ops.registration_update(ref, tm, st.best_model.unsqueeze(1).clone(), None, torch.ones(P, 1, device=dev, dtype=dt), THR, 64)
    ref = {k: getattr(ref, k).cpu() for k in KEYS}
    worst_s = worst_m = 0.0
    left = 0
    for p, c in enumerate(cases):
        o, fits, tol = c["after"], c["fits"], c["tol"]
        n_fit, moved = int(refits[p]), not torch.equal(after["best_model"][p], before["best_model"][p])
        print(f"lo {name} N={N} lo={lo} pair {p}: fits {n_fit} (oracle {len(fits)}), score {float(before['best_score'][p]):.4f} -> "
              f"{float(after['best_score'][p]):.4f} (oracle {o['best_score']:.4f}, tol {tol:.3g}), inliers {int(before['best_inliers'][p])} -> "
              f"{int(after['best_inliers'][p])} (oracle {o['best_inliers']}), left out {c['excluded']}")
        # ---- every case
        assert torch.equal(after["iters"][p], before["iters"][p])
        assert float(seen[p, 0]) == float(after["best_score"][p]) and torch.equal(seen[p, 1:], after["best_model"][p].reshape(16))
        if c["seed"]["best_inliers"] < 3:
            assert n_fit == 0 and all(torch.equal(after[k][p], before[k][p]) for k in KEYS), p
            continue
        assert 1 <= n_fit <= (1 if lo == 1 else LR.LO_ITERS), p
        assert float(after["best_score"][p]) >= float(before["best_score"][p]), p
        if moved:
            assert float(after["best_score"][p]) > float(before["best_score"][p]), p
            assert torch.equal(after["best_mask"][p], ref["best_mask"][p]) and int(after["best_inliers"][p]) == int(ref["best_inliers"][p]), p
            assert np.array_equal(after["best_model"][p, 3].numpy(), [0, 0, 0, 1]), p
            s_own = R.msac(c["matches"], after["best_model"][p].double().numpy(), c["thr"])[0]
            assert abs(float(after["best_score"][p]) - s_own) <= tol, (p, float(after["best_score"][p]), s_own, tol)
        else:
            assert all(torch.equal(after[k][p], before[k][p]) for k in ("best_score", "best_mask", "best_inliers")), p
        assert int(after["best_inliers"][p]) == int(after["best_mask"][p].sum()), p
        want = R.stop_rule(int(after["best_inliers"][p]), N, max_iterations=MAXIT)
        assert abs(float(after["max_iters"][p]) - want) <= 1e-12 * max(1.0, want), p
        if moved:
            assert float(after["max_iters"][p]) == float(ref["max_iters"][p]), p
        # ---- against the oracle's trajectory
        if c["excluded"]:
            left += 1
            continue
        assert n_fit == len(fits), (p, n_fit, len(fits))
        assert np.array_equal(after["best_mask"][p].numpy(), o["best_mask"]), p
        assert int(after["best_inliers"][p]) == o["best_inliers"], p
        assert abs(float(after["best_score"][p]) - o["best_score"]) <= tol, p
        worst_s = max(worst_s, abs(float(after["best_score"][p]) - o["best_score"]) / tol)
        dR, dT = R.model_error(after["best_model"][p].double().numpy(), R_rounded(o["best_model"], dt) if not moved else o["best_model"])
        mtol = _model_tol(dt, o["model_ratio"])
        assert max(dR, dT) <= mtol, (p, dR, dT, mtol)
        worst_m = max(worst_m, max(dR, dT) / mtol)
        want = R.stop_rule(o["best_inliers"], N, max_iterations=MAXIT)
        assert abs(float(after["max_iters"][p]) - want) <= 1e-12 * max(1.0, want), p
    print(f"lo {name} N={N} lo={lo}: left out {left}/{P}, worst score err/tol {worst_s:.3g}, worst model err/tol {worst_m:.3g}")
    if dt == torch.float64:
        assert left == 0


def R_rounded(a, dt):
    return torch.from_numpy(np.asarray(a, np.float64)).to(dt).double().numpy()


# ------------------------------------------------------------------------------------------------ gate, few inliers, repeatability
@pytest.mark.parametrize("dt", DTYPES)
def test_gate_guards_and_repeatability(dev, dt):
    name = NAME[dt]
    cases = _case(257, 2, name)
    m = np.stack([c["matches"] for c in cases])
    tm = torch.from_numpy(m).to(dev, dt)
    seeds = [dict(c["seed"]) for c in cases]
    two = np.zeros(257, bool)
    two[[5, 200]] = True
    seeds[4].update(best_mask=two, best_inliers=2)                  # a pair with two inliers
    runs = []
    for _ in range(2):                                              # two launches from copies of one state
        st, seen, refits, pads = _device_state(seeds, m, dev, dt, guard=True)
        before = _snap(st)
        _launch(st, tm, 2, seen, refits)
        runs.append((st, seen, refits, pads, before))
    (st, seen, refits, pads, before), (st2, seen2, refits2, pads2, _) = runs
    for k in KEYS:
        assert torch.equal(getattr(st, k), getattr(st2, k)), k
    assert torch.equal(seen, seen2) and torch.equal(refits, refits2)
    print(f"gate {name}: fits {refits.cpu().tolist()}")
    assert int(refits[4]) == 0 and all(torch.equal(getattr(st, k)[4], before[k][4]) for k in KEYS)
    assert float(seen[4, 0]) == float(st.best_score[4]) and torch.equal(seen[4, 1:], st.best_model[4].reshape(16))
    assert int(refits.max()) > 1
    for key in ("best_mask", "best_model", "seen"):                 # the guard rows
        g = pads[key]
        fill = torch.full_like(g[0], 0x5A if key == "best_mask" else -7.5)
        assert torch.equal(g[0], fill) and torch.equal(g[-1], fill), key
    # a second launch on the state the first one left: nothing moves
    first, first_seen, first_refits = _snap(st), seen.clone(), refits.clone()
    _launch(st, tm, 2, seen, refits)
    for k in KEYS:
        assert torch.equal(getattr(st, k), first[k]), k
    assert torch.equal(seen, first_seen) and torch.equal(refits, first_refits)
    # N = 1: untouched except for the snapshot
    from differentiable_ransac_amd import ops
    one = ops.RegistrationState(2, 1, MAXIT, dev, dt)
    one.best_score.fill_(0.25)
    one.best_mask.fill_(True)
    one.best_inliers.fill_(1)
    b1 = _snap(one)
    s1, r1 = torch.full((2, 17), float("nan"), device=dev, dtype=dt), torch.zeros(2, device=dev, dtype=torch.int32)
    _launch(one, tm[:2, :1].contiguous(), 2, s1, r1)
    assert all(torch.equal(getattr(one, k), b1[k]) for k in KEYS) and int(r1.sum()) == 0
    assert torch.equal(s1[:, 0], one.best_score) and torch.equal(s1[:, 1:], one.best_model.reshape(2, 16))


# ------------------------------------------------------------------------------------------------ BatchedRegistration(lo=)
def test_driver_against_run_lo(dev):
    """the pattern of test_gpu_registration.test_driver_against_oracle (f64, explicit noise, at most four rounds), with lo = 2: the
    condition on the input is that every decision margin -- of the rounds and of the LO fits -- and the final refit's exceed the score
    tolerance"""
    from differentiable_ransac_amd import ops
    from differentiable_ransac_amd.ransac import BatchedRegistration
    P, N, B = DRV["P"], DRV["N"], DRV["B"]
    max_iterations = 4 * B
    _, m, noise = _driver_inputs(math.ceil(2000 / B))
    dt = torch.float64
    tm = torch.from_numpy(m).to(dev)
    logits = torch.zeros(P, N, device=dev, dtype=dt)
    g = [x.to(dev) for x in noise[:4]]
    drv = BatchedRegistration(ransac_batch_size=B, threshold=THR, max_iterations=max_iterations, lo=2, lo_iters=8)
    out = {k: v.cpu() for k, v in drv(tm, logits, gumbels=g).items()}
    idx = [ops.gumbel_topk(logits, B, 3, 1.0, x, 0, soft=False)["idx"].cpu().numpy() for x in g]
    for p in range(P):
        o = LR.run_lo(m[p], [i[p] for i in idx], 2, 8, THR, max_iterations=max_iterations)
        tol = R.score_tolerance(m[p], o["model"], THR, "float64")
        margin = min(o["gaps"] + [o["refit_gap"]])
        band = np.abs(o["ratio2"] - 1.0) < R.BAND["float64"]
        print(f"driver lo=2 pair {p}: rounds {o['rounds']}, iterations {o['iterations']}, inliers {o['inliers']}, fits {o['lo_refits']} "
              f"(kernel {int(out['lo_refits'][p])}), score {o['score']:.6f} (kernel {float(out['score'][p]):.6f}), smallest margin "
              f"{margin:.3g} vs tolerance {tol:.3g}, band {int(band.sum())}")
        assert margin > tol, (p, margin, tol)                       # the condition on the input
        assert int(out["iterations"][p]) == o["iterations"] and int(out["inliers"][p]) == o["inliers"], p
        assert int(out["lo_refits"][p]) == o["lo_refits"], p
        assert np.array_equal(out["mask"][p].numpy()[~band], o["mask"][~band]), p
        assert abs(float(out["score"][p]) - o["score"]) <= tol, p
        dR, dT = R.model_error(out["model"][p].numpy(), o["model"])
        mtol = _model_tol(dt, o["model_ratio"])
        print(f"   model err {max(dR, dT):.3g}, tol {mtol:.3g}")
        assert max(dR, dT) <= mtol, (p, dR, dT, mtol)
    assert int(out["lo_refits"].max()) >= 1          # (LO ran: the 0.15 pair may not reach three inliers in four rounds)


@pytest.mark.parametrize("dt", DTYPES)
def test_one_round_lo2_is_never_below_lo0(dev, dt):
    from differentiable_ransac_amd.ransac import BatchedRegistration, adaptive_iteration_number
    P, N, B = 6, 500, 64
    m = np.stack([R.scene(600 + p, N, LR.LO_SHARES[p % 3], noise=0.02)["matches"] for p in range(P)])
    tm = torch.from_numpy(m).to(dev, dt)
    logits = torch.zeros(P, N, device=dev, dtype=dt)
    kw = dict(ransac_batch_size=B, threshold=THR, max_iterations=B, seed=5, refit=False)
    a = BatchedRegistration(**kw)(tm, logits)
    b = BatchedRegistration(lo=2, lo_iters=8, **kw)(tm, logits)
    assert "lo_refits" not in a and "lo_refits" in b
    print(f"one round {NAME[dt]}: score {a['score'].cpu().tolist()} -> {b['score'].cpu().tolist()}, inliers {a['inliers'].cpu().tolist()} -> "
          f"{b['inliers'].cpu().tolist()}, fits {b['lo_refits'].cpu().tolist()}")
    assert bool((b["score"] >= a["score"]).all())
    assert torch.equal(a["iterations"], b["iterations"]) and int(a["iterations"][0]) == B
    rose = 0
    for p in range(P):
        if int(b["inliers"][p]) > int(a["inliers"][p]):
            rose += 1
            bound = [adaptive_iteration_number(int(x["inliers"][p]), N, 3, 0.999, 1e-5, 5000) for x in (a, b)]
            assert bound[1] <= bound[0], (p, bound)
    assert rose > 0


@pytest.mark.parametrize("dt", DTYPES)
def test_device_termination_and_graph_replay_with_lo(dev, dt):
    """the pattern of test_gpu_registration.test_driver_device_termination_and_graph_replay with lo = 2"""
    from differentiable_ransac_amd.graphs import GraphedStep
    from differentiable_ransac_amd.ransac import BatchedRegistration
    P, N, B = DRV["P"], DRV["N"], DRV["B"]
    _, m, noise = _driver_inputs(math.ceil(2000 / B))
    tm = torch.from_numpy(m).to(dev, dt)
    logits = torch.zeros(P, N, device=dev, dtype=dt)
    g = [x.to(dev, dt) for x in noise[:16]]
    kw = dict(ransac_batch_size=B, threshold=THR, max_iterations=16 * B, lo=2, lo_iters=8)
    keys = ("model", "mask", "score", "inliers", "iterations", "lo_refits")
    host = BatchedRegistration(**kw)(tm, logits, gumbels=g)
    dterm = BatchedRegistration(**kw)
    dterm.device_termination = True
    eager = dterm(tm, logits, gumbels=g)
    assert all(torch.equal(host[k], eager[k]) for k in keys)
    print(f"device termination lo=2 {NAME[dt]}: iterations {host['iterations'].cpu().tolist()}, fits {host['lo_refits'].cpu().tolist()}")
    assert int(host["lo_refits"].min()) >= 1
    step = GraphedStep(lambda: dterm(tm, logits, gumbels=g), warmup=1)
    for _ in range(2):
        replay = step()
        torch.cuda.synchronize()
        assert all(torch.equal(eager[k], replay[k]) for k in keys)
