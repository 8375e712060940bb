"""Local optimisation on the device (dr_local_opt, lo = 1 / 2): one launch against the f64 restatement's LO step
(tests/lo_ref.py), its gating, the drivers on the reference's lo fixtures, batched against per pair, graph capture, and
the other solvers."""
import pytest
import torch

from oracle import cpu_ref as O
from tests import lo_ref
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

KEYS = ("model", "mask", "score", "iterations", "inliers")


def _seeded_state(dev, fmat, dt, P=8, N=2000, seed0=300):
    """P synthetic pairs and a test-mode state whose best model is the ground truth, perturbed, with its MSAC mask / score"""
    from differentiable_ransac_amd import ops, synth
    d = synth.batch_two_view(P, N, seed0=seed0, pixel=fmat, inlier_ratio=0.6)
    m = d["matches"].to(dt)
    thr = torch.stack([torch.tensor(float(O.normalized_threshold(0.75, d["K1"][p].double(), d["K2"][p].double(), fmat)))
                       for p in range(P)]).to(dt)
    gt = (d["gt_F"] if fmat else d["gt_E"]).double()
    g = torch.Generator().manual_seed(seed0)
    model = gt * (1 + 3e-3 * torch.randn(gt.shape, generator=g, dtype=torch.float64))
    model = model.to(dt)
    st = ops.RansacState(P, N, 5000, dev, dt)
    score, mask = [], []
    for p in range(P):
        s, mk = O.msac_score(m[p], model[p:p + 1], float(thr[p]))
        score.append(float(s[0]))
        mask.append(mk[0])
    st.best_score.copy_(torch.tensor(score, dtype=dt))
    st.best_model.copy_(model)
    st.best_mask.copy_(torch.stack(mask))
    st.best_inliers.copy_(torch.stack(mask).sum(-1).int())
    st.iters.fill_(16)
    return st, m, thr, model, torch.tensor(score, dtype=torch.float64), torch.stack(mask)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("lo", [1, 2])
@pytest.mark.parametrize("fmat", [False, True])
def test_one_launch_matches_the_restatement(dev, fmat, lo, dt):
    from differentiable_ransac_amd import ops
    P, N, lo_iters = 8, 2000, 8
    k = 7 if fmat else 5
    st, m, thr, model0, score0, mask0 = _seeded_state(dev, fmat, dt, P, N)
    seen = torch.full((P, 10), float("nan"), device=dev, dtype=dt)
    refits = torch.zeros(P, device=dev, dtype=torch.int32)
    md, td = m.to(dev), thr.to(dev)
    ops.local_optimize(st, md, td, fmat, lo, lo_iters, k, 0.999, 1e-5, 5000, seen, refits)
    torch.cuda.synchronize()
    changed = 0
    for p in range(P):
        sc, mk, mo, n = lo_ref.lo_step(m[p].double(), float(thr[p]), fmat, lo, lo_iters, float(score0[p]), mask0[p],
                                       model0[p].double())
        gs, gm = float(st.best_score[p]), st.best_mask[p].cpu()
        assert abs(gs - sc) <= (1e-4 if dt == torch.float32 else 1e-9) * max(1.0, sc), (p, gs, sc)
        assert int((gm != mk).sum()) <= (1 if dt == torch.float32 else 0), p
        assert int(st.best_inliers[p]) == int(gm.sum())
        tol = (1e-3 if not fmat else 1e-4) if dt == torch.float32 else 1e-7
        assert (O.canonical(st.best_model[p].cpu().double()) - O.canonical(mo.double())).abs().max() < tol, p
        want_mi = min(5000, O.adaptive_iteration_number(int(gm.sum()), N, k, 0.999, max_iterations=5000))
        assert abs(float(st.max_iters[p]) - want_mi) <= 1e-9 * max(1.0, want_mi), p
        assert 1 <= int(refits[p]) <= (1 if lo == 1 else lo_iters)
        if dt == torch.float64:
            assert int(refits[p]) == n, p
        changed += int(not torch.equal(gm, mask0[p]))
        # the snapshot holds the state LO left
        assert torch.equal(seen[p, 0].cpu(), st.best_score[p].cpu())
        assert torch.equal(seen[p, 1:].cpu(), st.best_model[p].reshape(9).cpu())
    assert changed >= 1             # the perturbed seeds leave LO something to do


@pytest.mark.parametrize("fmat", [False, True])
def test_gating_leaves_unreplaced_pairs_alone(dev, fmat):
    from differentiable_ransac_amd import ops
    P, N = 8, 2000
    k = 7 if fmat else 5
    st, m, thr, *_ = _seeded_state(dev, fmat, torch.float32, P, N, seed0=340)
    md, td = m.to(dev), thr.to(dev)
    seen = torch.full((P, 10), float("nan"), device=dev)
    # pairs 0-3 are marked as visited with their current state: LO must not touch them
    seen[:4, 0] = st.best_score[:4]
    seen[:4, 1:] = st.best_model[:4].reshape(4, 9)
    st.max_iters[:4] = 1234.5
    before = {key: getattr(st, key).clone() for key in ("best_score", "best_model", "best_mask", "best_inliers", "max_iters", "iters")}
    refits = torch.zeros(P, device=dev, dtype=torch.int32)
    ops.local_optimize(st, md, td, fmat, 2, 8, k, 0.999, 1e-5, 5000, seen, refits)
    torch.cuda.synchronize()
    for key, v in before.items():
        assert torch.equal(getattr(st, key)[:4], v[:4]), key
    assert (refits[:4] == 0).all() and (refits[4:] >= 1).all() and (refits[4:] <= 8).all()
    # a second launch with no update in between changes nothing at all
    after = {key: getattr(st, key).clone() for key in before}
    r1, s1 = refits.clone(), seen.clone()
    ops.local_optimize(st, md, td, fmat, 2, 8, k, 0.999, 1e-5, 5000, seen, refits)
    torch.cuda.synchronize()
    for key, v in after.items():
        assert torch.equal(getattr(st, key), v), key
    assert torch.equal(refits, r1) and torch.equal(seen.isnan(), s1.isnan()) and torch.equal(seen.nan_to_num(), s1.nan_to_num())


def _dropin(name, lo, dev, fused):
    from differentiable_ransac_amd.estimators import EssentialMatrixEstimatorNister, FundamentalMatrixEstimatorNew
    from differentiable_ransac_amd.ransac import RANSAC
    from differentiable_ransac_amd.samplers import GumbelSoftmaxSampler
    from differentiable_ransac_amd.scorings import MSACScore
    fmat = name == "f8"
    est = FundamentalMatrixEstimatorNew(dev) if fmat else EssentialMatrixEstimatorNister(dev)
    r = RANSAC(est, GumbelSoftmaxSampler(16, 8 if fmat else 5, device=dev), MSACScore(dev), fmat=fmat, train=False,
               ransac_batch_size=16, sampler_id=3 if fmat else 2, threshold=0.75, max_iterations=5000, lo=lo, lo_iters=8)
    r.fused = fused
    return r


def _check_against_restatement(name, g, lo, model, mask, score, iters, sample_size=None):
    dt = torch.float64
    mo, masko, so, ito, _ = lo_ref.ransac_test_lo(g["matches"].to(dt), g["logits"].to(dt), [x.to(dt) for x in g["gumbels"]],
                                                   g["K1"].to(dt), g["K2"].to(dt), name, lo, int(g["lo_iters"]),
                                                   sample_size=sample_size)
    assert int(iters) == ito
    assert int((mask.cpu() != masko).sum()) <= 1
    assert abs(float(score) - so) <= 1e-4 * max(1.0, so), (float(score), so)
    tol = 1e-4 if name == "f8" else 1e-3
    assert (O.canonical(model.cpu().double()) - O.canonical(mo.double())).abs().max() < tol


def _drivers_against_restatement(dev, name, lo):
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    g = load_golden(f"ransac_test_lo_{name}")
    noise = [x.to(dev) for x in g["gumbels"]]
    args = (g["matches"].to(dev), g["logits"].to(dev), g["K1"].to(dev), g["K2"].to(dev))
    # (every driver's adaptive stop takes the estimator's sample_size, 7 for the 8-point F estimator, as the reference's does)
    # drop-in, fused: the device-resident driver with dr_local_opt
    model, mask, score, iters = _dropin(name, lo, dev, True)(*args, None, gumbels=noise)
    _check_against_restatement(name, g, lo, model, mask, score, iters, sample_size=int(g["sample_size"]))
    # drop-in, plugin path: the host-side restatement with the package's estimators
    model, mask, score, iters = _dropin(name, lo, dev, False)(*args, None, gumbels=noise)
    _check_against_restatement(name, g, lo, model, mask, score, iters, sample_size=int(g["sample_size"]))
    # BatchedRANSAC, one pair
    drv = BatchedRANSAC(name, ransac_batch_size=16, threshold=0.75, max_iterations=5000, lo=lo, lo_iters=8,
                        num_samples=8 if name == "f8" else None)
    out = drv(*(a[None] for a in args), gumbels=[x[None] for x in noise])
    _check_against_restatement(name, g, lo, out["model"][0], out["mask"][0], out["score"][0], out["iterations"][0],
                               sample_size=int(g["sample_size"]))
    assert int(out["lo_refits"][0]) >= 1


@pytest.mark.parametrize("lo", [1, 2])
@pytest.mark.parametrize("name", ["nister"])
def test_drivers_reproduce_the_restatement_on_the_reference_fixtures(dev, name, lo):
    _drivers_against_restatement(dev, name, lo)


@pytest.mark.parametrize("lo", [1, 2])
def test_f8_drivers_reproduce_the_restatement_with_the_estimator_exponent(dev, lo):
    """the 8-point F drivers on the reference's lo fixture: all three stop with the F estimator's sample_size (7), the
    reference's exponent, although they sample 8 points (with lo = 2 the reference stopped at 528 on its bound; exponent 8
    runs to the end of the recorded list, 800)"""
    _drivers_against_restatement(dev, "f8", lo)


def test_batched_equals_per_pair_calls(dev):
    from differentiable_ransac_amd import synth
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    P, N, B = 8, 1000, 128
    d = synth.batch_two_view(P, N, seed0=60)
    noise = [synth.gumbel_noise((P, B, N), seed=70 + r).to(dev) for r in range(5)]
    kw = dict(ransac_batch_size=B, threshold=0.75, max_iterations=5 * B, lo=2, lo_iters=16)
    m, lg, K1, K2 = (d[k].to(dev) for k in ("matches", "logits", "K1", "K2"))
    out = BatchedRANSAC("nister", **kw)(m, lg, K1, K2, gumbels=noise)
    for p in range(P):
        one = BatchedRANSAC("nister", **kw)(m[p:p + 1], lg[p:p + 1], K1[p:p + 1], K2[p:p + 1], gumbels=[n[p:p + 1] for n in noise])
        assert int(one["iterations"][0]) == int(out["iterations"][p]), p
        assert torch.equal(one["mask"][0], out["mask"][p]), p
        assert int(one["lo_refits"][0]) == int(out["lo_refits"][p]), p


def test_device_terminated_graph_replay_equals_eager(dev):
    from differentiable_ransac_amd import synth
    from differentiable_ransac_amd.graphs import GraphedStep
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    P, N = 4, 2000
    d = synth.batch_two_view(P, N, seed0=80)
    m, lg, K1, K2 = (d[k].to(dev) for k in ("matches", "logits", "K1", "K2"))
    kw = dict(ransac_batch_size=1024, threshold=0.75, max_iterations=4096, seed=5, lo=1)
    # the host loop (pipelined, read-backs) and the device-terminated loop agree on a first call
    host = BatchedRANSAC("nister", **kw)(m, lg, K1, K2)
    dterm = BatchedRANSAC("nister", **kw)
    dterm.device_termination = True
    first = dterm(m, lg, K1, K2)
    for key in KEYS + ("lo_refits",):
        assert torch.equal(host[key], first[key]), key
    # eager device-terminated calls against a captured, replayed one (same seeds: every call takes one per batch)
    eager = BatchedRANSAC("nister", **kw)
    eager.device_termination = True
    graphed = BatchedRANSAC("nister", **kw).device_seeds(dev)
    graphed.device_termination = True
    warm = 2
    for _ in range(warm):
        eager(m, lg, K1, K2)
    step = GraphedStep(lambda: graphed(m, lg, K1, K2), warmup=warm)
    for r in range(3):
        want, got = eager(m, lg, K1, K2), step()
        for key in KEYS + ("lo_refits",):
            assert torch.equal(want[key], got[key]), (key, r)
    assert int(got["lo_refits"].min()) >= 1


def test_dropin_graph_path_equals_the_eager_driver(dev):
    """RANSAC(lo=1, -rbs 1024): 5 device rounds, one replayed graph per call; the same call on the eager driver with the seeds
    the graph draws (its two warm-up calls took 5 each, every replay takes 5)"""
    from differentiable_ransac_amd import estimators, samplers, scorings, synth
    from differentiable_ransac_amd.ransac import RANSAC, BatchedRANSAC
    P, N = 3, 2000
    d = synth.batch_two_view(P, N, seed0=90)
    m, lg, K1, K2 = (d[k].to(dev) for k in ("matches", "logits", "K1", "K2"))
    rn = RANSAC(estimators.EssentialMatrixEstimatorNister(dev), samplers.GumbelSoftmaxSampler(1024, 5, device=dev, seed=9),
                scorings.MSACScore(dev), train=False, ransac_batch_size=1024, sampler_id=2, threshold=0.75, max_iterations=5000,
                lo=1)
    base = (9 * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    ref = BatchedRANSAC("nister", ransac_batch_size=1024, threshold=0.75, max_iterations=5000, seed=base, refit=True, lo=1)
    ref.device_termination = True                          # every batch issued: 5 seeds per call, as in the graph
    ref.calls = 2 * 5
    for p in range(P):
        model, mask, score, iters = rn(m[p], lg[p], K1[p], K2[p], None)
        want = ref(m[p:p + 1], lg[p:p + 1], K1[p:p + 1], K2[p:p + 1])
        assert torch.equal(model, want["model"][0]) and torch.equal(mask, want["mask"][0]), p
        assert torch.equal(score, want["score"][0]) and int(iters) == int(want["iterations"][0]), p
    assert len(rn._graphs) == 1 and rn._graph_rounds == 5


@pytest.mark.parametrize("solver", ["stewenius", "f7"])
def test_other_solvers_run_with_lo(dev, solver):
    from differentiable_ransac_amd import synth
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    fmat = solver == "f7"
    P, N = 4, 1000
    d = synth.batch_two_view(P, N, seed0=110, pixel=fmat)
    m, lg, K1, K2 = (d[k].to(dev) for k in ("matches", "logits", "K1", "K2"))
    drv = BatchedRANSAC(solver, ransac_batch_size=256, threshold=0.75, max_iterations=1024, lo=2, lo_iters=8, refit=False)
    out = drv(m, lg, K1, K2)
    torch.cuda.synchronize()
    assert (out["lo_refits"] >= 1).all()
    for p in range(P):
        thr = float(O.normalized_threshold(0.75, d["K1"][p].double(), d["K2"][p].double(), fmat))
        _, mk = O.msac_score(m[p].cpu().double(), out["model"][p].cpu().double()[None], thr)
        assert int((mk[0] != out["mask"][p].cpu()).sum()) <= 1, p
        assert int(out["inliers"][p]) == int(out["mask"][p].sum()), p
