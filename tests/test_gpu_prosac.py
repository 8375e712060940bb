"""PROSAC sampling on the device: dr_prosac_sample bit for bit against the numpy reference (tests/prosac_ref.py), the ranking,
the two drivers against their own loops over the ops, what the sampler is for (a 3 % pair found in one round), and capture."""
import functools

import numpy as np
import pytest
import torch

from tests import prosac_ref as PR
from tests import registration_ref as R

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE12_9E3779B9          # 64 bits, high word in use
KEYS = ("model", "mask", "score", "inliers", "iterations")


def _signed(v):
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _same(a, b, keys=KEYS):
    return all(torch.equal(a[k], b[k]) for k in keys)


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("cfg", [(3, 3, 10), (9, 8, 20), (37, 3, 50), (37, 5, 50), (2049, 5, 4000)],
                         ids=lambda c: "-".join(map(str, c)))
def test_sampler_equals_the_reference_bit_for_bit(dev, cfg):
    """P = 3, B = 300 (a second, partial block; a partial wave); launches that start in the growth regime, cross into the tail,
    and start in the tail; a random order per pair and none; by-value and device seed; twice"""
    from differentiable_ransac_amd import ops
    N, k, T_N = cfg
    P, B = 3, 300
    table = PR.growth_table(N, k, T_N)
    growth = ops.prosac_growth(N, k, T_N, dev)
    assert np.array_equal(growth.cpu().numpy(), table)
    rng = np.random.default_rng(N * 100 + k)
    order = np.stack([rng.permutation(N) for _ in range(P)])
    t_order = torch.from_numpy(order).to(dev, torch.int32)
    seed_dev = torch.tensor([_signed(SEED)], dtype=torch.int64, device=dev)
    last = int(table[-1])
    for t0 in sorted({0, max(0, last - 150), last + 7}):
        for o_np, o_t in ((order, t_order), (None, None)):
            want = PR.sample(o_np, table, SEED, t0, P, B, N, k)
            got = ops.prosac_sample(o_t, growth, B, k, SEED, t0, P=P, N=N, device=dev)
            assert got.dtype == torch.int32 and got.shape == (P, B, k)
            assert np.array_equal(got.cpu().numpy(), want), (cfg, t0, o_np is None)
            assert torch.equal(got, ops.prosac_sample(o_t, growth, B, k, seed_dev, t0, P=P, N=N, device=dev))
            assert torch.equal(got, ops.prosac_sample(o_t, growth, B, k, SEED, t0, P=P, N=N, device=dev))
    if N > k:
        other = ops.prosac_sample(t_order, growth, B, k, SEED + 1, last + 7)
        assert not torch.equal(other, ops.prosac_sample(t_order, growth, B, k, SEED, last + 7))


def test_sampler_refuses_bad_arguments(dev):
    from differentiable_ransac_amd import _lib as L
    from differentiable_ransac_amd import ops
    growth = ops.prosac_growth(9, 3, 20, dev)
    with pytest.raises(L.DransacError):
        ops.prosac_sample(None, growth, 4, 3, 1, -1, P=1, N=9, device=dev)
    with pytest.raises(L.DransacError):
        ops.prosac_sample(None, growth, 4, 4, 1, 0, P=1, N=9, device=dev)      # a table made for another k
    with pytest.raises(L.DransacError):
        ops.prosac_sample(torch.zeros(1, 9, device=dev, dtype=torch.int64), growth, 4, 3, 1, 0)


# --------------------------------------------------------------------------------------------------------------- the ranking
def test_rank(dev):
    from differentiable_ransac_amd import ops
    assert ops.prosac_rank(None) is None
    nan, inf = float("nan"), float("inf")
    rows = [[0.5, nan, 2.0, 0.5, -inf, inf, -0.0, 0.0, 2.0],
            [0.0, -0.0, 0.0, -0.0, nan, nan, 1.0, -1.0, 0.0],
            [3.0] * 9]
    want = PR.rank(np.asarray(rows))
    assert want[0].tolist() == [5, 2, 8, 0, 3, 6, 7, 1, 4]
    assert want[1].tolist() == [6, 0, 1, 2, 3, 8, 7, 4, 5]
    assert want[2].tolist() == list(range(9))
    for dt in (torch.float32, torch.float64):
        got = ops.prosac_rank(torch.tensor(rows, dtype=dt, device=dev))
        assert got.dtype == torch.int32 and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy(), want), dt
    # long rows (another sort path of the library), heavy ties, both signs of zero, some NaN
    rng = np.random.default_rng(5)
    lg = np.round(rng.standard_normal((2, 5000)) * 4.0) / 4.0
    lg[rng.random(lg.shape) < 0.05] = -0.0
    lg[rng.random(lg.shape) < 0.01] = np.nan
    lg = lg.astype(np.float32)
    want = PR.rank(lg)
    g32 = ops.prosac_rank(torch.from_numpy(lg).to(dev))
    g64 = ops.prosac_rank(torch.from_numpy(lg).to(dev, torch.float64))
    assert np.array_equal(g32.cpu().numpy(), want)
    assert torch.equal(g32, g64)


# --------------------------------------------------------------------------------------------------------------- the drivers
DRV = dict(P=3, N=256, B=128, rounds=3, seed=4100)


@functools.lru_cache(maxsize=None)
def _registration_inputs():
    """scenes of 0.6 / 0.35 / 0.15 inliers; logits that know something: 1 for an inlier, 0 for an outlier, plus N(0, 0.5^2)"""
    sc = [R.scene(DRV["seed"] + p, DRV["N"], s) for p, s in enumerate((0.6, 0.35, 0.15))]
    rng = np.random.default_rng(DRV["seed"])
    m = np.stack([s["matches"] for s in sc])
    lg = np.stack([s["inlier"].astype(np.float64) for s in sc]) + 0.5 * rng.standard_normal((DRV["P"], DRV["N"]))
    return m, lg


def _registration_loop(twin, tm, logits, rounds):
    """the rounds of BatchedRegistration(sampling="prosac") spelt out over the ops, seeded by a twin driver's seed source"""
    from differentiable_ransac_amd import ops
    P, N, _ = tm.shape
    B, k = twin.B, twin.k
    st = ops.RegistrationState(P, N, twin.max_iterations, tm.device, tm.dtype)
    thr2 = ops.thr2_tensor(twin.threshold, P, tm)
    order = ops.prosac_rank(logits)
    growth = ops.prosac_growth(N, k, twin.prosac_draws, tm.device)
    magsac = twin.scoring == "magsac"
    rejected = None if twin.edge_similarity is None else torch.zeros(P, device=tm.device, dtype=torch.int32)
    for r in range(rounds):
        idx = ops.prosac_sample(order, growth, B, k, twin._seeds.next(), r * B)
        if rejected is None:
            models, valid = ops.kabsch_gather(tm, idx)
        else:
            models, valid = ops.kabsch_gather_checked(tm, idx, twin.edge_similarity, rejected)
        score_fn = ops.rigid_magsac_score if magsac else ops.rigid_msac_score
        scores, _ = score_fn(tm, models, None, valid, want_inliers=False, thr2=thr2)
        ops.registration_update(st, tm, models, valid, scores, None, B, twin.confidence, twin.eps, thr2=thr2)
    model, score = st.best_model, st.best_score
    if magsac:
        fits = torch.zeros(P, device=tm.device, dtype=torch.int32)
        ops.registration_irls(st, tm, thr2, twin.irls_iters, fits)
    else:
        cand, cvalid = ops.refit_rigid(tm, st.best_mask)
        cscore, _ = ops.rigid_msac_score(tm, cand.unsqueeze(1), None, cvalid.unsqueeze(1), want_inliers=False, thr2=thr2)
        take = cscore[:, 0] > score
        model = torch.where(take[:, None, None], cand, model)
        score = torch.where(take, cscore[:, 0], score)
    out = dict(model=model, mask=st.best_mask, score=score, inliers=st.best_inliers, iterations=st.iters)
    if rejected is not None:
        out["rejected"] = rejected
    return out


@pytest.mark.parametrize("variant", ["f32", "f64", "edge", "magsac"])
def test_registration_driver_equals_its_loop_over_the_ops(dev, variant):
    from differentiable_ransac_amd.ransac import BatchedRegistration
    dt = torch.float64 if variant == "f64" else torch.float32
    m, lg = _registration_inputs()
    tm, logits = torch.from_numpy(m).to(dev, dt), torch.from_numpy(lg).to(dev, dt)
    kw = dict(ransac_batch_size=DRV["B"], threshold=R.THRESHOLD, max_iterations=DRV["rounds"] * DRV["B"], seed=77,
              sampling="prosac", prosac_draws=2000)
    if variant == "edge":
        kw["edge_similarity"] = 0.9
    if variant == "magsac":
        kw["scoring"] = "magsac"
    out = BatchedRegistration(**kw)(tm, logits)
    want = _registration_loop(BatchedRegistration(**kw), tm, logits, DRV["rounds"])
    print(f"{variant}: iterations {out['iterations'].cpu().tolist()} inliers {out['inliers'].cpu().tolist()}")
    assert _same(out, want)
    if variant == "edge":
        # (the driver may stop issuing rounds once every pair has terminated: it then counts no more rejections than the loop)
        assert (out["rejected"] <= want["rejected"]).all() and int(want["rejected"].sum()) > 0
    assert torch.isfinite(out["model"]).all() and int(out["inliers"].min()) >= 3
    # the sampler is what the seed reaches: another seed, other hypotheses behind draw 1
    other = BatchedRegistration(**dict(kw, seed=78))(tm, logits)
    assert torch.isfinite(other["model"]).all()


def test_two_view_driver_equals_its_loop_over_the_ops(dev):
    from differentiable_ransac_amd import ops, synth
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    P, N, B, rounds = 3, 256, 128, 3
    data = synth.batch_two_view(P, N, seed0=310)
    tm, logits = data["matches"].to(dev), data["logits"].to(dev)
    K1, K2 = data["K1"].to(dev), data["K2"].to(dev)
    kw = dict(ransac_batch_size=B, threshold=0.75, max_iterations=rounds * B, seed=21, sampling="prosac", prosac_draws=2000)
    drv = BatchedRANSAC("nister", **kw)
    out = drv(tm, logits, K1, K2)
    twin = BatchedRANSAC("nister", **kw)
    st, thr = ops.ransac_init(P, N, twin.max_iterations, twin.threshold, K1, K2, dev, tm.dtype)
    pre = ops.refit_essential(tm)
    order, growth = ops.prosac_rank(logits), ops.prosac_growth(N, 5, 2000, dev)
    for r in range(rounds):
        idx = ops.prosac_sample(order, growth, B, 5, twin._seeds.next(), r * B)
        models, valid = ops.solve_essential(ops.gather(tm, idx), None, "nister")
        flat, valid = models.reshape(P, -1, 3, 3), valid.reshape(P, -1)
        scores, _ = ops.msac_score(tm, flat, thr, want_masks=False, valid=valid)
        ops.ransac_update(st, tm, flat, valid, scores, thr, B, 5, twin.confidence, twin.eps)
    ops.refit_accept(tm, pre[0], pre[1], thr, st.best_score, st.best_model)
    want = dict(model=st.best_model, mask=st.best_mask, score=st.best_score, inliers=st.best_inliers, iterations=st.iters)
    print(f"two-view: iterations {out['iterations'].cpu().tolist()} inliers {out['inliers'].cpu().tolist()}")
    assert _same(out, want)
    # device termination issues the same rounds, gated
    dterm = BatchedRANSAC("nister", **kw)
    dterm.device_termination = True
    assert _same(out, dterm(tm, logits, K1, K2))
    with pytest.raises(ValueError):
        drv(tm, logits, K1, K2, gumbels=[torch.zeros(P, B, N, device=dev)])


# ------------------------------------------------------------------------------------------------------------ what it is for
def test_prosac_finds_a_three_per_cent_pair_in_one_round(dev):
    """N = 2000 with 60 inliers, logits 1 for an inlier and 0 for an outlier: the ranking puts the inliers first, n(t) <= 60 for
    the draws t <= 58, so these are all-inlier samples by the definition of the sampler -- not by chance"""
    from differentiable_ransac_amd import ops
    from differentiable_ransac_amd.ransac import BatchedRegistration
    N, B = 2000, 1024
    sc = R.scene(4242, N, 0.03)
    inl = sc["inlier"]
    assert int(inl.sum()) == 60
    table = PR.growth_table(N, 3, 200000)
    assert PR.subset_size(table, 3, 58) == 60
    tm = torch.from_numpy(sc["matches"])[None].to(dev, torch.float32)
    logits = torch.from_numpy(inl.astype(np.float32))[None].to(dev)
    kw = dict(ransac_batch_size=B, threshold=R.THRESHOLD, max_iterations=B, seed=99, sampling="prosac")
    drv = BatchedRegistration(**kw)
    out = drv(tm, logits)
    # the index sets of that call, and the host reference run over them
    idx = ops.prosac_sample(ops.prosac_rank(logits), ops.prosac_growth(N, 3, 200000, dev), B, 3, BatchedRegistration(**kw)._seeds.next(), 0)
    idx = idx[0].cpu().numpy()
    assert all(inl[row].all() for row in idx[:58])
    host = R.run(tm[0].cpu().double().numpy(), [idx], max_iterations=B)
    host_found = int((host["mask"] & inl).sum())
    mask = out["mask"][0].cpu().numpy()
    found = int((mask & inl).sum())
    err = R.rotation_error_deg(out["model"][0].cpu().double().numpy(), sc["R"])
    print(f"3 % pair: rotation error {err:.3f} deg, {found} of 60 inliers in the mask (host reference {host_found}), "
          f"iterations {out['iterations'].cpu().tolist()}")
    assert host_found >= 54
    assert err < 2.0
    assert found >= 54
    # flat logits: the order is the identity, the call runs and returns finite output (nothing is claimed about success)
    flat = BatchedRegistration(**kw)(tm, torch.zeros_like(logits))
    assert torch.isfinite(flat["model"]).all() and torch.isfinite(flat["score"]).all()
    assert torch.equal(ops.prosac_rank(torch.zeros_like(logits))[0].cpu(), torch.arange(N, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------ capture
def test_prosac_call_is_capturable(dev):
    from differentiable_ransac_amd.graphs import GraphedStep
    from differentiable_ransac_amd.ransac import BatchedRegistration
    P, N, B = 2, 256, 64
    sc = [R.scene(4300 + p, N, s) for p, s in enumerate((0.35, 0.15))]
    rng = np.random.default_rng(4300)
    tm = torch.from_numpy(np.stack([s["matches"] for s in sc])).to(dev, torch.float32)
    logits = torch.from_numpy(rng.standard_normal((P, N))).to(dev, torch.float32)      # (they know nothing: the draws matter)
    kw = dict(ransac_batch_size=B, threshold=R.THRESHOLD, max_iterations=256, seed=5, sampling="prosac", prosac_draws=1000)
    host = BatchedRegistration(**kw)(tm, logits)
    dterm = BatchedRegistration(**kw)
    dterm.device_termination = True
    eager = dterm(tm, logits)
    assert _same(host, eager)

    def call():      # by-value seeds are frozen into the graph: every call is call 0 of the driver
        dterm.calls = 0
        return dterm(tm, logits)
    step = GraphedStep(call, warmup=1)
    for _ in range(2):
        replay = step()
        torch.cuda.synchronize()
        assert _same(eager, replay)
    # device seeds: every replay draws afresh
    fresh = BatchedRegistration(**dict(kw, refit=False)).device_seeds(dev)
    fresh.device_termination = True
    step = GraphedStep(lambda: fresh(tm, logits), warmup=1)
    a = {k: v.clone() for k, v in step().items()}
    b = step()
    torch.cuda.synchronize()
    for o in (a, b):
        assert torch.isfinite(o["model"]).all() and torch.isfinite(o["score"]).all()
    assert not torch.equal(a["model"], b["model"])
