"""Round-3 additions: the HIP path on the realistic-logits fixture, the plain multi-rank launch of bench.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture():
    z = np.load(os.path.join(GOLDEN, "clnet_logits.npz"))
    return {k: torch.from_numpy(z[k]) for k in ("matches", "log_probs", "K1", "K2", "gt_E", "geometric_inliers")}


def test_clnet_logits_fixture_explicit_noise_vs_oracle(dev):
    """BatchedRANSAC("nister") on the four reader-produced pairs with the reference network's log-probabilities as the
    sampler input (datasets.py:16-129 -> model_cl.py:450-490) and EXPLICIT Gumbel noise, against the f64 oracle's test-mode
    run on the same noise: iteration counts equal, score within 1e-3, at most two mask bytes, model within 1e-4."""
    from differentiable_ransac_amd import synth
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    f = _fixture()
    P, N = f["matches"].shape[:2]
    B = 128
    noise = [synth.gumbel_noise((P, B, N), seed=700 + r) for r in range(3)]
    rn = BatchedRANSAC("nister", ransac_batch_size=B, threshold=0.75, max_iterations=3 * B, refit=False)
    out = rn(f["matches"].to(dev), f["log_probs"].to(dev), f["K1"].to(dev), f["K2"].to(dev),
             gumbels=[n.to(dev) for n in noise])
    for p in range(P):
        m, mask, score, it = O.ransac_test(f["matches"][p].double(), f["log_probs"][p].double(),
                                           [n[p].double() for n in noise], f["K1"][p].double(), f["K2"][p].double(),
                                           "nister", max_iterations=3 * B, refit=False)
        assert int(out["iterations"][p]) == it, (p, int(out["iterations"][p]), it)
        assert abs(float(out["score"][p]) - score) <= 1e-3 * max(1.0, score), (p, float(out["score"][p]), score)
        assert int((out["mask"][p].cpu() != mask).sum()) <= 2
        d = (O.canonical(out["model"][p].cpu().double()) - O.canonical(m)).abs().max()
        assert d < 1e-4, (p, float(d))


def test_clnet_logits_fixture_philox_run_finds_the_geometry(dev):
    """The same pairs with the in-kernel noise (what bench.py's `clnet_logits` sub-record times): the best mask agrees with the
    geometric inliers of the ground-truth pose on >= 90 % of the points."""
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    f = _fixture()
    rn = BatchedRANSAC("nister", ransac_batch_size=1024, threshold=0.75, max_iterations=1024, refit=False, seed=11)
    out = rn(f["matches"].to(dev), f["log_probs"].to(dev), f["K1"].to(dev), f["K2"].to(dev))
    agree = (out["mask"].cpu() == f["geometric_inliers"]).float().mean(-1)
    assert float(agree.mean()) >= 0.90, agree
    assert float(agree.min()) >= 0.85, agree


def test_bench_plain_launch_two_ranks_on_one_gpu():
    """`python bench.py --gpus 2` started plain starts two ranks itself (gloo + --gpus-shared: RCCL refuses two ranks on one
    device) and rank 0 prints n_gpus = n_ranks_seen = 2, in both modes."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    for mode in ("test", "train"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--gpus-shared",
                            "--steps", "4", "--warmup", "2", "--pairs", "8", "--segments", "3", "--prewarm-s", "0.1",
                            "--mode", mode, "--full", "--no-configs", "--no-cpu-baseline", "--no-extras"],
                           capture_output=True, text=True, env=env, timeout=240, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        rec = json.loads(lines[0])
        assert rec["n_gpus"] == 2 and rec["n_ranks_seen"] == 2 and rec["steps"] == 4
        assert rec["segments"]["n"] == 3 and len(rec["segments"]["ms_per_step"]) == 3
        assert rec["collective_ms"] is not None
        if mode == "train":
            assert rec["collective_ms"] > 0 and rec["grad_finite"]
            # round 6: the line says which pairs every rank owned and that step i + 1 was enqueued before the wait on bucket i
            part = rec["pair_partition"]
            assert part["total_pairs"] == 16 and part["ranges"] == [[0, 8], [8, 16]] and part["covers_once"] and part["equals_pair_range"]
            assert rec["overlap_trace_ok"] is True



def _bench_line(*flags, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True, env=env,
                       timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_plain_run_is_lean_and_dumps_the_same_outputs_every_run(tmp_path):
    """a plain run (no --full) times exactly --steps steps and prints the headline only; --dump-outputs writes what the last
    timed step returned, and since the sampler is rewound before the timed steps, two runs whose pre-conditioning issued
    different numbers of steps write the same arrays"""
    recs = []
    for tag, pre in (("a", "0.05"), ("b", "0.4")):
        recs.append(_bench_line("--gpus", "1", "--steps", "5", "--warmup", "2", "--pairs", "8", "--prewarm-s", pre,
                                "--dump-outputs", str(tmp_path / tag)))
    for rec in recs:
        assert rec["steps"] == 5 and rec["n_gpus"] == 1 and rec["unit"] == "hypotheses/s" and rec["dtype"] == "f32"
        assert rec["segments"]["n"] == 1 and len(rec["segments"]["ms_per_step"]) == 1 and rec["ms_per_step"] > 0
        assert rec["value"] > 0 and rec["higher_is_better"] is True
        assert not {"roofline", "configs", "cpu_baseline", "check", "two_batches_in_flight"} & set(rec)
    assert recs[0]["prewarm_steps"] != recs[1]["prewarm_steps"]
    files = sorted(f.name for f in (tmp_path / "a").iterdir())
    assert files == sorted(f.name for f in (tmp_path / "b").iterdir())
    assert {"model.npy", "mask.npy", "score.npy", "inliers.npy"} <= set(files)
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    assert np.load(tmp_path / "a" / "model.npy").shape == (8, 3, 3)
    assert np.load(tmp_path / "a" / "mask.npy").shape == (8, 2000)


def test_bench_plain_two_rank_run_is_lean(tmp_path):
    """the same lean path with two ranks (gloo, one shared GPU), in both modes: the headline fields, nothing of --full"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    for mode in ("test", "train"):
        rec = _bench_line("--gpus", "2", "--backend", "gloo", "--gpus-shared", "--steps", "4", "--warmup", "2", "--pairs", "8",
                          "--prewarm-s", "0.1", "--mode", mode, "--dump-outputs", str(tmp_path / mode), env=env)
        assert rec["n_gpus"] == 2 and rec["n_ranks_seen"] == 2 and rec["steps"] == 4 and rec["segments"]["n"] == 1
        assert rec["ms_per_step"] > 0 and rec["value"] > 0
        assert "roofline" not in rec
        if mode == "train":
            assert rec["collective_ms"] is None and rec["grad_finite"] is None and rec["pair_partition"] is None
            assert np.load(tmp_path / mode / "grad.npy").shape == (8, 2000)
        else:
            assert np.load(tmp_path / mode / "model.npy").shape == (8, 3, 3)

# ---------------------------------------------------------------------------------------------------------------------
# weighted LSQ refit of F (`-fmat 1 -wei 1 -tr 0`, ransac.py:151-153)
def test_weighted_fundamental_refit_kernel_vs_reference(dev):
    """dr_refit_fundamental (weights given) on (inliers of the reference run's best mask, the reference run's row-0 soft weights) against the
    reference estimator's own output (fixture generated by importing /root/reference) and the f64 oracle."""
    from differentiable_ransac_amd import ops
    from tests.conftest import load_golden
    g = load_golden("ransac_test_f8_weighted")
    for dt, tol in ((torch.float32, 2e-4), (torch.float64, 1e-9)):
        F, ok = ops.refit_fundamental(g["matches"].to(dev, dt)[None], g["best_mask"].to(dev)[None],
                                      g["refit_weights"].to(dev, dt)[None])
        assert bool(ok[0])
        inl = g["best_mask"].nonzero(as_tuple=True)[0]
        ref64 = O.fundamental_8pt(g["matches"].double()[inl][None], g["refit_weights"].double()[inl][None])[0]
        d = (O.canonical(F[0].cpu().double()) - O.canonical(ref64)).abs().max()
        assert d < tol, (dt, float(d))
        d_ref = (O.canonical(F[0].cpu().double()) - O.canonical(g["refit_candidate"].double())).abs().max()
        assert d_ref < 1e-3, float(d_ref)                  # the reference ran in f32
        if dt == torch.float64:      # the weights matter (the soft weights of this run span 1e-5 .. 0.76: in f32 the
            # ill-conditioned weighted problem and the plain one are closer than the f32 tolerance, in f64 they are far apart)
            plain, _ = ops.refit_fundamental(g["matches"].to(dev, dt)[None], g["best_mask"].to(dev)[None])
            assert (O.canonical(plain[0].cpu().double()) - O.canonical(ref64)).abs().max() > 1e-5
        # moderate weights (0.2 .. 1): a well-conditioned weighted problem, tight tolerance in both precisions
        wm = 0.2 + 0.8 * torch.rand(g["matches"].shape[0], generator=torch.Generator().manual_seed(8), dtype=torch.float64)
        Fm, okm = ops.refit_fundamental(g["matches"].to(dev, dt)[None], g["best_mask"].to(dev)[None], wm.to(dev, dt)[None])
        refm = O.fundamental_8pt(g["matches"].double()[inl][None], wm[inl][None])[0]
        refp = O.fundamental_8pt(g["matches"].double()[inl][None])[0]
        dm = (O.canonical(Fm[0].cpu().double()) - O.canonical(refm)).abs().max()
        assert bool(okm[0]) and dm < (2e-5 if dt == torch.float32 else 1e-9), (dt, float(dm))
        assert (O.canonical(refm) - O.canonical(refp)).abs().max() > 20 * dm


@pytest.mark.parametrize("fused", [True, False])
def test_weighted_fundamental_test_mode_matches_reference_run(dev, fused):
    """The drop-in RANSAC (fmat, weighted=1, test mode) on the reference run's recorded noise: weighted minimal solves and the
    weighted refit, fused (BatchedRANSAC, per-pair "last batch" weights on the device) and per-batch (plugin path)."""
    from differentiable_ransac_amd.estimators import FundamentalMatrixEstimatorNew
    from differentiable_ransac_amd.ransac import RANSAC
    from differentiable_ransac_amd.samplers import GumbelSoftmaxSampler
    from differentiable_ransac_amd.scorings import MSACScore
    from tests.conftest import load_golden
    g = load_golden("ransac_test_f8_weighted")
    r = RANSAC(FundamentalMatrixEstimatorNew("cuda"), GumbelSoftmaxSampler(16, 8, device="cuda"), MSACScore("cuda"), fmat=True,
               train=False, ransac_batch_size=16, sampler_id=3, weighted=1, threshold=0.75, max_iterations=5000)
    r.fused = fused
    model, mask, score, iters = r(g["matches"].to(dev), g["logits"].to(dev), g["K1"].to(dev), g["K2"].to(dev), None,
                                  gumbels=[x.to(dev) for x in g["gumbels"]])
    dt = torch.float64
    mo, masko, so, ito = O.ransac_test(g["matches"].to(dt), g["logits"].to(dt), [x.to(dt) for x in g["gumbels"]],
                                       g["K1"].to(dt), g["K2"].to(dt), "f8", weighted=True)
    assert iters == ito == g["iterations"]
    assert int((mask.cpu() != masko).sum()) <= 1
    assert abs(float(score) - so) <= 1e-3 * max(1.0, so)
    assert (O.canonical(model.cpu().double()) - O.canonical(mo)).abs().max() < 1e-4
    # the reference's own f32 run: same ballpark, not the arbiter -- its weighted refit is ill-conditioned in f32 (weights span
    # 1e-5 .. 0.76) and wins there with a score the f64 solve does not reach (46.8 against 44.5; the f32 CPU oracle reproduces
    # the reference's figure to 1e-3, tests/test_oracle_golden.py)
    assert abs(float(score) - g["best_score"]) <= 0.1 * max(1.0, g["best_score"])


# ---------------------------------------------------------------------------------------------------------------------
# K6 of the 3-D path on the device (dr_ransac3d_update)
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_ransac3d_update_kernel(dev, dt):
    from differentiable_ransac_amd import ops
    g = torch.Generator().manual_seed(3)
    P, M, N = 5, 300, 5000
    pts = torch.rand(P, N, 6, generator=g, dtype=dt)
    models = torch.eye(4, dtype=dt).repeat(P, M, 1, 1)
    models[:, :, :3, 3] = 0.2 * torch.randn(P, M, 3, generator=g, dtype=dt)
    models[:, :, :3, :3] += 0.05 * torch.randn(P, M, 3, 3, generator=g, dtype=dt)
    valid = torch.rand(P, M, generator=g) < 0.7
    res = torch.rand(P, M, generator=g, dtype=dt) * 10 + 1
    res[0, 17] = float("nan")
    res[1, 5] = res[1, 200] = 0.5                 # a tie: the lower index wins
    valid[1, 5] = valid[1, 200] = True
    valid[2] = False                              # no valid model: the state is kept
    best = torch.full((P,), float("inf"), dtype=dt)
    best[3] = 0.0                                 # nothing beats it: kept
    bm = torch.eye(4, dtype=dt).repeat(P, 1, 1) * 7
    mask = torch.zeros(P, N, dtype=torch.bool)
    thr = 0.08
    nb, nm, idx = ops.ransac3d_update(pts.to(dev), models.to(dev), valid.to(dev), res.to(dev), thr, best.to(dev), bm.to(dev),
                                      (dmask := mask.to(dev)))
    key = torch.where(valid & ~torch.isnan(res), res, torch.full_like(res, float("inf")))
    val, b = key.min(1)
    for p in range(P):
        first = int((key[p] == val[p]).nonzero()[0]) if torch.isfinite(val[p]) else -1
        better = first >= 0 and float(val[p]) < float(best[p])
        assert int(idx[p]) == (first if better else -1), (p, int(idx[p]), first)
        if better:
            assert float(nb[p]) == float(res[p, first]) and torch.equal(nm[p].cpu(), models[p, first])
            T = models[p, first]
            d2 = ((pts[p, :, 3:] - (pts[p, :, :3] @ T[:3, :3].T + T[:3, 3])) ** 2).sum(-1)
            wrong = (dmask[p].cpu() != (d2 < thr))
            assert int(wrong.sum()) <= (2 if dt == torch.float32 else 0)
        else:
            assert float(nb[p]) == float(best[p]) and torch.equal(nm[p].cpu(), bm[p]) and not bool(dmask[p].any())
    assert int(idx[1]) == 5 and int(idx[2]) == -1 and int(idx[3]) == -1
    # a second round with worse sums keeps everything
    nb2, nm2, idx2 = ops.ransac3d_update(pts.to(dev), models.to(dev), valid.to(dev), (res + 100).to(dev), thr, nb, nm, dmask)
    assert torch.equal(nb2[[0, 1, 3, 4]], nb[[0, 1, 3, 4]]) and torch.equal(nm2, nm) and (idx2.cpu()[[0, 1, 3, 4]] == -1).all()


def test_rigid_residual_16_point_kernel_vs_general(dev):
    """The 16-points-per-lane kernel (clamped-difference mask bits, grouped model fetch, 16-model tiles) against the general
    kernel on ragged model counts and several chunk splits: identical masks, sums to reduction-order rounding."""
    from differentiable_ransac_amd import ops, synth
    for N, M, seed in ((4096, 37, 1), (50000, 70, 2), (2048 * 3 + 16, 16, 3), (16, 5, 4)):
        rp = synth.rigid_pair(seed, N)
        g = torch.Generator().manual_seed(seed)
        models = torch.eye(4).repeat(M, 1, 1)
        models[:, :3, :] = rp["gt_T"][:3, :].float()[None] + 0.02 * torch.randn(M, 3, 4, generator=g)
        pts = rp["matches"].float().to(dev)[None]
        res, masks = ops.rigid_residual(pts, models.to(dev)[None], 0.03, True)          # N % 16 == 0 -> the 16-point kernel
        res_g, _ = ops.rigid_residual(pts, models.to(dev)[None], 0.03, False)           # no masks -> the general kernel
        assert ((res - res_g).abs() / res_g).max() < 2e-5
        T = models.double()
        p3, q3 = rp["matches"][:, :3].double(), rp["matches"][:, 3:].double()
        d2 = ((q3[None] - (p3[None] @ T[:, :3, :3].transpose(-1, -2) + T[:, None, :3, 3])) ** 2).sum(-1)
        near = (d2 - 0.03).abs() < 1e-6
        assert bool(((masks[0].cpu() == (d2 < 0.03)) | near).all())
        assert ((res[0].cpu().double() - d2.sum(-1)).abs() / d2.sum(-1)).max() < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# MatchLoss residual kernel (32 models per block, points resident when they fit one pass): the paths the training shape does
# not take -- several 2048-point chunks, more than 1024 selected points per chunk, a ragged model count, no mask
@pytest.mark.parametrize("N,M,frac", [(5000, 45, 0.7), (2048, 33, 0.9), (6000, 70, None), (300, 3, 0.5)])
def test_episym_sums_and_gradients_long_rows(dev, N, M, frac):
    from differentiable_ransac_amd import ops, synth
    P = 2
    data = synth.batch_two_view(P, N, seed0=900 + N)
    gen = torch.Generator().manual_seed(N + M)
    models = data["gt_E"][:, None] + 0.05 * torch.randn(P, M, 3, 3, generator=gen)
    mask = None if frac is None else (torch.rand(P, N, generator=gen) < frac)
    valid = torch.rand(P, M, generator=gen) > 0.2
    md = models.to(dev).requires_grad_(True)
    sums = ops.episym_sums(data["matches"].to(dev), None if mask is None else mask.to(dev), md, valid.to(dev))
    gw = torch.randn(P, M, generator=gen)
    (sums * gw.to(dev)).sum().backward()
    m64 = models.double().requires_grad_(True)
    tot = 0
    for p in range(P):
        sel = torch.ones(N, dtype=torch.bool) if mask is None else mask[p]
        ys = O.episym(data["matches"][p, sel, :2].double(), data["matches"][p, sel, 2:].double(), m64[p])
        ref = torch.clamp(ys, max=1.0).sum(1)
        got = sums[p].detach().cpu().double()
        assert ((got - ref.detach()).abs()[valid[p]] / ref.detach()[valid[p]]).max() < 1e-4
        assert (got[~valid[p]] == 0).all()
        tot = tot + (ref * gw[p].double() * valid[p].double()).sum()
    tot.backward()
    g, gr = md.grad.cpu().double(), m64.grad
    assert (g[~valid] == 0).all()
    assert (g - gr).abs().max() <= 3e-4 * gr.abs().max()


# ---------------------------------------------------------------------------------------------------------------------
# K4 for short rows (a wave per model): every points-per-lane variant, ragged rows, invalid slots, non-finite / zero models,
# several pairs -- against the f64 oracle and against the long-row kernels' conventions
@pytest.mark.parametrize("N", [1, 7, 64, 65, 128, 130, 200, 256])
def test_msac_short_row_kernel(dev, N):
    from differentiable_ransac_amd import ops, synth
    from tests.test_gpu_msac import _check_scores_masks, _margin
    P, M = 3, 45
    b = synth.batch_two_view(P, max(N, 8), seed0=700 + N)
    matches = b["matches"][:, :N].contiguous()
    gen = torch.Generator().manual_seed(N)
    models = b["gt_E"][:, None] + 0.05 * torch.randn(P, M, 3, 3, generator=gen)
    models[:, 0] = b["gt_E"]
    models[0, 3, 1, 1] = float("nan")
    models[1, 4] = float("inf")
    models[2, 5] = 0.0                                           # all-zero model: NaN score, empty mask (reference: 0/0)
    valid = torch.rand(P, M, generator=gen) > 0.3
    valid[0, 3] = valid[1, 4] = valid[2, 5] = valid[:, 0] = True
    thr = torch.tensor([7.5e-4, 1e-3, 5e-4])
    s, k = ops.msac_score(matches.to(dev), models.to(dev), thr.to(dev), True, valid.to(dev))
    s_nomask, none = ops.msac_score(matches.to(dev), models.to(dev), thr.to(dev), False, valid.to(dev))
    assert none is None and torch.equal(torch.nan_to_num(s_nomask, nan=-7.0), torch.nan_to_num(s, nan=-7.0))
    for p in range(P):
        rs, rm = O.msac_score(matches[p].double(), models[p].double(), float(thr[p]))
        fin = torch.isfinite(models[p]).all(-1).all(-1) & (models[p].abs().amax((-1, -2)) > 0)
        ok = valid[p] & fin
        _check_scores_masks(s[p][ok], k[p][ok], rs[ok], rm[ok], _margin(matches[p], models[p], float(thr[p]), 2e-5)[ok])
        bad = valid[p] & ~fin
        assert torch.isnan(s[p][bad]).all() and not k[p][bad].any()
        assert (s[p][~valid[p]] == 0).all() and not k[p][~valid[p]].any()
    # without a validity mask every slot is evaluated
    s_all, k_all = ops.msac_score(matches.to(dev), models.to(dev), thr.to(dev))
    fin_all = torch.isfinite(models).all(-1).all(-1) & (models.abs().amax((-1, -2)) > 0)
    sel = (valid & fin_all).to(dev)
    assert torch.equal(s_all[sel], s[sel]) and torch.equal(k_all[sel], k[sel])


# ---------------------------------------------------------------------------------------------------------------------
# train-step glue folded into kernels: keep flag from K5, MatchLoss mean + its backward
def test_select_closest_keep_flag_and_fused_match_loss_mean(dev):
    from differentiable_ransac_amd import ops, synth
    from differentiable_ransac_amd.loss import MatchLoss
    for P in (3, 70):                                    # 70 > 64: the per-pair kernel + torch.mean fallback
        N, B = 400, 24
        data = synth.batch_two_view(P, N, seed0=1200 + P)
        gen = torch.Generator().manual_seed(P)
        models = (data["gt_E"][:, None, None] + 0.05 * torch.randn(P, B, 10, 3, 3, generator=gen)).to(dev)
        valid = (torch.rand(P, B, 10, generator=gen) > 0.6).to(dev)
        valid[0, 0] = False                              # a sample with no valid slot: which = -1, keep = False
        md = models.clone().requires_grad_(True)
        chosen, which, keep = ops.select_closest_autograd(md, valid, data["gt_E"].to(dev), want_keep=True)
        assert keep.dtype == torch.bool and torch.equal(keep, which >= 0) and not bool(keep[0, 0])
        c2, w2 = ops.select_closest_autograd(models, valid, data["gt_E"].to(dev))
        assert torch.equal(w2, which) and torch.equal(c2, chosen.detach())
        mask = data["inliers"].to(dev)
        loss = MatchLoss()(chosen, data["matches"].to(dev), mask, keep)
        assert loss.dim() == 0
        loss.backward(torch.full((), 2.5, device=dev))   # an upstream gradient other than 1
        ch2 = chosen.detach().clone().requires_grad_(True)
        ref = ops.match_loss_per_pair(data["matches"].to(dev), mask, ch2, keep).mean()
        (2.5 * ref).backward()
        assert abs(float(loss) - float(ref)) <= 2e-6 * abs(float(ref))
        # gradient w.r.t. the chosen models through both routes (the fused one arrives at `md` through K5's backward)
        g_ref = torch.zeros_like(models)
        idx = which.clamp(min=0).long()
        g_ref[torch.arange(P, device=dev)[:, None], torch.arange(B, device=dev)[None], idx] = ch2.grad * keep[..., None, None]
        assert (md.grad - g_ref).abs().max() <= 1e-5 * g_ref.abs().max()


def test_fused_solve_select_node_equals_the_two_node_route(dev):
    """BatchedRANSAC train mode (sampler -> solver + best-of-ten as one autograd node, sparse gradient into the solver's
    backward) against the two-node route (ops.solve_essential + ops.select_closest_autograd: dense [P,B,10,9] gradient) on the
    same explicit noise: same chosen models, same keep flags, same gradient w.r.t. the logits."""
    from differentiable_ransac_amd import ops, synth
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    P, N, B = 3, 600, 96
    data = synth.batch_two_view(P, N, seed0=1300)
    noise = synth.gumbel_noise((P, B, N), seed=77).to(dev)
    m, gt = data["matches"].to(dev), data["gt_E"].to(dev)
    W = torch.randn(P, B, 3, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    lg1 = data["logits"].to(dev).clone().requires_grad_(True)
    tr = BatchedRANSAC("nister", ransac_batch_size=B, train=True, max_iterations=B)
    chosen1, keep1 = tr(m, lg1, gt_model=gt, gumbels=[noise])
    (chosen1 * W * keep1[..., None, None]).sum().backward()
    lg2 = data["logits"].to(dev).clone().requires_grad_(True)
    samples, _, _ = ops.SampleGather.apply(m, lg2, B, 5, 1.0, noise, 0)
    models, valid = ops.solve_essential(samples, None, "nister")
    chosen2, which2 = ops.select_closest_autograd(models, valid, gt)
    keep2 = which2 >= 0
    (chosen2 * W * keep2[..., None, None]).sum().backward()
    assert torch.equal(keep1, keep2) and torch.equal(chosen1.detach(), chosen2.detach())
    assert float(lg2.grad.abs().max()) > 0
    assert (lg1.grad - lg2.grad).abs().max() <= 1e-6 * lg2.grad.abs().max()


def test_ransac3d_update_first_round_without_state(dev):
    """best_res = best_model = None: "no state yet" -- the same result as the explicit +inf / identity / empty-mask state, and
    a fully defined mask even for a pair with no valid model."""
    from differentiable_ransac_amd import ops
    g = torch.Generator().manual_seed(9)
    P, M, N = 4, 64, 3000
    pts = torch.rand(P, N, 6, generator=g).to(dev)
    models = torch.eye(4).repeat(P, M, 1, 1)
    models[:, :, :3, 3] = 0.1 * torch.randn(P, M, 3, generator=g)
    models = models.to(dev)
    valid = (torch.rand(P, M, generator=g) < 0.8).to(dev)
    valid[2] = False
    res = (torch.rand(P, M, generator=g) * 5 + 1).to(dev)
    mask_a = torch.ones(P, N, dtype=torch.bool, device=dev)          # garbage the kernel must overwrite
    ra, ma, ia = ops.ransac3d_update(pts, models, valid, res, 0.05, None, None, mask_a)
    mask_b = torch.zeros(P, N, dtype=torch.bool, device=dev)
    rb, mb, ib = ops.ransac3d_update(pts, models, valid, res, 0.05, torch.full((P,), float("inf"), device=dev),
                                     torch.eye(4, device=dev).repeat(P, 1, 1), mask_b)
    assert torch.equal(ra, rb) and torch.equal(ma, mb) and torch.equal(ia, ib) and torch.equal(mask_a, mask_b)
    assert int(ia[2]) == -1 and not bool(mask_a[2].any()) and torch.equal(ma[2].cpu(), torch.eye(4))


def test_fivepoint_nonminimal_backward_finite_difference(dev):
    """`-sam 3 -fmat 0 -tr 1` (ransac.py:82-83: 8-point Gumbel sampler feeding the five-point estimator, which runs its
    minimal code on all eight rows, nister.py:64-65): the implicit derivative of the invariant subspace + essential-manifold
    constraints (dr_solve_nister5_nm_bwd_f32) against central finite differences of the f64 CPU oracle, samples AND row
    weights, each solution tracked by proximity and sign-aligned."""
    from differentiable_ransac_amd import ops, synth
    from oracle import cpu_ref as O
    pair = synth.two_view_pair(91, 200, inlier_ratio=1.0, noise=2e-3, dtype=torch.float64)
    B, n = 8, 8
    smp = pair["matches"][: n * B].reshape(B, n, 4).contiguous()
    gen = torch.Generator().manual_seed(5)
    wts = (0.5 + torch.rand(B, n, generator=gen, dtype=torch.float64)).float().double()
    W = torch.randn(B, 10, 3, 3, generator=gen, dtype=torch.float64)
    for weighted in (False, True):
        s32 = smp.float().to(dev).requires_grad_(True)
        w32 = wts.float().to(dev).requires_grad_(True) if weighted else None
        E, valid = ops.solve_essential(s32, w32, "nister")
        assert int(valid.sum()) >= B          # at least the true model per sample
        (E * W.float().to(dev) * valid[..., None, None]).sum().backward()
        g = s32.grad.cpu().double()
        E0, v0 = E.detach().cpu().double(), valid.cpu()

        def loss_cpu(xb, wb, b):
            Eo, ok, real = O.nister_5pt(xb[None], None if wb is None else wb[None])
            tot = torch.zeros((), dtype=torch.float64)
            for sl in range(10):
                if not bool(v0[b, sl]):
                    continue
                cand = Eo[0][real[0]]
                d1 = (cand - E0[b, sl]).abs().amax((-1, -2))
                d2 = (cand + E0[b, sl]).abs().amax((-1, -2))
                j = torch.minimum(d1, d2).argmin()
                sgn = 1.0 if d1[j] <= d2[j] else -1.0
                tot = tot + (sgn * cand[j] * W[b, sl]).sum()
            return tot

        eps = 2e-5
        base = smp.float().double()
        num = torch.zeros_like(smp)
        numw = torch.zeros_like(wts)
        for b in range(B):
            wb = wts[b] if weighted else None
            for k in range(n):
                for d in range(4):
                    xp, xm = base[b].clone(), base[b].clone()
                    xp[k, d] += eps
                    xm[k, d] -= eps
                    num[b, k, d] = (loss_cpu(xp, wb, b) - loss_cpu(xm, wb, b)) / (2 * eps)
                if weighted:
                    wp, wm = wts[b].clone(), wts[b].clone()
                    wp[k] += eps
                    wm[k] -= eps
                    numw[b, k] = (loss_cpu(base[b], wp, b) - loss_cpu(base[b], wm, b)) / (2 * eps)
        rel = (g - num).abs().amax((-1, -2)) / num.abs().amax((-1, -2)).clamp(min=1e-9)
        assert rel.median() < 1e-3 and rel.max() < 2e-2, (weighted, rel.median(), rel.max())
        if weighted:
            gw = w32.grad.cpu().double()
            relw = (gw - numw).abs().amax(-1) / numw.abs().amax(-1).clamp(min=1e-9)
            assert relw.median() < 1e-3 and relw.max() < 2e-2, (relw.median(), relw.max())


def test_train_path_eight_point_sampler_into_five_point_estimator(dev):
    """The reference's `-sam 3 -fmat 0 -tr 1` through both drivers: every verified model of every 8-point sample comes back
    (ransac.py:82-83 keeps all estimated models), and the logits receive a finite, non-zero gradient."""
    from differentiable_ransac_amd import synth
    from differentiable_ransac_amd.estimators import EssentialMatrixEstimatorNister
    from differentiable_ransac_amd.ransac import RANSAC, BatchedRANSAC
    from differentiable_ransac_amd.samplers import GumbelSoftmaxSampler
    from differentiable_ransac_amd.scorings import MSACScore
    P, N, B = 2, 300, 32
    data = synth.batch_two_view(P, N, seed0=75, inlier_ratio=0.9)
    gt = data["gt_E"].to(dev)
    lg = data["logits"].to(dev).requires_grad_(True)
    tr = BatchedRANSAC("nister", ransac_batch_size=B, train=True, max_iterations=B, num_samples=8)
    chosen, keep = tr(data["matches"].to(dev), lg, gt_model=gt)
    assert chosen.shape == (P, B * 10, 3, 3) and keep.shape == (P, B * 10) and int(keep.sum()) >= P * B
    d = torch.minimum(((chosen - gt[:, None]) ** 2).sum((-1, -2)), ((chosen + gt[:, None]) ** 2).sum((-1, -2)))
    d[keep].mean().backward()
    assert torch.isfinite(lg.grad).all() and float(lg.grad.abs().sum()) > 0
    # the per-pair driver (reference constructor signature)
    lg1 = data["logits"][0].to(dev).requires_grad_(True)
    r = RANSAC(EssentialMatrixEstimatorNister(device="cuda"), GumbelSoftmaxSampler(B, 8, device="cuda"), MSACScore("cuda"),
               train=True, ransac_batch_size=B, sampler_id=3, max_iterations=B)
    K = torch.eye(3, device=dev)
    models_out, _, _, _ = r(data["matches"][0].to(dev), lg1, K, K, gt[0])
    models = models_out[0]
    assert models.shape[-2:] == (3, 3) and models.shape[0] >= B
    dd = torch.minimum(((models - gt[0]) ** 2).sum((-1, -2)), ((models + gt[0]) ** 2).sum((-1, -2)))
    dd.mean().backward()
    assert torch.isfinite(lg1.grad).all() and float(lg1.grad.abs().sum()) > 0


def test_sturm_isolation_finds_the_real_roots_the_oracle_finds(dev):
    """K3's root isolation (Sturm sequence) at scale: on 8192 RANSAC-like minimal samples (mixed inliers / outliers
    of four pairs) the verified solutions are the oracle's real solutions -- same count to 1e-3, and 99.8 % of either set has its
    partner in the other within the f32 output tolerance.  Nister and Stewenius share the isolation."""
    from differentiable_ransac_amd import ops, synth
    from oracle import cpu_ref as O
    gen = torch.Generator().manual_seed(21)
    smp = []
    for p in range(4):
        pair = synth.two_view_pair(300 + p, 600, inlier_ratio=0.6, noise=1e-3, dtype=torch.float64)
        idx = torch.stack([torch.randperm(600, generator=gen)[:5] for _ in range(2048)])
        smp.append(pair["matches"][idx])
    smp = torch.cat(smp).float()
    Eo, ok, real = O.nister_5pt(smp.double())
    n_real = int(real[ok].sum())
    for fn in (ops.solve_nister5, ops.solve_stewenius5):
        E, valid = fn(smp.to(dev))
        E, valid = E.cpu().double(), valid.cpu()
        n_valid = int(valid[ok].sum())
        assert abs(n_valid - n_real) <= 1e-3 * n_real + 2, (fn.__name__, n_valid, n_real)
        fw = torch.cat([O.match_solution_sets(E[b], valid[b], Eo[b], real[b]) for b in range(0, smp.shape[0], 8) if bool(ok[b])])
        bw = torch.cat([O.match_solution_sets(Eo[b], real[b], E[b], valid[b]) for b in range(0, smp.shape[0], 8) if bool(ok[b])])
        assert (fw > 1e-4).float().mean() < 2e-3 and (bw > 1e-4).float().mean() < 2e-3, (fn.__name__, fw.max(), bw.max())
