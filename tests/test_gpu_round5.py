"""Round 5 on the GPU: the two-phase five-point kernels (one lane per sample for the front stage, hand-over in accumulation
registers: dr_solve_nister5_f32 / dr_solve_stewenius5_f32 with path = 2) against the f64 CPU oracle and against the
lane-pair kernels they replace on large grids.  Reference: nister.py:69-408, stewenius.py:20-80."""
import pytest
import torch

from oracle import cpu_ref as O
from tests.test_gpu_solvers import TOL, _kat_essential, _set_dist

pytestmark = pytest.mark.gpu


def _samples(dev, n_rows, seed=3):
    from differentiable_ransac_amd import ops, synth
    pair = synth.two_view_pair(seed, 2000)
    r = ops.gumbel_topk(pair["logits"][None].to(dev), n_rows, 5, 1.0, None, seed)
    return ops.gather(pair["matches"][None].to(dev), r["idx"])[0]


@pytest.mark.parametrize("solver", ["nister", "stewenius"])
def test_two_phase_fivepoint_vs_oracle(dev, solver):
    """forced two-phase path (path = 2) at a size with a partial block (1000 = 15 x 64 + 40: the last block's second half holds
    8 samples) against the f64 oracle: same tolerances as the lane-pair kernels in test_gpu_solvers.py"""
    from differentiable_ransac_amd import ops
    smp = _samples(dev, 1000)
    fn = ops.solve_nister5 if solver == "nister" else ops.solve_stewenius5
    E, valid = fn(smp, path=2)
    E, valid = E.cpu().double(), valid.cpu()
    _kat_essential(E, valid, smp.cpu().double(), tol=2e-5)
    Eo, ok, real = O.nister_5pt(smp.cpu().double())
    fw, bw = _set_dist(E[ok], valid[ok], Eo[ok], real[ok])
    assert fw.quantile(0.995) < TOL and bw.quantile(0.995) < TOL, (fw.max(), bw.max())
    # round 6: the bars of the lane-pair test (test_gpu_solvers.py: 1e-3, +-4) -- the kernel on the headline path is held to them too
    assert (fw > TOL).float().mean() < 1e-3 and (bw > TOL).float().mean() < 1e-3
    assert abs(int(valid.sum()) - int(real[ok].sum())) <= 4


@pytest.mark.parametrize("rows", [1, 33, 64, 97, 4096])
def test_two_phase_fivepoint_equals_lane_pairs(dev, rows):
    """same solutions in the same slots as the lane-pair kernels (different elimination order in f64: the f32 models agree to
    rounding; a verification decided by the last bit may flip a slot -- at most a handful in 40 960)"""
    from differentiable_ransac_amd import ops
    smp = _samples(dev, rows, seed=11)
    for fn in (ops.solve_nister5, ops.solve_stewenius5):
        Ea, va = fn(smp, path=1)
        Eb, vb = fn(smp, path=2)
        flips = int((va != vb).sum())
        assert flips <= max(2, rows // 500), flips
        same = (va & vb)
        if same.any():
            d = (Ea[same] - Eb[same]).abs().amax((-1, -2))
            assert d.quantile(0.999) < 2e-6, d.max()
            assert (d > 1e-4).float().mean() < 1e-3
        eye = torch.eye(3, device=dev)
        assert (Eb[~vb] == eye).all()


def test_two_phase_nister_train_entry_and_weights(dev):
    """the f64 second output (train mode) and the weighted rows through the two-phase kernel"""
    from differentiable_ransac_amd import ops
    smp = _samples(dev, 300, seed=5)
    w = torch.rand(300, 5, device=dev) + 0.5
    m32a, m64a, va = ops.solve_nister5_hp(smp, w, path=1)
    m32b, m64b, vb = ops.solve_nister5_hp(smp, w, path=2)
    assert int((va != vb).sum()) <= 2
    same = va & vb
    assert (m64a[same] - m64b[same]).abs().max() < 1e-9
    assert torch.equal(m32b, m64b.float())
    Eo, ok, real = O.nister_5pt(smp.cpu().double(), w.cpu().double())
    fw, bw = _set_dist(m64b.cpu()[ok], vb.cpu()[ok], Eo[ok], real[ok])
    assert fw.quantile(0.99) < 1e-6 and bw.quantile(0.99) < 1e-6


def test_two_phase_automatic_choice_at_config_size(dev):
    """131 072 samples (BASELINE configs[1] at 128 pairs per step, configs[2]): the automatic path takes the two-phase kernels
    and returns what the forced path returns, bit for bit; degenerate inputs never produce NaN"""
    from differentiable_ransac_amd import ops
    smp = _samples(dev, 4096, seed=7).repeat(32, 1, 1).contiguous()
    smp[5] = 0.0
    smp[6] = float("nan")
    for fn in (ops.solve_nister5, ops.solve_stewenius5):
        Ea, va = fn(smp)
        Eb, vb = fn(smp, path=2)
        assert torch.equal(va, vb) and torch.equal(Ea, Eb)
        assert torch.isfinite(Ea).all() and not va[6].any()
        # the 32 copies of the 4096 samples give identical results wherever they sit in the grid
        ref = Ea[:4096]
        for c in (1, 17, 31):
            blk = Ea[4096 * c:4096 * (c + 1)]
            assert torch.equal(blk[7:], ref[7:])


# ------------------------------------------------------------------------------------- device-side termination, the drop-in as a graph
def _hard_pairs(dev, P, N=2000, pixel=False):
    """pairs with inlier ratios from 0.5 down to 0.2: the adaptive bound of ransac.py:135-144 asks for 1 to 5 batches of 1024"""
    from differentiable_ransac_amd import synth
    items = [synth.two_view_pair(100 + p, N, inlier_ratio=(0.5, 0.3, 0.2, 0.35)[p % 4], pixel=pixel) for p in range(P)]
    st = lambda k: torch.stack([it[k] for it in items]).to(dev)
    return st("matches"), st("logits"), st("K1"), st("K2")


@pytest.mark.parametrize("solver", ["nister", "stewenius", "f8"])
def test_device_termination_equals_the_host_loop(dev, solver):
    """every round issued, the kernels of a round skipping the pairs that have terminated (gated entry points), against the
    driver that reads the per-pair counters back after every round: same best model, mask, score and iteration count"""
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    m, lg, K1, K2 = _hard_pairs(dev, 4, pixel=solver == "f8")
    kw = dict(ransac_batch_size=1024, threshold=0.75, max_iterations=5000, seed=11, refit=True)
    host = BatchedRANSAC(solver, **kw)
    devt = BatchedRANSAC(solver, **kw)
    devt.device_termination = True
    for call in range(2):
        a = host(m, lg, K1, K2)
        b = devt(m, lg, K1, K2)
        for key in ("model", "mask", "score", "inliers", "iterations"):
            assert torch.equal(a[key], b[key]), (key, call)
    its = a["iterations"].tolist()
    assert max(its) >= 3072, its
    if solver != "f8":                                      # (eight-point samples at these inlier ratios: every pair runs all five batches)
        assert min(its) < max(its), its                     # the pairs really stop after different numbers of batches


@pytest.mark.parametrize("solver,B", [("nister", 8), ("stewenius", 8), ("nister", 2)])
def test_device_termination_with_solver_blocks_spanning_many_pairs(dev, solver, B):
    """round-5 advice (medium): with ransac_batch_size below half a solver block a block of samples spans three or more pairs; the
    gate must look at EVERY pair of the block, not only at the first and the last -- here 2304 pairs x 8 (or 2) samples
    (32- / 8-sample blocks = four pairs each) laid out closed | open | open | closed after the first round"""
    from differentiable_ransac_amd import synth
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    P = 2304
    items = [synth.two_view_pair(300 + q, 64, inlier_ratio=(0.95, 0.4, 0.4, 0.95)[q % 4], noise=1e-4) for q in range(8)]
    st = lambda k: torch.stack([items[p % 8][k] for p in range(P)]).to(dev)
    m, lg, K1, K2 = st("matches"), st("logits"), st("K1"), st("K2")
    kw = dict(ransac_batch_size=B, threshold=0.75, max_iterations=4 * B, seed=5, refit=False)
    host = BatchedRANSAC(solver, **kw)
    devt = BatchedRANSAC(solver, **kw)
    devt.device_termination = True
    a = host(m, lg, K1, K2)
    b = devt(m, lg, K1, K2)
    for key in ("model", "mask", "score", "inliers", "iterations"):
        assert torch.equal(a[key], b[key]), key
    its = a["iterations"].view(-1, 4)
    assert int(its.min()) < 4 * B and int(its.max()) == 4 * B
    # the layout the bug needs: blocks whose edge pairs have stopped while a middle pair has not
    edge_closed = (its[:, 0] < 4 * B) & (its[:, 3] < 4 * B) & ((its[:, 1] == 4 * B) | (its[:, 2] == 4 * B))
    assert int(edge_closed.sum()) > 50, int(edge_closed.sum())


def test_dropin_ransac_replays_a_graph_per_call(dev):
    """RANSAC.__call__ (test mode, this package's plugins, max_iterations <= 8 batches) = one replayed HIP graph per pair:
    pair after pair the results of a BatchedRANSAC with the same base seed, seeds and termination on the device, run eagerly;
    the tensors handed out stay what they were when the next pair overwrites the graph's buffers"""
    from differentiable_ransac_amd import estimators, samplers, scorings
    from differentiable_ransac_amd.ransac import RANSAC, BatchedRANSAC
    m, lg, K1, K2 = _hard_pairs(dev, 6)
    smp = samplers.GumbelSoftmaxSampler(1024, 5, device=dev, seed=3)
    rn = RANSAC(estimators.EssentialMatrixEstimatorNister(dev), smp, scorings.MSACScore(dev), train=False,
                ransac_batch_size=1024, sampler_id=2, threshold=0.75, max_iterations=5000)
    base = (3 * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)          # the sampler's first seed: the graph's base seed
    ref = BatchedRANSAC("nister", ransac_batch_size=1024, threshold=0.75, max_iterations=5000, seed=base, refit=True).device_seeds(dev)
    ref.device_termination = True
    for _ in range(2):                                         # the two warm-up calls of the capture advanced the device seed
        ref(m[:1], lg[:1], K1[:1], K2[:1])
    ref.calls = 0
    kept = []
    for p in range(6):
        model, mask, score, iters = rn(m[p], lg[p], K1[p], K2[p], None)
        want = ref(m[p:p + 1], lg[p:p + 1], K1[p:p + 1], K2[p:p + 1])
        assert torch.equal(model, want["model"][0]) and torch.equal(mask, want["mask"][0])
        assert torch.equal(score, want["score"][0]) and int(iters) == int(want["iterations"][0])
        kept.append((model, mask, score.clone(), want["model"][0].clone(), want["mask"][0].clone()))
    for model, mask, _, wm, wk in kept:
        assert torch.equal(model, wm) and torch.equal(mask, wk)
    assert len(rn._graphs) == 1
    # the eager fused path is still there (explicit noise, or graph = False) and agrees on the interface
    rn.graph = False
    model, mask, score, iters = rn(m[0], lg[0], K1[0], K2[0], None)
    assert model.shape == (3, 3) and mask.shape == (2000,) and isinstance(iters, int)


# ------------------------------------------------------------------------------------- MatchLoss: value + gradient in one pass
@pytest.mark.parametrize("N", [2000, 1000, 513])
def test_match_loss_value_and_gradient_in_one_pass(dev, N):
    """loss.py:107-153: the fused kernel (sums, per-pair means, their mean and the unscaled gradient of every model from ONE walk over
    the (model x point) grid, backward = one elementwise launch) against the two-pass form of rounds 3-4 and against torch autograd
    through the f64 restatement of batch_episym (cv_utils.py:680-695) -- incl. slots that are not kept and an empty mask row"""
    from differentiable_ransac_amd import ops, synth
    P, M = 3, 300
    d = synth.batch_two_view(P, N, seed0=5)
    gen = torch.Generator().manual_seed(N)
    models = torch.randn(P, M, 3, 3, generator=gen).to(dev) * 0.5 + d["gt_E"][:, None].to(dev)
    keep = (torch.rand(P, M, generator=gen) < 0.7).to(dev)
    mask = d["inliers"].to(dev).clone()
    mask[2] = False                                   # a pair without ground-truth inliers: loss 0, gradient 0
    m = d["matches"].to(dev)
    out = {}
    for fused in (True, False):
        ops.FUSED_MATCH_LOSS = fused
        try:
            md = models.clone().requires_grad_(True)
            loss = ops.match_loss_mean(m, mask, md, keep)
            (loss * 3.0).backward()
            out[fused] = (loss.detach(), md.grad.clone())
        finally:
            ops.FUSED_MATCH_LOSS = True
    (la, ga), (lb, gb) = out[True], out[False]
    assert abs(float(la) - float(lb)) <= 2e-6 * abs(float(lb))
    assert float((ga - gb).abs().max()) <= 2e-5 * max(1e-6, float(gb.abs().max()))
    assert float(ga[~keep].abs().max()) == 0.0 and float(ga[2].abs().max()) == 0.0
    # f64 autograd of the formula
    md = models.double().cpu().requires_grad_(True)
    x1 = torch.cat((m[..., :2], torch.ones_like(m[..., :1])), -1).double().cpu()
    x2 = torch.cat((m[..., 2:], torch.ones_like(m[..., :1])), -1).double().cpu()
    Fx1 = torch.einsum("pmij,pnj->pmni", md, x1)
    Ftx2 = torch.einsum("pmji,pnj->pmni", md, x2)
    r = (x2[:, None] * Fx1).sum(-1)
    ys = r ** 2 * (1 / (Fx1[..., 0] ** 2 + Fx1[..., 1] ** 2 + 1e-15) + 1 / (Ftx2[..., 0] ** 2 + Ftx2[..., 1] ** 2 + 1e-15))
    w = mask.cpu().double()[:, None, :] * keep.cpu().double()[:, :, None]
    den = (mask.cpu().double().sum(1) * keep.cpu().double().sum(1)).clamp(min=1.0)
    ref = ((ys.clamp(max=1.0) * w).sum((1, 2)) / den).mean()
    (ref * 3.0).backward()
    assert abs(float(la) - float(ref)) <= 1e-5 * abs(float(ref))
    assert float((ga.double().cpu() - md.grad).abs().max()) <= 2e-4 * float(md.grad.abs().max())


# ------------------------------------------------------------------------------------- f64 train mode without the f32 bottleneck
def test_f64_fivepoint_backward_in_double_precision(dev):
    """dr_solve_nister5_bwd_f64: samples, models and gradients f64 in memory.  Against central differences of the f64 forward itself
    (the solution that moves continuously with the sample), to 1e-6 of the gradient's scale -- the f32-I/O kernel of rounds 1-4
    could not be checked below one f32 rounding of its inputs (2e-3 in test_gpu_round4.py)"""
    from differentiable_ransac_amd import ops, synth
    pair = synth.two_view_pair(41, 400, inlier_ratio=1.0, noise=0.0, dtype=torch.float64)
    smp0 = pair["matches"][:40].reshape(8, 5, 4).to(dev)
    gen = torch.Generator().manual_seed(4)
    wgt = torch.randn(3, 3, generator=gen, dtype=torch.float64).to(dev)
    gt = pair["gt_E"].to(dev)

    def picked(smp):          # the solution closest to the ground truth (sign-fixed): a smooth function of the sample
        E, valid = ops.solve_essential(smp, None, "nister")
        d = torch.minimum(((E - gt) ** 2).sum((-1, -2)), ((E + gt) ** 2).sum((-1, -2)))
        d = torch.where(valid, d, torch.full_like(d, 1e9))
        j = d.argmin(-1)
        Ej = E[torch.arange(E.shape[0], device=dev), j]
        sgn = torch.sign((Ej * gt).sum((-1, -2)))
        return Ej * sgn[:, None, None], d.min(-1).values
    smp = smp0.clone().requires_grad_(True)
    Ej, dist = picked(smp)
    assert float(dist.max()) < 1e-12                       # noise-free samples: the ground truth is among the solutions
    (Ej * wgt).sum().backward()
    g = smp.grad
    assert g.dtype == torch.float64 and bool(torch.isfinite(g).all())
    h = 1e-6
    scale = g.abs().amax((1, 2))
    well = [b for b in range(8) if float(scale[b]) < 1e3]      # (an ill-conditioned sample's solution is not smooth over 2 h)
    assert len(well) >= 5
    checked = 0
    for i, b in enumerate(well[:5]):
        k, c = (2 * i) % 5, (3 * i) % 4
        sp, sm = smp0.clone(), smp0.clone()
        sp[b, k, c] += h
        sm[b, k, c] -= h
        fd = float(((picked(sp)[0] - picked(sm)[0]) * wgt).sum()) / (2 * h)
        assert abs(fd - float(g[b, k, c])) <= 1e-6 * float(scale[b]), (b, k, c, fd, float(g[b, k, c]))
        checked += 1
    assert checked == 5
    # and the f32-I/O kernel of rounds 1-4 on the same samples agrees to ITS rounding
    s32 = smp0.float().clone().requires_grad_(True)
    E32, v32 = ops.solve_essential(s32, None, "nister")
    d32 = torch.minimum(((E32 - gt.float()) ** 2).sum((-1, -2)), ((E32 + gt.float()) ** 2).sum((-1, -2)))
    j32 = torch.where(v32, d32, torch.full_like(d32, 1e9)).argmin(-1)
    Ej32 = E32[torch.arange(8, device=dev), j32]
    ((Ej32 * torch.sign((Ej32 * gt.float()).sum((-1, -2)))[:, None, None]) * wgt.float()).sum().backward()
    rel = (g - s32.grad.double()).abs().amax((1, 2)) / scale
    assert float(rel[well].max()) < 1e-4, rel.tolist()


def test_f64_train_step_with_match_loss_through_the_batched_driver(dev):
    """`-pr 2 -tr 1 -w2 1` (model_cl.py:164-169, Q17): the batched driver in double precision end to end -- sampler, gather, Nister,
    best-of-ten, MatchLoss (f64: torch ops on the device), backward to the logits -- against the f32 training path on the same
    seed: same index sets, models equal to f32 rounding, loss and gradient close"""
    from differentiable_ransac_amd import synth
    from differentiable_ransac_amd.loss import MatchLoss
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    d = synth.batch_two_view(2, 1000, seed0=13)
    out = {}
    for dt in (torch.float64, torch.float32):
        m, K1, K2, gt = (d[k].to(dev).to(dt) for k in ("matches", "K1", "K2", "gt_E"))
        lg = d["logits"].to(dev).to(dt).requires_grad_(True)
        drv = BatchedRANSAC("nister", ransac_batch_size=256, train=True, threshold=0.75, max_iterations=100, seed=5)
        noise = [synth.gumbel_noise((2, 256, 1000), seed=77).to(dev).to(dt)]
        chosen, keep = drv(m, lg, K1, K2, gt_model=gt, gumbels=noise)
        loss = MatchLoss()(chosen, m, d["inliers"].to(dev), keep)
        loss.backward()
        out[dt] = (chosen.detach(), keep, float(loss), lg.grad.clone())
    (c64, k64, l64, g64), (c32, k32, l32, g32) = out[torch.float64], out[torch.float32]
    assert c64.dtype == torch.float64 and g64.dtype == torch.float64 and bool(torch.isfinite(g64).all())
    both = k64 & k32
    assert float(both.float().mean()) > 0.9
    assert float((c64[both] - c32[both].double()).abs().amax((-1, -2)).quantile(0.99)) < 1e-4
    assert abs(l64 - l32) <= 1e-3 * abs(l64)
    assert float((g64 - g32.double()).abs().max()) <= 0.05 * float(g64.abs().max())


# ------------------------------------------------------------------------------------- round-4 advice: screened sampler, large logits
@pytest.mark.parametrize("bias", [0.0, 3.0e3, 1.0e5, -2.0e4])
def test_screened_sampler_with_large_logit_offsets_equals_the_unscreened_kernel(dev, bias):
    """the screening margin of dr_gumbel_topk_index_f32 covers the f32 rounding of logit + G only while the scores stay below ~1.6e4:
    pairs whose threshold lies beyond 4096 are not screened -- either way the index sets are those of the unscreened kernel"""
    from differentiable_ransac_amd import ops
    P, B, N, k = 2, 512, 16384, 3
    logits = torch.randn(P, N, generator=torch.Generator().manual_seed(3)) * 2.0 + bias
    logits[1] += 0.37 * bias
    logits = logits.to(dev)
    a = ops.gumbel_topk(logits, B, k, 1.0, None, 9, soft=False, screen=True)["idx"]
    b = ops.gumbel_topk(logits, B, k, 1.0, None, 9, soft=False, screen=False)["idx"]
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------- K1, short rows: the register kernel
@pytest.mark.parametrize("N,B,k", [(2048, 256, 3), (1000, 64, 5), (500, 1024, 1)])
def test_register_sampler_equals_the_general_kernel_and_the_oracle(dev, N, B, k):
    """dr_gumbel_topk_gather_f32 on rows the register kernel serves (two-logarithm form): the index sets are those of the general
    kernel for the same seed, and those of the CPU oracle on the noise the general kernel reports.  (What remains of the test of
    the screened short-row sampler, which was measured slower and removed: docs/LOG.md.)"""
    from differentiable_ransac_amd import ops, synth
    P = 3
    d = synth.batch_two_view(P, N, seed0=21)
    m = d["matches"].to(dev)
    lg = d["logits"].to(dev)
    r = ops.gumbel_topk(lg, B, k, 1.0, None, 5, want_noise=True)
    ia, _ = ops.gumbel_topk_gather(m, lg, B, k, 1.0, 5, race=False)
    assert torch.equal(ia, r["idx"])
    io, _, _ = O.gumbel_topk(d["logits"][0], r["gumbel"][0].cpu(), 1.0, k)
    assert torch.equal(ia[0].cpu().long(), io)


@pytest.mark.parametrize("N,B,k,dseed", [(2000, 256, 5, False), (2000, 100, 5, True), (512, 64, 8, False), (2500, 64, 5, False),
                                         (1001, 32, 3, False)])
def test_train_sampler_and_gather_in_one_launch_forward_and_backward(dev, N, B, k, dseed):
    """dr_gumbel_topk_gather_soft_f32 / dr_gumbel_topk_gather_bwd_f32 (round 5: K1 + K2 of train mode in one launch each way)
    against the two-launch forward / backward of rounds 1-4: identical index sets, weights and samples; gradients to the logits
    equal to accumulation rounding -- with and without a gradient on the y_sel output, register kernel (N <= 2048, N % 4 == 0) and
    the shapes that fall back to sampler + gather launches."""
    from differentiable_ransac_amd import ops
    P = 3
    g = torch.Generator().manual_seed(N + B)
    matches = torch.randn(P, N, 4, generator=g).to(dev)
    logits0 = (torch.randn(P, N, generator=g) * 2).to(dev)
    w_s = torch.randn(P, B, k, 4, generator=g).to(dev)
    w_y = torch.randn(P, B, k, generator=g).to(dev)

    def run(fused, use_y):
        ops.FUSED_SAMPLE_GATHER = fused
        try:
            if dseed:
                ds = ops.DeviceSeed(1234, dev)
                seed = ds.next()
            else:
                seed = 1234
            lg = logits0.clone().requires_grad_(True)
            samples, y_sel, idx = ops.SampleGather.apply(matches, lg, B, k, 1.0, None, seed)
            loss = (samples * w_s).sum() + ((y_sel * w_y).sum() if use_y else 0.0)
            loss.backward()
            return samples.detach(), y_sel.detach(), idx, lg.grad
        finally:
            ops.FUSED_SAMPLE_GATHER = True

    for use_y in (False, True):
        s1, y1, i1, g1 = run(True, use_y)
        s0, y0, i0, g0 = run(False, use_y)
        assert torch.equal(i1, i0) and torch.equal(y1, y0) and torch.equal(s1, s0)
        assert torch.isfinite(g1).all()
        scale = g0.abs().max()
        assert (g1 - g0).abs().max() <= 2e-5 * scale, ((g1 - g0).abs().max(), scale)


def test_batched_essential_refit_with_the_wave_cooperative_final_stage(dev):
    """K7 at >= 16 pairs per launch: the refit kernel's stages after the elimination are the minimal solver's wave-cooperative ones
    (round 5; launches of fewer pairs keep the one-sample form tested in test_gpu_solvers.py).  Against the reference's own
    non-minimal golden vector (replicated), the f64 oracle on synthetic pairs, and the small-launch form on the same pairs."""
    from differentiable_ransac_amd import ops, synth
    from tests.conftest import load_golden
    g = load_golden("nister_nonminimal")
    for dt, tol in ((torch.float64, 1e-6), (torch.float32, TOL)):
        m = g["matches"].to(dt).unsqueeze(0).repeat(16, 1, 1).to(dev)
        E, valid = ops.refit_essential(m)
        for p in (0, 7, 15):
            d = O.match_solution_sets(E[p].cpu().double(), valid[p].cpu(), g["models"], torch.ones(10, dtype=torch.bool))
            assert d.numel() >= 1 and d.max() < tol
    P, N = 20, 2000
    data = synth.batch_two_view(P, N, seed0=900)
    E, valid = ops.refit_essential(data["matches"].to(dev))
    for p in range(P):
        Eo, ok, real = O.nister_5pt(data["matches"][p].double().unsqueeze(0))
        fw = O.match_solution_sets(E[p].cpu().double(), valid[p].cpu(), Eo[0], real[0])
        bw = O.match_solution_sets(Eo[0], real[0], E[p].cpu().double(), valid[p].cpu())
        assert fw.numel() == bw.numel() and (fw.numel() == 0 or max(fw.max(), bw.max()) < TOL), p
    # the same pairs through launches of five (the light form): same solution sets
    for p0 in (0, 5):
        Es, vs = ops.refit_essential(data["matches"][p0:p0 + 5].to(dev))
        for q in range(5):
            assert int(vs[q].sum()) == int(valid[p0 + q].sum())
            fw = O.match_solution_sets(Es[q].cpu().double(), vs[q].cpu(), E[p0 + q].cpu().double(), valid[p0 + q].cpu())
            assert fw.numel() == 0 or fw.max() < TOL
    # masked, ragged over the pairs
    mask = torch.rand(P, N, generator=torch.Generator().manual_seed(2)) > 0.5
    Em, vm = ops.refit_essential(data["matches"].to(dev), mask.to(dev))
    for p in (0, 11, 19):
        Esol, vsol = ops.solve_nister5(data["matches"][p][mask[p]].unsqueeze(0).to(dev))
        fw = O.match_solution_sets(Em[p].cpu().double(), vm[p].cpu(), Esol[0].cpu().double(), vsol[0].cpu())
        assert int(vm[p].sum()) == int(vsol[0].sum()) and (fw.numel() == 0 or fw.max() < TOL)


def test_graph_replay_of_a_chip_filling_call_with_the_final_refit(dev):
    """64 pairs x 1024 hypotheses with K7: the refit is issued first on its side stream, one tiny launch in front of the sampler lets
    its blocks onto the chip before the sampler's 16 384 workgroups (round 5), the >= 16-pair form of the refit kernel runs -- the
    whole call captured in a HIP graph and replayed equals the eager driver with the same seeds, call after call"""
    from differentiable_ransac_amd import synth
    from differentiable_ransac_amd.graphs import GraphedStep
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    P, N, B = 64, 2000, 1024
    d = synth.batch_two_view(P, N, seed0=60)
    m, lg, K1, K2 = (d[k].to(dev) for k in ("matches", "logits", "K1", "K2"))
    kw = dict(ransac_batch_size=B, train=False, threshold=0.75, max_iterations=B, seed=5, keep_masks=False, refit=True)
    eager = BatchedRANSAC("nister", **kw)
    graphed = BatchedRANSAC("nister", **kw).device_seeds(dev)
    warm = 3
    for _ in range(warm):
        eager(m, lg, K1, K2)
    step = GraphedStep(lambda: graphed(m, lg, K1, K2), warmup=warm)
    for r in range(3):
        want = eager(m, lg, K1, K2)
        got = step()
        for key in ("model", "mask", "score", "inliers"):
            assert torch.equal(want[key], got[key]), (key, r)
    assert eager._gap is not None and graphed._gap is not None      # the dispatch gap was taken (P x B >= 65 536)
