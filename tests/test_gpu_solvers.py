"""K3 / K4r / K5 parity on the GPU: HIP solvers vs the f64 CPU oracle and the reference's golden vectors.

E/F/T tolerance (BASELINE.json north_star): 1e-4 on the recovered models.  Five-point solution SETS are
compared after canonicalisation (unit Frobenius norm, sign), because the null-space basis, root order and
sign are LAPACK artefacts in the reference (SURVEY hard part 2)."""
import pytest
import torch

from oracle import cpu_ref as O
from tests import refit_ref
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _set_dist(E, valid, Eo, valid_o):
    """for every sample: (distances of HIP solutions to nearest oracle solution, and the reverse)"""
    fw, bw = [], []
    for b in range(E.shape[0]):
        fw.append(O.match_solution_sets(E[b], valid[b], Eo[b], valid_o[b]))
        bw.append(O.match_solution_sets(Eo[b], valid_o[b], E[b], valid[b]))
    return torch.cat(fw), torch.cat(bw)


def _kat_essential(E, valid, smp, tol=1e-6):
    x1 = torch.cat((smp[..., 0:2], torch.ones_like(smp[..., :1])), -1)
    x2 = torch.cat((smp[..., 2:4], torch.ones_like(smp[..., :1])), -1)
    r = torch.einsum("bki,bsij,bkj->bsk", x2, E, x1).abs().amax(-1)
    assert r[valid].max() < tol
    assert torch.linalg.det(E)[valid].abs().max() < tol
    EEt = E @ E.transpose(-1, -2)
    tr = EEt.diagonal(dim1=-2, dim2=-1).sum(-1)
    assert (2 * EEt @ E - tr[..., None, None] * E)[valid].abs().max() < tol
    assert (torch.linalg.norm(E[valid], dim=(-1, -2)) - 1).abs().max() < tol
    eye = torch.eye(3, dtype=E.dtype)
    assert (E[~valid] == eye).all()


@pytest.mark.parametrize("path", [0, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("solver", ["nister", "stewenius"])
def test_fivepoint_golden(dev, solver, dtype, path):
    """path = 2: the reference-held vector through the TWO-PHASE kernels -- the ones every launch of >= 65 536 samples (the bench,
    configs 3 and 5) takes; 32 samples would take the lane-pair kernel on their own (round-5 review, missing item 5)"""
    from differentiable_ransac_amd import ops
    if path and dtype != torch.float32:
        pytest.skip("explicit kernel paths exist for f32 I/O only")
    g = load_golden("fivepoint")
    smp = g["samples"].to(dtype)
    fn = ops.solve_nister5 if solver == "nister" else ops.solve_stewenius5
    E, valid = fn(smp.to(dev), path=path) if path else fn(smp.to(dev))
    E, valid = E.cpu().double(), valid.cpu()
    assert E.shape == (32, 10, 3, 3) and valid.shape == (32, 10)
    _kat_essential(E, valid, smp.double())
    # reference (f64 run) real solutions: every one is reproduced, and nothing else is invented
    Eo, ok, real = O.nister_5pt(g["samples"])
    assert ok.all()
    fw, bw = _set_dist(E, valid, Eo, real)
    # (the f64 reference itself is only good to ~6e-7 on its worst solution here, see tests/test_oracle_golden.py)
    tol = TOL if dtype == torch.float32 else 5e-6
    assert fw.numel() >= 120 and bw.numel() >= 120
    assert fw.max() < tol and bw.max() < tol, (fw.max(), bw.max())
    if dtype == torch.float64:
        assert fw.median() < 1e-11
    # and directly against the stored reference output (which also contains Re(complex root) junk slots)
    ref = g["nister_f64"].reshape(32, 10, 3, 3)
    allv = torch.ones(10, dtype=torch.bool)
    d = torch.cat([O.match_solution_sets(E[b], valid[b], ref[b], allv) for b in range(32)])
    assert d.max() < tol


def test_nister_mixed_precision_entry(dev):
    """dr_solve_nister5_f32 with models_f64 (train mode): f64 models equal to the f64 entry on the widened samples up to the f64
    polish tolerance (the two instantiations are compiled separately, so not bit-for-bit), f32 models the exact
    rounding of the f64 ones, same valid flags."""
    from differentiable_ransac_amd import ops
    g = load_golden("fivepoint")
    smp = g["samples"].float().to(dev)
    m32, m64, valid = ops.solve_nister5_hp(smp)
    r64, rvalid = ops.solve_nister5(smp.double())
    assert m64.dtype == torch.float64 and m32.dtype == torch.float32
    assert torch.equal(valid, rvalid)
    assert (m64 - r64).abs().max() < 1e-12
    assert torch.equal(m32, m64.float())
    with pytest.raises(Exception):
        ops.solve_nister5_hp(smp.double())


@pytest.mark.parametrize("path", [0, 2])
def test_nister_weighted_and_nonminimal(dev, path):
    from differentiable_ransac_amd import ops
    g = load_golden("fivepoint")
    E, valid = ops.solve_nister5(g["samples"].float().to(dev), g["weights"].float().to(dev), path=path)
    Eo, ok, real = O.nister_5pt(g["samples"], g["weights"])
    fw, bw = _set_dist(E.cpu().double(), valid.cpu(), Eo, real)
    assert fw.max() < TOL and bw.max() < TOL
    g = load_golden("nister_nonminimal")
    E, valid = ops.solve_nister5(g["matches"].unsqueeze(0).to(dev))   # f64, all 256 points as one sample
    d = O.match_solution_sets(E[0].cpu(), valid[0].cpu(), g["models"], torch.ones(10, dtype=torch.bool))
    assert d.numel() >= 1 and d.max() < 1e-6


def test_fivepoint_config_sizes_vs_oracle(dev):
    """C2-sized batch (1024 Gumbel-sampled minimal samples of a 2000-point pair), f32 I/O"""
    from differentiable_ransac_amd import ops, synth
    pair = synth.two_view_pair(0, 2000)
    noise = synth.gumbel_noise((1, 1024, 2000), seed=1)
    r = ops.gumbel_topk(pair["logits"][None].to(dev), 1024, 5, 1.0, noise.to(dev))
    smp = ops.gather(pair["matches"][None].to(dev), r["idx"], r["y_sel"])[0]
    Eo, ok, real = O.nister_5pt(smp.cpu().double())
    for fn in (ops.solve_nister5, ops.solve_stewenius5):
        E, valid = fn(smp)
        E, valid = E.cpu().double(), valid.cpu()
        _kat_essential(E, valid, smp.cpu().double(), tol=2e-5)   # f32-rounded E
        fw, bw = _set_dist(E[ok], valid[ok], Eo[ok], real[ok])
        # f32 output rounding only: the solver itself runs in f64
        assert fw.quantile(0.995) < TOL and bw.quantile(0.995) < TOL, (fw.max(), bw.max())
        # round 5 (Sturm fallback, converged roots): measured 0 - 6.5e-4 over three seeds, valid counts equal to the oracle's
        assert (fw > TOL).float().mean() < 1e-3 and (bw > TOL).float().mean() < 1e-3
        assert abs(int(valid.sum()) - int(real[ok].sum())) <= 4


def test_fivepoint_noise_free_contains_ground_truth(dev):
    from differentiable_ransac_amd import ops, synth
    pair = synth.two_view_pair(77, 640, inlier_ratio=1.0, noise=0.0, dtype=torch.float64)
    smp = pair["matches"].reshape(128, 5, 4)
    one = torch.ones(1, dtype=torch.bool)
    for fn in (ops.solve_nister5, ops.solve_stewenius5):
        E, valid = fn(smp.to(dev))
        d = torch.stack([O.match_solution_sets(pair["gt_E"][None], one, E[b].cpu(), valid[b].cpu())[0] for b in range(128)])
        assert d.max() < 1e-6, d.max()


def test_fivepoint_degenerate_inputs_never_nan(dev):
    from differentiable_ransac_amd import ops
    smp = torch.zeros(70, 5, 4)
    smp[1] = 1.0
    smp[2, :, :] = torch.tensor([0.1, 0.2, 0.3, 0.4])          # five identical points
    smp[3] = float("nan")
    smp[4:] = torch.randn(66, 5, 4, generator=torch.Generator().manual_seed(0))
    smp[5, 1] = smp[5, 0]                                        # duplicate point (uniform sampler draws with replacement)
    for fn in (ops.solve_nister5, ops.solve_stewenius5):
        E, valid = fn(smp.to(dev))
        assert torch.isfinite(E).all()
        assert (E[~valid] == torch.eye(3, device=dev)).all()
        assert not valid[3].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_f8_golden(dev, dtype):
    from differentiable_ransac_amd import ops
    g = load_golden("f8")
    tol = TOL if dtype == torch.float32 else 1e-8
    for key, args in (("F", (g["samples"],)), ("F_w", (g["samples"], g["weights"])), ("F_nm", (g["samples_nm"],))):
        F, valid = ops.solve_f8(*[a.to(dtype).to(dev) for a in args])
        assert valid.all()
        # reference run in f64 on the SAME (dtype-rounded) inputs: pixel coordinates ~1e3 rounded to f32 move F by ~1e-4
        ref = g[f"{key}_f64"] if dtype == torch.float64 else O.fundamental_8pt(*[a.to(dtype).double() for a in args])
        if dtype == torch.float64:
            assert (O.canonical(O.fundamental_8pt(*args)) - O.canonical(ref)).abs().max() < 1e-9
        # un-normalised output: same scale as the reference (|F| fixed by the unit-norm null vector), sign free
        s = torch.sign((F.cpu().double() * ref).sum((-1, -2)))[:, None, None]
        rel = (F.cpu().double() * s - ref).abs().amax((-1, -2)) / ref.abs().amax((-1, -2))
        assert rel.max() < tol, rel.max()
    # recovers the GT fundamental matrix from noise-free inliers
    from differentiable_ransac_amd import synth
    pair = synth.two_view_pair(5, 64, inlier_ratio=1.0, noise=0.0, dtype=torch.float64, pixel=True)
    F, _ = ops.solve_f8(pair["matches"].reshape(8, 8, 4).to(dtype).to(dev))
    d = (O.canonical(F.cpu().double()) - O.canonical(pair["gt_F"])[None]).abs().amax((-1, -2))
    assert d.max() < (2e-2 if dtype == torch.float32 else 1e-6)


def test_f7_known_answers_and_oracle(dev):
    from differentiable_ransac_amd import ops
    g = load_golden("f8")
    smp = g["samples"][:, :7].contiguous()
    F, valid = ops.solve_f7(smp.to(dev))
    F, valid = F.cpu(), valid.cpu()
    assert F.shape == (32, 4, 3, 3) and not valid[:, 3].any() and (valid.sum(1) >= 1).all()
    assert torch.linalg.det(F)[valid].abs().max() < 1e-9
    x1 = torch.cat((smp[..., 0:2], torch.ones_like(smp[..., :1])), -1)
    x2 = torch.cat((smp[..., 2:4], torch.ones_like(smp[..., :1])), -1)
    r = torch.einsum("bki,bsij,bkj->bsk", x2, F, x1).abs().amax(-1)
    assert r[valid].max() < 1e-5
    assert (F[~valid] == torch.eye(3, dtype=F.dtype)).all()
    Fo, vo = O.fundamental_7pt(smp)
    fw, bw = _set_dist(F, valid, Fo, vo)
    assert fw.max() < 1e-6 and bw.max() < 1e-6
    F32, v32 = ops.solve_f7(smp.float().to(dev))
    fw, bw = _set_dist(F32.cpu().double(), v32.cpu(), Fo, vo)
    assert fw.max() < TOL and bw.max() < TOL


@pytest.mark.parametrize("flag", [True, False])
def test_rigid_golden(dev, flag):
    from differentiable_ransac_amd import ops
    from differentiable_ransac_amd import synth
    g = load_golden("rigid")
    model, R, t, scale, valid = ops.solve_rigid(g["samples"].to(dev), flag=flag)
    assert valid.all()
    mo, Ro, to, so, _ = O.rigid_svd(g["samples"].double(), flag=flag)
    assert (model.cpu().double() - mo).abs().max() < 1e-6                 # vs the f64 oracle
    err = (model.cpu() - g[f"model_{flag}"]).abs().amax((-1, -2))        # vs the reference's own f32 run
    if flag:
        # Q9: with flag=True R is the identity up to LAPACK noise; the reference's f32 SVD of the rank-2
        # cov^T cov leaves up to 6e-4 of that noise in 2 of the 32 samples (f64 oracle: 1e-12)
        assert (err < TOL).float().mean() >= 0.9 and err.max() < 2e-3
    else:
        assert err.max() < TOL
    assert (R.cpu() - g[f"R_{flag}"]).abs().max() < (2e-3 if flag else TOL)
    assert (scale.cpu() - g[f"scale_{flag}"]).abs().max() < 1e-5
    res, masks = ops.rigid_residual(g["matches"][None].to(dev), g[f"model_{flag}"][None].to(dev))
    assert ((res[0].cpu() - g[f"res_{flag}"]).abs() / g[f"res_{flag}"]).max() < 1e-5
    assert torch.equal(masks[0].cpu(), g[f"mask_{flag}"])
    if not flag:
        m, R, t, _, _ = ops.solve_rigid(g["matches"][128:].unsqueeze(0).to(dev), flag=False)
        assert (m.cpu() - g["model_nm"]).abs().max() < TOL
        assert (R[0] @ R[0].T - torch.eye(3, device=dev)).abs().max() < 1e-5
    # f64 + noise-free: exact alignment (R returned transposed w.r.t. the column-vector convention, Q9)
    rp = synth.rigid_pair(3, 300, inlier_ratio=1.0, noise=0.0, dtype=torch.float64)
    m, R, t, _, v = ops.solve_rigid(rp["matches"].reshape(100, 3, 6).to(dev), flag=False)
    assert (R.cpu() - rp["gt_T"][:3, :3].T[None]).abs().max() < 1e-8


def test_rigid_residual_config4_property(dev):
    """C4 shape (N = 50 000, M = 2048): point range split over blocks + atomics; checked against the oracle on a
    model subset and by the permutation-invariance of the sum."""
    from differentiable_ransac_amd import ops, synth
    rp = synth.rigid_pair(1, 50000)
    r = ops.gumbel_topk(rp["logits"][None].to(dev), 2048, 3, 1.0, None, seed=3)
    smp = ops.gather(rp["matches"][None].to(dev), r["idx"], r["y_sel"])
    model, _, _, _, valid = ops.solve_rigid(smp[0], flag=False)
    assert valid.all()
    res, masks = ops.rigid_residual(rp["matches"][None].to(dev), model[None])
    ro, _, mo = O.rigid_squared_residual(rp["matches"][:, :3].double(), rp["matches"][:, 3:].double(),
                                         model[:64, :3, :].transpose(-1, -2).cpu().double())
    assert ((res[0, :64].cpu().double() - ro).abs() / ro).max() < 1e-4
    assert (masks[0, :64].cpu() != mo).float().mean() < 1e-5
    perm = torch.randperm(50000, generator=torch.Generator().manual_seed(0))
    res2, _ = ops.rigid_residual(rp["matches"][perm][None].to(dev), model[None], want_masks=False)
    assert ((res2 - res).abs() / res).max() < 1e-4
    # flag=False recovers the motion from all-inlier samples: best residual is small
    assert float(res.min()) < 0.6 * float(res.median())


def test_select_closest(dev):
    from differentiable_ransac_amd import ops
    gen = torch.Generator().manual_seed(0)
    P, B, S = 3, 50, 10
    models = torch.randn(P, B, S, 3, 3, generator=gen)
    valid = torch.rand(P, B, S, generator=gen) > 0.4
    valid[0, 0] = False
    gt = torch.randn(P, 3, 3, generator=gen)
    chosen, which = ops.select_closest(models.to(dev), valid.to(dev), gt.to(dev))
    d = torch.linalg.norm(models - gt[:, None, None], dim=(-1, -2))
    d[~valid] = float("inf")
    ref = d.argmin(-1)
    any_valid = valid.any(-1)
    assert torch.equal(which.cpu()[any_valid].long(), ref[any_valid])
    assert (which.cpu()[~any_valid] == -1).all()
    pick = torch.gather(models, 2, ref[..., None, None, None].expand(P, B, 1, 3, 3))[:, :, 0]
    assert torch.equal(chosen.cpu()[any_valid], pick[any_valid])
    assert torch.equal(chosen.cpu()[0, 0], torch.eye(3))
    c2, w2 = ops.select_closest(models.to(dev), None, gt.to(dev))
    assert torch.equal(w2.cpu().long(), torch.linalg.norm(models - gt[:, None, None], dim=(-1, -2)).argmin(-1))


def test_batched_refit_kernels(dev):
    """K7: cooperative per-pair refit kernels vs the oracle (and the reference's non-minimal golden vector)."""
    from differentiable_ransac_amd import ops, synth
    g = load_golden("nister_nonminimal")
    for dt, tol in ((torch.float64, 1e-6), (torch.float32, TOL)):
        E, valid = ops.refit_essential(g["matches"].to(dt).unsqueeze(0).to(dev))
        d = O.match_solution_sets(E[0].cpu().double(), valid[0].cpu(), g["models"], torch.ones(10, dtype=torch.bool))
        assert d.numel() >= 1 and d.max() < tol
    P, N = 5, 2000
    data = synth.batch_two_view(P, N, seed0=700)
    E, valid = ops.refit_essential(data["matches"].to(dev))
    for p in range(P):
        Eo, ok, real = O.nister_5pt(data["matches"][p].double().unsqueeze(0))
        fw = O.match_solution_sets(E[p].cpu().double(), valid[p].cpu(), Eo[0], real[0])
        bw = O.match_solution_sets(Eo[0], real[0], E[p].cpu().double(), valid[p].cpu())
        assert fw.numel() == bw.numel() and (fw.numel() == 0 or max(fw.max(), bw.max()) < TOL)
    # masked variant == the per-sample kernel on the gathered points
    mask = torch.rand(P, N, generator=torch.Generator().manual_seed(1)) > 0.6
    Em, vm = ops.refit_essential(data["matches"].to(dev), mask.to(dev))
    for p in range(2):
        Es, vs = ops.solve_nister5(data["matches"][p][mask[p]].unsqueeze(0).to(dev))
        fw = O.match_solution_sets(Em[p].cpu().double(), vm[p].cpu(), Es[0].cpu().double(), vs[0].cpu())
        assert int(vm[p].sum()) == int(vs[0].sum()) and (fw.numel() == 0 or fw.max() < TOL)
    # fundamental: LSQ on the inliers of a mask, ragged over pairs
    dF = synth.batch_two_view(P, N, seed0=710, pixel=True)
    mask = dF["inliers"].clone()
    mask[3, 1500:] = False
    F, fv = ops.refit_fundamental(dF["matches"].to(dev), mask.to(dev))
    assert fv.all()
    for p in range(P):
        Fo = O.fundamental_8pt(dF["matches"][p][mask[p]].double().unsqueeze(0))[0]
        s = torch.sign((F[p].cpu().double() * Fo).sum())
        # the rule of tests/test_gpu_refit.py for this input (a wide eigen-gap, f32 in and out: the output's rounding dominates)
        cond = refit_ref.f_refit(dF["matches"][p].double(), mask[p])[2]
        assert ((F[p].cpu().double() * s - Fo).abs().max() / Fo.abs().max()) <= refit_ref.f_tolerance(cond, torch.float32)
        assert (O.canonical(F[p].cpu().double()) - O.canonical(dF["gt_F"][p].double())).abs().max() < 0.05
    few = torch.zeros(P, N, dtype=torch.bool)
    few[:, :5] = True
    F, fv = ops.refit_fundamental(dF["matches"].to(dev), few.to(dev))
    assert not fv.any() and (F.cpu() == torch.eye(3)).all()
