"""The adaptive stop's exponent (ransac.py:204-215): the reference raises the inlier ratio to its estimator's `sample_size`,
7 for the 8-point F estimator, not to the sampler's 8 points per sample.

The reference fixtures replay a recorded noise list, and a loop also stops when that list runs out; on the F fixtures the
list ends exactly where the reference's bound stopped it, so a wrong exponent (a larger bound) goes unnoticed.  Here every
list is lengthened by batches from a fixed generator: the loop must still stop at the reference's recorded iteration
count, i.e. on its bound and not on an empty list.  CPU only."""
import pytest
import torch

from differentiable_ransac_amd import synth
from oracle import cpu_ref as O
from tests import lo_ref
from tests.conftest import load_golden

torch.set_num_threads(1)

EXTRA = 48          # batches appended to every recorded list (the bound with exponent 8 lies ~40 batches further out)


def lengthened(g, seed=2024):
    """the fixture's recorded noise batches followed by EXTRA batches of the same shape from a fixed generator"""
    rec = list(g["gumbels"])
    B, N = rec[0].shape
    more = synth.gumbel_noise((EXTRA, B, N), seed=seed, dtype=rec[0].dtype)
    return rec + list(more)


def _args(g):
    return g["matches"], g["logits"], lengthened(g), g["K1"], g["K2"]


def test_the_f_bound_differs_between_the_exponents():
    """66 of 128 inliers: bound 710 with exponent 7 (the reference stops at 720 = 45 x 16), 1382 with exponent 8"""
    assert 704 < O.adaptive_iteration_number(66, 128, 7) <= 720
    assert O.adaptive_iteration_number(66, 128, 8) > 1300


@pytest.mark.parametrize("name,weighted", [("ransac_test_f8", False), ("ransac_test_f8_weighted", True)])
def test_oracle_stops_on_the_reference_bound(name, weighted):
    g = load_golden(name)
    model, mask, score, iters = O.ransac_test(*_args(g), "f8", weighted=weighted)
    assert iters == g["iterations"]
    assert torch.equal(mask, g["best_mask"])
    assert abs(score - g["best_score"]) <= 1e-3 * max(1.0, abs(g["best_score"]))


def test_oracle_stops_on_the_reference_bound_lo_fixture():
    g = load_golden("ransac_test_lo_f8")
    model, mask, score, iters = O.ransac_test(*_args(g), "f8")
    assert iters == g["iterations_lo0"]
    assert torch.equal(mask, g["mask_lo0"])


@pytest.mark.parametrize("lo", [0, 1, 2])
def test_lo_restatement_stops_on_the_reference_bound(lo):
    """tests/lo_ref.py with its default exponent (the estimator's sample_size) on the reference's lo runs"""
    g = load_golden("ransac_test_lo_f8")
    model, mask, score, iters, _ = lo_ref.ransac_test_lo(*_args(g), "f8", lo, int(g["lo_iters"]))
    assert iters == g[f"iterations_lo{lo}"]
    assert torch.equal(mask, g[f"mask_lo{lo}"])
    assert abs(score - g[f"score_lo{lo}"]) <= 1e-3 * max(1.0, abs(g[f"score_lo{lo}"]))


def test_num_samples_does_not_change_the_exponent():
    """the five-point estimator on 8-point samples (`-sam 3`) stops with exponent 5 by default"""
    g = load_golden("ransac_test_lo_nister")
    a = lo_ref.ransac_test_lo(*_args(g), "nister", 0, num_samples=8, refit=False)
    b = lo_ref.ransac_test_lo(*_args(g), "nister", 0, num_samples=8, refit=False, sample_size=5)
    assert a[3] == b[3] and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ the drivers (GPU)
def _dropin(name, dev, fused, weighted=0):
    from differentiable_ransac_amd.estimators import EssentialMatrixEstimatorNister, FundamentalMatrixEstimatorNew
    from differentiable_ransac_amd.ransac import RANSAC
    from differentiable_ransac_amd.samplers import GumbelSoftmaxSampler
    from differentiable_ransac_amd.scorings import MSACScore
    fmat = name == "f8"
    est = FundamentalMatrixEstimatorNew(dev) if fmat else EssentialMatrixEstimatorNister(dev)
    r = RANSAC(est, GumbelSoftmaxSampler(16, 8 if fmat else 5, device=dev), MSACScore(dev), fmat=fmat, train=False,
               ransac_batch_size=16, sampler_id=3 if fmat else 2, weighted=weighted, threshold=0.75, max_iterations=5000)
    r.fused = fused
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("name,weighted", [("ransac_test_f8", 0), ("ransac_test_f8_weighted", 1)])
def test_f8_drivers_stop_on_the_reference_bound(dev, name, weighted):
    """the fused drop-in, the plugin drop-in and BatchedRANSAC("f8") on the lengthened noise stop where the f64 oracle stops on
    the same noise -- on its bound, well before the list ends -- with the oracle's result.  Unweighted, that is the reference's
    iteration count.  Weighted, the reference's f32 run took another best model (its weighted solves are ill-conditioned in
    f32, see test_gpu_round3.py; the f32 CPU oracle reproduces its 944 in test_oracle_stops_on_the_reference_bound): the f64
    chain the drivers follow keeps 63 inliers, bound 985.2, and stops at 992 (exponent 8, bound 2008, runs to the list's end)."""
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    g = load_golden(name)
    noise = lengthened(g)
    args = (g["matches"].to(dev), g["logits"].to(dev), g["K1"].to(dev), g["K2"].to(dev))
    dt = torch.float64
    mo, masko, so, ito = O.ransac_test(g["matches"].to(dt), g["logits"].to(dt), [x.to(dt) for x in noise], g["K1"].to(dt),
                                       g["K2"].to(dt), "f8", weighted=bool(weighted))
    assert ito == (992 if weighted else g["iterations"])
    runs = {}
    for fused in (True, False):
        model, mask, score, iters = _dropin("f8", dev, fused, weighted)(*args, None, gumbels=[x.to(dev) for x in noise])
        runs["fused" if fused else "plugin"] = (model, mask, score, int(iters))
    out = BatchedRANSAC("f8", ransac_batch_size=16, threshold=0.75, max_iterations=5000, weighted=weighted)(
        *(a[None] for a in args), gumbels=[x[None].to(dev) for x in noise])
    runs["batched"] = (out["model"][0], out["mask"][0], out["score"][0], int(out["iterations"][0]))
    for key, (model, mask, score, iters) in runs.items():
        assert iters == ito, (key, iters)
        assert int((mask.cpu() != masko).sum()) <= 1, key
        assert abs(float(score) - so) <= 1e-3 * max(1.0, so), (key, float(score), so)
        assert (O.canonical(model.cpu().double()) - O.canonical(mo)).abs().max() < 1e-4, key


@pytest.mark.gpu
@pytest.mark.parametrize("lo", [1, 2])
def test_f8_lo_drivers_stop_on_the_reference_bound(dev, lo):
    """the lo fixture, lengthened: fused drop-in, plugin drop-in and BatchedRANSAC stop where the reference's lo run stopped"""
    from tests.test_gpu_local_opt import _dropin as dropin_lo
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    g = load_golden("ransac_test_lo_f8")
    noise = [x.to(dev) for x in lengthened(g)]
    args = (g["matches"].to(dev), g["logits"].to(dev), g["K1"].to(dev), g["K2"].to(dev))
    for fused in (True, False):
        iters = dropin_lo("f8", lo, dev, fused)(*args, None, gumbels=noise)[3]
        assert int(iters) == g[f"iterations_lo{lo}"], (fused, int(iters))
    out = BatchedRANSAC("f8", ransac_batch_size=16, threshold=0.75, max_iterations=5000, lo=lo, lo_iters=8)(
        *(a[None] for a in args), gumbels=[x[None] for x in noise])
    assert int(out["iterations"][0]) == g[f"iterations_lo{lo}"]


@pytest.mark.gpu
def test_nister_on_8_point_samples_stops_with_exponent_5(dev):
    """BatchedRANSAC("nister", num_samples=8) (`-sam 3`) against lo_ref.ransac_test_lo(lo=0, num_samples=8), whose stop takes
    the five-point estimator's sample_size: 640 iterations here, while exponent 8 runs to the end of the list (1920)"""
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    N, B = 500, 32
    d = synth.two_view_pair(77, N, inlier_ratio=0.55)
    noise = list(synth.gumbel_noise((60, B, N), seed=78))
    dt = torch.float64
    mo, masko, so, ito, _ = lo_ref.ransac_test_lo(d["matches"].to(dt), d["logits"].to(dt), [x.to(dt) for x in noise],
                                                  d["K1"].to(dt), d["K2"].to(dt), "nister", 0, num_samples=8, refit=False)
    assert ito < 60 * B                                # stopped on its bound, well before the list's end
    drv = BatchedRANSAC("nister", ransac_batch_size=B, threshold=0.75, max_iterations=5000, num_samples=8, refit=False)
    out = drv(d["matches"][None].to(dev), d["logits"][None].to(dev), d["K1"][None].to(dev), d["K2"][None].to(dev),
              gumbels=[x[None].to(dev) for x in noise])
    assert int(out["iterations"][0]) == ito
    assert int((out["mask"][0].cpu() != masko).sum()) <= 1
    assert abs(float(out["score"][0]) - so) <= 1e-3 * max(1.0, so), (float(out["score"][0]), so)
