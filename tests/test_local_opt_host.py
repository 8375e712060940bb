"""Host-side contract of local optimisation (lo): constructor validation of RANSAC / BatchedRANSAC, the batch-by-batch plan
it implies, and ops.local_optimize refusing CPU tensors before any device work.  No GPU needed."""
import pytest
import torch


def _plugins(fmat=False):
    from differentiable_ransac_amd.estimators import EssentialMatrixEstimatorNister, FundamentalMatrixEstimatorNew
    from differentiable_ransac_amd.samplers import GumbelSoftmaxSampler
    from differentiable_ransac_amd.scorings import MSACScore
    est = FundamentalMatrixEstimatorNew("cuda") if fmat else EssentialMatrixEstimatorNister("cuda")
    return est, GumbelSoftmaxSampler(64, 8 if fmat else 5, device="cuda"), MSACScore("cuda")


@pytest.mark.parametrize("lo", [1, 2])
def test_dropin_ransac_accepts_lo(lo):
    from differentiable_ransac_amd.ransac import RANSAC
    est, smp, sc = _plugins()
    r = RANSAC(est, smp, sc, sampler_id=2, lo=lo, lo_iters=8)
    assert r.lo == lo and r.lo_iters == 8
    assert r._fused_solver() == "nister"
    drv = r._make_fast("nister")
    assert drv.lo == lo and drv.lo_iters == 8


@pytest.mark.parametrize("lo", [3, 4, -1])
def test_dropin_ransac_refuses_other_lo(lo):
    from differentiable_ransac_amd.ransac import RANSAC
    est, smp, sc = _plugins()
    with pytest.raises(NotImplementedError):
        RANSAC(est, smp, sc, sampler_id=2, lo=lo)


def test_ransac3d_ignores_lo():
    from differentiable_ransac_amd.ransac import RANSAC3D
    RANSAC3D(None, None, None, lo=1)


def test_batched_ransac_lo_validation():
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    assert BatchedRANSAC("nister").lo == 0
    assert BatchedRANSAC("f8", lo=2, lo_iters=3).lo_iters == 3
    with pytest.raises(NotImplementedError):
        BatchedRANSAC("nister", lo=3)
    for bad in (4, -1, 5):
        with pytest.raises(ValueError):
            BatchedRANSAC("nister", lo=bad)
    with pytest.raises(ValueError):
        BatchedRANSAC("nister", lo=2, lo_iters=0)
    BatchedRANSAC("nister", lo=1, train=True)     # accepted, ignored in train mode


def test_batched_ransac_plan_with_lo():
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    # without lo: super-rounds (64 -> rounds of 1024 hypotheses); with lo: one batch per device round
    assert BatchedRANSAC("nister", ransac_batch_size=64, max_iterations=5000).plan() == [16, 16, 16, 16, 15]
    for lo in (1, 2):
        assert BatchedRANSAC("nister", ransac_batch_size=64, max_iterations=5000, lo=lo).plan() == [1] * 79
        assert BatchedRANSAC("f8", ransac_batch_size=1024, max_iterations=5000, lo=lo).plan() == [1] * 5
    # train mode ignores lo
    assert BatchedRANSAC("nister", ransac_batch_size=64, max_iterations=128, lo=1, train=True).plan() == [1, 1]


def test_local_optimize_refuses_cpu_tensors(monkeypatch):
    from differentiable_ransac_amd import _lib, ops
    calls = []
    monkeypatch.setattr(_lib, "call", lambda *a: calls.append(a))
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    P, N = 2, 64
    st = ops.RansacState(P, N, 5000, "cpu", torch.float32)
    matches = torch.rand(P, N, 4)
    thr = torch.full((P,), 0.01)
    seen = torch.full((P, 10), float("nan"))
    with pytest.raises(_lib.DransacError):
        ops.local_optimize(st, matches, thr, False, 1, 8, 5, 0.999, 1e-5, 5000, seen)
    assert calls == []
