"""BatchedRANSAC(scoring="magsac") end to end on synthetic two-view scenes: P = 4, N = 512, B = 256, max_iterations = 1024."""
import pytest
import torch

from tests import magsac_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, N, B, MAXIT, THR = 4, 512, 256, 1024, 0.75


def _scene(solver="nister"):
    """normalised coordinates for the essential solver, pixels for the fundamental one (its threshold is not normalised)"""
    from differentiable_ransac_amd import synth
    d = synth.batch_two_view(P, N, seed0=40, pixel=solver == "f8")
    return {k: (v.to(DEV) if torch.is_tensor(v) and v.dtype.is_floating_point else v) for k, v in d.items()}


def _driver(solver, **kw):
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    kw.setdefault("seed", 3)
    return BatchedRANSAC(solver, ransac_batch_size=B, max_iterations=MAXIT, threshold=THR, scoring=kw.pop("scoring", "magsac"), **kw)


def _call(drv, d):
    out = drv(d["matches"], d["logits"], d["K1"], d["K2"])
    torch.cuda.synchronize()
    return out


def _thr(solver, d):
    """the normalised threshold dr_ransac_init forms (ransac.py:49-53); F: the threshold as given"""
    if solver == "f8":
        return [THR] * P
    K1, K2 = d["K1"].cpu().float(), d["K2"].cpu().float()
    f = (((K1[:, 0, 0] + K1[:, 1, 1]) + K1[:, 0, 0]) + K2[:, 1, 1]) / 4
    return ((1.0 / f) * torch.tensor(THR, dtype=torch.float32)).tolist()


def _check_result(out, d, solver):
    thr = _thr(solver, d)
    assert set(out) >= {"model", "mask", "score", "inliers", "iterations", "irls_fits"}
    assert torch.equal(out["inliers"].long(), out["mask"].sum(-1))
    for p in range(P):
        mt, model = d["matches"][p].cpu(), out["model"][p].cpu()
        ref, _ = G.magsac(mt.double(), model.double(), thr[p])
        tol = G.score_tolerance(mt, model, thr[p], torch.float32)
        assert abs(float(out["score"][p]) - ref) <= tol, (p, float(out["score"][p]), ref, tol)


@pytest.mark.parametrize("solver", ["nister", "f8"])
def test_driver(solver):
    d = _scene(solver)
    out = _call(_driver(solver), d)
    _check_result(out, d, solver)
    assert bool((out["irls_fits"] <= 10).all()) and int(out["inliers"].min()) > 0
    again = _call(_driver(solver), d)
    assert all(torch.equal(out[k], again[k]) for k in ("model", "mask", "score", "inliers", "iterations", "irls_fits")), "same seed, other bits"
    # no polish: the RANSAC winner is one of the call's hypotheses, and the polish only raises the score
    for kw in (dict(irls_iters=0), dict(refit=False), dict(irls_iters=0, refit=False)):
        plain = _call(_driver(solver, **kw), d)
        _check_result(plain, d, solver)
        assert int(plain["irls_fits"].sum()) == 0 and torch.equal(plain["mask"], out["mask"])
        assert bool((out["score"] >= plain["score"]).all())
    plain = _call(_driver(solver, irls_iters=0, refit=False), d)      # the run whose model must be one of the call's hypotheses
    drv = _driver(solver, irls_iters=0, refit=False)
    hyp = []
    for _ in range(MAXIT // B):
        models, valid, _ = drv.hypotheses(d["matches"], d["logits"])
        hyp.append(models.reshape(P, -1, 9))
    hyp = torch.cat(hyp, 1)
    for p in range(P):
        assert bool((hyp[p] == plain["model"][p].reshape(1, 9)).all(-1).any()), f"pair {p}: the model is none of the call's hypotheses"


@pytest.mark.parametrize("solver", ["nister", "f8"])
def test_prosac_and_device_termination(solver):
    d = _scene(solver)
    _check_result(_call(_driver(solver, sampling="prosac"), d), d, solver)
    host = _call(_driver(solver), d)
    drv = _driver(solver)
    drv.device_termination = True
    out = _call(drv, d)
    _check_result(out, d, solver)
    assert all(torch.equal(out[k], host[k]) for k in ("model", "mask", "score", "inliers", "iterations", "irls_fits"))


def test_graph_capture_and_replay():
    from differentiable_ransac_amd.graphs import GraphedStep
    d = _scene()
    drv = _driver("nister", seed=5).device_seeds(DEV)
    drv.device_termination = True
    step = GraphedStep(lambda: drv(d["matches"], d["logits"], d["K1"], d["K2"]), warmup=1)
    for _ in range(2):
        out = step()
        torch.cuda.synchronize()
        _check_result(out, d, "nister")


@pytest.mark.parametrize("solver", ["nister", "f8"])
def test_msac_is_the_default_path(solver):
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    d = _scene(solver)
    a = _call(BatchedRANSAC(solver, ransac_batch_size=B, max_iterations=MAXIT, threshold=THR, seed=3), d)
    b = _call(_driver(solver, scoring="msac"), d)
    assert set(a) == set(b) and "irls_fits" not in a
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
