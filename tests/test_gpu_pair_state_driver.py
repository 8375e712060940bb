"""BatchedRegistration and BatchedHomography in test mode against the same sequence of ops calls written out by hand -- draw, fit,
score, update, read-back, refit and its strict acceptance, with the driver's seeds -- bit for bit.  This pins the order of launches
and seed draws of the loop the two drivers share (ransac._PairStateDriver); tests/test_gpu_homography.py has the train-mode form."""
import numpy as np
import pytest
import torch

from differentiable_ransac_amd import ops
from differentiable_ransac_amd.ransac import BatchedHomography, BatchedRegistration
from tests import homography_ref as HR
from tests import registration_ref as RR

pytestmark = pytest.mark.gpu

DEV = "cuda"
P, N, B, MAXIT = 3, 300, 64, 192
FAMILIES = {
    "registration": dict(driver=BatchedRegistration, ref=RR, k=3, state=ops.RegistrationState, fit=ops.kabsch_gather,
                         score=ops.rigid_msac_score, update=ops.registration_update, refit=ops.refit_rigid),
    "homography": dict(driver=BatchedHomography, ref=HR, k=4, state=ops.HomographyState, fit=ops.homography4_gather,
                       score=ops.homography_score, update=ops.homography_update, refit=ops.refit_homography),
}


@pytest.mark.parametrize("sampling", ["gumbel", "prosac"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_test_mode_is_the_op_sequence_by_hand(family, dt, sampling):
    f = FAMILIES[family]
    sc = [f["ref"].scene(600 + p, N, 0.4) for p in range(P)]
    m = torch.as_tensor(np.stack([s["matches"] for s in sc]), device=DEV).to(dt)
    logits = torch.as_tensor(np.stack([np.where(s["inlier"], 0.5, -0.5) for s in sc]), device=DEV).to(dt)
    logits = logits + 1e-3 * torch.arange(N, device=DEV, dtype=dt)          # (no ties for the PROSAC ranking)
    thr, seed = f["ref"].THRESHOLD, 11
    kw = dict(ransac_batch_size=B, threshold=thr, max_iterations=MAXIT, seed=seed, sampling=sampling)
    out = f["driver"](**kw)(m, logits)

    twin = f["driver"](**kw)          # the same seeds, drawn by hand
    st = f["state"](P, N, MAXIT, m.device, dt)
    thr2 = ops.thr2_tensor(thr, P, m)
    if sampling == "prosac":
        order, growth = ops.prosac_rank(logits), ops.prosac_growth(N, f["k"], twin.prosac_draws, m.device)
    rounds = 0
    for r in range(twin.rounds):
        if sampling == "prosac":
            idx = ops.prosac_sample(order, growth, B, f["k"], twin._seeds.next(), r * B)
        else:
            idx = ops.gumbel_topk(logits, B, f["k"], 1.0, None, twin._seeds.next(), soft=False)["idx"]
        models, valid = f["fit"](m, idx)
        scores, _ = f["score"](m, models, thr, valid, want_inliers=False)
        f["update"](st, m, models, valid, scores, thr, B, 0.999, 1e-5)
        rounds += 1
        if r + 1 < twin.rounds and not bool((st.iters.double() < st.max_iters).any()):
            break
    cand, cvalid = f["refit"](m, st.best_mask)
    cscore = f["score"](m, cand.unsqueeze(1), thr, cvalid.unsqueeze(1), want_inliers=False)[0][:, 0]
    take = cscore > st.best_score
    by_hand = dict(model=torch.where(take[:, None, None], cand, st.best_model), score=torch.where(take, cscore, st.best_score),
                   mask=st.best_mask, inliers=st.best_inliers, iterations=st.iters)
    print(f"{family} {sampling}: rounds {rounds}, refit taken {take.tolist()}, inliers {st.best_inliers.tolist()}")
    assert rounds >= 2          # (the loop, its seeds and t0 = r B are exercised past the first round)
    assert sorted(out) == sorted(by_hand)
    for key, want in by_hand.items():
        assert out[key].dtype == want.dtype and torch.equal(out[key], want), key
    assert twin.calls == rounds
