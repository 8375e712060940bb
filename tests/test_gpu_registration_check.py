"""dr_kabsch_gather_checked and ransac.BatchedRegistration(edge_similarity=...) on the GPU, against the f64 oracle
tests/registration_check_ref.py and against dr_kabsch_gather byte for byte.

Shapes (registration_check_ref.CASES): P = 2, N = 300, B = 130 -- a partial last wave, a partial block of 256, samples of both pairs
inside one wave and one block -- with k = 3 and k = 4 (six edges), and B = 700: six blocks, the last one partial, so the offsets of the
compaction across waves are used.  The scenes are synth.rigid_pair at 70 % outliers, the index sets ops.gumbel_topk's on explicit noise
plus two written by hand per pair (an index out of range, a repeated row); edge_similarity 0, 0.9 and 1.  The decision is compared outside
the oracle's margin (1e-9 for f64, 1e-5 for f32: the kernel decides in f64 on the same values, so only the fusing of its three-term sums
separates them), which may leave out at most 1 % of the samples; tests/test_registration_check_host.py asserts that cap on the oracle's
side.  Every test prints its figures before it asserts."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import registration_check_ref as C
from tests import registration_ref as R

pytestmark = pytest.mark.gpu

THR = R.THRESHOLD


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@functools.lru_cache(maxsize=None)
def _inputs(name, B):
    m, logits = C.scenes(name)
    return m, logits, C.noise(B, name)


# ------------------------------------------------------------------------------------------------ dr_kabsch_gather_checked
@pytest.mark.parametrize("name", ["float32", "float64"])
@pytest.mark.parametrize("B,k", C.CASES)
def test_checked_gather_against_oracle_and_unchecked_gather(dev, name, B, k):
    from differentiable_ransac_amd import ops
    m, logits, g = _inputs(name, B)
    tm = m.to(dev)
    idx = C.hand_made(ops.gumbel_topk(logits.to(dev), B, k, 1.0, g.to(dev), 0, soft=False)["idx"].cpu())
    assert torch.equal(idx, C.host_index_sets(logits, g, k)), "the sets the host test checked the cap on"
    tidx = idx.to(dev)
    want_m, want_v = ops.kabsch_gather(tm, tidx)
    eye = torch.eye(4, dtype=m.dtype)
    mw = m.double().numpy()                                       # the stored values, widened
    for sim in C.SIMILARITIES:
        rej = torch.zeros(C.P, device=dev, dtype=torch.int32)
        models, valid = ops.kabsch_gather_checked(tm, tidx, sim, rej)
        rej2 = torch.zeros(C.P, device=dev, dtype=torch.int32)
        models2, valid2 = ops.kabsch_gather_checked(tm, tidx, sim, rej2)
        assert _same_bytes(models, models2) and _same_bytes(valid, valid2) and torch.equal(rej, rej2), "a repeated launch, same bytes"
        none_m, none_v = ops.kabsch_gather_checked(tm, tidx, sim)             # rejected = NULL: not counted, same outputs
        assert _same_bytes(models, none_m) and _same_bytes(valid, none_v)
        mc, vc, wm, wv = models.cpu(), valid.cpu(), want_m.cpu(), want_v.cpu()
        left = survivors = 0
        for p in range(C.P):
            passed, margin, in_range = C.check(mw[p], idx[p].numpy(), sim)
            sure = margin >= C.LEFT_OUT[name]
            left += int((~sure).sum())
            for b in range(B):
                if vc[p, b]:                                      # a model was fitted: it is the unchecked kernel's, bit for bit
                    assert wv[p, b] and _same_bytes(mc[p, b], wm[p, b]), (sim, p, b)
                    survivors += 1
                else:
                    assert torch.equal(mc[p, b], eye), (sim, p, b)
                if not sure[b]:
                    continue
                if passed[b] or not in_range[b]:                  # what the unchecked kernel writes, degenerate samples included
                    assert bool(vc[p, b]) == bool(wv[p, b]) and _same_bytes(mc[p, b], wm[p, b]), (sim, p, b)
                else:
                    assert not vc[p, b], (sim, p, b)
            lo = int((~passed & in_range & sure).sum())
            assert lo <= int(rej[p]) <= lo + int((~sure).sum()), (sim, p, int(rej[p]), lo)
            assert not vc[p, 3] and not in_range[3], "the sample with an index out of range"
        print(f"{name} B={B} k={k} similarity {sim}: rejected {rej.cpu().tolist()}, fitted {survivors}, left out {left}/{C.P * B}")
        assert left <= C.LEFT_OUT_CAP * C.P * B
        if sim == 0.0:
            assert _same_bytes(models, want_m) and _same_bytes(valid, want_v) and int(rej.abs().sum()) == 0
        if sim == 0.9:
            assert 0 < survivors < C.P * B and int(rej.sum()) > 0


def test_checked_gather_special_rows(dev):
    """small integers (exact in both types): a NaN row fails at every similarity and is counted; coincident rows pass the check and the
    fit then rejects them, uncounted; a rigid triple passes at 1.0"""
    from differentiable_ransac_amd import ops
    for dt in (torch.float32, torch.float64):
        m = torch.tensor([[[0, 0, 0, 1, 1, 1], [2, 0, 0, 1, 3, 1], [0, 3, 0, -2, 1, 1], [0, 0, 5, 1, 1, 6],     # q = Rz(90) p + 1
                           [1, 2, 3, 4, 5, 6], [float("nan"), 0, 0, 0, 0, 0], [9, 9, 9, 0, 0, 0]]], dtype=dt)
        idx = torch.tensor([[[0, 1, 2], [0, 1, 5], [4, 4, 4], [0, 1, 6], [1, 2, 3]]], dtype=torch.int32)
        for sim, want_rej in ((0.0, 1), (0.9, 2), (1.0, 2)):
            rej = torch.zeros(1, device=dev, dtype=torch.int32)
            models, valid = ops.kabsch_gather_checked(m.to(dev), idx.to(dev), sim, rej)
            ref_m, ref_v = ops.kabsch_gather(m.to(dev), idx.to(dev))
            print(f"{dt} similarity {sim}: valid {valid.cpu().tolist()}, rejected {int(rej)}")
            assert valid.cpu().tolist() == [[True, False, False, sim == 0.0, True]]
            assert int(rej) == want_rej
            for b in (0, 2, 4):
                assert _same_bytes(models[0, b], ref_m[0, b]) and bool(valid[0, b]) == bool(ref_v[0, b])


# ------------------------------------------------------------------------------------------------ BatchedRegistration
DRIVER_MODES = [(0, "msac"), (2, "msac"), (0, "magsac")]          # (lo, scoring); the constructor refuses lo != 0 with "magsac"
KEYS = {"msac": ["model", "mask", "score", "inliers", "iterations", "rejected"]}
KEYS["magsac"] = KEYS["msac"] + ["irls_fits"]


def test_constructor_still_refuses_lo_with_magsac():
    from differentiable_ransac_amd.ransac import BatchedRegistration
    with pytest.raises(ValueError, match="MSAC"):
        BatchedRegistration(edge_similarity=0.9, lo=2, scoring="magsac")


@pytest.mark.parametrize("lo,scoring", DRIVER_MODES)
def test_driver_equals_the_loop_of_ops_calls(dev, lo, scoring):
    from differentiable_ransac_amd import ops
    from differentiable_ransac_amd.ransac import BatchedRegistration, _Seeds
    m, logits, _ = _inputs("float32", 130)
    tm, tl = m.to(dev), logits.to(dev)
    B, rounds, sim, seed = 130, 4, 0.9, 5
    kw = dict(ransac_batch_size=B, threshold=THR, max_iterations=rounds * B, seed=seed, lo=lo, scoring=scoring)
    out = BatchedRegistration(edge_similarity=sim, **kw)(tm, tl)
    plain = BatchedRegistration(**kw)(tm, tl)
    assert "rejected" in out and "rejected" not in plain
    assert out["rejected"].dtype == torch.int32 and out["rejected"].shape == (C.P,)
    # the loop
    seeds = _Seeds(seed)
    st = ops.RegistrationState(C.P, C.N, rounds * B, dev, tm.dtype)
    thr2 = ops.thr2_tensor(THR, C.P, tm)
    rejected = torch.zeros(C.P, device=dev, dtype=torch.int32)
    lo_seen = torch.full((C.P, 17), float("nan"), device=dev, dtype=tm.dtype)
    lo_refits = torch.zeros(C.P, device=dev, dtype=torch.int32)
    score_fn = ops.rigid_magsac_score if scoring == "magsac" else ops.rigid_msac_score
    for r in range(rounds):
        idx = ops.gumbel_topk(tl, B, 3, 1.0, None, seeds.next(), soft=False)["idx"]
        models, valid = ops.kabsch_gather_checked(tm, idx, sim, rejected)
        scores, _ = score_fn(tm, models, None, valid, want_inliers=False, thr2=thr2)
        ops.registration_update(st, tm, models, valid, scores, None, B, 0.999, 1e-5, thr2=thr2)
        if lo:
            ops.registration_local_optimize(st, tm, thr2, lo, 64, 0.999, 1e-5, rounds * B, lo_seen, lo_refits)
        if r + 1 < rounds and not bool((st.iters.double() < st.max_iters).any()):
            break
    model, score = st.best_model, st.best_score
    want = dict(mask=st.best_mask, inliers=st.best_inliers, iterations=st.iters, rejected=rejected)
    if scoring == "magsac":
        want["irls_fits"] = torch.zeros(C.P, device=dev, dtype=torch.int32)
        ops.registration_irls(st, tm, thr2, 10, want["irls_fits"])
    else:
        cand, cvalid = ops.refit_rigid(tm, st.best_mask)
        cscore, _ = ops.rigid_msac_score(tm, cand.unsqueeze(1), None, cvalid.unsqueeze(1), want_inliers=False, thr2=thr2)
        take = cscore[:, 0] > score
        model = torch.where(take[:, None, None], cand, model)
        score = torch.where(take, cscore[:, 0], score)
    want.update(model=model, score=score)
    if lo:
        want["lo_refits"] = lo_refits
    print(f"lo={lo} {scoring}: iterations {out['iterations'].cpu().tolist()}, rejected {out['rejected'].cpu().tolist()}, "
          f"inliers {out['inliers'].cpu().tolist()}")
    assert sorted(out) == sorted(want)
    for key in want:
        assert _same_bytes(out[key], want[key]), key
    assert int(out["rejected"].sum()) > 0


USE = dict(P=8, N=512, B=1024, max_iterations=5000, seed=3, sim=0.9)


def test_driver_is_as_useful_on_ninety_percent_outliers(dev):
    """eight synth.rigid_pair scenes of N = 512 with 10 % inliers, flat logits, f32; the same seed with and without the check, so the
    checked call scores a subset of the unchecked call's models.
     - rotation error below 2 degrees, the bound tests/test_gpu_registration.py applies to the unchecked driver;
     - the checked score is lower than the unchecked one on no pair.  On the CPU (the oracle's state step and refit on uniform triplets,
       five rounds of 1024, scenes 0..119, the same draws for both) the checked score was lower on 0 of 120 scenes: the check drops
       99.5 % of the draws, and when it drops the unchecked winner another all-inlier sample leads the refit to the same inlier set;
     - more than half of all draws are rejected."""
    from differentiable_ransac_amd import synth
    from differentiable_ransac_amd.ransac import BatchedRegistration
    sc = [synth.rigid_pair(s, USE["N"], 0.1) for s in range(USE["P"])]
    tm = torch.stack([s["matches"] for s in sc]).to(dev)
    logits = torch.zeros(USE["P"], USE["N"], device=dev)
    kw = dict(ransac_batch_size=USE["B"], threshold=THR, max_iterations=USE["max_iterations"], seed=USE["seed"])
    out = BatchedRegistration(edge_similarity=USE["sim"], **kw)(tm, logits)
    plain = BatchedRegistration(**kw)(tm, logits)
    err = [R.rotation_error_deg(out["model"][p].cpu().double().numpy(), sc[p]["gt_T"][:3, :3].double().numpy()) for p in range(USE["P"])]
    lower = int((out["score"] < plain["score"]).sum())
    draws = int(out["iterations"].sum())
    print(f"rotation error (deg) {[round(e, 3) for e in err]}; score checked {out['score'].cpu().tolist()} unchecked "
          f"{plain['score'].cpu().tolist()}; rejected {int(out['rejected'].sum())} of {draws} draws")
    assert max(err) < 2.0
    assert lower <= LOWER_ALLOWED
    assert int(out["rejected"].sum()) > 0.5 * draws


LOWER_ALLOWED = 0      # of USE["P"] = 8 pairs: the share the CPU experiment shows (0 of 120), see the test's docstring


@pytest.mark.parametrize("name", ["float32", "float64"])
def test_device_termination_counts_every_issued_round_and_replays(dev, name):
    """The fit is not gated on the device: `rejected` counts the samples dropped in every round the call ISSUED, also for a pair that
    had terminated by then.  Three scenes of 0.6 / 0.35 / 0.15 inliers, explicit noise, six rounds of 64: under device_termination all
    six are issued; the host-terminated call issues them until no pair continues.  Everything else of the result is the same bit for
    bit, eagerly and replayed from a graph."""
    from differentiable_ransac_amd import ops, synth
    from differentiable_ransac_amd.graphs import GraphedStep
    from differentiable_ransac_amd.ransac import BatchedRegistration
    dt = C.DTYPES[name]
    P, N, B, rounds, sim = 3, 300, 64, 6, 0.9
    tm = torch.from_numpy(np.stack([R.scene(900 + p, N, s)["matches"] for p, s in enumerate((0.6, 0.35, 0.15))])).to(dev, dt)
    logits = torch.zeros(P, N, device=dev, dtype=dt)
    g = [synth.gumbel_noise((P, B, N), seed=1000 + r, dtype=dt).to(dev) for r in range(rounds)]
    kw = dict(ransac_batch_size=B, threshold=THR, max_iterations=rounds * B, edge_similarity=sim)
    host = BatchedRegistration(**kw)(tm, logits, gumbels=g)
    dterm = BatchedRegistration(**kw)
    dterm.device_termination = True
    eager = dterm(tm, logits, gumbels=g)
    per_round = []
    for x in g:
        rej = torch.zeros(P, device=dev, dtype=torch.int32)
        ops.kabsch_gather_checked(tm, ops.gumbel_topk(logits, B, 3, 1.0, x, 0, soft=False)["idx"], sim, rej)
        per_round.append(rej.cpu())
    its = host["iterations"].cpu().tolist()
    host_rounds = max(its) // B
    print(f"{name}: iterations {its}, rejected host {host['rejected'].cpu().tolist()} device {eager['rejected'].cpu().tolist()}, "
          f"per round {[r.tolist() for r in per_round]}")
    assert min(its) < max(its) and math.ceil(min(its) / B) < host_rounds, "a pair stopped while the call went on"
    for key in ("model", "mask", "score", "inliers", "iterations"):
        assert _same_bytes(host[key], eager[key]), key
    assert torch.equal(eager["rejected"].cpu(), torch.stack(per_round).sum(0))
    assert torch.equal(host["rejected"].cpu(), torch.stack(per_round[:host_rounds]).sum(0))
    step = GraphedStep(lambda: dterm(tm, logits, gumbels=g), warmup=1)
    for _ in range(2):
        replay = step()
        torch.cuda.synchronize()
        for key in ("model", "mask", "score", "inliers", "iterations", "rejected"):
            assert _same_bytes(eager[key], replay[key]), key
