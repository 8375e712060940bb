"""The kernels of csrc/registration.hip, pinned bit for bit: every output of the two score ops, refit_rigid and its backward, the
three sample-fit ops, registration_local_optimize and registration_irls is compared, byte for byte, with
tests/golden/registration_kernels.npz.

The golden file pins what the kernels computed BEFORE the two score kernels, the moment passes and the candidate score passes
were folded into one helper each (the two backward ops are reached through autograd: ops.kabsch, ops.weighted_kabsch): it was written by `python tests/test_gpu_registration_pinned.py`
(write_golden below) with the library of commit 0eb87c0 in place, and is re-recorded only by a change that means to alter what the
kernels compute.  A refactor that fails here has changed the grouping or the contraction of an expression: restore it.

Inputs come from CPU torch.Generator seeds through rand, +, * and / alone (no library routine whose rounding could differ between
machines); only outputs are stored, as bytes (NaN snapshots and -1 scores are part of the state).

Shapes.  Score ops (P, N, M): (2, 5, 3) fewer than the 8 points of a lane; (2, 2049, 17) one point in the second 2048-point chunk and
one model in the second 16-model tile; (1, 4100, 33) three chunks, three tiles.  Block kernels (256 threads): N = 3, 257 (one row in
the second stride), 600 (a partial third stride).  Sample fits: Bt = 70 lanes (a second block of six), k = 3 and 8; the 70 samples
cycle through ten distinct ones (eight regular, a degenerate one, one whose weights are all zero), which keeps every lane's bytes in
the file at a tenth of the size."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "registration_kernels.npz")
DTYPES = {"f32": torch.float32, "f64": torch.float64}
THR = 0.05
PAIR_THR = (0.05, 0.08)
SCORE_SHAPES = [(2, 5, 3), (2, 2049, 17), (1, 4100, 33)]
BLOCK_NS = (3, 257, 600)
FILL = 77
MAXIT = 1000


# ------------------------------------------------------------------------------------------------ inputs
def _pose(gen):
    """a 4x4 rigid pose, f64: the rotation of a random quaternion by products and one division, a translation in [-1, 1]^3"""
    a, b, c, d = (2.0 * torch.rand(4, generator=gen, dtype=torch.float64) - 1.0).tolist()
    s = a * a + b * b + c * c + d * d
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = torch.tensor([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                              [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                              [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]], dtype=torch.float64) / s
    M[:3, 3] = 2.0 * torch.rand(3, generator=gen, dtype=torch.float64) - 1.0
    return M


def _scene(gen, N, share, noise=0.01):
    """-> (matches [N,6] f64, pose): unit-cube points, uniform noise on the first round(share N) rows, the others' q uniform in a
    cube of side 4 (the rows are not shuffled: no kernel here depends on their order)"""
    M = _pose(gen)
    p = torch.rand(N, 3, generator=gen, dtype=torch.float64)
    q = p @ M[:3, :3].T + M[:3, 3] + noise * (2.0 * torch.rand(N, 3, generator=gen, dtype=torch.float64) - 1.0)
    bad = 4.0 * torch.rand(N, 3, generator=gen, dtype=torch.float64) - 2.0
    q = torch.where((torch.arange(N) < round(share * N))[:, None], q, bad)
    return torch.cat([p, q], 1), M


def _moved(gen, M, size):
    """M with every entry of [R | t] moved by up to `size` (not a rotation any more: the score and IRLS kernels take any matrix)"""
    out = M.clone()
    out[:3] += size * (2.0 * torch.rand(3, 4, generator=gen, dtype=torch.float64) - 1.0)
    return out


def _score_inputs(P, N, M):
    gen = torch.Generator().manual_seed(100 + N)
    sc = [_scene(gen, N, 0.6) for _ in range(P)]
    matches = torch.stack([s[0] for s in sc])
    models = torch.stack([torch.stack([_moved(gen, s[1], 0.004 * j) for j in range(M)]) for s in sc])
    models[0, M - 1, 1, 2] = float("nan")
    valid = torch.rand(P, M, generator=gen) < 0.8
    valid[:, 0] = True
    valid[0, M - 1] = True          # (the NaN model is scored)
    valid[:, 1] = False
    return matches, models, valid


def _score_case(dev, dt, op, shape, mode):
    from differentiable_ransac_amd import _lib as L
    from differentiable_ransac_amd import ops
    P, N, M = shape
    matches, models, valid = _score_inputs(P, N, M)
    tm, tmod, tv = matches.to(dev, dt), models.to(dev, dt), valid.to(dev)
    thr = torch.tensor(PAIR_THR[:P], dtype=dt, device=dev)
    fn = getattr(ops, f"rigid_{op}_score")
    if mode == "counts":
        scores, inl = fn(tm, tmod, thr, tv)
        return {"scores": scores, "inliers": inl}
    if mode == "scores_only":
        scores, none = fn(tm, tmod, thr, tv, want_inliers=False)
        assert none is None
        return {"scores": scores}
    # the gate: pair 1 has terminated, its cells keep what the buffers were filled with
    st = ops.RegistrationState(P, N, 100, dev, dt)
    st.iters[1] = 100
    scores = torch.full((P, M), float(FILL), device=dev, dtype=dt)
    inl = torch.full((P, M), FILL, device=dev, dtype=torch.int32)
    L.call(f"dr_rigid_{op}_score_{L.suffix(dt)}", L.ptr(tm), L.ptr(tmod), L.ptr(tv.view(torch.uint8)), L.ptr(thr * thr), L.c_int(P),
           L.c_int(M), L.c_int(N), L.ptr(scores), L.ptr(inl), L.ptr(st.iters), L.ptr(st.max_iters), L.stream())
    assert bool((scores[1] == FILL).all()) and bool((inl[1] == FILL).all()) and bool((inl[0] != FILL).any())
    return {"scores": scores, "inliers": inl}


def _refit_inputs(N, sparse):
    """P = 4.  mask: pair 0 keeps a share of its rows (at least three), pair 1 two rows, pair 2 rows whose p lie on one line, pair 3 a
    share again; weights with zeros.  `sparse` (the backward, whose outputs are [P,N,6]): shares of 0.15 and 90 % zero weights, else 1/2
    and 30 %."""
    gen = torch.Generator().manual_seed(200 + N)
    sc = [_scene(gen, N, 0.8) for _ in range(4)]
    matches = torch.stack([s[0] for s in sc])
    share = 0.15 if sparse else 0.5
    mask = torch.rand(4, N, generator=gen) < share
    mask[:, :3] = True
    mask[1] = False
    mask[1, [0, N - 1]] = True
    line = torch.arange(N, dtype=torch.float64)[:, None] * torch.tensor([0.25, -0.5, 0.125], dtype=torch.float64) / N
    matches[2, :, :3] = torch.where(mask[2][:, None], line + 0.5, matches[2, :, :3])
    matches[2, :, 3:] = torch.where(mask[2][:, None], matches[2, :, :3] @ sc[2][1][:3, :3].T + sc[2][1][:3, 3], matches[2, :, 3:])
    weights = torch.rand(4, N, generator=gen, dtype=torch.float64)
    weights = torch.where(torch.rand(4, N, generator=gen) < (0.9 if sparse else 0.3), torch.zeros_like(weights), weights)
    weights[:, 0] = 0.75
    grad = 2.0 * torch.rand(4, 4, 4, generator=gen, dtype=torch.float64) - 1.0
    return matches, mask, weights, grad


def _refit_case(dev, dt, N, use_mask, use_weights):
    from differentiable_ransac_amd import ops
    matches, mask, weights, _ = _refit_inputs(N, False)
    model, valid = ops.refit_rigid(matches.to(dev, dt), mask.to(dev) if use_mask else None, weights.to(dev, dt) if use_weights else None)
    return {"model": model, "valid": valid}


def _refit_bwd_case(dev, dt, N, use_mask, use_weights):
    from differentiable_ransac_amd import ops
    matches, mask, weights, grad = _refit_inputs(N, True)
    tm = matches.to(dev, dt).requires_grad_(True)
    tw = weights.to(dev, dt).requires_grad_(True) if use_weights else None
    model, valid = ops.weighted_kabsch(tm, tw, mask.to(dev) if use_mask else None)
    model.backward(grad.to(dev, dt))
    out = {"model": model.detach(), "valid": valid, "grad_matches": tm.grad}
    if use_weights:
        out["grad_weights"] = tw.grad
    return out


KABSCH_BT, KABSCH_DISTINCT = 70, 10


def _kabsch_inputs(k):
    """-> (matches [2,40,6], idx [2,35,k] int32, samples [70,k,6], weights [70,k], grad [70,4,4]): sample s holds the rows of distinct
    sample s % 10 (the explicit samples all from pair 0, the gather from the pair of s); 8 is degenerate (k times one row), 9 has zero
    weights; the last index set of the gather holds one index = N"""
    gen = torch.Generator().manual_seed(300 + k)
    N = 40
    sc = [_scene(gen, N, 1.0) for _ in range(2)]
    matches = torch.stack([s[0] for s in sc])
    rows = torch.stack([torch.randperm(N, generator=gen)[:k] for _ in range(KABSCH_DISTINCT)]).to(torch.int32)
    rows[8] = rows[8, 0]
    idx = rows[torch.arange(KABSCH_BT) % KABSCH_DISTINCT].reshape(2, 35, k).clone()
    samples = matches[0][idx.reshape(KABSCH_BT, k).long()]
    idx_bad = idx.clone()
    idx_bad[1, 34, k - 1] = N
    w = torch.rand(KABSCH_DISTINCT, k, generator=gen, dtype=torch.float64)
    w[0, 1] = 0.0
    w[9] = 0.0
    g = 2.0 * torch.rand(KABSCH_DISTINCT, 4, 4, generator=gen, dtype=torch.float64) - 1.0
    cyc = torch.arange(KABSCH_BT) % KABSCH_DISTINCT
    return matches, idx_bad, samples, w[cyc], g[cyc]


def _kabsch_case(dev, dt, k, use_weights):
    from differentiable_ransac_amd import ops
    _, _, samples, weights, grad = _kabsch_inputs(k)
    ts = samples.to(dev, dt).requires_grad_(True)
    tw = weights.to(dev, dt).requires_grad_(True) if use_weights else None
    models, valid = ops.kabsch(ts, tw)
    models.backward(grad.to(dev, dt))
    out = {"models": models.detach(), "valid": valid, "grad_samples": ts.grad}
    if use_weights:
        out["grad_weights"] = tw.grad
    return out


def _gather_case(dev, dt, k):
    from differentiable_ransac_amd import ops
    matches, idx, _, _, _ = _kabsch_inputs(k)
    models, valid = ops.kabsch_gather(matches.to(dev, dt), idx.to(dev))
    assert not bool(valid[1, 34]) and bool(valid[0, 0])
    return {"models": models, "valid": valid}


STATE_KEYS = ("best_score", "best_model", "best_mask", "best_inliers", "iters", "max_iters")


def _state_inputs(N, seed, size):
    """five scenes (60 % inliers, all of them at N = 3; pair 3 without any) and their generating poses moved by up to `size` per entry"""
    gen = torch.Generator().manual_seed(seed + N)
    sc = [_scene(gen, N, (1.0 if N == 3 else 0.6) if p != 3 else 0.0) for p in range(5)]
    matches = torch.stack([s[0] for s in sc])
    start = torch.stack([_moved(gen, s[1], size) for s in sc])
    return gen, matches, start


def _lo_case(dev, dt, N, lo):
    """the pair states of tests/test_gpu_registration_lo.py: 0 a seed the first refit beats, 1 the same with a snapshot that already
    equals the state, 2 a mask of two rows, 3 an all-outlier pair with a few rows selected, 4 a terminated pair (LO does not ask).
    The masks, counts and stop bounds are registration_update's for the start models, with a claimed score of 1; above N = 3 the
    start models are 0.04 per entry off, so that their masks hold a part of the inliers and lo = 2 goes through several fits."""
    from differentiable_ransac_amd import ops
    gen, matches, start = _state_inputs(N, 400, 0.01 if N == 3 else 0.04)
    tm = matches.to(dev, dt)
    st = ops.RegistrationState(5, N, MAXIT, dev, dt)
    ops.registration_update(st, tm, start.to(dev, dt).unsqueeze(1).contiguous(), None, torch.ones(5, 1, device=dev, dtype=dt), THR, 64)
    two = torch.zeros(N, dtype=torch.bool)
    two[[0, N - 1]] = True
    st.best_mask[2] = two.to(dev)
    st.best_inliers[2] = 2
    few = torch.zeros(N, dtype=torch.bool)
    few[torch.randperm(N, generator=gen)[:min(N, 5)]] = True
    st.best_mask[3] = few.to(dev)
    st.best_inliers[3] = int(few.sum())
    st.best_score[3] = 0.0
    st.iters[4] = MAXIT
    st.max_iters[4] = 640.0
    seen = torch.full((5, 17), float("nan"), device=dev, dtype=dt)
    seen[1, 0] = st.best_score[1]
    seen[1, 1:] = st.best_model[1].reshape(16)
    refits = torch.zeros(5, device=dev, dtype=torch.int32)
    ops.registration_local_optimize(st, tm, ops.thr2_tensor(THR, 5, tm), lo, 4, 0.999, 1e-5, MAXIT, seen, refits)
    out = {k: getattr(st, k) for k in STATE_KEYS}
    out.update(lo_seen=seen, lo_refits=refits)
    return out


def _irls_case(dev, dt, N, iters):
    """the pair states of tests/test_gpu_registration_magsac.py: 0 and 1 moved poses with a claimed score of 0.5 (the first candidate
    wins, the later ones compare real scores), 2 the identity on an all-outlier pair, 3 a NaN model, 4 a moved pose under a
    best_score no fit reaches.  The other state fields are random and must come back untouched."""
    from differentiable_ransac_amd import ops
    gen, matches, start = _state_inputs(N, 500, 0.01)
    matches[2], matches[3] = matches[3].clone(), matches[2].clone()      # (the all-outlier scene goes to pair 2)
    start[2] = torch.eye(4, dtype=torch.float64)
    start[3] = float("nan")
    tm = matches.to(dev, dt)
    st = ops.RegistrationState(5, N, MAXIT, dev, dt)
    st.best_model.copy_(start)
    st.best_score.copy_(torch.tensor([0.5, 0.5, 0.0, 0.0, 1e6], dtype=torch.float64))
    st.best_mask.copy_(torch.rand(5, N, generator=gen) < 0.5)
    st.best_inliers.copy_(torch.randint(0, N, (5,), generator=gen).to(torch.int32))
    st.iters.copy_(torch.randint(0, 900, (5,), generator=gen).to(torch.int32))
    st.max_iters.copy_(1.0 + 999.0 * torch.rand(5, generator=gen, dtype=torch.float64))
    keep = {k: getattr(st, k).clone() for k in ("best_mask", "best_inliers", "iters", "max_iters")}
    fits = torch.zeros(5, device=dev, dtype=torch.int32)
    ops.registration_irls(st, tm, ops.thr2_tensor(THR, 5, tm), iters, fits)
    for k, v in keep.items():
        assert torch.equal(getattr(st, k).view(torch.uint8), v.view(torch.uint8)), k
    return {"best_score": st.best_score, "best_model": st.best_model, "irls_fits": fits}


def _cases():
    """{name: function of dev}"""
    c = {}
    for d, dt in DTYPES.items():
        for op in ("msac", "magsac"):
            for shape in SCORE_SHAPES:
                s = f"{op}_score_{d}_P{shape[0]}_N{shape[1]}_M{shape[2]}"
                for mode in ("counts", "scores_only") + (("gated",) if shape[0] == 2 else ()):
                    c[f"{s}_{mode}"] = lambda dev, dt=dt, op=op, shape=shape, mode=mode: _score_case(dev, dt, op, shape, mode)
        for N in BLOCK_NS:
            for um in (False, True):
                for uw in (False, True):
                    c[f"refit_{d}_N{N}_mask{int(um)}_weights{int(uw)}"] = (
                        lambda dev, dt=dt, N=N, um=um, uw=uw: _refit_case(dev, dt, N, um, uw))
            for lo in (1, 2):
                c[f"local_opt_{d}_N{N}_lo{lo}"] = lambda dev, dt=dt, N=N, lo=lo: _lo_case(dev, dt, N, lo)
            for iters in (1, 4):
                c[f"irls_{d}_N{N}_iters{iters}"] = lambda dev, dt=dt, N=N, iters=iters: _irls_case(dev, dt, N, iters)
        for N in BLOCK_NS[:2]:
            # (no mask with weights: both gradients of every row; a mask without weights; both: the three ways the rows are chosen)
            for um, uw in ((False, True), (True, False), (True, True)):
                c[f"refit_bwd_{d}_N{N}_mask{int(um)}_weights{int(uw)}"] = (
                    lambda dev, dt=dt, N=N, um=um, uw=uw: _refit_bwd_case(dev, dt, N, um, uw))
        for k in (3, 8):
            for uw in (False, True):
                c[f"kabsch_{d}_k{k}_weights{int(uw)}"] = lambda dev, dt=dt, k=k, uw=uw: _kabsch_case(dev, dt, k, uw)
            c[f"kabsch_gather_{d}_k{k}"] = lambda dev, dt=dt, k=k: _gather_case(dev, dt, k)
    return c


CASES = _cases()


def _bytes(t):
    return t.detach().contiguous().cpu().view(torch.uint8).flatten()


def record(dev):
    """every output of every case as bytes, laid end to end in the order of sorted(CASES) and, within a case, of its sorted output
    names: one array and the offsets at which the outputs start (one file entry per output would cost more in archive headers
    than in data)"""
    parts, starts = [], [0]
    for name in sorted(CASES):
        got = CASES[name](dev)
        for key in sorted(got):
            parts.append(_bytes(got[key]).numpy())
            starts.append(starts[-1] + parts[-1].size)
    return {"data": np.concatenate(parts), "start": np.asarray(starts, dtype=np.int64)}


def write_golden(path=GOLDEN):
    np.savez_compressed(path, **record(torch.device("cuda:0")))


@pytest.fixture(scope="module")
def pinned():
    with np.load(GOLDEN) as z:
        return torch.from_numpy(z["data"]), z["start"]


@pytest.fixture(scope="module")
def slots():
    """({case: index of its first output among the golden file's offsets}, number of outputs)"""
    out, i = {}, 0
    for name in sorted(CASES):
        out[name] = i
        i += len(_output_names(name))
    return out, i


def _output_names(name):
    if "_score_" in name:
        return ["scores"] if name.endswith("scores_only") else ["inliers", "scores"]
    if name.startswith("refit_bwd"):
        return ["grad_matches"] + (["grad_weights"] if name.endswith("weights1") else []) + ["model", "valid"]
    if name.startswith("refit"):
        return ["model", "valid"]
    if name.startswith("kabsch_gather"):
        return ["models", "valid"]
    if name.startswith("kabsch"):
        return ["grad_samples"] + (["grad_weights"] if name.endswith("weights1") else []) + ["models", "valid"]
    if name.startswith("local_opt"):
        return sorted(STATE_KEYS + ("lo_seen", "lo_refits"))
    return ["best_model", "best_score", "irls_fits"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_registration_kernels_compute_what_was_recorded(dev, pinned, slots, name):
    data, start = pinned
    first, total = slots
    assert total == len(start) - 1
    got = CASES[name](dev)
    assert sorted(got) == _output_names(name)
    for i, key in enumerate(sorted(got)):
        a, b = int(start[first[name] + i]), int(start[first[name] + i + 1])
        assert torch.equal(_bytes(got[key]), data[a:b]), (name, key)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_golden(*sys.argv[1:2])
