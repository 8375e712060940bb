"""The two-view score and polish kernels (csrc/magsac_score.hip, csrc/refit.hip, refit_accept_kernel and the short-row MSAC kernel of
csrc/msac_score.hip), pinned bit for bit: every output of magsac_score, msac_score at N <= 256, refit_accept, local_optimize,
magsac_irls, refit_essential and refit_fundamental is compared, byte for byte, with tests/golden/twoview_kernels.npz.

The golden file pins what the kernels computed BEFORE the Sampson form, the threshold form, the model classification, the block score
pass and the pair scaffold of refit.hip were folded into one piece each: it was written by `python tests/test_gpu_twoview_pinned.py`
(write_golden below) with the library of commit ac71ff0 in place, and is re-recorded only by a change that means to alter what the
kernels compute.  A refactor that fails here has changed the grouping or the contraction of an expression: restore it.

Inputs come from CPU torch.Generator seeds through rand, +, * and / alone (no library routine whose rounding could differ between
machines); the pair states of the two polish ops are then made by the library's own score ops, as tests/test_gpu_local_opt.py and
tests/test_gpu_magsac_irls.py make theirs on the host.  Only outputs are stored, as bytes.

Shapes.  magsac_score (P, M, N): (2, 5, 3) and (2, 5, 64) the wave kernel with one point per lane; (2, 17, 130) four points per lane, a
ragged tail, a second model tile; (2, 17, 256) the wave / block boundary; (2, 33, 257) the block kernel, one chunk, a partial second
tile; (1, 33, 2049) two chunks.  Block kernels (256 threads): N = 8 (the minimum of the F fit), 257 (one row in the second stride),
600 (a partial third stride); the IRLS at 8, 64 and 300.  Gated: pair 1 closed, pair 0 open; at P = 1 the one pair closed.  P = 2 and P = 16: the light and the wave-cooperative E finish."""
import functools
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twoview_kernels.npz")
DTYPES = {"f32": torch.float32, "f64": torch.float64}
THR = 0.004                      # the cutoff on the Sampson distance is (1.5 THR)^2; the inliers' noise is 0.002 per coordinate
MAGSAC_SHAPES = [(2, 5, 3), (2, 5, 64), (2, 17, 130), (2, 17, 256), (2, 33, 257), (1, 33, 2049)]
MSAC_SHAPES = MAGSAC_SHAPES[:3]
BLOCK_NS = (8, 257, 600)
IRLS_NS = (8, 64, 300)
PAIRS = (2, 16)
FILL = 77


# ------------------------------------------------------------------------------------------------ inputs
def _scene(gen, N, share, noise=0.002):
    """-> (matches [N,4] f64, E [3,3] f64): x1 uniform in [-1, 1]^2 at depths in [2, 6], moved by the rotation of a random quaternion
    and a translation, x2 its projection plus uniform noise on the first round(share N) rows, the others' x2 uniform in [-1, 1]^2;
    E = [t]x R.  Products, sums and divisions only."""
    a, b, c, d = (0.3 * (2.0 * torch.rand(4, generator=gen, dtype=torch.float64) - 1.0)).tolist()
    a += 1.0
    s = a * a + b * b + c * c + d * d
    R = torch.tensor([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                      [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                      [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]], dtype=torch.float64) / s
    t = 2.0 * torch.rand(3, generator=gen, dtype=torch.float64) - 1.0
    x1 = 2.0 * torch.rand(N, 2, generator=gen, dtype=torch.float64) - 1.0
    z = 2.0 + 4.0 * torch.rand(N, generator=gen, dtype=torch.float64)
    X = torch.stack([x1[:, 0] * z, x1[:, 1] * z, z], 1)
    X2 = torch.stack([X[:, 0] * R[j, 0] + X[:, 1] * R[j, 1] + X[:, 2] * R[j, 2] + t[j] for j in range(3)], 1)
    x2 = X2[:, :2] / X2[:, 2:] + noise * (2.0 * torch.rand(N, 2, generator=gen, dtype=torch.float64) - 1.0)
    bad = 2.0 * torch.rand(N, 2, generator=gen, dtype=torch.float64) - 1.0
    x2 = torch.where((torch.arange(N) < round(share * N))[:, None], x2, bad)
    tx = torch.tensor([[0.0, -float(t[2]), float(t[1])], [float(t[2]), 0.0, -float(t[0])], [-float(t[1]), float(t[0]), 0.0]],
                      dtype=torch.float64)
    E = torch.stack([torch.stack([tx[i, 0] * R[0, j] + tx[i, 1] * R[1, j] + tx[i, 2] * R[2, j] for j in range(3)]) for i in range(3)])
    return torch.cat([x1, x2], 1), E


def _moved(gen, E, size):
    """E with every entry moved by up to `size` (no essential matrix any more: the kernels take any 3x3)"""
    return E + size * (2.0 * torch.rand(3, 3, generator=gen, dtype=torch.float64) - 1.0)


@functools.lru_cache(maxsize=None)
def _score_inputs(P, M, N):
    """models: the pair's E moved by 0.002 j per entry; slot M - 1 holds a NaN, slot M - 2 is all zero; valid marks both of pair 0's
    as live, slot 0 always, slot 1 never, the others four times in five"""
    gen = torch.Generator().manual_seed(1000 + N)
    sc = [_scene(gen, N, 0.6) for _ in range(P)]
    matches = torch.stack([s[0] for s in sc])
    models = torch.stack([torch.stack([_moved(gen, s[1], 0.002 * j) for j in range(M)]) for s in sc])
    models[:, M - 1, 1, 2] = float("nan")
    models[:, M - 2] = 0.0
    valid = torch.rand(P, M, generator=gen) < 0.8
    valid[:, 0] = True
    valid[0, M - 1] = True
    valid[0, M - 2] = True
    valid[:, 1] = False
    return matches, models, valid


def _gate(dev, dt, P, N):
    """a state whose last pair has terminated (P = 2: one open and one closed pair; P = 1: the closed pair alone)"""
    from differentiable_ransac_amd import ops
    st = ops.RansacState(P, N, 100, dev, dt)
    st.iters[P - 1] = 100
    return st


def _magsac_score_case(dev, dt, shape, want_inliers, use_valid, gated):
    from differentiable_ransac_amd import _lib as L
    P, M, N = shape
    matches, models, valid = _score_inputs(P, M, N)
    tm, tmod = matches.to(dev, dt), models.to(dev, dt).contiguous()
    tv = valid.to(dev).view(torch.uint8) if use_valid else None
    thr = torch.tensor((THR, 1.5 * THR)[:P], dtype=dt, device=dev)
    scores = torch.full((P, M), float(FILL), device=dev, dtype=dt)
    inl = torch.full((P, M), FILL, device=dev, dtype=torch.int32) if want_inliers else None
    st = _gate(dev, dt, P, N) if gated else None
    L.call(f"dr_magsac_score_{L.suffix(dt)}", L.ptr(tm), L.ptr(tmod), L.ptr(tv), L.ptr(thr), L.c_int(P), L.c_int(M), L.c_int(N),
           L.ptr(scores), L.ptr(inl), L.ptr(st.iters if gated else None), L.ptr(st.max_iters if gated else None), L.stream())
    if gated:
        assert bool((scores[P - 1] == FILL).all()) and (P == 1 or bool((scores[0] != FILL).any()))
    else:
        assert bool((scores != FILL).all())
    out = {"scores": scores}
    if want_inliers:
        out["inliers"] = inl
    return out


def _msac_score_case(dev, dt, shape, want_masks):
    from differentiable_ransac_amd import ops
    P, M, N = shape
    matches, models, valid = _score_inputs(P, M, N)
    thr = torch.tensor((THR, 1.5 * THR)[:P], dtype=dt, device=dev)
    scores, masks = ops.msac_score(matches.to(dev, dt), models.to(dev, dt), thr, want_masks=want_masks, valid=valid.to(dev))
    out = {"scores": scores}
    if want_masks:
        out["masks"] = masks
    return out


@functools.lru_cache(maxsize=None)
def _pair_inputs(P, N, seed, size):
    """P scenes (60 % inliers; all of them at N = 8) and their E moved by up to `size` per entry.  Pair p is distinct scene p % 4 (a
    block sees its own pair only), which keeps the bytes of the P = 16 cases in the file at a quarter"""
    gen = torch.Generator().manual_seed(seed + 100 * P + N)
    sc = [_scene(gen, N, 1.0 if N == 8 else 0.6) for _ in range(min(P, 4))]
    matches = torch.stack([s[0] for s in sc])
    start = torch.stack([_moved(gen, s[1], size) for s in sc])
    cyc = torch.arange(P) % 4
    return matches[cyc].contiguous(), start[cyc].contiguous()


@functools.lru_cache(maxsize=None)
def _accept_inputs(S, N):
    """P = 4, candidates [4,S,3,3]: the pair's E moved by 0.001 (1 + slot); an invalid, a non-finite and an all-zero one (S = 1: the
    candidates of pairs 1, 2 and 3; S = 10: slots 0, 3 and 5 of every pair, the invalid one the closest to E)"""
    matches, start = _pair_inputs(4, N, 2000 + S, 0.0)
    gen = torch.Generator().manual_seed(2100 + S + N)
    cand = torch.stack([torch.stack([_moved(gen, start[p], 0.001 * (1 + c)) for c in range(S)]) for p in range(4)])
    cvalid = torch.ones(4, S, dtype=torch.bool)
    if S == 1:
        cvalid[1, 0] = False
        cand[2, 0, 0, 1] = float("inf")
        cand[3, 0] = 0.0
    else:
        cvalid[:, 0] = False
        cand[:, 3, 2, 2] = float("nan")
        cand[:, 5] = 0.0
    return matches, cand, cvalid


def _accept_case(dev, dt, S, N, beaten):
    """best_score -1: every scored candidate beats it (an all-zero one would too, with its sum of 0); 1e6: none does"""
    from differentiable_ransac_amd import ops
    matches, cand, cvalid = _accept_inputs(S, N)
    best_score = torch.full((4,), -1.0 if beaten else 1e6, device=dev, dtype=dt)
    best_model = torch.eye(3, device=dev, dtype=dt).repeat(4, 1, 1)
    ops.refit_accept(matches.to(dev, dt), cand.to(dev, dt), cvalid.to(dev), torch.full((4,), THR, device=dev, dtype=dt), best_score,
                     best_model)
    return {"best_score": best_score, "best_model": best_model}


LO_KEYS = ("best_score", "best_model", "best_mask", "best_inliers", "max_iters")


def _lo_case(dev, dt, fmat, N, P, lo):
    """the pair states of tests/test_gpu_local_opt.py (a moved E with its own MSAC score, mask and count), by pair index mod 4: 0 and 3
    as they are, 1 with a snapshot that already equals the state (the early return), 2 (P = 16) a mask of four rows (no fit runs)"""
    from differentiable_ransac_amd import ops
    matches, start = _pair_inputs(P, N, 3000 + int(fmat), 0.0002 if N == 8 else 0.004)   # (N = 8: the mask keeps all eight rows)
    tm, ts = matches.to(dev, dt), start.to(dev, dt)
    thr = torch.full((P,), THR, device=dev, dtype=dt)
    score, mask = ops.msac_score(tm, ts[:, None].contiguous(), thr)
    st = ops.RansacState(P, N, 5000, dev, dt)
    st.best_score.copy_(score[:, 0])
    st.best_model.copy_(ts)
    st.best_mask.copy_(mask[:, 0])
    for p in range(2, P, 4):
        st.best_mask[p] = False
        st.best_mask[p, :4] = True
    st.best_inliers.copy_(st.best_mask.sum(-1).int())
    st.iters.fill_(16)
    seen = torch.full((P, 10), float("nan"), device=dev, dtype=dt)
    for p in range(1, P, 4):
        seen[p, 0] = st.best_score[p]
        seen[p, 1:] = st.best_model[p].reshape(9)
    refits = torch.zeros(P, device=dev, dtype=torch.int32)
    ops.local_optimize(st, tm, thr, fmat, lo, 4, 7 if fmat else 5, 0.999, 1e-5, 5000, seen, refits)
    assert int(refits[0]) >= 1 and int(refits[1]) == 0
    out = {k: getattr(st, k) for k in LO_KEYS}
    out.update(lo_seen=seen, lo_refits=refits)
    return out


def _irls_case(dev, dt, fmat, N, P, iters):
    """the pair states of tests/test_gpu_magsac_irls.py (a moved E with its own MAGSAC++ score); pair 1 under a threshold no point
    meets (the exit before the first fit)"""
    from differentiable_ransac_amd import ops
    matches, start = _pair_inputs(P, N, 4000 + int(fmat), 0.001)
    tm, ts = matches.to(dev, dt), start.to(dev, dt)
    thr = torch.full((P,), 4.0 * THR, device=dev, dtype=dt)
    thr[1] = 1e-9
    score, _ = ops.magsac_score(tm, ts[:, None].contiguous(), thr)
    st = ops.RansacState(P, N, 1000, dev, dt)
    st.best_model.copy_(ts)
    st.best_score.copy_(score[:, 0])
    fits = torch.zeros(P, device=dev, dtype=torch.int32)
    ops.magsac_irls(st, tm, thr, fmat, iters, fits, torch.empty(P, N, device=dev, dtype=dt))
    assert int(fits[0]) >= 1 and int(fits[1]) == 0
    return {"best_score": st.best_score, "best_model": st.best_model, "irls_fits": fits}


@functools.lru_cache(maxsize=None)
def _refit_inputs(P, N):
    """mask: half of the rows (the first eight always; at N = 8 all of them), pair 1 only four rows; weights in [0, 1] with 30 % zeros;
    both cycle with the scenes"""
    matches, _ = _pair_inputs(P, N, 5000, 0.0)
    gen = torch.Generator().manual_seed(5100 + 100 * P + N)
    D = min(P, 4)
    mask = torch.rand(D, N, generator=gen) < 0.5
    mask[:, :8] = True
    mask[1] = False
    mask[1, :4] = True
    weights = torch.rand(D, N, generator=gen, dtype=torch.float64)
    weights = torch.where(torch.rand(D, N, generator=gen) < 0.3, torch.zeros_like(weights), weights)
    weights[:, 0] = 0.75
    cyc = torch.arange(P) % 4
    return matches, mask[cyc].contiguous(), weights[cyc].contiguous()


def _refit_case(dev, dt, fmat, P, N, use_mask, use_weights):
    from differentiable_ransac_amd import ops
    matches, mask, weights = _refit_inputs(P, N)
    tm, tk = matches.to(dev, dt), mask.to(dev) if use_mask else None
    if fmat:
        models, valid = ops.refit_fundamental(tm, tk, weights.to(dev, dt) if use_weights else None)
    else:
        models, valid = ops.refit_essential(tm, tk)
    return {"models": models, "valid": valid}


def _cases():
    """{name: function of dev}"""
    c = {}
    for d, dt in DTYPES.items():
        for shape in MAGSAC_SHAPES:
            for wi in (0, 1):
                for uv in (0, 1):
                    for gated in (0, 1):
                        c[f"magsac_score_{d}_P{shape[0]}_M{shape[1]}_N{shape[2]}_inliers{wi}_valid{uv}_gated{gated}"] = (
                            lambda dev, dt=dt, shape=shape, wi=wi, uv=uv, gated=gated: _magsac_score_case(dev, dt, shape, wi, uv, gated))
        for shape in MSAC_SHAPES:
            for wm in (0, 1):
                c[f"msac_score_{d}_P{shape[0]}_M{shape[1]}_N{shape[2]}_masks{wm}"] = (
                    lambda dev, dt=dt, shape=shape, wm=wm: _msac_score_case(dev, dt, shape, wm))
        for N in BLOCK_NS:
            for S in (1, 10):
                for beaten in (0, 1):
                    c[f"refit_accept_{d}_S{S}_N{N}_beaten{beaten}"] = (
                        lambda dev, dt=dt, S=S, N=N, beaten=beaten: _accept_case(dev, dt, S, N, beaten))
        for fmat, m in ((True, "F"), (False, "E")):
            for P in PAIRS:
                for N in BLOCK_NS:
                    for lo in (1, 2):
                        c[f"local_opt_{d}_{m}_P{P}_N{N}_lo{lo}"] = (
                            lambda dev, dt=dt, fmat=fmat, P=P, N=N, lo=lo: _lo_case(dev, dt, fmat, N, P, lo))
                    for um in (0, 1):
                        for uw in (0, 1) if fmat else (0,):
                            c[f"refit_{d}_{m}_P{P}_N{N}_mask{um}_weights{uw}"] = (
                                lambda dev, dt=dt, fmat=fmat, P=P, N=N, um=um, uw=uw: _refit_case(dev, dt, fmat, P, N, um, uw))
                for N in IRLS_NS:
                    for iters in (1, 4):
                        c[f"irls_{d}_{m}_P{P}_N{N}_iters{iters}"] = (
                            lambda dev, dt=dt, fmat=fmat, P=P, N=N, iters=iters: _irls_case(dev, dt, fmat, N, P, iters))
    return c


CASES = _cases()


def _bytes(t):
    return t.detach().contiguous().cpu().view(torch.uint8).flatten()


def record(dev):
    """every output of every case as bytes, laid end to end in the order of sorted(CASES) and, within a case, of its sorted output
    names: one array and the offsets at which the outputs start"""
    parts, starts = [], [0]
    for name in sorted(CASES):
        got = CASES[name](dev)
        assert sorted(got) == _output_names(name), name
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
    if name.startswith("magsac_score"):
        return (["inliers"] if "_inliers1_" in name else []) + ["scores"]
    if name.startswith("msac_score"):
        return (["masks"] if name.endswith("masks1") else []) + ["scores"]
    if name.startswith("refit_accept"):
        return ["best_model", "best_score"]
    if name.startswith("local_opt"):
        return sorted(LO_KEYS + ("lo_seen", "lo_refits"))
    if name.startswith("irls"):
        return ["best_model", "best_score", "irls_fits"]
    return ["models", "valid"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_twoview_kernels_compute_what_was_recorded(dev, pinned, slots, name):
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
