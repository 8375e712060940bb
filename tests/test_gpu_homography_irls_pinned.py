"""homography_irls_kernel of csrc/homography.hip, pinned bit for bit: best_score, best_model and irls_fits of every case are compared,
byte for byte, with tests/golden/homography_irls_pinned.npz (tests/test_gpu_registration_pinned.py does the same for the
registration kernels, its local optimisation and IRLS polish included).

The golden file pins what the kernel computed while it was a text of its own, before the polish kernels of the pair-state families
were folded into one accept loop and one block score (csrc/pair_state_device.hpp): it was written by
`python tests/test_gpu_homography_irls_pinned.py` (write_golden below) on one MI355X with the library of commit 1a0e515 in place, and
is re-recorded only by a change that means to alter what the kernel computes.  A refactor that fails here has changed the grouping or
the contraction of an expression, the order of a sum or the order of the loop's exits: restore it.

Inputs come from CPU torch.Generator seeds through rand, +, -, * and / alone (no library routine whose rounding could differ between
machines: the transfer of a point is written out, not a matrix product); only outputs are stored, as bytes in one array with offsets.
The golden file also holds the digest of every case's inputs: test_inputs_are_what_was_recorded runs without a GPU, so a generator
that drifts fails there and not as a kernel change.

Cases: f32 and f64; N = 4 (the minimum row count of a fit), 257 (one row in the second 256-thread stride), 600 (a partial third
stride); irls_iters = 1 and 4.  Six pair states each (after tests/test_gpu_homography_magsac.py and the registration file's
_irls_case): 0 and 1 the generating homography of the pair's scene moved by up to MOVED pixels, with a claimed score of 0.5 (the first
candidate wins, the later ones compare real scores); 2 the identity on an all-outlier pair (fewer than four rows: no fit); 3 a NaN
model and 4 a rank-one matrix of integers (det = 0 exactly): neither has rows; 5 a moved homography under a best_score of 1e6 (one
fit, which loses).  best_mask, best_inliers, iters and max_iters are filled at random and must come back byte-equal.

The pin reaches every exit of the loop -- test_golden_reaches_every_exit reads that off the recorded file, without a GPU: at N = 257
and 600 with four steps, in either type, a pair ran two fits or more, a pair ran a fit and kept its model (a candidate that lost), a
pair ran none, and a pair's model changed.  MOVED = 1 pixel leaves most inliers of pairs 0 and 1 inside the 3-pixel cutoff of their
start models, and tests/homography_magsac_ref.irls (the f64 oracle) takes two candidates or more from them on these inputs."""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "homography_irls_pinned.npz")
DTYPES = {"f32": torch.float32, "f64": torch.float64}
NS = (4, 257, 600)
ITERS = (1, 4)
P = 6
THR = 3.0
SIDE = 640.0
MOVED = 1.0
MAXIT = 1000
CLAIMED = (0.5, 0.5, 0.0, 0.0, 0.0, 1e6)
KEPT = ("best_mask", "best_inliers", "iters", "max_iters")
OUTPUTS = ("best_model", "best_score", "irls_fits")


# ------------------------------------------------------------------------------------------------ inputs
def _homography(gen):
    """scale 0.8-1.2 with a rotation-like part up to 0.3, a shift up to 40 pixels, perspective terms up to 3e-4 (the third coordinate
    stays above 0.6 on the square); not normalised: the kernel takes any matrix with det != 0"""
    r = torch.rand(6, generator=gen, dtype=torch.float64).tolist()
    a, b = 0.8 + 0.4 * r[0], 0.6 * r[1] - 0.3
    return torch.tensor([[a, -b, 80.0 * r[2] - 40.0], [b, a, 80.0 * r[3] - 40.0], [6e-4 * r[4] - 3e-4, 6e-4 * r[5] - 3e-4, 1.0]],
                        dtype=torch.float64)


def _scene(gen, N, share, noise=0.5):
    """-> (matches [N,4] f64, H): x1 uniform in the square; the first round(share N) rows are H x1 with uniform noise of up to `noise`
    pixels, the others' x2 uniform in the square (the rows are not shuffled: the kernel does not depend on their order)"""
    H = _homography(gen)
    x1 = SIDE * torch.rand(N, 2, generator=gen, dtype=torch.float64)
    x, y = x1[:, 0], x1[:, 1]
    w = H[2, 0] * x + H[2, 1] * y + H[2, 2]
    good = torch.stack([(H[0, 0] * x + H[0, 1] * y + H[0, 2]) / w, (H[1, 0] * x + H[1, 1] * y + H[1, 2]) / w], 1)
    good = good + noise * (2.0 * torch.rand(N, 2, generator=gen, dtype=torch.float64) - 1.0)
    bad = SIDE * torch.rand(N, 2, generator=gen, dtype=torch.float64)
    x2 = torch.where((torch.arange(N) < round(share * N))[:, None], good, bad)
    return torch.cat([x1, x2], 1), H


def _moved(gen, H, size):
    """H with every entry moved so that a point of the square moves by up to about `size` pixels per entry"""
    unit = torch.tensor([[1.0 / SIDE, 1.0 / SIDE, 1.0], [1.0 / SIDE, 1.0 / SIDE, 1.0],
                         [1.0 / (SIDE * SIDE), 1.0 / (SIDE * SIDE), 1.0 / SIDE]], dtype=torch.float64)
    return H + size * unit * (2.0 * torch.rand(3, 3, generator=gen, dtype=torch.float64) - 1.0)


@functools.lru_cache(maxsize=None)
def inputs(N):
    """-> dict of f64 / bool / int32 CPU tensors: matches [P,N,4], start [P,3,3], score [P], and the fill of the fields the kernel must
    leave alone"""
    gen = torch.Generator().manual_seed(600 + N)
    sc = [_scene(gen, N, (1.0 if N == 4 else 0.6) if p != 2 else 0.0) for p in range(P)]
    matches = torch.stack([s[0] for s in sc])
    start = torch.stack([_moved(gen, s[1], MOVED) for s in sc])
    start[2] = torch.eye(3, dtype=torch.float64)
    start[3] = float("nan")
    start[4] = torch.tensor([[1.0, -1.0, 2.0], [2.0, -2.0, 4.0], [3.0, -3.0, 6.0]], dtype=torch.float64)
    return dict(matches=matches, start=start, score=torch.tensor(CLAIMED, dtype=torch.float64),
                best_mask=torch.rand(P, N, generator=gen) < 0.5,
                best_inliers=(N * torch.rand(P, generator=gen, dtype=torch.float64)).to(torch.int32),
                iters=(900.0 * torch.rand(P, generator=gen, dtype=torch.float64)).to(torch.int32),
                max_iters=1.0 + 999.0 * torch.rand(P, generator=gen, dtype=torch.float64))


def _det3(h):
    return float(h[0, 0] * (h[1, 1] * h[2, 2] - h[1, 2] * h[2, 1]) - h[0, 1] * (h[1, 0] * h[2, 2] - h[1, 2] * h[2, 0])
                 + h[0, 2] * (h[1, 0] * h[2, 1] - h[1, 1] * h[2, 0]))


def input_digests():
    """[len(NS), 32] uint8"""
    out = []
    for N in NS:
        h = hashlib.sha256()
        for key, t in sorted(inputs(N).items()):
            h.update(key.encode() + str(tuple(t.shape)).encode() + t.contiguous().view(torch.uint8).numpy().tobytes())
        out.append(np.frombuffer(h.digest(), dtype=np.uint8))
    return np.stack(out)


def test_inputs_are_what_was_recorded():
    with np.load(GOLDEN) as z:
        want = z["inputs"]
    got = input_digests()
    assert got.shape == want.shape
    for i, N in enumerate(NS):
        assert bytes(got[i]) == bytes(want[i]), N
    # the pair states are what the module docstring says of them
    for N in NS:
        s = inputs(N)["start"]
        assert bool(torch.isnan(s[3]).all()) and torch.equal(s[2], torch.eye(3, dtype=s.dtype))
        assert torch.equal(s[4, 1], 2.0 * s[4, 0]) and torch.equal(s[4, 2], 3.0 * s[4, 0])      # rank one, in integers
        assert bool(torch.isfinite(s[[0, 1, 5]]).all()) and all(_det3(s[p]) > 0.5 for p in (0, 1, 5))


# ------------------------------------------------------------------------------------------------ cases
def _case(dev, dt, N, iters):
    from differentiable_ransac_amd import ops
    inp = inputs(N)
    tm = inp["matches"].to(dev, dt)
    st = ops.HomographyState(P, N, MAXIT, dev, dt)
    st.best_model.copy_(inp["start"])
    st.best_score.copy_(inp["score"])
    for k in KEPT:
        getattr(st, k).copy_(inp[k])
    keep = {k: getattr(st, k).clone() for k in KEPT}
    fits = torch.zeros(P, device=dev, dtype=torch.int32)
    ops.homography_irls(st, tm, ops.thr2_tensor(THR, P, tm), iters, fits)
    for k, v in keep.items():
        assert torch.equal(getattr(st, k).view(torch.uint8), v.view(torch.uint8)), k
    return {"best_score": st.best_score, "best_model": st.best_model, "irls_fits": fits}


CASES = {f"irls_{d}_N{N}_iters{iters}": (lambda dev, dt=dt, N=N, iters=iters: _case(dev, dt, N, iters))
         for d, dt in DTYPES.items() for N in NS for iters in ITERS}
SLOT = {name: len(OUTPUTS) * i for i, name in enumerate(sorted(CASES))}      # a case's first output among the golden file's offsets


def _bytes(t):
    return t.detach().contiguous().cpu().view(torch.uint8).flatten()


def record(dev):
    """every output of every case as bytes, laid end to end in the order of sorted(CASES) and, within a case, of OUTPUTS (sorted): one
    array and the offsets at which the outputs start; and the digests of the inputs"""
    parts, starts = [], [0]
    for name in sorted(CASES):
        got = CASES[name](dev)
        assert tuple(sorted(got)) == OUTPUTS, name
        for key in OUTPUTS:
            parts.append(_bytes(got[key]).numpy())
            starts.append(starts[-1] + parts[-1].size)
    return {"data": np.concatenate(parts), "start": np.asarray(starts, dtype=np.int64), "inputs": input_digests()}


def write_golden(path=GOLDEN):
    np.savez_compressed(path, **record(torch.device("cuda:0")))


@pytest.fixture(scope="module")
def pinned():
    with np.load(GOLDEN) as z:
        return torch.from_numpy(z["data"]), z["start"]


def _recorded(pinned, name, key):
    data, start = pinned
    i = SLOT[name] + OUTPUTS.index(key)
    return data[int(start[i]):int(start[i + 1])]


def test_golden_reaches_every_exit(pinned):
    """a condition on the inputs, read off the recorded outputs: with four steps at N = 257 and 600, in either type, the loop was left
    through each of its exits"""
    assert len(pinned[1]) - 1 == len(OUTPUTS) * len(CASES)
    for d, dt in DTYPES.items():
        for N in NS[1:]:
            name = f"irls_{d}_N{N}_iters4"
            fits = _recorded(pinned, name, "irls_fits").view(torch.int32)
            model = _recorded(pinned, name, "best_model").reshape(P, -1)
            same = torch.tensor([torch.equal(model[p], _bytes(inputs(N)["start"][p].to(dt))) for p in range(P)])
            assert bool((fits >= 2).any()), (name, fits.tolist())                   # a candidate won and the loop went on
            assert bool(((fits >= 1) & same).any()), (name, fits.tolist())          # a fit whose candidate lost
            assert bool((fits == 0).any()), (name, fits.tolist())                   # left before a fit
            assert bool((~same).any()), name                                         # a candidate was taken
            assert bool(same[2:].all()) and fits[2:].tolist() == [0, 0, 0, 1], (name, fits.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_homography_irls_computes_what_was_recorded(dev, pinned, name):
    got = CASES[name](dev)
    assert tuple(sorted(got)) == OUTPUTS
    for key in OUTPUTS:
        assert torch.equal(_bytes(got[key]), _recorded(pinned, name, key)), (name, key)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_golden(*sys.argv[1:2])
