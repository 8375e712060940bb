"""The reverse passes of the two Gram-eigenvector fits, pinned bit for bit: refit_homography_bwd_kernel (csrc/homography.hip (4b)) and
refit_fundamental_bwd_kernel (csrc/refit_fundamental_bwd.hip), reached through the autograd of ops.weighted_homography and
ops.weighted_fundamental.  grad_matches, grad_weights, the model and valid of every case are compared, byte for byte, with
tests/golden/weighted_fit_bwd.npz.

The two kernels are one algorithm written twice and are meant to share one scaffold; the golden file pins what they compute while they
are still two texts.  It was written by `python tests/test_gpu_weighted_fit_pinned.py` (write_golden below) with the library of commit
8f383ea in place, and is re-recorded only by a change that means to alter what the kernels compute.  A refactor that fails here has
changed the grouping or the contraction of an expression: restore it.  (A first merge of the two texts failed exactly the f64
grad_matches cases, in the second image's columns only, by one rounding of the result: docs/LOG.md 30.)

Inputs come from CPU torch.Generator seeds through rand, +, * and / alone (floor, for the integer offsets of the centroid case, is
exact); only outputs are stored, as bytes.  One plane-induced map x1 -> m(x1) serves both families: the homography's second point is
m(x1), the fundamental's lies on the line from a fixed epipole through m(x1), at 0.6 ... 1.4 of the way (rows that satisfy the rank-2
F = [e]_x H up to the noise).  Uniform noise of one pixel; the first 30 % of the rows have a second point uniform in the image
instead.  Weights: 0.5 ... 1 on the regular rows, 0.05 ... 0.25 on the scattered ones.

Cases, each in f32 and f64 and for both families (R = the family's minimal row count, 4 | 8; 256 threads own rows n, n + 256, ...):
  min            N = R, P = 2, no weights, no mask
  n257_masked    N = 257 (one row in the second stride), P = 2, weighted, about half the rows masked in
  n600           N = 600 (a partial third stride), P = 2, weighted, no mask
  short          N = 257, P = 3, weighted; pair 0's mask keeps R - 1 rows: every element of the pair an exact zero, valid = 0
  repeated       N = 16, P = 2, weighted; the eight rows pair 0's mask keeps are one point (of quarter-pixel coordinates: every sum is
                 exact, the centred rows are zeros): no simple smallest eigenvalue, exact zeros
  centroid       N = 13, P = 1, weighted: six integer offsets and their negatives about an integer centre in either image, the last
                 row exactly at both centroids (tests/fundamental_grad_ref.centroid_case's construction)
  weights_only   n257_masked's inputs, only the weights require a gradient: grad_matches is null
  matches_only   the same, only the matches require one

characters() checks on the CPU, with the f64 references' kappa (tests/homography_grad_ref.py, tests/fundamental_grad_ref.py) on the
inputs as either dtype sees them, that every case is what it is meant to be: every pair of the regular cases has a finite kappa below
the references' KAPPA_MAX, the short pair has R - 1 rows and the repeated-point pair is degenerate (kappa = inf).  write_golden runs
it before it records, and test_inputs_have_their_character runs it without a GPU."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weighted_fit_bwd.npz")
DTYPES = {"f32": torch.float32, "f64": torch.float64}
MIN_ROWS = {"homography": 4, "fundamental": 8}
SIDE = 640.0
H_PLANE = ((0.9, -0.2, 40.0), (0.25, 1.1, -30.0), (1e-4, -2e-4, 1.0))
EPIPOLE = (900.0, -150.0)
SCATTER = 0.3
KINDS = ("min", "n257_masked", "n600", "short", "repeated", "centroid", "weights_only", "matches_only")
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ inputs
def _rand(gen, *shape):
    return torch.rand(*shape, generator=gen, dtype=F64)


def _scene(gen, fam, N):
    """-> (matches [N,4] f64, scattered [N] bool): the module docstring's rows; the scattered ones stand first"""
    x1 = SIDE * _rand(gen, N, 2)
    x, y = x1[:, 0], x1[:, 1]
    (a, b, c), (d, e, f), (g, h, i) = H_PLANE
    wz = g * x + h * y + i
    m = torch.stack([(a * x + b * y + c) / wz, (d * x + e * y + f) / wz], 1)
    if fam == "fundamental":
        ep = torch.tensor(EPIPOLE, dtype=F64)
        m = ep + (0.6 + 0.8 * _rand(gen, N, 1)) * (m - ep)
    x2 = m + (2.0 * _rand(gen, N, 2) - 1.0)
    scattered = torch.arange(N) < round(SCATTER * N)
    x2 = torch.where(scattered[:, None], SIDE * _rand(gen, N, 2), x2)
    return torch.cat([x1, x2], 1), scattered


def _weights(gen, scattered):
    u = _rand(gen, *scattered.shape)
    return torch.where(scattered, 0.05 + 0.2 * u, 0.5 + 0.5 * u)


def _centroid_rows(gen):
    """[13,4]: +-o_k about an integer centre in either image, the centre itself last"""
    o1, o2 = ((81.0 * _rand(gen, 6, 2)).floor() - 40.0 for _ in range(2))
    c1, c2 = torch.tensor([100.0, 50.0], dtype=F64), torch.tensor([120.0, 70.0], dtype=F64)
    return torch.cat([torch.cat([c1 + o1, c1 - o1, c1[None]]), torch.cat([c2 + o2, c2 - o2, c2[None]])], 1)


def inputs(fam, kind):
    """-> dict(matches [P,N,4], weights [P,N] | None, mask [P,N] bool | None, grad [P,3,3], want = (matches, weights)), f64 on the CPU"""
    R = MIN_ROWS[fam]
    base = "n257_masked" if kind in ("weights_only", "matches_only") else kind
    gen = torch.Generator().manual_seed(700 + 10 * KINDS.index(base) + (fam == "fundamental"))
    P, N = {"min": (2, R), "n257_masked": (2, 257), "n600": (2, 600), "short": (3, 257), "repeated": (2, 16), "centroid": (1, 13)}[base]
    if base == "centroid":
        matches, scattered = _centroid_rows(gen)[None], torch.zeros(1, 13, dtype=torch.bool)
    else:
        sc = [_scene(gen, fam, N) for _ in range(P)]
        matches, scattered = torch.stack([s[0] for s in sc]), torch.stack([s[1] for s in sc])
    weights = None if base == "min" else _weights(gen, scattered)
    mask = None
    if base in ("n257_masked", "short"):
        mask = torch.rand(P, N, generator=gen) < 0.5
    if base == "short":
        mask[0] = False
        mask[0, 37 * torch.arange(R - 1)] = True
    if base == "repeated":
        mask = torch.ones(P, N, dtype=torch.bool)
        mask[0, 8:] = False
        matches[0, :8] = torch.tensor([100.25, 50.5, 120.75, 70.0], dtype=F64)
    grad = 2.0 * _rand(gen, P, 3, 3) - 1.0
    return dict(matches=matches, weights=weights, mask=mask, grad=grad, want=(kind != "weights_only", kind != "matches_only"))


def characters():
    """{(fam, kind, dtype): [kappa of pair p, ...]} from the f64 references, after asserting what the module docstring says of them"""
    from tests import fundamental_grad_ref, homography_grad_ref
    refs = {"homography": homography_grad_ref, "fundamental": fundamental_grad_ref}
    out = {}
    for fam, ref in refs.items():
        for kind in KINDS[:6]:
            inp = inputs(fam, kind)
            for d, dt in DTYPES.items():
                ks = []
                for p in range(inp["matches"].shape[0]):
                    sel = torch.ones(inp["matches"].shape[1], dtype=torch.bool) if inp["mask"] is None else inp["mask"][p]
                    x = inp["matches"][p][sel].to(dt).double().numpy()
                    w = None if inp["weights"] is None else inp["weights"][p][sel].to(dt).double().numpy()
                    if kind == "short" and p == 0:
                        assert len(x) == MIN_ROWS[fam] - 1
                        ks.append(float("inf"))
                        continue
                    assert len(x) >= MIN_ROWS[fam]
                    if kind == "repeated" and p == 0:
                        # (the centred rows are exact zeros: the reference's Gram matrix is NaN, which its eigh may also refuse)
                        assert (x == x[0]).all()
                        try:
                            ks.append(ref.kappa(x, w))
                        except torch.linalg.LinAlgError:
                            ks.append(float("inf"))
                        assert ks[-1] == float("inf"), (fam, kind, d, p, ks[-1])
                    else:
                        ks.append(ref.kappa(x, w))
                        assert ks[-1] < ref.KAPPA_MAX, (fam, kind, d, p, ks[-1])
                out[fam, kind, d] = ks
    return out


def test_inputs_have_their_character():
    characters()


# ------------------------------------------------------------------------------------------------ cases
def _case(dev, fam, kind, dt):
    from differentiable_ransac_amd import ops
    inp = inputs(fam, kind)
    want_m, want_w = inp["want"]
    tm = inp["matches"].to(dev, dt).requires_grad_(want_m)
    tw = None if inp["weights"] is None else inp["weights"].to(dev, dt).requires_grad_(want_w)
    mask = None if inp["mask"] is None else inp["mask"].to(dev)
    model, valid = getattr(ops, f"weighted_{fam}")(tm, tw, mask)
    model.backward(inp["grad"].to(dev, dt))
    assert (tm.grad is not None) == want_m
    out = {"model": model.detach(), "valid": valid}
    if want_m:
        out["grad_matches"] = tm.grad
    if tw is not None and want_w:
        out["grad_weights"] = tw.grad
    if kind == "short":
        assert not bool(valid[0]) and bool(valid[1:].all())
        for g in (tm.grad[0], tw.grad[0]):
            assert bool((g == 0).all())
    return out


CASES = {f"{fam}_{kind}_{d}": (lambda dev, fam=fam, kind=kind, dt=dt: _case(dev, fam, kind, dt))
         for fam in MIN_ROWS for kind in KINDS for d, dt in DTYPES.items()}


def _output_names(name):
    names = ["model", "valid"]
    if "_weights_only_" not in name:
        names.append("grad_matches")
    if "_matches_only_" not in name and "_min_" not in name:
        names.append("grad_weights")
    return sorted(names)


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
    characters()
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_weighted_fit_backward_computes_what_was_recorded(dev, pinned, slots, name):
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
