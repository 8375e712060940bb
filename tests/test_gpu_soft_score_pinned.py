"""The soft-inlier score kernels of the two pose families, pinned bit for bit: <family>_soft_score_kernel<T, false | true> and
<family>_soft_score_points_kernel<T> (csrc/soft_score_device.hpp on the terms of csrc/pnp_soft_score.hip and
csrc/registration_soft_score.hip), reached through ops.pnp_soft_score and ops.registration_soft_score and their autograd.  scores,
grad_models and grad_matches of every case are compared, byte for byte, with tests/golden/soft_score_pinned.npz.

The two files were one algorithm written twice; the golden file was written by `python tests/test_gpu_soft_score_pinned.py`
(write_golden below) on one MI355X with the library of commit a25ae9f in place, while they were still two texts, and is re-recorded
only by a change that means to alter what the kernels compute.  A refactor that fails here has changed the grouping or the contraction
of an expression, or the order of a sum: restore it (docs/LOG.md 30 and 32 say where to look).  The wrappers allocate their outputs
themselves (torch.empty), so nothing can be pre-filled with a sentinel: an element that a kernel leaves unwritten holds whatever the
allocator returns.

Inputs come from the CPU generators tests/pnp_soft_score_ref.case and tests/registration_soft_score_ref.case (points, model slots,
the generator's keep; every dropped slot holds NaN) and from numpy Generators seeded here (masks, the further keep, the upstream
grad_scores); only outputs are stored, as bytes, an array above 32 KiB as its SHA-256 digest.  The golden file also holds the digest
of every case's inputs: test_inputs_are_what_was_recorded runs without a GPU, so a generator that drifts fails there and not as a
kernel change.

Cases, each for both families in f32 and f64 -- the smallest shapes at which each mechanism can go wrong (64 lanes; 256-point tiles
of the model-lane kernels; blocks of 8 waves and 512-model tiles of the point-lane kernel):
  p2_n63_m7      (P, N, M) = (2, 63, 7): less than a wave of points; fewer models than waves, so waves 7.. of the point kernel idle;
                 a mask of about half; one threshold
  p3_n257_m65    (3, 257, 65): one point in the second 256-point tile, one lane in the second model block; per-pair thresholds; a mask
                 of about half whose first 64 points are all off in pair 1 (a point-kernel wave without a masked point, and the
                 compaction across an empty ballot); keep drops about half
  p1_n65_m513    (1, 65, 513): one model in the second 512-model tile, one lane in the second point block; no mask, no keep
  specials       p3_n257_m65's inputs with NaN upstream gradients in every dropped slot (which hold NaN models), one more kept slot
                 of pair 1 with an inf entry, threshold 0 in pair 0 and NaN in pair 2
  models_only    the same, the matches not requiring a gradient: the point pass is not launched"""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soft_score_pinned.npz")
DTYPES = {"f32": torch.float32, "f64": torch.float64}
FAMILIES = ("pnp", "registration")
SHAPES = {"p2_n63_m7": (2, 63, 7), "p3_n257_m65": (3, 257, 65), "p1_n65_m513": (1, 65, 513)}
KINDS = tuple(SHAPES) + ("specials", "models_only")
DIGEST_ABOVE = 32 * 1024
BETA = 5.0


# ------------------------------------------------------------------------------------------------ inputs
def _ref(fam):
    from tests import pnp_ref, pnp_soft_score_ref, registration_soft_score_ref
    return (pnp_soft_score_ref, pnp_ref.THRESHOLD) if fam == "pnp" else (registration_soft_score_ref, registration_soft_score_ref.THRESHOLD)


@functools.lru_cache(maxsize=None)
def inputs(fam, kind):
    """-> dict(m [P,N,5 | 6], models [P,M,4,4], keep [P,M] bool | None, mask [P,N] bool | None, thr [P], gs [P,M]) in f64 numpy, and
    want_matches"""
    S, threshold = _ref(fam)
    base = kind if kind in SHAPES else "p3_n257_m65"
    P, N, M = SHAPES[base]
    c = S.case(P, N, M)
    rng = np.random.default_rng(3200 + 10 * KINDS.index(base) + FAMILIES.index(fam))
    m, models, keep = c["m"].copy(), c["models"].copy(), c["keep"].copy()
    mask = None if base == "p1_n65_m513" else rng.random((P, N)) < 0.5
    thr = np.full(P, threshold)
    if base == "p3_n257_m65":
        mask[1, :64] = False
        thr = threshold * np.array(S.THR_PAIRS)
        keep[:, :M - 4] &= rng.random((P, M - 4)) < 0.5 / keep[:, :M - 4].mean()      # (about half of the slots stay)
    if base == "p1_n65_m513":
        models[~keep] = 0.0                                       # (no keep: a slot the generator dropped is a kept model of zeros)
        keep = None
    else:
        models[~keep] = np.nan
    gs = rng.normal(size=(P, M))
    if kind in ("specials", "models_only"):
        gs[~keep] = np.nan
        models[1, np.flatnonzero(keep[1])[0], 0, 3] = np.inf
        thr[0], thr[2] = 0.0, np.nan
    return dict(m=m, models=models, keep=keep, mask=mask, thr=thr, gs=gs, want_matches=kind != "models_only")


def input_digest(fam, kind):
    inp, h = inputs(fam, kind), hashlib.sha256()
    for key in ("m", "models", "keep", "mask", "thr", "gs"):
        a = inp[key]
        h.update(key.encode() + (b"-" if a is None else str(a.shape).encode() + np.ascontiguousarray(a).tobytes()))
    return np.frombuffer(h.digest(), dtype=np.uint8)


def input_digests():
    """[len(FAMILIES) len(KINDS), 32] uint8, in the order of FAMILIES x KINDS"""
    return np.stack([input_digest(fam, kind) for fam in FAMILIES for kind in KINDS])


def test_inputs_are_what_was_recorded():
    with np.load(GOLDEN) as z:
        want = z["inputs"]
    got = input_digests()
    assert got.shape == want.shape
    for i, (fam, kind) in enumerate((f, k) for f in FAMILIES for k in KINDS):
        assert bytes(got[i]) == bytes(want[i]), (fam, kind)
    # the cases are what the module docstring says of them
    for fam in FAMILIES:
        a, b, s = inputs(fam, "p2_n63_m7"), inputs(fam, "p3_n257_m65"), inputs(fam, "specials")
        assert 0.25 < a["mask"].mean() < 0.75 and 0.25 < b["mask"].mean() < 0.75 and not b["mask"][1, :64].any()
        assert b["mask"][1, 64:].any() and b["mask"][:, 256].any() and 0.25 < b["keep"].mean() < 0.75
        assert len(set(b["thr"])) == 3 and (b["thr"] > 0).all() and inputs(fam, "p1_n65_m513")["mask"] is None
        assert np.isnan(s["models"][~s["keep"]]).all() and np.isnan(s["gs"][~s["keep"]]).all() and not np.isnan(s["gs"][s["keep"]]).any()
        assert np.isinf(s["models"][1][s["keep"][1]]).any() and s["thr"][0] == 0.0 and s["thr"][1] > 0 and np.isnan(s["thr"][2])


# ------------------------------------------------------------------------------------------------ cases
def _case(dev, fam, kind, dt):
    from differentiable_ransac_amd import ops
    inp = inputs(fam, kind)

    def to(a, t=None):
        return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev, t)
    tm = to(inp["m"], dt).requires_grad_(inp["want_matches"])
    tmo = to(inp["models"], dt).requires_grad_(True)
    scores = getattr(ops, f"{fam}_soft_score")(tm, tmo, to(inp["thr"], dt), BETA, to(inp["mask"]), to(inp["keep"]))
    scores.backward(to(inp["gs"], dt))
    assert (tm.grad is not None) == inp["want_matches"]
    out = {"scores": scores.detach(), "grad_models": tmo.grad}
    if inp["want_matches"]:
        out["grad_matches"] = tm.grad
    return out


CASES = {f"{fam}_{kind}_{d}": (lambda dev, fam=fam, kind=kind, dt=dt: _case(dev, fam, kind, dt))
         for fam in FAMILIES for kind in KINDS for d, dt in DTYPES.items()}


def _output_names(name):
    return ["grad_models", "scores"] if "_models_only_" in name else ["grad_matches", "grad_models", "scores"]


def _bytes(t):
    """the tensor's bytes, or their SHA-256 digest where they are more than DIGEST_ABOVE"""
    b = t.detach().contiguous().cpu().view(torch.uint8).flatten()
    if b.numel() > DIGEST_ABOVE:
        b = torch.frombuffer(bytearray(hashlib.sha256(b.numpy().tobytes()).digest()), dtype=torch.uint8)
    return b


def record(dev):
    """every output of every case as bytes (or their digest), laid end to end in the order of sorted(CASES) and, within a case, of its
    sorted output names: one array and the offsets at which the outputs start; and the digests of the inputs"""
    parts, starts = [], [0]
    for name in sorted(CASES):
        got = CASES[name](dev)
        assert sorted(got) == _output_names(name), name
        for key in sorted(got):
            parts.append(_bytes(got[key]).numpy())
            starts.append(starts[-1] + parts[-1].size)
    return {"data": np.concatenate(parts), "start": np.asarray(starts, dtype=np.int64), "inputs": input_digests()}


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


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_soft_score_computes_what_was_recorded(dev, pinned, slots, name):
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
