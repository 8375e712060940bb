"""The register-resident sampler kernel (gumbel_topk_fast_kernel, csrc/gumbel_topk.hip), pinned bit for bit: idx, samples and, in
train mode, y_sel and lse of `ops.gumbel_topk_gather` and of the fused `ops.SampleGather.apply` forward are compared with
tests/golden/sampler_register_kernel.npz.

The golden file pins what the kernel computed BEFORE its short-row screened variant was removed and its three winner writes and
two exact thresholds were folded into one helper each: it was written by `python tests/test_gpu_sampler_register_kernel.py`
(write_golden below) with the library and ops.py of commit 311cc72 in place, and is re-recorded only by a change that means to
alter what the kernel computes.

Shapes: P = 2 pairs and B = 6 rows -- not a multiple of the four rows (waves) of a block, so two waves of the last block exit
early; N = 8 / 500 / 2048 points -- one 64-lane group of which two lanes hold elements, a partial last group, all eight register
groups; k = 1 / 5 / 8."""
import inspect
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_register_kernel.npz")
P, B = 2, 6
SHAPES = [(N, k) for N in (8, 500, 2048) for k in (1, 5, 8)]
FILL = 7


def _inputs(dev, N, kind):
    gen = torch.Generator().manual_seed(1000 + N)
    matches = torch.randn(P, N, 4, generator=gen)
    if kind == "normal":
        logits = torch.randn(P, N, generator=gen)
    elif kind == "constant":
        logits = torch.full((P, N), 1e8)    # (ulp 8: the scores take two or three values, 1e8 + 8 where the noise exceeds 4)
    elif kind == "ties":
        logits = torch.full((P, N), 1e9)    # (ulp 64, |noise| < 17: EVERY score rounds to 1e9)
    else:                                   # one dominant logit per pair (within the span the race form accepts)
        logits = torch.randn(P, N, generator=gen)
        logits[0, N // 3] += 30.0
        logits[1, N - 1] += 30.0
    return matches.to(dev), logits.to(dev)


def _test_mode(dev, N, k, kind, race, sub=0):
    from differentiable_ransac_amd import ops
    m, lg = _inputs(dev, N, kind)
    idx, smp = ops.gumbel_topk_gather(m, lg, B, k, 1.0, 77, sub=sub, race=race)
    return {"idx": idx, "samples": smp}


def _train_mode(dev, N, k, kind, race):
    """the fused SampleGather forward; lse is what the node saves for its backward"""
    from differentiable_ransac_amd import ops
    m, lg = _inputs(dev, N, kind)
    was = ops.K1_RACE_SOFT, ops._RACE_MIN
    ops.K1_RACE_SOFT, ops._RACE_MIN = race, (1, 1)
    try:
        smp, y_sel, idx = ops.SampleGather.apply(m, lg.requires_grad_(True), B, k, 1.0, None, 77)
    finally:
        ops.K1_RACE_SOFT, ops._RACE_MIN = was
    lse = smp.grad_fn.saved_tensors[4]
    return {"idx": idx, "samples": smp.detach(), "y_sel": y_sel.detach(), "lse": lse}


def _gated(dev, N, k):
    """a direct call of the entry into pre-filled buffers, with a state in which pair 1 has reached its bound"""
    from differentiable_ransac_amd import _lib as L
    from differentiable_ransac_amd import ops
    m, lg = _inputs(dev, N, "normal")
    st = ops.RansacState(P, N, 100, dev, torch.float32)
    st.iters[1] = 100
    idx = torch.full((P, B, k), FILL, device=dev, dtype=torch.int32)
    smp = torch.full((P, B, k, 4), float(FILL), device=dev, dtype=torch.float32)
    # (commit 311cc72, at which the golden file was recorded, took the screening workspace of the removed variant after `samples`)
    legacy = (L.ptr(None),) if "screen" in inspect.signature(ops.gumbel_topk_gather).parameters else ()
    L.call("dr_gumbel_topk_gather_f32", L.ptr(lg), L.ptr(m), *ops._seed_args(77), L.c_float(1.0), L.c_int(P), L.c_int(B), L.c_int(N),
           L.c_int(k), L.ptr(idx), L.ptr(smp), *legacy, *ops._gate_args(st), L.c_int(0), L.ptr(None), L.c_int(0), L.stream())
    return {"idx": idx, "samples": smp}


def _cases():
    """{name: (function of dev, the branch of the kernel the case was built to reach)}"""
    c = {}
    for N, k in SHAPES:
        s = f"N{N}_k{k}"
        for race in (False, True):
            r = "race" if race else "twolog"
            c[f"test_{s}_normal_{r}"] = (lambda dev, N=N, k=k, race=race: _test_mode(dev, N, k, "normal", race),
                                         "index-only kernel, wave-mask selection: exactly k candidates (no ranking) or a few more "
                                         "(ranked over v_readlane); race: the counted threshold, else the k-th lane maximum")
            c[f"test_{s}_dominant_{r}"] = (lambda dev, N=N, k=k, race=race: _test_mode(dev, N, k, "dominant", race),
                                           "one point wins every row: its lane's maximum is far above the other 63 (race: the "
                                           "threshold search starts far from the count it wants)")
            c[f"train_{s}_normal_{r}"] = (lambda dev, N=N, k=k, race=race: _train_mode(dev, N, k, "normal", race),
                                          "kSoft kernel: y_sel, lse and the straight-through gather of the winner write; race: the "
                                          "soft-max statistics from the reciprocals of the keys, else the online soft-max")
            c[f"train_{s}_dominant_{r}"] = (lambda dev, N=N, k=k, race=race: _train_mode(dev, N, k, "dominant", race),
                                            "kSoft kernel with one weight near 1 and the others near 0")
        c[f"test_{s}_constant_twolog"] = (lambda dev, N=N, k=k: _test_mode(dev, N, k, "constant", False),
                                          "massive ties on two or three score levels: the (value, index) ranking of the mask selection "
                                          "among ties; rows with fewer than k scores on the top level have > 64 candidates -> slow path")
        c[f"train_{s}_constant_twolog"] = (lambda dev, N=N, k=k: _train_mode(dev, N, k, "constant", False),
                                           "the same under kSoft")
        c[f"test_{s}_ties_twolog"] = (lambda dev, N=N, k=k: _test_mode(dev, N, k, "ties", False),
                                      "every score ties: N > 64 -> more than 64 candidates in the masks AND in the LDS list -> the tie "
                                      "slow path (k arg-max rounds, winners 0 .. k-1); N = 8 -> the mask selection ranks eight ties by index")
        c[f"train_{s}_ties_twolog"] = (lambda dev, N=N, k=k: _train_mode(dev, N, k, "ties", False),
                                       "the tie slow path under kSoft: its winner write with y_sel = 1 / N and the straight-through gather")
    for race in (False, True):
        r = "race" if race else "twolog"
        c[f"test_N500_k5_sub3_{r}"] = (lambda dev, race=race: _test_mode(dev, 500, 5, "normal", race, sub=3),
                                       "sub-batches: rows 3..5 draw rows 0..2 of the call keyed seed + 1 (sub_batch_row)")
    c["test_N500_k5_gated"] = (lambda dev: _gated(dev, 500, 5), "the gate: the blocks of a terminated pair return at once")
    return c


CASES = _cases()


KEYS = ("idx", "samples", "y_sel", "lse")


def record(dev):
    """the outputs of every case, flattened and laid end to end in the order of sorted(CASES): per output name one array and the
    offsets at which the cases start in it (one file entry per case would cost more in archive headers than in data)"""
    parts = {key: [] for key in KEYS}
    starts = {key: [0] for key in KEYS}
    for name in sorted(CASES):
        got = CASES[name][0](dev)
        for key in KEYS:
            if key in got:
                parts[key].append(got[key].cpu().numpy().ravel())
            starts[key].append(starts[key][-1] + (got[key].numel() if key in got else 0))
    out = {key: np.concatenate(parts[key]) for key in KEYS}
    out.update({key + "_start": np.asarray(starts[key], dtype=np.int64) for key in KEYS})
    return out


def write_golden(path=GOLDEN):
    np.savez_compressed(path, **record(torch.device("cuda:0")))


@pytest.fixture(scope="module")
def pinned():
    """{case: {output name: flat tensor}}"""
    with np.load(GOLDEN) as z:
        out = {}
        for i, name in enumerate(sorted(CASES)):
            out[name] = {}
            for key in KEYS:
                a, b = int(z[key + "_start"][i]), int(z[key + "_start"][i + 1])
                if b > a:
                    out[name][key] = torch.from_numpy(z[key][a:b])
        return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_register_kernel_computes_what_was_recorded(dev, pinned, name):
    fn, branch = CASES[name]
    got = fn(dev)
    assert sorted(got) == sorted(pinned[name]), branch
    for key, t in got.items():
        assert torch.equal(t.cpu().flatten(), pinned[name][key]), (name, key, branch)


@pytest.mark.gpu
def test_a_terminated_pair_keeps_its_rows(dev):
    """the gated case: pair 1 has reached its bound, so its rows of idx and samples keep the value they were filled with; pair 0
    is sampled (its values are pinned by the golden file above)"""
    got = _gated(dev, 500, 5)
    assert bool((got["idx"][1] == FILL).all()) and bool((got["samples"][1] == float(FILL)).all())
    assert bool((got["idx"][0] != FILL).any()) and int(got["idx"][0].min()) >= 0 and int(got["idx"][0].max()) < 500


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_golden(*sys.argv[1:2])
