"""Golden vectors of the reference's local optimisation (RANSAC(..., lo=1 / 2), ransac.py:122-132, 217-257): runs ONLY where
the reference exists, with the stubs and the noise recorder of gen_golden.py.

For each solver (Nister five-point, 8-point F) one pair of 128 points, B = 16, lo_iters = 8, torch.manual_seed(seed) before
each run: the reference's (model, mask, score, iterations) for lo = 0, 1 and 2 and the longest recorded Gumbel stream (LO
draws no random numbers: the shorter runs' streams are prefixes of it -- asserted).  Pairs / seeds are searched so that
lo = 1 and lo = 2 change the lo = 0 result and the f64 restatement tests/lo_ref.py reproduces the reference's iterations
and masks for all three (asserted; with the reference's adaptive-stop exponent, `sample_size`, stored too).  Re-run:  python tests/golden/gen_golden_lo.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (stubs, sys.path, NoiseRecorder, save)

from estimators.essential_matrix_estimator_nister import EssentialMatrixEstimatorNister  # noqa: E402
from estimators.fundamental_matrix_estimator import FundamentalMatrixEstimatorNew  # noqa: E402
from samplers.gumbel_sampler import GumbelSoftmaxSampler  # noqa: E402
from scorings.msac_score import MSACScore  # noqa: E402
from ransac import RANSAC  # noqa: E402

from differentiable_ransac_amd import synth  # noqa: E402
from tests import lo_ref  # noqa: E402

B, LO_ITERS = 16, 8


def run_ref(name, pair, seed, lo):
    fmat = name == "f8"
    est = FundamentalMatrixEstimatorNew(device="cpu") if fmat else EssentialMatrixEstimatorNister(device="cpu")
    smp = GumbelSoftmaxSampler(B, 8 if fmat else 5, device="cpu", data_type=torch.float32)
    rec = G.NoiseRecorder(smp.gumbel_dist)
    smp.gumbel_dist = rec
    r = RANSAC(est, smp, MSACScore(device="cpu"), fmat=fmat, train=False, ransac_batch_size=B, sampler_id=3 if fmat else 2,
               threshold=0.75, max_iterations=5000, lo=lo, lo_iters=LO_ITERS)
    torch.manual_seed(seed)
    model, mask, score, iters = r(pair["matches"], pair["logits"], pair["K1"], pair["K2"], None)
    return model, mask, float(score), int(iters), rec.draws


def est_sample_size(name):
    """the exponent of the reference's adaptive stop: its estimator's sample_size (7 for the 8-point F estimator)"""
    return (FundamentalMatrixEstimatorNew(device="cpu") if name == "f8" else EssentialMatrixEstimatorNister(device="cpu")).sample_size


def attempt(name, pseed, seed):
    pair = synth.two_view_pair(pseed, 128, inlier_ratio=0.7, pixel=(name == "f8"))
    runs = {lo: run_ref(name, pair, seed, lo) for lo in (0, 1, 2)}
    longest = max(runs.values(), key=lambda r: len(r[4]))[4]
    for r in runs.values():
        assert all(torch.equal(a, b) for a, b in zip(r[4], longest)), "LO consumed random numbers"
    # lo = 1 and lo = 2 must change the lo = 0 result
    base = runs[0]
    for lo in (1, 2):
        if runs[lo][3] == base[3] and torch.equal(runs[lo][1], base[1]):
            return None
    # the f64 restatement must reproduce iterations and masks
    m64 = pair["matches"].double()
    for lo, (model, mask, score, iters, _) in runs.items():
        # (on the longest stream: a run that merely exhausts its own draws would hide a different stop)
        _, mk, sc, it, _ = lo_ref.ransac_test_lo(m64, pair["logits"].double(), [g.double() for g in longest], pair["K1"].double(),
                                                 pair["K2"].double(), name, lo, LO_ITERS, sample_size=est_sample_size(name))
        if it != iters or not torch.equal(mk, mask) or abs(sc - score) > 1e-3 * max(1.0, score):
            return None
    return pair, runs, longest


def main():
    torch.set_num_threads(4)
    plan = {"nister": [(p, s) for p in (10, 12, 13, 14) for s in (63, 64, 65, 66, 67)],
            "f8": [(p, s) for p in (11, 12, 13, 14) for s in (63, 64, 65, 66, 67)]}
    for name, tries in plan.items():
        got = None
        for pseed, seed in tries:
            got = attempt(name, pseed, seed)
            print(name, "pair", pseed, "seed", seed, "ok" if got else "rejected", flush=True)
            if got:
                break
        assert got, f"no pair / seed reproduces the reference's LO run for {name}"
        pair, runs, longest = got
        out = dict(matches=pair["matches"], logits=pair["logits"], K1=pair["K1"], K2=pair["K2"], gumbels=torch.stack(longest),
                   pair_seed=pseed, seed=seed, lo_iters=LO_ITERS, sample_size=est_sample_size(name))
        for lo, (model, mask, score, iters, _) in runs.items():
            out.update({f"model_lo{lo}": model, f"mask_lo{lo}": mask, f"score_lo{lo}": score, f"iterations_lo{lo}": iters})
        G.save(f"ransac_test_lo_{name}", **out)


if __name__ == "__main__":
    main()
