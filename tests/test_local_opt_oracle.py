"""The f64 restatement of local optimisation (tests/lo_ref.py) against the reference's own lo = 0 / 1 / 2 runs
(ransac_test_lo_{nister,f8}.npz, tests/golden/gen_golden_lo.py), and its lo = 0 path against the oracle's test-mode loop."""
import pytest
import torch

from oracle import cpu_ref as O
from tests import lo_ref
from tests.conftest import load_golden


def _args(g, dt=torch.float64):
    return (g["matches"].to(dt), g["logits"].to(dt), [x.to(dt) for x in g["gumbels"]], g["K1"].to(dt), g["K2"].to(dt))


@pytest.mark.parametrize("name", ["nister", "f8"])
@pytest.mark.parametrize("lo", [0, 1, 2])
def test_restatement_reproduces_reference_lo_run(name, lo):
    g = load_golden(f"ransac_test_lo_{name}")
    # (sample_size: the reference's adaptive stop takes its estimator's sample_size, 7 for the 8-point F estimator)
    model, mask, score, iters, refits = lo_ref.ransac_test_lo(*_args(g), name, lo, int(g["lo_iters"]),
                                                              sample_size=int(g["sample_size"]))
    assert iters == g[f"iterations_lo{lo}"]
    assert torch.equal(mask, g[f"mask_lo{lo}"])
    ref = g[f"score_lo{lo}"]
    assert abs(score - ref) <= 1e-3 * max(1.0, ref), (score, ref)
    assert (refits > 0) == (lo > 0)


@pytest.mark.parametrize("name", ["nister", "f8"])
def test_fixture_lo_changes_the_result(name):
    g = load_golden(f"ransac_test_lo_{name}")
    for lo in (1, 2):
        assert (g[f"iterations_lo{lo}"] != g["iterations_lo0"]) or not torch.equal(g[f"mask_lo{lo}"], g["mask_lo0"])
    assert g["score_lo2"] >= g["score_lo0"]


@pytest.mark.parametrize("name", ["nister", "f8"])
def test_restatement_lo0_is_the_oracle_loop(name):
    g = load_golden(f"ransac_test_lo_{name}")
    m0, k0, s0, i0, r0 = lo_ref.ransac_test_lo(*_args(g), name, 0)
    m1, k1, s1, i1 = O.ransac_test(*_args(g), name)
    assert r0 == 0 and i0 == i1 and torch.equal(k0, k1) and s0 == s1 and torch.equal(m0, m1)
