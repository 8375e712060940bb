"""Host checks of the two-view MAGSAC++ oracle (tests/magsac_ref.py) and of the driver's refusals: no GPU."""
import pytest
import torch

from tests import magsac_ref as G
from tests import msac_ref as R


def test_closed_form_agrees_with_the_gamma_function_oracle():
    s = torch.linspace(0.0, 1.0, 100001, dtype=torch.float64)
    gain, w = G.closed_form(s)
    inside = s < 1.0
    assert float((gain - (1.0 - G.loss(s)))[inside].abs().max()) <= 1e-13
    assert float((w - G.weight(s))[inside].abs().max()) <= 1e-13
    assert abs(float(gain[-1])) <= 1e-13 and abs(float(w[-1])) <= 1e-13           # the closed form is continuous into the cutoff
    assert float(G.loss(0.0)) == 0.0 and float(G.loss(1.0)) == 1.0 and float(G.weight(0.0)) == 1.0 and float(G.weight(1.0)) == 0.0
    assert abs(G.K2 - 13.276704135987622) < 1e-14 and abs(G.GK - 0.0036112606177586) < 1e-15
    assert abs(G.RHO1 - 1.3015316073311318) < 1e-15 and abs(G.L - 4.50170667458135) < 1e-13
    g = 1.0 - G.loss(s)
    assert bool((g[1:] <= g[:-1]).all()) and float(g[0]) == 1.0 and float(g[-1]) == 0.0
    slope = (g[:-1] - g[1:]) / (s[1:] - s[:-1])
    assert float(slope.max()) <= G.L * (1 + 1e-9) and float(slope[0]) > 0.99 * G.L
    # d rho / du = Gamma(3/2, u) - Gamma_k
    u = torch.linspace(0.05, G.UK - 0.05, 2001, dtype=torch.float64)
    h = 1e-5
    rho = lambda v: G.loss(v / G.UK) * G.RHO1
    num = (rho(u + h) - rho(u - h)) / (2 * h)
    assert float((num - G.weight(u / G.UK) * (G.G0 - G.GK)).abs().max()) <= 1e-8


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_term_error_ceiling(dtype):
    s = torch.linspace(0.0, 1.0, 100001, dtype=torch.float64)[:-1]
    worst = float(G.term_error_bound(s, dtype).max())
    print(f"{dtype}: first-order error of a term, worst {worst:.2f} unit roundoffs; ceiling {G.E_TERM_UNITS[dtype]}")
    assert worst <= G.E_TERM_UNITS[dtype] <= 1.25 * worst


def test_dispatch_reaches_every_launch_path():
    seen = {G.dispatch(p, m, n, dt) for p, m, n, dt in G.score_shapes()}
    assert seen == G.intended_paths()
    assert {G.dispatch(p, m, n, dt) for p, m, n, dt in G.score_shapes() if dt == torch.float64} >= {("wave1", 1), ("block", 2)}


def test_reference_alone_meets_the_caps_on_the_gpu_inputs():
    """per M-prefix and per validity pattern, as the GPU tests apply them"""
    bad = []
    for c in G.gpu_cases():
        _, _, refs, valid = G.case_inputs(c)
        ex, inl, slots = G.reference_cap(refs, c["M"], c["P"], valid)
        if not G.within_caps(ex, inl, slots * c["N"]):
            bad.append((c["P"], c["M"], c["N"], c["dtype"], c["thr"], c["pattern"], ex, inl, slots * c["N"]))
    assert not bad, bad


@pytest.mark.parametrize("fundamental", [True, False], ids=["F", "E"])
def test_the_irls_scenes_keep_three_quarters_of_the_cases_inside_the_rule(fundamental):
    for N in G.IRLS_N:
        for dtype in (torch.float32, torch.float64):
            out = G.irls_outside(N, fundamental, dtype)
            print(f"{'F' if fundamental else 'E'} N={N} {dtype}: {out} of 16 cases outside the rule by the oracle alone")
            assert out <= 3        # (4 are allowed on the device, whose final model's tolerance may differ in the last digits)


def test_the_update_case_is_decided_by_the_reference():
    P, M, N = G.K6_SHAPE
    _, _, refs = G.case_refs(P, N, G.K6_SEED, torch.float32, True, R.THR, M)
    decided = 0
    for r in refs:
        sc = r["scores"].clone()
        sc[r["nan"]] = -float("inf")
        top = torch.argsort(sc, descending=True, stable=True)
        a, b = int(top[0]), int(top[1])
        decided += float(sc[a] - sc[b]) > 2 * float(max(r["tol"][a], r["tol"][b]))
    assert decided >= 0.9 * P


@pytest.mark.parametrize("kw,word", [(dict(train=True), "train"), (dict(lo=1), "lo"), (dict(weighted=1), "weighted"),
                                     (dict(keep_masks=True), "keep_masks")])
def test_constructor_refusals(kw, word):
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    with pytest.raises(ValueError, match=word):
        BatchedRANSAC("nister", scoring="magsac", **kw)


def test_constructor_refuses_unknown_scoring_and_negative_steps():
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    with pytest.raises(ValueError, match="scoring"):
        BatchedRANSAC("nister", scoring="ransac")
    with pytest.raises(ValueError, match="irls_iters"):
        BatchedRANSAC("f8", scoring="magsac", irls_iters=-1)
    d = BatchedRANSAC("f8", scoring="magsac", irls_iters=0)
    assert d.scoring == "magsac" and d.irls_iters == 0 and BatchedRANSAC("f8").scoring == "msac"
