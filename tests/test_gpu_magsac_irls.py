"""dr_magsac_irls against the f64 oracle tests/magsac_ref.py::irls: F and E, f32 and f64, P = 4 pairs of N = 8 / 64 / 300 rows, the
default threshold and four times it, 1 and 10 steps, from models gt + sigma randn.

Where every oracle margin (a candidate's lead over the current score, and for E over the runner-up candidate) exceeds the score
tolerance, the fit count equals the oracle's and the final model the oracle's up to sign and scale within the refit tests' bound
(F: refit_ref.f_tolerance of the last weighted fit; E: test_gpu_refit's E_TOL); at most a quarter of the cases may lie outside that
rule.  For every case: the final score is the oracle score of the final model within tolerance, it never drops, irls_fits <=
irls_iters, a pair with fewer than 8 (F) / 5 (E) points inside the cutoff comes back untouched, mask and inlier count keep their bytes."""
import pytest
import torch

from oracle import cpu_ref as O
from tests import magsac_ref as G
from tests import refit_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
E_TOL = {torch.float64: 1e-6, torch.float32: 1e-4}     # test_gpu_refit.E_TOL


def _model_distance(fundamental, model, ref, mt, thr, dtype):
    """(distance, bound) of the device's final model to the oracle's"""
    if not fundamental:
        return float((O.canonical(model.double()) - O.canonical(ref)).abs().max()), E_TOL[dtype]
    s = G._ratio(mt, ref, thr)
    live = torch.isfinite(s) & (s < 1.0)
    w = torch.where(live, G.weight(torch.where(live, s, torch.zeros_like(s))), torch.zeros_like(s))
    cond = RR.f_refit_forms(mt, None, torch.sqrt(w))["cond"]
    return RR.rel_err(model, ref), RR.f_tolerance(cond, dtype)


@pytest.mark.parametrize("N", G.IRLS_N)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("fundamental", [True, False], ids=["F", "E"])
def test_irls_matches_the_oracle(fundamental, dtype, N):
    from differentiable_ransac_amd import ops
    P = G.IRLS_P
    mt64, md64 = G.irls_inputs(N, fundamental)
    mt_h, md_h = mt64.to(dtype), md64.to(dtype)          # the oracle sees the values the kernel sees
    mt, md = mt_h.to(DEV), md_h.to(DEV)
    kmin = 8 if fundamental else 5
    cases, outside, report = 0, 0, []
    for thr in G.IRLS_THR:
        thr_t = torch.full((P,), thr, dtype=dtype, device=DEV)
        start, inl0 = ops.magsac_score(mt, md[:, None].contiguous(), thr_t, want_inliers=True)
        for iters in G.IRLS_ITERS:
            st = ops.RansacState(P, N, 1000, DEV, dtype)
            st.best_model.copy_(md)
            st.best_score.copy_(start[:, 0])
            mask0 = (torch.arange(P * N, device=DEV).view(P, N) % 3 == 0)
            st.best_mask.copy_(mask0)
            st.best_inliers.fill_(12345)
            st.iters.fill_(77)
            fits = torch.zeros(P, dtype=torch.int32, device=DEV)
            ws = torch.empty(P, N, dtype=dtype, device=DEV)
            ops.magsac_irls(st, mt, thr_t, fundamental, iters, fits, ws)
            torch.cuda.synchronize()
            assert torch.equal(st.best_mask, mask0) and (st.best_inliers == 12345).all() and (st.iters == 77).all()
            assert (st.max_iters == 1000.0).all()
            for p in range(P):
                cases += 1
                m64, s0 = mt_h[p].double(), float(start[p, 0])
                model, score, nfit = st.best_model[p].cpu(), float(st.best_score[p]), int(fits[p])
                ref_score, _ = G.magsac(m64, model.double(), float(thr_t[p]))
                tol = G.score_tolerance(mt_h[p], model, float(thr_t[p]), dtype)
                assert 0 <= nfit <= iters
                assert score >= s0, "the score dropped"
                assert abs(score - ref_score) <= tol, (score, ref_score, tol)
                if int(inl0[p, 0]) < kmin:
                    assert nfit == 0
                if nfit == 0 or score == s0:
                    assert torch.equal(model, md_h[p]) and score == s0, "no step taken: the state must be untouched"
                o_model, o_score, o_fits, margins = G.irls(m64, md_h[p].double(), float(thr_t[p]), iters, fundamental, score=s0, dtype=dtype)
                dist, bound = float("nan"), float("nan")
                if not margins:                          # no fit gave a candidate: nothing for a rounding to decide
                    ok = nfit == o_fits and torch.equal(model, md_h[p])
                elif min(margins) > tol:
                    dist, bound = _model_distance(fundamental, model, o_model, m64, float(thr_t[p]), dtype)
                    ok = nfit == o_fits and dist <= bound
                else:
                    ok = None                            # a margin within the tolerance: outside the rule
                report.append((thr, iters, p, nfit, o_fits, dist, bound, ok))
                outside += ok is None
    for r in report:
        print("thr %.3g iters %d pair %d: fits %d (oracle %d) model distance %.3g bound %.3g rule %s" % r)
    print(f"{cases} cases, {outside} outside the strict rule")
    bad = [r for r in report if r[-1] is False]
    assert not bad, f"inside the rule, yet another fit count or model: {bad}"
    assert outside <= cases // 4, f"{outside} of {cases} cases outside the fit-count / model rule"


@pytest.mark.parametrize("fundamental,N", [(True, 7), (False, 4), (True, 1)], ids=["F7", "E4", "F1"])
def test_too_few_points_is_a_polish_that_does_nothing(fundamental, N):
    """below 8 (F) / 5 (E) points no fit can run: the entry accepts the call and the state comes back as it was"""
    from differentiable_ransac_amd import ops
    P = 2
    mt = G.irls_inputs(8, fundamental)[0][:P, :N].float().contiguous().to(DEV)
    st = ops.RansacState(P, N, 100, DEV, torch.float32)
    st.best_score.fill_(0.25)
    model0, fits = st.best_model.clone(), torch.zeros(P, dtype=torch.int32, device=DEV)
    ops.magsac_irls(st, mt, torch.full((P,), 1e3, device=DEV), fundamental, 10, fits, torch.empty(P, N, device=DEV))
    torch.cuda.synchronize()
    assert int(fits.sum()) == 0 and torch.equal(st.best_model, model0) and bool((st.best_score == 0.25).all())
