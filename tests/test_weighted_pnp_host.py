"""The differentiable weighted PnP fit without a GPU: the reference tests/weighted_pnp_ref.py against central differences of its own
converged solution, what the GPU tests rely on (scenes within the exclusion cap, the full Hessian and J^T J apart by more than the
tolerance, the DLT start reaching the optimum), the ABI of the new entries and the refusals of the wrappers before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from tests import pnp_ref as R
from tests import weighted_pnp_ref as W

FD_H = 1e-6
FD_BOUND = 1e-6      # relative to the largest entry of the derivative: truncation h^2 L''' / 6 and rounding eps |L| / h ~ 1e-10 both lie below


def _value(m, w, init, G):
    T = W.minimiser(m, w, None, init)[0]
    return float(np.sum(G[:3] * T[:3]))


@pytest.mark.parametrize("N", [4, 7])
def test_ift_gradient_against_central_differences_of_the_converged_solution(N):
    cs = W.case(1, N)
    m, w, init = cs["m"][0], cs["w"][0], cs["start"][0]
    G = np.random.default_rng(N).normal(size=(4, 4))
    T, ok, rows, _ = W.minimiser(m, w, None, init)
    assert ok and rows.all()
    gm, gw, cond, _ = W.ift(m, w, rows, T, G)
    fd_m, fd_w = np.zeros_like(gm), np.zeros_like(gw)
    for i in range(N):
        for d in range(5):
            mp, mn = m.copy(), m.copy()
            mp[i, d] += FD_H
            mn[i, d] -= FD_H
            fd_m[i, d] = (_value(mp, w, T, G) - _value(mn, w, T, G)) / (2 * FD_H)
        wp, wn = w.copy(), w.copy()
        wp[i] += FD_H
        wn[i] -= FD_H
        fd_w[i] = (_value(m, wp, T, G) - _value(m, wn, T, G)) / (2 * FD_H)
    em, ew = np.abs(gm - fd_m).max() / np.abs(fd_m).max(), np.abs(gw - fd_w).max() / np.abs(fd_w).max()
    print(f"N = {N}: cond(H) {cond:.3g}, IFT against central differences: rows {em:.3g}, weights {ew:.3g} (bound {FD_BOUND:g})")
    assert em <= FD_BOUND and ew <= FD_BOUND
    # the Gauss-Newton Hessian gives another answer at this noise: the differences tell the two apart
    gm_gn, gw_gn, _, _ = W.ift(m, w, rows, T, G, gauss_newton=True)
    assert np.abs(gm_gn - fd_m).max() / np.abs(fd_m).max() > 100 * FD_BOUND


def test_the_scenes_of_the_gpu_tests_stay_within_the_exclusion_cap_and_separate_the_two_hessians():
    """per shape: at most EXCLUDED_MAX of the pairs above COND_MAX, and on N >= 7 the gradients under J^T J differ from the true ones
    by more than the tolerance the GPU test allows (8 x the case's float32 figures: the larger of the two types')"""
    for P, N in W.SHAPES:
        cs = W.case(P, N)
        left_out, pairs, fm, fw = 0, [], 0.0, 0.0
        for p in range(P):
            G = np.random.default_rng(100 + p).normal(size=(4, 4))
            a, m_, w_ = W.backward_figures(cs["m"][p], cs["w"][p], None, cs["start"][p], G, "float32")
            assert a["valid"]
            fm, fw = max(fm, m_), max(fw, w_)
            if a["cond"] > W.COND_MAX:
                left_out += 1
            elif N >= 7:
                pairs.append((a, W.solve_and_grad(cs["m"][p], cs["w"][p], None, a["T"], G, gauss_newton=True, iters=10)))
        for a, gn in pairs:
            assert W.deviation(gn["gm"], a["gm"]) > W.TOL_FACTOR * fm and W.deviation(gn["gw"], a["gw"]) > W.TOL_FACTOR * fw, (P, N)
        assert left_out <= W.EXCLUDED_MAX * P, (P, N, left_out)


def test_lm_from_the_dlt_start_reaches_what_lm_reaches_from_the_truth():
    """at ITERS passes, to a few of the reference's own convergence figures (its run at twice the passes, its run on moved inputs);
    the GPU test takes this difference into its figure"""
    for P, N in W.SHAPES:
        if N < 6:
            continue
        cs = W.case(P, N)
        for p in range(P):
            m, w = cs["m"][p], cs["w"][p]
            start, ok = W.dlt(m, w)
            assert ok, (N, p)
            Tg, fig = W.forward_figures(m, w, None, cs["gt"][p], "float64")
            a, oka = W.lm(m, w, None, start, W.ITERS)
            assert oka and W.deviation(a, Tg) <= max(W.TOL_FACTOR * fig, 1e-8), (N, p, W.deviation(a, Tg), fig)


def test_dlt_recovers_an_exact_pose_and_refuses_planes_and_short_sets():
    sc = R.scene(3, 12, 1.0, 0.0)
    T, ok = W.dlt(sc["matches"])
    assert ok and np.abs(T - sc["pose"]).max() < 1e-10
    assert not W.dlt(W.coplanar_case(12))[1]
    assert not W.dlt(sc["matches"][:5])[1]
    assert not W.dlt(sc["matches"], None, np.zeros(12, bool))[1]


SIGNATURES = {
    "dr_refit_pnp_weighted": "pppp" + "iii" + "ppp",       # matches, mask, weights, init_model, P, N, iters, model, valid, stream
    "dr_refit_pnp_bwd": "ppppp" + "ii" + "ppp",            # matches, mask, weights, model, grad_model, P, N, grad_matches, grad_weights, stream
    "dr_pnp_dlt": "ppp" + "ii" + "ppp",                    # matches, mask, weights, P, N, model, valid, stream
    "dr_refit_pnp": "ppp" + "iii" + "ppp",                 # (unchanged)
}


def test_header_declares_the_entries_with_the_stated_signatures_and_the_library_refuses_nulls():
    kinds = {"p": L.c_pointer, "i": ctypes.c_int}
    lib = L.lib()
    for name, sig in SIGNATURES.items():
        for sfx in ("f32", "f64"):
            full = f"{name}_{sfx}"
            assert L.entries()[full] == [kinds[k] for k in sig], full
            assert hasattr(lib, full)
            assert getattr(lib, full)(*[None if k == "p" else 0 for k in sig]) == -1 and lib.dr_last_error().startswith(full.encode())
    buf = (ctypes.c_char * 256)()
    assert lib.dr_refit_pnp_bwd_f32(buf, None, None, buf, buf, 1, 8, None, None, None) == -1 and b"no gradient" in lib.dr_last_error()
    assert lib.dr_refit_pnp_weighted_f64(buf, None, buf, buf, 1, 8, -1, buf, buf, None) == -1 and b"iters" in lib.dr_last_error()


def test_wrappers_refuse_before_any_launch(monkeypatch):
    from differentiable_ransac_amd import ops
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    m = torch.rand(2, 8, 5)
    for fn in (ops.weighted_pnp, ops.pnp_dlt):
        with pytest.raises(L.DransacError, match="GPU tensors"):
            fn(m)
        with pytest.raises(L.DransacError, match=r"\[P,N,5\]"):
            fn(torch.zeros(2, 8, 4))
        with pytest.raises(L.DransacError, match=r"\[P,N,5\]"):
            fn(torch.zeros(8, 5))
        with pytest.raises(L.DransacError, match="float32 or float64"):
            fn(torch.zeros(2, 8, 5, dtype=torch.float16))
        with pytest.raises(L.DransacError, match="weights"):
            fn(m, torch.ones(2, 7))
        with pytest.raises(L.DransacError, match="weights"):
            fn(m, torch.ones(2, 8, dtype=torch.int32))
        with pytest.raises(L.DransacError, match="mask"):
            fn(m, None, mask=torch.ones(2, 9, dtype=torch.bool))
        with pytest.raises(L.DransacError, match="mask"):
            fn(m, None, mask=torch.ones(2, 8))
    with pytest.raises(L.DransacError, match="init_model"):
        ops.weighted_pnp(m, None, torch.eye(4).repeat(3, 1, 1))
    with pytest.raises(L.DransacError, match="init_model"):
        ops.weighted_pnp(m, None, torch.eye(4, dtype=torch.float64).repeat(2, 1, 1))
    assert calls == []
