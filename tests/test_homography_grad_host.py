"""Host-side checks of the weighted-DLT gradient references (tests/homography_grad_ref.py) -- that the two agree on every input of
the GPU tests, how far apart they are (the tolerance constant of tests/test_gpu_homography_grad.py), central differences as a third
opinion, the conditioning the tolerance rule asks of the inputs -- and of what the feature adds to the header, the built library and
ops.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from differentiable_ransac_amd import ops
from tests import homography_grad_ref as G
from tests import homography_ref as HR

SYMBOLS = [f"dr_refit_homography_bwd_{s}" for s in ("f32", "f64")]


def test_forward_of_reference_a_is_the_dlt_of_homography_ref():
    """the same rows, the same weights: homography_ref.dlt (by SVD of the stacked system) against the eigh-based forward that is
    differentiated; the two differ by the conditioning of the smallest singular vector, far below 1e-9"""
    for key in [(5, 1, True, False), (257, 3, True, True), (1000, 3, False, True)]:
        cs, ref = G.cached_case(*key)
        for p in range(key[1]):
            _, xs, ws = G.selected(cs, p)
            H = G.torch_fit(torch.tensor(xs), None if ws is None else torch.tensor(ws)).numpy()
            d = HR.dlt(xs, ws)
            assert d["valid"] and np.abs(H - d["model"]).max() <= 1e-9


def test_the_two_references_agree_and_the_tolerance_constant():
    """(a) against (b) on every f64 input of the GPU tests; c is printed (docs/LOG.md records it)"""
    units = G.input_units()
    assert len(units) >= 60
    kap = np.array([k for _, _, k, _ in units])
    worst = max(units, key=lambda r: r[3])
    c = G.tolerance_constant()
    print(f"kappa over the inputs: {kap.min():.3g} .. {kap.max():.3g}; largest (a)-(b) distance {worst[3]:.3g} units of eps64 kappa mag "
          f"at case {worst[0]} pair {worst[1]}; tolerance constant c = {c:.4g}")
    assert 10.0 <= c < 1e4
    for key, p, k, u in units:
        assert u <= 0.1 * c + 1e-9


def test_input_conditioning_and_the_f32_condition():
    """no more than 1 % of a case above KAPPA_MAX -- with at most three pairs a case: none -- under the references alone, in the
    f32-rounded inputs too; and c eps64 kappa <= eps32 on everything compared in f32"""
    c = G.tolerance_constant()
    assert c * G.EPS64 * G.KAPPA_MAX <= G.EPS32
    for key in G.PAIR_CASES:
        for dt in ("float64", "float32"):
            cs, ref = G.cached_case(*key, dt)
            fitted = ref["rows"] >= 4
            over = (ref["kappa"][fitted] > G.KAPPA_MAX).sum()
            assert over <= 0.01 * key[1], (key, dt)
            assert (c * G.EPS64 * ref["kappa"][fitted] <= G.EPS32).all()
            # (the masked N = 4, 5 cases keep fewer than four rows: their defined result is zeros)
            assert fitted.all() or (key[0] <= 5 and key[3])


def test_reference_gradient_against_finite_differences():
    """neither reference is trusted on the other's word alone: central differences of L = <gH, H> through reference (a)'s forward
    on a handful of rows and weights.  Step 1e-4 (pixels, and weights of order 1): the truncation error is of relative order
    step^2, the rounding error eps64 kappa / step ~ 1e-10, so 1e-6 of the gradient's largest entry bounds both"""
    cs, ref = G.cached_case(257, 3, True, True)
    sel, xs, ws = G.selected(cs, 1)
    gH = cs["gH"][1]
    ax, aw = G.autograd(xs, ws, gH)

    def loss(xx, ww):
        with torch.no_grad():
            return float((G.torch_fit(torch.tensor(xx), torch.tensor(ww)).numpy() * gH).sum())
    step = 1e-4
    for n, d in ((0, 0), (7, 1), (60, 2), (len(xs) - 1, 3)):
        e = np.zeros_like(xs)
        e[n, d] = step
        assert abs((loss(xs + e, ws) - loss(xs - e, ws)) / (2 * step) - ax[n, d]) <= 1e-6 * np.abs(ax).max()
    for n in (1, 33, len(xs) - 2):
        e = np.zeros_like(ws)
        e[n] = step
        assert abs((loss(xs, ws + e) - loss(xs, ws - e)) / (2 * step) - aw[n]) <= 1e-6 * np.abs(aw).max()


def test_exact_correspondences_have_a_zero_weight_gradient_in_the_references():
    """N = 4 exact: a . h = b . h = 0 for every row, so dL/dw vanishes within the counted magnitude"""
    cs = G.exact_case()
    x, gH = cs["x"][0], cs["gH"][0]
    _, aw = G.autograd(x, None, gH)
    _, bw = G.closed_form(x, None, gH)
    tol = G.tolerance_constant() * G.EPS64 * G.kappa(x) * G.weight_grad_magnitude(x, None, gH)
    assert np.abs(aw).max() <= tol and np.abs(bw).max() <= tol
    assert G.kappa(x) <= G.KAPPA_MAX


def test_header_declares_and_library_exports_the_entries():
    declared = L.entries()
    ptr = L.c_pointer
    for s in SYMBOLS:
        # (matches, mask, weights, grad_model, P, N, grad_matches, grad_weights, stream)
        assert declared[s] == [ptr, ptr, ptr, ptr, ctypes.c_int, ctypes.c_int, ptr, ptr, ptr]
        assert hasattr(L.lib(), s)


def test_entries_refuse_bad_arguments_without_a_gpu():
    lib = L.lib()
    buf = (ctypes.c_char * 64)()
    for s in SYMBOLS:
        fn = getattr(lib, s)
        assert fn(None, None, None, None, 0, 0, None, None, None) == -1 and s.encode() in lib.dr_last_error()
        assert fn(None, None, None, buf, 1, 4, buf, buf, None) == -1 and b"null" in lib.dr_last_error()      # matches
        assert fn(buf, None, None, None, 1, 4, buf, buf, None) == -1                                          # grad_model
        assert fn(buf, None, None, buf, 1, 4, None, None, None) == -1 and b"nothing to write" in lib.dr_last_error()
        assert fn(buf, None, None, buf, 0, 4, buf, None, None) == -1
        assert fn(buf, None, None, buf, 1, 0, None, buf, None) == -1


def test_weighted_homography_refuses_cpu_tensors_and_wrong_shapes():
    m = torch.zeros(2, 8, 4)
    with pytest.raises(L.DransacError, match="GPU tensors only"):
        ops.weighted_homography(m)
    with pytest.raises(L.DransacError, match="GPU tensors only"):
        ops.weighted_homography(m.double(), torch.ones(2, 8, dtype=torch.float64), torch.ones(2, 8, dtype=torch.bool))
    with pytest.raises(L.DransacError, match="matches"):
        ops.weighted_homography(torch.zeros(2, 8, 6))
    with pytest.raises(L.DransacError, match="matches"):
        ops.weighted_homography(torch.zeros(8, 4))
    with pytest.raises(L.DransacError, match="matches"):
        ops.weighted_homography(torch.zeros(2, 8, 4, dtype=torch.float16))
    with pytest.raises(L.DransacError, match="weights"):
        ops.weighted_homography(m, torch.ones(2, 7))
    with pytest.raises(L.DransacError, match="weights"):
        ops.weighted_homography(m, torch.ones(2, 8, dtype=torch.int32))
    with pytest.raises(L.DransacError, match="mask"):
        ops.weighted_homography(m, None, torch.ones(2, 9, dtype=torch.bool))
    with pytest.raises(L.DransacError, match="mask"):
        ops.weighted_homography(m, None, torch.ones(2, 8))
