"""Host-side checks of the weighted eight-point gradient references (tests/fundamental_grad_ref.py) -- that the two agree on every input
of the GPU tests, how far apart they are (the tolerance constant of tests/test_gpu_fundamental_grad.py), central differences as a third
opinion, the conditioning cap the tolerance rule asks of the inputs -- and of what the feature adds to the header, the built library
and ops: the family record, the wrapper's checks, and the entries a forward and a backward issue.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from differentiable_ransac_amd import ops
from tests import fundamental_grad_ref as G
from tests import refit_ref as RR

SYMBOLS = [f"dr_refit_fundamental_bwd_{s}" for s in ("f32", "f64")]


def test_forward_of_reference_a_is_the_refit_of_refit_ref():
    """the same rows, the same weights: refit_ref.f_refit (Hartley + SVD of the design matrix, written from the oracle) against the
    eigh-based forward that is differentiated, up to the sign; the two differ by the conditioning of the null vector (f_tolerance)"""
    for key in [(8, 1, False, False), (257, 3, True, True), (1000, 3, True, False)]:
        cs, ref = G.cached_case(*key)
        for p in range(key[1]):
            m, k = torch.tensor(cs["x"][p]), None if cs["mask"] is None else torch.tensor(cs["mask"][p])
            F, valid, cond, _ = RR.f_refit(m, k, None if cs["w"] is None else torch.tensor(cs["w"][p]))
            assert valid and RR.rel_err(torch.tensor(ref["F"][p]), F) <= RR.f_tolerance(cond, torch.float64)


def test_the_two_references_agree_and_the_tolerance_constant():
    """(a) against (b) on every f64 input of the GPU tests; the figure and c are printed (docs/LOG.md records them)"""
    units = G.input_units()
    assert len(units) == sum(k[1] for k in G.PAIR_CASES) == 16
    kap = np.array([k for _, _, k, _ in units])
    worst = max(units, key=lambda r: r[3])
    c = G.tolerance_constant()
    print(f"kappa over the inputs: {kap.min():.3g} .. {kap.max():.3g}; largest (a)-(b) distance {worst[3]:.3g} units of eps64 kappa mag "
          f"at case {worst[0]} pair {worst[1]}; recorded {G.MEASURED_UNITS}; tolerance constant c = {c:.4g}")
    # the recorded figure is the measured one, rounded up: never below it, and not a loose guess above it
    assert 0.9 * G.MEASURED_UNITS <= worst[3] <= G.MEASURED_UNITS
    assert c == G.MARGIN * max(1.0, G.MEASURED_UNITS) and G.MARGIN == 8.0


def test_no_pair_of_the_cases_is_exempt_and_the_f32_condition():
    """kappa <= KAPPA_MAX on EVERY pair of every case, under the references alone, in the f32-rounded inputs too; every pair has its
    eight rows; c eps64 KAPPA_MAX <= eps32, so everything compared in f32 is compared at kappa_eff = 1"""
    assert G.tolerance_constant() * G.EPS64 * G.KAPPA_MAX <= G.EPS32
    for key in G.PAIR_CASES:
        for dt in ("float64", "float32"):
            cs, ref = G.cached_case(*key, dt)
            assert (ref["rows"] >= 8).all(), (key, dt)
            assert (ref["kappa"] <= G.KAPPA_MAX).all(), (key, dt, ref["kappa"])
            assert all(G.tolerances(ref, p, dt) is not None for p in range(key[1]))


def test_the_scenes_are_what_the_cases_claim():
    """depth, at least half inliers, pixel-scale noise, and outliers weighted below 1"""
    for key in G.PAIR_CASES:
        cs, _ = G.cached_case(*key)
        N, P, weighted, _ = key
        assert cs["inliers"].mean(1).min() >= 0.5
        assert (cs["inliers"].all()) == (N < G.ALL_INLIERS_BELOW)
        if weighted:
            assert (cs["w"][~cs["inliers"]] < 0.25).all() and (cs["w"][cs["inliers"]] >= 0.5).all() and (cs["w"] < 1.0).all()
        assert 100.0 < np.abs(cs["x"]).max() < 2000.0      # pixels
    # pixel-scale noise: the inliers' Sampson distance to the scene's own F is of the order of a pixel, the outliers' far above
    cs, _ = G.cached_case(1000, 3, True, False)
    for p in range(3):
        F, x = G.scene(p, 1000)["gt_F"], cs["x"][p]
        p1, p2 = np.concatenate([x[:, :2], np.ones((1000, 1))], 1), np.concatenate([x[:, 2:], np.ones((1000, 1))], 1)
        l2, l1 = p1 @ F.T, p2 @ F
        d = np.abs((p2 * l2).sum(1)) / np.sqrt(l2[:, 0] ** 2 + l2[:, 1] ** 2 + l1[:, 0] ** 2 + l1[:, 1] ** 2)
        assert 0.2 < np.median(d[cs["inliers"][p]]) < 3.0 and np.median(d[~cs["inliers"][p]]) > 20.0


def test_reference_gradient_against_finite_differences():
    """neither reference is trusted on the other's word alone: central differences of L = <gF, F> through reference (a)'s forward
    on a handful of rows and weights.  Step 1e-4 (pixels, and weights of order 1): the truncation error is of relative order
    step^2, the rounding error eps64 kappa / step ~ 1e-9, so 1e-6 of the gradient's largest entry bounds both"""
    cs, ref = G.cached_case(257, 3, True, True)
    sel, xs, ws = G.selected(cs, 1)
    gF, F0 = cs["gF"][1], ref["F"][1]
    ax, aw = ref["gx"][1, sel], ref["gw"][1, sel]

    def loss(xx, ww):
        with torch.no_grad():
            return float((G.torch_fit(torch.tensor(xx), torch.tensor(ww), F0).numpy() * gF).sum())
    step = 1e-4
    for n, d in ((0, 0), (7, 1), (60, 2), (len(xs) - 1, 3)):
        e = np.zeros_like(xs)
        e[n, d] = step
        assert abs((loss(xs + e, ws) - loss(xs - e, ws)) / (2 * step) - ax[n, d]) <= 1e-6 * np.abs(ax).max()
    for n in (1, 33, len(xs) - 2):
        e = np.zeros_like(ws)
        e[n] = step
        assert abs((loss(xs, ws + e) - loss(xs, ws - e)) / (2 * step) - aw[n]) <= 1e-6 * np.abs(aw).max()


def test_the_sign_of_the_forward_negates_the_references():
    cs, ref = G.cached_case(9, 3, True, False)
    x, w, gF, F = cs["x"][0], cs["w"][0], cs["gF"][0], ref["F"][0]
    ax, aw, Fa = G.autograd(x, w, gF, -F)
    bx, bw = G.closed_form(x, w, gF, -F)
    assert np.array_equal(Fa, -F) and np.array_equal(ax, -ref["gx"][0]) and np.array_equal(aw, -ref["gw"][0])
    px, pw = G.closed_form(x, w, gF, F)
    assert np.array_equal(bx, -px) and np.array_equal(bw, -pw)
    assert list(G.forward_signs(ref, -ref["F"])) == [-1.0] * 3 and list(G.forward_signs(ref, 3.0 * ref["F"])) == [1.0] * 3


def test_exact_correspondences_have_a_zero_weight_gradient_in_the_references():
    """exact rows: rho_n . fh = 0 for every row, so dL/dw vanishes within the counted magnitude"""
    cs = G.exact_case()
    x, gF = cs["x"][0], cs["gF"][0]
    _, aw, F = G.autograd(x, None, gF)
    _, bw = G.closed_form(x, None, gF, F)
    tol = G.tolerance_constant() * G.EPS64 * G.kappa(x) * G.weight_grad_magnitude(x, None, gF)
    assert np.abs(aw).max() <= tol and np.abs(bw).max() <= tol
    assert G.kappa(x) <= G.KAPPA_MAX
    assert np.array_equal(G.exact_case(np.float32)["x"], cs["x"])      # (exact in f32)


# ------------------------------------------------------------------------------------------------ header, library, ops
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
        assert fn(None, None, None, buf, 1, 8, buf, buf, None) == -1 and b"null" in lib.dr_last_error()      # matches
        assert fn(buf, None, None, None, 1, 8, buf, buf, None) == -1                                          # grad_model
        assert fn(buf, None, None, buf, 1, 8, None, None, None) == -1 and b"nothing to write" in lib.dr_last_error()
        assert fn(buf, None, None, buf, 0, 8, buf, None, None) == -1
        assert fn(buf, None, None, buf, 1, 0, None, buf, None) == -1


def test_the_family_record():
    fam = ops._FUNDAMENTAL
    assert (fam.refit, fam.shape, fam.width, fam.once) == ("refit_fundamental", (3, 3), 4, True)
    assert fam.shape_text == "matches [P,N,4] = (x1, y1, x2, y2)"
    assert fam.entry is None and fam.points is None and fam.gt_noun is None      # (unused by _WeightedFit)
    for sfx in ("f32", "f64"):
        assert f"dr_{fam.refit}_{sfx}" in L.entries() and f"dr_{fam.refit}_bwd_{sfx}" in L.entries()


def test_weighted_fundamental_refuses_cpu_tensors_and_wrong_shapes(monkeypatch):
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    m = torch.zeros(2, 8, 4)
    with pytest.raises(L.DransacError, match="GPU tensors only"):
        ops.weighted_fundamental(m)
    with pytest.raises(L.DransacError, match="GPU tensors only"):
        ops.weighted_fundamental(m.double(), torch.ones(2, 8, dtype=torch.float64), torch.ones(2, 8, dtype=torch.bool))
    with pytest.raises(L.DransacError, match=r"matches \[P,N,4\] = \(x1, y1, x2, y2\)"):
        ops.weighted_fundamental(torch.zeros(2, 8, 6))
    with pytest.raises(L.DransacError, match="matches"):
        ops.weighted_fundamental(torch.zeros(8, 4))
    with pytest.raises(L.DransacError, match="float32 or float64"):
        ops.weighted_fundamental(torch.zeros(2, 8, 4, dtype=torch.float16))
    with pytest.raises(L.DransacError, match="weights"):
        ops.weighted_fundamental(m, torch.ones(2, 7))
    with pytest.raises(L.DransacError, match="weights"):
        ops.weighted_fundamental(m, torch.ones(2, 8, dtype=torch.int32))
    with pytest.raises(L.DransacError, match="mask"):
        ops.weighted_fundamental(m, None, torch.ones(2, 9, dtype=torch.bool))
    with pytest.raises(L.DransacError, match="mask"):
        ops.weighted_fundamental(m, None, torch.ones(2, 8))
    assert calls == []


@pytest.mark.parametrize("dtype,sfx", [(torch.float32, "f32"), (torch.float64, "f64")])
@pytest.mark.parametrize("want_m,want_w", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("masked", [False, True])
def test_forward_and_backward_issue_the_entries(monkeypatch, dtype, sfx, want_m, want_w, masked):
    """the launches of one forward and one backward, recorded instead of made (tensors on the CPU, pointers replaced by what they point
    to): dr_refit_fundamental_* with (matches, mask | NULL, weights, P, N, model, valid), dr_refit_fundamental_bwd_* with
    (matches, mask | NULL, weights, grad_model [P,3,3], P, N, grad_matches | NULL, grad_weights | NULL)"""
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    monkeypatch.setattr(ops, "_gpu_only", lambda *a, **k: None)
    monkeypatch.setattr(ops, "ptr", lambda t: t)
    monkeypatch.setattr(ops, "stream", lambda: "stream")
    P, N = 2, 11
    m = torch.rand(P, N, 4, dtype=dtype).requires_grad_(want_m)
    w = torch.rand(P, N, dtype=torch.float64).requires_grad_(want_w)      # (another dtype than the matches': converted on the way in)
    mask = (torch.rand(P, N) < 0.9) if masked else None
    model, valid = ops.weighted_fundamental(m, w, mask)
    assert model.shape == (P, 3, 3) and model.dtype == dtype and valid.shape == (P,) and valid.dtype == torch.bool
    assert model.requires_grad and not valid.requires_grad
    (name, fm, fk, fw, fP, fN, fmodel, fvalid, fs), = calls
    assert name == f"dr_refit_fundamental_{sfx}" and (fP, fN, fs) == (P, N, "stream")
    assert torch.equal(fm, m.detach()) and fw.dtype == dtype and torch.equal(fw, w.detach().to(dtype))
    assert (fk is None) if not masked else (fk.dtype == torch.uint8 and torch.equal(fk.bool(), mask))
    assert fmodel.shape == (P, 3, 3) and fvalid.shape == (P,)
    g = torch.rand(P, 3, 3, dtype=dtype)
    model.backward(g)
    (name, bm, bk, bw, bg, bP, bN, gm, gw, bs), = calls[1:]
    assert name == f"dr_refit_fundamental_bwd_{sfx}" and (bP, bN, bs) == (P, N, "stream")
    assert torch.equal(bm, fm) and torch.equal(bw, fw) and torch.equal(bg, g) and bg.shape == (P, 3, 3)
    assert (bk is None) if not masked else torch.equal(bk, fk)
    assert (gm is not None) == want_m and (gw is not None) == want_w
    assert gm is None or (gm.shape == (P, N, 4) and gm.dtype == dtype)
    assert gw is None or (gw.shape == (P, N) and gw.dtype == dtype)
    assert (m.grad is not None) == want_m and (w.grad is not None) == want_w
    assert w.grad is None or w.grad.dtype == torch.float64      # (the gradient comes back in the caller's dtype)


def test_without_weights_the_slot_is_null_and_the_op_is_once_differentiable(monkeypatch):
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    monkeypatch.setattr(ops, "_gpu_only", lambda *a, **k: None)
    monkeypatch.setattr(ops, "ptr", lambda t: t)
    monkeypatch.setattr(ops, "stream", lambda: "stream")
    m = torch.rand(1, 8, 4, requires_grad=True)
    model, _ = ops.weighted_fundamental(m)
    assert calls[0][3] is None
    g = torch.rand(1, 3, 3, requires_grad=True)      # (an upstream gradient that is itself differentiated: a second derivative)
    (gm,) = torch.autograd.grad(model, m, g, create_graph=True)
    assert calls[1][0] == "dr_refit_fundamental_bwd_f32" and calls[1][3] is None and calls[1][8] is None
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gm.sum().backward()
