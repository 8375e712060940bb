"""dr_refit_fundamental_bwd and ops.weighted_fundamental against the f64 references of tests/fundamental_grad_ref.py, in f32 and f64.
Inputs, tolerance rule and its constant are that module's: per pair |g - g_ref|_inf <= c eps kappa_eff mag; no pair of its cases is
exempt (kappa <= KAPPA_MAX everywhere: tests/test_fundamental_grad_host.py).  The reference's gradients belong to the reference's F;
a device forward of the other sign has the negated ones (forward_signs): a backward that recomputed the eigenvector with another sign
than its forward fails every comparison here."""
import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from differentiable_ransac_amd import ops, synth
from differentiable_ransac_amd.loss import MatchLoss
from tests import fundamental_grad_ref as G

pytestmark = pytest.mark.gpu

DTYPES = {"f32": (torch.float32, "float32"), "f64": (torch.float64, "float64")}
SENTINEL = 777.0
WANTS = ((False, True), (True, False), (True, True))      # (grad_matches, grad_weights): weights only, matches only, both
WORST = {"f32": 0.0, "f64": 0.0}                          # the largest error / tolerance ratio seen, per dtype


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _dev(a, dev, tdt):
    return None if a is None else torch.tensor(a, dtype=tdt, device=dev)


def _mask(mask, dev):
    return None if mask is None else torch.tensor(mask, device=dev)


def _bwd(dev, tdt, x, w, mask, gF, want=(True, True)):
    """dr_refit_fundamental_bwd on buffers pre-filled with a sentinel -> (grad_matches | None, grad_weights | None) as f64 numpy"""
    m = _dev(x, dev, tdt)
    P, N, _ = m.shape
    wt, g = _dev(w, dev, tdt), _dev(gF, dev, tdt).reshape(P, 9)
    mk = None if mask is None else torch.tensor(mask, device=dev).view(torch.uint8)
    gm = torch.full((P, N, 4), SENTINEL, dtype=tdt, device=dev) if want[0] else None
    gw = torch.full((P, N), SENTINEL, dtype=tdt, device=dev) if want[1] else None
    L.call(f"dr_refit_fundamental_bwd_{L.suffix(tdt)}", L.ptr(m), L.ptr(mk), L.ptr(wt), L.ptr(g), P, N, L.ptr(gm), L.ptr(gw), L.stream())
    torch.cuda.synchronize()
    return tuple(None if t is None else t.double().cpu().numpy() for t in (gm, gw))


def _fwd(dev, tdt, x, w, mask):
    """ops.refit_fundamental -> (F [P,3,3] f64 numpy, valid [P] list)"""
    F, valid = ops.refit_fundamental(_dev(x, dev, tdt), _mask(mask, dev), _dev(w, dev, tdt))
    return F.double().cpu().numpy(), valid.cpu().tolist()


def _compare(got, ref, signs, case, dt, label):
    """every pair of (gm, gw) against a pair_reference (times the forward's sign) under the module's tolerance; exact zeros where the
    rules say so"""
    gm, gw = got
    P = case["x"].shape[0]
    for p in range(P):
        sel, _, _ = G.selected(case, p)
        tol = G.tolerances(ref, p, DTYPES[dt][1])
        assert tol is not None, (label, p, "kappa above KAPPA_MAX: the case must not be exempt")
        for out, want, k in ((gm, ref["gx"], 0), (gw, ref["gw"], 1)):
            if out is None:
                continue
            assert not (out[p] == SENTINEL).any(), (label, p, "an element was not written")
            assert (out[p][~sel] == 0.0).all(), (label, p, "a dropped row is not exactly zero")
            err = np.abs(out[p] - signs[p] * want[p]).max()
            WORST[dt] = max(WORST[dt], err / tol[k])
            print(f"{label} pair {p} {'gm' if k == 0 else 'gw'}: err {err:.3g} tol {tol[k]:.3g} ratio {err / tol[k]:.3g}")
            assert err <= tol[k], (label, p, k, err, tol[k])


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N,P,weighted,masked", G.PAIR_CASES)
def test_gradients_against_reference(dev, N, P, weighted, masked, dt):
    """every requested-output combination; what is requested alone has the bits of what is requested together"""
    tdt, name = DTYPES[dt]
    cs, ref = G.cached_case(N, P, weighted, masked, name)
    F, valid = _fwd(dev, tdt, cs["x"], cs["w"], cs["mask"])
    assert all(valid)
    both = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gF"])
    _compare(both, ref, G.forward_signs(ref, F), cs, dt, f"N={N} P={P} w={weighted} m={masked} {dt}")
    for want in WANTS[:2]:
        got = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gF"], want)
        for a, b, asked in zip(got, both, want):
            assert (a is None) == (not asked)
            assert a is None or np.array_equal(a, b)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N,P,weighted,masked", [(8, 1, False, False), (257, 3, True, True), (1000, 3, True, False)])
def test_forward_is_refit_fundamental_bit_for_bit_and_autograd_reaches_the_entry(dev, N, P, weighted, masked, dt):
    """want-only-weights and want-only-matches each leave the other gradient unallocated"""
    tdt, name = DTYPES[dt]
    cs, _ = G.cached_case(N, P, weighted, masked, name)
    mask = _mask(cs["mask"], dev)
    g = _dev(cs["gF"], dev, tdt)
    want_m, want_w = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gF"])
    for req_m, req_w in WANTS:
        m = _dev(cs["x"], dev, tdt).requires_grad_(req_m)
        # (the caller's weights may be of another dtype: the gradient comes back in it)
        w = None if cs["w"] is None else _dev(cs["w"], dev, torch.float64).requires_grad_(req_w)
        model, valid = ops.weighted_fundamental(m, w, mask)
        rm, rv = ops.refit_fundamental(m.detach(), mask, None if w is None else w.detach())
        assert torch.equal(model.detach(), rm) and torch.equal(valid, rv) and valid.dtype == torch.bool and not valid.requires_grad
        if not (req_m or (req_w and w is not None)):
            assert not model.requires_grad
            continue
        model.backward(g)
        assert (m.grad is not None) == req_m
        if req_m:
            assert np.array_equal(m.grad.double().cpu().numpy(), want_m)
        if w is not None:
            assert (w.grad is not None) == req_w
            if req_w:
                assert w.grad.dtype == torch.float64 and np.array_equal(w.grad.cpu().numpy(), want_w)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_a_mask_that_leaves_exactly_eight_rows(dev, dt):
    """eight kept rows scattered over 257 (both strides of the block): the minimal fit, against the reference on those rows"""
    tdt, name = DTYPES[dt]
    sc = G.scene(0, 8)      # (the well-conditioned minimal scene of the N = 8 case)
    filler, _ = G.cached_case(257, 3, True, True, name)
    keep = np.array([3, 64, 100, 191, 192, 255, 256, 17])
    x = filler["x"][:1].copy()
    x[0, keep] = G._round(sc["matches"], name)
    mask = np.zeros((1, 257), bool)
    mask[0, keep] = True
    w = filler["w"][:1].copy()
    w[0, keep] = G._round(0.5 + 0.5 * np.random.default_rng(8).uniform(size=8), name)      # (inliers' weights, as in the cases)
    cs = dict(x=x, w=w, mask=mask, gF=filler["gF"][:1])
    ref = G.pair_reference(cs)
    assert ref["rows"][0] == 8 and ref["kappa"][0] <= G.KAPPA_MAX
    F, valid = _fwd(dev, tdt, cs["x"], cs["w"], cs["mask"])
    assert valid == [True]
    got = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gF"])
    assert all(np.abs(o).max() > 0 for o in got)
    _compare(got, ref, G.forward_signs(ref, F), cs, dt, f"eight of 257 {dt}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_exact_correspondences(dev, dt):
    """exact rows: the weight gradient is zero within its counted magnitude, the matches gradient is the reference's"""
    tdt, name = DTYPES[dt]
    cs = G.exact_case(np.dtype(name))
    ref = G.pair_reference(cs)
    F, valid = _fwd(dev, tdt, cs["x"], None, None)
    assert valid == [True]
    s = G.forward_signs(ref, F)[0]
    gm, gw = _bwd(dev, tdt, cs["x"], None, None, cs["gF"])
    tol = G.tolerances(ref, 0, name)
    print(f"exact {dt}: |gw| {np.abs(gw).max():.3g} tol {tol[1]:.3g}; gm err {np.abs(gm - s * ref['gx']).max():.3g} tol {tol[0]:.3g}")
    assert np.abs(gw).max() <= tol[1]
    assert np.abs(gm - s * ref["gx"]).max() <= tol[0]


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_the_sign_of_the_upstream_negates_bit_for_bit(dev, dt):
    tdt, name = DTYPES[dt]
    cs, _ = G.cached_case(257, 3, True, True, name)
    pos = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gF"])
    neg = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], -cs["gF"])
    for a, b in zip(pos, neg):
        assert np.array_equal(a, -b) and np.abs(a).max() > 0


# ------------------------------------------------------------------------------------------------------------ zero rules
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_zero_rules(dev, dt):
    tdt, name = DTYPES[dt]
    cs, ref = G.cached_case(257, 3, True, True, name)
    x, w, mask, gF = cs["x"], cs["w"], cs["mask"], cs["gF"]
    base = _bwd(dev, tdt, x, w, mask, gF)
    # seven masked-in rows among 257: all zeros, every element written
    seven = np.zeros_like(mask)
    seven[:, [5, 64, 100, 191, 192, 255, 256]] = True
    for out in _bwd(dev, tdt, x, w, seven, gF):
        assert (out == 0.0).all()
    # an N = 7 pair (below what the forward's entry accepts): all zeros
    for out in _bwd(dev, tdt, x[:, :7], w[:, :7], None, gF):
        assert out.shape[1] == 7 and (out == 0.0).all()
    # NaN coordinates (and weights) in the rows the mask drops: exact zeros there, the kept rows' bits unchanged
    xn, wn = x.copy(), w.copy()
    xn[~mask], wn[~mask] = np.nan, np.nan
    for a, b in zip(_bwd(dev, tdt, xn, wn, mask, gF), base):
        assert np.array_equal(a, b) and (a[~mask] == 0.0).all() and np.abs(a[mask]).max() > 0
    # a NaN in a kept row of pair 1 (valid = 0): zeros for that pair, the other two pairs' bits as when run alone
    xd = x.copy()
    xd[1, np.flatnonzero(mask[1])[3], 2] = np.nan
    _, valid = _fwd(dev, tdt, xd, w, mask)
    assert valid == [True, False, True]
    got = _bwd(dev, tdt, xd, w, mask, gF)
    for k, out in enumerate(got):
        assert (out[1] == 0.0).all()
        for p in (0, 2):
            alone = _bwd(dev, tdt, x[p:p + 1], w[p:p + 1], mask[p:p + 1], gF[p:p + 1])[k]
            assert np.array_equal(out[p], alone[0]) and np.array_equal(out[p], base[k][p])
    # a NaN upstream gradient is a non-finite intermediate: zeros for that pair only
    gn = gF.copy()
    gn[2, 1, 1] = np.nan
    for a, b in zip(_bwd(dev, tdt, x, w, mask, gn), base):
        assert (a[2] == 0.0).all() and np.array_equal(a[:2], b[:2])


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_a_row_at_the_centroid(dev, dt):
    """thirteen rows, the last exactly at both centroids (point-symmetric integer offsets: the means are exact): |q| = 0 takes the zero
    subgradient, in the kernel and in the reference"""
    tdt, name = DTYPES[dt]
    cs = G.centroid_case(np.dtype(name))
    ref = G.pair_reference(cs)
    assert ref["kappa"][0] <= G.KAPPA_MAX
    F, valid = _fwd(dev, tdt, cs["x"], cs["w"], None)
    assert valid == [True]
    got = _bwd(dev, tdt, cs["x"], cs["w"], None, cs["gF"])
    assert all(np.isfinite(o).all() for o in got)
    _compare(got, ref, G.forward_signs(ref, F), cs, dt, f"centroid row {dt}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_two_launches_give_the_same_bytes(dev, dt):
    tdt, name = DTYPES[dt]
    cs, _ = G.cached_case(1000, 3, True, False, name)
    a = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gF"])
    b = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gF"])
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------------------ end to end
def test_logits_to_loss_end_to_end(dev):
    """w = sigmoid(logits) -> ops.weighted_fundamental -> MatchLoss(fmat=False) on model[:, None] with keep = valid -> backward, in
    f64 on calibrated matches (the fit is the linear estimate of E), against the same chain through reference (a) and the project's f64
    MatchLoss path (ops._match_loss_mean_f64: plain torch ops) on the CPU.  Per pair the bound is the weight gradient's, c eps64 kappa
    mag with mag counted for the loss's own dL/dF as the upstream; sigmoid' <= 1/4 leaves a factor four for the rounding of that upstream."""
    P, N = 3, 257
    scenes = [synth.two_view_pair(600 + p, N, inlier_ratio=G.INLIER_SHARE, noise=1e-3, dtype=torch.float64) for p in range(P)]
    x = np.stack([s["matches"].numpy() for s in scenes])
    inl = np.stack([s["inliers"].numpy() for s in scenes])
    rng = np.random.default_rng(9)
    logits = np.where(inl, 2.0, -2.0) + rng.standard_normal((P, N))
    lt = torch.tensor(logits, device=dev, requires_grad=True)
    m, gt_mask = torch.tensor(x, device=dev), torch.tensor(inl, device=dev)
    model, valid = ops.weighted_fundamental(m, torch.sigmoid(lt))
    assert valid.all()
    loss = MatchLoss(fmat=False)(model[:, None], m, gt_mask, keep=valid[:, None])
    loss.backward()
    # the reference chain on the CPU
    Fd = model.detach().cpu().numpy()
    lr, xr = torch.tensor(logits, requires_grad=True), torch.tensor(x)
    wr = torch.sigmoid(lr)
    models = torch.stack([G.torch_fit(xr[p], wr[p], Fd[p]) for p in range(P)])[:, None]
    models.retain_grad()
    ref_loss = ops._match_loss_mean_f64(xr, torch.tensor(inl), models, torch.ones(P, 1, dtype=torch.bool))
    ref_loss.backward()
    assert float(loss.detach()) == pytest.approx(float(ref_loss.detach()), rel=1e-9)
    got, want = lt.grad.cpu().numpy(), lr.grad.numpy()
    # (outliers at weight sigmoid(-2)^2 still bend the fit: the loss is above its noise floor and the logits have a real gradient)
    assert 0.0 < float(ref_loss.detach()) < 1.0 and np.abs(want).max() > 0.0
    for p in range(P):
        wp = wr[p].detach().numpy()
        kap = G.kappa(x[p], wp)
        assert kap <= G.KAPPA_MAX
        tol = G.tolerance_constant() * G.EPS64 * kap * G.weight_grad_magnitude(x[p], wp, models.grad[p, 0].numpy())
        err = np.abs(got[p] - want[p]).max()
        WORST["f64"] = max(WORST["f64"], err / tol)
        print(f"end to end pair {p}: err {err:.3g} tol {tol:.3g} |g| {np.abs(want[p]).max():.3g} ratio {err / tol:.3g}")
        assert err <= tol


def test_report_the_worst_ratio():
    """(last in the file) the largest error / tolerance ratio of the comparisons above, per dtype: docs/LOG.md records it"""
    print("worst error / tolerance ratio: " + ", ".join(f"{dt} {v:.3g}" for dt, v in WORST.items()))
    assert all(v <= 1.0 for v in WORST.values())
