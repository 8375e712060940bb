"""dr_refit_homography_bwd and ops.weighted_homography against the f64 references of tests/homography_grad_ref.py, in f32 and f64.
Inputs, tolerance rule and its constant are that module's: per pair |g - g_ref|_inf <= c eps kappa_eff mag, a pair with
kappa > KAPPA_MAX checked for finiteness only."""
import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from differentiable_ransac_amd import ops
from differentiable_ransac_amd.loss import HomographyLoss
from tests import homography_grad_ref as G
from tests import homography_loss_ref as HLR
from tests import homography_ref as HR

pytestmark = pytest.mark.gpu

DTYPES = {"f32": (torch.float32, "float32"), "f64": (torch.float64, "float64")}
SENTINEL = 777.0
WANTS = ((False, True), (True, False), (True, True))      # (grad_matches, grad_weights): weights only, matches only, both


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _dev(a, dev, tdt):
    return None if a is None else torch.tensor(a, dtype=tdt, device=dev)


def _bwd(dev, tdt, x, w, mask, gH, want=(True, True)):
    """dr_refit_homography_bwd on buffers pre-filled with a sentinel -> (grad_matches | None, grad_weights | None) as f64 numpy"""
    m = x if torch.is_tensor(x) else _dev(x, dev, tdt)
    P, N, _ = m.shape
    wt, g = _dev(w, dev, tdt), _dev(gH, dev, tdt).reshape(P, 9)
    mk = None if mask is None else torch.tensor(mask, device=dev).view(torch.uint8)
    gm = torch.full((P, N, 4), SENTINEL, dtype=tdt, device=dev) if want[0] else None
    gw = torch.full((P, N), SENTINEL, dtype=tdt, device=dev) if want[1] else None
    L.call(f"dr_refit_homography_bwd_{L.suffix(tdt)}", L.ptr(m), L.ptr(mk), L.ptr(wt), L.ptr(g), P, N, L.ptr(gm), L.ptr(gw), L.stream())
    torch.cuda.synchronize()
    return tuple(None if t is None else t.double().cpu().numpy() for t in (gm, gw))


def _compare(got, ref, case, dt, label):
    """every pair of (gm, gw) against a pair_reference under the module's tolerance; exact zeros where the rules say so"""
    gm, gw = got
    P = case["x"].shape[0]
    for p in range(P):
        sel, _, _ = G.selected(case, p)
        tol = G.tolerances(ref, p, DTYPES[dt][1])
        for out, want, k in ((gm, ref["gx"], 0), (gw, ref["gw"], 1)):
            if out is None:
                continue
            assert not (out[p] == SENTINEL).any(), (label, p, "an element was not written")
            assert (out[p][~sel] == 0.0).all(), (label, p, "a dropped row is not exactly zero")
            if ref["rows"][p] < 4:
                assert (out[p] == 0.0).all(), (label, p, "fewer than four rows")
            elif tol is None:
                assert np.isfinite(out[p]).all()
            else:
                err = np.abs(out[p] - want[p]).max()
                print(f"{label} pair {p} {'gm' if k == 0 else 'gw'}: err {err:.3g} tol {tol[k]:.3g} ratio {err / tol[k]:.3g}")
                assert err <= tol[k], (label, p, k, err, tol[k])


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N,P,weighted,masked", G.PAIR_CASES)
def test_gradients_against_reference(dev, N, P, weighted, masked, dt):
    """every requested-output combination; what is requested alone has the bits of what is requested together"""
    tdt, name = DTYPES[dt]
    cs, ref = G.cached_case(N, P, weighted, masked, name)
    both = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gH"])
    _compare(both, ref, cs, dt, f"N={N} P={P} w={weighted} m={masked} {dt}")
    for want in WANTS[:2]:
        got = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gH"], want)
        for a, b, asked in zip(got, both, want):
            assert (a is None) == (not asked)
            assert a is None or np.array_equal(a, b)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N,P,weighted,masked", [(4, 1, False, False), (257, 3, True, True), (1000, 3, True, False)])
def test_forward_is_refit_homography_bit_for_bit_and_autograd_reaches_the_entry(dev, N, P, weighted, masked, dt):
    tdt, name = DTYPES[dt]
    cs, _ = G.cached_case(N, P, weighted, masked, name)
    mask = None if cs["mask"] is None else torch.tensor(cs["mask"], device=dev)
    g = _dev(cs["gH"], dev, tdt)
    want_m, want_w = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gH"])
    for req_m, req_w in WANTS:
        m = _dev(cs["x"], dev, tdt).requires_grad_(req_m)
        # (the caller's weights may be of another dtype: the gradient comes back in it)
        w = None if cs["w"] is None else _dev(cs["w"], dev, torch.float64).requires_grad_(req_w)
        model, valid = ops.weighted_homography(m, w, mask)
        rm, rv = ops.refit_homography(m.detach(), mask, None if w is None else w.detach())
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
def test_exact_correspondences(dev, dt):
    """N = 4 exact: the weight gradient is zero within its counted magnitude, the matches gradient is the reference's"""
    tdt, name = DTYPES[dt]
    cs = G.exact_case(np.dtype(name))
    ref = G.pair_reference(cs)
    gm, gw = _bwd(dev, tdt, cs["x"], None, None, cs["gH"])
    tol = G.tolerances(ref, 0, name)
    print(f"exact {dt}: |gw| {np.abs(gw).max():.3g} tol {tol[1]:.3g}; gm err {np.abs(gm - ref['gx']).max():.3g} tol {tol[0]:.3g}")
    assert np.abs(gw).max() <= tol[1]
    assert np.abs(gm - ref["gx"]).max() <= tol[0]


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_a_multiple_of_h_passes_nothing_on_and_the_sign_of_the_upstream_negates(dev, dt):
    """grad_model = 2.5 H: what is left of it after the projection is its rounding, eps(dtype) |2.5 H| (in f32 H itself arrives rounded),
    and the derivative is linear in the upstream, so the bound is the case's tolerance scaled by |2.5 H| / |gH - H <H, gH>|.
    Feeding -gH negates every output bit for bit."""
    tdt, name = DTYPES[dt]
    cs, ref = G.cached_case(257, 3, True, True, name)
    mask = torch.tensor(cs["mask"], device=dev)
    H, _ = ops.refit_homography(_dev(cs["x"], dev, tdt), mask, _dev(cs["w"], dev, tdt))
    H = H.double().cpu().numpy()
    gm, gw = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], 2.5 * H)
    for p in range(3):
        perp = cs["gH"][p] - H[p] * (H[p] * cs["gH"][p]).sum()
        tm, tw = (t * 2.5 / np.linalg.norm(perp) for t in G.tolerances(ref, p, name))
        print(f"c H {dt} pair {p}: |gm| {np.abs(gm[p]).max():.3g} tol {tm:.3g}; |gw| {np.abs(gw[p]).max():.3g} tol {tw:.3g}")
        assert np.abs(gm[p]).max() <= tm and np.abs(gw[p]).max() <= tw
    pos = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gH"])
    neg = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], -cs["gH"])
    for a, b in zip(pos, neg):
        assert np.array_equal(a, -b) and np.abs(a).max() > 0


# ------------------------------------------------------------------------------------------------------------ zero rules
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_zero_rules(dev, dt):
    tdt, name = DTYPES[dt]
    cs, ref = G.cached_case(257, 3, True, True, name)
    x, w, mask, gH = cs["x"], cs["w"], cs["mask"], cs["gH"]
    base = _bwd(dev, tdt, x, w, mask, gH)
    # three masked-in rows among 257: all zeros, every element written
    three = np.zeros_like(mask)
    three[:, [5, 100, 256]] = True
    for out in _bwd(dev, tdt, x, w, three, gH):
        assert (out == 0.0).all()
    # NaN coordinates (and weights) in the rows the mask drops: exact zeros there, the kept rows' bits unchanged
    xn, wn = x.copy(), w.copy()
    xn[~mask], wn[~mask] = np.nan, np.nan
    for a, b in zip(_bwd(dev, tdt, xn, wn, mask, gH), base):
        assert np.array_equal(a, b) and (a[~mask] == 0.0).all() and np.abs(a[mask]).max() > 0
    # the kept rows of pair 1 are all one point (valid = 0): zeros for that pair, the other two pairs' bits as when run alone
    xd = x.copy()
    xd[1, mask[1]] = xd[1, mask[1]][0]
    _, valid = ops.refit_homography(_dev(xd, dev, tdt), torch.tensor(mask, device=dev), _dev(w, dev, tdt))
    assert valid.cpu().tolist() == [True, False, True]
    got = _bwd(dev, tdt, xd, w, mask, gH)
    for k, out in enumerate(got):
        assert (out[1] == 0.0).all()
        for p in (0, 2):
            alone = _bwd(dev, tdt, x[p:p + 1], w[p:p + 1], mask[p:p + 1], gH[p:p + 1])[k]
            assert np.array_equal(out[p], alone[0]) and np.array_equal(out[p], base[k][p])
    # a NaN upstream gradient is a non-finite intermediate: zeros for that pair only
    gn = gH.copy()
    gn[2, 1, 1] = np.nan
    for a, b in zip(_bwd(dev, tdt, x, w, mask, gn), base):
        assert (a[2] == 0.0).all() and np.array_equal(a[:2], b[:2])


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_a_row_at_the_centroid(dev, dt):
    """five rows, the last exactly at both centroids (symmetric integer offsets: the means are exact): |q| = 0 takes the zero
    subgradient, in the kernel and in the reference"""
    tdt, name = DTYPES[dt]
    c1, c2 = np.array([100.0, 50.0]), np.array([120.0, 70.0])
    o1, o2 = np.array([[30.0, 4.0], [-6.0, 25.0]]), np.array([[33.0, 1.0], [-9.0, 29.0]])
    x = np.concatenate([np.concatenate([c1 + o1, c1 - o1, c1[None]]), np.concatenate([c2 + o2, c2 - o2, c2[None]])], 1)[None]
    cs = dict(x=x, w=np.array([[0.5, 1.0, 0.75, 1.25, 1.0]]), mask=None, gH=G._round(np.random.default_rng(3).standard_normal((1, 3, 3)), name))
    ref = G.pair_reference(cs)
    assert ref["kappa"][0] <= G.KAPPA_MAX
    got = _bwd(dev, tdt, cs["x"], cs["w"], None, cs["gH"])
    assert all(np.isfinite(o).all() for o in got)
    _compare(got, ref, cs, dt, f"centroid row {dt}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_two_launches_give_the_same_bytes(dev, dt):
    tdt, name = DTYPES[dt]
    cs, _ = G.cached_case(1000, 3, True, True, name)
    a = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gH"])
    b = _bwd(dev, tdt, cs["x"], cs["w"], cs["mask"], cs["gH"])
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------------------ end to end
def test_logits_to_loss_end_to_end(dev):
    """w = sigmoid(logits) -> ops.weighted_homography -> HomographyLoss on model[:, None] -> backward, in f64, against the same chain
    through reference (a) and homography_loss_ref._loss.  Per pair the bound is the weight gradient's, c eps64 kappa mag with mag
    counted for the loss's own dL/dH as the upstream; sigmoid' <= 1/4 leaves a factor four for the rounding of that upstream."""
    P, N, thr = 3, 257, HR.THRESHOLD
    scenes = [HR.scene(300 + p, N, G.INLIER_SHARE) for p in range(P)]
    x = np.stack([s["matches"] for s in scenes])
    rng = np.random.default_rng(9)
    logits = np.stack([np.where(s["inlier"], 4.0, -4.0) for s in scenes]) + rng.standard_normal((P, N))
    lt = torch.tensor(logits, device=dev, requires_grad=True)
    m = torch.tensor(x, device=dev)
    model, valid = ops.weighted_homography(m, torch.sigmoid(lt))
    assert valid.all()
    loss = HomographyLoss(thr)(model[:, None], m, keep=valid[:, None])
    loss.backward()
    # the reference chain on the CPU
    lr, xr = torch.tensor(logits, requires_grad=True), torch.tensor(x)
    wr = torch.sigmoid(lr)
    models = torch.stack([G.torch_fit(xr[p], wr[p]) for p in range(P)])[:, None]
    models.retain_grad()
    ref_loss, *_ = HLR._loss(xr, models, torch.ones(P, N, dtype=torch.bool), torch.ones(P, 1, dtype=torch.bool),
                             torch.full((P,), thr * thr, dtype=torch.float64))
    ref_loss.backward()
    assert float(loss) == pytest.approx(float(ref_loss), rel=1e-10)
    got, want = lt.grad.cpu().numpy(), lr.grad.numpy()
    # (outliers at weight sigmoid(-4) still bend the fit: the loss is far from its floor and the logits have a real gradient)
    assert 0.0 < float(ref_loss) < 1.0 and np.abs(want).max() > 1e-3
    for p in range(P):
        wp = wr[p].detach().numpy()
        tol = G.tolerance_constant() * G.EPS64 * G.kappa(x[p], wp) * G.weight_grad_magnitude(x[p], wp, models.grad[p, 0].numpy())
        err = np.abs(got[p] - want[p]).max()
        print(f"end to end pair {p}: err {err:.3g} tol {tol:.3g} |g| {np.abs(want[p]).max():.3g}")
        assert err <= tol
