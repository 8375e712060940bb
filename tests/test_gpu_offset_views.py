"""Every op on contiguous views that start inside a larger buffer (tests/offset_views.py): a caller that packs ragged pairs into
one buffer and narrows per pair hands over tensors whose first byte is 4, 8 or 12 bytes (masks: 1, 4 or 8 bytes) past a 16-byte
boundary.  Each case runs once on aligned clones and once per offset view, same seeds, noise and thresholds.

Compared byte for byte (the view run takes the aligned run's arithmetic: the wrappers realign what the kernels read as vectors, or
the view only selects another LOAD / STORE form of the same kernel arithmetic):
  gumbel_topk / gumbel_topk_gather index sets and gathered samples (one Philox stream, the same keys in every kernel);
  gumbel_topk with explicit noise (all outputs); gumbel_topk_bwd and SampleGather forward / backward;
  msac_score, magsac_score, select_best, ransac_update (state in offset views, masks written into a caller's offset buffer; the
  scores of that call where the offset leaves the kernel unchanged);
  rigid_residual masks, ransac3d_update, rigid_msac_score, rigid_magsac_score;
  episym_sums, match_loss_mean, match_loss_per_pair (values and gradients);
  the pair families' score, soft score, loss, refit and weighted-fit ops; the three test-mode drivers.
Compared with the f64 reference at that reference's tolerance (the view selects a kernel with another summation order):
  gumbel_topk's soft-max statistics y_sel / lse with in-kernel noise where the aligned rows are served by the register or the
  long-row kernel and the view by the general kernel (oracle.cpu_ref.gumbel_topk, the bounds of tests/test_gpu_sampler.py);
  rigid_residual's sums where the view leaves the packed kernel for the general one (tests/msac_ref.py: rigid_ref, stack_refs);
  dr_msac_score's scores where a mask buffer that is not 16-byte aligned selects the eight-point kernel for rows of a multiple of
  16 points (sampson_ref, stack_refs: the rule of tests/test_gpu_msac_paths.py).
Every view's own content is unchanged by the calls, and the NaN / 0xFF slack around every view is intact after them."""
import math

import pytest
import torch

from oracle import cpu_ref as O
from tests import msac_ref as R
from tests.offset_views import SLACK, offset_view, slack_intact

F32, F64 = torch.float32, torch.float64


# ---- the helper itself: no GPU ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.uint8, torch.bool, torch.int32])
def test_offset_view_addresses_on_the_host(dtype):
    t = (torch.arange(2 * 7 * 4).reshape(2, 7, 4) % 2).to(dtype)
    for elems in (0, 1, 2, 3, 4, 8):
        v, buf = offset_view(t, elems, with_buffer=True)
        assert v.data_ptr() % 16 == (elems * t.element_size()) % 16, (dtype, elems)
        assert buf.data_ptr() % 16 == 0 and buf.numel() == t.numel() + SLACK
        assert v.is_contiguous() and v.shape == t.shape and v.dtype == t.dtype and torch.equal(v, t)
        assert slack_intact(v, buf)
        v.view(-1)[0] = 1          # writing the view leaves the slack alone ...
        assert slack_intact(v, buf)
        buf[elems + t.numel()] = 0      # ... and a write past it shows
        assert not slack_intact(v, buf)


# ---- shared -----------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b, what):
    """byte for byte (NaN payloads included)"""
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(_bits(a), _bits(b)), what


def _same_all(a, b, what):
    if torch.is_tensor(a) or a is None:
        return _same(a, b, what)
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same_all(a[k], b[k], f"{what}[{k}]")
        return
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        _same_all(x, y, f"{what}[{i}]")


class _Views:
    """offset views handed out for one call; check(): contents unchanged, slack intact"""

    def __init__(self, what):
        self.what, self.made = what, []

    def __call__(self, t, elems, writable=False):
        v, buf = offset_view(t, elems, with_buffer=True)
        self.made.append((v, buf, None if writable else t.clone(), elems))
        return v

    def check(self):
        for v, buf, orig, elems in self.made:
            assert slack_intact(v, buf), f"{self.what}: slack of the view at {elems} overwritten"
            if orig is not None:
                _same(v, orig, f"{self.what}: read-only view at {elems} changed")


def _two_view(dev, P, M, N, seed=700):
    mt, md = R.two_view_sets(P, M, N, seed)
    return mt.to(dev), md.to(dev)


def _valid(dev, P, M):
    return ((torch.arange(P * M).reshape(P, M) * 7) % 5 != 0).to(dev)


def _logits(P, N, seed=0):
    from differentiable_ransac_amd import synth
    return torch.stack([synth.two_view_pair(seed + 10 + p, max(N, 8))["logits"][:N] for p in range(P)])


# ---- K1 / K2 ----------------------------------------------------------------------------------------------------------------
GUMBEL = [(132, 5, None), (2052, 3, True), (2052, 3, False), (2052, 5, True), (2052, 5, False), (131, 8, None)]


def _soft_vs_oracle(r, logits, noise, k, what):
    """y_sel / lse against the f64 oracle under the noise the kernels drew (the bounds of test_gpu_sampler.py)"""
    for p in range(logits.shape[0]):
        idx, _, y_soft = O.gumbel_topk(logits[p], noise[p], 1.0, k)
        assert torch.equal(r["idx"][p].cpu().long(), idx), what
        ys = torch.gather(y_soft, 1, idx)
        assert (r["y_sel"][p].cpu() - ys).abs().max() <= 1e-6 + 1e-5 * ys.max(), what
        g = logits[p][None] + noise[p]
        assert (r["lse"][p].cpu() - torch.logsumexp(g.double(), -1)).abs().max() < 1e-4, what


@pytest.mark.gpu
@pytest.mark.parametrize("N,k,screen", GUMBEL)
def test_gumbel_topk_on_offset_logits(dev, N, k, screen):
    from differentiable_ransac_amd import ops
    P, B, seed = 2, 7, 1234
    lg_cpu = _logits(P, N)
    lg = lg_cpu.to(dev)
    ref = ops.gumbel_topk(lg.clone(), B, k, seed=seed, soft=False, screen=screen)["idx"]
    soft = ops.gumbel_topk(lg.clone(), B, k, seed=seed)
    noise = ops.gumbel_topk(lg.clone(), B, k, seed=seed, want_noise=True)["gumbel"].cpu()      # (the noise of the Philox stream)
    _same(soft["idx"], ref, f"gumbel_topk N={N} k={k}: soft and index-only index sets")
    _soft_vs_oracle(soft, lg_cpu, noise, k, f"gumbel_topk N={N} k={k} aligned soft")
    for off in (1, 2, 3):
        what = f"gumbel_topk N={N} k={k} screen={screen} logits at {off}"
        views = _Views(what)
        v = views(lg, off)
        _same(ops.gumbel_topk(v, B, k, seed=seed, soft=False, screen=screen)["idx"], ref, what + " index-only")
        r = ops.gumbel_topk(v, B, k, seed=seed)
        _same(r["idx"], ref, what + " soft idx")
        _soft_vs_oracle(r, lg_cpu, noise, k, what + " soft")
        views.check()


@pytest.mark.gpu
@pytest.mark.parametrize("N,k", [(132, 5), (131, 8)])
def test_gumbel_topk_explicit_noise_views(dev, N, k):
    from differentiable_ransac_amd import ops, synth
    P, B = 2, 7
    lg = _logits(P, N).to(dev)
    noise = synth.gumbel_noise((P, B, N), seed=N + k).to(dev)
    ref = ops.gumbel_topk(lg.clone(), B, k, 1.0, noise.clone(), dense=True)
    for lo, no in ((1, 0), (0, 1), (1, 1), (2, 3)):
        what = f"gumbel_topk explicit noise N={N}: logits at {lo}, noise at {no}"
        views = _Views(what)
        r = ops.gumbel_topk(views(lg, lo), B, k, 1.0, views(noise, no), dense=True)
        _same_all(r, ref, what)
        views.check()


@pytest.mark.gpu
@pytest.mark.parametrize("N,k", [(132, 5), (2052, 3), (2052, 5), (131, 8)])
def test_gumbel_topk_gather_views(dev, N, k):
    from differentiable_ransac_amd import ops
    P, B, seed = 2, 7, 77
    mt, _ = _two_view(dev, P, 1, N)
    lg = _logits(P, N).to(dev)
    ref = ops.gumbel_topk_gather(mt.clone(), lg.clone(), B, k, seed=seed)
    for mo, lo in ((0, 1), (0, 2), (0, 3), (1, 0), (1, 1)):
        what = f"gumbel_topk_gather N={N} k={k}: matches at {mo}, logits at {lo}"
        views = _Views(what)
        r = ops.gumbel_topk_gather(views(mt, mo), views(lg, lo), B, k, seed=seed)
        _same_all(r, ref, what)
        views.check()


@pytest.mark.gpu
@pytest.mark.parametrize("N,k", [(132, 5), (131, 5)])
def test_sampler_backward_views(dev, N, k):
    from differentiable_ransac_amd import ops
    P, B, seed = 2, 7, 99
    mt, _ = _two_view(dev, P, 1, N)
    lg = _logits(P, N).to(dev)
    g = torch.Generator().manual_seed(N)
    gs = torch.randn(P, B, k, 4, generator=g).to(dev)
    gw = torch.randn(P, B, k, generator=g).to(dev)

    def run(m, l, g_samples, g_w):
        l.requires_grad_(True)
        samples, w, idx = ops.SampleGather.apply(m, l, B, k, 1.0, None, seed)
        torch.autograd.backward([samples, w], [g_samples, g_w])
        return dict(samples=samples.detach(), w=w.detach(), idx=idx, grad=l.grad)

    ref = run(mt.clone(), lg.clone(), gs.clone(), gw.clone())
    assert ref["grad"].abs().sum() > 0
    for mo, lo, go in ((0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1)):
        what = f"SampleGather N={N}: matches at {mo}, logits at {lo}, upstream gradient at {go}"
        views = _Views(what)
        l = views(lg, lo)
        r = run(views(mt, mo), l, views(gs, go), gw.clone())
        _same_all(r, ref, what)
        assert r["grad"].shape == l.shape
        l.requires_grad_(False)
        views.check()
    # the sampler's backward entry on its own: the statistics of ONE forward, the logits aligned and at 1 element
    fwd = ops.gumbel_topk(lg.clone(), B, k, seed=seed)
    a_sel = torch.randn(P, B, k, generator=g).to(dev)
    gref = ops.gumbel_topk_bwd(lg.clone(), None, seed, 1.0, fwd["idx"], fwd["lse"], a_sel)
    views = _Views(f"gumbel_topk_bwd N={N}")
    gv = ops.gumbel_topk_bwd(views(lg, 1), None, seed, 1.0, fwd["idx"], fwd["lse"], views(a_sel, 1))
    _same(gv, gref, f"gumbel_topk_bwd N={N}: logits and a_sel at 1")
    views.check()


# ---- K4 / K6 ----------------------------------------------------------------------------------------------------------------
MSAC_SHAPES = [(33, 64), (64, 64), (33, 72), (64, 72), (33, 131), (33, 264), (33, 272)]      # (264: eight points per lane, 272: sixteen)
THR = R.THR


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", MSAC_SHAPES)
def test_two_view_scoring_views(dev, M, N):
    from differentiable_ransac_amd import ops
    P = 2
    mt, md = _two_view(dev, P, M, N)
    valid = _valid(dev, P, M)
    thr = torch.full((P,), THR, device=dev)

    def run(m, d, v):
        s, k = ops.msac_score(m, d, thr, valid=v)
        g, inl = ops.magsac_score(m, d, thr, valid=v, want_inliers=True)
        return dict(scores=s, masks=k, magsac=g, inliers=inl, best=ops.select_best(m, d, s, thr, valid=v))

    ref = run(mt.clone(), md.clone(), valid.clone())
    assert ref["masks"].any() and (ref["scores"] > 0).any()
    for mo, do, vo in ((1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        what = f"msac / magsac / select_best M={M} N={N}: matches at {mo}, models at {do}, valid at {vo}"
        views = _Views(what)
        _same_all(run(views(mt, mo), views(md, do), views(valid, vo)), ref, what)
        views.check()


def _msac_into(masks, mt, md, valid, thr):
    """dr_msac_score_f32 with the mask rows written into the caller's buffer (the binding ops.msac_score uses)"""
    from differentiable_ransac_amd import _lib as L
    P, N, _ = mt.shape
    M = md.shape[1]
    scores = torch.empty(P, M, device=mt.device)
    L.call("dr_msac_score_f32", L.ptr(mt), L.ptr(md), L.ptr(valid.view(torch.uint8)), L.ptr(thr), P, M, N, L.ptr(scores),
           L.ptr(masks), L.ptr(None), L.ptr(None), L.stream())
    return scores


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", MSAC_SHAPES)
def test_masks_written_into_offset_buffers(dev, M, N):
    from differentiable_ransac_amd import ops
    P, B, k = 2, M, 5
    mt, md = _two_view(dev, P, M, N)
    valid = _valid(dev, P, M)
    thr = torch.full((P,), THR, device=dev)
    ref_scores, ref_masks = ops.msac_score(mt, md, thr, valid=valid)

    def update(best_mask_off, mo):
        views = _Views(f"ransac_update M={M} N={N}: best_mask at {best_mask_off} bytes, matches at {mo}")
        st = ops.RansacState(P, N, 1000, dev, F32)
        if best_mask_off is not None:
            st.best_mask = views(st.best_mask, best_mask_off, writable=True)
            st.best_model = views(st.best_model, 1, writable=True)
            st.best_score = views(st.best_score, 1, writable=True)
        ops.ransac_update(st, views(mt, mo) if mo else mt, md, valid, ref_scores, thr, B, k)
        views.check()
        return dict(score=st.best_score, model=st.best_model, mask=st.best_mask, inliers=st.best_inliers, iters=st.iters,
                    max_iters=st.max_iters)

    ref = update(None, 0)
    assert ref["mask"].any()
    for off in (1, 4, 8):
        what = f"M={M} N={N}: caller-owned masks at {off} bytes"
        views = _Views(what)
        masks = views(torch.zeros(P, M, N, dtype=torch.bool, device=dev), off, writable=True)
        scores = _msac_into(masks, mt, md, valid, thr)
        _same(masks, ref_masks, what + ": dr_msac_score mask rows")
        if R.dispatch(P, M, N, F32, True)[0] == R.dispatch(P, M, N, F32, False)[0]:
            _same(scores, ref_scores, what + ": dr_msac_score scores")
        else:      # rows of a multiple of 16 points: the view leaves the sixteen-point kernel for the eight-point one
            d = R.dispatch(P, M, N, F32, False)
            exp = R.stack_refs([R.sampson_ref(mt[p].cpu(), md[p].cpu(), THR, R.unit(F32)) for p in range(P)], R.c_red(d[3], d[2]),
                               R.unit(F32))
            for sc, name in ((scores, "view"), (ref_scores, "aligned")):
                err = (sc.cpu().double() - exp["scores"]).abs()
                live = valid.cpu() & ~exp["nan"]
                assert (err[live] <= exp["tol"][live]).all(), (what, name, float((err[live] / exp["tol"][live]).max()))
                assert (sc.cpu()[~valid.cpu()] == 0).all(), (what, name)
        views.check()
        _same_all(update(off, 0), ref, what + ": ransac_update state")
    _same_all(update(1, 1), ref, f"M={M} N={N}: ransac_update, matches at 1 and best_mask at 1")
    _same_all(update(8, 2), ref, f"M={M} N={N}: ransac_update, matches at 2 and best_mask at 8")


# ---- the 3-D kernels ----------------------------------------------------------------------------------------------------------
def _rigid_into(masks, pts, md, threshold):
    from differentiable_ransac_amd import _lib as L
    P, N, _ = pts.shape
    M = md.shape[1]
    res = torch.empty(P, M, device=pts.device)
    L.call("dr_rigid_residual_f32", L.ptr(pts), L.ptr(md), threshold, P, M, N, L.ptr(res), L.ptr(masks), 0, L.stream())
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("N", [32, 40, 131])
def test_rigid_kernels_views(dev, N):
    from differentiable_ransac_amd import ops
    P, M, thr = 2, 33, 9e-4
    pts_c, md_c = R.rigid_sets(P, M, N, 3100 + N)
    pts, md = pts_c.to(dev), md_c.to(dev)
    valid = _valid(dev, P, M)
    exp = R.stack_refs([R.rigid_ref(pts_c[p], md_c[p], float(torch.tensor(thr, dtype=F32)), R.unit(F32)) for p in range(P)],
                       R.c_red_rigid(1, 1), R.unit(F32))

    def sums_ok(res, what):
        err = (res.cpu().double() - exp["scores"]).abs()
        assert (err <= exp["tol"]).all(), (what, float((err / exp["tol"]).max()))

    def run(x, d, v, best_mask):
        res, masks = ops.rigid_residual(x, d, thr)
        out_res, out_model, idx = ops.ransac3d_update(x, d, v, res, thr, None, None, best_mask)
        s1, i1 = ops.rigid_msac_score(x, d, 0.03, valid=v)
        s2, i2 = ops.rigid_magsac_score(x, d, 0.03, valid=v)
        return dict(res=res, masks=masks, out_res=out_res, out_model=out_model, idx=idx, best_mask=best_mask, msac=s1, msac_inl=i1,
                    magsac=s2, magsac_inl=i2)

    ref = run(pts.clone(), md.clone(), valid.clone(), torch.zeros(P, N, dtype=torch.bool, device=dev))
    sums_ok(ref["res"], f"rigid_residual N={N} aligned")
    assert ref["masks"].any() and (ref["idx"] >= 0).all()
    for p in range(P):      # (the winner's mask row: with few points the smallest residual sum may belong to a model without inliers)
        assert torch.equal(ref["best_mask"][p], ref["masks"][p, int(ref["idx"][p])]), f"ransac3d_update N={N}: best_mask of pair {p}"
    packed = N % 16 == 0      # (the aligned run is served by the packed kernel; a view of the points by the general one)
    for xo, do, vo, bo in ((1, 0, 0, 1), (2, 0, 0, 8), (0, 1, 1, 1), (2, 1, 1, 8)):
        what = f"3-D kernels N={N}: pts at {xo}, models at {do}, valid at {vo}, best_mask at {bo} bytes"
        views = _Views(what)
        bm = views(torch.zeros(P, N, dtype=torch.bool, device=dev), bo, writable=True)
        r = run(views(pts, xo), views(md, do), views(valid, vo), bm)
        views.check()
        if packed and xo == 2:      # 8-byte aligned points: float2 loads stay, the float4 kernel is left -- another reduction order
            sums_ok(r["res"], what)
            rest = [k for k in ref if k not in ("res", "out_res")]
            _same_all({k: r[k] for k in rest}, {k: ref[k] for k in rest}, what)
        else:
            _same_all(r, ref, what)
    for off in (1, 8):      # mask rows written into a caller's buffer
        what = f"dr_rigid_residual N={N}: caller-owned masks at {off} bytes"
        views = _Views(what)
        masks = views(torch.zeros(P, M, N, dtype=torch.bool, device=dev), off, writable=True)
        res = _rigid_into(masks, pts, md, thr)
        _same(masks, ref["masks"], what)
        sums_ok(res, what)
        if off == 8 or not packed:
            _same(res, ref["res"], what + " (the aligned run's kernel)")
        views.check()


# ---- MatchLoss ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,N", [(32, 64), (33, 131), (33, 64), (32, 131)])
def test_match_loss_views(dev, M, N):
    from differentiable_ransac_amd import ops
    P = 2
    mt, md = _two_view(dev, P, M, N, seed=810)
    gen = torch.Generator().manual_seed(M * N)
    mask = (torch.rand(P, N, generator=gen) < 0.7).to(dev)
    keep = (torch.rand(P, M, generator=gen) < 0.8).to(dev)

    def run(m, k, d, kp):
        d.requires_grad_(True)
        out = {}
        for name, fn in (("sums", lambda: ops.episym_sums(m, k, d, kp)), ("mean", lambda: ops.match_loss_mean(m, k, d, kp)),
                         ("per_pair", lambda: ops.match_loss_per_pair(m, k, d, kp))):
            d.grad = None
            y = fn()
            y.sum().backward()
            out[name], out[name + "_grad"] = y.detach(), d.grad.clone()
        d.requires_grad_(False)
        d.grad = None
        return out

    ref = run(mt.clone(), mask.clone(), md.clone(), keep.clone())
    assert math.isfinite(float(ref["mean"])) and ref["mean_grad"].abs().sum() > 0
    for mo, ko, do, kpo in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)):
        what = f"MatchLoss M={M} N={N}: matches at {mo}, mask at {ko}, models at {do}, keep at {kpo}"
        views = _Views(what)
        r = run(views(mt, mo), views(mask, ko), views(md, do), views(keep, kpo))
        _same_all(r, ref, what)
        views.check()
    # one pair narrowed out of packed buffers, as a matcher hands ragged pairs over: packed[s:e] with s odd
    s = 5
    packed_mask = torch.full((s + N + 3,), 1, dtype=torch.bool, device=dev)
    packed_mask[s:s + N] = mask[0]
    packed_mt = torch.full(((s + N + 3) * 4,), float("nan"), device=dev)
    packed_mt[1:1 + N * 4] = mt[0].reshape(-1)
    one = run(mt[:1].clone(), mask[:1].clone(), md[:1].clone(), keep[:1].clone())
    nar = run(packed_mt[1:1 + N * 4].view(1, N, 4), packed_mask[s:s + N][None], md[:1].clone(), keep[:1].clone())
    _same_all(nar, one, f"MatchLoss M={M} N={N}: P = 1 on narrows of packed matches and mask")


# ---- the pair families --------------------------------------------------------------------------------------------------------
def _homography_data(P, M, N, gen):
    H = torch.eye(3, dtype=F64) + 0.05 * torch.randn(P, 3, 3, generator=gen, dtype=F64)
    x1 = torch.rand(P, N, 2, generator=gen, dtype=F64) * 2 - 1
    y = torch.cat((x1, torch.ones(P, N, 1, dtype=F64)), -1) @ H.transpose(1, 2)
    x2 = y[..., :2] / y[..., 2:] + 1e-3 * torch.randn(P, N, 2, generator=gen, dtype=F64)
    x2[:, ::3] = torch.rand(P, (N + 2) // 3, 2, generator=gen, dtype=F64) * 2 - 1          # outliers
    models = H[:, None] + 1e-2 * torch.randn(P, M, 3, 3, generator=gen, dtype=F64) * (torch.arange(M) % 4)[None, :, None, None]
    return torch.cat((x1, x2), -1).float(), models.float()


def _pose(P, M, gen, spread):
    w = 0.2 * torch.randn(P, M, 3, generator=gen, dtype=F64) * spread
    K = torch.zeros(P, M, 3, 3, dtype=F64)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -w[..., 2], w[..., 1], -w[..., 0]
    K = K - K.transpose(-1, -2)
    T = torch.eye(4, dtype=F64).repeat(P, M, 1, 1)
    T[..., :3, :3] = torch.matrix_exp(K)
    T[..., :3, 3] = 0.1 * torch.randn(P, M, 3, generator=gen, dtype=F64) * spread
    return T


def _registration_data(P, M, N, gen):
    T = _pose(P, 1, gen, 1.0)
    p = torch.rand(P, N, 3, generator=gen, dtype=F64) * 2 - 1
    q = p @ T[:, 0, :3, :3].transpose(1, 2) + T[:, 0, None, :3, 3] + 5e-3 * torch.randn(P, N, 3, generator=gen, dtype=F64)
    q[:, ::3] = torch.rand(P, (N + 2) // 3, 3, generator=gen, dtype=F64) * 2 - 1
    models = T.repeat(1, M, 1, 1)
    models[..., :3, :] += 5e-3 * torch.randn(P, M, 3, 4, generator=gen, dtype=F64) * (torch.arange(M) % 4)[None, :, None, None]
    return torch.cat((p, q), -1).float(), models.float()


def _pnp_data(P, M, N, gen):
    T = _pose(P, 1, gen, 1.0)
    T[..., 2, 3] += 4.0
    X = torch.rand(P, N, 3, generator=gen, dtype=F64) * 2 - 1
    c = X @ T[:, 0, :3, :3].transpose(1, 2) + T[:, 0, None, :3, 3]
    uv = c[..., :2] / c[..., 2:] + 1e-3 * torch.randn(P, N, 2, generator=gen, dtype=F64)
    uv[:, ::3] = torch.rand(P, (N + 2) // 3, 2, generator=gen, dtype=F64) - 0.5
    models = T.repeat(1, M, 1, 1)
    models[..., :3, 3] += 5e-3 * torch.randn(P, M, 3, generator=gen, dtype=F64) * (torch.arange(M) % 4)[None, :, None]
    return torch.cat((X, uv), -1).float(), models.float()


def _family(name):
    from differentiable_ransac_amd import ops
    if name == "homography":
        return dict(data=_homography_data, thr=0.01, score=ops.homography_score, soft=ops.homography_soft_score,
                    loss=ops.homography_loss_mean, refit=lambda m, k, w, md: ops.refit_homography(m, k, w),
                    weighted=lambda m, w, k, md: ops.weighted_homography(m, w, k))
    if name == "registration":
        return dict(data=_registration_data, thr=0.05, score=ops.rigid_msac_score, soft=ops.registration_soft_score,
                    loss=ops.registration_loss_mean, refit=lambda m, k, w, md: ops.refit_rigid(m, k, w),
                    weighted=lambda m, w, k, md: ops.weighted_kabsch(m, w, k))
    if name == "pnp":
        return dict(data=_pnp_data, thr=0.01, score=ops.pnp_score, soft=ops.pnp_soft_score, loss=ops.pnp_loss_mean,
                    refit=lambda m, k, w, md: ops.refit_pnp(m, k, md[:, 0].contiguous()),
                    weighted=lambda m, w, k, md: ops.weighted_pnp(m, w, md[:, 0].contiguous(), k))
    return dict(data=_homography_data, thr=0.01, score=None, soft=None, loss=None,
                refit=lambda m, k, w, md: ops.refit_fundamental(m, k, w), weighted=lambda m, w, k, md: ops.weighted_fundamental(m, w, k))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["homography", "registration", "pnp", "fundamental"])
def test_pair_family_views(dev, name):
    fam = _family(name)
    P, M, N = 2, 9, 37
    gen = torch.Generator().manual_seed(len(name))
    mt, md = (t.to(dev) for t in fam["data"](P, M, N, gen))
    mask = (torch.rand(P, N, generator=gen) < 0.8).to(dev)
    keep = (torch.rand(P, M, generator=gen) < 0.8).to(dev)
    wts = (torch.rand(P, N, generator=gen) + 0.1).to(dev)

    def grads(fn, *leaves):
        """value(s) and the gradients with respect to the leaves"""
        for t in leaves:
            t.requires_grad_(True)
            t.grad = None
        y = fn()
        y0 = y[0] if isinstance(y, tuple) else y
        (y0 * torch.arange(1, y0.numel() + 1, device=y0.device, dtype=y0.dtype).reshape(y0.shape)).sum().backward()
        out = [t.detach() for t in (y if isinstance(y, tuple) else (y,))] + [t.grad for t in leaves]
        for t in leaves:
            t.requires_grad_(False)
        return out

    def run(m, d, k, kp, w):
        out = {}
        if fam["score"] is not None:
            out["score"] = fam["score"](m, d, fam["thr"], valid=kp)
            out["soft"] = grads(lambda: fam["soft"](m, d, fam["thr"], 5.0, k, kp), d)
            out["loss"] = grads(lambda: fam["loss"](m, k, d, fam["thr"], kp), d)
        out["refit"] = fam["refit"](m, k, w, d)
        out["weighted"] = grads(lambda: fam["weighted"](m, w, k, d), w)
        return out

    ref = run(mt.clone(), md.clone(), mask.clone(), keep.clone(), wts.clone())
    assert bool(ref["refit"][1].all()), f"{name}: the refit of the aligned run must be valid for the comparison to mean anything"
    for mo, do, ko, kpo, wo in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 1, 0), (0, 0, 0, 0, 1), (1, 1, 1, 1, 1), (2, 0, 0, 0, 0)):
        what = f"{name}: matches at {mo}, models at {do}, mask at {ko}, keep at {kpo}, weights at {wo}"
        views = _Views(what)
        r = run(views(mt, mo), views(md, do), views(mask, ko), views(keep, kpo), views(wts, wo))
        _same_all(r, ref, what)
        views.check()


# ---- the test-mode drivers on narrows of packed buffers ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nister", "homography", "registration"])
def test_drivers_on_narrows_of_packed_buffers(dev, name):
    from differentiable_ransac_amd.ransac import BatchedHomography, BatchedRANSAC, BatchedRegistration
    N, s = 132, 7
    gen = torch.Generator().manual_seed(5)
    if name == "nister":
        from differentiable_ransac_amd import synth
        pair = synth.two_view_pair(3, N)
        mt, lg = pair["matches"][None].to(dev), pair["logits"][None].to(dev)
        make = lambda: BatchedRANSAC("nister", ransac_batch_size=64, max_iterations=128, threshold=1e-3, seed=3, keep_masks=False)
    elif name == "homography":
        mt = _homography_data(1, 1, N, gen)[0].to(dev)
        lg = torch.randn(1, N, generator=gen).to(dev)
        make = lambda: BatchedHomography(ransac_batch_size=64, max_iterations=128, threshold=0.01, seed=3)
    else:
        mt = _registration_data(1, 1, N, gen)[0].to(dev)
        lg = torch.randn(1, N, generator=gen).to(dev)
        make = lambda: BatchedRegistration(ransac_batch_size=64, max_iterations=128, threshold=0.05, seed=3)
    c = mt.shape[-1]
    packed_lg = torch.full((s + N + 9,), float("nan"), device=dev)
    packed_lg[s:s + N] = lg[0]
    packed_mt = torch.full((1 + N * c + 7,), float("nan"), device=dev)
    packed_mt[1:1 + N * c] = mt[0].reshape(-1)
    ref = make()(mt.clone(), lg.clone())
    for what, m, l in (("logits narrowed at an odd element", mt.clone(), packed_lg[s:s + N][None]),
                       ("logits and matches narrowed at odd elements", packed_mt[1:1 + N * c].view(1, N, c), packed_lg[s:s + N][None])):
        assert l.data_ptr() % 16 != 0 and l.is_contiguous()
        out = make()(m, l)
        assert ref.keys() == out.keys()
        for k in ref:
            if torch.is_tensor(ref[k]):
                _same(out[k], ref[k], f"{name} driver, {what}: {k}")
    assert torch.isnan(packed_lg[:s]).all() and torch.isnan(packed_lg[s + N:]).all() and torch.equal(packed_lg[s:s + N], lg[0])
    assert torch.isnan(packed_mt[:1]).all() and torch.isnan(packed_mt[1 + N * c:]).all()
