"""Times the kernels of loss.HomographyLoss on one GPU against what a user would write without them.

    python tools/time_homography_loss.py [--pairs 32 --models 5120 --points 2000 --share 0.6 --chunk 256 --timeout 300]

P pairs x M models x N points, f32, `share` of the points in the ground-truth mask; the models are the closed-form solver's for
uniform four-point samples (keep = their validity), the scenes tests/homography_ref.scene's.  Timed, each on preallocated outputs:
  fused       dr_homography_loss_fused   (value + unscaled gradient, then the per-pair / mean reduction: two launches)
  value_only  dr_homography_loss_fwd
  scale       dr_homography_loss_scale   (the whole backward)
against two baselines:
  torch_autograd       the same definition in plain torch ops with autograd (forward + backward to the models), in chunks of
                       --chunk models so that the [P, chunk, N] intermediates fit: what a user of the package would write without the
                       kernel.  Its value and gradient are compared with the kernel's before anything is timed.
  registration_fused   dr_registration_loss_fused at the same P, M, N and mask: the same mapping on a 12-parameter model and a
                       3-vector residual, as a yardstick.
Device events around segments of back-to-back launches, a warm-up, the median [min, max] over the segments, the variants alternating;
one JSON line.  The process ends itself after --timeout s."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(variants, segments):
    """{name: (fn, launches per segment)} -> {name: [us per launch, one per segment]}, the variants alternating"""
    out = {k: [] for k in variants}
    for fn, launches in variants.values():
        for _ in range(min(10, launches)):
            fn()
    torch.cuda.synchronize()
    for _ in range(segments):
        for k, (fn, launches) in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(launches):
                fn()
            t1.record()
            t1.synchronize()
            out[k].append(1e3 * t0.elapsed_time(t1) / launches)
    return out


def summary(times):
    return {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in times.items()}


def torch_loss_and_grad(matches, mask, models, keep, thr2, chunk):
    """the definition of include/dransac.h in torch ops, differentiated by autograd, `chunk` models at a time -> (loss, grad [P,M,3,3])"""
    P, M = models.shape[:2]
    one = torch.ones_like(matches[..., :1])
    X1, X2 = torch.cat([matches[..., :2], one], -1), torch.cat([matches[..., 2:], one], -1)
    den = (keep.sum(1) * mask.sum(1)).clamp(min=1).to(matches.dtype)
    t2 = thr2[:, None, None]
    loss, grads = torch.zeros((), device=matches.device, dtype=matches.dtype), []
    for c0 in range(0, M, chunk):
        H = models[:, c0:c0 + chunk].detach().requires_grad_(True)
        h = H * torch.where(torch.linalg.det(H) < 0, -1.0, 1.0)[..., None, None]
        a = torch.stack([torch.linalg.cross(H[..., 1], H[..., 2]), torch.linalg.cross(H[..., 2], H[..., 0]),
                         torch.linalg.cross(H[..., 0], H[..., 1])], -2)      # rows of adj(H) = cross products of H's columns
        y, z = torch.einsum("pmij,pnj->pmni", h, X1), torch.einsum("pmij,pnj->pmni", a, X2)
        e = matches[:, None, :, 2:] - y[..., :2] / y[..., 2:]
        f = matches[:, None, :, :2] - z[..., :2] / z[..., 2:]
        d2 = (e * e).sum(-1) + (f * f).sum(-1)
        live = (y[..., 2] > 0) & (z[..., 2] > 0) & (d2 < t2)
        term = torch.where(live, d2 / t2, torch.ones_like(d2))
        sums = (term * mask[:, None, :]).sum(-1) * keep[:, c0:c0 + chunk]
        part = (sums.sum(1) / den).mean()
        part.backward()
        loss = loss + part.detach()
        grads.append(H.grad)
    return loss, torch.cat(grads, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--models", type=int, default=5120)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--share", type=float, default=0.6)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--segments", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.timeout, exit=True)
    if not torch.cuda.is_available():
        sys.exit("time_homography_loss: no GPU (a timing needs one)")
    from differentiable_ransac_amd import _lib as L
    from differentiable_ransac_amd import ops
    from tests import homography_ref as R
    dev, dt = torch.device("cuda:0"), torch.float32
    P, M, N = a.pairs, a.models, a.points
    ptr, stream = L.ptr, L.stream
    sc = [R.scene(7000 + p, N, a.share) for p in range(P)]
    m = torch.from_numpy(np.stack([s["matches"] for s in sc])).to(dev, dt)
    mask = torch.from_numpy(np.stack([s["inlier"] for s in sc])).to(dev)
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, N, (P, M, 4), generator=g).to(dev, torch.int32)      # (a repeated index gives an invalid sample: keep = 0)
    models, keep = ops.homography4_gather(m, idx)
    thr2 = ops.thr2_tensor(R.THRESHOLD, P, m)
    new = lambda *shape: torch.empty(shape, device=dev, dtype=dt)
    sums, gun, gm, per_pair, coef, mean = new(P, M), new(P, M, 3, 3), new(P, M, 3, 3), new(P), new(P), new(1)
    up = torch.ones(1, device=dev, dtype=dt)
    mk, kp = mask.view(torch.uint8), keep.view(torch.uint8)

    def fused():
        L.call("dr_homography_loss_fused_f32", ptr(m), ptr(mk), ptr(models), ptr(kp), ptr(thr2), P, M, N, ptr(sums), ptr(gun),
               ptr(per_pair), ptr(coef), ptr(mean), stream())

    def value_only():
        L.call("dr_homography_loss_fwd_f32", ptr(m), ptr(mk), ptr(models), ptr(kp), ptr(thr2), P, M, N, ptr(sums), ptr(per_pair),
               ptr(coef), ptr(mean), stream())

    def scale():
        L.call("dr_homography_loss_scale_f32", ptr(gun), ptr(coef), ptr(up), P, M, ptr(gm), stream())

    # the registration loss at the same shape: random poses near the identity on random points, the same mask and keep
    m6 = torch.randn(P, N, 6, generator=g).to(dev, dt)
    poses = torch.eye(4).repeat(P, M, 1, 1)
    poses[..., :3, 3] = 0.05 * torch.randn(P, M, 3, generator=g)
    poses = poses.to(dev, dt)
    m6[..., 3:] = m6[..., :3] + 0.02 * torch.randn(P, N, 3, generator=g).to(dev, dt)
    r_thr2 = ops.thr2_tensor(0.1, P, m6)
    r_sums, r_gun = new(P, M), new(P, M, 4, 4)

    def registration_fused():
        L.call("dr_registration_loss_fused_f32", ptr(m6), ptr(mk), ptr(poses), ptr(kp), ptr(r_thr2), P, M, N, ptr(r_sums), ptr(r_gun),
               ptr(per_pair), ptr(coef), ptr(mean), stream())

    # ---- the torch composition computes the same thing
    fused()
    scale()
    t_loss, t_grad = torch_loss_and_grad(m, mask, models, keep, thr2, a.chunk)
    torch.cuda.synchronize()
    # (autograd returns NaN for a model with a point of y_w or z_w = 0 or an overflowing d2 -- 0 x inf behind torch.where -- where the
    # kernel passes 0: such models are counted, the others compared)
    # The f32 composition is no reference for the gradient (its own cancellation error is the kernel's and more): the first chunk of
    # models is evaluated once more in f64 torch on the same f32 inputs, and both f32 gradients are measured against that per model
    finite = torch.isfinite(t_grad).all(-1).all(-1)
    c = min(a.chunk, M)
    _, d_grad = torch_loss_and_grad(m.double(), mask, models[:, :c].double(), keep[:, :c], thr2.double(), c)
    den_chunk = (keep[:, :c].sum(1) * mask.sum(1)).clamp(min=1).double()      # (the chunk alone has its own #kept: rescale to the batch's)
    den_all = (keep.sum(1) * mask.sum(1)).clamp(min=1).double()
    d_grad = d_grad * (den_chunk / den_all)[:, None, None, None]
    ok = torch.isfinite(d_grad).all(-1).all(-1) & finite[:, :c] & (d_grad.abs().amax((-1, -2)) > 0)

    def rel(gr):
        r = ((gr[:, :c].double() - d_grad).abs().amax((-1, -2)) / d_grad.abs().amax((-1, -2)))[ok]
        return dict(median=float(r.median()), p99=float(r.quantile(0.99)), max=float(r.max()))
    agreement = dict(loss_kernel=float(mean), loss_torch=float(t_loss), models_with_a_non_finite_torch_gradient=int((~finite).sum()),
                     models_compared_with_f64=int(ok.sum()), kernel_gradient_rel_error_vs_f64=rel(gm), torch_f32_gradient_rel_error_vs_f64=rel(t_grad),
                     live_share=float(1.0 - (sums.sum() / (keep.sum() * mask.sum(1).double().mean())).item()))

    def torch_autograd():
        torch_loss_and_grad(m, mask, models, keep, thr2, a.chunk)

    variants = {"fused": (fused, a.launches), "value_only": (value_only, a.launches), "scale": (scale, a.launches),
                "registration_fused": (registration_fused, a.launches), "torch_autograd": (torch_autograd, 2)}
    res = summary(timed(variants, a.segments))
    ours = res["fused"]["median_us"] + res["scale"]["median_us"]
    print(json.dumps(dict(workload=f"P={P} M={M} N={N} f32, {float(mask.float().mean()):.2f} of the points masked, "
                                   f"{float(keep.float().mean()):.3f} of the slots kept, torch in chunks of {a.chunk} models",
                          segments=a.segments, launches_per_segment=a.launches, agreement=agreement, **res,
                          fused_plus_scale_us=round(ours, 2), torch_over_fused_plus_scale=round(res["torch_autograd"]["median_us"] / ours, 1),
                          fused_over_registration_fused=round(res["fused"]["median_us"] / res["registration_fused"]["median_us"], 2))),
          flush=True)
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
