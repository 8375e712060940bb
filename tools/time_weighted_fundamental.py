"""Times the weighted eight-point fit and its backward (ops.weighted_fundamental) on one GPU against what a user would write without them.

    python tools/time_weighted_fundamental.py [--pairs 32 --points 2000 --timeout 300]

P pairs x N points, f32, pixels, 70 % inliers (tests/fundamental_grad_ref.scene's generator), half the rows masked, inliers weighted in
[0.5, 1) and outliers in [0.05, 0.25).  Timed, each on preallocated outputs:
  refit            dr_refit_fundamental
  refit_bwd        dr_refit_fundamental_bwd, both outputs
  refit_bwd_w      dr_refit_fundamental_bwd, the weight gradient only (what a weight head trains on)
  torch_autograd   the same fit in plain torch ops on the device (Hartley transforms of the masked rows, Gram matrix of the weighted
                   epipolar rows, torch.linalg.eigh, denormalise), forward + backward to matches and weights: what a user of the
                   package would write without the kernel.  Its gradient is compared with the kernel's (both against the f64
                   composition, each aligned to its own forward's sign) before anything is timed.
Device events around segments of back-to-back launches, a warm-up, the median [min, max] over the segments, the variants alternating;
one JSON line.  The process ends itself after --timeout s."""
import argparse
import faulthandler
import json
import math
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


def torch_fit(matches, weights, mask):
    """the definition of include/dransac.h in batched torch ops: matches [P,N,4], weights [P,N], mask [P,N] bool -> F [P,3,3] (the sign
    is eigh's)"""
    k = mask.to(matches.dtype)
    R = k.sum(1)
    parts = []
    for img in (matches[..., :2], matches[..., 2:]):
        c = (img * k[..., None]).sum(1) / R[:, None]
        q = (img - c[:, None]) * k[..., None]
        r = math.sqrt(2.0) * R / torch.linalg.norm(q, dim=-1).sum(1)
        parts.append((c, r, torch.cat([q * r[:, None, None], torch.ones_like(q[..., :1])], -1)))
    (c1, r1, p1), (c2, r2, p2) = parts
    A = (weights * k)[..., None] * (p2[..., :, None] * p1[..., None, :]).reshape(*k.shape, 9)
    _, V = torch.linalg.eigh(A.transpose(1, 2) @ A)
    Fn = V[..., 0].reshape(-1, 3, 3)
    o, z = torch.ones_like(r1), torch.zeros_like(r1)
    T1 = torch.stack([r1, z, -r1 * c1[:, 0], z, r1, -r1 * c1[:, 1], z, z, o], -1).reshape(-1, 3, 3)
    T2 = torch.stack([r2, z, -r2 * c2[:, 0], z, r2, -r2 * c2[:, 1], z, z, o], -1).reshape(-1, 3, 3)
    return T2.transpose(1, 2) @ Fn @ T1


def torch_grads(matches, weights, mask, gF):
    """-> (grad_matches, grad_weights, F)"""
    m, w = matches.detach().requires_grad_(True), weights.detach().requires_grad_(True)
    F = torch_fit(m, w, mask)
    (F * gF).sum().backward()
    return m.grad, w.grad, F.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--segments", type=int, default=9)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.timeout, exit=True)
    if not torch.cuda.is_available():
        sys.exit("time_weighted_fundamental: no GPU (a timing needs one)")
    from differentiable_ransac_amd import _lib as L
    from tests import fundamental_grad_ref as R
    dev, dt = torch.device("cuda:0"), torch.float32
    P, N = a.pairs, a.points
    ptr, stream = L.ptr, L.stream
    sc = [R.scene(8000 + p, N) for p in range(P)]
    rng = np.random.default_rng(5)
    g = torch.Generator().manual_seed(5)
    m = torch.from_numpy(np.stack([s["matches"] for s in sc])).to(dev, dt)
    w = torch.from_numpy(np.stack([R.scene_weights(s["inliers"], rng) for s in sc])).to(dev, dt)
    mask = (torch.rand(P, N, generator=g) < 0.5).to(dev)
    gF = torch.randn(P, 3, 3, generator=g).to(dev, dt)
    mk = mask.view(torch.uint8)
    new = lambda *shape: torch.empty(shape, device=dev, dtype=dt)
    model, gm, gw, gw_only = new(P, 3, 3), new(P, N, 4), new(P, N), new(P, N)
    valid = torch.empty(P, device=dev, dtype=torch.bool)

    def refit():
        L.call("dr_refit_fundamental_f32", ptr(m), ptr(mk), ptr(w), P, N, ptr(model), ptr(valid), stream())

    def refit_bwd():
        L.call("dr_refit_fundamental_bwd_f32", ptr(m), ptr(mk), ptr(w), ptr(gF), P, N, ptr(gm), ptr(gw), stream())

    def refit_bwd_w():
        L.call("dr_refit_fundamental_bwd_f32", ptr(m), ptr(mk), ptr(w), ptr(gF), P, N, ptr(None), ptr(gw_only), stream())

    def torch_autograd():
        torch_grads(m, w, mask, gF)

    variants = {"refit": (refit, a.launches), "refit_bwd": (refit_bwd, a.launches), "refit_bwd_w": (refit_bwd_w, a.launches),
                "torch_autograd": (torch_autograd, 5)}
    refit()
    refit_bwd()
    refit_bwd_w()
    torch.cuda.synchronize()
    agreement = dict(valid=int(valid.sum()), weights_only_bit_equal=bool(torch.equal(gw, gw_only)))
    # ---- the torch composition computes the same thing: both f32 gradients against the f64 composition on the same f32 inputs, each
    # aligned to the sign of the F its own forward returned
    d_gm, d_gw, d_F = torch_grads(m.double(), w.double(), mask, gF.double())
    t_gm, t_gw, t_F = torch_grads(m, w, mask, gF)
    sign = lambda F: torch.sign((F.double() * d_F).sum((1, 2)))
    rel = lambda got, s, ref: float(((got.double() * s[:, None] - ref).abs().amax(1) / ref.abs().amax(1)).max())
    ks, ts = sign(model), sign(t_F)
    agreement.update(kernel_gm_rel_error_vs_f64=rel(gm.reshape(P, -1), ks, d_gm.reshape(P, -1)), kernel_gw_rel_error_vs_f64=rel(gw, ks, d_gw),
                     torch_f32_gm_rel_error_vs_f64=rel(t_gm.reshape(P, -1), ts, d_gm.reshape(P, -1)),
                     torch_f32_gw_rel_error_vs_f64=rel(t_gw, ts, d_gw))
    res = summary(timed(variants, a.segments))
    print(json.dumps(dict(workload=f"P={P} N={N} f32, {float(mask.float().mean()):.2f} of the rows masked in, inliers weighted in [0.5, 1), "
                                   "outliers in [0.05, 0.25)",
                          segments=a.segments, launches_per_segment=a.launches, agreement=agreement, **res,
                          torch_over_refit_plus_bwd=round(res["torch_autograd"]["median_us"] / (res["refit"]["median_us"] + res["refit_bwd"]["median_us"]), 1))),
          flush=True)
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
