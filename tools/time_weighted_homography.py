"""Times the weighted DLT and its backward (ops.weighted_homography) on one GPU against what a user would write without them.

    python tools/time_weighted_homography.py [--pairs 32 --points 2000 --other-lib PATH --timeout 300]

P pairs x N points, f32, half the rows masked, random weights in [0.25, 1.25), the scenes tests/homography_ref.scene's.  Timed, each on
preallocated outputs:
  refit            dr_refit_homography of this build
  refit_other_lib  dr_refit_homography of the libdransac.so --other-lib names (built from another commit), in the same process: its
                   model is compared with this build's bit for bit before anything is timed
  refit_bwd        dr_refit_homography_bwd, both outputs
  torch_autograd   the same fit in plain torch ops on the device (Hartley transforms of the masked rows, weighted Gram matrix,
                   torch.linalg.eigh, denormalise, unit norm, det > 0), forward + backward to matches and weights: what a user of the
                   package would write without the kernel.  Its gradient is compared with the kernel's (both against the f64
                   composition) before anything is timed.
Device events around segments of back-to-back launches, a warm-up, the median [min, max] over the segments, the variants alternating;
one JSON line.  The process ends itself after --timeout s."""
import argparse
import ctypes
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
    """the definition of include/dransac.h in batched torch ops: matches [P,N,4], weights [P,N], mask [P,N] bool -> H [P,3,3]"""
    k = mask.to(matches.dtype)
    R = k.sum(1)
    parts = []
    for img in (matches[..., :2], matches[..., 2:]):
        c = (img * k[..., None]).sum(1) / R[:, None]
        q = (img - c[:, None]) * k[..., None]
        s = math.sqrt(2.0) * R / torch.linalg.norm(q, dim=-1).sum(1)
        parts.append((c, s, q * s[:, None, None]))
    (c1, s1, p1), (c2, s2, p2) = parts
    X = torch.cat([p1, torch.ones_like(p1[..., :1])], -1)
    Z = torch.zeros_like(X)
    A = torch.cat([torch.cat([Z, -X, p2[..., 1:2] * X], -1), torch.cat([X, Z, -p2[..., 0:1] * X], -1)], 1)
    wk = (weights * k).repeat(1, 2)
    G = A.transpose(1, 2) @ (wk[..., None] * A)
    _, V = torch.linalg.eigh(G)
    Hn = V[..., 0].reshape(-1, 3, 3)
    o, z = torch.ones_like(s1), torch.zeros_like(s1)
    T1 = torch.stack([s1, z, -s1 * c1[:, 0], z, s1, -s1 * c1[:, 1], z, z, o], -1).reshape(-1, 3, 3)
    T2i = torch.stack([1 / s2, z, c2[:, 0], z, 1 / s2, c2[:, 1], z, z, o], -1).reshape(-1, 3, 3)
    H0 = T2i @ Hn @ T1
    H = H0 / torch.linalg.norm(H0, dim=(-2, -1), keepdim=True)
    return H * torch.sign(torch.linalg.det(H)).detach()[:, None, None]


def torch_grads(matches, weights, mask, gH):
    m, w = matches.detach().requires_grad_(True), weights.detach().requires_grad_(True)
    (torch_fit(m, w, mask) * gH).sum().backward()
    return m.grad, w.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--segments", type=int, default=9)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.timeout, exit=True)
    if not torch.cuda.is_available():
        sys.exit("time_weighted_homography: no GPU (a timing needs one)")
    from differentiable_ransac_amd import _lib as L
    from tests import homography_ref as R
    dev, dt = torch.device("cuda:0"), torch.float32
    P, N = a.pairs, a.points
    ptr, stream = L.ptr, L.stream
    sc = [R.scene(8000 + p, N, 0.7) for p in range(P)]
    g = torch.Generator().manual_seed(5)
    m = torch.from_numpy(np.stack([s["matches"] for s in sc])).to(dev, dt)
    mask = (torch.rand(P, N, generator=g) < 0.5).to(dev)
    w = (0.25 + torch.rand(P, N, generator=g)).to(dev, dt)
    gH = torch.randn(P, 3, 3, generator=g).to(dev, dt)
    mk = mask.view(torch.uint8)
    new = lambda *shape: torch.empty(shape, device=dev, dtype=dt)
    model, gm, gw = new(P, 3, 3), new(P, N, 4), new(P, N)
    valid = torch.empty(P, device=dev, dtype=torch.bool)

    def refit():
        L.call("dr_refit_homography_f32", ptr(m), ptr(mk), ptr(w), P, N, ptr(model), ptr(valid), stream())

    def refit_bwd():
        L.call("dr_refit_homography_bwd_f32", ptr(m), ptr(mk), ptr(w), ptr(gH), P, N, ptr(gm), ptr(gw), stream())

    def torch_autograd():
        torch_grads(m, w, mask, gH)

    variants = {"refit": (refit, a.launches), "refit_bwd": (refit_bwd, a.launches), "torch_autograd": (torch_autograd, 5)}
    refit()
    refit_bwd()
    torch.cuda.synchronize()
    agreement = dict(valid=int(valid.sum()))
    if a.other_lib:
        other = ctypes.CDLL(a.other_lib)
        fn = other.dr_refit_homography_f32
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3
        o_model, o_valid = new(P, 3, 3), torch.empty(P, device=dev, dtype=torch.bool)
        args = (m.data_ptr(), mk.data_ptr(), w.data_ptr(), P, N, o_model.data_ptr(), o_valid.data_ptr())

        def refit_other_lib():
            if fn(*args, torch.cuda.current_stream(dev).cuda_stream) != 0:
                raise RuntimeError("dr_refit_homography_f32 of --other-lib failed")
        refit_other_lib()
        torch.cuda.synchronize()
        agreement["other_lib_model_bit_equal"] = bool(torch.equal(o_model, model) and torch.equal(o_valid, valid))
        variants["refit_other_lib"] = (refit_other_lib, a.launches)
    # ---- the torch composition computes the same thing: both f32 gradients against the f64 composition on the same f32 inputs
    d_gm, d_gw = torch_grads(m.double(), w.double(), mask, gH.double())
    t_gm, t_gw = torch_grads(m, w, mask, gH)
    rel = lambda got, ref: float(((got.double() - ref).abs().amax(1) / ref.abs().amax(1)).max())
    agreement.update(kernel_gm_rel_error_vs_f64=rel(gm.reshape(P, -1), d_gm.reshape(P, -1)), kernel_gw_rel_error_vs_f64=rel(gw, d_gw),
                     torch_f32_gm_rel_error_vs_f64=rel(t_gm.reshape(P, -1), d_gm.reshape(P, -1)), torch_f32_gw_rel_error_vs_f64=rel(t_gw, d_gw))
    res = summary(timed(variants, a.segments))
    print(json.dumps(dict(workload=f"P={P} N={N} f32, {float(mask.float().mean()):.2f} of the rows masked in, weights in [0.25, 1.25)",
                          segments=a.segments, launches_per_segment=a.launches, agreement=agreement, **res,
                          torch_over_refit_plus_bwd=round(res["torch_autograd"]["median_us"] / (res["refit"]["median_us"] + res["refit_bwd"]["median_us"]), 1))),
          flush=True)
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
