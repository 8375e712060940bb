"""Times loss.RegistrationLoss (fused kernel, forward + backward) against the same loss written in torch ops, on one GPU.

    python tools/time_registration_loss.py [--pairs 32 --models 5120 --points 2000 --chunk 256 --timeout 300]

Workload: P pairs x M hypotheses x N points, f32, half of the points ground-truth inliers, models = noisy ground-truth poses.  The
torch version evaluates the definition of include/dransac.h `chunk` models at a time (as ops._match_loss_mean_f64 does, so that its
[P, chunk, N] temporaries fit in memory) and lets autograd do the backward.  Device events around whole segments, a warm-up, the
median over the segments, the two versions alternating; one JSON line.  The process ends itself after --timeout seconds."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_loss(matches, mask, models, thr2, keep, chunk):
    P, N, _ = matches.shape
    M = models.shape[1]
    p, q = matches[..., :3], matches[..., 3:]
    total = torch.zeros((P,), device=matches.device, dtype=matches.dtype)
    for m0 in range(0, M, chunk):
        md = torch.where(keep[:, m0:m0 + chunk, None, None], models[:, m0:m0 + chunk], torch.zeros((), device=models.device, dtype=models.dtype))
        r = torch.einsum("pmij,pnj->pmni", md[..., :3, :3], p) + md[..., None, :3, 3] - q[:, None]
        d2 = (r * r).sum(-1)
        t2 = thr2[:, None, None]
        e = torch.where(d2 < t2, d2 / t2, torch.ones((), device=d2.device, dtype=d2.dtype))
        e = torch.where(mask[:, None, :], e, torch.zeros((), device=e.device, dtype=e.dtype))
        total = total + (e.sum(-1) * keep[:, m0:m0 + chunk]).sum(1)
    den = (mask.sum(1) * keep.sum(1)).clamp(min=1).to(total.dtype)
    return (total / den).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--models", type=int, default=5120)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--segments", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5, help="steps per segment")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    # the tool's own time limit: a watchdog thread that dumps every thread's stack and ends the process (exit status 1) after
    # --timeout seconds, whatever the main thread is blocked in; on a shared GPU run it under `timeout -k 10 <seconds>` as well
    faulthandler.dump_traceback_later(a.timeout, exit=True)
    if not torch.cuda.is_available():
        sys.exit("time_registration_loss: no GPU (a timing needs one)")
    from differentiable_ransac_amd import ops
    from differentiable_ransac_amd.loss import RegistrationLoss
    dev, thr = torch.device("cuda:0"), 0.05
    g = torch.Generator().manual_seed(3)
    P, M, N = a.pairs, a.models, a.points
    # a rotation about z and a shift per pair; half of the points follow it with 5 mm of noise, the others are uniform in a 4 m cube
    ang = torch.rand(P, generator=g) * 6.28
    pose = torch.eye(4).repeat(P, 1, 1)
    pose[:, 0, 0], pose[:, 0, 1], pose[:, 1, 0], pose[:, 1, 1] = ang.cos(), -ang.sin(), ang.sin(), ang.cos()
    pose[:, :3, 3] = torch.randn(P, 3, generator=g)
    pts = torch.rand(P, N, 3, generator=g)
    q = pts @ pose[:, :3, :3].transpose(1, 2) + pose[:, None, :3, 3] + 0.005 * torch.randn(P, N, 3, generator=g)
    out = q.mean(1, keepdim=True) + 4.0 * (torch.rand(P, N, 3, generator=g) - 0.5)
    inl = torch.arange(N)[None, :] % 2 == 0
    matches = torch.cat([pts, torch.where(inl[..., None], q, out)], -1).to(dev)
    models = pose[:, None].repeat(1, M, 1, 1)
    models[:, :, :3, :] += 0.02 * torch.randn(P, M, 3, 4, generator=g)
    models = models.to(dev).requires_grad_(True)
    keep = (torch.rand(P, M, generator=g) < 0.95).to(dev)
    pose = pose.to(dev)
    mask, count = ops.registration_gt_mask(matches, pose, thr)
    thr2 = ops.thr2_tensor(thr, P, matches)
    crit = RegistrationLoss(thr)

    def fused():
        models.grad = None
        loss = crit(models, matches, gt_mask=mask, keep=keep)
        loss.backward()
        return loss

    def plain():
        models.grad = None
        loss = torch_loss(matches, mask, models, thr2, keep, a.chunk)
        loss.backward()
        return loss

    lf, gf = fused().item(), models.grad.clone()
    lp, gp = plain().item(), models.grad.clone()
    agree = dict(loss_fused=lf, loss_torch=lp, grad_max_abs_diff=float((gf - gp).abs().max()), grad_max_abs=float(gp.abs().max()))
    times = {"fused": [], "torch": []}
    for fn in (fused, plain):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.segments):
        for name, fn in (("fused", fused), ("torch", plain)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / a.steps)
    res = dict(workload=f"P={P} M={M} N={N} f32 forward+backward", masked_share=float(count.sum()) / (P * N), chunk=a.chunk,
               fused_ms=statistics.median(times["fused"]), torch_ms=statistics.median(times["torch"]),
               fused_ms_min_max=[min(times["fused"]), max(times["fused"])], torch_ms_min_max=[min(times["torch"]), max(times["torch"])],
               segments=a.segments, steps_per_segment=a.steps, **agree)
    res["speedup"] = res["torch_ms"] / res["fused_ms"]
    print(json.dumps(res))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
