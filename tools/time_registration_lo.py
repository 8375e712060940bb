"""Times ransac.BatchedRegistration with lo = 0, 1 and 2 on one GPU.

    python tools/time_registration_lo.py [--pairs 32 --points 2000 --batch 1024 --max-iterations 5120 --timeout 300]

Workload: P pairs x N correspondences, f32, scenes like tests/registration_ref.scene (unit-cube points, a random pose, noise 0.02 on
the inliers, outliers uniform in a cube of side 4), once with 15 % and once with 35 % inliers.  lo = 0 runs no local-optimisation
code at all, so it is the driver without this option on the same box.  Every call of a variant starts from the same sampler seed.
Device events around whole segments, a warm-up, the median over the segments, the variants alternating; one JSON line per inlier
share with the time per call and the mean `iterations`, score and inliers of a call.  The process ends itself after --timeout s."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scenes(P, N, share, noise, gen):
    """[P,N,6]: a rotation (QR of a normal matrix, det +1) and a translation of norm 1-2 per pair"""
    q, r = torch.linalg.qr(torch.randn(P, 3, 3, generator=gen))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2))[:, None, :]
    q[:, :, 0] *= torch.sign(torch.linalg.det(q))[:, None]
    t = torch.randn(P, 3, generator=gen)
    t = t / t.norm(dim=1, keepdim=True) * (1.0 + torch.rand(P, 1, generator=gen))
    p = torch.rand(P, N, 3, generator=gen)
    good = p @ q.transpose(1, 2) + t[:, None] + noise * torch.randn(P, N, 3, generator=gen)
    centre = torch.full((1, 1, 3), 0.5) @ q.transpose(1, 2) + t[:, None]
    bad = centre + 4.0 * (torch.rand(P, N, 3, generator=gen) - 0.5)
    inl = torch.rand(P, N, generator=gen).argsort(1) < round(share * N)
    return torch.cat([p, torch.where(inl[..., None], good, bad)], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--max-iterations", type=int, default=5120)
    ap.add_argument("--lo-iters", type=int, default=64)
    ap.add_argument("--segments", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5, help="calls per segment")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    # the tool's own time limit: a watchdog thread that dumps every thread's stack and ends the process (exit status 1)
    faulthandler.dump_traceback_later(a.timeout, exit=True)
    if not torch.cuda.is_available():
        sys.exit("time_registration_lo: no GPU (a timing needs one)")
    from differentiable_ransac_amd.ransac import BatchedRegistration
    dev = torch.device("cuda:0")
    P, N = a.pairs, a.points
    for share in (0.15, 0.35):
        m = scenes(P, N, share, 0.02, torch.Generator().manual_seed(11)).to(dev)
        logits = torch.zeros(P, N, device=dev)

        def call(lo):
            drv = BatchedRegistration(ransac_batch_size=a.batch, threshold=0.05, max_iterations=a.max_iterations, seed=1, lo=lo,
                                      lo_iters=a.lo_iters)
            return drv(m, logits)

        res = dict(workload=f"P={P} N={N} B={a.batch} max_iterations={a.max_iterations} f32", inlier_share=share,
                   segments=a.segments, calls_per_segment=a.steps)
        times = {lo: [] for lo in (0, 1, 2)}
        for lo in times:
            for _ in range(3):
                out = call(lo)
            res[f"lo{lo}_mean_iterations"] = float(out["iterations"].double().mean())
            res[f"lo{lo}_mean_score"] = float(out["score"].double().mean())
            res[f"lo{lo}_mean_inliers"] = float(out["inliers"].double().mean())
            if lo:
                res[f"lo{lo}_mean_fits"] = float(out["lo_refits"].double().mean())
        torch.cuda.synchronize()
        for _ in range(a.segments):
            for lo in times:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.steps):
                    call(lo)
                t1.record()
                t1.synchronize()
                times[lo].append(t0.elapsed_time(t1) / a.steps)
        for lo, v in times.items():
            res[f"lo{lo}_ms"] = statistics.median(v)
            res[f"lo{lo}_ms_min_max"] = [min(v), max(v)]
        print(json.dumps(res), flush=True)
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
