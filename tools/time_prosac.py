"""Times the PROSAC sampler launch (ops.prosac_sample) against the index-only Gumbel top-k launch (ops.gumbel_topk(soft=False)) it
replaces in test mode, the ranking (ops.prosac_rank, once per call), and a whole BatchedRegistration call with either sampling, on one
GPU.

    python tools/time_prosac.py [--segments 7 --timeout 600]

Shapes: (P=32, N=2000, B=1024, k=3 and 5), (P=1 and 32, N=50000, B=2048, k=3); f32, logits N(0,1).  Every launch is captured into a
HIP graph of `reps` repetitions and the replays are timed with device events (tools/time_registration_check.Replayed): nothing but
device work is inside a timed region, and a launch's figure includes the gap to the next node of the graph.  A warm-up replay, then
`segments` timed replays per variant, the variants alternating; medians, with min and max.  The PROSAC launch is timed at t0 = 0 (the
growth regime: binary search, scattered reads of the order) and at t0 behind the growth regime (the tail).  The whole call: P=32,
N=2000, B=1024, max_iterations = 5 B with device_termination (every round issued, no read-back: both samplings run five rounds),
scenes of tools/time_registration_lo.py at 0.1 inliers, MSAC, refit.  One JSON line per shape.  The process ends itself after
--timeout s."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.time_registration_check import Replayed  # noqa: E402
from tools.time_registration_lo import scenes  # noqa: E402


def _timed(variants, segments):
    times = {n: [] for n in variants}
    for _ in range(segments):
        for n, g in variants.items():
            times[n].append(g.ms() * 1e3)
    out = {}
    for n, t in times.items():
        out[f"{n}_us"] = round(statistics.median(t), 3)
        out[f"{n}_us_min_max"] = [round(min(t), 3), round(max(t), 3)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--timeout", type=int, default=600)
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.timeout, exit=True)
    if not torch.cuda.is_available():
        sys.exit("time_prosac: no GPU (a timing needs one)")
    from differentiable_ransac_amd import ops
    from differentiable_ransac_amd.ransac import BatchedRegistration
    dev = torch.device("cuda:0")
    for P, N, B, k in ((32, 2000, 1024, 3), (32, 2000, 1024, 5), (1, 50000, 2048, 3), (32, 50000, 2048, 3)):
        logits = torch.randn(P, N, generator=torch.Generator().manual_seed(3)).to(dev)
        order = ops.prosac_rank(logits)
        growth = ops.prosac_growth(N, k, 200000, dev)
        tail = int(growth[-1])
        torch.cuda.synchronize()
        variants = dict(prosac_growth_regime=Replayed(lambda: ops.prosac_sample(order, growth, B, k, 1, 0), a.reps),
                        prosac_tail=Replayed(lambda: ops.prosac_sample(order, growth, B, k, 1, tail), a.reps),
                        gumbel_index_only=Replayed(lambda: ops.gumbel_topk(logits, B, k, 1.0, None, 1, soft=False), max(1, a.reps // 10)))
        res = dict(workload=f"P={P} N={N} B={B} k={k} f32", segments=a.segments, reps_per_graph=a.reps)
        res.update(_timed(variants, a.segments))
        # the ranking, eagerly (host clock included: it runs once per call), 20 calls between two events
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(20):
            ops.prosac_rank(logits)
        t1.record()
        t1.synchronize()
        res["rank_eager_us"] = round(t0.elapsed_time(t1) * 50.0, 3)
        print(json.dumps(res), flush=True)
        del variants
    P, N, B = 32, 2000, 1024
    m = scenes(P, N, 0.1, 0.02, torch.Generator().manual_seed(11)).to(dev)
    logits = torch.randn(P, N, generator=torch.Generator().manual_seed(3)).to(dev)
    variants, keep = {}, []
    for samp in ("gumbel", "prosac"):
        drv = BatchedRegistration(ransac_batch_size=B, threshold=0.05, max_iterations=5 * B, sampling=samp)
        drv.device_termination = True
        out = drv(m, logits)
        keep.append(out)
        variants[f"call_{samp}"] = Replayed(lambda drv=drv: drv(m, logits), 4)
    res = dict(workload=f"BatchedRegistration P={P} N={N} B={B} max_iterations={5 * B} device_termination f32", segments=a.segments,
               iterations=[int(o["iterations"].max()) for o in keep], inliers_mean=[float(o["inliers"].float().mean()) for o in keep])
    res.update(_timed(variants, a.segments))
    print(json.dumps(res), flush=True)
    # last, because a failed capture may leave the stream unusable: is the ranking capturable at both row lengths?
    for N in (2000, 50000):
        logits = torch.randn(2, N, generator=torch.Generator().manual_seed(3)).to(dev)
        try:
            g = Replayed(lambda: ops.prosac_rank(logits), 10)
            print(json.dumps(dict(workload=f"prosac_rank P=2 N={N} captured", rank_us=round(g.ms() * 1e3, 3))), flush=True)
        except Exception as e:      # noqa: BLE001 (reported, not hidden: the line says what failed)
            print(json.dumps(dict(workload=f"prosac_rank P=2 N={N} captured", error=str(e)[:200])), flush=True)
            break
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
