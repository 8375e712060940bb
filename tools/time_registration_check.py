"""Times one round of ransac.BatchedRegistration -- sampler, fit of the samples, score, state step -- with and without the rigidity
test of the samples (edge_similarity), and the round's four launches one by one, on one GPU.

    python tools/time_registration_check.py [--pairs 32 --points 2000 50000 --batch 1024 --similarities off 0.9 0.95 --timeout 600]

Workload: P pairs x N correspondences, f32, flat logits, scenes like tools/time_registration_lo.py's (unit-cube points, a random pose,
noise 0.02 on the inliers, outliers uniform in a cube of side 4) at outlier rates 0.5, 0.9 and 0.99.  "off" is dr_kabsch_gather, the
round without the option.  A round and each of its launches are captured into a HIP graph of `reps` repetitions (the same seed, so the
same draws every time) and the replays are timed with device events: nothing but device work is inside a timed region.  A warm-up
replay, then `segments` timed replays per variant, the variants alternating; medians.  The state step is timed on a state that already
holds the round's winner (a replay finds no better model), so its figure is the step without the rewrite of the mask.
Also reported per variant: the share of samples the test drops, the share of the score launch's blocks (a pair x 16 models) whose models are
all invalid, and the time of the score launch with EVERY model invalid -- what a block costs that only loads its points -- from which
`score_ms_in_dead_blocks` = dead share x that time is the part of the score launch spent in blocks with nothing to score.
One JSON line per (N, outlier rate).  The process ends itself after --timeout s."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.time_registration_lo import scenes  # noqa: E402


class Replayed:
    """fn() x reps captured once; ms() = one timed replay / reps"""

    def __init__(self, fn, reps):
        self.reps = reps
        self.graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        with torch.cuda.graph(self.graph):
            for _ in range(reps):
                fn()
        self.graph.replay()
        torch.cuda.synchronize()

    def ms(self):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        self.graph.replay()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / self.reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--points", type=int, nargs="+", default=[2000, 50000])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--outlier-rates", type=float, nargs="+", default=[0.5, 0.9, 0.99])
    ap.add_argument("--similarities", nargs="+", default=["off", "0.9", "0.95"])
    ap.add_argument("--segments", type=int, default=7)
    ap.add_argument("--graph-ms", type=float, default=50.0, help="device time a captured graph should hold: sets its repetitions")
    ap.add_argument("--timeout", type=int, default=600)
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.timeout, exit=True)
    if not torch.cuda.is_available():
        sys.exit("time_registration_check: no GPU (a timing needs one)")
    from differentiable_ransac_amd import _lib, ops
    dev = torch.device("cuda:0")
    P, B = a.pairs, a.batch
    sims = [None if s == "off" else float(s) for s in a.similarities]
    for N in a.points:
        for rate in a.outlier_rates:
            m = scenes(P, N, 1.0 - rate, 0.02, torch.Generator().manual_seed(11)).to(dev)
            logits = torch.zeros(P, N, device=dev)
            thr2 = ops.thr2_tensor(0.05, P, m)
            res = dict(workload=f"P={P} N={N} B={B} f32", outlier_rate=rate, segments=a.segments,
                       library=os.path.basename(_lib.LIB_PATH))
            variants, reps, keep = {}, None, []
            for sim in sims:
                name = "off" if sim is None else f"{sim:g}"
                st = ops.RegistrationState(P, N, 5 * B, dev, m.dtype)
                rejected = torch.zeros(P, device=dev, dtype=torch.int32)

                def sample():
                    return ops.gumbel_topk(logits, B, 3, 1.0, None, 1, soft=False)["idx"]

                def fit(idx, sim=sim, rejected=rejected):
                    return ops.kabsch_gather(m, idx) if sim is None else ops.kabsch_gather_checked(m, idx, sim, rejected)

                def score(models, valid):
                    return ops.rigid_msac_score(m, models, None, valid, want_inliers=False, thr2=thr2)[0]

                def update(models, valid, scores, st=st):
                    ops.registration_update(st, m, models, valid, scores, None, B, thr2=thr2)

                def whole():
                    idx = sample()
                    models, valid = fit(idx)
                    update(models, valid, score(models, valid))

                idx = sample()
                models, valid = fit(idx)
                scores = score(models, valid)
                update(models, valid, scores)
                if reps is None:      # from the first variant's eager round (the unchecked one when "off" comes first), for all of them
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    whole()
                    t1.record()
                    t1.synchronize()
                    reps = res["reps_per_graph"] = max(1, min(200, int(a.graph_ms / t0.elapsed_time(t1))))
                dead = ~valid.reshape(P, -1, 16).any(-1) if B % 16 == 0 else None
                none_valid = torch.zeros_like(valid)
                res[f"{name}_dropped_share"] = 0.0 if sim is None else float(rejected.sum()) / (P * B)
                res[f"{name}_invalid_share"] = 1.0 - float(valid.float().mean())
                if dead is not None:
                    res[f"{name}_dead_block_share"] = float(dead.float().mean())
                variants[name] = dict(round=Replayed(whole, reps), sampler=Replayed(sample, reps),
                                      gather=Replayed(lambda: fit(idx), reps), score=Replayed(lambda: score(models, valid), reps),
                                      update=Replayed(lambda: update(models, valid, scores), reps),
                                      score_all_invalid=Replayed(lambda: score(models, none_valid), reps))
                # a graph replays on the ADDRESSES it captured: the variant's inputs stay alive until its last replay
                keep.append((idx, models, valid, scores, none_valid, st, rejected))
            times = {n: {k: [] for k in v} for n, v in variants.items()}
            for _ in range(a.segments):
                for n, v in variants.items():
                    for k, g in v.items():
                        times[n][k].append(g.ms())
            for n, v in times.items():
                for k, t in v.items():
                    res[f"{n}_{k}_ms"] = round(statistics.median(t), 5)
                res[f"{n}_round_ms_min_max"] = [round(min(v["round"]), 5), round(max(v["round"]), 5)]
                if f"{n}_dead_block_share" in res:
                    res[f"{n}_score_ms_in_dead_blocks"] = round(res[f"{n}_dead_block_share"] * res[f"{n}_score_all_invalid_ms"], 5)
            print(json.dumps(res), flush=True)
            del variants, keep
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
