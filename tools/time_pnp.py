"""Times one round and one call of ransac.BatchedPnP on one GPU.

    python tools/time_pnp.py [--pairs 32 --samples 1024 --points 2000 --share 0.5 --timeout 300]

P pairs x B samples x N points, f32, tests/pnp_ref.scene's scenes with `share` inliers.  Timed, each with device events around
segments of back-to-back launches after a warm-up, the variants alternating, the median [min, max] over the segments:
  sample      ops.gumbel_topk        (index sets [P,B,3])
  p3p         ops.p3p_gather         (models [P,4B,4,4])
  score       ops.pnp_score          (4 B slots against N points)
  update      ops.pnp_update
  refit       ops.refit_pnp          (10 passes from the generating pose moved by 3 degrees, over the inlier rows)
  round       the four launches of a round back to back
  call        BatchedPnP(...)(matches, logits) with device_termination (every round issued, no read-back): max_iterations = 4 B
--train times the train step in their place (one round: max_iterations = B, so P x 4 B models):
  p3p         ops.p3p on explicit samples [P,B,3,5]   (dr_p3p)
  p3p_bwd     its backward                            (dr_p3p_bwd, one launch)
  loss        ops.pnp_loss_mean on models that require grad (dr_pnp_loss_fused: the grid and the mean reduction)
  loss_bwd    its backward                            (dr_pnp_loss_scale)
  step        BatchedPnP.hypotheses -> loss.PnPLoss(keep) -> backward to the logits, the gradient cleared in between
One JSON line.  The process ends itself after --timeout s."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--share", type=float, default=0.5)
    ap.add_argument("--segments", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--train", action="store_true")
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.timeout, exit=True)
    if not torch.cuda.is_available():
        sys.exit("time_pnp: no GPU (a timing needs one)")
    from differentiable_ransac_amd import ops
    from differentiable_ransac_amd.ransac import BatchedPnP
    from tests import pnp_ref as R
    dev, dt = torch.device("cuda:0"), torch.float32
    P, B, N = a.pairs, a.samples, a.points
    sc = [R.scene(9000 + p, N, a.share) for p in range(P)]
    m = torch.from_numpy(np.stack([s["matches"] for s in sc])).to(dev, dt)
    mask = torch.from_numpy(np.stack([s["inlier"] for s in sc])).to(dev)
    rng = np.random.default_rng(1)
    init = torch.from_numpy(np.stack([R.perturbed(s["pose"], rng) for s in sc])).to(dev, dt)
    logits = torch.zeros(P, N, device=dev, dtype=dt)
    if a.train:
        return train(a, ops, BatchedPnP, R, sc, m, mask, logits)
    thr2 = ops.thr2_tensor(R.THRESHOLD, P, m)
    idx = ops.gumbel_topk(logits, B, 3, 1.0, None, 1, soft=False)["idx"]
    models, valid = ops.p3p_gather(m, idx)
    scores, _ = ops.pnp_score(m, models, None, valid, want_inliers=False, thr2=thr2)
    st = ops.PnPState(P, N, 10 ** 9, dev, dt)

    def one_round():
        i = ops.gumbel_topk(logits, B, 3, 1.0, None, 1, soft=False)["idx"]
        mo, va = ops.p3p_gather(m, i)
        s = ops.pnp_score(m, mo, None, va, want_inliers=False, thr2=thr2)[0]
        ops.pnp_update(st, m, mo, va, s, None, B, thr2=thr2)

    drv = BatchedPnP(ransac_batch_size=B, threshold=R.THRESHOLD, max_iterations=4 * B)
    drv.device_termination = True
    out = drv(m, logits)
    found = [int(out["inliers"][p]) / max(1, int(sc[p]["inlier"].sum())) for p in range(P)]
    variants = {"sample": (lambda: ops.gumbel_topk(logits, B, 3, 1.0, None, 1, soft=False), a.launches),
                "p3p": (lambda: ops.p3p_gather(m, idx), a.launches),
                "score": (lambda: ops.pnp_score(m, models, None, valid, want_inliers=False, thr2=thr2), a.launches),
                "update": (lambda: ops.pnp_update(st, m, models, valid, scores, None, B, thr2=thr2), a.launches),
                "refit": (lambda: ops.refit_pnp(m, mask, init, 10), a.launches),
                "round": (one_round, a.launches),
                "call": (lambda: drv(m, logits), 3)}
    res = summary(timed(variants, a.segments))
    print(json.dumps(dict(workload=f"P={P} B={B} (4B={4 * B} slots) N={N} f32, {a.share:.2f} inliers, {float(valid.float().mean()):.3f} of the slots valid; "
                                   f"call = {drv.rounds} rounds + refit, device_termination",
                          segments=a.segments, launches_per_segment=a.launches, inliers_found_over_true_min=round(min(found), 3), **res)),
          flush=True)
    faulthandler.cancel_dump_traceback_later()


def train(a, ops, BatchedPnP, R, sc, m, mask, logits):
    from differentiable_ransac_amd.loss import PnPLoss
    P, B, N = a.pairs, a.samples, a.points
    crit = PnPLoss(R.THRESHOLD)
    drv = BatchedPnP(ransac_batch_size=B, threshold=R.THRESHOLD, max_iterations=B)
    lg = logits.clone().requires_grad_(True)

    def step():
        lg.grad = None
        out = drv.hypotheses(m, lg)
        crit(out["models"], m, gt_mask=mask, keep=out["keep"]).backward()

    step()
    assert bool(torch.isfinite(lg.grad).all()) and float(lg.grad.abs().sum()) > 0.0
    samples = ops.SampleGather.apply(m, logits, B, 3, 1.0, None, 1)[0].detach().requires_grad_(True)
    models, keep = ops.p3p(samples)
    flat, kflat = models.detach().reshape(P, 4 * B, 4, 4).requires_grad_(True), keep.reshape(P, 4 * B)
    g_models = torch.randn_like(models)
    loss = ops.pnp_loss_mean(m, mask, flat, R.THRESHOLD, kflat)
    one = torch.ones_like(loss)
    variants = {"p3p": (lambda: ops.p3p(samples), a.launches),
                "p3p_bwd": (lambda: torch.autograd.grad(models, samples, g_models, retain_graph=True), a.launches),
                "loss": (lambda: ops.pnp_loss_mean(m, mask, flat, R.THRESHOLD, kflat), a.launches),
                "loss_bwd": (lambda: torch.autograd.grad(loss, flat, one, retain_graph=True), a.launches),
                "step": (step, 5)}
    res = summary(timed(variants, a.segments))
    print(json.dumps(dict(workload=f"train step P={P} B={B} (4B={4 * B} models) N={N} f32, {a.share:.2f} inliers masked, "
                                   f"{float(keep.float().mean()):.3f} of the slots valid, loss {float(loss.detach()):.4f}",
                          segments=a.segments, launches_per_segment=a.launches, **res)), flush=True)
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
