"""Times ops.registration_soft_score (forward and backward) against the same maths composed from torch ops, on one GPU.

    python tools/time_registration_expected.py [--pairs 32 --samples 1024 --rounds 5 --points 2000 --share 0.5 --chunk 256 --timeout 600]

The train shape of loss.RegistrationExpectedLoss: P pairs x M = rounds x B model slots x N points, f32, synth.rigid_pair's scenes with
`share` inliers, the slots and their keep flags from BatchedRegistration(train=True).  Timed with device events around segments of
back-to-back calls after a warm-up, the variants alternating, the median [min, max] over the segments:
  fwd              ops.registration_soft_score                          (dr_registration_soft_score)
  bwd_models       its backward, matches without a gradient             (dr_registration_soft_score_bwd, one launch)
  bwd_both         its backward to models and matches                   (dr_registration_soft_score_bwd, two launches)
  loss_step        loss.RegistrationExpectedLoss forward + backward on these hypotheses (the op, the soft-max and the pose errors in torch)
  torch_fwd        the definition composed from torch ops on the same device, in chunks of --chunk slots so that the [P,chunk,N]
                   intermediates fit in memory
  torch_fwd_bwd    the composition's forward and autograd backward to models and matches, chunk by chunk
The parent of the commit that added the op has no such path: the composition, on the same machine in the same run, is the only
baseline there is, and no ratio is fixed in advance.  One JSON line, with the largest difference between the two forwards.  The process
ends itself after --timeout s."""
import argparse
import faulthandler
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.time_pnp import summary, timed  # noqa: E402

CUTOFF = -40.0


def torch_scores(m, models, keep, thr2, beta):
    """the definition on one chunk of slots: m [P,N,6], models [P,C,4,4], keep [P,C] -> scores [P,C]"""
    use = keep & torch.isfinite(models[:, :, :3]).all(-1).all(-1)
    safe = torch.where(use[:, :, None, None], models, torch.zeros_like(models))
    d = torch.einsum("pmij,pnj->pmni", safe[:, :, :3, :3], m[:, :, :3]) + safe[:, :, None, :3, 3] - m[:, None, :, 3:]
    d2 = (d * d).sum(-1)
    a = beta * (1.0 - d2 / thr2[:, None, None])
    live = torch.isfinite(d2) & (a >= CUTOFF) & use[:, :, None]
    return torch.where(live, torch.sigmoid(a.clamp(min=CUTOFF)), torch.zeros_like(a)).sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--share", type=float, default=0.5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--segments", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.timeout, exit=True)
    if not torch.cuda.is_available():
        sys.exit("time_registration_expected: no GPU (a timing needs one)")
    from differentiable_ransac_amd import ops, synth
    from differentiable_ransac_amd.loss import RegistrationExpectedLoss
    from differentiable_ransac_amd.ransac import BatchedRegistration
    dev, dt = torch.device("cuda:0"), torch.float32
    P, B, N, beta, thr = a.pairs, a.samples, a.points, 5.0, a.threshold
    sc = [synth.rigid_pair(9000 + p, N, a.share, dtype=dt) for p in range(P)]
    m = torch.stack([s["matches"] for s in sc]).to(dev)
    gt = torch.stack([s["gt_T"] for s in sc]).to(dev)
    logits = torch.stack([s["logits"] for s in sc]).to(dev)
    with torch.no_grad():
        out = BatchedRegistration(ransac_batch_size=B, threshold=thr, max_iterations=a.rounds * B, train=True)(m, logits)
    models, keep = out["models"].contiguous(), out["keep"].contiguous()
    M = models.shape[1]
    thr2 = ops.thr2_tensor(thr, P, m)
    g_up = torch.randn(P, M, device=dev, dtype=dt)

    mo_g, m_g = models.clone().requires_grad_(True), m.clone().requires_grad_(True)
    s_models = ops.registration_soft_score(m, mo_g, thr, beta, None, keep)
    s_both = ops.registration_soft_score(m_g, mo_g, thr, beta, None, keep)
    crit = RegistrationExpectedLoss(thr, beta)

    def loss_step():
        mo_g.grad = m_g.grad = None
        crit(mo_g, m_g, gt, keep=keep).backward()

    def torch_fwd():
        with torch.no_grad():
            return torch.cat([torch_scores(m, models[:, c:c + a.chunk], keep[:, c:c + a.chunk], thr2, beta) for c in range(0, M, a.chunk)], 1)

    def torch_fwd_bwd():
        mo_g.grad = m_g.grad = None
        for c in range(0, M, a.chunk):
            s = torch_scores(m_g, mo_g[:, c:c + a.chunk], keep[:, c:c + a.chunk], thr2, beta)
            s.backward(g_up[:, c:c + a.chunk])

    diff = float((torch_fwd() - s_models.detach()).abs().max())
    variants = {"fwd": (lambda: ops.registration_soft_score(m, models, thr, beta, None, keep), a.launches),
                "bwd_models": (lambda: torch.autograd.grad(s_models, mo_g, g_up, retain_graph=True), a.launches),
                "bwd_both": (lambda: torch.autograd.grad(s_both, (mo_g, m_g), g_up, retain_graph=True), a.launches),
                "loss_step": (loss_step, a.launches),
                "torch_fwd": (torch_fwd, 1),
                "torch_fwd_bwd": (torch_fwd_bwd, 1)}
    res = summary(timed(variants, a.segments))
    print(json.dumps(dict(workload=f"P={P} M={M} ({a.rounds} rounds x {B}) N={N} f32, {a.share:.2f} inliers, threshold {thr}, "
                                   f"{float(keep.float().mean()):.3f} of the slots kept, beta {beta}; torch composition in chunks of "
                                   f"{a.chunk} slots; largest |fused - torch| score {diff:.3g} of {float(s_models.max()):.4g}",
                          segments=a.segments, launches_per_segment=a.launches, **res)), flush=True)
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
