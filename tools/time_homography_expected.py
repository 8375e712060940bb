"""Times ops.homography_soft_score (forward and backward) against the same maths composed from torch ops and against
ops.registration_soft_score at the same (P, M, N), on one GPU.

    python tools/time_homography_expected.py [--pairs 32 --samples 1024 --rounds 5 --points 2000 --share 0.5 --chunk 128 --timeout 600]

The train shape of loss.HomographyExpectedLoss: P pairs x M = rounds x B model slots x N points, f32, scenes of a 640-pixel square
with `share` inliers under a random homography and 0.5 px of noise, the slots and their keep flags from
BatchedHomography(train=True).  Timed with device events around segments of back-to-back calls after a warm-up, the variants
alternating, the median [min, max] over the segments, all in one process:
  fwd              ops.homography_soft_score                            (dr_homography_soft_score)
  bwd_models       its backward, matches without a gradient             (dr_homography_soft_score_bwd, one launch)
  bwd_both         its backward to models and matches                   (dr_homography_soft_score_bwd, two launches)
  loss_step        loss.HomographyExpectedLoss forward + backward on these hypotheses (the op, the soft-max and the corner errors in torch)
  torch_fwd        the definition composed from f32 torch ops on the same device, in chunks of --chunk slots so that the [P,chunk,N]
                   intermediates fit in memory
  torch_fwd_bwd    the composition's forward and autograd backward to models and matches, chunk by chunk
  rigid_fwd, rigid_bwd_both   ops.registration_soft_score and its backward to models and matches at the same (P, M, N), on rigid
                   scenes (synth.rigid_pair) and BatchedRegistration's slots: the cost of the scaffold's rigid term next to this one
No ratio is fixed in advance.  One JSON line, with the largest difference between the two forwards.  The process ends itself after
--timeout s."""
import argparse
import faulthandler
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.time_pnp import summary, timed  # noqa: E402

CUTOFF = -40.0
SIDE = 640.0


def scene(seed, N, share, dev, dt):
    """matches [N,4] in a 640-pixel square under a random homography (rotation <= 0.4 rad, scale 0.8-1.25, shift <= 40 px and
    perspective terms <= 3e-4 about the centre), `share` inliers with 0.5 px of noise, the others uniform; -> (matches, H)"""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: float(torch.rand((), generator=g, dtype=torch.float64)) * (hi - lo) + lo
    a, s, c = u(-0.4, 0.4), u(0.8, 1.25), 0.5 * SIDE
    S = torch.tensor([[s * math.cos(a), -s * math.sin(a), u(-40, 40)], [s * math.sin(a), s * math.cos(a), u(-40, 40)],
                      [u(-3e-4, 3e-4), u(-3e-4, 3e-4), 1.0]], dtype=torch.float64)
    C = torch.tensor([[1.0, 0.0, c], [0.0, 1.0, c], [0.0, 0.0, 1.0]], dtype=torch.float64)
    H = C @ S @ torch.linalg.inv(C)
    H = H / H.norm()
    x1 = torch.rand(N, 2, generator=g, dtype=torch.float64) * SIDE
    y = torch.cat([x1, torch.ones(N, 1, dtype=torch.float64)], 1) @ H.T
    x2 = y[:, :2] / y[:, 2:] + 0.5 * torch.randn(N, 2, generator=g, dtype=torch.float64)
    out = torch.rand(N, generator=g) >= share
    x2[out] = torch.rand(int(out.sum()), 2, generator=g, dtype=torch.float64) * SIDE
    return torch.cat([x1, x2], 1).to(dt).to(dev), H.to(dt).to(dev)


def torch_scores(m, models, keep, thr2, beta):
    """the definition on one chunk of slots: m [P,N,4], models [P,C,3,3], keep [P,C] -> scores [P,C]"""
    c0, c1, c2 = models[..., :, 0], models[..., :, 1], models[..., :, 2]
    A = torch.stack([torch.linalg.cross(c1, c2), torch.linalg.cross(c2, c0), torch.linalg.cross(c0, c1)], -2)
    det = (models[..., 0, :] * A[..., :, 0]).sum(-1)
    use = keep & torch.isfinite(models).all(-1).all(-1) & torch.isfinite(det) & (det != 0)
    eye = torch.eye(3, device=models.device, dtype=models.dtype)
    h = torch.where(use[:, :, None, None], models * torch.where(det < 0, -1.0, 1.0)[..., None, None], eye)
    A = torch.where(use[:, :, None, None], A, eye)
    one = torch.ones_like(m[..., :1])
    y = torch.einsum("pmij,pnj->pmni", h, torch.cat([m[..., :2], one], -1))
    z = torch.einsum("pmij,pnj->pmni", A, torch.cat([m[..., 2:], one], -1))
    front = (y[..., 2] > 0) & (z[..., 2] > 0)
    yw, zw = torch.where(front, y[..., 2], torch.ones_like(y[..., 2])), torch.where(front, z[..., 2], torch.ones_like(z[..., 2]))
    e, f = m[:, None, :, 2:] - y[..., :2] / yw[..., None], m[:, None, :, :2] - z[..., :2] / zw[..., None]
    d2 = (e * e).sum(-1) + (f * f).sum(-1)
    a = beta * (1.0 - d2 / thr2[:, None, None])
    live = front & torch.isfinite(d2) & (a >= CUTOFF) & use[:, :, None]
    return torch.where(live, torch.sigmoid(a.clamp(min=CUTOFF)), torch.zeros_like(a)).sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--share", type=float, default=0.5)
    ap.add_argument("--threshold", type=float, default=3.0)
    ap.add_argument("--rigid-threshold", type=float, default=0.05)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--segments", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.timeout, exit=True)
    if not torch.cuda.is_available():
        sys.exit("time_homography_expected: no GPU (a timing needs one)")
    from differentiable_ransac_amd import ops, synth
    from differentiable_ransac_amd.loss import HomographyExpectedLoss
    from differentiable_ransac_amd.ransac import BatchedHomography, BatchedRegistration
    dev, dt = torch.device("cuda:0"), torch.float32
    P, B, N, beta, thr = a.pairs, a.samples, a.points, 5.0, a.threshold
    sc = [scene(9000 + p, N, a.share, dev, dt) for p in range(P)]
    m, gt = torch.stack([s[0] for s in sc]), torch.stack([s[1] for s in sc])
    logits = torch.zeros(P, N, device=dev, dtype=dt)
    with torch.no_grad():
        out = BatchedHomography(ransac_batch_size=B, threshold=thr, max_iterations=a.rounds * B, train=True)(m, logits)
    models, keep = out["models"].contiguous(), out["keep"].contiguous()
    M = models.shape[1]
    thr2 = ops.thr2_tensor(thr, P, m)
    g_up = torch.randn(P, M, device=dev, dtype=dt)

    mo_g, m_g = models.clone().requires_grad_(True), m.clone().requires_grad_(True)
    s_models = ops.homography_soft_score(m, mo_g, thr, beta, None, keep)
    s_both = ops.homography_soft_score(m_g, mo_g, thr, beta, None, keep)
    crit = HomographyExpectedLoss(thr, (SIDE, SIDE), beta)

    # the rigid term at the same (P, M, N)
    rs = [synth.rigid_pair(9000 + p, N, a.share, dtype=dt) for p in range(P)]
    rm = torch.stack([s["matches"] for s in rs]).to(dev)
    with torch.no_grad():
        rout = BatchedRegistration(ransac_batch_size=B, threshold=a.rigid_threshold, max_iterations=a.rounds * B, train=True)(
            rm, torch.stack([s["logits"] for s in rs]).to(dev))
    rmodels, rkeep = rout["models"].contiguous(), rout["keep"].contiguous()
    rmo_g, rm_g = rmodels.clone().requires_grad_(True), rm.clone().requires_grad_(True)
    r_both = ops.registration_soft_score(rm_g, rmo_g, a.rigid_threshold, beta, None, rkeep)

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
    variants = {"fwd": (lambda: ops.homography_soft_score(m, models, thr, beta, None, keep), a.launches),
                "bwd_models": (lambda: torch.autograd.grad(s_models, mo_g, g_up, retain_graph=True), a.launches),
                "bwd_both": (lambda: torch.autograd.grad(s_both, (mo_g, m_g), g_up, retain_graph=True), a.launches),
                "loss_step": (loss_step, a.launches),
                "torch_fwd": (torch_fwd, 1),
                "torch_fwd_bwd": (torch_fwd_bwd, 1),
                "rigid_fwd": (lambda: ops.registration_soft_score(rm, rmodels, a.rigid_threshold, beta, None, rkeep), a.launches),
                "rigid_bwd_both": (lambda: torch.autograd.grad(r_both, (rmo_g, rm_g), g_up, retain_graph=True), a.launches)}
    res = summary(timed(variants, a.segments))
    print(json.dumps(dict(workload=f"P={P} M={M} ({a.rounds} rounds x {B}) N={N} f32, {a.share:.2f} inliers, threshold {thr} px, "
                                   f"{float(keep.float().mean()):.3f} of the slots kept ({float(rkeep.float().mean()):.3f} of the rigid "
                                   f"ones), beta {beta}; torch composition in chunks of {a.chunk} slots; largest |fused - torch| score "
                                   f"{diff:.3g} of {float(s_models.max()):.4g}",
                          segments=a.segments, launches_per_segment=a.launches, **res)), flush=True)
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
