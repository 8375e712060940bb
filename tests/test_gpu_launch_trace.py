"""The launches the drivers issue, pinned: every libdransac launch goes through `_lib.call`, so wrapping it records, per
call, the entry point, the stream it went to (ordinal of first appearance within the case: 0, 1, 2) and its integer scalar
arguments (the `int` parameters of the header: P, B, N, k, sub, flags -- no pointers, no seeds).  A fixed list of driver calls on small seeded
synthetic input is compared with tests/golden/driver_launch_trace.json.

The golden file pins what the drivers issued BEFORE the host code of ransac.py / ops.py was deduplicated: it was written by
`python tests/test_gpu_launch_trace.py` (write_golden below) with the ransac.py / ops.py of commit 7cc2d56 in place, and is
re-recorded only by a change that means to alter what a call issues.  Where the length of the host-terminated loop depends
on the data it is fixed by max_iterations and a `sync_every` above the number of rounds, so no trace depends on a read-back."""
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "driver_launch_trace.json")
P, N, B = 3, 256, 32


class _Trace:
    """`with _Trace() as t:` -> t.calls = [[entry, stream ordinal, [c_int values]], ...] of the launches issued inside."""

    def __enter__(self):
        from differentiable_ransac_amd import _lib as L
        self.L, self.orig, self.calls, self.streams = L, L.call, [], {}
        L.call = self._call
        return self

    def _call(self, name, *a):
        s = self.streams.setdefault(a[-1].value, len(self.streams))     # (every wrapper ends its argument list with stream())
        ints = [x for x, t in zip(a, self.L.entries()[name]) if t is self.L.c_int]      # the `int` slots, plain or as c_int
        self.calls.append([name, s, [int(getattr(x, "value", x)) for x in ints]])
        self.orig(name, *a)

    def __exit__(self, *exc):
        self.L.call = self.orig


def _two_view(dev, dtype=torch.float32, pixel=False, pairs=P, points=N):
    from differentiable_ransac_amd import synth
    d = synth.batch_two_view(pairs, points, seed0=40, dtype=dtype, pixel=pixel)
    return {k: v.to(dev) for k, v in d.items()}


def _noise(dev, n, rows=B, dtype=torch.float32):
    from differentiable_ransac_amd import synth
    return [synth.gumbel_noise((P, rows, N), seed=7 + i, dtype=dtype).to(dev) for i in range(n)]


def _batched(dev, solver, *, dtype=torch.float32, devterm=False, gumbels=None, super_hypotheses=False, pairs=P, points=N,
             pipeline=True, device_seeds=True, **kw):
    """one test-mode BatchedRANSAC call: three batches of B unless `kw` says otherwise, every round issued"""
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    kw.setdefault("ransac_batch_size", B)
    kw.setdefault("max_iterations", 3 * B)
    d = _two_view(dev, dtype, pixel=solver in ("f8", "f7"), pairs=pairs, points=points)
    rn = BatchedRANSAC(solver, threshold=0.75, seed=11, **kw)
    rn.super_hypotheses = super_hypotheses
    rn.sync_every = 1000
    rn.pipeline = pipeline
    if devterm:
        rn.device_termination = True
        if gumbels is None and device_seeds:      # (the weighted refit's dense row-0 draw takes a by-value seed)
            rn.device_seeds(dev)
    rn(d["matches"], d["logits"], d["K1"], d["K2"], gumbels=gumbels)


def _train(dev, solver, *, rounds=1, device_seeds=False, dtype=torch.float32, **kw):
    from differentiable_ransac_amd.ransac import BatchedRANSAC
    d = _two_view(dev, dtype, pixel=solver == "f8")
    tr = BatchedRANSAC(solver, ransac_batch_size=B, train=True, max_iterations=rounds * B, seed=5, **kw)
    if device_seeds:
        tr.device_seeds(dev)
    lg = d["logits"].clone().requires_grad_(True)
    chosen, keep = tr(d["matches"], lg, gt_model=d["gt_F" if solver == "f8" else "gt_E"])
    torch.where(keep[..., None, None], chosen, torch.zeros((), device=dev, dtype=dtype)).sum().backward()


def _rigid(dev, train, device_seeds=False, dtype=torch.float32, keep_masks=False):
    from differentiable_ransac_amd import synth
    from differentiable_ransac_amd.ransac import BatchedRANSAC3D
    items = [synth.rigid_pair(60 + p, N, dtype=dtype) for p in range(P)]
    matches = torch.stack([it["matches"] for it in items]).to(dev)
    logits = torch.stack([it["logits"] for it in items]).to(dev)
    rn = BatchedRANSAC3D(ransac_batch_size=B, train=train, max_iterations=2 * B, seed=3, flag=False, keep_masks=keep_masks)
    if device_seeds:
        rn.device_seeds(dev)
    if train:
        logits.requires_grad_(True)
        out = rn(matches, logits)
        (out["residuals"].sum() + out["models"].sum()).backward()
    else:
        rn(matches, logits)


def _dropin(dev):
    """RANSAC.__call__ through the eager fused driver: 256 hypotheses in batches of 64 are ONE device round of four batches"""
    from differentiable_ransac_amd.estimators import EssentialMatrixEstimatorNister
    from differentiable_ransac_amd.ransac import RANSAC
    from differentiable_ransac_amd.samplers import GumbelSoftmaxSampler
    from differentiable_ransac_amd.scorings import MSACScore
    d = _two_view(dev)
    r = RANSAC(EssentialMatrixEstimatorNister("cuda"), GumbelSoftmaxSampler(64, 5, device="cuda"), MSACScore("cuda"), fmat=False,
               train=False, ransac_batch_size=64, sampler_id=2, threshold=0.75, max_iterations=256)
    r.graph = False
    r(d["matches"][0], d["logits"][0], d["K1"][0], d["K2"][0], None)


def _sampler_entries(dev):
    """every sampler entry of ops with a by-value seed and with a device seed (the seed argument pair)"""
    from differentiable_ransac_amd import ops
    d = _two_view(dev)
    long_ = _two_view(dev, pairs=2, points=2304)
    ds = ops.DeviceSeed(9, dev)
    for seed in (12345, None):
        s = (lambda: ds.next()) if seed is None else (lambda: seed)
        ops.gumbel_topk(d["logits"], B, 5, 1.0, None, s(), soft=False)
        ops.gumbel_topk(d["logits"], B, 5, 1.0, None, s())
        ops.gumbel_topk(long_["logits"], 64, 5, 1.0, None, s(), soft=False)
        ops.gumbel_topk_gather(d["matches"], d["logits"], B, 5, 1.0, s())
        ops.gumbel_topk_gather(d["matches"], d["logits"], 2 * B, 5, 1.0, s(), sub=B, race=True)
        ops.topdown_sample(d["logits"], B, 5, s())
        ops.uniform_sample(P, B, 8, N, s(), dev)
        ops.solve_f8_uniform(d["matches"], B, s())
        for fused in (True, False):
            was, ops.FUSED_SAMPLE_GATHER = ops.FUSED_SAMPLE_GATHER, fused
            try:
                lg = d["logits"].clone().requires_grad_(True)
                smp, w, _ = ops.SampleGather.apply(d["matches"], lg, B, 5, 1.0, None, s())
                (smp.sum() + w.sum()).backward()
            finally:
                ops.FUSED_SAMPLE_GATHER = was
    d64 = _two_view(dev, torch.float64)
    ops.topdown_sample(d64["logits"], B, 5, 77)
    lg = d64["logits"].clone().requires_grad_(True)
    smp, w, _ = ops.SampleGather.apply(d64["matches"], lg, B, 5, 1.0, None, 77)
    (smp.sum() + w.sum()).backward()


def _gated_and_losses(dev):
    """the gated entries against a live state, and the MatchLoss / episym autograd nodes, forward and backward"""
    from differentiable_ransac_amd import ops
    d = _two_view(dev)
    st, thr = ops.ransac_init(P, N, 4 * B, 0.75, d["K1"], d["K2"], dev, torch.float32)
    idx, smp = ops.gumbel_topk_gather(d["matches"], d["logits"], B, 5, 1.0, 3, gate=st)
    for which in ("nister", "stewenius"):
        models, valid = ops.solve_essential_gated(smp, which, st)
        ops.msac_score(d["matches"], models.reshape(P, -1, 3, 3), thr, want_masks=False, valid=valid.reshape(P, -1), gate=st)
    ops.solve_essential(smp, None, "nister")
    ops.solve_essential(smp, None, "stewenius")
    ops.solve_nister5(smp, path=1)
    ops.solve_stewenius5(smp, path=2)
    models = models.reshape(P, -1, 3, 3)[:, :40].contiguous()
    keep = valid.reshape(P, -1)[:, :40].contiguous()
    for mask, kp in ((d["inliers"], keep), (None, None)):
        for fused in (True, False):
            was, ops.FUSED_MATCH_LOSS = ops.FUSED_MATCH_LOSS, fused
            try:
                m = models.clone().requires_grad_(True)
                ops.match_loss_mean(d["matches"], mask, m, kp).backward()
            finally:
                ops.FUSED_MATCH_LOSS = was
        with torch.no_grad():
            ops.match_loss_mean(d["matches"], mask, models, kp)
        m = models.clone().requires_grad_(True)
        ops.match_loss_per_pair(d["matches"], mask, m, kp).sum().backward()
        m = models.clone().requires_grad_(True)
        ops.episym_sums(d["matches"], mask, m, kp).sum().backward()


CASES = {
    # the host-terminated, pipelined loop
    "test_nister": lambda dev: _batched(dev, "nister"),
    "test_stewenius": lambda dev: _batched(dev, "stewenius"),
    "test_f8": lambda dev: _batched(dev, "f8"),
    "test_f7": lambda dev: _batched(dev, "f7"),
    "test_nister_unpipelined": lambda dev: _batched(dev, "nister", pipeline=False),
    "test_nister_no_refit": lambda dev: _batched(dev, "nister", refit=False),
    "test_nister_eight_point_samples": lambda dev: _batched(dev, "nister", num_samples=8),
    # every round issued, the stop taken on the device
    "devterm_nister": lambda dev: _batched(dev, "nister", devterm=True),
    "devterm_stewenius": lambda dev: _batched(dev, "stewenius", devterm=True),
    "devterm_f8": lambda dev: _batched(dev, "f8", devterm=True),
    "devterm_one_pair_packed": lambda dev: _batched(dev, "nister", devterm=True, pairs=1),
    "devterm_nister_explicit_noise": lambda dev: _batched(dev, "nister", devterm=True, gumbels=_noise(dev, 3)),
    "devterm_nister_f64": lambda dev: _batched(dev, "nister", devterm=True, dtype=torch.float64),
    # super-rounds: 79 batches of 64 in device rounds of 1024 hypotheses
    "super_rounds": lambda dev: _batched(dev, "nister", ransac_batch_size=64, max_iterations=5000, super_hypotheses=(1024, 1024)),
    "super_rounds_devterm": lambda dev: _batched(dev, "stewenius", devterm=True, ransac_batch_size=64, max_iterations=5000,
                                                 super_hypotheses=(1024, 1024)),
    "super_rounds_f8_automatic": lambda dev: _batched(dev, "f8", ransac_batch_size=64, max_iterations=5000, super_hypotheses=None),
    "super_rounds_explicit_noise": lambda dev: _batched(dev, "nister", gumbels=_noise(dev, 3), super_hypotheses=(64, 64)),
    "super_rounds_explicit_noise_devterm": lambda dev: _batched(dev, "nister", devterm=True, gumbels=_noise(dev, 3),
                                                                super_hypotheses=(64, 64)),
    # the weighted refit's row-0 soft weights, local optimisation, the index-only samplers, explicit noise, masks, f64
    "weighted_f8": lambda dev: _batched(dev, "f8", weighted=1),
    "weighted_f8_devterm": lambda dev: _batched(dev, "f8", weighted=1, devterm=True, device_seeds=False),
    "weighted_f8_explicit_noise": lambda dev: _batched(dev, "f8", weighted=1, gumbels=_noise(dev, 3)),
    "weighted_nister": lambda dev: _batched(dev, "nister", weighted=1),
    "lo2_nister": lambda dev: _batched(dev, "nister", lo=2),
    "lo1_f8_devterm": lambda dev: _batched(dev, "f8", lo=1, devterm=True),
    "uniform_f8": lambda dev: _batched(dev, "f8", sampling="uniform"),
    "uniform_nister": lambda dev: _batched(dev, "nister", sampling="uniform"),
    "topdown_nister": lambda dev: _batched(dev, "nister", sampling="topdown"),
    "explicit_noise_nister": lambda dev: _batched(dev, "nister", gumbels=_noise(dev, 3)),
    "explicit_noise_f7": lambda dev: _batched(dev, "f7", gumbels=_noise(dev, 2)),
    "keep_masks": lambda dev: _batched(dev, "nister", keep_masks=True),
    "f64_nister": lambda dev: _batched(dev, "nister", dtype=torch.float64),
    "f64_f8": lambda dev: _batched(dev, "f8", dtype=torch.float64),
    # 64 pairs x 1024 rows: the one-logarithm sampler's weights out of the set-up launch, the dispatch gap in front of the sampler
    "large_grid": lambda dev: _batched(dev, "nister", pairs=64, points=128, ransac_batch_size=1024, max_iterations=2048),
    "large_grid_devterm": lambda dev: _batched(dev, "nister", devterm=True, pairs=64, points=128, ransac_batch_size=1024,
                                               max_iterations=2048),
    # train mode, forward and backward
    "train_nister": lambda dev: _train(dev, "nister"),
    "train_nister_two_rounds_device_seeds": lambda dev: _train(dev, "nister", rounds=2, device_seeds=True),
    "train_stewenius": lambda dev: _train(dev, "stewenius"),
    "train_f8": lambda dev: _train(dev, "f8"),
    "train_f8_weighted": lambda dev: _train(dev, "f8", weighted=1),
    "train_nister_eight_point_samples": lambda dev: _train(dev, "nister", num_samples=8),
    "train_nister_f64": lambda dev: _train(dev, "nister", dtype=torch.float64),
    # 3-D registration
    "rigid_train": lambda dev: _rigid(dev, True),
    "rigid_test": lambda dev: _rigid(dev, False, keep_masks=True),
    "rigid_test_device_seeds": lambda dev: _rigid(dev, False, device_seeds=True),
    "rigid_test_f64": lambda dev: _rigid(dev, False, dtype=torch.float64),
    # the drop-in class, and the ops entries whose argument lists carry a seed or a gate
    "dropin_eager_fused": _dropin,
    "ops_sampler_entries": _sampler_entries,
    "ops_gated_and_losses": _gated_and_losses,
}


def record(dev):
    """{case: [[entry, stream ordinal, [ints]], ...]} for every case of CASES"""
    out = {}
    for name, case in CASES.items():
        torch.cuda.synchronize()
        with _Trace() as t:
            case(dev)
        torch.cuda.synchronize()
        out[name] = t.calls
    return out


def write_golden(path=GOLDEN):
    with open(path, "w") as f:
        json.dump(record(torch.device("cuda:0")), f, separators=(",", ":"))
        f.write("\n")


@pytest.mark.gpu
def test_the_drivers_issue_the_recorded_launches(dev):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = record(dev)
    assert sorted(got) == sorted(want)
    for name in CASES:
        assert got[name] == want[name], name


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_golden(*sys.argv[1:2])
