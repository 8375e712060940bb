"""RANSAC drivers -- same classes, constructor arguments and return values as the reference's
ransac.py (RANSAC :6-299, RANSAC3D :303-450), plus BatchedRANSAC, which runs the same algorithm
over a whole (image-pair x hypothesis) grid in a handful of launches instead of the reference's
per-pair Python loop (model_cl.py:488).

Everything numeric happens in libdransac.so through differentiable_ransac_amd.ops; these classes
only sequence launches and keep the (tiny) per-pair state.
"""
from __future__ import annotations

import collections
import math
import types
from typing import Dict

import torch

from . import ops


def adaptive_iteration_number(inlier_number, point_number, sample_size, confidence=0.999, eps=1e-5,
                              max_iterations=5000):
    """ransac.py:202-215."""
    ratio = float(inlier_number) / float(point_number)
    prob = 1.0 - ratio ** sample_size
    if prob >= 1.0 - eps:
        return max_iterations
    return max(0.0, math.log10(1.0 - confidence) / math.log10(1 - ratio ** sample_size + eps))


def normalized_threshold(threshold, K1, K2, fmat):
    """ransac.py:49-53 -- (K1[0,0] + K1[1,1] + K1[0,0] + K2[1,1]) / 4, K1[0,0] twice on purpose (Q3)."""
    if fmat:
        return threshold
    return threshold / ((K1[..., 0, 0] + K1[..., 1, 1] + K1[..., 0, 0] + K2[..., 1, 1]) / 4)


def _takes_argument(fn) -> bool:
    """True when `fn` (a bound method) accepts one positional argument."""
    import inspect
    try:
        params = [p for p in inspect.signature(fn).parameters.values()
                  if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD, p.VAR_POSITIONAL)]
    except (TypeError, ValueError):
        return False
    return len(params) >= 1


def _check_lo(lo, lo_iters):
    """lo 0 / 1 / 2 (ransac.py:217-257); 3, the inner RANSAC of :258-299, never ran in the reference."""
    if lo == 3:
        raise NotImplementedError("lo=3 (inner RANSAC) is out of scope: it never ran in the reference either (its "
                                  "UniformSampler call raises TypeError, SURVEY Q2)")
    if lo not in (0, 1, 2):
        raise ValueError(f"lo must be 0, 1 (one LSQ refit on the inliers) or 2 (iterated refits), got {lo!r}")
    if int(lo_iters) < 1:
        raise ValueError(f"lo_iters must be at least 1, got {lo_iters!r}")


def _check_scoring(scoring, irls_iters=0):
    """scoring "msac" / "magsac" and irls_iters an int (no bool) of at least 0; BatchedRegistration reads its irls_iters through int()
    and checks it itself (_PairStateDriver.__init__)"""
    if scoring not in ("msac", "magsac"):
        raise ValueError(f"scoring must be 'msac' or 'magsac', got {scoring!r}")
    if isinstance(irls_iters, bool) or not isinstance(irls_iters, int) or irls_iters < 0:
        raise ValueError(f"irls_iters must be an int of at least 0, got {irls_iters!r}")


def _is_gumbel(sampler_id):
    # ids 2 and 3 in the reference; id 1 builds a Gumbel sampler there too but then crashes (Q16): treated as 2
    return sampler_id in (1, 2, 3)


class RANSAC(object):
    """Drop-in for the reference's RANSAC (ransac.py:6-200): __call__(matches [N,4], logits [N], K1, K2, gt_model)
    -> (best_model | {iteration: models}, best_mask, best_score, iterations).

    lo = 1 / 2 (test mode): localOptimization of ransac.py:217-257 after every new best model -- on the device (dr_local_opt)
    in the fused path, host-side with the plugins otherwise.  With lo > 0 every batch is a device round of its own, so a call
    replays as one graph when it is at most 8 rounds (`-rbs 1024` / 5000: 5) and runs the eager fused driver otherwise
    (`-rbs 64`: 79 rounds)."""

    def __init__(self, estimator, sampler, scoring, fmat=False, train=False, ransac_batch_size=64, sampler_id=0,
                 weighted=0, threshold=1e-3, confidence=0.999, max_iterations=5000, lo=0, lo_iters=64, eps=1e-5):
        self.estimator = estimator
        self.sampler = sampler
        self.scoring = scoring
        self.lo = lo
        self.lo_iters = lo_iters
        self.fmat = fmat
        self.train = train
        self.ransac_batch_size = ransac_batch_size
        self.sampler_id = sampler_id
        self.weighted = weighted
        self.threshold = threshold
        self.confidence = confidence
        self.max_iterations = max_iterations
        self.eps = eps
        self._soft0 = None       # y_soft of hypothesis 0 of the last batch (weighted F refit, ransac.py:151-153)
        self.fused = True        # test mode with this package's own plugins: run on the device-resident batched driver
        self.graph = True        # ... and, when a call is at most 8 device rounds, as ONE replayed HIP graph per call (_GraphedCall)
        # hypotheses per device round of the replayed call (BatchedRANSAC.super_hypotheses): the first 2048 hypotheses -- however many
        # batches of `ransac_batch_size` that is -- then everything `max_iterations` still allows in rounds of 4096, walked batch by
        # batch on the device with the loop's own stop rule: `-rbs 64 / 5000` is two device rounds, like `-rbs 1024`.  One pair
        # leaves the chip empty, so a device round of 2048 hypotheses costs 15-20 us more than one of 1024 while a second round
        # costs 70-90: measured per pair at 2000 points, 32 pairs of 36 % inliers (24 of them need a second batch of 1024), ms:
        #   (1024, 1024) 0.210 | (1024, 1024, 4096) 0.189 | (2048, 4096) 0.148 | (2048, 1024, 4096) 0.156 | (3072, 2048) 0.157 |
        #   (5120,) 0.168; with ransac_batch_size = 64: 0.221 | 0.198 | 0.154 | 0.165 | 0.165 | 0.175   (scratch/runs/r6_gpu_e.sh)
        self.graph_hypotheses = (2048, 4096)
        self.max_graphs = 8      # replayed calls kept (one per point count and device), least recently used evicted
        self._fast = None
        self._fast_cfg = None
        self._graphs = collections.OrderedDict()
        if lo not in (0, 1, 2):
            # any other value, not only the 3 _check_lo names, is "not implemented" for the drop-in class (BatchedRANSAC: ValueError)
            raise NotImplementedError(f"lo={lo!r}: only lo=1 (one LSQ refit on the inliers) and lo=2 (iterated refits) are "
                                      "implemented; lo=3 (inner RANSAC) never ran in the reference either (SURVEY Q2)")
        _check_lo(lo, lo_iters)

    def adaptive_iteration_number(self, inlier_number, point_number, confidence):
        """ransac.py:202-215, the reference's method form (sample size, eps and the cap come from the object)."""
        return adaptive_iteration_number(inlier_number, point_number, self.estimator.sample_size, confidence, self.eps,
                                         self.max_iterations)

    def _lo_candidates(self, matches, mask):
        """The LSQ refit of localOptimization (ransac.py:227-242) on the rows `mask` selects -> (models [S,3,3], valid [S] or None),
        or None when there are too few rows.  This package's estimators solve what dr_local_opt solves: F = the unweighted Hartley
        8-point (ops.refit_fundamental), E = the five-point solver on the selected rows in f64 (ops.refit_essential; the
        reference's f32 run of the same solver, Q11).  A third-party estimator goes through its estimate_model."""
        from .estimators import EssentialMatrixEstimator, EssentialMatrixEstimatorNister, FundamentalMatrixEstimatorNew
        n = int(mask.sum())
        if n < (8 if self.fmat else 5):
            return None
        if matches.is_cuda and type(self.estimator) is FundamentalMatrixEstimatorNew and self.fmat:
            F, v = ops.refit_fundamental(matches.unsqueeze(0), mask.unsqueeze(0))
            return F, v
        if matches.is_cuda and type(self.estimator) in (EssentialMatrixEstimatorNister, EssentialMatrixEstimator) and not self.fmat:
            E, v = ops.refit_essential(matches.unsqueeze(0), mask.unsqueeze(0))
            return E[0], v[0]
        models = self.estimator.estimate_model(matches[mask].unsqueeze(0))
        if models is None or models.shape[0] == 0:
            models = torch.eye(3, device=matches.device, dtype=matches.dtype).unsqueeze(0)   # ransac.py:243-244
        return models.reshape(-1, 3, 3).to(matches.dtype), None

    def _local_optimization(self, best_score, best_mask, best_model, best_inlier_number, matches, threshold):
        """localOptimization, ransac.py:217-257 (lo = 1: one refit, lo = 2: up to lo_iters): refit on the inliers, score, keep the
        result when it scores at least as well (a tie is taken), stop otherwise -- or when the mask did not change (the next
        refit would see the same rows).  The host-side twin of dr_local_opt (the fused path), for the plugin path."""
        for _ in range(1 if self.lo == 1 else self.lo_iters):
            got = self._lo_candidates(matches, best_mask)
            if got is None:
                break
            cand, cvalid = got
            scores, masks = self.scoring.score(matches, cand, threshold)
            ok = ~torch.isnan(scores) & torch.isfinite(cand).flatten(1).all(-1)
            if cvalid is not None:
                ok = ok & cvalid
            if not bool(ok.any()):
                break
            scores = torch.where(ok, scores, torch.full_like(scores, -float("inf")))
            b = int(torch.argmax(scores))
            if not float(scores[b]) >= float(best_score):
                break
            changed = bool((masks[b] != best_mask).any())
            best_score, best_mask, best_model = scores[b], masks[b], cand[b]
            best_inlier_number = int(torch.sum(best_mask))
            if not changed:
                break
        return best_score, best_mask, best_model, best_inlier_number

    # -- one batch: sample -> gather -> solve; returns models [B,S,3,3], valid [B,S], soft weights
    def _hypotheses(self, matches, logits, gumbels=None):
        B = self.ransac_batch_size
        k = self.sampler.num_samples
        own_sampler = hasattr(self.sampler, "_next_seed") and hasattr(self.sampler, "tau")
        if _is_gumbel(self.sampler_id) and own_sampler:
            seed = self.sampler._next_seed()
            g = None if gumbels is None else gumbels.unsqueeze(0)
            lg = logits.unsqueeze(0).to(matches.dtype)
            if not self.train and not self.weighted:
                # test mode: `points[samples != 0]` (ransac.py:65) -- the index sets and the points themselves
                idx = ops.gumbel_topk(lg, B, k, self.sampler.tau, g, seed, soft=False)["idx"]
                samples, w = ops.gather(matches.unsqueeze(0), idx)[0], None
            else:
                samples, w, _ = ops.SampleGather.apply(matches.unsqueeze(0), lg, B, k, self.sampler.tau, g, seed)
                samples, w = samples[0], w[0]
                if self.weighted and self.fmat and not self.train:      # the refit's `soft_weights[0, ...]` (ransac.py:151-153)
                    self._soft0 = ops.soft_weights_row0(lg, k, self.sampler.tau, g, seed)[0]
        elif _is_gumbel(self.sampler_id):
            # a third-party sampler with the reference's duck-typed contract only (ransac.py:63-65,73):
            # sample(logits) -> (ret [B,N], y_soft [B,N]); the straight-through gather in plain torch ops
            ret, y_soft = self.sampler.sample(logits)
            pts = matches.repeat([ret.shape[0], 1, 1]) * ret.unsqueeze(-1)
            samples = pts[ret != 0].view(ret.shape[0], -1, matches.shape[-1])
            w = y_soft[ret != 0].view(ret.shape[0], -1)
            self._soft0 = y_soft[0].detach()
        else:
            # the reference calls sampler.sample() (ransac.py:59); this package's UniformSampler takes the point count.  The call
            # form is read off the signature -- catching TypeError would also swallow one raised INSIDE a plugin and call it twice
            idx = self.sampler.sample(matches.shape[0]) if _takes_argument(self.sampler.sample) else self.sampler.sample()
            samples, w = matches[idx], None
        wts = w if self.weighted else None
        if hasattr(self.estimator, "estimate_model_slots"):
            return self.estimator.estimate_model_slots(samples, wts)
        # a third-party estimator with the reference's contract only (ransac.py:71-76): estimate_model(samples[, w]) ->
        # [S*B', 3, 3]; slots = consecutive groups per sample, every finite model valid
        models = self.estimator.estimate_model(samples, wts) if wts is not None else self.estimator.estimate_model(samples)
        nb = samples.shape[0]
        # fixed slots: exactly S models per sample, in sample order.  S is the estimator's `solutions_per_sample` when it declares
        # one; otherwise 1 / 10 / 4 for [B,3,3] / five-point / seven-point outputs of the reference's shapes (a ragged output that
        # merely happens to divide evenly would be mis-grouped silently, so nothing is inferred from divisibility alone)
        S = getattr(self.estimator, "solutions_per_sample", None)
        if S is None and models is not None and models.shape[0] in (nb, 10 * nb, 4 * nb):
            S = models.shape[0] // nb
        if models is None or S is None or models.shape[0] != S * nb:
            raise ValueError("a plugin estimator must return exactly S models per sample in sample order (declare "
                             "`solutions_per_sample`): got %s for %d samples" % (None if models is None else tuple(models.shape), nb))
        models = models.reshape(nb, S, 3, 3)
        return models, torch.isfinite(models).flatten(2).all(-1)

    def _make_fast(self, solver, seed=0, super_hypotheses=None):
        drv = BatchedRANSAC(solver, ransac_batch_size=self.ransac_batch_size, train=False, threshold=self.threshold,
                            confidence=self.confidence, max_iterations=self.max_iterations, tau=self.sampler.tau,
                            weighted=self.weighted, refit=True, eps=self.eps, seed=seed, lo=self.lo, lo_iters=self.lo_iters)
        drv.super_hypotheses = super_hypotheses
        return drv

    def _fused_solver(self):
        """Name of the BatchedRANSAC solver equivalent to this object's plugins, or None (custom plugins, uniform
        sampler, train mode): test mode then runs on the device-resident driver with P = 1 -- same result, no host
        round-trip per batch except the termination read-back (1.6 -> 0.5 ms per pair at 2000 points x 1024 hypotheses)."""
        from .estimators import (EssentialMatrixEstimator, EssentialMatrixEstimatorNister, FundamentalMatrixEstimatorNew)
        from .samplers import GumbelSoftmaxSampler
        from .scorings import MSACScore
        if self.train or not _is_gumbel(self.sampler_id) or type(self.sampler) is not GumbelSoftmaxSampler:
            return None
        if type(self.scoring) is not MSACScore:
            return None
        k = self.sampler.num_samples
        if type(self.estimator) is EssentialMatrixEstimatorNister and k == 5 and not self.fmat:
            return "nister"
        if type(self.estimator) is EssentialMatrixEstimator and k == 5 and not self.fmat:
            return "stewenius"
        if type(self.estimator) is FundamentalMatrixEstimatorNew and k == 8 and self.fmat:
            return "f8"
        return None

    def __call__(self, matches, logits, K1, K2, gt_model, gumbels=None):
        """`gumbels` (optional, list of [B,N] tensors, one per batch) replaces the in-kernel noise: parity runs."""
        self._soft0 = None       # the weighted refit only ever uses soft weights drawn in THIS call
        solver = self._fused_solver() if self.fused else None
        if solver is not None and matches.is_cuda:
            cfg = (solver, self.ransac_batch_size, self.threshold, self.confidence, self.max_iterations, self.sampler.tau,
                   self.weighted, self.eps, self.lo, self.lo_iters)
            cfg = cfg + (self.graph_hypotheses,)
            if self._fast_cfg != cfg:     # public attributes may change between calls (sweeps)
                self._fast, self._graphs, self._fast_cfg = None, collections.OrderedDict(), cfg
                self._graph_rounds = len(self._make_fast(solver, super_hypotheses=self.graph_hypotheses).plan())
            if (self.graph and gumbels is None and matches.dtype == torch.float32 and not self.weighted
                    and not torch.cuda.is_current_stream_capturing() and self._graph_rounds <= 8):
                # The reference calls this object one pair at a time (model_cl.py:488-490, test.py:38): ~25 launches of 5-30 us
                # per pair.  Round 5: the whole call -- threshold, every round, the adaptive stop taken on the device, refit --
                # is captured once per (point count, device) and replayed: one graph launch + one staging copy per pair.
                # Round 6: device rounds of `graph_hypotheses` hypotheses, whatever `ransac_batch_size` is.
                key = (matches.shape[0], matches.device.index)
                g = self._graphs.get(key)
                if g is None:
                    while len(self._graphs) >= max(1, self.max_graphs):      # bounded: variable-N inputs re-capture, the oldest goes
                        self._graphs.popitem(last=False)
                    g = self._graphs[key] = _GraphedCall(self._make_fast(solver, seed=self.sampler._next_seed(),
                                                                         super_hypotheses=self.graph_hypotheses),
                                                         matches.shape[0], matches.device)
                else:
                    self._graphs.move_to_end(key)
                return g(matches, logits, K1, K2)
            if self._fast is None:
                self._fast = self._make_fast(solver)
            self._fast.seed = self.sampler._next_seed()
            out = self._fast(matches.unsqueeze(0), logits.unsqueeze(0).to(matches.dtype), K1, K2,
                             gumbels=None if gumbels is None else [g.unsqueeze(0) for g in gumbels])
            return out["model"][0], out["mask"][0], out["score"][0], int(out["iterations"][0])
        iterations = 0
        best_score = 0
        point_number = matches.shape[0]
        best_mask, best_model = [], []
        models_out: Dict[int, torch.Tensor] = {}
        threshold = normalized_threshold(self.threshold, K1, K2, self.fmat)
        threshold = float(threshold) if not isinstance(threshold, float) else threshold
        max_iters = self.max_iterations
        batch = 0
        while iterations < max_iters:
            g = None
            if gumbels is not None:
                if batch >= len(gumbels):
                    break
                g = gumbels[batch]
            models, valid = self._hypotheses(matches, logits, g)
            batch += 1
            B, S = valid.shape
            if self.train:
                if S == 1:
                    chosen, keep = models[:, 0], valid[:, 0]
                elif self.sampler.num_samples == 8:
                    # ransac.py:82-83: with the 8-point sampler every estimated model is kept (no best-of-S); here that is
                    # every VERIFIED solution of every sample (the reference's ten slots include the non-real ones)
                    chosen, keep = models.reshape(B * S, 3, 3), valid.reshape(B * S)
                else:
                    chosen, which = ops.select_closest_autograd(models.unsqueeze(0), valid.unsqueeze(0),
                                                                gt_model.unsqueeze(0))
                    chosen, keep = chosen[0], which[0] >= 0
                models_out[iterations] = chosen[keep]
            else:
                flat = models.reshape(B * S, 3, 3)
                scores, masks = self.scoring.score(matches, flat, threshold)
                scores = torch.where(valid.reshape(-1) & ~torch.isnan(scores), scores, torch.full_like(scores, -1.0))
                best_idx = torch.argmax(scores)
                if scores[best_idx] > best_score or iterations == 0:
                    best_score = scores[best_idx]
                    best_mask = masks[best_idx]
                    best_model = flat[best_idx]
                    best_inlier_number = int(torch.sum(best_mask))
                    if self.lo:
                        best_score, best_mask, best_model, best_inlier_number = self._local_optimization(
                            best_score, best_mask, best_model, best_inlier_number, matches, threshold)
                    max_iters = min(self.max_iterations,
                                    adaptive_iteration_number(best_inlier_number, point_number, self.estimator.sample_size,
                                                              self.confidence, self.eps, self.max_iterations))
            iterations += self.ransac_batch_size

        if self.train:
            return models_out, best_mask, best_score, iterations

        # final refit on the inliers (ransac.py:148-195); not differentiable
        with torch.no_grad():
            inl = best_mask.nonzero(as_tuple=True)[0]
            slots = hasattr(self.estimator, "estimate_model_slots")
            cvalid = None
            rw = None
            if self.fmat:
                pts_ = matches[inl].unsqueeze(0) if inl.numel() >= 8 else None
                if self.weighted and pts_ is not None and getattr(self, "_soft0", None) is not None:
                    rw = self._soft0[inl].unsqueeze(0)      # ransac.py:151-153: soft_weights[0, inlier_indices[0]], last batch
            else:
                # pymagsac absent: Nister on ALL points in f64 as one sample (ransac.py:157-165 -> nister.py:64-65)
                pts_ = matches.unsqueeze(0).double()
            if pts_ is None:
                cand = None
            elif slots:      # fixed-shape slots + validity: the eye(3) fillers of failed solves must not compete
                cand, cvalid = self.estimator.estimate_model_slots(pts_, rw) if rw is not None else self.estimator.estimate_model_slots(pts_)
                cand, cvalid = cand.reshape(-1, 3, 3), cvalid.reshape(-1)
            else:
                cand = self.estimator.estimate_model(pts_, rw) if rw is not None else self.estimator.estimate_model(pts_)
            if cand is None or cand.shape[0] == 0:
                if not isinstance(best_model, torch.Tensor):
                    best_model = torch.eye(3, device=matches.device, dtype=matches.dtype)
            else:
                cand = cand.to(matches.dtype)
                scores, _ = self.scoring.score(matches, cand, threshold)
                scores = torch.where(torch.isnan(scores), torch.full_like(scores, -1.0), scores)
                if cvalid is not None:
                    scores = torch.where(cvalid, scores, torch.full_like(scores, -1.0))
                if scores.max() > best_score:
                    b = torch.argmax(scores)
                    best_model, best_score = cand[b], scores[b]
        return best_model, best_mask, best_score, iterations


class _GraphedCall(object):
    """One test-mode RANSAC call on one image pair as a replayed HIP graph (drop-in path of RANSAC.__call__).

    The captured call is BatchedRANSAC with P = 1, seeds advanced on the device (`device_seeds`) and the adaptive stop taken
    on the device (`device_termination`): every round is in the graph, the kernels of a round skip a pair that has terminated.
    Inputs are staged into the buffers the graph was captured on (one multi-tensor copy), results are handed out as fresh
    tensors (one more): the caller keeps them across calls, as `ret.append(Es)` of model_cl.py:492 does.  `iterations` is
    returned as a 0-dim int32 tensor -- reading it as an int would be the only host synchronisation of the call."""

    def __init__(self, driver, N, device):
        from .graphs import GraphedStep
        self.driver = driver.device_seeds(device)
        driver.device_termination = True
        self.matches = torch.zeros(1, N, 4, device=device)
        self.logits = torch.zeros(1, N, device=device)
        self.K1 = torch.eye(3, device=device).unsqueeze(0).clone()
        self.K2 = torch.eye(3, device=device).unsqueeze(0).clone()
        self.matches[0, :, :2] = torch.rand(N, 2, device=device)      # something solvable for the warm-up calls
        self.matches[0, :, 2:] = self.matches[0, :, :2] + 0.01 * torch.rand(N, 2, device=device)
        self._eye = None
        self.step = GraphedStep(self._run, warmup=2)

    def _run(self):
        out = self.driver(self.matches, self.logits, self.K1, self.K2)
        # one buffer for everything a call returns: model 36 B | score 4 | iterations 4 | mask N (handed out by ONE copy per call).
        # Round 6: the one-pair state of a device-terminated f32 call already lives in such a buffer (ops.RansacState.packed)
        if out.get("packed") is not None:
            return out["packed"]
        u8 = lambda t: t.contiguous().view(torch.uint8).reshape(-1)
        return torch.cat([u8(out["model"][0]), u8(out["score"][:1]), u8(out["iterations"][:1]), u8(out["mask"][0])])

    def __call__(self, matches, logits, K1, K2):
        src = [matches, logits.to(torch.float32)]
        dst = [self.matches[0], self.logits[0]]
        if K1 is not None and K2 is not None:
            src += [K1.to(device=matches.device, dtype=torch.float32).reshape(3, 3), K2.to(device=matches.device, dtype=torch.float32).reshape(3, 3)]
        else:
            # no intrinsics: the eager path hands None to dr_ransac_init (threshold used as is).  The captured call always normalises
            # with the staged K1 / K2, so identity goes in -- f = (1 + 1 + 1 + 1) / 4 = 1, threshold unchanged, exactly -- instead of
            # whatever the previous pair left in the buffers (round-5 advice)
            if self._eye is None:
                self._eye = torch.eye(3, device=matches.device)
            src += [self._eye, self._eye]
        dst += [self.K1[0], self.K2[0]]
        torch._foreach_copy_(dst, src)
        packed = self.step().clone()
        model = packed[:36].view(torch.float32).view(3, 3)
        score = packed[36:40].view(torch.float32)[0]
        iterations = packed[40:44].view(torch.int32)[0]
        mask = packed[44:].view(torch.bool)
        return model, mask, score, iterations


class RANSAC3D(object):
    """Drop-in for the reference's RANSAC3D (ransac.py:303-450).  Train mode as in the reference; test mode (dead code
    there) = arg-min of the residual sum."""

    def __init__(self, estimator, sampler, scoring, fmat=False, train=False, ransac_batch_size=64, sampler_id=0,
                 weighted=0, threshold=1e-3, confidence=0.999, max_iterations=5000, lo=0, lo_iters=64, eps=1e-5,
                 flag=True):
        self.estimator = estimator
        self.sampler = sampler
        self.scoring = scoring
        self.train = train
        self.ransac_batch_size = ransac_batch_size
        self.sampler_id = sampler_id
        self.threshold = threshold
        self.confidence = confidence
        self.max_iterations = max_iterations
        self.eps = eps
        self.flag = flag

    def adaptive_iteration_number(self, inlier_number, point_number, confidence):
        """ransac.py:452-465 (the same rule as RANSAC's)."""
        return adaptive_iteration_number(inlier_number, point_number, self.estimator.sample_size, confidence, self.eps,
                                         self.max_iterations)

    def __call__(self, matches, logits, gt_model, valid=False, gumbels=None):
        train = self.train and not valid
        B = self.ransac_batch_size
        iterations, batch = 0, 0
        models, residuals, mean_residuals = {}, {}, {}
        best_model, best_score = None, float("inf")
        while iterations < self.max_iterations:
            g = None
            if gumbels is not None:
                if batch >= len(gumbels):
                    break
                g = gumbels[batch].unsqueeze(0)
            batch += 1
            if _is_gumbel(self.sampler_id):
                # the sampler's own sample size: 3, or 8 for sampler id 3 (model_cl.py:185-207 builds an 8-point sampler and
                # the reference feeds its 8-point samples to the rigid solver, which accepts n >= 3)
                k = int(getattr(self.sampler, "num_samples", 3))
                if not 3 <= k <= 8:
                    raise ValueError("RANSAC3D needs a sampler with 3 <= num_samples <= 8")
                samples, _, _ = ops.SampleGather.apply(matches.unsqueeze(0), logits.unsqueeze(0).to(matches.dtype), B, k,
                                                       self.sampler.tau, g, self.sampler._next_seed())
                samples = samples[0]
            else:
                samples = matches[self.sampler.sample(matches.shape[0])]
            est, R, t, _ = self.estimator.estimate_model(samples, flag=self.flag)
            ok = self.estimator.last_valid
            res, mean_res, _ = self.estimator.squared_residual(matches[:, :3], matches[:, 3:],
                                                               est[:, :3, :].transpose(-1, -2))
            if train:
                models[iterations] = est[ok]
                residuals[iterations] = res
                mean_residuals[iterations] = mean_res
            else:
                b = torch.argmin(torch.where(ok, res, torch.full_like(res, float("inf"))))
                if float(res[b]) < best_score:
                    best_score, best_model = float(res[b]), est[b]
            iterations += B
        if train:
            return models, residuals, mean_residuals, 0, iterations
        return best_model, residuals, mean_residuals, best_score, iterations


class _Seeds(object):
    """The per-call sampler seeds of a batched driver: call number c of a driver with base seed s draws with the key
    s * 0x9E3779B97F4A7C15 + c (mod 2^64), from the host formula or, after on_device(), from a counter on the device
    (ops.DeviceSeed: graph-capturable steps) -- the same sequence either way."""

    def __init__(self, seed):
        self.seed, self.calls = seed, 0
        self.dev = None          # ops.DeviceSeed
        self.ahead = None        # (block, position): seeds drawn ahead for every batch of a call by ONE launch (device_termination)

    def on_device(self, device):
        self.dev = ops.DeviceSeed(self.seed, device, self.calls)

    def next(self, R=1):
        """the seed of the next batch.  R > 1: of the next batch of a device round of R batches; the R - 1 batches behind it take the
        consecutive seeds (consumed here: a batch-by-batch driver with the same base seed draws the same hypotheses)"""
        first = self.calls
        self.calls += R
        if self.dev is None:
            return (self.seed * 0x9E3779B97F4A7C15 + first) & (2 ** 64 - 1)
        if self.ahead is not None:
            blk, pos = self.ahead
            self.ahead = (blk, pos + R) if pos + R < blk.shape[0] else None
            return blk[pos:pos + 1]
        return self.dev.next() if R == 1 else self.dev.next_block(R)[:1]


class _SeededDriver(object):
    """`seed`, `calls` (assignable between calls), `_dev_seed` and device_seeds() of the batched drivers, kept in one _Seeds"""
    seed = property(lambda self: self._seeds.seed, lambda self, v: setattr(self._seeds, "seed", v))
    calls = property(lambda self: self._seeds.calls, lambda self, v: setattr(self._seeds, "calls", v))
    _dev_seed = property(lambda self: self._seeds.dev)

    def device_seeds(self, device):
        """From the next call on the per-call seed is computed on the device (ops.DeviceSeed) -- the same sequence of seeds,
        hence the same hypotheses, but nothing about a call depends on a host-side counter any more, so a call with
        max_iterations <= ransac_batch_size (one round, no read-back) can be captured in a HIP graph and replayed
        (differentiable_ransac_amd.graphs.GraphedStep)."""
        self._seeds.on_device(device)
        return self

    # ---- sampling="prosac" (BatchedRANSAC, BatchedRegistration; test mode): ops.prosac_sample draws from the ranking of the logits
    def _set_prosac_draws(self, prosac_draws):
        if isinstance(prosac_draws, bool) or not isinstance(prosac_draws, int) or prosac_draws < 1:
            raise ValueError(f"prosac_draws must be an int of at least 1, got {prosac_draws!r}")
        self.prosac_draws = prosac_draws
        self._prosac_tables = {}

    def _prosac_setup(self, logits, N, device):
        """(order, growth) of a call: the ranking of its logits and the growth table, cached per (N, k, prosac_draws, device)"""
        if N < self.k:
            raise ValueError(f"sampling='prosac' needs at least {self.k} points per pair, got {N}")
        key = (N, self.k, self.prosac_draws, str(device))
        growth = self._prosac_tables.get(key)
        if growth is None:
            growth = ops.prosac_growth(N, self.k, self.prosac_draws, device)
            if not torch.cuda.is_current_stream_capturing():      # (a table made inside a capture lives in that graph's pool)
                self._prosac_tables[key] = growth
        return ops.prosac_rank(logits), growth


class BatchedRANSAC(_SeededDriver):
    """The (pair x hypothesis) grid in one go: all P pairs sample, solve, score and select per round with a fixed
    number of launches (K1, K2, K3, K4, K6) and no [B,N] / [M,N] tensor in HBM unless `keep_masks` is set.

    solver: "nister" | "stewenius" | "f8" | "f7".  Test mode reproduces ransac.py:109-195 per pair (arg-max,
    adaptive stop with the per-pair inlier count evaluated on the device, final refit); train mode returns the
    chosen models [P, rounds*B, 3, 3] with autograd to `logits`.
    """

    _SOLVERS = {"nister": (5, 10), "stewenius": (5, 10), "f8": (8, 1), "f7": (7, 4)}
    # exponent of the adaptive stop: the reference raises the inlier ratio to its estimator's `sample_size` (ransac.py:204-215), 5 for
    # the essential estimators and 7 for FundamentalMatrixEstimatorNew (fundamental_matrix_estimator.py:164) -- not the sampler's
    # points per sample (8 for "f8", and for "nister" with num_samples=8)
    _STOP_EXPONENT = {"nister": 5, "stewenius": 5, "f8": 7, "f7": 7}

    def __init__(self, solver="nister", ransac_batch_size=1024, train=False, threshold=0.75, confidence=0.999,
                 max_iterations=5000, tau=1.0, seed=0, weighted=0, keep_masks=False, refit=True, eps=1e-5,
                 sampling="gumbel", num_samples=None, lo=0, lo_iters=64, prosac_draws=200000, scoring="msac", irls_iters=10):
        # scoring (test mode): "msac" = the reference's MSACScore (ops.msac_score); "magsac" = the two-view MAGSAC++ score
        # (ops.magsac_score) in its place -- dr_ransac_update, super-rounds and device_termination as they are -- and, with
        # refit=True and irls_iters > 0, the IRLS polish under that loss (ops.magsac_irls, up to irls_iters weighted refits) in the place
        # of the final refit and its acceptance step; the result gains irls_fits [P].  mask and inliers stay dr_ransac_update's.
        _check_scoring(scoring, irls_iters)
        if scoring == "magsac":
            if train:
                raise ValueError("scoring='magsac' is a test-mode score: train mode scores nothing")
            if lo:
                raise ValueError("scoring='magsac' needs lo=0: the local optimisation (dr_local_opt) scores its refits with MSAC")
            if weighted:
                raise ValueError("scoring='magsac' needs weighted=0: its polish computes its own row weights")
            if keep_masks:
                raise ValueError("scoring='magsac' needs keep_masks=False: the MAGSAC++ scoring launch writes no mask rows")
        self.scoring = scoring
        self.irls_iters = irls_iters
        # num_samples: points per sample when it is not the solver's minimal count -- 8 with solver="nister" is the reference's
        # `-sam 3` (8-point Gumbel sampler) feeding the five-point estimator (ransac.py:82-83; nister.py:64-65 runs on all rows)
        # sampling: "gumbel" = the reference's sampler (noise for every point of every hypothesis, top-k);
        # "topdown" = the same index-set distribution drawn as k sequential soft-max draws without replacement
        # (ops.topdown_sample, O(B k log N)); test mode only, no soft weights (weighted=0), no explicit noise.
        # "uniform" = UniformSampler.batch_generate (samplers/uniform_sampler.py:15-19: randint(0, N - 1), with replacement,
        # the last point never drawn) for all pairs in one launch; index sets only, logits ignored.
        # "prosac" = PROSAC (ops.prosac_sample, O(B k)): the logits are ranked once per call and draw t of a call -- hypothesis
        # t - 1 counted through its rounds -- takes the point of rank n(t) - 1 and k - 1 points ranked above it, n(t) growing from k to
        # N over about `prosac_draws` draws (ops.prosac_growth), uniform over all points from there on; draw 1 is the k best-ranked
        # points.  Test mode only, index sets only, no explicit noise; the adaptive stop stays the driver's own.
        if sampling not in ("gumbel", "topdown", "uniform", "prosac"):
            raise ValueError("sampling must be 'gumbel', 'topdown', 'uniform' or 'prosac'")
        self._set_prosac_draws(prosac_draws)
        # lo (test mode; ignored in train mode, as in the reference): local optimisation of ransac.py:217-257 after every new best
        # model -- 1 = one LSQ refit on its inliers, 2 = up to lo_iters of them (ops.local_optimize, one launch per device round)
        _check_lo(lo, lo_iters)
        self.lo = int(lo)
        self.lo_iters = int(lo_iters)
        if sampling in ("topdown", "uniform", "prosac") and (train or weighted):
            raise ValueError(f"{sampling} sampling yields index sets only: train mode and weighted=1 need the Gumbel sampler")
        self.sampling = sampling
        self.pipeline = True     # test mode: issue round r+1's sampler/solver on a second stream while round r is scored
        # test mode, round 5: True = every round of a call is ISSUED and the adaptive stop of ransac.py:135-144 is taken on the
        # device (the kernels of a round skip the pairs whose counter has reached its bound, ops `gate=`): no read-back, so a
        # whole call -- however many rounds the data ask for -- is capturable in one HIP graph.  Costs a handful of empty
        # launches per unneeded round; meant for few rounds (max_iterations / ransac_batch_size <= 8), refused above 16.
        self.device_termination = False
        self.sync_every = None   # device rounds between termination read-backs; None = max(1, 256 // hypotheses per device round)
        self._pipe = None
        self.solver = solver
        self.k, self.S = self._SOLVERS[solver]
        self.stop_k = self._STOP_EXPONENT[solver]     # (unchanged by num_samples)
        if num_samples is not None and num_samples != self.k:
            if solver not in ("nister", "f8") or not self.k < num_samples <= 8:
                raise ValueError(f"solver {solver!r} takes {self.k} points per sample (non-minimal samples: 'nister' / 'f8', up to 8)")
            self.k = int(num_samples)
        self.B = ransac_batch_size
        self.train = train
        self.threshold = threshold
        self.confidence = confidence
        self.max_iterations = max_iterations
        self.tau = tau
        self._seeds = _Seeds(seed)
        self.weighted = weighted
        self.keep_masks = keep_masks
        self.refit = refit
        self.eps = eps
        self.fmat = solver in ("f8", "f7")
        self._race_ws = None     # per-call weights of the one-logarithm sampler (written by dr_ransac_init, read by every round)
        self._prosac = None      # per-call (order, growth) of sampling="prosac" (made by the test-mode set-up, read by every round)
        self._side = None
        self._gap = None         # scratch word of the one-launch dispatch gap in front of the sampler (see __call__)
        # Super-rounds (round 6, test mode).  The loop of ransac.py:55-144 runs `ransac_batch_size` hypotheses per iteration of a
        # Python loop; with the reference's default of 64 a call is up to 79 iterations of four launches each.  A DEVICE round here is
        # R consecutive batches at once: the sampler draws row b of the round with the noise of row b % B of batch b // B (per-call
        # seeds are consecutive integers), solver and scoring see R * B hypotheses, and dr_ransac_update walks the R sub-batches IN
        # ORDER with the loop's own stop rule -- (model, mask, score, iterations) are those of the batch-by-batch loop, bit for bit,
        # whatever R is; hypotheses behind the stop are speculative work.  (h_0, h_1, ...) = hypotheses per device round, the last
        # entry repeated; None = automatic: rounds of 1024 hypotheses when ransac_batch_size is below 1024,
        # one batch per round otherwise; False = always one batch per round (the host loop of rounds 1-5).
        self.super_hypotheses = None

    def plan(self, n_batches=None, dtype=torch.float32):
        """Batches per device round of a test-mode call (see `super_hypotheses`): a list summing to the number of batches the loop
        of ransac.py:55 can run at most, ceil(max_iterations / ransac_batch_size)."""
        if n_batches is None:
            n_batches = max(1, math.ceil(self.max_iterations / self.B))
        sh = self.super_hypotheses
        one = [1] * n_batches
        if sh is False or self.train or self.sampling != "gumbel" or self.keep_masks or dtype != torch.float32:
            return one
        if self.lo and not self.train:
            # a local optimisation after sub-batch j changes the score sub-batch j + 1 must beat: dr_ransac_update cannot walk
            # several batches in one launch exactly, so every batch is a device round with its own local-optimisation launch
            return one
        if self.weighted:
            # weighted rows in the minimal solves (ransac.py:70-74) need the soft weights of every batch, and the weighted refit wants
            # the row-0 soft weights of the LAST batch a pair ran: batch by batch (a super-round samples index sets only)
            return one
        if sh is None:
            if self.B >= 1024:
                return one
            sh = (1024, 1024)
        # (dr_ransac_update walks at most 512 sub-batches per launch)
        sizes = [min(512, max(1, int(h) // self.B)) for h in sh]
        out, left = [], n_batches
        while left > 0:
            r = min(left, sizes[min(len(out), len(sizes) - 1)])
            out.append(r)
            left -= r
        return out

    def hypotheses(self, matches, logits, gumbels=None):
        """matches [P,N,4], logits [P,N] -> models [P,B,S,3,3], valid [P,B,S], idx [P,B,k] (differentiable w.r.t. logits)."""
        return self._hypotheses(matches, logits, gumbels)[:3]

    def _solve(self, samples, weights=None, gate=None):
        """samples [P,B,k,c] -> models [P,B,S,3,3], valid [P,B,S].  gate (a later round of a device-terminated call): the gated
        five-point entry, for minimal f32 samples."""
        if self.solver in ("nister", "stewenius"):
            if gate is not None and self.k == 5 and samples.dtype == torch.float32:
                return ops.solve_essential_gated(samples, self.solver, gate)
            return ops.solve_essential(samples, weights, self.solver)
        if self.solver == "f8":
            F, v = ops.solve_fundamental8(samples, weights)
            return F.unsqueeze(2), v.unsqueeze(2)
        return ops.solve_f7(samples)

    def _hypotheses(self, matches, logits, gumbels=None, gate=None, R=1, t0=0):
        """hypotheses() + the (seed, noise) pair of the draw when the weighted refit will need row 0's soft weights again
        (returned, not stashed on self: two rounds are in flight on two streams when `pipeline` is on), else None.
        R > 1 (test mode, see `super_hypotheses`): R consecutive batches in one go -> models [P, R * B, S, 3, 3]; explicit noise is the
        R batches' tensors concatenated along the hypothesis axis.
        t0 (sampling="prosac"): the hypotheses the call has drawn before this round; the round's rows are PROSAC draws t0 + 1 ..."""
        B, w, row0, solve_gate = R * self.B, None, None, None
        f32_two_view = matches.dtype == torch.float32 and matches.shape[-1] == 4
        if self.sampling == "uniform" and gumbels is None:
            if self.solver == "f8" and self.k == 8 and f32_two_view:
                # sampler + gather + 8-point solve in ONE launch (BASELINE configs[0] is launch-bound: six launches -> four)
                idx, F, v = ops.solve_f8_uniform(matches, B, self._seeds.next())
                return F.unsqueeze(2), v.unsqueeze(2), idx, None
            idx = ops.uniform_sample(matches.shape[0], B, self.k, matches.shape[1], self._seeds.next(), matches.device)
            samples = ops.gather(matches, idx)
        elif self.sampling == "topdown" and gumbels is None:
            idx = ops.topdown_sample(logits, B, self.k, self._seeds.next())
            samples = ops.gather(matches, idx)
        elif self.sampling == "prosac":
            if gumbels is not None:
                raise ValueError("sampling='prosac' draws index sets from the ranking of the logits: explicit noise is refused")
            if self._prosac is None:      # (hypotheses() outside a call: __call__ ranks once for all its rounds)
                order, growth = self._prosac_setup(logits, matches.shape[1], matches.device)
            else:
                order, growth = self._prosac
            idx = ops.prosac_sample(order, growth, B, self.k, self._seeds.next(), t0, P=matches.shape[0], N=matches.shape[1],
                                    device=matches.device)
            samples = ops.gather(matches, idx)
        elif self.train or self.weighted:
            seed = self._seeds.next()
            samples, w, idx = ops.SampleGather.apply(matches, logits, B, self.k, self.tau, gumbels, seed)
            if self.weighted and self.solver == "f8" and not self.train and self.refit:
                # the weighted LSQ refit (ransac.py:151-153) needs y_soft of hypothesis 0 of the LAST batch a pair ran: the seed is
                # handed back so that __call__ can re-draw that one row (ops.soft_weights_row0).  weighted=1 implies the Gumbel
                # sampler (__init__ refuses it with 'uniform' / 'topdown'); the 7-point solver takes no weights
                row0 = (seed, gumbels)
        # test mode consumes the index sets only (`points[samples != 0]`, ransac.py:65): no soft-max statistics, and the samples are
        # the points themselves (not points x a straight-through value of 1 +- 1 ulp)
        elif gumbels is None and f32_two_view and logits.dtype == torch.float32:
            idx, samples = ops.gumbel_topk_gather(matches, logits, B, self.k, self.tau, self._seeds.next(R), gate=gate,
                                                  sub=self.B if R > 1 else 0, race_ws=self._race_ws)   # one launch
            solve_gate = gate
        else:
            if gumbels is None and R > 1:
                raise ValueError("super-rounds with in-kernel noise serve f32 two-view correspondences (plan() says so)")
            idx = ops.gumbel_topk(logits, B, self.k, self.tau, gumbels, self._seeds.next(R), soft=False)["idx"]
            samples = ops.gather(matches, idx)
            solve_gate = gate if R > 1 else None      # (one batch per round: ungated as found, docs/LOG.md)
        models, valid = self._solve(samples, w if self.weighted else None, solve_gate)
        return models, valid, idx, row0

    def __call__(self, matches, logits, K1=None, K2=None, gt_model=None, gumbels=None):
        P, N, _ = matches.shape
        dev, dt = matches.device, matches.dtype
        self._race_ws = None      # (weights of THIS call's logits only: set by the test-mode set-up below, dropped by _finish)
        self._prosac = None
        if self.sampling == "prosac" and gumbels is not None:
            raise ValueError("sampling='prosac' draws index sets from the ranking of the logits: explicit noise is refused")
        rounds = max(1, math.ceil(self.max_iterations / self.B))
        if self.train:
            out = []
            for r in range(rounds):
                g = None if gumbels is None else gumbels[r]
                if (self.solver == "nister" and self.k == 5 and not self.weighted and matches.dtype == torch.float32
                        and logits.dtype == torch.float32 and logits.requires_grad):
                    # the training path proper (train mode implies the Gumbel sampler: __init__ refuses the index-only samplings):
                    # sampler + gather, then solver + best-of-ten as ONE autograd node whose backward
                    # takes the gradient of the chosen model in sparse form (ops.solve_select_essential)
                    samples, _, _ = ops.SampleGather.apply(matches, logits, self.B, self.k, self.tau, g, self._seeds.next())
                    chosen, _, keep, _, _ = ops.solve_select_essential(samples, gt_model)
                    out.append((chosen, keep))
                    continue
                models, valid, _ = self.hypotheses(matches, logits, g)
                if self.S == 1:
                    chosen = models[:, :, 0]
                    keep = valid[:, :, 0]
                elif self.k == 8:      # ransac.py:82-83: the 8-point sampler keeps every model of every sample
                    chosen = models.reshape(P, self.B * self.S, 3, 3)
                    keep = valid.reshape(P, self.B * self.S)
                else:
                    chosen, _, keep = ops.select_closest_autograd(models, valid, gt_model, want_keep=True)
                out.append((chosen, keep))
            if len(out) == 1:            # one batch (train.py's max_iters = 100 with -rbs >= 100): nothing to concatenate
                return out[0]
            return torch.cat([c for c, _ in out], dim=1), torch.cat([k for _, k in out], dim=1)

        with torch.no_grad():
            use_K = K1 is not None and not self.fmat
            # (views that start inside a larger buffer -- `packed[s:e]` of ragged pairs -- are realigned ONCE per call, not per launch)
            matches, logits = ops.L.aligned(matches.contiguous()), ops.L.aligned(logits)
            # device rounds (see `super_hypotheses`): plan[i] batches of B hypotheses in round i, the first of them batch first[i]
            n_batches = rounds if gumbels is None else min(rounds, len(gumbels))
            plan = self.plan(n_batches, dt) if n_batches > 0 else []
            first = [sum(plan[:i]) for i in range(len(plan))]
            rounds = len(plan)
            # The essential-matrix refit candidate (Nister on ALL points, ransac.py:157-165) depends on the matches only: it is issued
            # on a side stream and joins before the final scoring -- and it is issued FIRST, before the state set-up (round 5; see the
            # note on dispatch order below).
            pre = None
            if self.refit and not self.fmat and self.scoring == "msac":
                if self._side is None:
                    self._side = torch.cuda.Stream(device=dev)
                self._side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(self._side):
                    pre = ops.refit_essential(matches)
                    if not torch.cuda.is_current_stream_capturing():
                        matches.record_stream(self._side)
            # (device termination with device seeds: the keys of all batches of the call come out of the set-up launch; one pair in
            #  f32: the state lives in one buffer, which is what the replayed drop-in call hands out)
            draw = self.device_termination and self._dev_seed is not None and n_batches > 1 and gumbels is None
            # the weights of the one-logarithm sampler, once per call, out of the same launch (when that form pays: ops.race_form_pays)
            race_lg = None
            if (plan and gumbels is None and self.sampling == "gumbel" and not self.weighted and dt == torch.float32
                    and logits.dtype == torch.float32 and matches.shape[-1] == 4
                    and ops.race_form_pays(P, self.B * plan[0], N, self.tau)):
                race_lg = logits.contiguous()
            # threshold normalisation (ransac.py:49-53) + per-pair state in one launch
            st, thr = ops.ransac_init(P, N, self.max_iterations, self.threshold, K1 if use_K else None,
                                      K2 if use_K else None, dev, dt, seeds=(self._dev_seed, n_batches) if draw else None,
                                      packed=self.device_termination and P == 1, race_logits=race_lg)
            self._race_ws = st.race_ws
            if self.sampling == "prosac":
                self._prosac = self._prosac_setup(logits, N, dev)
            # what every round of the call works on (_round, _finish): state, inputs, the masks of the last round (keep_masks) and,
            # for the weighted refit, per pair the row-0 soft weights of the last batch it ran
            c = types.SimpleNamespace(st=st, thr=thr, matches=matches, logits=logits, plan=plan, pre=pre, all_masks=None,
                                      lo_seen=None, lo_refits=None, last_w=None)
            if self.lo:
                # the local optimisation's per-pair snapshot of (best_score, best_model) -- NaN: the first replacement is always
                # seen -- and its refit counters (capturable allocations: a replayed call re-fills them)
                c.lo_seen = torch.full((P, 10), float("nan"), device=dev, dtype=dt)
                c.lo_refits = torch.zeros(P, device=dev, dtype=torch.int32)
            if pre is not None and plan and P * self.B * plan[0] >= 65536:
                # Dispatch order (round 5): a refit block wants a whole SIMD's registers and 38.9 KB of LDS on its CU; once the
                # sampler's 32 768 light workgroups are in the queue it does not get them until the sampler's grid runs dry
                # (measured at 128 pairs: launched 6 us after the sampler it ran 15 -> 241 us for 52 us of work, and the solver
                # behind it started 56 us late on the SIMDs it held).  Hence the refit is issued before the set-up -- but it waits for
                # this stream's earlier work through an event and still lost that race by half a microsecond
                # (rocprofv3, 128 pairs: sampler dispatched at 5.4 us, refit at 5.9 -- it then ran 232 us for 57 us of work and the
                # solver behind it started 56 us late on the SIMDs it still held: step 0.947 -> 1.018 ms with the refit).  One
                # tiny launch in front of the sampler lets the refit's 128 blocks in first: refit 57 us, sampler 178 -> 191 us,
                # solver 146 us, step 0.996 ms.  (Set-up AND refit on the side stream with this stream waiting for the set-up:
                # refit first as well, but 57 us between two steps instead of 17: 1.043 ms.  The refit issued right before the first
                # scoring launch instead of up front -- scratch/runs/r5_gpu_w.sh, 128 pairs: step with refit 1.015 -> 1.063 ms;
                # the same on a high-priority stream: 1.069 ms.  Both measured and dropped.)
                if self._gap is None or self._gap.state.device != matches.device:
                    self._gap = ops.DeviceSeed(0, matches.device)
                self._gap.next()
            if self.weighted and self.solver == "f8" and self.refit:
                c.last_w = torch.zeros((P, N), device=dev, dtype=dt)

            def hyp(r, gate=None):
                """the hypotheses of device round r; explicit noise: its batches' tensors along the hypothesis axis"""
                g = None
                if gumbels is not None:
                    g = gumbels[first[r]] if plan[r] == 1 else torch.cat(list(gumbels[first[r]:first[r] + plan[r]]), dim=1)
                return self._hypotheses(matches, logits, g, gate=gate, R=plan[r], t0=first[r] * self.B)

            if self.device_termination:
                if rounds > 16:
                    raise ValueError("device_termination issues every round: at most 16 device rounds per call (see super_hypotheses)")
                if draw:
                    self._seeds.ahead = (st.seeds, 0)    # consecutive seeds, one per BATCH (drawn by dr_ransac_init)
                for r in range(rounds):
                    gate = st if r > 0 else None
                    self._round(c, r, hyp(r, gate), gate)
                self._seeds.ahead = None
                return self._finish(c)
            # Rounds are pipelined: the hypotheses of round r+1 (sampler + solver, latency-bound, independent of round r's
            # outcome) are issued on a second stream before round r is scored, so they run under K4/K6 and under the
            # host's "does any pair continue?" read-back.  If round r ends the loop they are simply dropped.
            main = torch.cuda.current_stream()
            ahead = hyp(0) if rounds > 0 else None
            r = 0
            while ahead is not None:
                h, ahead = ahead, None
                if self.pipeline and r + 1 < rounds:
                    if self._pipe is None:
                        self._pipe = torch.cuda.Stream(device=dev)
                    self._pipe.wait_stream(main)          # inputs (and, for explicit noise, the caller's tensors) are ready
                    with torch.cuda.stream(self._pipe):
                        ahead = hyp(r + 1)
                self._round(c, r, h)      # (local optimisation included: the read-back below sees the bound it set)
                r += 1
                if r >= rounds:
                    break
                # host read-back "does any pair continue?" only when another round could follow, and for small batches
                # only every few rounds (pairs that have terminated are frozen on the device by K6, so a round issued
                # after the last pair stopped changes nothing)
                sync_every = max(1, 256 // max(1, self.B * plan[r - 1])) if self.sync_every is None else self.sync_every
                if r % sync_every == 0 and not bool((st.iters.double() < st.max_iters).any()):
                    break
                if ahead is None:
                    ahead = hyp(r)
                else:
                    main.wait_stream(self._pipe)
                    for t_ in ahead[:2]:
                        t_.record_stream(main)
            if ahead is not None and self._pipe is not None:
                main.wait_stream(self._pipe)              # dropped speculative work: keep the allocator's stream order simple
            return self._finish(c)

    def _round(self, c, r, hyp, gate=None):
        """What device round r of a test-mode call does once its hypotheses `hyp` (_hypotheses' result) exist: soft-weight carry,
        scoring, arg-max / "better?" test / best mask / adaptive stop of ransac.py:135-142 on the device (K6), local optimisation.
        gate: the state, in a later round of a device-terminated call (the launches skip the pairs that have terminated)."""
        models, valid, _, row0 = hyp
        P = c.matches.shape[0]
        if c.last_w is not None:
            # pairs still iterating in this round take this round's row-0 soft weights; terminated pairs keep theirs
            # ("the last batch sampled", per pair)
            w0 = ops.soft_weights_row0(c.logits, self.k, self.tau, row0[1], row0[0])
            c.last_w = torch.where((c.st.iters.double() < c.st.max_iters)[:, None], w0, c.last_w)
        flat, valid = models.reshape(P, -1, 3, 3), valid.reshape(P, -1)
        if self.scoring == "magsac":
            scores, _ = ops.magsac_score(c.matches, flat, c.thr, valid=valid, gate=gate)
        else:
            scores, masks = ops.msac_score(c.matches, flat, c.thr, want_masks=self.keep_masks, valid=valid, gate=gate)
            if self.keep_masks:
                c.all_masks = masks
        # dr_ransac_update's sub_models: the round's models are plan[r] batches of B x S
        ops.ransac_update(c.st, c.matches, flat, valid, scores, c.thr, self.B, self.stop_k, self.confidence, self.eps,
                          sub_models=self.B * self.S if c.plan[r] > 1 else 0)
        if c.lo_seen is not None:
            ops.local_optimize(c.st, c.matches, c.thr, self.fmat, self.lo, self.lo_iters, self.stop_k, self.confidence, self.eps,
                               self.max_iterations, c.lo_seen, c.lo_refits)

    def _finish(self, c):
        """final refit on the inliers of the best model (ransac.py:148-195) and the result dictionary"""
        self._race_ws = None
        self._prosac = None
        st = c.st
        irls_fits = None
        if self.scoring == "magsac":
            P, N, _ = c.matches.shape
            irls_fits = torch.zeros(P, device=c.matches.device, dtype=torch.int32)
            if self.refit and self.irls_iters > 0:
                ops.magsac_irls(st, c.matches, c.thr, self.fmat, self.irls_iters, irls_fits,
                                torch.empty((P, N), device=c.matches.device, dtype=c.matches.dtype))
        elif self.refit:
            if self.fmat:
                F, fvalid = ops.refit_fundamental(c.matches, st.best_mask, c.last_w)   # (weighted) LSQ on the inliers of the best mask
                cand, cvalid = F.unsqueeze(1), fvalid.unsqueeze(1)
            else:
                torch.cuda.current_stream().wait_stream(self._side)
                cand, cvalid = c.pre
                if not torch.cuda.is_current_stream_capturing():
                    cand.record_stream(torch.cuda.current_stream())
                    cvalid.record_stream(torch.cuda.current_stream())
            # score the candidates and keep the best one where it beats the RANSAC result: one launch, in place
            ops.refit_accept(c.matches, cand, cvalid, c.thr, st.best_score, st.best_model)
        out = dict(model=st.best_model, mask=st.best_mask, score=st.best_score, iterations=st.iters, inliers=st.best_inliers,
                   masks=c.all_masks, packed=st.packed)
        if c.lo_refits is not None:
            out["lo_refits"] = c.lo_refits
        if irls_fits is not None:
            out["irls_fits"] = irls_fits
        return out


class BatchedRANSAC3D(_SeededDriver):
    """RANSAC3D (ransac.py:303-450) over a batch of point-cloud pairs in one go: matches [P,N,6] = (p, q), logits [P,N].

    One round = K1 Gumbel top-k (k = 3) -> K2 gather -> K3r rigid SVD solver -> K4r squared residuals of every model
    against every point (+ inlier masks).  Train mode returns what the reference's train branch collects
    (models [P, rounds*B, 4, 4], keep, residual sums [P, rounds*B], mean residual per round) with autograd to the
    logits; test mode (dead code upstream) keeps the arg-min of the residual sum per pair."""

    def __init__(self, ransac_batch_size=2048, train=False, threshold=0.03, max_iterations=1000, tau=1.0, seed=0,
                 flag=True, keep_masks=False):
        self.B = ransac_batch_size
        self.train = train
        self.threshold = threshold
        self.max_iterations = max_iterations
        self.tau = tau
        self._seeds = _Seeds(seed)
        self.flag = flag
        self.keep_masks = keep_masks

    def __call__(self, matches, logits, gumbels=None):
        P, N, _ = matches.shape
        rounds = max(1, math.ceil(self.max_iterations / self.B))
        if gumbels is not None:
            rounds = min(rounds, len(gumbels))
        if self.train:
            out = []
            for r in range(rounds):
                g = None if gumbels is None else gumbels[r]
                samples, _, _ = ops.SampleGather.apply(matches, logits, self.B, 3, self.tau, g, self._seeds.next())
                model, R, t, scale, valid = ops.solve_rigid_autograd(samples.reshape(P * self.B, 3, 6), None, self.flag)
                model = model.reshape(P, self.B, 4, 4)
                res, _ = ops.rigid_residual_autograd(matches, model, self.threshold)
                out.append((model, valid.reshape(P, self.B), res, res.sum(1) / (self.B * N)))
            return dict(models=torch.cat([o[0] for o in out], 1), keep=torch.cat([o[1] for o in out], 1),
                        residuals=torch.cat([o[2] for o in out], 1), mean_residuals=torch.stack([o[3] for o in out], 1))
        with torch.no_grad():
            matches, logits = ops.L.aligned(matches.contiguous()), ops.L.aligned(logits)
            best, best_model = None, None      # "no state yet": the first update writes it (no fill / copy launches per call)
            best_mask = torch.empty((P, N), device=matches.device, dtype=torch.bool) if self.keep_masks else None
            masks = None
            for r in range(rounds):
                g = None if gumbels is None else gumbels[r]
                idx = ops.gumbel_topk(logits, self.B, 3, self.tau, g, self._seeds.next(), soft=False)["idx"]
                if matches.dtype == torch.float32:
                    # K2 + K3r in one launch (samples read through the index sets), the round's residual sums cleared on the way
                    # the residual sums are ACCUMULATED (atomics: order-nondeterministic in the last bits) into a buffer that
                    # dr_solve_rigid_gather_f32 clears.  (Rounds 4-5 also zero-filled it outside a graph capture -- a 5 us torch fill
                    # launch per round in the eager step, round-5 review; an error between the two launches raises, so nobody reads
                    # the buffer then.)
                    res = torch.empty((P, self.B), device=matches.device, dtype=torch.float32)
                    model, valid = ops.solve_rigid_gather(matches, idx, self.flag, zero_sums=res)
                    res, masks = ops.rigid_residual(matches, model, self.threshold, self.keep_masks, res=res)
                else:
                    samples = ops.gather(matches, idx)
                    model, R, t, scale, valid = ops.solve_rigid(samples.reshape(P * self.B, 3, 6), None, self.flag)
                    model = model.reshape(P, self.B, 4, 4)
                    res, masks = ops.rigid_residual(matches, model, self.threshold, self.keep_masks)
                # K6 of the 3-D path on the device: arg-min over the valid models, strict "better" test, best model and mask
                # (one launch; was where / min / gather / where x3: ten torch kernels per round)
                best, best_model, _ = ops.ransac3d_update(matches, model, valid.reshape(P, self.B), res, self.threshold, best,
                                                          best_model, best_mask)
            return dict(model=best_model, residual=best, mask=best_mask, masks=masks)


class _PairStateDriver(_SeededDriver):
    """What BatchedRegistration, BatchedHomography and BatchedPnP share: the constructor's common checks and attributes, the index sets of a round
    (Gumbel top-k or PROSAC, one seed per round), the train loop (_train_rounds: ops.SampleGather -> the family's differentiable fit) and the test
    loop on a per-pair state on the device (draw -> fit -> score -> update -> _after_update -> read-back of "does any pair continue?"),
    and the final stage: the refit, taken where it scores strictly higher, or under scoring="magsac" the IRLS polish.  The constructor
    checks the options of both families once.  A family sets `k`, `_columns` / `_shape_error`, `_State` and the ops `_fit`, `_fit_train`,
    `_score_msac`, `_score_magsac`, `_update`, `_refit` (or `_refit_candidate`, where the refit needs more than the mask), `_irls`, and switches on what it supports: local optimisation by taking `lo` /
    `lo_iters` and naming `_lo_width` and `_local_optimize`, device_termination by exposing `_device_termination_switch` under that
    name.  What else it does hangs on _begin, _fit and _finish."""

    _irls_strict = True      # irls_iters must be an int (no bool); False: whatever int() reads, as BatchedRegistration always took it

    def __init__(self, ransac_batch_size, threshold, confidence, max_iterations, tau, seed, refit, eps, train, sampling, prosac_draws,
                 scoring, irls_iters, lo=0, lo_iters=64):
        _check_lo(lo, lo_iters)
        if sampling not in ("gumbel", "prosac"):
            raise ValueError(f"sampling must be 'gumbel' or 'prosac', got {sampling!r}")
        if sampling == "prosac" and train:
            raise ValueError("sampling='prosac' yields index sets only: train mode needs the Gumbel sampler")
        self._set_prosac_draws(prosac_draws)
        self.sampling = sampling
        if int(max_iterations) < 1:
            raise ValueError(f"max_iterations must be at least 1, got {max_iterations!r}")
        if int(ransac_batch_size) < 1:
            raise ValueError(f"ransac_batch_size must be at least 1, got {ransac_batch_size!r}")
        self.B = int(ransac_batch_size)
        self.threshold = threshold
        self.confidence = confidence
        self.max_iterations = int(max_iterations)
        self.tau = tau
        self._seeds = _Seeds(seed)
        self.refit = refit
        self.eps = eps
        self.train = bool(train)
        if lo and train:
            raise ValueError("lo (local optimisation) is a test-mode step: lo != 0 with train=True is refused")
        _check_scoring(scoring, irls_iters if self._irls_strict else 0)
        if scoring == "magsac" and lo:
            raise ValueError("scoring='magsac' with lo != 0 is refused: dr_registration_local_opt scores its candidates with MSAC")
        if scoring == "magsac" and train:
            raise ValueError("scoring='magsac' with train=True is refused: train mode scores nothing")
        if int(irls_iters) < 0:
            raise ValueError(f"irls_iters must be at least 0, got {irls_iters!r}")
        self.lo = int(lo)
        self.lo_iters = int(lo_iters)
        self.scoring = scoring
        self.irls_iters = int(irls_iters)
        self._device_termination = False

    def _switch_device_termination(self, on):
        if on and self.rounds > 16:
            raise ValueError(f"device_termination issues every round: at most 16 rounds per call, this driver has {self.rounds} "
                             "(raise ransac_batch_size or lower max_iterations)")
        self._device_termination = bool(on)

    # device_termination = True: every round is issued, gated on the device, and nothing is read back (a family exposes it by this name)
    _device_termination_switch = property(lambda self: self._device_termination, _switch_device_termination)

    @property
    def rounds(self):
        """rounds a call can run at most"""
        return max(1, math.ceil(self.max_iterations / self.B))

    def __call__(self, matches, logits, gumbels=None):
        """`gumbels` (optional, list of [P,B,N] tensors, one per round) replaces the in-kernel noise: parity runs."""
        if matches.dim() != 3 or matches.shape[-1] != self._columns:
            raise ValueError(self._shape_error)
        if self.sampling == "prosac" and gumbels is not None:
            raise ValueError("sampling='prosac' draws index sets from the ranking of the logits: explicit noise is refused")
        rounds = self.rounds if gumbels is None else min(self.rounds, len(gumbels))
        if self.train:
            return self._train_rounds(matches, logits, gumbels, rounds)
        with torch.no_grad():
            logits = ops.L.aligned(logits)      # (a view that starts inside a larger buffer: realigned once per call, as c.matches is)
            c = self._begin(matches, rounds)
            c.order = c.growth = None
            if self.sampling == "prosac":      # the ranking of this call's logits and the growth table, once for all its rounds
                c.order, c.growth = self._prosac_setup(logits, c.N, c.matches.device)
            for r in range(rounds):
                idx = self._draw(c, r, logits, None if gumbels is None else gumbels[r])
                models, valid = self._fit(c, idx)
                scores = self._score(c, r, models, valid)
                self._update(c.st, c.matches, models, valid, scores, None, self.B, self.confidence, self.eps, thr2=c.thr2)
                self._after_update(c)
                if self._stop_after(c, r, rounds):
                    break
            return self._finish(c)

    def _train_rounds(self, matches, logits, gumbels, rounds):
        """the train loop: every round ops.SampleGather -> the family's differentiable fit, one seed per round; no state, no read-back"""
        self._check_train(matches, logits)
        out = []
        for r in range(rounds):
            g = None if gumbels is None else gumbels[r]
            samples, _, _ = ops.SampleGather.apply(matches, logits, self.B, self.k, self.tau, g, self._seeds.next())
            out.append(self._fit_train(samples))
        return dict(models=torch.cat([o[0] for o in out], 1), keep=torch.cat([o[1] for o in out], 1))

    def _check_train(self, matches, logits):
        pass

    def _begin(self, matches, rounds):
        """the state of a test-mode call: c.matches (contiguous), c.P, c.N, c.st, c.thr2, and under lo the buffers of the LO launches"""
        if self._device_termination and rounds > 16:      # (max_iterations / ransac_batch_size assigned after the switch)
            raise ValueError("device_termination issues every round: at most 16 rounds per call")
        P, N, _ = matches.shape
        matches = ops.L.aligned(matches.contiguous())
        st = self._State(P, N, self.max_iterations, matches.device, matches.dtype)
        c = types.SimpleNamespace(matches=matches, P=P, N=N, st=st, thr2=ops.thr2_tensor(self.threshold, P, matches))
        c.lo_seen = c.lo_refits = None
        if self.lo:
            c.lo_seen = torch.full((P, self._lo_width), float("nan"), device=matches.device, dtype=matches.dtype)
            c.lo_refits = torch.zeros(P, device=matches.device, dtype=torch.int32)
        return c

    def _draw(self, c, r, logits, g):
        """the index sets of round r; under PROSAC its rows are draws r B + 1 .. (r + 1) B (t0 goes by value: a captured call replays it)"""
        if self.sampling == "prosac":
            return ops.prosac_sample(c.order, c.growth, self.B, self.k, self._seeds.next(), r * self.B, P=c.P, N=c.N,
                                     device=c.matches.device)
        return ops.gumbel_topk(logits, self.B, self.k, self.tau, g, self._seeds.next(), soft=False)["idx"]

    def _score(self, c, r, models, valid):
        """round r's models under the driver's scoring, under device_termination gated on the device from the second round on;
        r = None: a refit candidate (MSAC)"""
        score_fn = self._score_magsac if (r is not None and self.scoring == "magsac") else self._score_msac
        if self._device_termination and r:
            return score_fn(c.matches, models, None, valid, want_inliers=False, gate=c.st, thr2=c.thr2)[0]
        return score_fn(c.matches, models, None, valid, want_inliers=False, thr2=c.thr2)[0]

    def _after_update(self, c):
        if self.lo:     # (gates itself on the device: pairs the round left alone return at once)
            self._local_optimize(c.st, c.matches, c.thr2, self.lo, self.lo_iters, self.confidence, self.eps, self.max_iterations,
                                 c.lo_seen, c.lo_refits)

    def _stop_after(self, c, r, rounds):
        """the read-back after round r: has every pair terminated (none under device_termination)"""
        return not self._device_termination and r + 1 < rounds and not bool((c.st.iters.double() < c.st.max_iters).any())

    def _refit_candidate(self, c):
        """the refit candidate of this call -> (model [P,.,.], valid [P]); a family whose refit needs more than the mask overrides it"""
        return self._refit(c.matches, c.st.best_mask)

    def _finish(self, c):
        model, score, extra = c.st.best_model, c.st.best_score, {}
        if self.scoring == "magsac":      # the IRLS polish in the single refit's place, in place on the state; the mask stays the RANSAC winner's
            extra["irls_fits"] = torch.zeros(c.P, device=c.matches.device, dtype=torch.int32)
            if self.refit and self.irls_iters > 0:
                self._irls(c.st, c.matches, c.thr2, self.irls_iters, extra["irls_fits"])
        elif self.refit:
            cand, cvalid = self._refit_candidate(c)
            cscore = self._score(c, None, cand.unsqueeze(1), cvalid.unsqueeze(1))
            take = cscore[:, 0] > score          # (an invalid candidate scores -1 or 0, a NaN never compares higher: neither wins)
            model = torch.where(take[:, None, None], cand, model)
            score = torch.where(take, cscore[:, 0], score)
        if self.lo:
            extra["lo_refits"] = c.lo_refits
        return dict(model=model, mask=c.st.best_mask, score=score, inliers=c.st.best_inliers, iterations=c.st.iters, **extra)


class BatchedRegistration(_PairStateDriver):
    """Robust rigid registration of point-cloud pairs: matches [P,N,6] = (p, q), logits [P,N] -> in test mode (the default)
    dict(model [P,4,4] = [[R, t], [0, 0, 0, 1]] with q ~ R p + t, mask [P,N], score [P], inliers [P], iterations [P]).

    One round = K1 Gumbel top-k (index sets of `num_samples` points) -> dr_kabsch_gather (the least-squares rigid fit of every
    sample: a correct Kabsch solver, not the reference's estimate_model that RANSAC3D / BatchedRANSAC3D reproduce) ->
    dr_rigid_msac_score (MSAC score and inlier count of every model against every point) -> dr_registration_update (arg-max,
    "better?" test, mask, adaptive stop with sample size 3, all per-pair state on the device).  The host reads back "does any
    pair continue?" after each round.  With `refit`, the Kabsch fit on the best mask replaces the model where it scores strictly
    higher; the mask stays the RANSAC winner's, as in the two-view path.

    `threshold` is a DISTANCE: a point is an inlier iff |q - (R p + t)|^2 < threshold^2 (BatchedRANSAC3D and
    ops.rigid_residual compare the squared distance with their threshold itself).

    device_termination = True issues every round, gated on the device, with no read-back, so that a call can be captured by
    graphs.GraphedStep; it is refused above 16 rounds.  Pipelining and super-rounds: not here.

    lo = 1 / 2 (test mode only): local optimisation on the device, one dr_registration_local_opt launch behind every
    dr_registration_update, in the same stream and with no read-back: a pair whose best model the round replaced gets one Kabsch refit
    on its inliers (lo = 1) or up to `lo_iters` of them (lo = 2), each kept only where it scores strictly higher; mask, inlier count
    and stop bound follow, so the read-back after the round sees the tightened bound, and the final `refit` starts from LO's mask.
    The result gains lo_refits [P], the fits run per pair.  lo = 0 is the path without it: no launch, no allocation, no key.

    scoring = "magsac" (test mode, lo = 0 only): every round is scored by dr_rigid_magsac_score, the MAGSAC++ loss with `threshold`
    as the cutoff distance k sigma_max (ops.rigid_magsac_score states the formulas); mask, inlier count and the adaptive stop keep
    using d2 < threshold^2.  With `refit` and irls_iters > 0 the final stage is dr_registration_irls: up to `irls_iters` re-weighted
    Kabsch fits over all points, each kept only where it scores strictly higher; the mask stays the RANSAC winner's.  The result gains
    irls_fits [P].  scoring = "msac" is the path without it: no other launch, allocation or key.

    edge_similarity = a float in (0, 1] (test mode only): every round fits its samples with dr_kabsch_gather_checked in
    dr_kabsch_gather's place.  A sample is dropped before the fit -- identity, valid = 0, so the score kernel skips it and the update
    ignores it -- unless sigma |q_i - q_j|^2 <= |p_i - p_j|^2 <= |q_i - q_j|^2 / sigma, sigma = edge_similarity^2, holds for every
    pair of its rows: a rigid motion keeps distances (Open3D's CorrespondenceCheckerBasedOnEdgeLength, similarity_threshold there).
    Every sample that passes gives the model it gives without the check, bit for bit, and a dropped draw still counts in `iterations`;
    nothing else of the round changes and nothing is read back.  The result gains rejected [P] int32, the samples dropped in the rounds
    the call issued: the fit is not gated on the device, so a pair that has terminated keeps counting while other pairs (or, under
    device_termination, the remaining rounds) go on.  None is the path without it: no other launch, allocation or key.  With
    train = True it is refused: a dropped outlier sample is exactly the hypothesis whose loss teaches the logits.

    sampling = "prosac" (test mode only): the logits are ranked once per call (ops.prosac_rank) and every round draws its index sets
    with ops.prosac_sample in ops.gumbel_topk's place, round r being PROSAC draws r B + 1 .. (r + 1) B of every pair: draw 1 is the
    `num_samples` best-ranked points, draw t takes the point of rank n(t) - 1 and points ranked above it, n(t) growing from
    num_samples to N over about `prosac_draws` draws (ops.prosac_growth; uniform over all points from there on).  O(B k) random words
    per round instead of O(B N); everything behind the index sets is unchanged, `tau` plays no part, and the adaptive stop stays the
    driver's own (PROSAC's non-randomness and maximality criteria are not implemented).  Refused with train = True and with explicit
    `gumbels`.  sampling = "gumbel" is the path without it: no other launch, allocation or key.

    train = True: every round runs (no adaptive stop, as in the reference's train branches), each one ops.SampleGather (the
    straight-through samples of the Gumbel top-k) followed by ops.kabsch, and the call returns dict(models [P, rounds * B, 4, 4],
    keep [P, rounds * B] = the fit's validity) with autograd to the logits, and to `matches` where they require it.  The pose loss on
    the returned models is loss.RegistrationLoss (pass `keep`).  `refit`, `confidence` and `device_termination` play no part, and nothing is read
    back to the host."""

    def __init__(self, ransac_batch_size=1024, threshold=0.05, confidence=0.999, max_iterations=5000, tau=1.0, seed=0,
                 num_samples=3, refit=True, eps=1e-5, train=False, lo=0, lo_iters=64, scoring="msac", irls_iters=10,
                 edge_similarity=None, sampling="gumbel", prosac_draws=200000):
        super().__init__(ransac_batch_size, threshold, confidence, max_iterations, tau, seed, refit, eps, train, sampling, prosac_draws,
                         scoring, irls_iters, lo, lo_iters)
        if edge_similarity is not None:
            if not 0.0 < float(edge_similarity) <= 1.0:      # (false for NaN)
                raise ValueError(f"edge_similarity must be None or lie in (0, 1], got {edge_similarity!r}")
            if train:
                raise ValueError("edge_similarity with train=True is refused: a rejected outlier sample is exactly the hypothesis "
                                 "whose loss teaches the logits, and dropping it would remove the training signal")
        if not 3 <= int(num_samples) <= 8:
            raise ValueError(f"num_samples must be between 3 and 8 points per sample, got {num_samples!r}")
        self.k = int(num_samples)
        self.edge_similarity = None if edge_similarity is None else float(edge_similarity)

    _irls_strict = False
    device_termination = _PairStateDriver._device_termination_switch
    _columns, _shape_error = 6, "matches must be [P,N,6] = (p, q)"
    _State = ops.RegistrationState
    _fit_train = staticmethod(ops.kabsch)
    _score_msac = staticmethod(ops.rigid_msac_score)
    _score_magsac = staticmethod(ops.rigid_magsac_score)
    _update = staticmethod(ops.registration_update)
    _refit = staticmethod(ops.refit_rigid)
    _irls = staticmethod(ops.registration_irls)
    _lo_width, _local_optimize = 17, staticmethod(ops.registration_local_optimize)

    def _begin(self, matches, rounds):
        c = super()._begin(matches, rounds)
        c.rejected = None
        if self.edge_similarity is not None:
            c.rejected = torch.zeros(c.P, device=matches.device, dtype=torch.int32)
        return c

    def _fit(self, c, idx):
        if c.rejected is None:
            return ops.kabsch_gather(c.matches, idx)
        return ops.kabsch_gather_checked(c.matches, idx, self.edge_similarity, c.rejected)

    def _finish(self, c):
        out = super()._finish(c)
        if c.rejected is not None:
            out["rejected"] = c.rejected
        return out


class BatchedHomography(_PairStateDriver):
    """Robust plane-induced homographies of image pairs: matches [P,N,4] = (x1, y1, x2, y2) in the caller's own coordinates (pixels;
    there is no K), logits [P,N] -> in test mode (the default) dict(model [P,3,3] = H with x2 ~ H x1, unit Frobenius norm and
    det H > 0, mask [P,N], score [P], inliers [P], iterations [P]).  The model for planar scenes and pure rotations, where the E and F
    solvers of BatchedRANSAC degenerate.

    One round = K1 Gumbel top-k (index sets of 4 points) -> dr_homography4_gather (the closed-form model of every sample; a sample
    with three collinear points or an orientation that differs between the images is dropped: identity, valid = 0) ->
    dr_homography_score (MSAC score of every model against every point under the symmetric transfer error) -> dr_homography_update
    (first arg-max, strictly-better test, mask, adaptive stop with sample size 4, all per-pair state on the device).  The host reads
    back "does any pair continue?" after each round.  With `refit`, the normalised DLT on the best mask (dr_refit_homography) replaces
    the model where it scores strictly higher; the mask stays the RANSAC winner's.

    `threshold` is a DISTANCE in the matches' units: a point is an inlier iff d2 < threshold^2, d2 = |x2 - H x1|^2 + |x1 - H^-1 x2|^2
    after the perspective divisions; a point that H or H^-1 sends behind the camera is an outlier.

    scoring = "magsac" (test mode only): every round is scored by dr_homography_magsac_score, the MAGSAC++ loss with `threshold` as
    the cutoff distance k sigma_max (the transfer error is a 4-vector: k^2 = chi2.ppf(0.99, 4); ops.homography_magsac_score states the
    formulas) -- the score for a caller who cannot choose a tight pixel threshold in advance.  Mask, inlier count and the adaptive stop
    keep using d2 < threshold^2.  With `refit` and irls_iters > 0 the final stage is dr_homography_irls in the single refit's place: up
    to `irls_iters` re-weighted DLT fits over the points inside the cutoff, each kept only where it scores strictly higher; the mask
    stays the RANSAC winner's.  The result gains irls_fits [P].  Combines with sampling = "prosac".  scoring = "msac" is the path
    without it: no other launch, allocation or key.

    sampling = "prosac" (test mode only): ops.prosac_sample in ops.gumbel_topk's place, round r being PROSAC draws r B + 1 .. (r + 1) B
    of every pair, as in BatchedRegistration.  Refused with train = True and with explicit `gumbels`.

    train = True: every round runs (no adaptive stop), each one ops.SampleGather followed by ops.homography4, and the call returns
    dict(models [P, rounds * B, 3, 3], keep [P, rounds * B] = the sample's validity) with autograd to the logits, and to `matches`
    where they require it.  `refit` and `confidence` play no part and nothing is read back.  The loss on the returned models is
    loss.HomographyLoss (pass `keep`).

    Not here: local optimisation, device_termination, super-rounds, samples of more than 4 points."""

    k = 4

    def __init__(self, ransac_batch_size=1024, threshold=3.0, confidence=0.999, max_iterations=5000, tau=1.0, seed=0, refit=True,
                 eps=1e-5, train=False, sampling="gumbel", prosac_draws=200000, scoring="msac", irls_iters=10):
        super().__init__(ransac_batch_size, threshold, confidence, max_iterations, tau, seed, refit, eps, train, sampling, prosac_draws,
                         scoring, irls_iters)

    _columns, _shape_error = 4, "matches must be [P,N,4] = (x1, y1, x2, y2)"
    _State = ops.HomographyState
    _fit_train = staticmethod(ops.homography4)
    _score_msac = staticmethod(ops.homography_score)
    _score_magsac = staticmethod(ops.homography_magsac_score)
    _update = staticmethod(ops.homography_update)
    _refit = staticmethod(ops.refit_homography)
    _irls = staticmethod(ops.homography_irls)

    def _check_train(self, matches, logits):
        if logits.dtype != matches.dtype:      # (the straight-through weights are read in the matches' type)
            raise ValueError(f"train mode needs logits of the matches' dtype, got {logits.dtype} and {matches.dtype}")

    def _fit(self, c, idx):
        return ops.homography4_gather(c.matches, idx)


class BatchedPnP(_PairStateDriver):
    """Robust absolute camera pose from 2D-3D matches: matches [P,N,5] = (X, Y, Z, u, v) -- a world point and its observation in
    NORMALISED image coordinates (the caller has applied K^-1; there is no K) --, logits [P,N] -> dict(model [P,4,4] =
    [[R, t], [0, 0, 0, 1]] with x_cam = R X + t, mask [P,N], score [P], inliers [P], iterations [P]).  The model layout is
    BatchedRegistration's, so loss.registration_errors gives RRE / RTE on it.

    One round = K1 Gumbel top-k (index sets of 3 points) -> dr_p3p_gather (the closed-form P3P poses of every sample: 4 slots per
    sample, the valid ones first; a degenerate sample has none) -> dr_pnp_score (MSAC score of all 4 B slots against every point under
    the reprojection error) -> dr_pnp_update (first arg-max, strictly-better test, mask, adaptive stop with sample size 3, all
    per-pair state on the device).  `iterations` advances by the B SAMPLES of a round, not by its 4 B slots.  The host reads back "does
    any pair continue?" after each round.  With `refit`, dr_refit_pnp -- at most `refit_iters` Levenberg-Marquardt passes on the
    reprojection error, from the state's best model over its best mask -- replaces the model where it scores strictly higher; the mask
    stays the RANSAC winner's.

    `threshold` is a DISTANCE in normalised units (pixels divided by the focal length): a point is an inlier iff
    d2 = (x_c / z_c - u)^2 + (y_c / z_c - v)^2 < threshold^2; a point with z_c <= 0 never counts.

    device_termination = True issues every round, gated on the device, with no read-back; it is refused above 16 rounds.
    sampling = "prosac": ops.prosac_sample in ops.gumbel_topk's place, as in BatchedRegistration; refused with explicit `gumbels`.

    hypotheses(matches, logits, gumbels=None) is the train-mode call: every round runs (no adaptive stop), each one ops.SampleGather
    (k = 3) followed by ops.p3p, and it returns dict(models [P, rounds * 4 B, 4, 4], keep [P, rounds * 4 B] = the slots' validity; slots
    4 b + j of a round belong to its sample b) with autograd to the logits, and to `matches` where they require it.  `refit`,
    `confidence` and `threshold` play no part, nothing is read back and no state is kept.  The loss on the returned models is
    loss.PnPLoss (pass `keep`).  It is a method, not the constructor's train = True, which stays refused.  Refused with
    ValueError: sampling = "prosac", device_termination switched on, logits of another dtype than the matches.

    Not here, each refused with NotImplementedError: train = True in the constructor (the train path is `hypotheses`),
    scoring = "magsac", lo != 0."""

    k = 3

    def __init__(self, ransac_batch_size=1024, threshold=0.005, confidence=0.999, max_iterations=5000, tau=1.0, seed=0, refit=True,
                 refit_iters=10, eps=1e-5, sampling="gumbel", prosac_draws=200000, train=False, scoring="msac", lo=0):
        if train:
            raise NotImplementedError("BatchedPnP(train=True): the train path of this family is the method BatchedPnP.hypotheses, "
                                      "not the constructor flag (DESIGN.md §8)")
        if scoring != "msac":
            raise NotImplementedError(f"BatchedPnP(scoring={scoring!r}): only MSAC scoring is built for this family (DESIGN.md §8)")
        if lo:
            raise NotImplementedError(f"BatchedPnP(lo={lo!r}): local optimisation is not built for this family (DESIGN.md §8)")
        super().__init__(ransac_batch_size, threshold, confidence, max_iterations, tau, seed, refit, eps, False, sampling, prosac_draws,
                         "msac", 0)
        if isinstance(refit_iters, bool) or int(refit_iters) != refit_iters or int(refit_iters) < 0:
            raise ValueError(f"refit_iters must be an integer of at least 0, got {refit_iters!r}")
        self.refit_iters = int(refit_iters)

    device_termination = _PairStateDriver._device_termination_switch
    _columns, _shape_error = 5, "matches must be [P,N,5] = (X, Y, Z, u, v)"
    _State = ops.PnPState
    _score_msac = staticmethod(ops.pnp_score)
    _update = staticmethod(ops.pnp_update)

    @staticmethod
    def _fit_train(samples):
        """samples [P,B,3,5] -> (models [P,4B,4,4], keep [P,4B]): the four slots of a sample side by side, as p3p_gather lays them out"""
        models, keep = ops.p3p(samples)
        return models.reshape(samples.shape[0], -1, 4, 4), keep.reshape(samples.shape[0], -1)

    def _check_train(self, matches, logits):
        if self.sampling == "prosac":
            raise ValueError("sampling='prosac' yields index sets only: hypotheses needs the Gumbel sampler")
        if self._device_termination:
            raise ValueError("hypotheses runs every round and keeps no state: a driver with device_termination switched on is refused")
        if logits.dtype != matches.dtype:      # (the straight-through weights are read in the matches' type)
            raise ValueError(f"hypotheses needs logits of the matches' dtype, got {logits.dtype} and {matches.dtype}")

    def hypotheses(self, matches, logits, gumbels=None):
        """the train-mode call (class docstring): dict(models [P, rounds * 4 B, 4, 4], keep [P, rounds * 4 B])"""
        if matches.dim() != 3 or matches.shape[-1] != self._columns:
            raise ValueError(self._shape_error)
        rounds = self.rounds if gumbels is None else min(self.rounds, len(gumbels))
        return self._train_rounds(matches, logits, gumbels, rounds)

    def _fit(self, c, idx):
        return ops.p3p_gather(c.matches, idx)

    def _refit_candidate(self, c):
        return ops.refit_pnp(c.matches, c.st.best_mask, c.st.best_model, self.refit_iters)
