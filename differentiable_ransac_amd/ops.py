"""Functional wrappers over the C ABI (include/dransac.h) for batched [P, ...] GPU tensors, and
the torch.autograd.Function classes built on them.  Every function enqueues on the current
torch stream and returns freshly allocated torch tensors; nothing synchronises.
"""
from __future__ import annotations

import collections
from typing import Optional, Tuple

import torch

from . import _lib as L
from ._lib import ptr, stream

# Round 6: the exponential-race form of the index-only sampler (one logarithm per element; dr_gumbel_topk_gather_f32's race_ws).
# Same top-k up to the rounding of near-ties; False = the two-logarithm form of rounds 1-5.
# These are plain constants, not configuration: the tests set the attributes to use the older forms as oracles of the newer ones.
K1_RACE = True
K1_RACE_SOFT = True          # ... in train mode (SampleGather's fused launch)
_RACE_MIN = (32768, 32)      # (rows, pairs) from which the form is chosen automatically (race_form_pays)
FUSED_SAMPLE_GATHER = True   # False = the two-launch forward / backward of rounds 1-4
FUSED_MATCH_LOSS = True      # False = the two-pass form of rounds 3-4

# Correspondences and points are read as float4 / float2 by kernels that have no scalar form: a contiguous view that starts inside a
# larger buffer (`packed[s:e]`, `flat[1:1 + n].view(P, N, 4)`) is copied to an aligned temporary on the way in (L.aligned: the tensor
# itself whenever it is aligned).  Read-only arguments only; the caller's tensor stays the one autograd saves and differentiates.
_al = L.aligned


def _u8(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """an optional bool tensor as the bytes the C ABI takes"""
    return None if t is None else t.contiguous().view(torch.uint8)


def _u8_ptr(t: Optional[torch.Tensor]):
    return ptr(_u8(t))


def _gate_args(gate):
    """the (iters, max_iters) pointer pair of a gated entry: gate = RansacState (a later round of a multi-round call, the blocks of
    terminated pairs return at once) or None"""
    return (ptr(None), ptr(None)) if gate is None else (ptr(gate.iters), ptr(gate.max_iters))


def _dev_seed(seed):
    if torch.is_tensor(seed):
        if seed.dtype != torch.int64 or seed.numel() != 1 or not seed.is_cuda:
            L._reset()      # (may be raised half-way through an argument list: see _lib.ptr)
            raise L.DransacError("a device seed is a one-element int64 CUDA tensor (DeviceSeed.next())")
        return True
    return False


def _seed_args(seed):
    """the (seed by value, seed on the device) argument pair of a sampler entry: an int goes by value, a DeviceSeed.next() tensor
    by pointer (read when the kernel starts)"""
    if _dev_seed(seed):
        return 0, ptr(seed)
    return seed & (2 ** 64 - 1), ptr(None)


def _thr_tensor(threshold, P: int, like: torch.Tensor) -> torch.Tensor:
    if isinstance(threshold, torch.Tensor):
        t = threshold.to(device=like.device, dtype=like.dtype).reshape(-1)
        if t.numel() == 1 and P > 1:
            t = t.expand(P)
        return t.contiguous()
    return torch.full((P,), float(threshold), device=like.device, dtype=like.dtype)


def _gpu_only(tensors, optional: bool = False) -> None:
    """what the wrappers that check their tensors before the launch refuse first; optional: a None among them is an absent argument"""
    for t in tensors:      # (a plain loop: this runs in front of launches of every round)
        if not optional if t is None else not t.is_cuda:
            raise L.DransacError("libdransac operates on GPU tensors only (got a CPU tensor)")


def _check_counter(name: str, what: str, t: Optional[torch.Tensor], P: int) -> None:
    """a per-pair counter a kernel adds to (irls_fits, lo_refits, rejected): [P] int32, or None where the caller may leave it out"""
    if t is not None and (t.shape != (P,) or t.dtype != torch.int32):
        raise L.DransacError(f"{name}: {what} must be [P] int32")


# ------------------------------------------------------------------------------------------ K4 / K6
def msac_score(matches: torch.Tensor, models: torch.Tensor, threshold, want_masks: bool = True,
               valid: Optional[torch.Tensor] = None, path: int = 0, gate=None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """matches [P,N,4], models [P,M,3,3] (or [P,M,9]) -> scores [P,M], masks [P,M,N] bool | None.
    valid [P,M] bool (optional): invalid slots are skipped (score 0, empty mask row).
    path: 0 = 1 = the general kernels; 2 (the matrix-core candidate filter of round 2, measured slower: DESIGN 2b) left the
    library in round 4 and is refused."""
    P, N, _ = matches.shape
    M = models.shape[1]
    matches = matches.contiguous()
    models = models.contiguous()
    thr = _thr_tensor(threshold, P, matches)
    scores = torch.empty((P, M), device=matches.device, dtype=matches.dtype)
    masks = torch.empty((P, M, N), device=matches.device, dtype=torch.bool) if want_masks else None
    v = _u8(valid)
    if path not in (0, 1):
        raise L.DransacError("msac_score: path must be 0 or 1 (the general kernels); path 2, the matrix-core candidate filter of "
                             "round 2, was measured slower and left the library (scratch/k4_filter_kernel.patch)")
    if matches.dtype == torch.float32:
        # gate (a later round of a multi-round call): the blocks of terminated pairs (gate = RansacState) return at once, their
        # scores are never looked at (dr_ransac_update skips such pairs)
        L.call("dr_msac_score_f32", ptr(_al(matches)), ptr(models), ptr(v), ptr(thr), P, M, N, ptr(scores), ptr(masks), *_gate_args(gate),
               stream())
        return scores, masks
    L.call(f"dr_msac_score_{L.suffix(matches.dtype)}", ptr(_al(matches)), ptr(models), ptr(v), ptr(thr), P, M, N, ptr(scores), ptr(masks),
           stream())
    return scores, masks


def magsac_score(matches: torch.Tensor, models: torch.Tensor, threshold, valid: Optional[torch.Tensor] = None, gate=None,
                 want_inliers: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """dr_magsac_score: matches [P,N,4], models [P,M,3,3] (or [P,M,9]), threshold as msac_score takes it (float or [P]; the cutoff is
    (1.5 thr)^2, read as (k sigma_max)^2 with k^2 = chi2.ppf(0.99, 4)) -> (scores [P,M] = sum_n (1 - l(s_n)), inliers [P,M] int32 =
    #{s_n < 1} | None); include/dransac.h states l.  msac_score's slot rules (invalid: exactly 0, non-finite or all-zero model: NaN),
    no mask rows.  Bit-repeatable.  gate = RansacState: the blocks of terminated pairs return at once."""
    if matches.dim() != 3 or matches.shape[-1] != 4:
        raise L.DransacError("magsac_score: correspondences are [P,N,4]")
    P, N, _ = matches.shape
    if models.dim() not in (3, 4) or models.shape[0] != P or models.shape[2:].numel() != 9:
        raise L.DransacError("magsac_score: models are [P,M,3,3] (or [P,M,9])")
    if models.dtype != matches.dtype or models.device != matches.device:
        raise L.DransacError("magsac_score: models must have the correspondences' dtype and device")
    M = models.shape[1]
    if valid is not None and (valid.shape != (P, M) or valid.dtype not in (torch.bool, torch.uint8)):
        raise L.DransacError("magsac_score: valid is [P,M] bool")
    thr = _thr_tensor(threshold, P, matches)
    scores = torch.empty((P, M), device=matches.device, dtype=matches.dtype)
    inliers = torch.empty((P, M), device=matches.device, dtype=torch.int32) if want_inliers else None
    L.call(f"dr_magsac_score_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), ptr(models.contiguous()), _u8_ptr(valid), ptr(thr),
           P, M, N, ptr(scores), ptr(inliers), *_gate_args(gate), stream())
    return scores, inliers


def magsac_irls(state: "RansacState", matches, thr, fundamental: bool, irls_iters: int, irls_fits: torch.Tensor,
                weights_ws: torch.Tensor) -> None:
    """dr_magsac_irls: the IRLS polish under the two-view MAGSAC++ loss, in place on state.best_model / state.best_score: up to
    irls_iters times the weights w(s) under the current model, the row-weighted refit over all points (F: LSQ 8-point, E: five-point
    on the weighted Gram matrix) and the candidates' MAGSAC++ scores, the best taken only where it is strictly higher.  thr [P] as
    ransac_init returns it; irls_fits [P] int32 grows by the fits run; weights_ws [P,N] (matches' dtype) is workspace.  Mask, inlier
    count and counters of the state are left alone.  One launch, no synchronisation."""
    _gpu_only((matches, thr, irls_fits, weights_ws, state.best_score, state.best_model))
    if matches.dim() != 3 or matches.shape[-1] != 4:
        raise L.DransacError("magsac_irls: correspondences are [P,N,4]")
    P, N, _ = matches.shape
    dt = matches.dtype
    if thr.shape != (P,) or thr.dtype != dt or not thr.is_contiguous():
        raise L.DransacError("magsac_irls: thr must be a contiguous [P] tensor of the matches' dtype")
    if (state.best_score.shape != (P,) or state.best_score.dtype != dt or state.best_model.shape != (P, 3, 3)
            or state.best_model.dtype != dt):
        raise L.DransacError("magsac_irls: the state's best_score [P] / best_model [P,3,3] must have the matches' dtype")
    _check_counter("magsac_irls", "irls_fits", irls_fits, P)
    if weights_ws.shape != (P, N) or weights_ws.dtype != matches.dtype or not weights_ws.is_contiguous():
        raise L.DransacError("magsac_irls: weights_ws must be a contiguous [P,N] tensor of the matches' dtype")
    L.call(f"dr_magsac_irls_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), ptr(thr), P, N, bool(fundamental), int(irls_iters),
           ptr(state.best_score), ptr(state.best_model), ptr(weights_ws), ptr(irls_fits), stream())


def select_best(matches: torch.Tensor, models: torch.Tensor, scores: torch.Tensor, threshold,
                valid: Optional[torch.Tensor] = None):
    """Per pair: (best_idx [P] int32, best_score [P], best_model [P,3,3], best_mask [P,N] bool, inliers [P] int32)."""
    P, N, _ = matches.shape
    M = models.shape[1]
    dev, dt = matches.device, matches.dtype
    thr = _thr_tensor(threshold, P, matches)
    best_idx = torch.empty((P,), device=dev, dtype=torch.int32)
    best_score = torch.empty((P,), device=dev, dtype=dt)
    best_model = torch.empty((P, 3, 3), device=dev, dtype=dt)
    best_mask = torch.empty((P, N), device=dev, dtype=torch.bool)
    inliers = torch.empty((P,), device=dev, dtype=torch.int32)
    L.call(f"dr_select_best_{L.suffix(dt)}", ptr(_al(matches.contiguous())), ptr(models.contiguous()), _u8_ptr(valid),
           ptr(scores.contiguous()), ptr(thr), P, M, N, ptr(best_idx), ptr(best_score), ptr(best_model), ptr(best_mask), ptr(inliers),
           stream())
    return best_idx, best_score, best_model, best_mask, inliers


class RansacState:
    """Per-pair test-mode state kept on the device (best score / model / mask / inlier count, iteration counters)."""

    def __init__(self, P: int, N: int, max_iterations: int, device, dtype, _init: bool = True, packed: bool = False):
        alloc = torch.zeros if _init else torch.empty
        self.packed = None
        if packed and P == 1 and dtype == torch.float32 and not _init:
            # one pair, f32: everything a call hands out in ONE buffer -- model 36 B | score 4 | iterations 4 | mask N -- so that the
            # replayed drop-in call (ransac._GraphedCall) returns it without a gather launch (round 6)
            self.packed = torch.empty(44 + N, device=device, dtype=torch.uint8)
            self.best_model = self.packed[:36].view(torch.float32).view(1, 3, 3)
            self.best_score = self.packed[36:40].view(torch.float32)
            self.iters = self.packed[40:44].view(torch.int32)
            self.best_mask = self.packed[44:].view(torch.bool).view(1, N)
        else:
            self.best_score = alloc(P, device=device, dtype=dtype)
            self.best_model = (torch.eye(3, device=device, dtype=dtype).repeat(P, 1, 1) if _init
                               else torch.empty(P, 3, 3, device=device, dtype=dtype))
            self.best_mask = alloc(P, N, device=device, dtype=torch.bool)
            self.iters = alloc(P, device=device, dtype=torch.int32)
        self.best_inliers = alloc(P, device=device, dtype=torch.int32)
        self.max_iters = (torch.full((P,), float(max_iterations), device=device, dtype=torch.float64) if _init
                          else torch.empty(P, device=device, dtype=torch.float64))
        self.max_iterations = max_iterations


def ransac_init(P: int, N: int, max_iterations: int, threshold: float, K1: Optional[torch.Tensor],
                K2: Optional[torch.Tensor], device, dtype, seeds=None, packed: bool = False,
                race_logits: Optional[torch.Tensor] = None) -> Tuple[RansacState, torch.Tensor]:
    """dr_ransac_init: the per-pair state and the threshold normalised as ransac.py:49-53 (K1/K2 [3,3] or [P,3,3];
    None = threshold used as is), in ONE launch.  Returns (state, thr [P]).
    seeds = (DeviceSeed, n): the same launch also draws the next n sampler keys (DeviceSeed.next_block(n)); they are returned as
    `state.seeds` ([n] int64).  packed: one pair, f32 -- the state lives in one buffer (RansacState.packed).
    race_logits [P,N] f32: the same launch writes the per-pair weights of the one-logarithm sampler -> `state.race_ws`, to be handed
    to gumbel_topk_gather(race_ws=...) by every round of the call."""
    st = RansacState(P, N, max_iterations, device, dtype, _init=False, packed=packed)
    st.seeds = None
    st.race_ws = None
    if race_logits is not None:
        if race_logits.dtype != torch.float32 or race_logits.shape != (P, N) or not race_logits.is_contiguous():
            raise L.DransacError("ransac_init: race_logits must be contiguous f32 [P,N]")
        st.race_ws = torch.empty((P, N + 32), device=device, dtype=torch.float32)
    seed_state = None
    n_seeds = 0
    if seeds is not None:
        seed_state, n_seeds = seeds[0].state, int(seeds[1])
        st.seeds = torch.empty(n_seeds, dtype=torch.int64, device=device)
    thr = torch.empty(P, device=device, dtype=dtype)
    k_stride = 0
    if K1 is not None:
        K1 = K1.to(device=device, dtype=dtype).contiguous()
        K2 = K2.to(device=device, dtype=dtype).contiguous()
        if K1.dim() == 3 and K1.shape[0] != 1:
            if K1.shape[0] != P or K2.shape != K1.shape:
                raise ValueError("K1/K2 must be [3,3] or [P,3,3]")
            k_stride = 9
    L.call(f"dr_ransac_init_{L.suffix(dtype)}", ptr(K1), ptr(K2), k_stride, float(threshold), P, N, max_iterations, ptr(thr),
           ptr(st.best_score), ptr(st.best_model), ptr(st.best_mask), ptr(st.best_inliers), ptr(st.iters), ptr(st.max_iters),
           ptr(seed_state), ptr(st.seeds), n_seeds, ptr(race_logits), ptr(st.race_ws), stream())
    return st, thr


def ransac_update(state: RansacState, matches, models, valid, scores, thr, B: int, k: int, confidence: float = 0.999,
                  eps: float = 1e-5, sub_models: int = 0) -> None:
    """K6 fused (dr_ransac_update): arg-max, best-model bookkeeping and adaptive termination, in place, one launch.
    sub_models > 0: the M models are consecutive sub-batches of B hypotheses (sub_models models each), walked in order with the
    stop rule of ransac.py:55-144 -- the state afterwards is the batch-by-batch loop's."""
    P, N, _ = matches.shape
    M = models.shape[1]
    if sub_models and M > sub_models * 512:
        raise L.DransacError("ransac_update: at most 512 sub-batches per launch")
    L.call(f"dr_ransac_update_{L.suffix(matches.dtype)}", ptr(_al(matches)), ptr(models.contiguous()), _u8_ptr(valid),
           ptr(scores.contiguous()), ptr(thr), P, M, N, B, k, confidence, eps, state.max_iterations, ptr(state.best_score),
           ptr(state.best_model), ptr(state.best_mask), ptr(state.best_inliers), ptr(state.iters), ptr(state.max_iters),
           int(sub_models), stream())


# ------------------------------------------------------------------------------------------ K1 / K1u / K2
def _lo_args(name: str, width: int, state, matches, thr, lo_seen, lo_refits, max_iterations):
    """what local_optimize and registration_local_optimize check before their launch (lo_seen is [P,width]) -> (P, N, max_iterations)"""
    _gpu_only((matches, thr, lo_seen, lo_refits, state.best_score, state.best_model, state.best_mask, state.best_inliers,
               state.max_iters), optional=True)
    P, N, _ = matches.shape
    if lo_seen is None or lo_seen.shape != (P, width) or lo_seen.dtype != matches.dtype or not lo_seen.is_contiguous():
        raise L.DransacError(f"{name}: lo_seen must be a contiguous [P,{width}] tensor of the matches' dtype")
    _check_counter(name, "lo_refits", lo_refits, P)
    return P, N, int(state.max_iterations if max_iterations is None else max_iterations)


def local_optimize(state: RansacState, matches, thr, fundamental: bool, lo: int, lo_iters: int, k: int,
                   confidence: float = 0.999, eps: float = 1e-5, max_iterations: Optional[int] = None,
                   lo_seen: Optional[torch.Tensor] = None, lo_refits: Optional[torch.Tensor] = None) -> None:
    """K7b (dr_local_opt): local optimisation of ransac.py:217-257 (lo = 1: one LSQ refit on the inliers, lo = 2: up to
    lo_iters), in place on `state`, for the pairs whose best model dr_ransac_update replaced since the last visit.
    lo_seen [P,10] (matches' dtype) is the per-call snapshot, filled with NaN before the first round; lo_refits [P] int32
    (optional) accumulates the refits run per pair.  One launch, no synchronisation."""
    P, N, mi = _lo_args("local_optimize", 10, state, matches, thr, lo_seen, lo_refits, max_iterations)
    L.call(f"dr_local_opt_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), ptr(thr), P, N, bool(fundamental), int(lo),
           int(lo_iters), int(k), confidence, eps, mi, ptr(state.best_score), ptr(state.best_model),
           ptr(state.best_mask.view(torch.uint8)), ptr(state.best_inliers), ptr(state.max_iters), ptr(lo_seen), ptr(lo_refits),
           stream())


class DeviceSeed:
    """The per-call sampler seed of the batched drivers, kept on the device: state = (base, calls) and `next()` launches
    dr_seed_next_n -> a one-word tensor holding base * 0x9E3779B97F4A7C15 + calls (mod 2^64), calls += 1.  The samplers
    accept such a tensor wherever they accept an int seed and read it when their kernel starts, so a step captured in a
    HIP graph (torch.cuda.graph) draws fresh hypotheses at every replay -- the same ones an eager driver with the same
    base seed draws at the same call number."""

    def __init__(self, base: int, device, calls: int = 0):
        def signed(v):
            v &= 2 ** 64 - 1
            return v - 2 ** 64 if v >= 2 ** 63 else v
        self.state = torch.tensor([signed(base), signed(calls)], dtype=torch.int64, device=device)

    def next(self) -> torch.Tensor:
        out = torch.empty(1, dtype=torch.int64, device=self.state.device)
        L.call("dr_seed_next_n", ptr(self.state), ptr(out), 1, stream())
        return out

    def next_block(self, n: int) -> torch.Tensor:
        """the seeds of the next n calls from ONE launch (a multi-round call draws one per batch) as one [n] tensor of CONSECUTIVE
        integers: seeds[i:i + 1] is what next() would have returned for call i"""
        out = torch.empty(n, dtype=torch.int64, device=self.state.device)
        L.call("dr_seed_next_n", ptr(self.state), ptr(out), n, stream())
        return out

    def next_n(self, n: int):
        """next_block(n) as a list of n one-word tensors"""
        out = self.next_block(n)
        return [out[i:i + 1] for i in range(n)]


def gumbel_topk(logits: Optional[torch.Tensor], B: int, k: int, tau: float = 1.0,
                gumbel: Optional[torch.Tensor] = None, seed: int = 0, N: Optional[int] = None,
                dense: bool = False, want_noise: bool = False, device=None, dtype=torch.float32, soft: bool = True,
                screen: Optional[bool] = None):
    """K1 forward.  logits [P,N] (or None = all-ones, then pass N/device/dtype); gumbel [P,B,N] explicit
    noise or None (in-kernel Philox keyed by `seed`).

    Returns dict(idx [P,B,k] int32 ascending, y_sel [P,B,k], lse [P,B]) plus, when `dense`,
    y_soft / ret [P,B,N], and when `want_noise`, gumbel [P,B,N] (the noise the kernel used).
    soft=False: index sets only (y_sel = lse = None) -- what test mode consumes; the same idx, a cheaper kernel.
    screen (index-only mode, rows longer than 2048 points): None = on when it can pay (B >= 64 rows per pair), False = off
    (A/B and tests: the index sets are the same either way)."""
    if not soft and dense:
        raise ValueError("the dense outputs need the soft-max statistics (soft=True)")
    if logits is not None:
        logits = logits.contiguous()
        P, N = logits.shape
        device, dtype = logits.device, logits.dtype
    else:
        P = 1 if gumbel is None else gumbel.shape[0]
        assert N is not None and device is not None
    if gumbel is not None:
        gumbel = gumbel.contiguous()
        assert gumbel.shape == (P, B, N) and gumbel.dtype == dtype
    idx = torch.empty((P, B, k), device=device, dtype=torch.int32)
    if (not soft and logits is not None and gumbel is None and not want_noise and dtype == torch.float32 and tau == 1.0
            and N > 2048 and N % 4 == 0 and k <= 5 and (B >= 64 if screen is None else screen)):
        # long rows, index sets only: the screened one-pass kernel (dr_gumbel_topk_index_f32; same index sets, bit for bit)
        ws = torch.empty(((N + 32) * P,), device=device, dtype=torch.int32)
        L.call("dr_gumbel_topk_index_f32", ptr(logits), *_seed_args(seed), tau, P, B, N, k, ptr(idx), ptr(ws), stream())
        return dict(idx=idx, y_sel=None, lse=None)
    y_sel = torch.empty((P, B, k), device=device, dtype=dtype) if soft else None
    lse = torch.empty((P, B), device=device, dtype=dtype) if soft else None
    y_soft = torch.empty((P, B, N), device=device, dtype=dtype) if dense else None
    ret = torch.empty((P, B, N), device=device, dtype=dtype) if dense else None
    noise = torch.empty((P, B, N), device=device, dtype=dtype) if want_noise else None
    if _dev_seed(seed) and (gumbel is not None or dense or want_noise or logits is None):
        raise L.DransacError("a device seed serves the in-kernel noise of given logits only (no explicit noise / dense outputs)")
    L.call(f"dr_gumbel_topk_fwd_{L.suffix(dtype)}", ptr(logits), ptr(gumbel), *_seed_args(seed), tau, P, B, N, k, ptr(idx), ptr(y_sel),
           ptr(lse), ptr(y_soft), ptr(ret), ptr(noise), stream())
    out = dict(idx=idx, y_sel=y_sel, lse=lse)
    if dense:
        out.update(y_soft=y_soft, ret=ret)
    if want_noise:
        out["gumbel"] = noise
    return out


def race_form_pays(P: int, B: int, N: int, tau: float) -> bool:
    """the automatic choice of the one-logarithm sampler: rows the register kernel serves, from 32 pairs / 32 768 rows on (the
    prologue costs a launch, the form saves ~0.12 us per 1024 rows of 2000 points: scratch/runs/r6_gpu_o.sh)"""
    return K1_RACE and P * B >= _RACE_MIN[0] and P >= _RACE_MIN[1] and N <= 2048 and N % 4 == 0 and tau == 1.0


def gumbel_topk_gather(matches: torch.Tensor, logits: torch.Tensor, B: int, k: int, tau: float = 1.0, seed=0, gate=None,
                       sub: int = 0, race: Optional[bool] = None, race_ws: Optional[torch.Tensor] = None):
    """K1 (index sets only, in-kernel noise) + K2 in one call: matches [P,N,4] f32, logits [P,N] f32 ->
    (idx [P,B,k] int32 ascending, samples [P,B,k,4] = matches[p, idx]).  What test mode asks of sampler + gather
    (ransac.py:58-65); `seed`: int or a DeviceSeed.next() tensor.
    sub > 0 (super-rounds): the B rows are consecutive sub-batches of `sub` rows; row b draws what row b % sub of the call with
    seed + b // sub draws (the drivers' per-call seeds are consecutive integers).
    race (None = automatic, race_form_pays): the one-logarithm exponential-race form of the same top-k (rows of <= 2048 points);
    race_ws: its per-pair weights, already computed for these logits by ransac_init(race_logits=...)."""
    if matches.dtype != torch.float32 or logits.dtype != torch.float32 or matches.shape[-1] != 4:
        raise L.DransacError("gumbel_topk_gather: f32 two-view correspondences [P,N,4]")
    matches, logits = matches.contiguous(), logits.contiguous()
    P, N = logits.shape
    idx = torch.empty((P, B, k), device=logits.device, dtype=torch.int32)
    samples = torch.empty((P, B, k, 4), device=logits.device, dtype=torch.float32)
    # race_ws: a workspace dr_ransac_init has already filled for these logits (ransac_init(race_logits=...)): no prologue launch
    ready = race_ws is not None and N <= 2048 and N % 4 == 0 and tau == 1.0
    want_race = not ready and (race_form_pays(P, B, N, tau) if race is None else race) and N <= 2048 and N % 4 == 0 and tau == 1.0
    rws = race_ws if ready else (torch.empty((P, N + 32), device=logits.device, dtype=torch.float32) if want_race else None)
    L.call("dr_gumbel_topk_gather_f32", ptr(logits), ptr(matches), *_seed_args(seed), tau, P, B, N, k, ptr(idx), ptr(samples),
           *_gate_args(gate), 0 if sub >= B else int(sub), ptr(rws), ready, stream())
    return idx, samples


def gumbel_topk_bwd(logits, gumbel, seed, tau, idx, lse, a_sel):
    """grad_logits [P,N] from a_sel [P,B,k] (f32; f64 with a by-value seed or explicit noise)."""
    P, B, k = idx.shape
    N = logits.shape[1]
    grad = torch.empty_like(logits)
    if logits.dtype == torch.float64:
        if _dev_seed(seed):
            raise L.DransacError("gumbel_topk_bwd: device seeds serve f32 only")
        L.call("dr_gumbel_topk_bwd_f64", ptr(logits.contiguous()), ptr(gumbel), seed & (2 ** 64 - 1), tau, P, B, N, k, ptr(idx),
               ptr(lse.contiguous()), ptr(a_sel.to(torch.float64).contiguous()), ptr(grad), stream())
        return grad
    L.call("dr_gumbel_topk_bwd_f32", ptr(logits.contiguous()), ptr(None if _dev_seed(seed) else gumbel), *_seed_args(seed), tau, P, B,
           N, k, ptr(idx), ptr(lse), ptr(a_sel.contiguous()), ptr(grad), stream())
    return grad


def topdown_sample(logits: Optional[torch.Tensor], B: int, k: int, seed: int = 0, N: Optional[int] = None, P: int = 1,
                   device=None) -> torch.Tensor:
    """K1, inference variant (dr_topdown_sample): the Gumbel top-k INDEX SET drawn top-down -- k sequential draws
    without replacement from softmax(logits), the exact distribution of the top-k of logits + iid Gumbel(0,1) for any
    tau > 0 -- in O(B k log N).  logits [P,N] (or None = uniform: pass N, P, device) -> idx [P,B,k] int32 ascending.
    No y_sel / lse: train mode and weighted mode need the whole noise row (use gumbel_topk)."""
    if logits is not None:
        logits = logits.contiguous()
        P, N = logits.shape
        device = logits.device
        sfx = L.suffix(logits.dtype)
    else:
        sfx = "f32"
    ws = torch.empty((P, N), device=device, dtype=torch.float64)
    idx = torch.empty((P, B, k), device=device, dtype=torch.int32)
    if sfx == "f32":
        L.call("dr_topdown_sample_f32", ptr(logits), *_seed_args(seed), P, B, N, k, ptr(ws), ptr(idx), stream())
        return idx
    if _dev_seed(seed):
        raise L.DransacError("device seeds: f32 logits")
    L.call("dr_topdown_sample_f64", ptr(logits), _seed_args(seed)[0], P, B, N, k, ptr(ws), ptr(idx), stream())
    return idx


def uniform_sample(P: int, B: int, k: int, N: int, seed: int, device) -> torch.Tensor:
    """K1u: idx [P,B,k] int32 ~ U{0..N-2} (uniform_sampler.py:15-19 semantics)."""
    idx = torch.empty((P, B, k), device=device, dtype=torch.int32)
    L.call("dr_uniform_sample", *_seed_args(seed), P, B, k, N, ptr(idx), stream())
    return idx


def prosac_rank(logits: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """The ranking PROSAC samples from: order [P,N] int32, the points of every pair by descending logit, ties by ascending index,
    NaN logits last (-0.0 ranks with 0.0).  None stays None: no order, the sampler reads the identity."""
    if logits is None:
        return None
    # (l + 0.0 turns -0.0 into +0.0: a radix sort would tell their bit patterns apart)
    key = torch.where(torch.isnan(logits), torch.full_like(logits, float("-inf")), logits + 0.0)
    return torch.sort(key, dim=1, descending=True, stable=True).indices.to(torch.int32).contiguous()


def prosac_growth(N: int, k: int, prosac_draws: int = 200000, device=None) -> torch.Tensor:
    """PROSAC's growth function as a table, int64 [N - k + 1] on `device` (a CPU device works too): entry i is T'_{k+i}, the draw
    number up to which the sampler works on the k + i best-ranked points.  T_n = T_N prod_{i<k} (n - i) / (N - i) in f64 (one division
    and one multiplication per factor, in this order), T'_k = 1, T'_n = 1 + sum_{j=k+1..n} ceil(T_j - T_{j-1}): strictly increasing,
    and n(t) <= k + t - 1.  T_N = prosac_draws, the number of draws after which the sampler is uniform over all points."""
    N, k, T_N = int(N), int(k), int(prosac_draws)
    if k < 1 or N < k or T_N < 1:
        raise ValueError(f"prosac_growth needs 1 <= k <= N and prosac_draws >= 1, got N={N}, k={k}, prosac_draws={prosac_draws}")
    n = torch.arange(k, N + 1, device=device, dtype=torch.float64)
    T = torch.full_like(n, float(T_N))
    for i in range(k):
        T = T * ((n - float(i)) / float(N - i))
    steps = torch.ceil(T[1:] - T[:-1]).to(torch.int64)
    return torch.cat([torch.ones(1, device=device, dtype=torch.int64), 1 + torch.cumsum(steps, 0)])


def prosac_sample(order: Optional[torch.Tensor], growth: torch.Tensor, B: int, k: int, seed=0, t0: int = 0,
                  P: Optional[int] = None, N: Optional[int] = None, device=None) -> torch.Tensor:
    """K1p (dr_prosac_sample): draws t0 + 1 .. t0 + B of the PROSAC sampler for every pair -> idx [P,B,k] int32 ascending.
    order [P,N] int32 from prosac_rank (or None = the identity: pass P, N, device), growth from prosac_growth(N, k, ...);
    `seed`: int or a DeviceSeed.next() tensor.  Draw 1 is the k best-ranked points; O(B k) work whatever N is."""
    if order is not None:
        if order.dtype != torch.int32 or order.dim() != 2:
            raise L.DransacError("prosac_sample: order is an int32 [P,N] tensor (prosac_rank)")
        order = order.contiguous()
        P, N = order.shape
        device = order.device
    else:
        assert P is not None and N is not None and device is not None
    if growth.dtype != torch.int64 or growth.numel() != N - k + 1:
        raise L.DransacError("prosac_sample: growth is the int64 [N - k + 1] table of prosac_growth(N, k, ...)")
    idx = torch.empty((P, B, k), device=device, dtype=torch.int32)
    L.call("dr_prosac_sample", ptr(order), ptr(growth.contiguous()), *_seed_args(seed), int(t0), P, B, N, k, ptr(idx), stream())
    return idx


def gather(matches: torch.Tensor, idx: torch.Tensor, y_sel: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K2 forward: matches [P,N,c], idx [P,B,k] -> samples [P,B,k,c] (times the straight-through value)."""
    P, N, c = matches.shape
    _, B, k = idx.shape
    out = torch.empty((P, B, k, c), device=matches.device, dtype=matches.dtype)
    L.call(f"dr_gather_fwd_{L.suffix(matches.dtype)}", ptr(matches.contiguous()), ptr(idx), ptr(y_sel), P, N, B, k, c, ptr(out),
           stream())
    return out


def gather_bwd(matches, idx, y_sel, grad_samples, grad_w=None, want_grad_matches=False):
    P, N, c = matches.shape
    _, B, k = idx.shape
    a_sel = torch.empty((P, B, k), device=matches.device, dtype=matches.dtype)
    gm = torch.zeros_like(matches) if want_grad_matches else None
    dt = matches.dtype
    L.call(f"dr_gather_bwd_{L.suffix(dt)}", ptr(matches.contiguous()), ptr(idx), ptr(y_sel), ptr(grad_samples.to(dt).contiguous()),
           ptr(None if grad_w is None else grad_w.to(dt).contiguous()), P, N, B, k, c, ptr(a_sel), ptr(gm), stream())
    return a_sel, gm


class SampleGather(torch.autograd.Function):
    """K1+K2 fused at the autograd level: (matches [P,N,c], logits [P,N]) -> samples [P,B,k,c], weights [P,B,k].

    Forward: dr_gumbel_topk_fwd + dr_gather_fwd (no [B,N] tensor is materialised).
    Backward: dr_gather_bwd -> a_sel, dr_gumbel_topk_bwd -> grad_logits (f32 and f64)."""

    @staticmethod
    def forward(ctx, matches, logits, B, k, tau, gumbel, seed):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        if logits.dtype == torch.float64 and logits.requires_grad and gumbel is None and _dev_seed(seed):
            # refused HERE, not at backward time (round-4 advice): the f64 sampler backward takes a by-value seed or explicit noise
            raise L.DransacError("SampleGather: f64 logits with a device seed have no backward (device seeds serve f32 only)")
        fused = (FUSED_SAMPLE_GATHER and gumbel is None and logits.dtype == torch.float32 and matches.dtype == torch.float32
                 and matches.shape[-1] == 4)
        if fused:
            # round 5: sampler (soft-max statistics) + gather in ONE launch, and one launch back (dr_gumbel_topk_gather_soft_f32 /
            # dr_gumbel_topk_gather_bwd_f32): same index sets, weights and samples as the two-launch form, bit for bit
            matches, logits = matches.contiguous(), logits.contiguous()
            P, N = logits.shape
            # (realigned copies for the launch only: what is saved, and what the gradient belongs to, stays the caller's view)
            lg_in, mt_in = _al(logits), _al(matches)
            r = dict(idx=torch.empty((P, B, k), device=logits.device, dtype=torch.int32),
                     y_sel=torch.empty((P, B, k), device=logits.device, dtype=torch.float32),
                     lse=torch.empty((P, B), device=logits.device, dtype=torch.float32))
            samples = torch.empty((P, B, k, 4), device=logits.device, dtype=torch.float32)
            # round 6: the one-logarithm form in train mode too (keys, winners and soft-max statistics from one logarithm and one
            # reciprocal per element), where its weights prologue pays
            rws = (torch.empty((P, N + 32), device=logits.device, dtype=torch.float32)
                   if K1_RACE_SOFT and race_form_pays(P, B, N, tau) else None)
            L.call("dr_gumbel_topk_gather_soft_f32", ptr(lg_in), ptr(mt_in), *_seed_args(seed), tau, P, B, N, k, ptr(r["idx"]),
                   ptr(r["y_sel"]), ptr(r["lse"]), ptr(samples), ptr(rws), stream())
        else:
            r = gumbel_topk(logits, B, k, tau, gumbel, seed)
            samples = gather(matches, r["idx"], r["y_sel"])
        ctx.save_for_backward(matches, logits, r["idx"], r["y_sel"], r["lse"], gumbel if gumbel is not None else
                              torch.empty(0, device=logits.device))
        ctx.cfg = (tau, seed, gumbel is not None)
        ctx.fused = fused
        ctx.mark_non_differentiable(r["idx"])
        return samples, r["y_sel"], r["idx"]

    @staticmethod
    def backward(ctx, g_samples, g_w, _g_idx):
        if g_samples is None and g_w is None:
            return (None,) * 7
        matches, logits, idx, y_sel, lse, gumbel = ctx.saved_tensors
        if g_samples is None:
            g_samples = torch.zeros(idx.shape + (matches.shape[-1],), device=matches.device, dtype=matches.dtype)
        tau, seed, has_noise = ctx.cfg
        if ctx.fused and not ctx.needs_input_grad[0]:
            P, B, k = idx.shape
            gl = torch.empty_like(logits)
            L.call("dr_gumbel_topk_gather_bwd_f32", ptr(_al(logits)), ptr(_al(matches)), *_seed_args(seed), tau, P, B, logits.shape[1], k,
                   ptr(idx), ptr(lse), ptr(g_samples.contiguous()), ptr(None if g_w is None else g_w.contiguous()), ptr(gl), stream())
            return None, gl, None, None, None, None, None
        a_sel, gm = gather_bwd(matches, idx, y_sel, g_samples, g_w, want_grad_matches=ctx.needs_input_grad[0])
        gl = gumbel_topk_bwd(logits, gumbel if has_noise else None, seed, tau, idx, lse, a_sel)
        return gm, gl, None, None, None, None, None


# ------------------------------------------------------------------------------------------ K3 solvers
def _flat_samples(samples: torch.Tensor, c: int):
    s = samples.reshape(-1, samples.shape[-2], c).contiguous()
    return s, s.shape[0], s.shape[1]


def _solver_gate(gate, s: torch.Tensor, n: int):
    """gate = (RansacState, rows per pair) of solve_nister5 / solve_stewenius5 -> (rows per pair, state), (0, None) without one"""
    if gate is None:
        return 0, None
    if n != 5 or s.dtype != torch.float32:
        raise L.DransacError("the gated five-point entries take f32 minimal samples")
    return int(gate[1]), gate[0]


def solve_nister5(samples: torch.Tensor, weights: Optional[torch.Tensor] = None, path: int = 0, gate=None):
    """samples [..., n>=5, 4] -> models [..., 10, 3, 3], valid [..., 10] bool (real solutions, ascending root).
    path (f32 minimal samples only): 0 automatic, 1 lane-pair kernel, 2 two-phase kernel (include/dransac.h).
    gate = (RansacState, rows per pair), f32 minimal samples [P,B,5,4] of a later round of a multi-round test-mode call: the blocks
    of pairs that have terminated (iters >= max_iters) return at once and leave their part of the outputs unwritten --
    dr_ransac_update never looks at it."""
    s, Bt, n = _flat_samples(samples, 4)
    lead = samples.shape[:-2]
    models = torch.empty((Bt, 10, 3, 3), device=s.device, dtype=s.dtype)
    valid = torch.empty((Bt, 10), device=s.device, dtype=torch.bool)
    w = None if weights is None else weights.reshape(Bt, n).to(s.dtype).contiguous()
    if path != 0 and (n != 5 or s.dtype != torch.float32):
        raise L.DransacError("an explicit five-point kernel path exists for f32 minimal samples only")
    rows, st = _solver_gate(gate, s, n)
    if s.dtype == torch.float32:
        L.call("dr_solve_nister5_f32", ptr(s), ptr(w), Bt, n, ptr(models), ptr(None), ptr(valid), path, rows, *_gate_args(st),
               stream())
    else:
        L.call(f"dr_solve_nister5_{L.suffix(s.dtype)}", ptr(s), ptr(w), Bt, n, ptr(models), ptr(valid), stream())
    return models.reshape(*lead, 10, 3, 3), valid.reshape(*lead, 10)


def solve_nister5_hp(samples: torch.Tensor, weights: Optional[torch.Tensor] = None, path: int = 0):
    """Minimal f32 samples [..., 5, 4] -> (models f32, models f64, valid): the train-mode entry, one launch."""
    s, Bt, n = _flat_samples(samples, 4)
    if n != 5 or s.dtype != torch.float32:
        raise L.DransacError("solve_nister5_hp takes f32 minimal samples (5 correspondences)")
    lead = samples.shape[:-2]
    models = torch.empty((Bt, 10, 3, 3), device=s.device, dtype=torch.float32)
    m64 = torch.empty((Bt, 10, 3, 3), device=s.device, dtype=torch.float64)
    valid = torch.empty((Bt, 10), device=s.device, dtype=torch.bool)
    w = None if weights is None else weights.reshape(Bt, n).to(s.dtype).contiguous()
    L.call("dr_solve_nister5_f32", ptr(s), ptr(w), Bt, 5, ptr(models), ptr(m64), ptr(valid), path, 0, ptr(None), ptr(None), stream())
    return models.reshape(*lead, 10, 3, 3), m64.reshape(*lead, 10, 3, 3), valid.reshape(*lead, 10)


def solve_essential_gated(samples: torch.Tensor, which: str, gate):
    """A later round of a multi-round test-mode call: samples [P,B,5,4] f32 -> (models [P,B,10,3,3], valid [P,B,10]), the pairs
    that have terminated (gate = RansacState) skipped: solve_nister5 / solve_stewenius5 with `gate=`."""
    return (solve_nister5 if which == "nister" else solve_stewenius5)(samples, gate=(gate, samples.shape[1]))


def debug_real_roots10(coef: torch.Tensor, method: int = 1):
    """Test hook (dr_debug_real_roots10): coef [n,11] f64 ascending -> roots [n,2,10] f64, counts [n,2] int32; half 0 = |z| <= 1,
    half 1 = |z| > 1; method 0 = derivative chain, 1 = Sturm isolation (what the five-point kernels run)."""
    coef = coef.to(torch.float64).contiguous()
    n = coef.shape[0]
    roots = torch.zeros((n, 2, 10), device=coef.device, dtype=torch.float64)
    counts = torch.zeros((n, 2), device=coef.device, dtype=torch.int32)
    L.call("dr_debug_real_roots10", ptr(coef), n, method, ptr(roots), ptr(counts), stream())
    return roots, counts


def solve_stewenius5(samples: torch.Tensor, path: int = 0, gate=None):
    """samples [..., 5, 4] -> models [..., 10, 3, 3], valid [..., 10].  path, gate: as solve_nister5 (f32 only)."""
    s, Bt, n = _flat_samples(samples, 4)
    if n != 5:
        raise L.DransacError("the Stewenius solver takes exactly 5 correspondences per sample")
    lead = samples.shape[:-2]
    models = torch.empty((Bt, 10, 3, 3), device=s.device, dtype=s.dtype)
    valid = torch.empty((Bt, 10), device=s.device, dtype=torch.bool)
    if path != 0 and s.dtype != torch.float32:
        raise L.DransacError("an explicit five-point kernel path exists for f32 minimal samples only")
    rows, st = _solver_gate(gate, s, n)
    if s.dtype == torch.float32:
        L.call("dr_solve_stewenius5_f32", ptr(s), Bt, ptr(models), ptr(valid), path, rows, *_gate_args(st), stream())
    else:
        L.call(f"dr_solve_stewenius5_{L.suffix(s.dtype)}", ptr(s), Bt, ptr(models), ptr(valid), stream())
    return models.reshape(*lead, 10, 3, 3), valid.reshape(*lead, 10)


def solve_f8(samples: torch.Tensor, weights: Optional[torch.Tensor] = None):
    """samples [..., n>=8, 4] -> F [..., 3, 3], valid [...] bool."""
    s, Bt, n = _flat_samples(samples, 4)
    lead = samples.shape[:-2]
    models = torch.empty((Bt, 3, 3), device=s.device, dtype=s.dtype)
    valid = torch.empty((Bt,), device=s.device, dtype=torch.bool)
    w = None if weights is None else weights.reshape(Bt, n).to(s.dtype).contiguous()
    L.call(f"dr_solve_f8_{L.suffix(s.dtype)}", ptr(s), ptr(w), Bt, n, ptr(models), ptr(valid), stream())
    return models.reshape(*lead, 3, 3), valid.reshape(lead)


def solve_f8_uniform(matches: torch.Tensor, B: int, seed):
    """K1u + K2 + K3f8 in one launch (f32): matches [P,N,4] -> (idx [P,B,8] int32, F [P,B,3,3], valid [P,B] bool); the index sets
    are those of uniform_sample(P, B, 8, N, seed), the models those of solve_f8(gather(matches, idx))."""
    if matches.dtype != torch.float32 or matches.shape[-1] != 4:
        raise L.DransacError("solve_f8_uniform: f32 correspondences [P,N,4]")
    P, N, _ = matches.shape
    idx = torch.empty((P, B, 8), device=matches.device, dtype=torch.int32)
    models = torch.empty((P, B, 3, 3), device=matches.device, dtype=torch.float32)
    valid = torch.empty((P, B), device=matches.device, dtype=torch.bool)
    L.call("dr_solve_f8_uniform_f32", ptr(_al(matches.contiguous())), *_seed_args(seed), P, B, N, ptr(idx), ptr(models), ptr(valid),
           stream())
    return idx, models, valid


def solve_f7(samples: torch.Tensor):
    s, Bt, n = _flat_samples(samples, 4)
    if n != 7:
        raise L.DransacError("the 7-point solver takes exactly 7 correspondences per sample")
    lead = samples.shape[:-2]
    models = torch.empty((Bt, 4, 3, 3), device=s.device, dtype=s.dtype)
    valid = torch.empty((Bt, 4), device=s.device, dtype=torch.bool)
    L.call(f"dr_solve_f7_{L.suffix(s.dtype)}", ptr(s), Bt, ptr(models), ptr(valid), stream())
    return models.reshape(*lead, 4, 3, 3), valid.reshape(*lead, 4)


def solve_rigid(samples: torch.Tensor, weights: Optional[torch.Tensor] = None, flag: bool = True):
    """samples [..., n>=3, 6] -> model [...,4,4], R [...,3,3], t [...,3], scale [...], valid [...] bool."""
    s, Bt, n = _flat_samples(samples, 6)
    lead = samples.shape[:-2]
    dev, dt = s.device, s.dtype
    model = torch.empty((Bt, 4, 4), device=dev, dtype=dt)
    R = torch.empty((Bt, 3, 3), device=dev, dtype=dt)
    t = torch.empty((Bt, 3), device=dev, dtype=dt)
    scale = torch.empty((Bt,), device=dev, dtype=dt)
    valid = torch.empty((Bt,), device=dev, dtype=torch.bool)
    w = None if weights is None else weights.reshape(Bt, n).to(dt).contiguous()
    L.call(f"dr_solve_rigid_{L.suffix(dt)}", ptr(s), ptr(w), Bt, n, bool(flag), ptr(model), ptr(R), ptr(t), ptr(scale), ptr(valid),
           stream())
    return (model.reshape(*lead, 4, 4), R.reshape(*lead, 3, 3), t.reshape(*lead, 3), scale.reshape(lead),
            valid.reshape(lead))


def solve_rigid_gather(matches: torch.Tensor, idx: torch.Tensor, flag: bool = True, zero_sums: Optional[torch.Tensor] = None):
    """K2 + K3r in one launch (f32): matches [P,N,6], idx [P,B,k] int32 -> (model [P,B,4,4], valid [P,B] bool), the samples read
    through the index sets; zero_sums [P,B] (optional) is cleared by the same launch (the residual sums of the round:
    rigid_residual(..., res=zero_sums) then needs no memset)."""
    if matches.dtype != torch.float32 or matches.shape[-1] != 6:
        raise L.DransacError("solve_rigid_gather: f32 correspondences [P,N,6]")
    P, N, _ = matches.shape
    _, B, k = idx.shape
    model = torch.empty((P, B, 4, 4), device=matches.device, dtype=torch.float32)
    valid = torch.empty((P, B), device=matches.device, dtype=torch.bool)
    L.call("dr_solve_rigid_gather_f32", ptr(_al(matches.contiguous())), ptr(idx.contiguous()), P, B, N, k, bool(flag), ptr(model),
           ptr(None), ptr(None), ptr(None), ptr(valid), ptr(zero_sums), stream())
    return model, valid


def rigid_residual(pts: torch.Tensor, models: torch.Tensor, threshold: float = 0.03, want_masks: bool = True,
                   res: Optional[torch.Tensor] = None):
    """pts [P,N,6], models [P,M,4,4] -> res_sum [P,M], masks [P,M,N] bool | None.
    res (f32, optional): a [P,M] tensor of ZEROS to add the sums to (no memset launch): solve_rigid_gather(..., zero_sums=res)."""
    P, N, _ = pts.shape
    M = models.shape[1]
    masks = torch.empty((P, M, N), device=pts.device, dtype=torch.bool) if want_masks else None
    if res is not None:
        if pts.dtype != torch.float32 or res.shape != (P, M) or res.dtype != torch.float32:
            raise L.DransacError("rigid_residual: res must be an f32 [P,M] tensor of zeros")
        L.call("dr_rigid_residual_f32", ptr(_al(pts.contiguous(), 8)), ptr(models.contiguous()), threshold, P, M, N, ptr(res), ptr(masks), 1,
               stream())
        return res, masks
    res = torch.empty((P, M), device=pts.device, dtype=pts.dtype)
    if pts.dtype == torch.float32:
        L.call("dr_rigid_residual_f32", ptr(_al(pts.contiguous(), 8)), ptr(models.contiguous()), threshold, P, M, N, ptr(res), ptr(masks), 0,
               stream())
    else:
        L.call(f"dr_rigid_residual_{L.suffix(pts.dtype)}", ptr(_al(pts.contiguous(), 8)), ptr(models.contiguous()), threshold, P, M, N,
               ptr(res), ptr(masks), stream())
    return res, masks


def ransac3d_update(pts: torch.Tensor, models: torch.Tensor, valid: Optional[torch.Tensor], res: torch.Tensor,
                    threshold: float, best_res: Optional[torch.Tensor], best_model: Optional[torch.Tensor],
                    best_mask: Optional[torch.Tensor] = None):
    """K6 of the 3-D path (dr_ransac3d_update): per pair the valid model with the smallest residual sum replaces the state
    where it is strictly better.  pts [P,N,6], models [P,M,4,4], valid [P,M] | None, res [P,M]; state best_res [P],
    best_model [P,4,4] -> NEW (best_res, best_model) tensors (the small state is ping-ponged), best_mask [P,N] updated in
    place, idx [P] int32 = the round's winner or -1."""
    P, N, _ = pts.shape
    M = models.shape[1]
    # best_res = best_model = None: the first round (state = +inf / identity / empty mask, nothing to allocate or fill)
    out_res = torch.empty((P,), device=pts.device, dtype=pts.dtype)
    out_model = torch.empty((P, 4, 4), device=pts.device, dtype=pts.dtype)
    idx = torch.empty((P,), device=pts.device, dtype=torch.int32)
    mk = None if best_mask is None else best_mask.view(torch.uint8)
    L.call(f"dr_ransac3d_update_{L.suffix(pts.dtype)}", ptr(_al(pts.contiguous(), 8)), ptr(models.contiguous()), _u8_ptr(valid),
           ptr(res.contiguous()), threshold, P, M, N, ptr(None if best_res is None else best_res.contiguous()),
           ptr(None if best_model is None else best_model.contiguous()), ptr(out_res), ptr(out_model), ptr(mk), ptr(idx), stream())
    return out_res, out_model, idx


# ------------------------------------------------------------------------------------------ robust 3-D registration
# matches [P,N,6] = (p, q), models [.,4,4] = [[R, t], [0, 0, 0, 1]], q_hat = R p + t.  `threshold` is a DISTANCE here: a point is an
# inlier iff |q - q_hat|^2 < threshold^2 (rigid_residual compares the squared distance with its threshold itself).
def thr2_tensor(threshold, P: int, like: torch.Tensor) -> torch.Tensor:
    """threshold^2 per pair, [P] in the correspondences' dtype: what the kernels take (a driver computes it once per call and hands
    it to the wrappers below as `thr2=`)"""
    t = _thr_tensor(threshold, P, like)
    return t * t


def kabsch_gather(matches: torch.Tensor, idx: torch.Tensor):
    """dr_kabsch_gather: matches [P,N,6], idx [P,B,k] int32 (3 <= k <= 8) -> (models [P,B,4,4], valid [P,B] bool): the least-squares
    rigid fit (Kabsch) of every sample; a degenerate sample (coincident / collinear rows) is the identity with valid = 0."""
    if matches.dim() != 3 or matches.shape[-1] != 6 or idx.dim() != 3 or idx.dtype != torch.int32:
        raise L.DransacError("kabsch_gather: correspondences [P,N,6] and int32 index sets [P,B,k]")
    return _pair_sample_fit("kabsch_gather", 4, matches, idx, (idx.shape[2],))


def kabsch_gather_checked(matches: torch.Tensor, idx: torch.Tensor, edge_similarity: float, rejected: Optional[torch.Tensor] = None):
    """dr_kabsch_gather_checked: kabsch_gather behind a rigidity test of every sample.  With sigma = edge_similarity^2 a sample passes
    iff |p_i - p_j|^2 >= sigma |q_i - q_j|^2 and |q_i - q_j|^2 >= sigma |p_i - p_j|^2 for every pair of its rows (f64; Open3D's
    CorrespondenceCheckerBasedOnEdgeLength with similarity_threshold = edge_similarity); it then gets kabsch_gather's model and valid
    bit for bit.  A sample that fails is the identity with valid = 0, no fit is run for it, and it counts once in rejected [P] int32
    (optional; ADDED to, the caller zeroes it).  A sample with an index out of range is kabsch_gather's (identity, valid = 0) and is
    not counted.  edge_similarity lies in [0, 1]; at 0 the outputs are kabsch_gather's."""
    if matches.dim() != 3 or matches.shape[-1] != 6 or idx.dim() != 3 or idx.dtype != torch.int32:
        raise L.DransacError("kabsch_gather_checked: correspondences [P,N,6] and int32 index sets [P,B,k]")
    if not 0.0 <= float(edge_similarity) <= 1.0:      # (false for NaN)
        raise L.DransacError(f"kabsch_gather_checked: edge_similarity must lie in [0, 1], got {edge_similarity!r}")
    _check_counter("kabsch_gather_checked", "rejected", rejected, matches.shape[0])
    return _pair_sample_fit("kabsch_gather_checked", 4, matches, idx, (idx.shape[2], float(edge_similarity)), (rejected,))


# ---- what the families with their per-pair state on the device share (this one and the homographies below): one state class, and one
# helper each for "fit every sample", "score every model", "update the state", "refit over mask / weights" and "polish"; a family names
# its C entry and model side.  What more than one helper needs of a family stands in its record, which the training losses at the end
# of the file read too: the stem of the entries named after it (dr_<entry>_{update,irls,gt_mask,loss_*}), the columns of its matches,
# its model shape, the nouns of the loss messages, the stem of its refit (dr_<refit>, dr_<refit>_bwd), whether the backward of the
# weighted fit is once_differentiable, and the text of the shape check its wrappers open with (None: they run none).
_PairFamily = collections.namedtuple("_PairFamily", "entry width shape points gt_noun refit once shape_text")
_REGISTRATION = _PairFamily("registration", 6, (4, 4), "correspondences", "pose", "refit_rigid", False, None)
_HOMOGRAPHY = _PairFamily("homography", 4, (3, 3), "matches", "homography", "refit_homography", True,
                          "matches [P,N,4] = (x1, y1, x2, y2)")
_PNP = _PairFamily("pnp", 5, (4, 4), "matches", "pose", "refit_pnp", True, "matches [P,N,5] = (X, Y, Z, u, v)")
# the two-view fit is here for _WeightedFit alone (refit, shape, width, once, shape_text): its state, scoring and losses have entries of
# their own (dr_ransac_*, MatchLoss), so the entry stem, the nouns and the loss fields of this record are unused
_FUNDAMENTAL = _PairFamily(None, 4, (3, 3), None, None, "refit_fundamental", True, "matches [P,N,4] = (x1, y1, x2, y2)")


def _check_matches(fam, name: str, matches: torch.Tensor) -> None:
    if fam.shape_text is not None and (matches.dim() != 3 or matches.shape[-1] != fam.width):
        raise L.DransacError(f"{name}: {fam.shape_text}")


class _PairState:
    """best_score [P] (0), best_model [P,side,side] (identity), best_mask [P,N], best_inliers [P] int32, iters [P] int32,
    max_iters [P] f64 (= max_iterations).  Allocated and filled with torch (capturable)."""

    def __init__(self, side: int, P: int, N: int, max_iterations: int, device, dtype):
        self.best_score = torch.zeros(P, device=device, dtype=dtype)
        self.best_model = torch.eye(side, device=device, dtype=dtype).repeat(P, 1, 1)
        self.best_mask = torch.zeros(P, N, device=device, dtype=torch.bool)
        self.best_inliers = torch.zeros(P, device=device, dtype=torch.int32)
        self.iters = torch.zeros(P, device=device, dtype=torch.int32)
        self.max_iters = torch.full((P,), float(max_iterations), device=device, dtype=torch.float64)
        self.max_iterations = int(max_iterations)


def _pair_sample_fit(entry: str, side: int, matches, idx, scalars=(), counters=(), slots: int = 1):
    """dr_<entry>_{f32,f64}: the fit of every sample idx [P,B,k] names -> (models [P,slots B,side,side], valid [P,slots B] bool), `slots`
    model slots per sample; `scalars` follow P, B, N by value, `counters` (tensors or None) the outputs"""
    P, N, _ = matches.shape
    B = idx.shape[1]
    models = torch.empty((P, slots * B, side, side), device=matches.device, dtype=matches.dtype)
    valid = torch.empty((P, slots * B), device=matches.device, dtype=torch.bool)
    L.call(f"dr_{entry}_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), ptr(idx.contiguous()), P, B, N, *scalars, ptr(models),
           ptr(valid), *map(ptr, counters), stream())
    return models, valid


def _pair_score(entry: str, matches, models, threshold, valid, want_inliers, thr2, gated: bool = False, gate=None):
    """dr_<entry>_{f32,f64}: (scores [P,M], inliers [P,M] int32 | None) of models [P,M,.,.]; a `gated` entry takes the gate's pointers"""
    P, N, _ = matches.shape
    M = models.shape[1]
    thr2 = thr2_tensor(threshold, P, matches) if thr2 is None else thr2
    scores = torch.empty((P, M), device=matches.device, dtype=matches.dtype)
    inliers = torch.empty((P, M), device=matches.device, dtype=torch.int32) if want_inliers else None
    L.call(f"dr_{entry}_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), ptr(models.contiguous()), _u8_ptr(valid), ptr(thr2), P,
           M, N, ptr(scores), ptr(inliers), *(_gate_args(gate) if gated else ()), stream())
    return scores, inliers


def _pair_update(entry: str, state: _PairState, matches, models, valid, scores, threshold, B: int, confidence, eps, thr2) -> None:
    """dr_<entry>_{f32,f64}: the state step, in place on `state`"""
    P, N, _ = matches.shape
    M = models.shape[1]
    thr2 = thr2_tensor(threshold, P, matches) if thr2 is None else thr2
    L.call(f"dr_{entry}_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), ptr(models.contiguous()), _u8_ptr(valid),
           ptr(scores.contiguous()), ptr(thr2), P, M, N, int(B), confidence, eps, state.max_iterations, ptr(state.best_score),
           ptr(state.best_model), ptr(state.best_mask.view(torch.uint8)), ptr(state.best_inliers), ptr(state.iters),
           ptr(state.max_iters), stream())


def _pair_refit(entry: str, side: int, matches, mask, weights):
    """dr_<entry>_{f32,f64}: the fit over the rows mask [P,N] selects, under weights [P,N] -> (model [P,side,side], valid [P] bool)"""
    P, N, _ = matches.shape
    if weights is not None and weights.shape != (P, N):
        raise L.DransacError("refit weights are [P,N], one per point")
    if mask is not None and mask.shape != (P, N):
        raise L.DransacError("the refit mask is [P,N], one flag per point")
    model = torch.empty((P, side, side), device=matches.device, dtype=matches.dtype)
    valid = torch.empty((P,), device=matches.device, dtype=torch.bool)
    L.call(f"dr_{entry}_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), _u8_ptr(mask),
           ptr(None if weights is None else weights.to(matches.dtype).contiguous()), P, N, ptr(model), ptr(valid), stream())
    return model, valid


def _pair_irls(fam, state: _PairState, matches, thr2, irls_iters: int, irls_fits: torch.Tensor) -> None:
    """dr_<entry>_irls_{f32,f64}: the family's IRLS polish, in place on state.best_model / state.best_score"""
    _gpu_only((matches, thr2, irls_fits, state.best_score, state.best_model))
    _check_matches(fam, f"{fam.entry}_irls", matches)
    P, N, _ = matches.shape
    _check_counter(f"{fam.entry}_irls", "irls_fits", irls_fits, P)
    L.call(f"dr_{fam.entry}_irls_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), ptr(thr2), P, N, int(irls_iters),
           ptr(state.best_score), ptr(state.best_model), ptr(irls_fits), stream())


def rigid_msac_score(matches: torch.Tensor, models: torch.Tensor, threshold, valid: Optional[torch.Tensor] = None,
                     want_inliers: bool = True, gate=None, thr2: Optional[torch.Tensor] = None):
    """dr_rigid_msac_score: matches [P,N,6], models [P,M,4,4], threshold = inlier DISTANCE (float or [P]) ->
    (scores [P,M] = sum_n max(0, 1 - d2_n / threshold^2), inliers [P,M] int32 = #{d2_n < threshold^2} | None).  Invalid slots score
    -1.  Bit-repeatable (fixed reduction order).  gate = RegistrationState: the blocks of terminated pairs return at once."""
    return _pair_score("rigid_msac_score", matches, models, threshold, valid, want_inliers, thr2, True, gate)


def rigid_magsac_score(matches: torch.Tensor, models: torch.Tensor, threshold, valid: Optional[torch.Tensor] = None,
                       want_inliers: bool = True, gate=None, thr2: Optional[torch.Tensor] = None):
    """dr_rigid_magsac_score: rigid_msac_score's arguments and results with the MAGSAC++ score.  `threshold` is the cutoff DISTANCE,
    read as k sigma_max (k^2 = 11.344866730144373, the 0.99 quantile of chi^2 with 3 degrees of freedom).  With s = d2 / threshold^2,
    u_k = k^2 / 2, c = exp(-u_k): scores [P,M] = sum_n (1 - l(s_n)), l(s) = (1 - exp(-u_k s) - c u_k s) / (1 - c (1 + u_k)) for s < 1,
    else 1; inliers = #{d2_n < threshold^2}.  Invalid slots score -1.  Bit-repeatable; gate as in rigid_msac_score."""
    return _pair_score("rigid_magsac_score", matches, models, threshold, valid, want_inliers, thr2, True, gate)


class RegistrationState(_PairState):
    """Per-pair state of a BatchedRegistration call, on the device: best_score [P], best_model [P,4,4] (identity), best_mask [P,N],
    best_inliers [P] int32, iters [P] int32, max_iters [P] f64 (= max_iterations).  Allocated and filled with torch (capturable)."""

    def __init__(self, P: int, N: int, max_iterations: int, device, dtype):
        super().__init__(4, P, N, max_iterations, device, dtype)


def registration_update(state: RegistrationState, matches, models, valid, scores, threshold, B: int,
                        confidence: float = 0.999, eps: float = 1e-5, thr2: Optional[torch.Tensor] = None) -> None:
    """dr_registration_update, in place on `state`: per pair with iters < max_iters the first arg-max of scores [P,M] over valid,
    non-NaN models replaces the state if score > best_score or iters == 0 (mask and inlier count recomputed with the DISTANCE
    `threshold`, max_iters = min(max_iterations, adaptive_iteration_number(inliers, N, 3))); iters += B."""
    _pair_update("registration_update", state, matches, models, valid, scores, threshold, B, confidence, eps, thr2)


def registration_local_optimize(state: RegistrationState, matches, thr2, lo: int, lo_iters: int, confidence: float = 0.999,
                                eps: float = 1e-5, max_iterations: Optional[int] = None, lo_seen: Optional[torch.Tensor] = None,
                                lo_refits: Optional[torch.Tensor] = None) -> None:
    """dr_registration_local_opt: local optimisation (lo = 1: one Kabsch refit on the inliers, lo = 2: up to lo_iters, each kept only
    where it scores strictly higher), in place on `state`, for the pairs whose best model dr_registration_update replaced since the
    last visit.  thr2 [P] = threshold^2 (thr2_tensor).  lo_seen [P,17] (matches' dtype) is the per-call snapshot, filled with NaN
    before the first round; lo_refits [P] int32 (optional) accumulates the fits run per pair.  One launch, no synchronisation."""
    P, N, mi = _lo_args("registration_local_optimize", 17, state, matches, thr2, lo_seen, lo_refits, max_iterations)
    L.call(f"dr_registration_local_opt_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), ptr(thr2), P, N, int(lo), int(lo_iters),
           confidence, eps, mi, ptr(state.best_score), ptr(state.best_model), ptr(state.best_mask.view(torch.uint8)),
           ptr(state.best_inliers), ptr(state.max_iters), ptr(lo_seen), ptr(lo_refits), stream())


def registration_irls(state: RegistrationState, matches, thr2, irls_iters: int, irls_fits: torch.Tensor) -> None:
    """dr_registration_irls: the IRLS polish under the MAGSAC++ loss, in place on state.best_model / state.best_score: up to irls_iters
    times the weights w(s) = (exp(-u_k s) - c) / (1 - c) under the current model, the weighted Kabsch fit over all points and the
    candidate's MAGSAC++ score, taken only where it is strictly higher.  thr2 [P] = threshold^2 (thr2_tensor); irls_fits [P] int32
    grows by the fits run.  Mask, inlier count and counters of the state are left alone.  One launch, no synchronisation."""
    _pair_irls(_REGISTRATION, state, matches, thr2, irls_iters, irls_fits)


def refit_rigid(matches: torch.Tensor, mask: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None):
    """dr_refit_rigid: the Kabsch fit over the rows mask [P,N] selects (None = all), weights [P,N] (optional) multiplying a row's
    term in the means and in H -> (model [P,4,4], valid [P] bool); valid = 0 below three rows or for a degenerate selection."""
    return _pair_refit("refit_rigid", 4, matches, mask, weights)


def _kabsch_fwd(samples: torch.Tensor, weights: Optional[torch.Tensor]):
    """dr_kabsch on flattened samples [Bt,k,6] (contiguous), weights [Bt,k] | None -> (models [Bt,4,4], valid [Bt] bool)"""
    Bt, k, _ = samples.shape
    models = torch.empty((Bt, 4, 4), device=samples.device, dtype=samples.dtype)
    valid = torch.empty((Bt,), device=samples.device, dtype=torch.bool)
    L.call(f"dr_kabsch_{L.suffix(samples.dtype)}", ptr(samples), ptr(weights), Bt, k, ptr(models), ptr(valid), stream())
    return models, valid


def select_closest(models: torch.Tensor, valid: Optional[torch.Tensor], gt: torch.Tensor, want_keep: bool = False):
    """K5: models [P,B,S,3,3], valid [P,B,S] | None, gt [P,3,3] -> chosen [P,B,3,3], which [P,B] int32 (+ keep [P,B] bool =
    `which >= 0` from the same launch when want_keep)."""
    P, B, S = models.shape[:3]
    chosen = torch.empty((P, B, 3, 3), device=models.device, dtype=models.dtype)
    which = torch.empty((P, B), device=models.device, dtype=torch.int32)
    keep = torch.empty((P, B), device=models.device, dtype=torch.bool) if want_keep else None
    L.call(f"dr_select_closest_{L.suffix(models.dtype)}", ptr(models.contiguous()), _u8_ptr(valid),
           ptr(gt.to(models.dtype).contiguous()), P, B, S, ptr(chosen), ptr(which), ptr(keep), stream())
    return (chosen, which, keep) if want_keep else (chosen, which)


def refit_essential(matches: torch.Tensor, mask: Optional[torch.Tensor] = None):
    """K7 (E): five-point solver on all (masked) points of every pair as one sample, f64 inside.
    matches [P,N,4] -> models [P,10,3,3], valid [P,10]."""
    P, N, _ = matches.shape
    models = torch.empty((P, 10, 3, 3), device=matches.device, dtype=matches.dtype)
    valid = torch.empty((P, 10), device=matches.device, dtype=torch.bool)
    L.call(f"dr_refit_essential_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), _u8_ptr(mask), P, N, ptr(models), ptr(valid),
           stream())
    return models, valid


def refit_accept(matches: torch.Tensor, cand: torch.Tensor, cand_valid: Optional[torch.Tensor], thr: torch.Tensor,
                 best_score: torch.Tensor, best_model: torch.Tensor) -> None:
    """K7 acceptance in one launch (dr_refit_accept): scores cand [P,S,3,3] and replaces best_score [P] / best_model
    [P,3,3] IN PLACE where a candidate scores strictly higher (ransac.py:173-185)."""
    P, N, _ = matches.shape
    S = cand.shape[1]
    L.call(f"dr_refit_accept_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), ptr(cand.contiguous()), _u8_ptr(cand_valid),
           ptr(thr), P, S, N, ptr(best_score), ptr(best_model), stream())


def refit_fundamental(matches: torch.Tensor, mask: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None):
    """K7 (F): Hartley-normalised LSQ 8-point on the masked points of every pair.  -> F [P,3,3], valid [P].
    weights [P,N] (optional): per-point row weights, the `soft_weights[0, inlier_indices[0]]` of ransac.py:151-153."""
    P, N, _ = matches.shape
    models = torch.empty((P, 3, 3), device=matches.device, dtype=matches.dtype)
    valid = torch.empty((P,), device=matches.device, dtype=torch.bool)
    if weights is not None and weights.shape != (P, N):
        raise L.DransacError("refit weights are [P,N], one per point")
    L.call(f"dr_refit_fundamental_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), _u8_ptr(mask),
           ptr(None if weights is None else weights.to(matches.dtype).contiguous()), P, N, ptr(models), ptr(valid), stream())
    return models, valid


def soft_weights_row0(logits: torch.Tensor, k: int, tau: float, gumbel: Optional[torch.Tensor], seed: int) -> torch.Tensor:
    """y_soft of hypothesis 0 of a sampler call, [P,N]: softmax((logits + noise[:, 0]) / tau) with the SAME noise row the call
    with this seed (or this explicit noise) drew -- the in-kernel Philox counters are (element, hypothesis, pair), so row 0 does
    not depend on the batch size.  What ransac.py:151-153 indexes as `soft_weights[0, ...]`."""
    g = None if gumbel is None else gumbel[:, :1].contiguous()
    return gumbel_topk(logits, 1, k, tau, g, seed, dense=True)["y_soft"][:, 0]


# ------------------------------------------------------------------------------------------ autograd wrappers
# the five-point backward entry for (minimal sample, f64 in memory, sparse gradient through `which`)
_FIVEPOINT_BWD = {(True, False, False): "dr_solve_nister5_bwd_f32", (True, False, True): "dr_solve_nister5_bwd_sel_f32",
                  (True, True, False): "dr_solve_nister5_bwd_f64",
                  (False, False, False): "dr_solve_nister5_nm_bwd_f32", (False, True, False): "dr_solve_nister5_nm_bwd_f64"}


def _fivepoint_bwd(samples, models, m64, valid, grad, which=None, weights=None, want_gw=False):
    """The host path of every five-point backward: samples [...,n,4] and the gradient of their models ([...,10,3,3]; with `which`,
    [...,3,3]: that of the one model K5 picked per sample) -> (grad_samples, grad_weights); grad_weights is None unless the rows
    have weights (n > 5) and the caller wants their gradient.  f64 samples go f64 straight through, gradient included; f32 ones
    use the solver's f64 models where the forward kept them (m64 not empty): the tangent-space system is conditioned ~1e5."""
    s, Bt, n = _flat_samples(samples, 4)
    minimal, f64 = n == 5, s.dtype == torch.float64
    gs = torch.empty_like(s)
    w = None if minimal or weights is None else weights.reshape(Bt, n).to(s.dtype).contiguous()
    gw = torch.empty((Bt, n), device=s.device, dtype=s.dtype) if w is not None and want_gw else None
    args = [ptr(s)] + ([] if minimal else [ptr(w)]) + [ptr(models.contiguous())]
    if not f64:
        args.append(ptr(m64.contiguous() if m64.numel() else None))
    args += [_u8_ptr(valid), ptr((grad.to(torch.float64) if f64 else grad).contiguous())]
    if which is not None:
        args.append(ptr(which.contiguous()))
    args += [Bt] + ([] if minimal else [n]) + [ptr(gs)] + ([] if minimal else [ptr(gw)])
    L.call(_FIVEPOINT_BWD[minimal, f64, which is not None], *args, stream())
    return gs.reshape(samples.shape), (None if gw is None else gw.reshape(weights.shape).to(weights.dtype))


class _SolveEssential(torch.autograd.Function):
    """Five-point solve with implicit-function backward (dr_solve_nister5_bwd): at a returned model E the five
    epipolar constraints x2^T E x1 = 0 restricted to the tangent space of the essential manifold determine dE/dpts."""

    @staticmethod
    def forward(ctx, samples, weights, which):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        fn = (lambda s_, w_: solve_nister5(s_, w_)) if which == "nister" else (lambda s_, w_: solve_stewenius5(s_))
        need_grad = samples.requires_grad and samples.dtype == torch.float32
        if need_grad and which == "nister" and samples.shape[-2] == 5:
            # train mode: the kernel computes in f64 anyway; it writes the f64 models next to the f32 ones and the backward
            # keeps them -- its tangent-space system is conditioned ~1e5, which f32-rounded models cannot afford
            models, m64, valid = solve_nister5_hp(samples, weights)
        elif need_grad:
            m64, valid = fn(samples.double(), None if weights is None else weights.double())
            models = m64.float()
        else:
            models, valid = fn(samples, weights)
            m64 = torch.empty(0, device=samples.device, dtype=torch.float64)
        ctx.save_for_backward(samples, models, m64, valid)
        ctx.minimal = samples.shape[-2] == 5
        ctx.weights = None if ctx.minimal or weights is None else weights.detach()
        ctx.mark_non_differentiable(valid)
        return models, valid

    @staticmethod
    def backward(ctx, g_models, _g_valid):
        if g_models is None:
            return None, None, None
        samples, models, m64, valid = ctx.saved_tensors
        gs, gw = _fivepoint_bwd(samples, models, m64, valid, g_models, weights=ctx.weights, want_gw=ctx.needs_input_grad[1])
        return gs, gw, None


def solve_essential(samples, weights=None, which="nister"):
    """Differentiable five-point solve: samples [...,n,4] -> (models [...,10,3,3], valid [...,10]).
    Minimal samples (n = 5): implicit derivative of the five epipolar constraints.  Non-minimal samples (n > 5, Nister only:
    the reference's `-sam 3`, eight-point Gumbel sampler feeding the five-point estimator, ransac.py:82-83): implicit
    derivative of the invariant subspace the models live in (dr_solve_nister5_nm_bwd), gradients for the row weights too."""
    return _SolveEssential.apply(samples, weights, which)


class _SolveSelectEssential(torch.autograd.Function):
    """K3 (minimal five-point, train mode) + K5 (closest of the ten models to the ground truth) as ONE autograd node:
    samples [P,B,5,4] f32, gt [P,3,3] -> chosen [P,B,3,3], which [P,B], keep [P,B], models [P,B,10,3,3], valid [P,B,10].
    The backward hands the gradient of `chosen` to the solver's implicit-function backward in the sparse form
    (dr_solve_nister5_bwd_sel): no dense [P,B,10,9] gradient is written and scanned."""

    @staticmethod
    def forward(ctx, samples, weights, gt):
        ctx.set_materialize_grads(False)
        models, m64, valid = solve_nister5_hp(samples, weights)
        chosen, which, keep = select_closest(models, valid, gt, want_keep=True)
        ctx.save_for_backward(samples, models, m64, valid, which)
        ctx.mark_non_differentiable(which, keep, valid)
        return chosen, which, keep, models.detach(), valid

    @staticmethod
    def backward(ctx, g_chosen, _gw, _gk, g_models, _gv):
        if g_models is not None:
            raise L.DransacError("solve_select_essential: gradients flow through `chosen` only (use solve_essential + "
                                 "select_closest_autograd to differentiate the full model set)")
        if g_chosen is None:
            return None, None, None
        samples, models, m64, valid, which = ctx.saved_tensors
        return _fivepoint_bwd(samples, models, m64, valid, g_chosen, which=which)[0], None, None


def solve_select_essential(samples, gt, weights=None):
    """Train-mode K3 + K5 in one autograd node (Nister, minimal f32 samples): -> (chosen, which, keep, models, valid);
    `models` is returned detached (inspection / logging), the gradient path is samples -> chosen."""
    if samples.shape[-2] != 5 or samples.dtype != torch.float32:
        raise L.DransacError("solve_select_essential takes minimal f32 samples [...,5,4]")
    return _SolveSelectEssential.apply(samples, weights, gt)


class _SolveF8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, samples, weights):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        F, valid = solve_f8(samples, weights)
        ctx.save_for_backward(samples, weights if weights is not None else torch.empty(0, device=samples.device), F)
        ctx.has_w = weights is not None
        ctx.mark_non_differentiable(valid)
        return F, valid

    @staticmethod
    def backward(ctx, gF, _gv):
        if gF is None:
            return None, None
        samples, weights, F = ctx.saved_tensors
        dt = samples.dtype      # f32, or f64 (`-pr 2 -tr 1`): the same kernel with f64 in memory (round 5: nothing rounded to f32)
        s, Bt, n = _flat_samples(samples, 4)
        gs = torch.empty_like(s)
        w = weights.reshape(Bt, n).to(dt).contiguous() if ctx.has_w else None
        gw = torch.empty_like(w) if ctx.has_w else None
        L.call(f"dr_solve_f8_bwd_{L.suffix(dt)}", ptr(s), ptr(w), ptr(F.to(dt).contiguous()), ptr(gF.to(dt).contiguous()), Bt, n,
               ptr(gs), ptr(gw), stream())
        return gs.reshape(samples.shape), (gw.reshape(weights.shape) if ctx.has_w else None)


def solve_fundamental8(samples, weights=None):
    return _SolveF8.apply(samples, weights)


class _SolveRigid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, samples, weights, flag):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        out = solve_rigid(samples, weights, flag)
        ctx.save_for_backward(samples, out[0])
        ctx.flag = flag
        ctx.has_w = weights is not None
        ctx.mark_non_differentiable(out[4])
        return out

    @staticmethod
    def backward(ctx, g_model, g_R, g_t, g_scale, _gv):
        if g_model is None and g_R is None and g_t is None:
            return None, None, None
        samples, model = ctx.saved_tensors
        if samples.dtype != torch.float32:
            raise L.DransacError("backward is implemented for f32 only")
        if ctx.has_w:
            raise L.DransacError("backward of the weighted rigid solver is not implemented")
        g = g_model.clone() if g_model is not None else torch.zeros_like(model)
        if g_R is not None:
            g[..., :3, :3] += g_R
        if g_t is not None:
            g[..., :3, 3] += g_t
        s, Bt, n = _flat_samples(samples, 6)
        gs = torch.empty_like(s)
        L.call("dr_solve_rigid_bwd_f32", ptr(s), ptr(model.contiguous()), ptr(g.contiguous()), Bt, n, bool(ctx.flag), ptr(gs),
               stream())
        return gs.reshape(samples.shape), None, None


def solve_rigid_autograd(samples, weights=None, flag=True):
    return _SolveRigid.apply(samples, weights, flag)


class _Kabsch(torch.autograd.Function):
    """dr_kabsch / dr_kabsch_bwd: the backward recomputes the fit from the samples, so no model is saved"""

    @staticmethod
    def forward(ctx, samples, weights):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        s, Bt, k = _flat_samples(samples, 6)
        w = None if weights is None else weights.reshape(Bt, k).to(s.dtype).contiguous()
        models, valid = _kabsch_fwd(s, w)
        ctx.save_for_backward(s, *(() if w is None else (w,)))
        ctx.shapes = (samples.shape, None if weights is None else (weights.shape, weights.dtype))
        lead = samples.shape[:-2]
        valid = valid.reshape(lead)
        ctx.mark_non_differentiable(valid)
        return models.reshape(*lead, 4, 4), valid

    @staticmethod
    def backward(ctx, g_models, _gv):
        if g_models is None:
            return None, None
        s, *w = ctx.saved_tensors
        w = w[0] if w else None
        Bt, k, _ = s.shape
        gs = torch.empty_like(s)
        gw = torch.empty((Bt, k), device=s.device, dtype=s.dtype) if (w is not None and ctx.needs_input_grad[1]) else None
        L.call(f"dr_kabsch_bwd_{L.suffix(s.dtype)}", ptr(s), ptr(w), ptr(g_models.to(s.dtype).reshape(-1, 4, 4).contiguous()), Bt, k,
               ptr(gs), ptr(gw), stream())
        sshape, wshape = ctx.shapes
        return gs.reshape(sshape), None if gw is None else gw.reshape(wshape[0]).to(wshape[1])


def kabsch(samples, weights=None):
    """samples [..., k, 6] = (p, q) rows, 3 <= k <= 8, weights [..., k] | None -> (models [..., 4, 4], valid [...] bool): the weighted
    least-squares rigid fit (Kabsch) of every sample, with autograd to `samples` and `weights` in f32 and f64 (dr_kabsch,
    dr_kabsch_bwd).  Without weights, on samples = matches[idx], the models of kabsch_gather bit for bit.  A sample without a valid fit
    (valid = 0: the identity), or with a non-finite derivative, passes exact zeros back."""
    if samples.dim() < 3 or samples.shape[-1] != 6 or not 3 <= samples.shape[-2] <= 8:
        raise L.DransacError("kabsch: samples [..., k, 6] with 3 <= k <= 8 rows per sample")
    if weights is not None and weights.shape != samples.shape[:-1]:
        raise L.DransacError("kabsch: weights are [..., k], one per sample row")
    return _Kabsch.apply(samples, weights)


def _weighted_fit_bwd(ctx, g_model, _gv):
    _, want_m, want_w, _ = ctx.needs_input_grad      # (weights = None never wants a gradient)
    if g_model is None or not (want_m or want_w):
        return None, None, None, None
    m, *w = ctx.saved_tensors
    w = w[0] if w else None
    P, N, _ = m.shape
    gm = torch.empty_like(m) if want_m else None
    gw = torch.empty((P, N), device=m.device, dtype=m.dtype) if want_w else None
    L.call(f"dr_{ctx.fam.refit}_bwd_{L.suffix(m.dtype)}", ptr(_al(m)), ptr(ctx.mask), ptr(w),
           ptr(g_model.to(m.dtype).reshape(P, *ctx.fam.shape).contiguous()), P, N, ptr(gm), ptr(gw), stream())
    return None, gm, None if gw is None else gw.to(ctx.wdtype), None


class _WeightedFit(torch.autograd.Function):
    """dr_<refit> / dr_<refit>_bwd of a pair family (`fam` travels in ctx, as in _PairLossFused): the backward recomputes the fit from
    its inputs, so no model is saved.  Only a family with `once` set refuses a second derivative (once_differentiable); the rigid fit
    keeps letting one through unrecorded, as it always has."""

    @staticmethod
    def forward(ctx, fam, matches, weights, mask):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        m = matches.contiguous()
        w = None if weights is None else weights.to(m.dtype).contiguous()
        model, valid = _pair_refit(fam.refit, fam.shape[0], m, mask, w)
        ctx.save_for_backward(m, *(() if w is None else (w,)))
        ctx.fam = fam
        ctx.mask = None if mask is None else _u8(mask)
        ctx.wdtype = None if weights is None else weights.dtype
        ctx.mark_non_differentiable(valid)
        return model, valid

    @staticmethod
    def backward(ctx, g_model, _gv):
        bwd = torch.autograd.function.once_differentiable(_weighted_fit_bwd) if ctx.fam.once else _weighted_fit_bwd
        return bwd(ctx, g_model, _gv)


def weighted_kabsch(matches, weights=None, mask=None):
    """matches [P,N,6], weights [P,N] | None, mask [P,N] | None -> (model [P,4,4], valid [P] bool): refit_rigid (the weighted Procrustes
    fit over the rows the mask selects) with autograd to `weights` and / or `matches`, whichever require it (dr_refit_rigid_bwd).
    Rows the mask drops, and every row of a pair without a valid fit, get exact zeros; bit-repeatable."""
    if matches.dim() != 3 or matches.shape[-1] != 6:
        raise L.DransacError("weighted_kabsch: correspondences [P,N,6]")
    return _WeightedFit.apply(_REGISTRATION, matches, weights, mask)


# ------------------------------------------------------------------------------------------ plane-induced homographies
# matches [P,N,4] = (x1, y1, x2, y2) in the caller's coordinates (pixels), models [.,3,3] = H with x2 ~ H x1, unit Frobenius norm and
# det > 0.  d2 = the symmetric transfer error; `threshold` is a DISTANCE: inlier iff d2 < threshold^2 (thr2_tensor).
def homography4_gather(matches: torch.Tensor, idx: torch.Tensor):
    """dr_homography4_gather: matches [P,N,4], idx [P,B,4] int32 -> (models [P,B,3,3], valid [P,B] bool): the closed-form homography of
    every four-point sample; a sample with three collinear points, with an orientation that differs between the images, or without a
    finite non-singular model is the identity with valid = 0."""
    _check_matches(_HOMOGRAPHY, "homography4_gather", matches)
    if idx.dim() != 3 or idx.shape[-1] != 4 or idx.dtype != torch.int32 or idx.shape[0] != matches.shape[0]:
        raise L.DransacError("homography4_gather: int32 index sets [P,B,4]")
    return _pair_sample_fit("homography4_gather", 3, matches, idx)


def homography_score(matches: torch.Tensor, models: torch.Tensor, threshold, valid: Optional[torch.Tensor] = None,
                     want_inliers: bool = True, thr2: Optional[torch.Tensor] = None):
    """dr_homography_score: matches [P,N,4], models [P,M,3,3], threshold = inlier DISTANCE (float or [P]) ->
    (scores [P,M] = sum_n max(0, 1 - d2_n / threshold^2), inliers [P,M] int32 = #{d2_n < threshold^2} | None).  A slot with valid = 0
    scores exactly 0; a non-finite model or one with det == 0 scores NaN; a model of negative determinant scores like its negation.
    Bit-repeatable (fixed reduction order)."""
    _check_matches(_HOMOGRAPHY, "homography_score", matches)
    if models.shape != (matches.shape[0], models.shape[1], 3, 3) or models.dtype != matches.dtype:
        raise L.DransacError("homography_score: models [P,M,3,3] of the matches' dtype")
    return _pair_score("homography_score", matches, models, threshold, valid, want_inliers, thr2)


def homography_magsac_score(matches: torch.Tensor, models: torch.Tensor, threshold, valid: Optional[torch.Tensor] = None,
                            want_inliers: bool = True, thr2: Optional[torch.Tensor] = None):
    """dr_homography_magsac_score: homography_score's arguments, slot rules and inlier counts with the MAGSAC++ score.  `threshold` is
    the cutoff DISTANCE, read as k sigma_max (k^2 = 13.276704135987622, the 0.99 quantile of chi^2 with 4 degrees of freedom: the
    symmetric transfer error is a 4-vector).  With s = d2 / threshold^2: scores [P,M] = sum_n (1 - l(s_n)), l the two-view MAGSAC++ loss
    (magsac_score states it; 1 for s >= 1); inliers = #{d2_n < threshold^2}.  Bit-repeatable."""
    _check_matches(_HOMOGRAPHY, "homography_magsac_score", matches)
    if models.shape != (matches.shape[0], models.shape[1], 3, 3) or models.dtype != matches.dtype:
        raise L.DransacError("homography_magsac_score: models [P,M,3,3] of the matches' dtype")
    return _pair_score("homography_magsac_score", matches, models, threshold, valid, want_inliers, thr2)


class HomographyState(_PairState):
    """Per-pair state of a BatchedHomography call, on the device: best_score [P] (0), best_model [P,3,3] (identity), best_mask [P,N],
    best_inliers [P] int32, iters [P] int32, max_iters [P] f64 (= max_iterations).  Allocated and filled with torch."""

    def __init__(self, P: int, N: int, max_iterations: int, device, dtype):
        super().__init__(3, P, N, max_iterations, device, dtype)


def homography_update(state: HomographyState, matches, models, valid, scores, threshold, B: int, confidence: float = 0.999,
                      eps: float = 1e-5, thr2: Optional[torch.Tensor] = None) -> None:
    """dr_homography_update, in place on `state`: per pair with iters < max_iters the first arg-max of scores [P,M] over valid, non-NaN
    slots replaces the state if score > best_score (mask and inlier count recomputed with the score kernel's expression,
    max_iters = min(max_iterations, adaptive_iteration_number(inliers, N, 4))); iters += B."""
    _check_matches(_HOMOGRAPHY, "homography_update", matches)
    _pair_update("homography_update", state, matches, models, valid, scores, threshold, B, confidence, eps, thr2)


def refit_homography(matches: torch.Tensor, mask: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None):
    """dr_refit_homography: the normalised DLT over the rows mask [P,N] selects (None = all), weights [P,N] (optional) multiplying a
    row's terms in the Gram matrix -> (model [P,3,3], valid [P] bool); valid = 0 (identity) below four rows or for a non-finite or
    singular result."""
    _check_matches(_HOMOGRAPHY, "refit_homography", matches)
    return _pair_refit("refit_homography", 3, matches, mask, weights)


def homography_irls(state: HomographyState, matches, thr2, irls_iters: int, irls_fits: torch.Tensor) -> None:
    """dr_homography_irls: the IRLS polish under the MAGSAC++ loss, in place on state.best_model / state.best_score: up to irls_iters
    times the rows inside the cutoff and in front of both cameras under the current model, each with the two-view MAGSAC++ weight
    w(d2 / thr2) (f64), refit_homography's weighted DLT over them and the candidate's homography_magsac_score score over all points,
    taken only where it is strictly higher.  thr2 [P] = threshold^2 (thr2_tensor); irls_fits [P] int32 grows by the fits run.  Mask,
    inlier count and counters of the state are left alone.  One launch, no synchronisation."""
    _pair_irls(_HOMOGRAPHY, state, matches, thr2, irls_iters, irls_fits)


# ------------------------------------------------------------------------------------------ absolute pose from 2D-3D matches
# matches [P,N,5] = (X, Y, Z, u, v): a world point and its observation in NORMALISED image coordinates (K^-1 applied by the caller),
# models [.,4,4] = [[R, t], [0, 0, 0, 1]] with x_c = R X + t (the registration layout: loss.registration_errors reads it).
# d2 = (x_c / z_c - u)^2 + (y_c / z_c - v)^2; a point with z_c <= 0 never counts; `threshold` is a DISTANCE in normalised units.
def _check_pnp_models(name: str, matches: torch.Tensor, models: torch.Tensor) -> None:
    if models.dim() != 4 or models.shape != (matches.shape[0], models.shape[1], 4, 4) or models.dtype != matches.dtype:
        raise L.DransacError(f"{name}: models [P,M,4,4] of the matches' dtype")


def p3p_gather(matches: torch.Tensor, idx: torch.Tensor):
    """dr_p3p_gather: matches [P,N,5], idx [P,B,3] int32 -> (models [P,4B,4,4], valid [P,4B] bool): the closed-form P3P poses of every
    three-point sample.  Slots 4 b + j belong to sample b: the valid ones first, in ascending order of the quartic's root, each with R
    orthonormal, det R = +1 and the three sample points in front of the camera; every other slot is the identity with valid = 0.  A
    sample with coincident or collinear world points, coincident bearings or no finite solution has four invalid slots."""
    _gpu_only((matches, idx))
    _check_matches(_PNP, "p3p_gather", matches)
    if idx.dim() != 3 or idx.shape[-1] != 3 or idx.dtype != torch.int32 or idx.shape[0] != matches.shape[0]:
        raise L.DransacError("p3p_gather: int32 index sets [P,B,3]")
    return _pair_sample_fit("p3p_gather", 4, matches, idx, slots=4)


def pnp_score(matches: torch.Tensor, models: torch.Tensor, threshold, valid: Optional[torch.Tensor] = None,
              want_inliers: bool = True, gate=None, thr2: Optional[torch.Tensor] = None):
    """dr_pnp_score: matches [P,N,5], models [P,M,4,4], threshold = inlier DISTANCE in normalised units (float or [P]) ->
    (scores [P,M] = sum_n max(0, 1 - d2_n / threshold^2), inliers [P,M] int32 = #{d2_n < threshold^2} | None) over the points in front
    of the camera.  A slot with valid = 0 scores exactly 0; a non-finite model scores NaN.  Bit-repeatable (fixed reduction order).
    gate = PnPState: the blocks of terminated pairs return at once and their rows keep their contents."""
    _gpu_only((matches, models))
    _gpu_only((valid, thr2), optional=True)
    _check_matches(_PNP, "pnp_score", matches)
    _check_pnp_models("pnp_score", matches, models)
    if valid is not None and valid.shape != models.shape[:2]:
        raise L.DransacError("pnp_score: valid [P,M], one flag per model slot")
    return _pair_score("pnp_score", matches, models, threshold, valid, want_inliers, thr2, True, gate)


class PnPState(_PairState):
    """Per-pair state of a BatchedPnP call, on the device: best_score [P] (0), best_model [P,4,4] (identity), best_mask [P,N],
    best_inliers [P] int32, iters [P] int32, max_iters [P] f64 (= max_iterations).  Allocated and filled with torch (capturable)."""

    def __init__(self, P: int, N: int, max_iterations: int, device, dtype):
        super().__init__(4, P, N, max_iterations, device, dtype)


def pnp_update(state: PnPState, matches, models, valid, scores, threshold, B: int, confidence: float = 0.999, eps: float = 1e-5,
               thr2: Optional[torch.Tensor] = None) -> None:
    """dr_pnp_update, in place on `state`: per pair with iters < max_iters the first arg-max of scores [P,M] over valid, non-NaN slots
    replaces the state if score > best_score (mask and inlier count recomputed with the score kernel's expression,
    max_iters = min(max_iterations, adaptive_iteration_number(inliers, N, 3))); iters += B -- the SAMPLES of the round, M = 4 B slots."""
    _gpu_only((matches, models, scores, state.best_score))
    _gpu_only((valid, thr2), optional=True)
    _check_matches(_PNP, "pnp_update", matches)
    _check_pnp_models("pnp_update", matches, models)
    if scores.shape != models.shape[:2] or scores.dtype != matches.dtype:
        raise L.DransacError("pnp_update: scores [P,M] of the matches' dtype")
    if state.best_model.shape != (matches.shape[0], 4, 4) or state.best_mask.shape != matches.shape[:2]:
        raise L.DransacError("pnp_update: the state is a PnPState of this call's P and N")
    _pair_update("pnp_update", state, matches, models, valid, scores, threshold, B, confidence, eps, thr2)


def refit_pnp(matches: torch.Tensor, mask: Optional[torch.Tensor], init_model: torch.Tensor, iters: int = 10):
    """dr_refit_pnp: Levenberg-Marquardt on the reprojection error from init_model [P,4,4], over the rows mask [P,N] selects (None = all)
    that lie in front of the camera under the current iterate -> (model [P,4,4], valid [P] bool).  `iters` passes at most; a step (a
    left-multiplied rotation vector and a translation) is taken only on a strictly lower cost over the same rows, otherwise the damping
    grows.  valid = 0 (identity) for a non-finite start or result and below three rows."""
    _gpu_only((matches, init_model))
    _gpu_only((mask,), optional=True)
    _check_matches(_PNP, "refit_pnp", matches)
    P, N, _ = matches.shape
    if init_model.shape != (P, 4, 4) or init_model.dtype != matches.dtype:
        raise L.DransacError("refit_pnp: init_model [P,4,4] of the matches' dtype")
    if mask is not None and mask.shape != (P, N):
        raise L.DransacError("the refit mask is [P,N], one flag per point")
    if int(iters) < 0:
        raise L.DransacError(f"refit_pnp: iters must be at least 0, got {iters!r}")
    model = torch.empty((P, 4, 4), device=matches.device, dtype=matches.dtype)
    valid = torch.empty((P,), device=matches.device, dtype=torch.bool)
    L.call(f"dr_refit_pnp_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), _u8_ptr(mask), ptr(init_model.contiguous()), P, N,
           int(iters), ptr(model), ptr(valid), stream())
    return model, valid


def _check_weighted(name: str, fam, matches, weights, mask, init_model=None) -> None:
    """what the weighted fits refuse before the launch, in this order: matches [P,N,fam.width] f32 / f64, weights a floating
    [P,N] | None, mask a bool / uint8 [P,N] | None, a start model [P,*fam.shape] | None of the matches' dtype (the iterative fit's
    alone), and any of them on the CPU"""
    if not isinstance(matches, torch.Tensor) or matches.dim() != 3 or matches.shape[-1] != fam.width:
        raise L.DransacError(f"{name}: {fam.shape_text}")
    if matches.dtype not in (torch.float32, torch.float64):
        raise L.DransacError(f"{name}: matches must be float32 or float64")
    P, N, _ = matches.shape
    if weights is not None and (not isinstance(weights, torch.Tensor) or weights.shape != (P, N) or not weights.is_floating_point()):
        raise L.DransacError(f"{name}: weights must be floating point [P,N], one per row of matches")
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.shape != (P, N) or mask.dtype not in (torch.bool, torch.uint8)):
        raise L.DransacError(f"{name}: mask must be bool or uint8 [P,N]")
    if init_model is not None and (not isinstance(init_model, torch.Tensor) or init_model.shape != (P, *fam.shape)
                                   or init_model.dtype != matches.dtype):
        raise L.DransacError(f"{name}: init_model [P,{fam.shape[0]},{fam.shape[1]}] of the matches' dtype")
    _gpu_only((matches, weights, mask, init_model), optional=True)


def _pnp_dlt(m, w, mask):
    P, N, _ = m.shape
    model = torch.empty((P, 4, 4), device=m.device, dtype=m.dtype)
    valid = torch.empty((P,), device=m.device, dtype=torch.bool)
    L.call(f"dr_pnp_dlt_{L.suffix(m.dtype)}", ptr(_al(m)), _u8_ptr(mask), ptr(w), P, N, ptr(model), ptr(valid), stream())
    return model, valid


def pnp_dlt(matches, weights=None, mask=None):
    """dr_pnp_dlt: matches [P,N,5], weights [P,N] | None, mask [P,N] | None -> (model [P,4,4], valid [P] bool): a pose from six or more
    rows without a start model, by the weighted normalised DLT (Hartley-normalised world points, the smallest eigenvector of the 12x12
    Gram matrix, the rotation nearest to its 3x3 part, the sign that puts the weighted majority of the rows in front of the camera).
    Forward only, f32 and f64; weights are expected >= 0 and are not checked.  valid = 0 (identity) below six rows under the mask, for a
    non-finite sum or result, and when the smallest eigenvalue is not simple (within 1e-10 of the largest): a coplanar world set has no
    DLT pose -- pass such a pair's start to weighted_pnp yourself.  Bit-repeatable."""
    _check_weighted("pnp_dlt", _PNP, matches, weights, mask)
    m = matches.detach().contiguous()
    return _pnp_dlt(m, None if weights is None else weights.detach().to(m.dtype).contiguous(), mask)


class _WeightedPnP(torch.autograd.Function):
    """dr_refit_pnp_weighted / dr_refit_pnp_bwd.  Unlike _WeightedFit's closed forms the fit is iterative, so the backward does not
    recompute it: the forward's model is saved and the reverse pass differentiates the stationary point it stands (nearly) on."""

    @staticmethod
    def forward(ctx, matches, weights, init_model, mask, iters):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        m = matches.contiguous()
        w = None if weights is None else weights.to(m.dtype).contiguous()
        P, N, _ = m.shape
        model = torch.empty((P, 4, 4), device=m.device, dtype=m.dtype)
        valid = torch.empty((P,), device=m.device, dtype=torch.bool)
        L.call(f"dr_refit_pnp_weighted_{L.suffix(m.dtype)}", ptr(_al(m)), _u8_ptr(mask), ptr(w), ptr(init_model.contiguous()), P, N,
               int(iters), ptr(model), ptr(valid), stream())
        # the entry of the backward has no `valid`: a pair without a fit travels as a NaN model, which it answers with exact zeros
        saved = torch.where(valid[:, None, None], model, torch.full_like(model, float("nan")))
        ctx.save_for_backward(m, saved, *(() if w is None else (w,)))
        ctx.mask = None if mask is None else _u8(mask)
        ctx.wdtype = None if weights is None else weights.dtype
        ctx.mark_non_differentiable(valid)
        return model, valid

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_model, _gv):
        want_m, want_w = ctx.needs_input_grad[:2]      # (weights = None never wants a gradient)
        if g_model is None or not (want_m or want_w):
            return None, None, None, None, None
        m, model, *w = ctx.saved_tensors
        w = w[0] if w else None
        P, N, _ = m.shape
        gm = torch.empty_like(m) if want_m else None
        gw = torch.empty((P, N), device=m.device, dtype=m.dtype) if want_w else None
        L.call(f"dr_refit_pnp_bwd_{L.suffix(m.dtype)}", ptr(_al(m)), ptr(ctx.mask), ptr(w), ptr(model),
               ptr(g_model.to(m.dtype).reshape(P, 4, 4).contiguous()), P, N, ptr(gm), ptr(gw), stream())
        return gm, None if gw is None else gw.to(ctx.wdtype), None, None, None


def weighted_pnp(matches, weights=None, init_model=None, mask=None, iters: int = 20):
    """matches [P,N,5], weights [P,N] | None, init_model [P,4,4] | None, mask [P,N] | None -> (model [P,4,4], valid [P] bool): the pose
    that minimises sum_i w_i |r_i|^2 of the reprojection residual over the rows the mask selects that lie in front of the camera --
    refit_pnp's Levenberg-Marquardt loop (the same kernel; without weights the same bits) from `init_model`, `iters` passes at most,
    or from pnp_dlt(matches, weights, mask) when no start is given -- with autograd to `weights` and / or `matches`, whichever require
    it (dr_refit_pnp_bwd), in f32 and f64.  Once differentiable; `valid`, the mask (a selection) and `init_model` carry no gradient: the
    minimiser does not depend on where the loop started.  Weights are expected >= 0 and are not checked; a row of weight 0 still
    counts as a row.  The backward is the implicit function theorem at the stationary point with the full 6x6 Hessian (not J^T J),
    after two Newton steps onto the root in f64; it assumes the forward converged -- give it the passes it needs.
    Zero rules: rows the mask drops get exact zeros and are never read (a NaN there reaches nothing), and so do rows behind the camera
    under the returned model; every row of a pair gets exact zeros when the pair has fewer than three rows in front of the camera,
    valid = 0, its Hessian is not positive definite (not a strict minimum), or any result of the pair is not finite.  A pair whose
    DLT start fails (a coplanar world set, fewer than six rows) returns valid = 0 with the identity: pass a start.  Bit-repeatable."""
    _check_weighted("weighted_pnp", _PNP, matches, weights, mask, init_model)
    if int(iters) < 0:
        raise L.DransacError(f"weighted_pnp: iters must be at least 0, got {iters!r}")
    if init_model is None:
        m = matches.detach().contiguous()
        start, usable = _pnp_dlt(m, None if weights is None else weights.detach().to(m.dtype).contiguous(), mask)
        # a failed start is the identity, under which the loop might still find rows: such a pair stays invalid (NaN start -> valid = 0)
        start = torch.where(usable[:, None, None], start, torch.full_like(start, float("nan")))
    else:
        start = init_model.detach()
    return _WeightedPnP.apply(matches, weights, start, mask, int(iters))


class _P3P(torch.autograd.Function):
    """dr_p3p / dr_p3p_bwd: the backward recomputes the poses from the samples (the forward's device function, so the forward's slot
    order), so no model is saved"""

    @staticmethod
    def forward(ctx, samples):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        s, Bt, _ = _flat_samples(samples, 5)
        models = torch.empty((Bt, 4, 4, 4), device=s.device, dtype=s.dtype)
        valid = torch.empty((Bt, 4), device=s.device, dtype=torch.bool)
        L.call(f"dr_p3p_{L.suffix(s.dtype)}", ptr(s), Bt, ptr(models), ptr(valid), stream())
        ctx.save_for_backward(s)
        ctx.sshape = samples.shape
        lead = samples.shape[:-2]
        valid = valid.reshape(*lead, 4)
        ctx.mark_non_differentiable(valid)
        return models.reshape(*lead, 4, 4, 4), valid

    @staticmethod
    def backward(ctx, g_models, _gv):
        if g_models is None:
            return None
        (s,) = ctx.saved_tensors
        gs = torch.empty_like(s)
        L.call(f"dr_p3p_bwd_{L.suffix(s.dtype)}", ptr(s), ptr(g_models.to(s.dtype).reshape(-1, 4, 4).contiguous()), s.shape[0], ptr(gs),
               stream())
        return gs.reshape(ctx.sshape)


def p3p(samples):
    """samples [..., 3, 5] = three (X, Y, Z, u, v) rows -> (models [..., 4, 4, 4], keep [..., 4] bool): the closed-form P3P poses of
    every sample with autograd to `samples` in f32 and f64 (dr_p3p, dr_p3p_bwd).  Slot j of a sample: the valid ones first, in
    ascending order of the quartic's root, the identity with keep = 0 elsewhere; on samples = matches[idx] the models and flags of
    p3p_gather bit for bit.  The backward is one launch: per valid slot the implicit function theorem on the six reprojection
    equations of the sample, at the slot's pose after one Gauss-Newton step onto their root (include/dransac.h states it); only rows 0-2 of a model's gradient are read, and the part of the
    rotation's gradient normal to the rotation manifold passes nothing on.  A slot that is invalid (a NaN in its gradient reaches
    nothing), whose Jacobian is singular to 1e-12 of its largest entry, or whose derivative is not finite passes exact zeros back."""
    if not isinstance(samples, torch.Tensor) or samples.dim() < 3 or samples.shape[-2:] != (3, 5):
        raise L.DransacError("p3p: samples [..., 3, 5], three matches (X, Y, Z, u, v) per sample")
    if samples.dtype not in (torch.float32, torch.float64):
        raise L.DransacError("p3p: samples must be float32 or float64")
    _gpu_only((samples,))
    return _P3P.apply(samples)


class _Homography4(torch.autograd.Function):
    """dr_homography4 / dr_homography4_bwd: the backward recomputes the closed form from the samples, so no model is saved"""

    @staticmethod
    def forward(ctx, samples):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        s, Bt, _ = _flat_samples(samples, 4)
        models = torch.empty((Bt, 3, 3), device=s.device, dtype=s.dtype)
        valid = torch.empty((Bt,), device=s.device, dtype=torch.bool)
        L.call(f"dr_homography4_{L.suffix(s.dtype)}", ptr(s), Bt, ptr(models), ptr(valid), stream())
        ctx.save_for_backward(s)
        ctx.sshape = samples.shape
        lead = samples.shape[:-2]
        valid = valid.reshape(lead)
        ctx.mark_non_differentiable(valid)
        return models.reshape(*lead, 3, 3), valid

    @staticmethod
    def backward(ctx, g_models, _gv):
        if g_models is None:
            return None
        (s,) = ctx.saved_tensors
        gs = torch.empty_like(s)
        L.call(f"dr_homography4_bwd_{L.suffix(s.dtype)}", ptr(s), ptr(g_models.to(s.dtype).reshape(-1, 3, 3).contiguous()), s.shape[0],
               ptr(gs), stream())
        return gs.reshape(ctx.sshape)


def homography4(samples):
    """samples [..., 4, 4] = four (x1, y1, x2, y2) rows -> (models [..., 3, 3], keep [...] bool): the closed-form homography of every
    sample with autograd to `samples` in f32 and f64 (dr_homography4, dr_homography4_bwd).  On samples = matches[idx] the models of
    homography4_gather bit for bit.  A sample without a valid model (keep = 0: the identity), or with a non-finite derivative, passes
    exact zeros back."""
    if samples.dim() < 3 or samples.shape[-2:] != (4, 4):
        raise L.DransacError("homography4: samples [..., 4, 4], four matches per sample")
    return _Homography4.apply(samples)


def weighted_homography(matches, weights=None, mask=None):
    """matches [P,N,4], weights [P,N] | None, mask [P,N] | None -> (model [P,3,3], valid [P] bool): refit_homography (the normalised
    DLT over the rows the mask selects, a row's weight multiplying its terms in the Gram matrix; the same entry, the same bits) with
    autograd to `weights` and / or `matches`, whichever require it (dr_refit_homography_bwd), in f32 and f64; once differentiable,
    `valid` and the mask carry no gradient.  Weights are expected >= 0 and are not checked, as in the forward.
    Zero rules: rows the mask drops get exact zeros and are never read (a NaN there reaches nothing); every row of a pair gets exact
    zeros when the pair has fewer than four rows, valid = 0, the smallest eigenvalue of its Gram matrix is not simple (or an
    eigenvalue gap is not finite), or an intermediate of the derivative is not finite.  A multiple of H in the incoming gradient
    passes nothing on.  Bit-repeatable."""
    _check_weighted("weighted_homography", _HOMOGRAPHY, matches, weights, mask)
    return _WeightedFit.apply(_HOMOGRAPHY, matches, weights, mask)


def weighted_fundamental(matches, weights=None, mask=None):
    """matches [P,N,4] (N >= 8), weights [P,N] | None, mask [P,N] | None -> (F [P,3,3], valid [P] bool): refit_fundamental (the
    Hartley-normalised weighted eight-point fit over the rows the mask selects; the same entry, the same bits) with autograd to
    `weights` and / or `matches`, whichever require it (dr_refit_fundamental_bwd), in f32 and f64; once differentiable, `valid` and the
    mask carry no gradient.  The weights scale the epipolar ROWS, so they enter the Gram matrix SQUARED (hand over sqrt(w) for a fit
    that minimises sum w r^2); they are not checked, as in the forward.  F is the denormalised smallest eigenvector as it comes: not
    normalised (its scale follows the Hartley transforms) and not rank 2.  On calibrated matches (K^-1 applied) it is the linear
    estimate of E, which MatchLoss / PoseLoss accept.
    Zero rules: rows the mask drops get exact zeros and are never read (a NaN there reaches nothing); every row of a pair gets exact
    zeros when the pair has fewer than eight rows, valid = 0, the smallest eigenvalue of its Gram matrix is not simple (or an
    eigenvalue gap is not finite), or an intermediate of the derivative is not finite.  Bit-repeatable."""
    _check_weighted("weighted_fundamental", _FUNDAMENTAL, matches, weights, mask)
    return _WeightedFit.apply(_FUNDAMENTAL, matches, weights, mask)


class _MsacScore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, matches, models, thr, want_masks):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        scores, masks = msac_score(matches, models, thr, want_masks)
        ctx.save_for_backward(matches, models, thr)
        if masks is not None:
            ctx.mark_non_differentiable(masks)
        return scores, masks

    @staticmethod
    def backward(ctx, g_scores, _gm):
        if g_scores is None:
            return None, None, None, None
        matches, models, thr = ctx.saved_tensors
        if matches.dtype != torch.float32:
            raise L.DransacError("backward is implemented for f32 only")
        P, N, _ = matches.shape
        M = models.shape[1]
        gm = torch.empty_like(models)
        L.call("dr_msac_score_bwd_f32", ptr(_al(matches.contiguous())), ptr(models.contiguous()), ptr(thr), ptr(g_scores.contiguous()), P,
               M, N, ptr(gm), stream())
        return None, gm, None, None


def msac_score_autograd(matches, models, threshold, want_masks=True):
    thr = _thr_tensor(threshold, matches.shape[0], matches)
    return _MsacScore.apply(matches, models.reshape(models.shape[0], -1, 3, 3), thr, want_masks)


class _RigidResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, models, threshold):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        res, masks = rigid_residual(pts, models, threshold, True)
        ctx.save_for_backward(pts, models)
        ctx.mark_non_differentiable(masks)
        return res, masks

    @staticmethod
    def backward(ctx, g_res, _gm):
        if g_res is None:
            return None, None, None
        pts, models = ctx.saved_tensors
        if pts.dtype != torch.float32:
            raise L.DransacError("backward is implemented for f32 only")
        P, N, _ = pts.shape
        M = models.shape[1]
        gm = torch.empty_like(models)
        L.call("dr_rigid_residual_bwd_f32", ptr(_al(pts.contiguous(), 8)), ptr(models.contiguous()), ptr(g_res.contiguous()), P, M, N, ptr(gm),
               stream())
        return None, gm, None


def rigid_residual_autograd(pts, models, threshold=0.03):
    return _RigidResidual.apply(pts, models, threshold)


class _SelectClosest(torch.autograd.Function):
    @staticmethod
    def forward(ctx, models, valid, gt):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        chosen, which, keep = select_closest(models, valid, gt, want_keep=True)
        ctx.save_for_backward(which)
        ctx.shape = models.shape
        ctx.mark_non_differentiable(which, keep)
        return chosen, which, keep

    @staticmethod
    def backward(ctx, g_chosen, _gw, _gk):
        if g_chosen is None:
            return None, None, None
        (which,) = ctx.saved_tensors
        P, B, S = ctx.shape[:3]
        g = torch.empty(ctx.shape, device=g_chosen.device, dtype=g_chosen.dtype)
        L.call(f"dr_select_closest_bwd_{L.suffix(g_chosen.dtype)}", ptr(g_chosen.contiguous()), ptr(which), P, B, S, ptr(g), stream())
        return g, None, None


def select_closest_autograd(models, valid, gt, want_keep: bool = False):
    """-> (chosen, which) or, with want_keep, (chosen, which, keep [P,B] bool = which >= 0, written by the same launch)."""
    chosen, which, keep = _SelectClosest.apply(models, valid, gt)
    return (chosen, which, keep) if want_keep else (chosen, which)


# ------------------------------------------------------------------------------------------ MatchLoss residual (8(f) rank 2)
def _episym_fwd(matches, mask, models, valid):
    """dr_episym_fwd_f32, the first launch of every reduction below -> (matches, models: contiguous; mask, valid: as bytes or None;
    sums [P,M]: every slot is written, an invalid one with 0)"""
    P, N, _ = matches.shape
    M = models.shape[1]
    matches, models = matches.contiguous(), models.contiguous()
    mk, v = _u8(mask), _u8(valid)
    sums = torch.empty((P, M), device=matches.device, dtype=matches.dtype)
    L.call("dr_episym_fwd_f32", ptr(_al(matches)), ptr(mk), ptr(models), ptr(v), P, M, N, ptr(sums), stream())
    return matches, models, mk, v, sums


# What is made of the sums, one record per reduction: the wrapper's name (for its messages), the entry launched after the episym
# forward (None: the sums are the result), the outputs that entry writes, in its order (the mean where there is one, else the
# per-pair means, is the result; coef is saved for the backward), the backward entry (one episym_kernel<1> launch each), and what
# stands in its gradient argument(s): (upstream gradient, [coef] as saved, dtype) -> tensors.
_Reduction = collections.namedtuple("_Reduction", "name reduce outs bwd grad")
_SUMS = _Reduction("episym_sums", None, (), "dr_episym_bwd_f32", lambda g, coef, dt: (g.contiguous(),))
# (the per-pair gradient goes straight into the episym backward: one tiny torch op, no [P,M] gradient tensor)
_PER_PAIR = _Reduction("match_loss_per_pair", "dr_match_loss_pair_f32", ("per_pair", "coef"), "dr_episym_bwd_pair_f32",
                       lambda g, coef, dt: ((g * coef[0]).contiguous(),))
# (per-pair means AND their mean over the pairs in one launch; dr_episym_bwd_mean reads the upstream scalar gradient from device memory)
_MEAN = _Reduction("match_loss_mean", "dr_match_loss_mean_f32", ("per_pair", "coef", "mean"), "dr_episym_bwd_mean_f32",
                   lambda g, coef, dt: (coef[0], g.to(dt).contiguous()))


class _Episym(torch.autograd.Function):
    """The episym forward and one reduction of its sums (`red` travels in ctx: a Function cannot be parameterised by instance): one
    launch, or two with a reduce entry; the backward is one launch."""

    @staticmethod
    def forward(ctx, red, matches, mask, models, valid):
        given = (matches, models)
        matches, models, mk, v, sums = _episym_fwd(matches, mask, models, valid)
        ctx.red, ctx.aux = red, (mk, v)
        if red.reduce is None:
            ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
            ctx.save_for_backward(*given)      # (as given: the backward makes them contiguous once more)
            return sums
        (P, N, _), M = matches.shape, models.shape[1]
        dev, dt = matches.device, matches.dtype
        per_pair, coef = torch.empty((P,), device=dev, dtype=dt), torch.empty((P,), device=dev, dtype=dt)
        mean = (torch.empty((), device=dev, dtype=dt),) if "mean" in red.outs else ()
        L.call(red.reduce, ptr(sums), ptr(mk), ptr(v), P, M, N, ptr(per_pair), ptr(coef), *map(ptr, mean), stream())
        ctx.save_for_backward(matches, models, coef)
        ctx.aux = (mk, v)
        return mean[0] if mean else per_pair

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None
        red = ctx.red
        matches, models, *coef = ctx.saved_tensors
        if red.reduce is None:
            matches, models = matches.contiguous(), models.contiguous()
        mk, v = ctx.aux
        P, N, _ = matches.shape
        M = models.shape[1]
        grad = red.grad(g, coef, matches.dtype)
        gm = torch.empty_like(models)   # every slot is written (invalid: 0)
        L.call(red.bwd, ptr(_al(matches)), ptr(mk), ptr(models), ptr(v), *map(ptr, grad), P, M, N, ptr(gm), stream())
        return None, None, None, gm, None


def _episym(red, matches, mask, models, valid):
    if matches.dtype != torch.float32:
        raise L.DransacError(f"{red.name} is implemented for f32")
    return _Episym.apply(red, matches, mask, models.reshape(models.shape[0], -1, 3, 3), valid)


def episym_sums(matches, mask, models, valid=None):
    """sum over masked points of min(symmetric epipolar error, 1) for every model: matches [P,N,4], mask [P,N] bool |
    None, models [P,M,3,3], valid [P,M] bool | None -> [P,M] (differentiable w.r.t. models, f32)."""
    return _episym(_SUMS, matches, mask, models, valid)


class _MatchLossFused(torch.autograd.Function):
    """MatchLoss value AND gradient in one pass (round 5: dr_match_loss_fused_f32): the forward writes, next to the loss, the
    unscaled gradient of every model; the backward is one elementwise launch (x coef[p] x upstream / P) -- no second walk over
    the (model x point) grid.  Taken in training (the models require grad)."""

    @staticmethod
    def forward(ctx, matches, mask, models, keep):
        P, N, _ = matches.shape
        M = models.shape[1]
        matches, models = matches.contiguous(), models.contiguous()
        mk, v = _u8(mask), _u8(keep)
        dev, dt = matches.device, matches.dtype
        sums = torch.empty((P, M), device=dev, dtype=dt)
        gun = torch.empty((P, M, 3, 3), device=dev, dtype=dt)
        per_pair = torch.empty((P,), device=dev, dtype=dt)
        coef = torch.empty((P,), device=dev, dtype=dt)
        mean = torch.empty((), device=dev, dtype=dt)
        L.call("dr_match_loss_fused_f32", ptr(_al(matches)), ptr(mk), ptr(models), ptr(v), P, M, N, ptr(sums), ptr(gun), ptr(per_pair),
               ptr(coef), ptr(mean), stream())
        ctx.save_for_backward(gun, coef)
        return mean

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        gun, coef = ctx.saved_tensors
        P, M = gun.shape[0], gun.shape[1]
        gm = torch.empty_like(gun)
        L.call("dr_match_loss_scale_f32", ptr(gun), ptr(coef), ptr(g.to(gun.dtype).contiguous()), P, M, ptr(gm), stream())
        return None, None, gm, None


def match_loss_mean(matches, mask, models, keep=None):
    """MatchLoss of a batch: mean over pairs of the per-pair means (match_loss_per_pair(...).mean()) -> scalar, with the mean
    and its backward folded into the kernels (P <= 64; larger batches take the per-pair kernel + torch.mean).  When the models
    require grad (training), value and gradient come from ONE pass over the (model x point) grid (_MatchLossFused)."""
    models = models.reshape(models.shape[0], -1, 3, 3)
    if matches.dtype == torch.float64:
        return _match_loss_mean_f64(matches, mask, models, keep)
    if matches.dtype != torch.float32:
        raise L.DransacError("match_loss_mean is implemented for f32 and f64")
    if FUSED_MATCH_LOSS and torch.is_grad_enabled() and models.requires_grad:
        return _MatchLossFused.apply(matches, mask, models, keep)
    if matches.shape[0] > 64:
        return match_loss_per_pair(matches, mask, models, keep).mean()
    return _Episym.apply(_MEAN, matches, mask, models, keep)


def _match_loss_mean_f64(matches, mask, models, keep, chunk: int = 256):
    """`-pr 2 -tr 1 -w2 1` (model_cl.py:164-169, Q17): MatchLoss in double precision.  The episym kernels are packed-f32 code; the
    f64 parity path evaluates loss.py:137-153 / cv_utils.py:680-695 with torch ops ON THE DEVICE (autograd provides the backward),
    `chunk` models at a time so that the [P, chunk, N] temporaries stay small.  Not a hot path: the training path is f32."""
    P, N, _ = matches.shape
    M = models.shape[1]
    one = torch.ones_like(matches[..., :1])
    x1 = torch.cat((matches[..., :2], one), -1)
    x2 = torch.cat((matches[..., 2:], one), -1)
    w_pt = torch.ones((P, N), device=matches.device, dtype=matches.dtype) if mask is None else mask.to(matches.dtype)
    w_md = torch.ones((P, M), device=matches.device, dtype=matches.dtype) if keep is None else keep.to(matches.dtype)
    total = torch.zeros((P,), device=matches.device, dtype=matches.dtype)
    for m0 in range(0, M, chunk):
        F = models[:, m0:m0 + chunk]
        if keep is not None:
            # dropped slots are SELECTED out, not multiplied by 0: an invalid f8 / LSQ hypothesis may be NaN, and NaN * 0 would
            # turn the loss and every gradient into NaN where the f32 kernels skip the slot (round-5 advice)
            F = torch.where(keep[:, m0:m0 + chunk, None, None].bool(), F, torch.zeros((), device=F.device, dtype=F.dtype))
        Fx1 = torch.einsum("pmij,pnj->pmni", F, x1)
        Ftx2 = torch.einsum("pmji,pnj->pmni", F, x2)
        r = (x2[:, None] * Fx1).sum(-1)
        ys = r ** 2 * (1.0 / (Fx1[..., 0] ** 2 + Fx1[..., 1] ** 2 + 1e-15) + 1.0 / (Ftx2[..., 0] ** 2 + Ftx2[..., 1] ** 2 + 1e-15))
        ys = ys.clamp(max=1.0)
        if mask is not None:
            ys = torch.where(mask[:, None, :].bool(), ys, torch.zeros((), device=ys.device, dtype=ys.dtype))
        total = total + (ys * w_md[:, m0:m0 + chunk, None]).sum((1, 2))
    den = (w_pt.sum(1) * w_md.sum(1)).clamp(min=1.0)
    return (total / den).mean()


def match_loss_per_pair(matches, mask, models, keep=None):
    """MatchLoss per pair: mean over the kept models and the masked points of min(symmetric epipolar error, 1).
    matches [P,N,4] f32, mask [P,N] bool | None, models [P,M,3,3], keep [P,M] bool | None -> [P] (differentiable w.r.t.
    models)."""
    return _episym(_PER_PAIR, matches, mask, models, keep)


# ------------------------------------------------------------------------------------------ the pair families' training losses
# RegistrationLoss (3-D path): the truncated squared distance of every model on the ground-truth inliers (include/dransac.h, "The
# training loss of the registration path"): matches [P,N,6], mask [P,N] bool | None, models [P,M,4,4], keep [P,M] bool | None.
# HomographyLoss (homography path): the truncated symmetric transfer error (include/dransac.h, "The training loss of the homography
# path"): matches [P,N,4], models [P,M,3,3] of any scale and either sign.  threshold = DISTANCE in both.  One implementation behind the
# family record (_PairFamily): the C entries dr_<entry>_{gt_mask,loss_fwd,loss_fused,loss_scale}, the match width, the model shape, the
# messages' nouns.
def _pair_gt_mask(fam, matches, gt_model, threshold):
    P, N, _ = matches.shape
    r, c = fam.shape
    if gt_model.shape != (P, r, c) or gt_model.dtype != matches.dtype:
        raise L.DransacError(f"{fam.entry}_gt_mask: one ground-truth {fam.gt_noun} [P,{r},{c}] per pair, in the {fam.points}' dtype")
    mask = torch.empty((P, N), device=matches.device, dtype=torch.bool)
    count = torch.empty((P,), device=matches.device, dtype=torch.int32)
    L.call(f"dr_{fam.entry}_gt_mask_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), ptr(gt_model.contiguous()),
           ptr(thr2_tensor(threshold, P, matches)), P, N, ptr(mask.view(torch.uint8)), ptr(count), stream())
    return mask, count


def _pair_loss_inputs(fam, matches, mask, models, keep):
    r, c = fam.shape
    if matches.dim() != 3 or matches.shape[-1] != fam.width or models.dim() != 4 or models.shape[-2:] != fam.shape or \
            models.shape[0] != matches.shape[0] or models.dtype != matches.dtype:
        raise L.DransacError(f"{fam.entry} loss: {fam.points} [P,N,{fam.width}] and models [P,M,{r},{c}] of one dtype")
    P, N, _ = matches.shape
    M = models.shape[1]
    if (mask is not None and mask.shape != (P, N)) or (keep is not None and keep.shape != (P, M)):
        raise L.DransacError(f"{fam.entry} loss: mask is [P,N], keep is [P,M]")
    return matches.contiguous(), _u8(mask), models.contiguous(), _u8(keep), P, M, N


def _pair_loss_fwd(fam, matches, mask, models, threshold, keep):
    """dr_<entry>_loss_fwd -> (sums [P,M], per_pair [P], coef [P], mean [])"""
    matches, mk, models, kp, P, M, N = _pair_loss_inputs(fam, matches, mask, models, keep)
    dev, dt = matches.device, matches.dtype
    sums = torch.empty((P, M), device=dev, dtype=dt)
    per_pair, coef, mean = torch.empty((P,), device=dev, dtype=dt), torch.empty((P,), device=dev, dtype=dt), torch.empty((), device=dev, dtype=dt)
    L.call(f"dr_{fam.entry}_loss_fwd_{L.suffix(dt)}", ptr(_al(matches)), ptr(mk), ptr(models), ptr(kp),
           ptr(thr2_tensor(threshold, P, matches)), P, M, N, ptr(sums), ptr(per_pair), ptr(coef), ptr(mean), stream())
    return sums, per_pair, coef, mean


class _PairLossFused(torch.autograd.Function):
    """A pair family's loss value AND gradient in one pass (dr_<entry>_loss_fused), as _MatchLossFused: the forward writes the
    unscaled gradient of every model next to the loss, the backward is one elementwise launch (x coef[p] x upstream / P) that reads
    the upstream scalar from device memory.  `fam` travels in ctx (a Function cannot be parameterised by instance)."""

    @staticmethod
    def forward(ctx, fam, matches, mask, models, keep, thr2):
        matches, mk, models, kp, P, M, N = _pair_loss_inputs(fam, matches, mask, models, keep)
        dev, dt = matches.device, matches.dtype
        sums = torch.empty((P, M), device=dev, dtype=dt)
        gun = torch.empty((P, M, *fam.shape), device=dev, dtype=dt)
        per_pair, coef, mean = torch.empty((P,), device=dev, dtype=dt), torch.empty((P,), device=dev, dtype=dt), torch.empty((), device=dev, dtype=dt)
        L.call(f"dr_{fam.entry}_loss_fused_{L.suffix(dt)}", ptr(_al(matches)), ptr(mk), ptr(models), ptr(kp), ptr(thr2), P, M, N,
               ptr(sums), ptr(gun), ptr(per_pair), ptr(coef), ptr(mean), stream())
        ctx.save_for_backward(gun, coef)
        ctx.fam = fam
        return mean

    @staticmethod
    @torch.autograd.function.once_differentiable       # (gun is a kernel result: a second derivative through it would be silently wrong)
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None, None
        gun, coef = ctx.saved_tensors
        P, M = gun.shape[0], gun.shape[1]
        gm = torch.empty_like(gun)
        L.call(f"dr_{ctx.fam.entry}_loss_scale_{L.suffix(gun.dtype)}", ptr(gun), ptr(coef), ptr(g.to(gun.dtype).contiguous()), P, M,
               ptr(gm), stream())
        return None, None, None, gm, None, None


def _pair_loss_mean(fam, matches, mask, models, threshold, keep):
    if torch.is_grad_enabled() and matches.requires_grad:
        raise L.DransacError(f"{fam.entry}_loss_mean is differentiable w.r.t. the models only: pass matches.detach()")
    if torch.is_grad_enabled() and models.requires_grad:
        return _PairLossFused.apply(fam, matches, mask, models, keep, thr2_tensor(threshold, matches.shape[0], matches))
    return _pair_loss_fwd(fam, matches, mask, models, threshold, keep)[3]


def _pair_loss_sums(fam, matches, mask, models, threshold, keep, want_pairs):
    sums, per_pair, _, _ = _pair_loss_fwd(fam, matches.detach(), mask, models.detach(), threshold, keep)
    return (sums, per_pair) if want_pairs else sums


def registration_gt_mask(matches: torch.Tensor, gt_pose: torch.Tensor, threshold):
    """dr_registration_gt_mask: matches [P,N,6], gt_pose [P,4,4], threshold (float or [P]) -> (mask [P,N] bool = the points within the
    distance threshold of the pair's ground-truth pose, count [P] int32)."""
    return _pair_gt_mask(_REGISTRATION, matches, gt_pose, threshold)


def registration_loss_mean(matches, mask, models, threshold, keep=None):
    """The registration loss of a batch -> scalar in [0, 1]: per pair the mean over (kept models x masked points) of
    min(d2 / threshold^2, 1), then the mean over the pairs.  Differentiable w.r.t. `models` only; when they require grad, value and
    gradient come from one pass over the (model x point) grid (_PairLossFused), otherwise the value-only kernel runs.
    Correspondences that require grad are refused (detach them): no gradient is computed for them, and BatchedRegistration(train=True)
    does pass one to `matches`, so a silent zero here would be half a gradient."""
    return _pair_loss_mean(_REGISTRATION, matches, mask, models, threshold, keep)


def registration_loss_sums(matches, mask, models, threshold, keep=None, want_pairs: bool = False):
    """sums [P,M] = sum over the masked points of min(d2 / threshold^2, 1) for every model (0 for a slot keep drops); no autograd.
    want_pairs: -> (sums, per_pair [P]) with the per-pair means registration_loss_mean averages."""
    return _pair_loss_sums(_REGISTRATION, matches, mask, models, threshold, keep, want_pairs)


def homography_gt_mask(matches: torch.Tensor, gt_H: torch.Tensor, threshold):
    """dr_homography_gt_mask: matches [P,N,4], gt_H [P,3,3], threshold (float or [P]) -> (mask [P,N] bool = the points homography_score
    counts as inliers of the pair's ground-truth homography, count [P] int32)."""
    _check_matches(_HOMOGRAPHY, "homography_gt_mask", matches)
    return _pair_gt_mask(_HOMOGRAPHY, matches, gt_H, threshold)


def homography_loss_mean(matches, mask, models, threshold, keep=None):
    """The homography loss of a batch -> scalar in [0, 1]: per pair the mean over (kept models x masked points) of d2 / threshold^2
    for a point in front of both cameras with d2 < threshold^2 and of 1 for any other, then the mean over the pairs.  Differentiable
    w.r.t. `models` only; when they require grad, value and gradient come from one pass over the (model x point) grid
    (_PairLossFused), otherwise the value-only kernel runs.  Matches that require grad are refused (detach them): no gradient
    is computed for them, and BatchedHomography(train=True) does pass one to `matches`, so a silent zero here would be half a gradient."""
    return _pair_loss_mean(_HOMOGRAPHY, matches, mask, models, threshold, keep)


def homography_loss_sums(matches, mask, models, threshold, keep=None, want_pairs: bool = False):
    """sums [P,M] = sum over the masked points of the truncated d2 / threshold^2 for every model (0 for a slot keep drops); no autograd.
    want_pairs: -> (sums, per_pair [P]) with the per-pair means homography_loss_mean averages."""
    return _pair_loss_sums(_HOMOGRAPHY, matches, mask, models, threshold, keep, want_pairs)


def pnp_gt_mask(matches: torch.Tensor, gt_pose: torch.Tensor, threshold):
    """dr_pnp_gt_mask: matches [P,N,5], gt_pose [P,4,4], threshold (float or [P]) -> (mask [P,N] bool = the points pnp_score counts
    as inliers of the pair's ground-truth pose, count [P] int32)."""
    _check_matches(_PNP, "pnp_gt_mask", matches)
    return _pair_gt_mask(_PNP, matches, gt_pose, threshold)


def pnp_loss_mean(matches, mask, models, threshold, keep=None):
    """The absolute-pose loss of a batch -> scalar in [0, 1]: per pair the mean over (kept models x masked points) of d2 / threshold^2
    for a point in front of the camera with d2 < threshold^2 and of 1 for any other (d2 = the squared reprojection error in normalised
    units), then the mean over the pairs.  Differentiable w.r.t. `models` only; when they require grad, value and gradient come from
    one pass over the (model x point) grid (_PairLossFused), otherwise the value-only kernel runs.  Matches that require grad are
    refused (detach them): no gradient is computed for them, and BatchedPnP.hypotheses does pass one to `matches`, so a silent zero
    here would be half a gradient."""
    _check_matches(_PNP, "pnp_loss_mean", matches)
    return _pair_loss_mean(_PNP, matches, mask, models, threshold, keep)


def pnp_loss_sums(matches, mask, models, threshold, keep=None, want_pairs: bool = False):
    """sums [P,M] = sum over the masked points of the truncated d2 / threshold^2 for every model (0 for a slot keep drops); no autograd.
    want_pairs: -> (sums, per_pair [P]) with the per-pair means pnp_loss_mean averages."""
    _check_matches(_PNP, "pnp_loss_sums", matches)
    return _pair_loss_sums(_PNP, matches, mask, models, threshold, keep, want_pairs)


class _SoftScore(torch.autograd.Function):
    """dr_<entry>_soft_score / dr_<entry>_soft_score_bwd on checked, contiguous inputs (_soft_score): the backward recomputes the
    residuals from the saved inputs, writes grad_models and, when the matches need a gradient, grad_matches by the transposed launch."""

    @staticmethod
    def forward(ctx, matches, models, thr2, beta, mask, keep, entry):
        (P, N, _), M, dt = matches.shape, models.shape[1], matches.dtype
        scores = torch.empty((P, M), device=matches.device, dtype=dt)
        L.call(f"dr_{entry}_soft_score_{L.suffix(dt)}", ptr(_al(matches)), ptr(mask), ptr(models), ptr(keep), ptr(thr2), L.scalar(dt, beta),
               P, M, N, ptr(scores), stream())
        ctx.save_for_backward(matches, models, thr2, mask, keep)
        ctx.beta, ctx.entry = beta, entry
        return scores

    @staticmethod
    @torch.autograd.function.once_differentiable       # (the gradients are kernel results: a second derivative would be silently wrong)
    def backward(ctx, g):
        matches, models, thr2, mask, keep = ctx.saved_tensors
        (P, N, _), M, dt = matches.shape, models.shape[1], matches.dtype
        gm = torch.empty_like(models)
        gx = torch.empty_like(matches) if ctx.needs_input_grad[0] else None
        L.call(f"dr_{ctx.entry}_soft_score_bwd_{L.suffix(dt)}", ptr(_al(matches)), ptr(mask), ptr(models), ptr(keep), ptr(thr2),
               L.scalar(dt, ctx.beta), ptr(g.to(dt).contiguous()), P, M, N, ptr(gm), ptr(gx), stream())
        return gx, gm, None, None, None, None, None


def _soft_score(fam, name, matches, models, threshold, beta, mask, keep):
    """the argument checks of the soft-inlier scores (before any launch), then _SoftScore on the family's entries"""
    r, c = fam.shape
    _check_matches(fam, name, matches)
    if matches.dim() != 3 or matches.shape[-1] != fam.width:      # (a family whose record carries no shape text)
        raise L.DransacError(f"{name}: {fam.points} [P,N,{fam.width}]")
    if models.dim() != 4 or models.shape[-2:] != fam.shape or models.shape[0] != matches.shape[0]:
        raise L.DransacError(f"{name}: models [P,M,{r},{c}], one row of {fam.gt_noun}s per row of matches")
    if models.dtype != matches.dtype or matches.dtype not in (torch.float32, torch.float64):
        raise L.DransacError(f"{name}: matches and models of one dtype, float32 or float64")
    (P, N, _), M = matches.shape, models.shape[1]
    if (mask is not None and (mask.shape != (P, N) or mask.dtype != torch.bool)) or \
            (keep is not None and (keep.shape != (P, M) or keep.dtype != torch.bool)):
        raise L.DransacError(f"{name}: mask is [P,N] bool, keep is [P,M] bool")
    if isinstance(beta, torch.Tensor) or not 0.0 < float(beta) < float("inf"):      # (false for NaN)
        raise L.DransacError(f"{name}: beta is a positive, finite Python number, got {beta!r}")
    _gpu_only((matches, models))
    _gpu_only((mask, keep), optional=True)
    return _SoftScore.apply(matches.contiguous(), models.contiguous(), thr2_tensor(threshold, P, matches).detach(), float(beta),
                            _u8(mask), _u8(keep), fam.entry)


def pnp_soft_score(matches, models, threshold, beta: float = 5.0, mask=None, keep=None):
    """The differentiable soft-inlier score (DSAC) of every pose on every point: matches [P,N,5], models [P,M,4,4], threshold = the
    inlier DISTANCE (float or [P]), beta > 0, mask [P,N] bool | None (the points that are scored), keep [P,M] bool | None ->
    scores [P,M] = sum over the scored points of sigmoid(beta (1 - d2 / threshold^2)), d2 the squared reprojection error; a point
    behind the camera or with beta (1 - d2 / threshold^2) < -40 adds nothing (include/dransac.h states the rules).  A slot keep drops
    and a kept model with a non-finite entry score 0.  Differentiable (once) w.r.t. `models`, and w.r.t. `matches` when they require
    grad: the second pass over the grid runs only then.  No gradient for threshold, beta, mask or keep.  f32 and f64; nothing
    synchronises or reads back, so the op can be captured in a HIP graph."""
    return _soft_score(_PNP, "pnp_soft_score", matches, models, threshold, beta, mask, keep)


def registration_soft_score(matches, models, threshold, beta: float = 5.0, mask=None, keep=None):
    """The differentiable soft-inlier score (DSAC) of every rigid model on every correspondence: matches [P,N,6] = (p, q), models
    [P,M,4,4], threshold = the inlier DISTANCE (float or [P]), beta > 0, mask [P,N] bool | None (the points that are scored),
    keep [P,M] bool | None -> scores [P,M] = sum over the scored points of sigmoid(beta (1 - d2 / threshold^2)), d2 = |R p + t - q|^2;
    a point with beta (1 - d2 / threshold^2) < -40 adds nothing (include/dransac.h states the rules).  A slot keep drops, a kept model
    with a non-finite entry and a pair whose threshold is not > 0 score 0.  Differentiable (once) w.r.t. `models`, and w.r.t. `matches`
    when they require grad: the second pass over the grid runs only then.  No gradient for threshold, beta, mask or keep.  f32 and
    f64; nothing synchronises or reads back, so the op can be captured in a HIP graph."""
    return _soft_score(_REGISTRATION, "registration_soft_score", matches, models, threshold, beta, mask, keep)


def homography_soft_score(matches, models, threshold, beta: float = 5.0, mask=None, keep=None):
    """The differentiable soft-inlier score (DSAC) of every homography on every match: matches [P,N,4] = (x1, y1, x2, y2), models
    [P,M,3,3], threshold = the inlier DISTANCE in pixels (float or [P]), beta > 0, mask [P,N] bool | None (the points that are scored),
    keep [P,M] bool | None -> scores [P,M] = sum over the scored points of sigmoid(beta (1 - d2 / threshold^2)), d2 the squared
    symmetric transfer error of the score kernels and of HomographyLoss (y = H (x1, 1), z = adj(H) (x2, 1) under the det > 0 sign,
    d2 = |x2 - y_xy / y_w|^2 + |x1 - z_xy / z_w|^2); a point behind either camera (y_w <= 0 or z_w <= 0) or with
    beta (1 - d2 / threshold^2) < -40 adds nothing (include/dransac.h states the rules).  The score does not depend on the scale or
    the sign of a model.  A slot keep drops, a kept model with a non-finite entry or a zero or non-finite determinant and a pair whose
    threshold is not > 0 score 0.  Differentiable (once) w.r.t. `models`, and w.r.t. `matches` when they require grad: the second pass
    over the grid runs only then.  No gradient for threshold, beta, mask or keep.  f32 and f64; nothing synchronises or reads back,
    so the op can be captured in a HIP graph."""
    return _soft_score(_HOMOGRAPHY, "homography_soft_score", matches, models, threshold, beta, mask, keep)


# ------------------------------------------------------------------------------------------ PoseLoss pose error (8(f) rank 3)
class _PoseError(torch.autograd.Function):
    @staticmethod
    def forward(ctx, matches, models, gt_R, gt_t, distance_threshold, want_votes):
        ctx.set_materialize_grads(False)   # unused / non-differentiable outputs arrive as None, not as zero-filled tensors
        P, N, _ = matches.shape
        M = models.shape[1]
        dev, dt = matches.device, matches.dtype
        sfx = L.suffix(dt)
        matches, models = matches.contiguous(), models.contiguous()
        gt_R, gt_t = gt_R.to(dt).contiguous(), gt_t.to(dt).contiguous()
        err_R = torch.empty((P, M), device=dev, dtype=dt)
        err_t = torch.empty((P, M), device=dev, dtype=dt)
        which = torch.empty((P, M), device=dev, dtype=torch.int32)
        votes = torch.empty((P, M, 4), device=dev, dtype=torch.int32) if want_votes else None
        L.call(f"dr_pose_error_fwd_{sfx}", ptr(_al(matches)), ptr(models), ptr(gt_R), ptr(gt_t), P, M, N, float(distance_threshold),
               ptr(err_R), ptr(err_t), ptr(which), ptr(votes), stream())
        ctx.save_for_backward(models, gt_R, gt_t, which)
        ctx.mark_non_differentiable(which)
        if votes is not None:
            ctx.mark_non_differentiable(votes)
        return err_R, err_t, which, votes

    @staticmethod
    def backward(ctx, g_R, g_t, _gw, _gv):
        if g_R is None and g_t is None:
            return (None,) * 6
        models, gt_R, gt_t, which = ctx.saved_tensors
        P, M = which.shape
        gm = torch.empty_like(models)
        zero = None
        if g_R is None or g_t is None:
            zero = torch.zeros((P, M), device=models.device, dtype=models.dtype)
        g_R = zero if g_R is None else g_R.contiguous()
        g_t = zero if g_t is None else g_t.contiguous()
        L.call(f"dr_pose_error_bwd_{L.suffix(models.dtype)}", ptr(models), ptr(gt_R), ptr(gt_t), ptr(which), ptr(g_R), ptr(g_t), P, M,
               ptr(gm), stream())
        return None, gm, None, None, None, None


def pose_error(matches, models, gt_R, gt_t, distance_threshold: float = 50.0, want_votes: bool = False, svd: bool = False):
    """eval_essential_matrix (cv_utils.py:503-525) for all models of all pairs: matches [P,N,4] normalised,
    models [P,M,3,3], gt_R [P,3,3], gt_t [P,3] -> err_R, err_t [P,M] in degrees, the chosen candidate [P,M]
    (0..3 = (R1,t) (R2,t) (R1,-t) (R2,-t)) and, optionally, the four cheirality votes.
    svd=False: Horn decomposition (what train.py passes), differentiable w.r.t. the models.  svd=True: the SVD
    decomposition of decompose_E (cv_utils.py:83-116), forward only -- the reference's gradient goes through
    torch.linalg.svd of a matrix with two equal singular values, where it does not exist."""
    P = matches.shape[0]
    models = models.reshape(P, -1, 3, 3)
    if not svd:
        return _PoseError.apply(matches, models, gt_R.reshape(P, 9), gt_t.reshape(P, 3), distance_threshold, want_votes)
    if models.requires_grad and torch.is_grad_enabled():
        raise L.DransacError("pose_error(svd=True) is forward only: the gradient through the SVD of an essential matrix "
                             "(sigma_1 = sigma_2) is undefined; use svd=False (Horn) for training, as train.py does")
    N, M = matches.shape[1], models.shape[1]
    dev, dt = matches.device, matches.dtype
    err_R = torch.empty((P, M), device=dev, dtype=dt)
    err_t = torch.empty((P, M), device=dev, dtype=dt)
    which = torch.empty((P, M), device=dev, dtype=torch.int32)
    votes = torch.empty((P, M, 4), device=dev, dtype=torch.int32) if want_votes else None
    # keep every converted tensor alive until the launch is enqueued: a temporary passed straight to ptr() is freed at
    # once and the caching allocator hands its block to the next temporary
    mt_, md_ = matches.contiguous(), models.detach().contiguous()
    gR_, gt_ = gt_R.reshape(P, 9).to(dt).contiguous(), gt_t.reshape(P, 3).to(dt).contiguous()
    L.call(f"dr_pose_error_svd_fwd_{L.suffix(dt)}", ptr(mt_), ptr(md_), ptr(gR_), ptr(gt_), P, M, N, float(distance_threshold),
           ptr(err_R), ptr(err_t), ptr(which), ptr(votes), stream())
    return err_R, err_t, which, votes


def recover_pose_mask(matches, models, distance_threshold: float = 50.0):
    """The inlier mask of cv2.recoverPose(E, pts1, pts2) (what loss.py:99,134 uses as ground-truth inliers): matches
    [P,N,4] normalised, models [P,M,3,3] or [P,3,3] -> (mask [P,M,N] bool, which [P,M] int32 = winning candidate)."""
    P, N, _ = matches.shape
    models = models.reshape(P, -1, 3, 3).to(matches.dtype).contiguous()
    M = models.shape[1]
    mask = torch.empty((P, M, N), device=matches.device, dtype=torch.bool)
    which = torch.empty((P, M), device=matches.device, dtype=torch.int32)
    L.call(f"dr_recover_pose_mask_{L.suffix(matches.dtype)}", ptr(_al(matches.contiguous())), ptr(models), P, M, N,
           float(distance_threshold), ptr(which), ptr(mask), stream())
    return mask, which
