"""f64 reference, rounding bounds, launch-path restatement and sentinel harness of the scoring kernels K4 (dr_msac_score,
csrc/msac_score.hip) and K4r (dr_rigid_residual, csrc/solve_rigid.hip).  Plain torch / numpy; no project kernel is used
by the reference.  tests/test_msac_ref.py checks this file on the host, tests/test_gpu_msac_paths.py uses it on the GPU.

Rounding model.  u = 2^-24 (f32) or 2^-53 (f64) is the unit roundoff; every count below is for the expression AS WRITTEN
with a separate multiply and add (the contraction of a * b + c to one FMA only removes roundings, so the counts hold for
every kernel of the family: packed, FMA-chained or generic).

  a_k = x2 m_k + (y2 m_{3+k} + m_{6+k})         the deepest term passes a multiply and two adds: |da_k| <= 3 u A_k,
                                                A_k = |x2 m_k| + |y2 m_{3+k}| + |m_{6+k}|  (b_k, B_k alike)
  r   = x1 a_0 + (y1 a_1 + a_2)                 3 u Rabs handed on by the a_k + 3 u Rabs of its own chain:
                                                |dr| <= 6 u Rabs,  Rabs = |x1| A_0 + |y1| A_1 + A_2
  d2  = r^2 / jj  =>  from r:  (2 |r| dr + dr^2) / jj  =  u * K_R |r| Rabs / jj  +  (u K_R Rabs / 2)^2 / jj,   K_R = 2 * 6 = 12
  relative to d2:  r * r                    1
                   jj = a0^2 + (a1^2 + (b0^2 + b1^2)), positive terms, deepest: a multiply and three adds   4
                   v_rcp_f32, 1 ulp = 2 u   2
                   (r r) * rcp              1
                   ... * inv_thr2 (the final multiply; exact inside the clamped FMA, rounded in the 8-point kernel)   1
                   inv_thr2 = 1 / (t t), t = 1.5 thr: t enters squared (2), t t (1), the division (1)   4
                                            K_J = 1 + 4 + 2 + 1 + 1 + 4 = 13
                   the da_k, db_k inside jj: 2 * 3 u * sum(|a_k| A_k + |b_k| B_k) / jj = K_A u cj,   K_A = 6,
                   cj >= 1 the cancellation of the a_k, b_k (1 when none of them cancels), applied per byte
  bound = u * (K_R |r| Rabs / jj + (K_J + K_A cj) d2) + (u K_R Rabs / 2)^2 / jj

The inlier test itself adds nothing: 1 - pq * inv_thr2 is ONE rounding (clamped FMA), positive exactly when pq * inv_thr2 < 1.

Score.  A term max(0, 1 - d2 / thr2) is 1-Lipschitz in d2 / thr2, so the terms of a row are off by at most
sum_n bound_n / thr2 over the points with d2 < thr2 + 2 bound (all others are 0 on both sides).  The sum of the (non-negative)
terms loses at most depth * u relative: 16 sequential adds of a lane's points (the longest of the kernels: 16 / 8 / 4 per lane),
6 steps of the wave tree, chunks_per_block accumulations of the LDS partial, 3 adds of the waves' partials, ny atomic adds
onto the zeroed score, and 1 for the rounding of the term's own FMA:  C_RED = 16 + 6 + 3 + 1 + chunks_per_block + ny.
  |score - ref| <= 2 * (sum_n bound_n / thr2 + C_RED u ref)

K4r, d2 = sum_i e_i^2, e_i = (((q_i - t_i) - R_i2 p_2) - R_i1 p_1) - R_i0 p_0: the deepest term passes four operations,
|de_i| <= 4 u Eabs_i (Eabs_i = |q_i| + |t_i| + sum_j |R_ij p_j|); e_i * e_i and the three adds of the chain: 4 u d2:
  bound = u * (K_RE sum_i |e_i| Eabs_i + K_RD d2) + (u K_RE / 2)^2 sum_i Eabs_i^2,   K_RE = 2 * 4 = 8,  K_RD = 4
The residual sum runs over ALL points: |sum - ref| <= 2 * (sum_n bound_n + C_RED u ref), C_RED = 8 + 6 + 3 + cpb + ny.
"""
import numpy as np
import torch

U32, U64 = 2.0 ** -24, 2.0 ** -53
K_R, K_J, K_A = 12, 13, 6
K_RE, K_RD = 8, 4
SAFETY = 2.0                  # the safety factor of tests/test_gpu_gradients.py
CAP_BYTES, CAP_INLIERS = 1e-3, 1e-2
MASK_SENTINEL = 0xA5
SCORE_SENTINEL = -12345.6787109375     # exactly representable in f32; a score is >= 0 or NaN
MASK_GUARD, SCORE_GUARD = 256, 64      # bytes
SIGMAS = (0.0, 1e-4, 1e-3, 1e-2, 5e-2)
THR, THR_HUGE, THR_TINY = 7.5e-4, 1e3, 1e-9
F64 = torch.float64


def unit(dtype):
    return U32 if dtype == torch.float32 else U64


def c_red(chunks_per_block, ny):
    return 16 + 6 + 3 + 1 + chunks_per_block + ny


def c_red_rigid(chunks_per_block, ny):
    return 8 + 6 + 3 + chunks_per_block + ny


# --------------------------------------------------------------------------------------------- the launch paths, restated
def dispatch(P, M, N, dtype=torch.float32, mask_aligned=True):
    """msac_score_launch -> (kernel, slots_per_half, ny, chunks_per_block, use_atomic).  kernel: 'small1' / 'small2' / 'small4'
    (N <= 256), 'fast16' (16 points per lane), 'fast8' (8 points per lane), 'generic' (f64).  slots_per_half: the model slots a
    fast16 half owns (16 or 64), or the kernel's tile.  mask_aligned: the mask base is 16-byte aligned (or there are no masks)."""
    f32 = dtype == torch.float32
    if f32 and N <= 256:
        return ("small1" if N <= 64 else "small2" if N <= 128 else "small4"), 16, 1, 1, False
    fast16 = f32 and N % 16 == 0 and mask_aligned
    small_grid = fast16 and P * ((M + 127) // 128) < 512
    slots = (16 if small_grid else 64) if fast16 else (64 if f32 else 32)
    tile = 2 * slots if fast16 else slots
    tiles = (M + tile - 1) // tile
    chunks = (N + 2047) // 2048
    ny, base = 1, P * tiles
    if chunks > 1 and base < 2048:
        ny = min(chunks, (2048 + base - 1) // base)
    cpb = (chunks + ny - 1) // ny
    ny = (chunks + cpb - 1) // cpb
    return ("fast16" if fast16 else "fast8" if f32 else "generic"), slots, ny, cpb, ny > 1


def rigid_dispatch(P, M, N, threshold, dtype=torch.float32, want_masks=True, cus=256):
    """rigid_residual_launch -> (kernel, tile, ny, chunks_per_block): 'pk8' = rigid_residual_kernel_f32_pk<8> with its per-launch tile
    (an even value in [4, 64], from the resident 2-wave blocks of `cus` compute units), or 'general' (32-slot tiles)."""
    thr32 = float(np.float32(threshold))
    if dtype == torch.float32 and want_masks and N % 16 == 0 and np.float32(thr32) > np.float32(1e-12):
        resident = 12 * max(cus, 1)
        ny = (N + 1023) // 1024
        per_tile = P * ny
        min_tiles = (M + 63) // 64
        rounds = max(1, (per_tile * min_tiles + resident - 1) // resident)
        tiles_t = max(min_tiles, rounds * resident // per_tile)
        tile = (M + tiles_t - 1) // tiles_t
        tile = min(64, max(4, (tile + 1) & ~1))
        return "pk8", tile, ny, 1
    tiles = (M + 31) // 32
    chunks = (N + 2047) // 2048
    ny, base = 1, P * tiles
    if chunks > 1 and base < 2048:
        ny = min(chunks, (2048 + base - 1) // base)
    cpb = (chunks + ny - 1) // ny
    return "general", 32, (chunks + cpb - 1) // cpb, cpb


# --------------------------------------------------------------------------------------------- the shapes of the GPU tests
SHORT_N, SHORT_M = (1, 63, 64, 65, 128, 129, 255, 256), (1, 15, 16, 17, 33)
F16S_P, F16S_N = (1, 3), (272, 2032, 2048, 2064, 4096)
F16S_M = (1, 15, 16, 17, 31, 32, 33, 47, 64, 65)
F16L = tuple((512, m, 272) for m in (1, 31, 32, 33, 63, 64, 65, 127, 128)) + tuple((256, m, 272) for m in (129, 191, 256))
F16L_ATOMIC, F16L_RELOAD, F16S_CHUNKS = (512, 128, 2064), (2048, 70, 2064), (256, 128, 6160)
F8_N, F8_N16, F8_M = (257, 263, 264, 2047, 2049, 2056), (272, 2064), (1, 63, 64, 65)
F64_N, F64_M = (1, 7, 2049), (1, 31, 32, 33)
RIGID_P, RIGID_M, RIGID_N = (1, 3), (1, 3, 4, 5, 33, 34, 35, 70), (16, 2048, 2064, 4112)
# the listed shapes all get the smallest tile, 4; these get (on 256 compute units) 6, 34 (the benchmark's c4 tile) and 64 = kR16MaxTile,
# each with a partial last tile (4, 8 and 16 models)
RIGID_TILE6, RIGID_TILE34, RIGID_TILE64 = (3, 1000, 4112), (50, 2048, 64), (96, 2000, 64)


def intended_paths():
    """[(P, M, N, dtype, mask_aligned, expected dispatch() fields)]: every shape of tests/test_gpu_msac_paths.py with the path it
    is meant to reach; None = any value."""
    f32, f64 = torch.float32, torch.float64
    out = []
    for n in SHORT_N:
        k = "small1" if n <= 64 else "small2" if n <= 128 else "small4"
        out += [(3, m, n, f32, a, (k, 16, 1, 1, False)) for m in SHORT_M for a in (True, False)]
    for p in F16S_P:
        for n in F16S_N:
            ny = 2 if n > 2048 else 1
            out += [(p, m, n, f32, True, ("fast16", 16, ny, 1, ny > 1)) for m in F16S_M]
    out += [(p, m, n, f32, True, ("fast16", 64, 1, 1, False)) for p, m, n in F16L]
    out.append(F16L_ATOMIC + (f32, True, ("fast16", 64, 2, 1, True)))
    out.append(F16L_RELOAD + (f32, True, ("fast16", 64, 1, 2, False)))
    out.append(F16S_CHUNKS + (f32, True, ("fast16", 16, 2, 2, True)))
    for n in F8_N:
        out += [(3, m, n, f32, a, ("fast8", 64, 2 if n > 2048 else 1, 1, n > 2048)) for m in F8_M for a in (True, False)]
    for n in F8_N16:
        out += [(3, m, n, f32, False, ("fast8", 64, 2 if n > 2048 else 1, 1, n > 2048)) for m in F8_M]
    for n in F64_N:
        out += [(3, m, n, f64, True, ("generic", 32, 2 if n > 2048 else 1, 1, n > 2048)) for m in F64_M]
    return out


# --------------------------------------------------------------------------------------------- references
def sampson_ref(matches, models, thr, u=U32):
    """matches [N,4], models [M,3,3] or [M,9], thr = the threshold value the kernel is handed -> dict of f64 tensors:
    d2 [M,N], bound [M,N] (the forward bound of the module docstring), scores [M] (NaN for a non-finite or all-zero model),
    masks [M,N] bool, excl [M,N] bool (|d2 - thr2| <= 2 bound: the bytes that may differ), score_slack [M] (sum_n bound_n / thr2
    over the points that can hold a non-zero term), nan [M] bool, and the sums of absolute terms Rabs, A [M,3,N], B [M,2,N], cj."""
    mt = matches.to(F64)
    md = models.to(F64).reshape(-1, 9)
    x1, y1, x2, y2 = (mt[:, i][None] for i in range(4))
    m = [md[:, q][:, None] for q in range(9)]
    thr2 = (1.5 * float(thr)) ** 2
    a = [x2 * m[k] + y2 * m[3 + k] + m[6 + k] for k in range(3)]
    A = [(x2 * m[k]).abs() + (y2 * m[3 + k]).abs() + m[6 + k].abs() for k in range(3)]
    b = [x1 * m[3 * k] + y1 * m[3 * k + 1] + m[3 * k + 2] for k in range(2)]
    B = [(x1 * m[3 * k]).abs() + (y1 * m[3 * k + 1]).abs() + m[3 * k + 2].abs() for k in range(2)]
    r = x1 * a[0] + y1 * a[1] + a[2]
    Rabs = x1.abs() * A[0] + y1.abs() * A[1] + A[2]
    jj = a[0] ** 2 + a[1] ** 2 + b[0] ** 2 + b[1] ** 2
    d2 = r * r / jj
    cj = (a[0].abs() * A[0] + a[1].abs() * A[1] + b[0].abs() * B[0] + b[1].abs() * B[1]) / jj
    bound = u * (K_R * r.abs() * Rabs / jj + (K_J + K_A * cj) * d2) + (u * K_R * Rabs / 2) ** 2 / jj
    nan = ~torch.isfinite(md).all(-1) | (md == 0).all(-1)
    good = ~nan[:, None]
    masks = (d2 < thr2) & good                       # a 0/0 point: d2 = NaN, no inlier
    term = torch.where(masks, 1 - d2 / thr2, torch.zeros_like(d2))
    scores = term.sum(-1)
    scores[nan] = float("nan")
    bound = torch.where(torch.isfinite(bound), bound, torch.full_like(bound, float("inf")))
    excl = ((d2 - thr2).abs() <= SAFETY * bound) & good & torch.isfinite(d2)
    near = (d2 < thr2 + SAFETY * bound) & good
    slack = torch.where(near, bound, torch.zeros_like(bound)).sum(-1) / thr2
    return dict(d2=d2, bound=bound, scores=scores, masks=masks, excl=excl, score_slack=slack, nan=nan, Rabs=Rabs,
                A=torch.stack(A, 1), B=torch.stack(B, 1), cj=cj, thr2=thr2)


def rigid_ref(pts, models, threshold, u=U32):
    """pts [N,6] = (p, q), models [M,4,4], threshold compared with d2 as it is -> dict like sampson_ref (scores = the residual sums)."""
    x = pts.to(F64)
    md = models.to(F64).reshape(-1, 16)
    p, q = x[:, :3], x[:, 3:]
    d2 = torch.zeros(md.shape[0], x.shape[0], dtype=F64)
    eabs_sum, eabs2 = torch.zeros_like(d2), torch.zeros_like(d2)
    for i in range(3):
        R, t = md[:, 4 * i:4 * i + 3], md[:, 4 * i + 3][:, None]
        e = q[:, i][None] - t - R @ p.T
        Eabs = q[:, i].abs()[None] + t.abs() + R.abs() @ p.abs().T
        d2 = d2 + e * e
        eabs_sum = eabs_sum + e.abs() * Eabs
        eabs2 = eabs2 + Eabs ** 2
    bound = u * (K_RE * eabs_sum + K_RD * d2) + (u * K_RE / 2) ** 2 * eabs2
    thr = float(threshold)
    masks = d2 < thr
    return dict(d2=d2, bound=bound, scores=d2.sum(-1), masks=masks, excl=(d2 - thr).abs() <= SAFETY * bound,
                score_slack=bound.sum(-1), nan=torch.zeros(md.shape[0], dtype=torch.bool), thr2=thr)


def stack_refs(refs, cred, u=U32):
    """per-set references (sampson_ref / rigid_ref dicts) -> the expectation compare() takes: masks / excl [S,M,N], scores / tol
    [S,M] with tol = 2 (slack + C_RED u ref), nan [S,M]"""
    sc = torch.stack([r["scores"] for r in refs])
    tol = SAFETY * (torch.stack([r["score_slack"] for r in refs]) + cred * u * sc.abs().nan_to_num())
    return dict(masks=torch.stack([r["masks"] for r in refs]), excl=torch.stack([r["excl"] for r in refs]), scores=sc, tol=tol,
                nan=torch.stack([r["nan"] for r in refs]))


# --------------------------------------------------------------------------------------------- inputs
def two_view_sets(S, M, N, seed, dtype=torch.float32, specials=()):
    """S distinct (matches [N,4], models [M,3,3]) sets from synth.two_view_pair: models = gt_E + sigma * randn with sigma cycling
    through SIGMAS over the slots (a model does not depend on M: smaller M = the leading slots).
    specials: (slot, 'nan' | 'inf' | 'zero' | 'm0') -- 'm0' = only m[0] set, and point 0 of the set moved to x1 = x2 = 0 (a 0/0 point)."""
    from differentiable_ransac_amd import synth
    mts, mds = [], []
    for s in range(S):
        pair = synth.two_view_pair(seed + s, max(N, 8))
        g = torch.Generator().manual_seed(seed * 131 + s)
        sig = torch.tensor(SIGMAS, dtype=F64)[torch.arange(M) % len(SIGMAS)]
        md = pair["gt_E"].to(F64)[None] + sig[:, None, None] * torch.randn(M, 3, 3, generator=g, dtype=F64)
        mt = pair["matches"][:N].to(F64).clone()
        for slot, kind in specials:
            if slot >= M:
                continue
            if kind == "nan":
                md[slot, 1, 1] = float("nan")
            elif kind == "inf":
                md[slot, 2, 0] = float("inf")
            elif kind == "zero":
                md[slot] = 0.0
            elif kind == "m0":
                md[slot] = 0.0
                md[slot, 0, 0] = 1.0
                mt[0, 0] = 0.0
                mt[0, 2] = 0.0
        mts.append(mt.to(dtype))
        mds.append(md.to(dtype))
    return torch.stack(mts), torch.stack(mds)


def rigid_sets(S, M, N, seed, dtype=torch.float32):
    from differentiable_ransac_amd import synth
    pts, mds = [], []
    for s in range(S):
        pair = synth.rigid_pair(seed + s, max(N, 8))
        g = torch.Generator().manual_seed(seed * 137 + s)
        sig = torch.tensor(SIGMAS, dtype=F64)[torch.arange(M) % len(SIGMAS)]
        md = pair["gt_T"].to(F64)[None].repeat(M, 1, 1)
        md[:, :3, :] += sig[:, None, None] * torch.randn(M, 3, 4, generator=g, dtype=F64)
        pts.append(pair["matches"][:N].to(dtype))
        mds.append(md.to(dtype))
    return torch.stack(pts), torch.stack(mds)


VALID_PATTERNS = ("all", "none", "one", "all_but_one", "alternating", "second_word", "last_partial_word")


def valid_pattern(name, P, M):
    """[P,M] bool, laid out per 32-slot word (slot m = word m // 32, bit m % 32); the single slot moves with the pair"""
    m = torch.arange(M)[None].expand(P, M)
    p = torch.arange(P)[:, None].expand(P, M)
    w, b = m // 32, m % 32
    return {"all": torch.ones(P, M, dtype=torch.bool), "none": torch.zeros(P, M, dtype=torch.bool),
            "one": b == (3 + 7 * p) % 32, "all_but_one": b != (5 + 11 * p) % 32, "alternating": (b + p) % 2 == 0,
            "second_word": w % 2 == 1, "last_partial_word": w == (M - 1) // 32}[name].clone()


# --------------------------------------------------------------------------------------------- the f32 emulation (host)
def emulate_f32(matches, models, thr, valid=None):
    """msac_pair_term in numpy float32, one rounding per operation as written (no contraction), a correctly rounded reciprocal;
    the row sum in f32 (numpy's pairwise order) -> (scores f32 [M], masks uint8 [M,N])"""
    f = np.float32
    mt = matches.numpy().astype(f)
    md = models.reshape(-1, 9).numpy().astype(f)
    x1, y1, x2, y2 = (mt[None, :, i] for i in range(4))
    m = [md[:, q][:, None] for q in range(9)]
    with np.errstate(all="ignore"):
        a0 = x2 * m[0] + (y2 * m[3] + m[6])
        a1 = x2 * m[1] + (y2 * m[4] + m[7])
        a2 = x2 * m[2] + (y2 * m[5] + m[8])
        b0 = x1 * m[0] + (y1 * m[1] + m[2])
        b1 = x1 * m[3] + (y1 * m[4] + m[5])
        r = x1 * a0 + (y1 * a1 + a2)
        jj = a0 * a0 + (a1 * a1 + (b0 * b0 + b1 * b1))
        rc = (1.0 / jj.astype(np.float64)).astype(f)
        t = f(1.5) * f(thr)
        ith = f(1.0) / (t * t)
        x = ((r * r) * rc) * ith
        c = np.clip(f(1.0) - x, f(0), f(1))
        c = np.where(np.isnan(c), f(0), c).astype(f)
    bad = ~np.isfinite(md).all(-1) | (md == 0).all(-1)
    c[bad] = 0
    scores = c.sum(-1, dtype=f)
    scores[bad] = np.nan
    masks = (c > 0).astype(np.uint8)
    if valid is not None:
        v = valid.numpy().astype(bool)
        scores[~v] = 0
        masks[~v] = 0
    return torch.from_numpy(scores), torch.from_numpy(masks)


# --------------------------------------------------------------------------------------------- sentinel buffers
def new_buffers(P, M, N, dtype, device, mask_offset=0, want_masks=True, zero_scores=False):
    """(mask buffer | None, mask start, score buffer, score start in elements): the outputs are slices of larger buffers, masks behind
    MASK_GUARD + mask_offset bytes of guard and followed by >= MASK_GUARD more, scores between SCORE_GUARD bytes on either side."""
    mb = None
    if want_masks:
        mb = torch.full((MASK_GUARD + mask_offset + P * M * N + MASK_GUARD + 16,), MASK_SENTINEL, dtype=torch.uint8, device=device)
        assert mb.data_ptr() % 16 == 0
    g = SCORE_GUARD // (4 if dtype == torch.float32 else 8)
    sb = torch.full((2 * g + P * M,), SCORE_SENTINEL, dtype=dtype, device=device)
    if zero_scores:
        sb[g:g + P * M] = 0
    return mb, MASK_GUARD + mask_offset, sb, g


def call_with_sentinels(matches, models, thr, valid=None, want_masks=True, mask_offset=0, gate=None):
    """dr_msac_score through the ctypes binding ops.msac_score uses, on sentinel-filled guarded buffers.  matches [P,N,4], models
    [P,M,3,3], thr [P] (device tensors); gate = (iters int32 [P], max_iters f64 [P]) or None -> (mask buffer, start, score buffer, start)"""
    from differentiable_ransac_amd import _lib as L
    P, N, _ = matches.shape
    M = models.shape[1]
    mb, m0, sb, s0 = new_buffers(P, M, N, matches.dtype, matches.device, mask_offset, want_masks)
    masks = mb[m0:m0 + P * M * N] if want_masks else None
    scores = sb[s0:s0 + P * M]
    v = None if valid is None else valid.contiguous().view(torch.uint8)
    args = [L.ptr(matches.contiguous()), L.ptr(models.contiguous()), L.ptr(v), L.ptr(thr.contiguous()), L.c_int(P), L.c_int(M),
            L.c_int(N), L.ptr(scores), L.ptr(masks)]
    if matches.dtype == torch.float32:
        args += [L.ptr(None), L.ptr(None)] if gate is None else [L.ptr(gate[0]), L.ptr(gate[1])]
    L.call(f"dr_msac_score_{L.suffix(matches.dtype)}", *args, L.stream())
    return mb, m0, sb, s0


def call_rigid_with_sentinels(pts, models, threshold, accumulate=False):
    """dr_rigid_residual on guarded buffers; accumulate (f32): the sums are handed in as zeros and added to"""
    from differentiable_ransac_amd import _lib as L
    P, N, _ = pts.shape
    M = models.shape[1]
    mb, m0, sb, s0 = new_buffers(P, M, N, pts.dtype, pts.device, zero_scores=accumulate)
    args = [L.ptr(pts.contiguous()), L.ptr(models.contiguous()), L.scalar(pts.dtype, float(threshold)), L.c_int(P), L.c_int(M),
            L.c_int(N), L.ptr(sb[s0:s0 + P * M]), L.ptr(mb[m0:m0 + P * M * N])]
    if pts.dtype == torch.float32:
        args.append(L.c_int(1 if accumulate else 0))
    L.call(f"dr_rigid_residual_{L.suffix(pts.dtype)}", *args, L.stream())
    return mb, m0, sb, s0


# --------------------------------------------------------------------------------------------- the comparison
def _sentinel_scores(t):
    return t == torch.tensor(SCORE_SENTINEL, dtype=t.dtype, device=t.device)


def compare(mb, m0, sb, s0, exp, P, valid=None, gated=None, stats=None):
    """The mask, score, sentinel and guard rules on the buffers of one call (any device).  exp: stack_refs() of the S distinct
    sets, pair p is set p % S; valid [P,M] bool | None; gated [P] bool | None (pairs whose rows and scores must still be
    sentinel).  mb None: scores only.  Raises AssertionError; returns / fills `stats` with the excluded shares and the worst
    score error / tolerance."""
    dev = sb.device
    S, M, N = exp["masks"].shape
    sel = torch.arange(P, device=dev) % S
    e = {k: v.to(dev) for k, v in exp.items()}
    live = torch.ones(P, M, dtype=torch.bool, device=dev) if valid is None else valid.to(dev).bool().clone()
    open_ = torch.ones(P, dtype=torch.bool, device=dev) if gated is None else ~gated.to(dev)
    nan = e["nan"][sel] & live
    ev = live & ~nan                                     # the rows that are evaluated
    scores = sb[s0:s0 + P * M].view(P, M)
    assert _sentinel_scores(sb[:s0]).all() and _sentinel_scores(sb[s0 + P * M:]).all(), "score guard overwritten"
    assert _sentinel_scores(scores[~open_]).all(), "score of a gated pair written"
    so = scores[open_]
    assert not _sentinel_scores(so).any(), "score left unwritten"
    assert (so[~live[open_]] == 0).all(), "invalid slot: score not exactly 0"
    assert torch.isnan(so[nan[open_]]).all(), "non-finite or all-zero model: score not NaN"
    ref, tol = e["scores"][sel][open_], e["tol"][sel][open_]
    evo = ev[open_]
    err = (so.double() - ref).abs()
    ratio = torch.where(evo, err / tol.clamp(min=1e-300), torch.zeros_like(err))
    ratio = torch.where(evo & (tol == 0) & (err == 0), torch.zeros_like(ratio), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    out = dict(score_ratio=worst, excl_bytes=0.0, excl_inliers=0.0)
    assert not torch.isnan(so[evo]).any() and worst <= 1.0, f"score rule: worst |error| / tolerance = {worst}"
    if mb is not None:
        masks = mb[m0:m0 + P * M * N].view(P, M, N)
        assert (mb[:m0] == MASK_SENTINEL).all() and (mb[m0 + P * M * N:] == MASK_SENTINEL).all(), "mask guard overwritten"
        assert (masks[~open_] == MASK_SENTINEL).all(), "mask row of a gated pair written"
        mo = masks[open_]
        assert (mo <= 1).all(), f"mask bytes other than 0 / 1: {mo[mo > 1][:8].tolist()}"
        want = e["masks"][sel][open_] & evo[..., None]
        excl = e["excl"][sel][open_] & evo[..., None]
        diff = (mo != want.to(torch.uint8)) & ~excl
        nbad = int(diff.sum())
        assert nbad == 0, f"{nbad} mask bytes differ outside |d2 - thr2| <= 2 bound; first at {diff.nonzero()[0].tolist()}"
        n_excl, n_in, n_bytes = int(excl.sum()), int(want.sum()), want.numel()
        out["excl_bytes"] = n_excl / max(n_bytes, 1)
        out["excl_inliers"] = n_excl / n_in if n_in else (0.0 if n_excl == 0 else float("inf"))
        assert n_excl <= CAP_BYTES * n_bytes, f"excluded bytes {n_excl} of {n_bytes}: above the cap of {CAP_BYTES}"
        assert n_excl <= CAP_INLIERS * n_in, f"excluded bytes {n_excl} against {n_in} reference inliers: above the cap of {CAP_INLIERS}"
    if stats is not None:
        for k, v in out.items():
            stats[k] = max(stats.get(k, 0.0), v)
    return out


def fill_outputs(mb, m0, sb, s0, scores, masks):
    """write a (host-made) result into guarded buffers, as a kernel would"""
    sb[s0:s0 + scores.numel()] = scores.reshape(-1).to(sb.dtype)
    if mb is not None:
        mb[m0:m0 + masks.numel()] = masks.reshape(-1).to(torch.uint8)


# --------------------------------------------------------------------------------------------- the cases of the GPU tests
SPECIALS = ((0, "nan"), (15, "inf"), (7, "zero"), (16, "m0"), (40, "inf"), (63, "nan"), (64, "zero"), (69, "m0"))   # first / last / middle slots of 16- and 64-slot tiles
GROUP_MMAX = {"short": 33, "f16s": 65, "f16l": 256, "f16x": 128, "f8": 65, "f64": 33, "patterns": 70, "props": 70}


TINY_SEED, TINY_M = 2004, 17   # chosen below the cap: see _case


def _case(group, P, M, N, dtype=torch.float32, offset=0, pattern=None, special=False, thr=THR, want_masks=True):
    # the tiny threshold lies below what f32 resolves (the second-order term of the bound alone is ~1e-13 against thr2 = 2e-18), so a
    # point within 3e-7 of an epipolar line is an excluded byte against no inlier at all: its seed is one without such a point
    return dict(group=group, P=P, M=M, N=N, dtype=dtype, offset=offset, pattern=pattern, special=special, thr=thr,
                want_masks=want_masks, seed=TINY_SEED if thr == THR_TINY else 1000 + N,
                mmax=M if thr == THR_TINY else max(GROUP_MMAX[group], M))


def gpu_cases():
    """every (shape, mask offset, validity pattern, special models, threshold) the GPU tests run, so that the host test can hold the
    reference alone to the cap on exactly these inputs"""
    pats = (None,) + VALID_PATTERNS
    out, i = [], 0

    def add(*a, **k):
        nonlocal i
        k.setdefault("pattern", pats[i % len(pats)])
        k.setdefault("special", i % 2 == 1)
        out.append(_case(*a, **k))
        i += 1
    for n in SHORT_N:
        for m in SHORT_M:
            add("short", 3, m, n)
        for off in (1, 2):
            for m in (17, 33):
                add("short", 3, m, n, offset=off)
    for p in F16S_P:
        for n in F16S_N:
            for m in F16S_M:
                add("f16s", p, m, n, offset=16 * (i % 2))
    for p, m, n in F16L:
        add("f16l", p, m, n)
    for (p, m, n), pat in zip((F16L_ATOMIC, F16L_RELOAD, F16S_CHUNKS), (None, "all_but_one", "alternating")):   # (each walk with rows to evaluate)
        add("f16x", p, m, n, pattern=pat)
    for n in F8_N:
        for m in F8_M:
            add("f8", 3, m, n)
            add("f8", 3, m, n, offset=1)
    for n in F8_N16:
        for m in F8_M:
            add("f8", 3, m, n, offset=8)
    for n in F64_N:
        for m in F64_M:
            add("f64", 3, m, n, dtype=torch.float64)
            add("f64", 3, m, n, dtype=torch.float64, want_masks=False)
    for p, m, n, off in ((3, 70, 272, 0), (512, 70, 272, 0), (3, 70, 257, 0), (3, 33, 255, 0)):
        for pat in pats:
            add("patterns", p, m, n, offset=off, pattern=pat, special=True)
    for p, m, n in ((3, 65, 272), (512, 65, 272), (3, 65, 2064)):
        add("props", p, m, n, thr=THR_HUGE, pattern=None, special=False)
        if n == 272:
            add("props", p, TINY_M, n, thr=THR_TINY, pattern=None, special=False)
    return out


_SETS = {}


def case_inputs(c):
    """-> (matches [S,N,4], models [S,M,3,3], valid [P,M] | None, per-set references cut to the case's M)"""
    S = min(c["P"], 4)
    key = (S, c["mmax"], c["N"], c["seed"], c["dtype"], c["special"], c["thr"])
    if key not in _SETS:
        mt, md = two_view_sets(S, c["mmax"], c["N"], c["seed"], c["dtype"], SPECIALS if c["special"] else ())
        thr = c["thr"] if c["dtype"] == torch.float64 else float(torch.tensor(c["thr"], dtype=torch.float32))
        keep = ("masks", "excl", "scores", "score_slack", "nan", "thr2")     # (the [M,N] intermediates are not kept: dozens of cases)
        _SETS[key] = (mt, md, [{k: v for k, v in sampson_ref(mt[s], md[s], thr, unit(c["dtype"])).items() if k in keep}
                               for s in range(S)])
    mt, md, refs = _SETS[key]
    M = c["M"]
    refs = [{k: (v[:M] if torch.is_tensor(v) else v) for k, v in r.items()} for r in refs]
    valid = None if c["pattern"] is None else valid_pattern(c["pattern"], c["P"], M)
    return mt, md[:, :M].contiguous(), valid, refs


def reference_cap(refs, P, valid):
    """(excluded bytes, reference inliers, bytes) of a case from the reference alone, as compare() counts them"""
    S = len(refs)
    ex = torch.stack([r["excl"].sum(-1) for r in refs])[torch.arange(P) % S]
    inl = torch.stack([r["masks"].sum(-1) for r in refs])[torch.arange(P) % S]
    live = ~torch.stack([r["nan"] for r in refs])[torch.arange(P) % S]
    if valid is not None:
        live = live & valid
    return int((ex * live).sum()), int((inl * live).sum()), P * refs[0]["masks"].numel()

