"""numpy statement of the PROSAC sampler -- test infrastructure, independent of the kernel: the growth table from its
definition, the ranking by a stable sort, and one Python loop per sample that keeps its ranks in a set."""
import math

import numpy as np

from .philox_ref import philox4x32


def growth_table(N: int, k: int, T_N: int) -> np.ndarray:
    """int64 [N - k + 1]: entry i is T'_{k+i};  T_n = T_N prod_{i<k} (n - i) / (N - i),  T'_k = 1,
    T'_n = T'_{n-1} + ceil(T_n - T_{n-1})"""
    def T(n):
        v = np.float64(T_N)
        for i in range(k):
            v = v * (np.float64(n - i) / np.float64(N - i))
        return v
    out, prev = [1], T(k)
    for n in range(k + 1, N + 1):
        cur = T(n)
        out.append(out[-1] + int(math.ceil(cur - prev)))
        prev = cur
    return np.asarray(out, dtype=np.int64)


def subset_size(table: np.ndarray, k: int, t: int) -> int:
    """n(t) = min{ n in [k, N] : T'_n >= t }; only meaningful in the growth regime, t <= T'_N"""
    if t > int(table[-1]):
        raise ValueError("t lies behind the growth regime")
    return k + int(np.searchsorted(table, t, side="left"))


def rank(logits: np.ndarray) -> np.ndarray:
    """order [P,N]: descending logit, ties (and -0.0 / 0.0) by ascending index, NaN last"""
    out = []
    for row in np.asarray(logits):
        key = [(-math.inf if math.isnan(v) else float(v)) for v in row.tolist()]
        out.append(sorted(range(len(key)), key=lambda i: -key[i]))      # (sorted is stable; -(-inf) = inf sorts last)
    return np.asarray(out, dtype=np.int64)


def _words(seed: int, b: int, p: int, c: int):
    w = []
    for blk in range((c + 3) // 4):
        w += [int(x) for x in philox4x32(seed, np.uint32(blk), np.uint32(b), np.uint32(p), np.uint32(3))]
    return w[:c]


def floyd(words, pool: int) -> set:
    """len(words) distinct ranks out of [0, pool - 1]"""
    c, chosen = len(words), set()
    for i, word in enumerate(words):
        j = pool - c + i
        r = (word * (j + 1)) >> 32
        chosen.add(j if r in chosen else r)
    assert len(chosen) == c
    return chosen


def sample_ranks(table: np.ndarray, seed: int, t0: int, p: int, b: int, N: int, k: int) -> set:
    """the ranks of draw t = t0 + b + 1 of pair p"""
    t = t0 + b + 1
    if t <= int(table[-1]):
        n = subset_size(table, k, t)
        return floyd(_words(seed, b, p, k - 1), n - 1) | {n - 1}
    return floyd(_words(seed, b, p, k), N)


def sample(order, table: np.ndarray, seed: int, t0: int, P: int, B: int, N: int, k: int) -> np.ndarray:
    """idx [P,B,k], ascending in the point index; order [P,N] or None (the identity)"""
    out = np.zeros((P, B, k), dtype=np.int64)
    for p in range(P):
        for b in range(B):
            ranks = sample_ranks(table, seed, t0, p, b, N, k)
            out[p, b] = sorted(ranks if order is None else [int(order[p][r]) for r in ranks])
    return out
