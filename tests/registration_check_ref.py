"""f64 numpy oracle of the rigidity test in front of the registration fit (dr_kabsch_gather_checked,
ransac.BatchedRegistration(edge_similarity=...)), written from the rule and not from the kernel's code, and the inputs its tests share.

A rigid motion keeps distances, so a sample {(p_i, q_i)} of inliers has |p_i - p_j| ~ |q_i - q_j| for every pair of its rows.  For every
pair i < j of the k rows: a2 = sum_d (p_i[d] - p_j[d])^2, b2 = sum_d (q_i[d] - q_j[d])^2, and with sigma = edge_similarity^2 the edge
passes iff a2 >= sigma b2 and b2 >= sigma a2 (Open3D's CorrespondenceCheckerBasedOnEdgeLength, on squares).  A NaN fails the edge, two
coincident rows pass it.  A sample passes iff every edge does; a sample with an index outside [0, N) is not tested at all.

The margin of a sample is min over its edges of min(|a2 - sigma b2|, |b2 - sigma a2|) / max(a2, b2, tiny): how far, relative to the
edge's own size, the nearer of the two comparisons is from turning.  The kernel takes the decision in f64 on the same stored values, so
it can differ from this oracle only through the order and fusing of the three-term sums: a few f64 roundings, 1e-16 relative.  Samples
with a margin below LEFT_OUT (1e-9 for f64 tensors; 1e-5 for f32 tensors, whose values are widened to f64 before anything is computed) are
left out of a comparison of decisions."""
import numpy as np
import torch

LEFT_OUT = {"float32": 1e-5, "float64": 1e-9}
TINY = float(np.finfo(np.float64).tiny)

# the shapes and seeds the GPU test runs and the host test checks the left-out cap on
P, N = 2, 300
OUTLIER_RATE = 0.7
CASES = [(130, 3), (130, 4), (700, 3)]            # (B, k)
SIMILARITIES = [0.0, 0.9, 1.0]
DTYPES = {"float32": torch.float32, "float64": torch.float64}
LEFT_OUT_CAP = 0.01


def check(matches, idx, edge_similarity):
    """matches [N,6] (any float type; widened to f64), idx [B,k] -> (passed [B] bool, margin [B], in_range [B] bool); passed is False
    and the margin inf for a sample that is not in range; a NaN edge fails with margin inf (no rounding turns it)"""
    m = np.asarray(matches, np.float64)
    idx = np.asarray(idx)
    n, k = len(m), idx.shape[1]
    sigma = float(edge_similarity) ** 2
    in_range = ((idx >= 0) & (idx < n)).all(1)
    rows = m[np.where(in_range[:, None], idx, 0)]                 # [B,k,6]
    i, j = np.triu_indices(k, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        dp, dq = rows[:, i, :3] - rows[:, j, :3], rows[:, i, 3:] - rows[:, j, 3:]
        a2, b2 = (dp * dp).sum(-1), (dq * dq).sum(-1)             # [B,E]
        ok = (a2 >= sigma * b2) & (b2 >= sigma * a2)
        gap = np.minimum(np.abs(a2 - sigma * b2), np.abs(b2 - sigma * a2)) / np.maximum(np.maximum(a2, b2), TINY)
    gap = np.where(np.isnan(gap), np.inf, gap)
    return ok.all(1) & in_range, np.where(in_range, gap.min(1), np.inf), in_range


def scenes(dtype_name):
    """-> (matches [P,N,6], logits [P,N]) of dtype: synth.rigid_pair at OUTLIER_RATE, seeds 40, 41"""
    from differentiable_ransac_amd import synth
    sc = [synth.rigid_pair(40 + p, N, 1.0 - OUTLIER_RATE, dtype=DTYPES[dtype_name]) for p in range(P)]
    return torch.stack([s["matches"] for s in sc]), torch.stack([s["logits"] for s in sc])


def noise(B, dtype_name):
    """explicit sampler noise [P,B,N].  The seed is chosen on this oracle alone: the two hand-made repeated rows use up 2 of the 2.6
    samples the cap allows at B = 130, and at edge_similarity = 1 an all-inlier sample of f32 values falls below 1e-5 about once in
    500 samples (seeds 7000 and 7100 leave out 3 and 4 of 260, this one at most 2; tests/test_registration_check_host.py asserts it)"""
    from differentiable_ransac_amd import synth
    return synth.gumbel_noise((P, B, N), seed=7200 + B, dtype=DTYPES[dtype_name])


def hand_made(idx):
    """two samples per pair written by hand, in place: sample 3 gets an index out of range (N, then -1 in the second pair), sample 70
    repeats its first row"""
    idx = idx.clone()
    idx[0, 3, 1], idx[1, 3, 0] = N, -1
    idx[:, 70, 1] = idx[:, 70, 0]
    return idx


def host_index_sets(logits, g, k):
    """what ops.gumbel_topk(logits, B, k, 1.0, g, ...) gives on explicit noise: the k largest of logits + g per hypothesis, ascending"""
    return hand_made(torch.topk(logits[:, None, :] + g, k, dim=-1).indices.sort(-1).values.to(torch.int32))
