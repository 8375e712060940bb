"""The rigidity test in front of the registration fit without a GPU: the properties of the oracle tests/registration_check_ref.py, the
share of samples it leaves out on the inputs of the GPU test, the ABI of dr_kabsch_gather_checked (declared, exported, DR_EINVAL before
any device work) and the argument checks of ops.kabsch_gather_checked and BatchedRegistration(edge_similarity=)."""
import ctypes

import numpy as np
import pytest
import torch

from differentiable_ransac_amd import _lib as L
from tests import registration_check_ref as C
from tests import registration_ref as R

SYMBOLS = ["dr_kabsch_gather_checked_f32", "dr_kabsch_gather_checked_f64"]


def _triplets(n, count, k, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n)[:k] for _ in range(count)])


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("k", [3, 4, 8])
def test_similarity_zero_passes_every_finite_sample(k):
    m = R.scene(1, 200, 0.3)["matches"]
    passed, margin, in_range = C.check(m, _triplets(200, 500, k, 2), 0.0)
    assert passed.all() and in_range.all() and (margin > 0).all()


@pytest.mark.parametrize("k", [3, 4, 8])
def test_rigidly_moved_clean_cloud_passes_every_sample(k):
    m = R.scene(3, 200, 1.0, noise=0.0)["matches"]
    passed, margin, _ = C.check(m, _triplets(200, 500, k, 4), 0.999)
    print(f"k={k}: smallest margin {margin.min():.3g}")
    assert passed.all()
    # and an inlier sample with noise far below the edge lengths still does at 0.9
    noisy = R.scene(3, 200, 1.0, noise=1e-4)["matches"]
    assert C.check(noisy, _triplets(200, 500, k, 4), 0.9)[0].all()


def test_a_far_outlier_row_fails_the_sample():
    m = R.scene(5, 50, 1.0, noise=0.0)["matches"].copy()
    m[7, 3:] += 100.0
    idx = np.array([[1, 2, 3], [1, 7, 3], [7, 8, 9], [4, 5, 6]])
    passed, _, _ = C.check(m, idx, 0.9)
    assert passed.tolist() == [True, False, False, True]
    # the rule is symmetric: the outlier on the p side fails it too
    m2 = R.scene(5, 50, 1.0, noise=0.0)["matches"].copy()
    m2[7, :3] += 100.0
    assert C.check(m2, idx, 0.9)[0].tolist() == [True, False, False, True]


def test_a_nan_row_fails_and_an_index_out_of_range_is_not_tested():
    m = R.scene(6, 50, 1.0, noise=0.0)["matches"].copy()
    m[4, 1] = np.nan
    idx = np.array([[1, 2, 3], [1, 4, 3], [0, 50, 2], [0, -1, 2]])
    for sim in (0.0, 0.9, 1.0):
        passed, margin, in_range = C.check(m, idx, sim)
        assert passed[0] == (sim < 1.0) and not passed[1:].any(), sim
        assert in_range.tolist() == [True, True, False, False]
        assert np.isfinite(margin[:2]).all() and np.isinf(margin[2:]).all()      # (the NaN sample: its margin is its finite edge's)


def test_coincident_rows_pass_the_check():
    m = R.scene(7, 50, 1.0, noise=0.0)["matches"]
    for sim in (0.0, 0.9):
        for rows in ([2, 2, 2], [2, 2, 5], [5, 2, 2, 5]):
            assert C.check(m, np.array([rows]), sim)[0][0], (sim, rows)
    # at 1.0 an edge passes iff a2 == b2: the zero edges do, exactly
    passed, margin, _ = C.check(m, np.array([[2, 2, 2]]), 1.0)
    assert passed[0] and margin[0] == 0.0


def test_margin_is_the_relative_distance_to_the_nearer_comparison():
    m = np.zeros((2, 6))
    m[1, :3] = [2.0, 0.0, 0.0]          # a2 = 4
    m[1, 3:] = [0.0, 3.0, 0.0]          # b2 = 9
    passed, margin, _ = C.check(m, np.array([[0, 1, 1]]), 0.5)       # sigma = 0.25: 4 >= 2.25, 9 >= 1; the edge (1, 1) is 0 / 0
    assert passed[0] and margin[0] == 0.0
    a2, b2, s = 4.0, 9.0, 0.25
    passed, margin, _ = C.check(np.concatenate([m, m[1:] * 2.0]), np.array([[0, 1, 2]]), 0.5)
    want = min(min(abs(x - s * y), abs(y - s * x)) / max(x, y) for x, y in ((a2, b2), (4 * a2, 4 * b2), (a2, b2)))
    assert passed[0] and margin[0] == pytest.approx(want, rel=1e-15)
    assert not C.check(m, np.array([[0, 1, 1]]), 0.7)[0][0]          # sigma = 0.49: 4 < 4.41


# ------------------------------------------------------------------------------------------------ the GPU test's inputs
@pytest.mark.parametrize("name", ["float32", "float64"])
@pytest.mark.parametrize("B,k", C.CASES)
def test_oracle_leaves_out_few_samples_of_the_gpu_cases(name, B, k):
    """the cap tests/test_gpu_registration_check.py asserts, on the same scenes, noise and hand-made samples: at most 1 % of the samples
    have a margin below LEFT_OUT (the hand-made repeated rows are among them at 0 and 1.0: their zero edge has margin 0)"""
    m, logits = C.scenes(name)
    idx = C.host_index_sets(logits, C.noise(B, name), k)
    for sim in C.SIMILARITIES:
        left, rejected, total = 0, 0, 0
        for p in range(C.P):
            passed, margin, in_range = C.check(m[p].double().numpy(), idx[p].numpy(), sim)
            left += int((margin < C.LEFT_OUT[name]).sum())
            rejected += int((~passed & in_range).sum())
            total += len(passed)
        print(f"{name} B={B} k={k} similarity {sim}: left out {left}/{total}, rejected {rejected}")
        assert left <= C.LEFT_OUT_CAP * total
        if sim == 0.9:      # both kinds of sample, in numbers that fill and empty waves
            assert 0.2 * total < rejected < 0.98 * total


# ------------------------------------------------------------------------------------------------ library, wrapper and driver
def test_header_declares_and_library_exports_the_entries():
    declared = set(L.entries()) | {"dr_version", "dr_last_error"}
    assert not [s for s in SYMBOLS if s not in declared]
    lib = L.lib()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    assert lib.dr_version() == 1


def test_entries_refuse_bad_arguments_without_a_gpu():
    lib = L.lib()
    buf = (ctypes.c_char * 256)()
    for sfx in ("f32", "f64"):
        fn = getattr(lib, "dr_kabsch_gather_checked_" + sfx)

        def call(matches=buf, idx=buf, P=1, B=1, N=3, k=3, sim=0.9, models=buf, valid=buf, rejected=None):
            return fn(matches, idx, P, B, N, k, ctypes.c_double(sim), models, valid, rejected, None)

        for name in ("matches", "idx", "models", "valid"):
            assert call(**{name: None}) == -1 and b"null" in lib.dr_last_error(), name
        for kw in (dict(P=0), dict(B=0), dict(N=0), dict(k=2), dict(k=9), dict(P=1 << 16, B=1 << 15)):
            assert call(**kw) == -1 and b"dr_kabsch_gather_checked" in lib.dr_last_error(), kw
        for sim in (-0.1, 1.0001, float("nan"), float("inf")):
            assert call(sim=sim) == -1 and b"edge_similarity" in lib.dr_last_error(), sim


def test_wrapper_checks_its_arguments_before_any_launch(monkeypatch):
    from differentiable_ransac_amd import ops
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    m, idx = torch.rand(2, 16, 6), torch.zeros(2, 5, 3, dtype=torch.int32)
    for sim in (-0.5, 1.5, float("nan")):
        with pytest.raises(L.DransacError, match="edge_similarity"):
            ops.kabsch_gather_checked(m, idx, sim)
    for bad_m, bad_i in ((torch.rand(2, 16, 4), idx), (torch.rand(16, 6), idx), (m, idx.long()), (m, idx[0])):
        with pytest.raises(L.DransacError, match="kabsch_gather_checked"):
            ops.kabsch_gather_checked(bad_m, bad_i, 0.9)
    for bad_r in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(L.DransacError, match="rejected"):
            ops.kabsch_gather_checked(m, idx, 0.9, bad_r)
    with pytest.raises(L.DransacError, match="GPU tensors"):          # the checks passed: the CPU tensors are what is refused
        ops.kabsch_gather_checked(m, idx, 0.9, torch.zeros(2, dtype=torch.int32))
    assert calls == []


def test_constructor_checks():
    from differentiable_ransac_amd.ransac import BatchedRegistration
    assert BatchedRegistration().edge_similarity is None
    assert BatchedRegistration(edge_similarity=0.9).edge_similarity == 0.9
    assert BatchedRegistration(edge_similarity=1, lo=2).edge_similarity == 1.0
    assert BatchedRegistration(edge_similarity=0.5, scoring="magsac").scoring == "magsac"
    for bad in (0, 0.0, -0.1, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="edge_similarity"):
            BatchedRegistration(edge_similarity=bad)
    with pytest.raises(ValueError, match="training signal"):
        BatchedRegistration(edge_similarity=0.9, train=True)
    assert BatchedRegistration(train=True).train
