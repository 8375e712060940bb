"""PROSAC sampling, host side: the growth table of ops.prosac_growth against its definition and its pinned values, the properties
and the uniformity of the numpy reference (tests/prosac_ref.py), the drivers' constructors, and the C entry's argument checks.
No GPU is touched."""
import ctypes
import itertools
from collections import Counter

import numpy as np
import pytest
import torch

from tests import prosac_ref as PR

CONFIGS = [(37, 3, 50), (9, 8, 20), (5, 5, 10), (12, 3, 3000), (2000, 5, 200000), (50000, 3, 200000)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_growth_table_equals_the_reference(cfg):
    from differentiable_ransac_amd import ops
    N, k, T_N = cfg
    got = ops.prosac_growth(N, k, T_N, torch.device("cpu"))
    assert got.dtype == torch.int64 and got.shape == (N - k + 1,)
    assert np.array_equal(got.numpy(), PR.growth_table(N, k, T_N))


def test_growth_table_pinned_values():
    from differentiable_ransac_amd import ops

    def table(N, k, T_N):
        return ops.prosac_growth(N, k, T_N, torch.device("cpu")).tolist()

    def n_of(tb, k, t):
        return PR.subset_size(np.asarray(tb, np.int64), k, t)
    t = table(37, 3, 50)
    assert t[:6] == [1, 2, 3, 4, 5, 6] and t[-1] == 70
    assert table(9, 8, 20) == [1, 19]
    assert table(5, 5, 10) == [1]
    assert table(12, 3, 3000) == [1, 42, 124, 261, 466, 753, 1135, 1626, 2240, 2990]
    t = table(2000, 5, 200000)
    assert t[-1] == 201143 and n_of(t, 5, 1024) == 623 and n_of(t, 5, 5120) == 939
    t = table(50000, 3, 200000)
    assert t[-1] == 227825 and n_of(t, 3, 5120) == 5122


def test_growth_table_arguments():
    from differentiable_ransac_amd import ops
    for bad in [(2, 3, 10), (5, 0, 10), (5, 3, 0)]:
        with pytest.raises(ValueError):
            ops.prosac_growth(*bad, torch.device("cpu"))


@pytest.mark.parametrize("cfg", [(37, 3, 50), (9, 8, 20), (5, 5, 10), (12, 3, 3000), (37, 5, 50), (3, 3, 10)],
                         ids=lambda c: "-".join(map(str, c)))
def test_reference_properties(cfg):
    N, k, T_N = cfg
    tb = PR.growth_table(N, k, T_N)
    assert tb[0] == 1 and (np.diff(tb) > 0).all()
    assert PR.subset_size(tb, k, 1) == k
    last = int(tb[-1])
    for t in range(1, last + 1):
        assert PR.subset_size(tb, k, t) <= k + t - 1
    # every draw of the growth regime and 40 of the tail, two pairs
    for p in range(2):
        for t in range(1, last + 41):
            ranks = PR.sample_ranks(tb, 0xF00DFACE12345678, 0, p, t - 1, N, k)
            assert len(ranks) == k and min(ranks) >= 0 and max(ranks) < N
            if t <= last:
                n = PR.subset_size(tb, k, t)
                assert max(ranks) == n - 1
    assert PR.sample_ranks(tb, 5, 0, 0, 0, N, k) == set(range(k))


def _chi2(counts, cells, total):
    e = total / cells
    return sum((v - e) ** 2 / e for v in counts.values()) + (cells - len(counts)) * e


def test_floyd_is_uniform_in_the_tail():
    """N=6, k=3: 20 subsets, 20000 draws behind the growth regime; 0.999 quantile of chi-square with 19 dof"""
    tb = PR.growth_table(6, 3, 4)
    idx = PR.sample(None, tb, 12345, int(tb[-1]), 1, 20000, 6, 3)[0]
    counts = Counter(map(tuple, idx.tolist()))
    assert set(counts) == set(itertools.combinations(range(6), 3))
    x2 = _chi2(counts, 20, 20000)
    print(f"tail chi-square {x2:.2f}")
    assert x2 <= 43.8


def test_floyd_is_uniform_in_the_growth_regime():
    """N=12, k=3, T_N=3000: the 382 draws with n(t) = 9 hold rank 8 and a uniform pair of the ranks below it (28 pairs);
    0.999 quantile of chi-square with 27 dof"""
    tb = PR.growth_table(12, 3, 3000)
    t0, t1 = int(tb[8 - 3]), int(tb[9 - 3])
    assert t1 - t0 == 382
    assert PR.subset_size(tb, 3, t0 + 1) == 9 and PR.subset_size(tb, 3, t1) == 9 and PR.subset_size(tb, 3, t0) == 8
    idx = PR.sample(None, tb, 777, t0, 1, t1 - t0, 12, 3)[0]
    assert (idx[:, 2] == 8).all()
    counts = Counter(map(tuple, idx[:, :2].tolist()))
    assert set(counts) == set(itertools.combinations(range(8), 2))
    x2 = _chi2(counts, 28, t1 - t0)
    print(f"growth chi-square {x2:.2f}")
    assert x2 <= 55.5


def test_rank_reference():
    lg = np.array([[0.5, np.nan, 2.0, 0.5, -np.inf, np.inf, -0.0, 0.0, 2.0]])
    assert PR.rank(lg)[0].tolist() == [5, 2, 8, 0, 3, 6, 7, 1, 4]


def test_constructors_and_refusals():
    from differentiable_ransac_amd.ransac import BatchedRANSAC, BatchedRegistration
    reg = BatchedRegistration(sampling="prosac")
    assert reg.sampling == "prosac" and reg.prosac_draws == 200000
    assert BatchedRegistration().sampling == "gumbel"
    assert BatchedRegistration(sampling="prosac", prosac_draws=5, edge_similarity=0.9, scoring="magsac").prosac_draws == 5
    assert BatchedRegistration(sampling="prosac", lo=2).lo == 2
    two = BatchedRANSAC("nister", sampling="prosac", prosac_draws=1000)
    assert two.sampling == "prosac" and two.prosac_draws == 1000
    assert two.plan(4) == [1, 1, 1, 1]
    for cls in (BatchedRegistration, BatchedRANSAC):
        with pytest.raises(ValueError):
            cls(sampling="nope")
        with pytest.raises(ValueError):
            cls(sampling="prosac", train=True)
        for bad in (0, -3, 2.5, "many", None, True):
            with pytest.raises(ValueError):
                cls(sampling="prosac", prosac_draws=bad)
    with pytest.raises(ValueError):
        BatchedRANSAC("f8", sampling="prosac", weighted=1)
    # explicit noise is refused before anything is launched
    m3, m2, lg = torch.zeros(1, 8, 6), torch.zeros(1, 8, 4), torch.zeros(1, 8)
    with pytest.raises(ValueError):
        reg(m3, lg, gumbels=[torch.zeros(1, 4, 8)])
    with pytest.raises(ValueError):
        two(m2, lg, gumbels=[torch.zeros(1, 4, 8)])


def test_entry_is_exported_and_checks_its_arguments_without_touching_the_gpu():
    from differentiable_ransac_amd import _lib as L
    lib = L.lib()
    fn = lib.dr_prosac_sample
    u64, i64, i32, vp = ctypes.c_uint64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    fake = vp(64)      # never dereferenced: every call below is refused before a launch

    def call(order=None, growth=fake, t0=0, P=1, B=1, N=5, k=3, idx=fake):
        return fn(order, growth, u64(1), None, i64(t0), i32(P), i32(B), i32(N), i32(k), idx, None)
    assert call(idx=None) == -1
    assert b"null" in lib.dr_last_error()
    assert call(growth=None) == -1
    for kw in (dict(k=0), dict(k=9, N=20), dict(N=2), dict(P=0), dict(B=0), dict(t0=-1)):
        assert call(**kw) == -1, kw
        assert b"dr_prosac_sample" in lib.dr_last_error()
