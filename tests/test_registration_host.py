"""Host-side checks of the robust 3-D registration path: the f64 oracle tests/registration_ref.py against the maths it states (so
that the GPU tests compare the kernels with something that is itself pinned), the C header and the built library, and the
argument checks of ransac.BatchedRegistration.  No GPU."""
import math

import numpy as np
import pytest

from differentiable_ransac_amd import _lib as L
from tests import registration_ref as R

SYMBOLS = [f"dr_{n}_{s}" for n in ("kabsch_gather", "rigid_msac_score", "registration_update", "refit_rigid") for s in ("f32", "f64")]


def test_oracle_kabsch_recovers_the_generating_pose():
    for seed in range(5):
        sc = R.scene(seed, 40, 1.0, noise=0.0)
        m = sc["matches"]
        assert 1.0 <= np.linalg.norm(sc["t"]) <= 2.0 and abs(np.linalg.det(sc["R"]) - 1.0) < 1e-12
        for rows in (slice(0, 3), slice(0, 8), slice(None)):
            o = R.kabsch(m[rows, :3], m[rows, 3:])
            # (three points span a plane: sigma_3 = 0 and the sign of det(V U^T) is the SVD's choice -- the fix makes R proper either way)
            assert o["valid"] and (rows == slice(0, 3) or not o["flipped"])
            assert np.abs(o["model"][:3, :3] - sc["R"]).max() < 1e-12 and np.abs(o["model"][:3, 3] - sc["t"]).max() < 1e-12
            assert np.array_equal(o["model"][3], [0, 0, 0, 1])


def test_oracle_kabsch_is_a_proper_rotation_when_the_data_are_a_reflection():
    rng = np.random.default_rng(3)
    p = rng.uniform(0, 1, (6, 3))
    q = p * np.array([1.0, 1.0, -1.0]) + 0.3            # a mirror image: the unconstrained orthogonal fit has det -1
    o = R.kabsch(p, q)
    assert o["valid"] and o["flipped"], "the det(V U^T) < 0 branch was not taken"
    Rm = o["model"][:3, :3]
    assert abs(np.linalg.det(Rm) - 1.0) < 1e-12 and np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12
    # and it is the best proper rotation: no rotation near it has a smaller residual
    def cost(Rr):
        c0, c1 = p.mean(0), q.mean(0)
        return (((q - c1) - (p - c0) @ Rr.T) ** 2).sum()
    base = cost(Rm)
    for _ in range(50):
        w = 1e-3 * rng.standard_normal(3)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        dR = np.eye(3) + K + 0.5 * K @ K
        U, _, Vt = np.linalg.svd(dR)
        assert cost((U @ Vt) @ Rm) >= base - 1e-12


def test_oracle_degenerate_samples_are_invalid_identities():
    line = np.array([[0, 0, 0], [1, 2, 3], [2, 4, 6]], float)
    other = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], float)
    twin = np.array([[1, 2, 3], [1, 2, 3], [4, 0, 1]], float)
    for p, q in ((line, other), (other, line), (twin, twin + 1.0)):
        o = R.kabsch(p, q)
        assert not o["valid"] and np.array_equal(o["model"], np.eye(4))
    assert not R.kabsch(other[:2], other[:2])["valid"]
    bad = other.copy()
    bad[0, 0] = np.nan
    assert not R.kabsch(bad, other)["valid"]


def test_oracle_stop_rule_is_the_drivers():
    from differentiable_ransac_amd.ransac import adaptive_iteration_number
    for N in (7, 300, 2049):
        for inl in sorted({0, 1, 3, N // 7, N // 3, N // 2, N - 1, N}):
            for conf, eps, mx in ((0.999, 1e-5, 5000), (0.99, 1e-9, 2000), (0.999, 1e-5, 64)):
                want = min(mx, adaptive_iteration_number(inl, N, 3, conf, eps, mx))
                assert R.stop_rule(inl, N, conf, eps, mx) == pytest.approx(want, rel=1e-15, abs=0), (N, inl, conf, eps, mx)


def test_oracle_update_rules():
    sc = R.scene(2, 50, 0.7)
    m = sc["matches"]
    good = np.eye(4)
    good[:3, :3], good[:3, 3] = sc["R"], sc["t"]
    models = np.stack([np.eye(4), good, good])
    st = R.new_state(50, 1000)
    # iters == 0: a score below best_score is still taken; ties go to the lowest index; NaN and invalid slots never win
    st["best_score"] = 5.0
    assert R.update(st, m, models, np.array([1, 1, 1]), np.array([np.nan, 2.0, 2.0]), 0.05, 10, max_iterations=1000) == 1
    assert st["iters"] == 10 and st["best_score"] == 2.0 and st["best_inliers"] == int(st["best_mask"].sum()) >= 30
    assert st["max_iters"] == R.stop_rule(st["best_inliers"], 50, max_iterations=1000)
    before = dict(st)
    assert R.update(st, m, models, np.array([0, 0, 0]), np.array([9.0, 9.0, 9.0]), 0.05, 10, max_iterations=1000) is None
    if before["iters"] < before["max_iters"]:
        assert st["iters"] == 20 and st["best_score"] == 2.0
    st["iters"] = 10 ** 6                                # terminated: nothing moves
    assert R.update(st, m, models, None, np.array([9.0, 9.0, 9.0]), 0.05, 10) is None and st["iters"] == 10 ** 6


def test_oracle_msac_counts_by_distance():
    m = np.zeros((3, 6))
    m[:, 3] = [0.0, 0.03, 0.05]                         # distances 0, 0.03, 0.05 under the identity
    s, n, r = R.msac(m, np.eye(4), 0.05)
    assert n == 2 and np.allclose(r, [0, 0.36, 1.0]) and s == pytest.approx(1.0 + 0.64)


def test_header_declares_and_library_exports_the_registration_entries():
    declared = set(L.entries()) | {"dr_version", "dr_last_error"}
    assert not [s for s in SYMBOLS if s not in declared]
    lib = L.lib()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    assert lib.dr_version() == 1


def test_entries_refuse_bad_arguments_without_a_gpu():
    import ctypes
    lib = L.lib()
    assert lib.dr_kabsch_gather_f32(None, None, 1, 1, 3, 3, None, None, None) == -1 and b"null" in lib.dr_last_error()
    buf = (ctypes.c_char * 64)()
    assert lib.dr_kabsch_gather_f32(buf, buf, 1, 1, 3, 2, buf, buf, None) == -1       # k = 2
    assert lib.dr_kabsch_gather_f64(buf, buf, 1, 1, 3, 9, buf, buf, None) == -1       # k = 9
    assert lib.dr_rigid_msac_score_f32(buf, buf, None, buf, 1, 0, 3, buf, None, None, None, None) == -1
    assert lib.dr_rigid_msac_score_f32(buf, buf, None, buf, 1, 1, 3, buf, None, buf, None, None) == -1   # half a gate
    assert lib.dr_refit_rigid_f64(buf, None, None, 0, 3, buf, buf, None) == -1


def test_driver_constructor_checks():
    import differentiable_ransac_amd as pkg
    from differentiable_ransac_amd.ransac import BatchedRegistration, _SeededDriver
    assert pkg.BatchedRegistration is BatchedRegistration and issubclass(BatchedRegistration, _SeededDriver)
    drv = BatchedRegistration(ransac_batch_size=1024, threshold=0.05, confidence=0.999, max_iterations=5000, tau=1.0, seed=0,
                              num_samples=3, refit=True, eps=1e-5)
    assert drv.seed == 0 and drv.rounds == 5 and drv.device_termination is False
    for k in (2, 9, 0, -1):
        with pytest.raises(ValueError):
            BatchedRegistration(num_samples=k)
    for k in (3, 8):
        BatchedRegistration(num_samples=k)
    for mx in (0, -5):
        with pytest.raises(ValueError):
            BatchedRegistration(max_iterations=mx)
    # device termination issues every round: refused above 16 of them, before anything touches a GPU
    many = BatchedRegistration(ransac_batch_size=64, max_iterations=2000)       # 32 rounds
    with pytest.raises(ValueError):
        many.device_termination = True
    assert many.device_termination is False
    few = BatchedRegistration(ransac_batch_size=64, max_iterations=1024)        # 16 rounds
    few.device_termination = True
    assert few.device_termination is True
    few.max_iterations = 2000                                                    # changed after the switch: refused at the call
    import torch
    with pytest.raises(ValueError):
        few(torch.zeros(1, 4, 6), torch.zeros(1, 4))
    with pytest.raises(ValueError):
        drv(torch.zeros(1, 4, 4), torch.zeros(1, 4))                              # two-view correspondences
