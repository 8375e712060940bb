"""Local optimisation of the registration path without a GPU: the properties of the restatement tests/registration_lo_ref.py, the
ABI of dr_registration_local_opt (declared, exported, DR_EINVAL before any device work), the constructor checks of
BatchedRegistration(lo=, lo_iters=), and the cases of tests/test_gpu_registration_lo.py with the exclusion rule applied to them.

The exclusion cap on the reference's side.  A case (N, lo, pair, dtype) is left out of the comparison when a fit of the oracle's
trajectory has an acceptance margin below twice registration_ref.score_tolerance or a point inside registration_ref.BAND.  Asserted
here: no f64 case is left out; for every N >= 255 at least one remaining case with lo = 2 runs more than one fit, and one with lo = 1
runs its fit and accepts it (lo = 1 cannot run more than one).  The f32 cap "at most a quarter" cannot be met by any choice of seeds:
the f32 score tolerance 16 eps32 N mag^2 / thr^2 is 4-12 at N = 255..257 and 20-49 at N = 1000 on these scenes, a converging lo = 2
trajectory always ends in fits that gain less than that (all 24 f32 cases with lo = 2 and N >= 255 are left out by the margin rule
alone), and a 15 % pair's whole score stays below twice the tolerance.  Measured: 42 of the 60 f32 cases are left out (12 of the 18
kept are the N = 3 cases); the test pins that number so that a change of seeds cannot lose more.  The f32 kernel is held to the
oracle in the kept cases, and in the excluded ones to the decision-independent invariants of test_gpu_registration_lo.py."""
import ctypes

import numpy as np
import pytest

from differentiable_ransac_amd import _lib as L
from tests import registration_lo_ref as LR
from tests import registration_ref as R

SYMBOLS = ["dr_registration_local_opt_f32", "dr_registration_local_opt_f64"]
THR = R.THRESHOLD


def _copy(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def _seeded(seed, N, share, pick=0):
    sc = R.scene(seed, N, share, noise=0.02)
    rows = np.sort(np.random.default_rng(pick).choice(np.flatnonzero(sc["inlier"]), 3, replace=False))
    return sc, LR.seeded_state(sc["matches"], rows, THR)


SCENES = [(s, N, share) for s, (N, share) in enumerate([(300, 0.6), (300, 0.35), (300, 0.15), (120, 0.5), (700, 0.35), (64, 0.6)])]


# ------------------------------------------------------------------------------------------------ oracle properties
@pytest.mark.parametrize("seed,N,share", SCENES)
def test_lo_never_lowers_a_score_and_orders_its_modes(seed, N, share):
    sc, st0 = _seeded(50 + seed, N, share)
    m = sc["matches"]
    st1, st2 = _copy(st0), _copy(st0)
    f1 = LR.lo_step(st1, m, THR, 1, 8, LR.new_seen())
    f2 = LR.lo_step(st2, m, THR, 2, 8, LR.new_seen())
    assert st0["best_score"] <= st1["best_score"] <= st2["best_score"]
    assert len(f1) == 1 and 1 <= len(f2) <= 8 and st1["lo_refits"] == 1 and st2["lo_refits"] == len(f2)
    prev = st0["best_score"]
    for f in f2:                                        # every accepted fit raises the score strictly
        if f["accepted"]:
            assert f["score"] > prev
            prev = f["score"]
    for st in (st1, st2):                               # the state stays consistent
        s, n, r = R.msac(m, st["best_model"], THR)
        assert s == st["best_score"] and n == st["best_inliers"] and np.array_equal(r < 1.0, st["best_mask"])
        assert st["max_iters"] == R.stop_rule(n, N)
    # the rotation error to the generating pose does not grow (noise 0.02)
    e0, e2 = R.rotation_error_deg(st0["best_model"], sc["R"]), R.rotation_error_deg(st2["best_model"], sc["R"])
    print(f"N={N} share={share}: score {st0['best_score']:.2f} -> {st1['best_score']:.2f} -> {st2['best_score']:.2f}, fits {len(f2)}, "
          f"rotation error {e0:.3f} -> {e2:.3f} deg")
    assert e2 <= e0


def test_loop_stops_on_a_losing_candidate_and_on_an_unchanged_mask():
    # unchanged mask: exact correspondences -- the first fit is taken (the seed hypothesis is exact too, but of other rows: its score
    # is the same up to rounding, so force the seed's score down), the mask stays all-true, and the loop ends after one fit
    sc = R.scene(7, 40, 1.0, noise=0.0)
    st = LR.seeded_state(sc["matches"], np.array([0, 1, 2]), THR)
    assert st["best_mask"].all()
    st["best_score"] -= 1.0
    fits = LR.lo_step(st, sc["matches"], THR, 2, 8, LR.new_seen())
    assert len(fits) == 1 and fits[0]["accepted"] and st["best_mask"].all()
    # losing candidate: a state that claims more than any fit reaches
    sc, st = _seeded(51, 300, 0.6)
    st["best_score"] = 1e6
    before = _copy(st)
    fits = LR.lo_step(st, sc["matches"], THR, 2, 8, LR.new_seen())
    assert len(fits) == 1 and not fits[0]["accepted"]
    assert st["best_score"] == 1e6 and np.array_equal(st["best_mask"], before["best_mask"]) and st["lo_refits"] == 1
    assert np.array_equal(st["best_model"], before["best_model"])


def test_few_inliers_and_the_gate():
    sc, st = _seeded(52, 300, 0.6)
    m = sc["matches"]
    few = _copy(st)
    few["best_mask"] = np.zeros(300, bool)
    few["best_mask"][:2] = True
    few["best_inliers"] = 2
    before, seen = _copy(few), LR.new_seen()
    assert LR.lo_step(few, m, THR, 2, 8, seen) == []
    for k in ("best_score", "best_inliers", "max_iters"):
        assert few[k] == before[k]
    assert np.array_equal(few["best_mask"], before["best_mask"]) and np.array_equal(few["best_model"], before["best_model"])
    assert seen[0] == few["best_score"] and np.array_equal(seen[1:], few["best_model"].reshape(16)) and few["lo_refits"] == 0
    # the gate: a second visit of an unchanged pair does nothing; a replaced pair is visited again
    seen = LR.new_seen()
    assert LR.lo_step(st, m, THR, 2, 8, seen)
    after = _copy(st)
    assert LR.lo_step(st, m, THR, 2, 8, seen) is None
    assert all(np.array_equal(st[k], after[k]) for k in st)
    st["best_score"] -= 0.5
    assert LR.lo_step(st, m, THR, 2, 8, seen) is not None


def test_run_lo_without_a_usable_round_is_run():
    """lo_step after every update changes nothing where no update takes a model; and run_lo reports its fits"""
    sc = R.scene(53, 300, 0.6, noise=0.02)
    rng = np.random.default_rng(3)
    idx = [np.stack([rng.permutation(300)[:3] for _ in range(16)]) for _ in range(3)]
    base = R.run(sc["matches"], idx, THR, max_iterations=48)
    lo2 = LR.run_lo(sc["matches"], idx, 2, 8, THR, max_iterations=48)
    assert lo2["score"] >= base["score"] and lo2["lo_refits"] == len(lo2["lo_fits"]) and lo2["iterations"] <= base["iterations"]


# ------------------------------------------------------------------------------------------------ library and driver
def test_header_declares_and_library_exports_the_entries():
    declared = set(L.entries()) | {"dr_version", "dr_last_error"}
    assert not [s for s in SYMBOLS if s not in declared]
    lib = L.lib()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    assert lib.dr_version() == 1


def test_entries_refuse_bad_arguments_without_a_gpu():
    lib = L.lib()
    buf = (ctypes.c_char * 256)()
    d = ctypes.c_double
    for s in SYMBOLS:
        fn = getattr(lib, s)

        def call(matches=buf, thr2=buf, P=1, N=1, lo=1, lo_iters=1, score=buf, model=buf, mask=buf, inl=buf, mi=buf, seen=buf,
                 refits=None):
            return fn(matches, thr2, P, N, lo, lo_iters, d(0.999), d(1e-5), 100, score, model, mask, inl, mi, seen, refits, None)

        for name in ("matches", "thr2", "score", "model", "mask", "inl", "mi", "seen"):
            assert call(**{name: None}) == -1 and b"null" in lib.dr_last_error(), name
        for kw in (dict(P=0), dict(P=-1), dict(N=0), dict(N=-3)):
            assert call(**kw) == -1 and b"registration_local_opt" in lib.dr_last_error(), kw
        for lo in (0, 3, -1):
            assert call(lo=lo) == -1 and b"lo must be" in lib.dr_last_error()
        for lo in (1, 2):
            for it in (0, -1):
                assert call(lo=lo, lo_iters=it) == -1 and b"lo_iters" in lib.dr_last_error()


def test_constructor_checks():
    from differentiable_ransac_amd.ransac import BatchedRegistration
    d = BatchedRegistration()
    assert d.lo == 0 and d.lo_iters == 64
    assert BatchedRegistration(lo=0, train=True).lo == 0
    assert BatchedRegistration(lo=2, lo_iters=5).lo_iters == 5 and BatchedRegistration(lo=1).lo == 1
    with pytest.raises(NotImplementedError):
        BatchedRegistration(lo=3)
    for bad in (4, -1):
        with pytest.raises(ValueError):
            BatchedRegistration(lo=bad)
    with pytest.raises(ValueError):
        BatchedRegistration(lo=2, lo_iters=0)
    for lo in (1, 2):
        with pytest.raises(ValueError):
            BatchedRegistration(lo=lo, train=True)


def test_wrapper_refuses_cpu_tensors(monkeypatch):
    import torch
    from differentiable_ransac_amd import ops
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda *a: calls.append(a))
    st = ops.RegistrationState(2, 16, 100, "cpu", torch.float32)
    with pytest.raises(L.DransacError):
        ops.registration_local_optimize(st, torch.rand(2, 16, 6), torch.full((2,), 0.0025), 1, 8, lo_seen=torch.full((2, 17), float("nan")))
    assert calls == []


# ------------------------------------------------------------------------------------------------ the GPU test's cases
F32_LEFT_OUT = 42      # measured on the reference alone (module docstring)


def test_gpu_cases_respect_the_exclusion_cap():
    left = {"float32": 0, "float64": 0}
    for name in left:
        for N in LR.LO_NS:
            for lo in (1, 2):
                cases = LR.build_case(N, lo, name)
                left[name] += sum(c["excluded"] for c in cases)
                kept = [c for c in cases if not c["excluded"]]
                if N == 3:      # the few-inlier rule: no fit runs
                    assert all(c["seed"]["best_inliers"] < 3 and c["fits"] == [] for c in cases)
                elif name == "float64":
                    if lo == 2:
                        assert any(len(c["fits"]) > 1 for c in kept), (N, lo)
                        assert all(1 <= len(c["fits"]) <= LR.LO_ITERS for c in kept)
                    else:
                        assert any(len(c["fits"]) == 1 and c["fits"][0]["accepted"] for c in kept), (N, lo)
    print("cases left out:", left)
    assert left["float64"] == 0
    assert left["float32"] <= F32_LEFT_OUT
