"""tests/msac_ref.py checked on the host: the f64 reference against the CPU oracle, a plain f32 emulation of the scoring
expression against the bound, the cap and the score rule on every input family of tests/test_gpu_msac_paths.py, the six
corruptions the comparison has to reject, and the restated launch rule on every shape of the GPU tests."""
import pytest
import torch

from oracle import cpu_ref as O
from tests import msac_ref as R

F32 = torch.float32
# (name, M, N, threshold, specials): the families of the GPU tests at host-sized shapes
FAMILIES = [("ladder", 65, 2064, R.THR, ()), ("short", 33, 129, R.THR, ()), ("odd", 65, 263, R.THR, ()),
            ("huge_threshold", 17, 272, R.THR_HUGE, ()), ("tiny_threshold", R.TINY_M, 272, R.THR_TINY, ()),
            ("specials", 65, 272, R.THR, ((0, "nan"), (31, "inf"), (63, "zero"), (64, "m0"), (17, "m0")))]


def _thr32(thr):
    return float(torch.tensor(thr, dtype=F32))


@pytest.fixture(scope="module")
def families():
    out = {}
    for name, M, N, thr, specials in FAMILIES:
        mt, md = R.two_view_sets(2, M, N, seed=R.TINY_SEED if thr == R.THR_TINY else 900, specials=specials)
        refs = [R.sampson_ref(mt[s], md[s], _thr32(thr)) for s in range(2)]
        out[name] = (mt, md, thr, refs)
    return out


def _emulated_buffers(mt, md, thr, valid=None):
    S, M, N = md.shape[0], md.shape[1], mt.shape[1]
    mb, m0, sb, s0 = R.new_buffers(S, M, N, F32, "cpu")
    res = [R.emulate_f32(mt[s], md[s], thr, None if valid is None else valid[s]) for s in range(S)]
    R.fill_outputs(mb, m0, sb, s0, torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res]))
    return mb, m0, sb, s0


def test_reference_matches_the_cpu_oracle(families):
    for name in ("ladder", "short", "huge_threshold", "tiny_threshold"):
        mt, md, thr, refs = families[name]
        for s in range(2):
            so, mo = O.msac_score(mt[s].double(), md[s].double(), _thr32(thr))
            assert torch.equal(refs[s]["masks"], mo), name
            assert torch.allclose(refs[s]["scores"], so, rtol=1e-12, atol=1e-12), name
    rows = families["ladder"][3][0]["masks"].double().mean(-1)
    assert 0.3 < float(rows[0]) < 0.5 and float(rows[4]) < 0.02     # the ladder: many inliers at sigma = 0, few at 5e-2
    assert families["huge_threshold"][3][0]["masks"].all() and not families["tiny_threshold"][3][0]["masks"].any()


def test_special_models_and_zero_over_zero_points(families):
    mt, md, thr, refs = families["specials"]
    r = refs[0]
    assert r["nan"].nonzero().flatten().tolist() == [0, 31, 63]
    assert torch.isnan(r["scores"][[0, 31, 63]]).all() and not r["masks"][[0, 31, 63]].any()
    assert torch.isnan(r["d2"][64, 0]) and not r["masks"][64, 0] and torch.isfinite(r["scores"][64])   # 0/0: no inlier, adds 0


def test_f32_emulation_stays_inside_the_bound_the_cap_and_the_score_rule(families):
    worst = 0.0
    for name, (mt, md, thr, refs) in families.items():
        N = mt.shape[1]
        _, _, ny, cpb, _ = R.dispatch(2, md.shape[1], N)
        exp = R.stack_refs(refs, R.c_red(cpb, ny))
        st = R.compare(*_emulated_buffers(mt, md, thr), exp, 2)
        assert st["excl_bytes"] <= R.CAP_BYTES and st["excl_inliers"] <= R.CAP_INLIERS, name
        # the error of the emulated d2 itself against the bound, over the inlier range (d2 <= 4 thr2)
        for s in range(2):
            ref = refs[s]
            d2e = _emulated_d2(mt[s], md[s])
            rng = (ref["d2"] <= 4 * ref["thr2"]) & ~ref["nan"][:, None] & torch.isfinite(ref["d2"])
            if rng.any():
                ratio = ((d2e - ref["d2"]).abs() / ref["bound"])[rng]
                worst = max(worst, float(ratio.max()))
    print("worst |d2 error| / bound of the f32 emulation:", worst)
    assert worst <= 1.0


def _emulated_d2(mt, md):
    import numpy as np
    f = np.float32
    x1, y1, x2, y2 = (mt.numpy().astype(f)[None, :, i] for i in range(4))
    m = [md.reshape(-1, 9).numpy().astype(f)[:, q][:, None] for q in range(9)]
    with np.errstate(all="ignore"):
        a0 = x2 * m[0] + (y2 * m[3] + m[6])
        a1 = x2 * m[1] + (y2 * m[4] + m[7])
        a2 = x2 * m[2] + (y2 * m[5] + m[8])
        b0 = x1 * m[0] + (y1 * m[1] + m[2])
        b1 = x1 * m[3] + (y1 * m[4] + m[5])
        r = x1 * a0 + (y1 * a1 + a2)
        jj = a0 * a0 + (a1 * a1 + (b0 * b0 + b1 * b1))
        return torch.from_numpy(((r * r) * (1.0 / jj.astype(np.float64)).astype(f)).astype(np.float64))


def test_reference_alone_stays_inside_the_cap_on_every_case_of_the_gpu_tests():
    worst_b = worst_i = 0.0
    for c in R.gpu_cases():
        _, _, valid, refs = R.case_inputs(c)
        n_excl, n_in, n_bytes = R.reference_cap(refs, c["P"], valid)
        assert n_excl <= R.CAP_BYTES * n_bytes and n_excl <= R.CAP_INLIERS * n_in, (c, n_excl, n_in, n_bytes)
        worst_b = max(worst_b, n_excl / n_bytes)
        worst_i = max(worst_i, n_excl / n_in if n_in else 0.0)
    print("worst excluded share of the bytes / of the inliers:", worst_b, worst_i)


def test_valid_patterns():
    for name in R.VALID_PATTERNS:
        v = R.valid_pattern(name, 3, 70)
        assert v.shape == (3, 70) and v.dtype == torch.bool
    assert R.valid_pattern("one", 3, 70)[0, :32].sum() == 1 and R.valid_pattern("all_but_one", 3, 70)[1, 32:64].sum() == 31
    assert R.valid_pattern("second_word", 1, 70)[0].nonzero().flatten().tolist() == list(range(32, 64))
    assert R.valid_pattern("last_partial_word", 1, 70)[0].nonzero().flatten().tolist() == list(range(64, 70))


# ---- the comparison rejects each corruption of a correct output -------------------------------------------------------------
@pytest.fixture()
def correct(families):
    mt, md, thr, _ = families["specials"]
    M, N = md.shape[1], mt.shape[1]
    valid = R.valid_pattern("all_but_one", 2, M)
    valid[:, 40] = False
    refs = [R.sampson_ref(mt[s], md[s], _thr32(thr)) for s in range(2)]
    exp = R.stack_refs(refs, R.c_red(1, 1))
    bufs = _emulated_buffers(mt, md, thr, valid)
    R.compare(*bufs, exp, 2, valid=valid)              # the uncorrupted output passes
    return bufs, exp, valid, refs, (M, N)


def _rejected(bufs, exp, valid, match):
    with pytest.raises(AssertionError, match=match):
        R.compare(*bufs, exp, 2, valid=valid)


def test_rejects_an_empty_row_left_as_sentinel(correct):
    (mb, m0, sb, s0), exp, valid, _, (M, N) = correct
    mb[m0 + 40 * N:m0 + 41 * N] = R.MASK_SENTINEL       # slot 40 is invalid: its row is an empty one
    _rejected((mb, m0, sb, s0), exp, valid, "other than 0 / 1")


def test_rejects_two_bytes_swapped_inside_a_word(correct):
    (mb, m0, sb, s0), exp, valid, refs, (M, N) = correct
    row = mb[m0 + 10 * N:m0 + 11 * N]                   # slot 10: sigma = 0, a populated row
    free = ~refs[0]["excl"][10]
    w = next(i for i in range(0, N - 3, 4) if row[i] != row[i + 1] and free[i] and free[i + 1])
    row[w], row[w + 1] = row[w + 1].clone(), row[w].clone()
    _rejected((mb, m0, sb, s0), exp, valid, "mask bytes differ")


def test_rejects_a_score_without_one_lanes_partial(correct):
    (mb, m0, sb, s0), exp, valid, refs, (M, N) = correct
    r = refs[0]
    term = torch.where(r["masks"][10], 1 - r["d2"][10] / r["thr2"], torch.zeros(N, dtype=torch.float64))
    lane = max(range(0, N, 16), key=lambda i: float(term[i:i + 16].sum()))
    assert float(term[lane:lane + 16].sum()) > 0
    sb[s0 + 10] -= term[lane:lane + 16].sum().float()
    _rejected((mb, m0, sb, s0), exp, valid, "score rule")


def test_rejects_a_row_written_at_slot_M_of_a_partial_tile(correct):
    (mb, m0, sb, s0), exp, valid, _, (M, N) = correct
    mb[m0 + 2 * M * N:m0 + 2 * M * N + 16] = 0          # the first bytes past the last pair's last row
    _rejected((mb, m0, sb, s0), exp, valid, "mask guard")


def test_rejects_a_stale_mask_byte_of_two(correct):
    (mb, m0, sb, s0), exp, valid, _, (M, N) = correct
    mb[m0 + 10 * N + 5] = 2
    _rejected((mb, m0, sb, s0), exp, valid, "other than 0 / 1")


def test_rejects_a_zero_score_where_nan_is_due(correct):
    (mb, m0, sb, s0), exp, valid, _, (M, N) = correct
    assert valid[0, 31] and exp["nan"][0, 31]
    sb[s0 + 31] = 0.0
    _rejected((mb, m0, sb, s0), exp, valid, "score not NaN")


def test_rejects_writes_to_a_gated_pair_and_gaps_in_an_open_one(correct):
    (mb, m0, sb, s0), exp, valid, _, (M, N) = correct
    gated = torch.tensor([False, True])
    with pytest.raises(AssertionError, match="gated pair written"):
        R.compare(mb, m0, sb, s0, exp, 2, valid=valid, gated=gated)
    sb[s0 + M:s0 + 2 * M] = R.SCORE_SENTINEL
    mb[m0 + M * N:m0 + 2 * M * N] = R.MASK_SENTINEL
    R.compare(mb, m0, sb, s0, exp, 2, valid=valid, gated=gated)


# ---- the restated launch rules ------------------------------------------------------------------------------------------------
def test_dispatch_reaches_the_intended_path_for_every_gpu_shape():
    for P, M, N, dt, aligned, want in R.intended_paths():
        assert R.dispatch(P, M, N, dt, aligned) == want, (P, M, N, dt, aligned)
    assert R.dispatch(2, 10240, 2000) == ("fast16", 16, 1, 1, False)     # the full-size test of test_gpu_msac.py: a small grid
    assert R.dispatch(128, 10240, 2000) == ("fast16", 64, 1, 1, False)   # the benchmark's form


def test_rigid_dispatch_names_the_tile():
    assert R.rigid_dispatch(1, 2048, 50000 - 50000 % 16, 9e-4) == ("pk8", 34, 49, 1)       # one pair, 2048 models: 61 tiles of 34
    for P in R.RIGID_P:
        for M in R.RIGID_M:
            for N in R.RIGID_N:
                k, tile, ny, cpb = R.rigid_dispatch(P, M, N, 9e-4)
                assert (k, tile, ny, cpb) == ("pk8", 4, (N + 1023) // 1024, 1)
    assert R.rigid_dispatch(*R.RIGID_TILE6, 9e-4) == ("pk8", 6, 5, 1)
    assert R.rigid_dispatch(*R.RIGID_TILE34, 9e-4) == ("pk8", 34, 1, 1) and R.rigid_dispatch(*R.RIGID_TILE64, 9e-4) == ("pk8", 64, 1, 1)
    assert R.rigid_dispatch(3, 70, 2063, 9e-4)[0] == "general" and R.rigid_dispatch(3, 70, 2064, 1e-12)[0] == "general"
    assert R.rigid_dispatch(3, 70, 2064, 9e-4, torch.float64)[0] == "general"


def test_rigid_reference_alone_stays_inside_the_cap():
    for N in R.RIGID_N + (2063,):
        pts, md = R.rigid_sets(3, max(R.RIGID_M), N, 3000 + N)
        for thr in (9e-4, 1e-12):
            refs = [R.rigid_ref(pts[s], md[s], _thr32(thr)) for s in range(3)]
            for M in R.RIGID_M:
                for P in R.RIGID_P:
                    n_excl = sum(int(r["excl"][:M].sum()) for r in refs[:P])
                    n_in = sum(int(r["masks"][:M].sum()) for r in refs[:P])
                    assert n_excl <= R.CAP_BYTES * P * M * N and n_excl <= R.CAP_INLIERS * n_in, (N, thr, M, P, n_excl, n_in)
