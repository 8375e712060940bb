"""The refit restatements (tests/refit_ref.py) checked against themselves, on the CPU: the two f64 forms of the F refit agree on
every input the GPU tests use, the eigen-gap sweep holds the hard bins, and a transcription of the fixed 24-step inverse
iteration the F refit used to run misses the GPU test's tolerance on them -- which is why tests/test_gpu_refit.py exists."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from tests import refit_ref as R


@pytest.fixture(scope="module")
def f_inputs():
    return R.all_f_inputs()


def test_two_reference_forms_agree_on_every_gpu_input(f_inputs):
    """distance(eigh of A^T A, svd of A) <= REF_AGREEMENT * eps64 * cond, inputs in f64 and rounded to f32"""
    worst = 0.0
    for lab, m, k, w in f_inputs:
        for dt in (torch.float64, torch.float32):
            r = R.f_refit_forms(m.to(dt), k, None if w is None else w.to(dt))
            assert r["valid"], lab
            c = r["distance"] / (R.EPS64 * r["cond"])
            worst = max(worst, c)
            assert c <= R.REF_AGREEMENT, (lab, dt, c, r["cond"])
    print(f"worst distance / (eps64 * cond) = {worst:.1f}")
    assert worst > 0


def test_restatement_is_the_oracle_on_a_wide_gap():
    m, k = R.contaminated(0, 64, 0, R.SWEEP_N)
    F, valid, cond, ratio = R.f_refit(m, k)
    Fo = O.fundamental_8pt(m[k][None])[0]
    assert valid and R.rel_err(F, Fo) <= R.REF_AGREEMENT * R.EPS64 * cond
    w = R.moderate_weights(1, R.SWEEP_N)[0]
    Fw = R.f_refit(m, k, w)[0]
    assert R.rel_err(Fw, O.fundamental_8pt(m[k][None], w[k][None])[0]) <= R.REF_AGREEMENT * R.EPS64 * cond * 10
    F7, valid7, _, _ = R.f_refit(m[:7])
    assert not valid7 and torch.equal(F7, torch.eye(3, dtype=torch.float64))
    E, real = R.e_refit(m, k)
    Eo, ok, ro = O.nister_5pt(m[k][None])
    assert torch.equal(E, Eo[0]) and torch.equal(real, ro[0] & ok[0])


def test_sweep_covers_the_hard_bins():
    cases = R.sweep_cases()
    assert len(cases) <= 64
    ratios = []
    for lab, m, k in cases:
        assert int(k.sum()) <= 64 and m.shape == (R.SWEEP_N, 4)
        _, valid, cond, ratio = R.f_refit(m, k)
        assert valid and cond <= R.MAX_COND, (lab, cond)
        ratios.append(ratio)
    for lo, hi in R.RATIO_BINS:
        n = sum(1 for r in ratios if lo <= r < hi or (hi == R.RATIO_BINS[-1][1] and r == hi))
        assert n >= R.MIN_PER_BIN, ((lo, hi), n)


def invit24(G):
    """smallest_eigvec9_invit as the F refit ran it: Cholesky of G + 1e-14 tr(G) I, fixed start, 24 inverse-iteration steps"""
    G = np.asarray(G, dtype=np.float64)
    L = np.zeros((9, 9))
    inv = np.zeros(9)
    shift = 1e-14 * np.trace(G)
    for j in range(9):
        d = max(G[j, j] + shift - L[j, :j] @ L[j, :j], 1e-300)
        inv[j] = 1.0 / np.sqrt(d)
        for i in range(j + 1, 9):
            L[i, j] = (G[i, j] - L[i, :j] @ L[j, :j]) * inv[j]
    x = 1.0 / 3.0 + 0.01 * np.arange(9)
    for _ in range(24):
        y = np.zeros(9)
        for i in range(9):
            y[i] = (x[i] - L[i, :i] @ y[:i]) * inv[i]
        for i in range(8, -1, -1):
            x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) * inv[i]
        x = x / np.sqrt(x @ x)
    return x


def _f_from_null(m, k, vec_of_gram):
    n, T1, T2t = O.hartley_normalize(m[k][None].double())
    A = O._f_rows(n)[0]
    f = torch.from_numpy(vec_of_gram((A.T @ A).numpy()))
    return T2t[0] @ f.reshape(3, 3) @ T1[0]


def test_fixed_step_inverse_iteration_misses_the_tolerance_on_close_eigenvalues():
    """the reason for the GPU sweep: 24 steps converge like (lambda_9 / lambda_8)^24, so the routine is right on the wide gaps and
    wrong, by orders of magnitude more than the tolerance, wherever ratio >= 0.7"""
    hard = easy = 0
    for lab, m, k in R.sweep_cases():
        F, _, cond, ratio = R.f_refit(m, k)
        err = R.rel_err(_f_from_null(m, k, invit24), F)
        tol = R.f_tolerance(cond, torch.float64)
        if ratio >= 0.7:
            assert err > 100 * tol, (lab, ratio, err, tol)
            hard += 1
        elif ratio < 0.1:
            assert err <= tol, (lab, ratio, err, tol)
            easy += 1
    assert hard >= 2 * R.MIN_PER_BIN and easy >= R.MIN_PER_BIN
