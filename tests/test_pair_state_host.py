"""ops.RegistrationState and ops.HomographyState allocate what their docstrings state (CPU tensors: no library call is involved)."""
import pytest
import torch

from differentiable_ransac_amd import ops


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("cls,side", [(ops.RegistrationState, 4), (ops.HomographyState, 3)])
def test_state_shapes_dtypes_and_initial_values(cls, side, dt):
    P, N, maxit = 3, 7, 5000
    st = cls(P, N, maxit, "cpu", dt)
    want = dict(best_score=(torch.zeros(P, dtype=dt)), best_model=torch.eye(side, dtype=dt).expand(P, side, side),
                best_mask=torch.zeros(P, N, dtype=torch.bool), best_inliers=torch.zeros(P, dtype=torch.int32),
                iters=torch.zeros(P, dtype=torch.int32), max_iters=torch.full((P,), 5000.0, dtype=torch.float64))
    for name, w in want.items():
        got = getattr(st, name)
        assert got.dtype == w.dtype and got.shape == w.shape and torch.equal(got, w), name
        assert got.is_contiguous(), name
    assert st.max_iterations == maxit and isinstance(st.max_iterations, int)
    assert sorted(vars(st)) == sorted(list(want) + ["max_iterations"])
    # the pairs' models are separate storage: the update kernel writes one pair's slot
    st.best_model[0, 0, 0] = 2.0
    assert float(st.best_model[1, 0, 0]) == 1.0
