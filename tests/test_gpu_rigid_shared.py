"""What csrc/rigid_device.hpp guarantees across the parity kernels of csrc/solve_rigid.hip: dr_ransac3d_update recomputes the
winner's inlier mask with the distance function dr_rigid_residual used for its mask rows (rigid_d2), so the two agree exactly --
on data where many points sit at the threshold, which is where a different operation order would show.  (f32 rows of N % 16 == 0
get their mask rows from the packed residual kernel, which keeps its own form and promises the same masks: that case is here too.)"""
import numpy as np
import pytest
import torch

from tests import registration_ref as R

pytestmark = pytest.mark.gpu

THR = R.THRESHOLD


# f32 N = 1000: the general residual kernel; f32 N = 1024 (N % 16 == 0, masks wanted): the packed one; f64: the general one
@pytest.mark.parametrize("dt,N", [(torch.float32, 1000), (torch.float32, 1024), (torch.float64, 1000)])
def test_ransac3d_update_mask_is_the_winners_residual_row(dev, dt, N):
    from differentiable_ransac_amd import ops
    P, M = 2, 33
    sc = [R.boundary_scene(40 + p, N, M) for p in range(P)]
    m = torch.from_numpy(np.stack([s[0] for s in sc])).to(dt)
    models = torch.from_numpy(np.stack([s[1] for s in sc])).to(dt)
    for p in range(P):      # the condition on the input: a strict arg-min of the residual sums, in f64 on the rounded values
        sums = [R.ratio2(models[p, j].double().numpy(), m[p].double().numpy(), THR).sum() for j in range(M)]
        gap = R.best_gap(sums, largest=False)
        print(f"pair {p}: relative gap of the two smallest residual sums {gap:.3g}")
        assert gap >= 1e-3
    tm, tmod = m.to(dev), models.to(dev)
    res, masks = ops.rigid_residual(tm, tmod, THR * THR, want_masks=True)
    best_mask = torch.zeros(P, N, dtype=torch.bool, device=dev)
    _, _, idx = ops.ransac3d_update(tm, tmod, None, res, THR * THR, None, None, best_mask)
    idx = idx.cpu().tolist()
    assert min(idx) >= 0                # no previous state: the arg-min is taken
    near = [int((np.abs(R.ratio2(models[p, idx[p]].double().numpy(), m[p].double().numpy(), THR) - 1.0) < 0.05).sum()) for p in range(P)]
    diff = [int((best_mask[p] != masks[p, idx[p]]).sum()) for p in range(P)]
    print(f"winners {idx}, points within 5 % of the threshold {near}, differing mask entries {diff}")
    assert diff == [0] * P
