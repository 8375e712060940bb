"""The five-point backward kernels at the tail of a launch: Bt = 65 is one full wave plus a block with one live lane.  A lane's
arithmetic reads no other lane's data, so what sample 64 gets there equals what it gets alone (Bt = 1) bit for bit, and a
degenerate neighbour changes nobody else's gradient: every equality below is exact, not to a tolerance."""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

BT = 65           # 64 + 1: the second block has one live lane
DEGENERATE = 7    # the sample case 2 replaces


@functools.lru_cache(maxsize=None)
def _minimal_inputs():
    """samples [1,65,5,4] f32 (inliers of one synthetic pair, 2e-3 noise), gt [1,3,3], the upstream gradient of `chosen`"""
    from differentiable_ransac_amd import synth
    pair = synth.two_view_pair(1700, BT * 5, inlier_ratio=1.0, noise=2e-3)
    W = torch.randn(1, BT, 3, 3, generator=torch.Generator().manual_seed(17))
    return pair["matches"].reshape(1, BT, 5, 4).contiguous(), pair["gt_E"][None].contiguous(), W


def _one_node(samples, gt, W, dev):
    """ops.solve_select_essential: the sparse gradient (dr_solve_nister5_bwd_sel_f32) -> grad_samples, valid, keep on the host"""
    from differentiable_ransac_amd import ops
    s = samples.to(dev).requires_grad_(True)
    chosen, _, keep, _, valid = ops.solve_select_essential(s, gt.to(dev))
    (chosen * W.to(dev) * keep[..., None, None]).sum().backward()
    return s.grad.cpu(), valid.cpu(), keep.cpu()


def _two_node(samples, gt, W, dev):
    """ops.solve_essential + ops.select_closest_autograd: the dense [.,10,9] gradient (dr_solve_nister5_bwd_f32)"""
    from differentiable_ransac_amd import ops
    s = samples.to(dev).requires_grad_(True)
    models, valid = ops.solve_essential(s, None, "nister")
    chosen, which = ops.select_closest_autograd(models, valid, gt.to(dev))
    (chosen * W.to(dev) * (which >= 0)[..., None, None]).sum().backward()
    return s.grad.cpu(), valid.cpu(), (which >= 0).cpu()


@functools.lru_cache(maxsize=None)
def _minimal_baseline():
    """both routes on the undisturbed samples: computed once, read by cases 1 and 2"""
    dev = torch.device("cuda:0")
    return _one_node(*_minimal_inputs(), dev), _two_node(*_minimal_inputs(), dev)


def test_minimal_tail_lane_equals_the_sample_alone(dev):
    """Case 1: the one-node and the two-node route agree (the tolerance of tests/test_gpu_round3.py for this pair of routes:
    1e-6 of the largest entry), and sample 64 -- the only live lane of the second block -- gets the bits it gets at Bt = 1."""
    samples, gt, W = _minimal_inputs()
    (g1, _, keep1), (g2, _, keep2) = _minimal_baseline()
    assert torch.equal(keep1, keep2) and bool(keep1[0, BT - 1])
    assert float(g2.abs().max()) > 0 and torch.isfinite(g1).all() and torch.isfinite(g2).all()
    assert (g1 - g2).abs().max() <= 1e-6 * g2.abs().max()
    for route, g in ((_one_node, g1), (_two_node, g2)):
        alone, _, keep = route(samples[:, BT - 1:], gt, W[:, BT - 1:], dev)
        assert bool(keep[0, 0]) and float(alone.abs().max()) > 0
        assert torch.equal(alone[0, 0], g[0, BT - 1]), route.__name__


def test_degenerate_sample_gets_zero_and_disturbs_no_other(dev):
    """Case 2: sample 7 becomes a pair of views without motion, x2 = x1 in all five rows: every skew-symmetric matrix satisfies
    the five constraints, a continuum of essential matrices, and the solver verifies none.  (Five copies of one correspondence
    do not serve: the device verifies six models in the four null vectors it keeps of that rank-one system.)  The forward
    reports no valid model for the sample, its gradient rows are exact zeros in both routes, and every other sample's
    gradient keeps its bits."""
    samples, gt, W = _minimal_inputs()
    samples = samples.clone()
    samples[0, DEGENERATE, :, 2:] = samples[0, DEGENERATE, :, :2]
    others = torch.arange(BT) != DEGENERATE
    for route, base in zip((_one_node, _two_node), _minimal_baseline()):
        g, valid, keep = route(samples, gt, W, dev)
        assert not bool(valid[0, DEGENERATE].any()) and not bool(keep[0, DEGENERATE]), route.__name__
        assert torch.equal(g[0, DEGENERATE], torch.zeros(5, 4)), route.__name__
        assert torch.equal(g[0, others], base[0][0, others]), route.__name__


@pytest.mark.parametrize("n", [6, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_nonminimal_tail_lane_equals_the_sample_alone(dev, dtype, n):
    """Case 3: n > 5 rows with row weights that require grad (dr_solve_nister5_nm_bwd_f32 / _f64): grad_samples and
    grad_weights of sample 64 at Bt = 65 equal those of the same rows and weights alone; without weights the node returns
    None for the weight gradient although it is asked for one."""
    from differentiable_ransac_amd import ops, synth
    pair = synth.two_view_pair(1800 + n, BT * n, inlier_ratio=1.0, noise=2e-3, dtype=dtype)
    samples = pair["matches"].reshape(BT, n, 4).contiguous()
    gen = torch.Generator().manual_seed(n)
    weights = (0.5 + torch.rand(BT, n, generator=gen)).to(dtype)
    W = torch.randn(BT, 10, 3, 3, generator=gen).to(dtype)

    def run(rows):
        s = samples[rows].to(dev).requires_grad_(True)
        w = weights[rows].to(dev).requires_grad_(True)
        E, valid = ops.solve_essential(s, w, "nister")
        (E * W[rows].to(dev) * valid[..., None, None]).sum().backward()
        assert s.grad.dtype == dtype and w.grad.dtype == dtype
        return s.grad.cpu(), w.grad.cpu(), valid.cpu()

    gs, gw, valid = run(slice(None))
    assert bool(valid[BT - 1].any()) and torch.isfinite(gs).all() and torch.isfinite(gw).all()
    gs1, gw1, valid1 = run(slice(BT - 1, BT))
    assert torch.equal(valid1[0], valid[BT - 1])
    assert float(gs1.abs().max()) > 0 and float(gw1.abs().max()) > 0
    assert torch.equal(gs1[0], gs[BT - 1]) and torch.equal(gw1[0], gw[BT - 1])

    s = samples.to(dev).requires_grad_(True)
    E, valid_d = ops.solve_essential(s, None, "nister")
    node = E.grad_fn
    asked = types.SimpleNamespace(saved_tensors=node.saved_tensors, minimal=node.minimal, weights=node.weights,
                                  needs_input_grad=(True, True, False))
    out = ops._SolveEssential.backward(asked, W.to(dev) * valid_d[..., None, None], None)
    assert out[1] is None and out[2] is None and out[0].shape == s.shape and float(out[0].abs().max()) > 0
