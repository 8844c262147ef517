"""GPU (MI355X) checks of the fused LayerNorm + ReLU + dropout kernels and
of their wiring into the GCN / GraphSAGE models. Oracles and bounds:
tests/ln_fused_checks.py.

Run on the GPU box: python -m pytest tests/test_gpu_ln_fused.py -m gpu -x -q
"""
import pytest
import torch

import ln_fused_checks as L
from kernel_path_checks import EPS

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

# float4 form: 4 and 44 (part of one chunk), 132, 256 (one full chunk),
# 260 / 516 / 772 (the first width of the 2-, 3- and 4-chunk
# instantiations), 1024 (the largest); scalar form: 6, 41, 130
WIDTHS = [4, 44, 132, 256, 260, 516, 772, 1024, 6, 41, 130]


@needs_gpu
@pytest.mark.parametrize("F", WIDTHS)
def test_fused_equals_unfused_bitwise(F):
    """n = 1, 3 (less than a block), 4, 5 (a second block), 1030 (258
    blocks, the last half empty); act 0 / 1; keep 1.0 / 0.9 / 0.5."""
    for n in (1, 3, 4, 5, 1030):
        L.check_equal_unfused(n, F)


@needs_gpu
def test_fused_equals_unfused_beyond_block_caps():
    """131,077 rows of 4: 32,770 row groups, beyond the forward's 32,768
    blocks and 16 trips of the backward's 2,048."""
    L.check_equal_unfused(131077, 4, acts=(1,), keeps=(0.5,))


@needs_gpu
@pytest.mark.parametrize("n,F", [(5, 44), (1030, 256), (1030, 130),
                                 (9001, 132), (1030, 772)])
def test_column_sums_float64_and_repeatable(n, F):
    """9001 rows: more than the 8,192 rows of one trip of 2,048 blocks, so
    the running sums span several rows per lane and all partial rows are
    in use."""
    for act in (0, 1):
        for keep in (1.0, 0.5):
            L.check_column_sums(n, F, act, keep)


@needs_gpu
@pytest.mark.parametrize("model_name", ["graphsage", "gcn"])
def test_model_wiring_fused_vs_unfused(model_name):
    logits0, grads0, rec = L.run_model(model_name, fused=False)
    logits1, grads1, cnt = L.run_model(model_name, fused=True)
    assert torch.equal(logits1, logits0), "logits differ"
    # unfused: the input dropout + two inter-layer dropouts each way; two
    # LayerNorm backwards; a bias column sum per linear / bias_add
    final_bias_sums = 2 if model_name == "graphsage" else 1
    mid_bias_sums = 3 if model_name == "graphsage" else 2
    assert rec.calls.get("dropout_apply", 0) == 5, rec.calls
    assert rec.calls.get("ln_bwd", 0) == 2, rec.calls
    assert rec.calls.get("syncbn_stats", 0) == final_bias_sums + mid_bias_sums
    # fused: only the layer-0 input dropout and the final layer's sums
    assert cnt.calls.get("dropout_apply", 0) == 1, cnt.calls
    assert cnt.calls.get("ln_bwd", 0) == 0, cnt.calls
    assert cnt.calls.get("ln_fwd", 0) == 0, cnt.calls
    assert cnt.calls.get("syncbn_stats", 0) == final_bias_sums, cnt.calls
    assert cnt.calls.get("ln_act_drop_fwd", 0) == 2, cnt.calls
    assert cnt.calls.get("ln_act_drop_bwd", 0) == 2, cnt.calls
    assert set(grads0) == set(grads1)
    for name, g0 in grads0.items():
        g1 = grads1[name]
        assert g0 is not None and g1 is not None, f"{name}: no gradient"
        assert g1.shape == g0.shape, name
        assert torch.isfinite(g1).all(), name
        bound_abs, n_terms = L.grad_bound(name, g0.shape, rec)
        bound = 2 * (n_terms + 8.0) * EPS * bound_abs.reshape(g0.shape)
        err = (g1.double() - g0.double()).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{model_name} {name}: max err/bound = {worst:.3g}")
        assert not (err > bound).any(), \
            f"{name}: fused and unfused gradients differ by {worst:.3g} bounds"
    if model_name == "graphsage":
        assert torch.equal(grads1["layers.1.linear1.bias"],
                           grads1["layers.1.linear2.bias"])
