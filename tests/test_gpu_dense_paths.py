"""GPU (MI355X) checks of the dense and elementwise kernels — the fp32
MFMA GEMM with deep split-K, LayerNorm forward/backward, the mask-free
dropout and the fused attention dropout — and of every capped launch
beyond its clamp, where a grid-stride loop has to wrap.

Oracles (tests/dense_path_checks.py): E = exact integer arithmetic, S =
the any-order summation bound against float64, M = 8x the measured
fp32-CPU error against float64. Inputs come from seeded CPU generators;
no GPU kernel is ever the reference.

Run on the GPU box: python -m pytest tests/test_gpu_dense_paths.py -m gpu -x -q
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dense_path_checks as D
from kernel_path_checks import DEV, cu

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bnsgcn_amd.ops._ext import require_ext
    ext = require_ext()
else:
    ext = None

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

LAYOUTS = ("nt", "nn", "tn")


# ----------------------------------------------------------------- GEMM

@needs_gpu
@pytest.mark.parametrize("inner", [128, 129, 257, 513])
def test_gemm_splitk_boundaries(inner):
    """70 x 33 output (two tiles). Inner dimension 128: no split (K <=
    4*BK); 129: splitk 1; 257: splitk 2 (k_slice 160, last slice 97);
    513: splitk 3 (k_slice 192, last slice 129). All three layouts, with
    bias and without, oracles E and S."""
    for layout in LAYOUTS:
        for integer in (True, False):
            D.check_gemm(layout, 70, 33, inner, integer)
    for integer in (True, False):
        D.check_gemm("nt", 70, 33, inner, integer, bias=True)


@needs_gpu
def test_gemm_tn_deep_splitk_one_tile():
    """gemm_tn(g[16400, 41], x[16400, 64]): one tile, splitk = 64,
    k_slice = 288, so only 57 z-slices are launched. E: |sums| <= 65,600."""
    D.check_gemm("tn", 41, 64, 16400, integer=True)
    D.check_gemm("tn", 41, 64, 16400, integer=False)


@needs_gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gemm_deep_splitk_multi_tile(layout):
    """192 x 250 output (3 x 4 tiles, an N tail of 58), inner dimension
    16400: splitk = 64 over 12 tiles."""
    D.check_gemm(layout, 192, 250, 16400, integer=True,
                 bias=(layout == "nt"))


@needs_gpu
@pytest.mark.parametrize("M", [960, 961])
def test_gemm_base_blocks_255_vs_272(M):
    """960 x 1088 is 15 x 17 = 255 tiles (splitk = 3, atomic epilogue),
    961 x 1088 is 272 tiles (no split, plain stores); inner dimension
    700. The bias must appear exactly once in both."""
    D.check_gemm("nt", M, 1088, 700, integer=True, bias=True)
    D.check_gemm("nt", M, 1088, 700, integer=True, bias=False)
    D.check_gemm("nn", M, 1088, 700, integer=True)
    D.check_gemm("tn", M, 1088, 700, integer=True)


@needs_gpu
def test_gemm_minimal_outputs():
    """1 x 1 output with a K tail (K = 130) through gemm_nt_bias, and a
    1-row output through the NN staging layout (g[1, 200])."""
    D.check_gemm("nt", 1, 1, 130, integer=True, bias=True)
    D.check_gemm("nt", 1, 1, 130, integer=True, bias=False)
    D.check_gemm("nn", 1, 33, 200, integer=True)


@needs_gpu
@pytest.mark.parametrize("M,Kd,N", D.LINEAR_SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_linear_autograd_default_route(M, Kd, N, bias):
    """BF.linear as the models call it (dW through gemm_tn, the bias
    gradient through syncbn_stats): y, dx, dW, db with oracle S."""
    D.check_linear(M, Kd, N, bias)


@needs_gpu
def test_linear_autograd_hip_route_in_child_process():
    """BNSGCN_GEMM=hip (forward and dx through the MFMA GEMM too) is read
    at import of ops/functional.py, so it runs in a fresh child — one at
    a time, none started after one that failed, timed out or died."""
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "dense_path_checks.py")
    for case, (env_add, _) in D.CASES.items():
        env = dict(os.environ, **env_add)
        r = subprocess.run([sys.executable, helper, case], env=env,
                           timeout=180, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        print(r.stdout)
        assert r.returncode == 0, (
            f"child '{case}' exited {r.returncode}:\n{r.stdout[-4000:]}")


# ------------------------------------------------------------ LayerNorm

@needs_gpu
@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("F", [3, 4, 8, 63, 64, 65, 252, 256, 260, 1020,
                               1023, 1024])
def test_layer_norm_small_shapes(F, act):
    """F below 64 (most lanes idle), F and F/4 on either side of 64, the
    register limit (1020..1024); n = 67 (n % 4 = 3, one row chunk: plain
    stores in ln_bwd_w) and n = 257 (first atomic size). M on y, mean,
    rstd, dx; S on dgamma, dbeta."""
    for n in (67, 257):
        D.check_layer_norm_small(n, F, act)


@needs_gpu
@pytest.mark.parametrize("act", [False, True])
def test_layer_norm_large_row_mean(act):
    """x = 100 + randn: passes only if the variance is taken about the
    mean (E[x^2] - mean^2 loses every digit in fp32)."""
    D.check_layer_norm_small(67, 64, act, offset=100.0)


@needs_gpu
@pytest.mark.parametrize("n,F", [(67, 64), (257, 65)])
@pytest.mark.parametrize("act", [False, True])
def test_layer_norm_autograd(n, F, act):
    D.check_layer_norm_autograd(n, F, act)


@needs_gpu
def test_layer_norm_wide_falls_back_to_torch():
    """F = 1028 > 1024 is outside the kernels' register budget."""
    D.check_layer_norm_autograd(67, 1028, True)


@needs_gpu
@pytest.mark.parametrize("n,F,act", [(524300, 12, True), (524300, 12, False),
                                     (131077, 13, True), (131077, 13, False)])
def test_layer_norm_wrapped_rows(n, F, act):
    """(524300, 12): float4 kernels, four full passes of the 131,072-row
    grid and a fifth of 12 rows, ln_bwd_w with 2048 chunks of 257 rows.
    (131077, 13): scalar kernels, a second pass of 5 rows."""
    D.check_layer_norm_large(n, F, act)


# -------------------------------------------------------------- dropout

SEEDS = [0, 12345, 2**40 + 7, 2**62 - 1]


@needs_gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_dropout_mask_matches_host(seed):
    """Scalar (n % 4 != 0) and float4 forms at 1..1027 elements, bit for
    bit; the 1027-element mask equals the head of the 1028-element one
    (the two forms draw the same mask)."""
    for keep in (0.7, 0.25):
        for n in (1, 3, 4, 1023, 1024):
            D.check_dropout_exact(n, keep, seed)
        m_scalar = D.check_dropout_exact(1027, keep, seed)
        m_vec4 = D.check_dropout_exact(1028, keep, seed)
        assert torch.equal(m_scalar, m_vec4[:1027])


@needs_gpu
def test_dropout_wrapped_scalar():
    """8,388,611 elements: three past the 32768 x 256 threads of one pass."""
    D.check_dropout_exact(8_388_611, 0.7, 2**40 + 7)


@needs_gpu
def test_dropout_wrapped_vec4():
    """33,554,436 elements: one float4 past one pass (134 MB in and out)."""
    D.check_dropout_exact(33_554_436, 0.7, 12345)


@needs_gpu
@pytest.mark.parametrize("n", [1027, 1028])
def test_dropout_autograd_seed_from_torch(n):
    D.check_dropout_autograd(n, 0.3, 77)


@needs_gpu
@pytest.mark.parametrize("n", [1027, 1028])
def test_dropout_keep_rounds_to_one(n):
    """keep = 1 - 1e-9 is 1.0f in the kernel: every element kept, scale
    exactly 1 (2^32 does not fit the uint32 threshold)."""
    keep = 1 - 1e-9
    assert keep < 1.0 and float(np.float32(keep)) == 1.0
    x = torch.rand(n, generator=D.gen(9900 + n)) + 0.5
    for seed in SEEDS:
        got = ext.dropout_apply(cu(x), keep, seed).cpu()
        assert torch.equal(got, x), int((got != x).sum())


@needs_gpu
@pytest.mark.parametrize("n", [1027, 1028])
def test_dropout_p_one_gives_zeros(n):
    from bnsgcn_amd.ops import functional as BF
    x = (torch.rand(n, generator=D.gen(9950 + n)) + 0.5).to(DEV)
    x.requires_grad_(True)
    y = BF.dropout(x, 1.0, True)
    y.backward(torch.ones_like(y))
    assert torch.equal(y.detach().cpu(), torch.zeros(n))
    assert torch.equal(x.grad.cpu(), torch.zeros(n))


# ---------------------------------------------- fused attention dropout

@needs_gpu
@pytest.mark.parametrize("H", [4, 3, 8])
def test_fused_attn_dropout_mask_matches_host(H):
    """float4 (H = 4) and general (H = 3, 8) kernels."""
    D.check_softmax2_dropout_seeded(H)
    D.check_softmax2_dropout_seeded(H, keep=0.5, seed=2**62 - 1)


@needs_gpu
@pytest.mark.parametrize("H", [4, 3, 8])
def test_fused_attn_dropout_keep_rounds_to_one(H):
    """keep = 1 - 1e-9 is below 1 as a double and 1.0f in the kernel: the
    launcher must not hand out separate da1/da2 that no kernel writes."""
    D.check_softmax2_keep_rounds_to_one(H)


# ------------------------------------------------------ wrapped launches

@needs_gpu
@pytest.mark.parametrize("n,F", [(8200, 516), (4099, 257)])
def test_pack_scatter_wrapped(n, F):
    """float4 form (8200 x 129 = 1,057,800 slots) and scalar form (4099 x
    257 = 1,053,443) beyond the 1,048,576 threads of the clamped grid."""
    D.check_pack_scatter_wrapped(n, F)


@needs_gpu
def test_bincount_wrapped():
    """1,100,000 values in 150 bins, a quarter of them in one bin."""
    D.check_bincount_wrapped()


@needs_gpu
@pytest.mark.parametrize("n,F", [(1_000_000, 2), (600_001, 3)])
def test_syncbn_stats_wrapped(n, F):
    """n = 1,000,000: 2048 chunks of 489 rows, the last three start beyond
    n. n = 600,001: 293 rows per chunk."""
    D.check_syncbn_stats_wrapped(n, F)


@needs_gpu
@pytest.mark.parametrize("n,H,D_", [(65600, 4, 8), (65600, 4, 7),
                                    (524300, 1, 4)])
def test_attn_project_wrapped(n, H, D_):
    """Aligned and straddling forms beyond 65,536 waves; (524300, 1, 4)
    drives the dattn kernel with 2048 chunks (sums <= 2.1M)."""
    D.check_attn_project_wrapped(n, H, D_)


@needs_gpu
def test_segment_softmax_wrapped():
    D.check_softmax_wrapped(22000, 3)


@needs_gpu
@pytest.mark.parametrize("n_rows,H,form", [(22000, 3, "general"),
                                           (8200, 8, "general"),
                                           (262150, 4, "h4")])
def test_segment_softmax2_wrapped(n_rows, H, form):
    D.check_softmax2_wrapped(n_rows, H, form)


@needs_gpu
def test_spmm_edge_scalar_wrapped():
    D.check_spmm_edge_scalar_wrapped()
