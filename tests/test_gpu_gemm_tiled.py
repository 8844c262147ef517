"""GPU (MI355X) checks of the tiled 128x128 fp32 MFMA GEMM, its split-K,
the routing between it and the 64x64 kernel, the dropout fused into its
operand load and ops.functional.dropout_linear.

Oracles (tests/dense_path_checks.py, through tests/gemm_tiled_checks.py):
E = exact integer arithmetic, S = the any-order summation bound against
float64, and the host splitmix64 mask. No GPU kernel is ever the
reference. The tiled kernel is forced (kernel id 2) except where the
routing itself is under test.

Run on the GPU box: python -m pytest tests/test_gpu_gemm_tiled.py -m gpu -x -q
"""
import pytest
import torch

import dense_path_checks as D
import gemm_tiled_checks as T
from kernel_path_checks import assert_sum_bound, cu, dbl, gen

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

LAYOUTS = ("nt", "nn", "tn")


# ------------------------------------------------------------ tile edges

@needs_gpu
@pytest.mark.parametrize("inner", T.K_EDGES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_tile_edges(layout, inner):
    """M, N in {1, 127, 128, 129, 260} and the inner dimension in {4, 12,
    16, 20, 68} (K-tile 16), E and S, 'nt' with bias and without. Sizes
    that are no multiple of 4 in an operand's contiguous dimension take the
    kernel's scalar staging, the others its float4 staging."""
    for M in T.MN_EDGES:
        for N in T.MN_EDGES:
            for integer in (True, False):
                T.check_gemm(layout, M, N, inner, integer)
                if layout == "nt":
                    T.check_gemm(layout, M, N, inner, integer, bias=True)


@needs_gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_tile_edges_unaligned_inner(layout):
    """Inner dimensions 18 and 41 (not multiples of 4): the scalar staging
    with a K tail inside a float4 slot."""
    for inner in (18, 41):
        for M, N in ((129, 127), (128, 260)):
            for integer in (True, False):
                T.check_gemm(layout, M, N, inner, integer,
                             bias=(layout == "nt"))


# --------------------------------------------------------------- split-K

@needs_gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_splitk_one_tile(layout):
    """One output tile, inner dimension 16400: 114 slices of 144. 16404:
    the last slice holds 132 = 8 K-tiles + 4. E (integer bias in {1, 2}
    for 'nt': it must appear once) and S."""
    for inner in (16400, 16404):
        for integer in (True, False):
            T.check_gemm(layout, 64, 40, inner, integer,
                         bias=(layout == "nt"))


@needs_gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_splitk_multi_tile(layout):
    """192 x 252 output (2 x 2 tiles with tails), inner dimension 16400
    and 16396 (a slice length that does not divide it)."""
    for inner in (16400, 16396):
        T.check_gemm(layout, 192, 252, inner, True, bias=(layout == "nt"))
    T.check_gemm(layout, 192, 252, 16400, False, bias=(layout == "nt"))


# --------------------------------------------------------------- routing

@needs_gpu
def test_routing_refused_shapes_stay_exact():
    """Shapes the float4 fast path must refuse, through the public entry
    points with the default routing: inner dimension 130, and a 41-wide
    contiguous dimension in each layout. All still E-exact."""
    T.check_gemm("nt", 300, 256, 130, True, bias=True, kernel=T.AUTO)
    T.check_gemm("nn", 300, 256, 41, True, kernel=T.AUTO)   # g[300,41] w[41,256]
    T.check_gemm("tn", 41, 256, 300, True, kernel=T.AUTO)   # g[300,41] x[300,256]
    T.check_gemm("nn", 300, 41, 256, True, kernel=T.AUTO)   # w[256,41]
    T.check_gemm("nt", 300, 41, 256, True, bias=True, kernel=T.AUTO)


@needs_gpu
@pytest.mark.parametrize("kernel", [T.AUTO, T.OLD, T.TILED])
def test_every_kernel_id_same_result(kernel):
    """An aligned multi-tile shape through each kernel id, E."""
    for layout in LAYOUTS:
        T.check_gemm(layout, 260, 384, 132, True, bias=(layout == "nt"),
                     kernel=kernel)


@needs_gpu
def test_bad_kernel_id_raises():
    x = torch.ones(8, 8, device="cuda")
    with pytest.raises(RuntimeError):
        D._ext().gemm_nn(x, x, 3)


# ------------------------------------------------ headline shapes, scaled

@needs_gpu
@pytest.mark.parametrize("M,K,N", [(700, 1204, 256), (700, 256, 44)])
def test_linear_autograd_headline_shapes(M, K, N):
    """BF.linear under autograd at the benchmark's layer shapes with 700
    rows: S on forward, dx, dW and db."""
    D.check_linear(M, K, N, bias=True)


# --------------------------------------------------------- fused dropout

@needs_gpu
@pytest.mark.parametrize("seed", [12345, 2**40 + 7])
@pytest.mark.parametrize("M,K", [(130, 36), (257, 1204)])
def test_fused_dropout_exact(M, K, seed):
    """Integer x in [-2, 2], keep = 0.5 (scale 2 exact): forward and dW
    torch.equal the float64 product with the host mask of m*K + k."""
    for N in (33, 256):
        T.check_fused_dropout(M, K, N, 0.5, seed)


@needs_gpu
@pytest.mark.parametrize("keep", [1.0, 1.0 - 1e-9])
def test_fused_dropout_keep_one(keep):
    """keep = 1 and a keep that rounds to 1.0f: a plain GEMM."""
    T.check_fused_dropout(130, 36, 33, keep, 99)
    T.check_fused_dropout(257, 1204, 256, keep, 2**40 + 7)


@needs_gpu
def test_fused_dropout_randn():
    T.check_fused_dropout(257, 1204, 256, 0.7, 2**40 + 7, integer=False)


# -------------------------------------------- dropout_linear vs unfused

def _dl_operands(M, K, N, integer):
    g = gen(8600 + M + K + N)
    mk = (lambda *s: D.ints(s, g)) if integer else \
        (lambda *s: torch.randn(*s, generator=g))
    return mk(M, K), mk(N, K), mk(N), mk(M, N)


@needs_gpu
@pytest.mark.parametrize("M,K,N", [(130, 36, 33), (257, 1204, 256)])
def test_dropout_linear_bit_equal_to_unfused(M, K, N):
    """Same torch seed, integer operands, p = 0.5: forward, dW and db are
    bit-equal to linear(dropout(x)), and equal the host-mask product."""
    x, w, b, gy = _dl_operands(M, K, N, True)
    fused = T.run_dropout_linear(True, x, w, b, gy, 0.5, 4321)
    plain = T.run_dropout_linear(False, x, w, b, gy, 0.5, 4321)
    for name, a, c in zip(("y", "dW", "db"), fused, plain):
        assert torch.equal(a, c), f"{name} differs from the unfused path"
    assert fused[3] is None
    xd, _ = T.dropped64(x, 0.5, T.drawn_seed(4321))
    D.assert_exact(fused[0], xd @ dbl(w).t() + dbl(b),
                   xd.abs() @ dbl(w).abs().t() + dbl(b).abs(), "y [E]")
    D.assert_exact(fused[1], dbl(gy).t() @ xd, dbl(gy).abs().t() @ xd.abs(),
                   "dW [E]")


@needs_gpu
def test_dropout_linear_randn_within_sum_bound():
    M, K, N = 257, 1204, 256
    x, w, b, gy = _dl_operands(M, K, N, False)
    y, dw, db, _ = T.run_dropout_linear(True, x, w, b, gy, 0.3, 77)
    xd, _ = T.dropped64(x, 0.7, T.drawn_seed(77))
    assert_sum_bound(y, xd @ dbl(w).t() + dbl(b),
                     xd.abs() @ dbl(w).abs().t() + dbl(b).abs(), float(K), "y")
    assert_sum_bound(dw, dbl(gy).t() @ xd, dbl(gy).abs().t() @ xd.abs(),
                     float(M), "dW")
    assert_sum_bound(db, dbl(gy).sum(0), dbl(gy).abs().sum(0), float(M), "db")


@needs_gpu
def test_dropout_linear_falls_back_when_x_needs_grad():
    """x.requires_grad: the unfused composition runs, and dx (with y, dW,
    db) equals linear(dropout(x)) bit for bit under the same seed."""
    x, w, b, gy = _dl_operands(130, 36, 33, True)
    fused = T.run_dropout_linear(True, x, w, b, gy, 0.5, 555, x_grad=True)
    plain = T.run_dropout_linear(False, x, w, b, gy, 0.5, 555, x_grad=True)
    assert fused[3] is not None
    for name, a, c in zip(("y", "dW", "db", "dx"), fused, plain):
        assert torch.equal(a, c), f"{name} differs from the unfused path"
    xd, mask = T.dropped64(x, 0.5, T.drawn_seed(555))
    want_dx = (dbl(gy) @ dbl(w)) * torch.from_numpy(mask).double() * 2.0
    assert torch.equal(fused[3].double().cpu(), want_dx)


@needs_gpu
def test_dropout_linear_eval_and_p_zero_are_plain_linear():
    from bnsgcn_amd.ops import functional as BF
    x, w, b, _ = _dl_operands(130, 36, 33, True)
    want = dbl(x) @ dbl(w).t() + dbl(b)
    state = torch.random.get_rng_state()
    for p, training in ((0.5, False), (0.0, True)):
        y = BF.dropout_linear(cu(x), cu(w), cu(b), p, training)
        assert torch.equal(y.double().cpu(), want)
    assert torch.equal(torch.random.get_rng_state(), state), "a seed was drawn"
