"""Check functions for tests/test_gpu_gemm_tiled.py: the tiled 128x128 fp32
MFMA GEMM (ops/hip/gemm_tiled.hip), its split-K, the routing between it
and the 64x64 kernel, and the dropout fused into its operand staging.

Oracles are those of tests/dense_path_checks.py, imported: E (integer
operands, `torch.equal` the float64 product, every partial sum below
2^24), S (randn operands, kernel_path_checks.assert_sum_bound with
n_terms = the reduction length) and the host splitmix64 mask keep_mask /
inv_keep32. Inputs come from seeded CPU generators; no GPU kernel is ever
the reference.
"""
from __future__ import annotations

import numpy as np
import torch

import dense_path_checks as D
from kernel_path_checks import assert_sum_bound, cu, dbl, gen

# tile constants of gemm_tiled.hip and the `kernel` ids of the entry points
TBM = TBN = 128
TBK = 16
AUTO, OLD, TILED = 0, 1, 2

# one below / at / above the tile edge, a single row, and two tiles + tail
MN_EDGES = (1, TBM - 1, TBM, TBM + 1, 2 * TBM + 4)
# 4, one K-tile -4, one K-tile, one K-tile +4, four K-tiles + a tail
K_EDGES = (4, TBK - 4, TBK, TBK + 4, 4 * TBK + 4)


def _operands(layout, M, N, Kd, g, integer):
    """Tensors (a, b) as the entry point of `layout` takes them, plus the
    float64 [M,Kd] and [Kd,N] factors of the M x N result."""
    mk = (lambda *s: D.ints(s, g)) if integer else \
        (lambda *s: torch.randn(*s, generator=g))
    if layout == "nt":
        x, w = mk(M, Kd), mk(N, Kd)
        return x, w, dbl(x), dbl(w).t()
    if layout == "nn":
        gr, w = mk(M, Kd), mk(Kd, N)
        return gr, w, dbl(gr), dbl(w)
    gr, x = mk(Kd, M), mk(Kd, N)
    return gr, x, dbl(gr).t(), dbl(x)


def _call(layout, a, b, bias, kernel):
    ext = D._ext()
    if layout == "nt":
        return ext.gemm_nt_bias(cu(a), cu(b), cu(bias), kernel)
    assert bias is None
    fn = ext.gemm_nn if layout == "nn" else ext.gemm_tn
    return fn(cu(a), cu(b), kernel)


def check_gemm(layout, M, N, Kd, integer, bias=False, kernel=TILED, seed=0):
    """One M x N GEMM with inner dimension Kd through the public entry
    point with the given kernel id: E for integer operands (bias in {1, 2},
    so a bias added once per split-K slice shows), S for randn ones."""
    g = gen(8100 + seed + 13 * M + 7 * N + Kd)
    a, b, a64, b64 = _operands(layout, M, N, Kd, g, integer)
    bv = None
    if bias:
        bv = D.ints((N,), g, 1, 2) if integer else torch.randn(N, generator=g)
    want, want_abs = a64 @ b64, a64.abs() @ b64.abs()
    if bias:
        want, want_abs = want + dbl(bv), want_abs + dbl(bv).abs()
    got = _call(layout, a, b, bv, kernel)
    what = f"gemm_{layout}[kernel {kernel}] {M}x{N} inner {Kd} bias={bias}"
    if integer:
        D.assert_exact(got, want, want_abs, what + " [E]")
    else:
        assert_sum_bound(got, want, want_abs, float(Kd), what + " [S]")


# -------------------------------------------------------- fused dropout

def dropped64(x, keep, seed):
    """float64 dropout(x) with the kernels' mask and fp32 scale: element
    (m, k) of the [M, K] operand has flat index m*K + k."""
    idx = np.arange(x.numel(), dtype=np.int64)
    mask = D.keep_mask(idx, keep, seed).reshape(tuple(x.shape))
    scale = float(D.inv_keep32(keep))
    return dbl(x) * torch.from_numpy(mask).double() * scale, mask


def check_fused_dropout(M, K, N, keep, seed, integer=True):
    """gemm_nt_bias_drop and gemm_tn_drop against the float64 products of
    the host-masked operand. With integer x in [-2, 2] and keep = 0.5 the
    scale 2 is exact and both must be torch.equal (E)."""
    ext = D._ext()
    g = gen(8300 + M + K + N)
    mk = (lambda *s: D.ints(s, g)) if integer else \
        (lambda *s: torch.randn(*s, generator=g))
    x, w, gy = mk(M, K), mk(N, K), mk(M, N)
    b = D.ints((N,), g, 1, 2) if integer else torch.randn(N, generator=g)
    xd, mask = dropped64(x, keep, seed)
    if float(np.float32(keep)) < 1.0:
        assert 0 < int(mask.sum()) < mask.size
    else:
        assert mask.all()
    y = ext.gemm_nt_bias_drop(cu(x), cu(w), cu(b), keep, seed)
    dw = ext.gemm_tn_drop(cu(gy), cu(x), keep, seed)
    tag = f"fused dropout {M}x{K}->{N} keep={keep} seed={seed}"
    y_want = xd @ dbl(w).t() + dbl(b)
    y_abs = xd.abs() @ dbl(w).abs().t() + dbl(b).abs()
    dw_want, dw_abs = dbl(gy).t() @ xd, dbl(gy).abs().t() @ xd.abs()
    if integer:
        D.assert_exact(y, y_want, y_abs, tag + " y [E]")
        D.assert_exact(dw, dw_want, dw_abs, tag + " dW [E]")
    else:
        assert_sum_bound(y, y_want, y_abs, float(K), tag + " y [S]")
        assert_sum_bound(dw, dw_want, dw_abs, float(M), tag + " dW [S]")


def run_dropout_linear(fused, x, w, b, gy, p, torch_seed, x_grad=False):
    """(y, dW, db, dx) of dropout_linear (fused=True) or of the unfused
    linear(dropout(x)) on the GPU under the same torch seed."""
    from bnsgcn_amd.ops import functional as BF
    xg = cu(x).requires_grad_(x_grad)
    wg, bg = cu(w).requires_grad_(True), cu(b).requires_grad_(True)
    torch.manual_seed(torch_seed)
    if fused:
        y = BF.dropout_linear(xg, wg, bg, p, True)
    else:
        y = BF.linear(BF.dropout(xg, p, True), wg, bg)
    y.backward(cu(gy))
    return y.detach(), wg.grad, bg.grad, xg.grad


def drawn_seed(torch_seed):
    torch.manual_seed(torch_seed)
    return int(torch.randint(0, 2**62, (1,)).item())
