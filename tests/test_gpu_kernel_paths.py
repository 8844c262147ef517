"""GPU (MI355X) numerics for the kernel paths test_gpu.py never reaches:
scalar / second-feature-pass forms, split (atomic) work-list items, rows
longer than one wave pass, empty rows, the union softmax's shared max,
the D % 4 != 0 attention projection, zero-row launches and the variants
behind environment switches.

Oracle and tolerances: see tests/kernel_path_checks.py — float64
ops/reference.py on the same fp32 inputs, the any-order summation bound
for sum-type kernels, the project's rtol=1e-4/atol=1e-5 for softmax.

Run on the GPU box: python -m pytest tests/test_gpu_kernel_paths.py -m gpu -x -q
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_path_checks as K
from kernel_path_checks import DEV, N_COLS, N_COLS2, N_ROWS, cu, dbl, gen

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bnsgcn_amd.ops._ext import require_ext
    ext = require_ext()
else:
    ext = None

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

from bnsgcn_amd.ops.philox import bns_keys

# (H, D): (4,41) (2,7) (3,5) scalar spmm_edge + gen sddmm_dot; (4,128)
# (1,64) vec4 + fast; (8,128) vec4 second feature pass (H*D/4 = 256 > 128)
# + vec4 sddmm_dot (H*D > 512); (4,100) vec4 + vec4
GAT_SHAPES = [(4, 41), (2, 7), (3, 5), (4, 128), (8, 128), (1, 64), (4, 100)]


# ------------------------------------------------------------- spmm_sum

@needs_gpu
@pytest.mark.parametrize("F", [128, 64, 256, 602, 17, 257, 1032])
def test_spmm_sum_fixture(F):
    """vec4 half-wave (F=64,128), vec4 full-wave (256), vec4 second
    feature pass (1032: F/4 > 128), vec2 (602), scalar (17) and scalar
    second pass (257 > 256) on the fixture CSR: empty rows, rows of
    64/65/128/512 edges and 5 split items combined by atomicAdd.

    The out=None call follows the allocation and release of a NaN-filled
    tensor of the output's size, which the caching allocator is likely to
    hand back to the op's torch.empty — a best-effort probe (nothing
    forces the allocator to reuse the block) that the rows the kernel
    does not write are cleared."""
    K.check_spmm_sum(F, scales=True, acc=False, nan_prefill=True)
    K.check_spmm_sum(F, scales=False, acc=False, nan_prefill=True)
    K.check_spmm_sum(F, scales=False, acc=True)
    K.check_spmm_sum(F, scales=True, acc=True)


# ------------------------------------------------------- GAT kernel set

@needs_gpu
@pytest.mark.parametrize("H,D", GAT_SHAPES)
def test_spmm_edge_fixture(H, D):
    """spmm_edge_raw with/without out=, and with wperm on the transposed
    CSR (as _SpMMEdge.backward calls it; its hub column is a split row)."""
    K.check_spmm_edge(H, D)


@needs_gpu
@pytest.mark.parametrize("H,D", GAT_SHAPES)
def test_sddmm_dot_fixture(H, D):
    K.check_sddmm_dot(H, D)


@needs_gpu
@pytest.mark.parametrize("H", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("slope", [-1.0, 0.2])
def test_sddmm_add_fixture(H, slope):
    K.check_sddmm_add(H, slope)


@needs_gpu
@pytest.mark.parametrize("H", [1, 2, 3, 4, 8])
def test_segment_softmax_fixture(H):
    """Single-set softmax + backward with segments of 65..1300 edges (the
    `e += WAVE` loops take up to 21 trips)."""
    K.check_segment_softmax(H)


@needs_gpu
@pytest.mark.parametrize("H", [1, 2, 3, 4, 8])
def test_segment_sum_edges_fixture(H):
    """Generic H <= 8 form (H != 4) and the float4 form (H == 4), without
    perm on the forward CSR and with eperm on the transposed one."""
    K.check_segment_sum_edges(H)


# -------------------------------------------------------- union softmax

@needs_gpu
@pytest.mark.parametrize("H", [4, 3, 1, 8, 16, 32])
def test_segment_softmax2_shifted(H):
    """Union softmax + backward on two long-segment edge sets whose
    logits differ by +-90 per row: only the max over BOTH sets keeps
    fp32 exp finite. H = 4 is the float4 kernel, every other H the
    wave-per-(row, head) one."""
    K.check_softmax2(H)


@needs_gpu
@pytest.mark.parametrize("H", [4, 3])
def test_segment_softmax2_all_empty(H):
    K.check_softmax2_all_empty(H)


@needs_gpu
@pytest.mark.parametrize("H", [3, 8, 4])
def test_fused_attn_dropout_long_segments(H):
    """General-kernel (H != 4) and float4 (H == 4) dropout branches,
    forward and backward; the kept fraction must lie within
    5*sqrt(keep*(1-keep)/N) of keep (binomial standard deviation)."""
    K.check_softmax2_dropout(H)


# --------------------------------------------------------- attn_project

def _attn_project_case(H, D, n):
    K.check_attn_project(H, D, n)       # shared with the sparse sweep


@needs_gpu
@pytest.mark.parametrize("H,D", [(4, 41), (4, 47), (4, 7), (2, 6), (8, 3),
                                 (4, 128)])
def test_attn_project_unaligned_heads(H, D):
    """D % 4 != 0 with (H*D) % 4 == 0 — the GAT output layer (D =
    n_class): a float4 slot straddles two heads, so the head has to be
    derived per component. Forward and all three gradients."""
    _attn_project_case(H, D, 130)


@needs_gpu
def test_attn_project_zero_rows():
    _attn_project_case(4, 7, 0)
    torch.cuda.synchronize()


# ---------------------------------------------- composite GAT block grad

def _gat_block_plain(z_in, z_h, al, ar, csr1, csr2, slope=0.2):
    """The split GAT block in plain torch indexing + index_add (any
    dtype); autograd supplies the gradients."""
    (ip1, ix1), (ip2, ix2) = csr1, csr2
    n, H, D = N_ROWS, z_in.shape[1], z_in.shape[2]
    row1 = torch.repeat_interleave(torch.arange(n), ip1[1:] - ip1[:-1])
    row2 = torch.repeat_interleave(torch.arange(n), ip2[1:] - ip2[:-1])
    c1, c2 = ix1.long(), ix2.long()
    el_in, er = (z_in * al).sum(-1), (z_in * ar).sum(-1)
    el_h = (z_h * al).sum(-1)
    l1 = torch.nn.functional.leaky_relu(el_in[c1] + er[row1], slope)
    l2 = torch.nn.functional.leaky_relu(el_h[c2] + er[row2], slope)
    with torch.no_grad():             # the shift is a constant to autograd
        rows = torch.cat([row1, row2])[:, None].expand(-1, H)
        m = torch.full((n, H), float("-inf"), dtype=z_in.dtype)
        m = m.scatter_reduce(0, rows, torch.cat([l1, l2]), "amax")
    e1, e2 = torch.exp(l1 - m[row1]), torch.exp(l2 - m[row2])
    s = torch.zeros(n, H, dtype=z_in.dtype).index_add(0, row1, e1)
    s = s.index_add(0, row2, e2)
    a1, a2 = e1 / s[row1], e2 / s[row2]
    out = torch.zeros(n, H, D, dtype=z_in.dtype)
    out = out.index_add(0, row1, a1[:, :, None] * z_in[c1])
    out = out.index_add(0, row2, a2[:, :, None] * z_h[c2])
    return out


@needs_gpu
def test_gat_block_gradients_composite():
    """attn_project -> sddmm_add(slope=0.2) -> segment_softmax2 ->
    spmm_edge_sum2 from ops.functional at (H,D) = (4,7) on the two
    fixture edge sets, against the same mathematics in float64 torch
    autograd: output and the gradients w.r.t. z_in, z_h, attn_l, attn_r
    (wperm, eperm and the transposed halo CSR all exercised).

    Tolerance: the fp32 CPU run of the plain formulation is measured
    against float64 per tensor (max error / max magnitude); the GPU may
    use 8x that, floored at 1e-5 relative — it differs from the fp32 CPU
    run only in summation order, fast exp and atomics."""
    from bnsgcn_amd.ops import functional as BF
    from bnsgcn_amd.ops.csr_torch import transpose_csr
    H, D = 4, 7
    csr1, csr2 = K.fixture_csr(), K.fixture_csr2()
    g = gen(900)
    z_in = torch.randn(N_ROWS, H, D, generator=g)   # sources == dst rows
    z_h = torch.randn(N_COLS2, H, D, generator=g)
    al = torch.randn(1, H, D, generator=g)
    ar = torch.randn(1, H, D, generator=g)
    gout = torch.randn(N_ROWS, H, D, generator=g)
    leaves = (z_in, z_h, al, ar)
    names = ("out", "d z_in", "d z_h", "d attn_l", "d attn_r")

    def plain(dtype):
        ls = [t.clone().to(dtype).requires_grad_(True) for t in leaves]
        out = _gat_block_plain(*ls, csr1, csr2)
        (out * gout.to(dtype)).sum().backward()
        return [out.detach()] + [t.grad for t in ls]

    ref64, ref32 = plain(torch.float64), plain(torch.float32)

    ip, ix = cu(csr1[0]), cu(csr1[1])
    hip_, hix = cu(csr2[0]), cu(csr2[1])
    tip, tix, eperm = transpose_csr(ip, ix, N_ROWS)
    hbip, hbix, heperm = transpose_csr(hip_, hix, N_COLS2)
    inner5 = (ip, ix, tip, tix, eperm)
    halo5 = (hip_, hix, hbip, hbix, heperm)
    zi, zh, alg, arg = (cu(t).requires_grad_(True) for t in leaves)
    el_in, er = BF.attn_project(zi, alg, arg)
    el_h, _ = BF.attn_project(zh, alg, arg)
    li = BF.sddmm_add(el_in, er, *inner5, slope=0.2)
    lh = BF.sddmm_add(el_h, er, *halo5, slope=0.2)
    ai, ah = BF.segment_softmax2(li, lh, ip, hip_)
    out = BF.spmm_edge_sum2(zi, ai, zh, ah, inner5, halo5)
    (out * cu(gout)).sum().backward()
    got = [out.detach(), zi.grad, zh.grad, alg.grad, arg.grad]

    failures = []
    for name, g_, r64, r32 in zip(names, got, ref64, ref32):
        scale = float(r64.abs().max())
        e32 = float((r32.double() - r64).abs().max()) / scale
        egpu = float((g_.double().cpu() - r64).abs().max()) / scale
        tol = max(8 * e32, 1e-5)
        print(f"composite {name}: fp32-cpu rel err {e32:.3g}, "
              f"gpu rel err {egpu:.3g}, tol {tol:.3g}")
        assert torch.isfinite(g_).all(), name
        if not egpu <= tol:
            failures.append((name, egpu, tol))
    assert not failures, failures


# -------------------------------------------------------- zero-row ops

@needs_gpu
def test_zero_row_ops_launch_nothing():
    """n == 0 inputs (an empty halo / empty partition) must return the
    zero-initialised outputs without a zero-sized grid dimension, and
    leave no launch error pending for the next checked call."""
    from bnsgcn_amd.ops import functional as BF
    out = ext.syncbn_stats(torch.zeros(0, 24, device=DEV))
    assert torch.equal(out.cpu(), torch.zeros(2, 24))

    x = torch.zeros(0, 64, device=DEV, requires_grad=True)
    w = torch.randn(64, device=DEV, requires_grad=True)
    b = torch.randn(64, device=DEV, requires_grad=True)
    y = BF.layer_norm(x, w, b)
    assert y.shape == (0, 64)
    y.sum().backward()
    assert x.grad.shape == (0, 64)
    assert torch.equal(w.grad.cpu(), torch.zeros(64))
    assert torch.equal(b.grad.cpu(), torch.zeros(64))

    x = torch.zeros(0, 30, device=DEV, requires_grad=True)
    lw = torch.randn(16, 30, device=DEV, requires_grad=True)
    lb = torch.randn(16, device=DEV, requires_grad=True)
    y = BF.linear(x, lw, lb)
    assert y.shape == (0, 16)
    y.sum().backward()
    assert torch.equal(lb.grad.cpu(), torch.zeros(16))
    assert torch.equal(lw.grad.cpu(), torch.zeros(16, 30))

    torch.cuda.synchronize()
    assert float((torch.ones(8, device=DEV) * 2).sum()) == 16.0


# --------------------------------------------------------- smaller gaps

@needs_gpu
@pytest.mark.parametrize("n", [1, 200, 257])
@pytest.mark.parametrize("F", [24, 300])
def test_syncbn_stats_small_n_wide_f(n, F):
    """row_chunks == 1 (n <= 256: plain stores, no atomics), the first
    atomic size (257) and F > 256 (more than one column block)."""
    x = torch.randn(n, F, generator=gen(1000 + n + F))
    xd = dbl(x)
    want = torch.stack((xd.sum(0), (xd * xd).sum(0)))
    want_abs = torch.stack((xd.abs().sum(0), (xd * xd).sum(0)))
    got = ext.syncbn_stats(cu(x))
    K.assert_sum_bound(got, want, want_abs, float(n),
                       f"syncbn_stats n={n} F={F}")


@needs_gpu
@pytest.mark.parametrize("F", [1, 4, 30])
def test_pack_scatter_edges(F):
    """scale=None, n == 0 and all-equal indices (every scatter atomic
    lands on one row) at scalar and float4 widths."""
    from bnsgcn_amd.ops import reference as ref
    g = gen(1100 + F)
    x = torch.randn(40, F, generator=g)
    for idx in (torch.randint(0, 40, (70,), generator=g),
                torch.full((70,), 7, dtype=torch.long),
                torch.zeros(0, dtype=torch.long)):
        n = idx.numel()
        for scale in (None, torch.rand(n, generator=g) + 0.5):
            got = ext.pack_rows(cu(x), cu(idx), cu(scale))
            assert torch.equal(got.cpu(), ref.pack_rows(x, idx, scale))
            src = torch.randn(n, F, generator=g)
            base = torch.randn(40, F, generator=g)
            want = ref.scatter_add_rows(dbl(base).clone(), idx, dbl(src),
                                        dbl(scale))
            want_abs = ref.scatter_add_rows(dbl(base).abs(), idx,
                                            dbl(src).abs(), dbl(scale))
            out = cu(base).clone()
            ext.scatter_add_rows(out, cu(idx), cu(src), cu(scale))
            n_terms = torch.bincount(idx, minlength=40).double()[:, None]
            K.assert_sum_bound(out, want, want_abs, n_terms,
                               f"scatter_add_rows F={F} n={n}")


@needs_gpu
@pytest.mark.parametrize("seed", [2**40 + 12345, 2**62 - 1])
def test_philox_keys_wide_seed_epoch_ranks(seed):
    """seed_hi != 0, epoch above 2^31 and both rank halves at their
    16-bit limit, bitwise against the numpy implementation."""
    epoch = 2**31 + 5
    for (s, d) in ((0, 65535), (65535, 1)):
        for n in (1, 255, 256, 257):
            want = bns_keys(n, seed, epoch, s, d)
            got = ext.philox_keys(n, seed, epoch, s, d).cpu().numpy()
            np.testing.assert_array_equal(got, want)


@needs_gpu
def test_gemm_k_below_tile():
    """K = 5 < BK = 32: a single, mostly zero-padded K tile, all three
    layouts, against a float64 matmul with the summation bound."""
    M, N, Kd = 70, 33, 5
    g = gen(1200)
    x = torch.randn(M, Kd, generator=g)
    w = torch.randn(N, Kd, generator=g)
    b = torch.randn(N, generator=g)
    gr = torch.randn(M, N, generator=g)
    xd, wd, bd, gd = dbl(x), dbl(w), dbl(b), dbl(gr)
    K.assert_sum_bound(ext.gemm_nt_bias(cu(x), cu(w), cu(b)),
                       xd @ wd.t() + bd, xd.abs() @ wd.abs().t() + bd.abs(),
                       float(Kd), "gemm_nt_bias K=5")
    K.assert_sum_bound(ext.gemm_nn(cu(gr), cu(w)), gd @ wd,
                       gd.abs() @ wd.abs(), float(N), "gemm_nn K=5")
    K.assert_sum_bound(ext.gemm_tn(cu(gr), cu(x)), gd.t() @ xd,
                       gd.abs().t() @ xd.abs(), float(M), "gemm_tn K=5")


# ------------------------------------------- work-list host-side check

@needs_gpu
def test_worklist_entry_points_reject_12_waves():
    """Every work-list entry point sizes its grid as n_waves / (waves per
    block), so a wave_start of 13 entries (12 waves, not a multiple of 8)
    must raise on the host before anything is launched. The 12-wave
    schedule itself is well formed (monotone, ends at the item count)."""
    from bnsgcn_amd.ops.csr_torch import build_worklist
    n, H, D = 20, 4, 8
    rng = np.random.default_rng(1300)
    ip, ix = K._csr_from_degrees(rng.integers(0, 6, n), n, rng)
    ip, ix = cu(ip), cu(ix)
    wrow, wbeg, wend, wstart, _ = build_worklist(ip)
    assert (wstart.numel() - 1) % 8 == 0
    bad = torch.linspace(0, wrow.numel(), 13).to(torch.int32).to(DEV)
    assert bad.numel() == 13 and int(bad[-1]) == wrow.numel()
    wl = (wrow, wbeg, wend, bad)
    E = ix.numel()
    x2 = torch.randn(n, D, device=DEV)
    x3 = torch.randn(n, H, D, device=DEV)
    eh = torch.randn(E, H, device=DEV)
    nh = torch.randn(n, H, device=DEV)
    calls = {
        "spmm_sum": lambda: ext.spmm_sum(*wl, ix, x2, None, None,
                                         torch.zeros_like(x2), False),
        "sddmm_add": lambda: ext.sddmm_add(*wl, ip, ix, nh, nh, 0.2),
        "spmm_edge_sum": lambda: ext.spmm_edge_sum(
            *wl, ip, ix, eh, None, x3, torch.zeros_like(x3), False),
        "sddmm_dot": lambda: ext.sddmm_dot(*wl, ip, ix, x3, x3),
        "segment_sum_edges": lambda: ext.segment_sum_edges(*wl, None, eh, n),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="multiple of 8"):
            call()
    torch.cuda.synchronize()


# ------------------------------------- environment-gated kernel variants

@needs_gpu
def test_env_gated_variants_in_child_processes():
    """BNSGCN_SPMM_SUBW32_MAX=0 (narrow F through the 64-wide kernel, F in
    {64,128}). The extension reads each switch once per process, so every
    variant runs in a fresh child — one at a time, and none is started
    after one that failed, timed out or died on a signal."""
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "kernel_path_checks.py")
    for case, (env_add, _) in K.CASES.items():
        env = dict(os.environ, **env_add)
        r = subprocess.run([sys.executable, helper, case], env=env,
                           timeout=180, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        print(r.stdout)
        assert r.returncode == 0, (
            f"child '{case}' exited {r.returncode}:\n{r.stdout[-4000:]}")
