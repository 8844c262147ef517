"""Shared fixtures and check functions for tests/test_gpu_kernel_paths.py.

Every check runs a HIP kernel on fp32 inputs and compares `got.double()`
with ops/reference.py evaluated on float64 copies of the SAME inputs
(never with another GPU kernel). Two tolerances, neither tuned on the
kernels' output:

* sum-type kernels: |got - ref64| <= (n_terms + 8) * 2^-23 * ref64_abs
  elementwise, where ref64_abs is the reference evaluated on the absolute
  values of all inputs and n_terms the length of that element's
  reduction — the any-order summation bound with a 2x margin for the
  fused scales / FMAs. An element whose ref64_abs is 0 (empty row) must
  be exactly 0.
* softmax kernels, their backwards and the dropout chain: the project's
  rtol=1e-4, atol=1e-5.

Run as a script (`python tests/kernel_path_checks.py CASE`) it executes
one environment-gated kernel variant in a fresh process — those switches
are read once per process by the extension — and exits non-zero on a
mismatch.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bnsgcn_amd.ops import reference as ref  # noqa: E402

DEV = "cuda:0"
EPS = 2.0 ** -23
N_ROWS, N_COLS, N_COLS2 = 96, 80, 50
HUB_COL = 3


# ------------------------------------------------------------- fixtures

def _csr_from_degrees(deg, n_cols, rng, hub_col=None, hub_p=0.0):
    indptr = np.zeros(len(deg) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(deg)
    e = int(indptr[-1])
    cols = rng.integers(0, n_cols, e)
    if hub_col is not None:
        cols = np.where(rng.random(e) < hub_p, hub_col, cols)
    return (torch.from_numpy(indptr),
            torch.from_numpy(cols.astype(np.int32)))


def fixture_csr():
    """96 x 80; every third row empty, the others degree 1..19, seven rows
    forced to 1300/64/65/128/512/513/1 (SEG=512 splits 1300 and 513 into 5
    atomic items; 64/65/128 sit on the wave-width boundaries). Column 3 is
    a hub (> 512 edges), so the TRANSPOSED CSR has a split row too."""
    rng = np.random.default_rng(20240)
    deg = rng.integers(1, 20, N_ROWS)
    deg[::3] = 0
    for r, d in {0: 1300, 5: 64, 9: 65, 20: 128, 33: 512, 50: 513,
                 95: 1}.items():
        deg[r] = d
    indptr, indices = _csr_from_degrees(deg, N_COLS, rng, HUB_COL, 0.25)
    assert int((deg == 0).sum()) == 29
    assert int((indices == HUB_COL).sum()) > 512
    return indptr, indices


def fixture_csr2():
    """Second edge set for the union softmax, same 96 rows x 50 columns:
    every fourth row empty, forced degrees 700/130/70/0. Rows 3, 6, ... are
    empty in set 1 only, rows 4, 8, ... in set 2 only, rows 12, 24, ... in
    both; row 6 is long in set 2 alone, row 0 long in both."""
    rng = np.random.default_rng(20241)
    deg = rng.integers(1, 10, N_ROWS)
    deg[::4] = 0
    for r, d in {6: 700, 0: 130, 20: 70, 5: 0}.items():
        deg[r] = d
    indptr, indices = _csr_from_degrees(deg, N_COLS2, rng)
    d1 = (fixture_csr()[0][1:] - fixture_csr()[0][:-1]).numpy()
    assert ((d1 == 0) & (deg > 0)).any() and ((d1 > 0) & (deg == 0)).any()
    assert ((d1 == 0) & (deg == 0)).any()
    return indptr, indices


def degrees(indptr):
    return (indptr[1:] - indptr[:-1]).double()


def cu(t):
    return None if t is None else t.to(DEV)


def dbl(t):
    return None if t is None else t.double()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------- assertions

def assert_sum_bound(got, ref64, ref64_abs, n_terms, what):
    """Elementwise any-order summation bound (module docstring). Returns
    the largest err/bound ratio."""
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    n_terms = torch.as_tensor(n_terms, dtype=torch.float64)
    bound = (n_terms + 8.0) * EPS * ref64_abs
    err = (got - ref64).abs()
    bad = err > bound
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.
    print(f"{what}: max err/bound = {worst:.3g}")
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} of {bad.numel()} elements over the bound; "
        f"max err {float(err.max()):.3e}, max err/bound {worst:.3g}")
    return worst


def assert_softmax_close(got, ref64, what):
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    if got.numel():
        print(f"{what}: max abs err = {float((got - ref64).abs().max()):.3g}")
    torch.testing.assert_close(got, ref64, rtol=1e-4, atol=1e-5, msg=lambda m:
                               f"{what}: {m}")


# ------------------------------------------------------------- spmm_sum

def check_spmm_sum(F, scales, acc, nan_prefill=False):
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    indptr, indices = fixture_csr()
    g = gen(100 + F)
    x = torch.randn(N_COLS, F, generator=g)
    ss = torch.rand(N_COLS, generator=g) + 0.5 if scales else None
    ds = torch.rand(N_ROWS, generator=g) + 0.5 if scales else None
    base = torch.randn(N_ROWS, F, generator=g) if acc else None
    want = ref.spmm_sum(indptr, indices, dbl(x), dbl(ss), dbl(ds),
                        dbl(base).clone() if acc else None)
    want_abs = ref.spmm_sum(indptr, indices, dbl(x).abs(), dbl(ss), dbl(ds),
                            dbl(base).abs() if acc else None)
    ip, ix = cu(indptr), cu(indices)
    if nan_prefill and not acc:
        junk = torch.full((N_ROWS, F), float("nan"), device=DEV)
        torch.cuda.synchronize()
        del junk
    got = spmm_sum_raw(ip, ix, cu(x), cu(ss), cu(ds),
                       cu(base).clone() if acc else None)
    what = f"spmm_sum F={F} scales={scales} acc={acc}"
    assert_sum_bound(got, want, want_abs, degrees(indptr)[:, None], what)
    if not acc:
        empty = degrees(indptr) == 0
        assert (got.cpu()[empty] == 0).all(), f"{what}: empty rows not zero"


# ------------------------------------------------------- GAT kernel set

def check_spmm_edge(H, D):
    from bnsgcn_amd.ops.csr_torch import transpose_csr
    from bnsgcn_amd.ops.functional import spmm_edge_raw
    indptr, indices = fixture_csr()
    E = indices.numel()
    g = gen(200 + 10 * H + D)
    w = torch.randn(E, H, generator=g)
    x = torch.randn(N_COLS, H, D, generator=g)
    base = torch.randn(N_ROWS, H, D, generator=g)
    deg = degrees(indptr)[:, None, None]
    ip, ix = cu(indptr), cu(indices)
    tag = f"spmm_edge (H,D)=({H},{D})"

    want = ref.spmm_edge_sum(indptr, indices, dbl(w), dbl(x))
    want_abs = ref.spmm_edge_sum(indptr, indices, dbl(w).abs(), dbl(x).abs())
    junk = torch.full((N_ROWS, H, D), float("nan"), device=DEV)
    torch.cuda.synchronize()
    del junk
    got = spmm_edge_raw(ip, ix, cu(w), cu(x))
    assert_sum_bound(got, want, want_abs, deg, tag)
    assert (got.cpu()[degrees(indptr) == 0] == 0).all(), f"{tag}: empty rows"

    got = spmm_edge_raw(ip, ix, cu(w), cu(x), out=cu(base).clone())
    assert_sum_bound(got, want + dbl(base), want_abs + dbl(base).abs(), deg,
                     tag + " out=")

    # backward form: transposed CSR, weights permuted INSIDE the kernel
    tip, tix, eperm = transpose_csr(ip, ix, N_COLS)
    tip_c, tix_c, ep_c = tip.cpu(), tix.cpu(), eperm.cpu()
    gy = torch.randn(N_ROWS, H, D, generator=g)
    want = ref.spmm_edge_sum(tip_c, tix_c, dbl(w)[ep_c], dbl(gy))
    want_abs = ref.spmm_edge_sum(tip_c, tix_c, dbl(w)[ep_c].abs(),
                                 dbl(gy).abs())
    tdeg = degrees(tip_c)
    assert tdeg.max() > 512       # hub column -> split row
    got = spmm_edge_raw(tip, tix, cu(w), cu(gy), wperm=eperm)
    assert_sum_bound(got, want, want_abs, tdeg[:, None, None],
                     tag + " wperm")
    base_t = torch.randn(N_COLS, H, D, generator=g)
    got = spmm_edge_raw(tip, tix, cu(w), cu(gy), out=cu(base_t).clone(),
                        wperm=eperm)
    assert_sum_bound(got, want + dbl(base_t), want_abs + dbl(base_t).abs(),
                     tdeg[:, None, None], tag + " wperm out=")


def check_sddmm_dot(H, D):
    from bnsgcn_amd.ops.functional import sddmm_dot_raw
    indptr, indices = fixture_csr()
    g = gen(300 + 10 * H + D)
    a = torch.randn(N_ROWS, H, D, generator=g)
    b = torch.randn(N_COLS, H, D, generator=g)
    want = ref.sddmm_dot(indptr, indices, dbl(a), dbl(b))
    want_abs = ref.sddmm_dot(indptr, indices, dbl(a).abs(), dbl(b).abs())
    got = sddmm_dot_raw(cu(indptr), cu(indices), cu(a), cu(b))
    assert_sum_bound(got, want, want_abs, float(D),
                     f"sddmm_dot (H,D)=({H},{D})")


def check_sddmm_add(H, slope):
    from bnsgcn_amd.ops.functional import sddmm_add_raw
    indptr, indices = fixture_csr()
    g = gen(400 + H)
    el = torch.randn(N_COLS, H, generator=g)
    er = torch.randn(N_ROWS, H, generator=g)
    want = ref.sddmm_add(indptr, indices, dbl(el), dbl(er))
    if slope >= 0:
        want = torch.nn.functional.leaky_relu(want, slope)
    got = sddmm_add_raw(cu(indptr), cu(indices), cu(el), cu(er), slope)
    torch.testing.assert_close(got.double().cpu(), want, rtol=1e-5, atol=1e-5)


def check_segment_softmax(H):
    from bnsgcn_amd.ops.functional import (segment_softmax_raw,
                                           segment_softmax_bwd_raw)
    indptr, indices = fixture_csr()
    E = indices.numel()
    g = gen(500 + H)
    logits = 3 * torch.randn(E, H, generator=g)
    want = ref.segment_softmax(indptr, dbl(logits))
    got = segment_softmax_raw(cu(indptr), cu(logits))
    assert_softmax_close(got, want, f"segment_softmax H={H}")
    # backward on the fp32-rounded REFERENCE alpha (same inputs both sides)
    a32 = want.float()
    ga = torch.randn(E, H, generator=g)
    want_b = ref.segment_softmax_backward(indptr, dbl(a32), dbl(ga))
    got_b = segment_softmax_bwd_raw(cu(indptr), cu(a32), cu(ga))
    assert_softmax_close(got_b, want_b, f"segment_softmax_bwd H={H}")


def check_segment_sum_edges(H):
    from bnsgcn_amd.ops._ext import require_ext
    from bnsgcn_amd.ops.csr_torch import transpose_csr
    from bnsgcn_amd.ops.functional import _worklist_of
    ext = require_ext()
    indptr, indices = fixture_csr()
    E = indices.numel()
    grad = torch.randn(E, H, generator=gen(600 + H))
    row = torch.repeat_interleave(torch.arange(N_ROWS),
                                  indptr[1:] - indptr[:-1])
    ip, ix = cu(indptr), cu(indices)
    want = torch.zeros(N_ROWS, H, dtype=torch.float64).index_add(
        0, row, dbl(grad))
    want_abs = torch.zeros(N_ROWS, H, dtype=torch.float64).index_add(
        0, row, dbl(grad).abs())
    got = ext.segment_sum_edges(*_worklist_of(ip)[:4], None, cu(grad), N_ROWS)
    assert_sum_bound(got, want, want_abs, degrees(indptr)[:, None],
                     f"segment_sum_edges H={H}")
    tip, tix, eperm = transpose_csr(ip, ix, N_COLS)
    assert degrees(tip.cpu()).max() > 512
    want = torch.zeros(N_COLS, H, dtype=torch.float64).index_add(
        0, indices.long(), dbl(grad))
    want_abs = torch.zeros(N_COLS, H, dtype=torch.float64).index_add(
        0, indices.long(), dbl(grad).abs())
    got = ext.segment_sum_edges(*_worklist_of(tip)[:4], eperm, cu(grad),
                                N_COLS)
    assert_sum_bound(got, want, want_abs, degrees(tip.cpu())[:, None],
                     f"segment_sum_edges eperm H={H}")


# --------------------------------------------------------- attn_project

def check_attn_project(H, D, n):
    """Forward and the three gradients of ops.functional.attn_project
    through autograd (HIP kernels at H <= 8 and H*D % 4 == 0, the
    ops/reference.py formulas on device tensors otherwise)."""
    from bnsgcn_amd.ops import functional as BF
    g = gen(800 + 10 * H + D)
    z = torch.randn(n, H, D, generator=g)
    al = torch.randn(1, H, D, generator=g)
    ar = torch.randn(1, H, D, generator=g)
    g_el = torch.randn(n, H, generator=g)
    g_er = torch.randn(n, H, generator=g)
    zg, alg, arg = (cu(t).requires_grad_(True) for t in (z, al, ar))
    el, er = BF.attn_project(zg, alg, arg)
    assert el.shape == (n, H) and er.shape == (n, H)
    (el * cu(g_el) + er * cu(g_er)).sum().backward()

    tag = f"attn_project (H,D)=({H},{D}) n={n}"
    wel, wer = ref.attn_project(dbl(z), dbl(al), dbl(ar))
    ael, aer = ref.attn_project(dbl(z).abs(), dbl(al).abs(), dbl(ar).abs())
    worst = [assert_sum_bound(el, wel, ael, float(D), tag + " el"),
             assert_sum_bound(er, wer, aer, float(D), tag + " er")]
    wdz, wdal, wdar = ref.attn_project_backward(
        dbl(z), dbl(al), dbl(ar), dbl(g_el), dbl(g_er))
    adz, adal, adar = ref.attn_project_backward(
        dbl(z).abs(), dbl(al).abs(), dbl(ar).abs(), dbl(g_el).abs(),
        dbl(g_er).abs())
    worst += [assert_sum_bound(zg.grad, wdz, adz, 2.0, tag + " dz"),
              assert_sum_bound(alg.grad, wdal, adal, float(n), tag + " dal"),
              assert_sum_bound(arg.grad, wdar, adar, float(n), tag + " dar")]
    return max(worst)


# -------------------------------------------------------- union softmax

def softmax2_inputs(H, shifted=True):
    """3*randn logits on the two fixture edge sets; set 2 is shifted per
    row by +90 / -90 / 0 (cycling by row), so a kernel that takes the max
    from ONE set only overflows fp32 exp on the +90 rows instead of
    hiding behind softmax's shift invariance."""
    ip1, ix1 = fixture_csr()
    ip2, ix2 = fixture_csr2()
    g = gen(700 + H)
    l1 = 3 * torch.randn(ix1.numel(), H, generator=g)
    l2 = 3 * torch.randn(ix2.numel(), H, generator=g)
    if shifted:
        row2 = torch.repeat_interleave(torch.arange(N_ROWS),
                                       ip2[1:] - ip2[:-1])
        shift = torch.tensor([90.0, -90.0, 0.0])[row2 % 3]
        l2 = l2 + shift[:, None]
    return ip1, l1, ip2, l2, g


def check_softmax2(H):
    from bnsgcn_amd.ops.functional import (segment_softmax2_raw,
                                           segment_softmax2_bwd_raw)
    ip1, l1, ip2, l2, g = softmax2_inputs(H)
    w1, w2 = ref.segment_softmax2(ip1, dbl(l1), ip2, dbl(l2))
    g1, g2 = segment_softmax2_raw(cu(ip1), cu(l1), cu(ip2), cu(l2))
    assert_softmax_close(g1, w1, f"softmax2 H={H} set1")
    assert_softmax_close(g2, w2, f"softmax2 H={H} set2")
    a1, a2 = w1.float(), w2.float()
    ga = torch.randn(l1.shape, generator=g)
    gb = torch.randn(l2.shape, generator=g)
    wd1, wd2 = ref.segment_softmax2_backward(ip1, dbl(a1), dbl(ga),
                                             ip2, dbl(a2), dbl(gb))
    gd1, gd2 = segment_softmax2_bwd_raw(cu(ip1), cu(a1), cu(ga),
                                        cu(ip2), cu(a2), cu(gb))
    assert_softmax_close(gd1, wd1, f"softmax2_bwd H={H} set1")
    assert_softmax_close(gd2, wd2, f"softmax2_bwd H={H} set2")


def check_softmax2_all_empty(H):
    from bnsgcn_amd.ops.functional import (segment_softmax2_raw,
                                           segment_softmax2_bwd_raw)
    ip = torch.zeros(N_ROWS + 1, dtype=torch.long, device=DEV)
    l = torch.zeros(0, H, device=DEV)
    a1, a2 = segment_softmax2_raw(ip, l, ip, l)
    assert a1.shape == (0, H) and a2.shape == (0, H)
    d1, d2 = segment_softmax2_bwd_raw(ip, a1, l, ip, a2, l)
    assert d1.shape == (0, H) and d2.shape == (0, H)
    torch.cuda.synchronize()


def check_softmax2_dropout(H, keep=0.7):
    """The three assertions of test_gpu.test_fused_attn_dropout_softmax2,
    on the long-segment edge sets (unshifted logits: every alpha stays a
    normal fp32 number, so a zero in the output is a dropped entry)."""
    from bnsgcn_amd.ops import functional as BF
    ip1, l1, ip2, l2, g = softmax2_inputs(H, shifted=False)
    torch.manual_seed(1234 + H)           # the op draws its seed from torch
    l1g = cu(l1).requires_grad_(True)
    l2g = cu(l2).requires_grad_(True)
    da1, da2 = BF.segment_softmax2(l1g, l2g, cu(ip1), cu(ip2),
                                   p_drop=1 - keep)
    a1, a2 = ref.segment_softmax2(ip1, dbl(l1), ip2, dbl(l2))
    assert a1.min() > 1e-30 and a2.min() > 1e-30
    m1 = (da1 != 0).double().cpu()
    m2 = (da2 != 0).double().cpu()
    assert_softmax_close(da1, a1 * m1 / keep, f"dropout H={H} da1")
    assert_softmax_close(da2, a2 * m2 / keep, f"dropout H={H} da2")
    n = m1.numel() + m2.numel()
    frac = float(m1.sum() + m2.sum()) / n
    tol = 5 * (keep * (1 - keep) / n) ** 0.5
    print(f"dropout H={H}: kept {frac:.4f} of {n} (tol {tol:.4f})")
    assert abs(frac - keep) < tol, (frac, tol)

    ga = torch.randn(l1.shape, generator=g)
    gb = torch.randn(l2.shape, generator=g)
    ((da1 * cu(ga)).sum() + (da2 * cu(gb)).sum()).backward()
    d1, d2 = ref.segment_softmax2_backward(
        ip1, a1, dbl(ga) * m1 / keep, ip2, a2, dbl(gb) * m2 / keep)
    assert_softmax_close(l1g.grad, d1, f"dropout H={H} dl1")
    assert_softmax_close(l2g.grad, d2, f"dropout H={H} dl2")


# ---------------------------------------------------------- script mode

def _case_spmm_subw64():
    assert os.environ.get("BNSGCN_SPMM_SUBW32_MAX") == "0"
    for F in (64, 128):
        for scales, acc in ((True, False), (False, False), (False, True)):
            check_spmm_sum(F, scales, acc)


# case name -> (environment switch, runner)
CASES = {
    "spmm_subw64": ({"BNSGCN_SPMM_SUBW32_MAX": "0"}, _case_spmm_subw64),
}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print(f"usage: {argv[0]} {{{'|'.join(CASES)}}}", file=sys.stderr)
        return 2
    if not torch.cuda.is_available():
        print("no GPU", file=sys.stderr)
        return 3
    CASES[argv[1]][1]()
    torch.cuda.synchronize()
    print(f"{argv[1]}: ok")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
