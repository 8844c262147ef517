"""Fixtures, oracles and check functions for tests/test_gpu_dense_paths.py:
the fp32 MFMA GEMM, LayerNorm, the mask-free dropout and the capped /
grid-stride launches of the remaining kernels.

Rules. Every input is generated on the CPU from a seeded generator and no
GPU kernel is ever the reference. Three oracles, none tuned on the
kernels' output:

* E (exact). Inputs are small integers stored as fp32 (in [-2, 2] unless
  stated), chosen so that every partial sum stays below 2^24. Every order
  of fp32 additions, MFMA accumulation and float atomics is then exact,
  and the result must `torch.equal` the integer computation. The
  reference runs in float64, where the same products and sums are exact
  integers below 2^53, i.e. it IS the int64 result (each check asserts
  the 2^24 limit on the reference of the absolute values). E sees a
  single dropped, duplicated or misplaced element at any size; it is used
  for everything that wraps a grid, for deep split-K, copies and masks.
* S (summation bound). kernel_path_checks.assert_sum_bound with random
  normal inputs and n_terms = the reduction length; used at the small
  shapes, where it is tight.
* M (measured). For the elementwise LayerNorm outputs y, mean, rstd, dx:
  error = max|got - ref64| / max|ref64| per tensor. The fp32 CPU
  torch.native_layer_norm (+relu, autograd for dx) is measured against
  the float64 formula; the GPU may use 8x that, floored at 1e-5. A tensor
  whose reference magnitude is 0 must be exactly 0.

ReLU sign: with act=True the backward recomputes the pre-activation in
fp32, so wherever the float64 pre-activation satisfies
|pre| < 64*EPS*(|xhat*gamma| + |beta|) dy is set to 0 before any run (at
most 0.1% of the elements; asserted) and the mask cannot matter there.

dgamma / dbeta use S with the bounds (n + 8)*EPS*sum|dy*m| and
(n + 16)*EPS*sum|dy*m|*(|xhat| + 1): the +1 and +8 cover xhat, which the
kernel recomputes in fp32 from the saved fp32 mean and rstd (inputs keep
|mean|*rstd <= 1). At large n the bound only sees structural errors, so
dy is zero outside 64 probe rows and n_terms = 64.

Dropout masks are pinned bit for bit by keep_mask(), a numpy uint64
implementation of the kernels' splitmix64 drop_keep and threshold.

Run as a script (`python tests/dense_path_checks.py CASE`) it executes
one environment-gated case in a fresh process (BNSGCN_GEMM is read at
import of ops/functional.py) and exits non-zero on a mismatch.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import kernel_path_checks as K  # noqa: E402
from kernel_path_checks import (DEV, EPS, assert_softmax_close,  # noqa: E402
                                assert_sum_bound, cu, dbl, gen)
from bnsgcn_amd.ops import reference as ref  # noqa: E402

LN_EPS = 1e-5
EXACT_LIMIT = float(2 ** 24)


def _ext():
    from bnsgcn_amd.ops._ext import require_ext
    return require_ext()


# -------------------------------------------------------------- oracles

def ints(shape, g, lo=-2, hi=2):
    """Small integers stored as fp32 (oracle E)."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def assert_exact(got, want64, want64_abs, what):
    """Oracle E: `got` (fp32) equals the integer result `want64`;
    `want64_abs` (the reference on absolute values) bounds every partial
    sum and must stay below 2^24."""
    peak = float(want64_abs.max()) if want64_abs.numel() else 0.0
    assert peak < EXACT_LIMIT, f"{what}: fixture sums reach {peak} >= 2^24"
    got = got.detach().double().cpu()
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    bad = got != want64
    n_bad = int(bad.sum())
    print(f"{what}: exact, {n_bad} of {bad.numel()} elements differ "
          f"(peak |sum| {peak:.0f})")
    if n_bad:
        first = bad.flatten().nonzero()[:5, 0].tolist()
        raise AssertionError(
            f"{what}: {n_bad} of {bad.numel()} elements differ from the exact "
            f"result; first flat indices {first}, got "
            f"{got.flatten()[first].tolist()}, want "
            f"{want64.flatten()[first].tolist()}")


def assert_measured(got, ref64, ref32, what):
    """Oracle M (module docstring). Returns (e32, egpu, tol)."""
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    if scale == 0.0:
        print(f"{what}: reference is all zero")
        assert not got.any(), f"{what}: reference is 0, output is not"
        return 0.0, 0.0, 0.0
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    egpu = float((got - ref64).abs().max()) / scale
    tol = max(8 * e32, 1e-5)
    print(f"{what}: fp32-cpu rel err {e32:.3g}, gpu rel err {egpu:.3g}, "
          f"tol {tol:.3g}, gpu/cpu {egpu / max(e32, 1e-300):.3g}")
    assert egpu <= tol, (f"{what}: gpu rel err {egpu:.3g} over tol {tol:.3g} "
                         f"(fp32-cpu {e32:.3g})")
    return e32, egpu, tol


def keep_threshold(keep):
    """The kernels' threshold: `keep` arrives as a float; a value that
    rounds to 1.0f keeps everything (returned as 2^32)."""
    k32 = float(np.float32(keep))
    if k32 >= 1.0:
        return 1 << 32
    if k32 <= 0.0:
        return 0
    return int(np.uint32(np.float64(k32) * 4294967296.0))


def keep_mask(idx, keep, seed):
    """Host form of drop_keep (splitmix64 of seed + idx, high 32 bits
    below the threshold), in numpy uint64 arithmetic; idx is an integer
    array of flat element indices. Returns a bool array."""
    with np.errstate(over="ignore"):
        z = np.asarray(idx).astype(np.uint64) + np.uint64(seed)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(32)) < np.uint64(keep_threshold(keep))


def inv_keep32(keep):
    """fl32(1 / fl32(keep)), the kernels' scale (1 when keep rounds to 1)."""
    k32 = np.float32(keep)
    return np.float32(1.0) if k32 >= 1.0 else np.float32(1.0) / k32


# ----------------------------------------------------------------- GEMM

def _gemm_operands(layout, M, N, Kd, g, integer):
    """(call, A64 [M,Kd], B64 [Kd,N]) for an M x N output with inner
    dimension Kd through gemm_nt_bias / gemm_nn / gemm_tn."""
    ext = _ext()
    mk = (lambda *s: ints(s, g)) if integer else \
        (lambda *s: torch.randn(*s, generator=g))
    if layout == "nt":
        x, w = mk(M, Kd), mk(N, Kd)
        return (lambda b: ext.gemm_nt_bias(cu(x), cu(w), cu(b))), dbl(x), \
            dbl(w).t()
    if layout == "nn":
        gr, w = mk(M, Kd), mk(Kd, N)
        return (lambda b: ext.gemm_nn(cu(gr), cu(w))), dbl(gr), dbl(w)
    gr, x = mk(Kd, M), mk(Kd, N)
    return (lambda b: ext.gemm_tn(cu(gr), cu(x))), dbl(gr).t(), dbl(x)


def check_gemm(layout, M, N, Kd, integer, bias=False, seed=0):
    """One GEMM call against the float64 matmul: oracle E for integer
    operands, oracle S (n_terms = Kd) for randn ones. bias only with
    layout 'nt'; the integer bias is 1 or 2, never 0, so the exact check
    sees a bias added once per split-K slice as (slices - 1) * bias."""
    assert layout == "nt" or not bias
    g = gen(7000 + seed + 13 * M + 7 * N + Kd)
    call, a64, b64 = _gemm_operands(layout, M, N, Kd, g, integer)
    b = None
    if bias:
        b = ints((N,), g, 1, 2) if integer else torch.randn(N, generator=g)
    want, want_abs = a64 @ b64, a64.abs() @ b64.abs()
    if bias:
        want, want_abs = want + dbl(b), want_abs + dbl(b).abs()
    got = call(b)
    what = f"gemm_{layout} {M}x{N} inner {Kd} bias={bias}"
    if integer:
        assert_exact(got, want, want_abs, what + " [E]")
    else:
        assert_sum_bound(got, want, want_abs, float(Kd), what + " [S]")


def check_linear(M, Kd, N, bias, expect_mode=None):
    """BF.linear through autograd (forward, dx, dW, db) with oracle S
    against float64 matmuls; n_terms = K, N, M, M."""
    from bnsgcn_amd.ops import functional as BF
    if expect_mode is not None:
        assert BF._GEMM_MODE == expect_mode, BF._GEMM_MODE
    g = gen(7500 + M + Kd + N + int(bias))
    x = torch.randn(M, Kd, generator=g)
    w = torch.randn(N, Kd, generator=g)
    b = torch.randn(N, generator=g) if bias else None
    gy = torch.randn(M, N, generator=g)
    xg, wg = cu(x).requires_grad_(True), cu(w).requires_grad_(True)
    bg = cu(b).requires_grad_(True) if bias else None
    y = BF.linear(xg, wg, bg)
    y.backward(cu(gy))
    xd, wd, gd = dbl(x), dbl(w), dbl(gy)
    tag = f"linear[{BF._GEMM_MODE}] {M}x{Kd}->{N} bias={bias}"
    want, want_abs = xd @ wd.t(), xd.abs() @ wd.abs().t()
    if bias:
        want, want_abs = want + dbl(b), want_abs + dbl(b).abs()
    assert_sum_bound(y, want, want_abs, float(Kd), tag + " y")
    assert_sum_bound(xg.grad, gd @ wd, gd.abs() @ wd.abs(), float(N),
                     tag + " dx")
    assert_sum_bound(wg.grad, gd.t() @ xd, gd.abs().t() @ xd.abs(), float(M),
                     tag + " dW")
    if bias:
        assert_sum_bound(bg.grad, gd.sum(0), gd.abs().sum(0), float(M),
                         tag + " db")


LINEAR_SHAPES = [(300, 602, 41), (77, 129, 33)]


# ------------------------------------------------------------ LayerNorm

class LnCase:
    """Inputs and float64 / fp32-CPU references of one LayerNorm shape.

    x = z - rowmean(z) + 0.25 * rowstd(z) * u with z ~ N(0,1), u ~ U(-1,1)
    (so |mean| * rstd <= 1 with a non-zero mean), plus `offset`;
    gamma, beta ~ N(0,1)."""

    def __init__(self, n, F, act, seed, offset=0.0):
        self.n, self.F, self.act = n, F, bool(act)
        g = gen(seed)
        z = torch.randn(n, F, generator=g, dtype=torch.float64)
        u = 2 * torch.rand(n, 1, generator=g, dtype=torch.float64) - 1
        sd = z.var(1, unbiased=False, keepdim=True).sqrt()
        self.x = (z - z.mean(1, keepdim=True) + 0.25 * sd * u + offset).float()
        self.gamma = torch.randn(F, generator=g)
        self.beta = torch.randn(F, generator=g)
        self.g = g
        x, gm, bt = dbl(self.x), dbl(self.gamma), dbl(self.beta)
        self.mean = x.mean(1)
        var = x.var(1, unbiased=False)
        self.rstd = (var + LN_EPS).rsqrt()
        self.xhat = (x - self.mean[:, None]) * self.rstd[:, None]
        pre = self.xhat * gm + bt
        self.y = pre.clamp_min(0) if self.act else pre
        self.m = (pre > 0).double() if self.act else torch.ones_like(pre)
        # elements whose ReLU sign fp32 cannot be trusted with
        self.unsafe = (pre.abs() < 64 * EPS * ((self.xhat * gm).abs()
                                               + bt.abs())) \
            if self.act else torch.zeros_like(pre, dtype=torch.bool)
        n_unsafe = int(self.unsafe.sum())
        print(f"ln n={n} F={F} act={act}: {n_unsafe} sign-unsafe elements")
        assert n_unsafe <= 1e-3 * pre.numel(), n_unsafe
        if offset == 0.0:
            assert float((self.mean.abs() * self.rstd).max()) <= 1.0
        # fp32 CPU run of torch's own LayerNorm (oracle M's yardstick)
        self.x32 = self.x.clone().requires_grad_(True)
        y32, mean32, rstd32 = torch.native_layer_norm(
            self.x32, (F,), self.gamma, self.beta, LN_EPS)
        self.y32_graph = torch.relu(y32) if self.act else y32
        self.y32 = self.y32_graph.detach()
        self.mean32 = mean32.detach().reshape(n)
        self.rstd32 = rstd32.detach().reshape(n)

    def make_dy(self, rows=None):
        """randn dy, zero at the sign-unsafe elements; with `rows`, zero
        outside those rows."""
        dy = torch.randn(self.n, self.F, generator=self.g)
        if rows is not None:
            keep = torch.zeros(self.n, 1)
            keep[rows] = 1.0
            dy = dy * keep
        dy[self.unsafe] = 0.0
        return dy

    def backward64(self, dy):
        gm = dbl(self.gamma)
        dm = dbl(dy) * self.m
        gg = dm * gm
        dx = self.rstd[:, None] * (gg - gg.mean(1, keepdim=True) - self.xhat *
                                   (gg * self.xhat).mean(1, keepdim=True))
        return dx, (dm * self.xhat).sum(0), dm.sum(0), dm.abs()

    def dx32(self, dy):
        return torch.autograd.grad(self.y32_graph, self.x32, dy,
                                   retain_graph=True)[0]


def check_ln_forward(c, y, mean, rstd, tag, out):
    out[tag + " y"] = assert_measured(y, c.y, c.y32, tag + " y")
    out[tag + " mean"] = assert_measured(mean, c.mean, c.mean32, tag + " mean")
    out[tag + " rstd"] = assert_measured(rstd, c.rstd, c.rstd32, tag + " rstd")


def check_ln_weight_grads(c, dy, dgamma, dbeta, n_terms, tag):
    _, dg64, db64, dm_abs = c.backward64(dy)
    assert_sum_bound(dbeta, db64, dm_abs.sum(0), float(n_terms),
                     tag + " dbeta")
    assert_sum_bound(dgamma, dg64, (dm_abs * (c.xhat.abs() + 1)).sum(0),
                     float(n_terms) + 8.0, tag + " dgamma")


def check_layer_norm_small(n, F, act, offset=0.0):
    """ext.ln_fwd / ext.ln_bwd at one small shape: M on y, mean, rstd,
    dx; S on dgamma, dbeta (not in the ill-conditioned offset case,
    whose |mean|*rstd is ~100)."""
    ext = _ext()
    c = LnCase(n, F, act, 8000 + 3 * n + F + int(act), offset)
    dy = c.make_dy()
    tag = f"ln n={n} F={F} act={int(act)}" + (f" +{offset:g}" if offset else "")
    xg, gg, bg = cu(c.x), cu(c.gamma), cu(c.beta)
    y, mean, rstd = ext.ln_fwd(xg, gg, bg, LN_EPS, int(act))
    dx, dgamma, dbeta = ext.ln_bwd(xg, cu(dy), gg, bg, mean, rstd, int(act))
    res = {}
    check_ln_forward(c, y, mean, rstd, tag, res)
    res[tag + " dx"] = assert_measured(dx, c.backward64(dy)[0], c.dx32(dy),
                                       tag + " dx")
    if offset == 0.0:
        check_ln_weight_grads(c, dy, dgamma, dbeta, n, tag)
    return res


def check_layer_norm_autograd(n, F, act):
    """BF.layer_norm through autograd: M on y and dx, S on the weight
    gradients. F > 1024 takes the torch fall-back and must match too."""
    from bnsgcn_amd.ops import functional as BF
    c = LnCase(n, F, act, 8500 + n + F + int(act))
    dy = c.make_dy()
    xg, gg, bg = (cu(t).requires_grad_(True) for t in (c.x, c.gamma, c.beta))
    y = BF.layer_norm(xg, gg, bg, LN_EPS, act=act)
    y.backward(cu(dy))
    tag = f"BF.layer_norm n={n} F={F} act={int(act)}"
    assert_measured(y, c.y, c.y32, tag + " y")
    assert_measured(xg.grad, c.backward64(dy)[0], c.dx32(dy), tag + " dx")
    check_ln_weight_grads(c, dy, gg.grad, bg.grad, n, tag)


def ln_probe_rows(n, seed):
    """64 rows: 0, n-1, the rows around the first grid wrap (131,072 rows
    per pass), the first and last row of four ln_bwd_w row chunks (the
    last non-empty one included), filled up with seeded random rows."""
    row_chunks = min((n + 255) // 256, 2048)
    rows_per = (n + row_chunks - 1) // row_chunks
    last_chunk = (n - 1) // rows_per
    rows = {0, n - 1, 131071, 131072, 131073}
    for ch in (1, last_chunk // 2, last_chunk - 1, last_chunk):
        rows.add(ch * rows_per)
        rows.add(min((ch + 1) * rows_per, n) - 1)
    rows = {r for r in rows if 0 <= r < n}
    extra = torch.randperm(n, generator=gen(seed))[:128].tolist()
    for r in extra:
        if len(rows) == 64:
            break
        rows.add(r)
    assert len(rows) == 64
    return torch.tensor(sorted(rows))


def check_layer_norm_large(n, F, act):
    """Row loop beyond 131,072 rows and ln_bwd_w's row chunks. Dense dy:
    M on y, mean, rstd, dx. Probe dy (64 non-zero rows): S on dgamma /
    dbeta with n_terms = 64, dx exactly 0 wherever dy is 0."""
    ext = _ext()
    c = LnCase(n, F, act, 8800 + F + int(act))
    tag = f"ln n={n} F={F} act={int(act)}"
    xg, gg, bg = cu(c.x), cu(c.gamma), cu(c.beta)
    y, mean, rstd = ext.ln_fwd(xg, gg, bg, LN_EPS, int(act))
    res = {}
    check_ln_forward(c, y, mean, rstd, tag, res)
    dy = c.make_dy()
    dx = ext.ln_bwd(xg, cu(dy), gg, bg, mean, rstd, int(act))[0]
    res[tag + " dx"] = assert_measured(dx, c.backward64(dy)[0], c.dx32(dy),
                                       tag + " dense dx")
    rows = ln_probe_rows(n, 8900 + F)
    dy = c.make_dy(rows)
    dx, dgamma, dbeta = ext.ln_bwd(xg, cu(dy), gg, bg, mean, rstd, int(act))
    check_ln_weight_grads(c, dy, dgamma, dbeta, 64, tag + " probe")
    dx = dx.cpu()
    zero_rows = torch.ones(n, dtype=torch.bool)
    zero_rows[rows] = False
    assert torch.isfinite(dx).all(), tag
    assert not dx[zero_rows].any(), f"{tag}: dx != 0 on a row whose dy is 0"
    assert_measured(dx[rows], c.backward64(dy)[0][rows], c.dx32(dy)[rows],
                    tag + " probe dx")
    return res


# -------------------------------------------------------------- dropout

def dropout_want(x, keep, seed, start=0):
    """where(keep_mask, x * fl32(1/keep32), 0) in fp32; returns
    (want, mask)."""
    mask = keep_mask(np.arange(start, start + x.numel(), dtype=np.int64),
                     keep, seed).reshape(tuple(x.shape))
    want = np.where(mask, x.numpy() * inv_keep32(keep), np.float32(0))
    return torch.from_numpy(want.astype(np.float32)), torch.from_numpy(mask)


def check_dropout_exact(n, keep, seed):
    """ext.dropout_apply on strictly positive x, bit for bit against the
    host mask; returns the GPU's mask."""
    x = torch.rand(n, generator=gen(9000 + n % 1000)) + 0.5
    want, mask = dropout_want(x, keep, seed)
    got = _ext().dropout_apply(cu(x), keep, seed).cpu()
    n_bad = int((got != want).sum())
    print(f"dropout n={n} keep={keep} seed={seed}: kept "
          f"{int(mask.sum())}, {n_bad} elements differ")
    assert torch.equal(got != 0, mask), "mask differs from the host mask"
    assert torch.equal(got, want), f"{n_bad} values differ"
    return got != 0


def check_dropout_autograd(n, p, torch_seed):
    """BF.dropout with torch.manual_seed fixing the drawn seed: output and
    gradient equal the host-mask forms exactly."""
    from bnsgcn_amd.ops import functional as BF
    torch.manual_seed(torch_seed)
    seed = int(torch.randint(0, 2**62, (1,)).item())
    g = gen(9100 + n)
    x = torch.rand(n, generator=g) + 0.5
    gy = torch.randn(n, generator=g)
    keep = 1.0 - p
    xg = cu(x).requires_grad_(True)
    torch.manual_seed(torch_seed)
    y = BF.dropout(xg, p, True)
    y.backward(cu(gy))
    want, mask = dropout_want(x, keep, seed)
    assert torch.equal(y.detach().cpu(), want)
    want_g, _ = dropout_want(gy, keep, seed)
    assert torch.equal(xg.grad.cpu(), want_g)
    assert 0 < int(mask.sum()) < mask.numel()


# ---------------------------------------------- fused attention dropout

def check_softmax2_dropout_seeded(H, keep=0.7, seed=2**40 + 7):
    """ext.segment_softmax2 / _backward with an explicit seed on the
    unshifted fixture logits (all alphas > 1e-30, so a zero is a dropped
    entry): the masks of both sets equal the host mask (set 2 starting at
    offset l1.numel()), the values and the backward match the float64
    reference fed with the host masks."""
    ext = _ext()
    ip1, l1, ip2, l2, g = K.softmax2_inputs(H, shifted=False)
    r1, r2 = ref.segment_softmax2(ip1, dbl(l1), ip2, dbl(l2))
    assert r1.min() > 1e-30 and r2.min() > 1e-30
    n1, n2 = l1.numel(), l2.numel()
    m1 = torch.from_numpy(keep_mask(np.arange(n1), keep, seed)
                          .reshape(tuple(l1.shape)))
    m2 = torch.from_numpy(keep_mask(n1 + np.arange(n2), keep, seed)
                          .reshape(tuple(l2.shape)))
    k32 = float(np.float32(keep))
    a1, a2, da1, da2 = ext.segment_softmax2(cu(ip1), cu(l1), cu(ip2), cu(l2),
                                            keep, seed)
    tag = f"seeded dropout H={H}"
    assert torch.equal((da1 != 0).cpu(), m1), f"{tag}: set 1 mask"
    assert torch.equal((da2 != 0).cpu(), m2), f"{tag}: set 2 mask"
    k = min(n1, n2)       # set 2 must not reuse set 1's stream from 0
    assert not torch.equal(m1.flatten()[:k], m2.flatten()[:k])
    assert_softmax_close(a1, r1, f"{tag} a1")
    assert_softmax_close(a2, r2, f"{tag} a2")
    assert_softmax_close(da1, r1 * m1 / k32, f"{tag} da1")
    assert_softmax_close(da2, r2 * m2 / k32, f"{tag} da2")
    a1f, a2f = r1.float(), r2.float()
    ga = torch.randn(l1.shape, generator=g)
    gb = torch.randn(l2.shape, generator=g)
    w1, w2 = ref.segment_softmax2_backward(
        ip1, dbl(a1f), dbl(ga) * m1 / k32, ip2, dbl(a2f), dbl(gb) * m2 / k32)
    d1, d2 = ext.segment_softmax2_backward(
        cu(ip1), cu(a1f), cu(ga), cu(ip2), cu(a2f), cu(gb), keep, seed)
    assert_softmax_close(d1, w1, f"{tag} dl1")
    assert_softmax_close(d2, w2, f"{tag} dl2")


def check_softmax2_keep_rounds_to_one(H, keep=1 - 1e-9):
    """0 < p_drop < 2^-25: keep rounds to 1.0f, so nothing is dropped and
    nothing scaled — da must equal a in every element (run after a
    NaN-filled allocation of the same sizes was released, so memory the
    kernel leaves unwritten is likely to show), backward as without
    dropout."""
    ext = _ext()
    assert keep < 1.0 and float(np.float32(keep)) == 1.0
    ip1, l1, ip2, l2, g = K.softmax2_inputs(H, shifted=False)
    r1, r2 = ref.segment_softmax2(ip1, dbl(l1), ip2, dbl(l2))
    junk = [torch.full(tuple(t.shape), float("nan"), device=DEV)
            for t in (l1, l2, l1, l2)]
    torch.cuda.synchronize()
    del junk
    a1, a2, da1, da2 = ext.segment_softmax2(cu(ip1), cu(l1), cu(ip2), cu(l2),
                                            keep, 12345)
    tag = f"keep=1-1e-9 H={H}"
    assert torch.isfinite(da1).all() and torch.isfinite(da2).all(), tag
    assert torch.equal(da1, a1), f"{tag}: da1 != a1"
    assert torch.equal(da2, a2), f"{tag}: da2 != a2"
    assert_softmax_close(da1, r1, f"{tag} da1")
    assert_softmax_close(da2, r2, f"{tag} da2")
    a1f, a2f = r1.float(), r2.float()
    ga = torch.randn(l1.shape, generator=g)
    gb = torch.randn(l2.shape, generator=g)
    w1, w2 = ref.segment_softmax2_backward(ip1, dbl(a1f), dbl(ga),
                                           ip2, dbl(a2f), dbl(gb))
    d1, d2 = ext.segment_softmax2_backward(
        cu(ip1), cu(a1f), cu(ga), cu(ip2), cu(a2f), cu(gb), keep, 12345)
    assert_softmax_close(d1, w1, f"{tag} dl1")
    assert_softmax_close(d2, w2, f"{tag} dl2")


# ------------------------------------------------------ wrapped launches

def check_pack_scatter_wrapped(n, F):
    """n * F (or n * F/4) slots beyond the 4096-block clamp; 300 source
    rows, random idx with repeats. Pack is bit-equal to ref.pack_rows
    with and without a power-of-two scale; scatter is exact (E)."""
    ext = _ext()
    g = gen(9200 + F)
    slots = n * (F // 4 if F % 4 == 0 else F)
    assert slots > 4096 * 256
    x = torch.randn(300, F, generator=g)
    idx = torch.randint(0, 300, (n,), generator=g)
    pow2 = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0])[
        torch.randint(0, 5, (n,), generator=g)]
    src = ints((n, F), g)
    base = ints((300, F), g)
    xg, ig, sg, bg = cu(x), cu(idx), cu(src), cu(base)
    for scale in (None, pow2):
        tag = f"n={n} F={F} scale={'pow2' if scale is not None else None}"
        got = ext.pack_rows(xg, ig, cu(scale)).cpu()
        assert torch.equal(got, ref.pack_rows(x, idx, scale)), \
            f"pack_rows {tag}"
        want = ref.scatter_add_rows(dbl(base).clone(), idx, dbl(src),
                                    dbl(scale))
        want_abs = ref.scatter_add_rows(dbl(base).abs(), idx, dbl(src).abs(),
                                        dbl(scale))
        out = bg.clone()
        ext.scatter_add_rows(out, ig, sg, cu(scale))
        assert_exact(out, want, want_abs, f"scatter_add_rows {tag}")


def check_bincount_wrapped():
    n, bins = 1_100_000, 150
    assert n > 4096 * 256
    g = gen(9300)
    v = torch.randint(0, bins, (n,), generator=g)
    v[torch.randperm(n, generator=g)[:n // 4]] = 7
    got = _ext().bincount_i32(cu(v.int()), bins).cpu()
    want = torch.bincount(v, minlength=bins)
    assert want[7] > n // 4
    assert torch.equal(got, want), (got - want).abs().max()


def check_syncbn_stats_wrapped(n, F):
    """2048 row chunks with rows_per > 256 (the last chunks can start
    beyond n); both output rows exact (E)."""
    assert (n + 255) // 256 > 2048
    x = ints((n, F), gen(9400 + F))
    xd = dbl(x)
    want = torch.stack((xd.sum(0), (xd * xd).sum(0)))
    want_abs = torch.stack((xd.abs().sum(0), (xd * xd).sum(0)))
    assert_exact(_ext().syncbn_stats(cu(x)), want, want_abs,
                 f"syncbn_stats n={n} F={F}")


def check_attn_project_wrapped(n, H, D):
    """attn_project forward and all three gradients with integer inputs
    (E): n beyond the 65,536-wave grid (and, at n > 524,288, the dattn
    kernel's 2048 row chunks)."""
    from bnsgcn_amd.ops import functional as BF
    assert n > 65536
    g = gen(9500 + 10 * H + D)
    z, al, ar = ints((n, H, D), g), ints((1, H, D), g), ints((1, H, D), g)
    g_el, g_er = ints((n, H), g), ints((n, H), g)
    zg, alg, arg = (cu(t).requires_grad_(True) for t in (z, al, ar))
    el, er = BF.attn_project(zg, alg, arg)
    (el * cu(g_el) + er * cu(g_er)).sum().backward()
    tag = f"attn_project n={n} (H,D)=({H},{D})"
    wel, wer = ref.attn_project(dbl(z), dbl(al), dbl(ar))
    ael, aer = ref.attn_project(dbl(z).abs(), dbl(al).abs(), dbl(ar).abs())
    assert_exact(el, wel, ael, tag + " el")
    assert_exact(er, wer, aer, tag + " er")
    want = ref.attn_project_backward(dbl(z), dbl(al), dbl(ar), dbl(g_el),
                                     dbl(g_er))
    want_abs = ref.attn_project_backward(dbl(z).abs(), dbl(al).abs(),
                                         dbl(ar).abs(), dbl(g_el).abs(),
                                         dbl(g_er).abs())
    for name, got, w, a in zip(("dz", "dal", "dar"),
                               (zg.grad, alg.grad, arg.grad), want, want_abs):
        assert_exact(got, w, a, f"{tag} {name}")


def sparse_rows(n_rows, n_cols, seed):
    """CSR with degrees 0..3 per row."""
    rng = np.random.default_rng(seed)
    return K._csr_from_degrees(rng.integers(0, 4, n_rows), n_cols, rng)


def check_softmax_wrapped(n_rows, H):
    """segment_softmax (+ backward) with n_rows * H beyond the 65,536
    waves of one pass: every row of the later passes is written and
    right (float64 reference, the project's softmax tolerance)."""
    from bnsgcn_amd.ops.functional import (segment_softmax_raw,
                                           segment_softmax_bwd_raw)
    assert n_rows * H > 65536
    ip, ix = sparse_rows(n_rows, 500, 9600 + H)
    g = gen(9600 + H)
    logits = 3 * torch.randn(ix.numel(), H, generator=g)
    want = ref.segment_softmax(ip, dbl(logits))
    got = segment_softmax_raw(cu(ip), cu(logits))
    tag = f"segment_softmax rows={n_rows} H={H}"
    assert_softmax_close(got, want, tag)
    a32 = want.float()
    ga = torch.randn(logits.shape, generator=g)
    want_b = ref.segment_softmax_backward(ip, dbl(a32), dbl(ga))
    got_b = segment_softmax_bwd_raw(cu(ip), cu(a32), cu(ga))
    assert_softmax_close(got_b, want_b, tag + " bwd")


def check_softmax2_wrapped(n_rows, H, form):
    """Union softmax + backward beyond the first pass of the grid of the
    kernel form that H selects: 'general' is a wave per (row, head) on
    65,536 waves, 'h4' a wave per row on 262,144."""
    items, waves = {"general": (n_rows * H, 65536),
                    "h4": (n_rows, 262144)}[form]
    assert items > waves and (form == "h4") == (H == 4)
    from bnsgcn_amd.ops.functional import (segment_softmax2_raw,
                                           segment_softmax2_bwd_raw)
    ip1, ix1 = sparse_rows(n_rows, 500, 9700 + H)
    ip2, ix2 = sparse_rows(n_rows, 500, 9750 + H)
    g = gen(9700 + H)
    l1 = 3 * torch.randn(ix1.numel(), H, generator=g)
    l2 = 3 * torch.randn(ix2.numel(), H, generator=g)
    tag = f"segment_softmax2 rows={n_rows} H={H}"
    w1, w2 = ref.segment_softmax2(ip1, dbl(l1), ip2, dbl(l2))
    g1, g2 = segment_softmax2_raw(cu(ip1), cu(l1), cu(ip2), cu(l2))
    assert_softmax_close(g1, w1, tag + " set1")
    assert_softmax_close(g2, w2, tag + " set2")
    a1, a2 = w1.float(), w2.float()
    ga = torch.randn(l1.shape, generator=g)
    gb = torch.randn(l2.shape, generator=g)
    wd1, wd2 = ref.segment_softmax2_backward(ip1, dbl(a1), dbl(ga),
                                             ip2, dbl(a2), dbl(gb))
    gd1, gd2 = segment_softmax2_bwd_raw(cu(ip1), cu(a1), cu(ga),
                                        cu(ip2), cu(a2), cu(gb))
    assert_softmax_close(gd1, wd1, tag + " bwd set1")
    assert_softmax_close(gd2, wd2, tag + " bwd set2")


def check_spmm_edge_scalar_wrapped(n_rows=22000, H=3, D=5):
    """Scalar spmm_edge (D % 4 != 0) with n_rows * H beyond 65,536 waves,
    integer w and x (E), with and without out=."""
    from bnsgcn_amd.ops.functional import spmm_edge_raw
    assert n_rows * H > 65536 and D % 4
    n_cols = 500
    ip, ix = sparse_rows(n_rows, n_cols, 9800)
    g = gen(9800)
    w = ints((ix.numel(), H), g)
    x = ints((n_cols, H, D), g)
    base = ints((n_rows, H, D), g)
    want = ref.spmm_edge_sum(ip, ix, dbl(w), dbl(x))
    want_abs = ref.spmm_edge_sum(ip, ix, dbl(w).abs(), dbl(x).abs())
    ipg, ixg = cu(ip), cu(ix)
    junk = torch.full((n_rows, H, D), float("nan"), device=DEV)
    torch.cuda.synchronize()
    del junk
    got = spmm_edge_raw(ipg, ixg, cu(w), cu(x))
    assert_exact(got, want, want_abs, "spmm_edge scalar wrapped")
    got = spmm_edge_raw(ipg, ixg, cu(w), cu(x), out=cu(base).clone())
    assert_exact(got, want + dbl(base), want_abs + dbl(base).abs(),
                 "spmm_edge scalar wrapped out=")


# ---------------------------------------------------------- script mode

def _case_linear_hip():
    for (M, Kd, N) in LINEAR_SHAPES:
        for bias in (True, False):
            check_linear(M, Kd, N, bias, expect_mode="hip")


# case name -> (environment switch, runner)
CASES = {
    "linear_hip": ({"BNSGCN_GEMM": "hip"}, _case_linear_hip),
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
