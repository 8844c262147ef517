"""Check functions for tests/test_gpu_agg_bf16.py and
tests/test_agg_bf16_cpu.py: --agg-dtype bf16, the bf16-source forms of the
GCN/SAGE SpMM, the cast kernel and the bf16-source pack.

The feature's one rule: the source operand of an aggregation is rounded
once to bf16, round to nearest even; scales, products, sums and outputs
stay fp32. So every oracle here is float64 ops/reference.py (or the
project's CPU path in float64) on q(x) = x.bfloat16().double(), where the
rounding is torch's CPU cast, never the kernel under test — and because
bf16 -> fp32 is exact, the fp32 bound of tests/kernel_path_checks.py,
(n_terms + 8) * 2^-23 * ref_abs, is the derived bound, unchanged. An fp32
aggregation of the UNROUNDED x misses that bound on most elements, so the
sweeps fail when the rounding is left out, as they do without the kernels.

Graphs, generators and the bound are those of kernel_path_checks.py,
narrow_spmm_checks.py, rowgroup_checks.py and partition_path_checks.py.
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import kernel_path_checks as K  # noqa: E402
import partition_path_checks as P  # noqa: E402
import sparse_sweep_checks as S  # noqa: E402
from kernel_path_checks import (DEV, N_COLS, N_ROWS, assert_sum_bound, cu,  # noqa: E402
                                dbl, degrees, gen)
from bnsgcn_amd.ops import reference as ref  # noqa: E402

BF16 = torch.bfloat16
# narrow (f4 <= 16), half-wave (f4 <= 32), full-wave, second pass (f4 > 128)
SWEEP_F = (4, 8, 12, 44, 64, 68, 128, 132, 256, 260, 516)
FALLBACK_F = (6, 5)             # F % 4 != 0: upcast copy, fp32 kernels
GROUPED_GRAPHS = ("fixture", "zipf", "hubcol", "lastrow")
GROUPED_GSEGS = (1, 65, None)
GROUPED_WIDTHS = (132, 256, 260, 516)
STEP_FLOOR = 2.0 ** -8          # one bf16 ulp of a flipped term


def q(x):
    """The rule's rounding by torch's CPU cast, kept in x's dtype."""
    return x.float().bfloat16().to(x.dtype)


def _nan_junk(*shape):
    junk = torch.full(shape, float("nan"), device=DEV)
    torch.cuda.synchronize()
    del junk


# ------------------------------------------------------------------ cast

def crafted_rows():
    """fp32 values around everything the rounding can get wrong: exact
    ties to even both ways (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6), one
    fp32 ulp either side of each tie, +-0, +-inf, NaN, fp32 denormals, the
    smallest normal, the largest finite fp32 (-> inf) and the largest
    value that stays finite."""
    def bits(*words):
        return torch.tensor(words, dtype=torch.int64).to(torch.int32) \
            .view(torch.float32)
    tie_dn, tie_up = 0x3f808000, 0x3f818000      # 1 + 2^-8, 1 + 3 * 2^-8
    v = bits(tie_dn, tie_dn - 1, tie_dn + 1, tie_up, tie_up - 1, tie_up + 1,
             tie_dn | 0x80000000, tie_up | 0x80000000,
             0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000,
             0x7f800001, 0xffc12345,
             0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x007fffff,
             0x80008000, 0x00800000, 0x7f7fffff, 0xff7fffff, 0x7f7f7fff,
             0x7f7f8000)
    return v


def assert_cast_equal(x_cpu):
    """cast_bf16 (through round_bf16_raw) == torch's CPU cast bit for bit;
    NaNs are compared as NaNs (the vectorised and the scalar CPU casts
    already differ in the payload they give)."""
    from bnsgcn_amd.ops.functional import round_bf16_raw
    got = round_bf16_raw(cu(x_cpu))
    assert got.dtype == BF16 and got.is_cuda and got.shape == x_cpu.shape
    got = got.cpu()
    want = x_cpu.to(BF16)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    gb, wb = got.view(torch.int16), want.view(torch.int16)
    bad = (gb != wb) & ~nan
    assert not bad.any(), (
        f"{int(bad.sum())} of {bad.numel()} differ; first: "
        f"x={x_cpu[bad][:4].view(torch.int32).tolist()} "
        f"got={gb[bad][:4].tolist()} want={wb[bad][:4].tolist()}")


def check_cast():
    v = crafted_rows()
    # as one row, as a column (tail path: n % 4 != 0), and tiled so the
    # crafted values fall on every lane position of the vector path
    assert_cast_equal(v[None, :])
    assert_cast_equal(v[:, None].contiguous())
    assert_cast_equal(v[:25][None, :].contiguous())
    assert_cast_equal(torch.stack([torch.roll(v, k) for k in range(4)]))
    for shape, seed in (((257, 44), 1), ((3, 5), 2), ((0, 8), 3)):
        x = torch.randn(*shape, generator=gen(600 + seed))
        # spread over the exponent range, denormals included
        x = x * torch.exp2(torch.randint(-140, 120, shape,
                                         generator=gen(610 + seed)).float())
        assert_cast_equal(x)
    # a contiguous view whose base is not 16-byte aligned
    from bnsgcn_amd.ops.functional import round_bf16_raw
    x = torch.randn(9, 5, generator=gen(620))
    xg = cu(x)
    view = xg.view(-1)[5:].view(8, 5)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    assert torch.equal(round_bf16_raw(view).cpu(), x[1:].to(BF16))


# ---------------------------------------------------------- kernel sweep

def _sweep_case(indptr, indices, n_src, F, seed, label):
    """One graph and width: bf16-source spmm_sum_raw with and without the
    scales, overwrite (NaN-prefilled memory) and out= accumulate, against
    float64 on q(x) under assert_sum_bound; then the distance to the
    fp32-source result. Returns the worst err/bound."""
    from bnsgcn_amd.ops.functional import round_bf16_raw, spmm_sum_raw
    n_dst = indptr.numel() - 1
    deg = degrees(indptr)
    g = gen(seed + F)
    x = torch.randn(n_src, F, generator=g)
    ss = torch.rand(n_src, generator=g) + 0.5
    ds = torch.rand(n_dst, generator=g) + 0.5
    base = torch.randn(n_dst, F, generator=g)
    xq = x.to(BF16).double()
    ip, ix = cu(indptr), cu(indices)
    xb = round_bf16_raw(cu(x))
    assert xb.dtype == BF16
    worst = 0.0
    for scales, acc in S.ALL_VARIANTS:
        s_, d_ = (dbl(ss), dbl(ds)) if scales else (None, None)
        want = ref.spmm_sum(indptr, indices, xq, s_, d_,
                            dbl(base).clone() if acc else None)
        want_abs = ref.spmm_sum(indptr, indices, xq.abs(), s_, d_,
                                dbl(base).abs() if acc else None)
        if not acc:
            _nan_junk(n_dst, F)
        got = spmm_sum_raw(ip, ix, xb, cu(ss) if scales else None,
                           cu(ds) if scales else None,
                           cu(base).clone() if acc else None)
        what = f"bf16 spmm_sum {label} F={F} scales={scales} acc={acc}"
        assert got.dtype == torch.float32
        worst = max(worst, assert_sum_bound(got, want, want_abs, deg[:, None],
                                            what))
        if not acc:
            assert (got.cpu()[deg == 0] == 0).all(), f"{what}: empty rows"
        # against the fp32-source float64 result: each term moved by at
        # most half a bf16 ulp, 2^-8 of its size, and it did move
        full = ref.spmm_sum(indptr, indices, dbl(x), s_, d_,
                            dbl(base).clone() if acc else None)
        full_abs = ref.spmm_sum(indptr, indices, dbl(x).abs(), s_, d_,
                                dbl(base).abs() if acc else None)
        diff = (got.double().cpu() - full).abs()
        ratio = float((diff / full_abs.clamp_min(1e-300)).max())
        print(f"{what}: max |bf16 - fp32 source| / agg|x| = {ratio:.4g}")
        assert (diff <= 2.0 ** -8 * full_abs).all(), (what, ratio)
        assert not torch.equal(got.double().cpu(), full), \
            f"{what}: equals the fp32-source result"
    return worst


def check_sweep(F):
    """fixture_csr (forward shape) and its transpose (the backward's)."""
    import narrow_spmm_checks as NS
    indptr, indices = K.fixture_csr()
    tip, tix = NS.transposed_fixture_csr()
    w = _sweep_case(indptr, indices, N_COLS, F, 5100, "fixture")
    w = max(w, _sweep_case(tip, tix, N_ROWS, F, 5200, "transposed"))
    return w


def cpu_oracle_figures(F):
    """What the docstring of this module claims, computed on the CPU: the
    largest err/bound of an fp32 reference on rounded inputs, and the
    fraction of elements on which an fp32 aggregation of the unrounded x
    misses the bound."""
    indptr, indices = K.fixture_csr()
    deg = degrees(indptr)[:, None]
    x = torch.randn(N_COLS, F, generator=gen(5100 + F))
    xq = x.to(BF16)
    want = ref.spmm_sum(indptr, indices, xq.double())
    want_abs = ref.spmm_sum(indptr, indices, xq.double().abs())
    bound = (deg + 8.0) * K.EPS * want_abs
    live = want_abs > 0
    on_q = ref.spmm_sum(indptr, indices, xq.float()).double()
    on_x = ref.spmm_sum(indptr, indices, x).double()
    ok = float(((on_q - want).abs()[live] / bound[live]).max())
    miss = float(((on_x - want).abs()[live] > bound[live]).double().mean())
    return ok, miss


# --------------------------------------------------------------- grouped

def check_grouped_sweep(name, R):
    """rowgroup_checks.check_grouped_sweep with a bf16 source: every call
    reaches the grouped binding with a bf16 x."""
    import rowgroup_checks as RG
    from bnsgcn_amd.ops.functional import round_bf16_raw, spmm_sum_raw
    indptr, indices, n_cols = RG.graph(name)
    n_rows = indptr.numel() - 1
    deg = degrees(indptr)
    worst = 0.0
    for F in GROUPED_WIDTHS:
        g = gen(5300 + F)
        x = torch.randn(n_cols, F, generator=g)
        ss = torch.rand(n_cols, generator=g) + 0.5
        ds = torch.rand(n_rows, generator=g) + 0.5
        base = torch.randn(n_rows, F, generator=g)
        xq = x.to(BF16).double()
        refs = {}
        for scales in (False, True):
            s_, d_ = (dbl(ss), dbl(ds)) if scales else (None, None)
            refs[scales] = (ref.spmm_sum(indptr, indices, xq, s_, d_),
                            ref.spmm_sum(indptr, indices, xq.abs(), s_, d_))
        xb, ssg, dsg, bg = round_bf16_raw(cu(x)), cu(ss), cu(ds), cu(base)
        for gseg in GROUPED_GSEGS:
            ip, ix = RG.device_csr(name, R, gseg)
            for scales, acc in S.ALL_VARIANTS:
                want, want_abs = refs[scales]
                if acc:
                    want = want + dbl(base)
                    want_abs = want_abs + dbl(base).abs()
                else:
                    _nan_junk(n_rows, F)
                with spy_spmm() as calls:
                    got = spmm_sum_raw(ip, ix, xb, ssg if scales else None,
                                       dsg if scales else None,
                                       bg.clone() if acc else None)
                what = (f"bf16 grouped {name} R={R} gseg={gseg} F={F} "
                        f"scales={scales} acc={acc}")
                assert [(c["kind"], c["dtype"]) for c in calls] == \
                    [("grouped", BF16)], f"{what}: {calls}"
                worst = max(worst, assert_sum_bound(
                    got, want, want_abs, deg[:, None], what))
                if not acc:
                    assert (got.cpu()[deg == 0] == 0).all(), \
                        f"{what}: empty rows not zero"
    return worst


def check_grouped_isolation(R):
    """rowgroup_checks.check_isolation with a bf16 source: the cast keeps
    inf and NaN, and they stay in the one row that has the edge."""
    import rowgroup_checks as RG
    from bnsgcn_amd.ops.functional import round_bf16_raw, spmm_sum_raw
    indptr, indices, n_cols = RG.graph("isolate")
    n_rows = indptr.numel() - 1
    others = torch.arange(n_rows) != 5
    deg = degrees(indptr)[others, None]
    for F in (132, 256):
        g = gen(5400 + F)
        x = torch.randn(n_cols, F, generator=g)
        ss = torch.rand(n_cols, generator=g) + 0.5
        ds = torch.rand(n_rows, generator=g) + 0.5
        xq = x.to(BF16).double()
        want = ref.spmm_sum(indptr, indices, xq, dbl(ss), dbl(ds))[others]
        want_abs = ref.spmm_sum(indptr, indices, xq.abs(), dbl(ss),
                                dbl(ds))[others]
        for bad in (float("inf"), float("nan")):
            xbad = x.clone()
            xbad[33] = bad
            xb = round_bf16_raw(cu(xbad))
            assert not torch.isfinite(xb[33].float()).any()
            for gseg in (1, None):
                ip, ix = RG.device_csr("isolate", R, gseg)
                with spy_spmm() as calls:
                    got = spmm_sum_raw(ip, ix, xb, cu(ss), cu(ds))
                assert [(c["kind"], c["dtype"]) for c in calls] == \
                    [("grouped", BF16)]
                assert not torch.isfinite(got[5]).any()
                assert_sum_bound(got[others], want, want_abs, deg,
                                 f"bf16 isolation R={R} F={F} x[33]={bad} "
                                 f"gseg={gseg}")


# ----------------------------------------------------------- determinism

def check_deterministic_per_row(F):
    """SEG above every degree: no split row, one writer per row and a
    fixed order of terms, so two bf16 calls agree bitwise."""
    from bnsgcn_amd.ops.csr_torch import build_worklist
    from bnsgcn_amd.ops.functional import round_bf16_raw, spmm_sum_raw
    for name in ("fixture", "zipf"):
        indptr, indices, n_cols = S.graph(name)
        ip, ix = cu(indptr).clone(), cu(indices)
        ip._bns_worklist = build_worklist(ip, seg=1 << 20)
        assert int((ip._bns_worklist[0] < 0).sum()) == 0
        g = gen(5500 + F)
        xb = round_bf16_raw(cu(torch.randn(n_cols, F, generator=g)))
        ss = cu(torch.rand(n_cols, generator=g) + 0.5)
        ds = cu(torch.rand(indptr.numel() - 1, generator=g) + 0.5)
        with spy_spmm() as calls:
            a = spmm_sum_raw(ip, ix, xb, ss, ds)
            b = spmm_sum_raw(ip, ix, xb, ss, ds)
        assert [(c["kind"], c["dtype"]) for c in calls] == \
            [("per-row", BF16)] * 2
        assert torch.equal(a, b), f"{name} F={F}: two bf16 calls differ"


def check_deterministic_grouped(R, F=256):
    import rowgroup_checks as RG
    from bnsgcn_amd.ops.functional import round_bf16_raw, spmm_sum_raw
    for name in ("fixture", "zipf"):
        indptr, indices, n_cols = RG.graph(name)
        ip, ix = RG.device_csr(name, R, 1 << 20)
        assert int((ip._bns_rowgroups.sched[0] < 0).sum()) == 0
        g = gen(5600 + F)
        xb = round_bf16_raw(cu(torch.randn(n_cols, F, generator=g)))
        ss = cu(torch.rand(n_cols, generator=g) + 0.5)
        ds = cu(torch.rand(indptr.numel() - 1, generator=g) + 0.5)
        with spy_spmm() as calls:
            a = spmm_sum_raw(ip, ix, xb, ss, ds)
            b = spmm_sum_raw(ip, ix, xb, ss, ds)
        assert [(c["kind"], c["dtype"]) for c in calls] == \
            [("grouped", BF16)] * 2
        assert torch.equal(a, b), f"{name} R={R}: two bf16 calls differ"


# ------------------------------------------------------------------ pack

def check_pack(F):
    """bf16-source pack_rows == xb.float()[idx] * scale[:, None] exactly
    (one fp32 multiply): repeated indices, n = 0, with and without scale."""
    from bnsgcn_amd.ops.functional import pack_rows_raw, round_bf16_raw
    g = gen(5700 + F)
    x = torch.randn(37, F, generator=g)
    xb = round_bf16_raw(cu(x))
    xf = x.to(BF16).float()
    for n in (0, 1, 90):
        idx = torch.randint(0, 37, (n,), generator=g)
        if n == 90:
            idx[::3] = 36                # repeats, and the last row
            assert idx.unique().numel() < n
        scale = torch.rand(n, generator=g) * 9 + 0.1
        for sc in (None, scale):
            got = pack_rows_raw(xb, cu(idx), cu(sc))
            assert got.dtype == torch.float32 and got.shape == (n, F)
            want = xf[idx] if sc is None else xf[idx] * sc[:, None]
            assert torch.equal(got.cpu(), want), f"pack F={F} n={n} sc={sc is not None}"


# ------------------------------------------------------------- call spy

@contextlib.contextmanager
def spy_spmm():
    """Records every launch of the two SpMM bindings of the extension, in
    the manner of rowgroup_checks.count_grouped: kind, the data pointer of
    the column array (indices / ecol) that names the CSR, the source dtype
    and the current `phase` tag (spy_spmm.phase)."""
    from bnsgcn_amd.ops._ext import require_ext
    ext = require_ext()
    orig = (ext.spmm_sum, ext.spmm_sum_grouped)
    calls = []

    def per_row(wrow, wbeg, wend, ws, indices, x, *rest):
        calls.append({"kind": "per-row", "csr": indices.data_ptr(),
                      "dtype": x.dtype, "phase": spy_spmm.phase})
        return orig[0](wrow, wbeg, wend, ws, indices, x, *rest)

    def grouped(wg, wbeg, wend, ws, ecol, ew, x, *rest):
        calls.append({"kind": "grouped", "csr": ecol.data_ptr(),
                      "dtype": x.dtype, "phase": spy_spmm.phase})
        return orig[1](wg, wbeg, wend, ws, ecol, ew, x, *rest)
    ext.spmm_sum, ext.spmm_sum_grouped = per_row, grouped
    try:
        yield calls
    finally:
        ext.spmm_sum, ext.spmm_sum_grouped = orig


spy_spmm.phase = None


# -------------------------------------------------------- partition path

def run_aggregate(part, device, dtype, x, g, mode, rate, agg_dtype, epoch=3,
                  rows=None, absolute=False):
    """partition_path_checks.run_aggregate with ctx.agg_dtype set."""
    from bnsgcn_amd.models.context import GraphContext
    plan = P.make_plan(part, rate, device)
    st = plan.set_epoch(epoch)
    P.assert_halo_preconditions(plan, st, want_empty_row=rate < 1.0, rows=rows)
    ctx = GraphContext.for_partition(part, plan, device, need_eperm=False)
    assert ctx.agg_dtype is None         # the default changes nothing
    ctx.agg_dtype = agg_dtype
    r = None
    if rows is not None:
        r = rows.to(device)
        ctx.loss_rows = r
    if absolute:
        x, g = x.abs(), g.abs()
    xd = x.to(device=device, dtype=dtype).requires_grad_(True)
    gd = g.to(device=device, dtype=dtype)
    with P.installed(P.StubExchange(absolute)) as stub:
        out = ctx.aggregate(xd, mode, rows=r)
        out.backward(gd)
        P.sync(device)
    assert len(stub.log) == 2, len(stub.log)
    return {"out": out.detach().cpu(), "gx": xd.grad.cpu(),
            "pack": stub.log[0][0].cpu(), "gr": stub.log[1][0].cpu(),
            "st": st}


def check_partition_aggregate(mode, F, with_rows, monkeypatch):
    """Every rank of the 3-partition fixture, rate 0.4, ctx.agg_dtype =
    bf16, the overlap branch and BNSGCN_NO_OVERLAP=1: out, x.grad and the
    recorded gr against the same path on the CPU in float64 from the same
    fp32 x, g and stub rows, under assert_sum_bound with term_counts; the
    recorded forward send exactly q(x)[pack_idx] * pack_scale."""
    _, parts = P.fixture_parts(3)
    for part in parts:
        rows = None
        if with_rows:
            rows = torch.from_numpy(np.flatnonzero(part.train_mask))
            assert 0 < rows.numel() < part.n_inner
        x = torch.randn(part.n_inner, F, generator=gen(5800 + 10 * part.rank + F))
        g_rows = part.n_inner if rows is None else rows.numel()
        g = torch.randn(g_rows, F, generator=gen(5900 + 10 * part.rank + F))
        kw = dict(mode=mode, rate=0.4, agg_dtype=BF16, rows=rows)
        monkeypatch.delenv("BNSGCN_NO_OVERLAP", raising=False)
        r64 = run_aggregate(part, "cpu", torch.float64, x, g, **kw)
        rabs = run_aggregate(part, "cpu", torch.float64, x, g, absolute=True,
                             **kw)
        # the float64 run follows the rule: its send is q(x) gathered (the
        # float64 product is exact, the fp32 one is rounded once)
        st = r64["st"]
        want_pack = x.to(BF16).float()[st.pack_idx] * st.pack_scale[:, None]
        assert torch.equal(r64["pack"], x.to(BF16).double()[st.pack_idx]
                           * st.pack_scale.double()[:, None])
        plain = run_aggregate(part, "cpu", torch.float64, x, g,
                              **dict(kw, agg_dtype=None))
        assert not torch.equal(plain["out"], r64["out"])
        assert not torch.equal(plain["gx"], r64["gx"])
        n_out, n_gx, n_gr = P.term_counts(part, st, rows)
        for no_overlap in (False, True):
            if no_overlap:
                monkeypatch.setenv("BNSGCN_NO_OVERLAP", "1")
            with spy_spmm() as calls:
                got = run_aggregate(part, DEV, torch.float32, x, g, **kw)
            monkeypatch.delenv("BNSGCN_NO_OVERLAP", raising=False)
            tag = (f"bf16 agg rank {part.rank} {mode} F={F} rows={with_rows} "
                   f"no_overlap={no_overlap}")
            # inner fwd, halo fwd (fp32 recv), halo bwd, inner bwd
            assert sorted(str(c["dtype"]) for c in calls) == sorted(
                [str(BF16)] * 3 + [str(torch.float32)]), (tag, calls)
            assert got["pack"].dtype == got["gr"].dtype == torch.float32
            assert torch.equal(got["pack"], want_pack), f"{tag} pack"
            for key, n in (("out", n_out), ("gr", n_gr), ("gx", n_gx)):
                assert_sum_bound(got[key], r64[key], rabs[key], n,
                                 f"{tag} {key}")


# --------------------------------------------------------- training step

def compare_measured_floor(ref64, ref32, got, tag, floor=STEP_FLOOR):
    """partition_path_checks.compare_measured with the floor of the
    tolerance at 2^-8 instead of 1e-5: past the first aggregation the GPU
    and CPU inputs of a rounding differ by fp32 rounding, a value on a bf16
    boundary can round the other way, and one such flip moves a term by a
    bf16 ulp. (The sharp numeric checks are the sweeps and the partition
    path; liveness of the flag is asserted on the calls.)"""
    assert ref64.keys() == ref32.keys() == got.keys(), (
        sorted(ref64.keys() ^ got.keys()), sorted(ref64.keys() ^ ref32.keys()))
    failures = []
    for name, r64 in ref64.items():
        r64 = r64.double()
        g_, r32 = got[name].double(), ref32[name].double()
        assert g_.shape == r64.shape == r32.shape, (name, g_.shape, r64.shape)
        assert torch.isfinite(g_).all(), f"{tag} {name}: non-finite"
        scale = float(r64.abs().max()) if r64.numel() else 0.0
        if scale == 0.0:
            assert not g_.any(), f"{tag} {name}: reference is all zero"
            continue
        e32 = float((r32 - r64).abs().max()) / scale
        egot = float((g_ - r64).abs().max()) / scale
        tol = max(8 * e32, floor)
        print(f"{tag} {name}: fp32-cpu rel err {e32:.3g}, "
              f"got rel err {egot:.3g}, tol {tol:.3g}")
        if not egot <= tol:
            failures.append((name, egot, tol))
    assert not failures, (tag, failures)


def run_step_spied(part, g, args, device, dtype):
    """partition_path_checks.run_training_step with the SpMM bindings
    spied on. Returns (results, calls, inner) where `inner` is the set of
    column-array pointers of the context's inner CSRs (forward,
    transposed, their loss-row forms and row-group forms) and each call
    carries phase "pp" when RankState.precompute made it."""
    import bnsgcn_amd.runtime.trainer as trainer
    made = []

    class Recorded(trainer.RankState):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

        def precompute(self):
            spy_spmm.phase = "pp"
            try:
                return super().precompute()
            finally:
                spy_spmm.phase = None

    with pytest.MonkeyPatch.context() as mp, spy_spmm() as calls:
        mp.setattr(trainer, "RankState", Recorded)
        res = P.run_training_step(part, g, args, device, dtype)
    ctx = made[0].ctx
    csrs = [(ctx.indptr, ctx.indices), (ctx.t_indptr, ctx.t_indices)]
    if ctx._rows_static is not None:
        ip, ix, tip, tix = ctx._rows_static
        csrs += [(ip, ix), (tip, tix)]
    inner = set()
    for ip, ix in csrs:
        inner.add(ix.data_ptr())
        rg = getattr(ip, "_bns_rowgroups", None)
        if rg is not None:
            inner.add(rg.ecol.data_ptr())
    inner.discard(0)
    return res, calls, inner


def check_training_step(model, use_pp, rank):
    g, parts = P.fixture_parts(3)
    part = parts[rank]
    args = P.step_args(model, use_pp)
    assert args.agg_dtype == "fp32"
    tag = f"bf16 step {model} use_pp={use_pp} rank {rank}"
    _, calls32, inner32 = run_step_spied(part, g, args, DEV, torch.float32)
    args.agg_dtype = "bf16"
    ref64 = P.run_training_step(part, g, args, "cpu", torch.float64)
    ref32 = P.run_training_step(part, g, args, "cpu", torch.float32)
    got, calls, inner = run_step_spied(part, g, args, DEV, torch.float32)
    compare_measured_floor(ref64, ref32, got, tag)

    def agg_inner(cs, ptrs):
        return [c for c in cs if c["csr"] in ptrs and c["phase"] != "pp"]
    a16, a32 = agg_inner(calls, inner), agg_inner(calls32, inner32)
    # 2 aggregating layers at least, forward in train and in eval, and the
    # backward of every layer whose input needs a gradient
    assert len(a16) >= 5 and len(a16) == len(a32), (tag, len(a16), len(a32))
    assert all(c["dtype"] == BF16 for c in a16), (tag, a16)
    assert all(c["dtype"] == torch.float32 for c in calls32), (tag, calls32)
    # the one-time use_pp precompute stays fp32
    pp = [c for c in calls if c["phase"] == "pp"]
    assert (len(pp) > 0) == bool(use_pp)
    assert all(c["dtype"] == torch.float32 for c in pp), (tag, pp)
