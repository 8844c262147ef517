"""Format contract and check functions for tests/test_rowgroup_cpu.py and
tests/test_gpu_rowgroup_spmm.py: the row-group form of a static CSR
(ops/csr_torch.build_rowgroups) and spmm_sum_grouped_kernel behind
ops.functional.spmm_sum_raw.

Graphs are the family of tests/sparse_sweep_checks.py plus `dup256`, one
row that repeats one column 256 times (the uint8 weight field's maximum
+ 1). A format is selected without a child process by storing
`build_rowgroups(...)` in the `_bns_rowgroups` attribute of a device
`indptr`, the cache spmm_sum_raw reads; that bypasses the keep rule of
attach_rowgroups, which these small graphs would not pass.

Oracle and tolerance are those of tests/kernel_path_checks.py: float64
ops/reference.py on the same fp32 inputs, never another GPU kernel;
assert_sum_bound with n_terms = the row's edge count, duplicates counted.
The grouped kernel adds a duplicate edge as one term (count * scale) * x,
which is fewer roundings than the bound allows for.

Run as a script (`python tests/rowgroup_checks.py group_off`) it executes
the BNSGCN_SPMM_GROUP=0 case in a fresh process (the switch is read once,
at import).
"""
from __future__ import annotations

import contextlib
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sparse_sweep_checks as S  # noqa: E402
from kernel_path_checks import (DEV, assert_sum_bound, cu, dbl,  # noqa: E402
                                degrees, gen)
from bnsgcn_amd.ops import reference as ref  # noqa: E402

W_MAX = 255
RS = (4, 8)                             # every instantiated R
RS_BUILDER = (4, 8, 16)
GSEGS_CPU = (1, 3, 64, 65, 512)
GSEGS_GPU = (1, 3, 64, 65, None)        # None = the csr_torch default
CPU_GRAPHS = ("fixture", "zipf", "onerow", "lastrow", "tiny", "hubcol",
              "empty", "norows", "dup256")
GPU_GRAPHS = ("fixture", "zipf", "onerow", "lastrow", "tiny", "hubcol",
              "dup256")
WIDTHS = (132, 256, 260, 516)


@functools.lru_cache(maxsize=None)
def graph(name):
    """sparse_sweep_checks.graph plus
    dup256   one row, 256 edges, all to column 1 of 3
    isolate  16 rows x 40 columns, 6 random edges per row into columns
             0..29, and one extra edge row 5 -> column 33, which no other
             row has."""
    if name == "dup256":
        return (torch.tensor([0, W_MAX + 1]),
                torch.ones(W_MAX + 1, dtype=torch.int32), 3)
    if name == "isolate":
        rng = np.random.default_rng(20260)
        rows = [list(rng.integers(0, 30, 6)) for _ in range(16)]
        rows[5].insert(3, 33)
        deg = np.array([len(r) for r in rows], dtype=np.int64)
        flat = np.concatenate(rows).astype(np.int32)
        return (torch.from_numpy(np.concatenate([[0], np.cumsum(deg)])),
                torch.from_numpy(flat), 40)
    return S.graph(name)


# ------------------------------------------------------ format contract

def assert_rowgroup_contract(indptr, indices, n_cols, rg, R, gseg):
    """What spmm_sum_grouped_kernel relies on, and what the issue asks of
    the builder. Returns (n_entries, n_split_groups)."""
    indptr, indices = indptr.cpu(), indices.cpu()
    wgroup, wbeg, wend, ws = (t.cpu() for t in rg.sched)
    ecol, ew, zero_rows = rg.ecol.cpu(), rg.ew.cpu(), rg.zero_rows.cpu()
    n = indptr.numel() - 1
    E = indices.numel()
    deg = indptr[1:] - indptr[:-1]
    assert rg.R == R
    assert wgroup.dtype == torch.int32 and ws.dtype == torch.int32
    assert wbeg.dtype == torch.int64 and wend.dtype == torch.int64
    assert ecol.dtype == torch.int32 and ew.dtype == torch.uint8
    assert zero_rows.dtype == torch.int64
    n_ent = ecol.numel()
    assert ew.shape == (n_ent, R)
    assert rg.ratio == (n_ent / E if E else 1.0)
    total = wgroup.numel()
    assert wbeg.numel() == total and wend.numel() == total

    # schedule: n_waves % 8 == 0, monotone, ends at the item count
    n_waves = ws.numel() - 1
    assert n_waves % 8 == 0
    assert int(ws[0]) == 0 and int(ws[-1]) == total
    assert (ws[1:] >= ws[:-1]).all(), "wave_start not monotone"

    groups = torch.where(wgroup < 0, ~wgroup, wgroup).long()
    n_groups = (n + R - 1) // R
    split_groups = torch.zeros(n_groups, dtype=torch.bool)
    if total:
        # items tile [0, n_ent) without gap or overlap, <= gseg entries
        lens = wend - wbeg
        assert int(lens.min()) >= 1 and int(lens.max()) <= gseg
        assert int(wbeg[0]) == 0 and int(wend[-1]) == n_ent
        assert torch.equal(wbeg[1:], wend[:-1]), "items do not tile entries"
        assert int(groups.min()) >= 0 and int(groups.max()) < n_groups
        assert (groups[1:] >= groups[:-1]).all(), "group ids decrease"
        # split iff more than one item
        n_items = torch.bincount(groups, minlength=n_groups)
        assert torch.equal(wgroup < 0, n_items[groups] > 1), \
            "split mark != (group has more than one item)"
        split_groups = n_items > 1
    else:
        assert n_ent == 0 and E == 0

    # group of every entry, from the items
    egroup = torch.repeat_interleave(groups, wend - wbeg)
    assert egroup.numel() == n_ent
    assert (ecol >= 0).all() and (ecol < max(n_cols, 1)).all()
    assert (ew.max(1).values > 0).all() if n_ent else True, "all-zero entry"

    # columns strictly ascending within a group, except the repeats that
    # carry an overflowing count (the earlier copy holds a full field)
    same = egroup[1:] == egroup[:-1]
    dcol = ecol[1:].long() - ecol[:-1].long()
    assert (dcol[same] >= 0).all(), "columns not ascending within a group"
    rep = same & (dcol == 0)
    assert (ew[:-1][rep].max(1).values == W_MAX).all(), \
        "repeated column without a full weight field"

    # expanding reproduces the CSR's multiset of edges exactly
    e_idx, r_idx = torch.nonzero(ew, as_tuple=True)
    rows = egroup[e_idx] * R + r_idx
    assert (rows < n).all() if rows.numel() else True
    key = rows * max(n_cols, 1) + ecol[e_idx].long()
    got = torch.zeros(n * max(n_cols, 1), dtype=torch.int64)
    got.index_add_(0, key, ew[e_idx, r_idx].long())
    row_of_edge = torch.repeat_interleave(torch.arange(n), deg)
    want = torch.bincount(row_of_edge * max(n_cols, 1) + indices.long(),
                          minlength=n * max(n_cols, 1))
    assert torch.equal(got, want), "expanded format != CSR edge multiset"

    # zero_rows = rows of split groups + rows with no edge
    in_split = split_groups[torch.arange(n) // R] if n else \
        torch.zeros(0, dtype=torch.bool)
    want_zero = torch.nonzero(in_split | (deg == 0))[:, 0]
    assert torch.equal(zero_rows.sort().values, want_zero), \
        "zero_rows != rows of split groups + empty rows"
    return n_ent, int(split_groups.sum())


# -------------------------------------------------- device CSR + format

_DEV = {}


def device_csr(name, R, gseg):
    """(ip, ix) on the GPU with the row-group format (R, gseg) attached to
    a private copy of ip and checked against the contract; R None attaches
    nothing."""
    key = (name, R, gseg)
    if key not in _DEV:
        from bnsgcn_amd.ops import csr_torch
        indptr, indices, n_cols = graph(name)
        ip, ix = cu(indptr), cu(indices)
        if R is not None:
            rg = csr_torch.build_rowgroups(ip, ix, n_cols, R=R, gseg=gseg)
            assert_rowgroup_contract(indptr, indices, n_cols, rg, R,
                                     gseg or csr_torch.GSEG)
            ip._bns_rowgroups = rg
        _DEV[key] = (ip, ix)
    return _DEV[key]


@contextlib.contextmanager
def count_grouped():
    """Counts the launches of the grouped kernel's binding."""
    from bnsgcn_amd.ops._ext import require_ext
    ext = require_ext()
    orig, calls = ext.spmm_sum_grouped, [0]

    def spy(*a):
        calls[0] += 1
        return orig(*a)
    ext.spmm_sum_grouped = spy
    try:
        yield calls
    finally:
        ext.spmm_sum_grouped = orig


def _nan_junk(*shape):
    junk = torch.full(shape, float("nan"), device=DEV)
    torch.cuda.synchronize()
    del junk


# ---------------------------------------------------------------- sweep

def check_grouped_sweep(name, R, gsegs=GSEGS_GPU, widths=WIDTHS):
    """spmm_sum_raw on a CSR that carries the format: every width, with
    and without both scales, overwrite (from a NaN-prefilled allocation)
    and out= accumulate, every gseg; each call must reach the grouped
    binding. Empty rows of an overwrite come out exactly 0."""
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    indptr, indices, n_cols = graph(name)
    n_rows = indptr.numel() - 1
    deg = degrees(indptr)
    worst = 0.0
    for F in widths:
        g = gen(2300 + F)
        x = torch.randn(n_cols, F, generator=g)
        ss = torch.rand(n_cols, generator=g) + 0.5
        ds = torch.rand(n_rows, generator=g) + 0.5
        base = torch.randn(n_rows, F, generator=g)
        refs = {}
        for scales in (False, True):
            s_, d_ = (dbl(ss), dbl(ds)) if scales else (None, None)
            refs[scales] = (
                ref.spmm_sum(indptr, indices, dbl(x), s_, d_),
                ref.spmm_sum(indptr, indices, dbl(x).abs(), s_, d_))
        xg, ssg, dsg, bg = cu(x), cu(ss), cu(ds), cu(base)
        for gseg in gsegs:
            ip, ix = device_csr(name, R, gseg)
            for scales, acc in S.ALL_VARIANTS:
                want, want_abs = refs[scales]
                if acc:
                    want = want + dbl(base)
                    want_abs = want_abs + dbl(base).abs()
                else:
                    _nan_junk(n_rows, F)
                with count_grouped() as calls:
                    got = spmm_sum_raw(ip, ix, xg, ssg if scales else None,
                                       dsg if scales else None,
                                       bg.clone() if acc else None)
                what = (f"grouped {name} R={R} gseg={gseg} F={F} "
                        f"scales={scales} acc={acc}")
                assert calls[0] == 1, f"{what}: not routed to the grouped path"
                worst = max(worst, assert_sum_bound(
                    got, want, want_abs, deg[:, None], what))
                if not acc:
                    assert (got.cpu()[deg == 0] == 0).all(), \
                        f"{what}: empty rows not zero"
    print(f"grouped worst {name} R={R}: {worst:.3g}")
    return worst


# ------------------------------------------------------------ isolation

def check_isolation(R):
    """Column 33 is a neighbour of row 5 only. With x[33] = inf, then NaN,
    every other row stays finite and within the bound: a branch-free
    0 * x[33] would poison the rest of row 5's group."""
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    indptr, indices, n_cols = graph("isolate")
    n_rows = indptr.numel() - 1
    row_of_edge = torch.repeat_interleave(torch.arange(n_rows),
                                          indptr[1:] - indptr[:-1])
    assert row_of_edge[indices == 33].tolist() == [5]
    others = torch.arange(n_rows) != 5
    deg = degrees(indptr)[others, None]
    for F in (132, 256):
        g = gen(2400 + F)
        x = torch.randn(n_cols, F, generator=g)
        ss = torch.rand(n_cols, generator=g) + 0.5
        ds = torch.rand(n_rows, generator=g) + 0.5
        # column 33 reaches no other row: the reference of those rows does
        # not depend on x[33]
        want = ref.spmm_sum(indptr, indices, dbl(x), dbl(ss), dbl(ds))[others]
        want_abs = ref.spmm_sum(indptr, indices, dbl(x).abs(), dbl(ss),
                                dbl(ds))[others]
        for bad in (float("inf"), float("nan")):
            xb = x.clone()
            xb[33] = bad
            for gseg in (1, None):
                ip, ix = device_csr("isolate", R, gseg)
                with count_grouped() as calls:
                    got = spmm_sum_raw(ip, ix, cu(xb), cu(ss), cu(ds))
                assert calls[0] == 1
                assert not torch.isfinite(got[5]).any()
                assert_sum_bound(got[others], want, want_abs, deg,
                                 f"isolation R={R} F={F} x[33]={bad} "
                                 f"gseg={gseg}")


# ------------------------------------------------------ reproducibility

def check_reproducible(R):
    """No split group (gseg above every group's length): single-writer
    rows, fixed summation order, so two calls agree bitwise."""
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    for name in ("fixture", "zipf"):
        indptr, indices, n_cols = graph(name)
        ip, ix = device_csr(name, R, 1 << 20)
        assert int((ip._bns_rowgroups.sched[0] < 0).sum()) == 0
        g = gen(2500)
        x = cu(torch.randn(n_cols, 256, generator=g))
        ss = cu(torch.rand(n_cols, generator=g) + 0.5)
        ds = cu(torch.rand(indptr.numel() - 1, generator=g) + 0.5)
        with count_grouped() as calls:
            a = spmm_sum_raw(ip, ix, x, ss, ds)
            b = spmm_sum_raw(ip, ix, x, ss, ds)
        assert calls[0] == 2
        assert torch.equal(a, b), f"{name} R={R}: two calls differ"


# -------------------------------------------------------------- routing

def _per_row_direct(ip, ix, x, ss, ds):
    """The per-row kernel called as spmm_sum_raw calls it on a CSR without
    the format."""
    from bnsgcn_amd.ops._ext import require_ext
    from bnsgcn_amd.ops.functional import _worklist_of
    wrow, wbeg, wend, wave_start, zero_rows = _worklist_of(ip)
    out = torch.empty(ip.numel() - 1, x.shape[1], device=x.device)
    if zero_rows.numel():
        out.index_fill_(0, zero_rows, 0.0)
    return require_ext().spmm_sum(wrow, wbeg, wend, wave_start, ix, x, ss, ds,
                                  out, False)


def _routing_inputs(F):
    indptr, indices, n_cols = graph("fixture")
    g = gen(2600 + F)
    return (cu(torch.randn(n_cols, F, generator=g)),
            cu(torch.rand(n_cols, generator=g) + 0.5),
            cu(torch.rand(indptr.numel() - 1, generator=g) + 0.5))


def check_routing_no_attribute():
    """A CSR without the attribute runs the per-row kernel: bitwise equal
    to the direct call, and the grouped binding is never reached. Rows
    split by the default schedule are combined with atomics in either
    call, so those are compared within the bound's reach only by the
    sweep; here the schedule has no split row (seg above every degree)."""
    from bnsgcn_amd.ops.csr_torch import build_worklist
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    ip, ix = (t.clone() for t in device_csr("fixture", None, None))
    ip._bns_worklist = build_worklist(ip, seg=1 << 20)
    for F in (132, 256):
        x, ss, ds = _routing_inputs(F)
        with count_grouped() as calls:
            got = spmm_sum_raw(ip, ix, x, ss, ds)
        assert calls[0] == 0
        assert torch.equal(got, _per_row_direct(ip, ix, x, ss, ds))


def check_routing_narrow_widths(R):
    """F = 64 (narrow kernel) and F = 128 (half-wave kernel) with the
    attribute present: per-row path, bitwise equal to the CSR without it."""
    from bnsgcn_amd.ops.csr_torch import build_worklist
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    ip, ix = (t.clone() for t in device_csr("fixture", None, None))
    ip._bns_worklist = build_worklist(ip, seg=1 << 20)
    ipg = ip.clone()
    ipg._bns_worklist = ip._bns_worklist
    ipg._bns_rowgroups = device_csr("fixture", R, None)[0]._bns_rowgroups
    for F in (64, 128):
        x, ss, ds = _routing_inputs(F)
        with count_grouped() as calls:
            got = spmm_sum_raw(ipg, ix, x, ss, ds)
        assert calls[0] == 0, f"F={F} took the grouped path"
        assert torch.equal(got, spmm_sum_raw(ip, ix, x, ss, ds))


def _case_group_off():
    """BNSGCN_SPMM_GROUP=0: the attribute is ignored and attach_rowgroups
    builds nothing."""
    assert os.environ.get("BNSGCN_SPMM_GROUP") == "0"
    from bnsgcn_amd.ops import functional as BF
    from bnsgcn_amd.ops.csr_torch import build_worklist
    ip, ix = (t.clone() for t in device_csr("fixture", 8, None))
    ip._bns_rowgroups = device_csr("fixture", 8, None)[0]._bns_rowgroups
    ip._bns_worklist = build_worklist(ip, seg=1 << 20)
    for F in (132, 256):
        x, ss, ds = _routing_inputs(F)
        with count_grouped() as calls:
            got = BF.spmm_sum_raw(ip, ix, x, ss, ds)
        assert calls[0] == 0
        assert torch.equal(got, _per_row_direct(ip, ix, x, ss, ds))
    ip2 = ip.clone()
    assert BF.attach_rowgroups(ip2, ix, graph("fixture")[2]) is None
    assert not hasattr(ip2, "_bns_rowgroups")


# ----------------------------------------------------------- end to end

def check_end_to_end(mode, monkeypatch):
    """GraphContext.aggregate on the `tiny` dataset at F = 132 with the
    format kept on both CSRs (keep rule lifted): forward, and backward
    through the transposed CSR with the scales swapped, against the CPU
    reference path in float64."""
    from bnsgcn_amd.graph import load_data
    from bnsgcn_amd.models.context import GraphContext
    from bnsgcn_amd.ops import functional as BF
    monkeypatch.setattr(BF, "GROUP_TAU", 1.0)
    g = load_data("tiny", seed=0)
    args = (torch.from_numpy(g.adj_in.indptr),
            torch.from_numpy(g.adj_in.indices),
            torch.from_numpy(g.in_deg), torch.from_numpy(g.out_deg))
    # default: the transposed CSR alone carries the format
    ctx = GraphContext.for_full_graph(*args, DEV)
    assert not hasattr(ctx.indptr, "_bns_rowgroups")
    assert hasattr(ctx.t_indptr, "_bns_rowgroups")
    assert ctx.rowgroup_ratio[0] is None and 0 < ctx.rowgroup_ratio[1] <= 1
    monkeypatch.setattr(BF, "GROUP_FWD", True)
    ctx = GraphContext.for_full_graph(*args, DEV)
    cpu = GraphContext.for_full_graph(*args, "cpu")
    assert hasattr(ctx.indptr, "_bns_rowgroups")
    assert hasattr(ctx.t_indptr, "_bns_rowgroups")
    assert all(0 < r <= 1 for r in ctx.rowgroup_ratio)
    for name in ("in_norm_inv", "out_norm_inv", "in_deg_inv"):
        setattr(cpu, name, getattr(cpu, name).double())
    n = ctx.n_rows
    gq = gen(2700)
    x = torch.randn(n, 132, generator=gq)
    gy = torch.randn(n, 132, generator=gq)

    def run(c, x_, gy_):
        x_ = x_.clone().requires_grad_(True)
        y = c.aggregate(x_, mode)
        y.backward(gy_)
        return y.detach(), x_.grad

    with count_grouped() as calls:
        y, gx = run(ctx, cu(x), cu(gy))
    assert calls[0] == 2, "forward and backward must both be grouped"
    want_y, want_gx = run(cpu, dbl(x), dbl(gy))
    abs_y, abs_gx = run(cpu, dbl(x).abs(), dbl(gy).abs())
    assert_sum_bound(y, want_y, abs_y, degrees(cpu.indptr)[:, None],
                     f"aggregate {mode} forward")
    assert_sum_bound(gx, want_gx, abs_gx, degrees(cpu.t_indptr)[:, None],
                     f"aggregate {mode} backward")


# ---------------------------------------------------------- script mode

CASES = {"group_off": ({"BNSGCN_SPMM_GROUP": "0"}, _case_group_off)}


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
