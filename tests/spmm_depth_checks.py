"""Graph and check functions for tests/test_gpu_spmm_depth.py and
tests/test_spmm_depth_cpu.py: the depth parameter U of the wide SpMM
kernels (spmm_sum_wide_kernel, spmm_sum_grouped_kernel; U source-row reads
in flight, next chunk and next item prefetched).

The claim is "same sums, same order": for U in {8, 16} against U = 4 of
the same build,
* every row with a single writer (a row that is not split; a row of a
  group that is not split) is bitwise equal — the lists come from the
  work list / row-group schedule, as in tests/rowgroup_checks.py;
* split rows combine with atomics in an order that varies between any two
  calls, so they — and every other row, at every U including 4 — are held
  to the float64 reference of ops/reference.py with assert_sum_bound of
  tests/kernel_path_checks.py (n_terms = the row's edge count).

Graph `depthgraph`: 261 rows (not a multiple of 4) x 300 columns. Degrees
cycle through 0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128,
129: every remainder of a 4-, 8- and 16-entry window and both sides of the
64-entry chunk boundary. Row 40 has 1300 edges (split by seg = 512, and its
group by gseg = 256), row 77 repeats column 2 three hundred times (a
row-group count above 255: a repeated entry), column 299 belongs to row 12
alone, and the last row has 64 edges, so the last chunk of the last item
ends exactly at the end of the column array. That case, and the waves
without a following item, are here so that the prefetch RUNS where nothing
follows; a stray read past an array would not be noticed by any assertion
(the allocator pads), only a wrong value taken from it would.

Two schedules: max_waves = 8 gives every wave a range of some thirty items
(next-item prefetch, last item of a range), the default gives one wave per
item and leaves the rest of the waves without any (nothing follows).
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rowgroup_checks as G  # noqa: E402
from kernel_path_checks import (DEV, assert_sum_bound, cu, dbl,  # noqa: E402
                                degrees, gen)
from sparse_sweep_checks import ALL_VARIANTS  # noqa: E402
from bnsgcn_amd.ops import reference as ref  # noqa: E402

DEPTHS = (4, 8, 16)
WIDTHS = (132, 256, 260, 512, 516)
DTYPES = ("fp32", "bf16")
FAMILIES = ("per_row", "grouped")
MAX_WAVES = (8, None)
DEGREES = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129)
N_ROWS, N_COLS = 261, 300
LONG_ROW, DUP_ROW, LONE_ROW, LONE_COL = 40, 77, 12, 299
SEG, GSEG = 512, 256


@functools.lru_cache(maxsize=None)
def depthgraph():
    rng = np.random.default_rng(20261)
    deg = np.array([DEGREES[i % len(DEGREES)] for i in range(N_ROWS)])
    deg[LONG_ROW], deg[DUP_ROW], deg[N_ROWS - 1] = 1300, 300, 64
    assert deg[LONE_ROW] == 64
    rows = [rng.integers(0, N_COLS - 1, d) for d in deg]
    rows[DUP_ROW][:] = 2
    rows[LONE_ROW][17] = LONE_COL
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    assert int((indices == LONE_COL).sum()) == 1
    return torch.from_numpy(indptr), torch.from_numpy(indices), N_COLS


# ------------------------------------------------------------ schedules

def schedule(family, max_waves, ip, ix):
    """Work list (per_row) or R = 4 row-group format (grouped) of the graph
    held in (ip, ix), attached to ip as spmm_sum_raw reads it. Returns the
    bool mask of the rows that have a single writer, after checking that
    the schedule has the shape this module's docstring promises."""
    from bnsgcn_amd.ops import csr_torch
    indptr, indices, n_cols = depthgraph()
    single = torch.ones(N_ROWS, dtype=torch.bool)
    if family == "per_row":
        sched = csr_torch.build_worklist(ip, seg=SEG, max_waves=max_waves)
        ip._bns_worklist = sched
        wrow = sched[0].cpu()
        single[(~wrow[wrow < 0]).long().unique()] = False
        assert (~single).nonzero()[:, 0].tolist() == [LONG_ROW]
    else:
        rg = csr_torch.build_rowgroups(ip, ix, n_cols, R=4, gseg=GSEG,
                                       max_waves=max_waves)
        G.assert_rowgroup_contract(indptr, indices, n_cols, rg, 4, GSEG)
        ip._bns_rowgroups = rg
        sched = rg.sched
        # DUP_ROW's 300-fold edge: column 2 twice in its group, 255 + 45
        ecol, ew = rg.ecol.cpu(), rg.ew.cpu()
        dup = ew[:, DUP_ROW % 4] >= 45
        assert sorted(ew[dup & (ecol == 2), DUP_ROW % 4].tolist())[-2:] \
            == [45, 255]
        wg = sched[0].cpu()
        groups = (~wg[wg < 0]).long().unique()
        assert LONG_ROW // 4 in groups.tolist()
        rows = (groups[:, None] * 4 + torch.arange(4)).flatten()
        single[rows[rows < N_ROWS]] = False
    items = (sched[3][1:] - sched[3][:-1]).cpu()
    if max_waves == 8:
        # ranges of many items: prefetch across items, last item of a range
        assert items.numel() == 8 and int(items.min()) > 1
    else:
        # waves with exactly one item, and waves with none
        assert (items == 1).any() and (items == 0).any()
    # the last item ends on a chunk boundary, at the end of the column array
    assert int(sched[2][-1]) == (ix.numel() if family == "per_row"
                                 else rg.ecol.numel())
    return single


@functools.lru_cache(maxsize=None)
def device_csr(family, max_waves):
    """(ip, ix, single) on the GPU with the schedule attached."""
    indptr, indices, _ = depthgraph()
    ip, ix = cu(indptr), cu(indices)
    return ip, ix, schedule(family, max_waves, ip, ix)


def source(x, dtype):
    """(device source operand, its values in float64)."""
    from bnsgcn_amd.ops.functional import round_bf16_raw
    if dtype == "bf16":
        xq = round_bf16_raw(cu(x))
        assert xq.dtype == torch.bfloat16
        return xq, xq.cpu().double()
    return cu(x), dbl(x)


def run(family, ip, ix, x, ss, ds, out, depth):
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    with G.count_grouped() as calls:
        got = spmm_sum_raw(ip, ix, x, ss, ds, out, depth=depth)
    assert calls[0] == (1 if family == "grouped" else 0), \
        f"{family}: wrong kernel family"
    return got


# ---------------------------------------------------------------- checks

def check_depths(family, F, dtype):
    """Every depth, schedule, scale and output mode at one width and
    source type."""
    indptr, indices, n_cols = depthgraph()
    deg = degrees(indptr)
    g = gen(2800 + F)
    x = torch.randn(n_cols, F, generator=g)
    ss = torch.rand(n_cols, generator=g) + 0.5
    ds = torch.rand(N_ROWS, generator=g) + 0.5
    base = torch.randn(N_ROWS, F, generator=g)
    xg, xq = source(x, dtype)
    ssg, dsg, bg = cu(ss), cu(ds), cu(base)
    refs = {}
    for scales in (False, True):
        s_, d_ = (dbl(ss), dbl(ds)) if scales else (None, None)
        refs[scales] = (ref.spmm_sum(indptr, indices, xq, s_, d_),
                        ref.spmm_sum(indptr, indices, xq.abs(), s_, d_))
    worst = 0.0
    for max_waves in MAX_WAVES:
        ip, ix, single = device_csr(family, max_waves)
        for scales, acc in ALL_VARIANTS:
            want, want_abs = refs[scales]
            if acc:
                want = want + dbl(base)
                want_abs = want_abs + dbl(base).abs()
            got = {}
            for depth in DEPTHS:
                what = (f"{family} F={F} {dtype} max_waves={max_waves} "
                        f"scales={scales} acc={acc} depth={depth}")
                if not acc:
                    G._nan_junk(N_ROWS, F)
                got[depth] = run(family, ip, ix, xg,
                                 ssg if scales else None,
                                 dsg if scales else None,
                                 bg.clone() if acc else None, depth).cpu()
                worst = max(worst, assert_sum_bound(
                    got[depth], want, want_abs, deg[:, None], what))
                if not acc:
                    assert (got[depth][deg == 0] == 0).all(), \
                        f"{what}: empty rows not zero"
                if depth != 4:
                    same = (got[depth][single] == got[4][single]).all(1)
                    assert same.all(), (
                        f"{what}: single-writer rows "
                        f"{single.nonzero()[:, 0][~same].tolist()} differ "
                        f"from depth 4")
    return worst


def check_isolation(depth, dtype):
    """Grouped kernel: column LONE_COL is a neighbour of LONE_ROW only.
    With x[LONE_COL] = inf, then NaN, that row alone is not finite; every
    other single-writer row is bitwise what depth 4 gives, and all of them
    stay within the bound of a reference that never sees the value."""
    indptr, indices, n_cols = depthgraph()
    others = torch.arange(N_ROWS) != LONE_ROW
    deg = degrees(indptr)[others, None]
    F = 256
    g = gen(2900)
    x = torch.randn(n_cols, F, generator=g)
    ss = torch.rand(n_cols, generator=g) + 0.5
    ds = torch.rand(N_ROWS, generator=g) + 0.5
    for bad in (float("inf"), float("nan")):
        xb = x.clone()
        xb[LONE_COL] = bad
        xg, xq = source(xb, dtype)
        xq[LONE_COL] = 0.0               # reaches no row of `others`
        want = ref.spmm_sum(indptr, indices, xq, dbl(ss), dbl(ds))[others]
        want_abs = ref.spmm_sum(indptr, indices, xq.abs(), dbl(ss),
                                dbl(ds))[others]
        for max_waves in MAX_WAVES:
            ip, ix, single = device_csr("grouped", max_waves)
            got = {d: run("grouped", ip, ix, xg, cu(ss), cu(ds), None, d).cpu()
                   for d in (4, depth)}
            what = f"isolation depth={depth} {dtype} x={bad} mw={max_waves}"
            assert not torch.isfinite(got[depth][LONE_ROW]).any(), what
            assert_sum_bound(got[depth][others], want, want_abs, deg, what)
            keep = single & others
            assert torch.equal(got[depth][keep], got[4][keep]), what
