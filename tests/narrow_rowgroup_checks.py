"""Check functions for tests/test_gpu_narrow_rowgroup.py and
tests/test_narrow_rowgroup_cpu.py: spmm_sum_grouped_narrow_kernel, the
row-group form of the narrow SpMM (F % 4 == 0, F / 4 <= 16, fp32 source),
behind ops.functional.spmm_sum_raw.

Graphs, the format contract, the oracle (float64 ops/reference.py on the
same fp32 inputs, never another GPU kernel) and the tolerance
(assert_sum_bound, n_terms = the row's edge count) are those of
tests/rowgroup_checks.py. A format is forced on a CSR as there: stored in
the `_bns_rowgroups` attribute of a private copy of the device indptr, here
with the `narrow` flag set, which build_rowgroups leaves off.

Run as a script (`python tests/narrow_rowgroup_checks.py group_off FILE`)
it executes the BNSGCN_SPMM_GROUP=0 case in a fresh process (the switch is
read once, at import) against the tensors the parent test saved in FILE.
"""
from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rowgroup_checks as G  # noqa: E402
import sparse_sweep_checks as S  # noqa: E402
from kernel_path_checks import (assert_sum_bound, cu, dbl,  # noqa: E402
                                degrees, gen)
from bnsgcn_amd.ops import reference as ref  # noqa: E402

RS = (4, 8)                             # every instantiated R
# f4 = 1 (one live lane per 16-lane group), 11 (the headline's 44), 15, 16
WIDTHS = (4, 44, 60, 64)
# 1: every group split, all atomic; 3, 4, 5: around the 4 entries of a
# step; 64, 65: the chunk boundary; None: the csr_torch default
GSEGS = (1, 3, 4, 5, 64, 65, None)
LANE_GROUPS = 4                         # 64 / G entries per step

_DEV = {}


def narrow_csr(name, R, gseg, wide=True):
    """(ip, ix) on the GPU; ip is a private copy that carries the format
    (R, gseg) of rowgroup_checks.device_csr (contract asserted there) with
    narrow calls allowed."""
    key = (name, R, gseg, wide)
    if key not in _DEV:
        ip0, ix = G.device_csr(name, R, gseg)
        ip = ip0.clone()
        ip._bns_rowgroups = ip0._bns_rowgroups._replace(wide=wide,
                                                        narrow=True)
        _DEV[key] = (ip, ix)
    return _DEV[key]


def _inputs(n_cols, n_rows, F, seed):
    g = gen(seed)
    return (torch.randn(n_cols, F, generator=g),
            torch.rand(n_cols, generator=g) + 0.5,
            torch.rand(n_rows, generator=g) + 0.5,
            torch.randn(n_rows, F, generator=g))


# ---------------------------------------------------------------- sweep

def check_narrow_sweep(name, R, gsegs=GSEGS, widths=WIDTHS):
    """spmm_sum_raw on a CSR whose format allows narrow calls: every
    width, with and without both scales, overwrite (from a NaN-prefilled
    allocation) and out= accumulate, every gseg; each call must reach the
    grouped binding. Empty rows of an overwrite come out exactly 0. Some
    item's entry count is no multiple of the 4 entries of a step, so a
    last step with idle lane groups occurs."""
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    indptr, indices, n_cols = G.graph(name)
    n_rows = indptr.numel() - 1
    deg = degrees(indptr)
    ragged = False
    for gseg in gsegs:
        sched = narrow_csr(name, R, gseg)[0]._bns_rowgroups.sched
        ragged |= bool(((sched[2] - sched[1]) % LANE_GROUPS != 0).any())
    assert ragged, f"{name} R={R}: no item with a ragged last step"
    worst = 0.0
    for F in widths:
        x, ss, ds, base = _inputs(n_cols, n_rows, F, 3300 + F)
        refs = {}
        for scales in (False, True):
            s_, d_ = (dbl(ss), dbl(ds)) if scales else (None, None)
            refs[scales] = (
                ref.spmm_sum(indptr, indices, dbl(x), s_, d_),
                ref.spmm_sum(indptr, indices, dbl(x).abs(), s_, d_))
        xg, ssg, dsg, bg = cu(x), cu(ss), cu(ds), cu(base)
        for gseg in gsegs:
            ip, ix = narrow_csr(name, R, gseg)
            for scales, acc in S.ALL_VARIANTS:
                want, want_abs = refs[scales]
                if acc:
                    want = want + dbl(base)
                    want_abs = want_abs + dbl(base).abs()
                else:
                    G._nan_junk(n_rows, F)
                with G.count_grouped() as calls:
                    got = spmm_sum_raw(ip, ix, xg, ssg if scales else None,
                                       dsg if scales else None,
                                       bg.clone() if acc else None)
                what = (f"narrow grouped {name} R={R} gseg={gseg} F={F} "
                        f"scales={scales} acc={acc}")
                assert calls[0] == 1, f"{what}: not routed to the grouped path"
                worst = max(worst, assert_sum_bound(
                    got, want, want_abs, deg[:, None], what))
                if not acc:
                    assert (got.cpu()[deg == 0] == 0).all(), \
                        f"{what}: empty rows not zero"
    print(f"narrow grouped worst {name} R={R}: {worst:.3g}")
    return worst


# ------------------------------------------------------------ isolation

def check_isolation(R):
    """rowgroup_checks' `isolate` graph: column 33 is a neighbour of row 5
    only. With x[33] = inf, then NaN, every other row stays finite and
    within the bound."""
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    indptr, indices, n_cols = G.graph("isolate")
    n_rows = indptr.numel() - 1
    others = torch.arange(n_rows) != 5
    deg = degrees(indptr)[others, None]
    for F in (4, 44, 64):
        x, ss, ds, _ = _inputs(n_cols, n_rows, F, 3400 + F)
        want = ref.spmm_sum(indptr, indices, dbl(x), dbl(ss), dbl(ds))[others]
        want_abs = ref.spmm_sum(indptr, indices, dbl(x).abs(), dbl(ss),
                                dbl(ds))[others]
        for bad in (float("inf"), float("nan")):
            xb = x.clone()
            xb[33] = bad
            for gseg in (1, None):
                ip, ix = narrow_csr("isolate", R, gseg)
                with G.count_grouped() as calls:
                    got = spmm_sum_raw(ip, ix, cu(xb), cu(ss), cu(ds))
                assert calls[0] == 1
                assert not torch.isfinite(got[5]).any()
                assert_sum_bound(got[others], want, want_abs, deg,
                                 f"narrow isolation R={R} F={F} x[33]={bad} "
                                 f"gseg={gseg}")


# ------------------------------------------------------ reproducibility

def check_reproducible(R):
    """No split group: single-writer rows and a fixed summation order, so
    two calls agree bitwise."""
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    for name in ("fixture", "zipf"):
        indptr, indices, n_cols = G.graph(name)
        ip, ix = narrow_csr(name, R, 1 << 20)
        assert int((ip._bns_rowgroups.sched[0] < 0).sum()) == 0
        x, ss, ds, _ = _inputs(n_cols, indptr.numel() - 1, 44, 3500)
        x, ss, ds = cu(x), cu(ss), cu(ds)
        with G.count_grouped() as calls:
            a = spmm_sum_raw(ip, ix, x, ss, ds)
            b = spmm_sum_raw(ip, ix, x, ss, ds)
        assert calls[0] == 2
        assert torch.equal(a, b), f"{name} R={R}: two calls differ"
        assert a.abs().sum() > 0


# -------------------------------------------------------------- routing

def _unsplit_pair(R, **flags):
    """The fixture CSR twice over one per-row schedule without a split row
    (bitwise comparable): without the format, and with it."""
    from bnsgcn_amd.ops.csr_torch import build_worklist
    ip = G.device_csr("fixture", None, None)[0].clone()
    ix = G.device_csr("fixture", None, None)[1]
    ip._bns_worklist = build_worklist(ip, seg=1 << 20)
    ipg = ip.clone()
    ipg._bns_worklist = ip._bns_worklist
    ipg._bns_rowgroups = G.device_csr(
        "fixture", R, None)[0]._bns_rowgroups._replace(**flags)
    return ip, ipg, ix


def check_routing_narrow_only_keeps_wide_forward(R):
    """A forward CSR's format is narrow-only: at F = 256 it still runs the
    per-row kernel, bitwise the result of the CSR without the format,
    while F = 44 on it is grouped."""
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    ip, ipg, ix = _unsplit_pair(R, wide=False, narrow=True)
    x, ss, ds = G._routing_inputs(256)
    with G.count_grouped() as calls:
        got = spmm_sum_raw(ipg, ix, x, ss, ds)
    assert calls[0] == 0, "F=256 took the grouped path on a narrow-only format"
    assert torch.equal(got, spmm_sum_raw(ip, ix, x, ss, ds))
    x, ss, ds = G._routing_inputs(44)
    with G.count_grouped() as calls:
        spmm_sum_raw(ipg, ix, x, ss, ds)
    assert calls[0] == 1


def check_routing_bf16_source_stays_per_row(R):
    """A bf16 source at F = 44 stays on the per-row narrow kernel."""
    from bnsgcn_amd.ops.functional import round_bf16_raw, spmm_sum_raw
    ip, ipg, ix = _unsplit_pair(R, narrow=True)
    x, ss, ds = G._routing_inputs(44)
    xb = round_bf16_raw(x)
    with G.count_grouped() as calls:
        got = spmm_sum_raw(ipg, ix, xb, ss, ds)
    assert calls[0] == 0
    assert torch.equal(got, spmm_sum_raw(ip, ix, xb, ss, ds))


def routing_f68(R):
    """F = 68 (f4 = 17, no grouped kernel) on the CSR that carries the
    format for wide and narrow calls; the child process compares its
    BNSGCN_SPMM_GROUP=0 result with this one bit for bit."""
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    _, ipg, ix = _unsplit_pair(R, narrow=True)
    x, ss, ds = G._routing_inputs(68)
    with G.count_grouped() as calls:
        got = spmm_sum_raw(ipg, ix, x, ss, ds)
    assert calls[0] == 0, "F=68 took the grouped path"
    return got.cpu()


def _case_group_off(path):
    """BNSGCN_SPMM_GROUP=0: the format is ignored at every width. F = 68
    reproduces the parent process's result, F = 44 and 64 the per-row
    kernel called directly."""
    assert os.environ.get("BNSGCN_SPMM_GROUP") == "0"
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    saved = torch.load(path)
    for R in RS:
        _, ipg, ix = _unsplit_pair(R, narrow=True)
        for F in (44, 64, 68):
            x, ss, ds = G._routing_inputs(F)
            with G.count_grouped() as calls:
                got = spmm_sum_raw(ipg, ix, x, ss, ds)
            assert calls[0] == 0
            assert torch.equal(got, G._per_row_direct(ipg, ix, x, ss, ds))
            if F == 68:
                assert torch.equal(got.cpu(), saved[R]), \
                    f"R={R}: F=68 differs from the default process"


# ---------------------------------------------------------- model level

def fixture_context(rank, device):
    """(ctx, rows, part) of one rank of the 3-partition fixture with its
    train rows as loss rows."""
    import numpy as np
    import partition_path_checks as P
    from bnsgcn_amd.models.context import GraphContext
    _, parts = P.fixture_parts(3)
    part = parts[rank]
    plan = P.make_plan(part, 0.4, device)
    plan.set_epoch(3)
    ctx = GraphContext.for_partition(part, plan, device, need_eperm=False)
    rows = torch.from_numpy(np.flatnonzero(part.train_mask)).to(device)
    return ctx, rows, part


def check_gathered_contract(rank, device):
    """The gathered CSRs of the fixture: on the GPU (keep rule lifted by
    the caller) both carry a format that meets the contract, the forward
    one narrow-only; on the CPU nothing is attached."""
    from bnsgcn_amd.ops import csr_torch
    ctx, rows, part = fixture_context(rank, device)
    ip, ix, tip, tix = ctx._rows_inner_csrs(rows)
    if torch.device(device).type != "cuda":
        assert not hasattr(ip, "_bns_rowgroups")
        assert not hasattr(tip, "_bns_rowgroups")
        return
    fwd, bwd = ip._bns_rowgroups, tip._bns_rowgroups
    assert fwd.narrow and not fwd.wide
    assert bwd.narrow and bwd.wide
    G.assert_rowgroup_contract(ip, ix, ctx.plan.n_inner, fwd, csr_torch.GROUP_R,
                               csr_torch.GSEG)
    G.assert_rowgroup_contract(tip, tix, rows.numel(), bwd, csr_torch.GROUP_R,
                               csr_torch.GSEG)


# ---------------------------------------------------------- script mode

def main(argv):
    if len(argv) != 3 or argv[1] != "group_off":
        print(f"usage: {argv[0]} group_off FILE", file=sys.stderr)
        return 2
    if not torch.cuda.is_available():
        print("no GPU", file=sys.stderr)
        return 3
    _case_group_off(argv[2])
    torch.cuda.synchronize()
    print("group_off: ok")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
