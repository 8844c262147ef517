"""Graph family, schedule contract and check functions for
tests/test_worklist_cpu.py and tests/test_gpu_sparse_sweep.py.

The work-list kernels (spmm_sum, spmm_edge, sddmm_dot, sddmm_add,
segment_sum_edges) read a schedule built by ops/csr_torch.build_worklist.
The sweep runs them over a family of graph shapes and over schedules other
than the default one. A schedule is selected without a child process by
storing `build_worklist(indptr, seg=..., max_waves=...)` in the
`_bns_worklist` attribute of the device `indptr` — the cache that
ops.functional._worklist_of reads, zero_rows included.

Oracle and tolerances are those of tests/kernel_path_checks.py: float64
ops/reference.py (or the same sums written with index_add) on the same
fp32 inputs, never another GPU kernel; (n_terms + 8) * 2^-23 * ref_abs for
everything that is a sum. References do not depend on the schedule and are
computed once per shape.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import kernel_path_checks as K  # noqa: E402
from kernel_path_checks import (DEV, assert_sum_bound, cu, dbl,  # noqa: E402
                                degrees, gen)
from bnsgcn_amd.ops import reference as ref  # noqa: E402

SEGS = (1, 3, 64, 65, 512)
MAX_WAVES = (8, 24, None)
# (seg, max_waves); None = the csr_torch default
SCHEDULES = ((1, 8), (3, 24), (64, None), (65, 8), (512, 8), (512, None))

SPMM_F = (1, 2, 4, 64, 68, 132, 257, 514, 516)
EDGE_SHAPES = ((1, 4), (4, 16), (4, 100), (4, 132), (4, 41), (1, 1))
DOT_SHAPES = ((8, 8), (4, 16), (2, 32), (2, 256), (1, 512), (3, 256),
              (1, 24), (1, 4), (4, 41))
ADD_HEADS = (1, 3, 4, 8, 16)
ADD_SLOPES = (None, 0.2)        # None: no activation (kernel slope -1)

# graphs of the schedule property test / of the GPU sweep / launch-nothing
CPU_FAMILY = ("fixture", "zipf", "onerow", "lastrow", "tiny", "empty",
              "norows")
SWEEP_GRAPHS = ("fixture", "zipf", "onerow", "lastrow", "tiny", "hubcol")
DEGENERATE = ("empty", "norows")


# --------------------------------------------------------------- graphs

@functools.lru_cache(maxsize=None)
def graph(name):
    """(indptr int64, indices int32, n_cols), built once per process.

    fixture  the 96 x 80 kernel fixture (kernel_path_checks.fixture_csr)
    zipf     300 rows, Zipf(1.6) degrees clipped at 3000, 90 rows (30 %)
             empty: items of very different length share a wave
    onerow   one row of 5000 edges
    lastrow  41 rows, only the last non-empty (77 edges)
    tiny     degrees (1, 0, 2): fewer than 8 items, most waves empty
    hubcol   degrees (3, 130, 0, 5); all 130 edges of row 1 point at
             column 0
    empty    17 rows, no edge
    norows   no row
    """
    if name == "fixture":
        return K.fixture_csr() + (K.N_COLS,)
    rng = np.random.default_rng(20250)
    if name == "zipf":
        deg = np.minimum(rng.zipf(1.6, 300), 3000)
        deg[rng.permutation(300)[:90]] = 0
        assert deg.max() > 512 and int((deg == 0).sum()) == 90
        n_cols = 200
    elif name == "onerow":
        deg, n_cols = np.array([5000]), 200
    elif name == "lastrow":
        deg, n_cols = np.array([0] * 40 + [77]), 50
    elif name == "tiny":
        deg, n_cols = np.array([1, 0, 2]), 5
    elif name == "hubcol":
        deg, n_cols = np.array([3, 130, 0, 5]), 9
    elif name == "empty":
        deg, n_cols = np.zeros(17, dtype=np.int64), 7
    elif name == "norows":
        deg, n_cols = np.zeros(0, dtype=np.int64), 7
    else:
        raise KeyError(name)
    indptr, indices = K._csr_from_degrees(deg.astype(np.int64), n_cols, rng)
    if name == "hubcol":
        indices[3:133] = 0
    return indptr, indices, n_cols


def unit_degree_csr(n):
    """n rows of degree 1 into 1000 columns: n work-list items, the
    smallest graph on either side of build_worklist's million-item
    branch."""
    g = gen(31 + n % 7)
    return (torch.arange(n + 1, dtype=torch.int64),
            torch.randint(0, 1000, (n,), generator=g).to(torch.int32), 1000)


# ---------------------------------------------------- schedule contract

def expected_n_waves(total, max_waves):
    """roundup8(min(max_waves, max(8, total))); from a million items on,
    build_worklist raises max_waves to at least 262144."""
    from bnsgcn_amd.ops import csr_torch
    mw = max_waves or csr_torch.MAX_WAVES
    if total >= 1_000_000:
        mw = max(mw, 262144)
    return (min(mw, max(8, total)) + 7) // 8 * 8


def assert_worklist_contract(indptr, wl, seg, max_waves):
    """What the work-list kernels rely on (every index they form from the
    schedule stays in range exactly when this holds). `seg` / `max_waves`
    None mean the csr_torch defaults. Returns the worst balance ratio
    (edges in a wave - E / n_waves) / longest item, which must stay < 1."""
    from bnsgcn_amd.ops import csr_torch
    seg = seg or csr_torch.SEG
    indptr = indptr.cpu()
    wrow, wbeg, wend, ws, zero_rows = (t.cpu() for t in wl)
    deg = indptr[1:] - indptr[:-1]
    n = deg.numel()
    E = int(indptr[-1])
    # the dtypes the launchers check (index_fill_ needs int64 zero_rows)
    assert wrow.dtype == torch.int32 and ws.dtype == torch.int32
    assert wbeg.dtype == torch.int64 and wend.dtype == torch.int64
    assert zero_rows.dtype == torch.int64
    total = wrow.numel()
    assert wbeg.numel() == total and wend.numel() == total
    assert ws.dim() == 1 and wrow.dim() == 1

    want_zero = torch.nonzero((deg == 0) | (deg > seg))[:, 0]
    assert torch.equal(zero_rows.sort().values, want_zero), \
        "zero_rows != empty rows + split rows"

    if total == 0:
        assert E == 0
        assert ws.numel() == 1 and int(ws[0]) == 0
        return 0.0

    lens = wend - wbeg
    assert int(lens.min()) >= 1 and int(lens.max()) <= seg
    assert int(wbeg[0]) == 0 and int(wend[-1]) == E
    assert torch.equal(wbeg[1:], wend[:-1]), "items do not tile [0, E)"
    rows = torch.where(wrow < 0, ~wrow, wrow).long()
    assert int(rows.min()) >= 0 and int(rows.max()) < n
    assert (rows[1:] >= rows[:-1]).all(), "row ids decrease"
    assert (wbeg >= indptr[rows]).all() and (wend <= indptr[rows + 1]).all()
    assert torch.equal(wrow < 0, deg[rows] > seg), \
        "atomic flag != (row longer than seg)"

    n_waves = ws.numel() - 1
    assert n_waves % 8 == 0
    assert n_waves == expected_n_waves(total, max_waves), (n_waves, total)
    assert int(ws[0]) == 0 and int(ws[-1]) == total
    assert (ws[1:] >= ws[:-1]).all(), "wave_start not monotone"
    cum = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    per_wave = (cum[ws[1:].long()] - cum[ws[:-1].long()]).double()
    assert int(per_wave.sum()) == E
    ratio = float(((per_wave - E / n_waves) / float(lens.max())).max())
    assert ratio < 1.0, f"a wave holds {ratio:.3f} items over the mean"
    return ratio


# ------------------------------------------------- device CSR + schedule

_BASE = {}
_SCHED = {}
WORST = {}                      # op -> largest err/bound ratio so far


def note(op, ratio):
    WORST[op] = max(WORST.get(op, 0.0), ratio)
    return ratio


def _base_csr(name, csr=None):
    if name not in _BASE:
        from bnsgcn_amd.ops.csr_torch import transpose_csr
        indptr, indices, n_cols = csr or graph(name)
        ip, ix = cu(indptr), cu(indices)
        tip, tix, eperm = transpose_csr(ip, ix, n_cols)
        _BASE[name] = (ip, ix, tip, tix, eperm)
    return _BASE[name]


def device_csr(name, sched, csr=None):
    """(ip, ix, tip, tix, eperm) on the GPU with the schedule `sched` =
    (seg, max_waves) attached to ip and tip; sched None leaves the default
    to _worklist_of. Both schedules are checked against the contract
    before any kernel reads them. Cached per (graph, schedule)."""
    key = (name, sched)
    if key not in _SCHED:
        from bnsgcn_amd.ops.csr_torch import build_worklist
        from bnsgcn_amd.ops.functional import _worklist_of
        ip, ix, tip, tix, eperm = _base_csr(name, csr)
        ip, tip = ip.clone(), tip.clone()
        seg, mw = sched or (None, None)
        for p in (ip, tip):
            if sched is not None:
                p._bns_worklist = build_worklist(p, seg=seg, max_waves=mw)
            assert_worklist_contract(p, _worklist_of(p), seg, mw)
        _SCHED[key] = (ip, ix, tip, tix, eperm)
    return _SCHED[key]


def n_waves_of(indptr_dev):
    return indptr_dev._bns_worklist[3].numel() - 1


def _nan_junk(*shape):
    """Best-effort probe as in kernel_path_checks.check_spmm_sum: leave a
    NaN-filled block of the output's size in the caching allocator."""
    junk = torch.full(shape, float("nan"), device=DEV)
    torch.cuda.synchronize()
    del junk


# ------------------------------------------------------------- spmm_sum

ALL_VARIANTS = ((False, False), (False, True), (True, False), (True, True))


def check_spmm_sum_sweep(name, schedules=SCHEDULES, widths=SPMM_F, csr=None,
                         variants=ALL_VARIANTS):
    """spmm_sum_raw with and without the scales, with and without out=
    (`variants` = (scales, acc) pairs), at every width and schedule; for
    out=None empty rows are exactly 0."""
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    indptr, indices, n_cols = csr or graph(name)
    n_rows = indptr.numel() - 1
    deg = degrees(indptr)
    worst = 0.0
    for F in widths:
        g = gen(1300 + F)
        x = torch.randn(n_cols, F, generator=g)
        ss = torch.rand(n_cols, generator=g) + 0.5
        ds = torch.rand(n_rows, generator=g) + 0.5
        base = torch.randn(n_rows, F, generator=g)
        refs = {}
        for scales in sorted({v[0] for v in variants}):
            s_, d_ = (dbl(ss), dbl(ds)) if scales else (None, None)
            refs[scales] = (
                ref.spmm_sum(indptr, indices, dbl(x), s_, d_),
                ref.spmm_sum(indptr, indices, dbl(x).abs(), s_, d_))
        xg, ssg, dsg, bg = cu(x), cu(ss), cu(ds), cu(base)
        for sched in schedules:
            ip, ix = device_csr(name, sched, csr)[:2]
            for scales, acc in variants:
                want, want_abs = refs[scales]
                if acc:
                    want = want + dbl(base)
                    want_abs = want_abs + dbl(base).abs()
                else:
                    _nan_junk(n_rows, F)
                got = spmm_sum_raw(ip, ix, xg, ssg if scales else None,
                                   dsg if scales else None,
                                   bg.clone() if acc else None)
                what = (f"spmm_sum {name} sched={sched} F={F} "
                        f"scales={scales} acc={acc}")
                worst = max(worst, assert_sum_bound(
                    got, want, want_abs, deg[:, None], what))
                if not acc:
                    assert (got.cpu()[deg == 0] == 0).all(), \
                        f"{what}: empty rows not zero"
    print(f"sweep worst spmm_sum {name}: {note('spmm_sum', worst):.3g}")


# ------------------------------------------------------------ spmm_edge

def check_spmm_edge_sweep(name, schedules=SCHEDULES, shapes=EDGE_SHAPES):
    """spmm_edge_raw: the plain call, the out= call and the transposed
    call with wperm (as _SpMMEdge.backward issues it)."""
    from bnsgcn_amd.ops.functional import spmm_edge_raw
    indptr, indices, n_cols = graph(name)
    n_rows = indptr.numel() - 1
    E = indices.numel()
    tip_c, tix_c, ep_c = (t.cpu() for t in _base_csr(name)[2:])
    deg = degrees(indptr)[:, None, None]
    tdeg = degrees(tip_c)[:, None, None]
    worst = 0.0
    for H, D in shapes:
        g = gen(1400 + 10 * H + D)
        w = torch.randn(E, H, generator=g)
        x = torch.randn(n_cols, H, D, generator=g)
        base = torch.randn(n_rows, H, D, generator=g)
        gy = torch.randn(n_rows, H, D, generator=g)
        want = ref.spmm_edge_sum(indptr, indices, dbl(w), dbl(x))
        want_abs = ref.spmm_edge_sum(indptr, indices, dbl(w).abs(),
                                     dbl(x).abs())
        want_t = ref.spmm_edge_sum(tip_c, tix_c, dbl(w)[ep_c], dbl(gy))
        want_t_abs = ref.spmm_edge_sum(tip_c, tix_c, dbl(w)[ep_c].abs(),
                                       dbl(gy).abs())
        wg, xg, bg, gyg = cu(w), cu(x), cu(base), cu(gy)
        for sched in schedules:
            ip, ix, tip, tix, eperm = device_csr(name, sched)
            tag = f"spmm_edge {name} sched={sched} (H,D)=({H},{D})"
            _nan_junk(n_rows, H, D)
            got = spmm_edge_raw(ip, ix, wg, xg)
            r1 = assert_sum_bound(got, want, want_abs, deg, tag)
            assert (got.cpu()[degrees(indptr) == 0] == 0).all(), \
                f"{tag}: empty rows not zero"
            got = spmm_edge_raw(ip, ix, wg, xg, out=bg.clone())
            r2 = assert_sum_bound(got, want + dbl(base),
                                  want_abs + dbl(base).abs(), deg,
                                  tag + " out=")
            _nan_junk(n_cols, H, D)
            got = spmm_edge_raw(tip, tix, wg, gyg, wperm=eperm)
            r3 = assert_sum_bound(got, want_t, want_t_abs, tdeg,
                                  tag + " wperm")
            assert (got.cpu()[degrees(tip_c) == 0] == 0).all(), \
                f"{tag} wperm: empty rows not zero"
            worst = max(worst, r1, r2, r3)
    print(f"sweep worst spmm_edge {name}: {note('spmm_edge', worst):.3g}")


# ------------------------------------------------------------ sddmm_dot

def check_sddmm_dot_sweep(name, schedules=SCHEDULES, shapes=DOT_SHAPES):
    from bnsgcn_amd.ops.functional import sddmm_dot_raw
    indptr, indices, n_cols = graph(name)
    n_rows = indptr.numel() - 1
    worst = 0.0
    for H, D in shapes:
        g = gen(1500 + 10 * H + D)
        a = torch.randn(n_rows, H, D, generator=g)
        b = torch.randn(n_cols, H, D, generator=g)
        want = ref.sddmm_dot(indptr, indices, dbl(a), dbl(b))
        want_abs = ref.sddmm_dot(indptr, indices, dbl(a).abs(), dbl(b).abs())
        ag, bg = cu(a), cu(b)
        for sched in schedules:
            ip, ix = device_csr(name, sched)[:2]
            _nan_junk(indices.numel(), H)
            got = sddmm_dot_raw(ip, ix, ag, bg)
            worst = max(worst, assert_sum_bound(
                got, want, want_abs, float(D),
                f"sddmm_dot {name} sched={sched} (H,D)=({H},{D})"))
    print(f"sweep worst sddmm_dot {name}: {note('sddmm_dot', worst):.3g}")


# ------------------------------------- sddmm_add + segment_sum_edges

def check_sddmm_add_autograd(name, schedules=SCHEDULES, heads=ADD_HEADS,
                             csr=None):
    """ops.functional.sddmm_add forward and backward: the output, d el
    (segment_sum_edges over the transposed CSR with eperm) and d er
    (segment_sum_edges over the forward CSR); H = 4 is the float4 form,
    H = 16 the index_add_ route on device tensors.

    The output is one addition (n_terms = 1, ref_abs = |el| + |er|). The
    LeakyReLU mask is the sign of el + er, which fp32 rounding cannot
    change, so the float64 reference applies the same mask."""
    from bnsgcn_amd.ops import functional as BF
    indptr, indices, n_cols = csr or graph(name)
    n_rows = indptr.numel() - 1
    E = indices.numel()
    row = torch.repeat_interleave(torch.arange(n_rows),
                                  indptr[1:] - indptr[:-1])
    col = indices.long()
    deg = degrees(indptr)[:, None]
    tdeg = torch.bincount(col, minlength=n_cols).double()[:, None]
    worst_out = worst_seg = 0.0
    for H in heads:
        g = gen(1600 + H)
        el = torch.randn(n_cols, H, generator=g)
        er = torch.randn(n_rows, H, generator=g)
        gout = torch.randn(E, H, generator=g)
        pre = ref.sddmm_add(indptr, indices, dbl(el), dbl(er))
        pre_abs = ref.sddmm_add(indptr, indices, dbl(el).abs(),
                                dbl(er).abs())
        for slope in ADD_SLOPES:
            if slope is None:
                want, geff = pre, dbl(gout)
            else:
                want = torch.nn.functional.leaky_relu(pre, slope)
                geff = torch.where(pre > 0, dbl(gout), dbl(gout) * slope)
            z_el = torch.zeros(n_cols, H, dtype=torch.float64)
            z_er = torch.zeros(n_rows, H, dtype=torch.float64)
            want_del = z_el.index_add(0, col, geff)
            abs_del = z_el.index_add(0, col, geff.abs())
            want_der = z_er.index_add(0, row, geff)
            abs_der = z_er.index_add(0, row, geff.abs())
            for sched in schedules:
                csr5 = device_csr(name, sched, csr)
                elg = cu(el).requires_grad_(True)
                erg = cu(er).requires_grad_(True)
                out = BF.sddmm_add(elg, erg, *csr5, slope=slope)
                (out * cu(gout)).sum().backward()
                tag = f"sddmm_add {name} sched={sched} H={H} slope={slope}"
                worst_out = max(worst_out, assert_sum_bound(
                    out, want, pre_abs, 1.0, tag))
                worst_seg = max(
                    worst_seg,
                    assert_sum_bound(elg.grad, want_del, abs_del, tdeg,
                                     tag + " d el"),
                    assert_sum_bound(erg.grad, want_der, abs_der, deg,
                                     tag + " d er"))
    print(f"sweep worst sddmm_add {name}: {note('sddmm_add', worst_out):.3g}")
    print(f"sweep worst segment_sum_edges {name}: "
          f"{note('segment_sum_edges', worst_seg):.3g}")


# ---------------------------------------------------- degenerate graphs

def check_degenerate(op, name):
    """All rows empty / no row at all: zeros or empty outputs, out= left
    unchanged, and no launch error pending afterwards."""
    from bnsgcn_amd.ops import functional as BF
    indptr, indices, n_cols = graph(name)
    n_rows = indptr.numel() - 1
    assert indices.numel() == 0
    g = gen(1700)
    for sched in (None, (1, 8)):
        ip, ix, tip, tix, eperm = device_csr(name, sched)
        if op == "spmm_sum":
            for F in (4, 68, 257, 514):
                x = torch.randn(n_cols, F, generator=g)
                base = torch.randn(n_rows, F, generator=g)
                _nan_junk(max(n_rows, 1), F)
                got = BF.spmm_sum_raw(ip, ix, cu(x))
                assert torch.equal(got.cpu(), torch.zeros(n_rows, F))
                got = BF.spmm_sum_raw(ip, ix, cu(x), out=cu(base).clone())
                assert torch.equal(got.cpu(), base)
        elif op == "spmm_edge":
            for H, D in ((4, 16), (4, 41)):
                w = torch.zeros(0, H)
                x = torch.randn(n_cols, H, D, generator=g)
                gy = torch.randn(n_rows, H, D, generator=g)
                base = torch.randn(n_rows, H, D, generator=g)
                _nan_junk(max(n_rows, 1), H, D)
                got = BF.spmm_edge_raw(ip, ix, cu(w), cu(x))
                assert torch.equal(got.cpu(), torch.zeros(n_rows, H, D))
                got = BF.spmm_edge_raw(ip, ix, cu(w), cu(x),
                                       out=cu(base).clone())
                assert torch.equal(got.cpu(), base)
                got = BF.spmm_edge_raw(tip, tix, cu(w), cu(gy), wperm=eperm)
                assert torch.equal(got.cpu(), torch.zeros(n_cols, H, D))
        elif op == "sddmm_dot":
            for H, D in ((4, 16), (3, 256), (4, 41)):
                a = torch.randn(n_rows, H, D, generator=g)
                b = torch.randn(n_cols, H, D, generator=g)
                assert BF.sddmm_dot_raw(ip, ix, cu(a), cu(b)).shape == (0, H)
        elif op == "sddmm_add":
            for H in (3, 4, 16):
                for slope in ADD_SLOPES:
                    elg = cu(torch.randn(n_cols, H, generator=g))
                    erg = cu(torch.randn(n_rows, H, generator=g))
                    elg.requires_grad_(True)
                    erg.requires_grad_(True)
                    out = BF.sddmm_add(elg, erg, ip, ix, tip, tix, eperm,
                                       slope=slope)
                    assert out.shape == (0, H)
                    out.sum().backward()
                    assert torch.equal(elg.grad.cpu(), torch.zeros(n_cols, H))
                    assert torch.equal(erg.grad.cpu(), torch.zeros(n_rows, H))
        else:
            raise KeyError(op)
    torch.cuda.synchronize()
    assert float((torch.ones(8, device=DEV) * 2).sum()) == 16.0


# ------------------------------------------------- million-item branch

def check_unit_degree(op, n, n_waves):
    """`n` rows of degree 1 under the default schedule, which must have
    `n_waves` waves (262144, a 65,536-block grid, from a million items
    on)."""
    csr = unit_degree_csr(n)
    name = f"unit{n}"
    ip, _, tip = device_csr(name, None, csr)[:3]
    assert n_waves_of(ip) == n_waves, n_waves_of(ip)
    assert degrees(tip.cpu()).max() > 512         # transposed: split rows
    if op == "spmm_sum_4":
        check_spmm_sum_sweep(name, (None,), (4,), csr)
    elif op == "spmm_sum_64":
        # 64M outputs: one variant; F = 4 runs all four
        check_spmm_sum_sweep(name, (None,), (64,), csr,
                             variants=((True, False),))
    elif op == "sddmm_add_4":
        check_sddmm_add_autograd(name, (None,), (4,), csr)
    else:
        raise KeyError(op)
