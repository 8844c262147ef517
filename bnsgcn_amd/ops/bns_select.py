"""Boundary-node selection on the device: the s smallest of n keys per
segment, positions ascending, without a sort and without a read-back —
bit-identical to `sort(argsort(keys, stable=True)[:s])`.

Two forms share a call and write disjoint ranges of the same outputs:

* segments of up to SLICED_MIN_ROWS rows: ONE launch, one workgroup per
  segment (ops/hip/bns_select.hip);
* larger segments: cut into slices of SLICE_ROWS positions, one workgroup
  per (segment, slice), a fixed sequence of launches
  (ops/hip/bns_select_sliced.hip).

Two key sources share the kernel bodies:

* `PlanSelect` — the production form. Keys are the shared Philox keys of
  ops/philox.py, recomputed on the fly from (seed, epoch, src, dst, i); one
  call per epoch yields `pack_idx`, `hsel` and the two per-row floats of a
  HaloPlan (parallel/plan.py). The tables are built once per job.
* `select_smallest` — caller-supplied int64 keys, a public utility.

SAMPLE_HIP is the switch for the plan: on when the extension is loaded,
BNSGCN_SAMPLE_TORCH=1 turns it off, and with it off (or on the CPU) the
plan samples with philox_keys + argsort + sort as before. It is a module
attribute read at call time, like csr_torch.PLAN_HIP. BNSGCN_SELECT_SLICED=0
(SELECT_SLICED) takes the sliced form away from the plan: a plan with a
segment above MAX_SEG_ROWS then samples with the sorts, for A/B.

Everything the kernels trust is checked HERE, on the host values the tables
are built from: sizes below 2^31, key and gather ranges inside their
tensors, the slice size. Sizes, offsets and the (segment, slice) work list
are host integers throughout, so nothing is read back from the device.
"""
from __future__ import annotations

import os
from typing import Sequence

import torch

from ._ext import has_ext, require_ext

SAMPLE_HIP = has_ext() and os.environ.get("BNSGCN_SAMPLE_TORCH") != "1"
SELECT_SLICED = os.environ.get("BNSGCN_SELECT_SLICED") != "0"

KIND_PACK, KIND_HALO = 0, 1     # SEG_KIND of the table (bns_select_dev.h)
# Rows above which a segment takes the sliced form, and the rows of a slice.
# Measured on one segment alone (tools/select_micro.py,
# profiles/BENCH_SUMMARY_bnsselect_sliced.md): slices of 4096 rows are the
# fastest at 2M rows (0.197 ms against 0.203 at 2048 and 0.200 at 8192), and
# with them the sliced form (0.039 ms from 8k to 20k rows: 11 launches) meets
# the one-workgroup kernel (1.85 us per 1000 rows) between 16k and 20k rows.
SLICED_MIN_ROWS = 1 << 14
SLICE_ROWS = 4096
# Largest segment the one-workgroup kernel takes from a plan when the sliced
# form is switched off (BNSGCN_SELECT_SLICED=0). One workgroup walks a
# segment three times, 1.85 us per 1000 rows, against 0.084 ms per segment at
# 20k rows and 0.135 ms at 200k for the sort path; 100k rows = 0.19 ms is
# what the two sorted segments of the smallest job (2 partitions) cost. With
# the sliced form on, no segment size sends a plan to the sort path.
MAX_SEG_ROWS = 100_000


def sample_hip(device, seg_rows: Sequence[int] = ()) -> bool:
    """True where a plan on `device` whose segments hold `seg_rows` rows
    samples with the HIP kernels."""
    return (bool(SAMPLE_HIP) and torch.device(device).type == "cuda"
            and (bool(SELECT_SLICED)
                 or max(seg_rows, default=0) <= MAX_SEG_ROWS))


class _Tables:
    """The static device tables of a job and what the bindings take with
    them: `segs` [n, 6] int64 rows of (n, s, out_off, key word, kind, base)
    for the one-launch kernel; `ssegs` [m, 7], the same columns and the
    segment's first work item, for the sliced launches; `items` [k, 2] int32
    of (sliced segment, slice). Blocking copies — construction only."""

    def __init__(self, rows: list, device, cap, slice_rows, sliced_min_rows):
        ext = require_ext()
        self.cap = ext.BNS_SELECT_CAP if cap is None else int(cap)
        self.slice_rows = int(SLICE_ROWS if slice_rows is None
                              else slice_rows)
        lim = int(SLICED_MIN_ROWS if sliced_min_rows is None
                  else sliced_min_rows)
        assert self.slice_rows > 0 and self.slice_rows <= 2 ** 30 \
            and self.slice_rows % ext.BNS_SELECT_SLICE_MIN == 0, slice_rows
        one, sliced, items = [], [], []
        for row in rows:
            n, s, off, _, _, base = row
            assert 0 < n < 2 ** 31 and s > 0 and off >= 0 and base >= 0, rows
            if n <= lim:
                one.append(row)
                continue
            n_slice = -(-n // self.slice_rows)
            sliced.append((*row, len(items)))
            items += [(len(sliced) - 1, j) for j in range(n_slice)]
        assert len(items) < 2 ** 31
        self.segs = torch.tensor(one, dtype=torch.int64
                                 ).reshape(-1, 6).to(device)
        self.ssegs = torch.tensor(sliced, dtype=torch.int64
                                  ).reshape(-1, 7).to(device)
        self.items = torch.tensor(items, dtype=torch.int32
                                  ).reshape(-1, 2).to(device)

    def args(self) -> tuple:
        return self.segs, self.ssegs, self.items, self.slice_rows


def select_smallest(keys: torch.Tensor, seg_ptr: Sequence[int],
                    seg_s: Sequence[int], cap: int | None = None,
                    slice_rows: int | None = None,
                    sliced_min_rows: int | None = None
                    ) -> tuple[torch.Tensor, list]:
    """Segment k holds keys[seg_ptr[k]:seg_ptr[k+1]] (int64 in [0, 2^63),
    on the GPU). Returns (out, out_ptr): out[out_ptr[k]:out_ptr[k+1]] are
    the positions within segment k of its min(seg_s[k], n_k) smallest keys,
    ascending; equal keys rank by position. seg_ptr / seg_s are host
    integers. Segments of more than `sliced_min_rows` rows are cut into
    slices of `slice_rows` (a multiple of _C.BNS_SELECT_SLICE_MIN) over
    several launches; None takes SLICED_MIN_ROWS / SLICE_ROWS. `cap`
    (candidates kept for the threshold; the binding's default if None)
    changes how deep the radix descent goes. None of the three changes the
    result."""
    seg_ptr, seg_s = [int(v) for v in seg_ptr], [int(v) for v in seg_s]
    assert len(seg_ptr) == len(seg_s) + 1 and seg_ptr[0] >= 0
    assert seg_ptr[-1] <= keys.numel()
    rows, out_ptr = [], [0]
    for k, s in enumerate(seg_s):
        n = seg_ptr[k + 1] - seg_ptr[k]
        assert n >= 0, "seg_ptr must not decrease"
        if min(s, n) > 0:
            rows.append((n, s, out_ptr[-1], seg_ptr[k], KIND_HALO, 0))
        out_ptr.append(out_ptr[-1] + max(min(s, n), 0))
    tb = _Tables(rows, keys.device, cap, slice_rows, sliced_min_rows)
    out = require_ext().bns_select_raw(keys, *tb.args(), out_ptr[-1], tb.cap)
    return out, out_ptr


class PlanSelect:
    """Static selection job: `segments` are (n, s, src_rank, dst_rank, kind,
    base) in output order. A KIND_PACK segment emits boundary_cat[base + i]
    into `pack_idx`, a KIND_HALO segment base + i into `hsel` together with
    norm_full / deg_full at that row (when given). `self(epoch)` returns
    (pack_idx, hsel, norm_full[hsel], deg_full[hsel]) for that epoch.
    `cap`, `slice_rows`, `sliced_min_rows`: as for select_smallest."""

    def __init__(self, segments: list, seed: int, device,
                 boundary_cat: torch.Tensor | None = None,
                 norm_full: torch.Tensor | None = None,
                 deg_full: torch.Tensor | None = None,
                 cap: int | None = None, slice_rows: int | None = None,
                 sliced_min_rows: int | None = None):
        self.seed = int(seed)
        self.aux = (boundary_cat, norm_full, deg_full)
        lim = (None if boundary_cat is None else boundary_cat.numel(),
               None if norm_full is None else min(norm_full.numel(),
                                                  deg_full.numel()))
        rows, size = [], [0, 0]
        for n, s, src, dst, kind, base in segments:
            if min(s, n) <= 0:
                continue
            assert kind in (KIND_PACK, KIND_HALO)
            assert lim[kind] is None or base + n <= lim[kind], (base, n, lim)
            rows.append((n, s, size[kind],
                         ((src & 0xFFFF) << 16) | (dst & 0xFFFF), kind, base))
            size[kind] += min(s, n)
        self.n_pack, self.n_hsel = size
        self.tables = _Tables(rows, device, cap, slice_rows, sliced_min_rows)
        self.cap = self.tables.cap

    def __call__(self, epoch: int):
        return require_ext().bns_select_philox(
            *self.tables.args(), self.n_pack, self.n_hsel, *self.aux,
            self.seed, int(epoch) & 0xFFFFFFFF, self.cap)
