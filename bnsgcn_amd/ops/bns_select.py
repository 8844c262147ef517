"""Boundary-node selection on the device (ops/hip/bns_select.hip): the s
smallest of n keys per segment, positions ascending, every segment of a
call in ONE launch and without a sort — bit-identical to
`sort(argsort(keys, stable=True)[:s])`.

Two key sources share the kernel body:

* `PlanSelect` — the production form. Keys are the shared Philox keys of
  ops/philox.py, recomputed on the fly from (seed, epoch, src, dst, i); one
  call per epoch yields `pack_idx`, `hsel` and the two per-row floats of a
  HaloPlan (parallel/plan.py). The segment table is built once per job.
* `select_smallest` — caller-supplied int64 keys, a public utility.

SAMPLE_HIP is the switch for the plan: on when the extension is loaded,
BNSGCN_SAMPLE_TORCH=1 turns it off, and with it off (or on the CPU) the
plan samples with philox_keys + argsort + sort as before. It is a module
attribute read at call time, like csr_torch.PLAN_HIP.

Everything the kernel trusts is checked HERE, on the host values the table
is built from: sizes below 2^31, key and gather ranges inside their
tensors. Sizes and offsets are host integers throughout, so nothing is
read back from the device.
"""
from __future__ import annotations

import os
from typing import Sequence

import torch

from ._ext import has_ext, require_ext

SAMPLE_HIP = has_ext() and os.environ.get("BNSGCN_SAMPLE_TORCH") != "1"

KIND_PACK, KIND_HALO = 0, 1     # SEG_KIND of the table (bns_select.hip)
# Largest segment a plan gives to the kernel. One workgroup walks a segment
# three times, measured 1.85 us per 1000 rows (tools/select_micro.py:
# 0.042 ms at 20k rows, 0.37 ms at 200k, 3.7 ms at 2M), while the sort path
# costs 0.084 ms per segment at 20k rows and 0.135 ms at 200k. The segments
# of a launch run side by side and the sorts one after the other, so a build
# is bounded by its largest segment: 100k rows = 0.19 ms is what the two
# sorted segments of the smallest job (2 partitions) cost. A plan with a
# larger segment keeps the sort path (docs/DESIGN.md 7d, FUTURE.md #1).
MAX_SEG_ROWS = 100_000


def sample_hip(device, seg_rows: Sequence[int] = ()) -> bool:
    """True where a plan on `device` whose segments hold `seg_rows` rows
    samples with the HIP kernel."""
    return (bool(SAMPLE_HIP) and torch.device(device).type == "cuda"
            and max(seg_rows, default=0) <= MAX_SEG_ROWS)


def _table(rows: list, device) -> torch.Tensor:
    """[n_seg, 6] int64 device table of (n, s, out_off, key word, kind,
    base) rows. Blocking copy of a few hundred bytes — construction only."""
    for n, s, off, _, _, base in rows:
        assert 0 < n < 2 ** 31 and s > 0 and off >= 0 and base >= 0, rows
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 6).to(device)


def select_smallest(keys: torch.Tensor, seg_ptr: Sequence[int],
                    seg_s: Sequence[int], cap: int | None = None
                    ) -> tuple[torch.Tensor, list]:
    """Segment k holds keys[seg_ptr[k]:seg_ptr[k+1]] (int64 in [0, 2^63),
    on the GPU). Returns (out, out_ptr): out[out_ptr[k]:out_ptr[k+1]] are
    the positions within segment k of its min(seg_s[k], n_k) smallest keys,
    ascending; equal keys rank by position. seg_ptr / seg_s are host
    integers. `cap` (candidates kept in LDS; the binding's default if None)
    changes how deep the radix descent goes, never the result."""
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
    ext = require_ext()
    out = ext.bns_select_raw(keys, _table(rows, keys.device), out_ptr[-1],
                             ext.BNS_SELECT_CAP if cap is None else cap)
    return out, out_ptr


class PlanSelect:
    """Static selection job: `segments` are (n, s, src_rank, dst_rank, kind,
    base) in output order. A KIND_PACK segment emits boundary_cat[base + i]
    into `pack_idx`, a KIND_HALO segment base + i into `hsel` together with
    norm_full / deg_full at that row (when given). `self(epoch)` returns
    (pack_idx, hsel, norm_full[hsel], deg_full[hsel]) for that epoch."""

    def __init__(self, segments: list, seed: int, device,
                 boundary_cat: torch.Tensor | None = None,
                 norm_full: torch.Tensor | None = None,
                 deg_full: torch.Tensor | None = None,
                 cap: int | None = None):
        ext = require_ext()
        self.seed = int(seed)
        self.cap = ext.BNS_SELECT_CAP if cap is None else int(cap)
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
        self.table = _table(rows, device)

    def __call__(self, epoch: int):
        return require_ext().bns_select_philox(
            self.table, self.n_pack, self.n_hsel, *self.aux, self.seed,
            int(epoch) & 0xFFFFFFFF, self.cap)
