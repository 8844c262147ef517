"""GPU (MI355X): the sliced boundary selection
(ops/hip/bns_select_sliced.hip) at the smallest slice, against a stable
argsort of the same keys on the CPU, against the numpy Philox sampler, and —
through HaloPlan._build — against the plan sampled with torch sorts. Integer
(and copied float) outputs: torch.equal, no tolerance.

  python -m pytest tests/test_gpu_bns_select_sliced.py -m gpu -x -q
"""
import numpy as np
import pytest
import torch

import partition_path_checks as P
from partition_path_checks import DEV

from bnsgcn_amd.ops import bns_select as B
from bnsgcn_amd.ops._ext import require_ext
from bnsgcn_amd.ops.philox import sample_boundary

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="no GPU")]

# smallest slice = block of the sliced kernels (new binding: fails on the
# parent commit)
S = BLOCK = require_ext().BNS_SELECT_SLICE_MIN if torch.cuda.is_available() \
    else 256
CAP = 4096
# the last size has more slices than a block has threads
SIZES = (1, S - 1, S, S + 1, 2 * S, 3 * S + 5, (BLOCK + 3) * S + 7)


def raw_keys(pattern, n):
    """int64 keys in [0, 2^63) of one segment."""
    i = torch.arange(n, dtype=torch.int64)
    if pattern == "equal":          # ties decide everything
        return torch.full((n,), 5, dtype=torch.int64)
    if pattern == "low3":           # top 60 bits shared: every level runs
        return (i * 5 + 3) % 8
    if pattern == "descending":
        return (1 << 40) + n - i
    if pattern == "top11":          # one-level exit
        return ((i * 7 + 1) % 2048) << 52
    g = torch.Generator().manual_seed(n)
    k = torch.randint(0, 2 ** 63 - 1, (n,), generator=g, dtype=torch.int64)
    if n > S:                       # duplicates across the slice boundary
        k[n - 1] = k[100]           # and at the last position
        k[S] = k[S - 1] = k[5]
    return k


@pytest.mark.parametrize("cap", [CAP, 64])
@pytest.mark.parametrize("pattern", ["equal", "low3", "descending", "top11",
                                     "random"])
def test_select_smallest_sliced(pattern, cap):
    """Every (n, s) of the grid in one call, every segment sliced."""
    segs = [(raw_keys(pattern, n), s) for n in SIZES
            for s in (0, 1, n // 2, n - 1, n, n + 3)]
    ptr = np.cumsum([0] + [k.numel() for k, _ in segs]).tolist()
    want = [torch.sort(torch.argsort(k, stable=True)[:max(s, 0)])[0]
            for k, s in segs]
    out, out_ptr = B.select_smallest(
        torch.cat([k for k, _ in segs]).to(DEV), ptr, [s for _, s in segs],
        cap=cap, slice_rows=S, sliced_min_rows=0)
    assert out.is_cuda and out.dtype == torch.int64
    assert out_ptr == np.cumsum([0] + [w.numel() for w in want]).tolist()
    assert out.shape == (out_ptr[-1],)
    out = out.cpu()
    for k, (w, (key, s)) in enumerate(zip(want, segs)):
        assert torch.equal(out[out_ptr[k]:out_ptr[k + 1]], w), (
            pattern, cap, key.numel(), s)


def test_mixed_routing():
    """Segments of at most 2S rows go to the one-launch kernel, larger ones
    to the sliced launches; both write one output."""
    sizes = (S, 5 * S + 1, 0, 2 * S, 2 * S + 1, 3 * S, 2 * S + 1)
    segs = [(raw_keys("random", n), s)
            for n, s in zip(sizes, (S // 3, 2 * S, 4, S, S + 7, 0, 2 * S + 1))]
    ptr = np.cumsum([0] + [k.numel() for k, _ in segs]).tolist()
    want = torch.cat([torch.sort(torch.argsort(k, stable=True)[:s])[0]
                      for k, s in segs])
    out, out_ptr = B.select_smallest(
        torch.cat([k for k, _ in segs]).to(DEV), ptr, [s for _, s in segs],
        slice_rows=S, sliced_min_rows=2 * S)
    assert out_ptr[-1] == want.numel()
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("seed,epoch,src,dst", [
    (7, 0, 0, 1), ((1 << 40) + 12345, 3, 5, 2)])
def test_philox_sliced_matches_sample_boundary(seed, epoch, src, dst):
    """Both kinds: pack_idx through a permuted boundary_cat, hsel with its
    two per-row floats."""
    sizes = (3 * S + 5, 200_003)
    g = torch.Generator().manual_seed(1)
    cat = torch.randperm(sum(sizes) + 11, generator=g)
    norm, deg = torch.rand(2, sum(sizes) + 7, generator=g)
    segs, base = [], 0
    for n in sizes:
        segs += [(n, int(0.1 * n), src, dst, B.KIND_PACK, base + 11),
                 (n, int(0.1 * n), dst, src, B.KIND_HALO, base + 7)]
        base += n
    sel = B.PlanSelect(segs, seed, DEV, cat.to(DEV), norm.to(DEV),
                       deg.to(DEV), slice_rows=S, sliced_min_rows=0)
    got = [t.cpu() for t in sel(epoch)]
    pos = [torch.from_numpy(sample_boundary(n, s, seed, epoch, a, b)) + base
           for n, s, a, b, _, base in segs]
    hsel = torch.cat(pos[1::2])
    for g_, w in zip(got, (cat[torch.cat(pos[0::2])], hsel, norm[hsel],
                           deg[hsel])):
        assert g_.dtype == w.dtype and torch.equal(g_, w)


@pytest.mark.parametrize("unit_ratio", [False, True])
def test_plan_same_with_every_segment_sliced(unit_ratio, monkeypatch):
    """HaloPlan._build with every segment through the sliced launches
    against the same plan sampled with torch sorts."""
    assert B.SAMPLE_HIP
    monkeypatch.setattr(B, "SLICED_MIN_ROWS", 0)
    monkeypatch.setattr(B, "SLICE_ROWS", S)
    for part in P.fixture_parts(3)[1]:
        plan = P.make_plan(part, 0.4, DEV, unit_ratio=unit_ratio)
        assert plan._select_hip()[0].tables.segs.numel() == 0
        for epoch in (0, 3):
            states = []
            for on in (True, False):
                monkeypatch.setattr(B, "SAMPLE_HIP", on)
                states.append(plan._build(epoch))
            on, off = states
            tag = (part.rank, unit_ratio, epoch)
            for f, want in vars(off).items():
                got = getattr(on, f)
                if not torch.is_tensor(want):
                    assert got == want, (tag, f)
                    continue
                wg = getattr(got, "_bns_worklist", ())
                ww = getattr(want, "_bns_worklist", ())
                assert len(wg) == len(ww), (tag, f)
                for g, w in [(got, want), *zip(wg, ww)]:
                    assert g.is_cuda and g.dtype == w.dtype \
                        and g.shape == w.shape, (tag, f)
                    assert torch.equal(g, w), (tag, f)
