"""GPU (MI355X): the one-launch boundary selection (ops/hip/bns_select.hip)
against a stable argsort of the same keys on the CPU, against the numpy
Philox sampler, and — through HaloPlan._build — against the plan sampled
with torch sorts. Integer (and copied float) outputs: dtype, shape and
torch.equal, no tolerance.

  python -m pytest tests/test_gpu_bns_select.py -m gpu -x -q
"""
import numpy as np
import pytest
import torch

import partition_path_checks as P
from partition_path_checks import DEV

from bnsgcn_amd.ops import bns_select as B
from bnsgcn_amd.ops.philox import sample_boundary

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="no GPU")]

if torch.cuda.is_available():
    from bnsgcn_amd.ops._ext import require_ext
    CAP = require_ext().BNS_SELECT_CAP    # new binding: fails on the parent
else:
    CAP = 4096
SIZES = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 5)


def sizes_s(n):
    return (0, 1, n // 2, n - 1, n, n + 3)


def raw_keys(pattern, n):
    """int64 keys in [0, 2^63) of one segment."""
    i = torch.arange(n, dtype=torch.int64)
    if pattern == "equal":          # ties decide everything
        return torch.full((n,), 5, dtype=torch.int64)
    if pattern == "low3":           # top 60 bits shared: every level runs
        return (i * 5 + 3) % 8
    if pattern == "descending":
        return (1 << 40) + n - i
    if pattern == "top11":          # one key per first-level bin
        return ((i * 7 + 1) % 2048) << 52
    g = torch.Generator().manual_seed(n)
    k = torch.randint(0, 2 ** 63 - 1, (n,), generator=g, dtype=torch.int64)
    if n > 1024:                    # duplicates across the chunk boundary
        k[1024] = k[1023] = k[5]
        k[n - 1] = k[1000]
    return k


@pytest.mark.parametrize("pattern,cap", [
    ("equal", CAP), ("low3", CAP), ("descending", CAP), ("top11", CAP),
    ("random", CAP), ("equal", 64), ("low3", 64), ("descending", 64)])
def test_select_smallest(pattern, cap):
    """Every (n, s) of the grid in one call, segments with s = 0 or n = 0
    between full ones."""
    segs = [(raw_keys(pattern, n), s) for n in SIZES for s in sizes_s(n)]
    ptr = np.cumsum([0] + [k.numel() for k, _ in segs]).tolist()
    want = [torch.sort(torch.argsort(k, stable=True)[:max(s, 0)])[0]
            for k, s in segs]
    out, out_ptr = B.select_smallest(torch.cat([k for k, _ in segs]).to(DEV),
                                     ptr, [s for _, s in segs], cap=cap)
    assert out.is_cuda and out.dtype == torch.int64
    assert out_ptr == np.cumsum([0] + [w.numel() for w in want]).tolist()
    assert out.shape == (out_ptr[-1],)
    out = out.cpu()
    for k, (w, (_, s)) in enumerate(zip(want, segs)):
        assert torch.equal(out[out_ptr[k]:out_ptr[k + 1]], w), (
            pattern, cap, w.numel(), s)


@pytest.mark.parametrize("seed", [7, (1 << 40) + 12345])
@pytest.mark.parametrize("epoch,src,dst", [(0, 0, 1), (3, 5, 2)])
def test_philox_matches_sample_boundary(seed, epoch, src, dst):
    cases = [(n, s) for n in SIZES[6:] for s in sizes_s(n)]
    cases.append((200_003, int(0.1 * 200_003)))
    sel = B.PlanSelect([(n, s, src, dst, B.KIND_HALO, 0) for n, s in cases],
                       seed, DEV)
    pack, hsel, norm, deg = sel(epoch)
    assert pack.numel() == norm.numel() == deg.numel() == 0
    assert hsel.is_cuda and hsel.dtype == torch.int64
    want = [torch.from_numpy(sample_boundary(n, s, seed, epoch, src, dst))
            for n, s in cases]
    assert hsel.shape == (sum(w.numel() for w in want),)
    for (n, s), got, w in zip(cases, hsel.cpu().split(
            [w.numel() for w in want]), want):
        assert torch.equal(got, w), (n, s)


@pytest.mark.parametrize("unit_ratio", [False, True])
@pytest.mark.parametrize("rate", [0.4, 0.02])
def test_plan_same_with_switch_off(rate, unit_ratio, monkeypatch):
    """HaloPlan._build on the device with the HIP selection against the
    same plan sampled with torch sorts. At rate 0.02 the fixture's segments
    hold 0 or 1 rows and ranks 0 and 1 receive nothing."""
    assert B.SAMPLE_HIP
    for part in P.fixture_parts(3)[1]:
        plan = P.make_plan(part, rate, DEV, unit_ratio=unit_ratio)
        for epoch in (0, 3):
            states = []
            for on in (True, False):
                monkeypatch.setattr(B, "SAMPLE_HIP", on)
                states.append(plan._build(epoch))
            on, off = states
            tag = (part.rank, rate, unit_ratio, epoch)
            assert on.send_counts == off.send_counts, tag
            assert on.recv_counts == off.recv_counts, tag
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
