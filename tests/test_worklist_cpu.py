"""Property tests of ops/csr_torch.build_worklist, the schedule every
work-list kernel reads (spmm_sum, spmm_edge, sddmm_dot, sddmm_add,
segment_sum_edges). The contract itself is
sparse_sweep_checks.assert_worklist_contract: items tile [0, E) in order
inside their rows with 1..seg edges each, the atomic flag marks exactly
the rows longer than seg, zero_rows is exactly the empty plus the split
rows, the launcher's dtypes, wave_start monotone from 0 to the item count,
n_waves = roundup8(min(max_waves, max(8, items))), and every wave holds
less than one longest item more than E / n_waves edges.

CPU only; the GPU sweep (test_gpu_sparse_sweep.py) checks the same
contract on the schedules it builds on the device.
"""
import pytest
import torch

import sparse_sweep_checks as S
from bnsgcn_amd.ops import csr_torch
from bnsgcn_amd.ops.csr_torch import build_worklist


@pytest.mark.parametrize("name", S.CPU_FAMILY)
def test_worklist_contract_family(name):
    indptr = S.graph(name)[0]
    worst = 0.0
    for seg in S.SEGS:
        for mw in S.MAX_WAVES:
            wl = build_worklist(indptr, seg=seg, max_waves=mw)
            worst = max(worst,
                        S.assert_worklist_contract(indptr, wl, seg, mw))
    print(f"{name}: worst balance ratio {worst:.3f} of one item length")


def test_family_is_what_it_claims():
    """The shapes the family is there for: split rows at every seg below
    the longest row, fewer than 8 items, a single row, a lone last row."""
    deg = {n: (S.graph(n)[0][1:] - S.graph(n)[0][:-1]) for n in S.CPU_FAMILY}
    assert deg["zipf"].numel() == 300 and int(deg["zipf"].max()) == 3000
    assert int((deg["zipf"] == 0).sum()) == 90
    assert deg["onerow"].tolist() == [5000]
    assert deg["lastrow"].tolist() == [0] * 40 + [77]
    assert deg["tiny"].tolist() == [1, 0, 2]
    assert deg["empty"].numel() == 17 and int(deg["empty"].sum()) == 0
    assert deg["norows"].numel() == 0
    for n in S.SWEEP_GRAPHS:
        assert S.graph(n)[2] <= 200
    ip, ix, _ = S.graph("hubcol")
    assert int(ip[2] - ip[1]) == 130 and not ix[ip[1]:ip[2]].any()
    # items << waves, and a capped schedule: items >> waves
    assert build_worklist(deg_to_indptr([1, 0, 2]), seg=512)[0].numel() == 2
    wl = build_worklist(S.graph("zipf")[0], seg=1, max_waves=8)
    assert wl[0].numel() == int(deg["zipf"].sum()) and wl[3].numel() == 9


def deg_to_indptr(deg):
    return torch.cat([torch.zeros(1, dtype=torch.int64),
                      torch.cumsum(torch.tensor(deg, dtype=torch.int64), 0)])


@pytest.mark.parametrize("n,default_waves", [(999_999, 131072),
                                             (1_000_000, 262144)])
def test_worklist_million_item_branch(n, default_waves, monkeypatch):
    """One item per row on either side of the `total >= 1_000_000`
    branch, which raises max_waves to at least 262144 whatever was asked
    for; below it an explicit max_waves still caps the schedule."""
    monkeypatch.setattr(csr_torch, "MAX_WAVES", 131072)  # the shipped default
    indptr = torch.arange(n + 1, dtype=torch.int64)
    for seg in S.SEGS:
        for mw in S.MAX_WAVES:
            wl = build_worklist(indptr, seg=seg, max_waves=mw)
            S.assert_worklist_contract(indptr, wl, seg, mw)
            n_waves = wl[3].numel() - 1
            if mw is None or n >= 1_000_000:
                assert n_waves == default_waves
            else:
                assert n_waves == mw
            assert wl[4].numel() == 0


def test_worklist_defaults():
    """seg=None / max_waves=None fall back to csr_torch.SEG and
    csr_torch.MAX_WAVES (read at call time)."""
    indptr = deg_to_indptr([7, 0, 40, 3] * 5)
    assert all(torch.equal(a, b) for a, b in zip(
        build_worklist(indptr),
        build_worklist(indptr, seg=csr_torch.SEG,
                       max_waves=csr_torch.MAX_WAVES)))
    old = csr_torch.SEG, csr_torch.MAX_WAVES
    try:
        csr_torch.SEG, csr_torch.MAX_WAVES = 5, 16
        got = build_worklist(indptr)
        S.assert_worklist_contract(indptr, got, 5, 16)
        assert all(torch.equal(a, b) for a, b in zip(
            got, build_worklist(indptr, seg=5, max_waves=16)))
        assert int((got[2] - got[1]).max()) == 5       # 40 = 8 items of 5
        assert got[3].numel() - 1 == 16
        # an explicit argument wins over the module value
        assert build_worklist(indptr, seg=64, max_waves=8)[3].numel() == 9
    finally:
        csr_torch.SEG, csr_torch.MAX_WAVES = old
