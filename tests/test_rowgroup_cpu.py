"""Row-group format builder (ops/csr_torch.build_rowgroups) on the CPU:
the contract of tests/rowgroup_checks.assert_rowgroup_contract over the
graph family, R in {4, 8, 16} and gseg in {1, 3, 64, 65, 512}."""
import pytest
import torch

import rowgroup_checks as G
from bnsgcn_amd.ops.csr_torch import build_rowgroups


@pytest.mark.parametrize("R", G.RS_BUILDER)
@pytest.mark.parametrize("name", G.CPU_GRAPHS)
def test_rowgroup_contract(name, R):
    indptr, indices, n_cols = G.graph(name)
    E = indices.numel()
    for gseg in G.GSEGS_CPU:
        rg = build_rowgroups(indptr, indices, n_cols, R=R, gseg=gseg)
        n_ent, n_split = G.assert_rowgroup_contract(indptr, indices, n_cols,
                                                    rg, R, gseg)
        assert n_ent <= E or name == "dup256"
        if gseg == 1:
            # every group with two entries or more is split
            assert n_split == sum(
                1 for c in torch.bincount(
                    torch.where(rg.sched[0] < 0, ~rg.sched[0],
                                rg.sched[0]).long()).tolist() if c > 1)


@pytest.mark.parametrize("R", G.RS_BUILDER)
def test_count_overflow_repeats_entry(R):
    """256 parallel edges: two entries for the one column, 255 + 1, never
    a clamped count; hubcol's 130 parallel edges fit one field."""
    indptr, indices, n_cols = G.graph("dup256")
    rg = build_rowgroups(indptr, indices, n_cols, R=R, gseg=512)
    assert rg.ecol.tolist() == [1, 1]
    assert rg.ew[:, 0].tolist() == [255, 1]
    assert int(rg.ew[:, 1:].sum()) == 0
    assert rg.ratio == 2 / 256
    indptr, indices, n_cols = G.graph("hubcol")
    rg = build_rowgroups(indptr, indices, n_cols, R=R, gseg=512)
    assert 130 in rg.ew[:, 1].tolist()


def test_ratio_counts_shared_neighbours():
    """Eight rows with the same three neighbours: 3 entries for 24 edges
    at R = 8, 6 at R = 4."""
    indptr = torch.arange(0, 25, 3)
    indices = torch.tensor([4, 0, 2] * 8, dtype=torch.int32)
    rg = build_rowgroups(indptr, indices, 5, R=8, gseg=512)
    assert rg.ecol.tolist() == [0, 2, 4] and rg.ratio == 3 / 24
    assert (rg.ew == 1).all()
    assert build_rowgroups(indptr, indices, 5, R=4, gseg=512).ratio == 6 / 24
