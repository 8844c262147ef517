"""CPU side of the row-group form of the narrow SpMM: which calls
ops.functional routes to a format, the RowGroups flags, and that a CPU
context attaches nothing to its gathered CSRs. Check functions live in
tests/narrow_rowgroup_checks.py."""
import pytest
import torch

import narrow_rowgroup_checks as N
import rowgroup_checks as G
from bnsgcn_amd.ops import functional as BF
from bnsgcn_amd.ops import reference as ref
from bnsgcn_amd.ops.csr_torch import (build_rowgroups, gather_rows_csr,
                                      transpose_csr)


def test_builder_leaves_narrow_off():
    """A format straight from the builder serves wide calls only: narrow
    calls need the caller's (attach_rowgroups') consent."""
    rg = build_rowgroups(*G.graph("fixture"))
    assert rg.wide and not rg.narrow


@pytest.mark.parametrize("wide", (False, True))
@pytest.mark.parametrize("narrow", (False, True))
def test_route_by_width_and_flags(wide, narrow):
    """F / 4 in 1..16 follows `narrow` (fp32 source only), 17..32 is never
    grouped, above 32 follows `wide`; F % 4 != 0 and no format: never."""
    rg = build_rowgroups(*G.graph("tiny"))._replace(wide=wide, narrow=narrow)
    for F in range(1, 140):
        x = torch.empty(0, F)
        f4 = F // 4
        want = F % 4 == 0 and ((f4 <= 16 and narrow) or (f4 > 32 and wide))
        assert BF._grouped_route(rg, x) == want, F
        assert not BF._grouped_route(None, x)
        xb = x.bfloat16()
        assert BF._grouped_route(rg, xb) == (F % 4 == 0 and f4 > 32 and wide)
    assert not BF._grouped_route(rg, torch.empty(0, 0))


def test_attach_rowgroups_builds_nothing_on_cpu():
    indptr, indices, n_cols = G.graph("fixture")
    ip = indptr.clone()
    assert BF.attach_rowgroups(ip, indices, n_cols) is None
    assert not hasattr(ip, "_bns_rowgroups")


@pytest.mark.parametrize("rank", range(3))
def test_cpu_context_gathered_csrs_carry_no_format(rank):
    """_rows_inner_csrs attaches nothing on the CPU, and aggregate over the
    loss rows is the reference SpMM on the gathered CSR, bit for bit."""
    N.check_gathered_contract(rank, "cpu")
    ctx, rows, _ = N.fixture_context(rank, "cpu")
    ip, ix, tip, tix = ctx._rows_inner_csrs(rows)
    want_ip, want_ix = gather_rows_csr(ctx.indptr, ctx.indices, rows)
    assert torch.equal(ip, want_ip) and torch.equal(ix, want_ix)
    x = torch.randn(ctx.plan.n_inner, 44,
                    generator=torch.Generator().manual_seed(rank))
    got = BF.spmm_sum_raw(ip, ix, x, None, ctx.in_deg_inv[rows])
    assert torch.equal(got, ref.spmm_sum(ip, ix, x, None,
                                         ctx.in_deg_inv[rows]))


@pytest.mark.parametrize("R", (4, 8))
@pytest.mark.parametrize("rank", range(3))
def test_gathered_csrs_meet_contract_cpu(rank, R):
    """The builder's contract on the train-row-gathered CSRs of the
    fixture and their transposes."""
    ctx, rows, _ = N.fixture_context(rank, "cpu")
    ip, ix = gather_rows_csr(ctx.indptr, ctx.indices, rows)
    n_src = ctx.plan.n_inner
    tip, tix, _ = transpose_csr(ip, ix, n_src)
    for gseg in (3, 64, 1024):
        G.assert_rowgroup_contract(
            ip, ix, n_src, build_rowgroups(ip, ix, n_src, R=R, gseg=gseg),
            R, gseg)
        G.assert_rowgroup_contract(
            tip, tix, rows.numel(),
            build_rowgroups(tip, tix, rows.numel(), R=R, gseg=gseg), R, gseg)
