"""GPU (MI355X) tests of the row-group form of the narrow SpMM:
spmm_sum_grouped_narrow_kernel behind ops.functional.spmm_sum_raw on CSRs
whose row-group format allows narrow calls. Graphs, oracle (float64
ops/reference.py), tolerance (assert_sum_bound) and the check functions
live in tests/narrow_rowgroup_checks.py and tests/rowgroup_checks.py.

Run on the GPU box: python -m pytest tests/test_gpu_narrow_rowgroup.py -m gpu -x -q
"""
import os
import subprocess
import sys

import pytest
import torch

import narrow_rowgroup_checks as N
import partition_path_checks as P
import project_first_checks as L
import rowgroup_checks as G

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


@needs_gpu
@pytest.mark.parametrize("R", N.RS)
@pytest.mark.parametrize("name", G.GPU_GRAPHS)
def test_narrow_grouped_sweep(name, R):
    """F = 4 (one live lane per lane group), 44 (the headline), 60, 64
    (every lane live); scales on/off; overwrite from a NaN-prefilled
    allocation and out=; gseg 1 (every group split), 3, 4, 5 (around the 4
    entries of a step), 64 and 65 (the chunk boundary), default."""
    N.check_narrow_sweep(name, R)


@needs_gpu
@pytest.mark.parametrize("name", ("empty", "norows"))
def test_narrow_grouped_degenerate(name):
    """No edge / no row: nothing is launched, zeros (or nothing) come
    back, out= is left unchanged."""
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    indptr, indices, n_cols = G.graph(name)
    n_rows = indptr.numel() - 1
    ip, ix = N.narrow_csr(name, 4, None)
    x = torch.randn(n_cols, 44, device=G.DEV)
    base = torch.randn(n_rows, 44, device=G.DEV)
    with G.count_grouped() as calls:
        assert torch.equal(spmm_sum_raw(ip, ix, x).cpu(),
                           torch.zeros(n_rows, 44))
        assert torch.equal(spmm_sum_raw(ip, ix, x, out=base.clone()), base)
    assert calls[0] == 2


@needs_gpu
@pytest.mark.parametrize("R", N.RS)
def test_narrow_isolation(R):
    N.check_isolation(R)


@needs_gpu
@pytest.mark.parametrize("R", N.RS)
def test_narrow_reproducible(R):
    N.check_reproducible(R)


@needs_gpu
def test_narrow_only_format_keeps_wide_forward():
    N.check_routing_narrow_only_keeps_wide_forward(4)


@needs_gpu
def test_bf16_source_stays_per_row():
    N.check_routing_bf16_source_stays_per_row(4)


@needs_gpu
def test_routing_f68_and_env_off_in_child(tmp_path):
    """F = 68 on the format-carrying CSRs runs the per-row path, and gives
    bit for bit what a BNSGCN_SPMM_GROUP=0 process gives."""
    path = str(tmp_path / "f68.pt")
    torch.save({R: N.routing_f68(R) for R in N.RS}, path)
    env = dict(os.environ, BNSGCN_SPMM_GROUP="0")
    r = subprocess.run([sys.executable, N.__file__, "group_off", path],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "group_off: ok" in r.stdout


@needs_gpu
def test_gathered_csrs_meet_contract(monkeypatch):
    from bnsgcn_amd.ops import functional as BF
    monkeypatch.setattr(BF, "GROUP_TAU", 1.0)
    monkeypatch.setattr(BF, "GROUP_TAU_NARROW", 1.0)
    for rank in range(3):
        N.check_gathered_contract(rank, G.DEV)


@needs_gpu
def test_sage_layer_train_rows_formats_forced(monkeypatch):
    """A (64, 41) SAGE layer on every rank of the 3-partition fixture under
    the stub exchange, rows = the rank's train rows, keep rule lifted so
    that both gathered CSRs carry the format: forward and backward each
    make one grouped narrow call at F = 44. Against the aggregate-first
    formula in float64 on the CPU under compare_measured, as
    test_project_first_layer_train_rows_gpu."""
    from bnsgcn_amd.ops import functional as BF
    monkeypatch.setattr(BF, "GROUP_TAU_NARROW", 1.0)
    _, parts = P.fixture_parts(3)
    for part in parts:
        case = L.Case("sage", 64, 41, "partition", True, rank=part.rank)
        ref64 = L.run(case, "agg_first", "cpu", torch.float64)
        ref32 = L.run(case, "agg_first", "cpu", torch.float32)
        with G.count_grouped() as calls:
            got = L.run(case, "layer", P.DEV, torch.float32)
        assert calls[0] == 2, "forward and backward must both be grouped"
        assert got.pop("agg width") == 44
        ref64.pop("agg width"), ref32.pop("agg width")
        P.compare_measured(ref64, ref32, got, f"sage rank {part.rank}")
