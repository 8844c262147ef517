"""GPU (MI355X) tests of the row-group SpMM: spmm_sum_grouped_kernel
behind ops.functional.spmm_sum_raw on CSRs that carry the format of
ops/csr_torch.build_rowgroups. Graphs, oracle (float64 ops/reference.py),
tolerance (assert_sum_bound) and the check functions live in
tests/rowgroup_checks.py.

Run on the GPU box: python -m pytest tests/test_gpu_rowgroup_spmm.py -m gpu -x -q
"""
import os
import subprocess
import sys

import pytest
import torch

import rowgroup_checks as G

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


@needs_gpu
@pytest.mark.parametrize("R", G.RS)
@pytest.mark.parametrize("name", G.GPU_GRAPHS)
def test_grouped_sweep(name, R):
    """F = 132 (f4 = 33, first routed width), 256, 260 (one live lane in
    the second float4), 516 (second pass); scales on/off; overwrite from a
    NaN-prefilled allocation and out=; gseg 1 (every group split), 3, 64
    and 65 (items on the chunk boundary), default (nothing split).
    `dup256` is the count-overflow row, `hubcol` the 130-fold one."""
    G.check_grouped_sweep(name, R)


@needs_gpu
@pytest.mark.parametrize("name", ("empty", "norows"))
def test_grouped_degenerate(name):
    """No edge / no row: nothing is launched, zeros (or nothing) come
    back, out= is left unchanged."""
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    indptr, indices, n_cols = G.graph(name)
    n_rows = indptr.numel() - 1
    ip, ix = G.device_csr(name, 8, None)
    x = torch.randn(n_cols, 256, device=G.DEV)
    base = torch.randn(n_rows, 256, device=G.DEV)
    assert torch.equal(spmm_sum_raw(ip, ix, x).cpu(), torch.zeros(n_rows, 256))
    assert torch.equal(spmm_sum_raw(ip, ix, x, out=base.clone()), base)


@needs_gpu
@pytest.mark.parametrize("R", G.RS)
def test_isolation(R):
    G.check_isolation(R)


@needs_gpu
@pytest.mark.parametrize("R", G.RS)
def test_reproducible(R):
    G.check_reproducible(R)


@needs_gpu
def test_routing_without_attribute():
    G.check_routing_no_attribute()


@needs_gpu
def test_routing_narrow_widths_keep_their_kernels():
    G.check_routing_narrow_widths(8)


@needs_gpu
def test_routing_env_off_in_child():
    env = dict(os.environ, **G.CASES["group_off"][0])
    r = subprocess.run([sys.executable, G.__file__, "group_off"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "group_off: ok" in r.stdout


@needs_gpu
@pytest.mark.parametrize("mode", ("mean", "gcn"))
def test_end_to_end_aggregate(mode, monkeypatch):
    G.check_end_to_end(mode, monkeypatch)
