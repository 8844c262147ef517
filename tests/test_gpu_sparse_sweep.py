"""GPU (MI355X) sweep of the work-list kernels — spmm_sum (five forms),
sddmm_add, spmm_edge (two), sddmm_dot (three), segment_sum_edges (two) —
over graph shapes, schedules and the launchers' routing edges.

The other GPU files run these kernels on one graph under the default
schedule (72 waves, one item per non-empty row). Here every (op, graph)
test loops over the schedules (seg, max_waves) in {(1, 8), (3, 24),
(64, default), (65, 8), (512, 8), (512, default)}: capped schedules in
which a wave owns a long run of items, every edge an atomic item, items on
the wave-width boundary, grids of fewer than 8 blocks. The schedule is
attached to the device indptr (tests/sparse_sweep_checks.py), which also
holds the graph family, the oracle and the tolerances; nothing here starts
a child process.

Run on the GPU box: python -m pytest tests/test_gpu_sparse_sweep.py -m gpu -x -q
"""
import pytest
import torch

import kernel_path_checks as K
import sparse_sweep_checks as S

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


@needs_gpu
@pytest.mark.parametrize("name", S.SWEEP_GRAPHS)
def test_spmm_sum_sweep(name):
    """F = 1 (scalar), 2 (vec2), 4 and 64 (edge-parallel narrow form),
    68 (half-wave), 132 (f4 = 33, first full-wave width), 257 (scalar,
    second pass with one live lane), 514 (vec2 second pass), 516 (vec4
    second pass with only lane 0 live); with and without the scales and
    out=."""
    S.check_spmm_sum_sweep(name)


@needs_gpu
@pytest.mark.parametrize("name", S.SWEEP_GRAPHS)
def test_spmm_edge_sweep(name):
    """(H, D) = (4, 132): H*D/4 = 132, a partial second pass of the vec4
    form; (1, 4) one live lane; (4, 41) and (1, 1) the wave-per-(row, head)
    form; plain, out= and transposed-with-wperm calls."""
    S.check_spmm_edge_sweep(name)


@needs_gpu
@pytest.mark.parametrize("name", S.SWEEP_GRAPHS)
def test_sddmm_dot_sweep(name):
    """Fast form at every group size D/8 in {1, 2, 4, 32, 64}; (3, 256)
    (H*D > 512), (1, 24) (D/8 = 3, no power of two) and (1, 4) (D/8 = 0)
    must fall through to the vec4 form, (4, 41) to the general one."""
    S.check_sddmm_dot_sweep(name)


@needs_gpu
@pytest.mark.parametrize("name", S.SWEEP_GRAPHS)
def test_sddmm_add_autograd_sweep(name):
    """sddmm_add forward and, through autograd, segment_sum_edges in both
    forms on both CSRs; H = 16 takes _SDDMMAdd.backward's index_add_ route
    on device tensors. Slopes: none and 0.2."""
    S.check_sddmm_add_autograd(name)


@needs_gpu
@pytest.mark.parametrize("H,D", [(3, 5), (16, 8)])
def test_attn_project_fallbacks_on_device(H, D):
    """H*D % 4 != 0 and H > 8: _AttnProject runs the ops/reference.py
    formulas on device tensors, forward and backward."""
    S.note("attn_project", K.check_attn_project(H, D, 130))


@needs_gpu
def test_grid_residues():
    """The fixture graph at seg = 64 with max_waves = 8, 16, ..., 64:
    F = 128 (half-wave form, 8 subgroups per block) launches 1..8 blocks,
    F = 256 and F = 8 (narrow form) 2, 4, ..., 16, as do the other ops —
    every residue of the grid size mod 8 goes through xcd_remap_block,
    nb < 8 included."""
    scheds = tuple((64, m) for m in range(8, 72, 8))
    for s in scheds:
        assert S.n_waves_of(S.device_csr("fixture", s)[0]) == s[1]
    S.check_spmm_sum_sweep("fixture", scheds, (128, 256, 8))
    S.check_spmm_edge_sweep("fixture", scheds, ((4, 16),))
    S.check_sddmm_dot_sweep("fixture", scheds, ((4, 16), (1, 24), (4, 41)))
    S.check_sddmm_add_autograd("fixture", scheds, (3, 4))


@needs_gpu
@pytest.mark.parametrize("name", S.DEGENERATE)
@pytest.mark.parametrize("op", ["spmm_sum", "spmm_edge", "sddmm_dot",
                                "sddmm_add"])
def test_degenerate_graphs(op, name):
    S.check_degenerate(op, name)


@needs_gpu
@pytest.mark.parametrize("n,n_waves", [(999_999, 131072),
                                       (1_000_000, 262144)])
@pytest.mark.parametrize("op", ["spmm_sum_4", "spmm_sum_64", "sddmm_add_4"])
def test_million_item_branch(op, n, n_waves):
    """1,000,000 rows of degree 1 into 1000 columns: the smallest graph
    that takes build_worklist's `total >= 1_000_000` branch (262144 waves,
    a 65,536-block grid); 999,999 rows stay on 131072 waves."""
    S.check_unit_degree(op, n, n_waves)
