"""GPU (MI355X) tests of the depth parameter of the wide SpMM kernels
(spmm_sum_wide_kernel, spmm_sum_grouped_kernel): depths 8 and 16 against
depth 4 of the same build — bitwise on single-writer rows — and every depth
against the float64 reference. Graph, schedules, oracle and tolerance are
described in tests/spmm_depth_checks.py.

Run on the GPU box: python -m pytest tests/test_gpu_spmm_depth.py -m gpu -x -q
"""
import pytest
import torch

import spmm_depth_checks as D

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


@needs_gpu
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("F", D.WIDTHS)
@pytest.mark.parametrize("family", D.FAMILIES)
def test_depths_same_sums(family, F, dtype):
    """F = 132 and 256 (one float4 per lane; lanes past the row end at
    132), 260 (one live lane in the second float4), 512, 516 (second
    pass); with and without scales, overwrite from a NaN-prefilled
    allocation and out=; item ranges and single items."""
    D.check_depths(family, F, dtype)


@needs_gpu
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("depth", (8, 16))
def test_grouped_isolation(depth, dtype):
    D.check_isolation(depth, dtype)
