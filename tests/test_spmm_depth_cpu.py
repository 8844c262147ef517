"""CPU tests of the wide SpMM's depth routing (ops.functional.spmm_depth)
and of the schedules tests/spmm_depth_checks.py runs the kernels on."""
import pytest
import torch

import spmm_depth_checks as D
from bnsgcn_amd.ops import functional as BF

KEYS = [(f, d) for f in D.FAMILIES for d in (torch.float32, torch.bfloat16)]


def test_swept_default(monkeypatch):
    monkeypatch.delenv("BNSGCN_SPMM_DEPTH", raising=False)
    assert set(BF.SPMM_DEPTH_SWEPT) == {
        (f, "bf16" if d == torch.bfloat16 else "fp32") for f, d in KEYS}
    for family, dtype in KEYS:
        name = "bf16" if dtype == torch.bfloat16 else "fp32"
        depth = BF.spmm_depth(family, dtype)
        assert depth == BF.SPMM_DEPTH_SWEPT[(family, name)]
        assert depth in BF.SPMM_DEPTHS == D.DEPTHS


@pytest.mark.parametrize("forced", D.DEPTHS)
def test_env_forces_depth(monkeypatch, forced):
    monkeypatch.setenv("BNSGCN_SPMM_DEPTH", str(forced))
    for family, dtype in KEYS:
        assert BF.spmm_depth(family, dtype) == forced


@pytest.mark.parametrize("value", ("0", "2", "5", "32", "-8", "", "deep"))
def test_unsupported_depth_means_4(monkeypatch, value):
    monkeypatch.setenv("BNSGCN_SPMM_DEPTH", value)
    for family, dtype in KEYS:
        assert BF.spmm_depth(family, dtype) == 4


def test_depth_argument_reaches_cpu_reference():
    """On the CPU `depth` selects nothing: the reference runs."""
    indptr, indices, n_cols = D.depthgraph()
    x = torch.randn(n_cols, 8, generator=D.gen(1))
    assert torch.equal(BF.spmm_sum_raw(indptr, indices, x, depth=16),
                       BF.spmm_sum_raw(indptr, indices, x))


@pytest.mark.parametrize("max_waves", D.MAX_WAVES)
@pytest.mark.parametrize("family", D.FAMILIES)
def test_schedules_have_the_promised_shape(family, max_waves):
    """Split row / group, repeated entry, item ranges, last item at the
    end of the array: asserted inside schedule()."""
    indptr, indices, _ = D.depthgraph()
    single = D.schedule(family, max_waves, indptr.clone(), indices)
    assert not single[D.LONG_ROW] and single[D.LONE_ROW]
    deg = indptr[1:] - indptr[:-1]
    assert set(D.DEGREES) <= set(deg.tolist())
    assert int(deg[-1]) == 64 and D.N_ROWS % 4 != 0
