"""CPU tests of --gat-dtype bf16: the flag and its environment default, the
refusal for models other than GAT, the unchanged default, and the CPU form
of the rule — in float64 the forward, gx and gw of spmm_edge_sum equal the
reference evaluated on the rounded operands exactly.
"""
import pytest
import torch

import kernel_path_checks as K
import test_train_cpu as T
from kernel_path_checks import N_COLS, N_ROWS, gen

from bnsgcn_amd.ops import reference as ref
from bnsgcn_amd.runtime.config import create_parser, gat_dtype_of

BF16 = torch.bfloat16


def test_parser_and_environment_default(monkeypatch):
    monkeypatch.delenv("BNSGCN_GAT_DTYPE", raising=False)
    args = create_parser().parse_args(["--model", "gat"])
    assert args.gat_dtype == "fp32" and gat_dtype_of(args) is None
    for flag in ("--gat-dtype", "--gat_dtype"):
        args = create_parser().parse_args(["--model", "gat", flag, "bf16"])
        assert args.gat_dtype == "bf16" and gat_dtype_of(args) == BF16
    with pytest.raises(SystemExit):
        create_parser().parse_args(["--gat-dtype", "fp16"])
    args.gat_dtype = "fp16"
    with pytest.raises(ValueError, match="gat-dtype"):
        gat_dtype_of(args)
    monkeypatch.setenv("BNSGCN_GAT_DTYPE", "bf16")
    assert create_parser().parse_args([]).gat_dtype == "bf16"
    assert create_parser().parse_args(["--gat-dtype", "fp32"]).gat_dtype \
        == "fp32"


@pytest.mark.parametrize("model", ["gcn", "graphsage"])
def test_other_models_with_bf16_raise(tmp_path, model):
    args = create_parser().parse_args(["--model", model, "--gat-dtype",
                                       "bf16"])
    with pytest.raises(ValueError, match="gat-dtype"):
        gat_dtype_of(args)
    # and at start-up of a run, before any work
    from bnsgcn_amd.runtime.trainer import run
    args = T.make_args(tmp_path, model=model, gat_dtype="bf16",
                       n_partitions=1)
    with pytest.raises(ValueError, match="gat-dtype"):
        run(args, rank=0, world_size=1)
    args.model = "gat"
    assert gat_dtype_of(args) == BF16


def _edge_case(dtype, H=3, D=6):
    from bnsgcn_amd.ops.csr_torch import transpose_csr
    indptr, indices = K.fixture_csr()
    csr = (indptr, indices) + tuple(transpose_csr(indptr, indices, N_COLS))
    g = gen(8200)
    x = torch.randn(N_COLS, H, D, generator=g).to(dtype)
    w = torch.randn(indices.numel(), H, generator=g).to(dtype)
    gy = torch.randn(N_ROWS, H, D, generator=g).to(dtype)
    return csr, x, w, gy


def test_context_default_changes_nothing():
    from bnsgcn_amd.models.context import GraphContext
    from bnsgcn_amd.ops.functional import spmm_edge_sum
    indptr, indices = K.fixture_csr()
    deg = torch.ones(N_ROWS)
    ctx = GraphContext(indptr, indices, deg, deg, "cpu")
    assert ctx.gat_dtype is None
    csr, x, w, _ = _edge_case(torch.float32)
    plain = spmm_edge_sum(x, w, *csr)
    for dt in (None, torch.float32):
        assert torch.equal(spmm_edge_sum(x, w, *csr, src_dtype=dt), plain)
    assert not torch.equal(spmm_edge_sum(x, w, *csr, src_dtype=BF16), plain)
    with pytest.raises(ValueError):
        spmm_edge_sum(x, w, *csr, src_dtype=torch.float16)


def test_spmm_edge_sum_float64_follows_the_rule():
    """forward = ref(w, q(x)); gx = ref(A^T, w[eperm], q(grad)); gw =
    sddmm_dot(grad, q(x)) with grad unrounded — all exact in float64."""
    from bnsgcn_amd.ops.functional import spmm_edge_sum
    csr, x, w, gy = _edge_case(torch.float64)
    indptr, indices, tip, tix, eperm = csr
    xq, gq = x.float().to(BF16).double(), gy.float().to(BF16).double()
    assert not torch.equal(xq, x) and not torch.equal(gq, gy)
    xd, wd = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = spmm_edge_sum(xd, wd, *csr, src_dtype=BF16)
    y.backward(gy)
    assert torch.equal(y.detach(), ref.spmm_edge_sum(indptr, indices, w, xq))
    assert torch.equal(xd.grad, ref.spmm_edge_sum(tip, tix, w[eperm], gq))
    assert torch.equal(wd.grad, ref.sddmm_dot(indptr, indices, gy, xq))
