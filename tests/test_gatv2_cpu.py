"""CPU: --gat-attn v2 — the flag and its validation, the autograd wiring of
F.gatv2_score (float64 gradcheck), the per-head padding of GATv2Layer, and
2-partition training against the single-process run."""
import numpy as np
import pytest
import torch

import test_train_cpu as T
from bnsgcn_amd.ops import functional as F
from bnsgcn_amd.ops.csr_torch import transpose_csr
from bnsgcn_amd.runtime.config import create_parser, gat_attn_of


def test_flag_and_validation():
    args = create_parser().parse_args(["--model", "gat"])
    assert args.gat_attn == "v1" and gat_attn_of(args) == "v1"
    for flag in ("--gat-attn", "--gat_attn"):
        args = create_parser().parse_args(["--model", "gat", flag, "v2"])
        assert gat_attn_of(args) == "v2"
    args.model = "graphsage"
    with pytest.raises(ValueError, match="--model gat"):
        gat_attn_of(args)
    args.model, args.gat_dtype = "gat", "bf16"
    with pytest.raises(ValueError, match="fp32"):
        gat_attn_of(args)


@pytest.mark.parametrize("shift", [3.0, -3.0])
def test_gatv2_score_gradcheck(shift):
    """12 x 10 CSR with an empty row; |zs| <= 1 and zd = shift + [-1, 1], so
    no s = zs + zd is within 1 of the kink: every edge on the positive
    branch (shift 3) or the negative one (shift -3)."""
    g = torch.Generator().manual_seed(3)
    deg = torch.randint(1, 5, (12,), generator=g)
    deg[4] = 0
    indptr = torch.zeros(13, dtype=torch.int64)
    indptr[1:] = deg.cumsum(0)
    indices = torch.randint(0, 10, (int(indptr[-1]),), generator=g).int()
    tip, tix, eperm = transpose_csr(indptr, indices, 10)
    H, D = 2, 4
    zs = (torch.rand(10, H, D, generator=g, dtype=torch.float64) * 2 - 1)
    zd = (torch.rand(12, H, D, generator=g, dtype=torch.float64) * 2 - 1) + shift
    attn = torch.randn(1, H, D, generator=g, dtype=torch.float64)
    for t in (zs, zd, attn):
        t.requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda a, b, c: F.gatv2_score(a, b, c, indptr, indices, tip, tix,
                                      eperm, 0.2), (zs, zd, attn))


def test_layer_padding_matches_unpadded_math():
    """D = 5 runs on Dp = 8 with zero pads; output and parameter gradients
    equal the unpadded definition in float64."""
    from bnsgcn_amd.models.context import GraphContext
    from bnsgcn_amd.models.layers import GATv2Layer
    g = torch.Generator().manual_seed(5)
    n, H, D, fin = 9, 2, 5, 6
    deg = torch.randint(1, 5, (n,), generator=g)
    deg[8] = 0                                             # no in-edge
    indptr = torch.zeros(n + 1, dtype=torch.int64)
    indptr[1:] = deg.cumsum(0)
    indices = torch.randint(0, n, (int(indptr[-1]),), generator=g).int()
    ctx = GraphContext.for_full_graph(indptr, indices, deg, deg, "cpu")
    lay = GATv2Layer(fin, D, H).double()
    lay.bias.data.normal_(generator=g)
    x = torch.randn(n, fin, generator=g, dtype=torch.float64)
    out = lay(ctx, x)
    got = torch.autograd.grad(out.square().sum(), list(lay.parameters()))

    ip, ix = ctx.gat_block()[:2]
    row = torch.repeat_interleave(torch.arange(n), ip[1:] - ip[:-1])
    zs = lay.fc_src(x).view(n, H, D)
    zd = lay.fc_dst(x).view(n, H, D)
    s = zs[ix.long()] + zd[row]
    e = (torch.nn.functional.leaky_relu(s, 0.2) * lay.attn).sum(-1)
    alpha = torch.zeros_like(e)
    for r in range(n):
        alpha[row == r] = torch.softmax(e[row == r], 0)
    want = torch.zeros(n, H, D, dtype=torch.float64).index_add_(
        0, row, alpha.unsqueeze(-1) * zs[ix.long()]) + lay.bias.view(1, H, D)
    torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-12)
    for a, b in zip(got, torch.autograd.grad(want.square().sum(),
                                             list(lay.parameters()))):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-12)


def test_gatv2_dist_matches_single_at_full_rate(tmp_path):
    """test_gat_dist_matches_single_at_full_rate with gat_attn = "v2"."""
    kw = dict(model="gat", gat_attn="v2", heads=2, n_hidden=8,
              sampling_rate=1.0, n_epochs=10)
    single = T._run_config(tmp_path / "s", 1, **kw)
    multi = T._run_config(tmp_path / "m", 2, **kw)
    lh_single = np.array(single[0]["loss_history"])
    lh_multi = (np.array(multi[0]["loss_history"])
                + np.array(multi[1]["loss_history"]))
    np.testing.assert_allclose(lh_multi, lh_single, rtol=5e-3, atol=1e-3)
    v1 = T._run_config(tmp_path / "v1", 1, **dict(kw, gat_attn="v1"))
    assert not np.allclose(np.array(v1[0]["loss_history"]), lh_single)
