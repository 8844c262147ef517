"""Runner for the project-then-aggregate layer tests
(tests/test_project_first_cpu.py, tests/test_gpu_narrow_spmm.py).

run(case, "layer", ...) calls the layer's own forward; run(case,
"agg_first", ...) evaluates the order the layers had before — aggregate
the in_feats-wide input with ctx.aggregate, then
torch.nn.functional.linear — on the same parameters and inputs. Both
return the output and every gradient as CPU tensors.

One rank of a 3-partition job under a stubbed exchange: the two orders
put DIFFERENT tensors on the wire (projected rows of pad4(out) floats
against raw rows of in_feats), so the stub cannot hand both the same
rows. With H the raw rows the peers would send, B the gradient rows they
would return for the projected send, and Wp the zero-padded weight, the
stub is kept consistent with linearity:

                    forward receive      backward receive
    agg_first       H                    B @ Wp
    layer           H @ Wp^T             B

Output, d x, the bias gradients and the self-term weight gradient then
agree between the orders. The gradient of the AGGREGATED weight does not
agree per rank, and must not: with T1 the rank-local term,

    agg_first:  dW = T1 + gr^T H        (gr = this rank's backward send,
                                         in projected width)
    layer:      dW = T1 + B^T pack      (pack = scale * x[pack_idx], the
                                         raw forward send)

— the halo term moves from the receiver of a row to its sender, and only
the sum over ranks is the same. The runner therefore reports
dW + gr^T H for "layer" and dW + B^T pack for "agg_first" (each from the
sends that run recorded), which are equal, and both wire tensors mapped
to the other order's width.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

import partition_path_checks as P

RATE, EPOCH = 0.4, 3


@dataclasses.dataclass(frozen=True)
class Case:
    kind: str           # "sage" | "gcn"
    fin: int
    fout: int
    where: str          # "full" | "partition"
    use_rows: bool
    rank: int = 0


class LinearStub:
    """Drop-in for comm.all_to_all_rows: records each send (CPU copy) and
    fills the k-th receive buffer with fills[k]."""

    def __init__(self, fills):
        self.fills, self.log = list(fills), []

    def __call__(self, recv, send, recv_counts, send_counts, async_op=False):
        rows = self.fills[len(self.log)]
        self.log.append(send.detach().cpu().clone())
        assert tuple(rows.shape) == tuple(recv.shape), (rows.shape, recv.shape)
        recv.copy_(rows.to(recv.dtype))
        return None


def make_layer(case: Case):
    from bnsgcn_amd.models.layers import GCNLayer, SAGELayer
    torch.manual_seed(7 + case.fin + case.fout)
    cls = SAGELayer if case.kind == "sage" else GCNLayer
    return cls(case.fin, case.fout)


def agg_weight_name(case: Case) -> str:
    return "linear2.weight" if case.kind == "sage" else "linear.weight"


def _agg_first(layer, case, ctx, x, rows):
    lin = torch.nn.functional.linear
    if case.kind == "gcn":
        return lin(ctx.aggregate(x, "gcn", rows=rows), layer.linear.weight,
                   layer.linear.bias)
    ah = ctx.aggregate(x, "mean", rows=rows)
    x_dst = x[rows] if rows is not None else x
    return (lin(x_dst, layer.linear1.weight, layer.linear1.bias)
            + lin(ah, layer.linear2.weight, layer.linear2.bias))


def run(case: Case, order: str, device, dtype) -> dict:
    from bnsgcn_amd.models.context import GraphContext
    assert order in ("layer", "agg_first")
    g, parts = P.fixture_parts(3)
    plan = st = None
    if case.where == "full":
        ctx = GraphContext.for_full_graph(
            torch.from_numpy(g.adj_in.indptr), torch.from_numpy(g.adj_in.indices),
            torch.from_numpy(g.in_deg), torch.from_numpy(g.out_deg), device)
        n, train_mask = ctx.n_rows, g.train_mask
    else:
        part = parts[case.rank]
        plan = P.make_plan(part, RATE, device)
        st = plan.set_epoch(EPOCH)
        ctx = GraphContext.for_partition(part, plan, device, need_eperm=False)
        n, train_mask = part.n_inner, part.train_mask
    rows = None
    if case.use_rows:
        rows = torch.from_numpy(np.flatnonzero(train_mask)).to(device)
        assert 0 < rows.numel() < n
        ctx.loss_rows = rows            # as RankState does
    if plan is not None:
        P.assert_halo_preconditions(plan, st, rows=rows)

    layer = make_layer(case).to(device=device, dtype=dtype)
    fin, fout = case.fin, case.fout
    pad = (fout + 3) // 4 * 4
    gen = torch.Generator().manual_seed(1000 * fin + 10 * fout + case.rank)
    x = torch.randn(n, fin, generator=gen)
    n_out = n if rows is None else rows.numel()
    gout = torch.randn(n_out, fout, generator=gen)
    xd = x.to(device=device, dtype=dtype).requires_grad_(True)

    fills = []
    if plan is not None:
        H = torch.randn(sum(st.recv_counts), fin, generator=gen).double()
        B = torch.randn(sum(st.send_counts), pad, generator=gen).double()
        W = dict(layer.named_parameters())[agg_weight_name(case)]
        W = W.detach().double().cpu()
        Wp = torch.nn.functional.pad(W, (0, 0, 0, pad - fout))
        fills = [H, B @ Wp] if order == "agg_first" else [H @ Wp.t(), B]

    widths = []
    orig = ctx.aggregate

    def spy(x_, mode, rows=None):
        widths.append(int(x_.shape[1]))
        return orig(x_, mode, rows=rows)
    ctx.aggregate = spy

    stub = LinearStub(fills)
    with P.installed(stub):
        if order == "layer":
            out = layer(ctx, xd, rows=rows)
        else:
            out = _agg_first(layer, case, ctx, xd, rows)
        out.backward(gout.to(device=device, dtype=dtype))
        P.sync(device)
    assert len(stub.log) == len(fills) and len(widths) == 1

    res = {"out": out.detach().cpu(), "d x": xd.grad.cpu(),
           "agg width": widths[0]}
    for name, prm in layer.named_parameters():
        assert prm.grad is not None, name
        res["grad " + name] = prm.grad.detach().cpu()
    if plan is not None:
        fwd, bwd = (t.double() for t in stub.log)
        key = "grad " + agg_weight_name(case)
        dW = res.pop(key).double()
        if order == "layer":
            assert fwd.shape[1] == bwd.shape[1] == pad
            res[key + " + halo term"] = dW + bwd[:, :fout].t() @ H
            res["send fwd (projected)"] = fwd[:, :fout]
            res["send bwd (raw width)"] = bwd[:, :fout] @ W
        else:
            assert fwd.shape[1] == bwd.shape[1] == fin
            res[key + " + halo term"] = dW + B[:, :fout].t() @ fwd
            res["send fwd (projected)"] = fwd @ W.t()
            res["send bwd (raw width)"] = bwd
    return res
