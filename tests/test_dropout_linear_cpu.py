"""CPU: ops.functional.dropout_linear, and the dropout draws of the models.

On CPU tensors dropout_linear is the unfused composition, so under one
torch seed it equals torch's linear(dropout(x)) bit for bit. At model
level a tiny use_pp GraphSAGE / GCN (with and without an nn.Linear tail)
must consume exactly one dropout draw per layer, in order, and produce
the same loss and gradients as the formula written out here:
`layer(dropout(h))` with a separate dropout in front of every layer and
one plain linear as the use_pp layer 0. That holds whether or not a model
routes a layer through dropout_linear.
"""
import pytest
import torch
import torch.nn.functional as TF

import partition_path_checks as P
from bnsgcn_amd.models.context import GraphContext
from bnsgcn_amd.models.models import GCN, GraphSAGE
from bnsgcn_amd.ops import functional as BF


def test_dropout_linear_cpu_equals_torch_composition():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(37, 20, generator=g)
    w = torch.randn(9, 20, generator=g, requires_grad=True)
    b = torch.randn(9, generator=g, requires_grad=True)
    torch.manual_seed(11)
    y = BF.dropout_linear(x, w, b, 0.5, True)
    y.sum().backward()
    gw, gb = w.grad.clone(), b.grad.clone()
    w.grad = b.grad = None
    torch.manual_seed(11)
    want = TF.linear(TF.dropout(x, 0.5, True), w, b)
    want.sum().backward()
    assert torch.equal(y, want)
    assert torch.equal(gw, w.grad) and torch.equal(gb, b.grad)
    # eval / p = 0: a plain linear, no randomness consumed
    state = torch.random.get_rng_state()
    assert torch.equal(BF.dropout_linear(x, w, b, 0.5, False),
                       TF.linear(x, w, b))
    assert torch.equal(BF.dropout_linear(x, w, b, 0.0, True),
                       TF.linear(x, w, b))
    assert torch.equal(torch.random.get_rng_state(), state)


def _ctx():
    g, _ = P.fixture_parts(3)
    return GraphContext.for_full_graph(
        torch.from_numpy(g.adj_in.indptr), torch.from_numpy(g.adj_in.indices),
        torch.from_numpy(g.in_deg), torch.from_numpy(g.out_deg), "cpu")


def _earlier_forward(model, ctx, feat):
    """The forward as it was before dropout_linear: a separate dropout in
    front of every layer; the use_pp layer 0 is one plain linear."""
    h = feat
    for i, lay in enumerate(model.layers):
        h = model.dropout(h)
        if isinstance(lay, torch.nn.Linear):
            h = lay(h)
        elif lay.use_pp:
            h = BF.linear(h, lay.linear.weight, lay.linear.bias)
        else:
            h = lay(ctx, h)
        h = model._post(i, h)
    return h


@pytest.mark.parametrize("n_linear", [0, 1])
@pytest.mark.parametrize("cls", [GraphSAGE, GCN])
def test_pp_model_same_draws_and_loss_as_separate_dropout(cls, n_linear,
                                                          monkeypatch):
    ctx = _ctx()
    fin = 6
    torch.manual_seed(3)
    model = cls([fin, 12, 12, 5], TF.relu, use_pp=True, dropout=0.5,
                norm="layer", n_linear=n_linear).train()
    width = 2 * fin if cls is GraphSAGE else fin
    feat = torch.randn(ctx.n_rows, width)
    label = torch.randint(0, 5, (ctx.n_rows,))

    draws = []
    real = TF.dropout
    monkeypatch.setattr(TF, "dropout", lambda x, p=0.5, training=True,
                        inplace=False: (draws.append(tuple(x.shape)),
                                        real(x, p, training, inplace))[1])

    def run(fwd):
        draws.clear()
        model.zero_grad()
        torch.manual_seed(17)
        loss = TF.cross_entropy(fwd(), label, reduction="sum")
        loss.backward()
        grads = [p.grad.clone() for p in model.parameters()]
        return loss.detach(), grads, list(draws), torch.random.get_rng_state()

    new = run(lambda: model(ctx, feat))
    old = run(lambda: _earlier_forward(model, ctx, feat))
    assert len(new[2]) == model.n_layers == 3
    assert new[2] == old[2], "dropout draws differ in number, order or shape"
    assert torch.equal(new[3], old[3]), "RNG state differs after the forward"
    assert torch.equal(new[0], old[0]), (new[0], old[0])
    for a, b in zip(new[1], old[1]):
        assert torch.equal(a, b)
