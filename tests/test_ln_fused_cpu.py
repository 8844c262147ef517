"""CPU: ops.functional.layer_norm_act_dropout off the fused path, and the
order in which the GCN / GraphSAGE models draw their dropout seeds and
defer their bias gradients when the fused path is on.

The kernels need a GPU (tests/test_gpu_ln_fused.py). What can be pinned
here is the routing around them: with a CPU tensor, in eval or with p = 0
the entry point is the existing composition; and a model that fuses
LayerNorm, ReLU and the next layer's dropout draws one seed per layer in
the order the unfused model draws them, and leaves the generator in the
same state.
"""
import pytest
import torch
import torch.nn.functional as TF

import partition_path_checks as P
from bnsgcn_amd.models.context import GraphContext
from bnsgcn_amd.models.models import GCN, GraphSAGE
from bnsgcn_amd.ops import functional as BF


def test_entry_point_is_the_composition_off_the_fused_path():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(19, 12, generator=g)
    w = torch.randn(12, generator=g)
    b = torch.randn(12, generator=g)
    for act in (False, True):
        want = BF.layer_norm(x, w, b, 1e-5, act)
        state = torch.random.get_rng_state()
        # eval and p = 0: no dropout, no randomness consumed
        assert torch.equal(BF.layer_norm_act_dropout(
            x, w, b, 1e-5, act, 0.5, False), want)
        assert torch.equal(BF.layer_norm_act_dropout(
            x, w, b, 1e-5, act, 0.0, True), want)
        assert torch.equal(torch.random.get_rng_state(), state)
        # a CPU tensor in training: dropout(layer_norm(x)) under one seed
        torch.manual_seed(5)
        got = BF.layer_norm_act_dropout(x, w, b, 1e-5, act, 0.5, True)
        torch.manual_seed(5)
        assert torch.equal(got, BF.dropout(want, 0.5, True))
    assert not BF.ln_fuse_active(x, 12, 0.5, True)
    with pytest.raises(RuntimeError):
        BF.layer_norm_act_dropout(x, w, b, 1e-5, True, 0.5, True,
                                  bias_grad_to=(b,))


def _ctx():
    g, _ = P.fixture_parts(3)
    return GraphContext.for_full_graph(
        torch.from_numpy(g.adj_in.indptr), torch.from_numpy(g.adj_in.indices),
        torch.from_numpy(g.in_deg), torch.from_numpy(g.out_deg), "cpu")


@pytest.mark.parametrize("n_linear", [0, 1])
@pytest.mark.parametrize("cls", [GraphSAGE, GCN])
def test_model_seed_draws_keep_their_order_when_fused(cls, n_linear,
                                                      monkeypatch):
    """The GPU ops are replaced by stand-ins that draw their seed exactly
    as the real ones do (one torch.randint each) and compute with torch:
    dropout() keeps (seed, shape); the fused op keeps (seed, shape) and
    the bias parameters it was handed. Fused and unfused forwards must
    log the same (seed, shape) sequence, leave the same generator state
    and give the same loss and gradients; the fused op must have been
    handed exactly the biases of the conv layer in front of it."""
    ctx = _ctx()
    fin = 6
    torch.manual_seed(3)
    model = cls([fin, 12, 12, 5], TF.relu, use_pp=True, dropout=0.5,
                norm="layer", n_linear=n_linear).train()
    width = 2 * fin if cls is GraphSAGE else fin
    feat = torch.randn(ctx.n_rows, width)
    label = torch.randint(0, 5, (ctx.n_rows,))
    log, handed = [], []

    def seeded_dropout(x, seed):
        g = torch.Generator().manual_seed(seed % (2**31))
        keep = (torch.rand(x.shape, generator=g) < 0.5).to(x.dtype)
        return x * keep * 2.0

    def fake_dropout(x, p, training):
        if not training or p <= 0.0:
            return x
        seed = int(torch.randint(0, 2**62, (1,)).item())
        log.append((seed, tuple(x.shape)))
        return seeded_dropout(x, seed)

    def fake_fused(x, weight, bias, eps=1e-5, act=False, p=0.0,
                   training=False, bias_grad_to=()):
        assert training and p > 0.0
        seed = int(torch.randint(0, 2**62, (1,)).item())
        log.append((seed, tuple(x.shape)))
        handed.append(list(bias_grad_to))
        # the linears got bias.detach(): give each deferred bias its
        # gradient colsum(dx) by adding 0 * x + (b - b.detach()) to x
        for b in bias_grad_to:
            x = x + (b - b.detach())
        return seeded_dropout(BF.layer_norm(x, weight, bias, eps, act), seed)

    monkeypatch.setattr(BF, "dropout", fake_dropout)
    monkeypatch.setattr(BF, "layer_norm_act_dropout", fake_fused)

    def run(fused):
        monkeypatch.setattr(BF, "ln_fuse_active",
                            lambda x, width, p, training:
                            fused and training and p > 0.0)
        log.clear()
        handed.clear()
        model.zero_grad()
        torch.manual_seed(17)
        loss = TF.cross_entropy(model(ctx, feat), label, reduction="sum")
        loss.backward()
        grads = {k: p.grad.clone() for k, p in model.named_parameters()}
        return (loss.detach(), grads, list(log), list(handed),
                torch.random.get_rng_state())

    unf = run(False)
    fus = run(True)
    assert len(unf[2]) == model.n_layers == 3 and not unf[3]
    assert fus[2] == unf[2], "seed draws differ in number, order or shape"
    assert torch.equal(fus[4], unf[4]), "RNG state differs after the forward"
    assert torch.equal(fus[0], unf[0]), (fus[0], unf[0])
    # layer 0 and layer 1 are followed by a LayerNorm; a conv layer hands
    # over all its GEMM biases, an nn.Linear tail layer keeps its own
    lay = model.layers
    want = [[lay[0].linear.bias]]
    if cls is GraphSAGE:
        want.append([lay[1].linear1.bias, lay[1].linear2.bias])
    else:
        want.append([lay[1].linear.bias])
    assert len(fus[3]) == 2
    for got, exp in zip(fus[3], want):
        assert len(got) == len(exp) and all(a is b for a, b in zip(got, exp))
    assert set(fus[1]) == set(unf[1])
    for k in unf[1]:
        torch.testing.assert_close(fus[1][k], unf[1][k], rtol=1e-5, atol=1e-6,
                                   msg=lambda m: f"{k}: {m}")
