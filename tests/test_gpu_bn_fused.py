"""GPU (MI355X) checks of the fused SyncBatchNorm + ReLU + dropout kernels
(ops/hip/bn_fused.hip) and of their wiring into the models.

Reference: the module's formulas (models/sync_bn.py; var = E[x^2] - mean^2,
clamped at 0 under the root) in float64 on the CPU, dropout mask from
dense_path_checks.keep_mask on each part's flat indices, ReLU mask from the
float64 pre-activation. Yardstick: the same composition in fp32 on the CPU;
dense_path_checks.assert_measured (oracle M) allows the GPU 8x its error,
floored at 1e-5. x = 3 + randn, so the variance cancels; weight, bias, dy ~
N(0, 1); dy is zeroed where fp32 cannot be trusted with the ReLU sign,
|pre| < 1e-4 * (|xhat * w| + |b|) in float64 (at most 1e-3 of the elements).

Run on the GPU box: python -m pytest tests/test_gpu_bn_fused.py -m gpu -x -q
"""
import numpy as np
import pytest
import torch

import dense_path_checks as D
import ln_fused_checks as L
from kernel_path_checks import cu, dbl, gen

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

BN_EPS, MOM, SEED = 1e-5, 0.1, 2**40 + 4321
# the row-slab grid is clamped at 2048 blocks; at F = 8 a block steps over
# 128 sub-rows x 4 unrolled loads, so this n needs more than one step each
N_CLAMP = 2048 * 512 + 300


def inputs(n, F, act, seed):
    """(x, w, b, running_mean, running_var, dy) in fp32, dy zeroed at the
    sign-unsafe elements."""
    g = gen(seed)
    x = 3 + torch.randn(n, F, generator=g)
    w, b = torch.randn(F, generator=g), torch.randn(F, generator=g)
    rm, rv = torch.randn(F, generator=g), torch.rand(F, generator=g) + 0.5
    dy = torch.randn(n, F, generator=g)
    if act:
        r = reference(x, w, b, rm, rv, dy, 0, 1.0, (n,), torch.float64)
        xw = r["xhat"] * dbl(w)
        unsafe = r["pre"].abs() < 1e-4 * (xw.abs() + dbl(b).abs())
        print(f"n={n} F={F}: {int(unsafe.sum())} sign-unsafe elements")
        assert int(unsafe.sum()) <= 1e-3 * unsafe.numel()
        dy[unsafe] = 0.0
    return x, w, b, rm, rv, dy


def reference(x, w, b, rm, rv, dy, act, keep, part_rows, dtype, relu=None):
    """The module's training math, then relu and dropout, and its backward,
    in `dtype` on the CPU. part_rows: rows of each rank's part (every part
    numbers its dropout mask from 0). relu: a given ReLU mask."""
    x, w, b, rm, rv, dy = (t.to(dtype) for t in (x, w, b, rm, rv, dy))
    n, F = x.shape
    nt = max(n, 1)
    sx, sx2 = x.sum(0), (x * x).sum(0)
    mean = sx / nt
    var = (sx2 - mean * sx) / nt
    std = torch.sqrt(var.clamp_min(0.0) + BN_EPS)
    xhat = (x - mean) / std
    pre = xhat * w + b
    if relu is None:
        relu = pre > 0 if act else torch.ones_like(pre, dtype=torch.bool)
    drop = torch.from_numpy(np.concatenate(
        [D.keep_mask(np.arange(r * F), keep, SEED) for r in part_rows])
        .reshape(n, F))
    m = (relu & drop).to(dtype) * float(D.inv_keep32(keep))
    g = dy * m
    dbias, dweight = g.sum(0), (g * xhat).sum(0)
    return {"y": pre * m, "mean": mean, "rstd": 1 / std,
            "running_mean": rm * (1 - MOM) + mean * MOM,
            "running_var": rv * (1 - MOM) + var * MOM,
            "dx": w / std * (g - dbias / nt - xhat * (dweight / nt)),
            "dweight": dweight, "dbias": dbias,
            "xhat": xhat, "pre": pre, "relu": relu, "drop": drop}


def run_gpu(x, w, b, rm, rv, dy, act, keep, part_rows):
    """The five raw ops over the row parts of one batch, the [2F + 1]
    vectors added between them as the all-reduce would."""
    e = D._ext()
    F = x.shape[1]
    xs = [cu(t.contiguous()) for t in x.split(list(part_rows))]
    dys = [cu(t.contiguous()) for t in dy.split(list(part_rows))]
    wg, bg, rmg, rvg = cu(w), cu(b), cu(rm.clone()), cu(rv.clone())
    stats = sum(e.bn_colsums_fwd(t) for t in xs)
    assert float(stats[-1]) == x.shape[0]
    mean, rstd = e.bn_finalize(stats, rmg, rvg, MOM, BN_EPS)
    tail = (int(act), keep, SEED)
    ys = [e.bn_act_drop_fwd(t, mean, rstd, wg, bg, *tail) for t in xs]
    reds = [e.bn_colsums_bwd(t, d, mean, rstd, wg, bg, stats[-1:], *tail)
            for t, d in zip(xs, dys)]
    red = reds[0].clone()
    for r in reds[1:]:
        assert float(r[-1]) == x.shape[0]
        red[:2 * F] += r[:2 * F]
    dxs = [e.bn_act_drop_bwd_dx(t, d, mean, rstd, wg, bg, red, *tail)
           for t, d in zip(xs, dys)]
    return {"y": torch.cat(ys), "mean": mean, "rstd": rstd,
            "running_mean": rmg, "running_var": rvg, "dx": torch.cat(dxs),
            "dweight": red[F:2 * F], "dbias": red[:F]}


def check(n, F, act, keep, part_rows):
    args = inputs(n, F, act, 13000 + 7 * (n % 1000) + F + act)
    r64 = reference(*args, act, keep, part_rows, torch.float64)
    r32 = reference(*args, act, keep, part_rows, torch.float32,
                    relu=r64["relu"])
    got = run_gpu(*args, act, keep, part_rows)
    tag = f"n={n} F={F} act={act} keep={keep} parts={len(part_rows)}"
    for k, v in got.items():
        D.assert_measured(v, r64[k], r32[k], f"{tag} {k}")
    if not act and keep < 1.0 and n:
        assert torch.equal(got["y"].cpu() == 0, ~r64["drop"]), \
            f"{tag}: zeros of y are not the dropped elements"
    again = run_gpu(*args, act, keep, part_rows)
    for k, v in got.items():
        assert torch.equal(v, again[k]), f"{tag}: {k} differs between calls"


# scalar form; sub-wave row packing; exactly one column chunk; a ragged
# float4 chunk; several column chunks; the empty rank
SHAPES = [(5, 44), (700, 24), (1030, 256), (1030, 130), (3000, 516), (0, 24)]


@needs_gpu
@pytest.mark.parametrize("keep", [1.0, 0.5])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("n,F", SHAPES)
def test_raw_ops_against_float64(n, F, act, keep):
    check(n, F, act, keep, (n,))


@needs_gpu
def test_raw_ops_beyond_row_block_clamp():
    assert -(-N_CLAMP // (128 * 4)) > D._ext().BN_MAX_BLOCKS
    check(N_CLAMP, 8, 1, 0.5, (N_CLAMP,))


@needs_gpu
def test_split_batch_matches_whole_batch():
    """Two ranks' parts of one batch, cut at row 517, their partial
    vectors added: the multi-rank contract without a process group."""
    check(1030, 130, 1, 0.5, (517, 513))


# --------------------------------------------------------------- wiring

def host_dropout(x, p, training):
    """ops.functional.dropout for the CPU runs: the seed drawn as there,
    the mask the kernels' own."""
    if not training or p <= 0.0:
        return x
    seed = int(torch.randint(0, 2**62, (1,)).item())
    m = D.keep_mask(np.arange(x.numel()), 1.0 - p, seed)
    return x * torch.from_numpy(m.reshape(tuple(x.shape))).to(x.dtype) \
        * float(D.inv_keep32(1.0 - p))


def run_step(model_name, dev, dtype, fused):
    """One training step of a 3-layer norm='batch' model on `tiny`, set up
    as __graft_entry__.smoke() does. GAT's own feature and attention
    dropouts have no host form, so it runs with p = 0: BN + ReLU fused
    without dropout. Returns ({loss, gradients, buffers}, call counts)."""
    from bnsgcn_amd.graph import load_data, partition_graph
    from bnsgcn_amd.models.models import create_model
    from bnsgcn_amd.ops import functional as BF
    from bnsgcn_amd.runtime.config import create_parser
    from bnsgcn_amd.runtime.trainer import RankState, forward_train_logits
    args = create_parser().parse_args([])
    args.dataset, args.model, args.norm = "tiny", model_name, "batch"
    args.n_layers, args.n_hidden, args.n_partitions = 3, 36, 1
    args.sampling_rate, args.use_pp = 0.1, True
    args.dropout = 0.0 if model_name == "gat" else 0.5
    torch.manual_seed(0)
    g = load_data("tiny", seed=0)
    parts, meta = partition_graph(g, 1, method="metis")
    parts[0].meta = meta
    state = RankState(parts[0], args, dev)
    state.plan.set_epoch(0)
    model = create_model(args, n_feat=g.n_feat, n_class=g.n_class,
                         train_size=g.n_train).to(dev)
    state.precompute()
    if dtype is torch.float64:
        model.double()
        state.feat = state.feat.double()
        if getattr(state, "halo_feat0", None) is not None:
            state.halo_feat0 = state.halo_feat0.double()
    model.train()
    old = BF._BN_FUSE, BF.dropout, BF.get_ext
    BF._BN_FUSE = fused
    calls = {}
    if dev == "cpu":
        BF.dropout = host_dropout
    else:
        proxy = L.CountingExt(D._ext(), record=False)
        BF.get_ext, calls = (lambda: proxy), proxy.calls
    try:
        torch.manual_seed(17)
        logits = forward_train_logits(model, state)
        loss = torch.nn.functional.cross_entropy(
            logits, state.label[state.train_mask].long(), reduction="sum")
        loss.backward()
    finally:
        BF._BN_FUSE, BF.dropout, BF.get_ext = old
    out = {"loss": loss.detach().reshape(1)}
    out.update({k: p.grad.detach() for k, p in model.named_parameters()})
    out.update({k: v.detach() for k, v in model.named_buffers()})
    return {k: v.cpu() for k, v in out.items()}, calls


@needs_gpu
@pytest.mark.parametrize("model_name", ["gcn", "graphsage", "gat"])
def test_model_wiring(model_name):
    r64, _ = run_step(model_name, "cpu", torch.float64, True)
    r32, _ = run_step(model_name, "cpu", torch.float32, True)
    for fused in (True, False):
        got, calls = run_step(model_name, "cuda:0", torch.float32, fused)
        for op in ("bn_colsums_fwd", "bn_finalize", "bn_act_drop_fwd",
                   "bn_colsums_bwd", "bn_act_drop_bwd_dx"):
            assert calls.get(op, 0) == (2 if fused else 0), (op, calls)
        assert set(got) == set(r64)
        for k, v in got.items():
            tag = f"{model_name} fused={fused} {k}"
            if k.startswith("layers.") and k.endswith("bias") \
                    and int(k.split(".")[1]) < 2:
                # a bias in front of a batch norm: the gradient is 0 but
                # for rounding, so there is no scale to measure against
                assert float(r64[k].abs().max()) < 1e-9, tag
                tol = max(8 * float(r32[k].abs().max()), 1e-5)
                print(f"{tag}: |g| {float(v.abs().max()):.3g}, tol {tol:.3g}")
                assert float(v.abs().max()) <= tol, tag
            else:
                D.assert_measured(v, r64[k], r32[k], tag)
