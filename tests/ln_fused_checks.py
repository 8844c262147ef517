"""Check functions for tests/test_gpu_ln_fused.py: the fused LayerNorm +
ReLU + dropout kernels (ext.ln_act_drop_fwd / ln_act_drop_bwd) and their
wiring into the GCN / GraphSAGE models.

Oracles.

* Equality. y, mean, rstd and dx must `torch.equal` the unfused
  composition of the existing bindings, dropout_apply(ln_fwd(x)[0]) and
  ln_bwd(x, dropout_apply(dy)): the fused kernels share the row arithmetic
  with them, so not one bit may move. Those bindings are pinned against
  float64 and the host dropout mask by tests/test_gpu_dense_paths.py.
* Column sums: the any-order summation bound of dense_path_checks
  (kernel_path_checks.assert_sum_bound) against float64 on the same
  inputs. dgamma and dbeta use check_ln_weight_grads' bounds,
  (n + 8) * EPS * sum|dm| and (n + 16) * EPS * sum|dm| * (|xhat| + 1), with
  dm = the dropped-out, ReLU-masked dy. colsum(dx) sums the kernel's own
  fp32 dx, so its float64 reference is the float64 column sum of that dx
  (n terms). As there, dy is zeroed beforehand wherever the float64
  pre-activation is too close to 0 for fp32 to be trusted with its sign;
  a pre-activation that is EXACTLY 0 (gamma = beta = 0 in some columns)
  is not such an element: it must take the `<= 0` side and contribute
  nothing.
* Wiring: fused against unfused model run under one torch seed. Logits
  equal; each gradient within twice the summation bound of the sum that
  forms it, the absolute sums recorded from the unfused run's own kernel
  calls (both runs add the same terms, in different orders).
"""
from __future__ import annotations

import numpy as np
import torch

import dense_path_checks as D
from kernel_path_checks import EPS, assert_sum_bound, cu, dbl, gen

LN_EPS = D.LN_EPS
SEED = 2**40 + 12345


def ext():
    return D._ext()


def inputs(n, F, seed, zero_cols=()):
    """x as dense_path_checks.LnCase builds it (|mean| * rstd <= 1),
    gamma and beta ~ N(0, 1) (both signs), dy ~ N(0, 1); gamma = beta = 0
    in `zero_cols`."""
    g = gen(seed)
    z = torch.randn(n, F, generator=g, dtype=torch.float64)
    u = 2 * torch.rand(n, 1, generator=g, dtype=torch.float64) - 1
    sd = z.var(1, unbiased=False, keepdim=True).sqrt()
    x = (z - z.mean(1, keepdim=True) + 0.25 * sd * u).float()
    gamma = torch.randn(F, generator=g)
    beta = torch.randn(F, generator=g)
    for c in zero_cols:
        gamma[c] = 0.0
        beta[c] = 0.0
    dy = torch.randn(n, F, generator=g)
    return x, gamma, beta, dy


def check_equal_unfused(n, F, acts=(0, 1), keeps=(1.0, 0.9, 0.5)):
    e = ext()
    x, gamma, beta, dy = (cu(t) for t in inputs(n, F, 11000 + 7 * n + F))
    for act in acts:
        y0, mean0, rstd0 = e.ln_fwd(x, gamma, beta, LN_EPS, act)
        for keep in keeps:
            tag = f"n={n} F={F} act={act} keep={keep}"
            y, mean, rstd = e.ln_act_drop_fwd(x, gamma, beta, LN_EPS, act,
                                              keep, SEED)
            assert torch.equal(y, e.dropout_apply(y0, keep, SEED)), \
                f"{tag}: y differs from dropout_apply(ln_fwd)"
            assert torch.equal(mean, mean0), f"{tag}: mean"
            assert torch.equal(rstd, rstd0), f"{tag}: rstd"
            dx0 = e.ln_bwd(x, e.dropout_apply(dy, keep, SEED), gamma, beta,
                           mean0, rstd0, act)[0]
            dx = e.ln_act_drop_bwd(x, dy, gamma, beta, mean0, rstd0, act,
                                   keep, SEED)[0]
            assert torch.equal(dx, dx0), \
                f"{tag}: dx differs from ln_bwd(dropout_apply(dy))"
            if keep < 1.0 and n * F >= 64:
                assert bool((y == 0).any()) and bool((y != 0).any()), tag


def check_column_sums(n, F, act, keep):
    """dgamma, dbeta, colsum(dx) against float64 (module docstring), and
    two calls bit for bit equal."""
    e = ext()
    zero_cols = (0, F // 2, F - 1) if act else ()
    x, gamma, beta, dy = inputs(n, F, 12000 + 3 * n + F + act, zero_cols)
    x64, gm, bt = dbl(x), dbl(gamma), dbl(beta)
    mean = x64.mean(1)
    rstd = (x64.var(1, unbiased=False) + LN_EPS).rsqrt()
    xhat = (x64 - mean[:, None]) * rstd[:, None]
    pre = xhat * gm + bt
    if act:
        unsafe = pre.abs() < 64 * EPS * ((xhat * gm).abs() + bt.abs())
        assert int(unsafe.sum()) <= max(1, 1e-3 * pre.numel())
        dy[unsafe] = 0.0
        m = (pre > 0).double()
        assert int((pre[:, list(zero_cols)] == 0).sum()) == n * len(zero_cols)
        assert bool((dy[:, list(zero_cols)] != 0).any())
    else:
        m = torch.ones_like(pre)
    idx = np.arange(n * F, dtype=np.int64)
    keepm = torch.from_numpy(D.keep_mask(idx, keep, SEED).reshape(n, F))
    # the kernel's fp32 product dy * fl32(1 / keep), as dropout_want forms it
    dyd = torch.from_numpy(np.where(keepm.numpy(), dy.numpy() *
                                    D.inv_keep32(keep), np.float32(0))
                           .astype(np.float32))
    dm = dbl(dyd) * m
    tag = f"ln_act_drop_bwd n={n} F={F} act={act} keep={keep}"
    xg, gg, bg, dyg = cu(x), cu(gamma), cu(beta), cu(dy)
    _, mean32, rstd32 = e.ln_act_drop_fwd(xg, gg, bg, LN_EPS, act, keep, SEED)
    got = e.ln_act_drop_bwd(xg, dyg, gg, bg, mean32, rstd32, act, keep, SEED)
    dx, dgamma, dbeta, colsum = got
    assert_sum_bound(dbeta, dm.sum(0), dm.abs().sum(0), float(n),
                     tag + " dbeta")
    assert_sum_bound(dgamma, (dm * xhat).sum(0),
                     (dm.abs() * (xhat.abs() + 1)).sum(0), float(n) + 8.0,
                     tag + " dgamma")
    dx64 = dx.double().cpu()
    assert_sum_bound(colsum, dx64.sum(0), dx64.abs().sum(0), float(n),
                     tag + " colsum(dx)")
    if act:
        zc = list(zero_cols)
        assert not dgamma.cpu()[zc].any() and not dbeta.cpu()[zc].any(), \
            f"{tag}: a pre-activation of exactly 0 was let through"
    again = e.ln_act_drop_bwd(xg, dyg, gg, bg, mean32, rstd32, act, keep,
                              SEED)
    for name, a, b in zip(("dx", "dgamma", "dbeta", "colsum"), got, again):
        assert torch.equal(a, b), f"{tag}: {name} differs between two calls"


# --------------------------------------------------------------- wiring

class CountingExt:
    """Stands in for the extension module inside ops/functional.py: counts
    calls by name and, when `record`, keeps for the unfused run the
    absolute sums behind every column sum and dW (module docstring)."""

    def __init__(self, real, record):
        self._real, self._record = real, record
        self.calls = {}
        self.ln = []        # per ln_bwd call: dict of abs sums, n
        self.tn = []        # per gemm_tn call: (abs product, n)
        self.cs = []        # per syncbn_stats call: (abs column sums, n)

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapped(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            out = fn(*a, **k)
            if self._record and name == "ln_bwd":
                x, dyd, w, b, mean, rstd, act = a
                xh = (x.double() - mean.double()[:, None]) \
                    * rstd.double()[:, None]
                dm = dyd.double()   # unmasked: an upper bound of the sums
                self.ln.append({
                    "n": x.shape[0],
                    "dgamma": (dm.abs() * (xh.abs() + 1)).sum(0).cpu(),
                    "dbeta": dm.abs().sum(0).cpu(),
                    "colsum": out[0].double().abs().sum(0).cpu()})
            if self._record and name == "syncbn_stats":
                self.cs.append((a[0].double().abs().sum(0).cpu(),
                                a[0].shape[0]))
            if self._record and name == "gemm_tn":
                g, x = a[0], a[1]
                self.tn.append(((g.double().abs().t() @ x.double().abs())
                                .cpu(), g.shape[0]))
            return out
        return wrapped


def run_model(model_name, fused, n_hidden=132):
    """One forward + backward of a 3-layer use_pp model on `tiny`, as
    __graft_entry__.smoke() sets it up, under torch.manual_seed(0).
    Returns (logits, {param name: grad}, CountingExt)."""
    from bnsgcn_amd.graph import load_data, partition_graph
    from bnsgcn_amd.models.models import create_model
    from bnsgcn_amd.ops import functional as BF
    from bnsgcn_amd.runtime.config import create_parser
    from bnsgcn_amd.runtime.trainer import RankState, forward_train_logits

    args = create_parser().parse_args([])
    args.dataset, args.model = "tiny", model_name
    args.n_layers, args.n_hidden = 3, n_hidden
    args.sampling_rate, args.use_pp, args.n_partitions = 0.1, True, 1
    torch.manual_seed(0)
    g = load_data("tiny", seed=0)
    parts, meta = partition_graph(g, 1, method="metis")
    parts[0].meta = meta
    state = RankState(parts[0], args, "cuda:0")
    state.plan.set_epoch(0)
    model = create_model(args, n_feat=g.n_feat, n_class=g.n_class,
                         train_size=g.n_train).to("cuda:0")
    state.precompute()
    model.train()
    proxy = CountingExt(ext(), record=not fused)
    old = BF._LN_FUSE, BF.get_ext
    BF._LN_FUSE, BF.get_ext = fused, (lambda: proxy)
    try:
        torch.manual_seed(17)
        logits = forward_train_logits(model, state)
        loss = torch.nn.functional.cross_entropy(
            logits, state.label[state.train_mask].long(), reduction="sum")
        loss.backward()
        torch.cuda.synchronize()
    finally:
        BF._LN_FUSE, BF.get_ext = old
    grads = {k: (None if p.grad is None else p.grad.detach().cpu())
             for k, p in model.named_parameters()}
    return logits.detach().cpu(), grads, proxy


def grad_bound(name, shape, rec):
    """(abs sums, n_terms) of the sum that forms parameter `name`'s
    gradient, from the unfused run's records. LayerNorm i is the i-th
    from the END of rec.ln (backward order); a layer's deferred biases
    are column sums of that LayerNorm's dx; a weight is one gemm_tn —
    the elementwise largest of the recorded ones of its shape (the
    project-first weight is padded to a multiple of 4 rows); any other
    bias is one syncbn_stats column sum, matched by shape likewise."""
    parts = name.split(".")
    if parts[0] == "norm":
        r = rec.ln[len(rec.ln) - 1 - int(parts[1])]
        return r["dgamma" if parts[2] == "weight" else "dbeta"], r["n"] + 8
    if parts[-1] == "bias" and int(parts[1]) < len(rec.ln):
        r = rec.ln[len(rec.ln) - 1 - int(parts[1])]
        return r["colsum"], r["n"]
    if parts[-1] == "weight":
        pad = ((shape[0] + 3) // 4 * 4, shape[1])
        cands = [(a[:shape[0]], n) for a, n in rec.tn
                 if tuple(a.shape) in (tuple(shape), pad)]
        assert cands, name
        return (torch.stack([a for a, _ in cands]).amax(0),
                max(n for _, n in cands))
    cands = [(a, n) for a, n in rec.cs if tuple(a.shape) == tuple(shape)]
    assert cands, name
    return (torch.stack([a for a, _ in cands]).amax(0),
            max(n for _, n in cands))
