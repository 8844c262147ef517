"""Single-kernel SpMM microbenchmark (for rocprofv3 PMC counter runs —
the full bench crashed rocprofv3's counter collection in this image).

  python tools/spmm_micro.py                         # 20M-edge toy, F=256
  python tools/spmm_micro.py --graph reddit --feats 44,48,64,256 \
      --rows full,train

--graph reddit draws the Reddit-shaped edge set of graph/synthetic.py
(232,965 nodes, ~114.8M edges with self-loops; no features, no partition
reorder) and times, per feature width, the forward SpMM and the SpMM over
the transposed CSR (what the backward runs) — over all destination rows
and/or over the 66 % train rows only, as the final layer does. That is
the kernel-only before/after for the narrow-F path (F <= 64 takes
spmm_sum_narrow_kernel unless BNSGCN_SPMM_NARROW_MAX=0).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bnsgcn_amd.graph import CSR
from bnsgcn_amd.ops.functional import spmm_sum_raw


def toy_csr():
    rng = np.random.default_rng(0)
    n, e = 200_000, 20_000_000
    # power-law-ish columns with locality
    src = (rng.random(e) ** 4 * n).astype(np.int64)
    dst = np.sort(rng.integers(0, n, e))
    return CSR.from_edges(src, dst, n, n), None


def reddit_csr():
    """(in-edge CSR, train-row ids) of the Reddit-shaped synthetic graph."""
    from bnsgcn_amd.graph.csr import add_self_loops
    from bnsgcn_amd.graph.synthetic import DATASETS, _draw_edges
    spec = DATASETS["reddit"]
    rng = np.random.default_rng(0)
    src, dst = _draw_edges(spec, spec.n_nodes, spec.n_edges, rng)
    src, dst = add_self_loops(src, dst, spec.n_nodes)
    c = CSR.from_edges(src, dst, spec.n_nodes, spec.n_nodes)
    train = np.nonzero(rng.random(spec.n_nodes) < spec.train_frac)[0]
    return c, train


def time_call(fn, iters=5, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def device_csrs(c, train, which):
    """[(label, indptr, indices, n_src)] forward and transposed, on the
    device, for `which` in {"full", "train"}."""
    from bnsgcn_amd.ops.csr_torch import gather_rows_csr, transpose_csr
    ip = torch.from_numpy(c.indptr).cuda()
    ix = torch.from_numpy(c.indices).cuda()
    n = ip.numel() - 1
    if which == "train":
        ip, ix = gather_rows_csr(ip, ix, torch.from_numpy(train).cuda())
    tip, tix, _ = transpose_csr(ip, ix, n)
    return [(f"{which} fwd", ip, ix, n), (f"{which} bwd", tip, tix,
                                          ip.numel() - 1)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--graph", choices=["toy", "reddit"], default="toy")
    p.add_argument("--feats", default="256",
                   help="comma-separated feature widths")
    p.add_argument("--rows", default="full",
                   help="comma-separated subset of full,train")
    p.add_argument("--iters", type=int, default=5)
    a = p.parse_args()
    assert torch.cuda.is_available()
    c, train = toy_csr() if a.graph == "toy" else reddit_csr()
    for which in a.rows.split(","):
        assert which == "full" or train is not None, "toy graph has no rows"
        csrs = device_csrs(c, train, which)
        if a.graph == "toy":
            csrs = csrs[:1]
        for label, ip, ix, n_src in csrs:
            e = ix.numel()
            for F in (int(f) for f in a.feats.split(",")):
                x = torch.randn(n_src, F, device="cuda")
                dt = time_call(lambda: spmm_sum_raw(ip, ix, x), a.iters)
                gb = e * F * 4 / 1e9
                print(f"spmm {label} {e} edges F={F}: {dt*1e3:.3f} ms, "
                      f"{gb/dt:.2f} GB/s logical", flush=True)
                del x


if __name__ == "__main__":
    main()
