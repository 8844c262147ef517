"""A/B the two hand-written MFMA GEMMs against rocBLAS (torch) on the
bench shapes, per layout, plus the dropout-fused forward and dW against
their unfused forms.

Run on a GPU box from the repository root:

    PYTHONPATH=. python tools/gemm_micro.py [--reps 3] [--iters 10]

Every figure is the median of `reps` repeats of `iters` back-to-back calls,
with the (max - min) spread of the repeats beside it: a kernel only counts
as faster than the incumbent when the gap exceeds the incumbent's spread.
On a build without the tiled kernel only the old kernel and rocBLAS are
timed.
"""
import argparse
import statistics
import time

import torch

from bnsgcn_amd.ops._ext import get_ext

ext = get_ext()
dev = "cuda:0"
HAS_TILED = hasattr(ext, "gemm_nt_bias_drop")
OLD, TILED = 1, 2


def t(fn, iters, reps):
    for _ in range(3):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e3)
    return statistics.median(out), max(out) - min(out)


def bench_shape(M, K, N, iters, reps):
    x = torch.randn(M, K, device=dev)
    w = torch.randn(N, K, device=dev)       # torch Linear layout [out, in]
    b = torch.randn(N, device=dev)
    g = torch.randn(M, N, device=dev)

    r = {}
    if HAS_TILED:
        r["nt old"] = lambda: ext.gemm_nt_bias(x, w, b, OLD)
        r["nt tiled"] = lambda: ext.gemm_nt_bias(x, w, b, TILED)
    else:
        r["nt old"] = lambda: ext.gemm_nt_bias(x, w, b)
    r["nt rocblas"] = lambda: torch.nn.functional.linear(x, w, b)
    if HAS_TILED:
        r["nn old (dx)"] = lambda: ext.gemm_nn(g, w, OLD)
        r["nn tiled (dx)"] = lambda: ext.gemm_nn(g, w, TILED)
    else:
        r["nn old (dx)"] = lambda: ext.gemm_nn(g, w)
    r["nn rocblas (dx)"] = lambda: torch.mm(g, w)
    if HAS_TILED:
        r["tn old (dW)"] = lambda: ext.gemm_tn(g, x, OLD)
        r["tn tiled (dW)"] = lambda: ext.gemm_tn(g, x, TILED)
    else:
        r["tn old (dW)"] = lambda: ext.gemm_tn(g, x)
    r["tn rocblas (dW)"] = lambda: torch.mm(g.t(), x)
    if HAS_TILED:
        seed = (1 << 40) + 12345
        r["nt fused drop"] = lambda: ext.gemm_nt_bias_drop(x, w, b, 0.5, seed)
        r["nt rocblas+drop"] = lambda: torch.nn.functional.linear(
            ext.dropout_apply(x, 0.5, seed), w, b)
        r["tn fused drop (dW)"] = lambda: ext.gemm_tn_drop(g, x, 0.5, seed)
    print(f"[M={M} K={K} N={N}]", flush=True)
    for k, fn in r.items():
        v, spread = t(fn, iters, reps)
        fl = 2 * M * K * N / (v * 1e-3) / 1e12
        print(f"  {k:20s} {v:7.3f} ms  +-{spread:6.3f}  {fl:7.1f} TF/s",
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    for shape in [(232965, 1204, 256), (232965, 256, 256), (232965, 512, 256),
                  (232965, 256, 41), (153893, 256, 44), (2449029, 128, 128),
                  (716847, 512, 100)]:
        bench_shape(*shape, a.iters, a.reps)
