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

  python tools/spmm_micro.py --graph reddit --grouped \
      --group-r 4,8,16 --gseg 512,1024,4096 [--permute]

--grouped compares, per CSR (forward and transposed) and width, the per-row
kernel (median and max - min spread of --repeats timings) with the
row-group kernel for every (R, gseg): entries/edges, build time, format
size and kernel time. --permute relabels the nodes with a random
permutation first, which removes the id locality (the graph for finding
the keep threshold GROUP_TAU).

  python tools/spmm_micro.py --graph reddit --feats 44,128,256 \
      --src-dtype fp32,bf16 [--grouped --group-r 4 --gseg 1024]

--src-dtype times each listed source type on the same values: bf16 is the
copy round_bf16_raw makes for --agg-dtype bf16 (the cast is not in the
timed window). Every line then carries TB/s of requested rows: row reads
(edges, or entries for the grouped kernel) x F x bytes per element of the
source actually read, over the time of a call.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bnsgcn_amd.graph import CSR
from bnsgcn_amd.ops.functional import round_bf16_raw, spmm_sum_raw

SRC_BYTES = {"fp32": 4, "bf16": 2}


def source_of(x, src_dtype):
    """x itself, or its bf16 copy; F % 4 != 0 has no bf16 kernel (the copy
    is upcast again inside spmm_sum_raw), which the byte count follows."""
    if src_dtype == "bf16":
        xb = round_bf16_raw(x)
        return xb, (2 if x.shape[1] % 4 == 0 else 4)
    return x, 4


def _relabel(src, dst, n, permute):
    if not permute:
        return src, dst
    p = np.random.default_rng(1).permutation(n)
    return p[src], p[dst]


def toy_csr(permute=False):
    rng = np.random.default_rng(0)
    n, e = 200_000, 20_000_000
    # power-law-ish columns with locality
    src = (rng.random(e) ** 4 * n).astype(np.int64)
    dst = np.sort(rng.integers(0, n, e))
    src, dst = _relabel(src, dst, n, permute)
    return CSR.from_edges(src, dst, n, n), None


def reddit_csr(permute=False):
    """(in-edge CSR, train-row ids) of the Reddit-shaped synthetic graph."""
    from bnsgcn_amd.graph.csr import add_self_loops
    from bnsgcn_amd.graph.synthetic import DATASETS, _draw_edges
    spec = DATASETS["reddit"]
    rng = np.random.default_rng(0)
    src, dst = _draw_edges(spec, spec.n_nodes, spec.n_edges, rng)
    src, dst = add_self_loops(src, dst, spec.n_nodes)
    src, dst = _relabel(src, dst, spec.n_nodes, permute)
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


def grouped_table(label, ip, ix, n_src, F, a, src_dtype="fp32"):
    """Per-row kernel against the row-group kernel on one CSR."""
    from bnsgcn_amd.ops.csr_torch import build_rowgroups
    e = ix.numel()
    x32 = torch.randn(n_src, F, device="cuda")
    x, nbytes = source_of(x32, src_dtype)
    base = [time_call(lambda: spmm_sum_raw(ip, ix, x), a.iters)
            for _ in range(a.repeats)]
    med, spread = float(np.median(base)), max(base) - min(base)
    print(f"{label} F={F} src={src_dtype} {e} edges: per-row {med*1e3:.3f} ms "
          f"(spread {spread*1e3:.3f} over {a.repeats} x {a.iters}), "
          f"{e * F * nbytes / med / 1e12:.2f} TB/s requested", flush=True)
    for R in (int(r) for r in a.group_r.split(",")):
        for gseg in (int(g) for g in a.gseg.split(",")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rg = build_rowgroups(ip, ix, n_src, R=R, gseg=gseg)
            torch.cuda.synchronize()
            t_build = time.perf_counter() - t0
            ipg = ip.clone()
            ipg._bns_rowgroups = rg
            ts = [time_call(lambda: spmm_sum_raw(ipg, ix, x), a.iters)
                  for _ in range(a.repeats)]
            ref = spmm_sum_raw(ip, ix, x)
            got = spmm_sum_raw(ipg, ix, x)
            err = float((got - ref).abs().max() / ref.abs().max())
            mb = (rg.ecol.numel() * (4 + R)
                  + sum(t.numel() * t.element_size() for t in rg.sched)) / 1e6
            print(f"  R={R} gseg={gseg}: entries/edges {rg.ratio:.3f}, "
                  f"{rg.sched[0].numel()} items, "
                  f"{int((rg.sched[0] < 0).sum())} of split groups, "
                  f"build {t_build*1e3:.0f} ms, {mb:.0f} MB, grouped "
                  f"{np.median(ts)*1e3:.3f} ms (spread "
                  f"{(max(ts)-min(ts))*1e3:.3f}), x{med/np.median(ts):.2f}, "
                  f"{rg.ecol.numel() * F * nbytes / np.median(ts) / 1e12:.2f} "
                  f"TB/s requested, max|diff|/max|ref| {err:.1e}", flush=True)
            del rg, ipg, ref, got


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--graph", choices=["toy", "reddit"], default="toy")
    p.add_argument("--feats", default="256",
                   help="comma-separated feature widths")
    p.add_argument("--rows", default="full",
                   help="comma-separated subset of full,train")
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--grouped", action="store_true",
                   help="per-row against row-group kernel (module docstring)")
    p.add_argument("--group-r", default="4,8,16")
    p.add_argument("--gseg", default="512,1024,4096")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--src-dtype", default="fp32",
                   help="comma-separated subset of fp32,bf16: element type "
                        "of the gathered source rows")
    p.add_argument("--permute", action="store_true",
                   help="relabel nodes randomly (no id locality)")
    a = p.parse_args()
    src_dtypes = a.src_dtype.split(",")
    assert all(d in SRC_BYTES for d in src_dtypes), a.src_dtype
    assert torch.cuda.is_available()
    c, train = (toy_csr if a.graph == "toy" else reddit_csr)(a.permute)
    for which in a.rows.split(","):
        assert which == "full" or train is not None, "toy graph has no rows"
        csrs = device_csrs(c, train, which)
        if a.graph == "toy" and not a.grouped:
            csrs = csrs[:1]
        for label, ip, ix, n_src in csrs:
            e = ix.numel()
            for F in (int(f) for f in a.feats.split(",")):
                if a.grouped:
                    for sd in src_dtypes:
                        grouped_table(label, ip, ix, n_src, F, a, sd)
                    continue
                x32 = torch.randn(n_src, F, device="cuda")
                for sd in src_dtypes:
                    x, nbytes = source_of(x32, sd)
                    ts = [time_call(lambda: spmm_sum_raw(ip, ix, x), a.iters)
                          for _ in range(a.repeats)]
                    dt = float(np.median(ts))
                    print(f"spmm {label} {e} edges F={F} src={sd}: "
                          f"{dt*1e3:.3f} ms (spread "
                          f"{(max(ts)-min(ts))*1e3:.3f} over {a.repeats} x "
                          f"{a.iters}), {e * F * nbytes / dt / 1e12:.2f} TB/s "
                          f"requested", flush=True)
                    del x
                del x32


if __name__ == "__main__":
    main()
