"""Per-epoch plan build on one rank of a real multi-partition job, three
variants in the same process on the same inputs, alternating:

  torch    torch sampling and torch CSR surgery (csr_torch.PLAN_HIP and
           bns_select.SAMPLE_HIP off);
  hip      the device CSR build (ops/hip/plan_build.hip) with torch
           sampling: Philox keys, argsort, sort and index per peer and
           direction;
  hip+sel  the device CSR build with the one-launch device sampling
           (ops/hip/bns_select.hip) — the default path.

  python tools/plan_micro.py --store /tmp/plan_micro_store

The graph is partitioned on the CPU with the project's partitioner (reused
if the store exists), one rank is loaded and HaloPlan._build(epoch) plus
GraphContext._build_rows_halo(train rows) is timed over --builds
consecutive epochs per round. Reported per build:

  host ms   host clock from the first call to the return of the last one,
            no device synchronise added: what the launching thread loses,
            the read-backs that block it included;
  gpu ms    device events around the same calls;
  kernels / syncs   launches and blocking runtime calls of ONE build, from
            the profiler, in a run of their own.

Needs a GPU; the partitioning alone runs without one (--partition-only).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--dataset", default="reddit")
    p.add_argument("--data-scale", type=float, default=1.0)
    p.add_argument("--parts", type=int, default=8)
    p.add_argument("--rank", type=int, default=0)
    p.add_argument("--rate", type=float, default=0.1)
    p.add_argument("--partition-method", default="metis")
    p.add_argument("--store", default="plan_micro_store")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--builds", type=int, default=20)
    p.add_argument("--partition-only", action="store_true")
    return p.parse_args()


def count_calls(build, epoch):
    """(kernel launches, blocking runtime calls) of one build."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU,
                             ProfilerActivity.CUDA]) as prof:
        build(epoch)
        torch.cuda.synchronize()
    launches = syncs = 0
    for ev in prof.events():
        name = ev.name
        if "LaunchKernel" in name:
            launches += 1
        elif name in ("hipStreamSynchronize", "hipEventSynchronize",
                      "hipMemcpy", "hipMemcpyWithStream",
                      "hipMemcpyDtoH", "aten::_local_scalar_dense"):
            # a .item() / int() shows twice: the aten op and its copy
            syncs += 1
    return launches, syncs


def main():
    a = parse()
    from bnsgcn_amd.graph import load_partition
    from bnsgcn_amd.runtime.config import create_parser, graph_name_of
    from bnsgcn_amd.runtime.trainer import prepare_partitions
    args = create_parser().parse_args([])
    args.dataset, args.data_scale = a.dataset, a.data_scale
    args.n_partitions, args.partition_method = a.parts, a.partition_method
    args.partition_dir, args.skip_partition = a.store, True
    args.seed, args.eval = 0, False
    args.graph_name = graph_name_of(args)
    t0 = time.perf_counter()
    prepare_partitions(args)
    print(f"partition store ready in {time.perf_counter() - t0:.1f} s",
          flush=True)
    if a.partition_only:
        return
    assert torch.cuda.is_available(), "plan_micro measures on a GPU"

    from bnsgcn_amd.models.context import GraphContext
    from bnsgcn_amd.ops import bns_select, csr_torch
    from bnsgcn_amd.parallel.plan import HaloPlan
    assert csr_torch.PLAN_HIP, "extension not loaded or BNSGCN_PLAN_TORCH=1"
    assert bns_select.SAMPLE_HIP, "BNSGCN_SAMPLE_TORCH=1"
    dev = "cuda:0"
    part = load_partition(a.store, args.graph_name, a.rank)
    plan = HaloPlan(part, a.rate, seed=0, device=dev)
    ctx = GraphContext.for_partition(part, plan, dev, need_eperm=False)
    rows = torch.from_numpy(np.flatnonzero(part.train_mask)).to(dev)
    ctx.loss_rows = rows

    def build(epoch):
        st = plan._build(epoch)
        return st, ctx._build_rows_halo(rows, st)

    st, _ = build(0)
    print(f"rank {a.rank}/{a.parts} {a.dataset} x{a.data_scale}: n_inner "
          f"{part.n_inner}, n_halo {part.n_halo}, halo edges "
          f"{part.halo_indices.size}, rate {a.rate}: sampled rows "
          f"{st.hsel.numel()}, sampled edges {st.halo_bwd_indices.numel()}, "
          f"train rows {rows.numel()}", flush=True)

    variants = (("torch", (False, False)), ("hip", (True, False)),
                ("hip+sel", (True, True)))

    def switch(on):
        csr_torch.PLAN_HIP, bns_select.SAMPLE_HIP = on

    for _, on in variants:                      # warm every path
        switch(on)
        for e in range(3):
            build(e)
    torch.cuda.synchronize()
    res = {name: {"host": [], "gpu": []} for name, _ in variants}
    for rnd in range(a.rounds):
        for name, on in variants:
            switch(on)
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for e in range(a.builds):
                build(100 * rnd + e)
            host = (time.perf_counter() - t0) * 1e3 / a.builds
            e1.record()
            torch.cuda.synchronize()
            gpu = e0.elapsed_time(e1) / a.builds
            res[name]["host"].append(host)
            res[name]["gpu"].append(gpu)
            print(f"round {rnd} {name:7s} host {host:8.3f} ms/build  "
                  f"gpu {gpu:8.3f} ms/build", flush=True)
    for name, on in variants:
        switch(on)
        try:
            k, s = count_calls(build, 999)
            calls = f"kernels {k} syncs {s}"
        except Exception as exc:                # profiler unavailable
            calls = f"launch counts not measured ({type(exc).__name__})"
        h, g = res[name]["host"], res[name]["gpu"]
        print(f"{name:7s} host min-max {min(h):.3f}-{max(h):.3f} ms  "
              f"gpu min-max {min(g):.3f}-{max(g):.3f} ms  {calls}",
              flush=True)


if __name__ == "__main__":
    main()
