"""One boundary-selection segment of n rows at rate p, timed alone: the
one-workgroup-per-segment HIP selection (ops/hip/bns_select.hip), the
sliced form (ops/hip/bns_select_sliced.hip, one variant per --slice-rows
value) and the sort path they replace (Philox keys, stable argsort, slice,
sort), same process, alternating. Shows what each form costs as a segment
grows; the results are compared once per size.

  python tools/select_micro.py --sizes 20000 200000 2000000 \
      --slice-rows 2048 8192 32768

Per size and variant: GPU ms per call from device events around --calls
calls, min-max over --rounds rounds. Needs a GPU.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", type=int, nargs="+",
                   default=[20_000, 100_000, 200_000, 2_000_000, 8_000_000])
    p.add_argument("--slice-rows", type=int, nargs="+", default=None,
                   help="default: bns_select.SLICE_ROWS")
    p.add_argument("--rate", type=float, default=0.1)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--calls", type=int, default=20)
    a = p.parse_args()
    assert torch.cuda.is_available(), "select_micro measures on a GPU"
    from bnsgcn_amd.ops import bns_select
    from bnsgcn_amd.ops._ext import require_ext
    ext, dev, seed = require_ext(), "cuda:0", 0

    for n in a.sizes:
        s = int(a.rate * n)
        seg = [(n, s, 0, 1, bns_select.KIND_HALO, 0)]

        def sort(epoch):
            keys = ext.philox_keys(n, seed, epoch, 0, 1)
            return torch.sort(torch.argsort(keys, stable=True)[:s])[0]

        def variant(**kw):
            sel = bns_select.PlanSelect(seg, seed, dev, **kw)
            return lambda epoch: sel(epoch)[1]

        variants = [("sort", sort),
                    ("hip", variant(sliced_min_rows=2 ** 31))]
        for sr in a.slice_rows or [bns_select.SLICE_ROWS]:
            variants.append((f"sliced/{sr}",
                             variant(sliced_min_rows=0, slice_rows=sr)))
        want = sort(1)
        for name, fn in variants[1:]:
            assert torch.equal(fn(1), want), (n, name)
        res = {name: [] for name, _ in variants}
        for rnd in range(a.rounds):
            for name, fn in variants:
                fn(2)                                   # warm
                e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
                torch.cuda.synchronize()
                e0.record()
                for e in range(a.calls):
                    fn(100 * rnd + e)
                e1.record()
                torch.cuda.synchronize()
                res[name].append(e0.elapsed_time(e1) / a.calls)
        print(f"n {n} s {s}:", flush=True)
        for name, v in res.items():
            print(f"  {name:14s} gpu min-max {min(v):.3f}-{max(v):.3f} "
                  f"ms/call", flush=True)


if __name__ == "__main__":
    main()
