"""One boundary-selection segment of n rows at rate p, timed alone: the
one-workgroup-per-segment HIP selection (ops/hip/bns_select.hip) against
the sort path it replaces (Philox keys, stable argsort, slice, sort), same
process, alternating. Shows what the single-workgroup form costs as a
segment grows; the results are compared once per size.

  python tools/select_micro.py --sizes 20000 200000 2000000

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
                   default=[20_000, 200_000, 2_000_000, 8_000_000])
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
        sel = bns_select.PlanSelect([(n, s, 0, 1, bns_select.KIND_HALO, 0)],
                                    seed, dev)

        def hip(epoch):
            return sel(epoch)[1]

        def sort(epoch):
            keys = ext.philox_keys(n, seed, epoch, 0, 1)
            return torch.sort(torch.argsort(keys, stable=True)[:s])[0]

        variants = (("sort", sort), ("hip", hip))
        assert torch.equal(hip(1), sort(1)), n
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
        print(f"n {n} s {s}: " + "  ".join(
            f"{name} gpu min-max {min(v):.3f}-{max(v):.3f} ms/call"
            for name, v in res.items()), flush=True)


if __name__ == "__main__":
    main()
