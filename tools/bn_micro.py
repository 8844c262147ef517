"""Forward + backward of SyncBatchNorm + ReLU + dropout on one GPU: the fused
kernels (ops/hip/bn_fused.hip) against the same call with the fuse switch
off (models/sync_bn._SyncBNFunc, then relu and dropout()), same process,
same inputs, alternating.

  python tools/bn_micro.py [--out profiles/bn_micro.txt]

Per shape: device-event time of --iters calls per round, --rounds rounds
per variant, min and max over the rounds. The fused path moves 3 + 5 = 8
passes of n * F * 4 bytes (docs/DESIGN.md §5b); "TB/s" is those bytes over
the fused time. The outputs and gradients of both variants are compared on
the timed inputs before timing. Needs a GPU.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(232965, 256), (232965, 128), (232965, 64)]


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--p", type=float, default=0.5)
    p.add_argument("--out", default=None)
    return p.parse_args()


def main():
    a = parse()
    assert torch.cuda.is_available(), "bn_micro measures on a GPU"
    from bnsgcn_amd.ops import functional as BF
    assert BF._BN_FUSE, "BNSGCN_BN_FUSE=0 is set"
    dev = "cuda:0"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; p = {a.p}, act = relu; "
        f"{a.rounds} rounds x {a.iters} calls per variant, alternating")
    for n, F in SHAPES:
        g = torch.Generator().manual_seed(n + F)
        x = (3 + torch.randn(n, F, generator=g)).to(dev).requires_grad_(True)
        dy = torch.randn(n, F, generator=g).to(dev)
        w = torch.randn(F, generator=g).to(dev).requires_grad_(True)
        b = torch.randn(F, generator=g).to(dev).requires_grad_(True)
        rm, rv = torch.zeros(F, device=dev), torch.ones(F, device=dev)

        def call(fused, seed=None):
            BF._BN_FUSE = fused
            if seed is not None:
                torch.manual_seed(seed)
            x.grad = w.grad = b.grad = None
            y = BF.sync_batch_norm_act_dropout(x, w, b, rm, rv, 0.1, 1e-5,
                                               True, a.p, True)
            y.backward(dy)
            return y.detach(), x.grad, w.grad, b.grad

        # same seed, same mask: the two variants must agree
        ref = call(False, seed=1)
        got = call(True, seed=1)
        diffs = []
        # x_hat is rounded differently in the two variants, so a few of the
        # n * F ReLU signs flip; each flip moves one dx element by a whole
        # term. Counted apart: elements off by more than 1e-4 of the peak.
        for name, r, t in zip(("y", "dx", "dw", "db"), ref, got):
            d = (r - t).abs() / r.abs().max()
            off = int((d > 1e-4).sum())
            diffs.append(f"{name} {float(d[d <= 1e-4].max()):.1e}"
                         + (f" ({off} of {d.numel()} off)" if off else ""))
        for fused in (False, True):                 # warm both
            for _ in range(3):
                call(fused)
        torch.cuda.synchronize()
        ms = {False: [], True: []}
        for _ in range(a.rounds):
            for fused in (False, True):
                e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
                e0.record()
                for _ in range(a.iters):
                    call(fused)
                e1.record()
                torch.cuda.synchronize()
                ms[fused].append(e0.elapsed_time(e1) / a.iters)
        BF._BN_FUSE = True
        u, f = ms[False], ms[True]
        tbs = 8 * n * F * 4 / (min(f) * 1e-3) / 1e12
        say(f"[{n}, {F}] unfused {min(u):.3f}-{max(u):.3f} ms  fused "
            f"{min(f):.3f}-{max(f):.3f} ms  ratio {min(u) / min(f):.2f}x  "
            f"fused {tbs:.2f} TB/s over 8 passes  max rel diff: "
            + ", ".join(diffs))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
