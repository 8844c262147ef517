"""GPU (MI355X): the device plan build (ops/hip/plan_build.hip) against the
torch code of ops/csr_torch.py on CPU copies of the same inputs. Every
output is an integer tensor; the comparison is dtype, shape and
torch.equal, no tolerance.

  python -m pytest tests/test_gpu_plan_build.py -m gpu -x -q
"""
import functools

import numpy as np
import pytest
import torch

import partition_path_checks as P
from partition_path_checks import DEV

from bnsgcn_amd.ops import csr_torch as C

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="no GPU")]

if torch.cuda.is_available():
    from bnsgcn_amd.ops._ext import require_ext
    T = require_ext().PLAN_SCAN_TILE      # new bindings: fails on the parent
else:
    T = 1024
N_COLS = 300
PLAN_TENSORS = ("pack_idx", "pack_scale", "hsel",
                "halo_fwd_indptr", "halo_fwd_indices",
                "halo_bwd_indptr", "halo_bwd_indices",
                "halo_eperm_t", "halo_out_norm_inv", "halo_in_deg")


def same(got, want, tag):
    assert len(got) == len(want), tag
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape, (
            tag, i, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g.cpu(), w), (tag, i)


@functools.lru_cache(maxsize=None)
def hand_csr():
    """Rows of degree 0, 1, 63, 64, 65, L-1, L, L+1, 2L+1 for L = 128 and
    L = 1024, columns ascending within a row (so parallel edges wherever
    the degree exceeds N_COLS, and in the 5-edge row), one row on columns
    = 1 mod 3 (all filtered by the every-third selection) and one on
    multiples of 3 (all kept)."""
    g = torch.Generator().manual_seed(3)
    rows = [torch.sort(torch.randint(0, N_COLS, (d,), generator=g))[0]
            for d in (0, 1, 63, 64, 65, 127, 128, 129, 257, 0, 1023, 1024,
                      1025, 2049)]
    rows += [torch.tensor([7, 7, 7, 9, 9]), torch.arange(1, N_COLS, 3),
             torch.arange(0, N_COLS, 3).repeat_interleave(2)]
    ip = torch.tensor([0] + [r.numel() for r in rows]).cumsum(0)
    return ip, torch.cat(rows).to(torch.int32)


@functools.lru_cache(maxsize=None)
def sized_csr(n):
    """n rows of degree 1 or 2 (so n segments too), ascending columns
    below 64."""
    deg = 1 + torch.arange(n) % 2
    ip = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)])
    r = torch.repeat_interleave(torch.arange(n), deg)
    ix = (r % 60 + torch.arange(r.numel()) - ip[r]).to(torch.int32)
    return ip, ix


def csr_of(name):
    return hand_csr() if name == "hand" else sized_csr(int(name))


def select(n, how):
    """Row or column ids below n; "single" is row 8 (degree 2L + 1)."""
    return {"empty": torch.zeros(0, dtype=torch.int64),
            "all": torch.arange(n), "third": torch.arange(0, n, 3),
            "single": torch.tensor([8]),
            "reversed": torch.arange(n).flip(0)}[how]


# row / segment counts around the scan tile T and above T * T (the scans
# run over count + 1 elements; T * T + 1 takes a third level)
SIZES = [str(n) for n in (0, T - 2, T - 1, T, T + 1, T * T + 1)]
HAND = [("hand", s) for s in ("empty", "all", "third", "single")]


@pytest.mark.parametrize("name,how", HAND + [("hand", "reversed")]
                         + [(n, "all") for n in SIZES])
def test_csr_gather_rows(name, how):
    ip, ix = csr_of(name)
    rows = select(ip.numel() - 1, how)
    got = C.csr_gather_rows(ip.to(DEV), ix.to(DEV), rows.to(DEV))
    same(got, C.gather_rows_csr(ip, ix, rows), (name, how))


@pytest.mark.parametrize("L", [128, None])
@pytest.mark.parametrize("name,how", HAND + [(n, "third") for n in SIZES])
def test_csr_filter_cols(name, how, L):
    """Oracle: transpose, gather the selected columns, transpose back —
    the sorted route the filter replaces; `kept` against the composed edge
    permutations of the two transposes."""
    ip, ix = csr_of(name)
    n = ip.numel() - 1
    n_cols = N_COLS if name == "hand" else 64
    sel = select(n_cols, how)
    tip, tix, ep1 = C.transpose_csr(ip, ix, n_cols)
    gip, gix = C.gather_rows_csr(tip, tix, sel)
    src = C.gather_rows_csr(tip, ep1, sel)[1]
    oip, oix, ep2 = C.transpose_csr(gip, gix, n)
    colmap = torch.full((n_cols,), -1, dtype=torch.int32)
    colmap[sel] = torch.arange(sel.numel(), dtype=torch.int32)
    segs = C.build_segments(ip, L)
    assert name != "hand" or int((segs[2][1:] - segs[2][:-1]).max()) > 1
    got = C.csr_filter_cols(ip.to(DEV), ix.to(DEV), colmap.to(DEV),
                            tuple(s.to(DEV) for s in segs))
    same(got, (oip, oix, src[ep2]), (name, how, L))


@functools.lru_cache(maxsize=None)
def work_indptr(name):
    if name == "empty":
        return torch.zeros(50, dtype=torch.int64)
    if name == "offset":                     # a CSR that does not start at 0
        return hand_csr()[0] + 7
    if name == "million":                    # >= 1,000,000 items: 262144 waves
        return torch.arange(T * T + 2)
    return hand_csr()[0]


@pytest.mark.parametrize("name,seg,max_waves", [
    (n, s, w) for n in ("hand", "offset") for s in (8, 512)
    for w in (8, 64, None)] + [("empty", 512, None), ("million", 512, None)])
def test_build_worklist(name, seg, max_waves):
    ip = work_indptr(name)
    want = C.build_worklist(ip, seg=seg, max_waves=max_waves)
    assert name != "million" or want[3].numel() == 262144 + 1
    got = C.build_worklist_hip(ip.to(DEV), seg=seg, max_waves=max_waves)
    same(got, want, (name, seg, max_waves))


def _worklists_match(dev_ip, host_ip, tag):
    wl = dev_ip._bns_worklist          # attached by the composite call
    same(wl, C.build_worklist(host_ip), tag)


@pytest.mark.parametrize("unit_ratio", [False, True])
@pytest.mark.parametrize("rate", [0.1, 0.4])
def test_halo_plan_and_rows_halo(rate, unit_ratio, monkeypatch):
    """HaloPlan._build and GraphContext._build_rows_halo on the device
    (switch on) against the CPU plan, every rank of the 3-partition
    fixture at epochs 0 and 3: every EpochState tensor, the restricted
    CSRs and the cached work lists. SEG and FILTER_SEG are lowered so the
    fixture holds split items and multi-segment rows; the map `pos` is
    back to all -1 after each build."""
    from bnsgcn_amd.models.context import GraphContext
    assert C.PLAN_HIP
    monkeypatch.setattr(C, "SEG", 16)
    monkeypatch.setattr(C, "FILTER_SEG", 32)
    for part in P.fixture_parts(3)[1]:
        host = P.make_plan(part, rate, "cpu", unit_ratio=unit_ratio)
        dev = P.make_plan(part, rate, DEV, unit_ratio=unit_ratio)
        rows = torch.from_numpy(np.flatnonzero(part.train_mask))
        hctx = GraphContext.for_partition(part, host, "cpu", need_eperm=False)
        dctx = GraphContext.for_partition(part, dev, DEV, need_eperm=False)
        for epoch in (0, 3):
            sh, sd = host._build(epoch), dev._build(epoch)
            tag = (part.rank, rate, epoch)
            assert sd.send_counts == sh.send_counts, tag
            assert sd.recv_counts == sh.recv_counts, tag
            fields = [f for f in PLAN_TENSORS if getattr(sh, f) is not None]
            assert all(getattr(sd, f) is not None for f in fields)
            same([getattr(sd, f) for f in fields],
                 [getattr(sh, f) for f in fields], tag)
            assert bool((dev._hip[3] == -1).all()), tag
            _worklists_match(sd.halo_fwd_indptr, sh.halo_fwd_indptr, tag)
            _worklists_match(sd.halo_bwd_indptr, sh.halo_bwd_indptr, tag)
            rh = hctx._build_rows_halo(rows, sh)
            rd = dctx._build_rows_halo(rows.to(DEV), sd)
            same(rd, rh, tag)
            _worklists_match(rd[0], rh[0], tag)
            _worklists_match(rd[2], rh[2], tag)


@pytest.mark.parametrize("model", ["graphsage", "gat"])
def test_training_step_same_with_switch_off(model, monkeypatch):
    """One training step of rank 1 of the 2-partition fixture with the
    device plan build and again with the torch one: the kernels get the
    same integer inputs, so loss, logits, every gradient and every send
    are equal bit for bit."""
    g, parts = P.fixture_parts(2)
    args = P.step_args(model, use_pp=False)
    runs = []
    for on in (True, False):
        monkeypatch.setattr(C, "PLAN_HIP", on)
        runs.append(P.run_training_step(parts[1], g, args, DEV,
                                        torch.float32))
    assert runs[0].keys() == runs[1].keys()
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
