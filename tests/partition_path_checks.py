"""Stubbed halo exchange, fixtures and runners for
tests/test_gpu_partition_path.py.

One rank of a multi-partition job is checked in ONE process: everything a
rank computes in a step is either an output or a buffer it hands to the
exchange, so a stub with the signature of comm.all_to_all_rows that
RECORDS what is sent and FILLS what is received makes the whole per-rank
path comparable between devices. The reference is the project's own CPU
path (ops/reference.py under the same autograd Functions) in float64 on
the same fp32 inputs; nothing here starts a process group, calls a
collective or starts a child process.

Every function works on the CPU as well, so the float64-vs-fp32 CPU
comparison (and a deliberately broken stub) can be tried without a GPU.
"""
from __future__ import annotations

import contextlib
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kernel_path_checks import assert_sum_bound  # noqa: E402,F401

DEV = "cuda:0"
PLAN_SEED = 5
# device-side spin queued in front of every fill of a device buffer
# (torch.cuda._sleep cycles; about 0.09 ms on the MI355X)
DELAY_CYCLES = 200_000


# ----------------------------------------------------------------- stub

def stub_rows(shape, occurrence: int) -> torch.Tensor:
    """The rows the stub supplies for the `occurrence`-th call with a
    receive buffer of `shape`: CPU float64 randn from a seed made of the
    shape and the occurrence only (never a global call counter, so a
    harmless difference in call order between devices cannot
    desynchronise the values), rounded to fp32-representable values so a
    float64 and an fp32 receive buffer get the SAME numbers."""
    r, f = int(shape[0]), int(shape[1])
    g = torch.Generator().manual_seed((r * 1_000_003 + f) * 1_009 + occurrence)
    rows = torch.randn(r, f, generator=g, dtype=torch.float64)
    return rows.float().double()


class StubExchange:
    """Drop-in for comm.all_to_all_rows.

    Record: appends (send.detach().clone(), list(recv_counts),
    list(send_counts)) to `log`. Fill: copies stub_rows(...) cast to
    recv.dtype into recv, issued on the CURRENT stream (the comm stream
    in the overlap path). absolute=True fills |rows| (for the
    absolute-value reference run). delay_cycles > 0 queues a device-side
    spin in front of the fill of a device buffer: the host blocks in the
    staged host-to-device copy, so without it the rows would always have
    landed before the consumer is even launched and a missing
    cross-stream wait could not show. (Measured: with the wait_event
    calls of parallel/halo.py turned into no-ops, the overlap run of
    the stream test stays bitwise equal to the sequential one at 0 and
    20000 cycles and differs at 200000.)"""

    def __init__(self, absolute: bool = False,
                 delay_cycles: int = DELAY_CYCLES):
        self.log: list = []
        self.absolute = absolute
        self.delay_cycles = int(delay_cycles)
        self._seen: dict = {}

    def __call__(self, recv, send, recv_counts, send_counts, async_op=False):
        self.log.append((send.detach().clone(), list(recv_counts),
                         list(send_counts)))
        assert recv.shape[0] == sum(recv_counts), (recv.shape, recv_counts)
        assert send.shape[0] == sum(send_counts), (send.shape, send_counts)
        key = tuple(recv.shape)
        k = self._seen.get(key, 0)
        self._seen[key] = k + 1
        rows = stub_rows(key, k)
        if self.absolute:
            rows = rows.abs()
        rows = rows.to(recv.dtype)
        if recv.is_cuda and self.delay_cycles:
            rows = rows.to(recv.device)          # staged copy, host blocks
            torch.cuda._sleep(self.delay_cycles)  # then spin, then fill
        recv.copy_(rows)
        return None

    def sends(self):
        """Recorded send buffers as CPU tensors keyed (shape, occurrence)."""
        out, seen = {}, {}
        for send, _, _ in self.log:
            key = tuple(send.shape)
            k = seen.get(key, 0)
            seen[key] = k + 1
            out[(key, k)] = send.cpu()
        return out


@contextlib.contextmanager
def installed(stub):
    """monkeypatch.setattr of the two names the code under test calls."""
    import bnsgcn_amd.parallel.halo as halo
    import bnsgcn_amd.runtime.trainer as trainer
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(halo, "all_to_all_rows", stub)
        mp.setattr(trainer, "all_to_all_rows", stub)
        yield stub


def sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


# ------------------------------------------------------------- fixtures

@functools.lru_cache(maxsize=None)
def fixture_parts(n_parts: int):
    """tiny (200 nodes), seed 21, random partition seed 1. P=3: a boundary
    node can belong to two peers (repeated scatter indices); P=2: every
    packed row index is unique (order-independent scatter)."""
    from bnsgcn_amd.graph import load_data, partition_graph
    g = load_data("tiny", seed=21)
    parts, meta = partition_graph(g, n_parts, method="random", seed=1)
    for p in parts:
        p.meta = meta
    if n_parts == 3:
        rep = [np.unique(np.concatenate(p.boundary), return_counts=True)[1]
               for p in parts]
        assert all((c > 1).any() for c in rep), "no node borders two peers"
    return g, parts


def make_plan(part, rate, device, unit_ratio=False, wire_dtype=None):
    from bnsgcn_amd.parallel.plan import HaloPlan
    return HaloPlan(part, rate, seed=PLAN_SEED, device=device,
                    unit_ratio=unit_ratio, wire_dtype=wire_dtype)


def _assert_split_item(indptr, what):
    """zero_rows of the work list (empty + split rows) holds a non-empty
    row, i.e. a row split into items combined by atomicAdd."""
    from bnsgcn_amd.ops.csr_torch import build_worklist
    ip = indptr.cpu()
    deg = ip[1:] - ip[:-1]
    assert (deg[build_worklist(ip)[4]] > 0).any(), f"no split item in {what}"
    wl = getattr(indptr, "_bns_worklist", None)
    if wl is not None:           # the list the device kernel will use
        assert (deg[wl[4].cpu()] > 0).any(), f"device {what}: no split item"


def assert_halo_preconditions(plan, st, want_empty_row=True, split=None,
                              rows=None):
    """The fixture cannot silently degenerate: every peer sends and
    receives, the sampled halo CSR (restricted to `rows` if given) has
    empty AND non-empty destination rows, and, after SEG was lowered, the
    halo forward (split="fwd") or backward (split="bwd") work list holds
    a split item."""
    for j in range(plan.n_parts):
        if j == plan.rank:
            assert st.send_counts[j] == 0 and st.recv_counts[j] == 0
            continue
        assert st.send_counts[j] > 0, (plan.rank, j, st.send_counts)
        assert st.recv_counts[j] > 0, (plan.rank, j, st.recv_counts)
    assert st.pack_idx.numel() == sum(st.send_counts)
    assert st.hsel.numel() == sum(st.recv_counts)
    ip = st.halo_fwd_indptr.cpu()
    deg = ip[1:] - ip[:-1]
    if rows is not None:
        deg = deg[rows.cpu()]
    assert (deg > 0).any(), "halo CSR has no edge"
    if want_empty_row:
        assert (deg == 0).any(), "halo CSR has no empty destination row"
    assert split in (None, "fwd", "bwd"), split
    if split == "fwd":
        _assert_split_item(st.halo_fwd_indptr, "the halo forward list")
    elif split == "bwd":
        _assert_split_item(st.halo_bwd_indptr, "the halo backward list")


def term_counts(part, st, rows=None):
    """Reduction lengths of one partition_aggregate, from the partition's
    numpy arrays and the plan's hsel / pack_idx only (not from the CSRs
    the code under test builds): (out rows, x.grad rows, gr rows)."""
    n = part.n_inner
    keep = np.ones(n, dtype=bool)
    if rows is not None:
        keep[:] = False
        keep[rows.cpu().numpy()] = True
    ideg = np.diff(part.inner_indptr)
    dst_of_edge = np.repeat(np.arange(n), ideg)
    ek = keep[dst_of_edge]
    tdeg = np.bincount(part.inner_indices[ek], minlength=n)
    hsel = st.hsel.cpu().numpy()
    hip_, hix = part.halo_indptr, part.halo_indices
    hdeg = np.zeros(n, dtype=np.int64)
    gr_len = np.zeros(len(hsel), dtype=np.int64)
    for k, h in enumerate(hsel):
        cols = hix[hip_[h]:hip_[h + 1]]
        cols = cols[keep[cols]]
        np.add.at(hdeg, cols, 1)
        gr_len[k] = len(cols)
    n_out = ideg + hdeg
    if rows is not None:
        n_out = n_out[rows.cpu().numpy()]
    n_gx = tdeg + np.bincount(st.pack_idx.cpu().numpy(), minlength=n)
    as_col = lambda a: torch.from_numpy(a.astype(np.float64))[:, None]
    return as_col(n_out), as_col(n_gx), as_col(gr_len)


# -------------------------------------------------------------- runners

def run_aggregate(part, device, dtype, x, g, mode, rate, epoch=3, rows=None,
                  wire_dtype=None, absolute=False, split=None, mutate=None):
    """ctx.aggregate(x, mode[, rows]) + backward(g) for one rank under a
    fresh stub. x, g: fp32 CPU tensors, cast to (device, dtype);
    absolute=True runs on |x|, |g| and the stub's |rows|. Returns out,
    x.grad and the recorded forward / backward sends (CPU tensors)."""
    from bnsgcn_amd.models.context import GraphContext
    plan = make_plan(part, rate, device, wire_dtype=wire_dtype)
    st = plan.set_epoch(epoch)
    assert_halo_preconditions(plan, st, want_empty_row=rate < 1.0,
                              split=split, rows=rows)
    if mutate is not None:
        mutate(st)
    ctx = GraphContext.for_partition(part, plan, device, need_eperm=False)
    r = None
    if rows is not None:
        r = rows.to(device)
        ctx.loss_rows = r            # as RankState does
    if absolute:
        x, g = x.abs(), g.abs()
    xd = x.to(device=device, dtype=dtype).requires_grad_(True)
    gd = g.to(device=device, dtype=dtype)
    with installed(StubExchange(absolute)) as stub:
        out = ctx.aggregate(xd, mode, rows=r)
        out.backward(gd)
        sync(device)
    assert len(stub.log) == 2, len(stub.log)
    (fwd, rc0, sc0), (bwd, rc1, sc1) = stub.log
    assert rc0 == st.recv_counts and sc0 == st.send_counts
    assert rc1 == st.send_counts and sc1 == st.recv_counts
    return {"out": out.detach().cpu(), "gx": xd.grad.cpu(),
            "pack": fwd.cpu(), "gr": bwd.cpu(), "st": st}


def run_halo_exchange(part, device, dtype, x, g, rate, unit_ratio, epoch=3,
                      absolute=False):
    """halo_exchange(x) + backward(g) for one rank under a fresh stub."""
    from bnsgcn_amd.parallel.halo import halo_exchange
    plan = make_plan(part, rate, device, unit_ratio=unit_ratio)
    st = plan.set_epoch(epoch)
    assert_halo_preconditions(plan, st)
    assert (st.pack_scale is None) == unit_ratio
    if absolute:
        x, g = x.abs(), g.abs()
    xd = x.to(device=device, dtype=dtype).requires_grad_(True)
    gd = g.to(device=device, dtype=dtype)
    with installed(StubExchange(absolute)) as stub:
        recv = halo_exchange(xd, plan)
        recv.backward(gd)
        sync(device)
    assert len(stub.log) == 2
    return {"recv": recv.detach().cpu(), "gx": xd.grad.cpu(),
            "pack": stub.log[0][0].cpu(), "gback": stub.log[1][0].cpu(),
            "st": st}


def step_args(model, use_pp, norm="layer"):
    from bnsgcn_amd.runtime.config import create_parser
    args = create_parser().parse_args([])
    args.dataset = "tiny"
    args.model = model
    args.use_pp = use_pp
    args.norm = norm
    args.n_layers = 3
    args.n_hidden = 16
    args.heads = 2
    args.dropout = 0.0
    args.sampling_rate = 0.4
    args.seed = PLAN_SEED
    return args


def run_training_step(part, g, args, device, dtype, epoch=3, stub=None):
    """One training step (forward_train_logits, sum-reduced cross-entropy,
    backward) of one rank of a multi-partition job, then the eval-mode
    forward over the full halo state (the path dist_evaluate takes).
    Returns a dict name -> CPU tensor: logits, loss, eval logits, every
    parameter gradient and every recorded send."""
    from bnsgcn_amd.models.models import create_model
    from bnsgcn_amd.runtime.trainer import RankState, forward_train_logits
    stub = StubExchange() if stub is None else stub
    with installed(stub):
        state = RankState(part, args, device)
        if dtype != torch.float32:
            state.feat = state.feat.to(dtype)
            state.raw_feat = state.feat
        st = state.plan.set_epoch(epoch)
        assert_halo_preconditions(state.plan, st)
        torch.manual_seed(0)
        model = create_model(args, n_feat=g.n_feat, n_class=g.n_class,
                             train_size=g.n_train).to(device=device,
                                                      dtype=dtype)
        if args.use_pp or args.model == "gat":
            state.precompute()
            full = state.ctx.full_state()
            assert sum(full.recv_counts) == part.n_halo > 0
        model.train()
        logits = forward_train_logits(model, state)
        assert logits.shape[0] == int(part.train_mask.sum())
        labels = state.label[state.train_mask].long()
        loss = torch.nn.functional.cross_entropy(logits, labels,
                                                 reduction="sum")
        loss.backward()
        res = {"logits": logits.detach().cpu(),
               "loss": loss.detach().cpu().reshape(1)}
        for name, p in model.named_parameters():
            assert p.grad is not None, name
            res["grad " + name] = p.grad.detach().cpu()
        # eval-mode forward, as dist_evaluate runs it
        saved = state.plan._state
        state.plan._state = state.ctx.full_state()
        model.eval()
        with torch.no_grad():
            res["eval logits"] = model(state.ctx, state.raw_feat).cpu()
        state.plan._state = saved
        sync(device)
    for (shape, k), t in stub.sends().items():
        res[f"send {shape}#{k}"] = t
    return res


def compare_measured(ref64, ref32, got, tag):
    """The rule of test_gat_block_gradients_composite, per tensor:
    e32 = max|fp32-CPU - float64| / max|float64|; the GPU may differ from
    float64 by at most max(8 * e32, 1e-5) on the same scale (it differs
    from the fp32 CPU run only in summation order, fast exp and atomics).
    Prints the three figures per tensor; returns them."""
    assert ref64.keys() == ref32.keys() == got.keys(), (
        sorted(ref64.keys() ^ got.keys()), sorted(ref64.keys() ^ ref32.keys()))
    failures, figures = [], {}
    for name, r64 in ref64.items():
        r64 = r64.double()
        g_, r32 = got[name].double(), ref32[name].double()
        assert g_.shape == r64.shape == r32.shape, (name, g_.shape, r64.shape)
        assert torch.isfinite(g_).all(), f"{tag} {name}: non-finite"
        scale = float(r64.abs().max()) if r64.numel() else 0.0
        if scale == 0.0:
            assert not g_.any(), f"{tag} {name}: reference is all zero"
            continue
        e32 = float((r32 - r64).abs().max()) / scale
        egot = float((g_ - r64).abs().max()) / scale
        tol = max(8 * e32, 1e-5)
        figures[name] = (e32, egot, tol)
        print(f"{tag} {name}: fp32-cpu rel err {e32:.3g}, "
              f"got rel err {egot:.3g}, tol {tol:.3g}")
        if not egot <= tol:
            failures.append((name, egot, tol))
    assert not failures, (tag, failures)
    return figures


def train_epochs(part, g, model, device, epochs):
    """The loop of test_stream_overlap_ordering_stress on one rank of a
    2-partition job with the stub installed: returns (losses, final
    parameters, fewest rows received by an exchange call per epoch,
    exchange calls per epoch, epochs whose plan came from prefetch)."""
    from bnsgcn_amd.models.models import create_model
    from bnsgcn_amd.parallel import GradReducer
    from bnsgcn_amd.runtime.trainer import RankState, forward_train_logits
    args = step_args(model, use_pp=False)
    args.n_hidden = 32
    args.dropout = 0.2
    stub = StubExchange()
    with installed(stub):
        torch.manual_seed(11)
        state = RankState(part, args, device)
        st = state.plan.set_epoch(0)
        assert_halo_preconditions(state.plan, st)
        m = create_model(args, n_feat=g.n_feat, n_class=g.n_class,
                         train_size=g.n_train).to(device)
        if model == "gat":
            state.precompute()
        reducer = GradReducer(m, g.n_train)
        fused = torch.device(device).type == "cuda"
        opt = torch.optim.Adam(m.parameters(), lr=1e-2, fused=fused)
        lf = torch.nn.CrossEntropyLoss(reduction="sum")
        labels = state.label[state.train_mask].long()
        losses, moved, calls, prefetched = [], [], [], 0
        for ep in range(epochs):
            n0 = len(stub.log)
            state.plan.set_epoch(ep)
            m.train()
            loss = lf(forward_train_logits(m, state), labels)
            reducer.zero_grad()
            loss.backward()
            state.prefetch(ep + 1)
            prefetched += getattr(state.plan, "_next", None) is not None
            reducer.synchronize()
            opt.step()
            losses.append(loss.item())
            new = stub.log[n0:]
            calls.append(len(new))
            moved.append(min((sum(rc) for _, rc, _ in new), default=0))
        sync(device)
        params = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    return np.array(losses), params, moved, calls, prefetched
