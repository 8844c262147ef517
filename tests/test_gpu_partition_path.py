"""GPU (MI355X): one rank of a MULTI-partition job, with a non-empty halo.

Every other GPU test partitions into one part, where the halo plan is
empty and the exchange moves nothing. Here rank r of a 3- (or 2-)
partition job runs in one process against a stubbed exchange
(tests/partition_path_checks.py) that records every send buffer and
fills every receive buffer with the same pseudo-random rows on both
devices, so HaloPlan._build on device, pack_rows with the 1/ratio scale,
the halo SpMM accumulating into the inner SpMM's output, the backward
halo SpMM, scatter_add_rows, the loss-row restriction, halo_exchange,
the split GAT block fed by a real halo, RankState.precompute with a full
halo, the bf16 wire cast and the cross-stream ordering are all run with
data in them.

Reference: the project's own CPU path in float64 on the same fp32 inputs.
Tolerances: the any-order summation bound of kernel_path_checks.py for
the aggregation, the measured fp32-vs-float64 rule of
test_gat_block_gradients_composite for whole training steps, bitwise
equality for the stream tests.

Run on the GPU box:
  python -m pytest tests/test_gpu_partition_path.py -m gpu -x -q
"""
import numpy as np
import pytest
import torch

import partition_path_checks as P
from kernel_path_checks import gen
from partition_path_checks import DEV, assert_sum_bound

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bnsgcn_amd.ops._ext import require_ext
    ext = require_ext()
else:
    ext = None

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

EPOCH = 3       # rate 0.4: ranks 0 and 2 have a halo row of 97 / 44 edges

PLAN_TENSORS = ("pack_idx", "pack_scale", "hsel",
                "halo_fwd_indptr", "halo_fwd_indices",
                "halo_bwd_indptr", "halo_bwd_indices",
                "halo_eperm_t", "halo_out_norm_inv", "halo_in_deg")


def _row_of_edge(indptr):
    n = indptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n), indptr[1:] - indptr[:-1])


def _train_rows(part):
    return torch.from_numpy(np.flatnonzero(part.train_mask))


# ------------------------------------------------- 1. device plan == host

@needs_gpu
@pytest.mark.parametrize("unit_ratio", [False, True])
@pytest.mark.parametrize("rate", [0.1, 0.4, 1.0])
def test_device_plan_equals_host_plan(rate, unit_ratio):
    """HaloPlan._build on device (Philox keys kernel, stable argsort per
    peer, gather_rows_csr, transpose_csr, eperm_t inversion) against the
    numpy-sampled host plan, every rank of the 3-partition fixture at
    epochs 0, 1 and 7: every tensor of EpochState equal in value AND
    dtype, the count lists equal. halo_eperm_t is then checked against
    its definition on the device plan's tensors: a distinct per-edge
    payload w on the forward edge set, laid over the backward CSR as
    w[halo_eperm_t], describes the same (dst, recv row, w) triples."""
    _, parts = P.fixture_parts(3)
    for part in parts:
        host = P.make_plan(part, rate, "cpu", unit_ratio=unit_ratio)
        dev = P.make_plan(part, rate, DEV, unit_ratio=unit_ratio)
        for epoch in (0, 1, 7):
            # _build, not set_epoch: rate 1.0 would hand back epoch 0's
            # cached state
            sh, sd = host._build(epoch), dev._build(epoch)
            tag = f"rank {part.rank} rate {rate} epoch {epoch}"
            P.assert_halo_preconditions(host, sh, want_empty_row=rate < 1.0)
            assert sd.send_counts == sh.send_counts, tag
            assert sd.recv_counts == sh.recv_counts, tag
            assert sd.epoch == sh.epoch == epoch
            assert (sh.pack_scale is None) == unit_ratio
            for f in PLAN_TENSORS:
                th, td = getattr(sh, f), getattr(sd, f)
                if th is None:
                    assert td is None, (tag, f)
                    continue
                assert td.is_cuda, (tag, f)
                assert td.dtype == th.dtype, (tag, f, td.dtype, th.dtype)
                assert td.shape == th.shape, (tag, f, td.shape, th.shape)
                assert torch.equal(td.cpu(), th), (tag, f)

            fip, fix = sd.halo_fwd_indptr.cpu(), sd.halo_fwd_indices.cpu()
            bip, bix = sd.halo_bwd_indptr.cpu(), sd.halo_bwd_indices.cpu()
            ep = sd.halo_eperm_t.cpu()
            E = fix.numel()
            assert E > 0 and bix.numel() == E and ep.numel() == E
            assert torch.equal(torch.sort(ep)[0], torch.arange(E)), tag
            w = torch.randperm(E, generator=gen(epoch)).double()
            of, ob = torch.argsort(w), torch.argsort(w[ep])
            assert torch.equal(w[of], w[ep][ob])
            # forward: row = dst, col = recv row; backward: the transpose
            assert torch.equal(_row_of_edge(fip)[of], bix.long()[ob]), tag
            assert torch.equal(fix.long()[of], _row_of_edge(bip)[ob]), tag


# ------------------------------------- 2. partition_aggregate vs float64

def _check_aggregate(part, mode, F, rate, split=None, rows=None,
                     device=DEV, mutate=None):
    """out, x.grad, the packed forward send and the backward send gr of
    one ctx.aggregate on `device` in fp32 against the float64 CPU run of
    the same code on the same inputs, under assert_sum_bound with the
    float64 run on absolute values as ref64_abs."""
    x = torch.randn(part.n_inner, F, generator=gen(1000 + 10 * part.rank + F))
    g_rows = part.n_inner if rows is None else rows.numel()
    g = torch.randn(g_rows, F, generator=gen(2000 + 10 * part.rank + F))
    kw = dict(mode=mode, rate=rate, epoch=EPOCH, rows=rows)
    r64 = P.run_aggregate(part, "cpu", torch.float64, x, g, **kw)
    rabs = P.run_aggregate(part, "cpu", torch.float64, x, g, absolute=True,
                           **kw)
    got = P.run_aggregate(part, device, torch.float32, x, g, split=split,
                          mutate=mutate, **kw)
    n_out, n_gx, n_gr = P.term_counts(part, r64["st"], rows)
    tag = f"rank {part.rank} {mode} F={F} rate={rate} split={split}"
    if rows is not None:
        tag += " rows"
    assert got["pack"].dtype == got["gr"].dtype == torch.float32
    # an element with no term (empty halo row, node that is never packed
    # and has no out-edge, ...) has bound 0: it must be exactly 0
    for key, n in (("pack", 0.0), ("out", n_out), ("gr", n_gr),
                   ("gx", n_gx)):
        assert_sum_bound(got[key], r64[key], rabs[key], n, f"{tag} {key}")


@needs_gpu
@pytest.mark.parametrize("seg", [None, 16])
@pytest.mark.parametrize("rate", [0.4, 1.0])
@pytest.mark.parametrize("F", [17, 64])
@pytest.mark.parametrize("mode", ["gcn", "mean"])
def test_partition_aggregate_matches_float64(monkeypatch, mode, F, rate, seg):
    """_PartitionAggregate with a non-empty halo on every rank of the
    3-partition fixture: pack_rows with the 1/ratio scale, the halo SpMM
    accumulating into the inner SpMM's output (out=, acc, hscale for
    'gcn'), the backward halo SpMM and scatter_add_rows into gx with
    indices repeated across peers. F=17 takes the scalar kernels, F=64
    the vec4 ones. seg=16 lowers the heavy-row split granularity so the
    halo work lists hold split (atomicAdd) items: in the forward list,
    except on rank 1 at rate 0.4, whose sampled halo has at most 7 edges
    per destination row — there the BACKWARD halo list (23-edge row) is
    the one asserted to split."""
    from bnsgcn_amd.ops import csr_torch
    if seg is not None:
        monkeypatch.setattr(csr_torch, "SEG", seg)
    _, parts = P.fixture_parts(3)
    for part in parts:
        split = None
        if seg is not None:
            split = "bwd" if (part.rank == 1 and rate < 1.0) else "fwd"
        _check_aggregate(part, mode, F, rate, split=split)


@needs_gpu
def test_partition_aggregate_loss_rows_matches_float64():
    """The same comparison under the final-layer loss-row restriction
    (rows = the rank's train rows, ctx.loss_rows set as RankState does):
    _rows_inner_csrs and _rows_halo_csrs feed the kernels."""
    _, parts = P.fixture_parts(3)
    for part in parts:
        rows = _train_rows(part)
        assert 0 < rows.numel() < part.n_inner
        _check_aggregate(part, "mean", 17, 0.4, rows=rows)
        _check_aggregate(part, "mean", 64, 0.4, rows=rows)


# ------------------------------------------- 3. halo_exchange vs float64

@needs_gpu
@pytest.mark.parametrize("F", [16, 30])
@pytest.mark.parametrize("unit_ratio", [False, True])
def test_halo_exchange_matches_float64(unit_ratio, F):
    """_HaloExchange forward and backward on every rank: the recorded
    pack, the returned rows (what the stub supplied, bit for bit), the
    gradient handed back to the exchange (g itself) and x.grad after the
    scatter with repeated indices."""
    _, parts = P.fixture_parts(3)
    for part in parts:
        x = torch.randn(part.n_inner, F, generator=gen(3000 + F))
        plan = P.make_plan(part, 0.4, "cpu", unit_ratio=unit_ratio)
        R = sum(plan.set_epoch(EPOCH).recv_counts)
        g = torch.randn(R, F, generator=gen(3100 + F))
        kw = dict(rate=0.4, unit_ratio=unit_ratio, epoch=EPOCH)
        r64 = P.run_halo_exchange(part, "cpu", torch.float64, x, g, **kw)
        rabs = P.run_halo_exchange(part, "cpu", torch.float64, x, g,
                                   absolute=True, **kw)
        got = P.run_halo_exchange(part, DEV, torch.float32, x, g, **kw)
        tag = f"halo_exchange rank {part.rank} unit={unit_ratio} F={F}"
        assert got["recv"].dtype == torch.float32
        assert torch.equal(got["recv"].double(), r64["recv"]), tag
        assert torch.equal(got["recv"].double(), P.stub_rows((R, F), 0)), tag
        assert torch.equal(got["gback"].double(), r64["gback"]), tag
        assert torch.equal(got["gback"], g), tag
        n_gx = torch.bincount(r64["st"].pack_idx,
                              minlength=part.n_inner).double()[:, None]
        assert (n_gx > 1).any() and (n_gx == 0).any()
        assert_sum_bound(got["pack"], r64["pack"], rabs["pack"], 0.0,
                         f"{tag} pack")
        assert_sum_bound(got["gx"], r64["gx"], rabs["gx"], n_gx,
                         f"{tag} gx")


# ------------------------------------------------------------ 4. bf16 wire

@needs_gpu
def test_partition_aggregate_bf16_wire():
    """wire_dtype=torch.bfloat16 on the plan (rank 1, 'gcn', F=64, rate
    0.4): both recorded sends are bfloat16 and, upcast, equal the float64
    reference's unrounded pack / gr to within one bf16 ulp (rtol 2^-7,
    atol 0; exact zeros where the reference is zero). out and x.grad are
    compared under the ordinary bound with a float64 run on the same
    plan, which the stub feeds the same bf16-rounded rows."""
    _, parts = P.fixture_parts(3)
    part = parts[1]
    F, bf16 = 64, torch.bfloat16
    x = torch.randn(part.n_inner, F, generator=gen(4000))
    g = torch.randn(part.n_inner, F, generator=gen(4001))
    kw = dict(mode="gcn", rate=0.4, epoch=EPOCH)
    plain = P.run_aggregate(part, "cpu", torch.float64, x, g, **kw)
    r64 = P.run_aggregate(part, "cpu", torch.float64, x, g, wire_dtype=bf16,
                          **kw)
    rabs = P.run_aggregate(part, "cpu", torch.float64, x, g, wire_dtype=bf16,
                           absolute=True, **kw)
    got = P.run_aggregate(part, DEV, torch.float32, x, g, wire_dtype=bf16,
                          **kw)
    assert plain["pack"].dtype == plain["gr"].dtype == torch.float64
    for key in ("pack", "gr"):
        assert got[key].dtype == bf16, (key, got[key].dtype)
        assert r64[key].dtype == bf16
        up, want = got[key].double(), plain[key]
        assert (want != 0).any()
        assert not up[want == 0].any(), f"bf16 {key}: non-zero where ref is 0"
        torch.testing.assert_close(up, want, rtol=2.0 ** -7, atol=0.0,
                                   msg=lambda m: f"bf16 wire {key}: {m}")
    n_out, n_gx, _ = P.term_counts(part, r64["st"])
    assert got["out"].dtype == got["gx"].dtype == torch.float32
    assert_sum_bound(got["out"], r64["out"], rabs["out"], n_out,
                     "bf16 wire out")
    assert_sum_bound(got["gx"], r64["gx"], rabs["gx"], n_gx, "bf16 wire gx")


# -------------------------------- 5. one training step per model, rank 1

STEP_CONFIGS = [("gcn", False, "layer"), ("gcn", True, "layer"),
                ("graphsage", True, "layer"), ("graphsage", False, "layer"),
                ("gat", True, "layer"), ("gat", False, "none")]


@needs_gpu
@pytest.mark.parametrize("model,use_pp,norm", STEP_CONFIGS)
def test_training_step_multi_partition_rank(model, use_pp, norm):
    """Rank 1 of the 3-partition fixture, sampling rate 0.4, 3 layers,
    hidden 16, 2 heads, no dropout, epoch 3: RankState, precompute over
    the FULL halo (use_pp / gat), forward_train_logits with the final
    layer restricted to the train rows, sum-reduced cross-entropy,
    backward; then the eval-mode forward over the full halo state, the
    path dist_evaluate takes. Train logits, loss, eval logits, every
    parameter gradient and every recorded send (keyed by shape and
    occurrence) are compared with the float64 CPU run of the same code.

    Tolerance, measured per tensor and printed: e32 = max|fp32 CPU -
    float64| / max|float64|; the GPU may differ from float64 by at most
    max(8 * e32, 1e-5) on the same scale."""
    g, parts = P.fixture_parts(3)
    part = parts[1]
    args = P.step_args(model, use_pp, norm)
    ref64 = P.run_training_step(part, g, args, "cpu", torch.float64)
    ref32 = P.run_training_step(part, g, args, "cpu", torch.float32)
    got = P.run_training_step(part, g, args, DEV, torch.float32)
    n_sends = sum(k.startswith("send ") for k in got)
    assert n_sends >= 7, n_sends       # 2-3 layers x fwd/bwd + eval + pp
    P.compare_measured(ref64, ref32, got,
                       f"step {model} use_pp={use_pp} norm={norm}")


# ----------------------------- 6. stream ordering with data in the halo

def _stream_runs(monkeypatch, model, epochs):
    from bnsgcn_amd.ops import csr_torch
    monkeypatch.setattr(csr_torch, "SEG", 10 ** 9)
    g, parts = P.fixture_parts(2)
    part = parts[0]
    assert part.n_inner < 256          # syncbn_stats: one row chunk
    for p in parts:                    # P=2: packed row indices are unique
        assert np.unique(np.concatenate(p.boundary),
                         return_counts=True)[1].max() == 1

    def run(sequential):
        for name in ("BNSGCN_NO_OVERLAP", "BNSGCN_NO_PREFETCH"):
            if sequential:
                monkeypatch.setenv(name, "1")
            else:
                monkeypatch.delenv(name, raising=False)
        return P.train_epochs(part, g, model, DEV, epochs)

    a1, a2, b = run(False), run(False), run(True)
    for losses, _, moved, calls, prefetched in (a1, a2, b):
        assert np.isfinite(losses).all()
        assert all(c > 0 for c in calls), calls
        assert all(m > 0 for m in moved), moved   # every exchange had rows
    assert a1[4] == a2[4] == epochs and b[4] == 0  # prefetch really used
    assert a1[3] == b[3]
    np.testing.assert_array_equal(a1[0], a2[0])    # run-to-run deterministic
    np.testing.assert_array_equal(a1[0], b[0])     # overlap == sequential
    for name, t in a1[1].items():
        assert torch.equal(t, a2[1][name]), f"run-to-run: {name}"
        assert torch.equal(t, b[1][name]), f"overlap vs sequential: {name}"


@needs_gpu
def test_stream_ordering_with_halo_traffic_gcn(monkeypatch):
    """The setting of test_stream_overlap_ordering_stress (gcn, 3 layers,
    hidden 32, no use_pp, rate 0.4, dropout 0.2, fused Adam, SEG=1e9) on
    rank 0 of the 2-partition fixture with the stub installed, so the
    side-stream exchange moves rows in every layer and the prefetched
    plan holds real tensors. 12 epochs with prefetch(ep + 1) after
    backward: two overlap runs and one run with BNSGCN_NO_OVERLAP=1 and
    BNSGCN_NO_PREFETCH=1 must give bitwise identical losses AND final
    parameters — a missing wait_event / record_stream in halo.py, plan.py
    or context.py is a value change here. The stub spins on the device
    before it fills a receive buffer, so the rows land AFTER the host has
    queued the consumer; without that spin the removal of halo.py's waits
    was measured to change nothing. The plan prefetch has no such lever:
    its build synchronises with the host several times, which leaves only
    its last few kernels racing against a missing wait.

    Bitwise equality is legitimate: P=2 makes every packed row index
    unique (order-independent scatter), SEG=1e9 leaves no split rows, and
    100 inner rows stay under the 256-row / 128-deep thresholds at which
    syncbn_stats, ln_bwd and the split-K dW GEMM start combining with
    atomics."""
    _stream_runs(monkeypatch, "gcn", 12)


@needs_gpu
def test_stream_ordering_with_halo_traffic_gat(monkeypatch):
    """GAT variant, 6 epochs: halo_exchange in layers 1 and 2, the split
    block's per-epoch halo edge set and gat_rows_halo prefetched on the
    side stream."""
    _stream_runs(monkeypatch, "gat", 6)
