"""CPU (gloo) tests of --agg-dtype bf16: the flag and its environment
default, the GAT refusal, the CPU form of the rule (rounded values carried
in the tensor's own dtype, so a float64 run is a float64 oracle), the
straight-through gradient, and whole training runs on the tiny dataset:
distributed == single process at p = 1.0 under bf16 aggregation, and bf16
close to fp32 at p = 0.5.
"""
import numpy as np
import pytest
import torch

import agg_bf16_checks as A
import kernel_path_checks as K
import test_train_cpu as T
from kernel_path_checks import N_COLS, N_ROWS, assert_sum_bound, degrees, gen

from bnsgcn_amd.ops import reference as ref
from bnsgcn_amd.runtime.config import agg_dtype_of, create_parser

BF16 = torch.bfloat16


# ------------------------------------------------------------------ flag

def test_parser_default_is_fp32(monkeypatch):
    monkeypatch.delenv("BNSGCN_AGG_DTYPE", raising=False)
    args = create_parser().parse_args([])
    assert args.agg_dtype == "fp32"
    assert agg_dtype_of(args) is None
    for flag in ("--agg-dtype", "--agg_dtype"):
        args = create_parser().parse_args([flag, "bf16"])
        assert args.agg_dtype == "bf16" and agg_dtype_of(args) == BF16
    with pytest.raises(SystemExit):
        create_parser().parse_args(["--agg-dtype", "fp16"])


def test_env_default_is_picked_up(monkeypatch):
    monkeypatch.setenv("BNSGCN_AGG_DTYPE", "bf16")
    assert create_parser().parse_args([]).agg_dtype == "bf16"
    assert create_parser().parse_args(["--agg-dtype", "fp32"]).agg_dtype \
        == "fp32"


def test_gat_with_bf16_raises(tmp_path):
    args = create_parser().parse_args(["--model", "gat", "--agg-dtype",
                                       "bf16"])
    with pytest.raises(ValueError, match="agg-dtype"):
        agg_dtype_of(args)
    # and at start-up of a run, before any work
    from bnsgcn_amd.runtime.trainer import run
    args = T.make_args(tmp_path, model="gat", agg_dtype="bf16",
                       n_partitions=1)
    with pytest.raises(ValueError, match="agg-dtype"):
        run(args, rank=0, world_size=1)
    args.model = "gcn"
    assert agg_dtype_of(args) == BF16


def test_context_default_changes_nothing():
    """GraphContext.agg_dtype defaults to None, and None / fp32 give the
    result of the plain call bit for bit."""
    from bnsgcn_amd.ops.csr_torch import transpose_csr
    from bnsgcn_amd.ops.functional import spmm_sum
    indptr, indices = K.fixture_csr()
    tip, tix, _ = transpose_csr(indptr, indices, N_COLS)
    x = torch.randn(N_COLS, 12, generator=gen(7000))
    plain = spmm_sum(x, indptr, indices, tip, tix)
    for dt in (None, torch.float32):
        assert torch.equal(spmm_sum(x, indptr, indices, tip, tix,
                                    src_dtype=dt), plain)
    assert not torch.equal(spmm_sum(x, indptr, indices, tip, tix,
                                    src_dtype=BF16), plain)
    with pytest.raises(ValueError):
        spmm_sum(x, indptr, indices, tip, tix, src_dtype=torch.float16)


# ------------------------------------------------------------------ rule

def test_round_bf16_raw_cpu_carries_dtype():
    from bnsgcn_amd.ops.functional import round_bf16_raw
    v = A.crafted_rows()
    v = v[~torch.isnan(v)]
    for dt in (torch.float32, torch.float64):
        got = round_bf16_raw(v.to(dt))
        assert got.dtype == dt
        assert torch.equal(got, v.to(BF16).to(dt))
    # ties to even, and the largest finite fp32 rounds to inf
    one = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.4028234e38])
    assert round_bf16_raw(one).tolist() == [1.0, 1 + 2.0 ** -6, float("inf")]


@pytest.mark.parametrize("F", [5, 12, 44])
def test_spmm_sum_cpu_follows_the_rule(F):
    """spmm_sum(..., src_dtype=bf16) on the CPU, float64 and fp32, against
    the oracle of the GPU sweep — float64 ops/reference.py on
    x.bfloat16().double() — and the straight-through gradient: the
    transposed product of the rounded g."""
    from bnsgcn_amd.ops.csr_torch import transpose_csr
    from bnsgcn_amd.ops.functional import spmm_sum
    indptr, indices = K.fixture_csr()
    tip, tix, _ = transpose_csr(indptr, indices, N_COLS)
    g_ = gen(7100 + F)
    x = torch.randn(N_COLS, F, generator=g_)
    gy = torch.randn(N_ROWS, F, generator=g_)
    ss = torch.rand(N_COLS, generator=g_) + 0.5
    ds = torch.rand(N_ROWS, generator=g_) + 0.5
    xq, gq = x.to(BF16).double(), gy.to(BF16).double()
    want = ref.spmm_sum(indptr, indices, xq, ss.double(), ds.double())
    want_abs = ref.spmm_sum(indptr, indices, xq.abs(), ss.double(),
                            ds.double())
    want_gx = ref.spmm_sum(tip, tix, gq, ds.double(), ss.double())
    abs_gx = ref.spmm_sum(tip, tix, gq.abs(), ds.double(), ss.double())
    for dt in (torch.float64, torch.float32):
        xd = x.to(dt).requires_grad_(True)
        y = spmm_sum(xd, indptr, indices, tip, tix, ss.to(dt), ds.to(dt),
                     src_dtype=BF16)
        y.backward(gy.to(dt))
        assert y.dtype == dt and xd.grad.dtype == dt
        if dt == torch.float64:
            torch.testing.assert_close(y.detach(), want, rtol=1e-13, atol=0)
            torch.testing.assert_close(xd.grad, want_gx, rtol=1e-13, atol=0)
        else:
            assert_sum_bound(y, want, want_abs, degrees(indptr)[:, None],
                             f"cpu fp32 forward F={F}")
            assert_sum_bound(xd.grad, want_gx, abs_gx,
                             degrees(tip)[:, None], f"cpu fp32 backward F={F}")


@pytest.mark.parametrize("F", [4, 44, 256])
def test_oracle_separates_rounded_from_unrounded(F):
    """Why the GPU sweep fails when the flag is ignored: an fp32 reference
    on rounded inputs sits well inside the bound, an fp32 aggregation of
    the unrounded input misses it on most non-empty elements."""
    ok, miss = A.cpu_oracle_figures(F)
    print(f"F={F}: rounded err/bound {ok:.3g}, unrounded miss {miss:.2%}")
    assert ok < 0.5
    assert miss > 0.5


# ------------------------------------------------------- training, gloo

def _losses(res):
    return sum(np.array(r["loss_history"]) for r in res)


@pytest.mark.parametrize("model,use_pp", [("graphsage", False),
                                          ("graphsage", True),
                                          ("gcn", False), ("gcn", True)])
def test_dist_matches_single_at_full_rate_bf16(tmp_path, model, use_pp):
    """At p = 1.0 the pack scale is 1 and the halo rows are q(x) itself, so
    the 2-rank job aggregates exactly the terms of the single process."""
    kw = dict(model=model, use_pp=use_pp, sampling_rate=1.0, agg_dtype="bf16")
    single = T._run_config(tmp_path / "s", 1, **kw)
    multi = T._run_config(tmp_path / "m", 2, **kw)
    lh_single, lh_multi = _losses(single), _losses(multi)
    print("worst rel diff", float(np.abs(lh_multi / lh_single - 1).max()))
    np.testing.assert_allclose(lh_multi, lh_single, rtol=2e-3, atol=1e-3)
    assert lh_single[-1] < lh_single[0]


@pytest.mark.parametrize("model", ["graphsage", "gcn"])
def test_bf16_aggregation_close_to_fp32(tmp_path, model):
    kw = dict(model=model, sampling_rate=0.5, use_pp=True, n_epochs=10)
    a = _losses(T._run_config(tmp_path / "a", 2, **kw))
    b = _losses(T._run_config(tmp_path / "b", 2, agg_dtype="bf16", **kw))
    print("worst rel diff", float(np.abs(b / a - 1).max()))
    np.testing.assert_allclose(b, a, rtol=0.05)
    assert not np.array_equal(a, b)
    assert b[-1] < b[0]
