"""GPU (MI355X): --agg-dtype bf16 — the cast kernel, the bf16-source forms
of the per-row, narrow and row-group SpMM kernels, the bf16-source pack,
the partition path and a whole training step with the flag on.

Oracles and tolerances are in tests/agg_bf16_checks.py: float64 on
torch-rounded inputs under the unchanged fp32 summation bound, bit
equality for the cast and the pack, and for training steps the measured
fp32-vs-float64 rule with its floor at one bf16 ulp plus a call spy that
shows every aggregation SpMM got a bf16 source.

Run on the GPU box:
  python -m pytest tests/test_gpu_agg_bf16.py -m gpu -x -q
"""
import pytest
import torch

import agg_bf16_checks as A

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


# ---------------------------------------------------------------- 1. cast

@needs_gpu
def test_cast_bf16_equals_torch_cpu_cast_bitwise():
    """cast_bf16 against x.to(torch.bfloat16) on the CPU through
    .view(torch.int16): ties both ways and their neighbours, +-0, +-inf,
    NaN (compared with isnan), denormals, 0x7f7fffff -> inf; random
    [257, 44], [3, 5] (tail path) and [0, 8]; an unaligned view."""
    A.check_cast()


# -------------------------------------------------------- 2. kernel sweep

@needs_gpu
@pytest.mark.parametrize("F", A.SWEEP_F + A.FALLBACK_F)
def test_bf16_source_spmm_sweep(F):
    """bf16-source spmm_sum_raw on the kernel fixture and its transpose,
    with/without scales, overwrite from NaN-prefilled memory and out=
    accumulate: float64 reference on x.bfloat16().double() under
    assert_sum_bound (an fp32 aggregation of the unrounded x misses it on
    most elements), empty rows exactly 0, and within 2^-8 * agg(|x|) of —
    but not equal to — the fp32-source result. F = 6 and 5 take the
    upcast fallback: the same numbers from the fp32 kernels."""
    A.check_sweep(F)


# ------------------------------------------------------------- 3. grouped

@needs_gpu
@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("name", A.GROUPED_GRAPHS)
def test_bf16_source_grouped_sweep(name, R):
    """Row-group kernel with a bf16 source: gseg 1, 65 and the default,
    widths 132, 256, 260, 516 (one and two float4 per lane, with and
    without a row tail), every variant routed to the grouped binding."""
    A.check_grouped_sweep(name, R)


@needs_gpu
@pytest.mark.parametrize("R", [4, 8])
def test_bf16_source_grouped_isolation(R):
    """An inf / NaN source row survives the cast and reaches only the row
    that has an edge to it."""
    A.check_grouped_isolation(R)


# --------------------------------------------------------- 4. determinism

@needs_gpu
@pytest.mark.parametrize("F", [44, 256])
def test_bf16_source_per_row_deterministic(F):
    A.check_deterministic_per_row(F)


@needs_gpu
@pytest.mark.parametrize("R", [4, 8])
def test_bf16_source_grouped_deterministic(R):
    """F = 256; the grouped kernel does not cover F = 44."""
    A.check_deterministic_grouped(R)


# ---------------------------------------------------------------- 5. pack

@needs_gpu
@pytest.mark.parametrize("F", [1, 4, 30, 44])
def test_bf16_source_pack_rows_exact(F):
    A.check_pack(F)


# ------------------------------------------------------ 6. partition path

@needs_gpu
@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("F", [16, 44])
@pytest.mark.parametrize("mode", ["gcn", "mean"])
def test_partition_aggregate_bf16_matches_float64(monkeypatch, mode, F,
                                                  with_rows):
    A.check_partition_aggregate(mode, F, with_rows, monkeypatch)


# ------------------------------------------------------- 7. training step

@needs_gpu
@pytest.mark.parametrize("rank", [0, 1, 2])
@pytest.mark.parametrize("model,use_pp", [("graphsage", True),
                                          ("graphsage", False),
                                          ("gcn", True), ("gcn", False)])
def test_training_step_agg_bf16(model, use_pp, rank):
    """One training step and the eval-mode forward of one rank of the
    3-partition fixture with args.agg_dtype = "bf16": every tensor against
    the float64 CPU run within max(8 * e32, 2^-8); every inner-CSR SpMM of
    aggregate got a bf16 source, none did in the fp32 run of the same
    step, and the use_pp precompute stayed fp32."""
    A.check_training_step(model, use_pp, rank)
