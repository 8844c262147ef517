"""GPU (MI355X): the edge-parallel narrow-F SpMM (spmm_sum_narrow_kernel,
F % 4 == 0 and F <= 64) and the project-then-aggregate layers on it.

Kernel oracle and tolerance: kernel_path_checks.py — float64
ops/reference.py on the same fp32 inputs under the any-order summation
bound. Layer oracle: the aggregate-first formula in float64 on the CPU
under the measured-tolerance rule of partition_path_checks.compare_measured
(see project_first_checks.py).

Run on the GPU box: python -m pytest tests/test_gpu_narrow_spmm.py -m gpu -x -q
"""
import os
import subprocess
import sys

import pytest
import torch

import kernel_path_checks as K
import narrow_spmm_checks as N
import partition_path_checks as P
import project_first_checks as L
from kernel_path_checks import cu, gen

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


@needs_gpu
@pytest.mark.parametrize("F", [4, 8, 12, 44, 48, 60, 64, 68])
def test_narrow_spmm_fixture(F):
    """f4 = 1 (one lane per 16-lane group), 2, 3, 11 (the benchmark's 44),
    12, 15 and 16 (a full group) on the narrow kernel, and F = 68, where
    the routing hands over to the half-wave kernel: the fixture CSR (empty
    rows, rows of 1/64/65/128/512 edges, 5 atomic items) with and without
    scales and accumulation, as test_spmm_sum_fixture runs it."""
    for scales, acc in N.COMBOS:
        K.check_spmm_sum(F, scales, acc, nan_prefill=not acc)


@needs_gpu
@pytest.mark.parametrize("F", [4, 8, 12, 44, 48, 60, 64, 68])
def test_narrow_spmm_transposed_fixture(F):
    """The same on the transposed fixture CSR (the backward's path; the
    hub column is a row split into atomic items)."""
    for scales, acc in N.COMBOS:
        N.check_spmm_sum_transposed(F, scales, acc)


@needs_gpu
@pytest.mark.parametrize("F", [44, 64])
def test_narrow_spmm_deterministic_without_atomics(monkeypatch, F):
    """With SEG above every degree no item is atomic; the wave's own
    summation order and the fixed __shfl_xor combine then make two calls
    bitwise equal."""
    from bnsgcn_amd.ops import csr_torch
    from bnsgcn_amd.ops.functional import _worklist_of, spmm_sum_raw
    monkeypatch.setattr(csr_torch, "SEG", 1 << 20)
    for indptr, indices, n_src in ((*K.fixture_csr(), K.N_COLS),
                                   (*N.transposed_fixture_csr(), K.N_ROWS)):
        ip, ix = cu(indptr), cu(indices)
        assert (_worklist_of(ip)[0] >= 0).all()        # no atomic item
        g = gen(170 + F)
        x = cu(torch.randn(n_src, F, generator=g))
        ss = cu(torch.rand(n_src, generator=g) + 0.5)
        ds = cu(torch.rand(indptr.numel() - 1, generator=g) + 0.5)
        a = spmm_sum_raw(ip, ix, x, ss, ds)
        b = spmm_sum_raw(ip, ix, x, ss, ds)
        assert torch.equal(a, b)
        assert a.abs().sum() > 0


@needs_gpu
def test_narrow_max_zero_in_child_process():
    """BNSGCN_SPMM_NARROW_MAX=0 sends F in {44, 64} through the half-wave
    kernel again. The extension reads the switch once per process, so the
    variant runs in a fresh child, with a timeout."""
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "narrow_spmm_checks.py")
    for case, (env_add, _) in N.CASES.items():
        env = dict(os.environ, **env_add)
        r = subprocess.run([sys.executable, helper, case], env=env,
                           timeout=180, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        print(r.stdout)
        assert r.returncode == 0, (
            f"child '{case}' exited {r.returncode}:\n{r.stdout[-4000:]}")


@needs_gpu
@pytest.mark.parametrize("kind", ["sage", "gcn"])
def test_project_first_layer_train_rows_gpu(kind):
    """A (64, 41) layer on every rank of the 3-partition fixture, rows =
    the rank's train rows, sampled halo non-empty: the GPU forward and
    backward (projection GEMM, narrow SpMM at F = 44 with the halo SpMM
    accumulating into it, the transposed narrow SpMM, scatter_add_rows)
    against the aggregate-first formula in float64 on the CPU. e32 is the
    fp32 CPU run of that formula against float64; the GPU may differ from
    float64 by max(8 * e32, 1e-5)."""
    _, parts = P.fixture_parts(3)
    for part in parts:
        case = L.Case(kind, 64, 41, "partition", True, rank=part.rank)
        ref64 = L.run(case, "agg_first", "cpu", torch.float64)
        ref32 = L.run(case, "agg_first", "cpu", torch.float32)
        got = L.run(case, "layer", P.DEV, torch.float32)
        assert got.pop("agg width") == 44
        ref64.pop("agg width"), ref32.pop("agg width")
        P.compare_measured(ref64, ref32, got, f"{kind} rank {part.rank}")
