"""GPU (MI355X): --gat-dtype bf16 — the bf16-source forms of spmm_edge and
sddmm_dot, and a whole GAT training step with the flag on.

The rule: the gathered operand is rounded once to bf16 (round to nearest
even); weights, g, sums and outputs stay fp32. bf16 -> fp32 is exact, so
the oracle is float64 ops/reference.py on x.bfloat16().double() under the
unchanged fp32 summation bound of tests/kernel_path_checks.py, and the
same reference on the UNROUNDED x must miss that bound somewhere.

Run on the GPU box:
  python -m pytest tests/test_gpu_gat_bf16.py -m gpu -x -q
"""
import pytest
import torch

import agg_bf16_checks as A
import kernel_path_checks as K
import partition_path_checks as P
from kernel_path_checks import N_COLS, N_ROWS, cu, dbl, degrees, gen

from bnsgcn_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

BF16 = torch.bfloat16
# V = 8 one full slot | V = 8, NS = 2, sddmm fast at H * D = 1024 | 66 slots
# (second slot with a tail), sddmm general form | S < 64, H not a power of
# two | one lane per head | V = 4 | upcast fallback
SHAPES = [(4, 128), (8, 128), (2, 264), (3, 24), (4, 8), (1, 100), (2, 6)]


def check_edge(indptr, indices, w, x32, tag, wperm=None, base=None):
    """One bf16-source spmm_edge_raw call against float64 on the rounded x;
    the float64 result on the unrounded x must be outside the bound."""
    from bnsgcn_amd.ops.functional import round_bf16_raw, spmm_edge_raw
    ip_c, ix_c = indptr.cpu(), indices.cpu()
    deg = degrees(ip_c)[:, None, None]
    wd = dbl(w) if wperm is None else dbl(w)[wperm.cpu()]
    xq = x32.to(BF16).double()
    want = ref.spmm_edge_sum(ip_c, ix_c, wd, xq)
    want_abs = ref.spmm_edge_sum(ip_c, ix_c, wd.abs(), xq.abs())
    full = ref.spmm_edge_sum(ip_c, ix_c, wd, dbl(x32))
    if base is not None:
        want, full = want + dbl(base), full + dbl(base)
        want_abs = want_abs + dbl(base).abs()
    else:
        A._nan_junk(*want.shape)
    xb = round_bf16_raw(cu(x32))
    assert xb.dtype == BF16
    got = spmm_edge_raw(cu(ip_c), cu(ix_c), cu(w), xb, wperm=wperm,
                        out=None if base is None else cu(base).clone())
    assert got.dtype == torch.float32
    K.assert_sum_bound(got, want, want_abs, deg, tag)
    if base is None:
        assert (got.cpu()[degrees(ip_c) == 0] == 0).all(), f"{tag}: empty rows"
    miss = (got.double().cpu() - full).abs() > (deg + 8.0) * K.EPS * want_abs
    assert miss.any(), f"{tag}: within the bound of the unrounded x"


@needs_gpu
@pytest.mark.parametrize("H,D", SHAPES)
def test_spmm_edge_bf16_source(H, D):
    """Forward, out= accumulate, the wperm transposed form (split hub row)
    and wperm with out=, on the kernel fixture."""
    from bnsgcn_amd.ops.csr_torch import transpose_csr
    indptr, indices = K.fixture_csr()
    g = gen(8000 + 10 * H + D)
    w = torch.randn(indices.numel(), H, generator=g)
    x = torch.randn(N_COLS, H, D, generator=g)
    gy = torch.randn(N_ROWS, H, D, generator=g)
    base = torch.randn(N_ROWS, H, D, generator=g)
    base_t = torch.randn(N_COLS, H, D, generator=g)
    tag = f"bf16 spmm_edge (H,D)=({H},{D})"
    check_edge(indptr, indices, w, x, tag)
    check_edge(indptr, indices, w, x, tag + " out=", base=base)
    tip, tix, eperm = transpose_csr(cu(indptr), cu(indices), N_COLS)
    assert degrees(tip.cpu()).max() > 512
    check_edge(tip, tix, w, gy, tag + " wperm", wperm=eperm)
    check_edge(tip, tix, w, gy, tag + " wperm out=", wperm=eperm, base=base_t)


@needs_gpu
@pytest.mark.parametrize("H,D", SHAPES)
def test_sddmm_dot_bf16_source(H, D):
    """g fp32, x bf16: float64 on the rounded x, n_terms = D."""
    from bnsgcn_amd.ops.functional import round_bf16_raw, sddmm_dot_raw
    indptr, indices = K.fixture_csr()
    g = gen(8100 + 10 * H + D)
    a = torch.randn(N_ROWS, H, D, generator=g)
    x = torch.randn(N_COLS, H, D, generator=g)
    xq = x.to(BF16).double()
    want = ref.sddmm_dot(indptr, indices, dbl(a), xq)
    want_abs = ref.sddmm_dot(indptr, indices, dbl(a).abs(), xq.abs())
    full = ref.sddmm_dot(indptr, indices, dbl(a), dbl(x))
    A._nan_junk(*want.shape)
    got = sddmm_dot_raw(cu(indptr), cu(indices), cu(a), round_bf16_raw(cu(x)))
    assert got.dtype == torch.float32
    tag = f"bf16 sddmm_dot (H,D)=({H},{D})"
    K.assert_sum_bound(got, want, want_abs, float(D), tag)
    miss = (got.double().cpu() - full).abs() > (D + 8.0) * K.EPS * want_abs
    assert miss.any(), f"{tag}: within the bound of the unrounded x"


@needs_gpu
@pytest.mark.parametrize("rank", [0, 1, 2])
@pytest.mark.parametrize("use_pp", [True, False])
def test_training_step_gat_bf16(use_pp, rank):
    """One training step and the eval forward of one rank of the
    3-partition fixture with args.gat_dtype = "bf16": every tensor against
    the float64 CPU run of the same args within max(8 * e32, 2^-8), and
    logits that differ from the fp32 step's (the flag is live)."""
    g, parts = P.fixture_parts(3)
    args = P.step_args("gat", use_pp)
    assert args.gat_dtype == "fp32"
    plain = P.run_training_step(parts[rank], g, args, K.DEV, torch.float32)
    args.gat_dtype = "bf16"
    ref64 = P.run_training_step(parts[rank], g, args, "cpu", torch.float64)
    ref32 = P.run_training_step(parts[rank], g, args, "cpu", torch.float32)
    got = P.run_training_step(parts[rank], g, args, K.DEV, torch.float32)
    A.compare_measured_floor(ref64, ref32, got,
                             f"gat bf16 step use_pp={use_pp} rank {rank}")
    assert not torch.equal(got["logits"], plain["logits"])
