"""GPU (MI355X): --gat-attn v2 — the GATv2 score kernel and its backward in
both directions against float64 ops/reference.py on the same fp32 inputs
(any-order summation bound of tests/kernel_path_checks.py), and a whole
training step with the flag on.

Run on the GPU box: python -m pytest tests/test_gpu_gatv2.py -m gpu -x -q
"""
import pytest
import torch

import kernel_path_checks as K
import partition_path_checks as P
from kernel_path_checks import N_COLS, N_ROWS, cu, dbl, degrees, gen

from bnsgcn_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

SLOPE = 0.2
# one lane per head | power-of-two group | group of 3 lanes (general form) |
# general form, 25 lanes per head straddling | two slots per lane | four
SHAPES = [(1, 4), (4, 8), (2, 12), (3, 100), (4, 128), (8, 128)]


def inputs(H, D):
    g = gen(9000 + 10 * H + D)
    return (torch.randn(N_COLS, H, D, generator=g),
            torch.randn(N_ROWS, H, D, generator=g),
            torch.randn(H, D, generator=g),
            torch.randn(K.fixture_csr()[1].numel(), H, generator=g))


@needs_gpu
@pytest.mark.parametrize("H,D", SHAPES)
def test_gatv2_score_forward(H, D):
    from bnsgcn_amd.ops.functional import gatv2_score_raw
    indptr, indices = K.fixture_csr()
    zs, zd, attn, _ = inputs(H, D)
    want = ref.gatv2_score(indptr, indices, dbl(zs), dbl(zd), dbl(attn), SLOPE)
    # sum_d |attn| (|zs| + |zd|): every s is positive on absolute values
    want_abs = ref.gatv2_score(indptr, indices, dbl(zs).abs(), dbl(zd).abs(),
                               dbl(attn).abs(), SLOPE)
    got = gatv2_score_raw(cu(indptr), cu(indices), cu(zs), cu(zd), cu(attn),
                          SLOPE)
    K.assert_sum_bound(got, want, want_abs, float(D),
                       f"gatv2_score (H,D)=({H},{D})")


@needs_gpu
@pytest.mark.parametrize("seg", [512, 4])
@pytest.mark.parametrize("H,D", SHAPES)
def test_gatv2_score_backward(H, D, seg):
    """d zd and d attn on the forward CSR, d zs on the transposed one with
    the permutation fused (hub column: a split row there too). Rows without
    an edge are exactly zero behind a NaN-filled allocation; d attn of two
    calls is bitwise equal. seg = 4 splits almost every row (atomic
    combine) and gives 200+ blocks: the d attn column sum then runs over
    two chunks of partial rows, the second one ragged."""
    from bnsgcn_amd.ops.csr_torch import build_worklist, transpose_csr
    from bnsgcn_amd.ops.functional import gatv2_score_bwd_raw
    indptr, indices = K.fixture_csr()
    zs, zd, attn, g = inputs(H, D)
    ip, ix = cu(indptr), cu(indices)
    tip, tix, eperm = transpose_csr(ip, ix, N_COLS)
    for t in (ip, tip):
        t._bns_worklist = build_worklist(t, seg=seg)
    assert (ip._bns_worklist[3].numel() - 1) // 4 > 128 or seg == 512
    tip_c, tix_c, ep_c = tip.cpu(), tix.cpu(), eperm.cpu()
    assert degrees(tip_c).max() > 512
    tag = f"gatv2_score_bwd (H,D)=({H},{D})"

    def run(csr, perm, z_res, z_str, want_dattn):
        junk = torch.full(z_res.shape, float("nan"), device=K.DEV)
        torch.cuda.synchronize()
        del junk
        return gatv2_score_bwd_raw(*csr, perm, cu(g), cu(z_res), cu(z_str),
                                   cu(attn), SLOPE, want_dattn=want_dattn)

    def oracle(csr, perm, z_res, z_str, fn):
        return ref.gatv2_score_backward(*csr, fn(dbl(g)), fn(dbl(z_res)),
                                        fn(dbl(z_str)), fn(dbl(attn)), SLOPE,
                                        perm)

    fwd, bwd = (indptr, indices), (tip_c, tix_c)
    dzd, dattn = run((ip, ix), None, zd, zs, True)
    want, want_attn = oracle(fwd, None, zd, zs, lambda t: t)
    w_abs, w_attn_abs = oracle(fwd, None, zd, zs, torch.abs)
    deg = degrees(indptr)
    K.assert_sum_bound(dzd, want, w_abs, deg[:, None, None], tag + " dzd")
    assert (dzd.cpu()[deg == 0] == 0).all(), f"{tag}: empty rows"
    K.assert_sum_bound(dattn, want_attn, w_attn_abs, float(indices.numel()),
                       tag + " dattn")
    assert torch.equal(run((ip, ix), None, zd, zs, True)[1], dattn)

    dzs, none = run((tip, tix), eperm, zs, zd, False)
    assert none is None
    want = oracle(bwd, ep_c, zs, zd, lambda t: t)[0]
    w_abs = oracle(bwd, ep_c, zs, zd, torch.abs)[0]
    tdeg = degrees(tip_c)
    K.assert_sum_bound(dzs, want, w_abs, tdeg[:, None, None], tag + " dzs")
    assert (dzs.cpu()[tdeg == 0] == 0).all(), f"{tag}: empty columns"


@needs_gpu
def test_gatv2_score_rejects_unbuilt_shapes():
    from bnsgcn_amd.ops.functional import gatv2_score_raw
    ip, ix = (cu(t) for t in K.fixture_csr())
    for H, D, msg in ((2, 6, "D % 4"), (4, 512, "1024")):
        with pytest.raises(RuntimeError, match=msg):
            gatv2_score_raw(ip, ix, torch.zeros(N_COLS, H, D, device=K.DEV),
                            torch.zeros(N_ROWS, H, D, device=K.DEV),
                            torch.zeros(H, D, device=K.DEV), SLOPE)


@needs_gpu
@pytest.mark.parametrize("rank", [0, 1, 2])
@pytest.mark.parametrize("use_pp", [True, False])
def test_training_step_gatv2(use_pp, rank):
    """One training step and the eval forward of one rank of the
    3-partition fixture with args.gat_attn = "v2" (split inner/halo sets,
    restricted final layer, padded class count) against the CPU float64 /
    fp32 runs; logits differ from the v1 step's."""
    g, parts = P.fixture_parts(3)
    args = P.step_args("gat", use_pp)
    assert args.gat_attn == "v1"
    plain = P.run_training_step(parts[rank], g, args, K.DEV, torch.float32)
    args.gat_attn = "v2"
    ref64 = P.run_training_step(parts[rank], g, args, "cpu", torch.float64)
    ref32 = P.run_training_step(parts[rank], g, args, "cpu", torch.float32)
    got = P.run_training_step(parts[rank], g, args, K.DEV, torch.float32)
    assert g.n_class % 4 != 0
    P.compare_measured(ref64, ref32, got,
                       f"gatv2 step use_pp={use_pp} rank {rank}")
    assert not torch.equal(got["logits"], plain["logits"])
