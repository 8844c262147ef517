"""Autograd-wired compute ops with CPU(torch-reference) / GPU(HIP) dispatch.

Each op dispatches per-tensor-device: CPU → ops/reference.py; CUDA(HIP) →
the gfx950 extension (required — no silent eager fallback on GPU, see
ops/_ext.py). Backward passes reuse the same primitives on precomputed
transposed CSRs, so one kernel family serves both directions
(reference counterparts: SURVEY.md §2.3 K1-K6, K13-K14).
"""
from __future__ import annotations

import torch
from torch.autograd import Function

from . import reference as ref
from ._ext import get_ext, use_hip


# ---------------------------------------------------------------- raw ops

def _worklist_of(indptr):
    """Edge-balanced work list for the device SpMM (csr_torch.build_worklist),
    cached on the indptr tensor itself (same lifetime as the CSR). A
    contiguous int64 indptr on the GPU gets it from the device builder
    (csr_torch.build_worklist_hip, the same tensors) while csr_torch.PLAN_HIP
    is on; SEG and MAX_WAVES are read at call time either way."""
    wl = getattr(indptr, "_bns_worklist", None)
    if wl is None:
        from . import csr_torch
        if (csr_torch.plan_hip(indptr) and indptr.dtype == torch.int64
                and indptr.is_contiguous()):
            wl = csr_torch.build_worklist_hip(indptr)
        else:
            wl = csr_torch.build_worklist(indptr)
        indptr._bns_worklist = wl
    return wl


import os as _os

# Row-group SpMM (csr_torch.build_rowgroups + spmm_sum_grouped_kernel) for
# static CSRs. BNSGCN_SPMM_GROUP=0 turns the path off. The format is kept
# only when it asks for at most GROUP_TAU source-row reads per edge: above
# that the grouped kernel no longer beats the per-row one by more than the
# latter's repeat spread (profiles/BENCH_SUMMARY_rowgroup.md), and a graph
# without shared neighbours pays neither time nor memory.
_GROUP = _os.environ.get("BNSGCN_SPMM_GROUP", "1") != "0"
GROUP_TAU = float(_os.environ.get("BNSGCN_SPMM_GROUP_TAU", 0.6))
# The same rule for narrow calls (F / 4 <= 16, spmm_sum_grouped_narrow_kernel),
# measured on its own at F = 44 (profiles/BENCH_SUMMARY_narrowgroup.md): the
# grouped kernel wins on both CSRs up to the largest ratio below 0.9 that
# was measured, 0.66 (1.07x), and wins one CSR and ties the other at 0.92.
GROUP_TAU_NARROW = float(_os.environ.get("BNSGCN_SPMM_GROUP_TAU_NARROW", 0.7))
# GraphContext groups the TRANSPOSED inner CSR only (the backward SpMM).
# transpose_csr leaves its rows in ascending column order, which is the
# grouped kernel's summation order, and what the backward produces feeds
# no activation mask, so the step's results move by rounding alone. The
# forward CSR's rows are in edge order: grouping it re-orders every row's
# sum, the fused LayerNorm+ReLU after the layer then flips a few dozen of
# its 60M mask bits, and the gradients of a step move by up to 7e-4 of
# their largest element (profiles/BENCH_SUMMARY_rowgroup.md) — the size of
# the per-row path's own run-to-run change when a hub row's atomics land
# in another order, but on every run. BNSGCN_SPMM_GROUP_FWD=1 groups it too.
# The train-row-gathered forward CSR of the output layer carries a format
# for narrow calls only (its `wide` flag follows GROUP_FWD): a narrow
# result is the logits and feeds no mask.
GROUP_FWD = _os.environ.get("BNSGCN_SPMM_GROUP_FWD", "0") == "1"


def attach_rowgroups(indptr, indices, n_cols, wide=True, narrow=True):
    """Build the row-group form of a STATIC CSR, apply the keep rules and
    cache the result on the indptr tensor (`_bns_rowgroups`, lifetime of
    `_bns_worklist`). `wide` / `narrow` name the calls the caller allows on
    the format (F / 4 > 32, F / 4 <= 16); each is kept only below its own
    threshold, and the format is cached if either is. Returns the builder's
    entries/edges ratio, or None when the path is off or the CSR is not on
    the GPU."""
    if not (_GROUP and indptr.is_cuda):
        return None
    from .csr_torch import build_rowgroups
    rg = build_rowgroups(indptr, indices, n_cols)
    rg = rg._replace(wide=wide and rg.ratio <= GROUP_TAU,
                     narrow=narrow and rg.ratio <= GROUP_TAU_NARROW)
    keep = rg.wide or rg.narrow
    if keep:
        indptr._bns_rowgroups = rg
    if _os.environ.get("BNSGCN_SPMM_GROUP_LOG") == "1":
        print(f"rowgroup: R={rg.R} entries/edges {rg.ratio:.3f} "
              f"({indices.numel()} edges) -> "
              f"{'kept' if keep else 'dropped'}"
              f"{' wide' * rg.wide}{' narrow' * rg.narrow}", flush=True)
    return rg.ratio


def _grouped_route(rg, x):
    """True where spmm_sum_raw takes the row-group kernels: F % 4 == 0 and
    either F / 4 > 32 on a format kept for wide calls, or F / 4 <= 16 with
    an fp32 source on one kept for narrow calls (a bf16 source stays on
    the per-row narrow kernel). Widths F / 4 = 17 .. 32 have no grouped
    kernel."""
    if rg is None or x.shape[1] % 4:
        return False
    f4 = x.shape[1] // 4
    return (f4 > 32 and rg.wide) or (
        0 < f4 <= 16 and rg.narrow and x.dtype == torch.float32)


# Source-row reads a wave of the wide kernels (F / 4 > 32:
# spmm_sum_wide_kernel, spmm_sum_grouped_kernel) keeps in flight, per
# kernel family and source type: the depth the sweep of
# profiles/BENCH_SUMMARY_spmmdepth.md selected — 4 everywhere: with the
# chunk and item prefetch in place deeper windows gain 0-3 % on one graph
# and lose 1 % on another with an fp32 source, and a bf16 source gets
# slower with depth. Every depth computes the same sums in the same
# order. BNSGCN_SPMM_DEPTH forces one value for all four; a value the
# kernels are not built for means 4. Unlike the other knobs it is read on
# every spmm_sum_raw call, not once (tests set it per case), and it acts
# here only: a direct call of the extension's spmm_sum / spmm_sum_grouped
# gets the depth it passes, 4 by default.
SPMM_DEPTHS = (4, 8, 16)
SPMM_DEPTH_SWEPT = {("per_row", "fp32"): 4, ("per_row", "bf16"): 4,
                    ("grouped", "fp32"): 4, ("grouped", "bf16"): 4}


def spmm_depth(family, src_dtype):
    """Depth passed to the extension for `family` in {"per_row", "grouped"}
    and a source of torch dtype `src_dtype`."""
    forced = _os.environ.get("BNSGCN_SPMM_DEPTH")
    if forced is not None:
        try:
            depth = int(forced)
        except ValueError:
            depth = 4
        return depth if depth in SPMM_DEPTHS else 4
    name = "bf16" if src_dtype == torch.bfloat16 else "fp32"
    return SPMM_DEPTH_SWEPT[(family, name)]


def round_bf16_raw(x):
    """The source operand of --agg-dtype bf16: x rounded once to bf16,
    round to nearest even. On the GPU the HIP cast kernel returns a bf16
    tensor, which spmm_sum_raw / pack_rows_raw read at half the bytes. On
    the CPU the rounded values float(bf16(float32(x))) are carried in x's
    own dtype, so a float64 run is a float64 oracle of the same numbers."""
    if use_hip(x) and x.dtype == torch.float32:
        return get_ext().cast_bf16(x.contiguous())
    return x.float().bfloat16().to(x.dtype)


def spmm_sum_raw(indptr, indices, x, src_scale=None, dst_scale=None, out=None,
                 depth=None):
    """x may be a bf16 source (round_bf16_raw); the result is fp32 then.
    The bf16 kernels cover F % 4 == 0: other widths upcast the rounded
    copy and take the fp32 kernels — the same numbers, no byte saving.
    `depth` (4, 8 or 16) overrides spmm_depth for this call (tests,
    tools/spmm_micro); None means routed."""
    if x.dtype == torch.bfloat16 and not (use_hip(x) and x.shape[1] % 4 == 0):
        x = x.float()
    if use_hip(x):
        odt = torch.float32 if x.dtype == torch.bfloat16 else x.dtype
        rg = getattr(indptr, "_bns_rowgroups", None) if _GROUP else None
        if _grouped_route(rg, x):
            acc = out is not None
            if not acc:
                out = torch.empty(indptr.numel() - 1, x.shape[1],
                                  dtype=odt, device=x.device)
                if rg.zero_rows.numel():
                    out.index_fill_(0, rg.zero_rows, 0.0)
            return get_ext().spmm_sum_grouped(
                *rg.sched, rg.ecol, rg.ew, x, src_scale, dst_scale, out, acc,
                spmm_depth("grouped", x.dtype) if depth is None else depth)
        wrow, wbeg, wend, wave_start, zero_rows = _worklist_of(indptr)
        acc = out is not None
        if not acc:
            # allocate uninitialized and zero ONLY the rows the kernel does
            # not fully overwrite (split/atomic + empty rows)
            out = torch.empty(indptr.numel() - 1, x.shape[1],
                              dtype=odt, device=x.device)
            if zero_rows.numel():
                out.index_fill_(0, zero_rows, 0.0)
        return get_ext().spmm_sum(wrow, wbeg, wend, wave_start, indices, x,
                                  src_scale, dst_scale, out, acc,
                                  spmm_depth("per_row", x.dtype)
                                  if depth is None else depth)
    return ref.spmm_sum(indptr, indices, x, src_scale, dst_scale, out)


def _gat_src(x):
    """A bf16 source of the GAT kernels (round_bf16_raw of z or grad) as the
    kernels take it. The bf16 kernels cover D % 4 == 0 on the GPU: any other
    shape, or a CPU tensor, upcasts the rounded copy and takes the fp32
    path — the same numbers, no byte saving (as spmm_sum_raw does)."""
    if x.dtype == torch.bfloat16 and not (use_hip(x) and x.shape[2] % 4 == 0):
        return x.float()
    return x


def spmm_edge_raw(indptr, indices, eweight, x, out=None, wperm=None):
    """wperm: optional edge permutation applied to eweight INSIDE the HIP
    kernel (fuses the w[eperm] gather of the transposed backward pass).
    x may be a bf16 source (round_bf16_raw); the result is fp32 then."""
    x = _gat_src(x)
    if use_hip(x):
        wrow, wbeg, wend, wstart, zero_rows = _worklist_of(indptr)
        acc = out is not None
        if not acc:
            odt = torch.float32 if x.dtype == torch.bfloat16 else x.dtype
            out = torch.empty(indptr.numel() - 1, x.shape[1], x.shape[2],
                              dtype=odt, device=x.device)
            if zero_rows.numel():
                out.index_fill_(0, zero_rows, 0.0)
        return get_ext().spmm_edge_sum(wrow, wbeg, wend, wstart, indptr,
                                       indices, eweight.contiguous(), wperm,
                                       x.contiguous(), out, acc)
    ew = eweight if wperm is None else eweight[wperm]
    return ref.spmm_edge_sum(indptr, indices, ew, x, out)


def sddmm_dot_raw(indptr, indices, a_dst, b_src):
    """b_src (the streamed operand) may be a bf16 source; a_dst and the
    result are fp32."""
    b_src = _gat_src(b_src)
    if use_hip(a_dst):
        wl = _worklist_of(indptr)[:4]
        return get_ext().sddmm_dot(*wl, indptr, indices,
                                   a_dst.contiguous(), b_src.contiguous())
    return ref.sddmm_dot(indptr, indices, a_dst, b_src)


def sddmm_add_raw(indptr, indices, el_src, er_dst, slope=-1.0):
    """slope >= 0 fuses LeakyReLU into the kernel (HIP path); the torch
    path applies it separately."""
    if use_hip(el_src):
        wl = _worklist_of(indptr)[:4]
        return get_ext().sddmm_add(*wl, indptr, indices,
                                   el_src.contiguous(), er_dst.contiguous(),
                                   slope)
    out = ref.sddmm_add(indptr, indices, el_src, er_dst)
    if slope >= 0:
        out = torch.nn.functional.leaky_relu(out, slope)
    return out


def gatv2_score_raw(indptr, indices, zs, zd, attn, slope):
    """e[k,h] = Σ_d attn[h,d]·LeakyReLU(zs[col_k,h,d] + zd[row_k,h,d]) on
    the fused HIP gather kernel (fp32, D % 4 == 0, H·D <= 1024 — anything
    else raises there: no eager fallback on the GPU)."""
    if zd.shape[0] != indptr.numel() - 1:
        raise ValueError(f"gatv2_score: zd has {zd.shape[0]} rows, the CSR "
                         f"{indptr.numel() - 1}")
    if use_hip(zs):
        wl = _worklist_of(indptr)[:4]
        return get_ext().gatv2_score(*wl, indices, zs.contiguous(),
                                     zd.contiguous(), attn.contiguous(),
                                     float(slope))
    return ref.gatv2_score(indptr, indices, zs, zd, attn, slope)


def gatv2_score_bwd_raw(indptr, indices, eperm, g, z_res, z_str, attn, slope,
                        want_dattn=False):
    """Backward of gatv2_score for the operand indexed by the ROWS of the
    CSR given (ref.gatv2_score_backward): forward CSR with (z_res, z_str) =
    (zd, zs) for d zd, transposed CSR + its eperm with (zs, zd) for d zs.
    Returns (dz_res, dattn [H, D] or None)."""
    if z_res.shape[0] != indptr.numel() - 1:
        raise ValueError(f"gatv2_score_bwd: z_res has {z_res.shape[0]} rows, "
                         f"the CSR {indptr.numel() - 1}")
    if use_hip(g):
        ret = get_ext().gatv2_score_bwd(
            *_worklist_of(indptr), indices, eperm, g.contiguous(),
            z_res.contiguous(), z_str.contiguous(), attn.contiguous(),
            float(slope), want_dattn)
        return ret[0], (ret[1] if want_dattn else None)
    dz, dattn = ref.gatv2_score_backward(indptr, indices, g, z_res, z_str,
                                         attn, slope, eperm)
    return dz, (dattn if want_dattn else None)


def segment_softmax_raw(indptr, logits):
    if use_hip(logits):
        return get_ext().segment_softmax(indptr, logits)
    return ref.segment_softmax(indptr, logits)


def segment_softmax_bwd_raw(indptr, alpha, grad_alpha):
    if use_hip(alpha):
        return get_ext().segment_softmax_backward(indptr, alpha, grad_alpha)
    return ref.segment_softmax_backward(indptr, alpha, grad_alpha)


def pack_rows_raw(x, idx, scale=None):
    """A bf16 x (round_bf16_raw) packs to fp32 rows float(x[idx]) * scale."""
    if use_hip(x):
        return get_ext().pack_rows(x, idx, scale)
    if x.dtype == torch.bfloat16:
        x = x.float()
    return ref.pack_rows(x, idx, scale)


def scatter_add_rows_raw(out, idx, src, scale=None):
    if use_hip(out):
        get_ext().scatter_add_rows(out, idx, src, scale)
        return out
    return ref.scatter_add_rows(out, idx, src, scale)


# ----------------------------------------------------------- autograd ops

class _SpMMSum(Function):
    """y[r] = dst_scale[r] * Σ_{c∈row r} src_scale[c] * x[c]  (K1/K2 + K18).

    Backward runs the SAME kernel on the precomputed transposed CSR with the
    scale roles swapped — no atomics anywhere (SURVEY.md §7 'per-epoch block
    assembly' design).

    src_dtype=torch.bfloat16 (--agg-dtype bf16) rounds the source operand
    once to bf16 in both directions — x in forward, grad in backward
    (straight-through: the rounding has derivative 1). Scales, products,
    accumulation and the result stay fp32."""

    @staticmethod
    def forward(ctx, x, indptr, indices, indptr_t, indices_t, src_scale,
                dst_scale, src_dtype=None):
        ctx.save_for_backward(indptr_t, indices_t, src_scale, dst_scale)
        ctx.src_dtype = src_dtype
        if src_dtype == torch.bfloat16:
            x = round_bf16_raw(x)
        return spmm_sum_raw(indptr, indices, x, src_scale, dst_scale)

    @staticmethod
    def backward(ctx, grad):
        indptr_t, indices_t, src_scale, dst_scale = ctx.saved_tensors
        grad = grad.contiguous()
        if ctx.src_dtype == torch.bfloat16:
            grad = round_bf16_raw(grad)
        gx = spmm_sum_raw(indptr_t, indices_t, grad,
                          src_scale=dst_scale, dst_scale=src_scale)
        return gx, None, None, None, None, None, None, None


def check_src_dtype(src_dtype):
    if src_dtype not in (None, torch.float32, torch.bfloat16):
        raise ValueError(f"aggregation source dtype must be None, "
                         f"torch.float32 or torch.bfloat16, got {src_dtype}")
    return torch.bfloat16 if src_dtype == torch.bfloat16 else None


def spmm_sum(x, indptr, indices, indptr_t, indices_t,
             src_scale=None, dst_scale=None, src_dtype=None):
    return _SpMMSum.apply(x, indptr, indices, indptr_t, indices_t,
                          src_scale, dst_scale, check_src_dtype(src_dtype))


class _SpMMEdge(Function):
    """y[r,h] = Σ_{e∈row r} w[e,h] * x[col_e,h,:]  (GAT aggregate, K4/K5).

    src_dtype=torch.bfloat16 (--gat-dtype bf16) rounds the gathered operand
    once to bf16: x in forward, grad in the backward for x (straight-
    through). The backward for w streams the SAVED bf16 x against the fp32
    grad, so gw is the exact derivative of the rounded forward. Weights,
    accumulation and every result stay fp32."""

    @staticmethod
    def forward(ctx, x, w, indptr, indices, indptr_t, indices_t, eperm_t,
                src_dtype=None):
        ctx.src_dtype = src_dtype
        if src_dtype == torch.bfloat16:
            x = round_bf16_raw(x)
        ctx.save_for_backward(x, w, indptr, indices, indptr_t, indices_t, eperm_t)
        return spmm_edge_raw(indptr, indices, w, x)

    @staticmethod
    def backward(ctx, grad):
        x, w, indptr, indices, indptr_t, indices_t, eperm_t = ctx.saved_tensors
        grad = grad.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gsrc = round_bf16_raw(grad) \
                if ctx.src_dtype == torch.bfloat16 else grad
            gx = spmm_edge_raw(indptr_t, indices_t, w, gsrc, wperm=eperm_t)
        if ctx.needs_input_grad[1]:
            gw = sddmm_dot_raw(indptr, indices, grad, x)
        return gx, gw, None, None, None, None, None, None


def spmm_edge_sum(x, w, indptr, indices, indptr_t, indices_t, eperm_t,
                  src_dtype=None):
    return _SpMMEdge.apply(x, w, indptr, indices, indptr_t, indices_t, eperm_t,
                           check_src_dtype(src_dtype))


class _SpMMEdge2(Function):
    """Inner + halo GAT aggregation accumulated into ONE output buffer —
    removes the [N, H, D]-sized elementwise add between the two edge-set
    results (~5% of the Yelp GAT epoch in bare CUDAFunctor_add kernels,
    profiles/topk_gat2_r02.txt). src_dtype as in _SpMMEdge; one rounded
    copy of grad serves the inner and the halo backward."""

    @staticmethod
    def forward(ctx, x_in, w_in, x_h, w_h,
                ip, ix, tip, tix, eperm_t,
                hip_, hix_, hbip, hbix, heperm_t, src_dtype=None):
        ctx.src_dtype = src_dtype
        if src_dtype == torch.bfloat16:
            x_in, x_h = round_bf16_raw(x_in), round_bf16_raw(x_h)
        ctx.save_for_backward(x_in, w_in, x_h, w_h, ip, ix, tip, tix,
                              eperm_t, hip_, hix_, hbip, hbix, heperm_t)
        out = spmm_edge_raw(ip, ix, w_in, x_in)
        spmm_edge_raw(hip_, hix_, w_h, x_h, out=out)
        return out

    @staticmethod
    def backward(ctx, grad):
        (x_in, w_in, x_h, w_h, ip, ix, tip, tix, eperm_t,
         hip_, hix_, hbip, hbix, heperm_t) = ctx.saved_tensors
        grad = grad.contiguous()
        gx_in = gw_in = gx_h = gw_h = None
        gsrc = grad
        if ctx.src_dtype == torch.bfloat16 and (ctx.needs_input_grad[0]
                                                or ctx.needs_input_grad[2]):
            gsrc = round_bf16_raw(grad)
        if ctx.needs_input_grad[0]:
            gx_in = spmm_edge_raw(tip, tix, w_in, gsrc, wperm=eperm_t)
        if ctx.needs_input_grad[1]:
            gw_in = sddmm_dot_raw(ip, ix, grad, x_in)
        if ctx.needs_input_grad[2]:
            gx_h = spmm_edge_raw(hbip, hbix, w_h, gsrc, wperm=heperm_t)
        if ctx.needs_input_grad[3]:
            gw_h = sddmm_dot_raw(hip_, hix_, grad, x_h)
        return (gx_in, gw_in, gx_h, gw_h) + (None,) * 11


def spmm_edge_sum2(x_in, w_in, x_h, w_h, inner_csrs5, halo_csrs5,
                   src_dtype=None):
    """inner_csrs5 = (ip, ix, tip, tix, eperm_t); halo_csrs5 likewise."""
    return _SpMMEdge2.apply(x_in, w_in, x_h, w_h,
                            *inner_csrs5, *halo_csrs5,
                            check_src_dtype(src_dtype))


class _SDDMMAdd(Function):
    """logits[e,h] = [leaky_relu](el[col_e,h] + er[row_e,h])  (u_add_v
    SDDMM, optionally fused with the GAT LeakyReLU — the activation is
    monotonic with fixpoint 0, so the backward mask comes from the sign
    of the saved OUTPUT)."""

    @staticmethod
    def forward(ctx, el, er, indptr, indices, indptr_t, indices_t, eperm_t,
                slope):
        out = sddmm_add_raw(indptr, indices, el, er,
                            -1.0 if slope is None else float(slope))
        ctx.slope = slope
        if slope is not None:
            ctx.save_for_backward(indptr, indices, indptr_t, indices_t,
                                  eperm_t, out)
        else:
            ctx.save_for_backward(indptr, indices, indptr_t, indices_t,
                                  eperm_t)
        ctx.n_src, ctx.n_dst = el.shape[0], er.shape[0]
        return out

    @staticmethod
    def backward(ctx, grad):
        if ctx.slope is not None:
            indptr, indices, indptr_t, indices_t, eperm_t, out = ctx.saved_tensors
            grad = torch.where(out > 0, grad, grad * ctx.slope).contiguous()
        else:
            indptr, indices, indptr_t, indices_t, eperm_t = ctx.saved_tensors
            grad = grad.contiguous()
        g_el = g_er = None
        if use_hip(grad) and grad.shape[1] <= 8:
            e = get_ext()
            if ctx.needs_input_grad[0]:
                # d el[c] = Σ_{e: col_e=c} grad[e]: segment-sum over the
                # transposed CSR with the edge permutation
                g_el = e.segment_sum_edges(*_worklist_of(indptr_t)[:4], eperm_t,
                                           grad, ctx.n_src)
            if ctx.needs_input_grad[1]:
                g_er = e.segment_sum_edges(*_worklist_of(indptr)[:4], None,
                                           grad, ctx.n_dst)
            return g_el, g_er, None, None, None, None, None, None
        if ctx.needs_input_grad[0]:
            g_el = torch.zeros(ctx.n_src, grad.shape[1], dtype=grad.dtype,
                               device=grad.device)
            g_el.index_add_(0, indices.long(), grad)
        if ctx.needs_input_grad[1]:
            g_er = torch.zeros(ctx.n_dst, grad.shape[1], dtype=grad.dtype,
                               device=grad.device)
            row = torch.repeat_interleave(
                torch.arange(ctx.n_dst, device=grad.device),
                indptr[1:] - indptr[:-1])
            g_er.index_add_(0, row, grad)
        return g_el, g_er, None, None, None, None, None, None


def sddmm_add(el, er, indptr, indices, indptr_t, indices_t, eperm_t,
              slope=None):
    return _SDDMMAdd.apply(el, er, indptr, indices, indptr_t, indices_t,
                           eperm_t, slope)


class _GATv2Score(Function):
    """GATv2 logits (gatv2_score_raw). Saves zs, zd, attn and the CSRs —
    nothing per (edge, feature): the backward kernels recompute
    s = zs[col] + zd[row] from the rows they gather. d zd and d attn come
    from one pass over the forward CSR, d zs from one over the transposed
    CSR with eperm fused into the load of the gradient."""

    @staticmethod
    def forward(ctx, zs, zd, attn, indptr, indices, indptr_t, indices_t,
                eperm_t, slope):
        ctx.save_for_backward(zs, zd, attn, indptr, indices, indptr_t,
                              indices_t, eperm_t)
        ctx.slope = float(slope)
        return gatv2_score_raw(indptr, indices, zs, zd, attn, ctx.slope)

    @staticmethod
    def backward(ctx, grad):
        (zs, zd, attn, indptr, indices, indptr_t, indices_t,
         eperm_t) = ctx.saved_tensors
        grad = grad.contiguous()
        g_zs = g_zd = g_attn = None
        need_zs, need_zd, need_attn = ctx.needs_input_grad[:3]
        if need_zd or need_attn:
            g_zd, g_attn = gatv2_score_bwd_raw(
                indptr, indices, None, grad, zd, zs, attn, ctx.slope,
                want_dattn=need_attn)
            if need_attn:
                g_attn = g_attn.reshape(attn.shape)
        if need_zs:
            g_zs = gatv2_score_bwd_raw(indptr_t, indices_t, eperm_t, grad,
                                       zs, zd, attn, ctx.slope)[0]
        return (g_zs, g_zd if need_zd else None, g_attn) + (None,) * 6


def gatv2_score(zs, zd, attn, indptr, indices, indptr_t, indices_t, eperm_t,
                slope):
    """zs [n_src, H, D], zd [n_dst, H, D], attn H·D values -> e [E, H]."""
    return _GATv2Score.apply(zs, zd, attn, indptr, indices, indptr_t,
                             indices_t, eperm_t, slope)


class _SegmentSoftmax(Function):
    @staticmethod
    def forward(ctx, logits, indptr):
        alpha = segment_softmax_raw(indptr, logits)
        ctx.save_for_backward(alpha, indptr)
        return alpha

    @staticmethod
    def backward(ctx, grad):
        alpha, indptr = ctx.saved_tensors
        return segment_softmax_bwd_raw(indptr, alpha, grad.contiguous()), None


def segment_softmax(logits, indptr):
    return _SegmentSoftmax.apply(logits, indptr)


# GEMM dispatch (K6). Two hand-written fp32 MFMA kernels live behind
# gemm_nt_bias / gemm_nn / gemm_tn: the 64x64 gemm_f32_kernel and the tiled
# 128x128 kernel (ops/hip/gemm_tiled.hip); the extension routes between
# them by shape and alignment (kernels.hip route_tiled). Per-shape A/B on
# MI355X (profiles/BENCH_SUMMARY_gemm_tiled.md), ms, rocBLAS / tiled / 64x64:
#   NT forward [232965,1204]x[256,1204]^T  1.33 / 1.54 / 2.04  -> rocBLAS
#   NT forward [232965, 256]x[256, 256]^T  0.28 / 0.38 / 0.47  -> rocBLAS
#   NN dx      [232965, 256]x[256, 256]    0.33 / 0.32 / 0.44  -> rocBLAS
#     (a 3 % kernel-level gap, 0.02 ms per epoch: not moved)
#   TN dW      [232965,256]^T x [232965,1204]  1.83 / 1.41 / 2.06 -> tiled
#     and every other aligned dW (0.34 against 0.73 / 0.43 at 256x256);
#     41/44-wide outputs stay on the 64x64 kernel.
# "auto" routes each direction to the winner; BNSGCN_GEMM=hip forces the
# hand-written kernels everywhere.
_GEMM_MODE = _os.environ.get("BNSGCN_GEMM", "auto")


class _Linear(Function):
    """XW^T + b; see _GEMM_MODE for the MFMA/rocBLAS routing."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        if use_hip(x) and _GEMM_MODE == "hip":
            return get_ext().gemm_nt_bias(x, weight, bias)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, grad):
        x, weight = ctx.saved_tensors
        grad = grad.contiguous()
        gx = gw = gb = None
        if use_hip(x):
            e = get_ext()
            if ctx.needs_input_grad[0]:
                gx = e.gemm_nn(grad, weight) if _GEMM_MODE == "hip" \
                    else grad @ weight
            if ctx.needs_input_grad[1]:
                gw = e.gemm_tn(grad, x)     # split-K: ours wins
            if ctx.has_bias and ctx.needs_input_grad[2]:
                return gx, gw, e.syncbn_stats(grad)[0]
        else:
            if ctx.needs_input_grad[0]:
                gx = grad @ weight
            if ctx.needs_input_grad[1]:
                gw = grad.t() @ x
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = grad.sum(0)
        return gx, gw, gb


def linear(x, weight, bias=None):
    return _Linear.apply(x, weight, bias)


class _DropoutLinear(Function):
    """dropout(x) W^T + b with the dropout fused into the tiled GEMM's
    operand load, forward and dW: x itself is saved, the mask is
    regenerated from (seed, flat index) in backward, and the dropped-out
    copy of x never exists. x gets no gradient (the caller guarantees it
    needs none)."""

    @staticmethod
    def forward(ctx, x, weight, bias, keep, seed):
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.keep, ctx.seed = keep, seed
        ctx.has_bias = bias is not None
        return get_ext().gemm_nt_bias_drop(x, weight.contiguous(), bias,
                                           keep, seed)

    @staticmethod
    def backward(ctx, grad):
        x, weight = ctx.saved_tensors
        grad = grad.contiguous()
        e = get_ext()
        gw = gb = None
        if ctx.needs_input_grad[1]:
            gw = e.gemm_tn_drop(grad, x, ctx.keep, ctx.seed)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = e.syncbn_stats(grad)[0]
        return None, gw, gb, None, None


def dropout_linear(x, weight, bias, p: float, training: bool):
    """linear(dropout(x, p, training), weight, bias). On the GPU, for an
    fp32 x that needs no gradient, the dropout is applied inside the GEMMs
    (_DropoutLinear); the seed is drawn exactly as dropout() draws it, so
    masks are those of the unfused path. Everything else — CPU tensors,
    x.requires_grad, p <= 0, eval — is the unfused composition.

    A memory lever, not a speed one: it saves the dropped-out copy of x
    (1.12 GB for the headline layer-0 input) but recomputes the splitmix64
    mask once per output tile column, and the Reddit epoch measured 0.38 ms
    slower with it than with dropout() + rocBLAS
    (profiles/BENCH_SUMMARY_gemm_tiled.md) — the models do not call it."""
    if (training and p > 0.0 and use_hip(x) and x.dtype == torch.float32
            and not x.requires_grad):
        seed = int(torch.randint(0, 2**62, (1,)).item())
        return _DropoutLinear.apply(x, weight, bias, 1.0 - p, seed)
    return linear(dropout(x, p, training), weight, bias)


class _BiasAdd(Function):
    """h + b for a bias added outside a GEMM (the project-then-aggregate
    layers). The bias gradient is the K12 column-sum kernel on GPU, as in
    _Linear: torch's generic dim-0 reduction took 0.78 ms on the
    [154k, 41] logits gradient against 0.11 ms
    (profiles/BENCH_SUMMARY_projfirst.md)."""

    @staticmethod
    def forward(ctx, h, bias):
        return h + bias

    @staticmethod
    def backward(ctx, grad):
        gb = None
        if ctx.needs_input_grad[1]:
            gb = get_ext().syncbn_stats(grad.contiguous())[0] \
                if use_hip(grad) else grad.sum(0)
        return grad, gb


def bias_add(h, bias):
    return _BiasAdd.apply(h, bias)


class _LayerNormF(Function):
    """Row LayerNorm (K7) on the fused gfx950 kernels — torch's ROCm LN
    kernels measured ~27% of the ogbn-products epoch (profiles/
    topk_products_r02.txt). act=True additionally fuses the inter-layer
    ReLU (K9): forward emits relu(ln(x)); backward regenerates the
    activation mask from the saved LN state — no mask, no ReLU kernels."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, act):
        x = x.contiguous()
        y, mean, rstd = get_ext().ln_fwd(x, weight, bias, eps, int(act))
        ctx.save_for_backward(x, weight, bias, mean, rstd)
        ctx.act = int(act)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, mean, rstd = ctx.saved_tensors
        dx, dw, db = get_ext().ln_bwd(x, dy.contiguous(), w, b, mean, rstd,
                                      ctx.act)
        return dx, dw, db, None, None


def layer_norm(x, weight, bias, eps: float = 1e-5, act: bool = False):
    """act=True computes relu(layer_norm(x)) in one fused pair on GPU."""
    if use_hip(x) and x.shape[-1] <= 1024 and x.dtype == torch.float32:
        return _LayerNormF.apply(x, weight, bias, eps, act)
    y = torch.nn.functional.layer_norm(x, (x.shape[-1],), weight, bias, eps)
    return torch.relu(y) if act else y


class _DropoutF(Function):
    """Mask-free dropout (K8): the splitmix64 mask is regenerated from the
    saved seed in backward — one elementwise kernel each way, no mask
    tensor, no torch RNG-state kernels."""

    @staticmethod
    def forward(ctx, x, keep, seed):
        ctx.keep, ctx.seed = keep, seed
        return get_ext().dropout_apply(x.contiguous(), keep, seed)

    @staticmethod
    def backward(ctx, dy):
        return (get_ext().dropout_apply(dy.contiguous(), ctx.keep, ctx.seed),
                None, None)


def dropout(x, p: float, training: bool):
    if not training or p <= 0.0:
        return x
    if use_hip(x) and x.dtype == torch.float32:
        seed = int(torch.randint(0, 2**62, (1,)).item())
        return _DropoutF.apply(x, 1.0 - p, seed)
    return torch.nn.functional.dropout(x, p, training)


# Fused LayerNorm + ReLU + dropout between the layers (ln_act_drop_fwd /
# ln_act_drop_bwd). BNSGCN_LN_FUSE=0 (or setting _LN_FUSE False) keeps the
# separate layer_norm and dropout ops: the same masks and the same forward
# bits, three more passes over the activation per layer in each direction.
_LN_FUSE = _os.environ.get("BNSGCN_LN_FUSE", "1") != "0"


def ln_fuse_active(x, width: int, p: float, training: bool) -> bool:
    """True where layer_norm_act_dropout runs the fused kernels on a
    [*, width] activation that lives where x lives: HIP, fp32, width <=
    1024, training with p > 0. The models ask BEFORE the layer runs, since
    on this path the layer hands its bias gradients to the fused op."""
    return (_LN_FUSE and training and p > 0.0 and width <= 1024
            and x.dim() == 2 and x.dtype == torch.float32 and use_hip(x))


class _LayerNormActDropoutF(Function):
    """y = dropout(act(LN(x))) in one kernel, and the whole backward in
    one pass: dx, dgamma, dbeta and colsum(dx). `biases` are the bias
    parameters that the linears producing x added to every row of it;
    their values are not read, and their gradient is colsum(dx) by the
    chain rule — the caller passes bias.detach() to those linears so that
    nothing else computes it."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, act, keep, seed, *biases):
        x = x.contiguous()
        y, mean, rstd = get_ext().ln_act_drop_fwd(x, weight, bias, eps,
                                                  int(act), keep, seed)
        ctx.save_for_backward(x, weight, bias, mean, rstd)
        ctx.act, ctx.keep, ctx.seed = int(act), keep, seed
        ctx.n_biases = len(biases)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, mean, rstd = ctx.saved_tensors
        dx, dw, db, colsum = get_ext().ln_act_drop_bwd(
            x, dy.contiguous(), w, b, mean, rstd, ctx.act, ctx.keep, ctx.seed)
        # one tensor per parameter: .grad of two parameters never aliases
        gb = tuple(colsum if i == 0 else colsum.clone()
                   for i in range(ctx.n_biases))
        return (dx, dw, db, None, None, None, None) + gb


def layer_norm_act_dropout(x, weight, bias, eps: float = 1e-5,
                           act: bool = False, p: float = 0.0,
                           training: bool = False, bias_grad_to=()):
    """dropout(layer_norm(x, act=act), p, training), fused into one kernel
    each way where ln_fuse_active(x, ...) holds; the seed is drawn exactly
    as dropout() draws it, so the mask is the unfused one. bias_grad_to:
    see _LayerNormActDropoutF — only valid on the fused path."""
    if ln_fuse_active(x, x.shape[-1], p, training):
        seed = int(torch.randint(0, 2**62, (1,)).item())
        return _LayerNormActDropoutF.apply(x, weight, bias, eps, act,
                                           1.0 - p, seed, *bias_grad_to)
    if len(bias_grad_to):
        raise RuntimeError("layer_norm_act_dropout: bias_grad_to needs the "
                           "fused path (ln_fuse_active)")
    return dropout(layer_norm(x, weight, bias, eps, act), p, training)


# Fused SyncBatchNorm + ReLU + dropout for --norm batch (ops/hip/
# bn_fused.hip, docs/DESIGN.md §5b): 3 passes over the activation forward
# and 5 backward. BNSGCN_BN_FUSE=0 (or setting _BN_FUSE False) keeps
# models/sync_bn._SyncBNFunc followed by relu and dropout(): the same
# masks, about 13 and 18 passes.
_BN_FUSE = _os.environ.get("BNSGCN_BN_FUSE", "1") != "0"


def bn_fuse_active(x, training: bool) -> bool:
    """True where sync_batch_norm_act_dropout runs the fused kernels on x:
    HIP, fp32, 2-D, training."""
    return (_BN_FUSE and training and x.dim() == 2
            and x.dtype == torch.float32 and use_hip(x))


class _SyncBNActDropoutF(Function):
    """y = dropout(relu?(SyncBN(x))) over the bn_* kernels. The two
    all-reduces ([Σx, Σx², rows] forward, [Σg, Σg·x̂] backward) stay here,
    between the column-sum finish and the kernel that consumes the reduced
    vector; a rank without rows contributes zeros to both. Saved: x and the
    per-column mean, rstd, weight, bias — no x_hat, no mask — plus the
    one-element global row count, which stays on the device."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum,
                eps, act, keep, seed):
        from ..models.sync_bn import _maybe_all_reduce
        e = get_ext()
        x = x.contiguous()
        stats = e.bn_colsums_fwd(x)
        _maybe_all_reduce(stats)
        mean, rstd = e.bn_finalize(stats, running_mean, running_var,
                                   momentum, eps)
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        ctx.save_for_backward(x, mean, rstd, w, b)
        ctx.count = stats[-1:]
        ctx.act, ctx.keep, ctx.seed = int(act), keep, seed
        return e.bn_act_drop_fwd(x, mean, rstd, w, b, ctx.act, keep, seed)

    @staticmethod
    def backward(ctx, dy):
        from ..models.sync_bn import _maybe_all_reduce
        e = get_ext()
        x, mean, rstd, w, b = ctx.saved_tensors
        dy = dy.contiguous()
        tail = (ctx.act, ctx.keep, ctx.seed)
        red = e.bn_colsums_bwd(x, dy, mean, rstd, w, b, ctx.count, *tail)
        nf = x.shape[1]
        _maybe_all_reduce(red[:2 * nf])
        dx = e.bn_act_drop_bwd_dx(x, dy, mean, rstd, w, b, red, *tail)
        return (dx, red[nf:2 * nf], red[:nf]) + (None,) * 7


def sync_batch_norm_act_dropout(x, weight, bias, running_mean, running_var,
                                momentum: float, eps: float,
                                act: bool = False, p: float = 0.0,
                                training: bool = False):
    """dropout(relu?(SyncBatchNorm(x)), p, training). Fused where
    bn_fuse_active(x, training) holds; the dropout seed is drawn exactly as
    dropout() draws it and only when p > 0, so the RNG order and the masks
    are those of the unfused path, which is taken everywhere else."""
    if bn_fuse_active(x, training):
        seed = int(torch.randint(0, 2**62, (1,)).item()) if p > 0.0 else 0
        return _SyncBNActDropoutF.apply(x, weight, bias, running_mean,
                                        running_var, momentum, eps, act,
                                        1.0 - p, seed)
    from ..models.sync_bn import _SyncBNFunc
    y = _SyncBNFunc.apply(x, weight, bias, None, running_mean, running_var,
                          training, momentum, eps)
    if act:
        y = torch.relu(y)
    return dropout(y, p, training)


def segment_softmax2_raw(indptr1, logits1, indptr2, logits2):
    if use_hip(logits1):
        return get_ext().segment_softmax2(indptr1, logits1, indptr2, logits2,
                                          1.0, 0)[:2]
    return ref.segment_softmax2(indptr1, logits1, indptr2, logits2)


def segment_softmax2_bwd_raw(indptr1, a1, g1, indptr2, a2, g2):
    if use_hip(a1):
        return get_ext().segment_softmax2_backward(indptr1, a1, g1,
                                                   indptr2, a2, g2, 1.0, 0)
    return ref.segment_softmax2_backward(indptr1, a1, g1, indptr2, a2, g2)


class _SegmentSoftmax2(Function):
    """Union softmax over two per-row edge sets (split GAT block), with
    the GAT attention dropout FUSED on the HIP path (p_drop > 0): the
    forward emits the dropped weights alongside the saved pre-drop
    softmax, and the backward regenerates the Philox mask from the saved
    seed — no mask tensor, no separate dropout kernels (reference: DGL
    GATConv attn_drop)."""

    @staticmethod
    def forward(ctx, logits1, logits2, indptr1, indptr2, p_drop):
        keep = 1.0 - float(p_drop or 0.0)
        if use_hip(logits1):
            seed = int(torch.randint(0, 2**62, (1,)).item()) if keep < 1.0 \
                else 0
            a1, a2, da1, da2 = get_ext().segment_softmax2(
                indptr1, logits1, indptr2, logits2, keep, seed)
        else:
            a1, a2 = ref.segment_softmax2(indptr1, logits1, indptr2, logits2)
            seed = 0
            if keep < 1.0:
                m1 = (torch.rand_like(a1) < keep).float()
                m2 = (torch.rand_like(a2) < keep).float()
                da1, da2 = a1 * m1 / keep, a2 * m2 / keep
                ctx.cpu_masks = (m1, m2)
            else:
                da1, da2 = a1, a2
        ctx.keep, ctx.seed = keep, seed
        ctx.save_for_backward(a1, a2, indptr1, indptr2)
        return da1, da2

    @staticmethod
    def backward(ctx, g1, g2):
        a1, a2, indptr1, indptr2 = ctx.saved_tensors
        g1, g2 = g1.contiguous(), g2.contiguous()
        if use_hip(a1):
            d1, d2 = get_ext().segment_softmax2_backward(
                indptr1, a1, g1, indptr2, a2, g2, ctx.keep, ctx.seed)
        else:
            if ctx.keep < 1.0:
                m1, m2 = ctx.cpu_masks
                g1, g2 = g1 * m1 / ctx.keep, g2 * m2 / ctx.keep
            d1, d2 = ref.segment_softmax2_backward(indptr1, a1, g1,
                                                   indptr2, a2, g2)
        return d1, d2, None, None, None


def segment_softmax2(logits1, logits2, indptr1, indptr2, p_drop=0.0):
    return _SegmentSoftmax2.apply(logits1, logits2, indptr1, indptr2, p_drop)


class _AttnProject(Function):
    """Fused GAT attention projections (el, er) = (<z,a_l>, <z,a_r>) per
    (node, head) — one read of z instead of torch's broadcast-mul +
    reduce chains in each direction."""

    @staticmethod
    def forward(ctx, z, al, ar):
        ctx.save_for_backward(z, al, ar)
        if use_hip(z) and z.shape[1] * z.shape[2] % 4 == 0 and z.shape[1] <= 8:
            el, er = get_ext().attn_project(z.contiguous(), al.contiguous(),
                                            ar.contiguous())
            return el, er
        return ref.attn_project(z, al, ar)

    @staticmethod
    def backward(ctx, g_el, g_er):
        z, al, ar = ctx.saved_tensors
        g_el = g_el.contiguous()
        g_er = g_er.contiguous()
        if use_hip(z) and z.shape[1] * z.shape[2] % 4 == 0 and z.shape[1] <= 8:
            dz, dal, dar = get_ext().attn_project_backward(
                z.contiguous(), al.contiguous(), ar.contiguous(), g_el, g_er)
            return dz, dal, dar
        return ref.attn_project_backward(z, al, ar, g_el, g_er)


def attn_project(z, al, ar):
    return _AttnProject.apply(z, al, ar)
