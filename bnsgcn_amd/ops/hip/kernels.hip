// bnsgcn_amd gfx950 kernel library — batch 1 (the GCN/SAGE hot path).
//
// Hand-written HIP for CDNA4 (MI355X): wave64, float4-vectorized HBM
// access, MFMA (v_mfma_f32_16x16x4_f32) for the dense GEMMs. No CUDA
// compatibility paths, no Triton. Reference-kernel parity map in
// spmm_sum=K1/K2/K3+K18, pack_rows=K13,
// scatter_add_rows=K14, philox_keys=K16, gemm_*=K6, syncbn_stats=K12.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/util/Optional.h>
#include <algorithm>
#include <type_traits>
#include "common.h"
#include "gemm_tiled.h"

namespace {

// ============================== SpMM ===================================
// out[row, :] (+)= dst_scale[row] * sum_{e} src_scale[col_e] * x[col_e, :]
// Work-list driven: each item = (row, edge range<=SEG) built by
// ops/csr_torch.build_worklist — heavy (power-law hub) rows are split
// across items and combined with atomicAdd, so no wave serializes a
// 100k+-edge row. Per 64-edge chunk the wave loads 64 column ids (and
// src scales) with ONE coalesced load each and broadcasts them via
// __shfl, so the row-feature loads are address-independent and the
// unrolled inner loop keeps several 1-KiB row reads in flight (the naive
// row-loop form serializes two dependent loads per edge behind
// s_waitcnt vmcnt(0) — measured 25x slower).
// Feature dim is covered in passes of 2 float4 per lane (512 floats);
// scalar variant (4 floats/lane/pass) handles F % 4 != 0.

DEV_INLINE void f4_axpy(float4& a, float ss, const float4 v) {
  a.x += ss * v.x; a.y += ss * v.y; a.z += ss * v.z; a.w += ss * v.w;
}

// T = source element type (float, or bf16_t for --agg-dtype bf16): the
// row read goes through load_src4 (common.h), nothing else depends on it.
template <typename T, bool ACC, int SUBW>
__global__ __launch_bounds__(256) void spmm_sum_vec4_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int32_t* __restrict__ indices, const T* __restrict__ x,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    float* __restrict__ out, int f4) {
  // SUBW = scheduling width: 64 (full wave) for wide rows, 32 (half-wave
  // subgroups, independent items per half) when f4 <= 32 so narrow
  // feature dims (e.g. h=128 -> f4=32) keep every lane busy.
  // (A strided schedule — the waves of an XCD walking consecutive items
  // to share one sliding src window in L2 — was measured and LOSES ~1-6%:
  // drifting waves break their own temporal locality,
  // profiles/BENCH_SUMMARY_r02.md.)
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const WaveItems wi = wave_items<SUBW>(wl);
  const int lane = wi.lane;
  float4* __restrict__ out4 = reinterpret_cast<float4*>(out);

  for (int it = wi.beg; it < wi.end; ++it) {
    const WorkItem wk = work_item(wl, it);
    const float ds = dst_scale ? dst_scale[wk.row] : 1.0f;
    for (int f0 = 0; f0 < f4; f0 += 2 * SUBW) {
      const int fA = f0 + lane;
      const int fB = fA + SUBW;
      const bool hasA = fA < f4, hasB = fB < f4;
      float4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      for (int64_t e0 = wk.beg; e0 < wk.end; e0 += SUBW) {
        const Chunk ch = load_chunk<SUBW>(indices, src_scale, e0, wk.end, lane);
#pragma unroll 4
        for (int k = 0; k < ch.nv; ++k) {
          const int c = __shfl(ch.cid, k, SUBW);
          const float ss = src_scale ? __shfl(ch.ssc, k, SUBW) : 1.0f;
          const int64_t base = (int64_t)c * f4;
          if (hasA) f4_axpy(acc0, ss, load_src4(x, base + fA));
          if (hasB) f4_axpy(acc1, ss, load_src4(x, base + fB));
        }
      }
      const int64_t ob = (int64_t)wk.row * f4;
      if (hasA) store_row<ACC>(&out4[ob + fA], acc0, wk.atomic, ds);
      if (hasB) store_row<ACC>(&out4[ob + fB], acc1, wk.atomic, ds);
    }
  }
}

// Row-group form for a STATIC CSR and wide rows (f4 > 32): the schedule's
// "row" is a group of R consecutive destination rows and an item is a
// range of that group's entries — its distinct source columns, ascending,
// each with R uint8 edge counts (ops/csr_torch.build_rowgroups). The wave
// reads an entry's source row ONCE and adds it to every row of the group
// that has the edge: rows = consecutive ids of a locality-ordered
// partition share neighbours, so this asks for a fraction of the 1-KiB
// row reads the per-row kernel issues (entries / edges, the builder's
// `ratio`). Lane l owns float4 l (and l + 64 when NV = 2) of all R rows:
// R * NV float4 accumulators.
// Column id, src scale and the weight words of 64 entries arrive with one
// coalesced load each and are broadcast with readlane, so everything that
// steers an entry is wave-uniform: the test `w != 0` is a scalar branch.
// It is a correctness requirement, not an optimisation — a branch-free
// 0 * v would carry an inf/NaN of the source row into rows that have no
// edge to it. Four row reads are issued before the first accumulate.
// Within a row, terms are added in ascending column order, so a row of an
// unsplit group is bit-reproducible from run to run.
template <int NW>
DEV_INLINE void load_group_w(const uint32_t* __restrict__ p, uint32_t (&w)[NW]) {
  if constexpr (NW == 1) {
    w[0] = *p;
  } else {
    static_assert(NW == 2, "R in {4, 8}");
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    w[0] = t.x; w[1] = t.y;
  }
}

template <typename T, bool ACC, int R, int NV>
__global__ __launch_bounds__(256) void spmm_sum_grouped_kernel(
    const int32_t* __restrict__ wgroup, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int32_t* __restrict__ ecol, const uint32_t* __restrict__ ew,
    const T* __restrict__ x, const float* __restrict__ src_scale,
    const float* __restrict__ dst_scale, float* __restrict__ out, int f4,
    int n_rows) {
  constexpr int NW = R / 4;                  // 32-bit weight words per entry
  constexpr int U = 4;                       // row reads in flight
  const WorkList wl = {wgroup, wbeg, wend, wave_start};
  const WaveItems wi = wave_items<WAVE>(wl);
  const int lane = wi.lane;
  const int it_beg = __builtin_amdgcn_readfirstlane(wi.beg);
  const int it_end = __builtin_amdgcn_readfirstlane(wi.end);
  float4* __restrict__ out4 = reinterpret_cast<float4*>(out);
  const float4 zero4 = {0.f, 0.f, 0.f, 0.f};

  for (int it = it_beg; it < it_end; ++it) {
    const WorkItem wk = work_item(wl, it);   // wk.row = group id
    for (int f0 = 0; f0 < f4; f0 += NV * WAVE) {
      // a lane past the row's end reads the row's last float4 instead
      // (in bounds, one unconditional 16-byte load — 8-byte for a bf16
      // source) and never stores
      int fi[NV];
      bool has[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        fi[v] = f0 + v * WAVE + lane;
        has[v] = fi[v] < f4;
        if (!has[v]) fi[v] = f4 - 1;
      }
      float4 acc[NV][R];
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[v][r] = zero4;
      uint32_t seen[NW];                     // OR of the item's weight words
#pragma unroll
      for (int j = 0; j < NW; ++j) seen[j] = 0u;

      // one entry: add row `val` to every row of the group with w != 0
      auto accumulate = [&](int k, const float4 (&val)[NV], int ssc,
                            const uint32_t (&wv)[NW]) {
        const float ss = __int_as_float(__builtin_amdgcn_readlane(ssc, k));
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)wv[j], k);
          seen[j] |= w;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const uint32_t cnt = (w >> (8 * b)) & 0xffu;
            if (cnt != 0u) {
              const float s = (float)cnt * ss;
#pragma unroll
              for (int v = 0; v < NV; ++v) f4_axpy(acc[v][4 * j + b], s, val[v]);
            }
          }
        }
      };

      for (int64_t e0 = wk.beg; e0 < wk.end; e0 += WAVE) {
        const int nv = (int)((wk.end - e0 < WAVE) ? (wk.end - e0) : WAVE);
        int cid = 0, ssc = __float_as_int(1.0f);
        uint32_t wv[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) wv[j] = 0u;
        if (lane < nv) {
          cid = ecol[e0 + lane];
          if (src_scale) ssc = __float_as_int(src_scale[cid]);
          load_group_w<NW>(ew + (e0 + lane) * NW, wv);
        }
        int k = 0;
        for (; k + U <= nv; k += U) {
          float4 val[U][NV];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int64_t base =
                (int64_t)__builtin_amdgcn_readlane(cid, k + u) * f4;
#pragma unroll
            for (int v = 0; v < NV; ++v)
              val[u][v] = load_src4(x, base + fi[v]);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) accumulate(k + u, val[u], ssc, wv);
        }
        for (; k < nv; ++k) {
          float4 val[NV];
          const int64_t base = (int64_t)__builtin_amdgcn_readlane(cid, k) * f4;
#pragma unroll
          for (int v = 0; v < NV; ++v) val[v] = load_src4(x, base + fi[v]);
          accumulate(k, val, ssc, wv);
        }
      }

      // a row is stored only if the item holds an entry for it
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int row = wk.row * R + r;
        if (((seen[r / 4] >> (8 * (r % 4))) & 0xffu) != 0u && row < n_rows) {
          const float ds = dst_scale ? dst_scale[row] : 1.0f;
          const int64_t ob = (int64_t)row * f4;
#pragma unroll
          for (int v = 0; v < NV; ++v)
            if (has[v])
              store_row<ACC>(&out4[ob + fi[v]], acc[v][r], wk.atomic, ds);
        }
      }
    }
  }
}

// Narrow rows (f4 <= G float4, e.g. the 41->44-wide projected output
// layer): a row is at most G lanes wide, so the half-wave form above
// leaves most lanes without a load. Here the wave is EDGE-parallel
// instead: it still owns one contiguous worklist range and walks one item
// at a time (same load balance and XCD remap), but lane group g = lane/G
// takes edges k+g of the 64-edge chunk and lane j = lane%G loads float4 j
// of that source row — 64/G row reads per step, x4 unroll. The groups'
// partial sums are combined at the end of the item with __shfl_xor over
// offsets G, 2G, ... (a fixed order, so non-atomic rows stay run-to-run
// deterministic) and group 0 writes.
template <typename T, bool ACC, int G>
__global__ __launch_bounds__(256) void spmm_sum_narrow_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int32_t* __restrict__ indices, const T* __restrict__ x,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    float* __restrict__ out, int f4) {
  constexpr int NG = WAVE / G;  // edges per step
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const WaveItems wi = wave_items<WAVE>(wl);
  const int lane = wi.lane;
  const int g = lane / G, j = lane % G;
  const bool has = j < f4;
  float4* __restrict__ out4 = reinterpret_cast<float4*>(out);

  for (int it = wi.beg; it < wi.end; ++it) {
    const WorkItem wk = work_item(wl, it);
    const float ds = dst_scale ? dst_scale[wk.row] : 1.0f;
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t e0 = wk.beg; e0 < wk.end; e0 += WAVE) {
      const Chunk ch = load_chunk<WAVE>(indices, src_scale, e0, wk.end, lane);
#pragma unroll 4
      for (int k = 0; k < ch.nv; k += NG) {
        const int kk = k + g;  // k <= WAVE - NG, so kk < WAVE
        const int c = __shfl(ch.cid, kk, WAVE);
        const float ss = src_scale ? __shfl(ch.ssc, kk, WAVE) : 1.0f;
        if (has && kk < ch.nv)
          f4_axpy(acc, ss, load_src4(x, (int64_t)c * f4 + j));
      }
    }
#pragma unroll
    for (int off = G; off < WAVE; off <<= 1) {
      acc.x += __shfl_xor(acc.x, off, WAVE);
      acc.y += __shfl_xor(acc.y, off, WAVE);
      acc.z += __shfl_xor(acc.z, off, WAVE);
      acc.w += __shfl_xor(acc.w, off, WAVE);
    }
    if (g == 0 && has)
      store_row<ACC>(&out4[(int64_t)wk.row * f4 + j], acc, wk.atomic, ds);
  }
}

// float2 form for F % 2 == 0 (but % 4 != 0, e.g. the 602-wide Reddit
// feature matrix: rows are 8-byte but not 16-byte aligned): 4 float2
// accumulators cover 512 floats per edge walk — the scalar form needed
// 3 walks at 4-byte loads for F=602 (57 ms for the one-time precompute
// SpMM, profiles/topk_reddit_final_r02.txt).
template <bool ACC>
__global__ __launch_bounds__(256) void spmm_sum_vec2_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int32_t* __restrict__ indices, const float* __restrict__ x,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    float* __restrict__ out, int f2) {
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const WaveItems wi = wave_items<WAVE>(wl);
  const int lane = wi.lane;
  const float2* __restrict__ x2 = reinterpret_cast<const float2*>(x);
  float2* __restrict__ out2 = reinterpret_cast<float2*>(out);
  for (int it = wi.beg; it < wi.end; ++it) {
    const WorkItem wk = work_item(wl, it);
    const float ds = dst_scale ? dst_scale[wk.row] : 1.0f;
    for (int f0 = 0; f0 < f2; f0 += 4 * WAVE) {
      float2 acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
      for (int64_t e0 = wk.beg; e0 < wk.end; e0 += WAVE) {
        const Chunk ch = load_chunk<WAVE>(indices, src_scale, e0, wk.end, lane);
#pragma unroll 4
        for (int k = 0; k < ch.nv; ++k) {
          const int c = __shfl(ch.cid, k, WAVE);
          const float ss = src_scale ? __shfl(ch.ssc, k, WAVE) : 1.0f;
          const int64_t base = (int64_t)c * f2;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int f = f0 + j * WAVE + lane;
            if (f < f2) {
              const float2 v = x2[base + f];
              acc[j].x += ss * v.x;
              acc[j].y += ss * v.y;
            }
          }
        }
      }
      const int64_t ob = (int64_t)wk.row * f2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = f0 + j * WAVE + lane;
        if (f >= f2) break;
        store_row<ACC>(&out2[ob + f], acc[j], wk.atomic, ds);
      }
    }
  }
}

template <bool ACC>
__global__ __launch_bounds__(256) void spmm_sum_scalar_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int32_t* __restrict__ indices, const float* __restrict__ x,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    float* __restrict__ out, int F) {
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const WaveItems wi = wave_items<WAVE>(wl);
  const int lane = wi.lane;
  for (int it = wi.beg; it < wi.end; ++it) {
    const WorkItem wk = work_item(wl, it);
    const float ds = dst_scale ? dst_scale[wk.row] : 1.0f;
    for (int f0 = 0; f0 < F; f0 += 4 * WAVE) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int64_t e0 = wk.beg; e0 < wk.end; e0 += WAVE) {
        const Chunk ch = load_chunk<WAVE>(indices, src_scale, e0, wk.end, lane);
#pragma unroll 2
        for (int k = 0; k < ch.nv; ++k) {
          const int c = __shfl(ch.cid, k, WAVE);
          const float ss = src_scale ? __shfl(ch.ssc, k, WAVE) : 1.0f;
          const int64_t base = (int64_t)c * F;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int f = f0 + j * WAVE + lane;
            if (f < F) acc[j] += ss * x[base + f];
          }
        }
      }
      const int64_t ob = (int64_t)wk.row * F;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = f0 + j * WAVE + lane;
        if (f >= F) break;
        store_row<ACC>(&out[ob + f], acc[j], wk.atomic, ds);
      }
    }
  }
}

// ========================= pack / scatter ==============================
// pack: out[r, :] = scale[r] * x[idx[r], :]        (send-side gather, K13)
// scatter: out[idx[r], :] += scale[r] * src[r, :]  (grad unpack, K14).
// Scatter destinations can repeat ACROSS peers (a node bordering several
// partitions) -> atomicAdd (fp32, device scope).

// T = float or bf16_t (the rounded copy of --agg-dtype bf16): the output is
// fp32 float(x[idx]) * scale, one fp32 multiply, either way.
template <typename T>
__global__ void pack_rows_kernel(const T* __restrict__ x,
                                 const int64_t* __restrict__ idx,
                                 const float* __restrict__ scale,
                                 float* __restrict__ out, int n, int F) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)n * F;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = t; i < total; i += stride) {
    const int r = i / F, f = i - (int64_t)r * F;
    const float s = scale ? scale[r] : 1.0f;
    out[i] = s * load_src1(x, idx[r] * F + f);
  }
}

template <typename T>
__global__ void pack_rows_vec4_kernel(const T* __restrict__ x,
                                      const int64_t* __restrict__ idx,
                                      const float* __restrict__ scale,
                                      float* __restrict__ out, int n, int f4) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)n * f4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float4* __restrict__ out4 = reinterpret_cast<float4*>(out);
  for (int64_t i = t; i < total; i += stride) {
    const int r = i / f4, f = i - (int64_t)r * f4;
    const float s = scale ? scale[r] : 1.0f;
    const float4 v = load_src4(x, idx[r] * f4 + f);
    out4[i] = make_float4(s * v.x, s * v.y, s * v.z, s * v.w);
  }
}

__global__ void scatter_add_rows_kernel(float* __restrict__ out,
                                        const int64_t* __restrict__ idx,
                                        const float* __restrict__ src,
                                        const float* __restrict__ scale,
                                        int n, int F) {
  // 4 floats per thread (vectorized read; atomics stay per-float —
  // destination rows can repeat across peers)
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t q = F / 4;
  const bool vec = (F % 4 == 0);
  const int64_t total = vec ? (int64_t)n * q : (int64_t)n * F;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float4* __restrict__ src4 = reinterpret_cast<const float4*>(src);
  for (int64_t i = t; i < total; i += stride) {
    if (vec) {
      const int r = i / q, f = i - (int64_t)r * q;
      const float s = scale ? scale[r] : 1.0f;
      const float4 v = src4[i];
      float* p = &out[idx[r] * F + f * 4];
      atomicAdd(p + 0, s * v.x); atomicAdd(p + 1, s * v.y);
      atomicAdd(p + 2, s * v.z); atomicAdd(p + 3, s * v.w);
    } else {
      const int r = i / F, f = i - (int64_t)r * F;
      const float s = scale ? scale[r] : 1.0f;
      atomicAdd(&out[idx[r] * F + f], s * src[i]);
    }
  }
}

// ============================== bf16 cast ==============================
// out = bf16_rne(x) over a flat contiguous array (--agg-dtype bf16 rounds
// the SpMM's source operand once; bit-identical to torch's CPU
// .to(torch.bfloat16), NaN payloads aside). Thread i converts elements
// 4i .. 4i+3 for i < n4 with one 16-byte load and one 8-byte store; the
// elements from 4 * n4 on go one per thread. n4 = n / 4, or 0 for an x
// whose base is not 16-byte aligned (a view at an odd offset).
__global__ __launch_bounds__(256) void cast_bf16_kernel(
    const float* __restrict__ x, bf16_t* __restrict__ out, int64_t n,
    int64_t n4) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
  uint2* __restrict__ out2 = reinterpret_cast<uint2*>(out);
  for (int64_t i = t; i < n4; i += stride) {
    const float4 v = x4[i];
    out2[i] = make_uint2(bf16_rne_bits(v.x) | (bf16_rne_bits(v.y) << 16),
                         bf16_rne_bits(v.z) | (bf16_rne_bits(v.w) << 16));
  }
  for (int64_t i = 4 * n4 + t; i < n; i += stride)
    out[i] = (bf16_t)bf16_rne_bits(x[i]);
}

// ============================ Philox keys ==============================
// Device-side BNS sampling keys — bitwise-identical to ops/philox.py
// (numpy); the sorted-top-s selection runs as torch.sort on device.

__global__ void philox_keys_kernel(int64_t* __restrict__ out, int n,
                                   uint32_t seed_lo, uint32_t seed_hi,
                                   uint32_t epoch, uint32_t sd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  P4 r = philox4x32((uint32_t)i, epoch, sd, 0x424E5347u, seed_lo, seed_hi);
  uint64_t key = ((uint64_t)r.c0 << 32) | r.c1;
  out[i] = (int64_t)(key & 0x7FFFFFFFFFFFFFFFull);
}

// =========================== SyncBN stats ==============================
// Column sums: out[0, f] = sum_r x[r, f]; out[1, f] = sum_r x[r, f]^2.
// Lane-per-column (coalesced row-major reads), one block per (col-chunk,
// row-chunk), block-partial then atomicAdd — few atomics per column.

__global__ void syncbn_stats_kernel(const float* __restrict__ x,
                                    float* __restrict__ out,
                                    int64_t n, int F, int row_chunks) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const int64_t rows_per = (n + row_chunks - 1) / row_chunks;
  const int64_t r0 = blockIdx.y * rows_per;
  const int64_t r1 = (r0 + rows_per < n) ? r0 + rows_per : n;
  float s = 0.f, s2 = 0.f;
  for (int64_t r = r0; r < r1; ++r) {
    const float v = x[r * F + f];
    s += v; s2 += v * v;
  }
  if (row_chunks == 1) { out[f] = s; out[F + f] = s2; }
  else { atomicAdd(&out[f], s); atomicAdd(&out[F + f], s2); }
}

// ============================ fp32 MFMA GEMM ===========================
// C[M,N] = A' @ B' (+bias), exact fp32 via v_mfma_f32_16x16x4_f32 (the
// CDNA4 f32-input MFMA: A lane map A[i=l&15][k=l>>4], B[k=l>>4][j=l&15],
// C/D col=l&15, row=(l>>4)*4+reg — cdna_hip_programming.md §3).
// Layout-generic via element strides (handles NT/NN/TN from one kernel);
// 64x64 block tile, 4 waves each owning a 32x32 quadrant (2x2 fragments),
// BK=16 LDS-staged with +1-float row pad against bank conflicts.
// These GEMMs are tall-skinny (M up to ~500k, N,K in 41..1204) and
// memory-bound; correctness + coalesced staging matter, peak MFMA does not.

#define BM 64
#define BN 64
#define BK 32

// Double-buffered: while the MFMAs consume LDS buffer `buf`, the next
// K-tile is loaded into registers and written to buf^1 (one barrier per
// K-step). Staging thread->element maps follow each operand's unit stride
// so global reads stay coalesced for every trans layout.
template <bool ATOMIC>
__global__ __launch_bounds__(256)
void gemm_f32_kernel(const float* __restrict__ A, int64_t sAm, int64_t sAk,
                     const float* __restrict__ B, int64_t sBk, int64_t sBn,
                     const float* __restrict__ bias, float* __restrict__ C,
                     int M, int N, int K, int k_slice) {
  __shared__ float As[2][BM][BK + 1];
  __shared__ float Bs[2][BK][BN + 1];
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;          // 4 waves: quadrant (wr, wc)
  const int wr = (wid >> 1) * 32, wc = (wid & 1) * 32;

  const int kb = blockIdx.z * k_slice;
  const int ke = (kb + k_slice < K) ? kb + k_slice : K;

  // per-thread staging coordinates (8 elements of A, 8 of B per K-tile)
  int ai[8], ak[8], bk[8], bj[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int tA = tid + j * 256;      // over BM*BK = 2048
    if (sAk == 1) { ai[j] = tA / BK; ak[j] = tA % BK; }
    else          { ai[j] = tA % BM; ak[j] = tA / BM; }
    const int tB = tid + j * 256;      // over BK*BN = 2048
    if (sBn == 1) { bk[j] = tB / BN; bj[j] = tB % BN; }
    else          { bk[j] = tB % BK; bj[j] = tB / BK; }
  }
  float ra[8], rb[8];
  auto load_regs = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int gm = m0 + ai[j], gka = k0 + ak[j];
      ra[j] = (gm < M && gka < ke) ? A[gm * sAm + gka * sAk] : 0.f;
      const int gkb = k0 + bk[j], gn = n0 + bj[j];
      rb[j] = (gkb < ke && gn < N) ? B[gkb * sBk + gn * sBn] : 0.f;
    }
  };
  auto write_lds = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      As[buf][ai[j]][ak[j]] = ra[j];
      Bs[buf][bk[j]][bj[j]] = rb[j];
    }
  };

  using f32x4 = __attribute__((ext_vector_type(4))) float;
  f32x4 acc[2][2] = {};
  const int i_l = lane & 15, k_l = lane >> 4;

  load_regs(kb);
  write_lds(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kb; k0 < ke; k0 += BK) {
    const bool more = (k0 + BK) < ke;
    if (more) load_regs(k0 + BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
#pragma unroll
      for (int fi = 0; fi < 2; ++fi) {
        const float a = As[buf][wr + fi * 16 + i_l][kk + k_l];
#pragma unroll
        for (int fj = 0; fj < 2; ++fj) {
          const float b = Bs[buf][kk + k_l][wc + fj * 16 + i_l];
          acc[fi][fj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b,
                                                             acc[fi][fj], 0, 0, 0);
        }
      }
    }
    if (more) {
      write_lds(buf ^ 1);
      __syncthreads();
    }
    buf ^= 1;
  }

  // epilogue: C/D map col=l&15, row=(l>>4)*4+reg
  const int j_l = lane & 15, r_l = lane >> 4;
#pragma unroll
  for (int fi = 0; fi < 2; ++fi)
#pragma unroll
    for (int fj = 0; fj < 2; ++fj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gm = m0 + wr + fi * 16 + r_l * 4 + r;
        const int gn = n0 + wc + fj * 16 + j_l;
        if (gm < M && gn < N) {
          float v = acc[fi][fj][r];
          if (bias && blockIdx.z == 0) v += bias[gn];  // bias once (slice 0)
          if (ATOMIC) atomicAdd(&C[(int64_t)gm * N + gn], v);
          else C[(int64_t)gm * N + gn] = v;
        }
      }
}

// ============================ GAT kernel set ===========================
// SDDMM u_add_v, segmented edge-softmax fwd/bwd, edge-weighted SpMM and
// per-edge dot (reference K4/K5 — DGL GATConv internals). Edge tensors
// are CSR-ordered (grouped by destination row), so softmax segments are
// contiguous: one wave per (row, head) with shfl-based reductions.

DEV_INLINE float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

DEV_INLINE float wave_reduce_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
  return v;
}

// logits[e,h] = leaky_relu(el[col_e,h] + er[row_e,h]) — work-list
// scheduled with batched coalesced index loads (the row-serial form was
// dependent-load bound at ~200 GB/s); slope < 0 disables the activation.
__global__ __launch_bounds__(256) void sddmm_add_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int32_t* __restrict__ indices, const float* __restrict__ el,
    const float* __restrict__ er, float* __restrict__ out, int H,
    float slope) {
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const WaveItems wi = wave_items<WAVE>(wl);
  for (int it = wi.beg; it < wi.end; ++it) {
    const WorkItem wk = work_item(wl, it);
    for (int64_t e0 = wk.beg; e0 < wk.end; e0 += WAVE) {
      const int64_t e = e0 + wi.lane;
      if (e >= wk.end) break;
      const int64_t c = indices[e];
      for (int h = 0; h < H; ++h) {
        float v = el[c * H + h] + er[(int64_t)wk.row * H + h];
        if (slope >= 0.f && v < 0.f) v *= slope;
        out[e * H + h] = v;
      }
    }
  }
}

// alpha[e,h] = softmax over each row's edge segment (numerically stable).
__global__ void segment_softmax_kernel(const int64_t* __restrict__ indptr,
                                       const float* __restrict__ logits,
                                       float* __restrict__ alpha,
                                       int n_rows, int H) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n_waves = (gridDim.x * blockDim.x) / WAVE;
  for (int rh = wave; rh < n_rows * H; rh += n_waves) {
    const int r = rh / H, h = rh % H;
    const int64_t beg = indptr[r], end = indptr[r + 1];
    if (beg == end) continue;
    float m = -INFINITY;
    for (int64_t e = beg + lane; e < end; e += WAVE)
      m = fmaxf(m, logits[e * H + h]);
    m = wave_reduce_max(m);
    float sum = 0.f;
    for (int64_t e = beg + lane; e < end; e += WAVE)
      sum += __expf(logits[e * H + h] - m);
    sum = wave_reduce_sum(sum);
    const float inv = 1.0f / fmaxf(sum, 1e-38f);
    for (int64_t e = beg + lane; e < end; e += WAVE)
      alpha[e * H + h] = __expf(logits[e * H + h] - m) * inv;
  }
}

// dlogit[e,h] = a[e,h]*(g[e,h] - sum_seg a*g)
__global__ void segment_softmax_bwd_kernel(const int64_t* __restrict__ indptr,
                                           const float* __restrict__ alpha,
                                           const float* __restrict__ grad,
                                           float* __restrict__ out,
                                           int n_rows, int H) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n_waves = (gridDim.x * blockDim.x) / WAVE;
  for (int rh = wave; rh < n_rows * H; rh += n_waves) {
    const int r = rh / H, h = rh % H;
    const int64_t beg = indptr[r], end = indptr[r + 1];
    float sum = 0.f;
    for (int64_t e = beg + lane; e < end; e += WAVE)
      sum += alpha[e * H + h] * grad[e * H + h];
    sum = wave_reduce_sum(sum);
    for (int64_t e = beg + lane; e < end; e += WAVE)
      out[e * H + h] = alpha[e * H + h] * (grad[e * H + h] - sum);
  }
}

// Union softmax over TWO per-row edge segments (split GAT block:
// static inner edges + per-epoch sampled halo edges) — shared max/sum.
// The fused attention dropout uses the mask of common.h (drop_keep).

DEV_INLINE float4 f4_max(float4 a, float4 b) {
  return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z),
                     fmaxf(a.w, b.w));
}

DEV_INLINE float4 wave_reduce_sum4(float4 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v.x += __shfl_xor(v.x, off, WAVE);
    v.y += __shfl_xor(v.y, off, WAVE);
    v.z += __shfl_xor(v.z, off, WAVE);
    v.w += __shfl_xor(v.w, off, WAVE);
  }
  return v;
}

DEV_INLINE float4 wave_reduce_max4(float4 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    float4 o = make_float4(__shfl_xor(v.x, off, WAVE),
                           __shfl_xor(v.y, off, WAVE),
                           __shfl_xor(v.z, off, WAVE),
                           __shfl_xor(v.w, off, WAVE));
    v = f4_max(v, o);
  }
  return v;
}

// The four union-softmax kernels below write each pass ONCE and run it
// over both edge sets s = 0, 1 (fully unrolled): set s of row r is
// [ip[s][r], ip[s][r+1]) and its dropout-mask indices start at moff[s]
// (set 2 follows set 1 in the flat mask index space).

// H == 4 (the GAT bench head count): one wave per row, each LANE loads
// one edge's float4 of ALL FOUR heads — fully coalesced [E,4] access
// with the SAME per-row pass count as the per-(row,head) form (64 edges
// per pass; the head work rides in the lane's float4 ALU). The
// per-(row,head) form reads at stride 16 B (1/4 cacheline utilization)
// and measured ~20% of the Yelp GAT epoch. (A one-wave-per-row form for
// any power-of-two H, lanes interleaved over edge x head, was coalesced
// too but measured SLOWER on Yelp GAT, 85 -> 112 ms epoch: short
// power-law segments are latency-bound and lose the head parallelism.)
__global__ void segment_softmax2_h4_kernel(
    const int64_t* __restrict__ ip1, const float4* __restrict__ l1,
    const int64_t* __restrict__ ip2, const float4* __restrict__ l2,
    float4* __restrict__ a1, float4* __restrict__ a2,
    float4* __restrict__ da1, float4* __restrict__ da2,
    int n_rows, float keep, uint64_t seed, int64_t off2) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n_waves = (gridDim.x * blockDim.x) / WAVE;
  const bool drop = keep < 1.0f;
  const uint32_t thr = drop_threshold(keep);
  const float inv_keep = drop ? 1.0f / keep : 1.0f;
  const int64_t* const ip[2] = {ip1, ip2};
  const float4* const l[2] = {l1, l2};
  float4* const a[2] = {a1, a2};
  float4* const da[2] = {da1, da2};
  const int64_t moff[2] = {0, off2};
  for (int r = wave; r < n_rows; r += n_waves) {
    const int64_t beg[2] = {ip[0][r], ip[1][r]};
    const int64_t end[2] = {ip[0][r + 1], ip[1][r + 1]};
    if (beg[0] == end[0] && beg[1] == end[1]) continue;
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int64_t e = beg[s] + lane; e < end[s]; e += WAVE)
        m = f4_max(m, l[s][e]);
    m = wave_reduce_max4(m);
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int64_t e = beg[s] + lane; e < end[s]; e += WAVE) {
        const float4 v = l[s][e];
        sum.x += __expf(v.x - m.x); sum.y += __expf(v.y - m.y);
        sum.z += __expf(v.z - m.z); sum.w += __expf(v.w - m.w);
      }
    sum = wave_reduce_sum4(sum);
    const float4 inv = make_float4(
        1.0f / fmaxf(sum.x, 1e-38f), 1.0f / fmaxf(sum.y, 1e-38f),
        1.0f / fmaxf(sum.z, 1e-38f), 1.0f / fmaxf(sum.w, 1e-38f));
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int64_t e = beg[s] + lane; e < end[s]; e += WAVE) {
        const float4 v = l[s][e];
        float4 av;
        av.x = __expf(v.x - m.x) * inv.x; av.y = __expf(v.y - m.y) * inv.y;
        av.z = __expf(v.z - m.z) * inv.z; av.w = __expf(v.w - m.w) * inv.w;
        a[s][e] = av;
        if (drop)
          da[s][e] = drop_apply(av, moff[s] + e * 4, thr, seed, inv_keep);
      }
  }
}

__global__ void segment_softmax2_h4_bwd_kernel(
    const int64_t* __restrict__ ip1, const float4* __restrict__ a1,
    const float4* __restrict__ g1, const int64_t* __restrict__ ip2,
    const float4* __restrict__ a2, const float4* __restrict__ g2,
    float4* __restrict__ d1, float4* __restrict__ d2,
    int n_rows, float keep, uint64_t seed, int64_t off2) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n_waves = (gridDim.x * blockDim.x) / WAVE;
  const bool drop = keep < 1.0f;
  const uint32_t thr = drop_threshold(keep);
  const float inv_keep = drop ? 1.0f / keep : 1.0f;
  const int64_t* const ip[2] = {ip1, ip2};
  const float4* const a[2] = {a1, a2};
  const float4* const g[2] = {g1, g2};
  float4* const d[2] = {d1, d2};
  const int64_t moff[2] = {0, off2};
  for (int r = wave; r < n_rows; r += n_waves) {
    const int64_t beg[2] = {ip[0][r], ip[1][r]};
    const int64_t end[2] = {ip[0][r + 1], ip[1][r + 1]};
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int64_t e = beg[s] + lane; e < end[s]; e += WAVE) {
        const float4 av = a[s][e];
        float4 gv = g[s][e];
        if (drop) gv = drop_apply(gv, moff[s] + e * 4, thr, seed, inv_keep);
        sum.x += av.x * gv.x; sum.y += av.y * gv.y;
        sum.z += av.z * gv.z; sum.w += av.w * gv.w;
      }
    sum = wave_reduce_sum4(sum);
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int64_t e = beg[s] + lane; e < end[s]; e += WAVE) {
        const float4 av = a[s][e];
        float4 gv = g[s][e];
        if (drop) gv = drop_apply(gv, moff[s] + e * 4, thr, seed, inv_keep);
        d[s][e] = make_float4(av.x * (gv.x - sum.x), av.y * (gv.y - sum.y),
                              av.z * (gv.z - sum.z), av.w * (gv.w - sum.w));
      }
  }
}

// General H: one wave per (row, head).
// keep < 1: additionally writes the attn-dropout-applied weights into
// da1/da2 (the spmm input), while a1/a2 keep the pre-drop softmax (the
// backward state) — replaces the separate torch dropout pass
// (reference: DGL GATConv attn_drop).
__global__ void segment_softmax2_kernel(const int64_t* __restrict__ ip1,
                                        const float* __restrict__ l1,
                                        const int64_t* __restrict__ ip2,
                                        const float* __restrict__ l2,
                                        float* __restrict__ a1,
                                        float* __restrict__ a2,
                                        float* __restrict__ da1,
                                        float* __restrict__ da2,
                                        int n_rows, int H, float keep,
                                        uint64_t seed, int64_t off2) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n_waves = (gridDim.x * blockDim.x) / WAVE;
  const bool drop = keep < 1.0f;
  const uint32_t thr = drop_threshold(keep);
  const float inv_keep = drop ? 1.0f / keep : 1.0f;
  const int64_t* const ip[2] = {ip1, ip2};
  const float* const l[2] = {l1, l2};
  float* const a[2] = {a1, a2};
  float* const da[2] = {da1, da2};
  const int64_t moff[2] = {0, off2};
  for (int rh = wave; rh < n_rows * H; rh += n_waves) {
    const int r = rh / H, h = rh % H;
    const int64_t beg[2] = {ip[0][r], ip[1][r]};
    const int64_t end[2] = {ip[0][r + 1], ip[1][r + 1]};
    if (beg[0] == end[0] && beg[1] == end[1]) continue;
    float m = -INFINITY;
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int64_t e = beg[s] + lane; e < end[s]; e += WAVE)
        m = fmaxf(m, l[s][e * H + h]);
    m = wave_reduce_max(m);
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int64_t e = beg[s] + lane; e < end[s]; e += WAVE)
        sum += __expf(l[s][e * H + h] - m);
    sum = wave_reduce_sum(sum);
    const float inv = 1.0f / fmaxf(sum, 1e-38f);
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int64_t e = beg[s] + lane; e < end[s]; e += WAVE) {
        const float av = __expf(l[s][e * H + h] - m) * inv;
        a[s][e * H + h] = av;
        if (drop)
          da[s][e * H + h] =
              drop_apply(av, moff[s] + e * H + h, thr, seed, inv_keep);
      }
  }
}

// keep < 1: the incoming grads g1/g2 are w.r.t. the DROPPED weights; the
// dropout backward (mask/keep, mask regenerated from seed) is folded in
// before the softmax Jacobian.
__global__ void segment_softmax2_bwd_kernel(const int64_t* __restrict__ ip1,
                                            const float* __restrict__ a1,
                                            const float* __restrict__ g1,
                                            const int64_t* __restrict__ ip2,
                                            const float* __restrict__ a2,
                                            const float* __restrict__ g2,
                                            float* __restrict__ d1,
                                            float* __restrict__ d2,
                                            int n_rows, int H, float keep,
                                            uint64_t seed, int64_t off2) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n_waves = (gridDim.x * blockDim.x) / WAVE;
  const bool drop = keep < 1.0f;
  const uint32_t thr = drop_threshold(keep);
  const float inv_keep = drop ? 1.0f / keep : 1.0f;
  const int64_t* const ip[2] = {ip1, ip2};
  const float* const a[2] = {a1, a2};
  const float* const g[2] = {g1, g2};
  float* const d[2] = {d1, d2};
  const int64_t moff[2] = {0, off2};
  for (int rh = wave; rh < n_rows * H; rh += n_waves) {
    const int r = rh / H, h = rh % H;
    const int64_t beg[2] = {ip[0][r], ip[1][r]};
    const int64_t end[2] = {ip[0][r + 1], ip[1][r + 1]};
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int64_t e = beg[s] + lane; e < end[s]; e += WAVE) {
        float gv = g[s][e * H + h];
        if (drop) gv = drop_apply(gv, moff[s] + e * H + h, thr, seed, inv_keep);
        sum += a[s][e * H + h] * gv;
      }
    sum = wave_reduce_sum(sum);
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int64_t e = beg[s] + lane; e < end[s]; e += WAVE) {
        float gv = g[s][e * H + h];
        if (drop) gv = drop_apply(gv, moff[s] + e * H + h, thr, seed, inv_keep);
        d[s][e * H + h] = a[s][e * H + h] * (gv - sum);
      }
  }
}

// out[r,h,:] (+)= sum_e w[e,h] * x[col_e,h,:] — wave per (row,head),
// lanes stride D (coalesced within a head row).
template <bool ACC>
__global__ void spmm_edge_kernel(const int64_t* __restrict__ indptr,
                                 const int32_t* __restrict__ indices,
                                 const float* __restrict__ w,
                                 const float* __restrict__ x,
                                 float* __restrict__ out,
                                 int n_rows, int H, int D) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n_waves = (gridDim.x * blockDim.x) / WAVE;
  for (int rh = wave; rh < n_rows * H; rh += n_waves) {
    const int r = rh / H, h = rh % H;
    const int64_t beg = indptr[r], end = indptr[r + 1];
    for (int d = lane; d < D; d += WAVE) {
      float acc = 0.f;
      for (int64_t e = beg; e < end; ++e) {
        const int c = indices[e];
        acc += w[e * H + h] * x[((int64_t)c * H + h) * D + d];
      }
      const int64_t o = ((int64_t)r * H + h) * D + d;
      if (ACC) out[o] += acc; else out[o] = acc;
    }
  }
}

// gw[e,h] = <g[row_e,h,:], x[col_e,h,:]>, general-D form: work-list
// scheduled, batched coalesced index loads, full-wave shfl reduction per
// (edge, head). Used when the register-resident fast form's shape
// conditions fail (e.g. D % 8 != 0 on the GAT output layer).
__global__ __launch_bounds__(256) void sddmm_dot_gen_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int32_t* __restrict__ indices, const float* __restrict__ g,
    const float* __restrict__ x, float* __restrict__ out, int H, int D,
    int HD) {
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const WaveItems wi = wave_items<WAVE>(wl);
  const int lane = wi.lane;
  const int sg = lane >> 4;            // 4 subgroups of 16 lanes:
  const int gl = lane & 15;            // 4 (edge) pairs in flight per wave
  for (int it = wi.beg; it < wi.end; ++it) {
    const WorkItem wk = work_item(wl, it);
    for (int64_t e0 = wk.beg; e0 < wk.end; e0 += WAVE) {
      const Chunk ch = load_chunk<WAVE>(indices, nullptr, e0, wk.end, lane);
      for (int k0 = 0; k0 < ch.nv; k0 += 4) {
        const int k = k0 + sg;
        const bool act = k < ch.nv;
        const int c = __shfl(ch.cid, act ? k : 0, WAVE);
        for (int h = 0; h < H; ++h) {
          float p = 0.f;
          if (act)
            for (int d = gl; d < D; d += 16)
              p += g[(int64_t)wk.row * HD + h * D + d] *
                   x[(int64_t)c * HD + h * D + d];
#pragma unroll
          for (int off = 8; off > 0; off >>= 1) p += __shfl_xor(p, off, WAVE);
          if (act && gl == 0) out[(e0 + k) * H + h] = p;
        }
      }
    }
  }
}

// Work-list-scheduled GAT aggregation (same scheduling as spmm_sum:
// batched coalesced index loads + shfl broadcast so row-feature loads
// pipeline; heavy rows split across items with atomicAdd combine).
// x is [N, H, D] flat (HD = H*D, D % 4 == 0); lane f covers head
// h = f / (D/4). The naive wave-per-(row,head) serial-edge form measured
// 144 ms vs this structure on the Yelp-shaped GAT block.
template <bool ACC>
__global__ __launch_bounds__(256) void spmm_edge_vec4_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int32_t* __restrict__ indices, const float* __restrict__ w,
    const int64_t* __restrict__ wperm, const float* __restrict__ x,
    float* __restrict__ out, int H, int D4, int HD4) {
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const WaveItems wi = wave_items<WAVE>(wl);
  const int lane = wi.lane;
  const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
  float4* __restrict__ out4 = reinterpret_cast<float4*>(out);
  for (int it = wi.beg; it < wi.end; ++it) {
    const WorkItem wk = work_item(wl, it);
    // two float4 accumulators per lane (like spmm_sum_vec4): HD4 <= 128
    // — the common [H=4, D=128] GAT shape — walks the edge list ONCE
    // instead of once per 64-float4 feature pass
    for (int f0 = 0; f0 < HD4; f0 += 2 * WAVE) {
      const int fA = f0 + lane;
      const int fB = fA + WAVE;
      const bool hasA = fA < HD4, hasB = fB < HD4;
      const int hA = hasA ? fA / D4 : 0;
      const int hB = hasB ? fB / D4 : 0;
      float4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      for (int64_t e0 = wk.beg; e0 < wk.end; e0 += WAVE) {
        const Chunk ch = load_chunk<WAVE>(indices, nullptr, e0, wk.end, lane);
#pragma unroll 4
        for (int k = 0; k < ch.nv; ++k) {
          const int c = __shfl(ch.cid, k, WAVE);
          const int64_t we = wperm ? wperm[e0 + k] : (e0 + k);
          const int64_t base = (int64_t)c * HD4;
          if (hasA) f4_axpy(acc0, w[we * H + hA], x4[base + fA]);
          if (hasB) f4_axpy(acc1, w[we * H + hB], x4[base + fB]);
        }
      }
      const int64_t ob = (int64_t)wk.row * HD4;
      if (hasA) store_row<ACC>(&out4[ob + fA], acc0, wk.atomic);
      if (hasB) store_row<ACC>(&out4[ob + fB], acc1, wk.atomic);
    }
  }
}

// sddmm_dot, vec4 general form (any H, D % 4 == 0): same 4x16-subgroup
// edge pipeline as the gen kernel but float4 loads (4x fewer memory ops;
// the D=100 GAT output layer measured 7.8 ms/call on the scalar gen
// path, profiles/topk_gat_r02.txt)
__global__ __launch_bounds__(256) void sddmm_dot_vec4_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int32_t* __restrict__ indices, const float* __restrict__ g,
    const float* __restrict__ x, float* __restrict__ out, int H, int D,
    int HD) {
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const WaveItems wi = wave_items<WAVE>(wl);
  const int lane = wi.lane;
  const int sg = lane >> 4;            // 4 subgroups of 16 lanes
  const int gl = lane & 15;
  const int D4 = D >> 2;
  const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
  for (int it = wi.beg; it < wi.end; ++it) {
    const WorkItem wk = work_item(wl, it);
    const int64_t grow = (int64_t)wk.row * (HD >> 2);
    for (int64_t e0 = wk.beg; e0 < wk.end; e0 += WAVE) {
      const Chunk ch = load_chunk<WAVE>(indices, nullptr, e0, wk.end, lane);
      for (int k0 = 0; k0 < ch.nv; k0 += 4) {
        const int k = k0 + sg;
        const bool act = k < ch.nv;
        const int c = __shfl(ch.cid, act ? k : 0, WAVE);
        const int64_t crow = (int64_t)c * (HD >> 2);
        for (int h = 0; h < H; ++h) {
          float p = 0.f;
          if (act)
            for (int d = gl; d < D4; d += 16) {
              const float4 a = g4[grow + h * D4 + d];
              const float4 b = x4[crow + h * D4 + d];
              p += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
            }
#pragma unroll
          for (int off = 8; off > 0; off >>= 1) p += __shfl_xor(p, off, WAVE);
          if (act && gl == 0) out[(e0 + k) * H + h] = p;
        }
      }
    }
  }
}

// sddmm_dot, fast form (HD <= 512, D % 8 == 0, D/8 a power of two):
// each lane holds 8 consecutive floats of the FIXED dst-row g[row] in
// registers; per edge the x slice streams in, the per-lane partial dot
// reduces over the D/8-lane head group via shfl_xor, the group leader
// stores gw[e,h]. Batched index loads as everywhere else.
__global__ __launch_bounds__(256) void sddmm_dot_fast_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int32_t* __restrict__ indices, const float* __restrict__ g,
    const float* __restrict__ x, float* __restrict__ out, int H, int D,
    int HD) {
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const WaveItems wi = wave_items<WAVE>(wl);
  const int lane = wi.lane;
  const int grp = D / 8;               // lanes per head group (pow2)
  const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
  for (int it = wi.beg; it < wi.end; ++it) {
    // split rows need no atomics: each (e,h) is written exactly once
    const WorkItem wk = work_item(wl, it);
    const bool active = lane * 8 < HD;
    const int h = active ? (lane * 8) / D : 0;
    float4 rg0 = {0,0,0,0}, rg1 = {0,0,0,0};
    if (active) {
      rg0 = g4[(int64_t)wk.row * (HD / 4) + lane * 2];
      rg1 = g4[(int64_t)wk.row * (HD / 4) + lane * 2 + 1];
    }
    for (int64_t e0 = wk.beg; e0 < wk.end; e0 += WAVE) {
      const Chunk ch = load_chunk<WAVE>(indices, nullptr, e0, wk.end, lane);
#pragma unroll 2
      for (int k = 0; k < ch.nv; ++k) {
        const int c = __shfl(ch.cid, k, WAVE);
        float p = 0.f;
        if (active) {
          const float4 xa = x4[(int64_t)c * (HD / 4) + lane * 2];
          const float4 xb = x4[(int64_t)c * (HD / 4) + lane * 2 + 1];
          p = rg0.x * xa.x + rg0.y * xa.y + rg0.z * xa.z + rg0.w * xa.w +
              rg1.x * xb.x + rg1.y * xb.y + rg1.z * xb.z + rg1.w * xb.w;
        }
        // reduce within the head group (contiguous lanes, pow2 size)
        for (int off = grp >> 1; off > 0; off >>= 1)
          p += __shfl_xor(p, off, WAVE);
        if (active && (lane & (grp - 1)) == 0)
          out[(e0 + k) * H + h] = p;
      }
    }
  }
}

// out[r,h] (+)= sum_{e in row r} grad[perm ? perm[e] : e, h] — the
// SDDMM-add backward segment sums (g_er with perm = null on the forward
// CSR; g_el with perm = eperm on the transposed CSR), replacing torch
// index_add atomics.
__global__ __launch_bounds__(256) void segment_sum_edges_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int64_t* __restrict__ perm, const float* __restrict__ grad,
    float* __restrict__ out, int H) {
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const WaveItems wi = wave_items<WAVE>(wl);
  for (int it = wi.beg; it < wi.end; ++it) {
    const WorkItem wk = work_item(wl, it);
    // lane l accumulates head l%H over edges strided WAVE/H... simple:
    // each lane takes edges lane, lane+64, ... and adds all H into
    // per-lane partials, then wave-reduce per head.
    float acc[8];  // H <= 8 supported here (fallback in launcher)
#pragma unroll
    for (int h = 0; h < 8; ++h) acc[h] = 0.f;
    for (int64_t e = wk.beg + wi.lane; e < wk.end; e += WAVE) {
      const int64_t ee = perm ? perm[e] : e;
      for (int h = 0; h < H; ++h) acc[h] += grad[ee * H + h];
    }
    for (int h = 0; h < H; ++h) {
      float v = wave_reduce_sum(acc[h]);
      if (wi.lane == 0)
        store_row<true>(&out[(int64_t)wk.row * H + h], v, wk.atomic);
    }
  }
}

// H == 4 form: one float4 load per (permuted) edge instead of four
// scalars
__global__ __launch_bounds__(256) void segment_sum_edges_h4_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int64_t* __restrict__ perm, const float4* __restrict__ grad,
    float4* __restrict__ out) {
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const WaveItems wi = wave_items<WAVE>(wl);
  for (int it = wi.beg; it < wi.end; ++it) {
    const WorkItem wk = work_item(wl, it);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t e = wk.beg + wi.lane; e < wk.end; e += WAVE) {
      const int64_t ee = perm ? perm[e] : e;
      const float4 v = grad[ee];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    acc = wave_reduce_sum4(acc);
    if (wi.lane == 0) store_row<true>(&out[wk.row], acc, wk.atomic);
  }
}

// int32 bincount (torch's histogram kernel measured 6.8 ms on a 14M-edge
// per-epoch transpose; this is a plain atomic histogram, ~0.1 ms)
__global__ void bincount_i32_kernel(const int32_t* __restrict__ v, int64_t n,
                                    int64_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = t; i < n; i += stride)
    atomicAdd(reinterpret_cast<unsigned long long*>(&out[v[i]]), 1ull);
}

// Fused GAT attention projections: el[n,h] = <z[n,h,:], al[h,:]>,
// er[n,h] = <z[n,h,:], ar[h,:]> — z is read ONCE (torch's broadcast-mul
// + reduce chain reads/writes the [N,H,D] product twice per direction).
// Wave per node row; per-lane partial accumulators indexed by the head a
// float4 slot belongs to (H <= 8), wave-reduced per head.
// ALIGNED (D % 4 == 0): a float4 slot lies inside one head. Otherwise
// only (H*D) % 4 == 0 holds (e.g. the GAT output layer, D = n_class) and
// a slot can straddle two heads, so the head is derived per component.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void attn_project_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ al,
    const float* __restrict__ ar, float* __restrict__ el,
    float* __restrict__ er, int64_t n, int H, int D, int hd4) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n_waves = (gridDim.x * blockDim.x) / WAVE;
  const float4* __restrict__ z4 = reinterpret_cast<const float4*>(z);
  const float4* __restrict__ al4 = reinterpret_cast<const float4*>(al);
  const float4* __restrict__ ar4 = reinterpret_cast<const float4*>(ar);
  for (int64_t r = wave; r < n; r += n_waves) {
    float accl[8], accr[8];
#pragma unroll
    for (int h = 0; h < 8; ++h) { accl[h] = 0.f; accr[h] = 0.f; }
    for (int f = lane; f < hd4; f += WAVE) {
      const float4 zv = z4[r * hd4 + f];
      const float4 lv = al4[f];
      const float4 rv = ar4[f];
      if (ALIGNED) {
        const int h = (f * 4) / D;
        accl[h] += zv.x * lv.x + zv.y * lv.y + zv.z * lv.z + zv.w * lv.w;
        accr[h] += zv.x * rv.x + zv.y * rv.y + zv.z * rv.z + zv.w * rv.w;
      } else {
        const float zc[4] = {zv.x, zv.y, zv.z, zv.w};
        const float lc[4] = {lv.x, lv.y, lv.z, lv.w};
        const float rc[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int h = (f * 4 + j) / D;
          accl[h] += zc[j] * lc[j];
          accr[h] += zc[j] * rc[j];
        }
      }
    }
    for (int h = 0; h < H; ++h) {
      const float sl = wave_reduce_sum(accl[h]);
      const float sr = wave_reduce_sum(accr[h]);
      if (lane == 0) {
        el[r * H + h] = sl;
        er[r * H + h] = sr;
      }
    }
  }
}

// dz[n,h,d] = al[h,d]*g_el[n,h] + ar[h,d]*g_er[n,h] (single pass);
// ALIGNED as in the forward kernel
template <bool ALIGNED>
__global__ __launch_bounds__(256) void attn_project_dz_kernel(
    const float* __restrict__ al, const float* __restrict__ ar,
    const float* __restrict__ g_el, const float* __restrict__ g_er,
    float* __restrict__ dz, int64_t n, int H, int D, int hd4) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n_waves = (gridDim.x * blockDim.x) / WAVE;
  const float4* __restrict__ al4 = reinterpret_cast<const float4*>(al);
  const float4* __restrict__ ar4 = reinterpret_cast<const float4*>(ar);
  float4* __restrict__ dz4 = reinterpret_cast<float4*>(dz);
  for (int64_t r = wave; r < n; r += n_waves) {
    for (int f = lane; f < hd4; f += WAVE) {
      const float4 lv = al4[f];
      const float4 rv = ar4[f];
      if (ALIGNED) {
        const int h = (f * 4) / D;
        const float gl = g_el[r * H + h];
        const float gr = g_er[r * H + h];
        dz4[r * hd4 + f] = make_float4(lv.x * gl + rv.x * gr,
                                       lv.y * gl + rv.y * gr,
                                       lv.z * gl + rv.z * gr,
                                       lv.w * gl + rv.w * gr);
      } else {
        const float lc[4] = {lv.x, lv.y, lv.z, lv.w};
        const float rc[4] = {rv.x, rv.y, rv.z, rv.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int h = (f * 4 + j) / D;
          o[j] = lc[j] * g_el[r * H + h] + rc[j] * g_er[r * H + h];
        }
        dz4[r * hd4 + f] = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
  }
}

// dal[h,d] = sum_n z[n,h,d]*g_el[n,h]; dar likewise — column reduction
// with row chunks + atomics (out pre-zeroed by the launcher).
__global__ void attn_project_dattn_kernel(
    const float* __restrict__ z, const float* __restrict__ g_el,
    const float* __restrict__ g_er, float* __restrict__ dal,
    float* __restrict__ dar, int64_t n, int H, int D, int HD,
    int row_chunks) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= HD) return;
  const int h = f / D;
  const int64_t rows_per = (n + row_chunks - 1) / row_chunks;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per;
  const int64_t r1 = (r0 + rows_per < n) ? r0 + rows_per : n;
  float sl = 0.f, sr = 0.f;
  for (int64_t r = r0; r < r1; ++r) {
    const float zv = z[r * HD + f];
    sl += zv * g_el[r * H + h];
    sr += zv * g_er[r * H + h];
  }
  if (row_chunks == 1) { dal[f] = sl; dar[f] = sr; }
  else { atomicAdd(&dal[f], sl); atomicAdd(&dar[f], sr); }
}

// ============================ LayerNorm (K7) ===========================
// Row-wise LayerNorm over [N, F] fp32 (F <= 1024). One wave per row,
// 4 rows per 256-thread block, grid-stride; row values stay in registers
// across both reduction passes, lane l covers columns l, l+64, ...
// (coalesced). Replaces torch's ROCm LN kernels, which measured ~27% of
// the ogbn-products epoch (profiles/topk_products_r02.txt: 1 TB/s
// effective vs ~6 TB/s for this shape).

#define LN_MAX_K 16  // supports F up to 64*16

// act=1 fuses the inter-layer ReLU (model _post pairs them): forward
// writes max(ln, 0); backward recomputes the pre-activation from
// (x, mean, rstd, gamma, beta) and masks dy — no mask storage, no
// separate ReLU kernels (K9).
__global__ __launch_bounds__(256) void ln_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ y,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    int64_t n, int F, float eps, int act) {
  const int lane = threadIdx.x & 63;
  const float inv_f = 1.0f / F;
  float vals[LN_MAX_K], gm[LN_MAX_K], bt[LN_MAX_K];
  int K = 0;
  for (int f = lane; f < F; f += WAVE, ++K) { gm[K] = gamma[f]; bt[K] = beta[f]; }
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n;
       r += stride) {
    const float* xr = x + r * (int64_t)F;
    float s = 0.f;
    int k = 0;
    for (int f = lane; f < F; f += WAVE, ++k) { vals[k] = xr[f]; s += vals[k]; }
    s = wave_reduce_sum(s);
    const float mu = s * inv_f;
    float v = 0.f;
    for (int i = 0; i < K; ++i) { const float d = vals[i] - mu; v += d * d; }
    v = wave_reduce_sum(v);
    const float rstd = rsqrtf(v * inv_f + eps);
    float* yr = y + r * (int64_t)F;
    k = 0;
    for (int f = lane; f < F; f += WAVE, ++k) {
      const float o = (vals[k] - mu) * rstd * gm[k] + bt[k];
      yr[f] = act ? fmaxf(o, 0.f) : o;
    }
    if (lane == 0) { mean_out[r] = mu; rstd_out[r] = rstd; }
  }
}

// float4 variants (F % 4 == 0): lane l covers float4 chunks l, l+64, ...
// — 16 B loads instead of 4 B (the scalar LN backward measured 2.8 TB/s
// on [2.45M, 128]; products profile topk_products_final_r02.txt)
__global__ __launch_bounds__(256) void ln_fwd_v4_kernel(
    const float4* __restrict__ x, const float4* __restrict__ gamma,
    const float4* __restrict__ beta, float4* __restrict__ y,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    int64_t n, int F, float eps, int act) {
  const int lane = threadIdx.x & 63;
  const int F4 = F >> 2;
  const float inv_f = 1.0f / F;
  float4 vals[LN_MAX_K / 4 + 1], gm[LN_MAX_K / 4 + 1], bt[LN_MAX_K / 4 + 1];
  int K = 0;
  for (int f = lane; f < F4; f += WAVE, ++K) { gm[K] = gamma[f]; bt[K] = beta[f]; }
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n;
       r += stride) {
    const float4* xr = x + r * F4;
    float s = 0.f;
    int k = 0;
    for (int f = lane; f < F4; f += WAVE, ++k) {
      vals[k] = xr[f];
      s += vals[k].x + vals[k].y + vals[k].z + vals[k].w;
    }
    s = wave_reduce_sum(s);
    const float mu = s * inv_f;
    float v = 0.f;
    for (int i = 0; i < K; ++i) {
      const float a = vals[i].x - mu, b = vals[i].y - mu;
      const float c = vals[i].z - mu, d = vals[i].w - mu;
      v += a * a + b * b + c * c + d * d;
    }
    v = wave_reduce_sum(v);
    const float rstd = rsqrtf(v * inv_f + eps);
    float4* yr = y + r * F4;
    k = 0;
    for (int f = lane; f < F4; f += WAVE, ++k) {
      float4 o;
      o.x = (vals[k].x - mu) * rstd * gm[k].x + bt[k].x;
      o.y = (vals[k].y - mu) * rstd * gm[k].y + bt[k].y;
      o.z = (vals[k].z - mu) * rstd * gm[k].z + bt[k].z;
      o.w = (vals[k].w - mu) * rstd * gm[k].w + bt[k].w;
      if (act) {
        o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f);
        o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
      }
      yr[f] = o;
    }
    if (lane == 0) { mean_out[r] = mu; rstd_out[r] = rstd; }
  }
}

__global__ __launch_bounds__(256) void ln_bwd_dx_v4_kernel(
    const float4* __restrict__ x, const float4* __restrict__ dy,
    const float4* __restrict__ gamma, const float4* __restrict__ beta,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float4* __restrict__ dx, int64_t n, int F, int act) {
  const int lane = threadIdx.x & 63;
  const int F4 = F >> 2;
  const float inv_f = 1.0f / F;
  float4 xh[LN_MAX_K / 4 + 1], g[LN_MAX_K / 4 + 1];
  float4 gm[LN_MAX_K / 4 + 1], bt[LN_MAX_K / 4 + 1];
  int K = 0;
  for (int f = lane; f < F4; f += WAVE, ++K) {
    gm[K] = gamma[f];
    if (act) bt[K] = beta[f];
  }
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n;
       r += stride) {
    const float4* xr = x + r * F4;
    const float4* dr = dy + r * F4;
    const float mu = mean[r], rs = rstd[r];
    float a = 0.f, b = 0.f;
    int k = 0;
    for (int f = lane; f < F4; f += WAVE, ++k) {
      const float4 xv = xr[f];
      float4 dv = dr[f];
      xh[k].x = (xv.x - mu) * rs; xh[k].y = (xv.y - mu) * rs;
      xh[k].z = (xv.z - mu) * rs; xh[k].w = (xv.w - mu) * rs;
      if (act) {
        if (xh[k].x * gm[k].x + bt[k].x <= 0.f) dv.x = 0.f;
        if (xh[k].y * gm[k].y + bt[k].y <= 0.f) dv.y = 0.f;
        if (xh[k].z * gm[k].z + bt[k].z <= 0.f) dv.z = 0.f;
        if (xh[k].w * gm[k].w + bt[k].w <= 0.f) dv.w = 0.f;
      }
      g[k].x = dv.x * gm[k].x; g[k].y = dv.y * gm[k].y;
      g[k].z = dv.z * gm[k].z; g[k].w = dv.w * gm[k].w;
      a += g[k].x + g[k].y + g[k].z + g[k].w;
      b += g[k].x * xh[k].x + g[k].y * xh[k].y + g[k].z * xh[k].z +
           g[k].w * xh[k].w;
    }
    a = wave_reduce_sum(a) * inv_f;
    b = wave_reduce_sum(b) * inv_f;
    float4* dxr = dx + r * F4;
    k = 0;
    for (int f = lane; f < F4; f += WAVE, ++k) {
      float4 o;
      o.x = rs * (g[k].x - a - xh[k].x * b);
      o.y = rs * (g[k].y - a - xh[k].y * b);
      o.z = rs * (g[k].z - a - xh[k].z * b);
      o.w = rs * (g[k].w - a - xh[k].w * b);
      dxr[f] = o;
    }
  }
}

// dx = rstd * ( g - mean(g) - xhat * mean(g * xhat) ),  g = dy * gamma
// (act=1: g is first masked by the recomputed pre-activation sign)
__global__ __launch_bounds__(256) void ln_bwd_dx_kernel(
    const float* __restrict__ x, const float* __restrict__ dy,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ dx, int64_t n, int F, int act) {
  const int lane = threadIdx.x & 63;
  const float inv_f = 1.0f / F;
  float xh[LN_MAX_K], g[LN_MAX_K], gm[LN_MAX_K], bt[LN_MAX_K];
  int K = 0;
  for (int f = lane; f < F; f += WAVE, ++K) {
    gm[K] = gamma[f];
    bt[K] = act ? beta[f] : 0.f;
  }
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n;
       r += stride) {
    const float* xr = x + r * (int64_t)F;
    const float* dr = dy + r * (int64_t)F;
    const float mu = mean[r], rs = rstd[r];
    float a = 0.f, b = 0.f;
    int k = 0;
    for (int f = lane; f < F; f += WAVE, ++k) {
      xh[k] = (xr[f] - mu) * rs;
      float d = dr[f];
      if (act && xh[k] * gm[k] + bt[k] <= 0.f) d = 0.f;
      g[k] = d * gm[k];
      a += g[k];
      b += g[k] * xh[k];
    }
    a = wave_reduce_sum(a) * inv_f;
    b = wave_reduce_sum(b) * inv_f;
    float* dxr = dx + r * (int64_t)F;
    k = 0;
    for (int f = lane; f < F; f += WAVE, ++k)
      dxr[f] = rs * (g[k] - a - xh[k] * b);
  }
}

// dgamma[f] = sum_r dy*xhat, dbeta[f] = sum_r dy — column reduction in
// the syncbn_stats shape (thread per column, chunked rows, atomic
// combine); act=1 masks dy by the recomputed pre-activation sign
__global__ void ln_bwd_w_kernel(
    const float* __restrict__ x, const float* __restrict__ dy,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ out, int64_t n, int F, int row_chunks, int act) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const float gmf = act ? gamma[f] : 0.f;
  const float btf = act ? beta[f] : 0.f;
  const int64_t rows_per = (n + row_chunks - 1) / row_chunks;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per;
  const int64_t r1 = (r0 + rows_per < n) ? r0 + rows_per : n;
  float sg = 0.f, sb = 0.f;
  for (int64_t r = r0; r < r1; ++r) {
    const float xh = (x[r * (int64_t)F + f] - mean[r]) * rstd[r];
    float d = dy[r * (int64_t)F + f];
    if (act && xh * gmf + btf <= 0.f) d = 0.f;
    sg += d * xh;
    sb += d;
  }
  if (row_chunks == 1) { out[f] = sg; out[F + f] = sb; }
  else { atomicAdd(&out[f], sg); atomicAdd(&out[F + f], sb); }
}

// -------------------------- dropout (K8) -------------------------------
// Mask-free feature dropout: out[i] = keep(seed, i) ? x[i]/keep : 0,
// mask regenerated from splitmix64 — the SAME kernel serves forward and
// backward (apply to x, then to dy), so no mask tensor ever exists.
__global__ __launch_bounds__(256) void dropout_apply_kernel(
    const float* __restrict__ x, float* __restrict__ out, int64_t n,
    float keep, uint64_t seed) {
  const bool drop = keep < 1.0f;   // keep == 1.0f: plain copy
  const uint32_t thr = drop_threshold(keep);
  const float inv_keep = drop ? 1.0f / keep : 1.0f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    out[i] = (!drop || drop_keep(i, thr, seed)) ? x[i] * inv_keep : 0.f;
}

// float4 form (n % 4 == 0): identical per-element masks (drop_keep on
// the flat index), 4x wider memory ops
__global__ __launch_bounds__(256) void dropout_apply_v4_kernel(
    const float4* __restrict__ x, float4* __restrict__ out, int64_t n4,
    float keep, uint64_t seed) {
  const bool drop = keep < 1.0f;   // keep == 1.0f: plain copy
  const uint32_t thr = drop_threshold(keep);
  const float inv_keep = drop ? 1.0f / keep : 1.0f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    const float4 v = x[i];
    out[i] = drop ? drop_apply(v, i * 4, thr, seed, inv_keep) : v;
  }
}

// ------------------------------ launchers ------------------------------

inline void check_f32(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == at::kFloat,
              name, " must be contiguous fp32 CUDA tensor");
}

// Source operand of the gather kernels: fp32, or the bf16 copy made by
// cast_bf16. Rows are read with 16-byte (8-byte) vector loads, so the
// base must be aligned to that — true of every allocation, not of every
// view of one.
inline void check_src(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 2 &&
                  (t.scalar_type() == at::kFloat ||
                   t.scalar_type() == at::kBFloat16),
              name, " must be a contiguous 2-D fp32 or bf16 CUDA tensor");
  if (t.scalar_type() == at::kBFloat16)
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 8 == 0,
                name, ": bf16 source must be 8-byte aligned");
}

const bf16_t* bf16_ptr(const at::Tensor& t) {
  return reinterpret_cast<const bf16_t*>(t.data_ptr<at::BFloat16>());
}

const float* opt_ptr(const c10::optional<at::Tensor>& t) {
  return t.has_value() ? t->data_ptr<float>() : nullptr;
}

int spmm_grid(int n_rows) {
  // wave-per-row, 4 rows per block; >> 256 workgroups fills 8 XCDs
  const int blocks = (n_rows + 3) / 4;
  return std::min(blocks, 16384);
}

int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// Host side of the work-list contract (common.h): the four schedule
// arrays as built by ops/csr_torch.build_worklist, validated once for
// every entry point. n_waves % 8 == 0 is what lets each launcher size
// its grid as n_waves / (waves per 256-thread block) without a remainder
// — a schedule that broke it would silently skip its last items.
struct WorkListArgs {
  WorkList wl;
  int n_waves;
};

WorkListArgs worklist_args(const at::Tensor& wrow, const at::Tensor& wbeg,
                           const at::Tensor& wend,
                           const at::Tensor& wave_start) {
  TORCH_CHECK(wrow.scalar_type() == at::kInt &&
                  wbeg.scalar_type() == at::kLong &&
                  wend.scalar_type() == at::kLong &&
                  wave_start.scalar_type() == at::kInt,
              "worklist: wrow/wave_start int32 and wbeg/wend int64 expected");
  for (const at::Tensor* t : {&wrow, &wbeg, &wend, &wave_start})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->device() == wave_start.device(),
                "worklist arrays must be contiguous CUDA tensors on one "
                "device");
  // array-length consistency: the kernels index wbeg/wend by item id
  TORCH_CHECK(wave_start.numel() >= 1 && wbeg.numel() == wrow.numel() &&
                  wend.numel() == wrow.numel(),
              "worklist: inconsistent array lengths (wrow ", wrow.numel(),
              ", wbeg ", wbeg.numel(), ", wend ", wend.numel(),
              ", wave_start ", wave_start.numel(), ")");
  const int n_waves = (int)wave_start.numel() - 1;
  TORCH_CHECK(n_waves % 8 == 0, "worklist: n_waves (", n_waves,
              ") must be a multiple of 8");
  return {{wrow.data_ptr<int32_t>(), wbeg.data_ptr<int64_t>(),
           wend.data_ptr<int64_t>(), wave_start.data_ptr<int32_t>()},
          n_waves};
}

// One work-list kernel launch: 256-thread blocks of 256 / subw waves (or
// subgroups) each; the schedule pointers lead the argument list.
template <typename K, typename... Args>
void launch_worklist(K kernel, const WorkListArgs& w, int subw,
                     Args... args) {
  hipLaunchKernelGGL(kernel, dim3(w.n_waves / (256 / subw)), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(), w.wl.row, w.wl.beg,
                     w.wl.end, w.wl.wave_start, args...);
}

// Kernel routing of spmm_sum for one source type. A bf16 source has the
// F % 4 == 0 kernels only: other widths are upcast by the caller
// (ops/functional.spmm_sum_raw) and take the fp32 route.
template <typename T>
void spmm_sum_route(const WorkListArgs& wl, const int32_t* indices,
                    const T* x, const float* ss, const float* ds, float* out,
                    int F, bool acc) {
  // f4 <= this runs the half-wave variant
  static const int subw32_max = env_int("BNSGCN_SPMM_SUBW32_MAX", 32);
  // f4 <= this runs the edge-parallel narrow kernel (0 disables it)
  static const int narrow_max =
      std::min(env_int("BNSGCN_SPMM_NARROW_MAX", 16), 16);
  auto launch = [&](auto kernel, int subw, int width) {
    launch_worklist(kernel, wl, subw, indices, x, ss, ds, out, width);
  };
  if (F % 4 == 0 && F / 4 <= std::min(narrow_max, subw32_max))
    launch(acc ? spmm_sum_narrow_kernel<T, true, 16>
               : spmm_sum_narrow_kernel<T, false, 16>, 64, F / 4);
  else if (F % 4 == 0 && F / 4 <= subw32_max)
    launch(acc ? spmm_sum_vec4_kernel<T, true, 32>
               : spmm_sum_vec4_kernel<T, false, 32>, 32, F / 4);
  else if (F % 4 == 0)
    launch(acc ? spmm_sum_vec4_kernel<T, true, 64>
               : spmm_sum_vec4_kernel<T, false, 64>, 64, F / 4);
  else if constexpr (std::is_same<T, float>::value) {
    if (F % 2 == 0)
      launch(acc ? spmm_sum_vec2_kernel<true> : spmm_sum_vec2_kernel<false>,
             64, F / 2);
    else
      launch(acc ? spmm_sum_scalar_kernel<true>
                 : spmm_sum_scalar_kernel<false>, 64, F);
  } else {
    TORCH_CHECK(false, "spmm_sum: a bf16 source covers F % 4 == 0, got F = ",
                F);
  }
}

at::Tensor spmm_sum(at::Tensor wrow, at::Tensor wbeg, at::Tensor wend,
                    at::Tensor wave_start, at::Tensor indices, at::Tensor x,
                    c10::optional<at::Tensor> src_scale,
                    c10::optional<at::Tensor> dst_scale,
                    at::Tensor out, bool acc) {
  // `out` is always caller-allocated: accumulate when acc, otherwise the
  // kernel overwrites every non-empty row (caller pre-zeroed split/empty
  // rows — ops/csr_torch.build_worklist zero_rows). x is fp32 or bf16,
  // out fp32 either way.
  check_src(x, "x");
  check_f32(out, "out");
  TORCH_CHECK(indices.scalar_type() == at::kInt, "indices int32 expected");
  const WorkListArgs wl = worklist_args(wrow, wbeg, wend, wave_start);
  const int F = x.size(1);
  TORCH_CHECK(out.dim() == 2 && out.size(1) == F, "out: [n_rows, F] expected");
  if (wrow.numel() == 0 || wl.n_waves <= 0) return out;
  if (x.scalar_type() == at::kBFloat16)
    spmm_sum_route(wl, indices.data_ptr<int32_t>(), bf16_ptr(x),
                   opt_ptr(src_scale), opt_ptr(dst_scale),
                   out.data_ptr<float>(), F, acc);
  else
    spmm_sum_route(wl, indices.data_ptr<int32_t>(), x.data_ptr<float>(),
                   opt_ptr(src_scale), opt_ptr(dst_scale),
                   out.data_ptr<float>(), F, acc);
  return out;
}

// Row-group SpMM (spmm_sum_grouped_kernel): same contract as spmm_sum on
// the format of ops/csr_torch.build_rowgroups — (wgroup, wbeg, wend,
// wave_start) schedule the entries (ecol, ew[n_entries, R]); `out` is
// caller-allocated with the builder's zero_rows pre-zeroed unless acc.
template <typename T, int R>
void launch_grouped(const WorkListArgs& wl, bool acc, int f4,
                    const at::Tensor& ecol, const at::Tensor& ew,
                    const T* x, const float* ss, const float* ds,
                    at::Tensor& out) {
  auto launch = [&](auto kernel) {
    launch_worklist(kernel, wl, 64, ecol.data_ptr<int32_t>(),
                    reinterpret_cast<const uint32_t*>(ew.data_ptr<uint8_t>()),
                    x, ss, ds, out.data_ptr<float>(), f4, (int)out.size(0));
  };
  if (f4 > 64)                      // a second float4 per lane
    launch(acc ? spmm_sum_grouped_kernel<T, true, R, 2>
               : spmm_sum_grouped_kernel<T, false, R, 2>);
  else
    launch(acc ? spmm_sum_grouped_kernel<T, true, R, 1>
               : spmm_sum_grouped_kernel<T, false, R, 1>);
}

template <typename T>
void route_grouped(int R, const WorkListArgs& wl, bool acc, int f4,
                   const at::Tensor& ecol, const at::Tensor& ew, const T* x,
                   const float* ss, const float* ds, at::Tensor& out) {
  switch (R) {
    case 4: launch_grouped<T, 4>(wl, acc, f4, ecol, ew, x, ss, ds, out); break;
    case 8: launch_grouped<T, 8>(wl, acc, f4, ecol, ew, x, ss, ds, out); break;
    // R = 16 was built and measured: slower than the per-row kernel at
    // every gseg (profiles/BENCH_SUMMARY_rowgroup.md), so not instantiated
    default: TORCH_CHECK(false, "spmm_sum_grouped: R must be 4 or 8, got ", R);
  }
}

at::Tensor spmm_sum_grouped(at::Tensor wgroup, at::Tensor wbeg,
                            at::Tensor wend, at::Tensor wave_start,
                            at::Tensor ecol, at::Tensor ew, at::Tensor x,
                            c10::optional<at::Tensor> src_scale,
                            c10::optional<at::Tensor> dst_scale,
                            at::Tensor out, bool acc) {
  check_src(x, "x");
  check_f32(out, "out");
  const WorkListArgs wl = worklist_args(wgroup, wbeg, wend, wave_start);
  TORCH_CHECK(ecol.scalar_type() == at::kInt && ecol.is_cuda() &&
                  ecol.is_contiguous(), "ecol: contiguous int32 expected");
  TORCH_CHECK(ew.scalar_type() == at::kByte && ew.is_cuda() &&
                  ew.is_contiguous() && ew.dim() == 2 &&
                  ew.size(0) == ecol.numel(),
              "ew: contiguous uint8 [n_entries, R] expected");
  const int R = (int)ew.size(1);
  const int F = x.size(1);
  TORCH_CHECK(F % 4 == 0 && F / 4 > 32,
              "spmm_sum_grouped covers F % 4 == 0 with F / 4 > 32, got F = ",
              F);
  TORCH_CHECK(out.dim() == 2 && out.size(1) == F, "out: [n_rows, F] expected");
  if (src_scale.has_value())
    TORCH_CHECK(src_scale->numel() == x.size(0), "src_scale: one per x row");
  if (dst_scale.has_value())
    TORCH_CHECK(dst_scale->numel() == out.size(0),
                "dst_scale: one per out row");
  if (wgroup.numel() == 0 || wl.n_waves <= 0) return out;
  const float* ss = opt_ptr(src_scale);
  const float* ds = opt_ptr(dst_scale);
  if (x.scalar_type() == at::kBFloat16)
    route_grouped(R, wl, acc, F / 4, ecol, ew, bf16_ptr(x), ss, ds, out);
  else
    route_grouped(R, wl, acc, F / 4, ecol, ew, x.data_ptr<float>(), ss, ds,
                  out);
  return out;
}

template <typename T>
void launch_pack(const T* x, const at::Tensor& idx, const float* scale,
                 at::Tensor& out, int n, int F) {
  auto stream = at::cuda::getCurrentCUDAStream();
  const int64_t total = (int64_t)n * F;
  const int grid = std::min<int64_t>((total + 255) / 256, 4096);
  if (F % 4 == 0) {
    hipLaunchKernelGGL(pack_rows_vec4_kernel<T>, dim3(grid), dim3(256), 0,
                       stream, x, idx.data_ptr<int64_t>(), scale,
                       out.data_ptr<float>(), n, F / 4);
  } else {
    hipLaunchKernelGGL(pack_rows_kernel<T>, dim3(grid), dim3(256), 0, stream,
                       x, idx.data_ptr<int64_t>(), scale,
                       out.data_ptr<float>(), n, F);
  }
}

at::Tensor pack_rows(at::Tensor x, at::Tensor idx,
                     c10::optional<at::Tensor> scale) {
  // x fp32 or bf16; the packed rows are fp32 either way
  check_src(x, "x");
  TORCH_CHECK(idx.scalar_type() == at::kLong, "idx must be int64");
  const int n = idx.numel(), F = x.size(1);
  auto out = at::empty({n, F}, x.options().dtype(at::kFloat));
  if (n == 0) return out;
  if (x.scalar_type() == at::kBFloat16)
    launch_pack(bf16_ptr(x), idx, opt_ptr(scale), out, n, F);
  else
    launch_pack(x.data_ptr<float>(), idx, opt_ptr(scale), out, n, F);
  return out;
}

// fp32 -> bf16 copy, round to nearest even (cast_bf16_kernel).
at::Tensor cast_bf16(at::Tensor x) {
  check_f32(x, "x");
  auto out = at::empty(x.sizes(), x.options().dtype(at::kBFloat16));
  const int64_t n = x.numel();
  if (n == 0) return out;
  // the float4 / uint2 accesses need the bases aligned; `out` is a fresh
  // allocation, x may be a view at an odd element offset
  const bool aligned = reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0;
  const int64_t n4 = aligned ? n / 4 : 0;
  const int64_t threads = n4 + (n - 4 * n4);
  const int grid = std::min<int64_t>((threads + 255) / 256, 8192);
  hipLaunchKernelGGL(cast_bf16_kernel, dim3(grid), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(), x.data_ptr<float>(),
                     reinterpret_cast<bf16_t*>(out.data_ptr<at::BFloat16>()),
                     n, n4);
  return out;
}

void scatter_add_rows(at::Tensor out, at::Tensor idx, at::Tensor src,
                      c10::optional<at::Tensor> scale) {
  check_f32(out, "out");
  check_f32(src, "src");
  const int n = idx.numel(), F = out.size(1);
  if (n == 0) return;
  auto stream = at::cuda::getCurrentCUDAStream();
  const int64_t total = (int64_t)n * F;
  const int grid = std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(scatter_add_rows_kernel, dim3(grid), dim3(256), 0, stream,
                     out.data_ptr<float>(), idx.data_ptr<int64_t>(),
                     src.data_ptr<float>(), opt_ptr(scale), n, F);
}

at::Tensor philox_keys(int64_t n, int64_t seed, int64_t epoch,
                       int64_t src_rank, int64_t dst_rank) {
  auto out = at::empty({n}, at::dtype(at::kLong).device(at::kCUDA));
  if (n == 0) return out;
  auto stream = at::cuda::getCurrentCUDAStream();
  const uint32_t sd = (((uint32_t)src_rank & 0xFFFF) << 16) |
                      ((uint32_t)dst_rank & 0xFFFF);
  hipLaunchKernelGGL(philox_keys_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     stream, out.data_ptr<int64_t>(), (int)n,
                     (uint32_t)(seed & 0xFFFFFFFF),
                     (uint32_t)((seed >> 32) & 0xFFFFFFFF),
                     (uint32_t)(epoch & 0xFFFFFFFF), sd);
  return out;
}

at::Tensor syncbn_stats(at::Tensor x) {
  check_f32(x, "x");
  const int64_t n = x.size(0);
  const int F = x.size(1);
  auto out = at::zeros({2, F}, x.options());
  if (n == 0 || F == 0) return out;  // no zero-sized grid dimension
  auto stream = at::cuda::getCurrentCUDAStream();
  // enough row-chunks to fill 256 CUs even for one 256-wide column block
  const int row_chunks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  dim3 grid((F + 255) / 256, row_chunks);
  hipLaunchKernelGGL(syncbn_stats_kernel, grid, dim3(256), 0, stream,
                     x.data_ptr<float>(), out.data_ptr<float>(), n, F,
                     row_chunks);
  return out;
}

std::vector<at::Tensor> ln_fwd(at::Tensor x, at::Tensor gamma,
                               at::Tensor beta, double eps, int64_t act) {
  check_f32(x, "x");
  check_f32(gamma, "gamma");
  check_f32(beta, "beta");
  const int64_t n = x.size(0);
  const int F = (int)x.size(1);
  TORCH_CHECK(F <= 64 * LN_MAX_K, "ln_fwd: F too large (", F, ")");
  auto y = at::empty_like(x);
  auto mean = at::empty({n}, x.options());
  auto rstd = at::empty({n}, x.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  const int blocks = (int)std::min<int64_t>((n + 3) / 4, 32768);
  if (F % 4 == 0) {
    hipLaunchKernelGGL(
        ln_fwd_v4_kernel, dim3(std::max(blocks, 1)), dim3(256), 0, stream,
        reinterpret_cast<const float4*>(x.data_ptr<float>()),
        reinterpret_cast<const float4*>(gamma.data_ptr<float>()),
        reinterpret_cast<const float4*>(beta.data_ptr<float>()),
        reinterpret_cast<float4*>(y.data_ptr<float>()),
        mean.data_ptr<float>(), rstd.data_ptr<float>(), n, F, (float)eps,
        (int)act);
    return {y, mean, rstd};
  }
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(std::max(blocks, 1)), dim3(256), 0,
                     stream, x.data_ptr<float>(), gamma.data_ptr<float>(),
                     beta.data_ptr<float>(), y.data_ptr<float>(),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), n, F,
                     (float)eps, (int)act);
  return {y, mean, rstd};
}

std::vector<at::Tensor> ln_bwd(at::Tensor x, at::Tensor dy, at::Tensor gamma,
                               at::Tensor beta, at::Tensor mean,
                               at::Tensor rstd, int64_t act) {
  check_f32(x, "x");
  check_f32(dy, "dy");
  const int64_t n = x.size(0);
  const int F = (int)x.size(1);
  auto dx = at::empty_like(x);
  auto dw = at::zeros({2, F}, x.options());
  if (n == 0 || F == 0) return {dx, dw[0], dw[1]};  // no zero-sized grid
  auto stream = at::cuda::getCurrentCUDAStream();
  const int blocks = (int)std::min<int64_t>((n + 3) / 4, 32768);
  if (F % 4 == 0) {
    hipLaunchKernelGGL(
        ln_bwd_dx_v4_kernel, dim3(std::max(blocks, 1)), dim3(256), 0,
        stream, reinterpret_cast<const float4*>(x.data_ptr<float>()),
        reinterpret_cast<const float4*>(dy.data_ptr<float>()),
        reinterpret_cast<const float4*>(gamma.data_ptr<float>()),
        reinterpret_cast<const float4*>(beta.data_ptr<float>()),
        mean.data_ptr<float>(), rstd.data_ptr<float>(),
        reinterpret_cast<float4*>(dx.data_ptr<float>()), n, F, (int)act);
  } else
  hipLaunchKernelGGL(ln_bwd_dx_kernel, dim3(std::max(blocks, 1)), dim3(256),
                     0, stream, x.data_ptr<float>(), dy.data_ptr<float>(),
                     gamma.data_ptr<float>(), beta.data_ptr<float>(),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),
                     dx.data_ptr<float>(), n, F, (int)act);
  const int row_chunks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  dim3 grid((F + 255) / 256, row_chunks);
  hipLaunchKernelGGL(ln_bwd_w_kernel, grid, dim3(256), 0, stream,
                     x.data_ptr<float>(), dy.data_ptr<float>(),
                     gamma.data_ptr<float>(), beta.data_ptr<float>(),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),
                     dw.data_ptr<float>(), n, F, row_chunks, (int)act);
  return {dx, dw[0], dw[1]};
}

at::Tensor dropout_apply(at::Tensor x, double keep, int64_t seed) {
  check_f32(x, "x");
  auto out = at::empty_like(x);
  const int64_t n = x.numel();
  if (n == 0) return out;
  auto stream = at::cuda::getCurrentCUDAStream();
  if (n % 4 == 0) {
    const int64_t n4 = n / 4;
    const int blocks = (int)std::min<int64_t>((n4 + 255) / 256, 32768);
    hipLaunchKernelGGL(dropout_apply_v4_kernel, dim3(blocks), dim3(256), 0,
                       stream,
                       reinterpret_cast<const float4*>(x.data_ptr<float>()),
                       reinterpret_cast<float4*>(out.data_ptr<float>()), n4,
                       (float)keep, (uint64_t)seed);
    return out;
  }
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 32768);
  hipLaunchKernelGGL(dropout_apply_kernel, dim3(blocks), dim3(256), 0,
                     stream, x.data_ptr<float>(), out.data_ptr<float>(), n,
                     (float)keep, (uint64_t)seed);
  return out;
}

at::Tensor bincount_i32(at::Tensor v, int64_t n_bins) {
  TORCH_CHECK(v.is_cuda() && v.scalar_type() == at::kInt, "int32 cuda input");
  auto out = at::zeros({n_bins}, v.options().dtype(at::kLong));
  if (v.numel() == 0) return out;
  auto stream = at::cuda::getCurrentCUDAStream();
  const int grid = std::min<int64_t>((v.numel() + 255) / 256, 4096);
  hipLaunchKernelGGL(bincount_i32_kernel, dim3(grid), dim3(256), 0, stream,
                     v.data_ptr<int32_t>(), v.numel(), out.data_ptr<int64_t>());
  return out;
}

at::Tensor sddmm_add(at::Tensor wrow, at::Tensor wbeg, at::Tensor wend,
                     at::Tensor wstart, at::Tensor indptr, at::Tensor indices,
                     at::Tensor el, at::Tensor er, double slope) {
  check_f32(el, "el"); check_f32(er, "er");
  const WorkListArgs wl = worklist_args(wrow, wbeg, wend, wstart);
  const int H = el.size(1);
  auto out = at::empty({indices.numel(), H}, el.options());
  if (indices.numel() == 0 || wl.n_waves <= 0) return out;
  launch_worklist(sddmm_add_kernel, wl, 64, indices.data_ptr<int32_t>(),
                  el.data_ptr<float>(), er.data_ptr<float>(),
                  out.data_ptr<float>(), H, (float)slope);
  return out;
}

at::Tensor segment_softmax(at::Tensor indptr, at::Tensor logits) {
  check_f32(logits, "logits");
  const int n_rows = indptr.numel() - 1;
  const int H = logits.size(1);
  auto out = at::empty_like(logits);
  if (logits.numel() == 0) return out;
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(segment_softmax_kernel, dim3(spmm_grid(n_rows * H)),
                     dim3(256), 0, stream, indptr.data_ptr<int64_t>(),
                     logits.data_ptr<float>(), out.data_ptr<float>(), n_rows, H);
  return out;
}

at::Tensor segment_softmax_backward(at::Tensor indptr, at::Tensor alpha,
                                    at::Tensor grad) {
  check_f32(alpha, "alpha"); check_f32(grad, "grad");
  const int n_rows = indptr.numel() - 1;
  const int H = alpha.size(1);
  auto out = at::empty_like(alpha);
  if (alpha.numel() == 0) return out;
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(segment_softmax_bwd_kernel, dim3(spmm_grid(n_rows * H)),
                     dim3(256), 0, stream, indptr.data_ptr<int64_t>(),
                     alpha.data_ptr<float>(), grad.data_ptr<float>(),
                     out.data_ptr<float>(), n_rows, H);
  return out;
}

std::vector<at::Tensor> segment_softmax2(at::Tensor ip1, at::Tensor l1,
                                         at::Tensor ip2, at::Tensor l2,
                                         double keep, int64_t seed) {
  check_f32(l1, "l1"); check_f32(l2, "l2");
  const int n_rows = ip1.numel() - 1;
  const int H = l1.size(1);
  // decided on the float the kernels receive (see drop_threshold)
  const bool drop = (float)keep < 1.0f;
  auto a1 = at::empty_like(l1);
  auto a2 = at::empty_like(l2);
  auto da1 = drop ? at::empty_like(l1) : a1;
  auto da2 = drop ? at::empty_like(l2) : a2;
  if (n_rows == 0) return {a1, a2, da1, da2};
  auto stream = at::cuda::getCurrentCUDAStream();
  if (H == 4) {   // float4-lane form: coalesced, same pass structure
    // short power-law segments are latency-bound: give each wave as few
    // serial rows as possible (the 16384-block worklist cap left ~11
    // rows chained per wave)
    const int g4 = (int)std::min<int64_t>(((int64_t)n_rows + 3) / 4, 65536);
    hipLaunchKernelGGL(segment_softmax2_h4_kernel,
                       dim3(std::max(g4, 1)), dim3(256), 0, stream,
                       ip1.data_ptr<int64_t>(),
                       reinterpret_cast<const float4*>(l1.data_ptr<float>()),
                       ip2.data_ptr<int64_t>(),
                       reinterpret_cast<const float4*>(l2.data_ptr<float>()),
                       reinterpret_cast<float4*>(a1.data_ptr<float>()),
                       reinterpret_cast<float4*>(a2.data_ptr<float>()),
                       reinterpret_cast<float4*>(da1.data_ptr<float>()),
                       reinterpret_cast<float4*>(da2.data_ptr<float>()),
                       n_rows, (float)keep, (uint64_t)seed, l1.numel());
    return {a1, a2, da1, da2};
  }
  hipLaunchKernelGGL(segment_softmax2_kernel, dim3(spmm_grid(n_rows * H)),
                     dim3(256), 0, stream, ip1.data_ptr<int64_t>(),
                     l1.data_ptr<float>(), ip2.data_ptr<int64_t>(),
                     l2.data_ptr<float>(), a1.data_ptr<float>(),
                     a2.data_ptr<float>(), da1.data_ptr<float>(),
                     da2.data_ptr<float>(), n_rows, H, (float)keep,
                     (uint64_t)seed, l1.numel());
  return {a1, a2, da1, da2};
}

std::vector<at::Tensor> segment_softmax2_backward(at::Tensor ip1, at::Tensor a1,
                                                  at::Tensor g1, at::Tensor ip2,
                                                  at::Tensor a2, at::Tensor g2,
                                                  double keep, int64_t seed) {
  const int n_rows = ip1.numel() - 1;
  const int H = a1.size(1);
  auto d1 = at::empty_like(a1);
  auto d2 = at::empty_like(a2);
  if (n_rows == 0) return {d1, d2};
  auto stream = at::cuda::getCurrentCUDAStream();
  if (H == 4) {
    const int g4 = (int)std::min<int64_t>(((int64_t)n_rows + 3) / 4, 65536);
    hipLaunchKernelGGL(segment_softmax2_h4_bwd_kernel,
                       dim3(std::max(g4, 1)), dim3(256), 0, stream,
                       ip1.data_ptr<int64_t>(),
                       reinterpret_cast<const float4*>(a1.data_ptr<float>()),
                       reinterpret_cast<const float4*>(g1.data_ptr<float>()),
                       ip2.data_ptr<int64_t>(),
                       reinterpret_cast<const float4*>(a2.data_ptr<float>()),
                       reinterpret_cast<const float4*>(g2.data_ptr<float>()),
                       reinterpret_cast<float4*>(d1.data_ptr<float>()),
                       reinterpret_cast<float4*>(d2.data_ptr<float>()),
                       n_rows, (float)keep, (uint64_t)seed, a1.numel());
    return {d1, d2};
  }
  hipLaunchKernelGGL(segment_softmax2_bwd_kernel, dim3(spmm_grid(n_rows * H)),
                     dim3(256), 0, stream, ip1.data_ptr<int64_t>(),
                     a1.data_ptr<float>(), g1.data_ptr<float>(),
                     ip2.data_ptr<int64_t>(), a2.data_ptr<float>(),
                     g2.data_ptr<float>(), d1.data_ptr<float>(),
                     d2.data_ptr<float>(), n_rows, H, (float)keep,
                     (uint64_t)seed, a1.numel());
  return {d1, d2};
}

at::Tensor spmm_edge_sum(at::Tensor wrow, at::Tensor wbeg, at::Tensor wend,
                         at::Tensor wstart, at::Tensor indptr,
                         at::Tensor indices, at::Tensor w,
                         c10::optional<at::Tensor> wperm, at::Tensor x,
                         at::Tensor out, bool acc) {
  // out is caller-allocated (split/empty rows pre-zeroed — see spmm_sum)
  check_f32(w, "w"); check_f32(x, "x"); check_f32(out, "out");
  const WorkListArgs wl = worklist_args(wrow, wbeg, wend, wstart);
  const int n_rows = indptr.numel() - 1;
  const int H = x.size(1), D = x.size(2);
  if (indices.numel() == 0 || n_rows == 0) return out;
  if (D % 4 == 0 && wl.n_waves > 0) {
    launch_worklist(acc ? spmm_edge_vec4_kernel<true>
                        : spmm_edge_vec4_kernel<false>,
                    wl, 64, indices.data_ptr<int32_t>(), w.data_ptr<float>(),
                    wperm.has_value() ? wperm->data_ptr<int64_t>() : nullptr,
                    x.data_ptr<float>(), out.data_ptr<float>(), H, D / 4,
                    H * D / 4);
    return out;
  }
  if (wperm.has_value()) w = w.index_select(0, *wperm);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto kfn = acc ? spmm_edge_kernel<true> : spmm_edge_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3(spmm_grid(n_rows * H)), dim3(256), 0, stream,
                     indptr.data_ptr<int64_t>(), indices.data_ptr<int32_t>(),
                     w.data_ptr<float>(), x.data_ptr<float>(),
                     out.data_ptr<float>(), n_rows, H, D);
  return out;
}

at::Tensor sddmm_dot(at::Tensor wrow, at::Tensor wbeg, at::Tensor wend,
                     at::Tensor wstart, at::Tensor indptr, at::Tensor indices,
                     at::Tensor g, at::Tensor x) {
  check_f32(g, "g"); check_f32(x, "x");
  const WorkListArgs wl = worklist_args(wrow, wbeg, wend, wstart);
  const int H = x.size(1), D = x.size(2);
  const int HD = H * D;
  auto out = at::empty({indices.numel(), H}, x.options());
  if (indices.numel() == 0 || wl.n_waves <= 0) return out;
  const int grp = D / 8;
  const bool fast = HD <= 512 && D % 8 == 0 && grp > 0 &&
                    (grp & (grp - 1)) == 0;
  launch_worklist(fast ? sddmm_dot_fast_kernel
                       : D % 4 == 0 ? sddmm_dot_vec4_kernel
                                    : sddmm_dot_gen_kernel,
                  wl, 64, indices.data_ptr<int32_t>(), g.data_ptr<float>(),
                  x.data_ptr<float>(), out.data_ptr<float>(), H, D, HD);
  return out;
}

at::Tensor segment_sum_edges(at::Tensor wrow, at::Tensor wbeg, at::Tensor wend,
                             at::Tensor wstart,
                             c10::optional<at::Tensor> perm, at::Tensor grad,
                             int64_t n_rows) {
  check_f32(grad, "grad");
  const int H = grad.size(1);
  TORCH_CHECK(H <= 8, "segment_sum_edges supports H <= 8");
  const WorkListArgs wl = worklist_args(wrow, wbeg, wend, wstart);
  auto out = at::zeros({n_rows, H}, grad.options());
  if (wl.n_waves <= 0 || wrow.numel() == 0) return out;
  const int64_t* pp = perm.has_value() ? perm->data_ptr<int64_t>() : nullptr;
  if (H == 4)
    launch_worklist(segment_sum_edges_h4_kernel, wl, 64, pp,
                    reinterpret_cast<const float4*>(grad.data_ptr<float>()),
                    reinterpret_cast<float4*>(out.data_ptr<float>()));
  else
    launch_worklist(segment_sum_edges_kernel, wl, 64, pp,
                    grad.data_ptr<float>(), out.data_ptr<float>(), H);
  return out;
}

std::vector<at::Tensor> attn_project(at::Tensor z, at::Tensor al,
                                     at::Tensor ar) {
  check_f32(z, "z");
  const int64_t n = z.size(0);
  const int H = z.size(1), D = z.size(2);
  TORCH_CHECK(H <= 8 && (H * D) % 4 == 0, "attn_project shape limits");
  auto el = at::empty({n, H}, z.options());
  auto er = at::empty({n, H}, z.options());
  if (n == 0) return {el, er};
  auto stream = at::cuda::getCurrentCUDAStream();
  auto kfn = (D % 4 == 0) ? attn_project_fwd_kernel<true>
                          : attn_project_fwd_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3(spmm_grid((int)std::min<int64_t>(n, 1 << 28))),
                     dim3(256), 0, stream, z.data_ptr<float>(),
                     al.data_ptr<float>(), ar.data_ptr<float>(),
                     el.data_ptr<float>(), er.data_ptr<float>(), n, H, D,
                     H * D / 4);
  return {el, er};
}

std::vector<at::Tensor> attn_project_backward(at::Tensor z, at::Tensor al,
                                              at::Tensor ar, at::Tensor g_el,
                                              at::Tensor g_er) {
  check_f32(z, "z");
  const int64_t n = z.size(0);
  const int H = z.size(1), D = z.size(2);
  const int HD = H * D;
  TORCH_CHECK(H <= 8 && HD % 4 == 0, "attn_project shape limits");
  auto dz = at::empty_like(z);
  auto dal = at::zeros({1, H, D}, z.options());
  auto dar = at::zeros({1, H, D}, z.options());
  if (n == 0) return {dz, dal, dar};
  auto stream = at::cuda::getCurrentCUDAStream();
  auto kfn = (D % 4 == 0) ? attn_project_dz_kernel<true>
                          : attn_project_dz_kernel<false>;
  hipLaunchKernelGGL(kfn,
                     dim3(spmm_grid((int)std::min<int64_t>(n, 1 << 28))),
                     dim3(256), 0, stream, al.data_ptr<float>(),
                     ar.data_ptr<float>(), g_el.data_ptr<float>(),
                     g_er.data_ptr<float>(), dz.data_ptr<float>(), n, H, D,
                     HD / 4);
  const int row_chunks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  dim3 grid((HD + 255) / 256, row_chunks);
  hipLaunchKernelGGL(attn_project_dattn_kernel, grid, dim3(256), 0, stream,
                     z.data_ptr<float>(), g_el.data_ptr<float>(),
                     g_er.data_ptr<float>(), dal.data_ptr<float>(),
                     dar.data_ptr<float>(), n, H, D, HD, row_chunks);
  return {dz, dal, dar};
}

at::Tensor gemm_strided(const at::Tensor& A, int64_t sAm, int64_t sAk,
                        const at::Tensor& B, int64_t sBk, int64_t sBn,
                        const c10::optional<at::Tensor>& bias,
                        int M, int N, int K) {
  auto stream = at::cuda::getCurrentCUDAStream();
  if (M == 0 || N == 0) return at::zeros({M, N}, A.options());
  if (K == 0) {
    auto C = at::zeros({M, N}, A.options());
    if (bias.has_value()) C += *bias;
    return C;
  }
  dim3 grid((M + BM - 1) / BM, (N + BN - 1) / BN);
  // split-K when the M/N tile grid alone cannot fill the 256 CUs (dW
  // reductions: C is tiny, K is the node count)
  const int base_blocks = grid.x * grid.y;
  int splitk = 1;
  if (base_blocks < 256 && K > 4 * BK) {
    splitk = std::min({(int)(768 / base_blocks), (K + 255) / 256, 64});
    splitk = std::max(splitk, 1);
  }
  if (splitk > 1) {
    auto C = at::zeros({M, N}, A.options());
    const int k_slice = ((K + splitk - 1) / splitk + BK - 1) / BK * BK;
    grid.z = (K + k_slice - 1) / k_slice;
    hipLaunchKernelGGL(gemm_f32_kernel<true>, grid, dim3(256), 0, stream,
                       A.data_ptr<float>(), sAm, sAk, B.data_ptr<float>(), sBk,
                       sBn, opt_ptr(bias), C.data_ptr<float>(), M, N, K, k_slice);
    return C;
  }
  auto C = at::empty({M, N}, A.options());
  hipLaunchKernelGGL(gemm_f32_kernel<false>, grid, dim3(256), 0, stream,
                     A.data_ptr<float>(), sAm, sAk, B.data_ptr<float>(), sBk,
                     sBn, opt_ptr(bias), C.data_ptr<float>(), M, N, K, K);
  return C;
}

// Kernel choice of the three public GEMMs. `kernel`: GEMM_AUTO routes by
// shape, GEMM_OLD / GEMM_TILED force gemm_f32_kernel / the tiled kernel
// (gemm_tiled.hip) at any shape — for tests and A/B timing.
// Auto takes the tiled kernel when its float4 staging applies (16-byte
// aligned rows) and its 128x128 tile pads the output no more than 25 %
// beyond what the 64x64 tile does: 41-wide or K % 4 != 0 operands and
// small or narrow outputs (N = 44 pads to 128 against 64) stay on
// gemm_f32_kernel.
enum { GEMM_AUTO = 0, GEMM_OLD = 1, GEMM_TILED = 2 };

bool route_tiled(bns::GemmLayout layout, const at::Tensor& A,
                 const at::Tensor& B, int M, int N, int R, int64_t kernel) {
  TORCH_CHECK(kernel >= GEMM_AUTO && kernel <= GEMM_TILED, "bad kernel id");
  if (kernel == GEMM_OLD || M == 0 || N == 0 || R == 0) return false;
  if (kernel == GEMM_TILED) return true;
  if (!bns::gemm_tiled_aligned(layout, A, B, M, N, R) || R < 32) return false;
  auto pad = [](int64_t v, int64_t t) { return (v + t - 1) / t * t; };
  return 4 * pad(M, 128) * pad(N, 128) <= 5 * pad(M, BM) * pad(N, BN);
}

// y[M,N] = x[M,K] @ w[N,K]^T + b
at::Tensor gemm_nt_bias(at::Tensor x, at::Tensor w,
                        c10::optional<at::Tensor> bias, int64_t kernel) {
  check_f32(x, "x"); check_f32(w, "w");
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "shape mismatch");
  if (route_tiled(bns::GEMM_NT, x, w, M, N, K, kernel))
    return bns::gemm_tiled(bns::GEMM_NT, x, w, bias, M, N, K);
  return gemm_strided(x, K, 1, w, 1, K, bias, M, N, K);
}

// dx[M,K] = g[M,N] @ w[N,K]
at::Tensor gemm_nn(at::Tensor g, at::Tensor w, int64_t kernel) {
  check_f32(g, "g"); check_f32(w, "w");
  const int M = g.size(0), N = g.size(1), K = w.size(1);
  TORCH_CHECK(w.size(0) == N, "shape mismatch");
  if (route_tiled(bns::GEMM_NN, g, w, M, K, N, kernel))
    return bns::gemm_tiled(bns::GEMM_NN, g, w, c10::nullopt, M, K, N);
  return gemm_strided(g, N, 1, w, K, 1, c10::nullopt, M, K, N);
}

// dw[N,K] = g[M,N]^T @ x[M,K]
at::Tensor gemm_tn(at::Tensor g, at::Tensor x, int64_t kernel) {
  check_f32(g, "g"); check_f32(x, "x");
  const int M = g.size(0), N = g.size(1), K = x.size(1);
  TORCH_CHECK(x.size(0) == M, "shape mismatch");
  if (route_tiled(bns::GEMM_TN, g, x, N, K, M, kernel))
    return bns::gemm_tiled(bns::GEMM_TN, g, x, c10::nullopt, N, K, M);
  return gemm_strided(g, 1, N, x, K, 1, c10::nullopt, N, K, M);
}

// Dropout fused into the activation operand (tiled kernel only): the
// operand x is read as drop_apply(x[m, k], m*K + k, ...) while it is
// staged — the values entering the MFMAs are bit-identical to
// dropout_apply(x, keep, seed), which is never materialized.
// y[M,N] = dropout(x)[M,K] @ w[N,K]^T + b
at::Tensor gemm_nt_bias_drop(at::Tensor x, at::Tensor w,
                             c10::optional<at::Tensor> bias, double keep,
                             int64_t seed) {
  check_f32(x, "x"); check_f32(w, "w");
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "shape mismatch");
  if (M == 0 || N == 0 || K == 0)
    return gemm_strided(x, K, 1, w, 1, K, bias, M, N, K);
  return bns::gemm_tiled(bns::GEMM_NT, x, w, bias, M, N, K, bns::DROP_A,
                         (float)keep, (uint64_t)seed);
}

// dw[N,K] = g[M,N]^T @ dropout(x)[M,K]
at::Tensor gemm_tn_drop(at::Tensor g, at::Tensor x, double keep,
                        int64_t seed) {
  check_f32(g, "g"); check_f32(x, "x");
  const int M = g.size(0), N = g.size(1), K = x.size(1);
  TORCH_CHECK(x.size(0) == M, "shape mismatch");
  if (M == 0 || N == 0 || K == 0)
    return gemm_strided(g, 1, N, x, K, 1, c10::nullopt, N, K, M);
  return bns::gemm_tiled(bns::GEMM_TN, g, x, c10::nullopt, N, K, M,
                         bns::DROP_B, (float)keep, (uint64_t)seed);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("spmm_sum", &spmm_sum, "CSR SpMM sum with fused src/dst scales");
  m.def("spmm_sum_grouped", &spmm_sum_grouped,
        "row-group CSR SpMM sum with fused src/dst scales");
  m.def("pack_rows", &pack_rows, "gather rows + per-row scale");
  m.def("cast_bf16", &cast_bf16, "fp32 -> bf16 copy, round to nearest even");
  m.def("scatter_add_rows", &scatter_add_rows, "scatter-add rows + scale");
  m.def("philox_keys", &philox_keys, "BNS sampling keys (Philox4x32-10)");
  m.def("syncbn_stats", &syncbn_stats, "column sum + sum of squares");
  // kernel: 0 = routed by shape, 1 = 64x64 kernel, 2 = tiled 128x128 kernel
  m.def("gemm_nt_bias", &gemm_nt_bias, "fp32 MFMA GEMM x@w^T+b",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("kernel") = 0);
  m.def("gemm_nn", &gemm_nn, "fp32 MFMA GEMM g@w", py::arg("g"),
        py::arg("w"), py::arg("kernel") = 0);
  m.def("gemm_tn", &gemm_tn, "fp32 MFMA GEMM g^T@x", py::arg("g"),
        py::arg("x"), py::arg("kernel") = 0);
  m.def("gemm_nt_bias_drop", &gemm_nt_bias_drop,
        "tiled GEMM dropout(x)@w^T+b, dropout fused into the operand load");
  m.def("gemm_tn_drop", &gemm_tn_drop,
        "tiled GEMM g^T@dropout(x), dropout fused into the operand load");
  m.def("sddmm_add", &sddmm_add, "GAT u_add_v SDDMM");
  m.def("segment_softmax", &segment_softmax, "edge softmax by dst segment");
  m.def("segment_softmax_backward", &segment_softmax_backward,
        "edge softmax backward");
  m.def("segment_softmax2", &segment_softmax2,
        "union softmax over two edge sets (split GAT block)");
  m.def("segment_softmax2_backward", &segment_softmax2_backward,
        "union softmax backward");
  m.def("spmm_edge_sum", &spmm_edge_sum, "multi-head edge-weighted SpMM");
  m.def("sddmm_dot", &sddmm_dot, "per-edge per-head dot (spmm_edge grad)");
  m.def("bincount_i32", &bincount_i32, "atomic int32 histogram");
  m.def("ln_fwd", &ln_fwd, "row LayerNorm forward (y, mean, rstd); "
        "act=1 fuses ReLU");
  m.def("ln_bwd", &ln_bwd, "row LayerNorm backward (dx, dgamma, dbeta)");
  m.def("dropout_apply", &dropout_apply,
        "mask-free dropout (splitmix64; same kernel fwd and bwd)");
  m.def("attn_project", &attn_project, "fused GAT el/er projections");
  m.def("attn_project_backward", &attn_project_backward,
        "fused GAT projection backward");
  m.def("segment_sum_edges", &segment_sum_edges,
        "segment sum of (permuted) edge values by CSR row");
}
