// Common device helpers for the bnsgcn_amd gfx950 kernel library.
// CDNA4: wavefront = 64 lanes, 4 waves per 256-thread block.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define WAVE 64
#define DEV_INLINE __device__ __forceinline__

// ------------------------------------------------------------- work-list
// View of the edge-balanced schedule built by
// ops/csr_torch.build_worklist. Item `it` covers edges [beg[it], end[it])
// of one destination row; wave (or SUBW-lane subgroup) w owns the
// contiguous items wave_start[w] .. wave_start[w+1]. Two contracts with
// the builder live here and nowhere else:
//  * a row split over several items is stored bitwise NEGATED: its items
//    combine with atomicAdd, every other row has one item and one writer;
//  * n_waves is a multiple of 8, so a grid of 256-thread blocks (4 waves,
//    or 8 half-wave subgroups) covers every wave exactly — the launchers
//    check it (worklist_args in kernels.hip).
struct WorkList {
  const int32_t* __restrict__ row;
  const int64_t* __restrict__ beg;
  const int64_t* __restrict__ end;
  const int32_t* __restrict__ wave_start;
};

struct WaveItems { int lane, beg, end; };            // lane within SUBW
struct WorkItem { int row; bool atomic; int64_t beg, end; };

// XCD-aware bijective block remap (dispatcher places block b on XCD b%8):
// XCD x gets a CONTIGUOUS range of logical blocks, so consecutive waves on
// one chiplet touch consecutive worklist items -> dst-row locality in the
// XCD-private L2 (cdna_hip_programming.md T1; bijective form for nb%8!=0).
DEV_INLINE int xcd_remap_block(int b, int nb) {
  const int q = nb / 8, r = nb % 8;
  const int xcd = b % 8, j = b / 8;
  return (xcd < r) ? xcd * (q + 1) + j : r * (q + 1) + (xcd - r) * q + j;
}

// Item range of the calling wave (SUBW = 64) or half-wave subgroup (32).
template <int SUBW>
DEV_INLINE WaveItems wave_items(const WorkList& wl) {
  const int bb = xcd_remap_block(blockIdx.x, gridDim.x);
  const int w = bb * (blockDim.x / SUBW) + (threadIdx.x / SUBW);
  return {(int)(threadIdx.x & (SUBW - 1)), wl.wave_start[w],
          wl.wave_start[w + 1]};
}

DEV_INLINE WorkItem work_item(const WorkList& wl, int it) {
  const int row = wl.row[it];
  const bool atomic = row < 0;
  return {atomic ? ~row : row, atomic, wl.beg[it], wl.end[it]};
}

// One SUBW-edge chunk [e0, min(e0 + SUBW, end)): lane l holds column id
// (and src scale) of edge e0 + l from ONE coalesced load each; consumers
// broadcast them with __shfl(., k, SUBW) for k < nv.
struct Chunk { int cid; float ssc; int nv; };

template <int SUBW>
DEV_INLINE Chunk load_chunk(const int32_t* __restrict__ indices,
                            const float* __restrict__ src_scale, int64_t e0,
                            int64_t end, int lane) {
  Chunk c = {0, 1.0f, (int)((end - e0 < SUBW) ? (end - e0) : SUBW)};
  if (lane < c.nv) {
    c.cid = indices[e0 + lane];
    if (src_scale) c.ssc = src_scale[c.cid];
  }
  return c;
}

// ------------------------------------------------------------ source rows
// Element type of a gathered source matrix: float, or bf16 carried as its
// 16 raw bits (--agg-dtype bf16: the source operand was rounded once by
// cast_bf16_kernel, everything after the load is fp32). load_src4(x, i)
// returns elements 4i .. 4i+3 as fp32: one 16-byte load for float, one
// 8-byte load for bf16. bf16 -> fp32 is exact (the 16 bits are the high
// half of the fp32 word), so the expansion is a shift or a mask and a
// kernel templated on the source type differs in the load alone.
typedef uint16_t bf16_t;

DEV_INLINE float4 load_src4(const float* __restrict__ x, int64_t i) {
  return reinterpret_cast<const float4*>(x)[i];
}
DEV_INLINE float4 load_src4(const bf16_t* __restrict__ x, int64_t i) {
  const uint2 p = reinterpret_cast<const uint2*>(x)[i];
  return make_float4(__uint_as_float(p.x << 16),
                     __uint_as_float(p.x & 0xffff0000u),
                     __uint_as_float(p.y << 16),
                     __uint_as_float(p.y & 0xffff0000u));
}
DEV_INLINE float load_src1(const float* __restrict__ x, int64_t i) {
  return x[i];
}
DEV_INLINE float load_src1(const bf16_t* __restrict__ x, int64_t i) {
  return __uint_as_float((uint32_t)x[i] << 16);
}

// fp32 -> bf16 bits, round to nearest even, in integer arithmetic so that
// denormals round like every other value whatever the FP mode: add 0x7fff
// plus the lowest kept bit, keep the high half. The carry does the rest —
// a tie goes to the even neighbour, the largest finite fp32 becomes inf,
// +-inf and +-0 pass through. NaN (which the add could turn into inf) is
// the quiet NaN 0x7fc0, as torch's scalar conversion gives.
DEV_INLINE uint32_t bf16_rne_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// ------------------------------------------------------------- row store
DEV_INLINE void atomic_add(float* p, float v) { atomicAdd(p, v); }
DEV_INLINE void atomic_add(float2* p, float2 v) {
  float* f = reinterpret_cast<float*>(p);
  atomicAdd(f + 0, v.x); atomicAdd(f + 1, v.y);
}
DEV_INLINE void atomic_add(float4* p, float4 v) {
  float* f = reinterpret_cast<float*>(p);
  atomicAdd(f + 0, v.x); atomicAdd(f + 1, v.y);
  atomicAdd(f + 2, v.z); atomicAdd(f + 3, v.w);
}

// Write-out of s * v, one work item's result: split rows (atomic) combine
// with atomicAdd, otherwise accumulate (ACC) or overwrite. The row scale
// s is applied HERE because the accumulate form is one fused multiply-add
// per element (*dst + s * v, rounded once) — passing in an already
// rounded product would change the last bit of every accumulated row.
template <bool ACC>
DEV_INLINE void store_row(float* dst, float v, bool atomic, float s = 1.0f) {
  if (atomic) atomic_add(dst, s * v);
  else if (ACC) *dst = fmaf(s, v, *dst);
  else *dst = s * v;
}
template <bool ACC>
DEV_INLINE void store_row(float2* dst, float2 v, bool atomic, float s = 1.0f) {
  if (atomic) {
    atomic_add(dst, make_float2(s * v.x, s * v.y));
  } else if (ACC) {
    const float2 pv = *dst;
    *dst = make_float2(fmaf(s, v.x, pv.x), fmaf(s, v.y, pv.y));
  } else {
    *dst = make_float2(s * v.x, s * v.y);
  }
}
template <bool ACC>
DEV_INLINE void store_row(float4* dst, float4 v, bool atomic, float s = 1.0f) {
  if (atomic) {
    atomic_add(dst, make_float4(s * v.x, s * v.y, s * v.z, s * v.w));
  } else if (ACC) {
    const float4 pv = *dst;
    *dst = make_float4(fmaf(s, v.x, pv.x), fmaf(s, v.y, pv.y),
                       fmaf(s, v.z, pv.z), fmaf(s, v.w, pv.w));
  } else {
    *dst = make_float4(s * v.x, s * v.y, s * v.z, s * v.w);
  }
}

// ---------------------------------------------------------------- Philox
// Philox4x32-10 — MUST match bnsgcn_amd/ops/philox.py bitwise (tests
// assert equality). Key layout documented there.
DEV_INLINE uint32_t mulhi32(uint32_t a, uint32_t b) {
  return (uint32_t)(((uint64_t)a * b) >> 32);
}

struct P4 { uint32_t c0, c1, c2, c3; };

DEV_INLINE P4 philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                         uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  const uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0 = mulhi32(c0, M0), lo0 = c0 * M0;
    uint32_t hi1 = mulhi32(c2, M1), lo1 = c2 * M1;
    uint32_t n0 = hi1 ^ c1 ^ k0;
    uint32_t n1 = lo1;
    uint32_t n2 = hi0 ^ c3 ^ k1;
    uint32_t n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += W0; k1 += W1;
  }
  return {c0, c1, c2, c3};
}

// --------------------------------------------------------------- dropout
// Dropout mask (attention dropout fused into the union softmax, feature
// dropout, and the dropout fused into the tiled GEMM's operand staging —
// kernels.hip, gemm_tiled.hip): element idx keeps its value iff splitmix64(seed + idx) high bits < keep * 2^32. The mask is
// REGENERATED in backward from (seed, idx) — never stored. splitmix64
// (~8 ALU ops) instead of Philox4x32-10: the softmax kernel is
// latency-bound over short segments and the 10-round Philox measured
// +1.6 ms on the Yelp GAT backward (profiles/topk_gat2_r02.txt).
DEV_INLINE bool drop_keep(int64_t idx, uint32_t thr, uint64_t seed) {
  uint64_t z = seed + (uint64_t)idx;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> 32) < thr;
}

// `keep` reaches every kernel as a float, and dropout is active iff THAT
// float is below 1: a double just under 1 rounds to exactly 1.0f, and
// 1.0f * 2^32 does not fit a uint32_t (the conversion is undefined). The
// launchers decide on the same rounded value, so the kernels and the
// allocation of da1/da2 cannot disagree. keep <= 0 drops everything.
DEV_INLINE uint32_t drop_threshold(float keep) {
  return (keep > 0.f && keep < 1.0f)
             ? (uint32_t)((double)keep * 4294967296.0) : 0u;
}

// Dropout of one value / one float4 whose first component has flat mask
// index idx: kept elements are scaled by 1/keep, dropped ones are 0.
DEV_INLINE float drop_apply(float v, int64_t idx, uint32_t thr, uint64_t seed,
                            float inv_keep) {
  return drop_keep(idx, thr, seed) ? v * inv_keep : 0.f;
}

DEV_INLINE float4 drop_apply(float4 v, int64_t idx, uint32_t thr,
                             uint64_t seed, float inv_keep) {
  return make_float4(drop_apply(v.x, idx + 0, thr, seed, inv_keep),
                     drop_apply(v.y, idx + 1, thr, seed, inv_keep),
                     drop_apply(v.z, idx + 2, thr, seed, inv_keep),
                     drop_apply(v.w, idx + 3, thr, seed, inv_keep));
}
