// Tiled fp32 MFMA GEMM for the compute-bound dense shapes (K6, second
// kernel): exact fp32 on v_mfma_f32_32x32x2_f32 (lane l holds
// A[i=l&31][k=l>>5] and B[k=l>>5][j=l&31]; C/D col=l&31,
// row=(reg&3)+8*(reg>>2)+4*(l>>5) — cdna_hip_programming.md §3).
//
// * 128x128 block tile, 4 waves, each owning a 64x64 quadrant as 2x2
//   accumulators of 32x32 (64 accumulator registers, 4 independent MFMA
//   chains per wave).
// * K-tile of 16, double-buffered in LDS: the next tile is fetched into
//   registers with 16-byte global loads while the MFMAs run, then written
//   to the other buffer — one barrier per K-tile.
// * Two LDS images, chosen per operand by which of its dimensions is
//   contiguous in memory, so staging is always a float4 load and a
//   ds_write_b128 without a transpose:
//     KC (reduction index contiguous: x and w in NT, g in NN):
//        image [128 rows][16 + 4 pad]; a lane fetches k = 8g+4h .. +3 of
//        its row with ONE ds_read_b128 (h = lane>>5) — the operands of 4
//        consecutive MFMAs. Row stride 20 = 4*odd: the 16 lanes of a
//        ds_read_b128 group hit 16 distinct 4-bank slots.
//     KS (reduction index strided: w in NN, g and x in TN):
//        image [16 k][128 rows]; a lane fetches rows 2i, 2i+1 of k-row
//        8g+4h+s with ONE ds_read_b64 — the operands of BOTH of its
//        32x32 tiles. The wave's tile f therefore owns rows 2i+f (not
//        32f+i); the epilogue undoes that.
//   Both images use the same k order inside a group of 8 (MFMA step s
//   sums k = 8g+s and 8g+4+s), so any pair combines; it only reorders
//   the fp32 sum.
// * Dropout fused into the staging (DROP_A / DROP_B): the staged float4
//   becomes drop_apply(v, flat offset, ...) — bit-identical to what
//   dropout_apply would have written, so the dropped copy never exists.
// * VEC=false replaces the float4 global loads by guarded scalar loads for
//   operands whose rows are not 16-byte aligned; same images, same math.
#include <hip/hip_runtime.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/util/Exception.h>
#include <algorithm>
#include "common.h"
#include "gemm_tiled.h"

namespace {

constexpr int TBM = 128, TBN = 128, TBK = 16;
constexpr int KC_LD = TBK + 4;            // floats per KC image row
constexpr int KS_LD = 128;                // floats per KS image k-row
constexpr int KC_TILE = 128 * KC_LD;      // floats per KC K-tile image
constexpr int KS_TILE = TBK * KS_LD;

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct DropArgs { uint32_t thr; uint64_t seed; float inv_keep; };

// Tile-local coordinates (row, k) of the first element of this thread's
// j-th float4 (2 per operand per K-tile: 128 * 16 / 4 / 256).
template <bool KC>
DEV_INLINE void stage_coords(int tid, int j, int& row, int& k) {
  if (KC) { row = (tid >> 2) + 64 * j; k = (tid & 3) * 4; }
  else    { k = (tid >> 5) + 8 * j;    row = (tid & 31) * 4; }
}

// Global -> registers. P is [R rows][ld] (KC) or [k][ld] (KS); elements
// outside rows < R, k < ke read as 0.
template <bool KC, bool VEC>
DEV_INLINE void stage_load(const float* __restrict__ P, int64_t ld, int r0,
                           int R, int k0, int ke, int tid, float4 (&v)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int row, k;
    stage_coords<KC>(tid, j, row, k);
    const int gr = r0 + row, gk = k0 + k;
    const float* p = KC ? P + (int64_t)gr * ld + gk : P + (int64_t)gk * ld + gr;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (VEC) {
      // the contiguous extent is a multiple of 4 and gr/gk are too, so a
      // float4 is wholly inside or wholly outside
      if (gr < R && gk < ke) t = *reinterpret_cast<const float4*>(p);
    } else {
      const int lim = KC ? ((gr < R) ? ke - gk : 0) : ((gk < ke) ? R - gr : 0);
      if (lim > 0) t.x = p[0];
      if (lim > 1) t.y = p[1];
      if (lim > 2) t.z = p[2];
      if (lim > 3) t.w = p[3];
    }
    v[j] = t;
  }
}

// Registers -> LDS image, with the fused dropout (mask index = the
// operand's flat element offset, 64-bit).
template <bool KC, bool DROP>
DEV_INLINE void stage_store(float* __restrict__ S, int64_t ld, int r0, int k0,
                            int tid, const float4 (&v)[2], const DropArgs& d) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int row, k;
    stage_coords<KC>(tid, j, row, k);
    float4 t = v[j];
    if (DROP) {
      const int64_t idx = KC ? (int64_t)(r0 + row) * ld + (k0 + k)
                             : (int64_t)(k0 + k) * ld + (r0 + row);
      t = drop_apply(t, idx, d.thr, d.seed, d.inv_keep);
    }
    *reinterpret_cast<float4*>(S + (KC ? row * KC_LD + k : k * KS_LD + row)) = t;
  }
}

// Operands of MFMA steps s = 0..3 of k-group g for both of the wave's
// tiles f: o[s][f]. wo = the wave's 64-row offset inside the block tile.
template <bool KC>
DEV_INLINE void frag_read(const float* __restrict__ S, int wo, int i, int h,
                          int g, float (&o)[4][2]) {
  if (KC) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float4 t = *reinterpret_cast<const float4*>(
          S + (wo + f * 32 + i) * KC_LD + 8 * g + 4 * h);
      o[0][f] = t.x; o[1][f] = t.y; o[2][f] = t.z; o[3][f] = t.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float2 t = *reinterpret_cast<const float2*>(
          S + (8 * g + 4 * h + s) * KS_LD + wo + 2 * i);
      o[s][0] = t.x; o[s][1] = t.y;
    }
  }
}

// Tile-local index (0..63 inside the wave's quadrant) of element idx of
// the wave's tile f — the inverse of frag_read's row assignment.
template <bool KC>
DEV_INLINE int frag_index(int f, int idx) {
  return KC ? f * 32 + idx : 2 * idx + f;
}

template <bool A_KC, bool B_KC, bool VEC, int DROP, bool ATOMIC>
__global__ __launch_bounds__(256)
void gemm_tiled_kernel(const float* __restrict__ A, int64_t lda,
                       const float* __restrict__ B, int64_t ldb,
                       const float* __restrict__ bias, float* __restrict__ C,
                       int M, int N, int K, int k_slice, int tiles_n,
                       DropArgs drop) {
  constexpr int A_TILE = A_KC ? KC_TILE : KS_TILE;
  constexpr int B_TILE = B_KC ? KC_TILE : KS_TILE;
  // ONE LDS object (both operands, both buffers)
  __shared__ __attribute__((aligned(16))) float lds[2 * (A_TILE + B_TILE)];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int wr = (wid >> 1) * 64, wc = (wid & 1) * 64;
  const int i_l = lane & 31, h_l = lane >> 5;
  // N-tile fastest: the blocks sharing an A tile are neighbours in time
  const int m0 = (blockIdx.x / tiles_n) * TBM;
  const int n0 = (blockIdx.x % tiles_n) * TBN;
  const int kb = blockIdx.y * k_slice;
  const int ke = (kb + k_slice < K) ? kb + k_slice : K;

  float4 ra[2], rb[2];
  f32x16 acc[2][2];
#pragma unroll
  for (int fi = 0; fi < 2; ++fi)
#pragma unroll
    for (int fj = 0; fj < 2; ++fj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[fi][fj][r] = 0.f;

  stage_load<A_KC, VEC>(A, lda, m0, M, kb, ke, tid, ra);
  stage_load<B_KC, VEC>(B, ldb, n0, N, kb, ke, tid, rb);
  stage_store<A_KC, DROP == 1>(lds, lda, m0, kb, tid, ra, drop);
  stage_store<B_KC, DROP == 2>(lds + A_TILE, ldb, n0, kb, tid, rb, drop);
  __syncthreads();

  int buf = 0;
  for (int k0 = kb; k0 < ke; k0 += TBK) {
    const bool more = (k0 + TBK) < ke;
    if (more) {
      stage_load<A_KC, VEC>(A, lda, m0, M, k0 + TBK, ke, tid, ra);
      stage_load<B_KC, VEC>(B, ldb, n0, N, k0 + TBK, ke, tid, rb);
    }
    const float* As = lds + buf * (A_TILE + B_TILE);
    const float* Bs = As + A_TILE;
#pragma unroll
    for (int g = 0; g < TBK / 8; ++g) {
      float a[4][2], b[4][2];
      frag_read<A_KC>(As, wr, i_l, h_l, g, a);
      frag_read<B_KC>(Bs, wc, i_l, h_l, g, b);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int fi = 0; fi < 2; ++fi)
#pragma unroll
          for (int fj = 0; fj < 2; ++fj)
            acc[fi][fj] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                a[s][fi], b[s][fj], acc[fi][fj], 0, 0, 0);
    }
    if (more) {
      // buf^1 was last read before the previous barrier: free to refill
      float* Wn = lds + (buf ^ 1) * (A_TILE + B_TILE);
      stage_store<A_KC, DROP == 1>(Wn, lda, m0, k0 + TBK, tid, ra, drop);
      stage_store<B_KC, DROP == 2>(Wn + A_TILE, ldb, n0, k0 + TBK, tid, rb,
                                   drop);
      __syncthreads();
    }
    buf ^= 1;
  }

  // epilogue. B in the KS image: the lane's two tiles hold columns 2j and
  // 2j+1 — one float2 store (N % 4 == 0 on the VEC path).
  const bool add_bias = bias != nullptr && blockIdx.y == 0;
#pragma unroll
  for (int fi = 0; fi < 2; ++fi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int gm = m0 + wr +
                     frag_index<A_KC>(fi, (r & 3) + 8 * (r >> 2) + 4 * h_l);
      if (gm >= M) continue;
      float* crow = C + (int64_t)gm * N;
      if (!B_KC && VEC && !ATOMIC) {
        const int gn = n0 + wc + 2 * i_l;
        if (gn < N) {
          float2 v = make_float2(acc[fi][0][r], acc[fi][1][r]);
          if (add_bias) { v.x += bias[gn]; v.y += bias[gn + 1]; }
          *reinterpret_cast<float2*>(crow + gn) = v;
        }
      } else {
#pragma unroll
        for (int fj = 0; fj < 2; ++fj) {
          const int gn = n0 + wc + frag_index<B_KC>(fj, i_l);
          if (gn < N) {
            float v = acc[fi][fj][r];
            if (add_bias) v += bias[gn];       // bias once (slice 0)
            if (ATOMIC) atomicAdd(crow + gn, v);
            else crow[gn] = v;
          }
        }
      }
    }
}

struct LaunchArgs {
  const float *A, *B, *bias;
  float* C;
  int64_t lda, ldb;
  int M, N, K, k_slice, tiles_n;
  dim3 grid;
  DropArgs drop;
  hipStream_t stream;
};

template <bool A_KC, bool B_KC, bool VEC, int DROP, bool ATOMIC>
void launch_one(const LaunchArgs& a) {
  hipLaunchKernelGGL((gemm_tiled_kernel<A_KC, B_KC, VEC, DROP, ATOMIC>),
                     a.grid, dim3(256), 0, a.stream, a.A, a.lda, a.B, a.ldb,
                     a.bias, a.C, a.M, a.N, a.K, a.k_slice, a.tiles_n, a.drop);
}

template <bool A_KC, bool B_KC, int DROP>
void launch_layout(const LaunchArgs& a, bool vec, bool atomic) {
  if (vec) {
    if (atomic) launch_one<A_KC, B_KC, true, DROP, true>(a);
    else        launch_one<A_KC, B_KC, true, DROP, false>(a);
  } else {
    if (atomic) launch_one<A_KC, B_KC, false, DROP, true>(a);
    else        launch_one<A_KC, B_KC, false, DROP, false>(a);
  }
}

inline bool aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr<float>()) % 16 == 0;
}

}  // namespace

namespace bns {

bool gemm_tiled_aligned(GemmLayout layout, const at::Tensor& A,
                        const at::Tensor& B, int M, int N, int R) {
  if (!aligned16(A) || !aligned16(B)) return false;
  switch (layout) {
    case GEMM_NT: return R % 4 == 0;                    // lda = ldb = R
    case GEMM_NN: return R % 4 == 0 && N % 4 == 0;      // lda = R, ldb = N
    default:      return M % 4 == 0 && N % 4 == 0;      // lda = M, ldb = N
  }
}

at::Tensor gemm_tiled(GemmLayout layout, const at::Tensor& A,
                      const at::Tensor& B,
                      const c10::optional<at::Tensor>& bias, int M, int N,
                      int R, GemmDrop drop, float keep, uint64_t seed) {
  TORCH_CHECK(M > 0 && N > 0 && R > 0, "gemm_tiled: empty operand");
  LaunchArgs a;
  a.A = A.data_ptr<float>();
  a.B = B.data_ptr<float>();
  a.bias = bias.has_value() ? bias->data_ptr<float>() : nullptr;
  a.lda = (layout == GEMM_TN) ? M : R;
  a.ldb = (layout == GEMM_NT) ? R : N;
  a.M = M; a.N = N; a.K = R;
  a.stream = at::cuda::getCurrentCUDAStream();
  const bool vec = gemm_tiled_aligned(layout, A, B, M, N, R);

  // keep == 1.0f (after rounding to float): plain GEMM, as dropout_apply
  const bool dropping = drop != DROP_NONE && keep < 1.0f;
  a.drop.thr = (keep > 0.f && keep < 1.0f)
                   ? (uint32_t)((double)keep * 4294967296.0) : 0u;
  a.drop.seed = seed;
  a.drop.inv_keep = dropping ? 1.0f / keep : 1.0f;

  const int tiles_m = (M + TBM - 1) / TBM;
  a.tiles_n = (N + TBN - 1) / TBN;
  const int64_t tiles = (int64_t)tiles_m * a.tiles_n;
  // split-K when the tile grid alone cannot fill the device (the dW
  // reductions: C is small, R is the node count). The kernel's registers
  // allow 2 resident blocks per CU, 512 on 256 CUs; the slices are sized
  // so that the blocks fill those slots in ONE round (20 tiles x 25 = 500):
  // 760 blocks, a round and a half, measured 1.3x slower per FLOP on the
  // [256, 1204] dW than the same kernel's full rounds. At least 8 K-tiles
  // per slice.
  constexpr int64_t kResidentBlocks = 512;
  int splitk = 1;
  if (tiles < kResidentBlocks && R >= 16 * TBK) {
    splitk = (int)std::min<int64_t>(kResidentBlocks / tiles,
                                    (int64_t)R / (8 * TBK));
    splitk = std::max(splitk, 1);
  }
  a.k_slice = R;
  if (splitk > 1) {
    a.k_slice = ((R + splitk - 1) / splitk + TBK - 1) / TBK * TBK;
    splitk = (R + a.k_slice - 1) / a.k_slice;
  }
  const bool atomic = splitk > 1;
  a.grid = dim3((unsigned)tiles, (unsigned)splitk);
  auto C = atomic ? at::zeros({M, N}, A.options())
                  : at::empty({M, N}, A.options());
  a.C = C.data_ptr<float>();

  if (layout == GEMM_NT) {
    TORCH_CHECK(drop != DROP_B, "gemm_tiled: NT drops A");
    if (dropping) launch_layout<true, true, 1>(a, vec, atomic);
    else          launch_layout<true, true, 0>(a, vec, atomic);
  } else if (layout == GEMM_NN) {
    TORCH_CHECK(drop == DROP_NONE, "gemm_tiled: NN has no dropout form");
    launch_layout<true, false, 0>(a, vec, atomic);
  } else {
    TORCH_CHECK(drop != DROP_A, "gemm_tiled: TN drops B");
    if (dropping) launch_layout<false, false, 2>(a, vec, atomic);
    else          launch_layout<false, false, 0>(a, vec, atomic);
  }
  return C;
}

}  // namespace bns
