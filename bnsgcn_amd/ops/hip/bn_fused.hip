// Fused SyncBatchNorm + ReLU + dropout for --norm batch (docs/DESIGN.md
// §5b). fp32, row-major [n, F]. Three passes over the activation forward
// (read x for the sums; read x, write y) and five backward (read x and dy
// for the sums; read both again, write dx), with the all-reduces of the
// [2F + 1] vectors done by the caller between the kernels:
//
//   bn_colsums<fwd>   Σx, Σx² per column          -> per-block partial rows
//   bn_colsum_finish  partial rows -> [2F + 1]    (+ the local row count)
//        -- all-reduce --
//   bn_finalize       mean, rstd, running statistics (F threads)
//   bn_act_drop_fwd   y = dropout(relu?(x̂·w + b))
//
//   bn_colsums<bwd>   Σg, Σg·x̂ with g = dy·dropmask/keep·relumask
//   bn_colsum_finish  partial rows -> [2F + 1]    (+ the global row count)
//        -- all-reduce of the first 2F --
//   bn_act_drop_bwd_dx  dx = w·rstd·(g − Σg/n − x̂·Σg·x̂/n)
//
// Mapping, shared by the three kernels that walk rows (BnTile). A
// 256-thread block is a TY x TX tile. Each of the TX lanes owns VEC
// adjacent columns (one float4 when F % 4 == 0, one float otherwise), TX =
// min(64, pow2 >= F / VEC), so a wave reads one whole 1 KiB row per step at
// F = 256 and four rows per step at F = 64: no lane idles because F is
// narrow. F > 64 * VEC takes column chunks on blockIdx.x. blockIdx.y owns a
// contiguous slab of rows, which the TY sub-rows stride; the loop is
// unrolled U times with all U row loads issued before the first use. What a
// lane needs per COLUMN (mean, rstd, w, b, the reduced sums) it loads once
// into registers, so the streaming loop is loads, a handful of FMAs and
// the store.
//
// The column sums are running sums in registers, reduced over TY through
// LDS in a fixed tree and written as one partial row per block; the finish
// kernel adds the partial rows in a fixed order. No atomics: two runs give
// the same bits.
//
// x̂ and the pre-activation come from the same two functions (bn_xhat,
// bn_pre) with contraction off in all three places that form them, so the
// ReLU mask of the backward is the one the forward applied. The dropout
// mask is drop_keep on the flat index r * F + f, i.e. dropout_apply's.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <algorithm>
#include <vector>
#include "common.h"
#include "bn_fused.h"

namespace {

#define BN_EXACT _Pragma("clang fp contract(off)")
#define BN_MAX_BLOCKS 2048   // blocks of one row-walking launch
#define BN_TPB 256

struct BnDrop { bool on; uint32_t thr; float inv_keep; uint64_t seed; };
DEV_INLINE BnDrop bn_drop(float keep, uint64_t seed) {
  const bool on = keep < 1.0f;
  return {on, drop_threshold(keep), on ? 1.0f / keep : 1.0f, seed};
}

DEV_INLINE float bn_xhat(float x, float mean, float rstd) {
  BN_EXACT
  return (x - mean) * rstd;
}
DEV_INLINE float bn_pre(float xh, float w, float b) { return fmaf(xh, w, b); }

// g = dy * dropmask / keep * relumask for the element with flat index idx
DEV_INLINE float bn_g(float dy, float pre, int act, const BnDrop& dp,
                      int64_t idx) {
  float g = dp.on ? drop_apply(dy, idx, dp.thr, dp.seed, dp.inv_keep) : dy;
  if (act && pre <= 0.f) g = 0.f;
  return g;
}

// VEC adjacent floats of a row: one 16-byte access for VEC = 4.
template <int VEC> struct BnVec { float v[VEC]; };
template <int VEC>
DEV_INLINE BnVec<VEC> bn_load(const float* __restrict__ p) {
  BnVec<VEC> r;
  if (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    r.v[0] = q.x; r.v[1 % VEC] = q.y; r.v[2 % VEC] = q.z; r.v[3 % VEC] = q.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}
template <int VEC>
DEV_INLINE void bn_store(float* __restrict__ p, const BnVec<VEC>& r) {
  if (VEC == 4)
    *reinterpret_cast<float4*>(p) =
        make_float4(r.v[0], r.v[1 % VEC], r.v[2 % VEC], r.v[3 % VEC]);
  else
    *p = r.v[0];
}
template <int VEC> DEV_INLINE BnVec<VEC> bn_zero() {
  BnVec<VEC> r;
#pragma unroll
  for (int v = 0; v < VEC; ++v) r.v[v] = 0.f;
  return r;
}

// The calling thread's place in the TY x TX tile (file comment).
struct BnTile {
  int tx, ty, TX, TY;
  int c0;            // first of the lane's VEC columns
  bool col_ok;       // c0 < F (then c0 + VEC <= F: VEC divides F)
  int64_t r0, r1;    // the block's row slab
};
template <int VEC>
DEV_INLINE BnTile bn_tile(int64_t n, int F, int tx_log2, int64_t rows_per) {
  BnTile t;
  t.TX = 1 << tx_log2;
  t.TY = BN_TPB >> tx_log2;
  t.tx = threadIdx.x & (t.TX - 1);
  t.ty = threadIdx.x >> tx_log2;
  t.c0 = (blockIdx.x * t.TX + t.tx) * VEC;
  t.col_ok = t.c0 < F;
  t.r0 = (int64_t)blockIdx.y * rows_per;
  const int64_t e = t.r0 + rows_per;
  t.r1 = e < n ? e : n;
  return t;
}

// Per-column operands of a lane, loaded once.
template <int VEC> struct BnCols { BnVec<VEC> mean, rstd, w, b; };
template <int VEC>
DEV_INLINE BnCols<VEC> bn_cols(const float* __restrict__ mean,
                               const float* __restrict__ rstd,
                               const float* __restrict__ w,
                               const float* __restrict__ b, int c0) {
  return {bn_load<VEC>(mean + c0), bn_load<VEC>(rstd + c0),
          bn_load<VEC>(w + c0), bn_load<VEC>(b + c0)};
}

// --------------------------------------------------------------- colsums
// BWD = false: a = Σx, b = Σx².  BWD = true: a = Σg, b = Σg·x̂.
// partial is [gridDim.y, 2 * F]: row blockIdx.y holds this slab's a then b.
template <int VEC, bool BWD, int U>
NO_PACKED_FP32 __global__ __launch_bounds__(BN_TPB) void bn_colsums_kernel(
    const float* __restrict__ x, const float* __restrict__ dy,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ w, const float* __restrict__ b,
    float* __restrict__ partial, int64_t n, int F, int tx_log2,
    int64_t rows_per, int act, float keep, uint64_t seed) {
  BN_EXACT
  __shared__ float sm[2 * VEC * BN_TPB];
  const BnTile t = bn_tile<VEC>(n, F, tx_log2, rows_per);
  const BnDrop dp = bn_drop(keep, seed);
  BnVec<VEC> sa = bn_zero<VEC>(), sb = bn_zero<VEC>();
  if (t.col_ok) {
    BnCols<VEC> c;
    if (BWD) c = bn_cols<VEC>(mean, rstd, w, b, t.c0);
    const int64_t step = (int64_t)t.TY * U;
    for (int64_t r = t.r0 + t.ty; r < t.r1; r += step) {
      BnVec<VEC> xv[U], dv[U];
      // rows past the slab read as x = 0, dy = 0 and add nothing
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t rr = r + (int64_t)u * t.TY;
        const bool ok = rr < t.r1;
        xv[u] = ok ? bn_load<VEC>(x + rr * F + t.c0) : bn_zero<VEC>();
        if (BWD)
          dv[u] = ok ? bn_load<VEC>(dy + rr * F + t.c0) : bn_zero<VEC>();
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t idx = (r + (int64_t)u * t.TY) * F + t.c0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          if (BWD) {
            const float xh = bn_xhat(xv[u].v[v], c.mean.v[v], c.rstd.v[v]);
            const float g = bn_g(dv[u].v[v], bn_pre(xh, c.w.v[v], c.b.v[v]),
                                 act, dp, idx + v);
            sa.v[v] += g;
            sb.v[v] = fmaf(g, xh, sb.v[v]);
          } else {
            sa.v[v] += xv[u].v[v];
            sb.v[v] = fmaf(xv[u].v[v], xv[u].v[v], sb.v[v]);
          }
        }
      }
    }
  }
  // value (k, v) of thread tid sits at sm[(k * VEC + v) * 256 + tid]:
  // consecutive threads, consecutive banks. Sub-rows ty and ty + h combine
  // for h = TY/2 .. 1, the same tree in every run.
  const int tid = threadIdx.x;
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    sm[v * BN_TPB + tid] = sa.v[v];
    sm[(VEC + v) * BN_TPB + tid] = sb.v[v];
  }
  __syncthreads();
  for (int h = t.TY >> 1; h > 0; h >>= 1) {
    if (t.ty < h) {
#pragma unroll
      for (int k = 0; k < 2 * VEC; ++k)
        sm[k * BN_TPB + tid] += sm[k * BN_TPB + tid + h * t.TX];
    }
    __syncthreads();
  }
  if (t.ty == 0 && t.col_ok) {
    float* prow = partial + (int64_t)blockIdx.y * 2 * F;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      prow[t.c0 + v] = sm[v * BN_TPB + tid];
      prow[F + t.c0 + v] = sm[(VEC + v) * BN_TPB + tid];
    }
  }
}

// out[j] = sum over the nb partial rows of column j (j < C = 2F), and
// out[C] = the row count: `count` itself, or *count_src where that is given
// (the backward copies the forward's all-reduced count). A block takes 16
// columns; thread (ty, tx) adds rows ty, ty + 16, ... of column tx in
// order, then the 16 row lanes combine in a fixed tree. nb = 0 writes zeros.
__global__ __launch_bounds__(BN_TPB) void bn_colsum_finish_kernel(
    const float* __restrict__ partial, float* __restrict__ out, int nb, int C,
    float count, const float* __restrict__ count_src) {
  BN_EXACT
  __shared__ float red[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + tx;
  float s = 0.f;
  if (c < C)
    for (int r = ty; r < nb; r += 16) s += partial[(int64_t)r * C + c];
  red[ty][tx] = s;
  __syncthreads();
  for (int h = 8; h > 0; h >>= 1) {
    if (ty < h) red[ty][tx] += red[ty + h][tx];
    __syncthreads();
  }
  if (ty == 0 && c < C) out[c] = red[0][tx];
  if (blockIdx.x == 0 && threadIdx.x == 0)
    out[C] = count_src ? *count_src : count;
}

// -------------------------------------------------------------- finalize
// stats = [Σx (F), Σx² (F), rows] after the all-reduce. The few operations
// per column run in double and round once: var = E[x²] − mean² cancels.
__global__ __launch_bounds__(BN_TPB) void bn_finalize_kernel(
    const float* __restrict__ stats, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, float* __restrict__ running_mean,
    float* __restrict__ running_var, int F, float momentum, float one_minus,
    double eps) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const double n_total = fmax((double)stats[2 * F], 1.0);
  const double sx = stats[f], sx2 = stats[F + f];
  const double mean = sx / n_total;
  const double var = (sx2 - mean * sx) / n_total;   // may round below 0
  mean_out[f] = (float)mean;
  rstd_out[f] = (float)(1.0 / sqrt(fmax(var, 0.0) + eps));
  // running_x.mul_(1 - momentum).add_(x * momentum), var unclamped
  running_mean[f] = fmaf((float)mean, momentum, running_mean[f] * one_minus);
  running_var[f] = fmaf((float)var, momentum, running_var[f] * one_minus);
}

// ----------------------------------------------------------------- apply
template <int VEC, int U>
NO_PACKED_FP32 __global__ __launch_bounds__(BN_TPB) void bn_act_drop_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ w,
    const float* __restrict__ b, float* __restrict__ y, int64_t n, int F,
    int tx_log2, int64_t rows_per, int act, float keep, uint64_t seed) {
  BN_EXACT
  const BnTile t = bn_tile<VEC>(n, F, tx_log2, rows_per);
  if (!t.col_ok) return;
  const BnDrop dp = bn_drop(keep, seed);
  const BnCols<VEC> c = bn_cols<VEC>(mean, rstd, w, b, t.c0);
  const int64_t step = (int64_t)t.TY * U;
  for (int64_t r = t.r0 + t.ty; r < t.r1; r += step) {
    BnVec<VEC> xv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t rr = r + (int64_t)u * t.TY;
      if (rr < t.r1) xv[u] = bn_load<VEC>(x + rr * F + t.c0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t rr = r + (int64_t)u * t.TY;
      if (rr >= t.r1) break;
      const int64_t idx = rr * F + t.c0;
      BnVec<VEC> o;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float p = bn_pre(bn_xhat(xv[u].v[v], c.mean.v[v], c.rstd.v[v]),
                         c.w.v[v], c.b.v[v]);
        if (act) p = fmaxf(p, 0.f);
        if (dp.on) p = drop_apply(p, idx + v, dp.thr, dp.seed, dp.inv_keep);
        o.v[v] = p;
      }
      bn_store<VEC>(y + idx, o);
    }
  }
}

// red = [Σg (F), Σg·x̂ (F), rows], all three global.
template <int VEC, int U>
NO_PACKED_FP32 __global__ __launch_bounds__(BN_TPB)
void bn_act_drop_bwd_dx_kernel(
    const float* __restrict__ x, const float* __restrict__ dy,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ w, const float* __restrict__ b,
    const float* __restrict__ red, float* __restrict__ dx, int64_t n, int F,
    int tx_log2, int64_t rows_per, int act, float keep, uint64_t seed) {
  BN_EXACT
  const BnTile t = bn_tile<VEC>(n, F, tx_log2, rows_per);
  if (!t.col_ok) return;
  const BnDrop dp = bn_drop(keep, seed);
  const BnCols<VEC> c = bn_cols<VEC>(mean, rstd, w, b, t.c0);
  const float inv_n = 1.0f / fmaxf(red[2 * F], 1.0f);
  const BnVec<VEC> sg = bn_load<VEC>(red + t.c0);
  const BnVec<VEC> sgx = bn_load<VEC>(red + F + t.c0);
  BnVec<VEC> gm, gxm, wr;   // Σg/n, Σg·x̂/n, w·rstd
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    gm.v[v] = sg.v[v] * inv_n;
    gxm.v[v] = sgx.v[v] * inv_n;
    wr.v[v] = c.w.v[v] * c.rstd.v[v];
  }
  const int64_t step = (int64_t)t.TY * U;
  for (int64_t r = t.r0 + t.ty; r < t.r1; r += step) {
    BnVec<VEC> xv[U], dv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t rr = r + (int64_t)u * t.TY;
      if (rr < t.r1) {
        xv[u] = bn_load<VEC>(x + rr * F + t.c0);
        dv[u] = bn_load<VEC>(dy + rr * F + t.c0);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t rr = r + (int64_t)u * t.TY;
      if (rr >= t.r1) break;
      const int64_t idx = rr * F + t.c0;
      BnVec<VEC> o;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float xh = bn_xhat(xv[u].v[v], c.mean.v[v], c.rstd.v[v]);
        const float g = bn_g(dv[u].v[v], bn_pre(xh, c.w.v[v], c.b.v[v]), act,
                             dp, idx + v);
        o.v[v] = wr.v[v] * (g - gm.v[v] - xh * gxm.v[v]);
      }
      bn_store<VEC>(dx + idx, o);
    }
  }
}

// ------------------------------------------------------------------ host
void check_mat(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 2 &&
              t.scalar_type() == at::kFloat, name,
              ": contiguous 2-D fp32 cuda tensor expected");
  TORCH_CHECK(t.size(1) > 0 && t.size(1) <= (1 << 24), name, ": bad width");
}
void check_vec(const at::Tensor& t, int64_t len, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 1 &&
              t.scalar_type() == at::kFloat && t.numel() == len, name,
              ": contiguous fp32 cuda vector of ", len, " expected");
}
bool aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// Launch shape of the row-walking kernels (file comment).
struct BnLaunch {
  int vec, tx_log2;
  int64_t rows_per;
  dim3 grid;
};
BnLaunch bn_launch(int64_t n, int F, bool vec4, int unroll) {
  BnLaunch L;
  L.vec = vec4 ? 4 : 1;
  const int lanes = F / L.vec;
  L.tx_log2 = 0;
  while ((1 << L.tx_log2) < lanes && L.tx_log2 < 6) ++L.tx_log2;
  const int TX = 1 << L.tx_log2, TY = BN_TPB >> L.tx_log2;
  const int col_chunks = (lanes + TX - 1) / TX;
  const int64_t per_step = (int64_t)TY * unroll;
  const int64_t want = (n + per_step - 1) / per_step;
  const int64_t cap = std::max(1, BN_MAX_BLOCKS / col_chunks);
  const int64_t row_blocks = std::max<int64_t>(1, std::min(want, cap));
  L.rows_per = (n + row_blocks - 1) / row_blocks;
  L.grid = dim3(col_chunks, (unsigned)row_blocks);
  return L;
}

#define BN_VEC_DISPATCH(vec, ...)                          \
  do {                                                     \
    if ((vec) == 4) { constexpr int VEC = 4; __VA_ARGS__; } \
    else { constexpr int VEC = 1; __VA_ARGS__; }            \
  } while (0)

constexpr int U_SUMS = 4, U_APPLY = 4, U_DX = 2;

void check_cols(const at::Tensor& x, const at::Tensor& mean,
                const at::Tensor& rstd, const at::Tensor& w,
                const at::Tensor& b) {
  const int64_t F = x.size(1);
  check_vec(mean, F, "mean");
  check_vec(rstd, F, "rstd");
  check_vec(w, F, "weight");
  check_vec(b, F, "bias");
}

void finish(const at::Tensor& partial, at::Tensor& out, int nb, int F,
            float count, const float* count_src, hipStream_t stream) {
  hipLaunchKernelGGL(bn_colsum_finish_kernel, dim3((2 * F + 15) / 16),
                     dim3(BN_TPB), 0, stream,
                     nb ? partial.data_ptr<float>() : nullptr,
                     out.data_ptr<float>(), nb, 2 * F, count, count_src);
}

// [Σx (F), Σx² (F), n] of this rank's rows
at::Tensor bn_colsums_fwd(at::Tensor x) {
  check_mat(x, "x");
  const int64_t n = x.size(0);
  const int F = (int)x.size(1);
  auto out = at::empty({2 * (int64_t)F + 1}, x.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  if (n == 0) {
    finish(out, out, 0, F, 0.f, nullptr, stream);
    return out;
  }
  const BnLaunch L = bn_launch(n, F, F % 4 == 0 && aligned16(x), U_SUMS);
  auto partial = at::empty({(int64_t)L.grid.y, 2 * (int64_t)F}, x.options());
  BN_VEC_DISPATCH(L.vec, hipLaunchKernelGGL(
      (bn_colsums_kernel<VEC, false, U_SUMS>), L.grid, dim3(BN_TPB), 0, stream,
      x.data_ptr<float>(), nullptr, nullptr, nullptr, nullptr, nullptr,
      partial.data_ptr<float>(), n, F, L.tx_log2, L.rows_per, 0, 1.0f,
      (uint64_t)0));
  finish(partial, out, (int)L.grid.y, F, (float)n, nullptr, stream);
  return out;
}

// (mean, rstd) from the all-reduced stats; running statistics in place
std::vector<at::Tensor> bn_finalize(at::Tensor stats, at::Tensor running_mean,
                                    at::Tensor running_var, double momentum,
                                    double eps) {
  const int64_t F = running_mean.numel();
  TORCH_CHECK(F > 0, "bn_finalize: empty running_mean");
  check_vec(stats, 2 * F + 1, "stats");
  check_vec(running_mean, F, "running_mean");
  check_vec(running_var, F, "running_var");
  auto mr = at::empty({2, F}, stats.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((F + BN_TPB - 1) / BN_TPB),
                     dim3(BN_TPB), 0, stream, stats.data_ptr<float>(),
                     mr.data_ptr<float>(), mr.data_ptr<float>() + F,
                     running_mean.data_ptr<float>(),
                     running_var.data_ptr<float>(), (int)F, (float)momentum,
                     (float)(1.0 - momentum), eps);
  return {mr[0], mr[1]};
}

at::Tensor bn_act_drop_fwd(at::Tensor x, at::Tensor mean, at::Tensor rstd,
                           at::Tensor w, at::Tensor b, int64_t act,
                           double keep, int64_t seed) {
  check_mat(x, "x");
  check_cols(x, mean, rstd, w, b);
  const int64_t n = x.size(0);
  const int F = (int)x.size(1);
  auto y = at::empty_like(x);
  if (n == 0) return y;
  auto stream = at::cuda::getCurrentCUDAStream();
  const BnLaunch L = bn_launch(
      n, F, F % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(mean),
      U_APPLY);
  BN_VEC_DISPATCH(L.vec, hipLaunchKernelGGL(
      (bn_act_drop_fwd_kernel<VEC, U_APPLY>), L.grid, dim3(BN_TPB), 0, stream,
      x.data_ptr<float>(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
      w.data_ptr<float>(), b.data_ptr<float>(), y.data_ptr<float>(), n, F,
      L.tx_log2, L.rows_per, (int)act, (float)keep, (uint64_t)seed));
  return y;
}

bool bwd_vec4(const at::Tensor& x, const at::Tensor& dy,
              const at::Tensor& mean, const at::Tensor& rstd,
              const at::Tensor& w, const at::Tensor& b) {
  return x.size(1) % 4 == 0 && aligned16(x) && aligned16(dy) &&
         aligned16(mean) && aligned16(rstd) && aligned16(w) && aligned16(b);
}

// [Σg (F), Σg·x̂ (F), count] of this rank's rows; count is copied from
// `count` (one element on the device: the forward's all-reduced row count)
at::Tensor bn_colsums_bwd(at::Tensor x, at::Tensor dy, at::Tensor mean,
                          at::Tensor rstd, at::Tensor w, at::Tensor b,
                          at::Tensor count, int64_t act, double keep,
                          int64_t seed) {
  check_mat(x, "x");
  check_mat(dy, "dy");
  TORCH_CHECK(dy.sizes() == x.sizes(), "bn_colsums_bwd: dy must match x");
  check_cols(x, mean, rstd, w, b);
  check_vec(count, 1, "count");
  const int64_t n = x.size(0);
  const int F = (int)x.size(1);
  auto out = at::empty({2 * (int64_t)F + 1}, x.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  if (n == 0) {
    finish(out, out, 0, F, 0.f, count.data_ptr<float>(), stream);
    return out;
  }
  const BnLaunch L = bn_launch(n, F, bwd_vec4(x, dy, mean, rstd, w, b), U_SUMS);
  auto partial = at::empty({(int64_t)L.grid.y, 2 * (int64_t)F}, x.options());
  BN_VEC_DISPATCH(L.vec, hipLaunchKernelGGL(
      (bn_colsums_kernel<VEC, true, U_SUMS>), L.grid, dim3(BN_TPB), 0, stream,
      x.data_ptr<float>(), dy.data_ptr<float>(), mean.data_ptr<float>(),
      rstd.data_ptr<float>(), w.data_ptr<float>(), b.data_ptr<float>(),
      partial.data_ptr<float>(), n, F, L.tx_log2, L.rows_per, (int)act,
      (float)keep, (uint64_t)seed));
  finish(partial, out, (int)L.grid.y, F, 0.f, count.data_ptr<float>(), stream);
  return out;
}

at::Tensor bn_act_drop_bwd_dx(at::Tensor x, at::Tensor dy, at::Tensor mean,
                              at::Tensor rstd, at::Tensor w, at::Tensor b,
                              at::Tensor red, int64_t act, double keep,
                              int64_t seed) {
  check_mat(x, "x");
  check_mat(dy, "dy");
  TORCH_CHECK(dy.sizes() == x.sizes(), "bn_act_drop_bwd_dx: dy must match x");
  check_cols(x, mean, rstd, w, b);
  const int64_t n = x.size(0);
  const int F = (int)x.size(1);
  check_vec(red, 2 * (int64_t)F + 1, "red");
  auto dx = at::empty_like(x);
  if (n == 0) return dx;
  auto stream = at::cuda::getCurrentCUDAStream();
  const BnLaunch L = bn_launch(
      n, F, bwd_vec4(x, dy, mean, rstd, w, b) && aligned16(dx) &&
                aligned16(red), U_DX);
  BN_VEC_DISPATCH(L.vec, hipLaunchKernelGGL(
      (bn_act_drop_bwd_dx_kernel<VEC, U_DX>), L.grid, dim3(BN_TPB), 0, stream,
      x.data_ptr<float>(), dy.data_ptr<float>(), mean.data_ptr<float>(),
      rstd.data_ptr<float>(), w.data_ptr<float>(), b.data_ptr<float>(),
      red.data_ptr<float>(), dx.data_ptr<float>(), n, F, L.tx_log2,
      L.rows_per, (int)act, (float)keep, (uint64_t)seed));
  return dx;
}

}  // namespace

namespace bns {

void bind_bn_fused(pybind11::module& m) {
  m.attr("BN_MAX_BLOCKS") = BN_MAX_BLOCKS;
  m.def("bn_colsums_fwd", &bn_colsums_fwd,
        "[sum x, sum x^2, rows] of a [n, F] activation");
  m.def("bn_finalize", &bn_finalize,
        "(mean, rstd) from reduced stats; updates the running statistics");
  m.def("bn_act_drop_fwd", &bn_act_drop_fwd,
        "dropout(relu?(batch-norm(x))) in one pass");
  m.def("bn_colsums_bwd", &bn_colsums_bwd,
        "[sum g, sum g*xhat, rows] of the fused backward");
  m.def("bn_act_drop_bwd_dx", &bn_act_drop_bwd_dx,
        "dx of the fused batch-norm backward in one pass");
}

}  // namespace bns
