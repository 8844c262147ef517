// GATv2 attention score on gfx950 (--gat-attn v2, docs/DESIGN.md §4d):
//
//   e[k,h] = sum_d attn[h,d] * LeakyReLU(zs[col_k,h,d] + zd[row_k,h,d])
//
// The non-linearity sits inside the dot product, so the score does not
// factorise into per-node scalars (the v1 route attn_project + sddmm_add):
// every edge costs a gather of the full H*D source row, in the forward and
// again in each direction of the backward. Nothing of size [E, H, D] is
// ever stored — the backward recomputes s = zs + zd from the two rows it
// gathers anyway; a stored mask would be 1/32 of that tensor (0.9 GB on a
// 14M-edge, H*D = 512 block) and a stored s all of it.
//
// Lane mapping (all three uses): a row is S = H*D/4 float4 slots; the lane
// owns slots lane, lane + 64, .. (NS = 1, 2 or 4 of them: H*D <= 1024 in
// one walk of the edge list), slot f belongs to head f / (D/4). The
// RESIDENT row (the work item's own: zd[row] on the forward CSR, zs[col]
// on the transposed one) and attn stay in registers, the STREAMED rows come
// in on the depth-U gather stream (gather_stream.h) with 16-byte lane loads.
// s = streamed + resident is one fp32 add, never contracted, so its sign is
// the sign of the exact sum and the LeakyReLU branch matches a float64
// evaluation of the same fp32 inputs.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/util/Optional.h>
#include "common.h"
#include "gather_stream.h"
#include "worklist_launch.h"
#include "gatv2.h"

namespace {

// Row reads in flight per wave: 4 edges; 2 at four slots per lane, where a
// window of 4 would hold 64 registers of the 128 that keep 4 waves per SIMD.
template <int NS> struct Depth { static constexpr int U = NS == 4 ? 2 : 4; };

struct Lrelu4 { float x, y, z, w; };

// LeakyReLU(a + b) per component; pos[i] tells the branch taken.
DEV_INLINE Lrelu4 lrelu_sum(const float4 a, const float4 b, float slope,
                            bool (&pos)[4]) {
  const float s0 = __fadd_rn(a.x, b.x), s1 = __fadd_rn(a.y, b.y),
              s2 = __fadd_rn(a.z, b.z), s3 = __fadd_rn(a.w, b.w);
  pos[0] = s0 > 0.f; pos[1] = s1 > 0.f; pos[2] = s2 > 0.f; pos[3] = s3 > 0.f;
  return {pos[0] ? s0 : s0 * slope, pos[1] ? s1 : s1 * slope,
          pos[2] ? s2 : s2 * slope, pos[3] ? s3 : s3 * slope};
}

// The lane's NS slots of a one-pass row: index (clamped in bounds), head,
// and whether the slot exists.
template <int NS>
DEV_INLINE void lane_slots(int lane, int S, int D4, int (&si)[NS],
                           int (&hs)[NS], bool (&ok)[NS]) {
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int s = j * WAVE + lane;
    ok[j] = s < S;
    si[j] = ok[j] ? s : S - 1;
    hs[j] = si[j] / D4;
  }
}

// Forward. FAST: D4 = D/4 is a power of two <= 64, a head is D4 consecutive
// lanes of one slot set and its partials combine by shfl_xor inside the
// group; the group leader stores. General form (any D % 4 == 0, e.g.
// D = 100: 25 lanes per head, heads straddle every boundary): head by head
// the wave sums the partials that belong to it, lane h keeps head h, and
// lanes 0 .. H-1 store the edge's H scores with one coalesced write. Each
// (edge, head) is written exactly once, so split rows need no atomics.
template <int NS, bool FAST>
__global__ __launch_bounds__(256) NO_PACKED_FP32
void gatv2_score_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int32_t* __restrict__ indices, const float* __restrict__ zs,
    const float* __restrict__ zd, const float* __restrict__ attn,
    float* __restrict__ out, int H, int D4, int S, float slope) {
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const float4* __restrict__ zd4 = reinterpret_cast<const float4*>(zd);
  const int lane = threadIdx.x & (WAVE - 1);
  int ls[NS], hs[NS];
  bool ok[NS];
  lane_slots<NS>(lane, S, D4, ls, hs, ok);
  float4 at[NS], zr[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j)              // attn: once per wave
    at[j] = reinterpret_cast<const float4*>(attn)[ls[j]];
  const bool leader = (lane & (D4 - 1)) == 0;   // FAST only
  stream_edge_items<Depth<NS>::U, NS, float4, false>(
      wl, indices, nullptr, nullptr, zs, H, false, S,
      [&](int row, const int (&si)[NS], const bool (&)[NS])
          __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NS; ++j) zr[j] = zd4[(int64_t)row * S + si[j]];
      },
      [&](int k, const float4 (&val)[NS], const EdgeChunk&, int64_t e0)
          __attribute__((always_inline)) {
        float p[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          bool pos[4];
          const Lrelu4 l = lrelu_sum(val[j], zr[j], slope, pos);
          const float q =
              at[j].x * l.x + at[j].y * l.y + at[j].z * l.z + at[j].w * l.w;
          p[j] = ok[j] ? q : 0.f;            // a clamped lane adds nothing
        }
        float* __restrict__ oe = out + (e0 + k) * H;
        if constexpr (FAST) {
#pragma unroll
          for (int j = 0; j < NS; ++j) {
            float v = p[j];
            for (int off = D4 >> 1; off > 0; off >>= 1)
              v += __shfl_xor(v, off, WAVE);
            if (ok[j] && leader) oe[hs[j]] = v;
          }
        } else {
          float res = 0.f;
          for (int h = 0; h < H; ++h) {
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < NS; ++j) v += hs[j] == h ? p[j] : 0.f;
            v = wave_reduce_sum(v);
            if (lane == h) res = v;
          }
          if (lane < H) oe[lane] = res;
        }
      },
      [&](int, bool, const int (&)[NS], const bool (&)[NS])
          __attribute__((always_inline)) {});
}

// Backward, ONE kernel for both directions. With m = s > 0 ? 1 : slope and
// g' = g[gperm ? gperm[k] : k]:
//   dz_res[r,h,d] = attn[h,d] * sum_{k in row r} g'[k,h] * m(k,h,d)
//   dattn[h,d]    = sum_k g'[k,h] * LeakyReLU(s(k,h,d))          (DATTN)
// Forward CSR, z_res = zd, z_str = zs: d zd (and d attn). Transposed CSR
// with gperm = its edge permutation, z_res = zs, z_str = zd: d zs. No
// cross-lane step: a lane accumulates its own slots over the item, attn is
// multiplied in once at the store, and the head's g arrives with the edge
// chunk (H <= 4: load_edge_w, then H readlanes and a select per edge).
// Split items combine with atomicAdd into rows the launcher zeroed.
// d attn never touches a global atomic: the lane sums over every item of
// its wave, the block's four waves combine through LDS in a fixed order
// and write row blockIdx.x of part[n_blocks, H*D]; gatv2_colsum_kernel
// finishes. Two runs on one work list give the same bits.
template <int NS, bool DATTN>
__global__ __launch_bounds__(256) NO_PACKED_FP32
void gatv2_score_bwd_kernel(
    const int32_t* __restrict__ wrow, const int64_t* __restrict__ wbeg,
    const int64_t* __restrict__ wend, const int32_t* __restrict__ wave_start,
    const int32_t* __restrict__ indices, const float* __restrict__ g,
    const int64_t* __restrict__ gperm, const float* __restrict__ z_res,
    const float* __restrict__ z_str, const float* __restrict__ attn,
    float* __restrict__ dz, float* __restrict__ part, int H, int D4, int S,
    float slope, int g_vec4) {
  const WorkList wl = {wrow, wbeg, wend, wave_start};
  const float4* __restrict__ zr4 = reinterpret_cast<const float4*>(z_res);
  float4* __restrict__ dz4 = reinterpret_cast<float4*>(dz);
  const int lane = threadIdx.x & (WAVE - 1);
  int ls[NS], hs[NS];
  bool ok[NS];
  lane_slots<NS>(lane, S, D4, ls, hs, ok);
  float4 at[NS], zr[NS], acc[NS], da[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    at[j] = reinterpret_cast<const float4*>(attn)[ls[j]];
    da[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  stream_edge_items<Depth<NS>::U, NS, float4, true>(
      wl, indices, g, gperm, z_str, H, g_vec4 != 0, S,
      [&](int row, const int (&si)[NS], const bool (&)[NS])
          __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          zr[j] = zr4[(int64_t)row * S + si[j]];
          acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      },
      [&](int k, const float4 (&val)[NS], const EdgeChunk& ch, int64_t)
          __attribute__((always_inline)) {
        float gj[NS];
        if (H <= 4) {
          const float g0 = readlane_f(ch.w[0], k), g1 = readlane_f(ch.w[1], k),
                      g2 = readlane_f(ch.w[2], k), g3 = readlane_f(ch.w[3], k);
#pragma unroll
          for (int j = 0; j < NS; ++j)
            gj[j] = hs[j] == 0 ? g0 : hs[j] == 1 ? g1 : hs[j] == 2 ? g2 : g3;
        } else {
          const int64_t we =
              ((int64_t)__builtin_amdgcn_readlane((int)(ch.we >> 32), k) << 32) |
              (uint32_t)__builtin_amdgcn_readlane((int)ch.we, k);
#pragma unroll
          for (int j = 0; j < NS; ++j) gj[j] = g[we * H + hs[j]];
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          bool pos[4];
          const Lrelu4 l = lrelu_sum(val[j], zr[j], slope, pos);
          const float gs = gj[j] * slope;
          acc[j].x += pos[0] ? gj[j] : gs; acc[j].y += pos[1] ? gj[j] : gs;
          acc[j].z += pos[2] ? gj[j] : gs; acc[j].w += pos[3] ? gj[j] : gs;
          if constexpr (DATTN) {
            da[j].x += gj[j] * l.x; da[j].y += gj[j] * l.y;
            da[j].z += gj[j] * l.z; da[j].w += gj[j] * l.w;
          }
        }
      },
      [&](int row, bool atomic, const int (&si)[NS], const bool (&has)[NS])
          __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NS; ++j)
          if (has[j])
            store_row<false>(
                &dz4[(int64_t)row * S + si[j]],
                make_float4(at[j].x * acc[j].x, at[j].y * acc[j].y,
                            at[j].z * acc[j].z, at[j].w * acc[j].w),
                atomic);
      });
  if constexpr (DATTN) {
    __shared__ float4 red[4][NS * WAVE];
    const int wave = threadIdx.x / WAVE;
#pragma unroll
    for (int j = 0; j < NS; ++j) red[wave][j * WAVE + lane] = da[j];
    __syncthreads();
    const int t = threadIdx.x;               // S <= NS * 64 <= 256 slots
    if (t < S) {
      float4 s = red[0][t];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        s.x += red[w][t].x; s.y += red[w][t].y;
        s.z += red[w][t].z; s.w += red[w][t].w;
      }
      reinterpret_cast<float4*>(part)[(int64_t)blockIdx.x * S + t] = s;
    }
  }
}

// out[y, c] = sum of rows [y * chunk, min((y + 1) * chunk, nb)) of
// part[nb, C], in a fixed order: block (x, y) takes 64 columns of chunk y,
// wave w adds the chunk's rows w, w + 4, .. (one 256-byte read per row),
// then the four waves' sums are added 0 + 1 + 2 + 3. Run twice — chunks of
// COLSUM_CHUNK rows, then the chunk sums in one chunk — so that tens of
// thousands of partial rows are read by thousands of blocks, not by C / 64.
constexpr int COLSUM_CHUNK = 128;

__global__ __launch_bounds__(256) void gatv2_colsum_kernel(
    const float* __restrict__ part, float* __restrict__ out, int nb, int C,
    int chunk) {
  __shared__ float red[4][WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int c = blockIdx.x * WAVE + lane;
  const int r0 = blockIdx.y * chunk;
  const int r1 = r0 + chunk < nb ? r0 + chunk : nb;
  float s = 0.f;
  if (c < C)
    for (int r = r0 + wave; r < r1; r += 4) s += part[(int64_t)r * C + c];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < C)
    out[(int64_t)blockIdx.y * C + c] =
        ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// ------------------------------------------------------------- launchers

struct Shape { int H, D, D4, S, NS; };

// zs/zd-like operands [n, H, D] and attn [H, D]: fp32, contiguous, 16-byte
// aligned (rows are read as float4), D % 4 == 0, H * D <= 1024.
Shape check_shape(const char* op, const at::Tensor& a, const at::Tensor& b,
                  const at::Tensor& attn) {
  check_f32(a, "z"); check_f32(b, "z"); check_f32(attn, "attn");
  TORCH_CHECK(a.dim() == 3 && b.dim() == 3 && a.size(1) == b.size(1) &&
                  a.size(2) == b.size(2),
              op, ": [n, H, D] operands of one (H, D) expected");
  const int H = a.size(1), D = a.size(2);
  TORCH_CHECK(attn.numel() == (int64_t)H * D, op, ": attn must hold H * D = ",
              H * D, " values, got ", attn.numel());
  TORCH_CHECK(D > 0 && D % 4 == 0, op, ": D % 4 == 0 required, got D = ", D,
              " (GATv2Layer pads the per-head width to a multiple of 4)");
  TORCH_CHECK(H * D <= 1024 && H <= WAVE, op, ": built for H * D <= 1024 and "
              "H <= 64, got H = ", H, ", D = ", D);
  for (const at::Tensor* t : {&a, &b, &attn})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, op,
                ": operands must be 16-byte aligned");
  const int S = H * D / 4;
  return {H, D, D / 4, S, S <= WAVE ? 1 : S <= 2 * WAVE ? 2 : 4};
}

at::Tensor gatv2_score(at::Tensor wrow, at::Tensor wbeg, at::Tensor wend,
                       at::Tensor wstart, at::Tensor indices, at::Tensor zs,
                       at::Tensor zd, at::Tensor attn, double slope) {
  const Shape sh = check_shape("gatv2_score", zs, zd, attn);
  const WorkListArgs wl = worklist_args(wrow, wbeg, wend, wstart);
  auto out = at::empty({indices.numel(), sh.H}, zs.options());
  if (indices.numel() == 0 || wl.n_waves <= 0) return out;
  auto launch = [&](auto kernel) {
    launch_worklist(kernel, wl, 64, indices.data_ptr<int32_t>(),
                    zs.data_ptr<float>(), zd.data_ptr<float>(),
                    attn.data_ptr<float>(), out.data_ptr<float>(), sh.H,
                    sh.D4, sh.S, (float)slope);
  };
  const bool fast = (sh.D4 & (sh.D4 - 1)) == 0 && sh.D4 <= WAVE;
  if (fast) {
    if (sh.NS == 1) launch(gatv2_score_kernel<1, true>);
    else if (sh.NS == 2) launch(gatv2_score_kernel<2, true>);
    else launch(gatv2_score_kernel<4, true>);
  } else {
    if (sh.NS == 1) launch(gatv2_score_kernel<1, false>);
    else if (sh.NS == 2) launch(gatv2_score_kernel<2, false>);
    else launch(gatv2_score_kernel<4, false>);
  }
  return out;
}

// Returns {dz_res [n_rows, H, D], dattn [H, D]} (dz_res alone without
// want_dattn). zero_rows: the work list's fifth array — the rows no single
// item overwrites (split and empty ones); only those are cleared.
std::vector<at::Tensor> gatv2_score_bwd(
    at::Tensor wrow, at::Tensor wbeg, at::Tensor wend, at::Tensor wstart,
    at::Tensor zero_rows, at::Tensor indices, c10::optional<at::Tensor> eperm,
    at::Tensor g, at::Tensor z_res, at::Tensor z_str, at::Tensor attn,
    double slope, bool want_dattn) {
  const Shape sh = check_shape("gatv2_score_bwd", z_res, z_str, attn);
  check_f32(g, "g");
  const WorkListArgs wl = worklist_args(wrow, wbeg, wend, wstart);
  const int64_t E = indices.numel();
  TORCH_CHECK(g.dim() == 2 && g.size(0) == E && g.size(1) == sh.H,
              "gatv2_score_bwd: g [E, H] expected");
  TORCH_CHECK(!eperm.has_value() ||
                  (eperm->scalar_type() == at::kLong && eperm->is_cuda() &&
                   eperm->is_contiguous() && eperm->numel() == E),
              "gatv2_score_bwd: eperm must be a contiguous int64 [E] tensor");
  auto dz = at::empty_like(z_res);
  std::vector<at::Tensor> ret = {dz};
  if (E == 0 || wl.n_waves <= 0) {
    dz.zero_();
    if (want_dattn) ret.push_back(at::zeros({sh.H, sh.D}, g.options()));
    return ret;
  }
  if (zero_rows.numel()) dz.index_fill_(0, zero_rows, 0.0);
  const int n_blocks = wl.n_waves / 4;
  at::Tensor part;
  if (want_dattn) part = at::empty({n_blocks, sh.H * sh.D}, g.options());
  const int g_vec4 =
      sh.H == 4 && reinterpret_cast<uintptr_t>(g.data_ptr()) % 16 == 0;
  auto launch = [&](auto kernel) {
    launch_worklist(kernel, wl, 64, indices.data_ptr<int32_t>(),
                    g.data_ptr<float>(),
                    eperm.has_value() ? eperm->data_ptr<int64_t>() : nullptr,
                    z_res.data_ptr<float>(), z_str.data_ptr<float>(),
                    attn.data_ptr<float>(), dz.data_ptr<float>(),
                    want_dattn ? part.data_ptr<float>() : nullptr, sh.H,
                    sh.D4, sh.S, (float)slope, g_vec4);
  };
  if (want_dattn) {
    if (sh.NS == 1) launch(gatv2_score_bwd_kernel<1, true>);
    else if (sh.NS == 2) launch(gatv2_score_bwd_kernel<2, true>);
    else launch(gatv2_score_bwd_kernel<4, true>);
    auto dattn = at::empty({sh.H, sh.D}, g.options());
    const int C = sh.H * sh.D;
    const int n_chunks = (n_blocks + COLSUM_CHUNK - 1) / COLSUM_CHUNK;
    auto sums = at::empty({n_chunks, C}, g.options());
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(gatv2_colsum_kernel,
                       dim3((C + WAVE - 1) / WAVE, n_chunks), dim3(256), 0,
                       stream, part.data_ptr<float>(), sums.data_ptr<float>(),
                       n_blocks, C, COLSUM_CHUNK);
    hipLaunchKernelGGL(gatv2_colsum_kernel, dim3((C + WAVE - 1) / WAVE, 1),
                       dim3(256), 0, stream, sums.data_ptr<float>(),
                       dattn.data_ptr<float>(), n_chunks, C, n_chunks);
    ret.push_back(dattn);
  } else {
    if (sh.NS == 1) launch(gatv2_score_bwd_kernel<1, false>);
    else if (sh.NS == 2) launch(gatv2_score_bwd_kernel<2, false>);
    else launch(gatv2_score_bwd_kernel<4, false>);
  }
  return ret;
}

}  // namespace

namespace bns {

void bind_gatv2(pybind11::module& m) {
  m.def("gatv2_score", &gatv2_score,
        "GATv2 score e = attn . LeakyReLU(zs[col] + zd[row])");
  m.def("gatv2_score_bwd", &gatv2_score_bwd,
        "GATv2 score backward for the resident operand of one CSR "
        "direction (dz_res[, dattn])");
}

}  // namespace bns
