// Per-epoch sampled-halo plan build on the device: the CSR surgery and the
// work lists that boundary-node sampling redoes every epoch
// (parallel/plan.py HaloPlan._build, models/context.py _build_rows_halo),
// bit-identical to their torch counterparts in ops/csr_torch.py.
//
// Three primitives and the scan they share:
//
// * scan — exclusive prefix sum of K int64 arrays at once. A tile is
//   SCAN_TILE = 256 threads x 4 elements; tile totals are scanned by the
//   same code one level up (three levels reach 2^30 elements). The
//   elementwise counting kernels ARE the first level: produce_tile_kernel
//   evaluates a functor, stores the counts and writes the tile totals in
//   one pass. Every counted array carries one extra trailing 0, so after
//   the scan its last element is the total and the array is an indptr.
//
// * csr_gather_rows — segmented copy driven from the OUTPUT side: a wave
//   owns GATHER_CHUNK consecutive output edges, finds the rows its window
//   spans with two wave-uniform binary searches of the new indptr and the
//   row of each edge with a per-lane search inside that (usually one- or
//   two-row) range. Writes are fully coalesced, reads are coalesced within
//   a source row, a row longer than the window is split over waves and
//   short rows share one.
//
// * csr_filter_cols — order-preserving filter-compact. The row space is
//   cut into segments (a row, or a slice of <= L edges of a long row).
//   Pass 1: one wave per segment walks 64 edges at a time — colmap lookup,
//   __ballot, popcount — and writes the segment's kept count. The scan
//   turns counts into write bases; new_indptr[r] is the base of row r's
//   first segment. Pass 2 repeats the walk and writes edge e at
//   base + running + popcount(ballot & lanes_below). No atomics, no sort.
//   With EDGE_MAP the second pass also writes the backward->forward edge
//   map of the sampled halo block from the values it already holds.
//
// * build_worklist — csr_torch.build_worklist: items per row counted and
//   scanned together with the empty-row and split-row flags; one thread
//   per item finds its row by binary search of the scanned item counts;
//   wave_start[w] is a left binary search of wbeg (= the torch code's
//   prefix sum of item lengths, shifted by indptr[0]) for
//   trunc(double(E) * double(w) / n_waves), the same IEEE operations in
//   the same order as the torch expression. A segment table is a work
//   list without the row ids, so the dynamic one of rows_halo_build comes
//   from the same item kernel.
//
// Host synchronisation: each entry point runs every counting stage, reads
// ONE small vector of totals back, allocates, then runs every fill stage.
// Preconditions (not checked on the device): rows / hsel index valid rows,
// column ids index colmap, indptr is non-decreasing.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>
#include <algorithm>
#include <tuple>
#include <vector>
#include "common.h"
#include "plan_build.h"

namespace {

constexpr int TPB = 256;
constexpr int SCAN_ITEMS = 4;
constexpr int64_t SCAN_TILE = TPB * SCAN_ITEMS;      // 1024
constexpr int GATHER_CHUNK = 256;                    // output edges per wave

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------ scan
DEV_INLINE int64_t wave_incl_scan(int64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const int64_t u = __shfl_up(v, d, WAVE);
    if (lane >= d) v += u;
  }
  return v;
}

// Exclusive prefix of v over the block's threads; total = the block's sum.
DEV_INLINE int64_t block_excl_scan(int64_t v, int64_t& total) {
  __shared__ int64_t wsum[TPB / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const int64_t incl = wave_incl_scan(v, lane);
  __syncthreads();                       // wsum is reused by the next call
  if (lane == WAVE - 1) wsum[w] = incl;
  __syncthreads();
  int64_t off = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < TPB / WAVE; ++i) {
    if (i < w) off += wsum[i];
    total += wsum[i];
  }
  return off + incl - v;
}

// First scan level fused with an elementwise producer: f(i, v) yields the
// K values of element i; they are stored at out[k * stride + i] (if out)
// and each tile's sums at tile_tot[k * nb + tile].
template <int K, class F>
__global__ void __launch_bounds__(TPB)
produce_tile_kernel(F f, int64_t* __restrict__ out, int64_t stride, int64_t n,
                    int64_t* __restrict__ tile_tot, int64_t nb) {
  const int64_t i0 = ((int64_t)blockIdx.x * TPB + threadIdx.x) * SCAN_ITEMS;
  int64_t s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    const int64_t i = i0 + j;
    if (i < n) {
      int64_t v[K];
      f(i, v);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (out) out[k * stride + i] = v[k];
        s[k] += v[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int64_t tot;
    block_excl_scan(s[k], tot);
    if (threadIdx.x == 0) tile_tot[k * nb + blockIdx.x] = tot;
  }
}

// Producer that re-reads K stored arrays (tile totals of counts that a
// wave-per-segment kernel wrote).
template <int K>
struct LoadStored {
  const int64_t* data;
  int64_t stride;
  DEV_INLINE void operator()(int64_t i, int64_t (&v)[K]) const {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = data[k * stride + i];
  }
};

// In-place exclusive scan of one tile per block, plus the tile's offset
// from the level above (tile_off, null at the top). grand (top level
// only): the K totals.
template <int K>
__global__ void __launch_bounds__(TPB)
tile_scan_kernel(int64_t* __restrict__ data, int64_t stride, int64_t n,
                 const int64_t* __restrict__ tile_off, int64_t nb,
                 int64_t* __restrict__ grand) {
  const int64_t i0 = ((int64_t)blockIdx.x * TPB + threadIdx.x) * SCAN_ITEMS;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int64_t v[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      v[j] = (i0 + j < n) ? data[k * stride + i0 + j] : 0;
      s += v[j];
    }
    int64_t tot;
    int64_t run = block_excl_scan(s, tot);
    if (tile_off) run += tile_off[k * nb + blockIdx.x];
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      if (i0 + j < n) data[k * stride + i0 + j] = run;
      run += v[j];
    }
    if (grand && threadIdx.x == 0) grand[k] = tot;
  }
}

// Exclusive scan of data[k * stride + 0 .. n) for k < K, in place. tile_tot:
// the [K, nb] tile totals if a producer already wrote them, else null.
// grand: device pointer receiving the K totals, or null.
template <int K>
void scan_tiles(int64_t* data, int64_t stride, int64_t n, int64_t* tile_tot,
                int64_t* grand, const at::TensorOptions& lopt,
                hipStream_t stream) {
  const int64_t nb = cdiv(n, SCAN_TILE);
  if (nb <= 1) {
    hipLaunchKernelGGL(tile_scan_kernel<K>, dim3(1), dim3(TPB), 0, stream,
                       data, stride, n, (const int64_t*)nullptr, (int64_t)1,
                       grand);
    return;
  }
  at::Tensor tt;
  if (!tile_tot) {
    tt = at::empty({K * nb}, lopt);
    tile_tot = tt.data_ptr<int64_t>();
    hipLaunchKernelGGL((produce_tile_kernel<K, LoadStored<K>>), dim3(nb),
                       dim3(TPB), 0, stream, LoadStored<K>{data, stride},
                       (int64_t*)nullptr, (int64_t)0, n, tile_tot, nb);
  }
  scan_tiles<K>(tile_tot, nb, nb, nullptr, grand, lopt, stream);
  hipLaunchKernelGGL(tile_scan_kernel<K>, dim3(nb), dim3(TPB), 0, stream, data,
                     stride, n, (const int64_t*)tile_tot, nb,
                     (int64_t*)nullptr);
}

// out[k * stride + i] = exclusive prefix over i of f's k-th value, i < n.
template <int K, class F>
void produce_and_scan(F f, int64_t* out, int64_t stride, int64_t n,
                      int64_t* grand, const at::TensorOptions& lopt,
                      hipStream_t stream) {
  const int64_t nb = cdiv(n, SCAN_TILE);
  at::Tensor tt = at::empty({K * nb}, lopt);
  hipLaunchKernelGGL((produce_tile_kernel<K, F>), dim3(nb), dim3(TPB), 0,
                     stream, f, out, stride, n, tt.data_ptr<int64_t>(), nb);
  scan_tiles<K>(out, stride, n, tt.data_ptr<int64_t>(), grand, lopt, stream);
}

// Largest r in [lo, hi] with a[r] <= x (a non-decreasing, a[lo] <= x).
DEV_INLINE int64_t last_le(const int64_t* __restrict__ a, int64_t lo,
                           int64_t hi, int64_t x) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (a[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ----------------------------------------------------------- gather rows
struct GatherLen {            // length of new row i; the trailing element 0
  const int64_t* indptr;
  const int64_t* rows;
  int64_t R;
  DEV_INLINE void operator()(int64_t i, int64_t (&v)[1]) const {
    v[0] = 0;
    if (i < R) {
      const int64_t r = rows[i];
      v[0] = indptr[r + 1] - indptr[r];
    }
  }
};

__global__ void __launch_bounds__(TPB)
gather_copy_kernel(const int64_t* __restrict__ indptr,
                   const int32_t* __restrict__ indices,
                   const int64_t* __restrict__ rows,
                   const int64_t* __restrict__ new_ip, int64_t R, int64_t E,
                   int32_t* __restrict__ out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t w = (int64_t)blockIdx.x * (TPB / WAVE) + threadIdx.x / WAVE;
  const int64_t base = w * GATHER_CHUNK;
  if (base >= E) return;
  const int64_t lim = (base + GATHER_CHUNK < E) ? base + GATHER_CHUNK : E;
  // rows the window spans (new_ip[0] = 0 <= base, new_ip[R] = E > lim - 1)
  const int64_t r_lo = last_le(new_ip, 0, R - 1, base);
  const int64_t r_hi = last_le(new_ip, r_lo, R - 1, lim - 1);
  for (int64_t e = base + lane; e < lim; e += WAVE) {
    const int64_t r = last_le(new_ip, r_lo, r_hi, e);
    out[e] = indices[indptr[rows[r]] + (e - new_ip[r])];
  }
}

// ----------------------------------------------------------- filter cols
struct EpermArgs {            // sampled halo block: backward -> forward map
  const int64_t* t_eperm;     // static transposed edge -> static halo edge
  const int64_t* halo_ip;     // static halo indptr
  const int64_t* bwd_ip;      // sampled backward indptr
  int64_t* eperm_t;           // out, one entry per sampled backward edge
};

// One wave per segment. FILL = false: cnt[s] = kept edges of segment s
// (0 for s >= *n_seg, so the scan may run over the launched range).
// FILL = true: cnt holds the scanned write bases.
template <bool FILL, bool EDGE_MAP>
__global__ void __launch_bounds__(TPB)
filter_kernel(const int64_t* __restrict__ seg_beg,
              const int64_t* __restrict__ seg_end,
              const int64_t* __restrict__ n_seg, int64_t n_launch,
              const int32_t* __restrict__ indices,
              const int32_t* __restrict__ colmap, int64_t* __restrict__ cnt,
              int32_t* __restrict__ new_indices, int64_t* __restrict__ kept,
              EpermArgs ep) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t s = (int64_t)blockIdx.x * (TPB / WAVE) + threadIdx.x / WAVE;
  if (s >= n_launch) return;
  if (s >= *n_seg) {
    if (!FILL && lane == 0) cnt[s] = 0;
    return;
  }
  const int64_t beg = seg_beg[s], end = seg_end[s];
  int64_t run = FILL ? cnt[s] : 0;
  const uint64_t below = (1ull << lane) - 1ull;
  for (int64_t e0 = beg; e0 < end; e0 += WAVE) {
    const int64_t e = e0 + lane;
    int32_t h = 0, c = -1;
    if (e < end) {
      h = indices[e];
      c = colmap[h];
    }
    const uint64_t b = __ballot(c >= 0);
    if (FILL && c >= 0) {
      const int64_t k = run + __popcll(b & below);
      new_indices[k] = c;
      if (kept) kept[k] = e;
      if (EDGE_MAP)
        ep.eperm_t[ep.bwd_ip[c] + (ep.t_eperm[e] - ep.halo_ip[h])] = k;
    }
    run += __popcll(b);
  }
  if (!FILL && lane == 0) cnt[s] = run;
}

// new_indptr[r] = write base of row r's first segment, r <= n_rows
// (row_seg[n_rows] = number of segments, whose base is the total).
__global__ void __launch_bounds__(TPB)
row_base_kernel(const int64_t* __restrict__ base,
                const int64_t* __restrict__ row_seg, int64_t n,
                int64_t* __restrict__ new_ip) {
  const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (r < n) new_ip[r] = base[row_seg[r]];
}

// pos[hsel[k]] = k (set) or -1 (restore): only the sampled entries of the
// n_halo-long map are ever touched.
__global__ void __launch_bounds__(TPB)
scatter_pos_kernel(const int64_t* __restrict__ hsel, int64_t R,
                   int32_t* __restrict__ pos, bool set) {
  const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (k < R) pos[hsel[k]] = set ? (int32_t)k : -1;
}

// -------------------------------------------------------------- work list
struct WorkCount {     // items of row i, empty flag, split flag; trailing 0
  const int64_t* indptr;
  int64_t n, seg;
  DEV_INLINE void operator()(int64_t i, int64_t (&v)[3]) const {
    v[0] = v[1] = v[2] = 0;
    if (i < n) {
      const int64_t deg = indptr[i + 1] - indptr[i];
      v[0] = (deg + seg - 1) / seg;
      v[1] = deg == 0;
      v[2] = v[0] > 1;
    }
  }
};

struct SegCount {      // segments (items without the flags) of row i
  const int64_t* indptr;
  int64_t n, seg;
  DEV_INLINE void operator()(int64_t i, int64_t (&v)[1]) const {
    v[0] = (i < n) ? (indptr[i + 1] - indptr[i] + seg - 1) / seg : 0;
  }
};

// One thread per item k < item_first[n] (the launch may be larger): row by
// binary search of the scanned item counts, then the item's edge range.
// wrow may be null (segment table).
__global__ void __launch_bounds__(TPB)
items_kernel(const int64_t* __restrict__ indptr,
             const int64_t* __restrict__ item_first, int64_t n, int64_t seg,
             int64_t n_launch, int32_t* __restrict__ wrow,
             int64_t* __restrict__ wbeg, int64_t* __restrict__ wend) {
  const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (k >= n_launch || k >= item_first[n]) return;
  const int64_t r = last_le(item_first, 0, n - 1, k);
  const int64_t b = indptr[r] + (k - item_first[r]) * seg;
  const int64_t rend = indptr[r + 1];
  wbeg[k] = b;
  wend[k] = (b + seg < rend) ? b + seg : rend;
  if (wrow)
    wrow[k] = (item_first[r + 1] - item_first[r] > 1) ? ~(int32_t)r
                                                      : (int32_t)r;
}

// zero_rows = empty rows ascending, then split rows ascending: two ordered
// compactions from the scanned flags (sc rows 1 and 2, stride n + 1).
__global__ void __launch_bounds__(TPB)
zero_rows_kernel(const int64_t* __restrict__ sc, int64_t n, int64_t n_empty,
                 int64_t* __restrict__ zero_rows) {
  const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (r >= n) return;
  const int64_t* eo = sc + (n + 1);
  const int64_t* so = sc + 2 * (n + 1);
  if (eo[r + 1] > eo[r]) zero_rows[eo[r]] = r;
  if (so[r + 1] > so[r]) zero_rows[n_empty + so[r]] = r;
}

__global__ void __launch_bounds__(TPB)
wave_start_kernel(const int64_t* __restrict__ wbeg, int64_t total,
                  const int64_t* __restrict__ indptr, int64_t n,
                  int64_t n_waves, int32_t* __restrict__ wave_start) {
  const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (w > n_waves) return;
  int64_t res;
  if (w == 0) {
    res = 0;
  } else if (w == n_waves) {
    res = total;
  } else {
    const int64_t first = indptr[0], E = indptr[n] - first;
    const int64_t t = (int64_t)((double)E * (double)w / (double)n_waves);
    // first i in [0, total] with cum[i] >= t; cum[i] = wbeg[i] - first for
    // i < total and cum[total] = E >= t
    int64_t lo = 0, hi = total;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (wbeg[mid] - first >= t) hi = mid; else lo = mid + 1;
    }
    res = lo;
  }
  wave_start[w] = (int32_t)res;
}

// ------------------------------------------------------------ host stages
inline dim3 grid_of(int64_t n_threads) {
  return dim3((unsigned)cdiv(n_threads, TPB));
}

void check_i64(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 1 &&
              t.scalar_type() == at::kLong, name, ": 1-D int64 cuda tensor");
}
void check_i32(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 1 &&
              t.scalar_type() == at::kInt, name, ": 1-D int32 cuda tensor");
}
void check_csr(const at::Tensor& indptr, const at::Tensor& indices) {
  check_i64(indptr, "indptr");
  check_i32(indices, "indices");
  TORCH_CHECK(indptr.numel() >= 1, "indptr is empty");
}

struct Ctx {
  hipStream_t stream;
  at::TensorOptions lopt, iopt;
  explicit Ctx(const at::Tensor& t)
      : stream(at::cuda::getCurrentCUDAStream()),
        lopt(t.options().dtype(at::kLong)),
        iopt(t.options().dtype(at::kInt)) {}
};

// gather, counting stage: the new indptr; its total goes to *tot.
at::Tensor gather_count(const Ctx& c, const at::Tensor& indptr,
                        const at::Tensor& rows, int64_t* tot) {
  const int64_t R = rows.numel();
  at::Tensor new_ip = at::empty({R + 1}, c.lopt);
  produce_and_scan<1>(GatherLen{indptr.data_ptr<int64_t>(),
                                rows.data_ptr<int64_t>(), R},
                      new_ip.data_ptr<int64_t>(), R + 1, R + 1, tot, c.lopt,
                      c.stream);
  return new_ip;
}

at::Tensor gather_fill(const Ctx& c, const at::Tensor& indptr,
                       const at::Tensor& indices, const at::Tensor& rows,
                       const at::Tensor& new_ip, int64_t E) {
  at::Tensor out = at::empty({E}, c.iopt);
  if (E > 0)
    hipLaunchKernelGGL(gather_copy_kernel,
                       grid_of(cdiv(E, GATHER_CHUNK) * WAVE), dim3(TPB), 0,
                       c.stream, indptr.data_ptr<int64_t>(),
                       indices.data_ptr<int32_t>(), rows.data_ptr<int64_t>(),
                       new_ip.data_ptr<int64_t>(), rows.numel(), E,
                       out.data_ptr<int32_t>());
  return out;
}

// Segment table of a CSR: segment s covers edges [beg[s], end[s]); row r's
// segments are row_seg[r] .. row_seg[r + 1] (none for an empty row).
// n_launch >= the number of segments bounds what the kernels launch; the
// exact number is row_seg[n_rows], read on the device.
struct Segs {
  at::Tensor beg, end, row_seg;
  int64_t n_launch;
};

// Segment table of a per-epoch CSR, built without a read-back: sized by
// the bound sum(ceil(deg / L)) <= E / L + n_rows.
Segs segments_of(const Ctx& c, const at::Tensor& indptr, int64_t E,
                 int64_t L) {
  const int64_t n = indptr.numel() - 1;
  Segs s;
  s.n_launch = E / L + n;
  s.row_seg = at::empty({n + 1}, c.lopt);
  s.beg = at::empty({s.n_launch}, c.lopt);
  s.end = at::empty({s.n_launch}, c.lopt);
  produce_and_scan<1>(SegCount{indptr.data_ptr<int64_t>(), n, L},
                      s.row_seg.data_ptr<int64_t>(), n + 1, n + 1, nullptr,
                      c.lopt, c.stream);
  if (s.n_launch > 0)
    hipLaunchKernelGGL(items_kernel, grid_of(s.n_launch), dim3(TPB), 0,
                       c.stream, indptr.data_ptr<int64_t>(),
                       s.row_seg.data_ptr<int64_t>(), n, L, s.n_launch,
                       (int32_t*)nullptr, s.beg.data_ptr<int64_t>(),
                       s.end.data_ptr<int64_t>());
  return s;
}

struct FilterCount { at::Tensor base, new_ip; };

// filter, counting stage: pass 1, the scan and the new indptr.
FilterCount filter_count(const Ctx& c, const Segs& s,
                         const at::Tensor& indices, const at::Tensor& colmap,
                         int64_t* tot) {
  const int64_t n = s.row_seg.numel() - 1, nl = s.n_launch + 1;
  FilterCount f{at::empty({nl}, c.lopt), at::empty({n + 1}, c.lopt)};
  const int64_t* n_seg = s.row_seg.data_ptr<int64_t>() + n;
  hipLaunchKernelGGL((filter_kernel<false, false>), grid_of(nl * WAVE),
                     dim3(TPB), 0, c.stream, s.beg.data_ptr<int64_t>(),
                     s.end.data_ptr<int64_t>(), n_seg, nl,
                     indices.data_ptr<int32_t>(), colmap.data_ptr<int32_t>(),
                     f.base.data_ptr<int64_t>(), (int32_t*)nullptr,
                     (int64_t*)nullptr, EpermArgs{});
  scan_tiles<1>(f.base.data_ptr<int64_t>(), nl, nl, nullptr, tot, c.lopt,
                c.stream);
  hipLaunchKernelGGL(row_base_kernel, grid_of(n + 1), dim3(TPB), 0, c.stream,
                     f.base.data_ptr<int64_t>(),
                     s.row_seg.data_ptr<int64_t>(), n + 1,
                     f.new_ip.data_ptr<int64_t>());
  return f;
}

// filter, fill stage: pass 2. kept / ep.eperm_t are optional outputs.
at::Tensor filter_fill(const Ctx& c, const Segs& s, const FilterCount& f,
                       const at::Tensor& indices, const at::Tensor& colmap,
                       int64_t E, int64_t* kept, const EpermArgs* ep) {
  at::Tensor out = at::empty({E}, c.iopt);
  if (E == 0) return out;
  const int64_t n = s.row_seg.numel() - 1;
  const int64_t* n_seg = s.row_seg.data_ptr<int64_t>() + n;
  auto launch = [&](auto kernel, const EpermArgs& e) {
    hipLaunchKernelGGL(kernel, grid_of(s.n_launch * WAVE), dim3(TPB), 0,
                       c.stream, s.beg.data_ptr<int64_t>(),
                       s.end.data_ptr<int64_t>(), n_seg, s.n_launch,
                       indices.data_ptr<int32_t>(),
                       colmap.data_ptr<int32_t>(),
                       f.base.data_ptr<int64_t>(), out.data_ptr<int32_t>(),
                       kept, e);
  };
  if (ep) launch(filter_kernel<true, true>, *ep);
  else launch(filter_kernel<true, false>, EpermArgs{});
  return out;
}

using WorkListT = std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                             at::Tensor>;

// work list, counting stage: the scanned [3, n + 1] item counts and flags;
// tot[0..2] = items, empty rows, split rows.
at::Tensor worklist_count(const Ctx& c, const at::Tensor& indptr, int64_t seg,
                          int64_t* tot) {
  const int64_t n = indptr.numel() - 1;
  at::Tensor sc = at::empty({3, n + 1}, c.lopt);
  produce_and_scan<3>(WorkCount{indptr.data_ptr<int64_t>(), n, seg},
                      sc.data_ptr<int64_t>(), n + 1, n + 1, tot, c.lopt,
                      c.stream);
  return sc;
}

WorkListT worklist_fill(const Ctx& c, const at::Tensor& indptr,
                        const at::Tensor& sc, const int64_t* tot, int64_t seg,
                        int64_t max_waves) {
  const int64_t n = indptr.numel() - 1;
  const int64_t total = tot[0], n_empty = tot[1], n_split = tot[2];
  TORCH_CHECK(total < (int64_t(1) << 31) && n < (int64_t(1) << 31),
              "work list: item or row count does not fit int32");
  at::Tensor zero_rows = at::empty({n_empty + n_split}, c.lopt);
  if (zero_rows.numel() > 0)
    hipLaunchKernelGGL(zero_rows_kernel, grid_of(n), dim3(TPB), 0, c.stream,
                       sc.data_ptr<int64_t>(), n, n_empty,
                       zero_rows.data_ptr<int64_t>());
  at::Tensor wrow = at::empty({total}, c.iopt);
  at::Tensor wbeg = at::empty({total}, c.lopt);
  at::Tensor wend = at::empty({total}, c.lopt);
  if (total == 0)
    return {wrow, wbeg, wend, at::zeros({1}, c.iopt), zero_rows};
  hipLaunchKernelGGL(items_kernel, grid_of(total), dim3(TPB), 0, c.stream,
                     indptr.data_ptr<int64_t>(), sc.data_ptr<int64_t>(), n,
                     seg, total, wrow.data_ptr<int32_t>(),
                     wbeg.data_ptr<int64_t>(), wend.data_ptr<int64_t>());
  if (total >= 1000000) max_waves = std::max<int64_t>(max_waves, 262144);
  int64_t n_waves = std::min(max_waves, std::max<int64_t>(8, total));
  n_waves = (n_waves + 7) / 8 * 8;
  at::Tensor wave_start = at::empty({n_waves + 1}, c.iopt);
  hipLaunchKernelGGL(wave_start_kernel, grid_of(n_waves + 1), dim3(TPB), 0,
                     c.stream, wbeg.data_ptr<int64_t>(), total,
                     indptr.data_ptr<int64_t>(), n, n_waves,
                     wave_start.data_ptr<int32_t>());
  return {wrow, wbeg, wend, wave_start, zero_rows};
}

// The one device-to-host copy of an entry point.
std::vector<int64_t> read_totals(const at::Tensor& tot) {
  at::Tensor h = tot.cpu();
  const int64_t* p = h.data_ptr<int64_t>();
  return std::vector<int64_t>(p, p + h.numel());
}

void check_work_args(int64_t seg, int64_t max_waves) {
  TORCH_CHECK(seg >= 1 && max_waves >= 1, "seg and max_waves must be >= 1");
}

// ------------------------------------------------------------ entry points
std::tuple<at::Tensor, at::Tensor> csr_gather_rows(const at::Tensor& indptr,
                                                   const at::Tensor& indices,
                                                   const at::Tensor& rows) {
  check_csr(indptr, indices);
  check_i64(rows, "rows");
  c10::cuda::CUDAGuard guard(indptr.device());
  Ctx c(indptr);
  at::Tensor tot = at::empty({1}, c.lopt);
  at::Tensor new_ip = gather_count(c, indptr, rows, tot.data_ptr<int64_t>());
  const auto h = read_totals(tot);
  return {new_ip, gather_fill(c, indptr, indices, rows, new_ip, h[0])};
}

Segs static_segs(const at::Tensor& seg_beg, const at::Tensor& seg_end,
                 const at::Tensor& row_seg, int64_t n_rows) {
  check_i64(seg_beg, "seg_beg");
  check_i64(seg_end, "seg_end");
  check_i64(row_seg, "row_seg");
  TORCH_CHECK(seg_end.numel() == seg_beg.numel() &&
              row_seg.numel() == n_rows + 1, "segment table shape");
  return Segs{seg_beg, seg_end, row_seg, seg_beg.numel()};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> csr_filter_cols(
    const at::Tensor& indptr, const at::Tensor& indices,
    const at::Tensor& colmap, const at::Tensor& seg_beg,
    const at::Tensor& seg_end, const at::Tensor& row_seg) {
  check_csr(indptr, indices);
  check_i32(colmap, "colmap");
  c10::cuda::CUDAGuard guard(indptr.device());
  Ctx c(indptr);
  const Segs s = static_segs(seg_beg, seg_end, row_seg, indptr.numel() - 1);
  at::Tensor tot = at::empty({1}, c.lopt);
  const FilterCount f =
      filter_count(c, s, indices, colmap, tot.data_ptr<int64_t>());
  const auto h = read_totals(tot);
  at::Tensor kept = at::empty({h[0]}, c.lopt);
  at::Tensor out = filter_fill(c, s, f, indices, colmap, h[0],
                               kept.data_ptr<int64_t>(), nullptr);
  return {f.new_ip, out, kept};
}

WorkListT build_worklist(const at::Tensor& indptr, int64_t seg,
                         int64_t max_waves) {
  check_i64(indptr, "indptr");
  TORCH_CHECK(indptr.numel() >= 1, "indptr is empty");
  check_work_args(seg, max_waves);
  c10::cuda::CUDAGuard guard(indptr.device());
  Ctx c(indptr);
  at::Tensor tot = at::empty({3}, c.lopt);
  at::Tensor sc = worklist_count(c, indptr, seg, tot.data_ptr<int64_t>());
  const auto h = read_totals(tot);
  return worklist_fill(c, indptr, sc, h.data(), seg, max_waves);
}

// HaloPlan._build: sampled backward CSR (gather of the static halo CSR by
// hsel), sampled forward CSR (filter of the static transposed halo CSR by
// pos = inverse of hsel), the backward -> forward edge map and both work
// lists. pos is all -1 on entry and on return.
std::vector<at::Tensor> halo_epoch_build(
    const at::Tensor& halo_ip, const at::Tensor& halo_ix,
    const at::Tensor& hsel, const at::Tensor& t_ix, const at::Tensor& t_eperm,
    const at::Tensor& t_seg_beg, const at::Tensor& t_seg_end,
    const at::Tensor& t_row_seg, const at::Tensor& pos, int64_t seg,
    int64_t max_waves) {
  check_csr(halo_ip, halo_ix);
  check_i64(hsel, "hsel");
  check_i32(t_ix, "t_indices");
  check_i64(t_eperm, "t_eperm");
  check_i32(pos, "pos");
  check_work_args(seg, max_waves);
  TORCH_CHECK(pos.numel() == halo_ip.numel() - 1 &&
              t_ix.numel() == halo_ix.numel() &&
              t_eperm.numel() == halo_ix.numel() &&
              hsel.numel() <= pos.numel(), "halo plan shapes");
  c10::cuda::CUDAGuard guard(halo_ip.device());
  Ctx c(halo_ip);
  const Segs s = static_segs(t_seg_beg, t_seg_end, t_row_seg,
                             t_row_seg.numel() - 1);
  const int64_t R = hsel.numel();
  auto scatter = [&](bool set) {
    if (R > 0)
      hipLaunchKernelGGL(scatter_pos_kernel, grid_of(R), dim3(TPB), 0,
                         c.stream, hsel.data_ptr<int64_t>(), R,
                         pos.data_ptr<int32_t>(), set);
  };
  at::Tensor tot = at::empty({8}, c.lopt);
  int64_t* t = tot.data_ptr<int64_t>();
  at::Tensor bwd_ip = gather_count(c, halo_ip, hsel, t + 0);
  scatter(true);
  const FilterCount f = filter_count(c, s, t_ix, pos, t + 1);
  at::Tensor scb = worklist_count(c, bwd_ip, seg, t + 2);
  at::Tensor scf = worklist_count(c, f.new_ip, seg, t + 5);
  const auto h = read_totals(tot);
  TORCH_CHECK(h[0] == h[1], "halo plan: transposed halo CSR does not match");
  at::Tensor bwd_ix = gather_fill(c, halo_ip, halo_ix, hsel, bwd_ip, h[0]);
  at::Tensor eperm_t = at::empty({h[0]}, c.lopt);
  const EpermArgs ep{t_eperm.data_ptr<int64_t>(), halo_ip.data_ptr<int64_t>(),
                     bwd_ip.data_ptr<int64_t>(),
                     eperm_t.data_ptr<int64_t>()};
  at::Tensor fwd_ix = filter_fill(c, s, f, t_ix, pos, h[1], nullptr, &ep);
  scatter(false);
  const WorkListT wb = worklist_fill(c, bwd_ip, scb, &h[2], seg, max_waves);
  const WorkListT wf = worklist_fill(c, f.new_ip, scf, &h[5], seg, max_waves);
  return {bwd_ip, bwd_ix, f.new_ip, fwd_ix, eperm_t,
          std::get<0>(wb), std::get<1>(wb), std::get<2>(wb), std::get<3>(wb),
          std::get<4>(wb),
          std::get<0>(wf), std::get<1>(wf), std::get<2>(wf), std::get<3>(wf),
          std::get<4>(wf)};
}

// GraphContext._build_rows_halo: the sampled forward CSR gathered to the
// train rows, its transpose as the sampled backward CSR filtered to those
// columns (inner_pos: inner id -> position in the train rows, or -1), and
// both work lists. L: edges per segment of the backward CSR.
std::vector<at::Tensor> rows_halo_build(
    const at::Tensor& fwd_ip, const at::Tensor& fwd_ix,
    const at::Tensor& rows, const at::Tensor& bwd_ip,
    const at::Tensor& bwd_ix, const at::Tensor& inner_pos, int64_t L,
    int64_t seg, int64_t max_waves) {
  check_csr(fwd_ip, fwd_ix);
  check_csr(bwd_ip, bwd_ix);
  check_i64(rows, "rows");
  check_i32(inner_pos, "inner_pos");
  check_work_args(seg, max_waves);
  TORCH_CHECK(L >= 1 && inner_pos.numel() == fwd_ip.numel() - 1,
              "rows halo shapes");
  c10::cuda::CUDAGuard guard(fwd_ip.device());
  Ctx c(fwd_ip);
  at::Tensor tot = at::empty({8}, c.lopt);
  int64_t* t = tot.data_ptr<int64_t>();
  at::Tensor hf_ip = gather_count(c, fwd_ip, rows, t + 0);
  const Segs s = segments_of(c, bwd_ip, bwd_ix.numel(), L);
  const FilterCount f = filter_count(c, s, bwd_ix, inner_pos, t + 1);
  at::Tensor scf = worklist_count(c, hf_ip, seg, t + 2);
  at::Tensor scb = worklist_count(c, f.new_ip, seg, t + 5);
  const auto h = read_totals(tot);
  at::Tensor hf_ix = gather_fill(c, fwd_ip, fwd_ix, rows, hf_ip, h[0]);
  at::Tensor hb_ix =
      filter_fill(c, s, f, bwd_ix, inner_pos, h[1], nullptr, nullptr);
  const WorkListT wf = worklist_fill(c, hf_ip, scf, &h[2], seg, max_waves);
  const WorkListT wb = worklist_fill(c, f.new_ip, scb, &h[5], seg, max_waves);
  return {hf_ip, hf_ix, f.new_ip, hb_ix,
          std::get<0>(wf), std::get<1>(wf), std::get<2>(wf), std::get<3>(wf),
          std::get<4>(wf),
          std::get<0>(wb), std::get<1>(wb), std::get<2>(wb), std::get<3>(wb),
          std::get<4>(wb)};
}

}  // namespace

namespace bns {

void bind_plan_build(pybind11::module& m) {
  namespace py = pybind11;
  m.attr("PLAN_SCAN_TILE") = SCAN_TILE;
  m.def("csr_gather_rows", &csr_gather_rows,
        "sub-CSR of the listed rows (new_indptr, new_indices)",
        py::arg("indptr"), py::arg("indices"), py::arg("rows"));
  m.def("csr_filter_cols", &csr_filter_cols,
        "order-preserving column filter (new_indptr, new_indices, kept)",
        py::arg("indptr"), py::arg("indices"), py::arg("colmap"),
        py::arg("seg_beg"), py::arg("seg_end"), py::arg("row_seg"));
  m.def("build_worklist", &build_worklist,
        "edge-balanced work list (wrow, wbeg, wend, wave_start, zero_rows)",
        py::arg("indptr"), py::arg("seg"), py::arg("max_waves"));
  m.def("halo_epoch_build", &halo_epoch_build,
        "per-epoch sampled halo CSRs, edge map and work lists");
  m.def("rows_halo_build", &rows_halo_build,
        "train-row-restricted sampled halo CSRs and work lists");
}

}  // namespace bns
