// Boundary-node selection for LARGE segments: the selection of
// bns_select.hip — the s smallest of n keys, positions ascending,
// bit-identical to sort(argsort(keys, stable)[:s]) — with every segment cut
// into slices of slice_rows consecutive positions and one workgroup of 256
// threads per (segment, slice) work item, so that a segment of millions of
// rows fills the device instead of one compute unit.
//
// No workgroup waits for another: what one pass hands to the next goes
// through global scratch and the order of the launches on the stream. The
// host fixes the sequence and the grids when the job is constructed; all
// launches are enqueued unconditionally and nothing is read back. Keys are
// recomputed from the KeySrc in every pass, never stored. The only atomics
// are integer adds (LDS and global), and no result depends on the order in
// which they land: histogram bins and counters are sums, and the candidate
// buffer is read by a counting that does not look at slot order.
//
//   L0..L5  level: each item first brings the segment's state up to date —
//           a scan of the 2048 bins of the previous level's finished
//           histogram gives the pivot bin, the keys below it and the rank
//           wanted inside it (every block of a segment computes the same
//           state, the block of slice 0 stores it for the next launch) —
//           and then, unless the state is `done` (pivot bin <= CAP keys, or
//           all 63 bits fixed), adds its slice's LDS histogram of the next
//           11 bits (8 at the last level) into the segment's global one.
//           Blocks of a finished segment return after reading the state.
//   collect the final state from the last histogram; each item appends its
//           keys of the pivot bin to the segment's candidate buffer (CAP
//           (key, position) pairs, one slot counter) if the bin holds
//           <= CAP keys, and always stores how many it holds: match[item].
//   thresh  one workgroup of 1024 threads per segment: the threshold pair
//           (T, P) by the counting of bns_select.hip over the candidates;
//           or, with all bits fixed and more than CAP equal keys, T =
//           prefix, the slice holding the rank-th of them from a scan of
//           match[], and P from a ballot walk of that one slice.
//   count   cnt[item] = rows of the slice with (key, i) <= (T, P).
//   emit    base = sum of cnt[] over the earlier slices of the segment,
//           then the slice in index order in chunks of 256 (ballot +
//           popcount): row i of rank k goes to out_off + k as its final
//           value, exactly as in bns_select.hip.
//
// Segments with s >= n run only the emit (base = first position of the
// slice). Scratch per call, from host-known bounds: per segment 6 x 2048
// histogram bins and a slot counter (zeroed by one fill), 7 states, CAP
// candidates and the threshold; per item match and cnt.
//
// Preconditions as in bns_select.hip, checked by ops/bns_select.py and the
// binding: n < 2^31, slice_rows a multiple of 256 and <= 2^30, items list
// every slice of every segment of the table in order.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include "common.h"
#include "bns_select_dev.h"

namespace {

using namespace bns;

constexpr int TPB = SLICE_TPB;
constexpr int NW = TPB / WAVE;                 // 4
constexpr int BPT = NBIN / TPB;                // 8 bins per thread
constexpr int THR_TPB = 1024;                  // threshold kernel
constexpr int THR_NW = THR_TPB / WAVE;
constexpr int N_LEVEL = 6;                     // 5 x 11 bits + 8
constexpr int N_STATE = N_LEVEL + 1;           // before each level + final
static_assert(BPT == 8, "the pivot scan reads two uint4 per thread");
static_assert((N_LEVEL - 1) * RADIX_BITS < KEY_BITS &&
              N_LEVEL * RADIX_BITS >= KEY_BITS, "levels cover the key");

// Descent state of a segment: the key's bits above `shift` are `prefix`,
// the key wanted is the rank-th (1-based) of the in_bin keys sharing them.
struct SelState {
  uint64_t prefix;
  int32_t shift, rank, in_bin, done;
};
static_assert(sizeof(SelState) == 24, "three int64 of scratch per state");

struct Scratch {
  uint32_t* hist;        // [n_sseg][N_LEVEL][NBIN], zeroed
  int32_t* n_cand;       // [n_sseg], zeroed
  SelState* st;          // [n_sseg][N_STATE]
  uint64_t* cand_key;    // [n_sseg][cap]
  int32_t* cand_pos;     // [n_sseg][cap]
  uint64_t* thr_key;     // [n_sseg]
  int32_t* thr_pos;      // [n_sseg]
  int32_t* match;        // [n_item]
  int32_t* cnt;          // [n_item]
};

// The work item of the calling block.
struct Item {
  const int64_t* sg;     // row of the segment table
  int seg, slice;
  int n, s;              // rows, min(s, n) > 0
  int start, len;        // positions [start, start + len) of the segment
  bool all;              // s >= n: everything is selected
};

DEV_INLINE Item load_item(const int64_t* __restrict__ ssegs,
                          const int32_t* __restrict__ items, int slice_rows) {
  Item it;
  it.seg = items[2 * blockIdx.x];
  it.slice = items[2 * blockIdx.x + 1];
  it.sg = ssegs + (int64_t)it.seg * SSEG_COLS;
  it.n = (int)it.sg[SEG_N];
  it.s = it.sg[SEG_S] < (int64_t)it.n ? (int)it.sg[SEG_S] : it.n;
  it.all = it.s == it.n;
  const int64_t start = (int64_t)it.slice * slice_rows;      // < n
  it.start = (int)start;
  it.len = (int)((int64_t)it.n - start < slice_rows ? it.n - start
                                                    : slice_rows);
  return it;
}

// Sum of v over the block (wsum: NWAVES ints of LDS, free on return).
template <int NWAVES>
DEV_INLINE int block_sum(int v, int* wsum) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int i = 0; i < NWAVES; ++i) t += wsum[i];
  __syncthreads();
  return t;
}

// State of the item's segment before level `level` (level == N_LEVEL: the
// final one): the stored state of the level before, advanced through that
// level's finished histogram unless it is done. Every block of a segment
// computes the same value; the block of slice 0 stores it for the next
// launch. wsum: NW ints, piv: 3 ints of LDS.
DEV_INLINE SelState state_before(const Item& it, int level, int cap,
                                 const Scratch& sc, int* wsum, int* piv) {
  const int tid = threadIdx.x;
  SelState st;
  if (level == 0) {
    st.prefix = 0;
    st.shift = KEY_BITS;
    st.rank = it.s;
    st.in_bin = it.n;
    st.done = it.n <= cap;
  } else {
    st = sc.st[(int64_t)it.seg * N_STATE + level - 1];
    if (!st.done) {
      const uint4* h = reinterpret_cast<const uint4*>(
          sc.hist + ((int64_t)it.seg * N_LEVEL + level - 1) * NBIN);
      const uint4 a = h[2 * tid], b = h[2 * tid + 1];
      const int hb[BPT] = {(int)a.x, (int)a.y, (int)a.z, (int)a.w,
                           (int)b.x, (int)b.y, (int)b.z, (int)b.w};
      int sum = 0;
#pragma unroll
      for (int j = 0; j < BPT; ++j) sum += hb[j];
      if (tid == 0) piv[0] = piv[1] = piv[2] = 0;
      int below = block_excl_scan<NW>(sum, wsum);
#pragma unroll
      for (int j = 0; j < BPT; ++j) {      // true for one bin of one thread
        if (below < st.rank && st.rank <= below + hb[j]) {
          piv[0] = BPT * tid + j; piv[1] = below; piv[2] = hb[j];
        }
        below += hb[j];
      }
      __syncthreads();
      const int bits = st.shift < RADIX_BITS ? st.shift : RADIX_BITS;
      st.prefix = (st.prefix << bits) | (uint64_t)piv[0];
      st.shift -= bits;
      st.rank -= piv[1];
      st.in_bin = piv[2];
      st.done = st.in_bin <= cap || st.shift == 0;
    }
  }
  if (it.slice == 0 && tid == 0)
    sc.st[(int64_t)it.seg * N_STATE + level] = st;
  return st;
}

// ---------------------------------------------------------------- kernels
template <class KeySrc>
__global__ void __launch_bounds__(TPB)
bns_sliced_level_kernel(const int64_t* __restrict__ ssegs,
                        const int32_t* __restrict__ items, int slice_rows,
                        int level, int cap, KeySrc ks, Scratch sc) {
  __shared__ uint32_t hist[NBIN];
  __shared__ int wsum[NW];
  __shared__ int piv[3];
  const Item it = load_item(ssegs, items, slice_rows);
  if (it.all) return;
  const SelState st = state_before(it, level, cap, sc, wsum, piv);
  if (st.done) return;
  const int tid = threadIdx.x;
  for (int b = tid; b < NBIN; b += TPB) hist[b] = 0;
  __syncthreads();
  const int hi = st.shift;
  const int bits = hi < RADIX_BITS ? hi : RADIX_BITS;
  const int lo = hi - bits;
  const int64_t word = it.sg[SEG_KEY];
  for (int off = tid; off < it.len; off += TPB) {
    const uint64_t key = ks(word, it.start + off);
    if ((key >> hi) == st.prefix)
      atomicAdd(&hist[(uint32_t)(key >> lo) & ((1u << bits) - 1u)], 1u);
  }
  __syncthreads();
  uint32_t* g = sc.hist + ((int64_t)it.seg * N_LEVEL + level) * NBIN;
  for (int b = tid; b < NBIN; b += TPB) {
    const uint32_t h = hist[b];
    if (h) atomicAdd(&g[b], h);
  }
}

template <class KeySrc>
__global__ void __launch_bounds__(TPB)
bns_sliced_collect_kernel(const int64_t* __restrict__ ssegs,
                          const int32_t* __restrict__ items, int slice_rows,
                          int cap, KeySrc ks, Scratch sc) {
  __shared__ int wsum[NW];
  __shared__ int piv[3];
  const Item it = load_item(ssegs, items, slice_rows);
  if (it.all) return;
  const SelState st = state_before(it, N_LEVEL, cap, sc, wsum, piv);
  const bool keep = st.in_bin <= cap;
  const int64_t word = it.sg[SEG_KEY];
  uint64_t* ckey = sc.cand_key + (int64_t)it.seg * cap;
  int32_t* cpos = sc.cand_pos + (int64_t)it.seg * cap;
  int m = 0;
  for (int off = threadIdx.x; off < it.len; off += TPB) {
    const int i = it.start + off;
    const uint64_t key = ks(word, i);
    if ((key >> st.shift) != st.prefix) continue;
    ++m;
    if (keep) {
      const int slot = atomicAdd(&sc.n_cand[it.seg], 1);
      if (slot < cap) { ckey[slot] = key; cpos[slot] = i; }
    }
  }
  m = block_sum<NW>(m, wsum);
  if (threadIdx.x == 0) sc.match[blockIdx.x] = m;
}

template <class KeySrc, int CAP>
__global__ void __launch_bounds__(THR_TPB)
bns_sliced_threshold_kernel(const int64_t* __restrict__ ssegs,
                            int slice_rows, KeySrc ks, Scratch sc) {
  constexpr int PER = (CAP + THR_TPB - 1) / THR_TPB;   // candidates per thread
  __shared__ uint64_t cand_key[CAP];
  __shared__ int32_t cand_pos[CAP];
  __shared__ int wbuf[2][THR_NW];
  __shared__ int loc[3];               // slice, rank inside it, running sum
  const int seg = blockIdx.x, tid = threadIdx.x;
  const int64_t* sg = ssegs + (int64_t)seg * SSEG_COLS;
  const int n = (int)sg[SEG_N];
  if (sg[SEG_S] >= (int64_t)n) return;
  const SelState st = sc.st[(int64_t)seg * N_STATE + N_LEVEL];
  if (tid == 0) { sc.thr_key[seg] = 0; sc.thr_pos[seg] = -1; loc[0] = 0; loc[1] = 0; }
  __syncthreads();

  if (st.in_bin <= CAP) {
    // each thread keeps its candidates in registers and walks all of them
    // once; the one with rank - 1 below it in (key, position) order is (T, P)
    const int m = sc.n_cand[seg] < CAP ? sc.n_cand[seg] : CAP;
    for (int c = tid; c < m; c += THR_TPB) {
      cand_key[c] = sc.cand_key[(int64_t)seg * CAP + c];
      cand_pos[c] = sc.cand_pos[(int64_t)seg * CAP + c];
    }
    __syncthreads();
    uint64_t kc[PER];
    int pc[PER], below[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int c = tid + r * THR_TPB;
      kc[r] = c < m ? cand_key[c] : 0;
      pc[r] = c < m ? cand_pos[c] : 0;
      below[r] = 0;
    }
    for (int j = 0; j < m; ++j) {
      const uint64_t kj = cand_key[j];
      const int pj = cand_pos[j];
#pragma unroll
      for (int r = 0; r < PER; ++r)
        below[r] += (kj < kc[r]) || (kj == kc[r] && pj < pc[r]);
    }
#pragma unroll
    for (int r = 0; r < PER; ++r)
      if (tid + r * THR_TPB < m && below[r] == st.rank - 1) {
        sc.thr_key[seg] = kc[r]; sc.thr_pos[seg] = pc[r];
      }
    return;
  }

  // all 63 bits fixed and more than CAP keys equal prefix: the slice that
  // holds the rank-th of them, from the running sum of match[] ...
  const int32_t* match = sc.match + sg[SSEG_ITEM0];
  const int n_slice = (int)(((int64_t)n + slice_rows - 1) / slice_rows);
  int run = 0;
  for (int j0 = 0; j0 < n_slice; j0 += THR_TPB) {
    const int j = j0 + tid;
    const int v = j < n_slice ? match[j] : 0;
    const int ex = run + block_excl_scan<THR_NW>(v, wbuf[0]);
    if (ex < st.rank && st.rank <= ex + v) { loc[0] = j; loc[1] = st.rank - ex; }
    if (tid == THR_TPB - 1) loc[2] = ex + v;
    __syncthreads();
    run = loc[2];
  }
  // ... and P, the position of the rank-th equal key, by a ballot walk of
  // that slice which stops there
  const int start = (int)((int64_t)loc[0] * slice_rows), want = loc[1];
  const int len = n - start < slice_rows ? n - start : slice_rows;
  const int64_t word = sg[SEG_KEY];
  int seen = 0, par = 0;
  for (int o0 = 0; o0 < len && seen < want; o0 += THR_TPB) {
    const int off = o0 + tid;
    const bool eq = off < len && ks(word, start + off) == st.prefix;
    int tot;
    const int k = seen + chunk_rank<THR_NW>(eq, wbuf[par], tot);
    par ^= 1;
    if (eq && k == want - 1) {
      sc.thr_key[seg] = st.prefix; sc.thr_pos[seg] = start + off;
    }
    seen += tot;
  }
}

template <class KeySrc>
__global__ void __launch_bounds__(TPB)
bns_sliced_count_kernel(const int64_t* __restrict__ ssegs,
                        const int32_t* __restrict__ items, int slice_rows,
                        KeySrc ks, Scratch sc) {
  __shared__ int wsum[NW];
  const Item it = load_item(ssegs, items, slice_rows);
  if (it.all) return;
  const uint64_t T = sc.thr_key[it.seg];
  const int P = sc.thr_pos[it.seg];
  const int64_t word = it.sg[SEG_KEY];
  int c = 0;
  for (int off = threadIdx.x; off < it.len; off += TPB) {
    const int i = it.start + off;
    const uint64_t key = ks(word, i);
    c += key < T || (key == T && i <= P);
  }
  c = block_sum<NW>(c, wsum);
  if (threadIdx.x == 0) sc.cnt[blockIdx.x] = c;
}

template <class KeySrc>
__global__ void __launch_bounds__(TPB)
bns_sliced_emit_kernel(const int64_t* __restrict__ ssegs,
                       const int32_t* __restrict__ items, int slice_rows,
                       KeySrc ks, Scratch sc, SelectOut o) {
  __shared__ int wbuf[2][NW];
  const Item it = load_item(ssegs, items, slice_rows);
  const int tid = threadIdx.x;
  uint64_t T = 0;
  int P = -1, run = it.start;
  if (!it.all) {
    // output base: the selected rows of the earlier slices of the segment
    const int32_t* cnt = sc.cnt + ((int64_t)blockIdx.x - it.slice);
    int c = 0;
    for (int j = tid; j < it.slice; j += TPB) c += cnt[j];
    run = block_sum<NW>(c, wbuf[0]);
    T = sc.thr_key[it.seg];
    P = sc.thr_pos[it.seg];
  }
  const int64_t word = it.sg[SEG_KEY], kind = it.sg[SEG_KIND];
  const int64_t base = it.sg[SEG_BASE], out = it.sg[SEG_OUT];
  int par = 0;
  for (int o0 = 0; o0 < it.len && run < it.s; o0 += TPB) {
    const int off = o0 + tid, i = it.start + off;
    bool sel = off < it.len;
    if (sel && !it.all) {
      const uint64_t key = ks(word, i);
      sel = key < T || (key == T && i <= P);
    }
    int tot;
    const int k = run + chunk_rank<NW>(sel, wbuf[par], tot);
    par ^= 1;
    if (sel && k < it.s) o.emit(kind, out + k, base + i);
    run += tot;
  }
}

}  // namespace

// ------------------------------------------------------------------- host
namespace bns {

template <class KeySrc>
void launch_select_sliced(int64_t cap, const at::Tensor& ssegs,
                          const at::Tensor& items, int64_t slice_rows,
                          const KeySrc& ks, const SelectOut& o) {
  const int64_t n_sseg = ssegs.size(0), n_item = items.size(0);
  if (n_sseg == 0) return;
  TORCH_CHECK(cap == CAP_DEFAULT || cap == 64,
              "bns_select: cap must be ", CAP_DEFAULT, " or 64");
  TORCH_CHECK(n_item < (1ll << 31), "bns_select: too many slices");
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const auto iopt = ssegs.options().dtype(at::kInt);
  at::Tensor zeroed = at::zeros({n_sseg * (N_LEVEL * NBIN + 1)}, iopt);
  at::Tensor b64 = at::empty({n_sseg * (N_STATE * 3 + cap + 1)},
                             ssegs.options());
  at::Tensor b32 = at::empty({n_sseg * (cap + 1) + 2 * n_item}, iopt);
  Scratch sc;
  sc.hist = reinterpret_cast<uint32_t*>(zeroed.data_ptr<int32_t>());
  sc.n_cand = zeroed.data_ptr<int32_t>() + n_sseg * N_LEVEL * NBIN;
  int64_t* p64 = b64.data_ptr<int64_t>();
  sc.st = reinterpret_cast<SelState*>(p64);
  sc.cand_key = reinterpret_cast<uint64_t*>(p64 + n_sseg * N_STATE * 3);
  sc.thr_key = sc.cand_key + n_sseg * cap;
  sc.cand_pos = b32.data_ptr<int32_t>();
  sc.thr_pos = sc.cand_pos + n_sseg * cap;
  sc.match = sc.thr_pos + n_sseg;
  sc.cnt = sc.match + n_item;

  const int64_t* sp = ssegs.data_ptr<int64_t>();
  const int32_t* ip = items.data_ptr<int32_t>();
  const int sr = (int)slice_rows, cp = (int)cap;
  const dim3 grid((unsigned)n_item), block(TPB);
  const dim3 tgrid((unsigned)n_sseg), tblock(THR_TPB);
  for (int level = 0; level < N_LEVEL; ++level)
    hipLaunchKernelGGL((bns_sliced_level_kernel<KeySrc>), grid, block, 0,
                       stream, sp, ip, sr, level, cp, ks, sc);
  hipLaunchKernelGGL((bns_sliced_collect_kernel<KeySrc>), grid, block, 0,
                     stream, sp, ip, sr, cp, ks, sc);
  if (cap == CAP_DEFAULT)
    hipLaunchKernelGGL(
        (bns_sliced_threshold_kernel<KeySrc, (int)CAP_DEFAULT>), tgrid,
        tblock, 0, stream, sp, sr, ks, sc);
  else
    hipLaunchKernelGGL((bns_sliced_threshold_kernel<KeySrc, 64>), tgrid,
                       tblock, 0, stream, sp, sr, ks, sc);
  hipLaunchKernelGGL((bns_sliced_count_kernel<KeySrc>), grid, block, 0,
                     stream, sp, ip, sr, ks, sc);
  hipLaunchKernelGGL((bns_sliced_emit_kernel<KeySrc>), grid, block, 0,
                     stream, sp, ip, sr, ks, sc, o);
}

template void launch_select_sliced<PhiloxKeys>(
    int64_t, const at::Tensor&, const at::Tensor&, int64_t,
    const PhiloxKeys&, const SelectOut&);
template void launch_select_sliced<RawKeys>(
    int64_t, const at::Tensor&, const at::Tensor&, int64_t, const RawKeys&,
    const SelectOut&);

}  // namespace bns
