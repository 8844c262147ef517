// Per-epoch boundary-node selection: "the s smallest of n keys, positions
// ascending" for every (peer, direction) segment of a plan build in ONE
// launch, bit-identical to sort(argsort(keys, stable)[:s]) — the two full
// radix sorts of HaloPlan._sample (parallel/plan.py) become a selection and
// an ordered compaction.
//
// One workgroup of 1024 threads owns one segment and never talks to
// another. Keys are not stored: the production key is a pure function of
// (seed, epoch, src<<16|dst, i) (philox4x32, common.h) and is recomputed in
// every pass; the raw form reads a caller's int64 keys instead (KeySrc).
//
//  1. Radix descent. An LDS histogram (LDS atomics) of the next 11 key bits
//     of the keys that match the prefix chosen so far; a block scan of the
//     2048 bins gives the pivot bin, the keys below it and the rank wanted
//     inside it. 63 bits = 5 levels of 11 bits and one of 8. The descent
//     stops as soon as the pivot bin holds <= CAP keys — after ONE level
//     for Philox keys up to n ~ 2048 * CAP.
//  2. Candidates. The keys of the pivot bin go to LDS as (key, position).
//  3. Threshold. Every candidate counts the candidates below it in the
//     order (key, position); the one with rank - 1 below it is the
//     threshold pair (T, P). Pairs are distinct, so
//     selected <=> (key, i) <= (T, P) is exact and IS the tie rule of the
//     stable argsort (equal keys: lower position first).
//     If all 63 bits are fixed and more than CAP keys remain, they are all
//     equal to T: P is the position of the rank-th of them in index order,
//     found by a ballot walk that stops there.
//  4. Ordered emit. The segment is walked in chunks of 1024 in index
//     order: wave ballot + popcount, wave totals through LDS, a running
//     base across chunks. Element i of rank k is stored at out_off + k as
//     its FINAL value — boundary_cat[base + i] (send: pack_idx) or base + i
//     (receive: hsel, with the two per-row floats gathered by the same
//     thread). The walk ends once s elements are out.
//
// s >= n selects everything (steps 1-3 skipped); segments with s <= 0 or
// n <= 0 write nothing. No global scratch, no read-back, no inter-block
// dependency. LDS: 8 KB histogram + 12 B per candidate = 56 KB + for
// CAP = 4096.
//
// One workgroup is serial in n: the caller gives large segments to the
// sliced form (bns_select_sliced.hip) in the same call, through a second
// table; the device code both share is in bns_select_dev.h.
//
// Preconditions (checked by ops/bns_select.py, which builds the table, not
// on the device): n < 2^31; the outputs hold out_off + min(s, n) elements;
// base + n is within boundary_cat / the per-row arrays; raw keys lie in
// [0, 2^63) (bit 63 is ignored).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>
#include <c10/util/Optional.h>
#include <vector>
#include "common.h"
#include "bns_select.h"
#include "bns_select_dev.h"

namespace {

using namespace bns;

constexpr int TPB = 1024;
constexpr int NWAVE = TPB / WAVE;              // 16
static_assert(NBIN == 2 * TPB, "pivot search owns two bins per thread");

// ----------------------------------------------------------------- kernel
template <class KeySrc, int CAP>
__global__ void __launch_bounds__(TPB)
bns_select_kernel(const int64_t* __restrict__ segs, KeySrc ks, SelectOut o) {
  __shared__ uint32_t hist[NBIN];
  __shared__ uint64_t cand_key[CAP];
  __shared__ int32_t cand_pos[CAP];
  __shared__ int wbuf[2][NWAVE];
  __shared__ int piv[3];               // pivot bin, keys below it, keys in it
  __shared__ int n_cand;
  __shared__ uint64_t thr_key;
  __shared__ int thr_pos;

  const int64_t* sg = segs + (int64_t)blockIdx.x * SEG_COLS;
  const int n = (int)sg[SEG_N];
  const int cnt = sg[SEG_S] < (int64_t)n ? (int)sg[SEG_S] : n;
  if (cnt <= 0) return;
  const int64_t word = sg[SEG_KEY];
  const int tid = threadIdx.x;
  const bool all = cnt == n;
  uint64_t T = 0;
  int P = -1, par = 0;

  if (!all) {
    if (tid == 0) { thr_key = 0; thr_pos = -1; }
    // 1. radix descent: prefix = the bits above `shift` of the cnt-th key
    uint64_t prefix = 0;
    int rank = cnt, shift = KEY_BITS, in_bin = n;
    while (shift > 0) {
      const int hi = shift;
      const int bits = shift < RADIX_BITS ? shift : RADIX_BITS;
      shift -= bits;
      for (int b = tid; b < NBIN; b += TPB) hist[b] = 0;
      __syncthreads();       // also: every thread has read the last pivot
      if (tid == 0) piv[0] = piv[1] = piv[2] = 0;
      for (int i = tid; i < n; i += TPB) {
        const uint64_t key = ks(word, i);
        if ((key >> hi) == prefix)
          atomicAdd(&hist[(uint32_t)(key >> shift) & ((1u << bits) - 1u)], 1u);
      }
      __syncthreads();
      const int h0 = (int)hist[2 * tid], h1 = (int)hist[2 * tid + 1];
      const int below = block_excl_scan<NWAVE>(h0 + h1, wbuf[0]);
      if (below < rank && rank <= below + h0) {
        piv[0] = 2 * tid; piv[1] = below; piv[2] = h0;
      } else if (below + h0 < rank && rank <= below + h0 + h1) {
        piv[0] = 2 * tid + 1; piv[1] = below + h0; piv[2] = h1;
      }
      __syncthreads();
      prefix = (prefix << bits) | (uint64_t)piv[0];
      rank -= piv[1];
      in_bin = piv[2];
      if (in_bin <= CAP) break;
    }
    if (in_bin <= CAP) {
      // 2. candidates: the keys whose bits above `shift` equal prefix
      if (tid == 0) n_cand = 0;
      __syncthreads();
      for (int i = tid; i < n; i += TPB) {
        const uint64_t key = ks(word, i);
        if ((key >> shift) == prefix) {
          const int slot = atomicAdd(&n_cand, 1);
          if (slot < CAP) { cand_key[slot] = key; cand_pos[slot] = i; }
        }
      }
      __syncthreads();
      // 3. threshold: the candidate with rank - 1 candidates below it
      const int m = n_cand < CAP ? n_cand : CAP;
      for (int c = tid; c < m; c += TPB) {
        const uint64_t kc = cand_key[c];
        const int pc = cand_pos[c];
        int below = 0;
        for (int j = 0; j < m; ++j) {
          const uint64_t kj = cand_key[j];
          below += (kj < kc) || (kj == kc && cand_pos[j] < pc);
        }
        if (below == rank - 1) { thr_key = kc; thr_pos = pc; }
      }
    } else {
      // all 63 bits fixed: the in_bin > CAP remaining keys equal prefix;
      // P = position of the rank-th of them in index order
      int seen = 0;
      for (int i0 = 0; i0 < n && seen < rank; i0 += TPB) {
        const int i = i0 + tid;
        const bool eq = i < n && ks(word, i) == prefix;
        int tot;
        const int k = seen + chunk_rank<NWAVE>(eq, wbuf[par], tot);
        par ^= 1;
        if (eq && k == rank - 1) { thr_key = prefix; thr_pos = i; }
        seen += tot;
      }
    }
    __syncthreads();
    T = thr_key;
    P = thr_pos;
  }

  // 4. ordered emit
  const int64_t kind = sg[SEG_KIND], base = sg[SEG_BASE], out = sg[SEG_OUT];
  int run = 0;
  for (int i0 = 0; i0 < n && run < cnt; i0 += TPB) {
    const int i = i0 + tid;
    bool sel = i < n;
    if (sel && !all) {
      const uint64_t key = ks(word, i);
      sel = key < T || (key == T && i <= P);
    }
    int tot;
    const int k = run + chunk_rank<NWAVE>(sel, wbuf[par], tot);
    par ^= 1;
    if (sel && k < cnt) o.emit(kind, out + k, base + i);
    run += tot;
  }
}

// ------------------------------------------------------------------- host
template <class KeySrc>
void launch_select(int64_t cap, const at::Tensor& segs, const KeySrc& ks,
                   const SelectOut& o) {
  const int64_t n_seg = segs.size(0);
  if (n_seg == 0) return;
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const int64_t* sp = segs.data_ptr<int64_t>();
  const dim3 grid((unsigned)n_seg), block(TPB);
  if (cap == CAP_DEFAULT)
    hipLaunchKernelGGL((bns_select_kernel<KeySrc, (int)CAP_DEFAULT>), grid,
                       block, 0, stream, sp, ks, o);
  else if (cap == 64)
    hipLaunchKernelGGL((bns_select_kernel<KeySrc, 64>), grid, block, 0,
                       stream, sp, ks, o);
  else
    TORCH_CHECK(false, "bns_select: cap must be ", CAP_DEFAULT, " or 64");
}

// The two tables of a call: `segs` for the one-workgroup kernel above,
// `ssegs` with its (segment, slice) `items` for the sliced launches
// (bns_select_sliced.hip). Either may be empty.
struct Tables {
  const at::Tensor& segs;
  const at::Tensor& ssegs;
  const at::Tensor& items;
  int64_t slice_rows;

  void check() const {
    TORCH_CHECK(segs.is_cuda() && segs.is_contiguous() && segs.dim() == 2 &&
                segs.size(1) == SEG_COLS && segs.scalar_type() == at::kLong,
                "segs: [n_seg, ", (int)SEG_COLS, "] int64 cuda tensor");
    TORCH_CHECK(ssegs.is_contiguous() && ssegs.dim() == 2 &&
                ssegs.size(1) == SSEG_COLS &&
                ssegs.scalar_type() == at::kLong &&
                ssegs.device() == segs.device(),
                "ssegs: [n_sseg, ", (int)SSEG_COLS, "] int64 tensor on the "
                "device of segs");
    TORCH_CHECK(items.is_contiguous() && items.dim() == 2 &&
                items.size(1) == 2 && items.scalar_type() == at::kInt &&
                items.device() == segs.device() &&
                (items.size(0) > 0) == (ssegs.size(0) > 0),
                "items: [n_item, 2] int32 tensor on the device of segs");
    TORCH_CHECK(slice_rows > 0 && slice_rows % SLICE_TPB == 0 &&
                slice_rows <= (1 << 30),
                "slice_rows: a positive multiple of ", SLICE_TPB);
  }

  template <class KeySrc>
  void launch(int64_t cap, const KeySrc& ks, const SelectOut& o) const {
    launch_select(cap, segs, ks, o);
    launch_select_sliced(cap, ssegs, items, slice_rows, ks, o);
  }
};

const float* float_rows(const c10::optional<at::Tensor>& t, const char* name,
                        const at::Tensor& like) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->dim() == 1 &&
              t->scalar_type() == at::kFloat &&
              t->device() == like.device(), name, ": 1-D float cuda tensor");
  return t->data_ptr<float>();
}

// The plan's entry: (pack_idx [n_pack], hsel [n_hsel], norm_full[hsel],
// deg_full[hsel]); the two float outputs are empty without their sources.
std::vector<at::Tensor> bns_select_philox(
    const at::Tensor& segs, const at::Tensor& ssegs, const at::Tensor& items,
    int64_t slice_rows, int64_t n_pack, int64_t n_hsel,
    const c10::optional<at::Tensor>& boundary_cat,
    const c10::optional<at::Tensor>& norm_full,
    const c10::optional<at::Tensor>& deg_full, int64_t seed, int64_t epoch,
    int64_t cap) {
  const Tables tb{segs, ssegs, items, slice_rows};
  tb.check();
  TORCH_CHECK(n_pack >= 0 && n_hsel >= 0, "bns_select: negative output size");
  TORCH_CHECK(norm_full.has_value() == deg_full.has_value(),
              "bns_select: norm_full and deg_full go together");
  c10::cuda::CUDAGuard guard(segs.device());
  const auto lopt = segs.options();
  const auto fopt = segs.options().dtype(at::kFloat);
  SelectOut o{};
  if (boundary_cat.has_value()) {
    TORCH_CHECK(boundary_cat->is_cuda() && boundary_cat->is_contiguous() &&
                boundary_cat->scalar_type() == at::kLong &&
                boundary_cat->device() == segs.device(),
                "boundary_cat: contiguous int64 cuda tensor");
    o.gather = boundary_cat->data_ptr<int64_t>();
  }
  o.norm_full = float_rows(norm_full, "norm_full", segs);
  o.deg_full = float_rows(deg_full, "deg_full", segs);
  at::Tensor pack = at::empty({n_pack}, lopt);
  at::Tensor hsel = at::empty({n_hsel}, lopt);
  at::Tensor norm = at::empty({o.norm_full ? n_hsel : 0}, fopt);
  at::Tensor deg = at::empty({o.norm_full ? n_hsel : 0}, fopt);
  o.pack = pack.data_ptr<int64_t>();
  o.hsel = hsel.data_ptr<int64_t>();
  o.norm = norm.data_ptr<float>();
  o.deg = deg.data_ptr<float>();
  const uint64_t sd = (uint64_t)seed;
  tb.launch(cap, PhiloxKeys{(uint32_t)(sd & 0xFFFFFFFFull),
                            (uint32_t)(sd >> 32), (uint32_t)epoch}, o);
  return {pack, hsel, norm, deg};
}

// The raw-key utility: positions (segment-local) of the s smallest keys of
// every segment, ascending, concatenated ([n_out] int64).
at::Tensor bns_select_raw(const at::Tensor& keys, const at::Tensor& segs,
                          const at::Tensor& ssegs, const at::Tensor& items,
                          int64_t slice_rows, int64_t n_out, int64_t cap) {
  const Tables tb{segs, ssegs, items, slice_rows};
  tb.check();
  TORCH_CHECK(keys.is_cuda() && keys.is_contiguous() && keys.dim() == 1 &&
              keys.scalar_type() == at::kLong &&
              keys.device() == segs.device(),
              "keys: 1-D int64 cuda tensor on the device of segs");
  TORCH_CHECK(n_out >= 0, "bns_select: negative output size");
  c10::cuda::CUDAGuard guard(segs.device());
  at::Tensor out = at::empty({n_out}, segs.options());
  SelectOut o{};
  o.hsel = out.data_ptr<int64_t>();
  tb.launch(cap, RawKeys{keys.data_ptr<int64_t>()}, o);
  return out;
}

}  // namespace

namespace bns {

void bind_bns_select(pybind11::module& m) {
  namespace py = pybind11;
  m.attr("BNS_SELECT_CAP") = CAP_DEFAULT;
  m.attr("BNS_SELECT_SLICE_MIN") = (int64_t)SLICE_TPB;
  m.def("bns_select_philox", &bns_select_philox,
        "per-epoch BNS selection of every plan segment: `segs` in one "
        "launch, `ssegs` sliced over `items` "
        "(pack_idx, hsel, norm_full[hsel], deg_full[hsel])",
        py::arg("segs"), py::arg("ssegs"), py::arg("items"),
        py::arg("slice_rows"), py::arg("n_pack"), py::arg("n_hsel"),
        py::arg("boundary_cat"), py::arg("norm_full"), py::arg("deg_full"),
        py::arg("seed"), py::arg("epoch"), py::arg("cap") = CAP_DEFAULT);
  m.def("bns_select_raw", &bns_select_raw,
        "positions of the s smallest caller-supplied keys per segment",
        py::arg("keys"), py::arg("segs"), py::arg("ssegs"), py::arg("items"),
        py::arg("slice_rows"), py::arg("n_out"),
        py::arg("cap") = CAP_DEFAULT);
}

}  // namespace bns
