// Device code and launch entries shared by the two forms of the boundary
// selection: one workgroup per segment (bns_select.hip) and (segment, slice)
// workgroups over separate launches (bns_select_sliced.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <ATen/ATen.h>
#include "common.h"

namespace bns {

constexpr int RADIX_BITS = 11;
constexpr int NBIN = 1 << RADIX_BITS;          // 2048
constexpr int KEY_BITS = 63;
constexpr uint64_t KEY_MASK = 0x7FFFFFFFFFFFFFFFull;
constexpr int64_t CAP_DEFAULT = 4096;
constexpr int SLICE_TPB = 256;                 // block of the sliced kernels

// Segment table: int64 [n_seg, SEG_COLS], one row per segment. The table of
// the sliced form has one more column: the segment's first work item.
enum { SEG_N, SEG_S, SEG_OUT, SEG_KEY, SEG_KIND, SEG_BASE, SEG_COLS };
enum { SSEG_ITEM0 = SEG_COLS, SSEG_COLS };
enum { KIND_PACK = 0, KIND_HALO = 1 };

// ------------------------------------------------------------ key sources
// key(word, i): the 63-bit key of position i of a segment whose SEG_KEY
// column is `word`.
struct PhiloxKeys {           // word = src_rank << 16 | dst_rank
  uint32_t seed_lo, seed_hi, epoch;
  DEV_INLINE uint64_t operator()(int64_t word, int i) const {
    const P4 r = philox4x32((uint32_t)i, epoch, (uint32_t)word, 0x424E5347u,
                            seed_lo, seed_hi);
    return (((uint64_t)r.c0 << 32) | r.c1) & KEY_MASK;
  }
};

struct RawKeys {              // word = offset of the segment in `keys`
  const int64_t* __restrict__ keys;
  DEV_INLINE uint64_t operator()(int64_t word, int i) const {
    return (uint64_t)keys[word + i] & KEY_MASK;
  }
};

struct SelectOut {
  const int64_t* __restrict__ gather;     // boundary_cat, or null
  const float* __restrict__ norm_full;    // per halo row, or null
  const float* __restrict__ deg_full;
  int64_t* __restrict__ pack;             // KIND_PACK values
  int64_t* __restrict__ hsel;             // KIND_HALO values
  float* __restrict__ norm;               // norm_full[hsel]
  float* __restrict__ deg;                // deg_full[hsel]

  // Row v = base + i of a segment as element `at` of its output, final value.
  DEV_INLINE void emit(int64_t kind, int64_t at, int64_t v) const {
    if (kind == KIND_PACK) {
      pack[at] = gather ? gather[v] : v;
    } else {
      hsel[at] = v;
      if (norm_full) {
        norm[at] = norm_full[v];
        deg[at] = deg_full[v];
      }
    }
  }
};

// ------------------------------------------------------------ block steps
// Exclusive prefix of v over the NW * 64 threads of the block (wsum: NW ints
// of LDS, free again on return).
template <int NW>
DEV_INLINE int block_excl_scan(int v, int* wsum) {
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  int incl = v;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const int u = __shfl_up(incl, d, WAVE);
    if (lane >= d) incl += u;
  }
  if (lane == WAVE - 1) wsum[w] = incl;
  __syncthreads();
  int off = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i)
    if (i < w) off += wsum[i];
  __syncthreads();
  return off + incl - v;
}

// Rank of the calling thread among the threads of the block with f set, in
// thread order, and their number. wtot: NW ints of LDS; consecutive calls
// alternate between two such buffers, so that one barrier per call is
// enough (a buffer is written again only two barriers later).
template <int NW>
DEV_INLINE int chunk_rank(bool f, int* wtot, int& total) {
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const uint64_t b = __ballot(f);
  if (lane == 0) wtot[w] = __popcll(b);
  __syncthreads();
  int off = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int t = wtot[i];
    if (i < w) off += t;
    total += t;
  }
  return off + __popcll(b & ((1ull << lane) - 1ull));
}

// ------------------------------------------------- bns_select_sliced.hip
// The sliced form over `ssegs` ([n_sseg, SSEG_COLS] int64) and its work
// items ([n_item, 2] int32 of (segment, slice), slices of slice_rows
// positions): a fixed sequence of launches on the current stream, scratch
// allocated here. Instantiated for PhiloxKeys and RawKeys.
template <class KeySrc>
void launch_select_sliced(int64_t cap, const at::Tensor& ssegs,
                          const at::Tensor& items, int64_t slice_rows,
                          const KeySrc& ks, const SelectOut& o);

}  // namespace bns
