// The depth-U gather stream shared by the gather kernels of kernels.hip
// (wide SpMM, bf16 GAT kernels) and gatv2.hip: the per-chunk window of row
// reads (gather_chunk) and the item loop of the per-edge GAT kernels
// (stream_edge_items). The schedule is described at "depth-U gather stream"
// in kernels.hip.
#pragma once
#include "common.h"

DEV_INLINE float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

DEV_INLINE float readlane_f(float v, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

// Entries of [e0, end) in one chunk: at most 64, 0 for an empty range.
// Wave-uniform, and pinned to a scalar register: every branch on it is a
// scalar branch.
DEV_INLINE int chunk_count(int64_t e0, int64_t end) {
  const int64_t left = end - e0;
  return __builtin_amdgcn_readfirstlane(
      left < WAVE ? (left > 0 ? (int)left : 0) : WAVE);
}

// Entries 0 .. nv - 1 of one chunk, in order: accumulate(k, val) gets the
// NV registers of type R (common.h RowLoad: float4, or 8 / 4 packed bf16)
// of entry k's source row, whose length is f4 in units of R.
// behind_first() runs once, after the opening U reads have been issued.
template <int U, int NV, typename R = float4, typename T, typename Acc,
          typename Hook>
DEV_INLINE void gather_chunk(const T* __restrict__ x, int cid, int nv, int f4,
                             const int (&fi)[NV], Acc&& accumulate,
                             Hook&& behind_first) {
  R val[U][NV];
  auto read = [&](int k, R (&v)[NV]) __attribute__((always_inline)) {
    const int64_t base = (int64_t)__builtin_amdgcn_readlane(cid, k) * f4;
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = RowLoad<R>::at(x, base + fi[q]);
  };
  // One unconditional use of cid ahead of the branches below: its load is
  // then waited for here, once. Left to the first read inside a branch,
  // the wait is repeated in each of them as "everything outstanding", and
  // the U opening reads go out one latency apart.
  asm volatile("" ::"s"(__builtin_amdgcn_readlane(cid, 0)));
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (u < nv) read(u, val[u]);
  behind_first();
  int k = 0;
  for (; k + 2 * U <= nv; k += U) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      accumulate(k + u, val[u]);
      read(k + u + U, val[u]);
      // keeps each read next to its accumulate: without it all U reads
      // sink below the last accumulate of the window
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // Fewer than 2 U entries left, the first U of them already read. The
  // rest is read only after those are accumulated: reads issued between
  // conditional accumulates would each be waited for on their own. The
  // explicit s_waitcnt vmcnt(0) (every outstanding read is one the next
  // loop needs) is there for the same reason: placed by the compiler
  // inside the first branch, it would not count for the paths around it.
  __builtin_amdgcn_s_waitcnt(0x0f70);
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (k + u < nv) accumulate(k + u, val[u]);
  k += U;
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (k + u < nv) read(k + u, val[u]);
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (k + u < nv) accumulate(k + u, val[u]);
}

// What lane l holds of edge e0 + l of a chunk: column id, the index of its
// weights (wperm ? wperm[e] : e) and, for H <= 4, the H weights themselves.
struct EdgeChunk {
  int cid;
  int64_t we;
  float w[4];
};

template <bool WEIGHTS>
DEV_INLINE EdgeChunk load_edge_ids(const int32_t* __restrict__ indices,
                                   const int64_t* __restrict__ wperm,
                                   int64_t e0, int nv, int lane) {
  EdgeChunk c = {0, 0, {0.f, 0.f, 0.f, 0.f}};
  if (lane < nv) {
    c.cid = indices[e0 + lane];
    if constexpr (WEIGHTS) c.we = wperm ? wperm[e0 + lane] : e0 + lane;
  }
  return c;
}

// The chunk's one dependent load (through wperm in the backward): one
// float4 per lane when H == 4 and w is 16-byte aligned (w_vec4).
DEV_INLINE void load_edge_w(EdgeChunk& c, int nv, const float* __restrict__ w,
                            int H, bool w_vec4, int lane) {
  if (H > 4 || lane >= nv) return;
  if (w_vec4) {
    const float4 t = *reinterpret_cast<const float4*>(w + c.we * 4);
    c.w[0] = t.x; c.w[1] = t.y; c.w[2] = t.z; c.w[3] = t.w;
  } else {
#pragma unroll
    for (int h = 0; h < 4; ++h)
      if (h < H) c.w[h] = w[c.we * H + h];
  }
}

// stream_items for the edge kernels: the calling wave's items, each in
// passes of NS * 64 slots of a row of S slots of register type R, on the
// same schedule — window of U row reads, the next chunk's ids (and this
// chunk's weights, WEIGHTS) loaded behind the chunk's first U reads, the
// next item fetched during the last chunk. init(row, si, has) starts a
// pass, accumulate(k, val, chunk, e0) takes entry k (edge e0 + k),
// store(row, atomic, si, has) ends it. A lane past the row's end reads the
// row's last slot instead (in bounds) and has[] is false for it. T is the
// source element type (bf16_t, or float with R = float4).
template <int U, int NS, typename R, bool WEIGHTS, typename T, typename Init,
          typename Acc, typename Store>
DEV_INLINE void stream_edge_items(const WorkList& wl,
                                  const int32_t* __restrict__ indices,
                                  const float* __restrict__ w,
                                  const int64_t* __restrict__ wperm,
                                  const T* __restrict__ x, int H,
                                  bool w_vec4, int S, Init&& init,
                                  Acc&& accumulate, Store&& store) {
  const WaveItems wi = wave_items<WAVE>(wl);
  const int lane = wi.lane;
  const int it_beg = __builtin_amdgcn_readfirstlane(wi.beg);
  const int it_end = __builtin_amdgcn_readfirstlane(wi.end);
  if (it_beg >= it_end) return;

  int row = wl.row[it_beg];
  int64_t beg = wl.beg[it_beg], end = wl.end[it_beg];
  int nxt_nv = chunk_count(beg, end);
  EdgeChunk nxt = load_edge_ids<WEIGHTS>(indices, wperm, beg, nxt_nv, lane);
  for (int it = it_beg; it < it_end; ++it) {
    const bool has_next = it + 1 < it_end;
    int n_row = 0;
    int64_t n_beg = 0, n_end = 0;
    if (has_next) {
      n_row = wl.row[it + 1];
      n_beg = wl.beg[it + 1];
      n_end = wl.end[it + 1];
    }
    const bool atomic = row < 0;
    const int r = atomic ? ~row : row;
    for (int s0 = 0; s0 < S; s0 += NS * WAVE) {
      const bool last_pass = s0 + NS * WAVE >= S;
      int si[NS];
      bool has[NS];
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        si[j] = s0 + j * WAVE + lane;
        has[j] = si[j] < S;
        if (!has[j]) si[j] = S - 1;
      }
      if (s0 > 0) {                          // a further pass re-walks the item
        nxt_nv = chunk_count(beg, end);
        nxt = load_edge_ids<WEIGHTS>(indices, wperm, beg, nxt_nv, lane);
      }
      init(r, si, has);
      int64_t e0 = beg;
      do {
        EdgeChunk cur = nxt;
        const int cur_nv = nxt_nv;
        const int64_t e1 = e0 + WAVE;
        const bool more = e1 < end;
        const int64_t p0 = more ? e1 : n_beg;
        nxt_nv = more ? chunk_count(e1, end)
                      : (last_pass && has_next ? chunk_count(n_beg, n_end) : 0);
        gather_chunk<U, NS, R>(
            x, cur.cid, cur_nv, S, si,
            [&](int k, const R (&val)[NS]) __attribute__((always_inline)) {
              accumulate(k, val, cur, e0);
            },
            [&]() __attribute__((always_inline)) {
              if constexpr (WEIGHTS) load_edge_w(cur, cur_nv, w, H, w_vec4, lane);
              nxt = load_edge_ids<WEIGHTS>(indices, wperm, p0, nxt_nv, lane);
            });
        e0 = e1;
      } while (e0 < end);
      store(r, atomic, si, has);
    }
    row = n_row; beg = n_beg; end = n_end;
  }
}
