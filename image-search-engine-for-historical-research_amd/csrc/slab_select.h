// Selection in LDS on entries (order-preserving key, id), shared by the inverted file over raw rows (ivfflat.hip) and the Minkowski
// scan (minkowski.hip): the entry order, the bitonic sort, the best HALF entries of a stream and the emit of the first k.  Both
// give an answer the same order: (key asc, id asc), the sentinel (~0, -1) behind every row.  DESIGN.md 5.18, 5.19.
#pragma once
#include "common.h"
#include "f64_key.h"

namespace mi {

constexpr uint64_t SLAB_NOKEY = ~0ull;

// (key, id) ascending, id -1 behind every row: the order of refine_sort_kernel
__device__ __forceinline__ bool slab_after(uint64_t ka, int64_t ia, uint64_t kb, int64_t ib) {
  return ka != kb ? ka > kb : (uint64_t)ia > (uint64_t)ib;
}

// bitonic sort of N entries (a power of two) in LDS by NT threads; ends behind a barrier
template <int N, int NT>
__device__ __forceinline__ void slab_sort(uint64_t* s_key, int64_t* s_id, int tid) {
  for (uint32_t size = 2; size <= (uint32_t)N; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t p = tid; p < (uint32_t)N / 2; p += NT) {
        const uint32_t lo = 2 * p - (p & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint64_t ka = s_key[lo], kb = s_key[hi];
        const int64_t ia = s_id[lo], ib = s_id[hi];
        if (slab_after(ka, ia, kb, ib) == up) {
          s_key[lo] = kb;
          s_key[hi] = ka;
          s_id[lo] = ib;
          s_id[hi] = ia;
        }
      }
      __syncthreads();
    }
}

// The best HALF entries, in order, of a stream of `count` entries: s_key / s_id hold 2 HALF entries, [0, HALF) the best so far
// (sorted after every pass), [HALF, 2 HALF) the next HALF entries of the stream.  fetch(i, key, id) fills entry i of the stream and
// leaves the sentinel where the entry does not count.  Every thread of the workgroup calls it; ends behind a barrier
template <int HALF, int NT, typename Fetch>
__device__ __forceinline__ void slab_stream_best(uint64_t* s_key, int64_t* s_id, int64_t count, int tid, Fetch fetch) {
  for (int i = tid; i < HALF; i += NT) {
    s_key[i] = SLAB_NOKEY;
    s_id[i] = -1;
  }
  for (int64_t c0 = 0; c0 < count; c0 += HALF) {
    for (int i = tid; i < HALF; i += NT) {
      uint64_t key = SLAB_NOKEY;
      int64_t id = -1;
      if (c0 + i < count) fetch(c0 + i, key, id);
      s_key[HALF + i] = key;
      s_id[HALF + i] = id;
    }
    __syncthreads();
    slab_sort<2 * HALF, NT>(s_key, s_id, tid);
  }
  __syncthreads();
}

// the first k entries of a sorted list -> row q of the answer: ids (row_offset + id; -1 for the sentinel) and values.  ASC: the keys
// are those of the values, the padding +inf; otherwise those of 0.0 - value (best = largest), the padding -inf
template <bool ASC, int NT>
__device__ __forceinline__ void slab_emit(const uint64_t* s_key, const int64_t* s_id, int32_t k, int64_t q, int64_t row_offset,
                                          int64_t* __restrict__ out_idx, float* __restrict__ out_val, double* __restrict__ out_val64,
                                          int tid) {
  const double padv = ASC ? (double)INFINITY : -(double)INFINITY;
  for (int32_t i = tid; i < k; i += NT) {
    const int64_t id = s_id[i];
    const double dec = f64_key_value(s_key[i]);
    const double v = id < 0 ? padv : (ASC ? dec : 0.0 - dec);
    if (out_idx) out_idx[q * k + i] = id < 0 ? -1 : row_offset + id;
    if (out_val64) out_val64[q * k + i] = v;
    if (out_val) out_val[q * k + i] = (float)v;
  }
}

}  // namespace mi
