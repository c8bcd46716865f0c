// Exact re-ranking of a shortlist on the stored f32 rows (faiss IndexRefineFlat).
//
// Per query kc candidate ids from any index (global ids, any order, repeats allowed, anything outside the shard = padding) ->
// the best k DISTINCT candidates in the metric of the rows gallery.  Two launches:
//   refine_gather_kernel   grid (slab of candidates, query), one wave per candidate row: the f64 value of every candidate into a
//                          [nq][kc] workspace.  This is the HBM gather (4 * dp bytes per candidate); a query's rows are pulled by
//                          kc / REFINE_SLAB workgroups, not by one.
//   refine_sort_kernel     one workgroup per query: (key, id) pairs in LDS, bitonic sort by (value, id asc), repeats dropped by
//                          comparing neighbours, k rows written, the tail padded.
// L2 gallery: l2_direct_wave, the bits of mi_knn_search_l2, ascending.  Any other gallery: sum_j q_j g_j with the same lane and
// column walk and FMA chain, descending.  No atomics, no grid barrier.
#include "common.h"
#include "kernels.h"
#include "l2_wave.h"

namespace mi {

constexpr int REFINE_SLAB = 8;          // candidates per gather workgroup (4 waves, two rows each)

// qry [nq][dp] (16-byte aligned rows, d columns used), cand [nq][cand_stride], val [nq][kc].  A padding candidate gets no value
// here: the sort kernel decides padding from the id again and never reads its slot.
template <bool L2>
__global__ __launch_bounds__(256) void refine_gather_kernel(const float* __restrict__ gal_f32, const float* __restrict__ qry,
                                                            int32_t dp, int32_t d, int64_t n, int64_t row_offset,
                                                            const int64_t* __restrict__ cand, int32_t kc, int64_t cand_stride,
                                                            double* __restrict__ val) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t q = blockIdx.y;
  const float* qrow = qry + q * dp;
  const int32_t c0 = (int32_t)blockIdx.x * REFINE_SLAB;
  for (int32_t c = c0 + wv; c < min(c0 + REFINE_SLAB, kc); c += 4) {
    const int64_t id = cand[q * cand_stride + c];
    if (id < 0) continue;                                        // (wave-uniform, like the next one)
    const int64_t local = id - row_offset;
    if (local < 0 || local >= n) continue;
    const float* grow = gal_f32 + local * dp;
    const double v = L2 ? l2_direct_wave(qrow, grow, d, lane) : refine_dot_wave(qrow, grow, d, lane);
    if (lane == 0) val[q * kc + c] = v;
  }
}

// One workgroup per query.  NMAX entries of 16 bytes in LDS: 32 KiB for kc <= 2048 (256 threads, five workgroups fit a CU's
// 160 KiB), 128 KiB for kc <= 8192 (1024 threads, one workgroup per CU).  The key of a value v is f64_key_nan_highest(v) ascending for L2
// and f64_key_nan_highest(0.0 - v) for the inner product, so one ascending sort serves both; padding is (~0, -1), behind everything.
template <bool L2, int NMAX, int THREADS>
__global__ __launch_bounds__(THREADS) void refine_sort_kernel(const double* __restrict__ val, const int64_t* __restrict__ cand,
                                                              int32_t kc, int64_t cand_stride, int64_t n, int64_t row_offset,
                                                              int32_t k, int64_t* __restrict__ out_idx,
                                                              float* __restrict__ out_val, double* __restrict__ out_val64) {
  constexpr int PER = NMAX / THREADS;
  __shared__ uint64_t s_key[NMAX];
  __shared__ int64_t s_id[NMAX];
  __shared__ uint32_t s_cnt[THREADS];
  const int t = threadIdx.x;
  const int64_t q = blockIdx.x;
  uint32_t n2 = 2;
  while (n2 < (uint32_t)kc) n2 <<= 1;                            // <= NMAX (the launcher picks the tier)
  for (uint32_t i = t; i < n2; i += THREADS) {
    int64_t id = -1;
    uint64_t key = ~0ull;
    if (i < (uint32_t)kc) {
      id = cand[q * cand_stride + i];
      const int64_t local = id >= 0 ? id - row_offset : -1;       // (no difference is taken of a negative id: it may not fit)
      if (local >= 0 && local < n) {
        const double v = val[q * kc + i];
        key = f64_key_nan_highest(L2 ? v : 0.0 - v);
      } else {
        id = -1;
      }
    }
    s_key[i] = key;
    s_id[i] = id;
  }
  __syncthreads();
  for (uint32_t size = 2; size <= n2; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t p = t; p < n2 / 2; p += THREADS) {
        const uint32_t lo = 2 * p - (p & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint64_t ka = s_key[lo], kb = s_key[hi];
        const int64_t ia = s_id[lo], ib = s_id[hi];
        const bool after = ka != kb ? ka > kb : (uint64_t)ia > (uint64_t)ib;      // -1 -> the largest: padding last
        if (after == up) {
          s_key[lo] = kb;
          s_key[hi] = ka;
          s_id[lo] = ib;
          s_id[hi] = ia;
        }
      }
      __syncthreads();
    }
  // equal ids carry equal values, so after the sort they are neighbours: an entry stays if it is no padding and differs from
  // the one before it.  Thread t owns entries [t * PER, t * PER + PER): count, scan over the threads, write in order.
  const uint32_t e0 = (uint32_t)t * PER, e1 = min(e0 + (uint32_t)PER, n2);
  uint32_t mine = 0;
  for (uint32_t i = e0; i < e1; ++i) mine += (s_id[i] >= 0 && (i == 0 || s_id[i] != s_id[i - 1])) ? 1u : 0u;
  s_cnt[t] = mine;
  __syncthreads();
  for (int o = 1; o < THREADS; o <<= 1) {
    const uint32_t add = t >= o ? s_cnt[t - o] : 0u;
    __syncthreads();
    s_cnt[t] += add;
    __syncthreads();
  }
  const uint32_t total = s_cnt[THREADS - 1];
  uint32_t pos = s_cnt[t] - mine;
  for (uint32_t i = e0; i < e1 && pos < (uint32_t)k; ++i) {
    if (!(s_id[i] >= 0 && (i == 0 || s_id[i] != s_id[i - 1]))) continue;
    const double dec = f64_key_value(s_key[i]);
    const double v = L2 ? dec : 0.0 - dec;
    out_idx[q * k + pos] = s_id[i];
    if (out_val64) out_val64[q * k + pos] = v;
    if (out_val) out_val[q * k + pos] = (float)v;
    ++pos;
  }
  const double padv = L2 ? (double)INFINITY : -(double)INFINITY;
  for (uint32_t i = total + t; i < (uint32_t)k; i += THREADS) {
    out_idx[q * k + i] = -1;
    if (out_val64) out_val64[q * k + i] = padv;
    if (out_val) out_val[q * k + i] = (float)padv;
  }
}

template <bool L2>
static void refine_launch(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int64_t row_offset,
                          const int64_t* cand, int32_t kc, int64_t cand_stride, int32_t k, int64_t nq, double* val,
                          int64_t* out_idx, float* out_val, double* out_val64, hipStream_t stream) {
  const unsigned slabs = (unsigned)((kc + REFINE_SLAB - 1) / REFINE_SLAB);
  for (int64_t q0 = 0; q0 < nq; q0 += 65535) {                   // (grid.y holds 65535 queries)
    const unsigned b = (unsigned)std::min<int64_t>(65535, nq - q0);
    hipLaunchKernelGGL(refine_gather_kernel<L2>, dim3(slabs, b), dim3(256), 0, stream, gal_f32, qry + q0 * dp, dp, d, n, row_offset,
                       cand + q0 * cand_stride, kc, cand_stride, val + q0 * kc);
  }
  float* ov = out_val;
  double* ov64 = out_val64;
  if (kc <= REFINE_SMALL_KC)
    hipLaunchKernelGGL((refine_sort_kernel<L2, REFINE_SMALL_KC, 256>), dim3((unsigned)nq), dim3(256), 0, stream, val, cand, kc,
                       cand_stride, n, row_offset, k, out_idx, ov, ov64);
  else
    hipLaunchKernelGGL((refine_sort_kernel<L2, REFINE_MAX_KC, 1024>), dim3((unsigned)nq), dim3(1024), 0, stream, val, cand, kc,
                       cand_stride, n, row_offset, k, out_idx, ov, ov64);
}

void launch_refine(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int64_t row_offset, int l2,
                   const int64_t* cand, int32_t kc, int64_t cand_stride, int32_t k, int64_t nq, double* val, int64_t* out_idx,
                   float* out_val, double* out_val64, hipStream_t stream) {
  if (nq <= 0) return;
  if (l2)
    refine_launch<true>(gal_f32, qry, dp, d, n, row_offset, cand, kc, cand_stride, k, nq, val, out_idx, out_val, out_val64, stream);
  else
    refine_launch<false>(gal_f32, qry, dp, d, n, row_offset, cand, kc, cand_stride, k, nq, val, out_idx, out_val, out_val64, stream);
}

}  // namespace mi
