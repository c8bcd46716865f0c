// Kernels of the exact range search (api_range.hip): the fixed threshold of the scoring launches, the survivor rows handed to
// the exact re-score (rescore_kernel, select.hip, unchanged), the rows kept at exact score >= min_score, their per-query
// counts and offsets (CSR), and the order of every query's hits by (f64 score desc, row asc): runs of up to RANGE_RUN entries
// sorted in LDS, longer lists merged in global memory.  DESIGN.md section 5.9.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace mi {

// thr[q] = min_score - margin[q] / 2 in f64, rounded toward -inf into f32: every row with exact score >= min_score has a 16-bit
// (or f32) score >= thr (certificate, DESIGN 4: |approx - exact| <= eps_q = margin / 2).  Queries whose 16-bit image overflowed
// (init_query_state_kernel: thr = +inf, FLAG_RANGE) and padded queries keep +inf.  Zeroes the survivor counters.
__global__ __launch_bounds__(256) void range_threshold_kernel(QueryState st, int32_t nq, int32_t qpad, double min_score) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= qpad) return;
  st.cnt[q * CNT_STRIDE] = 0;
  if (q >= nq || st.thr[q] == INFINITY) return;
  const double t = min_score - 0.5 * (double)st.margin[q];
  float f = (float)t;
  if ((double)f > t) f = nextafterf(f, -INFINITY);
  st.thr[q] = f;
}

void launch_range_threshold(QueryState st, int32_t nq, int32_t qpad, double min_score, hipStream_t stream) {
  hipLaunchKernelGGL(range_threshold_kernel, dim3((qpad + 255) / 256), dim3(256), 0, stream, st, nq, qpad, min_score);
}

// start of a chunk: survivor counters and the chunk's hit counter to zero
__global__ __launch_bounds__(256) void range_chunk_begin_kernel(QueryState st, int32_t qpad, unsigned long long* total) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q == 0) *total = 0ull;
  if (q < qpad) st.cnt[q * CNT_STRIDE] = 0;
}

void launch_range_chunk_begin(QueryState st, int32_t qpad, unsigned long long* total, hipStream_t stream) {
  hipLaunchKernelGGL(range_chunk_begin_kernel, dim3((qpad + 255) / 256), dim3(256), 0, stream, st, qpad, total);
}

// rows to re-score, [nq][st.cap]: dense == 0 -> the survivors of the chunk (count clamped to the list's capacity); dense != 0 ->
// every row of [row0, row0 + nrows) (nrows <= st.cap), the dense path of a chunk whose survivors do not fit the buffers
__global__ __launch_bounds__(256) void range_rows_kernel(QueryState st, uint32_t* __restrict__ rows, uint32_t* __restrict__ rcnt,
                                                         int32_t dense, uint32_t row0, uint32_t nrows) {
  const uint32_t q = blockIdx.y;
  const uint32_t n = dense ? min(nrows, st.cap) : min(st.cnt[q * CNT_STRIDE], st.cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) rcnt[q] = n;
  const uint64_t* src = st.surv + (uint64_t)q * st.cap;
  uint32_t* dst = rows + (uint64_t)q * st.cap;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    dst[i] = dense ? row0 + i : entry_row(src[i]);
}

void launch_range_rows(QueryState st, int32_t nq, uint32_t* rows, uint32_t* rcnt, int dense, uint32_t row0, uint32_t nrows,
                       hipStream_t stream) {
  hipLaunchKernelGGL(range_rows_kernel, dim3(16, nq), dim3(256), 0, stream, st, rows, rcnt, dense, row0, nrows);
}

// order-preserving 64-bit key of an f64 score (the key of emit_kernel): NaN lowest, -0 == +0
__device__ __forceinline__ uint64_t range_key(double s) {
  if (s != s) return 0ull;
  if (s == 0.0) return 0x8000000000000000ull;
  const uint64_t b = (uint64_t)__double_as_longlong(s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double range_unkey(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)b);
}
// "a comes before b": score desc, row asc
__device__ __forceinline__ bool range_before(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
  return ka > kb || (ka == kb && ia < ib);
}

// keep the re-scored rows with f64 score >= min_score: query q's hits of this chunk go to key/row[off[q] .. off[q] + cnt[q]),
// off[q] = base + its share of the chunk's counter *total (the order of the queries inside a chunk is whatever the atomics
// give; api_range.hip orders every query's hits afterwards).  Writes past `cap` (never: the host sizes the buffer for every
// re-scored row) raise FLAG_SURV_OVERFLOW instead.
__global__ __launch_bounds__(256) void range_keep_kernel(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ rcnt,
                                                         const double* __restrict__ sc, uint32_t lcap, double min_score,
                                                         unsigned long long* total, uint64_t* __restrict__ off,
                                                         uint32_t* __restrict__ cnt, uint64_t* __restrict__ key,
                                                         uint32_t* __restrict__ row, uint64_t base, uint64_t cap,
                                                         uint32_t* flags) {
  __shared__ uint32_t c;
  __shared__ uint64_t o;
  const uint32_t q = blockIdx.x;
  const uint32_t n = min(rcnt[q], lcap);
  const double* s = sc + (uint64_t)q * lcap;
  const uint32_t* r = rows + (uint64_t)q * lcap;
  if (threadIdx.x == 0) c = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) mine += s[i] >= min_score ? 1u : 0u;
  if (mine) atomicAdd(&c, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    o = base + atomicAdd(total, (unsigned long long)c);
    off[q] = o;
    cnt[q] = c;
    c = 0;
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    const double v = s[i];
    if (v >= min_score) {
      const uint64_t p = o + atomicAdd(&c, 1u);
      if (p < cap) {
        key[p] = range_key(v);
        row[p] = r[i];
      } else {
        atomicOr(flags, FLAG_SURV_OVERFLOW);
      }
    }
  }
}

void launch_range_keep(const uint32_t* rows, const uint32_t* rcnt, const double* sc, uint32_t lcap, int32_t nq, double min_score,
                       unsigned long long* total, uint64_t* off, uint32_t* cnt, uint64_t* key, uint32_t* row, uint64_t base,
                       uint64_t cap, uint32_t* flags, hipStream_t stream) {
  hipLaunchKernelGGL(range_keep_kernel, dim3(nq), dim3(256), 0, stream, rows, rcnt, sc, lcap, min_score, total, off, cnt, key,
                     row, base, cap, flags);
}

// per-query hit counts summed over the chunks of a batch ([nchunks][ld]) and their exclusive prefix: lims[0 .. nq], one block
constexpr int RANGE_LIMS_THREADS = 1024;
__global__ __launch_bounds__(RANGE_LIMS_THREADS) void range_lims_kernel(const uint32_t* __restrict__ cnt, int32_t nchunks,
                                                                        int32_t ld, int32_t nq, int64_t* __restrict__ lims) {
  __shared__ int64_t sh[RANGE_LIMS_THREADS];
  const int q = threadIdx.x;
  int64_t v = 0;
  if (q < nq)
    for (int c = 0; c < nchunks; ++c) v += cnt[(uint64_t)c * ld + q];
  sh[q] = v;
  __syncthreads();
  for (int o = 1; o < RANGE_LIMS_THREADS; o <<= 1) {       // inclusive scan (Hillis-Steele)
    const int64_t add = q >= o ? sh[q - o] : 0;
    __syncthreads();
    sh[q] += add;
    __syncthreads();
  }
  if (q < nq) lims[q + 1] = sh[q];
  if (q == 0) lims[0] = 0;
}

void launch_range_lims(const uint32_t* cnt, int32_t nchunks, int32_t ld, int32_t nq, int64_t* lims, hipStream_t stream) {
  hipLaunchKernelGGL(range_lims_kernel, dim3(1), dim3(RANGE_LIMS_THREADS), 0, stream, cnt, nchunks, ld, nq, lims);
}

// the pieces of query q (one per chunk) into its CSR slot [lims[q], lims[q + 1])
__global__ __launch_bounds__(256) void range_gather_kernel(const uint64_t* __restrict__ akey, const uint32_t* __restrict__ arow,
                                                           const uint64_t* __restrict__ off, const uint32_t* __restrict__ cnt,
                                                           int32_t nchunks, int32_t ld, const int64_t* __restrict__ lims,
                                                           uint64_t* __restrict__ key, uint32_t* __restrict__ row) {
  const uint32_t q = blockIdx.x;
  uint64_t dst = (uint64_t)lims[q];
  for (int c = 0; c < nchunks; ++c) {
    const uint32_t n = cnt[(uint64_t)c * ld + q];
    const uint64_t src = off[(uint64_t)c * ld + q];
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      key[dst + i] = akey[src + i];
      row[dst + i] = arow[src + i];
    }
    dst += n;
  }
}

void launch_range_gather(const uint64_t* akey, const uint32_t* arow, const uint64_t* off, const uint32_t* cnt, int32_t nchunks,
                         int32_t ld, int32_t nq, const int64_t* lims, uint64_t* key, uint32_t* row, hipStream_t stream) {
  hipLaunchKernelGGL(range_gather_kernel, dim3(nq), dim3(256), 0, stream, akey, arow, off, cnt, nchunks, ld, lims, key, row);
}

// runs [lims[q] + r * RANGE_RUN, ...) of every query sorted in LDS (bitonic network, 1024 threads, 24 KiB), in place
constexpr int RANGE_RUN = 2048;
__global__ __launch_bounds__(1024) void range_sort_runs_kernel(uint64_t* __restrict__ key, uint32_t* __restrict__ row,
                                                               const int64_t* __restrict__ lims) {
  __shared__ uint64_t k[RANGE_RUN];
  __shared__ uint32_t id[RANGE_RUN];
  const uint32_t q = blockIdx.y;
  const int64_t lo = lims[q], n = lims[q + 1] - lo;
  const int64_t r0 = (int64_t)blockIdx.x * RANGE_RUN;
  if (r0 >= n) return;
  const uint32_t m = (uint32_t)min((int64_t)RANGE_RUN, n - r0);
  uint32_t len = 2;
  while (len < m) len <<= 1;                               // block-uniform network width
  for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) {
    const bool v = i < m;
    k[i] = v ? key[lo + r0 + i] : 0ull;                    // padding: key 0 with the largest id comes after everything
    id[i] = v ? row[lo + r0 + i] : 0xFFFFFFFFu;
  }
  __syncthreads();
  for (uint32_t w = 2; w <= len; w <<= 1) {
    for (uint32_t j = w >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < (len >> 1); t += blockDim.x) {
        const uint32_t a = 2 * j * (t / j) + (t % j), b = a + j;
        const bool up = (a & w) == 0;                      // this half of the network puts a before b
        const uint64_t ka = k[a], kb = k[b];
        const uint32_t ia = id[a], ib = id[b];
        const bool swap = up ? range_before(kb, ib, ka, ia) : range_before(ka, ia, kb, ib);
        if (swap) {
          k[a] = kb; k[b] = ka;
          id[a] = ib; id[b] = ia;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
    key[lo + r0 + i] = k[i];
    row[lo + r0 + i] = id[i];
  }
}

void launch_range_sort_runs(uint64_t* key, uint32_t* row, const int64_t* lims, int32_t nq, int64_t max_cnt, hipStream_t stream) {
  const unsigned runs = (unsigned)((max_cnt + RANGE_RUN - 1) / RANGE_RUN);
  if (runs == 0) return;
  hipLaunchKernelGGL(range_sort_runs_kernel, dim3(runs, nq), dim3(1024), 0, stream, key, row, lims);
}
int64_t range_run_length() { return RANGE_RUN; }

// one merge pass: sorted runs of width w of every query become runs of 2 w.  One thread per entry: its place in the merged
// run is its index in its own run plus the number of entries of the other run that come before it (binary search; an equal
// entry -- never, ids of a query are distinct -- counts as before for the second run only, so the places stay distinct).
__global__ __launch_bounds__(256) void range_merge_kernel(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ srow,
                                                          uint64_t* __restrict__ dkey, uint32_t* __restrict__ drow,
                                                          const int64_t* __restrict__ lims, int32_t nq, int64_t w) {
  const int64_t total = lims[nq];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = nq;                                    // query of entry i: lims[q] <= i < lims[q + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (lims[mid] <= i) lo = mid; else hi = mid;
    }
    const int64_t base = lims[lo], n = lims[lo + 1] - base, local = i - base;
    const int64_t start = local / (2 * w) * (2 * w);
    const int64_t a0 = start, a1 = min(start + w, n), b0 = a1, b1 = min(start + 2 * w, n);
    const uint64_t kx = skey[i];
    const uint32_t ix = srow[i];
    const bool in_a = local < a1;
    int64_t l = in_a ? b0 : a0, h = in_a ? b1 : a1;         // count the other run's entries before (a) / not after (b) x
    while (l < h) {
      const int64_t mid = (l + h) >> 1;
      const uint64_t km = skey[base + mid];
      const uint32_t im = srow[base + mid];
      const bool before = in_a ? range_before(km, im, kx, ix) : !range_before(kx, ix, km, im);
      if (before) l = mid + 1; else h = mid;
    }
    const int64_t place = start + (local - (in_a ? a0 : b0)) + (l - (in_a ? b0 : a0));
    dkey[base + place] = kx;
    drow[base + place] = ix;
  }
}

void launch_range_merge(const uint64_t* skey, const uint32_t* srow, uint64_t* dkey, uint32_t* drow, const int64_t* lims,
                        int32_t nq, int64_t total, int64_t w, hipStream_t stream) {
  if (total <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(range_merge_kernel, dim3(grid), dim3(256), 0, stream, skey, srow, dkey, drow, lims, nq, w);
}

// sorted hits -> (row_offset + row, f32 of the f64 score)
__global__ __launch_bounds__(256) void range_emit_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ row,
                                                         int64_t total, int64_t row_offset, int64_t* __restrict__ out_idx,
                                                         float* __restrict__ out_score) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    out_idx[i] = row_offset + (int64_t)row[i];
    out_score[i] = (float)range_unkey(key[i]);
  }
}

void launch_range_emit(const uint64_t* key, const uint32_t* row, int64_t total, int64_t row_offset, int64_t* out_idx,
                       float* out_score, hipStream_t stream) {
  if (total <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(range_emit_kernel, dim3(grid), dim3(256), 0, stream, key, row, total, row_offset, out_idx, out_score);
}

}  // namespace mi
