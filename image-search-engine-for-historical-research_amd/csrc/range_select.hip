// Kernels of the exact range search (api_range.hip): the fixed threshold of the scoring launches, the survivor rows handed to
// the exact re-score (rescore_kernel, select.hip, unchanged), the rows kept at exact score >= min_score, their per-query
// counts and offsets (CSR) and every query's hits gathered into its CSR slot as (~key of the f64 score, row): csr_order.hip puts
// them in (key asc, row asc) order, which is (score desc, row asc), and writes them out.  DESIGN.md section 5.9.
#include "common.h"
#include "f64_key.h"
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

// keep the re-scored rows with f64 score >= min_score: query q's hits of this chunk go to key/row[off[q] .. off[q] + cnt[q]),
// off[q] = base + its share of the chunk's counter *total (the order of the queries inside a chunk is whatever the atomics
// give; api_range.hip orders every query's hits afterwards), keyed by the complement of f64_key_nan_lowest(score).  Writes
// past `cap` (never: the host sizes the buffer for every re-scored row) raise FLAG_SURV_OVERFLOW instead.
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
        key[p] = ~f64_key_nan_lowest(v);                      // complemented: key ascending = score descending
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

}  // namespace mi
