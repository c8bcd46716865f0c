// The ordering stage of the exact range searches: a CSR list of (uint64 key, uint32 local row) entries per query
// -> every query's entries in (key ascending, row ascending) order -> ids and values.  Callers: the inner-product range search
// (api_range.hip) and the Minkowski radius search and self-join (api_minkowski_range.hip).
//
//   csr_sort_kernel    grid = (run of CSR_RUN entries, query): the run ordered in LDS by a bitonic network, in place
//   csr_merge_kernel   one pass: ordered runs of w entries of every query -> runs of 2 w, one thread per entry (its place =
//                      its index in its run + the entries of the other run before it), into the other buffer
//   csr_write_kernel   ordered entries -> int64 id, the float64 behind the key, its float32
// lims holds nq + 1 offsets of which only the differences and lims[0] count: the entries lie from place 0 of the buffers on, the
// outputs from place lims[0] on.  Every kernel first reads *total, the call's hit count, from device memory: beyond max_results it
// writes nothing (uniform per launch).
//
// The order is always ascending.  A caller that wants its values descending stores the COMPLEMENT of f64_key_nan_lowest(value):
// ~key reverses the order of the keys, and (~key asc, row asc) is (value desc, row asc).  That is sound because
//   - a hit is never a NaN (v >= min_score and v <= radius are both false for one), so no hit has the key of a NaN, whose
//     complement in that encoder is ~0: the padding (~0, ~0u) of a run stays behind every hit in either direction;
//   - the entries of one query have distinct rows, so (key, row) is a strict total order: the ordered list is one list, whatever
//     the network's index arithmetic and the order in which workgroups ran.
#include <algorithm>

#include "common.h"
#include "f64_key.h"
#include "kernels.h"

namespace mi {

constexpr int CSR_RUN = 2048;
constexpr int CSR_SORT_THREADS = 1024;

// (key, row) ascending; the padding (~0, ~0) behind every hit
__device__ __forceinline__ bool csr_after(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) { return ka != kb ? ka > kb : ia > ib; }

__global__ __launch_bounds__(CSR_SORT_THREADS) void csr_sort_kernel(uint64_t* __restrict__ key, uint32_t* __restrict__ row,
                                                                    const int64_t* __restrict__ lims,
                                                                    const int64_t* __restrict__ total, int64_t max_results) {
  __shared__ uint64_t k[CSR_RUN];
  __shared__ uint32_t id[CSR_RUN];
  if (*total > max_results) return;
  const uint32_t q = blockIdx.y;
  const int64_t lo = lims[q] - lims[0], n = lims[q + 1] - lims[q];
  const int64_t r0 = (int64_t)blockIdx.x * CSR_RUN;
  if (r0 >= n) return;
  const uint32_t m = (uint32_t)min((int64_t)CSR_RUN, n - r0);
  if (m < 2) return;
  uint32_t len = 2;
  while (len < m) len <<= 1;                                                // block-uniform network width
  for (uint32_t i = threadIdx.x; i < len; i += CSR_SORT_THREADS) {
    const bool v = i < m;
    k[i] = v ? key[lo + r0 + i] : ~0ull;
    id[i] = v ? row[lo + r0 + i] : 0xFFFFFFFFu;
  }
  __syncthreads();
  for (uint32_t w = 2; w <= len; w <<= 1) {
    for (uint32_t j = w >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < (len >> 1); t += CSR_SORT_THREADS) {
        const uint32_t a = 2 * t - (t & (j - 1)), b = a + j;
        const bool up = (a & w) == 0;                                       // this half of the network puts a before b
        const uint64_t ka = k[a], kb = k[b];
        const uint32_t ia = id[a], ib = id[b];
        if (csr_after(ka, ia, kb, ib) == up) {
          k[a] = kb; k[b] = ka;
          id[a] = ib; id[b] = ia;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = threadIdx.x; i < m; i += CSR_SORT_THREADS) {
    key[lo + r0 + i] = k[i];
    row[lo + r0 + i] = id[i];
  }
}

// Entries are distinct (a query holds a row once), so "not after" is "before"
__global__ __launch_bounds__(256) void csr_merge_kernel(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ srow,
                                                        uint64_t* __restrict__ dkey, uint32_t* __restrict__ drow,
                                                        const int64_t* __restrict__ lims, int32_t nq, int64_t w,
                                                        const int64_t* __restrict__ total, int64_t max_results) {
  if (*total > max_results) return;
  const int64_t first = lims[0], cnt = lims[nq] - first;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = nq;                                                    // query of entry i: lims[q] <= first + i < lims[q + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (lims[mid] - first <= i) lo = mid; else hi = mid;
    }
    const int64_t base = lims[lo] - first, n = lims[lo + 1] - lims[lo], local = i - base;
    const int64_t start = local / (2 * w) * (2 * w);
    const int64_t a0 = start, a1 = min(start + w, n), b0 = a1, b1 = min(start + 2 * w, n);
    const uint64_t kx = skey[i];
    const uint32_t ix = srow[i];
    const bool in_a = local < a1;
    int64_t l = in_a ? b0 : a0, h = in_a ? b1 : a1;                         // the other run's entries before x
    while (l < h) {
      const int64_t mid = (l + h) >> 1;
      if (csr_after(kx, ix, skey[base + mid], srow[base + mid])) l = mid + 1; else h = mid;
    }
    const int64_t place = start + (local - (in_a ? a0 : b0)) + (l - (in_a ? b0 : a0));
    dkey[base + place] = kx;
    drow[base + place] = ix;
  }
}

// COMPLEMENT: the stored key is ~f64_key_nan_lowest(value) (a descending caller), otherwise the key of the value itself
template <bool COMPLEMENT>
__global__ __launch_bounds__(256) void csr_write_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ row,
                                                        const int64_t* __restrict__ lims, int32_t nq, int64_t row_offset,
                                                        const int64_t* __restrict__ total, int64_t max_results,
                                                        int64_t* __restrict__ out_idx, float* __restrict__ out_val,
                                                        double* __restrict__ out_val64) {
  if (*total > max_results) return;
  const int64_t first = lims[0], cnt = lims[nq] - first;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = f64_key_value(COMPLEMENT ? ~key[i] : key[i]);
    out_idx[first + i] = row_offset + (int64_t)row[i];
    if (out_val64) out_val64[first + i] = v;
    if (out_val) out_val[first + i] = (float)v;
  }
}

static unsigned csr_flat_grid(int64_t max_total) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((max_total + 255) / 256, 8192)); }

int launch_csr_order(const CsrList& a, int64_t max_cnt, int64_t max_total, hipStream_t stream) {
  if (a.nq <= 0 || max_cnt < 2) return 0;
  const unsigned runs = (unsigned)((max_cnt + CSR_RUN - 1) / CSR_RUN);
  csr_sort_kernel<<<dim3(runs, (unsigned)a.nq), CSR_SORT_THREADS, 0, stream>>>(a.key[0], a.row[0], a.lims, a.total, a.max_results);
  int cur = 0;
  for (int64_t w = CSR_RUN; w < max_cnt; w *= 2) {
    csr_merge_kernel<<<dim3(csr_flat_grid(max_total)), 256, 0, stream>>>(a.key[cur], a.row[cur], a.key[cur ^ 1], a.row[cur ^ 1], a.lims,
                                                                        a.nq, w, a.total, a.max_results);
    cur ^= 1;
  }
  return cur;
}

void launch_csr_write(const CsrList& a, int cur, bool complement, int64_t max_total, int64_t row_offset, int64_t* out_idx,
                      float* out_val, double* out_val64, hipStream_t stream) {
  if (a.nq <= 0) return;
  auto kernel = complement ? csr_write_kernel<true> : csr_write_kernel<false>;
  kernel<<<dim3(csr_flat_grid(max_total)), 256, 0, stream>>>(a.key[cur], a.row[cur], a.lims, a.nq, row_offset, a.total, a.max_results,
                                                            out_idx, out_val, out_val64);
}

int64_t csr_run_length() { return CSR_RUN; }

}  // namespace mi
