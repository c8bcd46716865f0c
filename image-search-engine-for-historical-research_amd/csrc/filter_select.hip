// Kernels of the filtered top-K search (mi_knn_search_filtered, api_filter.hip).
//   filter_count_kernel / filter_scan_kernel / filter_compact_kernel: the allow bitmap -> ascending list of allowed local rows
//   subset_gather_kernel: the compacted sub-gallery (f32 rows, 16-bit tile-blocked image, RowStat) copied from the shard's
//   filter_overfetch_kernel: the first k allowed entries of a deeper unfiltered top-K' list, and whether they are certified
//   filter_remap_kernel: sub-gallery ids -> shard ids (row_offset + local row), -1 / -inf padding
// None uses scratch or LDS beyond a few hundred words; every store is a plain vector store.
#include "kernels.h"

namespace mi {

constexpr int FILTER_WORDS = 256;     // bitmap words per workgroup of the count / compact kernels (16 384 rows)
constexpr int FILTER_SCAN_THREADS = 1024;

// word w of the bitmap with the bits of rows >= n cleared (w < ceil(n / 64))
__device__ __forceinline__ uint64_t allow_word(const uint64_t* __restrict__ bits, int64_t w, int64_t n) {
  uint64_t v = bits[w];
  const int64_t rest = n - w * 64;
  if (rest < 64) v &= (1ull << rest) - 1ull;
  return v;
}

__device__ __forceinline__ bool allowed_row(const uint64_t* __restrict__ bits, int64_t row, int64_t n) {
  return row >= 0 && row < n && ((bits[row >> 6] >> (row & 63)) & 1ull);
}

// exclusive prefix of one value per thread over a 256-thread workgroup (4 waves); *total = the sum
__device__ __forceinline__ uint32_t block_exclusive_256(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {                 // inclusive scan within the wave
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < wv) before += wsum[i];
    all += wsum[i];
  }
  *total = all;
  return before + x - v;
}

__global__ __launch_bounds__(FILTER_WORDS) void filter_count_kernel(const uint64_t* __restrict__ bits, int64_t n, int64_t nwords,
                                                                    uint32_t* __restrict__ bcnt) {
  const int64_t w = (int64_t)blockIdx.x * FILTER_WORDS + threadIdx.x;
  const uint32_t c = w < nwords ? (uint32_t)__popcll(allow_word(bits, w, n)) : 0u;
  uint32_t total;
  (void)block_exclusive_256(c, &total);
  if (threadIdx.x == 0) bcnt[blockIdx.x] = total;
}

// one workgroup: boff[b] = sum of bcnt[0 .. b), boff[nblk] = total (in place is not allowed: bcnt and boff differ)
__global__ __launch_bounds__(FILTER_SCAN_THREADS) void filter_scan_kernel(const uint32_t* __restrict__ bcnt, int64_t nblk,
                                                                          uint32_t* __restrict__ boff) {
  __shared__ uint32_t sh[FILTER_SCAN_THREADS];
  const int t = threadIdx.x;
  uint32_t carry = 0;
  for (int64_t b0 = 0; b0 < nblk; b0 += FILTER_SCAN_THREADS) {
    const uint32_t v = b0 + t < nblk ? bcnt[b0 + t] : 0u;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < FILTER_SCAN_THREADS; o <<= 1) {      // inclusive scan (Hillis-Steele)
      const uint32_t add = t >= o ? sh[t - o] : 0u;
      __syncthreads();
      sh[t] += add;
      __syncthreads();
    }
    if (b0 + t < nblk) boff[b0 + t] = carry + sh[t] - v;
    carry += sh[FILTER_SCAN_THREADS - 1];
    __syncthreads();
  }
  if (t == 0) boff[nblk] = carry;
}

// thread t of workgroup b writes the allowed rows of word 256 b + t, ascending, from boff[b] + (its exclusive prefix)
__global__ __launch_bounds__(FILTER_WORDS) void filter_compact_kernel(const uint64_t* __restrict__ bits, int64_t n, int64_t nwords,
                                                                      const uint32_t* __restrict__ boff,
                                                                      uint32_t* __restrict__ rows) {
  const int64_t w = (int64_t)blockIdx.x * FILTER_WORDS + threadIdx.x;
  uint64_t v = w < nwords ? allow_word(bits, w, n) : 0ull;
  uint32_t total;
  uint32_t pos = boff[blockIdx.x] + block_exclusive_256((uint32_t)__popcll(v), &total);
  while (v) {
    const int b = __builtin_ctzll(v);
    rows[pos++] = (uint32_t)(w * 64 + b);
    v &= v - 1ull;
  }
}

// One wave per destination row j of the sub-gallery (4 per workgroup).  Row j < m is source row rows[j]: its f32 row is
// copied byte for byte, each 16-byte chunk of its image moves from the source row's swizzle slot to the destination row's
// (common.h: blocked[tile][slice][row % 256][32], physical chunk swz_chunk(row, c)), and its RowStat is copied.  Rows
// m <= j < mpad are the padding of the last tile, written as the ingest writes them: a zero image row and zero norms, no f32
// row.  Loads are issued in batches before their stores (16 B per lane).
constexpr int GATHER_BATCH = 8;
__global__ __launch_bounds__(256) void subset_gather_kernel(const float* __restrict__ src_f32, const uint4* __restrict__ src_img,
                                                            const RowStat* __restrict__ src_stat,
                                                            const uint32_t* __restrict__ rows, int64_t m, int64_t mpad,
                                                            int32_t dp, float* __restrict__ dst_f32,
                                                            uint4* __restrict__ dst_img, RowStat* __restrict__ dst_stat) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= mpad) return;
  const int32_t nslices = dp / SLICE_K;
  const int32_t nchunks = dp / 8;                        // 16-byte image chunks per row
  const int64_t tj = j / TILE;
  const uint32_t rj = (uint32_t)(j % TILE);
  // uint4 index of (tile, slice 0, row r, chunk 0): one slice block is SLICE_ELEMS * 2 / 16 = 1024 uint4
  const int64_t dbase = tj * nslices * (int64_t)(SLICE_ELEMS / 8) + (int64_t)rj * 4;
  if (j >= m) {
    for (int p = lane; p < nchunks; p += 64)
      dst_img[dbase + (int64_t)(p >> 2) * (SLICE_ELEMS / 8) + swz_chunk(rj, p & 3)] = make_uint4(0, 0, 0, 0);
    if (lane < 3) reinterpret_cast<float*>(dst_stat + j)[lane] = 0.0f;
    return;
  }
  const int64_t i = rows[j];
  const int64_t ti = i / TILE;
  const uint32_t ri = (uint32_t)(i % TILE);
  const int64_t sbase = ti * nslices * (int64_t)(SLICE_ELEMS / 8) + (int64_t)ri * 4;
  // f32 row: dp * 4 bytes = dp / 4 uint4
  const int32_t nv = dp / 4;
  const uint4* __restrict__ sf = reinterpret_cast<const uint4*>(src_f32 + i * dp);
  uint4* __restrict__ df = reinterpret_cast<uint4*>(dst_f32 + j * dp);
  int p = lane;
  for (; p + 64 * (GATHER_BATCH - 1) < nv; p += 64 * GATHER_BATCH) {
    uint4 v[GATHER_BATCH];
#pragma unroll
    for (int u = 0; u < GATHER_BATCH; ++u) v[u] = sf[p + 64 * u];
#pragma unroll
    for (int u = 0; u < GATHER_BATCH; ++u) df[p + 64 * u] = v[u];
  }
  for (; p < nv; p += 64) df[p] = sf[p];
  constexpr int IB = GATHER_BATCH / 2;
  auto chunk_at = [](int64_t base, uint32_t r, int c) { return base + (int64_t)(c >> 2) * (SLICE_ELEMS / 8) + swz_chunk(r, c & 3); };
  for (p = lane; p + 64 * (IB - 1) < nchunks; p += 64 * IB) {
    uint4 v[IB];
#pragma unroll
    for (int u = 0; u < IB; ++u) v[u] = src_img[chunk_at(sbase, ri, p + 64 * u)];
#pragma unroll
    for (int u = 0; u < IB; ++u) dst_img[chunk_at(dbase, rj, p + 64 * u)] = v[u];
  }
  for (; p < nchunks; p += 64) dst_img[chunk_at(dbase, rj, p)] = src_img[chunk_at(sbase, ri, p)];
  if (lane < 3) reinterpret_cast<float*>(dst_stat + j)[lane] = reinterpret_cast<const float*>(src_stat + i)[lane];
}

// One wave per query: walks the query's kp entries (score desc, id asc) in order and keeps the first k whose row the bitmap
// allows; the rest of the k slots get -1 / -inf.  ok[q] = 1 when the kept rows are certified to be the filtered answer: k of
// them were found, or the kp entries covered the whole shard (covers != 0).
__global__ __launch_bounds__(256) void filter_overfetch_kernel(const int64_t* __restrict__ in_idx, const float* __restrict__ in_sc,
                                                               int64_t nq, int32_t kp, int32_t k,
                                                               const uint64_t* __restrict__ bits, int64_t n, int64_t row_offset,
                                                               int32_t covers, int64_t* __restrict__ out_idx,
                                                               float* __restrict__ out_sc, uint32_t* __restrict__ ok) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  const int64_t* src_i = in_idx + q * kp;
  const float* src_s = in_sc + q * kp;
  int64_t* dst_i = out_idx + q * k;
  float* dst_s = out_sc + q * k;
  int32_t cnt = 0;                                      // wave-uniform
  for (int32_t b = 0; b < kp && cnt < k; b += 64) {
    const int32_t e = b + lane;
    int64_t id = -1;
    float s = -INFINITY;
    bool keep = false;
    if (e < kp) {
      id = src_i[e];
      s = src_s[e];
      keep = allowed_row(bits, id - row_offset, n);
    }
    const uint64_t mask = __ballot(keep);
    const int32_t pos = cnt + (int32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (keep && pos < k) {
      dst_i[pos] = id;
      dst_s[pos] = s;
    }
    cnt += (int32_t)__popcll(mask);
  }
  const int32_t kept = cnt < k ? cnt : k;
  for (int32_t p = kept + lane; p < k; p += 64) {
    dst_i[p] = -1;
    dst_s[p] = -INFINITY;
  }
  if (lane == 0) ok[q] = (kept >= k || covers) ? 1u : 0u;
}

// [nq][ke] sub-gallery answer -> [nq][k] shard answer: id row_offset + rows[local], score as is; slots ke <= j < k are padding
__global__ __launch_bounds__(256) void filter_remap_kernel(const int64_t* __restrict__ sidx, const float* __restrict__ ssc,
                                                           int64_t nq, int32_t ke, int32_t k, const uint32_t* __restrict__ rows,
                                                           int64_t m, int64_t row_offset, int64_t* __restrict__ out_idx,
                                                           float* __restrict__ out_sc) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nq * k) return;
  const int64_t q = t / k;
  const int32_t j = (int32_t)(t - q * k);
  int64_t id = -1;
  float s = -INFINITY;
  if (j < ke) {
    const int64_t l = sidx[q * ke + j];
    if (l >= 0 && l < m) {
      id = row_offset + rows[l];
      s = ssc[q * ke + j];
    }
  }
  out_idx[t] = id;
  out_sc[t] = s;
}

int64_t filter_blocks(int64_t n) { return ((n + 63) / 64 + FILTER_WORDS - 1) / FILTER_WORDS; }

void launch_filter_compact(const uint64_t* bits, int64_t n, uint32_t* bcnt, uint32_t* boff, uint32_t* rows, hipStream_t stream) {
  const int64_t nwords = (n + 63) / 64, nblk = filter_blocks(n);
  hipLaunchKernelGGL(filter_count_kernel, dim3((unsigned)nblk), dim3(FILTER_WORDS), 0, stream, bits, n, nwords, bcnt);
  hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(FILTER_SCAN_THREADS), 0, stream, (const uint32_t*)bcnt, nblk, boff);
  hipLaunchKernelGGL(filter_compact_kernel, dim3((unsigned)nblk), dim3(FILTER_WORDS), 0, stream, bits, n, nwords,
                     (const uint32_t*)boff, rows);
}

void launch_subset_gather(const float* src_f32, const void* src_img, const RowStat* src_stat, const uint32_t* rows, int64_t m,
                          int64_t mpad, int32_t dp, float* dst_f32, void* dst_img, RowStat* dst_stat, hipStream_t stream) {
  if (mpad <= 0) return;
  hipLaunchKernelGGL(subset_gather_kernel, dim3((unsigned)((mpad + 3) / 4)), dim3(256), 0, stream, src_f32,
                     (const uint4*)src_img, src_stat, rows, m, mpad, dp, dst_f32, (uint4*)dst_img, dst_stat);
}

void launch_filter_overfetch(const int64_t* in_idx, const float* in_sc, int64_t nq, int32_t kp, int32_t k, const uint64_t* bits,
                             int64_t n, int64_t row_offset, int32_t covers, int64_t* out_idx, float* out_sc, uint32_t* ok,
                             hipStream_t stream) {
  if (nq <= 0) return;
  hipLaunchKernelGGL(filter_overfetch_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, stream, in_idx, in_sc, nq, kp, k,
                     bits, n, row_offset, covers, out_idx, out_sc, ok);
}

void launch_filter_remap(const int64_t* sidx, const float* ssc, int64_t nq, int32_t ke, int32_t k, const uint32_t* rows,
                         int64_t m, int64_t row_offset, int64_t* out_idx, float* out_sc, hipStream_t stream) {
  const int64_t total = nq * k;
  if (total <= 0) return;
  hipLaunchKernelGGL(filter_remap_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, sidx, ssc, nq, ke, k, rows,
                     m, row_offset, out_idx, out_sc);
}

}  // namespace mi
