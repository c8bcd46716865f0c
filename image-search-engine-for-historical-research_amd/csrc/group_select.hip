// Kernels of the grouped top-K search (mi_knn_search_grouped, api_group.hip).
//   group_collapse_kernel  path 2: a query's unfiltered top-K' list -> the first entry of every group in rank order, the first k of
//                          them, and whether they are certified
//   group_best_kernel      path 1: dense float64 scores [query][row] -> (best value, lowest row among equals) of every group, over
//                          the group CSR cut into chunks of whole groups
//   group_lims_kernel      the CSR offsets of the per-query lists of G entries, for csr_order.hip
//   group_take_kernel      the first k entries of every ordered list -> candidate rows for rescore_kernel
//   group_emit_kernel      candidate rows and their re-scored values -> ids, float32 scores, labels, padding
// Wave64, plain vector stores, no scratch, no atomics: every result is a function of the inputs alone.
#include "common.h"
#include "f64_key.h"
#include "kernels.h"

namespace mi {

constexpr int COLLAPSE_THREADS = 1024;
constexpr int COLLAPSE_MAX = 2048;            // the deepest list (K' <= 2048)
constexpr uint32_t NO_GROUP = 0xFFFFFFFFu;    // no dense group id reaches it (G <= n < 2^32 - 1)

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int o) {
  const uint32_t lo = __shfl_down((uint32_t)v, o, 64), hi = __shfl_down((uint32_t)(v >> 32), o, 64);
  return ((uint64_t)hi << 32) | lo;
}

// Ascending bitonic sort of `len` distinct-or-padding uint64 keys in LDS (len a power of two, 64 <= len <= 2048, every thread of
// the 1024 calls it).  A step of distance j >= 64 exchanges through LDS: the 32 lanes of a half-wave touch 32 consecutive keys
// (256 B, one bank row) on either side, so ds_read_b64 / ds_write_b64 see no bank conflict.  The steps of distance <= 32 of a
// stage would put the half-wave on every other key or worse (2-way and up); they run in registers instead: thread t holds keys t
// and t + 1024, read and written back in consecutive order, and the partner of key i, key i ^ j, sits in the same wave.
__device__ __forceinline__ void sort_keys_lds(uint64_t* key, uint32_t len) {
  const uint32_t t = threadIdx.x;
  for (uint32_t w = 2; w <= len; w <<= 1) {
    uint32_t j = w >> 1;
    for (; j >= 64; j >>= 1) {
      for (uint32_t p = t; p < (len >> 1); p += COLLAPSE_THREADS) {
        const uint32_t a = 2 * p - (p & (j - 1)), b = a + j;
        const uint64_t ka = key[a], kb = key[b];
        if ((ka > kb) == ((a & w) == 0)) {
          key[a] = kb;
          key[b] = ka;
        }
      }
      __syncthreads();
    }
    for (uint32_t i = t; i < len; i += COLLAPSE_THREADS) {       // whole waves: len is a multiple of 64
      uint64_t x = key[i];
      const bool up = (i & w) == 0;
      for (uint32_t jj = j; jj > 0; jj >>= 1) {
        const uint64_t y = shfl_xor_u64(x, (int)jj);
        const bool lower = (i & jj) == 0;
        x = (lower == up) ? (x < y ? x : y) : (x > y ? x : y);
      }
      key[i] = x;
    }
    __syncthreads();
  }
}

// One workgroup per query.  in_idx / in_sc [nq][kp]: the query's list in (score desc, id asc) order.  Keys (dense group << 32 |
// rank) sorted ascending put the entries of a group side by side with the best-ranked first; that entry is marked at its rank unless
// the group is the excluded one (excl[q], NO_GROUP = none); a prefix count over the marks in rank order gives the kept entries
// their places, the first k are written, the rest of the k slots is padding.  ok[q] = 1 when the answer is certified: k entries
// were kept, or the list covered the shard.
__global__ __launch_bounds__(COLLAPSE_THREADS) void group_collapse_kernel(
    const int64_t* __restrict__ in_idx, const float* __restrict__ in_sc, int32_t kp, int32_t k, const uint32_t* __restrict__ grp,
    const int32_t* __restrict__ label_of_group, int64_t n, int64_t row_offset, const uint32_t* __restrict__ excl, int32_t covers,
    int64_t* __restrict__ out_idx, float* __restrict__ out_sc, int32_t* __restrict__ out_lab, uint32_t* __restrict__ ok) {
  __shared__ uint64_t key[COLLAPSE_MAX];
  __shared__ uint32_t gid[COLLAPSE_MAX];
  __shared__ __attribute__((aligned(8))) uint32_t mark[COLLAPSE_MAX];
  __shared__ uint32_t wsum[COLLAPSE_THREADS / 64];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t q = blockIdx.x;
  const uint32_t ukp = (uint32_t)min(kp, COLLAPSE_MAX);
  uint32_t len = 64;
  while (len < ukp) len <<= 1;
  const int64_t* src_i = in_idx + q * kp;
  const float* src_s = in_sc + q * kp;
  const uint32_t ex = excl[q];
  for (uint32_t i = t; i < COLLAPSE_MAX; i += COLLAPSE_THREADS) {
    uint32_t g = NO_GROUP;
    if (i < ukp) {
      const int64_t local = src_i[i] - row_offset;
      if (local >= 0 && local < n) g = grp[local];
    }
    gid[i] = g;
    mark[i] = 0u;
    key[i] = i < ukp ? (((uint64_t)g << 32) | i) : ~0ull;
  }
  __syncthreads();
  sort_keys_lds(key, len);
  for (uint32_t i = t; i < len; i += COLLAPSE_THREADS) {
    const uint64_t kk = key[i];
    const uint32_t g = (uint32_t)(kk >> 32);
    const bool first = i == 0 || (uint32_t)(key[i - 1] >> 32) != g;
    if (first && g != NO_GROUP && g != ex) mark[(uint32_t)kk] = 1u;       // g != NO_GROUP: the low word is a rank < kp
  }
  __syncthreads();
  // thread t owns ranks 2 t and 2 t + 1 (one 8-byte read: consecutive lanes, consecutive addresses)
  const uint2 m = reinterpret_cast<const uint2*>(mark)[t];
  const uint32_t c = m.x + m.y;
  uint32_t x = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (uint32_t i = 0; i < COLLAPSE_THREADS / 64; ++i) {
    const uint32_t s = wsum[i];
    if (i < wv) before += s;
    total += s;
  }
  int64_t* dst_i = out_idx + q * k;
  float* dst_s = out_sc + q * k;
  int32_t* dst_l = out_lab + q * k;
  uint32_t pos = before + x - c;
  const uint32_t uk = (uint32_t)k;
  if (m.x && pos < uk) {
    const uint32_t r = 2 * t;
    dst_i[pos] = src_i[r];
    dst_s[pos] = src_s[r];
    dst_l[pos] = label_of_group[gid[r]];
  }
  pos += m.x;
  if (m.y && pos < uk) {
    const uint32_t r = 2 * t + 1;
    dst_i[pos] = src_i[r];
    dst_s[pos] = src_s[r];
    dst_l[pos] = label_of_group[gid[r]];
  }
  const uint32_t kept = total < uk ? total : uk;
  for (uint32_t p = kept + t; p < uk; p += COLLAPSE_THREADS) {
    dst_i[p] = -1;
    dst_s[p] = -INFINITY;
    dst_l[p] = -1;
  }
  if (t == 0) ok[q] = (total >= uk || covers) ? 1u : 0u;
}

// (complemented key, row) ascending is (value desc, row asc)
__device__ __forceinline__ bool best_before(uint64_t ka, uint32_t ra, uint64_t kb, uint32_t rb) { return ka != kb ? ka < kb : ra < rb; }

// grid = (chunk, query).  Chunk c holds the groups [chunk_g0[c], chunk_g0[c + 1]): whole groups of at most GROUP_CHUNK_ROWS rows
// together, or ONE larger group, which this workgroup then walks alone.  The rows of the chunk are the places
// [group_off[g0], group_off[g1]) of group_rows, group after group, ascending inside a group.  Per tile of 256 places: every lane
// takes one place, a segmented shuffle reduction leaves the best entry of every run of equal group with the run's first lane, and
// the run heads go into the chunk's table in LDS wave after wave (two heads of one wave never name one group; a run cut by a wave
// or tile edge meets its other part there).  The minimum of a strict total order does not depend on the order of the steps anyway;
// the fixed order keeps two waves from writing one slot at once.  The entry of the excluded group (excl[q]) is replaced by the
// marker (~0, ~0u), which sorts behind every real entry.
__global__ __launch_bounds__(GROUP_BEST_THREADS) void group_best_kernel(
    const double* __restrict__ dense, int64_t ld, const uint32_t* __restrict__ grp, const uint32_t* __restrict__ group_rows,
    const uint32_t* __restrict__ group_off, const uint32_t* __restrict__ chunk_g0, int64_t G, const uint32_t* __restrict__ excl,
    uint64_t* __restrict__ out_key, uint32_t* __restrict__ out_row) {
  __shared__ uint64_t bk[GROUP_CHUNK_ROWS];
  __shared__ uint32_t br[GROUP_CHUNK_ROWS];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t q = blockIdx.y;
  const uint32_t g0 = chunk_g0[blockIdx.x], g1 = chunk_g0[blockIdx.x + 1];
  const uint32_t ng = min(g1 - g0, (uint32_t)GROUP_CHUNK_ROWS);
  const uint32_t r0 = group_off[g0], r1 = group_off[g1];
  const double* row_scores = dense + q * ld;
  for (uint32_t i = t; i < ng; i += GROUP_BEST_THREADS) {
    bk[i] = ~0ull;
    br[i] = ~0u;
  }
  __syncthreads();
  for (uint32_t base = r0; base < r1; base += GROUP_BEST_THREADS) {      // block-uniform trip count
    const uint32_t p = base + t;
    const bool valid = p < r1;
    uint64_t key = ~0ull;
    uint32_t row = ~0u, gi = NO_GROUP;
    if (valid) {
      row = group_rows[p];
      gi = grp[row] - g0;
      key = ~f64_key_nan_lowest(row_scores[row]);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t ok_ = shfl_down_u64(key, o);
      const uint32_t or_ = __shfl_down(row, o, 64), og = __shfl_down(gi, o, 64);
      if (lane + o < 64 && og == gi && best_before(ok_, or_, key, row)) {
        key = ok_;
        row = or_;
      }
    }
    const uint32_t gprev = __shfl_up(gi, 1, 64);
    const bool head = valid && gi < ng && (lane == 0 || gprev != gi);
#pragma unroll
    for (uint32_t w = 0; w < GROUP_BEST_THREADS / 64; ++w) {
      if (wv == w && head && best_before(key, row, bk[gi], br[gi])) {
        bk[gi] = key;
        br[gi] = row;
      }
      __syncthreads();
    }
  }
  const uint32_t ex = excl[q];
  for (uint32_t i = t; i < ng; i += GROUP_BEST_THREADS) {
    const bool gone = g0 + i == ex;
    out_key[q * G + g0 + i] = gone ? ~0ull : bk[i];
    out_row[q * G + g0 + i] = gone ? ~0u : br[i];
  }
}

__global__ __launch_bounds__(256) void group_lims_kernel(int64_t* __restrict__ lims, int64_t* __restrict__ total, int32_t nq, int64_t G) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i <= nq) lims[i] = (int64_t)i * G;
  if (i == 0) *total = 0;
}

// row [nq][G]: every query's entries in (value desc, row asc) order, the marker of an excluded group last.  -> cand_rows [nq][k]
// (slots past the list hold row 0) and cand_cnt [nq], the entries taken: one writer per query, the thread of the last real entry
__global__ __launch_bounds__(256) void group_take_kernel(const uint32_t* __restrict__ row, int64_t G, int32_t nq, int32_t k,
                                                         uint32_t* __restrict__ cand_rows, uint32_t* __restrict__ cand_cnt) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)nq * k) return;
  const int64_t q = t / k, j = t - q * k;
  const int64_t lim = G < k ? G : (int64_t)k;
  const uint32_t r = j < lim ? row[q * G + j] : ~0u;
  const bool real = r != ~0u;
  cand_rows[t] = real ? r : 0u;
  if (real && (j + 1 == lim || row[q * G + j + 1] == ~0u)) cand_cnt[q] = (uint32_t)(j + 1);
  if (j == 0 && !real) cand_cnt[q] = 0u;
}

__global__ __launch_bounds__(256) void group_emit_kernel(const uint32_t* __restrict__ cand_rows, const uint32_t* __restrict__ cand_cnt,
                                                         const double* __restrict__ cand_score, const uint32_t* __restrict__ grp,
                                                         const int32_t* __restrict__ label_of_group, int32_t nq, int32_t k,
                                                         int64_t row_offset, int64_t* __restrict__ out_idx,
                                                         float* __restrict__ out_sc, int32_t* __restrict__ out_lab) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)nq * k) return;
  const int64_t q = t / k, j = t - q * k;
  int64_t id = -1;
  float s = -INFINITY;
  int32_t lab = -1;
  if (j < (int64_t)min(cand_cnt[q], (uint32_t)k)) {
    const uint32_t r = cand_rows[t];
    id = row_offset + r;
    s = (float)cand_score[t];
    lab = label_of_group[grp[r]];
  }
  out_idx[t] = id;
  out_sc[t] = s;
  out_lab[t] = lab;
}

void launch_group_collapse(const int64_t* in_idx, const float* in_sc, int64_t nq, int32_t kp, int32_t k, const uint32_t* grp,
                           const int32_t* label_of_group, int64_t n, int64_t row_offset, const uint32_t* excl, int32_t covers,
                           int64_t* out_idx, float* out_sc, int32_t* out_lab, uint32_t* ok, hipStream_t stream) {
  if (nq <= 0) return;
  hipLaunchKernelGGL(group_collapse_kernel, dim3((unsigned)nq), dim3(COLLAPSE_THREADS), 0, stream, in_idx, in_sc, kp, k, grp,
                     label_of_group, n, row_offset, excl, covers, out_idx, out_sc, out_lab, ok);
}

void launch_group_best(const double* dense, int64_t ld, int32_t nq, const uint32_t* grp, const uint32_t* group_rows,
                       const uint32_t* group_off, const uint32_t* chunk_g0, int64_t chunks, int64_t G, const uint32_t* excl,
                       uint64_t* out_key, uint32_t* out_row, hipStream_t stream) {
  if (nq <= 0 || chunks <= 0) return;
  hipLaunchKernelGGL(group_best_kernel, dim3((unsigned)chunks, (unsigned)nq), dim3(GROUP_BEST_THREADS), 0, stream, dense, ld, grp,
                     group_rows, group_off, chunk_g0, G, excl, out_key, out_row);
}

void launch_group_lims(int64_t* lims, int64_t* total, int32_t nq, int64_t G, hipStream_t stream) {
  hipLaunchKernelGGL(group_lims_kernel, dim3((unsigned)(nq / 256 + 1)), dim3(256), 0, stream, lims, total, nq, G);
}

void launch_group_take(const uint32_t* row, int64_t G, int32_t nq, int32_t k, uint32_t* cand_rows, uint32_t* cand_cnt,
                       hipStream_t stream) {
  const int64_t total = (int64_t)nq * k;
  if (total <= 0) return;
  hipLaunchKernelGGL(group_take_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, row, G, nq, k, cand_rows, cand_cnt);
}

void launch_group_emit(const uint32_t* cand_rows, const uint32_t* cand_cnt, const double* cand_score, const uint32_t* grp,
                       const int32_t* label_of_group, int32_t nq, int32_t k, int64_t row_offset, int64_t* out_idx, float* out_sc,
                       int32_t* out_lab, hipStream_t stream) {
  const int64_t total = (int64_t)nq * k;
  if (total <= 0) return;
  hipLaunchKernelGGL(group_emit_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, cand_rows, cand_cnt, cand_score,
                     grp, label_of_group, nq, k, row_offset, out_idx, out_sc, out_lab);
}

}  // namespace mi
