// Best-first search of a neighbour graph over the stored f32 rows (the role of HNSW's bottom layer).
//
// One workgroup of four waves per query.  W, the best `ef` rows seen so far, lives in LDS as two arrays sorted by the ORDER
// (l2_dist_key of the value ascending, id ascending): a 64-bit key and a 32-bit word holding the local row with the `expanded`
// mark in bit 31.  One step:
//   1. every thread scans its share of W for the first row not yet expanded, one LDS atomicMin picks the first of all;
//   2. wave 0 reads that row's R table entries, drops -1s, ids outside [0, n), repeats within the row (compared in LDS) and rows
//      whose bit in the query's visited bitmap is already set (the bitmap is exact: n bits per query in HBM, set with atomicOr
//      so that two lanes of the wave may share a word), and compacts the rest by a ballot;
//   3. the four waves take the new rows in turn, one wave per row: l2_direct_wave / refine_dot_wave, the bits of mi_refine;
//   4. the up to 64 new rows are ordered by rank (each thread counts the rows before its own);
//   5. W and the new rows merge by rank into the other half of the double buffer: an element's place is its own index plus the
//      number of elements of the other list before it, found by binary search -- no serial insertion; places >= ef fall off.
// The loop ends when step 1 finds nothing, and after n expansions at the latest whatever the table holds.  No atomics across
// workgroups, no grid barrier.  The query row is read from global memory (every wave re-reads it per row: it stays in L1 / L2).
#include "common.h"
#include "kernels.h"
#include "l2_wave.h"

namespace mi {

constexpr uint32_t GS_EXPANDED = 0x80000000u, GS_NONE = 0xffffffffu;

// (key, id) before (okey, oid) in the order; ids are distinct wherever this is asked
__device__ __forceinline__ bool gs_before(uint64_t key, uint32_t id, uint64_t okey, uint32_t oid) {
  return key != okey ? key < okey : id < oid;
}

// number of elements of the sorted list (keys, ids)[0, len) that come before (key, id)
__device__ __forceinline__ int gs_rank(const uint64_t* keys, const uint32_t* ids, int len, uint64_t key, uint32_t id) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (gs_before(keys[mid], ids[mid] & ~GS_EXPANDED, key, id)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the value behind an l2_dist_key (NaN for the key of a NaN)
__device__ __forceinline__ double gs_key_value(uint64_t key) {
  const uint64_t u = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  return __longlong_as_double((long long)u);
}

// qry [nq][dp] (16-byte aligned rows, d columns used); adj [n][R]; entries [ne]; vis [gridDim.x][vis_words], all zero on entry
// (the caller clears it before every launch); dynamic LDS: graph_search_lds_bytes(ef), 24 bytes per place of W (two halves) + 1808.
template <bool L2>
__global__ __launch_bounds__(256) void graph_search_kernel(const float* __restrict__ gal_f32, const float* __restrict__ qry,
                                                           int32_t dp, int32_t d, int64_t n, int64_t row_offset,
                                                           const int32_t* __restrict__ adj, int32_t R,
                                                           const int32_t* __restrict__ entries, int32_t ne, int32_t k, int32_t ef,
                                                           uint32_t* __restrict__ vis, int64_t vis_words,
                                                           int64_t* __restrict__ out_idx, float* __restrict__ out_val,
                                                           double* __restrict__ out_val64, int32_t* __restrict__ out_visited) {
  extern __shared__ __attribute__((aligned(16))) char gs_smem[];
  const int efp = (ef + 3) & ~3;
  uint64_t* wk = reinterpret_cast<uint64_t*>(gs_smem);   // W; (wk2, wi2) is the half the next merge writes
  uint64_t* wk2 = wk + efp;
  uint64_t* n_key = wk2 + efp;                        // new rows as evaluated
  uint64_t* s_key = n_key + 64;                       // new rows in the order
  uint32_t* wi = reinterpret_cast<uint32_t*>(s_key + 64);
  uint32_t* wi2 = wi + efp;
  uint32_t* n_id = wi2 + efp;
  uint32_t* s_id = n_id + 64;
  uint32_t* s_raw = s_id + 64;                        // the table entries of the expanded row as read
  uint32_t* s_ctl = s_raw + 64;                       // [0] first unexpanded place, [1] number of new rows

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t q = blockIdx.x;
  const float* qrow = qry + q * dp;
  uint32_t* myvis = vis + q * vis_words;
  int wn = 0;
  int64_t visited = 0;

  // ---- start: the distinct entry rows are the first batch of new rows, none of them expanded
  if (wv == 0) {
    const int32_t e = lane < ne ? entries[lane] : -1;
    s_raw[lane] = (uint32_t)e;
  }
  __syncthreads();
  for (int64_t step = -1; step < n; ++step) {
    if (step >= 0) {
      // 1. the first row of W that is not yet expanded
      if (t == 0) s_ctl[0] = GS_NONE;
      __syncthreads();
      for (int i = t; i < wn; i += 256)
        if (!(wi[i] & GS_EXPANDED)) {
          atomicMin(&s_ctl[0], (uint32_t)i);
          break;
        }
      __syncthreads();
      const uint32_t first = s_ctl[0];
      if (first == GS_NONE) break;                    // (uniform: every thread reads the same word)
      const uint32_t row = wi[first];
      if (wv == 0) s_raw[lane] = lane < R ? (uint32_t)adj[(int64_t)row * R + lane] : GS_NONE;
      __syncthreads();
      if (t == 0) wi[first] = row | GS_EXPANDED;
    }
    // 2. wave 0: valid, first occurrence within the row, not visited -> n_id[0, m)
    if (wv == 0) {
      const int cnt = step < 0 ? ne : R;
      const uint32_t c = s_raw[lane];
      bool keep = lane < cnt && (int32_t)c >= 0 && (int64_t)c < n;
      if (keep)
        for (int j = 0; j < lane; ++j)
          if (s_raw[j] == c) {
            keep = false;
            break;
          }
      if (keep) {
        const uint32_t bit = 1u << (c & 31);
        keep = (atomicOr(&myvis[c >> 5], bit) & bit) == 0;
      }
      const unsigned long long m = __ballot(keep);
      if (keep) n_id[__popcll(m & ((1ull << lane) - 1))] = c;
      if (lane == 0) s_ctl[1] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    const int m = (int)s_ctl[1];
    visited += m;
    if (m == 0) continue;                             // (uniform)
    // 3. one wave per new row
    for (int i = wv; i < m; i += 4) {
      const float* grow = gal_f32 + (int64_t)n_id[i] * dp;
      const double v = L2 ? l2_direct_wave(qrow, grow, d, lane) : refine_dot_wave(qrow, grow, d, lane);
      if (lane == 0) n_key[i] = l2_dist_key(L2 ? v : 0.0 - v);
    }
    __syncthreads();
    // 4. the new rows in the order (their ids are distinct)
    if (t < m) {
      const uint64_t key = n_key[t];
      const uint32_t id = n_id[t];
      int r = 0;
      for (int j = 0; j < m; ++j) r += gs_before(n_key[j], n_id[j], key, id) ? 1 : 0;
      s_key[r] = key;
      s_id[r] = id;
    }
    __syncthreads();
    // 5. merge by rank into the other buffer; what lands at ef or beyond is pushed out (and stays visited)
    for (int i = t; i < wn; i += 256) {
      const uint64_t key = wk[i];
      const uint32_t idw = wi[i];
      const int p = i + gs_rank(s_key, s_id, m, key, idw & ~GS_EXPANDED);
      if (p < ef) {
        wk2[p] = key;
        wi2[p] = idw;
      }
    }
    if (t < m) {
      const uint64_t key = s_key[t];
      const uint32_t id = s_id[t];
      const int p = t + gs_rank(wk, wi, wn, key, id);
      if (p < ef) {
        wk2[p] = key;
        wi2[p] = id;
      }
    }
    wn = min(wn + m, ef);
    {
      uint64_t* tk = wk;
      wk = wk2, wk2 = tk;
      uint32_t* ti = wi;
      wi = wi2, wi2 = ti;
    }
    __syncthreads();
  }

  // ---- answer: the first k rows of W
  const double padv = L2 ? (double)INFINITY : -(double)INFINITY;
  for (int i = t; i < k; i += 256) {
    int64_t id = -1;
    double v = padv;
    if (i < wn) {
      id = row_offset + (int64_t)(wi[i] & ~GS_EXPANDED);
      const double dec = gs_key_value(wk[i]);
      v = L2 ? dec : 0.0 - dec;
    }
    out_idx[q * k + i] = id;
    if (out_val64) out_val64[q * k + i] = v;
    if (out_val) out_val[q * k + i] = (float)v;
  }
  if (out_visited && t == 0) out_visited[q] = (int32_t)visited;
}

size_t graph_search_lds_bytes(int32_t ef) {
  const size_t efp = ((size_t)ef + 3) & ~(size_t)3;
  return 2 * efp * 12 + 64 * 24 + 64 * 4 + 16;
}

void launch_graph_search(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int64_t row_offset, int l2,
                         const int32_t* adj, int32_t R, const int32_t* entries, int32_t ne, int32_t k, int32_t ef, int64_t nq,
                         uint32_t* vis, int64_t vis_words, int64_t* out_idx, float* out_val, double* out_val64,
                         int32_t* out_visited, hipStream_t stream) {
  if (nq <= 0) return;
  const size_t lds = graph_search_lds_bytes(ef);
  if (l2)
    hipLaunchKernelGGL(graph_search_kernel<true>, dim3((unsigned)nq), dim3(256), lds, stream, gal_f32, qry, dp, d, n, row_offset,
                       adj, R, entries, ne, k, ef, vis, vis_words, out_idx, out_val, out_val64, out_visited);
  else
    hipLaunchKernelGGL(graph_search_kernel<false>, dim3((unsigned)nq), dim3(256), lds, stream, gal_f32, qry, dp, d, n, row_offset,
                       adj, R, entries, ne, k, ef, vis, vis_words, out_idx, out_val, out_val64, out_visited);
}

}  // namespace mi
