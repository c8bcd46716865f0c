// Best-first search of a neighbour graph over the CODES of a PQ index (mi_pq_graph; the role of the reference's PQ + HNSW
// matchers), and the decoder that gives the build its queries.
//
// The traversal is graph_search.hip's, step for step; what differs is what a row costs.  There a row is an 8 KiB gather by a
// whole wave; here it is ceil(M / 4) dwords read by ONE lane and M reads of the query's distance table, which stays in LDS for
// the whole search.  One workgroup of four waves per query:
//   0. the query's table [M][Ks] (made by pq_table_kernel: the bits of mi_pq_dtable) -> LDS in pq_adc_row's image, 4 MQ books;
//   1. every thread scans its share of W for the first place not yet expanded, one LDS atomicMin picks the first of all;
//   2. wave 0 reads that row's R table entries, drops -1s, ids outside [0, n), repeats within the row (compared in LDS) and rows
//      whose bit in the query's visited bitmap is set (exact: n bits per query in HBM, atomicOr because two lanes may share a
//      word; the bitmap belongs to this workgroup alone), and compacts the rest by a ballot;
//   3. lane t of wave 0 evaluates new row t: pq_adc_row, float32 adds in ascending book order, the bits of mi_pq_search.  The
//      codes lie in the index's transposed blocks [block][MQ][64], so a row's code is MQ dwords 256 bytes apart and a dword is
//      the widest load that layout has; the 64 lanes of a block read 64 consecutive dwords;
//   4. the up to 64 new rows are ordered by rank among themselves;
//   5. W and the new rows merge by rank into the other half of the double buffer; places >= ef fall off (and stay visited).
// A place of W is ONE 64-bit word: pq_key(distance, row) -- float bits above, the 31-bit local row below -- with the `expanded`
// mark in bit 31 of the low word, masked out of every comparison.  Distances are >= +0.0 or +inf, so the integer order of the
// masked keys IS (distance asc, id asc), and keys of distinct rows are distinct: no tie class.
//
// Workgroup size.  Steps 2 to 4 are one wave's work (at most 64 rows).  The other three waves are kept for steps 0, 1 and 5: the
// table copy (up to 16384 floats), the scan of W and above all the merge, which at ef = 2048 is 2048 binary searches per step
// -- 8 per thread with 256 threads, 32 with 64.  At small ef they idle at the barriers, which costs little: the workgroup is
// LDS-bound to one or two per CU either way.
//
// Dynamic LDS, in bytes (pq_graph_lds_bytes): table 16 MQ Ks (at most 65536) | W 8 ef | other half 8 ef | new keys as evaluated
// 512 | new keys in the order 512 | table entries as read 256 | new ids 256 | control 16.  The largest carve the contract admits
// (M = 64, Ks = 256, ef = 2048) is 65536 + 32768 + 1552 = 99856 bytes of the 160 KiB of a CU.
// No atomics across workgroups, no grid barrier; results leave by ordinary vector stores.
#include <algorithm>

#include "kernels.h"
#include "pq_device.h"

namespace mi {

constexpr uint64_t PG_EXPANDED = 0x80000000ull;
constexpr uint32_t PG_NONE = 0xffffffffu;

__device__ __forceinline__ uint64_t pg_bare(uint64_t key) { return key & ~PG_EXPANDED; }

// number of places of the sorted list keys[0, len) that come before `key` (a bare key)
__device__ __forceinline__ int pg_rank(const uint64_t* keys, int len, uint64_t key) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pg_bare(keys[mid]) < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// codes [ceil(cap / 64)][MQ][64]; tab [gridDim.x][real = M Ks]; adj [n][R]; entries [ne]; vis [gridDim.x][vis_words], all zero
// on entry (the caller clears it before every launch); dynamic LDS: pq_graph_lds_bytes(MQ, Ks, ef)
__global__ __launch_bounds__(256) void pq_graph_search_kernel(const uint32_t* __restrict__ codes, int32_t MQ, int32_t Ks, int32_t real,
                                                              const float* __restrict__ tab, int64_t n, int64_t row_offset,
                                                              const int32_t* __restrict__ adj, int32_t R,
                                                              const int32_t* __restrict__ entries, int32_t ne, int32_t k, int32_t ef,
                                                              uint32_t* __restrict__ vis, int64_t vis_words,
                                                              int64_t* __restrict__ out_idx, float* __restrict__ out_dist,
                                                              int32_t* __restrict__ out_visited) {
  extern __shared__ __attribute__((aligned(16))) char pg_smem[];
  const int32_t ent = 4 * MQ * Ks;
  float* tl = reinterpret_cast<float*>(pg_smem);
  uint64_t* wk = reinterpret_cast<uint64_t*>(tl + ent);   // W; wk2 is the half the next merge writes
  uint64_t* wk2 = wk + ef;
  uint64_t* n_key = wk2 + ef;                          // new rows as evaluated
  uint64_t* s_key = n_key + 64;                        // new rows in the order
  uint32_t* s_raw = reinterpret_cast<uint32_t*>(s_key + 64);   // the table entries of the expanded row as read
  uint32_t* n_id = s_raw + 64;                         // new rows, compacted
  uint32_t* s_ctl = n_id + 64;                         // [0] first unexpanded place, [1] number of new rows

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t q = blockIdx.x;
  uint32_t* myvis = vis + q * vis_words;
  int wn = 0;
  int64_t visited = 0;

  // ---- start: the table, and the distinct entry rows as the first batch of new rows, none of them expanded
  pq_slab_load_table<256>(tl, tab + q * real, ent, real, t);
  if (wv == 0) {
    const int32_t e = lane < ne ? entries[lane] : -1;
    s_raw[lane] = (uint32_t)e;
  }
  __syncthreads();
  for (int64_t step = -1; step < n; ++step) {
    if (step >= 0) {
      // 1. the first place of W that is not yet expanded
      if (t == 0) s_ctl[0] = PG_NONE;
      __syncthreads();
      for (int i = t; i < wn; i += 256)
        if (!(wk[i] & PG_EXPANDED)) {
          atomicMin(&s_ctl[0], (uint32_t)i);
          break;
        }
      __syncthreads();
      const uint32_t first = s_ctl[0];
      if (first == PG_NONE) break;                     // (uniform: every thread reads the same word)
      const uint32_t row = (uint32_t)wk[first] & 0x7fffffffu;
      if (wv == 0) s_raw[lane] = lane < R ? (uint32_t)adj[(int64_t)row * R + lane] : PG_NONE;
      __syncthreads();
      if (t == 0) wk[first] |= PG_EXPANDED;
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
    if (m == 0) continue;                              // (uniform)
    // 3. one lane per new row
    if (t < m) {
      const uint32_t row = n_id[t];
      const uint32_t* src = codes + (int64_t)(row >> 6) * MQ * 64 + (row & 63u);
      n_key[t] = pq_key(pq_adc_row<1>(tl, src, MQ, Ks).v[0], row);
    }
    __syncthreads();
    // 4. the new rows in the order (their keys are distinct)
    if (t < m) {
      const uint64_t key = n_key[t];
      int r = 0;
      for (int j = 0; j < m; ++j) r += n_key[j] < key ? 1 : 0;
      s_key[r] = key;
    }
    __syncthreads();
    // 5. merge by rank into the other half; what lands at ef or beyond is pushed out (and stays visited)
    for (int i = t; i < wn; i += 256) {
      const uint64_t key = wk[i];
      const int p = i + pg_rank(s_key, m, pg_bare(key));
      if (p < ef) wk2[p] = key;
    }
    if (t < m) {
      const uint64_t key = s_key[t];
      const int p = t + pg_rank(wk, wn, key);
      if (p < ef) wk2[p] = key;
    }
    wn = min(wn + m, ef);
    {
      uint64_t* tk = wk;
      wk = wk2, wk2 = tk;
    }
    __syncthreads();
  }

  // ---- answer: the first k places of W
  for (int i = t; i < k; i += 256) {
    int64_t id = -1;
    float v = INFINITY;
    if (i < wn) {
      id = row_offset + (int64_t)(pq_key_row(wk[i]) & 0x7fffffffu);
      v = pq_key_dist(wk[i]);
    }
    out_idx[q * k + i] = id;
    if (out_dist) out_dist[q * k + i] = v;
  }
  if (out_visited && t == 0) out_visited[q] = (int32_t)visited;
}

// out [nrows][M L]: row row0 + r reconstructed, the concatenation of C[j][code[j]] (nanopq's pq.decode)
__global__ __launch_bounds__(256) void pq_decode_kernel(const uint32_t* __restrict__ codes, int32_t M, int32_t Ks, int32_t L,
                                                       const float* __restrict__ cb, int64_t row0, int64_t nrows,
                                                       float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int32_t d = M * L, MQ = (M + 3) / 4;
  if (i >= nrows * d) return;
  const int64_t row = row0 + i / d;
  const int32_t col = (int32_t)(i % d), j = col / L;
  const uint32_t g = codes[((row >> 6) * MQ + (j >> 2)) * 64 + (row & 63)];
  const int32_t c = (int32_t)((g >> (8 * (j & 3))) & 255u);
  out[i] = cb[((int64_t)j * Ks + c) * L + (col - j * L)];
}

size_t pq_graph_lds_bytes(int32_t M, int32_t Ks, int32_t ef) {
  const size_t MQ = ((size_t)M + 3) / 4;
  return 16 * MQ * (size_t)Ks + 2 * 8 * (size_t)ef + 2 * 64 * 8 + 2 * 64 * 4 + 16;
}

void launch_pq_graph_search(const uint32_t* codes, int32_t M, int32_t Ks, const float* tab, int64_t n, int64_t row_offset,
                            const int32_t* adj, int32_t R, const int32_t* entries, int32_t ne, int32_t k, int32_t ef, int64_t nq,
                            uint32_t* vis, int64_t vis_words, int64_t* out_idx, float* out_dist, int32_t* out_visited,
                            hipStream_t stream) {
  if (nq <= 0) return;
  ensure_dynamic_lds((const void*)pq_graph_search_kernel);     // beyond 64 KiB from M Ks = 4096 entries and ef = 2048 on
  hipLaunchKernelGGL(pq_graph_search_kernel, dim3((unsigned)nq), dim3(256), pq_graph_lds_bytes(M, Ks, ef), stream, codes,
                     (M + 3) / 4, Ks, M * Ks, tab, n, row_offset, adj, R, entries, ne, k, ef, vis, vis_words, out_idx, out_dist,
                     out_visited);
}

void launch_pq_decode(const uint32_t* codes, int32_t M, int32_t Ks, int32_t L, const float* cb, int64_t row0, int64_t nrows, float* out,
                      hipStream_t stream) {
  const int64_t d = (int64_t)M * L;
  const int64_t step = std::max<int64_t>(1, ((int64_t)1 << 30) / d);         // rows per launch
  for (int64_t r = 0; r < nrows; r += step) {
    const int64_t b = std::min(step, nrows - r);
    pq_decode_kernel<<<dim3((unsigned)((b * d + 255) / 256)), 256, 0, stream>>>(codes, M, Ks, L, cb, row0 + r, b, out + r * d);
  }
}

}  // namespace mi
