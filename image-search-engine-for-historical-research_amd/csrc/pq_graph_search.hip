// Best-first search of a neighbour graph over the CODES of a PQ index (mi_pq_graph; the role of the reference's PQ + HNSW
// matchers): the scorer of graph_walk.h for PQ codes.  (The decoder that gives the build its queries is pq.hip's.)
//
// What differs from graph_search.hip is what a row costs.  There a row is an 8 KiB gather by a whole wave; here it is
// ceil(M / 4) dwords read by ONE lane and M reads of the query's distance table, which the kernel copies to LDS before the walk
// ([M][Ks], made by pq_table_kernel: the bits of mi_pq_dtable; in pq_adc_row's image, 4 MQ books) and which stays there for the
// whole search.  Lane t of wave 0 evaluates new row t: pq_adc_row, float32 adds in ascending book order, the bits of
// mi_pq_search.  The codes lie in the index's transposed blocks [block][MQ][64], so a row's code is MQ dwords 256 bytes apart and
// a dword is the widest load that layout has; the 64 lanes of a block read 64 consecutive dwords.
// A place of W is ONE 64-bit word: pq_key(distance, row) -- float bits above, the 31-bit local row below -- with the `expanded`
// mark in bit 31 of the low word, masked out of every comparison.  Distances are >= +0.0 or +inf, so the integer order of the
// masked keys IS (distance asc, id asc), and keys of distinct rows are distinct: no tie class.
//
// Dynamic LDS, in bytes (pq_graph_lds_bytes): table 16 MQ Ks (at most 65536) | W 8 ef | other half 8 ef | new keys as evaluated
// 512 | new keys in the order 512 | table entries as read 256 | new ids 256 | control 16.  The largest carve the contract admits
// (M = 64, Ks = 256, ef = 2048) is 65536 + 32768 + 1552 = 99856 bytes of the 160 KiB of a CU.
#include "graph_walk.h"
#include "kernels.h"
#include "pq_device.h"

namespace mi {

constexpr uint64_t PG_EXPANDED = 0x80000000ull;

struct PgCodes {
  typedef uint64_t Place;
  struct List {
    uint64_t* k;
    __device__ __forceinline__ Place load(int j) const { return k[j]; }
    __device__ __forceinline__ void store(int j, Place p) const { k[j] = p; }
    __device__ __forceinline__ void mark(int j, Place) const { k[j] |= PG_EXPANDED; }
  };
  static __device__ __forceinline__ Place bare(Place p) { return p & ~PG_EXPANDED; }
  static __device__ __forceinline__ bool before(Place a, Place b) { return a < b; }
  static __device__ __forceinline__ bool expanded(Place p) { return p & PG_EXPANDED; }
  static __device__ __forceinline__ uint32_t row(Place p) { return (uint32_t)p & 0x7fffffffu; }

  List w, w2, nw, sn;
  uint32_t *n_id, *s_raw, *s_ctl;
  const float* tl;                 // the query's table in LDS
  const uint32_t* codes;
  int32_t MQ, Ks;
  int64_t row_offset;
  int64_t* out_idx;
  float* out_dist;

  // behind the table
  __device__ __forceinline__ void carve(char* smem, int ef) {
    w.k = reinterpret_cast<uint64_t*>(smem);
    w2.k = w.k + ef;
    nw.k = w2.k + ef;
    sn.k = nw.k + 64;
    s_raw = reinterpret_cast<uint32_t*>(sn.k + 64);
    n_id = s_raw + 64;
    s_ctl = n_id + 64;
  }
  // one lane per new row
  __device__ __forceinline__ void evaluate(int m, int t) const {
    if (t < m) {
      const uint32_t r = n_id[t];
      const uint32_t* src = codes + (int64_t)(r >> 6) * MQ * 64 + (r & 63u);
      nw.k[t] = pq_key(pq_adc_row<1>(tl, src, MQ, Ks).v[0], r);
    }
  }
  __device__ __forceinline__ void emit(int64_t o, int i, bool have) const {
    int64_t id = -1;
    float v = INFINITY;
    if (have) {
      id = row_offset + (int64_t)row(w.k[i]);
      v = pq_key_dist(w.k[i]);
    }
    out_idx[o] = id;
    if (out_dist) out_dist[o] = v;
  }
};

// codes [ceil(cap / 64)][MQ][64]; tab [gridDim.x][real = M Ks]; adj, entries, vis as graph_walk takes them; dynamic LDS:
// pq_graph_lds_bytes(MQ, Ks, ef)
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
  PgCodes p;
  p.carve(reinterpret_cast<char*>(tl + ent), ef);
  p.tl = tl, p.codes = codes, p.MQ = MQ, p.Ks = Ks, p.row_offset = row_offset, p.out_idx = out_idx, p.out_dist = out_dist;
  // the table; the walk's first barrier stands between this copy and its first reader
  pq_slab_load_table<256>(tl, tab + (int64_t)blockIdx.x * real, ent, real, threadIdx.x);
  graph_walk(p, n, adj, R, entries, ne, k, ef, vis, vis_words, out_visited);
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

}  // namespace mi
