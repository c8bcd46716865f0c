// Best-first search of a neighbour graph over the stored f32 rows (the role of HNSW's bottom layer): the scorer
// of graph_walk.h for raw rows.  A place of W is a 64-bit key (f64_key_nan_highest of the value, so ascending = best first) and a 32-bit
// word holding the local row with the `expanded` mark in bit 31; the order is (key ascending, id ascending).  A new row is
// evaluated by a whole wave, the four waves taking the rows in turn: l2_direct_wave / refine_dot_wave, the bits of mi_refine.  The
// query row is read from global memory (every wave re-reads it per row: it stays in L1 / L2).
#include "common.h"
#include "graph_walk.h"
#include "kernels.h"
#include "l2_wave.h"

namespace mi {

constexpr uint32_t GS_EXPANDED = 0x80000000u;

template <bool L2>
struct GsRows {
  struct Place { uint64_t key; uint32_t id; };
  struct List {
    uint64_t* k; uint32_t* i;
    __device__ __forceinline__ Place load(int j) const { return {k[j], i[j]}; }
    __device__ __forceinline__ void store(int j, Place p) const { k[j] = p.key, i[j] = p.id; }
    __device__ __forceinline__ void mark(int j, Place p) const { i[j] = p.id | GS_EXPANDED; }
  };
  static __device__ __forceinline__ Place bare(Place p) { return {p.key, p.id & ~GS_EXPANDED}; }
  // ids are distinct wherever this is asked
  static __device__ __forceinline__ bool before(Place a, Place b) { return a.key != b.key ? a.key < b.key : a.id < b.id; }
  static __device__ __forceinline__ bool expanded(Place p) { return p.id & GS_EXPANDED; }
  static __device__ __forceinline__ uint32_t row(Place p) { return p.id; }

  List w, w2, nw, sn;
  uint32_t *n_id, *s_raw, *s_ctl;
  const float *gal_f32, *qrow;
  int32_t dp, d;
  int64_t row_offset;
  int64_t* out_idx;
  float* out_val;
  double* out_val64;

  // 24 bytes per place of W (two halves) + 1808: graph_search_lds_bytes(ef)
  __device__ __forceinline__ void carve(char* smem, int ef) {
    const int efp = (ef + 3) & ~3;
    w.k = reinterpret_cast<uint64_t*>(smem);
    w2.k = w.k + efp;
    nw.k = w2.k + efp;
    sn.k = nw.k + 64;
    w.i = reinterpret_cast<uint32_t*>(sn.k + 64);
    w2.i = w.i + efp;
    nw.i = n_id = w2.i + efp;
    sn.i = nw.i + 64;
    s_raw = sn.i + 64;
    s_ctl = s_raw + 64;
  }
  // one wave per new row
  __device__ __forceinline__ void evaluate(int m, int t) const {
    const int lane = t & 63;
    for (int i = t >> 6; i < m; i += 4) {
      const float* grow = gal_f32 + (int64_t)n_id[i] * dp;
      const double v = L2 ? l2_direct_wave(qrow, grow, d, lane) : refine_dot_wave(qrow, grow, d, lane);
      if (lane == 0) nw.k[i] = f64_key_nan_highest(L2 ? v : 0.0 - v);
    }
  }
  __device__ __forceinline__ void emit(int64_t o, int i, bool have) const {
    int64_t id = -1;
    double v = L2 ? (double)INFINITY : -(double)INFINITY;
    if (have) {
      const Place p = bare(w.load(i));
      id = row_offset + (int64_t)p.id;
      const double dec = f64_key_value(p.key);
      v = L2 ? dec : 0.0 - dec;
    }
    out_idx[o] = id;
    if (out_val64) out_val64[o] = v;
    if (out_val) out_val[o] = (float)v;
  }
};

// qry [nq][dp] (16-byte aligned rows, d columns used); adj, entries, vis as graph_walk takes them; dynamic LDS:
// graph_search_lds_bytes(ef)
template <bool L2>
__global__ __launch_bounds__(256) void graph_search_kernel(const float* __restrict__ gal_f32, const float* __restrict__ qry,
                                                           int32_t dp, int32_t d, int64_t n, int64_t row_offset,
                                                           const int32_t* __restrict__ adj, int32_t R,
                                                           const int32_t* __restrict__ entries, int32_t ne, int32_t k, int32_t ef,
                                                           uint32_t* __restrict__ vis, int64_t vis_words,
                                                           int64_t* __restrict__ out_idx, float* __restrict__ out_val,
                                                           double* __restrict__ out_val64, int32_t* __restrict__ out_visited) {
  extern __shared__ __attribute__((aligned(16))) char gs_smem[];
  GsRows<L2> p;
  p.carve(gs_smem, ef);
  p.gal_f32 = gal_f32, p.qrow = qry + (int64_t)blockIdx.x * dp, p.dp = dp, p.d = d, p.row_offset = row_offset;
  p.out_idx = out_idx, p.out_val = out_val, p.out_val64 = out_val64;
  graph_walk(p, n, adj, R, entries, ne, k, ef, vis, vis_words, out_visited);
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
