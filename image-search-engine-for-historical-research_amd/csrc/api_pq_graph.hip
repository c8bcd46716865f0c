// Graph index over the codes of a PQ index (mi_pq_graph*; the role of the reference's PQ + HNSW matchers).  DESIGN.md 5.16b.
// The handle holds a neighbour table int32 [n][R] and up to 64 entry rows on the device, plus the workspace of its searches (the
// queries' distance tables, the visited bitmaps, the staging of a host call); codes, codebooks and the stream of the host entry
// points are the PQ index's.  Kernels: pq_graph_search.hip (one workgroup per query, the table of the query in LDS, one lane per
// evaluated row), pq.hip's table kernel, graph_build.hip (table from exact nearest-neighbour lists); the lists themselves are
// mi_pq_search_device's answers to the decoded rows.
#include "api_internal.h"

struct mi_pq_graph {
  mi_pq* codes = nullptr;
  int device = 0;
  uint64_t mod = 0;                    // table.n and the modification count of the PQ index when the table was made: a search
                                       // refuses any other pair
  DeviceBufSet bufs;                   // every device allocation of the handle: hbm_bytes is bufs.bytes()
  GraphTable table{&bufs};
  // grow-only workspace of the searches
  DeviceBuf<char> qraw{bufs};          // queries of a host call, packed [nq][d] in their own type
  DeviceBuf<float> tab{bufs};          // [queries of a chunk][m][ks] distance tables
  DeviceBuf<uint32_t> vis{bufs};       // [queries of a chunk][ceil(n / 32)] visited bitmaps
  DeviceBuf<int64_t> oidx{bufs};       // results of a host call
  DeviceBuf<float> odist{bufs};
  DeviceBuf<int32_t> ovis{bufs};
  std::mutex mu;
  explicit mi_pq_graph(mi_pq* h) : codes(h), device(h->device), mod(h->mod) {}      // (the caller holds h's lock)
};

// bytes of distance tables one launch may use: a batch that needs more is searched in chunks of queries
constexpr size_t PQ_GRAPH_TAB_BYTES = (size_t)256 << 20;

static int pq_graph_fresh(const mi_pq_graph* gr) {
  REQUIRE(gr->codes->n == gr->table.n && gr->codes->mod == gr->mod,
          "the PQ index has had rows added or removed since the graph was made: build a new graph");
  return MI_OK;
}

// tables of the queries at `src` (device memory, any strides) in gr->tab, then one launch per chunk of queries, all on `s`
static int pq_graph_enqueue(mi_pq_graph* gr, const void* src, int dtype, int64_t rs, int64_t cs, int64_t nq, int32_t k, int32_t ef,
                            int64_t* out_idx, float* out_dist, int32_t* out_visited, hipStream_t s) {
  mi_pq* h = gr->codes;
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  const GraphTable& t = gr->table;
  const auto [words, by_vis] = graph_vis_chunks(t.n, nq);
  const int64_t per = (int64_t)h->m * h->ks, chunk = std::max<int64_t>(1, std::min<int64_t>(by_vis, (int64_t)(PQ_GRAPH_TAB_BYTES / 4) / per));
  int rc;
  if ((rc = gr->vis.grow((size_t)chunk * words)) != MI_OK) return rc;
  if ((rc = gr->tab.grow((size_t)chunk * per)) != MI_OK) return rc;
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t b = std::min<int64_t>(chunk, nq - q0);
    launch_pq_table((const char*)src + (size_t)q0 * rs * esz, dtype, rs, cs, b, h->cb, h->m, h->ks, h->L, gr->tab, s);
    HIPC(hipMemsetAsync(gr->vis, 0, (size_t)b * words * 4, s));
    launch_pq_graph_search(h->codes, h->m, h->ks, gr->tab, t.n, h->row_offset, t.adj, t.R, t.entries, t.ne, k, ef, b, gr->vis,
                           words, out_idx + q0 * k, out_dist ? out_dist + q0 * k : nullptr, out_visited ? out_visited + q0 : nullptr, s);
  }
  HIPC(hipGetLastError());
  return MI_OK;
}

extern "C" {

int mi_pq_graph_create(mi_pq* codes, const int32_t* neighbors, int32_t R, int neighbors_memspace, const int32_t* entries, int32_t ne,
                       mi_pq_graph** out) {
  int rc = graph_create_check(codes, neighbors, R, neighbors_memspace, entries, ne, out);
  if (rc != MI_OK) return rc;
  std::lock_guard<std::mutex> lock(codes->mu);
  REQUIRE(codes->n >= 1, "the PQ index holds no rows");
  mi_pq_graph* gr = new mi_pq_graph(codes);
  if ((rc = graph_table_from_neighbors(gr->table, codes->n, codes->device, "PQ graph", neighbors, R, neighbors_memspace, entries, ne)) !=
      MI_OK) {
    delete gr;
    return rc;
  }
  *out = gr;
  return MI_OK;
}

int mi_pq_graph_build(mi_pq* codes, int32_t R, int32_t ne, mi_pq_graph** out) {
  int rc = graph_build_check(codes, R, ne, out);
  if (rc != MI_OK) return rc;
  mi_pq* h = codes;
  std::lock_guard<std::mutex> lock(h->mu);
  const int64_t n = h->n;
  if ((rc = graph_build_rows_check(n)) != MI_OK) return rc;
  HIPC(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int32_t ks = (int32_t)std::min<int64_t>(R + 1, n);
  mi_pq_graph* gr = new mi_pq_graph(h);
  if ((rc = graph_table_alloc(gr->table, n, R, (int32_t)std::min<int64_t>(ne, n), "PQ graph")) != MI_OK) {
    delete gr;
    return rc;
  }
  auto bail = [&](int code) {
    (void)hipStreamSynchronize(s);
    delete gr;
    return code;
  };
  TmpAlloc tmp;                                   // (freed on return; every path out of here has synchronised `s`)
  const int64_t bmax = std::min<int64_t>(GRAPH_BUILD_BATCH, n);
  const GraphBuildWs ws = graph_build_workspace(tmp, n, R);
  int64_t* ids = tmp.get<int64_t>((size_t)bmax * ks);
  float* rec = tmp.get<float>((size_t)bmax * h->d);
  if (!ws.F || !ws.B || !ws.cnt || !ws.off || !ids || !rec) return bail(fail(MI_ERR_NOMEM, "PQ graph build workspace"));
  // forward lists: every stored row's reconstruction is a query of the exhaustive ADC search, whose answer is already in the
  // graph's order (distance asc, id asc)
  for (int64_t r0 = 0; r0 < n; r0 += bmax) {
    const int64_t b = std::min<int64_t>(bmax, n - r0);
    launch_pq_decode(h->codes, 1, h->m, h->ks, h->L, h->cb, r0, b, rec, s);
    if ((rc = pq_search_core(h, rec, MI_F32, h->d, 1, b, ks, nullptr, ids, nullptr, s)) != MI_OK) return bail(rc);
    launch_graph_forward(ids, ks, r0, b, h->row_offset, n, R, ws.F, s);
    hipError_t e = hipStreamSynchronize(s);        // (rec / ids are reused by the next batch)
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return bail(fail(MI_ERR_HIP, std::string("PQ graph build: ") + hipGetErrorString(e)));
  }
  if ((rc = graph_table_finish(gr->table, ws, tmp, "PQ graph", s)) != MI_OK) return bail(rc);
  *out = gr;
  return MI_OK;
}

int mi_pq_graph_info(const mi_pq_graph* gr, int64_t* n, int32_t* R, int32_t* ne, int64_t* hbm_bytes) {
  REQUIRE(gr, "null handle");
  if (n) *n = gr->table.n;
  if (R) *R = gr->table.R;
  if (ne) *ne = gr->table.ne;
  if (hbm_bytes) *hbm_bytes = (int64_t)gr->bufs.bytes();
  return MI_OK;
}

int mi_pq_graph_get_neighbors(mi_pq_graph* gr, int64_t row0, int64_t nrows, int32_t* out_host) {
  REQUIRE(gr, "null handle");
  return graph_table_get_neighbors(gr->table, gr->mu, gr->device, row0, nrows, out_host);
}

int mi_pq_graph_get_entries(mi_pq_graph* gr, int32_t* out_host) {
  REQUIRE(gr, "null handle");
  return graph_table_get_entries(gr->table, gr->mu, gr->device, out_host);
}

int mi_pq_graph_destroy(mi_pq_graph* gr) {
  if (!gr) return MI_OK;
  (void)hipSetDevice(gr->device);
  (void)hipDeviceSynchronize();
  delete gr;
  return MI_OK;
}

int mi_pq_graph_search_device(mi_pq_graph* gr, const float* q_dev, int64_t nq, int32_t k, int32_t ef, int64_t* out_idx_dev,
                              float* out_dist_dev, int32_t* out_visited_dev, void* stream) {
  int rc = graph_search_check(gr, nq, k, ef);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q_dev, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx_dev, "null pointer: out_idx");
  if (nq == 0) return MI_OK;
  if ((rc = pq_graph_fresh(gr)) != MI_OK) return rc;
  HIPC(hipSetDevice(gr->device));
  return pq_graph_enqueue(gr, q_dev, MI_F32, gr->codes->d, 1, nq, k, ef, out_idx_dev, out_dist_dev, out_visited_dev,
                          (hipStream_t)stream);
}

int mi_pq_graph_search(mi_pq_graph* gr, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                       int32_t ef, int64_t* out_idx, float* out_dist, int32_t* out_visited, double* out_seconds) {
  int rc = graph_search_check(gr, nq, k, ef);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  if (out_seconds) *out_seconds = 0.0;
  if (nq == 0) return MI_OK;
  mi_pq* h = gr->codes;
  if ((rc = check_host_queries(h->d, q, nq, dtype, row_stride, col_stride)) != MI_OK) return rc;
  std::lock_guard<std::mutex> lock(gr->mu);
  std::lock_guard<std::mutex> lock_codes(h->mu);
  if ((rc = pq_graph_fresh(gr)) != MI_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(gr->device));
  hipStream_t s = h->stream;
  const size_t cnt = (size_t)nq * k;
  if ((rc = gr->oidx.grow(cnt)) != MI_OK) return rc;
  if (out_dist && (rc = gr->odist.grow(cnt)) != MI_OK) return rc;
  if (out_visited && (rc = gr->ovis.grow((size_t)nq)) != MI_OK) return rc;
  std::vector<char> pack;
  if ((rc = stage_host_rows(gr->qraw, h->d, s, q, 0, nq, dtype, row_stride, col_stride, pack)) != MI_OK) return rc;
  if ((rc = pq_graph_enqueue(gr, gr->qraw, dtype, h->d, 1, nq, k, ef, gr->oidx, out_dist ? gr->odist.get() : nullptr,
                             out_visited ? gr->ovis.get() : nullptr, s)) != MI_OK)
    return rc;
  if (out_visited) HIPC(hipMemcpyAsync(out_visited, gr->ovis, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  return topk_to_host(out_idx, gr->oidx.get(), out_dist, gr->odist.get(), cnt, s, t0, out_seconds);
}

}  // extern "C"
