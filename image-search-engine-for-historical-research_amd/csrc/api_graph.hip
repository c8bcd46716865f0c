// Graph index over the stored rows of a gallery (mi_graph*; the role of the reference's HNSW matchers).  DESIGN.md 5.16.
// The handle holds a GraphTable (neighbour table int32 [n][R] and up to 64 entry rows on the device), plus the workspace of its
// searches; the rows, their metric and the stream of the host entry points are the gallery's.  Kernels: graph_search.hip (one
// workgroup per query, best-first traversal), graph_build.hip (table from exact nearest-neighbour lists); the lists themselves
// come from the verified search of the gallery (search_sync) followed by launch_refine, which puts them in the graph's own order.
// The first half of the file is what every graph index does with its table (declared in api_internal.h; api_pq_graph.hip calls it).
#include "api_internal.h"

// ---- shared by the graph indexes

// what both search forms check before the handle is read
int graph_search_check(const void* gr, int64_t nq, int32_t k, int32_t ef) {
  REQUIRE(gr, "null handle");
  REQUIRE(ef >= 1 && ef <= GRAPH_MAX_EF, "ef must be in [1, 2048]");
  REQUIRE(k >= 1 && k <= ef, "k must be in [1, ef]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  return MI_OK;
}

int graph_create_check(const void* owner, const int32_t* neighbors, int32_t R, int neighbors_memspace, const int32_t* entries,
                       int32_t ne, const void* out) {
  REQUIRE(owner, "null handle");
  REQUIRE(neighbors, "null pointer: neighbors");
  REQUIRE(entries, "null pointer: entries");
  REQUIRE(out, "null pointer: out");
  REQUIRE(R >= 1 && R <= GRAPH_MAX_R, "R must be in [1, 64]");
  REQUIRE(ne >= 1 && ne <= GRAPH_MAX_ENTRIES, "ne must be in [1, 64]");
  REQUIRE(neighbors_memspace == MI_HOST || neighbors_memspace == MI_DEVICE, "neighbors_memspace must be MI_HOST or MI_DEVICE");
  for (int32_t i = 0; i < ne; ++i) REQUIRE(entries[i] >= 0, "entry rows must lie in [0, n)");
  return MI_OK;
}

int graph_build_check(const void* owner, int32_t R, int32_t ne, const void* out) {
  REQUIRE(owner, "null handle");
  REQUIRE(out, "null pointer: out");
  REQUIRE(R >= 2 && R <= GRAPH_MAX_R && R % 2 == 0, "R must be even and in [2, 64]");
  REQUIRE(ne >= 1 && ne <= GRAPH_MAX_ENTRIES, "ne must be in [1, 64]");
  return MI_OK;
}

int graph_build_rows_check(int64_t n) {
  REQUIRE(n >= 2, "a graph is built over at least two rows");
  REQUIRE(n <= 0x7fffffff, "a graph takes at most 2^31 - 1 rows");
  return MI_OK;
}

int graph_table_alloc(GraphTable& t, int64_t n, int32_t R, int32_t ne, const char* name) {
  const hipError_t e = t.alloc(n, R, ne);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, std::string(name) + " table: " + hipGetErrorString(e));
  return MI_OK;
}

int graph_table_from_neighbors(GraphTable& t, int64_t n, int device, const char* name, const int32_t* neighbors, int32_t R,
                               int neighbors_memspace, const int32_t* entries, int32_t ne) {
  REQUIRE(n <= 0x7fffffff, "a graph takes at most 2^31 - 1 rows");
  for (int32_t i = 0; i < ne; ++i) REQUIRE(entries[i] < n, "entry rows must lie in [0, n)");
  HIPC(hipSetDevice(device));
  const size_t cnt = (size_t)n * R;
  std::vector<int32_t> staged;
  const int32_t* tab = neighbors;
  if (neighbors_memspace == MI_DEVICE) {
    staged.resize(cnt);
    HIPC(hipMemcpy(staged.data(), neighbors, cnt * 4, hipMemcpyDeviceToHost));
    tab = staged.data();
  }
  for (size_t i = 0; i < cnt; ++i) REQUIRE(tab[i] >= -1 && tab[i] < n, "table values must be -1 (padding) or lie in [0, n)");
  int rc = graph_table_alloc(t, n, R, ne, name);
  if (rc != MI_OK) return rc;
  hipError_t e = hipMemcpy(t.adj, tab, cnt * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(t.entries, entries, (size_t)ne * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    t.adj.reset(), t.entries.reset();
    return fail(MI_ERR_HIP, std::string(name) + " table copy: " + hipGetErrorString(e));
  }
  return MI_OK;
}

GraphBuildWs graph_build_workspace(TmpAlloc& tmp, int64_t n, int32_t R) {
  int32_t* F = tmp.get<int32_t>((size_t)n * R);
  int32_t* B = tmp.get<int32_t>((size_t)n * R);
  uint32_t* cnt = tmp.get<uint32_t>((size_t)n * 2);
  return {F, B, cnt, tmp.get<unsigned long long>((size_t)n + 1)};
}

int graph_table_finish(GraphTable& t, const GraphBuildWs& ws, TmpAlloc& tmp, const char* name, hipStream_t s) {
  const int64_t n = t.n;
  const std::string what = std::string(name) + " build: ";
  hipError_t e = hipMemsetAsync(ws.cnt, 0, (size_t)n * 2 * 4, s);
  if (e != hipSuccess) return fail(MI_ERR_HIP, what + hipGetErrorString(e));
  launch_graph_rev_count(ws.F, n, t.R, ws.cnt, ws.off, s);
  unsigned long long total = 0;
  e = hipMemcpyAsync(&total, ws.off + n, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(MI_ERR_HIP, what + hipGetErrorString(e));
  unsigned long long* edges = tmp.get<unsigned long long>((size_t)std::max<unsigned long long>(total, 1));
  if (!edges) return fail(MI_ERR_NOMEM, what + "reverse edges");
  launch_graph_table(ws.F, n, t.R, ws.off, ws.cnt + n, edges, ws.B, t.adj, s);
  std::vector<int32_t> ent((size_t)t.ne);
  for (int32_t i = 0; i < t.ne; ++i) ent[i] = (int32_t)(((__int128)i * n) / t.ne);
  e = hipMemcpyAsync(t.entries, ent.data(), (size_t)t.ne * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail(MI_ERR_HIP, what + hipGetErrorString(e));
  return MI_OK;
}

int graph_table_get_neighbors(const GraphTable& t, std::mutex& mu, int device, int64_t row0, int64_t nrows, int32_t* out_host) {
  REQUIRE(nrows >= 0 && row0 >= 0, "negative row range");
  REQUIRE(nrows == 0 || out_host, "null pointer: out");
  REQUIRE(row0 + nrows <= t.n, "row range beyond the table");
  if (nrows == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(mu);
  HIPC(hipSetDevice(device));
  HIPC(hipMemcpy(out_host, t.adj + (size_t)row0 * t.R, (size_t)nrows * t.R * 4, hipMemcpyDeviceToHost));
  return MI_OK;
}

int graph_table_get_entries(const GraphTable& t, std::mutex& mu, int device, int32_t* out_host) {
  REQUIRE(out_host, "null pointer: out");
  std::lock_guard<std::mutex> lock(mu);
  HIPC(hipSetDevice(device));
  HIPC(hipMemcpy(out_host, t.entries, (size_t)t.ne * 4, hipMemcpyDeviceToHost));
  return MI_OK;
}

// ---- mi_graph

struct mi_graph {
  mi_gallery* rows = nullptr;
  GraphTable table;                    // table.n: rows of the gallery when it was made; a search refuses any other number
  // grow-only workspace of the searches (all of these free themselves when the handle is deleted)
  DeviceBuf<char> qraw;                // queries of a host call as given
  DeviceBuf<float> qpad;               // [nq][dp]
  DeviceBuf<uint32_t> vis;             // [queries of a chunk][ceil(n / 32)] visited bitmaps
  DeviceBuf<int64_t> oidx;             // results of a host call
  DeviceBuf<float> oval;
  DeviceBuf<double> oval64;
  DeviceBuf<int32_t> ovis;
  std::mutex mu;
};

static int graph_fresh(const mi_graph* gr) {
  REQUIRE(gr->rows->n == gr->table.n, "the gallery has been appended to or had rows removed since the graph was made: build a new graph");
  return MI_OK;
}

// queries [nq][dp] in gr->qpad (from `src`, device memory, any strides), then one launch per chunk of queries on `s`
static int graph_enqueue(mi_graph* gr, const void* src, int dtype, int64_t rs, int64_t cs, int64_t nq, int32_t k, int32_t ef,
                         int64_t* out_idx, float* out_val, double* out_val64, int32_t* out_visited, hipStream_t s) {
  mi_gallery* g = gr->rows;
  const GraphTable& t = gr->table;
  int rc;
  if ((rc = gr->qpad.grow((size_t)nq * g->dp)) != MI_OK) return rc;
  const auto [words, chunk] = graph_vis_chunks(t.n, nq);
  if ((rc = gr->vis.grow((size_t)chunk * words)) != MI_OK) return rc;
  launch_l2_augment(src, dtype, nq, g->ud, rs, cs, gr->qpad, g->dp, s);
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t b = std::min<int64_t>(chunk, nq - q0);
    HIPC(hipMemsetAsync(gr->vis, 0, (size_t)b * words * 4, s));
    launch_graph_search(g->gal_f32, gr->qpad + (size_t)q0 * g->dp, g->dp, g->ud, t.n, g->row_offset,
                        g->metric == MI_METRIC_L2 ? 1 : 0, t.adj, t.R, t.entries, t.ne, k, ef, b, gr->vis, words,
                        out_idx + q0 * k, out_val ? out_val + q0 * k : nullptr, out_val64 ? out_val64 + q0 * k : nullptr,
                        out_visited ? out_visited + q0 : nullptr, s);
  }
  HIPC(hipGetLastError());
  return MI_OK;
}

extern "C" {

int mi_graph_create(mi_gallery* rows, const int32_t* neighbors, int32_t R, int neighbors_memspace, const int32_t* entries,
                    int32_t ne, mi_graph** out) {
  int rc = graph_create_check(rows, neighbors, R, neighbors_memspace, entries, ne, out);
  if (rc != MI_OK) return rc;
  std::lock_guard<std::mutex> lock(rows->mu);
  REQUIRE(rows->n >= 1, "the gallery holds no rows");
  mi_graph* gr = new mi_graph();
  gr->rows = rows;
  if ((rc = graph_table_from_neighbors(gr->table, rows->n, rows->device, "graph", neighbors, R, neighbors_memspace, entries, ne)) != MI_OK) {
    delete gr;
    return rc;
  }
  *out = gr;
  return MI_OK;
}

int mi_graph_build(mi_gallery* rows, int32_t R, int32_t ne, mi_graph** out) {
  int rc = graph_build_check(rows, R, ne, out);
  if (rc != MI_OK) return rc;
  mi_gallery* g = rows;
  std::lock_guard<std::mutex> lock(g->mu);
  const int64_t n = g->n;
  if ((rc = graph_build_rows_check(n)) != MI_OK) return rc;
  HIPC(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  const bool l2 = g->metric == MI_METRIC_L2;
  const int32_t ks = (int32_t)std::min<int64_t>(R + 1, n);
  if ((rc = join_tails(g, s)) != MI_OK) return rc;
  mi_graph* gr = new mi_graph();
  gr->rows = g;
  if ((rc = graph_table_alloc(gr->table, n, R, (int32_t)std::min<int64_t>(ne, n), "graph")) != MI_OK) {
    delete gr;
    return rc;
  }
  auto bail = [&](int code) {
    (void)hipStreamSynchronize(s);
    delete gr;
    return code;
  };
  TmpAlloc tmp;                                  // (freed on return; every path out of here has synchronised `s`)
  const int64_t bmax = std::min<int64_t>(GRAPH_BUILD_BATCH, n);
  const GraphBuildWs ws = graph_build_workspace(tmp, n, R);
  int64_t* ids = tmp.get<int64_t>((size_t)bmax * ks);
  int64_t* ord = tmp.get<int64_t>((size_t)bmax * ks);
  double* val = tmp.get<double>((size_t)bmax * ks);
  float* qaug = l2 ? tmp.get<float>((size_t)bmax * g->dp) : nullptr;
  if (!ws.F || !ws.B || !ws.cnt || !ws.off || !ids || !ord || !val || (l2 && !qaug)) return bail(fail(MI_ERR_NOMEM, "graph build workspace"));
  // forward lists: the exact search of every stored row against the gallery, through the verified loop (a raised flag is answered
  // again inside search_sync), then the values and the order of mi_refine over what it returned
  for (int64_t r0 = 0; r0 < n; r0 += bmax) {
    const int64_t b = std::min<int64_t>(bmax, n - r0);
    const float* src = g->gal_f32 + (size_t)r0 * g->dp;
    if (l2) {
      // (an L2 gallery is searched with three 1.0 columns behind the caller's: api_l2.hip)
      launch_l2_augment(src, MI_F32, b, g->ud, g->dp, 1, qaug, g->dp, s);
      rc = search_sync(g, qaug, MI_F32, g->dp, 1, MI_NORM_NONE, b, ks, ids, nullptr, nullptr);
    } else {
      rc = search_sync(g, src, MI_F32, g->dp, 1, MI_NORM_NONE, b, ks, ids, nullptr, nullptr);
    }
    if (rc != MI_OK) return bail(rc);
    launch_refine(g->gal_f32, src, g->dp, g->ud, n, g->row_offset, l2 ? 1 : 0, ids, ks, ks, ks, b, val, ord, nullptr, nullptr, s);
    launch_graph_forward(ord, ks, r0, b, g->row_offset, n, R, ws.F, s);
    hipError_t e = hipStreamSynchronize(s);        // (ids / ord / val are reused by the next batch's search)
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return bail(fail(MI_ERR_HIP, std::string("graph build: ") + hipGetErrorString(e)));
  }
  if ((rc = graph_table_finish(gr->table, ws, tmp, "graph", s)) != MI_OK) return bail(rc);
  *out = gr;
  return MI_OK;
}

int mi_graph_info(const mi_graph* gr, int64_t* n, int32_t* R, int32_t* ne) {
  REQUIRE(gr, "null handle");
  if (n) *n = gr->table.n;
  if (R) *R = gr->table.R;
  if (ne) *ne = gr->table.ne;
  return MI_OK;
}

int mi_graph_get_neighbors(mi_graph* gr, int64_t row0, int64_t nrows, int32_t* out_host) {
  REQUIRE(gr, "null handle");
  return graph_table_get_neighbors(gr->table, gr->mu, gr->rows->device, row0, nrows, out_host);
}

int mi_graph_get_entries(mi_graph* gr, int32_t* out_host) {
  REQUIRE(gr, "null handle");
  return graph_table_get_entries(gr->table, gr->mu, gr->rows->device, out_host);
}

int mi_graph_destroy(mi_graph* gr) {
  if (!gr) return MI_OK;
  (void)hipSetDevice(gr->rows->device);
  (void)hipDeviceSynchronize();
  delete gr;
  return MI_OK;
}

int mi_graph_search_device(mi_graph* gr, const float* q_dev, int64_t nq, int32_t k, int32_t ef, int64_t* out_idx_dev,
                           float* out_val_dev, double* out_val64_dev, int32_t* out_visited_dev, void* stream) {
  int rc = graph_search_check(gr, nq, k, ef);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q_dev, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx_dev, "null pointer: out_idx");
  if (nq == 0) return MI_OK;
  if ((rc = graph_fresh(gr)) != MI_OK) return rc;
  HIPC(hipSetDevice(gr->rows->device));
  return graph_enqueue(gr, q_dev, MI_F32, gr->rows->ud, 1, nq, k, ef, out_idx_dev, out_val_dev, out_val64_dev, out_visited_dev,
                       (hipStream_t)stream);
}

int mi_graph_search(mi_graph* gr, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                    int32_t ef, int64_t* out_idx, float* out_val, double* out_val64, int32_t* out_visited, double* out_seconds) {
  int rc = graph_search_check(gr, nq, k, ef);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  if (out_seconds) *out_seconds = 0.0;
  if (nq == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(gr->mu);
  mi_gallery* g = gr->rows;
  std::lock_guard<std::mutex> lock_rows(g->mu);
  if ((rc = graph_fresh(gr)) != MI_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  int64_t elems;
  if ((rc = strided_extent(nq, g->ud, row_stride, col_stride, &elems)) != MI_OK) return rc;
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  if ((rc = gr->qraw.grow((size_t)elems * esz)) != MI_OK) return rc;
  const size_t cnt = (size_t)nq * k;
  if ((rc = gr->oidx.grow(cnt)) != MI_OK || (rc = gr->oval.grow(cnt)) != MI_OK ||
      (rc = gr->oval64.grow(cnt)) != MI_OK || (rc = gr->ovis.grow((size_t)nq)) != MI_OK)
    return rc;
  HIPC(hipMemcpyAsync(gr->qraw, q, (size_t)elems * esz, hipMemcpyHostToDevice, s));
  if ((rc = graph_enqueue(gr, gr->qraw, dtype, row_stride, col_stride, nq, k, ef, gr->oidx, gr->oval, gr->oval64, gr->ovis, s)) !=
      MI_OK)
    return rc;
  HIPC(hipMemcpyAsync(out_idx, gr->oidx, cnt * 8, hipMemcpyDeviceToHost, s));
  if (out_val) HIPC(hipMemcpyAsync(out_val, gr->oval, cnt * 4, hipMemcpyDeviceToHost, s));
  if (out_val64) HIPC(hipMemcpyAsync(out_val64, gr->oval64, cnt * 8, hipMemcpyDeviceToHost, s));
  if (out_visited) HIPC(hipMemcpyAsync(out_visited, gr->ovis, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return MI_OK;
}

}  // extern "C"
