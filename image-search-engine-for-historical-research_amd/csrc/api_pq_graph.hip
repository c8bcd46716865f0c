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
  int64_t n = 0;                       // rows and modification count of the PQ index when the table was made: a search refuses
  uint64_t mod = 0;                    // any other pair
  int32_t R = 0, ne = 0;
  DeviceBufSet bufs;                   // every device allocation of the handle: hbm_bytes is bufs.bytes()
  DeviceBuf<int32_t> adj{bufs};        // [n][R], -1 = padding
  DeviceBuf<int32_t> entries{bufs};    // [ne]
  // grow-only workspace of the searches
  DeviceBuf<char> qraw{bufs};          // queries of a host call, packed [nq][d] in their own type
  DeviceBuf<float> tab{bufs};          // [queries of a chunk][m][ks] distance tables
  DeviceBuf<uint32_t> vis{bufs};       // [queries of a chunk][ceil(n / 32)] visited bitmaps
  DeviceBuf<int64_t> oidx{bufs};       // results of a host call
  DeviceBuf<float> odist{bufs};
  DeviceBuf<int32_t> ovis{bufs};
  std::mutex mu;
};

// bytes of visited bitmaps, and of distance tables, one launch may use: a batch that needs more is searched in chunks of queries
constexpr size_t PQ_GRAPH_VIS_BYTES = (size_t)256 << 20, PQ_GRAPH_TAB_BYTES = (size_t)256 << 20;
constexpr int64_t PQ_GRAPH_BUILD_BATCH = 8192;   // rows per exact search of mi_pq_graph_build

// what both search forms check before the handle is read
static int pq_graph_search_check(const mi_pq_graph* gr, int64_t nq, int32_t k, int32_t ef) {
  REQUIRE(gr, "null handle");
  REQUIRE(ef >= 1 && ef <= GRAPH_MAX_EF, "ef must be in [1, 2048]");
  REQUIRE(k >= 1 && k <= ef, "k must be in [1, ef]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  return MI_OK;
}

static int pq_graph_fresh(const mi_pq_graph* gr) {
  REQUIRE(gr->codes->n == gr->n && gr->codes->mod == gr->mod,
          "the PQ index has had rows added or removed since the graph was made: build a new graph");
  return MI_OK;
}

// tables of the queries at `src` (device memory, any strides) in gr->tab, then one launch per chunk of queries, all on `s`
static int pq_graph_enqueue(mi_pq_graph* gr, const void* src, int dtype, int64_t rs, int64_t cs, int64_t nq, int32_t k, int32_t ef,
                            int64_t* out_idx, float* out_dist, int32_t* out_visited, hipStream_t s) {
  mi_pq* h = gr->codes;
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  const int64_t words = (gr->n + 31) / 32, per = (int64_t)h->m * h->ks;
  const int64_t chunk = std::max<int64_t>(
      1, std::min<int64_t>({nq, (int64_t)(PQ_GRAPH_VIS_BYTES / 4) / words, (int64_t)(PQ_GRAPH_TAB_BYTES / 4) / per}));
  int rc;
  if ((rc = gr->vis.grow((size_t)chunk * words)) != MI_OK) return rc;
  if ((rc = gr->tab.grow((size_t)chunk * per)) != MI_OK) return rc;
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t b = std::min<int64_t>(chunk, nq - q0);
    launch_pq_table((const char*)src + (size_t)q0 * rs * esz, dtype, rs, cs, b, h->cb, h->m, h->ks, h->L, gr->tab, s);
    HIPC(hipMemsetAsync(gr->vis, 0, (size_t)b * words * 4, s));
    launch_pq_graph_search(h->codes, h->m, h->ks, gr->tab, gr->n, h->row_offset, gr->adj, gr->R, gr->entries, gr->ne, k, ef, b, gr->vis,
                           words, out_idx + q0 * k, out_dist ? out_dist + q0 * k : nullptr, out_visited ? out_visited + q0 : nullptr, s);
  }
  HIPC(hipGetLastError());
  return MI_OK;
}

// a handle over `codes` (whose lock the caller holds) with room for the table and the entries (neither filled)
static int pq_graph_alloc(mi_pq* codes, int32_t R, int32_t ne, mi_pq_graph** out) {
  mi_pq_graph* gr = new mi_pq_graph();
  gr->codes = codes;
  gr->device = codes->device;
  gr->n = codes->n;
  gr->mod = codes->mod;
  gr->R = R;
  gr->ne = ne;
  hipError_t e = gr->adj.alloc((size_t)gr->n * R);
  if (e == hipSuccess) e = gr->entries.alloc((size_t)ne);
  if (e != hipSuccess) {
    delete gr;
    return fail(e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, std::string("PQ graph table: ") + hipGetErrorString(e));
  }
  *out = gr;
  return MI_OK;
}

extern "C" {

int mi_pq_graph_create(mi_pq* codes, const int32_t* neighbors, int32_t R, int neighbors_memspace, const int32_t* entries, int32_t ne,
                       mi_pq_graph** out) {
  REQUIRE(codes, "null handle");
  REQUIRE(neighbors, "null pointer: neighbors");
  REQUIRE(entries, "null pointer: entries");
  REQUIRE(out, "null pointer: out");
  REQUIRE(R >= 1 && R <= GRAPH_MAX_R, "R must be in [1, 64]");
  REQUIRE(ne >= 1 && ne <= GRAPH_MAX_ENTRIES, "ne must be in [1, 64]");
  REQUIRE(neighbors_memspace == MI_HOST || neighbors_memspace == MI_DEVICE, "neighbors_memspace must be MI_HOST or MI_DEVICE");
  for (int32_t i = 0; i < ne; ++i) REQUIRE(entries[i] >= 0, "entry rows must lie in [0, n)");
  std::lock_guard<std::mutex> lock(codes->mu);
  const int64_t n = codes->n;
  REQUIRE(n >= 1, "the PQ index holds no rows");
  REQUIRE(n <= 0x7fffffff, "a graph takes at most 2^31 - 1 rows");
  for (int32_t i = 0; i < ne; ++i) REQUIRE(entries[i] < n, "entry rows must lie in [0, n)");
  HIPC(hipSetDevice(codes->device));
  const size_t cnt = (size_t)n * R;
  std::vector<int32_t> staged;
  const int32_t* tab = neighbors;
  if (neighbors_memspace == MI_DEVICE) {
    staged.resize(cnt);
    HIPC(hipMemcpy(staged.data(), neighbors, cnt * 4, hipMemcpyDeviceToHost));
    tab = staged.data();
  }
  for (size_t i = 0; i < cnt; ++i) REQUIRE(tab[i] >= -1 && tab[i] < n, "table values must be -1 (padding) or lie in [0, n)");
  mi_pq_graph* gr = nullptr;
  int rc = pq_graph_alloc(codes, R, ne, &gr);
  if (rc != MI_OK) return rc;
  hipError_t e = hipMemcpy(gr->adj, tab, cnt * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(gr->entries, entries, (size_t)ne * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    delete gr;
    return fail(MI_ERR_HIP, std::string("PQ graph table copy: ") + hipGetErrorString(e));
  }
  *out = gr;
  return MI_OK;
}

int mi_pq_graph_build(mi_pq* codes, int32_t R, int32_t ne, mi_pq_graph** out) {
  REQUIRE(codes, "null handle");
  REQUIRE(out, "null pointer: out");
  REQUIRE(R >= 2 && R <= GRAPH_MAX_R && R % 2 == 0, "R must be even and in [2, 64]");
  REQUIRE(ne >= 1 && ne <= GRAPH_MAX_ENTRIES, "ne must be in [1, 64]");
  mi_pq* h = codes;
  std::lock_guard<std::mutex> lock(h->mu);
  const int64_t n = h->n;
  REQUIRE(n >= 2, "a graph is built over at least two rows");
  REQUIRE(n <= 0x7fffffff, "a graph takes at most 2^31 - 1 rows");
  HIPC(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int32_t ks = (int32_t)std::min<int64_t>(R + 1, n);
  const int32_t nent = (int32_t)std::min<int64_t>(ne, n);
  int rc;
  mi_pq_graph* gr = nullptr;
  if ((rc = pq_graph_alloc(h, R, nent, &gr)) != MI_OK) return rc;
  auto bail = [&](int code) {
    (void)hipStreamSynchronize(s);
    delete gr;
    return code;
  };
  TmpAlloc tmp;                                   // (freed on return; every path out of here has synchronised `s`)
  const int64_t bmax = std::min<int64_t>(PQ_GRAPH_BUILD_BATCH, n);
  int32_t* F = tmp.get<int32_t>((size_t)n * R);
  int32_t* B = tmp.get<int32_t>((size_t)n * R);
  uint32_t* cnt = tmp.get<uint32_t>((size_t)n * 2);               // counts, then fill cursors
  unsigned long long* off = tmp.get<unsigned long long>((size_t)n + 1);
  int64_t* ids = tmp.get<int64_t>((size_t)bmax * ks);
  float* rec = tmp.get<float>((size_t)bmax * h->d);
  if (!F || !B || !cnt || !off || !ids || !rec) return bail(fail(MI_ERR_NOMEM, "PQ graph build workspace"));
  // forward lists: every stored row's reconstruction is a query of the exhaustive ADC search, whose answer is already in the
  // graph's order (distance asc, id asc)
  for (int64_t r0 = 0; r0 < n; r0 += bmax) {
    const int64_t b = std::min<int64_t>(bmax, n - r0);
    launch_pq_decode(h->codes, h->m, h->ks, h->L, h->cb, r0, b, rec, s);
    if ((rc = pq_search_core(h, rec, MI_F32, h->d, 1, b, ks, nullptr, ids, nullptr, s)) != MI_OK) return bail(rc);
    launch_graph_forward(ids, ks, r0, b, h->row_offset, n, R, F, s);
    hipError_t e = hipStreamSynchronize(s);        // (rec / ids are reused by the next batch)
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return bail(fail(MI_ERR_HIP, std::string("PQ graph build: ") + hipGetErrorString(e)));
  }
  hipError_t e = hipMemsetAsync(cnt, 0, (size_t)n * 2 * 4, s);
  if (e != hipSuccess) return bail(fail(MI_ERR_HIP, std::string("PQ graph build: ") + hipGetErrorString(e)));
  launch_graph_rev_count(F, n, R, cnt, off, s);
  unsigned long long total = 0;
  e = hipMemcpyAsync(&total, off + n, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return bail(fail(MI_ERR_HIP, std::string("PQ graph build: ") + hipGetErrorString(e)));
  unsigned long long* edges = tmp.get<unsigned long long>((size_t)std::max<unsigned long long>(total, 1));
  if (!edges) return bail(fail(MI_ERR_NOMEM, "PQ graph build: reverse edges"));
  launch_graph_table(F, n, R, off, cnt + n, edges, B, gr->adj, s);
  std::vector<int32_t> ent((size_t)nent);
  for (int32_t t = 0; t < nent; ++t) ent[t] = (int32_t)(((__int128)t * n) / nent);
  e = hipMemcpyAsync(gr->entries, ent.data(), (size_t)nent * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return bail(fail(MI_ERR_HIP, std::string("PQ graph build: ") + hipGetErrorString(e)));
  *out = gr;
  return MI_OK;
}

int mi_pq_graph_info(const mi_pq_graph* gr, int64_t* n, int32_t* R, int32_t* ne, int64_t* hbm_bytes) {
  REQUIRE(gr, "null handle");
  if (n) *n = gr->n;
  if (R) *R = gr->R;
  if (ne) *ne = gr->ne;
  if (hbm_bytes) *hbm_bytes = (int64_t)gr->bufs.bytes();
  return MI_OK;
}

int mi_pq_graph_get_neighbors(mi_pq_graph* gr, int64_t row0, int64_t nrows, int32_t* out_host) {
  REQUIRE(gr, "null handle");
  REQUIRE(nrows >= 0 && row0 >= 0, "negative row range");
  REQUIRE(nrows == 0 || out_host, "null pointer: out");
  REQUIRE(row0 + nrows <= gr->n, "row range beyond the table");
  if (nrows == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(gr->mu);
  HIPC(hipSetDevice(gr->device));
  HIPC(hipMemcpy(out_host, gr->adj + (size_t)row0 * gr->R, (size_t)nrows * gr->R * 4, hipMemcpyDeviceToHost));
  return MI_OK;
}

int mi_pq_graph_get_entries(mi_pq_graph* gr, int32_t* out_host) {
  REQUIRE(gr, "null handle");
  REQUIRE(out_host, "null pointer: out");
  std::lock_guard<std::mutex> lock(gr->mu);
  HIPC(hipSetDevice(gr->device));
  HIPC(hipMemcpy(out_host, gr->entries, (size_t)gr->ne * 4, hipMemcpyDeviceToHost));
  return MI_OK;
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
  int rc = pq_graph_search_check(gr, nq, k, ef);
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
  int rc = pq_graph_search_check(gr, nq, k, ef);
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
