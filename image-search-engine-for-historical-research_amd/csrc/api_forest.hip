// Random-projection forest over the stored rows of a gallery (mi_forest*; the role of the reference's matching_ANNOY).  DESIGN.md 5.17.
// The handle holds the directions float64 [T L][d], the split values float64 [T][2^L - 1] and the row permutations int32 [T][n] on
// the device, plus the workspace of its searches; the rows, their metric and the stream of the host entry points are the gallery's.
// Kernels: forest_project.hip (the projections of stored rows and of queries: ONE kernel), forest_build.hip (a level of a group of
// trees: stable radix sort by (node, projection, id), split values, next level's nodes), forest_search.hip (descent and leaf copy);
// the answer is launch_refine over the candidate slots, so values, order and padding are mi_refine's.
#include "api_internal.h"

constexpr int32_t FOREST_MAX_T = 256, FOREST_MAX_L = 24, FOREST_MAX_D = 4096;
// projections, candidate slots and candidate values of one chunk of queries: a batch that needs more goes in chunks of queries
constexpr size_t FOREST_STAGE_BYTES = (size_t)64 << 20;

struct mi_forest {
  mi_gallery* rows = nullptr;
  int64_t n = 0;                       // rows of the gallery when the forest was made; a search refuses any other number
  int32_t d = 0, T = 0, L = 0, leaf_max = 0;
  DeviceBuf<double> dirs;              // [T L][d]
  DeviceBuf<double> splits;            // [T][2^L - 1]
  DeviceBuf<int32_t> leaves;           // [T][n]
  // grow-only workspace of the searches (all of these free themselves when the handle is deleted)
  DeviceBuf<char> qraw;                // queries of a host call as given
  DeviceBuf<float> qpad;               // [nq][dp]
  DeviceBuf<double> pq;                // [queries of a chunk][T L] projections
  DeviceBuf<int64_t> cand;             // [queries of a chunk][T leaf_max] candidate slots
  DeviceBuf<double> val;               // [queries of a chunk][T leaf_max] their values (launch_refine's workspace)
  DeviceBuf<int64_t> oidx;             // results of a host call
  DeviceBuf<float> oval;
  DeviceBuf<double> oval64;
  std::mutex mu;
  size_t nsplit() const { return ((size_t)1 << L) - 1; }
  int32_t kc() const { return T * leaf_max; }
};

// ---- checks that answer before a handle is read
static int forest_make_check(const void* rows, const double* dirs, int32_t T, int32_t L, const void* out) {
  REQUIRE(rows, "null handle");
  REQUIRE(dirs, "null pointer: dirs");
  REQUIRE(out, "null pointer: out");
  REQUIRE(T >= 1 && T <= FOREST_MAX_T, "T must be in [1, 256]");
  REQUIRE(L >= 1 && L <= FOREST_MAX_L, "L must be in [1, 24]");
  return MI_OK;
}

static int forest_query_check(const void* f, int64_t nq) {
  REQUIRE(f, "null handle");
  REQUIRE(nq >= 0, "nq must be >= 0");
  return MI_OK;
}

static int forest_search_check(const void* f, int64_t nq, int32_t k) {
  REQUIRE(f, "null handle");
  REQUIRE(k >= 1 && k <= REFINE_MAX_KC, "k must be in [1, T * leaf_max]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  return MI_OK;
}

// ---- checks on the gallery's shape (its lock is held) and on the directions; nothing touches a device
static int forest_shape_check(const mi_gallery* g, const double* dirs, int32_t T, int32_t L, int32_t* leaf_max) {
  const int64_t n = g->n;
  REQUIRE(n >= 1, "the gallery holds no rows");
  REQUIRE(n <= 0x7fffffff, "a forest takes at most 2^31 - 1 rows");
  REQUIRE(g->ud <= FOREST_MAX_D, "a forest takes rows of d <= 4096 columns");
  REQUIRE(((int64_t)1 << L) <= n, "2^L must not exceed the rows of the gallery (" + std::to_string(n) + ")");
  const int64_t lm = (n + ((int64_t)1 << L) - 1) >> L;
  REQUIRE((int64_t)T * lm <= REFINE_MAX_KC, "T * leaf_max = " + std::to_string((int64_t)T * lm) +
                                                " candidates per query: at most 8192 (more levels or fewer trees)");
  const size_t cnt = (size_t)T * L * g->ud;
  for (size_t i = 0; i < cnt; ++i) REQUIRE(std::isfinite(dirs[i]), "dirs must be finite");
  *leaf_max = (int32_t)lm;
  return MI_OK;
}

static int forest_alloc(mi_forest* f, mi_gallery* g, const double* dirs, int32_t T, int32_t L, int32_t leaf_max) {
  f->rows = g, f->n = g->n, f->d = g->ud, f->T = T, f->L = L, f->leaf_max = leaf_max;
  int rc;
  if ((rc = f->dirs.grow_exact((size_t)T * L * f->d)) != MI_OK || (rc = f->splits.grow_exact((size_t)T * f->nsplit())) != MI_OK ||
      (rc = f->leaves.grow_exact((size_t)T * f->n)) != MI_OK)
    return rc;
  HIPC(hipMemcpy(f->dirs, dirs, (size_t)T * L * f->d * 8, hipMemcpyHostToDevice));
  return MI_OK;
}

static int forest_fresh(const mi_forest* f) {
  REQUIRE(f->rows->n == f->n, "the gallery has been appended to or had rows removed since the forest was made: build a new forest");
  return MI_OK;
}

// queries [nq][dp] in f->qpad (from `src`, device memory, any strides); then per chunk of queries: projections, descent into the
// candidate slots (cand_dev [nq][T leaf_max], or the handle's own buffer, copied to cand_host [nq][T leaf_max] where given) and,
// with k >= 1, launch_refine over them.  All on `s`, no synchronisation
static int forest_enqueue(mi_forest* f, const void* src, int dtype, int64_t rs, int64_t cs, int64_t nq, int32_t k, int64_t* cand_dev,
                          int64_t* cand_host, int64_t* out_idx, float* out_val, double* out_val64, hipStream_t s) {
  mi_gallery* g = f->rows;
  const int32_t C = f->T * f->L, kc = f->kc();
  const size_t per = (size_t)C * 8 + (cand_dev ? 0 : (size_t)kc * 8) + (k ? (size_t)kc * 8 : 0);
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(FOREST_STAGE_BYTES / per)));
  int rc;
  if ((rc = f->qpad.grow((size_t)nq * g->dp)) != MI_OK || (rc = f->pq.grow((size_t)chunk * C)) != MI_OK) return rc;
  if (!cand_dev && (rc = f->cand.grow((size_t)chunk * kc)) != MI_OK) return rc;
  if (k && (rc = f->val.grow((size_t)chunk * kc)) != MI_OK) return rc;
  launch_l2_augment(src, dtype, nq, g->ud, rs, cs, f->qpad, g->dp, s);
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t b = std::min<int64_t>(chunk, nq - q0);
    const float* q = f->qpad + (size_t)q0 * g->dp;
    int64_t* c = cand_dev ? cand_dev + q0 * kc : f->cand.get();
    launch_forest_project(q, b, g->ud, g->dp, 1, f->dirs, C, f->pq, C, 1, s);
    launch_forest_descend(f->pq, f->splits, f->leaves, f->n, f->T, f->L, f->leaf_max, g->row_offset, b, c, kc, s);
    if (cand_host) HIPC(hipMemcpyAsync(cand_host + q0 * kc, c, (size_t)b * kc * 8, hipMemcpyDeviceToHost, s));
    if (k)
      launch_refine(g->gal_f32, q, g->dp, g->ud, f->n, g->row_offset, g->metric == MI_METRIC_L2 ? 1 : 0, c, kc, kc, k, b, f->val,
                    out_idx + q0 * k, out_val ? out_val + q0 * k : nullptr, out_val64 ? out_val64 + q0 * k : nullptr, s);
  }
  HIPC(hipGetLastError());
  return MI_OK;
}

// the queries of a host call onto the device, in f->qraw
static int forest_stage_queries(mi_forest* f, const void* q, int64_t nq, int dtype, int64_t rs, int64_t cs, hipStream_t s) {
  int64_t elems;
  int rc;
  if ((rc = strided_extent(nq, f->rows->ud, rs, cs, &elems)) != MI_OK) return rc;
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  if ((rc = f->qraw.grow((size_t)elems * esz)) != MI_OK) return rc;
  HIPC(hipMemcpyAsync(f->qraw, q, (size_t)elems * esz, hipMemcpyHostToDevice, s));
  return MI_OK;
}

// trees [tree0, tree0 + ntrees) of a per-tree table of `per` elements into host memory
template <typename E>
static int forest_get(mi_forest* f, const E* table, size_t per, int32_t tree0, int32_t ntrees, E* out_host) {
  REQUIRE(ntrees >= 0 && tree0 >= 0, "negative tree range");
  REQUIRE(ntrees == 0 || out_host, "null pointer: out");
  REQUIRE((int64_t)tree0 + ntrees <= f->T, "tree range beyond the forest");
  if (ntrees == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(f->mu);
  HIPC(hipSetDevice(f->rows->device));
  HIPC(hipMemcpy(out_host, table + (size_t)tree0 * per, (size_t)ntrees * per * sizeof(E), hipMemcpyDeviceToHost));
  return MI_OK;
}

extern "C" {

int mi_forest_create(mi_gallery* rows, const double* dirs, int32_t T, int32_t L, const double* splits, const int32_t* leaves,
                     int memspace, mi_forest** out) {
  int rc = forest_make_check(rows, dirs, T, L, out);
  if (rc != MI_OK) return rc;
  REQUIRE(splits, "null pointer: splits");
  REQUIRE(leaves, "null pointer: leaves");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  mi_gallery* g = rows;
  std::lock_guard<std::mutex> lock(g->mu);
  int32_t leaf_max;
  if ((rc = forest_shape_check(g, dirs, T, L, &leaf_max)) != MI_OK) return rc;
  const int64_t n = g->n;
  const size_t cnt = (size_t)T * n;
  const hipMemcpyKind kind = memspace == MI_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  std::vector<int32_t> staged;
  const int32_t* lv = leaves;
  if (memspace == MI_DEVICE) {
    HIPC(hipSetDevice(g->device));
    staged.resize(cnt);
    HIPC(hipMemcpy(staged.data(), leaves, cnt * 4, hipMemcpyDeviceToHost));
    lv = staged.data();
  }
  for (size_t i = 0; i < cnt; ++i) REQUIRE(lv[i] >= 0 && lv[i] < n, "leaf values must lie in [0, n)");
  HIPC(hipSetDevice(g->device));
  mi_forest* f = new mi_forest();
  if ((rc = forest_alloc(f, g, dirs, T, L, leaf_max)) != MI_OK) {
    delete f;
    return rc;
  }
  hipError_t e = hipMemcpy(f->splits, splits, (size_t)T * f->nsplit() * 8, kind);
  if (e == hipSuccess) e = hipMemcpy(f->leaves, leaves, cnt * 4, kind);
  if (e != hipSuccess) {
    delete f;
    return fail(MI_ERR_HIP, std::string("forest copy: ") + hipGetErrorString(e));
  }
  *out = f;
  return MI_OK;
}

int mi_forest_build(mi_gallery* rows, const double* dirs, int32_t T, int32_t L, mi_forest** out) {
  int rc = forest_make_check(rows, dirs, T, L, out);
  if (rc != MI_OK) return rc;
  mi_gallery* g = rows;
  std::lock_guard<std::mutex> lock(g->mu);
  int32_t leaf_max;
  if ((rc = forest_shape_check(g, dirs, T, L, &leaf_max)) != MI_OK) return rc;
  const int64_t n = g->n;
  HIPC(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  if ((rc = join_tails(g, s)) != MI_OK) return rc;
  mi_forest* f = new mi_forest();
  if ((rc = forest_alloc(f, g, dirs, T, L, leaf_max)) != MI_OK) {
    delete f;
    return rc;
  }
  // trees per group: what the scratch of one tree takes -- projections [L][n] float64, two id buffers and the nodes [n] int32, the
  // histograms [256][chunks] -- into option "forest_build_bytes", one tree at the least
  const int64_t nb = forest_sort_blocks(n);
  const size_t per_tree = (size_t)n * ((size_t)L * 8 + 12) + (size_t)nb * 256 * 4;
  const int32_t tg = (int32_t)std::max<int64_t>(1, std::min<int64_t>(T, g_forest_build_bytes.load() / (int64_t)per_tree));
  DeviceBuf<double> Pt;                          // (these free themselves on return; every path out of here has synchronised `s`)
  DeviceBuf<int32_t> ids, node;
  DeviceBuf<uint32_t> hist;
  auto bail = [&](int code) {
    (void)hipStreamSynchronize(s);
    delete f;
    return code;
  };
  if ((rc = Pt.grow_exact((size_t)tg * L * n)) != MI_OK || (rc = ids.grow_exact((size_t)2 * tg * n)) != MI_OK ||
      (rc = node.grow_exact((size_t)tg * n)) != MI_OK || (rc = hist.grow_exact((size_t)tg * 256 * nb)) != MI_OK)
    return bail(rc);
  for (int32_t t0 = 0; t0 < T; t0 += tg) {
    const int32_t tn = std::min(tg, T - t0);
    // column c = (t - t0) L + l of the group, stored one column after another: Pt[c][row]
    launch_forest_project(g->gal_f32, n, g->ud, g->dp, 1, f->dirs + (size_t)t0 * L * f->d, tn * L, Pt, 1, n, s);
    for (int32_t l = 0; l < L; ++l)
      launch_forest_level(Pt, n, tn, L, l, node, ids, hist, f->splits + (size_t)t0 * f->nsplit(), f->leaves + (size_t)t0 * n, s);
  }
  hipError_t e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return bail(fail(MI_ERR_HIP, std::string("forest build: ") + hipGetErrorString(e)));
  *out = f;
  return MI_OK;
}

int mi_forest_info(const mi_forest* f, int64_t* n, int32_t* d, int32_t* T, int32_t* L, int32_t* leaf_max) {
  REQUIRE(f, "null handle");
  if (n) *n = f->n;
  if (d) *d = f->d;
  if (T) *T = f->T;
  if (L) *L = f->L;
  if (leaf_max) *leaf_max = f->leaf_max;
  return MI_OK;
}

int mi_forest_get_splits(mi_forest* f, int32_t tree0, int32_t ntrees, double* out_host) {
  REQUIRE(f, "null handle");
  return forest_get<double>(f, f->splits, f->nsplit(), tree0, ntrees, out_host);
}

int mi_forest_get_leaves(mi_forest* f, int32_t tree0, int32_t ntrees, int32_t* out_host) {
  REQUIRE(f, "null handle");
  return forest_get<int32_t>(f, f->leaves, (size_t)f->n, tree0, ntrees, out_host);
}

int mi_forest_get_dirs(mi_forest* f, double* out_host) {
  REQUIRE(f, "null handle");
  return forest_get<double>(f, f->dirs, (size_t)f->L * f->d, 0, f->T, out_host);
}

int mi_forest_destroy(mi_forest* f) {
  if (!f) return MI_OK;
  (void)hipSetDevice(f->rows->device);
  (void)hipDeviceSynchronize();
  delete f;
  return MI_OK;
}

int mi_forest_candidates_device(mi_forest* f, const float* q_dev, int64_t nq, int64_t* out_cand_dev, void* stream) {
  int rc = forest_query_check(f, nq);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q_dev, "null pointer: queries");
  REQUIRE(nq == 0 || out_cand_dev, "null pointer: out_cand");
  if (nq == 0) return MI_OK;
  if ((rc = forest_fresh(f)) != MI_OK) return rc;
  HIPC(hipSetDevice(f->rows->device));
  return forest_enqueue(f, q_dev, MI_F32, f->rows->ud, 1, nq, 0, out_cand_dev, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int mi_forest_candidates(mi_forest* f, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int64_t* out_cand,
                         double* out_seconds) {
  int rc = forest_query_check(f, nq);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(nq == 0 || out_cand, "null pointer: out_cand");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  if (out_seconds) *out_seconds = 0.0;
  if (nq == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(f->mu);
  mi_gallery* g = f->rows;
  std::lock_guard<std::mutex> lock_rows(g->mu);
  if ((rc = forest_fresh(f)) != MI_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  if ((rc = forest_stage_queries(f, q, nq, dtype, row_stride, col_stride, s)) != MI_OK) return rc;
  if ((rc = forest_enqueue(f, f->qraw, dtype, row_stride, col_stride, nq, 0, nullptr, out_cand, nullptr, nullptr, nullptr, s)) != MI_OK)
    return rc;
  HIPC(hipStreamSynchronize(s));
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return MI_OK;
}

int mi_forest_search_device(mi_forest* f, const float* q_dev, int64_t nq, int32_t k, int64_t* out_idx_dev, float* out_val_dev,
                            double* out_val64_dev, void* stream) {
  int rc = forest_search_check(f, nq, k);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q_dev, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx_dev, "null pointer: out_idx");
  if (nq == 0) return MI_OK;
  REQUIRE(k <= f->kc(), "k must be in [1, T * leaf_max = " + std::to_string(f->kc()) + "]");
  if ((rc = forest_fresh(f)) != MI_OK) return rc;
  HIPC(hipSetDevice(f->rows->device));
  return forest_enqueue(f, q_dev, MI_F32, f->rows->ud, 1, nq, k, nullptr, nullptr, out_idx_dev, out_val_dev, out_val64_dev,
                        (hipStream_t)stream);
}

int mi_forest_search(mi_forest* f, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                     int64_t* out_idx, float* out_val, double* out_val64, double* out_seconds) {
  int rc = forest_search_check(f, nq, k);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  if (out_seconds) *out_seconds = 0.0;
  if (nq == 0) return MI_OK;
  REQUIRE(k <= f->kc(), "k must be in [1, T * leaf_max = " + std::to_string(f->kc()) + "]");
  std::lock_guard<std::mutex> lock(f->mu);
  mi_gallery* g = f->rows;
  std::lock_guard<std::mutex> lock_rows(g->mu);
  if ((rc = forest_fresh(f)) != MI_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  if ((rc = forest_stage_queries(f, q, nq, dtype, row_stride, col_stride, s)) != MI_OK) return rc;
  const size_t cnt = (size_t)nq * k;
  if ((rc = grow_all(cnt, f->oidx, f->oval, f->oval64)) != MI_OK) return rc;
  if ((rc = forest_enqueue(f, f->qraw, dtype, row_stride, col_stride, nq, k, nullptr, nullptr, f->oidx, f->oval, f->oval64, s)) != MI_OK)
    return rc;
  HIPC(hipMemcpyAsync(out_idx, f->oidx, cnt * 8, hipMemcpyDeviceToHost, s));
  if (out_val) HIPC(hipMemcpyAsync(out_val, f->oval, cnt * 4, hipMemcpyDeviceToHost, s));
  if (out_val64) HIPC(hipMemcpyAsync(out_val64, f->oval64, cnt * 8, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return MI_OK;
}

}  // extern "C"
