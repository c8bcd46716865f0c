// Exact radius search and self-join in the Minkowski metrics on the stored rows of a gallery (mi_range_search_minkowski,
// mi_range_search_minkowski_device, mi_minkowski_self_range): every admitted row whose value -- the float64 of
// mi_knn_search_minkowski, bit for bit, since the same scan kernel writes it -- is <= radius, in CSR form, ordered by (value asc, id asc).
// The queries go in chunks of whole scan tiles whose values and counts fit into "minkowski_range_bytes" (mink_range_plan.h).  Pass 1
// scans and counts every chunk and leaves the CSR offsets; pass 2 places, orders and writes the hits of one chunk after the other
// (a call of more than one chunk scans again: the values of a chunk are gone by then).  Kernels: minkowski.hip (the scan, unchanged),
// minkowski_range.hip (counts, offsets, placing), csr_order.hip (order and write-out).  Nothing is cached: the gallery is searched as
// it stands.
#include "api_internal.h"
#include "mink_range_plan.h"

namespace {

struct MrCall {
  bool self = false;                 // the self-join: query i is stored row row0 + i, only the rows above it are reported
  int64_t row0 = 0, nq = 0;
  int op = 0;
  double p = 0.0, radius = 0.0;
  const uint64_t* allow = nullptr;   // device bitmap or NULL
  const float* qry = nullptr;        // [nq][dp] on the device (not the self-join)
};
struct MrPlan {
  int64_t qc = 0, nchunks = 0, ld = 0;
};

// the first row a chunk scans: the self-join skips the 256-row scan blocks wholly below the chunk's first query
int64_t mr_row_base(const mi_gallery* g, const MrCall& c, int64_t q0) {
  if (!c.self) return 0;
  return std::min<int64_t>(g->n, (c.row0 + q0 + 1) / MINK_SCAN_BLOCK_ROWS * MINK_SCAN_BLOCK_ROWS);
}

int mr_prepare(mi_gallery* g, const MrCall& c, MrPlan* p) {
  auto& m = g->mink;
  const int64_t rows = g->n - mr_row_base(g, c, 0);            // the first chunk scans the most
  const int32_t nparts = mink_parts(rows);
  p->ld = std::max<int64_t>(rows, 1);
  p->qc = mink_range_chunk(g_minkowski_range_bytes.load(), rows, nparts, c.nq, mink_query_tile(g->ud));
  p->nchunks = (c.nq + p->qc - 1) / p->qc;
  int rc;
  if ((rc = m.val.grow((size_t)(p->qc * p->ld))) != MI_OK) return rc;
  if ((rc = grow_all((size_t)(p->qc * nparts), m.rcnt, m.roff)) != MI_OK) return rc;
  if (c.self) return m.qpad.grow((size_t)p->qc * g->dp);
  return MI_OK;
}

MinkRangeArgs mr_args(mi_gallery* g, const MrCall& c, const MrPlan& p, int64_t q0, int64_t* lims_dev) {
  auto& m = g->mink;
  MinkRangeArgs a;
  a.val = m.val;
  a.ld = p.ld;
  a.row_base = mr_row_base(g, c, q0);
  a.nrows = g->n - a.row_base;
  a.nq = (int32_t)std::min<int64_t>(p.qc, c.nq - q0);
  a.allow = c.allow;
  a.radius = c.radius;
  a.self_row0 = c.self ? c.row0 + q0 : -1;
  a.cnt = m.rcnt;
  a.off = m.roff;
  a.lims = lims_dev + q0;
  return a;
}

// the chunk's values and counts; write_lims: pass 1
void mr_scan_count(mi_gallery* g, const MrCall& c, const MinkRangeArgs& a, int64_t q0, bool write_lims, hipStream_t s) {
  auto& m = g->mink;
  const float* qry = c.qry ? c.qry + (size_t)q0 * g->dp : nullptr;
  if (c.self) {                                                  // stored rows -> the packed query staging
    launch_l2_augment(g->gal_f32 + (size_t)(c.row0 + q0) * g->dp, MI_F32, a.nq, g->ud, g->dp, 1, m.qpad, g->dp, s);
    qry = m.qpad;
  }
  launch_minkowski_scan(g->gal_f32 + (size_t)a.row_base * g->dp, qry, g->dp, g->ud, a.nrows, c.op, c.p, a.allow, a.nq, m.val, a.ld, s);
  launch_mink_range_count(a, q0 == 0, write_lims, s);
}

int mr_pass1(mi_gallery* g, const MrCall& c, const MrPlan& p, int64_t* lims_dev, hipStream_t s) {
  for (int64_t q0 = 0; q0 < c.nq; q0 += p.qc) mr_scan_count(g, c, mr_args(g, c, p, q0, lims_dev), q0, true, s);
  HIPC(hipGetLastError());
  return MI_OK;
}

// lims_host: the offsets on the host (a host call) or NULL; stage: entries the hit staging holds
int mr_pass2(mi_gallery* g, const MrCall& c, const MrPlan& p, int64_t* lims_dev, const int64_t* lims_host, int64_t stage,
             int64_t max_results, int64_t* out_idx, float* out_dist, double* out_dist64, hipStream_t s) {
  auto& m = g->mink;
  for (int64_t q0 = 0; q0 < c.nq; q0 += p.qc) {
    MinkRangeArgs a = mr_args(g, c, p, q0, lims_dev);
    int64_t max_cnt = std::min<int64_t>(a.nrows, stage), max_total = stage;
    if (lims_host) {
      max_cnt = 0;
      for (int64_t q = q0; q < q0 + a.nq; ++q) max_cnt = std::max(max_cnt, lims_host[q + 1] - lims_host[q]);
      max_total = lims_host[q0 + a.nq] - lims_host[q0];
      if (max_total == 0) continue;
    }
    if (a.nrows <= 0) continue;
    if (p.nchunks > 1) mr_scan_count(g, c, a, q0, false, s);
    a.total = lims_dev + c.nq;
    a.max_results = max_results;
    for (int i = 0; i < 2; ++i) a.key[i] = m.rkey[i], a.row[i] = m.rrow[i];
    launch_mink_range_emit(a, s);
    const int cur = launch_csr_order(a, max_cnt, max_total, s);
    launch_csr_write(a, cur, false, max_total, g->row_offset, out_idx, out_dist, out_dist64, s);
  }
  HIPC(hipGetLastError());
  return MI_OK;
}

int mr_stage_grow(mi_gallery* g, int64_t entries) {
  auto& m = g->mink;
  return grow_all((size_t)entries, m.rkey[0], m.rkey[1], m.rrow[0], m.rrow[1]);
}

// host output of a call whose queries (or rows) and bitmap are on the device; the caller holds the lock
int mr_host(mi_gallery* g, const MrCall& c, int64_t max_results, int64_t* out_lims, int64_t* out_idx, float* out_dist,
            double* out_dist64) {
  auto& m = g->mink;
  hipStream_t s = g->stream;
  MrPlan p;
  int rc;
  if ((rc = mr_prepare(g, c, &p)) != MI_OK) return rc;
  if ((rc = m.rlims.grow((size_t)c.nq + 1)) != MI_OK) return rc;
  if ((rc = mr_pass1(g, c, p, m.rlims, s)) != MI_OK) return rc;
  HIPC(hipMemcpyAsync(out_lims, m.rlims, ((size_t)c.nq + 1) * 8, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  const int64_t total = out_lims[c.nq];
  if (total > max_results)
    return fail(MI_ERR_CAPACITY, "radius search: " + std::to_string(total) + " results > max_results " + std::to_string(max_results) +
                                     "; call again with max_results >= out_lims[nq]");
  if (total == 0) return MI_OK;
  int64_t most = 0;                                   // hits of the fullest chunk
  for (int64_t q0 = 0; q0 < c.nq; q0 += p.qc) most = std::max(most, out_lims[std::min(q0 + p.qc, c.nq)] - out_lims[q0]);
  if ((rc = mr_stage_grow(g, most)) != MI_OK) return rc;
  if ((rc = m.oidx.grow((size_t)total)) != MI_OK) return rc;
  if (out_dist && (rc = m.odist.grow((size_t)total)) != MI_OK) return rc;
  if (out_dist64 && (rc = m.odist64.grow((size_t)total)) != MI_OK) return rc;
  if ((rc = mr_pass2(g, c, p, m.rlims, out_lims, most, total, m.oidx, out_dist ? m.odist.get() : nullptr,
                     out_dist64 ? m.odist64.get() : nullptr, s)) != MI_OK)
    return rc;
  HIPC(hipMemcpyAsync(out_idx, m.oidx, (size_t)total * 8, hipMemcpyDeviceToHost, s));
  if (out_dist) HIPC(hipMemcpyAsync(out_dist, m.odist, (size_t)total * 4, hipMemcpyDeviceToHost, s));
  if (out_dist64) HIPC(hipMemcpyAsync(out_dist64, m.odist64, (size_t)total * 8, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  return MI_OK;
}

// what the three entry points ask of their arguments before the handle is read
int mr_check(const mi_gallery* g, int64_t nq, int metric, double p, double radius, int64_t max_results, const void* out_lims,
             const void* out_idx, int* op) {
  const int rc = mink_check(g, nq, metric, p, 1, op);
  if (rc != MI_OK) return rc;
  REQUIRE(radius >= 0.0, "radius must be >= 0 and not NaN");
  REQUIRE(out_lims, "null pointer: out_lims");
  REQUIRE(max_results >= 0, "max_results must be >= 0");
  REQUIRE(max_results == 0 || out_idx, "null pointer: out_idx");
  return MI_OK;
}

int mr_gallery_check(const mi_gallery* g) {
  const int rc = mink_rows_check(g);
  if (rc != MI_OK) return rc;
  if (g->n >= (int64_t)1 << 32) return fail(MI_ERR_UNSUPPORTED, "a Minkowski radius search takes a gallery of fewer than 2^32 rows");
  return MI_OK;
}

}  // namespace

extern "C" {

int mi_range_search_minkowski(mi_gallery* rows, const void* q, int64_t nq, int q_dtype, int64_t row_stride, int64_t col_stride,
                              int metric, double p, double radius, const uint64_t* allow_bits, int allow_memspace,
                              int64_t max_results, int64_t* out_lims, int64_t* out_idx, float* out_dist, double* out_dist64,
                              double* out_seconds) {
  MrCall c;
  int rc = mr_check(rows, nq, metric, p, radius, max_results, out_lims, out_idx, &c.op);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(q_dtype == MI_F32 || q_dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  REQUIRE(!allow_bits || allow_memspace == MI_HOST || allow_memspace == MI_DEVICE, "allow_memspace must be MI_HOST or MI_DEVICE");
  if (out_seconds) *out_seconds = 0.0;
  out_lims[0] = 0;
  if (nq == 0) return MI_OK;
  mi_gallery* g = rows;
  std::lock_guard<std::mutex> lock(g->mu);
  if ((rc = mr_gallery_check(g)) != MI_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  auto& m = g->mink;
  int64_t elems;
  if ((rc = strided_extent(nq, g->ud, row_stride, col_stride, &elems)) != MI_OK) return rc;
  const size_t esz = q_dtype == MI_F32 ? 4 : 8;
  if ((rc = m.qraw.grow((size_t)elems * esz)) != MI_OK) return rc;
  if ((rc = m.qpad.grow((size_t)nq * g->dp)) != MI_OK) return rc;
  if ((rc = allow_on_device(m.bits, allow_bits, allow_memspace, g->n, s, &c.allow)) != MI_OK) return rc;
  if (g->n <= 0) c.allow = nullptr;                          // (no row to admit: the bitmap is never read)
  HIPC(hipMemcpyAsync(m.qraw, q, (size_t)elems * esz, hipMemcpyHostToDevice, s));
  launch_l2_augment(m.qraw, q_dtype, nq, g->ud, row_stride, col_stride, m.qpad, g->dp, s);
  c.qry = m.qpad;
  c.nq = nq;
  c.p = p;
  c.radius = radius;
  rc = mr_host(g, c, max_results, out_lims, out_idx, out_dist, out_dist64);
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int mi_range_search_minkowski_device(mi_gallery* rows, const float* q_dev, int64_t nq, int metric, double p, double radius,
                                     const uint64_t* allow_bits_dev, int64_t max_results, int64_t* out_lims_dev,
                                     int64_t* out_idx_dev, float* out_dist_dev, double* out_dist64_dev, void* stream) {
  MrCall c;
  int rc = mr_check(rows, nq, metric, p, radius, max_results, out_lims_dev, out_idx_dev, &c.op);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q_dev, "null pointer: queries");
  mi_gallery* g = rows;
  HIPC(hipSetDevice(g->device));
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) {
    HIPC(hipMemsetAsync(out_lims_dev, 0, 8, s));
    return MI_OK;
  }
  if ((rc = mr_gallery_check(g)) != MI_OK) return rc;
  auto& m = g->mink;
  if ((rc = m.qpad.grow((size_t)nq * g->dp)) != MI_OK) return rc;
  c.allow = g->n > 0 ? allow_bits_dev : nullptr;
  c.nq = nq;
  c.p = p;
  c.radius = radius;
  MrPlan pl;
  if ((rc = mr_prepare(g, c, &pl)) != MI_OK) return rc;
  // the hits of one chunk: at most the caller's capacity (beyond it nothing is written), at most every row for every query
  const int64_t stage = std::min<int64_t>(max_results, std::min(pl.qc, nq) * g->n);
  if (stage > 0 && (rc = mr_stage_grow(g, stage)) != MI_OK) return rc;
  launch_l2_augment(q_dev, MI_F32, nq, g->ud, g->ud, 1, m.qpad, g->dp, s);
  c.qry = m.qpad;
  if ((rc = mr_pass1(g, c, pl, out_lims_dev, s)) != MI_OK) return rc;
  if (stage == 0) return MI_OK;
  return mr_pass2(g, c, pl, out_lims_dev, nullptr, stage, max_results, out_idx_dev, out_dist_dev, out_dist64_dev, s);
}

int mi_minkowski_self_range(mi_gallery* rows, int64_t row0, int64_t nrows, int metric, double p, double radius, int64_t max_results,
                            int64_t* out_lims, int64_t* out_idx, float* out_dist, double* out_dist64, double* out_seconds) {
  MrCall c;
  int rc = mr_check(rows, 0, metric, p, radius, max_results, out_lims, out_idx, &c.op);
  if (rc != MI_OK) return rc;
  REQUIRE(row0 >= 0 && nrows >= 0, "row range outside the gallery");
  mi_gallery* g = rows;
  std::lock_guard<std::mutex> lock(g->mu);
  REQUIRE(row0 <= g->n && nrows <= g->n - row0, "row range outside the gallery");
  if (out_seconds) *out_seconds = 0.0;
  out_lims[0] = 0;
  if (nrows == 0) return MI_OK;
  if ((rc = mr_gallery_check(g)) != MI_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(g->device));
  c.self = true;
  c.row0 = row0;
  c.nq = nrows;
  c.p = p;
  c.radius = radius;
  rc = mr_host(g, c, max_results, out_lims, out_idx, out_dist, out_dist64);
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

}  // extern "C"
