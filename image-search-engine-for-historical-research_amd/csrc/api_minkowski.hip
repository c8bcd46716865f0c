// Exact Minkowski top-K on the stored rows of a gallery (faiss IndexFlat with METRIC_L1, METRIC_Linf, METRIC_Lp; the reference's
// fractional_distance): mi_knn_search_minkowski / mi_knn_search_minkowski_device.  DESIGN.md 5.19.  Every row of the gallery is
// evaluated in float64 against every query (minkowski.hip: the scan, then selection per part of the rows and a merge per query);
// nothing is cached, so a gallery that was appended to or had rows removed is searched as it then stands.
#include "api_internal.h"

// values and partial lists of one chunk of queries: a batch that needs more goes in chunks of queries
constexpr size_t MINK_STAGE_BYTES = (size_t)256 << 20;

// the argument checks both forms (and the radius search, api_minkowski_range.hip) share: they answer before the handle is read.  *op: the term the kernels evaluate
int mink_check(const mi_gallery* g, int64_t nq, int metric, double p, int32_t k, int* op) {
  REQUIRE(g, "null handle");
  REQUIRE(metric == MI_MINK_L1 || metric == MI_MINK_LINF || metric == MI_MINK_LP, "metric must be MI_MINK_L1, MI_MINK_LINF or MI_MINK_LP");
  REQUIRE(metric != MI_MINK_LP || (std::isfinite(p) && p > 0.0), "p must be finite and > 0 (MI_MINK_LINF is the infinite case)");
  REQUIRE(k >= 1 && k <= MINK_MAX_K, "k must be in [1, 2048]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  if (metric == MI_MINK_L1) *op = MINK_OP_L1;
  else if (metric == MI_MINK_LINF) *op = MINK_OP_LINF;
  else *op = p == 1.0 ? MINK_OP_L1 : p == 2.0 ? MINK_OP_SQ : p == 0.5 ? MINK_OP_SQRT : MINK_OP_POW;
  return MI_OK;
}

// what the gallery must be: one shard that holds its f32 rows, of a width whose query fits into LDS
int mink_rows_check(const mi_gallery* g) {
  if (!g->gal_f32) return fail(MI_ERR_UNSUPPORTED, "the gallery does not hold its f32 rows");
  if (mink_query_tile(g->ud) < 1)
    return fail(MI_ERR_UNSUPPORTED, "Minkowski search takes rows of at most 20480 columns (one float64 query in LDS)");
  return MI_OK;
}

// queries [nq][dp] in m.qpad (from `src`, device memory, any strides), then scan, selection and merge per chunk of queries on `s`
static int mink_enqueue(mi_gallery* g, const void* src, int dtype, int64_t rs, int64_t cs, int64_t nq, int op, double p, int32_t k,
                        const uint64_t* allow_dev, int64_t* out_idx, float* out_val, double* out_val64, hipStream_t s) {
  auto& m = g->mink;
  const int64_t n = g->n, ld = std::max<int64_t>(n, 1);
  const int32_t nparts = mink_parts(n);
  const size_t per = (size_t)ld * 8 + (size_t)nparts * k * 16;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nq, 65535), (int64_t)(MINK_STAGE_BYTES / per)));
  int rc;
  if ((rc = m.qpad.grow((size_t)nq * g->dp)) != MI_OK || (rc = m.val.grow((size_t)chunk * ld)) != MI_OK ||
      (rc = m.part_key.grow((size_t)chunk * nparts * k)) != MI_OK || (rc = m.part_id.grow((size_t)chunk * nparts * k)) != MI_OK)
    return rc;
  // rows of stride dp, the caller's ud columns (what follows them is never read: the scan stops at ud)
  launch_l2_augment(src, dtype, nq, g->ud, rs, cs, m.qpad, g->dp, s);
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t b = std::min<int64_t>(chunk, nq - q0);
    launch_minkowski(g->gal_f32, m.qpad + (size_t)q0 * g->dp, g->dp, g->ud, n, g->row_offset, op, p, allow_dev, k, (int32_t)b, m.val, ld,
                     m.part_key, m.part_id, out_idx + q0 * k, out_val ? out_val + q0 * k : nullptr,
                     out_val64 ? out_val64 + q0 * k : nullptr, s);
  }
  HIPC(hipGetLastError());
  return MI_OK;
}

extern "C" {

int mi_knn_search_minkowski_device(mi_gallery* rows, const float* q_dev, int64_t nq, int metric, double p, int32_t k,
                                   const uint64_t* allow_bits_dev, int64_t* out_idx_dev, float* out_dist_dev, double* out_dist64_dev,
                                   void* stream) {
  int op = 0;
  int rc = mink_check(rows, nq, metric, p, k, &op);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q_dev, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx_dev, "null pointer: out_idx");
  if (nq == 0) return MI_OK;
  if ((rc = mink_rows_check(rows)) != MI_OK) return rc;
  HIPC(hipSetDevice(rows->device));
  return mink_enqueue(rows, q_dev, MI_F32, rows->ud, 1, nq, op, p, k, allow_bits_dev, out_idx_dev, out_dist_dev, out_dist64_dev,
                      (hipStream_t)stream);
}

int mi_knn_search_minkowski(mi_gallery* rows, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int metric,
                            double p, int32_t k, const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_dist,
                            double* out_dist64, double* out_seconds) {
  int op = 0;
  int rc = mink_check(rows, nq, metric, p, k, &op);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  REQUIRE(!allow_bits || allow_memspace == MI_HOST || allow_memspace == MI_DEVICE, "allow_memspace must be MI_HOST or MI_DEVICE");
  if (out_seconds) *out_seconds = 0.0;
  if (nq == 0) return MI_OK;
  mi_gallery* g = rows;
  std::lock_guard<std::mutex> lock(g->mu);
  if ((rc = mink_rows_check(g)) != MI_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  auto& m = g->mink;
  int64_t elems;
  if ((rc = strided_extent(nq, g->ud, row_stride, col_stride, &elems)) != MI_OK) return rc;
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  if ((rc = m.qraw.grow((size_t)elems * esz)) != MI_OK) return rc;
  if ((rc = grow_all((size_t)nq * k, m.oidx, m.odist, m.odist64)) != MI_OK) return rc;
  const uint64_t* allow_dev = nullptr;
  if ((rc = allow_on_device(m.bits, allow_bits, allow_memspace, g->n, s, &allow_dev)) != MI_OK) return rc;
  if (g->n <= 0) allow_dev = nullptr;                       // (no row to admit: the bitmap is never read)
  HIPC(hipMemcpyAsync(m.qraw, q, (size_t)elems * esz, hipMemcpyHostToDevice, s));
  if ((rc = mink_enqueue(g, m.qraw, dtype, row_stride, col_stride, nq, op, p, k, allow_dev, m.oidx, m.odist, m.odist64, s)) != MI_OK)
    return rc;
  const size_t cnt = (size_t)nq * k;
  HIPC(hipMemcpyAsync(out_idx, m.oidx, cnt * 8, hipMemcpyDeviceToHost, s));
  if (out_dist) HIPC(hipMemcpyAsync(out_dist, m.odist, cnt * 4, hipMemcpyDeviceToHost, s));
  if (out_dist64) HIPC(hipMemcpyAsync(out_dist64, m.odist64, cnt * 8, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return MI_OK;
}

}  // extern "C"
