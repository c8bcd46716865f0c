// Squared-L2 (Euclidean) metric of the C ABI: L2 galleries, exact top-K by distance (host / device), the dense checker.
// DESIGN.md 5.11.  An L2 gallery is a raw gallery with three hidden bias columns (csrc/l2_metric.hip), so the selection below
// is the inner-product search as it is -- search_sync / search_device / the filtered paths, on queries extended by three 1.0
// columns -- and what it certifies, the K largest s = q.g - 1/2 ||g||^2 in float64, are the K smallest distances.  The tail
// then takes the distances of those K rows in the direct form and orders them.
#include "api_internal.h"

#define REQUIRE_L2(g) REQUIRE((g)->metric == MI_METRIC_L2, "not a squared-L2 gallery (mi_gallery_create_l2)")

// host results of a call: [nq][k] from the handle's output buffers, after the work on `s`
static int l2_copy_out(mi_gallery* g, int64_t nq, int32_t k, int64_t* out_idx, float* out_dist, double* out_dist64, hipStream_t s) {
  const size_t cnt = (size_t)nq * k;
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(out_idx, g->l2.oidx, cnt * 8, hipMemcpyDeviceToHost, s));
  if (out_dist) HIPC(hipMemcpyAsync(out_dist, g->l2.odist, cnt * 4, hipMemcpyDeviceToHost, s));
  if (out_dist64) HIPC(hipMemcpyAsync(out_dist64, g->l2.odist64, cnt * 8, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  return MI_OK;
}

// the caller's host queries -> l2.qaug [nq][dp] on the handle's stream
static int l2_stage_queries(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t rs, int64_t cs) {
  int64_t elems;
  int rc = strided_extent(nq, g->ud, rs, cs, &elems);
  if (rc != MI_OK) return rc;
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  if ((rc = g->l2.qraw.grow((size_t)elems * esz)) != MI_OK) return rc;
  if ((rc = g->l2.qaug.grow((size_t)nq * g->dp)) != MI_OK) return rc;
  HIPC(hipMemcpyAsync(g->l2.qraw, q, (size_t)elems * esz, hipMemcpyHostToDevice, g->stream));
  launch_l2_augment(g->l2.qraw, dtype, nq, g->ud, rs, cs, g->l2.qaug, g->dp, g->stream);
  HIPC(hipGetLastError());
  return MI_OK;
}

extern "C" {

int mi_gallery_create_l2(const void* data, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride, int memspace,
                         int device, int64_t row_offset, int64_t capacity, mi_gallery** out) {
  REQUIRE(out, "null pointer");
  REQUIRE(n >= 0, "negative number of rows");
  REQUIRE(d >= 1, "d must be >= 1");
  REQUIRE(capacity >= 0, "negative capacity");
  REQUIRE(data || n == 0, "null pointer: data");
  REQUIRE(n >= 1 || capacity >= 1, "an empty gallery needs a capacity");
  return gallery_create_any(data, n, d, dtype, row_stride, col_stride, memspace, MI_NORM_NONE, MI_METRIC_L2, device, row_offset,
                            capacity, out);
}

int mi_knn_search_l2(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                     const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_dist, double* out_dist64,
                     mi_filter_info* out_info, double* out_seconds) {
  REQUIRE(g, "null handle");
  REQUIRE(k >= 1 && k <= 2048, "k must be in [1, 2048]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  REQUIRE(!allow_bits || allow_memspace == MI_HOST || allow_memspace == MI_DEVICE, "allow_memspace must be MI_HOST or MI_DEVICE");
  REQUIRE_L2(g);
  std::lock_guard<std::mutex> lock(g->mu);       // one section: selection (plain or filtered) and distance tail
  mi_filter_info info;
  std::memset(&info, 0, sizeof info);
  info.allowed = g->n;
  if (out_info) *out_info = info;
  if (out_seconds) *out_seconds = 0.0;
  if (nq == 0) return MI_OK;
  const auto t0 = std::chrono::steady_clock::now();
  const int32_t ud = g->ud;
  int rc;
  std::vector<int64_t> sel;          // filtered: the ids the filtered inner-product search returned, [nq][k], -1 padded
  if (allow_bits && g->n >= 1) {
    // the filtered search takes host queries: extended here, [nq][ud + 3] f32 (rounded to f32 as the query ingest would)
    std::vector<float> aug((size_t)nq * (ud + 3));
    for (int64_t i = 0; i < nq; ++i) {
      float* dst = aug.data() + (size_t)i * (ud + 3);
      for (int32_t c = 0; c < ud; ++c) {
        const int64_t o = i * row_stride + (int64_t)c * col_stride;
        dst[c] = dtype == MI_F32 ? ((const float*)q)[o] : (float)((const double*)q)[o];
      }
      dst[ud] = dst[ud + 1] = dst[ud + 2] = 1.0f;
    }
    sel.resize((size_t)nq * k);
    if ((rc = filtered_search_host(g, aug.data(), nq, MI_F32, ud + 3, 1, k, allow_bits, allow_memspace, sel.data(), nullptr, &info,
                                   nullptr, /*l2_caller=*/true)) != MI_OK)
      return rc;
    if (out_info) *out_info = info;
  }
  HIPC(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  if ((rc = l2_stage_queries(g, q, nq, dtype, row_stride, col_stride)) != MI_OK) return rc;
  int32_t ke = (int32_t)std::min<int64_t>(k, g->n);
  if (allow_bits && g->n >= 1) {
    ke = k;
    if ((rc = g->l2.ids.grow((size_t)nq * ke)) != MI_OK) return rc;
    HIPC(hipMemcpyAsync(g->l2.ids, sel.data(), (size_t)nq * ke * 8, hipMemcpyHostToDevice, s));
  } else if (ke >= 1) {
    if ((rc = g->l2.ids.grow((size_t)nq * ke)) != MI_OK) return rc;
    if ((rc = search_sync(g, g->l2.qaug, MI_F32, g->dp, 1, MI_NORM_NONE, nq, ke, g->l2.ids, nullptr, nullptr)) != MI_OK) return rc;
  }
  if ((rc = grow_all((size_t)nq * k, g->l2.oidx, g->l2.odist, g->l2.odist64)) != MI_OK) return rc;
  launch_l2_tail(g->gal_f32, g->l2.qaug, g->dp, ud, g->n, g->row_offset, g->l2.ids, ke, k, nq, g->l2.oidx, g->l2.odist,
                 g->l2.odist64, s);
  if ((rc = l2_copy_out(g, nq, k, out_idx, out_dist, out_dist64, s)) != MI_OK) return rc;
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return MI_OK;
}

int mi_knn_search_l2_device(mi_gallery* g, const float* q_dev, int64_t nq, int32_t k, int64_t* out_idx_dev, float* out_dist_dev,
                            double* out_dist64_dev, void* stream) {
  REQUIRE(g, "null handle");
  REQUIRE(q_dev && out_idx_dev, "null pointer");
  REQUIRE(nq >= 1, "no queries");
  REQUIRE(k >= 1 && k <= 2048, "k must be in [1, 2048]");
  REQUIRE_L2(g);
  HIPC(hipSetDevice(g->device));
  hipStream_t s = (hipStream_t)stream;
  const int32_t ke = (int32_t)std::min<int64_t>(k, g->n);
  int rc;
  if ((rc = g->l2.qaug.grow((size_t)nq * g->dp)) != MI_OK) return rc;
  if ((rc = g->l2.ids.grow((size_t)nq * std::max<int32_t>(ke, 1))) != MI_OK) return rc;
  launch_l2_augment(q_dev, MI_F32, nq, g->ud, g->ud, 1, g->l2.qaug, g->dp, s);
  if (ke >= 1 && (rc = search_device(g, g->l2.qaug, MI_F32, g->dp, 1, MI_NORM_NONE, nq, ke, g->l2.ids, nullptr, nullptr,
                                     g->force_exact != 0, s, /*allow_async=*/false, /*caller_checks_flags=*/false)) != MI_OK)
    return rc;
  launch_l2_tail(g->gal_f32, g->l2.qaug, g->dp, g->ud, g->n, g->row_offset, g->l2.ids, ke, k, nq, out_idx_dev, out_dist_dev,
                 out_dist64_dev, s);
  HIPC(hipGetLastError());
  return MI_OK;
}

int mi_knn_dense64_search_l2(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                             int64_t* out_idx, float* out_dist, double* out_dist64, double* out_seconds) {
  REQUIRE(g, "null handle");
  REQUIRE(q && out_idx, "null pointer");
  REQUIRE(nq >= 1, "no queries");
  REQUIRE(k >= 1 && k <= 4096, "k must be in [1, 4096]");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  REQUIRE_L2(g);
  std::lock_guard<std::mutex> lock(g->mu);
  HIPC(hipSetDevice(g->device));
  const auto t0 = std::chrono::steady_clock::now();
  hipStream_t s = g->stream;
  int rc;
  if ((rc = join_tails(g, s)) != MI_OK) return rc;
  if ((rc = l2_stage_queries(g, q, nq, dtype, row_stride, col_stride)) != MI_OK) return rc;
  if ((rc = grow_all((size_t)nq * k, g->l2.oidx, g->l2.odist, g->l2.odist64)) != MI_OK) return rc;
  const int32_t ke = (int32_t)std::min<int64_t>(k, g->n);
  TmpAlloc tmp;
  if (ke >= 1) {
    // every direct-form distance of a sub-batch of queries (<= 2 GiB at a time), no threshold anywhere, then the exact top-k
    const int64_t qb = std::min<int64_t>(QB, std::max<int64_t>(16, ((int64_t)1 << 28) / g->n));
    double* dense = tmp.get<double>((size_t)std::min<int64_t>(qb, nq) * g->n);
    int64_t* tidx = tmp.get<int64_t>((size_t)nq * ke);
    double* tneg = tmp.get<double>((size_t)nq * ke);
    if (!dense || !tidx || !tneg) return fail(MI_ERR_NOMEM, "dense f64 distance buffer");
    for (int64_t q0 = 0; q0 < nq; q0 += qb) {
      const int32_t b = (int32_t)std::min<int64_t>(qb, nq - q0);
      launch_l2_dense_dist(g->gal_f32, g->l2.qaug + (size_t)q0 * g->dp, g->dp, g->ud, g->n, b, dense, g->n, s);
      launch_dense_topk64(dense, g->n, g->n, b, ke, g->row_offset, tidx + q0 * ke, nullptr, tneg + q0 * ke, s);
    }
    launch_l2_dense_emit(tidx, tneg, nq, ke, k, g->l2.oidx, g->l2.odist, g->l2.odist64, s);
  } else {
    launch_l2_dense_emit(nullptr, nullptr, nq, 0, k, g->l2.oidx, g->l2.odist, g->l2.odist64, s);
  }
  if ((rc = l2_copy_out(g, nq, k, out_idx, out_dist, out_dist64, s)) != MI_OK) return rc;      // (synchronises: `tmp` is freed on return)
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return MI_OK;
}

}  // extern "C"
