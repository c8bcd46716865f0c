// Exact re-ranking of index shortlists on the stored rows of a gallery (faiss IndexRefineFlat): mi_refine / mi_refine_device.
// DESIGN.md 5.15.  The candidates come from any index -- PQ, IVF-PQ, Hamming, LSH -- as global ids; the metric is the rows
// gallery's: direct-form squared distances on an L2 gallery (the bits of mi_knn_search_l2), inner products against the stored row
// on any other.  Kernels in refine.hip: one gather launch over (slab of candidates, query), one sort workgroup per query.
#include "api_internal.h"

// the argument checks both forms share: they answer before the handle is read
static int refine_check(const mi_gallery* g, int64_t nq, int32_t kc, int64_t cand_stride, int32_t k) {
  REQUIRE(g, "null handle");
  REQUIRE(kc >= 1 && kc <= REFINE_MAX_KC, "kc must be in [1, 8192]");
  REQUIRE(k >= 1 && k <= kc, "k must be in [1, kc]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(cand_stride >= kc, "cand_stride must be >= kc");
  return MI_OK;
}

// queries [nq][dp] in r.qpad (from `src`, device memory, any strides) + the value workspace, then the two launches on `s`
static int refine_enqueue(mi_gallery* g, const void* src, int dtype, int64_t rs, int64_t cs, int64_t nq, const int64_t* cand_dev,
                          int32_t kc, int64_t cand_stride, int32_t k, int64_t* out_idx, float* out_val, double* out_val64,
                          hipStream_t s) {
  auto& r = g->refine;
  int rc;
  if ((rc = r.qpad.grow((size_t)nq * g->dp)) != MI_OK) return rc;
  if ((rc = r.val.grow((size_t)nq * kc)) != MI_OK) return rc;
  // rows of stride dp, the caller's ud columns (what follows them is never read: both wave sums stop at ud)
  launch_l2_augment(src, dtype, nq, g->ud, rs, cs, r.qpad, g->dp, s);
  launch_refine(g->gal_f32, r.qpad, g->dp, g->ud, g->n, g->row_offset, g->metric == MI_METRIC_L2 ? 1 : 0, cand_dev, kc, cand_stride,
                k, nq, r.val, out_idx, out_val, out_val64, s);
  HIPC(hipGetLastError());
  return MI_OK;
}

extern "C" {

int mi_refine_device(mi_gallery* rows, const float* q_dev, int64_t nq, const int64_t* cand_dev, int32_t kc, int64_t cand_stride,
                     int32_t k, int64_t* out_idx_dev, float* out_val_dev, double* out_val64_dev, void* stream) {
  int rc = refine_check(rows, nq, kc, cand_stride, k);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q_dev, "null pointer: queries");
  REQUIRE(nq == 0 || cand_dev, "null pointer: candidates");
  REQUIRE(nq == 0 || out_idx_dev, "null pointer: out_idx");
  if (nq == 0) return MI_OK;
  HIPC(hipSetDevice(rows->device));
  return refine_enqueue(rows, q_dev, MI_F32, rows->ud, 1, nq, cand_dev, kc, cand_stride, k, out_idx_dev, out_val_dev, out_val64_dev,
                        (hipStream_t)stream);
}

int mi_refine(mi_gallery* rows, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, const int64_t* cand,
              int32_t kc, int64_t cand_stride, int32_t k, int64_t* out_idx, float* out_val, double* out_val64, double* out_seconds) {
  int rc = refine_check(rows, nq, kc, cand_stride, k);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(nq == 0 || cand, "null pointer: candidates");
  REQUIRE(nq == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  if (out_seconds) *out_seconds = 0.0;
  if (nq == 0) return MI_OK;
  mi_gallery* g = rows;
  std::lock_guard<std::mutex> lock(g->mu);
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  auto& r = g->refine;
  int64_t elems;
  if ((rc = strided_extent(nq, g->ud, row_stride, col_stride, &elems)) != MI_OK) return rc;
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  if ((rc = r.qraw.grow((size_t)elems * esz)) != MI_OK) return rc;
  if ((rc = r.cand.grow((size_t)nq * kc)) != MI_OK) return rc;
  if ((rc = grow_all((size_t)nq * k, r.oidx, r.oval, r.oval64)) != MI_OK) return rc;
  HIPC(hipMemcpyAsync(r.qraw, q, (size_t)elems * esz, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpy2DAsync(r.cand, (size_t)kc * 8, cand, (size_t)cand_stride * 8, (size_t)kc * 8, (size_t)nq, hipMemcpyHostToDevice, s));
  if ((rc = refine_enqueue(g, r.qraw, dtype, row_stride, col_stride, nq, r.cand, kc, kc, k, r.oidx, r.oval, r.oval64, s)) != MI_OK)
    return rc;
  const size_t cnt = (size_t)nq * k;
  HIPC(hipMemcpyAsync(out_idx, r.oidx, cnt * 8, hipMemcpyDeviceToHost, s));
  if (out_val) HIPC(hipMemcpyAsync(out_val, r.oval, cnt * 4, hipMemcpyDeviceToHost, s));
  if (out_val64) HIPC(hipMemcpyAsync(out_val64, r.oval64, cnt * 8, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return MI_OK;
}

int mi_debug_l2_tail_device(mi_gallery* g, const float* q_dev, int64_t nq, const int64_t* ids_dev, int32_t ke, int32_t k,
                            int64_t* out_idx_dev, double* out_dist64_dev, void* stream) {
  REQUIRE(g, "null handle");
  REQUIRE(q_dev && ids_dev && out_idx_dev, "null pointer");
  REQUIRE(nq >= 1, "no queries");
  REQUIRE(k >= 1 && k <= 2048 && ke >= 0 && ke <= k, "k must be in [1, 2048] and ke in [0, k]");
  REQUIRE(g->metric == MI_METRIC_L2, "not a squared-L2 gallery (mi_gallery_create_l2)");
  HIPC(hipSetDevice(g->device));
  int rc;
  if ((rc = g->refine.qpad.grow((size_t)nq * g->dp)) != MI_OK) return rc;
  launch_l2_augment(q_dev, MI_F32, nq, g->ud, g->ud, 1, g->refine.qpad, g->dp, (hipStream_t)stream);
  launch_l2_tail(g->gal_f32, g->refine.qpad, g->dp, g->ud, g->n, g->row_offset, ids_dev, ke, k, nq, out_idx_dev, nullptr,
                 out_dist64_dev, (hipStream_t)stream);
  HIPC(hipGetLastError());
  return MI_OK;
}

}  // extern "C"
