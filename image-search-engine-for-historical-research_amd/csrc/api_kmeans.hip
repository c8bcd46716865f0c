// k-means over whole rows of the C ABI (kernels in csrc/kmeans.hip): mi_kmeans_train is mi_pqw_train with m = 1,
// word for word and bit for bit, with the assignment of every iteration done by launch_km_assign -- an f64 MFMA kernel decides the
// rows its rounding certificate covers, the direct-form kernel the rest -- and init, move count and update those of pq_train.hip on
// uint16 codes.  mi_kmeans_assign / mi_kmeans_assign_device are the assignment alone, int32 ids.  No handle.
#include "api_internal.h"

namespace {

constexpr int64_t KM_WS_BYTES = (int64_t)64 << 20;     // the triples of a chunk of rows: 51 840 rows at k = 8192, 2.1 M at k = 128

int km_check(int64_t n, int32_t d, int dtype, int64_t rs, int64_t cs, int32_t k) {
  if (n < 0) return fail(MI_ERR_INVALID, "negative number of rows: n");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  REQUIRE(rs >= 0 && cs >= 0, "negative strides are not supported");
  REQUIRE(k >= 2 && k <= PQW_MAX_KS, "k (centroids) must be in [2, 8192]");
  REQUIRE(d >= 1 && d <= 4096, "d must be in [1, 4096]");
  return MI_OK;
}

// the workspace of a call that owns one: chunks of at most `n` rows within KM_WS_BYTES, 128 rows at the least
int km_own_workspace(TmpAlloc& tmp, int32_t k, int64_t n, KmWorkspace* w) {
  const int64_t bytes = std::max(km_workspace_bytes(k, 128), std::min(km_workspace_bytes(k, n), KM_WS_BYTES));
  char* p = tmp.get<char>((size_t)bytes);
  if (!p) return fail(MI_ERR_NOMEM, "k-means workspace");
  *w = km_workspace(p, bytes, k);
  return MI_OK;
}

}  // namespace

extern "C" {

int mi_kmeans_train(const void* x, int64_t n, int32_t d, int x_dtype, int64_t row_stride, int64_t col_stride, int memspace, int32_t k,
                    int32_t iters, const float* init_centroids_host, int device, float* out_centroids_host, int64_t* out_moved,
                    int64_t* out_flagged, double* out_seconds) {
  const int dtype = x_dtype;
  REQUIRE(x, "null pointer: rows");
  REQUIRE(out_centroids_host, "null pointer: out_centroids_host");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  int rc = km_check(n, d, dtype, row_stride, col_stride, k);
  if (rc != MI_OK) return rc;
  REQUIRE(n >= k, "training needs at least k rows (n >= k)");
  REQUIRE(iters >= 1, "iters must be >= 1");
  const size_t cb_count = (size_t)k * d;
  if (init_centroids_host)
    for (size_t i = 0; i < cb_count; ++i) REQUIRE(std::isfinite(init_centroids_host[i]), "initial centroids must be finite");
  if (memspace == MI_HOST) {
    const bool finite = dtype == MI_F32 ? pq_all_finite((const float*)x, n, d, row_stride, col_stride)
                                        : pq_all_finite((const double*)x, n, d, row_stride, col_stride);
    REQUIRE(finite, "training rows must be finite");
  }
  const auto t0 = std::chrono::steady_clock::now();
  if (out_seconds) *out_seconds = 0.0;
  TrainTimes& times = train_times();
  times.assign_ms.clear();
  times.update_ms.clear();
  HIPC(hipSetDevice(device));
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  const size_t code_bytes = (size_t)n * sizeof(uint16_t);
  TmpAlloc tmp;                                        // (freed after w has drained its stream)
  TrainScratch<uint16_t> w;
  HIPC(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
  for (hipEvent_t& e : w.ev) HIPC(hipEventCreate(&e));
  if (memspace == MI_HOST) HIPC(device_malloc(&w.xdev, (size_t)n * d * esz));
  HIPC(device_malloc((void**)&w.codes[0], code_bytes));
  HIPC(device_malloc((void**)&w.codes[1], code_bytes));
  HIPC(device_malloc((void**)&w.cols, code_bytes));
  HIPC(device_malloc((void**)&w.cb, cb_count * 4));
  HIPC(device_malloc((void**)&w.moved, 256));          // [0] moved, [1] flagged
  KmWorkspace ws;
  if ((rc = km_own_workspace(tmp, k, n, &ws)) != MI_OK) return rc;
  hipStream_t s = w.stream;
  const void* xd = x;
  int64_t rs = row_stride, cs = col_stride;
  if (memspace == MI_HOST) {
    if ((rc = train_upload(w, x, n, d, esz, row_stride, col_stride)) != MI_OK) return rc;
    xd = w.xdev;
    rs = d;
    cs = 1;
  }
  if (init_centroids_host) HIPC(hipMemcpyAsync(w.cb, init_centroids_host, cb_count * 4, hipMemcpyHostToDevice, s));
  else launch_pq_init_rows(xd, dtype, rs, cs, n, 1, k, d, w.cb, s);
  HIPC(hipGetLastError());

  int32_t t = 0;
  bool update_pending = false;                         // an update whose events have not been read yet
  auto read_update = [&]() -> int {
    if (!update_pending) return MI_OK;
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, w.ev[2], w.ev[3]));
    times.update_ms.push_back(ms);
    update_pending = false;
    return MI_OK;
  };
  for (; t < iters; ++t) {
    uint16_t* cur = w.codes[t & 1];
    const uint16_t* prev = w.codes[(t & 1) ^ 1];
    unsigned long long counts[2] = {0ull, 0ull};       // moved, flagged
    HIPC(hipEventRecord(w.ev[0], s));
    HIPC(hipMemsetAsync(w.moved, 0, 16, s));
    launch_km_assign(xd, dtype, n, d, rs, cs, w.cb, k, cur, w.moved + 1, ws, s);
    if (t > 0) launch_pq_moved(cur, prev, (int64_t)code_bytes, w.moved, s);
    HIPC(hipMemcpyAsync(counts, w.moved, 16, hipMemcpyDeviceToHost, s));
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(w.ev[1], s));
    HIPC(hipStreamSynchronize(s));
    if (t == 0) counts[0] = (unsigned long long)n;     // moved[0] = n: there is no assignment before the first
    if ((rc = read_update()) != MI_OK) return rc;
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
    times.assign_ms.push_back(ms);
    if (out_moved) out_moved[t] = (int64_t)counts[0];
    if (out_flagged) out_flagged[t] = (int64_t)counts[1];
    if (t > 0 && counts[0] == 0) break;                // the same members give the same sums: C_iters = C_t
    HIPC(hipEventRecord(w.ev[2], s));
    launch_pq_code_columns(cur, 1, n, w.cols, s);
    launch_pq_update(xd, dtype, rs, cs, n, w.cols, 1, k, d, w.cb, s);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(w.ev[3], s));
    update_pending = true;
  }
  for (int32_t u = t + 1; u < iters; ++u) {
    if (out_moved) out_moved[u] = 0;
    if (out_flagged) out_flagged[u] = 0;
  }
  HIPC(hipMemcpyAsync(out_centroids_host, w.cb, cb_count * 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  if ((rc = read_update()) != MI_OK) return rc;
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return MI_OK;
}

int mi_kmeans_assign_workspace_bytes(int32_t k, int64_t n, int64_t* out_bytes) {
  REQUIRE(out_bytes, "null pointer: out_bytes");
  REQUIRE(k >= 2 && k <= PQW_MAX_KS, "k (centroids) must be in [2, 8192]");
  REQUIRE(n >= 0, "negative number of rows: n");
  *out_bytes = std::max(km_workspace_bytes(k, 128), std::min(km_workspace_bytes(k, n), KM_WS_BYTES));
  return MI_OK;
}

int mi_kmeans_assign_device(const void* x_dev, int64_t n, int32_t d, int x_dtype, int64_t row_stride, int64_t col_stride,
                            const float* centroids_dev, int32_t k, int32_t* out_ids_dev, uint64_t* out_flagged_dev,
                            void* workspace_dev, int64_t workspace_bytes, void* stream) {
  const int dtype = x_dtype;
  const int rc = km_check(n, d, dtype, row_stride, col_stride, k);
  if (rc != MI_OK) return rc;
  REQUIRE(centroids_dev, "null pointer: centroids_dev");
  REQUIRE(workspace_dev, "null pointer: workspace_dev");
  REQUIRE((reinterpret_cast<uintptr_t>(workspace_dev) & 7u) == 0, "workspace_dev must be 8-byte aligned");
  const KmWorkspace ws = km_workspace(workspace_dev, workspace_bytes, k);
  REQUIRE(ws.rows >= 128, "workspace_bytes below what 128 rows need (mi_kmeans_assign_workspace_bytes)");
  hipStream_t s = (hipStream_t)stream;
  if (out_flagged_dev) HIPC(hipMemsetAsync(out_flagged_dev, 0, 8, s));
  if (n == 0) return MI_OK;
  REQUIRE(x_dev, "null pointer: x_dev");
  REQUIRE(out_ids_dev, "null pointer: out_ids_dev");
  launch_km_assign(x_dev, dtype, n, d, row_stride, col_stride, centroids_dev, k, out_ids_dev,
                   reinterpret_cast<unsigned long long*>(out_flagged_dev), ws, s);
  HIPC(hipGetLastError());
  return MI_OK;
}

int mi_kmeans_assign(const void* x, int64_t n, int32_t d, int x_dtype, int64_t row_stride, int64_t col_stride,
                     const float* centroids_host, int32_t k, int device, int32_t* out_ids, int64_t* out_flagged) {
  const int dtype = x_dtype;
  int rc = km_check(n, d, dtype, row_stride, col_stride, k);
  if (rc != MI_OK) return rc;
  REQUIRE(centroids_host, "null pointer: centroids_host");
  for (size_t i = 0; i < (size_t)k * d; ++i) REQUIRE(std::isfinite(centroids_host[i]), "centroids must be finite");
  if (out_flagged) *out_flagged = 0;
  if (n == 0) return MI_OK;
  REQUIRE(x, "null pointer: x");
  REQUIRE(out_ids, "null pointer: out_ids");
  const bool finite = dtype == MI_F32 ? pq_all_finite((const float*)x, n, d, row_stride, col_stride)
                                      : pq_all_finite((const double*)x, n, d, row_stride, col_stride);
  REQUIRE(finite, "rows must be finite");
  HIPC(hipSetDevice(device));
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  // rows pass through the device in blocks of at most 64 MiB of descriptors, as in mi_lsh_encode (no id depends on where a block
  // ends: a row's answer is its own)
  const int64_t step = std::max<int64_t>(128, ((int64_t)64 << 20) / ((int64_t)d * (int64_t)esz) / 128 * 128);
  const int64_t blk = std::min(step, n);
  TmpAlloc tmp;
  char* xd = tmp.get<char>((size_t)blk * d * esz);
  float* cd = tmp.get<float>((size_t)k * d);
  int32_t* od = tmp.get<int32_t>((size_t)blk);
  unsigned long long* fd = tmp.get<unsigned long long>(1);
  if (!xd || !cd || !od || !fd) return fail(MI_ERR_NOMEM, "k-means assign buffers");
  KmWorkspace ws;
  if ((rc = km_own_workspace(tmp, k, blk, &ws)) != MI_OK) return rc;
  HIPC(hipMemcpy(cd, centroids_host, (size_t)k * d * 4, hipMemcpyHostToDevice));
  HIPC(hipMemset(fd, 0, 8));
  const bool packed = col_stride == 1 && (row_stride == d || n == 1);
  std::vector<char> pack;
  for (int64_t r = 0; r < n; r += step) {
    const int64_t mm = std::min(step, n - r);
    const char* src = (const char*)x + (size_t)r * (size_t)row_stride * esz;
    if (!packed) {                                          // any other layout: the block is packed on the host first
      pack.resize((size_t)mm * d * esz);
      for (int64_t i = 0; i < mm; ++i)
        for (int32_t c = 0; c < d; ++c)
          std::memcpy(pack.data() + ((size_t)i * d + c) * esz, src + ((size_t)i * row_stride + (size_t)c * col_stride) * esz, esz);
      src = pack.data();
    }
    HIPC(hipMemcpy(xd, src, (size_t)mm * d * esz, hipMemcpyHostToDevice));
    launch_km_assign(xd, dtype, mm, d, d, 1, cd, k, od, fd, ws, nullptr);
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(out_ids + r, od, (size_t)mm * 4, hipMemcpyDeviceToHost));   // (synchronous: xd and od are free again)
  }
  unsigned long long flagged = 0;
  HIPC(hipMemcpy(&flagged, fd, 8, hipMemcpyDeviceToHost));
  if (out_flagged) *out_flagged = (int64_t)flagged;
  return MI_OK;
}

}  // extern "C"
