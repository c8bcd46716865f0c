// Learning PQ codebooks of the C ABI: mi_pq_train and, on uint16 codes with Ks <= 8192, mi_pqw_train -- one body, the code type
// a template argument (kernels in csrc/pq_train.hip and pq_encode_kernel of csrc/pq.hip).  scipy.cluster.vq.kmeans2(minit="matrix") per book -- what nanopq.PQ.fit runs -- made reproducible on the device:
// Lloyd's iteration from given centroids, every operation an IEEE float64 operation in a fixed order, centroids rounded to
// float32 after every iteration.  No handle: the call owns a stream and its buffers and frees them before it returns.
#include "api_internal.h"

namespace {

// the training proper; ks_max and ks_msg are the entry point's limit on ks
template <typename CodeT>
int train_run(const void* x, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride, int memspace, int32_t m,
              int32_t ks, int32_t ks_max, const char* ks_msg, int32_t iters, const float* init_codebooks_host, int device,
              float* out_codebooks_host, int64_t* out_moved, double* out_seconds) {
  REQUIRE(x, "null pointer: rows");
  REQUIRE(out_codebooks_host, "null pointer: out_codebooks_host");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  REQUIRE(row_stride >= 0 && col_stride >= 0, "negative strides are not supported");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  REQUIRE(m >= 1 && m <= 64, "m (books) must be in [1, 64]");
  REQUIRE(ks >= 2 && ks <= ks_max, ks_msg);
  REQUIRE(d >= 1 && d <= 4096, "d must be in [1, 4096]");
  REQUIRE(d % m == 0, "d must be a multiple of m");
  REQUIRE(n >= ks, "training needs at least ks rows (n >= ks)");
  REQUIRE(iters >= 1, "iters must be >= 1");
  const size_t cb_count = (size_t)ks * d;
  if (init_codebooks_host)
    for (size_t i = 0; i < cb_count; ++i) REQUIRE(std::isfinite(init_codebooks_host[i]), "initial codebooks must be finite");
  if (memspace == MI_HOST) {
    const bool finite = dtype == MI_F32 ? pq_all_finite((const float*)x, n, d, row_stride, col_stride)
                                        : pq_all_finite((const double*)x, n, d, row_stride, col_stride);
    REQUIRE(finite, "training rows must be finite");
  }
  const auto t0 = std::chrono::steady_clock::now();
  if (out_seconds) *out_seconds = 0.0;
  train_times().assign_ms.clear();
  train_times().update_ms.clear();
  HIPC(hipSetDevice(device));
  const int32_t L = d / m;
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  const size_t code_bytes = (size_t)n * m * sizeof(CodeT);
  TrainScratch<CodeT> w;
  HIPC(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
  for (hipEvent_t& e : w.ev) HIPC(hipEventCreate(&e));
  if (memspace == MI_HOST) HIPC(device_malloc(&w.xdev, (size_t)n * d * esz));
  HIPC(device_malloc((void**)&w.codes[0], code_bytes));
  HIPC(device_malloc((void**)&w.codes[1], code_bytes));
  HIPC(device_malloc((void**)&w.cols, code_bytes));
  HIPC(device_malloc((void**)&w.cb, cb_count * 4));
  HIPC(device_malloc((void**)&w.moved, 256));
  hipStream_t s = w.stream;
  const void* xd = x;
  int64_t rs = row_stride, cs = col_stride;
  if (memspace == MI_HOST) {
    int rc;
    if ((rc = train_upload(w, x, n, d, esz, row_stride, col_stride)) != MI_OK) return rc;
    xd = w.xdev;
    rs = d;
    cs = 1;
  }
  if (init_codebooks_host) HIPC(hipMemcpyAsync(w.cb, init_codebooks_host, cb_count * 4, hipMemcpyHostToDevice, s));
  else launch_pq_init_rows(xd, dtype, rs, cs, n, m, ks, L, w.cb, s);
  HIPC(hipGetLastError());

  int32_t t = 0;
  bool update_pending = false;                         // an update whose events have not been read yet
  auto read_update = [&]() -> int {
    if (!update_pending) return MI_OK;
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, w.ev[2], w.ev[3]));
    train_times().update_ms.push_back(ms);
    update_pending = false;
    return MI_OK;
  };
  for (; t < iters; ++t) {
    CodeT* cur = w.codes[t & 1];
    const CodeT* prev = w.codes[(t & 1) ^ 1];
    unsigned long long moved = (unsigned long long)n * (unsigned long long)m;
    HIPC(hipEventRecord(w.ev[0], s));
    launch_pq_encode(xd, dtype, rs, cs, n, w.cb, m, ks, L, cur, s);
    if (t > 0) {
      HIPC(hipMemsetAsync(w.moved, 0, 8, s));
      launch_pq_moved(cur, prev, (int64_t)code_bytes, w.moved, s);
      HIPC(hipMemcpyAsync(&moved, w.moved, 8, hipMemcpyDeviceToHost, s));
    }
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(w.ev[1], s));
    HIPC(hipStreamSynchronize(s));
    int rc;
    if ((rc = read_update()) != MI_OK) return rc;
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
    train_times().assign_ms.push_back(ms);
    if (out_moved) out_moved[t] = (int64_t)moved;
    if (t > 0 && moved == 0) break;                    // the same members give the same sums: C_iters = C_t
    HIPC(hipEventRecord(w.ev[2], s));
    launch_pq_code_columns(cur, m, n, w.cols, s);
    launch_pq_update(xd, dtype, rs, cs, n, w.cols, m, ks, L, w.cb, s);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(w.ev[3], s));
    update_pending = true;
  }
  if (out_moved)
    for (int32_t u = t + 1; u < iters; ++u) out_moved[u] = 0;
  HIPC(hipMemcpyAsync(out_codebooks_host, w.cb, cb_count * 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  int rc;
  if ((rc = read_update()) != MI_OK) return rc;
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return MI_OK;
}

}  // namespace

TrainTimes& train_times() {
  thread_local TrainTimes t;
  return t;
}

extern "C" {

int mi_pq_train(const void* x, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride, int memspace, int32_t m,
                int32_t ks, int32_t iters, const float* init_codebooks_host, int device, float* out_codebooks_host, int64_t* out_moved,
                double* out_seconds) {
  return train_run<uint8_t>(x, n, d, dtype, row_stride, col_stride, memspace, m, ks, 256, "ks (codewords per book) must be in [2, 256]",
                            iters, init_codebooks_host, device, out_codebooks_host, out_moved, out_seconds);
}

int mi_pqw_train(const void* x, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride, int memspace, int32_t m,
                 int32_t ks, int32_t iters, const float* init_codebooks_host, int device, float* out_codebooks_host, int64_t* out_moved,
                 double* out_seconds) {
  return train_run<uint16_t>(x, n, d, dtype, row_stride, col_stride, memspace, m, ks, PQW_MAX_KS,
                             "ks (codewords per book) must be in [2, 8192]", iters, init_codebooks_host, device, out_codebooks_host,
                             out_moved, out_seconds);
}

int mi_pq_train_timing(int32_t capacity, float* out_assign_ms, float* out_update_ms, int32_t* out_assignments, int32_t* out_updates) {
  REQUIRE(capacity >= 0, "negative capacity");
  REQUIRE(capacity == 0 || (out_assign_ms && out_update_ms), "null pointer");
  for (int32_t i = 0; i < capacity && i < (int32_t)train_times().assign_ms.size(); ++i) out_assign_ms[i] = train_times().assign_ms[i];
  for (int32_t i = 0; i < capacity && i < (int32_t)train_times().update_ms.size(); ++i) out_update_ms[i] = train_times().update_ms[i];
  if (out_assignments) *out_assignments = (int32_t)train_times().assign_ms.size();
  if (out_updates) *out_updates = (int32_t)train_times().update_ms.size();
  return MI_OK;
}

}  // extern "C"
