// Wide PQ index of the C ABI: exact ADC top-K on product-quantized codes of up to 8192 codewords per book (mi_pqw; kernels in
// csrc/pq_wide.hip, tables / encoder / selection / emit in csrc/pq.hip and dense.hip).  The reference's
// matching_Nano_PQ as its entry points call it: N_books = 16, n_bits_perbook = 13 (src/offline.py:110).  mi_pq entry point for
// entry point, with uint16 codes: the contract -- table entries, float32 sums in book order, order by (distance, id), the encoder's
// argmin -- is mi_pq's word for word, and for ks <= 256 so is every output bit.  Training is mi_pqw_train (api_pq_train.hip).
#include "api_internal.h"

namespace {

// the first m codes of every row are below `limit`
bool wide_codes_below(const uint16_t* p, int64_t rows, int64_t stride, int32_t m, int32_t limit) {
  for (int64_t r = 0; r < rows; ++r)
    for (int32_t b = 0; b < m; ++b)
      if (p[r * stride + b] >= limit) return false;
  return true;
}

// rows of codes, `stride` uint16 apart (host: checked by the caller; device: checked here) -> rows n .. n + rows of the index,
// synchronous on the handle's stream.  A device code >= ks: MI_ERR_INVALID, nothing written.
int pqw_ingest(mi_pqw* h, const void* codes, int64_t rows, int64_t stride, int memspace) {
  hipStream_t s = h->stream;
  if (memspace == MI_DEVICE) {
    uint32_t f = 0;
    launch_pqw_check((const uint16_t*)codes, stride, h->m, h->ks, rows, h->flag, s);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(&f, h->flag, 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (f) {
      HIPC(hipMemsetAsync(h->flag, 0, 4, s));
      HIPC(hipStreamSynchronize(s));
      return fail(MI_ERR_INVALID, "a code is >= ks");
    }
    launch_pqw_ingest((const uint16_t*)codes, stride, h->m, h->n, rows, h->codes, s);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    return MI_OK;
  }
  const int64_t step = std::max<int64_t>(1, ((int64_t)32 << 20) / h->m);
  int rc;
  if ((rc = h->cwords.grow((size_t)std::min(step, rows) * h->m)) != MI_OK) return rc;
  for (int64_t r = 0; r < rows; r += step) {
    const int64_t mm = std::min(step, rows - r);
    const uint16_t* src = (const uint16_t*)codes + r * stride;
    if (stride == h->m || mm == 1) HIPC(hipMemcpyAsync(h->cwords, src, (size_t)mm * h->m * 2, hipMemcpyHostToDevice, s));
    else HIPC(hipMemcpy2DAsync(h->cwords, (size_t)h->m * 2, src, (size_t)stride * 2, (size_t)h->m * 2, (size_t)mm, hipMemcpyHostToDevice, s));
    launch_pqw_ingest(h->cwords, h->m, h->m, h->n + r, mm, h->codes, s);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));                 // the staging buffer is reused by the next block
  }
  return MI_OK;
}

// encodes `rows` rows (host or device) in blocks; after each block `sink(r, mm)` consumes the packed codes of rows r .. r + mm in
// h->cwords.  Synchronous on the handle's stream.
template <typename Sink>
int pqw_encode_blocks(mi_pqw* h, const void* x, int64_t rows, int dtype, int64_t rs, int64_t cs, int memspace, Sink sink) {
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  const int64_t step = std::max<int64_t>(64, ((int64_t)64 << 20) / ((int64_t)h->d * (int64_t)esz));
  hipStream_t s = h->stream;
  int rc;
  if ((rc = h->cwords.grow((size_t)std::min(step, rows) * h->m)) != MI_OK) return rc;
  std::vector<char> pack;
  for (int64_t r = 0; r < rows; r += step) {
    const int64_t mm = std::min(step, rows - r);
    if (memspace == MI_HOST) {
      if ((rc = stage_host_rows(h->xraw, h->d, h->stream, x, r, mm, dtype, rs, cs, pack)) != MI_OK) return rc;
      launch_pq_encode(h->xraw, dtype, h->d, 1, mm, h->cb, h->m, h->ks, h->L, h->cwords.get(), s);
    } else {
      launch_pq_encode((const char*)x + (size_t)r * rs * esz, dtype, rs, cs, mm, h->cb, h->m, h->ks, h->L, h->cwords.get(), s);
    }
    HIPC(hipGetLastError());
    if ((rc = sink(r, mm)) != MI_OK) return rc;
  }
  return MI_OK;
}

// the search proper on stream s: queries on the device (any strides), results go to device buffers
int pqw_search_core(mi_pqw* h, const void* q_dev, int dtype, int64_t rs, int64_t cs, int64_t nq, int32_t k, const uint64_t* allow_dev,
                    int64_t* out_idx_dev, float* out_dist_dev, hipStream_t s) {
  const int64_t npad = round_up(h->n, 64);
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  if (npad == 0) {
    launch_pq_emit(nullptr, nullptr, nq, 0, k, h->row_offset, out_idx_dev, out_dist_dev, s);
    HIPC(hipGetLastError());
    return MI_OK;
  }
  // queries per pass: the matrix within "pq_matrix_bytes" and the tables (512 KiB a query at 16 x 8192) within 1 GiB, whole tiles
  // of 4, one tile at the least
  const int64_t per = (int64_t)h->m * h->ks;
  const int64_t budget = g_pq_matrix_bytes.load();
  int64_t qc = std::min<int64_t>({nq, budget / (npad * 4), ((int64_t)1 << 30) / (per * 4), (int64_t)1 << 20});
  qc = std::max<int64_t>(4, qc / 4 * 4);
  qc = std::min(qc, nq);
  const int32_t ke = (int32_t)std::min<int64_t>(k, npad);
  int rc;
  if ((rc = h->tab.grow((size_t)(qc * per))) != MI_OK) return rc;
  if ((rc = h->mat.grow((size_t)(qc * npad))) != MI_OK) return rc;
  if ((rc = h->tidx.grow((size_t)(qc * ke))) != MI_OK) return rc;
  if ((rc = h->tneg.grow((size_t)(qc * ke))) != MI_OK) return rc;
  for (int64_t q0 = 0; q0 < nq; q0 += qc) {
    const int32_t b = (int32_t)std::min<int64_t>(qc, nq - q0);
    launch_pq_table((const char*)q_dev + (size_t)q0 * rs * esz, dtype, rs, cs, b, h->cb, h->m, h->ks, h->L, h->tab, s);
    launch_pqw_scan(h->codes, h->m, h->ks, h->n, h->tab, b, pqw_query_tile(h->ks, b), allow_dev, h->mat, s);
    launch_dense_topk(h->mat, npad, npad, b, ke, 0, h->tidx, h->tneg, s);
    launch_pq_emit(h->tidx, h->tneg, b, ke, k, h->row_offset, out_idx_dev + q0 * k, out_dist_dev ? out_dist_dev + q0 * k : nullptr, s);
  }
  HIPC(hipGetLastError());
  return MI_OK;
}

}  // namespace

extern "C" {

int mi_pqw_create(const float* codebooks_host, int32_t d, int32_t m, int32_t ks, const void* codes, int64_t n, int64_t row_stride,
                  int memspace, int device, int64_t row_offset, int64_t capacity, mi_pqw** out) {
  REQUIRE(out, "null pointer: out");
  REQUIRE(codebooks_host, "null pointer: codebooks_host");
  REQUIRE(m >= 1 && m <= 64, "m (books) must be in [1, 64]");
  REQUIRE(ks >= 2 && ks <= PQW_MAX_KS, "ks (codewords per book) must be in [2, 8192]");
  REQUIRE(d >= 1 && d <= 4096, "d must be in [1, 4096]");
  REQUIRE(d % m == 0, "d must be a multiple of m");
  REQUIRE(n >= 0, "negative number of rows");
  REQUIRE(capacity >= 0, "negative capacity");
  REQUIRE(capacity == 0 || capacity >= n, "capacity below the number of rows");
  REQUIRE(codes || n == 0, "null pointer: codes");
  REQUIRE(n >= 1 || capacity >= 1, "an empty index needs a capacity");
  REQUIRE(n == 0 || row_stride >= m, "row_stride below m");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  if (capacity == 0) capacity = n;
  REQUIRE(capacity < ((int64_t)1 << 32) - 64, "an index holds fewer than 2^32 - 64 rows");
  const size_t cb_count = (size_t)ks * d;
  for (size_t i = 0; i < cb_count; ++i) REQUIRE(std::isfinite(codebooks_host[i]), "codebooks must be finite");
  REQUIRE(memspace != MI_HOST || wide_codes_below((const uint16_t*)codes, n, row_stride, m, ks), "a code is >= ks");
  HIPC(hipSetDevice(device));
  mi_pqw* h = new mi_pqw();
  h->device = device;
  h->cap = capacity;
  h->row_offset = row_offset;
  h->d = d;
  h->m = m;
  h->ks = ks;
  h->L = d / m;
  h->MH = (m + 1) / 2;
  h->cb_host.assign(codebooks_host, codebooks_host + cb_count);
  const size_t codes_words = (size_t)((capacity + 63) / 64) * h->MH * 64;
  auto cleanup = [&](int code) {
    mi_pqw_destroy(h);
    return code;
  };
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = h->codes.alloc(codes_words);
  if (e == hipSuccess) e = h->cb.alloc(cb_count);
  if (e == hipSuccess) e = h->flag.alloc(64);
  if (e == hipSuccess) e = hipMemsetAsync(h->codes, 0, codes_words * 4, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->flag, 0, 256, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->cb, h->cb_host.data(), cb_count * 4, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return cleanup(fail(e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, std::string("wide PQ index: ") + hipGetErrorString(e)));
  if (n > 0) {
    const int rc = pqw_ingest(h, codes, n, row_stride, memspace);
    if (rc != MI_OK) return cleanup(rc);
    h->n = n;
  }
  *out = h;
  return MI_OK;
}

int mi_pqw_append_codes(mi_pqw* h, const void* codes, int64_t rows, int64_t row_stride, int memspace) {
  REQUIRE(h, "null handle");
  REQUIRE(rows >= 0, "negative number of rows");
  REQUIRE(codes || rows == 0, "null pointer: codes");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  REQUIRE(rows == 0 || row_stride >= h->m, "row_stride below m");
  std::lock_guard<std::mutex> lock(h->mu);
  REQUIRE(h->n + rows <= h->cap, "index capacity exceeded");
  if (rows == 0) return MI_OK;
  REQUIRE(memspace != MI_HOST || wide_codes_below((const uint16_t*)codes, rows, row_stride, h->m, h->ks), "a code is >= ks");
  HIPC(hipSetDevice(h->device));
  const int rc = pqw_ingest(h, codes, rows, row_stride, memspace);
  if (rc != MI_OK) return rc;
  h->n += rows;
  return MI_OK;
}

int mi_pqw_add(mi_pqw* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace) {
  REQUIRE(h, "null handle");
  REQUIRE_ROWS(x, rows, dtype, row_stride, col_stride, memspace);
  std::lock_guard<std::mutex> lock(h->mu);
  REQUIRE(h->n + rows <= h->cap, "index capacity exceeded");
  if (rows == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  const int64_t n0 = h->n;
  // a block's codes land behind the rows that are there; h->n moves only when every block is in
  const int rc = pqw_encode_blocks(h, x, rows, dtype, row_stride, col_stride, memspace, [&](int64_t r, int64_t mm) {
    launch_pqw_ingest(h->cwords, h->m, h->m, n0 + r, mm, h->codes, h->stream);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(h->stream));
    return (int)MI_OK;
  });
  if (rc != MI_OK) return rc;
  h->n = n0 + rows;
  return MI_OK;
}

int mi_pqw_encode(mi_pqw* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace,
                  uint16_t* out_codes_host) {
  REQUIRE(h, "null handle");
  REQUIRE_ROWS(x, rows, dtype, row_stride, col_stride, memspace);
  REQUIRE(out_codes_host || rows == 0, "null pointer: out_codes_host");
  if (rows == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(h->mu);
  HIPC(hipSetDevice(h->device));
  return pqw_encode_blocks(h, x, rows, dtype, row_stride, col_stride, memspace, [&](int64_t r, int64_t mm) {
    HIPC(hipMemcpyAsync(out_codes_host + r * h->m, h->cwords, (size_t)mm * h->m * 2, hipMemcpyDeviceToHost, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    return (int)MI_OK;
  });
}

int mi_pqw_dtable(mi_pqw* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, float* out_table_host) {
  REQUIRE(h, "null handle");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nq == 0 || (q && out_table_host), "null pointer");
  if (nq == 0) return MI_OK;
  int rc;
  if ((rc = check_host_queries(h->d, q, nq, dtype, row_stride, col_stride)) != MI_OK) return rc;
  std::lock_guard<std::mutex> lock(h->mu);
  HIPC(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int64_t per = (int64_t)h->m * h->ks;
  const int64_t step = std::max<int64_t>(1, ((int64_t)64 << 20) / (per * 4));
  if ((rc = h->tab.grow((size_t)(std::min(step, nq) * per))) != MI_OK) return rc;
  std::vector<char> pack;
  for (int64_t q0 = 0; q0 < nq; q0 += step) {
    const int64_t b = std::min(step, nq - q0);
    if ((rc = stage_host_rows(h->xraw, h->d, h->stream, q, q0, b, dtype, row_stride, col_stride, pack)) != MI_OK) return rc;
    launch_pq_table(h->xraw, dtype, h->d, 1, b, h->cb, h->m, h->ks, h->L, h->tab, s);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(out_table_host + q0 * per, h->tab, (size_t)(b * per) * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
  }
  return MI_OK;
}

int mi_pqw_search(mi_pqw* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                  const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_dist, double* out_seconds) {
  REQUIRE(h, "null handle");
  REQUIRE(k >= 1 && k <= 2048, "k must be in [1, 2048]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(!allow_bits || allow_memspace == MI_HOST || allow_memspace == MI_DEVICE, "allow_memspace must be MI_HOST or MI_DEVICE");
  if (out_seconds) *out_seconds = 0.0;
  if (nq == 0) return MI_OK;
  int rc;
  if ((rc = check_host_queries(h->d, q, nq, dtype, row_stride, col_stride)) != MI_OK) return rc;
  std::lock_guard<std::mutex> lock(h->mu);
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t cnt = (size_t)nq * k;
  if ((rc = h->oidx.grow(cnt)) != MI_OK) return rc;
  if (out_dist && (rc = h->odist.grow(cnt)) != MI_OK) return rc;
  const uint64_t* allow_dev;
  if ((rc = allow_on_device(h->bits, allow_bits, allow_memspace, h->n, s, &allow_dev)) != MI_OK) return rc;
  std::vector<char> pack;
  if ((rc = stage_host_rows(h->xraw, h->d, h->stream, q, 0, nq, dtype, row_stride, col_stride, pack)) != MI_OK) return rc;
  if ((rc = pqw_search_core(h, h->xraw, dtype, h->d, 1, nq, k, allow_dev, h->oidx, out_dist ? h->odist.get() : nullptr, s)) != MI_OK) return rc;
  return topk_to_host(out_idx, h->oidx, out_dist, h->odist.get(), cnt, s, t0, out_seconds);
}

int mi_pqw_search_device(mi_pqw* h, const float* q_dev, int64_t nq, int32_t k, const uint64_t* allow_bits_dev, int64_t* out_idx_dev,
                         float* out_dist_dev, void* stream) {
  REQUIRE(h, "null handle");
  REQUIRE(k >= 1 && k <= 2048, "k must be in [1, 2048]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nq == 0 || (q_dev && out_idx_dev), "null pointer");
  if (nq == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  return pqw_search_core(h, q_dev, MI_F32, h->d, 1, nq, k, allow_bits_dev, out_idx_dev, out_dist_dev, (hipStream_t)stream);
}

int mi_pqw_info(const mi_pqw* h, int64_t* n, int32_t* d, int32_t* m, int32_t* ks, int32_t* device, int64_t* row_offset, int64_t* capacity,
                int64_t* hbm_bytes) {
  REQUIRE(h, "null handle");
  if (n) *n = h->n;
  if (d) *d = h->d;
  if (m) *m = h->m;
  if (ks) *ks = h->ks;
  if (device) *device = h->device;
  if (row_offset) *row_offset = h->row_offset;
  if (capacity) *capacity = h->cap;
  if (hbm_bytes) *hbm_bytes = (int64_t)h->bufs.bytes();
  return MI_OK;
}

int mi_pqw_get_codes(mi_pqw* h, int64_t row0, int64_t nrows, uint16_t* out_host) {
  REQUIRE(h, "null handle");
  REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= h->n, "row range outside the index");
  REQUIRE(out_host || nrows == 0, "null pointer: out_host");
  if (nrows == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(h->mu);
  HIPC(hipSetDevice(h->device));
  HIPC(hipStreamSynchronize(h->stream));
  const int64_t blk_words = (int64_t)h->MH * 64;
  const int64_t step = 65536;                      // blocks per copy
  std::vector<uint32_t> buf;
  for (int64_t b0 = row0 / 64; b0 * 64 < row0 + nrows; b0 += step) {
    const int64_t b1 = std::min(b0 + step, (row0 + nrows + 63) / 64);
    buf.resize((size_t)((b1 - b0) * blk_words));
    HIPC(hipMemcpy(buf.data(), h->codes + b0 * blk_words, buf.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t r = std::max(row0, b0 * 64); r < std::min(row0 + nrows, b1 * 64); ++r) {
      const uint32_t* src = buf.data() + ((r >> 6) - b0) * blk_words + (r & 63);
      uint16_t* dst = out_host + (r - row0) * h->m;
      for (int32_t j = 0; j < h->m; ++j) dst[j] = (uint16_t)(src[(int64_t)(j >> 1) * 64] >> (16 * (j & 1)));
    }
  }
  return MI_OK;
}

int mi_pqw_decode(mi_pqw* h, int64_t row0, int64_t nrows, float* out_host) {
  REQUIRE(h, "null handle");
  REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= h->n, "row range outside the index");
  REQUIRE(out_host || nrows == 0, "null pointer: out_host");
  if (nrows == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(h->mu);
  HIPC(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int64_t step = std::max<int64_t>(64, ((int64_t)64 << 20) / ((int64_t)h->d * 4));
  int rc;
  if ((rc = h->xraw.grow((size_t)std::min(step, nrows) * h->d * 4)) != MI_OK) return rc;
  for (int64_t r = 0; r < nrows; r += step) {
    const int64_t mm = std::min(step, nrows - r);
    launch_pqw_decode(h->codes, h->m, h->ks, h->L, h->cb, row0 + r, mm, (float*)h->xraw.get(), s);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(out_host + r * h->d, h->xraw, (size_t)mm * h->d * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));                 // the staging buffer is reused by the next block
  }
  return MI_OK;
}

int mi_pqw_get_codebooks(const mi_pqw* h, float* out_host) {
  REQUIRE(h, "null handle");
  REQUIRE(out_host, "null pointer: out_host");
  std::memcpy(out_host, h->cb_host.data(), h->cb_host.size() * 4);
  return MI_OK;
}

int mi_pqw_destroy(mi_pqw* h) {
  if (!h) return MI_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->bufs.reset();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return MI_OK;
}

}  // extern "C"
