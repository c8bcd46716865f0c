// The host functions of both flat PQ indexes (mi_pq in api_pq.hip, mi_pqw in api_pq_wide.hip): one
// implementation over the handle type H, a PqFlat<CodeT> (api_internal.h).  The extern "C" entry points of the two files forward
// here.  What follows from the code width is written once in terms of H::Code -- books to a dword, the 64 MiB host staging step, the
// widths of the strided copy, the stride in code elements, the device check that is skipped when no code of that width can reach
// ks -- and what really differs between the two indexes is PqTraits<H>, below.
#pragma once
#include "api_internal.h"

template <typename H> struct PqTraits;
template <> struct PqTraits<mi_pq> {
  static constexpr int32_t MAX_KS = 256;
  static constexpr const char* KS_MSG = "ks (codewords per book) must be in [2, 256]";
  static constexpr const char* CODE_MSG = "a code byte is >= ks";
  static constexpr const char* STRIDE_MSG = "row_stride_bytes below m";
  static constexpr const char* NAME = "PQ index: ";
  static constexpr int64_t TABLE_BYTES = 0;                    // the tables of a pass are not bounded (a known asymmetry)
  static void scan(mi_pq* h, int32_t b, const uint64_t* allow_dev, hipStream_t s) {
    launch_pq_scan(h->codes, h->m, h->ks, h->n, h->tab, b, pq_query_tile(h->m, h->ks, b), allow_dev, h->mat, s);
  }
  static void rows_changed(mi_pq* h) { ++h->mod; }
};
template <> struct PqTraits<mi_pqw> {
  static constexpr int32_t MAX_KS = PQW_MAX_KS;
  static constexpr const char* KS_MSG = "ks (codewords per book) must be in [2, 8192]";
  static constexpr const char* CODE_MSG = "a code is >= ks";
  static constexpr const char* STRIDE_MSG = "row_stride below m";
  static constexpr const char* NAME = "wide PQ index: ";
  static constexpr int64_t TABLE_BYTES = (int64_t)1 << 30;     // the tables of a pass (512 KiB a query at 16 x 8192) stay within 1 GiB
  static void scan(mi_pqw* h, int32_t b, const uint64_t* allow_dev, hipStream_t s) {
    launch_pqw_scan(h->codes, h->m, h->ks, h->n, h->tab, b, pqw_query_tile(h->ks, b), allow_dev, h->mat, s);
  }
  static void rows_changed(mi_pqw*) {}
};

// rows of codes, `stride` codes apart (host: checked by the caller; device: checked here) -> rows n .. n + rows of the index,
// synchronous on the handle's stream.  A device code >= ks: MI_ERR_INVALID, nothing written.
template <typename H>
static int pq_flat_ingest(H* h, const void* codes, int64_t rows, int64_t stride, int memspace) {
  using CodeT = typename H::Code;
  hipStream_t s = h->stream;
  int rc;
  if (memspace == MI_DEVICE) {
    if (h->ks < H::CODE_VALUES) {                  // else no code of this width reaches ks
      bool raised;
      launch_pq_check((const CodeT*)codes, stride, h->m, h->ks, rows, h->flag, s);
      if ((rc = check_flag(h->flag, s, &raised)) != MI_OK) return rc;
      if (raised) return fail(MI_ERR_INVALID, PqTraits<H>::CODE_MSG);
    }
    launch_pq_ingest((const CodeT*)codes, stride, h->m, h->n, rows, h->codes, s);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    return MI_OK;
  }
  const size_t row_bytes = (size_t)h->m * sizeof(CodeT);
  const int64_t step = std::max<int64_t>(1, ((int64_t)64 << 20) / (int64_t)row_bytes);
  if ((rc = h->cstage.grow((size_t)std::min(step, rows) * h->m)) != MI_OK) return rc;
  for (int64_t r = 0; r < rows; r += step) {
    const int64_t mm = std::min(step, rows - r);
    const CodeT* src = (const CodeT*)codes + r * stride;
    if (stride == h->m || mm == 1) HIPC(hipMemcpyAsync(h->cstage, src, (size_t)mm * row_bytes, hipMemcpyHostToDevice, s));
    else HIPC(hipMemcpy2DAsync(h->cstage, row_bytes, src, (size_t)stride * sizeof(CodeT), row_bytes, (size_t)mm, hipMemcpyHostToDevice, s));
    launch_pq_ingest(h->cstage.get(), h->m, h->m, h->n + r, mm, h->codes, s);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));                 // the staging buffer is reused by the next block
  }
  return MI_OK;
}

// encodes `rows` rows (host or device) in blocks; after each block `sink(r, mm)` consumes the packed codes of rows r .. r + mm in
// h->cstage.  Synchronous on the handle's stream.
template <typename H, typename Sink>
static int pq_flat_encode_blocks(H* h, const void* x, int64_t rows, int dtype, int64_t rs, int64_t cs, int memspace, Sink sink) {
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  const int64_t step = std::max<int64_t>(64, ((int64_t)64 << 20) / ((int64_t)h->d * (int64_t)esz));
  hipStream_t s = h->stream;
  int rc;
  if ((rc = h->cstage.grow((size_t)std::min(step, rows) * h->m)) != MI_OK) return rc;
  std::vector<char> pack;
  for (int64_t r = 0; r < rows; r += step) {
    const int64_t mm = std::min(step, rows - r);
    if (memspace == MI_HOST) {
      if ((rc = stage_host_rows(h->xraw, h->d, h->stream, x, r, mm, dtype, rs, cs, pack)) != MI_OK) return rc;
      launch_pq_encode(h->xraw, dtype, h->d, 1, mm, h->cb, h->m, h->ks, h->L, h->cstage.get(), s);
    } else {
      launch_pq_encode((const char*)x + (size_t)r * rs * esz, dtype, rs, cs, mm, h->cb, h->m, h->ks, h->L, h->cstage.get(), s);
    }
    HIPC(hipGetLastError());
    if ((rc = sink(r, mm)) != MI_OK) return rc;
  }
  return MI_OK;
}

// the search proper on stream s: queries on the device (any strides), results go to device buffers
template <typename H>
static int pq_flat_search_core(H* h, const void* q_dev, int dtype, int64_t rs, int64_t cs, int64_t nq, int32_t k, const uint64_t* allow_dev,
                               int64_t* out_idx_dev, float* out_dist_dev, hipStream_t s) {
  const int64_t npad = round_up(h->n, 64);
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  if (npad == 0) {
    launch_pq_emit(nullptr, nullptr, nq, 0, k, h->row_offset, out_idx_dev, out_dist_dev, s);
    HIPC(hipGetLastError());
    return MI_OK;
  }
  // queries per pass: the matrix within "pq_matrix_bytes" (and, wide index, the tables within TABLE_BYTES), whole tiles of 4, one
  // tile at the least
  const int64_t per = (int64_t)h->m * h->ks;
  const int64_t budget = g_pq_matrix_bytes.load();
  int64_t qc = std::min<int64_t>({nq, budget / (npad * 4), (int64_t)1 << 20});
  if (PqTraits<H>::TABLE_BYTES) qc = std::min(qc, PqTraits<H>::TABLE_BYTES / (per * 4));
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
    PqTraits<H>::scan(h, b, allow_dev, s);
    launch_dense_topk(h->mat, npad, npad, b, ke, 0, h->tidx, h->tneg, s);
    launch_pq_emit(h->tidx, h->tneg, b, ke, k, h->row_offset, out_idx_dev + q0 * k, out_dist_dev ? out_dist_dev + q0 * k : nullptr, s);
  }
  HIPC(hipGetLastError());
  return MI_OK;
}

template <typename H>
static int pq_flat_destroy(H* h) {
  if (!h) return MI_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->bufs.reset();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return MI_OK;
}

template <typename H>
static int pq_flat_create(const float* codebooks_host, int32_t d, int32_t m, int32_t ks, const void* codes, int64_t n, int64_t row_stride,
                          int memspace, int device, int64_t row_offset, int64_t capacity, H** out) {
  using CodeT = typename H::Code;
  using T = PqTraits<H>;
  REQUIRE(out, "null pointer: out");
  REQUIRE(codebooks_host, "null pointer: codebooks_host");
  REQUIRE(m >= 1 && m <= 64, "m (books) must be in [1, 64]");
  REQUIRE(ks >= 2 && ks <= T::MAX_KS, T::KS_MSG);
  REQUIRE(d >= 1 && d <= 4096, "d must be in [1, 4096]");
  REQUIRE(d % m == 0, "d must be a multiple of m");
  REQUIRE(n >= 0, "negative number of rows");
  REQUIRE(capacity >= 0, "negative capacity");
  REQUIRE(capacity == 0 || capacity >= n, "capacity below the number of rows");
  REQUIRE(codes || n == 0, "null pointer: codes");
  REQUIRE(n >= 1 || capacity >= 1, "an empty index needs a capacity");
  REQUIRE(n == 0 || row_stride >= m, T::STRIDE_MSG);
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  if (capacity == 0) capacity = n;
  REQUIRE(capacity < ((int64_t)1 << 32) - 64, "an index holds fewer than 2^32 - 64 rows");
  const size_t cb_count = (size_t)ks * d;
  for (size_t i = 0; i < cb_count; ++i) REQUIRE(std::isfinite(codebooks_host[i]), "codebooks must be finite");
  REQUIRE(memspace != MI_HOST || codes_below((const CodeT*)codes, n, row_stride, m, ks), T::CODE_MSG);
  HIPC(hipSetDevice(device));
  H* h = new H();
  h->device = device;
  h->cap = capacity;
  h->row_offset = row_offset;
  h->d = d;
  h->m = m;
  h->ks = ks;
  h->L = d / m;
  h->MW = pq_code_dwords<CodeT>(m);
  h->cb_host.assign(codebooks_host, codebooks_host + cb_count);
  const size_t codes_words = (size_t)((capacity + 63) / 64) * h->MW * 64;
  auto cleanup = [&](int code) {
    pq_flat_destroy(h);
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
    return cleanup(fail(e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, std::string(T::NAME) + hipGetErrorString(e)));
  if (n > 0) {
    const int rc = pq_flat_ingest(h, codes, n, row_stride, memspace);
    if (rc != MI_OK) return cleanup(rc);
    h->n = n;
  }
  *out = h;
  return MI_OK;
}

template <typename H>
static int pq_flat_append_codes(H* h, const void* codes, int64_t rows, int64_t row_stride, int memspace) {
  using CodeT = typename H::Code;
  REQUIRE(h, "null handle");
  REQUIRE(rows >= 0, "negative number of rows");
  REQUIRE(codes || rows == 0, "null pointer: codes");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  REQUIRE(rows == 0 || row_stride >= h->m, PqTraits<H>::STRIDE_MSG);
  std::lock_guard<std::mutex> lock(h->mu);
  REQUIRE(h->n + rows <= h->cap, "index capacity exceeded");
  if (rows == 0) return MI_OK;
  REQUIRE(memspace != MI_HOST || codes_below((const CodeT*)codes, rows, row_stride, h->m, h->ks), PqTraits<H>::CODE_MSG);
  HIPC(hipSetDevice(h->device));
  const int rc = pq_flat_ingest(h, codes, rows, row_stride, memspace);
  if (rc != MI_OK) return rc;
  h->n += rows;
  PqTraits<H>::rows_changed(h);
  return MI_OK;
}

template <typename H>
static int pq_flat_add(H* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace) {
  REQUIRE(h, "null handle");
  REQUIRE_ROWS(x, rows, dtype, row_stride, col_stride, memspace);
  std::lock_guard<std::mutex> lock(h->mu);
  REQUIRE(h->n + rows <= h->cap, "index capacity exceeded");
  if (rows == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  const int64_t n0 = h->n;
  // a block's codes land behind the rows that are there; h->n moves only when every block is in
  const int rc = pq_flat_encode_blocks(h, x, rows, dtype, row_stride, col_stride, memspace, [&](int64_t r, int64_t mm) {
    launch_pq_ingest(h->cstage.get(), h->m, h->m, n0 + r, mm, h->codes, h->stream);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(h->stream));
    return (int)MI_OK;
  });
  if (rc != MI_OK) return rc;
  h->n = n0 + rows;
  PqTraits<H>::rows_changed(h);
  return MI_OK;
}

template <typename H>
static int pq_flat_encode(H* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace,
                          typename H::Code* out_codes_host) {
  REQUIRE(h, "null handle");
  REQUIRE_ROWS(x, rows, dtype, row_stride, col_stride, memspace);
  REQUIRE(out_codes_host || rows == 0, "null pointer: out_codes_host");
  if (rows == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(h->mu);
  HIPC(hipSetDevice(h->device));
  return pq_flat_encode_blocks(h, x, rows, dtype, row_stride, col_stride, memspace, [&](int64_t r, int64_t mm) {
    HIPC(hipMemcpyAsync(out_codes_host + r * h->m, h->cstage, (size_t)mm * h->m * sizeof(typename H::Code), hipMemcpyDeviceToHost, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    return (int)MI_OK;
  });
}

template <typename H>
static int pq_flat_dtable(H* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, float* out_table_host) {
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

template <typename H>
static int pq_flat_search(H* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
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
  if ((rc = pq_flat_search_core(h, h->xraw, dtype, h->d, 1, nq, k, allow_dev, h->oidx, out_dist ? h->odist.get() : nullptr, s)) != MI_OK) return rc;
  return topk_to_host(out_idx, h->oidx, out_dist, h->odist.get(), cnt, s, t0, out_seconds);
}

template <typename H>
static int pq_flat_search_device(H* h, const float* q_dev, int64_t nq, int32_t k, const uint64_t* allow_bits_dev, int64_t* out_idx_dev,
                                 float* out_dist_dev, void* stream) {
  REQUIRE(h, "null handle");
  REQUIRE(k >= 1 && k <= 2048, "k must be in [1, 2048]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nq == 0 || (q_dev && out_idx_dev), "null pointer");
  if (nq == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  return pq_flat_search_core(h, q_dev, MI_F32, h->d, 1, nq, k, allow_bits_dev, out_idx_dev, out_dist_dev, (hipStream_t)stream);
}

template <typename H>
static int pq_flat_info(const H* h, int64_t* n, int32_t* d, int32_t* m, int32_t* ks, int32_t* device, int64_t* row_offset, int64_t* capacity,
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

template <typename H>
static int pq_flat_get_codes(H* h, int64_t row0, int64_t nrows, typename H::Code* out_host) {
  REQUIRE(h, "null handle");
  REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= h->n, "row range outside the index");
  REQUIRE(out_host || nrows == 0, "null pointer: out_host");
  if (nrows == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(h->mu);
  HIPC(hipSetDevice(h->device));
  HIPC(hipStreamSynchronize(h->stream));
  const int64_t blk_words = (int64_t)h->MW * 64;
  const int64_t step = 65536;                      // blocks per copy
  std::vector<uint32_t> buf;
  for (int64_t b0 = row0 / 64; b0 * 64 < row0 + nrows; b0 += step) {
    const int64_t b1 = std::min(b0 + step, (row0 + nrows + 63) / 64);
    buf.resize((size_t)((b1 - b0) * blk_words));
    HIPC(hipMemcpy(buf.data(), h->codes + b0 * blk_words, buf.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t r = std::max(row0, b0 * 64); r < std::min(row0 + nrows, b1 * 64); ++r)
      unpack_code_row(buf.data(), r - b0 * 64, h->MW, h->m, out_host + (r - row0) * h->m);
  }
  return MI_OK;
}

template <typename H>
static int pq_flat_decode(H* h, int64_t row0, int64_t nrows, float* out_host) {
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
    launch_pq_decode(h->codes, sizeof(typename H::Code), h->m, h->ks, h->L, h->cb, row0 + r, mm, (float*)h->xraw.get(), s);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(out_host + r * h->d, h->xraw, (size_t)mm * h->d * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));                 // the staging buffer is reused by the next block
  }
  return MI_OK;
}

template <typename H>
static int pq_flat_get_codebooks(const H* h, float* out_host) {
  REQUIRE(h, "null handle");
  REQUIRE(out_host, "null pointer: out_host");
  std::memcpy(out_host, h->cb_host.data(), h->cb_host.size() * 4);
  return MI_OK;
}
