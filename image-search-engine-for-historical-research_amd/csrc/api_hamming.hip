// Binary index of the C ABI: exact Hamming top-K on packed binary codes (mi_hamming; kernels in csrc/hamming.hip).
// The reference's matching_Greedyhash (src/utils/nnsearch.py:1001-1013), faiss IndexBinaryFlat.  A handle of its own: codes in
// transposed 64-row blocks, a uint16 distance matrix of at most "hamming_matrix_bytes" (queries go through it in chunks), grow-only
// staging for queries, bitmap and host results.  Integer and exact: no certificate, no flag, no fallback.
// Radius search and self-join (mi_hamming_range_search*, mi_hamming_self_range; kernels in csrc/hamming_range.hip):
// no matrix, one 64-bit ballot per (block, query) in a workspace of at most "hamming_range_bytes", counted first, filled second.
#include "api_internal.h"

// (struct mi_hamming: api_internal.h -- api_lsh.hip appends to its code storage)

// m host rows of nb bytes at `stride` -> packed device rows, on stream s
static int hm_copy_rows(uint8_t* dst, const uint8_t* src, int64_t stride, int32_t nb, int64_t m, hipStream_t s) {
  if (stride == nb || m == 1) HIPC(hipMemcpyAsync(dst, src, (size_t)m * nb, hipMemcpyHostToDevice, s));
  else HIPC(hipMemcpy2DAsync(dst, (size_t)nb, src, (size_t)stride, (size_t)nb, (size_t)m, hipMemcpyHostToDevice, s));
  return MI_OK;
}

// m packed-or-strided rows of code bytes (host or device) -> rows n .. n + m of the index, synchronous on the handle's stream.
// Host rows pass through a staging buffer of at most 64 MiB at a time.
static int hm_ingest(mi_hamming* h, const void* codes, int64_t m, int64_t stride, int memspace) {
  hipStream_t s = h->stream;
  if (memspace == MI_DEVICE) {
    launch_hamming_ingest((const uint8_t*)codes, stride, h->nbits, h->n, m, h->codes, s);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    return MI_OK;
  }
  const int64_t step = std::max<int64_t>(1, ((int64_t)64 << 20) / h->nb);
  int rc;
  TmpAlloc tmp;
  uint8_t* stage = tmp.get<uint8_t>((size_t)std::min(step, m) * h->nb);
  if (!stage) return fail(MI_ERR_NOMEM, "staging buffer of the code ingest");
  for (int64_t r = 0; r < m; r += step) {
    const int64_t mm = std::min(step, m - r);
    if ((rc = hm_copy_rows(stage, (const uint8_t*)codes + r * stride, stride, h->nb, mm, s)) != MI_OK) return rc;
    launch_hamming_ingest(stage, h->nb, h->nbits, h->n + r, mm, h->codes, s);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));                 // the staging buffer is reused by the next block
  }
  return MI_OK;
}

// the search proper on stream s: queries are words in h->qw, results go to device buffers
static int hm_search_core(mi_hamming* h, int64_t nq, int32_t k, const uint64_t* allow_dev, int64_t* out_idx_dev,
                          int32_t* out_dist_dev, hipStream_t s) {
  const int64_t npad = round_up(h->n, 64);
  const int64_t budget = g_hamming_matrix_bytes.load();
  const int64_t qc = npad == 0 ? nq : std::max<int64_t>(1, std::min<int64_t>(nq, budget / (npad * 2)));
  int rc;
  if ((rc = h->mat.grow((size_t)std::max<int64_t>(qc * npad, 64))) != MI_OK) return rc;
  for (int64_t q0 = 0; q0 < nq; q0 += qc) {
    const int32_t b = (int32_t)std::min<int64_t>(qc, nq - q0);
    launch_hamming_dist(h->codes, h->nbits, h->n, h->qw + q0 * h->wq, b, allow_dev, h->mat, s);
    launch_hamming_select(h->mat, h->n, h->nbits, b, k, h->row_offset, out_idx_dev + q0 * k,
                          out_dist_dev ? out_dist_dev + q0 * k : nullptr, s);
  }
  HIPC(hipGetLastError());
  return MI_OK;
}

// ---- radius search: what one call is about, and how its queries go through the workspace
struct HrCall {
  const uint32_t* qw = nullptr;      // query words [nq][wq] on the device; NULL: the self-join, query i is stored row row0 + i
  int64_t row0 = 0;
  int64_t nq = 0;
  uint32_t radius = 0;
  const uint64_t* allow = nullptr;
};
struct HrPlan {
  int64_t qc = 0;                    // queries per chunk, a multiple of 64: the row length of the workspace
  int64_t nchunks = 0;
};

// the workspace for chunks of a call whose first chunk scans the blocks from b0 on (later chunks of a self-join scan fewer):
// 8 + 2 bytes per (block, query), 4 per (segment of 64 blocks, query), within "hamming_range_bytes", 64 queries at the least
static int hr_prepare(mi_hamming* h, int64_t nq, int64_t b0, HrPlan* p) {
  const int64_t nbl = std::max<int64_t>(1, (h->n + 63) / 64 - b0), nseg = (nbl + 63) / 64;
  int64_t qc = g_hamming_range_bytes.load() / (nbl * 10 + nseg * 4) / 64 * 64;
  qc = std::max<int64_t>(64, std::min<int64_t>({qc, (int64_t)1 << 20, round_up(nq, 64)}));
  p->qc = qc;
  p->nchunks = (nq + qc - 1) / qc;
  int rc;
  if ((rc = h->rmask.grow((size_t)(nbl * qc))) != MI_OK) return rc;
  if ((rc = h->roffs.grow((size_t)(nbl * qc))) != MI_OK) return rc;
  return h->rseg.grow((size_t)(nseg * qc));
}

static HammingRangeArgs hr_args(const mi_hamming* h, const HrCall& c, const HrPlan& p, int64_t q0) {
  HammingRangeArgs a;
  a.codes = h->codes;
  a.nbits = h->nbits;
  a.n = h->n;
  a.self = c.qw == nullptr;
  a.b0 = a.self ? (c.row0 + q0 + 1) >> 6 : 0;      // the block of the first row above the chunk's first query
  a.qsrc = a.self ? h->codes : c.qw + q0 * h->wq;
  a.qrow0 = c.row0 + q0;
  a.nq = (int32_t)std::min<int64_t>(p.qc, c.nq - q0);
  a.allow = c.allow;
  a.radius = c.radius;
  a.early = g_hamming_range_early_exit.load();
  a.masks = h->rmask;
  a.offs = h->roffs;
  a.seg = h->rseg;
  a.qstride = p.qc;
  return a;
}

// pass 1 on stream s: the hit count of every query, then the CSR offsets lims_dev [nq + 1]
static int hr_count(mi_hamming* h, const HrCall& c, const HrPlan& p, int64_t* lims_dev, hipStream_t s) {
  for (int64_t q0 = 0; q0 < c.nq; q0 += p.qc) {
    const HammingRangeArgs a = hr_args(h, c, p, q0);
    if ((h->n + 63) / 64 <= a.b0) {                   // nothing to scan: an empty index, or a self-join chunk at the last rows
      HIPC(hipMemsetAsync(lims_dev + 1 + q0, 0, (size_t)a.nq * 8, s));
      continue;
    }
    launch_hamming_range_scan(a, s);
    launch_hamming_range_offsets(a, lims_dev + 1 + q0, s);
  }
  launch_hamming_range_lims(lims_dev, c.nq, s);
  HIPC(hipGetLastError());
  return MI_OK;
}

// pass 2 on stream s: the hits, ordered, into out_idx_dev / out_dist_dev -- unless lims_dev[nq] > max_results, which the kernels
// see for themselves.  h->rstage holds the hits of any one chunk.  A call of one chunk still has its ballots from pass 1
static int hr_fill(mi_hamming* h, const HrCall& c, const HrPlan& p, const int64_t* lims_dev, int64_t max_results,
                   int64_t* out_idx_dev, int32_t* out_dist_dev, hipStream_t s) {
  for (int64_t q0 = 0; q0 < c.nq; q0 += p.qc) {
    HammingRangeArgs a = hr_args(h, c, p, q0);
    if ((h->n + 63) / 64 <= a.b0) continue;
    if (p.nchunks > 1) {
      launch_hamming_range_scan(a, s);
      launch_hamming_range_offsets(a, nullptr, s);
    }
    a.lims = lims_dev + q0;
    a.total = lims_dev + c.nq;
    a.max_results = max_results;
    a.stage = h->rstage;
    launch_hamming_range_fill(a, s);
    launch_hamming_range_order(a, h->row_offset, out_idx_dev, out_dist_dev, s);
  }
  HIPC(hipGetLastError());
  return MI_OK;
}

// ---- the self-join's ballots without its pairs (api_components.hip): the same plan, the same scan launch, nothing behind it
static HrCall hr_self_call(int64_t row0, int64_t nrows, int32_t radius) {
  HrCall c;
  c.row0 = row0;
  c.nq = nrows;
  c.radius = (uint32_t)radius;
  return c;
}

int hamming_self_check(const mi_hamming* h, int64_t row0, int64_t nrows, int32_t radius) {
  REQUIRE(radius >= 0, "radius must be >= 0");
  REQUIRE(row0 >= 0 && nrows >= 0, "row range outside the index");
  REQUIRE(row0 <= h->n && nrows <= h->n - row0, "row range outside the index");
  return MI_OK;
}

int hamming_self_plan(mi_hamming* h, int64_t row0, int64_t nrows, int64_t* qc) {
  HrPlan p;
  const int rc = hr_prepare(h, nrows, (row0 + 1) >> 6, &p);
  *qc = p.qc;
  return rc;
}

int hamming_self_scan(mi_hamming* h, int64_t row0, int64_t nrows, int32_t radius, int64_t qc, int64_t q0, HammingBallots* out,
                      hipStream_t s) {
  HrPlan p;
  p.qc = qc;
  p.nchunks = (nrows + qc - 1) / qc;
  const HammingRangeArgs a = hr_args(h, hr_self_call(row0, nrows, radius), p, q0);
  out->masks = a.masks;
  out->b0 = a.b0;
  out->nbl = std::max<int64_t>(0, (h->n + 63) / 64 - a.b0);     // 0: a chunk at the last rows, nothing above it to scan
  out->qstride = a.qstride;
  out->qrow0 = a.qrow0;
  out->nq = a.nq;
  if (out->nbl == 0) return MI_OK;
  launch_hamming_range_scan(a, s);
  HIPC(hipGetLastError());
  return MI_OK;
}

// host output of a radius search or a self-join whose queries (and bitmap) are on the device already
static int hr_host(mi_hamming* h, const HrCall& c, int64_t max_results, int64_t* out_lims, int64_t* out_idx, int32_t* out_dist) {
  hipStream_t s = h->stream;
  HrPlan p;
  int rc;
  if ((rc = hr_prepare(h, c.nq, c.qw ? 0 : (c.row0 + 1) >> 6, &p)) != MI_OK) return rc;
  if ((rc = h->rlims.grow((size_t)c.nq + 1)) != MI_OK) return rc;
  if ((rc = hr_count(h, c, p, h->rlims, s)) != MI_OK) return rc;
  HIPC(hipMemcpyAsync(out_lims, h->rlims, ((size_t)c.nq + 1) * 8, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  const int64_t total = out_lims[c.nq];
  if (total > max_results)
    return fail(MI_ERR_CAPACITY, "radius search: " + std::to_string(total) + " results > max_results " +
                                     std::to_string(max_results) + "; call again with max_results >= out_lims[nq]");
  if (total == 0) return MI_OK;
  int64_t most = 0;                                   // hits of the fullest chunk
  for (int64_t q0 = 0; q0 < c.nq; q0 += p.qc) most = std::max(most, out_lims[std::min(q0 + p.qc, c.nq)] - out_lims[q0]);
  if ((rc = h->rstage.grow((size_t)most)) != MI_OK) return rc;
  if ((rc = h->oidx.grow((size_t)total)) != MI_OK) return rc;
  if (out_dist && (rc = h->odist.grow((size_t)total)) != MI_OK) return rc;
  if ((rc = hr_fill(h, c, p, h->rlims, total, h->oidx, out_dist ? h->odist.get() : nullptr, s)) != MI_OK) return rc;
  HIPC(hipMemcpyAsync(out_idx, h->oidx, (size_t)total * 8, hipMemcpyDeviceToHost, s));
  if (out_dist) HIPC(hipMemcpyAsync(out_dist, h->odist, (size_t)total * 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  return MI_OK;
}

extern "C" {

int mi_hamming_create(const void* codes, int64_t n, int32_t nbits, int64_t row_stride_bytes, int memspace, int device,
                      int64_t row_offset, int64_t capacity, mi_hamming** out) {
  REQUIRE(out, "null pointer: out");
  REQUIRE(n >= 0, "negative number of rows");
  REQUIRE(nbits >= 8 && nbits <= 4096 && nbits % 8 == 0, "nbits must be a multiple of 8 in [8, 4096]");
  REQUIRE(capacity >= 0, "negative capacity");
  REQUIRE(capacity == 0 || capacity >= n, "capacity below the number of rows");
  REQUIRE(codes || n == 0, "null pointer: codes");
  REQUIRE(n >= 1 || capacity >= 1, "an empty index needs a capacity");
  REQUIRE(n == 0 || row_stride_bytes >= nbits / 8, "row_stride_bytes below nbits / 8");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  if (capacity == 0) capacity = n;
  REQUIRE(capacity < (int64_t)1 << 32, "an index holds at most 2^32-1 rows");
  HIPC(hipSetDevice(device));
  mi_hamming* h = new mi_hamming();
  h->device = device;
  h->cap = capacity;
  h->row_offset = row_offset;
  h->nbits = nbits;
  h->nb = nbits / 8;
  h->W32 = (nbits + 31) / 32;
  h->wq = hamming_query_words(h->W32);
  const size_t codes_words = (size_t)((capacity + 63) / 64) * h->W32 * 64;
  auto cleanup = [&](int code) {
    mi_hamming_destroy(h);
    return code;
  };
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = h->codes.alloc(codes_words);
  if (e == hipSuccess) e = hipMemsetAsync(h->codes, 0, codes_words * 4, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return cleanup(fail(e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, std::string("binary index: ") + hipGetErrorString(e)));
  if (n > 0) {
    const int rc = hm_ingest(h, codes, n, row_stride_bytes, memspace);
    if (rc != MI_OK) return cleanup(rc);
    h->n = n;
  }
  *out = h;
  return MI_OK;
}

int mi_hamming_append(mi_hamming* h, const void* codes, int64_t m, int64_t row_stride_bytes, int memspace) {
  REQUIRE(h, "null handle");
  REQUIRE(m >= 0, "negative number of rows");
  REQUIRE(codes || m == 0, "null pointer: codes");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  REQUIRE(m == 0 || row_stride_bytes >= h->nb, "row_stride_bytes below nbits / 8");
  std::lock_guard<std::mutex> lock(h->mu);
  REQUIRE(h->n + m <= h->cap, "index capacity exceeded");
  if (m == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  const int rc = hm_ingest(h, codes, m, row_stride_bytes, memspace);
  if (rc != MI_OK) return rc;
  h->n += m;
  return MI_OK;
}

int mi_hamming_append_sign_device(mi_hamming* h, const float* x_dev, int64_t m, int32_t d, int64_t row_stride, void* stream) {
  REQUIRE(h, "null handle");
  REQUIRE(m >= 0, "negative number of rows");
  REQUIRE(x_dev || m == 0, "null pointer: x_dev");
  REQUIRE(d == h->nbits, "d must equal the index's nbits");
  REQUIRE(m == 0 || row_stride >= d, "row_stride below d");
  REQUIRE(h->n + m <= h->cap, "index capacity exceeded");
  if (m == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  launch_hamming_sign(x_dev, m, d, row_stride, nullptr, 0, h->codes, h->n, (hipStream_t)stream);
  HIPC(hipGetLastError());
  h->n += m;
  return MI_OK;
}

int mi_pack_sign_bits_device(const float* x_dev, int64_t n, int32_t d, int64_t row_stride, uint8_t* out_dev,
                             int64_t out_row_stride_bytes, void* stream) {
  REQUIRE(n >= 0, "negative number of rows");
  REQUIRE(d >= 8 && d % 8 == 0, "d must be a positive multiple of 8");
  REQUIRE(n == 0 || (x_dev && out_dev), "null pointer");
  REQUIRE(n == 0 || (row_stride >= d && out_row_stride_bytes >= d / 8), "row stride below the row length");
  if (n == 0) return MI_OK;
  launch_hamming_sign(x_dev, n, d, row_stride, out_dev, out_row_stride_bytes, nullptr, 0, (hipStream_t)stream);
  HIPC(hipGetLastError());
  return MI_OK;
}

int mi_hamming_info(const mi_hamming* h, int64_t* n, int32_t* nbits, int32_t* device, int64_t* row_offset, int64_t* capacity,
                    int64_t* hbm_bytes) {
  REQUIRE(h, "null handle");
  if (n) *n = h->n;
  if (nbits) *nbits = h->nbits;
  if (device) *device = h->device;
  if (row_offset) *row_offset = h->row_offset;
  if (capacity) *capacity = h->cap;
  if (hbm_bytes) *hbm_bytes = (int64_t)h->bufs.bytes();
  return MI_OK;
}

int mi_hamming_get_codes(mi_hamming* h, int64_t row0, int64_t nrows, uint8_t* out_host) {
  REQUIRE(h, "null handle");
  REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= h->n, "row range outside the index");
  REQUIRE(out_host || nrows == 0, "null pointer: out_host");
  if (nrows == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(h->mu);
  HIPC(hipSetDevice(h->device));
  HIPC(hipStreamSynchronize(h->stream));
  const int64_t blk_words = (int64_t)h->W32 * 64;
  const int64_t step = 4096;                       // blocks per copy
  std::vector<uint32_t> buf;
  for (int64_t b0 = row0 / 64; b0 * 64 < row0 + nrows; b0 += step) {
    const int64_t b1 = std::min(b0 + step, (row0 + nrows + 63) / 64);
    buf.resize((size_t)((b1 - b0) * blk_words));
    HIPC(hipMemcpy(buf.data(), h->codes + b0 * blk_words, buf.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t r = std::max(row0, b0 * 64); r < std::min(row0 + nrows, b1 * 64); ++r) {
      const uint32_t* src = buf.data() + ((r >> 6) - b0) * blk_words + (r & 63);
      uint8_t* dst = out_host + (r - row0) * h->nb;
      for (int32_t j = 0; j < h->nb; ++j) dst[j] = (uint8_t)(src[(int64_t)(j >> 2) * 64] >> (8 * (j & 3)));
    }
  }
  return MI_OK;
}

int mi_hamming_search(mi_hamming* h, const void* q_codes, int64_t nq, int64_t q_row_stride_bytes, int32_t k,
                      const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, int32_t* out_dist, double* out_seconds) {
  REQUIRE(h, "null handle");
  REQUIRE(k >= 1 && k <= 2048, "k must be in [1, 2048]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nq == 0 || q_codes, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(!allow_bits || allow_memspace == MI_HOST || allow_memspace == MI_DEVICE, "allow_memspace must be MI_HOST or MI_DEVICE");
  if (out_seconds) *out_seconds = 0.0;
  if (nq == 0) return MI_OK;
  REQUIRE(q_row_stride_bytes >= h->nb, "q_row_stride_bytes below nbits / 8");
  std::lock_guard<std::mutex> lock(h->mu);
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  int rc;
  const size_t cnt = (size_t)nq * k;
  if ((rc = h->qraw.grow((size_t)nq * h->nb)) != MI_OK) return rc;
  if ((rc = h->qw.grow((size_t)nq * h->wq)) != MI_OK) return rc;
  if ((rc = h->oidx.grow(cnt)) != MI_OK) return rc;
  if (out_dist && (rc = h->odist.grow(cnt)) != MI_OK) return rc;
  const uint64_t* allow_dev;
  if ((rc = allow_on_device(h->bits, allow_bits, allow_memspace, h->n, s, &allow_dev)) != MI_OK) return rc;
  if ((rc = hm_copy_rows(h->qraw, (const uint8_t*)q_codes, q_row_stride_bytes, h->nb, nq, s)) != MI_OK) return rc;
  launch_hamming_query_words(h->qraw, h->nb, h->nbits, nq, h->qw, s);
  if ((rc = hm_search_core(h, nq, k, allow_dev, h->oidx, out_dist ? h->odist.get() : nullptr, s)) != MI_OK) return rc;
  return topk_to_host(out_idx, h->oidx, out_dist, h->odist.get(), cnt, s, t0, out_seconds);
}

int mi_hamming_search_device(mi_hamming* h, const uint8_t* q_dev, int64_t nq, int32_t k, const uint64_t* allow_bits_dev,
                             int64_t* out_idx_dev, int32_t* out_dist_dev, void* stream) {
  REQUIRE(h, "null handle");
  REQUIRE(k >= 1 && k <= 2048, "k must be in [1, 2048]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nq == 0 || (q_dev && out_idx_dev), "null pointer");
  if (nq == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = h->qw.grow((size_t)nq * h->wq)) != MI_OK) return rc;
  launch_hamming_query_words(q_dev, h->nb, h->nbits, nq, h->qw, s);
  return hm_search_core(h, nq, k, allow_bits_dev, out_idx_dev, out_dist_dev, s);
}

int mi_hamming_range_search(mi_hamming* h, const void* q_codes, int64_t nq, int64_t q_row_stride_bytes, int32_t radius,
                            const uint64_t* allow_bits, int allow_memspace, int64_t max_results, int64_t* out_lims,
                            int64_t* out_idx, int32_t* out_dist, double* out_seconds) {
  REQUIRE(h, "null handle");
  REQUIRE(radius >= 0, "radius must be >= 0");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(out_lims, "null pointer: out_lims");
  REQUIRE(nq == 0 || q_codes, "null pointer: queries");
  REQUIRE(max_results >= 0, "max_results must be >= 0");
  REQUIRE(max_results == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(!allow_bits || allow_memspace == MI_HOST || allow_memspace == MI_DEVICE, "allow_memspace must be MI_HOST or MI_DEVICE");
  if (out_seconds) *out_seconds = 0.0;
  out_lims[0] = 0;
  if (nq == 0) return MI_OK;
  REQUIRE(q_row_stride_bytes >= h->nb, "q_row_stride_bytes below nbits / 8");
  std::lock_guard<std::mutex> lock(h->mu);
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  int rc;
  if ((rc = h->qraw.grow((size_t)nq * h->nb)) != MI_OK) return rc;
  if ((rc = h->qw.grow((size_t)nq * h->wq)) != MI_OK) return rc;
  HrCall c;
  if ((rc = allow_on_device(h->bits, allow_bits, allow_memspace, h->n, s, &c.allow)) != MI_OK) return rc;
  if ((rc = hm_copy_rows(h->qraw, (const uint8_t*)q_codes, q_row_stride_bytes, h->nb, nq, s)) != MI_OK) return rc;
  launch_hamming_query_words(h->qraw, h->nb, h->nbits, nq, h->qw, s);
  c.qw = h->qw;
  c.nq = nq;
  c.radius = (uint32_t)radius;
  rc = hr_host(h, c, max_results, out_lims, out_idx, out_dist);
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int mi_hamming_range_search_device(mi_hamming* h, const uint8_t* q_dev, int64_t nq, int32_t radius, const uint64_t* allow_bits_dev,
                                   int64_t max_results, int64_t* out_lims_dev, int64_t* out_idx_dev, int32_t* out_dist_dev,
                                   void* stream) {
  REQUIRE(h, "null handle");
  REQUIRE(radius >= 0, "radius must be >= 0");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(out_lims_dev, "null pointer: out_lims_dev");
  REQUIRE(nq == 0 || q_dev, "null pointer: queries");
  REQUIRE(max_results >= 0, "max_results must be >= 0");
  REQUIRE(max_results == 0 || out_idx_dev, "null pointer: out_idx_dev");
  HIPC(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) {
    HIPC(hipMemsetAsync(out_lims_dev, 0, 8, s));
    return MI_OK;
  }
  int rc;
  HrPlan p;
  if ((rc = h->qw.grow((size_t)nq * h->wq)) != MI_OK) return rc;
  if ((rc = hr_prepare(h, nq, 0, &p)) != MI_OK) return rc;
  // the hits of one chunk: at most the caller's capacity (beyond it nothing is written), at most every row for every query
  const int64_t stage = std::min<int64_t>(max_results, std::min(p.qc, nq) * h->n);
  if (stage > 0 && (rc = h->rstage.grow((size_t)stage)) != MI_OK) return rc;
  launch_hamming_query_words(q_dev, h->nb, h->nbits, nq, h->qw, s);
  HrCall c;
  c.qw = h->qw;
  c.nq = nq;
  c.radius = (uint32_t)radius;
  c.allow = allow_bits_dev;
  if ((rc = hr_count(h, c, p, out_lims_dev, s)) != MI_OK) return rc;
  if (stage == 0) return MI_OK;
  return hr_fill(h, c, p, out_lims_dev, max_results, out_idx_dev, out_dist_dev, s);
}

int mi_hamming_self_range(mi_hamming* h, int64_t row0, int64_t nrows, int32_t radius, int64_t max_results, int64_t* out_lims,
                          int64_t* out_idx, int32_t* out_dist, double* out_seconds) {
  REQUIRE(h, "null handle");
  REQUIRE(radius >= 0, "radius must be >= 0");
  REQUIRE(out_lims, "null pointer: out_lims");
  REQUIRE(max_results >= 0, "max_results must be >= 0");
  REQUIRE(max_results == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(row0 >= 0 && nrows >= 0, "row range outside the index");
  std::lock_guard<std::mutex> lock(h->mu);
  REQUIRE(row0 <= h->n && nrows <= h->n - row0, "row range outside the index");
  if (out_seconds) *out_seconds = 0.0;
  out_lims[0] = 0;
  if (nrows == 0) return MI_OK;
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(h->device));
  const int rc = hr_host(h, hr_self_call(row0, nrows, radius), max_results, out_lims, out_idx, out_dist);
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int mi_hamming_destroy(mi_hamming* h) {
  if (!h) return MI_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->bufs.reset();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return MI_OK;
}

}  // extern "C"
