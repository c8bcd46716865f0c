// LSH codes of the C ABI (kernel in csrc/lsh.hip): the first half of faiss IndexLSH (src/utils/nnsearch.py:734-745),
// float descriptors -> packed sign codes of their projections, as a stand-alone encoder (device, host) and as an append into a
// binary index (mi_hamming), whose search is the second half.  No handle of its own: R and the thresholds are the caller's.
#include "api_internal.h"

// what every entry point checks about the operands, before any device is touched
static int lsh_check(int64_t n, int32_t d, int dtype, int64_t rs, int64_t cs, const void* R, int32_t nbits, const char* rows_name) {
  if (n < 0) return fail(MI_ERR_INVALID, std::string("negative number of rows: ") + rows_name);
  REQUIRE(nbits >= 8 && nbits <= 4096 && nbits % 8 == 0, "nbits must be a multiple of 8 in [8, 4096]");
  REQUIRE(d >= 1 && d <= 4096, "d must be in [1, 4096]");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  REQUIRE(rs >= 0 && cs >= 0, "negative strides are not supported: row_stride, col_stride");
  REQUIRE(R, "null pointer: R");
  return MI_OK;
}

extern "C" {

int mi_lsh_encode_device(const void* X_dev, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride,
                         const double* R_dev, const double* thr_dev, int32_t nbits, uint8_t* out_dev, int64_t out_row_stride_bytes,
                         void* stream) {
  const int rc = lsh_check(n, d, dtype, row_stride, col_stride, R_dev, nbits, "n");
  if (rc != MI_OK) return rc;
  REQUIRE(out_row_stride_bytes >= nbits / 8, "out_row_stride_bytes below nbits / 8");
  if (n == 0) return MI_OK;
  REQUIRE(X_dev, "null pointer: X_dev");
  REQUIRE(out_dev, "null pointer: out_dev");
  launch_lsh_encode(X_dev, dtype, n, d, row_stride, col_stride, R_dev, thr_dev, nbits, out_dev, out_row_stride_bytes, nullptr, 0,
                    (hipStream_t)stream);
  HIPC(hipGetLastError());
  return MI_OK;
}

int mi_lsh_encode(const void* X, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride, const double* R,
                  const double* thr, int32_t nbits, int device, uint8_t* out) {
  int rc = lsh_check(n, d, dtype, row_stride, col_stride, R, nbits, "n");
  if (rc != MI_OK) return rc;
  if (n == 0) return MI_OK;
  REQUIRE(X, "null pointer: X");
  REQUIRE(out, "null pointer: out");
  HIPC(hipSetDevice(device));
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  const int32_t nb = nbits / 8;
  // rows pass through the device in blocks of at most 64 MiB of descriptors (a multiple of the kernel's 128-row tile, though no
  // bit depends on where a block ends: a row's sum is its own)
  const int64_t step = std::max<int64_t>(128, ((int64_t)64 << 20) / ((int64_t)d * (int64_t)esz) / 128 * 128);
  const int64_t blk = std::min(step, n);
  TmpAlloc tmp;
  char* xd = tmp.get<char>((size_t)blk * d * esz);
  double* rd = tmp.get<double>((size_t)nbits * d);
  double* td = thr ? tmp.get<double>((size_t)nbits) : nullptr;
  uint8_t* od = tmp.get<uint8_t>((size_t)blk * nb);
  if (!xd || !rd || (thr && !td) || !od) return fail(MI_ERR_NOMEM, "LSH encode buffers");
  HIPC(hipMemcpy(rd, R, (size_t)nbits * d * 8, hipMemcpyHostToDevice));
  if (thr) HIPC(hipMemcpy(td, thr, (size_t)nbits * 8, hipMemcpyHostToDevice));
  const bool packed = col_stride == 1 && (row_stride == d || n == 1);
  std::vector<char> pack;
  for (int64_t r = 0; r < n; r += step) {
    const int64_t mm = std::min(step, n - r);
    const char* src = (const char*)X + (size_t)r * (size_t)row_stride * esz;
    if (!packed) {                                          // any other layout: the block is packed on the host first
      pack.resize((size_t)mm * d * esz);
      for (int64_t i = 0; i < mm; ++i)
        for (int32_t c = 0; c < d; ++c)
          std::memcpy(pack.data() + ((size_t)i * d + c) * esz, src + ((size_t)i * row_stride + (size_t)c * col_stride) * esz, esz);
      src = pack.data();
    }
    HIPC(hipMemcpy(xd, src, (size_t)mm * d * esz, hipMemcpyHostToDevice));
    launch_lsh_encode(xd, dtype, mm, d, d, 1, rd, td, nbits, od, nb, nullptr, 0, nullptr);
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(out + (size_t)r * nb, od, (size_t)mm * nb, hipMemcpyDeviceToHost));   // (synchronous: xd and od are free again)
  }
  return MI_OK;
}

int mi_hamming_append_lsh_device(mi_hamming* h, const void* X_dev, int64_t m, int32_t d, int dtype, int64_t row_stride,
                                 int64_t col_stride, const double* R_dev, const double* thr_dev, void* stream) {
  REQUIRE(h, "null handle");
  const int rc = lsh_check(m, d, dtype, row_stride, col_stride, R_dev, h->nbits, "m");
  if (rc != MI_OK) return rc;
  REQUIRE(X_dev || m == 0, "null pointer: X_dev");
  REQUIRE(h->n + m <= h->cap, "index capacity exceeded");
  if (m == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  launch_lsh_encode(X_dev, dtype, m, d, row_stride, col_stride, R_dev, thr_dev, h->nbits, nullptr, 0, h->codes, h->n,
                    (hipStream_t)stream);
  HIPC(hipGetLastError());
  h->n += m;
  return MI_OK;
}

}  // extern "C"
