// Wide PQ index of the C ABI: exact ADC top-K on product-quantized codes of up to 8192 codewords per book (mi_pqw; the scan in
// csrc/pq_wide.hip, every other kernel in csrc/pq.hip and dense.hip).  The reference's matching_Nano_PQ as its
// entry points call it: N_books = 16, n_bits_perbook = 13 (src/offline.py:110).  mi_pq entry point for entry point, with uint16
// codes: the host functions are the ones mi_pq runs (pq_flat.h, H = mi_pqw; PqTraits there lists what differs), so the contract --
// table entries, float32 sums in book order, order by (distance, id), the encoder's argmin -- is mi_pq's, and for ks <= 256 so is
// every output bit.  Training is mi_pqw_train (api_pq_train.hip).
#include "pq_flat.h"

extern "C" {

int mi_pqw_create(const float* codebooks_host, int32_t d, int32_t m, int32_t ks, const void* codes, int64_t n, int64_t row_stride,
                 int memspace, int device, int64_t row_offset, int64_t capacity, mi_pqw** out) {
  return pq_flat_create(codebooks_host, d, m, ks, codes, n, row_stride, memspace, device, row_offset, capacity, out);
}

int mi_pqw_append_codes(mi_pqw* h, const void* codes, int64_t rows, int64_t row_stride, int memspace) {
  return pq_flat_append_codes(h, codes, rows, row_stride, memspace);
}

int mi_pqw_add(mi_pqw* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace) {
  return pq_flat_add(h, x, rows, dtype, row_stride, col_stride, memspace);
}

int mi_pqw_encode(mi_pqw* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace,
                 uint16_t* out_codes_host) {
  return pq_flat_encode(h, x, rows, dtype, row_stride, col_stride, memspace, out_codes_host);
}

int mi_pqw_dtable(mi_pqw* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, float* out_table_host) {
  return pq_flat_dtable(h, q, nq, dtype, row_stride, col_stride, out_table_host);
}

int mi_pqw_search(mi_pqw* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                 const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_dist, double* out_seconds) {
  return pq_flat_search(h, q, nq, dtype, row_stride, col_stride, k, allow_bits, allow_memspace, out_idx, out_dist, out_seconds);
}

int mi_pqw_search_device(mi_pqw* h, const float* q_dev, int64_t nq, int32_t k, const uint64_t* allow_bits_dev, int64_t* out_idx_dev,
                        float* out_dist_dev, void* stream) {
  return pq_flat_search_device(h, q_dev, nq, k, allow_bits_dev, out_idx_dev, out_dist_dev, stream);
}

int mi_pqw_info(const mi_pqw* h, int64_t* n, int32_t* d, int32_t* m, int32_t* ks, int32_t* device, int64_t* row_offset, int64_t* capacity,
               int64_t* hbm_bytes) {
  return pq_flat_info(h, n, d, m, ks, device, row_offset, capacity, hbm_bytes);
}

int mi_pqw_get_codes(mi_pqw* h, int64_t row0, int64_t nrows, uint16_t* out_host) { return pq_flat_get_codes(h, row0, nrows, out_host); }

int mi_pqw_decode(mi_pqw* h, int64_t row0, int64_t nrows, float* out_host) { return pq_flat_decode(h, row0, nrows, out_host); }

int mi_pqw_get_codebooks(const mi_pqw* h, float* out_host) { return pq_flat_get_codebooks(h, out_host); }

int mi_pqw_destroy(mi_pqw* h) { return pq_flat_destroy(h); }

}  // extern "C"
