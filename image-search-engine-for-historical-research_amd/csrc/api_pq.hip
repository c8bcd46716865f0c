// PQ index of the C ABI: exact ADC top-K on product-quantized codes (mi_pq; kernels in csrc/pq.hip).
// The reference's matching_PQ_Net (src/utils/nnsearch.py:905-946), nanopq's dtable / adist, faiss IndexPQ.search.  A handle of its
// own: codebooks, codes in transposed 64-row blocks, a float32 matrix of negated distances of at most "pq_matrix_bytes" (queries
// go through it in chunks), grow-only staging for rows, tables, bitmap and results.  The answer is a function of the inputs
// alone (float64 table entries rounded once, float32 sums in book order, order by (distance, id)): no certificate, no flag.
// The host functions are pq_flat.h's, shared with the wide index (api_pq_wide.hip): the entry points below forward to them with
// H = mi_pq.  What only this index has is here: the row removal, and the search core as a symbol for api_pq_graph.hip.
#include "pq_flat.h"

int pq_search_core(mi_pq* h, const void* q_dev, int dtype, int64_t rs, int64_t cs, int64_t nq, int32_t k,
                   const uint64_t* allow_dev, int64_t* out_idx_dev, float* out_dist_dev, hipStream_t s) {
  return pq_flat_search_core(h, q_dev, dtype, rs, cs, nq, k, allow_dev, out_idx_dev, out_dist_dev, s);
}

int remove_plan(const uint64_t* remove_bits, int memspace, int64_t n, RemovePlan* plan) {
  const int64_t nwords = (n + 63) / 64;
  plan->keep.resize((size_t)nwords);
  plan->prefix.resize((size_t)nwords + 1);
  plan->removed = 0, plan->first = -1;
  if (memspace == MI_HOST) std::memcpy(plan->keep.data(), remove_bits, (size_t)nwords * 8);
  else HIPC(hipMemcpy(plan->keep.data(), remove_bits, (size_t)nwords * 8, hipMemcpyDeviceToHost));
  const uint64_t tail = n % 64 ? (1ull << (n % 64)) - 1ull : ~0ull;
  int64_t kept = 0;
  for (int64_t w = 0; w < nwords; ++w) {
    const uint64_t in = w == nwords - 1 ? tail : ~0ull;
    const uint64_t v = plan->keep[(size_t)w] & in;
    if (v && plan->first < 0) plan->first = w * 64 + __builtin_ctzll(v);
    plan->removed += __builtin_popcountll(v);
    plan->keep[(size_t)w] = ~v & in;
    plan->prefix[(size_t)w] = (uint32_t)kept;
    kept += __builtin_popcountll(~v & in);
  }
  plan->prefix[(size_t)nwords] = (uint32_t)kept;
  return MI_OK;
}

extern "C" {

int mi_pq_create(const float* codebooks_host, int32_t d, int32_t m, int32_t ks, const void* codes, int64_t n, int64_t row_stride_bytes,
                 int memspace, int device, int64_t row_offset, int64_t capacity, mi_pq** out) {
  return pq_flat_create(codebooks_host, d, m, ks, codes, n, row_stride_bytes, memspace, device, row_offset, capacity, out);
}

int mi_pq_append_codes(mi_pq* h, const void* codes, int64_t rows, int64_t row_stride_bytes, int memspace) {
  return pq_flat_append_codes(h, codes, rows, row_stride_bytes, memspace);
}

int mi_pq_add(mi_pq* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace) {
  return pq_flat_add(h, x, rows, dtype, row_stride, col_stride, memspace);
}

int mi_pq_encode(mi_pq* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace,
                 uint8_t* out_codes_host) {
  return pq_flat_encode(h, x, rows, dtype, row_stride, col_stride, memspace, out_codes_host);
}

int mi_pq_dtable(mi_pq* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, float* out_table_host) {
  return pq_flat_dtable(h, q, nq, dtype, row_stride, col_stride, out_table_host);
}

int mi_pq_search(mi_pq* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                 const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_dist, double* out_seconds) {
  return pq_flat_search(h, q, nq, dtype, row_stride, col_stride, k, allow_bits, allow_memspace, out_idx, out_dist, out_seconds);
}

int mi_pq_search_device(mi_pq* h, const float* q_dev, int64_t nq, int32_t k, const uint64_t* allow_bits_dev, int64_t* out_idx_dev,
                        float* out_dist_dev, void* stream) {
  return pq_flat_search_device(h, q_dev, nq, k, allow_bits_dev, out_idx_dev, out_dist_dev, stream);
}

int mi_pq_info(const mi_pq* h, int64_t* n, int32_t* d, int32_t* m, int32_t* ks, int32_t* device, int64_t* row_offset, int64_t* capacity,
               int64_t* hbm_bytes) {
  return pq_flat_info(h, n, d, m, ks, device, row_offset, capacity, hbm_bytes);
}

int mi_pq_get_codes(mi_pq* h, int64_t row0, int64_t nrows, uint8_t* out_host) { return pq_flat_get_codes(h, row0, nrows, out_host); }

int mi_pq_decode(mi_pq* h, int64_t row0, int64_t nrows, float* out_host) { return pq_flat_decode(h, row0, nrows, out_host); }

int mi_pq_get_codebooks(const mi_pq* h, float* out_host) { return pq_flat_get_codebooks(h, out_host); }

// Row removal in place (faiss IndexPQ.remove_ids): `codes` compacted stably through a staging area of at most B
// rows (global option "pq_remove_block_rows").  The rows pass in chunks of B source rows, ascending, from the block of the first
// row that leaves: a chunk's survivors are gathered into the staging area at their new positions, then written to the index.
// A survivor never moves up, so a chunk's destination [d0, d0 + count) ends at or before the chunk's own last source row: what it
// overwrites are rows this chunk or an earlier one has read, the chunks behind it are unread sources, and the rows below d0
// are final.  Device memory beyond the index: the staging area, the bitmap and 4 bytes per bitmap word, all grow-only on the
// handle and all allocated before anything moves.
int mi_pq_remove_rows(mi_pq* h, const uint64_t* remove_bits, int memspace, int64_t* out_removed) {
  REQUIRE(h, "null handle");
  REQUIRE(remove_bits, "null pointer: remove_bits");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  if (out_removed) *out_removed = 0;
  std::lock_guard<std::mutex> lock(h->mu);
  const int64_t n = h->n;
  if (n == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  HIPC(hipStreamSynchronize(s));
  RemovePlan plan;
  int rc;
  if ((rc = remove_plan(remove_bits, memspace, n, &plan)) != MI_OK) return rc;
  if (plan.removed == 0) return MI_OK;                        // nothing changes
  const int64_t m = n - plan.removed;                         // n'
  // m == first: only trailing rows leave, no survivor lies behind a row that leaves, nothing moves
  if (m > plan.first) {
    const int64_t nwords = (n + 63) / 64;
    const int64_t blk_words = (int64_t)h->MW * 64;
    const int64_t start = plan.first / 64;                    // the blocks before the first row that leaves stay as they are
    const int64_t B = std::min<int64_t>(g_pq_remove_block_rows.load(), (nwords - start) * 64) / 64;   // source blocks per chunk
    if ((rc = h->bits.grow((size_t)nwords)) != MI_OK) return rc;
    if ((rc = h->rmpref.grow((size_t)nwords + 1)) != MI_OK) return rc;
    // a chunk's first survivor may sit in any lane of its destination block: one block more than the chunk's rows fill
    if ((rc = h->rmstage.grow((size_t)((B + 1) * blk_words))) != MI_OK) return rc;
    HIPC(hipMemcpyAsync(h->bits, plan.keep.data(), (size_t)nwords * 8, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(h->rmpref, plan.prefix.data(), ((size_t)nwords + 1) * 4, hipMemcpyHostToDevice, s));
    for (int64_t b0 = start; b0 < nwords; b0 += B) {
      const int64_t b1 = std::min(b0 + B, nwords);
      const int64_t d0 = plan.prefix[(size_t)b0], count = (int64_t)plan.prefix[(size_t)b1] - d0;
      if (count == 0) continue;
      const int64_t lo = d0 % 64;
      launch_pq_remove_gather(h->codes, h->m, h->bits, h->rmpref, b0, b1, d0 / 64, h->rmstage, s);
      launch_pq_remove_writeback(h->rmstage, h->m, d0 / 64, lo, lo + count, h->codes, s);
    }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
  }
  h->n = m;
  ++h->mod;
  if (out_removed) *out_removed = plan.removed;
  return MI_OK;
}

int mi_pq_destroy(mi_pq* h) { return pq_flat_destroy(h); }

}  // extern "C"
