// Host-callable launchers of the gfx950 kernels (internal).
#pragma once
#include "common.h"

namespace mi {

// ingest.hip
// strided source -> row-major [m][d] copy of the same element type (scratch for layouts launch_ingest does not take in one pass)
void launch_transpose_rows(const void* src, int dtype, int64_t m, int32_t d, int64_t rs, int64_t cs, void* dst, hipStream_t stream);
bool ingest_takes_layout(int32_t d, int64_t rs, int64_t cs);
bool ingest_takes_layout(int32_t d, int32_t dp, int64_t rs, int64_t cs);   // rows stored dp >= round_up(d, 64) wide
void launch_ingest(const void* src, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, int norm_mode,
                   float* out_f32, void* out_img, int img_f16, RowStat* rowstat, int32_t dp, int64_t npad, hipStream_t stream,
                   int64_t row_base = 0);
// query batch of the search path: ingest + the per-query search state (launch_init_query_state) in ONE launch; returns false
// (nothing launched) when the rows are too wide for it
bool launch_ingest_queries(const void* src, int dtype, int32_t nq, int32_t d, int64_t rs, int64_t cs, int norm_mode,
                           float* out_f32, void* out_img, int img_f16, RowStat* rowstat, int32_t dp, int32_t qpad,
                           const float* gstat3, float gamma, int use_img_terms, uint32_t first_cnt, const struct QueryState& st,
                           hipStream_t stream, uint32_t zero_scores = 0);
// bootstrap sample image (n_s = multiple of TILE rows, one hashed draw per stratum of the shard)
void launch_build_sample(const void* gal_img, void* samp_img, int64_t n, int64_t n_s, int32_t dp, hipStream_t stream);
void launch_build_sample_f32(const float* gal_f32, float* samp_f32, int64_t n, int64_t n_s, int32_t dp, hipStream_t stream);
int64_t sample_source_row_host(int64_t i, int64_t n, int64_t n_s);   // row_base: output rows start here (gallery append); src row 0 <-> row_base
void launch_checksum(const void* data, size_t bytes, unsigned long long* out_dev, hipStream_t stream);   // bytes % 8 == 0
void launch_rowstat_max(const RowStat* rowstat, int64_t n, float* out3, hipStream_t stream, bool reset = true);
// *flag = 1 if a row with a finite f32 norm (any_f32: any row) has a non-finite image norm (an element beyond the image type's
// range), else 0
void launch_rowstat_img_overflow(const RowStat* rowstat, int64_t n, uint32_t* flag, hipStream_t stream, bool any_f32 = false);

// gemm_select.hip -- fp16/bf16 MFMA scoring of gallery tiles [tile0, tile0+ntiles) against nqt query tiles with the
// fused survivor filter.  first != 0: store every score of the chunk (rows tile0*256.. at position row).
struct ScoreArgs {
  const void* gal_img;   // blocked image of the shard
  const void* qry_img;   // blocked image of the query batch
  int32_t img_f16;        // 16-bit image element type: 1 = fp16, 0 = bf16
  int32_t nslices;        // dp / 32
  int32_t tile0, ntiles;  // gallery tiles of this launch
  int32_t nqt;            // query tiles (qpad / 256)
  int64_t n;              // valid gallery rows in the shard
  int32_t nq;             // valid queries
  int32_t small_batch_kernel;   // 1: launches with <= STREAM_MAX_QUERIES queries go to stream_select.hip
  SurvRec* rec;           // [grid * 8 waves][rec_cap] wave-private survivor records of this launch
  uint32_t* rec_cnt;      // [grid * 8]
  uint32_t rec_cap;
  const uint32_t* cond;   // non-null: the whole launch is skipped when *cond == 0 (repair pass)
  const XccBalance* bal = nullptr;   // non-null: weighted split of the gallery tiles over the XCD labels (tile kernel)
  int32_t lad_k = 0;                 // > 0: in-launch threshold ladder on (K of the search); tile kernel, filtered launch only
  int32_t scores_only = 0;           // bootstrap launch on the sample image (stream_select MODE 2): store the scores as 4-byte
                                     // floats at ((float*)(surv + q * cap))[sample row] instead of 8-byte (score, row) entries --
                                     // sample_threshold_kernel reads nothing but the scores, and the entries are dropped afterwards
  float* samp_out = nullptr;         // scores_only: non-null -> the scores go to samp_out[q * samp_ld + sample row] instead of the
  uint32_t samp_ld = 0;              // survivor rows (the 65 536-row sample of shards beyond 3.9 M rows does not fit one)
  int32_t ksplit = 1;                // bootstrap launch with scores_only: workgroups per (sample tile, query group), each taking
                                     // nslices / ksplit K-slices and ADDING its partial scores (atomic f32 adds onto zeros
                                     // written by the query ingest): small batches have 32 .. 64 bootstrap workgroups of 64
                                     // serial slices each otherwise.  The sum order is then not fixed -- the sample scores
                                     // feed the speculative (verified) threshold and the ladder level only
  unsigned long long* dbg; // tile kernel, per wave [grid * 8][8]: word 3 = records emitted, 4 = XCC id, 5 = K-slices done, 6 = shader
                           // cycles, 7 = 10-ns ticks around the main loop (kernel_clock_mhz, the XCD shares); null: not written
  QueryState st;
};
// stream_select.hip: the scoring + filter launch for small query batches (HBM-bound; same records and thresholds)
constexpr int STREAM_MAX_QUERIES = 128;
bool stream_select_applies(const ScoreArgs& a);
bool stream_bootstrap_applies(const ScoreArgs& a);   // bootstrap launches of any batch size
void launch_stream_select(const ScoreArgs& a, bool first, hipStream_t stream);
void launch_gemm_select(const ScoreArgs& a, bool first, hipStream_t stream);
unsigned gemm_select_grid();   // persistent grid size (workgroups); record segments = grid * 8
// A wave whose private record segment is full (rec_cap records in one launch: ten times what a batch of descriptors leaves
// per wave, but a batch whose queries are ordered like the gallery -- five queries per landmark, landmarks stored together:
// bench.py `hard_data` -- or a batch of near-identical queries concentrates its survivors on the few waves that own the
// matching (gallery tile, query block) pairs) appends the record straight to its query's survivor bucket: one RETURNING atomic
// per record on this cold path (it drains the wave's DMA ring, which is why the hot path avoids it), the same counter
// scatter_records_kernel adds to afterwards.  Round 5 raised FLAG_REC_OVERFLOW instead and the whole batch was answered again.
__device__ __forceinline__ void spill_record(const QueryState& st, float score, uint32_t row, uint32_t q) {
  const uint32_t pos = atomicAdd(&st.cnt[q * CNT_STRIDE], 1u);
  if (pos < st.cap) st.surv[(uint64_t)q * st.cap + pos] = pack_entry(score, row);
  else atomicOr(st.flags, FLAG_SURV_OVERFLOW);
}

// Timing of ONE scoring launch without extra packets on the stream: the next launch_gemm_select / launch_stream_select of
// this thread goes out through hipExtLaunchKernelGGL with these events, which receive the begin / end timestamps of the
// dispatch itself (events recorded around a launch with hipEventRecord are barrier packets of their own: ~5 us of gap
// before and after a 3 ms kernel).  Consumed by that launch.
void set_launch_events(hipEvent_t start, hipEvent_t stop);
void take_launch_events(hipEvent_t* start, hipEvent_t* stop);
// buckets the wave-private records of the last scoring launch into the per-query survivor buffers
// bal / dbg / ntiles non-null / non-zero: block 0 also updates the XCD shares from the loop times of the launch that wrote dbg
void launch_scatter_records(const SurvRec* rec, const uint32_t* rec_cnt, uint32_t rec_cap, uint32_t nseg,
                            QueryState st, const uint32_t* cond, hipStream_t stream, XccBalance* bal = nullptr,
                            const unsigned long long* dbg = nullptr, uint32_t ntiles = 0, int32_t nq = 0);   // nq: queries of the batch
void init_xcc_balance_host(XccBalance* host);
void init_xcc_balance_from(XccBalance* host, const float* w8);   // from remembered shares (file / process cache)

// exact_score.hip -- f32 FMA scoring with the same filter (fallback / force_exact)
struct ExactArgs {
  const float* gal_f32;   // [n][dp]
  const float* qry_f32;   // [qpad][dp]
  int32_t dp;
  int64_t row0, row1;     // gallery rows of this launch
  int64_t n;
  int32_t nq;
  QueryState st;
  float* dense_out = nullptr;   // non-null: dense mode, scores to dense_out[q * dense_ld + row]
  int64_t dense_ld = 0;
};
void launch_exact_select(const ExactArgs& a, bool first, hipStream_t stream);

// select.hip
void launch_init_query_state(const RowStat* qstat, const float* gstat3, int32_t nq, int32_t qpad, float gamma,
                             int use_img_terms, uint32_t first_cnt, QueryState st, hipStream_t stream);
// mode 0: maintain (threshold <- K-th largest - margin, compact survivors)
// mode 1: maintain + write the K largest approximate values to topvals[q][K] and L_local[q]
// thresholds from the 2048 / 4096 / 8192-score bootstrap sample (single-launch schedule), cheaper than launch_select_maintain(mode 0)
bool sample_threshold_applies(uint32_t first_cnt, int32_t k, int32_t spec_r);
// the r-th / (4 r)-th / lad_r-th largest of n sample scores per query read from scores[q * ld + i] (samples too large for a survivor row)
void launch_sample_threshold_big(QueryState st, const float* scores, uint32_t ld, uint32_t n, int32_t nq, int32_t k,
                                 int32_t spec_r, int32_t lad_r, float order_slack, hipStream_t stream);
void launch_sample_threshold(QueryState st, int32_t nq, int32_t k, int32_t spec_r, uint32_t first_cnt, hipStream_t stream,
                             int32_t lad_r = 0, int32_t f32_scores = 0, float order_slack = 0.f);   // f32_scores: see ScoreArgs::scores_only
// what the in-kernel repair of a failed query scans (repair == 3): the shard's stored f32 rows and the batch's f32 queries
struct RepairScan {
  const float* gal_f32 = nullptr;
  const float* qry_f32 = nullptr;
  int32_t dp = 0;
  int64_t n = 0;
  uint64_t* repairs = nullptr;   // per query: in-kernel repairs so far (one writer per word; summed by mi_search_status)
};
void launch_select_maintain(QueryState st, int32_t nq, int32_t k, int mode, float* topvals, float* l_local,
                            uint64_t* stats2, int32_t spec_r, int32_t spec, int32_t repair, const uint32_t* cond,
                            hipStream_t stream, uint32_t* cand_rows = nullptr, uint32_t* cand_cnt = nullptr,
                            uint32_t rcap = 0,   // cand_*: mode 1 also writes the candidate rows (single-shard search)
                            const RepairScan* scan = nullptr);   // repair == 3: the workgroup of a failed query re-scans the shard
void launch_select_candidates(QueryState st, int32_t nq, const float* L, uint32_t* cand_rows, uint32_t* cand_cnt,
                              uint32_t rcap, uint64_t* stats2, hipStream_t stream);
void launch_rescore(const float* gal_f32, const float* qry_f32, int32_t dp, int32_t nq, const uint32_t* cand_rows,
                    const uint32_t* cand_cnt, uint32_t rcap, double* cand_score, hipStream_t stream,
                    uint32_t grid_x, uint32_t last_row);   // last_row: n - 1 of the shard (row ids are clamped to it)
void launch_rescore_resident(const float* gal_f32, const float* qry_f32, int32_t dp, int32_t nq, const uint32_t* cand_rows,
                             const uint32_t* cand_cnt, uint32_t rcap, double* cand_score, hipStream_t stream,
                             uint32_t last_row);
void launch_emit(const uint32_t* cand_rows, const uint32_t* cand_cnt, const double* cand_score, uint32_t rcap,
                 int32_t nq, int32_t k, int64_t row_offset, int64_t* out_idx, float* out_score,
                 double* out_score64, uint32_t* short_flag, hipStream_t stream);
void launch_kth_of_gathered(const float* gathered, int32_t nshards, int64_t nq, int32_t k, float* out_L,
                            hipStream_t stream);
void launch_merge(const double* score64, const int64_t* idx, int32_t nshards, int64_t nq, int32_t k, int64_t shard_stride,
                  int64_t* out_idx, float* out_score, hipStream_t stream);

// range_select.hip -- exact range search (api_range.hip): fixed threshold, survivor rows for rescore_kernel, rows kept at
// f64 score >= min_score (CSR per chunk, keyed by ~f64_key_nan_lowest(score)), per-query counts / offsets, the gather into the
// batch's CSR list; csr_order.hip orders it and writes it out
void launch_range_threshold(QueryState st, int32_t nq, int32_t qpad, double min_score, hipStream_t stream);
void launch_range_chunk_begin(QueryState st, int32_t qpad, unsigned long long* total, hipStream_t stream);
void launch_range_rows(QueryState st, int32_t nq, uint32_t* rows, uint32_t* rcnt, int dense, uint32_t row0, uint32_t nrows,
                       hipStream_t stream);
void launch_range_keep(const uint32_t* rows, const uint32_t* rcnt, const double* sc, uint32_t lcap, int32_t nq, double min_score,
                       unsigned long long* total, uint64_t* off, uint32_t* cnt, uint64_t* key, uint32_t* row, uint64_t base,
                       uint64_t cap, uint32_t* flags, hipStream_t stream);
void launch_range_lims(const uint32_t* cnt, int32_t nchunks, int32_t ld, int32_t nq, int64_t* lims, hipStream_t stream);
void launch_range_gather(const uint64_t* akey, const uint32_t* arow, const uint64_t* off, const uint32_t* cnt, int32_t nchunks,
                         int32_t ld, int32_t nq, const int64_t* lims, uint64_t* key, uint32_t* row, hipStream_t stream);

// csr_order.hip -- the ordering stage of the range searches (api_range.hip, api_minkowski_range.hip): the CSR list of
// a chunk of queries, (uint64 key, uint32 local row) entries, ordered per query by (key asc, row asc) and written out
struct CsrList {
  int32_t nq = 0;                    // queries of the chunk (<= 65535)
  int64_t* lims = nullptr;           // the CSR offsets from the chunk's first query on: [nq + 1]
  const int64_t* total = nullptr;    // the call's hit count on the device; nothing is written once *total > max_results
  int64_t max_results = 0;
  uint64_t* key[2] = {nullptr, nullptr};   // the chunk's hits from place 0 on: keys and local rows, ping-pong of the merge passes
  uint32_t* row[2] = {nullptr, nullptr};
};
// buffer 0 holds the lists; max_cnt: no query of the chunk has more hits, max_total: the chunk has no more.  -> the buffer (0 or 1)
// that holds the ordered lists
int launch_csr_order(const CsrList& a, int64_t max_cnt, int64_t max_total, hipStream_t stream);
// the ordered lists of buffer `cur` -> out_*[lims[0] ..]: id = row_offset + row, value = the float64 behind the key (complement: behind
// ~key, for lists keyed by ~f64_key_nan_lowest(value)) and its float32.  out_idx is written, either value output may be NULL
void launch_csr_write(const CsrList& a, int cur, bool complement, int64_t max_total, int64_t row_offset, int64_t* out_idx, float* out_val,
                      double* out_val64, hipStream_t stream);
int64_t csr_run_length();            // entries of one LDS-sorted run

// dense.hip -- exact top-k of dense score rows (global-memory radix select + LDS bitonic sort), k <= 4096
void launch_dense_topk(const float* scores, int64_t ld, int64_t n, int32_t nq, int32_t k, int64_t row_offset,
                       int64_t* out_idx, float* out_score, hipStream_t stream);

// last resort of the exhaustive search (massive ties): dense f64 scores of every row + exact top-k of them
void launch_dense_score64(const float* gal_f32, const float* qry_f32, int32_t dp, int64_t n, int32_t nq, double* out,
                          int64_t ld, hipStream_t stream);
void launch_dense_topk64(const double* scores, int64_t ld, int64_t n, int32_t nq, int32_t k, int64_t row_offset,
                         int64_t* out_idx, float* out_score, double* out_score64, hipStream_t stream);
void launch_rank_all(const float* scores, int64_t ld, int64_t n, int32_t nq, uint32_t* keys_a, uint32_t* idx_a,
                     uint32_t* keys_b, uint32_t* idx_b, int64_t row_offset, int64_t* out_idx, float* out_score,
                     hipStream_t stream);

void launch_rank_positions(const float* scores, int64_t ld, int64_t n, int32_t nq, const int64_t* ids, int32_t m,
                           int64_t row_offset, unsigned long long* out_pos, hipStream_t stream);
int rank_positions_max_listed();

// diffusion.hip
void launch_affinity(const int64_t* ids, const float* sims, int64_t ld, int64_t n, int32_t kd, int32_t gamma,
                     float alpha, float* lap, float* dinv, float* diag, hipStream_t stream);
void launch_diffusion_cg(const int64_t* ids, int64_t ld, int64_t n, int32_t T, int32_t kd, const float* lap,
                         const float* diag, int32_t maxiter, double tol, int32_t* map_all, unsigned grid,
                         int32_t* out_ids, float* out_vals, hipStream_t stream, int64_t node0 = 0,
                         int64_t node1 = -1);
void launch_diffusion_combine(const int64_t* nn_idx, const float* nn_sims, int32_t kq, int32_t gamma,
                              const int32_t* off_ids, const float* off_vals, int32_t T, int64_t n, int32_t nq,
                              float* dense, hipStream_t stream);

// kr_rerank.hip -- k-reciprocal re-ranking (src/utils/Reranking.py:447-624)
void launch_kr_pack(const void* src, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, float* out, int32_t dp,
                    hipStream_t stream);
void launch_kr_sets(const int64_t* rank, int ld, int all, int k1, int32_t* R, int32_t* Rcnt, uint32_t* flags,
                    hipStream_t stream);
void launch_kr_weights(const float* S, int all, const int32_t* R, const int32_t* Rcnt, float* V, float* dmax,
                       hipStream_t stream);
void launch_kr_expand(const int64_t* rank, int ld, int k2, int all, const int32_t* R, const int32_t* Rcnt, const float* V,
                      void* Vqe, void* VqeT, hipStream_t stream);
void launch_kr_final(const void* Vqe, const void* VqeT, bool f32, const float* S, const float* dmax, int all, int nq,
                     float w_jac, float w_org, float* neg_final, uint32_t* flags, hipStream_t stream);
int kr_rmax();

// whiten.hip
void launch_whiten(const void* X, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, const double* m,
                   const double* P, int32_t dims, double eps, double* Y, hipStream_t stream);

// scatter.hip -- scatter matrix C (+)= sum (x - c)(x - c)^T (rows) or sum (x_q - x_p)(x_q - x_p)^T (pairs), f64 MFMA, upper
// tiles + mirror, split reduction combined in a fixed order through `workspace` (scatter_workspace_bytes(d) bytes)
int scatter_max_splits(int32_t d);            // 0: d is beyond what the 512 MiB workspace bound allows
int64_t scatter_workspace_bytes(int32_t d);
void launch_scatter(const void* X, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, const double* centre,
                    const int64_t* pair_q, const int64_t* pair_p, int64_t n_pairs, double* C, int accumulate,
                    double* workspace, hipStream_t stream);

// desc_tail.hip
// widest input of the whitening layer: linear_rows_kernel stages 8 rows of c floats in dynamic LDS, 8 * 4968 * 4 = 158 976
// bytes of the CU's 163 840; launch_desc_tail opts the kernel in for exactly this, mi_desc_tail_device refuses more
constexpr int32_t DESC_TAIL_MAX_C = 4968;
void launch_desc_tail(const float* feat, int32_t b, int32_t c, int32_t hw, float p, float eps, const float* W,
                      const float* bias, int32_t c_out, float* pooled, float* out, hipStream_t stream);
void launch_ms_accumulate(float* acc, const float* desc, int64_t count, float msp, int first, hipStream_t stream);
void launch_ms_finish(float* acc, int32_t b, int32_t d, int32_t nscales, float msp, hipStream_t stream);

// aqe.hip
void launch_aqe_partial(const float* gal_f32, int32_t dp, int32_t d, int64_t n, int64_t row_offset,
                        const int64_t* ranks, int64_t sj, int64_t sq, int64_t nq, int32_t k_qe, double w,
                        const double* weights, double* out_sum, hipStream_t stream);
void launch_aqe_rows(const float* gal_f32, int32_t dp, int32_t d, int64_t n, int64_t row_offset, const int64_t* ranks,
                     int64_t sj, int64_t sq, int64_t nq, int32_t k_qe, float* out_rows, hipStream_t stream);
void launch_aqe_combine(const float* rows, int64_t nq, int32_t d, int32_t k_qe, double w, const double* weights,
                        double* out_sum, hipStream_t stream);
void launch_column_sum(const void* X, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, double* out,
                       hipStream_t stream);
void launch_aqe_finish(const double* sum, int64_t nq, int32_t d, double eps, float* out_q, double* out_q64,
                       hipStream_t stream);

// filter_select.hip -- filtered top-K search (api_filter.hip): allow bitmap -> ascending allowed rows (count, one-workgroup
// scan, compaction), the compacted sub-gallery's rows, the over-fetch selection with its certificate, the id remap
int64_t filter_blocks(int64_t n);   // workgroups of the count / compact kernels (bcnt holds this many, boff one more)
void launch_filter_compact(const uint64_t* bits, int64_t n, uint32_t* bcnt, uint32_t* boff, uint32_t* rows, hipStream_t stream);
void launch_subset_gather(const float* src_f32, const void* src_img, const RowStat* src_stat, const uint32_t* rows, int64_t m,
                          int64_t mpad, int32_t dp, float* dst_f32, void* dst_img, RowStat* dst_stat, hipStream_t stream);
void launch_filter_overfetch(const int64_t* in_idx, const float* in_sc, int64_t nq, int32_t kp, int32_t k, const uint64_t* bits,
                             int64_t n, int64_t row_offset, int32_t covers, int64_t* out_idx, float* out_sc, uint32_t* ok,
                             hipStream_t stream);
void launch_filter_remap(const int64_t* sidx, const float* ssc, int64_t nq, int32_t ke, int32_t k, const uint32_t* rows,
                         int64_t m, int64_t row_offset, int64_t* out_idx, float* out_sc, hipStream_t stream);

// group_select.hip -- grouped top-K search (api_group.hip).  grp [n]: dense group id of every local row;
// label_of_group [G]: the caller's label (-1 for a singleton row); the group CSR group_off [G + 1] / group_rows [n] (rows of a group
// contiguous, ascending); chunk_g0 [chunks + 1]: the CSR cut into chunks of whole groups of at most GROUP_CHUNK_ROWS rows, a larger
// group being a chunk of its own; excl [nq]: the dense id of the group a query excludes, 0xFFFFFFFF = none
constexpr int GROUP_CHUNK_ROWS = 2048, GROUP_BEST_THREADS = 256;
// in_idx / in_sc [nq][kp <= 2048] -> the first k group-distinct entries [nq][k] (padding -1 / -inf / -1), ok [nq] the certificate
void launch_group_collapse(const int64_t* in_idx, const float* in_sc, int64_t nq, int32_t kp, int32_t k, const uint32_t* grp,
                           const int32_t* label_of_group, int64_t n, int64_t row_offset, const uint32_t* excl, int32_t covers,
                           int64_t* out_idx, float* out_sc, int32_t* out_lab, uint32_t* ok, hipStream_t stream);
// dense [nq][ld] float64 scores -> out_key / out_row [nq][G]: ~f64_key_nan_lowest(best value) and the lowest row that has it, per
// group; the excluded group's entry is (~0, ~0u).  nq <= 65535
void launch_group_best(const double* dense, int64_t ld, int32_t nq, const uint32_t* grp, const uint32_t* group_rows,
                       const uint32_t* group_off, const uint32_t* chunk_g0, int64_t chunks, int64_t G, const uint32_t* excl,
                       uint64_t* out_key, uint32_t* out_row, hipStream_t stream);
void launch_group_lims(int64_t* lims, int64_t* total, int32_t nq, int64_t G, hipStream_t stream);   // lims[i] = i G, *total = 0
// row [nq][G] ordered by csr_order.hip -> cand_rows [nq][k], cand_cnt [nq] (what launch_rescore takes, rcap = k)
void launch_group_take(const uint32_t* row, int64_t G, int32_t nq, int32_t k, uint32_t* cand_rows, uint32_t* cand_cnt,
                       hipStream_t stream);
void launch_group_emit(const uint32_t* cand_rows, const uint32_t* cand_cnt, const double* cand_score, const uint32_t* grp,
                       const int32_t* label_of_group, int32_t nq, int32_t k, int64_t row_offset, int64_t* out_idx, float* out_sc,
                       int32_t* out_lab, hipStream_t stream);

// row_remove.hip -- in-place row removal (api_remove.hip): surviving rows rows[j0 .. j1) (padding rows up to j1_pad, j >= m,
// written as zeros) gathered into a staging area of the gallery's own layout, and the staging area written back as three
// contiguous runs (rows_f32 f32 rows, rows_pad image rows and RowStats)
void launch_remove_gather(const float* src_f32, const void* src_img, const RowStat* src_stat, const uint32_t* rows, int64_t j0,
                          int64_t j1_pad, int64_t m, int32_t dp, float* stg_f32, void* stg_img, RowStat* stg_stat,
                          hipStream_t stream);
void launch_remove_writeback(const float* stg_f32, const void* stg_img, const RowStat* stg_stat, int64_t rows_f32,
                             int64_t rows_pad, int32_t dp, float* dst_f32, void* dst_img, RowStat* dst_stat,
                             hipStream_t stream);

// l2_metric.hip -- squared-L2 metric (api_l2.hip): hidden bias columns of stored rows, query extension, direct-form f64 tail,
// dense direct-form distances (stored negated for launch_dense_topk64) and their emit
void launch_l2_bias(float* gal_f32, void* gal_img, int img_f16, RowStat* rowstat, int32_t dp, int32_t d, int64_t row0,
                    int64_t nrows, int64_t nrows_pad, hipStream_t stream);
void launch_l2_augment(const void* src, int dtype, int64_t nq, int32_t d, int64_t rs, int64_t cs, float* out, int32_t ld,
                       hipStream_t stream);
void launch_l2_tail(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int64_t row_offset,
                    const int64_t* ids, int32_t ke, int32_t k, int64_t nq, int64_t* out_idx, float* out_dist, double* out_dist64,
                    hipStream_t stream);
void launch_l2_dense_dist(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int32_t nq, double* out,
                          int64_t ld, hipStream_t stream);
void launch_l2_dense_emit(const int64_t* idx, const double* neg, int64_t nq, int32_t ke, int32_t k, int64_t* out_idx,
                          float* out_dist, double* out_dist64, hipStream_t stream);

// refine.hip -- exact re-ranking of index shortlists on the stored f32 rows (api_refine.hip; wave arithmetic in l2_wave.h): the
// f64 value of every candidate into val [nq][kc] (one wave per row, grid over (slab, query)), then one workgroup per query sorts
// (value, id), drops repeated ids and writes k rows.  l2 != 0: direct-form distances ascending, else inner products descending.
// qry [nq][dp] with 16-byte aligned rows; kc <= REFINE_MAX_KC; the LDS tier is chosen by kc <= REFINE_SMALL_KC.
constexpr int REFINE_SMALL_KC = 2048, REFINE_MAX_KC = 8192;
void launch_refine(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int64_t row_offset, int l2,
                   const int64_t* cand, int32_t kc, int64_t cand_stride, int32_t k, int64_t nq, double* val, int64_t* out_idx,
                   float* out_val, double* out_val64, hipStream_t stream);

// graph_search.hip -- best-first search of a neighbour graph on the stored f32 rows (api_graph.hip; the walk of graph_walk.h with
// values by l2_wave.h): one workgroup per query, W (the best ef rows, sorted) in LDS, an exact visited bitmap of vis_words 32-bit words per query in `vis`
// ([nq][vis_words], all zero when the launch starts).  adj [n][R] int32 (-1 = padding), entries [ne <= 64], 1 <= k <= ef <=
// GRAPH_MAX_EF, R <= GRAPH_MAX_R.  out_val, out_val64, out_visited may be NULL.
constexpr int GRAPH_MAX_EF = 2048, GRAPH_MAX_R = 64, GRAPH_MAX_ENTRIES = 64;
void launch_graph_search(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int64_t row_offset, int l2,
                         const int32_t* adj, int32_t R, const int32_t* entries, int32_t ne, int32_t k, int32_t ef, int64_t nq,
                         uint32_t* vis, int64_t vis_words, int64_t* out_idx, float* out_val, double* out_val64,
                         int32_t* out_visited, hipStream_t stream);
// graph_build.hip -- the table of mi_graph_build from exact nearest-neighbour lists: forward lists F [n][R] out of a batch of
// search answers, reverse-edge counts and their 64-bit exclusive prefix off [n + 1], then fill / select / compose (cnt and fill
// [n] zeroed by the caller, edges [off[n]], B [n][R] scratch)
void launch_graph_forward(const int64_t* ids, int32_t ks, int64_t row0, int64_t b, int64_t row_offset, int64_t n, int32_t R,
                          int32_t* F, hipStream_t stream);
void launch_graph_rev_count(const int32_t* F, int64_t n, int32_t R, uint32_t* cnt, unsigned long long* off, hipStream_t stream);
void launch_graph_table(const int32_t* F, int64_t n, int32_t R, const unsigned long long* off, uint32_t* fill,
                        unsigned long long* edges, int32_t* B, int32_t* adj, hipStream_t stream);

// hamming.hip -- exact Hamming top-K on packed binary codes (api_hamming.hip): gallery blocks of 64 rows with transposed words
// codes[block][w < ceil(nbits / 32)][64], queries as row-major words [nq][hamming_query_words(W32)], uint16 distance matrix
// [nq][round_up(n, 64)] (0xFFFF = row not admitted), counting selection by (distance asc, id asc)
int32_t hamming_query_words(int32_t W32);       // words per stored query: the register tile of the distance kernel
void launch_hamming_ingest(const uint8_t* src, int64_t stride, int32_t nbits, int64_t row0, int64_t m, uint32_t* codes,
                           hipStream_t stream);
void launch_hamming_query_words(const uint8_t* src, int64_t stride, int32_t nbits, int64_t nq, uint32_t* out, hipStream_t stream);
void launch_hamming_dist(const uint32_t* codes, int32_t nbits, int64_t n, const uint32_t* qw, int32_t nq, const uint64_t* allow,
                         uint16_t* dist, hipStream_t stream);
void launch_hamming_select(const uint16_t* dist, int64_t n, int32_t nbits, int32_t nq, int32_t k, int64_t row_offset,
                           int64_t* out_idx, int32_t* out_dist, hipStream_t stream);
// out_bytes != NULL: rows of d / 8 bytes at out_rs; else the words of rows row0 .. row0 + n of a gallery of d-bit codes
void launch_hamming_sign(const float* x, int64_t n, int32_t d, int64_t rs, uint8_t* out_bytes, int64_t out_rs, uint32_t* codes,
                         int64_t row0, hipStream_t stream);

// hamming_range.hip -- radius search and self-join on the same layout (api_hamming.hip): one 64-bit ballot per (block, query),
// prefix sums of their popcounts as output positions, a stable counting placement per query.  One chunk of queries at a time:
// masks / offs are [blocks scanned][qstride], seg is [ceil(blocks / 64)][qstride], qstride a multiple of 64 >= nq
struct HammingRangeArgs {
  const uint32_t* codes = nullptr;       // the index: [ceil(n / 64)][W32][64]
  int32_t nbits = 0;
  int64_t n = 0;
  int64_t b0 = 0;                        // first block scanned (self-join: the blocks below hold no row above a query)
  const uint32_t* qsrc = nullptr;        // query words [nq][hamming_query_words(W32)]; self: codes
  int64_t qrow0 = 0;                     // self: the stored row that is query 0 of the chunk
  bool self = false;
  int32_t nq = 0;                        // queries of the chunk
  const uint64_t* allow = nullptr;
  uint32_t radius = 0;
  int32_t early = 0;                     // drop a (block, query) once every partial sum is above the radius
  unsigned long long* masks = nullptr;
  uint16_t* offs = nullptr;
  uint32_t* seg = nullptr;
  int64_t qstride = 0;
  const int64_t* lims = nullptr;         // fill / order: CSR offsets of the chunk's queries [nq + 1]
  const int64_t* total = nullptr;        // fill / order: the call's total; above max_results nothing is written
  int64_t max_results = 0;
  unsigned long long* stage = nullptr;   // the chunk's hits in id order: distance << 32 | local row
};
void launch_hamming_range_scan(const HammingRangeArgs& a, hipStream_t stream);
// per-query prefix over the blocks; lims1 != NULL: hit count of query q of the chunk -> lims1[q]
void launch_hamming_range_offsets(const HammingRangeArgs& a, int64_t* lims1, hipStream_t stream);
void launch_hamming_range_lims(int64_t* lims, int64_t nq, hipStream_t stream);   // counts in lims[1 ..] -> offsets, in place
void launch_hamming_range_fill(const HammingRangeArgs& a, hipStream_t stream);
void launch_hamming_range_order(const HammingRangeArgs& a, int64_t row_offset, int64_t* out_idx, int32_t* out_dist,
                                hipStream_t stream);

// components.hip -- connected components of the rows [0, n) (api_components.hip): a union-find forest parent [n] int32 with
// parent[v] <= v, a root hooked only under a smaller root by compare-and-swap, so the label of a component is its smallest row
// whatever the order of the edges.  Ids are checked before a union launch; flatten runs behind the union launches of a call
void launch_components_init(int32_t* parent, int64_t n, hipStream_t stream);                     // parent[v] = v
// a, b (b may be NULL) [m]: an id outside [0, n) raises *flag
void launch_components_check(const int64_t* a, const int64_t* b, int64_t m, int64_t n, uint32_t* flag, hipStream_t stream);
void launch_components_pairs(int32_t* parent, const int64_t* i, const int64_t* j, int64_t m, hipStream_t stream);
// hit idx[t], lims[q] <= t < lims[q + 1], unites row0 + q with idx[t]; total = lims[nq]
void launch_components_csr(int32_t* parent, int64_t row0, const int64_t* lims, const int64_t* idx, int64_t nq, int64_t total,
                           hipStream_t stream);
// masks [nbl][qstride] of a self-join chunk (HammingRangeArgs::masks): bit l of masks[bl][q] unites qrow0 + q with (b0 + bl) 64 + l
void launch_components_ballots(int32_t* parent, const unsigned long long* masks, int64_t b0, int64_t nbl, int64_t qstride,
                               int64_t qrow0, int32_t nq, hipStream_t stream);
void launch_components_flatten(int32_t* parent, int64_t n, hipStream_t stream);                  // parent[v] = root(v)
void launch_components_count(const int32_t* parent, int64_t n, unsigned long long* count, hipStream_t stream);   // *count += roots

// lsh.hip -- LSH codes (api_lsh.hip): bit j of row i = (sum_k double(x[i][k]) R[j][k] >= thr[j]) (thr NULL: 0), f64 MFMA with the
// comparison and the packing in the epilogue.  out != NULL: rows of nbits / 8 bytes at out_rs; else the words of rows dst_row0 ..
// dst_row0 + n of a binary gallery of nbits-bit codes (hamming.hip's layout)
void launch_lsh_encode(const void* X, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, const double* R, const double* thr,
                       int32_t nbits, uint8_t* out, int64_t out_rs, uint32_t* codes, int64_t dst_row0, hipStream_t stream);

// forest_project.hip -- the projections of the random-projection forest (api_forest.hip): out[i * out_rs + c * out_cs]
// = sum_k double(X[i * rs + k * cs]) * R[c][k], f32 rows (any strides, in elements) against float64 directions [C][d], f64 MFMA, K
// ascending over the instruction's steps of 4.  The bits of a sum depend on the row, the direction and d alone
void launch_forest_project(const float* X, int64_t m, int32_t d, int64_t rs, int64_t cs, const double* R, int32_t C, double* out,
                           int64_t out_rs, int64_t out_cs, hipStream_t stream);
// forest_build.hip -- one level of `tg` trees at once.  Pt [tg][L][n]: the projections of the group, one column after another;
// node [tg][n]: the node of every row on this level (read from level 1 on); ids [2][tg][n] and hist [tg][256 * forest_sort_blocks(n)]:
// scratch of the stable LSD radix sort by (node, projection with -0.0 as +0.0, row id).  Writes the level's split values into
// splits [tg][2^L - 1], the nodes of the next level into `node` and, on the last level, the order into leaves [tg][n]
constexpr int FOREST_SORT_CHUNK = 2048;                                     // rows per sort workgroup
static inline int64_t forest_sort_blocks(int64_t n) { return (n + FOREST_SORT_CHUNK - 1) / FOREST_SORT_CHUNK; }
void launch_forest_level(const double* Pt, int64_t n, int32_t tg, int32_t L, int32_t level, int32_t* node, int32_t* ids, uint32_t* hist,
                         double* splits, int32_t* leaves, hipStream_t stream);
// forest_search.hip -- per (query, tree) the descent over the L split levels on the query's projections Pq [nq][T L], then the ids of
// the leaf reached into cand[q * cand_stride + t * leaf_max ..], -1 behind them
void launch_forest_descend(const double* Pq, const double* splits, const int32_t* leaves, int64_t n, int32_t T, int32_t L,
                           int32_t leaf_max, int64_t row_offset, int64_t nq, int64_t* cand, int64_t cand_stride, hipStream_t stream);

// pq.hip -- exact ADC top-K on product-quantized codes (api_pq.hip): codebooks [M][Ks][L] f32, gallery blocks of 64 rows with the
// code bytes four books to a dword and the dwords transposed, codes[block][w < ceil(M / 4)][64]; distance tables [nq][M][Ks] f32;
// a float32 matrix [nq][round_up(n, 64)] of NEGATED distances (NaN = row not admitted) for launch_dense_topk
// (the device code pq.hip, ivfpq.hip and ivfpq_residual.hip share is pq_device.h)
// Check, ingest, encode and decode exist once for both code widths, bytes and the wide index's uint16 (two books to a dword,
// codes[block][w < ceil(M / 2)][64]; pq_wide.hip): overloads on the pointer type; launch_pq_decode takes code_bytes = 1 or 2 and
// writes rows [row0, row0 + nrows) reconstructed, out [nrows][M L] f32
template <typename CodeT> constexpr int32_t pq_codes_per_dword() { return 4 / (int32_t)sizeof(CodeT); }
template <typename CodeT> constexpr int32_t pq_code_dwords(int32_t M) { return (M + pq_codes_per_dword<CodeT>() - 1) / pq_codes_per_dword<CodeT>(); }
void launch_pq_check(const uint8_t* src, int64_t stride, int32_t M, int32_t ks, int64_t m, uint32_t* flag, hipStream_t stream);
void launch_pq_check(const uint16_t* src, int64_t stride, int32_t M, int32_t ks, int64_t m, uint32_t* flag, hipStream_t stream);
void launch_pq_ingest(const uint8_t* src, int64_t stride, int32_t M, int64_t row0, int64_t m, uint32_t* codes, hipStream_t stream);
void launch_pq_ingest(const uint16_t* src, int64_t stride, int32_t M, int64_t row0, int64_t m, uint32_t* codes, hipStream_t stream);
void launch_pq_decode(const uint32_t* codes, int32_t code_bytes, int32_t M, int32_t Ks, int32_t L, const float* cb, int64_t row0,
                      int64_t nrows, float* out, hipStream_t stream);
void launch_pq_table(const void* x, int dtype, int64_t rs, int64_t cs, int64_t nq, const float* cb, int32_t M, int32_t Ks, int32_t L,
                     float* tab, hipStream_t stream);
// packed code bytes out [n][M]
void launch_pq_encode(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const float* cb, int32_t M, int32_t Ks, int32_t L,
                      uint8_t* out, hipStream_t stream);
void launch_pq_encode(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const float* cb, int32_t M, int32_t Ks, int32_t L,
                      uint16_t* out, hipStream_t stream);                // the wide index's codes (pq_wide.hip)
int32_t pq_query_tile(int32_t M, int32_t Ks, int64_t nq);      // queries per workgroup of the scan (1, 2 or 4): the LDS budget
void launch_pq_scan(const uint32_t* codes, int32_t M, int32_t Ks, int64_t n, const float* tab, int32_t nq, int32_t qt,
                    const uint64_t* allow, float* mat, hipStream_t stream);
void launch_pq_emit(const int64_t* tidx, const float* tneg, int64_t nq, int32_t ke, int32_t k, int64_t row_offset, int64_t* out_idx,
                    float* out_dist, hipStream_t stream);

// pq_graph_search.hip -- best-first search of a neighbour graph over the codes of a PQ index (api_pq_graph.hip): the walk of
// graph_walk.h with pq.hip's distances.  tab [nq][M][Ks] f32 as launch_pq_table writes it, codes in the index's transposed blocks; adj,
// entries, vis and the limits as for launch_graph_search; out_dist and out_visited may be NULL.  Dynamic LDS pq_graph_lds_bytes
// (at most 99856 bytes).  The build's queries are launch_pq_decode's rows (pq.hip)
size_t pq_graph_lds_bytes(int32_t M, int32_t Ks, int32_t ef);
void launch_pq_graph_search(const uint32_t* codes, int32_t M, int32_t Ks, const float* tab, int64_t n, int64_t row_offset,
                            const int32_t* adj, int32_t R, const int32_t* entries, int32_t ne, int32_t k, int32_t ef, int64_t nq,
                            uint32_t* vis, int64_t vis_words, int64_t* out_idx, float* out_dist, int32_t* out_visited,
                            hipStream_t stream);

// pq_train.hip -- learning PQ codebooks (api_pq_train.hip): Lloyd's iteration around launch_pq_encode.  cb [M][Ks][L] f32 is updated
// in place (a codeword without members keeps its value); codes [n][M] bytes, cols [M][n] bytes (one contiguous column per book).
// The uint16 overloads are mi_pqw_train's: the same kernels on two-byte codes
void launch_pq_init_rows(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, int32_t M, int32_t Ks, int32_t L, float* cb,
                         hipStream_t stream);
void launch_pq_code_columns(const uint8_t* codes, int32_t M, int64_t n, uint8_t* cols, hipStream_t stream);
// adds the number of differing bytes to *count; a and b 16-byte aligned
void launch_pq_moved(const uint8_t* a, const uint8_t* b, int64_t bytes, unsigned long long* count, hipStream_t stream);
void launch_pq_update(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const uint8_t* cols, int32_t M, int32_t Ks, int32_t L,
                      float* cb, hipStream_t stream);
void launch_pq_code_columns(const uint16_t* codes, int32_t M, int64_t n, uint16_t* cols, hipStream_t stream);
void launch_pq_moved(const uint16_t* a, const uint16_t* b, int64_t bytes, unsigned long long* count, hipStream_t stream);
void launch_pq_update(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const uint16_t* cols, int32_t M, int32_t Ks, int32_t L,
                      float* cb, hipStream_t stream);

// kmeans.hip -- k-means assignment over whole rows at f64 matrix rate (api_kmeans.hip): out[i] = the id of row i's
// nearest centroid of cb [k][d] f32 in the float64 direct form, ties to the lower id -- launch_pq_encode's answer with one book.
// An MFMA kernel decides the rows a rounding certificate covers, a fixed-grid direct-form kernel the rest; *total (may be NULL)
// += the number of rows the latter decided.  Everything is enqueued on `stream`, nothing is read back.  The rows pass in chunks of
// w.rows, so the workspace is bounded whatever n is: km_workspace lays `bytes` at `base` out (rows < 128: too small)
struct KmWorkspace {
  int64_t rows = 0;                  // rows per chunk, a multiple of 128
  double *cn = nullptr, *cmax2 = nullptr, *xn2 = nullptr, *wb = nullptr, *ws = nullptr;
  int32_t* wi = nullptr;
  uint32_t *list = nullptr, *count = nullptr;
};
int64_t km_workspace_bytes(int32_t k, int64_t rows);           // what chunks of `rows` rows need
KmWorkspace km_workspace(void* base, int64_t bytes, int32_t k);
void launch_km_assign(const void* X, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, const float* cb, int32_t k, int32_t* out,
                      unsigned long long* total, const KmWorkspace& w, hipStream_t stream);
void launch_km_assign(const void* X, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, const float* cb, int32_t k, uint16_t* out,
                      unsigned long long* total, const KmWorkspace& w, hipStream_t stream);   // the training's codes

// pq_wide.hip -- exact ADC top-K on wide PQ codes (api_pq_wide.hip): Ks <= 8192, a code is M uint16.  Gallery blocks
// of 64 rows, two books to a dword, dwords transposed: codes[block][w < ceil(M / 2)][64].  Only the scan is this file's: tables,
// matrix, selection and emit are pq.hip's (launch_pq_table, launch_dense_topk, launch_pq_emit), and so are check, ingest, encoder and
// decode (the uint16 overloads above)
constexpr int PQW_MAX_KS = 8192;
int32_t pqw_query_tile(int32_t Ks, int64_t nq);                // queries per workgroup of the scan (1, 2 or 4): the LDS budget
void launch_pqw_scan(const uint32_t* codes, int32_t M, int32_t Ks, int64_t n, const float* tab, int32_t nq, int32_t qt,
                     const uint64_t* allow, float* mat, hipStream_t stream);

// ivfpq.hip -- inverted-file search over PQ codes (api_ivfpq.hip).  Blocks of 64 slots from one pool: codes [pblock][MQ][64] in
// the PQ index's transposed form, rowid [pblock][64] the local row of a slot; list l is the chain of blocks
// blk_table[list_off[l] .. list_off[l + 1]), of whose slots the first list_rows[l] are filled.  probes [nq][nprobe] int32 (-1 = no list), pref [nq][nprobe + 1] the prefix of block
// counts over a query's probes; part [nq][nslab][k] sorted keys float_bits(dist) << 32 | local row (all ones = none)
void launch_ivf_probe(const void* x, int dtype, int64_t rs, int64_t cs, int64_t nq, const float* G, int32_t nlist, int32_t d,
                      int32_t nprobe, int32_t* out, hipStream_t stream);
// entries outside [0, nlist) and repeats of an earlier entry -> -1 (norm is a buffer of its own), then the prefix
void launch_ivf_prefix(const int32_t* in, int64_t nq, int32_t nlist, int32_t nprobe, const int32_t* list_off, int32_t* norm,
                       int32_t* pref, hipStream_t stream);
void launch_ivf_check(const uint8_t* ids, int32_t nlist, int64_t m, uint32_t* flag, hipStream_t stream);
// code bytes [m][stride] of the rows row0 .. row0 + m -> the slots slot[r] = pblock * 64 + lane
void launch_ivf_scatter(const uint8_t* src, int64_t stride, int32_t M, const int64_t* slot, int64_t row0, int64_t m, uint32_t* codes,
                        uint32_t* rowid, hipStream_t stream);
// grid (nslab, nq): nq <= 65535; a slab is 64 virtual blocks of a query; slabs beyond a query's own count write nothing; a slot
// is admitted when it lies below its list's fill list_rows[l] and the allow bitmap, if any, has its row's bit
void launch_ivf_scan_select(const uint32_t* codes, const uint32_t* rowid, const uint32_t* blk_table, const int32_t* list_off, int32_t M,
                            int32_t Ks, const float* tab, const int32_t* probes, const int32_t* pref, int32_t nprobe, int32_t nq,
                            const uint32_t* list_rows, const uint64_t* allow, int32_t k, int32_t nslab, uint64_t* part, hipStream_t stream);
void launch_ivf_merge(const uint64_t* part, const int32_t* pref, int32_t nprobe, int64_t nq, int32_t k, int32_t nslab, int64_t row_offset,
                      int64_t* out_idx, float* out_dist, hipStream_t stream);

// ivfpq_residual.hip -- residual codes on the same layout (api_ivfpq.hip): a code quantizes double(x) - double(G[list]), a query has
// one table per probe slot.  probes: the NORMALISED probes of launch_ivf_prefix; tab [nq][nprobe][M][Ks] f32, the tables of -1 slots
// are neither written nor read.  Prefix and merge are ivfpq.hip's
void launch_ivfr_table(const void* x, int dtype, int64_t rs, int64_t cs, int32_t nq, const float* G, int32_t d, const float* cb, int32_t M,
                       int32_t Ks, int32_t L, const int32_t* probes, int32_t nprobe, float* tab, hipStream_t stream);
// the grid, the slabs and the partial lists of launch_ivf_scan_select
void launch_ivfr_scan_select(const uint32_t* codes, const uint32_t* rowid, const uint32_t* blk_table, const int32_t* list_off, int32_t M,
                             int32_t Ks, const float* tab, const int32_t* probes, const int32_t* pref, int32_t nprobe, int32_t nq,
                             const uint32_t* list_rows, const uint64_t* allow, int32_t k, int32_t nslab, uint64_t* part, hipStream_t stream);
// lists [n] bytes (device), every one < nlist; packed code bytes out [n][M]
void launch_ivfr_encode(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const float* G, int32_t d, const uint8_t* lists,
                        const float* cb, int32_t M, int32_t Ks, int32_t L, uint8_t* out, hipStream_t stream);
// out [n][d] packed f32 = float(double(x) - double(G[list]))
void launch_ivfr_rows(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const float* G, int32_t d, const uint8_t* lists, float* out,
                      hipStream_t stream);

// ivfflat.hip -- inverted file over the stored f32 rows of a gallery (api_ivfflat.hip).  The value of a (query, row)
// pair and the order are launch_refine's; a list is a run of local rows, ascending, in list_rows [n] behind list_off int64 [nlist + 1]
constexpr int IVFFLAT_SLAB_ROWS = 2048;                                     // positions of a query's candidate sequence per scan workgroup
constexpr int IVFF_MAX_LISTS = 8192, IVFF_MAX_BLOCKS = 1024;
// rows per workgroup of the list build: 2048 at the least, a multiple of 256, at most IVFF_MAX_BLOCKS workgroups
static inline int64_t ivff_block_rows(int64_t n) {
  const int64_t r = ((n + IVFF_MAX_BLOCKS - 1) / IVFF_MAX_BLOCKS + 255) / 256 * 256;
  return r < 2048 ? 2048 : r;
}
void launch_ivff_take_ids(const int64_t* best, int64_t m, int32_t* out, hipStream_t stream);
void launch_ivff_check(const int32_t* ids, int32_t nlist, int64_t m, uint32_t* flag, hipStream_t stream);
// ids [n] int32, every one in [0, nlist) -> list_off, list_rows.  Scratch: hist [nlist][ceil(n / ivff_block_rows(n))], sizes [nlist]
void launch_ivff_lists(const int32_t* ids, int64_t n, int32_t nlist, uint32_t* hist, uint32_t* sizes, int64_t* list_off, int32_t* list_rows,
                       hipStream_t stream);
// mi_ivfflat_sync: the lists of n_old rows and the lists of the m rows behind them (tail_rows numbered from 0) -> the lists of
// n_old + m rows, new_off [nlist + 1] and new_rows [n_old + m], neither of them an input
void launch_ivff_splice(const int64_t* old_off, const int32_t* old_rows, const int64_t* tail_off, const int32_t* tail_rows, int32_t nlist,
                        int64_t n_old, int64_t m, int64_t* new_off, int32_t* new_rows, hipStream_t stream);
// mi_ivfflat_remove_rows: keep [ceil(n / 64)] the rows that stay (bits at or beyond n clear, at least one set), rank [ceil(n / 64) + 1]
// the exclusive count of its bits per word -> the lists of the survivors in their new numbering, new_off [nlist + 1] and new_rows
// [n'], neither of them an input.  Scratch: tpre [ceil(n / 256)], bcnt [ceil(n / ivff_block_rows(n))], total [1]
void launch_ivff_compact(const int64_t* old_off, const int32_t* old_rows, int64_t n, int32_t nlist, const uint64_t* keep,
                         const uint32_t* rank, uint32_t* tpre, uint32_t* bcnt, uint32_t* total, int64_t* new_off, int32_t* new_rows,
                         hipStream_t stream);
// probes [nq][nprobe], int64 (in_is_i64) or int32: entries outside [0, nlist) and repeats of an earlier entry -> -1 in norm, then
// the prefix of list sizes pref [nq][nprobe + 1]
void launch_ivff_prefix(const void* in, int in_is_i64, int64_t nq, int32_t nlist, int32_t nprobe, const int64_t* list_off, int32_t* norm,
                        int32_t* pref, hipStream_t stream);
// grid (nslab, nq): nq <= 65535, 1 <= k <= IVFFLAT_SLAB_ROWS; nslab * IVFFLAT_SLAB_ROWS covers every query's candidates; probes: the
// normalised ones.  part_key / part_id [nq][nslab][k], pcnt [nq][nslab]; any of the four outputs may be NULL
void launch_ivff_search(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int l2, const int64_t* list_off,
                        const int32_t* list_rows, const int32_t* probes, const int32_t* pref, int32_t nprobe, const uint64_t* allow,
                        int32_t k, int32_t nslab, int32_t nq, uint64_t* part_key, int64_t* part_id, uint32_t* pcnt, int64_t row_offset,
                        int64_t* out_idx, float* out_val, double* out_val64, int64_t* out_scanned, hipStream_t stream);

// minkowski.hip -- exact Minkowski top-K over the stored f32 rows of a gallery (api_minkowski.hip).  The term of a
// column with t = |q - g| in float64: t, max, t^2 (the bits of l2_direct_wave), sqrt(t), pow(t, p)
constexpr int MINK_OP_L1 = 0, MINK_OP_LINF = 1, MINK_OP_SQ = 2, MINK_OP_SQRT = 3, MINK_OP_POW = 4;
constexpr int MINK_MAX_K = 2048;
constexpr int64_t MINK_SLAB_ROWS = 2048, MINK_MAX_PARTS = 64;
constexpr int64_t MINK_SCAN_BLOCK_ROWS = 256;                     // rows per workgroup of the scan
// queries of a scan tile: as many of 8, 4, 2, 1 as fit into 160 KiB of LDS as float64 rows of round_up(d, 4); 0 = not even one
static inline int mink_query_tile(int32_t d) {
  const int64_t row = ((int64_t)d + 3) / 4 * 4 * 8;
  for (int qt = 8; qt >= 1; qt >>= 1)
    if (qt * row <= 160 * 1024) return qt;
  return 0;
}
// rows per select workgroup: whole slabs of 2048, at most MINK_MAX_PARTS partial lists a query
static inline int64_t mink_part_rows(int64_t n) {
  const int64_t r = ((n + MINK_MAX_PARTS - 1) / MINK_MAX_PARTS + MINK_SLAB_ROWS - 1) / MINK_SLAB_ROWS * MINK_SLAB_ROWS;
  return r < MINK_SLAB_ROWS ? MINK_SLAB_ROWS : r;
}
static inline int32_t mink_parts(int64_t n) {
  const int64_t p = (n + mink_part_rows(n) - 1) / mink_part_rows(n);
  return (int32_t)(p < 1 ? 1 : p);
}
// qry [nq][dp] with 16-byte aligned rows, nq <= 65535, 1 <= k <= MINK_MAX_K, mink_query_tile(d) >= 1; allow NULL or the bitmap over
// local rows.  Scratch: val [nq][ld] (ld >= n), part_key / part_id [nq][mink_parts(n)][k].  Any of the three outputs may be NULL
void launch_minkowski(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int64_t row_offset, int op, double p,
                      const uint64_t* allow, int32_t k, int32_t nq, double* val, int64_t ld, uint64_t* part_key, int64_t* part_id,
                      int64_t* out_idx, float* out_val, double* out_val64, hipStream_t stream);
// the scan alone: val [query][row] of the rows the bitmap admits (the others keep what they held); n < 1 launches nothing
void launch_minkowski_scan(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int op, double p, const uint64_t* allow,
                           int32_t nq, double* val, int64_t ld, hipStream_t stream);

// minkowski_range.hip -- what follows the scan in a Minkowski radius search or self-join (api_minkowski_range.hip): the
// hits value <= radius of one chunk of queries counted per (query, part of the rows) and placed by prefix sums as
// (f64_key_nan_highest(value), row) entries of a CsrList, which csr_order.hip orders and writes out.  A part is mink_part_rows(nrows)
// rows, a query has mink_parts(nrows).  total: the call's lims[all queries]
struct MinkRangeArgs : CsrList {
  const double* val = nullptr;       // [nq][ld]: column r is the value of local row row_base + r
  int64_t ld = 0, nrows = 0;         // nrows: the rows that were scanned
  int64_t row_base = 0;
  const uint64_t* allow = nullptr;   // NULL or the bitmap over local rows
  double radius = 0.0;
  int64_t self_row0 = -1;            // >= 0: the self-join, query q is stored row self_row0 + q and only the rows above it count
  uint32_t* cnt = nullptr;           // [nq][parts] hits
  int64_t* off = nullptr;            // [nq][parts] their first place among the chunk's hits
};
// counts, then off and (write_lims) lims[1 ..] on top of lims[0], which `first` sets to 0
void launch_mink_range_count(const MinkRangeArgs& a, bool first, bool write_lims, hipStream_t stream);
void launch_mink_range_emit(const MinkRangeArgs& a, hipStream_t stream);                 // -> key[0] / row[0], ascending rows per query

// pq_remove.hip -- in-place row removal of the PQ and the IVF-PQ index (api_pq.hip, api_ivfpq.hip).  keep [ceil(n / 64)]: the bitmap
// of the rows that stay (bits at or beyond n clear); prefix [ceil(n / 64) + 1]: the exclusive count of keep bits per word.
// Flat index, one chunk of source blocks [blk0, blk1): its survivors -> the staging area, whose block 0 stands for block dst_blk0
// of the index (the block of the chunk's first survivor); then the staging positions [lo, hi) -> the index
void launch_pq_remove_gather(const uint32_t* codes, int32_t M, const uint64_t* keep, const uint32_t* prefix, int64_t blk0, int64_t blk1,
                             int64_t dst_blk0, uint32_t* stg, hipStream_t stream);
void launch_pq_remove_writeback(const uint32_t* stg, int32_t M, int64_t dst_blk0, int64_t lo, int64_t hi, uint32_t* codes,
                                hipStream_t stream);
// IVF index: every chain compacted in place by one workgroup (blk_table, list_off, list_rows: the tables BEFORE the removal),
// row ids rewritten to the new numbering
void launch_ivf_remove(uint32_t* codes, uint32_t* rowid, const uint32_t* blk_table, const int32_t* list_off, const uint32_t* list_rows,
                       int32_t nlist, int32_t M, const uint64_t* keep, const uint32_t* prefix, hipStream_t stream);

// synth.hip
void launch_synth_fill(float* dst, uint64_t seed, int64_t row0, int64_t nrows, int32_t d, hipStream_t stream);

}  // namespace mi
