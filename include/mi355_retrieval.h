/*
 * mi355_retrieval.h -- C ABI of libmi355_retrieval.so, the MI355X (gfx950) retrieval hot path.
 *
 * Plain pointers and sizes only (no torch / numpy types).  Each entry point names the reference
 * interface it replaces (paths relative to the reference tree).  The reference has no FFI: its
 * "plugin surface" is the --matching_method if/elif chain calling free functions of
 * src/utils/nnsearch.py (src/offline.py:107-118, src/online.py:132-143), so the binding a
 * maintainer adds is the ctypes stub shown in INTEGRATION.md.
 *
 * Conventions
 *   - status codes (MI_OK == 0); mi_last_error() returns the message of the calling thread's last
 *     failure.  Nothing throws across the boundary.
 *   - a gallery handle is ONE row shard on ONE device (one process per GPU; row_offset globalises
 *     the indices it returns).  Inputs are never modified; outputs are caller-owned.
 *   - "host" entry points are synchronous and take strided f32/f64 host arrays (callers of the
 *     reference pass `.T` views of [D,N] arrays, so strides are part of the contract).
 *   - "_device" entry points take device pointers, enqueue on `stream` (a hipStream_t) and return
 *     without synchronising; sticky error flags are read with mi_search_status().
 *   - a handle is not re-entrant: serialise calls on one handle (online.py's Flask threads must
 *     hold a lock; the Python wrapper does).
 */
#ifndef MI355_RETRIEVAL_H
#define MI355_RETRIEVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_gallery mi_gallery; /* opaque */

enum mi_status {
  MI_OK = 0,
  MI_ERR_INVALID = 1,     /* bad argument (K > N like the reference's broadcast error, null ptr, ...) */
  MI_ERR_HIP = 2,         /* HIP runtime failure; message carries hipGetErrorString */
  MI_ERR_NOMEM = 3,
  MI_ERR_IO = 4,
  MI_ERR_OVERFLOW = 5,    /* candidate buffers overflowed and the exact fallback was disabled */
  MI_ERR_UNSUPPORTED = 6,
  MI_ERR_CAPACITY = 7     /* mi_range_search, mi_hamming_range_search, mi_hamming_self_range, mi_range_search_minkowski,
                             mi_range_search_minkowski_device (which reports it through out_lims_dev[nq] only),
                             mi_minkowski_self_range: more results than max_results; out_lims[nq] says how many */
};
enum mi_dtype { MI_F32 = 0, MI_F64 = 1 };
enum mi_memspace { MI_HOST = 0, MI_DEVICE = 1 };
enum mi_norm {
  MI_NORM_NONE = 0,  /* rows used as given: inner-product ranker, src/main_retrieve.py:175-176; faiss
                        IndexFlatIP, src/utils/knn.py:33-40; QGE re-score, src/utils/Reranking.py:206 */
  MI_NORM_L2 = 1,    /* x / ||x||, no eps: matching_L2, src/utils/nnsearch.py:693-698 */
  MI_NORM_L2_EPS = 2 /* x / (||x|| + 1e-6): l2n, src/layers/functional.py:129-130; whitenapply tail,
                        src/utils/whiten.py:10 */
};

enum mi_metric {
  MI_METRIC_IP = 0,  /* inner product, descending (every gallery but those of mi_gallery_create_l2) */
  MI_METRIC_L2 = 1   /* squared Euclidean distance, ascending: faiss IndexFlatL2, KNN(..., 'euclidean'), src/utils/knn.py:33-40 */
};

const char* mi_last_error(void);
int mi_device_count(int* count);

/* ---- gallery ingest: replaces the per-call normalisation of matching_L2
 * (src/utils/nnsearch.py:693-698) and faiss index.add (src/utils/knn.py:17-23).
 * data: element (i,j) at data[i*row_stride + j*col_stride] (strides in elements), n rows, d cols.
 * Builds, resident in HBM: normalised f32 rows [n][d64], the tile-blocked bf16 copy the MFMA
 * kernel streams, and per-row rounding-error norms used for the exactness certificate.
 * Synchronous.  MI_DEVICE data is read on a stream of the handle's own (non-blocking, NOT ordered against any stream of the
 * caller): whatever produced `data` must have completed -- synchronise the producing stream first -- and the pointer may be
 * freed as soon as the call returns.  mi_gallery_append_device is the stream-ordered way in.
 * MI_F64 data is read as float64 and leaves the ingest as float32: under MI_NORM_NONE every element is rounded to f32 as it
 * stands, under the normalising modes it is scaled in float64 by the row's float64 norm and rounded once.  The same holds for
 * mi_gallery_append and for the queries of every search on a gallery (mi_knn_search, mi_range_search, mi_knn_search_filtered,
 * mi_knn_dense_search, mi_knn_dense64_search, mi_rank_*, mi_diffusion_online): float64 holding float32 values gives the float32
 * answer bit for bit, whatever the strides (tests/test_gpu_input_layouts.py). */
int mi_gallery_create(const void* data, int64_t n, int32_t d, int dtype, int64_t row_stride,
                      int64_t col_stride, int memspace, int norm_mode, int device,
                      int64_t row_offset, mi_gallery** out);
/* Appendable gallery (offline pipeline): capacity rows are allocated, rows arrive from the device
 * (descriptors straight out of the extractor tail) and are normalised / imaged / measured in place.  Appends and
 * searches on one handle must be serialised by the caller; `stream` orders the append against the producer. */
int mi_gallery_create_empty(int64_t capacity, int32_t d, int norm_mode, int device, int64_t row_offset,
                            mi_gallery** out);
int mi_gallery_append_device(mi_gallery* g, const float* rows_dev /*[m][d] f32*/, int64_t m, void* stream);
/* Strided append of m rows (f32 | f64, host or device memory; synchronous, device rows must be complete as for create).  A host column block of a [D, N] array --
 * row_stride 1, col_stride N, the layout of the reference's feature pickles and of its 1M-distractor tensor
 * (src/utils/general.py:67-92, src/extract_1m.py:97-98, src/test_rOP1m.py:136-139) -- is packed by one 2-D copy and read
 * with strides on the device: no host transpose, no concatenated host copy, no float64 promotion. */
int mi_gallery_append(mi_gallery* g, const void* data, int64_t m, int dtype, int64_t row_stride, int64_t col_stride,
                      int memspace);
/* Removes rows in place (faiss IndexFlat.remove_ids).  remove_bits has the layout of allow_bits in mi_knn_search_filtered:
 * ceil(n / 64) words, bit (i & 63) of word (i >> 6) names LOCAL row i, bits at or beyond n are ignored; memspace is MI_HOST or
 * MI_DEVICE (a device bitmap must be complete when the call is made).  The surviving rows keep their relative order and are
 * renumbered 0 .. n' - 1: new row j is the j-th surviving old row.  row_offset and the capacity do not change; *out_removed (may
 * be NULL) receives n - n'.  Afterwards every section of the prepared gallery -- stored f32 rows, 16-bit image, rounding norms,
 * their padding rows up to the old padded size, the norm maxima, n -- holds, bit for bit, what the same ingest path would have
 * written for the surviving source rows alone AT THE SAME IMAGE TYPE: removing the one large row of a raw bf16 gallery does not
 * turn it into fp16 (mi_gallery_set_image_dtype is the caller's tool for that).  A bitmap with no bit set below n leaves the
 * gallery untouched; one that names every row leaves an empty appendable gallery of the same capacity and image type.  Works
 * on galleries of either metric and every norm mode.  Synchronous on the handle's stream; like mi_range_search it completes a
 * pending deferred tail first (its ids are in the old numbering).  Dropped with the old numbering: the cached sub-gallery of
 * the filtered search, the threshold samples, and the offline diffusion matrix (mi_diffusion_online then answers as on a handle
 * that never had one).  MI_ERR_INVALID while an online handle is built on the gallery (mi_online_destroy comes first), as for
 * mi_gallery_destroy.  Device memory beyond the gallery is bounded independently of n: a staging area of at most B rows in the gallery's
 * layout (B * (6 * d64 + 12) bytes; global option "remove_block_rows", an upper limit), 4 bytes per surviving row and the bitmap, kept on the
 * handle for the next call.  Shards of a sharded gallery are out of scope: the maxima the shards agreed on
 * (mi_gallery_norm_bounds) are replaced by the shard's own.  DESIGN.md 5.12. */
int mi_gallery_remove_rows(mi_gallery* g, const uint64_t* remove_bits, int memspace, int64_t* out_removed);
int mi_gallery_destroy(mi_gallery* g);
int mi_gallery_info(const mi_gallery* g, int64_t* n, int32_t* d, int32_t* norm_mode, int32_t* device,
                    int64_t* row_offset, int64_t* hbm_bytes);
/* Prepared-gallery persistence: the counterpart of the ANN methods' `outputs/<dataset>/` index files
 * guarded by `ifgenerate` (src/utils/nnsearch.py:503-525, 1033-1044). */
int mi_gallery_save(const mi_gallery* g, const char* path);
int mi_gallery_load(const char* path, int device, mi_gallery** out);
/* Copies normalised f32 rows [row0,row0+nrows) x d to a host buffer (tests / diffusion host logic). */
int mi_gallery_get_rows(const mi_gallery* g, int64_t row0, int64_t nrows, float* out_host);

/* ---- exhaustive kNN: replaces matching_L2(K, train, test) -> (idx, time_per_query)
 * (src/utils/nnsearch.py:687-706) and KNN.search (src/utils/knn.py:25-31).
 * q: nq x d strided host array.  out_idx [nq][k] int64 (row_offset + local row), out_score [nq][k]
 * f32 (may be NULL): exact inner product of the stored rows with the (normalised) query, descending,
 * ties to the lower index.  out_seconds (may be NULL): device-synchronised wall time of the call
 * including query upload/normalisation, excluding nothing. */
int mi_knn_search(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride,
                  int64_t col_stride, int32_t k, int64_t* out_idx, float* out_score,
                  double* out_seconds);

/* Exact range search: for every query, all rows whose exact score (the same float64 score mi_knn_search returns:
 * f32 stored rows, exact f64 products, f64 accumulation, query normalised by the gallery's norm mode) is >= min_score.
 * Results in CSR form: the hits of query i are out_idx/out_score[out_lims[i] .. out_lims[i+1]), ordered by
 * (score desc, id asc); ids are row_offset + local row.  out_lims [nq + 1] is always written in full.  If
 * out_lims[nq] > max_results, nothing is written to out_idx / out_score and MI_ERR_CAPACITY is returned:
 * call again with max_results >= out_lims[nq].  out_score may be NULL; out_idx may be NULL when max_results is 0.
 * out_seconds (may be NULL): wall time of the call.  Host input and host output, like mi_knn_search. */
int mi_range_search(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride,
                    double min_score, int64_t max_results, int64_t* out_lims, int64_t* out_idx, float* out_score,
                    double* out_seconds);

/* Exact filtered top-K: mi_knn_search over the rows an allow bitmap admits.  allow_bits holds ceil(n / 64) words; bit
 * (i & 63) of word (i >> 6) allows local row i of this shard, bits at or beyond n are ignored; allow_memspace is MI_HOST or
 * MI_DEVICE (a device bitmap must be complete when the call is made).  One bitmap applies to every query of the call.
 * The answer is exactly mi_knn_search's over the allowed rows: ids row_offset + local row, order (score desc, id asc), and each
 * row's f32 score bit-identical to the one mi_knn_search gives that row; with every row allowed it equals mi_knn_search bit for
 * bit.  If fewer than k rows are allowed, the trailing entries are id -1 and score -INFINITY.  1 <= k <= 2048.  Queries, strides
 * and dtype as in mi_knn_search (host input, host output).  out_score, out_info and out_seconds may be NULL.
 * Two exact paths, chosen per call from the selectivity s = allowed / n (options "filter_path",
 * "filter_compact_max"): 1 = the allowed rows are copied into a sub-gallery owned by the handle and searched (kept for the next
 * call with an equal bitmap while option "filter_cache" is 1; dropped by mi_gallery_append*, mi_gallery_set_image_dtype, mi_gallery_remove_rows);
 * 2 = the unfiltered search at depth K' = min(2048, ceil(1.25 k / s) + 32), keeping the first k allowed entries; a query that
 * found fewer while K' did not cover the shard is answered by path 1 instead.  Like mi_range_search, the call completes a
 * pending deferred tail first and leaves the sticky flags (mi_search_flags) as it found them. */
typedef struct mi_filter_info {
  int64_t allowed;        /* rows of this shard the bitmap allows */
  int32_t path;           /* 0 = no allowed row (nothing searched), 1 = compacted sub-gallery, 2 = over-fetch */
  int32_t kprime;         /* over-fetch depth used (0 on path 1) */
  int64_t rerun_queries;  /* queries the over-fetch could not certify; they were answered by path 1 */
  int32_t cache_hit;      /* path 1 reused the sub-gallery built by an earlier call */
} mi_filter_info;

int mi_knn_search_filtered(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride,
                           int32_t k, const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_score,
                           mi_filter_info* out_info, double* out_seconds);

/* ---- exact grouped top-K (collapse / group-by search): the best row of every group, k groups per query, one excluded group per
 * query.  The selection loop of the reference's hard-negative mining (create_epoch_tuples, src/datasets/traindataset.py:219-243,
 * 466-490: full sort of every column, skip the query's own cluster, at most one image per cluster).  DESIGN.md 5.10b.
 * mi_gallery_set_groups: one int32 label per LOCAL row, n == the gallery's n (else MI_ERR_INVALID); memspace MI_HOST or MI_DEVICE
 * (device labels are copied to the host first and must be complete).  Labels >= 0 are arbitrary, need not be dense; -1 makes the
 * row a group of its own; any other negative label is MI_ERR_INVALID.  labels == NULL clears the groups.  The handle keeps the
 * labels and a dense relabelling (built on the host, uploaded).  Whatever changes n or the rows -- mi_gallery_append*,
 * mi_gallery_remove_rows -- DROPS the labels: the grouped search then refuses (MI_ERR_INVALID, "not in step") until labels are
 * set again, like an index on a changed gallery.  mi_gallery_save does not write them.
 * mi_gallery_get_groups: the labels as given, [n] int32 to the host.  mi_gallery_group_count: the number of groups G, every -1 row
 * counting once.  Both are MI_ERR_INVALID without labels. */
int mi_gallery_set_groups(mi_gallery* g, const int32_t* labels, int64_t n, int memspace);
int mi_gallery_get_groups(mi_gallery* g, int32_t* out_host);
int mi_gallery_group_count(mi_gallery* g, int64_t* out);
/* mi_knn_search_grouped: take mi_knn_search's complete ranking of every stored row for a query, (score desc, id asc), walk it from
 * the top, keep a row if its group has not been kept yet and its label is not exclude_labels[query] (host array [nq] or NULL; -1
 * or a label no row carries excludes nothing), stop at k kept rows.  So the row kept for a group is the group's best row (the
 * lowest id among equal scores) and the groups come in the order of (their best row's score desc, that row's id asc).
 * out_idx [nq][k] = row_offset + local row; out_score [nq][k] (may be NULL) the f32 mi_knn_search returns for that row, bit for
 * bit; out_label [nq][k] (may be NULL) the caller's label, -1 for a singleton row.  Fewer than k eligible groups: trailing ids -1,
 * scores -INFINITY, labels -1.  1 <= k <= 2048.  With every row labelled -1 and no exclusion the output is mi_knn_search's.
 * Host input and host output, queries as in mi_knn_search (q_dtype is its dtype, MI_F32 or MI_F64: float64 is rounded to float32 as
 * every query batch is; every layout is swept by tests/test_gpu_input_layouts_grouped.py); out_info and out_seconds may be NULL.  Like mi_knn_search_filtered the
 * call completes a pending deferred tail first and leaves the sticky flags as it found them.  MI_ERR_UNSUPPORTED on an L2
 * gallery; MI_ERR_INVALID on a gallery without labels in step with its rows.
 * Two exact paths (option "group_path" 0 = auto, 1 = always the fallback, 2 = always the over-fetch; both give the same ids,
 * score bits and labels): 2 = the unfiltered search at depth K' = min(2048, n, f k + 32) (global option "group_overfetch", f = 4)
 * collapsed on the device; a query is certified when it kept k rows or K' covered the shard.  1 = what the over-fetch cannot
 * certify (a query whose own item has more than K' rows at the top): dense float64 scores of sub-batches of queries (global
 * option "group_dense_bytes", default 1 GiB, one query at the least), every group reduced to its best row over the group CSR,
 * the G entries of a query ordered, the first k written.
 * Out of scope: more than one row per group; an allow bitmap combined with groups; L2 and Minkowski galleries; the binary and PQ
 * index families; merging grouped answers across shards (a per-shard call honours row_offset, but a merge across shards must
 * collapse again); saving the labels with the gallery. */
typedef struct mi_group_info {
  int64_t groups;          /* G of the gallery */
  int32_t path;            /* 1 = dense fallback for every query, 2 = over-fetch */
  int32_t kprime;          /* over-fetch depth used (0 on path 1) */
  int64_t rerun_queries;   /* queries the over-fetch could not certify; they were answered by the fallback */
  int64_t excluded_found;  /* queries whose exclude label names a group of the gallery */
} mi_group_info;
int mi_knn_search_grouped(mi_gallery* g, const void* q, int64_t nq, int q_dtype, int64_t row_stride, int64_t col_stride,
                          int32_t k, const int32_t* exclude_labels, int64_t* out_idx, float* out_score, int32_t* out_label,
                          mi_group_info* out_info, double* out_seconds);

/* ---- exact squared-L2 (Euclidean) top-K on raw descriptors: faiss IndexFlatL2 behind KNN(database, 'euclidean')
 * (src/utils/knn.py:33-40), the metric string every reference entry point passes (src/offline.py:112, src/online.py:137,
 * src/test_rOP1m.py:156).  On rows that are not unit length its order differs from the inner product's.  DESIGN.md 5.11.
 * An L2 gallery (mi_get_option "metric" == MI_METRIC_L2, read-only) stores the rows as given, like MI_NORM_NONE, plus three hidden
 * columns that never leave the library: mi_gallery_info and mi_gallery_get_rows report the caller's d.  capacity 0 means n; with
 * capacity > n the gallery is appendable, and data == NULL with n == 0 gives an empty appendable one (appendable L2 galleries use
 * the bf16 image).  On an L2 gallery mi_gallery_append*, mi_gallery_info, mi_gallery_get_rows, mi_gallery_destroy,
 * mi_gallery_calibrate, mi_gallery_scatter, the options, statistics, flags and diagnostics work on the caller's d; every other
 * entry point that takes a gallery returns MI_ERR_UNSUPPORTED (radius search, alpha-QE, diffusion, the online front and
 * sharded search are not defined for this metric); mi_gallery_save / mi_gallery_load keep the metric (header word `metric`).  The _l2 entry points return MI_ERR_INVALID on any other gallery.  The order
 * among non-finite distances (non-finite inputs) is unspecified. */
int mi_gallery_create_l2(const void* data, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride,
                         int memspace, int device, int64_t row_offset, int64_t capacity, mi_gallery** out);
/* Host input, host output, the verified loop of mi_knn_search.  Queries are taken as given (f64 queries are rounded to f32 like
 * every query batch).  out_idx [nq][k] int64 (row_offset + local row), out_dist64 [nq][k] (may be NULL): sum_j (q_j - g_j)^2 in
 * the DIRECT form over the stored f32 row, f32 values promoted to float64, float64 accumulation -- a query equal to a stored row
 * is at distance 0.0 exactly --, ascending, ties to the lower id; out_dist [nq][k] f32 (may be NULL) = (float)out_dist64.  Fewer
 * than k rows (allowed): trailing ids -1, distances +INFINITY.  1 <= k <= 2048.  allow_bits NULL: every row; otherwise the
 * bitmap of mi_knn_search_filtered with its two paths, its options and out_info (may be NULL; without a bitmap only `allowed`
 * = n is filled in). */
int mi_knn_search_l2(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                     const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_dist, double* out_dist64,
                     mi_filter_info* out_info, double* out_seconds);
/* Device-resident variant, enqueued on `stream` like mi_knn_search_device (q_dev [nq][d] row-major f32; out_dist_dev and
 * out_dist64_dev may be NULL): no verified loop, a raised sticky flag (mi_search_flags) means the batch must be answered again.
 * The call stages its extended queries and the selected rows in buffers of the handle (grown, i.e. freed and allocated again,
 * when a larger batch comes): calls on one handle must be serialised by the caller and enqueued on ONE stream. */
int mi_knn_search_l2_device(mi_gallery* g, const float* q_dev, int64_t nq, int32_t k, int64_t* out_idx_dev,
                            float* out_dist_dev, double* out_dist64_dev, void* stream);
/* The L2 twin of mi_knn_dense64_search, the independent checker: EVERY direct-form float64 distance of the gallery, no threshold
 * logic at all, then the exact top-k by (distance asc, id asc), k <= 4096; padding as above. */
int mi_knn_dense64_search_l2(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride,
                             int32_t k, int64_t* out_idx, float* out_dist, double* out_dist64, double* out_seconds);

/* ---- exact re-ranking of an index's shortlist on the raw rows: faiss IndexRefineFlat, and the last step of the reference's
 * matching_ANNOY (exact distances over a candidate union).  DESIGN.md 5.15.  `rows` is the gallery that holds the raw rows, ONE
 * shard on one device; the candidates are what a PQ, IVF-PQ, binary or LSH index returned for the same rows: per query kc ids,
 * int64, global (row_offset + local row of `rows`), in any order, repeats allowed.  An id that is negative or outside
 * [row_offset, row_offset + n) is padding.  The answer per query is the best k DISTINCT candidates:
 *   L2 gallery (mi_gallery_create_l2): sum_j (q_j - g_j)^2 in the direct form over the caller's d columns -- the arithmetic and
 *     the bits of mi_knn_search_l2 --, ascending;
 *   any other gallery: sum_j q_j g_j against the STORED f32 row (the normalised row under MI_NORM_L2), f32 promoted to float64,
 *     float64 FMA accumulation, descending.  The query is used as given: normalise it yourself if the value matters; its scale
 *     does not change the order.
 * Order (value, id ascending); a repeated id counts once; fewer than k distinct candidates: trailing ids -1, values +INFINITY
 * (L2) or -INFINITY.  out_val (f32, may be NULL) = (float)out_val64 (may be NULL).  1 <= kc <= 8192, 1 <= k <= kc,
 * cand_stride >= kc (elements between the candidate rows of consecutive queries); nq == 0 is MI_OK and writes nothing.
 * mi_refine_device: q_dev [nq][d] packed f32; enqueued on `stream`, no synchronisation.  It stages the queries and the values of
 * the candidates in buffers of the handle (grown when a larger call comes): calls on one handle must be serialised by the caller
 * and enqueued on ONE stream.  Not built: refine over a sharded gallery, and an allow bitmap (the index that produced the
 * shortlist has applied its own). */
int mi_refine_device(mi_gallery* rows, const float* q_dev, int64_t nq, const int64_t* cand_dev, int32_t kc, int64_t cand_stride,
                     int32_t k, int64_t* out_idx_dev, float* out_val_dev, double* out_val64_dev, void* stream);
/* Host form: queries of any strides and dtype as in mi_knn_search_l2 (f64 rounded to f32), candidates [nq][cand_stride] in host
 * memory; synchronous. */
int mi_refine(mi_gallery* rows, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, const int64_t* cand,
              int32_t kc, int64_t cand_stride, int32_t k, int64_t* out_idx, float* out_val, double* out_val64, double* out_seconds);
/* Measurement only (scripts/refine_timing.py): the one-workgroup-per-query tail of mi_knn_search_l2 fed ke <= k <= 2048 ids per
 * query, [nq][ke] packed, on an L2 gallery; enqueued on `stream`. */
int mi_debug_l2_tail_device(mi_gallery* g, const float* q_dev, int64_t nq, const int64_t* ids_dev, int32_t ke, int32_t k,
                            int64_t* out_idx_dev, double* out_dist64_dev, void* stream);

/* ---- exact Minkowski top-K on the raw rows: faiss IndexFlat with METRIC_L1, METRIC_Linf and METRIC_Lp, and the reference's
 * fractional_distance (src/utils/nnsearch.py:46-56, p = 0.5 by default) behind matching_fractional_dis (:709-731).  DESIGN.md 5.19.
 * `rows` is ONE shard on one device that holds its f32 rows, as for mi_refine; a row wider than 20480 columns is
 * MI_ERR_UNSUPPORTED.  The value of a (query, row) pair is taken on the STORED f32 row g -- the row as given on MI_NORM_NONE and
 * squared-L2 galleries, over the caller's d columns only; the normalised row under MI_NORM_L2 -- and the query rounded to f32 like
 * every query batch and used as given.  With t_j = |(double)q_j - (double)g_j|:
 *   MI_MINK_L1                sum_j t_j, float64 adds;
 *   MI_MINK_LINF              max_j t_j (exact);
 *   MI_MINK_LP, p == 1        as MI_MINK_L1, the same bits;
 *   MI_MINK_LP, p == 2        sum_j t_j^2, float64 FMA: the arithmetic and the bits of mi_knn_search_l2;
 *   MI_MINK_LP, p == 0.5      sum_j sqrt(t_j), float64 sqrt and adds;
 *   MI_MINK_LP, other p > 0   sum_j pow(t_j, p), float64 pow and adds.
 * The Lp value is faiss's: it is NOT raised to 1 / p.  The reference's fractional_distance is value ** (1 / p), a monotone map of
 * it, so the order is the same up to ties which that last rounding creates.  Every sum runs in one fixed order, that of
 * mi_knn_search_l2's direct form (lane l of 64 adds columns 4 l + 256 i + {0, 1, 2, 3} in ascending order, then an xor butterfly
 * 32, 16, ... 1 over the lanes): the bits of a pair depend on nothing but the pair.  p <= 0, NaN or infinite is MI_ERR_INVALID
 * (MI_MINK_LINF is the infinite case); p is ignored unless metric == MI_MINK_LP.
 * Order (value asc, id asc); out_idx [nq][k] int64 (row_offset + local row), out_dist64 [nq][k] (may be NULL), out_dist [nq][k]
 * f32 (may be NULL) = (float)out_dist64.  Fewer than k admitted rows: trailing ids -1, values +INFINITY.  1 <= k <= 2048.
 * allow_bits NULL: every row; otherwise the bitmap of mi_knn_search_filtered over local rows.  The order among non-finite values
 * (non-finite inputs) is unspecified.  Nothing is cached: a gallery that rows were appended to or removed from is searched as it
 * then stands.  Host form: queries of any strides, q_dtype MI_F32 or MI_F64, as in mi_knn_search_l2; takes the handle's lock; synchronous; nq == 0
 * is MI_OK and writes nothing. */
#define MI_MINK_L1 1
#define MI_MINK_LINF 2
#define MI_MINK_LP 3
int mi_knn_search_minkowski(mi_gallery* rows, const void* q, int64_t nq, int q_dtype, int64_t row_stride, int64_t col_stride,
                            int metric, double p, int32_t k, const uint64_t* allow_bits, int allow_memspace,
                            int64_t* out_idx, float* out_dist, double* out_dist64, double* out_seconds);
/* Device form: q_dev [nq][d] packed f32, allow_bits_dev NULL or the bitmap in device memory; enqueued on `stream`, no
 * synchronisation.  It stages the queries, the float64 value of every (query, row) pair of a chunk of queries and partial lists in
 * buffers of the handle (grown when a larger call comes): calls on one handle must be serialised by the caller and enqueued on ONE
 * stream, as for mi_knn_search_l2_device. */
int mi_knn_search_minkowski_device(mi_gallery* rows, const float* q_dev, int64_t nq, int metric, double p, int32_t k,
                                   const uint64_t* allow_bits_dev, int64_t* out_idx_dev, float* out_dist_dev,
                                   double* out_dist64_dev, void* stream);

/* Exact radius search in the same metrics (faiss IndexFlat::range_search with METRIC_L1 / METRIC_Linf / METRIC_Lp / METRIC_L2):
 * every row the bitmap admits whose value is <= radius.  DESIGN.md 5.19b.  The value of a (query, row) pair is
 * mi_knn_search_minkowski's for that pair, bit for bit -- the same kernel computes it -- so it depends on nothing but the pair;
 * metric, p, the gallery and the query are taken exactly as there (an L2 gallery: the caller's d columns; MI_MINK_LP with p == 2
 * gives the bits of mi_knn_search_l2).  The comparison is made in float64 and is INCLUSIVE, like mi_hamming_range_search's; a NaN
 * value is never a hit.  For MI_MINK_LP the radius applies to the value as defined above, sum_j t_j^p (faiss's), NOT to its 1 / p-th
 * power: a Euclidean radius r is passed as r * r.  radius NaN or negative: MI_ERR_INVALID; +inf returns every admitted row whose
 * value is not NaN.
 * Results in CSR form: the hits of query i are out_idx / out_dist / out_dist64[out_lims[i] .. out_lims[i+1]), ordered by
 * (value asc, id asc), ids row_offset + local row; a query has anywhere from 0 to n hits; out_dist is (float)out_dist64.
 * out_lims [nq + 1] is always written in full.  If out_lims[nq] > max_results, nothing is written to out_idx / out_dist /
 * out_dist64 and MI_ERR_CAPACITY is returned: call again with max_results >= out_lims[nq].  Either distance output may be NULL;
 * out_idx may be NULL when max_results is 0.  nq == 0 is MI_OK.  Queries, bitmap and out_seconds as in mi_knn_search_minkowski.
 * Fully determined: every output position is a prefix sum over (query, part of the rows, row) in ascending order, never the order
 * in which the device ran, and the order inside a query is a total order.  The float64 values of a chunk of queries (8 bytes per
 * (query, row) pair) and its counts stay within the global option "minkowski_range_bytes" (default 256 MiB; one scan tile of
 * queries at the least), plus 24 bytes per hit of one chunk; a call of more than one chunk scans the gallery twice. */
int mi_range_search_minkowski(mi_gallery* rows, const void* q, int64_t nq, int q_dtype, int64_t row_stride, int64_t col_stride,
                              int metric, double p, double radius, const uint64_t* allow_bits, int allow_memspace,
                              int64_t max_results, int64_t* out_lims, int64_t* out_idx, float* out_dist, double* out_dist64,
                              double* out_seconds);
/* Device form: q_dev [nq][d] packed f32, allow_bits_dev NULL or the bitmap in device memory, out_lims_dev [nq + 1] and
 * out_idx_dev / out_dist_dev / out_dist64_dev [max_results] in device memory; enqueued on `stream`, no synchronisation.  The
 * capacity decision is made on the device: the call returns MI_OK, and when out_lims_dev[nq] > max_results nothing was written to
 * the three hit arrays -- the caller reads out_lims_dev[nq].  Buffers of the handle, serialisation and the ONE stream as for
 * mi_knn_search_minkowski_device. */
int mi_range_search_minkowski_device(mi_gallery* rows, const float* q_dev, int64_t nq, int metric, double p, double radius,
                                     const uint64_t* allow_bits_dev, int64_t max_results, int64_t* out_lims_dev,
                                     int64_t* out_idx_dev, float* out_dist_dev, double* out_dist64_dev, void* stream);
/* Self-join: query i is the stored row row0 + i (read on the device, never copied to the host), and only the rows j > row0 + i
 * are reported, so that a sweep over the whole gallery reports every pair once (ids are row_offset + j).  0 <= row0,
 * 0 <= nrows, row0 + nrows <= n, otherwise MI_ERR_INVALID; nrows == 0 is MI_OK.  No bitmap.  The 256-row blocks wholly below
 * row0 are not scanned.  Everything else as mi_range_search_minkowski. */
int mi_minkowski_self_range(mi_gallery* rows, int64_t row0, int64_t nrows, int metric, double p, double radius,
                            int64_t max_results, int64_t* out_lims, int64_t* out_idx, float* out_dist, double* out_dist64,
                            double* out_seconds);

/* ---- graph index: best-first search of a neighbour graph over the rows of a gallery, the role of the reference's HNSW matchers
 * (matching_HNSW and its kin, src/utils/nnsearch.py:59-538).  DESIGN.md 5.16.  What is approximate is WHICH rows the graph
 * reaches; everything else is an exact, deterministic function of graph, entry rows, stored rows and query.
 * A handle sits over ONE gallery `rows` (one shard on one device, squared-L2 or inner product, as for mi_refine), which must
 * outlive it.  It holds a neighbour table int32 [n][R] of LOCAL rows, -1 being padding anywhere in a row, and ne entry rows.
 * The VALUE of a row for a query is mi_refine's: on an L2 gallery the direct-form float64 squared distance (the bits of
 * mi_knn_search_l2), smaller is better; on any other gallery the float64 inner product against the stored row, larger is better.
 * The ORDER is (value best first, id ascending).  Per query, with 1 <= k <= ef <= 2048:
 *   start   the distinct entry rows are visited and evaluated; W is the best ef of them in the order; none is expanded;
 *   step    the first row of W (in the order) that is not yet expanded is marked expanded; of its R table entries the -1s, ids
 *           outside [0, n), repeats within the row and rows already visited are dropped, the rest are marked visited and
 *           evaluated; W becomes the best ef of W plus the new rows.  A row pushed out of W is never expanded and stays visited;
 *   stop    when every row of W is expanded (and after n expansions at the latest, whatever the table holds);
 *   answer  the first k rows of W: ids row_offset + local row (int64), values float64 (out_val64, may be NULL) with their f32
 *           cast (out_val, may be NULL); fewer than k rows in W: trailing ids -1, values +INFINITY (L2) or -INFINITY.
 *           out_visited (int32 [nq], may be NULL): the number of rows evaluated, entries included.
 * Without ties among values this is the reference's HNSW._search_graph (:321-350) on its bottom layer; with ties the order above
 * decides, not the accidents of Python's heaps.  The visited set is exact (a bitmap of n bits per query).
 * mi_graph_create takes a caller's table (a pickled HNSW bottom layer, a ring, ...): neighbors [n][R] packed int32 in host or
 * device memory, n the gallery's rows, 1 <= R <= 64; entries int32 [ne] in host memory, 1 <= ne <= 64.  An entry outside [0, n) or
 * a table value below -1 or >= n is MI_ERR_INVALID; self-loops and repeats are legal (the visited rule disposes of them).
 * mi_graph_build makes the table on the device, R even in [2, 64], 1 <= ne <= 64, n >= 2, the same bytes on every call:
 *   F(i)  the min(R, n - 1) nearest other rows of row i in the order, by the exact search of the gallery on its own stored rows
 *         with k = min(R + 1, n) (verified loop), i dropped from the answer -- or the last row where i is absent, which more than
 *         R identical rows can cause;
 *   B(i)  with h = R / 2, the rows j such that i is among the first h of F(j), ordered by (position of i in F(j), j);
 *   N(i)  F(i)[:h], then the first h rows of B(i) not yet present, then the rows of F(i)[h:] not yet present, R at most, -1 behind;
 *   entries  row floor(t * n / ne') for t = 0 .. ne' - 1, ne' = min(ne, n).
 * The handle records the gallery's n: after mi_gallery_append* or mi_gallery_remove_rows a search returns MI_ERR_INVALID and
 * reads no stale table.  Not built: updating a graph in place, HNSW's upper layers and insertion-order construction, an allow
 * bitmap, sharding. */
typedef struct mi_graph mi_graph; /* opaque */
int mi_graph_create(mi_gallery* rows, const int32_t* neighbors, int32_t R, int neighbors_memspace, const int32_t* entries,
                    int32_t ne, mi_graph** out);
int mi_graph_build(mi_gallery* rows, int32_t R, int32_t ne, mi_graph** out);
/* n, R, ne (any may be NULL); the table rows [row0, row0 + nrows) and the ne entries into host memory */
int mi_graph_info(const mi_graph* gr, int64_t* n, int32_t* R, int32_t* ne);
int mi_graph_get_neighbors(mi_graph* gr, int64_t row0, int64_t nrows, int32_t* out_host);
int mi_graph_get_entries(mi_graph* gr, int32_t* out_host);
int mi_graph_destroy(mi_graph* gr);
/* Host form: queries of any strides and dtype as in mi_knn_search_l2 (f64 rounded to f32), used as given; synchronous, on the
 * gallery's stream.  nq == 0 is MI_OK and writes nothing. */
int mi_graph_search(mi_graph* gr, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                    int32_t ef, int64_t* out_idx, float* out_val, double* out_val64, int32_t* out_visited, double* out_seconds);
/* q_dev [nq][d] packed f32; enqueued on `stream`, no synchronisation.  It stages the queries and the visited bitmaps in buffers
 * of the handle (grown when a larger call comes; a batch whose bitmaps would exceed 256 MiB runs in chunks of queries): calls on
 * one handle must be serialised by the caller and enqueued on ONE stream. */
int mi_graph_search_device(mi_graph* gr, const float* q_dev, int64_t nq, int32_t k, int32_t ef, int64_t* out_idx_dev,
                           float* out_val_dev, double* out_val64_dev, int32_t* out_visited_dev, void* stream);

/* ---- random-projection forest: T balanced trees over the rows of a gallery, the role of the reference's matching_ANNOY
 * (src/utils/nnsearch.py; its million-image driver's ANN choice, src/test_rOP1m.py:156).  DESIGN.md 5.17.  The forest is this
 * library's own -- one random direction per LEVEL of a tree, median splits --, not annoy's two-means hyperplanes, its RNG or its
 * file format.  What is approximate is WHICH rows the forest reaches; everything else is an exact, deterministic function of
 * directions, trees, stored rows and query.
 * A handle sits over ONE gallery `rows` (one shard on one device, squared-L2 or inner product, as for mi_refine and mi_graph),
 * which must outlive it.
 *   shape       T trees, 1 <= T <= 256, each a complete binary tree with L levels of splits, 1 <= L <= 24, 2^L <= n < 2^31, d <= 4096.
 *               Node (l, j), 0 <= l < L, 0 <= j < 2^l, owns the slice [floor(j n / 2^l), floor((j + 1) n / 2^l)) of the tree's row
 *               permutation leaves[t] (int32 [n], LOCAL rows); the slices nest; a leaf is a slice at l = L; leaf_max = ceil(n / 2^L);
 *               T * leaf_max <= 8192 (mi_refine's kc limit).
 *   directions  dirs float64 [T L][d] row-major, host memory, every value finite; row c = t L + l serves level l of tree t.  The
 *               scale of a direction changes nothing.
 *   projection  P[i][c] = sum_k double(x_i[k]) * dirs[c][k] over the stored f32 row that mi_refine evaluates, on the f64 matrix
 *               pipe, k ascending over the instruction's steps of 4 from +0.0; the error bound is mi_lsh_encode's,
 *               (d + 2) 2^-53 sum_k |x r|; -0.0 is ordered as +0.0.  ONE kernel projects the stored rows of a build and the queries
 *               of a search, and the bits of a sum do not depend on where its row falls in a launch: a query that equals a stored
 *               row bit for bit gets that row's projections bit for bit.
 *   build       per tree t, from the identity permutation, for l = 0 .. L - 1, in every node (l, j): the node's rows are ordered by
 *               (P[row][t L + l] ascending, row id ascending), and with mid = floor((2 j + 1) n / 2^(l + 1))
 *               split[t][2^l - 1 + j] = P[leaves[t][mid]][t L + l], the smallest projection of the right child.  The permutation as
 *               the last level leaves it is the tree.  The same bytes on every call; a tree depends on the order of summation only
 *               where two projections of a node lie within the error bound of each other, and sums that are exact in any order
 *               give exact trees.  (A NaN projection of a stored row is ordered by its bits: behind +inf, or before -inf when its
 *               sign bit is set.)  The trees are built in groups whose scratch fits the global option "forest_build_bytes"
 *               (default 1 GiB), one tree at the least: n (8 L + 12) + ceil(n / 2048) 1024 bytes per tree of a group.
 *   descent     per query q and tree t: j = 0; for l = 0 .. L - 1: j = 2 j + (Pq[t L + l] >= split[t][2^l - 1 + j]); a NaN goes
 *               left.  The query is used as given: on an MI_NORM_L2 gallery normalise it yourself, or projections of two scales
 *               are compared.
 *   candidates  int64 [nq][T leaf_max]: slot t leaf_max + i holds row_offset + leaves[t][a + i], [a, b) the slice of the leaf
 *               reached in tree t; slots i >= b - a hold -1.
 *   answer      mi_refine_device on those candidates: distinct rows, order (value best first, id ascending), mi_refine's float64
 *               bits and padding; 1 <= k <= T leaf_max.
 * mi_forest_build makes the trees on the device (rows and projections never cross the host link).  mi_forest_create takes a
 * caller's trees: splits float64 [T][2^L - 1] and leaves int32 [T][n], both in host or both in device memory (`memspace`); a leaf
 * value outside [0, n) is MI_ERR_INVALID; repeats are legal (refine counts a row once).
 * The handle records the gallery's n: after mi_gallery_append* or mi_gallery_remove_rows every search returns MI_ERR_INVALID and
 * reads no stale table.  Not built: annoy's two-means hyperplanes, a priority queue shared by the trees (search_k), vote
 * thresholds, sparse directions, an allow bitmap, sharding, updating a forest in place. */
typedef struct mi_forest mi_forest; /* opaque */
int mi_forest_build(mi_gallery* rows, const double* dirs, int32_t T, int32_t L, mi_forest** out);
int mi_forest_create(mi_gallery* rows, const double* dirs, int32_t T, int32_t L, const double* splits, const int32_t* leaves,
                     int memspace, mi_forest** out);
/* n, d, T, L, leaf_max (any may be NULL); the tables of trees [tree0, tree0 + ntrees) and all directions into host memory */
int mi_forest_info(const mi_forest* f, int64_t* n, int32_t* d, int32_t* T, int32_t* L, int32_t* leaf_max);
int mi_forest_get_splits(mi_forest* f, int32_t tree0, int32_t ntrees, double* out_host);
int mi_forest_get_leaves(mi_forest* f, int32_t tree0, int32_t ntrees, int32_t* out_host);
int mi_forest_get_dirs(mi_forest* f, double* out_host);
int mi_forest_destroy(mi_forest* f); /* NULL is MI_OK */
/* The candidate slots alone.  Host form: queries of any strides and dtype as in mi_knn_search_l2 (f64 rounded to f32), out_cand
 * int64 [nq][T leaf_max] in host memory; synchronous, on the gallery's stream.  _device: q_dev [nq][d] packed f32, out_cand_dev
 * int64 [nq][T leaf_max]; enqueued on `stream`, no synchronisation.  nq == 0 is MI_OK and writes nothing. */
int mi_forest_candidates(mi_forest* f, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int64_t* out_cand,
                         double* out_seconds);
int mi_forest_candidates_device(mi_forest* f, const float* q_dev, int64_t nq, int64_t* out_cand_dev, void* stream);
/* Host form: queries as above, used as given; out_val (f32) and out_val64 may be NULL; synchronous, on the gallery's stream.
 * nq == 0 is MI_OK and writes nothing. */
int mi_forest_search(mi_forest* f, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                     int64_t* out_idx, float* out_val, double* out_val64, double* out_seconds);
/* q_dev [nq][d] packed f32; enqueued on `stream`, no synchronisation.  It stages the queries, their projections, the candidate
 * slots and the candidates' values in buffers of the handle (grown when a larger call comes; a batch whose projections, slots and
 * values would exceed 64 MiB runs in chunks of queries): calls on one handle must be serialised by the caller and enqueued on ONE
 * stream. */
int mi_forest_search_device(mi_forest* f, const float* q_dev, int64_t nq, int32_t k, int64_t* out_idx_dev, float* out_val_dev,
                            double* out_val64_dev, void* stream);

/* ---- IVF-Flat index: an inverted file over the RAW rows of a gallery, faiss IndexIVFFlat -- the reference's
 * matching_PQ_Net_bucket without the PQ loss.  DESIGN.md 5.18.  What is approximate is WHICH rows a query reaches (the rows of the
 * lists it probes); everything else is an exact, deterministic function of centroids, lists, stored rows and query.
 * A handle sits over ONE gallery `rows` (one shard on one device, squared-L2 or inner product, as for mi_refine, mi_graph and
 * mi_forest), which must outlive it.  The rows are neither copied nor permuted: the index costs 4 bytes per row plus the centroids.
 *   centroids   float32 [nlist][d] row-major in host memory, every value finite, 2 <= nlist <= 8192, d the caller's d of the
 *               gallery.  The handle keeps them on the device in rows of the gallery's padded stride.
 *   value       of (x, centroid) and of (query, row) alike, mi_refine's, with the same lane and column walk: on an L2 gallery the
 *               direct-form float64 squared distance, smaller is better; on any other gallery the float64 FMA inner product against
 *               the f32 values as stored or given, larger is better.
 *   order       (value best first, id ascending), for lists and for rows alike.
 *   probe       the nprobe best lists of a query in that order, 1 <= nprobe <= nlist: mi_refine over the centroid table.
 *   assignment  row i belongs to the probe-1 list of its STORED f32 row, the row mi_refine evaluates.
 *   lists       list_off int64 [nlist + 1], list_rows int32 [n] of LOCAL rows, ascending within a list; empty lists are legal.
 * mi_ivfflat_build assigns on the device, in chunks of stored rows (no row crosses the host link), and gives the same bytes on
 * every call.  mi_ivfflat_create takes the caller's list ids, int32 [n] in host or device memory (`memspace`); a value outside
 * [0, nlist) is MI_ERR_INVALID.
 *   search      per query the candidates are the rows of the probed lists that the allow bitmap (that of mi_knn_search_filtered:
 *               ceil(n / 64) words, bit (i & 63) of word (i >> 6) admits local row i; NULL admits all) admits; the answer is the
 *               best k of them in the order, 1 <= k <= 2048: ids row_offset + local row (int64), values float64 (out_val64) with
 *               their f32 cast (out_val); either may be NULL.  Fewer than k candidates: trailing ids -1, values +INFINITY (L2) or
 *               -INFINITY.  out_scanned (int64 [nq], may be NULL): the rows evaluated.  probes (may be NULL): int32 [nq][nprobe],
 *               the caller's lists in place of the library's; an entry outside [0, nlist) or repeating an earlier entry of its row
 *               is "no list".  The query is used as given.  nq == 0 is MI_OK and writes nothing.
 * Consequences: with nprobe == nlist and no bitmap an L2 gallery gives mi_knn_search_l2's ids and dist64 bit for bit; any probe set
 * gives the answer of mi_knn_search_l2 with the allow bitmap of those lists.  The answer does not depend on the batch or on how it
 * is split into launches (no atomics, no grid barrier).
 * The handle records the gallery's n and its internal count of removals: after mi_gallery_append* or mi_gallery_remove_rows probe
 * and search return MI_ERR_INVALID and read no stale table -- also when a removal and an append have put n back where it was.
 * Updating in place.  The assignment reads the stored row alone and a removal leaves the stored rows of the survivors bit for
 * bit, so both calls below have one contract: afterwards mi_ivfflat_info's n, mi_ivfflat_list_sizes, mi_ivfflat_get_lists (both
 * tables) and every probe and search are, bit for bit, those of mi_ivfflat_build(rows, the same centroids) on the gallery as it
 * now stands.  The centroids do not move.  Both are synchronous on the gallery's stream and take the gallery's and the handle's
 * locks; rows appended with mi_gallery_append_device on another stream must be complete before the call.
 *   mi_ivfflat_sync         takes in the rows [index n, gallery n) that mi_gallery_append* added since the index was made or last
 *                           updated: assigned as the build assigns (in chunks of stored rows, no row crosses the host link) and
 *                           spliced behind the rows of their lists.  *out_added (may be NULL): their number.  Nothing appended:
 *                           MI_OK, nothing written, no launch.  More than 2^31 - 1 rows afterwards: MI_ERR_INVALID, index unchanged.
 *                           Work: m * nlist row-centroid values for m new rows, where a new build evaluates n * nlist.
 *   mi_ivfflat_remove_rows  removes rows from the gallery under the index AND from the index: arguments and bitmap of
 *                           mi_gallery_remove_rows (ceil(n / 64) words, bit (i & 63) of word (i >> 6) names local row i, bits at or
 *                           beyond n ignored, host or device memory).  The index must be fresh.  The lists are compacted by the
 *                           bitmap (survivor i becomes i - the named rows below i; lists stay ascending), the gallery's rows by
 *                           mi_gallery_remove_rows's own code.  *out_removed (may be NULL): n - n'.  No row named: MI_OK, 0,
 *                           nothing touched.  Every row named: MI_ERR_INVALID before anything is touched (an index needs a row).
 *                           Whatever makes mi_gallery_remove_rows refuse (an online handle on the gallery) makes this refuse,
 *                           index and gallery unchanged.
 * A removal made through mi_gallery_remove_rows alone is NOT followed: probe, search and mi_ivfflat_sync then return
 * MI_ERR_INVALID (a removal was made outside the index: build a new index).
 * Storage: either call writes new list tables beside the old ones, swaps them in and frees the old ones and its scratch.  After a
 * sync or a removal the handle costs what it costs after a build: 4 bytes per row (list_rows is exactly [n]) plus 8 * (nlist + 1)
 * bytes of list_off and the centroids; hbm_bytes reports what is held.  During the call the device also holds the new list_rows
 * (4 bytes per row of the result) and scratch: a sync 8 bytes per appended row plus the assignment's values (at most 64 MiB), a
 * removal the bitmap, its rank table and n / 64 bytes of counts.
 * Not built: sharding, residuals, a list-major scan that shares a list's rows between the queries that probe it, re-training or
 * moving centroids.  Nothing routes to this index by default, and its speed has not been measured. */
typedef struct mi_ivfflat mi_ivfflat; /* opaque */
int mi_ivfflat_build(mi_gallery* rows, const float* centroids, int32_t nlist, mi_ivfflat** out);
int mi_ivfflat_create(mi_gallery* rows, const float* centroids, int32_t nlist, const int32_t* list_ids, int memspace,
                      mi_ivfflat** out);
/* n, d, nlist, hbm_bytes (any may be NULL); the list sizes int64 [nlist], list_off int64 [nlist + 1] and list_rows int32 [n]
 * (either may be NULL) and the centroids float32 [nlist][d] into host memory */
int mi_ivfflat_info(const mi_ivfflat* f, int64_t* n, int32_t* d, int32_t* nlist, int64_t* hbm_bytes);
int mi_ivfflat_list_sizes(mi_ivfflat* f, int64_t* out_sizes);
int mi_ivfflat_get_lists(mi_ivfflat* f, int64_t* out_list_off, int32_t* out_list_rows);
int mi_ivfflat_get_centroids(mi_ivfflat* f, float* out_host);
int mi_ivfflat_destroy(mi_ivfflat* f); /* NULL is MI_OK */
int mi_ivfflat_sync(mi_ivfflat* f, int64_t* out_added);
int mi_ivfflat_remove_rows(mi_ivfflat* f, const uint64_t* remove_bits, int memspace, int64_t* out_removed);
/* Every query entry point is a device form: q_dev [nq][d] packed f32, probes_dev and allow_dev in device memory (either may be
 * NULL), outputs in device memory; enqueued on `stream`, no synchronisation.  It stages the queries, the probes, their prefixes
 * and the partial lists of the scan in buffers of the handle (grown when a larger call comes; a batch whose staging would exceed
 * 256 MiB runs in chunks of queries): calls on one handle must be serialised by the caller and enqueued on ONE stream.
 * mi_ivfflat_probe_device writes the probes alone, int32 [nq][nprobe].  Not built: host forms that take queries of any element
 * type and strides, as mi_knn_search_l2 does (a caller stages its queries as packed f32; the Python binding does). */
int mi_ivfflat_probe_device(mi_ivfflat* f, const float* q_dev, int64_t nq, int32_t nprobe, int32_t* out_probes_dev, void* stream);
int mi_ivfflat_search_device(mi_ivfflat* f, const float* q_dev, int64_t nq, int32_t k, int32_t nprobe, const int32_t* probes_dev,
                             const uint64_t* allow_dev, int64_t* out_idx_dev, float* out_val_dev, double* out_val64_dev,
                             int64_t* out_scanned_dev, void* stream);

/* ---- binary index: exact Hamming top-K on packed binary codes.  The reference's matching_Greedyhash(K, hash_codes_train,
 * hash_codes_test) (src/utils/nnsearch.py:1001-1013: XOR against every gallery code, sum, argsort, first K) and faiss
 * IndexBinaryFlat (what IndexLSH, src/utils/nnsearch.py:734-745, searches with internally).  DESIGN.md 5.13.
 * A code is nbits bits, nbits a multiple of 8 in [8, 4096], passed as nbits / 8 bytes per row: bit j is bit (j & 7) of byte
 * (j >> 3) -- np.packbits(..., bitorder='little'), faiss's convention.  A 2048-bit code takes 256 bytes of HBM.  The handle is
 * a type of its own, ONE row shard on ONE device like mi_gallery; none of the mi_gallery entry points takes it.  The answer is
 * integer and fully determined: ids row_offset + local row ordered by (distance asc, id asc), ties at the K-th distance to the
 * lowest ids, however many rows share it -- no certificate, no flag, no fallback path.  Out of scope for binary indexes: row
 * removal, save / load, sharding.
 * mi_hamming_create: n rows of `codes` (row i at codes + i * row_stride_bytes; MI_HOST or MI_DEVICE, device rows complete when
 * the call is made) into an index of `capacity` rows (0 = n); codes == NULL with n == 0 and capacity > 0 gives an empty
 * appendable index.  Synchronous. */
typedef struct mi_hamming mi_hamming; /* opaque */
int mi_hamming_create(const void* codes, int64_t n, int32_t nbits, int64_t row_stride_bytes, int memspace, int device,
                      int64_t row_offset, int64_t capacity, mi_hamming** out);
/* m more rows, synchronous.  Beyond the capacity: MI_ERR_INVALID like mi_gallery_append, and the index stays as it was. */
int mi_hamming_append(mi_hamming* h, const void* codes, int64_t m, int64_t row_stride_bytes, int memspace);
/* Sign bits of m device rows x_dev [m][d] f32 (row i at x_dev + i * row_stride floats), d == nbits, appended without leaving
 * the device: bit j = x[j] > 0 (NaN and +-0 give 0) -- GreedyHash's code layer is sign().  Enqueued on `stream`, no
 * synchronisation: later calls on the handle go to the same stream (or follow its completion). */
int mi_hamming_append_sign_device(mi_hamming* h, const float* x_dev, int64_t m, int32_t d, int64_t row_stride, void* stream);
/* The same packing stand-alone (queries): n rows of d floats (d a multiple of 8) -> n rows of d / 8 bytes at
 * out_row_stride_bytes.  Enqueued on `stream`. */
int mi_pack_sign_bits_device(const float* x_dev, int64_t n, int32_t d, int64_t row_stride, uint8_t* out_dev,
                             int64_t out_row_stride_bytes, void* stream);
/* Any out pointer may be NULL.  hbm_bytes: codes plus the grow-only search buffers the handle holds right now. */
int mi_hamming_info(const mi_hamming* h, int64_t* n, int32_t* nbits, int32_t* device, int64_t* row_offset, int64_t* capacity,
                    int64_t* hbm_bytes);
/* Rows [row0, row0 + nrows) as the caller gave them, nbits / 8 bytes each, to a host buffer. */
int mi_hamming_get_codes(mi_hamming* h, int64_t row0, int64_t nrows, uint8_t* out_host);
/* Host in, host out, synchronous.  q_codes: nq rows of nbits / 8 bytes at q_row_stride_bytes.  1 <= k <= 2048.  out_idx [nq][k]
 * int64, out_dist [nq][k] int32 (may be NULL).  allow_bits NULL: every row; otherwise the bitmap of mi_knn_search_filtered
 * (ceil(n / 64) words, bit (i & 63) of word (i >> 6) admits local row i; MI_HOST or MI_DEVICE), one bitmap for every query.
 * Fewer than k admitted rows: trailing ids -1, distances INT32_MAX.  nq == 0 is MI_OK.  out_seconds (may be NULL): wall time
 * of the call.  The queries of a call pass through a uint16 distance matrix [queries][n rounded up to 64] owned by the handle,
 * in chunks that keep it within the global option "hamming_matrix_bytes" (default 2 GiB; one query at the least). */
int mi_hamming_search(mi_hamming* h, const void* q_codes, int64_t nq, int64_t q_row_stride_bytes, int32_t k,
                      const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, int32_t* out_dist, double* out_seconds);
/* Device-resident variant, enqueued on `stream` without synchronising: q_dev packed [nq][nbits / 8], allow_bits_dev (may be
 * NULL) and the outputs are device buffers (out_dist_dev may be NULL).  The answer is complete when the stream reaches it;
 * there is no flag to read.  The call uses buffers of the handle (grown, i.e. freed and allocated again, when a larger batch
 * comes): calls on one handle must be serialised by the caller and enqueued on ONE stream. */
int mi_hamming_search_device(mi_hamming* h, const uint8_t* q_dev, int64_t nq, int32_t k, const uint64_t* allow_bits_dev,
                             int64_t* out_idx_dev, int32_t* out_dist_dev, void* stream);
/* Radius search: for every query, EVERY admitted row with Hamming distance <= radius -- inclusive, like the >= of
 * mi_range_search (faiss's binary range_search is believed to take distance < radius: its radius would be this one plus one).
 * 0 <= radius; a radius >= nbits returns every admitted row; a negative one is MI_ERR_INVALID.  Results in CSR form: the hits of
 * query i are out_idx/out_dist[out_lims[i] .. out_lims[i+1]), ordered by (distance asc, id asc), ids row_offset + local row; a
 * query has anywhere from 0 to n hits.  out_lims [nq + 1] is always written in full.  If out_lims[nq] > max_results, nothing is
 * written to out_idx / out_dist and MI_ERR_CAPACITY is returned: call again with max_results >= out_lims[nq].  out_dist may be
 * NULL; out_idx may be NULL when max_results is 0.  nq == 0 is MI_OK.  Queries, bitmap and out_seconds as in mi_hamming_search.
 * Integer and fully determined: positions are prefix sums, not the order in which the device ran.  There is no distance matrix:
 * a (block of 64 rows, query) pair leaves one 64-bit word in a workspace of at most the global option "hamming_range_bytes"
 * (10 bytes per pair; default 1 GiB), which the queries pass through in chunks of 64 at the least, plus 8 bytes per hit of one
 * chunk.  A call of more than one chunk scans the index three times instead of once. */
int mi_hamming_range_search(mi_hamming* h, const void* q_codes, int64_t nq, int64_t q_row_stride_bytes, int32_t radius,
                            const uint64_t* allow_bits, int allow_memspace, int64_t max_results, int64_t* out_lims,
                            int64_t* out_idx, int32_t* out_dist, double* out_seconds);
/* Device-resident variant, enqueued on `stream` without synchronising: q_dev packed [nq][nbits / 8], allow_bits_dev (may be NULL),
 * out_lims_dev [nq + 1], out_idx_dev / out_dist_dev [max_results] are device buffers.  The capacity is decided on the device:
 * when out_lims_dev[nq] > max_results nothing is written to out_idx_dev / out_dist_dev and the call still returns MI_OK -- the
 * caller reads out_lims_dev[nq] once the stream has reached it.  The staging of the hits is sized by max_results (at most
 * n hits per query of a chunk).  Buffers and stream contract of mi_hamming_search_device: one stream, calls serialised by the
 * caller. */
int mi_hamming_range_search_device(mi_hamming* h, const uint8_t* q_dev, int64_t nq, int32_t radius,
                                   const uint64_t* allow_bits_dev, int64_t max_results, int64_t* out_lims_dev,
                                   int64_t* out_idx_dev, int32_t* out_dist_dev, void* stream);
/* Self-join of stored rows: query i is row row0 + i, 0 <= i < nrows, read on the device from the index itself; only the rows
 * j > row0 + i are reported (each near pair once, no self pairs), and the blocks of rows at or below row0 are not scanned.
 * No bitmap.  Output and capacity protocol of mi_hamming_range_search.  row0 or nrows outside [0, n] (or row0 + nrows > n) is
 * MI_ERR_INVALID; nrows == 0 is MI_OK. */
int mi_hamming_self_range(mi_hamming* h, int64_t row0, int64_t nrows, int32_t radius, int64_t max_results, int64_t* out_lims,
                          int64_t* out_idx, int32_t* out_dist, double* out_seconds);
int mi_hamming_destroy(mi_hamming* h); /* NULL is MI_OK */

/* ---- Connected components: near-duplicate GROUPS from self-join hits.  DESIGN.md 5.13d.  The self-joins (mi_range_search on
 * stored rows, mi_minkowski_self_range, mi_hamming_self_range) return pairs; mi_gallery_set_groups wants one label per row.  This
 * handle closes "a ~ b and b ~ c, so a, b and c are one item" on the device: a union-find forest of n int32 entries, 4 bytes of
 * device memory per row, in which a root is only ever hooked under a smaller root.  Hence
 *   labels    out_labels[v] is the SMALLEST row of v's component (a row of its own is its own label); they are a function of the
 *             SET of edges added since creation or the last reset -- the order of the edges, their split into calls, the memspace
 *             and the source (pairs, CSR or ballots) make no difference, and neither does the order in which the device ran.
 * Ids.  Every id is a local row in [0, n); anything else is MI_ERR_INVALID.  Host arrays are checked on the host before a device
 * is touched, device arrays by a flag kernel before anything is united: a failed call leaves the components as they were.
 * i == j is allowed and does nothing; so does an edge given twice.  m == 0 or nq == 0 is MI_OK.
 * All calls are synchronous: they return when the work is done.  A handle is ONE device's; calls on one handle are serialised.
 * Integer and exact: no tolerance, no flag, no fallback.
 * Out of scope: pair-free paths for the inner-product and the Minkowski joins (they feed mi_components_add_csr from the host CSR
 * they return already); removing edges (reset and add again); sharded galleries, indexes with row_offset != 0, n > INT32_MAX;
 * saving a handle.
 * mi_components_create: 0 <= n <= INT32_MAX, else MI_ERR_INVALID before a device is touched; every row a component of its own.
 * mi_components_reset: every row a component of its own again. */
typedef struct mi_components mi_components; /* opaque; 4 bytes of device memory per row */
int mi_components_create(int64_t n, int device, mi_components** out);
int mi_components_reset(mi_components* h);
/* m edges (i[e], j[e]); both arrays MI_HOST or both MI_DEVICE (device arrays complete when the call is made). */
int mi_components_add_pairs(mi_components* h, const int64_t* i, const int64_t* j, int64_t m, int memspace);
/* The CSR output of a self-join whose queries are stored rows: query q is row row0 + q, 0 <= q < nq, and its hits are
 * idx[lims[q] .. lims[q+1]) -- what mi_range_search, mi_minkowski_self_range, mi_hamming_self_range and their Python forms return
 * for such queries (of an index with row_offset 0).  A row listed among its own hits is harmless.  lims [nq + 1] must be
 * non-decreasing with lims[0] == 0, and row0 .. row0 + nq must lie in [0, n]: otherwise MI_ERR_INVALID.  lims and idx are both
 * MI_HOST or both MI_DEVICE; device offsets are read back (8 (nq + 1) bytes), the hits stay where they are. */
int mi_components_add_csr(mi_components* h, int64_t row0, const int64_t* lims, const int64_t* idx, int64_t nq, int memspace);
/* Unites every pair (row0 + q, j), 0 <= q < nrows, j > row0 + q, of Hamming distance <= radius: exactly the pairs
 * mi_hamming_self_range(b, row0, nrows, radius, ...) reports -- but no pair is staged, counted, ordered or returned.  Per chunk of
 * queries the self-join's scan launch leaves its 64-bit ballots in the index's own workspace (chunked as there, global option
 * "hamming_range_bytes" included) and a union launch reads them; the offsets, fill and order stages do not run.  b must hold
 * exactly n rows on the handle's device with row_offset 0, else MI_ERR_INVALID; argument checks otherwise those of
 * mi_hamming_self_range; nrows == 0 is MI_OK.  Runs on the index's stream under the index's one-stream contract, and returns when
 * it is done. */
int mi_components_add_hamming_self(mi_components* h, mi_hamming* b, int64_t row0, int64_t nrows, int32_t radius);
/* out_labels [n] int32 in `memspace` (MI_HOST or MI_DEVICE), ready for mi_gallery_set_groups; out_groups (may be NULL) receives
 * the number of components.  The forest is kept flat between calls, so this is a copy (and a count).  The call does not end the
 * handle: more edges may be added afterwards. */
int mi_components_labels(mi_components* h, int32_t* out_labels, int memspace, int64_t* out_groups);
int mi_components_info(const mi_components* h, int64_t* n, int32_t* device);
int mi_components_destroy(mi_components* h); /* NULL is MI_OK */

/* ---- LSH codes: float descriptors -> packed sign codes of their projections, the first half of faiss IndexLSH(d, nbits)
 * (matching_LSH_faiss, src/utils/nnsearch.py:734-745); the second half is the Hamming search above.  DESIGN.md 5.13b.
 *   bit j of row i  =  ( sum_k double(x[i][k]) * R[j][k]  >=  t[j] ),       t == NULL: every threshold 0
 * with `>=`, faiss's fvecs2bitvecs rule -- not the `> 0` of mi_pack_sign_bits_device: a sum exactly at its threshold gives 1,
 * -0.0 >= 0 gives 1, a NaN sum gives 0.  Bit j is bit (j & 7) of byte (j >> 3), as for every binary code here.
 * X: n rows of d elements, MI_F32 or MI_F64, element (i, k) at X + i * row_stride + k * col_stride (in elements; the reference's
 * [D, N] matrix is row_stride 1, col_stride N).  R: float64 [nbits][d] row-major (any directions; faiss uses the first nbits rows
 * of a random rotation, _lib.lsh_rotation).  t: float64 [nbits].  nbits a multiple of 8 in [8, 4096], 1 <= d <= 4096, n >= 0
 * (n == 0 is MI_OK).  out: nbits / 8 bytes per row at out_row_stride_bytes >= nbits / 8; bytes of a row beyond nbits / 8 are
 * not touched.
 * The sum is float64 on the f64 matrix pipe, x promoted to double (exact), k ascending across the steps of 4 of the matrix
 * instruction: its error is at most (d + 2) 2^-53 sum_k |x[i][k] R[j][k]|, so a bit depends on the order of summation only when
 * the projection lies within that distance of its threshold; sums that are exact in any order (small integers) are compared
 * exactly.  The float64 products are never stored: the kernel writes the codes alone.
 * mi_lsh_encode_device: every operand on the device; enqueued on `stream`, no synchronisation. */
int mi_lsh_encode_device(const void* X_dev, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride,
                         const double* R_dev, const double* thr_dev, int32_t nbits, uint8_t* out_dev, int64_t out_row_stride_bytes,
                         void* stream);
/* Host operands, host result [n][nbits / 8] packed, synchronous.  The rows pass through the device in blocks of at most 64 MiB,
 * so host and device memory stay bounded whatever n is; the codes do not depend on the blocks. */
int mi_lsh_encode(const void* X, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride, const double* R,
                  const double* thr, int32_t nbits, int device, uint8_t* out);
/* The codes of m device rows appended to a binary index without leaving the device and without an intermediate buffer; nbits is
 * the handle's.  Stream contract of mi_hamming_append_sign_device: enqueued on `stream`, no synchronisation, later calls on the
 * handle go to the same stream (or follow its completion).  Beyond the capacity: MI_ERR_INVALID, and the index stays as it was. */
int mi_hamming_append_lsh_device(mi_hamming* h, const void* X_dev, int64_t m, int32_t d, int dtype, int64_t row_stride,
                                 int64_t col_stride, const double* R_dev, const double* thr_dev, void* stream);

/* ---- PQ index: exact ADC top-K on product-quantized codes.  The reference's matching_PQ_Net(K, Codewords, Query, N_books,
 * CW_idx) (src/utils/nnsearch.py:905-946), nanopq's pq.dtable(query).adist(codes), faiss IndexPQ.search.  DESIGN.md 5.14.
 * m books (1 <= m <= 64) of ks codewords (2 <= ks <= 256) of L = d / m floats, d <= 4096; a code is m bytes, byte j the
 * codeword of book j.  Codebooks are float32 [m][ks][L] in C order (nanopq's pq.codewords, faiss's ProductQuantizer.centroids)
 * and must be finite.  Given codebooks and codes the search is exhaustive and its answer is fully determined:
 *   table     T[q][j][c] = (float) sum_{i < L} (double(x[q][j L + i]) - double(C[j][c][i]))^2, the sum in float64 in ascending i,
 *             a separate multiply and add per term (nothing fused), rounded once to float32
 *   distance  dist[q][r] = T[q][0][code[r][0]] + T[q][1][code[r][1]] + ... in float32, added in ascending book order
 *   order     (distance asc, id asc), ids row_offset + local row; +inf (a table entry beyond float32) is an ordinary value
 *   encoding  code[r][j] = argmin_c of the float64 sum above (before the rounding), ties to the lower c
 * No certificate, no flag, no fallback path.  The handle is a type of its own, ONE row shard on ONE device; none of the mi_gallery
 * entry points takes it.  Codebooks are learned by mi_pq_train (below); mi_ivfpq (further below) searches such codes by inverted
 * lists.  Rows leave through mi_pq_remove_rows (below).  ks > 256: the wide index mi_pqw (below).  Out of scope: save / load, sharding, re-ranking.
 * mi_pq_create: n rows of `codes` (row i at codes + i * row_stride_bytes; MI_HOST or MI_DEVICE, device rows complete when the
 * call is made) into an index of `capacity` rows (0 = n); codes == NULL with n == 0 and capacity > 0 gives an empty appendable
 * index.  A code byte >= ks is MI_ERR_INVALID (host codes are checked before a device is touched).  Synchronous. */
typedef struct mi_pq mi_pq; /* opaque */
int mi_pq_create(const float* codebooks_host, int32_t d, int32_t m, int32_t ks, const void* codes, int64_t n,
                 int64_t row_stride_bytes, int memspace, int device, int64_t row_offset, int64_t capacity, mi_pq** out);
/* rows more codes, synchronous.  Beyond the capacity, or a code byte >= ks: MI_ERR_INVALID, and the index stays as it was. */
int mi_pq_append_codes(mi_pq* h, const void* codes, int64_t rows, int64_t row_stride_bytes, int memspace);
/* Encodes rows x [rows][d] (MI_F32 or MI_F64; element (i, j) at x + i * row_stride + j * col_stride elements; MI_HOST or
 * MI_DEVICE) on the device and appends the codes.  Synchronous; the same capacity rule. */
int mi_pq_add(mi_pq* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace);
/* The same encoding stand-alone: out_codes_host [rows][m] bytes; the index is unchanged. */
int mi_pq_encode(mi_pq* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace,
                 uint8_t* out_codes_host);
/* nanopq's dtable: the tables of nq host queries, out_table_host [nq][m][ks] float32.  Non-finite queries: MI_ERR_INVALID. */
int mi_pq_dtable(mi_pq* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, float* out_table_host);
/* Host in, host out, synchronous.  Queries as for mi_knn_search_l2 (any strides); non-finite queries are MI_ERR_INVALID.
 * 1 <= k <= 2048.  out_idx [nq][k] int64, out_dist [nq][k] float32 (may be NULL).  allow_bits NULL: every row; otherwise the
 * bitmap of mi_hamming_search, one for every query.  Fewer than k admitted rows: trailing ids -1, distances +inf.  nq == 0 is
 * MI_OK.  out_seconds (may be NULL): wall time of the call.  The queries of a call pass through a float32 matrix [queries][n
 * rounded up to 64] owned by the handle, in chunks that keep it within the global option "pq_matrix_bytes" (default 2 GiB; four
 * queries at the least); the answer does not depend on the chunking. */
int mi_pq_search(mi_pq* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                 const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_dist, double* out_seconds);
/* Device-resident variant, enqueued on `stream` without synchronising: q_dev packed [nq][d] float32, allow_bits_dev (may be
 * NULL) and the outputs are device buffers (out_dist_dev may be NULL).  A non-finite query leaves the order of ITS answer
 * unspecified (nothing is read or written out of bounds).  Buffers of the handle are used and grown as for
 * mi_hamming_search_device: calls on one handle must be serialised by the caller and enqueued on ONE stream. */
int mi_pq_search_device(mi_pq* h, const float* q_dev, int64_t nq, int32_t k, const uint64_t* allow_bits_dev, int64_t* out_idx_dev,
                        float* out_dist_dev, void* stream);
/* Any out pointer may be NULL.  hbm_bytes: codes, codebooks and the grow-only buffers the handle holds right now. */
int mi_pq_info(const mi_pq* h, int64_t* n, int32_t* d, int32_t* m, int32_t* ks, int32_t* device, int64_t* row_offset,
               int64_t* capacity, int64_t* hbm_bytes);
/* Rows [row0, row0 + nrows) as given or encoded, m bytes each, to a host buffer. */
int mi_pq_get_codes(mi_pq* h, int64_t row0, int64_t nrows, uint8_t* out_host);
/* The codebooks as given, [m][ks][L] float32. */
int mi_pq_get_codebooks(const mi_pq* h, float* out_host);
/* Removes rows in place (faiss IndexPQ.remove_ids); DESIGN.md 5.14e.  The arguments are those of mi_gallery_remove_rows:
 * remove_bits is a bitmap of ceil(n / 64) words over the index's LOCAL rows (bit i & 63 of word i >> 6 names row i), a host or a
 * device buffer (memspace); bits at or beyond n are ignored; out_removed (may be NULL) receives the number of rows that left.  The
 * survivors keep their relative order and are renumbered 0 .. n' - 1, so ids become row_offset + new local row.  Code bytes are
 * moved, never re-encoded, and the capacity stays: afterwards the index cannot be told apart, through any entry point, from a
 * fresh one of the same capacity, codebooks and row_offset to which the survivors' codes were appended in order (mi_pq_info's
 * hbm_bytes excepted: it counts the grow-only scratch) -- searches return the same ids and the same distance bits, and later
 * appends go behind row n' - 1.  Removing every row leaves a valid empty index.  A bitmap that names no row, or n == 0, is MI_OK and
 * touches nothing.  A NULL handle, a NULL bitmap or a bad memspace is MI_ERR_INVALID before anything else.  Synchronous, under the
 * handle's mutex, on the handle's stream.  Device memory beyond the index: a staging area of B rows of codes (global option
 * "pq_remove_block_rows"), the bitmap and 4 bytes per bitmap word, kept on the handle and allocated before anything moves, so an
 * allocation that fails (MI_ERR_NOMEM) leaves the index as it was. */
int mi_pq_remove_rows(mi_pq* h, const uint64_t* remove_bits, int memspace, int64_t* out_removed);
int mi_pq_destroy(mi_pq* h); /* NULL is MI_OK */
/* Learning the codebooks: Lloyd's k-means iteration per book from given initial centroids, as a deterministic function of its
 * inputs -- scipy.cluster.vq.kmeans2(minit="matrix"), the routine nanopq's PQ.fit runs, made reproducible on the device.  DESIGN.md
 * 5.14b.  Training rows x [n][d] (MI_F32 or MI_F64; element (r, i) at x + r * row_stride + i * col_stride elements; MI_HOST or
 * MI_DEVICE), m books of ks codewords of L = d / m floats with the limits of mi_pq_create, n >= ks, iters >= 1.  C_0 is
 * init_codebooks_host ([m][ks][L] float32, finite; passing a result back in RESUMES a run) or, when NULL, codeword c of every book
 * is the book's slice of row floor(c * n / ks), rounded to float32.  For t = 0 .. iters - 1:
 *   assign   code_t[r][j] = what mi_pq_encode returns for row r under C_t (float64 argmin, ties to the lower codeword)
 *   moved    moved[t] = number of (r, j) with code_t[r][j] != code_{t-1}[r][j]; moved[0] = n * m.  t > 0 and moved[t] == 0:
 *            training stops, the result is C_t and moved[t + 1 ..] = 0 (exact: the same members give the same sums)
 *   update   for every (j, c) with members: S[i] = sum of double(x[r][j L + i]) over the members r in ASCENDING r, from +0.0, each
 *            an IEEE float64 add; C_{t+1}[j][c][i] = (float)(S[i] / (double)count), one IEEE float64 divide, rounded once to
 *            float32.  A codeword without members keeps its value (kmeans2's rule, hence nanopq's)
 * out_codebooks_host [m][ks][L] receives C_iters, out_moved [iters] (may be NULL) the move counts, out_seconds (may be NULL) the
 * wall time of the call.  Centroids are rounded to float32 after EVERY iteration, so every step can be checked through
 * mi_pq_encode, and iters = a followed by iters = b from the result equals iters = a + b bit for bit; two calls on the same input
 * return the same bytes.  Not a goal: nanopq's or faiss's random draw of initial points, or their float32 arithmetic.
 * Synchronous, on a stream of its own, no handle and no state left behind.  Host rows are uploaded ONCE, packed [n][d] in their own
 * type (n * d * 4 or 8 bytes of device memory: 8.2 GB at 1 005 994 x 2048 float32), and all iterations run from that copy; device
 * rows are used where they lie and must be complete when the call is made.  Besides: 3 * n * m bytes of codes and the codebooks;
 * one 8-byte read-back per iteration decides the early stop.  Every argument check -- the limits, n >= ks, iters >= 1, NULL
 * pointers, a non-finite initial codebook, non-finite HOST rows -- answers MI_ERR_INVALID before a device is touched.  Non-finite
 * DEVICE rows leave the codebooks of the books they touch unspecified (nothing is read or written out of bounds).  An allocation
 * that fails: MI_ERR_NOMEM, everything freed. */
int mi_pq_train(const void* x, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride, int memspace, int32_t m,
                int32_t ks, int32_t iters, const float* init_codebooks_host, int device, float* out_codebooks_host,
                int64_t* out_moved, double* out_seconds);
/* Device times (HIP events, milliseconds) of the calling thread's last mi_pq_train: the assignment (encode and move count) of
 * every iteration that ran and the update of every iteration that had one; at most `capacity` values each are written, the
 * numbers that ran go to out_assignments / out_updates (may be NULL). */
int mi_pq_train_timing(int32_t capacity, float* out_assign_ms, float* out_update_ms, int32_t* out_assignments, int32_t* out_updates);

/* ---- Wide PQ index: mi_pq with up to 8192 codewords per book, the reference's matching_Nano_PQ as its entry points call it
 * (N_books = 16, n_bits_perbook = 13; src/offline.py:110).  DESIGN.md 5.14f.  m books (1 <= m <= 64) of ks codewords
 * (2 <= ks <= 8192) of L = d / m floats, d <= 4096; a code is m uint16, element j the codeword of book j, and crosses this
 * interface as uint16 [rows][row_stride] (row_stride in ELEMENTS, >= m; what lies between the rows is not read).  The handle is
 * a type of its own and mirrors mi_pq entry point for entry point; table, distance, order, encoding, allow bitmaps, k <= 2048,
 * the chunking within "pq_matrix_bytes" and every rule of synchronisation are those stated for mi_pq above, word for word, and
 * for ks <= 256 every output equals mi_pq's on the same codebooks and codes bit for bit.  A code >= ks is MI_ERR_INVALID (host
 * codes are checked before a device is touched, device codes by a kernel before anything is written).  The gallery holds
 * 4 * ceil(m / 2) bytes a row.  Out of scope: ks > 8192, row removal, an IVF or graph index over wide codes. */
typedef struct mi_pqw mi_pqw; /* opaque */
int mi_pqw_create(const float* codebooks_host, int32_t d, int32_t m, int32_t ks, const void* codes, int64_t n, int64_t row_stride,
                  int memspace, int device, int64_t row_offset, int64_t capacity, mi_pqw** out);
int mi_pqw_append_codes(mi_pqw* h, const void* codes, int64_t rows, int64_t row_stride, int memspace);
int mi_pqw_add(mi_pqw* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace);
/* out_codes_host [rows][m] uint16 */
int mi_pqw_encode(mi_pqw* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace,
                  uint16_t* out_codes_host);
/* out_table_host [nq][m][ks] float32: 512 KiB a query at 16 x 8192 */
int mi_pqw_dtable(mi_pqw* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, float* out_table_host);
int mi_pqw_search(mi_pqw* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                  const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_dist, double* out_seconds);
int mi_pqw_search_device(mi_pqw* h, const float* q_dev, int64_t nq, int32_t k, const uint64_t* allow_bits_dev, int64_t* out_idx_dev,
                         float* out_dist_dev, void* stream);
int mi_pqw_info(const mi_pqw* h, int64_t* n, int32_t* d, int32_t* m, int32_t* ks, int32_t* device, int64_t* row_offset,
                int64_t* capacity, int64_t* hbm_bytes);
/* Rows [row0, row0 + nrows) as given or encoded, m uint16 each, to a host buffer. */
int mi_pqw_get_codes(mi_pqw* h, int64_t row0, int64_t nrows, uint16_t* out_host);
int mi_pqw_get_codebooks(const mi_pqw* h, float* out_host);
/* As mi_pq_decode: float32 [nrows][d] to a host buffer. */
int mi_pqw_decode(mi_pqw* h, int64_t row0, int64_t nrows, float* out_host);
int mi_pqw_destroy(mi_pqw* h); /* NULL is MI_OK */
/* mi_pq_train with 2 <= ks <= 8192: the same arguments, the same iteration, the same bits (for ks <= 256 the result equals
 * mi_pq_train's).  3 * n * m * 2 bytes of codes on the device.  mi_pq_train_timing reports the calling thread's last training,
 * whichever of the two it was. */
int mi_pqw_train(const void* x, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride, int memspace, int32_t m,
                 int32_t ks, int32_t iters, const float* init_codebooks_host, int device, float* out_codebooks_host,
                 int64_t* out_moved, double* out_seconds);

/* ---- k-means over whole rows at f64 matrix rate: the coarse quantizer of the IVF indexes, faiss.Kmeans / Clustering, the
 * reference's sklearn.cluster.KMeans(n_clusters).fit / .predict (src/utils/nnsearch.py:967-989).  DESIGN.md 5.14g.
 * mi_kmeans_train is Lloyd's iteration with k centroids of d floats (2 <= k <= 8192, 1 <= d <= 4096, n >= k, iters >= 1) and its
 * contract is mi_pqw_train's with m = 1, word for word: the default C_0 (rows floor(c * n / k)), the float64 direct-form argmin
 * with ties to the lower centroid, moved[t] and the exact early stop, update sums in ascending row order with one divide, float32
 * centroids after every iteration, an empty centroid keeps its value, a result passed back in resumes the run.
 * out_centroids_host [k][d] and out_moved [iters] equal what mi_pqw_train(..., m = 1, ks = k, ...) writes, BIT FOR BIT.  What
 * differs is how the assignment is found: an f64 MFMA kernel evaluates ||c||^2 - 2 x.c for every (row, centroid) and decides every
 * row whose two best centroids lie further apart than a rounding bound (tau = 4 gamma (||x|| + max ||c||)^2, gamma = (d + 3) u /
 * (1 - (d + 3) u), u = 2^-53, every factor rounded up); the other rows -- near-ties, ties, NaN, infinity -- are decided by the
 * direct-form arithmetic itself.  out_flagged [iters] (may be NULL) receives, per iteration that ran, the number of rows of the
 * second kind (0 for the iterations that did not run).  Argument checks, the refusal of non-finite host rows, memory (one packed
 * copy of host rows, 3 * n * 2 bytes of ids, at most 64 MiB of workspace) and synchronisation are mi_pqw_train's; one 16-byte
 * read-back per iteration.  mi_pq_train_timing reports this call too.  x_dtype is MI_F32 or MI_F64, in all three entry points. */
int mi_kmeans_train(const void* x, int64_t n, int32_t d, int x_dtype, int64_t row_stride, int64_t col_stride, int memspace, int32_t k,
                    int32_t iters, const float* init_centroids_host, int device, float* out_centroids_host, int64_t* out_moved,
                    int64_t* out_flagged, double* out_seconds);
/* The assignment alone: out_ids[r] = the centroid nearest to row r, what mi_pqw_encode returns on a one-book index holding
 * centroids_host [k][d] (finite).  Host rows (any strides, finite) pass through the device in blocks of at most 64 MiB, as in
 * mi_lsh_encode; synchronous.  out_flagged (may be NULL): the rows the direct-form kernel decided. */
int mi_kmeans_assign(const void* x, int64_t n, int32_t d, int x_dtype, int64_t row_stride, int64_t col_stride,
                     const float* centroids_host, int32_t k, int device, int32_t* out_ids, int64_t* out_flagged);
/* The device form: rows, centroids [k][d] float32, ids [n] int32 and the optional flagged count (one uint64, set, not added to) on
 * the current device; enqueued on `stream`, no synchronisation, no allocation and NOTHING read back -- the direct-form kernel runs
 * with a fixed grid over a list whose length it reads from device memory.  The caller lends the workspace (8-byte aligned;
 * mi_kmeans_assign_workspace_bytes(k, n) is what serves n rows in the largest chunks the call uses, at most 64 MiB; anything from
 * mi_kmeans_assign_workspace_bytes(k, 128) up is accepted and only makes the chunks smaller) until the work on `stream` is done.
 * Non-finite rows get the id the direct form gives them. */
int mi_kmeans_assign_workspace_bytes(int32_t k, int64_t n, int64_t* out_bytes);
int mi_kmeans_assign_device(const void* x_dev, int64_t n, int32_t d, int x_dtype, int64_t row_stride, int64_t col_stride,
                            const float* centroids_dev, int32_t k, int32_t* out_ids_dev, uint64_t* out_flagged_dev,
                            void* workspace_dev, int64_t workspace_bytes, void* stream);

/* ---- graph index over PQ codes: best-first search of a neighbour graph whose rows are the codes of ONE mi_pq index, the role of
 * the reference's PQ + HNSW matchers (matching_HNSW_PQ, matching_HNSW_NanoPQ, matching_PQ_HNSW_faiss; src/utils/nnsearch.py:541-683,
 * 802-825).  DESIGN.md 5.16b.  No raw rows are resident: the index is the m code bytes and the 4 R table bytes of a row, and a
 * query's cost does not grow with n.  What is approximate is WHICH rows the graph reaches; given table, entries, codebooks,
 * codes and query the answer is fully determined:
 *   value      of a row: mi_pq_search's distance, bit for bit -- table entries T[j][c] the float64 sums rounded once to float32
 *              (the bits of mi_pq_dtable), the distance their float32 sum in ascending book order; +inf is an ordinary value
 *   order      (distance asc, id asc)
 *   traversal  mi_graph_search's start / step / stop / answer, word for word, with 1 <= k <= ef <= 2048: the visited set is exact,
 *              a row pushed out of W stays visited and is never expanded, and there are n expansions at the most whatever the
 *              table holds
 *   answer     the first k rows of W: ids row_offset + local row as mi_pq_search reports them, distances float32; fewer than k
 *              rows in W: trailing ids -1, distances +inf.  out_visited (int32 [nq], may be NULL): the number of rows evaluated,
 *              entries included.
 * The mi_pq handle must outlive the graph.  The graph records the index's rows and an internal modification count that
 * mi_pq_add, mi_pq_append_codes and mi_pq_remove_rows bump: after any of them -- also after a removal and an addition that
 * restore n -- a search returns MI_ERR_INVALID and reads no table.  The index itself is not changed by anything here.
 * mi_pq_graph_create takes a caller's table: neighbors [n][R] packed int32 of LOCAL rows in host or device memory, -1 being
 * padding anywhere in a row, n the index's rows (1 <= n <= 2^31 - 1), 1 <= R <= 64; entries int32 [ne] in host memory,
 * 1 <= ne <= 64.  An entry outside [0, n) or a table value below -1 or >= n is MI_ERR_INVALID; self-loops and repeats are legal.
 * (One use: mi_graph_get_neighbors of a graph built on the raw rows, searched on the codes once the raw gallery is closed.)
 * mi_pq_graph_build makes the table on the device, R even in [2, 64], 1 <= ne <= 64, n >= 2, the same bytes on every call: it is
 * mi_graph_build's F, B, N and entries over another value matrix -- row i's query is its own reconstruction, the float32
 * concatenation of C[j][code[i][j]], and its values are the distances above, from the exhaustive search (mi_pq_search_device with
 * k = min(R + 1, n), whose answers are in the order already).  Rows with identical codes are whole tie classes at distance 0; the
 * order and the rule "drop i, or the last row where i is absent" settle them.  The build is an n x n pass through the distance
 * matrix of the PQ index, in chunks within "pq_matrix_bytes".
 * Not built: an allow bitmap, sharding, updating a graph in place, ks > 256, the training of faiss's IndexHNSWPQ. */
typedef struct mi_pq_graph mi_pq_graph; /* opaque */
int mi_pq_graph_create(mi_pq* codes, const int32_t* neighbors, int32_t R, int neighbors_memspace, const int32_t* entries,
                       int32_t ne, mi_pq_graph** out);
int mi_pq_graph_build(mi_pq* codes, int32_t R, int32_t ne, mi_pq_graph** out);
/* n, R, ne, hbm_bytes (any may be NULL; hbm_bytes: table, entries and the grow-only workspace the handle holds right now); the
 * table rows [row0, row0 + nrows) and the ne entries into host memory */
int mi_pq_graph_info(const mi_pq_graph* gr, int64_t* n, int32_t* R, int32_t* ne, int64_t* hbm_bytes);
int mi_pq_graph_get_neighbors(mi_pq_graph* gr, int64_t row0, int64_t nrows, int32_t* out_host);
int mi_pq_graph_get_entries(mi_pq_graph* gr, int32_t* out_host);
int mi_pq_graph_destroy(mi_pq_graph* gr); /* NULL is MI_OK */
/* Host form: queries as for mi_pq_search (any strides, MI_F32 or MI_F64; non-finite queries are MI_ERR_INVALID); synchronous, on
 * the PQ index's stream.  out_dist and out_visited may be NULL.  nq == 0 is MI_OK and writes nothing. */
int mi_pq_graph_search(mi_pq_graph* gr, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                       int32_t ef, int64_t* out_idx, float* out_dist, int32_t* out_visited, double* out_seconds);
/* q_dev [nq][d] packed f32; enqueued on `stream`, no synchronisation.  A non-finite query leaves the order of ITS answer
 * unspecified (nothing is read or written out of bounds).  The queries' tables and the visited bitmaps live in buffers of the
 * graph handle (grown when a larger call comes; a batch whose bitmaps or tables would exceed 256 MiB runs in chunks of queries):
 * calls on one handle must be serialised by the caller and enqueued on ONE stream. */
int mi_pq_graph_search_device(mi_pq_graph* gr, const float* q_dev, int64_t nq, int32_t k, int32_t ef, int64_t* out_idx_dev,
                              float* out_dist_dev, int32_t* out_visited_dev, void* stream);
/* nanopq's pq.decode: rows [row0, row0 + nrows) of a PQ index reconstructed, float32 [nrows][d], to a host buffer; column
 * j L + i of a row is C[j][code[j]][i].  Synchronous, on the index's stream. */
int mi_pq_decode(mi_pq* h, int64_t row0, int64_t nrows, float* out_host);

/* ---- IVF index over PQ codes: exact ADC top-K over the rows of the probed lists.  The reference's matching_PQ_Net_bucket(K,
 * Codewords, Query, N_books, CW_idx, Gallery_features, n_clusters) (src/utils/nnsearch.py:949-998), faiss IndexIVFPQ with
 * by_residual = false.  DESIGN.md 5.14c.  nlist lists (2 <= nlist <= 256: a list id is one byte, like a code) with coarse centroids
 * G[nlist][d] float32, finite; codebooks, m, ks and d exactly as for mi_pq_create; fewer than 2^32 - 1 local rows.  The codes are
 * NOT residual codes: they are what mi_pq_encode gives the whole vector, so a query's table does not depend on the list and the
 * distance of (query, row) has the bits it has in mi_pq_search.  Given coarse centroids, codebooks, codes and the list of every
 * row the answer is fully determined:
 *   list      of a row the library assigns (mi_ivfpq_add): what mi_pq_encode returns on a 1-book index whose codebook is G -- the
 *             argmin over l of the float64 sum_i (double(x[i]) - double(G[l][i]))^2 (ascending i, nothing fused), ties to the lower l
 *   probes    of a query the library chooses: the nprobe lists smallest by (that float64 sum, l), in that order; 1 <= nprobe <=
 *             nlist.  Explicit probes (int32 [nq][nprobe]) replace the choice: the probe set of a query is the set of its distinct
 *             entries in [0, nlist); -1 is "no list", an entry equal to an earlier one of the same query is ignored; any other
 *             entry is MI_ERR_INVALID on the host path (before a device is touched) and counts as -1 on the device path
 *   answer    top-k by (distance asc, id asc) over the rows whose list is in the probe set and whose bit is set in the allow
 *             bitmap, if one is given; table, distance and the meaning of +inf are those of mi_pq_search, ids row_offset + local
 *             row; fewer than k such rows: trailing ids -1, distances +inf
 * With nprobe == nlist ids and distance bits equal mi_pq_search on the same codes.  The answer does not depend on the order in
 * which rows were appended, on how a batch is chunked or on how lists are cut into slabs.  No certificate, no flag, no fallback
 * path.  The handle is a type of its own, ONE row shard on ONE device; no mi_gallery or mi_pq entry point takes it.  Rows leave
 * through mi_ivfpq_remove_rows (below).  Out of scope: nlist > 256, grouping queries by list, save / load, sharding, re-ranking.
 * Residual codes: mi_ivfpq_create_residual (below).
 * mi_ivfpq_create: n rows of `codes` (as for mi_pq_create) with list_ids uint8 [n] in the same memspace, into an index of
 * `capacity` rows (0 = n); codes == NULL with n == 0 and capacity > 0 gives an empty appendable index.  A code byte >= ks or a
 * list id >= nlist is MI_ERR_INVALID: host data is checked on the host before a device is touched, device data by a flag kernel
 * whose flag is read before anything is ingested.  Synchronous.  An allocation that fails frees everything. */
typedef struct mi_ivfpq mi_ivfpq; /* opaque */
int mi_ivfpq_create(const float* coarse_host, int32_t nlist, const float* codebooks_host, int32_t d, int32_t m, int32_t ks,
                    const void* codes, const uint8_t* list_ids, int64_t n, int64_t row_stride_bytes, int memspace, int device,
                    int64_t row_offset, int64_t capacity, mi_ivfpq** out);
/* rows more codes with their lists, synchronous.  Beyond the capacity, a code byte >= ks or a list id >= nlist: MI_ERR_INVALID,
 * and the index stays as it was. */
int mi_ivfpq_append_codes(mi_ivfpq* h, const void* codes, const uint8_t* list_ids, int64_t rows, int64_t row_stride_bytes,
                          int memspace);
/* Assigns rows x [rows][d] (as for mi_pq_add) to their lists, encodes them and appends.  Synchronous; the same capacity rule. */
int mi_ivfpq_add(mi_ivfpq* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace);
/* The probes the library chooses for nq host queries: out_lists_host [nq][nprobe] int32.  Non-finite queries: MI_ERR_INVALID. */
int mi_ivfpq_probe(mi_ivfpq* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t nprobe,
                   int32_t* out_lists_host);
/* Host in, host out, synchronous.  Queries, k, allow_bits, outputs and out_seconds as for mi_pq_search; non-finite queries are
 * MI_ERR_INVALID; nq == 0 is MI_OK.  probes_host NULL: the library chooses nprobe lists per query; otherwise int32 [nq][nprobe]
 * as above.  The queries of a call pass in chunks that keep the partial lists ([queries][slabs of 4096 candidates][k] 8-byte
 * keys) within the global option "pq_matrix_bytes" (one query at the least); the answer does not depend on the chunking. */
int mi_ivfpq_search(mi_ivfpq* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                    int32_t nprobe, const int32_t* probes_host, const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx,
                    float* out_dist, double* out_seconds);
/* Device-resident variant, enqueued on `stream` without synchronising: q_dev packed [nq][d] float32; probes_dev (may be NULL)
 * int32 [nq][nprobe], allow_bits_dev (may be NULL) and the outputs are device buffers (out_dist_dev may be NULL).  A non-finite
 * query leaves ITS answer unspecified (nothing is read or written out of bounds).  Buffers of the handle are used and grown as
 * for mi_pq_search_device: calls on one handle must be serialised by the caller and enqueued on ONE stream. */
int mi_ivfpq_search_device(mi_ivfpq* h, const float* q_dev, int64_t nq, int32_t k, int32_t nprobe, const int32_t* probes_dev,
                           const uint64_t* allow_bits_dev, int64_t* out_idx_dev, float* out_dist_dev, void* stream);
/* Any out pointer may be NULL.  hbm_bytes: the block pool, tables, centroids and the grow-only buffers the handle holds now. */
int mi_ivfpq_info(const mi_ivfpq* h, int64_t* n, int32_t* d, int32_t* m, int32_t* ks, int32_t* nlist, int32_t* device,
                  int64_t* row_offset, int64_t* capacity, int64_t* hbm_bytes);
/* Rows per list: out [nlist] int64. */
int mi_ivfpq_list_sizes(const mi_ivfpq* h, int64_t* out);
/* Rows [row0, row0 + nrows) by ORIGINAL row order: out_codes_host [nrows][m] bytes, out_lists_host [nrows] bytes; either may be
 * NULL.  Only the blocks these rows lie in are read back from the device. */
int mi_ivfpq_get_rows(mi_ivfpq* h, int64_t row0, int64_t nrows, uint8_t* out_codes_host, uint8_t* out_lists_host);
/* Removes rows in place (faiss IndexIVFPQ.remove_ids), on either kind of index; DESIGN.md 5.14e.  Arguments, renumbering and error
 * answers are those of mi_pq_remove_rows.  A survivor keeps its code bytes and its list; every list is compacted where it lies and
 * the blocks it no longer reaches are reused by later appends, so n' + rows added later <= capacity works as on a fresh index.
 * Afterwards the index cannot be told apart, through any entry point (mi_ivfpq_info's n, mi_ivfpq_get_rows, mi_ivfpq_list_sizes,
 * the searches with library or explicit probes and with a bitmap in the NEW numbering, later appends), from a fresh one of the
 * same capacity, centroids, codebooks, kind and row_offset to which the survivors' codes and lists were appended in order;
 * hbm_bytes may include the scratch.  Device memory beyond the index: the bitmap and 4 bytes per bitmap word, allocated before
 * anything moves. */
int mi_ivfpq_remove_rows(mi_ivfpq* h, const uint64_t* remove_bits, int memspace, int64_t* out_removed);
int mi_ivfpq_destroy(mi_ivfpq* h); /* NULL is MI_OK */

/* ---- Residual IVF-PQ index: faiss IndexIVFPQ with by_residual = true (its default), the reference's ANN (src/utils/knn.py:43-53).
 * DESIGN.md 5.14d.  The same handle, limits, lists, probes and entry points; an index is residual or not for its whole life.  A
 * row's code quantizes its residual against the centroid of its list, and the arithmetic is the specification:
 *   residual  of a vector x (float32 or float64) against list l: r[j] = double(x[j]) - double(G[l][j]), ONE float64 subtraction per
 *             component, never rounded to float32 on the search or the encode path
 *   table     T[q][l][b][c] = float32(sum_j (r[b L + j] - double(C[b][c][j]))^2) for every probed list l of query q: ascending j, a
 *             separate float64 subtract, multiply and add per term (nothing fused), rounded once
 *   distance  of (query q, row i of list l): the float32 sum of T[q][l][b][code_i[b]] in ascending book order from +0.0f
 *   encoding  mi_ivfpq_add assigns the list as on any index; code byte b is then the argmin over c of that float64 sum taken of the
 *             row's own residual, ties to the lower c.  mi_ivfpq_append_codes and the codes given at creation ARE residual codes
 *             and are stored as given
 *   answer    as above: top-k by (distance asc, id asc) over the rows whose list is in the probe set and whose allow bit is set;
 *             independent of the order of appends, of the chunking of a batch and of how lists are cut into slabs
 * With every centroid zero the answer equals, bit for bit, that of a non-residual index over the same codes and lists.  The queries
 * of a call pass in chunks that keep the tables ([queries][nprobe][m][ks] float32) AND the partial lists within "pq_matrix_bytes"
 * (one query at the least).  mi_ivfpq_probe, _list_sizes, _get_rows, _info and _destroy do not depend on the kind.
 * mi_ivfpq_create_residual: the parameters, checks and error order of mi_ivfpq_create. */
int mi_ivfpq_create_residual(const float* coarse_host, int32_t nlist, const float* codebooks_host, int32_t d, int32_t m, int32_t ks,
                             const void* codes, const uint8_t* list_ids, int64_t n, int64_t row_stride_bytes, int memspace,
                             int device, int64_t row_offset, int64_t capacity, mi_ivfpq** out);
/* *out = 1 on a residual index, 0 otherwise. */
int mi_ivfpq_is_residual(const mi_ivfpq* h, int32_t* out);
/* out [rows][d] packed float32 = float32(double(x) - double(G[l])), one rounding: what codebook training consumes.  x as for
 * mi_ivfpq_add; l is list_ids[row] (uint8 [rows] in x's memspace; an id >= nlist is MI_ERR_INVALID) or, with list_ids NULL, the
 * list the library assigns.  out is a host or a device buffer (out_memspace).  Either kind of index; the index is unchanged.
 * Synchronous. */
int mi_ivfpq_residual_rows(mi_ivfpq* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace,
                           const uint8_t* list_ids, float* out, int out_memspace);
/* A measuring variant of mi_ivfpq_search_device (library probes, no bitmap; either kind of index): the same launches and the same
 * answer, with HIP events around the table kernel and around the scan-and-select of every chunk of queries; the sums over the
 * chunks, in milliseconds, go to *out_table_ms and *out_scan_ms.  It waits for every chunk: for benchmarks, not for serving. */
int mi_ivfpq_search_stages_device(mi_ivfpq* h, const float* q_dev, int64_t nq, int32_t k, int32_t nprobe, int64_t* out_idx_dev,
                                  float* out_dist_dev, void* stream, float* out_table_ms, float* out_scan_ms);

/* Device-resident variant: q_dev [nq][d] row-major f32 (C order), outputs are device buffers.
 * out_score64_dev (may be NULL) receives the float64 exact scores. */
int mi_knn_search_device(mi_gallery* g, const float* q_dev, int64_t nq, int32_t k,
                         int64_t* out_idx_dev, float* out_score_dev, double* out_score64_dev,
                         void* stream);

/* Asynchronous tail (mi_set_option "async_tail" = 1): mi_knn_search_device enqueues the scoring / filtering part of a batch
 * on `stream` and the exact re-score + sort on a stream of the handle, so that the tail of batch i runs beside the scoring
 * launch of batch i + 1 (the MFMA kernel leaves exactly the registers one re-score wave per SIMD needs and no LDS).  The
 * outputs of every call made so far are complete, in the order of `stream`, after mi_search_join(g, stream).  Default off:
 * outputs are then complete in stream order when mi_knn_search_device returns, as before.
 * "async_tail" = 3 (deferred): the tail of a batch of > 128 queries is not enqueued by its own call but by the NEXT
 * mi_knn_search_device call on the handle, after that batch's query ingest / bootstrap / threshold launches and right before
 * its scoring launch (or by mi_search_join, or by any call that cannot carry it on): the re-score gather then shares the
 * device with the power-bound scoring launch only.  The output buffers of a call must stay valid until the join. */
int mi_search_join(mi_gallery* g, void* stream);

/* Sharded search = phase 1 on every shard, all-gather of approx top-k values, phase 2, all-gather of
 * exact (score64, idx), merge.  New functionality (the reference is single-process).
 * phase 1: bf16 MFMA scoring + survivor filtering; writes the shard's k largest approximate scores
 *          (unsorted) to out_approx_dev [nq][k] (-inf padded when the shard has < k rows). */
int mi_knn_phase1_device(mi_gallery* g, const float* q_dev, int64_t nq, int32_t k,
                         float* out_approx_dev, void* stream);
/* K-th largest of the gathered [nshards][nq][k] approximate values -> lower bound L [nq].  The order is that of the
 * selection keys: NaN below -inf, -0.0 below +0.0, otherwise numeric; the answer is one of the gathered values, bit for bit
 * (some NaN when the K-th is a NaN).  nq >= 1, k >= 1, nshards >= 1 and nshards * k <= 8192, refused otherwise. */
int mi_kth_of_gathered_device(const float* gathered_dev, int32_t nshards, int64_t nq, int32_t k,
                              float* out_L_dev, void* stream);
/* phase 2: exact f64 re-score of every local row whose approximate score is within the rigorous error
 *          margin of L; emits the shard's exact top-k (score64 desc, idx asc), -inf/-1 padded. */
int mi_knn_phase2_device(mi_gallery* g, int64_t nq, int32_t k, const float* L_dev,
                         int64_t* out_idx_dev, float* out_score_dev, double* out_score64_dev,
                         void* stream);
/* merge of [nshards][nq][k] exact lists -> [nq][k] by (score64 desc, idx asc).  Every list must be what phase 2 emits:
 * sorted in that order, padded with -1 / -inf at the end; row ids of different shards are disjoint (row shards).
 * The order in full: an entry with idx < 0 is padding whatever its score and comes after everything; among the others a NaN
 * score comes after every number (-inf included), NaNs among themselves by ascending idx; numbers by descending score with
 * -0.0 == +0.0, equal scores by ascending idx -- across the lists as within one.  out_score is (float)score64 (a value beyond
 * the float32 range becomes +-inf), may be NULL; slots beyond the valid entries of all lists together hold -1 / -inf.
 * nq >= 1, k >= 1, nshards >= 1 and nshards * k <= 8192, refused otherwise. */
int mi_topk_merge_device(const double* score64_dev, const int64_t* idx_dev, int32_t nshards,
                         int64_t nq, int32_t k, int64_t* out_idx_dev, float* out_score_dev,
                         void* stream);
/* Same merge for lists that arrive interleaved per shard: shard g's scores start at score64_dev + g * shard_stride and its
 * indices at idx_dev + g * shard_stride (elements of 8 bytes), e.g. one all-gather of a packed [2][nq][k] buffer per rank
 * (scores, then indices) instead of two collectives.  shard_stride >= nq * k; what lies between the lists is not read. */
int mi_topk_merge_strided_device(const double* score64_dev, const int64_t* idx_dev, int64_t shard_stride,
                                 int32_t nshards, int64_t nq, int32_t k, int64_t* out_idx_dev,
                                 float* out_score_dev, void* stream);

/* ---- alpha query expansion: replaces feature_enhancement (src/utils/Reranking.py:195-208, copy at
 * :288-301): q' = sum_j ((k-j)/k)^w * G[ranks[j,q]], q' /= (||q'|| + eps), then a full re-search.
 * ranks: element (j,q) at ranks[j*rank_stride_j + q*rank_stride_q], global row ids (int64).
 * partial: this shard's contribution sum (rows it owns) as f64 [nq][d]; finish: normalise the
 * (all-reduced) sum into f32 queries [nq][d] (out_q64_dev, may be NULL: the same in f64 before the conversion; an all-zero
 * row stays zero for eps > 0); nq >= 1 and d >= 1, refused otherwise. */
int mi_aqe_partial_device(mi_gallery* g, const int64_t* ranks_dev, int64_t rank_stride_j,
                          int64_t rank_stride_q, int64_t nq, int32_t k_qe, double w,
                          double* out_sum_dev, void* stream);
/* Across shards (round 4; replaces the all-gather of f64 partial sums): `rows` writes, for every requested (j, q), the f32 row
 * this shard owns -- zeros when another shard owns it -- into out_rows_dev [k_qe][nq][d]; the blocks of all shards are SUMMED
 * (all-reduce: every element has exactly one non-zero contributor, so the sum is exact whatever order the collective adds
 * in; k_qe * nq * d * 4 bytes, 24 MiB at k_qe = 3, nq = 1024, d = 2048); `combine` adds the rows in j order with the
 * single-shard kernel's own weight and fused multiply-add -> the f64 sum [nq][d] of ONE gallery, bit for bit, independent of
 * the shard boundaries. */
int mi_aqe_rows_device(mi_gallery* g, const int64_t* ranks_dev, int64_t rank_stride_j, int64_t rank_stride_q, int64_t nq,
                       int32_t k_qe, float* out_rows_dev, void* stream);
int mi_aqe_combine_device(const float* rows_dev, int64_t nq, int32_t d, int32_t k_qe, double w, double* out_sum_dev,
                          void* stream);
int mi_aqe_finish_device(const double* sum_dev, int64_t nq, int32_t d, double eps, float* out_q_dev,
                         double* out_q64_dev, void* stream);
/* Host convenience (single shard): ranks host int64; out_qexp (may be NULL) f64 [nq][d]. */
int mi_aqe_search(mi_gallery* g, const int64_t* ranks, int64_t rank_stride_j, int64_t rank_stride_q,
                  int64_t nq, int32_t k_qe, double w, double eps, int32_t k, int64_t* out_idx,
                  float* out_score, double* out_qexp, double* out_seconds);

/* ---- dense exact kNN: faiss IndexFlatIP.search (src/utils/knn.py:25-31) when k is a large fraction of N (the kNN
 * graph of the diffusion, src/utils/diffusion.py:66).  Exact f32 inner products (k-ordered fmaf chain) of all
 * stored rows, top-k by (score desc, idx asc), k <= 4096. */
int mi_knn_dense_search(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride,
                        int64_t col_stride, int32_t k, int64_t* out_idx, float* out_score,
                        double* out_seconds);
/* The same at full precision and with no threshold logic at all: EVERY score of the gallery in float64 (f32 stored rows,
 * exact f64 products, f64 accumulation -- the arithmetic of the certificate's re-score) into a dense [queries, N] matrix,
 * then the exact top-k of it by (score desc, idx asc), k <= 4096.  The last resort of mi_knn_search on massively tied
 * data, and the INDEPENDENT checker of the filtered path at full size: whatever the filter, thresholds or candidate
 * buffers did, the two answers must agree (tests/test_gpu_full_size.py, bench.py `score_check`).  Replaces the full
 * argsort of src/utils/nnsearch.py:701-703 as the definition of "nothing is missing".  out_score / out_score64 may be NULL. */
int mi_knn_dense64_search(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride,
                          int64_t col_stride, int32_t k, int64_t* out_idx, float* out_score,
                          double* out_score64, double* out_seconds);

/* ---- full-length ranking: `np.argsort(-scores, axis=0)` over ALL rows (src/main_retrieve.py:176,
 * src/utils/Reranking.py:207; --mode mAP of src/test_rOP1m.py:144-149).  Exact f32 inner products, stable radix sort:
 * out_idx [nq][n] (score desc, idx asc, NaN last), out_score [nq][n] (may be NULL).  query_norm: -1 = normalise the
 * queries like the gallery, otherwise an mi_norm value (MI_NORM_NONE for an already expanded query). */
int mi_rank_all(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride,
                int query_norm, int64_t* out_idx, float* out_score, double* out_seconds);
/* The first `keep` columns of that ranking only ([nq, keep] outputs): K beyond the top-K path's limit without [nq, N] host
 * arrays (matching_HIP with 2048 < K < N). */
int mi_rank_prefix(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride,
                   int query_norm, int64_t keep, int64_t* out_idx, float* out_score, double* out_seconds);
/* Zero-based positions, in that same full ranking, of m listed rows per query (row_ids [nq, m], global ids, entries
 * outside the shard -> -1), computed by counting on the device: what compute_map2 needs of `ranks_aqe` [N, Q]
 * (src/utils/Reranking.py:280-283, src/utils/evaluate2.py:73-86) without the [N, Q] array.  m <= 2048. */
int mi_rank_positions(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride,
                      int query_norm, const int64_t* row_ids, int32_t m, int64_t* out_pos);

/* ---- k-reciprocal re-ranking: kr_reranking(qvecs, vecs) of src/utils/Reranking.py:447-624 (k1 = 20, k2 = 6,
 * lambda = 0.3 there).  qvecs [nq, d], vecs [n, d] host arrays (element strides; the reference takes the [d, .] arrays and
 * transposes), rows assumed L2-normalised like the reference assumes.  out_idx [nq, n]: gallery indices by ascending final
 * distance (= the reference's returned `indices`); out_dist (may be NULL): those distances.  nq + n <= 32768. */
int mi_kr_rerank(const void* qvecs, int64_t nq, int64_t q_row_stride, int64_t q_col_stride, const void* vecs, int64_t n,
                 int64_t v_row_stride, int64_t v_col_stride, int32_t d, int dtype, int32_t k1, int32_t k2,
                 double lambda_value, int device, int64_t* out_idx, float* out_dist);

/* ---- truncated graph diffusion: Diffusion.get_offline_results (src/utils/diffusion.py:52-84 with :15-19, :87-116)
 * on a MI_NORM_NONE gallery of the features.  out_ids [n][n_trunc] (the kNN lists = columns of the sparse
 * `offline` matrix), out_vals [n][n_trunc] f32 (its values), out_knn_sims (may be NULL).  The result also stays
 * on the device for mi_diffusion_online. */
int mi_diffusion_offline(mi_gallery* g, int32_t n_trunc, int32_t kd, double alpha, int32_t gamma,
                         int32_t maxiter, double tol, int64_t* out_ids, float* out_vals, float* out_knn_sims);
/* The same for the nodes [node0, node1) only (the N truncated CG solves of src/utils/diffusion.py:15-19 are
 * independent, so the ranks of a multi-GPU run each take a node range of the replicated feature set; the k-NN graph and
 * the Laplacian are computed in full on every rank).  out_ids [n][n_trunc] as above; out_vals [node1 - node0][n_trunc] =
 * those rows of the offline matrix.  Gather the parts and install them with mi_diffusion_set_offline. */
int mi_diffusion_offline_nodes(mi_gallery* g, int32_t n_trunc, int32_t kd, double alpha, int32_t gamma,
                               int32_t maxiter, double tol, int64_t node0, int64_t node1, int64_t* out_ids,
                               float* out_vals, float* out_knn_sims);
/* Re-installs a cached offline result (the reference caches it as offline.jbl, src/utils/diffusion.py:21-40).  Every id
 * lies in [0, N) and no row lists an id twice (MI_ERR_INVALID otherwise). */
int mi_diffusion_set_offline(mi_gallery* g, const int64_t* ids, const float* vals, int32_t n_trunc);
/* Online stage (src/utils/Reranking.py:238-253): top-k_query neighbours of each query, sims**gamma, weighted sum of
 * their offline rows, top-`trunc` ranks [nq][trunc] (score desc, idx asc) and scores.  q: nq x d strided host array, f32 | f64,
 * used as given (not normalised); the query ingest is mi_knn_search's, so f64 queries are rounded to f32. */
int mi_diffusion_online(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride,
                        int64_t col_stride, int32_t k_query, int32_t gamma, int32_t trunc,
                        int64_t* out_ranks, float* out_scores);

/* ---- descriptor tail of the extractor (src/networks/imageretrievalnet.py:183-187, 464-479; src/layers/functional.py:
 * 20-22, 129-130): GeM pooling of the last feature map feat[b][c][hw] (p, eps), L2N (eps 1e-6), optional whitening
 * Linear(c -> c_out, bias) + L2N (scratch_dev: [b][c] floats; c <= 4968 with whitening, the layer keeps 8 rows of c floats in
 * LDS), into out_dev [b][c_out or c].  The stream belongs to the current device.  Multi-scale: accumulate
 * desc^msp per scale (first != 0 overwrites), then finish = (acc / nscales)^(1/msp) / ||.||. */
int mi_desc_tail_device(const float* feat_dev, int32_t b, int32_t c, int32_t hw, float p, float eps,
                        const float* whiten_w_dev, const float* whiten_b_dev, int32_t c_out, float* scratch_dev,
                        float* out_dev, void* stream);
int mi_desc_ms_accumulate_device(float* acc_dev, const float* desc_dev, int64_t count, float msp, int first,
                                 void* stream);
int mi_desc_ms_finish_device(float* acc_dev, int32_t b, int32_t d, int32_t nscales, float msp, void* stream);

/* ---- building blocks of average_query_expansion / database_augmentation (src/utils/Reranking.py:314-432):
 * out_sum[q][:] = sum_j weights[j] * row(ranks[j,q]) in float64 (means / logspace-weighted sums of neighbours), and
 * column sums of a strided matrix (the centring step).  mi_column_sum / mi_column_sum_device: X f32 | f64, any strides; every
 * element is promoted to float64 and summed in float64 -- MI_F64 input is never rounded to float32. */
int mi_gather_weighted(mi_gallery* g, const int64_t* ranks, int64_t rank_stride_j, int64_t rank_stride_q, int64_t nq,
                       int32_t k, const double* weights, double* out_sum);
int mi_column_sum(const void* X, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride, int device,
                  double* out);

/* ---- whitenapply (src/utils/whiten.py:4-12): out[n][dims] = P[:dims] (x_n - m), rows divided by (||.|| + eps)
 * (eps < 0: no normalisation).  X: n images x d, strided (the reference's [D,N] array is passed with
 * row_stride 1, col_stride N); m f64 [d]; P f64 row-major [dims][d] (the first dims rows of the reference's P).
 * float64 arithmetic like the reference. */
int mi_whiten_apply(const void* X, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride,
                    const double* m, const double* P, int32_t dims, double eps, int device, double* out);

/* The same on device-resident operands, enqueued on `stream` without synchronising: X_dev strided f32 | f64, m_dev f64 [d],
 * P_dev f64 row-major [>= dims][d], out_dev f64 [n][dims] (un-normalised when eps < 0).  An f64 GEMM of 2 * dims * d flop per
 * image on v_mfma_f64_16x16x4_f64 (csrc/whiten.hip); the centring is applied while X is loaded. */
int mi_whiten_apply_device(const void* X_dev, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride,
                           const double* m_dev, const double* P_dev, int32_t dims, double eps, double* out_dev, void* stream);
/* ---- learning a whitening (src/utils/whiten.py:14-48 pcawhitenlearn / whitenlearn): the scatter matrix in front of the
 * D x D factorisation, float64 on v_mfma_f64_16x16x4_f64 (csrc/scatter.hip).
 *   rows mode  (pair_q == pair_p == NULL):  C (+)= sum_n (x_n - centre)(x_n - centre)^T over the n rows of X
 *   pairs mode (both given, n_pairs >= 1):  C (+)= sum_i (x_{q_i} - x_{p_i})(x_{q_i} - x_{p_i})^T; `centre` is ignored
 * X: n images x d, strided like mi_whiten_apply (f32 | f64, promoted and centred in float64 while it is loaded); centre f64
 * [d] or NULL (= 0); C f64 row-major [d][d], symmetric bit for bit (only tiles on or above the diagonal are multiplied, the
 * rest is mirrored); accumulate != 0 adds onto the C already there.  The row reduction is split over workgroups and combined
 * in a fixed order through a workspace: two calls on the same input return the same bits.  d <= 11520.
 * mi_scatter_workspace_bytes: bytes of device workspace one call needs for dimension d (a function of d alone, at most
 * 512 MiB; 272 MiB at d = 2048).  mi_column_sum_device: device twin of mi_column_sum (out_dev f64 [d]), for the mean. */
int mi_scatter_workspace_bytes(int32_t d, int64_t* bytes);
int mi_column_sum_device(const void* X_dev, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride,
                         double* out_dev, void* stream);
/* Device operands, enqueued on `stream` without synchronising.  Pair indices (int64, device) outside [0, n) are clamped: a
 * bad index costs a wrong number, never an access outside X. */
int mi_scatter_matrix_device(const void* X_dev, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride,
                             const double* centre_dev, const int64_t* pair_q_dev, const int64_t* pair_p_dev, int64_t n_pairs,
                             double* C_dev, int accumulate, void* workspace_dev, int64_t workspace_bytes, void* stream);
/* Host arrays in, host matrix out; synchronous.  X is never staged whole: row blocks (global option "scatter_block_rows",
 * default 64 MiB each) travel through two pinned buffers, the copy of block b + 1 under the kernel of block b.  In pairs
 * mode only the rows the pairs name are moved; a pair index outside [0, n) is MI_ERR_INVALID. */
int mi_scatter_matrix(const void* X, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride,
                      const double* centre, const int64_t* pair_q, const int64_t* pair_p, int64_t n_pairs, int device,
                      double* C_out);
/* Scatter matrix of the rows a gallery stores (after its normalisation), about `centre` (host f64 [d] or NULL): PCA whitening
 * learned from a prepared-gallery file.  Read-only on the handle, like mi_gallery_get_rows. */
int mi_gallery_scatter(const mi_gallery* g, const double* centre, double* C_out);

/* Learned whitening straight into an appendable gallery (mi_gallery_create_empty with d = dims and MI_NORM_L2_EPS, whose
 * normalisation IS whitenapply's tail `X / (norm + 1e-6)`, src/utils/whiten.py:10): m device rows are whitened in chunks of
 * 32 768 rows into one float64 scratch block and ingested from there -- the [N, dims] float64 matrix that
 * src/main_train.py:711-712 holds never exists.  Rows of P applied = the gallery's dimension.  Synchronises `stream` before
 * it returns (the scratch block is freed); appends and searches on one handle must be serialised by the caller. */
int mi_gallery_append_whitened_device(mi_gallery* g, const void* X_dev, int64_t m, int32_t d, int dtype, int64_t row_stride,
                                      int64_t col_stride, const double* mean_dev, const double* P_dev, void* stream);

/* ---- agreement between the shards of one gallery (multi-GPU).  The exactness certificate keeps every row
 * whose approximate score is within 2*eps of the K-th largest approximate score L of the WHOLE gallery; eps is derived
 * from the norm maxima measured at ingest {max ||g||, max ||g_hat||, max ||g_hat - g||} and from the image element type.
 * A row on shard B is only guaranteed approx >= L - eps_A - eps_B when the rows at L sit on shard A, so every shard must
 * use the maxima over ALL shards and the same image type: all-reduce(MAX) the bounds, all-reduce(MIN) the type, write
 * them back (sharded.ShardedGallery does this on construction). */
int mi_gallery_norm_bounds(mi_gallery* g, float* bounds3 /* in-out */, int raise);  /* raise=0: read; 1: bounds = max(own, given) */
int mi_gallery_set_image_dtype(mi_gallery* g, int f16);  /* re-images the stored f32 rows (1 = fp16, 0 = bf16); no-op if equal */

/* The eight XCDs of one MI355X hold different clocks under the same load, so the tile kernel splits the gallery tiles over
 * them by their MEASURED speed (option "xcc_balance"); the shares start equal and converge over the first ~4 large launches
 * of a handle (finish times spread by 2-3 % until then).  mi_gallery_calibrate runs `launches` (<= 64; 8 is plenty) scoring
 * launches of up to 1024 of the gallery's own rows against the whole gallery on `stream`, asynchronously, and discards the
 * answers: the shares are converged before the first real search instead of during it.  No-op for galleries of < 512 tiles
 * (131 072 rows).  One-off cost: `launches` x one batch (27 ms for 8 launches at 1 M x 2048 rows).  Clears the sticky flags
 * (read them first if asynchronous searches are outstanding). */
int mi_gallery_calibrate(mi_gallery* g, int32_t launches, void* stream);

/* ---- status / instrumentation */
typedef struct mi_search_stats {
  int64_t searches;           /* query batches processed */
  int64_t queries;
  int64_t overflow_batches;   /* batches whose candidate / survivor / record buffers overflowed (or whose queries left fp16's range):
                               * answered again through the f32 scorer, then the dense f64 path */
  int64_t survivors;          /* sum over queries of entries kept by the filter */
  int64_t candidates;         /* sum over queries of rows re-scored exactly */
  double gemm_ms;             /* HIP-event time of the MFMA scoring launches (profiling on) */
  int64_t gemm_launches;
  double gemm_flops;          /* algorithmic 2*Q*N*D of those launches */
  double gemm_bytes;          /* algorithmic gallery + query bytes of those launches */
  double kernel_clock_mhz;    /* shader clock inside the most recent tile-kernel launch (s_memtime / s_memrealtime around its
                               * main loop, median over waves); 0 if that kernel has not run.  The chip lowers its clock under
                               * MFMA load, so this is what the dense peak scales with */
  int64_t spec_retries;       /* batches whose speculative threshold failed its verification (and, where a device repair pass ran,
                               * that too): answered again by the rigorous chunk schedule.  Not an overflow */
  int64_t inkernel_repairs;   /* queries of batches of <= 128 queries on the asynchronous (device / phase) entry points whose
                               * speculative threshold failed and that were repaired INSIDE the maintain launch: the query's workgroup
                               * rescans the whole shard (~0.1 s per 1 M rows x 2048, over 1 s on a 10 M-row shard; expected once per
                               * ~10^7 queries).  The answer is complete; this counter is the only trace of why that call was slow */
} mi_search_stats;
int mi_profile_enable(mi_gallery* g, int on);      /* times the scoring launches with HIP events (dispatch timestamps) */
int mi_search_status(mi_gallery* g, mi_search_stats* out, int reset); /* synchronises the handle's work */
/* The durations (ms, launch order) of the timed scoring launches since the last mi_search_status(reset = 1): what gemm_ms is
 * the sum of.  Waits for the launches enqueued so far; writes min(count, cap) values, *out_count = launches logged. */
int mi_profile_launch_ms(mi_gallery* g, float* out_host, int64_t cap, int64_t* out_count);
/* Tunables (22 names; everything that was an A/B switch of a measured-and-rejected variant -- "debug", "kernel_variant",
 * "small_tail", "stream_lookahead", "inkernel_repair_max", "ladder" = 2 -- left the product in round 5: MI_ERR_INVALID):
 * "chunk0_tiles" (rows / 256 of the bootstrap chunk and of the threshold sample; 0 = default 32), "chunk_growth",
 * "workspace_slot" (0 | 1: which of the handle's two per-batch workspaces the phase API uses -- phase 1 of batch i + 1 may
 * be enqueued before phase 2 of batch i; sticky flags and statistics are one set for both),
 * "spec_max_ratio" (largest shard rows / sample rows for which the single-launch sample schedule is taken; default 160),
 * "survivor_cap", "rescore_cap", "exact_fallback" (0 = report MI_ERR_OVERFLOW instead of falling back to the f32 scorer and
 * then the dense f64 path), "ladder" (in-launch threshold ladder of the tile kernel: 0 = off, 1 = on (default)),
 * "boot_ksplit" (batches of <= 512 queries: the bootstrap launch
 * on the sample splits K over several workgroups that add their partial scores with float atomics; default 1.  The order of
 * those adds is not fixed, so the sample scores -- and with them the survivor / candidate statistics and which queries need a
 * repair -- may differ by an ulp from run to run; the answers do not: the threshold is speculative and verified), "xcc_balance" (XCD shares by measured
 * speed), "stream_tail" (default 1: a HOST entry point called with more than 1024 queries runs its internal batches with the
 * deferred tail of "async_tail" 3 and reads the sticky flags once at the end; 0 = one verified batch after the other),
 * "async_tail" (1 | 2 | 3: re-score + sort on the handle's own stream beside the next batch's scoring launch | beside its
 * query ingest and bootstrap only | deferred: enqueued by the next call right before its scoring launch; see mi_search_join), "rescore_grid_x" (workgroups of 2
 * candidates per query in the re-score launch; 0 = 64; a shard of a G-way gallery sets ~96 / G),
 * "force_exact" (score with the f32 kernel instead of the 16-bit MFMA), "speculative" (0 = rigorous chunk schedule only),
 * "device_repair" (-1 = default: the scoring launch of a batch of > 128 queries is followed by a device-conditional repair
 * pass for queries whose speculative threshold failed verification; smaller batches launch none: through a HOST entry point
 * the sticky flag makes the call answer the batch again, through the asynchronous device / phase entry points the workgroup
 * of the failed query repairs it inside the maintain launch (a scan of the shard's rows, ~0.1 s per million -- over a second
 * on a 10 M-row shard --, once per 10^7 queries; counted in mi_search_stats.inkernel_repairs), so their answers are complete
 * without anybody reading flags; 0 / 1 = never / always launch the repair pass),
 * "small_batch_kernel" (0 = batches of <= 128 queries use the 256 x 256-tile kernel too),
 * "query_norm_override" (-1 | mi_norm: how the _device entry points normalise their queries; MI_NORM_NONE for the
 * already normalised expanded queries of alpha-QE),
 * "filter_path" (mi_knn_search_filtered: 0 = auto (default), 1 = always the compacted sub-gallery, 2 = always the over-fetch;
 * a forced over-fetch still answers the queries it cannot certify by path 1), "filter_compact_max" (auto compacts at
 * selectivity <= this, whenever fewer than k rows are allowed, whenever the bitmap equals the one the stored sub-gallery
 * was built from, and -- not all rows allowed -- whenever it equals the previous call's; default 0.15, the crossover of first
 * calls at 1 and 70 queries measured in DESIGN.md 5.10), "filter_cache" (1 = keep the compacted
 * sub-gallery for the next call with an equal bitmap (default); 0 = free it now and at the end of every call, and do not
 * compact a bitmap only because it came twice; a kept sub-gallery holds up to 12 KB of HBM per allowed row at D = 2048),
 * "group_path" (mi_knn_search_grouped: 0 = auto (default: the over-fetch, and the dense fallback for what it cannot certify),
 * 1 = the dense fallback for every query, 2 = always the over-fetch, which still re-runs what it cannot certify).
 * mi_get_option also answers "image_dtype" (1 = fp16, 0 = bf16; read-only, see mi_gallery_set_image_dtype),
 * "sample_rows" (rows of the threshold sample in effect) and "metric" (an mi_metric value; read-only). */
int mi_set_option(mi_gallery* g, const char* name, double value);
int mi_get_option(const mi_gallery* g, const char* name, double* out_value);   /* same names as mi_set_option */
/* Synchronises the handle's work, returns the sticky device flags raised by the asynchronous _device entry points since
 * the last call (0 = none; any bit = that batch must be answered again: buffer overflow, failed speculative threshold, or a
 * query left with fewer than k candidates because NaN scores -- zero rows or queries under MI_NORM_L2 -- belong in its top k)
 * and clears them.  Unlike mi_search_status it leaves the statistics accumulators alone. */
int mi_search_flags(mi_gallery* g, uint32_t* out_flags);

/* Process-wide defaults for galleries created afterwards.  "image_dtype": element type of the 16-bit tile-blocked image the
 * MFMA kernel streams, 1 = fp16 (default: 2^-11 rounding, 8x tighter certificate than bf16 at the same MFMA rate;
 * un-normalised galleries whose rows exceed its comfortable range are stored as bf16 automatically), 0 = bf16.
 * "host_ingest": how mi_gallery_create moves a HOST array in one of the reference's two layouts to the device: 1 (default) = row
 * blocks of ~32 MiB copied by the runtime straight from the caller's pageable array into two alternating device blocks, the copy
 * of block i + 1 under the ingest of block i, no staging allocation the size of the gallery; 0 = one copy of the whole array into
 * a same-size staging buffer, then one ingest (rounds 1-4).  Both reach 0.96 of the pinned H2D rate (profiles/r05f_*).
 * "keep_buffers": 1 (default) = mi_gallery_destroy keeps the buffers of a gallery of up to 16 GiB and its search workspace (one
 * carved allocation of ~200 MB) in one spare slot each per process, and the next gallery of exactly the same sizes on the same
 * device takes them instead of allocating: a caller that prepares a gallery per call (create, search, destroy: a stateless
 * matching_<method>, src/utils/nnsearch.py:687-706) stops paying 1-6 ms of hipMalloc / hipFree per 12 GB and ~4 ms for the
 * workspace; 0 = free the spares now and keep nothing.
 * "remove_block_rows": upper limit B of the rows of the staging area mi_gallery_remove_rows moves the surviving rows through
 * (rounded up to a multiple of 256; 0 = default, 32 768 -- a first choice, not yet taken from a measured sweep).  The call uses
 * fewer rows when fewer move, and gives up whole tiles of 256 rows so that the allocation, as the driver rounds it, stays within
 * B * (6 * d64 + 12) bytes + 4 bytes per surviving row + the bitmap + 1 MiB.
 * "pq_remove_block_rows": upper limit B of the rows mi_pq_remove_rows moves through its staging area at a time (B * 4 * ceil(m / 4)
 * bytes; at least 64, rounded up to a multiple of 64; 0 = default, 2 097 152 -- a first choice, not taken from a sweep; a value
 * in (0, 64) or below 0 is MI_ERR_INVALID).  The result does not depend on it.  mi_ivfpq_remove_rows has no staging area.
 * "hamming_matrix_bytes": upper limit of the distance matrix of a binary index (mi_hamming_search*; 0 = default, 2 GiB).
 * "hamming_range_bytes": upper limit of the (block, query) workspace of a radius search on a binary index
 * (mi_hamming_range_search*, mi_hamming_self_range; 0 = default, 1 GiB; 64 queries at the least).  The result does not depend on it.
 * "minkowski_range_bytes": upper limit of the float64 values and counts of one chunk of queries of a Minkowski radius search
 * (mi_range_search_minkowski*, mi_minkowski_self_range; 0 = default, 256 MiB; one scan tile of queries -- 8 at d <= 2560 -- at the
 * least).  The result does not depend on it.
 * "hamming_range_early_exit": 1 (default) = the radius scan drops a (block, query) pair as soon as the partial distances of all
 * 64 rows exceed the radius; 0 = every pair is scanned to the last word.  The result does not depend on it.
 * "pq_matrix_bytes": upper limit of the distance matrix of a PQ index (mi_pq_search*; 0 = default, 2 GiB) and of the partial
 * lists of an IVF-PQ index (mi_ivfpq_search*).
 * "group_overfetch": the factor f of the over-fetch depth K' = min(2048, n, f k + 32) of mi_knn_search_grouped (1 .. 2048; 0 =
 * default, 4 -- a placeholder, not taken from a measurement yet).  "group_dense_bytes": upper limit of the float64 scores and group
 * tables of one sub-batch of its dense fallback (0 = default, 1 GiB; one query at the least).  The result depends on neither. */
int mi_set_global_option(const char* name, double value);
/* "release_spares" (any value) gives the spare slots back now and leaves "keep_buffers" as it is.  An allocation of the library
 * that fails with out-of-memory releases them by itself and is tried once more; a gallery of other sizes than the spare releases
 * it when the device could not hold both.  mi_get_global_option reads "image_dtype", "host_ingest", "keep_buffers", "scatter_block_rows",
 * "remove_block_rows", "pq_remove_block_rows", "hamming_matrix_bytes", "hamming_range_bytes", "minkowski_range_bytes", "hamming_range_early_exit", "pq_matrix_bytes", "group_overfetch", "group_dense_bytes" and "spare_bytes": the device memory the process holds in the spare slots right now -- what a co-tenant of the GPU (the
 * extractor's PyTorch allocator) cannot see otherwise. */
int mi_get_global_option(const char* name, double* out_value);

/* ---- the online chain behind one coalescing front: replaces the body of the Flask route of src/online.py:108-163 (threaded
 * server, every request thread searches on module-level globals) minus the CNN: search (K nearest by cosine on g_search,
 * src/online.py:124-131) -> qge1 expansion from the first k_qe rows as stored in g_rows (src/utils/Reranking.py:195-208; the
 * route uses k_qe = 3, w = 4, src/online.py:148) -> re-search of g_rows with the expanded query as it is.  g_rows = NULL: the
 * plain search.  A launch of <= 128 queries costs what a launch of one does, so concurrent callers of mi_online_query are
 * answered TOGETHER: they block inside the call (a Python host's request threads: outside the interpreter lock) while one
 * worker thread of the handle drains the waiting descriptors -- up to max_batch rows -- into one chain and hands every caller
 * its rows.  The worker waits -- at most until max_wait_us after it handed out the previous chain -- for as many requests as
 * callers were around then (answered + queued): the callers just answered are on their way back, and two half crowds taking
 * turns are half the throughput of one; a lone sequential caller never waits, nor does anyone after an idle period.  Every chain runs the verified
 * loop of the host entry points (sticky flags read, f32 scorer / dense float64 fallbacks), so the answers are those of
 * sequential mi_knn_search + mi_aqe_search calls bit for bit.  The galleries must outlive the handle (mi_gallery_destroy
 * refuses a gallery an online handle is built on) and share device, dimension and rows; other threads may keep using them
 * (the chain takes their locks). */
typedef struct mi_online mi_online;
int mi_online_create(mi_gallery* g_search, mi_gallery* g_rows, int32_t k, int32_t k_qe, double w, double eps,
                     int32_t max_batch /*1..1024, 128: the streaming kernel's limit*/, int32_t max_wait_us, mi_online** out);
/* desc: nq <= max_batch descriptors [nq][d] f32, host or device memory.  pending != 0 (device descriptors only): they are still
 * being produced on producer_stream (NULL = the null stream) -- an event is recorded there and the chain waits for it on the
 * device; pending = 0: they are complete.  Blocks until the chain that carried the request is done; out_idx [nq][k] int64 (global row ids) and out_score [nq][k] f32 (may be NULL) are HOST arrays.
 * A failed chain fails every request it carried, with the chain's message on each caller's thread (mi_last_error). */
int mi_online_query(mi_online* o, const float* desc, int32_t nq, int memspace, int pending, void* producer_stream,
                    int64_t* out_idx, float* out_score);
int mi_online_stats(mi_online* o, int64_t* out_chains, int64_t* out_requests);
/* Answers what is still queued, stops the worker, frees the handle (not the galleries). */
int mi_online_destroy(mi_online* o);

/* The XCD shares of the tile kernel (relative speeds of the eight XCD labels, summing to 1) as the handle's launches have left
 * them, and how many launches have updated them since the workspace was created (-1: no workspace yet; the values are then what
 * the first one will start from).  The shares are saved with the prepared-gallery file (optional trailer) and remembered per
 * device inside the process, so `load -> first search` and a second gallery of a process start calibrated. */
int mi_debug_xcc_shares(mi_gallery* g, float* out_w8, int32_t* out_launches);
/* Diagnostics / bench only: `threads` request threads of the library itself in a closed loop of per_thread requests each (request
 * i of thread t = descriptor (t + i) mod n_desc of desc_dev [n_desc][d], complete) -- what the coalescing front sustains when
 * the host's request threads are not serialised by an interpreter lock.  out_last_idx [threads][k] host: every thread's last answer. */
int mi_debug_online_clients(mi_online* o, const float* desc_dev, int32_t n_desc, int32_t threads, int32_t per_thread,
                            int64_t* out_last_idx, double* out_seconds);
/* Diagnostics only: the per-wave words the tile kernel leaves behind, layout [workgroups * 8][8]: word 5 = K-slices done, word 6 =
 * shader cycles and word 7 = 10-ns ticks around the main loop (what kernel_clock_mhz and the XCD shares are computed from); word 3 =
 * records the wave emitted, word 4 = the XCC id it ran on; words 0-2 are not written. */
int mi_debug_read_cycles(mi_gallery* g, uint64_t* out_host, int64_t count);

/* Diagnostics only: the gallery row that sample row i of the bootstrap sample image is drawn from (shard of n rows, sample
 * of n_s rows: one hashed draw per stratum of n / n_s consecutive rows).  Tests use it to plant rows inside the sample. */
int64_t mi_debug_sample_source_row(int64_t i, int64_t n, int64_t n_s);

/* ---- synthetic data (bench / tests): device twin of synth.synth_rows. */
int mi_synth_fill_device(float* dst_dev, uint64_t seed, int64_t row0, int64_t nrows, int32_t d,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355_RETRIEVAL_H */
