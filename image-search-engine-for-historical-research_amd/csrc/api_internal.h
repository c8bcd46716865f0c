// Internals shared by the translation units of the C ABI (api_*.hip): the handle, its workspace, the process-wide state and
// the helpers more than one of them calls.  Nothing here is part of the public interface (include/mi355_retrieval.h).
//   api_state.hip     process-wide state (spare-buffer slots, XCD-share cache, global options), workspace allocation
//   api_schedule.hip  the search itself: phase 1 (plan / pre / main: sample schedule, chunk schedule, repair), phase 2, the
//                     asynchronous tails, the verified host loop with its fallbacks, the dense paths
//   api_gallery.hip   gallery life cycle: create / append / destroy, ingest of any layout, norm bounds, image type
//   api_file.hip      the prepared-gallery file (MI355GAL v2): save / load, parallel copies, checksums
//   api_entry.hip     search entry points: kNN (host / device / phases / merge), alpha-QE, dense, full-length ranking
//   api_aux.hip       descriptor tail, whitening, scatter matrix, k-reciprocal re-ranking, diffusion, column sums, synthetic rows
//   api_options.hip   per-handle options, statistics, profiling, flags, diagnostics
//   api_range.hip     exact range search: fixed-threshold chunk schedule, overflow split, dense chunks, CSR tail
//   api_filter.hip    filtered top-K: compacted sub-gallery (cached per bitmap) or over-fetch with a certificate
//   api_group.hip     grouped top-K (one row per group, one excluded group per query): labels on the handle, over-fetch with a
//                     certificate or the dense float64 fallback over the group CSR
//   api_l2.hip        squared-L2 metric: L2 galleries (hidden bias columns), top-K by distance (host / device), dense checker
//   api_refine.hip    exact re-ranking of index shortlists on the stored rows (mi_refine*): gather launch + per-query sort
//   api_remove.hip    row removal in place: keep-list, block-ordered move through a bounded staging area, invalidations
//   api_hamming.hip   binary index (mi_hamming): packed codes, exact Hamming top-K through a bounded uint16 distance matrix;
//                     radius search and self-join through one ballot per (block, query)
//   api_components.hip  connected components (mi_components): union-find over pair lists, self-join CSR output or the Hamming
//                     self-join's ballots (hamming_self_scan below), labels for mi_gallery_set_groups
//   api_pq.hip        PQ index (mi_pq): codebooks and byte codes, exact ADC top-K through a bounded float32 distance matrix
//   pq_flat.h         the host functions of both flat PQ indexes, templates over the handle (PqFlat<CodeT> below); api_pq.hip and
//                     api_pq_wide.hip forward their entry points to them
//   api_pq_train.hip  learning PQ codebooks (mi_pq_train, mi_pqw_train): deterministic Lloyd iterations on device-resident rows
//   api_pq_wide.hip   wide PQ index (mi_pqw): uint16 codes, Ks <= 8192, the books pass through LDS in groups (pq_wide.hip)
//   api_ivfpq.hip     IVF index over PQ codes (mi_ivfpq): coarse lists as chains of 64-slot blocks, exact ADC top-K over the probed lists
//                     (row removal of both PQ handles: mi_pq_remove_rows in api_pq.hip, mi_ivfpq_remove_rows here; kernels in pq_remove.hip)
//   api_lsh.hip       LSH codes (mi_lsh_encode*, mi_hamming_append_lsh_device): f64 projection to sign bits, fused (lsh.hip)
//   api_graph.hip     graph index (mi_graph): neighbour table over a gallery's rows, best-first search (graph_search.hip), table
//                     from exact nearest-neighbour lists (graph_build.hip); and what every graph index does with its table
//                     (graph_table_*, graph_*_check: the checks, create from a caller's table, the tail of a build, the getters)
//   api_pq_graph.hip  graph index over PQ codes (mi_pq_graph): neighbour table over the rows of a mi_pq index, best-first search on
//                     ADC distances (pq_graph_search.hip), table from the exhaustive ADC search of the decoded rows
//   api_forest.hip    random-projection forest (mi_forest): directions, split values and row permutations over a gallery's rows; f64
//                     projections of rows and queries by one kernel (forest_project.hip), level-wise build (forest_build.hip), descent
//                     into candidate slots (forest_search.hip), the answer by launch_refine
//   api_ivfflat.hip   IVF-Flat index (mi_ivfflat): centroids, list offsets and row lists over a gallery's raw rows; probe and assignment
//                     by launch_refine over the centroid table, list build, scan with selection and merge in ivfflat.hip
//   api_minkowski.hip exact L1 / L-infinity / Lp top-K over a gallery's raw rows (mi_knn_search_minkowski*): float64 scan of every
//                     row on the vector pipe, selection and merge in minkowski.hip
//   api_minkowski_range.hip  radius search and self-join in the same metrics (mi_range_search_minkowski*, mi_minkowski_self_range):
//                     the same scan, then count / offsets / emit / order / write-out in minkowski_range.hip, chunked by
//                     "minkowski_range_bytes"; mink_range_plan.h has the chunk arithmetic
// Device code shared between kernel files lives in headers of its own: l2_wave.h (squared-L2 wave arithmetic), pq_device.h (PQ index
// family), graph_walk.h (the best-first walk of both graph indexes), slab_select.h (sort, stream selection and emit on (key, id)
// entries in LDS: ivfflat.hip, minkowski.hip)
// The handles' grow-only device buffers own themselves: device_buf.h (DeviceBuf<T> and the per-handle DeviceBufSet; host code only);
// graph_table.h (GraphTable: the neighbour table and entry rows both graph handles hold)
#pragma once
#include "../../include/mi355_retrieval.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <sys/stat.h>
#include <unistd.h>

#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.h"
#include "kernels.h"

using namespace mi;

#define MI_INTERNAL __attribute__((visibility("hidden")))

// ---- process-wide state (defined in api_state.hip; the comments on what each is for are there)
extern MI_INTERNAL std::atomic<int> g_default_img_f16;
extern MI_INTERNAL std::atomic<int> g_host_ingest;
extern MI_INTERNAL std::mutex g_bal_mu;
extern MI_INTERNAL std::map<int, std::vector<float>> g_bal_cache;
struct SpareBuffers {
  int device = -1;
  size_t f32_bytes = 0, img_bytes = 0, stat_bytes = 0;
  float* gal_f32 = nullptr;
  void* gal_img = nullptr;
  RowStat* rowstat = nullptr;
  float* gstat3 = nullptr;
};
struct SpareArena {           // the search workspace of the handle destroyed last (one carved allocation, ~200 MB)
  int device = -1;
  size_t bytes = 0;
  void* p = nullptr;
};
extern MI_INTERNAL std::mutex g_spare_mu;
extern MI_INTERNAL SpareBuffers g_spare;
extern MI_INTERNAL SpareArena g_spare_ws;
extern MI_INTERNAL std::atomic<int> g_keep_buffers;
extern MI_INTERNAL std::atomic<int64_t> g_scatter_block_rows;   // mi_scatter_matrix: rows per host block (0 = 64 MiB)
extern MI_INTERNAL std::atomic<int64_t> g_remove_block_rows;    // mi_gallery_remove_rows: rows of the staging area (0 = default)
extern MI_INTERNAL std::atomic<int64_t> g_pq_remove_block_rows; // mi_pq_remove_rows: rows of the staging area (default 2 097 152)
extern MI_INTERNAL std::atomic<int64_t> g_hamming_matrix_bytes; // mi_hamming_search*: bytes of the distance matrix (default 2 GiB)
extern MI_INTERNAL std::atomic<int64_t> g_hamming_range_bytes;  // mi_hamming_range_search* / self_range: bytes of the (block, query) workspace (default 1 GiB)
extern MI_INTERNAL std::atomic<int64_t> g_minkowski_range_bytes; // mi_range_search_minkowski* / mi_minkowski_self_range: bytes of the value matrix and counts of a chunk (default 256 MiB)
extern MI_INTERNAL std::atomic<int> g_hamming_range_early_exit; // ... drop a (block, query) whose partial sums are all above the radius (default 1)
extern MI_INTERNAL std::atomic<int64_t> g_pq_matrix_bytes;      // mi_pq_search*: bytes of the distance matrix (default 2 GiB); mi_ivfpq_search*: of the partial lists
extern MI_INTERNAL std::atomic<int64_t> g_group_dense_bytes;    // mi_knn_search_grouped: bytes of the float64 scores and group tables of a fallback sub-batch (default 1 GiB)
extern MI_INTERNAL std::atomic<int> g_group_overfetch;          // mi_knn_search_grouped: f of the over-fetch depth K' = f k + 32 (default 4)
extern MI_INTERNAL std::atomic<int64_t> g_forest_build_bytes;   // mi_forest_build: bytes of the scratch of a group of trees (default 1 GiB)
constexpr size_t SPARE_MAX_BYTES = (size_t)16 << 30;
MI_INTERNAL void spare_release_locked();
MI_INTERNAL void spare_ws_release_locked();
MI_INTERNAL hipError_t device_malloc(void** p, size_t bytes);      // hipMalloc; out of memory: spares released, one more try
MI_INTERNAL int fail(int code, const std::string& msg);            // records the calling thread's error message, returns code
MI_INTERNAL const char* last_error_message();
#define HIPC(expr)                                                                                   \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess)                                                                            \
      return fail(_e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP,                             \
                  std::string(#expr) + ": " + hipGetErrorString(_e));                                \
  } while (0)
#define REQUIRE(cond, msg) \
  do {                     \
    if (!(cond)) return fail(MI_ERR_INVALID, msg); \
  } while (0)
#include "device_buf.h"   // DeviceBuf<T>, DeviceBufSet, grow_all
#include "graph_table.h"  // GraphTable
#include "group_plan.h"   // GroupPlan


// The host half of a row removal on a PQ or an IVF-PQ index (mi_pq_remove_rows, mi_ivfpq_remove_rows; defined in api_pq.hip): the
// caller's bitmap of the rows that leave (host or device, ceil(n / 64) words, bits at or beyond n ignored) -> the bitmap of the
// rows that STAY and the exclusive count of its bits per word, which is what the kernels of pq_remove.hip renumber by
struct RemovePlan {
  std::vector<uint64_t> keep;      // [ceil(n / 64)], bits at or beyond n clear
  std::vector<uint32_t> prefix;    // [ceil(n / 64) + 1], prefix.back() = n' = n - removed
  int64_t removed = 0, first = -1; // rows that leave; the lowest of them
};
MI_INTERNAL int remove_plan(const uint64_t* remove_bits, int memspace, int64_t n, RemovePlan* plan);


constexpr int QB = 1024;  // queries per batch (workspace size)

struct Workspace {
  int32_t qcap = 0, kcap = 0;
  uint32_t cap = 0, rcap = 0;
  float* q_f32 = nullptr;
  void* q_img = nullptr;
  RowStat* q_stat = nullptr;
  float *thr = nullptr, *margin = nullptr, *thr2 = nullptr;
  uint32_t* qflag = nullptr;
  float* lad_tc = nullptr;
  uint32_t *lad_pack = nullptr, *lad_cnt = nullptr;
  uint32_t* cnt = nullptr;
  uint64_t* surv = nullptr;
  uint32_t* flags = nullptr;
  uint32_t* repair = nullptr;       // this workspace's own 'repair needed' word (never aliased)
  float *topvals = nullptr, *L = nullptr;
  uint32_t *cand_rows = nullptr, *cand_cnt = nullptr;
  double* cand_score = nullptr;
  // second set of the buffers the tail of a search (exact re-score + emit) reads, for the asynchronous tail: the tail of
  // batch i runs on its own stream beside the scoring launch of batch i + 1, which refills the other set
  float* q_f32_set[2] = {nullptr, nullptr};
  uint32_t *cand_rows_set[2] = {nullptr, nullptr}, *cand_cnt_set[2] = {nullptr, nullptr};
  double* cand_score_set[2] = {nullptr, nullptr};
  uint64_t* stats2 = nullptr;
  SurvRec* rec = nullptr;
  uint32_t* rec_cnt = nullptr;
  unsigned long long* dbg = nullptr;
  XccBalance* bal = nullptr;      // measured XCD shares of the tile kernel (device memory)
  uint32_t rec_cap = 4096, nseg = 0;
  std::vector<void*> allocs;
  size_t arena_bytes = 0;   // allocs[0] is one carved allocation of this size on device arena_device (ws_ensure)
  int arena_device = -1;
};
struct TmpAlloc {
  std::vector<void*> v;
  ~TmpAlloc() { for (void* p : v) (void)hipFree(p); }
  template <typename T> T* get(size_t count) {
    void* p = nullptr;
    if (device_malloc(&p, count * sizeof(T) + 256) != hipSuccess) return nullptr;
    v.push_back(p);
    return reinterpret_cast<T*>(p);
  }
};
// ---- what mi_graph and mi_pq_graph do with their GraphTable (api_graph.hip).  `name` ("graph", "PQ graph") opens the messages.
// The caller holds the owner's lock wherever the owner's rows are read
constexpr size_t GRAPH_VIS_BYTES = (size_t)256 << 20;      // visited bitmaps of one launch: a batch that needs more goes in chunks
constexpr int64_t GRAPH_BUILD_BATCH = 8192;                // rows per exact search of a build
MI_INTERNAL int graph_search_check(const void* gr, int64_t nq, int32_t k, int32_t ef);
MI_INTERNAL int graph_create_check(const void* owner, const int32_t* neighbors, int32_t R, int neighbors_memspace,
                                   const int32_t* entries, int32_t ne, const void* out);
MI_INTERNAL int graph_build_check(const void* owner, int32_t R, int32_t ne, const void* out);
MI_INTERNAL int graph_build_rows_check(int64_t n);
MI_INTERNAL int graph_table_alloc(GraphTable& t, int64_t n, int32_t R, int32_t ne, const char* name);
// the caller's table (host or device) and entries over n >= 1 rows: checked, copied into `t`; on failure nothing stays allocated
MI_INTERNAL int graph_table_from_neighbors(GraphTable& t, int64_t n, int device, const char* name, const int32_t* neighbors, int32_t R,
                                           int neighbors_memspace, const int32_t* entries, int32_t ne);
// the workspace of a build besides the forward-list loop's own: forward lists, scratch, counts then fill cursors, offsets
struct GraphBuildWs {
  int32_t *F, *B;
  uint32_t* cnt;
  unsigned long long* off;
};
MI_INTERNAL GraphBuildWs graph_build_workspace(TmpAlloc& tmp, int64_t n, int32_t R);
// the tail of a build: t.adj from the forward lists ws.F, the evenly spaced entries; `s` is synchronised where it returns MI_OK
MI_INTERNAL int graph_table_finish(GraphTable& t, const GraphBuildWs& ws, TmpAlloc& tmp, const char* name, hipStream_t s);
MI_INTERNAL int graph_table_get_neighbors(const GraphTable& t, std::mutex& mu, int device, int64_t row0, int64_t nrows, int32_t* out_host);
MI_INTERNAL int graph_table_get_entries(const GraphTable& t, std::mutex& mu, int device, int32_t* out_host);
// visited bitmaps of a search of nq queries: words per query, queries per launch
struct GraphVisChunks { int64_t words, chunk; };
static inline GraphVisChunks graph_vis_chunks(int64_t n, int64_t nq) {
  const int64_t words = (n + 31) / 32;
  return {words, std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(GRAPH_VIS_BYTES / 4) / words))};
}
// what phase 1 of one batch will do (pure arithmetic on the shapes; plan_phase1)
struct P1Plan {
  int32_t nq = 0, k = 0, qpad = 0;
  bool exact = false;
  int64_t ntiles = 0, t0 = 0;
  int32_t samp_r = 0;              // > 0: single-launch schedule on the threshold sample, speculative rank
  uint32_t first_cnt = 0;
  float gamma = 0.f;
  int32_t boot_ksplit = 1;
  bool sample_f32 = false;         // the bootstrap launch stores bare 4-byte scores
  bool thr_kernel = false;         // sample_threshold_kernel takes the thresholds (else select_maintain mode 0)
  int32_t lad_r = 0;               // ladder level (sample rank), 0 = off
  bool zero_scores = false;        // the query ingest writes zeros for the K-split bootstrap to add onto
  bool samp_ext = false;           // the sample's scores go to the handle's own buffer (mi_gallery::samp_scores), not into survivor rows
};

struct mi_gallery {
  int device = 0;
  int64_t n = 0, npad = 0, row_offset = 0;
  int64_t cap = 0;          // allocated rows (== n unless created with mi_gallery_create_empty)
  int32_t d = 0, dp = 0, norm_mode = 0;
  // MI_METRIC_L2: `d` counts the three hidden bias columns behind the user's `ud` columns (d == ud + 3), so the
  // search below the entry points sees an ordinary raw gallery; what faces the caller (ingest, info, get_rows) uses `ud`
  int32_t ud = 0, metric = 0;
  int img_f16 = 1;          // 16-bit image element type of the gallery AND of the query batches searched on it
  float* gal_f32 = nullptr;
  void* gal_img = nullptr;
  RowStat* rowstat = nullptr;
  float* gstat3 = nullptr;
  // bootstrap sample image of the speculative schedule (built lazily, rebuilt when rows were appended)
  void* samp_img = nullptr;
  int64_t samp_tiles = 0, samp_for_n = -1;
  float* samp_f32 = nullptr;       // the 8192-row sample as stored f32 rows (built when the f32 scorer first needs its thresholds)
  int64_t samp_f32_for_n = -1, samp_f32_tiles = 0;
  float* samp_scores = nullptr;    // [QB][samp_tiles * 256] scores of a sample too large for a survivor row (shards beyond 3.9 M rows)
  int64_t samp_scores_tiles = 0;
  int64_t hbm_bytes = 0;
  size_t buf_bytes[3] = {0, 0, 0};                 // gal_f32 / gal_img / rowstat as allocated (what a spare slot is matched by)
  // XCD shares read from the prepared-gallery file (MI355GAL trailer) / snapshotted for the next save
  float file_w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool file_w_valid = false;
  hipStream_t stream = nullptr;
  Workspace ws;
  // option "workspace_slot": the phase API of batch i + 1 may run in the other workspace while batch i waits for its
  // collectives (sharded search, two batches in flight).  `ws` is always the active one; `ws_alt` the parked one.  The
  // sticky flags, the statistics, the kernel clocks and the XCD shares are ONE set: the second workspace aliases them.
  Workspace ws_alt;
  int ws_slot = 0;
  // options
  int chunk0_tiles = 0 /* 0 = default, bootstrap_tiles() */, chunk_growth = 8, exact_fallback = 1, force_exact = 0,
      speculative = 1, rescore_grid_x = 0, spec_max_ratio = 160;
  int device_repair = -1;       // -1 = by batch size (off for <= 128 queries), 0 / 1 = never / always launch the conditional repair pass
  int small_batch_kernel = 1;   // batches of <= 128 queries are scored by stream_select.hip (HBM-bound kernel)
  int xcc_balance = 1;          // split the gallery tiles over the XCDs by their measured speed (common.h XccBalance)
  int ladder = 1;               // in-launch threshold ladder of the tile kernel (common.h QueryState::lad_*): 0 = off, 1 = on
  int boot_ksplit = 1;          // small batches: K-split bootstrap launch (kernels.h ScoreArgs::ksplit); 0 = one workgroup per tile
  int stream_tail = 1;          // host entry points with more than one batch of queries: deferred tail between their batches
  // asynchronous tail (option "async_tail", device entry point mi_knn_search_device only): the exact re-score + emit of a
  // batch run on tail_stream behind an event, beside the scoring launch of the NEXT batch (the tile kernel leaves 80
  // VGPRs per SIMD lane and no LDS: exactly one 70-register re-score wave per SIMD fits next to its two); results are
  // valid after mi_search_join
  int async_tail = 0, tail_set = 0;
  hipStream_t tail_stream = nullptr;
  hipEvent_t ev_p1[2] = {nullptr, nullptr}, ev_tail[2] = {nullptr, nullptr};
  bool ev_tail_valid[2] = {false, false};
  hipEvent_t gate_before_scoring = nullptr;   // async_tail 2: the filtered scoring launch of a batch waits for this event
  // async_tail 3 ("deferred"): the tail of batch i is ENQUEUED by the search call of batch i + 1, after that batch's query
  // ingest / bootstrap / threshold launches and right before its scoring launch, so that the re-score gather shares the
  // device with the power-bound scoring launch only -- not with the bootstrap, which wants the same memory system
  // (mode 1 starts the tail as soon as phase 1 is done, i.e. beside the next batch's bootstrap: 63 -> 214 us).
  struct PendingTail {
    bool valid = false;
    int32_t b = 0, k = 0;
    int set = 0;
    int slot = 0;                             // workspace slot (ws_slot) the batch ran in
    int64_t* out_idx = nullptr;
    float* out_score = nullptr;
    double* out_score64 = nullptr;
  } pending;
  hipEvent_t ev_pre = nullptr;                // recorded on the caller's stream right before the scoring launch
  int qnorm_override = -1;  // device entry points: normalise queries with this mi_norm instead of the gallery's (-1 = off)
  uint32_t surv_cap = 12288, rescore_cap = 2048;
  // stats
  mi_search_stats stats{};
  bool profile = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  std::vector<float> launch_ms_log;   // duration of every timed scoring launch since the last statistics reset (capped)
  hipStream_t ev_stream = nullptr;
  // Every grow-only device buffer below is a DeviceBuf on `scratch`: it dies with the handle (scratch.reset() in the destroy),
  // and nothing else has to name it.  The primary storage above and the workspace arena are NOT: their ownership is traded with
  // the process's spare slots (api_state.hip), so they stay bare pointers freed by hand.
  DeviceBufSet scratch;
  // device staging of the host entry point mi_knn_search (queries in, results out; io_stage): a hipMalloc / hipFree pair per
  // call costs more than a single-query search
  DeviceBuf<char> io_q{scratch}, io_idx{scratch}, io_sc{scratch};
  // the range search (api_range.hip)
  struct RangeScratch {
    explicit RangeScratch(DeviceBufSet& s) : rows(s), rcnt(s), sc(s), akey(s), arow(s), bkey{DeviceBuf<uint64_t>(s), DeviceBuf<uint64_t>(s)},
                                             brow{DeviceBuf<uint32_t>(s), DeviceBuf<uint32_t>(s)}, coff(s), ccnt(s), lims(s), total(s) {}
    DeviceBuf<uint32_t> rows;              // [QB][surv_cap] rows handed to the exact re-score (these three: exactly that size)
    DeviceBuf<uint32_t> rcnt;              // [QB]
    DeviceBuf<double> sc;                  // [QB][surv_cap] their f64 scores
    DeviceBuf<uint64_t> akey;              // hits of the batch, chunk after chunk
    DeviceBuf<uint32_t> arow;
    DeviceBuf<uint64_t> bkey[2];           // hits of the batch in CSR order (ping-pong of the merge passes)
    DeviceBuf<uint32_t> brow[2];
    DeviceBuf<uint64_t> coff;              // [chunks][QB] offset of query q's hits of chunk c in akey / arow
    DeviceBuf<uint32_t> ccnt;              // [chunks][QB] their number
    DeviceBuf<int64_t> lims;               // [QB + 1]
    DeviceBuf<unsigned long long> total;   // hits of the current chunk
  } range{scratch};
  // filtered top-K search (api_filter.hip): grow-only device buffers and the compacted sub-gallery, freed with the handle, never
  // handed to the spare-buffer slots; invalidated by mi_gallery_append*, mi_gallery_set_image_dtype and mi_gallery_remove_rows (filter_invalidate)
  int filter_path = 0;                 // option "filter_path": 0 = auto, 1 = always compact, 2 = always over-fetch
  double filter_compact_max = 0.15;    // option "filter_compact_max": auto compacts at selectivity <= this
  int filter_cache = 1;                // option "filter_cache": keep the sub-gallery for the next call with the same bitmap
  struct FilterScratch {
    explicit FilterScratch(DeviceBufSet& s) : bits(s), bcnt(s), boff(s), rows(s), idx(s), sidx(s), sc(s), ssc(s), ok(s), qbuf(s) {}
    DeviceBuf<uint64_t> bits;            // device copy of a host bitmap
    DeviceBuf<uint32_t> bcnt, boff;      // [blocks] allowed rows per compaction workgroup, then their offsets [blocks + 1]
    DeviceBuf<uint32_t> rows;            // allowed local rows of the sub-gallery's bitmap, ascending
    DeviceBuf<int64_t> idx, sidx;        // [nq][k] answer of the call / [nq][k_eff] answer of the sub-gallery
    DeviceBuf<float> sc, ssc;
    DeviceBuf<uint32_t> ok;              // [nq] over-fetch certificate per query
    DeviceBuf<char> qbuf;                // queries the over-fetch could not certify, packed
    mi_gallery* sub = nullptr;           // compacted sub-gallery (shares the parent's stream)
    int64_t sub_cap = 0;                 // rows its buffers hold
    bool valid = false;                  // sub holds the rows `key` allows of a parent of key_n rows
    int64_t key_n = -1;
    std::vector<uint64_t> key;           // the bitmap it was built from (bits at or beyond key_n cleared)
    std::vector<uint64_t> last_key;      // the bitmap of the previous call (auto compacts a bitmap it sees twice in a row)
    int64_t last_key_n = -1;
  } filt{scratch};
  // grouped top-K search (api_group.hip): the labels of mi_gallery_set_groups in the dense form the kernels read, and the
  // grow-only buffers of a call.  Dropped by whatever changes n or the rows (mi_gallery_append*, mi_gallery_remove_rows:
  // groups_drop); never written to the gallery file
  int group_path = 0;                  // option "group_path": 0 = auto, 1 = always the dense fallback, 2 = always over-fetch
  struct GroupState {
    explicit GroupState(DeviceBufSet& s) : grp(s), group_off(s), group_rows(s), chunk_g0(s), label_of_group(s), excl(s), ok(s), idx(s),
                                           sc(s), lab(s), qbuf(s), dense(s), key{DeviceBuf<uint64_t>(s), DeviceBuf<uint64_t>(s)},
                                           row{DeviceBuf<uint32_t>(s), DeviceBuf<uint32_t>(s)}, lims(s), cand_rows(s), cand_cnt(s),
                                           cand_score(s) {}
    bool valid = false;                  // the plan below is the one of the gallery's current n rows
    GroupPlan plan;                      // host copy (group_plan.h): label -> dense id, G, the chunk count
    std::vector<int32_t> labels;         // the labels as given (mi_gallery_get_groups)
    DeviceBuf<uint32_t> grp, group_off, group_rows, chunk_g0;
    DeviceBuf<int32_t> label_of_group;
    DeviceBuf<uint32_t> excl;            // [nq] dense id of the group a query excludes (GROUP_NONE = none)
    DeviceBuf<uint32_t> ok;              // [nq] over-fetch certificate per query
    DeviceBuf<int64_t> idx;              // [nq][k] answer of a path
    DeviceBuf<float> sc;
    DeviceBuf<int32_t> lab;
    DeviceBuf<char> qbuf;                // queries the over-fetch could not certify, packed
    DeviceBuf<double> dense;             // [queries of a sub-batch][n] float64 scores ("group_dense_bytes")
    DeviceBuf<uint64_t> key[2];          // [queries of a sub-batch][G] group table (ping-pong of csr_order.hip's merge passes)
    DeviceBuf<uint32_t> row[2];
    DeviceBuf<int64_t> lims;             // [queries of a sub-batch + 1] and, behind them, the list total csr_order.hip reads
    DeviceBuf<uint32_t> cand_rows, cand_cnt;   // [queries of a sub-batch][k] rows taken, re-scored by rescore_kernel
    DeviceBuf<double> cand_score;
  } groups{scratch};
  // squared-L2 search (api_l2.hip)
  struct L2Scratch {
    explicit L2Scratch(DeviceBufSet& s) : qraw(s), qaug(s), ids(s), oidx(s), odist(s), odist64(s) {}
    DeviceBuf<char> qraw;                // queries of a host call as given
    DeviceBuf<float> qaug;               // [nq][dp] extended queries
    DeviceBuf<int64_t> ids;              // [nq][ke] rows the selection certified
    DeviceBuf<int64_t> oidx;             // [nq][k] results of a host call
    DeviceBuf<float> odist;
    DeviceBuf<double> odist64;
  } l2{scratch};
  // re-ranking of shortlists (api_refine.hip)
  struct RefineScratch {
    explicit RefineScratch(DeviceBufSet& s) : qraw(s), qpad(s), val(s), cand(s), oidx(s), oval(s), oval64(s) {}
    DeviceBuf<char> qraw;                // queries of a host call as given
    DeviceBuf<float> qpad;               // [nq][dp] queries with 16-byte aligned rows
    DeviceBuf<double> val;               // [nq][kc] f64 value of every candidate
    DeviceBuf<int64_t> cand;             // [nq][kc] candidates of a host call
    DeviceBuf<int64_t> oidx;             // [nq][k] results of a host call
    DeviceBuf<float> oval;
    DeviceBuf<double> oval64;
  } refine{scratch};
  // Minkowski search (api_minkowski.hip)
  struct MinkScratch {
    explicit MinkScratch(DeviceBufSet& s) : qraw(s), qpad(s), val(s), part_key(s), part_id(s), bits(s), oidx(s), odist(s), odist64(s), rcnt(s),
                                            roff(s), rkey{DeviceBuf<uint64_t>(s), DeviceBuf<uint64_t>(s)},
                                            rrow{DeviceBuf<uint32_t>(s), DeviceBuf<uint32_t>(s)}, rlims(s) {}
    DeviceBuf<char> qraw;                // queries of a host call as given
    DeviceBuf<float> qpad;               // [nq][dp] queries with 16-byte aligned rows
    DeviceBuf<double> val;               // [queries of a chunk][n] f64 value of every row
    DeviceBuf<uint64_t> part_key;        // [queries of a chunk][parts][k]
    DeviceBuf<int64_t> part_id;
    DeviceBuf<uint64_t> bits;            // device copy of a host bitmap
    DeviceBuf<int64_t> oidx;             // [nq][k] results of a host call
    DeviceBuf<float> odist;
    DeviceBuf<double> odist64;
    // radius search (api_minkowski_range.hip): counts and places per (query, part) of a chunk, the chunk's hits (ping-pong of the
    // merge passes), the CSR offsets of a host call
    DeviceBuf<uint32_t> rcnt;
    DeviceBuf<int64_t> roff;
    DeviceBuf<uint64_t> rkey[2];
    DeviceBuf<uint32_t> rrow[2];
    DeviceBuf<int64_t> rlims;
  } mink{scratch};
  // row removal (api_remove.hip): one arena of exactly the bytes the largest call needed -- staging area of "remove_block_rows"
  // rows in the gallery's own layout, keep-list, bitmap, scan buffers
  DeviceBuf<char> rm_arena{scratch};
  // diffusion state (offline matrix rows kept on the device for the online stage); dropped by mi_gallery_remove_rows
  int32_t* dif_ids = nullptr;
  float* dif_vals = nullptr;
  int32_t dif_T = 0;
  uint64_t removals = 0;              // calls that removed at least one row (api_remove.hip); mi_ivfflat records it, nothing public shows it
  std::mutex mu;
  std::atomic<int> online_users{0};   // mi_online handles built on this gallery: it cannot be destroyed under them
};

// the binary index (api_hamming.hip; api_lsh.hip encodes rows straight into `codes`)
struct mi_hamming {
  int device = 0;
  int64_t n = 0, cap = 0, row_offset = 0;
  int32_t nbits = 0, nb = 0, W32 = 0, wq = 0;      // bits, bytes, 32-bit words of a code; words of a stored query
  DeviceBufSet bufs;                               // every device allocation of the handle: hbm_bytes is bufs.bytes()
  DeviceBuf<uint32_t> codes{bufs};                 // [ceil(cap / 64)][W32][64], exactly
  hipStream_t stream = nullptr;
  DeviceBuf<uint8_t> qraw{bufs};                   // query bytes of a host call, packed [nq][nb]
  DeviceBuf<uint32_t> qw{bufs};                    // [nq][wq]
  DeviceBuf<uint16_t> mat{bufs};                   // distance matrix [queries of a chunk][round_up(n, 64)]
  DeviceBuf<uint64_t> bits{bufs};                  // device copy of a host bitmap
  DeviceBuf<int64_t> oidx{bufs};                   // results of a host call
  DeviceBuf<int32_t> odist{bufs};
  // radius search (hamming_range.hip): ballots, prefixes and segment sums of one chunk of queries, the chunk's hits in id order,
  // CSR offsets of a host call
  DeviceBuf<unsigned long long> rmask{bufs};
  DeviceBuf<uint16_t> roffs{bufs};
  DeviceBuf<uint32_t> rseg{bufs};
  DeviceBuf<unsigned long long> rstage{bufs};
  DeviceBuf<int64_t> rlims{bufs};
  std::mutex mu;
};
// ---- api_hamming.hip, for api_components.hip: the ballots of a self-join over rows [row0, row0 + nrows) chunk by chunk, with no
// offsets, fill or order stage behind them.  The caller holds h->mu and has set the device.
struct HammingBallots {
  const unsigned long long* masks = nullptr;   // [nbl][qstride] in the index's own workspace, valid until its next scan
  int64_t b0 = 0, nbl = 0;                     // first block scanned, blocks scanned (0: no row above the chunk, nothing launched)
  int64_t qstride = 0, qrow0 = 0;              // words of a row of masks; the stored row that is query 0 of the chunk
  int32_t nq = 0;                              // queries of the chunk
};
MI_INTERNAL int hamming_self_check(const mi_hamming* h, int64_t row0, int64_t nrows, int32_t radius);   // mi_hamming_self_range's checks
// hr_prepare for the call: the workspace within "hamming_range_bytes", *qc queries per chunk
MI_INTERNAL int hamming_self_plan(mi_hamming* h, int64_t row0, int64_t nrows, int64_t* qc);
// the scan launch of the chunk that starts at query q0 (a multiple of qc), enqueued on s
MI_INTERNAL int hamming_self_scan(mi_hamming* h, int64_t row0, int64_t nrows, int32_t radius, int64_t qc, int64_t q0,
                                  HammingBallots* out, hipStream_t s);

// connected components of the rows [0, n) (api_components.hip; kernels in components.hip)
struct mi_components {
  int device = 0;
  int64_t n = 0;
  DeviceBufSet bufs;
  DeviceBuf<int32_t> parent{bufs};                 // [n] exactly: the forest, flat between calls (every entry a root)
  DeviceBuf<unsigned long long> word{bufs};        // the flag of an id check / the count of roots (256 bytes)
  hipStream_t stream = nullptr;
  std::mutex mu;
};

// what both flat PQ indexes hold (pq_flat.h has the host functions over it): CodeT is a code of one book, uint8_t for mi_pq (Ks <= 256,
// four books to a dword) and uint16_t for mi_pqw (Ks <= 8192, two)
template <typename CodeT>
struct PqFlat {
  typedef CodeT Code;
  static constexpr int32_t CODE_VALUES = 1 << (8 * sizeof(CodeT));   // no code of this width reaches it
  int device = 0;
  int64_t n = 0, cap = 0, row_offset = 0;
  int32_t d = 0, m = 0, ks = 0, L = 0, MW = 0;     // columns, books, codewords per book, columns per book, dwords of a code
  std::vector<float> cb_host;                      // [m][ks][L]
  DeviceBufSet bufs;                               // every device allocation of the handle: hbm_bytes is bufs.bytes()
  DeviceBuf<float> cb{bufs};                       // (cb, codes, flag: exactly their size, allocated at creation)
  DeviceBuf<uint32_t> codes{bufs};                 // [ceil(cap / 64)][MW][64]
  DeviceBuf<uint32_t> flag{bufs};                  // raised by the check of device-resident codes (256 bytes)
  hipStream_t stream = nullptr;
  DeviceBuf<char> xraw{bufs};                      // rows / queries of a host call, packed [rows][d] in their own type
  DeviceBuf<CodeT> cstage{bufs};                   // packed codes [rows][m]: host codes on their way in, encoder output
  DeviceBuf<float> tab{bufs};                      // distance tables [queries of a chunk][m][ks]
  DeviceBuf<float> mat{bufs};                      // negated distances [queries of a chunk][round_up(n, 64)]
  DeviceBuf<int64_t> tidx{bufs};                   // [queries of a chunk][ke] what the selection returns
  DeviceBuf<float> tneg{bufs};
  DeviceBuf<uint64_t> bits{bufs};                  // device copy of a host bitmap
  DeviceBuf<int64_t> oidx{bufs};                   // results of a host call
  DeviceBuf<float> odist{bufs};
  std::mutex mu;
};
// the PQ index (api_pq.hip; api_pq_graph.hip searches a neighbour graph over its codes)
struct mi_pq : PqFlat<uint8_t> {
  DeviceBuf<uint32_t> rmpref{bufs}, rmstage{bufs}; // mi_pq_remove_rows: prefix counts per bitmap word; staging blocks [..][MW][64]
  // bumped by every call that changes the rows (mi_pq_add, mi_pq_append_codes, mi_pq_remove_rows): what a mi_pq_graph records,
  // since rows can leave and as many come back.  Internal; nothing reports it
  uint64_t mod = 0;
};
// the search proper on stream s (api_pq.hip): queries on the device (any strides), results go to device buffers
MI_INTERNAL int pq_search_core(mi_pq* h, const void* q_dev, int dtype, int64_t rs, int64_t cs, int64_t nq, int32_t k,
                               const uint64_t* allow_dev, int64_t* out_idx_dev, float* out_dist_dev, hipStream_t s);
// the wide PQ index (api_pq_wide.hip)
struct mi_pqw : PqFlat<uint16_t> {};

// ---- api_state.hip
MI_INTERNAL int ws_free(Workspace& ws);
MI_INTERNAL int ws_ensure(mi_gallery* g, int32_t k);
MI_INTERNAL bool snapshot_balance(const mi_gallery* g, float* out_w8);
// ---- api_schedule.hip
MI_INTERNAL QueryState make_state(const Workspace& ws);
MI_INTERNAL int64_t bootstrap_tiles(const mi_gallery* g);      // rows / 256 of the bootstrap chunk / the default threshold sample
MI_INTERNAL int64_t sample_rows_in_effect(const mi_gallery* g);
MI_INTERNAL void prof_collect(mi_gallery* g);
MI_INTERNAL int flush_pending_tail(mi_gallery* g, hipStream_t s, bool beside_scoring);
MI_INTERNAL int phase1_batch(mi_gallery* g, const void* q_src, int q_dtype, int64_t q_rs, int64_t q_cs, int q_norm, int32_t nq,
                             int32_t k, bool exact, hipStream_t s, bool fuse_cand = false, bool caller_checks_flags = false);
MI_INTERNAL int phase2_batch(mi_gallery* g, int32_t nq, int32_t k, const float* L_dev, int64_t* out_idx, float* out_score,
                             double* out_score64, hipStream_t s, bool have_cand = false, bool resident = false,
                             Workspace* wsp = nullptr, bool flag_short = false);
MI_INTERNAL void count_flagged_batch(mi_gallery* g, uint32_t flags);
MI_INTERNAL int check_k(const mi_gallery* g, int32_t k);
MI_INTERNAL int search_device(mi_gallery* g, const void* q_src, int q_dtype, int64_t q_rs, int64_t q_cs, int q_norm, int64_t nq,
                              int32_t k, int64_t* out_idx, float* out_score, double* out_score64, bool exact, hipStream_t s,
                              bool allow_async = false, bool caller_checks_flags = false);
MI_INTERNAL int join_tails(mi_gallery* g, hipStream_t s);
MI_INTERNAL int strided_extent(int64_t n, int64_t d, int64_t rs, int64_t cs, int64_t* elems);
MI_INTERNAL int read_and_clear_flags(mi_gallery* g, uint32_t* flags);
MI_INTERNAL int search_sync(mi_gallery* g, const void* q_dev, int q_dtype, int64_t rs, int64_t cs, int q_norm, int64_t nq,
                            int32_t k, int64_t* idx_dev, float* score_dev, double* score64_dev);
MI_INTERNAL int dense_search_device(mi_gallery* g, const void* q_src, int q_dtype, int64_t rs, int64_t cs, int q_norm, int64_t nq,
                                    int32_t k, int64_t* out_idx_dev, float* out_score_dev, hipStream_t s);
MI_INTERNAL int dense64_search_device(mi_gallery* g, const void* q_src, int q_dtype, int64_t rs, int64_t cs, int q_norm,
                                      int64_t nq, int32_t k, int64_t* out_idx_dev, float* out_score_dev,
                                      double* out_score64_dev, hipStream_t s);
// ---- api_gallery.hip
MI_INTERNAL int gallery_alloc(mi_gallery* g);
// mi_gallery_create / mi_gallery_create_l2: n rows of `data` (n == 0: none) into a gallery of `capacity` rows (0 = n)
MI_INTERNAL int gallery_create_any(const void* data, int64_t n, int32_t d, int dtype, int64_t row_stride, int64_t col_stride,
                                   int memspace, int norm_mode, int metric, int device, int64_t row_offset, int64_t capacity,
                                   mi_gallery** out);
// ---- api_remove.hip
// mi_gallery_remove_rows behind its argument checks, its online-handle check and its lock, which the caller holds; out_removed (may
// be NULL) is written only when rows left
MI_INTERNAL int gallery_remove_rows_locked(mi_gallery* g, const uint64_t* remove_bits, int memspace, int64_t* out_removed);
// ---- api_filter.hip
MI_INTERNAL void filter_release_sub(mi_gallery* g);     // frees the compacted sub-gallery (option "filter_cache" 0)
MI_INTERNAL void filter_invalidate(mi_gallery* g);      // rows or image type of the parent changed: the sub-gallery is stale
// mi_knn_search_filtered (argument checks included); l2_caller: mi_knn_search_l2 on its own gallery, which HOLDS the handle's
// lock (otherwise the call takes it)
MI_INTERNAL int filtered_search_host(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride,
                                     int32_t k, const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_score,
                                     mi_filter_info* out_info, double* out_seconds, bool l2_caller);
// ---- api_group.hip
MI_INTERNAL void groups_drop(mi_gallery* g);            // n or the rows changed: the labels no longer name them
// ---- api_minkowski.hip
// the argument checks of every Minkowski entry point (*op: the term the kernels evaluate, MINK_OP_*); what the gallery must be
MI_INTERNAL int mink_check(const mi_gallery* g, int64_t nq, int metric, double p, int32_t k, int* op);
MI_INTERNAL int mink_rows_check(const mi_gallery* g);
// ---- helpers of the handles (static: every translation unit has its own, nothing is exported)
// the staging of a host search on a gallery (mi_gallery::io_*): `bytes` bytes, NULL when out of memory.  Sized in bytes, with its
// own spare of a quarter + 256
static inline void* io_stage(DeviceBuf<char>& b, size_t bytes) {
  return b.ensure(bytes, bytes + bytes / 4 + 256) == MI_OK ? b.get() : nullptr;
}
// the allow bitmap of a search on an index of n rows, where the kernels read it: the caller's device pointer, or the host words
// copied into `bits` on `stream`
static inline int allow_on_device(DeviceBuf<uint64_t>& bits, const uint64_t* allow_bits, int memspace, int64_t n, hipStream_t stream,
                                  const uint64_t** allow_dev) {
  *allow_dev = allow_bits;
  if (!allow_bits || memspace != MI_HOST || n <= 0) return MI_OK;
  const size_t words = (size_t)((n + 63) / 64);
  int rc;
  if ((rc = bits.grow(words)) != MI_OK) return rc;
  HIPC(hipMemcpyAsync(bits, allow_bits, words * 8, hipMemcpyHostToDevice, stream));
  *allow_dev = bits;
  return MI_OK;
}
// the tail of a host top-K search on an index: `cnt` ids and (when asked for) distances back to the caller, the stream drained,
// the call's wall time since t0
template <typename D>
static int topk_to_host(int64_t* out_idx, const int64_t* idx_dev, D* out_dist, const D* dist_dev, size_t cnt, hipStream_t s,
                        std::chrono::steady_clock::time_point t0, double* out_seconds) {
  HIPC(hipMemcpyAsync(out_idx, idx_dev, cnt * 8, hipMemcpyDeviceToHost, s));
  if (out_dist) HIPC(hipMemcpyAsync(out_dist, dist_dev, cnt * sizeof(D), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return MI_OK;
}
// api_pq.hip, api_pq_train.hip, api_ivfpq.hip: host rows (any strides, in elements) hold no NaN and no infinity
template <typename T>
static bool pq_all_finite(const T* x, int64_t rows, int32_t d, int64_t rs, int64_t cs) {
  for (int64_t r = 0; r < rows; ++r)
    for (int32_t c = 0; c < d; ++c)
      if (!std::isfinite(x[r * rs + (int64_t)c * cs])) return false;
  return true;
}
// api_pq_train.hip, api_kmeans.hip: what a training call owns -- a stream, its events and its buffers, freed before it returns
template <typename CodeT>
struct TrainScratch {
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};     // assignment begin / end, update begin / end
  void* xdev = nullptr;                    // host rows, packed [n][d] in their own type
  CodeT* codes[2] = {nullptr, nullptr};    // [n][m] of this iteration and of the one before
  CodeT* cols = nullptr;                   // [m][n]
  float* cb = nullptr;                     // [m][ks][L], updated in place
  unsigned long long* moved = nullptr;
  ~TrainScratch() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (void* p : {xdev, (void*)codes[0], (void*)codes[1], (void*)cols, (void*)cb, (void*)moved}) (void)hipFree(p);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
// host rows -> packed [n][d] on the device, once.  Rows that are not contiguous pass through a host block of 64 MiB
template <typename CodeT>
static int train_upload(TrainScratch<CodeT>& w, const void* x, int64_t n, int32_t d, size_t esz, int64_t rs, int64_t cs) {
  if (cs == 1 && (rs == d || n == 1)) {
    HIPC(hipMemcpyAsync(w.xdev, x, (size_t)n * d * esz, hipMemcpyHostToDevice, w.stream));
    HIPC(hipStreamSynchronize(w.stream));
    return MI_OK;
  }
  const int64_t step = std::max<int64_t>(1, ((int64_t)64 << 20) / ((int64_t)d * (int64_t)esz));
  std::vector<char> pack((size_t)std::min(step, n) * d * esz);
  for (int64_t r0 = 0; r0 < n; r0 += step) {
    const int64_t mm = std::min(step, n - r0);
    const char* src = (const char*)x + (size_t)r0 * rs * esz;
    for (int64_t r = 0; r < mm; ++r)
      for (int32_t c = 0; c < d; ++c)
        std::memcpy(pack.data() + ((size_t)r * d + c) * esz, src + ((size_t)r * rs + (size_t)c * cs) * esz, esz);
    HIPC(hipMemcpyAsync((char*)w.xdev + (size_t)r0 * d * esz, pack.data(), (size_t)mm * d * esz, hipMemcpyHostToDevice, w.stream));
    HIPC(hipStreamSynchronize(w.stream));              // the block is packed again
  }
  return MI_OK;
}
// device times of the calling thread's last mi_pq_train / mi_pqw_train / mi_kmeans_train, per iteration that ran
// (mi_pq_train_timing; defined in api_pq_train.hip)
struct TrainTimes { std::vector<float> assign_ms, update_ms; };
MI_INTERNAL TrainTimes& train_times();
// api_pq.hip, api_ivfpq.hip: the checks the host query entry points share
static inline int check_host_queries(int32_t d, const void* q, int64_t nq, int dtype, int64_t rs, int64_t cs) {
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  REQUIRE(rs >= 0 && cs >= 0, "negative strides are not supported");
  const bool finite = dtype == MI_F32 ? pq_all_finite((const float*)q, nq, d, rs, cs) : pq_all_finite((const double*)q, nq, d, rs, cs);
  REQUIRE(finite, "queries must be finite");
  return MI_OK;
}
// the first m codes of every row (code bytes or uint16, list ids) are below `limit`
template <typename CodeT>
static inline bool codes_below(const CodeT* p, int64_t rows, int64_t stride, int32_t m, int32_t limit) {
  if (limit >= PqFlat<CodeT>::CODE_VALUES) return true;
  for (int64_t r = 0; r < rows; ++r)
    for (int32_t b = 0; b < m; ++b)
      if (p[r * stride + b] >= limit) return false;
  return true;
}
// behind a check launch on `s` (launch_pq_check, launch_ivf_check): *raised = the check raised the handle's flag, which is cleared
// again for the next check
static inline int check_flag(uint32_t* flag, hipStream_t s, bool* raised) {
  uint32_t f = 0;
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(&f, flag, 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  if (f) {
    HIPC(hipMemsetAsync(flag, 0, 4, s));
    HIPC(hipStreamSynchronize(s));
  }
  *raised = f != 0;
  return MI_OK;
}
// the m codes of the row in slot `slot` (block * 64 + lane) of `blocks`, transposed 64-row blocks of `dwords` dwords a code, the
// first of them block 0 -> dst
template <typename CodeT>
static inline void unpack_code_row(const uint32_t* blocks, int64_t slot, int32_t dwords, int32_t m, CodeT* dst) {
  constexpr int32_t PER = pq_codes_per_dword<CodeT>(), BITS = 8 * sizeof(CodeT);
  const uint32_t* src = blocks + (slot >> 6) * dwords * 64 + (slot & 63);
  for (int32_t j = 0; j < m; ++j) dst[j] = (CodeT)(src[(int64_t)(j / PER) * 64] >> (BITS * (j % PER)));
}
// `rows` host rows of d elements from row r0 on -> xraw (grown to fit), packed [rows][d] in their own type, on `stream`.  Rows that
// are not contiguous are packed on the host first, in `pack` (the copy has completed on return in that case)
static inline int stage_host_rows(DeviceBuf<char>& xraw, int32_t d, hipStream_t stream, const void* x, int64_t r0, int64_t rows,
                                  int dtype, int64_t rs, int64_t cs, std::vector<char>& pack) {
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  const size_t bytes = (size_t)rows * d * esz;
  int rc;
  if ((rc = xraw.grow(bytes)) != MI_OK) return rc;
  const char* src = (const char*)x + (size_t)r0 * rs * esz;
  if (!(cs == 1 && (rs == d || rows == 1))) {
    pack.resize(bytes);
    for (int64_t r = 0; r < rows; ++r)
      for (int32_t c = 0; c < d; ++c)
        std::memcpy(pack.data() + ((size_t)r * d + c) * esz, src + ((size_t)r * rs + (size_t)c * cs) * esz, esz);
    src = pack.data();
  }
  HIPC(hipMemcpyAsync(xraw, src, bytes, hipMemcpyHostToDevice, stream));
  if (src == pack.data()) HIPC(hipStreamSynchronize(stream));
  return MI_OK;
}
// rows handed to an index: the argument checks of mi_pq_add / mi_pq_encode and their mi_ivfpq counterparts
#define REQUIRE_ROWS(x, rows, dtype, rs, cs, memspace)                                                       \
  REQUIRE((rows) >= 0, "negative number of rows");                                                           \
  REQUIRE((x) || (rows) == 0, "null pointer: rows");                                                         \
  REQUIRE((dtype) == MI_F32 || (dtype) == MI_F64, "dtype must be MI_F32 or MI_F64");                         \
  REQUIRE((rs) >= 0 && (cs) >= 0, "negative strides are not supported");                                     \
  REQUIRE((memspace) == MI_HOST || (memspace) == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE")
// entry points that are not defined on a squared-L2 gallery (include/mi355_retrieval.h: mi_metric)
#define REFUSE_L2(g, what)                                                                                          \
  do {                                                                                                              \
    if ((g)->metric != MI_METRIC_IP)                                                                                \
      return fail(MI_ERR_UNSUPPORTED, what " is not available on a gallery of metric MI_METRIC_L2 (squared "         \
                                           "Euclidean distance): use the mi_*_l2 entry points");                    \
  } while (0)
