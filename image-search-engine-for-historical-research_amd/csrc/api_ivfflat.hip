// Inverted file over the stored rows of a gallery (mi_ivfflat*; faiss IndexIVFFlat, the reference's matching_PQ_Net_bucket without the
// PQ loss).  DESIGN.md 5.18.  The handle holds the centroids float32 [nlist][dp] (rows of the gallery's padded stride, so the wave
// sums read them like stored rows), list_off int64 [nlist + 1] and list_rows int32 [n] on the device, plus the workspace of its
// searches; the rows and their metric are the gallery's.  Every query entry point is a device form (packed f32 queries, enqueued on the
// caller's stream); the binding stages host queries.  Probe and assignment are launch_refine
// over the centroid table (candidates 0 .. nlist - 1, one row of them shared by every query: cand_stride 0), so their values, ties and
// order are mi_refine's; the list build, the prefix, the scan with its selection and the merge are ivfflat.hip's.
// The index follows its gallery in place: mi_ivfflat_sync assigns the appended rows and splices them behind the rows of their lists,
// mi_ivfflat_remove_rows removes rows from the gallery (api_remove.hip's own code) and compacts the lists by the same bitmap.  Either
// writes new tables, swaps them in on success and leaves the bytes mi_ivfflat_build writes on the gallery as it then stands.
#include "api_internal.h"

// probe values, probes, prefixes, partial lists and counts of one chunk of queries: a batch that needs more goes in chunks of queries
constexpr size_t IVFF_STAGE_BYTES = (size_t)256 << 20;
// values of the centroids for one chunk of stored rows of a build
constexpr size_t IVFF_ASSIGN_BYTES = (size_t)64 << 20;

struct mi_ivfflat {
  mi_gallery* rows = nullptr;
  int64_t n = 0;                       // rows of the gallery the lists cover; probe and search refuse any other number
  uint64_t removals = 0;               // the gallery's count of removals the lists cover: one made outside the index shows here
  int32_t d = 0, nlist = 0;
  std::vector<int64_t> off_host;       // list_off on the host
  std::vector<int64_t> topsum;         // [nlist + 1]: topsum[p] = rows of the p longest lists, what p probes can reach at the most
  DeviceBufSet bufs;                   // every device allocation of the handle: hbm_bytes is bufs.bytes()
  DeviceBuf<float> cent{bufs};         // [nlist][dp], columns at and beyond d are zero
  DeviceBuf<int64_t> iota{bufs};       // [nlist]: 0 .. nlist - 1, the candidates of every probe
  DeviceBuf<int64_t> list_off{bufs};   // [nlist + 1]
  DeviceBuf<int32_t> list_rows{bufs};  // [n]
  DeviceBuf<uint32_t> flag{bufs};      // raised by the check of device-resident list ids (256 bytes)
  // grow-only workspace of the searches
  DeviceBuf<float> qpad{bufs};         // [nq][dp]
  DeviceBuf<double> pval{bufs};        // [queries of a chunk][nlist] values of the centroids (launch_refine's workspace)
  DeviceBuf<int64_t> pidx{bufs};       // [queries of a chunk][nprobe] the library's probes
  DeviceBuf<int32_t> norm{bufs};       // [queries of a chunk][nprobe] normalised probes
  DeviceBuf<int32_t> pref{bufs};       // [queries of a chunk][nprobe + 1]
  DeviceBuf<uint64_t> part_key{bufs};  // [queries of a chunk][nslab][k]
  DeviceBuf<int64_t> part_id{bufs};
  DeviceBuf<uint32_t> pcnt{bufs};      // [queries of a chunk][nslab]
  std::mutex mu;
};

// ---- checks that answer before a handle is read
static int ivff_make_check(const void* rows, const float* centroids, int32_t nlist, const void* out) {
  REQUIRE(rows, "null handle");
  REQUIRE(centroids, "null pointer: centroids");
  REQUIRE(out, "null pointer: out");
  REQUIRE(nlist >= 2 && nlist <= IVFF_MAX_LISTS, "nlist must be in [2, 8192]");
  return MI_OK;
}

static int ivff_search_check(const void* f, int64_t nq, int32_t k, int32_t nprobe) {
  REQUIRE(f, "null handle");
  REQUIRE(k >= 1 && k <= IVFFLAT_SLAB_ROWS, "k must be in [1, 2048]");
  REQUIRE(nprobe >= 1 && nprobe <= IVFF_MAX_LISTS, "nprobe must be in [1, nlist]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  return MI_OK;
}

// a removal the index was not told of renumbers the rows under its lists, and an append after it can put n back where it was
static int ivff_no_outside_removal(const mi_ivfflat* f) {
  REQUIRE(f->rows->removals == f->removals,
          "the gallery has been appended to or had rows removed since the index was made: a removal was made outside the index "
          "(mi_ivfflat_remove_rows keeps the two in step): build a new index");
  return MI_OK;
}

static int ivff_fresh(const mi_ivfflat* f) {
  int rc = ivff_no_outside_removal(f);
  if (rc != MI_OK) return rc;
  REQUIRE(f->rows->n == f->n,
          "the gallery has been appended to or had rows removed since the index was made: mi_ivfflat_sync takes the appended rows in, "
          "or build a new index");
  return MI_OK;
}

// rows per launch_refine call of an assignment of `rows` stored rows
static int64_t ivff_assign_chunk(int64_t rows, int32_t nlist) {
  return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(rows, 65535), (int64_t)(IVFF_ASSIGN_BYTES / 8) / nlist));
}

// list ids of the stored rows [r0, r1) of the gallery -> lid[0 .. r1 - r0): the probe-1 list of each, launch_refine with k = 1 over
// the centroid table.  The stored rows are the queries: rows of stride dp, d columns used.  val [chunk][nlist], best [chunk]
static void ivff_assign(const mi_ivfflat* f, int64_t r0, int64_t r1, int64_t chunk, double* val, int64_t* best, int32_t* lid,
                        hipStream_t s) {
  const mi_gallery* g = f->rows;
  const int32_t dp = g->dp, nlist = f->nlist;
  const int l2 = g->metric == MI_METRIC_L2 ? 1 : 0;
  for (int64_t r = r0; r < r1; r += chunk) {
    const int64_t b = std::min<int64_t>(chunk, r1 - r);
    launch_refine(f->cent, g->gal_f32 + (size_t)r * dp, dp, f->d, nlist, 0, l2, f->iota, nlist, 0, 1, b, val, best, nullptr, nullptr, s);
    launch_ivff_take_ids(best, b, lid + (r - r0), s);
  }
}

// off_host -> topsum
static void ivff_topsum(mi_ivfflat* f) {
  const int32_t nlist = f->nlist;
  std::vector<int64_t> sz((size_t)nlist);
  for (int32_t l = 0; l < nlist; ++l) sz[l] = f->off_host[l + 1] - f->off_host[l];
  std::sort(sz.begin(), sz.end(), [](int64_t a, int64_t b) { return a > b; });
  f->topsum.assign((size_t)nlist + 1, 0);
  for (int32_t l = 0; l < nlist; ++l) f->topsum[l + 1] = f->topsum[l] + sz[l];
}

static int ivff_nprobe(const mi_ivfflat* f, int32_t nprobe) {
  REQUIRE(nprobe <= f->nlist, "nprobe must be in [1, nlist = " + std::to_string(f->nlist) + "]");
  return MI_OK;
}

// The index over gallery g (its lock is held): centroids onto the device, then the lists from `ids` (int32 [n] in `memspace`), or,
// with ids NULL, from the assignment of every stored row to its best centroid.  Synchronous
static int ivff_make(mi_gallery* g, const float* centroids, int32_t nlist, const int32_t* ids, int memspace, mi_ivfflat** out) {
  const int64_t n = g->n;
  const int32_t d = g->ud, dp = g->dp;
  REQUIRE(n >= 1, "the gallery holds no rows");
  REQUIRE(n <= 0x7fffffff, "an IVF-Flat index takes at most 2^31 - 1 rows");
  for (size_t i = 0, cnt = (size_t)nlist * d; i < cnt; ++i) REQUIRE(std::isfinite(centroids[i]), "centroids must be finite");
  if (ids && memspace == MI_HOST)
    for (int64_t i = 0; i < n; ++i) REQUIRE(ids[i] >= 0 && ids[i] < nlist, "list ids must lie in [0, nlist)");
  HIPC(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  int rc;
  if ((rc = join_tails(g, s)) != MI_OK) return rc;
  mi_ivfflat* f = new mi_ivfflat();
  f->rows = g, f->n = n, f->removals = g->removals, f->d = d, f->nlist = nlist;
  const int64_t brows = ivff_block_rows(n), nb = (n + brows - 1) / brows;
  const int64_t chunk = ivff_assign_chunk(n, nlist);
  DeviceBuf<int32_t> lid;                        // (these free themselves on return; every path out of here has synchronised `s`)
  DeviceBuf<uint32_t> hist, sizes;
  DeviceBuf<double> val;
  DeviceBuf<int64_t> best;
  auto bail = [&](int code) {
    (void)hipStreamSynchronize(s);
    delete f;
    return code;
  };
  if ((rc = f->cent.grow_exact((size_t)nlist * dp)) != MI_OK || (rc = f->iota.grow_exact((size_t)nlist)) != MI_OK ||
      (rc = f->list_off.grow_exact((size_t)nlist + 1)) != MI_OK || (rc = f->list_rows.grow_exact((size_t)n)) != MI_OK ||
      (rc = f->flag.grow_exact(64)) != MI_OK || (rc = hist.grow_exact((size_t)nlist * nb)) != MI_OK ||
      (rc = sizes.grow_exact((size_t)nlist)) != MI_OK)
    return bail(rc);
  if (!(ids && memspace == MI_DEVICE) && (rc = lid.grow_exact((size_t)n)) != MI_OK) return bail(rc);
  if (!ids && ((rc = val.grow_exact((size_t)chunk * nlist)) != MI_OK || (rc = best.grow_exact((size_t)chunk)) != MI_OK)) return bail(rc);
  std::vector<float> padded((size_t)nlist * dp, 0.0f);
  std::vector<int64_t> seq((size_t)nlist);
  for (int32_t l = 0; l < nlist; ++l) {
    std::memcpy(padded.data() + (size_t)l * dp, centroids + (size_t)l * d, (size_t)d * 4);
    seq[l] = l;
  }
  hipError_t e = hipMemcpyAsync(f->cent, padded.data(), padded.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(f->iota, seq.data(), seq.size() * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(f->flag, 0, 256, s);
  if (e == hipSuccess && ids && memspace == MI_HOST) e = hipMemcpyAsync(lid, ids, (size_t)n * 4, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return bail(fail(MI_ERR_HIP, std::string("IVF-Flat copy: ") + hipGetErrorString(e)));
  const int32_t* lids = lid;
  if (ids && memspace == MI_DEVICE) {
    lids = ids;
    launch_ivff_check(ids, nlist, n, f->flag, s);
    bool raised = false;
    if ((rc = check_flag(f->flag, s, &raised)) != MI_OK) return bail(rc);
    if (raised) return bail(fail(MI_ERR_INVALID, "list ids must lie in [0, nlist)"));
  }
  if (!ids) ivff_assign(f, 0, n, chunk, val, best, lid, s);
  launch_ivff_lists(lids, n, nlist, hist, sizes, f->list_off, f->list_rows, s);
  f->off_host.resize((size_t)nlist + 1);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(f->off_host.data(), f->list_off, ((size_t)nlist + 1) * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return bail(fail(MI_ERR_HIP, std::string("IVF-Flat build: ") + hipGetErrorString(e)));
  ivff_topsum(f);
  *out = f;
  return MI_OK;
}

// queries [nq][dp] in f->qpad (from `src`, device memory, any strides); then per chunk of queries: the probes (the library's by
// launch_refine over the centroids, or the caller's probes_dev [nq][nprobe]), their normal form and prefix and, with k >= 1, scan,
// selection and merge.  norm_out: NULL, or [nq][nprobe] for the normalised probes of every query.  All on `s`, no synchronisation
static int ivff_enqueue(mi_ivfflat* f, const void* src, int dtype, int64_t rs, int64_t cs, int64_t nq, int32_t k, int32_t nprobe,
                        const int32_t* probes_dev, const uint64_t* allow_dev, int32_t* norm_out, int64_t* out_idx, float* out_val,
                        double* out_val64, int64_t* out_scanned, hipStream_t s) {
  mi_gallery* g = f->rows;
  const int32_t nlist = f->nlist, dp = g->dp;
  const int64_t reach = f->topsum[nprobe];
  const int32_t nslab = (int32_t)std::max<int64_t>(1, (reach + IVFFLAT_SLAB_ROWS - 1) / IVFFLAT_SLAB_ROWS);
  const size_t per = (probes_dev ? 0 : (size_t)nlist * 8 + (size_t)nprobe * 8) + (norm_out ? 0 : (size_t)nprobe * 4) +
                     ((size_t)nprobe + 1) * 4 + (k ? (size_t)nslab * ((size_t)k * 16 + 4) : 0);
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nq, 65535), (int64_t)(IVFF_STAGE_BYTES / per)));
  int rc;
  if ((rc = f->qpad.grow((size_t)nq * dp)) != MI_OK || (rc = f->pref.grow((size_t)chunk * (nprobe + 1))) != MI_OK) return rc;
  if (!probes_dev && ((rc = f->pval.grow((size_t)chunk * nlist)) != MI_OK || (rc = f->pidx.grow((size_t)chunk * nprobe)) != MI_OK)) return rc;
  if (!norm_out && (rc = f->norm.grow((size_t)chunk * nprobe)) != MI_OK) return rc;
  if (k && ((rc = f->part_key.grow((size_t)chunk * nslab * k)) != MI_OK || (rc = f->part_id.grow((size_t)chunk * nslab * k)) != MI_OK ||
            (rc = f->pcnt.grow((size_t)chunk * nslab)) != MI_OK))
    return rc;
  const int l2 = g->metric == MI_METRIC_L2 ? 1 : 0;
  launch_l2_augment(src, dtype, nq, g->ud, rs, cs, f->qpad, dp, s);
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t b = std::min<int64_t>(chunk, nq - q0);
    const float* q = f->qpad + (size_t)q0 * dp;
    int32_t* nm = norm_out ? norm_out + q0 * nprobe : f->norm.get();
    if (probes_dev) {
      launch_ivff_prefix(probes_dev + q0 * nprobe, 0, b, nlist, nprobe, f->list_off, nm, f->pref, s);
    } else {
      launch_refine(f->cent, q, dp, g->ud, nlist, 0, l2, f->iota, nlist, 0, nprobe, b, f->pval, f->pidx, nullptr, nullptr, s);
      launch_ivff_prefix(f->pidx, 1, b, nlist, nprobe, f->list_off, nm, f->pref, s);
    }
    if (k)
      launch_ivff_search(g->gal_f32, q, dp, g->ud, l2, f->list_off, f->list_rows, nm, f->pref, nprobe, allow_dev, k, nslab, (int32_t)b,
                         f->part_key, f->part_id, f->pcnt, g->row_offset, out_idx + q0 * k, out_val ? out_val + q0 * k : nullptr,
                         out_val64 ? out_val64 + q0 * k : nullptr, out_scanned ? out_scanned + q0 : nullptr, s);
  }
  HIPC(hipGetLastError());
  return MI_OK;
}

extern "C" {

int mi_ivfflat_build(mi_gallery* rows, const float* centroids, int32_t nlist, mi_ivfflat** out) {
  int rc = ivff_make_check(rows, centroids, nlist, out);
  if (rc != MI_OK) return rc;
  std::lock_guard<std::mutex> lock(rows->mu);
  return ivff_make(rows, centroids, nlist, nullptr, MI_HOST, out);
}

int mi_ivfflat_create(mi_gallery* rows, const float* centroids, int32_t nlist, const int32_t* list_ids, int memspace, mi_ivfflat** out) {
  int rc = ivff_make_check(rows, centroids, nlist, out);
  if (rc != MI_OK) return rc;
  REQUIRE(list_ids, "null pointer: list_ids");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  std::lock_guard<std::mutex> lock(rows->mu);
  return ivff_make(rows, centroids, nlist, list_ids, memspace, out);
}

int mi_ivfflat_info(const mi_ivfflat* f, int64_t* n, int32_t* d, int32_t* nlist, int64_t* hbm_bytes) {
  REQUIRE(f, "null handle");
  if (n) *n = f->n;
  if (d) *d = f->d;
  if (nlist) *nlist = f->nlist;
  if (hbm_bytes) *hbm_bytes = (int64_t)f->bufs.bytes();
  return MI_OK;
}

int mi_ivfflat_list_sizes(mi_ivfflat* f, int64_t* out_sizes) {
  REQUIRE(f, "null handle");
  REQUIRE(out_sizes, "null pointer: out_sizes");
  for (int32_t l = 0; l < f->nlist; ++l) out_sizes[l] = f->off_host[l + 1] - f->off_host[l];
  return MI_OK;
}

int mi_ivfflat_get_lists(mi_ivfflat* f, int64_t* out_list_off, int32_t* out_list_rows) {
  REQUIRE(f, "null handle");
  REQUIRE(out_list_off || out_list_rows, "null pointer: out_list_off and out_list_rows");
  if (out_list_off) std::memcpy(out_list_off, f->off_host.data(), ((size_t)f->nlist + 1) * 8);
  if (!out_list_rows) return MI_OK;
  std::lock_guard<std::mutex> lock(f->mu);
  HIPC(hipSetDevice(f->rows->device));
  HIPC(hipMemcpy(out_list_rows, f->list_rows, (size_t)f->n * 4, hipMemcpyDeviceToHost));
  return MI_OK;
}

int mi_ivfflat_get_centroids(mi_ivfflat* f, float* out_host) {
  REQUIRE(f, "null handle");
  REQUIRE(out_host, "null pointer: out");
  std::lock_guard<std::mutex> lock(f->mu);
  HIPC(hipSetDevice(f->rows->device));
  HIPC(hipMemcpy2D(out_host, (size_t)f->d * 4, f->cent, (size_t)f->rows->dp * 4, (size_t)f->d * 4, (size_t)f->nlist, hipMemcpyDeviceToHost));
  return MI_OK;
}

int mi_ivfflat_destroy(mi_ivfflat* f) {
  if (!f) return MI_OK;
  (void)hipSetDevice(f->rows->device);
  (void)hipDeviceSynchronize();
  delete f;
  return MI_OK;
}

// The new tables take the place of the old ones (new_off has been read into off_host and `s` synchronised): the memory moves, the
// old blocks are freed, the host mirrors follow
static void ivff_swap_in(mi_ivfflat* f, int64_t n, std::vector<int64_t>& off_host, DeviceBuf<int64_t>& new_off, DeviceBuf<int32_t>& new_rows) {
  f->list_off = std::move(new_off);
  f->list_rows = std::move(new_rows);
  f->off_host.swap(off_host);
  f->n = n;
  ivff_topsum(f);
}

int mi_ivfflat_sync(mi_ivfflat* f, int64_t* out_added) {
  REQUIRE(f, "null handle");
  if (out_added) *out_added = 0;
  mi_gallery* g = f->rows;
  std::lock_guard<std::mutex> glock(g->mu);
  std::lock_guard<std::mutex> lock(f->mu);
  int rc = ivff_no_outside_removal(f);
  if (rc != MI_OK) return rc;
  const int64_t n0 = f->n, n1 = g->n, m = n1 - n0;
  REQUIRE(m >= 0, "the gallery holds fewer rows than the index: build a new index");
  if (m == 0) return MI_OK;
  REQUIRE(n1 <= 0x7fffffff, "an IVF-Flat index takes at most 2^31 - 1 rows");
  HIPC(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  if ((rc = join_tails(g, s)) != MI_OK) return rc;
  const int32_t nlist = f->nlist;
  const int64_t brows = ivff_block_rows(m), nb = (m + brows - 1) / brows;
  const int64_t chunk = ivff_assign_chunk(m, nlist);
  // the lists of the appended rows alone, numbered from 0, then both spliced into tables of their own: until the swap the handle
  // holds what it held (these free themselves on return; every path out of here has synchronised `s`)
  DeviceBuf<int32_t> lid, tail_rows, new_rows;
  DeviceBuf<uint32_t> hist, sizes;
  DeviceBuf<double> val;
  DeviceBuf<int64_t> best, tail_off, new_off;
  if ((rc = lid.grow_exact((size_t)m)) != MI_OK || (rc = tail_rows.grow_exact((size_t)m)) != MI_OK ||
      (rc = new_rows.grow_exact((size_t)n1)) != MI_OK || (rc = hist.grow_exact((size_t)nlist * nb)) != MI_OK ||
      (rc = sizes.grow_exact((size_t)nlist)) != MI_OK || (rc = val.grow_exact((size_t)chunk * nlist)) != MI_OK ||
      (rc = best.grow_exact((size_t)chunk)) != MI_OK || (rc = tail_off.grow_exact((size_t)nlist + 1)) != MI_OK ||
      (rc = new_off.grow_exact((size_t)nlist + 1)) != MI_OK)
    return rc;
  ivff_assign(f, n0, n1, chunk, val, best, lid, s);
  launch_ivff_lists(lid, m, nlist, hist, sizes, tail_off, tail_rows, s);
  launch_ivff_splice(f->list_off, f->list_rows, tail_off, tail_rows, nlist, n0, m, new_off, new_rows, s);
  std::vector<int64_t> off_host((size_t)nlist + 1);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(off_host.data(), new_off, ((size_t)nlist + 1) * 8, hipMemcpyDeviceToHost, s);
  const hipError_t es = hipStreamSynchronize(s);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(MI_ERR_HIP, std::string("IVF-Flat sync: ") + hipGetErrorString(e));
  ivff_swap_in(f, n1, off_host, new_off, new_rows);
  if (out_added) *out_added = m;
  return MI_OK;
}

int mi_ivfflat_remove_rows(mi_ivfflat* f, const uint64_t* remove_bits, int memspace, int64_t* out_removed) {
  REQUIRE(f, "null handle");
  REQUIRE(remove_bits, "null pointer: remove_bits");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  if (out_removed) *out_removed = 0;
  mi_gallery* g = f->rows;
  REQUIRE(g->online_users.load() == 0, "the gallery is in use by an online handle: mi_online_destroy comes first");
  std::lock_guard<std::mutex> glock(g->mu);
  std::lock_guard<std::mutex> lock(f->mu);
  int rc = ivff_fresh(f);
  if (rc != MI_OK) return rc;
  const int64_t n = f->n;
  HIPC(hipSetDevice(g->device));
  RemovePlan plan;                                          // the bitmap of the rows that stay and its rank table, on the host
  if ((rc = remove_plan(remove_bits, memspace, n, &plan)) != MI_OK) return rc;
  if (plan.removed == 0) return MI_OK;                      // nothing changes
  REQUIRE(plan.removed < n, "the bitmap names every row: an index needs at least one row");
  hipStream_t s = g->stream;
  if ((rc = join_tails(g, s)) != MI_OK) return rc;
  const int32_t nlist = f->nlist;
  const int64_t m = n - plan.removed, nwords = (n + 63) / 64;
  const int64_t brows = ivff_block_rows(n), nb = (n + brows - 1) / brows;
  // First the lists of the survivors, into tables of their own; then the gallery's removal; then the swap.  A removal the gallery
  // refuses or fails leaves the handle with what it held
  DeviceBuf<uint64_t> keep;
  DeviceBuf<uint32_t> rank, tpre, bcnt, total;
  DeviceBuf<int64_t> new_off;
  DeviceBuf<int32_t> new_rows;
  if ((rc = keep.grow_exact((size_t)nwords)) != MI_OK || (rc = rank.grow_exact((size_t)nwords + 1)) != MI_OK ||
      (rc = tpre.grow_exact((size_t)((n + 255) / 256))) != MI_OK || (rc = bcnt.grow_exact((size_t)nb)) != MI_OK ||
      (rc = total.grow_exact(64)) != MI_OK || (rc = new_off.grow_exact((size_t)nlist + 1)) != MI_OK ||
      (rc = new_rows.grow_exact((size_t)m)) != MI_OK)
    return rc;
  std::vector<int64_t> off_host((size_t)nlist + 1);
  hipError_t e = hipMemcpyAsync(keep, plan.keep.data(), (size_t)nwords * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(rank, plan.prefix.data(), ((size_t)nwords + 1) * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    launch_ivff_compact(f->list_off, f->list_rows, n, nlist, keep, rank, tpre, bcnt, total, new_off, new_rows, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(off_host.data(), new_off, ((size_t)nlist + 1) * 8, hipMemcpyDeviceToHost, s);
  const hipError_t es = hipStreamSynchronize(s);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(MI_ERR_HIP, std::string("IVF-Flat remove: ") + hipGetErrorString(e));
  if (off_host[(size_t)nlist] != m) return fail(MI_ERR_HIP, "IVF-Flat remove: the lists do not hold every row of the gallery");
  // the caller's bitmap has been read once: the gallery removes by the same bits (those at or beyond n are ignored there)
  for (uint64_t& w : plan.keep) w = ~w;
  int64_t removed = 0;
  if ((rc = gallery_remove_rows_locked(g, plan.keep.data(), MI_HOST, &removed)) != MI_OK) return rc;
  ivff_swap_in(f, m, off_host, new_off, new_rows);
  f->removals = g->removals;
  if (out_removed) *out_removed = removed;
  return MI_OK;
}

int mi_ivfflat_probe_device(mi_ivfflat* f, const float* q_dev, int64_t nq, int32_t nprobe, int32_t* out_probes_dev, void* stream) {
  REQUIRE(f, "null handle");
  REQUIRE(nprobe >= 1 && nprobe <= IVFF_MAX_LISTS, "nprobe must be in [1, nlist]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nq == 0 || q_dev, "null pointer: queries");
  REQUIRE(nq == 0 || out_probes_dev, "null pointer: out_probes");
  if (nq == 0) return MI_OK;
  int rc;
  if ((rc = ivff_nprobe(f, nprobe)) != MI_OK) return rc;
  if ((rc = ivff_fresh(f)) != MI_OK) return rc;
  HIPC(hipSetDevice(f->rows->device));
  return ivff_enqueue(f, q_dev, MI_F32, f->rows->ud, 1, nq, 0, nprobe, nullptr, nullptr, out_probes_dev, nullptr, nullptr, nullptr, nullptr,
                      (hipStream_t)stream);
}

int mi_ivfflat_search_device(mi_ivfflat* f, const float* q_dev, int64_t nq, int32_t k, int32_t nprobe, const int32_t* probes_dev,
                             const uint64_t* allow_dev, int64_t* out_idx_dev, float* out_val_dev, double* out_val64_dev,
                             int64_t* out_scanned_dev, void* stream) {
  int rc = ivff_search_check(f, nq, k, nprobe);
  if (rc != MI_OK) return rc;
  REQUIRE(nq == 0 || q_dev, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx_dev, "null pointer: out_idx");
  if (nq == 0) return MI_OK;
  if ((rc = ivff_nprobe(f, nprobe)) != MI_OK) return rc;
  if ((rc = ivff_fresh(f)) != MI_OK) return rc;
  HIPC(hipSetDevice(f->rows->device));
  return ivff_enqueue(f, q_dev, MI_F32, f->rows->ud, 1, nq, k, nprobe, probes_dev, allow_dev, nullptr, out_idx_dev, out_val_dev,
                      out_val64_dev, out_scanned_dev, (hipStream_t)stream);
}

}  // extern "C"
