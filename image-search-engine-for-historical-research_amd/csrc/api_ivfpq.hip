// IVF index over PQ codes of the C ABI (mi_ivfpq; kernels in csrc/ivfpq.hip): the reference's
// matching_PQ_Net_bucket (src/utils/nnsearch.py:949-998), faiss IndexIVFPQ with by_residual = false.  A handle of its own: coarse
// centroids, codebooks, a pool of 64-slot blocks chained into lists, and grow-only staging.  The HOST decides where a row goes
// (the next free slot of its list; a new block from the pool when the tail is full) and keeps, per list, its block numbers and,
// per row, its slot and list; after every create / append / add it uploads the flattened block table and list_off.  The answer
// is a function of the inputs alone: the exact ADC top-K of mi_pq_search over the rows whose list is probed.
// A RESIDUAL index (mi_ivfpq_create_residual; kernels in csrc/ivfpq_residual.hip) is faiss's by_residual = true: the
// same handle, lists and blocks, but a code quantizes double(x) - double(G[list]) and a query has one table per probed list.  The
// kind is fixed at creation; `tab` then holds [queries of a chunk][nprobe][m][ks].
#include "api_internal.h"

struct mi_ivfpq {
  int device = 0;
  int64_t n = 0, cap = 0, row_offset = 0;
  int32_t d = 0, m = 0, ks = 0, L = 0, MQ = 0, nlist = 0;
  bool residual = false;                           // codes quantize the residual against the row's list
  std::vector<float> cb_host, coarse_host;         // [m][ks][L], [nlist][d]
  DeviceBufSet bufs;                               // every device allocation of the handle: hbm_bytes is bufs.bytes()
  DeviceBuf<float> cb{bufs}, coarse{bufs};         // (down to `flag`: exactly their size, allocated at creation)
  int64_t pool_blocks = 0, pool_used = 0;          // ceil(cap / 64) + nlist: every list may end in a partly filled block
  std::vector<uint32_t> free_blocks;               // blocks below pool_used that a removal emptied: taken first, last in first out
  DeviceBuf<uint32_t> codes{bufs};                 // [pool_blocks][MQ][64]
  DeviceBuf<uint32_t> rowid{bufs};                 // [pool_blocks][64]
  DeviceBuf<uint32_t> blk_table{bufs};             // [pool_blocks]: the blocks of list 0, of list 1, ...
  DeviceBuf<int32_t> list_off{bufs};               // [nlist + 1] into blk_table, followed by
  uint32_t* list_rows = nullptr;                   // [nlist] rows per list (the same allocation)
  std::vector<std::vector<uint32_t>> blocks;       // per list
  std::vector<int64_t> list_size;                  // rows per list
  std::vector<int64_t> slot_of_row;                // pblock * 64 + lane
  std::vector<uint8_t> list_of_row;
  DeviceBuf<uint32_t> flag{bufs};                  // (256 bytes)
  hipStream_t stream = nullptr;
  DeviceBuf<char> xraw{bufs};                      // rows / queries of a host call, packed [rows][d] in their own type
  DeviceBuf<uint8_t> cbytes{bufs}, lbytes{bufs};   // packed code bytes [rows][m] and list ids [rows] on their way in
  DeviceBuf<int64_t> slots{bufs};
  DeviceBuf<float> tab{bufs};                      // [queries of a chunk][m][ks]; residual: [queries of a chunk][nprobe][m][ks]
  DeviceBuf<int32_t> praw{bufs}, pnorm{bufs}, pref{bufs}, pex{bufs};   // probes: chosen, normalised, prefix; a host call's own
  DeviceBuf<uint64_t> part{bufs};                  // [queries of a chunk][slabs][k]
  DeviceBuf<uint64_t> bits{bufs};
  DeviceBuf<uint32_t> rmpref{bufs};                // mi_ivfpq_remove_rows: prefix counts per bitmap word
  DeviceBuf<int64_t> oidx{bufs};
  DeviceBuf<float> odist{bufs};
  std::mutex mu;
};

// ---- host bookkeeping.  A failed call puts the lists back: rows it already scattered sit in slots beyond their list's fill,
// which the scan does not admit and the next append overwrites
struct IvfMark {
  int64_t n, pool_used;
  std::vector<int64_t> list_size;
  std::vector<uint32_t> free_blocks;
};

static IvfMark ivf_mark(const mi_ivfpq* h) { return {h->n, h->pool_used, h->list_size, h->free_blocks}; }

// the blocks the failed call took, from the free list or from the end of the pool, go back where they came from: the chains are
// cut to the marked fills below, so none of them is in a chain any more
static void ivf_rollback(mi_ivfpq* h, const IvfMark& mk) {
  h->pool_used = mk.pool_used;
  h->free_blocks = mk.free_blocks;
  h->list_size = mk.list_size;
  for (int32_t l = 0; l < h->nlist; ++l) h->blocks[l].resize((size_t)((mk.list_size[l] + 63) / 64));
  h->slot_of_row.resize((size_t)mk.n);
  h->list_of_row.resize((size_t)mk.n);
}

// the slots of `rows` more rows with the given lists, in row order.  A new block is one a removal emptied, if there is one, else
// the next of the pool: the pool grows only while every block below pool_used is in a chain, and the chains hold
// sum ceil(list_size / 64) <= n / 64 + nlist blocks, so pool_used stays within pool_blocks after any removals and appends
static void ivf_place(mi_ivfpq* h, const uint8_t* lists, int64_t rows, int64_t* slots) {
  for (int64_t r = 0; r < rows; ++r) {
    const int32_t l = lists[r];
    const int64_t fill = h->list_size[l]++;
    if ((fill & 63) == 0) {
      if (h->free_blocks.empty()) h->blocks[l].push_back((uint32_t)h->pool_used++);
      else h->blocks[l].push_back(h->free_blocks.back()), h->free_blocks.pop_back();
    }
    slots[r] = (int64_t)h->blocks[l].back() * 64 + (fill & 63);
    h->slot_of_row.push_back(slots[r]);
    h->list_of_row.push_back((uint8_t)l);
  }
}

// block table, list_off and list_rows -> device, synchronous
static int ivf_publish(mi_ivfpq* h) {
  std::vector<uint32_t> flat;
  std::vector<int32_t> off(2 * (size_t)h->nlist + 1, 0);
  flat.reserve((size_t)h->pool_used);
  for (int32_t l = 0; l < h->nlist; ++l) {
    flat.insert(flat.end(), h->blocks[l].begin(), h->blocks[l].end());
    off[l + 1] = (int32_t)flat.size();
    off[h->nlist + 1 + l] = (int32_t)(uint32_t)h->list_size[l];
  }
  if (!flat.empty()) HIPC(hipMemcpyAsync(h->blk_table, flat.data(), flat.size() * 4, hipMemcpyHostToDevice, h->stream));
  HIPC(hipMemcpyAsync(h->list_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  return MI_OK;
}

// code bytes of `rows` rows at src (device, row stride `stride`) whose lists are lists_host -> the index, behind the rows that
// are there (h->n does not move).  Synchronous.
static int ivf_scatter_rows(mi_ivfpq* h, const uint8_t* src_dev, int64_t stride, const uint8_t* lists_host, int64_t row0, int64_t rows,
                            std::vector<int64_t>& slots) {
  int rc;
  slots.resize((size_t)rows);
  ivf_place(h, lists_host, rows, slots.data());
  // cannot happen while ivf_place's bound holds; a slot beyond the pool must never reach the scatter
  REQUIRE(h->pool_used <= h->pool_blocks, "internal: the block pool is exhausted");
  if ((rc = h->slots.grow((size_t)rows)) != MI_OK) return rc;
  HIPC(hipMemcpyAsync(h->slots, slots.data(), (size_t)rows * 8, hipMemcpyHostToDevice, h->stream));
  launch_ivf_scatter(src_dev, stride, h->m, h->slots, row0, rows, h->codes, h->rowid, h->stream);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(h->stream));
  return MI_OK;
}

// rows of code bytes with their list ids (host: checked by the caller; device: checked here, before anything is ingested)
static int ivf_ingest(mi_ivfpq* h, const void* codes, const uint8_t* list_ids, int64_t rows, int64_t stride, int memspace) {
  hipStream_t s = h->stream;
  int rc;
  std::vector<uint8_t> lists_back;
  if (memspace == MI_DEVICE) {
    bool bad_code = false, bad_list = false;
    if (h->ks < 256) launch_pq_check((const uint8_t*)codes, stride, h->m, h->ks, rows, h->flag, s);
    if ((rc = check_flag(h->flag, s, &bad_code)) != MI_OK) return rc;
    if (!bad_code && h->nlist < 256) {
      launch_ivf_check(list_ids, h->nlist, rows, h->flag, s);
      if ((rc = check_flag(h->flag, s, &bad_list)) != MI_OK) return rc;
    }
    if (bad_code || bad_list) return fail(MI_ERR_INVALID, bad_code ? "a code byte is >= ks" : "a list id is >= nlist");
    lists_back.resize((size_t)rows);
    HIPC(hipMemcpy(lists_back.data(), list_ids, (size_t)rows, hipMemcpyDeviceToHost));
    list_ids = lists_back.data();
  }
  const IvfMark mk = ivf_mark(h);
  const int64_t step = std::max<int64_t>(1, ((int64_t)64 << 20) / h->m);
  std::vector<int64_t> slots;
  rc = MI_OK;
  if (memspace == MI_HOST) rc = h->cbytes.grow((size_t)std::min(step, rows) * h->m);
  for (int64_t r = 0; r < rows && rc == MI_OK; r += step) {
    const int64_t mm = std::min(step, rows - r);
    const uint8_t* src = (const uint8_t*)codes + r * stride;
    auto upload = [&]() -> int {
      if (stride == h->m || mm == 1) HIPC(hipMemcpyAsync(h->cbytes, src, (size_t)mm * h->m, hipMemcpyHostToDevice, s));
      else HIPC(hipMemcpy2DAsync(h->cbytes, (size_t)h->m, src, (size_t)stride, (size_t)h->m, (size_t)mm, hipMemcpyHostToDevice, s));
      return MI_OK;
    };
    if (memspace == MI_HOST) {
      if ((rc = upload()) != MI_OK) break;
      rc = ivf_scatter_rows(h, h->cbytes, h->m, list_ids + r, h->n + r, mm, slots);
    } else {
      rc = ivf_scatter_rows(h, src, stride, list_ids + r, h->n + r, mm, slots);
    }
  }
  if (rc == MI_OK) rc = ivf_publish(h);
  if (rc != MI_OK) {
    ivf_rollback(h, mk);
    return rc;
  }
  h->n += rows;
  return MI_OK;
}

// the `nprobe` largest lists' blocks, in slabs of 64: what the grid of the scan has to cover for ANY choice of probes
static int64_t ivf_slab_bound(const mi_ivfpq* h, int32_t nprobe) {
  std::vector<int64_t> c((size_t)h->nlist);
  for (int32_t l = 0; l < h->nlist; ++l) c[l] = (int64_t)h->blocks[l].size();
  std::partial_sort(c.begin(), c.begin() + nprobe, c.end(), std::greater<int64_t>());
  int64_t tot = 0;
  for (int32_t i = 0; i < nprobe; ++i) tot += c[i];
  return (tot + 63) / 64;
}

// the search proper on stream s: queries on the device (any strides), probes_dev NULL or [nq][nprobe], results to device buffers
static int ivf_search_core(mi_ivfpq* h, const void* q_dev, int dtype, int64_t rs, int64_t cs, int64_t nq, int32_t k, int32_t nprobe,
                           const int32_t* probes_dev, const uint64_t* allow_dev, int64_t* out_idx_dev, float* out_dist_dev, hipStream_t s,
                           float* stage_ms = nullptr) {
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  const int64_t nslab = ivf_slab_bound(h, nprobe);
  const int64_t per = (int64_t)h->m * h->ks;
  // queries per pass: the partial lists within the budget, the tables within 256 MiB, the grid's y below 65536; one at the least.
  // A residual index has nprobe tables per query and keeps tables + partial lists within the budget
  const int64_t budget = g_pq_matrix_bytes.load();
  const int64_t tabs = h->residual ? per * nprobe : per;
  int64_t qc = h->residual ? std::min<int64_t>({nq, 65535, budget / (nslab * k * 8 + tabs * 4)})
                           : std::min<int64_t>({nq, 65535, budget / std::max<int64_t>(1, nslab * k * 8), ((int64_t)256 << 20) / (per * 4)});
  qc = std::max<int64_t>(1, qc);
  int rc;
  if ((rc = h->tab.grow((size_t)(qc * tabs))) != MI_OK) return rc;
  if ((rc = h->praw.grow((size_t)(qc * nprobe))) != MI_OK) return rc;
  if ((rc = h->pnorm.grow((size_t)(qc * nprobe))) != MI_OK) return rc;
  if ((rc = h->pref.grow((size_t)(qc * (nprobe + 1)))) != MI_OK) return rc;
  if ((rc = h->part.grow((size_t)(qc * nslab * k))) != MI_OK) return rc;
  // stage_ms (mi_ivfpq_search_stages_device): HIP events around the table and the scan of every chunk, read after each chunk
  // the guard destroys them on every way out of this function
  struct StageEvents {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~StageEvents() {
      for (hipEvent_t x : e)
        if (x) (void)hipEventDestroy(x);
    }
  } guard;
  hipEvent_t* ev = guard.e;
  if (stage_ms) {
    stage_ms[0] = stage_ms[1] = 0.0f;
    for (int i = 0; i < 3; ++i) HIPC(hipEventCreate(&ev[i]));
  }
  for (int64_t q0 = 0; q0 < nq; q0 += qc) {
    const int32_t b = (int32_t)std::min<int64_t>(qc, nq - q0);
    const char* qp = (const char*)q_dev + (size_t)q0 * rs * esz;
    const int32_t* in = probes_dev ? probes_dev + q0 * nprobe : h->praw;
    if (!probes_dev) launch_ivf_probe(qp, dtype, rs, cs, b, h->coarse, h->nlist, h->d, nprobe, h->praw, s);
    launch_ivf_prefix(in, b, h->nlist, nprobe, h->list_off, h->pnorm, h->pref, s);
    if (stage_ms) HIPC(hipEventRecord(ev[0], s));
    if (h->residual) {
      launch_ivfr_table(qp, dtype, rs, cs, b, h->coarse, h->d, h->cb, h->m, h->ks, h->L, h->pnorm, nprobe, h->tab, s);
      if (stage_ms) HIPC(hipEventRecord(ev[1], s));
      launch_ivfr_scan_select(h->codes, h->rowid, h->blk_table, h->list_off, h->m, h->ks, h->tab, h->pnorm, h->pref, nprobe, b, h->list_rows,
                              allow_dev, k, (int32_t)nslab, h->part, s);
    } else {
      launch_pq_table(qp, dtype, rs, cs, b, h->cb, h->m, h->ks, h->L, h->tab, s);
      if (stage_ms) HIPC(hipEventRecord(ev[1], s));
      launch_ivf_scan_select(h->codes, h->rowid, h->blk_table, h->list_off, h->m, h->ks, h->tab, h->pnorm, h->pref, nprobe, b, h->list_rows,
                             allow_dev, k, (int32_t)nslab, h->part, s);
    }
    if (stage_ms) {
      float t = 0.0f, u = 0.0f;
      HIPC(hipEventRecord(ev[2], s));
      HIPC(hipEventSynchronize(ev[2]));
      HIPC(hipEventElapsedTime(&t, ev[0], ev[1]));
      HIPC(hipEventElapsedTime(&u, ev[1], ev[2]));
      stage_ms[0] += t;
      stage_ms[1] += u;
    }
    launch_ivf_merge(h->part, h->pref, nprobe, b, k, (int32_t)nslab, h->row_offset, out_idx_dev + q0 * k,
                     out_dist_dev ? out_dist_dev + q0 * k : nullptr, s);
  }
  HIPC(hipGetLastError());
  return MI_OK;
}

// mi_ivfpq_create and mi_ivfpq_create_residual: one body, the kind is the only difference
static int ivf_create(bool residual, const float* coarse_host, int32_t nlist, const float* codebooks_host, int32_t d, int32_t m, int32_t ks,
                      const void* codes, const uint8_t* list_ids, int64_t n, int64_t row_stride_bytes, int memspace, int device,
                      int64_t row_offset, int64_t capacity, mi_ivfpq** out) {
  REQUIRE(out, "null pointer: out");
  REQUIRE(coarse_host, "null pointer: coarse_host");
  REQUIRE(codebooks_host, "null pointer: codebooks_host");
  REQUIRE(nlist >= 2 && nlist <= 256, "nlist (lists) must be in [2, 256]");
  REQUIRE(m >= 1 && m <= 64, "m (books) must be in [1, 64]");
  REQUIRE(ks >= 2 && ks <= 256, "ks (codewords per book) must be in [2, 256]");
  REQUIRE(d >= 1 && d <= 4096, "d must be in [1, 4096]");
  REQUIRE(d % m == 0, "d must be a multiple of m");
  REQUIRE(n >= 0, "negative number of rows");
  REQUIRE(capacity >= 0, "negative capacity");
  REQUIRE(capacity == 0 || capacity >= n, "capacity below the number of rows");
  REQUIRE(codes || n == 0, "null pointer: codes");
  REQUIRE(list_ids || n == 0, "null pointer: list_ids");
  REQUIRE(n >= 1 || capacity >= 1, "an empty index needs a capacity");
  REQUIRE(n == 0 || row_stride_bytes >= m, "row_stride_bytes below m");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  if (capacity == 0) capacity = n;
  REQUIRE(capacity < ((int64_t)1 << 32) - 1, "an index holds fewer than 2^32 - 1 rows");
  const size_t cb_count = (size_t)ks * d, co_count = (size_t)nlist * d;
  for (size_t i = 0; i < co_count; ++i) REQUIRE(std::isfinite(coarse_host[i]), "coarse centroids must be finite");
  for (size_t i = 0; i < cb_count; ++i) REQUIRE(std::isfinite(codebooks_host[i]), "codebooks must be finite");
  REQUIRE(memspace != MI_HOST || codes_below((const uint8_t*)codes, n, row_stride_bytes, m, ks), "a code byte is >= ks");
  REQUIRE(memspace != MI_HOST || codes_below(list_ids, n, 1, 1, nlist), "a list id is >= nlist");
  HIPC(hipSetDevice(device));
  mi_ivfpq* h = new mi_ivfpq();
  h->device = device;
  h->cap = capacity;
  h->row_offset = row_offset;
  h->d = d;
  h->m = m;
  h->ks = ks;
  h->L = d / m;
  h->MQ = (m + 3) / 4;
  h->nlist = nlist;
  h->residual = residual;
  h->cb_host.assign(codebooks_host, codebooks_host + cb_count);
  h->coarse_host.assign(coarse_host, coarse_host + co_count);
  h->blocks.resize((size_t)nlist);
  h->list_size.assign((size_t)nlist, 0);
  h->pool_blocks = (capacity + 63) / 64 + nlist;
  const size_t codes_bytes = (size_t)h->pool_blocks * h->MQ * 64 * 4, id_bytes = (size_t)h->pool_blocks * 64 * 4;
  auto cleanup = [&](int code) {
    mi_ivfpq_destroy(h);
    return code;
  };
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = h->codes.alloc(codes_bytes / 4);
  if (e == hipSuccess) e = h->rowid.alloc(id_bytes / 4);
  if (e == hipSuccess) e = h->blk_table.alloc((size_t)h->pool_blocks);
  if (e == hipSuccess) e = h->list_off.alloc(2 * (size_t)nlist + 1);
  if (e == hipSuccess) e = h->cb.alloc(cb_count);
  if (e == hipSuccess) e = h->coarse.alloc(co_count);
  if (e == hipSuccess) e = h->flag.alloc(64);
  if (e == hipSuccess) e = hipMemsetAsync(h->codes, 0, codes_bytes, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->rowid, 0xFF, id_bytes, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->blk_table, 0, (size_t)h->pool_blocks * 4, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->list_off, 0, (2 * (size_t)nlist + 1) * 4, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->flag, 0, 256, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->cb, h->cb_host.data(), cb_count * 4, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->coarse, h->coarse_host.data(), co_count * 4, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  h->list_rows = (uint32_t*)(h->list_off + nlist + 1);
  if (e != hipSuccess)
    return cleanup(fail(e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, std::string("IVF-PQ index: ") + hipGetErrorString(e)));
  if (n > 0) {
    const int rc = ivf_ingest(h, codes, list_ids, n, row_stride_bytes, memspace);
    if (rc != MI_OK) return cleanup(rc);
  }
  *out = h;
  return MI_OK;
}

extern "C" {

int mi_ivfpq_create(const float* coarse_host, int32_t nlist, const float* codebooks_host, int32_t d, int32_t m, int32_t ks, const void* codes,
                    const uint8_t* list_ids, int64_t n, int64_t row_stride_bytes, int memspace, int device, int64_t row_offset,
                    int64_t capacity, mi_ivfpq** out) {
  return ivf_create(false, coarse_host, nlist, codebooks_host, d, m, ks, codes, list_ids, n, row_stride_bytes, memspace, device, row_offset,
                    capacity, out);
}

int mi_ivfpq_create_residual(const float* coarse_host, int32_t nlist, const float* codebooks_host, int32_t d, int32_t m, int32_t ks,
                             const void* codes, const uint8_t* list_ids, int64_t n, int64_t row_stride_bytes, int memspace, int device,
                             int64_t row_offset, int64_t capacity, mi_ivfpq** out) {
  return ivf_create(true, coarse_host, nlist, codebooks_host, d, m, ks, codes, list_ids, n, row_stride_bytes, memspace, device, row_offset,
                    capacity, out);
}

int mi_ivfpq_is_residual(const mi_ivfpq* h, int32_t* out) {
  REQUIRE(h, "null handle");
  REQUIRE(out, "null pointer: out");
  *out = h->residual ? 1 : 0;
  return MI_OK;
}

int mi_ivfpq_append_codes(mi_ivfpq* h, const void* codes, const uint8_t* list_ids, int64_t rows, int64_t row_stride_bytes, int memspace) {
  REQUIRE(h, "null handle");
  REQUIRE(rows >= 0, "negative number of rows");
  REQUIRE(codes || rows == 0, "null pointer: codes");
  REQUIRE(list_ids || rows == 0, "null pointer: list_ids");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  REQUIRE(rows == 0 || row_stride_bytes >= h->m, "row_stride_bytes below m");
  std::lock_guard<std::mutex> lock(h->mu);
  REQUIRE(h->n + rows <= h->cap, "index capacity exceeded");
  if (rows == 0) return MI_OK;
  REQUIRE(memspace != MI_HOST || codes_below((const uint8_t*)codes, rows, row_stride_bytes, h->m, h->ks), "a code byte is >= ks");
  REQUIRE(memspace != MI_HOST || codes_below(list_ids, rows, 1, 1, h->nlist), "a list id is >= nlist");
  HIPC(hipSetDevice(h->device));
  return ivf_ingest(h, codes, list_ids, rows, row_stride_bytes, memspace);
}

int mi_ivfpq_add(mi_ivfpq* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace) {
  REQUIRE(h, "null handle");
  REQUIRE_ROWS(x, rows, dtype, row_stride, col_stride, memspace);
  std::lock_guard<std::mutex> lock(h->mu);
  REQUIRE(h->n + rows <= h->cap, "index capacity exceeded");
  if (rows == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  const int64_t step = std::max<int64_t>(64, ((int64_t)64 << 20) / ((int64_t)h->d * (int64_t)esz));
  hipStream_t s = h->stream;
  const IvfMark mk = ivf_mark(h);
  std::vector<char> pack;
  std::vector<uint8_t> lists;
  std::vector<int64_t> slots;
  // a block of rows: its codes (the encoder on the codebooks) and its lists (the encoder on ONE book, the coarse centroids); on a
  // residual index the lists come first and the codes are those of the residual against them
  auto block = [&](int64_t r, int64_t mm) -> int {
    int rc;
    const void* xp = (const char*)x + (size_t)r * row_stride * esz;
    int64_t rs = row_stride, cs = col_stride;
    if (memspace == MI_HOST) {
      if ((rc = stage_host_rows(h->xraw, h->d, h->stream, x, r, mm, dtype, row_stride, col_stride, pack)) != MI_OK) return rc;
      xp = h->xraw;
      rs = h->d;
      cs = 1;
    }
    if (!h->residual) launch_pq_encode(xp, dtype, rs, cs, mm, h->cb, h->m, h->ks, h->L, h->cbytes, s);
    launch_pq_encode(xp, dtype, rs, cs, mm, h->coarse, 1, h->nlist, h->d, h->lbytes, s);
    if (h->residual) launch_ivfr_encode(xp, dtype, rs, cs, mm, h->coarse, h->d, h->lbytes, h->cb, h->m, h->ks, h->L, h->cbytes, s);
    HIPC(hipGetLastError());
    lists.resize((size_t)mm);
    HIPC(hipMemcpyAsync(lists.data(), h->lbytes, (size_t)mm, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return ivf_scatter_rows(h, h->cbytes, h->m, lists.data(), mk.n + r, mm, slots);
  };
  int rc = h->cbytes.grow((size_t)std::min(step, rows) * h->m);
  if (rc == MI_OK) rc = h->lbytes.grow((size_t)std::min(step, rows));
  for (int64_t r = 0; r < rows && rc == MI_OK; r += step) rc = block(r, std::min(step, rows - r));
  if (rc == MI_OK) rc = ivf_publish(h);
  if (rc != MI_OK) {
    ivf_rollback(h, mk);
    return rc;
  }
  h->n = mk.n + rows;
  return MI_OK;
}

int mi_ivfpq_residual_rows(mi_ivfpq* h, const void* x, int64_t rows, int dtype, int64_t row_stride, int64_t col_stride, int memspace,
                           const uint8_t* list_ids, float* out, int out_memspace) {
  REQUIRE(h, "null handle");
  REQUIRE_ROWS(x, rows, dtype, row_stride, col_stride, memspace);
  REQUIRE(out || rows == 0, "null pointer: out");
  REQUIRE(out_memspace == MI_HOST || out_memspace == MI_DEVICE, "out_memspace must be MI_HOST or MI_DEVICE");
  if (rows == 0) return MI_OK;
  REQUIRE(!list_ids || memspace != MI_HOST || codes_below(list_ids, rows, 1, 1, h->nlist), "a list id is >= nlist");
  std::lock_guard<std::mutex> lock(h->mu);
  HIPC(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  int rc;
  if (list_ids && memspace == MI_DEVICE && h->nlist < 256) {
    bool bad_list;
    launch_ivf_check(list_ids, h->nlist, rows, h->flag, s);
    if ((rc = check_flag(h->flag, s, &bad_list)) != MI_OK) return rc;
    if (bad_list) return fail(MI_ERR_INVALID, "a list id is >= nlist");
  }
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  const int64_t step = std::max<int64_t>(64, ((int64_t)64 << 20) / ((int64_t)h->d * 8));
  const int64_t most = std::min(step, rows);
  if ((rc = h->lbytes.grow((size_t)most)) != MI_OK) return rc;
  if (out_memspace == MI_HOST && (rc = h->odist.grow((size_t)(most * h->d))) != MI_OK) return rc;
  std::vector<char> pack;
  for (int64_t r = 0; r < rows; r += step) {
    const int64_t mm = std::min(step, rows - r);
    const void* xp = (const char*)x + (size_t)r * row_stride * esz;
    int64_t rs = row_stride, cs = col_stride;
    if (memspace == MI_HOST) {
      if ((rc = stage_host_rows(h->xraw, h->d, h->stream, x, r, mm, dtype, row_stride, col_stride, pack)) != MI_OK) return rc;
      xp = h->xraw;
      rs = h->d;
      cs = 1;
    }
    const uint8_t* lp = h->lbytes;
    if (!list_ids) launch_pq_encode(xp, dtype, rs, cs, mm, h->coarse, 1, h->nlist, h->d, h->lbytes, s);
    else if (memspace == MI_HOST) HIPC(hipMemcpyAsync(h->lbytes, list_ids + r, (size_t)mm, hipMemcpyHostToDevice, s));
    else lp = list_ids + r;
    float* dst = out_memspace == MI_DEVICE ? out + r * h->d : h->odist;
    launch_ivfr_rows(xp, dtype, rs, cs, mm, h->coarse, h->d, lp, dst, s);
    HIPC(hipGetLastError());
    if (out_memspace == MI_HOST) HIPC(hipMemcpyAsync(out + r * h->d, h->odist, (size_t)(mm * h->d) * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
  }
  return MI_OK;
}

int mi_ivfpq_probe(mi_ivfpq* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t nprobe,
                   int32_t* out_lists_host) {
  REQUIRE(h, "null handle");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nprobe >= 1 && nprobe <= 256, "nprobe must be in [1, nlist]");
  REQUIRE(nq == 0 || (q && out_lists_host), "null pointer");
  REQUIRE(nprobe <= h->nlist, "nprobe must be in [1, nlist]");
  if (nq == 0) return MI_OK;
  int rc;
  if ((rc = check_host_queries(h->d, q, nq, dtype, row_stride, col_stride)) != MI_OK) return rc;
  std::lock_guard<std::mutex> lock(h->mu);
  HIPC(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  const int64_t step = std::max<int64_t>(1, ((int64_t)64 << 20) / ((int64_t)h->d * (int64_t)esz));
  if ((rc = h->praw.grow((size_t)(std::min(step, nq) * nprobe))) != MI_OK) return rc;
  std::vector<char> pack;
  for (int64_t q0 = 0; q0 < nq; q0 += step) {
    const int64_t b = std::min(step, nq - q0);
    if ((rc = stage_host_rows(h->xraw, h->d, h->stream, q, q0, b, dtype, row_stride, col_stride, pack)) != MI_OK) return rc;
    launch_ivf_probe(h->xraw, dtype, h->d, 1, b, h->coarse, h->nlist, h->d, nprobe, h->praw, s);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(out_lists_host + q0 * nprobe, h->praw, (size_t)(b * nprobe) * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
  }
  return MI_OK;
}

int mi_ivfpq_search(mi_ivfpq* h, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k, int32_t nprobe,
                    const int32_t* probes_host, const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_dist,
                    double* out_seconds) {
  REQUIRE(h, "null handle");
  REQUIRE(k >= 1 && k <= 2048, "k must be in [1, 2048]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nprobe >= 1 && nprobe <= 256, "nprobe must be in [1, nlist]");
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(!allow_bits || allow_memspace == MI_HOST || allow_memspace == MI_DEVICE, "allow_memspace must be MI_HOST or MI_DEVICE");
  if (out_seconds) *out_seconds = 0.0;
  // the entries are compared with the one-byte limit first and with the handle's nlist after it: no check before this line reads
  // the handle
  if (probes_host)
    for (int64_t i = 0; i < nq * nprobe; ++i)
      REQUIRE(probes_host[i] >= -1 && probes_host[i] < 256, "a probe entry is neither -1 nor in [0, nlist)");
  REQUIRE(nprobe <= h->nlist, "nprobe must be in [1, nlist]");
  if (nq == 0) return MI_OK;
  if (probes_host)
    for (int64_t i = 0; i < nq * nprobe; ++i) REQUIRE(probes_host[i] < h->nlist, "a probe entry is neither -1 nor in [0, nlist)");
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
  if (probes_host) {
    if ((rc = h->pex.grow((size_t)(nq * nprobe))) != MI_OK) return rc;
    HIPC(hipMemcpyAsync(h->pex, probes_host, (size_t)(nq * nprobe) * 4, hipMemcpyHostToDevice, s));
  }
  std::vector<char> pack;
  if ((rc = stage_host_rows(h->xraw, h->d, h->stream, q, 0, nq, dtype, row_stride, col_stride, pack)) != MI_OK) return rc;
  if ((rc = ivf_search_core(h, h->xraw, dtype, h->d, 1, nq, k, nprobe, probes_host ? h->pex.get() : nullptr, allow_dev, h->oidx,
                            out_dist ? h->odist.get() : nullptr, s)) != MI_OK)
    return rc;
  return topk_to_host(out_idx, h->oidx, out_dist, h->odist.get(), cnt, s, t0, out_seconds);
}

int mi_ivfpq_search_device(mi_ivfpq* h, const float* q_dev, int64_t nq, int32_t k, int32_t nprobe, const int32_t* probes_dev,
                           const uint64_t* allow_bits_dev, int64_t* out_idx_dev, float* out_dist_dev, void* stream) {
  REQUIRE(h, "null handle");
  REQUIRE(k >= 1 && k <= 2048, "k must be in [1, 2048]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nprobe >= 1 && nprobe <= 256, "nprobe must be in [1, nlist]");
  REQUIRE(nq == 0 || (q_dev && out_idx_dev), "null pointer");
  REQUIRE(nprobe <= h->nlist, "nprobe must be in [1, nlist]");
  if (nq == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  return ivf_search_core(h, q_dev, MI_F32, h->d, 1, nq, k, nprobe, probes_dev, allow_bits_dev, out_idx_dev, out_dist_dev, (hipStream_t)stream);
}

int mi_ivfpq_search_stages_device(mi_ivfpq* h, const float* q_dev, int64_t nq, int32_t k, int32_t nprobe, int64_t* out_idx_dev,
                                  float* out_dist_dev, void* stream, float* out_table_ms, float* out_scan_ms) {
  REQUIRE(h, "null handle");
  REQUIRE(k >= 1 && k <= 2048, "k must be in [1, 2048]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nprobe >= 1 && nprobe <= 256, "nprobe must be in [1, nlist]");
  REQUIRE(nq == 0 || (q_dev && out_idx_dev), "null pointer");
  REQUIRE(out_table_ms && out_scan_ms, "null pointer: out_table_ms / out_scan_ms");
  REQUIRE(nprobe <= h->nlist, "nprobe must be in [1, nlist]");
  float ms[2] = {0.0f, 0.0f};
  *out_table_ms = *out_scan_ms = 0.0f;
  if (nq == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  const int rc = ivf_search_core(h, q_dev, MI_F32, h->d, 1, nq, k, nprobe, nullptr, nullptr, out_idx_dev, out_dist_dev, (hipStream_t)stream, ms);
  if (rc != MI_OK) return rc;
  HIPC(hipStreamSynchronize((hipStream_t)stream));
  *out_table_ms = ms[0];
  *out_scan_ms = ms[1];
  return MI_OK;
}

int mi_ivfpq_info(const mi_ivfpq* h, int64_t* n, int32_t* d, int32_t* m, int32_t* ks, int32_t* nlist, int32_t* device, int64_t* row_offset,
                  int64_t* capacity, int64_t* hbm_bytes) {
  REQUIRE(h, "null handle");
  if (n) *n = h->n;
  if (d) *d = h->d;
  if (m) *m = h->m;
  if (ks) *ks = h->ks;
  if (nlist) *nlist = h->nlist;
  if (device) *device = h->device;
  if (row_offset) *row_offset = h->row_offset;
  if (capacity) *capacity = h->cap;
  if (hbm_bytes) *hbm_bytes = (int64_t)h->bufs.bytes();
  return MI_OK;
}

int mi_ivfpq_list_sizes(const mi_ivfpq* h, int64_t* out) {
  REQUIRE(h, "null handle");
  REQUIRE(out, "null pointer: out");
  for (int32_t l = 0; l < h->nlist; ++l) out[l] = h->list_size[l];
  return MI_OK;
}

int mi_ivfpq_get_rows(mi_ivfpq* h, int64_t row0, int64_t nrows, uint8_t* out_codes_host, uint8_t* out_lists_host) {
  REQUIRE(h, "null handle");
  REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= h->n, "row range outside the index");
  if (nrows == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(h->mu);
  if (out_lists_host) std::memcpy(out_lists_host, h->list_of_row.data() + row0, (size_t)nrows);
  if (!out_codes_host) return MI_OK;
  HIPC(hipSetDevice(h->device));
  HIPC(hipStreamSynchronize(h->stream));
  // only the blocks the rows touch are read back: the rows in ascending order of their slot, every run of consecutive block
  // numbers (at most 65536 blocks) in one copy
  const int64_t blk_words = (int64_t)h->MQ * 64;
  std::vector<std::pair<int64_t, int64_t>> by_slot((size_t)nrows);      // (slot, row)
  for (int64_t r = 0; r < nrows; ++r) by_slot[(size_t)r] = {h->slot_of_row[(size_t)(row0 + r)], r};
  std::sort(by_slot.begin(), by_slot.end());
  std::vector<uint32_t> buf;
  for (size_t t0 = 0; t0 < by_slot.size();) {
    const int64_t b0 = by_slot[t0].first >> 6;
    int64_t b1 = b0 + 1;
    size_t t1 = t0 + 1;
    while (t1 < by_slot.size() && (by_slot[t1].first >> 6) <= b1 && (by_slot[t1].first >> 6) - b0 < 65536) b1 = (by_slot[t1++].first >> 6) + 1;
    buf.resize((size_t)((b1 - b0) * blk_words));
    HIPC(hipMemcpy(buf.data(), h->codes + b0 * blk_words, buf.size() * 4, hipMemcpyDeviceToHost));
    for (size_t t = t0; t < t1; ++t) unpack_code_row(buf.data(), by_slot[t].first - b0 * 64, h->MQ, h->m, out_codes_host + by_slot[t].second * h->m);
    t0 = t1;
  }
  return MI_OK;
}

// Row removal in place (faiss IndexIVFPQ.remove_ids), either kind of index: every chain is compacted where it
// lies by one workgroup (pq_remove.hip), a survivor stays in its list and keeps its code bytes, its row id becomes its new local
// row.  The host then rebuilds its mirror the way the device moved the rows -- ascending row id, one counter per list, which is
// the order of a chain because appends fill a chain in row order and the renumbering is monotone -- hands the blocks the chains
// no longer reach to the free list, and publishes the tables.  Device memory beyond the index: the bitmap and 4 bytes per
// bitmap word, grow-only on the handle, allocated before anything moves.
int mi_ivfpq_remove_rows(mi_ivfpq* h, const uint64_t* remove_bits, int memspace, int64_t* out_removed) {
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
  const int64_t nwords = (n + 63) / 64;
  if ((rc = h->bits.grow((size_t)nwords)) != MI_OK) return rc;
  if ((rc = h->rmpref.grow((size_t)nwords + 1)) != MI_OK) return rc;
  HIPC(hipMemcpyAsync(h->bits, plan.keep.data(), (size_t)nwords * 8, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(h->rmpref, plan.prefix.data(), ((size_t)nwords + 1) * 4, hipMemcpyHostToDevice, s));
  // the tables on the device are those of the last publish: the chains and fills before the removal
  launch_ivf_remove(h->codes, h->rowid, h->blk_table, h->list_off, h->list_rows, h->nlist, h->m, h->bits, h->rmpref, s);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));
  std::vector<int64_t> fill((size_t)h->nlist, 0);
  int64_t j = 0;
  for (int64_t r = 0; r < n; ++r) {
    if (!((plan.keep[(size_t)(r >> 6)] >> (r & 63)) & 1ull)) continue;
    const int32_t l = h->list_of_row[(size_t)r];
    const int64_t c = fill[l]++;
    h->slot_of_row[(size_t)j] = (int64_t)h->blocks[l][(size_t)(c >> 6)] * 64 + (c & 63);
    h->list_of_row[(size_t)j] = (uint8_t)l;
    ++j;
  }
  h->slot_of_row.resize((size_t)m);
  h->list_of_row.resize((size_t)m);
  for (int32_t l = 0; l < h->nlist; ++l) {
    const size_t nb = (size_t)((fill[l] + 63) / 64);
    h->free_blocks.insert(h->free_blocks.end(), h->blocks[l].begin() + nb, h->blocks[l].end());
    h->blocks[l].resize(nb);
  }
  h->list_size = fill;
  h->n = m;
  if ((rc = ivf_publish(h)) != MI_OK) return rc;
  if (out_removed) *out_removed = plan.removed;
  return MI_OK;
}

int mi_ivfpq_destroy(mi_ivfpq* h) {
  if (!h) return MI_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->bufs.reset();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return MI_OK;
}

}  // extern "C"
