// Filtered top-K search (mi_knn_search_filtered): the exact top-K of every query over the rows an allow bitmap admits.
// DESIGN.md 5.10.  Two exact paths, chosen per call from the selectivity s = allowed / n:
//   1 (compact)    the allowed rows are copied into a sub-gallery owned by the handle (f32 rows, 16-bit image, RowStat: the same
//                  bits, no ingest), searched by the unchanged batched search, and its ids mapped back.  The sub-gallery is kept
//                  for the next call with the same bitmap (option "filter_cache").
//   2 (over-fetch) the unfiltered search at depth K' = min(2048, ceil(1.25 k / s) + 32), then the first k allowed entries of
//                  each list.  A query is certified when it found k of them, or when K' covered the whole shard: an allowed row
//                  outside the top-K' ranks after the K'-th entry, hence after every kept one.  The others are answered by path 1.
// Every returned score comes from rescore_kernel over the same stored f32 row, so it is the bits mi_knn_search gives that row.
#include "api_internal.h"

// the sub-gallery's workspaces, freed (never parked in the process's spare slot, as ws_free would)
static void sub_ws_free(mi_gallery* s) {
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  if (s->tail_stream) (void)hipStreamSynchronize(s->tail_stream);
  for (Workspace* w : {&s->ws, &s->ws_alt}) {
    for (void* p : w->allocs) (void)hipFree(p);
    *w = Workspace();
  }
}

// the sub-gallery's own allocations, workspace, tail stream and events; its stream is the parent's and stays
static void sub_free(mi_gallery* s) {
  if (!s) return;
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  if (s->tail_stream) (void)hipStreamSynchronize(s->tail_stream);
  for (int i = 0; i < 2; ++i) {
    if (s->ev_p1[i]) (void)hipEventDestroy(s->ev_p1[i]);
    if (s->ev_tail[i]) (void)hipEventDestroy(s->ev_tail[i]);
  }
  if (s->ev_pre) (void)hipEventDestroy(s->ev_pre);
  if (s->tail_stream) (void)hipStreamDestroy(s->tail_stream);
  sub_ws_free(s);
  for (auto& e : s->ev_pool) {
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  for (void* p : {(void*)s->gal_f32, s->gal_img, (void*)s->rowstat, (void*)s->gstat3, s->samp_img, (void*)s->samp_scores,
                  (void*)s->samp_f32})
    (void)hipFree(p);
  s->scratch.reset();
  s->stream = nullptr;
  delete s;
}

void filter_invalidate(mi_gallery* g) {
  g->filt.valid = false;
  g->filt.last_key_n = -1;
}

void filter_release_sub(mi_gallery* g) {
  auto& f = g->filt;
  sub_free(f.sub);
  f.sub = nullptr;
  f.sub_cap = 0;
  f.valid = false;
}

// the search options of the parent, for the sub-gallery's searches (the answers do not depend on them; the schedule does)
static void copy_search_options(const mi_gallery* g, mi_gallery* s) {
  s->chunk0_tiles = g->chunk0_tiles, s->chunk_growth = g->chunk_growth, s->exact_fallback = g->exact_fallback;
  s->force_exact = g->force_exact, s->speculative = g->speculative, s->rescore_grid_x = g->rescore_grid_x;
  s->spec_max_ratio = g->spec_max_ratio, s->device_repair = g->device_repair, s->small_batch_kernel = g->small_batch_kernel;
  s->xcc_balance = g->xcc_balance, s->ladder = g->ladder, s->boot_ksplit = g->boot_ksplit, s->stream_tail = g->stream_tail;
  s->surv_cap = g->surv_cap, s->rescore_cap = g->rescore_cap;
}

// The sub-gallery of the rows `key` allows (bits_dev: the same bitmap on the device, read only when it is (re)built).
// *hit: the stored one was built from an equal bitmap of a parent of the same n and is reused.
static int sub_prepare(mi_gallery* g, const std::vector<uint64_t>& key, const uint64_t* bits_dev, int64_t allowed, bool* hit) {
  auto& f = g->filt;
  hipStream_t s = g->stream;
  *hit = g->filter_cache && f.valid && f.sub && f.key_n == g->n && f.key == key;
  if (!*hit) {
    f.valid = false;
    if (f.sub && (f.sub->img_f16 != g->img_f16 || f.sub_cap < allowed)) {
      sub_free(f.sub);
      f.sub = nullptr;
      f.sub_cap = 0;
    }
    if (!f.sub) {
      mi_gallery* sg = new mi_gallery();
      sg->device = g->device;
      sg->d = sg->ud = g->d, sg->dp = g->dp, sg->norm_mode = g->norm_mode, sg->img_f16 = g->img_f16;
      sg->stream = s;
      const int64_t cap = std::max<int64_t>(allowed, std::min<int64_t>(g->n, allowed + allowed / 4));   // room to grow into
      const int64_t cap_pad = round_up(cap, TILE);
      f.sub = sg;
      hipError_t e = device_malloc((void**)&sg->gal_f32, (size_t)cap * g->dp * 4 + 256);
      if (e == hipSuccess) e = device_malloc(&sg->gal_img, (size_t)cap_pad * g->dp * 2 + 256);
      if (e == hipSuccess) e = device_malloc((void**)&sg->rowstat, (size_t)cap_pad * sizeof(RowStat));
      if (e == hipSuccess) e = device_malloc((void**)&sg->gstat3, 16);
      if (e != hipSuccess) {
        sub_free(sg);
        f.sub = nullptr;
        return fail(e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP,
                    std::string("sub-gallery of the filtered search: ") + hipGetErrorString(e));
      }
      sg->cap = cap;
      f.sub_cap = cap;
    }
    mi_gallery* sg = f.sub;
    const int64_t nblk = filter_blocks(g->n);
    int rc;
    if ((rc = f.rows.grow((size_t)allowed)) != MI_OK) return rc;
    if ((rc = grow_all((size_t)nblk + 1, f.bcnt, f.boff)) != MI_OK) return rc;
    const int64_t mpad = round_up(allowed, TILE);
    launch_filter_compact(bits_dev, g->n, f.bcnt, f.boff, f.rows, s);
    launch_subset_gather(g->gal_f32, g->gal_img, g->rowstat, f.rows, allowed, mpad, g->dp, sg->gal_f32, sg->gal_img, sg->rowstat,
                         s);
    HIPC(hipGetLastError());
    sg->n = allowed;
    sg->npad = mpad;
    sg->samp_for_n = -1;          // the threshold samples are drawn again from the new rows
    sg->samp_f32_for_n = -1;
    f.key = key;
    f.key_n = g->n;
    f.valid = true;
  }
  mi_gallery* sg = f.sub;
  // every call: the parent's norm maxima (a maximum over a superset: the certificate holds, a little looser; and
  // mi_gallery_norm_bounds may have raised them since) and its options
  HIPC(hipMemcpyAsync(sg->gstat3, g->gstat3, 12, hipMemcpyDeviceToDevice, s));
  copy_search_options(g, sg);
  // the workspace is sized for the largest k once, so that only new caps rebuild it; ws_ensure would park the old one in the
  // process's spare slot, so a workspace of other caps is freed here first
  if (!sg->ws.allocs.empty() && (sg->ws.cap != sg->surv_cap || sg->ws.rcap != sg->rescore_cap)) sub_ws_free(sg);
  return ws_ensure(sg, 2048);
}

// Path 1 for nq queries staged on the device (q_dev, strides rs / cs): host results [nq][k] in out_idx / out_score (may be NULL)
static int compact_search(mi_gallery* g, const void* q_dev, int dtype, int64_t rs, int64_t cs, int64_t nq, int32_t k,
                          const std::vector<uint64_t>& key, const uint64_t* bits_dev, int64_t allowed, int64_t* out_idx,
                          float* out_score, bool* hit) {
  auto& f = g->filt;
  hipStream_t s = g->stream;
  int rc = sub_prepare(g, key, bits_dev, allowed, hit);
  if (rc != MI_OK) return rc;
  mi_gallery* sg = f.sub;
  const int32_t ke = (int32_t)std::min<int64_t>(k, allowed);
  if ((rc = grow_all((size_t)nq * ke, f.sidx, f.ssc)) != MI_OK) return rc;
  if ((rc = grow_all((size_t)nq * k, f.idx, f.sc)) != MI_OK) return rc;
  if ((rc = search_sync(sg, q_dev, dtype, rs, cs, sg->norm_mode, nq, ke, f.sidx, f.ssc, nullptr)) != MI_OK) return rc;
  launch_filter_remap(f.sidx, f.ssc, nq, ke, k, f.rows, allowed, g->row_offset, f.idx, f.sc, s);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(out_idx, f.idx, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
  if (out_score) HIPC(hipMemcpyAsync(out_score, f.sc, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  return MI_OK;
}

extern "C" {

int mi_knn_search_filtered(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride,
                           int32_t k, const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_score,
                           mi_filter_info* out_info, double* out_seconds) {
  return filtered_search_host(g, q, nq, dtype, row_stride, col_stride, k, allow_bits, allow_memspace, out_idx, out_score, out_info,
                              out_seconds, /*l2_caller=*/false);
}

}  // extern "C"

int filtered_search_host(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                         const uint64_t* allow_bits, int allow_memspace, int64_t* out_idx, float* out_score,
                         mi_filter_info* out_info, double* out_seconds, bool l2_caller) {
  REQUIRE(g, "null handle");
  REQUIRE(allow_bits, "null pointer: allow_bits");
  REQUIRE(allow_memspace == MI_HOST || allow_memspace == MI_DEVICE, "allow_memspace must be MI_HOST or MI_DEVICE");
  REQUIRE(k >= 1 && k <= 2048, "k must be in [1, 2048]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  if (!l2_caller) REFUSE_L2(g, "mi_knn_search_filtered");
  mi_filter_info info;
  std::memset(&info, 0, sizeof info);
  if (out_info) *out_info = info;
  std::unique_lock<std::mutex> lock(g->mu, std::defer_lock);
  if (!l2_caller) lock.lock();                 // (mi_knn_search_l2 holds it across the selection and its distance tail)
  HIPC(hipSetDevice(g->device));
  const auto t0 = std::chrono::steady_clock::now();
  if (nq == 0) {
    if (out_seconds) *out_seconds = 0.0;
    return MI_OK;
  }
  REQUIRE(g->n >= 1, "empty gallery");
  int64_t elems;
  int rc = strided_extent(nq, g->d, row_stride, col_stride, &elems);
  if (rc != MI_OK) return rc;
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  hipStream_t s = g->stream;
  // the workspace and the staging are the search's: a deferred tail of an earlier batch still reads them
  if ((rc = join_tails(g, s)) != MI_OK) return rc;
  HIPC(hipStreamSynchronize(s));
  if ((rc = ws_ensure(g, std::max<int32_t>(1, g->ws.kcap))) != MI_OK) return rc;     // the flags word lives there
  // the sticky flags belong to the searches around this call: kept aside, put back at the end (as mi_range_search does)
  uint32_t kept_flags = 0;
  if ((rc = read_and_clear_flags(g, &kept_flags)) != MI_OK) return rc;
  auto& f = g->filt;
  auto done = [&](int code) {
    if (kept_flags) {
      uint32_t now = 0;
      if (hipMemcpy(&now, g->ws.flags, 4, hipMemcpyDeviceToHost) == hipSuccess) {
        now |= kept_flags;
        (void)hipMemcpy(g->ws.flags, &now, 4, hipMemcpyHostToDevice);
      }
    }
    if (!g->filter_cache && f.sub) filter_release_sub(g);   // option "filter_cache" 0: the sub-gallery does not outlive the call
    if (out_info) *out_info = info;
    if (code == MI_OK && out_seconds)
      *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return code;
  };

  // the bitmap on the host, bits at or beyond n cleared: the count that picks the path, and the key of the cached sub-gallery
  const int64_t nwords = (g->n + 63) / 64;
  std::vector<uint64_t> key((size_t)nwords);
  if (allow_memspace == MI_HOST) std::memcpy(key.data(), allow_bits, (size_t)nwords * 8);
  else if (hipMemcpy(key.data(), allow_bits, (size_t)nwords * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return done(fail(MI_ERR_HIP, "D2H copy of the allow bitmap failed"));
  if (g->n % 64) key.back() &= (1ull << (g->n % 64)) - 1ull;
  int64_t allowed = 0;
  for (uint64_t w : key) allowed += __builtin_popcountll(w);
  info.allowed = allowed;
  const double sel = (double)allowed / (double)g->n;
  // auto: compact when the bitmap is the one the stored sub-gallery was cut for, or the one of the previous call
  // (a bitmap seen twice is likely to come again: this call builds the sub-gallery, the next ones reuse it -- a cached compact
  // call beat the over-fetch at every measured selectivity below 1), at s <= filter_compact_max (the crossover of first
  // calls), and whenever fewer than k rows are allowed (the over-fetch cannot certify them).  With every row allowed a
  // compaction would copy the whole shard for nothing: the over-fetch certifies every query at K' = 1.25 k + 32.
  const bool cached = g->filter_cache && f.valid && f.sub && f.key_n == g->n && f.key == key;
  const bool repeat = g->filter_cache && allowed < g->n && f.last_key_n == g->n && f.last_key == key;
  f.last_key = key;
  f.last_key_n = g->n;
  int path = 0;
  if (allowed == 0) path = 0;
  else if (g->filter_path == 1 || g->filter_path == 2) path = g->filter_path;
  else path = (cached || repeat || sel <= g->filter_compact_max || allowed < k) ? 1 : 2;
  info.path = path;
  if (path == 0) {
    for (int64_t i = 0; i < nq * k; ++i) {
      out_idx[i] = -1;
      if (out_score) out_score[i] = -INFINITY;
    }
    return done(MI_OK);
  }

  // queries: the host staging of mi_knn_search (grow-only slot 0)
  void* qd = io_stage(g->io_q, (size_t)elems * esz);
  if (!qd) return done(fail(MI_ERR_NOMEM, "staging buffer of mi_knn_search_filtered"));
  if (hipMemcpy(qd, q, (size_t)elems * esz, hipMemcpyHostToDevice) != hipSuccess)
    return done(fail(MI_ERR_HIP, "H2D query copy failed"));
  // the bitmap on the device: the caller's, or the host one uploaded when a kernel is going to read it
  const uint64_t* bits_dev = allow_memspace == MI_DEVICE ? allow_bits : nullptr;
  auto upload_bits = [&]() -> int {
    if (bits_dev) return MI_OK;
    int r = f.bits.grow((size_t)nwords);
    if (r != MI_OK) return r;
    HIPC(hipMemcpy(f.bits, key.data(), (size_t)nwords * 8, hipMemcpyHostToDevice));
    bits_dev = f.bits;
    return MI_OK;
  };
  bool hit = false;

  if (path == 1) {
    if (!cached && (rc = upload_bits()) != MI_OK) return done(rc);
    rc = compact_search(g, qd, dtype, row_stride, col_stride, nq, k, key, bits_dev, allowed, out_idx, out_score, &hit);
    info.cache_hit = hit ? 1 : 0;
    return done(rc);
  }

  // path 2: over-fetch at depth K', keep the first k allowed entries, certify
  const int64_t want = (int64_t)std::ceil(1.25 * (double)k / sel) + 32;
  const int32_t kp = (int32_t)std::min<int64_t>({want, 2048, (int64_t)g->rescore_cap, (int64_t)(g->surv_cap / 4), g->n});
  const int32_t covers = kp >= g->n ? 1 : 0;
  info.kprime = kp;
  if ((rc = upload_bits()) != MI_OK) return done(rc);
  int64_t* tidx = (int64_t*)io_stage(g->io_idx, (size_t)nq * kp * 8);
  float* tsc = (float*)io_stage(g->io_sc, (size_t)nq * kp * 4);
  if (!tidx || !tsc) return done(fail(MI_ERR_NOMEM, "staging buffers of mi_knn_search_filtered"));
  if ((rc = grow_all((size_t)nq * k, f.idx, f.sc)) != MI_OK) return done(rc);
  if ((rc = f.ok.grow((size_t)nq)) != MI_OK) return done(rc);
  if ((rc = search_sync(g, qd, dtype, row_stride, col_stride, g->norm_mode, nq, kp, tidx, tsc, nullptr)) != MI_OK)
    return done(rc);
  launch_filter_overfetch(tidx, tsc, nq, kp, k, bits_dev, g->n, g->row_offset, covers, f.idx, f.sc, f.ok, s);
  if (hipGetLastError() != hipSuccess) return done(fail(MI_ERR_HIP, "filter_overfetch_kernel launch failed"));
  std::vector<uint32_t> ok((size_t)nq);
  if (hipMemcpyAsync(out_idx, f.idx, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
      (out_score && hipMemcpyAsync(out_score, f.sc, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
      hipMemcpyAsync(ok.data(), f.ok, (size_t)nq * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return done(fail(MI_ERR_HIP, "D2H copy of the over-fetch results failed"));
  std::vector<int64_t> rerun;
  for (int64_t i = 0; i < nq; ++i)
    if (!ok[(size_t)i]) rerun.push_back(i);
  info.rerun_queries = (int64_t)rerun.size();
  if (rerun.empty()) return done(MI_OK);
  // the queries it could not certify, packed [m][d] on the host, answered by path 1
  const int64_t m = (int64_t)rerun.size();
  const int32_t d = g->d;
  std::vector<char> packed((size_t)m * d * esz);
  for (int64_t r = 0; r < m; ++r) {
    const char* src = (const char*)q + (size_t)rerun[(size_t)r] * row_stride * esz;
    char* dst = packed.data() + (size_t)r * d * esz;
    if (col_stride == 1) std::memcpy(dst, src, (size_t)d * esz);
    else
      for (int32_t c = 0; c < d; ++c) std::memcpy(dst + (size_t)c * esz, src + (size_t)c * col_stride * esz, esz);
  }
  if ((rc = f.qbuf.grow(packed.size())) != MI_OK) return done(rc);
  if (hipMemcpy(f.qbuf, packed.data(), packed.size(), hipMemcpyHostToDevice) != hipSuccess)
    return done(fail(MI_ERR_HIP, "H2D copy of the re-run queries failed"));
  std::vector<int64_t> ridx((size_t)m * k);
  std::vector<float> rsc((size_t)m * k);
  rc = compact_search(g, f.qbuf, dtype, d, 1, m, k, key, bits_dev, allowed, ridx.data(), rsc.data(), &hit);
  info.cache_hit = hit ? 1 : 0;
  if (rc != MI_OK) return done(rc);
  for (int64_t r = 0; r < m; ++r) {
    const size_t o = (size_t)rerun[(size_t)r] * k;
    std::memcpy(out_idx + o, ridx.data() + (size_t)r * k, (size_t)k * 8);
    if (out_score) std::memcpy(out_score + o, rsc.data() + (size_t)r * k, (size_t)k * 4);
  }
  return done(MI_OK);
}
