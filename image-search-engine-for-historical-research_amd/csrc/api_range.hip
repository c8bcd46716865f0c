// Exact range search (mi_range_search): every row whose exact score is >= min_score, per query, in CSR form.  DESIGN.md 5.9.
// The certificate of the top-K path bounds |approx - exact| <= eps_q for every (query, row), so a filtered scoring
// launch at the FIXED threshold min_score - eps_q keeps every row of the answer; the survivors are re-scored in f64 by
// rescore_kernel (the arithmetic of mi_knn_search, bit for bit) and the rows at >= min_score are kept.  No sample, no ladder, no
// verification.  The gallery goes out in chunks of tiles: a chunk whose buffers overflow is done again in halves, and a
// single tile that still overflows is answered densely (every row of it re-scored).  Then the hits of every query are ordered
// by (score desc, row asc) on the device and copied out once per batch.
#include "api_internal.h"

// the buffers the exact re-score fills, exactly [QB][the workspace's survivor rows]: sized again when that number changes
static int range_scratch_ensure(mi_gallery* g) {
  auto& r = g->range;
  const size_t lists = (size_t)QB * g->ws.cap;
  if (r.rows.count() != lists) r.rows.reset(), r.rcnt.reset(), r.sc.reset();
  int rc;
  if ((rc = r.rows.grow_exact(lists)) != MI_OK || (rc = r.rcnt.grow_exact(QB)) != MI_OK || (rc = r.sc.grow_exact(lists)) != MI_OK)
    return rc;
  if ((rc = r.lims.grow_exact(QB + 1)) != MI_OK) return rc;
  return r.total.grow_exact(1);
}

// one batch (nb <= QB queries): scoring chunks, re-score, kept hits; then lims (host, batch-relative) and the
// ordered hits in *idx_out / *sc_out (device) when they fit `room` entries.  *need_exact: a query's 16-bit image overflowed (FLAG_RANGE), answer the batch with the f32
// scorer instead.  *overflowed: some chunk overflowed its buffers (split or answered densely).
static int range_batch(mi_gallery* g, const void* src, int dtype, int64_t rs, int64_t cs, int32_t nb, double min_score,
                       bool exact, int64_t room, std::vector<int64_t>& lims_h, int64_t** idx_out, float** sc_out,
                       bool* need_exact, bool* overflowed) {
  hipStream_t s = g->stream;
  Workspace& ws = g->ws;
  auto& r = g->range;
  const QueryState st = make_state(ws);
  const int32_t qpad = (int32_t)round_up(nb, TILE);
  const float gamma = 2.0f * (float)g->dp * 5.9604645e-08f;    // the search's (plan_phase1)
  const int use_img = exact ? 0 : 1;
  *need_exact = false;
  if (!launch_ingest_queries(src, dtype, nb, g->d, rs, cs, g->norm_mode, ws.q_f32, ws.q_img, g->img_f16, ws.q_stat, g->dp, qpad,
                             g->gstat3, gamma, use_img, 0u, st, s)) {
    launch_ingest(src, dtype, nb, g->d, rs, cs, g->norm_mode, ws.q_f32, ws.q_img, g->img_f16, ws.q_stat, g->dp, qpad, s);
    launch_init_query_state(ws.q_stat, g->gstat3, nb, qpad, gamma, use_img, 0u, st, s);
  }
  launch_range_threshold(st, nb, qpad, min_score, s);
  HIPC(hipGetLastError());

  const int64_t ntiles = g->npad / TILE;
  const uint32_t last_row = (uint32_t)std::max<int64_t>(0, g->n - 1);
  const int64_t dense_tiles = std::max<int64_t>(1, ws.cap / TILE);
  int64_t t = 0, len = ntiles, base = 0, nchunks = 0;
  bool dense = false;
  while (t < ntiles) {
    const int64_t cur = std::min<int64_t>(dense ? std::min(len, dense_tiles) : len, ntiles - t);
    const int64_t row0 = t * TILE, row1 = std::min<int64_t>(g->n, (t + cur) * TILE);
    int rc;
    // room for every row this chunk can keep, and for its counts / offsets
    const size_t hits_room = (size_t)base + (size_t)nb * ws.cap;
    if ((rc = r.akey.grow_keep(hits_room, (size_t)base)) != MI_OK || (rc = r.arow.grow_keep(hits_room, (size_t)base)) != MI_OK) return rc;
    if ((rc = r.coff.grow_keep((size_t)(nchunks + 1) * QB, (size_t)nchunks * QB)) != MI_OK) return rc;
    if ((rc = r.ccnt.grow_keep((size_t)(nchunks + 1) * QB, (size_t)nchunks * QB)) != MI_OK) return rc;
    launch_range_chunk_begin(st, qpad, r.total, s);
    if (dense) {
      launch_range_rows(st, nb, r.rows, r.rcnt, 1, (uint32_t)row0, (uint32_t)(row1 - row0), s);
    } else {
      if (exact) {
        ExactArgs a;
        a.gal_f32 = g->gal_f32;
        a.qry_f32 = ws.q_f32;
        a.dp = g->dp;
        a.row0 = row0;
        a.row1 = row1;
        a.n = g->n;
        a.nq = nb;
        a.st = st;
        launch_exact_select(a, false, s);
      } else {
        ScoreArgs a;
        a.gal_img = g->gal_img;
        a.qry_img = ws.q_img;
        a.img_f16 = g->img_f16;
        a.nslices = g->dp / SLICE_K;
        a.tile0 = (int32_t)t;
        a.ntiles = (int32_t)cur;
        a.nqt = qpad / TILE;
        a.n = g->n;
        a.nq = nb;
        a.small_batch_kernel = g->small_batch_kernel;
        a.rec = ws.rec;
        a.rec_cnt = ws.rec_cnt;
        a.rec_cap = ws.rec_cap;
        a.cond = nullptr;
        a.bal = g->xcc_balance ? ws.bal : nullptr;   // the measured split is read, not re-measured
        a.lad_k = 0;                                 // no ladder: the threshold is fixed
        a.dbg = ws.dbg;
        a.st = st;
        launch_gemm_select(a, false, s);
        launch_scatter_records(ws.rec, ws.rec_cnt, ws.rec_cap, ws.nseg, st, nullptr, s, nullptr, nullptr, 0u, nb);
      }
      launch_range_rows(st, nb, r.rows, r.rcnt, 0, 0u, 0u, s);
    }
    launch_rescore(g->gal_f32, ws.q_f32, g->dp, nb, r.rows, r.rcnt, ws.cap, r.sc, s, (uint32_t)g->rescore_grid_x, last_row);
    launch_range_keep(r.rows, r.rcnt, r.sc, ws.cap, nb, min_score, r.total, r.coff + (size_t)nchunks * QB,
                      r.ccnt + (size_t)nchunks * QB, r.akey, r.arow, (uint64_t)base, (uint64_t)r.akey.count(), ws.flags, s);
    HIPC(hipGetLastError());
    uint32_t flags = 0;
    unsigned long long hits = 0;
    HIPC(hipMemcpyAsync(&hits, r.total, sizeof hits, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(&flags, ws.flags, 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (flags) HIPC(hipMemset(ws.flags, 0, 4));
    if (flags & FLAG_RANGE) {
      if (exact) return fail(MI_ERR_HIP, "range search: FLAG_RANGE raised by the f32 scorer");
      *need_exact = true;
      return MI_OK;
    }
    if (flags & (FLAG_SURV_OVERFLOW | FLAG_REC_OVERFLOW | FLAG_CAND_OVERFLOW)) {
      // this chunk's work is dropped (base and the chunk count stay): again in halves, a single tile densely
      if (dense) return fail(MI_ERR_HIP, "range search: the dense path of a chunk overflowed its buffers");
      *overflowed = true;
      if (cur > 1) len = (cur + 1) / 2;
      else dense = true;
      continue;
    }
    base += (int64_t)hits;
    ++nchunks;
    t += cur;
    if (dense) {                 // back to the filtered launches, one tile first
      dense = false;
      len = 1;
    } else {
      len = std::min<int64_t>(2 * cur, ntiles);
    }
  }

  launch_range_lims(r.ccnt, (int32_t)nchunks, QB, nb, r.lims, s);
  lims_h.assign((size_t)nb + 1, 0);
  HIPC(hipMemcpyAsync(lims_h.data(), r.lims, ((size_t)nb + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  const int64_t total = lims_h[nb];
  if (total == 0 || total > room) return MI_OK;       // nothing to order, or it would not fit the caller's arrays
  int64_t max_cnt = 0;
  for (int32_t q = 0; q < nb; ++q) max_cnt = std::max(max_cnt, lims_h[q + 1] - lims_h[q]);
  int rc;
  if ((rc = grow_all((size_t)total, r.bkey[0], r.brow[0], r.bkey[1], r.brow[1])) != MI_OK) return rc;
  launch_range_gather(r.akey, r.arow, r.coff, r.ccnt, (int32_t)nchunks, QB, nb, r.lims, r.bkey[0], r.brow[0], s);
  // lims[0] is 0 and the total fits `room` (checked above), so the stage's capacity guard never fires here
  CsrList c;
  c.nq = nb;
  c.lims = r.lims;
  c.total = r.lims + nb;
  c.max_results = room;
  for (int i = 0; i < 2; ++i) c.key[i] = r.bkey[i], c.row[i] = r.brow[i];
  const int cur = launch_csr_order(c, max_cnt, total, s);
  // the write-out's staging: the other ping-pong buffer holds total * 12 bytes, enough for the int64 ids (8) + f32 scores (4)
  int64_t* idx_d = reinterpret_cast<int64_t*>(r.bkey[cur ^ 1].get());
  float* sc_d = reinterpret_cast<float*>(r.brow[cur ^ 1].get());
  launch_csr_write(c, cur, true, total, g->row_offset, idx_d, sc_d, nullptr, s);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));      // the handle's stream does not block: the caller's hipMemcpy would not wait for it
  *idx_out = idx_d;
  *sc_out = sc_d;
  return MI_OK;
}

extern "C" {

int mi_range_search(mi_gallery* g, const void* q, int64_t nq, int dtype, int64_t row_stride, int64_t col_stride,
                    double min_score, int64_t max_results, int64_t* out_lims, int64_t* out_idx, float* out_score,
                    double* out_seconds) {
  REQUIRE(g, "null handle");
  REQUIRE(out_lims, "null pointer: out_lims");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  REQUIRE(min_score == min_score, "min_score is NaN");
  REQUIRE(max_results >= 0, "max_results must be >= 0");
  REQUIRE(max_results == 0 || out_idx, "null pointer: out_idx");
  REFUSE_L2(g, "mi_range_search (radius search)");
  std::lock_guard<std::mutex> lock(g->mu);
  HIPC(hipSetDevice(g->device));
  const auto t0 = std::chrono::steady_clock::now();
  out_lims[0] = 0;
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
  // the workspace is the search's: a deferred tail of an earlier mi_knn_search_device batch still reads it
  if ((rc = join_tails(g, s)) != MI_OK) return rc;
  HIPC(hipStreamSynchronize(s));
  if ((rc = ws_ensure(g, std::max<int32_t>(1, g->ws.kcap))) != MI_OK) return rc;
  if ((rc = range_scratch_ensure(g)) != MI_OK) return rc;
  // the sticky flags belong to the searches around this call: kept aside, the range search's own are read and cleared per
  // chunk, and the kept ones are put back at the end
  uint32_t kept_flags = 0;
  if ((rc = read_and_clear_flags(g, &kept_flags)) != MI_OK) return rc;
  auto done = [&](int code) {
    if (kept_flags) {
      uint32_t now = 0;
      if (hipMemcpy(&now, g->ws.flags, 4, hipMemcpyDeviceToHost) == hipSuccess) {
        now |= kept_flags;
        (void)hipMemcpy(g->ws.flags, &now, 4, hipMemcpyHostToDevice);
      }
    }
    return code;
  };
  // queries: the host staging of mi_knn_search (grow-only slot 0)
  const size_t qbytes = (size_t)elems * esz;
  if (!io_stage(g->io_q, qbytes)) return done(fail(MI_ERR_NOMEM, "staging buffer of mi_range_search"));
  if (hipMemcpy(g->io_q, q, qbytes, hipMemcpyHostToDevice) != hipSuccess)
    return done(fail(MI_ERR_HIP, "H2D query copy failed"));
  // more than one batch: the hits are held on the host until the total is known (nothing reaches out_idx / out_score unless
  // all of them fit); one batch: straight into the caller's arrays
  const bool single = nq <= QB;
  std::vector<int64_t> hold_idx;
  std::vector<float> hold_sc;
  std::vector<int64_t> lims_b;
  int64_t cum = 0;
  for (int64_t q0 = 0; q0 < nq; q0 += QB) {
    const int32_t b = (int32_t)std::min<int64_t>(QB, nq - q0);
    const char* src = g->io_q.get() + (size_t)q0 * row_stride * esz;
    bool exact = g->force_exact != 0, overflowed = false;
    const int64_t room = std::max<int64_t>(0, max_results - cum);   // past the capacity, later batches are only counted
    int64_t* idx_d = nullptr;
    float* sc_d = nullptr;
    for (;;) {
      bool need_exact = false;
      rc = range_batch(g, src, dtype, row_stride, col_stride, b, min_score, exact, room, lims_b, &idx_d, &sc_d, &need_exact,
                       &overflowed);
      if (rc != MI_OK) return done(rc);
      if (!need_exact) break;
      exact = true;                          // FLAG_RANGE: the f32 scorer answers the batch, as in the search
    }
    if (overflowed) g->stats.overflow_batches += 1;
    const int64_t total = lims_b[b];
    for (int32_t i = 1; i <= b; ++i) out_lims[q0 + i] = cum + lims_b[i];
    if (total > 0 && total <= room) {
      if (single) {
        if (hipMemcpy(out_idx, idx_d, (size_t)total * 8, hipMemcpyDeviceToHost) != hipSuccess)
          return done(fail(MI_ERR_HIP, "D2H idx copy failed"));
        if (out_score && hipMemcpy(out_score, sc_d, (size_t)total * 4, hipMemcpyDeviceToHost) != hipSuccess)
          return done(fail(MI_ERR_HIP, "D2H score copy failed"));
      } else {
        hold_idx.resize((size_t)(cum + total));
        hold_sc.resize((size_t)(cum + total));
        if (hipMemcpy(hold_idx.data() + cum, idx_d, (size_t)total * 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hold_sc.data() + cum, sc_d, (size_t)total * 4, hipMemcpyDeviceToHost) != hipSuccess)
          return done(fail(MI_ERR_HIP, "D2H result copy failed"));
      }
    }
    cum += total;
  }
  if (out_seconds) *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (cum > max_results)
    return done(fail(MI_ERR_CAPACITY, "range search: " + std::to_string(cum) + " results > max_results " +
                                          std::to_string(max_results) + "; call again with max_results >= out_lims[nq]"));
  if (!single && cum > 0) {
    std::memcpy(out_idx, hold_idx.data(), (size_t)cum * 8);
    if (out_score) std::memcpy(out_score, hold_sc.data(), (size_t)cum * 4);
  }
  return done(MI_OK);
}

}  // extern "C"
