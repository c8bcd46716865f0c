// Grouped top-K search (mi_knn_search_grouped) and the group labels of a gallery (mi_gallery_set_groups): the best row of every
// group, k groups per query, one excluded group per query.  DESIGN.md 5.10b.  Two exact paths, as in api_filter.hip:
//   2 (over-fetch)  the unfiltered search at depth K' = min(2048, n, f k + 32), collapsed by group_collapse_kernel.  A query is
//                   certified when it kept k rows, or when K' covered the shard: a row beyond rank K' ranks after every kept row, so
//                   it can neither displace a kept group's row nor come before one.  The others are answered by path 1.
//   1 (fallback)    sub-batches of queries whose dense float64 scores [queries][n] and group tables fit "group_dense_bytes": the
//                   dense scorer of the exhaustive search's last resort, every group reduced to (best value, lowest row among
//                   equals) over the group CSR (group_best_kernel), the G entries of a query ordered by csr_order.hip, the first k
//                   taken.  The k rows taken are then re-scored by rescore_kernel, so the float32 written is the one mi_knn_search
//                   gives that row whichever of its own stages answered.
#include "api_internal.h"

void groups_drop(mi_gallery* g) { g->groups.valid = false; }

static int groups_in_step(const mi_gallery* g) {
  REQUIRE(g->groups.valid && (int64_t)g->groups.labels.size() == g->n,
          "the gallery has no group labels in step with its rows (none were set, or the gallery has been appended to or had rows "
          "removed since): call mi_gallery_set_groups");
  return MI_OK;
}

template <typename T>
static int upload(DeviceBuf<T>& b, const std::vector<T>& v) {
  int rc = b.grow(std::max<size_t>(1, v.size()));
  if (rc != MI_OK) return rc;
  if (!v.empty()) HIPC(hipMemcpy(b, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return MI_OK;
}

// queries per sub-batch of the fallback: scores, two group tables (the merge passes alternate) and the rows taken
static int64_t fallback_queries(int64_t bytes, int64_t n, int64_t G, int32_t k) {
  const int64_t per = n * 8 + G * 24 + (int64_t)k * 16;
  return std::max<int64_t>(1, std::min<int64_t>(QB, bytes / per));
}

// Path 1 for nq queries staged on the device (q_dev, strides rs / cs) with their excluded groups excl_dev [nq]: the answer
// [nq][k] into the handle's idx / sc / lab buffers, on the handle's stream
static int group_fallback(mi_gallery* g, const void* q_dev, int dtype, int64_t rs, int64_t cs, int64_t nq, int32_t k,
                          const uint32_t* excl_dev) {
  auto& gs = g->groups;
  hipStream_t s = g->stream;
  Workspace& ws = g->ws;
  const int64_t n = g->n, G = gs.plan.groups();
  const int64_t qb = std::min(nq, fallback_queries(g_group_dense_bytes.load(), n, G, k));
  int rc;
  if ((rc = gs.dense.grow((size_t)qb * n)) != MI_OK) return rc;
  for (int i = 0; i < 2; ++i) {
    if ((rc = gs.key[i].grow((size_t)qb * G)) != MI_OK) return rc;
    if ((rc = gs.row[i].grow((size_t)qb * G)) != MI_OK) return rc;
  }
  if ((rc = gs.lims.grow((size_t)qb + 2)) != MI_OK) return rc;
  if ((rc = grow_all((size_t)qb * k, gs.cand_rows, gs.cand_score)) != MI_OK) return rc;
  if ((rc = gs.cand_cnt.grow((size_t)qb)) != MI_OK) return rc;
  const size_t esz = dtype == MI_F32 ? 4 : 8;
  for (int64_t q0 = 0; q0 < nq; q0 += qb) {
    const int32_t b = (int32_t)std::min<int64_t>(qb, nq - q0);
    const int32_t qpad = (int32_t)round_up(b, TILE);
    launch_ingest((const char*)q_dev + (size_t)q0 * rs * esz, dtype, b, g->d, rs, cs, g->norm_mode, ws.q_f32, ws.q_img, g->img_f16,
                  ws.q_stat, g->dp, qpad, s);
    launch_dense_score64(g->gal_f32, ws.q_f32, g->dp, n, b, gs.dense, n, s);
    launch_group_best(gs.dense, n, b, gs.grp, gs.group_rows, gs.group_off, gs.chunk_g0, gs.plan.chunks(), G, excl_dev + q0, gs.key[0],
                      gs.row[0], s);
    CsrList list;
    list.nq = b;
    list.lims = gs.lims;
    list.total = gs.lims + (qb + 1);
    list.max_results = INT64_MAX;
    for (int i = 0; i < 2; ++i) list.key[i] = gs.key[i], list.row[i] = gs.row[i];
    launch_group_lims(gs.lims, gs.lims + (qb + 1), b, G, s);
    const int cur = launch_csr_order(list, G, (int64_t)b * G, s);
    launch_group_take(gs.row[cur], G, b, k, gs.cand_rows, gs.cand_cnt, s);
    launch_rescore(g->gal_f32, ws.q_f32, g->dp, b, gs.cand_rows, gs.cand_cnt, (uint32_t)k, gs.cand_score, s,
                   (uint32_t)g->rescore_grid_x, (uint32_t)(n - 1));
    launch_group_emit(gs.cand_rows, gs.cand_cnt, gs.cand_score, gs.grp, gs.label_of_group, b, k, g->row_offset,
                      gs.idx + (size_t)q0 * k, gs.sc + (size_t)q0 * k, gs.lab + (size_t)q0 * k, s);
    HIPC(hipGetLastError());
  }
  return MI_OK;
}

extern "C" {

int mi_gallery_set_groups(mi_gallery* g, const int32_t* labels, int64_t n, int memspace) {
  REQUIRE(g, "null handle");
  REFUSE_L2(g, "mi_gallery_set_groups");
  std::lock_guard<std::mutex> lock(g->mu);
  auto& gs = g->groups;
  if (!labels) {
    gs.valid = false;
    gs.labels.clear();
    gs.plan = GroupPlan();
    return MI_OK;
  }
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  REQUIRE(n == g->n, "mi_gallery_set_groups takes one label per row: n must be the gallery's n");
  REQUIRE(n >= 1 && n < (int64_t)GROUP_NONE, "mi_gallery_set_groups: the gallery must hold between 1 and 2^32 - 2 rows");
  HIPC(hipSetDevice(g->device));
  std::vector<int32_t> host((size_t)n);
  if (memspace == MI_HOST) std::memcpy(host.data(), labels, (size_t)n * 4);
  else HIPC(hipMemcpy(host.data(), labels, (size_t)n * 4, hipMemcpyDeviceToHost));
  GroupPlan plan;
  REQUIRE(group_plan_build(host.data(), n, GROUP_CHUNK_ROWS, &plan), "group labels must be >= 0, or -1 for a row that is a group of its own");
  HIPC(hipStreamSynchronize(g->stream));        // no search of this handle reads the old tables any more
  gs.valid = false;
  int rc;
  if ((rc = upload(gs.grp, plan.grp)) != MI_OK) return rc;
  if ((rc = upload(gs.group_off, plan.group_off)) != MI_OK) return rc;
  if ((rc = upload(gs.group_rows, plan.group_rows)) != MI_OK) return rc;
  if ((rc = upload(gs.chunk_g0, plan.chunk_g0)) != MI_OK) return rc;
  if ((rc = upload(gs.label_of_group, plan.label_of_group)) != MI_OK) return rc;
  // the device copies of these two are all the kernels need; the host keeps what the entry points read
  plan.grp = std::vector<uint32_t>();
  plan.group_rows = std::vector<uint32_t>();
  gs.plan = std::move(plan);
  gs.labels = std::move(host);
  gs.valid = true;
  return MI_OK;
}

int mi_gallery_get_groups(mi_gallery* g, int32_t* out_host) {
  REQUIRE(g && out_host, "null pointer");
  std::lock_guard<std::mutex> lock(g->mu);
  int rc = groups_in_step(g);
  if (rc != MI_OK) return rc;
  std::memcpy(out_host, g->groups.labels.data(), g->groups.labels.size() * 4);
  return MI_OK;
}

int mi_gallery_group_count(mi_gallery* g, int64_t* out) {
  REQUIRE(g && out, "null pointer");
  std::lock_guard<std::mutex> lock(g->mu);
  int rc = groups_in_step(g);
  if (rc != MI_OK) return rc;
  *out = g->groups.plan.groups();
  return MI_OK;
}

int mi_knn_search_grouped(mi_gallery* g, const void* q, int64_t nq, int q_dtype, int64_t row_stride, int64_t col_stride, int32_t k,
                          const int32_t* exclude_labels, int64_t* out_idx, float* out_score, int32_t* out_label,
                          mi_group_info* out_info, double* out_seconds) {
  REQUIRE(g, "null handle");
  REQUIRE(k >= 1 && k <= 2048, "k must be in [1, 2048]");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(nq == 0 || q, "null pointer: queries");
  REQUIRE(nq == 0 || out_idx, "null pointer: out_idx");
  REQUIRE(q_dtype == MI_F32 || q_dtype == MI_F64, "q_dtype must be MI_F32 or MI_F64");
  REFUSE_L2(g, "mi_knn_search_grouped");
  mi_group_info info;
  std::memset(&info, 0, sizeof info);
  if (out_info) *out_info = info;
  std::lock_guard<std::mutex> lock(g->mu);
  int rc = groups_in_step(g);
  if (rc != MI_OK) return rc;
  HIPC(hipSetDevice(g->device));
  const auto t0 = std::chrono::steady_clock::now();
  auto& gs = g->groups;
  const int64_t n = g->n, G = gs.plan.groups();
  info.groups = G;
  if (nq == 0) {
    if (out_info) *out_info = info;
    if (out_seconds) *out_seconds = 0.0;
    return MI_OK;
  }
  int64_t elems;
  if ((rc = strided_extent(nq, g->d, row_stride, col_stride, &elems)) != MI_OK) return rc;
  const size_t esz = q_dtype == MI_F32 ? 4 : 8;
  hipStream_t s = g->stream;
  // the workspace and the staging are the search's: a deferred tail of an earlier batch still reads them
  if ((rc = join_tails(g, s)) != MI_OK) return rc;
  HIPC(hipStreamSynchronize(s));
  if ((rc = ws_ensure(g, std::max<int32_t>(1, g->ws.kcap))) != MI_OK) return rc;     // the flags word lives there
  // the sticky flags belong to the searches around this call: kept aside, put back at the end (as mi_knn_search_filtered does)
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
    if (out_info) *out_info = info;
    if (code == MI_OK && out_seconds)
      *out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return code;
  };

  // the excluded group of every query as a dense id
  std::vector<uint32_t> excl((size_t)nq, GROUP_NONE);
  if (exclude_labels)
    for (int64_t i = 0; i < nq; ++i) {
      excl[(size_t)i] = group_plan_find(gs.plan, exclude_labels[i]);
      info.excluded_found += excl[(size_t)i] != GROUP_NONE;
    }
  if ((rc = gs.excl.grow((size_t)nq)) != MI_OK) return done(rc);
  if (hipMemcpy(gs.excl, excl.data(), (size_t)nq * 4, hipMemcpyHostToDevice) != hipSuccess)
    return done(fail(MI_ERR_HIP, "H2D copy of the excluded groups failed"));
  // queries: the host staging of mi_knn_search (grow-only slot 0)
  void* qd = io_stage(g->io_q, (size_t)elems * esz);
  if (!qd) return done(fail(MI_ERR_NOMEM, "staging buffer of mi_knn_search_grouped"));
  if (hipMemcpy(qd, q, (size_t)elems * esz, hipMemcpyHostToDevice) != hipSuccess)
    return done(fail(MI_ERR_HIP, "H2D query copy failed"));
  if ((rc = grow_all((size_t)nq * k, gs.idx, gs.sc, gs.lab)) != MI_OK) return done(rc);
  // the answer [m][k] of a path in idx / sc / lab -> the caller's rows `rows` (NULL: rows 0 .. m - 1)
  auto to_host = [&](int64_t m, const std::vector<int64_t>* rows) -> int {
    const size_t cnt = (size_t)m * k;
    std::vector<int64_t> hi;
    std::vector<float> hs;
    std::vector<int32_t> hl;
    if (rows) hi.resize(cnt), hs.resize(out_score ? cnt : 0), hl.resize(out_label ? cnt : 0);
    if (hipMemcpyAsync(rows ? hi.data() : out_idx, gs.idx, cnt * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        (out_score && hipMemcpyAsync(rows ? hs.data() : out_score, gs.sc, cnt * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
        (out_label && hipMemcpyAsync(rows ? hl.data() : out_label, gs.lab, cnt * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
        hipStreamSynchronize(s) != hipSuccess)
      return fail(MI_ERR_HIP, "D2H copy of the grouped results failed");
    if (rows)
      for (int64_t r = 0; r < m; ++r) {
        const size_t o = (size_t)(*rows)[(size_t)r] * k;
        std::memcpy(out_idx + o, hi.data() + (size_t)r * k, (size_t)k * 8);
        if (out_score) std::memcpy(out_score + o, hs.data() + (size_t)r * k, (size_t)k * 4);
        if (out_label) std::memcpy(out_label + o, hl.data() + (size_t)r * k, (size_t)k * 4);
      }
    return MI_OK;
  };

  info.path = g->group_path == 1 ? 1 : 2;
  if (info.path == 1) {
    if ((rc = group_fallback(g, qd, q_dtype, row_stride, col_stride, nq, k, gs.excl)) != MI_OK) return done(rc);
    return done(to_host(nq, nullptr));
  }

  // path 2: over-fetch at depth K', collapse, certify
  const int64_t want = (int64_t)g_group_overfetch.load() * k + 32;
  const int32_t kp = (int32_t)std::min<int64_t>({want, 2048, (int64_t)g->rescore_cap, (int64_t)(g->surv_cap / 4), n});
  const int32_t covers = kp >= n ? 1 : 0;
  info.kprime = kp;
  int64_t* tidx = (int64_t*)io_stage(g->io_idx, (size_t)nq * kp * 8);
  float* tsc = (float*)io_stage(g->io_sc, (size_t)nq * kp * 4);
  if (!tidx || !tsc) return done(fail(MI_ERR_NOMEM, "staging buffers of mi_knn_search_grouped"));
  if ((rc = gs.ok.grow((size_t)nq)) != MI_OK) return done(rc);
  if ((rc = search_sync(g, qd, q_dtype, row_stride, col_stride, g->norm_mode, nq, kp, tidx, tsc, nullptr)) != MI_OK) return done(rc);
  launch_group_collapse(tidx, tsc, nq, kp, k, gs.grp, gs.label_of_group, n, g->row_offset, gs.excl, covers, gs.idx, gs.sc, gs.lab,
                        gs.ok, s);
  if (hipGetLastError() != hipSuccess) return done(fail(MI_ERR_HIP, "group_collapse_kernel launch failed"));
  std::vector<uint32_t> ok((size_t)nq);
  if (hipMemcpyAsync(ok.data(), gs.ok, (size_t)nq * 4, hipMemcpyDeviceToHost, s) != hipSuccess)
    return done(fail(MI_ERR_HIP, "D2H copy of the certificates failed"));
  if ((rc = to_host(nq, nullptr)) != MI_OK) return done(rc);
  std::vector<int64_t> rerun;
  for (int64_t i = 0; i < nq; ++i)
    if (!ok[(size_t)i]) rerun.push_back(i);
  info.rerun_queries = (int64_t)rerun.size();
  if (rerun.empty()) return done(MI_OK);
  // the queries it could not certify, packed [m][d] on the host with their excluded groups, answered by path 1
  const int64_t m = (int64_t)rerun.size();
  const int32_t d = g->d;
  std::vector<char> packed((size_t)m * d * esz);
  std::vector<uint32_t> rexcl((size_t)m);
  for (int64_t r = 0; r < m; ++r) {
    const char* src = (const char*)q + (size_t)rerun[(size_t)r] * row_stride * esz;
    char* dst = packed.data() + (size_t)r * d * esz;
    if (col_stride == 1) std::memcpy(dst, src, (size_t)d * esz);
    else
      for (int32_t c = 0; c < d; ++c) std::memcpy(dst + (size_t)c * esz, src + (size_t)c * col_stride * esz, esz);
    rexcl[(size_t)r] = excl[(size_t)rerun[(size_t)r]];
  }
  if ((rc = gs.qbuf.grow(packed.size())) != MI_OK) return done(rc);
  if (hipMemcpy(gs.qbuf, packed.data(), packed.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(gs.excl, rexcl.data(), (size_t)m * 4, hipMemcpyHostToDevice) != hipSuccess)
    return done(fail(MI_ERR_HIP, "H2D copy of the re-run queries failed"));
  if ((rc = group_fallback(g, gs.qbuf, q_dtype, d, 1, m, k, gs.excl)) != MI_OK) return done(rc);
  return done(to_host(m, &rerun));
}

}  // extern "C"
