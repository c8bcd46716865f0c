// Row removal in place (mi_gallery_remove_rows): the rows a bitmap names leave the gallery, the survivors keep their order and
// are renumbered 0 .. n' - 1 (faiss IndexFlat.remove_ids).  DESIGN.md 5.12.  Afterwards every section of the prepared gallery
// holds the bits the same ingest path would have written for the surviving source rows alone, at the same image type: nothing is
// re-rounded, rows and image chunks are moved.  Device memory beyond the gallery: one grow-only arena on the handle with a
// staging area of B rows (global option "remove_block_rows"), the keep-list, the bitmap and the scan buffers.
#include "api_internal.h"

constexpr int64_t REMOVE_BLOCK_ROWS_DEFAULT = 32768;     // 403 MB of staging at D = 2048; a first choice, no sweep yet

static void diffusion_state_free(mi_gallery* g) {
  (void)hipFree(g->dif_ids);
  (void)hipFree(g->dif_vals);
  g->dif_ids = nullptr, g->dif_vals = nullptr, g->dif_T = 0;
}

// The removal itself, with the gallery's lock held by the caller (mi_gallery_remove_rows; mi_ivfflat_remove_rows, which compacts its
// lists by the same bitmap under the same lock)
int gallery_remove_rows_locked(mi_gallery* g, const uint64_t* remove_bits, int memspace, int64_t* out_removed) {
  const int64_t n = g->n;
  if (n == 0) return MI_OK;
  HIPC(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  int rc;
  // a deferred tail of an earlier batch reads the rows it re-scores, and its ids are in the old numbering: it completes first
  if ((rc = join_tails(g, s)) != MI_OK) return rc;
  HIPC(hipStreamSynchronize(s));

  // the bitmap of the rows that STAY, on the host: bits at or beyond n cleared
  const int64_t nwords = (n + 63) / 64;
  std::vector<uint64_t> keep((size_t)nwords);
  if (memspace == MI_HOST) std::memcpy(keep.data(), remove_bits, (size_t)nwords * 8);
  else HIPC(hipMemcpy(keep.data(), remove_bits, (size_t)nwords * 8, hipMemcpyDeviceToHost));
  if (n % 64) keep.back() &= (1ull << (n % 64)) - 1ull;
  int64_t removed = 0, first = -1;
  for (int64_t w = 0; w < nwords; ++w) {
    const uint64_t v = keep[(size_t)w];
    if (v && first < 0) first = w * 64 + __builtin_ctzll(v);
    removed += __builtin_popcountll(v);
    keep[(size_t)w] = ~v;
  }
  if (n % 64) keep.back() &= (1ull << (n % 64)) - 1ull;
  if (removed == 0) return MI_OK;                             // nothing changes, nothing is invalidated
  const int64_t m = n - removed;                              // n'
  const int64_t old_pad = round_up(n, TILE), new_pad = round_up(m, TILE);
  const int64_t start = first / TILE * TILE;                  // rows before the tile of the first removed row stay where they are
  const size_t img_row = (size_t)g->dp * 2;

  if (m == first) {
    // only trailing rows leave: no survivor lies behind a removed row, nothing moves.  The rows [m, new_pad) of the last tile
    // are zeroed where they lie (row r of every slice block: 64 bytes at r * 64, the blocks 16 KiB apart)
    const int64_t r = m % TILE;
    if (r) {
      char* tile = (char*)g->gal_img + (size_t)(m - r) * img_row;
      HIPC(hipMemset2DAsync(tile + (size_t)r * SLICE_K * 2, SLICE_BYTES, 0, (size_t)(TILE - r) * SLICE_K * 2,
                            (size_t)(g->dp / SLICE_K), s));
      HIPC(hipMemsetAsync(g->rowstat + m, 0, (size_t)(TILE - r) * sizeof(RowStat), s));
    }
  } else if (m > start) {
    int64_t B = g_remove_block_rows.load();
    B = round_up(B > 0 ? B : REMOVE_BLOCK_ROWS_DEFAULT, TILE);
    B = std::min<int64_t>(B, round_up(m - start, TILE));
    // one arena, carved: staging (f32 [B][dp], image [B][dp], RowStat[B]), keep-list [m], bitmap [nwords], scan buffers.
    // "remove_block_rows" is an UPPER limit: what the call may add to the device memory in use is bounded by B rows of staging +
    // keep-list + bitmap + 1 MiB ("Memory"), and device memory is handed out in granules (2 MiB on this driver),
    // so the staging area gives up whole tiles until the arena rounded up to a granule stays within that bound
    const int64_t nblk = filter_blocks(n);
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t lists = al((size_t)m * 4) + al((size_t)nwords * 8) + 2 * al((size_t)(nblk + 1) * 4);
    auto arena_bytes = [&](int64_t rows_staged) {
      return al((size_t)rows_staged * g->dp * 4) + al((size_t)rows_staged * img_row) + al((size_t)rows_staged * sizeof(RowStat)) + lists;
    };
    constexpr size_t GRANULE = (size_t)2 << 20;
    const size_t bound = (size_t)B * ((size_t)g->dp * 6 + sizeof(RowStat)) + (size_t)m * 4 + (size_t)nwords * 8 + ((size_t)1 << 20);
    while (B > TILE && (arena_bytes(B) + GRANULE - 1) / GRANULE * GRANULE > bound) B -= TILE;
    const size_t sz[6] = {al((size_t)B * g->dp * 4), al((size_t)B * img_row), al((size_t)B * sizeof(RowStat)), al((size_t)m * 4),
                          al((size_t)nwords * 8), al((size_t)(nblk + 1) * 4)};
    const size_t need = arena_bytes(B);
    if ((rc = g->rm_arena.grow_exact(need)) != MI_OK) return rc;
    char* p = g->rm_arena;
    float* stg_f32 = (float*)p;               p += sz[0];
    void* stg_img = p;                        p += sz[1];
    RowStat* stg_stat = (RowStat*)p;          p += sz[2];
    uint32_t* rows = (uint32_t*)p;            p += sz[3];
    uint64_t* bits = (uint64_t*)p;            p += sz[4];
    uint32_t* bcnt = (uint32_t*)p;            p += sz[5];
    uint32_t* boff = (uint32_t*)p;
    HIPC(hipMemcpyAsync(bits, keep.data(), (size_t)nwords * 8, hipMemcpyHostToDevice, s));
    launch_filter_compact(bits, n, bcnt, boff, rows, s);      // rows[j] = old local row of new row j, ascending
    // Block [i0, i1) of destination rows: its sources rows[i0 .. i1) are gathered into the staging area, then the staging area is
    // written over [i0, i1).  Every surviving row moves down or stays (rows[j] >= j), so the sources of block b + 1 are all
    // >= rows[i1] >= i1, and when they are read nothing at or above i1 has been written yet: the blocks before wrote below i1
    // only.  Within a block the gather completes before the write-back starts (one stream).  The last block also writes the
    // zero padding rows [m, new_pad), which nothing reads afterwards.
    for (int64_t i0 = start; i0 < m; i0 += B) {
      const int64_t i1 = std::min<int64_t>(i0 + B, m), i1_pad = round_up(i1, TILE);
      launch_remove_gather(g->gal_f32, g->gal_img, g->rowstat, rows, i0, i1_pad, m, g->dp, stg_f32, stg_img, stg_stat, s);
      launch_remove_writeback(stg_f32, stg_img, stg_stat, i1 - i0, i1_pad - i0, g->dp, g->gal_f32 + i0 * g->dp,
                              (char*)g->gal_img + (size_t)i0 * img_row, g->rowstat + i0, s);
    }
    HIPC(hipGetLastError());
  }
  // the tail: image rows and rounding norms of the tiles the gallery no longer reaches (appends write their own rows only, and
  // rows n .. npad are saved and checksummed)
  if (old_pad > new_pad) {
    HIPC(hipMemsetAsync((char*)g->gal_img + (size_t)new_pad * img_row, 0, (size_t)(old_pad - new_pad) * img_row, s));
    HIPC(hipMemsetAsync(g->rowstat + new_pad, 0, (size_t)(old_pad - new_pad) * sizeof(RowStat), s));
  }
  // the norm maxima of the survivors (a maximum over the old rows would be one over a superset)
  if (m > 0) launch_rowstat_max(g->rowstat, m, g->gstat3, s);
  else HIPC(hipMemsetAsync(g->gstat3, 0, 12, s));
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));
  g->n = m;
  g->npad = new_pad;
  filter_invalidate(g);          // a remove followed by an append of as many rows restores n: the sub-gallery's key would match
  groups_drop(g);              // the group labels named the old rows
  g->samp_for_n = -1;            // the threshold samples are keyed by n in the same way
  g->samp_f32_for_n = -1;
  diffusion_state_free(g);       // the offline matrix holds ids of the old numbering
  ++g->removals;                 // an index over the raw rows that was not told of this removal sees it, whatever n becomes
  if (out_removed) *out_removed = removed;
  return MI_OK;
}

extern "C" {

int mi_gallery_remove_rows(mi_gallery* g, const uint64_t* remove_bits, int memspace, int64_t* out_removed) {
  REQUIRE(g, "null handle");
  REQUIRE(remove_bits, "null pointer: remove_bits");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  if (out_removed) *out_removed = 0;
  // the worker thread of an online handle searches this gallery between two requests, and its answers are ids
  REQUIRE(g->online_users.load() == 0, "the gallery is in use by an online handle: mi_online_destroy comes first");
  std::lock_guard<std::mutex> lock(g->mu);
  return gallery_remove_rows_locked(g, remove_bits, memspace, out_removed);
}

}  // extern "C"
