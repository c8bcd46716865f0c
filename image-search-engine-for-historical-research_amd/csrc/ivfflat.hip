// Inverted file over the raw rows of a gallery (api_ivfflat.hip): faiss IndexIVFFlat, the reference's
// matching_PQ_Net_bucket without the PQ loss.  A query evaluates only the stored f32 rows whose list is one of its probed lists;
// the value of a (query, row) pair is refine.hip's (l2_direct_wave / refine_dot_wave, float64), the order (value best first, id
// ascending).  The rows stay where the gallery keeps them: a list is a run of LOCAL row numbers, ascending, in list_rows.
//
// Build (the same bytes on every call; the only atomics count rows in LDS, where no order can show):
//   ivff_take_ids_kernel    the int64 answers of launch_refine (k = 1 over the centroid table) -> int32 list ids of a chunk of rows
//   ivff_check_kernel       list ids outside [0, nlist) raise the flag (a caller's device-resident ids)
//   ivff_hist_kernel        workgroup = block of consecutive rows: its rows per list -> hist[list][block]
//   ivff_scan_blocks_kernel workgroup = list: exclusive prefix over its blocks in place, the list's size out
//   ivff_scan_lists_kernel  one workgroup: list_off int64 [nlist + 1] from the sizes
//   ivff_scatter_kernel     workgroup = block, tiles of 256 rows in ascending order: slot = list_off[l] + hist[l][block] + rows of
//                           list l earlier in the block (a running count per list plus the rank inside the tile)
// Update in place (into fresh tables, which the host swaps in; the bytes are those of a build on the gallery as it then stands):
//   ivff_splice_off_kernel  mi_ivfflat_sync: list_off of the old lists + list_off of the lists built from the appended rows alone
//   ivff_splice_kernel      thread = position of the new list_rows (binary search in the new list_off): the old run of its list,
//                           then the tail's run with the old n added
//   ivff_live_kernel        mi_ivfflat_remove_rows: workgroup = block of positions of list_rows, tiles of 256 in ascending order:
//                           survivors (ballots over the keep bitmap) before every tile of the block, and of the block
//   ivff_compact_kernel     the same walk: slot = survivors before the position (block prefix + running count + ballot prefix),
//                           written there the survivor's new number (rank table of the bitmap + popcount below its bit)
//   ivff_live_off_kernel    wave = entry of list_off: the survivors at positions below it
// Search:
//   ivff_prefix_kernel     workgroup = query: normalises a probe row (entries outside [0, nlist) and repeats of an earlier entry
//                           become -1) and writes the prefix of list sizes over it: the query's virtual sequence of candidates
//   ivff_scan_select_kernel the hot path.  Grid = (slab of IVFF_SLAB positions of that sequence, query), 512 threads: a wave resolves
//                           64 positions at a time (lane = position: binary search in the prefix, the row from list_rows, the allow
//                           bit), then evaluates them one row per step with all 64 lanes; entry = (f64_key_nan_highest(value or 0.0 -
//                           value), local row), the sentinel (~0, -1) for rows the bitmap clears and positions beyond the sequence;
//                           the 2048 entries are bitonic-sorted in LDS (32 KiB: five workgroups to a CU) and the first k written to
//                           part[query][slab][k], the rows evaluated to pcnt[query][slab]
//   ivff_merge_kernel       workgroup = query: the sorted partial lists of its slabs -> the k best in order (keeps the best H and
//                           folds in H new entries per bitonic sort of 2 H; H = 1024 for k <= 1024, else 2048), then ids, values
//                           and the number of rows evaluated
// No grid barrier; nothing depends on the launch shape.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "l2_wave.h"
#include "slab_select.h"

namespace mi {

constexpr int IVFF_THREADS = 512, IVFF_WAVES = IVFF_THREADS / 64;
constexpr int IVFF_SLAB = IVFFLAT_SLAB_ROWS;                     // positions per scan workgroup
constexpr int IVFF_WAVE_ROWS = IVFF_SLAB / IVFF_WAVES;           // consecutive positions one wave walks
constexpr int IVFF_TILE = 256;                                   // rows per step of a build workgroup
constexpr uint64_t IVFF_NOKEY = SLAB_NOKEY;

static_assert(IVFF_WAVE_ROWS % 64 == 0, "a wave resolves 64 positions at a time");

// ---- build
__global__ __launch_bounds__(256) void ivff_take_ids_kernel(const int64_t* __restrict__ best, int64_t m, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < m) out[i] = (int32_t)best[i];
}

__global__ __launch_bounds__(256) void ivff_check_kernel(const int32_t* __restrict__ ids, int32_t nlist, int64_t m,
                                                        uint32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < m && (ids[i] < 0 || ids[i] >= nlist)) *flag = 1u;
}

// dynamic LDS: counts [nlist]
__global__ __launch_bounds__(IVFF_TILE) void ivff_hist_kernel(const int32_t* __restrict__ ids, int64_t n, int64_t brows, int32_t nlist,
                                                             int32_t nb, uint32_t* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) char ivff_smem[];
  uint32_t* cnt = reinterpret_cast<uint32_t*>(ivff_smem);
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x, r0 = b * brows, r1 = min(n, r0 + brows);
  for (int32_t l = tid; l < nlist; l += IVFF_TILE) cnt[l] = 0u;
  __syncthreads();
  for (int64_t r = r0 + tid; r < r1; r += IVFF_TILE) atomicAdd(&cnt[ids[r]], 1u);      // (LDS; a count has no order)
  __syncthreads();
  for (int32_t l = tid; l < nlist; l += IVFF_TILE) hist[(int64_t)l * nb + b] = cnt[l];
}

// hist[l][0 .. nb) -> its exclusive prefix, sizes[l] = the sum.  nb <= IVFF_MAX_BLOCKS = 1024: four entries a thread
__global__ __launch_bounds__(256) void ivff_scan_blocks_kernel(uint32_t* __restrict__ hist, int32_t nb, uint32_t* __restrict__ sizes) {
  __shared__ uint32_t s[256];
  const int tid = threadIdx.x;
  uint32_t* row = hist + (int64_t)blockIdx.x * nb;
  uint32_t v[4], mine = 0;
  for (int j = 0; j < 4; ++j) {
    const int i = tid * 4 + j;
    v[j] = i < nb ? row[i] : 0u;
    mine += v[j];
  }
  s[tid] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const uint32_t add = tid >= o ? s[tid - o] : 0u;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  uint32_t run = s[tid] - mine;
  for (int j = 0; j < 4; ++j) {
    const int i = tid * 4 + j;
    if (i < nb) row[i] = run;
    run += v[j];
  }
  if (tid == 255) sizes[blockIdx.x] = s[255];
}

// sizes [nlist], nlist <= 8192: eight entries a thread of 1024
__global__ __launch_bounds__(1024) void ivff_scan_lists_kernel(const uint32_t* __restrict__ sizes, int32_t nlist, int64_t* __restrict__ list_off) {
  __shared__ uint32_t s[1024];
  const int tid = threadIdx.x;
  uint32_t v[8], mine = 0;
  for (int j = 0; j < 8; ++j) {
    const int i = tid * 8 + j;
    v[j] = i < nlist ? sizes[i] : 0u;
    mine += v[j];
  }
  s[tid] = mine;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const uint32_t add = tid >= o ? s[tid - o] : 0u;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  uint32_t run = s[tid] - mine;
  for (int j = 0; j < 8; ++j) {
    const int i = tid * 8 + j;
    if (i < nlist) list_off[i] = (int64_t)run;
    run += v[j];
  }
  if (tid == 1023) list_off[nlist] = (int64_t)s[1023];
}

// dynamic LDS: running counts [nlist] | the tile's list ids [IVFF_TILE]
__global__ __launch_bounds__(IVFF_TILE) void ivff_scatter_kernel(const int32_t* __restrict__ ids, int64_t n, int64_t brows, int32_t nlist,
                                                                int32_t nb, const uint32_t* __restrict__ hist,
                                                                const int64_t* __restrict__ list_off, int32_t* __restrict__ list_rows) {
  extern __shared__ __attribute__((aligned(16))) char ivff_smem[];
  uint32_t* cnt = reinterpret_cast<uint32_t*>(ivff_smem);
  int32_t* tl = reinterpret_cast<int32_t*>(cnt + nlist);
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x, r0 = b * brows, r1 = min(n, r0 + brows);
  for (int32_t l = tid; l < nlist; l += IVFF_TILE) cnt[l] = 0u;
  for (int64_t t0 = r0; t0 < r1; t0 += IVFF_TILE) {               // (uniform over the workgroup)
    const int64_t r = t0 + tid;
    const int32_t l = r < r1 ? ids[r] : -1;
    __syncthreads();                                              // the counts and the last tile's ids are done with
    tl[tid] = l;
    __syncthreads();
    uint32_t before = 0, all = 0;
    if (l >= 0) {
      for (int j = 0; j < IVFF_TILE; ++j) {
        const uint32_t same = tl[j] == l ? 1u : 0u;
        all += same;
        before += j < tid ? same : 0u;
      }
      list_rows[list_off[l] + hist[(int64_t)l * nb + b] + cnt[l] + before] = (int32_t)r;
    }
    __syncthreads();
    if (l >= 0 && before == 0) cnt[l] += all;                     // one thread per list of the tile
  }
}

// ---- update in place: splice (mi_ivfflat_sync)
// new_off[l] = old_off[l] + tail_off[l], l in [0, nlist]
__global__ __launch_bounds__(256) void ivff_splice_off_kernel(const int64_t* __restrict__ old_off, const int64_t* __restrict__ tail_off,
                                                             int32_t nlist, int64_t* __restrict__ new_off) {
  const int32_t l = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (l <= nlist) new_off[l] = old_off[l] + tail_off[l];
}

// thread = position p of the new list_rows [n_new]: its list is the last l with new_off[l] <= p (empty lists have empty ranges), its
// entry the old run of that list followed by the tail's run with n_old added.  A list may hold anything from no row to every row:
// the work is dealt out by position, not by list
__global__ __launch_bounds__(256) void ivff_splice_kernel(const int64_t* __restrict__ old_off, const int32_t* __restrict__ old_rows,
                                                         const int64_t* __restrict__ tail_off, const int32_t* __restrict__ tail_rows,
                                                         const int64_t* __restrict__ new_off, int32_t nlist, int64_t n_old, int64_t n_new,
                                                         int32_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_new) return;
  int32_t lo = 0, hi = nlist - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (new_off[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  const int64_t j = p - new_off[lo], a = old_off[lo], old_size = old_off[lo + 1] - a;
  out[p] = j < old_size ? old_rows[a + j] : (int32_t)(n_old + tail_rows[tail_off[lo] + (j - old_size)]);
}

// ---- update in place: compaction (mi_ivfflat_remove_rows).  keep [ceil(n / 64)]: the rows that stay; rank [ceil(n / 64) + 1]: the
// exclusive count of keep bits per word.  The lists lie one behind the other in list_rows and the renumbering is monotone, so the new
// list_rows is the old one with the entries of removed rows taken out and the others renumbered, in place order: ONE ordered
// compaction over the positions, and new list_off[l] = the survivors at positions below old list_off[l]
__device__ __forceinline__ bool ivff_stays(const uint64_t* __restrict__ keep, uint32_t row) {
  return (keep[row >> 6] >> (row & 63u)) & 1ull;
}

// workgroup = block of brows consecutive positions (brows a multiple of IVFF_TILE), tiles in ascending order: tpre[tile] = survivors
// of the block before the tile, bcnt[block] = survivors of the block
__global__ __launch_bounds__(IVFF_TILE) void ivff_live_kernel(const int32_t* __restrict__ list_rows, int64_t n, int64_t brows,
                                                             const uint64_t* __restrict__ keep, uint32_t* __restrict__ tpre,
                                                             uint32_t* __restrict__ bcnt) {
  __shared__ uint32_t s_w[IVFF_TILE / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x, r0 = b * brows, r1 = min(n, r0 + brows);
  uint32_t run = 0;
  for (int64_t t0 = r0; t0 < r1; t0 += IVFF_TILE) {                 // (uniform over the workgroup)
    const int64_t p = t0 + tid;
    const bool live = p < r1 && ivff_stays(keep, (uint32_t)list_rows[p]);
    const uint64_t mask = __ballot(live);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (tid == 0) tpre[t0 / IVFF_TILE] = run;
    for (int w = 0; w < IVFF_TILE / 64; ++w) run += s_w[w];
    __syncthreads();                                                // the counts are read before the next tile writes them
  }
  if (tid == 0) bcnt[b] = run;
}

// the same walk; a survivor's slot = boff[block] + survivors of the block in earlier tiles + in earlier waves of the tile + in lower
// lanes of its wave (ballot), and what is written there is its new number rank[w] + popcount(keep[w] below its bit)
__global__ __launch_bounds__(IVFF_TILE) void ivff_compact_kernel(const int32_t* __restrict__ list_rows, int64_t n, int64_t brows,
                                                                const uint64_t* __restrict__ keep, const uint32_t* __restrict__ rank,
                                                                const uint32_t* __restrict__ boff, int32_t* __restrict__ out) {
  __shared__ uint32_t s_w[IVFF_TILE / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x, r0 = b * brows, r1 = min(n, r0 + brows);
  int64_t run = boff[b];
  for (int64_t t0 = r0; t0 < r1; t0 += IVFF_TILE) {
    const int64_t p = t0 + tid;
    const uint32_t row = p < r1 ? (uint32_t)list_rows[p] : 0u;
    const bool live = p < r1 && ivff_stays(keep, row);
    const uint64_t mask = __ballot(live);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), all = 0;
    for (int w = 0; w < IVFF_TILE / 64; ++w) {
      before += w < wave ? s_w[w] : 0u;
      all += s_w[w];
    }
    if (live) out[run + before] = (int32_t)(rank[row >> 6] + (uint32_t)__popcll(keep[row >> 6] & ((1ull << (row & 63u)) - 1ull)));
    run += all;
    __syncthreads();
  }
}

// wave = entry l of list_off, l in [0, nlist]: new_off[l] = survivors at positions below p = old_off[l] = boff[block of p] +
// tpre[tile of p] + the survivors among the at most IVFF_TILE - 1 positions of that tile below p; p == n: all of them.  No barrier
__global__ __launch_bounds__(256) void ivff_live_off_kernel(const int64_t* __restrict__ old_off, const int32_t* __restrict__ list_rows,
                                                           int64_t n, int64_t brows, int32_t nlist, const uint64_t* __restrict__ keep,
                                                           const uint32_t* __restrict__ boff, const uint32_t* __restrict__ tpre,
                                                           const uint32_t* __restrict__ total, int64_t* __restrict__ new_off) {
  const int lane = threadIdx.x & 63;
  const int32_t l = (int32_t)(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (l > nlist) return;                                            // (wave-uniform)
  const int64_t p = old_off[l];
  if (p >= n) {
    if (lane == 0) new_off[l] = (int64_t)total[0];
    return;
  }
  const int64_t t0 = p / IVFF_TILE * IVFF_TILE;
  uint32_t c = 0;
  for (int j = 0; j < IVFF_TILE / 64; ++j) {
    const int64_t pos = t0 + j * 64 + lane;
    c += (uint32_t)__popcll(__ballot(pos < p && ivff_stays(keep, (uint32_t)list_rows[pos < p ? pos : t0])));
  }
  if (lane == 0) new_off[l] = (int64_t)boff[t0 / brows] + tpre[t0 / IVFF_TILE] + c;
}

// ---- probes in [nq][nprobe] (the library's int64 answers or the caller's int32) -> norm [nq][nprobe] (-1 = no list), pref
// [nq][nprobe + 1].  Dynamic LDS: first [nlist] int32 | counts [nprobe] int32 | scan [256] int32
// (no static LDS beside it: the kernel's dynamic limit is raised to the whole 160 KiB).  first[l] = the lowest position that names list l
// (an LDS minimum: no order can show)
template <typename InT>
__global__ __launch_bounds__(256) void ivff_prefix_kernel(const InT* __restrict__ in, int32_t nlist, int32_t nprobe,
                                                         const int64_t* __restrict__ list_off, int32_t* __restrict__ norm,
                                                         int32_t* __restrict__ pref) {
  extern __shared__ __attribute__((aligned(16))) char ivff_smem[];
  int32_t* first = reinterpret_cast<int32_t*>(ivff_smem);
  int32_t* cnt = first + nlist;
  int32_t* s = cnt + nprobe;
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  for (int32_t l = tid; l < nlist; l += 256) first[l] = 0x7fffffff;
  __syncthreads();
  for (int32_t i = tid; i < nprobe; i += 256) {
    const int64_t v = (int64_t)in[q * nprobe + i];
    if (v >= 0 && v < nlist) atomicMin(&first[v], i);
  }
  __syncthreads();
  for (int32_t i = tid; i < nprobe; i += 256) {
    int64_t v = (int64_t)in[q * nprobe + i];
    if (v < 0 || v >= nlist || first[v] != i) v = -1;
    norm[q * nprobe + i] = (int32_t)v;
    cnt[i] = v >= 0 ? (int32_t)(list_off[v + 1] - list_off[v]) : 0;
  }
  __syncthreads();
  // the prefix: thread t owns a run of consecutive entries, the runs are scanned over the threads
  const int32_t per = (nprobe + 255) / 256, e0 = min(nprobe, tid * per), e1 = min(nprobe, e0 + per);
  int32_t mine = 0;
  for (int32_t i = e0; i < e1; ++i) mine += cnt[i];
  s[tid] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int32_t add = tid >= o ? s[tid - o] : 0;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  int32_t run = s[tid] - mine;
  int32_t* o = pref + q * (nprobe + 1);
  for (int32_t i = e0; i < e1; ++i) {
    o[i] = run;
    run += cnt[i];
  }
  if (tid == 255) o[nprobe] = s[255];
}

// ---- scan and select.  qry [nq][dp] (16-byte aligned rows); probes: the NORMALISED probes; part_* [nq][nslab][k]; pcnt [nq][nslab]
template <bool L2>
__global__ __launch_bounds__(IVFF_THREADS) void ivff_scan_select_kernel(const float* __restrict__ gal_f32, const float* __restrict__ qry,
                                                                       int32_t dp, int32_t d, const int64_t* __restrict__ list_off,
                                                                       const int32_t* __restrict__ list_rows,
                                                                       const int32_t* __restrict__ probes, const int32_t* __restrict__ pref,
                                                                       int32_t nprobe, const uint64_t* __restrict__ allow, int32_t k,
                                                                       int32_t nslab, uint64_t* __restrict__ part_key,
                                                                       int64_t* __restrict__ part_id, uint32_t* __restrict__ pcnt) {
  __shared__ uint64_t s_key[IVFF_SLAB];
  __shared__ int64_t s_id[IVFF_SLAB];
  const int64_t q = blockIdx.y;
  const int32_t slab = (int32_t)blockIdx.x;
  const int32_t* qpref = pref + q * (nprobe + 1);
  const int32_t* qprobe = probes + q * nprobe;
  const int64_t total = qpref[nprobe];                               // candidates of this query
  // the merge reads only the slabs below the query's count, so nothing is written here.  The condition is uniform over the
  // workgroup and stands before every barrier: it must stay both
  if ((int64_t)slab * IVFF_SLAB >= total) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* qrow = qry + q * dp;
  for (int32_t g0 = 0; g0 < IVFF_WAVE_ROWS; g0 += 64) {
    const int32_t slot = wave * IVFF_WAVE_ROWS + g0 + lane;
    const int64_t v = (int64_t)slab * IVFF_SLAB + slot;
    int32_t row = -1;
    if (v < total) {
      // the probe whose range [pref[i], pref[i + 1]) holds v: the last i with pref[i] <= v (empty probes have empty ranges)
      int32_t lo = 0, hi = nprobe - 1;
      while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)qpref[mid] <= v) lo = mid;
        else hi = mid - 1;
      }
      const int32_t l = qprobe[lo];                                   // >= 0: its range is not empty
      row = list_rows[list_off[l] + (v - (int64_t)qpref[lo])];
      if (allow && !((allow[(uint32_t)row >> 6] >> ((uint32_t)row & 63u)) & 1ull)) row = -1;
    }
    const uint64_t live = __ballot(row >= 0);
    uint64_t key = IVFF_NOKEY;
    for (int j = 0; j < 64; ++j) {
      if (!((live >> j) & 1ull)) continue;                            // (wave-uniform)
      const int32_t r = __shfl(row, j);
      const float* grow = gal_f32 + (int64_t)r * dp;
      const double val = L2 ? l2_direct_wave(qrow, grow, d, lane) : refine_dot_wave(qrow, grow, d, lane);
      if (lane == j) key = f64_key_nan_highest(L2 ? val : 0.0 - val);
    }
    s_key[slot] = key;
    s_id[slot] = (int64_t)row;
  }
  __syncthreads();
  slab_sort<IVFF_SLAB, IVFF_THREADS>(s_key, s_id, tid);
  const int64_t o = ((int64_t)q * nslab + slab) * k;
  for (int32_t i = tid; i < k; i += IVFF_THREADS) {                   // k <= IVFF_SLAB
    part_key[o + i] = s_key[i];
    part_id[o + i] = s_id[i];
  }
  if (tid == 0) {                                                    // the rows evaluated: every one of them sorts before the sentinels
    uint32_t lo = 0, hi = IVFF_SLAB;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s_id[mid] >= 0) lo = mid + 1;
      else hi = mid;
    }
    pcnt[(int64_t)q * nslab + slab] = lo;
  }
}

// ---- merge.  Dynamic LDS: keys [2 HALF] u64 | ids [2 HALF] i64; [0, HALF) is the best so far (sorted after every pass), [HALF,
// 2 HALF) takes the next HALF entries of the query's partial lists read as one stream of slabs * k entries.  k <= HALF
template <bool L2, int HALF>
__global__ __launch_bounds__(IVFF_THREADS) void ivff_merge_kernel(const uint64_t* __restrict__ part_key, const int64_t* __restrict__ part_id,
                                                                 const uint32_t* __restrict__ pcnt, const int32_t* __restrict__ pref,
                                                                 int32_t nprobe, int32_t k, int32_t nslab, int64_t row_offset,
                                                                 int64_t* __restrict__ out_idx, float* __restrict__ out_val,
                                                                 double* __restrict__ out_val64, int64_t* __restrict__ out_scanned) {
  extern __shared__ __attribute__((aligned(16))) char ivff_smem[];
  uint64_t* s_key = reinterpret_cast<uint64_t*>(ivff_smem);
  int64_t* s_id = reinterpret_cast<int64_t*>(s_key + 2 * HALF);
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t total = pref[q * (nprobe + 1) + nprobe];
  const int32_t slabs = (int32_t)min((int64_t)nslab, (total + IVFF_SLAB - 1) / IVFF_SLAB);
  if (out_scanned) {                                                 // the rows evaluated: a sum over the slabs, in s_key for a moment
    uint64_t c = 0;
    for (int32_t s = tid; s < slabs; s += IVFF_THREADS) c += pcnt[q * nslab + s];
    s_key[tid] = c;
    __syncthreads();
    for (int o = IVFF_THREADS / 2; o > 0; o >>= 1) {
      if (tid < o) s_key[tid] += s_key[tid + o];
      __syncthreads();
    }
    if (tid == 0) out_scanned[q] = (int64_t)s_key[0];
    __syncthreads();
  }
  const int64_t count = (int64_t)slabs * k;
  const uint64_t* skey = part_key + (int64_t)q * nslab * k;
  const int64_t* sid = part_id + (int64_t)q * nslab * k;
  slab_stream_best<HALF, IVFF_THREADS>(s_key, s_id, count, tid, [&](int64_t i, uint64_t& key, int64_t& id) {
    key = skey[i];
    id = sid[i];
  });
  slab_emit<L2, IVFF_THREADS>(s_key, s_id, k, q, row_offset, out_idx, out_val, out_val64, tid);
}

// ---- launchers
void launch_ivff_take_ids(const int64_t* best, int64_t m, int32_t* out, hipStream_t stream) {
  if (m <= 0) return;
  ivff_take_ids_kernel<<<dim3((unsigned)((m + 255) / 256)), 256, 0, stream>>>(best, m, out);
}

void launch_ivff_check(const int32_t* ids, int32_t nlist, int64_t m, uint32_t* flag, hipStream_t stream) {
  if (m <= 0) return;
  ivff_check_kernel<<<dim3((unsigned)((m + 255) / 256)), 256, 0, stream>>>(ids, nlist, m, flag);
}

void launch_ivff_lists(const int32_t* ids, int64_t n, int32_t nlist, uint32_t* hist, uint32_t* sizes, int64_t* list_off, int32_t* list_rows,
                       hipStream_t stream) {
  if (n <= 0) return;
  const int64_t brows = ivff_block_rows(n);
  const int32_t nb = (int32_t)((n + brows - 1) / brows);
  ensure_dynamic_lds((const void*)ivff_hist_kernel);
  ensure_dynamic_lds((const void*)ivff_scatter_kernel);
  ivff_hist_kernel<<<dim3((unsigned)nb), IVFF_TILE, (size_t)nlist * 4, stream>>>(ids, n, brows, nlist, nb, hist);
  ivff_scan_blocks_kernel<<<dim3((unsigned)nlist), 256, 0, stream>>>(hist, nb, sizes);
  ivff_scan_lists_kernel<<<dim3(1), 1024, 0, stream>>>(sizes, nlist, list_off);
  ivff_scatter_kernel<<<dim3((unsigned)nb), IVFF_TILE, (size_t)nlist * 4 + IVFF_TILE * 4, stream>>>(ids, n, brows, nlist, nb, hist, list_off,
                                                                                                  list_rows);
}

void launch_ivff_splice(const int64_t* old_off, const int32_t* old_rows, const int64_t* tail_off, const int32_t* tail_rows, int32_t nlist,
                        int64_t n_old, int64_t m, int64_t* new_off, int32_t* new_rows, hipStream_t stream) {
  if (m <= 0) return;
  const int64_t n_new = n_old + m;
  ivff_splice_off_kernel<<<dim3((unsigned)(nlist / 256 + 1)), 256, 0, stream>>>(old_off, tail_off, nlist, new_off);
  ivff_splice_kernel<<<dim3((unsigned)((n_new + 255) / 256)), 256, 0, stream>>>(old_off, old_rows, tail_off, tail_rows, new_off, nlist, n_old,
                                                                               n_new, new_rows);
}

void launch_ivff_compact(const int64_t* old_off, const int32_t* old_rows, int64_t n, int32_t nlist, const uint64_t* keep,
                         const uint32_t* rank, uint32_t* tpre, uint32_t* bcnt, uint32_t* total, int64_t* new_off, int32_t* new_rows,
                         hipStream_t stream) {
  if (n <= 0) return;
  const int64_t brows = ivff_block_rows(n);
  const int32_t nb = (int32_t)((n + brows - 1) / brows);
  ivff_live_kernel<<<dim3((unsigned)nb), IVFF_TILE, 0, stream>>>(old_rows, n, brows, keep, tpre, bcnt);
  ivff_scan_blocks_kernel<<<dim3(1), 256, 0, stream>>>(bcnt, nb, total);           // bcnt -> its exclusive prefix, total[0] = n'
  ivff_compact_kernel<<<dim3((unsigned)nb), IVFF_TILE, 0, stream>>>(old_rows, n, brows, keep, rank, bcnt, new_rows);
  ivff_live_off_kernel<<<dim3((unsigned)(nlist / 4 + 1)), 256, 0, stream>>>(old_off, old_rows, n, brows, nlist, keep, bcnt, tpre, total,
                                                                           new_off);
}

void launch_ivff_prefix(const void* in, int in_is_i64, int64_t nq, int32_t nlist, int32_t nprobe, const int64_t* list_off, int32_t* norm,
                        int32_t* pref, hipStream_t stream) {
  if (nq <= 0) return;
  const size_t lds = ((size_t)nlist + nprobe + 256) * 4;
  if (in_is_i64) {
    ensure_dynamic_lds((const void*)ivff_prefix_kernel<int64_t>);
    ivff_prefix_kernel<int64_t><<<dim3((unsigned)nq), 256, lds, stream>>>((const int64_t*)in, nlist, nprobe, list_off, norm, pref);
  } else {
    ensure_dynamic_lds((const void*)ivff_prefix_kernel<int32_t>);
    ivff_prefix_kernel<int32_t><<<dim3((unsigned)nq), 256, lds, stream>>>((const int32_t*)in, nlist, nprobe, list_off, norm, pref);
  }
}

template <bool L2>
static void ivff_search_launch(const float* gal_f32, const float* qry, int32_t dp, int32_t d, const int64_t* list_off,
                               const int32_t* list_rows, const int32_t* probes, const int32_t* pref, int32_t nprobe, const uint64_t* allow,
                               int32_t k, int32_t nslab, int32_t nq, uint64_t* part_key, int64_t* part_id, uint32_t* pcnt, int64_t row_offset,
                               int64_t* out_idx, float* out_val, double* out_val64, int64_t* out_scanned, hipStream_t stream) {
  ivff_scan_select_kernel<L2><<<dim3((unsigned)nslab, (unsigned)nq), IVFF_THREADS, 0, stream>>>(
      gal_f32, qry, dp, d, list_off, list_rows, probes, pref, nprobe, allow, k, nslab, part_key, part_id, pcnt);
  if (k <= 1024) {
    ensure_dynamic_lds((const void*)ivff_merge_kernel<L2, 1024>);
    ivff_merge_kernel<L2, 1024><<<dim3((unsigned)nq), IVFF_THREADS, 2 * 1024 * 16, stream>>>(
        part_key, part_id, pcnt, pref, nprobe, k, nslab, row_offset, out_idx, out_val, out_val64, out_scanned);
  } else {
    ensure_dynamic_lds((const void*)ivff_merge_kernel<L2, 2048>);
    ivff_merge_kernel<L2, 2048><<<dim3((unsigned)nq), IVFF_THREADS, 2 * 2048 * 16, stream>>>(
        part_key, part_id, pcnt, pref, nprobe, k, nslab, row_offset, out_idx, out_val, out_val64, out_scanned);
  }
}

void launch_ivff_search(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int l2, const int64_t* list_off,
                        const int32_t* list_rows, const int32_t* probes, const int32_t* pref, int32_t nprobe, const uint64_t* allow,
                        int32_t k, int32_t nslab, int32_t nq, uint64_t* part_key, int64_t* part_id, uint32_t* pcnt, int64_t row_offset,
                        int64_t* out_idx, float* out_val, double* out_val64, int64_t* out_scanned, hipStream_t stream) {
  if (nq <= 0 || nslab <= 0) return;
  if (l2)
    ivff_search_launch<true>(gal_f32, qry, dp, d, list_off, list_rows, probes, pref, nprobe, allow, k, nslab, nq, part_key, part_id, pcnt,
                             row_offset, out_idx, out_val, out_val64, out_scanned, stream);
  else
    ivff_search_launch<false>(gal_f32, qry, dp, d, list_off, list_rows, probes, pref, nprobe, allow, k, nslab, nq, part_key, part_id, pcnt,
                              row_offset, out_idx, out_val, out_val64, out_scanned, stream);
}

}  // namespace mi
