// Best-first walk of a neighbour graph, once, for every graph index (graph_search.hip on stored f32 rows, pq_graph_search.hip on
// PQ codes).  Device code; the kernels build a policy P -- what a place of W is and what a row costs -- and call
// graph_walk<P>.
//
// One workgroup of four waves per query.  W, the best `ef` rows seen so far, lives in LDS sorted by the policy's order (value
// best first, id ascending), each place carrying an `expanded` mark that no comparison sees.  One step:
//   1. every thread scans its share of W for the first place not yet expanded, one LDS atomicMin picks the first of all;
//   2. wave 0 reads that row's R table entries, drops -1s, ids outside [0, n), repeats within the row (compared in LDS) and rows
//      whose bit in the query's visited bitmap is already set (the bitmap is exact: n bits per query in HBM, this workgroup's
//      alone, set with atomicOr so that two lanes of the wave may share a word), and compacts the rest by a ballot;
//   3. P::evaluate gives the up to 64 new rows their keys (all 256 threads call it: its barriers stay in uniform control flow);
//   4. the new rows are ordered by rank (each thread counts the rows before its own; their keys are distinct);
//   5. W and the new rows merge by rank into the other half of the double buffer: an element's place is its own index plus the
//      number of elements of the other list before it, found by binary search -- no serial insertion; places >= ef fall off
//      (and stay visited).
// The loop ends when step 1 finds nothing, and after n expansions at the latest whatever the table holds.  No atomics across
// workgroups, no grid barrier; results leave by ordinary vector stores.
//
// Why four waves.  Steps 2 and 4 are one wave's work (at most 64 rows).  The other three are kept for the scan of W, for what the
// policy gives them (a wave per row in step 3, the copy of a table) and above all for the merge, which at ef = 2048 is 2048
// binary searches per step: 8 per thread with 256 threads, 32 with 64.  At small ef they idle at the barriers, which costs little.
//
// A policy P is a plain struct of inline functions:
//   P::Place, P::List  a place of W by value; a list of places in LDS: load(i), store(i, place), mark(i, place) (place i, just
//                      loaded as `place` and not yet expanded, becomes expanded);
//   P::bare(place)     its order key (the mark masked out), P::before(a, b) on bare keys, P::expanded(place), P::row(place) of a
//                      place that is not expanded;
//   w, w2, nw, sn      lists: W, the half the next merge writes, the new rows as evaluated, the new rows in the order (the walk
//                      swaps copies of w and w2 and hands the final W back in w before it calls emit);
//   n_id, s_raw, s_ctl uint32 [64], [64], [4]: the new rows compacted, the table entries as read, [0] the first unexpanded place
//                      and [1] the number of new rows -- like the lists carved by the policy out of the dynamic LDS block;
//   evaluate(m, t)     step 3: nw[0, m) from n_id[0, m);  emit(o, i, have): answer slot o is place i of W, or the padding.
#pragma once
#include "common.h"

namespace mi {

constexpr uint32_t GW_NONE = 0xffffffffu;

// number of places of the sorted list l[0, len) that come before the bare key `key`
template <class P>
__device__ __forceinline__ int gw_rank(const typename P::List& l, int len, const typename P::Place& key) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (P::before(P::bare(l.load(mid)), key)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// adj [n][R]; entries [ne]; vis [gridDim.x][vis_words], all zero on entry (the caller clears it before every launch); answers
// [gridDim.x][k] through p.emit, out_visited [gridDim.x] or NULL.  256 threads
template <class P>
__device__ __forceinline__ void graph_walk(P& p, int64_t n, const int32_t* adj, int32_t R, const int32_t* entries, int32_t ne,
                                           int32_t k, int32_t ef, uint32_t* vis, int64_t vis_words, int32_t* out_visited) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t q = blockIdx.x;
  uint32_t* myvis = vis + q * vis_words;
  typename P::List w = p.w, w2 = p.w2;
  int wn = 0;
  int64_t visited = 0;

  // ---- start: the distinct entry rows are the first batch of new rows, none of them expanded
  if (wv == 0) {
    const int32_t e = lane < ne ? entries[lane] : -1;
    p.s_raw[lane] = (uint32_t)e;
  }
  __syncthreads();
  for (int64_t step = -1; step < n; ++step) {
    if (step >= 0) {
      // 1. the first place of W that is not yet expanded
      if (t == 0) p.s_ctl[0] = GW_NONE;
      __syncthreads();
      for (int i = t; i < wn; i += 256)
        if (!P::expanded(w.load(i))) {
          atomicMin(&p.s_ctl[0], (uint32_t)i);
          break;
        }
      __syncthreads();
      const uint32_t first = p.s_ctl[0];
      if (first == GW_NONE) break;                    // (uniform: every thread reads the same word)
      const typename P::Place place = w.load(first);
      if (wv == 0) p.s_raw[lane] = lane < R ? (uint32_t)adj[(int64_t)P::row(place) * R + lane] : GW_NONE;
      __syncthreads();
      if (t == 0) w.mark(first, place);
    }
    // 2. wave 0: valid, first occurrence within the row, not visited -> n_id[0, m)
    if (wv == 0) {
      const int cnt = step < 0 ? ne : R;
      const uint32_t c = p.s_raw[lane];
      bool keep = lane < cnt && (int32_t)c >= 0 && (int64_t)c < n;
      if (keep)
        for (int j = 0; j < lane; ++j)
          if (p.s_raw[j] == c) {
            keep = false;
            break;
          }
      if (keep) {
        const uint32_t bit = 1u << (c & 31);
        keep = (atomicOr(&myvis[c >> 5], bit) & bit) == 0;
      }
      const unsigned long long m = __ballot(keep);
      if (keep) p.n_id[__popcll(m & ((1ull << lane) - 1))] = c;
      if (lane == 0) p.s_ctl[1] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    const int m = (int)p.s_ctl[1];
    visited += m;
    if (m == 0) continue;                             // (uniform)
    // 3. the keys of the new rows
    p.evaluate(m, t);
    __syncthreads();
    // 4. the new rows in the order
    if (t < m) {
      const typename P::Place key = p.nw.load(t);
      int r = 0;
      for (int j = 0; j < m; ++j) r += P::before(p.nw.load(j), key) ? 1 : 0;
      p.sn.store(r, key);
    }
    __syncthreads();
    // 5. merge by rank into the other half; what lands at ef or beyond is pushed out
    for (int i = t; i < wn; i += 256) {
      const typename P::Place place = w.load(i);
      const int at = i + gw_rank<P>(p.sn, m, P::bare(place));
      if (at < ef) w2.store(at, place);
    }
    if (t < m) {
      const typename P::Place place = p.sn.load(t);
      const int at = t + gw_rank<P>(w, wn, place);
      if (at < ef) w2.store(at, place);
    }
    wn = min(wn + m, ef);
    {
      const typename P::List old = w;
      w = w2, w2 = old;
    }
    __syncthreads();
  }

  p.w = w;
  // ---- answer: the first k places of W
  for (int i = t; i < k; i += 256) p.emit(q * k + i, i, i < wn);
  if (out_visited && t == 0) out_visited[q] = (int32_t)visited;
}

}  // namespace mi
