// Radius search and self-join on packed binary codes (api_hamming.hip): every admitted row within `radius` bits
// of a query, in CSR form, ordered by (distance asc, id asc).  The layout and the distance loop are hamming.hip's: blocks of 64 rows
// with transposed 32-bit words, lane = gallery row with its words in VGPRs, the query's words at wave-uniform addresses.  There is
// no [queries][n] distance matrix: a (block, query) pair leaves one 64-bit ballot behind.
//
//   hamming_range_scan_kernel     xor / popcount / accumulate, hit = row < n && admitted && distance <= radius; the ballot of a
//                                 (block, query) goes to masks[block][query] (64 queries' masks gathered in the lanes, one
//                                 coalesced store).  With `early`, a pair whose 64 partial sums all exceed the radius after a
//                                 group of words is dropped there: partial sums only grow, so no answer changes
//   hamming_range_segsum_kernel   per query, popcounts of the masks prefixed inside segments of 64 blocks (uint16) + segment sums
//   hamming_range_segscan_kernel  per query, exclusive prefix of the segment sums; the query's hit count into lims[1 + query]
//   hamming_range_lims_kernel     in-place inclusive prefix of lims[1 ..]: the CSR offsets
//   hamming_range_fill_kernel     the pairs with a non-zero mask only: distances again, hit lanes write (distance, row) to the
//                                 staging list at lims[query] + prefix of (query, block) + lane prefix of the mask: id order
//   hamming_range_order_kernel    one wave per query: histogram of its hits' distances (<= radius + 1 bins), exclusive prefix,
//                                 then a stable counting placement in id order -- lanes at equal distance find each other with
//                                 one ballot per distance bit
// Every output position is a prefix sum of ballots: nothing depends on the order in which waves run, and no atomic decides a
// position (the LDS histogram adds are commutative counts).  The self-join reads its queries from the transposed layout itself
// (word w of row i is codes[i >> 6][w][i & 63], still wave-uniform) and reports only rows j > i.
#include "kernels.h"

namespace mi {

constexpr int HR_GROUP = 8;                  // words between two early-exit tests
constexpr int HR_SEG = 64;                   // blocks per segment of the per-query prefix: 63 * 64 < 2^16
constexpr int HR_BINS = 4097;                // distances 0 .. 4096

// the distances of the wave's 64 rows to one query.  SELF: qq points at word 0 of the query row inside the transposed layout
// (stride 64 words, W32 of them); otherwise at NW row-major words, zero padded.  early: see above; a dropped pair returns partial
// sums that are all above the radius on the admitted lanes
template <int NW, bool SELF>
__device__ __forceinline__ uint32_t hr_distance(const uint32_t (&g)[NW], const uint32_t* __restrict__ qq, int32_t W32, bool early,
                                                bool ok, uint32_t radius) {
  uint32_t acc = 0;
  bool live = true;                                        // wave-uniform (no break: the loops unroll and g stays in registers)
#pragma unroll
  for (int w0 = 0; w0 < NW; w0 += HR_GROUP) {
    if (live) {
#pragma unroll
      for (int w = w0; w < w0 + HR_GROUP && w < NW; ++w) {
        const uint32_t qv = SELF ? (w < W32 ? qq[(int64_t)w * 64] : 0u) : qq[w];
        acc += (uint32_t)__popc(g[w] ^ qv);
      }
      if (early && w0 + HR_GROUP < NW) live = __ballot(ok && acc <= radius) != 0ull;
    }
  }
  return acc;
}

// A wave takes block b0 + (4 * blockIdx.x + wave) and the queries [blockIdx.y * qper, + qper) of the chunk; qper is a multiple of
// 64 and the rows of `masks` are qstride >= round_up(nq, 64) words, so whole groups of 64 masks are stored.
template <int NW, bool SELF>
__global__ __launch_bounds__(256) void hamming_range_scan_kernel(const uint32_t* __restrict__ codes, int32_t W32, int64_t b0,
                                                                int64_t nblk, int64_t n, const uint32_t* __restrict__ qsrc,
                                                                int64_t qrow0, int32_t nq, int32_t qper,
                                                                const uint64_t* __restrict__ allow, uint32_t radius, int32_t early,
                                                                unsigned long long* __restrict__ masks, int64_t qstride) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t bl = (int64_t)blockIdx.x * 4 + wave;
  const int64_t b = b0 + bl;
  if (b >= nblk) return;                                   // wave-uniform
  const uint32_t* src = codes + b * W32 * 64 + lane;
  uint32_t g[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) g[w] = w < W32 ? src[(int64_t)w * 64] : 0u;
  const int64_t row = b * 64 + lane;
  bool ok = row < n;
  if (allow) ok = ok && ((allow[b] >> lane) & 1ull);
  const int32_t q0 = (int32_t)blockIdx.y * qper;
  const int32_t q1 = min(nq, q0 + qper);
  unsigned long long* mrow = masks + bl * qstride;
  unsigned long long mine = 0;
  for (int32_t q = q0; q < q1; ++q) {
    unsigned long long m = 0;
    const int64_t qi = qrow0 + q;                          // SELF: the stored row that is query q
    if (!SELF || b * 64 + 63 > qi) {                       // SELF: a block with no row above the query has no pair to report
      const uint32_t* qq = SELF ? qsrc + (qi >> 6) * W32 * 64 + (qi & 63) : qsrc + (int64_t)q * NW;
      const uint32_t acc = hr_distance<NW, SELF>(g, qq, W32, early != 0, ok, radius);
      bool hit = ok && acc <= radius;
      if (SELF) hit = hit && row > qi;
      m = __ballot(hit);
    }
    if (lane == (q & 63)) mine = m;
    if ((q & 63) == 63 || q == q1 - 1) {
      mrow[(q & ~63) + lane] = mine;
      mine = 0;
    }
  }
}

// thread = (query, segment): offs[block][query] = hits of the query in the segment's earlier blocks, seg[segment][query] = its hits
// in the whole segment
__global__ __launch_bounds__(256) void hamming_range_segsum_kernel(const unsigned long long* __restrict__ masks, int64_t nbl,
                                                                  int64_t qstride, int32_t nq, uint16_t* __restrict__ offs,
                                                                  uint32_t* __restrict__ seg) {
  const int32_t q = (int32_t)blockIdx.y * 256 + threadIdx.x;
  if (q >= nq) return;
  const int64_t s = blockIdx.x;
  const int64_t bl1 = min(nbl, (s + 1) * HR_SEG);
  uint32_t run = 0;
  for (int64_t bl = s * HR_SEG; bl < bl1; ++bl) {
    offs[bl * qstride + q] = (uint16_t)run;
    run += (uint32_t)__popcll(masks[bl * qstride + q]);
  }
  seg[s * qstride + q] = run;
}

// thread = query: seg[.][query] becomes its exclusive prefix; the total goes to lims1[query] (lims1 NULL: a chunk done again for
// its fill, the offsets are known)
__global__ __launch_bounds__(256) void hamming_range_segscan_kernel(uint32_t* __restrict__ seg, int64_t nseg, int64_t qstride,
                                                                   int32_t nq, int64_t* __restrict__ lims1) {
  const int32_t q = (int32_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  uint32_t run = 0;
  for (int64_t s = 0; s < nseg; ++s) {
    const uint32_t t = seg[s * qstride + q];
    seg[s * qstride + q] = run;
    run += t;
  }
  if (lims1) lims1[q] = (int64_t)run;
}

// one workgroup: lims[0] = 0, lims[1 + i] = sum of the counts found in lims[1 .. 1 + i]
__global__ __launch_bounds__(1024) void hamming_range_lims_kernel(int64_t* __restrict__ lims, int64_t nq) {
  __shared__ long long wt[2][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) lims[0] = 0;
  long long run = 0;
  int it = 0;
  for (int64_t base = 0; base < nq; base += 1024, ++it) {
    const int64_t i = base + tid;
    const long long v = i < nq ? (long long)lims[1 + i] : 0;
    long long incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    if (lane == 63) wt[it & 1][wave] = incl;
    __syncthreads();
    long long before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const long long x = wt[it & 1][w];
      if (w < wave) before += x;
      tot += x;
    }
    if (i < nq) lims[1 + i] = (int64_t)(run + before + incl);
    run += tot;
  }
}

// lims: the CSR offsets of the chunk's queries (lims[0] = the chunk's first hit); stage holds the chunk's hits from entry 0.
// *total > max_results: the answer does not fit the caller's arrays and nothing is written
template <int NW, bool SELF>
__global__ __launch_bounds__(256) void hamming_range_fill_kernel(const uint32_t* __restrict__ codes, int32_t W32, int64_t b0,
                                                                int64_t nblk, const uint32_t* __restrict__ qsrc, int64_t qrow0,
                                                                int32_t nq, int32_t qper,
                                                                const unsigned long long* __restrict__ masks,
                                                                const uint16_t* __restrict__ offs, const uint32_t* __restrict__ seg,
                                                                int64_t qstride, const int64_t* __restrict__ lims,
                                                                const int64_t* __restrict__ total, int64_t max_results,
                                                                unsigned long long* __restrict__ stage) {
  if (*total > max_results) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t bl = (int64_t)blockIdx.x * 4 + wave;
  const int64_t b = b0 + bl;
  if (b >= nblk) return;                                   // wave-uniform
  const uint32_t* src = codes + b * W32 * 64 + lane;
  uint32_t g[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) g[w] = w < W32 ? src[(int64_t)w * 64] : 0u;
  const int32_t q0 = (int32_t)blockIdx.y * qper;
  const int32_t q1 = min(nq, q0 + qper);
  const unsigned long long* mrow = masks + bl * qstride;
  const int64_t chunk0 = lims[0];
  for (int32_t q = q0; q < q1; ++q) {
    const unsigned long long m = mrow[q];                  // wave-uniform
    if (m == 0ull) continue;
    const int64_t qi = qrow0 + q;
    const uint32_t* qq = SELF ? qsrc + (qi >> 6) * W32 * 64 + (qi & 63) : qsrc + (int64_t)q * NW;
    const uint32_t acc = hr_distance<NW, SELF>(g, qq, W32, false, true, 0u);
    if ((m >> lane) & 1ull) {
      const int64_t pos = lims[q] - chunk0 + seg[(bl / HR_SEG) * qstride + q] + offs[bl * qstride + q] +
                          __popcll(m & ((1ull << lane) - 1ull));
      stage[pos] = ((unsigned long long)acc << 32) | (unsigned long long)(uint32_t)(b * 64 + lane);
    }
  }
}

// one wave per query of the chunk.  nbin = min(radius, nbits) + 1 distance bins
__global__ __launch_bounds__(64) void hamming_range_order_kernel(const unsigned long long* __restrict__ stage,
                                                                const int64_t* __restrict__ lims, const int64_t* __restrict__ total,
                                                                int64_t max_results, int32_t nbin, int64_t row_offset,
                                                                int64_t* __restrict__ out_idx, int32_t* __restrict__ out_dist) {
  __shared__ uint32_t bins[HR_BINS];
  if (*total > max_results) return;
  const int lane = threadIdx.x;
  const int64_t lo = lims[blockIdx.x], cnt = lims[blockIdx.x + 1] - lo;
  if (cnt == 0) return;
  const unsigned long long* src = stage + (lo - lims[0]);
  int64_t* oi = out_idx + lo;
  int32_t* od = out_dist ? out_dist + lo : nullptr;
  if (nbin == 1 || cnt == 1) {                             // one distance class: the id order is the answer
    for (int64_t i = lane; i < cnt; i += 64) {
      const unsigned long long key = src[i];
      oi[i] = row_offset + (int64_t)(key & 0xFFFFFFFFull);
      if (od) od[i] = (int32_t)(key >> 32);
    }
    return;
  }
  for (int j = lane; j < nbin; j += 64) bins[j] = 0;
  __syncthreads();
  for (int64_t i = lane; i < cnt; i += 64) atomicAdd(&bins[(uint32_t)(src[i] >> 32)], 1u);
  __syncthreads();
  // exclusive prefix of the histogram: each lane its run of `per` bins
  const int per = (nbin + 63) / 64;
  const int j0 = min(lane * per, nbin), j1 = min(j0 + per, nbin);
  uint32_t s = 0;
  for (int j = j0; j < j1; ++j) s += bins[j];
  uint32_t incl = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  uint32_t run = incl - s;
  for (int j = j0; j < j1; ++j) {
    const uint32_t t = bins[j];
    bins[j] = run;
    run += t;
  }
  __syncthreads();
  // placement in id order, 64 hits at a time: the lanes at one distance (found by a ballot per distance bit) take consecutive
  // places from the bin's running position, in lane order
  const int dbits = 32 - __clz(nbin - 1);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t base = 0; base < cnt; base += 64) {
    const int64_t i = base + lane;
    const bool valid = i < cnt;
    const unsigned long long key = valid ? src[i] : ~0ull;
    const uint32_t d = (uint32_t)(key >> 32);
    unsigned long long peers = __ballot(valid);
    for (int bit = 0; bit < dbits; ++bit) {
      const bool one = (d >> bit) & 1u;
      const unsigned long long bm = __ballot(one);
      peers &= one ? bm : ~bm;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & below);
    uint32_t start = 0;
    if (valid && rank == 0) {
      start = bins[d];
      bins[d] = start + (uint32_t)__popcll(peers);
    }
    __syncthreads();
    start = __shfl(start, valid ? __ffsll((long long)peers) - 1 : lane, 64);
    if (valid) {
      const int64_t pos = (int64_t)start + rank;
      oi[pos] = row_offset + (int64_t)(key & 0xFFFFFFFFull);
      if (od) od[pos] = (int32_t)d;
    }
  }
}

// ---- launchers
// blocks x query groups of the scan and fill grids: the queries of a chunk are split over blockIdx.y (in multiples of 64) only
// when the blocks alone do not fill the device, as in launch_hamming_dist
static dim3 hr_grid(int64_t nbl, int32_t nq, int32_t* qper) {
  const int64_t want = 4096, groups = (nq + 63) / 64;
  int64_t split = std::min<int64_t>({(want + nbl - 1) / nbl, groups, 65535});
  const int64_t gper = (groups + split - 1) / split;
  split = (groups + gper - 1) / gper;
  *qper = (int32_t)(gper * 64);
  return dim3((unsigned)((nbl + 3) / 4), (unsigned)split);
}

template <int NW, bool SELF>
static void hr_launch2(const HammingRangeArgs& a, bool fill, hipStream_t s) {
  const int32_t W32 = (a.nbits + 31) / 32;
  const int64_t nblk = (a.n + 63) / 64;
  int32_t qper;
  const dim3 grid = hr_grid(nblk - a.b0, a.nq, &qper);
  if (fill)
    hamming_range_fill_kernel<NW, SELF><<<grid, 256, 0, s>>>(a.codes, W32, a.b0, nblk, a.qsrc, a.qrow0, a.nq, qper, a.masks, a.offs,
                                                            a.seg, a.qstride, a.lims, a.total, a.max_results, a.stage);
  else
    hamming_range_scan_kernel<NW, SELF><<<grid, 256, 0, s>>>(a.codes, W32, a.b0, nblk, a.n, a.qsrc, a.qrow0, a.nq, qper, a.allow,
                                                            a.radius, a.early, a.masks, a.qstride);
}

template <int NW>
static void hr_launch(const HammingRangeArgs& a, bool fill, hipStream_t s) {
  if (a.self) hr_launch2<NW, true>(a, fill, s);
  else hr_launch2<NW, false>(a, fill, s);
}

static void hr_dispatch(const HammingRangeArgs& a, bool fill, hipStream_t s) {
  if (a.nq <= 0 || (a.n + 63) / 64 <= a.b0) return;
  switch (hamming_query_words((a.nbits + 31) / 32)) {
    case 1: hr_launch<1>(a, fill, s); break;
    case 2: hr_launch<2>(a, fill, s); break;
    case 3: hr_launch<3>(a, fill, s); break;
    case 4: hr_launch<4>(a, fill, s); break;
    case 6: hr_launch<6>(a, fill, s); break;
    case 8: hr_launch<8>(a, fill, s); break;
    case 12: hr_launch<12>(a, fill, s); break;
    case 16: hr_launch<16>(a, fill, s); break;
    case 24: hr_launch<24>(a, fill, s); break;
    case 32: hr_launch<32>(a, fill, s); break;
    case 48: hr_launch<48>(a, fill, s); break;
    case 64: hr_launch<64>(a, fill, s); break;
    case 96: hr_launch<96>(a, fill, s); break;
    default: hr_launch<128>(a, fill, s); break;
  }
}

void launch_hamming_range_scan(const HammingRangeArgs& a, hipStream_t stream) { hr_dispatch(a, false, stream); }

void launch_hamming_range_offsets(const HammingRangeArgs& a, int64_t* lims1, hipStream_t stream) {
  const int64_t nbl = (a.n + 63) / 64 - a.b0;
  if (a.nq <= 0 || nbl <= 0) return;
  const int64_t nseg = (nbl + HR_SEG - 1) / HR_SEG;
  hamming_range_segsum_kernel<<<dim3((unsigned)nseg, (unsigned)((a.nq + 255) / 256)), 256, 0, stream>>>(a.masks, nbl, a.qstride, a.nq,
                                                                                                      a.offs, a.seg);
  hamming_range_segscan_kernel<<<dim3((unsigned)((a.nq + 255) / 256)), 256, 0, stream>>>(a.seg, nseg, a.qstride, a.nq, lims1);
}

void launch_hamming_range_lims(int64_t* lims, int64_t nq, hipStream_t stream) {
  hamming_range_lims_kernel<<<dim3(1), 1024, 0, stream>>>(lims, nq);
}

void launch_hamming_range_fill(const HammingRangeArgs& a, hipStream_t stream) { hr_dispatch(a, true, stream); }

void launch_hamming_range_order(const HammingRangeArgs& a, int64_t row_offset, int64_t* out_idx, int32_t* out_dist,
                                hipStream_t stream) {
  if (a.nq <= 0) return;
  const int32_t nbin = (int32_t)std::min<uint32_t>(a.radius, (uint32_t)a.nbits) + 1;
  hamming_range_order_kernel<<<dim3((unsigned)a.nq), 64, 0, stream>>>(a.stage, a.lims, a.total, a.max_results, nbin, row_offset,
                                                                     out_idx, out_dist);
}

}  // namespace mi
