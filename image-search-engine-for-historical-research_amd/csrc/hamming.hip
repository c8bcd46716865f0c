// Exact Hamming top-K on packed binary codes (api_hamming.hip): the reference's matching_Greedyhash
// (src/utils/nnsearch.py:1001-1013), faiss IndexBinaryFlat.
//
// Gallery layout: blocks of 64 rows with the 32-bit words transposed, codes[block][w][lane], w < W32 = ceil(nbits / 32).  Lane l of
// a wave owns row 64 * block + l: word w of the 64 rows is one coalesced 256-byte read and the row's words stay in VGPRs.  Bit j
// of a code is bit (j & 31) of word (j >> 5), i.e. bit (j & 7) of byte (j >> 3) (np.packbits(bitorder='little')); rows and
// queries are padded with zero bits to whole words, so padding never contributes to a distance.
//
//   hamming_dist_kernel    lane = gallery row, the query's words are wave-uniform (scalar loads): one xor and one popcount-with-
//                          accumulate per (row, query, word); uint16 distances into dist[query][npad]; 0xFFFF = row not admitted
//   hamming_select_kernel  one workgroup per query: LDS histogram of its matrix row -> the K-th distance t; an ordered second scan
//                          collects the (< K) rows below t and the first rows AT t in id order; a stable counting placement
//                          of the former.  Nothing can overflow: both sets are bounded by K by construction of t.
#include "kernels.h"

namespace mi {

// ---- packed bytes [m][stride] -> words of rows row0 .. row0 + m of the transposed layout (thread = (word, row), rows fastest)
__global__ __launch_bounds__(256) void hamming_ingest_kernel(const uint8_t* __restrict__ src, int64_t stride, int32_t nb, int32_t W32,
                                                            int64_t row0, int64_t m, uint32_t* __restrict__ codes) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m * W32) return;
  const int64_t r = i % m;
  const int32_t w = (int32_t)(i / m);
  const uint8_t* p = src + r * stride;
  uint32_t v = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (4 * w + b < nb) v |= (uint32_t)p[4 * w + b] << (8 * b);
  const int64_t row = row0 + r;
  codes[((row >> 6) * W32 + w) * 64 + (row & 63)] = v;
}

// ---- packed query bytes [nq][stride] -> row-major words [nq][wq], zero beyond the code
__global__ __launch_bounds__(256) void hamming_query_words_kernel(const uint8_t* __restrict__ src, int64_t stride, int32_t nb, int32_t wq,
                                                                 int64_t nq, uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq * wq) return;
  const int64_t q = i / wq;
  const int32_t w = (int32_t)(i % wq);
  const uint8_t* p = src + q * stride;
  uint32_t v = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (4 * w + b < nb) v |= (uint32_t)p[4 * w + b] << (8 * b);
  out[i] = v;
}

// ---- distances.  NW >= W32 words per lane in registers (the smallest instantiation that holds the code; queries are stored NW
// words wide, zero padded).  A wave takes one block of 64 rows and the queries [blockIdx.y * qper, + qper).
template <int NW>
__global__ __launch_bounds__(256) void hamming_dist_kernel(const uint32_t* __restrict__ codes, int32_t W32, int64_t nblk, int64_t n,
                                                          const uint32_t* __restrict__ qw, int32_t nq, int32_t qper,
                                                          const uint64_t* __restrict__ allow, uint16_t* __restrict__ dist,
                                                          int64_t npad) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
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
  uint16_t* out = dist + row;
  for (int32_t q = q0; q < q1; ++q) {
    const uint32_t* qq = qw + (int64_t)q * NW;             // wave-uniform address: scalar loads
    uint32_t acc = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) acc += (uint32_t)__popc(g[w] ^ qq[w]);
    out[(int64_t)q * npad] = ok ? (uint16_t)acc : (uint16_t)0xFFFF;
  }
}

// ---- selection
constexpr int HS_THREADS = 1024, HS_WAVES = HS_THREADS / 64;
constexpr int HS_BINS = 4097;                // distances 0 .. 4096
constexpr int HS_PER = 5;                    // bins per thread of the prefix pass: 5 * 1024 >= 4097
constexpr int HS_VEC = 16;                   // matrix elements per thread and chunk of the ordered scan
constexpr int HS_KMAX = 2048;

// exclusive prefix of v over the workgroup in thread order; *total = the sum.  wt: HS_WAVES words nobody else writes until every
// thread has passed the NEXT barrier
__device__ __forceinline__ uint32_t hs_block_scan(uint32_t v, uint32_t* wt, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wt[wave] = incl;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < HS_WAVES; ++w) {
    const uint32_t x = wt[w];
    if (w < wave) base += x;
    tot += x;
  }
  *total = tot;
  return base + incl - v;
}

__global__ __launch_bounds__(HS_THREADS) void hamming_select_kernel(const uint16_t* __restrict__ dist, int64_t npad, int32_t nbits,
                                                                   int32_t k, int64_t row_offset, int64_t* __restrict__ out_idx,
                                                                   int32_t* __restrict__ out_dist) {
  __shared__ uint32_t hist[HS_PER * HS_THREADS];
  __shared__ uint32_t pre[HS_PER * HS_THREADS];
  __shared__ uint32_t cand_id[HS_KMAX];
  __shared__ uint16_t cand_d[HS_KMAX];
  __shared__ uint32_t wt[3][HS_WAVES];
  __shared__ uint32_t s_t, s_cumlt;
  const int tid = threadIdx.x;
  const uint16_t* row = dist + (int64_t)blockIdx.x * npad;
  int64_t* oi = out_idx + (int64_t)blockIdx.x * k;
  int32_t* od = out_dist ? out_dist + (int64_t)blockIdx.x * k : nullptr;
  const uint32_t nbin = (uint32_t)nbits + 1;

  for (int i = tid; i < HS_PER * HS_THREADS; i += HS_THREADS) hist[i] = 0;
  __syncthreads();
  // scan 1: histogram of the admitted rows' distances (npad is a multiple of 64: whole 16-byte vectors)
  const int64_t nvec = npad >> 3;
  for (int64_t v = tid; v < nvec; v += HS_THREADS) {
    const uint4 x = reinterpret_cast<const uint4*>(row)[v];
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t lo = xs[j] & 0xFFFFu, hi = xs[j] >> 16;
      if (lo < nbin) atomicAdd(&hist[lo], 1u);
      if (hi < nbin) atomicAdd(&hist[hi], 1u);
    }
  }
  __syncthreads();
  // exclusive prefix of the histogram; t = the smallest distance with cum(t) >= k
  uint32_t loc[HS_PER], h[HS_PER], s = 0;
#pragma unroll
  for (int j = 0; j < HS_PER; ++j) {
    h[j] = hist[tid * HS_PER + j];
    loc[j] = s;
    s += h[j];
  }
  uint32_t total;
  const uint32_t base = hs_block_scan(s, wt[2], &total);
#pragma unroll
  for (int j = 0; j < HS_PER; ++j) {
    const uint32_t p = base + loc[j];
    pre[tid * HS_PER + j] = p;
    if (p < (uint32_t)k && p + h[j] >= (uint32_t)k) {
      s_t = (uint32_t)(tid * HS_PER + j);
      s_cumlt = p;
    }
  }
  __syncthreads();
  // fewer than k admitted rows: every one of them is "below t", nothing is taken at t
  const bool shortq = total < (uint32_t)k;
  const uint32_t t = shortq ? nbin : s_t;
  const uint32_t cumlt = shortq ? total : s_cumlt;
  const uint32_t need = shortq ? 0u : (uint32_t)k - cumlt;

  // scan 2, ascending ids: rows below t go to the candidate list in id order (cumlt < k of them), the first `need` rows AT t go
  // straight to their final places cumlt, cumlt + 1, ...
  uint32_t lt_run = 0, eq_run = 0;
  int it = 0;
  for (int64_t cbase = 0; cbase < npad && (lt_run < cumlt || eq_run < need); cbase += (int64_t)HS_THREADS * HS_VEC, ++it) {
    const int64_t e0 = cbase + (int64_t)tid * HS_VEC;
    uint32_t xs[HS_VEC / 2];
    if (e0 < npad) {                                        // e0 and npad are multiples of 16: the whole vector is inside
      const uint4 a = reinterpret_cast<const uint4*>(row + e0)[0], c = reinterpret_cast<const uint4*>(row + e0)[1];
      xs[0] = a.x, xs[1] = a.y, xs[2] = a.z, xs[3] = a.w, xs[4] = c.x, xs[5] = c.y, xs[6] = c.z, xs[7] = c.w;
    } else {
#pragma unroll
      for (int j = 0; j < HS_VEC / 2; ++j) xs[j] = 0xFFFFFFFFu;
    }
    uint32_t cnt = 0;                                       // rows below t | rows at t << 16 (both <= 16384 per chunk)
#pragma unroll
    for (int j = 0; j < HS_VEC; ++j) {
      const uint32_t d = (xs[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
      cnt += (d < t ? 1u : 0u) + (d == t ? 0x10000u : 0u);
    }
    uint32_t tot;
    const uint32_t ex = hs_block_scan(cnt, wt[it & 1], &tot);
    uint32_t lt_pos = lt_run + (ex & 0xFFFFu), eq_pos = eq_run + (ex >> 16);
#pragma unroll
    for (int j = 0; j < HS_VEC; ++j) {
      const uint32_t d = (xs[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
      if (d < t) {
        if (lt_pos < HS_KMAX) {                             // (always: cumlt < k <= HS_KMAX)
          cand_d[lt_pos] = (uint16_t)d;
          cand_id[lt_pos] = (uint32_t)(e0 + j);
        }
        ++lt_pos;
      } else if (d == t) {
        if (eq_pos < need) {
          oi[cumlt + eq_pos] = row_offset + e0 + j;
          if (od) od[cumlt + eq_pos] = (int32_t)t;
        }
        ++eq_pos;
      }
    }
    lt_run += tot & 0xFFFFu;
    eq_run += tot >> 16;
  }
  __syncthreads();
  // stable counting placement of the rows below t: pre[d] + the number of earlier list entries at the same distance
  for (uint32_t i = tid; i < cumlt; i += HS_THREADS) {
    const uint16_t d = cand_d[i];
    uint32_t c = 0;
    for (uint32_t j = 0; j < i; ++j) c += cand_d[j] == d ? 1u : 0u;
    const uint32_t pos = pre[d] + c;
    oi[pos] = row_offset + (int64_t)cand_id[i];
    if (od) od[pos] = (int32_t)d;
  }
  for (uint32_t i = (shortq ? total : (uint32_t)k) + tid; i < (uint32_t)k; i += HS_THREADS) {
    oi[i] = -1;
    if (od) od[i] = 0x7FFFFFFF;
  }
}

// ---- sign bits of float rows: bit j = x[j] > 0 (NaN, +-0 -> 0; a positive denormal counts, whatever the float mode), one ballot
// per 64 columns.  out_bytes: rows of d / 8 bytes; else: words of rows row0 .. of the transposed gallery layout
__global__ __launch_bounds__(256) void hamming_sign_kernel(const float* __restrict__ x, int64_t n, int32_t d, int64_t rs,
                                                          uint8_t* __restrict__ out_bytes, int64_t out_rs,
                                                          uint32_t* __restrict__ codes, int32_t W32, int64_t row0) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;                                       // wave-uniform
  const float* xr = x + r * rs;
  for (int32_t c0 = 0; c0 < d; c0 += 64) {
    const int32_t col = c0 + lane;
    bool p = false;
    if (col < d) {
      const int32_t bits = __float_as_int(xr[col]);
      p = bits > 0 && bits <= 0x7F800000;
    }
    const unsigned long long m = __ballot(p);
    if (out_bytes) {
      if (lane < 8 && c0 + 8 * lane < d) out_bytes[r * out_rs + (c0 >> 3) + lane] = (uint8_t)(m >> (8 * lane));
    } else if (lane < 2) {
      const int32_t w = (c0 >> 5) + lane;
      const int64_t row = row0 + r;
      if (w < W32) codes[((row >> 6) * W32 + w) * 64 + (row & 63)] = (uint32_t)(m >> (32 * lane));
    }
  }
}

// ---- launchers
int32_t hamming_query_words(int32_t W32) {
  for (int32_t nw : {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128})
    if (nw >= W32) return nw;
  return 0;
}

void launch_hamming_ingest(const uint8_t* src, int64_t stride, int32_t nbits, int64_t row0, int64_t m, uint32_t* codes,
                           hipStream_t stream) {
  const int32_t nb = nbits / 8, W32 = (nbits + 31) / 32;
  constexpr int64_t STEP = (int64_t)1 << 22;                // rows per launch: the grid stays far below 2^31
  for (int64_t r = 0; r < m; r += STEP) {
    const int64_t mm = std::min(STEP, m - r);
    hamming_ingest_kernel<<<dim3((unsigned)((mm * W32 + 255) / 256)), 256, 0, stream>>>(src + r * stride, stride, nb, W32, row0 + r,
                                                                                       mm, codes);
  }
}

void launch_hamming_query_words(const uint8_t* src, int64_t stride, int32_t nbits, int64_t nq, uint32_t* out, hipStream_t stream) {
  const int32_t nb = nbits / 8, wq = hamming_query_words((nbits + 31) / 32);
  constexpr int64_t STEP = (int64_t)1 << 22;
  for (int64_t q = 0; q < nq; q += STEP) {
    const int64_t mm = std::min(STEP, nq - q);
    hamming_query_words_kernel<<<dim3((unsigned)((mm * wq + 255) / 256)), 256, 0, stream>>>(src + q * stride, stride, nb, wq, mm,
                                                                                            out + q * wq);
  }
}

template <int NW>
static void dist_launch(dim3 grid, hipStream_t s, const uint32_t* codes, int32_t W32, int64_t nblk, int64_t n, const uint32_t* qw,
                        int32_t nq, int32_t qper, const uint64_t* allow, uint16_t* dist, int64_t npad) {
  hamming_dist_kernel<NW><<<grid, 256, 0, s>>>(codes, W32, nblk, n, qw, nq, qper, allow, dist, npad);
}

void launch_hamming_dist(const uint32_t* codes, int32_t nbits, int64_t n, const uint32_t* qw, int32_t nq, const uint64_t* allow,
                         uint16_t* dist, hipStream_t stream) {
  const int32_t W32 = (nbits + 31) / 32, nw = hamming_query_words(W32);
  const int64_t nblk = (n + 63) / 64, npad = nblk * 64;
  if (nblk == 0 || nq <= 0) return;
  // enough waves to fill the device (256 CUs x 16): the queries of a batch are split over blockIdx.y only when the rows alone
  // do not give that many; a wave keeps its 64 rows in registers for all of its queries
  const int64_t want = 4096;
  int64_t split = std::min<int64_t>({(want + nblk - 1) / nblk, (int64_t)nq, 65535});
  const int32_t qper = (int32_t)((nq + split - 1) / split);
  split = (nq + qper - 1) / qper;
  const dim3 grid((unsigned)((nblk + 3) / 4), (unsigned)split);
  switch (nw) {
    case 1: dist_launch<1>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    case 2: dist_launch<2>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    case 3: dist_launch<3>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    case 4: dist_launch<4>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    case 6: dist_launch<6>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    case 8: dist_launch<8>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    case 12: dist_launch<12>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    case 16: dist_launch<16>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    case 24: dist_launch<24>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    case 32: dist_launch<32>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    case 48: dist_launch<48>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    case 64: dist_launch<64>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    case 96: dist_launch<96>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
    default: dist_launch<128>(grid, stream, codes, W32, nblk, n, qw, nq, qper, allow, dist, npad); break;
  }
}

void launch_hamming_select(const uint16_t* dist, int64_t n, int32_t nbits, int32_t nq, int32_t k, int64_t row_offset,
                           int64_t* out_idx, int32_t* out_dist, hipStream_t stream) {
  if (nq <= 0) return;
  const int64_t npad = (n + 63) / 64 * 64;
  hamming_select_kernel<<<dim3((unsigned)nq), HS_THREADS, 0, stream>>>(dist, npad, nbits, k, row_offset, out_idx, out_dist);
}

void launch_hamming_sign(const float* x, int64_t n, int32_t d, int64_t rs, uint8_t* out_bytes, int64_t out_rs, uint32_t* codes,
                         int64_t row0, hipStream_t stream) {
  if (n <= 0) return;
  hamming_sign_kernel<<<dim3((unsigned)((n + 3) / 4)), 256, 0, stream>>>(x, n, d, rs, out_bytes, out_rs, codes, (d + 31) / 32, row0);
}

}  // namespace mi
