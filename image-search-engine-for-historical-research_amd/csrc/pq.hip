// Exact ADC top-K on product-quantized codes (api_pq.hip): the reference's matching_PQ_Net
// (src/utils/nnsearch.py:905-946), nanopq's dtable(query).adist(codes), faiss IndexPQ.search.
//
// M books of Ks <= 256 codewords of L floats (codebooks [M][Ks][L] f32), a code is M bytes.  Gallery layout: blocks of 64 rows,
// four books to a dword, dwords transposed: codes[block][w][lane], w < MQ = ceil(M / 4), byte (m & 3) of dword (m >> 2) is the
// row's code in book m; the bytes of the books M .. 4 MQ - 1 are zero.  Lane l of a wave owns row 64 * block + l, one book-quad
// of the 64 rows is one coalesced 256-byte read.
//
//   pq_device.h       the pieces shared with ivfpq.hip and ivfpq_residual.hip.  pq_sqdist is THE arithmetic: sum_j (double(x_j) -
//                     double(c_j))^2 in float64, ascending j, a separate multiply and add per term (no contraction).  The table
//                     rounds it once to float32, the encoder takes its argmin; pq_adc_row is the scan's row sum
//   pq_check_kernel, pq_ingest_kernel, pq_decode_kernel
//                     the element-wise kernels, templates on the code type like the encoder: device codes >= ks raise the flag;
//                     codes [rows][stride] -> dwords of the transposed layout (pq_pack_dword); rows reconstructed from their codes.
//                     One copy serves this index (bytes, four books to a dword) and the wide one (uint16, two; pq_wide.hip)
//   pq_table_kernel   T[q][m][c] = (float)pq_sqdist(x[q][m L ..], C[m][c]), thread = (q, m, c)
//   pq_encode_kernel  code[i][m] = argmin_c pq_sqdist(x[i][m L ..], C[m][c]), ties to the lower c.  A workgroup takes 64 rows of
//                     one book; row and codeword slices pass through LDS as float64, 8 accumulators per thread.  The code type
//                     is a template argument: bytes here, uint16 for the wide index (pq_wide.hip), any Ks
//   pq_scan_kernel    the hot path: a workgroup loads the tables of a tile of QT queries into LDS interleaved query-fastest,
//                     T[m][c][QT], and walks a slab of row blocks; per (row, book) ONE LDS read of 4 QT bytes at the
//                     data-dependent address (m Ks + code) returns the entry of every query of the tile.  dist = T[0][code_0] +
//                     T[1][code_1] + ... in float32, ascending book order.  The NEGATED distance goes to a matrix
//                     [queries][npad]; rows not admitted (beyond n, or cleared in the allow bitmap) get NaN, which
//                     launch_dense_topk (dense.hip) orders below every number, -inf included
//   pq_emit_kernel    its (-distance desc, id asc) lists -> (distance asc, id asc) outputs, -1 / +inf where the list ran out of
//                     admitted rows
#include <algorithm>

#include "kernels.h"
#include "pq_device.h"

namespace mi {

// ---- codes >= ks raise the flag (device-resident codes; host codes are checked on the host)
template <typename CodeT>
__global__ __launch_bounds__(256) void pq_check_kernel(const CodeT* __restrict__ src, int64_t stride, int32_t M, int32_t ks, int64_t m,
                                                      uint32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m * M) return;
  const int64_t r = i / M;
  const int32_t b = (int32_t)(i % M);
  if ((int32_t)src[r * stride + b] >= ks) *flag = 1u;
}

// ---- codes [m][stride] -> dwords of rows row0 .. row0 + m of the transposed layout (thread = (dword, row), rows fastest)
template <typename CodeT>
__global__ __launch_bounds__(256) void pq_ingest_kernel(const CodeT* __restrict__ src, int64_t stride, int32_t M, int32_t MW, int64_t row0,
                                                       int64_t m, uint32_t* __restrict__ codes) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m * MW) return;
  const int64_t r = i % m;
  const int32_t w = (int32_t)(i / m);
  const int64_t row = row0 + r;
  codes[((row >> 6) * MW + w) * 64 + (row & 63)] = pq_pack_dword(src + r * stride, w, M);
}

// ---- out [nrows][M L]: row row0 + r reconstructed, the concatenation of C[j][code[j]] (nanopq's pq.decode); thread = one element
template <typename CodeT>
__global__ __launch_bounds__(256) void pq_decode_kernel(const uint32_t* __restrict__ codes, int32_t M, int32_t Ks, int32_t L,
                                                       const float* __restrict__ cb, int64_t row0, int64_t nrows,
                                                       float* __restrict__ out) {
  constexpr uint32_t PER = pq_codes_per_dword<CodeT>(), BITS = 8 * sizeof(CodeT);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int32_t d = M * L, MW = pq_code_dwords<CodeT>(M);
  if (i >= nrows * d) return;
  const int64_t row = row0 + i / d;
  const int32_t col = (int32_t)(i % d), j = col / L;
  const uint32_t g = codes[((row >> 6) * MW + (uint32_t)j / PER) * 64 + (row & 63)];
  const int32_t c = (int32_t)((g >> (BITS * ((uint32_t)j % PER))) & ((1u << BITS) - 1u));
  out[i] = cb[((int64_t)j * Ks + c) * L + (col - j * L)];
}

// ---- table
template <typename InT>
__global__ __launch_bounds__(256) void pq_table_kernel(const InT* __restrict__ x, int64_t rs, int64_t cs, int64_t nq,
                                                      const float* __restrict__ cb, int32_t M, int32_t Ks, int32_t L,
                                                      float* __restrict__ tab) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq * M * Ks) return;
  const int32_t c = (int32_t)(i % Ks);
  const int32_t m = (int32_t)((i / Ks) % M);
  const int64_t q = i / ((int64_t)Ks * M);
  const InT* xr = x + q * rs + (int64_t)m * L * cs;
  const float* cw = cb + ((int64_t)m * Ks + c) * L;
  tab[i] = (float)pq_sqdist([&](int32_t j) { return (double)xr[(int64_t)j * cs]; }, [&](int32_t j) { return (double)cw[j]; }, L);
}

// ---- encoder.  Workgroup = 64 rows x one book; thread t: row t & 63, codeword group t >> 6 (one wave each).  The codewords
// pass in tiles of PE_CT = 32 (8 per thread), the columns in slices of PE_JT = 64; xs[j][row] and cs[c][j] are float64 in LDS
// (xs: consecutive lanes, consecutive addresses; cs: one address per wave, a broadcast).  The tile constants PE_* are pq_device.h's: ivfr_encode_kernel
// (ivfpq_residual.hip) is this kernel on residuals and keeps the same tiling.
template <typename InT, typename CodeT>
__global__ __launch_bounds__(256) void pq_encode_kernel(const InT* __restrict__ x, int64_t rs, int64_t cs, int64_t n,
                                                       const float* __restrict__ cb, int32_t M, int32_t Ks, int32_t L,
                                                       CodeT* __restrict__ out) {
  __shared__ double xs[PE_JT][PE_ROWS];
  __shared__ double cw[PE_CT][PE_JT + 1];
  __shared__ double bd[4][PE_ROWS];
  __shared__ int32_t bc[4][PE_ROWS];
  const int tid = threadIdx.x, r = tid & 63, cg = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * PE_ROWS;
  const int32_t m = (int32_t)blockIdx.y;
  double best = __builtin_inf();
  int32_t best_c = 0;
  for (int32_t c0 = 0; c0 < Ks; c0 += PE_CT) {
    double acc[PE_PER];
#pragma unroll
    for (int e = 0; e < PE_PER; ++e) acc[e] = 0.0;
    for (int32_t j0 = 0; j0 < L; j0 += PE_JT) {
      const int32_t jn = min(PE_JT, L - j0);
      __syncthreads();
      for (int i = tid; i < PE_ROWS * PE_JT; i += 256) {          // consecutive threads, consecutive columns of one row
        const int j = i % PE_JT, rr = i / PE_JT;
        const int64_t row = row0 + rr;
        xs[j][rr] = (j < jn && row < n) ? (double)x[row * rs + ((int64_t)m * L + j0 + j) * cs] : 0.0;
      }
      for (int i = tid; i < PE_CT * PE_JT; i += 256) {
        const int j = i % PE_JT, cc = i / PE_JT;
        cw[cc][j] = (j < jn && c0 + cc < Ks) ? (double)cb[((int64_t)m * Ks + c0 + cc) * L + j0 + j] : 0.0;
      }
      __syncthreads();
      for (int32_t j = 0; j < jn; ++j) {
        const double xv = xs[j][r];
#pragma unroll
        for (int e = 0; e < PE_PER; ++e) acc[e] = pq_sqdist_step(acc[e], xv, cw[cg * PE_PER + e][j]);
      }
    }
#pragma unroll
    for (int e = 0; e < PE_PER; ++e) {
      const int32_t c = c0 + cg * PE_PER + e;
      if (c < Ks && acc[e] < best) {                              // ascending c, strict: ties stay with the lower c
        best = acc[e];
        best_c = c;
      }
    }
  }
  bd[cg][r] = best;
  bc[cg][r] = best_c;
  __syncthreads();
  if (tid < PE_ROWS && row0 + tid < n) {
    double b = bd[0][tid];
    int32_t c = bc[0][tid];
#pragma unroll
    for (int g = 1; g < 4; ++g) {
      const double v = bd[g][tid];
      const int32_t vc = bc[g][tid];
      if (v < b || (v == b && vc < c)) {
        b = v;
        c = vc;
      }
    }
    out[(row0 + tid) * M + m] = (CodeT)c;
  }
}

// ---- scan
constexpr int PS_THREADS = 512, PS_WAVES = PS_THREADS / 64;
constexpr int PS_LDS_BUDGET = 128 * 1024;

// grid = (query tiles, slabs).  tab: [nq][M][Ks] f32.  The LDS image holds 4 MQ books, zero entries for the books beyond M
// (pq_adc_row, pq_device.h).
template <int QT>
__global__ __launch_bounds__(PS_THREADS) void pq_scan_kernel(const uint32_t* __restrict__ codes, int32_t M, int32_t MQ, int32_t Ks,
                                                            int64_t nblk, int64_t blk_per, int64_t n, const float* __restrict__ tab,
                                                            int32_t nq, const uint64_t* __restrict__ allow, float* __restrict__ mat,
                                                            int64_t npad) {
  extern __shared__ __attribute__((aligned(16))) char pq_smem[];
  using Vec = typename PqVec<QT>::type;
  float* tl = reinterpret_cast<float*>(pq_smem);
  const int32_t q0 = (int32_t)blockIdx.x * QT;
  const int32_t ent = 4 * MQ * Ks, real = M * Ks;
  for (int32_t i = threadIdx.x; i < ent * QT; i += PS_THREADS) {     // consecutive threads, consecutive entries of one query
    const int32_t t = i / ent, e = i - t * ent;
    tl[e * QT + t] = (e < real && q0 + t < nq) ? tab[((int64_t)(q0 + t) * M) * Ks + e] : 0.0f;
  }
  __syncthreads();
  const Vec* tv = reinterpret_cast<const Vec*>(pq_smem);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b0 = (int64_t)blockIdx.y * blk_per, b1 = min(nblk, b0 + blk_per);
  for (int64_t b = b0 + wave; b < b1; b += PS_WAVES) {               // wave-uniform
    const PqSums<QT> acc = pq_adc_row<QT>(tv, codes + b * MQ * 64 + lane, MQ, Ks);
    const int64_t row = b * 64 + lane;
    bool ok = row < n;
    if (allow) ok = ok && ((allow[b] >> lane) & 1ull);
#pragma unroll
    for (int t = 0; t < QT; ++t)
      if (q0 + t < nq) mat[(int64_t)(q0 + t) * npad + row] = ok ? -acc.v[t] : __builtin_nanf("");
  }
}

// ---- emit: lists of launch_dense_topk over the negated matrix -> the caller's outputs
__global__ __launch_bounds__(256) void pq_emit_kernel(const int64_t* __restrict__ tidx, const float* __restrict__ tneg, int64_t nq,
                                                     int32_t ke, int32_t k, int64_t row_offset, int64_t* __restrict__ out_idx,
                                                     float* __restrict__ out_dist) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq * k) return;
  const int64_t q = i / k;
  const int32_t j = (int32_t)(i % k);
  int64_t id = -1;
  float dist = __builtin_inff();
  if (j < ke) {
    const float s = tneg[q * ke + j];
    if (s == s) {
      id = row_offset + tidx[q * ke + j];
      dist = -s;
    }
  }
  out_idx[i] = id;
  if (out_dist) out_dist[i] = dist;
}

// ---- launchers
constexpr int64_t PQ_STEP = (int64_t)1 << 22;                 // rows per launch of the element-wise kernels: grids stay below 2^31

template <typename CodeT>
static void check_launch(const CodeT* src, int64_t stride, int32_t M, int32_t ks, int64_t m, uint32_t* flag, hipStream_t stream) {
  for (int64_t r = 0; r < m; r += PQ_STEP) {
    const int64_t mm = std::min(PQ_STEP, m - r);
    pq_check_kernel<CodeT><<<dim3((unsigned)((mm * M + 255) / 256)), 256, 0, stream>>>(src + r * stride, stride, M, ks, mm, flag);
  }
}

void launch_pq_check(const uint8_t* src, int64_t stride, int32_t M, int32_t ks, int64_t m, uint32_t* flag, hipStream_t stream) {
  check_launch(src, stride, M, ks, m, flag, stream);
}

void launch_pq_check(const uint16_t* src, int64_t stride, int32_t M, int32_t ks, int64_t m, uint32_t* flag, hipStream_t stream) {
  check_launch(src, stride, M, ks, m, flag, stream);
}

template <typename CodeT>
static void ingest_launch(const CodeT* src, int64_t stride, int32_t M, int64_t row0, int64_t m, uint32_t* codes, hipStream_t stream) {
  const int32_t MW = pq_code_dwords<CodeT>(M);
  for (int64_t r = 0; r < m; r += PQ_STEP) {
    const int64_t mm = std::min(PQ_STEP, m - r);
    pq_ingest_kernel<CodeT><<<dim3((unsigned)((mm * MW + 255) / 256)), 256, 0, stream>>>(src + r * stride, stride, M, MW, row0 + r, mm, codes);
  }
}

void launch_pq_ingest(const uint8_t* src, int64_t stride, int32_t M, int64_t row0, int64_t m, uint32_t* codes, hipStream_t stream) {
  ingest_launch(src, stride, M, row0, m, codes, stream);
}

void launch_pq_ingest(const uint16_t* src, int64_t stride, int32_t M, int64_t row0, int64_t m, uint32_t* codes, hipStream_t stream) {
  ingest_launch(src, stride, M, row0, m, codes, stream);
}

void launch_pq_decode(const uint32_t* codes, int32_t code_bytes, int32_t M, int32_t Ks, int32_t L, const float* cb, int64_t row0,
                      int64_t nrows, float* out, hipStream_t stream) {
  const int64_t d = (int64_t)M * L;
  const int64_t step = std::max<int64_t>(1, ((int64_t)1 << 30) / d);         // rows per launch
  for (int64_t r = 0; r < nrows; r += step) {
    const int64_t b = std::min(step, nrows - r);
    const dim3 grid((unsigned)((b * d + 255) / 256));
    if (code_bytes == 1) pq_decode_kernel<uint8_t><<<grid, 256, 0, stream>>>(codes, M, Ks, L, cb, row0 + r, b, out + r * d);
    else pq_decode_kernel<uint16_t><<<grid, 256, 0, stream>>>(codes, M, Ks, L, cb, row0 + r, b, out + r * d);
  }
}

void launch_pq_table(const void* x, int dtype, int64_t rs, int64_t cs, int64_t nq, const float* cb, int32_t M, int32_t Ks, int32_t L,
                     float* tab, hipStream_t stream) {
  const int64_t per = (int64_t)M * Ks;
  const int64_t step = std::max<int64_t>(1, ((int64_t)1 << 30) / per);       // queries per launch
  for (int64_t q = 0; q < nq; q += step) {
    const int64_t b = std::min(step, nq - q);
    const dim3 grid((unsigned)((b * per + 255) / 256));
    if (dtype == 0)
      pq_table_kernel<float><<<grid, 256, 0, stream>>>((const float*)x + q * rs, rs, cs, b, cb, M, Ks, L, tab + q * per);
    else
      pq_table_kernel<double><<<grid, 256, 0, stream>>>((const double*)x + q * rs, rs, cs, b, cb, M, Ks, L, tab + q * per);
  }
}

template <typename CodeT>
static void encode_launch(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const float* cb, int32_t M, int32_t Ks, int32_t L,
                          CodeT* out, hipStream_t stream) {
  for (int64_t r = 0; r < n; r += PQ_STEP) {
    const int64_t mm = std::min(PQ_STEP, n - r);
    const dim3 grid((unsigned)((mm + PE_ROWS - 1) / PE_ROWS), (unsigned)M);
    if (dtype == 0)
      pq_encode_kernel<float, CodeT><<<grid, 256, 0, stream>>>((const float*)x + r * rs, rs, cs, mm, cb, M, Ks, L, out + r * M);
    else
      pq_encode_kernel<double, CodeT><<<grid, 256, 0, stream>>>((const double*)x + r * rs, rs, cs, mm, cb, M, Ks, L, out + r * M);
  }
}

void launch_pq_encode(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const float* cb, int32_t M, int32_t Ks, int32_t L,
                      uint8_t* out, hipStream_t stream) {
  encode_launch(x, dtype, rs, cs, n, cb, M, Ks, L, out, stream);
}

void launch_pq_encode(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const float* cb, int32_t M, int32_t Ks, int32_t L,
                      uint16_t* out, hipStream_t stream) {
  encode_launch(x, dtype, rs, cs, n, cb, M, Ks, L, out, stream);
}

int32_t pq_query_tile(int32_t M, int32_t Ks, int64_t nq) {
  const int64_t one = (int64_t)4 * ((M + 3) / 4) * Ks * 4;    // bytes of one query's LDS image
  if (nq >= 3 && 4 * one <= PS_LDS_BUDGET) return 4;
  if (nq >= 2 && 2 * one <= PS_LDS_BUDGET) return 2;
  return 1;
}

template <int QT>
static void scan_launch(hipStream_t s, const uint32_t* codes, int32_t M, int32_t Ks, int64_t n, const float* tab, int32_t nq,
                        const uint64_t* allow, float* mat) {
  const int32_t MQ = (M + 3) / 4;
  const int64_t nblk = (n + 63) / 64, npad = nblk * 64;
  const int lds = 4 * MQ * Ks * 4 * QT;
  ensure_dynamic_lds((const void*)pq_scan_kernel<QT>);
  // slabs: enough workgroups to fill the device (256 CUs, one or two workgroups each), but no slab below PS_WAVES blocks
  const int64_t tiles = (nq + QT - 1) / QT;
  int64_t slabs = std::min<int64_t>({(1024 + tiles - 1) / tiles, (nblk + PS_WAVES - 1) / PS_WAVES, 65535});
  slabs = std::max<int64_t>(slabs, 1);
  const int64_t blk_per = (nblk + slabs - 1) / slabs;
  slabs = (nblk + blk_per - 1) / blk_per;
  pq_scan_kernel<QT><<<dim3((unsigned)tiles, (unsigned)slabs), PS_THREADS, lds, s>>>(codes, M, MQ, Ks, nblk, blk_per, n, tab, nq, allow,
                                                                                    mat, npad);
}

void launch_pq_scan(const uint32_t* codes, int32_t M, int32_t Ks, int64_t n, const float* tab, int32_t nq, int32_t qt,
                    const uint64_t* allow, float* mat, hipStream_t stream) {
  if (n <= 0 || nq <= 0) return;
  switch (qt) {
    case 4: scan_launch<4>(stream, codes, M, Ks, n, tab, nq, allow, mat); break;
    case 2: scan_launch<2>(stream, codes, M, Ks, n, tab, nq, allow, mat); break;
    default: scan_launch<1>(stream, codes, M, Ks, n, tab, nq, allow, mat); break;
  }
}

void launch_pq_emit(const int64_t* tidx, const float* tneg, int64_t nq, int32_t ke, int32_t k, int64_t row_offset, int64_t* out_idx,
                    float* out_dist, hipStream_t stream) {
  if (nq <= 0) return;
  pq_emit_kernel<<<dim3((unsigned)((nq * k + 255) / 256)), 256, 0, stream>>>(tidx, tneg, nq, ke, k, row_offset, out_idx, out_dist);
}

}  // namespace mi
