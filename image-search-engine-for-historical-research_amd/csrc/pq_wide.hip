// Exact ADC top-K on WIDE product-quantized codes (api_pq_wide.hip): the reference's matching_Nano_PQ as its entry
// points call it, N_books = 16, n_bits_perbook = 13 (src/offline.py:110), 8192 codewords per book.
//
// M books of Ks <= 8192 codewords of L floats (codebooks [M][Ks][L] f32), a code is M uint16.  Gallery layout: blocks of 64 rows, two
// books to a dword, dwords transposed: codes[block][w][lane], w < MH = ceil(M / 2), the low half of dword w is the row's code in
// book 2 w, the high half in book 2 w + 1 (zero when that book is beyond M).  Lane l of a wave owns row 64 * block + l, one book
// pair of the 64 rows is one coalesced 256-byte read.  Tables, arithmetic, matrix, selection and emit are the byte index's
// (launch_pq_table, pq_acc, launch_dense_topk, launch_pq_emit), and check, ingest, encoder and decode are pq.hip's kernels with a
// uint16 code type: for Ks <= 256 every output has the bits of mi_pq's.  What is left here is the one kernel that differs:
//
//   pqw_scan_kernel    the hot path.  One query's tables are M Ks 4 bytes (512 KiB at 16 x 8192) and do not fit in LDS, so the books
//                      pass in GROUPS of GP book pairs: a workgroup owns a slab of at most PW_WAVES * PW_RPL row blocks and a tile
//                      of QT queries; per group it loads 2 GP Ks QT entries into LDS (interleaved query-fastest, T[book][c][QT], +0.0
//                      for a book beyond M), then every wave walks the group's dwords of its row blocks.  A lane owns up to PW_RPL
//                      rows (one per block of its wave) and carries their float32 partial sums in registers from group to group:
//                      the adds of a row happen in ascending book order whatever GP is, so the bits do not depend on it.  When
//                      all MH pairs fit (GP = MH) the kernel is one pass.  Output as pq_scan_kernel's: the NEGATED distance into
//                      the matrix [queries][npad], NaN for rows not admitted
#include <algorithm>

#include "kernels.h"
#include "pq_device.h"

namespace mi {

// ---- scan
constexpr int PW_THREADS = 1024, PW_WAVES = PW_THREADS / 64;
constexpr int PW_RPL = 16;                                    // rows per lane: a slab is at most PW_WAVES * PW_RPL = 256 blocks
constexpr int PW_LDS_BUDGET = 128 * 1024;

// grid = tiles * slabs, slab fastest: the workgroups that read one tile's tables run together.  tab: [nq][M][Ks] f32
template <int QT>
__global__ __launch_bounds__(PW_THREADS) void pqw_scan_kernel(const uint32_t* __restrict__ codes, int32_t M, int32_t MH, int32_t Ks,
                                                             int32_t GP, int64_t nblk, int64_t blk_per, int64_t slabs, int64_t n,
                                                             const float* __restrict__ tab, int32_t nq,
                                                             const uint64_t* __restrict__ allow, float* __restrict__ mat,
                                                             int64_t npad) {
  extern __shared__ __attribute__((aligned(16))) char pqw_smem[];
  using Vec = typename PqVec<QT>::type;
  float* tl = reinterpret_cast<float*>(pqw_smem);
  const Vec* tv = reinterpret_cast<const Vec*>(pqw_smem);
  const int64_t tile = (int64_t)blockIdx.x / slabs, slab = (int64_t)blockIdx.x - tile * slabs;
  const int32_t q0 = (int32_t)tile * QT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b0 = slab * blk_per, b1 = min(nblk, b0 + blk_per);
  float acc[PW_RPL][QT];
#pragma unroll
  for (int i = 0; i < PW_RPL; ++i)
#pragma unroll
    for (int t = 0; t < QT; ++t) acc[i][t] = 0.0f;

  for (int32_t w0 = 0; w0 < MH; w0 += GP) {                           // workgroup-uniform
    const int32_t wn = min(GP, MH - w0);
    const int32_t ent = 2 * wn * Ks, real = (min(M, 2 * (w0 + wn)) - 2 * w0) * Ks;
    if (w0) __syncthreads();                                          // the image is rewritten
    if ((Ks & 3) == 0) {                                              // 16-byte reads: M Ks and 2 w0 Ks are multiples of 4 floats
      const int32_t ent4 = ent >> 2;
      for (int32_t i = threadIdx.x; i < ent4 * QT; i += PW_THREADS) {
        const int32_t t = i / ent4, e = (i - t * ent4) << 2;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (e < real && q0 + t < nq) v = *reinterpret_cast<const float4*>(tab + ((int64_t)(q0 + t) * M + 2 * w0) * Ks + e);
        tl[e * QT + t] = v.x;
        tl[(e + 1) * QT + t] = v.y;
        tl[(e + 2) * QT + t] = v.z;
        tl[(e + 3) * QT + t] = v.w;
      }
    } else {
      for (int32_t i = threadIdx.x; i < ent * QT; i += PW_THREADS) {
        const int32_t t = i / ent, e = i - t * ent;
        tl[e * QT + t] = (e < real && q0 + t < nq) ? tab[((int64_t)(q0 + t) * M + 2 * w0) * Ks + e] : 0.0f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PW_RPL; ++i) {
      const int64_t b = b0 + wave + (int64_t)i * PW_WAVES;
      if (b < b1) {                                                   // wave-uniform
        const uint32_t* src = codes + (b * MH + w0) * 64 + lane;
#pragma unroll 2
        for (int32_t w = 0; w < wn; ++w) {
          const uint32_t g = src[(int64_t)w * 64];
          pq_acc<QT>(acc[i], tv[2 * w * Ks + (int32_t)(g & 0xffffu)]);
          pq_acc<QT>(acc[i], tv[(2 * w + 1) * Ks + (int32_t)(g >> 16)]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < PW_RPL; ++i) {
    const int64_t b = b0 + wave + (int64_t)i * PW_WAVES;
    if (b < b1) {
      const int64_t row = b * 64 + lane;
      bool ok = row < n;
      if (allow) ok = ok && ((allow[b] >> lane) & 1ull);
#pragma unroll
      for (int t = 0; t < QT; ++t)
        if (q0 + t < nq) mat[(int64_t)(q0 + t) * npad + row] = ok ? -acc[i][t] : __builtin_nanf("");
    }
  }
}

// ---- launchers
// one book pair of one query is 2 Ks 4 bytes: 64 KiB at Ks = 8192, so QT <= 2 there
int32_t pqw_query_tile(int32_t Ks, int64_t nq) {
  const int64_t pair = (int64_t)2 * Ks * 4;
  if (nq >= 3 && 4 * pair <= PW_LDS_BUDGET) return 4;
  if (nq >= 2 && 2 * pair <= PW_LDS_BUDGET) return 2;
  return 1;
}

template <int QT>
static void wide_scan_launch(hipStream_t s, const uint32_t* codes, int32_t M, int32_t Ks, int64_t n, const float* tab, int32_t nq,
                             const uint64_t* allow, float* mat) {
  const int32_t MH = (M + 1) / 2;
  const int64_t nblk = (n + 63) / 64, npad = nblk * 64;
  const int64_t pair = (int64_t)2 * Ks * 4 * QT;                      // LDS bytes of one book pair of the tile
  const int32_t GP = (int32_t)std::min<int64_t>(MH, PW_LDS_BUDGET / pair);
  const int lds = (int)(GP * pair);
  ensure_dynamic_lds((const void*)pqw_scan_kernel<QT>);
  // slabs: two workgroups per CU where the rows allow it, no slab above PW_WAVES * PW_RPL blocks (a lane's registers) and none
  // below PW_WAVES (a block per wave).  A larger slab pays a group's table load over more rows
  const int64_t tiles = (nq + QT - 1) / QT;
  const int64_t cap = (int64_t)PW_WAVES * PW_RPL;
  int64_t slabs = std::min<int64_t>((512 + tiles - 1) / tiles, (nblk + PW_WAVES - 1) / PW_WAVES);
  slabs = std::max<int64_t>({slabs, (nblk + cap - 1) / cap, 1});
  const int64_t blk_per = (nblk + slabs - 1) / slabs;
  slabs = (nblk + blk_per - 1) / blk_per;
  pqw_scan_kernel<QT><<<dim3((unsigned)(tiles * slabs)), PW_THREADS, lds, s>>>(codes, M, MH, Ks, GP, nblk, blk_per, slabs, n, tab, nq,
                                                                             allow, mat, npad);
}

void launch_pqw_scan(const uint32_t* codes, int32_t M, int32_t Ks, int64_t n, const float* tab, int32_t nq, int32_t qt,
                     const uint64_t* allow, float* mat, hipStream_t stream) {
  if (n <= 0 || nq <= 0) return;
  switch (qt) {
    case 4: wide_scan_launch<4>(stream, codes, M, Ks, n, tab, nq, allow, mat); break;
    case 2: wide_scan_launch<2>(stream, codes, M, Ks, n, tab, nq, allow, mat); break;
    default: wide_scan_launch<1>(stream, codes, M, Ks, n, tab, nq, allow, mat); break;
  }
}

}  // namespace mi
