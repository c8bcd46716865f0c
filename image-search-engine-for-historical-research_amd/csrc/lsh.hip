// LSH codes (api_lsh.hip): the first half of faiss IndexLSH (src/utils/nnsearch.py:734-745) -- project every
// descriptor onto nbits directions and keep one bit per direction,
//   bit j of row i = ( sum_k double(x[i][k]) * R[j][k]  >=  t[j] )        (fvecs2bitvecs' rule; a NaN sum gives 0, -0.0 >= 0 gives 1)
// packed like every binary code here: bit j is bit (j & 7) of byte (j >> 3).  The second half is the Hamming search of hamming.hip.
//
// The projection is the f64 GEMM of whiten.hip (2 * nbits * d flop per row) without the centring, on the 128 x 128 tile of
// f64_tile.h (geometry, K chunks through LDS, XCD-aware tile order); X is promoted to double on load.
// What differs is the epilogue: the 128 x 128 float64 products never leave the registers.  Each accumulator register is compared
// with its column's threshold and balloted; the C layout of the f64 MFMA (column = lane & 15, row = (lane >> 4) + 4 * register)
// puts the 16 outcomes of one row and one 16-column block into 16 consecutive ballot bits, so four ballots give four rows of 64
// bits.  Lane l of a wave collects the 64 bits of the wave's row l and stores them: 8 bytes per row and wave, 1 / 64 of the
// bytes of the float64 tile.  No atomics, no workspace, no cross-workgroup dependency.
#include "common.h"
#include "f64_tile.h"
#include "kernels.h"

namespace mi {

// ROWS: the K index is the contiguous one of X (cs == 1): a wave reads 4 rows x 16 consecutive k per instruction; otherwise
// (the reference's [D, N] layout, rs == 1, and any other strides) 64 consecutive rows of one k.
// out != NULL: rows of nbits / 8 bytes at out_rs (bytes beyond nbits / 8 are not touched); else the 32-bit words of rows
// dst_row0 .. dst_row0 + n of the transposed gallery layout of hamming.hip, codes[row >> 6][w < W32][row & 63], pad bits zero.
template <typename InT, bool ROWS>
__global__ __launch_bounds__(256, 2) void lsh_encode_kernel(const InT* __restrict__ X, int64_t n, int32_t d, int64_t rs, int64_t cs,
                                                            const double* __restrict__ R /*[nbits][d]*/,
                                                            const double* __restrict__ thr /*[nbits] or NULL*/, int32_t nbits,
                                                            uint8_t* __restrict__ out, int64_t out_rs, uint32_t* __restrict__ codes,
                                                            int32_t W32, int64_t dst_row0, uint32_t ncb, uint32_t nrb) {
  extern __shared__ __attribute__((aligned(16))) double l_lds[];
  double* const Xs0 = l_lds;
  double* const Ps0 = l_lds + 2 * F64T_BUF;
  uint32_t cb, rt;
  f64t_tile_order(blockIdx.x, ncb, nrb, &cb, &rt);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1, l15 = lane & 15, lq = lane >> 4;
  const int64_t row0 = (int64_t)rt * F64T_TILE;
  const int32_t col0 = (int32_t)cb * F64T_TILE;
  // element i of this thread in an operand chunk: X (r, kk) = (xr0 + 16 i, xk0) (ROWS) or (xr0 + 64 (i & 1), xk0 + 4 (i >> 1));
  // R (pj0 + 16 i, pk)
  const int xr0 = ROWS ? t / F64T_KC : t % 64, xk0 = ROWS ? t % F64T_KC : t / 64;
  auto x_r = [&](int i) { return ROWS ? xr0 + F64T_RSTEP * i : xr0 + 64 * (i & 1); };
  auto x_k = [&](int i) { return ROWS ? xk0 : xk0 + 4 * (i >> 1); };
  const int pj0 = t / F64T_KC, pk = t % F64T_KC;
  const bool interior = row0 + F64T_TILE <= n && col0 + F64T_TILE <= nbits;
  const InT* xp0 = X + (row0 + xr0) * rs + (int64_t)xk0 * cs;
  const double* pp0 = R + (int64_t)(col0 + pj0) * d + pk;

  InT xr[F64T_PER];
  double pr[F64T_PER];
  bool fast = false;                                        // the chunk in the registers lies inside X and R: no masking
  auto load_chunk = [&](int32_t k0) {
    fast = interior && k0 + F64T_KC <= d;
    if (fast) {
      const InT* xp = xp0 + (int64_t)k0 * cs;
      const double* pp = pp0 + k0;
#pragma unroll
      for (int i = 0; i < F64T_PER; ++i) {
        xr[i] = ROWS ? xp[(int64_t)F64T_RSTEP * i * rs] : xp[(int64_t)(64 * (i & 1)) * rs + (int64_t)(4 * (i >> 1)) * cs];
        pr[i] = pp[(int64_t)F64T_RSTEP * i * d];
      }
    } else {
#pragma unroll
      for (int i = 0; i < F64T_PER; ++i) {
        const int64_t row = row0 + x_r(i);
        const int32_t k = k0 + x_k(i);
        xr[i] = (row < n && k < d) ? X[row * rs + (int64_t)k * cs] : (InT)0;
        const int32_t pj = col0 + pj0 + F64T_RSTEP * i;
        pr[i] = (pj < nbits && k0 + pk < d) ? R[(int64_t)pj * d + k0 + pk] : 0.0;
      }
    }
  };
  auto store_chunk = [&](int buf) {
    double* const Xs = Xs0 + buf * F64T_BUF;
    double* const Ps = Ps0 + buf * F64T_BUF;
#pragma unroll
    for (int i = 0; i < F64T_PER; ++i) {
      Xs[x_r(i) * F64T_LD + x_k(i)] = (double)xr[i];           // padded rows / k were loaded as zero
      Ps[(pj0 + F64T_RSTEP * i) * F64T_LD + pk] = pr[i];
    }
  };

  f64x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = (f64x4){0.0, 0.0, 0.0, 0.0};

  const int xa_off = (wr * 64 + l15) * F64T_LD + lq;          // A[i = lane & 15][k = lane >> 4]
  const int pb_off = (wc * 64 + l15) * F64T_LD + lq;          // B[k = lane >> 4][j = lane & 15] = R[j][k]
  auto mfma_steps = [&](int buf, int ks0, int ks1) {
    f64t_mfma_steps(acc, Xs0 + buf * F64T_BUF + xa_off, Ps0 + buf * F64T_BUF + pb_off, ks0, ks1);
  };
  load_chunk(0);
  store_chunk(0);
  __syncthreads();
  int buf = 0;
  for (int32_t k0 = 0; k0 < d; k0 += F64T_KC, buf ^= 1) {
    const bool more = k0 + F64T_KC < d;
    if (more) load_chunk(k0 + F64T_KC);                       // in flight under the first three quarters of this chunk's MFMAs
    mfma_steps(buf, 0, 3);
    if (more) store_chunk(buf ^ 1);                        // the other buffer: nobody reads it before the barrier below
    mfma_steps(buf, 3, F64T_KC / 4);
    __syncthreads();                                       // chunk c + 1 is complete, chunk c's fragments are done with
  }

  // ---- epilogue.  Register r of block (mi, ni) holds row wr * 64 + mi * 16 + (lane >> 4) + 4 r, bit wc * 64 + ni * 16 + (lane & 15)
  // of the tile: bits 16 q .. 16 q + 15 of its ballot are the 16 bits of row mi * 16 + q + 4 r.  Lane l keeps the wave's row l, i.e.
  // the ballots of (mi, r) = (l >> 4, (l >> 2) & 3), quarter q = l & 3.
  double tv[4];
  bool cin[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int32_t c = col0 + wc * 64 + ni * 16 + l15;
    cin[ni] = c < nbits;                                   // columns beyond nbits give zero bits, whatever the threshold
    tv[ni] = (thr && cin[ni]) ? thr[c] : 0.0;
  }
  const int my_mi = lane >> 4, my_r = (lane >> 2) & 3, my_sh = 16 * (lane & 3);
  unsigned long long mine = 0;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      unsigned long long v = 0;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const unsigned long long bal = __ballot(cin[ni] && acc[mi][ni][r] >= tv[ni]);
        v |= ((bal >> my_sh) & 0xFFFFull) << (16 * ni);
      }
      if (my_mi == mi && my_r == r) mine = v;
    }
  const int64_t row = row0 + wr * 64 + lane;
  if (row >= n) return;
  const int32_t bit0 = col0 + wc * 64;                      // first bit of this wave's 64
  if (bit0 >= nbits) return;
  if (out) {
    const int32_t nbv = min(8, (nbits - bit0) >> 3);        // whole bytes of the code in this wave's columns
    uint8_t* p = out + row * out_rs + (bit0 >> 3);
    if (nbv == 8 && (reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
      *reinterpret_cast<unsigned long long*>(p) = mine;
    } else {
      for (int j = 0; j < nbv; ++j) p[j] = (uint8_t)(mine >> (8 * j));
    }
  } else {
    const int64_t dst = dst_row0 + row;
    uint32_t* p = codes + (dst >> 6) * W32 * 64 + (dst & 63);
    const int32_t w0 = bit0 >> 5;
    p[(int64_t)w0 * 64] = (uint32_t)mine;
    if (w0 + 1 < W32) p[(int64_t)(w0 + 1) * 64] = (uint32_t)(mine >> 32);
  }
}

void launch_lsh_encode(const void* X, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, const double* R, const double* thr,
                       int32_t nbits, uint8_t* out, int64_t out_rs, uint32_t* codes, int64_t dst_row0, hipStream_t stream) {
  if (n <= 0) return;
  const uint32_t ncb = (uint32_t)((nbits + F64T_TILE - 1) / F64T_TILE);
  const int32_t W32 = (nbits + 31) / 32;
  const size_t esz = dtype == 0 ? 4 : 8;
  constexpr int64_t STEP = (int64_t)1 << 22;                // rows per launch (a multiple of the tile): the grid stays below 2^31
  for (int64_t r0 = 0; r0 < n; r0 += STEP) {
    const int64_t nn = std::min(STEP, n - r0);
    const uint32_t nrb = (uint32_t)((nn + F64T_TILE - 1) / F64T_TILE);
    const dim3 grid(ncb * nrb);
    const void* x = (const char*)X + (size_t)r0 * (size_t)rs * esz;
    uint8_t* o = out ? out + r0 * out_rs : nullptr;
    f64t_launch(dtype, cs == 1, MI_F64T_KERNELS(lsh_encode_kernel), grid, stream, x, nn, d, rs, cs, R, thr, nbits, o, out_rs, codes,
                W32, dst_row0 + r0, ncb, nrb);
  }
}

}  // namespace mi
