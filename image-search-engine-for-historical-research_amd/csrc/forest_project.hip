// Projections of the random-projection forest (api_forest.hip):
//   P[i][c] = sum_k double(x_i[k]) * R[c][k]
// over f32 rows of any strides and float64 directions [C][d], on v_mfma_f64_16x16x4_f64.  ONE kernel serves the stored rows of a
// build and the queries of a search, so that a query equal to a stored row gets that row's projections bit for bit.  What makes
// that hold: an output is the accumulator of one (row, direction) pair, started at +0.0 and fed the k-steps 0-3, 4-7, ... in
// ascending order, k beyond d as 0.0 * 0.0; nothing else enters it -- not the tile the row falls in, not its place in the tile, not
// the number of rows or directions of the launch.  (A sum that starts at +0.0 is never -0.0.)
// The tile is a kernel of its own, not lsh.hip's loop: 64 rows x 64 directions per 256-thread workgroup, wave w the rows 16 w ..
// 16 w + 15 against four blocks of 16 directions; K in chunks of 16 through LDS rows of 18 doubles (lsh.hip's stride: 18 r mod 32
// is a different even slot for each of 16 rows), one buffer, two barriers per chunk.  Correct first: no double buffering, and four
// MFMAs per five LDS reads, so it runs well below the rate of lsh.hip's 128 x 128 tile (DESIGN.md 5.17 says what that costs).
#include "common.h"
#include "kernels.h"

namespace mi {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int FP_TILE = 64;          // rows and directions per workgroup
constexpr int FP_KC = 16;            // K-chunk staged in LDS
constexpr int FP_LD = FP_KC + 2;     // LDS row stride in doubles

__global__ __launch_bounds__(256) void forest_project_kernel(const float* __restrict__ X, int64_t m, int32_t d, int64_t rs, int64_t cs,
                                                             const double* __restrict__ R /*[C][d]*/, int32_t C,
                                                             double* __restrict__ out, int64_t out_rs, int64_t out_cs, uint32_t ncb) {
  __shared__ double Xs[FP_TILE * FP_LD];
  __shared__ double Rs[FP_TILE * FP_LD];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, l15 = lane & 15, lq = lane >> 4;
  const int64_t row0 = (int64_t)(blockIdx.x / ncb) * FP_TILE;
  const int32_t col0 = (int32_t)(blockIdx.x % ncb) * FP_TILE;
  const int lr = t / FP_KC, lk = t % FP_KC;                  // this thread stages (lr + 16 i, lk), i < 4, of both operands

  f64x4 acc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = (f64x4){0.0, 0.0, 0.0, 0.0};

  for (int32_t k0 = 0; k0 < d; k0 += FP_KC) {
    const int32_t k = k0 + lk;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = lr + 16 * i;
      const int64_t row = row0 + r;
      const int32_t col = col0 + r;
      Xs[r * FP_LD + lk] = (row < m && k < d) ? (double)X[row * rs + (int64_t)k * cs] : 0.0;
      Rs[r * FP_LD + lk] = (col < C && k < d) ? R[(int64_t)col * d + k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < FP_KC / 4; ++ks) {
      const double a = Xs[(w * 16 + l15) * FP_LD + ks * 4 + lq];           // A[i = lane & 15][k = lane >> 4]
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const double b = Rs[(ni * 16 + l15) * FP_LD + ks * 4 + lq];        // B[k = lane >> 4][j = lane & 15] = R[j][k]
        acc[ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[ni], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // register r of block ni: row 16 w + (lane >> 4) + 4 r, direction 16 ni + (lane & 15)
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int32_t col = col0 + ni * 16 + l15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = row0 + w * 16 + lq + 4 * r;
      if (row < m && col < C) out[row * out_rs + (int64_t)col * out_cs] = acc[ni][r];
    }
  }
}

void launch_forest_project(const float* X, int64_t m, int32_t d, int64_t rs, int64_t cs, const double* R, int32_t C, double* out,
                           int64_t out_rs, int64_t out_cs, hipStream_t stream) {
  if (m <= 0 || C <= 0) return;
  const uint32_t ncb = (uint32_t)((C + FP_TILE - 1) / FP_TILE);            // <= 96 (C <= 256 * 24)
  constexpr int64_t STEP = (int64_t)1 << 24;                               // rows per launch (a multiple of the tile): the grid stays below 2^31
  for (int64_t r0 = 0; r0 < m; r0 += STEP) {
    const int64_t mm = std::min(STEP, m - r0);
    const uint32_t nrb = (uint32_t)((mm + FP_TILE - 1) / FP_TILE);
    hipLaunchKernelGGL(forest_project_kernel, dim3(ncb * nrb), dim3(256), 0, stream, X + r0 * rs, mm, d, rs, cs, R, C, out + r0 * out_rs,
                       out_rs, out_cs, ncb);
  }
}

}  // namespace mi
