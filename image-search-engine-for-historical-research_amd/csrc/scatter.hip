// Scatter matrix for learning a whitening (src/utils/whiten.py:14-48: `np.dot(Xc, Xc.T)` of pcawhitenlearn, `np.dot(df, df.T)`
// of whitenlearn), float64 on the matrix pipe:
//   rows mode   C (+)= sum_n (x_n - c)(x_n - c)^T                       over the n rows of the strided matrix X
//   pairs mode  C (+)= sum_i (x_{q_i} - x_{p_i})(x_{q_i} - x_{p_i})^T   over n_pairs index pairs (no centre)
// It is the whitening GEMM (whiten.hip) turned on its side: the reduction runs over the ROWS of X, both operands come from the
// same rows (column block ti and column block tj), the output is d x d and symmetric.
//  * the 128 x 128 tile of f64_tile.h (geometry, fragment layout, MFMA steps), two workgroups per CU;
//  * the rows stream in chunks of 16: both 16 x 128 operand chunks are promoted to f64 and centred ((double)x - c[col]; pairs:
//    (double)x_q - (double)x_p) ON LOAD and stored [col][F64T_LD] in LDS (conflict-free ds_read_b64
//    fragments); two buffers, one barrier per chunk, the global loads of chunk c + 1 in flight under the MFMAs of chunk c.
//    Never sum x x^T - n c c^T: that cancels on non-negative descriptors;
//  * symmetry: only the T = nt (nt + 1) / 2 tiles with ti <= tj are multiplied (nt = ceil(d / 128); 136 of 256 at d = 2048);
//  * the rows are split over S workgroups per tile so that the grid fills the chip (136 tiles alone do not fill 256 CUs x 2).
//    Every (split, tile) workgroup writes its 128 x 128 partial sum into its own slab of the workspace; scatter_finish_kernel adds
//    the S slabs of an element in ascending split order (on top of the C already there when `accumulate`), writes C[i][j] and
//    mirrors the same double into C[j][i].  No floating-point atomics: the result does not depend on which workgroup finished
//    first, two calls on the same input give the same bits, and C == C.T bit for bit (on diagonal tiles only i <= j is read);
//  * launch order: block = split * T + tile, so the workgroups in flight at one time work on the same few row ranges and an
//    X chunk that left HBM once is served to the other tiles from L2 / Infinity Cache.
// Workspace: scatter_workspace_bytes(d) = scatter_max_splits(d) * T * 128 * 128 * 8 bytes, where scatter_max_splits(d) =
// min(16, 512 MiB / (T * 128 KiB)): 272 MiB at d = 2048, never more than 512 MiB; d <= 11520 (T <= 4096, one split).
// Layouts: KSEQ = the row index is the contiguous one (rs == 1, the reference's [D, N] array seen as .T): a wave reads 16
// consecutive rows of 4 columns per instruction; otherwise 64 consecutive columns of one row (coalesced for cs == 1, correct
// for any strides).  Pairs mode gathers rows and always takes the second path.
#include "common.h"
#include "f64_tile.h"
#include "kernels.h"

#include <algorithm>

namespace mi {

constexpr int S_MAX_SPLITS = 16;
constexpr int64_t S_SLAB = (int64_t)F64T_TILE * F64T_TILE;              // doubles per (split, tile)
constexpr int64_t S_WS_LIMIT = (int64_t)512 << 20;

static inline int64_t scatter_tiles(int32_t d) {
  const int64_t nt = (d + F64T_TILE - 1) / F64T_TILE;
  return nt * (nt + 1) / 2;
}

int scatter_max_splits(int32_t d) {
  const int64_t per = scatter_tiles(d) * S_SLAB * 8;
  return (int)std::min<int64_t>(S_MAX_SPLITS, S_WS_LIMIT / per);      // 0: d too large
}

int64_t scatter_workspace_bytes(int32_t d) { return (int64_t)scatter_max_splits(d) * scatter_tiles(d) * S_SLAB * 8; }

template <typename InT, bool KSEQ, bool PAIRS>
__global__ __launch_bounds__(256, 2) void scatter_mfma_kernel(const InT* __restrict__ X, int64_t n, int32_t d, int64_t rs,
                                                              int64_t cs, const double* __restrict__ centre,
                                                              const int64_t* __restrict__ pq, const int64_t* __restrict__ pp,
                                                              int64_t nk /*rows (pairs) to reduce over*/, uint32_t ntile,
                                                              uint32_t nt, int64_t chunks_per_split,
                                                              double* __restrict__ slabs) {
  extern __shared__ __attribute__((aligned(16))) double s_lds[];
  double* const As0 = s_lds;                                  // [2][128][F64T_LD]
  double* const Bs0 = s_lds + 2 * F64T_BUF;              // [2][128][F64T_LD]
  double* const cen = s_lds + 4 * F64T_BUF;              // [2][128]: centre of the columns of tile ti, tile tj
  const uint32_t tile = blockIdx.x % ntile, split = blockIdx.x / ntile;
  uint32_t ti = 0, rem = tile;
  while (rem >= nt - ti) {
    rem -= nt - ti;
    ++ti;
  }
  const uint32_t tj = ti + rem;
  const F64Lane ln;
  const int t = ln.t;
  const int32_t ca0 = (int32_t)ti * F64T_TILE, cb0 = (int32_t)tj * F64T_TILE;
  const int64_t k_begin = (int64_t)split * chunks_per_split * F64T_KC;
  const int64_t k_end = min(nk, k_begin + chunks_per_split * F64T_KC);

  {
    const int32_t c = (t < F64T_TILE ? ca0 : cb0) + (t & (F64T_TILE - 1));
    cen[t] = (!PAIRS && centre && c < d) ? centre[c] : 0.0;
  }
  // element i of this thread in an operand chunk: (k, col) = KSEQ ? (t % 16, t / 16 + 16 i) : (t / 128 + 2 i, t % 128)
  const int xk0 = KSEQ ? t % F64T_KC : t / F64T_TILE, xc0 = KSEQ ? t / F64T_KC : t % F64T_TILE;
  auto x_k = [&](int i) { return KSEQ ? xk0 : xk0 + 2 * i; };
  auto x_c = [&](int i) { return KSEQ ? xc0 + 16 * i : xc0; };
  const bool cols_inside = cb0 + F64T_TILE <= d;                  // ca0 <= cb0

  InT xa[F64T_PER], xb[F64T_PER];
  InT ya[PAIRS ? F64T_PER : 1], yb[PAIRS ? F64T_PER : 1];            // pairs: the p row
  bool fast = false;
  auto load_chunk = [&](int64_t k0) {
    fast = cols_inside && k0 + F64T_KC <= k_end;
#pragma unroll
    for (int i = 0; i < F64T_PER; ++i) {
      const int64_t k = k0 + x_k(i);
      const int32_t a = ca0 + x_c(i), b = cb0 + x_c(i);
      const bool kin = fast || k < k_end;
      if (PAIRS) {
        // a bad device index can cost a wrong number, never an access outside X
        int64_t rq = kin ? pq[k] : 0, rp = kin ? pp[k] : 0;
        rq = min(max(rq, (int64_t)0), n - 1);
        rp = min(max(rp, (int64_t)0), n - 1);
        const bool ina = fast || (kin && a < d), inb = fast || (kin && b < d);
        xa[i] = ina ? X[rq * rs + (int64_t)a * cs] : (InT)0;
        ya[i] = ina ? X[rp * rs + (int64_t)a * cs] : (InT)0;
        xb[i] = inb ? X[rq * rs + (int64_t)b * cs] : (InT)0;
        yb[i] = inb ? X[rp * rs + (int64_t)b * cs] : (InT)0;
      } else {
        xa[i] = (fast || (kin && a < d)) ? X[k * rs + (int64_t)a * cs] : (InT)0;
        xb[i] = (fast || (kin && b < d)) ? X[k * rs + (int64_t)b * cs] : (InT)0;
      }
    }
  };
  auto store_chunk = [&](int64_t k0, int buf) {
    double* const As = As0 + buf * F64T_BUF;
    double* const Bs = Bs0 + buf * F64T_BUF;
#pragma unroll
    for (int i = 0; i < F64T_PER; ++i) {
      const int kk = x_k(i), c = x_c(i);
      // promoted and centred in float64 exactly like `X - m` / `X[:, q] - X[:, p]` in the reference; padding: zero
      double va, vb;
      if (PAIRS) {
        va = (double)xa[i] - (double)ya[i];
        vb = (double)xb[i] - (double)yb[i];
      } else {
        va = (double)xa[i] - cen[c];
        vb = (double)xb[i] - cen[F64T_TILE + c];
      }
      if (!fast) {
        const bool kin = k0 + kk < k_end;
        va = (kin && ca0 + c < d) ? va : 0.0;
        vb = (kin && cb0 + c < d) ? vb : 0.0;
      }
      As[c * F64T_LD + kk] = va;
      Bs[c * F64T_LD + kk] = vb;
    }
  };

  f64x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = (f64x4){0.0, 0.0, 0.0, 0.0};

  const int a_off = ln.a_off();                              // A[i = lane & 15][k = lane >> 4] = x[k][ca0 + i]
  const int b_off = ln.b_off();                              // B[k = lane >> 4][j = lane & 15] = x[k][cb0 + j]
  auto mfma_steps = [&](int buf, int ks0, int ks1) {
    f64t_mfma_steps(acc, As0 + buf * F64T_BUF + a_off, Bs0 + buf * F64T_BUF + b_off, ks0, ks1);
  };
  if (k_begin < k_end) {
    __syncthreads();                                         // cen[]
    load_chunk(k_begin);
    store_chunk(k_begin, 0);
    __syncthreads();
    int buf = 0;
    for (int64_t k0 = k_begin; k0 < k_end; k0 += F64T_KC, buf ^= 1) {
      const bool more = k0 + F64T_KC < k_end;
      if (more) load_chunk(k0 + F64T_KC);                       // in flight under the first three quarters of this chunk's MFMAs
      mfma_steps(buf, 0, 3);
      if (more) store_chunk(k0 + F64T_KC, buf ^ 1);             // the other buffer: nobody reads it before the barrier below
      mfma_steps(buf, 3, F64T_KC / 4);
      __syncthreads();
    }
  }
  // The whole slab is written (zeros where the tile overhangs d or the split has no rows): the finishing kernel reads every slab of its tile.
  double* const out = slabs + ((int64_t)split * ntile + tile) * S_SLAB;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ln.row(mi, r);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) out[row * F64T_TILE + ln.col(ni)] = acc[mi][ni][r];
    }
}

// C[i][j] = C[j][i] = (accumulate ? C[i][j] : 0) + slab_0 + slab_1 + ... + slab_{S-1}, i <= j, ascending split order
__global__ __launch_bounds__(256) void scatter_finish_kernel(const double* __restrict__ slabs, uint32_t ntile, uint32_t nt,
                                                             int32_t nsplit, int32_t d, int accumulate,
                                                             double* __restrict__ C) {
  const uint32_t tile = blockIdx.x;
  uint32_t ti = 0, rem = tile;
  while (rem >= nt - ti) {
    rem -= nt - ti;
    ++ti;
  }
  const uint32_t tj = ti + rem;
  const int i = blockIdx.y * 2 + (threadIdx.x >> 7), j = threadIdx.x & 127;
  const int64_t gi = (int64_t)ti * F64T_TILE + i, gj = (int64_t)tj * F64T_TILE + j;
  if (gi >= d || gj >= d || gi > gj) return;
  double v = accumulate ? C[gi * d + gj] : 0.0;
  const double* p = slabs + (int64_t)tile * S_SLAB + i * F64T_TILE + j;
  for (int32_t s = 0; s < nsplit; ++s) v += p[(int64_t)s * ntile * S_SLAB];
  C[gi * d + gj] = v;
  C[gj * d + gi] = v;
}

// how many workgroups share the rows of one tile: the most even filling of the chip's 2 x CUs workgroup slots, at least 16
// chunks (256 rows) per workgroup, at most what the workspace holds
static int scatter_pick_splits(int32_t d, int64_t nk) {
  const int64_t T = scatter_tiles(d), slots = 2 * (int64_t)current_device_cus();
  const int64_t chunks = (nk + F64T_KC - 1) / F64T_KC;
  const int smax = (int)std::max<int64_t>(1, std::min<int64_t>(scatter_max_splits(d), chunks / 16));
  int best = 1;
  double best_eff = 0.0;
  for (int s = 1; s <= smax; ++s) {
    const int64_t wg = T * s;
    const double eff = (double)wg / (double)((wg + slots - 1) / slots * slots);
    if (eff > best_eff + 1e-9) {
      best = s;
      best_eff = eff;
    }
  }
  return best;
}

void launch_scatter(const void* X, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, const double* centre,
                    const int64_t* pair_q, const int64_t* pair_p, int64_t n_pairs, double* C, int accumulate,
                    double* workspace, hipStream_t stream) {
  const bool pairs = pair_q != nullptr;
  const int64_t nk = pairs ? n_pairs : n;
  const uint32_t nt = (uint32_t)((d + F64T_TILE - 1) / F64T_TILE), ntile = (uint32_t)scatter_tiles(d);
  const int nsplit = scatter_pick_splits(d, nk);
  const int64_t chunks = (nk + F64T_KC - 1) / F64T_KC;
  const int64_t cps = (chunks + nsplit - 1) / nsplit;
  const dim3 grid(ntile * (uint32_t)nsplit), block(256);
  const int lds = F64T_LDS_BYTES + 2 * F64T_TILE * (int)sizeof(double);          // and cen[]
#define MI_S_LAUNCH(T, KSEQ, PAIRS)                                                                                      \
  do {                                                                                                                   \
    ensure_dynamic_lds((const void*)scatter_mfma_kernel<T, KSEQ, PAIRS>, lds);                                           \
    hipLaunchKernelGGL((scatter_mfma_kernel<T, KSEQ, PAIRS>), grid, block, lds, stream, (const T*)X, n, d, rs, cs, centre, \
                       pair_q, pair_p, nk, ntile, nt, cps, workspace);                                                   \
  } while (0)
  if (dtype == 0) {
    if (pairs) MI_S_LAUNCH(float, false, true);
    else if (rs == 1 && cs != 1) MI_S_LAUNCH(float, true, false);
    else MI_S_LAUNCH(float, false, false);
  } else {
    if (pairs) MI_S_LAUNCH(double, false, true);
    else if (rs == 1 && cs != 1) MI_S_LAUNCH(double, true, false);
    else MI_S_LAUNCH(double, false, false);
  }
#undef MI_S_LAUNCH
  hipLaunchKernelGGL(scatter_finish_kernel, dim3(ntile, F64T_TILE / 2), block, 0, stream, workspace, ntile, nt, nsplit, d,
                     accumulate, C);
}

}  // namespace mi
