// k-means assignment over whole rows at f64 matrix rate (api_kmeans.hip): id[i] = argmin_c sum_j (double(x[i][j]) -
// double(C[c][j]))^2, the float64 direct-form argmin of pq_encode_kernel with one book, ties to the lower centroid -- the same ids,
// found by a filter, a certificate and an exact fallback:
//
//   km_sqnorm_*_kernel      sum_j double(v_j)^2 of every row of X (xn2) and of every centroid (cn); km_max_kernel: max_c cn[c]
//   km_assign_mfma_kernel   e[i][c] = cn[c] - 2 x_i . c, the expanded form without its row constant, as an f64 GEMM.  On the 128 x 128 tile of
//                           f64_tile.h (geometry, K chunks through LDS, XCD-aware tile order), X promoted to double on load; B is the
//                           centroid table, float32 in memory, promoted to double on load.  The products never leave the registers:
//                           the epilogue keeps per row (lowest e, its centroid, second lowest e) over the workgroup's 128 columns --
//                           4 columns in the lane, 16 lanes by shuffles, the two column waves through LDS -- and writes ONE triple per
//                           (row, column block) to the workspace W[column block][row]
//   km_fold_kernel          thread = row: folds the row's triples in ASCENDING column-block order (no float atomics anywhere; min with
//                           ties to the lower id is exact, so the fold has no rounding of its own), writes the id and, unless
//                           second - best > tau (km_tau below), appends the row to a list through an integer atomic counter
//   km_exact_rows_kernel    a FIXED grid strides over the list, whose length it reads from device memory: every listed row gets all k
//                           centroids in the direct form (pq_sqdist_step, ascending j, strict < over ascending c) and its id overwritten
//
// The list's order is the order the atomics landed in and shows in no result: every listed row is recomputed on its own.
#include <algorithm>

#include "f64_tile.h"
#include "kernels.h"
#include "pq_device.h"

namespace mi {

constexpr int KM_EXACT_GRID = 2048;  // workgroups of km_exact_rows_kernel, whatever the list holds

// ---- the certificate.  With u = 2^-53, gamma = (d + 3) u / (1 - (d + 3) u), xn >= ||x|| and cmax >= max_c ||c||: the direct form
// is within gamma D <= gamma (xn + cmax)^2 of the real squared distance and the computed e within gamma (xn + cmax)^2 of the real
// ||c||^2 - 2 x.c (DESIGN.md 5.14g derives both against this file), so two centroids whose computed e differ by more than
// 4 gamma (xn + cmax)^2 are ordered the same way by the direct form.  The factors 1 + 2^-30 round xn, cmax and tau UP past every
// rounding of this function and of the subtraction second - best; the last term covers operations that underflow.  *big: the
// bound is so large that the direct form may overflow -- the row is not decided here
__host__ __device__ __forceinline__ double km_tau(double xn2, double cmax2, int32_t d, bool* big) {
  const double up = 1.0 + 0x1p-30;
  const double xn = sqrt(xn2) * up, cm = sqrt(cmax2) * up;
  const double s = xn + cm, sq = s * s;
  const double du = (double)(d + 3) * 0x1p-53;
  const double gamma = du / (1.0 - du);
  *big = !(sq < 0x1p1000);
  return 4.0 * gamma * sq * up + (double)(d + 3) * 0x1p-1000;
}

// (best, id, second) of a set of columns, merged with that of another: the lower e wins, equal e go to the lower id; second is the
// lowest e of the rest, so a tie gives second == best
__device__ __forceinline__ void km_merge(double& b, int32_t& id, double& s, double ob, int32_t oid, double os) {
  if (ob < b || (ob == b && oid < id)) {
    s = b < os ? b : os;
    b = ob;
    id = oid;
  } else {
    s = ob < s ? ob : s;
  }
}

// ---- squared norms in float64.  ROWS (cs == 1): one wave per row, lanes stride over the columns; otherwise one thread per row,
// consecutive threads on consecutive rows (coalesced in the [D, N] layout, rs == 1).  Any summation order is within gamma_d
template <typename InT>
__global__ __launch_bounds__(256) void km_sqnorm_wave_kernel(const InT* __restrict__ x, int64_t n, int32_t d, int64_t rs,
                                                            double* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                                // wave-uniform
  const int lane = threadIdx.x & 63;
  const InT* p = x + row * rs;
  double acc = 0.0;
  for (int32_t j = lane; j < d; j += 64) {
    const double v = (double)p[j];
    acc += v * v;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) acc += __shfl_down(acc, s, 64);
  if (lane == 0) out[row] = acc;
}

template <typename InT>
__global__ __launch_bounds__(256) void km_sqnorm_thread_kernel(const InT* __restrict__ x, int64_t n, int32_t d, int64_t rs, int64_t cs,
                                                              double* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const InT* p = x + row * rs;
  double acc = 0.0;
  for (int32_t j = 0; j < d; ++j) {
    const double v = (double)p[(int64_t)j * cs];
    acc += v * v;
  }
  out[row] = acc;
}

// one workgroup: out[0] = max_c cn[c] (cn is finite: float32 centroids, d <= 4096)
__global__ __launch_bounds__(256) void km_max_kernel(const double* __restrict__ cn, int32_t k, double* __restrict__ out) {
  __shared__ double part[4];
  double m = 0.0;
  for (int32_t c = threadIdx.x; c < k; c += 256) m = cn[c] > m ? cn[c] : m;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const double o = __shfl_down(m, s, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int g = 1; g < 4; ++g) m = part[g] > m ? part[g] : m;
    out[0] = m;
  }
}

// ---- the matrix kernel.  ROWS: the K index is the contiguous one of X (cs == 1): a wave reads 4 rows x 16 consecutive k per
// instruction; otherwise (the reference's [D, N] layout, rs == 1, and any other strides) 64 consecutive rows of one k.
// Wb / Ws / Wi [ncb][wstride]: best e, second e (NaN: an e of the row was not finite) and the best's centroid per column block
template <typename InT, bool ROWS>
__global__ __launch_bounds__(256, 2) void km_assign_mfma_kernel(const InT* __restrict__ X, int64_t n, int32_t d, int64_t rs, int64_t cs,
                                                                const float* __restrict__ Cb /*[k][d]*/,
                                                                const double* __restrict__ cn /*[k]*/, int32_t k,
                                                                double* __restrict__ Wb, double* __restrict__ Ws,
                                                                int32_t* __restrict__ Wi, int64_t wstride, uint32_t ncb, uint32_t nrb) {
  extern __shared__ __attribute__((aligned(16))) double km_lds[];
  double* const Xs0 = km_lds;
  double* const Ps0 = km_lds + 2 * F64T_BUF;
  uint32_t cb, rt;
  f64t_tile_order(blockIdx.x, ncb, nrb, &cb, &rt);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1, l15 = lane & 15, lq = lane >> 4;
  const int64_t row0 = (int64_t)rt * F64T_TILE;
  const int32_t col0 = (int32_t)cb * F64T_TILE;
  // element i of this thread in an operand chunk: X (r, kk) = (xr0 + 16 i, xk0) (ROWS) or (xr0 + 64 (i & 1), xk0 + 4 (i >> 1));
  // C (pj0 + 16 i, pk)
  const int xr0 = ROWS ? t / F64T_KC : t % 64, xk0 = ROWS ? t % F64T_KC : t / 64;
  auto x_r = [&](int i) { return ROWS ? xr0 + F64T_RSTEP * i : xr0 + 64 * (i & 1); };
  auto x_k = [&](int i) { return ROWS ? xk0 : xk0 + 4 * (i >> 1); };
  const int pj0 = t / F64T_KC, pk = t % F64T_KC;
  const bool interior = row0 + F64T_TILE <= n && col0 + F64T_TILE <= k;
  const InT* xp0 = X + (row0 + xr0) * rs + (int64_t)xk0 * cs;
  const float* pp0 = Cb + (int64_t)(col0 + pj0) * d + pk;

  InT xr[F64T_PER];
  float pr[F64T_PER];
  bool fast = false;                                        // the chunk in the registers lies inside X and C: no masking
  auto load_chunk = [&](int32_t k0) {
    fast = interior && k0 + F64T_KC <= d;
    if (fast) {
      const InT* xp = xp0 + (int64_t)k0 * cs;
      const float* pp = pp0 + k0;
#pragma unroll
      for (int i = 0; i < F64T_PER; ++i) {
        xr[i] = ROWS ? xp[(int64_t)F64T_RSTEP * i * rs] : xp[(int64_t)(64 * (i & 1)) * rs + (int64_t)(4 * (i >> 1)) * cs];
        pr[i] = pp[(int64_t)F64T_RSTEP * i * d];
      }
    } else {
#pragma unroll
      for (int i = 0; i < F64T_PER; ++i) {
        const int64_t row = row0 + x_r(i);
        const int32_t kk = k0 + x_k(i);
        xr[i] = (row < n && kk < d) ? X[row * rs + (int64_t)kk * cs] : (InT)0;
        const int32_t pj = col0 + pj0 + F64T_RSTEP * i;
        pr[i] = (pj < k && k0 + pk < d) ? Cb[(int64_t)pj * d + k0 + pk] : 0.0f;
      }
    }
  };
  auto store_chunk = [&](int buf) {
    double* const Xs = Xs0 + buf * F64T_BUF;
    double* const Ps = Ps0 + buf * F64T_BUF;
#pragma unroll
    for (int i = 0; i < F64T_PER; ++i) {
      Xs[x_r(i) * F64T_LD + x_k(i)] = (double)xr[i];          // padded rows / k were loaded as zero
      Ps[(pj0 + F64T_RSTEP * i) * F64T_LD + pk] = (double)pr[i];
    }
  };

  f64x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = (f64x4){0.0, 0.0, 0.0, 0.0};

  const int xa_off = (wr * 64 + l15) * F64T_LD + lq;          // A[i = lane & 15][k = lane >> 4]
  const int pb_off = (wc * 64 + l15) * F64T_LD + lq;          // B[k = lane >> 4][j = lane & 15] = C[j][k]
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
    if (more) store_chunk(buf ^ 1);                         // the other buffer: nobody reads it before the barrier below
    mfma_steps(buf, 3, F64T_KC / 4);
    __syncthreads();                                        // chunk c + 1 is complete, chunk c's fragments are done with
  }

  // ---- epilogue.  Register r of block (mi, ni) holds row wr * 64 + mi * 16 + (lane >> 4) + 4 r, column wc * 64 + ni * 16 + (lane & 15)
  // of the tile.  Per (mi, r): the lane's 4 columns in ascending order, then the 16 lanes of the row by xor shuffles (every lane of
  // the 16 ends with the row's triple); lane (lq, l15) keeps the triple of (mi, r) = (l15 >> 2, l15 & 3), so the 64 lanes of a wave
  // hold its 64 rows.
  double cv[4];
  int32_t cid[4];
  bool cin[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    cid[ni] = col0 + wc * 64 + ni * 16 + l15;
    cin[ni] = cid[ni] < k;                                  // columns at or beyond k count as +inf
    cv[ni] = cin[ni] ? cn[cid[ni]] : 0.0;
  }
  double mb = __builtin_inf(), ms = __builtin_inf();
  int32_t mid = 0, mbad = 0;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double bst = __builtin_inf(), sec = __builtin_inf();
      int32_t id = 0, bad = 0;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        double e;
        {
#pragma clang fp contract(off)
          const double two = 2.0 * acc[mi][ni][r];          // exact
          e = cv[ni] - two;                                 // one rounding
        }
        if (cin[ni]) {
          bad |= !(__builtin_fabs(e) < __builtin_inf());
          if (e < bst) {
            sec = bst;
            bst = e;
            id = cid[ni];
          } else if (e < sec) {
            sec = e;
          }
        }
      }
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
        const double ob = __shfl_xor(bst, m, 64), os = __shfl_xor(sec, m, 64);
        const int32_t oid = __shfl_xor(id, m, 64);
        bad |= __shfl_xor(bad, m, 64);
        km_merge(bst, id, sec, ob, oid, os);
      }
      if (l15 == mi * 4 + r) {
        mb = bst;
        ms = sec;
        mid = id;
        mbad = bad;
      }
    }
  const int rl = (l15 >> 2) * 16 + lq + 4 * (l15 & 3);      // this lane's row of the wave's 64
  // the two column waves of a row half meet in LDS (the main loop's buffers are done with: its last statement is a barrier)
  double* const eb = km_lds;                                // [2][64] best, [2][64] second, then ids and flags
  double* const es = km_lds + 128;
  int32_t* const ei = reinterpret_cast<int32_t*>(km_lds + 256);
  int32_t* const ef = ei + 128;
  if (wc == 1) {
    eb[wr * 64 + rl] = mb;
    es[wr * 64 + rl] = ms;
    ei[wr * 64 + rl] = mid;
    ef[wr * 64 + rl] = mbad;
  }
  __syncthreads();
  if (wc == 1) return;
  km_merge(mb, mid, ms, eb[wr * 64 + rl], ei[wr * 64 + rl], es[wr * 64 + rl]);
  mbad |= ef[wr * 64 + rl];
  const int64_t row = row0 + wr * 64 + rl;
  if (row >= n) return;
  const int64_t o = (int64_t)cb * wstride + row;
  Wb[o] = mb;
  Ws[o] = mbad ? __builtin_nan("") : ms;
  Wi[o] = mid;
}

// ---- fold, certificate, list
template <typename OutT>
__global__ __launch_bounds__(256) void km_fold_kernel(const double* __restrict__ Wb, const double* __restrict__ Ws,
                                                     const int32_t* __restrict__ Wi, int64_t wstride, int64_t n, int32_t ncb,
                                                     const double* __restrict__ xn2, const double* __restrict__ cmax2, int32_t d,
                                                     OutT* __restrict__ out, uint32_t* __restrict__ list, uint32_t* __restrict__ count) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  double b = Wb[row], s = Ws[row];
  int32_t id = Wi[row];
  bool bad = s != s;
  for (int32_t cb = 1; cb < ncb; ++cb) {                    // ascending column blocks
    const int64_t o = (int64_t)cb * wstride + row;
    const double os = Ws[o];
    bad |= os != os;
    km_merge(b, id, s, Wb[o], Wi[o], os);
  }
  bool big;
  const double tau = km_tau(xn2[row], cmax2[0], d, &big);
  const bool decided = !bad && !big && (s - b > tau);        // a NaN or an infinity makes this false
  out[row] = (OutT)id;
  if (!decided) list[atomicAdd(count, 1u)] = (uint32_t)row;
}

// ---- the direct form for the listed rows.  Workgroup = one row at a time: the row as float64 in LDS, thread t takes the centroids
// t, t + 256, .. in ascending order.  total (may be NULL) += the list's length, once
template <typename InT, typename OutT>
__global__ __launch_bounds__(256) void km_exact_rows_kernel(const InT* __restrict__ x, int64_t rs, int64_t cs, int32_t d,
                                                           const float* __restrict__ cb, int32_t k, const uint32_t* __restrict__ list,
                                                           const uint32_t* __restrict__ count, OutT* __restrict__ out,
                                                           unsigned long long* __restrict__ total) {
  __shared__ double xs[4096];
  __shared__ double bd[4];
  __shared__ int32_t bc[4];
  const int tid = threadIdx.x;
  const uint32_t cnt = *count;
  if (blockIdx.x == 0 && tid == 0 && total) *total += cnt;
  for (uint32_t i = blockIdx.x; i < cnt; i += gridDim.x) {   // workgroup-uniform
    const int64_t row = (int64_t)list[i];
    __syncthreads();                                         // the row before is done with
    for (int32_t j = tid; j < d; j += 256) xs[j] = (double)x[row * rs + (int64_t)j * cs];
    __syncthreads();
    double best = __builtin_inf();
    int32_t best_c = 0;
    for (int32_t c = tid; c < k; c += 256) {
      const float* cw = cb + (int64_t)c * d;
      double acc = 0.0;
      for (int32_t j = 0; j < d; ++j) acc = pq_sqdist_step(acc, xs[j], (double)cw[j]);
      if (acc < best) {                                      // ascending c, strict: ties stay with the lower c
        best = acc;
        best_c = c;
      }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const double v = __shfl_down(best, s, 64);
      const int32_t vc = __shfl_down(best_c, s, 64);
      if (v < best || (v == best && vc < best_c)) {
        best = v;
        best_c = vc;
      }
    }
    if ((tid & 63) == 0) {
      bd[tid >> 6] = best;
      bc[tid >> 6] = best_c;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int g = 1; g < 4; ++g) {
        const double v = bd[g];
        const int32_t vc = bc[g];
        if (v < best || (v == best && vc < best_c)) {
          best = v;
          best_c = vc;
        }
      }
      out[row] = (OutT)best_c;
    }
  }
}

// ---- launchers
static void sqnorm_launch(const void* x, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, double* out, hipStream_t stream) {
  if (n <= 0) return;
  if (cs == 1) {
    const dim3 grid((unsigned)((n + 3) / 4));
    if (dtype == 0) km_sqnorm_wave_kernel<float><<<grid, 256, 0, stream>>>((const float*)x, n, d, rs, out);
    else km_sqnorm_wave_kernel<double><<<grid, 256, 0, stream>>>((const double*)x, n, d, rs, out);
  } else {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == 0) km_sqnorm_thread_kernel<float><<<grid, 256, 0, stream>>>((const float*)x, n, d, rs, cs, out);
    else km_sqnorm_thread_kernel<double><<<grid, 256, 0, stream>>>((const double*)x, n, d, rs, cs, out);
  }
}

KmWorkspace km_workspace(void* base, int64_t bytes, int32_t k) {
  KmWorkspace w;
  const int64_t ncb = (k + F64T_TILE - 1) / F64T_TILE;
  const int64_t head = ((int64_t)k * 8 + 8 + 8 + 255) / 256 * 256;          // cn, cmax2, count
  const int64_t per_row = 8 + 4 + ncb * (8 + 8 + 4);                        // xn2, list, the triples
  int64_t rows = bytes > head ? (bytes - head) / per_row / F64T_TILE * F64T_TILE : 0;
  rows = std::min<int64_t>(rows, (int64_t)1 << 22);                         // the grids stay far below 2^31
  w.rows = rows;
  if (rows < F64T_TILE) return w;
  char* p = (char*)base;
  w.cn = (double*)p;
  w.cmax2 = w.cn + k;
  w.count = (uint32_t*)(w.cmax2 + 1);
  p += head;
  w.xn2 = (double*)p;
  p += rows * 8;
  w.wb = (double*)p;
  p += rows * ncb * 8;
  w.ws = (double*)p;
  p += rows * ncb * 8;
  w.wi = (int32_t*)p;
  p += rows * ncb * 4;
  w.list = (uint32_t*)p;
  return w;
}

int64_t km_workspace_bytes(int32_t k, int64_t rows) {
  const int64_t ncb = (k + F64T_TILE - 1) / F64T_TILE;
  const int64_t head = ((int64_t)k * 8 + 8 + 8 + 255) / 256 * 256;
  const int64_t r = (rows + F64T_TILE - 1) / F64T_TILE * F64T_TILE;
  return head + r * (8 + 4 + ncb * 20) + 256;
}

template <typename OutT>
static void assign_launch(const void* X, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, const float* cb, int32_t k, OutT* out,
                          unsigned long long* total, const KmWorkspace& w, hipStream_t stream) {
  if (n <= 0) return;
  const uint32_t ncb = (uint32_t)((k + F64T_TILE - 1) / F64T_TILE);
  const size_t esz = dtype == 0 ? 4 : 8;
  sqnorm_launch(cb, 0, k, d, d, 1, w.cn, stream);
  km_max_kernel<<<1, 256, 0, stream>>>(w.cn, k, w.cmax2);
  for (int64_t r0 = 0; r0 < n; r0 += w.rows) {
    const int64_t nn = std::min(w.rows, n - r0);
    const uint32_t nrb = (uint32_t)((nn + F64T_TILE - 1) / F64T_TILE);
    const dim3 grid(ncb * nrb);
    const void* x = (const char*)X + (size_t)r0 * (size_t)rs * esz;
    (void)hipMemsetAsync(w.count, 0, 4, stream);
    sqnorm_launch(x, dtype, nn, d, rs, cs, w.xn2, stream);
    f64t_launch(dtype, cs == 1, MI_F64T_KERNELS(km_assign_mfma_kernel), grid, stream, x, nn, d, rs, cs, cb, w.cn, k, w.wb, w.ws, w.wi,
                w.rows, ncb, nrb);
    km_fold_kernel<OutT><<<dim3((unsigned)((nn + 255) / 256)), 256, 0, stream>>>(w.wb, w.ws, w.wi, w.rows, nn, (int32_t)ncb, w.xn2,
                                                                                 w.cmax2, d, out + r0, w.list, w.count);
    if (dtype == 0)
      km_exact_rows_kernel<float, OutT><<<KM_EXACT_GRID, 256, 0, stream>>>((const float*)x, rs, cs, d, cb, k, w.list, w.count,
                                                                           out + r0, total);
    else
      km_exact_rows_kernel<double, OutT><<<KM_EXACT_GRID, 256, 0, stream>>>((const double*)x, rs, cs, d, cb, k, w.list, w.count,
                                                                            out + r0, total);
  }
}

void launch_km_assign(const void* X, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, const float* cb, int32_t k, int32_t* out,
                      unsigned long long* total, const KmWorkspace& w, hipStream_t stream) {
  assign_launch(X, dtype, n, d, rs, cs, cb, k, out, total, w, stream);
}
void launch_km_assign(const void* X, int dtype, int64_t n, int32_t d, int64_t rs, int64_t cs, const float* cb, int32_t k, uint16_t* out,
                      unsigned long long* total, const KmWorkspace& w, hipStream_t stream) {
  assign_launch(X, dtype, n, d, rs, cs, cb, k, out, total, w, stream);
}

}  // namespace mi
