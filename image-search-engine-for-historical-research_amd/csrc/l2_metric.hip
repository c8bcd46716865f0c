// Squared-L2 metric on top of the inner-product search.
//
//   ||q - g||^2 = ||q||^2 - 2 (q.g - 1/2 ||g||^2)
//
// so ascending distance is descending s(q, g) = q.g - 1/2 ||g||^2 = [q, 1, 1, 1] . [g, c1, c2, c3] with c1 + c2 + c3 = -1/2 ||g||^2:
// an L2 gallery is a raw (MI_NORM_NONE) gallery that carries three hidden columns behind the user's d, and the scoring kernels,
// the certificate, the f64 re-score and the fallbacks run on it as they are.  This file holds what is new:
//   l2_bias_kernel        the hidden columns of a range of stored rows (f32 rows, 16-bit image, rounding norms)
//   l2_augment_kernel     queries as given + three 1.0 columns
//   l2_tail_kernel        the K certified rows of a query -> direct-form f64 distances, order (distance asc, id asc)
//   l2_dense_dist_kernel  every direct-form f64 distance of the gallery (the independent checker), negated for dense_topk64
//   l2_dense_emit_kernel  its (-distance desc) lists -> (distance asc) outputs with -1 / +inf padding
#include <hip/hip_fp16.h>

#include "common.h"
#include "kernels.h"
#include "l2_wave.h"

namespace mi {

// the conversions of ingest.hip's cvt_img
__device__ __forceinline__ uint16_t l2_img(float v, int f16, float& back) {
  if (f16) {
    const _Float16 h = (_Float16)v;
    back = (float)h;
    return __builtin_bit_cast(uint16_t, h);
  }
  const __hip_bfloat16 b = __float2bfloat16(v);
  back = __bfloat162float(b);
  return __builtin_bit_cast(uint16_t, b);
}

__device__ __forceinline__ uint16_t* l2_img_elem(uint16_t* img, int64_t row, int32_t nslices, uint32_t c) {
  const uint32_t r = (uint32_t)(row % TILE), sl = c / SLICE_K, ch = (c % SLICE_K) >> 3;
  return img + ((row / TILE) * nslices + sl) * (int64_t)SLICE_ELEMS + (int64_t)r * SLICE_K + (swz_chunk(r, ch) << 3) + (c & 7u);
}

// One wave per stored row of [row0, row0 + nrows_pad); rows at or beyond row0 + nrows are padding rows of the last tile.
// The row's d user columns are already in gal_f32 / gal_img (launch_ingest, MI_NORM_NONE).  b = -1/2 sum g_j^2 in f64 (products
// of f32 values are exact there), split into c1 = b rounded to the image's 16-bit type (so the image holds it without error;
// kept at fp16's largest finite value where b is beyond it), c2 = f32(b - c1), c3 = f32(b - c1 - c2); columns d + 3 .. dp - 1 are zeros.  The rounding norms are taken again over the
// whole augmented row (the same three sums the ingest takes, in an order of its own: inside their 1e-6 inflation).
__global__ __launch_bounds__(256) void l2_bias_kernel(float* __restrict__ gal_f32, uint16_t* __restrict__ gal_img, int img_f16,
                                                      RowStat* __restrict__ rowstat, int32_t dp, int32_t d, int64_t row0,
                                                      int64_t nrows, int64_t nrows_pad) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nrows_pad) return;
  const int64_t row = row0 + i;
  const int32_t nslices = dp / SLICE_K;
  if (i >= nrows) {                      // padding row: zero image behind the user's columns, no f32 row
    for (int32_t c = d + lane; c < dp; c += 64) *l2_img_elem(gal_img, row, nslices, (uint32_t)c) = 0;
    return;
  }
  float* g = gal_f32 + row * dp;
  double s_g = 0.0, s_b = 0.0, s_d = 0.0;
  for (int32_t c = lane; c < d; c += 64) {
    const float v = g[c];
    float vb;
    (void)l2_img(v, img_f16, vb);
    s_g = __builtin_fma((double)v, (double)v, s_g);
    s_b = __builtin_fma((double)vb, (double)vb, s_b);
    const double df = (double)vb - (double)v;
    s_d = __builtin_fma(df, df, s_d);
  }
  s_g = l2_wave_sum(s_g);
  s_b = l2_wave_sum(s_b);
  s_d = l2_wave_sum(s_d);
  const double b = -0.5 * s_g;
  float c[3], cb[3];
  uint16_t ci[3];
  ci[0] = l2_img((float)b, img_f16, c[0]);
  if (img_f16 && !isfinite(c[0]) && isfinite(b)) {
    // 1/2 ||g||^2 beyond fp16's range: c1 stays the largest finite fp16, so the f32 row and its norm stay finite and exact; the
    // remainder c2 then either fits (the gallery is valid as it is) or becomes inf in the IMAGE only, which is what the create
    // loop looks for (launch_rowstat_img_overflow) before it re-ingests the gallery as bf16
    c[0] = -65504.0f;
    ci[0] = __builtin_bit_cast(uint16_t, (_Float16)c[0]);
  }
  cb[0] = c[0];
  c[1] = (float)(b - (double)c[0]);
  c[2] = (float)(b - (double)c[0] - (double)c[1]);
  ci[1] = l2_img(c[1], img_f16, cb[1]);
  ci[2] = l2_img(c[2], img_f16, cb[2]);
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    s_g += (double)c[e] * (double)c[e];
    s_b += (double)cb[e] * (double)cb[e];
    s_d += ((double)cb[e] - (double)c[e]) * ((double)cb[e] - (double)c[e]);
  }
  for (int32_t col = d + lane; col < dp; col += 64) {
    const int e = col - d;
    g[col] = e < 3 ? (e == 0 ? c[0] : (e == 1 ? c[1] : c[2])) : 0.0f;
    *l2_img_elem(gal_img, row, nslices, (uint32_t)col) = e < 3 ? (e == 0 ? ci[0] : (e == 1 ? ci[1] : ci[2])) : (uint16_t)0;
  }
  if (lane == 0) {
    RowStat rs;
    rs.norm_f32 = (float)(sqrt(s_g) * (1.0 + 1e-6));
    rs.norm_img = (float)(sqrt(s_b) * (1.0 + 1e-6));
    rs.norm_diff = (float)(sqrt(s_d) * (1.0 + 1e-6));
    rowstat[row] = rs;
  }
}

void launch_l2_bias(float* gal_f32, void* gal_img, int img_f16, RowStat* rowstat, int32_t dp, int32_t d, int64_t row0,
                    int64_t nrows, int64_t nrows_pad, hipStream_t stream) {
  if (nrows_pad <= 0) return;
  hipLaunchKernelGGL(l2_bias_kernel, dim3((unsigned)((nrows_pad + 3) / 4)), dim3(256), 0, stream, gal_f32, (uint16_t*)gal_img,
                     img_f16, rowstat, dp, d, row0, nrows, nrows_pad);
}

// queries as given (strided f32 | f64, rounded to f32 like the query ingest does) -> [nq][ld] f32 rows: d columns, three 1.0
// columns (exact in 16 bits), zeros up to ld
template <typename InT>
__global__ __launch_bounds__(256) void l2_augment_kernel(const InT* __restrict__ src, int64_t nq, int32_t d, int64_t rs, int64_t cs,
                                                         float* __restrict__ out, int32_t ld) {
  const int64_t q = blockIdx.x;
  for (int32_t c = threadIdx.x; c < ld; c += 256)
    out[q * ld + c] = c < d ? (float)src[q * rs + (int64_t)c * cs] : (c < d + 3 ? 1.0f : 0.0f);
}

void launch_l2_augment(const void* src, int dtype, int64_t nq, int32_t d, int64_t rs, int64_t cs, float* out, int32_t ld,
                       hipStream_t stream) {
  if (nq <= 0) return;
  if (dtype == 0)
    hipLaunchKernelGGL(l2_augment_kernel<float>, dim3((unsigned)nq), dim3(256), 0, stream, (const float*)src, nq, d, rs, cs, out, ld);
  else
    hipLaunchKernelGGL(l2_augment_kernel<double>, dim3((unsigned)nq), dim3(256), 0, stream, (const double*)src, nq, d, rs, cs, out, ld);
}

constexpr int L2_TAIL_MAX = 2048;

// One workgroup per query: the ke rows the selection certified (ids = row_offset + local row, any order; anything outside the
// shard counts as padding) -> direct-form f64 distances, bitonic sort by (distance asc, id asc), k outputs, the tail padded
// with -1 / +inf.
__global__ __launch_bounds__(256) void l2_tail_kernel(const float* __restrict__ gal_f32, const float* __restrict__ qry,
                                                      int32_t dp, int32_t d, int64_t n, int64_t row_offset,
                                                      const int64_t* __restrict__ ids, int32_t ke, int32_t k,
                                                      int64_t* __restrict__ out_idx, float* __restrict__ out_dist,
                                                      double* __restrict__ out_dist64) {
  __shared__ double s_dist[L2_TAIL_MAX];
  __shared__ int64_t s_id[L2_TAIL_MAX];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t q = blockIdx.x;
  uint32_t k2 = 2;
  while (k2 < (uint32_t)k) k2 <<= 1;
  const float* qrow = qry + q * dp;
  for (uint32_t i = wv; i < k2; i += 4) {
    int64_t id = (int32_t)i < ke ? ids[q * ke + i] : -1;
    const int64_t local = id - row_offset;
    const bool ok = id >= 0 && local >= 0 && local < n;        // (wave-uniform)
    double dist = INFINITY;
    if (ok) dist = l2_direct_wave(qrow, gal_f32 + local * dp, d, lane);
    if (lane == 0) {
      s_dist[i] = dist;
      s_id[i] = ok ? id : -1;
    }
  }
  __syncthreads();
  auto after = [&](uint32_t a, uint32_t b) {                   // entry a belongs behind entry b
    const uint64_t ka = f64_key_nan_highest(s_dist[a]), kb = f64_key_nan_highest(s_dist[b]);
    if (ka != kb) return ka > kb;
    return (uint64_t)s_id[a] > (uint64_t)s_id[b];               // -1 -> the largest: padding last
  };
  for (uint32_t size = 2; size <= k2; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t p = t; p < k2 / 2; p += 256) {
        const uint32_t lo = 2 * p - (p & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        if (after(lo, hi) == up) {
          const double td = s_dist[lo];
          s_dist[lo] = s_dist[hi];
          s_dist[hi] = td;
          const int64_t ti = s_id[lo];
          s_id[lo] = s_id[hi];
          s_id[hi] = ti;
        }
      }
      __syncthreads();
    }
  for (int32_t i = t; i < k; i += 256) {
    out_idx[q * k + i] = s_id[i];
    if (out_dist64) out_dist64[q * k + i] = s_dist[i];
    if (out_dist) out_dist[q * k + i] = (float)s_dist[i];
  }
}

void launch_l2_tail(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int64_t row_offset,
                    const int64_t* ids, int32_t ke, int32_t k, int64_t nq, int64_t* out_idx, float* out_dist, double* out_dist64,
                    hipStream_t stream) {
  if (nq <= 0) return;
  hipLaunchKernelGGL(l2_tail_kernel, dim3((unsigned)nq), dim3(256), 0, stream, gal_f32, qry, dp, d, n, row_offset, ids, ke, k,
                     out_idx, out_dist, out_dist64);
}

// The checker: dense_score64_kernel's 64 x 64 tiling with (q_j - g_j)^2 in place of q_j g_j, over the user's d columns only;
// stores MINUS the distance, so that dense_topk64's (score desc, idx asc) is (distance asc, idx asc).
__global__ __launch_bounds__(256) void l2_dense_dist_kernel(const float* __restrict__ gal, const float* __restrict__ qry, int32_t dp,
                                                            int32_t d, int64_t n, int32_t nq, double* __restrict__ out, int64_t ld) {
  __shared__ double Qs[16][65];
  __shared__ double Gs[16][65];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * 64;
  const int q0 = blockIdx.y * 64;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  const int lr = t >> 2, lk = (t & 3) * 4;
  for (int k0 = 0; k0 < d; k0 += 16) {            // reads stay inside the dp-wide rows (dp is a multiple of 64)
    __syncthreads();
    float4 gv = make_float4(0.f, 0.f, 0.f, 0.f), qv = gv;
    if (row0 + lr < n) gv = *reinterpret_cast<const float4*>(gal + (uint64_t)(row0 + lr) * dp + k0 + lk);
    if (q0 + lr < nq) qv = *reinterpret_cast<const float4*>(qry + (uint64_t)(q0 + lr) * dp + k0 + lk);
    const int c = k0 + lk;                        // columns at or beyond d (the hidden ones) count as equal
    Gs[lk][lr] = c < d ? (double)gv.x : 0.0; Gs[lk + 1][lr] = c + 1 < d ? (double)gv.y : 0.0;
    Gs[lk + 2][lr] = c + 2 < d ? (double)gv.z : 0.0; Gs[lk + 3][lr] = c + 3 < d ? (double)gv.w : 0.0;
    Qs[lk][lr] = c < d ? (double)qv.x : 0.0; Qs[lk + 1][lr] = c + 1 < d ? (double)qv.y : 0.0;
    Qs[lk + 2][lr] = c + 2 < d ? (double)qv.z : 0.0; Qs[lk + 3][lr] = c + 3 < d ? (double)qv.w : 0.0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = Qs[k][ty * 4 + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Gs[k][tx * 4 + j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double df = a[i] - b[j];
          acc[i][j] = fma(df, df, acc[i][j]);
        }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = q0 + ty * 4 + i;
    if (q >= nq) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t r = row0 + tx * 4 + j;
      if (r < n) out[(uint64_t)q * ld + r] = -acc[i][j];
    }
  }
}

void launch_l2_dense_dist(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int32_t nq, double* out,
                          int64_t ld, hipStream_t stream) {
  hipLaunchKernelGGL(l2_dense_dist_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)((nq + 63) / 64)), dim3(256), 0, stream,
                     gal_f32, qry, dp, d, n, nq, out, ld);
}

// [nq][ke] lists of dense_topk64 on the negated distances -> [nq][k] outputs (0.0 - s: a distance of zero comes out as +0.0)
__global__ __launch_bounds__(256) void l2_dense_emit_kernel(const int64_t* __restrict__ idx, const double* __restrict__ neg,
                                                            int64_t nq, int32_t ke, int32_t k, int64_t* __restrict__ out_idx,
                                                            float* __restrict__ out_dist, double* __restrict__ out_dist64) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq * k) return;
  const int64_t q = i / k;
  const int32_t j = (int32_t)(i % k);
  const bool have = j < ke;
  const double dist = have ? 0.0 - neg[q * ke + j] : (double)INFINITY;
  out_idx[i] = have ? idx[q * ke + j] : -1;
  if (out_dist64) out_dist64[i] = dist;
  if (out_dist) out_dist[i] = (float)dist;
}

void launch_l2_dense_emit(const int64_t* idx, const double* neg, int64_t nq, int32_t ke, int32_t k, int64_t* out_idx,
                          float* out_dist, double* out_dist64, hipStream_t stream) {
  if (nq <= 0) return;
  hipLaunchKernelGGL(l2_dense_emit_kernel, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, stream, idx, neg, nq, ke, k,
                     out_idx, out_dist, out_dist64);
}

}  // namespace mi
