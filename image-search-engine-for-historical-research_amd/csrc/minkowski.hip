// Exact Minkowski top-K over the stored f32 rows of a gallery (api_minkowski.hip): faiss IndexFlat with METRIC_L1,
// METRIC_Linf and METRIC_Lp, the reference's fractional_distance.  With t_j = |double(q_j) - double(g_j)| over the caller's d columns
// the value of a (query, row) pair is sum t_j (L1), max t_j (Linf), sum t_j^2 (the bits of l2_direct_wave), sum sqrt(t_j) or
// sum pow(t_j, p), all in float64 and NOT raised to 1 / p.  None of them factors into a product: this is a scan on the vector pipe.
//
// The sum order is l2_direct_wave's: lane l adds columns 4 l + 256 i + {0, 1, 2, 3} in ascending order into one accumulator from +0,
// the 64 partials are combined by l2_wave_sum's xor butterfly (32, 16, ... 1).  A column at or beyond d adds t = 0, which leaves every
// accumulator as it is (they are never negative), so the bits are those of the walk that skips it.
//
//   mink_scan_kernel    the hot path.  Grid = (block of 256 consecutive rows, tile of QT queries), 512 threads.  The tile's queries go to
//                       LDS as float64 once ([QT][round_up(d, 4)], columns beyond d zero); a wave takes R rows at a time, loads them
//                       with float4 loads, converts them to float64 once and evaluates them against QI queries out of LDS at a time
//                       (R x QI accumulators in registers), so a row's HBM bytes and conversions are paid once per tile and a query's
//                       LDS bytes once per R rows.  Rows the allow bitmap clears are not evaluated.  The values go to val [query][row]
//   mink_select_kernel  grid = (part of part_rows consecutive rows, query): the part's values as a stream of (f64_key_nan_highest(value), local
//                       row) -- the sentinel for rows the bitmap clears -- through slab_stream_best; the best k to part [query][part][k]
//   mink_merge_kernel   workgroup = query: the partial lists of its parts -> the k best in order, then ids and values
// The scan cannot select by itself: beside 128 KiB of queries (QT = 8, d = 2048) LDS has no room for the 2048 entries of eight
// queries.  What it writes instead is 8 bytes per (query, row), against 4 d bytes read and 2 d float64 operations.
// No grid barrier, no atomics; the answer is the exact top-k by a total order, so it depends on no launch shape.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "l2_wave.h"
#include "slab_select.h"

namespace mi {

constexpr int MINK_THREADS = 512, MINK_WAVES = MINK_THREADS / 64;
constexpr int MINK_BLOCK_ROWS = 256;                              // rows per scan workgroup
constexpr int MINK_WAVE_ROWS = MINK_BLOCK_ROWS / MINK_WAVES;      // consecutive rows one wave walks

// rows a wave holds in registers at a time / queries it evaluates them against at a time.  sqrt and pow are long instruction
// sequences: they go one row at a time, pow one query at a time as well, so that the inner loop holds four calls, not 128
__host__ __device__ constexpr int mink_rows(int op) { return op == MINK_OP_SQRT || op == MINK_OP_POW ? 1 : 4; }
__host__ __device__ constexpr int mink_queries(int op, int qt) { return op == MINK_OP_POW ? 1 : qt; }
static_assert(MINK_WAVE_ROWS % 4 == 0, "a wave walks whole groups of rows");
static_assert(MINK_BLOCK_ROWS == MINK_SCAN_BLOCK_ROWS, "the self-join starts its scans at whole blocks (api_minkowski_range.hip)");

__device__ __forceinline__ double mink_wave_max(double x) {
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o));
  return x;
}

// one column: the accumulator after the term of (q, g)
template <int OP>
__device__ __forceinline__ double mink_step(double acc, double q, double g, double p) {
  if constexpr (OP == MINK_OP_SQ) {
    const double t = q - g;
    return __builtin_fma(t, t, acc);
  } else {
    const double t = fabs(q - g);
    if constexpr (OP == MINK_OP_L1) return acc + t;
    else if constexpr (OP == MINK_OP_LINF) return fmax(acc, t);
    else if constexpr (OP == MINK_OP_SQRT) return acc + sqrt(t);
    else return acc + pow(t, p);
  }
}

// R rows (16-byte aligned, at least round_up(d, 4) floats) against QI queries of the LDS tile (sq: float64 rows of stride dq)
template <int OP, int R, int QI>
__device__ __forceinline__ void mink_eval(const float* const (&grow)[R], const double* sq, int32_t dq, int32_t d, int lane, double p,
                                          double (&acc)[R][QI]) {
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int q = 0; q < QI; ++q) acc[r][q] = 0.0;
  for (int32_t c = 4 * lane; c < d; c += 256) {
    double g[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float4 b = *reinterpret_cast<const float4*>(grow[r] + c);
      g[r][0] = (double)b.x;
      g[r][1] = c + 1 < d ? (double)b.y : 0.0;                      // (the query tile holds 0.0 there as well: t = 0)
      g[r][2] = c + 2 < d ? (double)b.z : 0.0;
      g[r][3] = c + 3 < d ? (double)b.w : 0.0;
    }
#pragma unroll
    for (int q = 0; q < QI; ++q) {
      const double2 q01 = *reinterpret_cast<const double2*>(sq + (int64_t)q * dq + c);
      const double2 q23 = *reinterpret_cast<const double2*>(sq + (int64_t)q * dq + c + 2);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        double a = acc[r][q];
        a = mink_step<OP>(a, q01.x, g[r][0], p);
        a = mink_step<OP>(a, q01.y, g[r][1], p);
        a = mink_step<OP>(a, q23.x, g[r][2], p);
        a = mink_step<OP>(a, q23.y, g[r][3], p);
        acc[r][q] = a;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int q = 0; q < QI; ++q) acc[r][q] = OP == MINK_OP_LINF ? mink_wave_max(acc[r][q]) : l2_wave_sum(acc[r][q]);
}

__device__ __forceinline__ bool mink_allowed(const uint64_t* __restrict__ allow, int64_t row) {
  return !allow || ((allow[row >> 6] >> (row & 63)) & 1ull);
}

// qry [nq][dp] packed f32 (16-byte aligned rows); val [nq][ld].  Dynamic LDS: QT * round_up(d, 4) doubles
template <int OP, int QT>
__global__ __launch_bounds__(MINK_THREADS) void mink_scan_kernel(const float* __restrict__ gal_f32, const float* __restrict__ qry,
                                                                int32_t dp, int32_t d, int64_t n, int32_t nq,
                                                                const uint64_t* __restrict__ allow, double p, double* __restrict__ val,
                                                                int64_t ld) {
  constexpr int R = mink_rows(OP), QI = mink_queries(OP, QT);
  extern __shared__ __attribute__((aligned(16))) char mink_smem[];
  double* sq = reinterpret_cast<double*>(mink_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t dq = (d + 3) & ~3;
  const int64_t q0 = (int64_t)blockIdx.y * QT;
  const int32_t qn = (int32_t)min((int64_t)QT, (int64_t)nq - q0);    // queries of this tile; the rows of the others are zero
  for (int32_t q = 0; q < QT; ++q)
    for (int32_t c = tid; c < dq; c += MINK_THREADS) sq[q * dq + c] = q < qn && c < d ? (double)qry[(q0 + q) * dp + c] : 0.0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * MINK_BLOCK_ROWS + wave * MINK_WAVE_ROWS;
  for (int g0 = 0; g0 < MINK_WAVE_ROWS; g0 += R) {                    // (every condition below is wave-uniform)
    const int64_t r0 = base + g0;
    if (r0 >= n) break;
    bool live[R], any = false;
    const float* grow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      live[r] = r0 + r < n && mink_allowed(allow, r0 + r);
      any = any || live[r];
      grow[r] = gal_f32 + min(r0 + r, n - 1) * dp;                   // a row beyond n reads the last one and writes nothing
    }
    if (!any) continue;
#pragma unroll 1
    for (int qb = 0; qb < qn; qb += QI) {
      double acc[R][QI];
      mink_eval<OP, R, QI>(grow, sq + (int64_t)qb * dq, dq, d, lane, p, acc);
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int q = 0; q < QI; ++q)
            if (live[r] && qb + q < qn) val[(q0 + qb + q) * ld + r0 + r] = acc[r][q];
      }
    }
  }
}

// dynamic LDS: keys [2 HALF] u64 | ids [2 HALF] i64; k <= HALF.  part_* [nq][nparts][k]
template <int HALF>
__global__ __launch_bounds__(MINK_THREADS) void mink_select_kernel(const double* __restrict__ val, int64_t ld, int64_t n, int64_t part_rows,
                                                                  const uint64_t* __restrict__ allow, int32_t k, int32_t nparts,
                                                                  uint64_t* __restrict__ part_key, int64_t* __restrict__ part_id) {
  extern __shared__ __attribute__((aligned(16))) char mink_smem[];
  uint64_t* s_key = reinterpret_cast<uint64_t*>(mink_smem);
  int64_t* s_id = reinterpret_cast<int64_t*>(s_key + 2 * HALF);
  const int64_t q = blockIdx.y, part = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t r0 = part * part_rows, count = max((int64_t)0, min(n, r0 + part_rows) - r0);
  const double* v = val + q * ld;
  slab_stream_best<HALF, MINK_THREADS>(s_key, s_id, count, tid, [&](int64_t i, uint64_t& key, int64_t& id) {
    const int64_t row = r0 + i;
    if (mink_allowed(allow, row)) {
      key = f64_key_nan_highest(v[row]);
      id = row;
    }
  });
  const int64_t o = (q * nparts + part) * k;
  for (int32_t i = tid; i < k; i += MINK_THREADS) {
    part_key[o + i] = s_key[i];
    part_id[o + i] = s_id[i];
  }
}

template <int HALF>
__global__ __launch_bounds__(MINK_THREADS) void mink_merge_kernel(const uint64_t* __restrict__ part_key, const int64_t* __restrict__ part_id,
                                                                 int32_t k, int32_t nparts, int64_t row_offset,
                                                                 int64_t* __restrict__ out_idx, float* __restrict__ out_val,
                                                                 double* __restrict__ out_val64) {
  extern __shared__ __attribute__((aligned(16))) char mink_smem[];
  uint64_t* s_key = reinterpret_cast<uint64_t*>(mink_smem);
  int64_t* s_id = reinterpret_cast<int64_t*>(s_key + 2 * HALF);
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x;
  const uint64_t* skey = part_key + q * nparts * k;
  const int64_t* sid = part_id + q * nparts * k;
  slab_stream_best<HALF, MINK_THREADS>(s_key, s_id, (int64_t)nparts * k, tid, [&](int64_t i, uint64_t& key, int64_t& id) {
    key = skey[i];
    id = sid[i];
  });
  slab_emit<true, MINK_THREADS>(s_key, s_id, k, q, row_offset, out_idx, out_val, out_val64, tid);
}

// ---- launchers
template <int OP, int QT>
static void mink_scan_launch(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int32_t nq, const uint64_t* allow,
                             double p, double* val, int64_t ld, hipStream_t stream) {
  const size_t lds = (size_t)QT * ((d + 3) & ~3) * 8;
  ensure_dynamic_lds((const void*)mink_scan_kernel<OP, QT>);
  mink_scan_kernel<OP, QT><<<dim3((unsigned)((n + MINK_BLOCK_ROWS - 1) / MINK_BLOCK_ROWS), (unsigned)((nq + QT - 1) / QT)), MINK_THREADS, lds,
                            stream>>>(gal_f32, qry, dp, d, n, nq, allow, p, val, ld);
}

template <int OP>
static void mink_scan_op(int qt, const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int32_t nq, const uint64_t* allow,
                         double p, double* val, int64_t ld, hipStream_t stream) {
  if (qt == 8) mink_scan_launch<OP, 8>(gal_f32, qry, dp, d, n, nq, allow, p, val, ld, stream);
  else if (qt == 4) mink_scan_launch<OP, 4>(gal_f32, qry, dp, d, n, nq, allow, p, val, ld, stream);
  else if (qt == 2) mink_scan_launch<OP, 2>(gal_f32, qry, dp, d, n, nq, allow, p, val, ld, stream);
  else mink_scan_launch<OP, 1>(gal_f32, qry, dp, d, n, nq, allow, p, val, ld, stream);
}

template <int HALF>
static void mink_select_launch(const double* val, int64_t ld, int64_t n, const uint64_t* allow, int32_t k, int32_t nq, int64_t part_rows,
                               int32_t nparts, uint64_t* part_key, int64_t* part_id, int64_t row_offset, int64_t* out_idx, float* out_val,
                               double* out_val64, hipStream_t stream) {
  ensure_dynamic_lds((const void*)mink_select_kernel<HALF>);
  ensure_dynamic_lds((const void*)mink_merge_kernel<HALF>);
  mink_select_kernel<HALF><<<dim3((unsigned)nparts, (unsigned)nq), MINK_THREADS, 2 * HALF * 16, stream>>>(val, ld, n, part_rows, allow, k,
                                                                                                       nparts, part_key, part_id);
  mink_merge_kernel<HALF><<<dim3((unsigned)nq), MINK_THREADS, 2 * HALF * 16, stream>>>(part_key, part_id, k, nparts, row_offset, out_idx,
                                                                                      out_val, out_val64);
}

void launch_minkowski_scan(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int op, double p, const uint64_t* allow,
                           int32_t nq, double* val, int64_t ld, hipStream_t stream) {
  if (nq <= 0 || n < 1) return;
  const int qt = mink_query_tile(d);
  switch (op) {
    case MINK_OP_L1: mink_scan_op<MINK_OP_L1>(qt, gal_f32, qry, dp, d, n, nq, allow, p, val, ld, stream); break;
    case MINK_OP_LINF: mink_scan_op<MINK_OP_LINF>(qt, gal_f32, qry, dp, d, n, nq, allow, p, val, ld, stream); break;
    case MINK_OP_SQ: mink_scan_op<MINK_OP_SQ>(qt, gal_f32, qry, dp, d, n, nq, allow, p, val, ld, stream); break;
    case MINK_OP_SQRT: mink_scan_op<MINK_OP_SQRT>(qt, gal_f32, qry, dp, d, n, nq, allow, p, val, ld, stream); break;
    default: mink_scan_op<MINK_OP_POW>(qt, gal_f32, qry, dp, d, n, nq, allow, p, val, ld, stream); break;
  }
}

void launch_minkowski(const float* gal_f32, const float* qry, int32_t dp, int32_t d, int64_t n, int64_t row_offset, int op, double p,
                      const uint64_t* allow, int32_t k, int32_t nq, double* val, int64_t ld, uint64_t* part_key, int64_t* part_id,
                      int64_t* out_idx, float* out_val, double* out_val64, hipStream_t stream) {
  if (nq <= 0) return;
  launch_minkowski_scan(gal_f32, qry, dp, d, n, op, p, allow, nq, val, ld, stream);
  const int64_t part_rows = mink_part_rows(n);
  const int32_t nparts = mink_parts(n);
  if (k <= 1024)
    mink_select_launch<1024>(val, ld, n, allow, k, nq, part_rows, nparts, part_key, part_id, row_offset, out_idx, out_val, out_val64, stream);
  else
    mink_select_launch<2048>(val, ld, n, allow, k, nq, part_rows, nparts, part_key, part_id, row_offset, out_idx, out_val, out_val64, stream);
}

}  // namespace mi
