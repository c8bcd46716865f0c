// What follows the scan in a Minkowski radius search or self-join (api_minkowski_range.hip).  The scan itself is
// minkowski.hip's mink_scan_kernel, launched as it stands: val [query][row] holds the float64 value of every admitted (query, row)
// pair of one chunk of queries.  A hit is an admitted row with value <= radius (inclusive; a NaN is never one); in the self-join
// query q is stored row self_row0 + q and only the rows above it count.
//
//   mink_range_count_kernel    grid = (part of the rows, query), parts being whole 2048-row slabs as in mink_select_kernel: the part's
//                              hits, by a ballot / popcount per wave and a sum over the waves in LDS -> cnt [query][part]
//   mink_range_offsets_kernel  one workgroup: the exclusive prefix of cnt over (query, part) in that order -> off [query][part], the
//                              place of the pair's first hit among the chunk's; lims[1 + query] on top of lims[0], the chunk's base
//   mink_range_emit_kernel     the count's traversal again: a hit goes to off + hits before it in the part (the waves' counts of the
//                              step prefixed in LDS + the ballot below the lane), as (f64_key_nan_highest(value), local row): a
//                              query's list is in ascending row order
// csr_order.hip then orders every query's list by (key asc, row asc) and writes it out.  Every place is a prefix sum over (query,
// part, row) in ascending order and (key, row) is a total order, so nothing follows the order in which workgroups ran: no atomics, no
// grid barrier.  From the emit on every kernel first reads *total, the call's hit count, from device memory: beyond max_results it
// writes nothing (uniform per launch).
#include "common.h"
#include "f64_key.h"
#include "kernels.h"

namespace mi {

constexpr int MR_THREADS = 512, MR_WAVES = MR_THREADS / 64;
constexpr int MR_SCAN_THREADS = 1024;

// row r of the chunk's values (local row a.row_base + r) is a hit of query q
__device__ __forceinline__ bool mr_hit(const double* __restrict__ v, int64_t r, int64_t row_base, const uint64_t* __restrict__ allow,
                                       double radius, int64_t qrow) {
  const int64_t row = row_base + r;
  if (allow && !((allow[row >> 6] >> (row & 63)) & 1ull)) return false;     // (the scan left no value there)
  if (row <= qrow) return false;                                            // the self-join; qrow = -1 otherwise
  return v[r] <= radius;
}

__global__ __launch_bounds__(MR_THREADS) void mink_range_count_kernel(const double* __restrict__ val, int64_t ld, int64_t nrows,
                                                                     int64_t row_base, int64_t part_rows, int32_t nparts,
                                                                     const uint64_t* __restrict__ allow, double radius,
                                                                     int64_t self_row0, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t s_cnt[MR_WAVES];
  const int64_t q = blockIdx.y, part = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = part * part_rows, r1 = min(nrows, r0 + part_rows);
  const int64_t qrow = self_row0 >= 0 ? self_row0 + q : -1;
  const double* v = val + q * ld;
  uint32_t mine = 0;                                                        // wave-uniform
  for (int64_t b = r0; b < r1; b += MR_THREADS) {
    const int64_t r = b + tid;
    const bool hit = r < r1 && mr_hit(v, r, row_base, allow, radius, qrow);
    mine += (uint32_t)__popcll(__ballot(hit));
  }
  if (lane == 0) s_cnt[wave] = mine;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < MR_WAVES; ++w) t += s_cnt[w];
    cnt[q * nparts + part] = t;
  }
}

// m = nq * nparts counts; a thread sums a run of `per` consecutive ones, the runs' sums are prefixed across the workgroup
__global__ __launch_bounds__(MR_SCAN_THREADS) void mink_range_offsets_kernel(const uint32_t* __restrict__ cnt, int64_t m, int32_t nparts,
                                                                            int32_t first, int32_t write_lims,
                                                                            int64_t* __restrict__ off, int64_t* __restrict__ lims) {
  __shared__ long long s_wave[MR_SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t per = (m + MR_SCAN_THREADS - 1) / MR_SCAN_THREADS;
  const int64_t i0 = min(m, tid * per), i1 = min(m, i0 + per);
  long long sum = 0;
  for (int64_t i = i0; i < i1; ++i) sum += (long long)cnt[i];
  long long incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  long long before = 0;
  for (int w = 0; w < wave; ++w) before += s_wave[w];
  const int64_t base = first ? 0 : lims[0];
  int64_t run = (int64_t)(before + incl - sum);                             // hits of the chunk before entry i0
  for (int64_t i = i0; i < i1; ++i) {
    off[i] = run;
    run += (int64_t)cnt[i];
    if (write_lims && i % nparts == nparts - 1) lims[1 + i / nparts] = base + run;
  }
  if (write_lims && first && tid == 0) lims[0] = 0;
}

__global__ __launch_bounds__(MR_THREADS) void mink_range_emit_kernel(const double* __restrict__ val, int64_t ld, int64_t nrows,
                                                                    int64_t row_base, int64_t part_rows, int32_t nparts,
                                                                    const uint64_t* __restrict__ allow, double radius, int64_t self_row0,
                                                                    const int64_t* __restrict__ off, const int64_t* __restrict__ total,
                                                                    int64_t max_results, uint64_t* __restrict__ key,
                                                                    uint32_t* __restrict__ row) {
  __shared__ uint32_t s_cnt[2][MR_WAVES];
  if (*total > max_results) return;
  const int64_t q = blockIdx.y, part = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = part * part_rows, r1 = min(nrows, r0 + part_rows);
  const int64_t qrow = self_row0 >= 0 ? self_row0 + q : -1;
  const double* v = val + q * ld;
  int64_t run = off[q * nparts + part];
  int it = 0;
  for (int64_t b = r0; b < r1; b += MR_THREADS, it ^= 1) {
    const int64_t r = b + tid;
    const bool hit = r < r1 && mr_hit(v, r, row_base, allow, radius, qrow);
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_cnt[it][wave] = (uint32_t)__popcll(m);
    __syncthreads();                                                        // (the other half of s_cnt is the previous step's)
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < MR_WAVES; ++w) {
      const uint32_t c = s_cnt[it][w];
      if (w < wave) before += c;
      tot += c;
    }
    if (hit) {
      const int64_t pos = run + before + __popcll(m & ((1ull << lane) - 1ull));
      key[pos] = f64_key_nan_highest(v[r]);
      row[pos] = (uint32_t)(row_base + r);
    }
    run += tot;
  }
}

// ---- launchers
void launch_mink_range_count(const MinkRangeArgs& a, bool first, bool write_lims, hipStream_t stream) {
  if (a.nq <= 0) return;
  const int32_t nparts = mink_parts(a.nrows);
  mink_range_count_kernel<<<dim3((unsigned)nparts, (unsigned)a.nq), MR_THREADS, 0, stream>>>(
      a.val, a.ld, a.nrows, a.row_base, mink_part_rows(a.nrows), nparts, a.allow, a.radius, a.self_row0, a.cnt);
  mink_range_offsets_kernel<<<dim3(1), MR_SCAN_THREADS, 0, stream>>>(a.cnt, (int64_t)a.nq * nparts, nparts, first ? 1 : 0,
                                                                    write_lims ? 1 : 0, a.off, a.lims);
}

void launch_mink_range_emit(const MinkRangeArgs& a, hipStream_t stream) {
  if (a.nq <= 0) return;
  const int32_t nparts = mink_parts(a.nrows);
  mink_range_emit_kernel<<<dim3((unsigned)nparts, (unsigned)a.nq), MR_THREADS, 0, stream>>>(
      a.val, a.ld, a.nrows, a.row_base, mink_part_rows(a.nrows), nparts, a.allow, a.radius, a.self_row0, a.off, a.total, a.max_results,
      a.key[0], a.row[0]);
}

}  // namespace mi
