// Level-wise split of the random-projection forest (api_forest.hip).  On level l of a tree every node (l, j) orders
// its rows by (projection ascending, row id ascending) and hands the halves to its children; its slice of the permutation is the
// closed form [floor(j n / 2^l), floor((j + 1) n / 2^l)).  (projection, id) is a total order, so the order inside a node does not
// depend on what the level above left behind: one stable LSD radix sort of ALL n rows of the tree, started from the identity, by
// the 64-bit orderable image of the projection (8 digits of 8 bits) and then by the node of the row (ceil(l / 8) digits), puts
// every node's rows into its slice in the node's order -- ties by id because the sort is stable and starts in id order.  Then one
// pass reads the split values off the middles, names every row's node on the next level and, on the last level, writes the tree.
// A group of trees goes through each launch side by side (blockIdx.y).  Per digit: a histogram per chunk of 2048 rows, one
// exclusive scan over (digit, chunk), a stable scatter.  Integer LDS counters are the only atomics; every count, offset and
// position is a function of the keys alone, so the same bytes come out on every call.  No float is ever added here.
#include "common.h"
#include "kernels.h"

namespace mi {

// the digit of pass `ps` of row `id`: passes 0 .. 7 the bytes of the projection's orderable image, low byte first (-0.0 as +0.0;
// negative values with all bits flipped, the others with the sign bit set: unsigned order == (value, then NaN payload) order),
// passes 8 .. the bytes of the node
__device__ __forceinline__ uint32_t forest_digit(const double* __restrict__ col, const int32_t* __restrict__ node, int32_t id, int ps) {
  if (ps >= 8) return ((uint32_t)node[id] >> (8 * (ps - 8))) & 255u;
  unsigned long long u = (unsigned long long)__double_as_longlong(col[id]);
  if ((u << 1) == 0) u = 0;
  u ^= (u >> 63) ? ~0ull : 0x8000000000000000ull;
  return (uint32_t)(u >> (8 * ps)) & 255u;
}

// src == NULL: the identity (the first pass of a level)
__global__ __launch_bounds__(256) void forest_hist_kernel(const double* __restrict__ Pt, int64_t n, int32_t L, int32_t level, int ps,
                                                          const int32_t* __restrict__ node, const int32_t* __restrict__ src,
                                                          uint32_t* __restrict__ hist, int64_t nb) {
  __shared__ uint32_t cnt[256];
  const int64_t t = blockIdx.y, blk = blockIdx.x;
  const double* col = Pt + ((size_t)t * L + level) * n;
  const int32_t* nd = node + (size_t)t * n;
  const int32_t* s = src ? src + (size_t)t * n : nullptr;
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t p0 = blk * FOREST_SORT_CHUNK, p1 = min(p0 + FOREST_SORT_CHUNK, n);
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) atomicAdd(&cnt[forest_digit(col, nd, s ? s[p] : (int32_t)p, ps)], 1u);
  __syncthreads();
  hist[(size_t)t * 256 * nb + (size_t)threadIdx.x * nb + blk] = cnt[threadIdx.x];
}

// exclusive scan of hist [256 * nb] of one tree, in place: entry (digit, chunk) becomes the first position of the chunk's rows of
// that digit
__global__ __launch_bounds__(256) void forest_scan_kernel(uint32_t* __restrict__ hist, int64_t nb) {
  __shared__ uint32_t sc[256];
  uint32_t* h = hist + (size_t)blockIdx.x * 256 * nb;
  const int tid = threadIdx.x;
  uint32_t carry = 0;
  for (int64_t i0 = 0; i0 < 256 * nb; i0 += 256) {
    const uint32_t v = h[i0 + tid];
    sc[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const uint32_t add = tid >= off ? sc[tid - off] : 0u;
      __syncthreads();
      sc[tid] += add;
      __syncthreads();
    }
    h[i0 + tid] = carry + sc[tid] - v;
    carry += sc[255];
    __syncthreads();
  }
}

// one wave per chunk, 64 rows at a time in position order: a row's place is the chunk's cursor of its digit plus the number of
// lower lanes with the same digit; the lowest such lane moves the cursor on
__global__ __launch_bounds__(64) void forest_scatter_kernel(const double* __restrict__ Pt, int64_t n, int32_t L, int32_t level, int ps,
                                                            const int32_t* __restrict__ node, const int32_t* __restrict__ src,
                                                            int32_t* __restrict__ dst, const uint32_t* __restrict__ hist, int64_t nb) {
  __shared__ uint32_t cur[256];
  const int64_t t = blockIdx.y, blk = blockIdx.x;
  const int lane = threadIdx.x;
  const double* col = Pt + ((size_t)t * L + level) * n;
  const int32_t* nd = node + (size_t)t * n;
  const int32_t* s = src ? src + (size_t)t * n : nullptr;
  int32_t* o = dst + (size_t)t * n;
  for (int dg = lane; dg < 256; dg += 64) cur[dg] = hist[(size_t)t * 256 * nb + (size_t)dg * nb + blk];
  __syncthreads();
  const int64_t p0 = blk * FOREST_SORT_CHUNK, p1 = min(p0 + FOREST_SORT_CHUNK, n);
  for (int64_t r0 = p0; r0 < p1; r0 += 64) {
    const int64_t p = r0 + lane;
    const bool valid = p < p1;
    const int32_t id = valid ? (s ? s[p] : (int32_t)p) : 0;
    const uint32_t dg = valid ? forest_digit(col, nd, id, ps) : 0u;
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (dg >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    const uint32_t pos = cur[dg] + rank;
    if (valid && pos < (uint64_t)n) o[pos] = id;              // (pos < n always: the cursors come from the same keys)
    __syncthreads();
    if (valid && rank == 0) cur[dg] += (uint32_t)__popcll(same);
    __syncthreads();
  }
}

// position p of the sorted level: node j = floor(((p + 1) 2^l - 1) / n), its middle mid = floor((2 j + 1) n / 2^(l + 1))
__global__ __launch_bounds__(256) void forest_finish_kernel(const double* __restrict__ Pt, int64_t n, int32_t L, int32_t level,
                                                            const int32_t* __restrict__ sorted, int32_t* __restrict__ node,
                                                            double* __restrict__ splits, int32_t* __restrict__ leaves) {
  const int64_t t = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int32_t id = sorted[(size_t)t * n + p];
  const int64_t j = (((p + 1) << level) - 1) / n;
  const int64_t mid = ((2 * j + 1) * n) >> (level + 1);
  node[(size_t)t * n + id] = (int32_t)(2 * j + (p >= mid ? 1 : 0));
  if (p == mid) splits[(size_t)t * (((size_t)1 << L) - 1) + (((size_t)1 << level) - 1) + j] = Pt[((size_t)t * L + level) * n + id];
  if (level == L - 1) leaves[(size_t)t * n + p] = id;
}

void launch_forest_level(const double* Pt, int64_t n, int32_t tg, int32_t L, int32_t level, int32_t* node, int32_t* ids, uint32_t* hist,
                         double* splits, int32_t* leaves, hipStream_t stream) {
  if (n <= 0 || tg <= 0) return;
  const int64_t nb = forest_sort_blocks(n);
  const dim3 grid((uint32_t)nb, (uint32_t)tg);
  const int passes = 8 + (level + 7) / 8;
  const int32_t* src = nullptr;
  int32_t* buf[2] = {ids, ids + (size_t)tg * n};
  for (int ps = 0; ps < passes; ++ps) {
    int32_t* dst = buf[ps & 1];
    hipLaunchKernelGGL(forest_hist_kernel, grid, dim3(256), 0, stream, Pt, n, L, level, ps, node, src, hist, nb);
    hipLaunchKernelGGL(forest_scan_kernel, dim3((uint32_t)tg), dim3(256), 0, stream, hist, nb);
    hipLaunchKernelGGL(forest_scatter_kernel, grid, dim3(64), 0, stream, Pt, n, L, level, ps, node, src, dst, hist, nb);
    src = dst;
  }
  hipLaunchKernelGGL(forest_finish_kernel, dim3((uint32_t)((n + 255) / 256), (uint32_t)tg), dim3(256), 0, stream, Pt, n, L, level, src,
                     node, splits, leaves);
}

}  // namespace mi
