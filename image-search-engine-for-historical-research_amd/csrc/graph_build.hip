// Building the neighbour table of a graph index from exact nearest-neighbour lists (mi_graph_build).
//
// The forward lists come from the exact search (api_graph.hip runs it on the gallery's own stored rows); the kernels here turn
// them into the table.  With h = R / 2:
//   graph_forward_kernel     the search's answer for a batch of rows [b][ks] (global ids in the order) -> F [n][R]: the row itself
//                            dropped (absent: the last dropped), -1 behind the min(R, n - 1) entries
//   graph_rev_count_kernel   cnt[i] = number of (j, p < h) with F[j][p] == i            (atomics count; they decide no order)
//   graph_rev_scan_kernel    one workgroup: off = exclusive prefix of cnt, 64-bit
//   graph_rev_fill_kernel    the keys (p << 32 | j) of row i's reverse edges into its segment, in whatever order the waves run
//   graph_rev_select_kernel  one wave per row: the R smallest keys of its segment in ascending order -- (position, j), the order
//                            B(i) is defined by -- found one at a time as the smallest key above the last one taken, so the
//                            arrival order of the fill never shows
//   graph_table_kernel       N(i) = F(i)[:h] + the first h of B(i) not yet present + F(i)[h:] not yet present, up to R, then -1
// Two builds of one gallery give the same bytes.
#include "common.h"
#include "kernels.h"

namespace mi {

__global__ __launch_bounds__(256) void graph_forward_kernel(const int64_t* __restrict__ ids, int32_t ks, int64_t row0, int64_t b,
                                                            int64_t row_offset, int64_t n, int32_t R, int32_t* __restrict__ F) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= b) return;
  const int64_t self = row0 + r;
  const int32_t keep = (int32_t)min((int64_t)R, n - 1);     // ks == min(R + 1, n) == keep + 1
  int32_t* out = F + self * R;
  int32_t w = 0;
  for (int32_t c = 0; c < ks && w < keep; ++c) {
    const int64_t loc = ids[r * ks + c] - row_offset;
    if (loc == self || loc < 0 || loc >= n) continue;
    out[w++] = (int32_t)loc;
  }
  for (; w < R; ++w) out[w] = -1;
}

__global__ __launch_bounds__(256) void graph_rev_count_kernel(const int32_t* __restrict__ F, int64_t n, int32_t R, int32_t h,
                                                              uint32_t* __restrict__ cnt) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * h) return;
  const int32_t i = F[(e / h) * R + (e % h)];
  if (i >= 0) atomicAdd(&cnt[i], 1u);
}

// off [n + 1]; one workgroup of 1024 threads, each over a run of consecutive rows
__global__ __launch_bounds__(1024) void graph_rev_scan_kernel(const uint32_t* __restrict__ cnt, int64_t n,
                                                              unsigned long long* __restrict__ off) {
  __shared__ unsigned long long part[1024];
  const int t = threadIdx.x;
  const int64_t per = (n + 1023) / 1024, a = min(n, t * per), b = min(n, a + per);
  unsigned long long s = 0;
  for (int64_t i = a; i < b; ++i) s += cnt[i];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned long long add = t >= o ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  unsigned long long run = part[t] - s;
  for (int64_t i = a; i < b; ++i) {
    off[i] = run;
    run += cnt[i];
  }
  if (t == 1023) off[n] = part[1023];
}

// fill [n] starts at zero; edges [off[n]]
__global__ __launch_bounds__(256) void graph_rev_fill_kernel(const int32_t* __restrict__ F, int64_t n, int32_t R, int32_t h,
                                                             const unsigned long long* __restrict__ off,
                                                             uint32_t* __restrict__ fill, unsigned long long* __restrict__ edges) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * h) return;
  const int64_t j = e / h;
  const int32_t p = (int32_t)(e % h);
  const int32_t i = F[j * R + p];
  if (i < 0) return;
  const uint32_t slot = atomicAdd(&fill[i], 1u);
  edges[off[i] + slot] = ((unsigned long long)p << 32) | (unsigned long long)j;
}

// B [n][R]: the sources j of the R smallest keys of row i, ascending, -1 behind them
__global__ __launch_bounds__(256) void graph_rev_select_kernel(const unsigned long long* __restrict__ off,
                                                               const unsigned long long* __restrict__ edges, int64_t n, int32_t R,
                                                               int32_t* __restrict__ B) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                                           // (wave-uniform)
  const unsigned long long a = off[i], b = off[i + 1];
  unsigned long long last = 0;
  bool have_last = false;
  for (int32_t r = 0; r < R; ++r) {
    unsigned long long best = ~0ull;
    if ((unsigned long long)r < b - a)
      for (unsigned long long e = a + lane; e < b; e += 64) {
        const unsigned long long key = edges[e];
        if ((!have_last || key > last) && key < best) best = key;
      }
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(best, o);
      best = other < best ? other : best;
    }
    if (lane == 0) B[i * R + r] = best == ~0ull ? -1 : (int32_t)(best & 0xffffffffull);
    if (best != ~0ull) last = best, have_last = true;
  }
}

__global__ __launch_bounds__(256) void graph_table_kernel(const int32_t* __restrict__ F, const int32_t* __restrict__ B, int64_t n,
                                                          int32_t R, int32_t h, int32_t* __restrict__ adj) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t *f = F + i * R, *bsrc = B + i * R;
  int32_t* out = adj + i * R;
  int32_t w = 0;
  auto present = [&](int32_t x) {
    for (int32_t c = 0; c < w; ++c)
      if (out[c] == x) return true;
    return false;
  };
  for (int32_t c = 0; c < h && f[c] >= 0; ++c) out[w++] = f[c];
  int32_t took = 0;
  for (int32_t c = 0; c < R && took < h && w < R && bsrc[c] >= 0; ++c)
    if (!present(bsrc[c])) out[w++] = bsrc[c], ++took;
  for (int32_t c = h; c < R && w < R && f[c] >= 0; ++c)
    if (!present(f[c])) out[w++] = f[c];
  for (; w < R; ++w) out[w] = -1;
}

void launch_graph_forward(const int64_t* ids, int32_t ks, int64_t row0, int64_t b, int64_t row_offset, int64_t n, int32_t R,
                          int32_t* F, hipStream_t stream) {
  if (b <= 0) return;
  hipLaunchKernelGGL(graph_forward_kernel, dim3((unsigned)((b + 255) / 256)), dim3(256), 0, stream, ids, ks, row0, b, row_offset, n,
                     R, F);
}

void launch_graph_rev_count(const int32_t* F, int64_t n, int32_t R, uint32_t* cnt, unsigned long long* off, hipStream_t stream) {
  const int32_t h = R / 2;
  hipLaunchKernelGGL(graph_rev_count_kernel, dim3((unsigned)((n * h + 255) / 256)), dim3(256), 0, stream, F, n, R, h, cnt);
  hipLaunchKernelGGL(graph_rev_scan_kernel, dim3(1), dim3(1024), 0, stream, cnt, n, off);
}

void launch_graph_table(const int32_t* F, int64_t n, int32_t R, const unsigned long long* off, uint32_t* fill,
                        unsigned long long* edges, int32_t* B, int32_t* adj, hipStream_t stream) {
  const int32_t h = R / 2;
  hipLaunchKernelGGL(graph_rev_fill_kernel, dim3((unsigned)((n * h + 255) / 256)), dim3(256), 0, stream, F, n, R, h, off, fill,
                     edges);
  hipLaunchKernelGGL(graph_rev_select_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, off, edges, n, R, B);
  hipLaunchKernelGGL(graph_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, F, B, n, R, h, adj);
}

}  // namespace mi
