// Learning PQ codebooks on the device: the kernels of mi_pq_train (api_pq_train.hip).  Lloyd's iteration from
// given centroids is a deterministic function of its inputs; the assignment is pq_encode_kernel (pq.hip) as it stands, this file
// holds what goes around it.
//
//   pq_init_rows_kernel     the default C_0: codeword c of every book is the book's slice of row floor(c n / Ks), rounded to float32
// The code type is a template argument of the three kernels below: bytes for mi_pq_train, uint16 for mi_pqw_train (Ks <= 8192).
//
//   pq_code_columns_kernel  codes [n][M] -> one contiguous column per book, cols[M][n]: the update scans a column Ks times
//   pq_moved_kernel         number of differing codes of two code arrays, added into a device uint64 (one vector atomic per
//                           workgroup; integer addition has no order problem)
//   pq_update_kernel        THE centroid update.  One wave owns (book j, codeword c) and a slice of PU_COLS columns.  It walks the
//                           book's code column PU_ROWS rows at a step: lane l reads the code byte of row 64 b + l, the wave takes
//                           the __ballot of code == c, and every member writes its row to an LDS list at the position the ballot
//                           gives it (members below it in this block + members of the blocks before), i.e. in ASCENDING row order.
//                           The wave then walks the list PU_AHEAD members at a time: the loads of the member rows are independent
//                           and issued together, only the float64 add chain is sequential.  S[i] starts at +0.0 and takes
//                           double(x[r][j L + i]) member by member; at the end C[j][c][i] = (float)(S[i] / (double)count), one
//                           IEEE divide, one rounding.  No atomics on the sums: they would give neither the order nor the bits.
//                           A codeword without members stores nothing and so keeps its value.
#include <algorithm>

#include "kernels.h"

namespace mi {

template <typename InT>
__global__ __launch_bounds__(256) void pq_init_rows_kernel(const InT* __restrict__ x, int64_t rs, int64_t cs, int64_t n, int32_t M,
                                                          int32_t Ks, int32_t L, float* __restrict__ cb) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)M * Ks * L) return;
  const int32_t i = (int32_t)(t % L);
  const int32_t c = (int32_t)((t / L) % Ks);
  const int32_t j = (int32_t)(t / ((int64_t)L * Ks));
  const int64_t row = (int64_t)c * n / Ks;
  cb[t] = (float)x[row * rs + ((int64_t)j * L + i) * cs];
}

// grid = (row blocks of 256, M): consecutive threads write consecutive codes of one column
template <typename CodeT>
__global__ __launch_bounds__(256) void pq_code_columns_kernel(const CodeT* __restrict__ codes, int32_t M, int64_t row0, int64_t row1,
                                                             int64_t n, CodeT* __restrict__ cols) {
  const int64_t r = row0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= row1) return;
  const int32_t j = (int32_t)blockIdx.y;
  cols[(int64_t)j * n + r] = codes[r * M + j];
}

// thread = 16 bytes of both arrays (the buffers are 16-byte aligned; the last thread walks the bytes that are left)
template <typename CodeT>
__global__ __launch_bounds__(256) void pq_moved_kernel(const CodeT* __restrict__ ca, const CodeT* __restrict__ cb, int64_t bytes,
                                                      unsigned long long* __restrict__ count) {
  constexpr int BITS = 8 * (int)sizeof(CodeT);
  constexpr uint32_t MASK = (1u << BITS) - 1u;
  const uint8_t* a = reinterpret_cast<const uint8_t*>(ca);
  const uint8_t* b = reinterpret_cast<const uint8_t*>(cb);
  __shared__ uint32_t part[4];
  const int64_t o = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
  uint32_t diff = 0;
  if (o + 16 <= bytes) {
    const uint4 va = *reinterpret_cast<const uint4*>(a + o), vb = *reinterpret_cast<const uint4*>(b + o);
    const uint32_t w[4] = {va.x ^ vb.x, va.y ^ vb.y, va.z ^ vb.z, va.w ^ vb.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int s = 0; s < 32; s += BITS) diff += ((w[e] >> s) & MASK) != 0u;
  } else {
    for (int64_t p = o; p < bytes; p += (int64_t)sizeof(CodeT))
      diff += *reinterpret_cast<const CodeT*>(a + p) != *reinterpret_cast<const CodeT*>(b + p);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) diff += __shfl_down(diff, s, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = diff;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t total = part[0] + part[1] + part[2] + part[3];
    if (total) atomicAdd(count, (unsigned long long)total);
  }
}

// ---- update.  Workgroup = one wave; thread l owns the columns col0 + l + 64 k, k < PU_CPT, of the slice
constexpr int PU_CPT = 2, PU_COLS = 64 * PU_CPT;      // L = 128: one wave per (book, codeword), two coalesced 256-byte reads a row
constexpr int PU_BLOCKS = 8, PU_ROWS = 64 * PU_BLOCKS; // rows of the code column per step: 8 independent byte loads a lane
constexpr int PU_AHEAD = 4;                           // member rows whose loads are in flight together

template <typename InT, typename CodeT>
__global__ __launch_bounds__(64) void pq_update_kernel(const InT* __restrict__ x, int64_t rs, int64_t cs, int64_t n,
                                                      const CodeT* __restrict__ cols, int32_t Ks, int32_t L,
                                                      float* __restrict__ cb) {
#pragma clang fp contract(off)
  __shared__ uint32_t list[PU_ROWS];
  const int lane = threadIdx.x;
  const int32_t col0 = (int32_t)blockIdx.x * PU_COLS, c = (int32_t)blockIdx.y, j = (int32_t)blockIdx.z;
  const CodeT* col = cols + (int64_t)j * n;
  const unsigned long long below = (1ull << lane) - 1ull;
  bool own[PU_CPT];
  const InT* xc[PU_CPT];
#pragma unroll
  for (int k = 0; k < PU_CPT; ++k) {
    const int32_t i = col0 + lane + 64 * k;
    own[k] = i < L;
    xc[k] = x + ((int64_t)j * L + (own[k] ? i : 0)) * cs;   // a lane beyond L reads column 0 of the book and stores nothing
  }
  double acc[PU_CPT];
#pragma unroll
  for (int k = 0; k < PU_CPT; ++k) acc[k] = 0.0;
  int64_t count = 0;

  int32_t cur[PU_BLOCKS], nxt[PU_BLOCKS];
#pragma unroll
  for (int b = 0; b < PU_BLOCKS; ++b) {
    const int64_t row = (int64_t)64 * b + lane;
    cur[b] = row < n ? (int32_t)col[row] : -1;
  }
  for (int64_t r0 = 0; r0 < n; r0 += PU_ROWS) {        // wave-uniform
    // the next step's code bytes are on their way while this step's members are added
#pragma unroll
    for (int b = 0; b < PU_BLOCKS; ++b) {
      const int64_t row = r0 + PU_ROWS + (int64_t)64 * b + lane;
      nxt[b] = row < n ? (int32_t)col[row] : -1;
    }
    int32_t members = 0;
#pragma unroll
    for (int b = 0; b < PU_BLOCKS; ++b) {
      const bool mine = cur[b] == c;
      const unsigned long long mask = __ballot(mine);
      if (mine) list[members + __popcll(mask & below)] = (uint32_t)(64 * b + lane);
      members += __popcll(mask);
    }
    __syncthreads();
    for (int32_t p = 0; p < members; p += PU_AHEAD) {  // wave-uniform: members comes from ballots
      InT v[PU_AHEAD][PU_CPT];
#pragma unroll
      for (int u = 0; u < PU_AHEAD; ++u) {
        const int64_t row = r0 + (int64_t)__builtin_amdgcn_readfirstlane((int)list[min(p + u, members - 1)]);
#pragma unroll
        for (int k = 0; k < PU_CPT; ++k) v[u][k] = xc[k][row * rs];
      }
#pragma unroll
      for (int u = 0; u < PU_AHEAD; ++u)
        if (p + u < members) {
#pragma unroll
          for (int k = 0; k < PU_CPT; ++k) acc[k] = acc[k] + (double)v[u][k];
        }
    }
    __syncthreads();                                   // the list is rewritten by the next step
    count += members;
#pragma unroll
    for (int b = 0; b < PU_BLOCKS; ++b) cur[b] = nxt[b];
  }
  if (count == 0) return;
  const double cnt = (double)count;
#pragma unroll
  for (int k = 0; k < PU_CPT; ++k)
    if (own[k]) cb[((int64_t)j * Ks + c) * L + col0 + lane + 64 * k] = (float)(acc[k] / cnt);
}

// ---- launchers
void launch_pq_init_rows(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, int32_t M, int32_t Ks, int32_t L, float* cb,
                         hipStream_t stream) {
  const dim3 grid((unsigned)(((int64_t)M * Ks * L + 255) / 256));
  if (dtype == 0) pq_init_rows_kernel<float><<<grid, 256, 0, stream>>>((const float*)x, rs, cs, n, M, Ks, L, cb);
  else pq_init_rows_kernel<double><<<grid, 256, 0, stream>>>((const double*)x, rs, cs, n, M, Ks, L, cb);
}

template <typename CodeT>
static void code_columns_launch(const CodeT* codes, int32_t M, int64_t n, CodeT* cols, hipStream_t stream) {
  const int64_t step = (int64_t)1 << 30;               // rows per launch: the grid stays below 2^31
  for (int64_t r = 0; r < n; r += step) {
    const int64_t mm = std::min(step, n - r);
    pq_code_columns_kernel<CodeT><<<dim3((unsigned)((mm + 255) / 256), (unsigned)M), 256, 0, stream>>>(codes, M, r, r + mm, n, cols);
  }
}

template <typename CodeT>
static void moved_launch(const CodeT* a, const CodeT* b, int64_t bytes, unsigned long long* count, hipStream_t stream) {
  const int64_t step = (int64_t)1 << 40;               // bytes per launch, a multiple of 16 x 256
  for (int64_t o = 0; o < bytes; o += step) {
    const int64_t mm = std::min(step, bytes - o);
    pq_moved_kernel<CodeT><<<dim3((unsigned)((mm + 4095) / 4096)), 256, 0, stream>>>(a + o / (int64_t)sizeof(CodeT),
                                                                                    b + o / (int64_t)sizeof(CodeT), mm, count);
  }
}

template <typename CodeT>
static void update_launch(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const CodeT* cols, int32_t M, int32_t Ks,
                          int32_t L, float* cb, hipStream_t stream) {
  const dim3 grid((unsigned)((L + PU_COLS - 1) / PU_COLS), (unsigned)Ks, (unsigned)M);
  if (dtype == 0) pq_update_kernel<float, CodeT><<<grid, 64, 0, stream>>>((const float*)x, rs, cs, n, cols, Ks, L, cb);
  else pq_update_kernel<double, CodeT><<<grid, 64, 0, stream>>>((const double*)x, rs, cs, n, cols, Ks, L, cb);
}

void launch_pq_code_columns(const uint8_t* codes, int32_t M, int64_t n, uint8_t* cols, hipStream_t stream) {
  code_columns_launch(codes, M, n, cols, stream);
}
void launch_pq_code_columns(const uint16_t* codes, int32_t M, int64_t n, uint16_t* cols, hipStream_t stream) {
  code_columns_launch(codes, M, n, cols, stream);
}

void launch_pq_moved(const uint8_t* a, const uint8_t* b, int64_t bytes, unsigned long long* count, hipStream_t stream) {
  moved_launch(a, b, bytes, count, stream);
}
void launch_pq_moved(const uint16_t* a, const uint16_t* b, int64_t bytes, unsigned long long* count, hipStream_t stream) {
  moved_launch(a, b, bytes, count, stream);
}

void launch_pq_update(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const uint8_t* cols, int32_t M, int32_t Ks, int32_t L,
                      float* cb, hipStream_t stream) {
  update_launch(x, dtype, rs, cs, n, cols, M, Ks, L, cb, stream);
}
void launch_pq_update(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const uint16_t* cols, int32_t M, int32_t Ks, int32_t L,
                      float* cb, hipStream_t stream) {
  update_launch(x, dtype, rs, cs, n, cols, M, Ks, L, cb, stream);
}

}  // namespace mi
