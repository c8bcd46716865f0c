// Kernels of the in-place row removal (mi_gallery_remove_rows, api_remove.hip).
//   remove_gather_kernel: one block of surviving rows gathered from the gallery into a staging area of the gallery's own
//                         layout (f32 rows, 16-bit tile-blocked image, RowStat), one workgroup per (destination tile, K-slice)
//   remove_copy_kernel:   the staging area written back over the gallery as three contiguous runs
// Neither uses LDS or scratch; every store is a plain 16-byte vector store.
#include "kernels.h"

#include <algorithm>

namespace mi {

constexpr int REMOVE_BATCH = 8;       // 16-byte loads in flight per lane before their stores (f32 rows; checked in the ISA)

// Workgroup (t, sl) of the grid: destination tile t of the block (destination rows j0 + 256 t ... of the gallery, rows 256 t ...
// of the staging area; j0 is a multiple of 256, so a row's swizzle slot is the same in both) and K-slice sl.  It moves
//   the image:  the whole 16 KiB (tile, slice) block.  Lane l of pass u writes the 16-byte chunk 256 u + l of the block -- row
//               r = chunk >> 2, physical slot p = chunk & 3, i.e. logical chunk c = p ^ swz(r) -- so a wave stores 1 KiB
//               contiguous bytes per instruction, and reads chunk c from the slot of the SOURCE row, c ^ swz(ri).  Consecutive
//               surviving rows are consecutive source rows, so between two removed rows the reads are contiguous as well: a
//               tile's sources lie in two or three source tiles when removals are sparse.  Bytes are copied, never re-rounded.
//   f32 rows:   rows [256 sl / nslices, 256 (sl + 1) / nslices) of the tile, one wave per row at a time, whole rows as 16-byte
//               loads and stores (32 KiB per workgroup at any dp: the tile's f32 rows are split evenly over its slices)
//   RowStat:    slice 0 only, one row per lane
// Destination rows j >= m are the padding of the last tile: zero image rows and zero stats, as the ingest writes them.
__global__ __launch_bounds__(256) void remove_gather_kernel(const float* __restrict__ src_f32, const uint4* __restrict__ src_img,
                                                            const RowStat* __restrict__ src_stat,
                                                            const uint32_t* __restrict__ rows, int64_t j0, int64_t m,
                                                            int32_t dp, float* __restrict__ stg_f32,
                                                            uint4* __restrict__ stg_img, RowStat* __restrict__ stg_stat) {
  const int32_t nslices = dp / SLICE_K;
  const int64_t t = blockIdx.x;
  const int32_t sl = (int32_t)blockIdx.y;
  const int64_t jt = j0 + t * TILE;                          // first destination row of the tile
  constexpr int64_t BLK = SLICE_ELEMS / 8;                   // uint4 per (tile, slice) block
  uint4* __restrict__ dblk = stg_img + (t * nslices + sl) * BLK;
  uint4 v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const uint32_t q = (uint32_t)u * 256u + threadIdx.x;
    const uint32_t r = q >> 2, p = q & 3u;
    const int64_t j = jt + r;
    v[u] = make_uint4(0, 0, 0, 0);
    if (j < m) {
      const int64_t i = rows[j];
      const uint32_t ri = (uint32_t)(i % TILE);
      const uint32_t c = swz_chunk(r, p);                    // logical chunk held by slot p of row r (the swizzle is an involution)
      v[u] = src_img[((i / TILE) * nslices + sl) * BLK + (int64_t)ri * 4 + swz_chunk(ri, c)];
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) dblk[u * 256 + threadIdx.x] = v[u];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int32_t r0 = (int32_t)((int64_t)TILE * sl / nslices), r1 = (int32_t)((int64_t)TILE * (sl + 1) / nslices);
  const int32_t nv = dp / 4;                                 // uint4 per f32 row
  for (int32_t r = r0 + wv; r < r1; r += 4) {
    const int64_t j = jt + r;
    if (j >= m) break;
    const int64_t i = rows[j];
    const uint4* __restrict__ sf = reinterpret_cast<const uint4*>(src_f32 + i * dp);
    uint4* __restrict__ df = reinterpret_cast<uint4*>(stg_f32 + (t * TILE + r) * dp);
    int p = lane;
    for (; p + 64 * (REMOVE_BATCH - 1) < nv; p += 64 * REMOVE_BATCH) {
      uint4 w[REMOVE_BATCH];
#pragma unroll
      for (int u = 0; u < REMOVE_BATCH; ++u) w[u] = sf[p + 64 * u];
      // every load of the batch is issued before its first store: left alone, hipcc sinks each load to its store and waits for it
#pragma unroll
      for (int u = 0; u < REMOVE_BATCH; u += 4)
        asm volatile("" : "+v"(w[u].x), "+v"(w[u].y), "+v"(w[u].z), "+v"(w[u].w), "+v"(w[u + 1].x), "+v"(w[u + 1].y),
                          "+v"(w[u + 1].z), "+v"(w[u + 1].w), "+v"(w[u + 2].x), "+v"(w[u + 2].y), "+v"(w[u + 2].z),
                          "+v"(w[u + 2].w), "+v"(w[u + 3].x), "+v"(w[u + 3].y), "+v"(w[u + 3].z), "+v"(w[u + 3].w));
#pragma unroll
      for (int u = 0; u < REMOVE_BATCH; ++u) df[p + 64 * u] = w[u];
    }
    for (; p < nv; p += 64) df[p] = sf[p];
  }
  if (sl == 0) {
    const int64_t j = jt + threadIdx.x;
    float a = 0.0f, b = 0.0f, c = 0.0f;
    if (j < m) {
      const RowStat st = src_stat[rows[j]];
      a = st.norm_f32, b = st.norm_img, c = st.norm_diff;
    }
    RowStat out;
    out.norm_f32 = a, out.norm_img = b, out.norm_diff = c;
    stg_stat[t * TILE + threadIdx.x] = out;
  }
}

// three contiguous runs of 16-byte words, copied by one grid (grid-stride over each run in turn)
__global__ __launch_bounds__(256) void remove_copy_kernel(const uint4* __restrict__ s0, uint4* __restrict__ d0, int64_t n0,
                                                          const uint4* __restrict__ s1, uint4* __restrict__ d1, int64_t n1,
                                                          const uint4* __restrict__ s2, uint4* __restrict__ d2, int64_t n2) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x;
  auto run = [&](const uint4* __restrict__ s, uint4* __restrict__ d, int64_t n) {
    int64_t p = first;
    for (; p + 3 * stride < n; p += 4 * stride) {
      const uint4 a = s[p], b = s[p + stride], c = s[p + 2 * stride], e = s[p + 3 * stride];
      d[p] = a, d[p + stride] = b, d[p + 2 * stride] = c, d[p + 3 * stride] = e;
    }
    for (; p < n; p += stride) d[p] = s[p];
  };
  run(s0, d0, n0);
  run(s1, d1, n1);
  run(s2, d2, n2);
}

void launch_remove_gather(const float* src_f32, const void* src_img, const RowStat* src_stat, const uint32_t* rows, int64_t j0,
                          int64_t j1_pad, int64_t m, int32_t dp, float* stg_f32, void* stg_img, RowStat* stg_stat,
                          hipStream_t stream) {
  const int64_t tiles = (j1_pad - j0) / TILE;
  if (tiles <= 0) return;
  hipLaunchKernelGGL(remove_gather_kernel, dim3((unsigned)tiles, (unsigned)(dp / SLICE_K)), dim3(256), 0, stream, src_f32,
                     (const uint4*)src_img, src_stat, rows, j0, m, dp, stg_f32, (uint4*)stg_img, stg_stat);
}

void launch_remove_writeback(const float* stg_f32, const void* stg_img, const RowStat* stg_stat, int64_t rows_f32,
                             int64_t rows_pad, int32_t dp, float* dst_f32, void* dst_img, RowStat* dst_stat,
                             hipStream_t stream) {
  if (rows_pad <= 0) return;
  const int64_t n0 = rows_f32 * dp / 4, n1 = rows_pad * dp / 8, n2 = rows_pad * (int64_t)sizeof(RowStat) / 16;
  const int64_t most = std::max(n0, n1);
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(8192, (most + 1023) / 1024));
  hipLaunchKernelGGL(remove_copy_kernel, dim3(blocks), dim3(256), 0, stream, (const uint4*)stg_f32, (uint4*)dst_f32, n0,
                     (const uint4*)stg_img, (uint4*)dst_img, n1, (const uint4*)stg_stat, (uint4*)dst_stat, n2);
}

}  // namespace mi
