// Kernels of the in-place row removal of the PQ and the IVF-PQ index (mi_pq_remove_rows, api_pq.hip; mi_ivfpq_remove_rows,
// api_ivfpq.hip).  They only move memory: a code's dwords (codes[block][MQ][64], one dword column per lane) and,
// on the IVF handle, rowid[block][64].  Nothing is re-encoded.  Both read the same two host-made arrays:
//   keep    [ceil(n / 64)] the bitmap of the rows that STAY (bits at or beyond n clear)
//   prefix  [ceil(n / 64) + 1] the exclusive count of keep bits per word, prefix[last] = n'
// so the new local row of a survivor r is prefix[r >> 6] + popcount(keep[r >> 6] below bit r & 63).
//
//   pq_remove_gather_kernel     flat index: a wave takes one source block of 64 rows = one bitmap word, reads its MQ dword columns
//                               (256 contiguous bytes each) and writes the survivors' dwords to the staging area at their new
//                               position (the ballot / prefix idiom of pq_train.hip and hamming.hip, with the ballot read from
//                               the bitmap word).  The staging area has the index's own block layout, shifted so that its block 0
//                               is the destination block of the chunk's first survivor: the write-back is then a plain copy
//   pq_remove_writeback_kernel  staging -> codes, thread = dword, only the positions [lo, hi) of the chunk's survivors (the lanes
//                               below lo hold earlier chunks' final rows, the lanes from hi on later chunks' unread sources)
//   ivf_remove_kernel           IVF index: ONE workgroup per list, four waves, four blocks of the chain per step.  Every wave
//                               loads its block whole (MQ dword columns + row ids) and WAITS for the loads, then the barrier:
//                               the destinations of a step lie in the chain at or before the step's own blocks (a survivor
//                               never moves up), so they can be blocks another wave of the step has just read, never a block a
//                               later step has yet to read.  Survivors go to the chain's running fill with the row id
//                               rewritten.  Lists own disjoint blocks: no atomics, no grid barrier, no staging
// None uses scratch; LDS: 32 bytes in ivf_remove_kernel.  Slots the survivors vacate keep their old bytes: a slot at or beyond
// a list's fill (a row at or beyond n) is never admitted by a scan and is overwritten by the next append.
#include "kernels.h"

namespace mi {

constexpr int PQR_MAX_MQ = 16;        // dwords of a code: M <= 64 books, four to a dword
constexpr int IVR_WAVES = 4;

__global__ __launch_bounds__(256) void pq_remove_gather_kernel(const uint32_t* __restrict__ codes, int32_t MQ,
                                                              const uint64_t* __restrict__ keep, const uint32_t* __restrict__ prefix,
                                                              int64_t blk0, int64_t blk1, int64_t dst_blk0,
                                                              uint32_t* __restrict__ stg) {
  const int lane = threadIdx.x & 63;
  const int64_t b = blk0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // source block = bitmap word, wave-uniform
  if (b >= blk1) return;
  const uint64_t kw = keep[b];
  if (kw == 0) return;
  const bool stay = (kw >> lane) & 1ull;
  const int64_t s = (int64_t)prefix[b] + __popcll(kw & ((1ull << lane) - 1ull)) - dst_blk0 * 64;   // position in the staging area
  const uint32_t* __restrict__ src = codes + b * MQ * 64 + lane;
  uint32_t* __restrict__ dst = stg + (s >> 6) * MQ * 64 + (s & 63);
  uint32_t v[PQR_MAX_MQ];
#pragma unroll
  for (int w = 0; w < PQR_MAX_MQ; ++w)
    if (w < MQ) v[w] = src[w * 64];
  if (stay) {
#pragma unroll
    for (int w = 0; w < PQR_MAX_MQ; ++w)
      if (w < MQ) dst[w * 64] = v[w];
  }
}

// dword i of the staging area (block i / (64 MQ), lane i & 63) -> the same dword of the blocks from dst_blk0 on
__global__ __launch_bounds__(256) void pq_remove_writeback_kernel(const uint32_t* __restrict__ stg, int32_t MQ, int64_t dwords,
                                                                 int64_t lo, int64_t hi, uint32_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= dwords) return;
  const int64_t s = i / (64 * MQ) * 64 + (i & 63);
  if (s >= lo && s < hi) dst[i] = stg[i];
}

// codes and rowid are read and written through the same pointers on purpose (in place): no __restrict__ on them
__global__ __launch_bounds__(64 * IVR_WAVES) void ivf_remove_kernel(uint32_t* codes, uint32_t* rowid,
                                                                   const uint32_t* __restrict__ blk_table,
                                                                   const int32_t* __restrict__ list_off,
                                                                   const uint32_t* __restrict__ list_rows, int32_t MQ,
                                                                   const uint64_t* __restrict__ keep,
                                                                   const uint32_t* __restrict__ prefix) {
  __shared__ uint32_t cnt[2][IVR_WAVES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int32_t l = (int32_t)blockIdx.x;
  const uint32_t* __restrict__ chain = blk_table + list_off[l];
  const int32_t nb = list_off[l + 1] - list_off[l];
  const uint32_t rows = list_rows[l];                  // the chain's old fill
  uint32_t fill = 0;                                    // the chain's new fill so far (the same in every wave)
  for (int32_t b0 = 0, step = 0; b0 < nb; b0 += IVR_WAVES, ++step) {       // uniform over the workgroup: every wave meets the barrier
    const int32_t b = b0 + wv;
    const uint32_t slot = (uint32_t)b * 64u + (uint32_t)lane;               // position along the chain
    const bool filled = b < nb && slot < rows;
    uint32_t v[PQR_MAX_MQ];
#pragma unroll
    for (int w = 0; w < PQR_MAX_MQ; ++w) v[w] = 0u;
    uint32_t id = 0, nid = 0;
    bool stay = false;
    if (b < nb) {
      const int64_t pb = chain[b];
      const uint32_t* src = codes + pb * MQ * 64 + lane;
#pragma unroll
      for (int w = 0; w < PQR_MAX_MQ; ++w)
        if (w < MQ) v[w] = src[w * 64];
      if (filled) {                                     // a slot beyond the fill has no row id to look up
        id = rowid[pb * 64 + lane];
        const uint64_t kw = keep[id >> 6];
        stay = (kw >> (id & 63u)) & 1ull;
        nid = prefix[id >> 6] + (uint32_t)__popcll(kw & ((1ull << (id & 63u)) - 1ull));
      }
    }
    const unsigned long long mask = __ballot(stay);
    if (lane == 0) cnt[step & 1][wv] = (uint32_t)__popcll(mask);
    // every value of the block is in its register before the barrier: a load still in flight behind it could read what
    // another wave of this step has stored by then
#pragma unroll
    for (int w = 0; w < PQR_MAX_MQ; ++w)
      if (w < MQ) asm volatile("" : "+v"(v[w]));
    asm volatile("" : "+v"(id));
    __syncthreads();
    uint32_t base = fill;
#pragma unroll
    for (int u = 0; u < IVR_WAVES; ++u) {
      const uint32_t c = cnt[step & 1][u];
      if (u < wv) base += c;
      fill += c;
    }
    if (stay) {
      const uint32_t p = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (p != slot) {                                  // p == slot: nothing left the chain before this row, it stays where it is
        const int64_t pd = chain[p >> 6];
        uint32_t* dst = codes + pd * MQ * 64 + (p & 63u);
#pragma unroll
        for (int w = 0; w < PQR_MAX_MQ; ++w)
          if (w < MQ) dst[w * 64] = v[w];
      }
      if (p != slot || nid != id) rowid[(int64_t)chain[p >> 6] * 64 + (p & 63u)] = nid;
    }
    // cnt[step & 1] is written again two steps on, behind the next step's barrier, which this wave reaches after these reads
  }
}

void launch_pq_remove_gather(const uint32_t* codes, int32_t M, const uint64_t* keep, const uint32_t* prefix, int64_t blk0, int64_t blk1,
                             int64_t dst_blk0, uint32_t* stg, hipStream_t stream) {
  if (blk1 <= blk0) return;
  pq_remove_gather_kernel<<<dim3((unsigned)((blk1 - blk0 + 3) / 4)), 256, 0, stream>>>(codes, (M + 3) / 4, keep, prefix, blk0, blk1, dst_blk0,
                                                                                       stg);
}

void launch_pq_remove_writeback(const uint32_t* stg, int32_t M, int64_t dst_blk0, int64_t lo, int64_t hi, uint32_t* codes,
                                hipStream_t stream) {
  if (hi <= lo) return;
  const int32_t MQ = (M + 3) / 4;
  const int64_t dwords = (hi + 63) / 64 * MQ * 64;
  pq_remove_writeback_kernel<<<dim3((unsigned)((dwords + 255) / 256)), 256, 0, stream>>>(stg, MQ, dwords, lo, hi, codes + dst_blk0 * MQ * 64);
}

void launch_ivf_remove(uint32_t* codes, uint32_t* rowid, const uint32_t* blk_table, const int32_t* list_off, const uint32_t* list_rows,
                       int32_t nlist, int32_t M, const uint64_t* keep, const uint32_t* prefix, hipStream_t stream) {
  ivf_remove_kernel<<<dim3((unsigned)nlist), 64 * IVR_WAVES, 0, stream>>>(codes, rowid, blk_table, list_off, list_rows, (M + 3) / 4, keep,
                                                                         prefix);
}

}  // namespace mi
