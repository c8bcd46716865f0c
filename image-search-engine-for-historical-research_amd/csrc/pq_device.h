// The device code the PQ index family shares (pq.hip, pq_wide.hip, ivfpq.hip, ivfpq_residual.hip): every
// codebook, table, probe, code and partial list of these files is made of these pieces, so each exists once and all of them give the
// same bits.
//
//   pq_sqdist_step / pq_sqdist  THE arithmetic of a squared distance: float64 subtract, multiply, add, nothing fused
//   pq_pack_dword               the codes of a row (bytes: 4 w .. 4 w + 3, uint16: 2 w, 2 w + 1) -> a dword of the transposed layout
//   PE_*                        the tile constants of the two encoder kernels
//   pq_adc_row                  the ADC sum of one lane's row: float32 table entries in ascending book order
//   the slab vocabulary         an IVF query's candidates pass in slabs of 64 blocks = 4096 keys float_bits(dist) << 32 | local row,
//                               all ones = no candidate; prologue, admit test and the sort-and-write epilogue of the two
//                               scan-and-select kernels, and the sort the merge shares with them
#pragma once
#include "common.h"

namespace mi {

// ---- the one place the squared distance of a sub-vector is computed: one term of sum_j (x_j - c_j)^2 in float64.  fp contraction
// is off: hipcc would otherwise fuse d * d + acc
__device__ __forceinline__ double pq_sqdist_step(double acc, double x, double c) {
#pragma clang fp contract(off)
  const double d = x - c;
  const double p = d * d;
  return acc + p;
}

// the whole chain, ascending j
template <typename FX, typename FC>
__device__ __forceinline__ double pq_sqdist(FX x, FC c, int32_t L) {
  double acc = 0.0;
  for (int32_t j = 0; j < L; ++j) acc = pq_sqdist_step(acc, x(j), c(j));
  return acc;
}

// ---- the dword w of a row's code, PER = 4 (bytes) or 2 (uint16) books to a dword: field b is the code in book PER w + b, the
// fields of the books M .. are zero
template <typename CodeT>
__device__ __forceinline__ uint32_t pq_pack_dword(const CodeT* p, int32_t w, int32_t M) {
  constexpr int PER = 4 / (int)sizeof(CodeT), BITS = 8 * (int)sizeof(CodeT);
  uint32_t v = 0;
#pragma unroll
  for (int b = 0; b < PER; ++b)
    if (PER * w + b < M) v |= (uint32_t)p[PER * w + b] << (BITS * b);
  return v;
}

// ---- the encoder's tiling (pq_encode_kernel in pq.hip, ivfr_encode_kernel in ivfpq_residual.hip): 64 rows x one book to a workgroup,
// codewords in tiles of PE_CT (PE_PER per thread), columns in slices of PE_JT
constexpr int PE_ROWS = 64, PE_CT = 32, PE_JT = 64, PE_PER = PE_CT / 4;

// ---- the ADC sum.  tv: the LDS image of the tables of QT queries interleaved query-fastest, T[m][c][QT], 4 MQ books of Ks entries
// (the entries of the books M .. 4 MQ - 1 are +0.0 and the code bytes of those books are 0, so a whole dword of codes is walked
// without a branch and the extra adds change nothing: the running sum is never -0.0, it starts at +0.0 and takes non-negative
// terms).  src: the lane's dword 0 of its block, codes + (block MQ) 64 + lane.  Per (row, book) ONE LDS read of 4 QT bytes
template <int QT> struct PqVec;
template <> struct PqVec<1> { using type = float; };
template <> struct PqVec<2> { using type = float2; };
template <> struct PqVec<4> { using type = float4; };

template <int QT>
__device__ __forceinline__ void pq_acc(float (&acc)[QT], const typename PqVec<QT>::type v);
template <> __device__ __forceinline__ void pq_acc<1>(float (&acc)[1], const float v) { acc[0] = acc[0] + v; }
template <> __device__ __forceinline__ void pq_acc<2>(float (&acc)[2], const float2 v) {
  acc[0] = acc[0] + v.x;
  acc[1] = acc[1] + v.y;
}
template <> __device__ __forceinline__ void pq_acc<4>(float (&acc)[4], const float4 v) {
  acc[0] = acc[0] + v.x;
  acc[1] = acc[1] + v.y;
  acc[2] = acc[2] + v.z;
  acc[3] = acc[3] + v.w;
}

template <int QT> struct PqSums { float v[QT]; };

template <int QT>
__device__ __forceinline__ PqSums<QT> pq_adc_row(const typename PqVec<QT>::type* tv, const uint32_t* src, int32_t MQ, int32_t Ks) {
  PqSums<QT> acc;
#pragma unroll
  for (int t = 0; t < QT; ++t) acc.v[t] = 0.0f;
#pragma unroll 4
  for (int32_t w = 0; w < MQ; ++w) {
    const uint32_t g = src[(int64_t)w * 64];
    const int32_t base = 4 * w * Ks;
    pq_acc<QT>(acc.v, tv[base + (int32_t)(g & 255u)]);
    pq_acc<QT>(acc.v, tv[base + Ks + (int32_t)((g >> 8) & 255u)]);
    pq_acc<QT>(acc.v, tv[base + 2 * Ks + (int32_t)((g >> 16) & 255u)]);
    pq_acc<QT>(acc.v, tv[base + 3 * Ks + (int32_t)(g >> 24)]);
  }
  return acc;
}

// ---- slabs and keys of the IVF search.  Distances are >= +0.0, so the bit pattern is monotone and +inf an ordinary value; keys
// are distinct, there is no tie class
constexpr int PQ_SLAB_BLOCKS = 64, PQ_SLAB_KEYS = PQ_SLAB_BLOCKS * 64;         // 4096 candidates of a workgroup
constexpr uint64_t PQ_SENTINEL = ~0ull;                                        // no candidate: above every key

__device__ __forceinline__ uint64_t pq_key(float dist, uint32_t row) { return ((uint64_t)__float_as_uint(dist) << 32) | row; }
__device__ __forceinline__ uint32_t pq_key_row(uint64_t key) { return (uint32_t)key; }
__device__ __forceinline__ float pq_key_dist(uint64_t key) { return __uint_as_float((uint32_t)(key >> 32)); }

// ascending bitonic sort of 4096 keys in LDS by NT threads; ends with a barrier
template <int NT>
__device__ __forceinline__ void pq_sort4096(uint64_t* keys, int tid) {
  for (int k = 2; k <= PQ_SLAB_KEYS; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int t = tid; t < PQ_SLAB_KEYS / 2; t += NT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int p = i | j;
        const uint64_t a = keys[i], b = keys[p];
        const bool up = (i & k) == 0;
        if ((a > b) == up) {
          keys[i] = b;
          keys[p] = a;
        }
      }
      __syncthreads();
    }
  }
}

// prologue: the query's prefix of block counts and its normalised probes -> LDS (no barrier here)
template <int NT>
__device__ __forceinline__ void pq_slab_load_probes(int32_t* lpref, int32_t* lprobe, const int32_t* qpref, const int32_t* qprobes,
                                                    int32_t nprobe, int tid) {
  for (int32_t i = tid; i <= nprobe; i += NT) lpref[i] = qpref[i];
  for (int32_t i = tid; i < nprobe; i += NT) lprobe[i] = qprobes[i];
}

// one table of `real` = M Ks entries -> the LDS image of ent = 4 MQ Ks entries, zeros for the books beyond M (no barrier here)
template <int NT>
__device__ __forceinline__ void pq_slab_load_table(float* tl, const float* qt, int32_t ent, int32_t real, int tid) {
  for (int32_t i = tid; i < ent; i += NT) tl[i] = i < real ? qt[i] : 0.0f;
}

// the admit test: the slot lies below its list's fill and the allow bitmap, if any, has the row's bit
__device__ __forceinline__ bool pq_admit(bool filled, const uint64_t* allow, uint32_t row) {
  bool ok = filled;
  if (ok && allow) ok = (allow[row >> 6] >> (row & 63u)) & 1ull;
  return ok;
}

// epilogue, entered behind a barrier: the slab's keys sorted, the first k -> out
template <int NT>
__device__ __forceinline__ void pq_slab_select(uint64_t* keys, uint64_t* out, int32_t k, int tid) {
  pq_sort4096<NT>(keys, tid);
  for (int32_t i = tid; i < k; i += NT) out[i] = keys[i];
}

}  // namespace mi
