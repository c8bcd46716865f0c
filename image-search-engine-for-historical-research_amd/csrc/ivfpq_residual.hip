// Residual encoding for the IVF index over PQ codes (api_ivfpq.hip): faiss IndexIVFPQ with by_residual = true, the
// form the reference's ANN uses (src/utils/knn.py:43-53).  A row's code quantizes r = double(x) - double(G[list(x)]), so a query has
// one distance table per PROBED LIST: T[q][p][m][c] = float32(sum_j (r_j - double(C[m][c][j]))^2) with r the query's residual
// against the list of probe slot p.  Layout, lists, probes, keys and the merge are those of ivfpq.hip, whose kernels stay as they are.
//
// The squared-distance chain, the ADC row sum, the encoder's tile constants, the slab of 4096 keys and its sort are pq_device.h's, shared with
// pq.hip and ivfpq.hip.
//
//   ivfr_table_kernel      grid = (groups of IVFR_RP probe slots, query), thread = codeword.  Per (book, slice of IVFR_PJ columns) the
//                          codebook slice passes through LDS as float32 (row padded to an odd stride, as ivf_probe_kernel's
//                          centroids) and the residual slices of the group's slots as float64, xs[j][slot]: a thread converts its
//                          codeword's column ONCE and spends it on IVFR_RP accumulators, whose residuals come from two 16-byte
//                          broadcast reads.  Slots holding -1 compute on zeros and write nothing; a group of nothing but -1 returns
//   ivfr_scan_select_kernel ivf_scan_select_kernel with the table inside the loop: a slab of 64 virtual blocks spans the block
//                          ranges of one or more probe slots; for each of them in turn the workgroup loads that slot's table into
//                          LDS and all waves scan that slot's blocks of the slab.  The loop bounds come from the prefix in LDS and
//                          are the same for every thread, so every barrier is met by the whole workgroup
//   ivfr_encode_kernel     pq_encode_kernel (pq.hip) on the residual against the row's OWN list: the argmin over c of the float64
//                          sum, ties to the lower c
//   ivfr_rows_kernel       float32(double(x) - double(G[list])), one rounding: what codebook training consumes
#include <algorithm>

#include "kernels.h"
#include "pq_device.h"

namespace mi {

constexpr int IVFR_THREADS = 512, IVFR_WAVES = IVFR_THREADS / 64;
constexpr int IVFR_TT = 256;                                                   // threads of the table kernel = codewords of a book
constexpr int IVFR_PJ = 32;                                                    // columns of a slice
constexpr int IVFR_RP = 4;                                                     // probe slots of a workgroup

// ---- table.  probes: the NORMALISED probes [nq][nprobe] (-1 = no list).  tab [nq][nprobe][M][Ks]
template <typename InT>
__global__ __launch_bounds__(IVFR_TT) void ivfr_table_kernel(const InT* __restrict__ x, int64_t rs, int64_t cs,
                                                            const float* __restrict__ G, int32_t d, const float* __restrict__ cb,
                                                            int32_t M, int32_t Ks, int32_t L, const int32_t* __restrict__ probes,
                                                            int32_t nprobe, float* __restrict__ tab) {
  __shared__ float cw[IVFR_TT][IVFR_PJ + 1];
  __shared__ __attribute__((aligned(16))) double xs[IVFR_PJ][IVFR_RP];
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.y;
  const int32_t p0 = (int32_t)blockIdx.x * IVFR_RP;
  int32_t lst[IVFR_RP];
  bool any = false;
#pragma unroll
  for (int r = 0; r < IVFR_RP; ++r) {
    lst[r] = p0 + r < nprobe ? probes[q * nprobe + p0 + r] : -1;
    any = any || lst[r] >= 0;
  }
  if (!any) return;                                        // uniform over the workgroup, ahead of every barrier
  const InT* xr = x + q * rs;
  for (int32_t m = 0; m < M; ++m) {
    double acc[IVFR_RP];
#pragma unroll
    for (int r = 0; r < IVFR_RP; ++r) acc[r] = 0.0;
    for (int32_t j0 = 0; j0 < L; j0 += IVFR_PJ) {
      const int32_t jn = min(IVFR_PJ, L - j0);
      __syncthreads();
      for (int i = tid; i < IVFR_TT * IVFR_PJ; i += IVFR_TT) {      // consecutive threads, consecutive columns of one codeword
        const int j = i % IVFR_PJ, c = i / IVFR_PJ;
        cw[c][j] = (j < jn && c < Ks) ? cb[((int64_t)m * Ks + c) * L + j0 + j] : 0.0f;
      }
      if (tid < IVFR_PJ * IVFR_RP) {
        const int j = tid / IVFR_RP, r = tid % IVFR_RP;
        int32_t l = -1;
#pragma unroll
        for (int rr = 0; rr < IVFR_RP; ++rr) l = rr == r ? lst[rr] : l;   // a select chain: lst stays in registers
        double v = 0.0;
        if (j < jn && l >= 0) {
          const int32_t col = m * L + j0 + j;
          v = (double)xr[(int64_t)col * cs] - (double)G[(int64_t)l * d + col];
        }
        xs[j][r] = v;
      }
      __syncthreads();
      if (tid < Ks)
        for (int32_t j = 0; j < jn; ++j) {
          const double c = (double)cw[tid][j];
#pragma unroll
          for (int r = 0; r < IVFR_RP; ++r) acc[r] = pq_sqdist_step(acc[r], xs[j][r], c);
        }
    }
    if (tid < Ks) {
#pragma unroll
      for (int r = 0; r < IVFR_RP; ++r)
        if (lst[r] >= 0) tab[(((int64_t)q * nprobe + p0 + r) * M + m) * Ks + tid] = (float)acc[r];
    }
  }
}

// ---- scan and select.  Dynamic LDS: keys [4096] u64 | table [4 MQ Ks] f32 | pref [nprobe + 1] | probes [nprobe]
__global__ __launch_bounds__(IVFR_THREADS) void ivfr_scan_select_kernel(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ rowid,
                                                                       const uint32_t* __restrict__ blk_table,
                                                                       const int32_t* __restrict__ list_off, int32_t M, int32_t MQ, int32_t Ks,
                                                                       const float* __restrict__ tab, const int32_t* __restrict__ probes,
                                                                       const int32_t* __restrict__ pref, int32_t nprobe,
                                                                       const uint32_t* __restrict__ list_rows,
                                                                       const uint64_t* __restrict__ allow, int32_t k, int32_t nslab,
                                                                       uint64_t* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char ivfr_smem[];
  const int64_t q = blockIdx.y;
  const int32_t slab = (int32_t)blockIdx.x;
  const int32_t* qpref = pref + q * (nprobe + 1);
  const int32_t total = qpref[nprobe];                                 // virtual blocks of this query
  // the merge reads only the slabs below the query's count, so nothing is written here.  The condition is uniform over the
  // workgroup and stands before every barrier: it must stay both
  if ((int64_t)slab * PQ_SLAB_BLOCKS >= total) return;
  uint64_t* keys = reinterpret_cast<uint64_t*>(ivfr_smem);
  float* tl = reinterpret_cast<float*>(ivfr_smem + PQ_SLAB_KEYS * 8);
  const int32_t ent = 4 * MQ * Ks, real = M * Ks;
  int32_t* lpref = reinterpret_cast<int32_t*>(tl + ent);
  int32_t* lprobe = lpref + nprobe + 1;
  const int tid = threadIdx.x;
  for (int32_t i = tid; i < PQ_SLAB_KEYS; i += IVFR_THREADS) keys[i] = PQ_SENTINEL;   // the slots no probe's range covers
  pq_slab_load_probes<IVFR_THREADS>(lpref, lprobe, qpref, probes + q * nprobe, nprobe, tid);
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const int32_t v0 = slab * PQ_SLAB_BLOCKS, v1 = min(total, v0 + PQ_SLAB_BLOCKS);
  // every value that steers this loop is read from LDS behind the barrier above or is a kernel argument: the trip count and the
  // branch around the body are the same for all 512 threads, and both barriers of the body are met by all of them
  for (int32_t p = 0; p < nprobe; ++p) {
    const int32_t a = max(v0, lpref[p]), b = min(v1, lpref[p + 1]);    // this slot's virtual blocks inside the slab
    if (a >= b) continue;                                              // an empty range (a -1 slot, an empty list) or another slab
    __syncthreads();                                                   // the waves have finished with the previous table
    pq_slab_load_table<IVFR_THREADS>(tl, tab + ((int64_t)q * nprobe + p) * real, ent, real, tid);
    __syncthreads();
    const int32_t l = lprobe[p];                                       // >= 0: its range is not empty
    const int32_t first = lpref[p];
    for (int32_t v = a + wave; v < b; v += IVFR_WAVES) {                // wave-uniform
      const int64_t blk = blk_table[list_off[l] + (v - first)];
      const bool filled = (uint32_t)(v - first) * 64u + (uint32_t)lane < list_rows[l];    // the tail block is partly filled
      const uint32_t row = rowid[blk * 64 + lane];
      const float dist = pq_adc_row<1>(tl, codes + blk * MQ * 64 + lane, MQ, Ks).v[0];
      if (pq_admit(filled, allow, row)) keys[(v - v0) * 64 + lane] = pq_key(dist, row);
    }
  }
  __syncthreads();
  pq_slab_select<IVFR_THREADS>(keys, part + ((int64_t)q * nslab + slab) * k, k, tid);
}

// ---- encoder: pq_encode_kernel's tiling (64 rows x one book, 4 codeword groups of 8 accumulators), the row slice replaced by
// the residual against the row's list.  Kept as a kernel of its own beside pq_encode_kernel: a shared body did not reproduce the
// device code of either (profiles/pq_helpers_isa.txt); the step of the sum and the PE_* tile constants are pq_device.h's
template <typename InT>
__global__ __launch_bounds__(256) void ivfr_encode_kernel(const InT* __restrict__ x, int64_t rs, int64_t cs, int64_t n,
                                                         const float* __restrict__ G, int32_t d, const uint8_t* __restrict__ lists,
                                                         const float* __restrict__ cb, int32_t M, int32_t Ks, int32_t L,
                                                         uint8_t* __restrict__ out) {
  __shared__ double xs[PE_JT][PE_ROWS];
  __shared__ double cw[PE_CT][PE_JT + 1];
  __shared__ double bd[4][PE_ROWS];
  __shared__ int32_t bc[4][PE_ROWS];
  __shared__ int32_t rl[PE_ROWS];
  const int tid = threadIdx.x, r = tid & 63, cg = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * PE_ROWS;
  const int32_t m = (int32_t)blockIdx.y;
  if (tid < PE_ROWS) rl[tid] = row0 + tid < n ? (int32_t)lists[row0 + tid] : 0;
  double best = __builtin_inf();
  int32_t best_c = 0;
  for (int32_t c0 = 0; c0 < Ks; c0 += PE_CT) {
    double acc[PE_PER];
#pragma unroll
    for (int e = 0; e < PE_PER; ++e) acc[e] = 0.0;
    for (int32_t j0 = 0; j0 < L; j0 += PE_JT) {
      const int32_t jn = min(PE_JT, L - j0);
      __syncthreads();
      for (int i = tid; i < PE_ROWS * PE_JT; i += 256) {
        const int j = i % PE_JT, rr = i / PE_JT;
        const int64_t row = row0 + rr;
        const int32_t col = m * L + j0 + j;
        xs[j][rr] = (j < jn && row < n) ? (double)x[row * rs + (int64_t)col * cs] - (double)G[(int64_t)rl[rr] * d + col] : 0.0;
      }
      for (int i = tid; i < PE_CT * PE_JT; i += 256) {
        const int j = i % PE_JT, cc = i / PE_JT;
        cw[cc][j] = (j < jn && c0 + cc < Ks) ? (double)cb[((int64_t)m * Ks + c0 + cc) * L + j0 + j] : 0.0;
      }
      __syncthreads();
      for (int32_t j = 0; j < jn; ++j) {
        const double xv = xs[j][r];
#pragma unroll
        for (int e = 0; e < PE_PER; ++e) acc[e] = pq_sqdist_step(acc[e], xv, cw[cg * PE_PER + e][j]);
      }
    }
#pragma unroll
    for (int e = 0; e < PE_PER; ++e) {
      const int32_t c = c0 + cg * PE_PER + e;
      if (c < Ks && acc[e] < best) {                              // ascending c, strict: ties stay with the lower c
        best = acc[e];
        best_c = c;
      }
    }
  }
  bd[cg][r] = best;
  bc[cg][r] = best_c;
  __syncthreads();
  if (tid < PE_ROWS && row0 + tid < n) {
    double b = bd[0][tid];
    int32_t c = bc[0][tid];
#pragma unroll
    for (int g = 1; g < 4; ++g) {
      const double v = bd[g][tid];
      const int32_t vc = bc[g][tid];
      if (v < b || (v == b && vc < c)) {
        b = v;
        c = vc;
      }
    }
    out[(row0 + tid) * M + m] = (uint8_t)c;
  }
}

// ---- residual rows: out [n][d] packed f32
template <typename InT>
__global__ __launch_bounds__(256) void ivfr_rows_kernel(const InT* __restrict__ x, int64_t rs, int64_t cs, int64_t n,
                                                       const float* __restrict__ G, int32_t d, const uint8_t* __restrict__ lists,
                                                       float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * d) return;
  const int64_t r = i / d;
  const int32_t c = (int32_t)(i % d);
  out[i] = (float)((double)x[r * rs + (int64_t)c * cs] - (double)G[(int64_t)lists[r] * d + c]);
}

// ---- launchers
void launch_ivfr_table(const void* x, int dtype, int64_t rs, int64_t cs, int32_t nq, const float* G, int32_t d, const float* cb, int32_t M,
                       int32_t Ks, int32_t L, const int32_t* probes, int32_t nprobe, float* tab, hipStream_t stream) {
  if (nq <= 0) return;
  const dim3 grid((unsigned)((nprobe + IVFR_RP - 1) / IVFR_RP), (unsigned)nq);
  if (dtype == 0)
    ivfr_table_kernel<float><<<grid, IVFR_TT, 0, stream>>>((const float*)x, rs, cs, G, d, cb, M, Ks, L, probes, nprobe, tab);
  else
    ivfr_table_kernel<double><<<grid, IVFR_TT, 0, stream>>>((const double*)x, rs, cs, G, d, cb, M, Ks, L, probes, nprobe, tab);
}

void launch_ivfr_scan_select(const uint32_t* codes, const uint32_t* rowid, const uint32_t* blk_table, const int32_t* list_off, int32_t M,
                             int32_t Ks, const float* tab, const int32_t* probes, const int32_t* pref, int32_t nprobe, int32_t nq,
                             const uint32_t* list_rows, const uint64_t* allow, int32_t k, int32_t nslab, uint64_t* part, hipStream_t stream) {
  if (nq <= 0 || nslab <= 0) return;
  const int32_t MQ = (M + 3) / 4;
  const int lds = PQ_SLAB_KEYS * 8 + 4 * MQ * Ks * 4 + (2 * nprobe + 1) * 4;
  ensure_dynamic_lds((const void*)ivfr_scan_select_kernel);
  ivfr_scan_select_kernel<<<dim3((unsigned)nslab, (unsigned)nq), IVFR_THREADS, lds, stream>>>(codes, rowid, blk_table, list_off, M, MQ, Ks, tab,
                                                                                             probes, pref, nprobe, list_rows, allow, k, nslab, part);
}

constexpr int64_t IVFR_STEP = (int64_t)1 << 22;               // rows per launch: grids stay below 2^31

void launch_ivfr_encode(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const float* G, int32_t d, const uint8_t* lists,
                        const float* cb, int32_t M, int32_t Ks, int32_t L, uint8_t* out, hipStream_t stream) {
  for (int64_t r = 0; r < n; r += IVFR_STEP) {
    const int64_t mm = std::min(IVFR_STEP, n - r);
    const dim3 grid((unsigned)((mm + PE_ROWS - 1) / PE_ROWS), (unsigned)M);
    if (dtype == 0)
      ivfr_encode_kernel<float><<<grid, 256, 0, stream>>>((const float*)x + r * rs, rs, cs, mm, G, d, lists + r, cb, M, Ks, L, out + r * M);
    else
      ivfr_encode_kernel<double><<<grid, 256, 0, stream>>>((const double*)x + r * rs, rs, cs, mm, G, d, lists + r, cb, M, Ks, L, out + r * M);
  }
}

void launch_ivfr_rows(const void* x, int dtype, int64_t rs, int64_t cs, int64_t n, const float* G, int32_t d, const uint8_t* lists, float* out,
                      hipStream_t stream) {
  const int64_t step = std::max<int64_t>(1, ((int64_t)1 << 30) / d);
  for (int64_t r = 0; r < n; r += step) {
    const int64_t mm = std::min(step, n - r);
    const dim3 grid((unsigned)((mm * d + 255) / 256));
    if (dtype == 0) ivfr_rows_kernel<float><<<grid, 256, 0, stream>>>((const float*)x + r * rs, rs, cs, mm, G, d, lists + r, out + r * d);
    else ivfr_rows_kernel<double><<<grid, 256, 0, stream>>>((const double*)x + r * rs, rs, cs, mm, G, d, lists + r, out + r * d);
  }
}

}  // namespace mi
