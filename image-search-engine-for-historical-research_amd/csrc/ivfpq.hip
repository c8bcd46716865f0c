// Inverted-file search over PQ codes (api_ivfpq.hip): the reference's matching_PQ_Net_bucket
// (src/utils/nnsearch.py:949-998), faiss IndexIVFPQ with by_residual = false.  A query scans only the rows whose list is one of
// its probed lists; distances, arithmetic and order are those of pq.hip (float32 table sums in book order, (distance, id)).
//
// Layout: physical blocks of 64 slots from one pool.  codes[pblock][MQ][64] dwords is the PQ index's transposed block (four books
// to a dword, one book-quad of 64 rows is one coalesced 256-byte read), rowid[pblock][64] the local row of a slot.  A list is
// a chain of blocks: blk_table[list_off[l] .. list_off[l + 1]) are its block numbers, in no particular order in the pool (appends
// interleave the blocks of different lists); its first list_rows[l] slots, counted along the chain, are filled.
//
// The squared-distance chain, the ADC row sum, the code dword, the slab of 4096 keys and its sort are pq_device.h's, shared with
// pq.hip and ivfpq_residual.hip.
//
//   ivf_probe_kernel        workgroup = query, thread = list: float64 distance (pq_sqdist_step) to every coarse centroid, rank of a list = number
//                           of lists with a smaller (value, id), lists of rank < nprobe written at their rank
//   ivf_prefix_kernel       workgroup = query: normalises a probe row (entries outside [0, nlist) and repeats of an earlier
//                           entry become -1) and writes the prefix of block counts over it: the query's virtual block sequence
//   ivf_scatter_kernel      code bytes and row ids -> the slots the host computed
//   ivf_check_kernel        list ids >= nlist raise the flag (device-resident list ids)
//   ivf_scan_select_kernel  the hot path.  Grid = (slab of 64 virtual blocks, query), 512 threads.  ONE query's table in LDS,
//                           T[m][c]; every wave walks 8 blocks as pq_scan_kernel does (pq_adc_row); key = pq_key(dist, local row);
//                           slots beyond a list's fill and rows the allow bitmap clears get the all-ones sentinel; the 4096 keys are
//                           bitonic-sorted in LDS and the first k written to part[query][slab][k]
//   ivf_merge_kernel        workgroup = query: the sorted partial lists of its slabs -> the k smallest keys in order (keeps the
//                           best 2048 and folds in 2048 new keys per bitonic sort of 4096), then ids and distances
#include <algorithm>

#include "kernels.h"
#include "pq_device.h"

namespace mi {

constexpr int IVF_THREADS = 512, IVF_WAVES = IVF_THREADS / 64;
constexpr int IVF_MAX_LISTS = 256;
constexpr int IVF_PJ = 32;                                                     // columns of a probe slice

// ---- probe.  gs[l][j] holds a slice of IVF_PJ columns of every centroid (row padded to an odd stride: lane l reads bank
// (33 l + j) % 64, no conflict), xs[j] the query's slice in float64 (one address per wave, a broadcast)
template <typename InT>
__global__ __launch_bounds__(IVF_MAX_LISTS) void ivf_probe_kernel(const InT* __restrict__ x, int64_t rs, int64_t cs,
                                                                 const float* __restrict__ G, int32_t nlist, int32_t d, int32_t nprobe,
                                                                 int32_t* __restrict__ out) {
  __shared__ float gs[IVF_MAX_LISTS][IVF_PJ + 1];
  __shared__ double xs[IVF_PJ];
  __shared__ double dist[IVF_MAX_LISTS];
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const InT* xr = x + q * rs;
  double acc = 0.0;
  for (int32_t j0 = 0; j0 < d; j0 += IVF_PJ) {
    const int32_t jn = min(IVF_PJ, d - j0);
    __syncthreads();
    for (int i = tid; i < nlist * IVF_PJ; i += IVF_MAX_LISTS) {
      const int j = i % IVF_PJ, l = i / IVF_PJ;
      gs[l][j] = j < jn ? G[(int64_t)l * d + j0 + j] : 0.0f;
    }
    if (tid < IVF_PJ) xs[tid] = tid < jn ? (double)xr[(int64_t)(j0 + tid) * cs] : 0.0;
    __syncthreads();
    if (tid < nlist)
      for (int32_t j = 0; j < jn; ++j) acc = pq_sqdist_step(acc, xs[j], (double)gs[tid][j]);
  }
  dist[tid] = acc;
  if (tid < nprobe) out[q * nprobe + tid] = -1;           // a non-finite query may leave ranks unused: those stay "no list"
  __syncthreads();
  if (tid < nlist) {
    int32_t rank = 0;
    for (int32_t l = 0; l < nlist; ++l) {
      const double v = dist[l];
      rank += (v < acc || (v == acc && l < tid)) ? 1 : 0;
    }
    if (rank < nprobe) out[q * nprobe + rank] = tid;
  }
}

// ---- probes in [nq][nprobe] (library-chosen or the caller's) -> norm [nq][nprobe] (-1 = no list), pref [nq][nprobe + 1]
__global__ __launch_bounds__(IVF_MAX_LISTS) void ivf_prefix_kernel(const int32_t* __restrict__ in, int32_t nlist, int32_t nprobe,
                                                                  const int32_t* __restrict__ list_off, int32_t* __restrict__ norm,
                                                                  int32_t* __restrict__ pref) {
  __shared__ int32_t p[IVF_MAX_LISTS];
  __shared__ int32_t cnt[IVF_MAX_LISTS];
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  int32_t v = -1;
  if (tid < nprobe) {
    v = in[q * nprobe + tid];
    if (v < 0 || v >= nlist) v = -1;
  }
  p[tid] = v;
  __syncthreads();
  if (v >= 0)
    for (int i = 0; i < tid; ++i)
      if (p[i] == v) {
        v = -1;
        break;
      }
  cnt[tid] = v >= 0 ? list_off[v + 1] - list_off[v] : 0;
  if (tid < nprobe) norm[q * nprobe + tid] = v;
  __syncthreads();
  if (tid == 0) {
    int32_t s = 0;
    int32_t* o = pref + q * (nprobe + 1);
    o[0] = 0;
    for (int i = 0; i < nprobe; ++i) {
      s += cnt[i];
      o[i + 1] = s;
    }
  }
}

// ---- list ids >= nlist raise the flag
__global__ __launch_bounds__(256) void ivf_check_kernel(const uint8_t* __restrict__ ids, int32_t nlist, int64_t m, uint32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < m && (int32_t)ids[i] >= nlist) *flag = 1u;
}

// ---- code bytes [m][stride] -> dwords at the slots slot[r] (thread = (dword, row), rows fastest); dword 0's thread writes the id
__global__ __launch_bounds__(256) void ivf_scatter_kernel(const uint8_t* __restrict__ src, int64_t stride, int32_t M, int32_t MQ,
                                                         const int64_t* __restrict__ slot, int64_t row0, int64_t m,
                                                         uint32_t* __restrict__ codes, uint32_t* __restrict__ rowid) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m * MQ) return;
  const int64_t r = i % m;
  const int32_t w = (int32_t)(i / m);
  const uint32_t v = pq_pack_dword(src + r * stride, w, M);
  const int64_t s = slot[r];
  codes[((s >> 6) * MQ + w) * 64 + (s & 63)] = v;
  if (w == 0) rowid[s] = (uint32_t)(row0 + r);
}

// ---- scan and select.  Dynamic LDS: keys [4096] u64 | table [4 MQ Ks] f32 | pref [nprobe + 1] | probes [nprobe]
__global__ __launch_bounds__(IVF_THREADS) void ivf_scan_select_kernel(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ rowid,
                                                                     const uint32_t* __restrict__ blk_table,
                                                                     const int32_t* __restrict__ list_off, int32_t M, int32_t MQ, int32_t Ks,
                                                                     const float* __restrict__ tab, const int32_t* __restrict__ probes,
                                                                     const int32_t* __restrict__ pref, int32_t nprobe,
                                                                     const uint32_t* __restrict__ list_rows,
                                                                     const uint64_t* __restrict__ allow, int32_t k, int32_t nslab,
                                                                     uint64_t* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char ivf_smem[];
  const int64_t q = blockIdx.y;
  const int32_t slab = (int32_t)blockIdx.x;
  const int32_t* qpref = pref + q * (nprobe + 1);
  const int32_t total = qpref[nprobe];                                 // virtual blocks of this query
  // the merge reads only the slabs below the query's count, so nothing is written here.  The condition is uniform over the
  // workgroup and stands before every barrier: it must stay both
  if ((int64_t)slab * PQ_SLAB_BLOCKS >= total) return;
  uint64_t* keys = reinterpret_cast<uint64_t*>(ivf_smem);
  float* tl = reinterpret_cast<float*>(ivf_smem + PQ_SLAB_KEYS * 8);
  const int32_t ent = 4 * MQ * Ks, real = M * Ks;
  int32_t* lpref = reinterpret_cast<int32_t*>(tl + ent);
  int32_t* lprobe = lpref + nprobe + 1;
  const int tid = threadIdx.x;
  pq_slab_load_table<IVF_THREADS>(tl, tab + q * real, ent, real, tid);
  pq_slab_load_probes<IVF_THREADS>(lpref, lprobe, qpref, probes + q * nprobe, nprobe, tid);
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  for (int32_t vb = wave; vb < PQ_SLAB_BLOCKS; vb += IVF_WAVES) {      // wave-uniform
    const int32_t v = slab * PQ_SLAB_BLOCKS + vb;
    uint64_t key = PQ_SENTINEL;
    if (v < total) {
      // the probe whose range [pref[i], pref[i + 1]) holds v: the last i with pref[i] <= v (empty probes have empty ranges)
      int32_t lo = 0, hi = nprobe - 1;
      while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (lpref[mid] <= v) lo = mid;
        else hi = mid - 1;
      }
      const int32_t l = lprobe[lo];                                     // >= 0: its range is not empty
      const int64_t b = blk_table[list_off[l] + (v - lpref[lo])];
      const bool filled = (uint32_t)(v - lpref[lo]) * 64u + (uint32_t)lane < list_rows[l];   // the tail block is partly filled
      const uint32_t row = rowid[b * 64 + lane];
      const float dist = pq_adc_row<1>(tl, codes + b * MQ * 64 + lane, MQ, Ks).v[0];
      if (pq_admit(filled, allow, row)) key = pq_key(dist, row);
    }
    keys[vb * 64 + lane] = key;
  }
  __syncthreads();
  pq_slab_select<IVF_THREADS>(keys, part + ((int64_t)q * nslab + slab) * k, k, tid);
}

// ---- merge: LDS keys [4096]; [0, 2048) is the best so far (sorted after every pass), [2048, 4096) takes the next 2048 keys of
// the query's partial lists read as one stream of slabs * k keys
__global__ __launch_bounds__(IVF_THREADS) void ivf_merge_kernel(const uint64_t* __restrict__ part, const int32_t* __restrict__ pref,
                                                               int32_t nprobe, int32_t k, int32_t nslab, int64_t row_offset,
                                                               int64_t* __restrict__ out_idx, float* __restrict__ out_dist) {
  __shared__ uint64_t keys[PQ_SLAB_KEYS];
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x;
  const int32_t total = pref[q * (nprobe + 1) + nprobe];
  const int32_t slabs = min(nslab, (total + PQ_SLAB_BLOCKS - 1) / PQ_SLAB_BLOCKS);
  const int64_t count = (int64_t)slabs * k;
  const uint64_t* src = part + (int64_t)q * nslab * k;
  constexpr int HALF = PQ_SLAB_KEYS / 2;
  for (int i = tid; i < HALF; i += IVF_THREADS) keys[i] = PQ_SENTINEL;
  for (int64_t c0 = 0; c0 < count; c0 += HALF) {
    for (int i = tid; i < HALF; i += IVF_THREADS) keys[HALF + i] = c0 + i < count ? src[c0 + i] : PQ_SENTINEL;
    __syncthreads();
    pq_sort4096<IVF_THREADS>(keys, tid);
  }
  __syncthreads();
  for (int32_t i = tid; i < k; i += IVF_THREADS) {
    const uint64_t key = keys[i];
    const bool none = key == PQ_SENTINEL;
    out_idx[q * k + i] = none ? -1 : row_offset + (int64_t)pq_key_row(key);
    if (out_dist) out_dist[q * k + i] = none ? __builtin_inff() : pq_key_dist(key);
  }
}

// ---- launchers
void launch_ivf_probe(const void* x, int dtype, int64_t rs, int64_t cs, int64_t nq, const float* G, int32_t nlist, int32_t d,
                      int32_t nprobe, int32_t* out, hipStream_t stream) {
  if (nq <= 0) return;
  if (dtype == 0)
    ivf_probe_kernel<float><<<dim3((unsigned)nq), IVF_MAX_LISTS, 0, stream>>>((const float*)x, rs, cs, G, nlist, d, nprobe, out);
  else
    ivf_probe_kernel<double><<<dim3((unsigned)nq), IVF_MAX_LISTS, 0, stream>>>((const double*)x, rs, cs, G, nlist, d, nprobe, out);
}

void launch_ivf_prefix(const int32_t* in, int64_t nq, int32_t nlist, int32_t nprobe, const int32_t* list_off, int32_t* norm,
                       int32_t* pref, hipStream_t stream) {
  if (nq <= 0) return;
  ivf_prefix_kernel<<<dim3((unsigned)nq), IVF_MAX_LISTS, 0, stream>>>(in, nlist, nprobe, list_off, norm, pref);
}

void launch_ivf_check(const uint8_t* ids, int32_t nlist, int64_t m, uint32_t* flag, hipStream_t stream) {
  constexpr int64_t step = (int64_t)1 << 30;
  for (int64_t r = 0; r < m; r += step) {
    const int64_t mm = std::min(step, m - r);
    ivf_check_kernel<<<dim3((unsigned)((mm + 255) / 256)), 256, 0, stream>>>(ids + r, nlist, mm, flag);
  }
}

void launch_ivf_scatter(const uint8_t* src, int64_t stride, int32_t M, const int64_t* slot, int64_t row0, int64_t m, uint32_t* codes,
                        uint32_t* rowid, hipStream_t stream) {
  if (m <= 0) return;
  const int32_t MQ = (M + 3) / 4;
  ivf_scatter_kernel<<<dim3((unsigned)((m * MQ + 255) / 256)), 256, 0, stream>>>(src, stride, M, MQ, slot, row0, m, codes, rowid);
}

void launch_ivf_scan_select(const uint32_t* codes, const uint32_t* rowid, const uint32_t* blk_table, const int32_t* list_off, int32_t M,
                            int32_t Ks, const float* tab, const int32_t* probes, const int32_t* pref, int32_t nprobe, int32_t nq,
                            const uint32_t* list_rows, const uint64_t* allow, int32_t k, int32_t nslab, uint64_t* part, hipStream_t stream) {
  if (nq <= 0 || nslab <= 0) return;
  const int32_t MQ = (M + 3) / 4;
  const int lds = PQ_SLAB_KEYS * 8 + 4 * MQ * Ks * 4 + (2 * nprobe + 1) * 4;
  ensure_dynamic_lds((const void*)ivf_scan_select_kernel);
  ivf_scan_select_kernel<<<dim3((unsigned)nslab, (unsigned)nq), IVF_THREADS, lds, stream>>>(codes, rowid, blk_table, list_off, M, MQ, Ks, tab,
                                                                                            probes, pref, nprobe, list_rows, allow, k, nslab, part);
}

void launch_ivf_merge(const uint64_t* part, const int32_t* pref, int32_t nprobe, int64_t nq, int32_t k, int32_t nslab, int64_t row_offset,
                      int64_t* out_idx, float* out_dist, hipStream_t stream) {
  if (nq <= 0) return;
  ivf_merge_kernel<<<dim3((unsigned)nq), IVF_THREADS, 0, stream>>>(part, pref, nprobe, k, nslab, row_offset, out_idx, out_dist);
}

}  // namespace mi
