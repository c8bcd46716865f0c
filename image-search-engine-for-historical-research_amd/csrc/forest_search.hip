// Descent of the random-projection forest (api_forest.hip): one wave per (query, tree).  Every lane walks the L
// levels on the query's projections -- j = 2 j + (Pq[t L + l] >= split[t][2^l - 1 + j]), a NaN compares false and goes left --,
// then the lanes copy the leaf's slice [floor(j n / 2^L), floor((j + 1) n / 2^L)) of the tree's permutation into the query's
// candidate slots t * leaf_max .., as global ids, and put -1 into the slots the leaf does not fill.  Plain 8-byte vector stores.
#include "common.h"
#include "kernels.h"

namespace mi {

__global__ __launch_bounds__(256) void forest_descend_kernel(const double* __restrict__ Pq /*[nq][T L]*/,
                                                             const double* __restrict__ splits /*[T][2^L - 1]*/,
                                                             const int32_t* __restrict__ leaves /*[T][n]*/, int64_t n, int32_t T, int32_t L,
                                                             int32_t leaf_max, int64_t row_offset, int64_t nq, int64_t* __restrict__ cand,
                                                             int64_t cand_stride) {
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= nq * T) return;
  const int lane = threadIdx.x & 63;
  const int64_t q = wid / T;
  const int32_t t = (int32_t)(wid % T);
  const double* pq = Pq + (size_t)q * T * L + (size_t)t * L;
  const double* sp = splits + (size_t)t * (((size_t)1 << L) - 1);
  int64_t j = 0;
  for (int32_t l = 0; l < L; ++l) j = 2 * j + (pq[l] >= sp[(((int64_t)1 << l) - 1) + j] ? 1 : 0);
  const int64_t a = (j * n) >> L, b = ((j + 1) * n) >> L;      // (j < 2^24, n < 2^31)
  const int32_t* lv = leaves + (size_t)t * n + a;
  int64_t* o = cand + q * cand_stride + (int64_t)t * leaf_max;
  for (int32_t i = lane; i < leaf_max; i += 64) o[i] = i < b - a ? row_offset + lv[i] : (int64_t)-1;
}

void launch_forest_descend(const double* Pq, const double* splits, const int32_t* leaves, int64_t n, int32_t T, int32_t L,
                           int32_t leaf_max, int64_t row_offset, int64_t nq, int64_t* cand, int64_t cand_stride, hipStream_t stream) {
  if (nq <= 0) return;
  const int64_t waves = nq * T;
  hipLaunchKernelGGL(forest_descend_kernel, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, stream, Pq, splits, leaves, n, T, L, leaf_max,
                     row_offset, nq, cand, cand_stride);
}

}  // namespace mi
