// The 128 x 128 float64 MFMA workgroup tile, spelled out once for the four product kernels that run on it:
// whiten_mfma_kernel (whiten.hip), lsh_encode_kernel (lsh.hip), km_assign_mfma_kernel (kmeans.hip), which compute X * B^T, and
// scatter_mfma_kernel (scatter.hip), whose operands both come from X and whose reduction runs over rows.
//  * v_mfma_f64_16x16x4_f64, 128 x 128 outputs per 256-thread workgroup = 4 waves x (64 x 64) = 4 x 4 MFMA blocks per wave (128
//    accumulator registers); two workgroups per CU, so one of them stages while the other multiplies;
//  * K streams in chunks of 16 through LDS, two buffers per operand (73.7 KB of dynamic LDS per workgroup): chunk c + 1 is
//    written into the other buffer while chunk c is multiplied, ONE barrier per chunk (one buffer and two barriers per 64 MFMAs
//    kept the matrix pipe busy 0.69, profiles/r06z_whiten_pmc.txt); the global loads of chunk c + 1 are in flight under the
//    first 48 of the 64 MFMAs of chunk c;
//  * the K order inside a 16x16x4 step is the hardware's; across steps it is ascending, like a row-major dot product.
// Here: the geometry, the tile order, the fragment and C layout, the lane coordinates (used by scatter), the MFMA steps and the
// host-side choice of instantiation: what leaves every kernel's instructions as they were (profiles/f64_tile_isa.txt).
// The loop "load c + 1, 3 steps, store c + 1, 1 step, barrier", the zeroing of the accumulators, the operand loaders and, outside
// scatter, the lane coordinates are still written out in each kernel.  Moved into functions they are optimised on their own
// before they are inlined and every kernel came out with other instructions (profiles/f64_tile_attempts.txt, per kernel):
// whiten and LSH spill already and changed their spills; in scatter and k-means, which mostly do not spill, the loop changed
// vgpr_count in two instantiations each, and the variants that kept every counted figure were not timed on the GPU.
// forest_project.hip is NOT one of these: one row of MFMA blocks per wave and no LDS ring -- another geometry, do not fold it in.
// The constants and the tile order are plain arithmetic and live in f64_tile_order.h, which a host compiler takes alone.
#pragma once
#include "common.h"
#include "f64_tile_order.h"

namespace mi {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// Lane coordinates, computed by each kernel as wr = wave >> 1, wc = wave & 1, l15 = lane & 15, lq = lane >> 4: wave (wr, wc) owns a
// 64 x 64 quadrant; an A fragment is A[i = l15][k = lq] at (wr * 64 + l15) * F64T_LD + lq of an A buffer, a B fragment
// B[k = lq][j = l15] = (row j of the B operand)[k] at (wc * 64 + l15) * F64T_LD + lq of a B buffer.  C layout of
// v_mfma_f64_16x16x4_f64: column = lane & 15, row = (lane >> 4) + 4 * register, so register r of block (mi, ni) is the tile's
// element (wr * 64 + mi * 16 + lq + 4 r, wc * 64 + ni * 16 + l15).  The same as a struct, for the kernel that keeps its
// instructions with it (scatter_mfma_kernel):
struct F64Lane {
  int t, lane, wr, wc, l15, lq;
  __device__ __forceinline__ F64Lane() {
    t = threadIdx.x, lane = t & 63;
    const int w = t >> 6;
    wr = w >> 1, wc = w & 1, l15 = lane & 15, lq = lane >> 4;
  }
  __device__ __forceinline__ int a_off() const { return (wr * 64 + l15) * F64T_LD + lq; }      // into an A buffer
  __device__ __forceinline__ int b_off() const { return (wc * 64 + l15) * F64T_LD + lq; }      // into a B buffer
  __device__ __forceinline__ int row(int mi, int r) const { return wr * 64 + mi * 16 + lq + 4 * r; }
  __device__ __forceinline__ int col(int ni) const { return wc * 64 + ni * 16 + l15; }
};

// MFMA steps ks0 .. ks1 - 1 (4 k each, ascending) of the chunk whose fragments start at xa (A buffer + a_off), pb (B + b_off)
__device__ __forceinline__ void f64t_mfma_steps(f64x4 (&acc)[4][4], const double* xa, const double* pb, int ks0, int ks1) {
#pragma unroll
  for (int ks = ks0; ks < ks1; ++ks) {
    double a[4], bb[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) a[mi] = xa[mi * 16 * F64T_LD + ks * 4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) bb[ni] = pb[ni * 16 * F64T_LD + ks * 4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], bb[ni], acc[mi][ni], 0, 0, 0);
  }
}

// ---- host side: the (float | double) x (ROWS | not) choice among the four instantiations of an X * B^T kernel, whose first
// parameter is X; every instantiation gets its dynamic LDS limit raised
template <typename T>
struct F64TSame { typedef T type; };

template <typename T, typename... A>
static inline void f64t_launch_one(void (*kern)(const T*, A...), dim3 grid, hipStream_t stream, const void* X, A... a) {
  ensure_dynamic_lds((const void*)kern, F64T_LDS_BYTES);
  hipLaunchKernelGGL(kern, grid, dim3(256), F64T_LDS_BYTES, stream, (const T*)X, a...);
}

template <typename... A>
static inline void f64t_launch(int dtype, bool rows, void (*f_rows)(const float*, A...), void (*f_any)(const float*, A...),
                               void (*d_rows)(const double*, A...), void (*d_any)(const double*, A...), dim3 grid,
                               hipStream_t stream, const void* X, typename F64TSame<A>::type... a) {
  if (dtype == 0) f64t_launch_one(rows ? f_rows : f_any, grid, stream, X, a...);
  else f64t_launch_one(rows ? d_rows : d_any, grid, stream, X, a...);
}
#define MI_F64T_KERNELS(K) K<float, true>, K<float, false>, K<double, true>, K<double, false>

}  // namespace mi
