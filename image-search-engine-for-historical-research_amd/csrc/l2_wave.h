// The wave-level arithmetic of the squared-L2 metric, shared by the tail of the flat search (l2_metric.hip), the re-ranking
// of shortlists (refine.hip) and the graph search (graph_search.hip): all give a (query, row) pair the same bits.  DESIGN.md 5.11, 5.15.
#pragma once
#include "common.h"
#include "f64_key.h"

namespace mi {

__device__ __forceinline__ double l2_wave_sum(double x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// sum_j (q_j - g_j)^2 over the user's d columns by one wave: the DIRECT form (a query equal to the stored row gives 0.0 exactly;
// the expansion ||q||^2 - 2 q.g + ||g||^2 gives rounding noise there).  f32 values promoted to f64, f64 accumulation.  Both rows
// are 16-byte aligned and at least round_up(d, 4) floats long (rows of stride dp).
__device__ __forceinline__ double l2_direct_wave(const float* __restrict__ q, const float* __restrict__ g, int32_t d, int lane) {
  double acc = 0.0;
  for (int32_t c = 4 * lane; c < d; c += 256) {
    const float4 a = *reinterpret_cast<const float4*>(q + c), b = *reinterpret_cast<const float4*>(g + c);
    const double d0 = (double)a.x - (double)b.x, d1 = (double)a.y - (double)b.y, d2 = (double)a.z - (double)b.z,
                 d3 = (double)a.w - (double)b.w;
    acc = __builtin_fma(d0, d0, acc);
    if (c + 1 < d) acc = __builtin_fma(d1, d1, acc);
    if (c + 2 < d) acc = __builtin_fma(d2, d2, acc);
    if (c + 3 < d) acc = __builtin_fma(d3, d3, acc);
  }
  return l2_wave_sum(acc);
}

// sum_j q_j g_j over d columns by one wave: l2_direct_wave's walk with the product in place of the squared difference (products of
// f32 values are exact in f64, so every FMA rounds once, as rescore_kernel's sum does: select.hip)
__device__ __forceinline__ double refine_dot_wave(const float* __restrict__ q, const float* __restrict__ g, int32_t d, int lane) {
  double acc = 0.0;
  for (int32_t c = 4 * lane; c < d; c += 256) {
    const float4 a = *reinterpret_cast<const float4*>(q + c), b = *reinterpret_cast<const float4*>(g + c);
    acc = __builtin_fma((double)a.x, (double)b.x, acc);
    if (c + 1 < d) acc = __builtin_fma((double)a.y, (double)b.y, acc);
    if (c + 2 < d) acc = __builtin_fma((double)a.z, (double)b.z, acc);
    if (c + 3 < d) acc = __builtin_fma((double)a.w, (double)b.w, acc);
  }
  return l2_wave_sum(acc);
}

}  // namespace mi
