// The order-preserving 64-bit key of a float64: a < b  <=>  key(a) < key(b) as unsigned integers, so a sort, a radix select or a
// binary search on values is one on integers.  A non-negative value keeps its bits with the sign bit set, a negative one has all
// bits flipped; -0 and +0 are one value and get one key, 0x8000000000000000.  The two encoders differ only in where a NaN goes.
// ~key reverses the order, so a descending sort is an ascending one on the complement.  Nothing of HIP is used but the function
// qualifiers, which the includer has in scope: a stand-alone host program defines them away (tests/f64_key_check.cpp).
#pragma once
#include <cstdint>

namespace mi {

__host__ __device__ __forceinline__ uint64_t f64_bits(double x) {
  uint64_t u;
  __builtin_memcpy(&u, &x, sizeof u);
  return u;
}

// NaN lowest (key 0, below -inf): a NaN score comes last where the larger is the better (emit_kernel, dense top-k, range search).
// (The zero rule is spelled as a comparison here and as an addition in f64_key_nan_highest: each keeps the instructions its
// first user, emit_kernel / the squared-L2 tail, always had.)
__host__ __device__ __forceinline__ uint64_t f64_key_nan_lowest(double s) {
  if (s != s) return 0ull;
  if (s == 0.0) return 0x8000000000000000ull;
  const uint64_t b = f64_bits(s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// NaN highest (key ~0, above +inf, the key of the padding): a NaN distance comes last where the smaller is the better
__host__ __device__ __forceinline__ uint64_t f64_key_nan_highest(double x) {
  if (x != x) return ~0ull;
  x += 0.0;
  const uint64_t u = f64_bits(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// the value behind a key of either encoder: +0 for the key of a zero, a NaN for the key of a NaN
__host__ __device__ __forceinline__ double f64_key_value(uint64_t key) {
  const uint64_t u = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  double x;
  __builtin_memcpy(&x, &u, sizeof x);
  return x;
}

}  // namespace mi
