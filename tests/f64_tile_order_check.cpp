// csrc/f64_tile_order.h on the host: the tile order of the 128 x 128 f64 MFMA kernels over a sweep of grids.  A program of its own
// (tests/test_f64_tile_cpu.py compiles it under AddressSanitizer and UBSan); prints "f64_tile_order_check ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../image-search-engine-for-historical-research_amd/csrc/f64_tile_order.h"

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("line %d: %s (ncb %u nrb %u b %u)\n", __LINE__, #cond, ncb, nrb, b); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

int main() {
  using namespace mi;
  const uint32_t nrbs[] = {1, 2, 3, 7, 8, 9, 64};
  for (uint32_t ncb = 1; ncb <= 40; ++ncb)
    for (uint32_t nrb : nrbs) {
      std::vector<int> seen((size_t)ncb * nrb, 0);
      for (uint32_t b = 0; b < ncb * nrb; ++b) {
        uint32_t cb = ~0u, rt = ~0u;
        f64t_tile_order(b, ncb, nrb, &cb, &rt);
        CHECK(cb < ncb && rt < nrb);                                       // onto the grid
        CHECK(seen.at((size_t)cb * nrb + rt)++ == 0);                      // every tile once: a bijection
        if (ncb % 8 == 0) CHECK(cb % 8 == b % 8);                          // XCD x owns the column blocks x, x + 8, ..
        else CHECK(cb == b % ncb && rt == b / ncb);
      }
    }
  static_assert(F64T_TILE == 128 && F64T_KC == 16 && F64T_LD == 18 && F64T_PER == 8 && F64T_RSTEP == 16, "geometry");
  static_assert(F64T_LDS_BYTES == 73728, "two buffers of two operands");
  std::printf("f64_tile_order_check ok\n");
  return 0;
}
