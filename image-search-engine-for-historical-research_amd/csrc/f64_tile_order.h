// Geometry and tile order of the 128 x 128 float64 MFMA tile (f64_tile.h).  Pure arithmetic, no HIP, so a
// stand-alone program can include it alone (tests/f64_tile_order_check.cpp); constexpr, so device code may call it too.
#pragma once
#include <cstdint>

namespace mi {

constexpr int F64T_TILE = 128;                            // rows and columns of the product per workgroup
constexpr int F64T_KC = 16;                               // K-chunk staged in LDS
// LDS row stride in doubles: 18 r mod 32 is a different even 8-byte slot for each of the 16 rows of a ds_read_b64 fragment
// read, + k: conflict-free
constexpr int F64T_LD = F64T_KC + 2;
constexpr int F64T_PER = F64T_TILE * F64T_KC / 256;       // elements of one operand chunk per thread (8)
constexpr int F64T_RSTEP = 256 / F64T_KC;                 // tile rows between a thread's elements when K is its fast index (16)
constexpr int F64T_BUF = F64T_TILE * F64T_LD;             // doubles of one buffer of one operand
constexpr int F64T_LDS_BYTES = 4 * F64T_BUF * 8;          // A [2][128][18], then B [2][128][18]

// Tile order: block b of a grid of ncb column blocks x nrb row tiles -> (column block, row tile).  When ncb is a multiple of 8,
// XCD x (= b mod 8) owns the column blocks x, x + 8, .. (its slab of B stays in its L2) and all XCDs walk the row tiles in the
// same order (an X tile leaves HBM once and is served to the other seven from the Infinity Cache); otherwise plain row-major.
constexpr void f64t_tile_order(uint32_t b, uint32_t ncb, uint32_t nrb, uint32_t* cb, uint32_t* rt) {
  if ((ncb & 7u) == 0) {
    const uint32_t x = b & 7u, j = b >> 3;
    *cb = x + 8u * (j / nrb);
    *rt = j % nrb;
  } else {
    *cb = b % ncb;
    *rt = b / ncb;
  }
}

}  // namespace mi
