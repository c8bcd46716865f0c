// The neighbour table of a graph index, owned once for mi_graph (api_graph.hip) and mi_pq_graph (api_pq_graph.hip): what the two
// handles hold in common.  Host code only; needs nothing beyond device_buf.h, so a program with stand-ins for the HIP runtime can
// include it (tests/device_buf_check.cpp).  The functions that fill and read a table are declared in api_internal.h.
#pragma once
#include <cstdint>

#include "device_buf.h"

struct GraphTable {
  int64_t n = 0;                       // rows of the owner when the table was made
  int32_t R = 0, ne = 0;
  DeviceBuf<int32_t> adj;              // [n][R], -1 = padding
  DeviceBuf<int32_t> entries;          // [ne]
  // on the set whose bytes() the handle reports, or on none
  explicit GraphTable(DeviceBufSet* set = nullptr) : adj(set), entries(set) {}
  // room for a table of n rows and ne entries, exactly (neither filled); a failure leaves nothing allocated
  hipError_t alloc(int64_t n_, int32_t R_, int32_t ne_) {
    n = n_, R = R_, ne = ne_;
    hipError_t e = adj.alloc((size_t)n * R);
    if (e == hipSuccess) e = entries.alloc((size_t)ne);
    if (e != hipSuccess) adj.reset(), entries.reset();
    return e;
  }
};
