// How a Minkowski radius search cuts its queries into chunks (api_minkowski_range.hip).  Pure arithmetic on the
// shapes: host code, no HIP, so a stand-alone program can include it alone.
#pragma once
#include <cstdint>

namespace mi {

constexpr int64_t MINK_RANGE_MAX_CHUNK = 65535;      // blockIdx.y of the (part, query) grids

// bytes of workspace one query of a chunk takes: its float64 values of `rows` scanned rows, a count (4 bytes) and a place (8) per part
static inline int64_t mink_range_query_bytes(int64_t rows, int32_t nparts) {
  return (rows < 1 ? 1 : rows) * 8 + (int64_t)nparts * 12;
}

// queries per chunk: as many whole tiles of `qt` queries as fit into `bytes`, one tile at the least, no more than the call has
// (rounded up to a tile) and no more than a grid takes
static inline int64_t mink_range_chunk(int64_t bytes, int64_t rows, int32_t nparts, int64_t nq, int32_t qt) {
  const int64_t t = qt < 1 ? 1 : qt;
  int64_t qc = bytes / mink_range_query_bytes(rows, nparts) / t * t;
  const int64_t need = (nq + t - 1) / t * t, most = MINK_RANGE_MAX_CHUNK / t * t;
  if (qc > need) qc = need;
  if (qc > most) qc = most;
  return qc < t ? t : qc;
}

}  // namespace mi
