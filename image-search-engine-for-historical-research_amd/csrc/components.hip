// Connected components of the rows of an index (api_components.hip): a union-find forest `parent`, int32 [n], in
// device memory, fed with edges from pair lists, from the CSR output of a self-join, or straight from the 64-bit ballots the
// Hamming self-join leaves per (64-row block, query) (hamming_range.hip) -- in which case no pair is ever materialised.
//
// The invariant.  A root is only ever hooked under a SMALLER root, and every other write lowers an entry to another ancestor, so
// parent[v] <= v always holds, with equality exactly at the roots.  Three things follow:
//   * there is no cycle (a walk v, parent[v], parent[parent[v]], ... strictly decreases until it stands on a root);
//   * the root of a tree is its smallest row, so the label of a component is the smallest row in it;
//   * the labels depend on the SET of edges alone: whatever order edges, waves and launches arrive in, the trees at the end are the
//     connected components of the edges, and each is named by its minimum.
// A node that has stopped being a root never becomes one again: the hook is a compare-and-swap that expects parent[r] == r, and
// compression only lowers entries that were already seen below their index.
//
// Memory model.  Inside a union launch every read and write of `parent` is a relaxed atomic at device (agent) scope: cc_load,
// atomicCAS for the hook, atomicMin for path halving.  Correctness does NOT depend on how fresh a read is:
//   * a stale parent is still an ancestor -- entries move only towards the root of the same tree -- so a walk over old values
//     still climbs the right tree and still strictly decreases;
//   * the compare-and-swap decides a hook: it succeeds only if, at that instant, the larger node really is a root; a walk that
//     ended on a node hooked in the meantime fails there, receives the node's present parent and goes on from it;
//   * compression writes only to nodes already seen as non-roots, which are never hooked again, and only values that are ancestors
//     of the node, so it can neither split a tree nor undo a hook.
// Atomic loads are used all the same, and plain loads are not, because a plain load may be served from this CU's L1, which no other
// CU's store ever refreshes: a wave could keep walking a chain that was compressed or hooked long ago, and would see its own
// failed compare-and-swap "succeed to change nothing" again and again.  Device-scope atomics are resolved beyond the L1.
// There is no grid barrier, no spin on a flag, no cooperative launch and no lock: a retry happens only after a value was observed
// to have CHANGED (so some other union made progress), and no wave ever waits for another.
//
//   cc_pairs_kernel    one thread per edge (i[e], j[e]), int64 ids checked beforehand
//   cc_csr_kernel      one thread per hit idx[t]; its query row is row0 + q with lims[q] <= t < lims[q + 1], q by binary search
//   cc_ballots_kernel  one thread per mask word masks[bl * qstride + q]: every set bit l unites qrow0 + q with (b0 + bl) * 64 + l
//   cc_check_kernel    flag kernel for device-resident ids: any id outside [0, n) raises the flag; nothing is united then
//   cc_flatten_kernel  parent[v] = root(v) for all v, a launch of its own behind the union launches of a call
//   cc_count_kernel    the number of v with parent[v] == v
#include "kernels.h"

namespace mi {

__device__ __forceinline__ int32_t cc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_store(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A root above v as this walk saw it (the caller's compare-and-swap finds out whether it still is one), with path halving.
// Ends: p != v means p < v (the invariant), so v strictly decreases every turn and is bounded below by 0.
__device__ __forceinline__ int32_t cc_find(int32_t* parent, int32_t v) {
  for (;;) {
    const int32_t p = cc_load(parent + v);
    if (p == v) return v;
    const int32_t gp = cc_load(parent + p);
    if (gp != p) atomicMin(parent + v, gp);       // v is not a root; gp <= p < v is an ancestor of v: the entry only decreases
    v = p;
  }
}

// One edge.  Ends: a and b only ever move to ancestors (cc_find), and a failed compare-and-swap returns the present parent of
// `a`, which is below `a` because `a` has been hooked by somebody else; so a + b strictly decreases with every retry and is
// bounded below by 0.  Nothing waits: a retry follows an observed change.
__device__ __forceinline__ void cc_unite(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;                            // one tree already (and trees are never split)
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = atomicCAS(parent + a, a, b);   // the larger root under the smaller one
    if (old == a) return;
    a = old;                                       // `a` was no root any more: old < a is its parent now
  }
}

constexpr int CC_THREADS = 256;
constexpr int64_t CC_MAX_BLOCKS = (int64_t)1 << 20;

// Every kernel below walks its items with a grid stride.  Ends: t grows by the same positive step every turn up to `count`.
#define CC_FOR_EACH(t, count) \
  for (int64_t t = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; t < (count); t += (int64_t)gridDim.x * CC_THREADS)

__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(int32_t* __restrict__ parent, int64_t n) {
  CC_FOR_EACH(v, n) parent[v] = (int32_t)v;
}

// a, b (b may be NULL): m ids each
__global__ __launch_bounds__(CC_THREADS) void cc_check_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int64_t m,
                                                             int64_t n, uint32_t* __restrict__ flag) {
  CC_FOR_EACH(t, m) {
    bool bad = (uint64_t)a[t] >= (uint64_t)n;
    if (b) bad = bad || (uint64_t)b[t] >= (uint64_t)n;
    if (bad) *flag = 1u;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_pairs_kernel(int32_t* parent, const int64_t* __restrict__ i, const int64_t* __restrict__ j,
                                                             int64_t m) {
  CC_FOR_EACH(e, m) {
    const int32_t a = (int32_t)i[e], b = (int32_t)j[e];
    if (a != b) cc_unite(parent, a, b);
  }
}

// lims [nq + 1] non-decreasing from 0 (checked by the host), total = lims[nq]
__global__ __launch_bounds__(CC_THREADS) void cc_csr_kernel(int32_t* parent, int64_t row0, const int64_t* __restrict__ lims,
                                                           const int64_t* __restrict__ idx, int64_t nq, int64_t total) {
  CC_FOR_EACH(t, total) {
    // the last q in [0, nq) with lims[q] <= t (queries without hits share their offset with the next one).  Ends: hi - lo
    // shrinks by at least one every turn
    int64_t lo = 0, hi = nq - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (lims[mid] <= t) lo = mid;
      else hi = mid - 1;
    }
    const int32_t a = (int32_t)(row0 + lo), b = (int32_t)idx[t];
    if (a != b) cc_unite(parent, a, b);
  }
}

// masks [nbl][qstride]: what hamming_range_scan_kernel<_, SELF = true> leaves behind -- bit l of masks[bl][q] is set when row
// (b0 + bl) * 64 + l is below n, above query row qrow0 + q and within the radius.  Queries fastest: the loads are coalesced
__global__ __launch_bounds__(CC_THREADS) void cc_ballots_kernel(int32_t* parent, const unsigned long long* __restrict__ masks, int64_t b0,
                                                               int64_t nbl, int64_t qstride, int64_t qrow0, int32_t nq) {
  CC_FOR_EACH(t, nbl * nq) {
    const int64_t bl = t / nq, q = t % nq;
    unsigned long long m = masks[bl * qstride + q];
    const int32_t a = (int32_t)(qrow0 + q);
    const int64_t base = (b0 + bl) * 64;
    while (m) {                                    // ends: every turn clears one bit of m
      const int l = __ffsll((long long)m) - 1;
      m &= m - 1ull;
      cc_unite(parent, a, (int32_t)(base + l));
    }
  }
}

// No union runs beside this launch, so no root changes in it: the entry of a root is never written with another value, every
// other entry is only ever replaced by its root.  A reader therefore sees, at any node, its old parent or its root -- both
// ancestors below the node.  Ends: r strictly decreases (parent[r] < r at every non-root) down to a root.
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int32_t* parent, int64_t n) {
  CC_FOR_EACH(v, n) {
    int32_t r = cc_load(parent + v);
    for (;;) {
      const int32_t p = cc_load(parent + r);
      if (p == r) break;
      r = p;
    }
    cc_store(parent + v, r);
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_count_kernel(const int32_t* __restrict__ parent, int64_t n,
                                                             unsigned long long* __restrict__ count) {
  unsigned long long mine = 0;
  CC_FOR_EACH(v, n) mine += parent[v] == (int32_t)v;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}

// ---- launchers
static unsigned cc_blocks(int64_t count) { return (unsigned)std::min<int64_t>(CC_MAX_BLOCKS, (count + CC_THREADS - 1) / CC_THREADS); }

void launch_components_init(int32_t* parent, int64_t n, hipStream_t stream) {
  if (n > 0) cc_init_kernel<<<cc_blocks(n), CC_THREADS, 0, stream>>>(parent, n);
}

void launch_components_check(const int64_t* a, const int64_t* b, int64_t m, int64_t n, uint32_t* flag, hipStream_t stream) {
  if (m > 0) cc_check_kernel<<<cc_blocks(m), CC_THREADS, 0, stream>>>(a, b, m, n, flag);
}

void launch_components_pairs(int32_t* parent, const int64_t* i, const int64_t* j, int64_t m, hipStream_t stream) {
  if (m > 0) cc_pairs_kernel<<<cc_blocks(m), CC_THREADS, 0, stream>>>(parent, i, j, m);
}

void launch_components_csr(int32_t* parent, int64_t row0, const int64_t* lims, const int64_t* idx, int64_t nq, int64_t total,
                           hipStream_t stream) {
  if (nq > 0 && total > 0) cc_csr_kernel<<<cc_blocks(total), CC_THREADS, 0, stream>>>(parent, row0, lims, idx, nq, total);
}

void launch_components_ballots(int32_t* parent, const unsigned long long* masks, int64_t b0, int64_t nbl, int64_t qstride,
                               int64_t qrow0, int32_t nq, hipStream_t stream) {
  if (nbl > 0 && nq > 0)
    cc_ballots_kernel<<<cc_blocks(nbl * nq), CC_THREADS, 0, stream>>>(parent, masks, b0, nbl, qstride, qrow0, nq);
}

void launch_components_flatten(int32_t* parent, int64_t n, hipStream_t stream) {
  if (n > 0) cc_flatten_kernel<<<cc_blocks(n), CC_THREADS, 0, stream>>>(parent, n);
}

void launch_components_count(const int32_t* parent, int64_t n, unsigned long long* count, hipStream_t stream) {
  if (n > 0) cc_count_kernel<<<cc_blocks(n), CC_THREADS, 0, stream>>>(parent, n, count);
}

}  // namespace mi
