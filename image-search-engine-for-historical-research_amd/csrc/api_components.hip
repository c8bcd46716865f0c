// Connected components of the C ABI (mi_components; kernels in csrc/components.hip): the transitive closure of
// "row a is a near duplicate of row b" as one int32 label per row, the smallest row of the component -- what mi_gallery_set_groups
// takes.  A handle of its own: 4 bytes of device memory per row.  Edges arrive as pair lists, as the CSR output of a self-join, or
// as the ballots of the Hamming self-join (hamming_self_scan in api_hamming.hip), in which case no pair exists anywhere.
// Every add call: ids checked (host arrays on the host, device arrays by a flag kernel) -> union launches -> one flatten launch ->
// synchronise.  The forest is flat between calls, so mi_components_labels is a copy.
#include "api_internal.h"

constexpr int64_t CC_STAGE_EDGES = (int64_t)4 << 20;     // host pairs pass through the device this many at a time (2 x 32 MiB)

static bool ids_in_range(const int64_t* a, int64_t m, int64_t n) {
  for (int64_t t = 0; t < m; ++t)
    if ((uint64_t)a[t] >= (uint64_t)n) return false;
  return true;
}

// behind launch_components_check on s: the flag read and, where raised, cleared again
static int cc_flag_raised(mi_components* h, hipStream_t s, bool* raised) {
  unsigned long long f = 0;
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(&f, h->word, 8, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  if (f) {
    HIPC(hipMemsetAsync(h->word, 0, 8, s));
    HIPC(hipStreamSynchronize(s));
  }
  *raised = f != 0;
  return MI_OK;
}

// the tail of every add call on s: the forest flat again, the work done
static int cc_finish(mi_components* h, hipStream_t s) {
  launch_components_flatten(h->parent, h->n, s);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));
  return MI_OK;
}

extern "C" {

int mi_components_create(int64_t n, int device, mi_components** out) {
  REQUIRE(out, "null pointer: out");
  REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, "mi_components_create: n must be in [0, 2^31 - 1]");
  HIPC(hipSetDevice(device));
  mi_components* h = new mi_components();
  h->device = device;
  h->n = n;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess && n > 0) e = h->parent.alloc((size_t)n);
  if (e == hipSuccess) e = h->word.alloc(32);
  if (e == hipSuccess) e = hipMemsetAsync(h->word, 0, 256, h->stream);
  if (e == hipSuccess) {
    launch_components_init(h->parent, n, h->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    mi_components_destroy(h);
    return fail(e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, std::string("components: ") + hipGetErrorString(e));
  }
  *out = h;
  return MI_OK;
}

int mi_components_reset(mi_components* h) {
  REQUIRE(h, "null handle");
  std::lock_guard<std::mutex> lock(h->mu);
  HIPC(hipSetDevice(h->device));
  launch_components_init(h->parent, h->n, h->stream);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(h->stream));
  return MI_OK;
}

int mi_components_add_pairs(mi_components* h, const int64_t* i, const int64_t* j, int64_t m, int memspace) {
  REQUIRE(h, "null handle");
  REQUIRE(m >= 0, "negative number of pairs");
  REQUIRE(m == 0 || (i && j), "null pointer: pairs");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  if (m == 0) return MI_OK;
  std::lock_guard<std::mutex> lock(h->mu);
  hipStream_t s = h->stream;
  if (memspace == MI_HOST) {
    REQUIRE(ids_in_range(i, m, h->n) && ids_in_range(j, m, h->n), "mi_components_add_pairs: an id outside [0, n)");
    HIPC(hipSetDevice(h->device));
    const int64_t step = std::min(m, CC_STAGE_EDGES);
    TmpAlloc tmp;
    int64_t* stage = tmp.get<int64_t>((size_t)step * 2);
    if (!stage) return fail(MI_ERR_NOMEM, "staging buffer of mi_components_add_pairs");
    for (int64_t e0 = 0; e0 < m; e0 += step) {
      const int64_t mm = std::min(step, m - e0);
      HIPC(hipMemcpyAsync(stage, i + e0, (size_t)mm * 8, hipMemcpyHostToDevice, s));
      HIPC(hipMemcpyAsync(stage + step, j + e0, (size_t)mm * 8, hipMemcpyHostToDevice, s));
      launch_components_pairs(h->parent, stage, stage + step, mm, s);
      HIPC(hipGetLastError());
      HIPC(hipStreamSynchronize(s));               // the staging buffer is reused by the next block
    }
    return cc_finish(h, s);
  }
  HIPC(hipSetDevice(h->device));
  bool bad;
  launch_components_check(i, j, m, h->n, (uint32_t*)h->word.get(), s);
  int rc = cc_flag_raised(h, s, &bad);
  if (rc != MI_OK) return rc;
  REQUIRE(!bad, "mi_components_add_pairs: an id outside [0, n)");
  launch_components_pairs(h->parent, i, j, m, s);
  return cc_finish(h, s);
}

int mi_components_add_csr(mi_components* h, int64_t row0, const int64_t* lims, const int64_t* idx, int64_t nq, int memspace) {
  REQUIRE(h, "null handle");
  REQUIRE(nq >= 0, "nq must be >= 0");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  if (nq == 0) return MI_OK;
  REQUIRE(lims, "null pointer: lims");
  std::lock_guard<std::mutex> lock(h->mu);
  REQUIRE(row0 >= 0 && row0 <= h->n && nq <= h->n - row0, "mi_components_add_csr: query rows row0 .. row0 + nq outside [0, n)");
  hipStream_t s = h->stream;
  // the offsets are read on the host either way: they size the launch
  std::vector<int64_t> host_lims;
  const int64_t* hl = lims;
  if (memspace == MI_DEVICE) {
    HIPC(hipSetDevice(h->device));
    host_lims.resize((size_t)nq + 1);
    HIPC(hipMemcpy(host_lims.data(), lims, ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost));
    hl = host_lims.data();
  }
  REQUIRE(hl[0] == 0, "mi_components_add_csr: lims[0] must be 0");
  for (int64_t q = 0; q < nq; ++q) REQUIRE(hl[q] <= hl[q + 1], "mi_components_add_csr: lims must be non-decreasing");
  const int64_t total = hl[nq];
  if (total == 0) return MI_OK;
  REQUIRE(idx, "null pointer: idx");
  if (memspace == MI_HOST) {
    REQUIRE(ids_in_range(idx, total, h->n), "mi_components_add_csr: an id outside [0, n)");
    HIPC(hipSetDevice(h->device));
    TmpAlloc tmp;
    int64_t* stage = tmp.get<int64_t>((size_t)(nq + 1 + total));
    if (!stage) return fail(MI_ERR_NOMEM, "staging buffer of mi_components_add_csr");
    HIPC(hipMemcpyAsync(stage, lims, ((size_t)nq + 1) * 8, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(stage + nq + 1, idx, (size_t)total * 8, hipMemcpyHostToDevice, s));
    launch_components_csr(h->parent, row0, stage, stage + nq + 1, nq, total, s);
    return cc_finish(h, s);                        // synchronises: the staging buffer is freed behind it
  }
  bool bad;
  launch_components_check(idx, nullptr, total, h->n, (uint32_t*)h->word.get(), s);
  int rc = cc_flag_raised(h, s, &bad);
  if (rc != MI_OK) return rc;
  REQUIRE(!bad, "mi_components_add_csr: an id outside [0, n)");
  launch_components_csr(h->parent, row0, lims, idx, nq, total, s);
  return cc_finish(h, s);
}

int mi_components_add_hamming_self(mi_components* h, mi_hamming* b, int64_t row0, int64_t nrows, int32_t radius) {
  REQUIRE(h, "null handle");
  REQUIRE(b, "null pointer: binary index");
  std::lock_guard<std::mutex> lock(h->mu);
  std::lock_guard<std::mutex> block(b->mu);
  REQUIRE(b->n == h->n, "mi_components_add_hamming_self: the binary index must hold n rows, one per row of the components");
  REQUIRE(b->device == h->device, "mi_components_add_hamming_self: the binary index is on another device");
  REQUIRE(b->row_offset == 0, "mi_components_add_hamming_self: the binary index must have row_offset 0");
  int rc = hamming_self_check(b, row0, nrows, radius);
  if (rc != MI_OK) return rc;
  if (nrows == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  hipStream_t s = b->stream;                       // the index's one stream: its workspace is written and read in order
  int64_t qc;
  if ((rc = hamming_self_plan(b, row0, nrows, &qc)) != MI_OK) return rc;
  for (int64_t q0 = 0; q0 < nrows; q0 += qc) {
    HammingBallots m;
    if ((rc = hamming_self_scan(b, row0, nrows, radius, qc, q0, &m, s)) != MI_OK) return rc;
    launch_components_ballots(h->parent, m.masks, m.b0, m.nbl, m.qstride, m.qrow0, m.nq, s);
  }
  return cc_finish(h, s);
}

int mi_components_labels(mi_components* h, int32_t* out_labels, int memspace, int64_t* out_groups) {
  REQUIRE(h, "null handle");
  REQUIRE(out_labels || h->n == 0, "null pointer: out_labels");
  REQUIRE(memspace == MI_HOST || memspace == MI_DEVICE, "memspace must be MI_HOST or MI_DEVICE");
  std::lock_guard<std::mutex> lock(h->mu);
  if (out_groups) *out_groups = 0;
  if (h->n == 0) return MI_OK;
  HIPC(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  unsigned long long roots = 0;
  HIPC(hipMemcpyAsync(out_labels, h->parent, (size_t)h->n * 4, memspace == MI_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
  if (out_groups) {
    launch_components_count(h->parent, h->n, h->word, s);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(&roots, h->word, 8, hipMemcpyDeviceToHost, s));
    HIPC(hipMemsetAsync(h->word, 0, 8, s));
  }
  HIPC(hipStreamSynchronize(s));
  if (out_groups) *out_groups = (int64_t)roots;
  return MI_OK;
}

int mi_components_info(const mi_components* h, int64_t* n, int32_t* device) {
  REQUIRE(h, "null handle");
  if (n) *n = h->n;
  if (device) *device = h->device;
  return MI_OK;
}

int mi_components_destroy(mi_components* h) {
  if (!h) return MI_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->bufs.reset();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return MI_OK;
}

}  // extern "C"
