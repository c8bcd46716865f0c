// Standalone driver for the scoring launches of libmi355_retrieval.so (no Python, no torch): builds random 16-bit operand
// images with the score distribution of unit vectors (sigma = 1 / sqrt(D)), runs the filtered launch of every batch size named
// on the command line in interleaved rounds inside ONE process (boxes of the pool differ by several per cent, and so do
// separate processes), times every launch with HIP events, reads the in-kernel clock of the tile kernel and prints an
// order-independent checksum of the survivor records (the same for two builds that compute the same thing).
//
//   kbench [--rows N] [--dim D] [--rounds R] [--reps K] [--thr T] [--bf16] [--rotate] [queries ...]      default: 1024
//   (<= 128 queries: the streaming kernel; 129 .. 256: the tile kernel with nt gallery pieces; more: the tile kernel)
//
// Build: see scripts/kbench_build.sh.  It compiles the library's own sources unchanged: what it times is the product.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../image-search-engine-for-historical-research_amd/csrc/kernels.h"

using namespace mi;

#define CK(e)                                                                      \
  do {                                                                             \
    hipError_t _e = (e);                                                           \
    if (_e != hipSuccess) {                                                        \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #e, hipGetErrorString(_e)); \
      exit(2);                                                                     \
    }                                                                              \
  } while (0)

__device__ __forceinline__ uint64_t mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// element e of the image: approximately N(0, scale^2) (sum of four uniforms), stored as fp16 or bf16
__global__ void fill_image(uint16_t* img, size_t count, uint64_t seed, float scale, int f16) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const uint64_t h = mix(seed ^ (i * 0x2545F4914F6CDD1Dull));
    float u = 0.f;
    for (int j = 0; j < 4; ++j) u += (float)((h >> (16 * j)) & 0xFFFF) * (1.0f / 65536.0f);
    const float v = (u - 2.0f) * 1.7320508f * scale;   // var of sum of 4 U(0,1) = 1/3
    uint16_t bits;
    if (f16) {
      const _Float16 hv = (_Float16)v;
      bits = *reinterpret_cast<const uint16_t*>(&hv);
    } else {
      const uint32_t ub = __float_as_uint(v);
      bits = (uint16_t)((ub + 0x7FFFu + ((ub >> 16) & 1u)) >> 16);
    }
    img[i] = bits;
  }
}

__global__ void fill_f32(float* p, int n, float v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// order-independent checksum of the survivor records of one launch
__global__ void rec_checksum(const SurvRec* rec, const uint32_t* rec_cnt, uint32_t rec_cap, uint32_t nseg,
                             unsigned long long* out2) {
  const uint32_t seg = blockIdx.x;
  if (seg >= nseg) return;
  const uint32_t n = min(rec_cnt[seg], rec_cap);
  unsigned long long s = 0, c = 0;
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    const SurvRec r = rec[(size_t)seg * rec_cap + i];
    s += mix(((uint64_t)r.q << 40) ^ ((uint64_t)r.row << 8) ^ ((uint64_t)__float_as_uint(r.score) * 0x9E3779B1ull));
    c += 1;
  }
  atomicAdd(&out2[0], s);
  atomicAdd(&out2[1], c);
}

struct Batch {
  int nq = 0;
  std::vector<float> ms;
  unsigned long long sum = 0, cnt = 0;
  double mhz = 0, cps = 0;        // tile kernel: median in-kernel clock, loop cycles per K-slice
};

int main(int argc, char** argv) {
  int64_t rows = 1005994;
  int d = 2048, rounds = 3, reps = 5, f16 = 1, rotate = 0;
  float thr = 0.0663f;
  std::vector<Batch> vs;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto next = [&]() { return std::string(i + 1 < argc ? argv[++i] : "0"); };
    if (a == "--rows") rows = atoll(next().c_str());
    else if (a == "--dim") d = atoi(next().c_str());
    else if (a == "--rounds") rounds = atoi(next().c_str());
    else if (a == "--reps") reps = atoi(next().c_str());
    else if (a == "--thr") thr = (float)atof(next().c_str());
    else if (a == "--bf16") f16 = 0;
    else if (a == "--rotate") rotate = 1;     // round r starts at batch r: no batch is always the one behind the same neighbour
    else if (atoi(a.c_str()) >= 1 && atoi(a.c_str()) <= 1024) { vs.emplace_back(); vs.back().nq = atoi(a.c_str()); }
    else { fprintf(stderr, "kbench: %s is neither an option nor a batch size of 1 .. 1024 queries\n", a.c_str()); return 2; }
  }
  if (vs.empty()) { vs.emplace_back(); vs.back().nq = 1024; }
  const int dp = (int)round_up(d, BK);
  const int64_t npad = round_up(rows, TILE), ntiles = npad / TILE;
  const int qmax = 1024;
  const int nsl = dp / SLICE_K;
  const size_t gal_elems = (size_t)npad * dp, q_elems = (size_t)qmax * dp;
  uint16_t *gal = nullptr, *qry = nullptr;
  CK(hipMalloc((void**)&gal, gal_elems * 2 + 256));
  CK(hipMalloc((void**)&qry, q_elems * 2 + 256));
  const float scale = 1.0f / std::sqrt((float)d);
  hipLaunchKernelGGL(fill_image, dim3(4096), dim3(256), 0, 0, gal, gal_elems, 0x1234ull, scale, f16);
  hipLaunchKernelGGL(fill_image, dim3(512), dim3(256), 0, 0, qry, q_elems, 0x9876ull, scale, f16);
  QueryState st{};
  CK(hipMalloc((void**)&st.thr, qmax * 4));
  CK(hipMalloc((void**)&st.margin, qmax * 4));
  CK(hipMalloc((void**)&st.thr2, qmax * 4));
  CK(hipMalloc((void**)&st.qflag, qmax * 4));
  CK(hipMalloc((void**)&st.cnt, (size_t)qmax * CNT_STRIDE * 4));
  CK(hipMalloc((void**)&st.flags, 16));
  CK(hipMemset(st.flags, 0, 16));
  st.repair = st.flags + 1;
  CK(hipMemset(st.cnt, 0, (size_t)qmax * CNT_STRIDE * 4));
  st.cap = 12288;
  st.surv = nullptr;                                     // only a bootstrap launch writes survivors directly
  const uint32_t nseg = gemm_select_grid() * 8, rec_cap = 4096;
  SurvRec* rec = nullptr;
  uint32_t* rec_cnt = nullptr;
  unsigned long long *dbg = nullptr, *chk = nullptr;
  CK(hipMalloc((void**)&rec, (size_t)nseg * rec_cap * sizeof(SurvRec)));
  CK(hipMalloc((void**)&rec_cnt, nseg * 4));
  CK(hipMalloc((void**)&dbg, (size_t)nseg * 8 * 8));
  CK(hipMalloc((void**)&chk, 16));
  CK(hipDeviceSynchronize());

  ScoreArgs a{};
  a.gal_img = gal;
  a.qry_img = qry;
  a.img_f16 = f16;
  a.nslices = nsl;
  a.tile0 = 0;
  a.ntiles = (int32_t)ntiles;
  a.n = rows;
  a.small_batch_kernel = 1;
  a.rec = rec;
  a.rec_cnt = rec_cnt;
  a.rec_cap = rec_cap;
  a.cond = nullptr;
  a.dbg = dbg;
  a.st = st;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  printf("# rows=%lld d=%d tiles=%lld slices=%d thr=%.4f %s grid=%u\n", (long long)rows, d, (long long)ntiles, nsl, thr,
         f16 ? "f16" : "bf16", nseg / 8);
  for (int r = 0; r < rounds; ++r)
    for (size_t vi = 0; vi < vs.size(); ++vi) {
      auto& v = vs[(vi + (rotate ? (size_t)r : 0)) % vs.size()];
      a.nq = v.nq;
      a.nqt = (int32_t)(round_up(v.nq, TILE) / TILE);
      hipLaunchKernelGGL(fill_f32, dim3(qmax / 256), dim3(256), 0, 0, st.thr, qmax, INFINITY);   // padded queries keep nothing
      hipLaunchKernelGGL(fill_f32, dim3((v.nq + 255) / 256), dim3(256), 0, 0, st.thr, v.nq, thr);
      CK(hipMemset(rec_cnt, 0, nseg * 4));
      CK(hipMemset(dbg, 0, (size_t)nseg * 8 * 8));
      launch_gemm_select(a, false, nullptr);   // warm-up of this launch (code + clocks)
      CK(hipDeviceSynchronize());
      for (int k = 0; k < reps; ++k) {
        CK(hipEventRecord(e0, nullptr));
        launch_gemm_select(a, false, nullptr);
        CK(hipEventRecord(e1, nullptr));
        CK(hipEventSynchronize(e1));
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        v.ms.push_back(ms);
      }
      CK(hipGetLastError());
      CK(hipMemset(chk, 0, 16));
      hipLaunchKernelGGL(rec_checksum, dim3(nseg), dim3(256), 0, 0, rec, rec_cnt, rec_cap, nseg, chk);
      unsigned long long h[2];
      CK(hipMemcpy(h, chk, 16, hipMemcpyDeviceToHost));
      v.sum = h[0];
      v.cnt = h[1];
      // the tile kernel's per-wave words (word 5 = K-slices, 6 = shader cycles, 7 = 10-ns ticks around the main loop)
      std::vector<unsigned long long> c((size_t)nseg * 8);
      CK(hipMemcpy(c.data(), dbg, c.size() * 8, hipMemcpyDeviceToHost));
      std::vector<double> mhz, cps;
      for (uint32_t w = 0; w < nseg; ++w)
        if (c[(size_t)w * 8 + 7] > 0 && c[(size_t)w * 8 + 5] > 0) {
          mhz.push_back((double)c[(size_t)w * 8 + 6] / (double)c[(size_t)w * 8 + 7] * 100.0);
          cps.push_back((double)c[(size_t)w * 8 + 6] / (double)c[(size_t)w * 8 + 5]);
        }
      if (!mhz.empty()) {
        std::sort(mhz.begin(), mhz.end());
        std::sort(cps.begin(), cps.end());
        v.mhz = mhz[mhz.size() / 2];
        v.cps = cps[cps.size() / 2];
      }
    }
  for (auto& v : vs) {
    std::vector<float> m = v.ms;
    std::sort(m.begin(), m.end());
    const double med = m[m.size() / 2], mn = m.front(), flops = 2.0 * v.nq * (double)rows * d;
    printf("q=%-5d median %.4f ms = %7.1f TF   min %.4f ms = %7.1f TF   clock %.0f MHz, %.0f cycles/slice   records=%llu sum=%016llx\n",
           v.nq, med, flops / med / 1e9, mn, flops / mn / 1e9, v.mhz, v.cps, v.cnt, v.sum);
  }
  return 0;
}
