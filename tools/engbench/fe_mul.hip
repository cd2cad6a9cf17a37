// One Fp12 product per item, R <- R * A, in both lane models:
//   lanes12  the engine's compiled E_XIA, E_MUL (engine_compiled.h): 12 lanes
//            per item, 5 items per wave, k_eng_fe_seg's LDS layout and launch
//            bounds (3 waves per SIMD)
//   lanes6   feseg6.cuh: one Fp2 coefficient per lane, Karatsuba inside the
//            lane, 10 items per wave, 2,016 bytes of LDS per item, 2 waves
//            per SIMD
// Every wave repeats the product `reps` times on random field elements in LDS
// (no plane loads from memory: the arithmetic alone), and the host reports ms
// per 1M item-products.  The go / no-go measurement for k_eng_fe_seg6.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Rpass-analysis=kernel-resource-usage -o fe_mul fe_mul.hip
//   fe_mul [reps]      -> one JSON line per lane model (FE_MUL_ONLY=lanes6|lanes12: that model alone)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../drand_amd/csrc/feseg6.cuh"

using namespace dgpu;

#define CK(x)                                                                          \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      exit(1);                                                                         \
    }                                                                                  \
  } while (0)

constexpr int W12 = ENG_LDS_SLOTS_FE * ENG_SLOT_WORDS;
constexpr int W6 = M6_ITEMS_PER_WAVE * M6_ITEM_WORDS;
static_assert(W6 * 4 * 8 <= 160 * 1024, "eight waves per CU fit the 160 KiB of LDS");

__global__ void __launch_bounds__(64, 3) k_mul12(int reps, const uint32_t* __restrict__ init, uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[W12];
  const uint32_t* src = init + (size_t)(blockIdx.x & 63) * W12;
  for (int t = threadIdx.x; t < W12; t += blockDim.x) lds[t] = src[t];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int gi = lane < 60 ? lane / 12 : 4;
  const int k = lane < 60 ? lane % 12 : lane - 60;
  uint32_t* c = lds;
  uint32_t* g = lds + ENG_GBASE_FE[gi] * ENG_SLOT_WORDS;
  uint32_t sink_acc = 0;
  auto snk = [&](uint32_t e, const fp& v) { sink_acc += v.l[0] ^ e; };
#pragma unroll 1
  for (int r = 0; r < reps; ++r) {
    eng_run_c2<false>(OP_E_XIA, g, c, k, snk);
    eng_run_c2<false>(OP_E_MUL, g, c, k, snk);
  }
  asm volatile("" ::: "memory");
  uint32_t h = sink_acc;
  for (int i = 0; i < ENG_SLOTS_FE * ENG_SLOT_WORDS; i += 64) h ^= g[(i + lane) % (ENG_SLOTS_FE * ENG_SLOT_WORDS)];
  out[(size_t)blockIdx.x * 64 + threadIdx.x] = h;
}

__global__ void __launch_bounds__(64, 2) k_mul6(int reps, const uint32_t* __restrict__ init, uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[W6];
  const uint32_t* src = init + (size_t)(blockIdx.x & 63) * W6;
  for (int t = threadIdx.x; t < W6; t += blockDim.x) lds[t] = src[t];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int gi = lane < 60 ? lane / M6_LANES : M6_ITEMS_PER_WAVE - 1;
  const int m = lane < 60 ? lane % M6_LANES : lane - 60;
  uint32_t* it = lds + gi * M6_ITEM_WORDS;
#pragma unroll 1
  for (int r = 0; r < reps; ++r) {
    // every lane's reads of an op issue before its writes, and one wave's LDS
    // queue is in order (engine.cuh eng_sync): a compiler fence orders the ops
    fp re, im;
    fs6_mul(it, m, re, im);
    asm volatile("" ::: "memory");
    m6_store(it, m, re, im);
    asm volatile("" ::: "memory");
  }
  uint32_t h = 0;
  for (int i = 0; i < M6_ITEM_WORDS; i += 64) h ^= it[(i + lane) % M6_ITEM_WORDS];
  out[(size_t)blockIdx.x * 64 + threadIdx.x] = h;
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 64;
  // lanes6: four full rounds of resident waves on 256 CUs, 8 per CU.  lanes12: the same count as at 12 per CU, but
  // its 14,224 B of LDS per wave (k_eng_fe_seg's footprint) let 11 fit in 160 KiB, so its grid is 4.4 rounds of 11
  const int blocks_of[2] = {256 * 12 * 4, 256 * 8 * 4};
  constexpr int WMAX = W12 > W6 ? W12 : W6;
  std::vector<uint32_t> h((size_t)64 * WMAX);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (size_t i = 0; i < h.size(); ++i) {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    const int limb = (int)(i % ENG_SLOT_WORDS);
    h[i] = limb == FP_LIMBS - 1 ? (uint32_t)(s % FP_P[FP_LIMBS - 1]) : (uint32_t)(s & FP_MASK);
  }
  uint32_t *d_init, *d_out;
  CK(hipMalloc(&d_init, h.size() * 4));
  CK(hipMalloc(&d_out, (size_t)blocks_of[0] * 64 * 4));
  CK(hipMemcpy(d_init, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const char* only = getenv("FE_MUL_ONLY");
  for (int model = 0; model < 2; ++model) {
    const char* name = model ? "lanes6" : "lanes12";
    if (only && strcmp(only, name)) continue;
    const int blocks = blocks_of[model];
    auto launch = [&](int r) {
      if (model) hipLaunchKernelGGL(k_mul6, dim3(blocks), dim3(64), 0, 0, r, d_init, d_out);
      else hipLaunchKernelGGL(k_mul12, dim3(blocks), dim3(64), 0, 0, r, d_init, d_out);
      CK(hipGetLastError());
    };
    launch(2);
    CK(hipDeviceSynchronize());
    float best = 1e30f, worst = 0.f;
    for (int rep = 0; rep < 5; ++rep) {
      CK(hipEventRecord(e0));
      launch(reps);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      best = ms < best ? ms : best;
      worst = ms > worst ? ms : worst;
    }
    const double products = (double)blocks * (model ? M6_ITEMS_PER_WAVE : ENG_GROUPS_PER_WAVE) * reps;
    printf("{\"model\": \"%s\", \"reps\": %d, \"ms_best\": %.3f, \"ms_worst\": %.3f, \"ms_per_1M_item_products\": %.4f}\n", name,
           reps, best, worst, best * 1e6 / products);
    fflush(stdout);
  }
  return 0;
}
