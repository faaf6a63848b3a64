// dpp64_rate.hip -- issue rate of the 64-bit DPP forms the column prox broadcasts with, against plain v_fma_f64 (gfx950):
//   fma       16 independent v_fma_f64 per loop trip
//   fmac_dpp  16 independent v_fmac_f64_dpp row_newbcast:n (operand 0 = lane n of the reader's row of 16)
//   mov_fma   16 pairs v_mov_b64_dpp row_newbcast:n + v_fma_f64 on the moved value
// each on ONE wave and on 12 waves of one workgroup (three per SIMD of one CU).  Times are HIP events around one launch; cycles are
// time x the reported clock, so read the RATIOS first.  Prints one JSON line.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/dpp64_rate.hip -o tools/micro/dpp64_rate.bin
#include <hip/hip_runtime.h>
#include <stdio.h>

#define NACC 16
#define FMAC_DPP(Q) asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc[Q]) : "v"(e), "v"(b), "i"(Q))
#define MOV_FMA(Q) acc[Q] = fma(__longlong_as_double(__builtin_amdgcn_update_dpp(0LL, ei, 0x150 + Q, 0xF, 0xF, true)), b, acc[Q])

template <int FORM>      // 0: fma, 1: fmac_dpp, 2: mov_dpp + fma
__global__ void __launch_bounds__(768) k_rate(double* out, int iters) {
  double acc[NACC];
#pragma unroll
  for (int q = 0; q < NACC; ++q) acc[q] = 1e-3 * (q + threadIdx.x);
  double e = 1.0 + 1e-12 * threadIdx.x;
  const double b = 1e-13;
  for (int it = 0; it < iters; ++it) {
    if constexpr (FORM == 0) {
#pragma unroll
      for (int q = 0; q < NACC; ++q) acc[q] = fma(e, b, acc[q]);
      asm volatile("" : "+v"(e));
    } else if constexpr (FORM == 1) {
      FMAC_DPP(0); FMAC_DPP(1); FMAC_DPP(2); FMAC_DPP(3); FMAC_DPP(4); FMAC_DPP(5); FMAC_DPP(6); FMAC_DPP(7);
      FMAC_DPP(8); FMAC_DPP(9); FMAC_DPP(10); FMAC_DPP(11); FMAC_DPP(12); FMAC_DPP(13); FMAC_DPP(14); FMAC_DPP(15);
    } else {
      asm volatile("" : "+v"(e));      // the moves stay in the loop
      const long long ei = __double_as_longlong(e);
      MOV_FMA(0); MOV_FMA(1); MOV_FMA(2); MOV_FMA(3); MOV_FMA(4); MOV_FMA(5); MOV_FMA(6); MOV_FMA(7);
      MOV_FMA(8); MOV_FMA(9); MOV_FMA(10); MOV_FMA(11); MOV_FMA(12); MOV_FMA(13); MOV_FMA(14); MOV_FMA(15);
    }
  }
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < NACC; ++q) s += acc[q];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <class F>
static double time_ms(F launch) {
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  launch(); (void)hipDeviceSynchronize();
  double best = 1e30;
  for (int r = 0; r < 5; ++r) {
    (void)hipEventRecord(e0); launch(); (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    if (ms < best) best = ms;
  }
  return best;
}

int main() {
  hipDeviceProp_t p; (void)hipGetDeviceProperties(&p, 0);
  double* out; if (hipMalloc(&out, sizeof(double) * 768) != hipSuccess) { fprintf(stderr, "no device memory\n"); return 1; }
  const int iters = 1 << 16;
  const double mhz = p.clockRate / 1000.0;
  double cyc[3][2];
  for (int wv = 0; wv < 2; ++wv) {
    const int threads = wv ? 768 : 64;
    const double ms[3] = {time_ms([&] { hipLaunchKernelGGL((k_rate<0>), dim3(1), dim3(threads), 0, 0, out, iters); }),
                          time_ms([&] { hipLaunchKernelGGL((k_rate<1>), dim3(1), dim3(threads), 0, 0, out, iters); }),
                          time_ms([&] { hipLaunchKernelGGL((k_rate<2>), dim3(1), dim3(threads), 0, 0, out, iters); })};
    // cycles per instruction (per pair for mov_fma) as one SIMD sees them: a SIMD runs 1 or 3 of the waves
    for (int f = 0; f < 3; ++f) cyc[f][wv] = ms[f] * 1e-3 * mhz * 1e6 / ((double)iters * NACC * (wv ? 3 : 1));
  }
  if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "device error\n"); return 1; }
  printf("{\"device\": \"%s\", \"clock_mhz\": %.0f, \"cycles_per_inst_1wave\": {\"fma\": %.2f, \"fmac_dpp\": %.2f, \"mov_fma_pair\": %.2f}, "
         "\"cycles_per_inst_3waves_per_simd\": {\"fma\": %.2f, \"fmac_dpp\": %.2f, \"mov_fma_pair\": %.2f}, "
         "\"fmac_dpp_over_fma\": [%.2f, %.2f], \"mov_fma_pair_over_fma\": [%.2f, %.2f]}\n",
         p.name, mhz, cyc[0][0], cyc[1][0], cyc[2][0], cyc[0][1], cyc[1][1], cyc[2][1],
         cyc[1][0] / cyc[0][0], cyc[1][1] / cyc[0][1], cyc[2][0] / cyc[0][0], cyc[2][1] / cyc[0][1]);
  (void)hipFree(out);
  return 0;
}
