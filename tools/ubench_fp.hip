// Field-multiplication throughput on gfx950: lazy-limb product scanning (fp.h, used by the
// kernels) vs saturated CIOS (fp_cios.h).  Prints modmul/s and cycles per wave-modmul.
// Then the LATENCY of one product in a dependent chain, one wave per SIMD: the per-lane fe_mul against the row-form
// fe_mul_row (fp_rows.h, one limb per lane), after checking the row routines against the per-lane ones on random and
// lazy operands.
#include <hip/hip_runtime.h>
#include <cstdio>
#include "../msm_zprize_amd/csrc/constants_gen.h"
#include "../msm_zprize_amd/csrc/fp.h"
#include "../msm_zprize_amd/csrc/fp_cios.h"
#include "../msm_zprize_amd/csrc/fp_rows.h"
#include <cstdlib>
#include <vector>
using namespace msmz;
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("HIP error %s at %d\n",hipGetErrorString(e),__LINE__);return 1;}}while(0)
constexpr int ITERS = 512;

template <class F, int MODE> __global__ void __launch_bounds__(256) k(uint32_t* io) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t w[F::NW];
  for (int i = 0; i < F::NW; i++) w[i] = io[i] + (i == 0 ? tid : 0);
  if (MODE == 0 || MODE == 2) {
    Fe<F> x, y; fe_unpack<F>(x, w); y = x; y.l[1] ^= 5;
    for (int it = 0; it < ITERS; it++) {
      if (MODE == 0) { fe_mul<F>(x, x, y); fe_mul<F>(y, y, x); }
      else { fe_sqr<F>(x, x); fe_sqr<F>(y, y); fe_add<F>(x, x, y); fe_carry<F>(x);} 
    }
    fe_add<F>(x, x, y); fe_store<F>(w, x);
  } else {
    uint32_t v[F::NW];
    for (int i = 0; i < F::NW; i++) v[i] = w[i] ^ 5;
    for (int it = 0; it < ITERS; it++) { cios_mul<F, 0xffffffffu>(w, w, v); cios_mul<F, 0xffffffffu>(v, v, w); }
    for (int i = 0; i < F::NW; i++) w[i] ^= v[i];
  }
  uint32_t s = 0; for (int i = 0; i < F::NW; i++) s ^= w[i];
  if (s == 0x12345) io[0] = s;
}

template <class F, int MODE> int run(const char* name, int bpc) {
  uint32_t* io; CK(hipMalloc(&io, 64)); CK(hipMemset(io, 0x11, 64));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  int grid = 256 * bpc;
  for (int i = 0; i < 3; i++) k<F, MODE><<<grid, 256>>>(io);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0));
  for (int r = 0; r < 5; r++) k<F, MODE><<<grid, 256>>>(io);
  CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= 5;
  double muls = (double)grid * 256 * ITERS * 2;
  double wave_muls_per_simd = muls / 64 / 1024;
  printf("%-28s blocks/CU=%d  %.3f ms  %.2f Gmodmul/s  %.0f cycles/wave-modmul/SIMD @2.4GHz\n", name, bpc, ms, muls / ms / 1e6, ms * 1e-3 * 2.4e9 / wave_muls_per_simd);
  return 0;
}

// ------------------------------------------------------------------------------------------------ dependent chains
constexpr int CHAIN = 64, CHAIN_REPS = 16;

template <class F, bool ROWS> __global__ void __launch_bounds__(256) k_chain(uint32_t* io) {
  uint32_t w[F::NW];
  for (int i = 0; i < F::NW; i++) w[i] = io[i];
  uint32_t s = 0;
  if (ROWS) {
    const RowLane<F> rk = row_lane<F>();
    int32_t x = fe_load_row<F>(io, rk), y = x ^ (rk.j == 1 ? 5 : 0);
    for (int rep = 0; rep < CHAIN_REPS; rep++) {
#pragma unroll 1
      for (int c = 0; c < CHAIN; c++) x = fe_mul_row<F>(x, y, rk);
    }
    s = (uint32_t)x;
  } else {
    Fe<F> x, y; fe_unpack<F>(x, w); y = x; y.l[1] ^= 5;
    for (int rep = 0; rep < CHAIN_REPS; rep++) {
#pragma unroll 1
      for (int c = 0; c < CHAIN; c++) fe_mul<F>(x, x, y);
    }
    for (int j = 0; j < F::N; j++) s ^= (uint32_t)x.l[j];
  }
  if (s == 0x12345) io[0] = s;
}

template <class F, bool ROWS> int run_chain(const char* name) {
  uint32_t* io; CK(hipMalloc(&io, 64)); CK(hipMemset(io, 0x01, 64));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int grid = 256;   // one 256-thread workgroup per CU: one wave on each SIMD
  for (int i = 0; i < 3; i++) k_chain<F, ROWS><<<grid, 256>>>(io);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0));
  for (int r = 0; r < 5; r++) k_chain<F, ROWS><<<grid, 256>>>(io);
  CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= 5;
  printf("chain %-28s %d x %d dependent products  %.3f ms  %.3f us/product\n", name, CHAIN_REPS, CHAIN, ms, ms * 1e3 / (CHAIN * CHAIN_REPS));
  CK(hipFree(io));
  return 0;
}

// ------------------------------------------------------------------------------------------------ row routines vs per-lane
// One wave per four operand pairs, row r of the wave works on pair 4 wave + r.  bad[] counts, per check:
//   0: (x - y)(x + y) differs   1: its square differs   2: an output limb outside the fe_mul contract
//   3: load -> store round trip differs   4: is-zero wrong
template <class F> __global__ void __launch_bounds__(64) k_check(const uint32_t* xs, const uint32_t* ys, unsigned* bad) {
  constexpr int NW = F::NW;
  __shared__ uint32_t sw[4][3][NW];
  const int row = threadIdx.x >> 4;
  const uint32_t* xw = xs + (size_t)(blockIdx.x * 4 + row) * NW;
  const uint32_t* yw = ys + (size_t)(blockIdx.x * 4 + row) * NW;
  const RowLane<F> rk = row_lane<F>();
  // per lane
  Fe<F> x, y, d, t, m, m2;
  fe_unpack<F>(x, xw); fe_unpack<F>(y, yw);
  fe_sub<F>(d, x, y); fe_add<F>(t, x, y);
  fe_mul<F>(m, d, t); fe_mul<F>(m2, m, m);
  uint32_t c1[NW], c2[NW], c3[NW];
  fe_to_canon_words<F>(c1, m); fe_to_canon_words<F>(c2, m2); fe_to_canon_words<F>(c3, x);
  // rows
  const int32_t rx = fe_load_row<F>(xw, rk), ry = fe_load_row<F>(yw, rk);
  const int32_t rm = fe_mul_row<F>(rx - ry, rx + ry, rk);
  const int32_t rm2 = fe_mul_row<F>(rm, rm, rk);
  const bool lowbad = rk.j < F::N - 1 ? ((uint32_t)rm >> F::W) != 0 || ((uint32_t)rm2 >> F::W) != 0 : (rk.j >= F::N && (rm | rm2) != 0);
  const bool topbad = rk.j == F::N - 1 && (rm != m.l[F::N - 1] && (rm < -64 || rm > 64));
  fe_store_row<F>(sw[row][0], rm, rk);
  fe_store_row<F>(sw[row][1], rm2, rk);
  fe_store_row<F>(sw[row][2], rx, rk);
  const bool z0 = fe_is_zero_row<F>(rx - rx, rk), z1 = fe_is_zero_row<F>(rk.pl, rk), z2 = fe_is_zero_row<F>(rk.p2 - rk.pl * 3, rk);
  const bool z3 = fe_is_zero_row<F>(rm, rk), z3ref = fe_is_zero_mod_p<F>(m);
  __syncthreads();
  if (lowbad || topbad) atomicAdd(&bad[2], 1u);
  if (rk.j == 0) {
    uint32_t r[NW];
    for (int v = 0; v < 3; v++) {
      for (int i = 0; i < NW; i++) r[i] = sw[row][v][i];
      words_canon<F>(r);
      const uint32_t* c = v == 0 ? c1 : v == 1 ? c2 : c3;
      if (!words_eq<NW>(r, c)) atomicAdd(&bad[v == 2 ? 3 : v], 1u);
    }
    if (!z0 || !z1 || !z2 || z3 != z3ref) atomicAdd(&bad[4], 1u);
  }
}

template <class F> int run_check(const char* name) {
  constexpr int NW = F::NW, PAIRS = 4096;
  std::vector<uint32_t> hx((size_t)PAIRS * NW), hy((size_t)PAIRS * NW);
  srand(12345);
  for (int i = 0; i < PAIRS; i++)
    for (int j = 0; j < NW; j++) {
      uint32_t a = ((uint32_t)rand() << 16) ^ (uint32_t)rand(), b = ((uint32_t)rand() << 16) ^ (uint32_t)rand();
      if (j == NW - 1) { a %= F::PW[NW - 1]; b %= F::PW[NW - 1]; }   // below p
      if (i == 0) a = b = 0;
      if (i == 1) b = a;
      hx[(size_t)i * NW + j] = a; hy[(size_t)i * NW + j] = b;
    }
  uint32_t *dx, *dy; unsigned* dbad; unsigned bad[5];
  CK(hipMalloc(&dx, hx.size() * 4)); CK(hipMalloc(&dy, hy.size() * 4)); CK(hipMalloc(&dbad, sizeof(bad)));
  CK(hipMemcpy(dx, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dy, hy.data(), hy.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemset(dbad, 0, sizeof(bad)));
  k_check<F><<<PAIRS / 4, 64>>>(dx, dy, dbad);
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(bad, dbad, sizeof(bad), hipMemcpyDeviceToHost));
  printf("check %-12s %d pairs: product %u, square of it %u, output limbs %u, round trip %u, is-zero %u mismatches\n", name, PAIRS,
         bad[0], bad[1], bad[2], bad[3], bad[4]);
  CK(hipFree(dx)); CK(hipFree(dy)); CK(hipFree(dbad));
  return (bad[0] | bad[1] | bad[2] | bad[3] | bad[4]) != 0;
}

int main(int argc, char** argv) {
  const bool chains_only = argc > 1 && argv[1][0] == 'c';
  if (run_check<Bls377Fp>("bls377") | run_check<PallasFp>("pallas")) { printf("row routines disagree with fp.h\n"); return 1; }
  run_chain<Bls377Fp, false>("bls377 lazy14x28 fe_mul");
  run_chain<Bls377Fp, true>("bls377 lazy14x28 fe_mul_row");
  run_chain<PallasFp, false>("pallas lazy9x29 fe_mul");
  run_chain<PallasFp, true>("pallas lazy9x29 fe_mul_row");
  if (chains_only) return 0;
  for (int bpc : {2, 4, 6, 8}) {
    run<Bls377Fp, 0>("bls377 lazy14x28 mul", bpc);
    run<Bls377Fp, 2>("bls377 lazy14x28 sqr", bpc);
    run<Bls377Fp, 1>("bls377 cios 12x32 mul", bpc);
    run<PallasFp, 0>("pallas lazy9x29 mul", bpc);
    run<PallasFp, 1>("pallas cios 8x32 mul", bpc);
    run<Bls381Fp, 0>("bls381 lazy14x28 mul", bpc);
  }
  return 0;
}
