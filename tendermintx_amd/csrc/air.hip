// The constraint quotient of the ladder rows (include/tmx.h "the constraint quotient of the ladder rows"): the pass over the extended
// ladder columns that turns the 33 polynomial constraints of every proof into one F_p^2 column pair, and the identity check at zeta from a
// batch proof's openings.  Field-only kernels (goldilocks_ext.hpp); gamma comes from phase 9 of k_fri_transcript (poseidon.hip).  No MFMA
// (nothing is a contraction).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "air.h"
#include "goldilocks_ext.hpp"

namespace tmx {

// Column offsets inside a proof's 65 columns; each point is x limbs, then y limbs
constexpr uint32_t L_BIT = 0, L_ACC = 1, L_DBL = 17, L_ADD = 33, L_NXT = 49, L_LIMBS = 16;

// One thread per table entry: the selector by i mod 256 B, 1 / (x^N - 1) by i mod B (one Fermat chain each), the 35 gamma powers.
__global__ __launch_bounds__(256) void k_air_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n256,
                                                    uint64_t w_n256, uint64_t om256_inv, const uint64_t* __restrict__ gamma, uint64_t* __restrict__ tab) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < (256u << log_blowup)) tab[AIR_TAB_SEL + k] = gl_sub(gl_mul(s_n256, gl_pow(w_n256, k)), om256_inv);
  if (k < (1u << log_blowup)) tab[AIR_TAB_ZINV + k] = gl_pow(gl_sub(gl_mul(s_n, gl_pow(w_n, k)), 1), GL_P - 2);
  if (k <= AIR_LADDER_CONSTRAINTS + 1) {
    const gl2 g = gl2_pow({gamma[0], gamma[1]}, k <= AIR_LADDER_CONSTRAINTS ? (uint64_t)k : AIR_LADDER_CONSTRAINTS * first_proof);
    tab[AIR_TAB_GPOW + 2 * k] = g.c0;
    tab[AIR_TAB_GPOW + 2 * k + 1] = g.c1;
  }
}

// The hot pass: every word of the table is read once (bit, dbl, add, nxt at the lane's row; acc at the NEXT row, 2^log_blowup words further
// along its column -- acc at the lane's own row is in no constraint).  One lane per row, a loop over the proofs from the last to the first
// (Horner by gamma^33), and inside it over the limbs four at a time: sixteen loads in flight per lane, all of them 64 consecutive words of
// one column per wave.  Only `bit` and the words of four limbs are live.  The gamma powers are wave-uniform table entries (scalar loads).
// Per proof  v = sum_(j < 17) gamma^j C_j + S(x) sum_(l < 16) gamma^(17 + l) (acc_l' - nxt_l)   (S is a base-field word: factored out),
// the products reduced (gl_mul), the sums lazy; then  t = t gamma^33 + v.  At the end  q = gamma^(33 first) t / (x^N - 1), written planar and
// canonical, or (ACC) added to what the buffer holds: a table fed in pieces of whole proofs.
constexpr int AIR_THREADS = 256, AIR_UNROLL = 4;
template <bool ACC>
__global__ __launch_bounds__(AIR_THREADS) void k_air_ladder_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs,
                                                                     const uint64_t* __restrict__ cols, const uint64_t* __restrict__ tab,
                                                                     uint64_t* __restrict__ out) {
  const uint64_t M = 1ull << log_m, i = (uint64_t)blockIdx.x * AIR_THREADS + threadIdx.x;
  if (i >= M) return;
  const uint64_t nx = (i + (1ull << log_blowup)) & (M - 1);
  const uint64_t* __restrict__ gp = tab + AIR_TAB_GPOW;
  uint64_t h0 = 0, h1 = 0;
  if (ACC) {  // (requested before the pass: its latency hides behind the column loop)
    h0 = out[i];
    h1 = out[M + i];
  }
  const uint64_t sel = tab[AIR_TAB_SEL + (i & ((256ull << log_blowup) - 1))];
  const uint64_t zinv = tab[AIR_TAB_ZINV + (i & ((1ull << log_blowup) - 1))];
  const gl2 g33 = {gp[2 * AIR_LADDER_CONSTRAINTS], gp[2 * AIR_LADDER_CONSTRAINTS + 1]};
  gl2 t = {0, 0};
  for (uint32_t p = n_proofs; p-- > 0;) {
    const uint64_t* __restrict__ c = cols + (((uint64_t)p * AIR_LADDER_WIDTH) << log_m);
    const uint64_t bit = gl_canon(__builtin_nontemporal_load(c + i));
    uint64_t a0 = gl_sub(gl_mul(bit, bit), bit), a1 = 0, b0 = 0, b1 = 0;  // (gamma^0 = (1, 0))
#pragma unroll 1
    for (uint32_t l0 = 0; l0 < L_LIMBS; l0 += AIR_UNROLL) {
      uint64_t acc[AIR_UNROLL], dbl[AIR_UNROLL], add[AIR_UNROLL], nxt[AIR_UNROLL];
#pragma unroll
      for (uint32_t k = 0; k < AIR_UNROLL; k++) {
        acc[k] = __builtin_nontemporal_load(c + ((uint64_t)(L_ACC + l0 + k) << log_m) + nx);
        dbl[k] = __builtin_nontemporal_load(c + ((uint64_t)(L_DBL + l0 + k) << log_m) + i);
        add[k] = __builtin_nontemporal_load(c + ((uint64_t)(L_ADD + l0 + k) << log_m) + i);
        nxt[k] = __builtin_nontemporal_load(c + ((uint64_t)(L_NXT + l0 + k) << log_m) + i);
      }
#pragma unroll
      for (uint32_t k = 0; k < AIR_UNROLL; k++) {
        const uint32_t l = l0 + k;
        const uint64_t d = gl_canon(dbl[k]), n = gl_canon(nxt[k]);
        const uint64_t c1 = gl_sub(gl_sub(n, d), gl_mul(bit, gl_sub(gl_canon(add[k]), d)));
        const uint64_t c2 = gl_sub(gl_canon(acc[k]), n);
        a0 = gl_add_lazy(a0, gl_mul(gp[2 * (1 + l)], c1));
        a1 = gl_add_lazy(a1, gl_mul(gp[2 * (1 + l) + 1], c1));
        b0 = gl_add_lazy(b0, gl_mul(gp[2 * (17 + l)], c2));
        b1 = gl_add_lazy(b1, gl_mul(gp[2 * (17 + l) + 1], c2));
      }
    }
    const gl2 v = {gl_add(gl_canon(a0), gl_mul(sel, b0)), gl_add(gl_canon(a1), gl_mul(sel, b1))};
    t = gl2_add(gl2_mul(t, g33), v);
  }
  gl2 q = gl2_mul(gl2_scale(t, zinv), {gp[2 * (AIR_LADDER_CONSTRAINTS + 1)], gp[2 * (AIR_LADDER_CONSTRAINTS + 1) + 1]});
  if (ACC) q = gl2_add(q, {gl_canon(h0), gl_canon(h1)});
  out[i] = q.c0;
  out[M + i] = q.c1;
}

// The identity at zeta, one workgroup: thread t takes the proofs t, t + 256, ...; per proof the 33 constraints over F_p^2 from the trace's
// openings at zeta (y0) and zeta omega_N (y1: acc only), weighted with gamma^(33 p + j); the sums meet in LDS.  Thread 0 compares with
// (u_0 + X u_1) (zeta^N - 1), X (a, b) = (7 b, a); on a mismatch every query's verdict is cleared.  Opening words are taken mod p.
constexpr int AIR_CHECK_THREADS = 256;
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_ladder_check(uint32_t n_proofs, uint32_t log_r, uint32_t log_sub, uint64_t om256_inv,
                                                                        const uint64_t* __restrict__ open_t, const uint64_t* __restrict__ open_q,
                                                                        const uint64_t* __restrict__ zeta, const uint64_t* __restrict__ gamma,
                                                                        uint32_t n_queries, uint32_t* __restrict__ ok) {
  __shared__ uint64_t red[2][AIR_CHECK_THREADS];
  __shared__ uint32_t holds;
  const uint32_t t = threadIdx.x;
  const uint64_t R = 1ull << log_r;
  const gl2 g = {gamma[0], gamma[1]}, z = {zeta[0], zeta[1]};
  gl2 zp = z;  // zeta^(N/256), then S(zeta)
  for (uint32_t k = 8; k < log_sub; k++) zp = gl2_mul(zp, zp);
  const gl2 S = {gl_sub(zp.c0, om256_inv), zp.c1};
  auto y0 = [&](uint64_t c) -> gl2 { return {gl_canon(open_t[c]), gl_canon(open_t[R + c])}; };
  auto y1 = [&](uint64_t c) -> gl2 { return {gl_canon(open_t[2 * R + c]), gl_canon(open_t[3 * R + c])}; };
  gl2 sum = {0, 0};
  for (uint32_t p = t; p < n_proofs; p += AIR_CHECK_THREADS) {
    const uint64_t c = (uint64_t)p * AIR_LADDER_WIDTH;
    gl2 gw = gl2_pow(g, (uint64_t)AIR_LADDER_CONSTRAINTS * p);
    const gl2 bit = y0(c + L_BIT);
    sum = gl2_add(sum, gl2_mul(gw, gl2_sub(gl2_mul(bit, bit), bit)));
    for (uint32_t l = 0; l < L_LIMBS; l++) {
      gw = gl2_mul(gw, g);
      const gl2 d = y0(c + L_DBL + l);
      sum = gl2_add(sum, gl2_mul(gw, gl2_sub(gl2_sub(y0(c + L_NXT + l), d), gl2_mul(bit, gl2_sub(y0(c + L_ADD + l), d)))));
    }
    for (uint32_t l = 0; l < L_LIMBS; l++) {
      gw = gl2_mul(gw, g);
      sum = gl2_add(sum, gl2_mul(gw, gl2_mul(S, gl2_sub(y1(c + L_ACC + l), y0(c + L_NXT + l)))));
    }
  }
  red[0][t] = sum.c0;
  red[1][t] = sum.c1;
  for (uint32_t h = AIR_CHECK_THREADS / 2; h; h >>= 1) {
    __syncthreads();
    if (t < h) {
      red[0][t] = gl_add(red[0][t], red[0][t + h]);
      red[1][t] = gl_add(red[1][t], red[1][t + h]);
    }
  }
  __syncthreads();
  if (t == 0) {
    gl2 zn = zp;  // zeta^N = (zeta^(N/256))^256
    for (uint32_t k = 0; k < 8; k++) zn = gl2_mul(zn, zn);
    const gl2 u0 = {gl_canon(open_q[0]), gl_canon(open_q[2])}, u1 = {gl_canon(open_q[1]), gl_canon(open_q[3])};
    const gl2 q = {gl_add(u0.c0, gl_mul(u1.c1, 7)), gl_add(u0.c1, u1.c0)};
    const gl2 rhs = gl2_mul(q, {gl_sub(zn.c0, 1), zn.c1});
    holds = gl2_eq({red[0][0], red[1][0]}, rhs) ? 1u : 0u;
  }
  __syncthreads();
  if (!holds)
    for (uint32_t q = t; q < n_queries; q += AIR_CHECK_THREADS) ok[q] = 0;
}

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

int launch_air_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n256, uint64_t w_n256, uint64_t om256_inv,
                      const void* d_gamma, void* d_tab, void* stream) {
  hipLaunchKernelGGL(k_air_tables, dim3(1u << log_blowup), dim3(256), 0, S_(stream), log_blowup, first_proof, s_n, w_n, s_n256, w_n256, om256_inv,
                     reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<uint64_t*>(d_tab));
  return (int)hipGetLastError();
}
int launch_air_ladder_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_tab, int accumulate,
                               void* d_quot, void* stream) {
  const dim3 grid((uint32_t)(((1ull << log_m) + AIR_THREADS - 1) / AIR_THREADS)), block(AIR_THREADS);
  const uint64_t* cols = reinterpret_cast<const uint64_t*>(d_cols);
  const uint64_t* tab = reinterpret_cast<const uint64_t*>(d_tab);
  uint64_t* out = reinterpret_cast<uint64_t*>(d_quot);
  if (accumulate) hipLaunchKernelGGL(k_air_ladder_quotient<true>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, tab, out);
  else hipLaunchKernelGGL(k_air_ladder_quotient<false>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, tab, out);
  return (int)hipGetLastError();
}
int launch_air_ladder_check(uint32_t n_proofs, uint32_t log_r, uint32_t log_sub, uint64_t om256_inv, const void* d_open_t, const void* d_open_q,
                            const void* d_zeta, const void* d_gamma, uint32_t n_queries, void* d_ok, void* stream) {
  hipLaunchKernelGGL(k_air_ladder_check, dim3(1), dim3(AIR_CHECK_THREADS), 0, S_(stream), n_proofs, log_r, log_sub, om256_inv,
                     reinterpret_cast<const uint64_t*>(d_open_t), reinterpret_cast<const uint64_t*>(d_open_q), reinterpret_cast<const uint64_t*>(d_zeta),
                     reinterpret_cast<const uint64_t*>(d_gamma), n_queries, reinterpret_cast<uint32_t*>(d_ok));
  return (int)hipGetLastError();
}

}  // namespace tmx
