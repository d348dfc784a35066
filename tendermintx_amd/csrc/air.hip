// The constraint quotient of the ladder rows (include/tmx.h "the constraint quotient of the ladder rows"): the pass over the extended
// ladder columns that turns the 33 polynomial constraints of every proof into one F_p^2 column pair, and the identity check at zeta from a
// batch proof's openings.  Field-only kernels (goldilocks_ext.hpp); gamma comes from phase 9 of k_fri_transcript (poseidon.hip).  No MFMA
// (nothing is a contraction).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "air.h"
#include "goldilocks_ext.hpp"
#include "sha2.hpp"

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

// The end of every identity check, called by all the threads of the one workgroup: their sums meet in LDS, and thread 0 compares the
// total with (u_0 + X u_1) rhs, X (a, b) = (7 b, a), u the quotient's openings taken mod p; on a mismatch every query's verdict is cleared.
constexpr int AIR_CHECK_THREADS = 256;
__device__ __forceinline__ void air_check_verdict(gl2 sum, const uint64_t* __restrict__ open_q, gl2 rhs, uint32_t n_queries,
                                                  uint32_t* __restrict__ ok) {
  __shared__ uint64_t red[2][AIR_CHECK_THREADS];
  __shared__ uint32_t holds;
  const uint32_t t = threadIdx.x;
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
    const gl2 u0 = {gl_canon(open_q[0]), gl_canon(open_q[2])}, u1 = {gl_canon(open_q[1]), gl_canon(open_q[3])};
    const gl2 q = {gl_add(u0.c0, gl_mul(u1.c1, 7)), gl_add(u0.c1, u1.c0)};
    holds = gl2_eq({red[0][0], red[1][0]}, gl2_mul(q, rhs)) ? 1u : 0u;
  }
  __syncthreads();
  if (!holds)
    for (uint32_t q = t; q < n_queries; q += AIR_CHECK_THREADS) ok[q] = 0;
}

// The identity at zeta, one workgroup: thread t takes the proofs t, t + 256, ...; per proof the 33 constraints over F_p^2 from the trace's
// openings at zeta (y0) and zeta omega_N (y1: acc only), weighted with gamma^(33 p + j); the sum is compared with (u_0 + X u_1)
// (zeta^N - 1).  Opening words are taken mod p.
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_ladder_check(uint32_t n_proofs, uint32_t log_r, uint32_t log_sub, uint64_t om256_inv,
                                                                        const uint64_t* __restrict__ open_t, const uint64_t* __restrict__ open_q,
                                                                        const uint64_t* __restrict__ zeta, const uint64_t* __restrict__ gamma,
                                                                        uint32_t n_queries, uint32_t* __restrict__ ok) {
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
  gl2 zn = zp;  // zeta^N = (zeta^(N/256))^256
  for (uint32_t k = 0; k < 8; k++) zn = gl2_mul(zn, zn);
  air_check_verdict(sum, open_q, {gl_sub(zn.c0, 1), zn.c1}, n_queries, ok);
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

// ---- constraint set 2: the boundary constraints against a public table (include/tmx.h "the boundary constraints of the ladder rows") -------
// Set 1's kernels above stay as they are; these are siblings with tables of their own (air.h AIR2_TAB_*).

// As k_air_tables for 65 constraints per proof, plus 1 / S(x_i) by i mod 256 B (a second Fermat chain per selector entry).
__global__ __launch_bounds__(256) void k_air_boundary_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n256,
                                                             uint64_t w_n256, uint64_t om256_inv, const uint64_t* __restrict__ gamma,
                                                             uint64_t* __restrict__ tab) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < (256u << log_blowup)) {
    const uint64_t sel = gl_sub(gl_mul(s_n256, gl_pow(w_n256, k)), om256_inv);
    tab[AIR2_TAB_SEL + k] = sel;
    tab[AIR2_TAB_SINV + k] = gl_pow(sel, GL_P - 2);
  }
  if (k < (1u << log_blowup)) tab[AIR2_TAB_ZINV + k] = gl_pow(gl_sub(gl_mul(s_n, gl_pow(w_n, k)), 1), GL_P - 2);
  if (k <= AIR_BOUNDARY_CONSTRAINTS + 2) {
    const gl2 g = gl2_pow({gamma[0], gamma[1]}, k <= AIR_BOUNDARY_CONSTRAINTS + 1 ? (uint64_t)k : AIR_BOUNDARY_CONSTRAINTS * first_proof);
    tab[AIR2_TAB_GPOW + 2 * k] = g.c0;
    tab[AIR2_TAB_GPOW + 2 * k + 1] = g.c1;
  }
}

// One lane per (proof, ladder): the sixteen end words of the ladder from D.1b of its lane (sB for the even ladder, hA for the odd one), and
// live = the words are not all zero.  Ladders beyond 2 n_max are padding: all zero.  Lanes run over the ladders, so each of the 17 stores
// of a wave covers consecutive words of one column.
__global__ __launch_bounds__(256) void k_air_public_gather(const uint64_t* __restrict__ rows, uint64_t elem_stride, uint32_t d1b_start,
                                                           uint32_t lane_elems, uint32_t point_off, uint32_t n_max, uint32_t log_k, uint32_t n_proofs,
                                                           uint64_t* __restrict__ pub) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((uint64_t)n_proofs << log_k)) return;
  const uint32_t p = (uint32_t)(idx >> log_k), k = (uint32_t)(idx & ((1u << log_k) - 1));
  uint64_t w[L_LIMBS], any = 0;
#pragma unroll
  for (uint32_t l = 0; l < L_LIMBS; l++) w[l] = 0;
  if (k < 2 * n_max) {
    const uint64_t* __restrict__ src = rows + (uint64_t)p * elem_stride + d1b_start + (uint64_t)(k >> 1) * lane_elems + point_off + L_LIMBS * (k & 1);
#pragma unroll
    for (uint32_t l = 0; l < L_LIMBS; l++) {
      w[l] = gl_canon(src[l]);
      any |= w[l];
    }
  }
  uint64_t* __restrict__ dst = pub + (((uint64_t)p * AIR_PUBLIC_WIDTH) << log_k) + k;
#pragma unroll
  for (uint32_t l = 0; l < L_LIMBS; l++) dst[(uint64_t)l << log_k] = w[l];
  dst[(uint64_t)L_LIMBS << log_k] = any ? 1 : 0;
}

// V_k, one lane per k: per proof  W_p = sum_l gamma^(33 + l) pub[17 p + l][k] + gamma^57 pub[17 p + 16][(k + 1) mod K], Horner over the
// proofs by gamma^65.  pub is column-major: a wave reads 64 consecutive words per column; the 26 gamma powers sit in LDS, wave-uniform.
__global__ __launch_bounds__(256) void k_air_public_combine(uint32_t log_k, uint32_t n_proofs, const uint64_t* __restrict__ pub,
                                                            const uint64_t* __restrict__ gamma, uint64_t* __restrict__ v) {
  __shared__ uint64_t gw[2 * 26];  // gamma^33 .. gamma^57, then gamma^65
  if (threadIdx.x < 26) {
    const gl2 g = gl2_pow({gamma[0], gamma[1]}, threadIdx.x < 25 ? 33 + threadIdx.x : AIR_BOUNDARY_CONSTRAINTS);
    gw[2 * threadIdx.x] = g.c0;
    gw[2 * threadIdx.x + 1] = g.c1;
  }
  __syncthreads();
  const uint32_t K = 1u << log_k, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const uint32_t kn = (k + 1) & (K - 1);
  const gl2 g65 = {gw[50], gw[51]};
  gl2 t = {0, 0};
  for (uint32_t p = n_proofs; p-- > 0;) {
    const uint64_t* __restrict__ c = pub + (((uint64_t)p * AIR_PUBLIC_WIDTH) << log_k);
    uint64_t w0 = 0, w1 = 0;
#pragma unroll 4
    for (uint32_t l = 0; l < L_LIMBS; l++) {
      const uint64_t x = gl_canon(c[((uint64_t)l << log_k) + k]);
      w0 = gl_add_lazy(w0, gl_mul(gw[2 * l], x));
      w1 = gl_add_lazy(w1, gl_mul(gw[2 * l + 1], x));
    }
    const uint64_t live = gl_canon(c[((uint64_t)L_LIMBS << log_k) + kn]);
    w0 = gl_add_lazy(w0, gl_mul(gw[48], live));
    w1 = gl_add_lazy(w1, gl_mul(gw[49], live));
    t = gl2_add(gl2_mul(t, g65), {gl_canon(w0), gl_canon(w1)});
  }
  v[2 * k] = t.c0;
  v[2 * k + 1] = t.c1;
}

__global__ __launch_bounds__(256) void k_air_public_twiddles(uint32_t log_k, uint64_t om_k, uint64_t* __restrict__ tw) {
  const uint32_t half = 1u << (log_k - 1), e = blockIdx.x * 256 + threadIdx.x;
  if (e >= half) return;
  const uint64_t f = gl_pow(om_k, e);
  tw[e] = f;
  tw[half + e] = gl_pow(f, GL_P - 2);
}

// A size-K transform of two planes in LDS, in place: the caller stored element j at the bit-reversed j, the stages are decimation in time,
// out[b] = sum_j in[j] om^(j b) in natural order (tw[e] = om^e, e < K / 2).  Every thread of the workgroup calls it.  Bank behaviour
// (ds_read_b64 / ds_write_b64: 32 resp. 16 lanes per group over 64 banks of 4 B): from half-size 32 on a group's lanes touch consecutive
// 8-byte words, conflict-free; the first five stages step by two words inside a half-size and meet 2-way conflicts.  Left as it is: the
// kernel is launch-sized next to the hot pass (docs/kernels.md).
__device__ __forceinline__ void air_lds_transform(uint64_t* a0, uint64_t* a1, uint32_t log_k, const uint64_t* __restrict__ tw) {
  const uint32_t half = 1u << (log_k - 1);
  for (uint32_t s = 0; s < log_k; s++) {
    __syncthreads();
    const uint32_t h = 1u << s;
    for (uint32_t t = threadIdx.x; t < half; t += blockDim.x) {
      const uint32_t pos = t & (h - 1), i0 = ((t >> s) << (s + 1)) + pos, i1 = i0 + h;
      const uint64_t w = tw[pos << (log_k - 1 - s)];
      const uint64_t u0 = a0[i0], v0 = gl_mul(a0[i1], w), u1 = a1[i0], v1 = gl_mul(a1[i1], w);
      a0[i0] = gl_add(u0, v0);
      a0[i1] = gl_sub(u0, v0);
      a1[i0] = gl_add(u1, v1);
      a1[i1] = gl_sub(u1, v1);
    }
  }
  __syncthreads();
}
__device__ __forceinline__ uint32_t air_bitrev(uint32_t j, uint32_t log_k) { return __brev(j) >> (32 - log_k); }

// The coefficients of Pub_gamma, one workgroup: V_k = Pub(om^255 om_K^k) = sum_j (c_j om^(255 j)) om_K^(j k), so an inverse transform of V
// gives d_j = c_j om^(255 j) and c_j = d_j om^(-255 j).  2 K words of dynamic LDS.
constexpr int AIR_PUB_THREADS = 256;
__global__ __launch_bounds__(AIR_PUB_THREADS) void k_air_public_coefs(uint32_t log_k, uint64_t k_inv, uint64_t om255_inv, const uint64_t* __restrict__ v,
                                                                      const uint64_t* __restrict__ tw, uint64_t* __restrict__ coef) {
  extern __shared__ uint64_t air_lds[];
  const uint32_t K = 1u << log_k;
  uint64_t *a0 = air_lds, *a1 = air_lds + K;
  for (uint32_t j = threadIdx.x; j < K; j += AIR_PUB_THREADS) {
    const uint32_t r = air_bitrev(j, log_k);
    a0[r] = gl_canon(v[2 * j]);
    a1[r] = gl_canon(v[2 * j + 1]);
  }
  air_lds_transform(a0, a1, log_k, tw + (K >> 1));
  uint64_t f = gl_mul(k_inv, gl_pow(om255_inv, threadIdx.x));
  const uint64_t step = gl_pow(om255_inv, AIR_PUB_THREADS);
  for (uint32_t j = threadIdx.x; j < K; j += AIR_PUB_THREADS, f = gl_mul(f, step)) {
    coef[j] = gl_mul(a0[j], f);
    coef[K + j] = gl_mul(a1[j], f);
  }
}

// Pub_gamma on the whole coset.  The points x_(a + (M / K) b) = x_a om_K^b, b < K, are a coset of the K-subgroup: Pub there is the size-K
// transform of c_j x_a^j.  A workgroup takes 2^log_a consecutive a (2 K 2^log_a words of dynamic LDS, at most 64 KB) so that its stores are
// runs of 2^log_a consecutive words: lanes run over (b, a) with a fastest.
__global__ __launch_bounds__(AIR_PUB_THREADS) void k_air_public_extend(uint32_t log_m, uint32_t log_k, uint32_t log_a, uint64_t s, uint64_t w,
                                                                       const uint64_t* __restrict__ coef, const uint64_t* __restrict__ tw,
                                                                       uint64_t* __restrict__ ext) {
  extern __shared__ uint64_t air_lds[];
  const uint32_t K = 1u << log_k, A = 1u << log_a;
  const uint64_t M = 1ull << log_m, a_base = (uint64_t)blockIdx.x << log_a;
  uint64_t xa = gl_mul(s, gl_pow(w, a_base));
  for (uint32_t al = 0; al < A; al++, xa = gl_mul(xa, w)) {
    uint64_t *a0 = air_lds + (size_t)al * 2 * K, *a1 = a0 + K;
    uint64_t xj = gl_pow(xa, threadIdx.x);
    const uint64_t step = gl_pow(xa, AIR_PUB_THREADS);
    for (uint32_t j = threadIdx.x; j < K; j += AIR_PUB_THREADS, xj = gl_mul(xj, step)) {
      const uint32_t r = air_bitrev(j, log_k);
      a0[r] = gl_mul(coef[j], xj);
      a1[r] = gl_mul(coef[K + j], xj);
    }
    air_lds_transform(a0, a1, log_k, tw);
  }
  for (uint32_t idx = threadIdx.x; idx < (K << log_a); idx += AIR_PUB_THREADS) {
    const uint32_t al = idx & (A - 1), b = idx >> log_a;
    const uint64_t i = a_base + al + ((uint64_t)b << (log_m - log_k));
    const uint64_t* a0 = air_lds + (size_t)al * 2 * K;
    ext[i] = a0[b];
    ext[M + i] = a0[K + b];
  }
}

// The set-2 hot pass: k_air_ladder_quotient's access shape (one lane per row, every table word read once) with a second Horner accumulator
// over the proofs, by gamma^65, for the boundary sum  w_p = sum_l gamma^(33 + l) nxt_l + gamma^(49 + l) acc_l'  (four more reduced products
// per limb on words the pass already holds).  At the end
//   q = gamma^(65 first) (t / (x^N - 1) + u / S(x)) - Pub_gamma(x) / S(x)
// the last term only where pubext is set: the piece that starts at proof 0.
template <bool ACC>
__global__ __launch_bounds__(AIR_THREADS) void k_air_ladder_boundary_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs,
                                                                              const uint64_t* __restrict__ cols, const uint64_t* __restrict__ tab,
                                                                              const uint64_t* __restrict__ pubext, uint64_t* __restrict__ out) {
  const uint64_t M = 1ull << log_m, i = (uint64_t)blockIdx.x * AIR_THREADS + threadIdx.x;
  if (i >= M) return;
  const uint64_t nx = (i + (1ull << log_blowup)) & (M - 1);
  const uint64_t* __restrict__ gp = tab + AIR2_TAB_GPOW;
  uint64_t h0 = 0, h1 = 0, e0 = 0, e1 = 0;
  if (ACC) {
    h0 = out[i];
    h1 = out[M + i];
  }
  if (pubext) {
    e0 = pubext[i];
    e1 = pubext[M + i];
  }
  const uint64_t sel = tab[AIR2_TAB_SEL + (i & ((256ull << log_blowup) - 1))];
  const uint64_t sinv = tab[AIR2_TAB_SINV + (i & ((256ull << log_blowup) - 1))];
  const uint64_t zinv = tab[AIR2_TAB_ZINV + (i & ((1ull << log_blowup) - 1))];
  const gl2 g65 = {gp[2 * AIR_BOUNDARY_CONSTRAINTS], gp[2 * AIR_BOUNDARY_CONSTRAINTS + 1]};
  gl2 t = {0, 0}, u = {0, 0};
  for (uint32_t p = n_proofs; p-- > 0;) {
    const uint64_t* __restrict__ c = cols + (((uint64_t)p * AIR_LADDER_WIDTH) << log_m);
    const uint64_t bit = gl_canon(__builtin_nontemporal_load(c + i));
    uint64_t a0 = gl_sub(gl_mul(bit, bit), bit), a1 = 0, b0 = 0, b1 = 0, w0 = 0, w1 = 0;
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
        const uint64_t d = gl_canon(dbl[k]), n = gl_canon(nxt[k]), a = gl_canon(acc[k]);
        const uint64_t c1 = gl_sub(gl_sub(n, d), gl_mul(bit, gl_sub(gl_canon(add[k]), d)));
        const uint64_t c2 = gl_sub(a, n);
        a0 = gl_add_lazy(a0, gl_mul(gp[2 * (1 + l)], c1));
        a1 = gl_add_lazy(a1, gl_mul(gp[2 * (1 + l) + 1], c1));
        b0 = gl_add_lazy(b0, gl_mul(gp[2 * (17 + l)], c2));
        b1 = gl_add_lazy(b1, gl_mul(gp[2 * (17 + l) + 1], c2));
        w0 = gl_add_lazy(gl_add_lazy(w0, gl_mul(gp[2 * (33 + l)], n)), gl_mul(gp[2 * (49 + l)], a));
        w1 = gl_add_lazy(gl_add_lazy(w1, gl_mul(gp[2 * (33 + l) + 1], n)), gl_mul(gp[2 * (49 + l) + 1], a));
      }
    }
    const gl2 v = {gl_add(gl_canon(a0), gl_mul(sel, b0)), gl_add(gl_canon(a1), gl_mul(sel, b1))};
    t = gl2_add(gl2_mul(t, g65), v);
    u = gl2_add(gl2_mul(u, g65), {gl_canon(w0), gl_canon(w1)});
  }
  gl2 q = gl2_mul(gl2_add(gl2_scale(t, zinv), gl2_scale(u, sinv)),
                  {gp[2 * (AIR_BOUNDARY_CONSTRAINTS + 2)], gp[2 * (AIR_BOUNDARY_CONSTRAINTS + 2) + 1]});
  if (pubext) q = gl2_sub(q, gl2_scale({gl_canon(e0), gl_canon(e1)}, sinv));
  if (ACC) q = gl2_add(q, {gl_canon(h0), gl_canon(h1)});
  out[i] = q.c0;
  out[M + i] = q.c1;
}

// The set-2 identity at zeta, one workgroup, division-free with Z = zeta^N - 1:
//   S(zeta) main + Z (bsum - Pub_gamma(zeta)) == (u_0 + X u_1) Z S(zeta)
// main: set 1's 33 constraints with the weights gamma^(65 p + j); bsum: the boundary columns' openings; Pub_gamma(zeta) barycentric over the
// K <= 2^12 points y_k = om255 om_K^k from the verifier's own V: thread t takes k = t, t + 256, ... (at most 16) and inverts its zeta - y_k
// with one F_p^2 inversion (prefix products, one Fermat chain, back-substitution).  zeta lies outside F_p, so no zeta - y_k is zero.
constexpr int AIR_BARY_PER = (1 << AIR_PUBLIC_MAX_LOG_K) / AIR_CHECK_THREADS;
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_ladder_boundary_check(uint32_t n_proofs, uint32_t log_r, uint32_t log_sub, uint64_t om256_inv,
                                                                                 uint64_t om255, uint64_t om_k, uint64_t bary_inv,
                                                                                 const uint64_t* __restrict__ open_t, const uint64_t* __restrict__ open_q,
                                                                                 const uint64_t* __restrict__ zeta, const uint64_t* __restrict__ gamma,
                                                                                 const uint64_t* __restrict__ vk, uint32_t n_queries,
                                                                                 uint32_t* __restrict__ ok) {
  const uint32_t t = threadIdx.x, K = 1u << (log_sub - 8);
  const uint64_t R = 1ull << log_r;
  const gl2 g = {gamma[0], gamma[1]}, z = {zeta[0], zeta[1]};
  gl2 zp = z;  // zeta^(N/256), then S(zeta)
  for (uint32_t k = 8; k < log_sub; k++) zp = gl2_mul(zp, zp);
  const gl2 S = {gl_sub(zp.c0, om256_inv), zp.c1};
  auto y0 = [&](uint64_t c) -> gl2 { return {gl_canon(open_t[c]), gl_canon(open_t[R + c])}; };
  auto y1 = [&](uint64_t c) -> gl2 { return {gl_canon(open_t[2 * R + c]), gl_canon(open_t[3 * R + c])}; };
  gl2 sum = {0, 0}, bsum = {0, 0}, psum = {0, 0};
  for (uint32_t p = t; p < n_proofs; p += AIR_CHECK_THREADS) {
    const uint64_t c = (uint64_t)p * AIR_LADDER_WIDTH;
    gl2 gw = gl2_pow(g, (uint64_t)AIR_BOUNDARY_CONSTRAINTS * p);
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
    for (uint32_t l = 0; l < L_LIMBS; l++) {
      gw = gl2_mul(gw, g);
      bsum = gl2_add(bsum, gl2_mul(gw, y0(c + L_NXT + l)));
    }
    for (uint32_t l = 0; l < L_LIMBS; l++) {
      gw = gl2_mul(gw, g);
      bsum = gl2_add(bsum, gl2_mul(gw, y1(c + L_ACC + l)));
    }
  }
  {
    gl2 pre[AIR_BARY_PER];
    uint64_t yk[AIR_BARY_PER];
    gl2 run = {1, 0};
    const uint64_t stride = gl_pow(om_k, AIR_CHECK_THREADS);
    uint64_t y = gl_mul(om255, gl_pow(om_k, t));
#pragma unroll
    for (int m = 0; m < AIR_BARY_PER; m++) {
      const bool in = t + m * AIR_CHECK_THREADS < K;
      yk[m] = y;
      pre[m] = run;
      if (in) run = gl2_mul(run, {gl_sub(z.c0, y), z.c1});
      y = gl_mul(y, stride);
    }
    gl2 inv = gl2_inv(run);
#pragma unroll
    for (int m = AIR_BARY_PER - 1; m >= 0; m--) {
      const uint32_t k = t + m * AIR_CHECK_THREADS;
      if (k < K) {
        const gl2 di = gl2_mul(inv, pre[m]);  // 1 / (zeta - y_k)
        inv = gl2_mul(inv, {gl_sub(z.c0, yk[m]), z.c1});
        const gl2 V = {gl_canon(vk[2 * k]), gl_canon(vk[2 * k + 1])};
        psum = gl2_add(psum, gl2_mul(gl2_scale(V, yk[m]), di));
      }
    }
  }
  gl2 zn = zp;  // zeta^N = (zeta^(N/256))^256
  for (uint32_t k = 0; k < 8; k++) zn = gl2_mul(zn, zn);
  const gl2 Z = {gl_sub(zn.c0, 1), zn.c1};
  // (the left side is linear in the three sums and S, Z are uniform: every thread folds its own share, and one sum meets in LDS)
  const gl2 pub = gl2_mul(gl2_scale(S, bary_inv), psum);
  air_check_verdict(gl2_add(gl2_mul(S, sum), gl2_mul(Z, gl2_sub(bsum, pub))), open_q, gl2_mul(Z, S), n_queries, ok);
}

int launch_air_boundary_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n256, uint64_t w_n256,
                               uint64_t om256_inv, const void* d_gamma, void* d_tab, void* stream) {
  hipLaunchKernelGGL(k_air_boundary_tables, dim3(1u << log_blowup), dim3(256), 0, S_(stream), log_blowup, first_proof, s_n, w_n, s_n256, w_n256,
                     om256_inv, reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<uint64_t*>(d_tab));
  return (int)hipGetLastError();
}
int launch_air_public_gather(const void* d_rows, uint64_t elem_stride, uint32_t d1b_start, uint32_t lane_elems, uint32_t point_off, uint32_t n_max,
                             uint32_t log_k, uint32_t n_proofs, void* d_pub, void* stream) {
  const uint64_t n = (uint64_t)n_proofs << log_k;
  hipLaunchKernelGGL(k_air_public_gather, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S_(stream), reinterpret_cast<const uint64_t*>(d_rows),
                     elem_stride, d1b_start, lane_elems, point_off, n_max, log_k, n_proofs, reinterpret_cast<uint64_t*>(d_pub));
  return (int)hipGetLastError();
}
int launch_air_public_combine(uint32_t log_k, uint32_t n_proofs, const void* d_pub, const void* d_gamma, void* d_v, void* stream) {
  hipLaunchKernelGGL(k_air_public_combine, dim3(((1u << log_k) + 255) / 256), dim3(256), 0, S_(stream), log_k, n_proofs,
                     reinterpret_cast<const uint64_t*>(d_pub), reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<uint64_t*>(d_v));
  return (int)hipGetLastError();
}
int launch_air_public_twiddles(uint32_t log_k, uint64_t om_k, void* d_tw, void* stream) {
  hipLaunchKernelGGL(k_air_public_twiddles, dim3(((1u << (log_k - 1)) + 255) / 256), dim3(256), 0, S_(stream), log_k, om_k,
                     reinterpret_cast<uint64_t*>(d_tw));
  return (int)hipGetLastError();
}
int launch_air_public_coefs(uint32_t log_k, uint64_t k_inv, uint64_t om255_inv, const void* d_v, const void* d_tw, void* d_coef, void* stream) {
  hipLaunchKernelGGL(k_air_public_coefs, dim3(1), dim3(AIR_PUB_THREADS), (size_t)16 << log_k, S_(stream), log_k, k_inv, om255_inv,
                     reinterpret_cast<const uint64_t*>(d_v), reinterpret_cast<const uint64_t*>(d_tw), reinterpret_cast<uint64_t*>(d_coef));
  return (int)hipGetLastError();
}
int launch_air_public_extend(uint32_t log_m, uint32_t log_k, uint64_t s, uint64_t w, const void* d_coef, const void* d_tw, void* d_ext, void* stream) {
  // 2^log_a points a per workgroup: at most 8 (64-byte runs), within 64 KB of LDS, and no more than there are
  uint32_t log_a = 3;
  if (log_a > AIR_PUBLIC_MAX_LOG_K - log_k) log_a = AIR_PUBLIC_MAX_LOG_K - log_k;
  if (log_a > log_m - log_k) log_a = log_m - log_k;
  hipLaunchKernelGGL(k_air_public_extend, dim3(1u << (log_m - log_k - log_a)), dim3(AIR_PUB_THREADS), (size_t)16 << (log_k + log_a), S_(stream), log_m,
                     log_k, log_a, s, w, reinterpret_cast<const uint64_t*>(d_coef), reinterpret_cast<const uint64_t*>(d_tw),
                     reinterpret_cast<uint64_t*>(d_ext));
  return (int)hipGetLastError();
}
int launch_air_ladder_boundary_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_tab,
                                        const void* d_pubext, int accumulate, void* d_quot, void* stream) {
  const dim3 grid((uint32_t)(((1ull << log_m) + AIR_THREADS - 1) / AIR_THREADS)), block(AIR_THREADS);
  const uint64_t* cols = reinterpret_cast<const uint64_t*>(d_cols);
  const uint64_t* tab = reinterpret_cast<const uint64_t*>(d_tab);
  const uint64_t* pe = reinterpret_cast<const uint64_t*>(d_pubext);
  uint64_t* out = reinterpret_cast<uint64_t*>(d_quot);
  if (accumulate) hipLaunchKernelGGL(k_air_ladder_boundary_quotient<true>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, tab, pe, out);
  else hipLaunchKernelGGL(k_air_ladder_boundary_quotient<false>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, tab, pe, out);
  return (int)hipGetLastError();
}
int launch_air_ladder_boundary_check(uint32_t n_proofs, uint32_t log_r, uint32_t log_sub, uint64_t om256_inv, uint64_t om255, uint64_t om_k,
                                     uint64_t bary_inv, const void* d_open_t, const void* d_open_q, const void* d_zeta, const void* d_gamma,
                                     const void* d_v, uint32_t n_queries, void* d_ok, void* stream) {
  hipLaunchKernelGGL(k_air_ladder_boundary_check, dim3(1), dim3(AIR_CHECK_THREADS), 0, S_(stream), n_proofs, log_r, log_sub, om256_inv, om255, om_k,
                     bary_inv, reinterpret_cast<const uint64_t*>(d_open_t), reinterpret_cast<const uint64_t*>(d_open_q),
                     reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<const uint64_t*>(d_v),
                     n_queries, reinterpret_cast<uint32_t*>(d_ok));
  return (int)hipGetLastError();
}

// ---- constraint sets 3, 4 and 5: the SHA-256 tables ------------------------------------------------------------------------------------------
// Siblings of the ladder sets: nothing above changes.  Every constraint of these sets is written once, in an evaluator templated on a field
// policy and on a view of "one proof at one point".  The hot pass instantiates it over F_p at a coset point (CosetView), the identity check
// over F_p^2 at zeta (ZetaView): prover and verifier agree term for term and index for index because they are the same source.  How a
// kernel combines a proof's gamma sums stays in the kernel: there the hot passes and the checks differ on purpose (sets 7 - 9, whose
// selectors are columns: in the two views' `combined`).

// The two field policies: F_p on canonical words, and F_p^2.  scale and add_const take a base-field constant.
struct FieldP {
  using T = uint64_t;
  static __device__ __forceinline__ T zero() { return 0; }
  static __device__ __forceinline__ T add(T a, T b) { return gl_add(a, b); }
  static __device__ __forceinline__ T sub(T a, T b) { return gl_sub(a, b); }
  static __device__ __forceinline__ T mul(T a, T b) { return gl_mul(a, b); }
  static __device__ __forceinline__ T scale(T a, uint64_t s) { return gl_mul(a, s); }
  static __device__ __forceinline__ T add_const(T a, uint64_t k) { return gl_add(a, k); }
};
struct FieldP2 {
  using T = gl2;
  static __device__ __forceinline__ T zero() { return {0, 0}; }
  static __device__ __forceinline__ T add(T a, T b) { return gl2_add(a, b); }
  static __device__ __forceinline__ T sub(T a, T b) { return gl2_sub(a, b); }
  static __device__ __forceinline__ T mul(T a, T b) { return gl2_mul(a, b); }
  static __device__ __forceinline__ T scale(T a, uint64_t s) { return gl2_scale(a, s); }
  static __device__ __forceinline__ T add_const(T a, uint64_t k) { return {gl_add(a.c0, k), a.c1}; }
};
// A policy with the small forms the three sets share
template <class F>
struct Forms : F {
  using T = typename F::T;
  static __device__ __forceinline__ T boolean(T x) { return F::sub(F::mul(x, x), x); }
  static __device__ __forceinline__ T exor(T x, T y) {  // x + y - 2 x y
    const T xy = F::mul(x, y);
    return F::sub(F::add(x, y), F::add(xy, xy));
  }
  static __device__ __forceinline__ T dbl_add(T s, T x) { return F::add(F::add(s, s), x); }
  static __device__ __forceinline__ T c32(T x0, T x1, T x2) {  // the carry word 2^32 (x0 + 2 x1 + 4 x2)
    return F::scale(F::add(x0, F::add(F::add(x1, x1), F::scale(x2, 4))), 1ull << 32);
  }
};

// One proof at one point of the coset, for a hot pass: c and h are the proof's table and helper columns, i the lane's point and nx the
// point of the next row, 2^log_blowup words further along every column.  Every word is read from HBM once (`once`, non-temporal); `again`
// is for the columns the evaluator reads more than once per lane, through the cache, `next` for the words at nx.  Words are taken mod p.
// The gamma sums are lazy pairs against the gamma table gp (wave-uniform entries: scalar loads): a the plain sum; b the selected sum of
// set 3, or the start sum of set 5; c the chain sum of set 5.  The evaluator's loops are unrolled as the hot passes want them.
struct CosetView {
  static constexpr uint32_t BITS = 2, SHORT = 16;  // (16: every short loop in full)
  const uint64_t* __restrict__ c;
  const uint64_t* __restrict__ h;
  const uint64_t* __restrict__ gp;
  uint32_t log_m;
  uint64_t i, nx;
  uint64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0, c0 = 0, c1 = 0;
  __device__ __forceinline__ uint64_t once(uint32_t col) const { return gl_canon(__builtin_nontemporal_load(h + ((uint64_t)col << log_m) + i)); }
  __device__ __forceinline__ uint64_t again(uint32_t col) const { return gl_canon(h[((uint64_t)col << log_m) + i]); }
  __device__ __forceinline__ uint64_t next(uint32_t col) const { return gl_canon(h[((uint64_t)col << log_m) + nx]); }
  __device__ __forceinline__ uint64_t tbl(uint32_t col) const { return gl_canon(c[((uint64_t)col << log_m) + i]); }
  __device__ __forceinline__ uint64_t tbl_next(uint32_t col) const { return gl_canon(c[((uint64_t)col << log_m) + nx]); }
  __device__ __forceinline__ void weigh(uint64_t& s0, uint64_t& s1, uint32_t j, uint64_t v) const {
    s0 = gl_add_lazy(s0, gl_mul(gp[2 * j], v));
    s1 = gl_add_lazy(s1, gl_mul(gp[2 * j + 1], v));
  }
  __device__ __forceinline__ void plain(uint32_t j, uint64_t v) { weigh(a0, a1, j, v); }
  __device__ __forceinline__ void selected(uint32_t j, uint64_t v) { weigh(b0, b1, j, v); }
  __device__ __forceinline__ void started(uint32_t j, uint64_t v) { weigh(b0, b1, j, v); }
  __device__ __forceinline__ void chained(uint32_t j, uint64_t v) { weigh(c0, c1, j, v); }
  // A proof's value where the selectors are columns (sets 7 - 9): a + s[0] b, with SUMS = 2 also + s[1] c; s the selectors at the point
  template <uint32_t SUMS>
  __device__ __forceinline__ gl2 combined(const uint64_t* s) const {
    gl2 v = {gl_add(gl_canon(a0), gl_mul(s[0], b0)), gl_add(gl_canon(a1), gl_mul(s[0], b1))};
    if (SUMS == 2) v = {gl_add(v.c0, gl_mul(s[1], c0)), gl_add(v.c1, gl_mul(s[1], c1))};
    return v;
  }
};

// One proof at zeta, for an identity check: t and h are the proof's columns inside the table's and the helper's openings blocks, whose
// planes lie R words apart: the value at zeta in planes 0 and 1, at zeta omega_N (`next`) in planes 2 and 3.  The gamma powers are in
// LDS; the sums a, b, c are CosetView's, over F_p^2.  No unrolling: a check kernel is one workgroup and must not grow.
struct ZetaView {
  static constexpr uint32_t BITS = 1, SHORT = 1;
  const uint64_t* __restrict__ t;
  const uint64_t* __restrict__ h;
  uint64_t RT, RH;
  const uint64_t* gpw;
  gl2 a = {0, 0}, b = {0, 0}, c = {0, 0};
  __device__ __forceinline__ gl2 once(uint32_t col) const { return {gl_canon(h[col]), gl_canon(h[RH + col])}; }
  __device__ __forceinline__ gl2 again(uint32_t col) const { return once(col); }
  __device__ __forceinline__ gl2 next(uint32_t col) const { return {gl_canon(h[2 * RH + col]), gl_canon(h[3 * RH + col])}; }
  __device__ __forceinline__ gl2 tbl(uint32_t col) const { return {gl_canon(t[col]), gl_canon(t[RT + col])}; }
  __device__ __forceinline__ gl2 tbl_next(uint32_t col) const { return {gl_canon(t[2 * RT + col]), gl_canon(t[3 * RT + col])}; }
  __device__ __forceinline__ gl2 weight(uint32_t j) const { return {gpw[2 * j], gpw[2 * j + 1]}; }
  __device__ __forceinline__ void plain(uint32_t j, gl2 v) { a = gl2_add(a, gl2_mul(weight(j), v)); }
  __device__ __forceinline__ void selected(uint32_t j, gl2 v) { b = gl2_add(b, gl2_mul(weight(j), v)); }
  __device__ __forceinline__ void started(uint32_t j, gl2 v) { b = gl2_add(b, gl2_mul(weight(j), v)); }
  __device__ __forceinline__ void chained(uint32_t j, gl2 v) { c = gl2_add(c, gl2_mul(weight(j), v)); }
  template <uint32_t SUMS>  // (CosetView::combined over F_p^2)
  __device__ __forceinline__ gl2 combined(const gl2* s) const {
    gl2 v = gl2_mul(s[0], b);
    if (SUMS == 2) v = gl2_add(v, gl2_mul(s[1], c));
    return gl2_add(a, v);
  }
};

// gamma^0 .. gamma^n into LDS, the workgroup's threads striding over the powers; the caller's next barrier completes it
__device__ __forceinline__ void air_gamma_powers(gl2 g, uint32_t n, uint64_t* gpw) {
  for (uint32_t k = threadIdx.x; k <= n; k += AIR_CHECK_THREADS) {
    const gl2 gk = gl2_pow(g, k);
    gpw[2 * k] = gk.c0;
    gpw[2 * k + 1] = gk.c1;
  }
}

// The polynomial of degree < 64 with P(omega_64^t) = val(t), into LDS: thread j < 64 takes coefficient j, an inverse transform written out
// (64 terms; launch-sized work).  Every thread of the workgroup calls it, and it ends with a barrier; 64^-1 = p - (p - 1) / 64.
template <class Val>
__device__ __forceinline__ void air_interpolate64(uint64_t om64_inv, uint64_t* coef, Val val) {
  if (threadIdx.x < 64) {
    const uint64_t step = gl_pow(om64_inv, threadIdx.x);
    uint64_t cur = 1, acc = 0;
    for (uint32_t t = 0; t < 64; t++, cur = gl_mul(cur, step)) acc = gl_add(acc, gl_mul(cur, val(t)));
    coef[threadIdx.x] = gl_mul(acc, GL_P - (GL_P - 1) / 64);
  }
  __syncthreads();
}
// P_K(omega_64^t) = K256[t]; P_F(omega_64^t) = 1 for 15 <= t <= 62 and 0 otherwise (the next row is a schedule row)
struct RoundConstant {
  __device__ __forceinline__ uint64_t operator()(uint32_t t) const { return K_SHA256[t]; }
};
struct ScheduleRow {
  __device__ __forceinline__ uint64_t operator()(uint32_t t) const { return t >= 15 && t <= 62 ? 1 : 0; }
};
// Such a polynomial at a point of F_p and of F_p^2
__device__ __forceinline__ uint64_t air_horner64(const uint64_t* coef, uint64_t y) {
  uint64_t acc = 0;
  for (int j = 63; j >= 0; j--) acc = gl_add(gl_mul(acc, y), coef[j]);
  return acc;
}
__device__ __forceinline__ gl2 air_horner64(const uint64_t* coef, gl2 y) {
  gl2 acc = {0, 0};
  for (int j = 63; j >= 0; j--) {
    acc = gl2_mul(acc, y);
    acc.c0 = gl_add(acc.c0, coef[j]);
  }
  return acc;
}

// Thread k's share of the two tables every one of these sets has: 1 / (x^N - 1) by i mod B (one Fermat chain), gamma^0 .. gamma^n and
// behind them gamma^(n first_proof), the weight of a piece whose first proof is proof first_proof of the table (k_air_tables' last entry)
__device__ __forceinline__ void air_zinv_gpow(uint32_t k, uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n,
                                              const uint64_t* __restrict__ gamma, uint32_t n, uint64_t* __restrict__ zinv,
                                              uint64_t* __restrict__ gpow) {
  if (k < (1u << log_blowup)) zinv[k] = gl_pow(gl_sub(gl_mul(s_n, gl_pow(w_n, k)), 1), GL_P - 2);
  if (k <= n + 1) {
    const gl2 g = gl2_pow({gamma[0], gamma[1]}, k <= n ? (uint64_t)k : n * first_proof);
    gpow[2 * k] = g.c0;
    gpow[2 * k + 1] = g.c1;
  }
}

// The round-bit machinery of sets 3 and 5.  It runs on six registers of a row in the roles a, b, c, e, f, g of the round function: set 3
// fills them with a, b, c, e, f, g themselves, set 5 with b, c, d, f, g, h (row 0 of a block is round 0 applied to the words the block
// starts from).  RoundBits holds the helper offsets of the six registers' bit columns, whose X^2 - X constraints have the same indices,
// and the helper offsets and constraint indices of U0, U1 and V.
struct RoundBits {
  uint32_t a, b, c, e, f, g, u0, u1, v, j_u0, j_u1, j_v;
};
template <class F>
struct RoundWords {
  typename F::T a, b, c, e, f, g, s0, s1, ch, maj;
};
// On the coset a bit column is a full field element, so a pass never holds the 288 bit words: it walks the bit index b from 31 down to 0
// and per b holds the nine bit words A_b .. V_b and the six rotated ones (A_(b+2), A_(b+13), A_(b+22), E_(b+6), E_(b+11), E_(b+25)), which
// are re-read through the cache (another b of the same lane reads them as its own).  Per b: nine constraints (six X^2 - X, U0, U1, V), and
// one Horner step by 2 of the ten word sums (the six registers, Sigma0, Sigma1, Ch, Maj), so that no power of two is multiplied: 13
// reduced column products and 18 gamma weights per b.  The word sums go back to the set's evaluator.
template <class F, class View>
__device__ __forceinline__ RoundWords<F> air_round_bits(View& at, const RoundBits r) {
  using A = Forms<F>;
  using T = typename F::T;
  RoundWords<F> w = {F::zero(), F::zero(), F::zero(), F::zero(), F::zero(), F::zero(), F::zero(), F::zero(), F::zero(), F::zero()};
#pragma unroll View::BITS
  for (uint32_t b = 32; b-- > 0;) {
    const T A_ = at.again(r.a + b), B = at.once(r.b + b), C = at.once(r.c + b), E = at.again(r.e + b), F_ = at.once(r.f + b), G = at.once(r.g + b);
    const T U0 = at.once(r.u0 + b), U1 = at.once(r.u1 + b), V = at.once(r.v + b);
    const T A2 = at.again(r.a + ((b + 2) & 31)), A13 = at.again(r.a + ((b + 13) & 31)), A22 = at.again(r.a + ((b + 22) & 31));
    const T E6 = at.again(r.e + ((b + 6) & 31)), E11 = at.again(r.e + ((b + 11) & 31)), E25 = at.again(r.e + ((b + 25) & 31));
    at.plain(r.a + b, A::boolean(A_));
    at.plain(r.b + b, A::boolean(B));
    at.plain(r.c + b, A::boolean(C));
    at.plain(r.e + b, A::boolean(E));
    at.plain(r.f + b, A::boolean(F_));
    at.plain(r.g + b, A::boolean(G));
    at.plain(r.j_u0 + b, A::sub(U0, A::exor(A2, A13)));
    at.plain(r.j_u1 + b, A::sub(U1, A::exor(E6, E11)));
    at.plain(r.j_v + b, A::sub(V, A::mul(A_, B)));
    w.a = A::dbl_add(w.a, A_);
    w.b = A::dbl_add(w.b, B);
    w.c = A::dbl_add(w.c, C);
    w.e = A::dbl_add(w.e, E);
    w.f = A::dbl_add(w.f, F_);
    w.g = A::dbl_add(w.g, G);
    w.s0 = A::dbl_add(w.s0, A::exor(U0, A22));
    w.s1 = A::dbl_add(w.s1, A::exor(U1, E25));
    w.ch = A::dbl_add(w.ch, A::add(G, A::mul(E, A::sub(F_, G))));
    w.maj = A::dbl_add(w.maj, A::add(V, A::mul(C, A::sub(A::add(A_, B), A::add(V, V)))));
  }
  return w;
}

// ---- constraint set 3: the round constraints of the SHA-256 tables (include/tmx.h "the round constraints of the SHA-256 tables") ------------
// Helper column offsets inside a proof's 300, and the constraint indices inside its 315.
constexpr uint32_t H_A = 0, H_B = 32, H_C = 64, H_E = 96, H_F = 128, H_G = 160, H_U0 = 192, H_U1 = 224, H_V = 256, H_S0 = 288, H_S1 = 289, H_CH = 290,
                   H_MAJ = 291, H_LIVE = 292, H_KL = 293, H_CA = 294, H_CE = 297;
constexpr uint32_t T_W = 0, T_A = 1, T_B = 2, T_C = 3, T_D = 4, T_E = 5, T_F = 6, T_G = 7, T_H = 8;
constexpr uint32_t J_CARRY = 192, J_LIVE = 198, J_WORD = 199, J_U0 = 205, J_U1 = 237, J_V = 269, J_S0 = 301, J_S1 = 302, J_CH = 303, J_MAJ = 304,
                   J_KL = 305, J_SHIFT = 306, J_LIVEN = 312, J_NA = 313, J_NE = 314;

// One lane per (proof, row) of the pre-LDE table: the nine words of the row, the block's first row (LIVE) and W of the next row (the
// carries), then 300 stores, each of them consecutive words of one column across the wave.  Operands are the low 32 bits of the words.
__global__ __launch_bounds__(256) void k_air_sha_helper(uint32_t log_rows, uint32_t n_proofs, const uint64_t* __restrict__ table,
                                                        uint64_t* __restrict__ helper) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((uint64_t)n_proofs << log_rows)) return;
  const uint32_t p = (uint32_t)(idx >> log_rows);
  const uint64_t r = idx & ((1ull << log_rows) - 1), r0 = r & ~63ull;
  const uint32_t rnd = (uint32_t)(r & 63);
  const uint64_t* __restrict__ t = table + (((uint64_t)p * AIR_SHA_WIDTH) << log_rows);
  uint32_t w[AIR_SHA_WIDTH];
  uint64_t any = 0;
#pragma unroll
  for (uint32_t c = 0; c < AIR_SHA_WIDTH; c++) {
    w[c] = (uint32_t)t[((uint64_t)c << log_rows) + r];
    any |= t[((uint64_t)c << log_rows) + r0];
  }
  const uint32_t live = any ? 1u : 0u;
  const uint32_t a = w[T_A], b = w[T_B], c = w[T_C], e = w[T_E], f = w[T_F], g = w[T_G];
  const uint32_t s0 = rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22), s1 = rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25);
  const uint32_t chv = (e & f) ^ (~e & g), mjv = (a & b) ^ (a & c) ^ (b & c);
  const uint32_t u0 = rotr32(a, 2) ^ rotr32(a, 13), u1 = rotr32(e, 6) ^ rotr32(e, 11), v = a & b;
  uint64_t* __restrict__ o = helper + (((uint64_t)p * AIR_SHA_HELPER_COLS) << log_rows) + r;
  auto put = [&](uint32_t col, uint64_t x) { o[(uint64_t)col << log_rows] = x; };
#pragma unroll 4
  for (uint32_t i = 0; i < 32; i++) {
    put(H_A + i, (a >> i) & 1);
    put(H_B + i, (b >> i) & 1);
    put(H_C + i, (c >> i) & 1);
    put(H_E + i, (e >> i) & 1);
    put(H_F + i, (f >> i) & 1);
    put(H_G + i, (g >> i) & 1);
    put(H_U0 + i, (u0 >> i) & 1);
    put(H_U1 + i, (u1 >> i) & 1);
    put(H_V + i, (v >> i) & 1);
  }
  put(H_S0, s0);
  put(H_S1, s1);
  put(H_CH, chv);
  put(H_MAJ, mjv);
  put(H_LIVE, live);
  put(H_KL, live ? K_SHA256[rnd] : 0u);
  uint32_t ca = 0, ce = 0;
  if (rnd != 63) {
    const uint32_t wn = (uint32_t)t[((uint64_t)T_W << log_rows) + r + 1];
    const uint64_t t1 = (uint64_t)w[T_H] + s1 + chv + (live ? K_SHA256[rnd + 1] : 0u) + wn;
    ca = (uint32_t)((t1 + s0 + mjv) >> 32) & 7;
    ce = (uint32_t)((t1 + w[T_D]) >> 32) & 7;
  }
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    put(H_CA + k, (ca >> k) & 1);
    put(H_CE + k, (ce >> k) & 1);
  }
}

// One thread per table entry: S and K by i mod 64 B (K by Horner on P_K's coefficients in LDS), 1 / (x^N - 1) by i mod B, gamma^0 .. 315.
__global__ __launch_bounds__(256) void k_air_sha_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n64, uint64_t w_n64,
                                                        uint64_t om64_inv, const uint64_t* __restrict__ gamma, uint64_t* __restrict__ tab) {
  __shared__ uint64_t pk[64];
  air_interpolate64(om64_inv, pk, RoundConstant{});
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < (64u << log_blowup)) {
    const uint64_t y = gl_mul(s_n64, gl_pow(w_n64, k));
    tab[AIR3_TAB_SEL + k] = gl_sub(y, om64_inv);
    tab[AIR3_TAB_K + k] = air_horner64(pk, y);
  }
  air_zinv_gpow(k, log_blowup, first_proof, s_n, w_n, gamma, AIR_SHA_CONSTRAINTS, tab + AIR3_TAB_ZINV, tab + AIR3_TAB_GPOW);
}

// The 315 constraints of one proof at one point; kx is K at the point.  Behind the bit loop 8 more column products, the word constraints
// and the nine selected ones, which go to a gamma sum of their own: S(x) is factored out of it, the kernel applies it once.
template <class F, class View>
__device__ __forceinline__ void air_sha_constraints(View& at, typename F::T kx) {
  using A = Forms<F>;
  using T = typename F::T;
  const RoundWords<F> w = air_round_bits<F>(at, {H_A, H_B, H_C, H_E, H_F, H_G, H_U0, H_U1, H_V, J_U0, J_U1, J_V});
  const T ta = at.tbl(T_A), tb = at.tbl(T_B), tc = at.tbl(T_C), td = at.tbl(T_D), te = at.tbl(T_E), tf = at.tbl(T_F), tg = at.tbl(T_G),
          th = at.tbl(T_H);
  at.plain(J_WORD + 0, A::sub(ta, w.a));
  at.plain(J_WORD + 1, A::sub(tb, w.b));
  at.plain(J_WORD + 2, A::sub(tc, w.c));
  at.plain(J_WORD + 3, A::sub(te, w.e));
  at.plain(J_WORD + 4, A::sub(tf, w.f));
  at.plain(J_WORD + 5, A::sub(tg, w.g));
  const T S0 = at.once(H_S0), S1 = at.once(H_S1), CH = at.once(H_CH), MAJ = at.once(H_MAJ), LIVE = at.again(H_LIVE), KL = at.again(H_KL);
  at.plain(J_S0, A::sub(S0, w.s0));
  at.plain(J_S1, A::sub(S1, w.s1));
  at.plain(J_CH, A::sub(CH, w.ch));
  at.plain(J_MAJ, A::sub(MAJ, w.maj));
  at.plain(J_LIVE, A::boolean(LIVE));
  at.plain(J_KL, A::sub(KL, A::mul(LIVE, kx)));
  T carry[6];
#pragma unroll View::SHORT
  for (uint32_t k = 0; k < 6; k++) {
    carry[k] = at.once(H_CA + k);
    at.plain(J_CARRY + k, A::boolean(carry[k]));
  }
  at.selected(J_SHIFT + 0, A::sub(at.tbl_next(T_B), ta));
  at.selected(J_SHIFT + 1, A::sub(at.tbl_next(T_C), tb));
  at.selected(J_SHIFT + 2, A::sub(at.tbl_next(T_D), tc));
  at.selected(J_SHIFT + 3, A::sub(at.tbl_next(T_F), te));
  at.selected(J_SHIFT + 4, A::sub(at.tbl_next(T_G), tf));
  at.selected(J_SHIFT + 5, A::sub(at.tbl_next(T_H), tg));
  at.selected(J_LIVEN, A::sub(at.next(H_LIVE), LIVE));
  const T kln = at.next(H_KL);
  const T t1 = A::add(A::add(A::add(th, S1), A::add(CH, kln)), at.tbl_next(T_W));
  at.selected(J_NA, A::sub(A::add(at.tbl_next(T_A), A::c32(carry[0], carry[1], carry[2])), A::add(t1, A::add(S0, MAJ))));
  at.selected(J_NE, A::sub(A::add(at.tbl_next(T_E), A::c32(carry[3], carry[4], carry[5])), A::add(td, t1)));
}

// The set-3 hot pass, k_air_ladder_quotient's shape: one lane per point, a loop over the proofs from the last to the first (Horner by
// gamma^315), the nine table columns and the 300 helper columns read once from HBM.  Per proof  v = a + S(x) b; at the end 1 / (x^N - 1).
// FORM: AIR_FORM_WHOLE is the whole table.  A piece (AIR_FORM_PIECE, AIR_FORM_PIECE_ACC) is n_proofs whole proofs whose first is proof
// `first` of the table: cols is that proof's table column 0, hcols the piece's own helper buffer, and the sum takes the weight
// gamma^(315 first), the table entry behind the powers.  _ACC adds what `out` holds, loaded behind the proof loop (sets 3 and 5 sit 31
// VGPRs under the two-wave limit: two more live words across the loop are not worth risking a wave), and writes the sum canonical.
template <int FORM>
__global__ __launch_bounds__(AIR_THREADS) void k_air_sha_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs,
                                                                  const uint64_t* __restrict__ cols, const uint64_t* __restrict__ hcols,
                                                                  const uint64_t* __restrict__ tab, uint64_t* __restrict__ out) {
  const uint64_t M = 1ull << log_m, i = (uint64_t)blockIdx.x * AIR_THREADS + threadIdx.x;
  if (i >= M) return;
  const uint64_t nx = (i + (1ull << log_blowup)) & (M - 1);
  const uint64_t* __restrict__ gp = tab + AIR3_TAB_GPOW;
  const uint64_t sel = tab[AIR3_TAB_SEL + (i & ((64ull << log_blowup) - 1))];
  const uint64_t kx = tab[AIR3_TAB_K + (i & ((64ull << log_blowup) - 1))];
  const uint64_t zinv = tab[AIR3_TAB_ZINV + (i & ((1ull << log_blowup) - 1))];
  const gl2 g315 = {gp[2 * AIR_SHA_CONSTRAINTS], gp[2 * AIR_SHA_CONSTRAINTS + 1]};
  gl2 t = {0, 0};
  for (uint32_t p = n_proofs; p-- > 0;) {
    CosetView at = {cols + (((uint64_t)p * AIR_SHA_WIDTH) << log_m), hcols + (((uint64_t)p * AIR_SHA_HELPER_COLS) << log_m), gp, log_m, i, nx};
    air_sha_constraints<FieldP>(at, kx);
    const gl2 v = {gl_add(gl_canon(at.a0), gl_mul(sel, at.b0)), gl_add(gl_canon(at.a1), gl_mul(sel, at.b1))};
    t = gl2_add(gl2_mul(t, g315), v);
  }
  gl2 q = gl2_scale(t, zinv);
  if (FORM != AIR_FORM_WHOLE) q = gl2_mul(q, {gp[2 * (AIR_SHA_CONSTRAINTS + 1)], gp[2 * (AIR_SHA_CONSTRAINTS + 1) + 1]});
  if (FORM == AIR_FORM_PIECE_ACC) q = gl2_add(q, {gl_canon(out[i]), gl_canon(out[M + i])});
  out[i] = q.c0;
  out[M + i] = q.c1;
}

// The set-3 identity at zeta, one workgroup: gamma^0 .. gamma^315 and P_K go to LDS first; thread t takes the proofs t, t + 256, ... and
// evaluates their 315 constraints over F_p^2 from the table's and the helper's openings; K(zeta) by Horner on P_K at zeta^(N/64).  A proof
// contributes gamma^(315 p) (a + S(zeta) b); the sum is compared with (u_0 + X u_1) (zeta^N - 1).
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_sha_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub,
                                                                      uint64_t om64_inv, const uint64_t* __restrict__ open_t,
                                                                      const uint64_t* __restrict__ open_h, const uint64_t* __restrict__ open_q,
                                                                      const uint64_t* __restrict__ zeta, const uint64_t* __restrict__ gamma,
                                                                      uint32_t n_queries, uint32_t* __restrict__ ok) {
  __shared__ uint64_t gpw[2 * (AIR_SHA_CONSTRAINTS + 1)];
  __shared__ uint64_t pk[64];
  const gl2 g = {gamma[0], gamma[1]};
  air_gamma_powers(g, AIR_SHA_CONSTRAINTS, gpw);
  air_interpolate64(om64_inv, pk, RoundConstant{});  // (ends with a barrier: gpw is complete behind it too)
  gl2 zp = {zeta[0], zeta[1]};  // zeta^(N/64)
  for (uint32_t k = 6; k < log_sub; k++) zp = gl2_mul(zp, zp);
  const gl2 S = {gl_sub(zp.c0, om64_inv), zp.c1}, K = air_horner64(pk, zp);
  gl2 sum = {0, 0};
  for (uint32_t p = threadIdx.x; p < n_proofs; p += AIR_CHECK_THREADS) {
    ZetaView at = {open_t + (uint64_t)p * AIR_SHA_WIDTH, open_h + (uint64_t)p * AIR_SHA_HELPER_COLS, 1ull << log_r_t, 1ull << log_r_h, gpw};
    air_sha_constraints<FieldP2>(at, K);
    sum = gl2_add(sum, gl2_mul(gl2_pow(g, (uint64_t)AIR_SHA_CONSTRAINTS * p), gl2_add(at.a, gl2_mul(S, at.b))));
  }
  gl2 zn = zp;  // zeta^N = (zeta^(N/64))^64
  for (uint32_t k = 0; k < 6; k++) zn = gl2_mul(zn, zn);
  air_check_verdict(sum, open_q, {gl_sub(zn.c0, 1), zn.c1}, n_queries, ok);
}

int launch_air_sha_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream) {
  const uint64_t n = (uint64_t)n_proofs << log_rows;
  hipLaunchKernelGGL(k_air_sha_helper, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S_(stream), log_rows, n_proofs,
                     reinterpret_cast<const uint64_t*>(d_table), reinterpret_cast<uint64_t*>(d_helper));
  return (int)hipGetLastError();
}
int launch_air_sha_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n64, uint64_t w_n64, uint64_t om64_inv, const void* d_gamma,
                          void* d_tab, void* stream) {
  // (at least two workgroups: the 317 gamma powers)
  const uint32_t blocks = ((64u << log_blowup) + 255) / 256;
  hipLaunchKernelGGL(k_air_sha_tables, dim3(blocks < 2 ? 2 : blocks), dim3(256), 0, S_(stream), log_blowup, first_proof, s_n, w_n, s_n64, w_n64, om64_inv,
                     reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<uint64_t*>(d_tab));
  return (int)hipGetLastError();
}
int launch_air_sha_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_helper_cols, const void* d_tab,
                            int form, void* d_quot, void* stream) {
  const dim3 grid((uint32_t)(((1ull << log_m) + AIR_THREADS - 1) / AIR_THREADS)), block(AIR_THREADS);
  const uint64_t* cols = reinterpret_cast<const uint64_t*>(d_cols);
  const uint64_t* hcols = reinterpret_cast<const uint64_t*>(d_helper_cols);
  const uint64_t* tab = reinterpret_cast<const uint64_t*>(d_tab);
  uint64_t* out = reinterpret_cast<uint64_t*>(d_quot);
  if (form == AIR_FORM_WHOLE)
    hipLaunchKernelGGL(k_air_sha_quotient<AIR_FORM_WHOLE>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, hcols, tab, out);
  else if (form == AIR_FORM_PIECE)
    hipLaunchKernelGGL(k_air_sha_quotient<AIR_FORM_PIECE>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, hcols, tab, out);
  else
    hipLaunchKernelGGL(k_air_sha_quotient<AIR_FORM_PIECE_ACC>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, hcols, tab, out);
  return (int)hipGetLastError();
}
int launch_air_sha_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint64_t om64_inv, const void* d_open_t,
                         const void* d_open_h, const void* d_open_q, const void* d_zeta, const void* d_gamma, uint32_t n_queries, void* d_ok,
                         void* stream) {
  hipLaunchKernelGGL(k_air_sha_check, dim3(1), dim3(AIR_CHECK_THREADS), 0, S_(stream), n_proofs, log_r_t, log_r_h, log_sub, om64_inv,
                     reinterpret_cast<const uint64_t*>(d_open_t), reinterpret_cast<const uint64_t*>(d_open_h),
                     reinterpret_cast<const uint64_t*>(d_open_q), reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<const uint64_t*>(d_gamma),
                     n_queries, reinterpret_cast<uint32_t*>(d_ok));
  return (int)hipGetLastError();
}

// ---- constraint set 4: the message schedule of the SHA-256 tables (include/tmx.h "the message schedule of the SHA-256 tables") --------------
// Helper column offsets inside a proof's 115 (Q_k at S_Q + k), constraint indices inside its 117 (Q_k's at JS_Q + k).
constexpr uint32_t S_WB = 0, S_X0 = 32, S_X1 = 64, S_G0 = 96, S_G1 = 97, S_Q = 97, S_CW = 113;
constexpr uint32_t JS_CW = 32, JS_WORD = 34, JS_X0 = 35, JS_X1 = 67, JS_G0 = 99, JS_G1 = 100, JS_Q = 100, JS_NEXT = 116;

__device__ __forceinline__ uint32_t sched_s0(uint32_t w) { return rotr32(w, 7) ^ rotr32(w, 18) ^ (w >> 3); }
__device__ __forceinline__ uint32_t sched_s1(uint32_t w) { return rotr32(w, 17) ^ rotr32(w, 19) ^ (w >> 10); }

// One lane per (proof, row) of the pre-LDE table, 115 stores, each of them consecutive words of one column across the wave.  The pipeline
// unrolled: Q_k(r) = W(r-k) + sigma0(W(r-k+1)) + [k >= 9] W(r-k+9) + [k >= 14] sigma1(W(r-k+14)), rows cyclic inside the proof, so the lane
// reads W of the sixteen rows r - 15 .. r (its neighbours' lines) and recomputes sigma0 / sigma1 instead of exchanging them; Q_15 needs
// W at r, r - 1, r - 6, r - 14 and r - 15 only.  W is the low 32 bits of the table word.
__global__ __launch_bounds__(256) void k_air_sched_helper(uint32_t log_rows, uint32_t n_proofs, const uint64_t* __restrict__ table,
                                                          uint64_t* __restrict__ helper) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((uint64_t)n_proofs << log_rows)) return;
  const uint32_t p = (uint32_t)(idx >> log_rows);
  const uint64_t mask = (1ull << log_rows) - 1, r = idx & mask;
  const uint64_t* __restrict__ t = table + (((uint64_t)p * AIR_SHA_WIDTH) << log_rows);  // (W is column 0)
  uint32_t w[16];  // w[d] = W(r - d)
#pragma unroll
  for (uint32_t d = 0; d < 16; d++) w[d] = (uint32_t)t[(r - d) & mask];
  const uint32_t w0 = w[0], x0 = rotr32(w0, 7) ^ rotr32(w0, 18), x1 = rotr32(w0, 17) ^ rotr32(w0, 19);
  uint64_t* __restrict__ o = helper + (((uint64_t)p * AIR_SCHED_HELPER_COLS) << log_rows) + r;
  auto put = [&](uint32_t col, uint64_t x) { o[(uint64_t)col << log_rows] = x; };
#pragma unroll 4
  for (uint32_t i = 0; i < 32; i++) {
    put(S_WB + i, (w0 >> i) & 1);
    put(S_X0 + i, (x0 >> i) & 1);
    put(S_X1 + i, (x1 >> i) & 1);
  }
  put(S_G0, sched_s0(w0));
  put(S_G1, sched_s1(w0));
  uint64_t q15 = 0;
#pragma unroll
  for (uint32_t k = 1; k <= 15; k++) {
    uint64_t q = (uint64_t)w[k] + sched_s0(w[k - 1]);
    if (k >= 9) q += w[k - 9];
    if (k >= 14) q += sched_s1(w[k - 14]);
    put(S_Q + k, q);
    q15 = q;
  }
  const uint32_t rnd = (uint32_t)(r & 63);
  const uint32_t cw = (rnd >= 15 && rnd <= 62) ? (uint32_t)(q15 >> 32) & 3 : 0;
  put(S_CW, cw & 1);
  put(S_CW + 1, cw >> 1);
}

// One thread per table entry: F by i mod 64 B (Horner on P_F's coefficients in LDS), 1 / (x^N - 1) by i mod B, gamma^0 .. 117.
__global__ __launch_bounds__(256) void k_air_sched_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n64, uint64_t w_n64,
                                                          uint64_t om64_inv, const uint64_t* __restrict__ gamma, uint64_t* __restrict__ tab) {
  __shared__ uint64_t pf[64];
  air_interpolate64(om64_inv, pf, ScheduleRow{});
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < (64u << log_blowup)) tab[AIR4_TAB_F + k] = air_horner64(pf, gl_mul(s_n64, gl_pow(w_n64, k)));
  air_zinv_gpow(k, log_blowup, first_proof, s_n, w_n, gamma, AIR_SCHED_CONSTRAINTS, tab + AIR4_TAB_ZINV, tab + AIR4_TAB_GPOW);
}

// The 117 constraints of one proof at one point; fx is F at the point.  The bit index b walks from 31 down to 0 and per b the pass holds
// WB_b, X0_b, X1_b and the six rotated or shifted bit words (WB_(b+7), WB_(b+18), WB_(b+17), WB_(b+19), and WB_(b+3) for b < 29, WB_(b+10)
// for b < 22), which are re-read through the cache.  Per b: three constraints (X^2 - X, X0, X1) and one Horner step by 2 of the three word
// sums (W, sigma0, sigma1), so that no power of two is multiplied: 5 reduced column products and 6 gamma weights.  Behind the loop the
// three word constraints, the two carry bits, the fifteen pipeline constraints (linear: W', G0', G1' and Q_1' .. Q_15' at the next row) and
// the selected one, whose F(x) is applied once to its value.
template <class F, class View>
__device__ __forceinline__ void air_sched_constraints(View& at, typename F::T fx) {
  using A = Forms<F>;
  using T = typename F::T;
  T ww = F::zero(), wg0 = F::zero(), wg1 = F::zero();
#pragma unroll View::BITS
  for (uint32_t b = 32; b-- > 0;) {
    const T WB = at.again(S_WB + b), X0 = at.once(S_X0 + b), X1 = at.once(S_X1 + b);
    const T W7 = at.again(S_WB + ((b + 7) & 31)), W18 = at.again(S_WB + ((b + 18) & 31));
    const T W17 = at.again(S_WB + ((b + 17) & 31)), W19 = at.again(S_WB + ((b + 19) & 31));
    at.plain(S_WB + b, A::boolean(WB));
    at.plain(JS_X0 + b, A::sub(X0, A::exor(W7, W18)));
    at.plain(JS_X1 + b, A::sub(X1, A::exor(W17, W19)));
    ww = A::dbl_add(ww, WB);
    wg0 = A::dbl_add(wg0, b < 29 ? A::exor(X0, at.again(S_WB + ((b + 3) & 31))) : X0);  // (b is uniform: a scalar branch)
    wg1 = A::dbl_add(wg1, b < 22 ? A::exor(X1, at.again(S_WB + ((b + 10) & 31))) : X1);
  }
  const T W = at.tbl(T_W), Wn = at.tbl_next(T_W);
  const T G0 = at.again(S_G0), G1 = at.again(S_G1), CW0 = at.once(S_CW), CW1 = at.once(S_CW + 1);
  at.plain(JS_WORD, A::sub(W, ww));
  at.plain(JS_G0, A::sub(G0, wg0));
  at.plain(JS_G1, A::sub(G1, wg1));
  at.plain(JS_CW, A::boolean(CW0));
  at.plain(JS_CW + 1, A::boolean(CW1));
  T prev = A::add(W, at.next(S_G0));  // what Q_k' must equal: W + G0' for k = 1, then Q_(k-1) (+ W' for k = 9, + G1' for k = 14)
#pragma unroll View::SHORT
  for (uint32_t k = 1; k <= 15; k++) {
    at.plain(JS_Q + k, A::sub(at.next(S_Q + k), prev));
    prev = at.again(S_Q + k);
    if (k + 1 == 9) prev = A::add(prev, Wn);
    if (k + 1 == 14) prev = A::add(prev, at.next(S_G1));
  }
  // (prev = Q_15)  F(x) (W' + 2^32 (CW_0 + 2 CW_1) - Q_15)
  const T carry = A::scale(A::add(CW0, A::add(CW1, CW1)), 1ull << 32);
  at.plain(JS_NEXT, A::mul(fx, A::sub(A::add(Wn, carry), prev)));
}

// The set-4 hot pass, k_air_sha_quotient's shape: one lane per point, a loop over the proofs from the last to the first (Horner by
// gamma^117), W and the 115 helper columns.  One gamma sum per proof, lazy as in set 3's pass; at the end 1 / (x^N - 1).  FORM as there.
template <int FORM>
__global__ __launch_bounds__(AIR_THREADS) void k_air_sched_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs,
                                                                    const uint64_t* __restrict__ cols, const uint64_t* __restrict__ hcols,
                                                                    const uint64_t* __restrict__ tab, uint64_t* __restrict__ out) {
  const uint64_t M = 1ull << log_m, i = (uint64_t)blockIdx.x * AIR_THREADS + threadIdx.x;
  if (i >= M) return;
  const uint64_t nx = (i + (1ull << log_blowup)) & (M - 1);
  const uint64_t* __restrict__ gp = tab + AIR4_TAB_GPOW;
  const uint64_t fx = tab[AIR4_TAB_F + (i & ((64ull << log_blowup) - 1))];
  const uint64_t zinv = tab[AIR4_TAB_ZINV + (i & ((1ull << log_blowup) - 1))];
  const gl2 g117 = {gp[2 * AIR_SCHED_CONSTRAINTS], gp[2 * AIR_SCHED_CONSTRAINTS + 1]};
  gl2 t = {0, 0};
  for (uint32_t p = n_proofs; p-- > 0;) {
    CosetView at = {cols + (((uint64_t)p * AIR_SHA_WIDTH) << log_m), hcols + (((uint64_t)p * AIR_SCHED_HELPER_COLS) << log_m), gp, log_m, i, nx};
    air_sched_constraints<FieldP>(at, fx);
    t = gl2_add(gl2_mul(t, g117), {gl_canon(at.a0), gl_canon(at.a1)});
  }
  gl2 q = gl2_scale(t, zinv);
  if (FORM != AIR_FORM_WHOLE) q = gl2_mul(q, {gp[2 * (AIR_SCHED_CONSTRAINTS + 1)], gp[2 * (AIR_SCHED_CONSTRAINTS + 1) + 1]});
  if (FORM == AIR_FORM_PIECE_ACC) q = gl2_add(q, {gl_canon(out[i]), gl_canon(out[M + i])});
  out[i] = q.c0;
  out[M + i] = q.c1;
}

// The set-4 identity at zeta, one workgroup: gamma^0 .. gamma^117 and P_F go to LDS first; thread t takes the proofs t, t + 256, ... and
// evaluates their 117 constraints over F_p^2 from the table's and the helper's openings; F(zeta) by Horner on P_F at zeta^(N/64).  A proof
// contributes gamma^(117 p) a; the sum is compared with (u_0 + X u_1) (zeta^N - 1).
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_sched_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub,
                                                                        uint64_t om64_inv, const uint64_t* __restrict__ open_t,
                                                                        const uint64_t* __restrict__ open_h, const uint64_t* __restrict__ open_q,
                                                                        const uint64_t* __restrict__ zeta, const uint64_t* __restrict__ gamma,
                                                                        uint32_t n_queries, uint32_t* __restrict__ ok) {
  __shared__ uint64_t gpw[2 * (AIR_SCHED_CONSTRAINTS + 1)];
  __shared__ uint64_t pf[64];
  const gl2 g = {gamma[0], gamma[1]};
  air_gamma_powers(g, AIR_SCHED_CONSTRAINTS, gpw);
  air_interpolate64(om64_inv, pf, ScheduleRow{});  // (ends with a barrier: gpw is complete behind it too)
  gl2 zp = {zeta[0], zeta[1]};  // zeta^(N/64)
  for (uint32_t k = 6; k < log_sub; k++) zp = gl2_mul(zp, zp);
  const gl2 F = air_horner64(pf, zp);
  gl2 sum = {0, 0};
  for (uint32_t p = threadIdx.x; p < n_proofs; p += AIR_CHECK_THREADS) {
    ZetaView at = {open_t + (uint64_t)p * AIR_SHA_WIDTH, open_h + (uint64_t)p * AIR_SCHED_HELPER_COLS, 1ull << log_r_t, 1ull << log_r_h, gpw};
    air_sched_constraints<FieldP2>(at, F);
    sum = gl2_add(sum, gl2_mul(gl2_pow(g, (uint64_t)AIR_SCHED_CONSTRAINTS * p), at.a));
  }
  gl2 zn = zp;  // zeta^N = (zeta^(N/64))^64
  for (uint32_t k = 0; k < 6; k++) zn = gl2_mul(zn, zn);
  air_check_verdict(sum, open_q, {gl_sub(zn.c0, 1), zn.c1}, n_queries, ok);
}

int launch_air_sched_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream) {
  const uint64_t n = (uint64_t)n_proofs << log_rows;
  hipLaunchKernelGGL(k_air_sched_helper, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S_(stream), log_rows, n_proofs,
                     reinterpret_cast<const uint64_t*>(d_table), reinterpret_cast<uint64_t*>(d_helper));
  return (int)hipGetLastError();
}
int launch_air_sched_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n64, uint64_t w_n64, uint64_t om64_inv, const void* d_gamma,
                            void* d_tab, void* stream) {
  hipLaunchKernelGGL(k_air_sched_tables, dim3(((64u << log_blowup) + 255) / 256), dim3(256), 0, S_(stream), log_blowup, first_proof, s_n, w_n, s_n64,
                     w_n64, om64_inv, reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<uint64_t*>(d_tab));
  return (int)hipGetLastError();
}
int launch_air_sched_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_helper_cols,
                              const void* d_tab, int form, void* d_quot, void* stream) {
  const dim3 grid((uint32_t)(((1ull << log_m) + AIR_THREADS - 1) / AIR_THREADS)), block(AIR_THREADS);
  const uint64_t* cols = reinterpret_cast<const uint64_t*>(d_cols);
  const uint64_t* hcols = reinterpret_cast<const uint64_t*>(d_helper_cols);
  const uint64_t* tab = reinterpret_cast<const uint64_t*>(d_tab);
  uint64_t* out = reinterpret_cast<uint64_t*>(d_quot);
  if (form == AIR_FORM_WHOLE)
    hipLaunchKernelGGL(k_air_sched_quotient<AIR_FORM_WHOLE>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, hcols, tab, out);
  else if (form == AIR_FORM_PIECE)
    hipLaunchKernelGGL(k_air_sched_quotient<AIR_FORM_PIECE>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, hcols, tab, out);
  else
    hipLaunchKernelGGL(k_air_sched_quotient<AIR_FORM_PIECE_ACC>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, hcols, tab, out);
  return (int)hipGetLastError();
}
int launch_air_sched_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint64_t om64_inv, const void* d_open_t,
                           const void* d_open_h, const void* d_open_q, const void* d_zeta, const void* d_gamma, uint32_t n_queries, void* d_ok,
                           void* stream) {
  hipLaunchKernelGGL(k_air_sched_check, dim3(1), dim3(AIR_CHECK_THREADS), 0, S_(stream), n_proofs, log_r_t, log_r_h, log_sub, om64_inv,
                     reinterpret_cast<const uint64_t*>(d_open_t), reinterpret_cast<const uint64_t*>(d_open_h),
                     reinterpret_cast<const uint64_t*>(d_open_q), reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<const uint64_t*>(d_gamma),
                     n_queries, reinterpret_cast<uint32_t*>(d_ok));
  return (int)hipGetLastError();
}

// ---- constraint set 5: the block starts of the SHA-256 tables (include/tmx.h "the block starts of the SHA-256 tables") ----------------------
// Row 0 of a block is round 0 applied to the words the block starts from, so six of those eight words stand in row 0 itself (b, c, d, f,
// g, h) and the round-bit machinery runs on them with the register names shifted by one.  Helper column offsets inside a proof's 315,
// constraint indices inside its 337.
constexpr uint32_t I_B = 0, I_C = 32, I_D = 64, I_F = 96, I_G = 128, I_H = 160, I_U0 = 192, I_U1 = 224, I_V = 256, I_S0 = 288, I_S1 = 289, I_CH = 290,
                   I_MAJ = 291, I_LV = 292, I_PZ = 293, I_CZ = 301, I_CA = 309, I_CE = 312;
constexpr uint32_t JI_CZ = 192, JI_CARRY = 200, JI_LV = 206, JI_WORD = 207, JI_U0 = 213, JI_U1 = 245, JI_V = 277, JI_S0 = 309, JI_S1 = 310, JI_CH = 311,
                   JI_MAJ = 312, JI_PZ = 313, JI_START = 321, JI_CHAIN = 329;
__device__ __constant__ const uint32_t IV_SHA256[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                                                       0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
constexpr uint64_t INIT_IV3 = 0xa54ff53aull, INIT_IV7 = 0x5be0cd19ull, INIT_K0 = 0x428a2f98ull;

__device__ __forceinline__ uint32_t init_big0(uint32_t b) { return rotr32(b, 2) ^ rotr32(b, 13) ^ rotr32(b, 22); }
__device__ __forceinline__ uint32_t init_big1(uint32_t f) { return rotr32(f, 6) ^ rotr32(f, 11) ^ rotr32(f, 25); }

// One lane per (proof, row) of the pre-LDE table: the nine words of the row, the first row of its block (LV) and of the next row's block
// (LV'; rows are cyclic inside the proof), on a boundary row also the nine words of the next row (the two round-0 sums), then 315 stores,
// each of them consecutive words of one column across the wave.  Operands are the low 32 bits of the words.
__global__ __launch_bounds__(256) void k_air_init_helper(uint32_t log_rows, uint32_t n_proofs, uint32_t chain, const uint64_t* __restrict__ table,
                                                         uint64_t* __restrict__ helper) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((uint64_t)n_proofs << log_rows)) return;
  const uint32_t p = (uint32_t)(idx >> log_rows);
  const uint64_t mask = (1ull << log_rows) - 1, r = idx & mask, rn = (r + 1) & mask;
  const uint64_t* __restrict__ t = table + (((uint64_t)p * AIR_SHA_WIDTH) << log_rows);
  uint32_t w[AIR_SHA_WIDTH];
  uint64_t any = 0, any_next = 0;
#pragma unroll
  for (uint32_t c = 0; c < AIR_SHA_WIDTH; c++) {
    w[c] = (uint32_t)t[((uint64_t)c << log_rows) + r];
    any |= t[((uint64_t)c << log_rows) + (r & ~63ull)];
    any_next |= t[((uint64_t)c << log_rows) + (rn & ~63ull)];
  }
  const uint32_t live = any ? 1u : 0u, live_next = any_next ? 1u : 0u;
  const uint32_t b = w[T_B], c = w[T_C], d = w[T_D], f = w[T_F], g = w[T_G], hh = w[T_H];
  const uint32_t u0 = rotr32(b, 2) ^ rotr32(b, 13), u1 = rotr32(f, 6) ^ rotr32(f, 11), v = b & c;
  uint64_t* __restrict__ o = helper + (((uint64_t)p * AIR_INIT_HELPER_COLS) << log_rows) + r;
  auto put = [&](uint32_t col, uint64_t x) { o[(uint64_t)col << log_rows] = x; };
#pragma unroll 4
  for (uint32_t i = 0; i < 32; i++) {
    put(I_B + i, (b >> i) & 1);
    put(I_C + i, (c >> i) & 1);
    put(I_D + i, (d >> i) & 1);
    put(I_F + i, (f >> i) & 1);
    put(I_G + i, (g >> i) & 1);
    put(I_H + i, (hh >> i) & 1);
    put(I_U0 + i, (u0 >> i) & 1);
    put(I_U1 + i, (u1 >> i) & 1);
    put(I_V + i, (v >> i) & 1);
  }
  put(I_S0, init_big0(b));
  put(I_S1, init_big1(f));
  put(I_CH, (f & g) ^ (~f & hh));
  put(I_MAJ, (b & c) ^ (b & d) ^ (c & d));
  put(I_LV, live);
  uint32_t pz[8];
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    const uint64_t s = (uint64_t)IV_SHA256[j] + w[1 + j];
    pz[j] = live_next ? (uint32_t)s : 0u;
    put(I_PZ + j, pz[j]);
    put(I_CZ + j, s >> 32);
  }
  uint32_t ca = 0, ce = 0;
  if ((r & 63) == 63) {  // a boundary row: round 0 of the next row's block, from the IV (a start row) or from PZ (a chain row)
    uint32_t n[AIR_SHA_WIDTH];
#pragma unroll
    for (uint32_t k = 0; k < AIR_SHA_WIDTH; k++) n[k] = (uint32_t)t[((uint64_t)k << log_rows) + rn];
    const bool chained = chain && (r & 127) == 63;
    const uint64_t t1 = (uint64_t)init_big1(n[T_F]) + ((n[T_F] & n[T_G]) ^ (~n[T_F] & n[T_H])) + n[T_W] + (live_next ? INIT_K0 : 0);
    const uint64_t t2 = (uint64_t)init_big0(n[T_B]) + ((n[T_B] & n[T_C]) ^ (n[T_B] & n[T_D]) ^ (n[T_C] & n[T_D]));
    const uint64_t h7 = chained ? pz[7] : live_next ? INIT_IV7 : 0, h3 = chained ? pz[3] : live_next ? INIT_IV3 : 0;
    ca = (uint32_t)((h7 + t1 + t2) >> 32) & 7;
    ce = (uint32_t)((h3 + h7 + t1) >> 32) & 7;
  }
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    put(I_CA + k, (ca >> k) & 1);
    put(I_CE + k, (ce >> k) & 1);
  }
}

// Eight nonzero values inverted with one field inversion (Montgomery's trick)
__device__ __forceinline__ void air_init_batch_inverse(uint64_t (&v)[8]) {
  uint64_t pre[8], acc = 1;
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    pre[j] = acc;
    acc = gl_mul(acc, v[j]);
  }
  uint64_t inv = gl_pow(acc, GL_P - 2);
#pragma unroll
  for (uint32_t j = 8; j-- > 0;) {
    const uint64_t x = gl_mul(inv, pre[j]);
    inv = gl_mul(inv, v[j]);
    v[j] = x;
  }
}

// One thread per eight selector entries, inverted as a batch: 1 / D_s(x_i) by i mod 64 B (chain = 0: D_s = x^(N/64) - omega_64^-1) or by
// i mod 128 B (chain = 1: D_s = x^(N/128) - rho, rho = omega_128^-1), from s_sel = s^(N/64) or s^(N/128) and w_sel likewise; and one thread
// per entry of 1 / (x^N - 1) by i mod B and per power gamma^0 .. gamma^337.  Under chain = 1 the same table holds 1 / D_c: x^(N/128)
// changes its sign 64 B points on, so D_c(x_i) = x_i^(N/128) + rho = -D_s(x_(i + 64 B)).  No entry vanishes: D_s divides x^N - 1, which
// the caller checked.
__global__ __launch_bounds__(256) void k_air_init_tables(uint32_t log_blowup, uint32_t chain, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_sel,
                                                         uint64_t w_sel, uint64_t rho, const uint64_t* __restrict__ gamma,
                                                         uint64_t* __restrict__ tab) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x, first = 8 * k;
  if (first < ((chain ? 128u : 64u) << log_blowup)) {  // (a multiple of 8)
    uint64_t v[8], x = gl_mul(s_sel, gl_pow(w_sel, first));
#pragma unroll
    for (uint32_t j = 0; j < 8; j++, x = gl_mul(x, w_sel)) v[j] = gl_sub(x, rho);
    air_init_batch_inverse(v);
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) tab[AIR5_TAB_SEL + first + j] = v[j];
  }
  air_zinv_gpow(k, log_blowup, first_proof, s_n, w_n, gamma, AIR_INIT_CONSTRAINTS, tab + AIR5_TAB_ZINV, tab + AIR5_TAB_GPOW);
}

// The 337 constraints of one proof at one point; chain is uniform.  Behind the bit loop the word constraints, LV, the eight PZ constraints
// with their CZ bits, the six carry bits, and the sixteen selected linear forms at the next row in two gamma sums of their own, so that
// the kernel applies D_s once to the start sum and D_c once to the chain sum (empty under chain = 0: E_c = 0).
template <class F, class View>
__device__ __forceinline__ void air_init_constraints(View& at, uint32_t chain) {
  using A = Forms<F>;
  using T = typename F::T;
  const RoundWords<F> w = air_round_bits<F>(at, {I_B, I_C, I_D, I_F, I_G, I_H, I_U0, I_U1, I_V, JI_U0, JI_U1, JI_V});
  at.plain(JI_WORD + 0, A::sub(at.tbl(T_B), w.a));
  at.plain(JI_WORD + 1, A::sub(at.tbl(T_C), w.b));
  at.plain(JI_WORD + 2, A::sub(at.tbl(T_D), w.c));
  at.plain(JI_WORD + 3, A::sub(at.tbl(T_F), w.e));
  at.plain(JI_WORD + 4, A::sub(at.tbl(T_G), w.f));
  at.plain(JI_WORD + 5, A::sub(at.tbl(T_H), w.g));
  at.plain(JI_S0, A::sub(at.again(I_S0), w.s0));
  at.plain(JI_S1, A::sub(at.again(I_S1), w.s1));
  at.plain(JI_CH, A::sub(at.again(I_CH), w.ch));
  at.plain(JI_MAJ, A::sub(at.again(I_MAJ), w.maj));
  at.plain(JI_LV, A::boolean(at.again(I_LV)));
  // the six carry bits, folded into the two words 2^32 CA and 2^32 CE at once
  T ca32 = F::zero(), ce32 = F::zero();
#pragma unroll View::SHORT
  for (uint32_t k = 3; k-- > 0;) {
    const T CA = at.once(I_CA + k), CE = at.once(I_CE + k);
    at.plain(JI_CARRY + k, A::boolean(CA));
    at.plain(JI_CARRY + 3 + k, A::boolean(CE));
    ca32 = A::dbl_add(ca32, CA);
    ce32 = A::dbl_add(ce32, CE);
  }
  ca32 = A::scale(ca32, 1ull << 32);
  ce32 = A::scale(ce32, 1ull << 32);
  // PZ_j - LV' (IV_j + s_j - 2^32 CZ_j), and with each of the six words that stand in row 0 its two selected linear forms: the next
  // row's word against IV_j LV' (start rows) and against PZ_j (chain rows; skipped under chain = 0, uniformly)
  const T LVn = at.next(I_LV);
  T pz3 = F::zero(), pz7 = F::zero();
#pragma unroll 1
  for (uint32_t j = 0; j < 8; j++) {
    const T CZ = at.once(I_CZ + j), PZ = at.once(I_PZ + j);
    at.plain(JI_CZ + j, A::boolean(CZ));
    at.plain(JI_PZ + j, A::sub(PZ, A::mul(LVn, A::sub(A::add_const(at.tbl(T_A + j), IV_SHA256[j]), A::scale(CZ, 1ull << 32)))));
    if (j == 3) pz3 = PZ;
    if (j == 7) pz7 = PZ;
    if (j != 3 && j != 7) {
      const uint32_t k = j < 3 ? j : j - 1;
      const T xn = at.tbl_next(T_B + j);
      at.started(JI_START + k, A::sub(xn, A::scale(LVn, IV_SHA256[j])));
      if (chain) at.chained(JI_CHAIN + k, A::sub(xn, PZ));
    }
  }
  // round 0 of the next row's block: a' and e' against the two sums
  const T t1 = A::add(A::add(at.next(I_S1), at.next(I_CH)), at.tbl_next(T_W)), t12 = A::add(t1, A::add(at.next(I_S0), at.next(I_MAJ)));
  const T an = A::add(at.tbl_next(T_A), ca32), en = A::add(at.tbl_next(T_E), ce32);
  at.started(JI_START + 6, A::sub(an, A::add(A::scale(LVn, INIT_IV7 + INIT_K0), t12)));
  at.started(JI_START + 7, A::sub(en, A::add(A::scale(LVn, INIT_IV3 + INIT_IV7 + INIT_K0), t1)));
  if (chain) {  // (uniform)
    const T kl = A::scale(LVn, INIT_K0);
    at.chained(JI_CHAIN + 6, A::sub(an, A::add(A::add(pz7, kl), t12)));
    at.chained(JI_CHAIN + 7, A::sub(en, A::add(A::add(pz3, pz7), A::add(kl, t1))));
  }
}

// The set-5 hot pass, k_air_sha_quotient's shape: one lane per point, a loop over the proofs from the last to the first (Horner by
// gamma^337), the nine table columns and the 315 helper columns.  Per proof 1 / D_s is applied once to the start sum, 1 / D_c once to the
// chain sum (skipped under chain = 0), 1 / (x^N - 1) once to the rest.  FORM as in k_air_sha_quotient.
template <int FORM>
__global__ __launch_bounds__(AIR_THREADS) void k_air_init_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, uint32_t chain,
                                                                   const uint64_t* __restrict__ cols, const uint64_t* __restrict__ hcols,
                                                                   const uint64_t* __restrict__ tab, uint64_t* __restrict__ out) {
  const uint64_t M = 1ull << log_m, i = (uint64_t)blockIdx.x * AIR_THREADS + threadIdx.x;
  if (i >= M) return;
  const uint64_t nx = (i + (1ull << log_blowup)) & (M - 1);
  const uint64_t* __restrict__ gp = tab + AIR5_TAB_GPOW;
  const uint64_t sel_mask = ((chain ? 128ull : 64ull) << log_blowup) - 1;
  const uint64_t dsinv = tab[AIR5_TAB_SEL + (i & sel_mask)];
  const uint64_t dcinv = chain ? gl_neg(tab[AIR5_TAB_SEL + ((i + (64ull << log_blowup)) & sel_mask)]) : 0;
  const uint64_t zinv = tab[AIR5_TAB_ZINV + (i & ((1ull << log_blowup) - 1))];
  const gl2 g337 = {gp[2 * AIR_INIT_CONSTRAINTS], gp[2 * AIR_INIT_CONSTRAINTS + 1]};
  gl2 t = {0, 0};
  for (uint32_t p = n_proofs; p-- > 0;) {
    CosetView at = {cols + (((uint64_t)p * AIR_SHA_WIDTH) << log_m), hcols + (((uint64_t)p * AIR_INIT_HELPER_COLS) << log_m), gp, log_m, i, nx};
    air_init_constraints<FieldP>(at, chain);
    uint64_t v0 = gl_add(gl_mul(gl_canon(at.a0), zinv), gl_mul(gl_canon(at.b0), dsinv));
    uint64_t v1 = gl_add(gl_mul(gl_canon(at.a1), zinv), gl_mul(gl_canon(at.b1), dsinv));
    if (chain) {  // (uniform)
      v0 = gl_add(v0, gl_mul(gl_canon(at.c0), dcinv));
      v1 = gl_add(v1, gl_mul(gl_canon(at.c1), dcinv));
    }
    t = gl2_add(gl2_mul(t, g337), {v0, v1});
  }
  if (FORM != AIR_FORM_WHOLE) t = gl2_mul(t, {gp[2 * (AIR_INIT_CONSTRAINTS + 1)], gp[2 * (AIR_INIT_CONSTRAINTS + 1) + 1]});
  if (FORM == AIR_FORM_PIECE_ACC) t = gl2_add(t, {gl_canon(out[i]), gl_canon(out[M + i])});
  out[i] = t.c0;
  out[M + i] = t.c1;
}

// The set-5 identity at zeta, one workgroup, division-free: gamma^0 .. gamma^337 go to LDS first; thread t takes the proofs t, t + 256, ...
// and evaluates their 337 constraints over F_p^2 from the table's and the helper's openings, in three sums.  With z = zeta^(N/128),
// D_s = z - rho, D_c = z + rho and S = D_s D_c under chain = 1 (z = zeta^(N/64), S = z - rho, D_c = 1 and no chain sum under chain = 0), a
// proof contributes gamma^(337 p) (S a + (zeta^N - 1) (D_c b + D_s c)); the sum is compared with (u_0 + X u_1) (zeta^N - 1) S.
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_init_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub,
                                                                       uint32_t chain, uint64_t rho, const uint64_t* __restrict__ open_t,
                                                                       const uint64_t* __restrict__ open_h, const uint64_t* __restrict__ open_q,
                                                                       const uint64_t* __restrict__ zeta, const uint64_t* __restrict__ gamma,
                                                                       uint32_t n_queries, uint32_t* __restrict__ ok) {
  __shared__ uint64_t gpw[2 * (AIR_INIT_CONSTRAINTS + 1)];
  const gl2 g = {gamma[0], gamma[1]};
  air_gamma_powers(g, AIR_INIT_CONSTRAINTS, gpw);
  __syncthreads();
  const uint32_t log_sel = chain ? 7 : 6;
  gl2 zp = {zeta[0], zeta[1]};  // zeta^(N/128) or zeta^(N/64)
  for (uint32_t k = log_sel; k < log_sub; k++) zp = gl2_mul(zp, zp);
  gl2 zn = zp;  // zeta^N
  for (uint32_t k = 0; k < log_sel; k++) zn = gl2_mul(zn, zn);
  const gl2 zn1 = {gl_sub(zn.c0, 1), zn.c1};
  const gl2 Ds = {gl_sub(zp.c0, rho), zp.c1}, Dc = chain ? gl2{gl_add(zp.c0, rho), zp.c1} : gl2{1, 0};
  const gl2 S = chain ? gl2_mul(Ds, Dc) : Ds;
  gl2 sum = {0, 0};
  for (uint32_t p = threadIdx.x; p < n_proofs; p += AIR_CHECK_THREADS) {
    ZetaView at = {open_t + (uint64_t)p * AIR_SHA_WIDTH, open_h + (uint64_t)p * AIR_INIT_HELPER_COLS, 1ull << log_r_t, 1ull << log_r_h, gpw};
    air_init_constraints<FieldP2>(at, chain);
    const gl2 v = gl2_add(gl2_mul(S, at.a), gl2_mul(zn1, gl2_add(gl2_mul(Dc, at.b), gl2_mul(Ds, at.c))));
    sum = gl2_add(sum, gl2_mul(gl2_pow(g, (uint64_t)AIR_INIT_CONSTRAINTS * p), v));
  }
  air_check_verdict(sum, open_q, gl2_mul(zn1, S), n_queries, ok);
}

int launch_air_init_helper(uint32_t log_rows, uint32_t n_proofs, uint32_t chain, const void* d_table, void* d_helper, void* stream) {
  const uint64_t n = (uint64_t)n_proofs << log_rows;
  hipLaunchKernelGGL(k_air_init_helper, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S_(stream), log_rows, n_proofs, chain,
                     reinterpret_cast<const uint64_t*>(d_table), reinterpret_cast<uint64_t*>(d_helper));
  return (int)hipGetLastError();
}
int launch_air_init_tables(uint32_t log_blowup, uint32_t chain, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_sel, uint64_t w_sel, uint64_t rho,
                           const void* d_gamma, void* d_tab, void* stream) {
  // (at least two workgroups: the 339 gamma powers)
  const uint32_t blocks = ((((chain ? 128u : 64u) << log_blowup) / 8) + 255) / 256;
  hipLaunchKernelGGL(k_air_init_tables, dim3(blocks < 2 ? 2 : blocks), dim3(256), 0, S_(stream), log_blowup, chain, first_proof, s_n, w_n, s_sel, w_sel,
                     rho,
                     reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<uint64_t*>(d_tab));
  return (int)hipGetLastError();
}
int launch_air_init_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, uint32_t chain, const void* d_cols, const void* d_helper_cols,
                             const void* d_tab, int form, void* d_quot, void* stream) {
  const dim3 grid((uint32_t)(((1ull << log_m) + AIR_THREADS - 1) / AIR_THREADS)), block(AIR_THREADS);
  const uint64_t* cols = reinterpret_cast<const uint64_t*>(d_cols);
  const uint64_t* hcols = reinterpret_cast<const uint64_t*>(d_helper_cols);
  const uint64_t* tab = reinterpret_cast<const uint64_t*>(d_tab);
  uint64_t* out = reinterpret_cast<uint64_t*>(d_quot);
  if (form == AIR_FORM_WHOLE)
    hipLaunchKernelGGL(k_air_init_quotient<AIR_FORM_WHOLE>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, chain, cols, hcols, tab, out);
  else if (form == AIR_FORM_PIECE)
    hipLaunchKernelGGL(k_air_init_quotient<AIR_FORM_PIECE>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, chain, cols, hcols, tab, out);
  else
    hipLaunchKernelGGL(k_air_init_quotient<AIR_FORM_PIECE_ACC>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, chain, cols, hcols, tab, out);
  return (int)hipGetLastError();
}
int launch_air_init_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint32_t chain, uint64_t rho,
                          const void* d_open_t, const void* d_open_h, const void* d_open_q, const void* d_zeta, const void* d_gamma,
                          uint32_t n_queries, void* d_ok, void* stream) {
  hipLaunchKernelGGL(k_air_init_check, dim3(1), dim3(AIR_CHECK_THREADS), 0, S_(stream), n_proofs, log_r_t, log_r_h, log_sub, chain, rho,
                     reinterpret_cast<const uint64_t*>(d_open_t), reinterpret_cast<const uint64_t*>(d_open_h),
                     reinterpret_cast<const uint64_t*>(d_open_q), reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<const uint64_t*>(d_gamma),
                     n_queries, reinterpret_cast<uint32_t*>(d_ok));
  return (int)hipGetLastError();
}

// ---- constraint set 6: the SHA-256 tables' link to Level-1 (include/tmx.h "the SHA-256 tables' link to Level-1") -----------------------------
// The public table and the helper oracle; sets 3 - 5 above stay as they are.

// One byte of an element row: eight big-endian bit elements
__device__ __forceinline__ uint32_t link_byte(const uint64_t* __restrict__ at) {
  uint32_t v = 0;
#pragma unroll
  for (uint32_t b = 0; b < 8; b++) v = (v << 1) | ((uint32_t)at[b] & 1u);
  return v;
}

// One hash of a table as the element row holds it: a message of `len` bytes (0: a zero hash, no block is live) -- the byte `prefix` at
// position 0 where a_lo = 1, then the bytes at element a_at on positions [a_lo, a_hi) and those at b_at on [b_lo, b_hi), zero elsewhere --
// and the 32 digest bytes at element dig_at.
struct LinkHash {
  uint32_t len, prefix, a_at, a_lo, a_hi, b_at, b_lo, b_hi, dig_at;
};

// Which hash stands at item `it` of the section's table, in the order k_trace_sha256 / k_trace_sha256x2 (trace.hip) write them.
__device__ __forceinline__ LinkHash link_hash(const AirShaPublicGeom& G, const uint64_t* __restrict__ row, uint32_t it) {
  LinkHash H = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t n = G.n, sets = G.kind == 0 ? 2u : 1u;
  if (G.section == 4u) {  // T.3: 00 | marshalled[0 .. validator_byte_length), item (set, lane)
    if (it >= sets * n) return H;
    const uint32_t set = it >= n ? 1u : 0u, i = it - set * n;
    const uint32_t lane = set ? G.d2a + G.d2a_lane * i : G.d1a + G.d1a_lane * i;
    const uint32_t vlen = (uint32_t)row[set ? G.h4 + G.h4_lane * i + G.h4_vlen : G.h2 + G.h2_lane * i + G.h2_vlen];
    H.len = 1u + (vlen > 46u ? 46u : vlen);
    H.a_at = lane; H.a_lo = 1; H.a_hi = 47;
    H.dig_at = lane + G.lane_leaf;
    return H;
  }
  if (G.section == 16u) {  // T.5: 01 | L | R over the slot's two children, item (set, slot); a promoted slot is a zero hash
    if (it >= sets * G.tn) return H;
    const uint32_t set = it >= G.tn ? 1u : 0u, nodes = set ? G.d4 : G.d3;
    uint32_t rem = it - set * G.tn, sz = n, level = 0, first = 0, prev_first = 0;
    for (;;) {
      const uint32_t nx = (sz + 1u) / 2u;
      if (rem < nx) break;
      rem -= nx; prev_first = first; first += nx; sz = nx; level++;
    }
    if (2u * rem + 1u >= sz) return H;
    const uint32_t step = level ? 256u : (set ? G.d2a_lane : G.d1a_lane);
    const uint32_t l = level ? nodes + 256u * (prev_first + 2u * rem) : (set ? G.d2a : G.d1a) + step * 2u * rem + G.lane_leaf;
    H.len = 65; H.prefix = 1;
    H.a_at = l; H.a_lo = 1; H.a_hi = 33;
    H.b_at = l + step; H.b_lo = 33; H.b_hi = 65;
    H.dig_at = nodes + 256u * (first + rem);
    return H;
  }
  // T.6: item (proof q, hash h): h = 0 the leaf 00 | leaf as the proof struct carries it, h = 1 .. 4 the path nodes 01 | left | right
  const uint32_t nq = G.kind == 0 ? 4u : 5u, q = it / 5u, h = it - 5u * q;
  if (q >= nq) return H;
  const uint32_t step_kind = G.kind == 0 ? 0u : 1u;
  const uint32_t d5q = G.d5 + G.d5_proof[q], aunts = G.h3 + G.aunts[q];
  H.dig_at = d5q + 256u * h;
  if (h == 0) {
    if (q == 0) {  // the chain id: 52 bytes carried, the encoded length decides
      const uint32_t cl = (uint32_t)row[G.h3 + G.cid_len];
      H.len = (cl > 79u ? 79u : cl) + 1u;
      H.a_at = G.h3 + G.cid; H.a_lo = 1; H.a_hi = 53;
    } else if (q == 1) {  // the height leaf 00 08 varint9 of D.5
      const uint32_t hl = (uint32_t)row[G.h3 + G.h_len];
      H.len = (hl > 79u ? 79u : hl) + 1u;
      H.a_at = G.d5 + G.d5_hleaf; H.a_lo = 0; H.a_hi = 11;
    } else {
      const uint32_t w = G.leaf_bytes[q];
      H.len = w + 1u;
      H.a_at = G.h3 + G.leaf[q]; H.a_lo = 1; H.a_hi = 1u + w;
    }
    return H;
  }
  const uint32_t k = h - 1u, index = q == 0 ? 1u : (q == 1 ? 2u : (q == 2 ? 7u : (q == 3 ? (step_kind ? 4u : 7u) : 8u)));
  const uint32_t cur = d5q + 256u * k, aunt = aunts + 256u * k;
  const bool right = (index >> k) & 1u;  // the running hash is the right child
  H.len = 65; H.prefix = 1;
  H.a_at = right ? aunt : cur; H.a_lo = 1; H.a_hi = 33;
  H.b_at = right ? cur : aunt; H.b_lo = 33; H.b_hi = 65;
  return H;
}

// Byte `pos` of the padded message: the message, 80, zeros, the bit length in the last four bytes of the last block
__device__ __forceinline__ uint32_t link_padded_byte(const LinkHash& H, const uint64_t* __restrict__ row, uint32_t n_blocks, uint32_t pos) {
  if (pos >= H.len) {
    if (pos == H.len) return 0x80u;
    const uint32_t tail = 64u * n_blocks - 1u - pos;
    return tail < 4u ? ((8u * H.len) >> (8u * tail)) & 0xffu : 0u;
  }
  if (pos < H.a_lo) return H.prefix;
  if (pos < H.a_hi) return link_byte(row + H.a_at + 8u * (pos - H.a_lo));
  if (pos >= H.b_lo && pos < H.b_hi) return link_byte(row + H.b_at + 8u * (pos - H.b_lo));
  return 0u;
}

// One lane per (proof, block): the sixteen message words of the block, the digest where the block is the last live one of its hash, new
// and chn, from the element row of the proof alone.  Blocks of a zero hash, unused second blocks and the padding behind the section's own
// blocks are all zero.  Lanes run over the blocks, so each of the 26 stores of a wave covers consecutive words of one column.
__global__ __launch_bounds__(256) void k_air_sha_public_gather(const uint64_t* __restrict__ rows, AirShaPublicGeom G, uint32_t log_k, uint32_t n_proofs,
                                                               uint64_t* __restrict__ pub) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((uint64_t)n_proofs << log_k)) return;
  const uint32_t p = (uint32_t)(idx >> log_k), k = (uint32_t)(idx & ((1u << log_k) - 1));
  const uint64_t* __restrict__ row = rows + (uint64_t)p * G.elem_stride;
  const uint32_t log_per = G.section == 4u ? 0u : 1u, b = k & ((1u << log_per) - 1u);
  const LinkHash H = link_hash(G, row, k >> log_per);
  const uint32_t n_blocks = H.len == 0 ? 0u : (H.len + 9u > 64u ? 2u : 1u);
  const bool live = b < n_blocks, last = live && b + 1u == n_blocks;
  uint64_t* __restrict__ dst = pub + (((uint64_t)p * AIR_SHA_PUBLIC_WIDTH) << log_k) + k;
#pragma unroll 1
  for (uint32_t t = 0; t < 16; t++) {
    uint32_t word = 0;
    if (live) {
#pragma unroll 1
      for (uint32_t c = 0; c < 4; c++) word = (word << 8) | link_padded_byte(H, row, n_blocks, 64u * b + 4u * t + c);
    }
    dst[(uint64_t)t << log_k] = word;
  }
#pragma unroll 1
  for (uint32_t j = 0; j < 8; j++) {
    uint32_t word = 0;
    if (last) {
#pragma unroll
      for (uint32_t c = 0; c < 4; c++) word = (word << 8) | link_byte(row + H.dig_at + 8u * (4u * j + c));
    }
    dst[(uint64_t)(16 + j) << log_k] = word;
  }
  dst[(uint64_t)24 << log_k] = live && b == 0 ? 1 : 0;
  dst[(uint64_t)25 << log_k] = live && b != 0 ? 1 : 0;
}

// One lane per (proof, row) of the pre-LDE table: the row's eight state words, the flags of its block and chn of the next block (blocks
// cyclic inside the proof), under chn the eight state words of the row in front of the block; then 33 stores, each of them consecutive
// words of one column across the wave.  Operands are the low 32 bits of the words; a flag is set when its low 32 bits are not zero.
__global__ __launch_bounds__(256) void k_air_link_helper(uint32_t log_rows, uint32_t n_proofs, const uint64_t* __restrict__ table,
                                                         const uint64_t* __restrict__ pub, uint64_t* __restrict__ helper) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((uint64_t)n_proofs << log_rows)) return;
  const uint32_t p = (uint32_t)(idx >> log_rows), log_k = log_rows - 6;
  const uint64_t mask = (1ull << log_rows) - 1, r = idx & mask, prev = ((r & ~63ull) - 1) & mask;
  const uint32_t k = (uint32_t)(r >> 6), kn = (k + 1u) & ((1u << log_k) - 1u);
  const uint64_t* __restrict__ t = table + (((uint64_t)p * AIR_SHA_WIDTH) << log_rows);
  const uint64_t* __restrict__ u = pub + (((uint64_t)p * AIR_SHA_PUBLIC_WIDTH) << log_k);
  const bool is_new = (uint32_t)u[((uint64_t)24 << log_k) + k] != 0, is_chn = !is_new && (uint32_t)u[((uint64_t)25 << log_k) + k] != 0;
  const uint64_t chn_next = (uint32_t)u[((uint64_t)25 << log_k) + kn] != 0 ? 1 : 0;
  uint64_t* __restrict__ o = helper + (((uint64_t)p * AIR_LINK_HELPER_COLS) << log_rows) + r;
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    const uint64_t* __restrict__ col = t + ((uint64_t)(1 + j) << log_rows);
    const uint32_t cv = is_new ? IV_SHA256[j] : is_chn ? IV_SHA256[j] + (uint32_t)col[prev] : 0u;
    const uint64_t s = (uint64_t)cv + (uint32_t)col[r];
    o[(uint64_t)j << log_rows] = cv;
    o[(uint64_t)(8 + j) << log_rows] = (uint32_t)s;
    o[(uint64_t)(16 + j) << log_rows] = s >> 32;
    o[(uint64_t)(24 + j) << log_rows] = chn_next ? (uint32_t)s : 0u;
  }
  o[(uint64_t)32 << log_rows] = chn_next;
}

// Helper column offsets inside a proof's 33; the constraint indices inside its 50 are written where they are used.
constexpr uint32_t K_CV = 0, K_DG = 8, K_CD = 16, K_CH = 24, K_CHN = 32;

// The 50 constraints of one proof at one point, once for prover and verifier: 0 .. 31 into the plain sum (24 .. 31 carry the factor S),
// the column parts of 32 .. 48 into the selected sum (what T = (x^N - 1) / S multiplies, less the public polynomials), W into the third
// sum (what sum_t T_t multiplies, less E_t).  Constraint 49 has one weight for its sixteen parts: the T_t vanish on disjoint classes of
// rows, so the sum is zero on the domain exactly when each part is.
template <class F, class View>
__device__ __forceinline__ void air_link_constraints(View& at, typename F::T S) {
  using A = Forms<F>;
  using T = typename F::T;
  const T CHN = at.again(K_CHN);
#pragma unroll View::BITS
  for (uint32_t j = 0; j < 8; j++) {
    const T CV = at.once(K_CV + j), DG = at.once(K_DG + j), CD = at.once(K_CD + j), CH = at.once(K_CH + j), CVn = at.next(K_CV + j);
    at.plain(j, A::boolean(CD));
    at.plain(8 + j, A::sub(A::add(DG, A::scale(CD, 1ull << 32)), A::add(CV, at.tbl(T_A + j))));
    at.plain(16 + j, A::sub(CH, A::mul(CHN, DG)));
    at.plain(24 + j, A::mul(S, A::sub(CVn, CV)));
    at.selected(32 + j, A::sub(CVn, CH));
    at.selected(40 + j, A::sub(DG, CH));
  }
  at.selected(48, CHN);
  at.chained(49, at.tbl(T_W));
}

// One thread per entry i < 64 B of the selector tables: z = x_i^K, the seventeen denominators z - omega_64^-1 and z - omega_64^t inverted
// with one Fermat chain (Montgomery's trick), and their sum over t; and air_zinv_gpow's share.  No entry vanishes: S and every D_t
// divide x^N - 1, which the caller checked.
__global__ __launch_bounds__(256) void k_air_link_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_k, uint64_t w_k,
                                                         uint64_t om64, const uint64_t* __restrict__ gamma, uint64_t* __restrict__ tab) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < (64u << log_blowup)) {
    const uint64_t z = gl_mul(s_k, gl_pow(w_k, k));
    uint64_t d[17], pre[17], acc = 1, o = 1;
#pragma unroll
    for (uint32_t t = 0; t < 16; t++, o = gl_mul(o, om64)) d[1 + t] = gl_sub(z, o);
    d[0] = gl_sub(z, gl_pow(om64, 63));
#pragma unroll
    for (uint32_t t = 0; t < 17; t++) {
      pre[t] = acc;
      acc = gl_mul(acc, d[t]);
    }
    uint64_t inv = gl_pow(acc, GL_P - 2), dsum = 0;
#pragma unroll
    for (uint32_t t = 17; t-- > 0;) {
      const uint64_t x = gl_mul(inv, pre[t]);
      inv = gl_mul(inv, d[t]);
      if (t) {
        tab[AIR6_TAB_DINV + (t - 1) * AIR6_PER_MAX + k] = x;
        dsum = gl_add(dsum, x);
      } else {
        tab[AIR6_TAB_SINV + k] = x;
      }
    }
    tab[AIR6_TAB_S + k] = d[0];
    tab[AIR6_TAB_DSUM + k] = dsum;
  }
  air_zinv_gpow(k, log_blowup, first_proof, s_n, w_n, gamma, AIR_LINK_CONSTRAINTS, tab + AIR6_TAB_ZINV, tab + AIR6_TAB_GPOW);
}

// The seventeen value vectors, one lane per (vector, block k) -- blockIdx.y is the vector: 0 for V63, 1 + t for V^t --, Horner over the
// proofs by gamma^50:
//   V63_k = sum_p gamma^(50 p) [G_new new_p[k + 1] + sum_j gamma^(40 + j) dig_p[k][j] + gamma^48 chn_p[k + 1]],  G_new = sum_j gamma^(32 + j) IV_j
//   V^t_k = gamma^49 sum_p gamma^(50 p) w_p[k][t]
// (k + 1 mod K).  pub is column-major: a wave reads 64 consecutive words per column; the gamma powers sit in LDS, wave-uniform.
__global__ __launch_bounds__(256) void k_air_link_combine(uint32_t log_k, uint32_t n_proofs, const uint64_t* __restrict__ pub,
                                                          const uint64_t* __restrict__ gamma, uint64_t* __restrict__ v) {
  __shared__ uint64_t gw[2 * 12];  // gamma^40 .. gamma^50, then G_new
  if (threadIdx.x < 11) {
    const gl2 g = gl2_pow({gamma[0], gamma[1]}, 40 + threadIdx.x);
    gw[2 * threadIdx.x] = g.c0;
    gw[2 * threadIdx.x + 1] = g.c1;
  } else if (threadIdx.x == 11) {
    gl2 g = gl2_pow({gamma[0], gamma[1]}, 32), s = {0, 0};
    for (uint32_t j = 0; j < 8; j++, g = gl2_mul(g, {gamma[0], gamma[1]})) s = gl2_add(s, gl2_scale(g, IV_SHA256[j]));
    gw[22] = s.c0;
    gw[23] = s.c1;
  }
  __syncthreads();
  const uint32_t K = 1u << log_k, k = blockIdx.x * 256 + threadIdx.x, which = blockIdx.y;
  if (k >= K) return;
  const uint32_t kn = (k + 1) & (K - 1);
  const gl2 g50 = {gw[20], gw[21]};
  gl2 t = {0, 0};
  if (which == 0) {
    const gl2 g48 = {gw[16], gw[17]}, g_new = {gw[22], gw[23]};
    for (uint32_t p = n_proofs; p-- > 0;) {
      const uint64_t* __restrict__ c = pub + (((uint64_t)p * AIR_SHA_PUBLIC_WIDTH) << log_k);
      gl2 w = gl2_add(gl2_scale(g_new, gl_canon(c[((uint64_t)24 << log_k) + kn])), gl2_scale(g48, gl_canon(c[((uint64_t)25 << log_k) + kn])));
#pragma unroll
      for (uint32_t j = 0; j < 8; j++) w = gl2_add(w, gl2_scale({gw[2 * j], gw[2 * j + 1]}, gl_canon(c[((uint64_t)(16 + j) << log_k) + k])));
      t = gl2_add(gl2_mul(t, g50), w);
    }
  } else {
    for (uint32_t p = n_proofs; p-- > 0;) {
      const uint64_t x = gl_canon(pub[(((uint64_t)p * AIR_SHA_PUBLIC_WIDTH + (which - 1)) << log_k) + k]);
      t = gl2_mul(t, g50);
      t.c0 = gl_add(t.c0, x);
    }
    t = gl2_mul(t, {gw[18], gw[19]});
  }
  v[((uint64_t)which << (log_k + 1)) + 2 * k] = t.c0;
  v[((uint64_t)which << (log_k + 1)) + 2 * k + 1] = t.c1;
}

// The fold of one extended public polynomial into PQ, one lane per point: pq = (first ? 0 : pq) + ext / divisor, both planes
__global__ __launch_bounds__(256) void k_air_link_fold(uint32_t log_m, uint32_t log_blowup, uint32_t which, uint32_t first, const uint64_t* __restrict__ ext,
                                                       const uint64_t* __restrict__ tab, uint64_t* __restrict__ pq) {
  const uint64_t M = 1ull << log_m, i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const uint64_t per = i & ((64ull << log_blowup) - 1);
  const uint64_t inv = which ? tab[AIR6_TAB_DINV + (uint64_t)(which - 1) * AIR6_PER_MAX + per] : tab[AIR6_TAB_SINV + per];
  uint64_t q0 = gl_mul(gl_canon(ext[i]), inv), q1 = gl_mul(gl_canon(ext[M + i]), inv);
  if (!first) {
    q0 = gl_add(q0, pq[i]);
    q1 = gl_add(q1, pq[M + i]);
  }
  pq[i] = q0;
  pq[M + i] = q1;
}

// The set-6 hot pass, k_air_ladder_boundary_quotient's shape: one lane per point, a loop over the proofs from the last to the first
// (Horner by gamma^50), the nine table columns and the 33 helper columns at i and the eight CV at i + B.  Per proof 1 / (x^N - 1) is applied
// once to the plain sum, 1 / S once to the selected sum and sum_t 1 / D_t once to gamma^49 W.  pq: the folded public side, subtracted by
// the piece that starts at proof 0 (null elsewhere).  FORM as in k_air_sha_quotient.
template <int FORM>
__global__ __launch_bounds__(AIR_THREADS) void k_air_link_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs,
                                                                   const uint64_t* __restrict__ cols, const uint64_t* __restrict__ hcols,
                                                                   const uint64_t* __restrict__ tab, const uint64_t* __restrict__ pq,
                                                                   uint64_t* __restrict__ out) {
  const uint64_t M = 1ull << log_m, i = (uint64_t)blockIdx.x * AIR_THREADS + threadIdx.x;
  if (i >= M) return;
  const uint64_t nx = (i + (1ull << log_blowup)) & (M - 1), per = i & ((64ull << log_blowup) - 1);
  const uint64_t* __restrict__ gp = tab + AIR6_TAB_GPOW;
  const uint64_t S = tab[AIR6_TAB_S + per], sinv = tab[AIR6_TAB_SINV + per], dsum = tab[AIR6_TAB_DSUM + per];
  const uint64_t zinv = tab[AIR6_TAB_ZINV + (i & ((1ull << log_blowup) - 1))];
  const gl2 g50 = {gp[2 * AIR_LINK_CONSTRAINTS], gp[2 * AIR_LINK_CONSTRAINTS + 1]};
  gl2 t = {0, 0};
  for (uint32_t p = n_proofs; p-- > 0;) {
    CosetView at = {cols + (((uint64_t)p * AIR_SHA_WIDTH) << log_m), hcols + (((uint64_t)p * AIR_LINK_HELPER_COLS) << log_m), gp, log_m, i, nx};
    air_link_constraints<FieldP>(at, S);
    const uint64_t v0 = gl_add(gl_add(gl_mul(gl_canon(at.a0), zinv), gl_mul(gl_canon(at.b0), sinv)), gl_mul(gl_canon(at.c0), dsum));
    const uint64_t v1 = gl_add(gl_add(gl_mul(gl_canon(at.a1), zinv), gl_mul(gl_canon(at.b1), sinv)), gl_mul(gl_canon(at.c1), dsum));
    t = gl2_add(gl2_mul(t, g50), {v0, v1});
  }
  if (FORM != AIR_FORM_WHOLE) t = gl2_mul(t, {gp[2 * (AIR_LINK_CONSTRAINTS + 1)], gp[2 * (AIR_LINK_CONSTRAINTS + 1) + 1]});
  if (pq) t = gl2_sub(t, {gl_canon(pq[i]), gl_canon(pq[M + i])});
  if (FORM == AIR_FORM_PIECE_ACC) t = gl2_add(t, {gl_canon(out[i]), gl_canon(out[M + i])});
  out[i] = t.c0;
  out[M + i] = t.c1;
}

// The set-6 identity at zeta, one workgroup:
//   sum_p gamma^(50 p) (a + Z (b / S + c sum_t 1 / D_t)) - Z PQ(zeta) == (u_0 + X u_1) Z,   Z = zeta^N - 1
// a, b, c the three sums of air_link_constraints over F_p^2 from the openings; thread t takes the proofs t, t + 256, ...  PQ(zeta) is the sum
// over the seventeen cosets y_k = omega^off omega_K^k (off = 63, then 0 .. 15) of 1 / (K y_0^K) sum_k V_k y_k / (zeta - y_k), barycentric from
// the verifier's own V as in k_air_ladder_boundary_check: thread t takes k = t, t + 256, ... (at most 16) of every coset and inverts its
// zeta - y_k with one F_p^2 inversion per coset.  Every term is linear in the sums, so each thread folds its own share and one sum meets in
// LDS.  A zero denominator (S, a D_t or a zeta - y_k: zeta lies outside F_p, so only a zeta^K inside it can do that) clears every verdict.
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_link_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint64_t om64,
                                                                       uint64_t om, uint64_t om_k, uint64_t k_inv,
                                                                       const uint64_t* __restrict__ open_t, const uint64_t* __restrict__ open_h,
                                                                       const uint64_t* __restrict__ open_q, const uint64_t* __restrict__ zeta,
                                                                       const uint64_t* __restrict__ gamma, const uint64_t* __restrict__ vk,
                                                                       uint32_t n_queries, uint32_t* __restrict__ ok) {
  __shared__ uint64_t gpw[2 * (AIR_LINK_CONSTRAINTS + 1)];
  const uint32_t t = threadIdx.x, log_k = log_sub - 6, K = 1u << log_k;
  const gl2 g = {gamma[0], gamma[1]}, z = {zeta[0], zeta[1]};
  air_gamma_powers(g, AIR_LINK_CONSTRAINTS, gpw);
  __syncthreads();
  gl2 zk = z;  // zeta^K
  for (uint32_t k = 0; k < log_k; k++) zk = gl2_mul(zk, zk);
  gl2 zn = zk;  // zeta^N
  for (uint32_t k = 0; k < 6; k++) zn = gl2_mul(zn, zn);
  const gl2 Z = {gl_sub(zn.c0, 1), zn.c1};
  const gl2 S = {gl_sub(zk.c0, gl_pow(om64, 63)), zk.c1};
  bool bad = gl2_eq(S, {0, 0});
  gl2 dsum = {0, 0};
  {
    uint64_t o = 1;
    for (uint32_t k = 0; k < 16; k++, o = gl_mul(o, om64)) {
      const gl2 d = {gl_sub(zk.c0, o), zk.c1};
      bad = bad || gl2_eq(d, {0, 0});
      dsum = gl2_add(dsum, gl2_inv(d));
    }
  }
  const gl2 sinv = gl2_inv(S);
  gl2 sum = {0, 0};
  for (uint32_t p = t; p < n_proofs; p += AIR_CHECK_THREADS) {
    ZetaView at = {open_t + (uint64_t)p * AIR_SHA_WIDTH, open_h + (uint64_t)p * AIR_LINK_HELPER_COLS, 1ull << log_r_t, 1ull << log_r_h, gpw};
    air_link_constraints<FieldP2>(at, S);
    const gl2 v = gl2_add(at.a, gl2_mul(Z, gl2_add(gl2_mul(at.b, sinv), gl2_mul(at.c, dsum))));
    sum = gl2_add(sum, gl2_mul(gl2_pow(g, (uint64_t)AIR_LINK_CONSTRAINTS * p), v));
  }
  gl2 pqz = {0, 0};
  const uint64_t stride = gl_pow(om_k, AIR_CHECK_THREADS);
#pragma unroll 1
  for (uint32_t c = 0; c < 17; c++) {
    const uint32_t off = c ? c - 1 : 63;
    const uint64_t* __restrict__ v = vk + ((uint64_t)c << (log_k + 1));
    gl2 pre[AIR_BARY_PER];
    uint64_t yk[AIR_BARY_PER];
    gl2 run = {1, 0}, psum = {0, 0};
    uint64_t y = gl_mul(gl_pow(om, off), gl_pow(om_k, t));
#pragma unroll
    for (int m = 0; m < AIR_BARY_PER; m++) {
      const bool in = t + m * AIR_CHECK_THREADS < K;
      yk[m] = y;
      pre[m] = run;
      if (in) {
        const gl2 d = {gl_sub(z.c0, y), z.c1};
        bad = bad || gl2_eq(d, {0, 0});
        run = gl2_mul(run, d);
      }
      y = gl_mul(y, stride);
    }
    gl2 inv = gl2_inv(run);
#pragma unroll
    for (int m = AIR_BARY_PER - 1; m >= 0; m--) {
      const uint32_t k = t + m * AIR_CHECK_THREADS;
      if (k < K) {
        const gl2 di = gl2_mul(inv, pre[m]);  // 1 / (zeta - y_k)
        inv = gl2_mul(inv, {gl_sub(z.c0, yk[m]), z.c1});
        const gl2 V = {gl_canon(v[2 * k]), gl_canon(v[2 * k + 1])};
        psum = gl2_add(psum, gl2_mul(gl2_scale(V, yk[m]), di));
      }
    }
    // 1 / (K y_0^K), y_0^K = omega_64^off
    pqz = gl2_add(pqz, gl2_scale(psum, gl_mul(k_inv, gl_pow(om64, 64 - off))));
  }
  sum = gl2_sub(sum, gl2_mul(Z, pqz));
  __shared__ uint32_t any_bad;
  if (t == 0) any_bad = 0;
  __syncthreads();
  if (bad) any_bad = 1;  // (a thread's own zeta - y_k: not uniform)
  air_check_verdict(sum, open_q, Z, n_queries, ok);
  if (any_bad)
    for (uint32_t q = t; q < n_queries; q += AIR_CHECK_THREADS) ok[q] = 0;
}

int launch_air_link_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_k, uint64_t w_k, uint64_t om64,
                           const void* d_gamma, void* d_tab, void* stream) {
  const uint32_t blocks = ((64u << log_blowup) + 255) / 256;
  hipLaunchKernelGGL(k_air_link_tables, dim3(blocks), dim3(256), 0, S_(stream), log_blowup, first_proof, s_n, w_n, s_k, w_k, om64,
                     reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<uint64_t*>(d_tab));
  return (int)hipGetLastError();
}
int launch_air_link_combine(uint32_t log_k, uint32_t n_proofs, const void* d_pub, const void* d_gamma, void* d_v, void* stream) {
  hipLaunchKernelGGL(k_air_link_combine, dim3(((1u << log_k) + 255) / 256, 17), dim3(256), 0, S_(stream), log_k, n_proofs,
                     reinterpret_cast<const uint64_t*>(d_pub), reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<uint64_t*>(d_v));
  return (int)hipGetLastError();
}
int launch_air_link_fold(uint32_t log_m, uint32_t log_blowup, uint32_t which, int first, const void* d_ext, const void* d_tab, void* d_pq, void* stream) {
  hipLaunchKernelGGL(k_air_link_fold, dim3((uint32_t)(((1ull << log_m) + 255) / 256)), dim3(256), 0, S_(stream), log_m, log_blowup, which,
                     first ? 1u : 0u, reinterpret_cast<const uint64_t*>(d_ext), reinterpret_cast<const uint64_t*>(d_tab), reinterpret_cast<uint64_t*>(d_pq));
  return (int)hipGetLastError();
}
int launch_air_link_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_helper_cols,
                             const void* d_tab, const void* d_pq, int form, void* d_quot, void* stream) {
  const dim3 grid((uint32_t)(((1ull << log_m) + AIR_THREADS - 1) / AIR_THREADS)), block(AIR_THREADS);
  const uint64_t* cols = reinterpret_cast<const uint64_t*>(d_cols);
  const uint64_t* hcols = reinterpret_cast<const uint64_t*>(d_helper_cols);
  const uint64_t* tab = reinterpret_cast<const uint64_t*>(d_tab);
  const uint64_t* pq = reinterpret_cast<const uint64_t*>(d_pq);
  uint64_t* out = reinterpret_cast<uint64_t*>(d_quot);
  if (form == AIR_FORM_WHOLE)
    hipLaunchKernelGGL(k_air_link_quotient<AIR_FORM_WHOLE>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, hcols, tab, pq, out);
  else if (form == AIR_FORM_PIECE)
    hipLaunchKernelGGL(k_air_link_quotient<AIR_FORM_PIECE>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, hcols, tab, pq, out);
  else
    hipLaunchKernelGGL(k_air_link_quotient<AIR_FORM_PIECE_ACC>, grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, hcols, tab, pq, out);
  return (int)hipGetLastError();
}
int launch_air_link_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint64_t om64, uint64_t om, uint64_t om_k,
                          uint64_t k_inv, const void* d_open_t, const void* d_open_h, const void* d_open_q, const void* d_zeta,
                          const void* d_gamma, const void* d_v, uint32_t n_queries, void* d_ok, void* stream) {
  hipLaunchKernelGGL(k_air_link_check, dim3(1), dim3(AIR_CHECK_THREADS), 0, S_(stream), n_proofs, log_r_t, log_r_h, log_sub, om64, om, om_k, k_inv,
                     reinterpret_cast<const uint64_t*>(d_open_t), reinterpret_cast<const uint64_t*>(d_open_h),
                     reinterpret_cast<const uint64_t*>(d_open_q), reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<const uint64_t*>(d_gamma),
                     reinterpret_cast<const uint64_t*>(d_v), n_queries, reinterpret_cast<uint32_t*>(d_ok));
  return (int)hipGetLastError();
}

int launch_air_sha_public_gather(const void* d_rows, const AirShaPublicGeom& G, uint32_t log_k, uint32_t n_proofs, void* d_pub, void* stream) {
  const uint64_t n = (uint64_t)n_proofs << log_k;
  hipLaunchKernelGGL(k_air_sha_public_gather, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S_(stream), reinterpret_cast<const uint64_t*>(d_rows), G,
                     log_k, n_proofs, reinterpret_cast<uint64_t*>(d_pub));
  return (int)hipGetLastError();
}
int launch_air_link_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, const void* d_pub, void* d_helper, void* stream) {
  const uint64_t n = (uint64_t)n_proofs << log_rows;
  hipLaunchKernelGGL(k_air_link_helper, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S_(stream), log_rows, n_proofs,
                     reinterpret_cast<const uint64_t*>(d_table), reinterpret_cast<const uint64_t*>(d_pub), reinterpret_cast<uint64_t*>(d_helper));
  return (int)hipGetLastError();
}

// ---- constraint set 7: the round constraints of the SHA-512 table (include/tmx.h "the round constraints of the SHA-512 table") -------------
// A sibling of set 3 on T.2: 64-bit words as lo / hi limbs, 80-row blocks.  No power-of-two subgroup fits 80 rows, so the selector and the
// round constants are three preprocessed columns of full degree (SEL, KLO, KHI): the prover fills and extends them like helper columns, the
// verifier evaluates them at zeta barycentrically over the N rows.  The kernels that do so, the hot pass and the check are written once for
// sets 7, 8 and 9, behind set 9's evaluator; a set's own part is its helper kernel, its evaluator and its row values.  Nothing above changes.
// Helper column offsets inside a proof's 599, table columns inside its 18 (the low limb; the high limb is the next one), constraint indices
// inside its 628.
constexpr uint32_t Q_A = 0, Q_B = 64, Q_C = 128, Q_E = 192, Q_F = 256, Q_G = 320, Q_U0 = 384, Q_U1 = 448, Q_V = 512, Q_S0 = 576, Q_S1 = 578,
                   Q_CH = 580, Q_MAJ = 582, Q_LIVE = 584, Q_KL = 585, Q_CAL = 587, Q_CAH = 590, Q_CEL = 593, Q_CEH = 596;
constexpr uint32_t R_W = 0, R_A = 2, R_B = 4, R_C = 6, R_D = 8, R_E = 10, R_F = 12, R_G = 14, R_H = 16;
constexpr uint32_t JQ_CARRY = 384, JQ_LIVE = 396, JQ_WORD = 397, JQ_U0 = 409, JQ_U1 = 473, JQ_V = 537, JQ_S0 = 601, JQ_S1 = 603, JQ_CH = 605,
                   JQ_MAJ = 607, JQ_KL = 609, JQ_SHIFT = 611, JQ_LIVEN = 623, JQ_NA = 624, JQ_NE = 626;
constexpr uint32_t SHA512_BLOCK = 80;

// SEL at row r of N: off on the last row of every block and on the wrap row N - 1 (N is no multiple of 80, so the latter is a row of its own)
__device__ __forceinline__ bool sha512_sel(uint32_t r, uint32_t n) { return r % SHA512_BLOCK != SHA512_BLOCK - 1 && r != n - 1; }

// One lane per (proof, row) of the pre-LDE table, k_air_sha_helper's shape: the eighteen limbs of the row, the block's first row (LIVE)
// and W of the next row (the carries), then 599 stores, each of them consecutive words of one column across the wave.  Operands are the
// low 32 bits of the words.  Where SEL = 1 the next row lies in the lane's own block, so KL' = LIVE K512[rnd + 1].
__global__ __launch_bounds__(256) void k_air_sha512_helper(uint32_t log_rows, uint32_t n_proofs, const uint64_t* __restrict__ table,
                                                           uint64_t* __restrict__ helper) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((uint64_t)n_proofs << log_rows)) return;
  const uint32_t p = (uint32_t)(idx >> log_rows), N = 1u << log_rows;
  const uint32_t r = (uint32_t)(idx & (N - 1)), rnd = r % SHA512_BLOCK, r0 = r - rnd;
  const uint64_t* __restrict__ t = table + (((uint64_t)p * AIR_SHA512_WIDTH) << log_rows);
  uint32_t w[AIR_SHA512_WIDTH], any = 0;
#pragma unroll
  for (uint32_t c = 0; c < AIR_SHA512_WIDTH; c++) {
    w[c] = (uint32_t)t[((uint64_t)c << log_rows) + r];
    any |= (uint32_t)t[((uint64_t)c << log_rows) + r0];
  }
  const uint32_t live = any ? 1u : 0u;
  auto word = [&](uint32_t c) { return (uint64_t)w[c] | (uint64_t)w[c + 1] << 32; };
  const uint64_t a = word(R_A), b = word(R_B), c = word(R_C), e = word(R_E), f = word(R_F), g = word(R_G);
  const uint64_t u0 = rotr64(a, 28) ^ rotr64(a, 34), u1 = rotr64(e, 14) ^ rotr64(e, 18), v = a & b;
  const uint64_t s0 = u0 ^ rotr64(a, 39), s1 = u1 ^ rotr64(e, 41);
  const uint64_t chv = (e & f) ^ (~e & g), mjv = (a & b) ^ (a & c) ^ (b & c);
  uint64_t* __restrict__ o = helper + (((uint64_t)p * AIR_SHA512_HELPER_COLS) << log_rows) + r;
  auto put = [&](uint32_t col, uint64_t x) { o[(uint64_t)col << log_rows] = x; };
#pragma unroll 4
  for (uint32_t i = 0; i < 64; i++) {
    put(Q_A + i, (a >> i) & 1);
    put(Q_B + i, (b >> i) & 1);
    put(Q_C + i, (c >> i) & 1);
    put(Q_E + i, (e >> i) & 1);
    put(Q_F + i, (f >> i) & 1);
    put(Q_G + i, (g >> i) & 1);
    put(Q_U0 + i, (u0 >> i) & 1);
    put(Q_U1 + i, (u1 >> i) & 1);
    put(Q_V + i, (v >> i) & 1);
  }
  auto put2 = [&](uint32_t col, uint64_t x) {
    put(col, (uint32_t)x);
    put(col + 1, x >> 32);
  };
  put2(Q_S0, s0);
  put2(Q_S1, s1);
  put2(Q_CH, chv);
  put2(Q_MAJ, mjv);
  put(Q_LIVE, live);
  put2(Q_KL, live ? K_SHA512[rnd] : 0);
  uint32_t cal = 0, cah = 0, cel = 0, ceh = 0;
  if (sha512_sel(r, N)) {
    const uint64_t kn = live ? K_SHA512[rnd + 1] : 0;
    const uint32_t wn_lo = (uint32_t)t[((uint64_t)R_W << log_rows) + r + 1], wn_hi = (uint32_t)t[((uint64_t)(R_W + 1) << log_rows) + r + 1];
    const uint64_t t1_lo = (uint64_t)w[R_H] + (uint32_t)s1 + (uint32_t)chv + (uint32_t)kn + wn_lo;
    const uint64_t t1_hi = (uint64_t)w[R_H + 1] + (s1 >> 32) + (chv >> 32) + (kn >> 32) + wn_hi;
    cal = (uint32_t)((t1_lo + (uint32_t)s0 + (uint32_t)mjv) >> 32) & 7;
    cah = (uint32_t)((t1_hi + (s0 >> 32) + (mjv >> 32) + cal) >> 32) & 7;
    cel = (uint32_t)((t1_lo + w[R_D]) >> 32) & 7;
    ceh = (uint32_t)((t1_hi + w[R_D + 1] + cel) >> 32) & 7;
  }
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    put(Q_CAL + k, (cal >> k) & 1);
    put(Q_CAH + k, (cah >> k) & 1);
    put(Q_CEL + k, (cel >> k) & 1);
    put(Q_CEH + k, (ceh >> k) & 1);
  }
}

// The round-bit machinery of sets 7 and 9, the 64-bit sibling of air_round_bits: six registers of a row in the roles a, b, c, e, f, g (set
// 7: themselves; set 9: b, c, d, f, g, h).  `bits` as in RoundBits, the columns 64 per register.  The six registers' table columns are t_a
// + 0, 2, 4, 8, 10, 12 and their word constraints j_word + 0, 2, .. 10; S0, S1, CH and MAJ are the helper columns h_s0 + 0, 2, 4, 6 with the
// constraints j_s0 + 0, 2, 4, 6.  Everywhere the low limb's column or index; the high limb's is the next one.
struct RoundBits512 {
  RoundBits bits;
  uint32_t t_a, j_word, h_s0, j_s0;
};
// Set 3's bit loop per 32-bit limb, the high limb first, with the rotations of SHA-512 taken mod 64 across both limbs: per bit index the
// nine bit words and the six rotated ones (A_(i+28), A_(i+34), A_(i+39), E_(i+14), E_(i+18), E_(i+41)), re-read through the cache; nine
// constraints and one Horner step by 2 of the ten word sums.  The ten sums of a limb go into its word constraints before the other limb
// starts, so no more than ten are ever live.
template <class F, class View>
__device__ __forceinline__ void air_round_bits512(View& at, const RoundBits512 s) {
  using A = Forms<F>;
  using T = typename F::T;
  const RoundBits r = s.bits;
#pragma unroll 1
  for (uint32_t l = 2; l-- > 0;) {
    RoundWords<F> w = {F::zero(), F::zero(), F::zero(), F::zero(), F::zero(), F::zero(), F::zero(), F::zero(), F::zero(), F::zero()};
#pragma unroll View::BITS
    for (uint32_t b = 32; b-- > 0;) {
      const uint32_t i = 32 * l + b;
      const T A_ = at.again(r.a + i), B = at.once(r.b + i), C = at.once(r.c + i), E = at.again(r.e + i), F_ = at.once(r.f + i), G = at.once(r.g + i);
      const T U0 = at.once(r.u0 + i), U1 = at.once(r.u1 + i), V = at.once(r.v + i);
      const T A28 = at.again(r.a + ((i + 28) & 63)), A34 = at.again(r.a + ((i + 34) & 63)), A39 = at.again(r.a + ((i + 39) & 63));
      const T E14 = at.again(r.e + ((i + 14) & 63)), E18 = at.again(r.e + ((i + 18) & 63)), E41 = at.again(r.e + ((i + 41) & 63));
      at.plain(r.a + i, A::boolean(A_));
      at.plain(r.b + i, A::boolean(B));
      at.plain(r.c + i, A::boolean(C));
      at.plain(r.e + i, A::boolean(E));
      at.plain(r.f + i, A::boolean(F_));
      at.plain(r.g + i, A::boolean(G));
      at.plain(r.j_u0 + i, A::sub(U0, A::exor(A28, A34)));
      at.plain(r.j_u1 + i, A::sub(U1, A::exor(E14, E18)));
      at.plain(r.j_v + i, A::sub(V, A::mul(A_, B)));
      w.a = A::dbl_add(w.a, A_);
      w.b = A::dbl_add(w.b, B);
      w.c = A::dbl_add(w.c, C);
      w.e = A::dbl_add(w.e, E);
      w.f = A::dbl_add(w.f, F_);
      w.g = A::dbl_add(w.g, G);
      w.s0 = A::dbl_add(w.s0, A::exor(U0, A39));
      w.s1 = A::dbl_add(w.s1, A::exor(U1, E41));
      w.ch = A::dbl_add(w.ch, A::add(G, A::mul(E, A::sub(F_, G))));
      w.maj = A::dbl_add(w.maj, A::add(V, A::mul(C, A::sub(A::add(A_, B), A::add(V, V)))));
    }
    at.plain(s.j_word + 0 + l, A::sub(at.tbl(s.t_a + 0 + l), w.a));
    at.plain(s.j_word + 2 + l, A::sub(at.tbl(s.t_a + 2 + l), w.b));
    at.plain(s.j_word + 4 + l, A::sub(at.tbl(s.t_a + 4 + l), w.c));
    at.plain(s.j_word + 6 + l, A::sub(at.tbl(s.t_a + 8 + l), w.e));
    at.plain(s.j_word + 8 + l, A::sub(at.tbl(s.t_a + 10 + l), w.f));
    at.plain(s.j_word + 10 + l, A::sub(at.tbl(s.t_a + 12 + l), w.g));
    at.plain(s.j_s0 + 0 + l, A::sub(at.again(s.h_s0 + 0 + l), w.s0));
    at.plain(s.j_s0 + 2 + l, A::sub(at.again(s.h_s0 + 2 + l), w.s1));
    at.plain(s.j_s0 + 4 + l, A::sub(at.again(s.h_s0 + 4 + l), w.ch));
    at.plain(s.j_s0 + 6 + l, A::sub(at.again(s.h_s0 + 6 + l), w.maj));
  }
}
// The twelve carry bits of sets 7 and 9 (CAL, CAH, CEL, CEH, three bits each from helper column h on): their X^2 - X constraints from index j
// on and the four values.  In full under either view: carry stays in registers.
template <class F, class View>
__device__ __forceinline__ void air_carries512(View& at, uint32_t h, uint32_t j, typename F::T carry[4]) {
  using A = Forms<F>;
  using T = typename F::T;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const T x0 = at.once(h + 3 * k), x1 = at.once(h + 3 * k + 1), x2 = at.once(h + 3 * k + 2);
    at.plain(j + 3 * k, A::boolean(x0));
    at.plain(j + 3 * k + 1, A::boolean(x1));
    at.plain(j + 3 * k + 2, A::boolean(x2));
    carry[k] = A::add(x0, A::add(A::add(x1, x1), A::scale(x2, 4)));
  }
}

// The 628 constraints of one proof at one point; klo and khi are KLO and KHI at the point.  The bit loop on a, b, c, e, f, g; behind it the
// words are read again for the two-limb updates; the thirteen selected constraints go to a gamma sum of their own: SEL(x) is factored out
// of it, the kernel applies it once.
template <class F, class View>
__device__ __forceinline__ void air_sha512_constraints(View& at, typename F::T klo, typename F::T khi) {
  using A = Forms<F>;
  using T = typename F::T;
  static_assert(R_B == R_A + 2 && R_C == R_A + 4 && R_E == R_A + 8 && R_F == R_A + 10 && R_G == R_A + 12 && R_H == R_A + 14 && Q_S1 == Q_S0 + 2 &&
                    Q_CH == Q_S0 + 4 && Q_MAJ == Q_S0 + 6 && JQ_S1 == JQ_S0 + 2 && JQ_CH == JQ_S0 + 4 && JQ_MAJ == JQ_S0 + 6,
                "RoundBits512 counts on these strides");
  air_round_bits512<F>(at, {{Q_A, Q_B, Q_C, Q_E, Q_F, Q_G, Q_U0, Q_U1, Q_V, JQ_U0, JQ_U1, JQ_V}, R_A, JQ_WORD, Q_S0, JQ_S0});
  const T LIVE = at.again(Q_LIVE);
  at.plain(JQ_LIVE, A::boolean(LIVE));
  at.plain(JQ_KL, A::sub(at.again(Q_KL), A::mul(LIVE, klo)));
  at.plain(JQ_KL + 1, A::sub(at.again(Q_KL + 1), A::mul(LIVE, khi)));
  at.selected(JQ_LIVEN, A::sub(at.next(Q_LIVE), LIVE));
  T carry[4];  // the values CAL, CAH, CEL, CEH
  air_carries512<F>(at, Q_CAL, JQ_CARRY, carry);
#pragma unroll
  for (uint32_t l = 0; l < 2; l++) {
    const T ta = at.tbl(R_A + l), tb = at.tbl(R_B + l), tc = at.tbl(R_C + l), td = at.tbl(R_D + l), te = at.tbl(R_E + l), tf = at.tbl(R_F + l),
            tg = at.tbl(R_G + l), th = at.tbl(R_H + l);
    at.selected(JQ_SHIFT + 0 + l, A::sub(at.tbl_next(R_B + l), ta));
    at.selected(JQ_SHIFT + 2 + l, A::sub(at.tbl_next(R_C + l), tb));
    at.selected(JQ_SHIFT + 4 + l, A::sub(at.tbl_next(R_D + l), tc));
    at.selected(JQ_SHIFT + 6 + l, A::sub(at.tbl_next(R_F + l), te));
    at.selected(JQ_SHIFT + 8 + l, A::sub(at.tbl_next(R_G + l), tf));
    at.selected(JQ_SHIFT + 10 + l, A::sub(at.tbl_next(R_H + l), tg));
    const T t1 = A::add(A::add(A::add(th, at.again(Q_S1 + l)), A::add(at.again(Q_CH + l), at.next(Q_KL + l))), at.tbl_next(R_W + l));
    T na = A::sub(A::add(at.tbl_next(R_A + l), A::scale(carry[l], 1ull << 32)), A::add(t1, A::add(at.again(Q_S0 + l), at.again(Q_MAJ + l))));
    T ne = A::sub(A::add(at.tbl_next(R_E + l), A::scale(carry[2 + l], 1ull << 32)), A::add(td, t1));
    if (l) {  // the carry out of the low limb comes in
      na = A::sub(na, carry[0]);
      ne = A::sub(ne, carry[2]);
    }
    at.selected(JQ_NA + l, na);
    at.selected(JQ_NE + l, ne);
  }
}

// ---- constraint set 8: the message schedule of the SHA-512 table (include/tmx.h "the message schedule of the SHA-512 table") ----------------
// A sibling of set 4 on T.2: W as lo / hi limbs, the schedule sum as one carry-free pipeline per limb, 80-row blocks.  The selector "the
// next row is a schedule row" has the period 80: one preprocessed column of full degree (SCH).
// Helper column offsets inside a proof's 230 (QL_k at Z_QL + k, QH_k at Z_QH + k), constraint indices inside its 234 (the pipelines' at
// JZ_QL + k and JZ_QH + k).  The low limb's column or index first; the high limb's is the next one.
constexpr uint32_t Z_WB = 0, Z_X0 = 64, Z_X1 = 128, Z_G0 = 192, Z_G1 = 194, Z_QL = 195, Z_QH = 210, Z_CL = 226, Z_CH = 228;
constexpr uint32_t JZ_CARRY = 64, JZ_WORD = 68, JZ_X0 = 70, JZ_X1 = 134, JZ_G0 = 198, JZ_G1 = 200, JZ_QL = 201, JZ_QH = 216, JZ_NEXT = 232;

__device__ __forceinline__ uint64_t sched512_s0(uint64_t w) { return rotr64(w, 1) ^ rotr64(w, 8) ^ (w >> 7); }
__device__ __forceinline__ uint64_t sched512_s1(uint64_t w) { return rotr64(w, 19) ^ rotr64(w, 61) ^ (w >> 6); }

// SCH at row r of N: on where the NEXT row is a schedule row of the same block, off on the wrap row N - 1 ((N - 1) mod 80 always lies in
// 15 .. 78, while row 0 is W_0 of a block)
__device__ __forceinline__ bool sha512_sch(uint32_t r, uint32_t n) {
  const uint32_t t = r % SHA512_BLOCK;
  return t >= 15 && t <= SHA512_BLOCK - 2 && r != n - 1;
}

// One lane per (proof, row) of the pre-LDE table, k_air_sched_helper's shape: 230 stores, each of them consecutive words of one column
// across the wave.  Both pipelines unrolled: Q_k(r) = W(r-k) + sigma0(W(r-k+1)) + [k >= 9] W(r-k+9) + [k >= 14] sigma1(W(r-k+14)) per limb
// and without carries, rows cyclic inside the proof, so the lane reads W of the sixteen rows r - 15 .. r and recomputes sigma0 / sigma1
// instead of exchanging them.  The operands are the low 32 bits of the two W columns.
__global__ __launch_bounds__(256) void k_air_sha512_sched_helper(uint32_t log_rows, uint32_t n_proofs, const uint64_t* __restrict__ table,
                                                                 uint64_t* __restrict__ helper) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((uint64_t)n_proofs << log_rows)) return;
  const uint32_t p = (uint32_t)(idx >> log_rows);
  const uint64_t mask = (1ull << log_rows) - 1, r = idx & mask;
  const uint64_t* __restrict__ t = table + (((uint64_t)p * AIR_SHA512_WIDTH) << log_rows);  // (W lo is column 0, W hi column 1)
  uint64_t w[16];  // w[d] = W(r - d)
#pragma unroll
  for (uint32_t d = 0; d < 16; d++) w[d] = (uint64_t)(uint32_t)t[(r - d) & mask] | (uint64_t)(uint32_t)t[(mask + 1) + ((r - d) & mask)] << 32;
  const uint64_t w0 = w[0], x0 = rotr64(w0, 1) ^ rotr64(w0, 8), x1 = rotr64(w0, 19) ^ rotr64(w0, 61);
  uint64_t* __restrict__ o = helper + (((uint64_t)p * AIR_SHA512_SCHED_HELPER_COLS) << log_rows) + r;
  auto put = [&](uint32_t col, uint64_t x) { o[(uint64_t)col << log_rows] = x; };
#pragma unroll 4
  for (uint32_t i = 0; i < 64; i++) {
    put(Z_WB + i, (w0 >> i) & 1);
    put(Z_X0 + i, (x0 >> i) & 1);
    put(Z_X1 + i, (x1 >> i) & 1);
  }
  const uint64_t g0 = sched512_s0(w0), g1 = sched512_s1(w0);
  put(Z_G0, (uint32_t)g0);
  put(Z_G0 + 1, g0 >> 32);
  put(Z_G1, (uint32_t)g1);
  put(Z_G1 + 1, g1 >> 32);
  uint64_t ql15 = 0, qh15 = 0;
#pragma unroll
  for (uint32_t k = 1; k <= 15; k++) {
    const uint64_t s0 = sched512_s0(w[k - 1]);
    uint64_t ql = (uint64_t)(uint32_t)w[k] + (uint32_t)s0, qh = (w[k] >> 32) + (s0 >> 32);
    if (k >= 9) ql += (uint32_t)w[k - 9], qh += w[k - 9] >> 32;
    if (k >= 14) {
      const uint64_t s1 = sched512_s1(w[k - 14]);
      ql += (uint32_t)s1, qh += s1 >> 32;
    }
    put(Z_QL + k, ql);
    put(Z_QH + k, qh);
    ql15 = ql, qh15 = qh;
  }
  uint32_t cl = 0, ch = 0;
  if (sha512_sch((uint32_t)r, (uint32_t)(mask + 1))) {
    cl = (uint32_t)(ql15 >> 32) & 3;
    ch = (uint32_t)((qh15 + cl) >> 32) & 3;
  }
  put(Z_CL, cl & 1);
  put(Z_CL + 1, cl >> 1);
  put(Z_CH, ch & 1);
  put(Z_CH + 1, ch >> 1);
}

// The 234 constraints of one proof at one point.  The bit loop is set 4's (air_sched_constraints) per 32-bit limb, the high limb first, with
// the rotations of SHA-512 taken mod 64 across both limbs as column offsets: per bit index i the pass holds WB_i, X0_i, X1_i and the rotated
// or shifted bit words (WB_(i+1), WB_(i+8), WB_(i+19), WB_(i+61), and WB_(i+7) for i < 57, WB_(i+6) for i < 58), re-read through the cache.
// Per i: three constraints (X^2 - X, X0, X1) and one Horner step by 2 of the limb's three word sums: 5 reduced column products and 6 gamma
// weights, as in set 4.  A limb's three sums go into its word constraints before the other limb starts, so no more than three are ever
// live.  Behind the loops the four carry bits, the two pipelines (linear) and the two selected constraints, which go to a gamma sum of
// their own: SCH(x) is factored out of it, the kernel applies it once.
template <class F, class View>
__device__ __forceinline__ void air_sha512_sched_constraints(View& at) {
  using A = Forms<F>;
  using T = typename F::T;
#pragma unroll 1
  for (uint32_t l = 2; l-- > 0;) {
    T ww = F::zero(), wg0 = F::zero(), wg1 = F::zero();
#pragma unroll View::BITS
    for (uint32_t b = 32; b-- > 0;) {
      const uint32_t i = 32 * l + b;
      const T WB = at.again(Z_WB + i), X0 = at.once(Z_X0 + i), X1 = at.once(Z_X1 + i);
      const T W1 = at.again(Z_WB + ((i + 1) & 63)), W8 = at.again(Z_WB + ((i + 8) & 63));
      const T W19 = at.again(Z_WB + ((i + 19) & 63)), W61 = at.again(Z_WB + ((i + 61) & 63));
      at.plain(Z_WB + i, A::boolean(WB));
      at.plain(JZ_X0 + i, A::sub(X0, A::exor(W1, W8)));
      at.plain(JZ_X1 + i, A::sub(X1, A::exor(W19, W61)));
      ww = A::dbl_add(ww, WB);
      wg0 = A::dbl_add(wg0, i < 57 ? A::exor(X0, at.again(Z_WB + i + 7)) : X0);  // (i is uniform: a scalar branch)
      wg1 = A::dbl_add(wg1, i < 58 ? A::exor(X1, at.again(Z_WB + i + 6)) : X1);
    }
    at.plain(JZ_WORD + l, A::sub(at.tbl(R_W + l), ww));
    at.plain(JZ_G0 + l, A::sub(at.again(Z_G0 + l), wg0));
    at.plain(JZ_G1 + l, A::sub(at.again(Z_G1 + l), wg1));
  }
  // the values CL, CH (two scalars, not an array: the limb loop below is not unrolled)
  const T cl0 = at.once(Z_CL), cl1 = at.once(Z_CL + 1), ch0 = at.once(Z_CH), ch1 = at.once(Z_CH + 1);
  at.plain(JZ_CARRY, A::boolean(cl0));
  at.plain(JZ_CARRY + 1, A::boolean(cl1));
  at.plain(JZ_CARRY + 2, A::boolean(ch0));
  at.plain(JZ_CARRY + 3, A::boolean(ch1));
  const T CL = A::add(cl0, A::add(cl1, cl1)), CH = A::add(ch0, A::add(ch1, ch1));
  // one pipeline at a time, as the bit loop takes one limb at a time: the fifteen Q_k and Q_k' of a limb are spent before the other starts
#pragma unroll 1
  for (uint32_t l = 0; l < 2; l++) {
    const uint32_t zq = l ? Z_QH : Z_QL, jq = l ? JZ_QH : JZ_QL;  // (l is uniform: scalar selects)
    const T Wn = at.tbl_next(R_W + l);
    T prev = A::add(at.tbl(R_W + l), at.next(Z_G0 + l));  // what Q_k' must equal: W + G0' for k = 1, then Q_(k-1) (+ W' for k = 9, + G1' for k = 14)
#pragma unroll View::SHORT
    for (uint32_t k = 1; k <= 15; k++) {
      at.plain(jq + k, A::sub(at.next(zq + k), prev));
      prev = at.again(zq + k);
      if (k + 1 == 9) prev = A::add(prev, Wn);
      if (k + 1 == 14) prev = A::add(prev, at.next(Z_G1 + l));
    }
    // (prev = Q_15)  W' + 2^32 C - Q_15, and in the high limb the carry out of the low limb comes in
    T nw = A::sub(A::add(Wn, A::scale(l ? CH : CL, 1ull << 32)), prev);
    if (l) nw = A::sub(nw, CL);
    at.selected(JZ_NEXT + l, nw);
  }
}

// ---- constraint set 9: the block starts of the SHA-512 table (include/tmx.h "the block starts of the SHA-512 table") ------------------------
// A sibling of set 5 on T.2: row 0 of a block is round 0 applied to the eight words the block starts from, so six of them stand in row 0
// itself (b, c, d, f, g, h) and the bit loop (air_round_bits512) runs on them with the register names shifted by one.  A lane is two
// blocks of 80 rows: the selectors "the next row starts a hash" and "the next row starts a second block" are two preprocessed columns of
// full degree (STA, CHN).
// Helper column offsets inside a proof's 629 (a word's low limb first; PZ_j and CZ_j at + 2 j), constraint indices inside its 673.
constexpr uint32_t Y_B = 0, Y_C = 64, Y_D = 128, Y_F = 192, Y_G = 256, Y_H = 320, Y_U0 = 384, Y_U1 = 448, Y_V = 512, Y_S0 = 576, Y_S1 = 578,
                   Y_CH = 580, Y_MAJ = 582, Y_LV = 584, Y_PZ = 585, Y_CZ = 601, Y_CAL = 617, Y_CAH = 620, Y_CEL = 623, Y_CEH = 626;
constexpr uint32_t JY_CZ = 384, JY_CARRY = 400, JY_LV = 412, JY_WORD = 413, JY_U0 = 425, JY_U1 = 489, JY_V = 553, JY_S0 = 617, JY_S1 = 619,
                   JY_CH = 621, JY_MAJ = 623, JY_PZ = 625, JY_START = 641, JY_CHAIN = 657;
constexpr uint32_t SHA512_LANE = 2 * SHA512_BLOCK;
__device__ __constant__ const uint64_t IV_SHA512[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                                                       0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
constexpr uint64_t INIT512_IV3 = 0xa54ff53a5f1d36f1ull, INIT512_IV7 = 0x5be0cd19137e2179ull, INIT512_K0 = 0x428a2f98d728ae22ull;
// limb l of a 64-bit constant
__host__ __device__ constexpr uint64_t limb_of(uint64_t x, uint32_t l) { return l ? x >> 32 : x & 0xffffffffull; }

// STA at row r of N: on where the NEXT row is row 0 of a first block.  The wrap row N - 1 is switched on explicitly: row 0 starts a hash,
// and (N - 1) mod 160 is 127, 95, 31 or 63, never 159.  CHN: on where the next row is row 0 of a second block (never the wrap row).
__device__ __forceinline__ bool sha512_sta(uint32_t r, uint32_t n) { return r % SHA512_LANE == SHA512_LANE - 1 || r == n - 1; }
__device__ __forceinline__ bool sha512_chn(uint32_t r) { return r % SHA512_LANE == SHA512_BLOCK - 1; }

// One lane per (proof, row) of the pre-LDE table, k_air_sha512_helper's shape: the eighteen limbs of the row and the block's first row
// (LV), then 629 stores, each of them consecutive words of one column across the wave.  The next row (cyclic inside the proof) is loaded
// only where STA or CHN is on: there it is row 0 of its block, so it gives LV' and the two round-0 sums; on every other row the next row
// lies in the lane's own block and LV' = LV.  Operands are the low 32 bits of the words.
__global__ __launch_bounds__(256) void k_air_sha512_init_helper(uint32_t log_rows, uint32_t n_proofs, const uint64_t* __restrict__ table,
                                                                uint64_t* __restrict__ helper) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((uint64_t)n_proofs << log_rows)) return;
  const uint32_t p = (uint32_t)(idx >> log_rows), N = 1u << log_rows;
  const uint32_t r = (uint32_t)(idx & (N - 1)), r0 = r - r % SHA512_BLOCK;
  const uint64_t* __restrict__ t = table + (((uint64_t)p * AIR_SHA512_WIDTH) << log_rows);
  uint32_t w[AIR_SHA512_WIDTH], any = 0;
#pragma unroll
  for (uint32_t c = 0; c < AIR_SHA512_WIDTH; c++) {
    w[c] = (uint32_t)t[((uint64_t)c << log_rows) + r];
    any |= (uint32_t)t[((uint64_t)c << log_rows) + r0];
  }
  const uint32_t live = any ? 1u : 0u;
  const bool chn = sha512_chn(r), edge = chn || sha512_sta(r, N);
  uint32_t n[AIR_SHA512_WIDTH] = {}, live_next = live;
  if (edge) {
    const uint32_t rn = (r + 1) & (N - 1);
    uint32_t any_next = 0;
#pragma unroll
    for (uint32_t c = 0; c < AIR_SHA512_WIDTH; c++) {
      n[c] = (uint32_t)t[((uint64_t)c << log_rows) + rn];
      any_next |= n[c];
    }
    live_next = any_next ? 1u : 0u;
  }
  auto word = [&](const uint32_t* x, uint32_t c) { return (uint64_t)x[c] | (uint64_t)x[c + 1] << 32; };
  const uint64_t b = word(w, R_B), c = word(w, R_C), d = word(w, R_D), f = word(w, R_F), g = word(w, R_G), hh = word(w, R_H);
  const uint64_t u0 = rotr64(b, 28) ^ rotr64(b, 34), u1 = rotr64(f, 14) ^ rotr64(f, 18), v = b & c;
  uint64_t* __restrict__ o = helper + (((uint64_t)p * AIR_SHA512_INIT_HELPER_COLS) << log_rows) + r;
  auto put = [&](uint32_t col, uint64_t x) { o[(uint64_t)col << log_rows] = x; };
#pragma unroll 4
  for (uint32_t i = 0; i < 64; i++) {
    put(Y_B + i, (b >> i) & 1);
    put(Y_C + i, (c >> i) & 1);
    put(Y_D + i, (d >> i) & 1);
    put(Y_F + i, (f >> i) & 1);
    put(Y_G + i, (g >> i) & 1);
    put(Y_H + i, (hh >> i) & 1);
    put(Y_U0 + i, (u0 >> i) & 1);
    put(Y_U1 + i, (u1 >> i) & 1);
    put(Y_V + i, (v >> i) & 1);
  }
  auto put2 = [&](uint32_t col, uint64_t x) {
    put(col, (uint32_t)x);
    put(col + 1, x >> 32);
  };
  put2(Y_S0, u0 ^ rotr64(b, 39));
  put2(Y_S1, u1 ^ rotr64(f, 41));
  put2(Y_CH, (f & g) ^ (~f & hh));
  put2(Y_MAJ, (b & c) ^ (b & d) ^ (c & d));
  put(Y_LV, live);
  uint64_t pz3 = 0, pz7 = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    const uint64_t lo = limb_of(IV_SHA512[j], 0) + w[R_A + 2 * j], czl = lo >> 32;
    const uint64_t hi = limb_of(IV_SHA512[j], 1) + w[R_A + 2 * j + 1] + czl, czh = hi >> 32;
    const uint64_t pz = live_next ? (uint64_t)(uint32_t)lo | hi << 32 : 0;
    put2(Y_PZ + 2 * j, pz);
    put(Y_CZ + 2 * j, czl);
    put(Y_CZ + 2 * j + 1, czh);
    if (j == 3) pz3 = pz;
    if (j == 7) pz7 = pz;
  }
  uint32_t cal = 0, cah = 0, cel = 0, ceh = 0;
  if (edge) {  // round 0 of the next row's block, from the IV (a start row) or from PZ (a chain row)
    const uint64_t nb = word(n, R_B), nc = word(n, R_C), nd = word(n, R_D), nf = word(n, R_F), ng = word(n, R_G), nh = word(n, R_H);
    const uint64_t s0 = rotr64(nb, 28) ^ rotr64(nb, 34) ^ rotr64(nb, 39), s1 = rotr64(nf, 14) ^ rotr64(nf, 18) ^ rotr64(nf, 41);
    const uint64_t chv = (nf & ng) ^ (~nf & nh), mjv = (nb & nc) ^ (nb & nd) ^ (nc & nd);
    const uint64_t k0 = live_next ? INIT512_K0 : 0;
    const uint64_t h7 = chn ? pz7 : live_next ? INIT512_IV7 : 0, h3 = chn ? pz3 : live_next ? INIT512_IV3 : 0;
    const uint64_t t1_lo = limb_of(s1, 0) + limb_of(chv, 0) + n[R_W] + limb_of(k0, 0);
    const uint64_t t1_hi = limb_of(s1, 1) + limb_of(chv, 1) + n[R_W + 1] + limb_of(k0, 1);
    cal = (uint32_t)((limb_of(h7, 0) + t1_lo + limb_of(s0, 0) + limb_of(mjv, 0)) >> 32) & 7;
    cah = (uint32_t)((limb_of(h7, 1) + t1_hi + limb_of(s0, 1) + limb_of(mjv, 1) + cal) >> 32) & 7;
    cel = (uint32_t)((limb_of(h3, 0) + limb_of(h7, 0) + t1_lo) >> 32) & 7;
    ceh = (uint32_t)((limb_of(h3, 1) + limb_of(h7, 1) + t1_hi + cel) >> 32) & 7;
  }
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    put(Y_CAL + k, (cal >> k) & 1);
    put(Y_CAH + k, (cah >> k) & 1);
    put(Y_CEL + k, (cel >> k) & 1);
    put(Y_CEH + k, (ceh >> k) & 1);
  }
}

// The 673 constraints of one proof at one point.  The bit loop (air_round_bits512) on b, c, d, f, g, h in the roles a, b, c, e, f, g.
// Behind it LV, the twelve carry bits, and one rolled loop over the eight words the next block starts from: per word and limb the CZ
// bit, the PZ constraint (it holds on every row: no selector) and, for the six words that stand in row 0, the two selected linear forms
// at the next row.  The selected forms go to two gamma sums of their own (started, chained): STA(x) and CHN(x) are factored out of them,
// the kernel applies each once.
template <class F, class View>
__device__ __forceinline__ void air_sha512_init_constraints(View& at) {
  using A = Forms<F>;
  using T = typename F::T;
  static_assert(Y_S1 == Y_S0 + 2 && Y_CH == Y_S0 + 4 && Y_MAJ == Y_S0 + 6 && JY_S1 == JY_S0 + 2 && JY_CH == JY_S0 + 4 && JY_MAJ == JY_S0 + 6,
                "RoundBits512 counts on these strides");
  air_round_bits512<F>(at, {{Y_B, Y_C, Y_D, Y_F, Y_G, Y_H, Y_U0, Y_U1, Y_V, JY_U0, JY_U1, JY_V}, R_B, JY_WORD, Y_S0, JY_S0});
  at.plain(JY_LV, A::boolean(at.again(Y_LV)));
  T carry[4];  // the values CAL, CAH, CEL, CEH
  air_carries512<F>(at, Y_CAL, JY_CARRY, carry);
  // PZ_(j,l) - LV' (IV_(j,l) + s_(j,l) [+ CZL_j] - 2^32 CZ_(j,l)), and with each of the six words that stand in row 0 its two selected
  // linear forms per limb: the next row's limb against IV_(j,l) LV' (start rows) and against PZ_(j,l) (chain rows).  Rolled over j.
  const T LVn = at.next(Y_LV);
  T pz3[2] = {F::zero(), F::zero()}, pz7[2] = {F::zero(), F::zero()};
#pragma unroll 1
  for (uint32_t j = 0; j < 8; j++) {
    const uint64_t iv = IV_SHA512[j];  // (j is uniform: a scalar load)
    T czl = F::zero();
#pragma unroll
    for (uint32_t l = 0; l < 2; l++) {
      const T CZ = at.once(Y_CZ + 2 * j + l), PZ = at.once(Y_PZ + 2 * j + l);
      at.plain(JY_CZ + 2 * j + l, A::boolean(CZ));
      T s = A::sub(A::add_const(at.tbl(R_A + 2 * j + l), limb_of(iv, l)), A::scale(CZ, 1ull << 32));
      if (l) s = A::add(s, czl);  // the carry out of the low limb comes in
      else czl = CZ;
      at.plain(JY_PZ + 2 * j + l, A::sub(PZ, A::mul(LVn, s)));
      if (j == 3) pz3[l] = PZ;
      if (j == 7) pz7[l] = PZ;
      if (j != 3 && j != 7) {
        const uint32_t k = j < 3 ? j : j - 1;
        const T xn = at.tbl_next(R_B + 2 * j + l);
        at.started(JY_START + 2 * k + l, A::sub(xn, A::scale(LVn, limb_of(iv, l))));
        at.chained(JY_CHAIN + 2 * k + l, A::sub(xn, PZ));
      }
    }
  }
  // round 0 of the next row's block: a' and e' per limb against the two sums, the low limb's carry entering the high limb
#pragma unroll
  for (uint32_t l = 0; l < 2; l++) {
    const T t1 = A::add(A::add(at.next(Y_S1 + l), at.next(Y_CH + l)), at.tbl_next(R_W + l));
    const T t12 = A::add(t1, A::add(at.next(Y_S0 + l), at.next(Y_MAJ + l)));
    T an = A::add(at.tbl_next(R_A + l), A::scale(carry[l], 1ull << 32)), en = A::add(at.tbl_next(R_E + l), A::scale(carry[2 + l], 1ull << 32));
    if (l) {
      an = A::sub(an, carry[0]);
      en = A::sub(en, carry[2]);
    }
    const T kl = A::scale(LVn, limb_of(INIT512_K0, l));
    at.started(JY_START + 12 + l, A::sub(an, A::add(A::scale(LVn, limb_of(INIT512_IV7, l) + limb_of(INIT512_K0, l)), t12)));
    at.started(JY_START + 14 + l,
               A::sub(en, A::add(A::scale(LVn, limb_of(INIT512_IV3, l) + limb_of(INIT512_IV7, l) + limb_of(INIT512_K0, l)), t1)));
    at.chained(JY_CHAIN + 12 + l, A::sub(an, A::add(A::add(pz7[l], kl), t12)));
    at.chained(JY_CHAIN + 14 + l, A::sub(en, A::add(A::add(pz3[l], pz7[l]), A::add(kl, t1))));
  }
}

// ---- sets 7, 8 and 9: the kernels around the preprocessed columns ----------------------------------------------------------------------------
// What a set is to them: its counts and table offsets (air.h), the values of its preprocessed planes at row r of N, and how a proof at one
// point becomes one value given the planes at that point.  The first SELECTORS planes hold 0 / 1 and weigh the proof's selected gamma
// sums (View::combined); set 7's other two are operands of its evaluator.  Every kernel below is written once over such a descriptor.
struct Sha512Round {  // set 7: SEL, KLO, KHI
  static constexpr uint32_t PLANES = 3, SELECTORS = 1, HELPER_COLS = AIR_SHA512_HELPER_COLS, CONSTRAINTS = AIR_SHA512_CONSTRAINTS;
  static constexpr uint32_t TAB_GPOW = AIR7_TAB_GPOW, TAB_ZINV = AIR7_TAB_ZINV, PART_WORDS = AIR7_PART_WORDS;
  static __device__ __forceinline__ void planes(uint32_t r, uint32_t n, uint64_t v[PLANES]) {
    const uint64_t k = K_SHA512[r % SHA512_BLOCK];
    v[0] = sha512_sel(r, n) ? 1 : 0;
    v[1] = (uint32_t)k;
    v[2] = k >> 32;
  }
  template <class F, class View>
  static __device__ __forceinline__ gl2 proof(View& at, const typename F::T* pv) {
    air_sha512_constraints<F>(at, pv[1], pv[2]);
    return at.template combined<SELECTORS>(pv);
  }
};
struct Sha512Sched {  // set 8: SCH
  static constexpr uint32_t PLANES = 1, SELECTORS = 1, HELPER_COLS = AIR_SHA512_SCHED_HELPER_COLS, CONSTRAINTS = AIR_SHA512_SCHED_CONSTRAINTS;
  static constexpr uint32_t TAB_GPOW = AIR8_TAB_GPOW, TAB_ZINV = AIR8_TAB_ZINV, PART_WORDS = AIR8_PART_WORDS;
  static __device__ __forceinline__ void planes(uint32_t r, uint32_t n, uint64_t v[PLANES]) { v[0] = sha512_sch(r, n) ? 1 : 0; }
  template <class F, class View>
  static __device__ __forceinline__ gl2 proof(View& at, const typename F::T* pv) {
    air_sha512_sched_constraints<F>(at);
    return at.template combined<SELECTORS>(pv);
  }
};
struct Sha512Init {  // set 9: STA, CHN
  static constexpr uint32_t PLANES = 2, SELECTORS = 2, HELPER_COLS = AIR_SHA512_INIT_HELPER_COLS, CONSTRAINTS = AIR_SHA512_INIT_CONSTRAINTS;
  static constexpr uint32_t TAB_GPOW = AIR9_TAB_GPOW, TAB_ZINV = AIR9_TAB_ZINV, PART_WORDS = AIR9_PART_WORDS;
  static __device__ __forceinline__ void planes(uint32_t r, uint32_t n, uint64_t v[PLANES]) {
    v[0] = sha512_sta(r, n) ? 1 : 0;
    v[1] = sha512_chn(r) ? 1 : 0;
  }
  template <class F, class View>
  static __device__ __forceinline__ gl2 proof(View& at, const typename F::T* pv) {
    air_sha512_init_constraints<F>(at);
    return at.template combined<SELECTORS>(pv);
  }
};

// Set 10, the link to Level-1 (its public table and helper kernels stand at the end of this file; the block "constraint set 10" there says
// what the columns are).  Helper column offsets inside a proof's 65, public columns inside its 49 (a word's low limb first: word j at
// + 2 j, + 2 j + 1), constraint indices inside its 115 (a family's member 2 j + limb).
constexpr uint32_t L_CV = 0, L_DG = 16, L_CD = 32, L_LN = 48, L_CH = 49;
constexpr uint32_t U_W = 0, U_DIG = 32, U_LV = 48;
constexpr uint32_t JL_CD = 0, JL_SUM = 16, JL_CH = 32, JL_SEL = 48, JL_CHN = 64, JL_STA = 80, JL_LVN = 96, JL_DIG = 97, JL_MSG = 113;

// The 115 constraints of one proof at one point: the column parts -- what the public polynomial Pub_gamma is subtracted from (the families
// from JL_LVN on carry a public term).  Every nonlinear one has degree 2 and no selector; a selected one is a plane times a linear form.
// STA(x) and CHN(x) are factored out into the started and the chained sum (the kernel applies each once); SEL, E79 and MSG are operands.
template <class F, class View>
__device__ __forceinline__ void air_sha512_link_constraints(View& at, typename F::T SEL, typename F::T E79, typename F::T MSG) {
  using A = Forms<F>;
  using T = typename F::T;
  const T LN = at.again(L_LN);
#pragma unroll 1
  for (uint32_t j = 0; j < 8; j++) {
    const uint64_t iv = IV_SHA512[j];  // (j is uniform: a scalar load)
    T cdl = F::zero();
#pragma unroll
    for (uint32_t l = 0; l < 2; l++) {
      const uint32_t c = 2 * j + l;
      const T CV = at.once(L_CV + c), DG = at.once(L_DG + c), CD = at.once(L_CD + c), CH = at.once(L_CH + c), CVn = at.next(L_CV + c);
      at.plain(JL_CD + c, A::boolean(CD));
      T s = A::sub(A::add(DG, A::scale(CD, 1ull << 32)), A::add(CV, at.tbl(R_A + c)));
      if (l) s = A::sub(s, cdl);  // the carry out of the low limb comes in
      else cdl = CD;
      at.plain(JL_SUM + c, s);
      at.plain(JL_CH + c, A::sub(CH, A::mul(LN, DG)));
      at.plain(JL_SEL + c, A::mul(SEL, A::sub(CVn, CV)));
      at.chained(JL_CHN + c, A::sub(CVn, CH));
      at.started(JL_STA + c, A::sub(CVn, A::scale(LN, limb_of(iv, l))));
      at.plain(JL_DIG + c, A::mul(E79, DG));  // E79 DG - CHN CH
      at.chained(JL_DIG + c, A::sub(F::zero(), CH));
    }
  }
  at.started(JL_LVN, LN);  // (CHN + STA) LN
  at.chained(JL_LVN, LN);
  at.plain(JL_MSG, A::mul(MSG, at.tbl(R_W)));
  at.plain(JL_MSG + 1, A::mul(MSG, at.tbl(R_W + 1)));
}

struct Sha512Link {  // set 10: STA, CHN (set 9's), then SEL (set 7's), E79 "the last row of a block", MSG "a message row"
  static constexpr uint32_t PLANES = 5, SELECTORS = 2, HELPER_COLS = AIR_SHA512_LINK_HELPER_COLS, CONSTRAINTS = AIR_SHA512_LINK_CONSTRAINTS;
  static constexpr uint32_t TAB_GPOW = AIR10_TAB_GPOW, TAB_ZINV = AIR10_TAB_ZINV, PART_WORDS = AIR10_PART_WORDS;
  static __device__ __forceinline__ void planes(uint32_t r, uint32_t n, uint64_t v[PLANES]) {
    v[0] = sha512_sta(r, n) ? 1 : 0;
    v[1] = sha512_chn(r) ? 1 : 0;
    v[2] = sha512_sel(r, n) ? 1 : 0;
    v[3] = r % SHA512_BLOCK == SHA512_BLOCK - 1 ? 1 : 0;
    v[4] = r % SHA512_BLOCK < 16 ? 1 : 0;
  }
  template <class F, class View>
  static __device__ __forceinline__ gl2 proof(View& at, const typename F::T* pv) {
    air_sha512_link_constraints<F>(at, pv[2], pv[3], pv[4]);
    return at.template combined<SELECTORS>(pv);
  }
};

// One lane per row: the planes before the LDE, planar (PLANES << log_rows words)
template <class S>
__global__ __launch_bounds__(256) void k_air_sha512_periodic(uint32_t log_rows, uint64_t* __restrict__ pre) {
  const uint32_t N = 1u << log_rows, r = blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  uint64_t v[S::PLANES];
  S::planes(r, N, v);
#pragma unroll
  for (uint32_t j = 0; j < S::PLANES; j++) pre[j * (size_t)N + r] = v[j];
}

// One thread per table entry: 1 / (x^N - 1) by i mod B and gamma^0 .. gamma^CONSTRAINTS, gamma^(CONSTRAINTS first); the selectors and the
// round constants are columns, not tables
template <class S>
__global__ __launch_bounds__(256) void k_air_sha512_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n,
                                                           const uint64_t* __restrict__ gamma, uint64_t* __restrict__ tab) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  air_zinv_gpow(k, log_blowup, first_proof, s_n, w_n, gamma, S::CONSTRAINTS, tab + S::TAB_ZINV, tab + S::TAB_GPOW);
}

// The hot pass, k_air_sha_quotient's shape: one lane per point, a loop over the proofs from the last to the first (Horner by
// gamma^CONSTRAINTS), the eighteen table columns and the helper columns read once from HBM.  pre: the extended preprocessed planes
// (PLANES << log_m words), one word each per lane, read once per point.  Per proof S::proof; at the end 1 / (x^N - 1).  FORM as in set 3.
template <class S, int FORM>
__global__ __launch_bounds__(AIR_THREADS) void k_air_sha512_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs,
                                                                     const uint64_t* __restrict__ cols, const uint64_t* __restrict__ hcols,
                                                                     const uint64_t* __restrict__ pre, const uint64_t* __restrict__ tab,
                                                                     uint64_t* __restrict__ out) {
  const uint64_t M = 1ull << log_m, i = (uint64_t)blockIdx.x * AIR_THREADS + threadIdx.x;
  if (i >= M) return;
  const uint64_t nx = (i + (1ull << log_blowup)) & (M - 1);
  const uint64_t* __restrict__ gp = tab + S::TAB_GPOW;
  uint64_t pv[S::PLANES];
#pragma unroll
  for (uint32_t j = 0; j < S::PLANES; j++) pv[j] = gl_canon(pre[j * M + i]);
  const uint64_t zinv = tab[S::TAB_ZINV + (i & ((1ull << log_blowup) - 1))];
  const gl2 gn = {gp[2 * S::CONSTRAINTS], gp[2 * S::CONSTRAINTS + 1]};
  gl2 t = {0, 0};
  for (uint32_t p = n_proofs; p-- > 0;) {
    CosetView at = {cols + (((uint64_t)p * AIR_SHA512_WIDTH) << log_m), hcols + (((uint64_t)p * S::HELPER_COLS) << log_m), gp, log_m, i, nx};
    const gl2 v = S::template proof<FieldP>(at, pv);  // (first: t gn would be live across the evaluator)
    t = gl2_add(gl2_mul(t, gn), v);
  }
  gl2 q = gl2_scale(t, zinv);
  if (FORM != AIR_FORM_WHOLE) q = gl2_mul(q, {gp[2 * (S::CONSTRAINTS + 1)], gp[2 * (S::CONSTRAINTS + 1) + 1]});
  if (FORM == AIR_FORM_PIECE_ACC) q = gl2_add(q, {gl_canon(out[i]), gl_canon(out[M + i])});
  out[i] = q.c0;
  out[M + i] = q.c1;
}

// The planes at zeta, barycentric over the N rows: P(zeta) = (zeta^N - 1) / N  sum_r v_r omega^r / (zeta - omega^r).  Several workgroups;
// thread g of T takes the rows g, g + T, ... four at a time, inverting its four zeta - omega^r with one F_p^2 inversion (prefix products,
// one Fermat chain, back-substitution); v_r comes from r itself (S::planes).  A workgroup's sums meet in LDS and go to its row of `part`:
// [2 PLANES] words of sums, then 1 if a denominator was zero (such a term is left out).  air_sha512_periodic_at folds the rows.
constexpr int AIR_SHA512_EVAL_PER = 4;
template <class S>
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_sha512_periodic_eval(uint32_t log_rows, uint64_t om, const uint64_t* __restrict__ zeta,
                                                                                 uint64_t* __restrict__ part) {
  static_assert(2 * S::PLANES + 1 <= S::PART_WORDS, "a row of `part` holds the sums and the flag");
  __shared__ uint64_t red[2 * S::PLANES][AIR_CHECK_THREADS];
  __shared__ uint32_t bad;
  const uint32_t N = 1u << log_rows, T = gridDim.x * AIR_CHECK_THREADS, g = blockIdx.x * AIR_CHECK_THREADS + threadIdx.x;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const gl2 z = {gl_canon(zeta[0]), gl_canon(zeta[1])};
  const uint64_t stride = gl_pow(om, T);
  uint64_t y = gl_pow(om, g);
  gl2 sum[S::PLANES] = {};
  for (uint32_t r0 = g; r0 < N; r0 += AIR_SHA512_EVAL_PER * T) {
    gl2 pre[AIR_SHA512_EVAL_PER], den[AIR_SHA512_EVAL_PER];
    uint64_t yk[AIR_SHA512_EVAL_PER];
    gl2 run = {1, 0};
#pragma unroll
    for (int m = 0; m < AIR_SHA512_EVAL_PER; m++) {
      const bool in = r0 + m * T < N;
      yk[m] = y;
      den[m] = {gl_sub(z.c0, y), z.c1};
      pre[m] = run;
      if (in && den[m].c0 == 0 && den[m].c1 == 0) {
        bad = 1;
        den[m] = {1, 0};
      }
      if (in) run = gl2_mul(run, den[m]);
      y = gl_mul(y, stride);
    }
    gl2 inv = gl2_inv(run);
#pragma unroll
    for (int m = AIR_SHA512_EVAL_PER - 1; m >= 0; m--) {
      const uint32_t r = r0 + m * T;
      if (r < N) {
        const gl2 term = gl2_scale(gl2_mul(inv, pre[m]), yk[m]);  // omega^r / (zeta - omega^r)
        inv = gl2_mul(inv, den[m]);
        if (gl_sub(z.c0, yk[m]) == 0 && z.c1 == 0) continue;
        uint64_t v[S::PLANES];
        S::planes(r, N, v);
#pragma unroll
        for (uint32_t j = 0; j < S::PLANES; j++) {
          if (j >= S::SELECTORS) sum[j] = gl2_add(sum[j], gl2_scale(term, v[j]));
          else if (v[j]) sum[j] = gl2_add(sum[j], term);
        }
      }
    }
  }
  const uint32_t t = threadIdx.x;
#pragma unroll
  for (uint32_t j = 0; j < S::PLANES; j++) red[2 * j][t] = sum[j].c0, red[2 * j + 1][t] = sum[j].c1;
  for (uint32_t h = AIR_CHECK_THREADS / 2; h; h >>= 1) {
    __syncthreads();
    if (t < h)
      for (uint32_t k = 0; k < 2 * S::PLANES; k++) red[k][t] = gl_add(red[k][t], red[k][t + h]);
  }
  __syncthreads();
  if (t < 2 * S::PLANES) part[(size_t)blockIdx.x * S::PART_WORDS + t] = red[t][0];
  if (t == 2 * S::PLANES) part[(size_t)blockIdx.x * S::PART_WORDS + 2 * S::PLANES] = bad;
}

// The planes at zeta from the workgroups' rows of `part`; n_inv = 1 / N; returns false if a denominator was zero
template <class S>
__device__ __forceinline__ bool air_sha512_periodic_at(const uint64_t* __restrict__ part, uint32_t n_parts, gl2 zn, uint64_t n_inv, gl2 v[S::PLANES]) {
  uint64_t s[2 * S::PLANES] = {}, bad = 0;
  for (uint32_t k = 0; k < n_parts; k++) {
    for (uint32_t j = 0; j < 2 * S::PLANES; j++) s[j] = gl_add(s[j], part[(size_t)k * S::PART_WORDS + j]);
    bad |= part[(size_t)k * S::PART_WORDS + 2 * S::PLANES];
  }
  const gl2 lead = gl2_scale({gl_sub(zn.c0, 1), zn.c1}, n_inv);
  for (uint32_t j = 0; j < S::PLANES; j++) v[j] = gl2_mul(lead, {s[2 * j], s[2 * j + 1]});
  return bad == 0;
}

// One thread: the values (2 PLANES words), then 1 if a denominator was zero, at out[0 .. 2 PLANES]
template <class S>
__global__ void k_air_sha512_periodic_fold(uint32_t log_rows, uint32_t n_parts, uint64_t n_inv, const uint64_t* __restrict__ part,
                                           const uint64_t* __restrict__ zeta, uint64_t* __restrict__ out) {
  gl2 zn = {gl_canon(zeta[0]), gl_canon(zeta[1])}, v[S::PLANES];
  for (uint32_t k = 0; k < log_rows; k++) zn = gl2_mul(zn, zn);
  const bool fine = air_sha512_periodic_at<S>(part, n_parts, zn, n_inv, v);
  for (uint32_t j = 0; j < S::PLANES; j++) {
    out[2 * j] = v[j].c0;
    out[2 * j + 1] = v[j].c1;
  }
  out[2 * S::PLANES] = fine ? 0 : 1;
}

// The identity at zeta, one workgroup: gamma^0 .. gamma^CONSTRAINTS go to LDS first; thread t takes the proofs t, t + 256, ... and
// evaluates their constraints over F_p^2 from the table's and the helper's openings, with the planes at zeta from the barycentric
// kernel's rows.  A proof contributes gamma^(CONSTRAINTS p) S::proof; the sum is compared with (u_0 + X u_1) (zeta^N - 1).  A zero
// denominator in the barycentric sums clears every verdict.
template <class S>
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_sha512_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub,
                                                                         uint32_t n_parts, uint64_t n_inv, const uint64_t* __restrict__ part,
                                                                         const uint64_t* __restrict__ open_t, const uint64_t* __restrict__ open_h,
                                                                         const uint64_t* __restrict__ open_q, const uint64_t* __restrict__ zeta,
                                                                         const uint64_t* __restrict__ gamma, uint32_t n_queries,
                                                                         uint32_t* __restrict__ ok) {
  __shared__ uint64_t gpw[2 * (S::CONSTRAINTS + 1)];
  const gl2 g = {gamma[0], gamma[1]};
  air_gamma_powers(g, S::CONSTRAINTS, gpw);
  __syncthreads();
  gl2 zn = {zeta[0], zeta[1]}, pv[S::PLANES];
  for (uint32_t k = 0; k < log_sub; k++) zn = gl2_mul(zn, zn);
  const bool fine = air_sha512_periodic_at<S>(part, n_parts, zn, n_inv, pv);
  gl2 sum = {0, 0};
  for (uint32_t p = threadIdx.x; p < n_proofs; p += AIR_CHECK_THREADS) {
    ZetaView at = {open_t + (uint64_t)p * AIR_SHA512_WIDTH, open_h + (uint64_t)p * S::HELPER_COLS, 1ull << log_r_t, 1ull << log_r_h, gpw};
    const gl2 v = S::template proof<FieldP2>(at, pv);
    sum = gl2_add(sum, gl2_mul(gl2_pow(g, (uint64_t)S::CONSTRAINTS * p), v));
  }
  air_check_verdict(sum, open_q, {gl_sub(zn.c0, 1), zn.c1}, n_queries, ok);
  if (!fine)
    for (uint32_t q = threadIdx.x; q < n_queries; q += AIR_CHECK_THREADS) ok[q] = 0;
}

template <class S>
static int launch_sha512_periodic(uint32_t log_rows, void* d_pre, void* stream) {
  hipLaunchKernelGGL(k_air_sha512_periodic<S>, dim3(((1u << log_rows) + 255) / 256), dim3(256), 0, S_(stream), log_rows,
                     reinterpret_cast<uint64_t*>(d_pre));
  return (int)hipGetLastError();
}
template <class S>
static int launch_sha512_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, const void* d_gamma, void* d_tab, void* stream) {
  // (one workgroup per 256 of the CONSTRAINTS + 2 gamma powers; 2^log_blowup <= 64 inverses)
  hipLaunchKernelGGL(k_air_sha512_tables<S>, dim3((S::CONSTRAINTS + 2 + 255) / 256), dim3(256), 0, S_(stream), log_blowup, first_proof, s_n, w_n,
                     reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<uint64_t*>(d_tab));
  return (int)hipGetLastError();
}
template <class S>
static int launch_sha512_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_helper_cols,
                                  const void* d_pre, const void* d_tab, int form, void* d_quot, void* stream) {
  const dim3 grid((uint32_t)(((1ull << log_m) + AIR_THREADS - 1) / AIR_THREADS)), block(AIR_THREADS);
  const uint64_t* cols = reinterpret_cast<const uint64_t*>(d_cols);
  const uint64_t* hcols = reinterpret_cast<const uint64_t*>(d_helper_cols);
  const uint64_t* pre = reinterpret_cast<const uint64_t*>(d_pre);
  const uint64_t* tab = reinterpret_cast<const uint64_t*>(d_tab);
  uint64_t* out = reinterpret_cast<uint64_t*>(d_quot);
  if (form == AIR_FORM_WHOLE)
    hipLaunchKernelGGL((k_air_sha512_quotient<S, AIR_FORM_WHOLE>), grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, hcols, pre, tab, out);
  else if (form == AIR_FORM_PIECE)
    hipLaunchKernelGGL((k_air_sha512_quotient<S, AIR_FORM_PIECE>), grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, hcols, pre, tab, out);
  else
    hipLaunchKernelGGL((k_air_sha512_quotient<S, AIR_FORM_PIECE_ACC>), grid, block, 0, S_(stream), log_m, log_blowup, n_proofs, cols, hcols, pre, tab,
                       out);
  return (int)hipGetLastError();
}
template <class S>
static int launch_sha512_periodic_eval(uint32_t log_rows, uint64_t om, const void* d_zeta, void* d_part, void* stream) {
  hipLaunchKernelGGL(k_air_sha512_periodic_eval<S>, dim3(air_sha512_eval_parts(log_rows)), dim3(AIR_CHECK_THREADS), 0, S_(stream), log_rows, om,
                     reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<uint64_t*>(d_part));
  return (int)hipGetLastError();
}
template <class S>
static int launch_sha512_periodic_fold(uint32_t log_rows, uint64_t n_inv, const void* d_part, const void* d_zeta, void* d_out, void* stream) {
  hipLaunchKernelGGL(k_air_sha512_periodic_fold<S>, dim3(1), dim3(1), 0, S_(stream), log_rows, air_sha512_eval_parts(log_rows), n_inv,
                     reinterpret_cast<const uint64_t*>(d_part), reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<uint64_t*>(d_out));
  return (int)hipGetLastError();
}
template <class S>
static int launch_sha512_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint64_t n_inv, const void* d_part,
                               const void* d_open_t, const void* d_open_h, const void* d_open_q, const void* d_zeta, const void* d_gamma,
                               uint32_t n_queries, void* d_ok, void* stream) {
  hipLaunchKernelGGL(k_air_sha512_check<S>, dim3(1), dim3(AIR_CHECK_THREADS), 0, S_(stream), n_proofs, log_r_t, log_r_h, log_sub,
                     air_sha512_eval_parts(log_sub), n_inv, reinterpret_cast<const uint64_t*>(d_part), reinterpret_cast<const uint64_t*>(d_open_t),
                     reinterpret_cast<const uint64_t*>(d_open_h), reinterpret_cast<const uint64_t*>(d_open_q),
                     reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<const uint64_t*>(d_gamma), n_queries,
                     reinterpret_cast<uint32_t*>(d_ok));
  return (int)hipGetLastError();
}
// (internal, and handed out by a host function: a table of host functions must not be a constant the device pass emits too)
template <class S>
static constexpr AirSha512Launch AIR_SHA512_LAUNCH_OF = {launch_sha512_periodic<S>,      launch_sha512_tables<S>,        launch_sha512_quotient<S>,
                                                         launch_sha512_periodic_eval<S>, launch_sha512_periodic_fold<S>, launch_sha512_check<S>};
const AirSha512Launch* air_sha512_launch(uint32_t set) {
  return set == 7    ? &AIR_SHA512_LAUNCH_OF<Sha512Round>
         : set == 8  ? &AIR_SHA512_LAUNCH_OF<Sha512Sched>
         : set == 10 ? &AIR_SHA512_LAUNCH_OF<Sha512Link>
                     : &AIR_SHA512_LAUNCH_OF<Sha512Init>;
}

// The three helper oracles: one lane per (proof, row)
template <class Kernel>
static int launch_sha512_helper(Kernel k, uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream) {
  const uint64_t n = (uint64_t)n_proofs << log_rows;
  hipLaunchKernelGGL(k, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S_(stream), log_rows, n_proofs, reinterpret_cast<const uint64_t*>(d_table),
                     reinterpret_cast<uint64_t*>(d_helper));
  return (int)hipGetLastError();
}
int launch_air_sha512_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream) {
  return launch_sha512_helper(k_air_sha512_helper, log_rows, n_proofs, d_table, d_helper, stream);
}
int launch_air_sha512_sched_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream) {
  return launch_sha512_helper(k_air_sha512_sched_helper, log_rows, n_proofs, d_table, d_helper, stream);
}
int launch_air_sha512_init_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream) {
  return launch_sha512_helper(k_air_sha512_init_helper, log_rows, n_proofs, d_table, d_helper, stream);
}

// ---- constraint set 10: the SHA-512 table's link to Level-1 (include/tmx.h "the SHA-512 table's link to Level-1") ----------------------------
// The public table and the helper oracle; sets 7 - 9 above stay as they are.

// plonky2x DUMMY_PUBLIC_KEY and the R half of DUMMY_SIGNATURE, little-endian words (trace.hip and kernels.hip have the same words; pinned
// by tests/test_oracle_kat.py::test_dummy_constants and, here, by the gather test on a lane that did not sign)
__device__ __constant__ const uint32_t LINK512_DUMMY_PK[8] = {0xdde3888au, 0x95f10974u, 0x2ddb52fdu, 0x725dba3cu, 0xbf0967cau, 0x1b12941du, 0x018874f3u, 0x5c6f0fb4u};
__device__ __constant__ const uint32_t LINK512_DUMMY_R[8] = {0x9e681437u, 0x11c27854u, 0xa49ded06u, 0x899e5855u, 0xf0bb77bbu, 0x3f50499fu, 0x5b4aa285u, 0x8a063530u};

// Byte `pos` of the padded message R | A | M of a lane (v: its ValidatorVariable): `total` message bytes, 80, zeros, the bit length at the
// end of the last block (8 total < 2^16: the other fourteen length bytes are zero).  A lane that did not sign hashes the dummy triple.
__device__ __forceinline__ uint32_t link512_padded_byte(const AirSha512PublicGeom& G, const uint64_t* __restrict__ v, bool is_signed, uint32_t total,
                                                        uint32_t n_blocks, uint32_t pos) {
  if (pos >= total) {
    if (pos == total) return 0x80u;
    const uint32_t tail = 128u * n_blocks - 1u - pos;
    return tail < 2u ? ((8u * total) >> (8u * tail)) & 0xffu : 0u;
  }
  if (pos < 32u) return is_signed ? link_byte(v + G.h2_r + 8u * pos) : (LINK512_DUMMY_R[pos >> 2] >> (8u * (pos & 3u))) & 0xffu;
  if (pos < 64u) return is_signed ? link_byte(v + G.h2_pk + 8u * (pos - 32u)) : (LINK512_DUMMY_PK[(pos - 32u) >> 2] >> (8u * (pos & 3u))) & 0xffu;
  return is_signed ? link_byte(v + G.h2_msg + 8u * (pos - 64u)) : 0u;
}

// One lane per (proof, block slot k): lane i = k / 2 of the validators, block b = k mod 2 of its hash.  The sixteen message words of the
// block, the digest where the block is the last live one of its lane, and lv, from H.2 and D.1a of the proof's element row alone, by the
// rules of k_trace_sha512 (trace.hip): the dummy triple for a lane that did not sign, the message length clamped to 124.  Slots of lanes
// >= n -- the partial last slot and the padding are among them -- and unused second blocks are all zero.  Lanes run over the slots, so each
// of the 49 stores of a wave covers consecutive words of one column.
__global__ __launch_bounds__(256) void k_air_sha512_public_gather(const uint64_t* __restrict__ rows, AirSha512PublicGeom G, uint32_t log_k,
                                                                  uint32_t n_proofs, uint64_t* __restrict__ pub) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((uint64_t)n_proofs << log_k)) return;
  const uint32_t p = (uint32_t)(idx >> log_k), k = (uint32_t)(idx & ((1u << log_k) - 1));
  const uint64_t* __restrict__ row = rows + (uint64_t)p * G.elem_stride;
  const uint32_t i = k >> 1, b = k & 1u;
  const bool inside = i < G.n;
  const uint64_t* __restrict__ v = row + G.h2 + (uint64_t)G.h2_lane * (inside ? i : 0u);
  const uint64_t* __restrict__ dig = row + G.d1a + (uint64_t)G.d1a_lane * (inside ? i : 0u) + G.d1a_digest;
  const bool is_signed = (uint32_t)v[G.h2_signed] != 0;
  const uint64_t len = v[G.h2_mlen];
  const uint32_t total = 64u + (is_signed ? (len > 124u ? 124u : (uint32_t)len) : 32u), n_blocks = total + 17u > 128u ? 2u : 1u;
  const bool live = inside && b < n_blocks, last = live && b + 1u == n_blocks;
  uint64_t* __restrict__ dst = pub + (((uint64_t)p * AIR_SHA512_PUBLIC_WIDTH) << log_k) + k;
#pragma unroll 1
  for (uint32_t t = 0; t < 32; t++) {  // limb t & 1 of word t / 2: the low limb is the word's last four bytes
    uint32_t limb = 0;
    if (live) {
#pragma unroll 1
      for (uint32_t c = 0; c < 4; c++) limb = (limb << 8) | link512_padded_byte(G, v, is_signed, total, n_blocks, 128u * b + 4u * (t ^ 1u) + c);
    }
    dst[(uint64_t)(U_W + t) << log_k] = limb;
  }
#pragma unroll 1
  for (uint32_t t = 0; t < 16; t++) {
    uint32_t limb = 0;
    if (last) {
#pragma unroll
      for (uint32_t c = 0; c < 4; c++) limb = (limb << 8) | link_byte(dig + 8u * (4u * (t ^ 1u) + c));
    }
    dst[(uint64_t)(U_DIG + t) << log_k] = limb;
  }
  dst[(uint64_t)U_LV << log_k] = live ? 1 : 0;
}

// One lane per (proof, row) of the pre-LDE table: the row's eight state words, lv of its slot and of the next one (the slot of the next
// row, cyclic inside the proof: behind the partial last slot stands slot 0), and in a second block the eight state words of the row in
// front of it; then 65 stores, each of them consecutive words of one column across the wave.  CV, the state a block starts from, is the
// IV in a live first block, the first block's feed-forward in a live second block and 0 in a block that is not live; DG = CV + s mod 2^64
// with its two carry bits; LN and CH = LN DG.  Operands are the low 32 bits of the words; lv is set when its low 32 bits are not zero.
__global__ __launch_bounds__(256) void k_air_sha512_link_helper(uint32_t log_rows, uint32_t log_k, uint32_t n_proofs, const uint64_t* __restrict__ table,
                                                                const uint64_t* __restrict__ pub, uint64_t* __restrict__ helper) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((uint64_t)n_proofs << log_rows)) return;
  const uint32_t p = (uint32_t)(idx >> log_rows), N = 1u << log_rows;
  const uint32_t r = (uint32_t)(idx & (N - 1)), k = r / SHA512_BLOCK, kn = SHA512_BLOCK * (k + 1) < N ? k + 1 : 0;
  const uint64_t* __restrict__ t = table + (((uint64_t)p * AIR_SHA512_WIDTH) << log_rows);
  const uint64_t* __restrict__ lv = pub + (((uint64_t)p * AIR_SHA512_PUBLIC_WIDTH + U_LV) << log_k);
  const bool live = (uint32_t)lv[k] != 0, second = k & 1u, live_front = second && (uint32_t)lv[k - 1] != 0;
  const uint64_t ln = (uint32_t)lv[kn] != 0 ? 1 : 0;
  const uint32_t front = second ? SHA512_BLOCK * k - 1 : r;  // (the last row of the first block)
  uint64_t* __restrict__ o = helper + (((uint64_t)p * AIR_SHA512_LINK_HELPER_COLS) << log_rows) + r;
  auto put = [&](uint32_t col, uint64_t x) { o[(uint64_t)col << log_rows] = x; };
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    const uint64_t* __restrict__ lo_col = t + ((uint64_t)(R_A + 2 * j) << log_rows);
    const uint64_t* __restrict__ hi_col = t + ((uint64_t)(R_A + 2 * j + 1) << log_rows);
    uint64_t cv = 0;
    if (live) cv = second ? (live_front ? IV_SHA512[j] : 0) + ((uint64_t)(uint32_t)lo_col[front] | (uint64_t)(uint32_t)hi_col[front] << 32) : IV_SHA512[j];
    const uint64_t lo = limb_of(cv, 0) + (uint32_t)lo_col[r], cdl = lo >> 32;
    const uint64_t hi = limb_of(cv, 1) + (uint32_t)hi_col[r] + cdl, cdh = hi >> 32;
    put(L_CV + 2 * j, limb_of(cv, 0));
    put(L_CV + 2 * j + 1, limb_of(cv, 1));
    put(L_DG + 2 * j, (uint32_t)lo);
    put(L_DG + 2 * j + 1, (uint32_t)hi);
    put(L_CD + 2 * j, cdl);
    put(L_CD + 2 * j + 1, cdh);
    put(L_CH + 2 * j, ln ? (uint32_t)lo : 0u);
    put(L_CH + 2 * j + 1, ln ? (uint32_t)hi : 0u);
  }
  put(L_LN, ln);
}

// The public side under gamma, one lane per row r: V_r = sum_p gamma^(115 p) sum_j gamma^j (the public term of constraint j of proof p on
// row r), Horner over the proofs from the last to the first.  The public terms: lv of the next slot where STA or CHN is on (JL_LVN), dig
// of the row's slot on the last row of a block (JL_DIG ..), w[k][t] on row 80 k + t, t < 16 (JL_MSG, + 1); most rows have none.  v: two
// planes of N canonical words.
__global__ __launch_bounds__(256) void k_air_sha512_link_combine(uint32_t log_rows, uint32_t log_k, uint32_t n_proofs, const uint64_t* __restrict__ pub,
                                                                 const uint64_t* __restrict__ gamma, uint64_t* __restrict__ v) {
  const uint32_t N = 1u << log_rows, r = blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  const uint32_t k = r / SHA512_BLOCK, t = r % SHA512_BLOCK, kn = SHA512_BLOCK * (k + 1) < N ? k + 1 : 0;
  const bool edge = sha512_sta(r, N) || sha512_chn(r), e79 = t == SHA512_BLOCK - 1, msg = t < 16;
  gl2 acc = {0, 0};
  if (edge || e79 || msg) {
    const gl2 g = {gamma[0], gamma[1]};
    const gl2 g_lvn = gl2_pow(g, JL_LVN), g_msg = gl2_pow(g, JL_MSG), g_all = gl2_pow(g, AIR_SHA512_LINK_CONSTRAINTS);
    for (uint32_t p = n_proofs; p-- > 0;) {
      const uint64_t* __restrict__ u = pub + (((uint64_t)p * AIR_SHA512_PUBLIC_WIDTH) << log_k);
      gl2 s = {0, 0};
      if (edge) s = gl2_scale(g_lvn, gl_canon(u[((uint64_t)U_LV << log_k) + kn]));
      if (e79) {
        gl2 w = gl2_mul(g_lvn, g);  // gamma^JL_DIG
#pragma unroll 1
        for (uint32_t c = 0; c < 16; c++, w = gl2_mul(w, g)) s = gl2_add(s, gl2_scale(w, gl_canon(u[((uint64_t)(U_DIG + c) << log_k) + k])));
      }
      if (msg) {
        s = gl2_add(s, gl2_scale(g_msg, gl_canon(u[((uint64_t)(U_W + 2 * t) << log_k) + k])));
        s = gl2_add(s, gl2_scale(gl2_mul(g_msg, g), gl_canon(u[((uint64_t)(U_W + 2 * t + 1) << log_k) + k])));
      }
      acc = gl2_add(gl2_mul(acc, g_all), s);
    }
  }
  v[r] = acc.c0;
  v[(size_t)N + r] = acc.c1;
}

// One lane per point: quot -= Pub_gamma / (x^N - 1), both planes; ext the extended V (2 << log_m words), zinv the quotient tables' (by i mod B)
__global__ __launch_bounds__(256) void k_air_sha512_link_public_sub(uint32_t log_m, uint32_t log_blowup, const uint64_t* __restrict__ ext,
                                                                    const uint64_t* __restrict__ zinv, uint64_t* __restrict__ quot) {
  const uint64_t M = 1ull << log_m, i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const uint64_t z = zinv[i & ((1ull << log_blowup) - 1)];
  quot[i] = gl_sub(gl_canon(quot[i]), gl_mul(gl_canon(ext[i]), z));
  quot[M + i] = gl_sub(gl_canon(quot[M + i]), gl_mul(gl_canon(ext[M + i]), z));
}

// Pub_gamma at zeta, barycentric over the N rows from the verifier's own V: k_air_sha512_periodic_eval's walk with ONE F_p^2 value per
// row, read from v.  A workgroup's sum goes to its row of `part`: two words of sum, then 1 if a denominator was zero.
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_sha512_link_public_eval(uint32_t log_rows, uint64_t om, const uint64_t* __restrict__ zeta,
                                                                                   const uint64_t* __restrict__ v, uint64_t* __restrict__ part) {
  __shared__ uint64_t red[2][AIR_CHECK_THREADS];
  __shared__ uint32_t bad;
  const uint32_t N = 1u << log_rows, T = gridDim.x * AIR_CHECK_THREADS, g = blockIdx.x * AIR_CHECK_THREADS + threadIdx.x;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const gl2 z = {gl_canon(zeta[0]), gl_canon(zeta[1])};
  const uint64_t stride = gl_pow(om, T);
  uint64_t y = gl_pow(om, g);
  gl2 sum = {0, 0};
  for (uint32_t r0 = g; r0 < N; r0 += AIR_SHA512_EVAL_PER * T) {
    gl2 pre[AIR_SHA512_EVAL_PER], den[AIR_SHA512_EVAL_PER];
    uint64_t yk[AIR_SHA512_EVAL_PER];
    gl2 run = {1, 0};
#pragma unroll
    for (int m = 0; m < AIR_SHA512_EVAL_PER; m++) {
      const bool in = r0 + m * T < N;
      yk[m] = y;
      den[m] = {gl_sub(z.c0, y), z.c1};
      pre[m] = run;
      if (in && den[m].c0 == 0 && den[m].c1 == 0) {
        bad = 1;
        den[m] = {1, 0};
      }
      if (in) run = gl2_mul(run, den[m]);
      y = gl_mul(y, stride);
    }
    gl2 inv = gl2_inv(run);
#pragma unroll
    for (int m = AIR_SHA512_EVAL_PER - 1; m >= 0; m--) {
      const uint32_t r = r0 + m * T;
      if (r < N) {
        const gl2 term = gl2_scale(gl2_mul(inv, pre[m]), yk[m]);  // omega^r / (zeta - omega^r)
        inv = gl2_mul(inv, den[m]);
        if (gl_sub(z.c0, yk[m]) == 0 && z.c1 == 0) continue;
        sum = gl2_add(sum, gl2_mul(term, {gl_canon(v[r]), gl_canon(v[(size_t)N + r])}));
      }
    }
  }
  const uint32_t t = threadIdx.x;
  red[0][t] = sum.c0, red[1][t] = sum.c1;
  for (uint32_t h = AIR_CHECK_THREADS / 2; h; h >>= 1) {
    __syncthreads();
    if (t < h) red[0][t] = gl_add(red[0][t], red[0][t + h]), red[1][t] = gl_add(red[1][t], red[1][t + h]);
  }
  __syncthreads();
  if (t < 2) part[(size_t)blockIdx.x * AIR10_PUB_PART_WORDS + t] = red[t][0];
  if (t == 2) part[(size_t)blockIdx.x * AIR10_PUB_PART_WORDS + 2] = bad;
}

// The set-10 identity at zeta, one workgroup: k_air_sha512_check over Sha512Link with the public side -- the sum over the proofs less
// Pub_gamma(zeta), folded from the rows of pub_part, against (u_0 + X u_1) (zeta^N - 1).  A zero denominator in either barycentric sum
// clears every verdict.
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_sha512_link_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub,
                                                                             uint32_t n_parts, uint64_t n_inv, const uint64_t* __restrict__ part,
                                                                             const uint64_t* __restrict__ pub_part, const uint64_t* __restrict__ open_t,
                                                                             const uint64_t* __restrict__ open_h, const uint64_t* __restrict__ open_q,
                                                                             const uint64_t* __restrict__ zeta, const uint64_t* __restrict__ gamma,
                                                                             uint32_t n_queries, uint32_t* __restrict__ ok) {
  using S = Sha512Link;
  __shared__ uint64_t gpw[2 * (S::CONSTRAINTS + 1)];
  const gl2 g = {gamma[0], gamma[1]};
  air_gamma_powers(g, S::CONSTRAINTS, gpw);
  __syncthreads();
  gl2 zn = {zeta[0], zeta[1]}, pv[S::PLANES];
  for (uint32_t k = 0; k < log_sub; k++) zn = gl2_mul(zn, zn);
  bool fine = air_sha512_periodic_at<S>(part, n_parts, zn, n_inv, pv);
  gl2 sum = {0, 0};
  for (uint32_t p = threadIdx.x; p < n_proofs; p += AIR_CHECK_THREADS) {
    ZetaView at = {open_t + (uint64_t)p * AIR_SHA512_WIDTH, open_h + (uint64_t)p * S::HELPER_COLS, 1ull << log_r_t, 1ull << log_r_h, gpw};
    const gl2 v = S::template proof<FieldP2>(at, pv);
    sum = gl2_add(sum, gl2_mul(gl2_pow(g, (uint64_t)S::CONSTRAINTS * p), v));
  }
  gl2 ps = {0, 0};
  for (uint32_t k = 0; k < n_parts; k++) {
    ps = gl2_add(ps, {pub_part[(size_t)k * AIR10_PUB_PART_WORDS], pub_part[(size_t)k * AIR10_PUB_PART_WORDS + 1]});
    if (pub_part[(size_t)k * AIR10_PUB_PART_WORDS + 2]) fine = false;
  }
  if (threadIdx.x == 0) sum = gl2_sub(sum, gl2_mul(gl2_scale({gl_sub(zn.c0, 1), zn.c1}, n_inv), ps));
  air_check_verdict(sum, open_q, {gl_sub(zn.c0, 1), zn.c1}, n_queries, ok);
  if (!fine)
    for (uint32_t q = threadIdx.x; q < n_queries; q += AIR_CHECK_THREADS) ok[q] = 0;
}

// One thread: Pub_gamma(zeta) from the rows of `part` (2 words), then 1 if a denominator was zero, at out[0 .. 2]
__global__ void k_air_sha512_link_public_fold(uint32_t log_rows, uint32_t n_parts, uint64_t n_inv, const uint64_t* __restrict__ part,
                                              const uint64_t* __restrict__ zeta, uint64_t* __restrict__ out) {
  gl2 zn = {gl_canon(zeta[0]), gl_canon(zeta[1])}, ps = {0, 0};
  for (uint32_t k = 0; k < log_rows; k++) zn = gl2_mul(zn, zn);
  uint64_t bad = 0;
  for (uint32_t k = 0; k < n_parts; k++) {
    ps = gl2_add(ps, {part[(size_t)k * AIR10_PUB_PART_WORDS], part[(size_t)k * AIR10_PUB_PART_WORDS + 1]});
    bad |= part[(size_t)k * AIR10_PUB_PART_WORDS + 2];
  }
  const gl2 v = gl2_mul(gl2_scale({gl_sub(zn.c0, 1), zn.c1}, n_inv), ps);
  out[0] = v.c0;
  out[1] = v.c1;
  out[2] = bad ? 1 : 0;
}

int launch_air_sha512_link_public_fold(uint32_t log_rows, uint64_t n_inv, const void* d_part, const void* d_zeta, void* d_out, void* stream) {
  hipLaunchKernelGGL(k_air_sha512_link_public_fold, dim3(1), dim3(1), 0, S_(stream), log_rows, air_sha512_eval_parts(log_rows), n_inv,
                     reinterpret_cast<const uint64_t*>(d_part), reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<uint64_t*>(d_out));
  return (int)hipGetLastError();
}
int launch_air_sha512_link_combine(uint32_t log_rows, uint32_t n_proofs, const void* d_pub, const void* d_gamma, void* d_v, void* stream) {
  hipLaunchKernelGGL(k_air_sha512_link_combine, dim3(((1u << log_rows) + 255) / 256), dim3(256), 0, S_(stream), log_rows,
                     air_sha512_public_log_k(log_rows), n_proofs, reinterpret_cast<const uint64_t*>(d_pub), reinterpret_cast<const uint64_t*>(d_gamma),
                     reinterpret_cast<uint64_t*>(d_v));
  return (int)hipGetLastError();
}
int launch_air_sha512_link_public_sub(uint32_t log_m, uint32_t log_blowup, const void* d_ext, const void* d_tab, void* d_quot, void* stream) {
  hipLaunchKernelGGL(k_air_sha512_link_public_sub, dim3((uint32_t)(((1ull << log_m) + 255) / 256)), dim3(256), 0, S_(stream), log_m, log_blowup,
                     reinterpret_cast<const uint64_t*>(d_ext), reinterpret_cast<const uint64_t*>(d_tab) + AIR10_TAB_ZINV,
                     reinterpret_cast<uint64_t*>(d_quot));
  return (int)hipGetLastError();
}
int launch_air_sha512_link_public_eval(uint32_t log_rows, uint64_t om, const void* d_zeta, const void* d_v, void* d_part, void* stream) {
  hipLaunchKernelGGL(k_air_sha512_link_public_eval, dim3(air_sha512_eval_parts(log_rows)), dim3(AIR_CHECK_THREADS), 0, S_(stream), log_rows, om,
                     reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<const uint64_t*>(d_v), reinterpret_cast<uint64_t*>(d_part));
  return (int)hipGetLastError();
}
int launch_air_sha512_link_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint64_t n_inv, const void* d_part,
                                 const void* d_pub_part, const void* d_open_t, const void* d_open_h, const void* d_open_q, const void* d_zeta,
                                 const void* d_gamma, uint32_t n_queries, void* d_ok, void* stream) {
  hipLaunchKernelGGL(k_air_sha512_link_check, dim3(1), dim3(AIR_CHECK_THREADS), 0, S_(stream), n_proofs, log_r_t, log_r_h, log_sub,
                     air_sha512_eval_parts(log_sub), n_inv, reinterpret_cast<const uint64_t*>(d_part), reinterpret_cast<const uint64_t*>(d_pub_part),
                     reinterpret_cast<const uint64_t*>(d_open_t), reinterpret_cast<const uint64_t*>(d_open_h),
                     reinterpret_cast<const uint64_t*>(d_open_q), reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<const uint64_t*>(d_gamma),
                     n_queries, reinterpret_cast<uint32_t*>(d_ok));
  return (int)hipGetLastError();
}
int launch_air_sha512_public_gather(const void* d_rows, const AirSha512PublicGeom& G, uint32_t log_k, uint32_t n_proofs, void* d_pub, void* stream) {
  const uint64_t n = (uint64_t)n_proofs << log_k;
  hipLaunchKernelGGL(k_air_sha512_public_gather, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S_(stream), reinterpret_cast<const uint64_t*>(d_rows),
                     G, log_k, n_proofs, reinterpret_cast<uint64_t*>(d_pub));
  return (int)hipGetLastError();
}
int launch_air_sha512_link_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, const void* d_pub, void* d_helper, void* stream) {
  const uint64_t n = (uint64_t)n_proofs << log_rows;
  hipLaunchKernelGGL(k_air_sha512_link_helper, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S_(stream), log_rows, air_sha512_public_log_k(log_rows),
                     n_proofs, reinterpret_cast<const uint64_t*>(d_table), reinterpret_cast<const uint64_t*>(d_pub),
                     reinterpret_cast<uint64_t*>(d_helper));
  return (int)hipGetLastError();
}

}  // namespace tmx
