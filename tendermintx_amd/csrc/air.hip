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
  __shared__ uint64_t red[6][AIR_CHECK_THREADS];
  __shared__ uint32_t holds;
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
  red[0][t] = sum.c0;
  red[1][t] = sum.c1;
  red[2][t] = bsum.c0;
  red[3][t] = bsum.c1;
  red[4][t] = psum.c0;
  red[5][t] = psum.c1;
  for (uint32_t h = AIR_CHECK_THREADS / 2; h; h >>= 1) {
    __syncthreads();
    if (t < h)
      for (uint32_t r = 0; r < 6; r++) red[r][t] = gl_add(red[r][t], red[r][t + h]);
  }
  __syncthreads();
  if (t == 0) {
    gl2 zn = zp;  // zeta^N = (zeta^(N/256))^256
    for (uint32_t k = 0; k < 8; k++) zn = gl2_mul(zn, zn);
    const gl2 Z = {gl_sub(zn.c0, 1), zn.c1};
    const gl2 pub = gl2_mul(gl2_scale(S, bary_inv), {red[4][0], red[5][0]});
    const gl2 lhs = gl2_add(gl2_mul(S, {red[0][0], red[1][0]}), gl2_mul(Z, gl2_sub({red[2][0], red[3][0]}, pub)));
    const gl2 u0 = {gl_canon(open_q[0]), gl_canon(open_q[2])}, u1 = {gl_canon(open_q[1]), gl_canon(open_q[3])};
    const gl2 q = {gl_add(u0.c0, gl_mul(u1.c1, 7)), gl_add(u0.c1, u1.c0)};
    holds = gl2_eq(lhs, gl2_mul(q, gl2_mul(Z, S))) ? 1u : 0u;
  }
  __syncthreads();
  if (!holds)
    for (uint32_t q = t; q < n_queries; q += AIR_CHECK_THREADS) ok[q] = 0;
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

// ---- constraint set 3: the round constraints of the SHA-256 tables (include/tmx.h "the round constraints of the SHA-256 tables") ------------
// Siblings again: nothing above changes.  Helper column offsets inside a proof's 300, and the constraint indices inside its 315.
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
  auto rot = [](uint32_t x, uint32_t n) { return (x >> n) | (x << (32 - n)); };
  const uint32_t s0 = rot(a, 2) ^ rot(a, 13) ^ rot(a, 22), s1 = rot(e, 6) ^ rot(e, 11) ^ rot(e, 25);
  const uint32_t chv = (e & f) ^ (~e & g), mjv = (a & b) ^ (a & c) ^ (b & c);
  const uint32_t u0 = rot(a, 2) ^ rot(a, 13), u1 = rot(e, 6) ^ rot(e, 11), v = a & b;
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

// P_K, the polynomial of degree < 64 with P_K(omega_64^t) = K256[t], into LDS: thread j < 64 takes coefficient j, an inverse transform
// written out (64 terms; launch-sized work).  Every thread of the workgroup calls it; 64^-1 = p - (p - 1) / 64.
__device__ __forceinline__ void air_sha_pk(uint64_t om64_inv, uint64_t* pk) {
  if (threadIdx.x < 64) {
    const uint64_t step = gl_pow(om64_inv, threadIdx.x);
    uint64_t cur = 1, acc = 0;
    for (uint32_t t = 0; t < 64; t++, cur = gl_mul(cur, step)) acc = gl_add(acc, gl_mul(cur, K_SHA256[t]));
    pk[threadIdx.x] = gl_mul(acc, GL_P - (GL_P - 1) / 64);
  }
  __syncthreads();
}

// One thread per table entry: S and K by i mod 64 B (K by Horner on P_K's coefficients in LDS), 1 / (x^N - 1) by i mod B, gamma^0 .. 315.
__global__ __launch_bounds__(256) void k_air_sha_tables(uint32_t log_blowup, uint64_t s_n, uint64_t w_n, uint64_t s_n64, uint64_t w_n64,
                                                        uint64_t om64_inv, const uint64_t* __restrict__ gamma, uint64_t* __restrict__ tab) {
  __shared__ uint64_t pk[64];
  air_sha_pk(om64_inv, pk);
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < (64u << log_blowup)) {
    const uint64_t y = gl_mul(s_n64, gl_pow(w_n64, k));
    tab[AIR3_TAB_SEL + k] = gl_sub(y, om64_inv);
    uint64_t acc = 0;
    for (int j = 63; j >= 0; j--) acc = gl_add(gl_mul(acc, y), pk[j]);
    tab[AIR3_TAB_K + k] = acc;
  }
  if (k < (1u << log_blowup)) tab[AIR3_TAB_ZINV + k] = gl_pow(gl_sub(gl_mul(s_n, gl_pow(w_n, k)), 1), GL_P - 2);
  if (k <= AIR_SHA_CONSTRAINTS) {
    const gl2 g = gl2_pow({gamma[0], gamma[1]}, k);
    tab[AIR3_TAB_GPOW + 2 * k] = g.c0;
    tab[AIR3_TAB_GPOW + 2 * k + 1] = g.c1;
  }
}

// The set-3 hot pass, k_air_ladder_quotient's shape: one lane per point, a loop over the proofs from the last to the first (Horner by
// gamma^315), the nine table columns and the 300 helper columns read once from HBM.  On the coset a bit column is a full field element, so
// the pass never holds the 300 words: it walks the bit index b from 31 down to 0 and per b holds the nine bit words A_b .. V_b and the six
// rotated ones (A_(b+2), A_(b+13), A_(b+22), E_(b+6), E_(b+11), E_(b+25)), which are re-read through the cache (another b of the same lane
// reads them as its own).  Per b: nine constraints (six X^2 - X, U0, U1, V), and one Horner step by 2 of the ten word sums (a, b, c, e,
// f, g, Sigma0, Sigma1, Ch, Maj), so that no power of two is multiplied.  13 reduced column products and 18 gamma weights per b; behind
// the loop 8 more column products, the word constraints and the nine selected ones, whose S(x) is factored out of their gamma sum.
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
    const uint64_t* __restrict__ c = cols + (((uint64_t)p * AIR_SHA_WIDTH) << log_m);
    const uint64_t* __restrict__ h = hcols + (((uint64_t)p * AIR_SHA_HELPER_COLS) << log_m);
    auto once = [&](uint32_t col) { return gl_canon(__builtin_nontemporal_load(h + ((uint64_t)col << log_m) + i)); };
    auto again = [&](uint32_t col) { return gl_canon(h[((uint64_t)col << log_m) + i]); };
    auto tbl = [&](uint32_t col, uint64_t at) { return gl_canon(c[((uint64_t)col << log_m) + at]); };
    uint64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;  // the plain and the selected gamma sums, lazy
    auto plain = [&](uint32_t j, uint64_t v) {
      a0 = gl_add_lazy(a0, gl_mul(gp[2 * j], v));
      a1 = gl_add_lazy(a1, gl_mul(gp[2 * j + 1], v));
    };
    auto selected = [&](uint32_t j, uint64_t v) {
      b0 = gl_add_lazy(b0, gl_mul(gp[2 * j], v));
      b1 = gl_add_lazy(b1, gl_mul(gp[2 * j + 1], v));
    };
    auto boolean = [](uint64_t x) { return gl_sub(gl_mul(x, x), x); };
    auto exor = [](uint64_t x, uint64_t y) {  // x + y - 2 x y
      const uint64_t xy = gl_mul(x, y);
      return gl_sub(gl_add(x, y), gl_add(xy, xy));
    };
    auto dbl_add = [](uint64_t s, uint64_t x) { return gl_add(gl_add(s, s), x); };
    uint64_t wa = 0, wb = 0, wc = 0, we = 0, wf = 0, wg = 0, ws0 = 0, ws1 = 0, wch = 0, wmj = 0;
#pragma unroll 2
    for (uint32_t b = 32; b-- > 0;) {
      const uint64_t A = again(H_A + b), B = once(H_B + b), C = once(H_C + b), E = again(H_E + b), F = once(H_F + b), G = once(H_G + b);
      const uint64_t U0 = once(H_U0 + b), U1 = once(H_U1 + b), V = once(H_V + b);
      const uint64_t A2 = again(H_A + ((b + 2) & 31)), A13 = again(H_A + ((b + 13) & 31)), A22 = again(H_A + ((b + 22) & 31));
      const uint64_t E6 = again(H_E + ((b + 6) & 31)), E11 = again(H_E + ((b + 11) & 31)), E25 = again(H_E + ((b + 25) & 31));
      plain(H_A + b, boolean(A));
      plain(H_B + b, boolean(B));
      plain(H_C + b, boolean(C));
      plain(H_E + b, boolean(E));
      plain(H_F + b, boolean(F));
      plain(H_G + b, boolean(G));
      plain(J_U0 + b, gl_sub(U0, exor(A2, A13)));
      plain(J_U1 + b, gl_sub(U1, exor(E6, E11)));
      const uint64_t AB = gl_mul(A, B);
      plain(J_V + b, gl_sub(V, AB));
      wa = dbl_add(wa, A);
      wb = dbl_add(wb, B);
      wc = dbl_add(wc, C);
      we = dbl_add(we, E);
      wf = dbl_add(wf, F);
      wg = dbl_add(wg, G);
      ws0 = dbl_add(ws0, exor(U0, A22));
      ws1 = dbl_add(ws1, exor(U1, E25));
      wch = dbl_add(wch, gl_add(G, gl_mul(E, gl_sub(F, G))));
      wmj = dbl_add(wmj, gl_add(V, gl_mul(C, gl_sub(gl_add(A, B), gl_add(V, V)))));
    }
    const uint64_t ta = tbl(T_A, i), tb = tbl(T_B, i), tc = tbl(T_C, i), td = tbl(T_D, i), te = tbl(T_E, i), tf = tbl(T_F, i), tg = tbl(T_G, i),
                   th = tbl(T_H, i);
    plain(J_WORD + 0, gl_sub(ta, wa));
    plain(J_WORD + 1, gl_sub(tb, wb));
    plain(J_WORD + 2, gl_sub(tc, wc));
    plain(J_WORD + 3, gl_sub(te, we));
    plain(J_WORD + 4, gl_sub(tf, wf));
    plain(J_WORD + 5, gl_sub(tg, wg));
    const uint64_t S0 = once(H_S0), S1 = once(H_S1), CH = once(H_CH), MAJ = once(H_MAJ), LIVE = again(H_LIVE), KL = again(H_KL);
    plain(J_S0, gl_sub(S0, ws0));
    plain(J_S1, gl_sub(S1, ws1));
    plain(J_CH, gl_sub(CH, wch));
    plain(J_MAJ, gl_sub(MAJ, wmj));
    plain(J_LIVE, boolean(LIVE));
    plain(J_KL, gl_sub(KL, gl_mul(LIVE, kx)));
    uint64_t carry[6];
#pragma unroll
    for (uint32_t k = 0; k < 6; k++) {
      carry[k] = once(H_CA + k);
      plain(J_CARRY + k, boolean(carry[k]));
    }
    selected(J_SHIFT + 0, gl_sub(tbl(T_B, nx), ta));
    selected(J_SHIFT + 1, gl_sub(tbl(T_C, nx), tb));
    selected(J_SHIFT + 2, gl_sub(tbl(T_D, nx), tc));
    selected(J_SHIFT + 3, gl_sub(tbl(T_F, nx), te));
    selected(J_SHIFT + 4, gl_sub(tbl(T_G, nx), tf));
    selected(J_SHIFT + 5, gl_sub(tbl(T_H, nx), tg));
    selected(J_LIVEN, gl_sub(gl_canon(h[((uint64_t)H_LIVE << log_m) + nx]), LIVE));
    const uint64_t kln = gl_canon(h[((uint64_t)H_KL << log_m) + nx]);
    const uint64_t t1 = gl_add(gl_add(gl_add(th, S1), gl_add(CH, kln)), tbl(T_W, nx));
    auto c32 = [](uint64_t x0, uint64_t x1, uint64_t x2) { return gl_mul(gl_add(x0, gl_add(gl_add(x1, x1), gl_mul(x2, 4))), 1ull << 32); };
    selected(J_NA, gl_sub(gl_add(tbl(T_A, nx), c32(carry[0], carry[1], carry[2])), gl_add(t1, gl_add(S0, MAJ))));
    selected(J_NE, gl_sub(gl_add(tbl(T_E, nx), c32(carry[3], carry[4], carry[5])), gl_add(td, t1)));
    const gl2 v = {gl_add(gl_canon(a0), gl_mul(sel, b0)), gl_add(gl_canon(a1), gl_mul(sel, b1))};
    t = gl2_add(gl2_mul(t, g315), v);
  }
  const gl2 q = gl2_scale(t, zinv);
  out[i] = q.c0;
  out[M + i] = q.c1;
}

// The set-3 identity at zeta, one workgroup: gamma^0 .. gamma^315 and P_K go to LDS first; thread t takes the proofs t, t + 256, ... and
// evaluates their 315 constraints over F_p^2 from the table's and the helper's openings at zeta (y0) and zeta omega_N (y1) in the order of
// the hot pass; K(zeta) by Horner on P_K at zeta^(N/64).  The sums meet in LDS; thread 0 compares with (u_0 + X u_1) (zeta^N - 1).
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_sha_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub,
                                                                      uint64_t om64_inv, const uint64_t* __restrict__ open_t,
                                                                      const uint64_t* __restrict__ open_h, const uint64_t* __restrict__ open_q,
                                                                      const uint64_t* __restrict__ zeta, const uint64_t* __restrict__ gamma,
                                                                      uint32_t n_queries, uint32_t* __restrict__ ok) {
  __shared__ uint64_t red[2][AIR_CHECK_THREADS];
  __shared__ uint64_t gpw[2 * (AIR_SHA_CONSTRAINTS + 1)];
  __shared__ uint64_t pk[64];
  __shared__ uint32_t holds;
  const uint32_t t = threadIdx.x;
  const uint64_t RT = 1ull << log_r_t, RH = 1ull << log_r_h;
  const gl2 g = {gamma[0], gamma[1]}, z = {zeta[0], zeta[1]};
  for (uint32_t k = t; k <= AIR_SHA_CONSTRAINTS; k += AIR_CHECK_THREADS) {
    const gl2 gk = gl2_pow(g, k);
    gpw[2 * k] = gk.c0;
    gpw[2 * k + 1] = gk.c1;
  }
  air_sha_pk(om64_inv, pk);  // (ends with a barrier: gpw is complete behind it too)
  gl2 zp = z;  // zeta^(N/64)
  for (uint32_t k = 6; k < log_sub; k++) zp = gl2_mul(zp, zp);
  const gl2 S = {gl_sub(zp.c0, om64_inv), zp.c1};
  gl2 K = {0, 0};
  for (int j = 63; j >= 0; j--) {
    K = gl2_mul(K, zp);
    K.c0 = gl_add(K.c0, pk[j]);
  }
  auto t0 = [&](uint64_t c) -> gl2 { return {gl_canon(open_t[c]), gl_canon(open_t[RT + c])}; };
  auto t1 = [&](uint64_t c) -> gl2 { return {gl_canon(open_t[2 * RT + c]), gl_canon(open_t[3 * RT + c])}; };
  auto h0 = [&](uint64_t c) -> gl2 { return {gl_canon(open_h[c]), gl_canon(open_h[RH + c])}; };
  auto h1 = [&](uint64_t c) -> gl2 { return {gl_canon(open_h[2 * RH + c]), gl_canon(open_h[3 * RH + c])}; };
  auto boolean = [](gl2 x) { return gl2_sub(gl2_mul(x, x), x); };
  auto exor = [](gl2 x, gl2 y) {
    const gl2 xy = gl2_mul(x, y);
    return gl2_sub(gl2_add(x, y), gl2_add(xy, xy));
  };
  auto dbl_add = [](gl2 s, gl2 x) { return gl2_add(gl2_add(s, s), x); };
  gl2 sum = {0, 0};
  for (uint32_t p = t; p < n_proofs; p += AIR_CHECK_THREADS) {
    const uint64_t ct = (uint64_t)p * AIR_SHA_WIDTH, chh = (uint64_t)p * AIR_SHA_HELPER_COLS;
    gl2 a = {0, 0}, bsel = {0, 0};
    auto plain = [&](uint32_t j, gl2 v) { a = gl2_add(a, gl2_mul({gpw[2 * j], gpw[2 * j + 1]}, v)); };
    auto selected = [&](uint32_t j, gl2 v) { bsel = gl2_add(bsel, gl2_mul({gpw[2 * j], gpw[2 * j + 1]}, v)); };
    gl2 wa = {0, 0}, wb = wa, wc = wa, we = wa, wf = wa, wg = wa, ws0 = wa, ws1 = wa, wch = wa, wmj = wa;
    for (uint32_t b = 32; b-- > 0;) {
      const gl2 A = h0(chh + H_A + b), B = h0(chh + H_B + b), C = h0(chh + H_C + b), E = h0(chh + H_E + b), F = h0(chh + H_F + b),
                G = h0(chh + H_G + b), U0 = h0(chh + H_U0 + b), U1 = h0(chh + H_U1 + b), V = h0(chh + H_V + b);
      const gl2 A2 = h0(chh + H_A + ((b + 2) & 31)), A13 = h0(chh + H_A + ((b + 13) & 31)), A22 = h0(chh + H_A + ((b + 22) & 31));
      const gl2 E6 = h0(chh + H_E + ((b + 6) & 31)), E11 = h0(chh + H_E + ((b + 11) & 31)), E25 = h0(chh + H_E + ((b + 25) & 31));
      plain(H_A + b, boolean(A));
      plain(H_B + b, boolean(B));
      plain(H_C + b, boolean(C));
      plain(H_E + b, boolean(E));
      plain(H_F + b, boolean(F));
      plain(H_G + b, boolean(G));
      plain(J_U0 + b, gl2_sub(U0, exor(A2, A13)));
      plain(J_U1 + b, gl2_sub(U1, exor(E6, E11)));
      plain(J_V + b, gl2_sub(V, gl2_mul(A, B)));
      wa = dbl_add(wa, A);
      wb = dbl_add(wb, B);
      wc = dbl_add(wc, C);
      we = dbl_add(we, E);
      wf = dbl_add(wf, F);
      wg = dbl_add(wg, G);
      ws0 = dbl_add(ws0, exor(U0, A22));
      ws1 = dbl_add(ws1, exor(U1, E25));
      wch = dbl_add(wch, gl2_add(G, gl2_mul(E, gl2_sub(F, G))));
      wmj = dbl_add(wmj, gl2_add(V, gl2_mul(C, gl2_sub(gl2_add(A, B), gl2_add(V, V)))));
    }
    const gl2 ta = t0(ct + T_A), tb = t0(ct + T_B), tc = t0(ct + T_C), td = t0(ct + T_D), te = t0(ct + T_E), tf = t0(ct + T_F), tg = t0(ct + T_G),
              th = t0(ct + T_H);
    plain(J_WORD + 0, gl2_sub(ta, wa));
    plain(J_WORD + 1, gl2_sub(tb, wb));
    plain(J_WORD + 2, gl2_sub(tc, wc));
    plain(J_WORD + 3, gl2_sub(te, we));
    plain(J_WORD + 4, gl2_sub(tf, wf));
    plain(J_WORD + 5, gl2_sub(tg, wg));
    const gl2 S0 = h0(chh + H_S0), S1 = h0(chh + H_S1), CH = h0(chh + H_CH), MAJ = h0(chh + H_MAJ), LIVE = h0(chh + H_LIVE), KL = h0(chh + H_KL);
    plain(J_S0, gl2_sub(S0, ws0));
    plain(J_S1, gl2_sub(S1, ws1));
    plain(J_CH, gl2_sub(CH, wch));
    plain(J_MAJ, gl2_sub(MAJ, wmj));
    plain(J_LIVE, boolean(LIVE));
    plain(J_KL, gl2_sub(KL, gl2_mul(LIVE, K)));
    gl2 carry[6];
    for (uint32_t k = 0; k < 6; k++) {
      carry[k] = h0(chh + H_CA + k);
      plain(J_CARRY + k, boolean(carry[k]));
    }
    selected(J_SHIFT + 0, gl2_sub(t1(ct + T_B), ta));
    selected(J_SHIFT + 1, gl2_sub(t1(ct + T_C), tb));
    selected(J_SHIFT + 2, gl2_sub(t1(ct + T_D), tc));
    selected(J_SHIFT + 3, gl2_sub(t1(ct + T_F), te));
    selected(J_SHIFT + 4, gl2_sub(t1(ct + T_G), tf));
    selected(J_SHIFT + 5, gl2_sub(t1(ct + T_H), tg));
    selected(J_LIVEN, gl2_sub(h1(chh + H_LIVE), LIVE));
    const gl2 tt = gl2_add(gl2_add(gl2_add(th, S1), gl2_add(CH, h1(chh + H_KL))), t1(ct + T_W));
    auto c32 = [](gl2 x0, gl2 x1, gl2 x2) { return gl2_scale(gl2_add(x0, gl2_add(gl2_add(x1, x1), gl2_scale(x2, 4))), 1ull << 32); };
    selected(J_NA, gl2_sub(gl2_add(t1(ct + T_A), c32(carry[0], carry[1], carry[2])), gl2_add(tt, gl2_add(S0, MAJ))));
    selected(J_NE, gl2_sub(gl2_add(t1(ct + T_E), c32(carry[3], carry[4], carry[5])), gl2_add(td, tt)));
    sum = gl2_add(sum, gl2_mul(gl2_pow(g, (uint64_t)AIR_SHA_CONSTRAINTS * p), gl2_add(a, gl2_mul(S, bsel))));
  }
  red[0][t] = sum.c0;
  red[1][t] = sum.c1;
  for (uint32_t hh = AIR_CHECK_THREADS / 2; hh; hh >>= 1) {
    __syncthreads();
    if (t < hh) {
      red[0][t] = gl_add(red[0][t], red[0][t + hh]);
      red[1][t] = gl_add(red[1][t], red[1][t + hh]);
    }
  }
  __syncthreads();
  if (t == 0) {
    gl2 zn = zp;  // zeta^N = (zeta^(N/64))^64
    for (uint32_t k = 0; k < 6; k++) zn = gl2_mul(zn, zn);
    const gl2 u0 = {gl_canon(open_q[0]), gl_canon(open_q[2])}, u1 = {gl_canon(open_q[1]), gl_canon(open_q[3])};
    const gl2 q = {gl_add(u0.c0, gl_mul(u1.c1, 7)), gl_add(u0.c1, u1.c0)};
    holds = gl2_eq({red[0][0], red[1][0]}, gl2_mul(q, {gl_sub(zn.c0, 1), zn.c1})) ? 1u : 0u;
  }
  __syncthreads();
  if (!holds)
    for (uint32_t q = t; q < n_queries; q += AIR_CHECK_THREADS) ok[q] = 0;
}

int launch_air_sha_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream) {
  const uint64_t n = (uint64_t)n_proofs << log_rows;
  hipLaunchKernelGGL(k_air_sha_helper, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S_(stream), log_rows, n_proofs,
                     reinterpret_cast<const uint64_t*>(d_table), reinterpret_cast<uint64_t*>(d_helper));
  return (int)hipGetLastError();
}
int launch_air_sha_tables(uint32_t log_blowup, uint64_t s_n, uint64_t w_n, uint64_t s_n64, uint64_t w_n64, uint64_t om64_inv, const void* d_gamma,
                          void* d_tab, void* stream) {
  // (at least two workgroups: the 316 gamma powers)
  const uint32_t blocks = ((64u << log_blowup) + 255) / 256;
  hipLaunchKernelGGL(k_air_sha_tables, dim3(blocks < 2 ? 2 : blocks), dim3(256), 0, S_(stream), log_blowup, s_n, w_n, s_n64, w_n64, om64_inv,
                     reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<uint64_t*>(d_tab));
  return (int)hipGetLastError();
}
int launch_air_sha_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_helper_cols, const void* d_tab,
                            void* d_quot, void* stream) {
  hipLaunchKernelGGL(k_air_sha_quotient, dim3((uint32_t)(((1ull << log_m) + AIR_THREADS - 1) / AIR_THREADS)), dim3(AIR_THREADS), 0, S_(stream), log_m,
                     log_blowup, n_proofs, reinterpret_cast<const uint64_t*>(d_cols), reinterpret_cast<const uint64_t*>(d_helper_cols),
                     reinterpret_cast<const uint64_t*>(d_tab), reinterpret_cast<uint64_t*>(d_quot));
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
// Siblings again: nothing above changes.  Helper column offsets inside a proof's 115 (Q_k at S_Q + k), constraint indices inside its 117
// (Q_k's at JS_Q + k).
constexpr uint32_t S_WB = 0, S_X0 = 32, S_X1 = 64, S_G0 = 96, S_G1 = 97, S_Q = 97, S_CW = 113;
constexpr uint32_t JS_CW = 32, JS_WORD = 34, JS_X0 = 35, JS_X1 = 67, JS_G0 = 99, JS_G1 = 100, JS_Q = 100, JS_NEXT = 116;

__device__ __forceinline__ uint32_t sched_rot(uint32_t x, uint32_t n) { return (x >> n) | (x << (32 - n)); }
__device__ __forceinline__ uint32_t sched_s0(uint32_t w) { return sched_rot(w, 7) ^ sched_rot(w, 18) ^ (w >> 3); }
__device__ __forceinline__ uint32_t sched_s1(uint32_t w) { return sched_rot(w, 17) ^ sched_rot(w, 19) ^ (w >> 10); }

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
  const uint32_t w0 = w[0], x0 = sched_rot(w0, 7) ^ sched_rot(w0, 18), x1 = sched_rot(w0, 17) ^ sched_rot(w0, 19);
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

// P_F, the polynomial of degree < 64 with P_F(omega_64^t) = 1 for 15 <= t <= 62 and 0 otherwise (the next row is a schedule row), into
// LDS: thread j < 64 takes coefficient j, an inverse transform written out.  Every thread of the workgroup calls it.
__device__ __forceinline__ void air_sched_pf(uint64_t om64_inv, uint64_t* pf) {
  if (threadIdx.x < 64) {
    const uint64_t step = gl_pow(om64_inv, threadIdx.x);
    uint64_t cur = gl_pow(step, 15), acc = 0;
    for (uint32_t t = 15; t <= 62; t++, cur = gl_mul(cur, step)) acc = gl_add(acc, cur);
    pf[threadIdx.x] = gl_mul(acc, GL_P - (GL_P - 1) / 64);
  }
  __syncthreads();
}

// One thread per table entry: F by i mod 64 B (Horner on P_F's coefficients in LDS), 1 / (x^N - 1) by i mod B, gamma^0 .. 117.
__global__ __launch_bounds__(256) void k_air_sched_tables(uint32_t log_blowup, uint64_t s_n, uint64_t w_n, uint64_t s_n64, uint64_t w_n64,
                                                          uint64_t om64_inv, const uint64_t* __restrict__ gamma, uint64_t* __restrict__ tab) {
  __shared__ uint64_t pf[64];
  air_sched_pf(om64_inv, pf);
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < (64u << log_blowup)) {
    const uint64_t y = gl_mul(s_n64, gl_pow(w_n64, k));
    uint64_t acc = 0;
    for (int j = 63; j >= 0; j--) acc = gl_add(gl_mul(acc, y), pf[j]);
    tab[AIR4_TAB_F + k] = acc;
  }
  if (k < (1u << log_blowup)) tab[AIR4_TAB_ZINV + k] = gl_pow(gl_sub(gl_mul(s_n, gl_pow(w_n, k)), 1), GL_P - 2);
  if (k <= AIR_SCHED_CONSTRAINTS) {
    const gl2 g = gl2_pow({gamma[0], gamma[1]}, k);
    tab[AIR4_TAB_GPOW + 2 * k] = g.c0;
    tab[AIR4_TAB_GPOW + 2 * k + 1] = g.c1;
  }
}

// The set-4 hot pass, k_air_sha_quotient's shape: one lane per point, a loop over the proofs from the last to the first (Horner by
// gamma^117), W and the 115 helper columns.  It walks the bit index b from 31 down to 0 and per b holds WB_b, X0_b, X1_b and the six
// rotated or shifted bit words (WB_(b+7), WB_(b+18), WB_(b+17), WB_(b+19), and WB_(b+3) for b < 29, WB_(b+10) for b < 22), which are re-read
// through the cache.  Per b: three constraints (X^2 - X, X0, X1) and one Horner step by 2 of the three word sums (W, sigma0, sigma1), so
// that no power of two is multiplied: 5 reduced column products and 6 gamma weights.  Behind the loop the three word constraints, the two
// carry bits, the fifteen pipeline constraints (linear: W', G0', G1' and Q_1' .. Q_15' at i + B) and the selected one, whose F(x) is
// applied once to its value.  The gamma sums are lazy, as in set 3's pass.
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
    const uint64_t* __restrict__ c = cols + (((uint64_t)p * AIR_SHA_WIDTH) << log_m);  // (W is column 0)
    const uint64_t* __restrict__ h = hcols + (((uint64_t)p * AIR_SCHED_HELPER_COLS) << log_m);
    auto once = [&](uint32_t col) { return gl_canon(__builtin_nontemporal_load(h + ((uint64_t)col << log_m) + i)); };
    auto again = [&](uint32_t col) { return gl_canon(h[((uint64_t)col << log_m) + i]); };
    auto next = [&](uint32_t col) { return gl_canon(h[((uint64_t)col << log_m) + nx]); };
    uint64_t a0 = 0, a1 = 0;  // the gamma sums, lazy
    auto plain = [&](uint32_t j, uint64_t v) {
      a0 = gl_add_lazy(a0, gl_mul(gp[2 * j], v));
      a1 = gl_add_lazy(a1, gl_mul(gp[2 * j + 1], v));
    };
    auto boolean = [](uint64_t x) { return gl_sub(gl_mul(x, x), x); };
    auto exor = [](uint64_t x, uint64_t y) {  // x + y - 2 x y
      const uint64_t xy = gl_mul(x, y);
      return gl_sub(gl_add(x, y), gl_add(xy, xy));
    };
    auto dbl_add = [](uint64_t s, uint64_t x) { return gl_add(gl_add(s, s), x); };
    uint64_t ww = 0, wg0 = 0, wg1 = 0;
#pragma unroll 2
    for (uint32_t b = 32; b-- > 0;) {
      const uint64_t WB = again(S_WB + b), X0 = once(S_X0 + b), X1 = once(S_X1 + b);
      const uint64_t W7 = again(S_WB + ((b + 7) & 31)), W18 = again(S_WB + ((b + 18) & 31));
      const uint64_t W17 = again(S_WB + ((b + 17) & 31)), W19 = again(S_WB + ((b + 19) & 31));
      plain(S_WB + b, boolean(WB));
      plain(JS_X0 + b, gl_sub(X0, exor(W7, W18)));
      plain(JS_X1 + b, gl_sub(X1, exor(W17, W19)));
      ww = dbl_add(ww, WB);
      wg0 = dbl_add(wg0, b < 29 ? exor(X0, again(S_WB + ((b + 3) & 31))) : X0);   // (b is uniform: a scalar branch)
      wg1 = dbl_add(wg1, b < 22 ? exor(X1, again(S_WB + ((b + 10) & 31))) : X1);
    }
    const uint64_t W = gl_canon(c[i]), Wn = gl_canon(c[nx]);
    const uint64_t G0 = again(S_G0), G1 = again(S_G1), CW0 = once(S_CW), CW1 = once(S_CW + 1);
    plain(JS_WORD, gl_sub(W, ww));
    plain(JS_G0, gl_sub(G0, wg0));
    plain(JS_G1, gl_sub(G1, wg1));
    plain(JS_CW, boolean(CW0));
    plain(JS_CW + 1, boolean(CW1));
    uint64_t prev = gl_add(W, next(S_G0));  // what Q_k' must equal: W + G0' for k = 1, then Q_(k-1) (+ W' for k = 9, + G1' for k = 14)
#pragma unroll
    for (uint32_t k = 1; k <= 15; k++) {
      plain(JS_Q + k, gl_sub(next(S_Q + k), prev));
      prev = again(S_Q + k);
      if (k + 1 == 9) prev = gl_add(prev, Wn);
      if (k + 1 == 14) prev = gl_add(prev, next(S_G1));
    }
    // (prev = Q_15)  F(x) (W' + 2^32 (CW_0 + 2 CW_1) - Q_15)
    const uint64_t carry = gl_mul(gl_add(CW0, gl_add(CW1, CW1)), 1ull << 32);
    plain(JS_NEXT, gl_mul(fx, gl_sub(gl_add(Wn, carry), prev)));
    t = gl2_add(gl2_mul(t, g117), {gl_canon(a0), gl_canon(a1)});
  }
  const gl2 q = gl2_scale(t, zinv);
  out[i] = q.c0;
  out[M + i] = q.c1;
}

// The set-4 identity at zeta, one workgroup: gamma^0 .. gamma^117 and P_F go to LDS first; thread t takes the proofs t, t + 256, ... and
// evaluates their 117 constraints over F_p^2 from the table's and the helper's openings at zeta (y0) and zeta omega_N (y1) in the order of
// the hot pass; F(zeta) by Horner on P_F at zeta^(N/64).  The sums meet in LDS; thread 0 compares with (u_0 + X u_1) (zeta^N - 1).
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_sched_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub,
                                                                        uint64_t om64_inv, const uint64_t* __restrict__ open_t,
                                                                        const uint64_t* __restrict__ open_h, const uint64_t* __restrict__ open_q,
                                                                        const uint64_t* __restrict__ zeta, const uint64_t* __restrict__ gamma,
                                                                        uint32_t n_queries, uint32_t* __restrict__ ok) {
  __shared__ uint64_t red[2][AIR_CHECK_THREADS];
  __shared__ uint64_t gpw[2 * (AIR_SCHED_CONSTRAINTS + 1)];
  __shared__ uint64_t pf[64];
  __shared__ uint32_t holds;
  const uint32_t t = threadIdx.x;
  const uint64_t RT = 1ull << log_r_t, RH = 1ull << log_r_h;
  const gl2 g = {gamma[0], gamma[1]}, z = {zeta[0], zeta[1]};
  for (uint32_t k = t; k <= AIR_SCHED_CONSTRAINTS; k += AIR_CHECK_THREADS) {
    const gl2 gk = gl2_pow(g, k);
    gpw[2 * k] = gk.c0;
    gpw[2 * k + 1] = gk.c1;
  }
  air_sched_pf(om64_inv, pf);  // (ends with a barrier: gpw is complete behind it too)
  gl2 zp = z;  // zeta^(N/64)
  for (uint32_t k = 6; k < log_sub; k++) zp = gl2_mul(zp, zp);
  gl2 F = {0, 0};
  for (int j = 63; j >= 0; j--) {
    F = gl2_mul(F, zp);
    F.c0 = gl_add(F.c0, pf[j]);
  }
  auto t0 = [&](uint64_t c) -> gl2 { return {gl_canon(open_t[c]), gl_canon(open_t[RT + c])}; };
  auto t1 = [&](uint64_t c) -> gl2 { return {gl_canon(open_t[2 * RT + c]), gl_canon(open_t[3 * RT + c])}; };
  auto h0 = [&](uint64_t c) -> gl2 { return {gl_canon(open_h[c]), gl_canon(open_h[RH + c])}; };
  auto h1 = [&](uint64_t c) -> gl2 { return {gl_canon(open_h[2 * RH + c]), gl_canon(open_h[3 * RH + c])}; };
  auto boolean = [](gl2 x) { return gl2_sub(gl2_mul(x, x), x); };
  auto exor = [](gl2 x, gl2 y) {
    const gl2 xy = gl2_mul(x, y);
    return gl2_sub(gl2_add(x, y), gl2_add(xy, xy));
  };
  auto dbl_add = [](gl2 s, gl2 x) { return gl2_add(gl2_add(s, s), x); };
  gl2 sum = {0, 0};
  for (uint32_t p = t; p < n_proofs; p += AIR_CHECK_THREADS) {
    const uint64_t ct = (uint64_t)p * AIR_SHA_WIDTH, chh = (uint64_t)p * AIR_SCHED_HELPER_COLS;
    gl2 a = {0, 0};
    auto plain = [&](uint32_t j, gl2 v) { a = gl2_add(a, gl2_mul({gpw[2 * j], gpw[2 * j + 1]}, v)); };
    gl2 ww = {0, 0}, wg0 = ww, wg1 = ww;
    for (uint32_t b = 32; b-- > 0;) {
      const gl2 WB = h0(chh + S_WB + b), X0 = h0(chh + S_X0 + b), X1 = h0(chh + S_X1 + b);
      const gl2 W7 = h0(chh + S_WB + ((b + 7) & 31)), W18 = h0(chh + S_WB + ((b + 18) & 31));
      const gl2 W17 = h0(chh + S_WB + ((b + 17) & 31)), W19 = h0(chh + S_WB + ((b + 19) & 31));
      plain(S_WB + b, boolean(WB));
      plain(JS_X0 + b, gl2_sub(X0, exor(W7, W18)));
      plain(JS_X1 + b, gl2_sub(X1, exor(W17, W19)));
      ww = dbl_add(ww, WB);
      wg0 = dbl_add(wg0, b < 29 ? exor(X0, h0(chh + S_WB + ((b + 3) & 31))) : X0);
      wg1 = dbl_add(wg1, b < 22 ? exor(X1, h0(chh + S_WB + ((b + 10) & 31))) : X1);
    }
    const gl2 W = t0(ct), Wn = t1(ct);
    const gl2 G0 = h0(chh + S_G0), G1 = h0(chh + S_G1), CW0 = h0(chh + S_CW), CW1 = h0(chh + S_CW + 1);
    plain(JS_WORD, gl2_sub(W, ww));
    plain(JS_G0, gl2_sub(G0, wg0));
    plain(JS_G1, gl2_sub(G1, wg1));
    plain(JS_CW, boolean(CW0));
    plain(JS_CW + 1, boolean(CW1));
    gl2 prev = gl2_add(W, h1(chh + S_G0));
    for (uint32_t k = 1; k <= 15; k++) {
      plain(JS_Q + k, gl2_sub(h1(chh + S_Q + k), prev));
      prev = h0(chh + S_Q + k);
      if (k + 1 == 9) prev = gl2_add(prev, Wn);
      if (k + 1 == 14) prev = gl2_add(prev, h1(chh + S_G1));
    }
    const gl2 carry = gl2_scale(gl2_add(CW0, gl2_add(CW1, CW1)), 1ull << 32);
    plain(JS_NEXT, gl2_mul(F, gl2_sub(gl2_add(Wn, carry), prev)));
    sum = gl2_add(sum, gl2_mul(gl2_pow(g, (uint64_t)AIR_SCHED_CONSTRAINTS * p), a));
  }
  red[0][t] = sum.c0;
  red[1][t] = sum.c1;
  for (uint32_t hh = AIR_CHECK_THREADS / 2; hh; hh >>= 1) {
    __syncthreads();
    if (t < hh) {
      red[0][t] = gl_add(red[0][t], red[0][t + hh]);
      red[1][t] = gl_add(red[1][t], red[1][t + hh]);
    }
  }
  __syncthreads();
  if (t == 0) {
    gl2 zn = zp;  // zeta^N = (zeta^(N/64))^64
    for (uint32_t k = 0; k < 6; k++) zn = gl2_mul(zn, zn);
    const gl2 u0 = {gl_canon(open_q[0]), gl_canon(open_q[2])}, u1 = {gl_canon(open_q[1]), gl_canon(open_q[3])};
    const gl2 q = {gl_add(u0.c0, gl_mul(u1.c1, 7)), gl_add(u0.c1, u1.c0)};
    holds = gl2_eq({red[0][0], red[1][0]}, gl2_mul(q, {gl_sub(zn.c0, 1), zn.c1})) ? 1u : 0u;
  }
  __syncthreads();
  if (!holds)
    for (uint32_t q = t; q < n_queries; q += AIR_CHECK_THREADS) ok[q] = 0;
}

int launch_air_sched_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream) {
  const uint64_t n = (uint64_t)n_proofs << log_rows;
  hipLaunchKernelGGL(k_air_sched_helper, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S_(stream), log_rows, n_proofs,
                     reinterpret_cast<const uint64_t*>(d_table), reinterpret_cast<uint64_t*>(d_helper));
  return (int)hipGetLastError();
}
int launch_air_sched_tables(uint32_t log_blowup, uint64_t s_n, uint64_t w_n, uint64_t s_n64, uint64_t w_n64, uint64_t om64_inv, const void* d_gamma,
                            void* d_tab, void* stream) {
  hipLaunchKernelGGL(k_air_sched_tables, dim3(((64u << log_blowup) + 255) / 256), dim3(256), 0, S_(stream), log_blowup, s_n, w_n, s_n64, w_n64,
                     om64_inv, reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<uint64_t*>(d_tab));
  return (int)hipGetLastError();
}
int launch_air_sched_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_helper_cols,
                              const void* d_tab, void* d_quot, void* stream) {
  hipLaunchKernelGGL(k_air_sched_quotient, dim3((uint32_t)(((1ull << log_m) + AIR_THREADS - 1) / AIR_THREADS)), dim3(AIR_THREADS), 0, S_(stream),
                     log_m, log_blowup, n_proofs, reinterpret_cast<const uint64_t*>(d_cols), reinterpret_cast<const uint64_t*>(d_helper_cols),
                     reinterpret_cast<const uint64_t*>(d_tab), reinterpret_cast<uint64_t*>(d_quot));
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
// Siblings again: nothing above changes.  Row 0 of a block is round 0 applied to the words the block starts from, so six of those eight
// words stand in row 0 itself (b, c, d, f, g, h) and set 3's bit machinery runs on them with the register names shifted by one.  Helper
// column offsets inside a proof's 315, constraint indices inside its 337.
constexpr uint32_t I_B = 0, I_C = 32, I_D = 64, I_F = 96, I_G = 128, I_H = 160, I_U0 = 192, I_U1 = 224, I_V = 256, I_S0 = 288, I_S1 = 289, I_CH = 290,
                   I_MAJ = 291, I_LV = 292, I_PZ = 293, I_CZ = 301, I_CA = 309, I_CE = 312;
constexpr uint32_t JI_CZ = 192, JI_CARRY = 200, JI_LV = 206, JI_WORD = 207, JI_U0 = 213, JI_U1 = 245, JI_V = 277, JI_S0 = 309, JI_S1 = 310, JI_CH = 311,
                   JI_MAJ = 312, JI_PZ = 313, JI_START = 321, JI_CHAIN = 329;
__device__ __constant__ const uint32_t IV_SHA256[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                                                       0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
constexpr uint64_t INIT_IV3 = 0xa54ff53aull, INIT_IV7 = 0x5be0cd19ull, INIT_K0 = 0x428a2f98ull;

__device__ __forceinline__ uint32_t init_rot(uint32_t x, uint32_t n) { return (x >> n) | (x << (32 - n)); }
__device__ __forceinline__ uint32_t init_big0(uint32_t b) { return init_rot(b, 2) ^ init_rot(b, 13) ^ init_rot(b, 22); }
__device__ __forceinline__ uint32_t init_big1(uint32_t f) { return init_rot(f, 6) ^ init_rot(f, 11) ^ init_rot(f, 25); }

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
  const uint32_t u0 = init_rot(b, 2) ^ init_rot(b, 13), u1 = init_rot(f, 6) ^ init_rot(f, 11), v = b & c;
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

// n <= 8 nonzero values inverted with one field inversion (Montgomery's trick)
__device__ __forceinline__ void air_init_batch_inverse(uint64_t (&v)[8], uint32_t n) {
  uint64_t pre[8], acc = 1;
#pragma unroll
  for (uint32_t j = 0; j < 8; j++)
    if (j < n) {
      pre[j] = acc;
      acc = gl_mul(acc, v[j]);
    }
  uint64_t inv = gl_pow(acc, GL_P - 2);
#pragma unroll
  for (uint32_t j = 8; j-- > 0;)
    if (j < n) {
      const uint64_t x = gl_mul(inv, pre[j]);
      inv = gl_mul(inv, v[j]);
      v[j] = x;
    }
}

// One thread per eight table entries, inverted as a batch: 1 / D_s(x_i) by i mod 64 B (chain = 0: D_s = x^(N/64) - omega_64^-1) or by
// i mod 128 B (chain = 1: D_s = x^(N/128) - rho, rho = omega_128^-1), from s_sel = s^(N/64) or s^(N/128) and w_sel likewise; 1 / (x^N - 1)
// by i mod B; and one thread per power gamma^0 .. gamma^337.  Under chain = 1 the same table holds 1 / D_c: x^(N/128) changes its sign
// 64 B points on, so D_c(x_i) = x_i^(N/128) + rho = -D_s(x_(i + 64 B)).  No entry vanishes: D_s divides x^N - 1, which the caller checked.
__global__ __launch_bounds__(256) void k_air_init_tables(uint32_t log_blowup, uint32_t chain, uint64_t s_n, uint64_t w_n, uint64_t s_sel,
                                                         uint64_t w_sel, uint64_t rho, const uint64_t* __restrict__ gamma,
                                                         uint64_t* __restrict__ tab) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x, first = 8 * k;
  const uint32_t n_sel = (chain ? 128u : 64u) << log_blowup, n_z = 1u << log_blowup;
  uint64_t v[8];
  if (first < n_sel) {  // (n_sel is a multiple of 8)
    uint64_t x = gl_mul(s_sel, gl_pow(w_sel, first));
#pragma unroll
    for (uint32_t j = 0; j < 8; j++, x = gl_mul(x, w_sel)) v[j] = gl_sub(x, rho);
    air_init_batch_inverse(v, 8);
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) tab[AIR5_TAB_SEL + first + j] = v[j];
  }
  if (first < n_z) {
    const uint32_t n = n_z - first < 8 ? n_z - first : 8;
    uint64_t x = gl_mul(s_n, gl_pow(w_n, first));
#pragma unroll
    for (uint32_t j = 0; j < 8; j++, x = gl_mul(x, w_n)) v[j] = gl_sub(x, 1);
    air_init_batch_inverse(v, n);
#pragma unroll
    for (uint32_t j = 0; j < 8; j++)
      if (j < n) tab[AIR5_TAB_ZINV + first + j] = v[j];
  }
  if (k <= AIR_INIT_CONSTRAINTS) {
    const gl2 g = gl2_pow({gamma[0], gamma[1]}, k);
    tab[AIR5_TAB_GPOW + 2 * k] = g.c0;
    tab[AIR5_TAB_GPOW + 2 * k + 1] = g.c1;
  }
}

// The set-5 hot pass, k_air_sha_quotient's shape: one lane per point, a loop over the proofs from the last to the first (Horner by
// gamma^337), the nine table columns and the 315 helper columns.  It walks the bit index b from 31 down to 0 and per b holds the nine bit
// words B_b .. V_b and the six rotated ones (B_(b+2), B_(b+13), B_(b+22), F_(b+6), F_(b+11), F_(b+25)), which are re-read through the
// cache, so the 288 bit words are never held.  Per b: nine constraints (six X^2 - X, U0, U1, V) and one Horner step by 2 of the ten word
// sums: 13 reduced column products and 18 gamma weights.  Behind the loop the word constraints, LV, the eight PZ constraints with their CZ
// bits, the six carry bits, and the sixteen selected linear forms at i + B in two gamma sums of their own: 1 / D_s is applied once to the
// start sum, 1 / D_c once to the chain sum (skipped under chain = 0: E_c = 0), 1 / (x^N - 1) once to the rest.  The gamma sums are lazy.
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
    const uint64_t* __restrict__ c = cols + (((uint64_t)p * AIR_SHA_WIDTH) << log_m);
    const uint64_t* __restrict__ h = hcols + (((uint64_t)p * AIR_INIT_HELPER_COLS) << log_m);
    auto once = [&](uint32_t col) { return gl_canon(__builtin_nontemporal_load(h + ((uint64_t)col << log_m) + i)); };
    auto again = [&](uint32_t col) { return gl_canon(h[((uint64_t)col << log_m) + i]); };
    auto next = [&](uint32_t col) { return gl_canon(h[((uint64_t)col << log_m) + nx]); };
    auto tbl = [&](uint32_t col, uint64_t at) { return gl_canon(c[((uint64_t)col << log_m) + at]); };
    uint64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0, c0 = 0, c1 = 0;  // the plain, the start and the chain gamma sums, lazy
    auto plain = [&](uint32_t j, uint64_t v) {
      a0 = gl_add_lazy(a0, gl_mul(gp[2 * j], v));
      a1 = gl_add_lazy(a1, gl_mul(gp[2 * j + 1], v));
    };
    auto started = [&](uint32_t j, uint64_t v) {
      b0 = gl_add_lazy(b0, gl_mul(gp[2 * j], v));
      b1 = gl_add_lazy(b1, gl_mul(gp[2 * j + 1], v));
    };
    auto chained = [&](uint32_t j, uint64_t v) {
      c0 = gl_add_lazy(c0, gl_mul(gp[2 * j], v));
      c1 = gl_add_lazy(c1, gl_mul(gp[2 * j + 1], v));
    };
    auto boolean = [](uint64_t x) { return gl_sub(gl_mul(x, x), x); };
    auto exor = [](uint64_t x, uint64_t y) {  // x + y - 2 x y
      const uint64_t xy = gl_mul(x, y);
      return gl_sub(gl_add(x, y), gl_add(xy, xy));
    };
    auto dbl_add = [](uint64_t s, uint64_t x) { return gl_add(gl_add(s, s), x); };
    uint64_t wb = 0, wc = 0, wd = 0, wf = 0, wg = 0, wh = 0, ws0 = 0, ws1 = 0, wch = 0, wmj = 0;
#pragma unroll 2
    for (uint32_t b = 32; b-- > 0;) {
      const uint64_t B = again(I_B + b), C = once(I_C + b), D = once(I_D + b), F = again(I_F + b), G = once(I_G + b), H = once(I_H + b);
      const uint64_t U0 = once(I_U0 + b), U1 = once(I_U1 + b), V = once(I_V + b);
      const uint64_t B2 = again(I_B + ((b + 2) & 31)), B13 = again(I_B + ((b + 13) & 31)), B22 = again(I_B + ((b + 22) & 31));
      const uint64_t F6 = again(I_F + ((b + 6) & 31)), F11 = again(I_F + ((b + 11) & 31)), F25 = again(I_F + ((b + 25) & 31));
      plain(I_B + b, boolean(B));
      plain(I_C + b, boolean(C));
      plain(I_D + b, boolean(D));
      plain(I_F + b, boolean(F));
      plain(I_G + b, boolean(G));
      plain(I_H + b, boolean(H));
      plain(JI_U0 + b, gl_sub(U0, exor(B2, B13)));
      plain(JI_U1 + b, gl_sub(U1, exor(F6, F11)));
      plain(JI_V + b, gl_sub(V, gl_mul(B, C)));
      wb = dbl_add(wb, B);
      wc = dbl_add(wc, C);
      wd = dbl_add(wd, D);
      wf = dbl_add(wf, F);
      wg = dbl_add(wg, G);
      wh = dbl_add(wh, H);
      ws0 = dbl_add(ws0, exor(U0, B22));
      ws1 = dbl_add(ws1, exor(U1, F25));
      wch = dbl_add(wch, gl_add(H, gl_mul(F, gl_sub(G, H))));
      wmj = dbl_add(wmj, gl_add(V, gl_mul(D, gl_sub(gl_add(B, C), gl_add(V, V)))));
    }
    plain(JI_WORD + 0, gl_sub(tbl(T_B, i), wb));
    plain(JI_WORD + 1, gl_sub(tbl(T_C, i), wc));
    plain(JI_WORD + 2, gl_sub(tbl(T_D, i), wd));
    plain(JI_WORD + 3, gl_sub(tbl(T_F, i), wf));
    plain(JI_WORD + 4, gl_sub(tbl(T_G, i), wg));
    plain(JI_WORD + 5, gl_sub(tbl(T_H, i), wh));
    plain(JI_S0, gl_sub(again(I_S0), ws0));
    plain(JI_S1, gl_sub(again(I_S1), ws1));
    plain(JI_CH, gl_sub(again(I_CH), wch));
    plain(JI_MAJ, gl_sub(again(I_MAJ), wmj));
    plain(JI_LV, boolean(again(I_LV)));
    // the six carry bits, folded into the two words 2^32 CA and 2^32 CE at once
    uint64_t ca32 = 0, ce32 = 0;
#pragma unroll
    for (uint32_t k = 3; k-- > 0;) {
      const uint64_t CA = once(I_CA + k), CE = once(I_CE + k);
      plain(JI_CARRY + k, boolean(CA));
      plain(JI_CARRY + 3 + k, boolean(CE));
      ca32 = dbl_add(ca32, CA);
      ce32 = dbl_add(ce32, CE);
    }
    ca32 = gl_mul(ca32, 1ull << 32);
    ce32 = gl_mul(ce32, 1ull << 32);
    // PZ_j - LV' (IV_j + s_j - 2^32 CZ_j), and with each of the six words that stand in row 0 its two selected linear forms: the next
    // row's word against IV_j LV' (start rows) and against PZ_j (chain rows; skipped under chain = 0, uniformly)
    const uint64_t LVn = next(I_LV);
    uint64_t pz3 = 0, pz7 = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < 8; j++) {
      const uint64_t CZ = once(I_CZ + j), PZ = once(I_PZ + j);
      plain(JI_CZ + j, boolean(CZ));
      plain(JI_PZ + j, gl_sub(PZ, gl_mul(LVn, gl_sub(gl_add(tbl(T_A + j, i), IV_SHA256[j]), gl_mul(CZ, 1ull << 32)))));
      if (j == 3) pz3 = PZ;
      if (j == 7) pz7 = PZ;
      if (j != 3 && j != 7) {
        const uint32_t k = j < 3 ? j : j - 1;
        const uint64_t xn = tbl(T_B + j, nx);
        started(JI_START + k, gl_sub(xn, gl_mul(LVn, IV_SHA256[j])));
        if (chain) chained(JI_CHAIN + k, gl_sub(xn, PZ));
      }
    }
    // round 0 of the next row's block: a' and e' against the two sums
    const uint64_t t1 = gl_add(gl_add(next(I_S1), next(I_CH)), tbl(T_W, nx)), t12 = gl_add(t1, gl_add(next(I_S0), next(I_MAJ)));
    const uint64_t an = gl_add(tbl(T_A, nx), ca32), en = gl_add(tbl(T_E, nx), ce32);
    started(JI_START + 6, gl_sub(an, gl_add(gl_mul(LVn, INIT_IV7 + INIT_K0), t12)));
    started(JI_START + 7, gl_sub(en, gl_add(gl_mul(LVn, INIT_IV3 + INIT_IV7 + INIT_K0), t1)));
    uint64_t v0 = gl_add(gl_mul(gl_canon(a0), zinv), gl_mul(gl_canon(b0), dsinv));
    uint64_t v1 = gl_add(gl_mul(gl_canon(a1), zinv), gl_mul(gl_canon(b1), dsinv));
    if (chain) {  // (uniform)
      const uint64_t kl = gl_mul(LVn, INIT_K0);
      chained(JI_CHAIN + 6, gl_sub(an, gl_add(gl_add(pz7, kl), t12)));
      chained(JI_CHAIN + 7, gl_sub(en, gl_add(gl_add(pz3, pz7), gl_add(kl, t1))));
      v0 = gl_add(v0, gl_mul(gl_canon(c0), dcinv));
      v1 = gl_add(v1, gl_mul(gl_canon(c1), dcinv));
    }
    t = gl2_add(gl2_mul(t, g337), {v0, v1});
  }
  out[i] = t.c0;
  out[M + i] = t.c1;
}

// The set-5 identity at zeta, one workgroup, division-free: gamma^0 .. gamma^337 go to LDS first; thread t takes the proofs t, t + 256, ...
// and evaluates their 337 constraints over F_p^2 from the table's and the helper's openings at zeta (y0) and zeta omega_N (y1) in the
// order of the hot pass, in three sums.  With z = zeta^(N/128), D_s = z - rho, D_c = z + rho and S = D_s D_c under chain = 1 (z =
// zeta^(N/64), S = z - rho, D_c = 1 and no chain sum under chain = 0), a proof contributes S a + (zeta^N - 1) (D_c b + D_s c); the sums meet
// in LDS; thread 0 compares with (u_0 + X u_1) (zeta^N - 1) S.
__global__ __launch_bounds__(AIR_CHECK_THREADS) void k_air_init_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub,
                                                                       uint32_t chain, uint64_t rho, const uint64_t* __restrict__ open_t,
                                                                       const uint64_t* __restrict__ open_h, const uint64_t* __restrict__ open_q,
                                                                       const uint64_t* __restrict__ zeta, const uint64_t* __restrict__ gamma,
                                                                       uint32_t n_queries, uint32_t* __restrict__ ok) {
  __shared__ uint64_t red[2][AIR_CHECK_THREADS];
  __shared__ uint64_t gpw[2 * (AIR_INIT_CONSTRAINTS + 1)];
  __shared__ uint32_t holds;
  const uint32_t t = threadIdx.x;
  const uint64_t RT = 1ull << log_r_t, RH = 1ull << log_r_h;
  const gl2 g = {gamma[0], gamma[1]}, z = {zeta[0], zeta[1]};
  for (uint32_t k = t; k <= AIR_INIT_CONSTRAINTS; k += AIR_CHECK_THREADS) {
    const gl2 gk = gl2_pow(g, k);
    gpw[2 * k] = gk.c0;
    gpw[2 * k + 1] = gk.c1;
  }
  __syncthreads();
  const uint32_t log_sel = chain ? 7 : 6;
  gl2 zp = z;  // zeta^(N/128) or zeta^(N/64)
  for (uint32_t k = log_sel; k < log_sub; k++) zp = gl2_mul(zp, zp);
  gl2 zn = zp;  // zeta^N
  for (uint32_t k = 0; k < log_sel; k++) zn = gl2_mul(zn, zn);
  const gl2 zn1 = {gl_sub(zn.c0, 1), zn.c1};
  const gl2 Ds = {gl_sub(zp.c0, rho), zp.c1}, Dc = chain ? gl2{gl_add(zp.c0, rho), zp.c1} : gl2{1, 0};
  const gl2 S = chain ? gl2_mul(Ds, Dc) : Ds;
  auto t0 = [&](uint64_t c) -> gl2 { return {gl_canon(open_t[c]), gl_canon(open_t[RT + c])}; };
  auto t1 = [&](uint64_t c) -> gl2 { return {gl_canon(open_t[2 * RT + c]), gl_canon(open_t[3 * RT + c])}; };
  auto h0 = [&](uint64_t c) -> gl2 { return {gl_canon(open_h[c]), gl_canon(open_h[RH + c])}; };
  auto h1 = [&](uint64_t c) -> gl2 { return {gl_canon(open_h[2 * RH + c]), gl_canon(open_h[3 * RH + c])}; };
  auto boolean = [](gl2 x) { return gl2_sub(gl2_mul(x, x), x); };
  auto exor = [](gl2 x, gl2 y) {
    const gl2 xy = gl2_mul(x, y);
    return gl2_sub(gl2_add(x, y), gl2_add(xy, xy));
  };
  auto dbl_add = [](gl2 s, gl2 x) { return gl2_add(gl2_add(s, s), x); };
  gl2 sum = {0, 0};
  for (uint32_t p = t; p < n_proofs; p += AIR_CHECK_THREADS) {
    const uint64_t ct = (uint64_t)p * AIR_SHA_WIDTH, chh = (uint64_t)p * AIR_INIT_HELPER_COLS;
    gl2 a = {0, 0}, bs = {0, 0}, bc = {0, 0};
    auto plain = [&](uint32_t j, gl2 v) { a = gl2_add(a, gl2_mul({gpw[2 * j], gpw[2 * j + 1]}, v)); };
    auto started = [&](uint32_t j, gl2 v) { bs = gl2_add(bs, gl2_mul({gpw[2 * j], gpw[2 * j + 1]}, v)); };
    auto chained = [&](uint32_t j, gl2 v) { bc = gl2_add(bc, gl2_mul({gpw[2 * j], gpw[2 * j + 1]}, v)); };
    gl2 wb = {0, 0}, wc = wb, wd = wb, wf = wb, wg = wb, wh = wb, ws0 = wb, ws1 = wb, wch = wb, wmj = wb;
    for (uint32_t b = 32; b-- > 0;) {
      const gl2 B = h0(chh + I_B + b), C = h0(chh + I_C + b), D = h0(chh + I_D + b), F = h0(chh + I_F + b), G = h0(chh + I_G + b),
                H = h0(chh + I_H + b), U0 = h0(chh + I_U0 + b), U1 = h0(chh + I_U1 + b), V = h0(chh + I_V + b);
      const gl2 B2 = h0(chh + I_B + ((b + 2) & 31)), B13 = h0(chh + I_B + ((b + 13) & 31)), B22 = h0(chh + I_B + ((b + 22) & 31));
      const gl2 F6 = h0(chh + I_F + ((b + 6) & 31)), F11 = h0(chh + I_F + ((b + 11) & 31)), F25 = h0(chh + I_F + ((b + 25) & 31));
      plain(I_B + b, boolean(B));
      plain(I_C + b, boolean(C));
      plain(I_D + b, boolean(D));
      plain(I_F + b, boolean(F));
      plain(I_G + b, boolean(G));
      plain(I_H + b, boolean(H));
      plain(JI_U0 + b, gl2_sub(U0, exor(B2, B13)));
      plain(JI_U1 + b, gl2_sub(U1, exor(F6, F11)));
      plain(JI_V + b, gl2_sub(V, gl2_mul(B, C)));
      wb = dbl_add(wb, B);
      wc = dbl_add(wc, C);
      wd = dbl_add(wd, D);
      wf = dbl_add(wf, F);
      wg = dbl_add(wg, G);
      wh = dbl_add(wh, H);
      ws0 = dbl_add(ws0, exor(U0, B22));
      ws1 = dbl_add(ws1, exor(U1, F25));
      wch = dbl_add(wch, gl2_add(H, gl2_mul(F, gl2_sub(G, H))));
      wmj = dbl_add(wmj, gl2_add(V, gl2_mul(D, gl2_sub(gl2_add(B, C), gl2_add(V, V)))));
    }
    plain(JI_WORD + 0, gl2_sub(t0(ct + T_B), wb));
    plain(JI_WORD + 1, gl2_sub(t0(ct + T_C), wc));
    plain(JI_WORD + 2, gl2_sub(t0(ct + T_D), wd));
    plain(JI_WORD + 3, gl2_sub(t0(ct + T_F), wf));
    plain(JI_WORD + 4, gl2_sub(t0(ct + T_G), wg));
    plain(JI_WORD + 5, gl2_sub(t0(ct + T_H), wh));
    plain(JI_S0, gl2_sub(h0(chh + I_S0), ws0));
    plain(JI_S1, gl2_sub(h0(chh + I_S1), ws1));
    plain(JI_CH, gl2_sub(h0(chh + I_CH), wch));
    plain(JI_MAJ, gl2_sub(h0(chh + I_MAJ), wmj));
    plain(JI_LV, boolean(h0(chh + I_LV)));
    gl2 ca32 = {0, 0}, ce32 = {0, 0};
    for (uint32_t k = 3; k-- > 0;) {
      const gl2 CA = h0(chh + I_CA + k), CE = h0(chh + I_CE + k);
      plain(JI_CARRY + k, boolean(CA));
      plain(JI_CARRY + 3 + k, boolean(CE));
      ca32 = dbl_add(ca32, CA);
      ce32 = dbl_add(ce32, CE);
    }
    ca32 = gl2_scale(ca32, 1ull << 32);
    ce32 = gl2_scale(ce32, 1ull << 32);
    const gl2 LVn = h1(chh + I_LV);
    gl2 pz3 = {0, 0}, pz7 = {0, 0};
#pragma unroll 1
    for (uint32_t j = 0; j < 8; j++) {
      const gl2 CZ = h0(chh + I_CZ + j), PZ = h0(chh + I_PZ + j);
      gl2 s = t0(ct + T_A + j);
      s.c0 = gl_add(s.c0, IV_SHA256[j]);
      plain(JI_CZ + j, boolean(CZ));
      plain(JI_PZ + j, gl2_sub(PZ, gl2_mul(LVn, gl2_sub(s, gl2_scale(CZ, 1ull << 32)))));
      if (j == 3) pz3 = PZ;
      if (j == 7) pz7 = PZ;
      if (j != 3 && j != 7) {
        const uint32_t k = j < 3 ? j : j - 1;
        const gl2 xn = t1(ct + T_B + j);
        started(JI_START + k, gl2_sub(xn, gl2_scale(LVn, IV_SHA256[j])));
        if (chain) chained(JI_CHAIN + k, gl2_sub(xn, PZ));
      }
    }
    const gl2 tt = gl2_add(gl2_add(h1(chh + I_S1), h1(chh + I_CH)), t1(ct + T_W)), tt2 = gl2_add(tt, gl2_add(h1(chh + I_S0), h1(chh + I_MAJ)));
    const gl2 an = gl2_add(t1(ct + T_A), ca32), en = gl2_add(t1(ct + T_E), ce32);
    started(JI_START + 6, gl2_sub(an, gl2_add(gl2_scale(LVn, INIT_IV7 + INIT_K0), tt2)));
    started(JI_START + 7, gl2_sub(en, gl2_add(gl2_scale(LVn, INIT_IV3 + INIT_IV7 + INIT_K0), tt)));
    if (chain) {
      const gl2 kl = gl2_scale(LVn, INIT_K0);
      chained(JI_CHAIN + 6, gl2_sub(an, gl2_add(gl2_add(pz7, kl), tt2)));
      chained(JI_CHAIN + 7, gl2_sub(en, gl2_add(gl2_add(pz3, pz7), gl2_add(kl, tt))));
    }
    const gl2 v = gl2_add(gl2_mul(S, a), gl2_mul(zn1, gl2_add(gl2_mul(Dc, bs), gl2_mul(Ds, bc))));
    sum = gl2_add(sum, gl2_mul(gl2_pow(g, (uint64_t)AIR_INIT_CONSTRAINTS * p), v));
  }
  red[0][t] = sum.c0;
  red[1][t] = sum.c1;
  for (uint32_t hh = AIR_CHECK_THREADS / 2; hh; hh >>= 1) {
    __syncthreads();
    if (t < hh) {
      red[0][t] = gl_add(red[0][t], red[0][t + hh]);
      red[1][t] = gl_add(red[1][t], red[1][t + hh]);
    }
  }
  __syncthreads();
  if (t == 0) {
    const gl2 u0 = {gl_canon(open_q[0]), gl_canon(open_q[2])}, u1 = {gl_canon(open_q[1]), gl_canon(open_q[3])};
    const gl2 q = {gl_add(u0.c0, gl_mul(u1.c1, 7)), gl_add(u0.c1, u1.c0)};
    holds = gl2_eq({red[0][0], red[1][0]}, gl2_mul(gl2_mul(q, zn1), S)) ? 1u : 0u;
  }
  __syncthreads();
  if (!holds)
    for (uint32_t q = t; q < n_queries; q += AIR_CHECK_THREADS) ok[q] = 0;
}

int launch_air_init_helper(uint32_t log_rows, uint32_t n_proofs, uint32_t chain, const void* d_table, void* d_helper, void* stream) {
  const uint64_t n = (uint64_t)n_proofs << log_rows;
  hipLaunchKernelGGL(k_air_init_helper, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S_(stream), log_rows, n_proofs, chain,
                     reinterpret_cast<const uint64_t*>(d_table), reinterpret_cast<uint64_t*>(d_helper));
  return (int)hipGetLastError();
}
int launch_air_init_tables(uint32_t log_blowup, uint32_t chain, uint64_t s_n, uint64_t w_n, uint64_t s_sel, uint64_t w_sel, uint64_t rho,
                           const void* d_gamma, void* d_tab, void* stream) {
  // (at least two workgroups: the 338 gamma powers)
  const uint32_t blocks = ((((chain ? 128u : 64u) << log_blowup) / 8) + 255) / 256;
  hipLaunchKernelGGL(k_air_init_tables, dim3(blocks < 2 ? 2 : blocks), dim3(256), 0, S_(stream), log_blowup, chain, s_n, w_n, s_sel, w_sel, rho,
                     reinterpret_cast<const uint64_t*>(d_gamma), reinterpret_cast<uint64_t*>(d_tab));
  return (int)hipGetLastError();
}
int launch_air_init_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, uint32_t chain, const void* d_cols, const void* d_helper_cols,
                             const void* d_tab, void* d_quot, void* stream) {
  hipLaunchKernelGGL(k_air_init_quotient, dim3((uint32_t)(((1ull << log_m) + AIR_THREADS - 1) / AIR_THREADS)), dim3(AIR_THREADS), 0, S_(stream),
                     log_m, log_blowup, n_proofs, chain, reinterpret_cast<const uint64_t*>(d_cols), reinterpret_cast<const uint64_t*>(d_helper_cols),
                     reinterpret_cast<const uint64_t*>(d_tab), reinterpret_cast<uint64_t*>(d_quot));
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

}  // namespace tmx
