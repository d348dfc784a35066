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

}  // namespace tmx
