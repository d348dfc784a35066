// The field-only kernels of the batched FRI proof (include/tmx.h "a batched FRI low-degree proof"): the batching pass over the committed
// columns, the folds between layers and the final polynomial.  The kernels that need the Poseidon permutation (transcript, verifier) sit
// beside it in poseidon.hip.  Goldilocks words, F_p^2 = F_p[X] / (X^2 - 7) values (goldilocks_ext.hpp); no MFMA (nothing is a contraction).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "fri.h"
#include "goldilocks_ext.hpp"

namespace tmx {

__global__ __launch_bounds__(256) void k_fri_alpha_powers(uint32_t n_cols, const uint64_t* __restrict__ alpha, uint64_t* __restrict__ apow) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cols) return;
  const gl2 a = gl2_pow({alpha[0], alpha[1]}, c);
  apow[2 * c] = a.c0;
  apow[2 * c + 1] = a.c1;
}

// The only pass over the committed data: every word is read once.  A block is 64 rows (one per lane) and four waves; wave w takes the
// w-th quarter of the columns, so every load is one column's 64 consecutive words (a 512-B wave load) and the column index is wave-uniform:
// alpha^c comes through the scalar cache (s_load of the wave-uniform table entry) instead of an LDS tile.  Eight columns are loaded
// before they are accumulated (eight loads in flight per wave).  The products are reduced (gl_mul), the sums are lazy (any representative:
// gl_add_lazy with a canonical second operand), and the four partial sums meet in LDS -- no atomics.  Writes layer 0 planar, canonical.
// ACC (the batch proof: the second and later oracles of a group): the row's sum is added to what `out` holds -- one more read of the
// output per ROW, nothing per word; the oracle's alpha offset is in the table pointer, not in the loop.
constexpr int COMBINE_WAVES = 4, COMBINE_UNROLL = 8;
template <bool ACC>
__global__ __launch_bounds__(64 * COMBINE_WAVES) void k_fri_combine(uint32_t log_m, uint32_t n_cols, const uint64_t* __restrict__ cols,
                                                                    const uint64_t* __restrict__ apow, uint64_t* __restrict__ out) {
  __shared__ uint64_t part[COMBINE_WAVES - 1][2][64];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t M = 1ull << log_m, row = (uint64_t)blockIdx.x * 64 + lane;
  const uint32_t chunk = (n_cols + COMBINE_WAVES - 1) / COMBINE_WAVES;
  const uint32_t c_lo = min(n_cols, wave * chunk), c_hi = min(n_cols, c_lo + chunk);
  uint64_t a0 = 0, a1 = 0, h0 = 0, h1 = 0;
  if (ACC && wave == 0 && row < M) {  // (what the buffer holds, requested before the pass: its latency hides behind the column loop)
    h0 = out[row];
    h1 = out[M + row];
  }
  if (row < M) {
    const uint64_t* p = cols + ((uint64_t)c_lo << log_m) + row;
    uint32_t c = c_lo;
    for (; c + COMBINE_UNROLL <= c_hi; c += COMBINE_UNROLL) {
      uint64_t w[COMBINE_UNROLL];
#pragma unroll
      for (int k = 0; k < COMBINE_UNROLL; k++) w[k] = __builtin_nontemporal_load(p + ((uint64_t)k << log_m));
      p += (uint64_t)COMBINE_UNROLL << log_m;
#pragma unroll
      for (int k = 0; k < COMBINE_UNROLL; k++) {
        a0 = gl_add_lazy(a0, gl_mul(apow[2 * (c + k)], w[k]));
        a1 = gl_add_lazy(a1, gl_mul(apow[2 * (c + k) + 1], w[k]));
      }
    }
    for (; c < c_hi; c++, p += M) {
      const uint64_t w = *p;
      a0 = gl_add_lazy(a0, gl_mul(apow[2 * c], w));
      a1 = gl_add_lazy(a1, gl_mul(apow[2 * c + 1], w));
    }
  }
  if (wave) {
    part[wave - 1][0][lane] = a0;
    part[wave - 1][1][lane] = a1;
  }
  __syncthreads();
  if (wave == 0 && row < M) {
    a0 = gl_canon(a0); a1 = gl_canon(a1);
#pragma unroll
    for (int w = 0; w < COMBINE_WAVES - 1; w++) {
      a0 = gl_add(a0, gl_canon(part[w][0][lane]));
      a1 = gl_add(a1, gl_canon(part[w][1][lane]));
    }
    if (ACC) {
      a0 = gl_add(a0, h0);
      a1 = gl_add(a1, h1);
    }
    out[row] = a0;
    out[M + row] = a1;
  }
}

// dst[i] += src[i] over n canonical words (both planes of a group's buffer at once): a streamed oracle that does not open its group is
// combined on the trace domain, extended next to the buffer and added here -- what k_fri_combine<true> does in its last step.
__global__ __launch_bounds__(256) void k_fri_add(uint64_t n, const uint64_t* __restrict__ src, uint64_t* __restrict__ dst) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = gl_add(gl_canon(src[i]), dst[i]);
}

// One thread per leaf coset r < M' of layer l (M' = M_(l+1)): its 2^B values in registers, B radix-2 folds (fri_fold_leaf), one value of
// layer l + 1 out.  x_0^-1 = s^-1 (w^-1)^r: one exponentiation per thread.
// ADD (the batch proof: a group of smaller oracles enters layer l + 1): the group's quotient sum at the OUTPUT index r joins the value
// scaled by beta^(2^B), the first power the fold did not use -- one extra read of M_(l+1) values, no pass of its own.
template <int B, bool ADD>
__global__ __launch_bounds__(256) void k_fri_fold(uint32_t log_mn, uint64_t s_inv, uint64_t w_inv, uint64_t g, const uint64_t* __restrict__ beta,
                                                  const uint64_t* __restrict__ in, const uint64_t* __restrict__ add, uint64_t* __restrict__ out) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, Mn = 1ull << log_mn, M = Mn << B;
  if (r >= Mn) return;
  gl2 v[1 << B];
#pragma unroll
  for (int j = 0; j < (1 << B); j++) v[j] = {in[r + j * Mn], in[M + r + j * Mn]};
  gl2 f = fri_fold_leaf<B>(v, gl_mul(s_inv, gl_pow(w_inv, r)), g, {beta[0], beta[1]});
  if (ADD) {
    gl2 bp = {beta[0], beta[1]};
#pragma unroll
    for (int k = 0; k < B; k++) bp = gl2_mul(bp, bp);
    f = gl2_add(f, gl2_mul(bp, {add[r], add[Mn + r]}));
  }
  out[r] = f.c0;
  out[Mn + r] = f.c1;
}

// The final polynomial: one workgroup, one plane at a time in LDS (2^12 values + 2^11 twiddles: 48 KiB).  Inverse NTT (bit-reversed load,
// radix-2 DIT), then coefficient k times M^-1 s^-k; the low 2^final_log go out, the others must be zero (the degree flag).
constexpr int FINAL_THREADS = 1024, FINAL_MAX_LOG = 12;
__global__ __launch_bounds__(FINAL_THREADS) void k_fri_final(uint32_t log_m, uint32_t final_log, uint64_t w_inv, uint64_t s_inv, uint64_t m_inv,
                                                             const uint64_t* __restrict__ in, uint64_t* __restrict__ coef, uint32_t* __restrict__ flag) {
  __shared__ uint64_t x[1 << FINAL_MAX_LOG], tw[1 << (FINAL_MAX_LOG - 1)];
  __shared__ uint32_t nonzero;
  const uint32_t M = 1u << log_m, t = threadIdx.x;
  if (t == 0) nonzero = 0;
  for (uint32_t k = t; k < M / 2; k += FINAL_THREADS) tw[k] = gl_pow(w_inv, k);
  for (uint32_t plane = 0; plane < 2; plane++) {
    __syncthreads();
    for (uint32_t i = t; i < M; i += FINAL_THREADS) {
      const uint32_t rev = log_m ? __brev(i) >> (32 - log_m) : 0;
      x[rev] = gl_canon(in[(uint64_t)plane * M + i]);
    }
    for (uint32_t len = 2; len <= M; len <<= 1) {
      __syncthreads();
      const uint32_t half = len >> 1, step = M / len;
      for (uint32_t b = t; b < M / 2; b += FINAL_THREADS) {
        const uint32_t j = b & (half - 1), base = (b - j) * 2 + j;
        const uint64_t u = x[base], v = gl_mul(x[base + half], tw[j * step]);
        x[base] = gl_add(u, v);
        x[base + half] = gl_sub(u, v);
      }
    }
    __syncthreads();
    for (uint32_t k = t; k < M; k += FINAL_THREADS) {
      const uint64_t c = gl_mul(gl_mul(x[k], m_inv), gl_pow(s_inv, k));
      if (k >> final_log) {
        if (c) atomicOr(&nonzero, 1u);
      } else {
        coef[2 * k + plane] = c;
      }
    }
  }
  __syncthreads();
  if (t == 0) flag[0] = nonzero ? 0u : 1u;
}

// ---- DEEP: the openings at zeta and zeta omega_N (include/tmx.h "out-of-domain openings") ----------------------------------------------
// Barycentric weights on the subset x_j = s omega_N^j: one thread per j, one Fermat inversion in F_p^2 each.  K is folded in, so an opening is
// the plain dot product of a column with the table (and with the table rotated by one for zeta omega_N).
__global__ __launch_bounds__(256) void k_deep_weights(uint32_t log_sub, uint64_t s, uint64_t omega_n, uint64_t s_n, uint64_t k_inv,
                                                      const uint64_t* __restrict__ zeta, uint64_t* __restrict__ wt) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >> log_sub) return;
  const gl2 z = {zeta[0], zeta[1]};
  gl2 zn = z;
  for (uint32_t k = 0; k < log_sub; k++) zn = gl2_mul(zn, zn);
  const gl2 K = gl2_scale({gl_sub(zn.c0, s_n), zn.c1}, k_inv);
  const uint64_t x = gl_mul(s, gl_pow(omega_n, j));
  const gl2 w = gl2_mul(gl2_scale(gl2_inv({gl_sub(z.c0, x), z.c1}), x), K);
  wt[2 * j] = w.c0;
  wt[2 * j + 1] = w.c1;
}

// The hot pass: every word of the subset is read once.  A block is one wave and owns a row tile of 64 R rows (lane + 64 k, k < R: each load
// is 64 consecutive rows of one column) and a chunk of columns.  The tile's weights sit in registers for the whole chunk -- w[j] and w[j - 1]
// (the rotation that gives zeta omega_N), 4 words per row -- so the 0.5-MB table is read once per wave, not once per column.  Per column: R
// loads in flight, 4 R reduced products (a base word times an F_p^2 weight, twice), lazy sums, then one butterfly reduction over the wave;
// lane 0 writes the tile's four partial sums (k_deep_open adds the tiles).
constexpr int DEEP_ROWS = 8;
template <int R>
__global__ __launch_bounds__(64) void k_deep_eval(uint32_t log_sub, uint32_t log_col, uint32_t stride_log, uint32_t n_cols, uint32_t cols_per_chunk,
                                                  const uint64_t* __restrict__ cols, const uint64_t* __restrict__ wt, uint64_t* __restrict__ part) {
  const uint32_t lane = threadIdx.x, tile = blockIdx.x;
  const uint64_t N = 1ull << log_sub, mask = N - 1;
  uint64_t w0[R][2], w1[R][2];
  bool live[R];
#pragma unroll
  for (int k = 0; k < R; k++) {
    const uint64_t j = ((uint64_t)tile * R + k) * 64 + lane;
    live[k] = j < N;
    const uint64_t jm = (j - 1) & mask;
    w0[k][0] = live[k] ? wt[2 * j] : 0;
    w0[k][1] = live[k] ? wt[2 * j + 1] : 0;
    w1[k][0] = live[k] ? wt[2 * jm] : 0;
    w1[k][1] = live[k] ? wt[2 * jm + 1] : 0;
  }
  const uint32_t c_lo = blockIdx.y * cols_per_chunk, c_hi = min(n_cols, c_lo + cols_per_chunk);
  for (uint32_t c = c_lo; c < c_hi; c++) {
    const uint64_t* p = cols + ((uint64_t)c << log_col);
    uint64_t v[R];
#pragma unroll
    for (int k = 0; k < R; k++) {
      const uint64_t j = ((uint64_t)tile * R + k) * 64 + lane;
      v[k] = live[k] ? __builtin_nontemporal_load(p + (j << stride_log)) : 0;
    }
    uint64_t a[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < R; k++) {
      a[0] = gl_add_lazy(a[0], gl_mul(w0[k][0], v[k]));
      a[1] = gl_add_lazy(a[1], gl_mul(w0[k][1], v[k]));
      a[2] = gl_add_lazy(a[2], gl_mul(w1[k][0], v[k]));
      a[3] = gl_add_lazy(a[3], gl_mul(w1[k][1], v[k]));
    }
#pragma unroll
    for (int off = 32; off; off >>= 1)
#pragma unroll
      for (int t = 0; t < 4; t++) a[t] = gl_add_lazy(a[t], gl_canon(__shfl_xor(a[t], off)));
    if (lane == 0) {
      uint64_t* o = part + ((uint64_t)tile * n_cols + c) * 4;
#pragma unroll
      for (int t = 0; t < 4; t++) o[t] = gl_canon(a[t]);
    }
  }
}

// One thread per row r of a plane: the tiles' partial sums of column r added, or zero at r >= n_cols.  Writes the four planes.
__global__ __launch_bounds__(256) void k_deep_open(uint32_t tiles, uint32_t n_cols, uint32_t log_r, const uint64_t* __restrict__ part,
                                                   uint64_t* __restrict__ open) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, Rr = 1ull << log_r;
  if (r >= Rr) return;
  uint64_t y[4] = {0, 0, 0, 0};
  if (r < n_cols)
    for (uint32_t t = 0; t < tiles; t++)
#pragma unroll
      for (int k = 0; k < 4; k++) y[k] = gl_add(y[k], part[((uint64_t)t * n_cols + r) * 4 + k]);
#pragma unroll
  for (int k = 0; k < 4; k++) open[k * Rr + r] = y[k];
}

// One workgroup: Y_k = sum_c alpha^c y_(c,k) (opening words taken mod p), and alpha^n_cols.  y[6] = Y_0, Y_1, alpha^n.
constexpr int DEEP_Y_THREADS = 256;
__global__ __launch_bounds__(DEEP_Y_THREADS) void k_deep_y(uint32_t n_cols, uint32_t log_r, const uint64_t* __restrict__ open,
                                                           const uint64_t* __restrict__ apow, const uint64_t* __restrict__ alpha, uint64_t* __restrict__ y) {
  __shared__ uint64_t red[4][DEEP_Y_THREADS];
  const uint32_t t = threadIdx.x;
  const uint64_t Rr = 1ull << log_r;
  gl2 s0 = {0, 0}, s1 = {0, 0};
  for (uint32_t c = t; c < n_cols; c += DEEP_Y_THREADS) {
    const gl2 a = {apow[2 * c], apow[2 * c + 1]};
    s0 = gl2_add(s0, gl2_mul(a, {gl_canon(open[c]), gl_canon(open[Rr + c])}));
    s1 = gl2_add(s1, gl2_mul(a, {gl_canon(open[2 * Rr + c]), gl_canon(open[3 * Rr + c])}));
  }
  red[0][t] = s0.c0; red[1][t] = s0.c1; red[2][t] = s1.c0; red[3][t] = s1.c1;
  for (uint32_t h = DEEP_Y_THREADS / 2; h; h >>= 1) {
    __syncthreads();
    if (t < h)
#pragma unroll
      for (int k = 0; k < 4; k++) red[k][t] = gl_add(red[k][t], red[k][t + h]);
  }
  __syncthreads();
  if (t == 0) {
    const gl2 an = gl2_pow({alpha[0], alpha[1]}, n_cols);
#pragma unroll
    for (int k = 0; k < 4; k++) y[k] = red[k][0];
    y[4] = an.c0;
    y[5] = an.c1;
  }
}

// The batch proof's Y sums: workgroup g adds, over the oracles k of group g, sum_c alpha^(off_k + c) y_(k,c,j) (opening words taken mod p,
// oracle k's planar block at proof + o_off_open[k]); y[6 g ..] = Y_0, Y_1 of the group, then alpha^C (the last entry of the table).
__global__ __launch_bounds__(DEEP_Y_THREADS) void k_batch_y(FriGeom G, const uint64_t* __restrict__ proof, const uint64_t* __restrict__ apow,
                                                            uint64_t* __restrict__ y) {
  __shared__ uint64_t red[4][DEEP_Y_THREADS];
  const uint32_t t = threadIdx.x, g = blockIdx.x;
  gl2 s0 = {0, 0}, s1 = {0, 0};
  for (uint32_t k = 0; k < G.n_oracles; k++) {
    if (G.o_group[k] != g) continue;
    const uint64_t Rr = 1ull << G.o_log_r[k];
    const uint64_t* open = proof + G.o_off_open[k];
    const uint64_t* ap = apow + 2ull * G.o_alpha_off[k];
    for (uint32_t c = t; c < G.o_n_cols[k]; c += DEEP_Y_THREADS) {
      const gl2 a = {ap[2 * c], ap[2 * c + 1]};
      s0 = gl2_add(s0, gl2_mul(a, {gl_canon(open[c]), gl_canon(open[Rr + c])}));
      s1 = gl2_add(s1, gl2_mul(a, {gl_canon(open[2 * Rr + c]), gl_canon(open[3 * Rr + c])}));
    }
  }
  red[0][t] = s0.c0; red[1][t] = s0.c1; red[2][t] = s1.c0; red[3][t] = s1.c1;
  for (uint32_t h = DEEP_Y_THREADS / 2; h; h >>= 1) {
    __syncthreads();
    if (t < h)
#pragma unroll
      for (int k = 0; k < 4; k++) red[k][t] = gl_add(red[k][t], red[k][t + h]);
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < 4; k++) y[6 * g + k] = red[k][0];
    y[6 * g + 4] = apow[2ull * G.total_cols];
    y[6 * g + 5] = apow[2ull * G.total_cols + 1];
  }
}

// One thread per point of D_0: layer 0 (k_fri_combine's output, canonical) rewritten in place into the DEEP quotient.
__global__ __launch_bounds__(256) void k_deep_quotient(uint32_t log_m, uint64_t s, uint64_t w, uint64_t omega_n, const uint64_t* __restrict__ zeta,
                                                       const uint64_t* __restrict__ y, uint64_t* __restrict__ layer) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, M = 1ull << log_m;
  if (i >= M) return;
  const gl2 z0 = {zeta[0], zeta[1]}, z1 = gl2_scale(z0, omega_n);
  const gl2 f = deep_layer0({layer[i], layer[M + i]}, gl_mul(s, gl_pow(w, i)), z0, z1, {y[0], y[1]}, {y[2], y[3]}, {y[4], y[5]});
  layer[i] = f.c0;
  layer[M + i] = f.c1;
}

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

int launch_fri_alpha_powers(uint32_t n_cols, const void* d_alpha, void* d_apow, void* stream) {
  hipLaunchKernelGGL(k_fri_alpha_powers, dim3((n_cols + 255) / 256), dim3(256), 0, S_(stream), n_cols, reinterpret_cast<const uint64_t*>(d_alpha),
                     reinterpret_cast<uint64_t*>(d_apow));
  return (int)hipGetLastError();
}
int launch_fri_combine(uint32_t log_m, uint32_t n_cols, const void* d_cols, const void* d_apow, void* d_out, void* stream) {
  const uint64_t blocks = ((1ull << log_m) + 63) / 64;
  hipLaunchKernelGGL(k_fri_combine<false>, dim3((uint32_t)blocks), dim3(64 * COMBINE_WAVES), 0, S_(stream), log_m, n_cols,
                     reinterpret_cast<const uint64_t*>(d_cols), reinterpret_cast<const uint64_t*>(d_apow), reinterpret_cast<uint64_t*>(d_out));
  return (int)hipGetLastError();
}
int launch_fri_combine_add(uint32_t log_m, uint32_t n_cols, const void* d_cols, const void* d_apow, void* d_out, void* stream) {
  const uint64_t blocks = ((1ull << log_m) + 63) / 64;
  hipLaunchKernelGGL(k_fri_combine<true>, dim3((uint32_t)blocks), dim3(64 * COMBINE_WAVES), 0, S_(stream), log_m, n_cols,
                     reinterpret_cast<const uint64_t*>(d_cols), reinterpret_cast<const uint64_t*>(d_apow), reinterpret_cast<uint64_t*>(d_out));
  return (int)hipGetLastError();
}
int launch_fri_add(uint64_t n_words, const void* d_src, void* d_dst, void* stream) {
  hipLaunchKernelGGL(k_fri_add, dim3((uint32_t)((n_words + 255) / 256)), dim3(256), 0, S_(stream), n_words, reinterpret_cast<const uint64_t*>(d_src),
                     reinterpret_cast<uint64_t*>(d_dst));
  return (int)hipGetLastError();
}
template <bool ADD>
static int fri_fold_launch(uint32_t log_mn, uint32_t bits, uint64_t s_inv, uint64_t w_inv, uint64_t g, const void* d_beta, const void* d_in,
                           const void* d_add, void* d_out, void* stream) {
  const dim3 grid((uint32_t)(((1ull << log_mn) + 255) / 256));
  const uint64_t* beta = reinterpret_cast<const uint64_t*>(d_beta);
  const uint64_t* in = reinterpret_cast<const uint64_t*>(d_in);
  const uint64_t* add = reinterpret_cast<const uint64_t*>(d_add);
  uint64_t* out = reinterpret_cast<uint64_t*>(d_out);
  switch (bits) {
    case 1: hipLaunchKernelGGL((k_fri_fold<1, ADD>), grid, dim3(256), 0, S_(stream), log_mn, s_inv, w_inv, g, beta, in, add, out); break;
    case 2: hipLaunchKernelGGL((k_fri_fold<2, ADD>), grid, dim3(256), 0, S_(stream), log_mn, s_inv, w_inv, g, beta, in, add, out); break;
    case 3: hipLaunchKernelGGL((k_fri_fold<3, ADD>), grid, dim3(256), 0, S_(stream), log_mn, s_inv, w_inv, g, beta, in, add, out); break;
    case 4: hipLaunchKernelGGL((k_fri_fold<4, ADD>), grid, dim3(256), 0, S_(stream), log_mn, s_inv, w_inv, g, beta, in, add, out); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}
int launch_fri_fold(uint32_t log_mn, uint32_t bits, uint64_t s_inv, uint64_t w_inv, uint64_t g, const void* d_beta, const void* d_in, void* d_out,
                    void* stream) {
  return fri_fold_launch<false>(log_mn, bits, s_inv, w_inv, g, d_beta, d_in, nullptr, d_out, stream);
}
int launch_fri_fold_add(uint32_t log_mn, uint32_t bits, uint64_t s_inv, uint64_t w_inv, uint64_t g, const void* d_beta, const void* d_in,
                        const void* d_add, void* d_out, void* stream) {
  return fri_fold_launch<true>(log_mn, bits, s_inv, w_inv, g, d_beta, d_in, d_add, d_out, stream);
}
int launch_fri_final(uint32_t log_m, uint32_t final_log, uint64_t w_inv, uint64_t s_inv, uint64_t m_inv, const void* d_in, void* d_coef, void* d_flag,
                     void* stream) {
  if (log_m > (uint32_t)FINAL_MAX_LOG || final_log > log_m) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fri_final, dim3(1), dim3(FINAL_THREADS), 0, S_(stream), log_m, final_log, w_inv, s_inv, m_inv,
                     reinterpret_cast<const uint64_t*>(d_in), reinterpret_cast<uint64_t*>(d_coef), reinterpret_cast<uint32_t*>(d_flag));
  return (int)hipGetLastError();
}

int launch_deep_weights(uint32_t log_sub, uint64_t s, uint64_t omega_n, uint64_t s_n, uint64_t k_inv, const void* d_zeta, void* d_wt, void* stream) {
  hipLaunchKernelGGL(k_deep_weights, dim3((uint32_t)(((1ull << log_sub) + 255) / 256)), dim3(256), 0, S_(stream), log_sub, s, omega_n, s_n, k_inv,
                     reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<uint64_t*>(d_wt));
  return (int)hipGetLastError();
}
uint64_t deep_eval_tiles(uint32_t log_sub) { return ((1ull << log_sub) + 64 * DEEP_ROWS - 1) / (64 * DEEP_ROWS); }
int launch_deep_eval(uint32_t log_sub, uint32_t log_col, uint32_t stride_log, uint32_t n_cols, const void* d_cols, const void* d_wt, void* d_part,
                     void* stream) {
  // about 4096 waves in all (16 per CU): the columns are split into as many chunks as the row tiles leave room for
  const uint64_t tiles = deep_eval_tiles(log_sub);
  uint64_t chunks = std::min<uint64_t>(n_cols, std::max<uint64_t>(1, 4096 / tiles));
  const uint32_t per = (uint32_t)((n_cols + chunks - 1) / chunks);
  chunks = (n_cols + per - 1) / per;
  hipLaunchKernelGGL(k_deep_eval<DEEP_ROWS>, dim3((uint32_t)tiles, (uint32_t)chunks), dim3(64), 0, S_(stream), log_sub, log_col, stride_log, n_cols, per,
                     reinterpret_cast<const uint64_t*>(d_cols), reinterpret_cast<const uint64_t*>(d_wt), reinterpret_cast<uint64_t*>(d_part));
  return (int)hipGetLastError();
}
int launch_deep_open(uint32_t log_sub, uint32_t n_cols, uint32_t log_r, const void* d_part, void* d_open, void* stream) {
  hipLaunchKernelGGL(k_deep_open, dim3((uint32_t)(((1ull << log_r) + 255) / 256)), dim3(256), 0, S_(stream), (uint32_t)deep_eval_tiles(log_sub), n_cols,
                     log_r, reinterpret_cast<const uint64_t*>(d_part), reinterpret_cast<uint64_t*>(d_open));
  return (int)hipGetLastError();
}
int launch_deep_y(uint32_t n_cols, uint32_t log_r, const void* d_open, const void* d_apow, const void* d_alpha, void* d_y, void* stream) {
  hipLaunchKernelGGL(k_deep_y, dim3(1), dim3(DEEP_Y_THREADS), 0, S_(stream), n_cols, log_r, reinterpret_cast<const uint64_t*>(d_open),
                     reinterpret_cast<const uint64_t*>(d_apow), reinterpret_cast<const uint64_t*>(d_alpha), reinterpret_cast<uint64_t*>(d_y));
  return (int)hipGetLastError();
}
int launch_batch_y(const FriGeom& G, const void* d_proof, const void* d_apow, void* d_y, void* stream) {
  hipLaunchKernelGGL(k_batch_y, dim3(G.n_groups), dim3(DEEP_Y_THREADS), 0, S_(stream), G, reinterpret_cast<const uint64_t*>(d_proof),
                     reinterpret_cast<const uint64_t*>(d_apow), reinterpret_cast<uint64_t*>(d_y));
  return (int)hipGetLastError();
}
int launch_deep_quotient(uint32_t log_m, uint64_t s, uint64_t w, uint64_t omega_n, const void* d_zeta, const void* d_y, void* d_layer, void* stream) {
  hipLaunchKernelGGL(k_deep_quotient, dim3((uint32_t)(((1ull << log_m) + 255) / 256)), dim3(256), 0, S_(stream), log_m, s, w, omega_n,
                     reinterpret_cast<const uint64_t*>(d_zeta), reinterpret_cast<const uint64_t*>(d_y), reinterpret_cast<uint64_t*>(d_layer));
  return (int)hipGetLastError();
}

}  // namespace tmx
