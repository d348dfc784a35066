// The field-only kernels of the batched FRI proof (include/tmx.h "a batched FRI low-degree proof"): the batching pass over the committed
// columns, the folds between layers and the final polynomial.  The kernels that need the Poseidon permutation (transcript, verifier) sit
// beside it in poseidon.hip.  Goldilocks words, F_p^2 = F_p[X] / (X^2 - 7) values (goldilocks_ext.hpp); no MFMA (nothing is a contraction).
#include <hip/hip_runtime.h>

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
constexpr int COMBINE_WAVES = 4, COMBINE_UNROLL = 8;
__global__ __launch_bounds__(64 * COMBINE_WAVES) void k_fri_combine(uint32_t log_m, uint32_t n_cols, const uint64_t* __restrict__ cols,
                                                                    const uint64_t* __restrict__ apow, uint64_t* __restrict__ out) {
  __shared__ uint64_t part[COMBINE_WAVES - 1][2][64];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t M = 1ull << log_m, row = (uint64_t)blockIdx.x * 64 + lane;
  const uint32_t chunk = (n_cols + COMBINE_WAVES - 1) / COMBINE_WAVES;
  const uint32_t c_lo = min(n_cols, wave * chunk), c_hi = min(n_cols, c_lo + chunk);
  uint64_t a0 = 0, a1 = 0;
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
    out[row] = a0;
    out[M + row] = a1;
  }
}

// One thread per leaf coset r < M' of layer l (M' = M_(l+1)): its 2^B values in registers, B radix-2 folds (fri_fold_leaf), one value of
// layer l + 1 out.  x_0^-1 = s^-1 (w^-1)^r: one exponentiation per thread.
template <int B>
__global__ __launch_bounds__(256) void k_fri_fold(uint32_t log_mn, uint64_t s_inv, uint64_t w_inv, uint64_t g, const uint64_t* __restrict__ beta,
                                                  const uint64_t* __restrict__ in, uint64_t* __restrict__ out) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, Mn = 1ull << log_mn, M = Mn << B;
  if (r >= Mn) return;
  gl2 v[1 << B];
#pragma unroll
  for (int j = 0; j < (1 << B); j++) v[j] = {in[r + j * Mn], in[M + r + j * Mn]};
  const gl2 f = fri_fold_leaf<B>(v, gl_mul(s_inv, gl_pow(w_inv, r)), g, {beta[0], beta[1]});
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

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

int launch_fri_alpha_powers(uint32_t n_cols, const void* d_alpha, void* d_apow, void* stream) {
  hipLaunchKernelGGL(k_fri_alpha_powers, dim3((n_cols + 255) / 256), dim3(256), 0, S_(stream), n_cols, reinterpret_cast<const uint64_t*>(d_alpha),
                     reinterpret_cast<uint64_t*>(d_apow));
  return (int)hipGetLastError();
}
int launch_fri_combine(uint32_t log_m, uint32_t n_cols, const void* d_cols, const void* d_apow, void* d_out, void* stream) {
  const uint64_t blocks = ((1ull << log_m) + 63) / 64;
  hipLaunchKernelGGL(k_fri_combine, dim3((uint32_t)blocks), dim3(64 * COMBINE_WAVES), 0, S_(stream), log_m, n_cols,
                     reinterpret_cast<const uint64_t*>(d_cols), reinterpret_cast<const uint64_t*>(d_apow), reinterpret_cast<uint64_t*>(d_out));
  return (int)hipGetLastError();
}
int launch_fri_fold(uint32_t log_mn, uint32_t bits, uint64_t s_inv, uint64_t w_inv, uint64_t g, const void* d_beta, const void* d_in, void* d_out,
                    void* stream) {
  const dim3 grid((uint32_t)(((1ull << log_mn) + 255) / 256));
  const uint64_t* beta = reinterpret_cast<const uint64_t*>(d_beta);
  const uint64_t* in = reinterpret_cast<const uint64_t*>(d_in);
  uint64_t* out = reinterpret_cast<uint64_t*>(d_out);
  switch (bits) {
    case 1: hipLaunchKernelGGL(k_fri_fold<1>, grid, dim3(256), 0, S_(stream), log_mn, s_inv, w_inv, g, beta, in, out); break;
    case 2: hipLaunchKernelGGL(k_fri_fold<2>, grid, dim3(256), 0, S_(stream), log_mn, s_inv, w_inv, g, beta, in, out); break;
    case 3: hipLaunchKernelGGL(k_fri_fold<3>, grid, dim3(256), 0, S_(stream), log_mn, s_inv, w_inv, g, beta, in, out); break;
    case 4: hipLaunchKernelGGL(k_fri_fold<4>, grid, dim3(256), 0, S_(stream), log_mn, s_inv, w_inv, g, beta, in, out); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}
int launch_fri_final(uint32_t log_m, uint32_t final_log, uint64_t w_inv, uint64_t s_inv, uint64_t m_inv, const void* d_in, void* d_coef, void* d_flag,
                     void* stream) {
  if (log_m > (uint32_t)FINAL_MAX_LOG || final_log > log_m) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fri_final, dim3(1), dim3(FINAL_THREADS), 0, S_(stream), log_m, final_log, w_inv, s_inv, m_inv,
                     reinterpret_cast<const uint64_t*>(d_in), reinterpret_cast<uint64_t*>(d_coef), reinterpret_cast<uint32_t*>(d_flag));
  return (int)hipGetLastError();
}

}  // namespace tmx
