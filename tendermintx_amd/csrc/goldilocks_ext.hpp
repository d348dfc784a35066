// The quadratic extension F_p^2 = F_p[X] / (X^2 - 7) of the Goldilocks field (fri.hip, poseidon.hip: the FRI challenges and folded values),
// and the fold of one FRI leaf coset, shared by the prover's k_fri_fold and the verifier.  Values are pairs (c0, c1) of canonical words.
#pragma once
#include "goldilocks.hpp"

namespace tmx {

struct gl2 { uint64_t c0, c1; };

constexpr uint64_t GL_INV2 = 0x7fffffff80000001ull;  // (p + 1) / 2

__device__ __forceinline__ gl2 gl2_add(gl2 a, gl2 b) { return {gl_add(a.c0, b.c0), gl_add(a.c1, b.c1)}; }
__device__ __forceinline__ gl2 gl2_sub(gl2 a, gl2 b) { return {gl_sub(a.c0, b.c0), gl_sub(a.c1, b.c1)}; }
__device__ __forceinline__ gl2 gl2_scale(gl2 a, uint64_t s) { return {gl_mul(a.c0, s), gl_mul(a.c1, s)}; }  // by a base-field element
__device__ __forceinline__ gl2 gl2_mul(gl2 a, gl2 b) {  // (a0 b0 + 7 a1 b1, a0 b1 + a1 b0)
  return {gl_add(gl_mul(a.c0, b.c0), gl_mul(gl_mul(a.c1, b.c1), 7)), gl_add(gl_mul(a.c0, b.c1), gl_mul(a.c1, b.c0))};
}
__device__ __forceinline__ bool gl2_eq(gl2 a, gl2 b) { return a.c0 == b.c0 && a.c1 == b.c1; }
__device__ __forceinline__ gl2 gl2_pow(gl2 b, uint64_t e) {
  gl2 r = {1, 0};
  while (e) {
    if (e & 1) r = gl2_mul(r, b);
    b = gl2_mul(b, b);
    e >>= 1;
  }
  return r;
}
// a^-1 = conj(a) / norm(a), norm = a0^2 - 7 a1^2 in F_p: never zero for a != 0 (7 is not a square mod p); one Fermat chain
__device__ __forceinline__ gl2 gl2_inv(gl2 a) {
  const uint64_t n = gl_sub(gl_mul(a.c0, a.c0), gl_mul(gl_mul(a.c1, a.c1), 7));
  const uint64_t ni = gl_pow(n, GL_P - 2);
  return {gl_mul(a.c0, ni), gl_mul(gl_neg(a.c1), ni)};
}
// DEEP layer 0 at a point x of D_0 (include/tmx.h "out-of-domain openings"): (F - Y_0) / (x - z_0) + alpha^n (F - Y_1) / (x - z_1);
// z_0, z_1 lie outside F_p, so x - z_k is never zero.  Shared by k_deep_quotient and the verifier.
__device__ __forceinline__ gl2 deep_layer0(gl2 F, uint64_t x, gl2 z0, gl2 z1, gl2 Y0, gl2 Y1, gl2 alpha_n) {
  const gl2 q0 = gl2_mul(gl2_sub(F, Y0), gl2_inv({gl_sub(x, z0.c0), gl_neg(z0.c1)}));
  const gl2 q1 = gl2_mul(gl2_sub(F, Y1), gl2_inv({gl_sub(x, z1.c0), gl_neg(z1.c1)}));
  return gl2_add(q0, gl2_mul(alpha_n, q1));
}

// One leaf of a FRI layer: v[j] = f(x_j) at the a = 2^B points x_j = s w^(r + j M'), M' = M / a, of a domain of M points (canonical values).
// On return v[0] = f_next(x_0^a) after B radix-2 folds with beta, beta^2, ...: fold t pairs j with j + h (h = a >> (t + 1): x_(j + h) = -x_j)
// into (f(x) + f(-x)) / 2 + beta (f(x) - f(-x)) / (2 x).  x_j^-1 comes from xinv0 = (s w^r)^-1 and g = w^-M' (x_j^-1 = xinv0 g^j); the next
// fold's points are the squares, and so are their inverses -- no inversion on the device.
template <int B>
__device__ __forceinline__ gl2 fri_fold_leaf(gl2 (&v)[1 << B], uint64_t xinv0, uint64_t g, gl2 beta) {
  constexpr int A = 1 << B;
  uint64_t xi[A / 2 > 0 ? A / 2 : 1];
  xi[0] = xinv0;
#pragma unroll
  for (int j = 1; j < A / 2; j++) xi[j] = gl_mul(xi[j - 1], g);
#pragma unroll
  for (int t = 0; t < B; t++) {
    const int h = A >> (t + 1);
#pragma unroll
    for (int j = 0; j < h; j++) {
      const gl2 s = gl2_add(v[j], v[j + h]), d = gl2_sub(v[j], v[j + h]);
      v[j] = gl2_scale(gl2_add(s, gl2_scale(gl2_mul(beta, d), xi[j])), GL_INV2);
    }
#pragma unroll
    for (int j = 0; j < h / 2; j++) xi[j] = gl_mul(xi[j], xi[j]);
    beta = gl2_mul(beta, beta);
  }
  return v[0];
}

}  // namespace tmx
