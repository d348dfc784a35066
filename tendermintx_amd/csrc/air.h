// Launch wrappers of the constraint-quotient kernels (air.hip; include/tmx.h "the constraint quotient of the ladder rows").  Host side:
// plain C++, no HIP headers.  gamma itself comes from phase 9 of the lone-lane transcript kernel (poseidon.hip, fri.h).
#pragma once
#include <cstdint>

#include "fri.h"

namespace tmx {

constexpr uint32_t AIR_LADDER_WIDTH = 65, AIR_LADDER_CONSTRAINTS = 33;
// the challenge words of a transcript that draws gamma (FRI_GAMMA_AT lies behind the 64 words the FRI provers keep)
constexpr uint32_t AIR_CHAL_WORDS = 72;

// The tables one quotient launch reads (u64 words at d_tab), all functions of gamma, the domain and the piece's first proof:
//   gpow  [35][2]                gamma^0 .. gamma^33, then gamma^(33 first): the exponent offset of the piece's first proof
//   zinv  [2^log_blowup]         1 / (x_i^N - 1), by i mod 2^log_blowup            (x_i^N = s^N (w^N)^i)
//   sel   [256 << log_blowup]    S(x_i) = x_i^(N/256) - omega_256^-1, by i mod (256 << log_blowup)
constexpr uint32_t AIR_TAB_GPOW = 0, AIR_TAB_ZINV = 72, AIR_TAB_SEL = 136;
inline uint64_t air_table_words(uint32_t log_blowup) { return AIR_TAB_SEL + (256ull << log_blowup); }
// s_n = s^N, w_n = w^N, s_n256 = s^(N/256), w_n256 = w^(N/256), om256_inv = omega_256^-1; gamma at d_gamma (2 words)
int launch_air_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n256, uint64_t w_n256, uint64_t om256_inv,
                      const void* d_gamma, void* d_tab, void* stream);
// The hot pass over the extended ladder columns of n_proofs proofs (d_cols: column 0 of the piece's first proof; 65 columns of 2^log_m
// words per proof): d_quot (planar, 2 << log_m words, canonical) = or += gamma^(33 first) sum_p sum_j gamma^(33 p + j) C_(p,j) / (x^N - 1).
int launch_air_ladder_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_tab, int accumulate,
                               void* d_quot, void* stream);
// The identity at zeta from a batch proof's openings blocks (one workgroup): d_open_t the trace's block (planar, 2^log_r rows per plane,
// 65 n_proofs columns), d_open_q the quotient's (2 rows per plane); log_sub = log2 N; zeta and gamma 2 words each.  A failed identity
// writes 0 to every d_ok[q], q < n_queries; a holding one leaves d_ok as it is.
int launch_air_ladder_check(uint32_t n_proofs, uint32_t log_r, uint32_t log_sub, uint64_t om256_inv, const void* d_open_t, const void* d_open_q,
                            const void* d_zeta, const void* d_gamma, uint32_t n_queries, void* d_ok, void* stream);

}  // namespace tmx
