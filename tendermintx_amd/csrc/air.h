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

// ---- constraint set 2: set 1 plus the boundary constraints against a public table (include/tmx.h "the boundary constraints of the ladder
// rows").  65 constraints per proof; gamma comes from phase 10 of the transcript kernel (the public digest observed behind the trace cap).
constexpr uint32_t AIR_BOUNDARY_CONSTRAINTS = 65, AIR_PUBLIC_WIDTH = 17, AIR_PUBLIC_MAX_LOG_K = 12;
// The tables one set-2 quotient launch reads (u64 words at d_tab; a layout of its own, set 1's stays as it is):
//   gpow  [68][2]                gamma^0 .. gamma^66, then gamma^(65 first)
//   zinv  [2^log_blowup]         1 / (x_i^N - 1), by i mod 2^log_blowup
//   sel   [256 << log_blowup]    S(x_i), by i mod (256 << log_blowup)
//   sinv  [256 << log_blowup]    1 / S(x_i), same period (x_i^K = s^K (w^K)^i, w^K of order 256 B)
constexpr uint32_t AIR2_TAB_GPOW = 0, AIR2_TAB_ZINV = 136, AIR2_TAB_SEL = 200, AIR2_TAB_SINV = AIR2_TAB_SEL + (256u << 6);
constexpr uint64_t AIR2_TAB_WORDS = AIR2_TAB_SINV + (256u << 6);
int launch_air_boundary_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n256, uint64_t w_n256,
                               uint64_t om256_inv, const void* d_gamma, void* d_tab, void* stream);
// pub (column-major, 17 n_proofs columns of 2^log_k words) from the element rows: row p's lane i has its D.1b words at
// d_rows + p elem_stride + d1b_start + i lane_elems, the sixteen words of sB then hA at point_off within them
int launch_air_public_gather(const void* d_rows, uint64_t elem_stride, uint32_t d1b_start, uint32_t lane_elems, uint32_t point_off, uint32_t n_max,
                             uint32_t log_k, uint32_t n_proofs, void* d_pub, void* stream);
// d_v[2 k], d_v[2 k + 1] = V_k (k < 2^log_k) from pub and gamma (2 words at d_gamma)
int launch_air_public_combine(uint32_t log_k, uint32_t n_proofs, const void* d_pub, const void* d_gamma, void* d_v, void* stream);
// the twiddles of the size-K transforms: d_tw[e] = om_k^e, d_tw[K/2 + e] = om_k^-e, e < K/2
int launch_air_public_twiddles(uint32_t log_k, uint64_t om_k, void* d_tw, void* stream);
// the coefficients of Pub_gamma (planar, 2 K words at d_coef) from V: a size-K inverse transform, then c_j = d_j om255_inv^j / K
int launch_air_public_coefs(uint32_t log_k, uint64_t k_inv, uint64_t om255_inv, const void* d_v, const void* d_tw, void* d_coef, void* stream);
// Pub_gamma on the M = 2^log_m points x_i = s w^i (planar, 2 M words at d_ext): workgroup a < M / K scales the coefficients by x_a^j and runs
// a size-K transform of both planes in LDS; point a + (M / K) b receives output b
int launch_air_public_extend(uint32_t log_m, uint32_t log_k, uint64_t s, uint64_t w, const void* d_coef, const void* d_tw, void* d_ext, void* stream);
// The set-2 hot pass; d_pubext = null: a piece that does not carry the public term
int launch_air_ladder_boundary_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_tab,
                                        const void* d_pubext, int accumulate, void* d_quot, void* stream);
// The set-2 identity at zeta (one workgroup), with Pub_gamma(zeta) barycentric over the K points y_k = om255 om_k^k from d_v
int launch_air_ladder_boundary_check(uint32_t n_proofs, uint32_t log_r, uint32_t log_sub, uint64_t om256_inv, uint64_t om255, uint64_t om_k,
                                     uint64_t bary_inv, const void* d_open_t, const void* d_open_q, const void* d_zeta, const void* d_gamma,
                                     const void* d_v, uint32_t n_queries, void* d_ok, void* stream);

// ---- constraint set 3: the round constraints of the SHA-256 tables (include/tmx.h "the round constraints of the SHA-256 tables").  A table
// of 9 columns per proof, a helper oracle of 300 columns per proof (bits), 315 constraints per proof; gamma comes from a lone-lane transcript
// kernel of its own (poseidon.hip k_air_sha_gamma: k_fri_transcript stays as it is).
constexpr uint32_t AIR_SHA_WIDTH = 9, AIR_SHA_HELPER_COLS = 300, AIR_SHA_CONSTRAINTS = 315;
// The tables one set-3 quotient launch reads (u64 words at d_tab; they fit the table part of set 1's scratch):
//   gpow  [317][2]               gamma^0 .. gamma^315, then gamma^(315 first): the exponent offset of a piece's first proof
//   zinv  [2^log_blowup]         1 / (x_i^N - 1), by i mod 2^log_blowup
//   sel   [64 << log_blowup]     S(x_i) = x_i^(N/64) - omega_64^-1, by i mod (64 << log_blowup)
//   kx    [64 << log_blowup]     K(x_i) = P_K(x_i^(N/64)), same period
constexpr uint32_t AIR3_TAB_GPOW = 0, AIR3_TAB_ZINV = 640, AIR3_TAB_SEL = 704, AIR3_TAB_K = AIR3_TAB_SEL + (64u << 6);
constexpr uint64_t AIR3_TAB_WORDS = AIR3_TAB_K + (64u << 6);
static_assert(2 * (AIR_SHA_CONSTRAINTS + 2) <= AIR3_TAB_ZINV && AIR3_TAB_WORDS <= AIR_TAB_SEL + (256ull << 6), "the set-3 tables live in the table part of set 1's scratch");
// gamma of set 3 (one lane): 2^33, obs[0 .. 5) = {3, log_n, log_blowup, cap_height, n_proofs}, cap_words words at d_cap, cap_words words
// at d_cap_helper; the duplex is left at d_state (32 words), gamma at d_chal[FRI_GAMMA_AT]
int launch_air_sha_gamma(const void* d_consts, int mode, const uint32_t obs[5], uint32_t cap_words, const void* d_cap, const void* d_cap_helper,
                         void* d_state, void* d_chal, void* stream);
// The helper oracle from pre-LDE columns: one lane per (proof, row); d_table 9 n_proofs columns of 2^log_rows words, d_helper 300 n_proofs
int launch_air_sha_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream);
// s_n = s^N, w_n = w^N, s_n64 = s^(N/64), w_n64 = w^(N/64), om64_inv = omega_64^-1; gamma at d_gamma (2 words); first_proof = 0 for a whole table
int launch_air_sha_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n64, uint64_t w_n64, uint64_t om64_inv, const void* d_gamma,
                          void* d_tab, void* stream);
// The hot pass: d_quot (planar, 2 << log_m words, canonical) = sum_p sum_j gamma^(315 p + j) C_(p,j) / (x^N - 1)
// form, for this pass and its siblings of sets 4 and 5: AIR_FORM_WHOLE is the whole table.  A piece is n_proofs whole proofs whose first is
// proof `first` of the table (the tables' first_proof): d_cols is that proof's table column 0, d_helper_cols the piece's own helper buffer
// (its first column at offset 0), and d_quot = (AIR_FORM_PIECE) or += (AIR_FORM_PIECE_ACC) gamma^(C first) times the sum over the piece.
constexpr int AIR_FORM_WHOLE = 0, AIR_FORM_PIECE = 1, AIR_FORM_PIECE_ACC = 2;
int launch_air_sha_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_helper_cols, const void* d_tab,
                            int form, void* d_quot, void* stream);
// The identity at zeta from the openings blocks of the table (2^log_r_t rows per plane), the helper (2^log_r_h) and the quotient
int launch_air_sha_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint64_t om64_inv, const void* d_open_t,
                         const void* d_open_h, const void* d_open_q, const void* d_zeta, const void* d_gamma, uint32_t n_queries, void* d_ok,
                         void* stream);

// ---- constraint set 4: the message schedule of the SHA-256 tables (include/tmx.h "the message schedule of the SHA-256 tables").  The same
// table, a helper oracle of 115 columns per proof, 117 constraints per proof; gamma comes from set 3's lone-lane kernel with the set id 4 in
// obs[0] (launch_air_sha_gamma: the kernel is the same code object, so neither it nor k_fri_transcript changes).
constexpr uint32_t AIR_SCHED_HELPER_COLS = 115, AIR_SCHED_CONSTRAINTS = 117;
// The tables one set-4 quotient launch reads (u64 words at d_tab; they fit the table part of set 1's scratch):
//   gpow  [119][2]               gamma^0 .. gamma^117, then gamma^(117 first)
//   zinv  [2^log_blowup]         1 / (x_i^N - 1), by i mod 2^log_blowup
//   fx    [64 << log_blowup]     F(x_i) = P_F(x_i^(N/64)), by i mod (64 << log_blowup)
constexpr uint32_t AIR4_TAB_GPOW = 0, AIR4_TAB_ZINV = 256, AIR4_TAB_F = 320;
constexpr uint64_t AIR4_TAB_WORDS = AIR4_TAB_F + (64u << 6);
static_assert(2 * (AIR_SCHED_CONSTRAINTS + 2) <= AIR4_TAB_ZINV && AIR4_TAB_WORDS <= AIR_TAB_SEL + (256ull << 6),
              "the set-4 tables live in the table part of set 1's scratch");
// The helper oracle from pre-LDE columns: one lane per (proof, row); d_table 9 n_proofs columns of 2^log_rows words, d_helper 115 n_proofs
int launch_air_sched_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream);
// s_n = s^N, w_n = w^N, s_n64 = s^(N/64), w_n64 = w^(N/64), om64_inv = omega_64^-1; gamma at d_gamma (2 words)
int launch_air_sched_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n64, uint64_t w_n64, uint64_t om64_inv, const void* d_gamma,
                            void* d_tab, void* stream);
// The hot pass: d_quot (planar, 2 << log_m words, canonical) = sum_p sum_j gamma^(117 p + j) C_(p,j) / (x^N - 1)
int launch_air_sched_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_helper_cols,
                              const void* d_tab, int form, void* d_quot, void* stream);
// The identity at zeta from the openings blocks of the table (2^log_r_t rows per plane), the helper (2^log_r_h) and the quotient
int launch_air_sched_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint64_t om64_inv, const void* d_open_t,
                           const void* d_open_h, const void* d_open_q, const void* d_zeta, const void* d_gamma, uint32_t n_queries, void* d_ok,
                           void* stream);

// ---- constraint set 5: the block starts of the SHA-256 tables (include/tmx.h "the block starts of the SHA-256 tables").  The same table, a
// helper oracle of 315 columns per proof, 337 constraints per proof, a mode chain in {0, 1}; gamma comes from set 3's lone-lane kernel with
// 5 | chain << 8 in obs[0] (launch_air_sha_gamma: the same code object, so neither it nor k_fri_transcript changes).
constexpr uint32_t AIR_INIT_HELPER_COLS = 315, AIR_INIT_CONSTRAINTS = 337;
// The tables one set-5 quotient launch reads (u64 words at d_tab; they fit the table part of set 1's scratch):
//   gpow  [339][2]               gamma^0 .. gamma^337, then gamma^(337 first)
//   zinv  [2^log_blowup]         1 / (x_i^N - 1), by i mod 2^log_blowup
//   sel   [64 << log_blowup]     chain = 0: 1 / D_s(x_i), D_s = x^(N/64) - omega_64^-1, by i mod (64 << log_blowup)
//         [128 << log_blowup]    chain = 1: 1 / D_s(x_i), D_s = x^(N/128) - omega_128^-1, by i mod (128 << log_blowup); 1 / D_c(x_i), D_c =
//                                x^(N/128) + omega_128^-1, is the negated entry (64 << log_blowup) places on
constexpr uint32_t AIR5_TAB_GPOW = 0, AIR5_TAB_ZINV = 704, AIR5_TAB_SEL = 768;
constexpr uint64_t AIR5_TAB_WORDS = AIR5_TAB_SEL + (128u << 6);
static_assert(2 * (AIR_INIT_CONSTRAINTS + 2) <= AIR5_TAB_ZINV && AIR5_TAB_WORDS <= AIR_TAB_SEL + (256ull << 6),
              "the set-5 tables live in the table part of set 1's scratch");
// The helper oracle from pre-LDE columns: one lane per (proof, row); d_table 9 n_proofs columns of 2^log_rows words, d_helper 315 n_proofs
int launch_air_init_helper(uint32_t log_rows, uint32_t n_proofs, uint32_t chain, const void* d_table, void* d_helper, void* stream);
// s_n = s^N, w_n = w^N; s_sel = s^(N/64), w_sel = w^(N/64), rho = omega_64^-1 under chain = 0; s^(N/128), w^(N/128), omega_128^-1 under
// chain = 1; gamma at d_gamma (2 words)
int launch_air_init_tables(uint32_t log_blowup, uint32_t chain, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_sel, uint64_t w_sel, uint64_t rho,
                           const void* d_gamma, void* d_tab, void* stream);
// The hot pass: d_quot (planar, 2 << log_m words, canonical) = sum_p (sum_(j < 321) gamma^(337 p + j) C_(p,j) / (x^N - 1)
// + sum_(321 <= j < 329) gamma^(337 p + j) L_(p,j) / D_s + sum_(j >= 329) gamma^(337 p + j) L_(p,j) / D_c)
int launch_air_init_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, uint32_t chain, const void* d_cols, const void* d_helper_cols,
                             const void* d_tab, int form, void* d_quot, void* stream);
// The division-free identity at zeta from the openings blocks of the table (2^log_r_t rows per plane), the helper (2^log_r_h) and the quotient
int launch_air_init_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint32_t chain, uint64_t rho,
                          const void* d_open_t, const void* d_open_h, const void* d_open_q, const void* d_zeta, const void* d_gamma,
                          uint32_t n_queries, void* d_ok, void* stream);

// ---- constraint set 6: the SHA-256 tables' link to Level-1 (include/tmx.h "the SHA-256 tables' link to Level-1").  The same table, a public
// table of 26 columns per proof on the table's blocks, a helper oracle of 33 columns per proof, 50 constraints per proof.
constexpr uint32_t AIR_SHA_PUBLIC_WIDTH = 26, AIR_LINK_HELPER_COLS = 33, AIR_LINK_CONSTRAINTS = 50;
constexpr uint32_t AIR_SHA_PUBLIC_MIN_LOG_K = 1, AIR_SHA_PUBLIC_MAX_LOG_K = 12;
// Where the gather reads in an element row (docs/witness_layout.md): the first elements of H.2 (ValidatorVariable[N]), H.3 (nb, round, the
// proof structs), H.4 (skip: ValidatorHashFieldVariable[N]), D.1a, D.2a (skip), D.3, D.4 (skip) and D.5; section = TMX_TRACE_SHA256, _TREE
// or _HEADER; n = the context's n_max, tn = the slots of its fixed-shape tree
// Every offset below is recorded by build_program (api.cpp) while it emits the serializer's table, so a layout change is made there alone:
//   h2_lane, h2_vlen   a ValidatorVariable's elements and where its validator_byte_length stands; h4_lane, h4_vlen likewise for H.4
//   cid_len, cid, h_len   inside H.3: the encoded chain-id length, the 52 chain-id bytes, the encoded height length
//   aunts[q], leaf[q]  inside H.3: the four aunts of header proof q and its leaf bytes (q >= 2; leaf_bytes[q] of them)
//   d1a_lane, d2a_lane, lane_leaf   a lane's elements in D.1a / D.2a (the marshalled validator first) and where its leaf hash stands
//   d5_proof[q], d5_hleaf   inside D.5: leaf hash and four path nodes of proof q, and the height leaf 00 08 varint9
struct AirShaPublicGeom {
  uint64_t elem_stride;
  uint32_t kind, section, n, tn;
  uint32_t h2, h3, h4, d1a, d2a, d3, d4, d5;
  uint32_t h2_lane, h2_vlen, h4_lane, h4_vlen, cid_len, cid, h_len, aunts[5], leaf[5], leaf_bytes[5];
  uint32_t d1a_lane, d2a_lane, lane_leaf, d5_proof[5], d5_hleaf;
};
// The public table from element rows: one lane per (proof, block); d_pub 26 n_proofs columns of 2^log_k words
int launch_air_sha_public_gather(const void* d_rows, const AirShaPublicGeom& G, uint32_t log_k, uint32_t n_proofs, void* d_pub, void* stream);
// The helper oracle from pre-LDE columns and the public flags: one lane per (proof, row); d_table 9 n_proofs columns of 2^log_rows words,
// d_pub 26 n_proofs columns of 2^(log_rows - 6), d_helper 33 n_proofs columns of 2^log_rows
int launch_air_link_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, const void* d_pub, void* d_helper, void* stream);
// gamma of set 6: set 3's lone-lane form as a kernel of its own (poseidon.hip k_air_link_gamma; k_air_sha_gamma and k_fri_transcript stay
// as they are): a fresh duplex over 2^33, obs (6, log_n, log_blowup, cap_height, n_proofs), the table cap, the helper cap (cap_words each),
// the four words of the public digest
int launch_air_link_gamma(const void* d_consts, int mode, const uint32_t obs[5], uint32_t cap_words, const void* d_cap, const void* d_cap_helper,
                          const void* d_digest, void* d_state, void* d_chal, void* stream);
// The tables one set-6 quotient launch reads (u64 words at d_tab, in the set's own scratch); per = i mod (64 << log_blowup):
//   gpow  [52][2]   gamma^0 .. gamma^50, then gamma^(50 first)          zinv  [2^log_blowup]   1 / (x_i^N - 1), by i mod 2^log_blowup
//   s, sinv [per]   S(x_i) = x_i^K - omega_64^-1 and its inverse         dsum  [per]            sum_(t < 16) 1 / D_t(x_i)
//   dinv  [16][AIR6_PER_MAX]   1 / D_t(x_i), D_t = x^K - omega_64^t (the fold of the public side reads them; the pass reads dsum)
constexpr uint32_t AIR6_PER_MAX = 64u << 6;
constexpr uint32_t AIR6_TAB_GPOW = 0, AIR6_TAB_ZINV = 128, AIR6_TAB_S = 192, AIR6_TAB_SINV = AIR6_TAB_S + AIR6_PER_MAX,
                   AIR6_TAB_DSUM = AIR6_TAB_SINV + AIR6_PER_MAX, AIR6_TAB_DINV = AIR6_TAB_DSUM + AIR6_PER_MAX;
constexpr uint64_t AIR6_TAB_WORDS = AIR6_TAB_DINV + 16ull * AIR6_PER_MAX;
static_assert(2 * (AIR_LINK_CONSTRAINTS + 2) <= AIR6_TAB_ZINV, "gamma^0 .. gamma^51 in front of zinv");
// s_n = s^N, w_n = w^N, s_k = s^K, w_k = w^K (K = N / 64), om64 = omega_64; gamma at d_gamma (2 words)
int launch_air_link_tables(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_k, uint64_t w_k, uint64_t om64,
                           const void* d_gamma, void* d_tab, void* stream);
// The seventeen value vectors under gamma, one lane per (vector, block k): d_v [17][K][2] words, V63 first, then V^0 .. V^15
int launch_air_link_combine(uint32_t log_k, uint32_t n_proofs, const void* d_pub, const void* d_gamma, void* d_v, void* stream);
// d_pq (planar, 2 << log_m) = (first ? 0 : d_pq) + d_ext / divisor: which = 0 divides by S, 1 + t by D_t (tables at d_tab)
int launch_air_link_fold(uint32_t log_m, uint32_t log_blowup, uint32_t which, int first, const void* d_ext, const void* d_tab, void* d_pq, void* stream);
// The hot pass: d_quot (planar, 2 << log_m words, canonical) = sum_p [sum_(j < 32) gamma^(50 p + j) C_(p,j) / (x^N - 1) + sum_(32 <= j < 49)
// gamma^(50 p + j) L_(p,j) / S + gamma^(50 p + 49) W_p sum_t 1 / D_t] - PQ; d_pq null: a piece that does not start at proof 0
int launch_air_link_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_helper_cols,
                             const void* d_tab, const void* d_pq, int form, void* d_quot, void* stream);
// The identity at zeta from the openings blocks of the table (2^log_r_t rows per plane), the helper (2^log_r_h) and the quotient, with the
// seventeen public polynomials barycentric from the verifier's own d_v; om = omega_N, om_k = omega_N^64, k_inv = 1 / K
int launch_air_link_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint64_t om64, uint64_t om, uint64_t om_k,
                          uint64_t k_inv, const void* d_open_t, const void* d_open_h, const void* d_open_q, const void* d_zeta,
                          const void* d_gamma, const void* d_v, uint32_t n_queries, void* d_ok, void* stream);

// ---- constraint sets 7, 8 and 9: the SHA-512 table (include/tmx.h "the round constraints of the SHA-512 table", "the message schedule of
// the SHA-512 table", "the block starts of the SHA-512 table").  A table of 18 columns per proof (T.2: nine 64-bit words as lo, hi) and per
// set a helper oracle and a constraint count:
//   set 7, the round function   599 helper columns, 628 constraints
//   set 8, the message schedule 230 helper columns (set 4's 115 twice: lo / hi limbs), 234 constraints
//   set 9, the block starts     629 helper columns (set 5's 315 in lo / hi limbs), 673 constraints
// gamma comes from set 3's lone-lane kernel with the set id in obs[0] (launch_air_sha_gamma: the same code object).  The blocks are 80 rows
// (set 9: lanes of 160 with a wrap row of their own), which no power-of-two subgroup fits, so the selectors and set 7's round constants are
// preprocessed columns of full degree: SEL, KLO, KHI (set 7), SCH "the next row is a schedule row" (set 8), STA "the next row starts a
// hash" and CHN "the next row starts a second block" (set 9).  The prover fills and extends them like helper columns, the verifier
// evaluates them at zeta barycentrically over the N rows.
constexpr uint32_t AIR_SHA512_WIDTH = 18, AIR_SHA512_HELPER_COLS = 599, AIR_SHA512_CONSTRAINTS = 628;
constexpr uint32_t AIR_SHA512_SCHED_HELPER_COLS = 230, AIR_SHA512_SCHED_CONSTRAINTS = 234;
constexpr uint32_t AIR_SHA512_INIT_HELPER_COLS = 629, AIR_SHA512_INIT_CONSTRAINTS = 673;
// The tables one quotient launch of a set reads (u64 words at d_tab; they fit the table part of set 1's scratch), n its constraint count:
//   gpow  [n + 2][2]             gamma^0 .. gamma^n, then gamma^(n first)
//   zinv  [2^log_blowup]         1 / (x_i^N - 1), by i mod 2^log_blowup
constexpr uint32_t AIR7_TAB_GPOW = 0, AIR7_TAB_ZINV = 1280, AIR8_TAB_GPOW = 0, AIR8_TAB_ZINV = 512, AIR9_TAB_GPOW = 0, AIR9_TAB_ZINV = 1408;
constexpr uint64_t AIR7_TAB_WORDS = AIR7_TAB_ZINV + 64, AIR8_TAB_WORDS = AIR8_TAB_ZINV + 64, AIR9_TAB_WORDS = AIR9_TAB_ZINV + 64;
static_assert(2 * (AIR_SHA512_CONSTRAINTS + 2) <= AIR7_TAB_ZINV && AIR7_TAB_WORDS <= AIR_TAB_SEL + (256ull << 6),
              "the set-7 tables live in the table part of set 1's scratch");
static_assert(2 * (AIR_SHA512_SCHED_CONSTRAINTS + 2) <= AIR8_TAB_ZINV && AIR8_TAB_WORDS <= AIR_TAB_SEL + (256ull << 6),
              "the set-8 tables live in the table part of set 1's scratch");
static_assert(2 * (AIR_SHA512_INIT_CONSTRAINTS + 2) <= AIR9_TAB_ZINV && AIR9_TAB_WORDS <= AIR_TAB_SEL + (256ull << 6),
              "the set-9 tables live in the table part of set 1's scratch");
// The barycentric kernel's output: one row of AIR*_PART_WORDS words per workgroup (two words of sum per plane, a zero-denominator flag, the
// rest unused), 1024 rows of the table per workgroup, at most AIR7_MAX_PARTS workgroups
constexpr uint32_t AIR7_PART_WORDS = 8, AIR8_PART_WORDS = 4, AIR9_PART_WORDS = 8, AIR7_MAX_PARTS = 64;
inline uint32_t air_sha512_eval_parts(uint32_t log_rows) {
  const uint32_t n = log_rows > 10 ? 1u << (log_rows - 10) : 1u;
  return n < AIR7_MAX_PARTS ? n : AIR7_MAX_PARTS;
}
// The helper oracles from pre-LDE columns: one lane per (proof, row); d_table 18 n_proofs columns of 2^log_rows words, d_helper 599 / 230 /
// 629 n_proofs
int launch_air_sha512_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream);
int launch_air_sha512_sched_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream);
int launch_air_sha512_init_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, void* d_helper, void* stream);
// Every other launch is the same code for the three sets, instantiated per set: one table of launchers each.  `planes` below is 3, 1, 2.
struct AirSha512Launch {
  // The planes before the LDE (planar, planes << log_rows words at d_pre): one lane per row
  int (*fill)(uint32_t log_rows, void* d_pre, void* stream);
  // s_n = s^N, w_n = w^N; gamma at d_gamma (2 words); first_proof = 0 for a whole table
  int (*tables)(uint32_t log_blowup, uint64_t first_proof, uint64_t s_n, uint64_t w_n, const void* d_gamma, void* d_tab, void* stream);
  // The hot pass: d_quot (planar, 2 << log_m words, canonical) = sum_p sum_j gamma^(n p + j) C_(p,j) / (x^N - 1); d_pre the extended
  // preprocessed planes (planes << log_m words); form as in launch_air_sha_quotient
  int (*quotient)(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, const void* d_cols, const void* d_helper_cols, const void* d_pre,
                  const void* d_tab, int form, void* d_quot, void* stream);
  // The barycentric sums of the planes at zeta (2 words at d_zeta) over the N = 2^log_rows rows, om = omega_N: air_sha512_eval_parts(log_rows)
  // rows at d_part
  int (*eval)(uint32_t log_rows, uint64_t om, const void* d_zeta, void* d_part, void* stream);
  // d_out[0 .. 2 planes) = the planes at zeta, d_out[2 planes] = 1 if a denominator was zero; n_inv = 1 / N
  int (*fold)(uint32_t log_rows, uint64_t n_inv, const void* d_part, const void* d_zeta, void* d_out, void* stream);
  // The identity at zeta from the openings blocks of the table (2^log_r_t rows per plane), the helper (2^log_r_h) and the quotient, with the
  // planes at zeta from the barycentric kernel's rows at d_part
  int (*check)(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint64_t n_inv, const void* d_part, const void* d_open_t,
               const void* d_open_h, const void* d_open_q, const void* d_zeta, const void* d_gamma, uint32_t n_queries, void* d_ok, void* stream);
};
const AirSha512Launch* air_sha512_launch(uint32_t set);  // set = 7, 8, 9 or 10

// ---- constraint set 10: the SHA-512 table's link to Level-1 (include/tmx.h "the SHA-512 table's link to Level-1").  The same table, a public
// table of 49 columns per proof on the table's block slots (slot k = rows 80 k .. 80 k + 79, the partial last slot included), a helper
// oracle of 65 columns per proof, 115 constraints per proof, five preprocessed planes (STA, CHN, SEL, E79, MSG) behind the descriptor of sets
// 7 - 9 (air_sha512_launch(10): fill, tables, quotient, eval and fold; its check is the one below, which knows the public side).  gamma is set
// 6's rule with the set id 10 (launch_air_link_gamma).  All public terms enter linearly: under gamma they are ONE F_p^2 value V_r per row.
constexpr uint32_t AIR_SHA512_PUBLIC_WIDTH = 49, AIR_SHA512_LINK_HELPER_COLS = 65, AIR_SHA512_LINK_CONSTRAINTS = 115;
// The tables of a quotient launch (sets 7 - 9's layout) and the rows of the two barycentric kernels: the planes' (five sums and a flag) and
// the public side's (one sum and a flag)
constexpr uint32_t AIR10_TAB_GPOW = 0, AIR10_TAB_ZINV = 256, AIR10_PART_WORDS = 16, AIR10_PUB_PART_WORDS = 4;
constexpr uint64_t AIR10_TAB_WORDS = AIR10_TAB_ZINV + 64;
static_assert(2 * (AIR_SHA512_LINK_CONSTRAINTS + 2) <= AIR10_TAB_ZINV && AIR10_TAB_WORDS <= AIR_TAB_SEL + (256ull << 6),
              "the set-10 tables live in the table part of set 1's scratch");
// log2 of the public table's rows for a table of 2^log_rows rows: the slots ceil(2^log_rows / 80), padded to a power of two
inline uint32_t air_sha512_public_log_k(uint32_t log_rows) {
  const uint64_t slots = ((1ull << log_rows) + 79) / 80;
  uint32_t lg = 0;
  while ((1ull << lg) < slots) lg++;
  return lg;
}
// Where the gather reads in an element row, recorded by build_program (api.cpp) beside AirShaPublicGeom and for the same reason.  A struct
// of its own: set 6's gather takes AirShaPublicGeom by value, so a field added there would change that kernel's arguments.
//   h2, h2_lane, d1a, d1a_lane   as in AirShaPublicGeom
//   h2_pk, h2_r, h2_msg          inside a ValidatorVariable: the bits of pubkey, signature.r and message[124]
//   h2_mlen, h2_signed           message_byte_length and signed
//   d1a_digest                   inside a D.1a lane: the 512 bits of the SHA-512 digest
struct AirSha512PublicGeom {
  uint64_t elem_stride;
  uint32_t n;
  uint32_t h2, h2_lane, h2_pk, h2_r, h2_msg, h2_mlen, h2_signed;
  uint32_t d1a, d1a_lane, d1a_digest;
};
// The public table from element rows: one lane per (proof, block slot); d_pub 49 n_proofs columns of 2^log_k words
int launch_air_sha512_public_gather(const void* d_rows, const AirSha512PublicGeom& G, uint32_t log_k, uint32_t n_proofs, void* d_pub, void* stream);
// The helper oracle from pre-LDE columns and the public lv: one lane per (proof, row); d_table 18 n_proofs columns of 2^log_rows words, d_pub
// 49 n_proofs columns of 2^air_sha512_public_log_k(log_rows), d_helper 65 n_proofs columns of 2^log_rows
int launch_air_sha512_link_helper(uint32_t log_rows, uint32_t n_proofs, const void* d_table, const void* d_pub, void* d_helper, void* stream);
// d_v (planar, 2 << log_rows canonical words) = V_r from pub and gamma (2 words at d_gamma): one lane per row, Horner over the proofs
int launch_air_sha512_link_combine(uint32_t log_rows, uint32_t n_proofs, const void* d_pub, const void* d_gamma, void* d_v, void* stream);
// d_quot (planar, 2 << log_m) -= Pub_gamma / (x^N - 1): d_ext the extended V, d_tab the quotient launch's tables.  The piece that starts at
// proof 0 is followed by it (set 6's rule)
int launch_air_sha512_link_public_sub(uint32_t log_m, uint32_t log_blowup, const void* d_ext, const void* d_tab, void* d_quot, void* stream);
// The barycentric sums of Pub_gamma at zeta over the N rows from d_v: air_sha512_eval_parts(log_rows) rows of AIR10_PUB_PART_WORDS at d_part
int launch_air_sha512_link_public_eval(uint32_t log_rows, uint64_t om, const void* d_zeta, const void* d_v, void* d_part, void* stream);
// d_out[0 .. 2) = Pub_gamma(zeta) from those rows, d_out[2] = 1 if a denominator was zero; n_inv = 1 / N
int launch_air_sha512_link_public_fold(uint32_t log_rows, uint64_t n_inv, const void* d_part, const void* d_zeta, void* d_out, void* stream);
// The identity at zeta: AirSha512Launch::check with the public side's rows at d_pub_part
int launch_air_sha512_link_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint64_t n_inv, const void* d_part,
                                 const void* d_pub_part, const void* d_open_t, const void* d_open_h, const void* d_open_q, const void* d_zeta,
                                 const void* d_gamma, uint32_t n_queries, void* d_ok, void* stream);

}  // namespace tmx
