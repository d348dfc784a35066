// Launch wrappers of the FRI kernels (fri.hip: field-only; poseidon.hip: transcript and verifier).  Host side: plain C++, no HIP headers.
#pragma once
#include <cstdint>

namespace tmx {

constexpr uint32_t FRI_MAX_LAYERS = 28, FRI_MAX_QUERIES = 256, FRI_MAX_ORACLES = 8;

// Everything a FRI kernel needs to know about one proof, built on the host from the parameters, their schedule and the domain (passed
// by value: no upload).  Layer l's domain: s_l, w_l; the fold needs s_l^-1, w_l^-1 and g_l = w_l^-M_(l+1).  Offsets in u64 words.
struct FriGeom {
  uint32_t params[8];  // log_n, n_cols, cap_height, log_blowup, arity_bits, final_log_max, n_queries (the observed order), reserved
  uint32_t log_n, n_cols, cap_height, n_queries, n_layers, final_log;
  uint32_t bits[FRI_MAX_LAYERS], cap_h[FRI_MAX_LAYERS];
  uint64_t s_inv[FRI_MAX_LAYERS], w_inv[FRI_MAX_LAYERS], g[FRI_MAX_LAYERS];
  uint64_t s_fin, w_fin, s_fin_inv, w_fin_inv, m_fin_inv;  // the last domain (D_L), its inverses, 1 / M_L
  uint64_t off_caps[FRI_MAX_LAYERS], off_final, off_indices, off_init_rows, off_init_paths, off_rows[FRI_MAX_LAYERS], off_paths[FRI_MAX_LAYERS];
  // DEEP (include/tmx.h "out-of-domain openings"): deep = 1 for a DEEP transcript / verifier; log_r = log2 of the rows per openings plane;
  // s0, w0: layer 0's domain D_0; omega_n = w0^B, the trace domain's generator (z_1 = zeta omega_n)
  uint32_t deep, log_r;
  uint64_t s0, w0, omega_n;
  // proof of work (include/tmx.h "proof of work"): pow_bits = 0 for a plain transcript / verifier; off_nonce: the nonce word, behind the
  // FRI part
  uint32_t pow_bits;
  uint64_t off_nonce;
  // the mixed-size batch proof (include/tmx.h "one DEEP-FRI proof over several oracles"): n_oracles = 0 for the single-oracle proofs above.
  // Oracle k: its shape, its group (the oracles of one size), alpha_off = n_cols_0 + ... + n_cols_(k-1), its own domain generator w and
  // trace generator omega (the coset shift s0 is common), and where its openings block, rows and paths sit in the proof.  total_cols = C.
  // enter[l] = g >= 1: the fold of layer l adds beta_l^(a_l) Q^(g) (layer l + 1 has the size of group g); 0: a plain fold.
  // batch_head: the words the transcript starts with (2^32 + K, the six scalars); the (log_n_k, n_cols_k) pairs come from the table.
  uint32_t n_oracles, n_groups, total_cols;
  uint64_t batch_head[7];
  uint32_t o_log_n[FRI_MAX_ORACLES], o_n_cols[FRI_MAX_ORACLES], o_cap_h[FRI_MAX_ORACLES], o_log_r[FRI_MAX_ORACLES], o_group[FRI_MAX_ORACLES],
      o_alpha_off[FRI_MAX_ORACLES], o_cap_at[FRI_MAX_ORACLES];  // (o_cap_at: word offset of oracle k's cap in the concatenated caps)
  uint64_t o_w[FRI_MAX_ORACLES], o_omega[FRI_MAX_ORACLES], o_off_open[FRI_MAX_ORACLES], o_off_rows[FRI_MAX_ORACLES], o_off_paths[FRI_MAX_ORACLES];
  uint32_t enter[FRI_MAX_LAYERS];
};

// where the DEEP scratch keeps zeta between launches: chal[FRI_ZETA_AT], chal[FRI_ZETA_AT + 1] (after alpha and the betas)
constexpr uint32_t FRI_ZETA_AT = 2 + 2 * FRI_MAX_LAYERS + 2;
// where the grinding prover keeps the search's two words: chal[FRI_POW_AT] = the smallest satisfying nonce so far (2^64 - 1: none),
// chal[FRI_POW_AT + 1] = the candidates evaluated.  The search gives up after 2^(pow_bits + FRI_POW_SLACK_BITS) candidates.
constexpr uint32_t FRI_POW_AT = FRI_ZETA_AT + 2, FRI_POW_SLACK_BITS = 6, FRI_POW_MAX_BITS = 24;
// where a constraint-challenge transcript (phase 9; include/tmx.h "the constraint quotient of the ladder rows") leaves gamma:
// chal[FRI_GAMMA_AT], chal[FRI_GAMMA_AT + 1] -- word 64 on: such a transcript brings challenge words of its own (air.h AIR_CHAL_WORDS)
constexpr uint32_t FRI_GAMMA_AT = FRI_POW_AT + 2;

// apow[c] = alpha^c (c < n_cols, pairs of u64), alpha at d_alpha
int launch_fri_alpha_powers(uint32_t n_cols, const void* d_alpha, void* d_apow, void* stream);
// layer 0, planar: out[i] = sum_c apow[c].c0 cols[c][i], out[M + i] = sum_c apow[c].c1 cols[c][i]  (M = 2^log_m, canonical)
int launch_fri_combine(uint32_t log_m, uint32_t n_cols, const void* d_cols, const void* d_apow, void* d_out, void* stream);
// the same pass ADDED to what d_out holds (canonical): the second and later oracles of a group, d_apow already offset to alpha^off_k
int launch_fri_combine_add(uint32_t log_m, uint32_t n_cols, const void* d_cols, const void* d_apow, void* d_out, void* stream);
// d_dst[i] = d_dst[i] + d_src[i] mod p over n_words words (d_dst canonical, and canonical after)
int launch_fri_add(uint64_t n_words, const void* d_src, void* d_dst, void* stream);
// layer l (planar, M_l points) -> layer l + 1 (planar, M_l >> bits), with beta at d_beta
int launch_fri_fold(uint32_t log_m_next, uint32_t bits, uint64_t s_inv, uint64_t w_inv, uint64_t g, const void* d_beta, const void* d_in,
                    void* d_out, void* stream);
// the fold that takes a group in: as launch_fri_fold, plus beta^(2^bits) d_add[i] at every output index i (d_add planar, 2^log_m_next points)
int launch_fri_fold_add(uint32_t log_m_next, uint32_t bits, uint64_t s_inv, uint64_t w_inv, uint64_t g, const void* d_beta, const void* d_in,
                        const void* d_add, void* d_out, void* stream);
// the final polynomial of the last layer (planar, 2^log_m points, log_m <= 12): coefficients into d_coef interleaved (c0, c1), the low
// 2^final_log of them; d_flag[0] = 1 if the others are all zero, else 0
int launch_fri_final(uint32_t log_m, uint32_t final_log, uint64_t w_inv, uint64_t s_inv, uint64_t m_inv, const void* d_in, void* d_coef,
                     void* d_flag, void* stream);

// DEEP, the openings of the columns at zeta and zeta omega_N (barycentric on the subset x_j = s omega_N^j, j < N = 2^log_sub).
// wt[j] (interleaved c0, c1) = K x_j / (zeta - x_j), K = (zeta^N - s^N) k_inv with k_inv = 1 / (N s^N); zeta at d_zeta.
int launch_deep_weights(uint32_t log_sub, uint64_t s, uint64_t omega_n, uint64_t s_n, uint64_t k_inv, const void* d_zeta, void* d_wt, void* stream);
// The partial sums of sum_j v_j wt[j] and sum_j v_j wt[j - 1 mod N] of every column over row tiles: column c's word j is
// cols[(c << log_col) + (j << stride_log)].  d_part[tiles][n_cols][4] (y0.c0, y0.c1, y1.c0, y1.c1), tiles = deep_eval_tiles(log_sub).
uint64_t deep_eval_tiles(uint32_t log_sub);
int launch_deep_eval(uint32_t log_sub, uint32_t log_col, uint32_t stride_log, uint32_t n_cols, const void* d_cols, const void* d_wt, void* d_part,
                     void* stream);
// The openings section (planar, 2^log_r rows per plane, zero padding) from the partial sums
int launch_deep_open(uint32_t log_sub, uint32_t n_cols, uint32_t log_r, const void* d_part, void* d_open, void* stream);
// Y_0, Y_1 = sum_c alpha^c y_(c,k) (apow: k_fri_alpha_powers' table) and alpha^n_cols into d_y[6], alpha at d_alpha
int launch_deep_y(uint32_t n_cols, uint32_t log_r, const void* d_open, const void* d_apow, const void* d_alpha, void* d_y, void* stream);
// the batch proof's Y sums, one workgroup per group g: d_y[6 g ..] = sum over the group's oracles k of sum_c alpha^(off_k + c) y_(k,c,j)
// (j = 0, 1; the openings blocks sit in d_proof at G.o_off_open[k]), then alpha^C.  d_apow: the table of C + 1 powers.
int launch_batch_y(const FriGeom& G, const void* d_proof, const void* d_apow, void* d_y, void* stream);
// layer 0 (planar, 2^log_m points of s w^i) in place: f_0 = (F - Y_0) / (x - z_0) + alpha^n (F - Y_1) / (x - z_1)
int launch_deep_quotient(uint32_t log_m, uint64_t s, uint64_t w, uint64_t omega_n, const void* d_zeta, const void* d_y, void* d_layer, void* stream);

// The single-lane transcript between the prover's stages (poseidon.hip).  d_state: the duplex state between launches (32 u64); d_chal:
// alpha (2 u64) then beta_l (2 u64 each).  phase 0: parameters + commit cap -> alpha; phase 1: cap of `layer` (in the proof) -> beta_layer;
// phase 2: final coefficients -> query indices into the proof and each layer's leaf indices into d_qidx[n_layers][n_queries];
// DEEP: phase 3: parameters, the word 2, commit cap -> zeta (chal[FRI_ZETA_AT]); phase 4: the openings root at d_commit_cap -> alpha.
// The batch proof: phase 7: the batch start over the K caps concatenated at d_commit_cap -> zeta; phase 8: the K openings roots (4 K words
// at d_commit_cap) -> alpha.  The other phases serve it unchanged (G.log_n = the largest oracle's).
// Grinding splits phase 2: phase 5 (2a): final coefficients and pow_bits observed, the duplex left in d_state, the search's words reset;
// phase 6 (2b): the nonce the search left -> the proof, observed, r drawn, then the indices as phase 2.
// The constraint challenge: phase 9: a fresh duplex, 2^33, G.params[0 .. 5) (set id, log_n, log_blowup, cap_height, n_proofs), the trace cap
// at d_commit_cap (4 << G.cap_height words) -> gamma (chal[FRI_GAMMA_AT]).  phase 10: the same, then the 4 words of the public table's
// digest, READ at d_proof, before gamma is drawn (constraint set 2).
int launch_fri_transcript(const void* d_consts, int mode, const FriGeom& G, int phase, uint32_t layer, const void* d_commit_cap, void* d_proof,
                          void* d_state, void* d_chal, void* d_qidx, void* stream);
// The search between phases 5 and 6: the smallest nonce whose challenge has pow_bits leading zero bits, from the duplex in d_state, into
// d_pow[0] (atomic minimum), the candidates evaluated added to d_pow[1].  One launch that ends itself; the grid is sized from pow_bits.
int launch_fri_grind(const void* d_consts, int mode, uint32_t pow_bits, const void* d_state, void* d_pow, void* stream);
// d_ok[q] for every query of the proof against d_cap (one workgroup).  G.deep: d_proof is the FRI part of a DEEP proof, d_open its
// openings section and d_root the root of the openings tree; otherwise both are unused.  G.n_oracles: the batch proof: d_cap the K caps
// concatenated, d_proof the whole proof, d_root the K roots (4 words each); d_open unused.
int launch_fri_verify(const void* d_consts, int mode, const FriGeom& G, const void* d_cap, const void* d_proof, const void* d_open, const void* d_root,
                      void* d_ok, void* stream);

}  // namespace tmx
