// Launch wrappers of the FRI kernels (fri.hip: field-only; poseidon.hip: transcript and verifier).  Host side: plain C++, no HIP headers.
#pragma once
#include <cstdint>

namespace tmx {

constexpr uint32_t FRI_MAX_LAYERS = 28, FRI_MAX_QUERIES = 256;

// Everything a FRI kernel needs to know about one proof, built on the host from the parameters, their schedule and the domain (passed
// by value: no upload).  Layer l's domain: s_l, w_l; the fold needs s_l^-1, w_l^-1 and g_l = w_l^-M_(l+1).  Offsets in u64 words.
struct FriGeom {
  uint32_t params[8];  // log_n, n_cols, cap_height, log_blowup, arity_bits, final_log_max, n_queries (the observed order), reserved
  uint32_t log_n, n_cols, cap_height, n_queries, n_layers, final_log;
  uint32_t bits[FRI_MAX_LAYERS], cap_h[FRI_MAX_LAYERS];
  uint64_t s_inv[FRI_MAX_LAYERS], w_inv[FRI_MAX_LAYERS], g[FRI_MAX_LAYERS];
  uint64_t s_fin, w_fin, s_fin_inv, w_fin_inv, m_fin_inv;  // the last domain (D_L), its inverses, 1 / M_L
  uint64_t off_caps[FRI_MAX_LAYERS], off_final, off_indices, off_init_rows, off_init_paths, off_rows[FRI_MAX_LAYERS], off_paths[FRI_MAX_LAYERS];
};

// apow[c] = alpha^c (c < n_cols, pairs of u64), alpha at d_alpha
int launch_fri_alpha_powers(uint32_t n_cols, const void* d_alpha, void* d_apow, void* stream);
// layer 0, planar: out[i] = sum_c apow[c].c0 cols[c][i], out[M + i] = sum_c apow[c].c1 cols[c][i]  (M = 2^log_m, canonical)
int launch_fri_combine(uint32_t log_m, uint32_t n_cols, const void* d_cols, const void* d_apow, void* d_out, void* stream);
// layer l (planar, M_l points) -> layer l + 1 (planar, M_l >> bits), with beta at d_beta
int launch_fri_fold(uint32_t log_m_next, uint32_t bits, uint64_t s_inv, uint64_t w_inv, uint64_t g, const void* d_beta, const void* d_in,
                    void* d_out, void* stream);
// the final polynomial of the last layer (planar, 2^log_m points, log_m <= 12): coefficients into d_coef interleaved (c0, c1), the low
// 2^final_log of them; d_flag[0] = 1 if the others are all zero, else 0
int launch_fri_final(uint32_t log_m, uint32_t final_log, uint64_t w_inv, uint64_t s_inv, uint64_t m_inv, const void* d_in, void* d_coef,
                     void* d_flag, void* stream);

// The single-lane transcript between the prover's stages (poseidon.hip).  d_state: the duplex state between launches (32 u64); d_chal:
// alpha (2 u64) then beta_l (2 u64 each).  phase 0: parameters + commit cap -> alpha; phase 1: cap of `layer` (in the proof) -> beta_layer;
// phase 2: final coefficients -> query indices into the proof and each layer's leaf indices into d_qidx[n_layers][n_queries].
int launch_fri_transcript(const void* d_consts, int mode, const FriGeom& G, int phase, uint32_t layer, const void* d_commit_cap, void* d_proof,
                          void* d_state, void* d_chal, void* d_qidx, void* stream);
// d_ok[q] for every query of the proof against d_cap (one workgroup)
int launch_fri_verify(const void* d_consts, int mode, const FriGeom& G, const void* d_cap, const void* d_proof, void* d_ok, void* stream);

}  // namespace tmx
