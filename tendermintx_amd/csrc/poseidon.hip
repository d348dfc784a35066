// Poseidon over Goldilocks and the Merkle-cap commitment of LDE'd columns ("commit primitives": what a
// plonky2-style prover does with the trace columns after the LDE -- the reference reaches it through plonky2x `prove`, reference
// circuits/skip.rs:119-133; plonky2 itself is absent from the reference tree, Cargo.lock:2957-2982).
// Definition (include/tmx.h; restated on the CPU by the test oracle): width 12, x^7, 4 + 22 + 4 rounds, circulant-plus-diagonal MDS, overwrite-mode sponge of rate 8,
// two_to_one, hash_or_noop leaves.  Round constants and MDS rows are DATA (injected through tmx_poseidon_set_constants; the defaults are
// the Poseidon paper's Grain-LFSR stream, not plonky2's table: parity unpinned), read with scalar loads -- wave-uniform addresses.
//
// One permutation per thread, the twelve state elements in 24 VGPRs as arbitrary 64-bit representatives of their classes ("lazy": only the
// stored digests are canonical).  This is pure 64-bit integer VALU work -- no MFMA (nothing is a dense contraction: the MDS layer is a
// 12 x 12 product by 6-bit constants), HBM traffic is 8 B in / 0.5 B out per hashed element -- so its roof is VALU issue:
//   S-box x^7 = 4 field products (4 v_mad_u64_u32 + ~14 for the reduction each), 118 S-boxes per permutation;
//   MDS layer with small entries: the sums  sum c_i lo(s_i)  and  sum c_i hi(s_i)  over the 32-bit halves fit 64 bits, so a row is
//   24 v_mad_u64_u32 and ONE reduction (2^32 (h_lo + 2^32 h_hi) = 2^32 h_lo + (2^32 - 1) h_hi) instead of 12 field products.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "air.h"
#include "fri.h"
#include "goldilocks_ext.hpp"
#include "poseidon.h"

namespace tmx {

struct PosConsts {
  const uint64_t* rc;    // [POS_ROUNDS][12]
  const uint64_t* circ;  // [12]
  const uint64_t* diag;  // [12]
  const uint64_t* x;     // the whole buffer (poseidon.h: POS_X_* tables of the merged partial rounds)
};
__device__ __forceinline__ PosConsts pos_consts(const uint64_t* c) { return PosConsts{c, c + POS_ROUNDS * POS_T, c + POS_ROUNDS * POS_T + POS_T, c}; }

__device__ __forceinline__ uint64_t pos_sbox(uint64_t x) {
  const uint64_t x2 = gl_mul_lazy(x, x), x3 = gl_mul_lazy(x2, x), x4 = gl_mul_lazy(x2, x2);
  return gl_mul_lazy(x3, x4);
}
// lo + 2^32 hi for lo, hi < 2^62: any representative.  2^32 hi = 2^32 h_lo + 2^64 h_hi = 2^32 h_lo + (2^32 - 1) h_hi: the second term
// rides on ONE v_mad_u64_u32 with lo as its addend (< 2^30 2^32 + 2^62: no carry), the first is an add into the high word whose carry
// (2^64 = 2^32 - 1) is folded back once -- after a carry the sum is < 2^63, so it cannot wrap again.
__device__ __forceinline__ uint64_t pos_fold(uint64_t lo, uint64_t hi) {
  const uint32_t h_lo = (uint32_t)hi, h_hi = (uint32_t)(hi >> 32);
  const uint64_t t = (uint64_t)h_hi * 0xffffffffu + lo;
  uint32_t n_hi;
  const bool carry = __builtin_uadd_overflow((uint32_t)(t >> 32), h_lo, &n_hi);
  const uint64_t s = ((uint64_t)n_hi << 32) | (uint32_t)t;
  return s + (carry ? GL_EPS : 0ull);
}
// MDS layer.  SMALL (every entry < 2^16): the diagonal entry joins the circulant's entry 0 on the scalar unit, and the NEXT round's
// constants enter as one more multiply-add per accumulator (rc_lo * inj, rc_hi * inj with inj = 1 in a VGPR; 0 behind the last round) --
// two instructions per element instead of a 64-bit modular add (five).  Bounds: 13 products < 2^17 2^32 and one < 2^32: < 2^53.
template <bool SMALL>
__device__ __forceinline__ void pos_mds(uint64_t (&s)[12], const PosConsts& K, const uint64_t* __restrict__ rc_next, bool more, uint32_t inj) {
  uint64_t o[12];
  if (SMALL) {
    uint32_t lo[12], hi[12];
#pragma unroll
    for (int i = 0; i < 12; i++) { lo[i] = (uint32_t)s[i]; hi[i] = (uint32_t)(s[i] >> 32); }
#pragma unroll
    for (int r = 0; r < 12; r++) {
      const uint64_t rcn = rc_next[r];
      uint64_t al = (uint64_t)(uint32_t)rcn * inj, ah = (uint64_t)(uint32_t)(rcn >> 32) * inj;
#pragma unroll
      for (int i = 0; i < 12; i++) {
        const uint32_t c = (uint32_t)K.circ[i] + (i == 0 ? (uint32_t)K.diag[r] : 0u);
        al += (uint64_t)c * lo[(i + r) % 12];
        ah += (uint64_t)c * hi[(i + r) % 12];
      }
      o[r] = pos_fold(al, ah);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 12; r++) {
      uint64_t acc = gl_mul(s[r], K.diag[r]);
#pragma unroll
      for (int i = 0; i < 12; i++) acc = gl_add(acc, gl_mul(s[(i + r) % 12], K.circ[i]));
      o[r] = more ? gl_add_lazy(acc, rc_next[r]) : acc;  // (uniform)
    }
  }
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = o[i];
}
// Three partial rounds at once (poseidon.h: POS_MODE_MERGE3).  s holds u = the state with its round constants added; on return the same
// three rounds later.  428 multiply-adds instead of 3 x 324.  The coefficients are scalar loads; the compiler barriers keep them row by row
// (hoisted to the top of the group, the 200 dwords do not fit the scalar registers and were spilled into VGPR lanes: 700 v_writelane /
// v_readlane per group).
__device__ __forceinline__ void pos_group3(uint64_t (&s)[12], const PosConsts& K, uint32_t g, uint32_t vone) {
  const uint64_t* G = K.x + POS_X_GROUPS + g * POS_X_GROUP_WORDS;
  const uint32_t* U = reinterpret_cast<const uint32_t*>(K.x + POS_X_U32);
  s[0] = pos_sbox(s[0]);
  uint32_t lo[12], hi[12];
#pragma unroll
  for (int i = 0; i < 12; i++) { lo[i] = (uint32_t)s[i]; hi[i] = (uint32_t)(s[i] >> 32); }
  uint64_t al, ah;
  // y1 = M[0,:] v + K1
  al = (uint64_t)(uint32_t)G[0] * vone; ah = (uint64_t)(uint32_t)(G[0] >> 32) * vone;
#pragma unroll
  for (int i = 0; i < 12; i++) { const uint32_t c = U[POS_U_R1 + i]; al += (uint64_t)c * lo[i]; ah += (uint64_t)c * hi[i]; }
  const uint64_t y1 = pos_fold(al, ah);
  const uint64_t d1 = gl_sub_lazy(pos_sbox(y1), gl_canon(y1));
  const uint32_t d1lo = (uint32_t)d1, d1hi = (uint32_t)(d1 >> 32);
  asm volatile("" ::: "memory");
  // y2 = M^2[0,:] v + d1 M[0,0] + K2
  al = (uint64_t)(uint32_t)G[1] * vone; ah = (uint64_t)(uint32_t)(G[1] >> 32) * vone;
#pragma unroll
  for (int i = 0; i < 12; i++) { const uint32_t c = U[POS_U_R2 + i]; al += (uint64_t)c * lo[i]; ah += (uint64_t)c * hi[i]; }
  { const uint32_t c = U[POS_U_C1]; al += (uint64_t)c * d1lo; ah += (uint64_t)c * d1hi; }
  const uint64_t y2 = pos_fold(al, ah);
  const uint64_t d2 = gl_sub_lazy(pos_sbox(y2), gl_canon(y2));
  const uint32_t d2lo = (uint32_t)d2, d2hi = (uint32_t)(d2 >> 32);
  // u' = M^3 v + d1 M^2[:,0] + d2 M[:,0] + K3: the coefficients of row r + 1 are requested before the arithmetic of row r and waited for
  // behind it (the empty asm with "s" operands is where the compiler puts the s_waitcnt: scalar loads return out of order, so a wait in
  // front of the arithmetic would wait for the next row's too)
  typedef uint32_t pos_u32x4 __attribute__((ext_vector_type(4)));
  struct Row { pos_u32x4 a, b, c; uint32_t c2, c1; uint64_t k3; };
  auto load_row = [&](int r) {
    Row w;
    const pos_u32x4* m = reinterpret_cast<const pos_u32x4*>(U + POS_U_M3 + 12 * r);
    w.a = m[0]; w.b = m[1]; w.c = m[2]; w.c2 = U[POS_U_C2 + r]; w.c1 = U[POS_U_C1 + r]; w.k3 = G[2 + r];
    return w;
  };
  auto settle = [&](const Row& w) {
    asm volatile("" ::"s"(w.a.x), "s"(w.a.y), "s"(w.a.z), "s"(w.a.w), "s"(w.b.x), "s"(w.b.y), "s"(w.b.z), "s"(w.b.w), "s"(w.c.x), "s"(w.c.y), "s"(w.c.z),
                 "s"(w.c.w), "s"(w.c2), "s"(w.c1), "s"(w.k3)
                 : "memory");
  };
  Row nxt = load_row(0);
  settle(nxt);
#pragma unroll
  for (int r = 0; r < 12; r++) {
    const Row w = nxt;
    if (r + 1 < 12) nxt = load_row(r + 1);
    const uint32_t cf[12] = {w.a.x, w.a.y, w.a.z, w.a.w, w.b.x, w.b.y, w.b.z, w.b.w, w.c.x, w.c.y, w.c.z, w.c.w};
    al = (uint64_t)(uint32_t)w.k3 * vone; ah = (uint64_t)(uint32_t)(w.k3 >> 32) * vone;
#pragma unroll
    for (int i = 0; i < 12; i++) { al += (uint64_t)cf[i] * lo[i]; ah += (uint64_t)cf[i] * hi[i]; }
    al += (uint64_t)w.c2 * d1lo; ah += (uint64_t)w.c2 * d1hi;
    al += (uint64_t)w.c1 * d2lo; ah += (uint64_t)w.c1 * d2hi;
    s[r] = pos_fold(al, ah);
    if (r + 1 < 12) settle(nxt); else asm volatile("" ::: "memory");
  }
}
template <int MODE>
__device__ __forceinline__ void pos_permute(uint64_t (&s)[12], const PosConsts& K) {
  constexpr bool SMALL = MODE != POS_MODE_GENERAL;
  uint32_t vone;
  asm volatile("v_mov_b32 %0, 1" : "=v"(vone));  // (opaque to the optimizer: rc * 1 has to stay a multiply-add)
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = gl_add_lazy(s[i], K.rc[i]);
#pragma unroll 1
  for (int r = 0; r < (int)POS_ROUNDS; r++) {
    if (MODE == POS_MODE_MERGE3 && r == (int)POS_MERGE_FIRST) {  // rounds 5 .. 25 in seven groups of three
#pragma unroll 1
      for (uint32_t g = 0; g < POS_MERGE_GROUPS; g++) pos_group3(s, K, g, vone);
      r = (int)(POS_RF / 2 + POS_RP) - 1;
      continue;
    }
    if (r < (int)POS_RF / 2 || r >= (int)(POS_RF / 2 + POS_RP)) {  // (uniform: a scalar branch)
#pragma unroll
      for (int i = 0; i < 12; i++) s[i] = pos_sbox(s[i]);
    } else {
      s[0] = pos_sbox(s[0]);
    }
    const bool more = r + 1 < (int)POS_ROUNDS;
    pos_mds<SMALL>(s, K, K.rc + (more ? r + 1 : r) * 12, more, more ? vone : 0u);
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_poseidon_permute(const uint64_t* __restrict__ consts, uint32_t n, const uint64_t* __restrict__ in,
                                                          uint64_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const PosConsts K = pos_consts(consts);
  uint64_t s[12];
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = in[(size_t)i * 12 + k];
  pos_permute<MODE>(s, K);
#pragma unroll
  for (int k = 0; k < 12; k++) out[(size_t)i * 12 + k] = gl_canon(s[k]);
}

// leaf digest of row r: the row's n_cols values (column c at cols[(c << log_n) + r]: consecutive threads read consecutive addresses of
// every column), absorbed eight at a time in overwrite mode; rows of at most four values are their own digest (hash_or_noop)
template <int MODE>
__global__ __launch_bounds__(256) void k_poseidon_leaves(const uint64_t* __restrict__ consts, uint32_t log_n, uint32_t n_cols,
                                                         const uint64_t* __restrict__ cols, uint64_t* __restrict__ digests) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >> log_n) return;
  const PosConsts K = pos_consts(consts);
  uint64_t s[12];
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  if (n_cols <= 4) {
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) s[c] = c < n_cols ? gl_canon(cols[((uint64_t)c << log_n) + r]) : 0;  // (inputs are taken mod p: any u64 < 2 p)
  } else {
    for (uint32_t c0 = 0; c0 < n_cols; c0 += 8) {
#pragma unroll
      for (uint32_t k = 0; k < 8; k++)
        if (c0 + k < n_cols) s[k] = cols[((uint64_t)(c0 + k) << log_n) + r];
      pos_permute<MODE>(s, K);
    }
  }
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  u64x2 a, b;
  a.x = gl_canon(s[0]); a.y = gl_canon(s[1]); b.x = gl_canon(s[2]); b.y = gl_canon(s[3]);
  u64x2* o = reinterpret_cast<u64x2*>(digests + 4 * r);
  o[0] = a; o[1] = b;
}

// The same sponge over ONE CHUNK of a row's columns (the streamed members of a commit set: the extended columns exist a chunk at a time).
// `first`: start from the zero state, else load the row's 12 state words; absorb the chunk's n_cols columns eight at a time exactly as
// k_poseidon_leaves does; `last`: write the canonical digest, else store the 12 words as they are (lazy representatives: the next chunk
// goes on with the very words the one-pass kernel would hold).  All 12 travel: overwrite mode keeps the rate words of a short block.
// state is planar, word k of row r at state[(k << log_n) + r], so consecutive lanes load and store consecutive addresses.  A chunk that is
// not the last has a multiple of eight columns (the caller's rule), so a short block only ever ends the row; rows of <= 4 columns are
// never streamed.  first and last are wave-uniform (scalar branches).
template <int MODE>
__global__ __launch_bounds__(256) void k_poseidon_leaves_chunk(const uint64_t* __restrict__ consts, uint32_t log_n, uint32_t n_cols,
                                                               const uint64_t* __restrict__ cols, uint32_t first, uint32_t last,
                                                               uint64_t* __restrict__ state, uint64_t* __restrict__ digests) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >> log_n) return;
  const PosConsts K = pos_consts(consts);
  uint64_t s[12];
  if (first) {
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = 0;
  } else {
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = state[((uint64_t)k << log_n) + r];
  }
  for (uint32_t c0 = 0; c0 < n_cols; c0 += 8) {
#pragma unroll
    for (uint32_t k = 0; k < 8; k++)
      if (c0 + k < n_cols) s[k] = cols[((uint64_t)(c0 + k) << log_n) + r];
    pos_permute<MODE>(s, K);
  }
  if (last) {
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    u64x2 a, b;
    a.x = gl_canon(s[0]); a.y = gl_canon(s[1]); b.x = gl_canon(s[2]); b.y = gl_canon(s[3]);
    u64x2* o = reinterpret_cast<u64x2*>(digests + 4 * r);
    o[0] = a; o[1] = b;
  } else {
#pragma unroll
    for (int k = 0; k < 12; k++) state[((uint64_t)k << log_n) + r] = s[k];
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_poseidon_level(const uint64_t* __restrict__ consts, uint64_t n_out, const uint64_t* __restrict__ in,
                                                        uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  const PosConsts K = pos_consts(consts);
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  const u64x2* p = reinterpret_cast<const u64x2*>(in + 8 * i);
  const u64x2 v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
  uint64_t s[12] = {v0.x, v0.y, v1.x, v1.y, v2.x, v2.y, v3.x, v3.y, 0, 0, 0, 0};
  pos_permute<MODE>(s, K);
  u64x2 a, b;
  a.x = gl_canon(s[0]); a.y = gl_canon(s[1]); b.x = gl_canon(s[2]); b.y = gl_canon(s[3]);
  u64x2* o = reinterpret_cast<u64x2*>(out + 4 * i);
  o[0] = a; o[1] = b;
}

// ---- openings of a tree (the query phase of a FRI-style consumer) ----------------------------------------------------------------------
// Query q opens leaf i = idx[q] (validated on the host: i < 2^log_n).  Rows: rows[q][c] = cols[(c << log_n) + i], the stored word as it is
// (no reduction).  Block (q, y) copies columns y * 256 + t, y * 256 + t + gridDim.y * 256, ...: consecutive threads write consecutive words
// of one row, and each read is the one word of a different column that sits 2^log_n * 8 B from its neighbour -- a cache line per (query,
// column), so the grid is sized to keep many of them in flight.  Paths: block (q, 0) also writes paths[q][l] = levels[off_l + ((i >> l) ^ 1)]
// for l < path_len (bottom-up, the leaf's sibling first), off_l = 2^(log_n + 1) - 2^(log_n + 1 - l) digests (the leaves, then each level).
// Either pointer may be null: the split form runs the rows and the paths as two launches.
__global__ __launch_bounds__(256) void k_merkle_open(uint32_t log_n, uint32_t n_cols, const uint64_t* __restrict__ cols, uint32_t path_len,
                                                     const uint64_t* __restrict__ levels, const uint64_t* __restrict__ idx,
                                                     uint64_t* __restrict__ rows, uint64_t* __restrict__ paths) {
  const uint32_t q = blockIdx.x;
  const uint64_t i = idx[q];
  if (rows) {
    uint64_t* row = rows + (uint64_t)q * n_cols;
    for (uint64_t c = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; c < n_cols; c += (uint64_t)gridDim.y * blockDim.x)
      row[c] = cols[(c << log_n) + i];
  }
  if (paths && blockIdx.y == 0 && threadIdx.x < 4 * path_len) {
    const uint32_t l = threadIdx.x >> 2, w = threadIdx.x & 3;
    const uint64_t off = (2ull << log_n) - (2ull << (log_n - l));
    paths[((uint64_t)q * path_len + l) * 4 + w] = levels[(off + ((i >> l) ^ 1ull)) * 4 + w];
  }
}

// The rows of k_merkle_open for one chunk of a wider row (a streamed member: `cols` holds n_cols of the row's row_stride columns, `rows`
// points at the chunk's first column inside row 0): rows[q * row_stride + c] = cols[(c << log_n) + idx[q]], c < n_cols.
__global__ __launch_bounds__(256) void k_merkle_open_chunk(uint32_t log_n, uint32_t n_cols, const uint64_t* __restrict__ cols,
                                                           const uint64_t* __restrict__ idx, uint64_t* __restrict__ rows, uint64_t row_stride) {
  const uint32_t q = blockIdx.x;
  const uint64_t i = idx[q];
  uint64_t* row = rows + (uint64_t)q * row_stride;
  for (uint64_t c = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; c < n_cols; c += (uint64_t)gridDim.y * blockDim.x)
    row[c] = cols[(c << log_n) + i];
}

__device__ __forceinline__ void pos_digest_out(const uint64_t (&s)[12], uint64_t (&d)[4]) {
#pragma unroll
  for (int k = 0; k < 4; k++) d[k] = gl_canon(s[k]);
}

// Does row (n_cols words) with its path (path_len digests, bottom-up) lead to cap[i >> path_len]?  The leaf digest is formed exactly as
// k_poseidon_leaves forms it (rows of <= 4 words: their own canonical, zero-padded digest; else the overwrite-mode sponge, whose short last
// chunk leaves the unused rate words as they were), then the path (bit l of i set: cur = two_to_one(sib, cur), else two_to_one(cur, sib)),
// then cur == the cap digest word for word.  Sequential: one permutation per 8 columns plus one per level.
template <int MODE>
__device__ bool merkle_leads_to_cap(const PosConsts& K, const uint64_t* __restrict__ row, uint32_t n_cols, const uint64_t* __restrict__ path,
                                    uint32_t path_len, uint64_t i, const uint64_t* __restrict__ cap) {
  uint64_t s[12];
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  if (n_cols <= 4) {
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) s[c] = c < n_cols ? gl_canon(row[c]) : 0;
  } else {
    for (uint32_t c0 = 0; c0 < n_cols; c0 += 8) {
#pragma unroll
      for (uint32_t k = 0; k < 8; k++)
        if (c0 + k < n_cols) s[k] = row[c0 + k];
      pos_permute<MODE>(s, K);
    }
  }
  uint64_t cur[4];
  pos_digest_out(s, cur);
  for (uint32_t l = 0; l < path_len; l++) {
    const bool right = (i >> l) & 1ull;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint64_t sib = path[4 * l + k];
      s[k] = right ? sib : cur[k];
      s[4 + k] = right ? cur[k] : sib;
      s[8 + k] = 0;
    }
    pos_permute<MODE>(s, K);
    pos_digest_out(s, cur);
  }
  const uint64_t* want = cap + 4 * (i >> path_len);
  return cur[0] == want[0] && cur[1] == want[1] && cur[2] == want[2] && cur[3] == want[3];
}

// One thread per query (merkle_leads_to_cap); blocks of one wave spread the queries over the CUs.
template <int MODE>
__global__ __launch_bounds__(64) void k_merkle_verify(const uint64_t* __restrict__ consts, uint32_t n_cols, uint32_t path_len, uint32_t n_queries,
                                                      const uint64_t* __restrict__ cap, const uint64_t* __restrict__ idx,
                                                      const uint64_t* __restrict__ rows, const uint64_t* __restrict__ paths, uint32_t* __restrict__ ok) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_queries) return;
  const PosConsts K = pos_consts(consts);
  ok[q] = merkle_leads_to_cap<MODE>(K, rows + (uint64_t)q * n_cols, n_cols, paths + (uint64_t)q * path_len * 4, path_len, idx[q], cap) ? 1u : 0u;
}

// ---- the FRI transcript (include/tmx.h "transcript"): a Poseidon duplex modelled on plonky2's Challenger ---------------------------------
// The buffers are indexed by selects over unrolled loops (no dynamic register indexing: the whole duplex stays in VGPRs).
struct FriChal {
  uint64_t st[12], in[8], out[8];
  uint32_t n_in, n_out;
};
__device__ __forceinline__ void chal_init(FriChal& c) {
#pragma unroll
  for (int k = 0; k < 12; k++) c.st[k] = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) c.in[k] = c.out[k] = 0;
  c.n_in = c.n_out = 0;
}
template <int MODE>
__device__ __forceinline__ void chal_duplex(FriChal& c, const PosConsts& K) {
#pragma unroll
  for (uint32_t k = 0; k < 8; k++)
    if (k < c.n_in) c.st[k] = c.in[k];
  c.n_in = 0;
  pos_permute<MODE>(c.st, K);
#pragma unroll
  for (int k = 0; k < 12; k++) c.st[k] = gl_canon(c.st[k]);
#pragma unroll
  for (int k = 0; k < 8; k++) c.out[k] = c.st[k];
  c.n_out = 8;
}
template <int MODE>
__device__ __forceinline__ void chal_observe(FriChal& c, const PosConsts& K, uint64_t x) {
  c.n_out = 0;
  x = gl_canon(x);
#pragma unroll
  for (uint32_t k = 0; k < 8; k++)
    if (k == c.n_in) c.in[k] = x;
  if (++c.n_in == 8) chal_duplex<MODE>(c, K);
}
template <int MODE>
__device__ __forceinline__ uint64_t chal_challenge(FriChal& c, const PosConsts& K) {
  if (c.n_in || !c.n_out) chal_duplex<MODE>(c, K);
  const uint32_t at = --c.n_out;
  uint64_t x = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; k++)
    if (k == at) x = c.out[k];
  return x;
}
template <int MODE>
__device__ void chal_observe_span(FriChal& c, const PosConsts& K, const uint64_t* __restrict__ p, uint64_t n) {
  for (uint64_t k = 0; k < n; k++) chal_observe<MODE>(c, K, p[k]);
}
// the duplex between the prover's launches: st | in | out | n_in, n_out (32 u64)
__device__ __forceinline__ void chal_load(FriChal& c, const uint64_t* __restrict__ m) {
#pragma unroll
  for (int k = 0; k < 12; k++) c.st[k] = m[k];
#pragma unroll
  for (int k = 0; k < 8; k++) { c.in[k] = m[12 + k]; c.out[k] = m[20 + k]; }
  c.n_in = (uint32_t)m[28]; c.n_out = (uint32_t)m[29];
}
__device__ __forceinline__ void chal_store(const FriChal& c, uint64_t* __restrict__ m) {
#pragma unroll
  for (int k = 0; k < 12; k++) m[k] = c.st[k];
#pragma unroll
  for (int k = 0; k < 8; k++) { m[12 + k] = c.in[k]; m[20 + k] = c.out[k]; }
  m[28] = c.n_in; m[29] = c.n_out;
}
template <int MODE>
__device__ __forceinline__ void chal_start(FriChal& c, const PosConsts& K, const FriGeom& G, const uint64_t* __restrict__ commit_cap) {
  chal_init(c);
  for (int k = 0; k < 7; k++) chal_observe<MODE>(c, K, G.params[k]);
  chal_observe_span<MODE>(c, K, commit_cap, 4ull << G.cap_height);
}
// DEEP: the same start with the word 2 (the number of opening points) between the parameters and the cap, then zeta = (challenge(),
// challenge()), drawn again while zeta.c1 == 0 (zeta outside F_p)
template <int MODE>
__device__ __forceinline__ gl2 chal_start_deep(FriChal& c, const PosConsts& K, const FriGeom& G, const uint64_t* __restrict__ commit_cap) {
  chal_init(c);
  for (int k = 0; k < 7; k++) chal_observe<MODE>(c, K, G.params[k]);
  chal_observe<MODE>(c, K, 2);
  chal_observe_span<MODE>(c, K, commit_cap, 4ull << G.cap_height);
  gl2 z;
  do {
    z.c0 = chal_challenge<MODE>(c, K);
    z.c1 = chal_challenge<MODE>(c, K);
  } while (z.c1 == 0);
  return z;
}
// The batch proof (include/tmx.h "one DEEP-FRI proof over several oracles"): 2^32 + K and the six scalars, the (log_n_k, n_cols_k) pairs,
// the word 2, the K caps (concatenated at `caps`), then zeta as DEEP draws it
template <int MODE>
__device__ __forceinline__ gl2 chal_start_batch(FriChal& c, const PosConsts& K, const FriGeom& G, const uint64_t* __restrict__ caps) {
  chal_init(c);
  for (int k = 0; k < 7; k++) chal_observe<MODE>(c, K, G.batch_head[k]);
  for (uint32_t k = 0; k < 2 * G.n_oracles; k++) chal_observe<MODE>(c, K, (k & 1) ? G.o_n_cols[k >> 1] : G.o_log_n[k >> 1]);
  chal_observe<MODE>(c, K, 2);
  const uint32_t last = G.n_oracles - 1;
  chal_observe_span<MODE>(c, K, caps, G.o_cap_at[last] + (4ull << G.o_cap_h[last]));
  gl2 z;
  do {
    z.c0 = chal_challenge<MODE>(c, K);
    z.c1 = chal_challenge<MODE>(c, K);
  } while (z.c1 == 0);
  return z;
}

// One lane, between the prover's stages (fri.h launch_fri_transcript): the parameters and the commit cap -> alpha (phase 0), the cap of
// `layer` -> beta_layer (phase 1), the final coefficients -> the query indices and every layer's leaf indices (phase 2).  DEEP: the start
// with its point count and the commit cap -> zeta (phase 3), the openings root at commit_cap -> alpha (phase 4).  Grinding: phase 2 in two
// halves around k_fri_grind: the final coefficients and pow_bits observed (phase 5), the nonce observed and r drawn -> the indices (phase 6).
// The batch proof: its start over the K caps at commit_cap -> zeta (phase 7), the K openings roots at commit_cap -> alpha (phase 8).
// The constraint challenge (include/tmx.h "the constraint quotient of the ladder rows"): a transcript of its own over the trace cap at
// commit_cap -> gamma (phase 9); constraint set 2: the same with the public table's digest (4 words at `proof`) behind the cap (phase 10).
template <int MODE>
__global__ __launch_bounds__(64) void k_fri_transcript(const uint64_t* __restrict__ consts, FriGeom G, int phase, uint32_t layer,
                                                       const uint64_t* __restrict__ commit_cap, uint64_t* __restrict__ proof, uint64_t* __restrict__ state,
                                                       uint64_t* __restrict__ chal, uint64_t* __restrict__ qidx) {
  if (threadIdx.x) return;
  const PosConsts K = pos_consts(consts);
  FriChal c;
  if (phase == 0) {
    chal_start<MODE>(c, K, G, commit_cap);
    chal[0] = chal_challenge<MODE>(c, K);
    chal[1] = chal_challenge<MODE>(c, K);
  } else if (phase == 3) {
    const gl2 z = chal_start_deep<MODE>(c, K, G, commit_cap);
    chal[FRI_ZETA_AT] = z.c0;
    chal[FRI_ZETA_AT + 1] = z.c1;
  } else if (phase == 7) {
    const gl2 z = chal_start_batch<MODE>(c, K, G, commit_cap);
    chal[FRI_ZETA_AT] = z.c0;
    chal[FRI_ZETA_AT + 1] = z.c1;
  } else if (phase == 9) {
    chal_init(c);
    chal_observe<MODE>(c, K, 1ull << 33);
    for (int k = 0; k < 5; k++) chal_observe<MODE>(c, K, G.params[k]);
    chal_observe_span<MODE>(c, K, commit_cap, 4ull << G.cap_height);
    gl2 g;
    do {
      g.c0 = chal_challenge<MODE>(c, K);
      g.c1 = chal_challenge<MODE>(c, K);
    } while (g.c1 == 0);
    chal[FRI_GAMMA_AT] = g.c0;
    chal[FRI_GAMMA_AT + 1] = g.c1;
  } else if (phase == 10) {
    // constraint set 2 (include/tmx.h "the boundary constraints of the ladder rows"): as phase 9 with G.params[0] = 2, then the four words
    // of the public table's digest, read at `proof` (nothing is written there)
    chal_init(c);
    chal_observe<MODE>(c, K, 1ull << 33);
    for (int k = 0; k < 5; k++) chal_observe<MODE>(c, K, G.params[k]);
    chal_observe_span<MODE>(c, K, commit_cap, 4ull << G.cap_height);
    chal_observe_span<MODE>(c, K, proof, 4);
    gl2 g;
    do {
      g.c0 = chal_challenge<MODE>(c, K);
      g.c1 = chal_challenge<MODE>(c, K);
    } while (g.c1 == 0);
    chal[FRI_GAMMA_AT] = g.c0;
    chal[FRI_GAMMA_AT + 1] = g.c1;
  } else if (phase == 4 || phase == 8) {
    chal_load(c, state);
    chal_observe_span<MODE>(c, K, commit_cap, phase == 4 ? 4 : 4 * G.n_oracles);
    chal[0] = chal_challenge<MODE>(c, K);
    chal[1] = chal_challenge<MODE>(c, K);
  } else if (phase == 1) {
    chal_load(c, state);
    chal_observe_span<MODE>(c, K, proof + G.off_caps[layer], 4ull << G.cap_h[layer]);
    chal[2 + 2 * layer] = chal_challenge<MODE>(c, K);
    chal[3 + 2 * layer] = chal_challenge<MODE>(c, K);
  } else if (phase == 5) {
    chal_load(c, state);
    chal_observe_span<MODE>(c, K, proof + G.off_final, 2ull << G.final_log);
    chal_observe<MODE>(c, K, G.pow_bits);  // (a buffer this fills is duplexed here, once: a candidate is one permutation either way)
    chal[FRI_POW_AT] = ~0ull;              // the search's minimum and its counter start here, not in a launch of their own
    chal[FRI_POW_AT + 1] = 0;
  } else {
    chal_load(c, state);
    if (phase == 6) {
      const uint64_t nonce = chal[FRI_POW_AT];  // (2^64 - 1 if the search gave up: the verifier rejects it)
      proof[G.off_nonce] = nonce;
      chal_observe<MODE>(c, K, nonce);
      (void)chal_challenge<MODE>(c, K);  // r, consumed: the indices come from the remaining output words
    } else {
      chal_observe_span<MODE>(c, K, proof + G.off_final, 2ull << G.final_log);
    }
    const uint64_t mask = (1ull << G.log_n) - 1;
    for (uint32_t q = 0; q < G.n_queries; q++) {
      uint64_t i = chal_challenge<MODE>(c, K) & mask;
      proof[G.off_indices + q] = i;
      uint32_t lg = G.log_n;
      for (uint32_t l = 0; l < G.n_layers; l++) {
        lg -= G.bits[l];
        i &= (1ull << lg) - 1;
        qidx[(uint64_t)l * G.n_queries + q] = i;
      }
    }
  }
  chal_store(c, state);
}

// The constraint challenge of set 3 (include/tmx.h "the round constraints of the SHA-256 tables"), one lane, a kernel of its own so that
// k_fri_transcript keeps its registers: a fresh duplex over 2^33, the five words obs (set id 3, log_n, log_blowup, cap_height, n_proofs),
// the table cap, then the helper cap (cap_words words each) -> gamma, drawn as phase 9 draws it.
struct AirShaObs { uint32_t v[5]; };
template <int MODE>
__global__ __launch_bounds__(64) void k_air_sha_gamma(const uint64_t* __restrict__ consts, AirShaObs obs, uint32_t cap_words,
                                                      const uint64_t* __restrict__ cap, const uint64_t* __restrict__ cap_helper,
                                                      uint64_t* __restrict__ state, uint64_t* __restrict__ chal) {
  if (threadIdx.x) return;
  const PosConsts K = pos_consts(consts);
  FriChal c;
  chal_init(c);
  chal_observe<MODE>(c, K, 1ull << 33);
  for (int k = 0; k < 5; k++) chal_observe<MODE>(c, K, obs.v[k]);
  chal_observe_span<MODE>(c, K, cap, cap_words);
  chal_observe_span<MODE>(c, K, cap_helper, cap_words);
  gl2 g;
  do {
    g.c0 = chal_challenge<MODE>(c, K);
    g.c1 = chal_challenge<MODE>(c, K);
  } while (g.c1 == 0);
  chal[FRI_GAMMA_AT] = g.c0;
  chal[FRI_GAMMA_AT + 1] = g.c1;
  chal_store(c, state);
}

// The constraint challenge of set 6 (include/tmx.h "the SHA-256 tables' link to Level-1"): k_air_sha_gamma's form with a third span, the
// four words of the public table's digest.  A kernel of its own beside it: k_air_sha_gamma and k_fri_transcript stay as they are.
template <int MODE>
__global__ __launch_bounds__(64) void k_air_link_gamma(const uint64_t* __restrict__ consts, AirShaObs obs, uint32_t cap_words,
                                                       const uint64_t* __restrict__ cap, const uint64_t* __restrict__ cap_helper,
                                                       const uint64_t* __restrict__ digest, uint64_t* __restrict__ state,
                                                       uint64_t* __restrict__ chal) {
  if (threadIdx.x) return;
  const PosConsts K = pos_consts(consts);
  FriChal c;
  chal_init(c);
  chal_observe<MODE>(c, K, 1ull << 33);
  for (int k = 0; k < 5; k++) chal_observe<MODE>(c, K, obs.v[k]);
  chal_observe_span<MODE>(c, K, cap, cap_words);
  chal_observe_span<MODE>(c, K, cap_helper, cap_words);
  chal_observe_span<MODE>(c, K, digest, 4);
  gl2 g;
  do {
    g.c0 = chal_challenge<MODE>(c, K);
    g.c1 = chal_challenge<MODE>(c, K);
  } while (g.c1 == 0);
  chal[FRI_GAMMA_AT] = g.c0;
  chal[FRI_GAMMA_AT + 1] = g.c1;
  chal_store(c, state);
}

// The proof-of-work search (include/tmx.h "proof of work"), the one wide piece of the transcript: every candidate is one permutation of the
// duplex phase 5 left in `state` (12 words and the n_in <= 7 pending input words, uniform across the grid: scalar loads) with the
// candidate as the next input word; it satisfies the condition if output word 7, the one challenge() pops, has pow_bits leading zero bits.
// Lane t of a grid of G lanes tries t, t + G, t + 2 G, ...; a hit is a 64-bit atomic minimum on pow[0], and a lane stops when its next
// candidate lies above the current minimum (one relaxed load per round) or at the bound 2^(pow_bits + FRI_POW_SLACK_BITS) <= 2^30.  The
// minimum over all hits is the smallest satisfying nonce whatever order the workgroups run in: every candidate below it is evaluated by
// its lane before that lane stops, and no workgroup waits for another.  pow[1] += the candidates evaluated, one add per wave (it depends
// on timing: rounds in flight finish).
template <int MODE>
__global__ __launch_bounds__(256, 4) void k_fri_grind(const uint64_t* __restrict__ consts, uint32_t pow_bits, const uint64_t* __restrict__ state,
                                                   uint64_t* __restrict__ pow) {
  const PosConsts K = pos_consts(consts);
  const uint32_t n_in = (uint32_t)state[28];
  uint64_t base[12];
#pragma unroll
  for (int k = 0; k < 12; k++) base[k] = state[k];
#pragma unroll
  for (uint32_t k = 0; k < 8; k++)
    if (k < n_in) base[k] = state[12 + k];
  const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x, bound = 1ull << (pow_bits + FRI_POW_SLACK_BITS);
  uint32_t evaluated = 0;
  for (uint64_t cand = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; cand < bound; cand += lanes) {
    if (cand > __hip_atomic_load(pow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    uint64_t s[12];
#pragma unroll
    for (uint32_t k = 0; k < 12; k++) s[k] = k == n_in ? cand : base[k];
    pos_permute<MODE>(s, K);
    evaluated++;
    if ((gl_canon(s[7]) >> (64 - pow_bits)) == 0) __hip_atomic_fetch_min(pow, cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) evaluated += __shfl_down(evaluated, off);
  if ((threadIdx.x & 63) == 0 && evaluated) __hip_atomic_fetch_add(pow + 1, (uint64_t)evaluated, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int B>
__device__ __forceinline__ gl2 fri_fold_row(const uint64_t* __restrict__ row, uint64_t xinv0, uint64_t g, gl2 beta) {
  gl2 v[1 << B];
#pragma unroll
  for (int j = 0; j < (1 << B); j++) v[j] = {gl_canon(row[j]), gl_canon(row[(1 << B) + j])};
  return fri_fold_leaf<B>(v, xinv0, g, beta);
}

// The verifier: one workgroup, lane 0 re-derives the transcript from the proof and the caller's commit cap (alpha, every beta_l, the
// expected indices), then one thread per query walks its openings (include/tmx.h "query q").  Latency-bound like k_merkle_verify.
// DEEP: `proof` is the FRI part of a DEEP proof, `open` its openings section and `root` the root of the openings tree (enqueued before);
// the transcript starts with zeta and the root, the whole workgroup forms Y_0, Y_1 from the openings and checks their padding, and a
// query's v_0 is the DEEP layer 0 at its point instead of the plain combination.
// G.pow_bits != 0 (a grinding proof): lane 0 also observes pow_bits and the nonce word and draws r in front of the indices; every query is
// rejected if the nonce is not canonical or r has fewer than pow_bits leading zero bits.
// BATCH (the mixed-size batch proof): `cap` is the K caps concatenated, `proof` the whole proof (its offsets are absolute), `root` the K
// openings roots.  The workgroup forms the Y sums group by group; a query checks every oracle's row at idx mod M_k against its cap, forms
// Q^(g) of every group from the opened rows at the oracle's OWN point s w_k^(idx mod M_k), starts from Q^(0) and adds beta_l^(a_l) Q^(g)
// behind the fold of the layer that group g enters.
template <int MODE, bool DEEP, bool BATCH>
__global__ __launch_bounds__(FRI_MAX_QUERIES) void k_fri_verify(const uint64_t* __restrict__ consts, FriGeom G, const uint64_t* __restrict__ cap,
                                                                const uint64_t* __restrict__ proof, const uint64_t* __restrict__ open,
                                                                const uint64_t* __restrict__ root, uint32_t* __restrict__ ok) {
  __shared__ uint64_t s_chal[2 + 2 * FRI_MAX_LAYERS], s_idx[FRI_MAX_QUERIES];
  __shared__ uint64_t s_deep[DEEP || BATCH ? 4 : 1][DEEP || BATCH ? FRI_MAX_QUERIES : 1], s_z[DEEP || BATCH ? 4 : 1];
  __shared__ uint64_t s_y[BATCH ? FRI_MAX_ORACLES : 1][4];
  __shared__ uint32_t s_pow_ok;
  const PosConsts K = pos_consts(consts);
  if (threadIdx.x == 0) {
    FriChal c;
    if constexpr (BATCH) {
      const gl2 z = chal_start_batch<MODE>(c, K, G, cap);
      s_z[0] = z.c0;
      s_z[1] = z.c1;
      chal_observe_span<MODE>(c, K, root, 4 * G.n_oracles);
    } else if constexpr (DEEP) {
      const gl2 z = chal_start_deep<MODE>(c, K, G, cap);
      s_z[0] = z.c0;
      s_z[1] = z.c1;
      chal_observe_span<MODE>(c, K, root, 4);
    } else {
      chal_start<MODE>(c, K, G, cap);
    }
    s_chal[0] = chal_challenge<MODE>(c, K);
    s_chal[1] = chal_challenge<MODE>(c, K);
    for (uint32_t l = 0; l < G.n_layers; l++) {
      chal_observe_span<MODE>(c, K, proof + G.off_caps[l], 4ull << G.cap_h[l]);
      s_chal[2 + 2 * l] = chal_challenge<MODE>(c, K);
      s_chal[3 + 2 * l] = chal_challenge<MODE>(c, K);
    }
    chal_observe_span<MODE>(c, K, proof + G.off_final, 2ull << G.final_log);
    bool pow_ok = true;
    if (G.pow_bits) {
      chal_observe<MODE>(c, K, G.pow_bits);
      const uint64_t nonce = proof[G.off_nonce];
      chal_observe<MODE>(c, K, nonce);
      pow_ok = nonce < GL_P && (chal_challenge<MODE>(c, K) >> (64 - G.pow_bits)) == 0;
    }
    s_pow_ok = pow_ok ? 1u : 0u;
    for (uint32_t q = 0; q < G.n_queries; q++) s_idx[q] = chal_challenge<MODE>(c, K) & ((1ull << G.log_n) - 1);
  }
  __syncthreads();
  gl2 Y0 = {0, 0}, Y1 = {0, 0};
  bool pad_ok = true;
  if constexpr (DEEP) {
    // every thread: its share of Y_k = sum_c alpha^c y_(c,k) (c = t mod the block), a tree sum in LDS; and the padding rows must be zero
    const uint32_t t = threadIdx.x;
    const uint64_t Rr = 1ull << G.log_r;
    const gl2 alpha = {s_chal[0], s_chal[1]};
    gl2 ap = gl2_pow(alpha, t);
    const gl2 step = gl2_pow(alpha, FRI_MAX_QUERIES);
    for (uint32_t c = t; c < G.n_cols; c += FRI_MAX_QUERIES) {
      Y0 = gl2_add(Y0, gl2_mul(ap, {gl_canon(open[c]), gl_canon(open[Rr + c])}));
      Y1 = gl2_add(Y1, gl2_mul(ap, {gl_canon(open[2 * Rr + c]), gl_canon(open[3 * Rr + c])}));
      ap = gl2_mul(ap, step);
    }
    bool pad_bad = false;
    for (uint64_t r = G.n_cols + t; r < Rr; r += FRI_MAX_QUERIES)
      pad_bad = pad_bad || open[r] || open[Rr + r] || open[2 * Rr + r] || open[3 * Rr + r];
    s_deep[0][t] = Y0.c0; s_deep[1][t] = Y0.c1; s_deep[2][t] = Y1.c0; s_deep[3][t] = Y1.c1;
    pad_ok = !__syncthreads_or(pad_bad);
    for (uint32_t h = FRI_MAX_QUERIES / 2; h; h >>= 1) {
      if (t < h)
#pragma unroll
        for (int k = 0; k < 4; k++) s_deep[k][t] = gl_add(s_deep[k][t], s_deep[k][t + h]);
      __syncthreads();
    }
    Y0 = {s_deep[0][0], s_deep[1][0]};
    Y1 = {s_deep[2][0], s_deep[3][0]};
  }
  if constexpr (BATCH) {
    // group by group: every thread's share of the group's Y sums (alpha^(off_k + c) y_(k,c,j)) and the padding rows of its blocks
    const uint32_t t = threadIdx.x;
    const gl2 alpha = {s_chal[0], s_chal[1]};
    const gl2 step = gl2_pow(alpha, FRI_MAX_QUERIES);
    bool pad_bad = false;
    for (uint32_t g = 0; g < G.n_groups; g++) {
      gl2 y0 = {0, 0}, y1 = {0, 0};
      for (uint32_t k = 0; k < G.n_oracles; k++) {
        if (G.o_group[k] != g) continue;
        const uint64_t Rr = 1ull << G.o_log_r[k];
        const uint64_t* ob = proof + G.o_off_open[k];
        gl2 ap = gl2_pow(alpha, (uint64_t)G.o_alpha_off[k] + t);
        for (uint32_t c = t; c < G.o_n_cols[k]; c += FRI_MAX_QUERIES) {
          y0 = gl2_add(y0, gl2_mul(ap, {gl_canon(ob[c]), gl_canon(ob[Rr + c])}));
          y1 = gl2_add(y1, gl2_mul(ap, {gl_canon(ob[2 * Rr + c]), gl_canon(ob[3 * Rr + c])}));
          ap = gl2_mul(ap, step);
        }
        for (uint64_t r = G.o_n_cols[k] + t; r < Rr; r += FRI_MAX_QUERIES)
          pad_bad = pad_bad || ob[r] || ob[Rr + r] || ob[2 * Rr + r] || ob[3 * Rr + r];
      }
      s_deep[0][t] = y0.c0; s_deep[1][t] = y0.c1; s_deep[2][t] = y1.c0; s_deep[3][t] = y1.c1;
      __syncthreads();
      for (uint32_t h = FRI_MAX_QUERIES / 2; h; h >>= 1) {
        if (t < h)
#pragma unroll
          for (int k = 0; k < 4; k++) s_deep[k][t] = gl_add(s_deep[k][t], s_deep[k][t + h]);
        __syncthreads();
      }
      if (t < 4) s_y[g][t] = s_deep[t][0];
      __syncthreads();
    }
    pad_ok = !__syncthreads_or(pad_bad);
  }
  const uint32_t q = threadIdx.x;
  if (q >= G.n_queries) return;
  uint64_t i = s_idx[q];
  bool good = proof[G.off_indices + q] == i && pad_ok && s_pow_ok;
  const gl2 alpha = {s_chal[0], s_chal[1]};
  gl2 v = {0, 0}, ap = {1, 0};
  gl2 Qg[BATCH ? FRI_MAX_ORACLES : 1];
  if constexpr (BATCH) {
    // every oracle's row against its own cap; F of every group (the alpha powers run on across the oracles: alpha^(off_k + c))
    for (uint32_t k = 0; k < G.n_oracles; k++) {
      const uint32_t lgk = G.o_log_n[k], nck = G.o_n_cols[k], plk = lgk - G.o_cap_h[k];
      const uint64_t ik = i & ((1ull << lgk) - 1);
      const uint64_t* row = proof + G.o_off_rows[k] + (uint64_t)q * nck;
      good = merkle_leads_to_cap<MODE>(K, row, nck, proof + G.o_off_paths[k] + (uint64_t)q * plk * 4, plk, ik, cap + G.o_cap_at[k]) && good;
      if (k == 0 || G.o_group[k] != G.o_group[k - 1]) v = {0, 0};
      for (uint32_t c = 0; c < nck; c++) {
        v = gl2_add(v, gl2_scale(ap, gl_canon(row[c])));
        ap = gl2_mul(ap, alpha);
      }
      Qg[G.o_group[k]] = v;
    }
    // (ap = alpha^C here) the quotients, each at its group's own point s w_k^(idx mod M_k) and with its own omega_(N_k)
    const gl2 z0 = {s_z[0], s_z[1]};
    for (uint32_t k = 0; k < G.n_oracles; k++) {
      if (k && G.o_group[k] == G.o_group[k - 1]) continue;
      const uint32_t g = G.o_group[k];
      const uint64_t ik = i & ((1ull << G.o_log_n[k]) - 1);
      Qg[g] = deep_layer0(Qg[g], gl_mul(G.s0, gl_pow(G.o_w[k], ik)), z0, gl2_scale(z0, G.o_omega[k]), {s_y[g][0], s_y[g][1]}, {s_y[g][2], s_y[g][3]}, ap);
    }
    v = Qg[0];
  } else {
    const uint32_t pl0 = G.log_n - G.cap_height;
    const uint64_t* row = proof + G.off_init_rows + (uint64_t)q * G.n_cols;
    good = merkle_leads_to_cap<MODE>(K, row, G.n_cols, proof + G.off_init_paths + (uint64_t)q * pl0 * 4, pl0, i, cap) && good;
    for (uint32_t c = 0; c < G.n_cols; c++) {
      v = gl2_add(v, gl2_scale(ap, gl_canon(row[c])));
      ap = gl2_mul(ap, alpha);
    }
    if constexpr (DEEP) {  // (ap = alpha^n_cols here)
      const gl2 z0 = {s_z[0], s_z[1]};
      v = deep_layer0(v, gl_mul(G.s0, gl_pow(G.w0, i)), z0, gl2_scale(z0, G.omega_n), Y0, Y1, ap);
    }
  }
  uint32_t lg = G.log_n;
  for (uint32_t l = 0; l < G.n_layers; l++) {
    const uint32_t b = G.bits[l], a = 1u << b, lgn = lg - b, pl = lgn - G.cap_h[l];
    const uint64_t r = i & ((1ull << lgn) - 1), j = i >> lgn;
    const uint64_t* lr = proof + G.off_rows[l] + (uint64_t)q * 2 * a;
    good = good && gl_canon(lr[j]) == v.c0 && gl_canon(lr[a + j]) == v.c1;
    good = merkle_leads_to_cap<MODE>(K, lr, 2 * a, proof + G.off_paths[l] + (uint64_t)q * pl * 4, pl, r, proof + G.off_caps[l]) && good;
    const uint64_t xinv0 = gl_mul(G.s_inv[l], gl_pow(G.w_inv[l], r));
    const gl2 beta = {s_chal[2 + 2 * l], s_chal[3 + 2 * l]};
    switch (b) {
      case 1: v = fri_fold_row<1>(lr, xinv0, G.g[l], beta); break;
      case 2: v = fri_fold_row<2>(lr, xinv0, G.g[l], beta); break;
      case 3: v = fri_fold_row<3>(lr, xinv0, G.g[l], beta); break;
      default: v = fri_fold_row<4>(lr, xinv0, G.g[l], beta); break;
    }
    if constexpr (BATCH) {
      if (G.enter[l]) {  // the group that has layer l + 1's size joins, scaled by beta^(2^b)
        gl2 bp = beta;
        for (uint32_t k = 0; k < b; k++) bp = gl2_mul(bp, bp);
        v = gl2_add(v, gl2_mul(bp, Qg[G.enter[l]]));
      }
    }
    i = r;
    lg = lgn;
  }
  const uint64_t x = gl_mul(G.s_fin, gl_pow(G.w_fin, i));
  const uint64_t* coef = proof + G.off_final;
  gl2 e = {0, 0};
  for (int k = (1 << G.final_log) - 1; k >= 0; k--) e = gl2_add(gl2_scale(e, x), {gl_canon(coef[2 * k]), gl_canon(coef[2 * k + 1])});
  ok[q] = (good && gl2_eq(e, v)) ? 1u : 0u;
}

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

int launch_poseidon_permute(const void* d_consts, int mode, uint32_t n, const void* d_in, void* d_out, void* stream) {
  if (n == 0) return 0;
  const dim3 grid((n + 255) / 256);
  if (mode == POS_MODE_MERGE3)
    hipLaunchKernelGGL(k_poseidon_permute<POS_MODE_MERGE3>, grid, dim3(256), 0, S_(stream), reinterpret_cast<const uint64_t*>(d_consts), n,
                       reinterpret_cast<const uint64_t*>(d_in), reinterpret_cast<uint64_t*>(d_out));
  else if (mode == POS_MODE_SMALL)
    hipLaunchKernelGGL(k_poseidon_permute<POS_MODE_SMALL>, grid, dim3(256), 0, S_(stream), reinterpret_cast<const uint64_t*>(d_consts), n,
                       reinterpret_cast<const uint64_t*>(d_in), reinterpret_cast<uint64_t*>(d_out));
  else
    hipLaunchKernelGGL(k_poseidon_permute<POS_MODE_GENERAL>, grid, dim3(256), 0, S_(stream), reinterpret_cast<const uint64_t*>(d_consts), n,
                       reinterpret_cast<const uint64_t*>(d_in), reinterpret_cast<uint64_t*>(d_out));
  return (int)hipGetLastError();
}
int launch_poseidon_leaves(const void* d_consts, int mode, uint32_t log_n, uint32_t n_cols, const void* d_cols, void* d_digests, void* stream) {
  const uint64_t n = 1ull << log_n;
  const dim3 grid((uint32_t)((n + 255) / 256));
  if (mode == POS_MODE_MERGE3)
    hipLaunchKernelGGL(k_poseidon_leaves<POS_MODE_MERGE3>, grid, dim3(256), 0, S_(stream), reinterpret_cast<const uint64_t*>(d_consts), log_n, n_cols,
                       reinterpret_cast<const uint64_t*>(d_cols), reinterpret_cast<uint64_t*>(d_digests));
  else if (mode == POS_MODE_SMALL)
    hipLaunchKernelGGL(k_poseidon_leaves<POS_MODE_SMALL>, grid, dim3(256), 0, S_(stream), reinterpret_cast<const uint64_t*>(d_consts), log_n, n_cols,
                       reinterpret_cast<const uint64_t*>(d_cols), reinterpret_cast<uint64_t*>(d_digests));
  else
    hipLaunchKernelGGL(k_poseidon_leaves<POS_MODE_GENERAL>, grid, dim3(256), 0, S_(stream), reinterpret_cast<const uint64_t*>(d_consts), log_n, n_cols,
                       reinterpret_cast<const uint64_t*>(d_cols), reinterpret_cast<uint64_t*>(d_digests));
  return (int)hipGetLastError();
}
int launch_poseidon_leaves_chunk(const void* d_consts, int mode, uint32_t log_n, uint32_t n_cols, const void* d_cols, bool first, bool last,
                                 void* d_state, void* d_digests, void* stream) {
  const uint64_t n = 1ull << log_n;
  const dim3 grid((uint32_t)((n + 255) / 256));
  const uint64_t* K = reinterpret_cast<const uint64_t*>(d_consts);
  const uint64_t* cols = reinterpret_cast<const uint64_t*>(d_cols);
  uint64_t* state = reinterpret_cast<uint64_t*>(d_state);
  uint64_t* dig = reinterpret_cast<uint64_t*>(d_digests);
  const uint32_t f = first ? 1u : 0u, l = last ? 1u : 0u;
  if (mode == POS_MODE_MERGE3)
    hipLaunchKernelGGL(k_poseidon_leaves_chunk<POS_MODE_MERGE3>, grid, dim3(256), 0, S_(stream), K, log_n, n_cols, cols, f, l, state, dig);
  else if (mode == POS_MODE_SMALL)
    hipLaunchKernelGGL(k_poseidon_leaves_chunk<POS_MODE_SMALL>, grid, dim3(256), 0, S_(stream), K, log_n, n_cols, cols, f, l, state, dig);
  else
    hipLaunchKernelGGL(k_poseidon_leaves_chunk<POS_MODE_GENERAL>, grid, dim3(256), 0, S_(stream), K, log_n, n_cols, cols, f, l, state, dig);
  return (int)hipGetLastError();
}
int launch_poseidon_level(const void* d_consts, int mode, uint64_t n_out, const void* d_in, void* d_out, void* stream) {
  if (n_out == 0) return 0;
  const dim3 grid((uint32_t)((n_out + 255) / 256));
  if (mode == POS_MODE_MERGE3)
    hipLaunchKernelGGL(k_poseidon_level<POS_MODE_MERGE3>, grid, dim3(256), 0, S_(stream), reinterpret_cast<const uint64_t*>(d_consts), n_out,
                       reinterpret_cast<const uint64_t*>(d_in), reinterpret_cast<uint64_t*>(d_out));
  else if (mode == POS_MODE_SMALL)
    hipLaunchKernelGGL(k_poseidon_level<POS_MODE_SMALL>, grid, dim3(256), 0, S_(stream), reinterpret_cast<const uint64_t*>(d_consts), n_out,
                       reinterpret_cast<const uint64_t*>(d_in), reinterpret_cast<uint64_t*>(d_out));
  else
    hipLaunchKernelGGL(k_poseidon_level<POS_MODE_GENERAL>, grid, dim3(256), 0, S_(stream), reinterpret_cast<const uint64_t*>(d_consts), n_out,
                       reinterpret_cast<const uint64_t*>(d_in), reinterpret_cast<uint64_t*>(d_out));
  return (int)hipGetLastError();
}

int launch_merkle_open(uint32_t log_n, uint32_t n_cols, const void* d_cols, uint32_t path_len, const void* d_levels, uint32_t n_queries,
                       const void* d_idx, void* d_rows, void* d_paths, bool split, void* stream) {
  if (n_queries == 0) return 0;
  // column blocks per query: all of the row's columns at once up to 64 blocks (16 k columns), then a grid-stride loop
  const uint32_t col_blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n_cols + 255) / 256, 64);
  const uint64_t* cols = reinterpret_cast<const uint64_t*>(d_cols);
  const uint64_t* lv = reinterpret_cast<const uint64_t*>(d_levels);
  const uint64_t* idx = reinterpret_cast<const uint64_t*>(d_idx);
  uint64_t* rows = reinterpret_cast<uint64_t*>(d_rows);
  uint64_t* paths = path_len ? reinterpret_cast<uint64_t*>(d_paths) : nullptr;
  if (!split || !paths) {
    hipLaunchKernelGGL(k_merkle_open, dim3(n_queries, col_blocks), dim3(256), 0, S_(stream), log_n, n_cols, cols, path_len, lv, idx, rows, paths);
  } else {
    hipLaunchKernelGGL(k_merkle_open, dim3(n_queries, col_blocks), dim3(256), 0, S_(stream), log_n, n_cols, cols, 0u, lv, idx, rows, nullptr);
    hipLaunchKernelGGL(k_merkle_open, dim3(n_queries, 1), dim3(256), 0, S_(stream), log_n, n_cols, cols, path_len, lv, idx, nullptr, paths);
  }
  return (int)hipGetLastError();
}
int launch_merkle_open_chunk(uint32_t log_n, uint32_t n_cols, const void* d_cols, uint32_t n_queries, const void* d_idx, void* d_rows,
                             uint64_t row_stride, void* stream) {
  if (n_queries == 0 || n_cols == 0) return 0;
  const uint32_t col_blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n_cols + 255) / 256, 64);
  hipLaunchKernelGGL(k_merkle_open_chunk, dim3(n_queries, col_blocks), dim3(256), 0, S_(stream), log_n, n_cols,
                     reinterpret_cast<const uint64_t*>(d_cols), reinterpret_cast<const uint64_t*>(d_idx), reinterpret_cast<uint64_t*>(d_rows), row_stride);
  return (int)hipGetLastError();
}
int launch_merkle_verify(const void* d_consts, int mode, uint32_t n_cols, uint32_t path_len, uint32_t n_queries, const void* d_cap, const void* d_idx,
                         const void* d_rows, const void* d_paths, void* d_ok, void* stream) {
  if (n_queries == 0) return 0;
  const dim3 grid((n_queries + 63) / 64);
  const uint64_t* K = reinterpret_cast<const uint64_t*>(d_consts);
  const uint64_t* cap = reinterpret_cast<const uint64_t*>(d_cap);
  const uint64_t* idx = reinterpret_cast<const uint64_t*>(d_idx);
  const uint64_t* rows = reinterpret_cast<const uint64_t*>(d_rows);
  const uint64_t* paths = reinterpret_cast<const uint64_t*>(d_paths);
  uint32_t* ok = reinterpret_cast<uint32_t*>(d_ok);
  if (mode == POS_MODE_MERGE3)
    hipLaunchKernelGGL(k_merkle_verify<POS_MODE_MERGE3>, grid, dim3(64), 0, S_(stream), K, n_cols, path_len, n_queries, cap, idx, rows, paths, ok);
  else if (mode == POS_MODE_SMALL)
    hipLaunchKernelGGL(k_merkle_verify<POS_MODE_SMALL>, grid, dim3(64), 0, S_(stream), K, n_cols, path_len, n_queries, cap, idx, rows, paths, ok);
  else
    hipLaunchKernelGGL(k_merkle_verify<POS_MODE_GENERAL>, grid, dim3(64), 0, S_(stream), K, n_cols, path_len, n_queries, cap, idx, rows, paths, ok);
  return (int)hipGetLastError();
}

template <int MODE>
static void fri_transcript_launch(const uint64_t* K, const FriGeom& G, int phase, uint32_t layer, const uint64_t* commit_cap, uint64_t* proof,
                                  uint64_t* state, uint64_t* chal, uint64_t* qidx, hipStream_t s) {
  hipLaunchKernelGGL(k_fri_transcript<MODE>, dim3(1), dim3(64), 0, s, K, G, phase, layer, commit_cap, proof, state, chal, qidx);
}
int launch_fri_transcript(const void* d_consts, int mode, const FriGeom& G, int phase, uint32_t layer, const void* d_commit_cap, void* d_proof,
                          void* d_state, void* d_chal, void* d_qidx, void* stream) {
  const uint64_t* K = reinterpret_cast<const uint64_t*>(d_consts);
  const uint64_t* cap = reinterpret_cast<const uint64_t*>(d_commit_cap);
  uint64_t* proof = reinterpret_cast<uint64_t*>(d_proof);
  uint64_t* st = reinterpret_cast<uint64_t*>(d_state);
  uint64_t* ch = reinterpret_cast<uint64_t*>(d_chal);
  uint64_t* qi = reinterpret_cast<uint64_t*>(d_qidx);
  if (mode == POS_MODE_MERGE3) fri_transcript_launch<POS_MODE_MERGE3>(K, G, phase, layer, cap, proof, st, ch, qi, S_(stream));
  else if (mode == POS_MODE_SMALL) fri_transcript_launch<POS_MODE_SMALL>(K, G, phase, layer, cap, proof, st, ch, qi, S_(stream));
  else fri_transcript_launch<POS_MODE_GENERAL>(K, G, phase, layer, cap, proof, st, ch, qi, S_(stream));
  return (int)hipGetLastError();
}
int launch_air_sha_gamma(const void* d_consts, int mode, const uint32_t obs[5], uint32_t cap_words, const void* d_cap, const void* d_cap_helper,
                         void* d_state, void* d_chal, void* stream) {
  const uint64_t* K = reinterpret_cast<const uint64_t*>(d_consts);
  const uint64_t* cap = reinterpret_cast<const uint64_t*>(d_cap);
  const uint64_t* cap_h = reinterpret_cast<const uint64_t*>(d_cap_helper);
  uint64_t* st = reinterpret_cast<uint64_t*>(d_state);
  uint64_t* ch = reinterpret_cast<uint64_t*>(d_chal);
  AirShaObs o;
  for (int k = 0; k < 5; k++) o.v[k] = obs[k];
  if (mode == POS_MODE_MERGE3) hipLaunchKernelGGL(k_air_sha_gamma<POS_MODE_MERGE3>, dim3(1), dim3(64), 0, S_(stream), K, o, cap_words, cap, cap_h, st, ch);
  else if (mode == POS_MODE_SMALL) hipLaunchKernelGGL(k_air_sha_gamma<POS_MODE_SMALL>, dim3(1), dim3(64), 0, S_(stream), K, o, cap_words, cap, cap_h, st, ch);
  else hipLaunchKernelGGL(k_air_sha_gamma<POS_MODE_GENERAL>, dim3(1), dim3(64), 0, S_(stream), K, o, cap_words, cap, cap_h, st, ch);
  return (int)hipGetLastError();
}
int launch_air_link_gamma(const void* d_consts, int mode, const uint32_t obs[5], uint32_t cap_words, const void* d_cap, const void* d_cap_helper,
                          const void* d_digest, void* d_state, void* d_chal, void* stream) {
  const uint64_t* K = reinterpret_cast<const uint64_t*>(d_consts);
  const uint64_t* cap = reinterpret_cast<const uint64_t*>(d_cap);
  const uint64_t* cap_h = reinterpret_cast<const uint64_t*>(d_cap_helper);
  const uint64_t* dg = reinterpret_cast<const uint64_t*>(d_digest);
  uint64_t* st = reinterpret_cast<uint64_t*>(d_state);
  uint64_t* ch = reinterpret_cast<uint64_t*>(d_chal);
  AirShaObs o;
  for (int k = 0; k < 5; k++) o.v[k] = obs[k];
  if (mode == POS_MODE_MERGE3) hipLaunchKernelGGL(k_air_link_gamma<POS_MODE_MERGE3>, dim3(1), dim3(64), 0, S_(stream), K, o, cap_words, cap, cap_h, dg, st, ch);
  else if (mode == POS_MODE_SMALL) hipLaunchKernelGGL(k_air_link_gamma<POS_MODE_SMALL>, dim3(1), dim3(64), 0, S_(stream), K, o, cap_words, cap, cap_h, dg, st, ch);
  else hipLaunchKernelGGL(k_air_link_gamma<POS_MODE_GENERAL>, dim3(1), dim3(64), 0, S_(stream), K, o, cap_words, cap, cap_h, dg, st, ch);
  return (int)hipGetLastError();
}
// The grid of the search: one lane per expected candidate (2^pow_bits: a 4-bit search is one workgroup), at most four 256-thread workgroups
// per compute unit: the four waves per SIMD the kernel's launch bounds keep its registers within (docs/kernels.md).
int launch_fri_grind(const void* d_consts, int mode, uint32_t pow_bits, const void* d_state, void* d_pow, void* stream) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
    return (int)hipErrorInvalidDevice;
  const uint64_t want = std::max<uint64_t>(1, (1ull << pow_bits) / 256);
  const dim3 grid((uint32_t)std::min<uint64_t>(want, 4ull * (uint64_t)cus)), block(256);
  const uint64_t* K = reinterpret_cast<const uint64_t*>(d_consts);
  const uint64_t* st = reinterpret_cast<const uint64_t*>(d_state);
  uint64_t* pw = reinterpret_cast<uint64_t*>(d_pow);
  if (mode == POS_MODE_MERGE3) hipLaunchKernelGGL(k_fri_grind<POS_MODE_MERGE3>, grid, block, 0, S_(stream), K, pow_bits, st, pw);
  else if (mode == POS_MODE_SMALL) hipLaunchKernelGGL(k_fri_grind<POS_MODE_SMALL>, grid, block, 0, S_(stream), K, pow_bits, st, pw);
  else hipLaunchKernelGGL(k_fri_grind<POS_MODE_GENERAL>, grid, block, 0, S_(stream), K, pow_bits, st, pw);
  return (int)hipGetLastError();
}
template <bool DEEP, bool BATCH = false>
static void fri_verify_launch(const uint64_t* K, int mode, const FriGeom& G, const uint64_t* cap, const uint64_t* proof, const uint64_t* open,
                              const uint64_t* root, uint32_t* ok, hipStream_t s) {
  const dim3 grid(1), block(FRI_MAX_QUERIES);
  if (mode == POS_MODE_MERGE3) hipLaunchKernelGGL((k_fri_verify<POS_MODE_MERGE3, DEEP, BATCH>), grid, block, 0, s, K, G, cap, proof, open, root, ok);
  else if (mode == POS_MODE_SMALL) hipLaunchKernelGGL((k_fri_verify<POS_MODE_SMALL, DEEP, BATCH>), grid, block, 0, s, K, G, cap, proof, open, root, ok);
  else hipLaunchKernelGGL((k_fri_verify<POS_MODE_GENERAL, DEEP, BATCH>), grid, block, 0, s, K, G, cap, proof, open, root, ok);
}
int launch_fri_verify(const void* d_consts, int mode, const FriGeom& G, const void* d_cap, const void* d_proof, const void* d_open, const void* d_root,
                      void* d_ok, void* stream) {
  const uint64_t* K = reinterpret_cast<const uint64_t*>(d_consts);
  const uint64_t* cap = reinterpret_cast<const uint64_t*>(d_cap);
  const uint64_t* proof = reinterpret_cast<const uint64_t*>(d_proof);
  const uint64_t* open = reinterpret_cast<const uint64_t*>(d_open);
  const uint64_t* root = reinterpret_cast<const uint64_t*>(d_root);
  uint32_t* ok = reinterpret_cast<uint32_t*>(d_ok);
  if (G.n_oracles) fri_verify_launch<false, true>(K, mode, G, cap, proof, open, root, ok, S_(stream));
  else if (G.deep) fri_verify_launch<true>(K, mode, G, cap, proof, open, root, ok, S_(stream));
  else fri_verify_launch<false>(K, mode, G, cap, proof, open, root, ok, S_(stream));
  return (int)hipGetLastError();
}

}  // namespace tmx
