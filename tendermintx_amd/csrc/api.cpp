// libtmx C ABI (include/tmx.h): context, device scratch, serializer program, launch sequence.
//
// Host side of the drop-in boundary: what SkipOffchainInputs::hint / StepOffchainInputs::hint
// (reference circuits/skip.rs:64-102, circuits/step.rs:56-89) do after the RPC/fixture fetch, expressed as
//   records -> [k_eddsa] -> [k_proof] -> [k_serialize] -> Goldilocks elements (+ tmx_report)
// on one HIP stream.  No CPU compute path exists here: without a usable HIP device every call fails.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kernels.h"
#include "air.h"
#include "fri.h"
#include "ntt.h"
#include "poseidon.h"
#include "trace.h"
#include "tmx.h"
#include "value.h"

using namespace tmx;

// why the last context-less call of this thread failed (tmx_comm_unique_id has no context to carry the text): tmx_last_error(NULL)
static thread_local std::string g_tls_err;

static_assert(sizeof(tmx_validator_rec) == VR_STRIDE, "validator record layout");
static_assert(sizeof(tmx_hashfield_rec) == HR_STRIDE, "hash-field record layout");
static_assert(sizeof(tmx_header_rec) == HDR_SIZE, "header record layout");
static_assert(sizeof(tmx_proof_rec) == PR_STRIDE, "proof record layout");
static_assert(sizeof(tmx_report) == 64, "report layout");
static_assert(offsetof(tmx_validator_rec, message_byte_length) == VR_OFF_MLEN, "mlen offset");
static_assert(offsetof(tmx_validator_rec, voting_power) == VR_OFF_POWER, "power offset");
static_assert(offsetof(tmx_hashfield_rec, validator_byte_length) == HR_OFF_VLEN, "vlen offset");
static_assert(offsetof(tmx_proof_rec, header_b) == PR_OFF_HDR_B, "header_b offset");
static_assert(TMX_N_MAX_LIMIT == TMX_N_LIMIT, "n_max limit");
static_assert(sizeof(tmx_validator_value) == VAL_VALIDATOR && sizeof(tmx_hashfield_value) == VAL_HASHFIELD, "typed value: lane structs");
static_assert(sizeof(tmx_skip_inputs_fixed) == VAL_FIXED_SKIP && sizeof(tmx_step_inputs_fixed) == VAL_FIXED_STEP, "typed value: fixed parts");
static_assert(sizeof(tmx_target_lane_derived) == VAL_LANE_T && sizeof(tmx_trusted_lane_derived) == VAL_LANE_R && sizeof(tmx_proof_derived) == VAL_PROOF_D,
              "typed value: derived structs");
static_assert(offsetof(tmx_validator_value, message_byte_length) == 220 && offsetof(tmx_validator_value, voting_power) == 224 &&
                  offsetof(tmx_validator_value, validator_byte_length) == 232 && offsetof(tmx_validator_value, signed_) == 236,
              "tmx_validator_value: k_pack_value writes these offsets");
static_assert(offsetof(tmx_target_lane_derived, eddsa_ok) == ED_OFF_OK && offsetof(tmx_target_lane_derived, marshalled) == TL_OFF_LT + LN_OFF_MARSHAL &&
                  offsetof(tmx_target_lane_derived, leaf_hash) == TL_OFF_LT + LN_OFF_LEAF && offsetof(tmx_target_lane_derived, flags) == TL_OFF_LT + LN_OFF_FLAGS &&
                  offsetof(tmx_target_lane_derived, total_prefix) == TL_OFF_LT + LN_OFF_TOT && offsetof(tmx_target_lane_derived, signed_prefix) == TL_OFF_LT + LN_OFF_ACC,
              "tmx_target_lane_derived mirrors the context's lane record");
static_assert(offsetof(tmx_trusted_lane_derived, flags) == LN_OFF_FLAGS && offsetof(tmx_trusted_lane_derived, matched_prefix) == LN_OFF_ACC, "tmx_trusted_lane_derived");
static_assert(offsetof(tmx_proof_derived, height_leaf) == PF_OFF_HLEAF - PF_OFF_PROOFD && offsetof(tmx_proof_derived, tally_target) == PF_OFF_TALLY_T - PF_OFF_PROOFD &&
                  offsetof(tmx_proof_derived, tally_trusted) == PF_OFF_TALLY_R - PF_OFF_PROOFD && offsetof(tmx_proof_derived, verdicts) == PF_OFF_VERDICTS - PF_OFF_PROOFD &&
                  offsetof(tmx_proof_derived, checks) == PF_OFF_CHECKS - PF_OFF_PROOFD && offsetof(tmx_proof_derived, all_ok) == PF_OFF_ALLOK - PF_OFF_PROOFD &&
                  offsetof(tmx_proof_derived, height) == PF_OFF_HEIGHT - PF_OFF_PROOFD,
              "tmx_proof_derived mirrors the context's per-proof record");

// ------------------------------------------------------------------------------------------------ element layout
// Declarative description of the witness row: hint section H in the field order of VerifySkipVariable<N> /
// VerifyStepVariable<N> (reference circuits/variables.rs:91-120) with the element widths of the plonky2x
// variable types (ByteVariable = 8 big-endian bits, U32/Variable/Bool = 1, U64 = 2 LE limbs, U256 = 8 LE limbs),
// followed by the derived section D (DESIGN.md "Witness layout").
namespace {

struct LutBuilder {  // offsets are relative to the section's single source record
  std::vector<uint32_t> v;
  void bytes(uint32_t off, uint32_t n) {  // ByteVariable: 8 elements per byte, most significant bit first
    for (uint32_t i = 0; i < n; i++)
      for (uint32_t k = 0; k < 8; k++) v.push_back(lut_field(W_BIT, off + i, 7 - k));
  }
  void u8(uint32_t off) { v.push_back(lut_field(W_U8, off, 0)); }
  void u16(uint32_t off) { v.push_back(lut_field(W_U16, off, 0)); }  // 2-aligned inside its dword
  void u32(uint32_t off) { v.push_back(lut_field(W_U32, off, 0)); }  // 4-aligned
  void u64(uint32_t off) { u32(off); u32(off + 4); }
  void u256(uint32_t off) { for (uint32_t k = 0; k < 8; k++) u32(off + 4 * k); }
  void flag0(uint32_t off) { v.push_back(lut_field(W_BIT, off, 0)); }
};

uint32_t tree_nodes(uint32_t n) {
  uint32_t c = 0;
  while (n > 1) { n = (n + 1) / 2; c += n; }
  return c;
}

// MerkleInclusionProofVariable<4, LEAF>: proof[4] (Bytes32 each) then leaf bytes  (variables.rs:58-62)
// (*aunts_at, *leaf_at: where the two fields start in the table, for the readers of the row that need them)
void emit_inclusion_proof(LutBuilder& L, int q, uint32_t leaf_src_off, uint32_t leaf_size, uint32_t* aunts_at, uint32_t* leaf_at) {
  *aunts_at = (uint32_t)L.v.size();
  L.bytes(PF_OFF_AUNTS + 128 * q, 128);
  *leaf_at = (uint32_t)L.v.size();
  L.bytes(leaf_src_off, leaf_size);
}
// derived: leaf hash + the four path nodes of proof q
void emit_proof_d(LutBuilder& L, int q) { L.bytes(PF_OFF_PROOFD + 160 * q, 160); }

struct Program {
  SerializeProgram sp;
  std::vector<uint32_t> lut;
  uint32_t mask_inputs = 0, mask_proof = 0, mask_final = 0, mask_tail = 0, mask_p1 = 0, mask_leaves = 0;  // sections by readiness: inputs only / after k_proof / after EdDSA / after k_verdict
  std::vector<uint32_t> seam_waves;  // indices of the spans that straddle a boundary (0xff entries of wave_sec)
  std::vector<uint8_t> wave_sec;  // per sp.span-element span of a row: its section, or 0xff if it straddles a boundary / the row end
  uint32_t hint_elems;
  uint32_t d1b_start = 0;  // first element of D.1b in a row (the EdDSA finish writes that section directly: RowOut)
  uint32_t mask_hint = 0, mask_derived = 0;  // sections of H / of D (tmx_witness_batch_opts: a caller may ask for one of them only)
  AirShaPublicGeom pub = {};  // where tmx_air_sha256_public_device reads in a row: recorded while the table is emitted (air.h)
  AirSha512PublicGeom pub512 = {};  // likewise for tmx_air_sha512_public_device: H.2 and the digest of D.1a
  uint32_t tail_dep_elem = 0;  // first element of a row whose value is written by the final checks (verdicts, check words, all_ok): the small-launch tail
};

Program build_program(int kind, uint32_t n) {
  Program P;
  std::memset(&P.sp, 0, sizeof P.sp);
  LutBuilder L;
  const bool skip = kind == TMX_KIND_SKIP;
  const uint32_t tn = tree_nodes(n);
  uint32_t elem = 0;
  // ready: 0 = needs only the input records, 1 = needs k_proof, 2 = needs the EdDSA kernels (and k_proof), 3 = needs k_verdict,
  // 4 = needs the leaves (k_leaves, or k_proof) and phase 1 (not k_ed_fin), 5 = needs only the leaves
  auto add_section = [&](uint32_t lane_elems, uint32_t n_lanes, uint32_t lut_off, uint32_t kind_, uint32_t src, int ready) {
    (ready == 0 ? P.mask_inputs : ready == 1 ? P.mask_proof : ready == 2 ? P.mask_final : ready == 4 ? P.mask_p1 : ready == 5 ? P.mask_leaves : P.mask_tail) |=
        1u << P.sp.n_sections;
    Section& s = P.sp.sec[P.sp.n_sections++];
    s.elem_start = elem; s.lane_elems = lane_elems; s.n_lanes = n_lanes; s.lut_off = lut_off; s.kind = kind_; s.src = src;
    s.magic = (uint32_t)((0x100000000ull + lane_elems - 1) / lane_elems);  // lane = mulhi(rel, magic); rel * lane_elems < 2^32 here
    s.rec_stride = 0; s.rec_mul = 0; s.pad = 0; s.base = nullptr;
    elem += lane_elems * n_lanes;
  };
  uint32_t mark;

  // H.1 target_header / next_header : Bytes32
  mark = (uint32_t)L.v.size();
  L.bytes(PF_OFF_HEADER, 32);
  add_section((uint32_t)L.v.size() - mark, 1, mark, SEC_LUT, SRC_PF, 1);

  // H.2 validators[N] : ValidatorVariable (variables.rs:69-79) = pubkey, signature{r, s}, message[124],
  //     message_byte_length, voting_power, validator_byte_length, signed
  mark = (uint32_t)L.v.size();
  P.pub512.h2_pk = (uint32_t)L.v.size() - mark;
  L.bytes(VR_OFF_PK, 32);
  P.pub512.h2_r = (uint32_t)L.v.size() - mark;
  L.bytes(VR_OFF_SIG, 32);
  L.u256(VR_OFF_SIG + 32);
  P.pub512.h2_msg = (uint32_t)L.v.size() - mark;
  L.bytes(VR_OFF_MSG, 124);
  P.pub512.h2_mlen = (uint32_t)L.v.size() - mark;
  L.u16(VR_OFF_MLEN);
  L.u64(VR_OFF_POWER);
  P.pub.h2_vlen = (uint32_t)L.v.size() - mark;
  L.u8(VR_OFF_VLEN);
  P.pub512.h2_signed = (uint32_t)L.v.size() - mark;
  L.flag0(VR_OFF_FLAGS);
  P.pub.h2 = elem; P.pub.h2_lane = (uint32_t)L.v.size() - mark;
  P.pub512.h2 = P.pub.h2; P.pub512.h2_lane = P.pub.h2_lane;
  add_section((uint32_t)L.v.size() - mark, n, mark, SEC_LUT, SRC_TARGET, 0);

  // H.3 nb_validators, round, ChainIdProofVariable, HeightProofVariable, validators-hash proof, then
  //     skip: trusted nb + trusted validators-hash proof ; step: last_block_id proof + prev next_validators_hash proof
  mark = (uint32_t)L.v.size();
  auto here = [&]() { return (uint32_t)L.v.size(); };
  AirShaPublicGeom& U = P.pub;
  L.u32(PF_OFF_NB_A);
  L.u64(PF_OFF_ROUND);
  U.aunts[0] = here();
  L.bytes(PF_OFF_AUNTS + 128 * 0, 128);   // chain_id_proof.proof
  U.cid_len = here();
  L.u32(PF_OFF_CIDLEN);                   // enc_chain_id_byte_length
  U.cid = here();
  L.bytes(PF_OFF_CID52, 52);              // chain_id
  U.aunts[1] = here();
  L.bytes(PF_OFF_AUNTS + 128 * 1, 128);   // height_proof.proof
  U.h_len = here();
  L.u32(PF_OFF_HLEN);                     // enc_height_byte_length
  L.u64(PF_OFF_HEIGHT);                   // height
  emit_inclusion_proof(L, 2, PF_OFF_LEAFV, 34, &U.aunts[2], &U.leaf[2]);
  U.leaf_bytes[0] = 52; U.leaf_bytes[1] = 11; U.leaf_bytes[2] = 34; U.leaf_bytes[3] = skip ? 34 : 72; U.leaf_bytes[4] = 34;
  if (skip) {
    L.u32(PF_OFF_NB_B);
    emit_inclusion_proof(L, 3, PF_OFF_LEAFX, 34, &U.aunts[3], &U.leaf[3]);
  } else {
    emit_inclusion_proof(L, 3, PF_OFF_LEAFX, 72, &U.aunts[3], &U.leaf[3]);
    emit_inclusion_proof(L, 4, PF_OFF_LEAFY, 34, &U.aunts[4], &U.leaf[4]);
  }
  // (table positions -> elements inside H.3)
  for (uint32_t* at : {&U.cid_len, &U.cid, &U.h_len}) *at -= mark;
  for (int q = 0; q < 5; q++) { U.aunts[q] = q < (skip ? 4 : 5) ? U.aunts[q] - mark : 0; U.leaf[q] = (q >= 2 && q < (skip ? 4 : 5)) ? U.leaf[q] - mark : 0; }
  U.h3 = elem;
  add_section((uint32_t)L.v.size() - mark, 1, mark, SEC_LUT, SRC_PF, 1);

  // H.4 skip: trusted_header_validator_hash_fields[N] : ValidatorHashFieldVariable (variables.rs:82-88)
  if (skip) {
    mark = (uint32_t)L.v.size();
    L.bytes(HR_OFF_PK, 32);
    L.u64(HR_OFF_POWER);
    P.pub.h4_vlen = (uint32_t)L.v.size() - mark;
    L.u8(HR_OFF_VLEN);
    P.pub.h4 = elem; P.pub.h4_lane = (uint32_t)L.v.size() - mark;
    add_section((uint32_t)L.v.size() - mark, n, mark, SEC_LUT, SRC_TRUSTED, 0);
  }
  P.hint_elems = elem;

  // D.1a per target lane: the byte fields (marshalled validator, leaf hash: k_proof; SHA-512 digest: phase 1).  Their own section so that
  // they are written while the table walk runs; only D.1b waits for k_ed_fin.
  mark = (uint32_t)L.v.size();
  L.bytes(TL_OFF_LT + LN_OFF_MARSHAL, 46);
  P.pub.lane_leaf = (uint32_t)L.v.size() - mark;  // (the marshalled validator first, then the leaf hash: D.2a the same)
  L.bytes(TL_OFF_LT + LN_OFF_LEAF, 32);
  P.pub512.d1a_digest = (uint32_t)L.v.size() - mark;
  L.bytes(TL_OFF_ED + ED_OFF_DIGEST, 64);
  P.pub.d1a = elem; P.pub.d1a_lane = (uint32_t)L.v.size() - mark;
  P.pub512.d1a = P.pub.d1a; P.pub512.d1a_lane = P.pub.d1a_lane;
  add_section((uint32_t)L.v.size() - mark, n, mark, SEC_LUT, SRC_TL, 4);
  // D.1b per target lane: h, the ten coordinates, the EdDSA verdict, the six flags, the two prefix sums
  mark = (uint32_t)L.v.size();
  L.u256(TL_OFF_ED + ED_OFF_H);
  for (int p = 0; p < 10; p++) L.u256(TL_OFF_ED + ED_OFF_PTS + 32 * p);
  L.u32(TL_OFF_ED + ED_OFF_OK);
  for (int f = 0; f < 6; f++) L.u8(TL_OFF_LT + LN_OFF_FLAGS + f);
  L.u64(TL_OFF_LT + LN_OFF_TOT);
  L.u64(TL_OFF_LT + LN_OFF_ACC);
  P.d1b_start = elem;
  if ((uint32_t)L.v.size() - mark != D1B_LANE_ELEMS) P.d1b_start = 0xffffffffu;  // (caught by tmx_ctx_create: layout.h and this list must agree)
  add_section((uint32_t)L.v.size() - mark, n, mark, SEC_LUT, SRC_TL, 2);

  // D.2a / D.2b per trusted lane: byte fields (marshalled validator, leaf hash: ready with the leaves), word fields (flags, prefix sums: k_proof)
  if (skip) {
    mark = (uint32_t)L.v.size();
    L.bytes(LN_OFF_MARSHAL, 46);
    L.bytes(LN_OFF_LEAF, 32);
    P.pub.d2a = elem; P.pub.d2a_lane = (uint32_t)L.v.size() - mark;
    add_section((uint32_t)L.v.size() - mark, n, mark, SEC_LUT, SRC_LR, 5);
    mark = (uint32_t)L.v.size();
    L.u8(LN_OFF_FLAGS);
    L.u8(LN_OFF_FLAGS + 1);
    L.u64(LN_OFF_TOT);
    L.u64(LN_OFF_ACC);
    add_section((uint32_t)L.v.size() - mark, n, mark, SEC_LUT, SRC_LR, 1);
  }
  // D.3 / D.4 tree nodes
  if (tn) {
    P.pub.d3 = elem;
    add_section(tn * 256, 1, 0, SEC_LINEAR_T, SRC_PF, 1);
    if (skip) { P.pub.d4 = elem; add_section(tn * 256, 1, 0, SEC_LINEAR_R, SRC_PF, 1); }
  }
  // D.5 header proofs, tallies, checks, verdict
  mark = (uint32_t)L.v.size();
  P.pub.d5 = elem;
  emit_proof_d(L, 0);
  P.pub.d5_hleaf = (uint32_t)L.v.size() - mark;
  L.bytes(PF_OFF_HLEAF, 11);
  for (int q = 1; q < (skip ? 4 : 5); q++) {
    P.pub.d5_proof[q] = (uint32_t)L.v.size() - mark;
    emit_proof_d(L, q);
  }
  for (int k = 0; k < 4; k++) L.u64(PF_OFF_TALLY_T + 8 * k);
  P.tail_dep_elem = elem + ((uint32_t)L.v.size() - mark);
  L.u32(PF_OFF_VERDICTS);
  if (skip) {
    for (int k = 0; k < 4; k++) L.u64(PF_OFF_TALLY_R + 8 * k);
    L.u32(PF_OFF_VERDICTS + 4);
    L.u32(PF_OFF_VERDICTS + 8);
    L.u32(PF_OFF_VERDICTS + 12);
  }
  const int n_checks = skip ? 13 : 15;
  for (int k = 0; k < n_checks; k++) L.u32(PF_OFF_CHECKS + 4 * k);
  L.u32(PF_OFF_ALLOK);
  add_section((uint32_t)L.v.size() - mark, 1, mark, SEC_LUT, SRC_PF, 3);
  P.mask_tail |= 1u << 31;  // boundary waves are written last, when every source is ready
  for (uint32_t k = 0; k < P.sp.n_sections; k++) (P.sp.sec[k].elem_start < P.hint_elems ? P.mask_hint : P.mask_derived) |= 1u << k;

  P.sp.elem_count = elem;
  P.sp.elem_stride = (elem + 15) & ~15u;  // rows start on a 128-byte line
  P.sp.n = n;
  P.sp.tree_nodes = tn;
  P.lut = std::move(L.v);
  const uint32_t span = SER_SPAN_ELEMS;  // elements per wave (layout.h TMX_SER_SPAN): 128 and 512 measured slower on MI355X (round 1; round 6: docs/experiments.md)
  P.sp.span = span;
  for (uint32_t w = 0; w * span < P.sp.elem_stride; w++) {
    const uint32_t first = w * span, last = first + span - 1;
    uint8_t sec = 0xff;
    if (last < P.sp.elem_count)
      for (uint32_t s = 0; s < P.sp.n_sections; s++) {
        const uint32_t lo = P.sp.sec[s].elem_start, hi = lo + P.sp.sec[s].lane_elems * P.sp.sec[s].n_lanes;
        if (first >= lo && last < hi) sec = (uint8_t)s;
      }
    if (sec == 0xff) P.seam_waves.push_back(w);
    P.wave_sec.push_back(sec);
  }
  return P;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ context
constexpr int EV_RING_DECL = 128;
constexpr uint64_t THROUGHPUT_LANES = 81920;  // proofs x validators from which run_batch schedules for throughput (see beside_chain_wgs)
// Schedule knobs, read ONCE at context creation (getenv is not safe against a concurrent setenv, and the enqueue path is
// latency-critical).  Each selects a schedule, never a value (tests/test_gpu_parity.py::test_schedule_knobs_give_the_same_bits); the A/B
// harness that measured the alternatives no longer in the product lives in tools/ (DESIGN.md appendix "measured and dropped").
struct Knobs {
  uint32_t dedup_mode = 1;   // TMX_DEDUP=0|1|2: never use per-key tables / automatic / whenever they fit
  bool key_cache = true;     // TMX_KEY_CACHE=0: the per-key tables do not survive a call (every call cold)
  uint32_t key_cache_keys = 0;  // TMX_KEY_CACHE_KEYS: capacity of the cache in keys (0: by max_batch * n_max)
  bool ser_split = true;     // TMX_SER_SPLIT=0: one k_serialize launch at the end of the step (times the kernel on its own)
  int leaves = -1;           // TMX_LEAVES=0|1: leaf hashes as a launch of their own in front of k_proof (default: from 131072 lanes)
  int walk_parts = -1;       // TMX_WALK_PARTS=0|1: the table walk follows the table build part by part (default: from 65536 lanes)
  bool ext_events = true;    // TMX_EXT_EVENTS=0: record packets instead of completion signals on the chain kernels
  int warm_schedule = -1;    // TMX_SCHEDULE=warm|cold: the EdDSA schedule for resident / new keys (default: by what the last launch saw)
  int phase1_max = -1;       // TMX_PHASE1_MAX=<lanes>: up to that many lanes the warm schedule runs s*B as a role of the hash launch (default 16384: 128 proofs at N = 128)
  bool join1 = true;         // TMX_JOIN1=0: the small form's tail behind two wait packets (k_proof, the new-key lanes' finish) instead of one joined on side2
  long tiny_max = -1;        // TMX_TINY_MAX=<lanes>: the two-launch small path up to that many lanes (default 1536, at most TINY_MAX_LANES = 2048)
  int one_launch_max = -1;   // TMX_SER_ONE_LAUNCH=<proofs>: up to that many proofs the uncapped serializer calls are one launch each (default 8)
  bool proof_roles = true;   // TMX_PROOF_ROLES=0: k_proof as one workgroup per proof (the round-3 kernel) instead of four role workgroups
  int tail_wide = 1;         // TMX_TAIL_WIDE=0: k_verdict -> D.5 -> the seam spans as three launches / one workgroup per proof (rounds 2 - 5) instead of ONE launch of independent workgroups (k_verdict_tail_wide)
  int p1_early = -1;         // TMX_P1_EARLY=0|1|2: D.1a behind k_proof's sections on the side stream (1: on a capped grid, 2: full grid) instead of behind k_ed_fin (default: capped, from 131072 lanes)
  int hash_first = -1;       // TMX_HASH_FIRST=0|1: warm schedule with the hash role in front of the dedup (which moves to side2); default: see run_eddsa
  bool walk_split = true;    // TMX_WALK_SPLIT=0: the warm schedule's table walk as ONE launch behind the table build (the round-4 form) instead of resident lanes at once + new-key lanes behind the build
  bool compact = true;       // TMX_COMPACT=0: every lane through the EdDSA kernels (round 4), also the ones that did not sign
  bool set_cache = true;     // TMX_SET_CACHE=0: k_proof computes the leaves and the tree of every validator set of every proof (round 4)
  bool epi_late = true;      // TMX_EPI_LATE=0: the cache epilogue of a split warm batch in front of the input sections on side3 (the first round-5 form)
  bool ser_lanes = true;     // TMX_SER_LANES=0: no scalar-lane path for the spans that lie inside one lane of a per-lane section (serialize_span)
  int fused_base = -1, fused_walk = -1;  // TMX_FUSED_ROWS=<b>[,<w>]: input-only row spans a wave of s*B / of the resident walk takes per table addition
                                         // (fused rows, layout.h FusedRows); 0,0 = off: the sections as capped launches of their own (round 5); default: see run_batch
  long inputs_first_min = -1; // TMX_INPUTS_FIRST=<lanes>: from that many lanes on the split warm schedule enqueues the input sections IN FRONT of the new-key pipeline on the low-priority stream (0: never)
  bool ser_rows = true;      // TMX_SER_ROWS=0: the capped row-writer launches grid-stride over (proof, block) (k_serialize_few, round 5) instead of proof-major (k_serialize_rows)
  int writer_prio = -1;      // TMX_WRITER_PRIO=<0..3>: s_setprio of the row-writer waves (default: by size, run_batch)
  int tail_aside_min = -1;   // TMX_TAIL_ASIDE_MIN=<lanes>: from how many lanes on the verdict + its sections leave the caller's stream (default 28672)
  int few_wgs = 0;           // TMX_FEW_WGS=<n>: workgroups of the serializer launches beside the chain (A/B; 0: by size, run_batch)
  int tiny = -1;             // TMX_TINY=0|1: never / always (also under a forced TMX_SCHEDULE) take the two-launch small path for <= TINY_MAX_LANES lanes
};
static Knobs read_knobs() {
  Knobs k;
  const char* v;
  if ((v = std::getenv("TMX_DEDUP")) && v[0] >= '0' && v[0] <= '2') k.dedup_mode = (uint32_t)(v[0] - '0');
  k.key_cache = !((v = std::getenv("TMX_KEY_CACHE")) && v[0] == '0');
  if ((v = std::getenv("TMX_KEY_CACHE_KEYS")) && std::atoll(v) > 0) k.key_cache_keys = (uint32_t)std::min<long long>(std::atoll(v), 1 << 20);
  k.ser_split = !((v = std::getenv("TMX_SER_SPLIT")) && v[0] == '0');
  k.leaves = (v = std::getenv("TMX_LEAVES")) ? (v[0] != '0' ? 1 : 0) : -1;
  k.walk_parts = (v = std::getenv("TMX_WALK_PARTS")) ? (v[0] == '1' ? 1 : 0) : -1;
  k.ext_events = !((v = std::getenv("TMX_EXT_EVENTS")) && v[0] == '0');
  k.warm_schedule = (v = std::getenv("TMX_SCHEDULE")) ? (v[0] == 'w' ? 1 : 0) : -1;
  k.tiny = (v = std::getenv("TMX_TINY")) ? (v[0] != '0' ? 1 : 0) : -1;
  k.walk_split = !((v = std::getenv("TMX_WALK_SPLIT")) && v[0] == '0');
  k.proof_roles = !((v = std::getenv("TMX_PROOF_ROLES")) && v[0] == '0');
  if ((v = std::getenv("TMX_SER_ONE_LAUNCH"))) k.one_launch_max = std::atoi(v);
  if ((v = std::getenv("TMX_TINY_MAX"))) k.tiny_max = std::atol(v);
  if ((v = std::getenv("TMX_JOIN1"))) k.join1 = v[0] != '0';
  if ((v = std::getenv("TMX_PHASE1_MAX"))) k.phase1_max = std::atoi(v);
  k.hash_first = (v = std::getenv("TMX_HASH_FIRST")) ? (v[0] != '0' ? 1 : 0) : -1;
  if ((v = std::getenv("TMX_TAIL_WIDE"))) k.tail_wide = v[0] != '0' ? 1 : 0;
  k.p1_early = (v = std::getenv("TMX_P1_EARLY")) && v[0] >= '0' && v[0] <= '2' ? v[0] - '0' : -1;
  k.compact = !((v = std::getenv("TMX_COMPACT")) && v[0] == '0');
  k.set_cache = !((v = std::getenv("TMX_SET_CACHE")) && v[0] == '0');
  k.epi_late = !((v = std::getenv("TMX_EPI_LATE")) && v[0] == '0');
  if ((v = std::getenv("TMX_FEW_WGS"))) k.few_wgs = std::atoi(v);
  if ((v = std::getenv("TMX_TAIL_ASIDE_MIN"))) k.tail_aside_min = std::atoi(v);
  if ((v = std::getenv("TMX_WRITER_PRIO"))) k.writer_prio = std::atoi(v);
  k.ser_rows = !((v = std::getenv("TMX_SER_ROWS")) && v[0] == '0');
  if ((v = std::getenv("TMX_INPUTS_FIRST"))) k.inputs_first_min = std::atol(v);
  if ((v = std::getenv("TMX_FUSED_ROWS"))) {
    k.fused_base = std::atoi(v);
    const char* comma = std::strpbrk(v, ",:");
    k.fused_walk = comma ? std::atoi(comma + 1) : 0;
    if (k.fused_base < 0) k.fused_base = 0;
    if (k.fused_walk < 0) k.fused_walk = 0;
  }
  if ((v = std::getenv("TMX_SER_LANES"))) k.ser_lanes = std::atoi(v) != 0;
  return k;
}

struct tmx_ctx {
  tmx_config cfg;
  Knobs knobs;
  std::string err;
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;  // k_proof runs here, concurrently with the EdDSA kernels of the caller's stream
  hipEvent_t ev_join = nullptr;
  hipEvent_t ev_side[EV_RING_DECL][4] = {};
  hipEvent_t ev_hash = nullptr;  // phase 1 is done: the SHA-512 digest and h of every lane are in the lane records
  bool ev_hash_recorded = false;
  hipEvent_t ev_leaves = nullptr;
  hipEvent_t ev_tail = nullptr, ev_fork2 = nullptr, ev_hash_clean = nullptr, ev_keys = nullptr;
  bool fin_done_attached = false;
  void* fin_done = nullptr;  // set by run_batch around the EdDSA producer: the event k_ed_fin signals
  RowOut row = {};           // set by run_batch around the EdDSA producer: where the finish writes D.1b into the rows (or null)
  FusedRows fused = {};      // set by run_batch around the EdDSA producer: the input-only row spans its throughput kernels carry (ctr null: none)
  SerializeProgram fused_prog = {};
  uint32_t* d_span_ctr = nullptr;  // two claim counters (a fused launch uses one, its sweeper zeroes the other for the next)
  uint32_t span_parity = 0;
  bool span_ctr_dirty = false;     // a fused launch failed half-way: both counters are zeroed before the next one
  hipEvent_t ev_direct = nullptr;  // the table-free lanes of a launch are done (side2)
  volatile uint32_t* h_hint = nullptr;  // page-locked, written by k_kc_epilogue: [0] launches committed, [1] new keys of the last one
  hipEvent_t ev_part[4] = {};
  bool have_streams = false;
  // ring of HIP-event sets: one set (TMX_N_KERNELS + 1 events) per enqueued batch, so that kernel durations can be
  // averaged over a whole timed region afterwards without synchronising inside it
  static constexpr int EV_RING = EV_RING_DECL;
  hipEvent_t ev[EV_RING][4] = {};
  uint64_t n_calls = 0;
  hipStream_t last_stream = nullptr;  // stream and end event of the previous batch (cross-stream callers are ordered behind it)
  bool last_stream_valid = false;
  hipEvent_t ev_done = nullptr;
  hipEvent_t ev_value = nullptr;  // end of the last typed-value batch (its k_pack_value launch)
  hipEvent_t ev_base = nullptr;   // s*B of the batch being enqueued is done (the split warm schedule: its own launch on side2)
  // the EdDSA schedule of the batch being enqueued, decided ONCE (the hint it looks at lives in host memory the device writes)
  struct EdPlan { bool valid, tiny, warm, hash_first, sb_with_hash, split; } plan = {};
  bool epilogue_pending = false;  // (TMX_EPI_LATE) the epilogue of the batch being enqueued goes behind the input sections on side3
  EdQuad pending_q;
  int32_t last_kind = -1;       // kind and size of the last Level-1 batch (tmx_trace_rows_device reads its lane records)
  uint32_t last_n_proofs = 0;
  Program prog[2];
  void* d_lut[2] = {nullptr, nullptr};
  void* d_wave_sec[2] = {nullptr, nullptr};
  void* d_seams[2] = {nullptr, nullptr};
  void* d_table = nullptr;
  void *d_qtable = nullptr, *d_pre = nullptr, *d_mulout = nullptr;
  // EdDSA stage: the launch's own dedup structures, the key records (cache slots, then one per lane for keys without a slot), the
  // anchor scratch of the tables being built, and the persistent key cache
  // the lanes that did not sign: one precomputed record for all of them (dummy_record), the dense list of the others per launch
  void *d_live = nullptr, *d_dummy_ed = nullptr, *d_dummy_in = nullptr;
  bool dummy_ready = false;
  SetCache setc = {};   // the validator-set cache (layout.h); table == nullptr: off (TMX_SET_CACHE=0)
  uint32_t setc_epoch = 1;  // LRU stamp of the next k_proof launch (never 0: a slot's 0 means free)
  void *d_hash = nullptr, *d_cnt = nullptr, *d_owner_of = nullptr, *d_slot_of_owner = nullptr, *d_slot_of_uid = nullptr, *d_owners = nullptr,
       *d_keyrec = nullptr, *d_anchors = nullptr, *d_keytab = nullptr;
  KeyCache kc = {};
  uint32_t hash_mask = 0;
  hipStream_t side2 = nullptr;  // new-key pipeline, concurrent with phase 1
  hipStream_t side3 = nullptr;  // early serialization of the input-only sections
  hipEvent_t ev_join3 = nullptr;
  uint32_t parity = 0;  // which of the two counter sets this launch uses
  void* d_commit = nullptr;    // scratch of tmx_trace_commit_device: columns | extended columns | tree levels (grows on demand)
  size_t commit_bytes = 0;
  hipEvent_t ev_commit[4] = {};
  // the last tmx_trace_commit_device (what tmx_trace_commit_open_device opens): its shape and where its extended columns and levels sit in
  // d_commit.  valid: that call finished enqueueing (any failure of a later commit call, or an empty shard, clears it)
  // (and the log_blowup and NTT domain it was extended with: what tmx_trace_commit_fri_device proves under)
  struct CommitRec { bool valid; uint32_t log_m, n_cols, cap_height; size_t lde_off, lev_off; uint32_t log_blowup; uint64_t root, shift; } last_commit = {};
  // scratch of the FRI provers (transcript state, challenges, degree flag, alpha powers, leaf indices, layers, layer trees; grows on demand)
  // and the events around the stages of the last prove.  fri_valid: a prove finished enqueueing (tmx_fri_last_degree_ok / _ms read it)
  void* d_fri = nullptr;
  size_t fri_bytes = 0, fri_flag_off = 0;
  hipEvent_t ev_fri[5] = {};
  bool fri_valid = false;
  bool fri_deep = false;  // the last prove was a DEEP prove (its zeta sits in d_fri: tmx_deep_last_zeta)
  uint32_t fri_pow_bits = 0;  // non-zero: the last prove was a grinding prove (the search's two words sit in d_fri: tmx_pow_last)
  // the commit set (tmx_trace_commit_set_device): several sections committed side by side in a scratch of its own -- per oracle its pre-LDE
  // columns | extended columns | tree levels -- in the oracle order of the batch proof.  Independent of last_commit and d_commit.
  // A streamed member (tmx_trace_commit_set_streamed_device) keeps no extended columns (lde_off unused); behind the last member sit the two
  // buffers all streamed members share: the sponge states [12][2^log_m] and one chunk of extended columns [chunk_cols][2^log_m], both sized
  // by the tallest streamed member.
  void* d_set = nullptr;
  size_t set_bytes = 0;
  struct SetRec {
    bool valid; uint32_t n_oracles, log_blowup, cap_height; uint64_t root, shift;
    // buf: the scratch the offsets refer to if it is not d_set (ext: d_set_air): a member added by tmx_trace_commit_set_air_sha256_device
    // chunk_cols != 0: a streamed member with a chunk buffer of its own at chunk_off of buf (a streamed helper of constraint sets 3 - 5, 7 - 9)
    struct Oracle {
      uint32_t section, log_m, n_cols; size_t cols_off, lde_off, lev_off; bool streamed, ext; const void* buf = nullptr;
      uint32_t chunk_cols = 0; size_t chunk_off = 0;
    } o[8];
    uint32_t chunk_cols; size_t state_off, chunk_off;
  } set = {};
  // the constraint quotient (tmx_air_*): d_air = prover transcript state 32 | challenges 72 (gamma at FRI_GAMMA_AT) | verifier state 32 |
  // verifier challenges 72 | the tables of one quotient launch (air.h); ev_air behind the last quotient (tmx_air_last_gamma waits for it).
  // d_set_air: the quotient member of the commit set (Oracle.ext: lde_off and lev_off are offsets into it, not into d_set; no pre-LDE columns).
  void* d_air = nullptr;
  size_t air_bytes = 0;
  hipEvent_t ev_air = nullptr;
  bool air_valid = false;
  void* d_set_air = nullptr;
  size_t set_air_bytes = 0;
  // constraint sets 3, 4 and 5 (tmx_trace_commit_set_air_sha256_device, _sched_device, _init_device), [set (ShaSet.scratch)][section (SHA256,
  // TREE, HEADER)]: one scratch that holds the set's helper member of that section -- pre-LDE columns | extended columns | tree levels --
  // and its quotient member -- extended columns | tree levels (Oracle.buf names it).  With a streamed helper
  // (tmx_trace_commit_set_air_sha256_streamed_device, _sha512_streamed_device) the helper's extended columns are absent and behind the quotient's levels sit the
  // sponge states [12][M] and the helper's chunk buffer [chunk_proofs helper_cols][M]
  void* d_set_sha[8][3] = {};  // (rows 0 .. 2: constraint sets 3 .. 5; row 3: set 6; rows 4 .. 7: sets 7, 8, 9 and 10, whose one section uses slot 0)
  size_t set_sha_bytes[8][3] = {};
  // constraint set 2 (tmx_air_ladder_boundary_*): the set-2 tables | the size-K twiddles | V (prover) | V (verifier) | the coefficients of
  // Pub_gamma | the public tree's levels (prover) | (verifier) | Pub_gamma on the coset (2 << log_m words: the part that grows)
  void* d_air2 = nullptr;
  size_t air2_bytes = 0;
  void* d_air6 = nullptr;  // constraint set 6's caller-level scratch (AIR6_OFF_*)
  size_t air6_bytes = 0;
  // constraint set 7 (tmx_air_sha512_*): the barycentric kernel's rows (prover-free: the verifier's) | SEL, KLO, KHI before the LDE (3 N)
  // | the three extended planes (3 M: the part that grows)
  void* d_air7 = nullptr;
  size_t air7_bytes = 0;
  // constraint set 8 (tmx_air_sha512_sched_*), a scratch of its own so that set 7's stays as it is: the barycentric kernel's rows | SCH
  // before the LDE (N) | the extended plane (M: the part that grows)
  void* d_air8 = nullptr;
  size_t air8_bytes = 0;
  // constraint set 9 (tmx_air_sha512_init_*), again a scratch of its own: the barycentric kernel's rows | STA, CHN before the LDE (2 N) |
  // the two extended planes (2 M: the part that grows)
  void* d_air9 = nullptr;
  size_t air9_bytes = 0;
  void* d_air10 = nullptr;  // set 10's own: its planes as sets 7 - 9 keep theirs, and the public side (link512_* below)
  size_t air10_bytes = 0;
  // the DEEP verifier's scratch: the openings tree of the proof it checks (grows on demand)
  void* d_deepv = nullptr;
  size_t deepv_bytes = 0;
  // staging of the host query indices of the opening / verifying calls: a ring of page-locked + device buffers, each slot reused only once
  // the event behind the launch that read it has completed
  struct IdxSlot { uint64_t* h = nullptr; uint64_t* d = nullptr; uint64_t cap = 0; hipEvent_t ev = nullptr; bool used = false; };
  static constexpr int IDX_RING = 4;
  IdxSlot idx_ring[IDX_RING];
  uint32_t idx_next = 0;
  void* comm = nullptr;        // ncclComm_t of this context's device (tmx_comm_create), or null
  bool comm_aborted = false;   // a local failure (or a peer's) in front of a collective aborted the communicator: tmx_comm_create again
  uint32_t comm_rank = 0, comm_world = 1;
  void* d_tiny = nullptr;      // counters of the small-launch path (kernels.h: tiny_counter_words), zero between launches
  void* d_shadow = nullptr;    // key bytes + flags of the lanes of a small launch (TINY_MAX_LANES records): what its key pipeline reads
  bool slot_tiny[EV_RING_DECL] = {};  // which event sets of the ring belong to small launches (their four events mark other points)
  uint64_t last_lanes = 0;
  int32_t last_proof_path = TMX_PROOF_PATH_NONE;  // which launch computed the proof-level values of the last batch (tmx_last_proof_path)
  // scratch sized for cfg.max_batch proofs
  void *d_ed = nullptr, *d_tl = nullptr, *d_lr = nullptr, *d_pf = nullptr, *d_nodes_t = nullptr, *d_nodes_r = nullptr, *d_reports = nullptr;
  // staging for the host-buffer entry points
  void *d_in_proofs = nullptr, *d_in_targets = nullptr, *d_in_trusteds = nullptr, *d_out = nullptr;
  uint64_t d_out_elems = 0;
  hipEvent_t ev_trace[17] = {};  // ladder segments done (up to 16) + [16] the side stream's pass 2 done
  hipEvent_t ev_trace_rest[2] = {};  // the other sections beside the ladders: fork, join
  void* d_trace_tmp = nullptr;  // projective ladder points between the two passes of the Level-2 ladder kernels (allocated on first use)
  void* d_pack = nullptr;  // dense / narrowed rows for tmx_witness_batch_opts (allocated on first use)
  void* d_val_lut[2] = {nullptr, nullptr};  // fixed-part gather tables of the typed value (value.h), per kind
  void* d_value = nullptr;  // device staging of tmx_inputs_value_batch when `out` is not page-locked (allocated on first use)
  uint64_t d_value_bytes = 0;
  uint64_t d_pack_bytes = 0;
  uint32_t sections = 3;  // TMX_SEC_* of the batch being enqueued
  // Goldilocks NTT: twiddle tables per transform size (built on first use), scratch for the four-step split / LDE
  void* d_ntt_w[TMX_NTT_MAX_LOG + 1] = {};
  void* d_ntt_m[2][TMX_NTT_MAX_LOG + 1] = {};  // four-step twiddle matrices omega_N^(+- n2 k1) (forward, inverse), built on first use
  void* d_lde_s[TMX_NTT_MAX_LOG + 1] = {};  // coset-LDE scale vectors S[i] = shift^i / N per column length (built on first use, dropped with the domain)
  void* d_ntt_tmp = nullptr;
  size_t ntt_tmp_bytes = 0;
  // NTT domain: primitive 2^32-th root of unity and coset shift.  Default: the constants recalled from plonky2's GoldilocksField
  // (POWER_OF_TWO_GENERATOR, MULTIPLICATIVE_GROUP_GENERATOR; self-consistent: the first is the second to the (p-1)/2^32).
  uint64_t ntt_root = 7277203076849721926ull, ntt_shift = 14293326489335486720ull;
  // Poseidon: round constants | MDS circulant | MDS diagonal, host copy and device copy (uploaded on first use / on change)
  std::vector<uint64_t> pos_consts;
  void* d_pos_consts = nullptr;
  bool pos_dirty = true;
  int pos_mode = POS_MODE_SMALL;  // poseidon.h POS_MODE_*: chosen from the MDS entries when the tables are uploaded
  bool pos_rc_injected = false;  // round constants came from tmx_poseidon_set_constants (the defaults are NOT plonky2's table)
};

static int32_t fail(tmx_ctx* c, int32_t st, const std::string& msg) {
  if (c) c->err = msg;
  return st;
}
#define HIPCK(c, call)                                                                                   \
  do {                                                                                                    \
    hipError_t e_ = (call);                                                                               \
    if (e_ != hipSuccess) return fail(c, TMX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

static ProofParams proof_params(const tmx_ctx* c, int32_t kind, bool leaves_done) {
  ProofParams P;
  std::memset(&P, 0, sizeof P);
  P.leaves_done = leaves_done ? 1u : 0u;
  P.kind = (uint32_t)kind; P.n = c->cfg.n_max; P.tree_nodes = tree_nodes(c->cfg.n_max); P.chain_id_len = c->cfg.chain_id_len;
  P.skip_max = c->cfg.skip_max;
  P.setc_epoch = c->setc_epoch;
  std::memcpy(P.chain_id, c->cfg.chain_id, sizeof P.chain_id);
  return P;
}

#ifndef TMX_FUSED_BASE_DEFAULT
#define TMX_FUSED_BASE_DEFAULT 0  // (spans per table addition of s*B / of the resident walk; set by measurement: docs/experiments.md round 6)
#define TMX_FUSED_WALK_DEFAULT 0
#endif
#ifndef TMX_HASH_FIRST_MAX
#define TMX_HASH_FIRST_MAX 16384u  // measured: 64 / 128 proofs at N = 128 -3 %, 256 +2 %, 1024 +6 % (the dedup beside the hash role on a full chip)
#endif
// which EdDSA schedule a launch of n_lanes takes (run_eddsa has the graphs).  in_batch: the launch is the EdDSA stage of run_batch, which
// can put s*B first on its low-priority stream.
static tmx_ctx::EdPlan ed_plan(const tmx_ctx* c, uint32_t n_lanes, bool in_batch) {
  const Knobs& K = c->knobs;
  tmx_ctx::EdPlan P = {};
  P.valid = true;
  P.tiny = n_lanes != 0 && n_lanes <= 512;
  P.warm = K.warm_schedule >= 0 ? K.warm_schedule != 0
                                : (c->kc.persist && K.dedup_mode != 0 && c->h_hint && c->h_hint[0] != 0 && c->h_hint[1] == 0);
  P.hash_first = P.warm && !P.tiny && n_lanes != 0 && (K.hash_first >= 0 ? K.hash_first != 0 : n_lanes <= TMX_HASH_FIRST_MAX);
  P.sb_with_hash = P.tiny || (K.phase1_max >= 0 ? n_lanes <= (uint32_t)K.phase1_max : n_lanes <= 16384);
  // the warm schedule split by residency (run_eddsa_split): only as the EdDSA stage of a batch (run_batch reorders its low-priority stream for it)
  P.split = in_batch && K.walk_split && P.warm && !P.tiny && n_lanes != 0 && K.dedup_mode != 0 && c->kc.cap != 0;
  return P;
}

// Launch sequence of one batch.  Caller's stream s: [ev0] EdDSA kernels [ev1] k_serialize of the EdDSA-dependent section [ev3]
//                               side:   (after ev0) [side0] k_proof [side1], then the sections that only need it -> ev_join
//                               side3:  (after ev0) the sections that only expand the input records -> ev_join3
//                               side2:  the new-key pipeline of the EdDSA stage; the tail: k_verdict + the sections that carry it -> ev_tail
// k_proof does not depend on the EdDSA results, so it overlaps with them; `ed_producer` enqueues whatever fills the ED part of
// c->d_tl on s (the EdDSA kernels, or a strided copy of caller-provided lane records).
template <typename EdProducer>
static int32_t run_batch(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets, const void* d_trusteds,
                         void* d_out_elems, void* d_reports, hipStream_t s, bool eddsa_writes_rows, EdProducer ed_producer) {
  const uint32_t n = c->cfg.n_max;
  const Knobs& K = c->knobs;
  uint8_t* tl = reinterpret_cast<uint8_t*>(c->d_tl);
  void* reports = d_reports ? d_reports : c->d_reports;
  const uint64_t slot = c->n_calls % tmx_ctx::EV_RING;
  hipEvent_t* ev = c->ev[slot];
  hipEvent_t* evs = c->ev_side[slot];
  SerializeSources src;
  std::memset(&src, 0, sizeof src);
  src.base[SRC_TARGET] = (const uint8_t*)d_targets; src.base[SRC_TRUSTED] = (const uint8_t*)d_trusteds;
  src.base[SRC_TL] = tl; src.base[SRC_LR] = (const uint8_t*)c->d_lr; src.base[SRC_PF] = (const uint8_t*)c->d_pf;
  src.nodes_t = (const uint8_t*)c->d_nodes_t; src.nodes_r = (const uint8_t*)c->d_nodes_r;
  Program& prog = c->prog[kind];
  // Throughput regime (round 6, profiles/r06_throughput_regime_ab.txt): from 512 proofs x 128 on a step is a VALU-bound chain plus an HBM-bound tail
  // that overlap badly -- whatever shortens one lengthens the other.  What moves the sum: the row writers' short waves at wave priority 3 (they
  // issue a dozen instructions between memory round trips: first in line they keep the store path fed, and the walk loses < 10 % of its slots) and,
  // from 1024 proofs on, the input sections in front of the new-key pipeline so that the stores start with the step: 512 / 1024 / 2048 proofs
  // 0.764 -> 0.741, 1.479 -> 1.422, 3.12 -> 2.81 ms.  (256 proofs: +1 % / +4.6 %: the latency regime keeps the round-5 form.)
  const uint64_t lanes_w = (uint64_t)n_proofs * c->cfg.n_max;
  prog.sp.wave_prio = K.writer_prio >= 0 ? (uint32_t)K.writer_prio : (lanes_w >= 65536 ? 3u : 0u);
  prog.sp.rows_major = K.ser_rows ? 1u : 0u;
  // (round 6: in the small form of the tail -- below 28 672 lanes, see tail_aside -- k_proof's sections + D.1a are ONE launch instead of four: 80 / 128 /
  // 208 proofs x 128 -1.6 / -4.5 / -2.6 %, N = 512 x 32 proofs -5.6 %, 20 ... 48 proofs level; at 256 proofs +2 %: profiles/r06_one_launch_ab.txt)
  const bool tail_aside_early = K.ser_split && (uint64_t)n_proofs * n >= (K.tail_aside_min >= 0 ? (uint64_t)K.tail_aside_min : 28672u);
  prog.sp.one_launch_max = K.one_launch_max >= 0 ? (uint32_t)K.one_launch_max : (tail_aside_early ? 8u : n_proofs);
  auto serialize = [&](uint32_t mask, hipStream_t on, uint32_t max_wgs = 0) -> int32_t {
    if (!d_out_elems) return TMX_OK;
    // (sections the caller did not ask for are not written; the seam spans are few and always written)
    mask &= ((c->sections & TMX_SEC_HINT) ? prog.mask_hint : 0u) | ((c->sections & TMX_SEC_DERIVED) ? prog.mask_derived : 0u) | (1u << 31);
    int r = launch_serialize(prog.sp, src, c->d_lut[kind], c->d_wave_sec[kind], c->d_seams[kind], (uint32_t)prog.seam_waves.size(), n_proofs,
                             d_out_elems, mask, on, max_wgs);
    if (r) return fail(c, TMX_ERR_HIP, std::string("k_serialize launch: ") + hipGetErrorString((hipError_t)r));
    return TMX_OK;
  };
  // (every record / wait is a packet the command processor handles in order: the caller's stream carries the critical path, so
  // events are shared where they mark the same point and joins are chained through the side streams)
  // One set of scratch buffers and join events per context: a call on another stream starts behind the previous call's end
  // (a no-op in the usual case of one stream per context)
  if (c->last_stream_valid && c->last_stream != s) HIPCK(c, hipStreamWaitEvent(s, c->ev_done, 0));
  HIPCK(c, hipEventRecord(ev[0], s));
  HIPCK(c, hipStreamWaitEvent(c->side, ev[0], 0));
  int32_t st0 = TMX_OK;
  int rc = 0;
  // (round 5, once the compaction and the validator-set cache had shortened the chain and the step's end was the row writes: 2048 workgroups at
  // 256 proofs 0.377 - 0.387 vs 0.395 - 0.410 ms with 1024; 512 / 768: 0.455 / 0.432; 3072 / 4096 / 8192: 0.385 / 0.381 / 0.393; no difference
  // at 64, 128, 512 and 1024 proofs)
  const uint64_t lanes_bc = (uint64_t)n_proofs * n;
  // (round 6, profiles/r06_writer_cap_sweep.txt: from 1024 proofs on -- where the leaves go first and the step is the sum of a VALU-bound chain
  // and an HBM-bound tail -- 8192 workgroups: 1024 / 1280 / 1536 proofs 1.557 -> 1.455, 2.008 -> 1.890, 2.358 -> 2.145 ms, 2048 proofs flat;
  // 512 to 1023 proofs 1536 instead of 1024: 640 / 768 / 896 proofs 1.11 -> 0.98, 1.164 -> 1.116, 1.332 -> 1.315 ms, 512 proofs unchanged)
  // (round 6, with the proof-major writer k_serialize_rows, profiles/r06_writer_cap_sweep2.txt: persistent writers hold their wave slots for
  // the whole launch and the chain's kernels wait for a slot; 32768 short-lived workgroups instead of 8192: 1024 / 1536 / 2048 proofs
  // 1.42 -> 1.28, 2.06 -> 1.91, 2.81 -> 2.59 ms; 65536: the same; 131072 and uncapped: +6 ... +10 %.  The whole throughput regime -- this cap,
  // the input sections first, the leaves first, D.1a early -- from THROUGHPUT_LANES on (first 98304: 768 / 896 proofs 1.08 -> 1.05, 1.25 -> 1.20 ms; then 81920: 672 / 704 / 736 proofs 0.894 -> 0.854, 0.943 -> 0.876, 1.011 -> 0.946, 640 level);
  // 512 / 640 proofs within +-2 % either way and left as they were)
  const bool throughput = lanes_bc >= THROUGHPUT_LANES;
  const uint32_t beside_chain_wgs = K.few_wgs > 0 ? (uint32_t)K.few_wgs : (throughput ? 32768u : (lanes_bc >= 65536 ? 1536u : (lanes_bc > 16384 ? 2048u : 1024u)));  // (warm key cache, 256 proofs: 2048 / 4096 / uncapped +10 / +4 / +2 %)
  // Leaves first (TMX_LEAVES=1|0, default by size): marshalled validators + leaf hashes as a 10-us launch of their own in front of k_proof,
  // so that the byte fields of the two per-lane derived sections (D.2a: the leaves; D.1a: the leaves + phase 1 -- 42 % of a skip row) are
  // written by the low-priority stream behind the input sections instead of behind k_proof (which ends at ~300 us inside a step) / k_ed_fin.
  // Measured at N = 128: -5 % step at 1024 proofs (on top of the -6 % of D.1a behind k_proof's sections), but +1.5 % at 256, +4.5 % at 512,
  // +8 % at 64: below ~1000 proofs every extra concurrent launch stretches the EdDSA chain by more than the tail it removes.
  const bool leaves_first = K.ser_split && d_out_elems && (K.leaves >= 0 ? K.leaves != 0 : throughput);
  // side: k_proof first -- for a single proof it IS the critical path, and every API call in front of its launch is latency --, its two
  // timing events on the dispatch itself; then the sections that only need its results
  const bool xp = K.ext_events && !leaves_first;
  if (!xp) HIPCK(c, hipEventRecord(evs[0], c->side));
  if (leaves_first) {
    rc = launch_leaves((uint32_t)kind, n, n_proofs, d_targets, d_trusteds, tl + TL_OFF_LT, TL_STRIDE, c->d_lr, c->side, K.ext_events ? c->ev_leaves : nullptr);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_leaves launch: ") + hipGetErrorString((hipError_t)rc));
    if (!K.ext_events) HIPCK(c, hipEventRecord(c->ev_leaves, c->side));
  }
  // k_proof as four role workgroups per proof where its latency is the call's (a handful of proofs, or no EdDSA stage beside it: the
  // validator-sharded finish); as one workgroup per proof in a batch, where 2048 role waves held up the EdDSA chain (256 proofs: 0.60
  // vs 0.41 ms) and k_proof is hidden behind it anyway (32 / 64 proofs: +-1 %)
  const uint64_t lanes_all = (uint64_t)n_proofs * n;
  const bool roles = K.proof_roles && c->d_tiny && (lanes_all <= 2048 || (!eddsa_writes_rows && lanes_all <= 16384));
  static_assert(PROOF_KERNEL_R168 == TMX_PROOF_PATH_R168 && PROOF_KERNEL_K256 == TMX_PROOF_PATH_K256 && PROOF_KERNEL_WIDE == TMX_PROOF_PATH_WIDE, "tmx.h");
  c->last_proof_path = roles ? TMX_PROOF_PATH_ROLES : (int32_t)proof_kernel_of(n);   // (launch_proof picks its kernel by the same function)
  if (!roles && c->setc.table && ++c->setc_epoch == 0) c->setc_epoch = 1;  // (ages are differences mod 2^32: a wrap is harmless)
  rc = roles
           ? launch_proof_roles(proof_params(c, kind, leaves_first), n_proofs, d_proofs, d_targets, d_trusteds, tl + TL_OFF_LT, TL_STRIDE, c->d_lr, c->d_pf,
                                c->d_nodes_t, c->d_nodes_r, reports, c->d_tiny, c->side, xp ? evs[0] : nullptr, xp ? evs[1] : nullptr)
           : launch_proof(proof_params(c, kind, leaves_first), n_proofs, d_proofs, d_targets, d_trusteds, tl + TL_OFF_LT, TL_STRIDE, c->d_lr, c->d_pf,
                          c->d_nodes_t, c->d_nodes_r, reports, c->side, xp ? evs[0] : nullptr, xp ? evs[1] : nullptr, c->setc);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_proof launch: ") + hipGetErrorString((hipError_t)rc));
  if (!xp) HIPCK(c, hipEventRecord(evs[1], c->side));
  // side3: the sections that are a pure expansion of the input records (42 % of a skip row) -- HBM is idle while EdDSA runs.
  // Launches that run beside the EdDSA latency chain are walked by a fixed number of workgroups (k_serialize_few): a memory-bound grid of
  // half a million short waves keeps every wave slot of the chip taken, and the chain's workgroups then wait for a slot whatever their
  // priority (a pure store stream beside the EdDSA stage: k_ed_keys 50 -> 103 us, the stage 0.42 -> 0.72 ms).  Four workgroups per CU
  // still write at the rate these sections need: step -3 % at 256 proofs x 128 (1024 workgroups; 512: the EdDSA stage -48 us but the
  // sections end after it), -4.5 % at 512, -3 % at 1024 (1536), -1 % at 64, +-0 at 32.
  // (the split warm schedule puts the new-key pipeline on side3 IN FRONT of these sections -- usually three empty launches; with new keys
  // the pipeline must not queue behind 200 us of trickling stores -- so the sections are enqueued behind the EdDSA stage then)
  c->plan = eddsa_writes_rows ? ed_plan(c, (uint32_t)lanes_all, true) : tmx_ctx::EdPlan{};
  // Fused rows (round 6; layout.h FusedRows): in the split warm schedule above 16384 lanes -- s*B and the resident walk are launches of their
  // own there, throughput-bound and on the chip from ~40 us on -- the input-only sections are not a launch that queues beside the chain but
  // work items the waves of those kernels claim between their table additions; the capped launch on side3 sweeps up what they leave.
  FusedRows fused = {};
  {
    const uint32_t in_mask = prog.mask_inputs & (((c->sections & TMX_SEC_HINT) ? prog.mask_hint : 0u) | ((c->sections & TMX_SEC_DERIVED) ? prog.mask_derived : 0u));
    const int fb = K.fused_base >= 0 ? K.fused_base : TMX_FUSED_BASE_DEFAULT, fw = K.fused_walk >= 0 ? K.fused_walk : TMX_FUSED_WALK_DEFAULT;
    if (c->plan.split && !c->plan.sb_with_hash && K.ser_split && d_out_elems && in_mask && (fb | fw) && c->d_span_ctr) {
      uint32_t lo = 0xffffffffu, hi = 0;
      for (uint32_t k = 0; k < prog.sp.n_sections; k++) {
        if (!((in_mask >> k) & 1u)) continue;
        const Section& sc = prog.sp.sec[k];
        lo = std::min(lo, sc.elem_start);
        hi = std::max(hi, sc.elem_start + sc.lane_elems * sc.n_lanes);
      }
      const uint32_t first = lo / prog.sp.span, last = (hi + prog.sp.span - 1) / prog.sp.span;
      if (prog.sp.span == SER_SPAN_ELEMS && last > first && (uint64_t)(last - first) * n_proofs < 0x7fffffffull) {
        if (c->span_ctr_dirty) { HIPCK(c, hipMemsetAsync(c->d_span_ctr, 0, 256, s)); c->span_ctr_dirty = false; }
        fused.ctr = c->d_span_ctr + 32 * c->span_parity;  // (the two counters on lines of their own)
        fused.lut = reinterpret_cast<const uint32_t*>(c->d_lut[kind]); fused.wave_sec = reinterpret_cast<const uint8_t*>(c->d_wave_sec[kind]);
        fused.out = reinterpret_cast<uint64_t*>(d_out_elems); fused.sec_mask = in_mask; fused.first_span = first; fused.n_spans = last - first;
        fused.n_proofs = n_proofs; fused.per_base = (uint32_t)fb; fused.per_walk = (uint32_t)fw;
        c->fused_prog = resolve_serialize_program(prog.sp, src);
      }
    }
  }
  auto side3_inputs = [&]() -> int32_t {
    HIPCK(c, hipStreamWaitEvent(c->side3, ev[0], 0));
    if (fused.ctr) {
      int r = launch_serialize_claim(c->fused_prog, fused, c->d_span_ctr + 32 * (c->span_parity ^ 1u), c->side3, beside_chain_wgs);
      if (r) c->span_ctr_dirty = true;
      if (r) return fail(c, TMX_ERR_HIP, std::string("k_serialize_claim launch: ") + hipGetErrorString((hipError_t)r));
      c->span_parity ^= 1u;
    } else if (K.ser_split && (st0 = serialize(prog.mask_inputs, c->side3, beside_chain_wgs))) return st0;
    if (leaves_first) {
      HIPCK(c, hipStreamWaitEvent(c->side3, c->ev_leaves, 0));
      if ((st0 = serialize(prog.mask_leaves, c->side3, beside_chain_wgs))) return st0;
    }
    HIPCK(c, hipEventRecord(c->ev_join3, c->side3));
    return TMX_OK;
  };
  const bool inputs_first = K.inputs_first_min >= 0 ? (K.inputs_first_min > 0 && lanes_bc >= (uint64_t)K.inputs_first_min) : throughput;
  const bool defer3 = c->plan.split && !inputs_first;
  if (!defer3 && (st0 = side3_inputs())) return st0;

  // ev[1] rides on the k_ed_fin dispatch itself (TMX_EXT_EVENTS=0: a record packet behind it)
  c->fin_done = K.ext_events ? ev[1] : nullptr;
  c->fin_done_attached = false;
  c->ev_hash_recorded = false;
  // D.1b (the word fields of the per-target-lane derived values: h, the ten coordinates, the verdict) goes straight from the EdDSA
  // finish into the rows when the EdDSA kernels run here (and k_verdict adds the lane's ten k_proof-derived elements): no serializer
  // launch behind the last kernel of the chain.  A producer that copies caller-provided lane records leaves the section to the serializer.
  RowOut row = {};
  if (eddsa_writes_rows && d_out_elems && (c->sections & TMX_SEC_DERIVED)) {
    row.rows = reinterpret_cast<uint64_t*>(d_out_elems); row.elem_stride = prog.sp.elem_stride; row.n = n; row.d1b_start = prog.d1b_start;
  }
  const uint32_t mask_final = row.rows ? 0u : prog.mask_final;
  c->row = row;
  c->fused = fused;
  int32_t st = ed_producer(s);
  c->fused = FusedRows{};
  if (fused.ctr && st) c->span_ctr_dirty = true;  // (the sweeper that zeroes the next counter was never enqueued)
  const bool fin_split = c->plan.split;  // (the lanes of new keys are finished on side2: whatever reads every lane's verdict on s waits for ev_direct)
  c->plan.valid = false;
  c->fin_done = nullptr;
  c->row = RowOut{};
  // the late epilogue (TMX_EPI_LATE): owed to the NEXT launch once the producer has enqueued the dedup -- on the error paths too, or that launch
  // would probe a dirty hash table behind an event that was never re-recorded
  auto late_epilogue = [&]() -> int32_t {
    if (!c->epilogue_pending) return TMX_OK;
    c->epilogue_pending = false;
    if ((size_t)c->hash_mask + 1 > KC_EPILOGUE_CLEARS_UP_TO) HIPCK(c, hipMemsetAsync(c->d_hash, 0xff, ((size_t)c->hash_mask + 1) * 4, c->side3));
    if ((rc = launch_kc_epilogue(c->pending_q, c->side3))) return fail(c, TMX_ERR_HIP, std::string("k_kc_epilogue launch: ") + hipGetErrorString((hipError_t)rc));
    HIPCK(c, hipEventRecord(c->ev_hash_clean, c->side3));
    HIPCK(c, hipEventRecord(c->ev_join3, c->side3));
    return TMX_OK;
  };
  if (st) { (void)late_epilogue(); return st; }
  if (defer3 && (st0 = side3_inputs())) { (void)late_epilogue(); return st0; }
  if ((st0 = late_epilogue())) return st0;
  if (leaves_first) {  // side3, behind the input sections and D.2a: D.1a as soon as phase 1 is done; ev_join3 moves behind it
    if (!c->ev_hash_recorded) HIPCK(c, hipEventRecord(c->ev_hash, s));  // (a producer without a phase-1 event: everything it enqueued)
    HIPCK(c, hipStreamWaitEvent(c->side3, c->ev_hash, 0));
    if ((st0 = serialize(prog.mask_p1, c->side3, beside_chain_wgs))) return st0;
    HIPCK(c, hipEventRecord(c->ev_join3, c->side3));
  }
  // (a small batch is pure latency: its tail stays on s, two cross-stream hops cost more than the overlap gains)
  // (round 6: the threshold moved from 4096 to 10240 lanes -- 32 / 48 / 64 proofs x 128: 0.210 -> 0.199, 0.222 -> 0.214, 0.259 -> 0.252 ms with the
  // one-launch tail on s; 96 proofs: 0.2625 aside vs 0.2715 on s.  profiles/r06_small_tail_ab.txt)
  // (round 6, with k_verdict_tail_wide as the one launch -- profiles/r06_tail_wide_ab.txt: 32 / 48 / 64 proofs 0.209 -> 0.204, 0.233 -> 0.224, 0.244 -> 0.225;
  // the one-launch form on s up to 28 672 lanes instead of 10 240: 80 / 96 / 160 / 208 proofs x 128 0.269 -> 0.257, 0.284 -> 0.273, 0.309 -> 0.300, 0.326 -> 0.318,
  // 224 / 240 level, 256 +1.4 %; N = 32: 512 / 768 proofs -3.7 / -1.8 %, 1024 +5 %; N = 512: 48 proofs -4 %, 32 / 64 level)
  const bool tail_aside = tail_aside_early;
  const bool small_tail = K.ser_split && !tail_aside;  // D.1a goes into the SAME launch as k_proof's sections (one launch, behind the hash event)
  if (small_tail && !leaves_first) {
    if (!c->ev_hash_recorded) HIPCK(c, hipEventRecord(c->ev_hash, s));  // (a producer without a phase-1 event: everything it enqueued)
    HIPCK(c, hipStreamWaitEvent(c->side, c->ev_hash, 0));
  }
  st0 = K.ser_split ? serialize(prog.mask_proof | (leaves_first ? 0u : prog.mask_leaves) | (small_tail && !leaves_first ? prog.mask_p1 : 0u), c->side) : TMX_OK;
  if (st0) return st0;
  // the validator-set cache's LRU: one workgroup behind k_proof and its sections on this stream (the next k_proof is behind it), off every chain
  if (!roles && c->setc.table && (rc = launch_setc_evict(c->setc, c->setc_epoch, c->side)))
    return fail(c, TMX_ERR_HIP, std::string("k_setc_evict launch: ") + hipGetErrorString((hipError_t)rc));
  // D.1a (the byte fields of the per-target-lane derived values: a quarter of the row) needs k_proof and phase 1, not k_ed_fin: behind
  // k_proof's sections on the side stream, i.e. while the table walk and the finish run.  Measured (round 2): -6.3 % step at 1024
  // proofs x 128; +-0.5 % at 256 and 64, +1 ... +2 % at 512 proofs (and +7 % at 256 with a warm key cache): on from 131072 lanes
  const bool p1_early = leaves_first || small_tail ||
                        (K.ser_split && c->ev_hash_recorded && (K.p1_early >= 0 ? K.p1_early != 0 : throughput));
  if (p1_early && !leaves_first && !small_tail) {
    HIPCK(c, hipStreamWaitEvent(c->side, c->ev_hash, 0));
    if ((st0 = serialize(prog.mask_p1, c->side, K.p1_early == 2 ? 0u : beside_chain_wgs))) return st0;
  }

  HIPCK(c, hipStreamWaitEvent(c->side, c->ev_join3, 0));  // ev_join = both low-priority streams done
  HIPCK(c, hipEventRecord(c->ev_join, c->side));
  if (!c->fin_done_attached) HIPCK(c, hipEventRecord(ev[1], s));
  if (small_tail) {
    // D.1a (needs the leaves and the hash role, both long done) goes with k_proof's sections on the side stream; what follows the join of
    // k_proof and the EdDSA finish on s is ONE launch: verdict + the sections that carry it + the seam spans (k_verdict_tail)
    if (fin_split && K.join1) {
      // ONE wait packet between the finish and the tail instead of two: side2 -- idle behind the new-key lanes' finish -- waits for k_proof and
      // records ev_direct again, which then stands for both
      HIPCK(c, hipStreamWaitEvent(c->side2, evs[1], 0));
      HIPCK(c, hipEventRecord(c->ev_direct, c->side2));
      HIPCK(c, hipStreamWaitEvent(s, c->ev_direct, 0));
    } else {
      HIPCK(c, hipStreamWaitEvent(s, evs[1], 0));
      if (fin_split) HIPCK(c, hipStreamWaitEvent(s, c->ev_direct, 0));
    }
    const bool xv = K.ext_events && n_proofs != 0;  // the verdict's two timing events ride on its dispatch
    if (!xv) HIPCK(c, hipEventRecord(evs[2], s));
    const bool with_rows = d_out_elems != nullptr;
    uint32_t tail_mask = (mask_final | prog.mask_tail) & (((c->sections & TMX_SEC_HINT) ? prog.mask_hint : 0u) | ((c->sections & TMX_SEC_DERIVED) ? prog.mask_derived : 0u) | (1u << 31));
    if (K.tail_wide && !(tail_mask & mask_final))  // (k_verdict_tail: one 1024-thread workgroup per proof expands D.5 and the seam spans element by element -- 21 us at 32 proofs, 82 at 256)
      rc = launch_verdict_tail_wide((uint32_t)kind, n, n_proofs, tl + TL_OFF_ED, TL_STRIDE, c->d_pf, reports, row, prog.sp, src, c->d_lut[kind], c->d_wave_sec[kind],
                                    c->d_seams[kind], (uint32_t)prog.seam_waves.size(), with_rows ? d_out_elems : nullptr, tail_mask, prog.tail_dep_elem, s,
                                    xv ? evs[2] : nullptr, xv ? evs[3] : nullptr);
    else
    rc = launch_verdict_tail((uint32_t)kind, n, n_proofs, tl + TL_OFF_ED, TL_STRIDE, c->d_pf, reports, row, prog.sp, src, c->d_lut[kind], c->d_seams[kind],
                             (uint32_t)prog.seam_waves.size(), with_rows ? d_out_elems : nullptr, tail_mask, s, xv ? evs[2] : nullptr, xv ? evs[3] : nullptr);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_verdict_tail launch: ") + hipGetErrorString((hipError_t)rc));
    if (!xv) HIPCK(c, hipEventRecord(evs[3], s));
    HIPCK(c, hipStreamWaitEvent(s, c->ev_join, 0));
  } else if (K.ser_split) {
    // tail: the per-lane derived section (a quarter of the row) only needs k_ed_fin + k_proof, so it is written on s while the
    // verdict and the few sections that carry it go through the high-priority side stream.  (ev[2] = ev[1] here: every packet
    // between k_ed_fin and the serializer is latency on the critical path.)
    // (the wait that is over first goes first: k_proof ends before the finish, and a wait packet behind the finish's is ~5 us of the tail's start)
    if (K.join1) {
      HIPCK(c, hipStreamWaitEvent(c->side2, evs[1], 0));  // k_proof itself, not the serializer launches queued behind it
      HIPCK(c, hipStreamWaitEvent(c->side2, ev[1], 0));
    } else {
    HIPCK(c, hipStreamWaitEvent(c->side2, ev[1], 0));
    HIPCK(c, hipStreamWaitEvent(c->side2, evs[1], 0));  // k_proof itself, not the serializer launches queued behind it
    }
    if (K.tail_wide && n_proofs) {
      const bool xv = K.ext_events;
      if (!xv) HIPCK(c, hipEventRecord(evs[2], c->side2));
      const uint32_t tail_mask = prog.mask_tail & (((c->sections & TMX_SEC_HINT) ? prog.mask_hint : 0u) | ((c->sections & TMX_SEC_DERIVED) ? prog.mask_derived : 0u) | (1u << 31));
      rc = launch_verdict_tail_wide((uint32_t)kind, n, n_proofs, tl + TL_OFF_ED, TL_STRIDE, c->d_pf, reports, row, prog.sp, src, c->d_lut[kind], c->d_wave_sec[kind],
                                    c->d_seams[kind], (uint32_t)prog.seam_waves.size(), d_out_elems, tail_mask, prog.tail_dep_elem, c->side2,
                                    xv ? evs[2] : nullptr, xv ? evs[3] : nullptr);
      if (rc) return fail(c, TMX_ERR_HIP, std::string("k_verdict_tail_wide launch: ") + hipGetErrorString((hipError_t)rc));
      if (!xv) HIPCK(c, hipEventRecord(evs[3], c->side2));
    } else {
    HIPCK(c, hipEventRecord(evs[2], c->side2));
    rc = launch_verdict((uint32_t)kind, n, n_proofs, tl + TL_OFF_ED, TL_STRIDE, c->d_pf, reports, row, c->side2);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_verdict launch: ") + hipGetErrorString((hipError_t)rc));
    HIPCK(c, hipEventRecord(evs[3], c->side2));
    if ((st0 = serialize(prog.mask_tail, c->side2))) return st0;
    }
    HIPCK(c, hipStreamWaitEvent(c->side2, c->ev_join, 0));  // ev_tail = every side stream done
    HIPCK(c, hipEventRecord(c->ev_tail, c->side2));
    if (mask_final | (p1_early ? 0u : prog.mask_p1)) {
      HIPCK(c, hipStreamWaitEvent(s, evs[1], 0));
      if ((st0 = serialize(mask_final | (p1_early ? 0u : prog.mask_p1), s))) return st0;
    }
    HIPCK(c, hipStreamWaitEvent(s, c->ev_tail, 0));
  } else {
    HIPCK(c, hipStreamWaitEvent(s, c->ev_join, 0));
    if (fin_split) HIPCK(c, hipStreamWaitEvent(s, c->ev_direct, 0));
    HIPCK(c, hipEventRecord(evs[2], s));
    rc = launch_verdict((uint32_t)kind, n, n_proofs, tl + TL_OFF_ED, TL_STRIDE, c->d_pf, reports, row, s);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_verdict launch: ") + hipGetErrorString((hipError_t)rc));
    HIPCK(c, hipEventRecord(evs[3], s));
    HIPCK(c, hipEventRecord(ev[2], s));
    if ((st0 = serialize(prog.mask_inputs | prog.mask_proof | prog.mask_leaves | mask_final | prog.mask_p1 | prog.mask_tail, s))) return st0;
  }
  HIPCK(c, hipEventRecord(ev[3], s));
  c->slot_tiny[slot] = false;
  c->last_stream = s; c->last_stream_valid = true;
  c->ev_done = ev[3];
  c->last_kind = kind; c->last_n_proofs = n_proofs;
  c->n_calls++;
  return TMX_OK;
}

// ---- the small-launch path (kernels.h TinyLaunch, tiny.hpp): <= TINY_MAX_LANES validator lanes.
// Two launches on the caller's stream, no cross-stream hand-off in front of any of them: k_tiny (every role that needs only the input
// records) and k_tiny_tail (checks, verdict, the sections that needed k_tiny).  A lane whose key is not resident is computed table-free
// inside its workgroup.  The key cache is only READ by k_tiny; its bookkeeping is the classic key pipeline, unchanged, enqueued on the
// high-priority side stream BEHIND k_tiny over the context's shadow copy of the lanes' keys (k_ed_dedup -> k_ed_keys -> tables of the new
// keys -> k_kc_epilogue): hit / miss counters, LRU stamps, insertion, eviction and the schedule hint are exactly what a classic launch
// leaves, and nothing reads the caller's buffers once the caller's stream is done.  TMX_TINY=0 never takes this path.
static bool use_tiny(const tmx_ctx* c, uint64_t n_lanes) {
  const Knobs& K = c->knobs;
  // (round 6: up to 1536 lanes instead of TINY_MAX_LANES = 2048 -- with the validator-set cache, the one-launch tail and the one-launch sections the
  // classic graph needs 0.18 - 0.205 ms at 13 ... 16 proofs x 128 where the two launches need 0.207 ... 0.225 (a workgroup per lane: their time grows
  // with the lanes); N = 64: 28 proofs 0.216 -> 0.201; N = 512: 4 proofs 0.51 -> 0.44; N = 32 loses 3 - 5 % between 1536 and 2048 lanes.
  // profiles/r06_small_batches_ab.txt)
  // (small validator sets keep the old bound: N = 32 x 56 / 64 proofs 0.222 / 0.219 on the small path against 0.228 / 0.230)
  const uint64_t tiny_max = K.tiny_max >= 0 ? std::min<uint64_t>((uint64_t)K.tiny_max, TINY_MAX_LANES) : (c->cfg.n_max <= 32 ? TINY_MAX_LANES : 1536u);
  if (K.tiny == 0 || n_lanes == 0 || n_lanes > tiny_max || !c->d_tiny || !c->d_shadow) return false;
  if (c->kc.cap == 0 || K.dedup_mode == 0) return false;  // (TMX_DEDUP=0: no per-key tables at all -- the classic table-free kernels)
  if (K.warm_schedule >= 0 && K.tiny < 0) return false;   // a forced schedule names one of the classic graphs
  return true;
}
static void tiny_common(tmx_ctx* c, TinyLaunch& T, uint32_t n_lanes, const void* d_lanes, void* d_ed, uint32_t ed_stride) {
  std::memset(&T, 0, sizeof T);
  T.n_lanes = n_lanes; T.d_target = d_lanes; T.d_ed = d_ed; T.ed_stride = ed_stride;
  T.d_qtable = c->d_qtable; T.d_keytab = c->d_keytab; T.d_keyrec = c->d_keyrec; T.kc = c->kc; T.d_tiny = c->d_tiny; T.d_shadow = c->d_shadow;
  c->last_lanes = n_lanes;
}
// the ordering a small launch needs in front of it: the previous batch if it ran on another stream, and the tail of the key pipeline
// the previous launch left on the side stream (it may still be inserting keys into the cache this launch probes)
static int32_t tiny_order(tmx_ctx* c, hipStream_t s) {
  if (c->last_stream_valid && c->last_stream != s) HIPCK(c, hipStreamWaitEvent(s, c->ev_done, 0));
  // (an isolated call finds the previous key pipeline long finished: a host-side query instead of a wait packet in front of the first launch)
  if (hipEventQuery(c->ev_hash_clean) != hipSuccess) {
    (void)hipGetLastError();
    HIPCK(c, hipStreamWaitEvent(s, c->ev_hash_clean, 0));
  }
  return TMX_OK;
}
// the cache bookkeeping of a small launch: the classic key pipeline on side2, behind k_tiny (event `after`), over the shadow records
static int32_t tiny_key_pipeline(tmx_ctx* c, uint32_t n_lanes, hipEvent_t after) {
  const Knobs& K = c->knobs;
  EdQuad Q;
  std::memset(&Q, 0, sizeof Q);
  Q.n_lanes = n_lanes; Q.d_target = c->d_shadow; Q.d_qtable = c->d_qtable; Q.d_pre = c->d_pre; Q.d_mulout = c->d_mulout;
  Q.d_hash = c->d_hash; Q.hash_mask = c->hash_mask; Q.d_owner_of = c->d_owner_of; Q.d_slot_of_owner = c->d_slot_of_owner;
  Q.d_slot_of_uid = c->d_slot_of_uid; Q.d_owners = c->d_owners; Q.d_keyrec = c->d_keyrec; Q.d_anchors = c->d_anchors; Q.d_keytab = c->d_keytab;
  Q.kc = c->kc; Q.mode = K.dedup_mode;
  Q.d_cnt = reinterpret_cast<uint32_t*>(c->d_cnt) + 8 * c->parity;
  Q.d_cnt_next = reinterpret_cast<uint32_t*>(c->d_cnt) + 8 * (c->parity ^ 1);
  c->parity ^= 1;
  Q.use_new = 0;  // nobody waits for the tables of this launch: they are for the next call
  Q.warm = (c->kc.persist && c->h_hint && c->h_hint[0] != 0 && c->h_hint[1] == 0) ? 1u : 0u;  // (grid sizes of the new-key kernels only)
  HIPCK(c, hipStreamWaitEvent(c->side2, after, 0));
  int rc = launch_ed_dedup(Q, c->side2);
  if (!rc) rc = launch_ed_keys(Q, c->side2);
  if (!rc) rc = launch_ed_tab_anchor(Q, 0, 1, c->side2);
  if (!rc) rc = launch_ed_tab_mult(Q, 0, 1, c->side2);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("key pipeline launch: ") + hipGetErrorString((hipError_t)rc));
  if ((size_t)c->hash_mask + 1 > KC_EPILOGUE_CLEARS_UP_TO) HIPCK(c, hipMemsetAsync(c->d_hash, 0xff, ((size_t)c->hash_mask + 1) * 4, c->side2));
  rc = launch_kc_epilogue(Q, c->side2);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_kc_epilogue launch: ") + hipGetErrorString((hipError_t)rc));
  HIPCK(c, hipEventRecord(c->ev_hash_clean, c->side2));
  return TMX_OK;
}
static int32_t run_tiny_lanes(tmx_ctx* c, uint32_t n_lanes, const void* d_lanes, void* d_ed, uint32_t ed_stride, hipStream_t s) {
  int32_t st = tiny_order(c, s);
  if (st) return st;
  TinyLaunch T;
  tiny_common(c, T, n_lanes, d_lanes, d_ed, ed_stride);
  const bool x = c->knobs.ext_events;
  int rc = launch_tiny(T, s, nullptr, x ? c->ev_fork2 : nullptr);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_tiny launch: ") + hipGetErrorString((hipError_t)rc));
  if (!x) HIPCK(c, hipEventRecord(c->ev_fork2, s));
  return tiny_key_pipeline(c, n_lanes, c->ev_fork2);
}
static int32_t run_tiny(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets, const void* d_trusteds,
                        void* d_out_elems, void* d_reports, hipStream_t s) {
  const uint32_t n = c->cfg.n_max;
  const Knobs& K = c->knobs;
  int32_t st = tiny_order(c, s);
  if (st) return st;
  uint8_t* tl = reinterpret_cast<uint8_t*>(c->d_tl);
  const uint64_t slot = c->n_calls % tmx_ctx::EV_RING;
  hipEvent_t* ev = c->ev[slot];
  const Program& prog = c->prog[kind];
  SerializeSources src;
  std::memset(&src, 0, sizeof src);
  src.base[SRC_TARGET] = (const uint8_t*)d_targets; src.base[SRC_TRUSTED] = (const uint8_t*)d_trusteds;
  src.base[SRC_TL] = tl; src.base[SRC_LR] = (const uint8_t*)c->d_lr; src.base[SRC_PF] = (const uint8_t*)c->d_pf;
  src.nodes_t = (const uint8_t*)c->d_nodes_t; src.nodes_r = (const uint8_t*)c->d_nodes_r;
  TinyLaunch T;
  tiny_common(c, T, n_proofs * n, d_targets, tl + TL_OFF_ED, TL_STRIDE);
  T.n_proofs = n_proofs; T.P = proof_params(c, kind, false); T.d_proofs = d_proofs; T.d_trusted = d_trusteds;
  T.d_lt = tl + TL_OFF_LT; T.lt_stride = TL_STRIDE; T.d_lr = c->d_lr; T.d_pf = c->d_pf; T.d_nodes_t = c->d_nodes_t; T.d_nodes_r = c->d_nodes_r;
  T.d_reports = d_reports ? d_reports : c->d_reports;
  T.S = &prog.sp; T.src = &src; T.d_lut = c->d_lut[kind]; T.d_wave_sec = c->d_wave_sec[kind]; T.d_seams = c->d_seams[kind];
  T.n_seams = (uint32_t)prog.seam_waves.size(); T.d_out = d_out_elems;
  // sections the caller asked for (the seam spans are few and always written); D.1b goes straight from the finish into the rows
  const uint32_t want = ((c->sections & TMX_SEC_HINT) ? prog.mask_hint : 0u) | ((c->sections & TMX_SEC_DERIVED) ? prog.mask_derived : 0u) | (1u << 31);
  if (d_out_elems && (c->sections & TMX_SEC_DERIVED)) {
    T.row.rows = reinterpret_cast<uint64_t*>(d_out_elems); T.row.elem_stride = prog.sp.elem_stride; T.row.n = n; T.row.d1b_start = prog.d1b_start;
  }
  T.mask_inputs = prog.mask_inputs & want;
  T.mask_after = (prog.mask_proof | prog.mask_leaves | prog.mask_p1 | (T.row.rows ? 0u : prog.mask_final)) & want;
  T.mask_tail = prog.mask_tail & want;
  T.tail_dep_elem = prog.tail_dep_elem;
  const bool x = K.ext_events;
  if (!x) HIPCK(c, hipEventRecord(ev[0], s));
  int rc = launch_tiny(T, s, x ? ev[0] : nullptr, x ? ev[1] : nullptr);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_tiny launch: ") + hipGetErrorString((hipError_t)rc));
  if (!x) { HIPCK(c, hipEventRecord(ev[1], s)); HIPCK(c, hipEventRecord(ev[2], s)); }
  rc = launch_tiny_tail(T, s, x ? ev[2] : nullptr, x ? ev[3] : nullptr);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_tiny_tail launch: ") + hipGetErrorString((hipError_t)rc));
  if (!x) HIPCK(c, hipEventRecord(ev[3], s));
  // (enqueued after both launches of the caller's stream: the key pipeline is nobody's critical path)
  if ((st = tiny_key_pipeline(c, n_proofs * n, ev[1]))) return st;
  c->last_proof_path = TMX_PROOF_PATH_TINY;
  c->slot_tiny[slot] = true;
  c->last_stream = s; c->last_stream_valid = true;
  c->ev_done = ev[3];
  c->last_kind = kind; c->last_n_proofs = n_proofs;
  c->n_calls++;
  return TMX_OK;
}

static int32_t check_batch_args(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets, const void* d_trusteds) {
  if (!c || (kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP) || !d_proofs || !d_targets) return TMX_ERR_BAD_ARG;
  if (kind == TMX_KIND_SKIP && !d_trusteds) return fail(c, TMX_ERR_BAD_ARG, "skip needs the trusted hash fields");
  if (n_proofs > c->cfg.max_batch) return fail(c, TMX_ERR_CAPACITY, "n_proofs exceeds the context's max_batch");
  return TMX_OK;
}

// EdDSA stage: begins and ends on stream s.  The new-key pipeline (decode -> doubling chain -> window tables -> cache epilogue) runs on
// the high-priority stream side2; what s does beside it depends on what the launch EXPECTS (the epilogue of the last finished launch left
// a hint in page-locked memory: did it see new keys?) -- either schedule is correct for any input, the expectation only picks the faster:
//   cold (new keys expected):  s: dedup -> phase 1 (hash | s*B) -> [keys] table-free lanes -> [tables, part by part] walk -> finish
//   warm (keys resident):      s: dedup -> hash -> [tables] walk -> [s*B and the table-free lanes, on side2] -> finish
//                              -- the walk waits for the hash role only, nothing empty is launched on s, the new-key kernels are
//                              small grids that find nothing to do long before the hash role ends, and s*B (which only the finish
//                              needs) fills the machine beside the 512 latency-bound waves of the hash role
//   tiny (<= 512 lanes):       s: dedup -> phase 1 -> walk of the resident keys -> [table-free lanes + their finish, on side2] -> finish;
//                              never waits for tables: the tables of new keys are built on side2 for the next call
static int run_eddsa(tmx_ctx* c, uint32_t n_lanes, const void* d_lanes, void* d_ed, uint32_t ed_stride, hipStream_t s) {
  const Knobs& K = c->knobs;
  EdQuad Q;
  Q.n_lanes = n_lanes; Q.d_target = d_lanes; Q.d_ed = d_ed; Q.ed_stride = ed_stride; Q.d_qtable = c->d_qtable; Q.d_pre = c->d_pre;
  Q.d_mulout = c->d_mulout; Q.d_hash = c->d_hash; Q.hash_mask = c->hash_mask; Q.d_owner_of = c->d_owner_of;
  Q.d_slot_of_owner = c->d_slot_of_owner; Q.d_slot_of_uid = c->d_slot_of_uid; Q.d_owners = c->d_owners; Q.d_keyrec = c->d_keyrec;
  Q.d_anchors = c->d_anchors; Q.d_keytab = c->d_keytab;
  Q.kc = c->kc; Q.mode = K.dedup_mode;
  Q.fin_done = c->fin_done; c->fin_done = nullptr;
  Q.row = c->row;
  Q.fused = c->fused; Q.fused_prog = c->fused_prog;
  c->last_lanes = n_lanes;
  Q.d_cnt = reinterpret_cast<uint32_t*>(c->d_cnt) + 8 * c->parity;
  Q.d_cnt_next = reinterpret_cast<uint32_t*>(c->d_cnt) + 8 * (c->parity ^ 1);
  c->parity ^= 1;
  const tmx_ctx::EdPlan plan = c->plan.valid ? c->plan : ed_plan(c, n_lanes, false);
  const bool tiny = plan.tiny, warm = plan.warm;
  // Compacted launch (kernels.h EdQuad): wherever the dedup opens the chain on s -- the warm schedules above 16384 lanes and every cold
  // launch.  (Up to 16384 lanes a warm launch opens with the hash role instead, the dedup beside it: those launches are latency-bound,
  // fewer lanes do not shorten them -- measured: 0.244 / 0.261 / 0.285 ms compacted against 0.200 / 0.251 / 0.261 at 32 / 64 / 128 proofs.)
  Q.compact = (c->dummy_ready && K.compact && !tiny && n_lanes > 2048 && !plan.hash_first && Q.mode != 0 && Q.kc.cap != 0) ? 1u : 0u;
  Q.d_live = c->d_live; Q.d_dummy_ed = c->d_dummy_ed;
  Q.use_new = tiny ? 0u : 1u;
  Q.warm = warm ? 1u : 0u;
  hipError_t e;
  // (the launch's hash table was cleared, and the cache committed, on side2 by the previous launch.  Skipping this wait when s has
  // already waited for side2's tail was measured: k_proof 0.45 -> 0.52 ms beside it and the step +2 % at 256 proofs -- the packet stays.)
  // Hash first (warm schedule, not tiny): SHA-512 mod l reads the lane records only, so it opens the chain on s while the dedup (cache
  // probe) and the key pipeline run on a side stream -- the walk waits for its ev_part[0] either way.  s then carries no wait for
  // ev_hash_clean; the side stream that runs the dedup does (the previous launch's tail may have run on the other one).
  const bool hash_first = plan.hash_first;
  // Events that mark the end of one kernel ride on its dispatch (completion signal) instead of a record packet behind it: on the
  // chain every packet is latency.  `x` = that is on and the kernel really is launched.
  const bool x = K.ext_events && n_lanes != 0, xt = x && Q.mode != 0 && Q.kc.cap != 0;
  int rc = 0;
  const bool sb_with_hash_hf = plan.sb_with_hash;
  if (plan.split) {
    // ---- warm, split by residency (round 5).  Three chains that meet only where the data says so:
    //   s      [dedup] -> hash -> walk of the RESIDENT lanes -> [s*B] finish of the RESIDENT lanes          (the critical chain: waits for no table)
    //   side3  [dedup] -> k_ed_keys -> anchors -> multiples -> cache epilogue                                (the new-key pipeline: usually four empty launches)
    //   side2  s*B -> [tables, hash] walk of the NEW-KEY lanes -> table-free lanes -> finish of both         (usually: s*B and three empty launches)
    // Round 4 ran the new-key kernels and s*B one after the other on side2 and made the whole walk and the whole finish wait for them:
    // four new keys of 401 -- the daily churn of a validator set -- stalled 32 768 lanes behind a decode + 252-doubling chain + 60 us of
    // s*B (+28 % step).  Now only the lanes that need the new tables wait for them, and the lanes' D.1b rows are written by whichever
    // finish owns the lane.  Everything that reads ALL lanes' verdicts (k_verdict, on side2 itself or behind ev_direct) is ordered after both.
    hipStream_t kq = c->side3;
    if (hash_first) {
      if ((e = hipEventRecord(c->ev_fork2, s)) != hipSuccess) return (int)e;
    } else {
      if ((e = hipStreamWaitEvent(s, c->ev_hash_clean, 0)) != hipSuccess) return (int)e;
      if ((rc = launch_ed_dedup(Q, s, x ? c->ev_fork2 : nullptr))) return rc;
      if (!x && (e = hipEventRecord(c->ev_fork2, s)) != hipSuccess) return (int)e;
    }
    rc = plan.sb_with_hash ? launch_ed_phase1(Q, s, x ? c->ev_hash : nullptr) : launch_ed_hash(Q, s, x ? c->ev_hash : nullptr);
    if (rc) return rc;
    if (!x && (e = hipEventRecord(c->ev_hash, s)) != hipSuccess) return (int)e;
    c->ev_hash_recorded = true;
    // Enqueue order = the order of need: a step that starts on an idle device (a single call behind a synchronize) is launched at the pace of
    // the host, ~4 us per call, and the resident walk used to be the twelfth launch of the stage (it started at ~125 instead of ~70 us):
    // the head of the new-key chain (it is the longer one when there are new keys), s*B, the resident walk and finish, then the rest.
    if (hash_first) {  // the dedup beside the hash role; the walk reads the owners it writes (ev_keys: free in this schedule)
      if ((e = hipStreamWaitEvent(kq, c->ev_fork2, 0)) != hipSuccess) return (int)e;
      // The previous launch's key-pipeline tail (hash table cleared, cache committed) may sit on ANOTHER stream than kq: a tiny call, a cold
      // or a non-split launch leave it on side2.  Without this wait the dedup raced it on d_hash / owner_of / the cache.
      // A no-op packet when the tail was on kq itself (split launch after split launch: the usual case).
      if ((e = hipStreamWaitEvent(kq, c->ev_hash_clean, 0)) != hipSuccess) return (int)e;
      if ((rc = launch_ed_dedup(Q, kq, x ? c->ev_keys : nullptr))) return rc;
      if (!x && (e = hipEventRecord(c->ev_keys, kq)) != hipSuccess) return (int)e;
      if ((e = hipStreamWaitEvent(s, c->ev_keys, 0)) != hipSuccess) return (int)e;
    }
    // side3: the new-key pipeline and the end of the launch's cache bookkeeping
    if (!hash_first && (e = hipStreamWaitEvent(kq, c->ev_fork2, 0)) != hipSuccess) return (int)e;
    if ((rc = launch_ed_keys(Q, kq, xt ? c->ev_part[1] : nullptr))) return rc;
    if (!xt && (e = hipEventRecord(c->ev_part[1], kq)) != hipSuccess) return (int)e;
    if ((rc = launch_ed_tab_anchor(Q, 0, 1, kq))) return rc;
    if ((rc = launch_ed_tab_mult(Q, 0, 1, kq, xt ? c->ev_part[0] : nullptr))) return rc;
    if (!xt && (e = hipEventRecord(c->ev_part[0], kq)) != hipSuccess) return (int)e;
    // (the epilogue -- one 1024-thread workgroup that needs sixteen free wave slots on one CU: 50 - 65 us to get them on the busy chip -- and the
    // clearing of the launch's hash table are needed by the NEXT launch only: run_batch enqueues them behind the input sections of side3, which then
    // start at ~70 instead of ~160 us.  0.401 -> 0.391, 0.382 -> 0.376 ms once the step's end was the row writes: round 5, after the compaction)
    if (K.epi_late) {
      c->epilogue_pending = true; c->pending_q = Q;
    } else {
      if ((size_t)c->hash_mask + 1 > KC_EPILOGUE_CLEARS_UP_TO && (e = hipMemsetAsync(c->d_hash, 0xff, ((size_t)c->hash_mask + 1) * 4, kq)) != hipSuccess) return (int)e;
      if ((rc = launch_kc_epilogue(Q, kq))) return rc;
      if ((e = hipEventRecord(c->ev_hash_clean, kq)) != hipSuccess) return (int)e;
    }
    // side2: s*B (a launch of its own above 16384 lanes), then the lanes that are not resident
    if ((e = hipStreamWaitEvent(c->side2, c->ev_fork2, 0)) != hipSuccess) return (int)e;
    if (!plan.sb_with_hash) {
      if ((rc = launch_ed_base(Q, c->side2, x ? c->ev_base : nullptr))) return rc;
      if (!x && (e = hipEventRecord(c->ev_base, c->side2)) != hipSuccess) return (int)e;
    }
    // s: the resident lanes
    if ((rc = launch_ed_mul_tab(Q, 0, 1, s, 1u))) return rc;
    if (!plan.sb_with_hash && (e = hipStreamWaitEvent(s, c->ev_base, 0)) != hipSuccess) return (int)e;
    rc = launch_ed_fin(Q, s, false, 1u);
    c->fin_done_attached = rc == 0 && Q.fin_done != nullptr;
    if (rc) return rc;
    // (the table-free lanes -- keys the cache has no room for: usually an empty launch -- need the decoded keys, not the tables: in front of
    // the wait for the tables instead of 12 us between the walk and the finish of the new-key lanes)
    if ((e = hipStreamWaitEvent(c->side2, c->ev_part[1], 0)) != hipSuccess) return (int)e;
    if ((e = hipStreamWaitEvent(c->side2, c->ev_hash, 0)) != hipSuccess) return (int)e;
    if ((rc = launch_ed_mul_direct(Q, c->side2, false, nullptr))) return rc;
    if ((e = hipStreamWaitEvent(c->side2, c->ev_part[0], 0)) != hipSuccess) return (int)e;
    if ((rc = launch_ed_mul_tab(Q, 0, 1, c->side2, 2u))) return rc;
    {
      EdQuad Q2 = Q;
      Q2.fin_done = nullptr;
      if ((rc = launch_ed_fin(Q2, c->side2, false, 2u))) return rc;
    }
    if ((e = hipEventRecord(c->ev_direct, c->side2)) != hipSuccess) return (int)e;
    return rc;
  }
  if (hash_first) {
    if ((e = hipEventRecord(c->ev_fork2, s)) != hipSuccess) return (int)e;
    rc = sb_with_hash_hf ? launch_ed_phase1(Q, s, x ? c->ev_hash : nullptr) : launch_ed_hash(Q, s, x ? c->ev_hash : nullptr);
    if (rc) return rc;
    if (!x && (e = hipEventRecord(c->ev_hash, s)) != hipSuccess) return (int)e;
    c->ev_hash_recorded = true;
    if ((e = hipStreamWaitEvent(c->side2, c->ev_fork2, 0)) != hipSuccess) return (int)e;
    // (the previous launch's tail is on side3 when that launch took the split schedule: side2's own order does not cover it)
    if ((e = hipStreamWaitEvent(c->side2, c->ev_hash_clean, 0)) != hipSuccess) return (int)e;
    rc = launch_ed_dedup(Q, c->side2, nullptr);
    if (rc) return rc;
  } else {
    if ((e = hipStreamWaitEvent(s, c->ev_hash_clean, 0)) != hipSuccess) return (int)e;
    rc = launch_ed_dedup(Q, s, x ? c->ev_fork2 : nullptr);
    if (rc) return rc;
    if (!x && (e = hipEventRecord(c->ev_fork2, s)) != hipSuccess) return (int)e;
    if ((e = hipStreamWaitEvent(c->side2, c->ev_fork2, 0)) != hipSuccess) return (int)e;
  }
  rc = launch_ed_keys(Q, c->side2, x ? c->ev_keys : nullptr);
  if (rc) return rc;
  if (!x && (e = hipEventRecord(c->ev_keys, c->side2)) != hipSuccess) return (int)e;
  // the end of side2's part of a launch: the launch's hash table cleared for the next one, the cache committed
  auto side2_tail = [&]() -> int {
    hipError_t e2;
    if ((size_t)c->hash_mask + 1 > KC_EPILOGUE_CLEARS_UP_TO &&  // (small tables: the epilogue clears them itself)
        (e2 = hipMemsetAsync(c->d_hash, 0xff, ((size_t)c->hash_mask + 1) * 4, c->side2)) != hipSuccess) return (int)e2;
    // (with parts > 1 the multiples of the earlier parts run on s: the epilogue only needs the counters k_ed_keys left, not the tables)
    int r2 = launch_kc_epilogue(Q, c->side2);
    if (r2) return r2;
    return (int)hipEventRecord(c->ev_hash_clean, c->side2);
  };
  // the table-free lanes on side2, behind the hash role of s (their h) -- off s, where an empty launch costs ~10 us of the chain
  auto direct_on_side2 = [&](bool fuse) -> int {
    hipError_t e2;
    if ((e2 = hipStreamWaitEvent(c->side2, c->ev_hash, 0)) != hipSuccess) return (int)e2;
    int r2 = launch_ed_mul_direct(Q, c->side2, fuse, x ? c->ev_direct : nullptr);
    if (r2) return r2;
    if (!x && (e2 = hipEventRecord(c->ev_direct, c->side2)) != hipSuccess) return (int)e2;
    return 0;
  };

  if (tiny || warm) {
    // hash role (tiny: all of phase 1 -- a launch of a few waves is pure latency, its roles side by side) on s
    // (a few thousand lanes: s*B as a role of the same launch as the hash, as in a tiny launch -- on side2 it started behind three empty
    // launches, ran into the walk and held the finish back by ~50 us: profiles/r04_p32_timeline.txt)
    const bool sb_with_hash = plan.sb_with_hash;
    if (!hash_first) {
      rc = sb_with_hash ? launch_ed_phase1(Q, s, x ? c->ev_hash : nullptr) : launch_ed_hash(Q, s, x ? c->ev_hash : nullptr);
      if (rc) return rc;
      if (!x && (e = hipEventRecord(c->ev_hash, s)) != hipSuccess) return (int)e;
      c->ev_hash_recorded = true;
    }
    // (up to 256 lanes the finish of the table-free lanes is fused into their kernel: at 512 the 512 waves of the fused kernel slow
    // k_proof, the longer of the two there, by more than they save)
    const bool fuse = tiny && n_lanes <= 256;
    if (tiny && (rc = direct_on_side2(fuse))) return rc;  // first on side2: a cold single proof is this kernel's latency
    rc = launch_ed_tab_anchor(Q, 0, 1, c->side2);
    if (rc) return rc;
    rc = launch_ed_tab_mult(Q, 0, 1, c->side2, xt ? c->ev_part[0] : nullptr);
    if (rc) return rc;
    if (!xt && (e = hipEventRecord(c->ev_part[0], c->side2)) != hipSuccess) return (int)e;
    if (!tiny) {  // s*B (only the finish needs it) beside the hash role and the walk, then the table-free lanes: ev_direct = both done
      rc = sb_with_hash ? 0 : launch_ed_base(Q, c->side2);
      if (rc) return rc;
      if ((rc = direct_on_side2(false))) return rc;
    }
    if ((rc = side2_tail())) return rc;
    if (!tiny && (e = hipStreamWaitEvent(s, c->ev_part[0], 0)) != hipSuccess) return (int)e;  // (an expectation that fails: s waits for the build)
    rc = launch_ed_mul_tab(Q, 0, 1, s);
    if (rc) return rc;
    if ((e = hipStreamWaitEvent(s, c->ev_direct, 0)) != hipSuccess) return (int)e;
    rc = launch_ed_fin(Q, s, fuse);
    c->fin_done_attached = rc == 0 && Q.fin_done != nullptr;
    return rc;
  }

  // The anchor chain is cut into `parts` launches on side2; the cached multiples of part p are built on s (idle once phase 1 is
  // done) while side2 doubles part p+1, so that only the multiples of the last part follow the chain.
  // (small launches: one part -- nothing to overlap, and every part is one more launch on s)
  const uint32_t parts = n_lanes <= 2048 ? 1u : 2u;  // (4 parts: no further gain)
  for (uint32_t p = 0; p < parts; p++) {
    const bool last = p + 1 == parts;
    rc = launch_ed_tab_anchor(Q, p, parts, c->side2, xt && !last ? c->ev_part[p] : nullptr);
    if (rc) return rc;
    if (last) {  // the multiples of the last part stay on the high-priority stream: nothing is left to overlap them with
      rc = launch_ed_tab_mult(Q, p, parts, c->side2, xt ? c->ev_part[p] : nullptr);
      if (rc) return rc;
    }
    if (!xt && (e = hipEventRecord(c->ev_part[p], c->side2)) != hipSuccess) return (int)e;
  }
  if ((rc = side2_tail())) return rc;
  // phase 1 (SHA-512 mod l, s*B: throughput work for every lane) on s
  rc = launch_ed_phase1(Q, s, x ? c->ev_hash : nullptr);
  if (rc) return rc;
  if (!x && (e = hipEventRecord(c->ev_hash, s)) != hipSuccess) return (int)e;
  c->ev_hash_recorded = true;
  if ((e = hipStreamWaitEvent(s, c->ev_keys, 0)) != hipSuccess) return (int)e;
  rc = launch_ed_mul_direct(Q, s);  // exits at once for the lanes that walk a table: enqueued before the wait for the tables
  if (rc) return rc;
  // The table walk can follow the table build part by part (partial sums in mulout).  Measured: +4 % step time at 256-512 proofs (the
  // parts sit on the caller's normal-priority queue beside the chain), -2.7 % at 1024, where the walk dominates -> by batch size.
  const bool walk_parts = parts > 1 && (K.walk_parts >= 0 ? K.walk_parts == 1 : n_lanes >= 65536);
  for (uint32_t p = 0; p < parts; p++) {
    if ((e = hipStreamWaitEvent(s, c->ev_part[p], 0)) != hipSuccess) return (int)e;
    if (p + 1 < parts) {
      rc = launch_ed_tab_mult(Q, p, parts, s);
      if (rc) return rc;
    }
    if (walk_parts) {
      rc = launch_ed_mul_tab(Q, p, parts, s);
      if (rc) return rc;
    }
  }
  if (!walk_parts) {
    rc = launch_ed_mul_tab(Q, 0, 1, s);
    if (rc) return rc;
  }
  rc = launch_ed_fin(Q, s);
  c->fin_done_attached = rc == 0 && Q.fin_done != nullptr && n_lanes != 0;
  return rc;
}

extern "C" {

uint32_t tmx_version(void) { return 0x000100; }

const char* tmx_status_str(int32_t s) {
  switch (s) {
    case TMX_OK: return "ok";
    case TMX_ERR_BAD_ARG: return "bad argument";
    case TMX_ERR_SET_TOO_LARGE: return "validator set larger than VALIDATOR_SET_SIZE_MAX";
    case TMX_ERR_HIP: return "HIP error (no usable MI355X device?)";
    case TMX_ERR_CAPACITY: return "capacity too small";
    case TMX_ERR_PARSE: return "malformed JSON";
    case TMX_ERR_MSG_TOO_LONG: return "sign-bytes longer than 124 bytes";
    case TMX_ERR_RCCL: return "RCCL error";
    default: return "unknown";
  }
}

uint64_t tmx_elem_count(int32_t kind, uint32_t n) {
  if ((kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP) || n == 0 || n > TMX_N_MAX_LIMIT) return 0;
  const uint64_t tn = tree_nodes(n);
  if (kind == TMX_KIND_SKIP) return 1776ull * n + 5320 + 1235ull * n + 630ull * n + 2 * tn * 256 + (4 * 1280 + 88) + 34;
  return 1517ull * n + 6919 + 1235ull * n + tn * 256 + (5 * 1280 + 88) + 25;
}
uint64_t tmx_elem_stride(int32_t kind, uint32_t n) { return (tmx_elem_count(kind, n) + 15) & ~15ull; }  // rows start on a 128-byte line
uint64_t tmx_hint_elem_count(int32_t kind, uint32_t n) {
  if (n == 0 || n > TMX_N_MAX_LIMIT) return 0;
  return kind == TMX_KIND_SKIP ? 1776ull * n + 5320 : 1517ull * n + 6919;
}

const char* tmx_last_error(const tmx_ctx* ctx) { return ctx ? ctx->err.c_str() : (g_tls_err.empty() ? "null context" : g_tls_err.c_str()); }

}  // extern "C"

// One set of streams per device, shared by every context of the process.  The HIP runtime multiplexes streams onto at most four
// hardware queues per priority level, and two streams that land on the same queue lose their concurrency (measured: a step goes
// from 0.86 ms to 1.3-1.7 ms once a fifth stream of a level exists) -- so streams are treated as a scarce per-process resource.
// Sharing is safe: every cross-stream dependency of a batch is an event of its own context; stream order only adds ordering.
namespace {
struct DeviceStreams {
  hipStream_t stream = nullptr, side = nullptr, side2 = nullptr, side3 = nullptr;
  int refs = 0;
};
std::mutex g_streams_mu;
DeviceStreams g_streams[64];

hipError_t acquire_streams(int device, DeviceStreams** out) {
  std::lock_guard<std::mutex> lk(g_streams_mu);
  DeviceStreams& d = g_streams[device];
  if (d.refs == 0) {
    // The key pipeline is on the critical path (high priority); the early serialization only fills otherwise idle HBM cycles and
    // must not starve the caller's stream (low priority).  k_proof's stream is at the caller's priority: the sections that wait for
    // it are the last thing a step writes, and at low priority the kernel stretched from 0.30 ms (alone) to 0.5 ms (measured:
    // normal -2 % step time at 256 proofs, -0.8 % at 1024; high +40 %: two high-priority queues fight).
    int prio_low = 0, prio_high = 0;
    hipError_t e;
    if ((e = hipDeviceGetStreamPriorityRange(&prio_low, &prio_high)) != hipSuccess) return e;
    if ((e = hipStreamCreateWithPriority(&d.side, hipStreamNonBlocking, (prio_low + prio_high) / 2)) != hipSuccess) return e;
    if ((e = hipStreamCreateWithPriority(&d.side2, hipStreamNonBlocking, prio_high)) != hipSuccess) return e;
    if ((e = hipStreamCreateWithPriority(&d.side3, hipStreamNonBlocking, prio_low)) != hipSuccess) return e;
  }
  d.refs++;
  *out = &d;
  return hipSuccess;
}
// The normal-priority stream the host-buffer entry points work on: created on first use, because the device-pointer entry points
// run on the caller's stream and an idle extra stream would still take one of the four normal-priority hardware queues.
hipError_t host_stream(int device, hipStream_t* out) {
  std::lock_guard<std::mutex> lk(g_streams_mu);
  DeviceStreams& d = g_streams[device];
  if (!d.stream) {
    hipError_t e = hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
  }
  *out = d.stream;
  return hipSuccess;
}
void release_streams(int device) {
  std::lock_guard<std::mutex> lk(g_streams_mu);
  DeviceStreams& d = g_streams[device];
  if (d.refs > 0 && --d.refs == 0) {
    if (d.side3) (void)hipStreamDestroy(d.side3);
    if (d.side2) (void)hipStreamDestroy(d.side2);
    if (d.side) (void)hipStreamDestroy(d.side);
    if (d.stream) (void)hipStreamDestroy(d.stream);
    d = DeviceStreams();
  }
}
}  // namespace

// The EdDSA values of a lane that did not sign -- the dummy public key, signature and message of plonky2x (verify.rs:248-259 evaluates every
// such lane on them) -- are the same for every lane of every proof: computed ONCE per context, by the same kernels, on a one-lane launch over
// an all-zero lane record (flags = 0: did not sign); the key cache is emptied again afterwards, so a context starts as it always did.
static int32_t dummy_record(tmx_ctx* c) {
  // (on the context's own side stream, idle at creation: a stream created and destroyed here would shift which hardware queues the
  // streams of the process's NEXT context land on -- second context of a process: 0.63 instead of 0.38 ms per step, tools/churn_probe.py)
  hipStream_t ts = c->side;
  int32_t st = TMX_OK;
  if (use_tiny(c, 1)) st = run_tiny_lanes(c, 1, c->d_dummy_in, c->d_dummy_ed, ED_STRIDE, ts);
  else if (int rc = run_eddsa(c, 1, c->d_dummy_in, c->d_dummy_ed, ED_STRIDE, ts)) st = fail(c, TMX_ERR_HIP, std::string("dummy record: ") + hipGetErrorString((hipError_t)rc));
  hipError_t e = hipStreamSynchronize(ts);
  if (e == hipSuccess) e = hipStreamSynchronize(c->side2);
  if (e == hipSuccess) e = hipStreamSynchronize(c->side);
  if (e == hipSuccess) e = hipStreamSynchronize(c->side3);
  if (st) return st;
  if (e != hipSuccess) return fail(c, TMX_ERR_HIP, std::string("dummy record: ") + hipGetErrorString(e));
  int rc = launch_kc_reset(c->kc, c->side2);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_kc_reset launch: ") + hipGetErrorString((hipError_t)rc));
  HIPCK(c, hipStreamSynchronize(c->side2));
  c->h_hint[0] = 0; c->h_hint[1] = 0;
  c->last_stream_valid = false;
  c->dummy_ready = true;
  return TMX_OK;
}

// (re)allocate the key cache for `keys` slots and empty it.  The caller has made sure nothing of this context is in flight.
// Transactional: the new buffers are allocated and reset first; the old cache is freed only when all of that succeeded, so a failed
// (e.g. oversized) request leaves the context exactly as it was.  A request whose tables cannot fit in the device's free memory is
// refused up front with TMX_ERR_CAPACITY.
static int32_t alloc_key_cache(tmx_ctx* c, uint32_t keys) {
  const size_t lanes = (size_t)c->cfg.max_batch * c->cfg.n_max;
  if (keys > (1u << 20)) keys = 1u << 20;
  if (keys == 0) keys = 1;
  uint64_t hsz = 1;
  while (hsz < 4 * (uint64_t)keys) hsz <<= 1;
  KeyCache kc = c->kc;
  kc.cap = keys;
  kc.hash_mask = (uint32_t)(hsz - 1);
  kc.new_cap = (uint32_t)std::min<size_t>(std::min<size_t>(keys, 4096), lanes);  // tables one launch builds at most: the anchor scratch
  kc.persist = c->knobs.key_cache ? 1u : 0u;
  kc.hint = const_cast<uint32_t*>(c->h_hint);
  kc.d_hash = kc.d_pk = kc.d_used = kc.d_free = kc.d_state = nullptr;
  const size_t sizes[8] = {(size_t)hsz * 4, (size_t)keys * 32, (size_t)keys * 4, (size_t)keys * 4, (size_t)KC_STATE_WORDS * 4,
                           ((size_t)keys + lanes) * key_bytes_per_key(), (size_t)kc.new_cap * anchor_bytes_per_key(), (size_t)keys * keytab_bytes_per_key()};
  {
    size_t want = 0, free_b = 0, total_b = 0;
    for (size_t b : sizes) want += b;
    // (the new cache is allocated before the old one is released, so it has to fit beside it)
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && want > free_b)
      return fail(c, TMX_ERR_CAPACITY, "key cache of " + std::to_string(keys) + " keys needs " + std::to_string(want >> 20) + " MiB, " +
                                           std::to_string(free_b >> 20) + " MiB free on the device");
  }
  void* nb[8] = {};
  hipError_t e = hipSuccess;
  for (int i = 0; i < 8 && e == hipSuccess; i++) e = hipMalloc(&nb[i], sizes[i]);
  if (e == hipSuccess) {
    kc.d_hash = (uint32_t*)nb[0]; kc.d_pk = (uint32_t*)nb[1]; kc.d_used = (uint32_t*)nb[2]; kc.d_free = (uint32_t*)nb[3]; kc.d_state = (uint32_t*)nb[4];
    e = (hipError_t)launch_kc_reset(kc, c->side2);
    if (e == hipSuccess) e = hipStreamSynchronize(c->side2);
  }
  if (e != hipSuccess) {  // the old cache stays in place and usable
    (void)hipGetLastError();
    for (void* b : nb)
      if (b) (void)hipFree(b);
    return fail(c, e == hipErrorOutOfMemory ? TMX_ERR_CAPACITY : TMX_ERR_HIP, std::string("key cache allocation: ") + hipGetErrorString(e));
  }
  void* old[] = {c->kc.d_hash, c->kc.d_pk, c->kc.d_used, c->kc.d_free, c->kc.d_state, c->d_keyrec, c->d_anchors, c->d_keytab};
  for (void* b : old)
    if (b) (void)hipFree(b);
  c->kc = kc;
  c->d_keyrec = nb[5]; c->d_anchors = nb[6]; c->d_keytab = nb[7];
  c->h_hint[0] = 0; c->h_hint[1] = 0;
  return TMX_OK;
}

extern "C" {

void tmx_ctx_destroy(tmx_ctx* c) {
  if (!c) return;
  (void)tmx_comm_destroy(c);
  if (c->have_streams) {  // side streams may still hold work enqueued by the last call (hash-table reset for the next launch)
    (void)hipSetDevice(c->cfg.device);
    (void)hipDeviceSynchronize();
  }
  void* bufs[] = {c->d_lut[0], c->d_lut[1], c->d_wave_sec[0], c->d_wave_sec[1], c->d_seams[0], c->d_seams[1], c->d_table, c->d_qtable, c->d_pre, c->d_mulout, c->d_hash, c->d_cnt, c->d_live, c->d_dummy_ed, c->d_dummy_in, c->setc.table, c->setc.state, c->setc.slots, c->d_span_ctr, c->d_owner_of, c->d_slot_of_owner, c->d_slot_of_uid, c->d_owners, c->d_keyrec,
                  c->d_anchors, c->d_keytab, c->kc.d_hash, c->kc.d_pk, c->kc.d_used, c->kc.d_free, c->kc.d_state, c->d_ed, c->d_tl, c->d_lr, c->d_pf, c->d_nodes_t, c->d_nodes_r,
                  c->d_reports, c->d_in_proofs, c->d_in_targets, c->d_in_trusteds, c->d_out, c->d_pack, c->d_trace_tmp, c->d_tiny, c->d_shadow, c->d_commit,
                  c->d_val_lut[0], c->d_val_lut[1], c->d_value};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  for (void* w : c->d_ntt_w)
    if (w) (void)hipFree(w);
  for (auto& dir : c->d_ntt_m)
    for (void* m : dir)
      if (m) (void)hipFree(m);
  for (void* v : c->d_lde_s)
    if (v) (void)hipFree(v);
  if (c->d_ntt_tmp) (void)hipFree(c->d_ntt_tmp);
  if (c->d_pos_consts) (void)hipFree(c->d_pos_consts);
  for (auto& set : c->ev)
    for (auto& e : set)
      if (e) (void)hipEventDestroy(e);
  for (auto& set : c->ev_side)
    for (auto& e : set)
      if (e) (void)hipEventDestroy(e);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->ev_fork2) (void)hipEventDestroy(c->ev_fork2);
  for (hipEvent_t ev : c->ev_part)
    if (ev) (void)hipEventDestroy(ev);
  if (c->ev_keys) (void)hipEventDestroy(c->ev_keys);
  if (c->ev_direct) (void)hipEventDestroy(c->ev_direct);
  if (c->h_hint) (void)hipHostFree((void*)c->h_hint);
  if (c->ev_hash) (void)hipEventDestroy(c->ev_hash);
  if (c->ev_leaves) (void)hipEventDestroy(c->ev_leaves);
  if (c->ev_hash_clean) (void)hipEventDestroy(c->ev_hash_clean);
  if (c->ev_join3) (void)hipEventDestroy(c->ev_join3);
  if (c->ev_value) (void)hipEventDestroy(c->ev_value);
  if (c->ev_base) (void)hipEventDestroy(c->ev_base);
  for (hipEvent_t e : c->ev_trace_rest)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev_trace)
    if (e) (void)hipEventDestroy(e);
  if (c->ev_tail) (void)hipEventDestroy(c->ev_tail);
  for (hipEvent_t e : c->ev_commit)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev_fri)
    if (e) (void)hipEventDestroy(e);
  if (c->d_fri) (void)hipFree(c->d_fri);
  if (c->d_deepv) (void)hipFree(c->d_deepv);
  if (c->d_set) (void)hipFree(c->d_set);
  if (c->d_set_air) (void)hipFree(c->d_set_air);
  for (auto& of_set : c->d_set_sha)
    for (void* b : of_set)
      if (b) (void)hipFree(b);
  if (c->d_air) (void)hipFree(c->d_air);
  if (c->d_air2) (void)hipFree(c->d_air2);
  if (c->d_air6) (void)hipFree(c->d_air6);
  if (c->d_air7) (void)hipFree(c->d_air7);
  if (c->d_air8) (void)hipFree(c->d_air8);
  if (c->d_air9) (void)hipFree(c->d_air9);
  if (c->d_air10) (void)hipFree(c->d_air10);
  if (c->ev_air) (void)hipEventDestroy(c->ev_air);
  for (auto& sl : c->idx_ring) {
    if (sl.ev) (void)hipEventSynchronize(sl.ev), (void)hipEventDestroy(sl.ev);
    if (sl.d) (void)hipFree(sl.d);
    if (sl.h) (void)hipHostFree(sl.h);
  }
  if (c->have_streams) release_streams(c->cfg.device);
  delete c;
}

int32_t tmx_ctx_create(const tmx_config* cfg, tmx_ctx** out) {
  if (!cfg || !out) return TMX_ERR_BAD_ARG;
  *out = nullptr;
  if (cfg->n_max == 0 || cfg->n_max > TMX_N_MAX_LIMIT || cfg->chain_id_len > 50 || cfg->max_batch == 0) return TMX_ERR_BAD_ARG;
  tmx_ctx* c = new tmx_ctx();
  c->cfg = *cfg;
  *out = c;  // returned even on HIP failure so that tmx_last_error is readable; caller destroys it
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) return fail(c, TMX_ERR_HIP, std::string("no HIP device: ") + hipGetErrorString(e));
  if (cfg->device < 0 || cfg->device >= ndev) return fail(c, TMX_ERR_BAD_ARG, "device ordinal out of range");
  HIPCK(c, hipSetDevice(cfg->device));
  if (cfg->device >= 64) return fail(c, TMX_ERR_BAD_ARG, "device ordinal out of range");
  DeviceStreams* ds = nullptr;
  HIPCK(c, acquire_streams(cfg->device, &ds));
  c->side = ds->side; c->side2 = ds->side2; c->side3 = ds->side3;
  c->have_streams = true;
  HIPCK(c, hipEventCreateWithFlags(&c->ev_join3, hipEventDisableTiming));
  HIPCK(c, hipEventCreateWithFlags(&c->ev_value, hipEventDisableTiming));
  HIPCK(c, hipEventCreateWithFlags(&c->ev_base, hipEventDisableTiming));
  HIPCK(c, hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming));
  HIPCK(c, hipEventCreateWithFlags(&c->ev_fork2, hipEventDisableTiming));
  for (auto& ev : c->ev_part) HIPCK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  c->knobs = read_knobs();
  HIPCK(c, hipEventCreateWithFlags(&c->ev_keys, hipEventDisableTiming));
  HIPCK(c, hipEventCreateWithFlags(&c->ev_direct, hipEventDisableTiming));
  {
    void* hp = nullptr;
    HIPCK(c, hipHostMalloc(&hp, 64, hipHostMallocDefault));
    std::memset(hp, 0, 64);
    c->h_hint = reinterpret_cast<volatile uint32_t*>(hp);
  }
  HIPCK(c, hipEventCreateWithFlags(&c->ev_hash, hipEventDisableTiming));
  HIPCK(c, hipEventCreateWithFlags(&c->ev_leaves, hipEventDisableTiming));
  HIPCK(c, hipEventCreateWithFlags(&c->ev_hash_clean, hipEventDisableTiming));
  HIPCK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  for (auto& set : c->ev_side)
    for (auto& ev : set) HIPCK(c, hipEventCreate(&ev));
  for (auto& set : c->ev)
    for (auto& ev : set) HIPCK(c, hipEventCreate(&ev));
  const uint32_t n = cfg->n_max;
  const size_t B = cfg->max_batch, lanes = B * n;
  if (lanes > ((size_t)1 << 30)) return fail(c, TMX_ERR_CAPACITY, "max_batch * n_max exceeds 2^30 lanes");
  for (int k = 0; k < 2; k++) {
    c->prog[k] = build_program(k, n);
    c->prog[k].sp.lane_fast = c->knobs.ser_lanes ? 1u : 0u;
    if (c->prog[k].sp.elem_count != tmx_elem_count(k, n) || c->prog[k].d1b_start == 0xffffffffu) return fail(c, TMX_ERR_BAD_ARG, "internal: layout size mismatch");
    HIPCK(c, hipMalloc(&c->d_lut[k], c->prog[k].lut.size() * 4));
    HIPCK(c, hipMemcpyAsync(c->d_lut[k], c->prog[k].lut.data(), c->prog[k].lut.size() * 4, hipMemcpyHostToDevice, c->side2));
    HIPCK(c, hipMalloc(&c->d_wave_sec[k], c->prog[k].wave_sec.size()));
    HIPCK(c, hipMemcpyAsync(c->d_wave_sec[k], c->prog[k].wave_sec.data(), c->prog[k].wave_sec.size(), hipMemcpyHostToDevice, c->side2));
    HIPCK(c, hipMalloc(&c->d_seams[k], c->prog[k].seam_waves.size() * 4 + 4));
    HIPCK(c, hipMemcpyAsync(c->d_seams[k], c->prog[k].seam_waves.data(), c->prog[k].seam_waves.size() * 4, hipMemcpyHostToDevice, c->side2));
  }
  HIPCK(c, hipMalloc(&c->d_ed, lanes * ED_STRIDE));
  HIPCK(c, hipMalloc(&c->d_tl, lanes * TL_STRIDE));
  HIPCK(c, hipMalloc(&c->d_lr, lanes * LANE_STRIDE));
  HIPCK(c, hipMalloc(&c->d_pf, B * PF_STRIDE));
  const size_t tn = tree_nodes(n);
  HIPCK(c, hipMalloc(&c->d_nodes_t, B * (tn + 1) * 32));
  HIPCK(c, hipMalloc(&c->d_nodes_r, B * (tn + 1) * 32));
  HIPCK(c, hipMalloc(&c->d_reports, B * sizeof(tmx_report)));
  HIPCK(c, hipMalloc(&c->d_tiny, tiny_counter_words(cfg->max_batch) * 4));
  HIPCK(c, hipMemsetAsync(c->d_tiny, 0, tiny_counter_words(cfg->max_batch) * 4, c->side2));
  HIPCK(c, hipMalloc(&c->d_shadow, (size_t)TINY_MAX_LANES * VR_STRIDE));
  HIPCK(c, hipMemsetAsync(c->d_shadow, 0, (size_t)TINY_MAX_LANES * VR_STRIDE, c->side2));
  // fixed-base table of B (13-bit signed windows: kernels.hip BASE_W), affine form, then the quad layout the kernels read
  HIPCK(c, hipMalloc(&c->d_table, base_table_bytes()));
  int rc = launch_init_base(c->d_table, c->side2);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_init_base launch: ") + hipGetErrorString((hipError_t)rc));
  HIPCK(c, hipMalloc(&c->d_qtable, quad_table_bytes()));
  HIPCK(c, hipMalloc(&c->d_pre, lanes * pre_bytes_per_lane()));
  HIPCK(c, hipMalloc(&c->d_mulout, lanes * mulout_bytes_per_lane()));
  {
    uint64_t cap = 1;
    while (cap < 2 * (uint64_t)lanes) cap <<= 1;  // <= 2^31: the open-addressing table of the launch's own key deduplication
    c->hash_mask = (uint32_t)(cap - 1);
    HIPCK(c, hipMalloc(&c->d_hash, (size_t)cap * 4));
    HIPCK(c, hipMalloc(&c->d_cnt, 64));
    HIPCK(c, hipMalloc(reinterpret_cast<void**>(&c->d_span_ctr), 256));
    HIPCK(c, hipMemsetAsync(c->d_span_ctr, 0, 256, c->side2));
    HIPCK(c, hipMemsetAsync(c->d_hash, 0xff, (size_t)cap * 4, c->side2));
    HIPCK(c, hipMemsetAsync(c->d_cnt, 0, 64, c->side2));
    HIPCK(c, hipMalloc(&c->d_live, lanes * 4));
    if (c->knobs.set_cache) {  // 256 validator sets (20 KB each at N = 128, 82 KB at N = 512), a table of 1024 entries
      SetCache& sc = c->setc;
      // (TMX_SET_CACHE_SETS: a smaller cache for the eviction tests; the table keeps four entries per slot)
      const char* v = std::getenv("TMX_SET_CACHE_SETS");
      const long want = v ? std::atol(v) : 0;
      sc.cap = want >= 4 && want <= (long)SETC_MAX_SLOTS ? (uint32_t)want : SETC_MAX_SLOTS;
      sc.tab_mask = 1023; sc.slot_bytes = (setcache_slot_bytes(n, tree_nodes(n)) + 63u) & ~63u;
      HIPCK(c, hipMalloc(reinterpret_cast<void**>(&sc.table), (sc.tab_mask + 1) * 4));
      HIPCK(c, hipMalloc(reinterpret_cast<void**>(&sc.state), (SETC_STATE_WORDS + SETC_MAX_SLOTS) * 4));
      HIPCK(c, hipMalloc(reinterpret_cast<void**>(&sc.slots), (size_t)sc.cap * sc.slot_bytes));
      HIPCK(c, hipMemsetAsync(sc.table, 0, (sc.tab_mask + 1) * 4, c->side2));
      HIPCK(c, hipMemsetAsync(sc.state, 0, (SETC_STATE_WORDS + SETC_MAX_SLOTS) * 4, c->side2));
    }
    HIPCK(c, hipMalloc(&c->d_dummy_ed, 512));
    HIPCK(c, hipMalloc(&c->d_dummy_in, VR_STRIDE));
    HIPCK(c, hipMemsetAsync(c->d_dummy_ed, 0, 512, c->side2));
    HIPCK(c, hipMemsetAsync(c->d_dummy_in, 0, VR_STRIDE, c->side2));
    HIPCK(c, hipMalloc(&c->d_owner_of, lanes * 4));
    HIPCK(c, hipMalloc(&c->d_slot_of_owner, lanes * 4));
    HIPCK(c, hipMalloc(&c->d_slot_of_uid, lanes * 4));
    HIPCK(c, hipMalloc(&c->d_owners, lanes * 4));
  }
  // key cache: by default room for the keys of 4 x max_batch x n_max lanes at 8 lanes per key, between 1024 and 8192 keys (655 KB each:
  // 0.7 - 5.4 GB of the 288 GB); TMX_KEY_CACHE_KEYS / tmx_key_cache_resize choose another capacity
  {
    size_t keys = c->knobs.key_cache_keys ? c->knobs.key_cache_keys : std::min<size_t>(8192, std::max<size_t>(1024, lanes / 2));
    // TMX_KEY_CACHE=0: a table lives for one launch only, so the slots one launch can build (<= 4096, <= lanes) are all it ever uses
    if (!c->knobs.key_cache && !c->knobs.key_cache_keys) keys = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(4096, lanes), keys));
    int32_t st = alloc_key_cache(c, (uint32_t)keys);
    if (st) return st;
  }
  rc = launch_init_base_quad(c->d_table, c->d_qtable, c->side2);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_init_base_quad launch: ") + hipGetErrorString((hipError_t)rc));
  HIPCK(c, hipEventRecord(c->ev_hash_clean, c->side2));
  HIPCK(c, hipStreamSynchronize(c->side2));
  return dummy_record(c);
}

static int32_t ensure_host_stream(tmx_ctx* c) {
  if (c->stream) return TMX_OK;
  HIPCK(c, hipSetDevice(c->cfg.device));
  HIPCK(c, host_stream(c->cfg.device, &c->stream));
  return TMX_OK;
}
void* tmx_ctx_stream(tmx_ctx* c) { return c && ensure_host_stream(c) == TMX_OK ? reinterpret_cast<void*>(c->stream) : nullptr; }

// Nothing of this context may be in flight when the cache is reshaped: wait for the last batch and the side streams' tails.
static int32_t quiesce(tmx_ctx* c) {
  HIPCK(c, hipSetDevice(c->cfg.device));
  if (c->last_stream_valid) HIPCK(c, hipEventSynchronize(c->ev_done));
  HIPCK(c, hipStreamSynchronize(c->side2));
  HIPCK(c, hipStreamSynchronize(c->side));
  HIPCK(c, hipStreamSynchronize(c->side3));
  if (c->stream) HIPCK(c, hipStreamSynchronize(c->stream));
  return TMX_OK;
}
static int32_t read_kc_state(tmx_ctx* c, uint32_t st[KC_STATE_WORDS]) {
  int32_t q = quiesce(c);
  if (q) return q;
  HIPCK(c, hipMemcpy(st, c->kc.d_state, KC_STATE_WORDS * 4, hipMemcpyDeviceToHost));
  return TMX_OK;
}

// distinct effective public keys among the lanes of the last EdDSA launch (resident ones that were hit + new ones) and whether any lane
// walked a per-key table (blocks until that launch is done)
int32_t tmx_last_dedup(tmx_ctx* c, uint32_t* n_unique, uint32_t* used_tables) {
  if (!c || !n_unique || !used_tables) return TMX_ERR_BAD_ARG;
  *n_unique = 0; *used_tables = 0;
  if (c->last_lanes == 0) return TMX_OK;
  uint32_t st[KC_STATE_WORDS];
  int32_t r = read_kc_state(c, st);
  if (r) return r;
  *n_unique = st[KC_LAST_NEW] + st[KC_LAST_HIT_KEYS];
  *used_tables = (c->knobs.dedup_mode != 0 && (st[KC_LAST_HIT_LANES] != 0 || (st[KC_LAST_BUILT] != 0 && st[KC_LAST_USE_NEW] != 0))) ? 1u : 0u;
  return TMX_OK;
}

int32_t tmx_last_proof_path(tmx_ctx* c) { return c ? c->last_proof_path : TMX_ERR_BAD_ARG; }

int32_t tmx_key_cache_stats(tmx_ctx* c, tmx_key_cache_info* out) {
  if (!c || !out) return TMX_ERR_BAD_ARG;
  uint32_t st[KC_STATE_WORDS];
  int32_t r = read_kc_state(c, st);
  if (r) return r;
  uint64_t tot[8];
  std::memcpy(tot, st + KC_TOTALS, sizeof(uint64_t) * 6);
  std::memset(out, 0, sizeof *out);
  out->capacity_keys = c->kc.cap; out->resident_keys = st[KC_RESIDENT]; out->enabled = c->kc.persist; out->epoch = st[KC_EPOCH];
  out->bytes_per_key = keytab_bytes_per_key() + key_bytes_per_key() + 32;
  out->last_new_keys = st[KC_LAST_NEW]; out->last_hit_keys = st[KC_LAST_HIT_KEYS]; out->last_hit_lanes = st[KC_LAST_HIT_LANES];
  out->last_built_keys = st[KC_LAST_BUILT];
  out->hit_lanes = tot[KC_TOT_HIT_LANES]; out->miss_lanes = tot[KC_TOT_MISS_LANES]; out->built_keys = tot[KC_TOT_BUILT];
  out->evicted_keys = tot[KC_TOT_EVICTED]; out->evictions = tot[KC_TOT_GC_RUNS]; out->launches = tot[KC_TOT_LAUNCHES];
  return TMX_OK;
}

int32_t tmx_key_cache_flush(tmx_ctx* c) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t q = quiesce(c);
  if (q) return q;
  int rc = launch_kc_reset(c->kc, c->side2);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_kc_reset launch: ") + hipGetErrorString((hipError_t)rc));
  if (c->setc.table) {  // (the validator-set cache goes with it: "flush" = a context as new)
    HIPCK(c, hipMemsetAsync(c->setc.table, 0, (c->setc.tab_mask + 1) * 4, c->side2));
    HIPCK(c, hipMemsetAsync(c->setc.state, 0, (SETC_STATE_WORDS + SETC_MAX_SLOTS) * 4, c->side2));
  }
  HIPCK(c, hipStreamSynchronize(c->side2));
  c->h_hint[0] = 0; c->h_hint[1] = 0;  // an empty cache: the next enqueue takes the cold schedule, as the first call of a context does
  return TMX_OK;
}

int32_t tmx_set_cache_stats(tmx_ctx* c, uint32_t out[8]) {
  if (!c || !out) return TMX_ERR_BAD_ARG;
  std::memset(out, 0, 8 * sizeof(uint32_t));
  if (!c->setc.table) return TMX_OK;
  int32_t q = quiesce(c);
  if (q) return q;
  uint32_t st[SETC_STATE_WORDS];
  HIPCK(c, hipMemcpy(st, c->setc.state, sizeof st, hipMemcpyDeviceToHost));
  const uint32_t hi = st[0] > c->setc.cap ? c->setc.cap : st[0], fr = (int32_t)st[4] > 0 ? st[4] : 0u;
  out[0] = hi - (fr > hi ? hi : fr);  // resident = slots ever used - slots on the free list
  out[1] = st[1]; out[2] = st[2]; out[3] = st[3]; out[4] = st[6]; out[5] = c->setc.cap;
  return TMX_OK;
}

int32_t tmx_key_cache_config(tmx_ctx* c, uint32_t enabled, uint32_t max_keys) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t q = quiesce(c);
  if (q) return q;
  const bool was = c->knobs.key_cache;
  c->knobs.key_cache = enabled != 0;
  if (max_keys != 0 && max_keys != c->kc.cap) {
    int32_t st = alloc_key_cache(c, max_keys);  // (on failure the old cache, and the old setting, stay)
    if (st) { c->knobs.key_cache = was; return st; }
  } else if (was && !enabled) {
    // persistence switched off: every launch starts from an empty cache, so the resident keys go now (a full cache would otherwise
    // leave the launches without free slots, i.e. without per-launch tables)
    int rc = launch_kc_reset(c->kc, c->side2);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_kc_reset launch: ") + hipGetErrorString((hipError_t)rc));
    HIPCK(c, hipStreamSynchronize(c->side2));
    c->h_hint[0] = 0; c->h_hint[1] = 0;
  }
  c->kc.persist = enabled ? 1u : 0u;
  return TMX_OK;
}

int32_t tmx_sync(tmx_ctx* c) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (c->stream) HIPCK(c, hipStreamSynchronize(c->stream));  // (the host-buffer entry points already synchronise before returning)
  return TMX_OK;
}

int32_t tmx_witness_batch_device(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets,
                                 const void* d_trusteds, void* d_out_elems, void* d_reports, void* hip_stream) {
  int32_t st = check_batch_args(c, kind, n_proofs, d_proofs, d_targets, d_trusteds);
  if (st) return st;
  if (n_proofs == 0) return TMX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);  // NULL = the HIP default stream, exactly as passed
  if (use_tiny(c, (uint64_t)n_proofs * c->cfg.n_max)) return run_tiny(c, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_out_elems, d_reports, s);
  return run_batch(c, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_out_elems, d_reports, s, true, [&](hipStream_t ss) -> int32_t {
    int rc = run_eddsa(c, n_proofs * c->cfg.n_max, d_targets, reinterpret_cast<uint8_t*>(c->d_tl) + TL_OFF_ED, TL_STRIDE, ss);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("EdDSA kernel launch: ") + hipGetErrorString((hipError_t)rc));
    return TMX_OK;
  });
}

int32_t tmx_eddsa_lanes_device(tmx_ctx* c, uint32_t n_lanes, const void* d_lanes, void* d_ed_out, void* hip_stream) {
  if (!c || !d_lanes || !d_ed_out) return TMX_ERR_BAD_ARG;
  if (n_lanes == 0) return TMX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  if ((uint64_t)n_lanes > (uint64_t)c->cfg.max_batch * c->cfg.n_max) return fail(c, TMX_ERR_CAPACITY, "n_lanes exceeds max_batch * n_max");
  if (use_tiny(c, n_lanes)) return run_tiny_lanes(c, n_lanes, d_lanes, d_ed_out, ED_STRIDE, s);
  int rc = run_eddsa(c, n_lanes, d_lanes, d_ed_out, ED_STRIDE, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("EdDSA kernel launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

int32_t tmx_finish_batch_device(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets,
                                const void* d_trusteds, const void* d_ed, void* d_out_elems, void* d_reports, void* hip_stream) {
  int32_t st = check_batch_args(c, kind, n_proofs, d_proofs, d_targets, d_trusteds);
  if (st) return st;
  if (!d_ed) return TMX_ERR_BAD_ARG;
  if (n_proofs == 0) return TMX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  return run_batch(c, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_out_elems, d_reports, s, false, [&](hipStream_t ss) -> int32_t {
    // caller's records are 448 B apart; place them into the ED part of the unified per-lane records
    HIPCK(c, hipMemcpy2DAsync(reinterpret_cast<uint8_t*>(c->d_tl) + TL_OFF_ED, TL_STRIDE, d_ed, ED_STRIDE, ED_STRIDE,
                              (size_t)n_proofs * c->cfg.n_max, hipMemcpyDeviceToDevice, ss));
    return TMX_OK;
  });
}

uint64_t tmx_trace_elem_count(int32_t kind, uint32_t n) {
  if ((kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP) || n == 0 || n > TMX_N_MAX_LIMIT) return 0;
  return trace_elems((uint32_t)kind, n);
}

}  // extern "C"
// lane0 / lane_count: the ladder and SHA-512 rows (the per-lane sections) of lanes [lane0, lane0 + lane_count) of the batch only -- the
// lane-sharded form; the other sections are written for every proof either way
static int32_t trace_rows_impl(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_targets, const void* d_trusteds, void* d_trace_out,
                               uint32_t sections, void* hip_stream, uint32_t lane0, uint32_t lane_count) {
  if (!c || (kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP) || !d_targets || !d_trace_out || (sections & ~(uint32_t)TMX_TRACE_ALL) || sections == 0)
    return TMX_ERR_BAD_ARG;
  if (kind == TMX_KIND_SKIP && !d_trusteds) return fail(c, TMX_ERR_BAD_ARG, "skip needs the trusted hash fields");
  if (n_proofs > c->cfg.max_batch) return fail(c, TMX_ERR_CAPACITY, "n_proofs exceeds the context's max_batch");
  if (n_proofs == 0) return TMX_OK;
  // the trace kernels read the Level-1 lane records of the context: they must be those of a batch of this kind and at least this size
  if (c->last_kind != kind || c->last_n_proofs < n_proofs)
    return fail(c, TMX_ERR_BAD_ARG, "tmx_trace_rows_device: call tmx_witness_batch_device for the same batch (kind, >= n_proofs) first");
  if ((sections & TMX_TRACE_LADDERS) && !c->d_trace_tmp) {  // 82 KB per ladder between the two ladder passes: allocated (blocking) on the first call
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipMalloc(&c->d_trace_tmp, trace_tmp_bytes(c->cfg.n_max, c->cfg.max_batch)));
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  const uint8_t* edr = reinterpret_cast<const uint8_t*>(c->d_tl) + TL_OFF_ED;
  const uint32_t n = c->cfg.n_max;
  int rc = 0;
  // The other sections (0.6 ms of short, memory-bound kernels per 256-proof batch) beside the ladders, whose first segment is one
  // latency-bound wave per SIMD with nothing else on the chip: on the low-priority side stream, joined at the end (all sections 5.6 -> 5.3 ms)
  const bool rest_aside = (sections & TMX_TRACE_LADDERS) && (sections & ~(uint32_t)TMX_TRACE_LADDERS);
  if (rest_aside) {
    for (auto& e : c->ev_trace_rest)
      if (!e) HIPCK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPCK(c, hipEventRecord(c->ev_trace_rest[0], s));
    HIPCK(c, hipStreamWaitEvent(c->side3, c->ev_trace_rest[0], 0));
    const TraceLevel1 L1 = {reinterpret_cast<const uint8_t*>(c->d_tl) + TL_OFF_LT, c->d_lr, c->d_nodes_t, c->d_nodes_r, c->d_pf, TL_STRIDE};
    rc = launch_trace_rest((uint32_t)kind, n, n_proofs, d_targets, d_trusteds, L1, d_trace_out, sections, c->side3, lane0, lane_count);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_trace launch: ") + hipGetErrorString((hipError_t)rc));
    HIPCK(c, hipEventRecord(c->ev_trace_rest[1], c->side3));
  }
  if (sections & TMX_TRACE_LADDERS) {
    // The chain (pass 1: 1024 latency-bound waves per 256 proofs) in segments on the caller's stream; the affine rows of a segment (pass 2)
    // follow on the side stream while the next segment is being doubled.  Measured per 256-proof batch at N = 128 (round 4 kernels): two
    // segments of 128 rows 4.95 ms, four 5.4, eight 6.7; both passes one after the other on one stream 6.4.  TMX_TRACE_SEGS overrides.
    static const uint32_t segs_env = std::getenv("TMX_TRACE_SEGS") ? (uint32_t)std::atoi(std::getenv("TMX_TRACE_SEGS")) : 2u;
    const uint32_t segs = (segs_env == 1 || segs_env == 4 || segs_env == 8 || segs_env == 16) ? segs_env : 2u;
    for (auto& e : c->ev_trace)
      if (!e) HIPCK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (uint32_t g = 0; g < segs && !rc; g++) {
      const uint32_t r0 = TR_LADDER_ROWS * g / segs, r1 = TR_LADDER_ROWS * (g + 1) / segs;
      rc = launch_trace_ladder_pass1(n, n_proofs, d_targets, edr, TL_STRIDE, c->d_trace_tmp, r0, r1, s, lane0, lane_count);
      if (rc) break;
      hipStream_t p2 = c->side;
      {
        HIPCK(c, hipEventRecord(c->ev_trace[g], s));
        HIPCK(c, hipStreamWaitEvent(p2, c->ev_trace[g], 0));
      }
      rc = launch_trace_ladder_pass2((uint32_t)kind, n, n_proofs, d_targets, edr, TL_STRIDE, c->d_trace_tmp, d_trace_out, r0, r1, p2, lane0, lane_count);
    }
    if (!rc) {
      HIPCK(c, hipEventRecord(c->ev_trace[16], c->side));
    }
  }
  if (!rc && rest_aside) HIPCK(c, hipStreamWaitEvent(s, c->ev_trace_rest[1], 0));
  if (!rc && (sections & ~(uint32_t)TMX_TRACE_LADDERS) && !rest_aside) {
    const TraceLevel1 L1 = {reinterpret_cast<const uint8_t*>(c->d_tl) + TL_OFF_LT, c->d_lr, c->d_nodes_t, c->d_nodes_r, c->d_pf, TL_STRIDE};
    rc = launch_trace_rest((uint32_t)kind, n, n_proofs, d_targets, d_trusteds, L1, d_trace_out, sections, s, lane0, lane_count);
  }
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_trace launch: ") + hipGetErrorString((hipError_t)rc));
  if ((sections & TMX_TRACE_LADDERS) && c->ev_trace[16]) HIPCK(c, hipStreamWaitEvent(s, c->ev_trace[16], 0));  // the call ends on the caller's stream
  return TMX_OK;
}
extern "C" {
int32_t tmx_trace_rows_device(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_targets, const void* d_trusteds, void* d_trace_out,
                              uint32_t sections, void* hip_stream) {
  return trace_rows_impl(c, kind, n_proofs, d_targets, d_trusteds, d_trace_out, sections, hip_stream, 0, 0xffffffffu);
}

int32_t tmx_kernel_ms_mean(tmx_ctx* c, uint32_t last_k, float ms[TMX_N_KERNELS]) {
  if (!c || !ms || last_k == 0) return TMX_ERR_BAD_ARG;
  if (c->n_calls == 0) return fail(c, TMX_ERR_BAD_ARG, "no batch has been enqueued yet");
  if (last_k > tmx_ctx::EV_RING) last_k = tmx_ctx::EV_RING;
  if (last_k > c->n_calls) last_k = (uint32_t)c->n_calls;
  double acc[TMX_N_KERNELS] = {0};
  for (uint32_t j = 0; j < last_k; j++) {
    hipEvent_t* ev = c->ev[(c->n_calls - 1 - j) % tmx_ctx::EV_RING];
    HIPCK(c, hipEventSynchronize(ev[3]));
    if (c->slot_tiny[(c->n_calls - 1 - j) % tmx_ctx::EV_RING]) {
      // a small launch: ev[0] .. ev[1] = k_tiny (the EdDSA lanes and the proof roles side by side: attributed ONCE, to the EdDSA slot),
      // ev[1] .. ev[2] = the gap between the two launches (the serializer slot), ev[2] .. ev[3] = k_tiny_tail (the verdict slot) -- the four
      // figures are disjoint intervals, so their sum is the small launch's length as it is for a classic one
      float t = 0;
      HIPCK(c, hipEventElapsedTime(&t, ev[0], ev[1])); acc[TMX_K_EDDSA] += t;
      HIPCK(c, hipEventElapsedTime(&t, ev[2], ev[3])); acc[TMX_K_VERDICT] += t;
      HIPCK(c, hipEventElapsedTime(&t, ev[1], ev[2])); acc[TMX_K_SERIALIZE] += t;
      continue;
    }
    hipEvent_t* evs = c->ev_side[(c->n_calls - 1 - j) % tmx_ctx::EV_RING];
    HIPCK(c, hipEventSynchronize(evs[1]));
    float t = 0;
    HIPCK(c, hipEventElapsedTime(&t, ev[0], ev[1])); acc[TMX_K_EDDSA] += t;
    HIPCK(c, hipEventElapsedTime(&t, evs[0], evs[1])); acc[TMX_K_PROOF] += t;
    HIPCK(c, hipEventElapsedTime(&t, evs[2], evs[3])); acc[TMX_K_VERDICT] += t;
    HIPCK(c, hipEventElapsedTime(&t, c->knobs.ser_split ? ev[1] : ev[2], ev[3])); acc[TMX_K_SERIALIZE] += t;
  }
  for (int k = 0; k < TMX_N_KERNELS; k++) ms[k] = (float)(acc[k] / last_k);
  return TMX_OK;
}
int32_t tmx_last_kernel_ms(tmx_ctx* c, float ms[TMX_N_KERNELS]) { return tmx_kernel_ms_mean(c, 1, ms); }

static int32_t ensure_staging_inputs(tmx_ctx* c) {
  int32_t hs = ensure_host_stream(c);
  if (hs) return hs;
  if (c->d_in_proofs) return TMX_OK;
  HIPCK(c, hipSetDevice(c->cfg.device));
  const size_t B = c->cfg.max_batch, lanes = B * c->cfg.n_max;
  HIPCK(c, hipMalloc(&c->d_in_proofs, B * sizeof(tmx_proof_rec)));
  HIPCK(c, hipMalloc(&c->d_in_targets, lanes * sizeof(tmx_validator_rec)));
  HIPCK(c, hipMalloc(&c->d_in_trusteds, lanes * sizeof(tmx_hashfield_rec)));
  return TMX_OK;
}
static int32_t ensure_staging(tmx_ctx* c) {  // + the row buffer of the element-producing host entry points (the typed-value calls never need it)
  int32_t st = ensure_staging_inputs(c);
  if (st) return st;
  if (c->d_out) return TMX_OK;
  const size_t B = c->cfg.max_batch;
  uint64_t stride = tmx_elem_stride(TMX_KIND_SKIP, c->cfg.n_max), st2 = tmx_elem_stride(TMX_KIND_STEP, c->cfg.n_max);
  c->d_out_elems = (stride > st2 ? stride : st2) * B;
  HIPCK(c, hipMalloc(&c->d_out, c->d_out_elems * 8));
  return TMX_OK;
}

// Host-buffer path shared by tmx_witness_batch (full rows of tmx_elem_stride u64) and tmx_witness_batch_opts (dense rows of the selected
// sections, u64 or u32): H2D of the records, the batch on the context's stream, D2H of what the caller asked for.
static int32_t witness_batch_host(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const tmx_proof_rec* proofs, const tmx_validator_rec* targets,
                                  const tmx_hashfield_rec* trusteds, bool opts, uint32_t sections, uint32_t format, void* out, uint64_t cap_bytes,
                                  tmx_report* reports) {
  if (!c || !proofs || !targets || (kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP)) return TMX_ERR_BAD_ARG;
  if (kind == TMX_KIND_SKIP && !trusteds) return fail(c, TMX_ERR_BAD_ARG, "skip needs the trusted hash fields");
  if (opts && ((sections & ~(uint32_t)TMX_SEC_ALL) || sections == 0 || (format != TMX_OUT_U64 && format != TMX_OUT_U32)))
    return fail(c, TMX_ERR_BAD_ARG, "sections must be a non-empty subset of TMX_SEC_ALL and format TMX_OUT_U64 or TMX_OUT_U32");
  if (n_proofs == 0) return TMX_OK;
  if (n_proofs > c->cfg.max_batch) return fail(c, TMX_ERR_CAPACITY, "n_proofs exceeds the context's max_batch");
  const uint32_t n = c->cfg.n_max;
  const uint64_t stride = tmx_elem_stride(kind, n), count = tmx_elem_count(kind, n), hint = tmx_hint_elem_count(kind, n);
  const uint64_t first = opts && sections == TMX_SEC_DERIVED ? hint : 0;
  const uint64_t row_elems = opts ? tmx_out_row_elems(kind, n, sections) : count;
  const uint64_t esz = opts && format == TMX_OUT_U32 ? 4 : 8;
  if (out && opts && cap_bytes < (uint64_t)n_proofs * row_elems * esz) return fail(c, TMX_ERR_CAPACITY, "out buffer too small");
  if (out && !opts && cap_bytes < ((uint64_t)(n_proofs - 1) * stride + count) * 8) return fail(c, TMX_ERR_CAPACITY, "out_elems too small");
  for (uint32_t p = 0; p < n_proofs; p++)  // reference input/mod.rs:439-444, 338-342
    if (proofs[p].nb_a > n || (kind == TMX_KIND_SKIP && proofs[p].nb_b > n)) return fail(c, TMX_ERR_SET_TOO_LARGE, "validator set larger than VALIDATOR_SET_SIZE_MAX");
  int32_t st = ensure_staging(c);
  if (st) return st;
  const size_t lanes = (size_t)n_proofs * n;
  HIPCK(c, hipMemcpyAsync(c->d_in_proofs, proofs, (size_t)n_proofs * sizeof(tmx_proof_rec), hipMemcpyHostToDevice, c->stream));
  HIPCK(c, hipMemcpyAsync(c->d_in_targets, targets, lanes * sizeof(tmx_validator_rec), hipMemcpyHostToDevice, c->stream));
  if (kind == TMX_KIND_SKIP)
    HIPCK(c, hipMemcpyAsync(c->d_in_trusteds, trusteds, lanes * sizeof(tmx_hashfield_rec), hipMemcpyHostToDevice, c->stream));
  c->sections = opts ? sections : (uint32_t)TMX_SEC_ALL;
  st = tmx_witness_batch_device(c, kind, n_proofs, c->d_in_proofs, c->d_in_targets, kind == TMX_KIND_SKIP ? c->d_in_trusteds : nullptr,
                                out ? c->d_out : nullptr, c->d_reports, c->stream);
  c->sections = TMX_SEC_ALL;
  if (st) return st;
  if (out && !opts) {
    // rows are stride apart on the device; the last row is copied without its pad element
    const size_t bytes = ((size_t)(n_proofs - 1) * stride + count) * 8;
    HIPCK(c, hipMemcpyAsync(out, c->d_out, bytes, hipMemcpyDeviceToHost, c->stream));
  } else if (out) {
    const size_t bytes = (size_t)n_proofs * row_elems * esz;
    const void* src = c->d_out;
    if (!(first == 0 && row_elems == stride && esz == 8)) {  // dense rows of the selection, u64 or narrowed to u32, then ONE contiguous copy
      if (c->d_pack_bytes < bytes) {
        if (c->d_pack) { HIPCK(c, hipStreamSynchronize(c->stream)); HIPCK(c, hipFree(c->d_pack)); c->d_pack = nullptr; c->d_pack_bytes = 0; }
        const size_t want = (size_t)c->cfg.max_batch * (size_t)(tmx_elem_count(TMX_KIND_SKIP, n) > tmx_elem_count(TMX_KIND_STEP, n) ? tmx_elem_count(TMX_KIND_SKIP, n) : tmx_elem_count(TMX_KIND_STEP, n)) * 8;
        HIPCK(c, hipMalloc(&c->d_pack, want));
        c->d_pack_bytes = want;
      }
      int rc = launch_pack_rows(c->d_out, c->d_pack, (uint32_t)stride, (uint32_t)first, (uint32_t)row_elems, n_proofs, esz == 4, c->stream);
      if (rc) return fail(c, TMX_ERR_HIP, std::string("k_pack_rows launch: ") + hipGetErrorString((hipError_t)rc));
      src = c->d_pack;
    }
    HIPCK(c, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->stream));
  }
  if (reports) HIPCK(c, hipMemcpyAsync(reports, c->d_reports, (size_t)n_proofs * sizeof(tmx_report), hipMemcpyDeviceToHost, c->stream));
  HIPCK(c, hipStreamSynchronize(c->stream));
  return TMX_OK;
}

int32_t tmx_witness_batch(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const tmx_proof_rec* proofs, const tmx_validator_rec* targets,
                          const tmx_hashfield_rec* trusteds, uint64_t* out_elems, uint64_t cap_elems, tmx_report* reports) {
  return witness_batch_host(c, kind, n_proofs, proofs, targets, trusteds, false, TMX_SEC_ALL, TMX_OUT_U64, out_elems, cap_elems * 8, reports);
}

int32_t tmx_witness_batch_opts(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const tmx_proof_rec* proofs, const tmx_validator_rec* targets,
                               const tmx_hashfield_rec* trusteds, uint32_t sections, uint32_t format, void* out, uint64_t cap_bytes,
                               tmx_report* reports) {
  return witness_batch_host(c, kind, n_proofs, proofs, targets, trusteds, true, sections, format, out, cap_bytes, reports);
}

uint64_t tmx_out_row_elems(int32_t kind, uint32_t n, uint32_t sections) {
  const uint64_t count = tmx_elem_count(kind, n), hint = tmx_hint_elem_count(kind, n);
  if (count == 0) return 0;
  return (sections & TMX_SEC_ALL) == TMX_SEC_ALL ? count : (sections & TMX_SEC_HINT) ? hint : (sections & TMX_SEC_DERIVED) ? count - hint : 0;
}

int32_t tmx_witness_batch_device_sections(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets,
                                          const void* d_trusteds, void* d_out_elems, void* d_reports, void* hip_stream, uint32_t sections) {
  if (!c || (sections & ~(uint32_t)TMX_SEC_ALL) || sections == 0) return TMX_ERR_BAD_ARG;
  c->sections = sections;
  const int32_t st = tmx_witness_batch_device(c, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_out_elems, d_reports, hip_stream);
  c->sections = TMX_SEC_ALL;
  return st;
}

int32_t tmx_skip_witness(tmx_ctx* c, const tmx_proof_rec* proof, const tmx_validator_rec* target, const tmx_hashfield_rec* trusted,
                         uint64_t* out_elems, uint64_t cap_elems, tmx_report* report) {
  return tmx_witness_batch(c, TMX_KIND_SKIP, 1, proof, target, trusted, out_elems, cap_elems, report);
}
int32_t tmx_step_witness(tmx_ctx* c, const tmx_proof_rec* proof, const tmx_validator_rec* target, uint64_t* out_elems, uint64_t cap_elems,
                         tmx_report* report) {
  return tmx_witness_batch(c, TMX_KIND_STEP, 1, proof, target, nullptr, out_elems, cap_elems, report);
}

}  // extern "C"

// ---- the typed value of the hint (include/tmx.h "TYPED VALUE"; value.h / value.hip) ----------------------------------------------------
static ValueLayout value_layout_for(int32_t kind, uint32_t n, uint32_t sections) { return value_layout((uint32_t)kind, n, tree_nodes(n), sections); }

// fixed-part gather table of one kind, straight from the public structs' offsetof: whatever include/tmx.h declares is what the device writes
static std::vector<uint16_t> value_fixed_lut(int32_t kind) {
  std::vector<uint16_t> lut(VAL_FIXED_MAX, VAL_LUT_ZERO);
  auto put = [&](size_t dst, size_t len, uint32_t src, uint32_t off) {
    for (size_t i = 0; i < len; i++) lut[dst + i] = (uint16_t)((src << 12) | (off + (uint32_t)i));
  };
  auto chain_id_proof = [&](size_t at) {
    put(at + offsetof(tmx_chain_id_proof_value, proof), 128, VSRC_PF, PF_OFF_AUNTS + 128 * 0);
    put(at + offsetof(tmx_chain_id_proof_value, enc_chain_id_byte_length), 4, VSRC_PF, PF_OFF_CIDLEN);
    put(at + offsetof(tmx_chain_id_proof_value, chain_id), 52, VSRC_PF, PF_OFF_CID52);
  };
  auto height_proof = [&](size_t at) {
    put(at + offsetof(tmx_height_proof_value, proof), 128, VSRC_PF, PF_OFF_AUNTS + 128 * 1);
    put(at + offsetof(tmx_height_proof_value, enc_height_byte_length), 4, VSRC_PF, PF_OFF_HLEN);
    put(at + offsetof(tmx_height_proof_value, height), 8, VSRC_PF, PF_OFF_HEIGHT);
  };
  auto hash_proof = [&](size_t at, int q, uint32_t leaf_off) {
    put(at + offsetof(tmx_hash_inclusion_proof_value, proof), 128, VSRC_PF, PF_OFF_AUNTS + 128 * (uint32_t)q);
    put(at + offsetof(tmx_hash_inclusion_proof_value, leaf), 34, VSRC_PF, leaf_off);
  };
  if (kind == TMX_KIND_SKIP) {
    put(offsetof(tmx_skip_inputs_fixed, target_header), 32, VSRC_PF, PF_OFF_HEADER);
    put(offsetof(tmx_skip_inputs_fixed, trusted_header), 32, VSRC_PROOF, PR_OFF_HASH);
    put(offsetof(tmx_skip_inputs_fixed, round), 8, VSRC_PROOF, PR_OFF_ROUND);
    put(offsetof(tmx_skip_inputs_fixed, nb_target_validators), 4, VSRC_PROOF, PR_OFF_NB_A);
    put(offsetof(tmx_skip_inputs_fixed, nb_trusted_validators), 4, VSRC_PROOF, PR_OFF_NB_B);
    chain_id_proof(offsetof(tmx_skip_inputs_fixed, target_block_chain_id_proof));
    height_proof(offsetof(tmx_skip_inputs_fixed, target_block_height_proof));
    hash_proof(offsetof(tmx_skip_inputs_fixed, target_block_validators_hash_proof), 2, PF_OFF_LEAFV);
    hash_proof(offsetof(tmx_skip_inputs_fixed, trusted_block_validators_hash_proof), 3, PF_OFF_LEAFX);
    put(offsetof(tmx_skip_inputs_fixed, report), sizeof(tmx_report), VSRC_REPORT, 0);
  } else {
    put(offsetof(tmx_step_inputs_fixed, next_header), 32, VSRC_PF, PF_OFF_HEADER);
    put(offsetof(tmx_step_inputs_fixed, round), 8, VSRC_PROOF, PR_OFF_ROUND);
    put(offsetof(tmx_step_inputs_fixed, nb_validators), 4, VSRC_PROOF, PR_OFF_NB_A);
    chain_id_proof(offsetof(tmx_step_inputs_fixed, next_block_chain_id_proof));
    height_proof(offsetof(tmx_step_inputs_fixed, next_block_height_proof));
    hash_proof(offsetof(tmx_step_inputs_fixed, next_block_validators_hash_proof), 2, PF_OFF_LEAFV);
    const size_t lb = offsetof(tmx_step_inputs_fixed, next_block_last_block_id_proof);
    put(lb + offsetof(tmx_block_id_inclusion_proof_value, proof), 128, VSRC_PF, PF_OFF_AUNTS + 128 * 3);
    put(lb + offsetof(tmx_block_id_inclusion_proof_value, leaf), 72, VSRC_PF, PF_OFF_LEAFX);
    hash_proof(offsetof(tmx_step_inputs_fixed, prev_block_next_validators_hash_proof), 4, PF_OFF_LEAFY);
    put(offsetof(tmx_step_inputs_fixed, report), sizeof(tmx_report), VSRC_REPORT, 0);
  }
  return lut;
}

extern "C" {

int32_t tmx_value_layout_of(int32_t kind, uint32_t n, uint32_t sections, tmx_value_layout* out) {
  if (!out || (kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP) || n == 0 || n > TMX_N_MAX_LIMIT || (sections != TMX_SEC_HINT && sections != TMX_SEC_ALL))
    return TMX_ERR_BAD_ARG;
  const ValueLayout L = value_layout_for(kind, n, sections);
  std::memset(out, 0, sizeof *out);
  auto at = [&](uint32_t p) { return L.off[p + 1] > L.off[p] ? L.off[p] : 0u; };
  out->bytes = L.off[VP_COUNT];
  out->fixed_bytes = L.off[VP_FIXED + 1] - L.off[VP_FIXED];
  out->off_validators = at(VP_VALIDATORS); out->off_hashfields = at(VP_HASHFIELDS);
  out->off_target_lanes = at(VP_LANE_T); out->off_trusted_lanes = at(VP_LANE_R);
  out->off_nodes_target = at(VP_NODES_T); out->off_nodes_trusted = at(VP_NODES_R); out->off_proof_derived = at(VP_PROOF_D);
  out->tree_nodes = L.tree_nodes;
  return TMX_OK;
}

int32_t tmx_inputs_value_batch_device(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets, const void* d_trusteds,
                                      uint32_t sections, void* d_out, void* hip_stream) {
  int32_t st = check_batch_args(c, kind, n_proofs, d_proofs, d_targets, d_trusteds);
  if (st) return st;
  if (!d_out || (sections != TMX_SEC_HINT && sections != TMX_SEC_ALL)) return fail(c, TMX_ERR_BAD_ARG, "d_out must be set and sections TMX_SEC_HINT or TMX_SEC_ALL");
  if (n_proofs == 0) return TMX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  if (!c->d_val_lut[kind]) {  // once per kind (blocking: the table is a local)
    const std::vector<uint16_t> lut = value_fixed_lut(kind);
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipMalloc(&c->d_val_lut[kind], lut.size() * 2));
    HIPCK(c, hipMemcpy(c->d_val_lut[kind], lut.data(), lut.size() * 2, hipMemcpyHostToDevice));
  }
  // the Level-1 kernels without a single element row: no serializer launch, only the lane / proof records and the reports
  st = tmx_witness_batch_device(c, kind, n_proofs, d_proofs, d_targets, d_trusteds, nullptr, c->d_reports, hip_stream);
  if (st) return st;
  const ValueLayout L = value_layout_for(kind, c->cfg.n_max, sections);
  ValueSources V;
  V.proofs = (const uint8_t*)d_proofs; V.targets = (const uint8_t*)d_targets; V.trusteds = (const uint8_t*)d_trusteds;
  V.tl = (const uint8_t*)c->d_tl; V.lr = (const uint8_t*)c->d_lr; V.pf = (const uint8_t*)c->d_pf;
  V.nodes_t = (const uint8_t*)c->d_nodes_t; V.nodes_r = (const uint8_t*)c->d_nodes_r; V.reports = (const uint8_t*)c->d_reports;
  int rc = launch_pack_value(L, V, c->d_val_lut[kind], n_proofs, d_out, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_pack_value launch: ") + hipGetErrorString((hipError_t)rc));
  // the batch now ends with this launch: a later call on another stream must start behind it, not behind the Level-1 kernels' end
  HIPCK(c, hipEventRecord(c->ev_value, s));
  c->ev_done = c->ev_value;
  return TMX_OK;
}

// the device address of `p` if it is mapped page-locked host memory (hipHostMalloc / hipHostRegister with the mapped flag), else null
static void* mapped_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  std::memset(&a, 0, sizeof a);
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (a.type != hipMemoryTypeHost || !a.devicePointer) return nullptr;
  return a.devicePointer;
}

int32_t tmx_inputs_value_batch(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const tmx_proof_rec* proofs, const tmx_validator_rec* targets,
                               const tmx_hashfield_rec* trusteds, uint32_t sections, void* out, uint64_t cap_bytes) {
  if (!c || !proofs || !targets || !out || (kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP)) return TMX_ERR_BAD_ARG;
  if (kind == TMX_KIND_SKIP && !trusteds) return fail(c, TMX_ERR_BAD_ARG, "skip needs the trusted hash fields");
  if (sections != TMX_SEC_HINT && sections != TMX_SEC_ALL) return fail(c, TMX_ERR_BAD_ARG, "sections must be TMX_SEC_HINT or TMX_SEC_ALL");
  if (n_proofs == 0) return TMX_OK;
  if (n_proofs > c->cfg.max_batch) return fail(c, TMX_ERR_CAPACITY, "n_proofs exceeds the context's max_batch");
  const uint32_t n = c->cfg.n_max;
  const ValueLayout L = value_layout_for(kind, n, sections);
  const size_t bytes = (size_t)n_proofs * L.off[VP_COUNT];
  if (cap_bytes < bytes) return fail(c, TMX_ERR_CAPACITY, "out buffer too small");
  for (uint32_t p = 0; p < n_proofs; p++)  // reference input/mod.rs:439-444, 338-342
    if (proofs[p].nb_a > n || (kind == TMX_KIND_SKIP && proofs[p].nb_b > n)) return fail(c, TMX_ERR_SET_TOO_LARGE, "validator set larger than VALIDATOR_SET_SIZE_MAX");
  int32_t st = ensure_staging_inputs(c);
  if (st) return st;
  const size_t lanes = (size_t)n_proofs * n;
  HIPCK(c, hipMemcpyAsync(c->d_in_proofs, proofs, (size_t)n_proofs * sizeof(tmx_proof_rec), hipMemcpyHostToDevice, c->stream));
  HIPCK(c, hipMemcpyAsync(c->d_in_targets, targets, lanes * sizeof(tmx_validator_rec), hipMemcpyHostToDevice, c->stream));
  if (kind == TMX_KIND_SKIP)
    HIPCK(c, hipMemcpyAsync(c->d_in_trusteds, trusteds, lanes * sizeof(tmx_hashfield_rec), hipMemcpyHostToDevice, c->stream));
  // A page-locked `out` is written by k_pack_value itself (posted writes over PCIe: no device-to-host copy to enqueue and wait for) up to
  // TMX_VALUE_DIRECT_MAX bytes; larger transfers, and pageable buffers, go through device staging and one copy.
  static const size_t direct_max = std::getenv("TMX_VALUE_DIRECT_MAX") ? (size_t)std::atoll(std::getenv("TMX_VALUE_DIRECT_MAX")) : ((size_t)1 << 20);
  void* direct = bytes <= direct_max ? mapped_device_ptr(out) : nullptr;
  void* dst = direct;
  if (!dst) {
    if (c->d_value_bytes < bytes) {
      if (c->d_value) { HIPCK(c, hipStreamSynchronize(c->stream)); HIPCK(c, hipFree(c->d_value)); c->d_value = nullptr; c->d_value_bytes = 0; }
      const size_t per = std::max<size_t>(value_layout_for(TMX_KIND_STEP, n, TMX_SEC_ALL).off[VP_COUNT], value_layout_for(TMX_KIND_SKIP, n, TMX_SEC_ALL).off[VP_COUNT]);
      const size_t want = (size_t)c->cfg.max_batch * per;
      HIPCK(c, hipMalloc(&c->d_value, want));
      c->d_value_bytes = want;
    }
    dst = c->d_value;
  }
  st = tmx_inputs_value_batch_device(c, kind, n_proofs, c->d_in_proofs, c->d_in_targets, kind == TMX_KIND_SKIP ? c->d_in_trusteds : nullptr, sections, dst,
                                     c->stream);
  if (st) return st;
  if (!direct) HIPCK(c, hipMemcpyAsync(out, c->d_value, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCK(c, hipStreamSynchronize(c->stream));
  return TMX_OK;
}

int32_t tmx_skip_inputs_value(tmx_ctx* c, const tmx_proof_rec* proof, const tmx_validator_rec* target, const tmx_hashfield_rec* trusted, uint32_t sections,
                              void* out, uint64_t cap_bytes) {
  return tmx_inputs_value_batch(c, TMX_KIND_SKIP, 1, proof, target, trusted, sections, out, cap_bytes);
}
int32_t tmx_step_inputs_value(tmx_ctx* c, const tmx_proof_rec* proof, const tmx_validator_rec* target, uint32_t sections, void* out, uint64_t cap_bytes) {
  return tmx_inputs_value_batch(c, TMX_KIND_STEP, 1, proof, target, nullptr, sections, out, cap_bytes);
}

void* tmx_host_alloc(tmx_ctx* c, uint64_t bytes) {
  if (!c || bytes == 0) return nullptr;
  if (hipSetDevice(c->cfg.device) != hipSuccess) return nullptr;
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}
void tmx_host_free(tmx_ctx* c, void* p) {
  (void)c;
  if (p) (void)hipHostFree(p);
}

}  // extern "C"

extern "C" {

int32_t tmx_eddsa_lanes(tmx_ctx* c, uint32_t n_lanes, const tmx_validator_rec* lanes, uint8_t* out) {
  if (!c || !lanes || !out) return TMX_ERR_BAD_ARG;
  if (n_lanes == 0) return TMX_OK;
  if ((uint64_t)n_lanes > (uint64_t)c->cfg.max_batch * c->cfg.n_max) return fail(c, TMX_ERR_CAPACITY, "n_lanes exceeds max_batch * n_max");
  int32_t st = ensure_staging_inputs(c);
  if (st) return st;
  HIPCK(c, hipMemcpyAsync(c->d_in_targets, lanes, (size_t)n_lanes * sizeof(tmx_validator_rec), hipMemcpyHostToDevice, c->stream));
  if (use_tiny(c, n_lanes)) {
    st = run_tiny_lanes(c, n_lanes, c->d_in_targets, c->d_ed, ED_STRIDE, c->stream);
    if (st) return st;
  } else {
    int rc = run_eddsa(c, n_lanes, c->d_in_targets, c->d_ed, ED_STRIDE, c->stream);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_eddsa launch: ") + hipGetErrorString((hipError_t)rc));
  }
  HIPCK(c, hipMemcpyAsync(out, c->d_ed, (size_t)n_lanes * ED_STRIDE, hipMemcpyDeviceToHost, c->stream));
  HIPCK(c, hipStreamSynchronize(c->stream));
  return TMX_OK;
}

int32_t tmx_valid_skip_batch(tmx_ctx* c, uint32_t n_cand, const tmx_addr_rec* start, uint32_t n_start, const tmx_addr_rec* targets,
                             const uint32_t* n_targets, const tmx_addr_rec* sigs, const uint32_t* n_sigs, uint8_t* valid, uint64_t* shared_power,
                             uint64_t* total_power) {
  if (!c || !start || !targets || !n_targets || !sigs || !n_sigs || !valid || !shared_power || !total_power) return TMX_ERR_BAD_ARG;
  if (n_cand == 0) return TMX_OK;
  const uint32_t n = c->cfg.n_max;
  if (n_start > n) return fail(c, TMX_ERR_SET_TOO_LARGE, "start validator set larger than VALIDATOR_SET_SIZE_MAX");
  static_assert(sizeof(tmx_addr_rec) == 32, "address record layout");
  int32_t hs = ensure_host_stream(c);
  if (hs) return hs;
  const size_t per = (size_t)n * 32;
  // small, latency-only call: temporary device buffers on the context's stream
  void *d_start = nullptr, *d_t = nullptr, *d_s = nullptr, *d_nt = nullptr, *d_ns = nullptr, *d_v = nullptr, *d_sh = nullptr, *d_to = nullptr;
  auto cleanup = [&]() { for (void* p : {d_start, d_t, d_s, d_nt, d_ns, d_v, d_sh, d_to}) if (p) (void)hipFree(p); };
  hipError_t e = hipSuccess;
  auto ck = [&](hipError_t r) { if (e == hipSuccess && r != hipSuccess) e = r; };
  ck(hipMalloc(&d_start, per)); ck(hipMalloc(&d_t, per * n_cand)); ck(hipMalloc(&d_s, per * n_cand)); ck(hipMalloc(&d_nt, 4 * (size_t)n_cand));
  ck(hipMalloc(&d_ns, 4 * (size_t)n_cand)); ck(hipMalloc(&d_v, n_cand)); ck(hipMalloc(&d_sh, 8 * (size_t)n_cand)); ck(hipMalloc(&d_to, 8 * (size_t)n_cand));
  if (e == hipSuccess) {
    ck(hipMemcpyAsync(d_start, start, (size_t)n_start * 32, hipMemcpyHostToDevice, c->stream));
    ck(hipMemcpyAsync(d_t, targets, per * n_cand, hipMemcpyHostToDevice, c->stream));
    ck(hipMemcpyAsync(d_s, sigs, per * n_cand, hipMemcpyHostToDevice, c->stream));
    ck(hipMemcpyAsync(d_nt, n_targets, 4 * (size_t)n_cand, hipMemcpyHostToDevice, c->stream));
    ck(hipMemcpyAsync(d_ns, n_sigs, 4 * (size_t)n_cand, hipMemcpyHostToDevice, c->stream));
  }
  if (e == hipSuccess) ck((hipError_t)launch_valid_skip(n_cand, n, d_start, n_start, d_t, d_nt, d_s, d_ns, d_v, d_sh, d_to, c->stream));
  if (e == hipSuccess) {
    ck(hipMemcpyAsync(valid, d_v, n_cand, hipMemcpyDeviceToHost, c->stream));
    ck(hipMemcpyAsync(shared_power, d_sh, 8 * (size_t)n_cand, hipMemcpyDeviceToHost, c->stream));
    ck(hipMemcpyAsync(total_power, d_to, 8 * (size_t)n_cand, hipMemcpyDeviceToHost, c->stream));
    ck(hipStreamSynchronize(c->stream));
  }
  cleanup();
  if (e != hipSuccess) return fail(c, TMX_ERR_HIP, std::string("tmx_valid_skip_batch: ") + hipGetErrorString(e));
  return TMX_OK;
}

// ---- public I/O packing (big-endian, abi.encodePacked): TendermintX.sol:104-108, skip.rs:120-122, step.rs:107-108
static void be64(uint64_t v, uint8_t* o) { for (int i = 0; i < 8; i++) o[i] = (uint8_t)(v >> (56 - 8 * i)); }
static uint64_t rd_be64(const uint8_t* p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v = (v << 8) | p[i]; return v; }
void tmx_pack_skip_input(uint64_t trusted_block, const uint8_t h[32], uint64_t target_block, uint8_t out[48]) {
  be64(trusted_block, out); std::memcpy(out + 8, h, 32); be64(target_block, out + 40);
}
void tmx_unpack_skip_input(const uint8_t in[48], uint64_t* trusted_block, uint8_t h[32], uint64_t* target_block) {
  *trusted_block = rd_be64(in); std::memcpy(h, in + 8, 32); *target_block = rd_be64(in + 40);
}
void tmx_pack_step_input(uint64_t prev_block, const uint8_t h[32], uint8_t out[40]) { be64(prev_block, out); std::memcpy(out + 8, h, 32); }
void tmx_unpack_step_input(const uint8_t in[40], uint64_t* prev_block, uint8_t h[32]) { *prev_block = rd_be64(in); std::memcpy(h, in + 8, 32); }


// ---- Goldilocks NTT / coset LDE ------------------------------------------------------------------------------------------------
static int32_t ntt_table(tmx_ctx* c, uint32_t log_n, hipStream_t s, void** w) {
  if (!c->d_ntt_w[log_n]) {
    const size_t half = log_n ? ((size_t)1 << (log_n - 1)) : 1;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipMalloc(&c->d_ntt_w[log_n], half * 8));
    int rc = launch_ntt_table(c->d_ntt_w[log_n], log_n, c->ntt_root, s);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_ntt_table launch: ") + hipGetErrorString((hipError_t)rc));
    HIPCK(c, hipStreamSynchronize(s));  // once per size: later calls may come on another stream
  }
  *w = c->d_ntt_w[log_n];
  return TMX_OK;
}
// the twiddles between the two passes of a four-step transform (log_n > 11), as a matrix in the layout pass A writes: N x 8 bytes per
// size and direction, built once (the passes then read them with the coalescing of their own stores instead of gathering 8-byte words)
static int32_t ntt_matrix(tmx_ctx* c, uint32_t log_n, uint32_t log_n2, bool inverse, const void* w, hipStream_t s, void** m) {
  void*& slot = c->d_ntt_m[inverse ? 1 : 0][log_n];
  if (!slot) {
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipMalloc(&slot, (size_t)8 << log_n));
    int rc = launch_ntt_matrix(slot, w, log_n, log_n2, inverse, s);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_ntt_matrix launch: ") + hipGetErrorString((hipError_t)rc));
    HIPCK(c, hipStreamSynchronize(s));
  }
  *m = slot;
  return TMX_OK;
}
static int32_t ntt_scratch(tmx_ctx* c, size_t bytes, hipStream_t s) {
  if (c->ntt_tmp_bytes >= bytes) return TMX_OK;
  HIPCK(c, hipSetDevice(c->cfg.device));
  if (c->d_ntt_tmp) {
    HIPCK(c, hipStreamSynchronize(s));  // earlier transforms on this stream may still read it
    HIPCK(c, hipFree(c->d_ntt_tmp));
    c->d_ntt_tmp = nullptr; c->ntt_tmp_bytes = 0;
  }
  HIPCK(c, hipMalloc(&c->d_ntt_tmp, bytes));
  c->ntt_tmp_bytes = bytes;
  return TMX_OK;
}
static uint64_t gl_pow_host(uint64_t b, uint64_t e) {
  const unsigned __int128 p = 0xffffffff00000001ull;
  unsigned __int128 r = 1, x = b % p;
  while (e) {
    if (e & 1) r = r * x % p;
    x = x * x % p;
    e >>= 1;
  }
  return (uint64_t)r;
}
// columns of 2^log_n elements, column c at element c * col_stride; `tmp` (n_cols << log_n elements) only for log_n > 11
// post_vec (or null): the outputs are multiplied by post_vec[k] INSTEAD of the inverse transform's 1 / N (a vector that carries it);
// nonzero (or 0): only the first `nonzero` inputs of every column are non-zero and read (a multiple of N2 for a two-pass transform).
static int32_t ntt_run(tmx_ctx* c, uint32_t log_n, uint32_t n_cols, const void* d_in, uint64_t in_stride, void* d_out, uint64_t out_stride,
                       void* tmp, bool inverse, hipStream_t s, const void* post_vec = nullptr, uint64_t nonzero = 0) {
  void* w = nullptr;
  int32_t st = ntt_table(c, log_n, s, &w);
  if (st) return st;
  const uint64_t n_inv = inverse ? gl_pow_host((uint64_t)1 << log_n, 0xffffffff00000001ull - 2) : 1;
  NttPass P;
  std::memset(&P, 0, sizeof P);
  P.log_n = log_n; P.inverse = inverse ? 1 : 0;
  {  // omega_16 of the domain (its inverse for an inverse transform) is an odd power k of 2^12: the kernel loads in the order kinv i
    const uint64_t w16 = gl_pow_host(c->ntt_root, (1ull << 28) * (inverse ? 15u : 1u));
    uint32_t k = 0;
    for (uint32_t t = 1; t < 16; t += 2)
      if (gl_pow_host(1ull << 12, t) == w16) k = t;
    if (!k) return fail(c, TMX_ERR_BAD_ARG, "omega_16 of the NTT domain is not a power of 2^12");
    for (uint32_t t = 1; t < 16; t += 2)
      if (((t * k) & 15u) == 1u) P.kinv = t;
  }
  int rc;
  if (log_n <= 11) {  // one pass: whole columns in LDS, T columns per tile
    P.log_l = log_n; P.log_t = 12 - log_n;
    if (((uint64_t)1 << P.log_t) > n_cols) { P.log_t = 0; while (((uint64_t)2 << P.log_t) <= n_cols) P.log_t++; }
    const uint32_t T = 1u << P.log_t;
    // the "columns" of the kernel are groups of T real columns: sub-transform t of a group = column, stride = column stride
    P.tiles_per_col = (n_cols + T - 1) / T; P.n_sub = n_cols;
    P.col_stride_in = 0; P.t_stride_in = in_stride; P.j_stride_in = 1;
    P.col_stride_out = 0; P.t_stride_out = out_stride; P.j_stride_out = 1;
    P.scale = post_vec ? 1 : n_inv; P.post_twiddle = post_vec ? 1 : 0; P.tm_t_stride = 0; P.j_nonzero = (uint32_t)nonzero;
    rc = launch_ntt_pass(P, 1, d_in, d_out, w, post_vec, s);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_ntt_tile launch: ") + hipGetErrorString((hipError_t)rc));
    return TMX_OK;
  }
  // N = N1 N2, N1 = 2^a (pass A, strided), N2 = 2^b (pass B, contiguous).  (Round 3 re-measured the split and the tile sizes at 2^16 / 2^20 /
  // 2^22: a = ceil(log_n / 2) -1 / -2 / +1 and tiles of 2^12 / 2^13 / 2^14 elements everywhere -- the balanced split with the tile rule below wins each; round 4 re-measured pass A's tile alone at
  // 2^16 / 2^20 / 2^22: 0.161 / 4.53 / 2.11 ms with 2^12, 0.169 / 3.29 / 1.71 with 2^13, 0.191 / 3.32 / 1.24 with 2^14 -- the rule's choices.)
  const uint32_t a = (log_n + 1) / 2, b = log_n - a;
  const uint64_t N = (uint64_t)1 << log_n, N1 = (uint64_t)1 << a, N2 = (uint64_t)1 << b;
  // tiles of the two strided passes: T >= 8 sub-transforms side by side (runs of >= 64 B along the unit-stride dimension; with T = 4 at
  // N1 = 2^10, FETCH_SIZE was 4x the data), in the smallest tile that allows it (2^12 .. 2^14 elements: three, two or one workgroup per
  // CU's LDS).  Measured at 2^16 / 2^20 / 2^22: tiles of 2^12 / 2^13 / 2^14 elements are each the fastest there.
  auto tile_log_of = [&](uint32_t log_l) { return std::min(14u, std::max(12u, log_l + 3u)); };
  P.log_l = a; P.log_t = std::min(tile_log_of(a) - a, b); P.n_sub = N2; P.tiles_per_col = (uint32_t)(N2 >> P.log_t);
  P.col_stride_in = in_stride; P.t_stride_in = 1; P.j_stride_in = N2;
  P.col_stride_out = N; P.t_stride_out = 1; P.j_stride_out = N2;
  P.post_twiddle = 1; P.scale = 1; P.tm_t_stride = P.t_stride_out;
  P.j_nonzero = nonzero ? (uint32_t)(nonzero >> b) : 0u;  // input n1 N2 + n2 is zero from n1 = nonzero / N2 on
  void* m = nullptr;
  st = ntt_matrix(c, log_n, b, inverse, w, s, &m);
  if (st) return st;
  rc = launch_ntt_pass(P, n_cols, d_in, tmp, w, m, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_ntt_tile launch: ") + hipGetErrorString((hipError_t)rc));
  P.log_l = b; P.log_t = std::min(tile_log_of(b) - b, a); P.n_sub = N1; P.tiles_per_col = (uint32_t)(N1 >> P.log_t);
  P.col_stride_in = N; P.t_stride_in = N2; P.j_stride_in = 1;
  P.col_stride_out = out_stride; P.t_stride_out = 1; P.j_stride_out = N1;
  P.post_twiddle = post_vec ? 1 : 0; P.scale = post_vec ? 1 : n_inv; P.tm_t_stride = P.t_stride_out; P.j_nonzero = 0;
  rc = launch_ntt_pass(P, n_cols, tmp, d_out, w, post_vec, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_ntt_tile launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

int32_t tmx_ntt_set_domain(tmx_ctx* c, uint64_t root_2_32, uint64_t coset_shift) {
  if (!c) return TMX_ERR_BAD_ARG;
  const uint64_t P = 0xffffffff00000001ull;
  if (root_2_32 >= P || coset_shift == 0 || coset_shift >= P || gl_pow_host(root_2_32, 1ull << 31) != P - 1)
    return fail(c, TMX_ERR_BAD_ARG, "root_2_32 must be a primitive 2^32-th root of unity of the Goldilocks field, coset_shift a non-zero element");
  if (root_2_32 != c->ntt_root || coset_shift != c->ntt_shift) {  // the tables belong to the old domain
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipDeviceSynchronize());
    for (auto& v : c->d_lde_s)
      if (v) { (void)hipFree(v); v = nullptr; }
  }
  if (root_2_32 != c->ntt_root) {
    for (auto& w : c->d_ntt_w)
      if (w) { (void)hipFree(w); w = nullptr; }
    for (auto& dir : c->d_ntt_m)
      for (auto& m : dir)
        if (m) { (void)hipFree(m); m = nullptr; }
  }
  c->ntt_root = root_2_32; c->ntt_shift = coset_shift;
  return TMX_OK;
}

int32_t tmx_ntt_goldilocks_device(tmx_ctx* c, uint32_t log_n, uint32_t n_cols, const uint64_t* d_in, uint64_t* d_out, int32_t inverse,
                                  void* hip_stream) {
  if (!c || !d_in || !d_out) return TMX_ERR_BAD_ARG;
  if (log_n > TMX_NTT_MAX_LOG) return fail(c, TMX_ERR_CAPACITY, "log_n exceeds TMX_NTT_MAX_LOG");
  if (n_cols == 0) return TMX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  const uint64_t N = (uint64_t)1 << log_n;
  if (log_n > 11) {
    int32_t st = ntt_scratch(c, (size_t)n_cols * N * 8, s);
    if (st) return st;
  }
  return ntt_run(c, log_n, n_cols, d_in, N, d_out, N, c->d_ntt_tmp, inverse != 0, s);
}

int32_t tmx_lde_goldilocks_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t n_cols, const uint64_t* d_in, uint64_t* d_out,
                                  void* hip_stream) {
  if (!c || !d_in || !d_out) return TMX_ERR_BAD_ARG;
  const uint32_t log_m = log_n + log_blowup;
  if (log_m > TMX_NTT_MAX_LOG) return fail(c, TMX_ERR_CAPACITY, "log_n + log_blowup exceeds TMX_NTT_MAX_LOG");
  if (n_cols == 0) return TMX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  const uint64_t N = (uint64_t)1 << log_n, M = (uint64_t)1 << log_m;
  // scratch: [coefficients, n_cols x M] [four-step intermediate, n_cols x M]
  int32_t st = ntt_scratch(c, (size_t)n_cols * M * 8 * 2, s);
  if (st) return st;
  uint64_t* coef = reinterpret_cast<uint64_t*>(c->d_ntt_tmp);
  uint64_t* tmp = coef + (size_t)n_cols * M;
  // Fused form: the inverse transform's last pass multiplies coefficient i by S[i] = shift^i / N (one vector per column length, built
  // once), and the forward transform does not read the zero padding -- its pass A loads the first N / N2 inputs of every strided
  // sub-transform only.  (Before: k_lde_expand rewrote all M slots, a gl_pow per coefficient, and pass A read them back: 17 of the ~55 GB
  // an 8x LDE of 2^15-row columns moved.)  A split whose N2 exceeds N keeps the padded form.
  const uint32_t b_fwd = log_m > 11 ? log_m - (log_m + 1) / 2 : 0;
  const bool fused = !(std::getenv("TMX_LDE_FUSED") && std::getenv("TMX_LDE_FUSED")[0] == '0') && log_n >= b_fwd;
  if (fused) {
    if (!c->d_lde_s[log_n]) {
      HIPCK(c, hipSetDevice(c->cfg.device));
      HIPCK(c, hipMalloc(&c->d_lde_s[log_n], (size_t)8 << log_n));
      int rc = launch_lde_scale_table(c->d_lde_s[log_n], log_n, c->ntt_shift, gl_pow_host(N, 0xffffffff00000001ull - 2), s);
      if (rc) return fail(c, TMX_ERR_HIP, std::string("k_lde_scale_table launch: ") + hipGetErrorString((hipError_t)rc));
      HIPCK(c, hipStreamSynchronize(s));  // once per size: later calls may come on another stream
    }
    st = ntt_run(c, log_n, n_cols, d_in, N, coef, M, tmp, true, s, c->d_lde_s[log_n]);  // scaled coefficients into the first N slots of every M-slot column
    if (st) return st;
    return ntt_run(c, log_m, n_cols, coef, M, d_out, M, tmp, false, s, nullptr, N);
  }
  st = ntt_run(c, log_n, n_cols, d_in, N, coef, M, tmp, true, s);  // coefficients into the first N slots of every M-slot column
  if (st) return st;
  int rc = launch_lde_expand(coef, log_n, log_m, n_cols, c->ntt_shift, s);  // c_i shift^i, zero padding
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_lde_expand launch: ") + hipGetErrorString((hipError_t)rc));
  return ntt_run(c, log_m, n_cols, coef, M, d_out, M, tmp, false, s);
}

// self-test hook: both inversions mod 2^255 - 19 (the Fermat chain and the safegcd one k_ed_fin uses) on n values of eight LE words
int32_t tmx_selftest_f16(tmx_ctx* c, uint32_t n, uint32_t doublings, const uint32_t* in_words, uint32_t* out_words) {
  if (!c || !in_words || !out_words) return TMX_ERR_BAD_ARG;
  if (n == 0) return TMX_OK;
  HIPCK(c, hipSetDevice(c->cfg.device));
  void *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, (size_t)n * 512);
  if (e == hipSuccess) e = hipMalloc(&d_out, (size_t)n * 1024);
  if (e == hipSuccess) e = hipMemcpy(d_in, in_words, (size_t)n * 512, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, (size_t)n * 1024, c->side2);
  if (e == hipSuccess) e = (hipError_t)launch_selftest_f16(n, doublings, d_in, d_out, c->side2);
  if (e == hipSuccess) e = hipStreamSynchronize(c->side2);
  if (e == hipSuccess) e = hipMemcpy(out_words, d_out, (size_t)n * 1024, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  if (e != hipSuccess) return fail(c, TMX_ERR_HIP, std::string("tmx_selftest_f16: ") + hipGetErrorString(e));
  return TMX_OK;
}

int32_t tmx_selftest_fe_invert(tmx_ctx* c, uint32_t n, const uint32_t* in_words, uint32_t* out_words) {
  if (!c || !in_words || !out_words) return TMX_ERR_BAD_ARG;
  if (n == 0) return TMX_OK;
  HIPCK(c, hipSetDevice(c->cfg.device));
  void *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, (size_t)n * 32);
  if (e == hipSuccess) e = hipMalloc(&d_out, (size_t)n * 64);
  if (e == hipSuccess) e = hipMemcpy(d_in, in_words, (size_t)n * 32, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = (hipError_t)launch_selftest_invert(n, d_in, d_out, c->side2);
  if (e == hipSuccess) e = hipStreamSynchronize(c->side2);
  if (e == hipSuccess) e = hipMemcpy(out_words, d_out, (size_t)n * 64, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  if (e != hipSuccess) return fail(c, TMX_ERR_HIP, std::string("tmx_selftest_fe_invert: ") + hipGetErrorString(e));
  return TMX_OK;
}

}  // extern "C"

// ---- Poseidon over Goldilocks + Merkle caps --------------------------------------------------------------------------------------
// default round constants: the Poseidon paper's Grain LFSR (80 bits: field 1 | sbox 0 | n 64 | t 12 | R_F 8 | R_P 22 | thirty ones; 160 bits
// discarded; bits taken in pairs, the second kept when the first is 1; 64-bit big-endian integers, rejected when >= p) -- a third
// implementation beside the two of the test oracle (tests compare the streams)
static void poseidon_default_constants(std::vector<uint64_t>& k) {
  k.assign(POS_CONST_WORDS, 0);
  uint8_t st[80];
  int n = 0;
  const uint32_t fields[6][2] = {{1, 2}, {0, 4}, {64, 12}, {POS_T, 12}, {POS_RF, 10}, {POS_RP, 10}};
  for (auto& f : fields)
    for (int i = (int)f[1] - 1; i >= 0; i--) st[n++] = (uint8_t)((f[0] >> i) & 1u);
  while (n < 80) st[n++] = 1;
  int head = 0;
  auto next = [&]() {
    const uint8_t b = st[(head + 62) % 80] ^ st[(head + 51) % 80] ^ st[(head + 38) % 80] ^ st[(head + 23) % 80] ^ st[(head + 13) % 80] ^ st[head];
    st[head] = b;
    head = (head + 1) % 80;
    return b;
  };
  for (int i = 0; i < 160; i++) (void)next();
  uint32_t got = 0;
  while (got < POS_ROUNDS * POS_T) {
    uint64_t v = 0;
    for (int bits = 0; bits < 64;) {
      const uint8_t a = next(), b = next();
      if (a) { v = (v << 1) | b; bits++; }
    }
    if (v < 0xffffffff00000001ull) k[got++] = v;
  }
  static const uint64_t circ[POS_T] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
  for (uint32_t i = 0; i < POS_T; i++) { k[POS_ROUNDS * POS_T + i] = circ[i]; k[POS_ROUNDS * POS_T + POS_T + i] = i == 0 ? 8 : 0; }
}
// The device buffer behind the caller-visible constants: the tables of the merged partial rounds (poseidon.h), from the MDS matrix over
// the integers.  Returns the mode the kernels can run in.
static int poseidon_tables(const std::vector<uint64_t>& k, std::vector<uint64_t>& dev) {
  const unsigned __int128 P = 0xffffffff00000001ull;
  dev.assign(POS_CONST_WORDS_EXT, 0);
  std::copy(k.begin(), k.begin() + POS_CONST_WORDS, dev.begin());
  const uint64_t* circ = &k[POS_ROUNDS * POS_T];
  const uint64_t* diag = circ + POS_T;
  for (uint32_t i = 0; i < 2 * POS_T; i++)
    if (circ[i] >> 16) return POS_MODE_GENERAL;
  // M[r][j] = circ[(j - r) mod 12] + (j == r) diag[r]   (out[r] = sum_i circ[i] s[(i + r) mod 12] + diag[r] s[r], poseidon.hip: pos_mds)
  unsigned __int128 M[3][POS_T][POS_T];
  const unsigned __int128 LIM = (unsigned __int128)1 << 26;
  for (uint32_t r = 0; r < POS_T; r++)
    for (uint32_t j = 0; j < POS_T; j++) M[0][r][j] = circ[(j + POS_T - r) % POS_T] + (j == r ? diag[r] : 0);
  for (int e = 1; e < 3; e++)
    for (uint32_t r = 0; r < POS_T; r++)
      for (uint32_t j = 0; j < POS_T; j++) {
        unsigned __int128 a = 0;
        for (uint32_t t = 0; t < POS_T; t++) a += M[e - 1][r][t] * M[0][t][j];
        if (a >= LIM) return POS_MODE_SMALL;  // (entries only grow: M^3 decides)
        M[e][r][j] = a;
      }
  for (uint32_t r = 0; r < POS_T; r++)
    for (uint32_t j = 0; j < POS_T; j++)
      if (M[0][r][j] >= LIM) return POS_MODE_SMALL;
  uint32_t* U = reinterpret_cast<uint32_t*>(&dev[POS_X_U32]);
  for (uint32_t i = 0; i < POS_T; i++) {
    U[POS_U_R1 + i] = (uint32_t)M[0][0][i]; U[POS_U_R2 + i] = (uint32_t)M[1][0][i];
    U[POS_U_C2 + i] = (uint32_t)M[1][i][0]; U[POS_U_C1 + i] = (uint32_t)M[0][i][0];
    for (uint32_t j = 0; j < POS_T; j++) U[POS_U_M3 + POS_T * i + j] = (uint32_t)M[2][i][j];
  }
  auto mat_vec = [&](int e, const uint64_t* v, uint64_t* out) {  // out = M^(e+1) v mod p
    for (uint32_t r = 0; r < POS_T; r++) {
      unsigned __int128 a = 0;
      for (uint32_t j = 0; j < POS_T; j++) a = (a + M[e][r][j] * v[j]) % P;
      out[r] = (uint64_t)a;
    }
  };
  for (uint32_t g = 0; g < POS_MERGE_GROUPS; g++) {
    const uint32_t r = POS_MERGE_FIRST + 3 * g;
    const uint64_t *rc1 = &k[(r + 1) * POS_T], *rc2 = &k[(r + 2) * POS_T], *rc3 = &k[(r + 3) * POS_T];
    uint64_t m_rc1[POS_T], m2_rc1[POS_T], m_rc2[POS_T];
    mat_vec(0, rc1, m_rc1); mat_vec(1, rc1, m2_rc1); mat_vec(0, rc2, m_rc2);
    uint64_t* G = &dev[POS_X_GROUPS + g * POS_X_GROUP_WORDS];
    G[0] = rc1[0];
    G[1] = (uint64_t)(((unsigned __int128)m_rc1[0] + rc2[0]) % P);
    for (uint32_t i = 0; i < POS_T; i++) G[2 + i] = (uint64_t)(((unsigned __int128)m2_rc1[i] + m_rc2[i] + rc3[i]) % P);
  }
  return POS_MODE_MERGE3;
}
static int32_t poseidon_ready(tmx_ctx* c, hipStream_t s) {
  if (c->pos_consts.empty()) poseidon_default_constants(c->pos_consts);
  if (!c->d_pos_consts) {
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipMalloc(&c->d_pos_consts, POS_CONST_WORDS_EXT * 8));
    c->pos_dirty = true;
  }
  if (c->pos_dirty) {
    std::vector<uint64_t> dev;
    int mode = poseidon_tables(c->pos_consts, dev);
    if (const char* v = std::getenv("TMX_POSEIDON_MERGE"))  // TMX_POSEIDON_MERGE=0: one dense layer per partial round (times the merged form against it)
      if (v[0] == '0' && mode == POS_MODE_MERGE3) mode = POS_MODE_SMALL;
    HIPCK(c, hipMemcpyAsync(c->d_pos_consts, dev.data(), POS_CONST_WORDS_EXT * 8, hipMemcpyHostToDevice, s));
    HIPCK(c, hipStreamSynchronize(s));  // once per change of the tables: later calls may come on another stream (and `dev` is a local)
    c->pos_dirty = false;
    c->pos_mode = mode;
  }
  return TMX_OK;
}

extern "C" {

int32_t tmx_poseidon_set_constants(tmx_ctx* c, const uint64_t* rc, const uint64_t* circ, const uint64_t* diag) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (c->pos_consts.empty()) poseidon_default_constants(c->pos_consts);
  const uint64_t P = 0xffffffff00000001ull;
  if (rc) {
    for (uint32_t i = 0; i < POS_ROUNDS * POS_T; i++) c->pos_consts[i] = rc[i] % P;
    c->pos_rc_injected = true;
  }
  if (circ) for (uint32_t i = 0; i < POS_T; i++) c->pos_consts[POS_ROUNDS * POS_T + i] = circ[i] % P;
  if (diag) for (uint32_t i = 0; i < POS_T; i++) c->pos_consts[POS_ROUNDS * POS_T + POS_T + i] = diag[i] % P;
  if (c->d_pos_consts) {  // kernels in flight may still read the old tables
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipDeviceSynchronize());
  }
  c->pos_dirty = true;
  return TMX_OK;
}

int32_t tmx_poseidon_constants_injected(const tmx_ctx* c) { return c ? (c->pos_rc_injected ? 1 : 0) : TMX_ERR_BAD_ARG; }

uint64_t tmx_poseidon_merkle_digests(uint32_t log_n, uint32_t cap_height) {
  if (log_n > 30 || cap_height > log_n) return 0;
  uint64_t total = 0;
  for (uint32_t k = 0; k + cap_height <= log_n; k++) total += 1ull << (log_n - k);
  return total;
}

int32_t tmx_poseidon_merkle_device(tmx_ctx* c, uint32_t log_n, uint32_t n_cols, const uint64_t* d_cols, uint32_t cap_height, uint64_t* d_levels,
                                   void* hip_stream) {
  if (!c || !d_cols || !d_levels || n_cols == 0) return TMX_ERR_BAD_ARG;
  if (log_n > 30 || cap_height > log_n) return fail(c, TMX_ERR_BAD_ARG, "cap_height must not exceed log_n (<= 30)");
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  int32_t st = poseidon_ready(c, s);
  if (st) return st;
  int rc = launch_poseidon_leaves(c->d_pos_consts, c->pos_mode, log_n, n_cols, d_cols, d_levels, s);
  uint64_t* cur = d_levels;
  for (uint32_t k = 0; !rc && k + cap_height < log_n; k++) {
    const uint64_t cnt = 1ull << (log_n - k);
    rc = launch_poseidon_level(c->d_pos_consts, c->pos_mode, cnt / 2, cur, cur + 4 * cnt, s);
    cur += 4 * cnt;
  }
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_poseidon launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

int32_t tmx_poseidon_permute(tmx_ctx* c, uint32_t n, const uint64_t* in, uint64_t* out) {
  if (!c || !in || !out) return TMX_ERR_BAD_ARG;
  if (n == 0) return TMX_OK;
  HIPCK(c, hipSetDevice(c->cfg.device));
  int32_t st = poseidon_ready(c, c->side2);
  if (st) return st;
  void *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, (size_t)n * 96);
  if (e == hipSuccess) e = hipMalloc(&d_out, (size_t)n * 96);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, (size_t)n * 96, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = (hipError_t)launch_poseidon_permute(c->d_pos_consts, c->pos_mode, n, d_in, d_out, c->side2);
  if (e == hipSuccess) e = hipStreamSynchronize(c->side2);
  if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n * 96, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  if (e != hipSuccess) return fail(c, TMX_ERR_HIP, std::string("tmx_poseidon_permute: ") + hipGetErrorString(e));
  return TMX_OK;
}

}  // extern "C"

// ---- multi-GPU: RCCL behind the C ABI (include/tmx.h "multi-GPU") -------------------------------------------------------
// RCCL is bound at run time: dlopen / dlsym, never a DT_NEEDED -- the process that loads libtmx decides which librccl (and which HIP
// runtime under it) it runs on.  PyTorch bundles its own; a C / Rust host gets /opt/rocm's.
#include <dlfcn.h>
#include <link.h>

namespace {
struct RcclId { char internal[TMX_UNIQUE_ID_BYTES]; };
static_assert(sizeof(RcclId) == 128, "ncclUniqueId is 128 bytes");
struct Rccl {
  void* lib = nullptr;
  std::string err;
  int (*GetUniqueId)(RcclId*) = nullptr;
  int (*CommInitRank)(void**, int, RcclId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*CommAbort)(void*) = nullptr;               // optional (every NCCL >= 2.4 / RCCL has both): without them an abort is a destroy
  int (*CommGetAsyncError)(void*, int*) = nullptr;
  int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
std::mutex g_rccl_mu;
Rccl g_rccl;
int find_loaded_rccl(struct dl_phdr_info* info, size_t, void* out) {
  if (info->dlpi_name && std::strstr(info->dlpi_name, "librccl")) {
    *reinterpret_cast<std::string*>(out) = info->dlpi_name;
    return 1;
  }
  return 0;
}
// empty on success, else why not (returned by value: the caller's copy cannot change under it)
std::string rccl_load() {
  std::lock_guard<std::mutex> lk(g_rccl_mu);
  Rccl& R = g_rccl;
  if (R.lib) return std::string();
  // an explicit TMX_RCCL_LIB is the ONLY candidate (a host that names a library means it, and a wrong name must be an error, not a silent
  // fall-through to some other copy -- tests/fake_rccl runs two ranks on one GPU this way); otherwise the copy the process already runs on
  // (PyTorch's), then the loader's search path
  std::vector<std::string> names;
  const char* forced = std::getenv("TMX_RCCL_LIB");
  if (forced && forced[0]) {
    names.push_back(forced);
  } else {
    std::string loaded;
    (void)dl_iterate_phdr(find_loaded_rccl, &loaded);
    if (!loaded.empty()) names.push_back(loaded);
    names.push_back("librccl.so.1");
    names.push_back("librccl.so");
    names.push_back("/opt/rocm/lib/librccl.so.1");
  }
  void* h = nullptr;
  std::string why;
  for (const std::string& nm : names) {
    if ((h = dlopen(nm.c_str(), RTLD_NOW | RTLD_GLOBAL))) break;
    const char* e = dlerror();  // (one call: dlerror clears the message it returns)
    if (why.empty()) why = e ? e : "?";
  }
  if (!h) return R.err = "librccl not loadable: " + why;
  Rccl T;
  auto sym = [&](const char* n) { return dlsym(h, n); };
  T.GetUniqueId = reinterpret_cast<decltype(T.GetUniqueId)>(sym("ncclGetUniqueId"));
  T.CommInitRank = reinterpret_cast<decltype(T.CommInitRank)>(sym("ncclCommInitRank"));
  T.CommDestroy = reinterpret_cast<decltype(T.CommDestroy)>(sym("ncclCommDestroy"));
  T.CommAbort = reinterpret_cast<decltype(T.CommAbort)>(sym("ncclCommAbort"));
  T.CommGetAsyncError = reinterpret_cast<decltype(T.CommGetAsyncError)>(sym("ncclCommGetAsyncError"));
  T.Broadcast = reinterpret_cast<decltype(T.Broadcast)>(sym("ncclBroadcast"));
  T.AllGather = reinterpret_cast<decltype(T.AllGather)>(sym("ncclAllGather"));
  T.GroupStart = reinterpret_cast<decltype(T.GroupStart)>(sym("ncclGroupStart"));
  T.GroupEnd = reinterpret_cast<decltype(T.GroupEnd)>(sym("ncclGroupEnd"));
  T.GetErrorString = reinterpret_cast<decltype(T.GetErrorString)>(sym("ncclGetErrorString"));
  if (!T.GetUniqueId || !T.CommInitRank || !T.CommDestroy || !T.Broadcast || !T.AllGather || !T.GroupStart || !T.GroupEnd || !T.GetErrorString) {
    (void)dlclose(h);  // nothing of a half-bound library stays: the next attempt starts from scratch
    return R.err = "librccl lacks one of ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclBroadcast / ncclAllGather / ncclGroupStart / "
                   "ncclGroupEnd / ncclGetErrorString";
  }
  T.lib = h;
  R = T;
  return std::string();
}
int32_t rccl_fail(tmx_ctx* c, const char* what, int rc) {
  return fail(c, TMX_ERR_RCCL, std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?"));
}
// A collective is entered by every rank or by none.  A rank that fails LOCALLY between the start of a sharded call and its exchange (its shard
// exceeds its context's max_batch, a launch fails) would leave the others waiting in the collective for ever: it aborts the communicator
// instead (ncclCommAbort: its peers' pending operations fail), and so does a rank whose collective reports an error.  Either way the call
// returns TMX_ERR_RCCL, the context refuses further sharded calls, and every rank makes a new communicator (tmx_comm_create).
void comm_abort(tmx_ctx* c) {
  if (!c->comm) return;
  if (c->have_streams) (void)hipSetDevice(c->cfg.device);
  if (g_rccl.CommAbort) (void)g_rccl.CommAbort(c->comm);
  else if (g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
  c->comm = nullptr;
  c->comm_aborted = true;
}
int32_t shard_fail(tmx_ctx* c, int32_t st) {
  if (st == TMX_OK || !c->comm) return st;
  const std::string local = c->err;
  comm_abort(c);
  return fail(c, TMX_ERR_RCCL, "local failure in front of a collective (" + std::string(tmx_status_str(st)) + (local.empty() ? "" : ": " + local) +
                                   "): communicator aborted so that no peer waits for this rank; tmx_comm_create again on every rank");
}
int32_t comm_usable(tmx_ctx* c) {
  return c->comm_aborted ? fail(c, TMX_ERR_RCCL, "the communicator of this context was aborted: tmx_comm_create again on every rank") : TMX_OK;
}
int32_t rccl_fail_abort(tmx_ctx* c, const char* what, int rc) {
  const int32_t st = rccl_fail(c, what, rc);
  comm_abort(c);
  return st;
}
constexpr int RCCL_UINT8 = 1;  // ncclUint8
// every rank's slice [lo_r, hi_r) of `n_items` records of `rec_bytes` becomes resident on every rank: one exchange, in place.
// Equal slices (n_items a multiple of the world: 256 proofs or 512 lanes over 2 / 4 / 8 ranks, BASELINE configs[3] / [4]) are ONE
// ncclAllGather -- the collective north_star names and the one RCCL schedules over all seven xGMI links at once -- in its in-place form
// (sendbuff = recvbuff + rank * count); ragged slices fall back to a group of broadcasts, each rank the root of its own slice.
int32_t exchange_slices(tmx_ctx* c, void* d_buf, uint64_t n_items, size_t rec_bytes, hipStream_t s) {
  if (!c->comm || !d_buf || n_items == 0) return TMX_OK;
  int rc;
  if (n_items % c->comm_world == 0) {
    const size_t per = (size_t)(n_items / c->comm_world) * rec_bytes;
    uint8_t* base = reinterpret_cast<uint8_t*>(d_buf);
    rc = g_rccl.AllGather(base + (size_t)c->comm_rank * per, base, per, RCCL_UINT8, c->comm, s);
    if (rc) return rccl_fail_abort(c, "ncclAllGather", rc);
    return TMX_OK;
  }
  rc = g_rccl.GroupStart();
  if (rc) return rccl_fail_abort(c, "ncclGroupStart", rc);
  for (uint32_t r = 0; r < c->comm_world; r++) {
    uint64_t lo, hi;
    tmx_shard_range(n_items, r, c->comm_world, &lo, &hi);
    if (hi == lo) continue;
    uint8_t* p = reinterpret_cast<uint8_t*>(d_buf) + lo * rec_bytes;
    rc = g_rccl.Broadcast(p, p, (size_t)(hi - lo) * rec_bytes, RCCL_UINT8, (int)r, c->comm, s);
    if (rc) { (void)g_rccl.GroupEnd(); return rccl_fail_abort(c, "ncclBroadcast", rc); }
  }
  rc = g_rccl.GroupEnd();
  if (rc) return rccl_fail_abort(c, "ncclGroupEnd", rc);
  return TMX_OK;
}
}  // namespace

extern "C" {

void tmx_shard_range(uint64_t n_items, uint32_t rank, uint32_t world, uint64_t* lo, uint64_t* hi) {
  if (world == 0) world = 1;
  if (rank >= world) rank = world - 1;
  const uint64_t base = n_items / world, rem = n_items % world;
  const uint64_t a = (uint64_t)rank * base + (rank < rem ? rank : rem);
  if (lo) *lo = a;
  if (hi) *hi = a + base + (rank < rem ? 1 : 0);
}

int32_t tmx_comm_unique_id(uint8_t out[TMX_UNIQUE_ID_BYTES]) {
  if (!out) return TMX_ERR_BAD_ARG;
  if (!(g_tls_err = rccl_load()).empty()) return TMX_ERR_RCCL;
  RcclId id;
  std::memset(&id, 0, sizeof id);
  if (const int rc = g_rccl.GetUniqueId(&id)) {
    g_tls_err = std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(rc);
    return TMX_ERR_RCCL;
  }
  std::memcpy(out, id.internal, TMX_UNIQUE_ID_BYTES);
  return TMX_OK;
}

int32_t tmx_comm_create(tmx_ctx* c, const uint8_t* unique_id, uint32_t rank, uint32_t world) {
  if (!c || world == 0 || rank >= world || (world > 1 && !unique_id)) return TMX_ERR_BAD_ARG;
  if (unique_id && c->cfg.device < 0) return TMX_ERR_BAD_ARG;
  int32_t st = tmx_comm_destroy(c);
  if (st) return st;
  c->comm_aborted = false;
  if (world == 1 && !unique_id) { c->comm_rank = 0; c->comm_world = 1; return TMX_OK; }  // nothing to exchange, nothing to load
  // (world == 1 WITH an id makes a real one-rank communicator: the exchange then runs through RCCL -- a broadcast to itself -- which is
  // how the 1-GPU boxes exercise this path)
  {
    const std::string why = rccl_load();
    if (!why.empty()) return fail(c, TMX_ERR_RCCL, why);
  }
  HIPCK(c, hipSetDevice(c->cfg.device));
  RcclId id;
  std::memcpy(id.internal, unique_id, TMX_UNIQUE_ID_BYTES);
  void* comm = nullptr;
  const int rc = g_rccl.CommInitRank(&comm, (int)world, id, (int)rank);
  if (rc) return rccl_fail(c, "ncclCommInitRank", rc);
  c->comm = comm; c->comm_rank = rank; c->comm_world = world;
  c->comm_aborted = false;
  return TMX_OK;
}

int32_t tmx_comm_destroy(tmx_ctx* c) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (c->comm) {
    if (c->have_streams) { (void)hipSetDevice(c->cfg.device); (void)hipDeviceSynchronize(); }
    const int rc = g_rccl.CommDestroy ? g_rccl.CommDestroy(c->comm) : 0;
    c->comm = nullptr;
    if (rc) return rccl_fail(c, "ncclCommDestroy", rc);
  }
  c->comm_rank = 0; c->comm_world = 1;
  return TMX_OK;
}

int32_t tmx_comm_info(const tmx_ctx* c, uint32_t* rank, uint32_t* world) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (rank) *rank = c->comm_rank;
  if (world) *world = c->comm_world;
  return TMX_OK;
}

int32_t tmx_comm_abort(tmx_ctx* c) {
  if (!c) return TMX_ERR_BAD_ARG;
  comm_abort(c);
  return TMX_OK;
}

int32_t tmx_comm_sync(tmx_ctx* c, void* hip_stream, uint32_t timeout_ms) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (c->comm_aborted) return comm_usable(c);
  HIPCK(c, hipSetDevice(c->cfg.device));
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spin = 0;; spin++) {
    const hipError_t q = hipStreamQuery(s);
    if (q == hipSuccess) return TMX_OK;
    if (q != hipErrorNotReady) { (void)hipGetLastError(); comm_abort(c); return fail(c, TMX_ERR_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(q)); }
    (void)hipGetLastError();
    if (c->comm && g_rccl.CommGetAsyncError && (spin & 15) == 0) {
      int async_rc = 0;
      const int rc = g_rccl.CommGetAsyncError(c->comm, &async_rc);
      if (rc || async_rc) return rccl_fail_abort(c, "asynchronous error of the communicator (a peer aborted or died)", rc ? rc : async_rc);
    }
    if (timeout_ms) {
      const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
      if (ms >= (long long)timeout_ms) {
        comm_abort(c);
        return fail(c, TMX_ERR_RCCL, "tmx_comm_sync: the stream did not drain within " + std::to_string(timeout_ms) + " ms: communicator aborted");
      }
    }
    if (spin > 200) std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}

int32_t tmx_witness_batch_sharded_device(tmx_ctx* c, int32_t kind, uint32_t n_total, const void* d_proofs, const void* d_targets,
                                         const void* d_trusteds, void* d_out_elems, void* d_reports, uint32_t gather, void* hip_stream) {
  int32_t st = check_batch_args(c, kind, 0, d_proofs, d_targets, d_trusteds);
  if (st) return st;
  if (n_total == 0) return TMX_OK;
  // (a one-rank communicator made WITH an id exchanges through RCCL too: the guard is on the communicator, not on the world size)
  if (gather && (c->comm || c->comm_world > 1) && (!d_out_elems || !d_reports)) return fail(c, TMX_ERR_BAD_ARG, "gather needs the row and report buffers");
  uint64_t lo, hi;
  tmx_shard_range(n_total, c->comm_rank, c->comm_world, &lo, &hi);
  if (gather && (st = comm_usable(c))) return st;
  // (from here on a failure is LOCAL -- this rank's shard, this rank's context -- while the peers go on to the exchange: shard_fail)
  if (hi - lo > c->cfg.max_batch) { st = fail(c, TMX_ERR_CAPACITY, "this rank's shard exceeds the context's max_batch"); return gather ? shard_fail(c, st) : st; }
  const uint32_t n = c->cfg.n_max;
  const size_t row_bytes = (size_t)tmx_elem_stride(kind, n) * 8;
  auto at = [](const void* p, size_t off) { return p ? reinterpret_cast<const uint8_t*>(p) + off : nullptr; };
  if (hi > lo) {
    st = tmx_witness_batch_device(c, kind, (uint32_t)(hi - lo), at(d_proofs, lo * PR_STRIDE), at(d_targets, lo * n * VR_STRIDE),
                                  at(d_trusteds, lo * n * HR_STRIDE), const_cast<uint8_t*>(at(d_out_elems, lo * row_bytes)),
                                  const_cast<uint8_t*>(at(d_reports, lo * sizeof(tmx_report))), hip_stream);
    if (st) return gather ? shard_fail(c, st) : st;
  }
  if (!gather) return TMX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  if ((st = exchange_slices(c, d_out_elems, n_total, row_bytes, s))) return st;
  return exchange_slices(c, d_reports, n_total, sizeof(tmx_report), s);
}

int32_t tmx_witness_validator_sharded_device(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets,
                                             const void* d_trusteds, void* d_out_elems, void* d_reports, void* hip_stream) {
  int32_t st = check_batch_args(c, kind, n_proofs, d_proofs, d_targets, d_trusteds);
  if (st) return st;
  if (n_proofs == 0) return TMX_OK;
  if ((st = comm_usable(c))) return st;
  const uint64_t lanes = (uint64_t)n_proofs * c->cfg.n_max;
  uint64_t lo, hi;
  tmx_shard_range(lanes, c->comm_rank, c->comm_world, &lo, &hi);
  uint8_t* ed = reinterpret_cast<uint8_t*>(c->d_ed);
  if (hi > lo) {
    st = tmx_eddsa_lanes_device(c, (uint32_t)(hi - lo), reinterpret_cast<const uint8_t*>(d_targets) + lo * VR_STRIDE, ed + lo * ED_STRIDE, hip_stream);
    if (st) return shard_fail(c, st);
  }
  if ((st = exchange_slices(c, ed, lanes, ED_STRIDE, reinterpret_cast<hipStream_t>(hip_stream)))) return st;
  return tmx_finish_batch_device(c, kind, n_proofs, d_proofs, d_targets, d_trusteds, ed, d_out_elems, d_reports, hip_stream);
}

// ---- Level-2 trace rows across the ranks (north_star: "validators AND TRACE ROWS shard across the 8 GPUs ... with an RCCL all-gather").
// The rows are the one payload of this path that is big enough for xGMI to matter: 41 MB per proof at N = 128, 136 MB at N = 512.
int32_t tmx_trace_rows_sharded_device(tmx_ctx* c, int32_t kind, uint32_t n_total, const void* d_targets, const void* d_trusteds, void* d_trace_out,
                                      uint32_t sections, uint32_t gather, void* hip_stream) {
  if (!c || (kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP) || !d_targets || !d_trace_out) return TMX_ERR_BAD_ARG;
  if (n_total == 0) return TMX_OK;
  uint64_t lo, hi;
  tmx_shard_range(n_total, c->comm_rank, c->comm_world, &lo, &hi);
  const uint32_t n = c->cfg.n_max;
  const size_t row_bytes = (size_t)trace_elems((uint32_t)kind, n) * 8;
  auto at = [](const void* p, size_t off) { return p ? reinterpret_cast<const uint8_t*>(p) + off : nullptr; };
  if (gather) { const int32_t su = comm_usable(c); if (su) return su; }
  if (hi > lo) {  // the Level-1 records this reads are those of the rank's own shard: tmx_witness_batch_sharded_device of the same n_total came first
    int32_t st = tmx_trace_rows_device(c, kind, (uint32_t)(hi - lo), at(d_targets, lo * n * VR_STRIDE), at(d_trusteds, lo * n * HR_STRIDE),
                                       const_cast<uint8_t*>(at(d_trace_out, lo * row_bytes)), sections, hip_stream);
    if (st) return gather ? shard_fail(c, st) : st;
  }
  if (!gather) return TMX_OK;
  return exchange_slices(c, d_trace_out, n_total, row_bytes, reinterpret_cast<hipStream_t>(hip_stream));
}

int32_t tmx_trace_rows_validator_sharded_device(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_targets, const void* d_trusteds, void* d_trace_out,
                                                uint32_t sections, void* hip_stream) {
  if (!c || (kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP) || !d_targets || !d_trace_out) return TMX_ERR_BAD_ARG;
  if (n_proofs == 0) return TMX_OK;
  const uint32_t n = c->cfg.n_max;
  const uint64_t lanes = (uint64_t)n_proofs * n;
  uint64_t lo, hi;
  tmx_shard_range(lanes, c->comm_rank, c->comm_world, &lo, &hi);
  // the per-lane sections (ladders: 266 KB per lane, SHA-512: 23 KB) for this rank's lanes; the small per-proof sections on every rank
  int32_t st = comm_usable(c);
  if (st) return st;
  st = trace_rows_impl(c, kind, n_proofs, d_targets, d_trusteds, d_trace_out, sections, hip_stream, (uint32_t)lo, (uint32_t)(hi - lo));
  if (st) return shard_fail(c, st);
  if (!c->comm) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  uint8_t* out = reinterpret_cast<uint8_t*>(d_trace_out);
  const size_t row_bytes = (size_t)trace_elems((uint32_t)kind, n) * 8;
  struct Sec { uint32_t bit; size_t off, per_lane; };
  const Sec secs[2] = {{TMX_TRACE_LADDERS, 0, (size_t)2 * TR_LADDER_ROWS * TR_LADDER_ROW * 8},
                       {TMX_TRACE_SHA512, (size_t)n * 2 * TR_LADDER_ROWS * TR_LADDER_ROW * 8, (size_t)2 * 80 * TR_SHA512_ROW * 8}};
  for (const Sec& sc : secs) {
    if (!(sections & sc.bit)) continue;
    if (n_proofs == 1) {  // one proof: its lanes' slabs are contiguous -- the all-gather of SURVEY 8(e) when the lanes divide evenly
      if ((st = exchange_slices(c, out + sc.off, lanes, sc.per_lane, s))) return st;
      continue;
    }
    // several proofs: a rank's lanes are one run per proof it touches; every run is broadcast by its owner, grouped
    int rc = g_rccl.GroupStart(), in_group = 0;
    if (rc) return rccl_fail_abort(c, "ncclGroupStart", rc);
    for (uint32_t r = 0; r < c->comm_world; r++) {
      uint64_t rlo, rhi;
      tmx_shard_range(lanes, r, c->comm_world, &rlo, &rhi);
      for (uint64_t p = rlo / n; p < n_proofs && p * n < rhi; p++) {
        const uint64_t a = std::max<uint64_t>(rlo, p * n), b = std::min<uint64_t>(rhi, (p + 1) * n);
        if (b <= a) continue;
        uint8_t* ptr = out + p * row_bytes + sc.off + (a - p * n) * sc.per_lane;
        rc = g_rccl.Broadcast(ptr, ptr, (size_t)(b - a) * sc.per_lane, RCCL_UINT8, (int)r, c->comm, s);
        if (rc) { (void)g_rccl.GroupEnd(); return rccl_fail_abort(c, "ncclBroadcast", rc); }
        if (++in_group == 32) {  // (bounded groups: a group is one fused launch, and a thousand-entry group helps nobody)
          if ((rc = g_rccl.GroupEnd())) return rccl_fail_abort(c, "ncclGroupEnd", rc);
          if ((rc = g_rccl.GroupStart())) return rccl_fail_abort(c, "ncclGroupStart", rc);
          in_group = 0;
        }
      }
    }
    if ((rc = g_rccl.GroupEnd())) return rccl_fail_abort(c, "ncclGroupEnd", rc);
  }
  return TMX_OK;
}

}  // extern "C"

// ---- the commit pipeline on the device: section rows -> columns -> LDE -> Poseidon Merkle cap (include/tmx.h) ---------------------------
extern "C" {

int32_t tmx_trace_commit_shape(int32_t kind, uint32_t n, uint32_t section, uint32_t* log_rows, uint32_t* width) {
  if ((kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP) || n == 0 || n > TMX_N_MAX_LIMIT) return TMX_ERR_BAD_ARG;
  uint64_t off, rows;
  uint32_t w;
  if (!trace_section_geom((uint32_t)kind, n, section, &off, &rows, &w)) return TMX_ERR_BAD_ARG;
  uint32_t lg = 6;  // (the transpose moves 64 rows per workgroup)
  while (((uint64_t)1 << lg) < rows) lg++;
  if (log_rows) *log_rows = lg;
  if (width) *width = w;
  return TMX_OK;
}

int32_t tmx_trace_commit_device(tmx_ctx* c, int32_t kind, uint32_t n_proofs, uint32_t section, uint32_t log_blowup, uint32_t cap_height,
                                const void* d_trace_rows, uint64_t* d_cap, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  c->last_commit.valid = false;  // (set again at the end: a call that fails anywhere leaves nothing to open)
  if (!d_trace_rows || !d_cap || n_proofs == 0) return TMX_ERR_BAD_ARG;
  uint32_t log_n = 0, width = 0;
  if (tmx_trace_commit_shape(kind, c->cfg.n_max, section, &log_n, &width)) return fail(c, TMX_ERR_BAD_ARG, "section must be one row table of the trace block");
  const uint32_t log_m = log_n + log_blowup;
  if (log_m > TMX_NTT_MAX_LOG) return fail(c, TMX_ERR_CAPACITY, "log_rows + log_blowup exceeds TMX_NTT_MAX_LOG");
  if (cap_height > log_m) return fail(c, TMX_ERR_BAD_ARG, "cap_height exceeds the height of the tree");
  const uint64_t n_cols64 = (uint64_t)n_proofs * width;
  if (n_cols64 > 0xffffffffull) return fail(c, TMX_ERR_CAPACITY, "too many columns");
  const uint32_t n_cols = (uint32_t)n_cols64;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  uint64_t off, rows;
  uint32_t w;
  (void)trace_section_geom((uint32_t)kind, c->cfg.n_max, section, &off, &rows, &w);
  const size_t cols_b = ((size_t)n_cols << log_n) * 8, lde_b = ((size_t)n_cols << log_m) * 8;
  const size_t lev_b = (size_t)tmx_poseidon_merkle_digests(log_m, cap_height) * 32, want = cols_b + lde_b + lev_b;
  HIPCK(c, hipSetDevice(c->cfg.device));
  if (c->commit_bytes < want) {
    if (c->d_commit) { HIPCK(c, hipStreamSynchronize(s)); HIPCK(c, hipFree(c->d_commit)); c->d_commit = nullptr; c->commit_bytes = 0; }
    size_t free_b = 0, total_b = 0;
    // (the LDE's own scratch is twice the extended columns again: refuse what cannot fit instead of driving the device out of memory)
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && want + 2 * lde_b > free_b + c->ntt_tmp_bytes)
      return fail(c, TMX_ERR_CAPACITY, "commit pipeline needs " + std::to_string((want + 2 * lde_b) >> 20) + " MiB of scratch, " + std::to_string(free_b >> 20) + " MiB free");
    HIPCK(c, hipMalloc(&c->d_commit, want));
    c->commit_bytes = want;
  }
  for (auto& e : c->ev_commit)
    if (!e) HIPCK(c, hipEventCreate(&e));
  uint8_t* base = reinterpret_cast<uint8_t*>(c->d_commit);
  uint64_t* cols = reinterpret_cast<uint64_t*>(base);
  uint64_t* lde = reinterpret_cast<uint64_t*>(base + cols_b);
  uint64_t* levels = reinterpret_cast<uint64_t*>(base + cols_b + lde_b);
  HIPCK(c, hipEventRecord(c->ev_commit[0], s));
  int rc = launch_trace_to_columns(d_trace_rows, trace_elems((uint32_t)kind, c->cfg.n_max), off, rows, width, log_n, n_proofs, cols, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_trace_to_columns launch: ") + hipGetErrorString((hipError_t)rc));
  HIPCK(c, hipEventRecord(c->ev_commit[1], s));
  int32_t st = tmx_lde_goldilocks_device(c, log_n, log_blowup, n_cols, cols, lde, hip_stream);
  if (st) return st;
  HIPCK(c, hipEventRecord(c->ev_commit[2], s));
  st = tmx_poseidon_merkle_device(c, log_m, n_cols, lde, cap_height, levels, hip_stream);
  if (st) return st;
  const uint64_t n_dig = tmx_poseidon_merkle_digests(log_m, cap_height), n_cap = (uint64_t)1 << cap_height;
  HIPCK(c, hipMemcpyAsync(d_cap, levels + 4 * (n_dig - n_cap), n_cap * 32, hipMemcpyDeviceToDevice, s));
  HIPCK(c, hipEventRecord(c->ev_commit[3], s));
  c->last_commit = {true, log_m, n_cols, cap_height, cols_b, cols_b + lde_b, log_blowup, c->ntt_root, c->ntt_shift};
  return TMX_OK;
}

// the commit of a proof-sharded batch: every rank commits the columns of ITS proofs (their rows are already in its HBM: no row crosses a
// link), its cap lands in slot `rank` of d_caps, and ONE all-gather of the caps (16 digests each at cap_height 4: 512 B) leaves all of
// them on every rank -- the batch's commitment is the `world` caps, each over n_shard * width columns
int32_t tmx_trace_commit_sharded_device(tmx_ctx* c, int32_t kind, uint32_t n_total, uint32_t section, uint32_t log_blowup, uint32_t cap_height,
                                        const void* d_trace_rows, uint64_t* d_caps, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  c->last_commit.valid = false;
  if (!d_trace_rows || !d_caps || n_total == 0) return TMX_ERR_BAD_ARG;
  uint64_t lo, hi;
  tmx_shard_range(n_total, c->comm_rank, c->comm_world, &lo, &hi);
  const size_t row_bytes = (size_t)trace_elems((uint32_t)kind, c->cfg.n_max) * 8, cap_bytes = ((size_t)4 << cap_height) * 8;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  uint64_t* mine = d_caps + (size_t)c->comm_rank * (cap_bytes / 8);
  if (hi > lo) {
    int32_t st = comm_usable(c);
    if (st) return st;
    st = tmx_trace_commit_device(c, kind, (uint32_t)(hi - lo), section, log_blowup, cap_height, reinterpret_cast<const uint8_t*>(d_trace_rows) + lo * row_bytes,
                                 mine, hip_stream);
    if (st) return shard_fail(c, st);
  } else {
    HIPCK(c, hipMemsetAsync(mine, 0, cap_bytes, s));  // an empty shard commits to nothing: a zero cap (and leaves nothing to open)
  }
  const int32_t st = exchange_slices(c, d_caps, c->comm_world, cap_bytes, s);
  if (st) c->last_commit.valid = false;
  return st;
}

int32_t tmx_trace_commit_last_ms(tmx_ctx* c, float ms[3]) {
  if (!c || !ms) return TMX_ERR_BAD_ARG;
  if (!c->ev_commit[3]) return fail(c, TMX_ERR_BAD_ARG, "no tmx_trace_commit_device call yet");
  HIPCK(c, hipEventSynchronize(c->ev_commit[3]));
  for (int k = 0; k < 3; k++) HIPCK(c, hipEventElapsedTime(&ms[k], c->ev_commit[k], c->ev_commit[k + 1]));
  return TMX_OK;
}

}  // extern "C"

// ---- openings of a Poseidon Merkle tree: rows + paths, and their verification on the device (include/tmx.h) -------------------------------
constexpr uint32_t OPEN_MAX_QUERIES = 1u << 22;  // (one workgroup per query in k_merkle_open's first grid dimension)

static int32_t check_indices(tmx_ctx* c, uint32_t log_n, uint32_t n_queries, const uint64_t* h_idx) {
  if (n_queries == 0) return fail(c, TMX_ERR_BAD_ARG, "n_queries must be at least 1");
  if (n_queries > OPEN_MAX_QUERIES) return fail(c, TMX_ERR_BAD_ARG, "n_queries exceeds " + std::to_string(OPEN_MAX_QUERIES) + " per call");
  if (!h_idx) return fail(c, TMX_ERR_BAD_ARG, "h_indices is null");
  for (uint32_t q = 0; q < n_queries; q++)
    if (h_idx[q] >> log_n)
      return fail(c, TMX_ERR_BAD_ARG, "query " + std::to_string(q) + ": index " + std::to_string(h_idx[q]) + " is not below 2^" + std::to_string(log_n));
  return TMX_OK;
}

// the next slot of the index ring, holding a device copy of h_idx enqueued on s.  The caller records slot->ev on s behind the launch that
// reads it (index_release), whatever became of the launch: the slot is not written again before that event has completed.
static int32_t index_stage(tmx_ctx* c, uint32_t n, const uint64_t* h_idx, hipStream_t s, tmx_ctx::IdxSlot** out) {
  tmx_ctx::IdxSlot& sl = c->idx_ring[c->idx_next];
  HIPCK(c, hipSetDevice(c->cfg.device));
  if (!sl.ev) HIPCK(c, hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
  if (sl.used) HIPCK(c, hipEventSynchronize(sl.ev));
  sl.used = false;
  if (sl.cap < n) {
    if (sl.d) { HIPCK(c, hipFree(sl.d)); sl.d = nullptr; }
    if (sl.h) { HIPCK(c, hipHostFree(sl.h)); sl.h = nullptr; }
    sl.cap = 0;
    const uint64_t want = std::max<uint64_t>(n, 1024);
    HIPCK(c, hipHostMalloc(reinterpret_cast<void**>(&sl.h), want * 8, hipHostMallocDefault));
    HIPCK(c, hipMalloc(reinterpret_cast<void**>(&sl.d), want * 8));
    sl.cap = want;
  }
  std::memcpy(sl.h, h_idx, (size_t)n * 8);
  HIPCK(c, hipMemcpyAsync(sl.d, sl.h, (size_t)n * 8, hipMemcpyHostToDevice, s));
  sl.used = true;  // (from here on the copy may be pending: index_release records the event)
  c->idx_next = (c->idx_next + 1) % tmx_ctx::IDX_RING;
  *out = &sl;
  return TMX_OK;
}
static int32_t index_release(tmx_ctx* c, tmx_ctx::IdxSlot* sl, hipStream_t s, int launch_rc, const char* what) {
  const hipError_t e = hipEventRecord(sl->ev, s);
  if (e != hipSuccess) {  // (no event to wait for: drain the stream so that the slot is free when it comes round again)
    (void)hipStreamSynchronize(s);
    sl->used = false;
  }
  if (launch_rc) return fail(c, TMX_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString((hipError_t)launch_rc));
  if (e != hipSuccess) return fail(c, TMX_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
  return TMX_OK;
}

static int32_t merkle_open(tmx_ctx* c, uint32_t log_n, uint32_t n_cols, const uint64_t* d_cols, uint32_t cap_height, const uint64_t* d_levels,
                           uint32_t n_queries, const uint64_t* h_idx, uint64_t* d_rows, uint64_t* d_paths, void* hip_stream) {
  const uint32_t path_len = log_n - cap_height;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  tmx_ctx::IdxSlot* sl = nullptr;
  int32_t st = index_stage(c, n_queries, h_idx, s, &sl);
  if (st) return st;
  const char* split = std::getenv("TMX_OPEN_SPLIT");  // TMX_OPEN_SPLIT=1: rows and paths as two launches (times the one-launch form against it)
  const int rc = launch_merkle_open(log_n, n_cols, d_cols, path_len, d_levels, n_queries, sl->d, d_rows, d_paths, split && split[0] == '1', s);
  return index_release(c, sl, s, rc, "k_merkle_open");
}

extern "C" {

uint32_t tmx_poseidon_merkle_path_len(uint32_t log_n, uint32_t cap_height) {
  if (log_n > 30 || cap_height > log_n) return 0;
  return log_n - cap_height;
}

int32_t tmx_poseidon_merkle_open_device(tmx_ctx* c, uint32_t log_n, uint32_t n_cols, const uint64_t* d_cols, uint32_t cap_height,
                                        const uint64_t* d_levels, uint32_t n_queries, const uint64_t* h_indices, uint64_t* d_rows,
                                        uint64_t* d_paths, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (log_n > 30 || cap_height > log_n) return fail(c, TMX_ERR_BAD_ARG, "cap_height must not exceed log_n (<= 30)");
  if (!d_cols || !d_levels || !d_rows || n_cols == 0) return fail(c, TMX_ERR_BAD_ARG, "d_cols, d_levels and d_rows must be set and n_cols >= 1");
  if (!d_paths && log_n > cap_height) return fail(c, TMX_ERR_BAD_ARG, "d_paths is null but the paths are not empty");
  int32_t st = check_indices(c, log_n, n_queries, h_indices);
  if (st) return st;
  return merkle_open(c, log_n, n_cols, d_cols, cap_height, d_levels, n_queries, h_indices, d_rows, d_paths, hip_stream);
}

int32_t tmx_trace_commit_last_shape(const tmx_ctx* c, uint32_t* log_rows_ext, uint32_t* n_cols, uint32_t* cap_height) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (!c->last_commit.valid)
    return fail(const_cast<tmx_ctx*>(c), TMX_ERR_BAD_ARG, "no commit to open: no tmx_trace_commit_device call has completed since the context was created or since the last failed or empty-shard commit");
  if (log_rows_ext) *log_rows_ext = c->last_commit.log_m;
  if (n_cols) *n_cols = c->last_commit.n_cols;
  if (cap_height) *cap_height = c->last_commit.cap_height;
  return TMX_OK;
}

int32_t tmx_trace_commit_open_device(tmx_ctx* c, uint32_t n_queries, const uint64_t* h_indices, uint64_t* d_rows, uint64_t* d_paths,
                                     void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = tmx_trace_commit_last_shape(c, nullptr, nullptr, nullptr);
  if (st) return st;
  const tmx_ctx::CommitRec r = c->last_commit;
  if (!d_rows) return fail(c, TMX_ERR_BAD_ARG, "d_rows is null");
  if (!d_paths && r.log_m > r.cap_height) return fail(c, TMX_ERR_BAD_ARG, "d_paths is null but the paths are not empty");
  st = check_indices(c, r.log_m, n_queries, h_indices);
  if (st) return st;
  const uint8_t* base = reinterpret_cast<const uint8_t*>(c->d_commit);
  return merkle_open(c, r.log_m, r.n_cols, reinterpret_cast<const uint64_t*>(base + r.lde_off), r.cap_height,
                     reinterpret_cast<const uint64_t*>(base + r.lev_off), n_queries, h_indices, d_rows, d_paths, hip_stream);
}

int32_t tmx_poseidon_merkle_verify_device(tmx_ctx* c, uint32_t log_n, uint32_t n_cols, uint32_t cap_height, const uint64_t* d_cap,
                                          uint32_t n_queries, const uint64_t* h_indices, const uint64_t* d_rows, const uint64_t* d_paths,
                                          uint32_t* d_ok, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (log_n > 30 || cap_height > log_n) return fail(c, TMX_ERR_BAD_ARG, "cap_height must not exceed log_n (<= 30)");
  if (!d_cap || !d_rows || !d_ok || n_cols == 0) return fail(c, TMX_ERR_BAD_ARG, "d_cap, d_rows and d_ok must be set and n_cols >= 1");
  if (!d_paths && log_n > cap_height) return fail(c, TMX_ERR_BAD_ARG, "d_paths is null but the paths are not empty");
  int32_t st = check_indices(c, log_n, n_queries, h_indices);
  if (st) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCK(c, hipSetDevice(c->cfg.device));
  st = poseidon_ready(c, s);
  if (st) return st;
  tmx_ctx::IdxSlot* sl = nullptr;
  st = index_stage(c, n_queries, h_indices, s, &sl);
  if (st) return st;
  const int rc = launch_merkle_verify(c->d_pos_consts, c->pos_mode, n_cols, log_n - cap_height, n_queries, d_cap, sl->d, d_rows, d_paths, d_ok, s);
  return index_release(c, sl, s, rc, "k_merkle_verify");
}

}  // extern "C"

// ---- a batched FRI low-degree proof over committed columns (include/tmx.h "a batched FRI low-degree proof") ---------------------------------
static int32_t fri_check(tmx_ctx* c, const tmx_fri_params* p) {
  auto bad = [&](const char* why) { return c ? fail(c, TMX_ERR_BAD_ARG, why) : TMX_ERR_BAD_ARG; };
  if (!p) return bad("params is null");
  if (p->log_blowup < 1 || p->log_blowup > 6) return bad("log_blowup must be 1 .. 6");
  if (p->log_n <= p->log_blowup || p->log_n > 28) return bad("log_n must exceed log_blowup and be at most 28");
  if (p->n_cols < 1) return bad("n_cols must be at least 1");
  if (p->cap_height > p->log_n) return bad("cap_height must not exceed log_n");
  if (p->arity_bits < 1 || p->arity_bits > 4) return bad("arity_bits must be 1 .. 4");
  if (p->final_log_max > 8 || p->final_log_max + p->log_blowup > 12) return bad("final_log_max must be at most 8 and final_log_max + log_blowup at most 12");
  if (p->n_queries < 1 || p->n_queries > FRI_MAX_QUERIES) return bad("n_queries must be 1 .. 256");
  if (p->reserved) return bad("reserved must be 0");
  return TMX_OK;
}

static void fri_layout(const tmx_fri_params& p, tmx_fri_layout& L) {
  std::memset(&L, 0, sizeof L);
  uint32_t d = p.log_n - p.log_blowup;
  while (d > p.final_log_max) {
    const uint32_t b = std::min(p.arity_bits, d - p.final_log_max);
    L.layer_bits[L.n_layers++] = b;
    d -= b;
  }
  L.final_log = d;
  uint64_t w = 0;
  uint32_t lg = p.log_n;
  for (uint32_t l = 0; l < L.n_layers; l++) {
    lg -= L.layer_bits[l];
    L.layer_cap_height[l] = std::min(p.cap_height, lg);
    L.off_caps[l] = w;
    w += 4ull << L.layer_cap_height[l];
  }
  L.off_final = w; w += 2ull << L.final_log;
  L.off_indices = w; w += p.n_queries;
  L.off_init_rows = w; w += (uint64_t)p.n_queries * p.n_cols;
  L.off_init_paths = w; w += (uint64_t)p.n_queries * (p.log_n - p.cap_height) * 4;
  lg = p.log_n;
  for (uint32_t l = 0; l < L.n_layers; l++) {
    lg -= L.layer_bits[l];
    L.off_rows[l] = w; w += (uint64_t)p.n_queries * (2ull << L.layer_bits[l]);
    L.off_paths[l] = w; w += (uint64_t)p.n_queries * (lg - L.layer_cap_height[l]) * 4;
  }
  L.words = w;
}

static FriGeom fri_geom(const tmx_fri_params& p, const tmx_fri_layout& L, uint64_t root_2_32, uint64_t shift) {
  const uint64_t P = 0xffffffff00000001ull;
  auto inv = [&](uint64_t x) { return gl_pow_host(x, P - 2); };
  FriGeom G;
  std::memset(&G, 0, sizeof G);
  const uint32_t obs[8] = {p.log_n, p.n_cols, p.cap_height, p.log_blowup, p.arity_bits, p.final_log_max, p.n_queries, 0};
  std::memcpy(G.params, obs, sizeof obs);
  G.log_n = p.log_n; G.n_cols = p.n_cols; G.cap_height = p.cap_height; G.n_queries = p.n_queries;
  G.n_layers = L.n_layers; G.final_log = L.final_log;
  uint64_t s = shift % P, w = gl_pow_host(root_2_32, 1ull << (32 - p.log_n));
  G.s0 = s; G.w0 = w; G.omega_n = gl_pow_host(w, 1ull << p.log_blowup);
  uint32_t lg = p.log_n;
  for (uint32_t l = 0; l < L.n_layers; l++) {
    lg -= L.layer_bits[l];
    G.bits[l] = L.layer_bits[l]; G.cap_h[l] = L.layer_cap_height[l];
    G.s_inv[l] = inv(s); G.w_inv[l] = inv(w); G.g[l] = gl_pow_host(G.w_inv[l], 1ull << lg);
    s = gl_pow_host(s, 1ull << L.layer_bits[l]); w = gl_pow_host(w, 1ull << L.layer_bits[l]);
    G.off_caps[l] = L.off_caps[l]; G.off_rows[l] = L.off_rows[l]; G.off_paths[l] = L.off_paths[l];
  }
  G.s_fin = s; G.w_fin = w; G.s_fin_inv = inv(s); G.w_fin_inv = inv(w); G.m_fin_inv = inv(1ull << lg);
  G.off_final = L.off_final; G.off_indices = L.off_indices; G.off_init_rows = L.off_init_rows; G.off_init_paths = L.off_init_paths;
  return G;
}

// The columns a DEEP prove evaluates at zeta and zeta omega_N: N = 2^(log_n - log_blowup) words per column, word j of column c at
// cols[(c << log_col) + (j << stride_log)], on the coset s <omega_N>.  The extended columns themselves (stride B, s = the domain's shift)
// or the commit's pre-LDE columns (stride 1, s = 1).
struct DeepSrc { const uint64_t* cols; uint32_t log_col, stride_log; uint64_t s; };

static uint32_t deep_log_r(uint32_t n_cols) {
  uint32_t lr = 0;
  while ((1ull << lr) < n_cols) lr++;
  return lr;
}

// cols / levels: the committed columns and their tree; (root_2_32, shift): the domain they were extended on.  Validated by the caller.
// deep: null for a plain FRI prove; else the DEEP prove: the openings section first, then the FRI proof of the DEEP quotients.  Everything
// after layer 0 is the same for both.  pow_bits: 0, or the grinding variant of either: the transcript's last phase in two halves around the
// search, and the nonce word behind the FRI part.
static int32_t fri_prove(tmx_ctx* c, const tmx_fri_params& p, const uint64_t* cols, const uint64_t* levels, uint64_t root_2_32, uint64_t shift,
                         uint64_t* proof, void* hip_stream, const DeepSrc* deep = nullptr, uint32_t pow_bits = 0) {
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  tmx_fri_layout L;
  fri_layout(p, L);
  FriGeom G = fri_geom(p, L, root_2_32, shift);
  const uint32_t log_r = deep ? deep_log_r(p.n_cols) : 0, log_sub = p.log_n - p.log_blowup;
  uint64_t* open = proof;
  if (deep) {
    G.deep = 1;
    G.log_r = log_r;
    proof += 4ull << log_r;  // (the FRI part: every offset of the layout shifted by the openings section)
  }
  G.pow_bits = pow_bits;
  G.off_nonce = L.words;
  HIPCK(c, hipSetDevice(c->cfg.device));
  int32_t st = poseidon_ready(c, s);
  if (st) return st;
  // scratch (u64 words): transcript state 32 | challenges 64 | degree flag 8 | alpha powers | leaf indices | layers 0 .. L | layer trees
  const uint64_t nq = p.n_queries;
  uint64_t at = 104;
  const uint64_t o_apow = at; at += 2ull * p.n_cols;
  const uint64_t o_qidx = at; at += L.n_layers * nq;
  uint64_t o_layer[FRI_MAX_LAYERS + 1], o_lev[FRI_MAX_LAYERS];
  uint32_t lg = p.log_n;
  for (uint32_t l = 0; l <= L.n_layers; l++) {
    o_layer[l] = at; at += 2ull << lg;
    if (l < L.n_layers) lg -= L.layer_bits[l];
  }
  lg = p.log_n;
  for (uint32_t l = 0; l < L.n_layers; l++) {
    lg -= L.layer_bits[l];
    o_lev[l] = at; at += 4 * tmx_poseidon_merkle_digests(lg, L.layer_cap_height[l]);
  }
  // DEEP: weights [N][2] | partial sums [tiles][n_cols][4] | openings tree | Y_0, Y_1, alpha^n
  uint64_t o_wt = 0, o_part = 0, o_olev = 0, o_y = 0;
  if (deep) {
    o_wt = at; at += 2ull << log_sub;
    o_part = at; at += deep_eval_tiles(log_sub) * p.n_cols * 4;
    o_olev = at; at += 4 * tmx_poseidon_merkle_digests(log_r, 0);
    o_y = at; at += 8;
  }
  if (c->fri_bytes < at * 8) {
    if (c->d_fri) { HIPCK(c, hipDeviceSynchronize()); HIPCK(c, hipFree(c->d_fri)); c->d_fri = nullptr; c->fri_bytes = 0; }
    HIPCK(c, hipMalloc(&c->d_fri, at * 8));
    c->fri_bytes = at * 8;
  }
  for (auto& e : c->ev_fri)
    if (!e) HIPCK(c, hipEventCreate(&e));
  c->fri_valid = false;
  c->fri_deep = deep != nullptr;
  c->fri_pow_bits = pow_bits;
  uint64_t* W = reinterpret_cast<uint64_t*>(c->d_fri);
  uint64_t *state = W, *chal = W + 32, *apow = W + o_apow, *qidx = W + o_qidx;
  c->fri_flag_off = 96 * 8;
  const uint64_t* commit_cap = levels + 4 * (tmx_poseidon_merkle_digests(p.log_n, p.cap_height) - (1ull << p.cap_height));
  auto launched = [&](int rc, const char* what) { return rc ? fail(c, TMX_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString((hipError_t)rc)) : TMX_OK; };

  HIPCK(c, hipEventRecord(c->ev_fri[0], s));
  if (!deep) {
    if ((st = launched(launch_fri_transcript(c->d_pos_consts, c->pos_mode, G, 0, 0, commit_cap, proof, state, chal, qidx, s), "k_fri_transcript"))) return st;
    if ((st = launched(launch_fri_alpha_powers(p.n_cols, chal, apow, s), "k_fri_alpha_powers"))) return st;
    if ((st = launched(launch_fri_combine(p.log_n, p.n_cols, cols, apow, W + o_layer[0], s), "k_fri_combine"))) return st;
  } else {
    // zeta; the openings (weights, the pass over the columns, the tiles added into the proof's planes); their root -> alpha; layer 0 as
    // for FRI, then rewritten into the DEEP quotient
    const uint64_t P = 0xffffffff00000001ull, s_n = gl_pow_host(deep->s, 1ull << log_sub);
    const uint64_t k_inv = gl_pow_host((uint64_t)(((unsigned __int128)(1ull << log_sub) * s_n) % P), P - 2);
    const uint64_t* zeta = chal + FRI_ZETA_AT;
    const uint64_t* root = W + o_olev + 4 * (tmx_poseidon_merkle_digests(log_r, 0) - 1);
    if ((st = launched(launch_fri_transcript(c->d_pos_consts, c->pos_mode, G, 3, 0, commit_cap, proof, state, chal, qidx, s), "k_fri_transcript"))) return st;
    if ((st = launched(launch_deep_weights(log_sub, deep->s, G.omega_n, s_n, k_inv, zeta, W + o_wt, s), "k_deep_weights"))) return st;
    if ((st = launched(launch_deep_eval(log_sub, deep->log_col, deep->stride_log, p.n_cols, deep->cols, W + o_wt, W + o_part, s), "k_deep_eval"))) return st;
    if ((st = launched(launch_deep_open(log_sub, p.n_cols, log_r, W + o_part, open, s), "k_deep_open"))) return st;
    if ((st = tmx_poseidon_merkle_device(c, log_r, 4, open, 0, W + o_olev, hip_stream))) return st;
    if ((st = launched(launch_fri_transcript(c->d_pos_consts, c->pos_mode, G, 4, 0, root, proof, state, chal, qidx, s), "k_fri_transcript"))) return st;
    if ((st = launched(launch_fri_alpha_powers(p.n_cols, chal, apow, s), "k_fri_alpha_powers"))) return st;
    if ((st = launched(launch_fri_combine(p.log_n, p.n_cols, cols, apow, W + o_layer[0], s), "k_fri_combine"))) return st;
    if ((st = launched(launch_deep_y(p.n_cols, log_r, open, apow, chal, W + o_y, s), "k_deep_y"))) return st;
    if ((st = launched(launch_deep_quotient(p.log_n, G.s0, G.w0, G.omega_n, zeta, W + o_y, W + o_layer[0], s), "k_deep_quotient"))) return st;
  }
  HIPCK(c, hipEventRecord(c->ev_fri[1], s));
  lg = p.log_n;
  for (uint32_t l = 0; l < L.n_layers; l++) {
    const uint32_t b = L.layer_bits[l], h = L.layer_cap_height[l];
    lg -= b;
    st = tmx_poseidon_merkle_device(c, lg, 2u << b, W + o_layer[l], h, W + o_lev[l], hip_stream);
    if (st) return st;
    const uint64_t nd = tmx_poseidon_merkle_digests(lg, h);
    HIPCK(c, hipMemcpyAsync(proof + L.off_caps[l], W + o_lev[l] + 4 * (nd - (1ull << h)), 32ull << h, hipMemcpyDeviceToDevice, s));
    if ((st = launched(launch_fri_transcript(c->d_pos_consts, c->pos_mode, G, 1, l, commit_cap, proof, state, chal, qidx, s), "k_fri_transcript"))) return st;
    if ((st = launched(launch_fri_fold(lg, b, G.s_inv[l], G.w_inv[l], G.g[l], chal + 2 + 2 * l, W + o_layer[l], W + o_layer[l + 1], s), "k_fri_fold")))
      return st;
  }
  HIPCK(c, hipEventRecord(c->ev_fri[2], s));
  if ((st = launched(launch_fri_final(lg, L.final_log, G.w_fin_inv, G.s_fin_inv, G.m_fin_inv, W + o_layer[L.n_layers], proof + L.off_final, W + 96, s),
                     "k_fri_final")))
    return st;
  if (!pow_bits) {
    if ((st = launched(launch_fri_transcript(c->d_pos_consts, c->pos_mode, G, 2, 0, commit_cap, proof, state, chal, qidx, s), "k_fri_transcript"))) return st;
  } else {
    if ((st = launched(launch_fri_transcript(c->d_pos_consts, c->pos_mode, G, 5, 0, commit_cap, proof, state, chal, qidx, s), "k_fri_transcript"))) return st;
    if ((st = launched(launch_fri_grind(c->d_pos_consts, c->pos_mode, pow_bits, state, chal + FRI_POW_AT, s), "k_fri_grind"))) return st;
    if ((st = launched(launch_fri_transcript(c->d_pos_consts, c->pos_mode, G, 6, 0, commit_cap, proof, state, chal, qidx, s), "k_fri_transcript"))) return st;
  }
  HIPCK(c, hipEventRecord(c->ev_fri[3], s));
  // the openings, with the indices the transcript drew (device side): the commit's rows and paths, then every layer's leaf
  if ((st = launched(launch_merkle_open(p.log_n, p.n_cols, cols, p.log_n - p.cap_height, levels, p.n_queries, proof + L.off_indices,
                                        proof + L.off_init_rows, proof + L.off_init_paths, false, s), "k_merkle_open")))
    return st;
  lg = p.log_n;
  for (uint32_t l = 0; l < L.n_layers; l++) {
    lg -= L.layer_bits[l];
    if ((st = launched(launch_merkle_open(lg, 2u << L.layer_bits[l], W + o_layer[l], lg - L.layer_cap_height[l], W + o_lev[l], p.n_queries,
                                          qidx + l * nq, proof + L.off_rows[l], proof + L.off_paths[l], false, s), "k_merkle_open")))
      return st;
  }
  HIPCK(c, hipEventRecord(c->ev_fri[4], s));
  c->fri_valid = true;
  return TMX_OK;
}

// The verifier of all four proofs (parameters validated by the caller).  deep: the openings tree goes into the context's verifier scratch
// first and the FRI part sits behind the openings section; pow_bits: the nonce word sits behind the FRI part.
static int32_t fri_verify(tmx_ctx* c, const tmx_fri_params& p, bool deep, uint32_t pow_bits, const uint64_t* d_cap, const uint64_t* d_proof,
                          uint32_t* d_ok, void* hip_stream) {
  if (!d_cap || !d_proof || !d_ok) return fail(c, TMX_ERR_BAD_ARG, "d_cap, d_proof and d_ok must be set");
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCK(c, hipSetDevice(c->cfg.device));
  int32_t st = poseidon_ready(c, s);
  if (st) return st;
  tmx_fri_layout L;
  fri_layout(p, L);
  FriGeom G = fri_geom(p, L, c->ntt_root, c->ntt_shift);
  G.pow_bits = pow_bits;
  G.off_nonce = L.words;
  const uint64_t *open = nullptr, *root = nullptr;
  if (deep) {
    const uint32_t log_r = deep_log_r(p.n_cols);
    const uint64_t nd = tmx_poseidon_merkle_digests(log_r, 0);
    if (c->deepv_bytes < nd * 32) {
      if (c->d_deepv) { HIPCK(c, hipDeviceSynchronize()); HIPCK(c, hipFree(c->d_deepv)); c->d_deepv = nullptr; c->deepv_bytes = 0; }
      HIPCK(c, hipMalloc(&c->d_deepv, nd * 32));
      c->deepv_bytes = nd * 32;
    }
    uint64_t* lev = reinterpret_cast<uint64_t*>(c->d_deepv);
    if ((st = tmx_poseidon_merkle_device(c, log_r, 4, d_proof, 0, lev, hip_stream))) return st;
    G.deep = 1;
    G.log_r = log_r;
    open = d_proof;
    root = lev + 4 * (nd - 1);
    d_proof += 4ull << log_r;
  }
  const int rc = launch_fri_verify(c->d_pos_consts, c->pos_mode, G, d_cap, d_proof, open, root, d_ok, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_fri_verify launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

extern "C" {

int32_t tmx_fri_layout_of(const tmx_fri_params* p, tmx_fri_layout* out) {
  if (!out || fri_check(nullptr, p)) return TMX_ERR_BAD_ARG;
  fri_layout(*p, *out);
  return TMX_OK;
}

int32_t tmx_fri_prove_device(tmx_ctx* c, const tmx_fri_params* p, const uint64_t* d_cols, const uint64_t* d_levels, uint64_t* d_proof, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = fri_check(c, p);
  if (st) return st;
  if (!d_cols || !d_levels || !d_proof) return fail(c, TMX_ERR_BAD_ARG, "d_cols, d_levels and d_proof must be set");
  return fri_prove(c, *p, d_cols, d_levels, c->ntt_root, c->ntt_shift, d_proof, hip_stream);
}

int32_t tmx_trace_commit_fri_device(tmx_ctx* c, const tmx_fri_params* p, uint64_t* d_proof, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = fri_check(c, p);
  if (st) return st;
  st = tmx_trace_commit_last_shape(c, nullptr, nullptr, nullptr);
  if (st) return st;
  const tmx_ctx::CommitRec r = c->last_commit;
  if (p->log_n != r.log_m || p->n_cols != r.n_cols || p->cap_height != r.cap_height || p->log_blowup != r.log_blowup)
    return fail(c, TMX_ERR_BAD_ARG, "FRI parameters do not match the last commit: log_n " + std::to_string(r.log_m) + ", n_cols " + std::to_string(r.n_cols) +
                                        ", cap_height " + std::to_string(r.cap_height) + ", log_blowup " + std::to_string(r.log_blowup));
  if (!d_proof) return fail(c, TMX_ERR_BAD_ARG, "d_proof is null");
  const uint8_t* base = reinterpret_cast<const uint8_t*>(c->d_commit);
  return fri_prove(c, *p, reinterpret_cast<const uint64_t*>(base + r.lde_off), reinterpret_cast<const uint64_t*>(base + r.lev_off), r.root, r.shift,
                   d_proof, hip_stream);
}

int32_t tmx_fri_verify_device(tmx_ctx* c, const tmx_fri_params* p, const uint64_t* d_cap, const uint64_t* d_proof, uint32_t* d_ok, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = fri_check(c, p);
  if (st) return st;
  return fri_verify(c, *p, false, 0, d_cap, d_proof, d_ok, hip_stream);
}

int32_t tmx_fri_last_degree_ok(tmx_ctx* c) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (!c->fri_valid) return fail(c, TMX_ERR_BAD_ARG, "no FRI prove has completed on this context");
  HIPCK(c, hipSetDevice(c->cfg.device));
  HIPCK(c, hipEventSynchronize(c->ev_fri[4]));
  uint32_t flag = 0;
  HIPCK(c, hipMemcpy(&flag, reinterpret_cast<uint8_t*>(c->d_fri) + c->fri_flag_off, 4, hipMemcpyDeviceToHost));
  return flag ? 1 : 0;
}

int32_t tmx_fri_last_ms(tmx_ctx* c, float ms[4]) {
  if (!c || !ms) return TMX_ERR_BAD_ARG;
  if (!c->fri_valid) return fail(c, TMX_ERR_BAD_ARG, "no FRI prove has completed on this context");
  HIPCK(c, hipEventSynchronize(c->ev_fri[4]));
  for (int k = 0; k < 4; k++) HIPCK(c, hipEventElapsedTime(&ms[k], c->ev_fri[k], c->ev_fri[k + 1]));
  return TMX_OK;
}

// ---- DEEP: the committed columns opened at zeta and zeta omega_N (include/tmx.h "out-of-domain openings") --------------------------------
uint64_t tmx_deep_openings_words(uint32_t n_cols) {
  if (n_cols == 0 || n_cols > TMX_DEEP_MAX_COLS) return 0;
  return 4ull << deep_log_r(n_cols);
}

static int32_t deep_check(tmx_ctx* c, const tmx_fri_params* p) {
  int32_t st = fri_check(c, p);
  if (st) return st;
  if (p->n_cols > TMX_DEEP_MAX_COLS) return fail(c, TMX_ERR_BAD_ARG, "n_cols must be at most 2^24 for a DEEP proof");
  return TMX_OK;
}

int32_t tmx_deep_prove_device(tmx_ctx* c, const tmx_fri_params* p, const uint64_t* d_cols, const uint64_t* d_levels, uint64_t* d_proof, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = deep_check(c, p);
  if (st) return st;
  if (!d_cols || !d_levels || !d_proof) return fail(c, TMX_ERR_BAD_ARG, "d_cols, d_levels and d_proof must be set");
  const DeepSrc src = {d_cols, p->log_n, p->log_blowup, c->ntt_shift % 0xffffffff00000001ull};
  return fri_prove(c, *p, d_cols, d_levels, c->ntt_root, c->ntt_shift, d_proof, hip_stream, &src);
}

int32_t tmx_trace_commit_deep_device(tmx_ctx* c, const tmx_fri_params* p, uint64_t* d_proof, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = deep_check(c, p);
  if (st) return st;
  st = tmx_trace_commit_last_shape(c, nullptr, nullptr, nullptr);
  if (st) return st;
  const tmx_ctx::CommitRec r = c->last_commit;
  if (p->log_n != r.log_m || p->n_cols != r.n_cols || p->cap_height != r.cap_height || p->log_blowup != r.log_blowup)
    return fail(c, TMX_ERR_BAD_ARG, "DEEP parameters do not match the last commit: log_n " + std::to_string(r.log_m) + ", n_cols " + std::to_string(r.n_cols) +
                                        ", cap_height " + std::to_string(r.cap_height) + ", log_blowup " + std::to_string(r.log_blowup));
  if (!d_proof) return fail(c, TMX_ERR_BAD_ARG, "d_proof is null");
  const uint8_t* base = reinterpret_cast<const uint8_t*>(c->d_commit);
  // the openings read the pre-LDE columns at offset 0 of the commit scratch (k_trace_to_columns: n_cols x N, on the subgroup itself)
  const DeepSrc src = {reinterpret_cast<const uint64_t*>(base), r.log_m - r.log_blowup, 0, 1};
  return fri_prove(c, *p, reinterpret_cast<const uint64_t*>(base + r.lde_off), reinterpret_cast<const uint64_t*>(base + r.lev_off), r.root, r.shift,
                   d_proof, hip_stream, &src);
}

int32_t tmx_deep_verify_device(tmx_ctx* c, const tmx_fri_params* p, const uint64_t* d_cap, const uint64_t* d_proof, uint32_t* d_ok, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = deep_check(c, p);
  if (st) return st;
  return fri_verify(c, *p, true, 0, d_cap, d_proof, d_ok, hip_stream);
}

int32_t tmx_deep_last_zeta(tmx_ctx* c, uint64_t z[2]) {
  if (!c || !z) return TMX_ERR_BAD_ARG;
  if (!c->fri_valid || !c->fri_deep) return fail(c, TMX_ERR_BAD_ARG, "the last prove of this context was not a DEEP prove");
  HIPCK(c, hipSetDevice(c->cfg.device));
  HIPCK(c, hipEventSynchronize(c->ev_fri[4]));
  HIPCK(c, hipMemcpy(z, reinterpret_cast<uint64_t*>(c->d_fri) + 32 + FRI_ZETA_AT, 16, hipMemcpyDeviceToHost));
  return TMX_OK;
}

// ---- proof of work: the grinding variants of both proofs (include/tmx.h "proof of work") ---------------------------------------------------
static int32_t pow_check(tmx_ctx* c, const tmx_pow_params* pp) {
  auto bad = [&](const char* why) { return c ? fail(c, TMX_ERR_BAD_ARG, why) : TMX_ERR_BAD_ARG; };
  if (!pp) return bad("params is null");
  int32_t st = fri_check(c, &pp->fri);
  if (st) return st;
  if (pp->deep > 1) return bad("deep must be 0 or 1");
  if (pp->deep && pp->fri.n_cols > TMX_DEEP_MAX_COLS) return bad("n_cols must be at most 2^24 for a DEEP proof");
  if (pp->pow_bits < 1 || pp->pow_bits > FRI_POW_MAX_BITS) return bad("pow_bits must be 1 .. 24");
  return TMX_OK;
}

uint64_t tmx_pow_proof_words(const tmx_pow_params* pp) {
  if (pow_check(nullptr, pp)) return 0;
  tmx_fri_layout L;
  fri_layout(pp->fri, L);
  return L.words + 1 + (pp->deep ? tmx_deep_openings_words(pp->fri.n_cols) : 0);
}

int32_t tmx_pow_prove_device(tmx_ctx* c, const tmx_pow_params* pp, const uint64_t* d_cols, const uint64_t* d_levels, uint64_t* d_proof,
                             void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = pow_check(c, pp);
  if (st) return st;
  if (!d_cols || !d_levels || !d_proof) return fail(c, TMX_ERR_BAD_ARG, "d_cols, d_levels and d_proof must be set");
  const tmx_fri_params& p = pp->fri;
  const DeepSrc src = {d_cols, p.log_n, p.log_blowup, c->ntt_shift % 0xffffffff00000001ull};
  return fri_prove(c, p, d_cols, d_levels, c->ntt_root, c->ntt_shift, d_proof, hip_stream, pp->deep ? &src : nullptr, pp->pow_bits);
}

int32_t tmx_trace_commit_pow_device(tmx_ctx* c, const tmx_pow_params* pp, uint64_t* d_proof, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = pow_check(c, pp);
  if (st) return st;
  st = tmx_trace_commit_last_shape(c, nullptr, nullptr, nullptr);
  if (st) return st;
  const tmx_fri_params& p = pp->fri;
  const tmx_ctx::CommitRec r = c->last_commit;
  if (p.log_n != r.log_m || p.n_cols != r.n_cols || p.cap_height != r.cap_height || p.log_blowup != r.log_blowup)
    return fail(c, TMX_ERR_BAD_ARG, "proof parameters do not match the last commit: log_n " + std::to_string(r.log_m) + ", n_cols " + std::to_string(r.n_cols) +
                                        ", cap_height " + std::to_string(r.cap_height) + ", log_blowup " + std::to_string(r.log_blowup));
  if (!d_proof) return fail(c, TMX_ERR_BAD_ARG, "d_proof is null");
  const uint8_t* base = reinterpret_cast<const uint8_t*>(c->d_commit);
  const DeepSrc src = {reinterpret_cast<const uint64_t*>(base), r.log_m - r.log_blowup, 0, 1};  // (as tmx_trace_commit_deep_device)
  return fri_prove(c, p, reinterpret_cast<const uint64_t*>(base + r.lde_off), reinterpret_cast<const uint64_t*>(base + r.lev_off), r.root, r.shift,
                   d_proof, hip_stream, pp->deep ? &src : nullptr, pp->pow_bits);
}

int32_t tmx_pow_verify_device(tmx_ctx* c, const tmx_pow_params* pp, const uint64_t* d_cap, const uint64_t* d_proof, uint32_t* d_ok, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = pow_check(c, pp);
  if (st) return st;
  return fri_verify(c, pp->fri, pp->deep != 0, pp->pow_bits, d_cap, d_proof, d_ok, hip_stream);
}

int32_t tmx_pow_last(tmx_ctx* c, uint64_t* nonce, uint64_t* tried) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (!c->fri_valid || !c->fri_pow_bits) return fail(c, TMX_ERR_BAD_ARG, "the last prove of this context was not a grinding prove");
  HIPCK(c, hipSetDevice(c->cfg.device));
  HIPCK(c, hipEventSynchronize(c->ev_fri[4]));
  uint64_t w[2] = {0, 0};
  HIPCK(c, hipMemcpy(w, reinterpret_cast<uint64_t*>(c->d_fri) + 32 + FRI_POW_AT, 16, hipMemcpyDeviceToHost));
  if (nonce) *nonce = w[0];
  if (tried) *tried = w[1];
  if (w[0] == ~0ull)
    return fail(c, TMX_ERR_CAPACITY, "the proof-of-work search gave up after 2^(pow_bits + 6) candidates: the proof's nonce word is 2^64 - 1 and does not verify");
  return TMX_OK;
}

}  // extern "C"

// ---- one DEEP-FRI proof over several oracles of different sizes, and the commit set (include/tmx.h "one DEEP-FRI proof over several oracles")
static int32_t batch_check(tmx_ctx* c, const tmx_batch_params* p) {
  auto bad = [&](const std::string& why) { return c ? fail(c, TMX_ERR_BAD_ARG, why) : TMX_ERR_BAD_ARG; };
  if (!p) return bad("params is null");
  if (p->n_oracles < 1 || p->n_oracles > TMX_BATCH_MAX_ORACLES) return bad("n_oracles must be 1 .. 8");
  if (p->log_blowup < 1 || p->log_blowup > 6) return bad("log_blowup must be 1 .. 6");
  if (p->arity_bits < 1 || p->arity_bits > 4) return bad("arity_bits must be 1 .. 4");
  if (p->final_log_max > 8 || p->final_log_max + p->log_blowup > 12) return bad("final_log_max must be at most 8 and final_log_max + log_blowup at most 12");
  if (p->n_queries < 1 || p->n_queries > FRI_MAX_QUERIES) return bad("n_queries must be 1 .. 256");
  if (p->pow_bits > FRI_POW_MAX_BITS) return bad("pow_bits must be at most 24");
  if (p->reserved) return bad("reserved must be 0");
  uint64_t total = 0;
  for (uint32_t k = 0; k < TMX_BATCH_MAX_ORACLES; k++) {
    const std::string who = "oracle " + std::to_string(k) + ": ";
    if (k >= p->n_oracles) {
      if (p->log_n[k] || p->n_cols[k]) return bad(who + "unused array entries must be zero");
      continue;
    }
    if (p->log_n[k] <= p->log_blowup || p->log_n[k] > 28) return bad(who + "log_n must exceed log_blowup and be at most 28");
    if (p->n_cols[k] < 1) return bad(who + "n_cols must be at least 1");
    if (k && p->log_n[k] > p->log_n[k - 1]) return bad(who + "the oracles must be ordered by non-increasing log_n");
    total += p->n_cols[k];
  }
  if (p->cap_height > p->log_n[0]) return bad("cap_height must not exceed log_n of the first oracle");
  if (total > TMX_DEEP_MAX_COLS) return bad("the oracles must have at most 2^24 columns in all");
  return TMX_OK;
}

static void batch_layout(const tmx_batch_params& p, tmx_batch_layout& L) {
  std::memset(&L, 0, sizeof L);
  const uint32_t K = p.n_oracles;
  uint32_t sizes[TMX_BATCH_MAX_ORACLES];
  for (uint32_t k = 0; k < K; k++) {
    if (k && p.log_n[k] != p.log_n[k - 1]) L.n_groups++;
    L.group_of[k] = L.n_groups;
    sizes[L.n_groups] = p.log_n[k];
    L.cap_height_of[k] = std::min(p.cap_height, p.log_n[k]);
  }
  L.n_groups++;
  uint32_t d = p.log_n[0] - p.log_blowup;
  for (uint32_t g = 0; g + 1 < L.n_groups; g++) {
    uint32_t gap = sizes[g] - sizes[g + 1];
    while (gap > 0) {
      const uint32_t b = std::min(p.arity_bits, gap);
      L.layer_bits[L.n_layers++] = b;
      gap -= b;
      d -= b;
    }
    L.layer_enter[L.n_layers - 1] = g + 1;  // (the fold of this layer produces the layer of group g + 1's size)
  }
  while (d > p.final_log_max) {
    const uint32_t b = std::min(p.arity_bits, d - p.final_log_max);
    L.layer_bits[L.n_layers++] = b;
    d -= b;
  }
  L.final_log = d;
  uint64_t w = 0;
  for (uint32_t k = 0; k < K; k++) {
    L.off_open[k] = w;
    w += 4ull << deep_log_r(p.n_cols[k]);
  }
  uint32_t lg = p.log_n[0];
  for (uint32_t l = 0; l < L.n_layers; l++) {
    lg -= L.layer_bits[l];
    L.layer_cap_height[l] = std::min(p.cap_height, lg);
    L.off_caps[l] = w;
    w += 4ull << L.layer_cap_height[l];
  }
  L.off_final = w; w += 2ull << L.final_log;
  L.off_indices = w; w += p.n_queries;
  for (uint32_t k = 0; k < K; k++) {
    L.off_init_rows[k] = w; w += (uint64_t)p.n_queries * p.n_cols[k];
    L.off_init_paths[k] = w; w += (uint64_t)p.n_queries * (p.log_n[k] - L.cap_height_of[k]) * 4;
  }
  lg = p.log_n[0];
  for (uint32_t l = 0; l < L.n_layers; l++) {
    lg -= L.layer_bits[l];
    L.off_rows[l] = w; w += (uint64_t)p.n_queries * (2ull << L.layer_bits[l]);
    L.off_paths[l] = w; w += (uint64_t)p.n_queries * (lg - L.layer_cap_height[l]) * 4;
  }
  L.off_nonce = w;
  if (p.pow_bits) w++;
  L.words = w;
}

// The geometry of a batch proof: FRI's (over the largest oracle's domain and the batch schedule; offsets absolute in the proof) and the
// oracle table
static FriGeom batch_geom(const tmx_batch_params& p, const tmx_batch_layout& L, uint64_t root_2_32, uint64_t shift) {
  tmx_fri_params fp = {p.log_n[0], p.n_cols[0], p.cap_height, p.log_blowup, p.arity_bits, p.final_log_max, p.n_queries, 0};
  tmx_fri_layout FL;
  std::memset(&FL, 0, sizeof FL);
  FL.n_layers = L.n_layers; FL.final_log = L.final_log;
  for (uint32_t l = 0; l < L.n_layers; l++) {
    FL.layer_bits[l] = L.layer_bits[l]; FL.layer_cap_height[l] = L.layer_cap_height[l];
    FL.off_caps[l] = L.off_caps[l]; FL.off_rows[l] = L.off_rows[l]; FL.off_paths[l] = L.off_paths[l];
  }
  FL.off_final = L.off_final; FL.off_indices = L.off_indices;
  FriGeom G = fri_geom(fp, FL, root_2_32, shift);
  G.pow_bits = p.pow_bits;
  G.off_nonce = L.off_nonce;
  G.n_oracles = p.n_oracles; G.n_groups = L.n_groups;
  const uint64_t head[7] = {(1ull << 32) + p.n_oracles, p.log_blowup, p.cap_height, p.arity_bits, p.final_log_max, p.n_queries, p.pow_bits};
  std::memcpy(G.batch_head, head, sizeof head);
  uint32_t off = 0, cap_at = 0;
  for (uint32_t k = 0; k < p.n_oracles; k++) {
    G.o_log_n[k] = p.log_n[k]; G.o_n_cols[k] = p.n_cols[k]; G.o_cap_h[k] = L.cap_height_of[k]; G.o_log_r[k] = deep_log_r(p.n_cols[k]);
    G.o_group[k] = L.group_of[k]; G.o_alpha_off[k] = off; G.o_cap_at[k] = cap_at;
    G.o_w[k] = gl_pow_host(root_2_32, 1ull << (32 - p.log_n[k]));
    G.o_omega[k] = gl_pow_host(G.o_w[k], 1ull << p.log_blowup);
    G.o_off_open[k] = L.off_open[k]; G.o_off_rows[k] = L.off_init_rows[k]; G.o_off_paths[k] = L.off_init_paths[k];
    off += p.n_cols[k];
    cap_at += 4u << L.cap_height_of[k];
  }
  G.total_cols = off;
  for (uint32_t l = 0; l < L.n_layers; l++) G.enter[l] = L.layer_enter[l];
  return G;
}

// What a batch prove reads: per oracle its extended columns, its tree, and the columns its openings are evaluated from (DeepSrc)
// A streamed oracle (chunk_cols[k] != 0, a member of a commit set) has no extended columns (cols[k] == nullptr): its deep[k] columns are the
// set's pre-LDE columns, extended chunk_cols[k] at a time into chunk_buf[k] (chunk_cols[k] << log_n words: the set's shared buffer, or the
// oracle's own for a streamed helper of constraint sets 3 - 5 and 7 - 9) when the queried rows are gathered.
struct BatchSrc {
  const uint64_t* cols[TMX_BATCH_MAX_ORACLES]; const uint64_t* levels[TMX_BATCH_MAX_ORACLES]; DeepSrc deep[TMX_BATCH_MAX_ORACLES];
  uint32_t chunk_cols[TMX_BATCH_MAX_ORACLES]; uint64_t* chunk_buf[TMX_BATCH_MAX_ORACLES];
};

// Validated by the caller.  The stages are DEEP's, run per oracle (evaluation, openings block and its tree) and per group (combine of every
// oracle of the group into ONE buffer, the Y sums, one quotient pass), then ONE set of layers whose folds take the smaller groups in.
static int32_t batch_prove(tmx_ctx* c, const tmx_batch_params& p, const BatchSrc& src, uint64_t root_2_32, uint64_t shift, uint64_t* proof,
                           void* hip_stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  tmx_batch_layout L;
  batch_layout(p, L);
  const FriGeom G = batch_geom(p, L, root_2_32, shift);
  const uint32_t K = p.n_oracles;
  HIPCK(c, hipSetDevice(c->cfg.device));
  int32_t st = poseidon_ready(c, s);
  if (st) return st;
  // scratch (u64 words): transcript state 32 | challenges 64 | degree flag 8 | the K caps | the K openings roots | alpha powers (C + 1) |
  // leaf indices | Y sums [G][8] | layers 0 .. L | Q^(g) of groups 1 .. G - 1 | layer trees | weights | partial sums | an openings tree
  const uint64_t nq = p.n_queries;
  uint64_t at = 104;
  const uint64_t o_caps = at; at += G.o_cap_at[K - 1] + (4ull << G.o_cap_h[K - 1]);
  const uint64_t o_roots = at; at += 4ull * K;
  const uint64_t o_apow = at; at += 2ull * (G.total_cols + 1);
  const uint64_t o_qidx = at; at += L.n_layers * nq;
  const uint64_t o_y = at; at += 8ull * L.n_groups;
  uint64_t o_layer[FRI_MAX_LAYERS + 1], o_lev[FRI_MAX_LAYERS], o_q[TMX_BATCH_MAX_ORACLES] = {};
  uint32_t g_log[TMX_BATCH_MAX_ORACLES] = {}, g_enter_layer[TMX_BATCH_MAX_ORACLES] = {};
  uint32_t lg = p.log_n[0];
  for (uint32_t l = 0; l <= L.n_layers; l++) {
    o_layer[l] = at; at += 2ull << lg;
    if (l < L.n_layers) lg -= L.layer_bits[l];
  }
  for (uint32_t k = 0; k < K; k++) g_log[L.group_of[k]] = p.log_n[k];
  o_q[0] = o_layer[0];
  for (uint32_t g = 1; g < L.n_groups; g++) { o_q[g] = at; at += 2ull << g_log[g]; }
  for (uint32_t l = 0; l < L.n_layers; l++)
    if (L.layer_enter[l]) g_enter_layer[L.layer_enter[l]] = l;
  lg = p.log_n[0];
  for (uint32_t l = 0; l < L.n_layers; l++) {
    lg -= L.layer_bits[l];
    o_lev[l] = at; at += 4 * tmx_poseidon_merkle_digests(lg, L.layer_cap_height[l]);
  }
  uint64_t part_words = 0, olev_words = 0;
  for (uint32_t k = 0; k < K; k++) {
    part_words = std::max<uint64_t>(part_words, deep_eval_tiles(p.log_n[k] - p.log_blowup) * p.n_cols[k] * 4);
    olev_words = std::max<uint64_t>(olev_words, 4 * tmx_poseidon_merkle_digests(G.o_log_r[k], 0));
  }
  const uint64_t o_wt = at; at += 2ull << (p.log_n[0] - p.log_blowup);
  const uint64_t o_part = at; at += part_words;
  const uint64_t o_olev = at; at += olev_words;
  // streamed oracles: F_k on the trace domain (two planes of N_k words), and its extension (two planes of M_k words) for one that does not
  // open its group
  uint64_t sc_words = 0, sx_words = 0;
  for (uint32_t k = 0; k < K; k++) {
    if (!src.chunk_cols[k]) continue;
    sc_words = std::max<uint64_t>(sc_words, 2ull << (p.log_n[k] - p.log_blowup));
    if (k && L.group_of[k] == L.group_of[k - 1]) sx_words = std::max<uint64_t>(sx_words, 2ull << p.log_n[k]);
  }
  const uint64_t o_sc = at; at += sc_words;
  const uint64_t o_sx = at; at += sx_words;
  if (c->fri_bytes < at * 8) {
    if (c->d_fri) { HIPCK(c, hipDeviceSynchronize()); HIPCK(c, hipFree(c->d_fri)); c->d_fri = nullptr; c->fri_bytes = 0; }
    HIPCK(c, hipMalloc(&c->d_fri, at * 8));
    c->fri_bytes = at * 8;
  }
  for (auto& e : c->ev_fri)
    if (!e) HIPCK(c, hipEventCreate(&e));
  c->fri_valid = false;
  c->fri_deep = true;
  c->fri_pow_bits = p.pow_bits;
  uint64_t* W = reinterpret_cast<uint64_t*>(c->d_fri);
  uint64_t *state = W, *chal = W + 32, *apow = W + o_apow, *qidx = W + o_qidx;
  c->fri_flag_off = 96 * 8;
  auto launched = [&](int rc, const char* what) { return rc ? fail(c, TMX_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString((hipError_t)rc)) : TMX_OK; };
  auto transcript = [&](int phase, uint32_t layer, const uint64_t* in) {
    return launched(launch_fri_transcript(c->d_pos_consts, c->pos_mode, G, phase, layer, in, proof, state, chal, qidx, s), "k_fri_transcript");
  };

  HIPCK(c, hipEventRecord(c->ev_fri[0], s));
  for (uint32_t k = 0; k < K; k++) {
    const uint64_t nd = tmx_poseidon_merkle_digests(p.log_n[k], G.o_cap_h[k]), nc = 1ull << G.o_cap_h[k];
    HIPCK(c, hipMemcpyAsync(W + o_caps + G.o_cap_at[k], src.levels[k] + 4 * (nd - nc), nc * 32, hipMemcpyDeviceToDevice, s));
  }
  if ((st = transcript(7, 0, W + o_caps))) return st;
  const uint64_t P = 0xffffffff00000001ull;
  const uint64_t* zeta = chal + FRI_ZETA_AT;
  // the openings, oracle by oracle: one weights table per distinct size (equal sizes are adjacent), the pass over the oracle's columns, its
  // block of the openings section, that block's tree and its root
  for (uint32_t k = 0; k < K; k++) {
    const DeepSrc& d = src.deep[k];
    const uint32_t log_sub = p.log_n[k] - p.log_blowup, log_r = G.o_log_r[k];
    if (k == 0 || p.log_n[k] != p.log_n[k - 1] || d.s != src.deep[k - 1].s) {
      const uint64_t s_n = gl_pow_host(d.s, 1ull << log_sub);
      const uint64_t k_inv = gl_pow_host((uint64_t)(((unsigned __int128)(1ull << log_sub) * s_n) % P), P - 2);
      if ((st = launched(launch_deep_weights(log_sub, d.s, G.o_omega[k], s_n, k_inv, zeta, W + o_wt, s), "k_deep_weights"))) return st;
    }
    uint64_t* open = proof + L.off_open[k];
    if ((st = launched(launch_deep_eval(log_sub, d.log_col, d.stride_log, p.n_cols[k], d.cols, W + o_wt, W + o_part, s), "k_deep_eval"))) return st;
    if ((st = launched(launch_deep_open(log_sub, p.n_cols[k], log_r, W + o_part, open, s), "k_deep_open"))) return st;
    if ((st = tmx_poseidon_merkle_device(c, log_r, 4, open, 0, W + o_olev, hip_stream))) return st;
    HIPCK(c, hipMemcpyAsync(W + o_roots + 4 * k, W + o_olev + 4 * (tmx_poseidon_merkle_digests(log_r, 0) - 1), 32, hipMemcpyDeviceToDevice, s));
  }
  if ((st = transcript(8, 0, W + o_roots))) return st;
  if ((st = launched(launch_fri_alpha_powers(G.total_cols + 1, chal, apow, s), "k_fri_alpha_powers"))) return st;
  // every oracle's columns into its group's buffer (the first of a group writes, the others add), the alpha offset in the table pointer
  for (uint32_t k = 0; k < K; k++) {
    uint64_t* q = W + o_q[L.group_of[k]];
    const bool first = k == 0 || L.group_of[k] != L.group_of[k - 1];
    if (src.chunk_cols[k]) {
      // a streamed oracle: the combination is F_p-linear in the columns and so is the LDE, so combining the pre-LDE columns and extending
      // the two planes gives the words combining the extended columns gives.  The LDE writes into the group's buffer when the oracle opens
      // the group, else next to it, and k_fri_add adds it in.
      const uint32_t log_sub = p.log_n[k] - p.log_blowup;
      if ((st = launched(launch_fri_combine(log_sub, p.n_cols[k], src.deep[k].cols, apow + 2ull * G.o_alpha_off[k], W + o_sc, s), "k_fri_combine"))) return st;
      if ((st = tmx_lde_goldilocks_device(c, log_sub, p.log_blowup, 2, W + o_sc, first ? q : W + o_sx, hip_stream))) return st;
      if (!first && (st = launched(launch_fri_add(2ull << p.log_n[k], W + o_sx, q, s), "k_fri_add"))) return st;
      continue;
    }
    const int rc = first ? launch_fri_combine(p.log_n[k], p.n_cols[k], src.cols[k], apow + 2ull * G.o_alpha_off[k], q, s)
                         : launch_fri_combine_add(p.log_n[k], p.n_cols[k], src.cols[k], apow + 2ull * G.o_alpha_off[k], q, s);
    if ((st = launched(rc, "k_fri_combine"))) return st;
  }
  if ((st = launched(launch_batch_y(G, proof, apow, W + o_y, s), "k_batch_y"))) return st;
  for (uint32_t k = 0; k < K; k++) {
    if (k && L.group_of[k] == L.group_of[k - 1]) continue;
    const uint32_t g = L.group_of[k];
    if ((st = launched(launch_deep_quotient(p.log_n[k], G.s0, G.o_w[k], G.o_omega[k], zeta, W + o_y + 6 * g, W + o_q[g], s), "k_deep_quotient"))) return st;
  }
  HIPCK(c, hipEventRecord(c->ev_fri[1], s));
  lg = p.log_n[0];
  for (uint32_t l = 0; l < L.n_layers; l++) {
    const uint32_t b = L.layer_bits[l], h = L.layer_cap_height[l];
    lg -= b;
    st = tmx_poseidon_merkle_device(c, lg, 2u << b, W + o_layer[l], h, W + o_lev[l], hip_stream);
    if (st) return st;
    const uint64_t nd = tmx_poseidon_merkle_digests(lg, h);
    HIPCK(c, hipMemcpyAsync(proof + L.off_caps[l], W + o_lev[l] + 4 * (nd - (1ull << h)), 32ull << h, hipMemcpyDeviceToDevice, s));
    if ((st = transcript(1, l, W + o_caps))) return st;
    const int rc = L.layer_enter[l] ? launch_fri_fold_add(lg, b, G.s_inv[l], G.w_inv[l], G.g[l], chal + 2 + 2 * l, W + o_layer[l], W + o_q[L.layer_enter[l]],
                                                          W + o_layer[l + 1], s)
                                    : launch_fri_fold(lg, b, G.s_inv[l], G.w_inv[l], G.g[l], chal + 2 + 2 * l, W + o_layer[l], W + o_layer[l + 1], s);
    if ((st = launched(rc, "k_fri_fold"))) return st;
  }
  HIPCK(c, hipEventRecord(c->ev_fri[2], s));
  if ((st = launched(launch_fri_final(lg, L.final_log, G.w_fin_inv, G.s_fin_inv, G.m_fin_inv, W + o_layer[L.n_layers], proof + L.off_final, W + 96, s),
                     "k_fri_final")))
    return st;
  if (!p.pow_bits) {
    if ((st = transcript(2, 0, W + o_caps))) return st;
  } else {
    if ((st = transcript(5, 0, W + o_caps))) return st;
    if ((st = launched(launch_fri_grind(c->d_pos_consts, c->pos_mode, p.pow_bits, state, chal + FRI_POW_AT, s), "k_fri_grind"))) return st;
    if ((st = transcript(6, 0, W + o_caps))) return st;
  }
  HIPCK(c, hipEventRecord(c->ev_fri[3], s));
  // the openings: oracle k at idx mod M_k -- the drawn indices for group 0, the leaf indices of the layer it entered for a later group
  for (uint32_t k = 0; k < K; k++) {
    const uint32_t g = L.group_of[k];
    const uint64_t* idx = g ? qidx + g_enter_layer[g] * nq : proof + L.off_indices;
    if (src.chunk_cols[k]) {  // a streamed oracle: every chunk extended once more, its part of the queried rows gathered; the paths as ever
      const uint32_t log_sub = p.log_n[k] - p.log_blowup;
      for (uint32_t c0 = 0; c0 < p.n_cols[k]; c0 += src.chunk_cols[k]) {
        const uint32_t n = std::min(src.chunk_cols[k], p.n_cols[k] - c0);
        if ((st = tmx_lde_goldilocks_device(c, log_sub, p.log_blowup, n, src.deep[k].cols + ((uint64_t)c0 << log_sub), src.chunk_buf[k], hip_stream))) return st;
        if ((st = launched(launch_merkle_open_chunk(p.log_n[k], n, src.chunk_buf[k], p.n_queries, idx, proof + L.off_init_rows[k] + c0, p.n_cols[k], s),
                           "k_merkle_open_chunk")))
          return st;
      }
      if ((st = launched(launch_merkle_open(p.log_n[k], 1, src.levels[k], p.log_n[k] - G.o_cap_h[k], src.levels[k], p.n_queries, idx, nullptr,
                                            proof + L.off_init_paths[k], false, s), "k_merkle_open")))
        return st;
      continue;
    }
    if ((st = launched(launch_merkle_open(p.log_n[k], p.n_cols[k], src.cols[k], p.log_n[k] - G.o_cap_h[k], src.levels[k], p.n_queries, idx,
                                          proof + L.off_init_rows[k], proof + L.off_init_paths[k], false, s), "k_merkle_open")))
      return st;
  }
  lg = p.log_n[0];
  for (uint32_t l = 0; l < L.n_layers; l++) {
    lg -= L.layer_bits[l];
    if ((st = launched(launch_merkle_open(lg, 2u << L.layer_bits[l], W + o_layer[l], lg - L.layer_cap_height[l], W + o_lev[l], p.n_queries,
                                          qidx + l * nq, proof + L.off_rows[l], proof + L.off_paths[l], false, s), "k_merkle_open")))
      return st;
  }
  HIPCK(c, hipEventRecord(c->ev_fri[4], s));
  c->fri_valid = true;
  return TMX_OK;
}

extern "C" {

int32_t tmx_batch_layout_of(const tmx_batch_params* p, tmx_batch_layout* out) {
  if (!out || batch_check(nullptr, p)) return TMX_ERR_BAD_ARG;
  batch_layout(*p, *out);
  return TMX_OK;
}

int32_t tmx_batch_prove_device(tmx_ctx* c, const tmx_batch_params* p, const uint64_t* const d_cols[], const uint64_t* const d_levels[], uint64_t* d_proof,
                               void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = batch_check(c, p);
  if (st) return st;
  if (!d_cols || !d_levels || !d_proof) return fail(c, TMX_ERR_BAD_ARG, "d_cols, d_levels and d_proof must be set");
  BatchSrc src = {};
  for (uint32_t k = 0; k < p->n_oracles; k++) {
    if (!d_cols[k] || !d_levels[k]) return fail(c, TMX_ERR_BAD_ARG, "oracle " + std::to_string(k) + ": d_cols and d_levels must be set");
    src.cols[k] = d_cols[k];
    src.levels[k] = d_levels[k];
    src.deep[k] = {d_cols[k], p->log_n[k], p->log_blowup, c->ntt_shift % 0xffffffff00000001ull};
  }
  return batch_prove(c, *p, src, c->ntt_root, c->ntt_shift, d_proof, hip_stream);
}

int32_t tmx_batch_verify_device(tmx_ctx* c, const tmx_batch_params* p, const uint64_t* d_caps, const uint64_t* d_proof, uint32_t* d_ok, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = batch_check(c, p);
  if (st) return st;
  if (!d_caps || !d_proof || !d_ok) return fail(c, TMX_ERR_BAD_ARG, "d_caps, d_proof and d_ok must be set");
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCK(c, hipSetDevice(c->cfg.device));
  if ((st = poseidon_ready(c, s))) return st;
  tmx_batch_layout L;
  batch_layout(*p, L);
  const FriGeom G = batch_geom(*p, L, c->ntt_root, c->ntt_shift);
  // the verifier scratch: the K roots, then one openings tree at a time (its root copied out before the next one is built)
  uint64_t tree = 0;
  for (uint32_t k = 0; k < p->n_oracles; k++) tree = std::max<uint64_t>(tree, tmx_poseidon_merkle_digests(G.o_log_r[k], 0));
  const size_t want = (4ull * TMX_BATCH_MAX_ORACLES + 4 * tree) * 8;
  if (c->deepv_bytes < want) {
    if (c->d_deepv) { HIPCK(c, hipDeviceSynchronize()); HIPCK(c, hipFree(c->d_deepv)); c->d_deepv = nullptr; c->deepv_bytes = 0; }
    HIPCK(c, hipMalloc(&c->d_deepv, want));
    c->deepv_bytes = want;
  }
  uint64_t* roots = reinterpret_cast<uint64_t*>(c->d_deepv);
  uint64_t* lev = roots + 4 * TMX_BATCH_MAX_ORACLES;
  for (uint32_t k = 0; k < p->n_oracles; k++) {
    if ((st = tmx_poseidon_merkle_device(c, G.o_log_r[k], 4, d_proof + L.off_open[k], 0, lev, hip_stream))) return st;
    HIPCK(c, hipMemcpyAsync(roots + 4 * k, lev + 4 * (tmx_poseidon_merkle_digests(G.o_log_r[k], 0) - 1), 32, hipMemcpyDeviceToDevice, s));
  }
  const int rc = launch_fri_verify(c->d_pos_consts, c->pos_mode, G, d_caps, d_proof, nullptr, roots, d_ok, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_fri_verify launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

// The plan of a commit set: the oracle list in proof order, where every member's parts sit in the set's scratch, the scratch's size and the
// size of the LDE's own scratch (twice the largest thing it extends at once: a resident member's columns, or one chunk).  Host only; on
// refusal the status and `err`.
struct SetPlan {
  tmx_ctx::SetRec r;
  struct Geo { uint64_t off, rows; uint32_t width, log_n; } geo[8];
  size_t want, lde_scratch;
};
static int32_t set_plan(int32_t kind, uint32_t n_max, uint32_t n_proofs, uint32_t sections, uint32_t streamed, uint32_t chunk_cols, uint32_t log_blowup,
                        uint32_t cap_height, SetPlan& P, std::string& err) {
  const uint32_t tables = TMX_TRACE_LADDERS | TMX_TRACE_SHA512 | TMX_TRACE_SHA256 | TMX_TRACE_TREE | TMX_TRACE_HEADER;
  if (n_proofs == 0) { err = "n_proofs must not be zero"; return TMX_ERR_BAD_ARG; }
  if (sections == 0 || (sections & ~tables)) { err = "sections must be a non-empty mask of row tables of the trace block"; return TMX_ERR_BAD_ARG; }
  if (streamed & ~sections) { err = "streamed must be a subset of sections"; return TMX_ERR_BAD_ARG; }
  if (chunk_cols < 8 || chunk_cols % 8) { err = "chunk_cols must be a multiple of 8, at least 8 (the sponge absorbs eight columns at a time)"; return TMX_ERR_BAD_ARG; }
  tmx_ctx::SetRec& r = P.r;
  r = {};
  for (uint32_t bit = 1; bit <= TMX_TRACE_HEADER; bit <<= 1) {
    if (!(sections & bit)) continue;
    uint32_t log_n = 0, width = 0;
    if (tmx_trace_commit_shape(kind, n_max, bit, &log_n, &width)) { err = "section must be one row table of the trace block"; return TMX_ERR_BAD_ARG; }
    if (log_n + log_blowup > TMX_NTT_MAX_LOG) { err = "log_rows + log_blowup exceeds TMX_NTT_MAX_LOG"; return TMX_ERR_CAPACITY; }
    if ((uint64_t)n_proofs * width > 0xffffffffull) { err = "too many columns"; return TMX_ERR_CAPACITY; }
    // insertion by decreasing log_rows; the bits come in ascending order, so ties keep ascending section bits
    uint32_t at = r.n_oracles++;
    while (at && r.o[at - 1].log_m < log_n + log_blowup) { r.o[at] = r.o[at - 1]; P.geo[at] = P.geo[at - 1]; at--; }
    // (a member that fits one chunk takes the resident path: nothing to carry between chunks)
    r.o[at] = {bit, log_n + log_blowup, n_proofs * width, 0, 0, 0, (streamed & bit) != 0 && n_proofs * width > chunk_cols, false};
    P.geo[at].width = width; P.geo[at].log_n = log_n;
    (void)trace_section_geom((uint32_t)kind, n_max, bit, &P.geo[at].off, &P.geo[at].rows, &width);
  }
  if (cap_height > r.o[0].log_m) { err = "cap_height exceeds the height of the largest tree"; return TMX_ERR_BAD_ARG; }
  size_t want = 0, lde_max = 0;
  uint32_t st_log_m = 0;
  bool any = false;
  for (uint32_t k = 0; k < r.n_oracles; k++) {
    auto& o = r.o[k];
    const size_t cols_b = ((size_t)o.n_cols << P.geo[k].log_n) * 8, lde_b = o.streamed ? 0 : ((size_t)o.n_cols << o.log_m) * 8;
    o.cols_off = want; o.lde_off = want + cols_b; o.lev_off = want + cols_b + lde_b;
    want = o.lev_off + (size_t)tmx_poseidon_merkle_digests(o.log_m, std::min(cap_height, o.log_m)) * 32;
    lde_max = std::max(lde_max, lde_b);
    if (o.streamed) { any = true; st_log_m = std::max(st_log_m, o.log_m); }
  }
  r.chunk_cols = chunk_cols;
  if (any) {
    r.state_off = want; want += ((size_t)12 << st_log_m) * 8;
    r.chunk_off = want; want += ((size_t)chunk_cols << st_log_m) * 8;
    lde_max = std::max(lde_max, ((size_t)chunk_cols << st_log_m) * 8);
  }
  P.want = want; P.lde_scratch = 2 * lde_max;
  r.log_blowup = log_blowup; r.cap_height = cap_height;
  return TMX_OK;
}

uint64_t tmx_trace_commit_set_bytes(int32_t kind, uint32_t n_max, uint32_t n_proofs, uint32_t sections, uint32_t streamed, uint32_t chunk_cols,
                                    uint32_t log_blowup, uint32_t cap_height) {
  SetPlan P;
  std::string err;
  if (set_plan(kind, n_max, n_proofs, sections, streamed, chunk_cols, log_blowup, cap_height, P, err)) return 0;
  return (uint64_t)P.want + P.lde_scratch;
}

int32_t tmx_trace_commit_set_streamed_device(tmx_ctx* c, int32_t kind, uint32_t n_proofs, uint32_t sections, uint32_t streamed, uint32_t chunk_cols,
                                             uint32_t log_blowup, uint32_t cap_height, const void* d_trace_rows, uint64_t* d_caps, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  c->set.valid = false;  // (set again at the end: a call that fails anywhere leaves no set)
  if (!d_trace_rows || !d_caps || n_proofs == 0) return TMX_ERR_BAD_ARG;
  SetPlan P;
  std::string err;
  int32_t st = set_plan(kind, c->cfg.n_max, n_proofs, sections, streamed, chunk_cols, log_blowup, cap_height, P, err);
  if (st) return fail(c, st, err);
  tmx_ctx::SetRec& r = P.r;
  const size_t want = P.want;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCK(c, hipSetDevice(c->cfg.device));
  if (c->set_bytes < want) {
    if (c->d_set) { HIPCK(c, hipStreamSynchronize(s)); HIPCK(c, hipFree(c->d_set)); c->d_set = nullptr; c->set_bytes = 0; }
    size_t free_b = 0, total_b = 0;
    // (the rule of tmx_trace_commit_device summed over the sections; the LDE's own scratch is twice the largest thing extended at once)
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && want + P.lde_scratch > free_b + c->ntt_tmp_bytes)
      return fail(c, TMX_ERR_CAPACITY, "commit set needs " + std::to_string((want + P.lde_scratch) >> 20) + " MiB of scratch, " + std::to_string(free_b >> 20) + " MiB free");
    HIPCK(c, hipMalloc(&c->d_set, want));
    c->set_bytes = want;
  }
  uint8_t* base = reinterpret_cast<uint8_t*>(c->d_set);
  uint64_t cap_at = 0;
  for (uint32_t k = 0; k < r.n_oracles; k++) {
    const auto& o = r.o[k];
    const auto& g = P.geo[k];
    uint64_t* cols = reinterpret_cast<uint64_t*>(base + o.cols_off);
    uint64_t* levels = reinterpret_cast<uint64_t*>(base + o.lev_off);
    const uint32_t h = std::min(cap_height, o.log_m);
    int rc = launch_trace_to_columns(d_trace_rows, trace_elems((uint32_t)kind, c->cfg.n_max), g.off, g.rows, g.width, g.log_n, n_proofs, cols, s);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_trace_to_columns launch: ") + hipGetErrorString((hipError_t)rc));
    if (!o.streamed) {
      uint64_t* lde = reinterpret_cast<uint64_t*>(base + o.lde_off);
      if ((st = tmx_lde_goldilocks_device(c, g.log_n, log_blowup, o.n_cols, cols, lde, hip_stream))) return st;
      if ((st = tmx_poseidon_merkle_device(c, o.log_m, o.n_cols, lde, h, levels, hip_stream))) return st;
    } else {
      // chunk by chunk: extend chunk_cols columns into the shared chunk buffer, absorb them into the rows' sponge states; the last chunk
      // leaves the leaf digests where k_poseidon_leaves would, and the levels above them are the resident path's
      uint64_t* state = reinterpret_cast<uint64_t*>(base + r.state_off);
      uint64_t* chunk = reinterpret_cast<uint64_t*>(base + r.chunk_off);
      if ((st = poseidon_ready(c, s))) return st;
      for (uint32_t c0 = 0; c0 < o.n_cols; c0 += chunk_cols) {
        const uint32_t n = std::min(chunk_cols, o.n_cols - c0);
        if ((st = tmx_lde_goldilocks_device(c, g.log_n, log_blowup, n, cols + ((uint64_t)c0 << g.log_n), chunk, hip_stream))) return st;
        rc = launch_poseidon_leaves_chunk(c->d_pos_consts, c->pos_mode, o.log_m, n, chunk, c0 == 0, c0 + n == o.n_cols, state, levels, s);
        if (rc) return fail(c, TMX_ERR_HIP, std::string("k_poseidon_leaves_chunk launch: ") + hipGetErrorString((hipError_t)rc));
      }
      uint64_t* cur = levels;
      for (uint32_t l = 0; l + h < o.log_m; l++) {
        const uint64_t cnt = 1ull << (o.log_m - l);
        rc = launch_poseidon_level(c->d_pos_consts, c->pos_mode, cnt / 2, cur, cur + 4 * cnt, s);
        if (rc) return fail(c, TMX_ERR_HIP, std::string("k_poseidon_level launch: ") + hipGetErrorString((hipError_t)rc));
        cur += 4 * cnt;
      }
    }
    const uint64_t n_dig = tmx_poseidon_merkle_digests(o.log_m, h), n_cap = (uint64_t)1 << h;
    HIPCK(c, hipMemcpyAsync(d_caps + cap_at, levels + 4 * (n_dig - n_cap), n_cap * 32, hipMemcpyDeviceToDevice, s));
    cap_at += 4 * n_cap;
  }
  r.valid = true; r.root = c->ntt_root; r.shift = c->ntt_shift;
  c->set = r;
  return TMX_OK;
}

int32_t tmx_trace_commit_set_device(tmx_ctx* c, int32_t kind, uint32_t n_proofs, uint32_t sections, uint32_t log_blowup, uint32_t cap_height,
                                    const void* d_trace_rows, uint64_t* d_caps, void* hip_stream) {
  return tmx_trace_commit_set_streamed_device(c, kind, n_proofs, sections, 0, 8, log_blowup, cap_height, d_trace_rows, d_caps, hip_stream);
}

int32_t tmx_trace_commit_set_shape(const tmx_ctx* c, tmx_batch_params* out, uint32_t section_of[TMX_BATCH_MAX_ORACLES]) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (!c->set.valid)
    return fail(const_cast<tmx_ctx*>(c), TMX_ERR_BAD_ARG, "no commit set: no tmx_trace_commit_set_device call has completed since the context was created or since the last failed one");
  if (out) {
    std::memset(out, 0, sizeof *out);
    out->n_oracles = c->set.n_oracles; out->log_blowup = c->set.log_blowup; out->cap_height = c->set.cap_height;
  }
  for (uint32_t k = 0; k < TMX_BATCH_MAX_ORACLES; k++) {
    const bool live = k < c->set.n_oracles;
    if (out && live) { out->log_n[k] = c->set.o[k].log_m; out->n_cols[k] = c->set.o[k].n_cols; }
    if (section_of) section_of[k] = live ? c->set.o[k].section : 0;
  }
  return TMX_OK;
}

int32_t tmx_trace_commit_set_prove_device(tmx_ctx* c, const tmx_batch_params* p, uint64_t* d_proof, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = batch_check(c, p);
  if (st) return st;
  if ((st = tmx_trace_commit_set_shape(c, nullptr, nullptr))) return st;
  const tmx_ctx::SetRec& r = c->set;
  bool same = p->n_oracles == r.n_oracles && p->log_blowup == r.log_blowup && p->cap_height == r.cap_height;
  for (uint32_t k = 0; same && k < r.n_oracles; k++) same = p->log_n[k] == r.o[k].log_m && p->n_cols[k] == r.o[k].n_cols;
  if (!same) return fail(c, TMX_ERR_BAD_ARG, "batch parameters do not match the commit set (tmx_trace_commit_set_shape gives its oracle list, log_blowup and cap_height)");
  if (!d_proof) return fail(c, TMX_ERR_BAD_ARG, "d_proof is null");
  const uint8_t* base = reinterpret_cast<const uint8_t*>(c->d_set);
  BatchSrc src = {};
  bool any = false;
  for (uint32_t k = 0; k < r.n_oracles; k++) {
    if (r.o[k].streamed) {  // (the set's chunk size and buffer, or the member's own)
      any = true;
      const bool own = r.o[k].chunk_cols != 0;
      src.chunk_cols[k] = own ? r.o[k].chunk_cols : r.chunk_cols;
      src.chunk_buf[k] = own ? reinterpret_cast<uint64_t*>(const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(r.o[k].buf) + r.o[k].chunk_off))
                             : reinterpret_cast<uint64_t*>(c->d_set) + r.chunk_off / 8;
    }
    if (r.o[k].ext) {
      // the constraint quotient (tmx_trace_commit_set_air_device): extended columns and levels in a scratch of its own, no pre-LDE columns --
      // its openings read the strided subset of the extended columns, as the caller-oracle path of tmx_batch_prove_device does
      const uint8_t* ab = reinterpret_cast<const uint8_t*>(r.o[k].buf ? r.o[k].buf : c->d_set_air);
      src.cols[k] = reinterpret_cast<const uint64_t*>(ab + r.o[k].lde_off);
      src.levels[k] = reinterpret_cast<const uint64_t*>(ab + r.o[k].lev_off);
      src.deep[k] = {src.cols[k], r.o[k].log_m, r.log_blowup, r.shift % 0xffffffff00000001ull};
      continue;
    }
    // (a helper member of constraint sets 3 - 5 is a resident or a streamed member in a scratch of its own)
    const uint8_t* mb = r.o[k].buf ? reinterpret_cast<const uint8_t*>(r.o[k].buf) : base;
    src.cols[k] = r.o[k].streamed ? nullptr : reinterpret_cast<const uint64_t*>(mb + r.o[k].lde_off);
    src.levels[k] = reinterpret_cast<const uint64_t*>(mb + r.o[k].lev_off);
    // the openings read the pre-LDE columns (n_cols x N_k, on the subgroup itself), as tmx_trace_commit_deep_device does
    src.deep[k] = {reinterpret_cast<const uint64_t*>(mb + r.o[k].cols_off), r.o[k].log_m - r.log_blowup, 0, 1};
  }
  if (!any) return batch_prove(c, *p, src, r.root, r.shift, d_proof, hip_stream);
  // the streamed members are extended again inside the prove, under the domain the set was committed with.  If tmx_ntt_set_domain has
  // changed the context's since, it is put back for the prove and restored after it (each change waits for the device: the tables of the
  // other domain are dropped)
  const uint64_t root = c->ntt_root, shift = c->ntt_shift;
  const bool moved = root != r.root || shift != r.shift;
  if (moved && (st = tmx_ntt_set_domain(c, r.root, r.shift))) return st;
  st = batch_prove(c, *p, src, r.root, r.shift, d_proof, hip_stream);
  if (moved) {
    const int32_t back = tmx_ntt_set_domain(c, root, shift);
    if (!st) st = back;
  }
  return st;
}

}  // extern "C"

// ---- the constraint quotient of the ladder rows: constraint set 1 (include/tmx.h "the constraint quotient of the ladder rows") and set 2,
// set 1 plus the boundary constraints against a public table ("the boundary constraints of the ladder rows") ---------------------------------
// One host path drives both.  `boundary` selects set 2: two more row bounds, a scratch of its own (d_air2) beside set 1's, the public
// table's digest in gamma (phase 10 of the transcript), Pub_gamma ahead of the first piece, and the boundary tables, quotient and check
// launches with d_pub and V.  d_pub is null under set 1.  K = N / 256 ladders; the public table is 17 n_proofs columns of K words.
// The domain constants of one quotient: x_i = s w^i over M = 2^log_n points, N = M >> log_blowup; from log_k on, set 2's alone
struct AirGeo {
  uint64_t s_n, w_n, s_n256, w_n256, om256_inv;
  uint32_t log_k;
  uint64_t s, w, om_k, om255, om255_inv, k_inv, bary_inv;
};
constexpr uint64_t AIR2_K_MAX = 1ull << AIR_PUBLIC_MAX_LOG_K;
constexpr uint64_t AIR2_OFF_TW = AIR2_TAB_WORDS, AIR2_OFF_VP = AIR2_OFF_TW + AIR2_K_MAX, AIR2_OFF_VV = AIR2_OFF_VP + 2 * AIR2_K_MAX,
                   AIR2_OFF_COEF = AIR2_OFF_VV + 2 * AIR2_K_MAX, AIR2_OFF_LEVP = AIR2_OFF_COEF + 2 * AIR2_K_MAX,
                   AIR2_OFF_LEVV = AIR2_OFF_LEVP + 8 * AIR2_K_MAX, AIR2_OFF_EXT = AIR2_OFF_LEVV + 8 * AIR2_K_MAX;

static int32_t air_check(tmx_ctx* c, bool boundary, uint32_t log_n, uint32_t log_blowup, uint32_t n_proofs) {
  if (log_blowup < 1 || log_blowup > 6) return fail(c, TMX_ERR_BAD_ARG, "log_blowup must be 1 .. 6");
  if (log_n <= log_blowup || log_n > 28) return fail(c, TMX_ERR_BAD_ARG, "log_n must exceed log_blowup and be at most 28");
  if (log_n - log_blowup < 8) return fail(c, TMX_ERR_BAD_ARG, "log_n - log_blowup must be at least 8: a ladder is 256 rows");
  if (n_proofs < 1) return fail(c, TMX_ERR_BAD_ARG, "n_proofs must be at least 1");
  if ((uint64_t)n_proofs * AIR_LADDER_WIDTH > TMX_DEEP_MAX_COLS) return fail(c, TMX_ERR_BAD_ARG, "65 n_proofs must be at most 2^24");
  if (!boundary) return TMX_OK;
  if (log_n - log_blowup < 9) return fail(c, TMX_ERR_BAD_ARG, "log_n - log_blowup must be at least 9: the boundary constraints need two ladders");
  if (log_n - log_blowup > 8 + AIR_PUBLIC_MAX_LOG_K) return fail(c, TMX_ERR_BAD_ARG, "log_n - log_blowup must be at most 20: at most 2^12 ladders");
  return TMX_OK;
}

static int32_t air_geo(tmx_ctx* c, bool boundary, uint32_t log_n, uint32_t log_blowup, uint64_t root_2_32, uint64_t shift, AirGeo& A) {
  const uint64_t P = 0xffffffff00000001ull;
  const uint64_t s = shift % P, w = gl_pow_host(root_2_32, 1ull << (32 - log_n)), n = 1ull << (log_n - log_blowup);
  A.s_n = gl_pow_host(s, n); A.w_n = gl_pow_host(w, n);
  A.s_n256 = gl_pow_host(s, n >> 8); A.w_n256 = gl_pow_host(w, n >> 8);
  A.om256_inv = gl_pow_host(gl_pow_host(w, 1ull << (log_n - 8)), P - 2);  // omega_256 = omega_N^(N/256) = w^(M/256)
  uint64_t x = A.s_n;
  for (uint32_t k = 0; k < (1u << log_blowup); k++, x = (uint64_t)(((unsigned __int128)x * A.w_n) % P))
    if (x == 1) return fail(c, TMX_ERR_BAD_ARG, "x^N - 1 vanishes on the evaluation domain: the coset shift lies in the trace domain");
  if (!boundary) return TMX_OK;
  A.log_k = log_n - log_blowup - 8;
  A.s = s; A.w = w;
  A.om_k = gl_pow_host(w, 1ull << (8 + log_blowup));  // omega_N^256 = w^(256 B)
  A.om255 = gl_pow_host(w, 255ull << log_blowup);
  A.om255_inv = gl_pow_host(A.om255, P - 2);
  A.k_inv = gl_pow_host(1ull << A.log_k, P - 2);
  A.bary_inv = (uint64_t)(((unsigned __int128)A.k_inv * gl_pow_host(A.om256_inv, P - 2)) % P);  // 1 / (K omega_256^-1)
  return TMX_OK;
}

static int32_t air_scratch(tmx_ctx* c, uint32_t log_blowup) {
  const size_t want = (2 * (32 + AIR_CHAL_WORDS) + air_table_words(6)) * 8;
  (void)log_blowup;
  if (c->air_bytes < want) {
    if (c->d_air) { HIPCK(c, hipDeviceSynchronize()); HIPCK(c, hipFree(c->d_air)); c->d_air = nullptr; c->air_bytes = 0; }
    HIPCK(c, hipMalloc(&c->d_air, want));
    c->air_bytes = want;
  }
  if (!c->ev_air) HIPCK(c, hipEventCreate(&c->ev_air));
  return TMX_OK;
}

// the set-2 scratch, for a coset of 2^log_m points (log_m = 0: the verifier, which extends nothing)
static int32_t air2_scratch(tmx_ctx* c, uint32_t log_m) {
  const size_t want = (AIR2_OFF_EXT + (log_m ? (size_t)2 << log_m : 0)) * 8;
  if (c->air2_bytes < want) {
    if (c->d_air2) { HIPCK(c, hipDeviceSynchronize()); HIPCK(c, hipFree(c->d_air2)); c->d_air2 = nullptr; c->air2_bytes = 0; }
    HIPCK(c, hipMalloc(&c->d_air2, want));
    c->air2_bytes = want;
  }
  return TMX_OK;
}

// gamma into the prover's (verifier = false) or the verifier's challenge words of d_air.  Set 1: phase 9 over the trace cap.  Set 2: the
// public table's digest (its Poseidon Merkle root) first, then phase 10 over the trace cap and the digest
static int32_t air_gamma(tmx_ctx* c, bool boundary, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs, const uint64_t* d_cap,
                         const uint64_t* d_pub, bool verifier, hipStream_t s) {
  uint64_t* digest = nullptr;
  if (boundary) {
    const uint32_t log_k = log_n - log_blowup - 8;
    uint64_t* lev = reinterpret_cast<uint64_t*>(c->d_air2) + (verifier ? AIR2_OFF_LEVV : AIR2_OFF_LEVP);
    const int32_t st = tmx_poseidon_merkle_device(c, log_k, AIR_PUBLIC_WIDTH * n_proofs, d_pub, 0, lev, s);
    if (st) return st;
    digest = lev + 4 * (tmx_poseidon_merkle_digests(log_k, 0) - 1);
  }
  FriGeom G;
  std::memset(&G, 0, sizeof G);
  const uint32_t obs[5] = {boundary ? 2u : 1u /* the constraint-set id: the ladder rows, with their boundaries */, log_n, log_blowup, cap_height, n_proofs};
  std::memcpy(G.params, obs, sizeof obs);
  G.cap_height = std::min(cap_height, log_n);
  uint64_t* W = reinterpret_cast<uint64_t*>(c->d_air) + (verifier ? 32 + AIR_CHAL_WORDS : 0);
  const int rc = launch_fri_transcript(c->d_pos_consts, c->pos_mode, G, boundary ? 10 : 9, 0, d_cap, digest, W, W + 32, nullptr, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_fri_transcript launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

// Pub_gamma on the coset from the public table and the prover's gamma: V, the coefficients, the extension
static int32_t air2_public(tmx_ctx* c, uint32_t log_m, const AirGeo& B, uint32_t n_proofs, const uint64_t* d_pub, hipStream_t s) {
  uint64_t* X = reinterpret_cast<uint64_t*>(c->d_air2);
  const uint64_t* gamma = reinterpret_cast<const uint64_t*>(c->d_air) + 32 + FRI_GAMMA_AT;
  int rc = launch_air_public_combine(B.log_k, n_proofs, d_pub, gamma, X + AIR2_OFF_VP, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_public_combine launch: ") + hipGetErrorString((hipError_t)rc));
  rc = launch_air_public_twiddles(B.log_k, B.om_k, X + AIR2_OFF_TW, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_public_twiddles launch: ") + hipGetErrorString((hipError_t)rc));
  rc = launch_air_public_coefs(B.log_k, B.k_inv, B.om255_inv, X + AIR2_OFF_VP, X + AIR2_OFF_TW, X + AIR2_OFF_COEF, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_public_coefs launch: ") + hipGetErrorString((hipError_t)rc));
  rc = launch_air_public_extend(log_m, B.log_k, B.s, B.w, X + AIR2_OFF_COEF, X + AIR2_OFF_TW, X + AIR2_OFF_EXT, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_public_extend launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

// one piece of the table: n proofs whose first is proof `first` of the table, their extended columns at cols.  Set 2 keeps its tables in
// its own scratch, and the piece whose first proof is proof 0 carries - Pub_gamma / S
static int32_t air_piece(tmx_ctx* c, bool boundary, uint32_t log_n, uint32_t log_blowup, const AirGeo& A, uint32_t first, uint32_t n,
                         const uint64_t* cols, bool accumulate, uint64_t* d_quot, hipStream_t s) {
  uint64_t* W = reinterpret_cast<uint64_t*>(c->d_air);
  const uint64_t* gamma = W + 32 + FRI_GAMMA_AT;
  if (boundary) {
    uint64_t* X = reinterpret_cast<uint64_t*>(c->d_air2);
    int rc = launch_air_boundary_tables(log_blowup, first, A.s_n, A.w_n, A.s_n256, A.w_n256, A.om256_inv, gamma, X, s);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_boundary_tables launch: ") + hipGetErrorString((hipError_t)rc));
    rc = launch_air_ladder_boundary_quotient(log_n, log_blowup, n, cols, X, first == 0 ? X + AIR2_OFF_EXT : nullptr, accumulate ? 1 : 0, d_quot, s);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_ladder_boundary_quotient launch: ") + hipGetErrorString((hipError_t)rc));
    return TMX_OK;
  }
  uint64_t* tab = W + 2 * (32 + AIR_CHAL_WORDS);
  int rc = launch_air_tables(log_blowup, first, A.s_n, A.w_n, A.s_n256, A.w_n256, A.om256_inv, gamma, tab, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_tables launch: ") + hipGetErrorString((hipError_t)rc));
  rc = launch_air_ladder_quotient(log_n, log_blowup, n, cols, tab, accumulate ? 1 : 0, d_quot, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_ladder_quotient launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

static int32_t air_quotient_range_call(tmx_ctx* c, bool boundary, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                       uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols, const uint64_t* d_cap,
                                       const uint64_t* d_pub, uint64_t* d_quot, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = air_check(c, boundary, log_n, log_blowup, n_proofs);
  if (st) return st;
  if (proof_lo >= proof_hi || proof_hi > n_proofs) return fail(c, TMX_ERR_BAD_ARG, "the proof range must be non-empty and lie within n_proofs");
  if (accumulate > 1) return fail(c, TMX_ERR_BAD_ARG, "accumulate must be 0 or 1");
  if (!d_cols || !d_cap || (boundary && !d_pub) || !d_quot)
    return fail(c, TMX_ERR_BAD_ARG, boundary ? "d_cols, d_cap, d_pub and d_quot must be set" : "d_cols, d_cap and d_quot must be set");
  AirGeo A;
  if ((st = air_geo(c, boundary, log_n, log_blowup, c->ntt_root, c->ntt_shift, A))) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCK(c, hipSetDevice(c->cfg.device));
  if ((st = poseidon_ready(c, s))) return st;
  c->air_valid = false;
  if ((st = air_scratch(c, log_blowup))) return st;
  if (boundary && (st = air2_scratch(c, log_n))) return st;
  if ((st = air_gamma(c, boundary, log_n, log_blowup, cap_height, n_proofs, d_cap, d_pub, false, s))) return st;
  if (boundary && proof_lo == 0 && (st = air2_public(c, log_n, A, n_proofs, d_pub, s))) return st;
  if ((st = air_piece(c, boundary, log_n, log_blowup, A, proof_lo, proof_hi - proof_lo, d_cols + (((uint64_t)proof_lo * AIR_LADDER_WIDTH) << log_n),
                      accumulate != 0, d_quot, s)))
    return st;
  HIPCK(c, hipEventRecord(c->ev_air, s));
  c->air_valid = true;
  return TMX_OK;
}

extern "C" {

int32_t tmx_air_ladder_quotient_range_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                             uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols, const uint64_t* d_cap,
                                             uint64_t* d_quot, void* hip_stream) {
  return air_quotient_range_call(c, false, log_n, log_blowup, cap_height, n_proofs, proof_lo, proof_hi, accumulate, d_cols, d_cap, nullptr, d_quot,
                                 hip_stream);
}

int32_t tmx_air_ladder_quotient_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs, const uint64_t* d_cols,
                                       const uint64_t* d_cap, uint64_t* d_quot, void* hip_stream) {
  return tmx_air_ladder_quotient_range_device(c, log_n, log_blowup, cap_height, n_proofs, 0, n_proofs, 0, d_cols, d_cap, d_quot, hip_stream);
}

int32_t tmx_air_last_gamma(tmx_ctx* c, uint64_t g[2]) {
  if (!c || !g) return TMX_ERR_BAD_ARG;
  if (!c->air_valid) return fail(c, TMX_ERR_BAD_ARG, "no constraint quotient has completed on this context");
  HIPCK(c, hipSetDevice(c->cfg.device));
  HIPCK(c, hipEventSynchronize(c->ev_air));
  HIPCK(c, hipMemcpy(g, reinterpret_cast<uint64_t*>(c->d_air) + 32 + FRI_GAMMA_AT, 16, hipMemcpyDeviceToHost));
  return TMX_OK;
}

}  // extern "C"

static int32_t air_verify_call(tmx_ctx* c, bool boundary, const tmx_batch_params* p, uint32_t k_trace, const uint64_t* d_caps, const uint64_t* d_proof,
                               const uint64_t* d_pub, uint32_t* d_ok, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = batch_check(c, p);
  if (st) return st;
  if (k_trace + 1 >= p->n_oracles) return fail(c, TMX_ERR_BAD_ARG, "k_trace and k_trace + 1 must both be oracles of the proof");
  if (p->n_cols[k_trace] % AIR_LADDER_WIDTH) return fail(c, TMX_ERR_BAD_ARG, "oracle k_trace must have a multiple of 65 columns");
  if (p->log_n[k_trace + 1] != p->log_n[k_trace] || p->n_cols[k_trace + 1] != 2)
    return fail(c, TMX_ERR_BAD_ARG, "oracle k_trace + 1 must be the quotient: the log_n of oracle k_trace and 2 columns");
  const uint32_t log_n = p->log_n[k_trace], n_proofs = p->n_cols[k_trace] / AIR_LADDER_WIDTH;
  if ((st = air_check(c, boundary, log_n, p->log_blowup, n_proofs))) return st;
  if (boundary && !d_pub) return fail(c, TMX_ERR_BAD_ARG, "d_pub is null");
  AirGeo A;
  if ((st = air_geo(c, boundary, log_n, p->log_blowup, c->ntt_root, c->ntt_shift, A))) return st;
  if ((st = tmx_batch_verify_device(c, p, d_caps, d_proof, d_ok, hip_stream))) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  if ((st = air_scratch(c, p->log_blowup))) return st;
  if (boundary && (st = air2_scratch(c, 0))) return st;
  tmx_batch_layout L;
  batch_layout(*p, L);
  const FriGeom G = batch_geom(*p, L, c->ntt_root, c->ntt_shift);
  // zeta as the batch transcript draws it, gamma from the trace cap (set 2: and the verifier's own digest of d_pub): both into the
  // verifier's words of d_air, then the identity (set 2: V from d_pub first)
  uint64_t* V = reinterpret_cast<uint64_t*>(c->d_air) + 32 + AIR_CHAL_WORDS;
  int rc = launch_fri_transcript(c->d_pos_consts, c->pos_mode, G, 7, 0, d_caps, nullptr, V, V + 32, nullptr, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_fri_transcript launch: ") + hipGetErrorString((hipError_t)rc));
  if ((st = air_gamma(c, boundary, log_n, p->log_blowup, p->cap_height, n_proofs, d_caps + G.o_cap_at[k_trace], d_pub, true, s))) return st;
  const uint64_t *open_t = d_proof + L.off_open[k_trace], *open_q = d_proof + L.off_open[k_trace + 1];
  if (!boundary) {
    rc = launch_air_ladder_check(n_proofs, G.o_log_r[k_trace], log_n - p->log_blowup, A.om256_inv, open_t, open_q, V + 32 + FRI_ZETA_AT,
                                 V + 32 + FRI_GAMMA_AT, p->n_queries, d_ok, s);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_ladder_check launch: ") + hipGetErrorString((hipError_t)rc));
    return TMX_OK;
  }
  uint64_t* vv = reinterpret_cast<uint64_t*>(c->d_air2) + AIR2_OFF_VV;
  rc = launch_air_public_combine(A.log_k, n_proofs, d_pub, V + 32 + FRI_GAMMA_AT, vv, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_public_combine launch: ") + hipGetErrorString((hipError_t)rc));
  rc = launch_air_ladder_boundary_check(n_proofs, G.o_log_r[k_trace], log_n - p->log_blowup, A.om256_inv, A.om255, A.om_k, A.bary_inv, open_t, open_q,
                                        V + 32 + FRI_ZETA_AT, V + 32 + FRI_GAMMA_AT, vv, p->n_queries, d_ok, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_ladder_boundary_check launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

static int32_t air_set_call(tmx_ctx* c, bool boundary, const uint64_t* d_pub, uint64_t* d_cap_q, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = tmx_trace_commit_set_shape(c, nullptr, nullptr);
  if (st) return st;
  if (boundary && !d_pub) return fail(c, TMX_ERR_BAD_ARG, "d_pub is null");
  if (!d_cap_q) return fail(c, TMX_ERR_BAD_ARG, "d_cap_q is null");
  tmx_ctx::SetRec r = c->set;
  uint32_t kt = r.n_oracles;
  for (uint32_t k = 0; k < r.n_oracles; k++) {
    if (r.o[k].section == TMX_TRACE_LADDERS_QUOTIENT) return fail(c, TMX_ERR_BAD_ARG, "the commit set already holds the ladders' constraint quotient");
    if (r.o[k].section == TMX_TRACE_LADDERS) kt = k;
  }
  if (kt == r.n_oracles) return fail(c, TMX_ERR_BAD_ARG, "the commit set does not hold TMX_TRACE_LADDERS");
  if (r.n_oracles >= TMX_BATCH_MAX_ORACLES) return fail(c, TMX_ERR_BAD_ARG, "the commit set has no room for one more oracle");
  const tmx_ctx::SetRec::Oracle lad = r.o[kt];
  const uint32_t log_m = lad.log_m, log_sub = log_m - r.log_blowup, n_proofs = lad.n_cols / AIR_LADDER_WIDTH, h = std::min(r.cap_height, log_m);
  if ((st = air_check(c, boundary, log_m, r.log_blowup, n_proofs))) return st;
  if (lad.streamed && r.chunk_cols < AIR_LADDER_WIDTH)
    return fail(c, TMX_ERR_BAD_ARG, "a streamed ladders member is fed in chunks of whole proofs: chunk_cols must be at least 65");
  AirGeo A;
  if ((st = air_geo(c, boundary, log_m, r.log_blowup, r.root, r.shift, A))) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCK(c, hipSetDevice(c->cfg.device));
  if ((st = poseidon_ready(c, s))) return st;
  c->air_valid = false;
  if ((st = air_scratch(c, r.log_blowup))) return st;
  if (boundary && (st = air2_scratch(c, log_m))) return st;
  const uint64_t n_dig = tmx_poseidon_merkle_digests(log_m, h), n_cap = 1ull << h;
  const size_t quot_b = ((size_t)2 << log_m) * 8, want = quot_b + (size_t)n_dig * 32;
  if (c->set_air_bytes < want) {
    if (c->d_set_air) { HIPCK(c, hipStreamSynchronize(s)); HIPCK(c, hipFree(c->d_set_air)); c->d_set_air = nullptr; c->set_air_bytes = 0; }
    HIPCK(c, hipMalloc(&c->d_set_air, want));
    c->set_air_bytes = want;
  }
  uint8_t* base = reinterpret_cast<uint8_t*>(c->d_set);
  uint64_t* quot = reinterpret_cast<uint64_t*>(c->d_set_air);
  uint64_t* lev_q = quot + ((size_t)2 << log_m);
  const uint64_t* lev_t = reinterpret_cast<const uint64_t*>(base + lad.lev_off);
  if ((st = air_gamma(c, boundary, log_m, r.log_blowup, r.cap_height, n_proofs, lev_t + 4 * (n_dig - n_cap), d_pub, false, s))) return st;
  // Pub_gamma is extended by kernels of its own from the set's root and shift: the context's NTT domain plays no part in it
  if (boundary && (st = air2_public(c, log_m, A, n_proofs, d_pub, s))) return st;
  if (!lad.streamed) {
    if ((st = air_piece(c, boundary, log_m, r.log_blowup, A, 0, n_proofs, reinterpret_cast<const uint64_t*>(base + lad.lde_off), false, quot, s)))
      return st;
  } else {
    // chunks of whole proofs, each extended once more into the set's chunk buffer under the set's domain (as the streamed prove does: if
    // tmx_ntt_set_domain has changed the context's since, it is put back for this call and restored after it)
    const uint64_t root = c->ntt_root, shift = c->ntt_shift;
    const bool moved = root != r.root || shift != r.shift;
    if (moved && (st = tmx_ntt_set_domain(c, r.root, r.shift))) return st;
    const uint64_t* cols = reinterpret_cast<const uint64_t*>(base + lad.cols_off);
    uint64_t* chunk = reinterpret_cast<uint64_t*>(base + r.chunk_off);
    const uint32_t per = r.chunk_cols / AIR_LADDER_WIDTH;
    for (uint32_t p0 = 0; p0 < n_proofs && !st; p0 += per) {
      const uint32_t n = std::min(per, n_proofs - p0);
      st = tmx_lde_goldilocks_device(c, log_sub, r.log_blowup, n * AIR_LADDER_WIDTH, cols + (((uint64_t)p0 * AIR_LADDER_WIDTH) << log_sub), chunk, hip_stream);
      if (!st) st = air_piece(c, boundary, log_m, r.log_blowup, A, p0, n, chunk, p0 != 0, quot, s);
    }
    if (moved) {
      const int32_t back = tmx_ntt_set_domain(c, root, shift);
      if (!st) st = back;
    }
    if (st) return st;
  }
  HIPCK(c, hipEventRecord(c->ev_air, s));
  c->air_valid = true;
  if ((st = tmx_poseidon_merkle_device(c, log_m, 2, quot, h, lev_q, hip_stream))) return st;
  HIPCK(c, hipMemcpyAsync(d_cap_q, lev_q + 4 * (n_dig - n_cap), n_cap * 32, hipMemcpyDeviceToDevice, s));
  for (uint32_t k = r.n_oracles; k > kt + 1; k--) r.o[k] = r.o[k - 1];
  r.o[kt + 1] = {TMX_TRACE_LADDERS_QUOTIENT, log_m, 2, 0, 0, quot_b, false, true};
  r.n_oracles++;
  c->set = r;
  return TMX_OK;
}

extern "C" {

int32_t tmx_air_verify_device(tmx_ctx* c, const tmx_batch_params* p, uint32_t k_trace, const uint64_t* d_caps, const uint64_t* d_proof, uint32_t* d_ok,
                              void* hip_stream) {
  return air_verify_call(c, false, p, k_trace, d_caps, d_proof, nullptr, d_ok, hip_stream);
}

int32_t tmx_trace_commit_set_air_device(tmx_ctx* c, uint64_t* d_cap_q, void* hip_stream) {
  return air_set_call(c, false, nullptr, d_cap_q, hip_stream);
}

// ---- the public table of the ladder rows from element rows, and set 2's entry points

int32_t tmx_air_ladder_public_shape(int32_t kind, uint32_t n_max, uint32_t n_proofs, uint32_t* log_k, uint32_t* n_cols) {
  uint32_t log_rows = 0, width = 0;
  if (n_proofs < 1 || tmx_trace_commit_shape(kind, n_max, TMX_TRACE_LADDERS, &log_rows, &width) != TMX_OK) return TMX_ERR_BAD_ARG;
  if (log_rows < 9 || log_rows > 8 + AIR_PUBLIC_MAX_LOG_K || (uint64_t)n_proofs * AIR_LADDER_WIDTH > TMX_DEEP_MAX_COLS) return TMX_ERR_BAD_ARG;
  if (log_k) *log_k = log_rows - 8;
  if (n_cols) *n_cols = AIR_PUBLIC_WIDTH * n_proofs;
  return TMX_OK;
}

int32_t tmx_air_ladder_public_device(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_elems, uint64_t* d_pub, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP) return fail(c, TMX_ERR_BAD_ARG, "kind must be TMX_KIND_SKIP or TMX_KIND_STEP");
  uint32_t log_k = 0;
  if (tmx_air_ladder_public_shape(kind, c->cfg.n_max, n_proofs, &log_k, nullptr))
    return fail(c, TMX_ERR_BAD_ARG, "n_proofs must be at least 1 (65 n_proofs at most 2^24) and the ladders table 2 .. 2^12 ladders");
  if (!d_elems || !d_pub) return fail(c, TMX_ERR_BAD_ARG, "d_elems and d_pub must be set");
  HIPCK(c, hipSetDevice(c->cfg.device));
  const Program& prog = c->prog[kind];
  // D.1b of a lane: h (8), then A.x A.y R.x R.y, then sB.x sB.y hA.x hA.y: the sixteen words of sB start at element 40
  const int rc = launch_air_public_gather(d_elems, prog.sp.elem_stride, prog.d1b_start, D1B_LANE_ELEMS, 8 + 4 * 8, c->cfg.n_max, log_k, n_proofs, d_pub,
                                          hip_stream);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_public_gather launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

int32_t tmx_air_ladder_boundary_quotient_range_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                      uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                      const uint64_t* d_cap, const uint64_t* d_pub, uint64_t* d_quot, void* hip_stream) {
  return air_quotient_range_call(c, true, log_n, log_blowup, cap_height, n_proofs, proof_lo, proof_hi, accumulate, d_cols, d_cap, d_pub, d_quot,
                                 hip_stream);
}

int32_t tmx_air_ladder_boundary_quotient_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                const uint64_t* d_cols, const uint64_t* d_cap, const uint64_t* d_pub, uint64_t* d_quot,
                                                void* hip_stream) {
  return tmx_air_ladder_boundary_quotient_range_device(c, log_n, log_blowup, cap_height, n_proofs, 0, n_proofs, 0, d_cols, d_cap, d_pub, d_quot,
                                                       hip_stream);
}

int32_t tmx_air_boundary_verify_device(tmx_ctx* c, const tmx_batch_params* p, uint32_t k_trace, const uint64_t* d_caps, const uint64_t* d_proof,
                                       const uint64_t* d_pub, uint32_t* d_ok, void* hip_stream) {
  return air_verify_call(c, true, p, k_trace, d_caps, d_proof, d_pub, d_ok, hip_stream);
}

int32_t tmx_trace_commit_set_air_boundary_device(tmx_ctx* c, const uint64_t* d_pub, uint64_t* d_cap_q, void* hip_stream) {
  return air_set_call(c, true, d_pub, d_cap_q, hip_stream);
}

}  // extern "C"

// ---- constraint sets 3, 4, 5 and 6 on the SHA-256 tables: the round constraints, the message schedule, the block starts and the link to
// Level-1 (include/tmx.h "the round constraints of the SHA-256 tables", "the message schedule ...", "the block starts ...", "the SHA-256
// tables' link to Level-1") -----------------------------------------------------------------------------------------------------------------
// One host path drives all four: the same argument checks, the same geometry, the same tables-then-quotient pass, the same scratch layout
// and the same placement in the commit set.  The tables of a quotient launch of sets 3 - 5 sit in the table part of d_air (air.h
// AIR3_TAB_*, AIR4_TAB_*, AIR5_TAB_*), the challenge words of all four where set 1 keeps its own.  What differs between the sets is a
// ShaSet: the id, the helper's column count, whether the set has a chain mode, whether it has a public table, the rows it accepts, the two
// section ids, the row of tmx_ctx::d_set_sha, the words its messages differ in, and the four launches of a set without a public table
// under set 5's signatures (sets 3 and 4 have no mode: their adapters drop `chain`).  A set with a public table (set 6) takes d_pub, null
// for the others, and does its public step at four places, each a branch on has_public: gamma observes the table's digest (sha_gamma), the
// pass writes its tables to d_air6 and the piece that starts at proof 0 carries - PQ (sha_pass), the verifier forms V before its check
// (sha_verify_call), and the helper kernel reads d_pub (sha_helper_launch).  Its helper is resident only: the streamed calls take sets 3 - 5 and 7 - 9.
// Sets 7, 8 and 9 (the SHA-512 table: 18 columns per proof, 80-row blocks) are the fifth, sixth and seventh rows.  Where they differ from
// rows 3 - 6 is a branch on has_periodic: the pass reads the extended preprocessed planes of the set's scratch instead of period-64 tables
// (sha_pass; sha512_periodic fills and extends them in front of it), the verifier runs the barycentric kernel in front of its check
// (sha_verify_call), and the set-level call takes TMX_TRACE_SHA512 alone.  Rows 3 - 6 take none of these branches.  What the three differ
// in there is a ShaPeriodic the row carries: how many preprocessed planes there are (3, 1, 2), the context scratch that holds them (d_air7,
// d_air8, d_air9), and the set's instantiations of the launches that fill them, read them in the pass and evaluate them at zeta.
// Set 10 (the SHA-512 table's link to Level-1) is the eighth row and has BOTH has_public and has_periodic.  Set 6's public step is taken
// under has_public && !has_periodic; set 10 takes the periodic branch and, inside it, a public step of its own at the same four places:
// gamma observes the digest of its 49-column table (sha_gamma), the piece that starts at proof 0 is followed by - Pub_gamma / (x^N - 1)
// (sha_pass: link512_public), the verifier forms V and evaluates Pub_gamma(zeta) before a check that knows it (sha_verify_call), and the
// helper kernel reads d_pub (sha_helper_launch).  Rows 3 - 9 enqueue what they enqueued.  Resident only.
struct ShaPeriodic {
  uint32_t planes, part_words;  // the preprocessed columns; the words of one workgroup's row of the barycentric kernel
  void* tmx_ctx::*scratch;      // rows of the barycentric kernel | the planes before the LDE [planes][N] | extended [planes][M]
  size_t tmx_ctx::*bytes;
  const AirSha512Launch* k;  // fill, tables, quotient, eval, fold, check (air.h)
  uint32_t fixed_words = 0;  // set 10: words of its public side between the rows and the planes (LINK512_*); its V and extended Pub follow the planes
};
struct ShaSet {
  uint32_t id, helper_cols;
  bool has_chain, has_public;
  uint32_t rows_lo, rows_hi;  // log2 of the pre-LDE rows it accepts
  uint32_t helper_section, quotient_section;
  int scratch;
  const char *bad_sub, *bad_rows;               // the refusals of log_n - log_blowup and of log_rows outside rows_lo .. rows_hi
  const char *stem, *word, *already;            // k_air_<stem>_*, "the <word> member", the refusal of a second set-level call
  const char *at_helper, *at_quot, *bad_index;  // how the verifier's messages name the helper's and the quotient's oracle index
  int (*helper)(uint32_t log_rows, uint32_t n_proofs, uint32_t chain, const void* d_table, void* d_helper, void* stream);
  int (*tables)(uint32_t log_blowup, uint32_t chain, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_sel, uint64_t w_sel, uint64_t rho,
                const void* d_gamma, void* d_tab, void* stream);
  int (*quotient)(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, uint32_t chain, const void* d_cols, const void* d_helper_cols,
                  const void* d_tab, int form, void* d_quot, void* stream);
  int (*check)(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint32_t chain, uint64_t rho, const void* d_open_t,
               const void* d_open_h, const void* d_open_q, const void* d_zeta, const void* d_gamma, uint32_t n_queries, void* d_ok, void* stream);
  uint32_t width;     // the table's columns per proof
  bool has_periodic;  // sets 7, 8 and 9: preprocessed columns of full degree in place of the period-64 tables
  const ShaPeriodic* per;  // what such a set's preprocessed columns are; null without has_periodic
};

static int sha3_helper(uint32_t log_rows, uint32_t n_proofs, uint32_t, const void* d_table, void* d_helper, void* stream) {
  return launch_air_sha_helper(log_rows, n_proofs, d_table, d_helper, stream);
}
static int sha3_tables(uint32_t log_blowup, uint32_t, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n64, uint64_t w_n64,
                       uint64_t om64_inv, const void* d_gamma, void* d_tab, void* stream) {
  return launch_air_sha_tables(log_blowup, first_proof, s_n, w_n, s_n64, w_n64, om64_inv, d_gamma, d_tab, stream);
}
static int sha3_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, uint32_t, const void* d_cols, const void* d_helper_cols,
                         const void* d_tab, int form, void* d_quot, void* stream) {
  return launch_air_sha_quotient(log_m, log_blowup, n_proofs, d_cols, d_helper_cols, d_tab, form, d_quot, stream);
}
static int sha3_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint32_t, uint64_t om64_inv, const void* d_open_t,
                      const void* d_open_h, const void* d_open_q, const void* d_zeta, const void* d_gamma, uint32_t n_queries, void* d_ok,
                      void* stream) {
  return launch_air_sha_check(n_proofs, log_r_t, log_r_h, log_sub, om64_inv, d_open_t, d_open_h, d_open_q, d_zeta, d_gamma, n_queries, d_ok, stream);
}
static int sha4_helper(uint32_t log_rows, uint32_t n_proofs, uint32_t, const void* d_table, void* d_helper, void* stream) {
  return launch_air_sched_helper(log_rows, n_proofs, d_table, d_helper, stream);
}
static int sha4_tables(uint32_t log_blowup, uint32_t, uint64_t first_proof, uint64_t s_n, uint64_t w_n, uint64_t s_n64, uint64_t w_n64,
                       uint64_t om64_inv, const void* d_gamma, void* d_tab, void* stream) {
  return launch_air_sched_tables(log_blowup, first_proof, s_n, w_n, s_n64, w_n64, om64_inv, d_gamma, d_tab, stream);
}
static int sha4_quotient(uint32_t log_m, uint32_t log_blowup, uint32_t n_proofs, uint32_t, const void* d_cols, const void* d_helper_cols,
                         const void* d_tab, int form, void* d_quot, void* stream) {
  return launch_air_sched_quotient(log_m, log_blowup, n_proofs, d_cols, d_helper_cols, d_tab, form, d_quot, stream);
}
static int sha4_check(uint32_t n_proofs, uint32_t log_r_t, uint32_t log_r_h, uint32_t log_sub, uint32_t, uint64_t om64_inv, const void* d_open_t,
                      const void* d_open_h, const void* d_open_q, const void* d_zeta, const void* d_gamma, uint32_t n_queries, void* d_ok,
                      void* stream) {
  return launch_air_sched_check(n_proofs, log_r_t, log_r_h, log_sub, om64_inv, d_open_t, d_open_h, d_open_q, d_zeta, d_gamma, n_queries, d_ok, stream);
}

static int sha7_helper(uint32_t log_rows, uint32_t n_proofs, uint32_t, const void* d_table, void* d_helper, void* stream) {
  return launch_air_sha512_helper(log_rows, n_proofs, d_table, d_helper, stream);
}
static int sha8_helper(uint32_t log_rows, uint32_t n_proofs, uint32_t, const void* d_table, void* d_helper, void* stream) {
  return launch_air_sha512_sched_helper(log_rows, n_proofs, d_table, d_helper, stream);
}
static int sha9_helper(uint32_t log_rows, uint32_t n_proofs, uint32_t, const void* d_table, void* d_helper, void* stream) {
  return launch_air_sha512_init_helper(log_rows, n_proofs, d_table, d_helper, stream);
}
static const ShaPeriodic SHA7_PERIODIC = {3, AIR7_PART_WORDS, &tmx_ctx::d_air7, &tmx_ctx::air7_bytes, air_sha512_launch(7)};
static const ShaPeriodic SHA8_PERIODIC = {1, AIR8_PART_WORDS, &tmx_ctx::d_air8, &tmx_ctx::air8_bytes, air_sha512_launch(8)};
static const ShaPeriodic SHA9_PERIODIC = {2, AIR9_PART_WORDS, &tmx_ctx::d_air9, &tmx_ctx::air9_bytes, air_sha512_launch(9)};
// Set 10's fixed words behind the rows of the planes' barycentric kernel: the rows of the public side's | the levels of the public digest,
// prover | verifier (a table of at most 2^12 slots)
constexpr uint64_t LINK512_LEV_WORDS = 8ull << 12, LINK512_OFF_PUB_PART = (uint64_t)AIR7_MAX_PARTS * AIR10_PART_WORDS,
                   LINK512_OFF_LEVP = LINK512_OFF_PUB_PART + (uint64_t)AIR7_MAX_PARTS * AIR10_PUB_PART_WORDS,
                   LINK512_OFF_LEVV = LINK512_OFF_LEVP + LINK512_LEV_WORDS;
static const ShaPeriodic SHA10_PERIODIC = {5, AIR10_PART_WORDS, &tmx_ctx::d_air10, &tmx_ctx::air10_bytes, air_sha512_launch(10),
                                           (uint32_t)(LINK512_OFF_LEVV + LINK512_LEV_WORDS - LINK512_OFF_PUB_PART)};

// by ascending id: a set-level call places its pair behind the pairs of the sets in front of it
static const char SHA_BAD_SUB[] = "log_n - log_blowup must be at least 6: a SHA-256 block is 64 rows";
static const char SHA_BAD_ROWS[] = "log_rows must be 6 .. 27: a SHA-256 block is 64 rows";
static const ShaSet SHA_SETS[8] = {
    {3, AIR_SHA_HELPER_COLS, false, false, 6, 27, TMX_TRACE_SHA256_HELPER, TMX_TRACE_SHA256_QUOTIENT, 0, SHA_BAD_SUB, SHA_BAD_ROWS, "sha", "helper",
     "the commit set already holds the helper and the quotient of that section", "k_trace + 1", "k_trace + 2",
     "k_trace, k_trace + 1 and k_trace + 2 must all be oracles of the proof", sha3_helper, sha3_tables, sha3_quotient, sha3_check, AIR_SHA_WIDTH, false, nullptr},
    {4, AIR_SCHED_HELPER_COLS, false, false, 6, 27, TMX_TRACE_SHA256_SCHED_HELPER, TMX_TRACE_SHA256_SCHED_QUOTIENT, 1, SHA_BAD_SUB, SHA_BAD_ROWS,
     "sched", "schedule helper", "the commit set already holds the schedule helper and quotient of that section", "k_helper", "k_helper + 1",
     "k_trace < k_helper, and k_helper and k_helper + 1 must be oracles of the proof", sha4_helper, sha4_tables, sha4_quotient, sha4_check, AIR_SHA_WIDTH, false,
     nullptr},
    {5, AIR_INIT_HELPER_COLS, true, false, 6, 27, TMX_TRACE_SHA256_INIT_HELPER, TMX_TRACE_SHA256_INIT_QUOTIENT, 2, SHA_BAD_SUB, SHA_BAD_ROWS, "init",
     "block-start helper", "the commit set already holds the block-start helper and quotient of that section", "k_helper", "k_helper + 1",
     "k_trace < k_helper, and k_helper and k_helper + 1 must be oracles of the proof", launch_air_init_helper, launch_air_init_tables,
     launch_air_init_quotient, launch_air_init_check, AIR_SHA_WIDTH, false, nullptr},
    {6, AIR_LINK_HELPER_COLS, false, true, 6 + AIR_SHA_PUBLIC_MIN_LOG_K, 6 + AIR_SHA_PUBLIC_MAX_LOG_K, TMX_TRACE_SHA256_LINK_HELPER,
     TMX_TRACE_SHA256_LINK_QUOTIENT, 3, "log_n - log_blowup must be 7 .. 18: the public table has 2 .. 2^12 blocks of 64 rows",
     "log_rows must be 7 .. 18: the public table has 2 .. 2^12 blocks of 64 rows", "link", "link helper",
     "the commit set already holds the link helper and quotient of that section", "k_helper", "k_helper + 1",
     "k_trace < k_helper, and k_helper and k_helper + 1 must be oracles of the proof", nullptr, nullptr, nullptr, nullptr, AIR_SHA_WIDTH, false,
     nullptr},
    {7, AIR_SHA512_HELPER_COLS, false, false, 7, 18, TMX_TRACE_SHA512_HELPER, TMX_TRACE_SHA512_QUOTIENT, 4,
     "log_n - log_blowup must be 7 .. 18: a SHA-512 block is 80 rows and the verifier evaluates the preprocessed columns over all of them",
     "log_rows must be 7 .. 18: a SHA-512 block is 80 rows and the verifier evaluates the preprocessed columns over all of them", "sha512",
     "SHA-512 helper", "the commit set already holds the SHA-512 helper and quotient of that section", "k_trace + 1", "k_trace + 2",
     "k_trace, k_trace + 1 and k_trace + 2 must all be oracles of the proof", sha7_helper, nullptr, nullptr, nullptr, AIR_SHA512_WIDTH, true,
     &SHA7_PERIODIC},
    {8, AIR_SHA512_SCHED_HELPER_COLS, false, false, 7, 18, TMX_TRACE_SHA512_SCHED_HELPER, TMX_TRACE_SHA512_SCHED_QUOTIENT, 5,
     "log_n - log_blowup must be 7 .. 18: a SHA-512 block is 80 rows and the verifier evaluates the preprocessed column over all of them",
     "log_rows must be 7 .. 18: a SHA-512 block is 80 rows and the verifier evaluates the preprocessed column over all of them", "sha512_sched",
     "SHA-512 schedule helper", "the commit set already holds the SHA-512 schedule helper and quotient of that section", "k_helper", "k_helper + 1",
     "k_trace < k_helper, and k_helper and k_helper + 1 must be oracles of the proof", sha8_helper, nullptr, nullptr, nullptr, AIR_SHA512_WIDTH, true,
     &SHA8_PERIODIC},
    {9, AIR_SHA512_INIT_HELPER_COLS, false, false, 7, 18, TMX_TRACE_SHA512_INIT_HELPER, TMX_TRACE_SHA512_INIT_QUOTIENT, 6,
     "log_n - log_blowup must be 7 .. 18: a SHA-512 block is 80 rows and the verifier evaluates the preprocessed columns over all of them",
     "log_rows must be 7 .. 18: a SHA-512 block is 80 rows and the verifier evaluates the preprocessed columns over all of them", "sha512_init",
     "SHA-512 block-start helper", "the commit set already holds the SHA-512 block-start helper and quotient of that section", "k_helper",
     "k_helper + 1", "k_trace < k_helper, and k_helper and k_helper + 1 must be oracles of the proof", sha9_helper, nullptr, nullptr, nullptr,
     AIR_SHA512_WIDTH, true, &SHA9_PERIODIC},
    // (set 10: BOTH a public table and preprocessed planes; its helper reads d_pub, its pass and its check know the public side)
    {10, AIR_SHA512_LINK_HELPER_COLS, false, true, 7, 18, TMX_TRACE_SHA512_LINK_HELPER, TMX_TRACE_SHA512_LINK_QUOTIENT, 7,
     "log_n - log_blowup must be 7 .. 18: a SHA-512 block is 80 rows and the verifier evaluates the preprocessed columns over all of them",
     "log_rows must be 7 .. 18: a SHA-512 block is 80 rows and the verifier evaluates the preprocessed columns over all of them", "sha512_link",
     "SHA-512 link helper", "the commit set already holds the SHA-512 link helper and quotient of that section", "k_helper", "k_helper + 1",
     "k_trace < k_helper, and k_helper and k_helper + 1 must be oracles of the proof", nullptr, nullptr, nullptr, nullptr, AIR_SHA512_WIDTH, true,
     &SHA10_PERIODIC},
};

static int32_t sha_launch_failed(tmx_ctx* c, const ShaSet& d, const char* kernel, int rc) {
  return fail(c, TMX_ERR_HIP, std::string("k_air_") + d.stem + "_" + kernel + " launch: " + hipGetErrorString((hipError_t)rc));
}

static std::string sha_too_many_cols(const ShaSet& d) { return std::to_string(d.helper_cols) + " n_proofs must be at most 2^24"; }

// chain is 0 for a set without a mode
static int32_t sha_check(tmx_ctx* c, const ShaSet& d, uint32_t log_n, uint32_t log_blowup, uint32_t n_proofs, uint32_t chain) {
  if (log_blowup < 1 || log_blowup > 6) return fail(c, TMX_ERR_BAD_ARG, "log_blowup must be 1 .. 6");
  if (log_n <= log_blowup || log_n > 28) return fail(c, TMX_ERR_BAD_ARG, "log_n must exceed log_blowup and be at most 28");
  if (log_n - log_blowup < d.rows_lo || log_n - log_blowup > d.rows_hi) return fail(c, TMX_ERR_BAD_ARG, d.bad_sub);
  if (n_proofs < 1) return fail(c, TMX_ERR_BAD_ARG, "n_proofs must be at least 1");
  if ((uint64_t)n_proofs * d.helper_cols > TMX_DEEP_MAX_COLS) return fail(c, TMX_ERR_BAD_ARG, sha_too_many_cols(d));
  if (chain > 1) return fail(c, TMX_ERR_BAD_ARG, "chain must be 0 or 1");
  if (chain && log_n - log_blowup < 7) return fail(c, TMX_ERR_BAD_ARG, "chain = 1 needs at least 128 rows: a chained hash is two blocks");
  return TMX_OK;
}

// s, w the coset; om = omega_N = w^B, om_k = omega_K = om^64, om64 = omega_64 = om^K, k_inv = 1 / K
struct LinkGeo { uint32_t log_k; uint64_t s, w, om, om_k, om64, k_inv; };
static void link_geo(uint32_t log_n, uint32_t log_blowup, uint64_t root_2_32, uint64_t shift, LinkGeo& B) {
  const uint64_t P = 0xffffffff00000001ull;
  B.log_k = log_n - log_blowup - 6;
  B.s = shift % P;
  B.w = gl_pow_host(root_2_32, 1ull << (32 - log_n));
  B.om = gl_pow_host(B.w, 1ull << log_blowup);
  B.om_k = gl_pow_host(B.om, 64);
  B.om64 = gl_pow_host(B.om, 1ull << B.log_k);
  B.k_inv = gl_pow_host(1ull << B.log_k, P - 2);
}

// s_n = s^N, w_n = w^N; the selector's period is 64 << chain rows: s_sel = s^(N/64), w_sel = w^(N/64), rho = omega_64^-1 under chain = 0,
// s^(N/128), w^(N/128), omega_128^-1 under chain = 1; link: filled for a set with a public table
struct ShaGeo { uint64_t s_n, w_n, s_sel, w_sel, rho; LinkGeo link; uint64_t root, shift; /* the domain they were taken under */ };

static int32_t sha_geo(tmx_ctx* c, const ShaSet& d, uint32_t log_n, uint32_t log_blowup, uint32_t chain, uint64_t root_2_32, uint64_t shift, ShaGeo& A) {
  const uint64_t P = 0xffffffff00000001ull;
  if (d.has_public && !d.has_periodic) link_geo(log_n, log_blowup, root_2_32, shift, A.link);
  A.root = root_2_32; A.shift = shift;
  const uint64_t s = shift % P, w = gl_pow_host(root_2_32, 1ull << (32 - log_n)), n = 1ull << (log_n - log_blowup);
  const uint32_t log_per = 6 + chain;
  A.s_n = gl_pow_host(s, n); A.w_n = gl_pow_host(w, n);
  A.s_sel = gl_pow_host(s, n >> log_per); A.w_sel = gl_pow_host(w, n >> log_per);
  A.rho = gl_pow_host(gl_pow_host(w, 1ull << (log_n - log_per)), P - 2);  // omega_64 = omega_N^(N/64) = w^(M/64), omega_128 = w^(M/128)
  uint64_t x = A.s_n;
  for (uint32_t k = 0; k < (1u << log_blowup); k++, x = (uint64_t)(((unsigned __int128)x * A.w_n) % P))
    if (x == 1) return fail(c, TMX_ERR_BAD_ARG, "x^N - 1 vanishes on the evaluation domain: the coset shift lies in the trace domain");
  return TMX_OK;
}

// What set 6 has of its own inside that path: the public side.  Set 3's geometry and LinkGeo, and a scratch of its own (words at d_air6):
//   tables (air.h AIR6_TAB_*) | twiddles [K] | V of the prover [17][K][2] | V of the verifier | coefficients [2 K] | the public digest's
//   levels, prover and verifier | one extended public polynomial (2 M) | PQ (2 M)
// One extended public polynomial and PQ live here per context, not per section; the scratch of a section is sets 3 - 5's layout with 33
// columns per proof (row 3 of d_set_sha).
constexpr uint64_t AIR6_K_MAX = 1ull << AIR_SHA_PUBLIC_MAX_LOG_K;
constexpr uint64_t AIR6_OFF_TW = AIR6_TAB_WORDS, AIR6_OFF_VP = AIR6_OFF_TW + AIR6_K_MAX, AIR6_OFF_VV = AIR6_OFF_VP + 34 * AIR6_K_MAX,
                   AIR6_OFF_COEF = AIR6_OFF_VV + 34 * AIR6_K_MAX, AIR6_OFF_LEVP = AIR6_OFF_COEF + 2 * AIR6_K_MAX,
                   AIR6_OFF_LEVV = AIR6_OFF_LEVP + 8 * AIR6_K_MAX, AIR6_OFF_EXT = AIR6_OFF_LEVV + 8 * AIR6_K_MAX;

// the set-6 scratch, for a coset of 2^log_m points (log_m = 0: the verifier, which extends nothing)
static int32_t link_scratch(tmx_ctx* c, uint32_t log_m) {
  const size_t want = (AIR6_OFF_EXT + (log_m ? (size_t)4 << log_m : 0)) * 8;
  if (c->air6_bytes < want) {
    if (c->d_air6) { HIPCK(c, hipDeviceSynchronize()); HIPCK(c, hipFree(c->d_air6)); c->d_air6 = nullptr; c->air6_bytes = 0; }
    HIPCK(c, hipMalloc(&c->d_air6, want));
    c->air6_bytes = want;
  }
  return TMX_OK;
}

// PQ on the coset from the public table and the prover's gamma: V, then per coset the coefficients, the extension and its fold.  The
// tables (first = 0) are written first: the fold reads 1 / S and 1 / D_t
static int32_t link_public(tmx_ctx* c, uint32_t log_m, uint32_t log_blowup, const ShaGeo& A, uint32_t n_proofs, const uint64_t* d_pub, hipStream_t s) {
  const uint64_t P = 0xffffffff00000001ull;
  const LinkGeo& B = A.link;
  uint64_t* X = reinterpret_cast<uint64_t*>(c->d_air6);
  const uint64_t* gamma = reinterpret_cast<const uint64_t*>(c->d_air) + 32 + FRI_GAMMA_AT;
  int rc = launch_air_link_tables(log_blowup, 0, A.s_n, A.w_n, A.s_sel, A.w_sel, B.om64, gamma, X, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_link_tables launch: ") + hipGetErrorString((hipError_t)rc));
  rc = launch_air_link_combine(B.log_k, n_proofs, d_pub, gamma, X + AIR6_OFF_VP, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_link_combine launch: ") + hipGetErrorString((hipError_t)rc));
  rc = launch_air_public_twiddles(B.log_k, B.om_k, X + AIR6_OFF_TW, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_public_twiddles launch: ") + hipGetErrorString((hipError_t)rc));
  uint64_t* ext = X + AIR6_OFF_EXT;
  uint64_t* pq = ext + ((size_t)2 << log_m);
  for (uint32_t k = 0; k < 17; k++) {
    const uint32_t off = k ? k - 1 : 63;
    const uint64_t off_inv = gl_pow_host(gl_pow_host(B.om, off), P - 2);
    rc = launch_air_public_coefs(B.log_k, B.k_inv, off_inv, X + AIR6_OFF_VP + ((uint64_t)k << (B.log_k + 1)), X + AIR6_OFF_TW, X + AIR6_OFF_COEF, s);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_public_coefs launch: ") + hipGetErrorString((hipError_t)rc));
    rc = launch_air_public_extend(log_m, B.log_k, B.s, B.w, X + AIR6_OFF_COEF, X + AIR6_OFF_TW, ext, s);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_public_extend launch: ") + hipGetErrorString((hipError_t)rc));
    rc = launch_air_link_fold(log_m, log_blowup, k, k == 0, ext, X, pq, s);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_link_fold launch: ") + hipGetErrorString((hipError_t)rc));
  }
  return TMX_OK;
}

// What set 7 has of its own inside that path: the preprocessed columns.  A scratch of its own (words at d_air7): the barycentric kernel's
// rows | SEL, KLO, KHI before the LDE [3][N] | the three extended planes [3][M].  One per context, not per section.
// Set 8 has the same of its own (words at d_air8) with one plane, SCH: d_air7 does not grow for it.  Set 9 likewise (d_air9; STA, CHN).
static uint64_t sha512_off_pre(const ShaSet& d) { return (uint64_t)AIR7_MAX_PARTS * d.per->part_words + d.per->fixed_words; }
static_assert(AIR7_MAX_PARTS * AIR7_PART_WORDS == 512, "set 7's scratch layout stays as it is");

// the scratch of set 7, 8 or 9, for a coset of 2^log_m points over 2^log_sub rows (log_m = 0: the verifier, which fills and extends nothing)
static int32_t sha512_scratch(tmx_ctx* c, const ShaSet& d, uint32_t log_m, uint32_t log_sub) {
  // (a set with a public table, set 10: behind the planes the extended Pub_gamma [2][M], then V [2][N]; the verifier passes its log_sub for V)
  const size_t planes = d.per->planes, pub = d.has_public ? 2 : 0;
  const size_t want = (sha512_off_pre(d) + (log_m ? (planes << log_sub) + ((planes + pub) << log_m) : 0) + (pub << log_sub)) * 8;
  void*& buf = c->*(d.per->scratch);
  size_t& bytes = c->*(d.per->bytes);
  if (bytes < want) {
    if (buf) { HIPCK(c, hipDeviceSynchronize()); HIPCK(c, hipFree(buf)); buf = nullptr; bytes = 0; }
    HIPCK(c, hipMalloc(&buf, want));
    bytes = want;
  }
  return TMX_OK;
}
static const uint64_t* sha512_planes(const tmx_ctx* c, const ShaSet& d, uint32_t log_sub) {
  return reinterpret_cast<const uint64_t*>(c->*(d.per->scratch)) + sha512_off_pre(d) + ((size_t)d.per->planes << log_sub);
}

// set 10's extended Pub_gamma and its V inside that scratch (log_m = 0: the verifier's layout, V alone)
static uint64_t* link512_pubext(const tmx_ctx* c, const ShaSet& d, uint32_t log_m, uint32_t log_sub) {
  return reinterpret_cast<uint64_t*>(c->*(d.per->scratch)) + sha512_off_pre(d) + ((size_t)d.per->planes << log_sub) + ((size_t)d.per->planes << log_m);
}
static uint64_t* link512_v(const tmx_ctx* c, const ShaSet& d, uint32_t log_m, uint32_t log_sub) {
  return log_m ? link512_pubext(c, d, log_m, log_sub) + ((size_t)2 << log_m) : reinterpret_cast<uint64_t*>(c->*(d.per->scratch)) + sha512_off_pre(d);
}

// The public side of set 10's pass: V_r from d_pub under the prover's gamma, extended like two helper columns under the domain the geometry
// was taken under (put there for the extension if the context's has moved), and subtracted from the quotient over x^N - 1
static int32_t link512_public(tmx_ctx* c, const ShaSet& d, uint32_t log_m, uint32_t log_blowup, const ShaGeo& A, uint32_t n_proofs,
                              const uint64_t* d_pub, const uint64_t* tab, uint64_t* d_quot, hipStream_t s) {
  const uint32_t log_sub = log_m - log_blowup;
  uint64_t* v = link512_v(c, d, log_m, log_sub);
  uint64_t* ext = link512_pubext(c, d, log_m, log_sub);
  int rc = launch_air_sha512_link_combine(log_sub, n_proofs, d_pub, reinterpret_cast<const uint64_t*>(c->d_air) + 32 + FRI_GAMMA_AT, v, s);
  if (rc) return sha_launch_failed(c, d, "combine", rc);
  const uint64_t root = c->ntt_root, shift = c->ntt_shift;
  const bool moved = root != A.root || shift != A.shift;
  int32_t st;
  if (moved && (st = tmx_ntt_set_domain(c, A.root, A.shift))) return st;
  st = tmx_lde_goldilocks_device(c, log_sub, log_blowup, 2, v, ext, s);
  if (moved) {
    const int32_t back = tmx_ntt_set_domain(c, root, shift);
    if (!st) st = back;
  }
  if (st) return st;
  rc = launch_air_sha512_link_public_sub(log_m, log_blowup, ext, tab, d_quot, s);
  if (rc) return sha_launch_failed(c, d, "public_sub", rc);
  return TMX_OK;
}

// The preprocessed columns (SEL, KLO and KHI; SCH) filled and extended exactly as helper columns are: under the context's current NTT
// domain (the set-level call has put the set's domain there)
static int32_t sha512_periodic(tmx_ctx* c, const ShaSet& d, uint32_t log_m, uint32_t log_blowup, void* hip_stream) {
  const uint32_t log_sub = log_m - log_blowup;
  uint64_t* pre = reinterpret_cast<uint64_t*>(c->*(d.per->scratch)) + sha512_off_pre(d);
  const int rc = d.per->k->fill(log_sub, pre, hip_stream);
  if (rc) return sha_launch_failed(c, d, "periodic", rc);
  return tmx_lde_goldilocks_device(c, log_sub, log_blowup, d.per->planes, pre, pre + ((size_t)d.per->planes << log_sub), hip_stream);
}

// gamma from the table cap and the helper cap, into the prover's (verifier = false) or the verifier's challenge words of d_air.  A set with
// a public table: the table's digest (its Poseidon Merkle root) first, then the lone-lane kernel over the two caps and the digest
static int32_t sha_gamma(tmx_ctx* c, const ShaSet& d, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs, uint32_t chain,
                         const uint64_t* d_cap, const uint64_t* d_cap_helper, const uint64_t* d_pub, bool verifier, hipStream_t s) {
  const uint32_t obs[5] = {d.id | chain << 8 /* the constraint-set id, and set 5's mode */, log_n, log_blowup, cap_height, n_proofs};
  const uint32_t cap_words = 4u << std::min(cap_height, log_n);
  uint64_t* W = reinterpret_cast<uint64_t*>(c->d_air) + (verifier ? 32 + AIR_CHAL_WORDS : 0);
  if (!d.has_public) {
    const int rc = launch_air_sha_gamma(c->d_pos_consts, c->pos_mode, obs, cap_words, d_cap, d_cap_helper, W, W + 32, s);
    if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_sha_gamma launch: ") + hipGetErrorString((hipError_t)rc));
    return TMX_OK;
  }
  // (set 10: the slots of its 80-row blocks, 49 columns per proof, the levels in its own scratch; the lone-lane kernel is set 6's)
  const uint32_t log_k = d.has_periodic ? air_sha512_public_log_k(log_n - log_blowup) : log_n - log_blowup - 6;
  uint64_t* lev = d.has_periodic ? reinterpret_cast<uint64_t*>(c->d_air10) + (verifier ? LINK512_OFF_LEVV : LINK512_OFF_LEVP)
                                 : reinterpret_cast<uint64_t*>(c->d_air6) + (verifier ? AIR6_OFF_LEVV : AIR6_OFF_LEVP);
  const int32_t st = tmx_poseidon_merkle_device(c, log_k, (d.has_periodic ? AIR_SHA512_PUBLIC_WIDTH : AIR_SHA_PUBLIC_WIDTH) * n_proofs, d_pub, 0, lev, s);
  if (st) return st;
  const int rc = launch_air_link_gamma(c->d_pos_consts, c->pos_mode, obs, cap_words, d_cap, d_cap_helper,
                                       lev + 4 * (tmx_poseidon_merkle_digests(log_k, 0) - 1), W, W + 32, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_link_gamma launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

// the tables from the prover's gamma, then the pass.  form = AIR_FORM_WHOLE: the whole table (first = 0).  A piece: n_proofs proofs whose
// first is proof `first` of the table, cols that proof's table column 0 and hcols the piece's own helper columns.  A set with a public
// table (d_pub, of n_all proofs): the piece that starts at proof 0 first forms PQ, which writes the tables too, and carries - PQ
static int32_t sha_pass(tmx_ctx* c, const ShaSet& d, uint32_t log_n, uint32_t log_blowup, uint32_t chain, const ShaGeo& A, uint32_t first,
                        uint32_t n_proofs, const uint64_t* cols, const uint64_t* hcols, const uint64_t* d_pub, uint32_t n_all, int form,
                        uint64_t* d_quot, hipStream_t s) {
  uint64_t* W = reinterpret_cast<uint64_t*>(c->d_air);
  int rc;
  if (d.has_public && !d.has_periodic) {
    uint64_t* X = reinterpret_cast<uint64_t*>(c->d_air6);
    if (first == 0) {
      const int32_t st = link_public(c, log_n, log_blowup, A, n_all, d_pub, s);
      if (st) return st;
    } else if ((rc = launch_air_link_tables(log_blowup, first, A.s_n, A.w_n, A.s_sel, A.w_sel, A.link.om64, W + 32 + FRI_GAMMA_AT, X, s))) {
      return sha_launch_failed(c, d, "tables", rc);
    }
    rc = launch_air_link_quotient(log_n, log_blowup, n_proofs, cols, hcols, X, first == 0 ? X + AIR6_OFF_EXT + ((size_t)2 << log_n) : nullptr, form,
                                  d_quot, s);
  } else if (d.has_periodic) {  // the extended planes (sha512_periodic, in front of this call) instead of the period-64 tables
    uint64_t* tab = W + 2 * (32 + AIR_CHAL_WORDS);
    if ((rc = d.per->k->tables(log_blowup, first, A.s_n, A.w_n, W + 32 + FRI_GAMMA_AT, tab, s))) return sha_launch_failed(c, d, "tables", rc);
    rc = d.per->k->quotient(log_n, log_blowup, n_proofs, cols, hcols, sha512_planes(c, d, log_n - log_blowup), tab, form, d_quot, s);
    // (set 10: the piece that starts at proof 0 carries - Pub_gamma / (x^N - 1), set 6's rule)
    if (!rc && d.has_public && first == 0) return link512_public(c, d, log_n, log_blowup, A, n_all, d_pub, tab, d_quot, s);
  } else {
    uint64_t* tab = W + 2 * (32 + AIR_CHAL_WORDS);
    if ((rc = d.tables(log_blowup, chain, first, A.s_n, A.w_n, A.s_sel, A.w_sel, A.rho, W + 32 + FRI_GAMMA_AT, tab, s)))
      return sha_launch_failed(c, d, "tables", rc);
    rc = d.quotient(log_n, log_blowup, n_proofs, chain, cols, hcols, tab, form, d_quot, s);
  }
  if (rc) return sha_launch_failed(c, d, "quotient", rc);
  return TMX_OK;
}

static int sha_helper_launch(const ShaSet& d, uint32_t log_rows, uint32_t n_proofs, uint32_t chain, const void* d_table, const void* d_pub,
                             void* d_helper, void* stream) {
  return d.has_public ? (d.has_periodic ? launch_air_sha512_link_helper(log_rows, n_proofs, d_table, d_pub, d_helper, stream)
                                        : launch_air_link_helper(log_rows, n_proofs, d_table, d_pub, d_helper, stream))
                      : d.helper(log_rows, n_proofs, chain, d_table, d_helper, stream);
}

static int32_t sha_helper_call(tmx_ctx* c, const ShaSet& d, uint32_t log_rows, uint32_t n_proofs, uint32_t chain, const uint64_t* d_table,
                               const uint64_t* d_pub, uint64_t* d_helper, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (log_rows < d.rows_lo || log_rows > d.rows_hi) return fail(c, TMX_ERR_BAD_ARG, d.bad_rows);
  if (n_proofs < 1) return fail(c, TMX_ERR_BAD_ARG, "n_proofs must be at least 1");
  if ((uint64_t)n_proofs * d.helper_cols > TMX_DEEP_MAX_COLS) return fail(c, TMX_ERR_BAD_ARG, sha_too_many_cols(d));
  if (chain > 1) return fail(c, TMX_ERR_BAD_ARG, "chain must be 0 or 1");
  if (chain && log_rows < 7) return fail(c, TMX_ERR_BAD_ARG, "chain = 1 needs at least 128 rows: a chained hash is two blocks");
  if (!d_table || (d.has_public && !d_pub) || !d_helper)
    return fail(c, TMX_ERR_BAD_ARG, d.has_public ? "d_table, d_pub and d_helper must be set" : "d_table and d_helper must be set");
  HIPCK(c, hipSetDevice(c->cfg.device));
  const int rc = sha_helper_launch(d, log_rows, n_proofs, chain, d_table, d_pub, d_helper, hip_stream);
  if (rc) return sha_launch_failed(c, d, "helper", rc);
  return TMX_OK;
}

// form = AIR_FORM_WHOLE: the quotient of the whole table (proof_lo = 0, proof_hi = n_proofs).  Else the piece [proof_lo, proof_hi), whose
// helper columns alone are at d_helper_cols; gamma is drawn over n_proofs either way
static int32_t sha_quotient_call(tmx_ctx* c, const ShaSet& d, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                 uint32_t chain, uint32_t proof_lo, uint32_t proof_hi, int form, const uint64_t* d_cols,
                                 const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper, const uint64_t* d_pub,
                                 uint64_t* d_quot, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = sha_check(c, d, log_n, log_blowup, n_proofs, chain);
  if (st) return st;
  if (proof_lo >= proof_hi || proof_hi > n_proofs) return fail(c, TMX_ERR_BAD_ARG, "the proof range must be non-empty and lie within n_proofs");
  if (!d_cols || !d_helper_cols || !d_cap || !d_cap_helper || (d.has_public && !d_pub) || !d_quot)
    return fail(c, TMX_ERR_BAD_ARG, d.has_public ? "d_cols, d_helper_cols, d_cap, d_cap_helper, d_pub and d_quot must be set"
                                                 : "d_cols, d_helper_cols, d_cap, d_cap_helper and d_quot must be set");
  ShaGeo A;
  if ((st = sha_geo(c, d, log_n, log_blowup, chain, c->ntt_root, c->ntt_shift, A))) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCK(c, hipSetDevice(c->cfg.device));
  if ((st = poseidon_ready(c, s))) return st;
  c->air_valid = false;
  if ((st = air_scratch(c, log_blowup))) return st;
  if (d.has_public && !d.has_periodic && (st = link_scratch(c, log_n))) return st;
  if (d.has_periodic && ((st = sha512_scratch(c, d, log_n, log_n - log_blowup)) || (st = sha512_periodic(c, d, log_n, log_blowup, hip_stream)))) return st;
  if ((st = sha_gamma(c, d, log_n, log_blowup, cap_height, n_proofs, chain, d_cap, d_cap_helper, d_pub, false, s))) return st;
  if ((st = sha_pass(c, d, log_n, log_blowup, chain, A, proof_lo, proof_hi - proof_lo, d_cols + (((uint64_t)proof_lo * d.width) << log_n),
                     d_helper_cols, d_pub, n_proofs, form, d_quot, s)))
    return st;
  HIPCK(c, hipEventRecord(c->ev_air, s));
  c->air_valid = true;
  return TMX_OK;
}

static int32_t sha_quotient_range_call(tmx_ctx* c, const ShaSet& d, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                       uint32_t chain, uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                       const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper, const uint64_t* d_pub,
                                       uint64_t* d_quot, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (accumulate > 1) return fail(c, TMX_ERR_BAD_ARG, "accumulate must be 0 or 1");
  return sha_quotient_call(c, d, log_n, log_blowup, cap_height, n_proofs, chain, proof_lo, proof_hi, accumulate ? AIR_FORM_PIECE_ACC : AIR_FORM_PIECE,
                           d_cols, d_helper_cols, d_cap, d_cap_helper, d_pub, d_quot, hip_stream);
}

static int32_t sha_verify_call(tmx_ctx* c, const ShaSet& d, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, uint32_t chain,
                               const uint64_t* d_caps, const uint64_t* d_proof, const uint64_t* d_pub, uint32_t* d_ok, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = batch_check(c, p);
  if (st) return st;
  if (k_helper <= k_trace || (uint64_t)k_helper + 1 >= p->n_oracles) return fail(c, TMX_ERR_BAD_ARG, d.bad_index);
  if (p->n_cols[k_trace] == 0 || p->n_cols[k_trace] % d.width)
    return fail(c, TMX_ERR_BAD_ARG, "oracle k_trace must have a multiple of " + std::to_string(d.width) + " columns");
  const uint32_t log_n = p->log_n[k_trace], n_proofs = p->n_cols[k_trace] / d.width;
  if (p->log_n[k_helper] != log_n || (uint64_t)p->n_cols[k_helper] != (uint64_t)d.helper_cols * n_proofs)
    return fail(c, TMX_ERR_BAD_ARG, std::string("oracle ") + d.at_helper + " must be the helper: the log_n of oracle k_trace and " +
                                        std::to_string(d.helper_cols) + " columns per proof");
  if (p->log_n[k_helper + 1] != log_n || p->n_cols[k_helper + 1] != 2)
    return fail(c, TMX_ERR_BAD_ARG, std::string("oracle ") + d.at_quot + " must be the quotient: the log_n of oracle k_trace and 2 columns");
  if ((st = sha_check(c, d, log_n, p->log_blowup, n_proofs, chain))) return st;
  if (d.has_public && !d_pub) return fail(c, TMX_ERR_BAD_ARG, "d_pub is null");
  ShaGeo A;
  if ((st = sha_geo(c, d, log_n, p->log_blowup, chain, c->ntt_root, c->ntt_shift, A))) return st;
  if ((st = tmx_batch_verify_device(c, p, d_caps, d_proof, d_ok, hip_stream))) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  if ((st = air_scratch(c, p->log_blowup))) return st;
  if (d.has_public && !d.has_periodic && (st = link_scratch(c, 0))) return st;
  if (d.has_periodic && (st = sha512_scratch(c, d, 0, d.has_public ? log_n - p->log_blowup : 0))) return st;
  tmx_batch_layout L;
  batch_layout(*p, L);
  const FriGeom G = batch_geom(*p, L, c->ntt_root, c->ntt_shift);
  // zeta as the batch transcript draws it, gamma from the two caps (and the verifier's own digest of d_pub): both into the verifier's words
  // of d_air, then the identity (a set with a public table: V from d_pub first)
  uint64_t* V = reinterpret_cast<uint64_t*>(c->d_air) + 32 + AIR_CHAL_WORDS;
  int rc = launch_fri_transcript(c->d_pos_consts, c->pos_mode, G, 7, 0, d_caps, nullptr, V, V + 32, nullptr, s);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_fri_transcript launch: ") + hipGetErrorString((hipError_t)rc));
  if ((st = sha_gamma(c, d, log_n, p->log_blowup, p->cap_height, n_proofs, chain, d_caps + G.o_cap_at[k_trace], d_caps + G.o_cap_at[k_helper], d_pub,
                      true, s)))
    return st;
  const uint64_t *open_t = d_proof + L.off_open[k_trace], *open_h = d_proof + L.off_open[k_helper], *open_q = d_proof + L.off_open[k_helper + 1];
  if (d.has_public && !d.has_periodic) {
    const LinkGeo& B = A.link;
    uint64_t* vv = reinterpret_cast<uint64_t*>(c->d_air6) + AIR6_OFF_VV;
    rc = launch_air_link_combine(B.log_k, n_proofs, d_pub, V + 32 + FRI_GAMMA_AT, vv, s);
    if (rc) return sha_launch_failed(c, d, "combine", rc);
    rc = launch_air_link_check(n_proofs, G.o_log_r[k_trace], G.o_log_r[k_helper], log_n - p->log_blowup, B.om64, B.om, B.om_k, B.k_inv, open_t, open_h,
                               open_q, V + 32 + FRI_ZETA_AT, V + 32 + FRI_GAMMA_AT, vv, p->n_queries, d_ok, s);
  } else if (d.has_periodic) {  // the barycentric kernel in front of the check: the preprocessed columns at zeta over the N rows
    const uint32_t log_sub = log_n - p->log_blowup;
    const uint64_t P = 0xffffffff00000001ull, om = gl_pow_host(c->ntt_root, 1ull << (32 - log_sub)), n_inv = gl_pow_host(1ull << log_sub, P - 2);
    void* part = c->*(d.per->scratch);
    rc = d.per->k->eval(log_sub, om, V + 32 + FRI_ZETA_AT, part, s);
    if (rc) return sha_launch_failed(c, d, "periodic_eval", rc);
    if (d.has_public) {  // set 10: the verifier's own V from d_pub and its gamma, Pub_gamma(zeta) over the N rows, then the check that knows it
      uint64_t* vv = link512_v(c, d, 0, log_sub);
      uint64_t* pub_part = reinterpret_cast<uint64_t*>(part) + LINK512_OFF_PUB_PART;
      if ((rc = launch_air_sha512_link_combine(log_sub, n_proofs, d_pub, V + 32 + FRI_GAMMA_AT, vv, s))) return sha_launch_failed(c, d, "combine", rc);
      if ((rc = launch_air_sha512_link_public_eval(log_sub, om, V + 32 + FRI_ZETA_AT, vv, pub_part, s))) return sha_launch_failed(c, d, "public_eval", rc);
      rc = launch_air_sha512_link_check(n_proofs, G.o_log_r[k_trace], G.o_log_r[k_helper], log_sub, n_inv, part, pub_part, open_t, open_h, open_q,
                                        V + 32 + FRI_ZETA_AT, V + 32 + FRI_GAMMA_AT, p->n_queries, d_ok, s);
    } else
      rc = d.per->k->check(n_proofs, G.o_log_r[k_trace], G.o_log_r[k_helper], log_sub, n_inv, part, open_t, open_h, open_q, V + 32 + FRI_ZETA_AT,
                           V + 32 + FRI_GAMMA_AT, p->n_queries, d_ok, s);
  } else {
    rc = d.check(n_proofs, G.o_log_r[k_trace], G.o_log_r[k_helper], log_n - p->log_blowup, chain, A.rho, open_t, open_h, open_q, V + 32 + FRI_ZETA_AT,
                 V + 32 + FRI_GAMMA_AT, p->n_queries, d_ok, s);
  }
  if (rc) return sha_launch_failed(c, d, "check", rc);
  return TMX_OK;
}

// The scratch of one set and section.  Resident: helper pre-LDE columns | helper extended columns | helper levels | quotient | quotient
// levels.  Streamed (chunk_proofs < n_proofs): the extended columns are absent, and behind the quotient's levels sit the sponge states
// [12][M] and one chunk of extended helper columns [chunk_proofs helper_cols][M].  lde: the LDE's own scratch, twice what is extended at
// once: one proof's helper columns (resident), one chunk (streamed: ONE LDE call per chunk, as the prove's gather of a streamed member
// extends it, so the call grows the LDE's scratch to what the prove needs anyway and launches 1 / chunk_proofs as many transforms).
struct ShaScratch { size_t pre_b, ext_b, lev_b, quot_b, state_b, chunk_b, want, lde; };
static ShaScratch sha_scratch_plan(const ShaSet& d, uint32_t log_m, uint32_t log_blowup, uint32_t h, uint32_t n_proofs, uint32_t chunk_proofs) {
  const bool streamed = chunk_proofs < n_proofs;
  const size_t n_hcols = (size_t)n_proofs * d.helper_cols, chunk_cols = (size_t)chunk_proofs * d.helper_cols;
  ShaScratch P;
  P.pre_b = (n_hcols << (log_m - log_blowup)) * 8;
  P.ext_b = streamed ? 0 : (n_hcols << log_m) * 8;
  P.lev_b = (size_t)tmx_poseidon_merkle_digests(log_m, h) * 32;
  P.quot_b = ((size_t)2 << log_m) * 8;
  P.state_b = streamed ? ((size_t)12 << log_m) * 8 : 0;
  P.chunk_b = streamed ? (chunk_cols << log_m) * 8 : 0;
  P.want = P.pre_b + P.ext_b + 2 * P.lev_b + P.quot_b + P.state_b + P.chunk_b;
  P.lde = 2 * (streamed ? P.chunk_b : ((size_t)d.helper_cols << log_m) * 8);
  return P;
}

// what a chunk size must satisfy whatever the set holds; null: it does
static const char* sha_chunk_refusal(const ShaSet& d, uint32_t chunk_proofs) {
  if (chunk_proofs < 1) return "chunk_proofs must be at least 1";
  if (((uint64_t)chunk_proofs * d.helper_cols) % 8)
    return "chunk_proofs times the helper's columns per proof must be a multiple of 8 (the sponge absorbs eight columns at a time)";
  return nullptr;
}

// chunk_proofs = 0: the resident calls.  Else tmx_trace_commit_set_air_sha256_streamed_device (sets 3 - 5) or
// tmx_trace_commit_set_air_sha512_streamed_device (sets 7 - 9): the helper streamed in chunks of chunk_proofs whole proofs, or resident
// exactly as from the resident calls if one chunk holds it all.  The pair goes behind every pair of a lower set that follows the table,
// and the calls of lower sets insert in front of later members: every order ends as table, H3, Q3, ..., H6, Q6 (T.2: H7, Q7, ..., H9, Q9).
static int32_t sha_set_call(tmx_ctx* c, const ShaSet& d, uint32_t section, uint32_t chunk_proofs, bool by_chunks, const uint64_t* d_pub,
                            uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  int32_t st = tmx_trace_commit_set_shape(c, nullptr, nullptr);
  if (st) return st;
  if (by_chunks)
    if (const char* why = sha_chunk_refusal(d, chunk_proofs)) return fail(c, TMX_ERR_BAD_ARG, why);
  const int slot = d.has_periodic ? (section == TMX_TRACE_SHA512 ? 0 : -1)
                                  : section == TMX_TRACE_SHA256 ? 0 : section == TMX_TRACE_TREE ? 1 : section == TMX_TRACE_HEADER ? 2 : -1;
  if (slot < 0)
    return fail(c, TMX_ERR_BAD_ARG, d.has_periodic ? "section must be TMX_TRACE_SHA512" : "section must be TMX_TRACE_SHA256, TMX_TRACE_TREE or TMX_TRACE_HEADER");
  if ((d.has_public && !d_pub) || !d_cap_h || !d_cap_q)
    return fail(c, TMX_ERR_BAD_ARG, d.has_public ? "d_pub, d_cap_h and d_cap_q must be set" : "d_cap_h and d_cap_q must be set");
  const uint32_t chain = d.has_chain && section != TMX_TRACE_SHA256;  // T.3 hashes are single blocks, T.5 and T.6 hashes pairs of blocks
  tmx_ctx::SetRec r = c->set;
  uint32_t kt = r.n_oracles;
  for (uint32_t k = 0; k < r.n_oracles; k++)
    if (r.o[k].section == section) kt = k;
  if (kt == r.n_oracles) return fail(c, TMX_ERR_BAD_ARG, "the commit set does not hold that section");
  // the pair goes behind the pairs of every lower-numbered set that follow the table
  uint32_t at = kt + 1;
  for (const ShaSet* lower = SHA_SETS; lower != &d; lower++)
    if (at < r.n_oracles && r.o[at].section == lower->helper_section) at += 2;
  if (at < r.n_oracles && r.o[at].section == d.helper_section) return fail(c, TMX_ERR_BAD_ARG, d.already);
  const tmx_ctx::SetRec::Oracle tabm = r.o[kt];
  if (tabm.streamed) return fail(c, TMX_ERR_BAD_ARG, "a streamed member has no resident extended columns: the helper is not streamed");
  if (r.n_oracles + 2 > TMX_BATCH_MAX_ORACLES) return fail(c, TMX_ERR_BAD_ARG, "the commit set has no room for two more oracles");
  const uint32_t log_m = tabm.log_m, log_sub = log_m - r.log_blowup, n_proofs = tabm.n_cols / d.width, h = std::min(r.cap_height, log_m);
  if ((st = sha_check(c, d, log_m, r.log_blowup, n_proofs, chain))) return st;
  ShaGeo A;
  if ((st = sha_geo(c, d, log_m, r.log_blowup, chain, r.root, r.shift, A))) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCK(c, hipSetDevice(c->cfg.device));
  if ((st = poseidon_ready(c, s))) return st;
  c->air_valid = false;
  if ((st = air_scratch(c, r.log_blowup))) return st;
  if (d.has_public && !d.has_periodic && (st = link_scratch(c, log_m))) return st;
  if (d.has_periodic && (st = sha512_scratch(c, d, log_m, log_sub))) return st;
  // the scratch of this set and section (ShaScratch)
  const bool streamed = by_chunks && chunk_proofs < n_proofs;
  const uint32_t n_hcols = n_proofs * d.helper_cols;
  const uint64_t n_dig = tmx_poseidon_merkle_digests(log_m, h), n_cap = 1ull << h;
  const ShaScratch SP = sha_scratch_plan(d, log_m, r.log_blowup, h, n_proofs, streamed ? chunk_proofs : n_proofs);
  const size_t pre_b = SP.pre_b, ext_b = SP.ext_b, lev_b = SP.lev_b, quot_b = SP.quot_b, want = SP.want;
  void*& d_scratch = c->d_set_sha[d.scratch][slot];
  size_t& scratch_bytes = c->set_sha_bytes[d.scratch][slot];
  // (a streamed call keeps exactly what it needs: a larger scratch left by a resident call is given back, which is what streaming is for)
  if (streamed ? scratch_bytes != want : scratch_bytes < want) {
    if (d_scratch) { HIPCK(c, hipStreamSynchronize(s)); HIPCK(c, hipFree(d_scratch)); d_scratch = nullptr; scratch_bytes = 0; }
    size_t free_b = 0, total_b = 0;
    if (streamed && hipMemGetInfo(&free_b, &total_b) == hipSuccess && want + SP.lde > free_b + c->ntt_tmp_bytes)
      return fail(c, TMX_ERR_CAPACITY, "the streamed " + std::string(d.word) + " member needs " + std::to_string((want + SP.lde) >> 20) +
                                           " MiB of scratch, the LDE's own included, " + std::to_string(free_b >> 20) + " MiB free");
    if (!streamed && hipMemGetInfo(&free_b, &total_b) == hipSuccess && want > free_b)
      return fail(c, TMX_ERR_CAPACITY, "the " + std::string(d.word) + " member needs " + std::to_string(want >> 20) + " MiB of scratch, " +
                                           std::to_string(free_b >> 20) + " MiB free");
    HIPCK(c, hipMalloc(&d_scratch, want));
    scratch_bytes = want;
  }
  const uint8_t* base = reinterpret_cast<const uint8_t*>(c->d_set);
  uint8_t* sb = reinterpret_cast<uint8_t*>(d_scratch);
  uint64_t* hpre = reinterpret_cast<uint64_t*>(sb);
  uint64_t* hext = reinterpret_cast<uint64_t*>(sb + pre_b);
  uint64_t* lev_h = reinterpret_cast<uint64_t*>(sb + pre_b + ext_b);
  uint64_t* quot = reinterpret_cast<uint64_t*>(sb + pre_b + ext_b + lev_b);
  uint64_t* lev_q = reinterpret_cast<uint64_t*>(sb + pre_b + ext_b + lev_b + quot_b);
  const uint64_t* lev_t = reinterpret_cast<const uint64_t*>(base + tabm.lev_off);
  const int rc = sha_helper_launch(d, log_sub, n_proofs, chain, base + tabm.cols_off, d_pub, hpre, s);
  if (rc) return sha_launch_failed(c, d, "helper", rc);
  if (streamed) {
    // The helper never exists extended.  Sweep 1: chunk by chunk, extended into the chunk buffer and absorbed into the rows' sponge states;
    // the last chunk leaves the leaf digests where k_poseidon_leaves would, the levels above them are the resident path's.  Then gamma
    // and, sweep 2, every chunk extended again and its piece of the quotient added to quot (the first piece writes).  Both sweeps run
    // under the set's domain: put back for the call if tmx_ntt_set_domain moved the context's, restored after.
    uint64_t* state = reinterpret_cast<uint64_t*>(sb + pre_b + 2 * lev_b + quot_b);
    uint64_t* chunk = reinterpret_cast<uint64_t*>(sb + pre_b + 2 * lev_b + quot_b + SP.state_b);
    const uint64_t* tcols = reinterpret_cast<const uint64_t*>(base + tabm.lde_off);
    auto extend = [&](uint32_t p0, uint32_t n) {
      return tmx_lde_goldilocks_device(c, log_sub, r.log_blowup, n * d.helper_cols, hpre + (((uint64_t)p0 * d.helper_cols) << log_sub), chunk, hip_stream);
    };
    auto sweeps = [&]() -> int32_t {
      int32_t e;
      for (uint32_t p0 = 0; p0 < n_proofs; p0 += chunk_proofs) {
        const uint32_t n = std::min(chunk_proofs, n_proofs - p0);
        if ((e = extend(p0, n))) return e;
        const int lrc = launch_poseidon_leaves_chunk(c->d_pos_consts, c->pos_mode, log_m, n * d.helper_cols, chunk, p0 == 0, p0 + n == n_proofs, state,
                                                     lev_h, s);
        if (lrc) return fail(c, TMX_ERR_HIP, std::string("k_poseidon_leaves_chunk launch: ") + hipGetErrorString((hipError_t)lrc));
      }
      uint64_t* cur = lev_h;
      for (uint32_t l = 0; l + h < log_m; l++) {
        const uint64_t cnt = 1ull << (log_m - l);
        const int lrc = launch_poseidon_level(c->d_pos_consts, c->pos_mode, cnt / 2, cur, cur + 4 * cnt, s);
        if (lrc) return fail(c, TMX_ERR_HIP, std::string("k_poseidon_level launch: ") + hipGetErrorString((hipError_t)lrc));
        cur += 4 * cnt;
      }
      HIPCK(c, hipMemcpyAsync(d_cap_h, lev_h + 4 * (n_dig - n_cap), n_cap * 32, hipMemcpyDeviceToDevice, s));
      if ((e = sha_gamma(c, d, log_m, r.log_blowup, r.cap_height, n_proofs, chain, lev_t + 4 * (n_dig - n_cap), lev_h + 4 * (n_dig - n_cap), d_pub, false,
                         s)))
        return e;
      // (sets 7 - 9: the preprocessed planes every piece of sweep 2 reads, filled and extended once, under the set's domain as the chunks are)
      if (d.has_periodic && (e = sha512_periodic(c, d, log_m, r.log_blowup, hip_stream))) return e;
      for (uint32_t p0 = 0; p0 < n_proofs; p0 += chunk_proofs) {
        const uint32_t n = std::min(chunk_proofs, n_proofs - p0);
        if ((e = extend(p0, n))) return e;
        if ((e = sha_pass(c, d, log_m, r.log_blowup, chain, A, p0, n, tcols + (((uint64_t)p0 * d.width) << log_m), chunk, d_pub, n_proofs,
                          p0 ? AIR_FORM_PIECE_ACC : AIR_FORM_PIECE, quot, s)))
          return e;
      }
      return TMX_OK;
    };
    const uint64_t root = c->ntt_root, shift = c->ntt_shift;
    const bool moved = root != r.root || shift != r.shift;
    if (moved && (st = tmx_ntt_set_domain(c, r.root, r.shift))) return st;
    st = sweeps();
    if (moved) {
      const int32_t back = tmx_ntt_set_domain(c, root, shift);
      if (!st) st = back;
    }
    if (st) return st;
  } else {
    // the helper extended under the set's domain, one proof's columns at a time (the LDE's own scratch is twice what it extends at once)
    const uint64_t root = c->ntt_root, shift = c->ntt_shift;
    const bool moved = root != r.root || shift != r.shift;
    if (moved && (st = tmx_ntt_set_domain(c, r.root, r.shift))) return st;
    for (uint32_t c0 = 0; c0 < n_hcols && !st; c0 += d.helper_cols)
      st = tmx_lde_goldilocks_device(c, log_sub, r.log_blowup, d.helper_cols, hpre + ((uint64_t)c0 << log_sub), hext + ((uint64_t)c0 << log_m), hip_stream);
    if (!st && d.has_periodic) st = sha512_periodic(c, d, log_m, r.log_blowup, hip_stream);
    if (moved) {
      const int32_t back = tmx_ntt_set_domain(c, root, shift);
      if (!st) st = back;
    }
    if (st) return st;
    if ((st = tmx_poseidon_merkle_device(c, log_m, n_hcols, hext, h, lev_h, hip_stream))) return st;
    HIPCK(c, hipMemcpyAsync(d_cap_h, lev_h + 4 * (n_dig - n_cap), n_cap * 32, hipMemcpyDeviceToDevice, s));
    if ((st = sha_gamma(c, d, log_m, r.log_blowup, r.cap_height, n_proofs, chain, lev_t + 4 * (n_dig - n_cap), lev_h + 4 * (n_dig - n_cap), d_pub, false,
                        s)))
      return st;
    if ((st = sha_pass(c, d, log_m, r.log_blowup, chain, A, 0, n_proofs, reinterpret_cast<const uint64_t*>(base + tabm.lde_off), hext, d_pub, n_proofs,
                       AIR_FORM_WHOLE, quot, s)))
      return st;
  }
  HIPCK(c, hipEventRecord(c->ev_air, s));
  c->air_valid = true;
  if ((st = tmx_poseidon_merkle_device(c, log_m, 2, quot, h, lev_q, hip_stream))) return st;
  HIPCK(c, hipMemcpyAsync(d_cap_q, lev_q + 4 * (n_dig - n_cap), n_cap * 32, hipMemcpyDeviceToDevice, s));
  for (uint32_t k = r.n_oracles + 1; k >= at + 2; k--) r.o[k] = r.o[k - 2];
  r.o[at] = {d.helper_section, log_m, n_hcols, 0, pre_b, pre_b + ext_b, streamed, false, sb};
  if (streamed) { r.o[at].chunk_cols = chunk_proofs * d.helper_cols; r.o[at].chunk_off = pre_b + 2 * lev_b + quot_b + SP.state_b; }
  r.o[at + 1] = {d.quotient_section, log_m, 2, 0, pre_b + ext_b + lev_b, pre_b + ext_b + lev_b + quot_b, false, true, sb};
  r.n_oracles += 2;
  c->set = r;
  return TMX_OK;
}

extern "C" {

int32_t tmx_air_sha256_helper_device(tmx_ctx* c, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, uint64_t* d_helper, void* hip_stream) {
  return sha_helper_call(c, SHA_SETS[0], log_rows, n_proofs, 0, d_table, nullptr, d_helper, hip_stream);
}

int32_t tmx_air_sha256_quotient_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs, const uint64_t* d_cols,
                                       const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper, uint64_t* d_quot,
                                       void* hip_stream) {
  return sha_quotient_call(c, SHA_SETS[0], log_n, log_blowup, cap_height, n_proofs, 0, 0, n_proofs, AIR_FORM_WHOLE, d_cols, d_helper_cols, d_cap,
                           d_cap_helper, nullptr, d_quot, hip_stream);
}

// (the helper sits directly behind the table; a k_trace + 1 that wraps to 0 fails the index rule as it should)
int32_t tmx_air_sha256_verify_device(tmx_ctx* c, const tmx_batch_params* p, uint32_t k_trace, const uint64_t* d_caps, const uint64_t* d_proof,
                                     uint32_t* d_ok, void* hip_stream) {
  return sha_verify_call(c, SHA_SETS[0], p, k_trace, k_trace + 1, 0, d_caps, d_proof, nullptr, d_ok, hip_stream);
}

int32_t tmx_trace_commit_set_air_sha256_device(tmx_ctx* c, uint32_t section, uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream) {
  return sha_set_call(c, SHA_SETS[0], section, 0, false, nullptr, d_cap_h, d_cap_q, hip_stream);
}

int32_t tmx_air_sha256_sched_helper_device(tmx_ctx* c, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, uint64_t* d_helper,
                                           void* hip_stream) {
  return sha_helper_call(c, SHA_SETS[1], log_rows, n_proofs, 0, d_table, nullptr, d_helper, hip_stream);
}

int32_t tmx_air_sha256_sched_quotient_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                             const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap,
                                             const uint64_t* d_cap_helper, uint64_t* d_quot, void* hip_stream) {
  return sha_quotient_call(c, SHA_SETS[1], log_n, log_blowup, cap_height, n_proofs, 0, 0, n_proofs, AIR_FORM_WHOLE, d_cols, d_helper_cols, d_cap,
                           d_cap_helper, nullptr, d_quot, hip_stream);
}

int32_t tmx_air_sha256_sched_verify_device(tmx_ctx* c, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, const uint64_t* d_caps,
                                           const uint64_t* d_proof, uint32_t* d_ok, void* hip_stream) {
  return sha_verify_call(c, SHA_SETS[1], p, k_trace, k_helper, 0, d_caps, d_proof, nullptr, d_ok, hip_stream);
}

int32_t tmx_trace_commit_set_air_sha256_sched_device(tmx_ctx* c, uint32_t section, uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream) {
  return sha_set_call(c, SHA_SETS[1], section, 0, false, nullptr, d_cap_h, d_cap_q, hip_stream);
}

int32_t tmx_air_sha256_init_helper_device(tmx_ctx* c, uint32_t log_rows, uint32_t n_proofs, uint32_t chain, const uint64_t* d_table,
                                          uint64_t* d_helper, void* hip_stream) {
  return sha_helper_call(c, SHA_SETS[2], log_rows, n_proofs, chain, d_table, nullptr, d_helper, hip_stream);
}

int32_t tmx_air_sha256_init_quotient_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs, uint32_t chain,
                                            const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap,
                                            const uint64_t* d_cap_helper, uint64_t* d_quot, void* hip_stream) {
  return sha_quotient_call(c, SHA_SETS[2], log_n, log_blowup, cap_height, n_proofs, chain, 0, n_proofs, AIR_FORM_WHOLE, d_cols, d_helper_cols, d_cap,
                           d_cap_helper, nullptr, d_quot, hip_stream);
}

int32_t tmx_air_sha256_init_verify_device(tmx_ctx* c, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, uint32_t chain,
                                          const uint64_t* d_caps, const uint64_t* d_proof, uint32_t* d_ok, void* hip_stream) {
  return sha_verify_call(c, SHA_SETS[2], p, k_trace, k_helper, chain, d_caps, d_proof, nullptr, d_ok, hip_stream);
}

int32_t tmx_trace_commit_set_air_sha256_init_device(tmx_ctx* c, uint32_t section, uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream) {
  return sha_set_call(c, SHA_SETS[2], section, 0, false, nullptr, d_cap_h, d_cap_q, hip_stream);
}

int32_t tmx_air_sha256_quotient_range_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs, uint32_t proof_lo,
                                             uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols, const uint64_t* d_helper_cols,
                                             const uint64_t* d_cap, const uint64_t* d_cap_helper, uint64_t* d_quot, void* hip_stream) {
  return sha_quotient_range_call(c, SHA_SETS[0], log_n, log_blowup, cap_height, n_proofs, 0, proof_lo, proof_hi, accumulate, d_cols, d_helper_cols, d_cap,
                                 d_cap_helper, nullptr, d_quot, hip_stream);
}

int32_t tmx_air_sha256_sched_quotient_range_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                   uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                   const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                                   uint64_t* d_quot, void* hip_stream) {
  return sha_quotient_range_call(c, SHA_SETS[1], log_n, log_blowup, cap_height, n_proofs, 0, proof_lo, proof_hi, accumulate, d_cols, d_helper_cols, d_cap,
                                 d_cap_helper, nullptr, d_quot, hip_stream);
}

int32_t tmx_air_sha256_init_quotient_range_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs, uint32_t chain,
                                                  uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                  const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                                  uint64_t* d_quot, void* hip_stream) {
  return sha_quotient_range_call(c, SHA_SETS[2], log_n, log_blowup, cap_height, n_proofs, chain, proof_lo, proof_hi, accumulate, d_cols, d_helper_cols,
                                 d_cap, d_cap_helper, nullptr, d_quot, hip_stream);
}

int32_t tmx_trace_commit_set_air_sha256_link_device(tmx_ctx* c, uint32_t section, const uint64_t* d_pub, uint64_t* d_cap_h, uint64_t* d_cap_q,
                                                    void* hip_stream) {
  return sha_set_call(c, SHA_SETS[3], section, 0, false, d_pub, d_cap_h, d_cap_q, hip_stream);
}

int32_t tmx_air_sha256_link_quotient_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                            const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap,
                                            const uint64_t* d_cap_helper, const uint64_t* d_pub, uint64_t* d_quot, void* hip_stream) {
  return sha_quotient_call(c, SHA_SETS[3], log_n, log_blowup, cap_height, n_proofs, 0, 0, n_proofs, AIR_FORM_WHOLE, d_cols, d_helper_cols, d_cap,
                           d_cap_helper, d_pub, d_quot, hip_stream);
}

int32_t tmx_air_sha256_link_quotient_range_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                  uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                  const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                                  const uint64_t* d_pub, uint64_t* d_quot, void* hip_stream) {
  return sha_quotient_range_call(c, SHA_SETS[3], log_n, log_blowup, cap_height, n_proofs, 0, proof_lo, proof_hi, accumulate, d_cols, d_helper_cols, d_cap,
                                 d_cap_helper, d_pub, d_quot, hip_stream);
}

int32_t tmx_air_sha256_link_verify_device(tmx_ctx* c, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, const uint64_t* d_caps,
                                          const uint64_t* d_proof, const uint64_t* d_pub, uint32_t* d_ok, void* hip_stream) {
  return sha_verify_call(c, SHA_SETS[3], p, k_trace, k_helper, 0, d_caps, d_proof, d_pub, d_ok, hip_stream);
}

// ---- the public table of a SHA-256 table from element rows, and the helper oracle over it
int32_t tmx_air_sha256_public_shape(int32_t kind, uint32_t section, uint32_t n_max, uint32_t n_proofs, uint32_t* log_k, uint32_t* n_cols) {
  uint32_t log_rows = 0, width = 0;
  if (section != TMX_TRACE_SHA256 && section != TMX_TRACE_TREE && section != TMX_TRACE_HEADER) return TMX_ERR_BAD_ARG;
  if (n_proofs < 1 || tmx_trace_commit_shape(kind, n_max, section, &log_rows, &width) != TMX_OK) return TMX_ERR_BAD_ARG;
  if (log_rows < 6 + AIR_SHA_PUBLIC_MIN_LOG_K || log_rows > 6 + AIR_SHA_PUBLIC_MAX_LOG_K) return TMX_ERR_BAD_ARG;
  if ((uint64_t)n_proofs * AIR_LINK_HELPER_COLS > TMX_DEEP_MAX_COLS) return TMX_ERR_BAD_ARG;
  if (log_k) *log_k = log_rows - 6;
  if (n_cols) *n_cols = AIR_SHA_PUBLIC_WIDTH * n_proofs;
  return TMX_OK;
}

int32_t tmx_air_sha256_public_device(tmx_ctx* c, int32_t kind, uint32_t section, uint32_t n_proofs, const void* d_elems, uint64_t* d_pub,
                                     void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP) return fail(c, TMX_ERR_BAD_ARG, "kind must be TMX_KIND_SKIP or TMX_KIND_STEP");
  if (section != TMX_TRACE_SHA256 && section != TMX_TRACE_TREE && section != TMX_TRACE_HEADER)
    return fail(c, TMX_ERR_BAD_ARG, "section must be TMX_TRACE_SHA256, TMX_TRACE_TREE or TMX_TRACE_HEADER");
  uint32_t log_k = 0;
  if (tmx_air_sha256_public_shape(kind, section, c->cfg.n_max, n_proofs, &log_k, nullptr))
    return fail(c, TMX_ERR_BAD_ARG, "n_proofs must be at least 1 (33 n_proofs at most 2^24) and the table 2 .. 2^12 blocks");
  if (!d_elems || !d_pub) return fail(c, TMX_ERR_BAD_ARG, "d_elems and d_pub must be set");
  HIPCK(c, hipSetDevice(c->cfg.device));
  const Program& prog = c->prog[kind];
  const SerializeProgram& sp = prog.sp;
  AirShaPublicGeom G = prog.pub;  // (every offset as build_program recorded it)
  G.elem_stride = sp.elem_stride; G.kind = (uint32_t)kind; G.section = section; G.n = c->cfg.n_max; G.tn = sp.tree_nodes;
  const int rc = launch_air_sha_public_gather(d_elems, G, log_k, n_proofs, d_pub, hip_stream);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_sha_public_gather launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

int32_t tmx_air_sha256_link_helper_device(tmx_ctx* c, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, const uint64_t* d_pub,
                                          uint64_t* d_helper, void* hip_stream) {
  return sha_helper_call(c, SHA_SETS[3], log_rows, n_proofs, 0, d_table, d_pub, d_helper, hip_stream);
}

// ---- the public table of the SHA-512 table from element rows, and the helper oracle over it (constraint set 10)
int32_t tmx_air_sha512_public_shape(int32_t kind, uint32_t n_max, uint32_t n_proofs, uint32_t* log_k, uint32_t* n_cols) {
  uint32_t log_rows = 0, width = 0;
  if (n_proofs < 1 || tmx_trace_commit_shape(kind, n_max, TMX_TRACE_SHA512, &log_rows, &width) != TMX_OK) return TMX_ERR_BAD_ARG;
  if (log_rows < 7 || log_rows > 18) return TMX_ERR_BAD_ARG;
  if ((uint64_t)n_proofs * AIR_SHA512_LINK_HELPER_COLS > TMX_DEEP_MAX_COLS) return TMX_ERR_BAD_ARG;
  if (log_k) *log_k = air_sha512_public_log_k(log_rows);
  if (n_cols) *n_cols = AIR_SHA512_PUBLIC_WIDTH * n_proofs;
  return TMX_OK;
}

int32_t tmx_air_sha512_public_device(tmx_ctx* c, int32_t kind, uint32_t n_proofs, const void* d_elems, uint64_t* d_pub, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (kind != TMX_KIND_SKIP && kind != TMX_KIND_STEP) return fail(c, TMX_ERR_BAD_ARG, "kind must be TMX_KIND_SKIP or TMX_KIND_STEP");
  uint32_t log_k = 0;
  if (tmx_air_sha512_public_shape(kind, c->cfg.n_max, n_proofs, &log_k, nullptr))
    return fail(c, TMX_ERR_BAD_ARG, "n_proofs must be at least 1 (65 n_proofs at most 2^24) and the table 2^7 .. 2^18 rows");
  if (!d_elems || !d_pub) return fail(c, TMX_ERR_BAD_ARG, "d_elems and d_pub must be set");
  HIPCK(c, hipSetDevice(c->cfg.device));
  const Program& prog = c->prog[kind];
  AirSha512PublicGeom G = prog.pub512;  // (every offset as build_program recorded it)
  G.elem_stride = prog.sp.elem_stride; G.n = c->cfg.n_max;
  const int rc = launch_air_sha512_public_gather(d_elems, G, log_k, n_proofs, d_pub, hip_stream);
  if (rc) return fail(c, TMX_ERR_HIP, std::string("k_air_sha512_public_gather launch: ") + hipGetErrorString((hipError_t)rc));
  return TMX_OK;
}

int32_t tmx_air_sha512_link_helper_device(tmx_ctx* c, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, const uint64_t* d_pub,
                                          uint64_t* d_helper, void* hip_stream) {
  return sha_helper_call(c, SHA_SETS[7], log_rows, n_proofs, 0, d_table, d_pub, d_helper, hip_stream);
}

// ---- constraint set 10 through row 7 of the host path above
int32_t tmx_air_sha512_link_quotient_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                            const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap,
                                            const uint64_t* d_cap_helper, const uint64_t* d_pub, uint64_t* d_quot, void* hip_stream) {
  return sha_quotient_call(c, SHA_SETS[7], log_n, log_blowup, cap_height, n_proofs, 0, 0, n_proofs, AIR_FORM_WHOLE, d_cols, d_helper_cols, d_cap,
                           d_cap_helper, d_pub, d_quot, hip_stream);
}

int32_t tmx_air_sha512_link_quotient_range_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                  uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                  const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                                  const uint64_t* d_pub, uint64_t* d_quot, void* hip_stream) {
  return sha_quotient_range_call(c, SHA_SETS[7], log_n, log_blowup, cap_height, n_proofs, 0, proof_lo, proof_hi, accumulate, d_cols, d_helper_cols, d_cap,
                                 d_cap_helper, d_pub, d_quot, hip_stream);
}

int32_t tmx_air_sha512_link_verify_device(tmx_ctx* c, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, const uint64_t* d_caps,
                                          const uint64_t* d_proof, const uint64_t* d_pub, uint32_t* d_ok, void* hip_stream) {
  return sha_verify_call(c, SHA_SETS[7], p, k_trace, k_helper, 0, d_caps, d_proof, d_pub, d_ok, hip_stream);
}

int32_t tmx_trace_commit_set_air_sha512_link_device(tmx_ctx* c, uint32_t section, const uint64_t* d_pub, uint64_t* d_cap_h, uint64_t* d_cap_q,
                                                    void* hip_stream) {
  return sha_set_call(c, SHA_SETS[7], section, 0, false, d_pub, d_cap_h, d_cap_q, hip_stream);
}

// The public side on its own, for tests: V (planar, 2 << log_rows words at d_v) from d_pub and the two words at d_gamma, and, extended
// under the current NTT domain, Pub_gamma on the coset (2 << (log_rows + log_blowup) words at d_ext; log_blowup = 0: d_v alone)
int32_t tmx_air_sha512_link_public_side_device(tmx_ctx* c, uint32_t log_rows, uint32_t log_blowup, uint32_t n_proofs, const uint64_t* d_pub,
                                               const uint64_t* d_gamma, uint64_t* d_v, uint64_t* d_ext, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  const ShaSet& d = SHA_SETS[7];
  if (log_rows < d.rows_lo || log_rows > d.rows_hi) return fail(c, TMX_ERR_BAD_ARG, d.bad_rows);
  if (log_blowup > 6) return fail(c, TMX_ERR_BAD_ARG, "log_blowup must be at most 6");
  if (n_proofs < 1 || (uint64_t)n_proofs * d.helper_cols > TMX_DEEP_MAX_COLS) return fail(c, TMX_ERR_BAD_ARG, "n_proofs must be at least 1 and " + sha_too_many_cols(d));
  if (!d_pub || !d_gamma || !d_v || (log_blowup && !d_ext)) return fail(c, TMX_ERR_BAD_ARG, "d_pub, d_gamma and d_v must be set, and d_ext unless log_blowup is 0");
  HIPCK(c, hipSetDevice(c->cfg.device));
  const int rc = launch_air_sha512_link_combine(log_rows, n_proofs, d_pub, d_gamma, d_v, hip_stream);
  if (rc) return sha_launch_failed(c, d, "combine", rc);
  return log_blowup ? tmx_lde_goldilocks_device(c, log_rows, log_blowup, 2, d_v, d_ext, hip_stream) : TMX_OK;
}

// d_out[0 .. 2) = Pub_gamma(zeta) from V at d_v (2 << log_rows words) and the two words at d_zeta, d_out[2] = 1 if a denominator was zero
int32_t tmx_air_sha512_link_public_eval_device(tmx_ctx* c, uint32_t log_rows, const uint64_t* d_v, const uint64_t* d_zeta, uint64_t* d_out,
                                               void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  const ShaSet& d = SHA_SETS[7];
  if (log_rows < d.rows_lo || log_rows > d.rows_hi) return fail(c, TMX_ERR_BAD_ARG, d.bad_rows);
  if (!d_v || !d_zeta || !d_out) return fail(c, TMX_ERR_BAD_ARG, "d_v, d_zeta and d_out must be set");
  HIPCK(c, hipSetDevice(c->cfg.device));
  int32_t st = sha512_scratch(c, d, 0, 0);
  if (st) return st;
  const uint64_t P = 0xffffffff00000001ull, om = gl_pow_host(c->ntt_root, 1ull << (32 - log_rows)), n_inv = gl_pow_host(1ull << log_rows, P - 2);
  uint64_t* pub_part = reinterpret_cast<uint64_t*>(c->d_air10) + LINK512_OFF_PUB_PART;
  int rc = launch_air_sha512_link_public_eval(log_rows, om, d_zeta, d_v, pub_part, hip_stream);
  if (rc) return sha_launch_failed(c, d, "public_eval", rc);
  rc = launch_air_sha512_link_public_fold(log_rows, n_inv, pub_part, d_zeta, d_out, hip_stream);
  if (rc) return sha_launch_failed(c, d, "public_fold", rc);
  return TMX_OK;
}

uint64_t tmx_trace_commit_set_air_sha256_streamed_bytes(uint32_t constraint_set, uint32_t log_m, uint32_t log_blowup, uint32_t cap_height,
                                                        uint32_t n_proofs, uint32_t chunk_proofs, uint64_t* lde_scratch_bytes) {
  if (lde_scratch_bytes) *lde_scratch_bytes = 0;
  if (constraint_set < 3 || constraint_set > 5) return 0;
  const ShaSet& d = SHA_SETS[constraint_set - 3];
  if (sha_chunk_refusal(d, chunk_proofs) || sha_check(nullptr, d, log_m, log_blowup, n_proofs, 0)) return 0;
  const ShaScratch SP = sha_scratch_plan(d, log_m, log_blowup, std::min(cap_height, log_m), n_proofs, std::min(chunk_proofs, n_proofs));
  if (lde_scratch_bytes) *lde_scratch_bytes = SP.lde;
  return SP.want;
}

int32_t tmx_trace_commit_set_air_sha256_streamed_device(tmx_ctx* c, uint32_t constraint_set, uint32_t section, uint32_t chunk_proofs, uint64_t* d_cap_h,
                                                        uint64_t* d_cap_q, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (constraint_set < 3 || constraint_set > 5) return fail(c, TMX_ERR_BAD_ARG, "constraint_set must be 3, 4 or 5");
  return sha_set_call(c, SHA_SETS[constraint_set - 3], section, chunk_proofs, true, nullptr, d_cap_h, d_cap_q, hip_stream);
}

uint64_t tmx_trace_commit_set_air_sha256_scratch_bytes(const tmx_ctx* c, uint32_t constraint_set, uint32_t section) {
  if (!c || constraint_set < 3 || constraint_set > 5) return 0;
  const int slot = section == TMX_TRACE_SHA256 ? 0 : section == TMX_TRACE_TREE ? 1 : section == TMX_TRACE_HEADER ? 2 : -1;
  if (slot < 0) return 0;
  return c->set_sha_bytes[SHA_SETS[constraint_set - 3].scratch][slot];
}

// ---- streamed helpers of the SHA-512 sets: rows 4 - 6 of the host path above through its streamed branch, under names of their own (the
// SHA-256 names keep refusing every set but 3, 4 and 5)
uint64_t tmx_trace_commit_set_air_sha512_streamed_bytes(uint32_t constraint_set, uint32_t log_m, uint32_t log_blowup, uint32_t cap_height,
                                                        uint32_t n_proofs, uint32_t chunk_proofs, uint64_t* lde_scratch_bytes) {
  if (lde_scratch_bytes) *lde_scratch_bytes = 0;
  if (constraint_set < 7 || constraint_set > 9) return 0;
  const ShaSet& d = SHA_SETS[constraint_set - 3];
  if (sha_chunk_refusal(d, chunk_proofs) || sha_check(nullptr, d, log_m, log_blowup, n_proofs, 0)) return 0;
  const ShaScratch SP = sha_scratch_plan(d, log_m, log_blowup, std::min(cap_height, log_m), n_proofs, std::min(chunk_proofs, n_proofs));
  if (lde_scratch_bytes) *lde_scratch_bytes = SP.lde;
  return SP.want;
}

int32_t tmx_trace_commit_set_air_sha512_streamed_device(tmx_ctx* c, uint32_t constraint_set, uint32_t section, uint32_t chunk_proofs, uint64_t* d_cap_h,
                                                        uint64_t* d_cap_q, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (constraint_set < 7 || constraint_set > 9) return fail(c, TMX_ERR_BAD_ARG, "constraint_set must be 7, 8 or 9");
  return sha_set_call(c, SHA_SETS[constraint_set - 3], section, chunk_proofs, true, nullptr, d_cap_h, d_cap_q, hip_stream);
}

uint64_t tmx_trace_commit_set_air_sha512_scratch_bytes(const tmx_ctx* c, uint32_t constraint_set, uint32_t section) {
  if (!c || constraint_set < 7 || constraint_set > 9 || section != TMX_TRACE_SHA512) return 0;
  return c->set_sha_bytes[SHA_SETS[constraint_set - 3].scratch][0];
}

// ---- constraint set 7: the round constraints of the SHA-512 table, through row 4 of the host path above
int32_t tmx_air_sha512_helper_device(tmx_ctx* c, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, uint64_t* d_helper, void* hip_stream) {
  return sha_helper_call(c, SHA_SETS[4], log_rows, n_proofs, 0, d_table, nullptr, d_helper, hip_stream);
}

int32_t tmx_air_sha512_quotient_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs, const uint64_t* d_cols,
                                       const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper, uint64_t* d_quot,
                                       void* hip_stream) {
  return sha_quotient_call(c, SHA_SETS[4], log_n, log_blowup, cap_height, n_proofs, 0, 0, n_proofs, AIR_FORM_WHOLE, d_cols, d_helper_cols, d_cap,
                           d_cap_helper, nullptr, d_quot, hip_stream);
}

int32_t tmx_air_sha512_quotient_range_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs, uint32_t proof_lo,
                                             uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols, const uint64_t* d_helper_cols,
                                             const uint64_t* d_cap, const uint64_t* d_cap_helper, uint64_t* d_quot, void* hip_stream) {
  return sha_quotient_range_call(c, SHA_SETS[4], log_n, log_blowup, cap_height, n_proofs, 0, proof_lo, proof_hi, accumulate, d_cols, d_helper_cols, d_cap,
                                 d_cap_helper, nullptr, d_quot, hip_stream);
}

int32_t tmx_air_sha512_verify_device(tmx_ctx* c, const tmx_batch_params* p, uint32_t k_trace, const uint64_t* d_caps, const uint64_t* d_proof,
                                     uint32_t* d_ok, void* hip_stream) {
  return sha_verify_call(c, SHA_SETS[4], p, k_trace, k_trace + 1, 0, d_caps, d_proof, nullptr, d_ok, hip_stream);
}

int32_t tmx_trace_commit_set_air_sha512_device(tmx_ctx* c, uint32_t section, uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream) {
  return sha_set_call(c, SHA_SETS[4], section, 0, false, nullptr, d_cap_h, d_cap_q, hip_stream);
}

}  // extern "C"

// the preprocessed columns of set 7, 8 or 9 on their own: what the quotient call fills and extends, and what the verifier evaluates
static int32_t sha_periodic_call(tmx_ctx* c, const ShaSet& d, uint32_t log_rows, uint32_t log_blowup, uint64_t* d_pre, uint64_t* d_ext, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (log_rows < d.rows_lo || log_rows > d.rows_hi) return fail(c, TMX_ERR_BAD_ARG, d.bad_rows);
  if (log_blowup > 6) return fail(c, TMX_ERR_BAD_ARG, "log_blowup must be at most 6");
  if (!d_pre || (log_blowup && !d_ext)) return fail(c, TMX_ERR_BAD_ARG, "d_pre must be set, and d_ext unless log_blowup is 0");
  HIPCK(c, hipSetDevice(c->cfg.device));
  const int rc = d.per->k->fill(log_rows, d_pre, hip_stream);
  if (rc) return sha_launch_failed(c, d, "periodic", rc);
  return log_blowup ? tmx_lde_goldilocks_device(c, log_rows, log_blowup, d.per->planes, d_pre, d_ext, hip_stream) : TMX_OK;
}

static int32_t sha_periodic_eval_call(tmx_ctx* c, const ShaSet& d, uint32_t log_rows, const uint64_t* d_zeta, uint64_t* d_out, void* hip_stream) {
  if (!c) return TMX_ERR_BAD_ARG;
  if (log_rows < d.rows_lo || log_rows > d.rows_hi) return fail(c, TMX_ERR_BAD_ARG, d.bad_rows);
  if (!d_zeta || !d_out) return fail(c, TMX_ERR_BAD_ARG, "d_zeta and d_out must be set");
  HIPCK(c, hipSetDevice(c->cfg.device));
  int32_t st = sha512_scratch(c, d, 0, 0);
  if (st) return st;
  const uint64_t P = 0xffffffff00000001ull, om = gl_pow_host(c->ntt_root, 1ull << (32 - log_rows)), n_inv = gl_pow_host(1ull << log_rows, P - 2);
  void* part = c->*(d.per->scratch);
  int rc = d.per->k->eval(log_rows, om, d_zeta, part, hip_stream);
  if (rc) return sha_launch_failed(c, d, "periodic_eval", rc);
  rc = d.per->k->fold(log_rows, n_inv, part, d_zeta, d_out, hip_stream);
  if (rc) return sha_launch_failed(c, d, "periodic_fold", rc);
  return TMX_OK;
}

extern "C" {

int32_t tmx_air_sha512_periodic_device(tmx_ctx* c, uint32_t log_rows, uint32_t log_blowup, uint64_t* d_pre, uint64_t* d_ext, void* hip_stream) {
  return sha_periodic_call(c, SHA_SETS[4], log_rows, log_blowup, d_pre, d_ext, hip_stream);
}

int32_t tmx_air_sha512_periodic_eval_device(tmx_ctx* c, uint32_t log_rows, const uint64_t* d_zeta, uint64_t* d_out, void* hip_stream) {
  return sha_periodic_eval_call(c, SHA_SETS[4], log_rows, d_zeta, d_out, hip_stream);
}

// (set 10's planes STA, CHN, SEL, E79, MSG on their own; the rest of set 10 stands with its public table further up)
int32_t tmx_air_sha512_link_periodic_device(tmx_ctx* c, uint32_t log_rows, uint32_t log_blowup, uint64_t* d_pre, uint64_t* d_ext, void* hip_stream) {
  return sha_periodic_call(c, SHA_SETS[7], log_rows, log_blowup, d_pre, d_ext, hip_stream);
}

int32_t tmx_air_sha512_link_periodic_eval_device(tmx_ctx* c, uint32_t log_rows, const uint64_t* d_zeta, uint64_t* d_out, void* hip_stream) {
  return sha_periodic_eval_call(c, SHA_SETS[7], log_rows, d_zeta, d_out, hip_stream);
}

// ---- constraint set 8: the message schedule of the SHA-512 table, through row 5 of the host path above
int32_t tmx_air_sha512_sched_helper_device(tmx_ctx* c, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, uint64_t* d_helper,
                                           void* hip_stream) {
  return sha_helper_call(c, SHA_SETS[5], log_rows, n_proofs, 0, d_table, nullptr, d_helper, hip_stream);
}

int32_t tmx_air_sha512_sched_quotient_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                             const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                             uint64_t* d_quot, void* hip_stream) {
  return sha_quotient_call(c, SHA_SETS[5], log_n, log_blowup, cap_height, n_proofs, 0, 0, n_proofs, AIR_FORM_WHOLE, d_cols, d_helper_cols, d_cap,
                           d_cap_helper, nullptr, d_quot, hip_stream);
}

int32_t tmx_air_sha512_sched_quotient_range_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                   uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                   const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper, uint64_t* d_quot,
                                                   void* hip_stream) {
  return sha_quotient_range_call(c, SHA_SETS[5], log_n, log_blowup, cap_height, n_proofs, 0, proof_lo, proof_hi, accumulate, d_cols, d_helper_cols, d_cap,
                                 d_cap_helper, nullptr, d_quot, hip_stream);
}

int32_t tmx_air_sha512_sched_verify_device(tmx_ctx* c, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, const uint64_t* d_caps,
                                           const uint64_t* d_proof, uint32_t* d_ok, void* hip_stream) {
  return sha_verify_call(c, SHA_SETS[5], p, k_trace, k_helper, 0, d_caps, d_proof, nullptr, d_ok, hip_stream);
}

int32_t tmx_trace_commit_set_air_sha512_sched_device(tmx_ctx* c, uint32_t section, uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream) {
  return sha_set_call(c, SHA_SETS[5], section, 0, false, nullptr, d_cap_h, d_cap_q, hip_stream);
}

int32_t tmx_air_sha512_sched_periodic_device(tmx_ctx* c, uint32_t log_rows, uint32_t log_blowup, uint64_t* d_pre, uint64_t* d_ext, void* hip_stream) {
  return sha_periodic_call(c, SHA_SETS[5], log_rows, log_blowup, d_pre, d_ext, hip_stream);
}

int32_t tmx_air_sha512_sched_periodic_eval_device(tmx_ctx* c, uint32_t log_rows, const uint64_t* d_zeta, uint64_t* d_out, void* hip_stream) {
  return sha_periodic_eval_call(c, SHA_SETS[5], log_rows, d_zeta, d_out, hip_stream);
}

// ---- constraint set 9: the block starts of the SHA-512 table, through row 6 of the host path above
int32_t tmx_air_sha512_init_helper_device(tmx_ctx* c, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, uint64_t* d_helper,
                                          void* hip_stream) {
  return sha_helper_call(c, SHA_SETS[6], log_rows, n_proofs, 0, d_table, nullptr, d_helper, hip_stream);
}

int32_t tmx_air_sha512_init_quotient_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                            const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                            uint64_t* d_quot, void* hip_stream) {
  return sha_quotient_call(c, SHA_SETS[6], log_n, log_blowup, cap_height, n_proofs, 0, 0, n_proofs, AIR_FORM_WHOLE, d_cols, d_helper_cols, d_cap,
                           d_cap_helper, nullptr, d_quot, hip_stream);
}

int32_t tmx_air_sha512_init_quotient_range_device(tmx_ctx* c, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                  uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                  const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper, uint64_t* d_quot,
                                                  void* hip_stream) {
  return sha_quotient_range_call(c, SHA_SETS[6], log_n, log_blowup, cap_height, n_proofs, 0, proof_lo, proof_hi, accumulate, d_cols, d_helper_cols, d_cap,
                                 d_cap_helper, nullptr, d_quot, hip_stream);
}

int32_t tmx_air_sha512_init_verify_device(tmx_ctx* c, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, const uint64_t* d_caps,
                                          const uint64_t* d_proof, uint32_t* d_ok, void* hip_stream) {
  return sha_verify_call(c, SHA_SETS[6], p, k_trace, k_helper, 0, d_caps, d_proof, nullptr, d_ok, hip_stream);
}

int32_t tmx_trace_commit_set_air_sha512_init_device(tmx_ctx* c, uint32_t section, uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream) {
  return sha_set_call(c, SHA_SETS[6], section, 0, false, nullptr, d_cap_h, d_cap_q, hip_stream);
}

int32_t tmx_air_sha512_init_periodic_device(tmx_ctx* c, uint32_t log_rows, uint32_t log_blowup, uint64_t* d_pre, uint64_t* d_ext, void* hip_stream) {
  return sha_periodic_call(c, SHA_SETS[6], log_rows, log_blowup, d_pre, d_ext, hip_stream);
}

int32_t tmx_air_sha512_init_periodic_eval_device(tmx_ctx* c, uint32_t log_rows, const uint64_t* d_zeta, uint64_t* d_out, void* hip_stream) {
  return sha_periodic_eval_call(c, SHA_SETS[6], log_rows, d_zeta, d_out, hip_stream);
}

}  // extern "C"
