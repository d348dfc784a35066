/* libtmx -- MI355X-native witness generator for the TendermintX skip / step circuits.  C ABI.
 *
 * This is the drop-in boundary for ONE path of succinctlabs/tendermintx: the value-level witness that the
 * off-chain-input hints produce and the gadget tree consumes.  Reference interfaces replaced:
 *
 *   SkipOffchainInputs::hint   reference circuits/skip.rs:64-102   (reads U64, Bytes32, U64; writes VerifySkipVariable<N>)
 *   StepOffchainInputs::hint   reference circuits/step.rs:56-89    (reads U64, Bytes32;      writes VerifyStepVariable<N>)
 *   InputDataFetcher::get_skip_inputs / get_step_inputs   reference circuits/input/mod.rs:425-523, 316-423
 *   get_validator_data_from_block / validator_hash_field_from_block   reference circuits/input/conversion.rs:59-178
 *   verify_skip / verify_step gadget values   reference circuits/builder/verify.rs:469-563 (+ validator.rs, voting.rs, shared.rs)
 *
 * The Rust host keeps `impl Circuit for SkipCircuit / StepCircuit` (skip.rs:113-143, step.rs:100-127) and
 * bin/skip.rs / bin/step.rs unchanged; only the hint body calls into this library (INTEGRATION.md shows the
 * FFI stub).  All compute below runs in hand-written HIP kernels for gfx950; there is no CPU fallback: every
 * entry point fails with TMX_ERR_HIP if no device is usable.
 *
 * Conventions: every function returns 0 on success or a negative tmx_status; nothing throws across the ABI;
 * the caller owns all buffers passed in; the library never keeps caller pointers after returning; a tmx_ctx is
 * not thread-safe (use one per thread).  Contexts of one device share three internal side streams (the GPU runs four hardware queues:
 * DESIGN.md section 3) and each context owns ONE set of scratch buffers and join events, reused by every call: consecutive
 * tmx_witness_batch_device / tmx_finish_batch_device calls on one context are ordered by the library itself (a call on another stream
 * waits for the end of the previous one); the other *_device entry points (EdDSA lanes, trace rows, NTT) must be stream-ordered by the
 * caller -- the same stream, or an explicit dependency.
 * The host-buffer entry points block until their results are in host memory, so they are ordered by construction.
 */
#ifndef TMX_H
#define TMX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMX_KIND_SKIP 0
#define TMX_KIND_STEP 1

#define TMX_N_MAX_LIMIT 512 /* largest VALIDATOR_SET_SIZE_MAX a context accepts (BASELINE config 5) */

/* reference circuits/consts.rs:9-29 */
#define TMX_VALIDATOR_MESSAGE_BYTES_LENGTH_MAX 124
#define TMX_VALIDATOR_BYTE_LENGTH_MAX 46
#define TMX_PROTOBUF_CHAIN_ID_SIZE_BYTES 52
#define TMX_HEADER_PROOF_DEPTH 4

#define TMX_FLAG_SIGNED 1u  /* CommitSig::is_commit() -- conversion.rs:79 */
#define TMX_FLAG_PRESENT 2u /* lane index < commit.signatures.len() -- conversion.rs:70 vs :118 */

typedef enum {
  TMX_OK = 0,
  TMX_ERR_BAD_ARG = -1,
  TMX_ERR_SET_TOO_LARGE = -2, /* reference input/mod.rs:439-444, 338-342: validator set larger than N */
  TMX_ERR_HIP = -3,           /* no device / HIP runtime error (message in tmx_last_error) */
  TMX_ERR_CAPACITY = -4,      /* output buffer or context batch capacity too small */
  TMX_ERR_PARSE = -5,         /* malformed fixture / RPC JSON */
  TMX_ERR_MSG_TOO_LONG = -6,  /* sign-bytes longer than 124 B -- conversion.rs:52 `try_into().unwrap()` */
  TMX_ERR_RCCL = -7           /* RCCL not loadable / a collective failed (message in tmx_last_error) -- SURVEY 8(b) error convention */
} tmx_status;

/* One lane of `target_block_validators` (ValidatorType, reference circuits/variables.rs:69-79) before
 * field-element expansion.  256 B so that a wavefront's lanes read 16-B aligned, coalescable records. */
typedef struct {
  uint8_t pubkey[32];
  uint8_t signature[64]; /* R || s, s little-endian (conversion.rs:43-46) */
  uint8_t message[TMX_VALIDATOR_MESSAGE_BYTES_LENGTH_MAX]; /* sign-bytes, zero padded (conversion.rs:37-39) */
  uint16_t message_byte_length;
  uint8_t validator_byte_length;
  uint8_t flags; /* TMX_FLAG_* */
  uint64_t voting_power;
  uint8_t pad[24];
} tmx_validator_rec;

/* One lane of `trusted_header_validator_hash_fields` (ValidatorHashField, variables.rs:82-88). */
typedef struct {
  uint8_t pubkey[32];
  uint64_t voting_power;
  uint8_t validator_byte_length;
  uint8_t flags;
  uint8_t pad[6];
} tmx_hashfield_rec;

/* The 14 protobuf-encoded header fields (reference circuits/input/tendermint_utils.rs:374-393), each < 80 B. */
typedef struct {
  uint8_t leaf_len[14];
  uint8_t pad[2];
  uint8_t leaf[14][80];
} tmx_header_rec;

/* Per-proof fixed inputs.  skip: block_a = trusted_block, block_b = target_block, hash = trusted_header_hash,
 * header_a = target header, header_b = trusted header, nb_a / nb_b = target / trusted validator counts.
 * step: block_a = prev_block_number, block_b = prev + 1, hash = prev_header_hash, header_a = next header,
 * header_b = prev header, nb_a = next validator count, nb_b = 0. */
typedef struct {
  uint64_t block_a;
  uint64_t block_b;
  uint8_t hash[32];
  uint64_t round; /* commit.round of header_a's block */
  uint32_t nb_a;
  uint32_t nb_b;
  tmx_header_rec header_a;
  tmx_header_rec header_b;
} tmx_proof_rec;

/* Level-0 output + verdicts, one per proof.  fail_mask bit order: DESIGN.md "checks". */
typedef struct {
  uint8_t header[32]; /* target_header (skip.rs:132) / next_header (step.rs:116) */
  uint32_t all_ok;
  uint32_t fail_mask;
  int32_t first_bad_sig; /* first lane whose EdDSA equation fails (conversion.rs:48-49 panic site), or -1 */
  uint32_t gt_target;    /* signed power * 3 > total * 2   (verify.rs:289-303) */
  uint32_t gt_trusted;   /* matched power * 3 > total * 1  (verify.rs:428-436), skip only */
  uint32_t dist_ok;      /* verify_skip_distance (verify.rs:508-526), skip only */
  uint32_t precond;      /* host preconditions of the reference that the circuit itself does not assert: bit 0 nb_a > n_max,
                            bit 1 nb_b > n_max (input/mod.rs:439-444, 338-342 panic there; in-circuit `idx == nb` never fires and
                            every lane counts as enabled).  The host entry points refuse such input with TMX_ERR_SET_TOO_LARGE; the
                            device entry points cannot look at device memory before enqueueing and report it here instead. */
  uint32_t reserved;
} tmx_report;

typedef struct {
  uint32_t n_max;        /* VALIDATOR_SET_SIZE_MAX (const generic of SkipCircuit / StepCircuit), 1..512 */
  uint32_t chain_id_len; /* CHAIN_ID_SIZE_BYTES */
  uint8_t chain_id[TMX_PROTOBUF_CHAIN_ID_SIZE_BYTES]; /* TendermintConfig::CHAIN_ID_BYTES (config.rs:6) */
  uint64_t skip_max;     /* TendermintConfig::SKIP_MAX (config.rs:7) */
  int32_t device;        /* HIP device ordinal */
  uint32_t max_batch;    /* proofs per call this context preallocates scratch for (>= 1) */
} tmx_config;

typedef struct tmx_ctx tmx_ctx;

/* names of the kernels timed by tmx_last_kernel_ms, in launch order */
#define TMX_N_KERNELS 4
#define TMX_K_EDDSA 0     /* per-validator Ed25519 (k_ed_dedup, k_ed_keys, k_ed_tab_x, k_ed_phase1, k_ed_mul_x, k_ed_fin): SHA-512, decode, s*B, h*A, R+hA, affine */
#define TMX_K_PROOF 1     /* k_proof on the context's side stream, concurrent with the EdDSA kernels: marshal + SHA-256 leaves +
                             Merkle trees + header proofs + NxN match + tallies */
#define TMX_K_VERDICT 2   /* join: wait for k_proof, merge the per-lane EdDSA verdicts (k_verdict) */
#define TMX_K_SERIALIZE 3 /* Goldilocks element fill */

uint32_t tmx_version(void);
const char* tmx_status_str(int32_t status);

int32_t tmx_ctx_create(const tmx_config* cfg, tmx_ctx** out);
void tmx_ctx_destroy(tmx_ctx* ctx);
const char* tmx_last_error(const tmx_ctx* ctx);

/* number of Goldilocks elements of one witness, and the row stride used in batched output (a multiple of 16 elements: rows start on a
 * 128-byte line; the pad elements are written as zeros) */
uint64_t tmx_elem_count(int32_t kind, uint32_t n_max);
uint64_t tmx_elem_stride(int32_t kind, uint32_t n_max);
/* offset and length of the hint section H (= VerifySkipVariable<N> / VerifyStepVariable<N> elements) in a row */
uint64_t tmx_hint_elem_count(int32_t kind, uint32_t n_max);

/* ---- host-buffer entry points: what the Rust hint binds.  out_elems receives tmx_elem_count() elements. */
int32_t tmx_skip_witness(tmx_ctx* ctx, const tmx_proof_rec* proof, const tmx_validator_rec* target /*[n_max]*/,
                         const tmx_hashfield_rec* trusted /*[n_max]*/, uint64_t* out_elems, uint64_t cap_elems,
                         tmx_report* report);
int32_t tmx_step_witness(tmx_ctx* ctx, const tmx_proof_rec* proof, const tmx_validator_rec* target /*[n_max]*/,
                         uint64_t* out_elems, uint64_t cap_elems, tmx_report* report);
/* n_proofs independent proofs; rows of tmx_elem_stride() elements; out_elems may be NULL (reports only) */
int32_t tmx_witness_batch(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, const tmx_proof_rec* proofs,
                          const tmx_validator_rec* targets /*[n_proofs][n_max]*/,
                          const tmx_hashfield_rec* trusteds /*[n_proofs][n_max], NULL for step*/, uint64_t* out_elems,
                          uint64_t cap_elems, tmx_report* reports);

/* ---- host-buffer entry point with a section selection and a transfer format.  A hint body only needs H (43 % of a skip row at
 * N = 128: what SkipOffchainInputs::hint writes to its output stream, skip.rs:85-100), and every element of this witness is < 2^32
 * (a bit, a byte, a u32 limb), so a PCIe-bound caller can fetch it as u32 and widen with F::from_canonical_u32 on its side.
 * out receives n_proofs DENSE rows of tmx_out_row_elems(kind, n_max, sections) elements of 8 (TMX_OUT_U64) or 4 (TMX_OUT_U32) bytes;
 * with both sections selected a row is H then D.  Sections that are not selected are not serialized on the device either. */
#define TMX_SEC_HINT 1u
#define TMX_SEC_DERIVED 2u
#define TMX_SEC_ALL 3u
#define TMX_OUT_U64 0u
#define TMX_OUT_U32 1u
uint64_t tmx_out_row_elems(int32_t kind, uint32_t n_max, uint32_t sections);
int32_t tmx_witness_batch_opts(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, const tmx_proof_rec* proofs,
                               const tmx_validator_rec* targets, const tmx_hashfield_rec* trusteds /*NULL for step*/, uint32_t sections,
                               uint32_t format, void* out, uint64_t cap_bytes, tmx_report* reports);

/* ---- the TYPED VALUE of the hint: what the reference's hint bodies actually hold before plonky2x expands it into field elements.
 * SkipOffchainInputs::hint builds a `VerifySkipStruct` literal from a `SkipInputs<F>` (reference circuits/skip.rs:85-98, circuits/input/mod.rs:60-74)
 * and hands it to `write_value` (skip.rs:100), which does the bit / limb expansion itself; StepOffchainInputs::hint the same with `StepInputs<F>`
 * (step.rs:75-87, input/mod.rs:45-58).  These structs mirror those two types FIELD BY FIELD -- bytes as bytes, u64 as u64 -- so a hint body
 * assigns them by name (rust-shim/skip_hint.rs.example) and no knowledge of the element order inside plonky2x's variable types is needed:
 * 38 KB per N = 128 skip proof instead of the 1.86 MB of u64 elements (0.93 MB as u32) of the expanded row.
 * One proof's value = fixed part | tmx_validator_value[n_max] | tmx_hashfield_value[n_max] (skip only)
 *                     [| derived values, with TMX_SEC_DERIVED: see tmx_value_layout], every part 16-byte aligned, little-endian. */
typedef struct {             /* ValidatorType<F>: the value type of ValidatorVariable, reference circuits/variables.rs:69-79; built by
                                get_validator_data_from_block, circuits/input/conversion.rs:59-137 */
  uint8_t pubkey[32];        /* CompressedEdwardsY */
  uint8_t sig_r[32];         /* EDDSASignatureVariableValue.r (compressed point) */
  uint8_t sig_s[32];         /* EDDSASignatureVariableValue.s: U256, little-endian */
  uint8_t message[TMX_VALIDATOR_MESSAGE_BYTES_LENGTH_MAX];
  uint32_t message_byte_length;
  uint64_t voting_power;
  uint32_t validator_byte_length;
  uint32_t signed_;          /* bool `signed` */
} tmx_validator_value;       /* 240 B */
typedef struct {             /* ValidatorHashField<F>: variables.rs:82-88; validator_hash_field_from_block, conversion.rs:139-178 */
  uint8_t pubkey[32];
  uint64_t voting_power;
  uint32_t validator_byte_length;
  uint32_t pad;
} tmx_hashfield_value;       /* 48 B */
typedef struct {             /* ChainIdProofValueType<F>: variables.rs:35-41; input/mod.rs:471-482 */
  uint8_t proof[TMX_HEADER_PROOF_DEPTH][32];
  uint32_t enc_chain_id_byte_length;
  uint8_t chain_id[TMX_PROTOBUF_CHAIN_ID_SIZE_BYTES]; /* the encoded field resized to 52 bytes */
  uint8_t pad[8];
} tmx_chain_id_proof_value;  /* 192 B */
typedef struct {             /* HeightProofValueType<F>: variables.rs:49-55; input/mod.rs:484-493 */
  uint8_t proof[TMX_HEADER_PROOF_DEPTH][32];
  uint32_t enc_height_byte_length;
  uint32_t pad;
  uint64_t height;
} tmx_height_proof_value;    /* 144 B */
typedef struct {             /* InclusionProof<HEADER_PROOF_DEPTH, PROTOBUF_HASH_SIZE_BYTES, F>: input/mod.rs:303-314 */
  uint8_t proof[TMX_HEADER_PROOF_DEPTH][32];
  uint8_t leaf[34];
  uint8_t pad[14];
} tmx_hash_inclusion_proof_value;     /* 176 B */
typedef struct {             /* InclusionProof<HEADER_PROOF_DEPTH, PROTOBUF_BLOCK_ID_SIZE_BYTES, F> */
  uint8_t proof[TMX_HEADER_PROOF_DEPTH][32];
  uint8_t leaf[72];
  uint8_t pad[8];
} tmx_block_id_inclusion_proof_value; /* 208 B */
typedef struct {             /* SkipInputs<F> (input/mod.rs:60-74) without its two Vecs, which follow as arrays; + the verdicts */
  uint8_t target_header[32];
  uint8_t trusted_header[32];
  uint64_t round;
  uint32_t nb_target_validators;
  uint32_t nb_trusted_validators;
  tmx_chain_id_proof_value target_block_chain_id_proof;
  tmx_height_proof_value target_block_height_proof;
  tmx_hash_inclusion_proof_value target_block_validators_hash_proof;
  tmx_hash_inclusion_proof_value trusted_block_validators_hash_proof;
  tmx_report report;
} tmx_skip_inputs_fixed;     /* 832 B */
typedef struct {             /* StepInputs<F> (input/mod.rs:45-58) without its Vec; + the verdicts */
  uint8_t next_header[32];
  uint64_t round;
  uint32_t nb_validators;
  uint32_t pad;
  tmx_chain_id_proof_value next_block_chain_id_proof;
  tmx_height_proof_value next_block_height_proof;
  tmx_hash_inclusion_proof_value next_block_validators_hash_proof;
  tmx_block_id_inclusion_proof_value next_block_last_block_id_proof;
  tmx_hash_inclusion_proof_value prev_block_next_validators_hash_proof;
  tmx_report report;
} tmx_step_inputs_fixed;     /* 1008 B */
/* Derived Level-1 values (section D of the row, DESIGN.md "Witness layout") in packed form -- optional (TMX_SEC_DERIVED): what a
 * replacement for Curta's result hints would consume.  Pad bytes are written as zeros. */
typedef struct {             /* D.1a + D.1b of one target lane */
  uint8_t sha512_digest[64]; /* SHA-512(R | A | M) of the lane's effective triple */
  uint8_t h[32];             /* digest mod l, little-endian */
  uint8_t points[10][32];    /* A.x A.y R.x R.y sB.x sB.y hA.x hA.y (R+hA).x (R+hA).y: canonical, little-endian */
  uint32_t eddsa_ok;
  uint32_t decode_ok;
  uint8_t pad0[24];
  uint8_t marshalled[TMX_VALIDATOR_BYTE_LENGTH_MAX];
  uint8_t pad1[2];
  uint8_t leaf_hash[32];
  uint8_t flags[6];          /* enabled, hash_in_msg, is_precommit, height_ok, round_ok, sigdata_ok */
  uint8_t pad2[2];
  uint64_t total_prefix;     /* running sum of enabled powers (voting.rs:31-63) */
  uint64_t signed_prefix;    /* running sum of signed powers (voting.rs:79-89) */
  uint8_t pad3[8];
} tmx_target_lane_derived;   /* 560 B */
typedef struct {             /* D.2a + D.2b of one trusted lane (skip) */
  uint8_t marshalled[TMX_VALIDATOR_BYTE_LENGTH_MAX];
  uint8_t pad1[2];
  uint8_t leaf_hash[32];
  uint8_t flags[2];          /* enabled, matched (verify.rs:398-418) */
  uint8_t pad2[6];
  uint64_t total_prefix;
  uint64_t matched_prefix;
  uint8_t pad3[8];
} tmx_trusted_lane_derived;  /* 112 B */
typedef struct {             /* D.5 / D.6 of one proof */
  uint8_t proofs[5][5][32];  /* chain id, height, validators hash, X, Y (step only): leaf hash then the four path nodes */
  uint8_t height_leaf[11];   /* 00 08 varint9(height) */
  uint8_t pad0[5];
  uint64_t tally_target[4];  /* total, acc, acc * 3, total * 2 */
  uint64_t tally_trusted[4]; /* skip only */
  uint32_t verdicts[4];      /* gt_target, gt_trusted, dist_gt, dist_le (the last three: skip only) */
  uint32_t checks[16];       /* 13 (skip) / 15 (step) check words, tmx_report.fail_mask bit order */
  uint32_t all_ok;
  uint32_t pad1;
  uint64_t height;
} tmx_proof_derived;         /* 976 B */
typedef struct {
  uint64_t bytes;              /* of one proof's value: proof p of a batch starts at p * bytes */
  uint32_t fixed_bytes;        /* sizeof(tmx_skip_inputs_fixed) / sizeof(tmx_step_inputs_fixed), at offset 0 */
  uint32_t off_validators;     /* tmx_validator_value[n_max] */
  uint32_t off_hashfields;     /* tmx_hashfield_value[n_max]; 0 for step */
  uint32_t off_target_lanes;   /* tmx_target_lane_derived[n_max]; this and the following: 0 without TMX_SEC_DERIVED */
  uint32_t off_trusted_lanes;  /* tmx_trusted_lane_derived[n_max]; 0 for step */
  uint32_t off_nodes_target;   /* [tree_nodes][32]: every node of the fixed-shape validator tree, layer by layer (D.3) */
  uint32_t off_nodes_trusted;  /* (D.4) 0 for step */
  uint32_t off_proof_derived;  /* tmx_proof_derived */
  uint32_t tree_nodes;
  uint32_t reserved;
} tmx_value_layout;
/* sections: TMX_SEC_HINT (the reference's hint value) or TMX_SEC_ALL (+ the derived values); TMX_ERR_BAD_ARG otherwise */
int32_t tmx_value_layout_of(int32_t kind, uint32_t n_max, uint32_t sections, tmx_value_layout* out);
/* Host buffers in, host buffer out: `out` receives n_proofs values of layout.bytes each.  No element row is produced on the device at all
 * (the serializer does not run).  Fastest with page-locked buffers (tmx_host_alloc): the copies are then direct DMA, and a page-locked
 * `out` is written by the GPU itself. */
int32_t tmx_inputs_value_batch(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, const tmx_proof_rec* proofs, const tmx_validator_rec* targets,
                               const tmx_hashfield_rec* trusteds /*NULL for step*/, uint32_t sections, void* out, uint64_t cap_bytes);
/* the single-proof forms a hint body binds (reference circuits/skip.rs:64-102, circuits/step.rs:56-89) */
int32_t tmx_skip_inputs_value(tmx_ctx* ctx, const tmx_proof_rec* proof, const tmx_validator_rec* target /*[n_max]*/,
                              const tmx_hashfield_rec* trusted /*[n_max]*/, uint32_t sections, void* out, uint64_t cap_bytes);
int32_t tmx_step_inputs_value(tmx_ctx* ctx, const tmx_proof_rec* proof, const tmx_validator_rec* target /*[n_max]*/, uint32_t sections,
                              void* out, uint64_t cap_bytes);
/* Device pointers in and out, asynchronous on hip_stream like tmx_witness_batch_device (d_out may also be the device address of mapped
 * page-locked host memory). */
int32_t tmx_inputs_value_batch_device(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets,
                                      const void* d_trusteds, uint32_t sections, void* d_out, void* hip_stream);
/* page-locked host memory for the host entry points (hipHostMalloc: mapped, portable).  NULL on failure. */
void* tmx_host_alloc(tmx_ctx* ctx, uint64_t bytes);
void tmx_host_free(tmx_ctx* ctx, void* p);

/* ---- device-resident entry point: inputs already in HBM, outputs stay in HBM.  All pointers are device
 * pointers of the context's device; `hip_stream` is the hipStream_t to enqueue on, used exactly as passed (NULL = the HIP
 * default stream; tmx_ctx_stream() = the context's own stream).  Asynchronous: returns after enqueueing. */
void* tmx_ctx_stream(tmx_ctx* ctx);
int32_t tmx_witness_batch_device(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets,
                                 const void* d_trusteds, void* d_out_elems, void* d_reports, void* hip_stream);
/* the same with a section selection: rows keep tmx_elem_stride(), sections that are not selected are left unwritten */
int32_t tmx_witness_batch_device_sections(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets,
                                          const void* d_trusteds, void* d_out_elems, void* d_reports, void* hip_stream, uint32_t sections);
/* The two halves of the call above, for the validator-sharded single-proof mode (BASELINE config 5): each GPU runs
 * k_eddsa on its slice of lanes, the 448-B lane records are exchanged (one RCCL all-gather), then k_proof + k_serialize
 * run on the reassembled records.  d_ed_out / d_ed: TMX ED records, 448 B per lane (layout at tmx_eddsa_lanes). */
int32_t tmx_eddsa_lanes_device(tmx_ctx* ctx, uint32_t n_lanes, const void* d_lanes, void* d_ed_out, void* hip_stream);
int32_t tmx_finish_batch_device(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets,
                                const void* d_trusteds, const void* d_ed, void* d_out_elems, void* d_reports, void* hip_stream);
/* HIP-event times (ms) of the kernels of the LAST tmx_witness_batch_device / host call; blocks until they finished */
int32_t tmx_last_kernel_ms(tmx_ctx* ctx, float ms[TMX_N_KERNELS]);
/* mean over the last `last_k` enqueued batches (each batch keeps its own event set, ring of 128): lets a caller time
 * a whole region without synchronising inside it */
int32_t tmx_kernel_ms_mean(tmx_ctx* ctx, uint32_t last_k, float ms[TMX_N_KERNELS]);
int32_t tmx_sync(tmx_ctx* ctx);
/* EdDSA stage bookkeeping of the last launch: number of distinct (effective) public keys among its lanes and whether h*A of any lane
 * walked a per-key table (a key resident in the key cache, or a new key with >= 8 lanes per key on average; TMX_DEDUP=0|1|2 forces
 * never / automatic / whenever a table fits).  Blocks. */
int32_t tmx_last_dedup(tmx_ctx* ctx, uint32_t* n_unique, uint32_t* used_tables);
/* Which launch computed the proof-level values (header and validator trees, tallies, trusted-key match) of the last batch enqueued on
 * this context: the small path's two launches, k_proof as role workgroups, or one workgroup per proof in the instantiation for
 * VALIDATOR_SET_SIZE_MAX <= 128 / <= 256 / <= 512.  A host-side field: no device traffic, does not block.  NONE before the first batch;
 * calls that run no proof stage (the EdDSA-only, trace and commitment entry points) leave it as it is; TMX_ERR_BAD_ARG for a null context. */
enum tmx_proof_path {
  TMX_PROOF_PATH_NONE = 0,
  TMX_PROOF_PATH_TINY = 1,
  TMX_PROOF_PATH_ROLES = 2,
  TMX_PROOF_PATH_R168 = 3,
  TMX_PROOF_PATH_K256 = 4,
  TMX_PROOF_PATH_WIDE = 5
};
int32_t tmx_last_proof_path(tmx_ctx* ctx);

/* ---- multi-GPU: one process per GPU, the exchange step behind this ABI so that the host the reference actually has -- the
 * Rust process of bin/skip.rs, reached only through SkipOffchainInputs::hint (reference circuits/skip.rs:64-102) -- can shard without
 * any Python.  RCCL is resolved at run time from the host process (no DT_NEEDED, like the HIP runtime): $TMX_RCCL_LIB if set (then it is
 * the only candidate), else an already loaded librccl, else librccl.so.1 / librccl.so by the loader's search path.  A context-less call
 * (tmx_comm_unique_id) leaves its reason in tmx_last_error(NULL), per thread.  Bootstrap as with NCCL: ONE rank calls
 * tmx_comm_unique_id, hands the 128 bytes to the others by whatever channel the host has (a file, its RPC, MPI ...), then every rank calls
 * tmx_comm_create(ctx, id, rank, world) on a context of ITS device.  world = 1 needs no id and loads nothing.
 *   tmx_shard_range                       contiguous [lo, hi) of n_items for `rank` of `world`; sizes differ by at most one
 *   tmx_witness_batch_sharded_device      BASELINE configs[3]: n_total independent proofs, every rank holds all input records and an output
 *                                         buffer for all rows; rank r computes rows [lo_r, hi_r) in place; gather != 0 then makes every row
 *                                         (and report) resident on every rank -- ONE exchange in place, no padding, no staging copy: an
 *                                         ncclAllGather when n_total divides by the world (256 proofs over 2 / 4 / 8 ranks), else a group of
 *                                         broadcasts, each rank the root of its own slice.  gather = 0: no data-path collective at all.
 *   tmx_witness_validator_sharded_device  BASELINE configs[4]: the n_proofs * n_max validator lanes split across the ranks for the EdDSA stage,
 *                                         ONE grouped exchange of the 448-byte lane records, then every rank finishes every proof
 *                                         (tmx_finish_batch_device on the reassembled records): full rows + reports on every rank.
 * Both are asynchronous on hip_stream like tmx_witness_batch_device; n_total / the lanes may be smaller than the world (empty shards).
 *
 * FAILURE CONTRACT of the sharded calls (round 6).  A collective is entered by every rank or by none.  Argument errors (TMX_ERR_BAD_ARG) are
 * assumed to be the same on every rank and are returned before anything is enqueued.  A failure that is LOCAL to one rank between the start of
 * a sharded call and its exchange -- its shard exceeds ITS context's max_batch, a launch fails on ITS device -- must not leave the peers waiting
 * in the collective: the failing rank aborts its communicator (ncclCommAbort) and returns TMX_ERR_RCCL (tmx_last_error names the local cause);
 * the peers' exchange then fails instead of hanging -- at the collective call itself, or asynchronously: a host that needs a bounded wait
 * synchronises with tmx_comm_sync(ctx, stream, timeout_ms) instead of hipStreamSynchronize; it polls the stream and ncclCommGetAsyncError, and on
 * an asynchronous error or the timeout aborts this rank's communicator too and returns TMX_ERR_RCCL.  After TMX_ERR_RCCL from any sharded call
 * or from tmx_comm_sync the context refuses further sharded calls (TMX_ERR_RCCL) until tmx_comm_create is called again -- on EVERY rank, with
 * a fresh id; the non-sharded entry points and the caches of the context are unaffected.  The buffers of a failed call hold nothing defined.
 *   tmx_comm_abort   what a host calls on its healthy contexts when IT learns (by its own channel) that a peer process died
 *   tmx_comm_sync    timeout_ms = 0: no timeout (asynchronous errors still end the wait) */
#define TMX_UNIQUE_ID_BYTES 128
void tmx_shard_range(uint64_t n_items, uint32_t rank, uint32_t world, uint64_t* lo, uint64_t* hi);
int32_t tmx_comm_unique_id(uint8_t out[TMX_UNIQUE_ID_BYTES]);
int32_t tmx_comm_create(tmx_ctx* ctx, const uint8_t unique_id[TMX_UNIQUE_ID_BYTES] /* NULL iff world == 1 */, uint32_t rank, uint32_t world);
int32_t tmx_comm_destroy(tmx_ctx* ctx);
int32_t tmx_comm_info(const tmx_ctx* ctx, uint32_t* rank, uint32_t* world);  /* (0, 1) before tmx_comm_create */
int32_t tmx_comm_abort(tmx_ctx* ctx);
int32_t tmx_comm_sync(tmx_ctx* ctx, void* hip_stream, uint32_t timeout_ms);
int32_t tmx_witness_batch_sharded_device(tmx_ctx* ctx, int32_t kind, uint32_t n_total, const void* d_proofs, const void* d_targets,
                                         const void* d_trusteds, void* d_out_elems, void* d_reports, uint32_t gather, void* hip_stream);
int32_t tmx_witness_validator_sharded_device(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, const void* d_proofs, const void* d_targets,
                                             const void* d_trusteds, void* d_out_elems, void* d_reports, void* hip_stream);

/* The Level-2 trace rows across the ranks (the one payload of this path big enough for xGMI to matter: 41 MB per proof at N = 128, 136 MB at
 * N = 512).  Same conventions as above: d_trace_out holds the rows of ALL proofs (tmx_trace_elem_count() u64 each), asynchronous on hip_stream.
 *   tmx_trace_rows_sharded_device            after tmx_witness_batch_sharded_device of the same n_total: rank r writes the rows of its proofs
 *                                            [lo_r, hi_r) in place; gather != 0: one exchange (ncclAllGather when the shards are equal) leaves
 *                                            every proof's rows on every rank.
 *   tmx_trace_rows_validator_sharded_device  after tmx_witness_validator_sharded_device of the same n_proofs: the per-lane sections (ladders,
 *                                            SHA-512 rounds: 93 % of the rows) are computed for this rank's lanes only and exchanged lane slab
 *                                            by lane slab (one proof: one all-gather per section); the small per-proof sections (leaf / tree /
 *                                            header SHA-256, N x N) are computed on every rank.  All rows on every rank afterwards.
 *   tmx_trace_commit_sharded_device          tmx_trace_commit_device over this rank's own proofs (no row crosses a link), its cap into slot
 *                                            `rank` of d_caps[world][4 << cap_height], then ONE all-gather of the caps.
 *                                            tmx_trace_commit_open_device then opens this rank's tree (cap slot `rank`); an empty shard
 *                                            leaves nothing to open. */
int32_t tmx_trace_rows_sharded_device(tmx_ctx* ctx, int32_t kind, uint32_t n_total, const void* d_targets, const void* d_trusteds, void* d_trace_out,
                                      uint32_t sections, uint32_t gather, void* hip_stream);
int32_t tmx_trace_rows_validator_sharded_device(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, const void* d_targets, const void* d_trusteds,
                                                void* d_trace_out, uint32_t sections, void* hip_stream);
int32_t tmx_trace_commit_sharded_device(tmx_ctx* ctx, int32_t kind, uint32_t n_total, uint32_t section, uint32_t log_blowup, uint32_t cap_height,
                                        const void* d_trace_rows, uint64_t* d_caps /*[world][4 << cap_height]*/, void* hip_stream);

/* ---- persistent per-key table cache.  h*A of a lane is 32 additions from a 655-KB window table of its public key instead of 252
 * doublings + 64 additions; the context keeps those tables in a content-addressed cache in HBM (key = the 32 public-key bytes, all 32
 * compared on a hit), so that a validator set that was seen by an earlier call -- a light client re-verifies the same, slowly changing set
 * for days (reference bin/tendermintx.rs:171) -- skips the decode -> doubling chain -> table build entirely.  New keys are inserted by the
 * call that first sees them (a single-proof call builds their tables off its critical path, for the next call); when the cache runs full
 * the least recently used keys are evicted.  Exact group arithmetic on every path: the witness is bit-identical with the cache on, off,
 * cold or warm.  Default capacity: 1024 .. 8192 keys by max_batch * n_max (TMX_KEY_CACHE_KEYS overrides; TMX_KEY_CACHE=0 disables).
 * All three calls block until the context's work in flight is done. */
typedef struct {
  uint32_t capacity_keys, resident_keys, enabled, epoch;
  uint64_t bytes_per_key;
  uint32_t last_new_keys, last_hit_keys, last_hit_lanes, last_built_keys; /* the last EdDSA launch */
  uint64_t hit_lanes, miss_lanes, built_keys, evicted_keys, evictions, launches; /* since the cache was created / flushed */
} tmx_key_cache_info;
int32_t tmx_key_cache_stats(tmx_ctx* ctx, tmx_key_cache_info* out);
int32_t tmx_key_cache_flush(tmx_ctx* ctx);                                      /* forget every key */
int32_t tmx_key_cache_config(tmx_ctx* ctx, uint32_t enabled, uint32_t max_keys); /* max_keys = 0 keeps the capacity; a new capacity flushes */
/* The validator-set cache of a context (round 5): marshalled validators, leaf hashes and every node of the fixed-shape tree
 * (reference circuits/builder/validator.rs:185-252) depend on the validator set alone -- (pubkey, voting power, validator_byte_length) of every lane and
 * the number of enabled lanes -- not on the proof, and a light client re-verifies the same slowly changing sets.  A batch's k_proof looks both
 * sets of a proof up by a 64-bit fingerprint, compares EVERY key byte, and copies the cached values instead of hashing (15 SHA-256
 * compressions off its chain); sets it had to compute are inserted.  256 sets per context, least-recently-used eviction at launch granularity
 * (round 6): a hit or an insert stamps the set with the launch's number, and a one-workgroup kernel behind every k_proof launch keeps an eighth of the slots free by
 * evicting the sets used longest ago -- a prover that lives for months (reference bin/tendermintx.rs:171) keeps the sets it is verifying now, not
 * the first 256 it ever saw.  tmx_key_cache_flush empties it too; TMX_SET_CACHE=0 disables; TMX_SET_CACHE_SETS=<4..256> = capacity (tests).
 * Bit-identical by construction.  out: [0] sets resident [1] sets served from the cache [2] sets computed [3] sets inserted [4] sets evicted
 * (totals since creation / the last flush) [5] capacity [6..7] reserved (0). */
int32_t tmx_set_cache_stats(tmx_ctx* ctx, uint32_t out[8]);

/* ---- Level-2 trace rows (SURVEY 8a "Level-2", 8f rank 2): the row-level execution trace behind the Level-1 values -- what the reference
 * produces inside Curta's trace generators for `curta_eddsa_verify_sigs_conditional` (reference circuits/builder/verify.rs:248-259) and
 * `curta_sha256_variable` (validator.rs:228).  Those sources are absent, so the row layout is this build's own specification (DESIGN.md
 * "Level-2 trace rows"), validated row by row by the constraint checker under oracle/c -- NOT claimed equal to Curta's columns.
 * Per proof tmx_trace_elem_count() elements (u64, every value < 2^32):
 *   ladders   lane i, ladder k (0: s*B, 1: h*A), 256 rows x 65: bit | acc | dbl = 2 acc | add = dbl + P | nxt = bit ? add : dbl,
 *             points as canonical affine (x, y) in eight little-endian u32 limbs each; acc_0 = (0, 1), acc_{r+1} = nxt_r, nxt_255 = k * P
 *   SHA-512   lane i, block b < 2, 80 rounds x 18: W_t and a..h after the round (64-bit words as lo, hi)
 *   SHA-256   validator leaf hashes of the target (and, for skip, trusted) set: 64 rounds x 9
 *   N x N     skip: signed[i] & (target pubkey i == trusted pubkey j)
 *   tree      set s, node slot of the fixed-shape validator tree (Level-1 order): 2 blocks x 64 rounds x 9 of SHA-256(01 | L | R) over the
 *             slot's two children as Level-1 holds them (every pair is hashed, then selected: validator.rs:248-251); promoted slots are zero
 *   header    the header proofs in Level-1 order (chain id, height, validators hash, X, Y), each the leaf hash and the four path-node
 *             hashes: 2 blocks x 64 x 9 each (verify.rs:189-209, shared.rs:183-203)
 * tmx_trace_rows_device reads the Level-1 lane records the context holds: call it after tmx_witness_batch_device of the SAME batch, on the
 * same stream.  d_trace_out: n_proofs * tmx_trace_elem_count() u64.  41 MB per proof at N = 128: this launch is HBM-write work. */
#define TMX_TRACE_LADDERS 1u
#define TMX_TRACE_SHA512 2u
#define TMX_TRACE_SHA256 4u
#define TMX_TRACE_MATCH 8u
#define TMX_TRACE_TREE 16u
#define TMX_TRACE_HEADER 32u
#define TMX_TRACE_ALL 63u
uint64_t tmx_trace_elem_count(int32_t kind, uint32_t n_max);
int32_t tmx_trace_rows_device(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, const void* d_targets, const void* d_trusteds, void* d_trace_out,
                              uint32_t sections, void* hip_stream);

/* ---- the commit pipeline on the device: what the reference's `prove` does with the trace in ONE process -- witness ->
 * trace -> low-degree extension -> Merkle commit (reference circuits/skip.rs:119-133, through plonky2x / starkyx / plonky2, absent here) --
 * chained on the GPU so that only the cap leaves it: the rows of ONE section of every proof of the batch (d_trace_rows: what
 * tmx_trace_rows_device wrote; row-major, tmx_trace_elem_count() elements per proof) become n_proofs * width columns of 2^log_rows
 * elements (zero rows behind a proof's own; a tiled transpose), every column is extended to the coset shift <omega_(2^log_rows << log_blowup)>
 * (tmx_lde_goldilocks_device), and the Merkle tree over the extended rows (leaf = row across ALL columns of the batch, hash_no_pad; inner
 * nodes two_to_one: tmx_poseidon_merkle_device) is reduced to its cap: d_cap receives 4 << cap_height u64.
 * section: ONE of TMX_TRACE_LADDERS / SHA512 / SHA256 / TREE / HEADER (the N x N match bits are not a row table).
 * Same caveats as its stages: own row layout, natural (not bit-reversed) row order, no salt, Poseidon constants as set on the context --
 * parity is pinned against the CPU chain under oracle/c (tmxo_trace -> tmxo_ntt -> tmxo_poseidon), not against plonky2.
 * Scratch (columns, extended columns, tree levels) is owned by the context and grows on demand: (1 + 3 * 2^log_blowup) * n_proofs * width *
 * 2^log_rows * 8 B -- 30 GB for the SHA-512 section of 256 proofs at N = 128, 8 x blow-up.  Asynchronous on hip_stream. */
int32_t tmx_trace_commit_shape(int32_t kind, uint32_t n_max, uint32_t section, uint32_t* log_rows, uint32_t* width);
int32_t tmx_trace_commit_device(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, uint32_t section, uint32_t log_blowup, uint32_t cap_height,
                                const void* d_trace_rows, uint64_t* d_cap, void* hip_stream);
/* HIP-event times (ms) of the stages of the LAST tmx_trace_commit_device: columns, LDE, Merkle; blocks until they finished */
int32_t tmx_trace_commit_last_ms(tmx_ctx* ctx, float ms[3]);

/* ---- per-lane Level-1 EdDSA values only (unit-test / profiling hook of the dominant kernel).
 * d_out: 448 B per lane = digest[64] | h[32] | A.x A.y R.x R.y sB.x sB.y hA.x hA.y sum.x sum.y [10][32] | ok u32 |
 * decode_ok u32 | pad.  Host variant copies in/out. */
int32_t tmx_eddsa_lanes(tmx_ctx* ctx, uint32_t n_lanes, const tmx_validator_rec* lanes, uint8_t* out /*[n_lanes][448]*/);

/* ---- input codec: the reference's on-disk fixture / CometBFT RPC JSON -> packed records
 * (InputDataFetcher fixture mode, reference circuits/input/mod.rs:188-282; conversion.rs:59-178;
 *  tendermint_utils.rs:374-441).  Pure host code, no hashing: the trusted header hash is NOT computed here. */
int32_t tmx_skip_inputs_from_json(const char* trusted_commit_json, const char* trusted_validators_json,
                                  const char* target_commit_json, const char* target_validators_json, uint32_t n_max,
                                  uint64_t trusted_block, const uint8_t trusted_header_hash[32], uint64_t target_block,
                                  tmx_proof_rec* proof, tmx_validator_rec* target, tmx_hashfield_rec* trusted);
int32_t tmx_step_inputs_from_json(const char* prev_commit_json, const char* next_commit_json, const char* next_validators_json,
                                  uint32_t n_max, uint64_t prev_block, const uint8_t prev_header_hash[32],
                                  tmx_proof_rec* proof, tmx_validator_rec* target);

/* ---- the caller of the path: `is_valid_skip` (reference circuits/input/tendermint_utils.rs:444-482) for many
 * candidate target blocks at once -- what `find_block_to_request` (reference circuits/input/mod.rs:160-186) asks block by block.
 * For candidate c:  shared = sum over start validators found (by address) in target set c of
 *                            power_in_target * #(commit signatures of c carrying that address, commit or nil votes alike),
 *                   valid  = f64(total power of target set c) * (1/3) <= f64(shared)      (IEEE double, as the reference computes it). */
typedef struct {
  uint8_t address[20];
  uint8_t has_address; /* signatures: CommitSig::validator_address().is_some() (flags 2 and 3); validators: 1 */
  uint8_t pad[3];
  uint64_t voting_power; /* validators only */
} tmx_addr_rec; /* 32 B */
/* start[n_start]; per candidate: targets[c][n_max] (n_targets[c] used), sigs[c][n_max] (n_sigs[c] used).  Outputs per candidate. */
int32_t tmx_valid_skip_batch(tmx_ctx* ctx, uint32_t n_candidates, const tmx_addr_rec* start, uint32_t n_start,
                             const tmx_addr_rec* targets, const uint32_t* n_targets, const tmx_addr_rec* sigs, const uint32_t* n_sigs,
                             uint8_t* valid, uint64_t* shared_power, uint64_t* total_power);
/* codec for it: `/validators` JSON of the start block, `/validators` + `/commit` JSON of one candidate -> records (each array n_max long) */
int32_t tmx_skipcheck_inputs_from_json(const char* start_validators_json, const char* target_validators_json, const char* target_commit_json,
                                       uint32_t n_max, tmx_addr_rec* start, uint32_t* n_start, tmx_addr_rec* target, uint32_t* n_target,
                                       tmx_addr_rec* sigs, uint32_t* n_sigs);

/* ---- public I/O packing: abi.encodePacked(uint64,bytes32,uint64) / (uint64,bytes32)
 * (reference contracts/src/TendermintX.sol:104-108, circuits/skip.rs:120-122, circuits/step.rs:107-108) */
void tmx_pack_skip_input(uint64_t trusted_block, const uint8_t trusted_header_hash[32], uint64_t target_block, uint8_t out[48]);
void tmx_unpack_skip_input(const uint8_t in[48], uint64_t* trusted_block, uint8_t trusted_header_hash[32], uint64_t* target_block);
void tmx_pack_step_input(uint64_t prev_block, const uint8_t prev_header_hash[32], uint8_t out[40]);
void tmx_unpack_step_input(const uint8_t in[40], uint64_t* prev_block, uint8_t prev_header_hash[32]);

/* ---- Goldilocks NTT / coset low-degree extension (the step after the witness fill of a plonky2-style prover).
 * Own statement of the published definitions (plonky2_field is not in the reference tree; parity pinned against the CPU restatement
 * under oracle/c):  p = 2^64 - 2^32 + 1, omega_N = root^(2^32 / N) for a primitive 2^32-th root of unity `root`; forward
 * X[j] = sum_i x[i] omega_N^(ij), inverse with N^-1, natural order in and out, any u64 input taken mod p, canonical outputs.
 * Domain constants: by default the ones recalled from plonky2's GoldilocksField -- POWER_OF_TWO_GENERATOR = 7277203076849721926 and coset
 * shift MULTIPLICATIVE_GROUP_GENERATOR = 14293326489335486720 (the first is the second to the power (p-1)/2^32: checked in
 * tests/test_ntt_oracle.py; plonky2's source is absent, so "recalled" stays the word).  tmx_ntt_set_domain selects another convention,
 * e.g. g = 7 with root 0x185629dcda58878c (Plonky3 / winterfell).
 * n_cols columns of 2^log_n elements, column c at element c << log_n; device pointers, asynchronous on hip_stream (used exactly as
 * passed).  In place (d_out == d_in) is allowed.
 * tmx_lde_goldilocks_device: evaluations on <omega_N> -> evaluations on the coset shift <omega_M>, M = N << log_blowup (interpolate,
 * scale coefficient i by shift^i, zero-pad, evaluate); d_out holds n_cols << (log_n + log_blowup) elements. */
int32_t tmx_ntt_set_domain(tmx_ctx* ctx, uint64_t root_2_32, uint64_t coset_shift);
#define TMX_NTT_MAX_LOG 22
int32_t tmx_ntt_goldilocks_device(tmx_ctx* ctx, uint32_t log_n, uint32_t n_cols, const uint64_t* d_in, uint64_t* d_out,
                                  int32_t inverse, void* hip_stream);
int32_t tmx_lde_goldilocks_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t n_cols, const uint64_t* d_in,
                                  uint64_t* d_out, void* hip_stream);

/* ---- Poseidon over Goldilocks + Merkle caps ("commit primitives": what a plonky2-style prover does with the LDE'd trace
 * columns -- the reference reaches it through plonky2x `prove`, reference circuits/skip.rs:119-133; plonky2 0.2.0 is an un-vendored
 * dependency, Cargo.lock:2957-2982).  Width 12 (rate 8, capacity 4), S-box x^7, 4 + 22 + 4 rounds, MDS = circulant + diagonal:
 * new[r] = sum_i circ[i] old[(i + r) mod 12] + diag[r] old[r]; hash_no_pad = overwrite-mode sponge; leaf of a row of C columns = the row
 * itself (zero padded) if C <= 4, else hash_no_pad(row); two_to_one(l, r) = permute(l | r | 0000)[0..4).
 * PARITY UNPINNED: plonky2's 360 round constants are not in the reference tree and cannot be recalled, so the default round constants are
 * the Poseidon paper's own Grain-LFSR stream for these parameters (field 1, sbox 0, n 64, t 12, R_F 8, R_P 22) -- NOT plonky2's table; the
 * default MDS is the circulant recalled from plonky2 (17 15 41 16 2 28 13 13 39 18 34 20, diagonal 8 0 .. 0).  tmx_poseidon_set_constants
 * injects the real tables (any argument NULL keeps the current one; values are taken mod p).  Checked against the CPU oracle and
 * an independent Python model; the algebraic self-checks (bijection through the inverse permutation, MDS invertible) are in tests/.
 * tmx_poseidon_merkle_device: n_cols columns of 2^log_n u64 (column c at element c << log_n, e.g. the output of tmx_lde_goldilocks_device),
 * device pointers, asynchronous on hip_stream.  d_levels receives tmx_poseidon_merkle_digests() digests of 4 u64: the 2^log_n leaf digests,
 * then each level above them down to the cap (the last 2^cap_height digests). */
int32_t tmx_poseidon_set_constants(tmx_ctx* ctx, const uint64_t* round_constants /*[360]*/, const uint64_t* mds_circ /*[12]*/,
                                   const uint64_t* mds_diag /*[12]*/);
/* 1 once tmx_poseidon_set_constants has been given round constants, 0 while the context still hashes with the DEFAULT ones -- the Poseidon
 * paper's Grain stream, which can never equal plonky2's table (a seeded ChaCha stream): a cap computed with them is self-consistent and
 * oracle-checked but is NOT the reference prover's commitment.  A host that wants drop-in caps must inject plonky2's ALL_ROUND_CONSTANTS,
 * hand over the extended rows in plonky2's order (it commits bit-reversed, optionally salted LDE rows; this API hashes the columns as given,
 * natural order, no salt) and should assert this returns 1. */
int32_t tmx_poseidon_constants_injected(const tmx_ctx* ctx);
uint64_t tmx_poseidon_merkle_digests(uint32_t log_n, uint32_t cap_height);
int32_t tmx_poseidon_merkle_device(tmx_ctx* ctx, uint32_t log_n, uint32_t n_cols, const uint64_t* d_cols, uint32_t cap_height, uint64_t* d_levels,
                                   void* hip_stream);
/* n permutations of caller-provided states (host buffers, 12 u64 each, blocking): test hook and micro-benchmark */
int32_t tmx_poseidon_permute(tmx_ctx* ctx, uint32_t n, const uint64_t* states_in, uint64_t* states_out);

/* ---- openings of a Poseidon Merkle tree: the query phase of a FRI-style consumer of a cap.  An opening of leaf i of a tree of 2^log_n rows
 * over n_cols columns (column-major as for tmx_poseidon_merkle_device) is
 *   row   n_cols u64: element i of every column, the stored words as they are (no reduction mod p);
 *   path  tmx_poseidon_merkle_path_len(log_n, cap_height) = log_n - cap_height digests of 4 u64, bottom-up: the sibling of the leaf first,
 *         then the sibling of its parent, ... (plonky2's MerkleProof.siblings order); path[l] = levels[off_l + ((i >> l) ^ 1)] in the layout
 *         of tmx_poseidon_merkle_device's d_levels (off_l: the start of level l).
 * It is checked as the tree was built: leaf = the row itself, canonical and zero padded, if n_cols <= 4, else hash_no_pad(row) (overwrite
 * mode: the unused rate words of a short last chunk keep their values); then for l = 0 .. path_len - 1 cur = bit l of i ? two_to_one(path[l],
 * cur) : two_to_one(cur, path[l]); accepted iff cur == cap[i >> path_len] word for word.
 * Indices are a HOST array of uint64_t, validated before anything is enqueued (n_queries >= 1 and at most 2^22, every index < 2^log_n: else
 * TMX_ERR_BAD_ARG and nothing is written), then copied to the device on hip_stream through the context's own staging: the caller may reuse
 * its array when the call returns.  Outputs are device pointers; every call is asynchronous on hip_stream.  d_paths may be NULL when the
 * paths are empty (cap_height == log_n).
 *   tmx_poseidon_merkle_open_device    openings of caller columns and their d_levels (what tmx_poseidon_merkle_device wrote for them).
 *                                      d_rows[n_queries][n_cols], d_paths[n_queries][path_len][4].
 *   tmx_trace_commit_last_shape        (log_rows + log_blowup, n_proofs * width, cap_height) of the context's most recent commit.
 *   tmx_trace_commit_open_device       openings of the context's most recent tmx_trace_commit_device: its extended columns and levels are still
 *                                      in the context's scratch.  Order it after that commit on the same stream (the rule of
 *                                      tmx_trace_rows_device), and before the next commit call overwrites the scratch.  A commit call that
 *                                      fails anywhere leaves nothing to open, and so does tmx_trace_commit_sharded_device on a rank with an
 *                                      empty shard: these two calls then return TMX_ERR_BAD_ARG (tmx_last_error says why), as on a fresh
 *                                      context.  After tmx_trace_commit_sharded_device, rank r opens the tree of ITS proofs, the one behind
 *                                      cap slot r (no collective: gathering openings across ranks is the caller's).
 *   tmx_poseidon_merkle_verify_device  d_ok[q] = 1 if opening q leads to d_cap[4 << cap_height], else 0; one thread per query (sequential:
 *                                      one permutation per 8 columns and per level).  It hashes with the context's CURRENT constants: an
 *                                      opening is checked against the caller's tables, and fails under any other.
 * The caveats of the commit hold: natural row order, no salt, injectable constants -- parity unpinned against plonky2. */
uint32_t tmx_poseidon_merkle_path_len(uint32_t log_n, uint32_t cap_height); /* log_n - cap_height; 0 if cap_height > log_n or log_n > 30 */
int32_t tmx_poseidon_merkle_open_device(tmx_ctx* ctx, uint32_t log_n, uint32_t n_cols, const uint64_t* d_cols, uint32_t cap_height,
                                        const uint64_t* d_levels, uint32_t n_queries, const uint64_t* h_indices, uint64_t* d_rows,
                                        uint64_t* d_paths, void* hip_stream);
int32_t tmx_trace_commit_last_shape(const tmx_ctx* ctx, uint32_t* log_rows_ext, uint32_t* n_cols, uint32_t* cap_height);
int32_t tmx_trace_commit_open_device(tmx_ctx* ctx, uint32_t n_queries, const uint64_t* h_indices, uint64_t* d_rows, uint64_t* d_paths,
                                     void* hip_stream);
int32_t tmx_poseidon_merkle_verify_device(tmx_ctx* ctx, uint32_t log_n, uint32_t n_cols, uint32_t cap_height, const uint64_t* d_cap,
                                          uint32_t n_queries, const uint64_t* h_indices, const uint64_t* d_rows, const uint64_t* d_paths,
                                          uint32_t* d_ok, void* hip_stream);

/* ---- a batched FRI low-degree proof over committed columns: the consumer of the cap and its openings.  PARITY UNPINNED against plonky2
 * (natural row order, no salt, injectable Poseidon constants, this project's own transcript below); everything is over the Goldilocks
 * field p = 2^64 - 2^32 + 1 and its extension F_p^2 = F_p[X] / (X^2 - 7), values (c0, c1).
 * Input: n_cols columns of M = 2^log_n u64 (column-major, words taken mod p), their evaluations on D_0 = { s w^i : i < M } with (w, s) the
 * NTT domain (tmx_ntt_set_domain) -- what tmx_lde_goldilocks_device writes -- and d_levels, tmx_poseidon_merkle_device's tree of them.  The
 * claim: every column has degree < 2^(log_n - log_blowup).
 *   batching   f_0(x_i) = sum_c alpha^c col_c[i], alpha in F_p^2.
 *   schedule   d = log_n - log_blowup; while d > final_log_max: b = min(arity_bits, d - final_log_max), append b, d -= b.  final_log = the d
 *              left (2^final_log final coefficients); zero layers if d <= final_log_max from the start.  Layer l has arity a_l = 2^b_l.
 *   domains    D_(l+1) = { y^a_l : y in D_l }: s_(l+1) = s_l^a_l, w_(l+1) = w_l^a_l, M_(l+1) = M_l / a_l, natural order.
 *   layer tree layer l is stored planar (all c0, then all c1); leaf r < M_(l+1) is the coset { r + j M_(l+1) : j < a_l }, its row (c0 of those
 *              a_l points, c1 of them): the planar buffer IS the column-major matrix of 2 a_l columns over M_(l+1) rows, and the tree is
 *              tmx_poseidon_merkle_device's tree of it (rows of <= 4 words are their own leaf), cap height h_l = min(cap_height, log M_(l+1)).
 *   fold       f(x) = sum_(j < a) x^j f_j(x^a) -> f_(l+1)(y) = sum_j beta_l^j f_j(y): b_l radix-2 folds with beta, beta^2, beta^4, ..., each
 *              g(x^2) = (f(x) + f(-x)) / 2 + beta (f(x) - f(-x)) / (2 x), x = point i, -x = point i + M / 2 (a fold stays inside a leaf).
 *   final      the last layer interpolated on its coset (inverse NTT of both planes, coefficient k times s_L^-k), the low 2^final_log
 *              coefficients kept; whether the dropped ones were all zero is recorded (tmx_fri_last_degree_ok).
 *   transcript a Poseidon duplex modelled on plonky2's Challenger, with the context's CURRENT width-12 permutation: state[12] = 0, an input
 *              and an output buffer.  observe(x): clear the output buffer, append x mod p to the input buffer, duplex when it holds 8.
 *              duplex: state[0..k) = the input buffer, clear it, permute, output buffer = state[0..8).  challenge(): duplex if the input
 *              buffer is non-empty or the output buffer empty, then pop the LAST output word.  An extension challenge = (challenge(),
 *              challenge()).  Order: observe the seven parameters (log_n, n_cols, cap_height, log_blowup, arity_bits, final_log_max,
 *              n_queries); observe the commit cap (4 << cap_height words), draw alpha; per layer observe its cap, draw beta_l; observe the
 *              final coefficients (c0, c1 of coefficient 0, then 1, ...); per query idx_q = challenge() mod 2^log_n.
 *   query q    the commit's opening of row idx_q (as tmx_trace_commit_open_device), and per layer the opening of leaf r_l = i_l mod M_(l+1)
 *              (i_0 = idx_q, i_(l+1) = r_l); the value sits at entry j_l = i_l >> log M_(l+1) of that leaf.  Checked: the commit opening
 *              against the commit cap; v = sum alpha^c row_c; per layer leaf entry j_l == v, the leaf's path against layer cap l, v = the
 *              leaf folded with beta_l; at the end v == the final polynomial at point i_L of D_L.  Any other transcript (a wrong idx_q in the
 *              proof included) rejects the query.
 * The proof is one flat buffer of u64 words (tmx_fri_layout_of gives every offset): each layer's cap; the final coefficients interleaved
 * (c0, c1); the n_queries indices; the initial rows [n_queries][n_cols] and paths [n_queries][log_n - cap_height][4]; then per layer its rows
 * [n_queries][2 a_l] (planar, as hashed) and paths [n_queries][log M_(l+1) - h_l][4].
 * Validation (every call, before anything is enqueued; TMX_ERR_BAD_ARG, nothing written, tmx_last_error says why): 1 <= log_blowup <= 6,
 * log_blowup < log_n <= 28, n_cols >= 1, cap_height <= log_n, 1 <= arity_bits <= 4, final_log_max <= 8, final_log_max + log_blowup <= 12,
 * 1 <= n_queries <= 256, reserved == 0.
 *   tmx_fri_layout_of            host only: the schedule and the offsets of the proof for these parameters.
 *   tmx_fri_prove_device         a proof over caller columns d_cols and their d_levels, under the context's CURRENT NTT domain.
 *   tmx_trace_commit_fri_device  a proof over the context's last tmx_trace_commit_device (its extended columns and tree, still in the
 *                                commit's scratch, under the domain in use at commit time).  The parameters must match that commit
 *                                (log_n = log_rows + log_blowup, n_cols, cap_height, log_blowup); with no commit to open (fresh context,
 *                                failed commit, empty shard) TMX_ERR_BAD_ARG, as for the openings.  Proving leaves the commit's scratch
 *                                untouched: its openings still work afterwards.
 *   tmx_fri_verify_device        d_ok[q] = 1 if query q of the proof checks against the commit cap d_cap[4 << cap_height], else 0.  One
 *                                workgroup: one lane re-derives the transcript from the proof, then one thread per query (latency-bound).
 *   tmx_fri_last_degree_ok       blocks until the last prove of this context finished: 1 if the dropped coefficients were zero, else 0.
 *   tmx_fri_last_ms              HIP-event times of the last prove's stages: combine, layers (trees + folds), final + transcript, openings.
 * Both provers and the verifier hash with the context's CURRENT Poseidon constants.  Prove and verify are asynchronous on hip_stream, with
 * no host synchronisation and no device-to-host copy inside (alpha, the beta_l and the query indices are drawn on the device); the prover's
 * scratch is the context's own (separate from the commit's; it grows on demand, which waits for the device once), so proves of one context
 * are ordered on one stream. */
typedef struct { uint32_t log_n, n_cols, cap_height, log_blowup, arity_bits, final_log_max, n_queries, reserved; } tmx_fri_params;
#define TMX_FRI_MAX_LAYERS 28
typedef struct {
  uint32_t n_layers, final_log;
  uint32_t layer_bits[TMX_FRI_MAX_LAYERS], layer_cap_height[TMX_FRI_MAX_LAYERS];
  uint64_t off_caps[TMX_FRI_MAX_LAYERS], off_final, off_indices, off_init_rows, off_init_paths;
  uint64_t off_rows[TMX_FRI_MAX_LAYERS], off_paths[TMX_FRI_MAX_LAYERS], words;  /* u64 offsets into the proof; words = total */
} tmx_fri_layout;
int32_t tmx_fri_layout_of(const tmx_fri_params* p, tmx_fri_layout* out);  /* host only: TMX_OK or TMX_ERR_BAD_ARG */
int32_t tmx_fri_prove_device(tmx_ctx* ctx, const tmx_fri_params* p, const uint64_t* d_cols, const uint64_t* d_levels, uint64_t* d_proof,
                             void* hip_stream);
int32_t tmx_trace_commit_fri_device(tmx_ctx* ctx, const tmx_fri_params* p, uint64_t* d_proof, void* hip_stream);
int32_t tmx_fri_verify_device(tmx_ctx* ctx, const tmx_fri_params* p, const uint64_t* d_cap, const uint64_t* d_proof, uint32_t* d_ok,
                              void* hip_stream);
int32_t tmx_fri_last_degree_ok(tmx_ctx* ctx);                  /* blocks; 1 / 0 for the last prove, TMX_ERR_BAD_ARG if none */
int32_t tmx_fri_last_ms(tmx_ctx* ctx, float ms[4]);

/* ---- out-of-domain openings (DEEP-FRI): the committed columns opened at a point the transcript picks, and at the next row.  The FRI proof
 * above then runs over the DEEP quotients instead of the raw columns, so the commitment serves as a polynomial commitment.  Same field,
 * extension, parameters, validation (plus n_cols <= 2^24), transcript duplex and caveats as the FRI block (parity unpinned against plonky2).
 * Notation: M = 2^log_n, B = 2^log_blowup, N = M / B; D_0 = { s w^i } the NTT domain as for FRI; omega_N = w^B generates the trace domain.
 *   points     the transcript observes the seven parameters as FRI does, then the word 2 (the number of points: a FRI transcript and a DEEP
 *              transcript never coincide), then the commit cap; it draws zeta = (challenge(), challenge()), again while zeta.c1 == 0, so zeta
 *              is not in F_p.  z_0 = zeta, z_1 = zeta omega_N: neither lies in F_p, so no x - z_k is zero on D_0.
 *   openings   y_(c,k) = the value at z_k of the unique polynomial of degree < N that agrees with column c (words mod p) on the points
 *              x_(jB) = s omega_N^j (j < N) of D_0.  For an honest LDE that is f_c(z_k); the definition holds for any input.
 *   digest     the openings section is planar with R = 2^ceil(log2 n_cols) rows per plane: y_(.,0).c0, y_(.,0).c1, y_(.,1).c0, y_(.,1).c1, rows
 *              n_cols and above zero.  That buffer IS the column-major 4-column matrix tmx_poseidon_merkle_device(log2 R, 4, cap_height 0)
 *              hashes (each 4-word row its own leaf); the transcript observes its root (4 words) and draws alpha.
 *   after      everything is the FRI above (layers, betas, final coefficients, query indices: the same draws in the same order), with layer 0
 *              f_0(x_i) = (F(x_i) - Y_0) / (x_i - z_0) + alpha^n_cols (F(x_i) - Y_1) / (x_i - z_1), F(x_i) = sum_c alpha^c col_c[i] and
 *              Y_k = sum_c alpha^c y_(c,k): degree < N - 1 for honest columns; schedule, layers and degree flag as for FRI.
 *   proof      the openings section (tmx_deep_openings_words(n_cols) = 4 R words), then a FRI proof laid out exactly as tmx_fri_layout_of
 *              gives it, every offset shifted by 4 R.
 *   verifier   every query is rejected if a padding word of the openings section is non-zero; opening words are taken mod p (the leaves hash
 *              canonically: y + p verifies as y); per query v_0 is the layer-0 formula at x_idx from the opened row and the Y_k the
 *              verifier forms from the openings; every other check is FRI's.  A changed opening changes the root, hence alpha, the betas
 *              and the indices: every query is rejected.
 *   tmx_deep_openings_words       host only: 4 R, or 0 if n_cols is 0 or above 2^24.
 *   tmx_deep_prove_device         a proof over caller columns d_cols (extended: the openings read the strided subset x_(jB)) and their d_levels,
 *                                 under the context's CURRENT NTT domain.
 *   tmx_trace_commit_deep_device  a proof over the context's last commit, under the rules of tmx_trace_commit_fri_device (matching parameters;
 *                                 TMX_ERR_BAD_ARG with no commit).  The openings read the commit's pre-LDE columns (1/B of the bytes, the same
 *                                 openings bit for bit); the commit's scratch is left untouched.
 *   tmx_deep_verify_device        d_ok[q] as tmx_fri_verify_device: enqueues the openings tree into a verifier scratch of the context, then the
 *                                 verifier.  Verifies of one context are ordered on one stream, as proves are.
 *   tmx_deep_last_zeta            blocks, then zeta of the last prove; TMX_ERR_BAD_ARG if there was none or it was a plain FRI prove.
 * tmx_fri_last_degree_ok and tmx_fri_last_ms report on DEEP proves too; ms[0] ("combine") then covers everything before the first layer:
 * transcript start, evaluation, openings tree, combine and quotient.  Asynchronous, no host synchronisation and no device-to-host copy
 * inside; validation before anything is enqueued (TMX_ERR_BAD_ARG: nothing written). */
#define TMX_DEEP_MAX_COLS (1u << 24)
uint64_t tmx_deep_openings_words(uint32_t n_cols);
int32_t tmx_deep_prove_device(tmx_ctx* ctx, const tmx_fri_params* p, const uint64_t* d_cols, const uint64_t* d_levels, uint64_t* d_proof,
                              void* hip_stream);
int32_t tmx_trace_commit_deep_device(tmx_ctx* ctx, const tmx_fri_params* p, uint64_t* d_proof, void* hip_stream);
int32_t tmx_deep_verify_device(tmx_ctx* ctx, const tmx_fri_params* p, const uint64_t* d_cap, const uint64_t* d_proof, uint32_t* d_ok,
                               void* hip_stream);
int32_t tmx_deep_last_zeta(tmx_ctx* ctx, uint64_t z[2]);

/* ---- proof of work (grinding): a variant of the FRI proof and of the DEEP proof above whose transcript ends with a nonce the prover has to
 * search for, so that pow_bits bits of soundness come from one word of proof and one permutation of the verifier instead of from more
 * queries.  The plain entry points, proof layouts and transcripts above are unchanged (tmx_fri_params.reserved stays refused when non-zero);
 * the new parameter has a struct of its own.  Same field, duplex, caveats (parity unpinned against plonky2) as the blocks above.
 *   parameters tmx_pow_params { fri, pow_bits, deep }: deep = 0 the FRI proof, 1 the DEEP proof.  Validation is that of the underlying proof
 *              (FRI's rules; n_cols <= 2^24 when deep), plus 1 <= pow_bits <= TMX_POW_MAX_BITS (24) and deep <= 1: TMX_ERR_BAD_ARG, nothing
 *              written, tmx_last_error says why, before anything is enqueued.  The bound 24 keeps the longest possible search short on a
 *              shared device (see "bound").
 *   transcript exactly the FRI (deep: the DEEP) transcript up to and including the final coefficients.  Then
 *              1. observe(pow_bits): a proof made for one pow_bits does not verify under another, and no grinding transcript coincides with
 *                 a plain one (which draws the indices right after the final coefficients);
 *              2. the nonce is the SMALLEST n in 0, 1, 2, ... such that, on a copy of the duplex at this point, observe(n) followed by
 *                 r = challenge() gives r < 2^(64 - pow_bits) (r is canonical: its top pow_bits bits are zero).  Whatever the input buffer
 *                 holds after step 1, a candidate costs one permutation (if step 1 filled the buffer, that duplex happens once, before the
 *                 search).  Smallest, not any: the proof is a function of its inputs;
 *              3. the real transcript does observe(nonce), challenge() (the same r, consumed), and goes on with the query indices from the
 *                 remaining output words, as the plain transcript does.
 *   proof      the FRI (deep: the DEEP) proof laid out as above, then one more word, the nonce.  tmx_pow_proof_words gives the total:
 *              tmx_fri_layout_of(...).words + 1, plus tmx_deep_openings_words(n_cols) when deep; 0 for parameters that do not validate.
 *   verifier   as above, plus: every query is rejected if the nonce word is >= p, or if r has fewer than pow_bits leading zero bits.  A
 *              changed nonce that still satisfies the condition changes the indices, so the index check rejects every query, as it does
 *              for any other change of the transcript.
 *   bound      the search gives up after 2^(pow_bits + 6) candidates (an honest search fails with probability about e^-64).  Then the nonce
 *              word is written as 2^64 - 1 (which the verifier rejects), the rest of the proof is still written, and tmx_pow_last reports
 *              it.  This makes the search's running time finite by construction: at most 2^30 permutations, under half a second at the
 *              bulk Poseidon rate.  It cannot be reached with honest inputs, so no test reaches it.
 *   tmx_pow_proof_words          host only.
 *   tmx_pow_prove_device         a proof over caller columns, as tmx_fri_prove_device / tmx_deep_prove_device.
 *   tmx_trace_commit_pow_device  a proof over the context's last commit, under the rules of tmx_trace_commit_fri_device.
 *   tmx_pow_verify_device        d_ok[q] as tmx_fri_verify_device / tmx_deep_verify_device.
 *   tmx_pow_last                 blocks like tmx_fri_last_degree_ok, then the nonce of the last prove and the number of candidates the search
 *                                evaluated (either pointer may be null; the count depends on timing: rounds in flight finish).
 *                                TMX_ERR_BAD_ARG if there was no prove or the last one was not a grinding prove; TMX_ERR_CAPACITY, with both
 *                                values still written (nonce = 2^64 - 1), if the search gave up.
 * tmx_fri_last_degree_ok, tmx_fri_last_ms and (deep) tmx_deep_last_zeta report on grinding proves too; the search's time is part of ms[2]
 * ("final + transcript").  Prove and verify are asynchronous on hip_stream, no host synchronisation and no device-to-host copy inside: the
 * search is one launch that ends itself. */
#define TMX_POW_MAX_BITS 24
typedef struct { tmx_fri_params fri; uint32_t pow_bits, deep; } tmx_pow_params;
uint64_t tmx_pow_proof_words(const tmx_pow_params* pp);
int32_t tmx_pow_prove_device(tmx_ctx* ctx, const tmx_pow_params* pp, const uint64_t* d_cols, const uint64_t* d_levels, uint64_t* d_proof,
                             void* hip_stream);
int32_t tmx_trace_commit_pow_device(tmx_ctx* ctx, const tmx_pow_params* pp, uint64_t* d_proof, void* hip_stream);
int32_t tmx_pow_verify_device(tmx_ctx* ctx, const tmx_pow_params* pp, const uint64_t* d_cap, const uint64_t* d_proof, uint32_t* d_ok,
                              void* hip_stream);
int32_t tmx_pow_last(tmx_ctx* ctx, uint64_t* nonce, uint64_t* tried);

/* ---- one DEEP-FRI proof over several oracles of different sizes, and the commit set it consumes.  The entry points above work on ONE
 * committed section; a batch's trace is five row tables of different heights, and a consumer needs all of them opened at the SAME
 * out-of-domain point.  This block adds a commit set (several sections committed and kept resident side by side) and one proof over a list
 * of committed oracles: ONE zeta, one set of layers, one final polynomial, one query set.  plonky2's `prove` (what the reference calls,
 * circuits/skip.rs:119-133) opens several oracles in one FRI proof; this is that capability in the project's own format.  Nothing above
 * changes: the single-commit entry points, proofs, layouts, transcripts and scratch are what they were.  Same field, extension
 * F_p^2 = F_p[X] / (X^2 - 7), Poseidon duplex, NTT domain convention and caveats as the FRI and DEEP blocks (natural order, no salt,
 * injectable constants, the project's own transcript: PARITY UNPINNED against plonky2).
 *   oracles    K oracles, 1 <= K <= TMX_BATCH_MAX_ORACLES (8).  Oracle k is n_cols_k columns of M_k = 2^log_n_k words (column-major, taken
 *              mod p): evaluations on D^(k) = { s w_k^i }, w_k the 2^log_n_k-th root of the NTT domain and THE SAME coset shift s for every
 *              size (what tmx_lde_goldilocks_device writes), with its own Poseidon tree (tmx_poseidon_merkle_device) of cap height
 *              h_k = min(cap_height, log_n_k).  One log_blowup B for all; N_k = M_k / 2^B; the claim is degree < N_k for every column of
 *              oracle k.  The list is ordered by non-increasing log_n_k; equal sizes are allowed.  off_k = n_cols_0 + ... + n_cols_(k-1),
 *              C = sum n_cols_k (C <= 2^24).  A group g is the set of oracles of one size; the distinct sizes are m^(0) > ... > m^(G-1).
 *   parameters tmx_batch_params.  TMX_ERR_BAD_ARG before anything is enqueued (nothing written, tmx_last_error says which rule): the FRI
 *              rules on every oracle (1 <= log_blowup <= 6, log_blowup < log_n_k <= 28, n_cols_k >= 1, 1 <= arity_bits <= 4,
 *              final_log_max <= 8, final_log_max + log_blowup <= 12, 1 <= n_queries <= 256, reserved == 0), cap_height <= log_n_0,
 *              pow_bits <= TMX_POW_MAX_BITS (0 = no grinding), the ordering rule, C <= 2^24, unused array entries zero.
 *   schedule   d = m^(0) - B.  For g = 0 .. G - 2: gap = m^(g) - m^(g+1); while gap > 0: b = min(arity_bits, gap), append b, gap -= b,
 *              d -= b.  Then FRI's rule on what is left: while d > final_log_max: b = min(arity_bits, d - final_log_max), append b, d -= b.
 *              final_log = d.  So a layer boundary falls on every distinct oracle size whatever arity_bits is.  Layer domains, layer trees,
 *              leaves, cap heights, final polynomial and degree flag are FRI's, unchanged.
 *   transcript observe 2^32 + K (no FRI / DEEP / grinding transcript starts with a word >= 2^32, so none coincides), then log_blowup,
 *              cap_height, arity_bits, final_log_max, n_queries, pow_bits, then (log_n_k, n_cols_k) for each k, then the word 2, then the K
 *              commit caps in order (4 << h_k words each).  zeta as DEEP draws it (again while zeta.c1 == 0).  Points of oracle k:
 *              z_(k,0) = zeta, z_(k,1) = zeta omega_(N_k), omega_(N_k) = w_k^(2^B).  Openings y_(k,c,j) as DEEP defines them, on oracle k's own
 *              subset x_(i 2^B).  Openings section: K blocks in order, block k exactly DEEP's planar section for n_cols_k (4 R_k words,
 *              R_k = 2^ceil(log2 n_cols_k), zero padding), each hashed as DEEP hashes its section; the transcript observes the K roots in
 *              order (4 words each) and draws ONE alpha.  After that: per layer its cap -> beta_l; the final coefficients; if pow_bits > 0
 *              the grinding steps 1 - 3 exactly as the proof-of-work block defines them; indices idx_q = challenge() mod 2^(m^(0)).
 *   layers     for oracle k and i < M_k, x = s w_k^i:  F_k(x) = sum_c alpha^(off_k + c) col_(k,c)[i],  Y_(k,j) = sum_c alpha^(off_k + c) y_(k,c,j),
 *              Q_k[i] = (F_k(x) - Y_(k,0)) / (x - z_(k,0)) + alpha^C (F_k(x) - Y_(k,1)) / (x - z_(k,1));  Q^(g)[i] = sum of Q_k[i] over group g.
 *              Layer 0 = Q^(0).  The fold from layer l (arity a_l) is FRI's, and when the new layer has 2^(m^(g)) points for some g >= 1 the
 *              group enters it INDEX FOR INDEX, scaled by the first power of beta_l the fold did not use:
 *              f_(l+1)[i] = sum_(j < a_l) beta_l^j f_j(...) + beta_l^(a_l) Q^(g)[i].
 *              The one non-obvious step: layer l + 1's nominal domain has shift s^(a_0 ... a_l), the group's has shift s.  Reading a vector of
 *              evaluations on one coset as evaluations on another coset of the same subgroup substitutes x -> c x in the polynomial: its
 *              degree is the same, so the low-degree claim carries over, and the sum of the two vectors is low-degree exactly if (up to the
 *              random beta_l) both are.  The verifier therefore uses each oracle's OWN x for Q_k and the layer's own x for the folds.
 *   query q    i_0 = idx_q, i_(l+1) = i_l mod M_(l+1) as in FRI.  Oracle k is opened at row idx_q mod M_k (a row of n_cols_k words and a path
 *              of log_n_k - h_k digests, as tmx_poseidon_merkle_open_device); layers as in FRI.  Checks: each oracle opening against its
 *              cap; v_0 = Q^(0) from the opened rows of group 0 and the Y sums the verifier forms from the openings section; per layer: leaf
 *              entry == v, path against the layer cap, v = leaf folded with beta_l, plus beta_l^(a_l) Q^(g) from the opened rows of group g
 *              when that layer takes one in; at the end v == the final polynomial at point i_L.  A non-zero padding word in any openings
 *              block, a nonce >= p or a failed grinding condition rejects every query.
 *   proof      one flat u64 buffer, every offset in tmx_batch_layout: the K openings blocks; the layer caps; the final coefficients
 *              (c0, c1); the indices; for k = 0 .. K - 1 the oracle rows [n_queries][n_cols_k] and paths [n_queries][log_n_k - h_k][4]; per
 *              layer its rows and paths as FRI; one nonce word if pow_bits > 0 (off_nonce; == words without grinding).
 *              layer_enter[l] = g >= 1: the fold of layer l takes group g in; 0: a plain fold.
 * A K = 1 batch proof is a different transcript from a DEEP proof of the same oracle and does not equal it.
 *   tmx_batch_layout_of                host only.
 *   tmx_batch_prove_device             caller oracles (d_cols[k], d_levels[k]: what tmx_lde_goldilocks_device / tmx_poseidon_merkle_device
 *                                      wrote for oracle k; host arrays of K device pointers), under the context's CURRENT NTT domain.
 *   tmx_batch_verify_device            d_caps: the K caps concatenated in order; d_ok[q] as tmx_fri_verify_device.
 *   tmx_trace_commit_set_device        commits every section of the mask `sections` (row tables only: TMX_TRACE_MATCH refused) through the
 *                                      stages of tmx_trace_commit_device into a scratch of the SET'S OWN, where the pre-LDE columns, extended
 *                                      columns and tree levels of every section stay resident together.  Oracle order: by decreasing
 *                                      log_rows, ties by ascending section bit; d_caps receives the caps in that order (4 << h_k words each),
 *                                      each word for word what tmx_trace_commit_device writes for that section alone.  It does not touch the
 *                                      last single commit or its scratch, and tmx_trace_commit_device does not touch the set: both can be
 *                                      open at once.  A call that fails anywhere leaves no set.  The scratch is checked against free memory
 *                                      before allocation (the rule of tmx_trace_commit_device summed over the sections): TMX_ERR_CAPACITY.  At
 *                                      256 proofs x N = 128 and blow-up 8 the ladders section alone needs > 200 GB, so a full-size set holds
 *                                      the other four (about 55 GB + the LDE's scratch; derived from that formula, not measured).
 *   tmx_trace_commit_set_shape         the set's oracle list into out (n_oracles, log_blowup, cap_height, log_n[], n_cols[]; the other
 *                                      fields zero, for the caller to fill) and each oracle's section bit; TMX_ERR_BAD_ARG with no set.
 *   tmx_trace_commit_set_prove_device  a proof over the set; the oracle list, log_blowup and cap_height must match it (TMX_ERR_BAD_ARG).  The
 *                                      openings read the set's pre-LDE columns, as tmx_trace_commit_deep_device does; the set stays intact.
 * tmx_fri_last_degree_ok, tmx_fri_last_ms, tmx_deep_last_zeta and (pow_bits > 0) tmx_pow_last report on batch proves too; ms[0] covers
 * everything before the first layer, over all oracles.  Asynchronous on hip_stream, no host synchronisation and no device-to-host copy
 * inside; the prover's scratch is the FRI provers' (grows on demand). */
#define TMX_BATCH_MAX_ORACLES 8
typedef struct {
  uint32_t n_oracles, log_blowup, cap_height, arity_bits, final_log_max, n_queries, pow_bits, reserved;
  uint32_t log_n[TMX_BATCH_MAX_ORACLES], n_cols[TMX_BATCH_MAX_ORACLES];
} tmx_batch_params;
typedef struct {
  uint32_t n_layers, final_log, n_groups, reserved;
  uint32_t layer_bits[TMX_FRI_MAX_LAYERS], layer_cap_height[TMX_FRI_MAX_LAYERS], layer_enter[TMX_FRI_MAX_LAYERS];
  uint32_t group_of[TMX_BATCH_MAX_ORACLES], cap_height_of[TMX_BATCH_MAX_ORACLES];
  uint64_t off_open[TMX_BATCH_MAX_ORACLES], off_caps[TMX_FRI_MAX_LAYERS], off_final, off_indices;
  uint64_t off_init_rows[TMX_BATCH_MAX_ORACLES], off_init_paths[TMX_BATCH_MAX_ORACLES];
  uint64_t off_rows[TMX_FRI_MAX_LAYERS], off_paths[TMX_FRI_MAX_LAYERS], off_nonce, words;  /* u64 offsets into the proof; words = total */
} tmx_batch_layout;
int32_t tmx_batch_layout_of(const tmx_batch_params* p, tmx_batch_layout* out);  /* host only: TMX_OK or TMX_ERR_BAD_ARG */
int32_t tmx_batch_prove_device(tmx_ctx* ctx, const tmx_batch_params* p, const uint64_t* const d_cols[], const uint64_t* const d_levels[],
                               uint64_t* d_proof, void* hip_stream);
int32_t tmx_batch_verify_device(tmx_ctx* ctx, const tmx_batch_params* p, const uint64_t* d_caps, const uint64_t* d_proof, uint32_t* d_ok,
                                void* hip_stream);
int32_t tmx_trace_commit_set_device(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, uint32_t sections, uint32_t log_blowup, uint32_t cap_height,
                                    const void* d_trace_rows, uint64_t* d_caps, void* hip_stream);
int32_t tmx_trace_commit_set_shape(const tmx_ctx* ctx, tmx_batch_params* out, uint32_t section_of[TMX_BATCH_MAX_ORACLES]);
int32_t tmx_trace_commit_set_prove_device(tmx_ctx* ctx, const tmx_batch_params* p, uint64_t* d_proof, void* hip_stream);

/* ---- streamed members of a commit set ----------------------------------------------------------------------------------------------
 * A resident member of a commit set keeps its extended columns (n_cols << log_n words) and the LDE wants twice that again as scratch: at 256
 * proofs x N = 128 and blow-up 8 the ladders section alone would ask for about 218 GB.  None of those words has to stay:
 *   - the leaf sponge absorbs a row eight columns at a time and can stop after any multiple of eight and go on from its 12-word state;
 *   - the openings at zeta, zeta omega read the pre-LDE columns;
 *   - F_k = sum alpha^c col_c is F_p-linear in the columns and so is the LDE: combining the pre-LDE columns and extending the two planes of
 *     the result gives the same canonical words as combining the extended columns;
 *   - the queried rows are produced after the indices are drawn, by extending the columns once more, a chunk at a time.
 * A STREAMED member therefore keeps in the set's scratch its pre-LDE columns and its tree levels, nothing else of its own.  All streamed
 * members share one sponge-state buffer ([12][2^log_n] words, planar) and one chunk buffer (chunk_cols << log_n words), sized by the tallest.
 * The chunk rule: chunk_cols is a multiple of 8, at least 8, so every chunk but a member's last ends on a block boundary of the sponge.  A
 * member of `streamed` whose n_cols <= chunk_cols fits one chunk and is kept resident.
 * THE EQUALITY PROMISE: the caps, tmx_trace_commit_set_shape, and every word of tmx_trace_commit_set_prove_device's proof (and so the
 * transcript, zeta, the layout and the verifier) are those of the resident set of the same sections, whatever `streamed` and chunk_cols.
 *   tmx_trace_commit_set_bytes            host only: the bytes tmx_trace_commit_set_streamed_device checks against free memory before it
 *                                         allocates -- the set's scratch (per member: pre-LDE columns + extended columns unless streamed +
 *                                         levels; then the state and chunk buffers if any member is streamed) plus the LDE's own scratch,
 *                                         twice the largest thing extended at once (a resident member's extended columns, or the chunk
 *                                         buffer).  0 for arguments the commit would refuse.
 *   tmx_trace_commit_set_streamed_device  tmx_trace_commit_set_device with the members of the mask `streamed` (a subset of `sections`)
 *                                         streamed in chunks of chunk_cols columns; chunk_cols is checked even when nothing is streamed.
 *                                         Anything else -> TMX_ERR_BAD_ARG before anything is enqueued; a failed call leaves no set.
 *                                         streamed == 0 is tmx_trace_commit_set_device exactly.  TMX_COMMIT_SET_CHUNK_COLS is the smallest
 *                                         chunk of the measured sweep (256 .. 2048) within spread of the fastest commit: the
 *                                         state round trip, 192 B per row and chunk, is 9 % of the column traffic there and hides.
 * tmx_trace_commit_set_prove_device works on a set with streamed members unchanged.  It extends a streamed member's two planes of F_k (into
 * the group's buffer if the member opens its size group, else next to it and added in) and, after the indices are drawn, every chunk once
 * more to gather the queried rows: that second LDE pass is the price of streaming.  These LDEs run under the domain the set was committed
 * with: if tmx_ntt_set_domain has changed the context's since, the prove puts the set's domain back for its own duration and restores the
 * caller's before it returns -- the one case in which this call waits for the device. */
#define TMX_COMMIT_SET_CHUNK_COLS 256
uint64_t tmx_trace_commit_set_bytes(int32_t kind, uint32_t n_max, uint32_t n_proofs, uint32_t sections, uint32_t streamed, uint32_t chunk_cols,
                                    uint32_t log_blowup, uint32_t cap_height);
int32_t tmx_trace_commit_set_streamed_device(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, uint32_t sections, uint32_t streamed,
                                             uint32_t chunk_cols, uint32_t log_blowup, uint32_t cap_height, const void* d_trace_rows,
                                             uint64_t* d_caps, void* hip_stream);

/* ---- the constraint quotient of the ladder rows -------------------------------------------------------------------------------------
 * The proofs above show that committed columns are low-degree and that their openings are right; they say nothing about the rows.  This
 * block adds the step plonky2's `prove` takes between the commitment and the openings -- the constraint quotient -- for the ladders table
 * (TMX_TRACE_LADDERS): a second oracle q, committed after the trace, with  sum gamma^i C_i(x) = q(x) (x^N - 1)  checked at zeta from the
 * openings every batch proof already carries (each column at zeta AND at the next row, zeta omega_N).  Same field, extension, duplex, NTT
 * domain convention and caveats as the FRI / DEEP / batch blocks (PARITY UNPINNED against plonky2); nothing above changes.
 *   table      n_proofs * 65 columns over M = 2^log_n points x_i = s w^i (tmx_lde_goldilocks_device's output), N = M / 2^log_blowup rows;
 *              the "next row" of point i is point (i + 2^log_blowup) mod M.  Column offsets inside a proof's 65: bit 0, acc 1 .. 16,
 *              dbl 17 .. 32, add 33 .. 48, nxt 49 .. 64; each point is its x limbs, then its y limbs; words taken mod p.
 *   constraints  the ones that are polynomial in the columns as they stand (32-bit limbs, no helper columns), 33 per proof:
 *              C_0      = bit^2 - bit
 *              C_(1+l)  = nxt_l - dbl_l - bit (add_l - dbl_l)                l < 16
 *              C_(17+l) = S(x) (acc_l(omega_N x) - nxt_l(x))                 l < 16
 *              S(x) = x^(N/256) - omega_256^-1, omega_256 = omega_N^(N/256): zero exactly on the rows r = 255 mod 256, so neither the seam
 *              between two ladders nor the wrap-around is constrained.  Zero padding rows and the all-zero ladders of undecodable lanes
 *              satisfy all 33, which is why the boundary acc_0 = (0, 1) is NOT in the set.
 *   NOT PROVED by this block (the follow-ups): the curve arithmetic (dbl = 2 acc, add = dbl + P), the limb ranges, the boundary rows, the
 *              link to the Level-1 points, and every SHA table.  A changed acc at r = 0, dbl where bit = 1 or add where bit = 0 goes
 *              undetected (tests/test_air.py records it).  The boundary rows and the link to the Level-1 points are constraint set 2,
 *              the next block.
 *   challenge  a fresh duplex (as the FRI block defines it): observe 2^33 (no other transcript starts at or above 2^32 except the batch's
 *              2^32 + K, K <= 8), then the constraint-set id 1, log_n, log_blowup, cap_height, n_proofs, then the trace cap
 *              (4 << min(cap_height, log_n) words); gamma = (challenge(), challenge()), drawn again while gamma.c1 == 0.
 *   quotient   q(x_i) = (sum_p sum_(j < 33) gamma^(33 p + j) C_(p,j)(x_i)) / (x_i^N - 1) in F_p^2, written planar (all c0, then all c1),
 *              canonical: the buffer IS a column-major 2-column oracle of log_n rows.  Pointwise: defined for any input columns, satisfying
 *              or not (x^N - 1 has no zero on the coset).  For satisfying rows of degree < N it has degree < N (measured: N - 2).
 *   identity   t^0, t^1 the trace openings at zeta and zeta omega_N, u_0, u_1 the quotient columns' openings at zeta:
 *              sum gamma^(33 p + j) C_(p,j)(t^0, t^1; zeta) == (u_0 + X u_1) (zeta^N - 1),  X (a, b) = (7 b, a).
 *   binding    gamma depends on the trace cap only; the batch transcript observes both caps before it draws zeta.  The batch proof is
 *              used UNCHANGED: the quotient is one more oracle, directly after its table (same log_n, n_cols = 2).
 *   tmx_air_ladder_quotient_device        gamma from d_cap, then the quotient of caller columns d_cols into d_quot (2 << log_n words), under
 *                                         the context's CURRENT NTT domain.  TMX_ERR_BAD_ARG before anything is enqueued: FRI's rules on log_n
 *                                         and log_blowup, log_n - log_blowup >= 8, n_proofs >= 1, 65 n_proofs <= 2^24.
 *   tmx_air_ladder_quotient_range_device  the same over the proofs [proof_lo, proof_hi) of the table only (d_cols still the whole table's
 *                                         column 0; gamma still over n_proofs), added to what d_quot holds if accumulate = 1: a table fed in
 *                                         pieces gives the same words.  Also refused: an empty range, proof_hi > n_proofs, accumulate > 1.
 *   tmx_air_last_gamma                    blocks, then gamma of the last quotient call (set-level included); TMX_ERR_BAD_ARG if none.
 *   tmx_air_verify_device                 tmx_batch_verify_device, then the identity for oracle k_trace (the table) and k_trace + 1 (its
 *                                         quotient): a failed identity rejects every query.  TMX_ERR_BAD_ARG unless oracle k_trace has a
 *                                         multiple of 65 columns and oracle k_trace + 1 the same log_n and 2 columns (and the rules above).
 *   tmx_trace_commit_set_air_device       on a commit set that holds TMX_TRACE_LADDERS: gamma from the ladders' cap, the quotient, its
 *                                         Poseidon tree (d_cap_q receives 4 << min(cap_height, log_n) words), and the quotient registered as
 *                                         a member right after the ladders.  tmx_trace_commit_set_shape then reports K + 1 oracles with
 *                                         TMX_TRACE_LADDERS_QUOTIENT in section_of, and tmx_trace_commit_set_prove_device proves the enlarged
 *                                         list as it is (the quotient has no pre-LDE columns: its openings read the strided subset of its
 *                                         extended columns, the same words by definition).  A STREAMED ladders member is fed in chunks of
 *                                         floor(chunk_cols / 65) whole proofs, each extended once more into the set's chunk buffer under the
 *                                         set's domain, the kernel accumulating: TMX_ERR_BAD_ARG if chunk_cols < 65.  The equality promise
 *                                         extends: the quotient cap and every proof word equal the resident set's.  A second call on the same
 *                                         set, a set without the ladders or a full set (8 oracles) is refused; a set without the call behaves
 *                                         exactly as before.
 * Asynchronous on hip_stream, no host synchronisation and no device-to-host copy inside (gamma is drawn on the device and stays there);
 * the scratch is the context's own (grows on first use, which waits for the device once). */
#define TMX_TRACE_LADDERS_QUOTIENT 64u
int32_t tmx_air_ladder_quotient_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                       const uint64_t* d_cols, const uint64_t* d_cap, uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_ladder_quotient_range_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                             uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                             const uint64_t* d_cap, uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_last_gamma(tmx_ctx* ctx, uint64_t g[2]);
int32_t tmx_air_verify_device(tmx_ctx* ctx, const tmx_batch_params* p, uint32_t k_trace, const uint64_t* d_caps, const uint64_t* d_proof,
                              uint32_t* d_ok, void* hip_stream);
int32_t tmx_trace_commit_set_air_device(tmx_ctx* ctx, uint64_t* d_cap_q, void* hip_stream);

/* ---- the boundary constraints of the ladder rows (constraint set 2) ------------------------------------------------------------------
 * Set 1 above holds for ANY chain of acc / nxt values, wherever it starts and ends, and it is blind on row 255 of a ladder (the chain is
 * switched off there: dbl / add and nxt can change together).  Set 2 is set 1 plus 32 boundary constraints per proof that pin the first
 * accumulator and the last nxt of every ladder to a PUBLIC TABLE the verifier holds: the Level-1 end points s*B and h*A of every lane, which
 * the element rows already carry (D.1b, docs/witness_layout.md).  Built beside set 1: set 1's transcript, gamma, quotient words, kernels and
 * calls are what they were; the proof format, the batch prover and the batch verifier do not change; the quotient is again one two-column
 * oracle directly behind its table (TMX_TRACE_LADDERS_QUOTIENT).  Notation as above: N rows, M = N B points x_i = s w^i, omega = omega_N,
 * K = N / 256 ladders (padding included), S(x) = x^K - omega_256^-1 (zero exactly on the last rows r = 255 mod 256).  2 <= K <= 2^12, i.e.
 * 9 <= log_n - log_blowup <= 20: TMX_ERR_BAD_ARG outside.
 *   pub        the public table, column-major, 17 n_proofs columns of K rows, canonical words.  Column 17 p + l, l < 16, row k: limb l of the
 *              Level-1 end point of ladder k of proof p (x limbs, then y limbs); ladder 2 i is s*B of lane i, ladder 2 i + 1 is h*A.
 *              Column 17 p + 16, row k: live = 1 if the 16 end words are not all zero, else 0.  Ladders beyond 2 n_max (padding) and lanes
 *              whose Level-1 points are zero are all zero; (0, 0) is not on the curve, so live is well defined.
 *   constraints  65 per proof: C_0 .. C_32 as in set 1, and with T(x) = (x^N - 1) / S(x)
 *              C_(33+l) = T(x) (nxt_l(x) - E_l(x))                       l < 16    E_l of degree < K, E_l(omega^(256 k + 255)) = pub[17 p + l][k]
 *              C_(49+l) = T(x) (acc_l(omega x) - [l = 8] L(x))           l < 16    L of degree < K, L(omega^(256 k + 255)) = pub[17 p + 16][(k + 1) mod K]
 *              The second group states the first-row boundary acc_0 = (0, live) on the row BEFORE it (the wrap-around included), so that both
 *              groups share the row set and the divisor, and it reads acc(omega x) only: acc at the lane's own row stays unread.
 *   NOT PROVED by set 2: the curve arithmetic (dbl = 2 acc, add = dbl + P), the limb ranges, and every SHA table.  dbl where bit = 1 and
 *              add where bit = 0 still go undetected (tests/test_air_boundary.py records it).
 *   challenge  a transcript of its own, as set 1's with the set id 2: observe 2^33, then 2, log_n, log_blowup, cap_height, n_proofs, then the
 *              trace cap, then the four words of the PUBLIC DIGEST: the Poseidon Merkle root (cap height 0) of pub taken as a column-major
 *              oracle of log2 K rows and 17 n_proofs columns, exactly as tmx_poseidon_merkle_device defines it.  gamma drawn as in set 1.
 *   quotient   weights gamma^(65 p + j).  The public side collapses to one F_p^2 polynomial:
 *              V_k = sum_p [ sum_(l < 16) gamma^(65 p + 33 + l) pub[17 p + l][k] + gamma^(65 p + 57) pub[17 p + 16][(k + 1) mod K] ]
 *              Pub_gamma = the interpolant of degree < K of V_k on the points y_k = omega^(256 k + 255)
 *              q(x_i) = [sum_p sum_(j < 33) gamma^(65 p + j) C_(p,j)(x_i)] / (x_i^N - 1)
 *                     + [sum_p sum_(l < 16) (gamma^(65 p + 33 + l) nxt_(p,l)(x_i) + gamma^(65 p + 49 + l) acc_(p,l)(omega x_i)) - Pub_gamma(x_i)] / S(x_i)
 *              planar and canonical as in set 1; pointwise defined for any columns and any pub.  In the range form the piece with
 *              proof_lo == 0 carries the - Pub_gamma / S term: any split into whole-proof pieces adds up to the same words.  For satisfying
 *              rows of degree < N it has degree < N (measured: N - 2; the boundary part alone N - 1 - K).
 *   identity   division-free, with Z = zeta^N - 1, t^0, t^1, u_0, u_1 as in set 1:
 *              S(zeta) sum_p sum_(j < 33) gamma^(65 p + j) C_(p,j)(t^0, t^1; zeta)
 *                + Z [sum_p sum_l (gamma^(65 p + 33 + l) t^0[nxt_(p,l)] + gamma^(65 p + 49 + l) t^1[acc_(p,l)]) - Pub_gamma(zeta)]
 *                == (u_0 + X u_1) Z S(zeta)
 *              Pub_gamma(zeta) = S(zeta) / (K omega_256^-1) sum_k V_k y_k / (zeta - y_k), from the verifier's own V_k.  A failed identity
 *              clears every query's verdict.
 *   tmx_air_ladder_public_shape           host only: log2 K and the column count 17 n_proofs of pub for (kind, n_max, n_proofs);
 *                                         TMX_ERR_BAD_ARG if the ladders table of that shape has K outside 2 .. 2^12 or n_proofs = 0.
 *   tmx_air_ladder_public_device          pub (17 n_proofs << log2 K words at d_pub) from the element rows as tmx_witness_batch_device leaves
 *                                         them (u64, row stride tmx_elem_stride, section D.1b) for the context's n_max.
 *   tmx_air_ladder_boundary_quotient_device, .._range_device   as tmx_air_ladder_quotient_device / _range_device plus d_pub: the digest and
 *                                         gamma, then (proof_lo == 0) V, Pub_gamma on the coset, then the pass.  Set 1's rules, and
 *                                         log_n - log_blowup in 9 .. 20.
 *   tmx_air_boundary_verify_device        tmx_batch_verify_device, then the set-2 identity with d_pub (the verifier hashes d_pub itself).
 *                                         tmx_air_verify_device's rules, and log_n - log_blowup in 9 .. 20, d_pub set.
 *   tmx_trace_commit_set_air_boundary_device   tmx_trace_commit_set_air_device for set 2: resident and streamed ladders members (chunks of
 *                                         whole proofs, re-extended under the set's domain, accumulating), the same quotient member
 *                                         registered.  Pub_gamma is extended by kernels of its own from the set's root and shift, not through
 *                                         the context's NTT domain.  The two set-level calls exclude each other on one set: whichever comes
 *                                         second is refused.  The equality promise extends as for set 1.
 * Every refusal comes before anything is enqueued; everything is asynchronous on hip_stream; tmx_air_last_gamma covers these calls too. */
int32_t tmx_air_ladder_public_shape(int32_t kind, uint32_t n_max, uint32_t n_proofs, uint32_t* log_k, uint32_t* n_cols);
int32_t tmx_air_ladder_public_device(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, const void* d_elems, uint64_t* d_pub, void* hip_stream);
int32_t tmx_air_ladder_boundary_quotient_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                const uint64_t* d_cols, const uint64_t* d_cap, const uint64_t* d_pub, uint64_t* d_quot,
                                                void* hip_stream);
int32_t tmx_air_ladder_boundary_quotient_range_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                      uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                      const uint64_t* d_cap, const uint64_t* d_pub, uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_boundary_verify_device(tmx_ctx* ctx, const tmx_batch_params* p, uint32_t k_trace, const uint64_t* d_caps, const uint64_t* d_proof,
                                       const uint64_t* d_pub, uint32_t* d_ok, void* hip_stream);
int32_t tmx_trace_commit_set_air_boundary_device(tmx_ctx* ctx, const uint64_t* d_pub, uint64_t* d_cap_q, void* hip_stream);

/* ---- the round constraints of the SHA-256 tables (constraint set 3) ---------------------------------------------------------------------
 * Sets 1 and 2 argue about the ladders; three of the five committed row tables are SHA-256 round tables -- T.3 the validator leaf hashes
 * (TMX_TRACE_SHA256), T.5 the validator-tree nodes (TMX_TRACE_TREE), T.6 the header inclusion proofs (TMX_TRACE_HEADER) -- and the proofs
 * above say nothing about their rows.  Set 3 proves the SHA-256 ROUND FUNCTION on them: a helper oracle of bits committed behind the table,
 * 315 constraints per proof, one two-column quotient oracle behind the helper, and the identity at zeta.  Built beside sets 1 and 2: no
 * existing kernel, transcript phase, proof word or call changes; the batch prover, its proof format and tmx_batch_verify_device are used
 * UNCHANGED.  Notation as above: N rows, M = N B points x_i = s w^i, omega = omega_N, omega_64 = omega^(N/64) (N >= 64),
 * S(x) = x^(N/64) - omega_64^-1 (zero exactly on the rows r = 63 mod 64), K(x) = P_K(x^(N/64)) with P_K of degree < 64 and
 * P_K(omega_64^t) = K256[t], the SHA-256 round constants.  Same field, extension, duplex and caveats as the blocks above (PARITY UNPINNED).
 *   table      9 n_proofs columns; inside a proof W 0, a 1, b 2, c 3, d 4, e 5, f 6, g 7, h 8; row t of a block holds W_t and the state after
 *              round t (docs/level2_rows.md); every block sits on a 64-row boundary.
 *   helper     300 columns per proof, the table's rows, bits LSB first.  Offsets inside a proof:
 *                0 .. 31   A   bits of a            128 .. 159  F   bits of f             256 .. 287  V   V_i = A_i B_i
 *               32 .. 63   B   bits of b            160 .. 191  G   bits of g             288 S0 = Sigma0(a)   289 S1 = Sigma1(e)   (words)
 *               64 .. 95   C   bits of c            192 .. 223  U0  U0_i = A_(i+2) xor A_(i+13)   290 CH = Ch(e,f,g)   291 MAJ = Maj(a,b,c)
 *               96 .. 127  E   bits of e            224 .. 255  U1  U1_i = E_(i+6) xor E_(i+11)   292 LIVE   293 KL   294 .. 296 CA   297 .. 299 CE
 *              (indices of A and E mod 32).  LIVE = 1 iff row r - r mod 64 of the proof's table has a nonzero word; KL = LIVE K256[r mod 64];
 *              CA, CE the carry bits of the a and e updates.  Defined for ANY input: the operands are the low 32 bits of each table word;
 *              on rows r != 63 mod 64, with primed values from row r + 1,  CA = ((h + S1 + CH + KL' + W' + S0 + MAJ) >> 32) & 7  and
 *              CE = ((d + h + S1 + CH + KL' + W') >> 32) & 7;  both are 0 on rows r = 63 mod 64.
 *   constraints  315 per proof, at index j; a prime is the value at omega x:
 *                0 .. 191   X^2 - X for helper columns 0 .. 191          192 .. 197  X^2 - X for helper columns 294 .. 299
 *              198          LIVE^2 - LIVE
 *              199 .. 204   word - sum_i 2^i bit_i for (a, A), (b, B), (c, C), (e, E), (f, F), (g, G)
 *              205 + i      U0_i - (A_(i+2) + A_(i+13) - 2 A_(i+2) A_(i+13))
 *              237 + i      U1_i - (E_(i+6) + E_(i+11) - 2 E_(i+6) E_(i+11))
 *              269 + i      V_i - A_i B_i
 *              301          S0 - sum 2^i (U0_i + A_(i+22) - 2 U0_i A_(i+22))     302   S1 - sum 2^i (U1_i + E_(i+25) - 2 U1_i E_(i+25))
 *              303          CH - sum 2^i (G_i + E_i (F_i - G_i))                 304   MAJ - sum 2^i (V_i + C_i (A_i + B_i - 2 V_i))
 *              305          KL - LIVE K(x)
 *              306 .. 311   S(x) (b' - a), (c' - b), (d' - c), (f' - e), (g' - f), (h' - g)         312   S(x) (LIVE' - LIVE)
 *              313          S(x) (a' + 2^32 (CA_0 + 2 CA_1 + 4 CA_2) - h - S1 - CH - KL' - W' - S0 - MAJ)
 *              314          S(x) (e' + 2^32 (CE_0 + 2 CE_1 + 4 CE_2) - d - h - S1 - CH - KL' - W')
 *              Every nonlinear constraint has degree 2 and no selector, every selected one is linear in the columns: the honest quotient has
 *              degree < N (measured: N - 2) and one two-column quotient oracle is enough.  Zero blocks and zero padding satisfy all 315 with
 *              LIVE = 0, which is why K enters through KL.
 *   NOT PROVED by set 3: the message schedule (W_t for t >= 16), which constraint set 4 below proves; row 0 of a block against the IV or
 *              the chaining value and the feed-forward between the two blocks of T.5 / T.6 hashes, which constraint set 5 below proves;
 *              the digest's link to Level-1, which constraint set 6 below proves; and, still open (the follow-ups): LIVE against anything
 *              public (set 6's flags); SHA-512 beyond its round function and message schedule (constraint sets 7 and 8 below).  Under set 3 ALONE a
 *              block re-run consistently from a changed W_t or a changed row-0 state goes undetected (tests/test_sha_air.py records it).
 *   challenge  a fresh duplex, as set 1: observe 2^33, then the set id 3, log_n, log_blowup, cap_height, n_proofs, then the table cap, then
 *              the helper cap (4 << min(cap_height, log_n) words each); gamma drawn as in set 1.
 *   quotient   q(x_i) = sum_p sum_(j < 315) gamma^(315 p + j) C_(p,j)(x_i) / (x_i^N - 1), planar and canonical as in set 1; pointwise: defined
 *              for any columns.
 *   identity   t^0, t^1, h^0, h^1 the table's and the helper's openings at zeta and zeta omega_N, u_0, u_1 the quotient's at zeta:
 *              sum gamma^(315 p + j) C_(p,j)(t, h; zeta) == (u_0 + X u_1) (zeta^N - 1); K(zeta) by Horner on P_K's 64 coefficients at
 *              zeta^(N/64).  A failed identity clears every query's verdict.
 *   tmx_air_sha256_helper_device        the helper (300 n_proofs columns of 2^log_rows words at d_helper) from PRE-LDE table columns
 *                                       (9 n_proofs columns at d_table).  TMX_ERR_BAD_ARG: log_rows outside 6 .. 27, n_proofs = 0,
 *                                       300 n_proofs > 2^24, a null pointer.
 *   tmx_air_sha256_quotient_device      gamma from d_cap and d_cap_helper, then the quotient of the EXTENDED columns d_cols and d_helper_cols
 *                                       into d_quot (2 << log_n words), under the context's CURRENT NTT domain.  TMX_ERR_BAD_ARG: FRI's rules
 *                                       on log_n and log_blowup, log_n - log_blowup < 6, n_proofs = 0, 300 n_proofs > 2^24, a null pointer.
 *   tmx_air_sha256_verify_device        tmx_batch_verify_device, then the identity for the oracles k_trace (the table), k_trace + 1 (the
 *                                       helper) and k_trace + 2 (the quotient).  TMX_ERR_BAD_ARG unless their column counts are 9 k, 300 k
 *                                       and 2 and their log_n equal (and the rules above).
 *   tmx_trace_commit_set_air_sha256_device   on a commit set that holds `section` (TMX_TRACE_SHA256, TMX_TRACE_TREE or TMX_TRACE_HEADER) as a
 *                                       RESIDENT member: the helper from the member's pre-LDE columns, extended under the set's domain and
 *                                       committed as a normal resident member directly behind the table (d_cap_h receives its cap), gamma, the
 *                                       quotient and its tree behind the helper (d_cap_q).  tmx_trace_commit_set_shape then reports K + 2
 *                                       oracles with TMX_TRACE_SHA256_HELPER and TMX_TRACE_SHA256_QUOTIENT in section_of.  It may be called
 *                                       for several sections of one set and beside the ladders' calls.  Refused: a streamed or absent
 *                                       section, a second call on the same section, a set that would exceed 8 oracles.  The helper is 33x
 *                                       its table and is NOT streamed: the call needs (300 n_proofs (N + M) + 2 M) 8 bytes plus two trees of
 *                                       its own, and the LDE scratch of 300 columns (TMX_ERR_CAPACITY if the card cannot hold it).
 * Every refusal comes before anything is enqueued; everything is asynchronous on hip_stream, no device-to-host copy inside, the scratch is the
 * context's own; tmx_air_last_gamma covers these calls too. */
#define TMX_AIR_SHA256_HELPER_COLS 300
#define TMX_AIR_SHA256_CONSTRAINTS 315
#define TMX_TRACE_SHA256_HELPER 128u
#define TMX_TRACE_SHA256_QUOTIENT 256u
int32_t tmx_air_sha256_helper_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, uint64_t* d_helper,
                                     void* hip_stream);
int32_t tmx_air_sha256_quotient_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                       const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                       uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha256_verify_device(tmx_ctx* ctx, const tmx_batch_params* p, uint32_t k_trace, const uint64_t* d_caps, const uint64_t* d_proof,
                                     uint32_t* d_ok, void* hip_stream);
int32_t tmx_trace_commit_set_air_sha256_device(tmx_ctx* ctx, uint32_t section, uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream);

/* ---- the message schedule of the SHA-256 tables (constraint set 4) ------------------------------------------------------------------------
 * Set 3 proves the round function row to row and leaves the W column free.  Set 4 proves the MESSAGE SCHEDULE on the same three tables:
 * W_t = sigma1(W_(t-2)) + W_(t-7) + sigma0(W_(t-15)) + W_(t-16) mod 2^32 for t = 16 .. 63 of every block.  With set 3, every live block of
 * T.3, T.5 and T.6 is then a real SHA-256 compression of its first sixteen W words from its row-0 state.  Built beside set 3 with the same
 * machinery: a helper oracle of its own, 117 constraints per proof, one two-column quotient oracle, the identity at zeta; no existing kernel,
 * transcript phase, proof word, call or refusal changes.  Notation of the block above: N rows, 9 columns per proof with W as column 0,
 * M = N B points, omega = omega_N, y = x^(N/64), a prime is the value at omega x.  Same field, extension, duplex and caveats (PARITY UNPINNED).
 *   helper     115 columns per proof, the table's rows, bits LSB first, rows taken CYCLICALLY inside one proof's 2^log_rows rows (row -1 is
 *              the last row).  Offsets inside a proof:
 *                0 .. 31   WB   bits of W (the low 32 bits of the table word, as in set 3)
 *               32 .. 63   X0   X0_i = WB_(i+7) xor WB_(i+18)  (indices mod 32)       64 .. 95   X1   X1_i = WB_(i+17) xor WB_(i+19)
 *               96  G0 = sigma0(W) = rotr7 ^ rotr18 ^ shr3     97  G1 = sigma1(W) = rotr17 ^ rotr19 ^ shr10   (words)
 *               98 .. 112  Q_1 .. Q_15   the schedule sum as a pipeline: Q_1(r) = W(r-1) + G0(r),
 *                          Q_k(r) = Q_(k-1)(r-1) + [k = 9] W(r) + [k = 14] G1(r) for k = 2 .. 15, so that
 *                          Q_15(r) = W(r-15) + sigma0(W(r-14)) + W(r-6) + sigma1(W(r-1)), the unreduced W_t for t = r + 1, always < 2^34
 *              113, 114   CW_0, CW_1   CW = (Q_15 >> 32) & 3 on the rows with r mod 64 in 15 .. 62, and 0 elsewhere
 *              Defined for ANY input; the pipeline runs across block boundaries and the wrap, which is harmless: only the last constraint is
 *              selected.
 *   constraints  117 per proof, at index j:
 *                0 .. 31    WB_i^2 - WB_i                          32, 33   CW_k^2 - CW_k               34   W - sum 2^i WB_i
 *               35 + i      X0_i - xor(WB_(i+7), WB_(i+18))        67 + i   X1_i - xor(WB_(i+17), WB_(i+19)),   xor(x, y) = x + y - 2 x y
 *               99          G0 - sum 2^i g0_i,  g0_i = xor(X0_i, WB_(i+3)) for i < 29 and X0_i for i >= 29
 *              100          G1 - sum 2^i g1_i,  g1_i = xor(X1_i, WB_(i+10)) for i < 22 and X1_i for i >= 22
 *              101          Q_1' - W - G0'
 *              100 + k      Q_k' - Q_(k-1) - [k = 9] W' - [k = 14] G1'    for k = 2 .. 15
 *              116          F(x) (W' + 2^32 (CW_0 + 2 CW_1) - Q_15)
 *              F(x) = P_F(y), P_F of degree < 64 with P_F(omega_64^t) = 1 for 15 <= t <= 62 and 0 otherwise: the NEXT row is a schedule row.
 *              Every nonlinear constraint has degree 2 and no selector; the one selected constraint is linear, its degree below 63 N / 64 + N:
 *              the honest quotient has degree < N (measured: N - 2) and one two-column quotient oracle is enough.  Zero blocks, promoted slots
 *              and zero padding satisfy all 117 without a LIVE column.
 *   NOT PROVED by sets 3 and 4: row 0 of a block against the IV or the chaining value and the feed-forward between the two blocks of
 *              T.5 / T.6 hashes, which constraint set 5 below proves; the first sixteen W of a block against Level-1, which constraint
 *              set 6 below proves; and, still open (the follow-ups): LIVE against anything public (set 6's flags); SHA-512 beyond its round function and message schedule (constraint sets 7 and 8 below).  Under sets
 *              3 and 4 ALONE a block re-run consistently (schedule
 *              and rounds) from a changed W_t, t < 16, or from a changed row-0 state goes undetected (tests/test_sha_sched.py records it).
 *   challenge  as set 3 with the set id 4: a fresh duplex observes 2^33, then 4, log_n, log_blowup, cap_height, n_proofs, then the table cap,
 *              then THIS helper's cap; gamma drawn as in set 1.
 *   quotient   q(x_i) = sum_p sum_(j < 117) gamma^(117 p + j) C_(p,j)(x_i) / (x_i^N - 1), planar and canonical; pointwise: defined for any
 *              columns.
 *   identity   sum gamma^(117 p + j) C_(p,j)(t, h; zeta) == (u_0 + X u_1) (zeta^N - 1) from the openings at zeta and zeta omega_N; F(zeta) by
 *              Horner on P_F's 64 coefficients at zeta^(N/64).  A failed identity clears every query's verdict.
 *   tmx_air_sha256_sched_helper_device     the helper (115 n_proofs columns of 2^log_rows words at d_helper) from PRE-LDE table columns
 *                                          (9 n_proofs columns at d_table).  TMX_ERR_BAD_ARG: log_rows outside 6 .. 27, n_proofs = 0,
 *                                          115 n_proofs > 2^24, a null pointer.
 *   tmx_air_sha256_sched_quotient_device   gamma from d_cap and d_cap_helper, then the quotient of the EXTENDED columns d_cols and
 *                                          d_helper_cols into d_quot (2 << log_n words), under the context's CURRENT NTT domain.  Set 3's
 *                                          rules for refusing arguments, with 115 n_proofs <= 2^24.
 *   tmx_air_sha256_sched_verify_device     tmx_batch_verify_device, then the identity for the oracles k_trace (the table), k_helper (this
 *                                          helper) and k_helper + 1 (this quotient): the helper's index is explicit because set 3's pair may
 *                                          sit between the table and this one.  TMX_ERR_BAD_ARG unless the column counts are 9 k, 115 k and 2,
 *                                          the log_n equal, k_helper > k_trace and k_helper + 1 < n_oracles.
 *   tmx_trace_commit_set_air_sha256_sched_device   mirrors tmx_trace_commit_set_air_sha256_device: the helper from the resident member's
 *                                          pre-LDE columns, extended one proof's 115 columns at a time under the set's domain and committed
 *                                          (d_cap_h), gamma, the quotient and its tree (d_cap_q), in a scratch of its own per section.  The pair
 *                                          goes behind the table, or behind set 3's helper and quotient when those already follow the table;
 *                                          set 3's call, run afterwards, inserts directly behind the table and moves this pair back by two:
 *                                          both orders end as table, H3, Q3, H4, Q4.  tmx_trace_commit_set_shape reports
 *                                          TMX_TRACE_SHA256_SCHED_HELPER and TMX_TRACE_SHA256_SCHED_QUOTIENT in section_of.  Refused: a wrong,
 *                                          absent or streamed section, a second call on the section, a set that would exceed 8 oracles.  The
 *                                          helper is NOT streamed: the call needs (115 n_proofs (N + M) + 2 M) 8 bytes plus two trees
 *                                          (TMX_ERR_CAPACITY if the card cannot hold it).
 * Every refusal comes before anything is enqueued; everything is asynchronous on hip_stream, no device-to-host copy inside;
 * tmx_air_last_gamma covers these calls too. */
#define TMX_AIR_SHA256_SCHED_HELPER_COLS 115
#define TMX_AIR_SHA256_SCHED_CONSTRAINTS 117
#define TMX_TRACE_SHA256_SCHED_HELPER 512u
#define TMX_TRACE_SHA256_SCHED_QUOTIENT 1024u
int32_t tmx_air_sha256_sched_helper_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, uint64_t* d_helper,
                                           void* hip_stream);
int32_t tmx_air_sha256_sched_quotient_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                             const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap,
                                             const uint64_t* d_cap_helper, uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha256_sched_verify_device(tmx_ctx* ctx, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, const uint64_t* d_caps,
                                           const uint64_t* d_proof, uint32_t* d_ok, void* hip_stream);
int32_t tmx_trace_commit_set_air_sha256_sched_device(tmx_ctx* ctx, uint32_t section, uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream);

/* ---- the block starts of the SHA-256 tables (constraint set 5) --------------------------------------------------------------------------
 * Sets 3 and 4 prove the round function and the message schedule: every live block is a real SHA-256 compression of its first sixteen W
 * words FROM ITS ROW-0 STATE, and row 0 itself is tied to nothing.  Set 5 proves on the same three tables that every live hash starts from
 * the SHA-256 IV, and that the second block of a two-block hash (T.5, T.6) starts from IV + (the state after round 63 of the first block).
 * Row 0 of a block is round 0 applied to the words H_0 .. H_7 the block starts from: b = H_0, c = H_1, d = H_2, f = H_4, g = H_5, h = H_6,
 * a = T1 + T2, e = H_3 + T1 with T1 = H_7 + Sigma1(H_4) + Ch(H_4, H_5, H_6) + K_0 + W_0 and T2 = Sigma0(H_0) + Maj(H_0, H_1, H_2).  Six
 * of the eight words stand in row 0 itself, so set 3's bit machinery runs on the columns b, c, d, f, g, h of the same row (the register
 * names shifted by one); H_3 and H_7 enter two sums mod 2^32 only, and the link to the row before is linear.  Built beside sets 3 and 4 with
 * the same machinery: a helper oracle of its own, 337 constraints per proof, one two-column quotient oracle, the identity at zeta; no
 * existing kernel, transcript phase, proof word, call or refusal changes.  Notation of the blocks above: N rows, 9 columns per proof (W 0,
 * a 1 .. h 8; s_j is the state column 1 + j), M = N B points, omega = omega_N, a prime is the value at omega x, rows cyclic inside a proof,
 * operands the low 32 bits of a table word; IV_0 .. IV_7 and K_0 = 0x428a2f98 the SHA-256 constants.  Same field, extension, duplex and
 * caveats (PARITY UNPINNED).
 *   chain      a mode in {0, 1}, a parameter of every call.  chain = 0: every block is a hash of its own (T.3).  chain = 1: hashes are pairs of
 *              blocks on 128-row boundaries (T.5, T.6); N >= 128.  A row r = 63 (mod 64) is a BOUNDARY row; under chain = 1 a row
 *              r = 63 (mod 128) is a CHAIN row (the next row continues a hash); every other boundary row is a START row.  The wrap from row
 *              N - 1 to row 0 is a start boundary.
 *   helper     315 columns per proof, the table's rows, bits LSB first, defined for ANY input.  Offsets inside a proof:
 *                0 .. 191   B, C, D, F, G, H   bits of b, c, d, f, g, h of the row
 *              192 .. 223   U0   U0_i = B_(i+2) xor B_(i+13)  (indices mod 32)         224 .. 255   U1   U1_i = F_(i+6) xor F_(i+11)
 *              256 .. 287   V    V_i = B_i C_i
 *              288 S0 = Sigma0(b)   289 S1 = Sigma1(f)   290 CH = Ch(f, g, h)   291 MAJ = Maj(b, c, d)   (words)
 *              292  LV   1 iff row r - r mod 64 of the proof's table has a nonzero word (set 3's LIVE rule)
 *              293 .. 300   PZ_j(r) = LV(r + 1) ((IV_j + s_j(r)) mod 2^32), on every row
 *              301 .. 308   CZ_j(r) = (IV_j + s_j(r)) >> 32, on every row
 *              309 .. 311   CA   on boundary rows the three bits of the a-sum >> 32, 0 elsewhere
 *              312 .. 314   CE   on boundary rows the three bits of the e-sum >> 32, 0 elsewhere
 *              The a-sum and the e-sum are those of constraints 327 / 328 on a start row and of 335 / 336 on a chain row: seven terms below
 *              2^32 (carry <= 6) and six (carry <= 5).
 *   constraints  337 per proof, at index j:
 *                0 .. 191   X^2 - X for the helper columns 0 .. 191     192 .. 199   for CZ     200 .. 205   for CA, CE     206   LV^2 - LV
 *              207 .. 212   word - sum 2^i bit_i   for (b, B), (c, C), (d, D), (f, F), (g, G), (h, H)
 *              213 + i      U0_i - xor(B_(i+2), B_(i+13))     245 + i   U1_i - xor(F_(i+6), F_(i+11))     277 + i   V_i - B_i C_i
 *              309   S0 - sum 2^i xor(U0_i, B_(i+22))         310   S1 - sum 2^i xor(U1_i, F_(i+25)),   xor(x, y) = x + y - 2 x y
 *              311   CH - sum 2^i (H_i + F_i (G_i - H_i))     312   MAJ - sum 2^i (V_i + D_i (B_i + C_i - 2 V_i))
 *              313 + j, j < 8   PZ_j - LV' (IV_j + s_j - 2^32 CZ_j)      degree 2, no selector: it holds on every row by construction
 *              321 .. 326   E_s:  x' - IV_j LV'   for (x, j) = (b, 0), (c, 1), (d, 2), (f, 4), (g, 5), (h, 6)
 *              327          E_s:  a' + 2^32 (CA_0 + 2 CA_1 + 4 CA_2) - (IV_7 + K_0) LV' - S1' - CH' - W' - S0' - MAJ'
 *              328          E_s:  e' + 2^32 (CE_0 + 2 CE_1 + 4 CE_2) - (IV_3 + IV_7 + K_0) LV' - S1' - CH' - W'
 *              329 .. 334   E_c:  x' - PZ_j       for the same six pairs
 *              335          E_c:  a' + 2^32 CA - PZ_7 - K_0 LV' - S1' - CH' - W' - S0' - MAJ'
 *              336          E_c:  e' + 2^32 CE - PZ_3 - PZ_7 - K_0 LV' - S1' - CH' - W'
 *              Selectors, with y = x^(N/64), z = x^(N/128), rho = omega_128^-1: chain = 0: E_s = (x^N - 1) / (y - omega_64^-1), E_c = 0;
 *              chain = 1: E_s = (x^N - 1) / (z - rho), nonzero exactly on r = 127 (mod 128), and E_c = (x^N - 1) / (z + rho), nonzero exactly
 *              on r = 63 (mod 128) (omega_128^64 = -1).  Every nonlinear constraint has degree 2 and no selector, every selected one is
 *              linear in the columns: the honest quotient has degree < N and one two-column quotient oracle is enough.  Zero blocks,
 *              promoted slots, unused second blocks and zero padding satisfy all 337 with LV = 0, which is why K_0 and the IV enter
 *              multiplied by LV' and why PZ carries LV'.
 *   NOT PROVED by sets 3 + 4 + 5 (the follow-ups): the first sixteen W of a block against Level-1; the digest (IV or chaining value plus
 *              the state after the last round) against Level-1; LV against anything public -- a hash whose live second block is replaced
 *              by a zero block goes unseen, because the set cannot know that a second block was due; SHA-512 beyond its round function and message schedule (constraint sets 7 and 8 below); the ladders' curve arithmetic
 *              and limb ranges (tests/test_sha_init.py records the first and the third).  Constraint set 6 below ("the SHA-256 tables'
 *              link to Level-1") closes the first three: it pins the first sixteen W, the digest and the block structure to Level-1.
 *   challenge  set 3's lone-lane kernel: a fresh duplex observes 2^33, then 5 | chain << 8, log_n, log_blowup, cap_height, n_proofs, then the
 *              table cap, then THIS helper's cap; gamma drawn as in set 1.
 *   quotient   with D_s and D_c the selectors' denominators (y - omega_64^-1 under chain = 0; z - rho and z + rho under chain = 1),
 *              q(x_i) = sum_p [ sum_(j < 321) gamma^(337 p + j) C_j / (x_i^N - 1) + sum_(321 <= j < 329) gamma^(337 p + j) L_j / D_s
 *                               + sum_(j >= 329) gamma^(337 p + j) L_j / D_c ],   L_j the linear forms behind E_s and E_c above (the last
 *              sum is absent under chain = 0); planar and canonical; pointwise: defined for any columns.
 *   identity   division-free, from the openings at zeta and zeta omega_N.  chain = 1, with S = D_s D_c at zeta:
 *              S sum_unselected + (zeta^N - 1) (D_c sum_start + D_s sum_chain) == (u_0 + X u_1) (zeta^N - 1) S;   chain = 0, with S = D_s:
 *              S sum_unselected + (zeta^N - 1) sum_start == (u_0 + X u_1) (zeta^N - 1) S.  A failed identity clears every query's verdict.
 *   tmx_air_sha256_init_helper_device      the helper (315 n_proofs columns of 2^log_rows words at d_helper) from PRE-LDE table columns
 *                                          (9 n_proofs columns at d_table).  TMX_ERR_BAD_ARG: log_rows outside 6 .. 27, n_proofs = 0,
 *                                          315 n_proofs > 2^24, chain > 1, chain = 1 with log_rows < 7, a null pointer.
 *   tmx_air_sha256_init_quotient_device    gamma from d_cap and d_cap_helper, then the quotient of the EXTENDED columns d_cols and
 *                                          d_helper_cols into d_quot (2 << log_n words), under the context's CURRENT NTT domain.  Set 4's
 *                                          rules for refusing arguments, with 315 n_proofs <= 2^24; chain > 1 and chain = 1 with fewer than
 *                                          128 rows are refused.
 *   tmx_air_sha256_init_verify_device      tmx_batch_verify_device, then the identity for the oracles k_trace (the table), k_helper (this
 *                                          helper) and k_helper + 1 (this quotient).  TMX_ERR_BAD_ARG unless the column counts are 9 k, 315 k
 *                                          and 2, the log_n equal, k_helper > k_trace, k_helper + 1 < n_oracles, and chain as above.
 *   tmx_trace_commit_set_air_sha256_init_device   mirrors tmx_trace_commit_set_air_sha256_sched_device: the helper from the resident member's
 *                                          pre-LDE columns, extended one proof's 315 columns at a time under the set's domain and committed
 *                                          (d_cap_h), gamma, the quotient and its tree (d_cap_q), in a scratch of its own per section; chain
 *                                          is 0 for TMX_TRACE_SHA256 and 1 for TMX_TRACE_TREE and TMX_TRACE_HEADER.  The pair goes behind the
 *                                          last helper/quotient pair that already follows the table; set 3's and set 4's calls, unchanged,
 *                                          insert in front of later members: every order of the three calls ends as table, H3, Q3, H4, Q4,
 *                                          H5, Q5.  tmx_trace_commit_set_shape reports TMX_TRACE_SHA256_INIT_HELPER and
 *                                          TMX_TRACE_SHA256_INIT_QUOTIENT in section_of.  Refused: a wrong, absent or streamed section, a
 *                                          second call on the section, a set that would exceed 8 oracles.  The helper is NOT streamed: the
 *                                          call needs (315 n_proofs (N + M) + 2 M) 8 bytes plus two trees (TMX_ERR_CAPACITY if the card
 *                                          cannot hold it); at 256 proofs and blow-up 8 that is 23.8 GB for HEADER (N = 2^12), 95.1 GB for
 *                                          T.3 (N = 2^14) and 190 GB for TREE (N = 2^15): as with set 3, only HEADER is meant to run
 *                                          resident at full size.
 * Every refusal comes before anything is enqueued; everything is asynchronous on hip_stream, no device-to-host copy inside;
 * tmx_air_last_gamma covers these calls too. */
#define TMX_AIR_SHA256_INIT_HELPER_COLS 315
#define TMX_AIR_SHA256_INIT_CONSTRAINTS 337
#define TMX_TRACE_SHA256_INIT_HELPER 2048u
#define TMX_TRACE_SHA256_INIT_QUOTIENT 4096u
int32_t tmx_air_sha256_init_helper_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t n_proofs, uint32_t chain, const uint64_t* d_table,
                                          uint64_t* d_helper, void* hip_stream);
int32_t tmx_air_sha256_init_quotient_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs, uint32_t chain,
                                            const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap,
                                            const uint64_t* d_cap_helper, uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha256_init_verify_device(tmx_ctx* ctx, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, uint32_t chain,
                                          const uint64_t* d_caps, const uint64_t* d_proof, uint32_t* d_ok, void* hip_stream);
int32_t tmx_trace_commit_set_air_sha256_init_device(tmx_ctx* ctx, uint32_t section, uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream);

/* ---- streamed helpers of the SHA-256 sets: constraint sets 3, 4 and 5 on full-size tables ----
 * The helper oracle of a set is 300, 115 or 315 columns per proof, 13 to 35 times its table; kept extended it is what bounds the size the
 * set-level calls above can run at.  Here the helper is fed in chunks of whole proofs and never exists extended; the table member stays
 * resident, and so do the helper's PRE-LDE columns (the prove's openings at zeta read them).  Field arithmetic is exact, so the pieces in
 * any order give the resident call's words: for every valid chunk size d_cap_h, d_cap_q, tmx_air_last_gamma,
 * tmx_trace_commit_set_shape and every word of tmx_trace_commit_set_prove_device's proof equal the resident call's.  Resident and
 * streamed pairs may be mixed within a set and within a section; the verifiers need nothing.
 *   tmx_air_sha256_quotient_range_device, _sched_quotient_range_device, _init_quotient_range_device
 *                                          the quotient calls over the proofs [proof_lo, proof_hi) of the table only, as
 *                                          tmx_air_ladder_quotient_range_device: d_cols is still the whole table's column 0, but
 *                                          d_helper_cols is the FIRST HELPER COLUMN OF PROOF proof_lo -- a buffer that holds the piece's
 *                                          columns alone will do.  gamma is drawn over n_proofs; the piece's sum is weighted with
 *                                          gamma^(C proof_lo), C = 315, 117 or 337, divided as the whole call divides, and written
 *                                          (accumulate = 0) or added to what d_quot holds and written canonical (accumulate = 1).  Pieces
 *                                          that cover [0, n_proofs) once, in any order, the first with accumulate = 0, leave the whole
 *                                          call's words.  TMX_ERR_BAD_ARG: an empty range, proof_hi > n_proofs, accumulate > 1, and the
 *                                          whole call's rules.
 *   tmx_trace_commit_set_air_sha256_streamed_bytes   host only: the bytes the call below allocates for its [set][section] scratch -- pre-LDE
 *                                          helper | helper levels | quotient | quotient levels | sponge states [12][M] | chunk
 *                                          [chunk_proofs helper_cols][M] -- and, in *lde_scratch_bytes (may be null), the LDE's own scratch:
 *                                          twice what is extended at once, which is one chunk (ONE transform call per chunk, as the prove's
 *                                          gather extends a streamed member; per-proof calls would need 1 / chunk_proofs of it but the
 *                                          prove grows it to the chunk regardless).  With chunk_proofs >= n_proofs: the resident call's
 *                                          (helper_cols n_proofs (N + M) + 2 M) 8 bytes plus two trees, and twice one proof's helper columns.
 *                                          0 on a refused shape: constraint_set outside 3 .. 5, chunk_proofs = 0, chunk_proofs helper_cols
 *                                          no multiple of 8 (the sponge absorbs eight columns at a time: chunk_proofs even for set 3, a
 *                                          multiple of 8 for sets 4 and 5), log_blowup outside 1 .. 6, fewer than 64 rows, n_proofs = 0,
 *                                          helper_cols n_proofs > 2^24.
 *   tmx_trace_commit_set_air_sha256_streamed_device   the set-level call of constraint_set 3, 4 or 5 on `section`.  chunk_proofs >=
 *                                          n_proofs takes the resident path exactly.  Else: the helper kernel into the pre-LDE columns;
 *                                          sweep 1, per chunk the LDE into the chunk buffer and k_poseidon_leaves_chunk, then the levels and
 *                                          d_cap_h; gamma; sweep 2, per chunk the LDE again and the accumulating piece of the quotient; the
 *                                          quotient's tree and d_cap_q.  Both sweeps run under the set's NTT domain: if
 *                                          tmx_ntt_set_domain moved the context's it is put back for the call and restored after.  The pair
 *                                          is registered by the resident calls' rules (same place by set id, same refusals); a streamed
 *                                          scratch is sized exactly (a larger one left by a resident call on that set and section is
 *                                          released).  TMX_ERR_BAD_ARG: no set, constraint_set outside 3 .. 5, a wrong, absent or streamed
 *                                          section (the TABLE member must be resident), null caps, a chunk_proofs _bytes refuses, a second
 *                                          call on the section in either form, a full set.  TMX_ERR_CAPACITY against free memory, the
 *                                          LDE's scratch included.  At 256 proofs, blow-up 8 and chunk_proofs = 8 the three pairs of TREE
 *                                          (N = 2^15) need about 49 GB of helper columns where the resident calls need about 441 GB.
 * Every refusal comes before anything is enqueued; everything is asynchronous on hip_stream apart from a domain change. */
int32_t tmx_air_sha256_quotient_range_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                             uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                             const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper, uint64_t* d_quot,
                                             void* hip_stream);
int32_t tmx_air_sha256_sched_quotient_range_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                   uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                   const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                                   uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha256_init_quotient_range_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                  uint32_t chain, uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                  const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                                  uint64_t* d_quot, void* hip_stream);
uint64_t tmx_trace_commit_set_air_sha256_streamed_bytes(uint32_t constraint_set, uint32_t log_m, uint32_t log_blowup, uint32_t cap_height,
                                                        uint32_t n_proofs, uint32_t chunk_proofs, uint64_t* lde_scratch_bytes);
int32_t tmx_trace_commit_set_air_sha256_streamed_device(tmx_ctx* ctx, uint32_t constraint_set, uint32_t section, uint32_t chunk_proofs,
                                                        uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream);
/* Host only, for tests and memory accounting: the bytes of the [set][section] scratch the context holds right now, as the last resident or
 * streamed set-level call of constraint_set on `section` left it (a streamed call leaves exactly what _streamed_bytes returns); 0 if there
 * is none, for a constraint_set outside 3 .. 5 and for a section that is no SHA-256 table. */
uint64_t tmx_trace_commit_set_air_sha256_scratch_bytes(const tmx_ctx* ctx, uint32_t constraint_set, uint32_t section);

/* ---- the SHA-256 tables' link to Level-1 (constraint set 6) -------------------------------------------------------------------------------
 * Sets 3 + 4 + 5 prove that every live block of T.3, T.5 and T.6 is a real SHA-256 compression of its first sixteen W words and that every
 * hash starts from the IV and chains correctly.  Nothing there says WHICH message was hashed or that the result is the digest the product
 * returns.  Set 6 is set 2's sibling for the three SHA-256 tables: a public table gathered from the Level-1 ELEMENT rows, to which the
 * first sixteen W of every block, the digest of every hash and the block structure are pinned.  Built beside what exists: no existing
 * kernel, transcript, proof word, call or refusal changes.  Notation of the blocks above: N rows, K = N / 64 blocks per proof (padding
 * included), 2 <= K <= 2^12; columns W 0, a 1 .. h 8, s_j the state column 1 + j; rows and blocks cyclic inside a proof; operands the low
 * 32 bits of a table word; IV_0 .. IV_7 the SHA-256 constants.  There is NO chain parameter: the public flags carry the block structure.
 *   pub        the public table: 26 columns per proof, K rows (one per block of the table, in the table's order), column-major, canonical
 *              words below 2^32.  Inside a proof's 26:
 *                 0 .. 15   w[k][t]     the sixteen message words of block k, SHA padding included; zero for a dead block
 *                16 .. 23   dig[k][j]   word j of the digest, big-endian words as SHA-256 emits them, set only where block k is the LAST
 *                                       LIVE block of its hash, else zero
 *                24         new[k]      1 iff block k is live and starts a hash
 *                25         chn[k]      1 iff block k is live and continues the hash of block k - 1
 *              What the gather reads per section (docs/witness_layout.md; bytes are eight big-endian bit elements, packed by the kernel):
 *                T.3   message 00 | marshalled[0 .. validator_byte_length) of the lane (D.1a / D.2a; the length from H, clamped to 46 as
 *                      the product clamps it); digest: the lane's leaf hash (D.1a / D.2a).  One block per hash.
 *                T.5   message 01 | L | R over the slot's two children as Level-1 holds them (the leaf hashes below the first level,
 *                      D.3 / D.4 above); a promoted slot is all zero with its flags clear; digest: the slot's node (D.3 / D.4).  Two blocks.
 *                      Level-1 holds `both children enabled ? hash : L` in a node, and the rows hash every pair: on a slot whose right
 *                      child is NOT enabled the node is L, not the hash of the rows, and the link does not hold there -- the set is
 *                      for batches whose trees are full (nb >= N), as every committed workload is.
 *                T.6   the leaf block 00 | leaf as the proof struct in H carries it (the chain id's 52 bytes under its encoded length, the
 *                      height's leaf 00 08 varint9 from D.5 under its encoded length, the 34- or 72-byte leaves; lengths clamped to 79), then
 *                      the four path nodes 01 | left | right from the aunts in H and the previous node in D.5, path bits LSB-first;
 *                      digests: D.5.  Two blocks per hash, the second unused (zero, flags clear) but for the 72-byte leaf and the path nodes.
 *              The block order, the liveness rules and the one-block / two-block shapes are those of docs/level2_rows.md.
 *   helper     33 columns per proof on the table's rows, defined for ANY input; a flag of pub is SET when its low 32 bits are not zero, new
 *              before chn.  For a row r in block k, offsets inside a proof:
 *                 0 ..  7   CV_j    IV_j if new[k]; (IV_j + s_j(row 63 of block k - 1)) mod 2^32 if chn[k]; else 0.  Constant in a block.
 *                 8 .. 15   DG_j    (CV_j + s_j(r)) mod 2^32, on every row          16 .. 23   CD_j   that sum's carry bit
 *                24 .. 31   CH_j    CHN DG_j                                       32         CHN    1 iff chn[(k + 1) mod K] is set
 *   constraints  50 per proof, weights gamma^(50 p + j), with S = x^K - omega_64^-1, zero exactly on rows r = 63 (mod 64), T = (x^N - 1) / S,
 *              D_t = x^K - omega_64^t, zero exactly on rows r = t (mod 64), T_t = (x^N - 1) / D_t; a prime is the value at omega x:
 *                 0 ..  7   CD_j^2 - CD_j                    8 .. 15   DG_j + 2^32 CD_j - CV_j - s_j        16 .. 23   CH_j - CHN DG_j
 *                24 .. 31   S (CV_j' - CV_j)                32 .. 39   T (CV_j' - CH_j - IV_j NEW)          40 .. 47   T (DG_j - CH_j - DIG_j)
 *                48         T (CHN - CHNP)                  49         sum_(t < 16) T_t (W - E_t)
 *              NEW, DIG_j, CHNP and E_t the public polynomials of degree < K with NEW(omega^(64 k + 63)) = new[(k + 1) mod K],
 *              CHNP(omega^(64 k + 63)) = chn[(k + 1) mod K], DIG_j(omega^(64 k + 63)) = dig[k][j], E_t(omega^(64 k + t)) = w[k][t].
 *              Constraint 49 has ONE weight for its sixteen parts: the T_t vanish on disjoint classes of rows, so the sum is zero on the
 *              domain exactly when each part is.  Every nonlinear constraint has degree 2 and no selector, every selected one is linear
 *              in the columns: the honest quotient has degree < N and one two-column quotient oracle is enough.  Dead blocks, promoted
 *              slots, unused second blocks and zero padding satisfy all 50 with their flags clear.
 *   public side  collapses under gamma as in set 2, to seventeen F_p^2 polynomials of degree < K: P63 through
 *              V63_k = sum_p [sum_j gamma^(50 p + 32 + j) IV_j new_p[(k + 1) % K] + sum_j gamma^(50 p + 40 + j) dig_p[k][j]
 *                             + gamma^(50 p + 48) chn_p[(k + 1) % K]]   on the coset omega^(64 k + 63),
 *              and P_t, t < 16, through V^t_k = sum_p gamma^(50 p + 49) w_p[k][t] on the coset omega^(64 k + t).  The prover extends each
 *              (set 2's coefficient and extension kernels with the coset's offset) and folds them into one plane
 *              PQ(x_i) = P63(x_i) / S(x_i) + sum_t P_t(x_i) / D_t(x_i); the 1 / S and 1 / D_t tables have period 64 B.
 *   challenge  a lone-lane kernel with its own duplex, set 3's form with the set id 6: it observes 2^33, then 6, log_n, log_blowup,
 *              cap_height, n_proofs, then the table cap, then THIS helper's cap, then the four words of the PUBLIC DIGEST -- the Poseidon
 *              Merkle root, cap height 0, of pub taken as a column-major oracle of log2 K rows and 26 n_proofs columns (set 2's rule);
 *              gamma drawn as in set 1.
 *   quotient   q(x_i) = [sum_p sum_(j < 32) gamma^(50 p + j) C_(p,j)] / (x_i^N - 1)
 *                     + [sum_p sum_(j = 32 .. 48) gamma^(50 p + j) (the constraint's column part: CV_j' - CH_j, DG_j - CH_j, CHN)] / S(x_i)
 *                     + [sum_p gamma^(50 p + 49) W_p] sum_t 1 / D_t(x_i)  -  PQ(x_i);
 *              constraints 24 .. 31 carry the factor S(x_i); planar and canonical; pointwise: defined for any columns and any pub.
 *   identity   from the openings at zeta and zeta omega_N, with Z = zeta^N - 1 and the three gamma sums a (j < 32), b (32 .. 48), c (49):
 *              a + Z (b / S(zeta) + c sum_t 1 / D_t(zeta) - PQ(zeta)) == (u_0 + X u_1) Z.  The verifier hashes d_pub itself, forms its
 *              own V63 and V^t, and evaluates the seventeen polynomials barycentrically, set 2's form with K <= 2^12 per coset:
 *              P_c(zeta) / D_c(zeta) = 1 / (K y_0^K) sum_k V_k y_k / (zeta - y_k).  A failed identity, or a zero denominator, clears
 *              every query's verdict.
 *   NOT PROVED by sets 3 + 4 + 5 + 6: LIVE / LV of sets 3 and 5 against set 6's public flags; SHA-512 beyond its round function and message schedule (constraint sets 7 and 8 below); the ladders' curve arithmetic and
 *              limb ranges; a T.5 slot whose right child is not enabled (above); and there is no range argument for DG on chain rows --
 *              the identities are integer identities far below p and the digest is pinned to a public word below 2^32, so the digest is
 *              right mod 2^32 provided set 3 range-checks s_j.  TMX_BATCH_MAX_ORACLES stays 8: a section that already carries sets 3 + 4 + 5 has seven oracles
 *              and refuses set 6's pair by the existing rule (no room for two more oracles); widening the cap changes an ABI struct
 *              and is the next follow-up, as is a streamed form of this helper.
 *   tmx_air_sha256_public_shape          host only: log2 K and the column count 26 n_proofs of pub for (kind, section, n_max, n_proofs);
 *                                        either pointer may be null.  TMX_ERR_BAD_ARG: a section other than TMX_TRACE_SHA256, _TREE,
 *                                        _HEADER, a table the kind and n_max do not have, K outside 2 .. 2^12, n_proofs = 0,
 *                                        33 n_proofs > 2^24.
 *   tmx_air_sha256_public_device         gathers pub (26 n_proofs columns of K words at d_pub) from the element rows at d_elems as
 *                                        tmx_witness_batch_device leaves them (rows tmx_elem_stride apart, the context's n_max).  One lane
 *                                        per (proof, block).  It reads neither the trace rows nor the context's Level-1 scratch.  The
 *                                        shape call's refusals, a bad kind, a null pointer.
 *   tmx_air_sha256_link_helper_device    the helper (33 n_proofs columns of 2^log_rows words at d_helper) from PRE-LDE table columns
 *                                        (9 n_proofs columns at d_table) and pub's flags (26 n_proofs columns of 2^(log_rows - 6) words at
 *                                        d_pub).  TMX_ERR_BAD_ARG: log_rows outside 7 .. 18, n_proofs = 0, 33 n_proofs > 2^24, a null
 *                                        pointer.
 *   tmx_air_sha256_link_quotient_device  the public digest and gamma from d_cap, d_cap_helper and d_pub, the public side, then the
 *                                        quotient of the EXTENDED columns d_cols (9 n_proofs) and d_helper_cols (33 n_proofs) into d_quot
 *                                        (2 << log_n words), under the context's CURRENT NTT domain (root and shift: its own twiddle
 *                                        kernels, not the NTT's tables).  TMX_ERR_BAD_ARG: log_blowup outside 1 .. 6, log_n > 28,
 *                                        log_n - log_blowup outside 7 .. 18 (2 <= K <= 2^12: set 2's rule), n_proofs = 0,
 *                                        33 n_proofs > 2^24, a coset on which x^N - 1 vanishes, a null pointer.
 *   tmx_air_sha256_link_quotient_range_device   the same over the proofs [proof_lo, proof_hi) only, as the range calls of sets 3 - 5:
 *                                        d_cols the whole table's column 0, d_helper_cols the FIRST HELPER COLUMN OF PROOF proof_lo, gamma
 *                                        over n_proofs, the piece weighted with gamma^(50 proof_lo), written (accumulate = 0) or added
 *                                        (accumulate = 1).  The piece with proof_lo = 0 carries - PQ.  Pieces that cover [0, n_proofs)
 *                                        once, in any order, the first with accumulate = 0, leave the whole call's words.  An empty
 *                                        range, proof_hi > n_proofs and accumulate > 1 are refused.
 *   tmx_air_sha256_link_verify_device    tmx_batch_verify_device, then the identity for the oracles k_trace (the table), k_helper (this
 *                                        helper) and k_helper + 1 (this quotient) against d_pub.  TMX_ERR_BAD_ARG unless the column
 *                                        counts are 9 k, 33 k and 2, the log_n equal, k_helper > k_trace, k_helper + 1 < n_oracles, the
 *                                        quotient call's rules hold and d_pub is set.
 *   tmx_trace_commit_set_air_sha256_link_device   mirrors tmx_trace_commit_set_air_sha256_init_device on a RESIDENT member `section`: the
 *                                        helper from the member's pre-LDE columns and d_pub (26 n_proofs columns of K words, as the gather
 *                                        leaves it), extended one proof's 33 columns at a time under the set's domain and committed
 *                                        (d_cap_h); gamma over the table cap, that cap and d_pub's digest; the public side from the SET's
 *                                        root and shift; the quotient and its tree (d_cap_q).  The pair goes behind the last
 *                                        helper/quotient pair that already follows the table; the calls of sets 3 - 5, unchanged, insert in
 *                                        front of it: every order ends as table, H3, Q3, H4, Q4, H5, Q5, H6, Q6 with the same caps and the
 *                                        same proof.  tmx_trace_commit_set_shape reports TMX_TRACE_SHA256_LINK_HELPER and
 *                                        TMX_TRACE_SHA256_LINK_QUOTIENT in section_of.  A scratch of its own per section,
 *                                        (33 n_proofs (N + M) + 2 M) 8 bytes plus two trees, and 4 M words (one extended public
 *                                        polynomial and PQ) in the context's set-6 scratch: 19.9 GB for TREE at 256 proofs and blow-up 8
 *                                        (TMX_ERR_CAPACITY if the card cannot hold it).  TMX_ERR_BAD_ARG: no set, a section that is no
 *                                        SHA-256 table, an absent or streamed section, a second call on the section, a set with no room for
 *                                        two more oracles, K outside 2 .. 2^12, a null pointer.
 * Every refusal comes before anything is enqueued; everything is asynchronous on hip_stream, no device-to-host copy inside -- but a scratch
 * that has to grow is released and allocated anew, which waits for the device (hipDeviceSynchronize for the context's set-6 scratch,
 * as the other sets' scratches do): a caller that must not stall makes one warm call at its largest shape.  Every range piece hashes
 * d_pub and draws gamma again (only the piece with proof_lo = 0 builds the public side): repeated launch-sized work that a streamed
 * form of the helper would hoist.  tmx_air_last_gamma covers the quotient calls and the set-level call too. */
#define TMX_TRACE_SHA256_LINK_HELPER 8192u
#define TMX_TRACE_SHA256_LINK_QUOTIENT 16384u
#define TMX_AIR_SHA256_PUBLIC_WIDTH 26
#define TMX_AIR_SHA256_LINK_HELPER_COLS 33
#define TMX_AIR_SHA256_LINK_CONSTRAINTS 50
int32_t tmx_air_sha256_public_shape(int32_t kind, uint32_t section, uint32_t n_max, uint32_t n_proofs, uint32_t* log_k, uint32_t* n_cols);
int32_t tmx_air_sha256_public_device(tmx_ctx* ctx, int32_t kind, uint32_t section, uint32_t n_proofs, const void* d_elems, uint64_t* d_pub,
                                     void* hip_stream);
int32_t tmx_air_sha256_link_helper_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, const uint64_t* d_pub,
                                          uint64_t* d_helper, void* hip_stream);
int32_t tmx_air_sha256_link_quotient_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                            const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap,
                                            const uint64_t* d_cap_helper, const uint64_t* d_pub, uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha256_link_quotient_range_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                  uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                  const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                                  const uint64_t* d_pub, uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha256_link_verify_device(tmx_ctx* ctx, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, const uint64_t* d_caps,
                                          const uint64_t* d_proof, const uint64_t* d_pub, uint32_t* d_ok, void* hip_stream);
int32_t tmx_trace_commit_set_air_sha256_link_device(tmx_ctx* ctx, uint32_t section, const uint64_t* d_pub, uint64_t* d_cap_h, uint64_t* d_cap_q,
                                                    void* hip_stream);

/* ---- the round constraints of the SHA-512 table (constraint set 7) ----------------------------------------------------------------------
 * Sets 3 - 6 argue about the three SHA-256 tables.  The fifth committed row table, T.2 (TMX_TRACE_SHA512), holds the SHA-512 rows of every
 * lane's SHA-512(R || A || M), the hash that yields the scalar h of h A.  Set 7 proves the SHA-512 ROUND FUNCTION on it: the sibling of
 * set 3, with the same machinery -- a helper oracle behind the table, one two-column quotient oracle behind the helper, the identity at
 * zeta -- and no change to any existing kernel, transcript phase, proof word, call, refusal or scratch; the batch prover, its proof format
 * and tmx_batch_verify_device are used UNCHANGED.  Same field, extension, duplex and caveats as the blocks above (PARITY UNPINNED).
 *   table      18 n_proofs columns of 32-bit limbs; inside a proof W lo 0, W hi 1, a lo 2, a hi 3, ... h lo 16, h hi 17; row
 *              (2 i + b) 80 + t holds W_t and the state after round t of block b of lane i (docs/level2_rows.md).  Of the N = 2^log_rows
 *              rows the first 160 lanes are live or zero, the rest zero padding; N is never a multiple of 80.
 *   preprocessed columns  A block is 80 rows, and no power-of-two subgroup has a coset structure of period 80: a selector x^(N/80) - c
 *              does not exist.  Three PUBLIC columns that depend on N alone take its place, each a polynomial of degree <= N - 1:
 *                SEL_r = 1, but 0 where r mod 80 = 79 and at r = N - 1 (the wrap row must be off: (N - 1) mod 80 != 79)
 *                KLO_r, KHI_r = the low and the high 32 bits of K512[r mod 80], on every row r < N
 *              The prover fills them (k_air_sha512_periodic<Sha512Round>) and extends them exactly as helper columns are extended.  The verifier
 *              commits to nothing: it computes SEL(zeta), KLO(zeta), KHI(zeta) itself, barycentrically over the N rows,
 *                P(zeta) = (zeta^N - 1) / N  sum_r v_r omega^r / (zeta - omega^r)
 *              in a multi-workgroup kernel (k_air_sha512_periodic_eval<Sha512Round>, one batched inversion per four rows of a thread).  A zero
 *              denominator clears every verdict.  This O(N) work bounds the rows set 7 accepts to log_rows 7 .. 18 (the full size is 15).
 *   helper     599 columns per proof, the table's rows, bits LSB first, bit 32 limb + i in limb `limb`, bit indices mod 64:
 *                0 .. 63  A      128 .. 191  C      256 .. 319  F      384 .. 447  U0_i = A_(i+28) xor A_(i+34)     512 .. 575  V_i = A_i B_i
 *               64 .. 127 B      192 .. 255  E      320 .. 383  G      448 .. 511  U1_i = E_(i+14) xor E_(i+18)
 *               576 / 577 Sigma0 lo / hi   578 / 579 Sigma1   580 / 581 Ch   582 / 583 Maj   584 LIVE   585 / 586 KL = LIVE K512[r mod 80]
 *               587 .. 589 CAL   590 .. 592 CAH  (carry bits of the a update, low and high limb)   593 .. 595 CEL   596 .. 598 CEH  (e update)
 *              LIVE = 1 iff row r - r mod 80 of the proof's table has a word whose low 32 bits are not zero.  Defined for ANY input: the
 *              operands are the low 32 bits of each table word; carries are 0 where SEL = 0; elsewhere, primes from row r + 1,
 *              CAL = ((h + Sigma1 + Ch + KL' + W' + Sigma0 + Maj)_lo >> 32) & 7, CAH the same over the high limbs plus the value of CAL;
 *              CEL, CEH the same over d + h + Sigma1 + Ch + KL' + W'.  Seven summands: the a carries are <= 6; six: the e carries <= 5; every
 *              identity is an integer identity below 2^35.
 *   constraints  628 per proof, at index j; a prime is the value at omega x:
 *                0 .. 383   X^2 - X for helper columns 0 .. 383          384 .. 395  X^2 - X for helper columns 587 .. 598
 *              396          LIVE^2 - LIVE
 *              397 .. 408   limb - sum_(i < 32) 2^i bit_(32 limb + i) for (a, A) lo, hi, then b, c, e, f, g
 *              409 + i      U0_i - (A_(i+28) + A_(i+34) - 2 A_(i+28) A_(i+34))       473 + i   U1_i - (E_(i+14) + E_(i+18) - 2 E_(i+14) E_(i+18))
 *              537 + i      V_i - A_i B_i
 *              601 .. 608   Sigma0, Sigma1, Ch, Maj, lo then hi each, against sum 2^i of U0_j + A_(j+39) - 2 U0_j A_(j+39),
 *                           U1_j + E_(j+41) - 2 U1_j E_(j+41), G_j + E_j (F_j - G_j), V_j + C_j (A_j + B_j - 2 V_j), j = 32 limb + i
 *              609, 610     KL_lo - LIVE KLO(x), KL_hi - LIVE KHI(x)
 *              611 .. 622   SEL(x) (b' - a), (c' - b), (d' - c), (f' - e), (g' - f), (h' - g), lo then hi each      623   SEL(x) (LIVE' - LIVE)
 *              624          SEL(x) (a'_lo + 2^32 (CAL_0 + 2 CAL_1 + 4 CAL_2) - h_lo - Sigma1_lo - Ch_lo - KL'_lo - W'_lo - Sigma0_lo - Maj_lo)
 *              625          the same over the high limbs with CAH, minus (CAL_0 + 2 CAL_1 + 4 CAL_2)
 *              626, 627     the e update: d + h + Sigma1 + Ch + KL' + W', with CEL / CEH
 *              Every nonlinear constraint has degree 2 in the columns and no selector, every selected one is SEL (linear), the K constraint
 *              KL - LIVE K(x): every constraint has degree <= 2 N - 2, the honest quotient degree <= N - 2, and ONE two-column quotient
 *              oracle still suffices.  Zero blocks and zero padding satisfy all 628 with LIVE = 0.
 *   NOT PROVED by set 7: the message schedule (W_t for t >= 16) and W's limb range -- both are constraint set 8 below --; the IV and the
 *              feed-forward of the two blocks -- constraint set 9 below --; the link of message and digest to Level-1, and so of h; LIVE
 *              against anything public.
 *              Under set 7 ALONE a block re-run consistently from a changed W_t goes undetected (tests/test_sha512_air.py records it;
 *              set 8 rejects it, tests/test_sha512_sched.py).
 *   challenge  a fresh duplex, as set 3: observe 2^33, then the set id 7, log_n, log_blowup, cap_height, n_proofs, then the table cap, then
 *              the helper cap.  The preprocessed columns are a function of log_n - log_blowup and are not observed.
 *   quotient   q(x_i) = sum_p sum_(j < 628) gamma^(628 p + j) C_(p,j)(x_i) / (x_i^N - 1), planar and canonical as in set 1; pointwise.
 *   identity   as set 3's, with SEL(zeta), KLO(zeta), KHI(zeta) from the barycentric kernel.  A failed identity clears every verdict.
 *   tmx_air_sha512_helper_device        the helper (599 n_proofs columns at d_helper) from PRE-LDE table columns (18 n_proofs at d_table).
 *                                       TMX_ERR_BAD_ARG: log_rows outside 7 .. 18, n_proofs = 0, 599 n_proofs > 2^24, a null pointer.
 *   tmx_air_sha512_quotient_device      fills and extends the preprocessed columns under the context's CURRENT NTT domain, draws gamma from
 *                                       d_cap and d_cap_helper, then the quotient of the EXTENDED columns into d_quot (2 << log_n words).
 *                                       TMX_ERR_BAD_ARG: FRI's rules on log_n and log_blowup, log_n - log_blowup outside 7 .. 18,
 *                                       n_proofs = 0, 599 n_proofs > 2^24, a null pointer.
 *   tmx_air_sha512_quotient_range_device   set 3's range call: the piece [proof_lo, proof_hi), d_helper_cols that piece's own columns,
 *                                       written or (accumulate = 1) added; also refused: an empty or overhanging range, accumulate > 1.
 *   tmx_air_sha512_verify_device        tmx_batch_verify_device, the barycentric kernel, then the identity for the oracles k_trace (18 k
 *                                       columns), k_trace + 1 (599 k) and k_trace + 2 (2).  TMX_ERR_BAD_ARG unless the column counts are these
 *                                       and the three log_n equal (and the rules above).
 *   tmx_trace_commit_set_air_sha512_device   set 3's set-level call for `section` = TMX_TRACE_SHA512, a RESIDENT member only: the pair goes
 *                                       directly behind the table; tmx_trace_commit_set_shape reports TMX_TRACE_SHA512_HELPER and
 *                                       TMX_TRACE_SHA512_QUOTIENT.  Refused: any other section, an absent or streamed section, a second
 *                                       call on the section, a set with no room for two more oracles.
 *   tmx_air_sha512_periodic_device      the three preprocessed columns on their own: 3 << log_rows words at d_pre and, extended under the
 *                                       current NTT domain, 3 << (log_rows + log_blowup) words at d_ext (log_blowup = 0: d_pre alone).
 *   tmx_air_sha512_periodic_eval_device d_out[0 .. 6) = SEL(zeta), KLO(zeta), KHI(zeta) for the two words at d_zeta, d_out[6] = 1 if a
 *                                       denominator was zero (d_out: 7 words).  Both refuse log_rows outside 7 .. 18 and null pointers.
 * Scratch: per section set 3's formula with 599 columns -- (599 n_proofs (N + M) + 2 M) 8 bytes plus two trees and the LDE scratch of 599
 * columns -- and once per context (3 (N + M) + 512) 8 bytes for the preprocessed columns and the barycentric kernel's rows.  At 256 proofs,
 * N = 2^15 and blow-up 8 the helper alone is 599 256 2^15 9 8 bytes, about 360 GB: it CANNOT be resident on one card.  The SHA-256-named streamed
 * call keeps refusing every constraint_set but 3, 4 and 5; the streamed form of this helper is
 * tmx_trace_commit_set_air_sha512_streamed_device ("streamed helpers of the SHA-512 sets" below).  Every refusal comes before anything
 * is enqueued; everything is asynchronous on hip_stream; tmx_air_last_gamma covers the quotient calls and the set-level call. */
#define TMX_AIR_SHA512_HELPER_COLS 599
#define TMX_AIR_SHA512_CONSTRAINTS 628
#define TMX_TRACE_SHA512_HELPER 32768u
#define TMX_TRACE_SHA512_QUOTIENT 65536u
int32_t tmx_air_sha512_helper_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, uint64_t* d_helper,
                                     void* hip_stream);
int32_t tmx_air_sha512_quotient_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                       const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                       uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha512_quotient_range_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                             uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                             const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper, uint64_t* d_quot,
                                             void* hip_stream);
int32_t tmx_air_sha512_verify_device(tmx_ctx* ctx, const tmx_batch_params* p, uint32_t k_trace, const uint64_t* d_caps, const uint64_t* d_proof,
                                     uint32_t* d_ok, void* hip_stream);
int32_t tmx_trace_commit_set_air_sha512_device(tmx_ctx* ctx, uint32_t section, uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream);
int32_t tmx_air_sha512_periodic_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t log_blowup, uint64_t* d_pre, uint64_t* d_ext, void* hip_stream);
int32_t tmx_air_sha512_periodic_eval_device(tmx_ctx* ctx, uint32_t log_rows, const uint64_t* d_zeta, uint64_t* d_out, void* hip_stream);

/* ---- the message schedule of the SHA-512 table (constraint set 8) ------------------------------------------------------------------------
 * Set 7 proves the round function on T.2 and leaves W free from row 16 of each block on.  Set 8 is the SCHEDULE: the sibling of set 4 on
 * 64-bit words in lo / hi limbs, with set 7's preprocessed-column mechanism for the period 80.  Sets 7 + 8 together state that every live
 * block of T.2 is a real SHA-512 compression of its first sixteen W words from the state in front of it, and W's limbs are range-checked
 * by their bits.  Everything is additive: no existing kernel, launch, transcript word, refusal, scratch layout or proof word changes; the
 * batch prover, its proof format and tmx_batch_verify_device are used UNCHANGED.  Same field, extension, duplex and caveats as above.
 *   table      T.2 as in set 7: 18 n_proofs columns of 32-bit limbs, W lo at 0 and W hi at 1 inside a proof; row (2 i + b) 80 + t holds W_t.
 *   schedule   W_t = sigma1(W_(t-2)) + W_(t-7) + sigma0(W_(t-15)) + W_(t-16) mod 2^64 for t = 16 .. 79, with
 *              sigma0(x) = x >>> 1 xor x >>> 8 xor x >> 7 and sigma1(x) = x >>> 19 xor x >>> 61 xor x >> 6 (>>> rotates, >> shifts).
 *   preprocessed column  ONE more public column of full degree N - 1 that depends on N alone:
 *                SCH_r = 1 where the NEXT row is a schedule row of the same block, 15 <= r mod 80 <= 78, and r != N - 1; 0 elsewhere.
 *              The wrap row must be switched off explicitly: (2^k - 1) mod 80 is 47, 15, 31, 63 for k = 3, 0, 1, 2 mod 4, always inside
 *              15 .. 78, while row 0 is W_0 of a block.  The prover fills it (k_air_sha512_periodic<Sha512Sched>) and extends it exactly as helper
 *              columns are extended; the verifier commits to nothing and computes SCH(zeta) itself, barycentrically over the N rows
 *              (k_air_sha512_periodic_eval<Sha512Sched>, four rows per F_p^2 inversion, up to 64 workgroups).  It is not observed
 *              by gamma, as SEL, KLO and KHI are not.  A zero denominator clears every verdict.  log_rows 7 .. 18, set 7's range, for the
 *              same reason.
 *   helper     230 columns per proof (twice set 4's 115), bits LSB first, bit indices mod 64; defined for ANY input: the operands are the
 *              low 32 bits of each table word.  Offsets inside a proof:
 *                0 .. 63    WB_i, the bits of W (0 .. 31 the low limb, 32 .. 63 the high limb)
 *               64 .. 127   X0_i = WB_(i+1) xor WB_(i+8)              128 .. 191   X1_i = WB_(i+19) xor WB_(i+61)
 *              192, 193     sigma0(W) lo, hi (G0)                     194, 195     sigma1(W) lo, hi (G1)
 *              195 + k      QL_k, k = 1 .. 15, the low-limb pipeline of the schedule sum      210 + k   QH_k, the same over the high limbs
 *              226, 227     the two bits of CL, the low limb's carry                          228, 229  the two bits of CH
 *              The pipelines are per limb and WITHOUT carries, set 4's pipeline twice, rows cyclic inside one proof:
 *              QL_1(r+1) = W_lo(r) + G0_lo(r+1); QL_k(r+1) = QL_(k-1)(r), plus W_lo(r+1) for k = 9, plus G1_lo(r+1) for k = 14; so
 *              QL_15(r) = W_lo(r-15) + sigma0_lo(r-14) + W_lo(r-6) + sigma1_lo(r-1).  QH the same over the high limbs.  Four summands
 *              below 2^32: a limb sum stays below 2^34.  CL = (QL_15 >> 32) & 3 and CH = ((QH_15 + CL) >> 32) & 3, both 0 where
 *              SCH = 0: every carry is at most 3 and every identity is an integer identity below 2^35.
 *   constraints  234 per proof (twice set 4's 117), at index j; a prime is the value at omega x:
 *                0 .. 63    X^2 - X for WB                               64 .. 67   X^2 - X for the four carry bits (CL_0, CL_1, CH_0, CH_1)
 *               68, 69      W_lo, W_hi - sum_(i < 32) 2^i WB_(32 limb + i)
 *               70 + i      X0_i - (WB_(i+1) + WB_(i+8) - 2 WB_(i+1) WB_(i+8))      134 + i   the same for X1 with 19 and 61
 *              198, 199     sigma0 lo, hi - sum 2^i of X0_j xor WB_(j+7) for j < 57 and X0_j for j >= 57, j = 32 limb + i (the shift by 7
 *                           brings nothing in)                          200, 201   sigma1 the same, with WB_(j+6) for j < 58
 *              201 + k      QL_k' - (W_lo + G0_lo') for k = 1, QL_k' - QL_(k-1) - [k = 9] W_lo' - [k = 14] G1_lo' (linear, unselected)
 *              216 + k      the same for QH over the high limbs
 *              232          SCH(x) (W_lo' + 2^32 (CL_0 + 2 CL_1) - QL_15)
 *              233          SCH(x) (W_hi' + 2^32 (CH_0 + 2 CH_1) - QH_15 - (CL_0 + 2 CL_1))
 *              Every nonlinear constraint has degree 2 and no selector, the two selected ones are SCH (linear): every constraint has degree
 *              <= 2 N - 2, the honest quotient degree <= N - 2, and ONE two-column quotient oracle suffices, as in set 7.  Zero blocks and
 *              zero padding satisfy all 234.
 *   NOT PROVED by sets 7 + 8: the IV and the feed-forward of the two blocks, which constraint set 9 below proves; the link of message and
 *              digest to Level-1, and so of h; LIVE
 *              against anything public; and so a message word W_t, t < 16, changed with the schedule recomputed from it goes undetected
 *              (tests/test_sha512_sched.py records it).
 *   challenge  word for word set 7's with the set id 8: a fresh duplex observes 2^33, then 8, log_n, log_blowup, cap_height, n_proofs, then
 *              the table cap, then THIS helper's cap; gamma drawn again while gamma.c1 == 0.
 *   quotient   q(x_i) = sum_p sum_(j < 234) gamma^(234 p + j) C_(p,j)(x_i) / (x_i^N - 1), planar and canonical; pointwise.
 *   identity   sum_p gamma^(234 p) (a_p + SCH(zeta) b_p) == (u_0 + X u_1) (zeta^N - 1), a the gamma sum of constraints 0 .. 231, b of 232
 *              and 233 without SCH.  The helper's oracle index is explicit, k_helper with the quotient at k_helper + 1, as in set 4: set 7's
 *              pair and set 8's pair can both sit behind one table in one proof.
 *   tmx_air_sha512_sched_helper_device     the helper (230 n_proofs columns at d_helper) from PRE-LDE table columns (18 n_proofs at d_table).
 *                                          TMX_ERR_BAD_ARG: log_rows outside 7 .. 18, n_proofs = 0, 230 n_proofs > 2^24, a null pointer.
 *   tmx_air_sha512_sched_quotient_device   fills and extends SCH under the context's CURRENT NTT domain, draws gamma from d_cap and
 *                                          d_cap_helper, then the quotient of the EXTENDED columns into d_quot (2 << log_n words).
 *                                          TMX_ERR_BAD_ARG: FRI's rules on log_n and log_blowup, log_n - log_blowup outside 7 .. 18,
 *                                          n_proofs = 0, 230 n_proofs > 2^24, a null pointer.
 *   tmx_air_sha512_sched_quotient_range_device   set 3's range call: the piece [proof_lo, proof_hi), d_helper_cols that piece's own columns,
 *                                          written or (accumulate = 1) added; also refused: an empty or overhanging range, accumulate > 1.
 *   tmx_air_sha512_sched_verify_device     tmx_batch_verify_device, the barycentric kernel, then the identity for the oracles k_trace (18 k
 *                                          columns), k_helper (230 k) and k_helper + 1 (2).  TMX_ERR_BAD_ARG unless the column counts are
 *                                          these, the three log_n equal, k_helper > k_trace, k_helper + 1 < n_oracles (and the rules above).
 *   tmx_trace_commit_set_air_sha512_sched_device   set 7's set-level call for this set: `section` = TMX_TRACE_SHA512 alone, a RESIDENT member
 *                                          only; the pair goes behind set 7's pair if that follows the table, and set 7's call inserts in
 *                                          front of it: either order ends as table, H7, Q7, H8, Q8 with the same caps and the same proof.
 *                                          tmx_trace_commit_set_shape reports TMX_TRACE_SHA512_SCHED_HELPER and _SCHED_QUOTIENT.  Refused:
 *                                          any other section, an absent or streamed section, a second call on the section, a set with no
 *                                          room for two more oracles.
 *   tmx_air_sha512_sched_periodic_device   SCH on its own: 1 << log_rows words at d_pre and, extended under the current NTT domain,
 *                                          1 << (log_rows + log_blowup) words at d_ext (log_blowup = 0: d_pre alone).
 *   tmx_air_sha512_sched_periodic_eval_device   d_out[0 .. 2) = SCH(zeta) for the two words at d_zeta, d_out[2] = 1 if a denominator was zero
 *                                          (d_out: 3 words).  Both refuse log_rows outside 7 .. 18 and null pointers.
 * Scratch: per section set 3's formula with 230 columns, and once per context ((N + M) + 256) 8 bytes of its own for SCH and the
 * barycentric kernel's rows (set 7's context scratch is not touched).  The streamed call keeps refusing every constraint_set but 3, 4 and 5.
 * Every refusal comes before anything is enqueued; everything is asynchronous on hip_stream; tmx_air_last_gamma covers the quotient calls
 * and the set-level call.  The block starts of T.2 (IV, feed-forward) are constraint set 9 below.  Follow-up: the link of T.2 to Level-1.  The
 * streamed form of the helper is tmx_trace_commit_set_air_sha512_streamed_device below. */
#define TMX_AIR_SHA512_SCHED_HELPER_COLS 230
#define TMX_AIR_SHA512_SCHED_CONSTRAINTS 234
#define TMX_TRACE_SHA512_SCHED_HELPER 131072u
#define TMX_TRACE_SHA512_SCHED_QUOTIENT 262144u
int32_t tmx_air_sha512_sched_helper_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, uint64_t* d_helper,
                                           void* hip_stream);
int32_t tmx_air_sha512_sched_quotient_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                             const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap,
                                             const uint64_t* d_cap_helper, uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha512_sched_quotient_range_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                   uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                   const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                                   uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha512_sched_verify_device(tmx_ctx* ctx, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, const uint64_t* d_caps,
                                           const uint64_t* d_proof, uint32_t* d_ok, void* hip_stream);
int32_t tmx_trace_commit_set_air_sha512_sched_device(tmx_ctx* ctx, uint32_t section, uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream);
int32_t tmx_air_sha512_sched_periodic_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t log_blowup, uint64_t* d_pre, uint64_t* d_ext, void* hip_stream);
int32_t tmx_air_sha512_sched_periodic_eval_device(tmx_ctx* ctx, uint32_t log_rows, const uint64_t* d_zeta, uint64_t* d_out, void* hip_stream);

/* ---- the block starts of the SHA-512 table (constraint set 9) ----------------------------------------------------------------------------
 * Sets 7 and 8 prove that every live 80-row block of T.2 is a real SHA-512 compression FROM THE STATE IN FRONT OF IT, and tie that state
 * to nothing: SEL is 0 on the last row of every block and on row N - 1, so row 0 of a block is free.  Set 9 is the BLOCK STARTS: the
 * sibling of set 5 on 64-bit words in lo / hi limbs, with sets 7 and 8's preprocessed columns in the place of set 5's subgroup selectors.
 * It proves that every live hash starts from the SHA-512 IV and that the second block of a lane starts from IV + (the state after round
 * 79 of the first block) mod 2^64.  Everything is additive: no existing kernel, launch, transcript word, refusal, scratch layout or proof
 * word changes; the batch prover, its proof format and tmx_batch_verify_device are used UNCHANGED.  Same field, extension, duplex and
 * caveats as above.  Notation as in sets 5 and 7: a prime is the value at omega x, rows are cyclic inside a proof, operands are the low
 * 32 bits of a table word, limb 0 is lo and limb 1 is hi.
 *   table      T.2 as in set 7: 18 n_proofs columns of 32-bit limbs; inside a proof W at 0, 1 and the state words s_0 .. s_7 = a .. h at
 *              2 + 2 j + limb.  A lane is two blocks of 80 rows; row t of a block holds W_t and a .. h AFTER round t; the first block
 *              starts from IV512, an unused second block is zero.
 *   row 0      of a block that starts from H_0 .. H_7 is round 0 applied to them: b = H_0, c = H_1, d = H_2, f = H_4, g = H_5, h = H_6,
 *              a = T1 + T2, e = H_3 + T1 mod 2^64 with T1 = H_7 + Sigma1(H_4) + Ch(H_4, H_5, H_6) + K_0 + W_0 and T2 = Sigma0(H_0) +
 *              Maj(H_0, H_1, H_2); Sigma0(x) = x >>> 28 xor x >>> 34 xor x >>> 39, Sigma1(x) = x >>> 14 xor x >>> 18 xor x >>> 41,
 *              K_0 = 0x428a2f98d728ae22.  Six of the eight words stand in row 0 itself.
 *   preprocessed columns  TWO more public columns of full degree N - 1 that depend on N alone:
 *                STA_r = 1 where the NEXT row is row 0 of a FIRST block: r mod 160 = 159, AND r = N - 1; 0 elsewhere.
 *                CHN_r = 1 where r mod 160 = 79 (the next row is row 0 of a second block); 0 elsewhere.
 *              (2^k - 1) mod 160 is 127, 95, 31, 63 for k = 3, 0, 1, 2 mod 4, never 79 or 159: the wrap row is never a chain row, and
 *              it must be switched ON in STA explicitly, because row 0 is the first row of a hash -- the opposite of SEL and SCH, whose
 *              wrap row is switched off.  The prover fills them (k_air_sha512_periodic<Sha512Init>) and extends them exactly as helper columns
 *              are extended; the verifier commits to nothing and computes STA(zeta) and CHN(zeta) itself, barycentrically over the N rows
 *              (k_air_sha512_periodic_eval<Sha512Init>, four rows per F_p^2 inversion, up to 64 workgroups).  gamma does not
 *              observe them.  A zero denominator clears every verdict.  log_rows 7 .. 18, set 7's range, for the same reason.
 *   helper     629 columns per proof (set 5's 315 in limbs), bits LSB first, bit indices mod 64; defined for ANY input.  Offsets inside
 *              a proof:
 *                0 .. 383   the bits B_i, C_i, D_i, F_i, G_i, H_i of b, c, d, f, g, h of the row, 64 each in this order
 *              384 .. 447   U0_i = B_(i+28) xor B_(i+34)       448 .. 511   U1_i = F_(i+14) xor F_(i+18)       512 .. 575   V_i = B_i C_i
 *              576 .. 583   Sigma0(b), Sigma1(f), Ch(f, g, h), Maj(b, c, d), each as lo, hi
 *              584          LV: set 7's LIVE rule, 1 iff row r - r mod 80 of the proof has a nonzero word
 *              585 + 2 j + limb   PZ_j = LV(r+1) ((IV_j + s_j(r)) mod 2^64), j = 0 .. 7, on every row
 *              601 + 2 j + limb   CZL_j, CZH_j: the carry bits of that sum's two limbs (CZL out of IV_(j,lo) + s_(j,lo), CZH out of
 *                                 IV_(j,hi) + s_(j,hi) + CZL), on every row and whatever LV is
 *              617 .. 628   three bits each of CAL, CAH, CEL, CEH: the limb carries of the a-sum and the e-sum below, masked to three
 *                           bits; 0 unless STA or CHN is 1 on the row
 *              With LV' = LV(r+1), S0' .. MAJ' the four helper words of the next row, and X the start word of the row's kind -- on a
 *              row with STA = 1: H7 = IV_7 LV', H3 = IV_3 LV'; on a row with CHN = 1: H7 = PZ_7, H3 = PZ_3 -- per limb
 *                a-sum = H7 + K_0 LV' + S1' + CH' + W' + S0' + MAJ' (+ CAL in the high limb) = a' + 2^32 CA
 *                e-sum = H3 + H7 + K_0 LV' + S1' + CH' + W' (+ CEL in the high limb) = e' + 2^32 CE
 *              Seven summands below 2^32 and a carry-in of at most 6: CA <= 6.  Six summands: CE <= 5.  Every identity is an integer
 *              identity below 2^35.
 *   constraints  673 per proof, at index j:
 *                0 .. 383   X^2 - X for the bit columns                 384 .. 399   X^2 - X for CZ (at the column's offset - 217)
 *              400 .. 411   X^2 - X for the twelve carry bits           412          LV^2 - LV
 *              413 .. 424   word_limb - sum_(i < 32) 2^i bit_(32 limb + i) for b, c, d, f, g, h (413 + 2 k + limb)
 *              425 + i      U0_i - (B_(i+28) xor B_(i+34))    489 + i   U1_i - (F_(i+14) xor F_(i+18))    553 + i   V_i - B_i C_i
 *              617, 618     Sigma0 lo, hi - sum 2^i (U0_j xor B_(j+39))                619, 620   Sigma1 with U1_j xor F_(j+41)
 *              621, 622     Ch - sum 2^i (H_j + F_j (G_j - H_j))                      623, 624   Maj - sum 2^i (V_j + D_j (B_j + C_j - 2 V_j))
 *              625 + 2 j + limb   PZ_(j,limb) - LV' (IV_(j,limb) + s_(j,limb) [+ CZL_j in the high limb] - 2^32 CZ_(j,limb)): holds on
 *                                 every row by construction, no selector
 *              641 .. 656   STA(x) times: 641 + 2 k + limb   x'_limb - IV_(j,limb) LV' for the six words x = b, c, d, f, g, h
 *                           (j = 0, 1, 2, 4, 5, 6; k counts them); 653, 654   a'_limb + 2^32 CA_limb [- CAL] - ((IV_7 + K_0)_limbwise LV'
 *                           + S1' + CH' + W' + S0' + MAJ'); 655, 656   e'_limb + 2^32 CE_limb [- CEL] - ((IV_3 + IV_7 + K_0)_limbwise LV' +
 *                           S1' + CH' + W'), where "limbwise" adds the constants' limbs as integers
 *              657 .. 672   CHN(x) times: 657 + 2 k + limb   x'_limb - PZ_(j,limb); 669, 670 the a-sum with PZ_7 + K_0 LV'; 671, 672 the
 *                           e-sum with PZ_3 + PZ_7 + K_0 LV'
 *              641 carry no selector; every nonlinear one has degree 2; every selected one is a preprocessed column times a linear form:
 *              every constraint has degree <= 2 N - 2, the honest quotient degree <= N - 2, and ONE two-column quotient oracle suffices,
 *              divided by x^N - 1 alone (set 5's D_s and D_c have no counterpart).  Zero blocks, unused second blocks and zero padding
 *              satisfy all 673 with LV = 0.
 *   NOT PROVED by sets 7 + 8 + 9 (the follow-ups): the first sixteen W of a block and the digest against Level-1, and so h; LV against
 *              anything public -- a hash whose live second block is replaced by a zero block goes unseen, as in set 5
 *              (tests/test_sha512_init.py records both).
 *   challenge  word for word set 7's with the set id 9: a fresh duplex observes 2^33, then 9, log_n, log_blowup, cap_height, n_proofs, then
 *              the table cap, then THIS helper's cap; gamma drawn again while gamma.c1 == 0.
 *   quotient   q(x_i) = sum_p sum_(j < 673) gamma^(673 p + j) C_(p,j)(x_i) / (x_i^N - 1), planar and canonical; pointwise.
 *   identity   sum_p gamma^(673 p) (A_p + STA(zeta) S_p + CHN(zeta) C_p) == (u_0 + X u_1) (zeta^N - 1), A the gamma sum of constraints
 *              0 .. 640, S of 641 .. 656 without STA, C of 657 .. 672 without CHN.  The helper's oracle index is explicit, k_helper with
 *              the quotient at k_helper + 1: [table, H7, Q7, H8, Q8, H9, Q9] is one proof of seven oracles.
 *   tmx_air_sha512_init_helper_device      the helper (629 n_proofs columns at d_helper) from PRE-LDE table columns (18 n_proofs at d_table).
 *                                          TMX_ERR_BAD_ARG: log_rows outside 7 .. 18, n_proofs = 0, 629 n_proofs > 2^24, a null pointer.
 *   tmx_air_sha512_init_quotient_device    fills and extends STA and CHN under the context's CURRENT NTT domain, draws gamma from d_cap
 *                                          and d_cap_helper, then the quotient of the EXTENDED columns into d_quot (2 << log_n words).
 *                                          TMX_ERR_BAD_ARG: FRI's rules on log_n and log_blowup, log_n - log_blowup outside 7 .. 18,
 *                                          n_proofs = 0, 629 n_proofs > 2^24, a null pointer.
 *   tmx_air_sha512_init_quotient_range_device   set 3's range call: the piece [proof_lo, proof_hi), d_helper_cols that piece's own columns,
 *                                          written or (accumulate = 1) added; also refused: an empty or overhanging range, accumulate > 1.
 *   tmx_air_sha512_init_verify_device      tmx_batch_verify_device, the barycentric kernel, then the identity for the oracles k_trace (18 k
 *                                          columns), k_helper (629 k) and k_helper + 1 (2).  TMX_ERR_BAD_ARG unless the column counts are
 *                                          these, the three log_n equal, k_helper > k_trace, k_helper + 1 < n_oracles (and the rules above).
 *   tmx_trace_commit_set_air_sha512_init_device   the set-level call: `section` = TMX_TRACE_SHA512 alone, a RESIDENT member only; the pair
 *                                          goes behind the pairs of sets 7 and 8 where they follow the table, and their calls insert in front
 *                                          of it: every call order ends as table, H7, Q7, H8, Q8, H9, Q9 with the same caps and the same
 *                                          proof.  tmx_trace_commit_set_shape reports TMX_TRACE_SHA512_INIT_HELPER and _INIT_QUOTIENT.
 *                                          Refused: any other section, an absent or streamed section, a second call on the section, a set
 *                                          with no room for two more oracles (TMX_BATCH_MAX_ORACLES = 8: the three pairs leave room for one
 *                                          more table).
 *   tmx_air_sha512_init_periodic_device    STA and CHN on their own: planar, 2 << log_rows words at d_pre and, extended under the current
 *                                          NTT domain, 2 << (log_rows + log_blowup) words at d_ext (log_blowup = 0: d_pre alone).
 *   tmx_air_sha512_init_periodic_eval_device   d_out[0 .. 4) = STA(zeta), CHN(zeta) for the two words at d_zeta, d_out[4] = 1 if a
 *                                          denominator was zero (d_out: 5 words).  Both refuse log_rows outside 7 .. 18 and null pointers.
 * Scratch: per section set 3's formula with 629 columns, and once per context (2 (N + M) + 512) 8 bytes of its own for STA, CHN and the
 * barycentric kernel's rows (the context scratch of sets 7 and 8 is not touched).  The streamed call keeps refusing every constraint_set
 * but 3, 4 and 5.  Every refusal comes before anything is enqueued; everything is asynchronous on hip_stream; tmx_air_last_gamma covers
 * the quotient calls and the set-level call.  The link of T.2 to Level-1 is constraint set 10 ("the SHA-512 table's link to Level-1"
 * below).  At 629 columns the full 256-proof T.2 cannot be
 * resident: the streamed form of the helpers of sets 7 - 9 is the block "streamed helpers of the SHA-512 sets" below. */
#define TMX_AIR_SHA512_INIT_HELPER_COLS 629
#define TMX_AIR_SHA512_INIT_CONSTRAINTS 673
#define TMX_TRACE_SHA512_INIT_HELPER 524288u
#define TMX_TRACE_SHA512_INIT_QUOTIENT 1048576u
int32_t tmx_air_sha512_init_helper_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, uint64_t* d_helper,
                                          void* hip_stream);
int32_t tmx_air_sha512_init_quotient_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                            const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap,
                                            const uint64_t* d_cap_helper, uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha512_init_quotient_range_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                  uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                  const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                                  uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha512_init_verify_device(tmx_ctx* ctx, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, const uint64_t* d_caps,
                                          const uint64_t* d_proof, uint32_t* d_ok, void* hip_stream);
int32_t tmx_trace_commit_set_air_sha512_init_device(tmx_ctx* ctx, uint32_t section, uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream);
int32_t tmx_air_sha512_init_periodic_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t log_blowup, uint64_t* d_pre, uint64_t* d_ext, void* hip_stream);
int32_t tmx_air_sha512_init_periodic_eval_device(tmx_ctx* ctx, uint32_t log_rows, const uint64_t* d_zeta, uint64_t* d_out, void* hip_stream);

/* ---- streamed helpers of the SHA-512 sets: constraint sets 7, 8 and 9 on the full-size T.2 ----
 * The sibling of "streamed helpers of the SHA-256 sets" above, under the same contract.  The helper oracle of a set is 599, 230 or 629
 * columns per proof, 13 to 35 times the 18 columns of T.2; kept extended it is what bounds the size the three set-level calls above can
 * run at.  Here the helper is fed in chunks of whole proofs and never exists extended; the table member stays resident, and so do the
 * helper's PRE-LDE columns (the prove's openings at zeta read them).  Field arithmetic is exact, so the pieces in any order give the
 * resident call's words: for every valid chunk size d_cap_h, d_cap_q, tmx_air_last_gamma, tmx_trace_commit_set_shape and every word of
 * tmx_trace_commit_set_prove_device's proof equal the resident call's.  Resident and streamed pairs may be mixed within the section; the
 * verifiers need nothing.  The pieces of the quotient are those of tmx_air_sha512_quotient_range_device, _sched_quotient_range_device and
 * _init_quotient_range_device above (C = 628, 234, 673).
 *   tmx_trace_commit_set_air_sha512_streamed_bytes   host only: the bytes the call below allocates for its scratch -- pre-LDE helper |
 *                                          helper levels | quotient | quotient levels | sponge states [12][M] | chunk [chunk_proofs
 *                                          helper_cols][M] -- and, in *lde_scratch_bytes (may be null), the LDE's own scratch: twice what
 *                                          is extended at once, which is one chunk (ONE transform call per chunk, as the prove's gather
 *                                          extends a streamed member).  With chunk_proofs >= n_proofs: the resident call's (helper_cols
 *                                          n_proofs (N + M) + 2 M) 8 bytes plus two trees, and twice one proof's helper columns.  0 on a
 *                                          refused shape: constraint_set outside 7 .. 9, chunk_proofs = 0, chunk_proofs helper_cols no
 *                                          multiple of 8 (the sponge absorbs eight columns at a time: a multiple of 8 for sets 7 and 9, of
 *                                          4 for set 8), log_blowup outside 1 .. 6, log_m - log_blowup outside 7 .. 18, n_proofs = 0,
 *                                          helper_cols n_proofs > 2^24.
 *   tmx_trace_commit_set_air_sha512_streamed_device   the set-level call of constraint_set 7, 8 or 9 on TMX_TRACE_SHA512.  chunk_proofs
 *                                          >= n_proofs takes the resident path exactly.  Else: the helper kernel into the pre-LDE columns;
 *                                          sweep 1, per chunk the LDE into the chunk buffer and k_poseidon_leaves_chunk, then the levels and
 *                                          d_cap_h; gamma; the set's preprocessed planes filled and extended once; sweep 2, per chunk the
 *                                          LDE again and the accumulating piece of the quotient; the quotient's tree and d_cap_q.  All of
 *                                          it runs under the set's NTT domain: if tmx_ntt_set_domain moved the context's it is put back
 *                                          for the call and restored after.  The pair is registered by the resident calls' rules (same
 *                                          place by set id, same refusals); a streamed scratch is sized exactly (a larger one left by a
 *                                          resident call on that set is released).  TMX_ERR_BAD_ARG: no set, constraint_set outside
 *                                          7 .. 9, a section other than TMX_TRACE_SHA512 or one that is absent or streamed (the TABLE
 *                                          member must be resident), null caps, a chunk_proofs _bytes refuses, a second call on the
 *                                          section in either form, a full set.  TMX_ERR_CAPACITY against free memory, the LDE's scratch
 *                                          included.  At 256 proofs, N = 2^15, blow-up 8 and chunk_proofs = 8 the three pairs need about
 *                                          50 + 19 + 53 GB where the resident calls need about 880 GB.
 * Every refusal comes before anything is enqueued; everything is asynchronous on hip_stream apart from a domain change.
 * tmx_trace_commit_set_air_sha256_streamed_* keep refusing every constraint_set but 3, 4 and 5: these calls have names of their own. */
uint64_t tmx_trace_commit_set_air_sha512_streamed_bytes(uint32_t constraint_set, uint32_t log_m, uint32_t log_blowup, uint32_t cap_height,
                                                        uint32_t n_proofs, uint32_t chunk_proofs, uint64_t* lde_scratch_bytes);
int32_t tmx_trace_commit_set_air_sha512_streamed_device(tmx_ctx* ctx, uint32_t constraint_set, uint32_t section, uint32_t chunk_proofs,
                                                        uint64_t* d_cap_h, uint64_t* d_cap_q, void* hip_stream);
/* Host only, for tests and memory accounting: the bytes of the scratch the context holds right now for constraint_set 7, 8 or 9 on
 * TMX_TRACE_SHA512, as the last resident or streamed set-level call left it (a streamed call leaves exactly what _streamed_bytes returns);
 * 0 if there is none, for a constraint_set outside 7 .. 9 and for any other section. */
uint64_t tmx_trace_commit_set_air_sha512_scratch_bytes(const tmx_ctx* ctx, uint32_t constraint_set, uint32_t section);

/* ---- the SHA-512 table's link to Level-1 (constraint set 10) ------------------------------------------------------------------------------
 * Sets 7 + 8 + 9 prove that every live block of T.2 is a SHA-512 compression that starts from the IV or from the first block's
 * feed-forward; they do not say WHICH message was hashed nor that the result is the digest Level-1 returns.  Set 10 is set 6's sibling for
 * T.2, built from set 6's public table gathered from the element rows and the preprocessed planes of full degree of sets 7 - 9 (an
 * 80-row block fits no subgroup, so set 6's seventeen coset polynomials have no counterpart and are not needed).  Resident only.
 *   PROVED     together with sets 7 + 8 + 9: for every lane of T.2 the sixteen W words of each live block are the padded message R | A | M
 *              that Level-1's element row carries (the dummy triple where the lane did not sign), the blocks that are live are exactly those
 *              the message length calls for, a first block starts from the IV and a second one from the first block's feed-forward, and
 *              the last live block's feed-forward is the digest of D.1a.  Range argument, set 6's: every constraint below is an integer
 *              identity between values far below p once CD is boolean, the public words are below 2^32 and s_j is range-checked by set
 *              7's bits; the digest rows pin DG to public words below 2^32 and the chain carries that to CV of the next block; the limbs
 *              of DG on the rows between are NOT range-checked by this set (they are in no selected constraint).
 *   slots      T.2 of N = 2^log_rows rows is cut into block slots k = r / 80: lane k / 2, block k mod 2 of its hash.  Every slot with a row
 *              below N counts, the partial last slot too: ceil(N / 80) slots, padded with zero rows to K = 2^log_k, a power of two, so that
 *              set 2's Poseidon digest rule applies to the table as a column-major oracle.
 *   pub        column-major, 49 n_proofs columns of K words, every word < 2^32; per proof (a 64-bit word's LOW limb first, T.2's order):
 *              0 .. 31    w[k][t] as 2 t (low limb), 2 t + 1 (high limb): the sixteen message words of the block
 *              32 .. 47   dig[k][j] as 32 + 2 j, 33 + 2 j: the eight digest words on the LAST LIVE block of a lane, zero elsewhere
 *              48         lv[k]: 1 where the block is live
 *              gathered from H.2 (pubkey, signature.r, message, message_byte_length, signed; a byte is eight big-endian bit elements)
 *              and the 512 digest elements of D.1a ALONE -- neither the trace rows nor the context's Level-1 scratch are read -- by the
 *              rules T.2 is generated by: the message is R | A | M[0 .. min(message_byte_length, 124)); a lane that did not sign is
 *              hashed on the dummy triple (dummy key, dummy R, 32 zero bytes: ONE block, lv = 0 on its second slot); SHA-512 padding
 *              (80, zeros, the 128-bit bit length at the end of the last block; two blocks from message_byte_length = 48 on); lanes >= n_max,
 *              the partial last slot and the padding are zero with lv = 0.
 *   helper     65 columns per proof of N words, all < 2^32, defined for any input (operands are the low 32 bits of the words, lv is set
 *              when its low 32 bits are not zero):
 *              0 .. 15    CV_j as 2 j, 2 j + 1: the state the row's block starts from, constant inside a block -- IV_j in a live first
 *                         block; in a live second block lv[k - 1] IV_j + s_j of the row in front of it, mod 2^64; 0 where lv[k] = 0
 *              16 .. 31   DG_j = (CV_j + s_j) mod 2^64 on every row, s_j the row's state word j (a .. h)
 *              32 .. 47   CDL_j, CDH_j as 32 + 2 j, 33 + 2 j: the carry bits out of the low and the high limb of that sum
 *              48         LN: lv of the NEXT slot -- the slot of the next row, cyclic: behind the last slot stands slot 0
 *              49 .. 64   CH_j = LN DG_j
 *   planes     five preprocessed columns of full degree, filled and extended by the prover like helper columns and evaluated at zeta by the
 *              verifier barycentrically over the N rows: STA (r mod 160 = 159, and the wrap row N - 1 switched on explicitly) and CHN
 *              (r mod 160 = 79), set 9's; SEL, set 7's; E79 (r mod 80 = 79); MSG (r mod 80 < 16).
 *   constraints 115 per proof, x' the value at the next row, c = 2 j + limb:
 *              0 .. 15    CD_c (CD_c - 1)
 *              16 .. 31   DG_c + 2^32 CD_c - CV_c - s_c [- CDL_j in the high limb]
 *              32 .. 47   CH_c - LN DG_c
 *              48 .. 63   SEL (CV_c' - CV_c)
 *              64 .. 79   CHN (CV_c' - CH_c): the second block starts from this block's DG, or from 0
 *              80 .. 95   STA (CV_c' - IV_c LN)
 *              96         (CHN + STA) LN - lv of the next slot
 *              97 .. 112  E79 DG_c - CHN CH_c - dig_c of the row's slot
 *              113, 114   MSG W_limb - w[k][t]_limb on row 80 k + t
 *              Every nonlinear one has degree 2 and no selector, every selected one is a plane times a linear form: ONE two-column
 *              quotient over x^N - 1 suffices, of honest degree N - 2.  The public terms (96 .. 114) enter linearly: under gamma they are ONE
 *              F_p^2 value per row, V_r = sum_p sum_j gamma^(115 p + j) (the term of constraint j of proof p on row r), and Pub_gamma is
 *              the polynomial of degree < N through V_r on the trace domain.
 *   challenge  set 6's rule with the set id 10: a fresh duplex observes 2^33, then 10, log_n, log_blowup, cap_height, n_proofs, the table
 *              cap, THIS helper's cap, then the Poseidon Merkle root (cap height 0) of pub as a column-major oracle of K rows; gamma drawn
 *              again while gamma.c1 == 0.
 *   quotient   q(x_i) = (sum_p sum_(j < 115) gamma^(115 p + j) C_(p,j)(x_i) - Pub_gamma(x_i)) / (x_i^N - 1), C the column parts, planar and
 *              canonical.  In pieces, Pub_gamma is subtracted by the piece that starts at proof 0 (set 6's rule).
 *   identity   sum_p gamma^(115 p) (A_p + STA(zeta) S_p + CHN(zeta) C_p) - Pub_gamma(zeta) == (u_0 + X u_1) (zeta^N - 1).  The verifier hashes
 *              d_pub itself, forms its own V_r and evaluates Pub_gamma(zeta) barycentrically over the N rows; it trusts nothing the prover
 *              extended.  A zero denominator in either barycentric sum or a failed identity clears every verdict.
 *   tmx_air_sha512_public_shape          host only: log2 K and the column count 49 n_proofs of pub for (kind, n_max, n_proofs), from
 *                                        tmx_trace_commit_shape's rows of TMX_TRACE_SHA512.  TMX_ERR_BAD_ARG: a bad kind or n_max,
 *                                        n_proofs = 0, 65 n_proofs > 2^24, a table outside 2^7 .. 2^18 rows.
 *   tmx_air_sha512_public_device         gathers pub from the element rows at d_elems as tmx_witness_batch_device leaves them (n_proofs rows
 *                                        of the context's n_max): one lane per (proof, slot).  Also refused: a null pointer.
 *   tmx_air_sha512_link_helper_device    the helper (65 n_proofs columns at d_helper) from PRE-LDE table columns (18 n_proofs at d_table) and
 *                                        pub (49 n_proofs columns of 2^log_k words, log_k = ceil(log2(ceil(2^log_rows / 80)))): one lane per
 *                                        (proof, row).  TMX_ERR_BAD_ARG: log_rows outside 7 .. 18, n_proofs = 0, 65 n_proofs > 2^24, a null
 *                                        pointer.
 *   tmx_air_sha512_link_quotient_device  fills and extends the five planes under the context's CURRENT NTT domain, draws gamma from d_cap,
 *                                        d_cap_helper and the digest of d_pub, then the quotient of the EXTENDED columns into d_quot (2 <<
 *                                        log_n words), V_r, its extension and the subtraction.  TMX_ERR_BAD_ARG: FRI's rules on log_n and
 *                                        log_blowup, log_n - log_blowup outside 7 .. 18, n_proofs = 0, 65 n_proofs > 2^24, a null pointer.
 *   tmx_air_sha512_link_quotient_range_device   set 3's range call: the piece [proof_lo, proof_hi), d_helper_cols that piece's own columns,
 *                                        written or (accumulate = 1) added; also refused: an empty or overhanging range, accumulate > 1.
 *   tmx_air_sha512_link_verify_device    tmx_batch_verify_device, gamma from the caps and the verifier's own digest of d_pub, the two
 *                                        barycentric kernels, then the identity for the oracles k_trace (18 k columns), k_helper (65 k) and
 *                                        k_helper + 1 (2).  TMX_ERR_BAD_ARG unless the column counts are these, the three log_n equal,
 *                                        k_helper > k_trace, k_helper + 1 < n_oracles, d_pub set (and the rules above).
 *   tmx_trace_commit_set_air_sha512_link_device   the set-level call: `section` = TMX_TRACE_SHA512 alone, a RESIDENT member only; the pair
 *                                        (TMX_TRACE_SHA512_LINK_HELPER, _LINK_QUOTIENT) goes behind every pair of sets 7 - 9 that follows
 *                                        the table, and their calls insert in front of it.  Refused before anything is enqueued: any other
 *                                        section, an absent or streamed section, a second call on the section, a null pointer, a set with
 *                                        no room for two more oracles.  TMX_BATCH_MAX_ORACLES stays 8: [table, H7, Q7, H8, Q8, H9, Q9]
 *                                        refuses this pair, so sets 7 - 9 combine with set 10 at most two at a time on one section.
 *   tmx_air_sha512_link_periodic_device, _periodic_eval_device   the five planes on their own (5 << log_rows words, extended 5 << (log_rows +
 *                                        log_blowup)), and at zeta: d_out[0 .. 10), d_out[10] = 1 if a denominator was zero.
 *   tmx_air_sha512_link_public_side_device, _public_eval_device   the public side on its own, for tests: V (2 << log_rows words) under a given
 *                                        gamma and its extension; Pub_gamma(zeta) from a V: d_out[0 .. 2), d_out[2] the flag.
 * Scratch: per section set 3's formula with 65 columns, and once per context (7 (N + M) + 66816) 8 bytes of its own (the planes,
 * V and the extended Pub_gamma, the rows of the two barycentric kernels, the levels of the public digest; the scratch of sets 6 - 9 is not
 * touched).  Every refusal comes before anything is enqueued; everything is asynchronous on hip_stream apart from a domain change;
 * tmx_air_last_gamma covers the quotient calls and the set-level call.  The streamed SHA-512 call keeps refusing constraint_set 10.  Still
 * open: the reduction h = digest mod L against D.1b; LIVE / LV of sets 7 and 9 against this lv; a streamed form of the helper (65 columns
 * per proof at 256 proofs, N = 2^15 and blow-up 8 are about 39 GB extended: resident only); a wider oracle cap. */
#define TMX_AIR_SHA512_PUBLIC_WIDTH 49
#define TMX_AIR_SHA512_LINK_HELPER_COLS 65
#define TMX_AIR_SHA512_LINK_CONSTRAINTS 115
#define TMX_TRACE_SHA512_LINK_HELPER 2097152u
#define TMX_TRACE_SHA512_LINK_QUOTIENT 4194304u
int32_t tmx_air_sha512_public_shape(int32_t kind, uint32_t n_max, uint32_t n_proofs, uint32_t* log_k, uint32_t* n_cols);
int32_t tmx_air_sha512_public_device(tmx_ctx* ctx, int32_t kind, uint32_t n_proofs, const void* d_elems, uint64_t* d_pub, void* hip_stream);
int32_t tmx_air_sha512_link_helper_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t n_proofs, const uint64_t* d_table, const uint64_t* d_pub,
                                          uint64_t* d_helper, void* hip_stream);
int32_t tmx_air_sha512_link_quotient_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                            const uint64_t* d_cols, const uint64_t* d_helper_cols, const uint64_t* d_cap,
                                            const uint64_t* d_cap_helper, const uint64_t* d_pub, uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha512_link_quotient_range_device(tmx_ctx* ctx, uint32_t log_n, uint32_t log_blowup, uint32_t cap_height, uint32_t n_proofs,
                                                  uint32_t proof_lo, uint32_t proof_hi, uint32_t accumulate, const uint64_t* d_cols,
                                                  const uint64_t* d_helper_cols, const uint64_t* d_cap, const uint64_t* d_cap_helper,
                                                  const uint64_t* d_pub, uint64_t* d_quot, void* hip_stream);
int32_t tmx_air_sha512_link_verify_device(tmx_ctx* ctx, const tmx_batch_params* p, uint32_t k_trace, uint32_t k_helper, const uint64_t* d_caps,
                                          const uint64_t* d_proof, const uint64_t* d_pub, uint32_t* d_ok, void* hip_stream);
int32_t tmx_trace_commit_set_air_sha512_link_device(tmx_ctx* ctx, uint32_t section, const uint64_t* d_pub, uint64_t* d_cap_h, uint64_t* d_cap_q,
                                                    void* hip_stream);
int32_t tmx_air_sha512_link_periodic_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t log_blowup, uint64_t* d_pre, uint64_t* d_ext, void* hip_stream);
int32_t tmx_air_sha512_link_periodic_eval_device(tmx_ctx* ctx, uint32_t log_rows, const uint64_t* d_zeta, uint64_t* d_out, void* hip_stream);
int32_t tmx_air_sha512_link_public_side_device(tmx_ctx* ctx, uint32_t log_rows, uint32_t log_blowup, uint32_t n_proofs, const uint64_t* d_pub,
                                               const uint64_t* d_gamma, uint64_t* d_v, uint64_t* d_ext, void* hip_stream);
int32_t tmx_air_sha512_link_public_eval_device(tmx_ctx* ctx, uint32_t log_rows, const uint64_t* d_v, const uint64_t* d_zeta, uint64_t* d_out,
                                               void* hip_stream);

/* Self-test hook: k_ed_fin inverts with Bernstein-Yang division steps (inv25519.hpp); this runs that inversion and the Fermat chain
 * on n caller-provided values (eight little-endian words each, taken mod 2^255 - 19) and returns both results per value:
 * out_words[16 i .. 16 i + 7] = Fermat, out_words[16 i + 8 .. 16 i + 15] = division steps.  Host buffers, blocking. */
int32_t tmx_selftest_fe_invert(tmx_ctx* ctx, uint32_t n, const uint32_t* in_words, uint32_t* out_words);

/* Self test of the limb-parallel field arithmetic used by the table chain: per item 128 words in (A, B: 4 rows x 16 limbs), 256 words
 * out (A*B | 2^doublings * A as a point | A in ten limbs | B's ten-limb words in 16-bit limbs).  Test hook, not part of the path. */
int32_t tmx_selftest_f16(tmx_ctx* ctx, uint32_t n, uint32_t doublings, const uint32_t* in_words, uint32_t* out_words);

#ifdef __cplusplus
}
#endif
#endif
