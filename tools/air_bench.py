#!/usr/bin/env python3
"""The ladder rows' constraint quotient (tmx_air_*) next to what it is measured against: one JSON line per mode (MODE=kernels,set by default).
  kernels  COLS_PROOFS proofs x 65 random columns of 2^LOG_M words resident on the device (the SHA-512-sized shape: 70 x 65 = 4550 columns of
           2^18): the quotient call (transcript + tables + k_air_ladder_quotient) and a plain FRI prove over the SAME columns, alternating,
           REPS calls each per round.  The prove's "combine" stage (tmx_fri_last_ms) is k_fri_combine over the same bytes.  Run the tool
           under `rocprofv3 --kernel-trace --stats -- python tools/air_bench.py` (MODE=kernels) for the two kernels' own times in one run.
  set      P proofs at N = n (64 x 128 by default: the ladders fit resident), all five tables: the set prove without and with the quotient
           oracle, alternating; the set-air call on a resident and on a streamed (CHUNK columns) ladders member.  The streamed call extends
           every chunk once more: its excess over the resident call is the re-LDE.
  kernels2 the same resident columns as `kernels` with a random public table: the set-1 quotient call and the set-2 call (digest, transcript,
           V, coefficients, extension, tables, k_air_ladder_boundary_quotient), alternating.  Under `rocprofv3 --kernel-trace --stats` (MODE=
           kernels2,set2) both hot passes and the public-side kernels show in ONE trace.
  set2     as `set` for constraint set 2 next to set 1: the gather, then the set-level calls of both sets on a resident and on a streamed
           ladders member, alternating inside one process; the prove and tmx_air_boundary_verify_device over the set-2 quotient.
  sha      constraint set 3 (tmx_air_sha256_*): SHA_PROOFS proofs x 9 random table columns of 2^LOG_M words (64 proofs at 2^16 by default; the
           helper is 300 columns per proof, 33x the table): the helper kernel on the pre-LDE shape, the quotient call (transcript + tables +
           k_air_sha_quotient) beside a plain FRI prove over the SAME table, alternating -- under `rocprofv3 --kernel-trace --stats` (MODE=sha)
           k_air_sha_helper, k_air_sha_quotient and k_fri_combine show in ONE trace -- and the set-level call on the HEADER member of a set of
           SHA_SET_P proofs at N = n (skip), with the prove and tmx_air_sha256_verify_device over the enlarged set.
  sched    constraint set 4 (tmx_air_sha256_sched_*) beside set 3 over the SAME table: SHA_PROOFS proofs x 9 random table columns of 2^LOG_M
           words, set 4's helper (115 columns per proof) and set 3's (300): k_air_sched_helper on the pre-LDE shape, then the set-4 quotient
           call and the set-3 quotient call, alternating -- under `rocprofv3 --kernel-trace --stats` (MODE=sched, or MODE=sha,sched)
           k_air_sched_quotient and k_air_sha_quotient show in ONE trace -- and both set-level calls on the HEADER member of one set of
           SHA_SET_P proofs at N = n (skip), alternating, with the prove and both verifiers over the set of five oracles.
  init     constraint set 5 (tmx_air_sha256_init_*) beside set 3 over the SAME table: SHA_PROOFS proofs x 9 random table columns of 2^LOG_M
           words, set 5's helper (315 columns per proof, CHAIN=1 by default) and set 3's (300): k_air_init_helper on the pre-LDE shape, then
           the set-5 quotient call and the set-3 quotient call, alternating -- under `rocprofv3 --kernel-trace --stats` (MODE=sha,init)
           k_air_init_quotient and k_air_sha_quotient show in ONE trace -- and the three set-level calls on the HEADER member of one set of
           SHA_SET_P proofs at N = n (skip), alternating, with the prove and the three verifiers over the set of seven oracles.
  parent   the set commit + prove WITHOUT any air call, then the set-3 and set-4 set-level calls on HEADER (MODE=set_plain,sets34), for library
           builds named in LIBS (comma separated), one subprocess per measurement, alternating under TMX_LIB (differences between boxes exceed
           most changes: compare inside one call).  PARENT_MODES names other modes for the subprocesses: `init,set_plain` adds the set-5
           set-level call (a parent that has set 5).
  sha_streamed  the streamed helpers of constraint sets 3 - 5 (tmx_trace_commit_set_air_sha256_streamed_device) on a set SHA256 | SECTION
           of SHA_SET_P proofs at N = n (skip), the sets named in SETS (3 by default; 3,4,5), CHUNK_PROOFS proofs per chunk (8).  SECTION=
           HEADER (default): the resident and the streamed set-level calls, alternating in one process after a warm call, with the prove
           after each; cap digests of both forms; and the chunk LDE alone (the two sweeps' transforms over buffers of the same sizes): the
           helper-LDE share of the streamed call.  SECTION=TREE or SHA256: the streamed calls only, once (the resident helper does not
           fit at full size): the bytes from tmx_trace_commit_set_air_sha256_streamed_bytes, free memory before and after, digests of
           both caps per set, the times, and the verdicts of the three verifiers on one proof over the set.
  link     the public table and the helper of constraint set 6 (tmx_air_sha256_public_device, tmx_air_sha256_link_helper_device): the gather
           of T.3, T.5 and T.6 from the element rows of P proofs at N = n (skip), one time per section, and k_air_link_helper over
           SHA_PROOFS proofs x 9 random table columns of 2^LOG_ROWS words (13 by default) under random public flags, with the bytes it moves
           and link_helper_sha256, the SHA-256 of the words it leaves; then the quotient call (the public digest, gamma, the tables, the
           public side, k_air_link_quotient) over random extended columns of the same shape beside a plain FRI prove over the SAME helper
           columns, alternating.  Under `rocprofv3 --kernel-trace --stats` (MODE=link) k_air_sha_public_gather, k_air_link_helper,
           k_air_link_quotient and k_fri_combine show in ONE trace.  Between the two: the set-level call
           (tmx_trace_commit_set_air_sha256_link_device) on the HEADER member of a set SHA256 | HEADER of the same P proofs beside set 5's
           call on the same set, alternating, with the prove over table, H5, Q5, H6, Q6 and both verifiers.
  sha512   constraint set 7 (tmx_air_sha512_*) beside set 3, its yardstick: k_air_sha512_helper over S512_PROOFS proofs (16) x 18 random table
           columns, then the quotient call of set 7 (the preprocessed columns filled and extended, gamma, the tables, k_air_sha512_quotient<Sha512Round, FORM>)
           and of set 3 (SHA_PROOFS proofs, 32) over random extended columns at M = 2^LOG_M (16), and a plain FRI prove over set 7's table
           columns, alternating; ns_per_helper_word_set7 / _set3 and their ratio.  Under `rocprofv3 --kernel-trace --stats` (MODE=sha512) the
           helper kernel, both hot passes and k_fri_combine show in ONE trace.  Then the set-level call on the SHA512 member of a set
           SHA512 | HEADER of S512_SET_P proofs (16) at N = n, the prove over table, helper, quotient and HEADER, and the verifier.
  sha512_sched   constraint set 8 (tmx_air_sha512_sched_*) beside set 4, its yardstick: k_air_sha512_sched_helper over S512_PROOFS proofs (16)
           x 18 random table columns, then the quotient call of set 8 (SCH filled and extended, gamma, the tables,
           k_air_sha512_quotient<Sha512Sched, FORM>; 248 columns per proof) and of set 4 (SCHED_PROOFS proofs, 32; 124 columns per proof) over random
           extended columns at M = 2^LOG_M (16), alternating; ps_per_helper_word_set8 / _set4 and their ratio.  Then the set-level call of
           set 8 on the SHA512 member of a set SHA512 | HEADER of S512_SET_P proofs (16) at N = n, the prove and the verifier.
  sha512_init    constraint set 9 (tmx_air_sha512_init_*) beside set 7, its yardstick: k_air_sha512_init_helper over S512_PROOFS proofs (16)
           x 18 random table columns of 2^(LOG_M - BLOWUP) rows, then the quotient call of set 9 (STA and CHN filled and extended, gamma, the
           tables, k_air_sha512_quotient<Sha512Init, FORM>; 647 columns per proof) and of set 7 (617 columns per proof) over random extended columns at
           M = 2^LOG_M (16) and the SAME table, alternating in one process; ps_per_helper_word_set9 / _set7 and their ratio.  Then the
           set-level call of set 9 on the SHA512 member of a set SHA512 | HEADER of S512_SET_P proofs (16) at N = n, the prove and the
           verifier.
  sha512_link    constraint set 10 (tmx_air_sha512_link_*), the SHA-512 table's link to Level-1, beside set 6 and set 8: the gather
           (k_air_sha512_public_gather over S512_SET_P proofs at N = n) and the helper kernel (S512_PROOFS proofs, 16, of 2^(LOG_M - BLOWUP)
           rows), then the quotient call of set 10 (five planes filled and extended, gamma with the public digest, the tables,
           k_air_sha512_quotient<Sha512Link, FORM>, V, its extension and the subtraction; 83 columns per proof), of set 8 (248) and of set 6
           (42, 9 table columns) over random extended columns at M = 2^LOG_M (16), alternating in one process; ps per word read of each and
           the ratios.  Then the set-level call of set 10 on the SHA512 member of a set SHA512 | HEADER of S512_SET_P proofs (16) at N = n,
           the prove over the four oracles and the verifier.
  sha512_streamed  the streamed helpers of constraint sets 7 - 9 (tmx_trace_commit_set_air_sha512_streamed_device), sha_streamed's sibling, on
           a set SHA512 | HEADER of SHA_SET_P proofs (16) at N = n, the sets named in SETS (7 by default; 7,8,9), CHUNK_PROOFS proofs per
           chunk (8).  The resident and the streamed set-level calls, alternating in one process after a warm call, every round listed,
           with the prove after each; cap digests of both forms; and the chunk LDE alone (one sweep's and the two sweeps' transforms over
           buffers of the same sizes: what the call and the prove have over the resident form).  FULL=1: the streamed calls only, once each
           (the resident helpers do not fit at full size): the bytes from tmx_trace_commit_set_air_sha512_streamed_bytes, free memory
           before and after every call, digests of both caps per set, the times, one prove, the degree flag and the verdicts of the sets'
           verifiers; a refusal (TMX_ERR_CAPACITY on a shared card) is recorded with its text.
Times per call from HIP events around REPS back-to-back calls after one warm call.  The modes sha, sched and init draw their columns from
SEED (1 by default) and print quotient_sha256, the SHA-256 of the quotient words their call leaves: equal digests from two library builds
(one of them named by TMX_LIB) say that both write the same words at the timed size.
   P=64 N=128 python tools/air_bench.py   (BLOWUP=3 CAP=4 ARITY=4 FINAL=5 QUERIES=28 CHUNK=512 REPS=5 ROUNDS=3 by default)"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
modes = os.environ.get("MODE", "kernels,set").split(",")
P, n = int(os.environ.get("P", "64")), int(os.environ.get("N", "128"))
log_blowup, cap_h, reps = int(os.environ.get("BLOWUP", "3")), int(os.environ.get("CAP", "4")), int(os.environ.get("REPS", "5"))
arity, final_max, nq = int(os.environ.get("ARITY", "4")), int(os.environ.get("FINAL", "5")), int(os.environ.get("QUERIES", "28"))
chunk, rounds = int(os.environ.get("CHUNK", "512")), int(os.environ.get("ROUNDS", "3"))
seed = int(os.environ.get("SEED", "1"))
r4 = lambda x: round(x, 4)

if "parent" in modes:
    libs = [os.path.abspath(x) for x in os.environ["LIBS"].split(",")]
    res = {os.path.basename(os.path.dirname(l)) + "/" + os.path.basename(l): [] for l in libs}
    for _ in range(rounds):
        for l, key in zip(libs, res):
            o = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, MODE=os.environ.get("PARENT_MODES", "sets34,set_plain"), TMX_LIB=l), capture_output=True, text=True)
            line = [json.loads(x) for x in o.stdout.splitlines() if x.startswith("{")]
            res[key].append(line if line else {"failed": o.stderr[-300:]})
    print(json.dumps({"mode": "parent", "proofs": P, "n": n, "runs": res}), flush=True)
    modes = [m for m in modes if m != "parent"]
    if not modes:
        sys.exit(0)

import torch  # noqa: E402
from tendermintx_amd import Context, _lib  # noqa: E402
from tendermintx_amd.context import KIND_SKIP  # noqa: E402

dev = torch.device("cuda:0")


def words_digest(call, buf):
    """SHA-256 of the words `call` leaves in the device buffer `buf`"""
    call()
    torch.cuda.synchronize(dev)
    return hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest()


def timed(fn, k, before=None):
    """ms per call; `before` runs ahead of every call, outside the timed events (a call that can only be made once per set)"""
    (before or (lambda: None))()
    fn()  # (warm: the scratch grows on first use)
    torch.cuda.synchronize(dev)
    total = 0.0
    for _ in range(k):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        total += a.elapsed_time(b)
    return total / k


if "kernels" in modes:
    log_m, cp = int(os.environ.get("LOG_M", "18")), int(os.environ.get("COLS_PROOFS", "70"))
    n_cols = 65 * cp
    ctx = Context(4, b"celestia", device=0)
    cols = torch.randint(0, 2**62, (n_cols << log_m,), dtype=torch.int64, device=dev)
    lv = torch.empty(4 * ctx.poseidon_merkle_digests(log_m, cap_h), dtype=torch.int64, device=dev)
    ctx.poseidon_merkle_device(log_m, n_cols, cols.data_ptr(), cap_h, lv.data_ptr(), 0)
    cap = lv[-(4 << cap_h):]
    quot = torch.empty(2 << log_m, dtype=torch.int64, device=dev)
    fp = dict(log_n=log_m, n_cols=n_cols, cap_height=cap_h, log_blowup=log_blowup, arity_bits=arity, final_log_max=final_max, n_queries=nq)
    proof = torch.empty(ctx.fri_layout(fp)["words"], dtype=torch.int64, device=dev)
    res = {"mode": "kernels", "columns": n_cols, "log_m": log_m, "table_gib": round(n_cols * 8 * 2**log_m / 2**30, 2), "reps": reps,
           "air_quotient_call_ms": [], "fri_prove_ms": [], "fri_combine_stage_ms": []}
    for _ in range(rounds):
        res["air_quotient_call_ms"].append(r4(timed(lambda: ctx.air_ladder_quotient_device(log_m, log_blowup, cap_h, cp, cols.data_ptr(), cap.data_ptr(),
                                                                                           quot.data_ptr(), 0), reps)))
        res["fri_prove_ms"].append(r4(timed(lambda: ctx.fri_prove_device(fp, cols.data_ptr(), lv.data_ptr(), proof.data_ptr(), 0), reps)))
        res["fri_combine_stage_ms"].append(r4(ctx.fri_last_ms()["combine"]))
    best = min(res["air_quotient_call_ms"])
    res["air_gb_per_s"] = round(n_cols * 8 * 2**log_m / best / 1e6, 1)
    res["ratio_air_over_combine"] = round(best / min(res["fri_combine_stage_ms"]), 3)
    print(json.dumps(res), flush=True)
    ctx.close()
    del cols, lv, quot, proof
    torch.cuda.empty_cache()

if "kernels2" in modes:
    log_m, cp = int(os.environ.get("LOG_M", "18")), int(os.environ.get("COLS_PROOFS", "70"))
    n_cols, log_k = 65 * cp, log_m - log_blowup - 8
    ctx = Context(4, b"celestia", device=0)
    cols = torch.randint(0, 2**62, (n_cols << log_m,), dtype=torch.int64, device=dev)
    pub = torch.randint(0, 2**62, ((17 * cp) << log_k,), dtype=torch.int64, device=dev)
    lv = torch.empty(4 * ctx.poseidon_merkle_digests(log_m, cap_h), dtype=torch.int64, device=dev)
    ctx.poseidon_merkle_device(log_m, n_cols, cols.data_ptr(), cap_h, lv.data_ptr(), 0)
    cap = lv[-(4 << cap_h):]
    quot = torch.empty(2 << log_m, dtype=torch.int64, device=dev)
    res = {"mode": "kernels2", "columns": n_cols, "log_m": log_m, "log_k": log_k, "table_gib": round(n_cols * 8 * 2**log_m / 2**30, 2), "reps": reps,
           "set1_call_ms": [], "set2_call_ms": []}
    for _ in range(rounds):
        res["set1_call_ms"].append(r4(timed(lambda: ctx.air_ladder_quotient_device(log_m, log_blowup, cap_h, cp, cols.data_ptr(), cap.data_ptr(),
                                                                                   quot.data_ptr(), 0), reps)))
        res["set2_call_ms"].append(r4(timed(lambda: ctx.air_ladder_boundary_quotient_device(log_m, log_blowup, cap_h, cp, cols.data_ptr(), cap.data_ptr(),
                                                                                            pub.data_ptr(), quot.data_ptr(), 0), reps)))
    res["set2_gb_per_s"] = round(n_cols * 8 * 2**log_m / min(res["set2_call_ms"]) / 1e6, 1)
    res["ratio_set2_over_set1_call"] = round(min(res["set2_call_ms"]) / min(res["set1_call_ms"]), 3)
    print(json.dumps(res), flush=True)
    ctx.close()
    del cols, pub, lv, quot
    torch.cuda.empty_cache()

if "sha" in modes:
    log_m, cp = int(os.environ.get("LOG_M", "16")), int(os.environ.get("SHA_PROOFS", "64"))
    log_rows, n_cols, n_hcols = log_m - log_blowup, 9 * cp, 300 * cp
    torch.manual_seed(seed)
    ctx = Context(4, b"celestia", device=0)
    table = torch.randint(0, 2**62, (n_cols << log_rows,), dtype=torch.int64, device=dev)
    pre = torch.empty(n_hcols << log_rows, dtype=torch.int64, device=dev)
    cols = torch.randint(0, 2**62, (n_cols << log_m,), dtype=torch.int64, device=dev)
    hcols = torch.randint(0, 2**62, (n_hcols << log_m,), dtype=torch.int64, device=dev)
    caps = []
    for c_, k_ in ((cols, n_cols), (hcols, n_hcols)):
        lv = torch.empty(4 * ctx.poseidon_merkle_digests(log_m, cap_h), dtype=torch.int64, device=dev)
        ctx.poseidon_merkle_device(log_m, k_, c_.data_ptr(), cap_h, lv.data_ptr(), 0)
        caps.append(lv)
    quot = torch.empty(2 << log_m, dtype=torch.int64, device=dev)
    fp = dict(log_n=log_m, n_cols=n_cols, cap_height=cap_h, log_blowup=log_blowup, arity_bits=arity, final_log_max=final_max, n_queries=nq)
    proof = torch.empty(ctx.fri_layout(fp)["words"], dtype=torch.int64, device=dev)
    words = (n_cols + n_hcols) << log_m
    res = {"mode": "sha", "proofs": cp, "log_m": log_m, "table_columns": n_cols, "helper_columns": n_hcols, "read_gib": round(words * 8 / 2**30, 2),
           "reps": reps, "helper_kernel_ms": [], "sha_quotient_call_ms": [], "fri_prove_table_ms": [], "fri_combine_stage_ms": []}
    for _ in range(rounds):
        res["helper_kernel_ms"].append(r4(timed(lambda: ctx.air_sha256_helper_device(log_rows, cp, table.data_ptr(), pre.data_ptr(), 0), reps)))
        res["sha_quotient_call_ms"].append(r4(timed(lambda: ctx.air_sha256_quotient_device(log_m, log_blowup, cap_h, cp, cols.data_ptr(), hcols.data_ptr(),
                                                                                            caps[0][-(4 << cap_h):].data_ptr(),
                                                                                            caps[1][-(4 << cap_h):].data_ptr(), quot.data_ptr(), 0), reps)))
        res["fri_prove_table_ms"].append(r4(timed(lambda: ctx.fri_prove_device(fp, cols.data_ptr(), caps[0].data_ptr(), proof.data_ptr(), 0), reps)))
        res["fri_combine_stage_ms"].append(r4(ctx.fri_last_ms()["combine"]))
    res["quotient_sha256"] = words_digest(lambda: ctx.air_sha256_quotient_device(log_m, log_blowup, cap_h, cp, cols.data_ptr(), hcols.data_ptr(),
                                                                                 caps[0][-(4 << cap_h):].data_ptr(),
                                                                                 caps[1][-(4 << cap_h):].data_ptr(), quot.data_ptr(), 0), quot)
    best = min(res["sha_quotient_call_ms"])
    res["sha_gb_per_s"] = round(words * 8 / best / 1e6, 1)
    res["helper_store_gb_per_s"] = round((n_hcols << log_rows) * 8 / min(res["helper_kernel_ms"]) / 1e6, 1)
    res["ns_per_point_proof"] = round(best * 1e6 / (cp << log_m), 2)
    print(json.dumps(res), flush=True)
    ctx.close()
    del table, pre, cols, hcols, caps, quot, proof
    torch.cuda.empty_cache()
    # the set-level call on HEADER
    from tendermintx_amd.synth import bench_workload
    sp = int(os.environ.get("SHA_SET_P", "16"))
    w = bench_workload("survey8d", n, sp, seed=0x544D58)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = Context(n, b"celestia", 100800, device=0, max_batch=sp)
    out = torch.empty(sp * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
    rep = torch.empty(sp * 64, dtype=torch.uint8, device=dev)
    tr = torch.empty(sp * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(KIND_SKIP, sp, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(KIND_SKIP, sp, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    del out
    SHA256, HEADER = 4, 32
    cw = 4 << cap_h
    scaps, cap_h_, cap_q = torch.zeros(2 * cw, dtype=torch.int64, device=dev), torch.zeros(cw, dtype=torch.int64, device=dev), torch.zeros(cw, dtype=torch.int64, device=dev)
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)
    commit3 = lambda: ctx.trace_commit_set_device(KIND_SKIP, sp, SHA256 | HEADER, log_blowup, cap_h, tr.data_ptr(), scaps.data_ptr(), 0)
    res = {"mode": "sha_set", "proofs": sp, "n": n, "reps": reps, "commit_ms": r4(timed(commit3, 2)), "air_sha256_header_ms": [], "prove_with_ms": []}
    for _ in range(rounds):
        res["air_sha256_header_ms"].append(r4(timed(lambda: ctx.trace_commit_set_air_sha256_device(HEADER, cap_h_.data_ptr(), cap_q.data_ptr(), 0), reps,
                                                    before=commit3)))
        shape, order = ctx.trace_commit_set_shape()
        bp = dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=0)
        proof = torch.empty(ctx.batch_layout(bp)["words"], dtype=torch.int64, device=dev)
        res["prove_with_ms"].append(r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), reps)))
        res["degree_ok"] = ctx.fri_last_degree_ok()
        kt = order.index(HEADER)
        all_caps = torch.cat([scaps[:(kt + 1) * cw], cap_h_, cap_q, scaps[(kt + 1) * cw:]])
        res["verify_ms"] = r4(timed(lambda: ctx.air_sha256_verify_device(bp, kt, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0), 3))
        res["all_ok"] = bool((ok.cpu().numpy() == 1).all())
        res.update(order=order, log_n=bp["log_n"], columns=bp["n_cols"])
        del proof
    print(json.dumps(res), flush=True)
    ctx.close()
    del tr
    torch.cuda.empty_cache()

if "sched" in modes:
    log_m, cp = int(os.environ.get("LOG_M", "16")), int(os.environ.get("SHA_PROOFS", "64"))
    log_rows, n_cols, n_h3, n_h4 = log_m - log_blowup, 9 * cp, 300 * cp, 115 * cp
    torch.manual_seed(seed)
    ctx = Context(4, b"celestia", device=0)
    table = torch.randint(0, 2**62, (n_cols << log_rows,), dtype=torch.int64, device=dev)
    pre = torch.empty(n_h4 << log_rows, dtype=torch.int64, device=dev)
    cols = torch.randint(0, 2**62, (n_cols << log_m,), dtype=torch.int64, device=dev)
    h3 = torch.randint(0, 2**62, (n_h3 << log_m,), dtype=torch.int64, device=dev)
    h4 = torch.randint(0, 2**62, (n_h4 << log_m,), dtype=torch.int64, device=dev)
    caps = []
    for c_, k_ in ((cols, n_cols), (h3, n_h3), (h4, n_h4)):
        lv = torch.empty(4 * ctx.poseidon_merkle_digests(log_m, cap_h), dtype=torch.int64, device=dev)
        ctx.poseidon_merkle_device(log_m, k_, c_.data_ptr(), cap_h, lv.data_ptr(), 0)
        caps.append(lv[-(4 << cap_h):])
    quot = torch.empty(2 << log_m, dtype=torch.int64, device=dev)
    res = {"mode": "sched", "proofs": cp, "log_m": log_m, "table_columns": n_cols, "sched_helper_columns": n_h4, "sha_helper_columns": n_h3,
           "reps": reps, "sched_helper_kernel_ms": [], "sched_quotient_call_ms": [], "sha_quotient_call_ms": []}
    for _ in range(rounds):
        res["sched_helper_kernel_ms"].append(r4(timed(lambda: ctx.air_sha256_sched_helper_device(log_rows, cp, table.data_ptr(), pre.data_ptr(), 0), reps)))
        res["sched_quotient_call_ms"].append(r4(timed(lambda: ctx.air_sha256_sched_quotient_device(
            log_m, log_blowup, cap_h, cp, cols.data_ptr(), h4.data_ptr(), caps[0].data_ptr(), caps[2].data_ptr(), quot.data_ptr(), 0), reps)))
        res["sha_quotient_call_ms"].append(r4(timed(lambda: ctx.air_sha256_quotient_device(
            log_m, log_blowup, cap_h, cp, cols.data_ptr(), h3.data_ptr(), caps[0].data_ptr(), caps[1].data_ptr(), quot.data_ptr(), 0), reps)))
    res["quotient_sha256"] = words_digest(lambda: ctx.air_sha256_sched_quotient_device(
        log_m, log_blowup, cap_h, cp, cols.data_ptr(), h4.data_ptr(), caps[0].data_ptr(), caps[2].data_ptr(), quot.data_ptr(), 0), quot)
    best = min(res["sched_quotient_call_ms"])
    res["sched_gb_per_s"] = round(((n_cols + n_h4) << log_m) * 8 / best / 1e6, 1)
    res["helper_store_gb_per_s"] = round((n_h4 << log_rows) * 8 / min(res["sched_helper_kernel_ms"]) / 1e6, 1)
    res["ns_per_point_proof"] = round(best * 1e6 / (cp << log_m), 2)
    res["ratio_sched_over_sha_call"] = round(best / min(res["sha_quotient_call_ms"]), 3)
    print(json.dumps(res), flush=True)
    ctx.close()
    del table, pre, cols, h3, h4, caps, quot
    torch.cuda.empty_cache()
    # both set-level calls on HEADER
    from tendermintx_amd.synth import bench_workload
    sp = int(os.environ.get("SHA_SET_P", "16"))
    w = bench_workload("survey8d", n, sp, seed=0x544D58)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = Context(n, b"celestia", 100800, device=0, max_batch=sp)
    out = torch.empty(sp * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
    rep = torch.empty(sp * 64, dtype=torch.uint8, device=dev)
    tr = torch.empty(sp * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(KIND_SKIP, sp, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(KIND_SKIP, sp, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    del out
    SHA256, HEADER = 4, 32
    cw = 4 << cap_h
    scaps = torch.zeros(2 * cw, dtype=torch.int64, device=dev)
    c3, c4 = torch.zeros(2 * cw, dtype=torch.int64, device=dev), torch.zeros(2 * cw, dtype=torch.int64, device=dev)
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)
    commit4 = lambda: ctx.trace_commit_set_device(KIND_SKIP, sp, SHA256 | HEADER, log_blowup, cap_h, tr.data_ptr(), scaps.data_ptr(), 0)
    air3 = lambda: ctx.trace_commit_set_air_sha256_device(HEADER, c3[:cw].data_ptr(), c3[cw:].data_ptr(), 0)
    air4 = lambda: ctx.trace_commit_set_air_sha256_sched_device(HEADER, c4[:cw].data_ptr(), c4[cw:].data_ptr(), 0)
    res = {"mode": "sched_set", "proofs": sp, "n": n, "reps": reps, "air_sha256_header_ms": [], "air_sha256_sched_header_ms": [], "prove_with_both_ms": []}
    for _ in range(rounds):
        res["air_sha256_header_ms"].append(r4(timed(air3, reps, before=commit4)))
        res["air_sha256_sched_header_ms"].append(r4(timed(air4, reps, before=commit4)))
        air3()  # (the set now holds table, H3, Q3, H4, Q4)
        shape, order = ctx.trace_commit_set_shape()
        bp = dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=0)
        proof = torch.empty(ctx.batch_layout(bp)["words"], dtype=torch.int64, device=dev)
        res["prove_with_both_ms"].append(r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), reps)))
        res["degree_ok"] = ctx.fri_last_degree_ok()
        kt = order.index(HEADER)
        all_caps = torch.cat([scaps[:(kt + 1) * cw], c3, c4, scaps[(kt + 1) * cw:]])
        res["verify_sched_ms"] = r4(timed(lambda: ctx.air_sha256_sched_verify_device(bp, kt, kt + 3, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0), 3))
        res["all_ok"] = bool((ok.cpu().numpy() == 1).all())
        ctx.air_sha256_verify_device(bp, kt, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
        res["all_ok_set3"] = bool((ok.cpu().numpy() == 1).all())
        res.update(order=order, log_n=bp["log_n"], columns=bp["n_cols"])
        del proof
    res["ratio_sched_over_sha_set_call"] = round(min(res["air_sha256_sched_header_ms"]) / min(res["air_sha256_header_ms"]), 3)
    print(json.dumps(res), flush=True)
    ctx.close()
    del tr
    torch.cuda.empty_cache()

if "init" in modes or "sets34" in modes:
    from tendermintx_amd.synth import bench_workload
    SHA256, HEADER = 4, 32
    only34 = "init" not in modes  # (the calls an older library has too)
    if not only34:
        log_m, cp, chain = int(os.environ.get("LOG_M", "16")), int(os.environ.get("SHA_PROOFS", "64")), int(os.environ.get("CHAIN", "1"))
        log_rows, n_cols, n_h3, n_h5 = log_m - log_blowup, 9 * cp, 300 * cp, 315 * cp
        torch.manual_seed(seed)
        ctx = Context(4, b"celestia", device=0)
        table = torch.randint(0, 2**62, (n_cols << log_rows,), dtype=torch.int64, device=dev)
        pre = torch.empty(n_h5 << log_rows, dtype=torch.int64, device=dev)
        cols = torch.randint(0, 2**62, (n_cols << log_m,), dtype=torch.int64, device=dev)
        h3 = torch.randint(0, 2**62, (n_h3 << log_m,), dtype=torch.int64, device=dev)
        h5 = torch.randint(0, 2**62, (n_h5 << log_m,), dtype=torch.int64, device=dev)
        caps = []
        for c_, k_ in ((cols, n_cols), (h3, n_h3), (h5, n_h5)):
            lv = torch.empty(4 * ctx.poseidon_merkle_digests(log_m, cap_h), dtype=torch.int64, device=dev)
            ctx.poseidon_merkle_device(log_m, k_, c_.data_ptr(), cap_h, lv.data_ptr(), 0)
            caps.append(lv[-(4 << cap_h):])
        quot = torch.empty(2 << log_m, dtype=torch.int64, device=dev)
        res = {"mode": "init", "proofs": cp, "log_m": log_m, "chain": chain, "table_columns": n_cols, "init_helper_columns": n_h5,
               "sha_helper_columns": n_h3, "reps": reps, "init_helper_kernel_ms": [], "init_quotient_call_ms": [], "sha_quotient_call_ms": []}
        for _ in range(rounds):
            res["init_helper_kernel_ms"].append(r4(timed(lambda: ctx.air_sha256_init_helper_device(log_rows, cp, chain, table.data_ptr(), pre.data_ptr(), 0),
                                                         reps)))
            res["init_quotient_call_ms"].append(r4(timed(lambda: ctx.air_sha256_init_quotient_device(
                log_m, log_blowup, cap_h, cp, chain, cols.data_ptr(), h5.data_ptr(), caps[0].data_ptr(), caps[2].data_ptr(), quot.data_ptr(), 0), reps)))
            res["sha_quotient_call_ms"].append(r4(timed(lambda: ctx.air_sha256_quotient_device(
                log_m, log_blowup, cap_h, cp, cols.data_ptr(), h3.data_ptr(), caps[0].data_ptr(), caps[1].data_ptr(), quot.data_ptr(), 0), reps)))
        res["quotient_sha256"] = words_digest(lambda: ctx.air_sha256_init_quotient_device(
            log_m, log_blowup, cap_h, cp, chain, cols.data_ptr(), h5.data_ptr(), caps[0].data_ptr(), caps[2].data_ptr(), quot.data_ptr(), 0), quot)
        best = min(res["init_quotient_call_ms"])
        res["init_gb_per_s"] = round(((n_cols + n_h5) << log_m) * 8 / best / 1e6, 1)
        res["helper_store_gb_per_s"] = round((n_h5 << log_rows) * 8 / min(res["init_helper_kernel_ms"]) / 1e6, 1)
        res["ns_per_point_proof"] = round(best * 1e6 / (cp << log_m), 2)
        res["ratio_init_over_sha_call"] = round(best / min(res["sha_quotient_call_ms"]), 3)
        print(json.dumps(res), flush=True)
        ctx.close()
        del table, pre, cols, h3, h5, caps, quot
        torch.cuda.empty_cache()
    # the set-level calls on HEADER
    sp = int(os.environ.get("SHA_SET_P", "16"))
    w = bench_workload("survey8d", n, sp, seed=0x544D58)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = Context(n, b"celestia", 100800, device=0, max_batch=sp)
    out = torch.empty(sp * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
    rep = torch.empty(sp * 64, dtype=torch.uint8, device=dev)
    tr = torch.empty(sp * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(KIND_SKIP, sp, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(KIND_SKIP, sp, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    del out
    cw = 4 << cap_h
    scaps = torch.zeros(2 * cw, dtype=torch.int64, device=dev)
    c3, c4, c5 = (torch.zeros(2 * cw, dtype=torch.int64, device=dev) for _ in range(3))
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)
    commit5 = lambda: ctx.trace_commit_set_device(KIND_SKIP, sp, SHA256 | HEADER, log_blowup, cap_h, tr.data_ptr(), scaps.data_ptr(), 0)
    air3 = lambda: ctx.trace_commit_set_air_sha256_device(HEADER, c3[:cw].data_ptr(), c3[cw:].data_ptr(), 0)
    air4 = lambda: ctx.trace_commit_set_air_sha256_sched_device(HEADER, c4[:cw].data_ptr(), c4[cw:].data_ptr(), 0)
    res = {"mode": "sets34" if only34 else "init_set", "proofs": sp, "n": n, "reps": reps, "air_sha256_header_ms": [], "air_sha256_sched_header_ms": []}
    if not only34:
        air5 = lambda: ctx.trace_commit_set_air_sha256_init_device(HEADER, c5[:cw].data_ptr(), c5[cw:].data_ptr(), 0)
        res.update(air_sha256_init_header_ms=[], prove_with_all_ms=[])
    for _ in range(rounds):
        res["air_sha256_header_ms"].append(r4(timed(air3, reps, before=commit5)))
        res["air_sha256_sched_header_ms"].append(r4(timed(air4, reps, before=commit5)))
        if only34:
            continue
        res["air_sha256_init_header_ms"].append(r4(timed(air5, reps, before=commit5)))
        air3()
        air4()  # (the set now holds table, H3, Q3, H4, Q4, H5, Q5)
        shape, order = ctx.trace_commit_set_shape()
        bp = dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=0)
        proof = torch.empty(ctx.batch_layout(bp)["words"], dtype=torch.int64, device=dev)
        res["prove_with_all_ms"].append(r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), reps)))
        res["degree_ok"] = ctx.fri_last_degree_ok()
        kt = order.index(HEADER)
        all_caps = torch.cat([scaps[:(kt + 1) * cw], c3, c4, c5, scaps[(kt + 1) * cw:]])
        res["verify_init_ms"] = r4(timed(lambda: ctx.air_sha256_init_verify_device(bp, kt, kt + 5, 1, all_caps.data_ptr(), proof.data_ptr(),
                                                                                  ok.data_ptr(), 0), 3))
        res["all_ok"] = bool((ok.cpu().numpy() == 1).all())
        ctx.air_sha256_sched_verify_device(bp, kt, kt + 3, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
        res["all_ok_set4"] = bool((ok.cpu().numpy() == 1).all())
        ctx.air_sha256_verify_device(bp, kt, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
        res["all_ok_set3"] = bool((ok.cpu().numpy() == 1).all())
        res.update(order=order, log_n=bp["log_n"], columns=bp["n_cols"])
        del proof
    if not only34:
        res["ratio_init_over_sha_set_call"] = round(min(res["air_sha256_init_header_ms"]) / min(res["air_sha256_header_ms"]), 3)
    print(json.dumps(res), flush=True)
    ctx.close()
    del tr
    torch.cuda.empty_cache()

if "sha_streamed" in modes:
    from tendermintx_amd.synth import bench_workload
    from tendermintx_amd.context import trace_commit_set_air_sha256_streamed_bytes
    SHA256 = 4
    sec_name = os.environ.get("SECTION", "HEADER")
    section = {"SHA256": 4, "TREE": 16, "HEADER": 32}[sec_name]
    sets, cpf = [int(x) for x in os.environ.get("SETS", "3").split(",")], int(os.environ.get("CHUNK_PROOFS", "8"))
    hcols = {3: 300, 4: 115, 5: 315}
    sp = int(os.environ.get("SHA_SET_P", "16"))
    w = bench_workload("survey8d", n, sp, seed=0x544D58)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = Context(n, b"celestia", 100800, device=0, max_batch=sp)
    out = torch.empty(sp * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
    rep = torch.empty(sp * 64, dtype=torch.uint8, device=dev)
    tr = torch.empty(sp * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(KIND_SKIP, sp, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(KIND_SKIP, sp, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    del out
    cw = 4 << cap_h
    mask = SHA256 | section
    scaps = torch.zeros((2 if mask != SHA256 else 1) * cw, dtype=torch.int64, device=dev)
    pair = {s_: torch.zeros(2 * cw, dtype=torch.int64, device=dev) for s_ in sets}
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)
    commit = lambda: ctx.trace_commit_set_device(KIND_SKIP, sp, mask, log_blowup, cap_h, tr.data_ptr(), scaps.data_ptr(), 0)
    resident = {3: ctx.trace_commit_set_air_sha256_device, 4: ctx.trace_commit_set_air_sha256_sched_device,
                5: ctx.trace_commit_set_air_sha256_init_device}

    def calls(streamed):
        for s_ in sets:
            if streamed:
                ctx.trace_commit_set_air_sha256_streamed_device(s_, section, cpf, pair[s_][:cw].data_ptr(), pair[s_][cw:].data_ptr(), 0)
            else:
                resident[s_](section, pair[s_][:cw].data_ptr(), pair[s_][cw:].data_ptr(), 0)

    digests = lambda: {str(s_): [hashlib.sha256(pair[s_][k * cw:(k + 1) * cw].cpu().numpy().tobytes()).hexdigest()[:16] for k in (0, 1)] for s_ in sets}
    commit()
    shape0, order0 = ctx.trace_commit_set_shape()
    log_m = shape0["log_n"][order0.index(section)]
    res = {"mode": "sha_streamed", "section": sec_name, "sets": sets, "proofs": sp, "n": n, "log_m": log_m, "chunk_proofs": cpf, "reps": reps,
           "bytes": {str(s_): list(trace_commit_set_air_sha256_streamed_bytes(s_, log_m, log_blowup, cap_h, sp, cpf)) for s_ in sets},
           "bytes_resident": {str(s_): list(trace_commit_set_air_sha256_streamed_bytes(s_, log_m, log_blowup, cap_h, sp, sp)) for s_ in sets}}

    def prove_and_verify():
        shape, order = ctx.trace_commit_set_shape()
        bp = dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=0)
        proof = torch.empty(ctx.batch_layout(bp)["words"], dtype=torch.int64, device=dev)
        ms = r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), reps))
        kt = order.index(section)
        caps, at = [scaps[:(kt + 1) * cw]], kt + 1
        where = {}
        for s_ in sorted(sets):
            caps.append(pair[s_])
            where[s_] = at
            at += 2
        all_caps = torch.cat(caps + [scaps[(kt + 1) * cw:]])
        verdicts = {}
        for s_, kh in where.items():
            if s_ == 3:
                ctx.air_sha256_verify_device(bp, kt, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
            elif s_ == 4:
                ctx.air_sha256_sched_verify_device(bp, kt, kh, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
            else:
                ctx.air_sha256_init_verify_device(bp, kt, kh, int(section != SHA256), all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
            verdicts[str(s_)] = bool((ok.cpu().numpy() == 1).all())
        return ms, verdicts, ctx.fri_last_degree_ok(), order

    def all_calls_ms(streamed, k):
        return r4(timed(lambda: calls(streamed), k, before=commit))

    if sec_name == "HEADER":
        res.update(resident_call_ms=[], streamed_call_ms=[], prove_resident_ms=[], prove_streamed_ms=[])
        for _ in range(rounds):
            res["resident_call_ms"].append(all_calls_ms(False, reps))
            ms, res["verdicts_resident"], _, _ = prove_and_verify()
            res["prove_resident_ms"].append(ms)
            res["caps_resident"] = digests()
            res["streamed_call_ms"].append(all_calls_ms(True, reps))
            ms, res["verdicts_streamed"], res["degree_ok"], res["order"] = prove_and_verify()
            res["prove_streamed_ms"].append(ms)
            res["caps_streamed"] = digests()
        res["caps_equal"] = res["caps_resident"] == res["caps_streamed"]
        # the chunk LDE alone: both sweeps' transforms of every set over buffers of the sizes the call uses
        log_sub = log_m - log_blowup
        big = max(hcols[s_] for s_ in sets)
        pre = torch.randint(0, 2**62, ((big * sp) << log_sub,), dtype=torch.int64, device=dev)
        chunk_buf = torch.empty((big * cpf) << log_m, dtype=torch.int64, device=dev)

        def lde_alone():
            for s_ in sets:
                for _sweep in (0, 1):
                    for p0 in range(0, sp, cpf):
                        k_ = min(cpf, sp - p0) * hcols[s_]
                        ctx.lde_device(log_sub, log_blowup, k_, pre[(p0 * hcols[s_]) << log_sub:].data_ptr(), chunk_buf.data_ptr(), 0)

        res["chunk_lde_two_sweeps_ms"] = [r4(timed(lde_alone, reps)) for _ in range(rounds)]
        best_s, best_r = min(res["streamed_call_ms"]), min(res["resident_call_ms"])
        res["ratio_streamed_over_resident_call"] = round(best_s / best_r, 3)
        res["ratio_streamed_over_resident_prove"] = round(min(res["prove_streamed_ms"]) / min(res["prove_resident_ms"]), 3)
        res["helper_lde_share_of_streamed"] = round(min(res["chunk_lde_two_sweeps_ms"]) / best_s, 3)
        del pre, chunk_buf
    else:
        res["free_before_mib"] = torch.cuda.mem_get_info(dev)[0] >> 20
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        calls(True)
        b.record()
        torch.cuda.synchronize(dev)
        res["streamed_call_ms"] = r4(a.elapsed_time(b))
        res["free_after_mib"] = torch.cuda.mem_get_info(dev)[0] >> 20
        res["caps_streamed"] = digests()
        res["prove_streamed_ms"], res["verdicts_streamed"], res["degree_ok"], res["order"] = prove_and_verify()
    print(json.dumps(res), flush=True)
    ctx.close()
    del tr
    torch.cuda.empty_cache()

if "set2" in modes:
    from tendermintx_amd.synth import bench_workload
    w = bench_workload("survey8d", n, P, seed=0x544D58)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = Context(n, b"celestia", 100800, device=0, max_batch=P)
    out = torch.empty(P * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
    rep = torch.empty(P * 64, dtype=torch.uint8, device=dev)
    tr = torch.empty(P * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(KIND_SKIP, P, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(KIND_SKIP, P, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    ALL, LADDERS = 1 | 2 | 4 | 16 | 32, 1
    log_k, pub_cols = ctx.air_ladder_public_shape(KIND_SKIP, P)
    pub = torch.empty(pub_cols << log_k, dtype=torch.int64, device=dev)
    caps = torch.zeros(5 * (4 << cap_h), dtype=torch.int64, device=dev)
    cap_q = torch.zeros(4 << cap_h, dtype=torch.int64, device=dev)
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)

    def commit2(streamed):
        if streamed:
            ctx.trace_commit_set_streamed_device(KIND_SKIP, P, ALL, LADDERS, chunk, log_blowup, cap_h, tr.data_ptr(), caps.data_ptr(), 0)
        else:
            ctx.trace_commit_set_device(KIND_SKIP, P, ALL, log_blowup, cap_h, tr.data_ptr(), caps.data_ptr(), 0)

    air1 = lambda: ctx.trace_commit_set_air_device(cap_q.data_ptr(), 0)
    air2 = lambda: ctx.trace_commit_set_air_boundary_device(pub.data_ptr(), cap_q.data_ptr(), 0)
    res = {"mode": "set2", "proofs": P, "n": n, "chunk_cols": chunk, "reps": reps, "log_k": log_k, "public_columns": pub_cols,
           "gather_ms": r4(timed(lambda: ctx.air_ladder_public_device(KIND_SKIP, P, out.data_ptr(), pub.data_ptr(), 0), reps)),
           "set1_resident_ms": [], "set2_resident_ms": [], "set1_streamed_ms": [], "set2_streamed_ms": [], "prove_with_set2_ms": []}
    for _ in range(rounds):
        res["set1_resident_ms"].append(r4(timed(air1, reps, before=lambda: commit2(False))))
        res["set2_resident_ms"].append(r4(timed(air2, reps, before=lambda: commit2(False))))
        shape, order = ctx.trace_commit_set_shape()
        bp = dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=0)
        proof = torch.empty(ctx.batch_layout(bp)["words"], dtype=torch.int64, device=dev)
        res["prove_with_set2_ms"].append(r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), reps)))
        res["degree_ok"] = ctx.fri_last_degree_ok()
        kt, cw = order.index(LADDERS), 4 << cap_h
        all_caps = torch.cat([caps[:(kt + 1) * cw], cap_q, caps[(kt + 1) * cw:]])
        res["verify_set2_ms"] = r4(timed(lambda: ctx.air_boundary_verify_device(bp, kt, all_caps.data_ptr(), proof.data_ptr(), pub.data_ptr(),
                                                                                ok.data_ptr(), 0), 3))
        res["all_ok"] = bool((ok.cpu().numpy() == 1).all())
        keep = cap_q.clone()
        res["set1_streamed_ms"].append(r4(timed(air1, reps, before=lambda: commit2(True))))
        res["set2_streamed_ms"].append(r4(timed(air2, reps, before=lambda: commit2(True))))
        res["streamed_cap_equal"] = bool(torch.equal(keep, cap_q))
        del proof
    res["ratio_set2_over_set1_resident"] = round(min(res["set2_resident_ms"]) / min(res["set1_resident_ms"]), 3)
    res["ratio_set2_over_set1_streamed"] = round(min(res["set2_streamed_ms"]) / min(res["set1_streamed_ms"]), 3)
    print(json.dumps(res), flush=True)
    ctx.close()
    del out, tr, pub
    torch.cuda.empty_cache()

if "set" in modes or "set_plain" in modes:
    from tendermintx_amd.synth import bench_workload
    plain = "set_plain" in modes
    w = bench_workload("survey8d", n, P, seed=0x544D58)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = Context(n, b"celestia", 100800, device=0, max_batch=P)
    out = torch.empty(P * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
    rep = torch.empty(P * 64, dtype=torch.uint8, device=dev)
    tr = torch.empty(P * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(KIND_SKIP, P, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(KIND_SKIP, P, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    del out
    ALL, LADDERS = 1 | 2 | 4 | 16 | 32, 1
    caps = torch.zeros(5 * (4 << cap_h), dtype=torch.int64, device=dev)
    cap_q = torch.zeros(4 << cap_h, dtype=torch.int64, device=dev)
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)

    def commit(streamed):
        if streamed:
            ctx.trace_commit_set_streamed_device(KIND_SKIP, P, ALL, LADDERS, chunk, log_blowup, cap_h, tr.data_ptr(), caps.data_ptr(), 0)
        else:
            ctx.trace_commit_set_device(KIND_SKIP, P, ALL, log_blowup, cap_h, tr.data_ptr(), caps.data_ptr(), 0)

    def params():
        shape, order = ctx.trace_commit_set_shape()
        return dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=0), order

    def prove_ms():
        bp, _ = params()
        proof = torch.empty(ctx.batch_layout(bp)["words"], dtype=torch.int64, device=dev)
        return r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), reps)), bp, proof

    res = {"mode": "set_plain" if plain else "set", "proofs": P, "n": n, "chunk_cols": chunk, "reps": reps}
    if plain:
        res["commit_ms"] = r4(timed(lambda: commit(False), 2))
        res["prove_ms"] = [prove_ms()[0] for _ in range(rounds)]
    else:
        res.update(prove_without_ms=[], prove_with_ms=[], air_resident_ms=[], air_streamed_ms=[])
        for _ in range(rounds):
            commit(False)
            res["prove_without_ms"].append(prove_ms()[0])
            res["air_resident_ms"].append(r4(timed(lambda: ctx.trace_commit_set_air_device(cap_q.data_ptr(), 0), reps, before=lambda: commit(False))))
            ms, bp, proof = prove_ms()
            res["prove_with_ms"].append(ms)
            res["degree_ok"] = ctx.fri_last_degree_ok()
            kt = params()[1].index(LADDERS)
            cw = 4 << cap_h
            all_caps = torch.cat([caps[:(kt + 1) * cw], cap_q, caps[(kt + 1) * cw:]])
            res["verify_ms"] = r4(timed(lambda: ctx.air_verify_device(bp, kt, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0), 3))
            res["all_ok"] = bool((ok.cpu().numpy() == 1).all())
            keep = cap_q.clone()
            res["air_streamed_ms"].append(r4(timed(lambda: ctx.trace_commit_set_air_device(cap_q.data_ptr(), 0), reps, before=lambda: commit(True))))
            res["streamed_cap_equal"] = bool(torch.equal(keep, cap_q))
            del proof
        res.update(order=params()[1], log_n=bp["log_n"], columns=bp["n_cols"])
        res["re_lde_share_of_streamed"] = round(1 - min(res["air_resident_ms"]) / min(res["air_streamed_ms"]), 3)
    print(json.dumps(res), flush=True)
    ctx.close()

if "link" in modes:
    from tendermintx_amd.synth import bench_workload
    SHA256_T, TREE_T, HEADER_T = 4, 16, 32
    w = bench_workload("survey8d", n, P, seed=0x544D58)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = Context(n, b"celestia", 100800, device=0, max_batch=P)
    out = torch.empty(P * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
    rep = torch.empty(P * 64, dtype=torch.uint8, device=dev)
    ctx.witness_batch_device(KIND_SKIP, P, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    torch.cuda.synchronize(dev)
    res = {"mode": "link", "proofs": P, "n": n, "reps": reps, "gather_ms": {}, "public_words": {}}
    for name, sec in (("sha256", SHA256_T), ("tree", TREE_T), ("header", HEADER_T)):
        log_k, pub_cols = ctx.air_sha256_public_shape(KIND_SKIP, sec, P)
        pub = torch.empty(pub_cols << log_k, dtype=torch.int64, device=dev)
        res["gather_ms"][name] = r4(timed(lambda: ctx.air_sha256_public_device(KIND_SKIP, sec, P, out.data_ptr(), pub.data_ptr(), 0), reps))
        res["public_words"][name] = pub_cols << log_k
    # the set-level call on HEADER (pub is HEADER's table now) beside set 5's on the same set, alternating; the prove and both verifiers
    tr = torch.empty(P * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
    ctx.trace_rows_device(KIND_SKIP, P, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    cw = 4 << cap_h
    scaps, c5, c6 = (torch.zeros(2 * cw, dtype=torch.int64, device=dev) for _ in range(3))
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)
    hpub = pub
    commit6 = lambda: ctx.trace_commit_set_device(KIND_SKIP, P, SHA256_T | HEADER_T, log_blowup, cap_h, tr.data_ptr(), scaps.data_ptr(), 0)
    air5 = lambda: ctx.trace_commit_set_air_sha256_init_device(HEADER_T, c5[:cw].data_ptr(), c5[cw:].data_ptr(), 0)
    air6 = lambda: ctx.trace_commit_set_air_sha256_link_device(HEADER_T, hpub.data_ptr(), c6[:cw].data_ptr(), c6[cw:].data_ptr(), 0)
    res.update(air_sha256_link_header_ms=[], air_sha256_init_header_ms=[], prove_with_sets_5_6_ms=[])
    for _ in range(rounds):
        res["air_sha256_link_header_ms"].append(r4(timed(air6, reps, before=commit6)))
        res["air_sha256_init_header_ms"].append(r4(timed(air5, reps, before=commit6)))
        air6()  # (the set now holds table, H5, Q5, H6, Q6)
        shape, order = ctx.trace_commit_set_shape()
        bp = dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=0)
        proof = torch.empty(ctx.batch_layout(bp)["words"], dtype=torch.int64, device=dev)
        res["prove_with_sets_5_6_ms"].append(r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), reps)))
        res["degree_ok"] = ctx.fri_last_degree_ok()
        kt = order.index(HEADER_T)
        all_caps = torch.cat([scaps[:(kt + 1) * cw], c5, c6, scaps[(kt + 1) * cw:]])
        res["verify_link_ms"] = r4(timed(lambda: ctx.air_sha256_link_verify_device(bp, kt, kt + 3, all_caps.data_ptr(), proof.data_ptr(), hpub.data_ptr(),
                                                                                  ok.data_ptr(), 0), 3))
        res["all_ok"] = bool((ok.cpu().numpy() == 1).all())
        ctx.air_sha256_init_verify_device(bp, kt, kt + 1, 1, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
        res["all_ok_set5"] = bool((ok.cpu().numpy() == 1).all())
        res.update(order=order, log_n=bp["log_n"], columns=bp["n_cols"])
        del proof
    del tr
    log_rows, sp_ = int(os.environ.get("LOG_ROWS", "13")), int(os.environ.get("SHA_PROOFS", "64"))
    g = torch.Generator(device=dev).manual_seed(seed)
    table = torch.randint(0, 2**62, ((9 * sp_) << log_rows,), dtype=torch.int64, device=dev, generator=g)
    pub = torch.randint(0, 2, ((26 * sp_) << (log_rows - 6),), dtype=torch.int64, device=dev, generator=g)
    helper = torch.empty((33 * sp_) << log_rows, dtype=torch.int64, device=dev)
    call = lambda: ctx.air_sha256_link_helper_device(log_rows, sp_, table.data_ptr(), pub.data_ptr(), helper.data_ptr(), 0)
    res.update(helper_proofs=sp_, helper_log_rows=log_rows, helper_ms=[r4(timed(call, reps)) for _ in range(rounds)])
    res["helper_gb_per_s"] = round((33 + 8) * sp_ * 8 * 2**log_rows / min(res["helper_ms"]) / 1e6, 1)
    res["link_helper_sha256"] = words_digest(call, helper)
    # the quotient call (digest, gamma, tables, the public side, k_air_link_quotient) over random extended columns, beside a plain FRI prove
    # over the SAME helper columns: its combine stage is k_fri_combine over 33 of the 50 columns the pass reads per proof
    log_m = log_rows + log_blowup
    cols = torch.randint(0, 2**62, ((9 * sp_) << log_m,), dtype=torch.int64, device=dev, generator=g)
    hcols = torch.randint(0, 2**62, ((33 * sp_) << log_m,), dtype=torch.int64, device=dev, generator=g)
    caps = []
    for c_, k_ in ((cols, 9 * sp_), (hcols, 33 * sp_)):
        lv = torch.empty(4 * ctx.poseidon_merkle_digests(log_m, cap_h), dtype=torch.int64, device=dev)
        ctx.poseidon_merkle_device(log_m, k_, c_.data_ptr(), cap_h, lv.data_ptr(), 0)
        caps.append(lv)
    quot = torch.empty(2 << log_m, dtype=torch.int64, device=dev)
    qcall = lambda: ctx.air_sha256_link_quotient_device(log_m, log_blowup, cap_h, sp_, cols.data_ptr(), hcols.data_ptr(), caps[0][-(4 << cap_h):].data_ptr(),
                                                        caps[1][-(4 << cap_h):].data_ptr(), pub.data_ptr(), quot.data_ptr(), 0)
    fp = dict(log_n=log_m, n_cols=33 * sp_, cap_height=cap_h, log_blowup=log_blowup, arity_bits=arity, final_log_max=final_max, n_queries=nq)
    proof = torch.empty(ctx.fri_layout(fp)["words"], dtype=torch.int64, device=dev)
    res.update(log_m=log_m, link_quotient_call_ms=[], fri_prove_helper_ms=[], fri_combine_stage_ms=[])
    for _ in range(rounds):
        res["link_quotient_call_ms"].append(r4(timed(qcall, reps)))
        res["fri_prove_helper_ms"].append(r4(timed(lambda: ctx.fri_prove_device(fp, hcols.data_ptr(), caps[1].data_ptr(), proof.data_ptr(), 0), reps)))
        res["fri_combine_stage_ms"].append(r4(ctx.fri_last_ms()["combine"]))
    res["quotient_read_gib"] = round((50 * sp_ << log_m) * 8 / 2**30, 2)
    res["combine_read_gib"] = round((33 * sp_ << log_m) * 8 / 2**30, 2)
    res["quotient_sha256"] = words_digest(qcall, quot)
    print(json.dumps(res), flush=True)
    ctx.close()

if "sha512" in modes:
    # constraint set 7 beside set 3, its yardstick: the helper kernel, the caller-level quotient call of each set over random extended columns
    # (S512_PROOFS proofs of 18 + 599 columns against SHA_PROOFS proofs of 9 + 300, M = 2^LOG_M each) and a plain FRI prove over set 7's table
    # columns, alternating -- under `rocprofv3 --kernel-trace --stats` (MODE=sha512) k_air_sha512_helper, k_air_sha512_quotient<Sha512Round, FORM>,
    # k_air_sha_quotient and k_fri_combine show in ONE trace.  ns_per_helper_word: the call's time per helper word read, the figure the two
    # passes are compared on.  Then the set-level call on SHA512 of a set SHA512 | HEADER of S512_SET_P proofs at N = n.
    log_m, cp, cp3 = int(os.environ.get("LOG_M", "16")), int(os.environ.get("S512_PROOFS", "16")), int(os.environ.get("SHA_PROOFS", "32"))
    log_rows = log_m - log_blowup
    torch.manual_seed(seed)
    ctx = Context(4, b"celestia", device=0)

    def columns(width, helper, proofs):
        cols = torch.randint(0, 2**62, ((width * proofs) << log_m,), dtype=torch.int64, device=dev)
        hcols = torch.randint(0, 2**62, ((helper * proofs) << log_m,), dtype=torch.int64, device=dev)
        caps = []
        for c_, k_ in ((cols, width * proofs), (hcols, helper * proofs)):
            lv = torch.empty(4 * ctx.poseidon_merkle_digests(log_m, cap_h), dtype=torch.int64, device=dev)
            ctx.poseidon_merkle_device(log_m, k_, c_.data_ptr(), cap_h, lv.data_ptr(), 0)
            caps.append(lv)
        return cols, hcols, caps

    cols7, hcols7, caps7 = columns(18, 599, cp)
    cols3, hcols3, caps3 = columns(9, 300, cp3)
    table = torch.randint(0, 2**62, ((18 * cp) << log_rows,), dtype=torch.int64, device=dev)
    pre = torch.empty((599 * cp) << log_rows, dtype=torch.int64, device=dev)
    quot = torch.empty(2 << log_m, dtype=torch.int64, device=dev)
    fp = dict(log_n=log_m, n_cols=18 * cp, cap_height=cap_h, log_blowup=log_blowup, arity_bits=arity, final_log_max=final_max, n_queries=nq)
    proof = torch.empty(ctx.fri_layout(fp)["words"], dtype=torch.int64, device=dev)
    q7 = lambda: ctx.air_sha512_quotient_device(log_m, log_blowup, cap_h, cp, cols7.data_ptr(), hcols7.data_ptr(), caps7[0][-(4 << cap_h):].data_ptr(),
                                                caps7[1][-(4 << cap_h):].data_ptr(), quot.data_ptr(), 0)
    q3 = lambda: ctx.air_sha256_quotient_device(log_m, log_blowup, cap_h, cp3, cols3.data_ptr(), hcols3.data_ptr(), caps3[0][-(4 << cap_h):].data_ptr(),
                                                caps3[1][-(4 << cap_h):].data_ptr(), quot.data_ptr(), 0)
    res = {"mode": "sha512", "log_m": log_m, "proofs_set7": cp, "proofs_set3": cp3, "read_gib_set7": round(((617 * cp) << log_m) * 8 / 2**30, 2),
           "read_gib_set3": round(((309 * cp3) << log_m) * 8 / 2**30, 2), "reps": reps, "helper_kernel_ms": [], "sha512_quotient_call_ms": [],
           "sha256_quotient_call_ms": [], "fri_prove_table_ms": [], "fri_combine_stage_ms": []}
    for _ in range(rounds):
        res["helper_kernel_ms"].append(r4(timed(lambda: ctx.air_sha512_helper_device(log_rows, cp, table.data_ptr(), pre.data_ptr(), 0), reps)))
        res["sha512_quotient_call_ms"].append(r4(timed(q7, reps)))
        res["sha256_quotient_call_ms"].append(r4(timed(q3, reps)))
        res["fri_prove_table_ms"].append(r4(timed(lambda: ctx.fri_prove_device(fp, cols7.data_ptr(), caps7[0].data_ptr(), proof.data_ptr(), 0), reps)))
        res["fri_combine_stage_ms"].append(r4(ctx.fri_last_ms()["combine"]))
    res["quotient_sha256"] = words_digest(q7, quot)
    ns7 = min(res["sha512_quotient_call_ms"]) * 1e6 / ((599 * cp) << log_m)
    ns3 = min(res["sha256_quotient_call_ms"]) * 1e6 / ((300 * cp3) << log_m)
    res.update(ns_per_helper_word_set7=round(ns7, 4), ns_per_helper_word_set3=round(ns3, 4), ratio_set7_over_set3=round(ns7 / ns3, 3),
               helper_store_gb_per_s=round(((599 * cp) << log_rows) * 8 / min(res["helper_kernel_ms"]) / 1e6, 1))
    print(json.dumps(res), flush=True)
    ctx.close()
    del cols7, hcols7, caps7, cols3, hcols3, caps3, table, pre, quot, proof
    torch.cuda.empty_cache()
    # the set-level call on SHA512
    from tendermintx_amd.synth import bench_workload
    sp = int(os.environ.get("S512_SET_P", "16"))
    w = bench_workload("survey8d", n, sp, seed=0x544D58)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = Context(n, b"celestia", 100800, device=0, max_batch=sp)
    out = torch.empty(sp * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
    rep = torch.empty(sp * 64, dtype=torch.uint8, device=dev)
    tr = torch.empty(sp * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(KIND_SKIP, sp, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(KIND_SKIP, sp, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    del out
    SHA512, HEADER = 2, 32
    cw = 4 << cap_h
    scaps, cap_h_, cap_q = (torch.zeros(k * cw, dtype=torch.int64, device=dev) for k in (2, 1, 1))
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)
    commit = lambda: ctx.trace_commit_set_device(KIND_SKIP, sp, SHA512 | HEADER, log_blowup, cap_h, tr.data_ptr(), scaps.data_ptr(), 0)
    res = {"mode": "sha512_set", "proofs": sp, "n": n, "reps": reps, "commit_ms": r4(timed(commit, 2)), "air_sha512_ms": [], "prove_with_ms": []}
    for _ in range(rounds):
        res["air_sha512_ms"].append(r4(timed(lambda: ctx.trace_commit_set_air_sha512_device(SHA512, cap_h_.data_ptr(), cap_q.data_ptr(), 0), reps,
                                             before=commit)))
        shape, order = ctx.trace_commit_set_shape()
        bp = dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=0)
        proof = torch.empty(ctx.batch_layout(bp)["words"], dtype=torch.int64, device=dev)
        res["prove_with_ms"].append(r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), reps)))
        res["degree_ok"] = ctx.fri_last_degree_ok()
        kt = order.index(SHA512)
        all_caps = torch.cat([scaps[:(kt + 1) * cw], cap_h_, cap_q, scaps[(kt + 1) * cw:]])
        res["verify_ms"] = r4(timed(lambda: ctx.air_sha512_verify_device(bp, kt, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0), 3))
        res["all_ok"] = bool((ok.cpu().numpy() == 1).all())
        res.update(order=order, log_n=bp["log_n"], columns=bp["n_cols"])
        del proof
    print(json.dumps(res), flush=True)
    ctx.close()

if "sha512_sched" in modes:
    # constraint set 8 beside set 4, its yardstick: the helper kernel, then the caller-level quotient call of each set over random extended
    # columns (S512_PROOFS proofs of 18 + 230 columns against SCHED_PROOFS proofs of 9 + 115, M = 2^LOG_M each: an equal count of words read),
    # alternating -- under `rocprofv3 --kernel-trace --stats` (MODE=sha512_sched) k_air_sha512_sched_helper, k_air_sha512_quotient<Sha512Sched, FORM> and
    # k_air_sched_quotient show in ONE trace.  ps_per_helper_word: the call's time per helper word read, the figure the two passes are
    # compared on.  Then the set-level call of set 8 on SHA512 of a set SHA512 | HEADER of S512_SET_P proofs at N = n.
    log_m, cp, cp4 = int(os.environ.get("LOG_M", "16")), int(os.environ.get("S512_PROOFS", "16")), int(os.environ.get("SCHED_PROOFS", "32"))
    log_rows = log_m - log_blowup
    torch.manual_seed(seed)
    ctx = Context(4, b"celestia", device=0)

    def columns(width, helper, proofs):
        cols = torch.randint(0, 2**62, ((width * proofs) << log_m,), dtype=torch.int64, device=dev)
        hcols = torch.randint(0, 2**62, ((helper * proofs) << log_m,), dtype=torch.int64, device=dev)
        caps = []
        for c_, k_ in ((cols, width * proofs), (hcols, helper * proofs)):
            lv = torch.empty(4 * ctx.poseidon_merkle_digests(log_m, cap_h), dtype=torch.int64, device=dev)
            ctx.poseidon_merkle_device(log_m, k_, c_.data_ptr(), cap_h, lv.data_ptr(), 0)
            caps.append(lv)
        return cols, hcols, caps

    cols8, hcols8, caps8 = columns(18, 230, cp)
    cols4, hcols4, caps4 = columns(9, 115, cp4)
    table = torch.randint(0, 2**62, ((18 * cp) << log_rows,), dtype=torch.int64, device=dev)
    pre = torch.empty((230 * cp) << log_rows, dtype=torch.int64, device=dev)
    quot = torch.empty(2 << log_m, dtype=torch.int64, device=dev)
    q8 = lambda: ctx.air_sha512_sched_quotient_device(log_m, log_blowup, cap_h, cp, cols8.data_ptr(), hcols8.data_ptr(),
                                                      caps8[0][-(4 << cap_h):].data_ptr(), caps8[1][-(4 << cap_h):].data_ptr(), quot.data_ptr(), 0)
    q4 = lambda: ctx.air_sha256_sched_quotient_device(log_m, log_blowup, cap_h, cp4, cols4.data_ptr(), hcols4.data_ptr(),
                                                      caps4[0][-(4 << cap_h):].data_ptr(), caps4[1][-(4 << cap_h):].data_ptr(), quot.data_ptr(), 0)
    res = {"mode": "sha512_sched", "log_m": log_m, "proofs_set8": cp, "proofs_set4": cp4, "read_gib_set8": round(((232 * cp) << log_m) * 8 / 2**30, 2),
           "read_gib_set4": round(((116 * cp4) << log_m) * 8 / 2**30, 2), "reps": reps, "helper_kernel_ms": [], "sha512_sched_quotient_call_ms": [],
           "sha256_sched_quotient_call_ms": []}
    for _ in range(rounds):
        res["helper_kernel_ms"].append(r4(timed(lambda: ctx.air_sha512_sched_helper_device(log_rows, cp, table.data_ptr(), pre.data_ptr(), 0), reps)))
        res["sha512_sched_quotient_call_ms"].append(r4(timed(q8, reps)))
        res["sha256_sched_quotient_call_ms"].append(r4(timed(q4, reps)))
    res["quotient_sha256"] = words_digest(q8, quot)
    ps8 = min(res["sha512_sched_quotient_call_ms"]) * 1e9 / ((230 * cp) << log_m)
    ps4 = min(res["sha256_sched_quotient_call_ms"]) * 1e9 / ((115 * cp4) << log_m)
    res.update(ps_per_helper_word_set8=round(ps8, 2), ps_per_helper_word_set4=round(ps4, 2), ratio_set8_over_set4=round(ps8 / ps4, 3),
               helper_store_gb_per_s=round(((230 * cp) << log_rows) * 8 / min(res["helper_kernel_ms"]) / 1e6, 1))
    print(json.dumps(res), flush=True)
    ctx.close()
    del cols8, hcols8, caps8, cols4, hcols4, caps4, table, pre, quot
    torch.cuda.empty_cache()
    # the set-level call of set 8 on SHA512
    from tendermintx_amd.synth import bench_workload
    sp = int(os.environ.get("S512_SET_P", "16"))
    w = bench_workload("survey8d", n, sp, seed=0x544D58)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = Context(n, b"celestia", 100800, device=0, max_batch=sp)
    out = torch.empty(sp * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
    rep = torch.empty(sp * 64, dtype=torch.uint8, device=dev)
    tr = torch.empty(sp * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(KIND_SKIP, sp, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(KIND_SKIP, sp, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    del out
    SHA512, HEADER = 2, 32
    cw = 4 << cap_h
    scaps, cap_h_, cap_q = (torch.zeros(k * cw, dtype=torch.int64, device=dev) for k in (2, 1, 1))
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)
    commit = lambda: ctx.trace_commit_set_device(KIND_SKIP, sp, SHA512 | HEADER, log_blowup, cap_h, tr.data_ptr(), scaps.data_ptr(), 0)
    res = {"mode": "sha512_sched_set", "proofs": sp, "n": n, "reps": reps, "commit_ms": r4(timed(commit, 2)), "air_sha512_sched_ms": [], "prove_with_ms": []}
    for _ in range(rounds):
        res["air_sha512_sched_ms"].append(r4(timed(lambda: ctx.trace_commit_set_air_sha512_sched_device(SHA512, cap_h_.data_ptr(), cap_q.data_ptr(), 0),
                                                   reps, before=commit)))
        shape, order = ctx.trace_commit_set_shape()
        bp = dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=0)
        proof = torch.empty(ctx.batch_layout(bp)["words"], dtype=torch.int64, device=dev)
        res["prove_with_ms"].append(r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), reps)))
        res["degree_ok"] = ctx.fri_last_degree_ok()
        kt = order.index(SHA512)
        all_caps = torch.cat([scaps[:(kt + 1) * cw], cap_h_, cap_q, scaps[(kt + 1) * cw:]])
        res["verify_ms"] = r4(timed(lambda: ctx.air_sha512_sched_verify_device(bp, kt, kt + 1, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0), 3))
        res["all_ok"] = bool((ok.cpu().numpy() == 1).all())
        res.update(order=order, log_n=bp["log_n"], columns=bp["n_cols"])
        del proof
    print(json.dumps(res), flush=True)
    ctx.close()

if "sha512_init" in modes:
    # constraint set 9 beside set 7, its yardstick: the helper kernel, then the caller-level quotient call of each set over random extended
    # columns (S512_PROOFS proofs of the SAME 18 table columns, 629 against 599 helper columns, M = 2^LOG_M), alternating in one process --
    # under `rocprofv3 --kernel-trace --stats` (MODE=sha512_init) k_air_sha512_init_helper, k_air_sha512_quotient<Sha512Init, FORM> and
    # k_air_sha512_quotient<Sha512Round, FORM> show in ONE trace.  ps_per_helper_word: the call's time per helper word read, the figure the two passes are
    # compared on.  Then the set-level call of set 9 on SHA512 of a set SHA512 | HEADER of S512_SET_P proofs at N = n.
    log_m, cp = int(os.environ.get("LOG_M", "16")), int(os.environ.get("S512_PROOFS", "16"))
    log_rows = log_m - log_blowup
    torch.manual_seed(seed)
    ctx = Context(4, b"celestia", device=0)

    def capped(words, k_):
        c_ = torch.randint(0, 2**62, (words,), dtype=torch.int64, device=dev)
        lv = torch.empty(4 * ctx.poseidon_merkle_digests(log_m, cap_h), dtype=torch.int64, device=dev)
        ctx.poseidon_merkle_device(log_m, k_, c_.data_ptr(), cap_h, lv.data_ptr(), 0)
        return c_, lv[-(4 << cap_h):]

    cols, cap_t = capped((18 * cp) << log_m, 18 * cp)
    hcols9, cap9 = capped((629 * cp) << log_m, 629 * cp)
    hcols7, cap7 = capped((599 * cp) << log_m, 599 * cp)
    table = torch.randint(0, 2**62, ((18 * cp) << log_rows,), dtype=torch.int64, device=dev)
    pre = torch.empty((629 * cp) << log_rows, dtype=torch.int64, device=dev)
    quot = torch.empty(2 << log_m, dtype=torch.int64, device=dev)
    q9 = lambda: ctx.air_sha512_init_quotient_device(log_m, log_blowup, cap_h, cp, cols.data_ptr(), hcols9.data_ptr(), cap_t.data_ptr(),
                                                     cap9.data_ptr(), quot.data_ptr(), 0)
    q7 = lambda: ctx.air_sha512_quotient_device(log_m, log_blowup, cap_h, cp, cols.data_ptr(), hcols7.data_ptr(), cap_t.data_ptr(),
                                                cap7.data_ptr(), quot.data_ptr(), 0)
    res = {"mode": "sha512_init", "log_m": log_m, "proofs": cp, "read_gib_set9": round(((647 * cp) << log_m) * 8 / 2**30, 2),
           "read_gib_set7": round(((617 * cp) << log_m) * 8 / 2**30, 2), "reps": reps, "helper_kernel_ms": [], "sha512_init_quotient_call_ms": [],
           "sha512_quotient_call_ms": []}
    for _ in range(rounds):
        res["helper_kernel_ms"].append(r4(timed(lambda: ctx.air_sha512_init_helper_device(log_rows, cp, table.data_ptr(), pre.data_ptr(), 0), reps)))
        res["sha512_init_quotient_call_ms"].append(r4(timed(q9, reps)))
        res["sha512_quotient_call_ms"].append(r4(timed(q7, reps)))
    res["quotient_sha256"] = words_digest(q9, quot)
    ps9 = min(res["sha512_init_quotient_call_ms"]) * 1e9 / ((629 * cp) << log_m)
    ps7 = min(res["sha512_quotient_call_ms"]) * 1e9 / ((599 * cp) << log_m)
    res.update(ps_per_helper_word_set9=round(ps9, 2), ps_per_helper_word_set7=round(ps7, 2), ratio_set9_over_set7=round(ps9 / ps7, 3),
               helper_rows=1 << log_rows, helper_store_tb_per_s=round(((629 * cp) << log_rows) * 8 / min(res["helper_kernel_ms"]) / 1e9, 3))
    print(json.dumps(res), flush=True)
    ctx.close()
    del cols, cap_t, hcols9, cap9, hcols7, cap7, table, pre, quot
    torch.cuda.empty_cache()
    # the set-level call of set 9 on SHA512
    from tendermintx_amd.synth import bench_workload
    sp = int(os.environ.get("S512_SET_P", "16"))
    w = bench_workload("survey8d", n, sp, seed=0x544D58)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = Context(n, b"celestia", 100800, device=0, max_batch=sp)
    out = torch.empty(sp * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
    rep = torch.empty(sp * 64, dtype=torch.uint8, device=dev)
    tr = torch.empty(sp * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(KIND_SKIP, sp, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(KIND_SKIP, sp, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    del out
    SHA512, HEADER = 2, 32
    cw = 4 << cap_h
    scaps, cap_h_, cap_q = (torch.zeros(k * cw, dtype=torch.int64, device=dev) for k in (2, 1, 1))
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)
    commit = lambda: ctx.trace_commit_set_device(KIND_SKIP, sp, SHA512 | HEADER, log_blowup, cap_h, tr.data_ptr(), scaps.data_ptr(), 0)
    res = {"mode": "sha512_init_set", "proofs": sp, "n": n, "reps": reps, "commit_ms": r4(timed(commit, 2)), "air_sha512_init_ms": [], "prove_with_ms": []}
    for _ in range(rounds):
        res["air_sha512_init_ms"].append(r4(timed(lambda: ctx.trace_commit_set_air_sha512_init_device(SHA512, cap_h_.data_ptr(), cap_q.data_ptr(), 0),
                                                  reps, before=commit)))
        shape, order = ctx.trace_commit_set_shape()
        bp = dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=0)
        proof = torch.empty(ctx.batch_layout(bp)["words"], dtype=torch.int64, device=dev)
        res["prove_with_ms"].append(r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), reps)))
        res["degree_ok"] = ctx.fri_last_degree_ok()
        kt = order.index(SHA512)
        all_caps = torch.cat([scaps[:(kt + 1) * cw], cap_h_, cap_q, scaps[(kt + 1) * cw:]])
        res["verify_ms"] = r4(timed(lambda: ctx.air_sha512_init_verify_device(bp, kt, kt + 1, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0), 3))
        res["all_ok"] = bool((ok.cpu().numpy() == 1).all())
        res.update(order=order, log_n=bp["log_n"], columns=bp["n_cols"])
        del proof
    print(json.dumps(res), flush=True)
    ctx.close()
    del tr  # (given back so that a mode chained behind this one, such as sha512_streamed, starts from the memory it reports as free)
    torch.cuda.empty_cache()

if "sha512_link" in modes:
    # constraint set 10 beside its two siblings: set 6 (the same kind of statement on the SHA-256 tables) and set 8 (the lightest pass of
    # the shared k_air_sha512_quotient frame), caller-level calls over random extended columns at the same M, alternating in one process.
    # ps_per_word: the call's time per column word read (table + helper), the figure the passes are compared on.
    log_m, cp = int(os.environ.get("LOG_M", "16")), int(os.environ.get("S512_PROOFS", "16"))
    log_rows = log_m - log_blowup
    torch.manual_seed(seed)
    ctx = Context(4, b"celestia", device=0)

    def capped(words, k_):
        c_ = torch.randint(0, 2**62, (words,), dtype=torch.int64, device=dev)
        lv = torch.empty(4 * ctx.poseidon_merkle_digests(log_m, cap_h), dtype=torch.int64, device=dev)
        ctx.poseidon_merkle_device(log_m, k_, c_.data_ptr(), cap_h, lv.data_ptr(), 0)
        return c_, lv[-(4 << cap_h):]

    log_k10 = (-(-(1 << log_rows) // 80) - 1).bit_length()
    cols, cap_t = capped((18 * cp) << log_m, 18 * cp)
    cols6, cap_t6 = capped((9 * cp) << log_m, 9 * cp)
    hcols10, cap10 = capped((65 * cp) << log_m, 65 * cp)
    hcols8, cap8 = capped((230 * cp) << log_m, 230 * cp)
    hcols6, cap6 = capped((33 * cp) << log_m, 33 * cp)
    pub10 = torch.randint(0, 2**32, ((49 * cp) << log_k10,), dtype=torch.int64, device=dev)
    pub6 = torch.randint(0, 2**32, ((26 * cp) << (log_rows - 6),), dtype=torch.int64, device=dev)
    table = torch.randint(0, 2**62, ((18 * cp) << log_rows,), dtype=torch.int64, device=dev)
    pre = torch.empty((65 * cp) << log_rows, dtype=torch.int64, device=dev)
    quot = torch.empty(2 << log_m, dtype=torch.int64, device=dev)
    q10 = lambda: ctx.air_sha512_link_quotient_device(log_m, log_blowup, cap_h, cp, cols.data_ptr(), hcols10.data_ptr(), cap_t.data_ptr(),
                                                      cap10.data_ptr(), pub10.data_ptr(), quot.data_ptr(), 0)
    q8 = lambda: ctx.air_sha512_sched_quotient_device(log_m, log_blowup, cap_h, cp, cols.data_ptr(), hcols8.data_ptr(), cap_t.data_ptr(),
                                                      cap8.data_ptr(), quot.data_ptr(), 0)
    q6 = lambda: ctx.air_sha256_link_quotient_device(log_m, log_blowup, cap_h, cp, cols6.data_ptr(), hcols6.data_ptr(), cap_t6.data_ptr(),
                                                     cap6.data_ptr(), pub6.data_ptr(), quot.data_ptr(), 0)
    res = {"mode": "sha512_link", "log_m": log_m, "proofs": cp, "reps": reps, "helper_kernel_ms": [], "sha512_link_quotient_call_ms": [],
           "sha512_sched_quotient_call_ms": [], "sha256_link_quotient_call_ms": []}
    for _ in range(rounds):
        res["helper_kernel_ms"].append(r4(timed(lambda: ctx.air_sha512_link_helper_device(log_rows, cp, table.data_ptr(), pub10.data_ptr(),
                                                                                         pre.data_ptr(), 0), reps)))
        res["sha512_link_quotient_call_ms"].append(r4(timed(q10, reps)))
        res["sha512_sched_quotient_call_ms"].append(r4(timed(q8, reps)))
        res["sha256_link_quotient_call_ms"].append(r4(timed(q6, reps)))
    res["quotient_sha256"] = words_digest(q10, quot)
    ps10 = min(res["sha512_link_quotient_call_ms"]) * 1e9 / ((83 * cp) << log_m)
    ps8 = min(res["sha512_sched_quotient_call_ms"]) * 1e9 / ((248 * cp) << log_m)
    ps6 = min(res["sha256_link_quotient_call_ms"]) * 1e9 / ((42 * cp) << log_m)
    res.update(ps_per_word_set10=round(ps10, 2), ps_per_word_set8=round(ps8, 2), ps_per_word_set6=round(ps6, 2),
               ratio_set10_over_set8=round(ps10 / ps8, 3), ratio_set10_over_set6=round(ps10 / ps6, 3), helper_rows=1 << log_rows,
               helper_store_tb_per_s=round(((65 * cp) << log_rows) * 8 / min(res["helper_kernel_ms"]) / 1e9, 3))
    print(json.dumps(res), flush=True)
    ctx.close()
    del cols, cap_t, cols6, cap_t6, hcols10, cap10, hcols8, cap8, hcols6, cap6, pub10, pub6, table, pre, quot
    torch.cuda.empty_cache()
    # the gather, the set-level call of set 10 on SHA512, the prove over the four oracles and the verifier
    from tendermintx_amd.synth import bench_workload
    sp = int(os.environ.get("S512_SET_P", "16"))
    w = bench_workload("survey8d", n, sp, seed=0x544D58)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = Context(n, b"celestia", 100800, device=0, max_batch=sp)
    out = torch.empty(sp * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
    rep = torch.empty(sp * 64, dtype=torch.uint8, device=dev)
    tr = torch.empty(sp * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(KIND_SKIP, sp, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(KIND_SKIP, sp, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    SHA512, HEADER = 2, 32
    cw = 4 << cap_h
    log_k, pub_cols = ctx.air_sha512_public_shape(KIND_SKIP, sp)
    pub = torch.empty(pub_cols << log_k, dtype=torch.int64, device=dev)
    gather = lambda: ctx.air_sha512_public_device(KIND_SKIP, sp, out.data_ptr(), pub.data_ptr(), 0)
    scaps, cap_h_, cap_q = (torch.zeros(k * cw, dtype=torch.int64, device=dev) for k in (2, 1, 1))
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)
    commit = lambda: ctx.trace_commit_set_device(KIND_SKIP, sp, SHA512 | HEADER, log_blowup, cap_h, tr.data_ptr(), scaps.data_ptr(), 0)
    res = {"mode": "sha512_link_set", "proofs": sp, "n": n, "reps": reps, "gather_ms": [], "commit_ms": r4(timed(commit, 2)), "air_sha512_link_ms": [],
           "prove_with_ms": []}
    for _ in range(rounds):
        res["gather_ms"].append(r4(timed(gather, reps)))
        res["air_sha512_link_ms"].append(r4(timed(lambda: ctx.trace_commit_set_air_sha512_link_device(SHA512, pub.data_ptr(), cap_h_.data_ptr(),
                                                                                                      cap_q.data_ptr(), 0), reps, before=commit)))
        shape, order = ctx.trace_commit_set_shape()
        bp = dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=0)
        proof = torch.empty(ctx.batch_layout(bp)["words"], dtype=torch.int64, device=dev)
        res["prove_with_ms"].append(r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), reps)))
        res["degree_ok"] = ctx.fri_last_degree_ok()
        kt = order.index(SHA512)
        all_caps = torch.cat([scaps[:(kt + 1) * cw], cap_h_, cap_q, scaps[(kt + 1) * cw:]])
        res["verify_ms"] = r4(timed(lambda: ctx.air_sha512_link_verify_device(bp, kt, kt + 1, all_caps.data_ptr(), proof.data_ptr(), pub.data_ptr(),
                                                                              ok.data_ptr(), 0), 3))
        res["all_ok"] = bool((ok.cpu().numpy() == 1).all())
        res.update(order=order, log_n=bp["log_n"], columns=bp["n_cols"], cap_h_sha256=hashlib.sha256(cap_h_.cpu().numpy().tobytes()).hexdigest()[:16],
                   cap_q_sha256=hashlib.sha256(cap_q.cpu().numpy().tobytes()).hexdigest()[:16])
        del proof
    print(json.dumps(res), flush=True)
    ctx.close()
    del tr, out
    torch.cuda.empty_cache()

if "sha512_streamed" in modes:
    from tendermintx_amd.synth import bench_workload
    from tendermintx_amd.context import trace_commit_set_air_sha512_streamed_bytes
    SHA512, HEADER = 2, 32
    sets, cpf = [int(x) for x in os.environ.get("SETS", "7").split(",")], int(os.environ.get("CHUNK_PROOFS", "8"))
    full = os.environ.get("FULL", "0") == "1"
    hcols = {7: 599, 8: 230, 9: 629}
    sp = int(os.environ.get("SHA_SET_P", "16"))
    w = bench_workload("survey8d", n, sp, seed=0x544D58)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = Context(n, b"celestia", 100800, device=0, max_batch=sp)
    out = torch.empty(sp * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
    rep = torch.empty(sp * 64, dtype=torch.uint8, device=dev)
    tr = torch.empty(sp * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(KIND_SKIP, sp, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(KIND_SKIP, sp, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    del out
    cw = 4 << cap_h
    scaps = torch.zeros(2 * cw, dtype=torch.int64, device=dev)
    pair = {s_: torch.zeros(2 * cw, dtype=torch.int64, device=dev) for s_ in sets}
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)
    commit = lambda: ctx.trace_commit_set_device(KIND_SKIP, sp, SHA512 | HEADER, log_blowup, cap_h, tr.data_ptr(), scaps.data_ptr(), 0)
    resident = {7: ctx.trace_commit_set_air_sha512_device, 8: ctx.trace_commit_set_air_sha512_sched_device,
                9: ctx.trace_commit_set_air_sha512_init_device}

    def call(s_, streamed):
        if streamed:
            ctx.trace_commit_set_air_sha512_streamed_device(s_, SHA512, cpf, pair[s_][:cw].data_ptr(), pair[s_][cw:].data_ptr(), 0)
        else:
            resident[s_](SHA512, pair[s_][:cw].data_ptr(), pair[s_][cw:].data_ptr(), 0)

    def calls(streamed):
        for s_ in sets:
            call(s_, streamed)

    digests = lambda: {str(s_): [hashlib.sha256(pair[s_][k * cw:(k + 1) * cw].cpu().numpy().tobytes()).hexdigest()[:16] for k in (0, 1)] for s_ in sets}
    commit()
    shape0, order0 = ctx.trace_commit_set_shape()
    log_m = shape0["log_n"][order0.index(SHA512)]
    res = {"mode": "sha512_streamed", "full": full, "sets": sets, "proofs": sp, "n": n, "log_m": log_m, "chunk_proofs": cpf, "reps": reps,
           "bytes": {str(s_): list(trace_commit_set_air_sha512_streamed_bytes(s_, log_m, log_blowup, cap_h, sp, cpf)) for s_ in sets},
           "bytes_resident": {str(s_): list(trace_commit_set_air_sha512_streamed_bytes(s_, log_m, log_blowup, cap_h, sp, sp)) for s_ in sets}}

    def prove_and_verify(k):
        """k timed proves after a warm one (k = 0: ONE prove, timed cold); the verdicts of the sets' verifiers on the last proof"""
        shape, order = ctx.trace_commit_set_shape()
        bp = dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=0)
        proof = torch.empty(ctx.batch_layout(bp)["words"], dtype=torch.int64, device=dev)
        if k:
            ms = r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), k))
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0)
            b.record()
            torch.cuda.synchronize(dev)
            ms = r4(a.elapsed_time(b))
        kt = order.index(SHA512)
        caps, at, where = [scaps[:(kt + 1) * cw]], kt + 1, {}
        for s_ in sorted(sets):
            caps.append(pair[s_])
            where[s_] = at
            at += 2
        all_caps = torch.cat(caps + [scaps[(kt + 1) * cw:]])
        verdicts = {}
        for s_, kh in where.items():
            if s_ == 7:
                ctx.air_sha512_verify_device(bp, kt, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
            elif s_ == 8:
                ctx.air_sha512_sched_verify_device(bp, kt, kh, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
            else:
                ctx.air_sha512_init_verify_device(bp, kt, kh, all_caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
            verdicts[str(s_)] = bool((ok.cpu().numpy() == 1).all())
        return ms, verdicts, ctx.fri_last_degree_ok(), order, bp["n_cols"]

    if not full:
        res.update(resident_call_ms=[], streamed_call_ms=[], prove_resident_ms=[], prove_streamed_ms=[])
        calls(False)   # (the warm call: the context's scratches and the LDE's grow here, outside every round)
        for _ in range(rounds):
            res["resident_call_ms"].append(r4(timed(lambda: calls(False), reps, before=commit)))
            ms, res["verdicts_resident"], _, _, _ = prove_and_verify(reps)
            res["prove_resident_ms"].append(ms)
            res["caps_resident"] = digests()
            res["streamed_call_ms"].append(r4(timed(lambda: calls(True), reps, before=commit)))
            ms, res["verdicts_streamed"], res["degree_ok"], res["order"], res["columns"] = prove_and_verify(reps)
            res["prove_streamed_ms"].append(ms)
            res["caps_streamed"] = digests()
        res["caps_equal"] = res["caps_resident"] == res["caps_streamed"]
        # the chunk LDE alone: both sweeps' transforms of every set over buffers of the sizes the call uses, and the prove's third
        log_sub = log_m - log_blowup
        big = max(hcols[s_] for s_ in sets)
        pre = torch.randint(0, 2**62, ((big * sp) << log_sub,), dtype=torch.int64, device=dev)
        chunk_buf = torch.empty((big * cpf) << log_m, dtype=torch.int64, device=dev)

        def lde_alone(sweeps):
            for s_ in sets:
                for _sweep in range(sweeps):
                    for p0 in range(0, sp, cpf):
                        k_ = min(cpf, sp - p0) * hcols[s_]
                        ctx.lde_device(log_sub, log_blowup, k_, pre[(p0 * hcols[s_]) << log_sub:].data_ptr(), chunk_buf.data_ptr(), 0)

        res["chunk_lde_two_sweeps_ms"] = [r4(timed(lambda: lde_alone(2), reps)) for _ in range(rounds)]
        res["chunk_lde_one_sweep_ms"] = [r4(timed(lambda: lde_alone(1), reps)) for _ in range(rounds)]
        best_s, best_r = min(res["streamed_call_ms"]), min(res["resident_call_ms"])
        res["ratio_streamed_over_resident_call"] = round(best_s / best_r, 3)
        res["ratio_streamed_over_resident_prove"] = round(min(res["prove_streamed_ms"]) / min(res["prove_resident_ms"]), 3)
        res["call_excess_ms"] = r4(best_s - best_r)
        res["prove_excess_ms"] = r4(min(res["prove_streamed_ms"]) - min(res["prove_resident_ms"]))
        res["helper_lde_share_of_streamed"] = round(min(res["chunk_lde_two_sweeps_ms"]) / best_s, 3)
        del pre, chunk_buf
    else:
        # the streamed calls only, once each (the resident helpers do not fit): a refusal is recorded as it is worded, not worked around
        res["free_before_mib"] = torch.cuda.mem_get_info(dev)[0] >> 20
        res["streamed_call_ms"], res["free_after_mib"] = {}, {}
        try:
            for s_ in sets:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call(s_, True)
                b.record()
                torch.cuda.synchronize(dev)
                res["streamed_call_ms"][str(s_)] = r4(a.elapsed_time(b))
                res["free_after_mib"][str(s_)] = torch.cuda.mem_get_info(dev)[0] >> 20
                res["scratch_bytes_" + str(s_)] = ctx.trace_commit_set_air_sha512_scratch_bytes(s_, SHA512)
            res["caps_streamed"] = digests()
            res["prove_streamed_ms"], res["verdicts_streamed"], res["degree_ok"], res["order"], res["columns"] = prove_and_verify(0)
            res["free_after_prove_mib"] = torch.cuda.mem_get_info(dev)[0] >> 20
        except _lib.TmxError as e:
            res["refused"] = {"status": e.status, "text": str(e)}
    print(json.dumps(res), flush=True)
    ctx.close()
    del tr
    torch.cuda.empty_cache()
