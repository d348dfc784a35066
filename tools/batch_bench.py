#!/usr/bin/env python3
"""One mixed-size batch proof over a commit set (tmx_trace_commit_set_device, tmx_trace_commit_set_prove_device) next to what it replaces:
the SUM of one DEEP prove per section (tmx_trace_commit_deep_device, each after its own tmx_trace_commit_device), back to back on the same
trace rows: one JSON line.  Times per call from HIP events around REPS back-to-back calls; the four single proves are repeated ROUNDS
times, section by section, and the spread of their sum is what the set prove is held against.  Also: both sides' stages (tmx_fri_last_ms;
"combine" holds everything before the first layer), the device verifier of the set proof against the sum of the four single verifies,
the proof words of both, all-queries-accept.  POW_BITS=b (1 .. 24) runs the grinding variants of both sides.
   P=256 N=128 python tools/batch_bench.py   (SECTIONS=sha512,tree,sha256,header BLOWUP=3 CAP=4 ARITY=4 FINAL=5 QUERIES=28 by default)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tendermintx_amd import Context, _lib  # noqa: E402
from tendermintx_amd.context import KIND_SKIP, deep_proof_words, pow_proof_words  # noqa: E402
from tendermintx_amd.synth import bench_workload  # noqa: E402

P, n = int(os.environ.get("P", "256")), int(os.environ.get("N", "128"))
SEC = {"ladders": _lib.TRACE_LADDERS, "sha512": _lib.TRACE_SHA512, "sha256": _lib.TRACE_SHA256, "tree": _lib.TRACE_TREE, "header": _lib.TRACE_HEADER}
names = os.environ.get("SECTIONS", "sha512,tree,sha256,header").split(",")
log_blowup, cap_h, reps = int(os.environ.get("BLOWUP", "3")), int(os.environ.get("CAP", "4")), int(os.environ.get("REPS", "10"))
arity, final_max, nq = int(os.environ.get("ARITY", "4")), int(os.environ.get("FINAL", "5")), int(os.environ.get("QUERIES", "28"))
pow_bits, rounds = int(os.environ.get("POW_BITS", "0")), int(os.environ.get("ROUNDS", "3"))
w = bench_workload("survey8d", n, P, seed=0x544D58)
dev = torch.device("cuda:0")
d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
ctx = Context(n, b"celestia", 100800, device=0, max_batch=P)
out = torch.empty(P * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
rep = torch.empty(P * 64, dtype=torch.uint8, device=dev)
tr = torch.empty(P * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
ctx.witness_batch_device(KIND_SKIP, P, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
ctx.trace_rows_device(KIND_SKIP, P, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
del out


def timed(fn, k):
    fn()  # (warm: the prover's scratch grows on first use)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / k


r4 = lambda x: round(x, 4)
stage4 = lambda s: {k: r4(v) for k, v in s.items()}
ok = torch.zeros(nq, dtype=torch.int32, device=dev)

# ---- the four single proves, ROUNDS times: commit, DEEP prove (grinding: its pow variant), verify once per section in the first round
single = {nm: {"prove_ms": []} for nm in names}
sums = []
for rnd in range(rounds):
    total = 0.0
    for nm in names:
        cap = torch.zeros(4 << cap_h, dtype=torch.int64, device=dev)
        ctx.trace_commit_device(KIND_SKIP, P, SEC[nm], log_blowup, cap_h, tr.data_ptr(), cap.data_ptr(), 0)
        log_m, n_cols, ch = ctx.trace_commit_last_shape()
        fp = dict(log_n=log_m, n_cols=n_cols, cap_height=ch, log_blowup=log_blowup, arity_bits=arity, final_log_max=final_max, n_queries=nq)
        words = pow_proof_words(fp, pow_bits, True) if pow_bits else deep_proof_words(fp)
        proof = torch.empty(words, dtype=torch.int64, device=dev)
        if pow_bits:
            prove = lambda: ctx.trace_commit_pow_device(fp, pow_bits, True, proof.data_ptr(), 0)
            verify = lambda: ctx.pow_verify_device(fp, pow_bits, True, cap.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
        else:
            prove = lambda: ctx.trace_commit_deep_device(fp, proof.data_ptr(), 0)
            verify = lambda: ctx.deep_verify_device(fp, cap.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
        ms = timed(prove, reps)
        total += ms
        s = single[nm]
        s["prove_ms"].append(r4(ms))
        if rnd == 0:
            s.update(log_rows_ext=log_m, columns=n_cols, proof_words=words, stage_ms=stage4(ctx.fri_last_ms()), verify_ms=r4(timed(verify, 3)),
                     all_ok=bool((ok.cpu().numpy() == 1).all()), degree_ok=ctx.fri_last_degree_ok())
        del proof
    sums.append(r4(total))

# ---- the set: commit all sections side by side, ONE proof
mask = sum(SEC[nm] for nm in names)
caps = torch.zeros(len(names) * (4 << cap_h), dtype=torch.int64, device=dev)
commit_set_ms = timed(lambda: ctx.trace_commit_set_device(KIND_SKIP, P, mask, log_blowup, cap_h, tr.data_ptr(), caps.data_ptr(), 0), 1)
shape, section_of = ctx.trace_commit_set_shape()
bp = dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=pow_bits)
layout = ctx.batch_layout(bp)
bproof = torch.empty(layout["words"], dtype=torch.int64, device=dev)
set_ms = [r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, bproof.data_ptr(), 0), reps)) for _ in range(rounds)]
set_stages = ctx.fri_last_ms()
set_degree_ok = ctx.fri_last_degree_ok()
set_verify_ms = timed(lambda: ctx.batch_verify_device(bp, caps.data_ptr(), bproof.data_ptr(), ok.data_ptr(), 0), 3)
set_ok = bool((ok.cpu().numpy() == 1).all())
print(json.dumps({"proofs": P, "n": n, "sections": names, "set_order": section_of, "log_blowup": log_blowup, "cap_height": cap_h, "arity_bits": arity,
                  "final_log_max": final_max, "queries": nq, "pow_bits": pow_bits, "reps": reps, "set_log_n": bp["log_n"], "set_columns": bp["n_cols"],
                  "set_layer_bits": layout["layer_bits"], "set_layer_enter": layout["layer_enter"], "set_final_log": layout["final_log"],
                  "commit_set_ms": r4(commit_set_ms), "set_prove_ms": set_ms, "set_stage_ms": stage4(set_stages), "single": single,
                  "single_prove_sum_ms": sums, "single_sum_spread_ms": r4(max(sums) - min(sums)),
                  "set_minus_single_sum_ms": r4(min(set_ms) - min(sums)), "set_verify_ms": r4(set_verify_ms),
                  "single_verify_sum_ms": r4(sum(s["verify_ms"] for s in single.values())), "set_proof_words": layout["words"],
                  "single_proof_words_sum": sum(s["proof_words"] for s in single.values()), "set_degree_ok": set_degree_ok, "set_all_ok": set_ok,
                  "single_all_ok": all(s["all_ok"] for s in single.values())}), flush=True)
ctx.close()
