#!/usr/bin/env python3
"""The batched FRI proof over the last commit (tmx_trace_commit_fri_device) and its device check (tmx_fri_verify_device) on the bench
workload, next to the commit it proves: one JSON line.  Prove time per call (HIP events around REPS back-to-back calls) and split by
tmx_fri_last_ms (combine, layers, final + transcript, openings); the combine's achieved TB/s over the n_cols x 2^log_m x 8 B it reads once;
verify time per call; degree flag and verdicts.  POW_BITS=b (1 .. 24) adds the grinding prove of the same commit
(tmx_trace_commit_pow_device), back to back with the plain one: its time, stages, nonce, candidates evaluated, and the search's time taken
as the difference of the two "final" stages (the search is the only wide launch there), hence candidates per second.
   P=256 N=128 python tools/fri_bench.py   (SECTION=sha512 BLOWUP=3 CAP=4 ARITY=4 FINAL=5 QUERIES=28 by default)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tendermintx_amd import Context, _lib  # noqa: E402
from tendermintx_amd.context import KIND_SKIP  # noqa: E402
from tendermintx_amd.synth import bench_workload  # noqa: E402

P, n = int(os.environ.get("P", "256")), int(os.environ.get("N", "128"))
SEC = {"ladders": _lib.TRACE_LADDERS, "sha512": _lib.TRACE_SHA512, "sha256": _lib.TRACE_SHA256, "tree": _lib.TRACE_TREE, "header": _lib.TRACE_HEADER}
name = os.environ.get("SECTION", "sha512")
log_blowup, cap_h, reps = int(os.environ.get("BLOWUP", "3")), int(os.environ.get("CAP", "4")), int(os.environ.get("REPS", "20"))
arity, final_max, nq = int(os.environ.get("ARITY", "4")), int(os.environ.get("FINAL", "5")), int(os.environ.get("QUERIES", "28"))
pow_bits = int(os.environ.get("POW_BITS", "0"))
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
cap = torch.zeros(4 << cap_h, dtype=torch.int64, device=dev)
for _ in range(2):
    ctx.trace_commit_device(KIND_SKIP, P, SEC[name], log_blowup, cap_h, tr.data_ptr(), cap.data_ptr(), 0)
commit_ms = ctx.trace_commit_last_ms()
log_m, n_cols, ch = ctx.trace_commit_last_shape()
params = dict(log_n=log_m, n_cols=n_cols, cap_height=ch, log_blowup=log_blowup, arity_bits=arity, final_log_max=final_max, n_queries=nq)
layout = ctx.fri_layout(params)
proof = torch.empty(layout["words"], dtype=torch.int64, device=dev)
ok = torch.zeros(nq, dtype=torch.int32, device=dev)


def timed(fn, k):
    fn()  # (warm: the FRI scratch grows on first use)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / k


prove_ms = timed(lambda: ctx.trace_commit_fri_device(params, proof.data_ptr(), 0), reps)
stages = ctx.fri_last_ms()
degree_ok = ctx.fri_last_degree_ok()
verify_ms = timed(lambda: ctx.fri_verify_device(params, cap.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0), 3)
combine_bytes = n_cols * (1 << log_m) * 8
grind = {}
if pow_bits:
    pproof = torch.empty(ctx.pow_proof_words(params, pow_bits, False), dtype=torch.int64, device=dev)
    pow_ms = timed(lambda: ctx.trace_commit_pow_device(params, pow_bits, False, pproof.data_ptr(), 0), reps)
    pstages = ctx.fri_last_ms()
    nonce, tried = ctx.pow_last()
    plain_again_ms = timed(lambda: ctx.trace_commit_fri_device(params, proof.data_ptr(), 0), reps)
    ctx.pow_verify_device(params, pow_bits, False, cap.data_ptr(), pproof.data_ptr(), ok.data_ptr(), 0)
    pow_ok = bool((ok.cpu().numpy() == 1).all())
    ctx.fri_verify_device(params, cap.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0)
    search_ms = pstages["final"] - stages["final"]
    grind = {"pow_bits": pow_bits, "pow_prove_ms": round(pow_ms, 4), "plain_prove_again_ms": round(plain_again_ms, 4),
             "pow_extra_ms": round(pow_ms - (prove_ms + plain_again_ms) / 2, 4), "pow_stage_ms": {k: round(v, 4) for k, v in pstages.items()},
             "nonce": nonce, "tried": tried, "search_ms_by_stage_difference": round(search_ms, 4),
             "candidates_per_s": round(tried / (search_ms * 1e-3)) if search_ms > 0 else None, "pow_all_ok": pow_ok}
print(json.dumps({**grind, "section": name, "proofs": P, "n": n, "log_rows_ext": log_m, "columns": n_cols, "cap_height": ch, "arity_bits": arity,
                  "final_log_max": final_max, "queries": nq, "layer_bits": layout["layer_bits"], "final_log": layout["final_log"],
                  "proof_words": layout["words"], "commit_ms_total": round(sum(commit_ms.values()), 4), "prove_ms": round(prove_ms, 4),
                  "prove_stage_ms": {k: round(v, 4) for k, v in stages.items()}, "combine_gb": round(combine_bytes / 1e9, 3),
                  "combine_tb_s": round(combine_bytes / (stages["combine"] * 1e-3) / 1e12, 3), "verify_ms": round(verify_ms, 4),
                  "degree_ok": degree_ok, "all_ok": bool((ok.cpu().numpy() == 1).all())}), flush=True)
ctx.close()
