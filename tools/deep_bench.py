#!/usr/bin/env python3
"""DEEP-FRI over the last commit (tmx_trace_commit_deep_device) next to the plain FRI prove of the same commit (back to back, same
parameters) and its device check (tmx_deep_verify_device), on the tools/fri_bench.py workload: one JSON line.  Prove times per call (HIP
events around REPS back-to-back calls), the DEEP prove split by tmx_fri_last_ms (its "combine" holds everything before the first layer:
transcript start, evaluation, openings tree, combine, quotient), verify time per call, the bytes the evaluation reads (n_cols x N x 8),
all-queries-accept, and a spot check: the openings of 8 columns against the CPU oracle (interpolation + Horner, tests/deep_model.py).
POW_BITS=b (1 .. 24) adds the grinding DEEP prove of the same commit (tmx_trace_commit_pow_device), back to back with the plain one: its
time, stages, nonce, candidates evaluated, and the search's time as the difference of the two "final" stages, hence candidates per second.
   P=256 N=128 python tools/deep_bench.py   (SECTION=sha512 BLOWUP=3 CAP=4 ARITY=4 FINAL=5 QUERIES=28 by default)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "py"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from tendermintx_amd import Context, _lib  # noqa: E402
from tendermintx_amd.context import KIND_SKIP, deep_proof_words  # noqa: E402
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
fri_proof = torch.empty(layout["words"], dtype=torch.int64, device=dev)
proof = torch.empty(deep_proof_words(params), dtype=torch.int64, device=dev)
ok = torch.zeros(nq, dtype=torch.int32, device=dev)


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


fri_ms = timed(lambda: ctx.trace_commit_fri_device(params, fri_proof.data_ptr(), 0), reps)
fri_stages = ctx.fri_last_ms()
deep_ms = timed(lambda: ctx.trace_commit_deep_device(params, proof.data_ptr(), 0), reps)
stages = ctx.fri_last_ms()
degree_ok = ctx.fri_last_degree_ok()
zeta = ctx.deep_last_zeta()
verify_ms = timed(lambda: ctx.deep_verify_device(params, cap.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0), 3)
all_ok = bool((ok.cpu().numpy() == 1).all())
grind = {}
if pow_bits:
    pproof = torch.empty(ctx.pow_proof_words(params, pow_bits, True), dtype=torch.int64, device=dev)
    pow_ms = timed(lambda: ctx.trace_commit_pow_device(params, pow_bits, True, pproof.data_ptr(), 0), reps)
    pstages = ctx.fri_last_ms()
    nonce, tried = ctx.pow_last()
    plain_again_ms = timed(lambda: ctx.trace_commit_deep_device(params, proof.data_ptr(), 0), reps)
    ctx.pow_verify_device(params, pow_bits, True, cap.data_ptr(), pproof.data_ptr(), ok.data_ptr(), 0)
    pow_ok = bool((ok.cpu().numpy() == 1).all())
    search_ms = pstages["final"] - stages["final"]
    grind = {"pow_bits": pow_bits, "pow_prove_ms": round(pow_ms, 4), "plain_prove_again_ms": round(plain_again_ms, 4),
             "pow_extra_ms": round(pow_ms - (deep_ms + plain_again_ms) / 2, 4), "pow_stage_ms": {k: round(v, 4) for k, v in pstages.items()},
             "nonce": nonce, "tried": tried, "search_ms_by_stage_difference": round(search_ms, 4),
             "candidates_per_s": round(tried / (search_ms * 1e-3)) if search_ms > 0 else None, "pow_all_ok": pow_ok}
# spot check: 8 columns' openings against interpolation + Horner of the trace columns on the CPU (tests/deep_model.py over the oracle's NTT;
# a column is one (proof, cell) of the section's rows, natural order, zero padded -- tmx_trace_commit_device's first stage)
import deep_model as dm  # noqa: E402
import oracle_c  # noqa: E402
from test_merkle_open import _section_geom  # noqa: E402

oracle_c.build()
off, rows, width = _section_geom(0, n, SEC[name])
host_tr = tr.cpu().numpy().view(np.uint64).reshape(P, -1)
pick = [int(c) for c in np.linspace(0, n_cols - 1, 8)]
cols = np.zeros((len(pick), 1 << (log_m - log_blowup)), dtype=np.uint64)
for k, c in enumerate(pick):
    cols[k, :rows] = host_tr[c // width, off:off + rows * width].reshape(rows, width)[:, c % width]
ys = dm.evaluate(oracle_c, cols, 1, dm.points(oracle_c, params, zeta))
got = dm.openings_of(params, proof.cpu().numpy().view(np.uint64))
spot_ok = all(tuple(ys[k]) == got[c] for k, c in enumerate(pick))
print(json.dumps({**grind, "section": name, "proofs": P, "n": n, "log_rows_ext": log_m, "columns": n_cols, "cap_height": ch, "arity_bits": arity,
                  "final_log_max": final_max, "queries": nq, "layer_bits": layout["layer_bits"], "final_log": layout["final_log"],
                  "proof_words": proof.numel(), "commit_ms_total": round(sum(commit_ms.values()), 4), "fri_prove_ms": round(fri_ms, 4),
                  "fri_stage_ms": {k: round(v, 4) for k, v in fri_stages.items()}, "deep_prove_ms": round(deep_ms, 4),
                  "deep_stage_ms": {k: round(v, 4) for k, v in stages.items()}, "eval_gb": round(n_cols * (1 << (log_m - log_blowup)) * 8 / 1e9, 3),
                  "verify_ms": round(verify_ms, 4), "degree_ok": degree_ok, "all_ok": all_ok, "spot_columns": pick, "spot_ok": spot_ok}), flush=True)
ctx.close()
