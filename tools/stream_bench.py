#!/usr/bin/env python3
"""Streamed members of a commit set (tmx_trace_commit_set_streamed_device) next to the resident set they must equal: one JSON line.
  1. one section that fits both ways (SECTION=sha512): commit resident and streamed with every chunk size of CHUNKS, alternating, ROUNDS
     times in this one process; then the one-member set proved both ways, stage by stage (tmx_fri_last_ms), and the proofs compared.
  2. the full set (all five row tables) with the ladders streamed at CHUNK columns per chunk: commit, prove without and with POW_BITS bits
     of grinding, the device verifier, proof words, tmx_trace_commit_set_bytes and free device memory before / after.  FULL=0 skips it.
Times per call from HIP events around REPS back-to-back calls, after one warm call (scratch grows on first use).
   P=256 N=128 python tools/stream_bench.py   (BLOWUP=3 CAP=4 ARITY=4 FINAL=5 QUERIES=28 CHUNKS=256,512,1024,2048 CHUNK=512 by default)"""
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
ALL = sum(SEC.values())
section = SEC[os.environ.get("SECTION", "sha512")]
chunks = [int(x) for x in os.environ.get("CHUNKS", "256,512,1024,2048").split(",")]
chunk = int(os.environ.get("CHUNK", "512"))
log_blowup, cap_h, reps = int(os.environ.get("BLOWUP", "3")), int(os.environ.get("CAP", "4")), int(os.environ.get("REPS", "5"))
arity, final_max, nq = int(os.environ.get("ARITY", "4")), int(os.environ.get("FINAL", "5")), int(os.environ.get("QUERIES", "28"))
pow_bits, rounds, do_full = int(os.environ.get("POW_BITS", "16")), int(os.environ.get("ROUNDS", "3")), os.environ.get("FULL", "1") != "0"
w = bench_workload("survey8d", n, P, seed=0x544D58)
dev = torch.device("cuda:0")
d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
ctx = Context(n, b"celestia", 100800, device=0, max_batch=P)
out = torch.empty(P * ctx.elem_stride(KIND_SKIP), dtype=torch.int64, device=dev)
rep = torch.empty(P * 64, dtype=torch.uint8, device=dev)
tr = torch.empty(P * ctx.trace_elem_count(KIND_SKIP), dtype=torch.int64, device=dev)
ctx.witness_batch_device(KIND_SKIP, P, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
ctx.trace_rows_device(KIND_SKIP, P, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
torch.cuda.synchronize(dev)
del out


def timed(fn, k):
    fn()  # (warm: the scratch grows on first use)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / k


def free_gib():
    torch.cuda.synchronize(dev)
    return round(torch.cuda.mem_get_info(dev)[0] / 2**30, 2)


r4 = lambda x: round(x, 4)
stage4 = lambda s: {k: r4(v) for k, v in s.items()}
gib = lambda b: round(b / 2**30, 2)
ok = torch.zeros(nq, dtype=torch.int32, device=dev)
res = {"proofs": P, "n": n, "log_blowup": log_blowup, "cap_height": cap_h, "arity_bits": arity, "final_log_max": final_max, "queries": nq,
       "reps": reps, "rounds": rounds, "free_gib_start": free_gib()}


def commit(sections, streamed, cc, caps):
    if streamed is None:
        ctx.trace_commit_set_device(KIND_SKIP, P, sections, log_blowup, cap_h, tr.data_ptr(), caps.data_ptr(), 0)
    else:
        ctx.trace_commit_set_streamed_device(KIND_SKIP, P, sections, streamed, cc, log_blowup, cap_h, tr.data_ptr(), caps.data_ptr(), 0)


def prove_params(bits):
    shape, order = ctx.trace_commit_set_shape()
    return dict(shape, arity_bits=arity, final_log_max=final_max, n_queries=nq, pow_bits=bits), order


# ---- 1. one section both ways (the resident commit first: the set's scratch only grows, so nothing is reallocated inside a timed call)
caps_r = torch.zeros(4 << cap_h, dtype=torch.int64, device=dev)
caps_s = torch.zeros_like(caps_r)
one = {"commit_resident_ms": [], "commit_streamed_ms": {str(c): [] for c in chunks}}
for _ in range(rounds):
    one["commit_resident_ms"].append(r4(timed(lambda: commit(section, None, 0, caps_r), reps)))
    for c in chunks:
        one["commit_streamed_ms"][str(c)].append(r4(timed(lambda: commit(section, section, c, caps_s), reps)))
        assert torch.equal(caps_r, caps_s), c
proofs, prove = {}, {"resident_ms": [], "streamed_ms": []}
for _ in range(rounds):
    for key, streamed in (("resident", None), ("streamed", section)):
        commit(section, streamed, chunk, caps_s)
        bp, _ = prove_params(0)
        words = ctx.batch_layout(bp)["words"]
        proofs[key] = torch.empty(words, dtype=torch.int64, device=dev)
        prove[key + "_ms"].append(r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proofs[key].data_ptr(), 0), reps)))
        prove[key + "_stage_ms"] = stage4(ctx.fri_last_ms())
prove["proofs_equal"] = bool(torch.equal(proofs["resident"], proofs["streamed"]))
prove["columns"], prove["log_rows_ext"], prove["chunk_cols"], prove["proof_words"] = bp["n_cols"][0], bp["log_n"][0], chunk, words
one["prove"] = prove
res["one_section"] = one
res["free_gib_after_one_section"] = free_gib()
del proofs

# ---- 2. all five row tables, the ladders streamed
if do_full:
    full = {"chunk_cols": chunk, "bytes_streamed_gib": gib(ctx.trace_commit_set_bytes(KIND_SKIP, P, ALL, SEC["ladders"], chunk, log_blowup, cap_h)),
            "bytes_resident_gib": gib(ctx.trace_commit_set_bytes(KIND_SKIP, P, ALL, 0, chunk, log_blowup, cap_h))}
    caps = torch.zeros(5 * (4 << cap_h), dtype=torch.int64, device=dev)
    full["commit_ms"] = [r4(timed(lambda: commit(ALL, SEC["ladders"], chunk, caps), 1)) for _ in range(rounds)]
    full["free_gib_after_commit"] = free_gib()
    for bits in (0, pow_bits):
        bp, order = prove_params(bits)
        layout = ctx.batch_layout(bp)
        proof = torch.empty(layout["words"], dtype=torch.int64, device=dev)
        tag = "pow%d" % bits if bits else "plain"
        full["prove_%s_ms" % tag] = [r4(timed(lambda: ctx.trace_commit_set_prove_device(bp, proof.data_ptr(), 0), reps)) for _ in range(rounds)]
        full["stage_%s_ms" % tag] = stage4(ctx.fri_last_ms())
        full["degree_ok_" + tag] = ctx.fri_last_degree_ok()
        full["verify_%s_ms" % tag] = r4(timed(lambda: ctx.batch_verify_device(bp, caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0), 3))
        full["all_ok_" + tag] = bool((ok.cpu().numpy() == 1).all())
        full["proof_words_" + tag] = layout["words"]
        del proof
    full.update(order=order, log_n=bp["log_n"], columns=bp["n_cols"], layer_bits=layout["layer_bits"], layer_enter=layout["layer_enter"])
    full["free_gib_after_prove"] = free_gib()
    res["five_sections"] = full
print(json.dumps(res), flush=True)
ctx.close()
