#!/usr/bin/env python3
"""Openings of the last commit (tmx_trace_commit_open_device) and their device check (tmx_poseidon_merkle_verify_device) on the bench
workload, next to the commit they open: one JSON line.  Open time in us per call (HIP events around REPS back-to-back calls, the one-launch
form and TMX_OPEN_SPLIT=1's two launches), verify time in ms per call, for 16 / 128 / 1024 random queries.
   P=16 N=32 python tools/open_bench.py          P=256 N=128 python tools/open_bench.py   (SECTION=sha512 BLOWUP=3 CAP=4 by default)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from tendermintx_amd import Context, _lib  # noqa: E402
from tendermintx_amd.context import KIND_SKIP  # noqa: E402
from tendermintx_amd.synth import bench_workload  # noqa: E402

P, n = int(os.environ.get("P", "16")), int(os.environ.get("N", "32"))
SEC = {"ladders": _lib.TRACE_LADDERS, "sha512": _lib.TRACE_SHA512, "sha256": _lib.TRACE_SHA256, "tree": _lib.TRACE_TREE, "header": _lib.TRACE_HEADER}
name = os.environ.get("SECTION", "sha512")
log_blowup, cap_h, reps = int(os.environ.get("BLOWUP", "3")), int(os.environ.get("CAP", "4")), int(os.environ.get("REPS", "50"))
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
pl = log_m - ch
rng = np.random.default_rng(5)


def timed(fn, k):
    fn()  # (warm: the index staging grows on first use)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / k


res = {}
for nq in (16, 128, 1024):
    idx = rng.integers(0, 1 << log_m, nq, dtype=np.uint64)
    rows = torch.empty((nq, n_cols), dtype=torch.int64, device=dev)
    paths = torch.empty((nq, pl, 4), dtype=torch.int64, device=dev)
    ok = torch.zeros(nq, dtype=torch.int32, device=dev)
    r = {}
    for form, env in (("open_us", "0"), ("open_split_us", "1")):
        os.environ["TMX_OPEN_SPLIT"] = env
        r[form] = round(1e3 * timed(lambda: ctx.trace_commit_open_device(idx, rows.data_ptr(), paths.data_ptr(), 0), reps), 2)
    os.environ.pop("TMX_OPEN_SPLIT")
    r["verify_ms"] = round(timed(lambda: ctx.poseidon_merkle_verify_device(log_m, n_cols, ch, cap.data_ptr(), idx, rows.data_ptr(), paths.data_ptr(),
                                                                            ok.data_ptr(), 0), max(3, reps // 10)), 4)
    r["all_ok"] = bool((ok.cpu().numpy() == 1).all())
    r["open_of_commit"] = round(r["open_us"] * 1e-3 / sum(commit_ms.values()), 6)
    res[str(nq)] = r
print(json.dumps({"section": name, "proofs": P, "n": n, "log_rows_ext": log_m, "columns": n_cols, "cap_height": ch, "path_len": pl,
                  "permutations_per_query": (n_cols + 7) // 8 + pl, "commit_ms": {k: round(v, 4) for k, v in commit_ms.items()},
                  "commit_ms_total": round(sum(commit_ms.values()), 4), "queries": res}), flush=True)
ctx.close()
