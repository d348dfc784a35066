"""The driver keeps the tail of bench.py's stdout and parses its LAST line (contract: task description "bench.py").
Round 5's 20.5-KB line came back `parsed: null`: the record line is now a compact projection of the full record (bench.compact_line),
capped well under 8 KB; the full record goes to bench_extras.json and to an earlier, prefixed stdout line."""
import glob
import io
import json
import os
from contextlib import redirect_stdout

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")


def _full_records():
    """Every full bench record the builder committed (round 5's is the one the driver could not parse) + this round's when present."""
    out = []
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[4-9]_bench*.json"))):
        try:
            d = json.load(open(p))
        except ValueError:
            continue
        if isinstance(d, dict) and "bench_extras" in d:
            d = d["bench_extras"]
        if isinstance(d, dict) and "metric" in d and "roofline" in d:
            out.append((os.path.basename(p), d))
    return out


@pytest.mark.parametrize("name,full", _full_records(), ids=[n for n, _ in _full_records()])
def test_record_line_is_short_and_complete(name, full):
    import bench
    line = json.dumps(bench.compact_line(full))
    assert len(line) < 8192 and len(line) <= bench.LINE_CAP
    rec = json.loads(line)
    for k in CONTRACT:
        assert k in rec, k
    assert rec["vs_baseline"] is None and rec["higher_is_better"] is False
    assert "workload" in rec["config"] and "model" not in rec["config"]
    assert isinstance(rec["roofline"]["frac"], float) and rec["roofline"]["bound"] == "hbm" and "traffic" in rec["roofline"]
    if "extras" not in full:      # a full record (a compact one replayed through compact_line keeps what it has)
        assert rec["cpu_baseline"]["cores"] >= 1 and rec["cpu_baseline"]["kind"] in ("port", "reference")
    # no prose rides in the line
    def strings(o):
        if isinstance(o, dict):
            for v in o.values():
                yield from strings(v)
        elif isinstance(o, str):
            yield o
    assert max(len(x) for x in strings(rec)) <= 200


def test_committed_round6_line_parses():
    """profiles/r06_bench.json is the LAST stdout line of the builder's own round-6 run, byte for byte."""
    p = os.path.join(ROOT, "profiles", "r06_bench.json")
    if not os.path.exists(p):
        pytest.skip("no round-6 bench line committed yet")
    line = open(p).read().strip()
    assert "\n" not in line and len(line) < 8192
    rec = json.loads(line)
    assert rec["roofline"]["frac"] > 0 and rec["cpu_baseline"]["cores"] >= 1 and rec["ms_per_step"] > 0


def test_emit_prints_the_record_last_and_caps_it(tmp_path, monkeypatch):
    import bench
    full = _full_records()[-1][1]
    bloated = dict(full, commit_pipeline={"sections": {"sha512": dict(full["commit_pipeline"]["sections"]["sha512"])}},
                   other_scaling={f"k{i}": {"ms_per_step": 1.0, "value": 1.0, "proofs_total": 1, "error": "x" * 500} for i in range(40)})
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.emit(bloated)
    lines = buf.getvalue().strip().split("\n")
    assert lines[0].startswith("# bench_extras ") and len(lines) == 2
    assert len(lines[-1]) <= bench.LINE_CAP and json.loads(lines[-1])["roofline"]["frac"] == full["roofline"]["frac"]
    assert json.load(open(tmp_path / "bench_extras.json"))["metric"] == full["metric"]


def test_plain_run_options():
    """A plain run times the steps and nothing else; everything beside the headline needs --full."""
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse_args(["--steps", "3", "--full", "--dump-outputs", "out"])
    assert a.steps == 3 and a.full and a.dump_outputs == "out"


def test_dump_outputs_is_exact_and_small(tmp_path):
    """--dump-outputs: float64 files that carry the u64 elements exactly (sampled), exact per-row limb sums and the reports."""
    import numpy as np
    import torch
    import bench
    rng = np.random.default_rng(5)
    P, stride, count = 6, 1200, 1100
    u = rng.integers(0, 2**64 - 2**32 + 1, size=(P, stride), dtype=np.uint64)
    rows = torch.from_numpy(u.view(np.int64).copy())
    reps = rng.integers(0, 256, size=(P, 64), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), rows[:, :count], reps)
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == ["elems_row_sums.npy", "elems_sample.npy", "elems_sample_index.npy", "report_header.npy", "report_verdict.npy"]
    assert sum(p.stat().st_size for p in tmp_path.iterdir()) <= bench.DUMP_CAP
    got = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    idx = got["elems_sample_index"].astype(np.int64)
    assert idx.size == P * count and np.all(np.diff(idx) >= 0)
    s = got["elems_sample"]
    back = (s[:, 0].astype(np.uint64) << np.uint64(32)) | s[:, 1].astype(np.uint64)
    assert np.array_equal(back, u[:, :count].reshape(-1)[idx])
    want = np.stack([((u[:, :count] >> np.uint64(16 * k)) & np.uint64(0xFFFF)).sum(axis=1) for k in range(4)], axis=1)
    assert np.array_equal(got["elems_row_sums"], want.astype(np.float64))
    assert np.array_equal(got["report_header"], reps[:, :32].astype(np.float64))
    assert np.array_equal(got["report_verdict"][:, 2], reps[:, 40:44].copy().view(np.int32)[:, 0].astype(np.float64))
    # the same rows give the same files (the sample is seeded)
    again = tmp_path / "again"
    bench.dump_outputs(str(again), rows[:, :count], reps)
    assert all(np.array_equal(np.load(again / f), got[f[:-4]]) for f in files)
