"""Differential tests of the typed value of the hint (tmx_inputs_value_batch / tmx_inputs_value_batch_device, k_pack_value in value.hip)
against the oracle's value sink, byte for byte, at the schedules and sizes the element-row tests cover.

The value path is not the row path with another packer: it runs the Level-1 producer without a row buffer (no leaves-first, no fused rows,
no direct D.1b row writes, no serializer), so the lane, proof and report records k_pack_value gathers come from a producer configuration
of their own.  Covered here: mutated batches (test_fuzz_extended.py) cold and warm through every entry point, every schedule knob of
test_gpu_parity.py, the exact batch bench.py times and the throughput regime (the split tail, key- and set-cache hits), one context
serving value and row calls of every size in random order, and a value call above the 65 535 proofs one k_pack_value launch holds.

The oracle's hint-only value is a prefix of the full one (test_typed_value.py), so every batch's oracle values are computed once with the
derived part and sliced."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import test_fuzz_extended
from test_fuzz_extended import _mutated_batch
from test_gpu_parity import KNOBS, _check_vs_oracle
from test_typed_value import _oracle_value, expand_derived, expand_hint

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 8)
CID = b"celestia"


@pytest.fixture(scope="module")
def tmx(built_lib):
    import tendermintx_amd
    return tendermintx_amd


def _want(oracle, kind, n, proofs, targets, trusteds, chain_id=CID, skip_max=100800):
    """the oracle's values of a batch WITH the derived part (np.uint8 [P, bytes]): _oracle_value over chunks of proofs on a thread pool
    (the oracle's C calls release the GIL)"""
    P = len(proofs) // 2336
    step = -(-P // THREADS)
    chunk = lambda p0: _oracle_value(oracle, kind, proofs[2336 * p0:2336 * (p0 + step)], targets[256 * n * p0:256 * n * (p0 + step)],
                                     trusteds[48 * n * p0:48 * n * (p0 + step)] if trusteds else None, n, chain_id, skip_max, True)
    with ThreadPoolExecutor(THREADS) as ex:
        return np.concatenate(list(ex.map(chunk, range(0, P, step))))


def _parts(lay, kind, n):
    """(name, first byte, bytes, bytes per lane / node or 0, unit) of every part of one proof's value, from tmx_value_layout"""
    tn = lay.tree_nodes
    parts = [("fixed", 0, lay.fixed_bytes, 0, ""), ("validators", lay.off_validators, 240 * n, 240, "lane")]
    if kind == 0:
        parts.append(("hash fields", lay.off_hashfields, 48 * n, 48, "lane"))
    if lay.off_proof_derived:
        parts.append(("target lanes", lay.off_target_lanes, 560 * n, 560, "lane"))
        if kind == 0:
            parts.append(("trusted lanes", lay.off_trusted_lanes, 112 * n, 112, "lane"))
        parts.append(("target nodes", lay.off_nodes_target, 32 * tn, 32, "node"))
        if kind == 0:
            parts.append(("trusted nodes", lay.off_nodes_trusted, 32 * tn, 32, "node"))
        parts.append(("proof-derived", lay.off_proof_derived, 976, 0, ""))
    return parts


def _where(lay, kind, n, byte):
    for name, first, size, unit, what in _parts(lay, kind, n):
        if first <= byte < first + size:
            rel = byte - first
            return f"{name} {what} {rel // unit} byte {rel % unit}" if unit else f"{name} byte {rel}"
    return f"value byte {byte} (in no part)"


def _assert_value(got, want, lay, kind, n, what, proof_ids=None):
    """got == want byte for byte, else a failure that names the proof, the value part, the lane (or tree node) and the byte of the first
    differences, and how many bytes differ; proof_ids: the proof number of each row when the rows are a subset of the batch"""
    assert got.shape == want.shape and want.shape[1] == lay.bytes, (what, got.shape, want.shape, lay.bytes)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    pid = (lambda r: int(proof_ids[r])) if proof_ids is not None else int
    lines = [f"proof {pid(r)}, {_where(lay, kind, n, int(b))}: got 0x{int(got[r, b]):02x}, want 0x{int(want[r, b]):02x}" for r, b in bad[:8]]
    raise AssertionError(f"{what}: {len(bad)} value bytes differ in {len(np.unique(bad[:, 0]))} of {want.shape[0]} proofs\n  " + "\n  ".join(lines))


def _report(kind, value):
    """the tmx_report packed at the end of a value's fixed part"""
    from tendermintx_amd import _lib
    fixed = _lib.SkipInputsFixed if kind == 0 else _lib.StepInputsFixed
    return fixed.from_buffer_copy(bytes(value[:C.sizeof(fixed)])).report


def _pinned(ctx, *bufs):
    """page-locked copies of the input records (None stays None)"""
    out = []
    for b in bufs:
        if b is None:
            out.append(None)
            continue
        a = ctx.host_alloc(len(b))
        a[:] = np.frombuffer(b, dtype=np.uint8)
        out.append(a)
    return out


def _bad_signature(targets, n, p):
    """the targets with R of the first signing lane of proof p flipped in one bit (its equation fails: the proof's verdict changes)"""
    t = bytearray(targets)
    lane = next(l for l in range(n) if t[(p * n + l) * 256 + 223] & 1)
    t[(p * n + lane) * 256 + 40] ^= 0x10
    return bytes(t), lane


def _on_device(dev, *bufs):
    import torch
    return [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b is not None else None for b in bufs]


def _value_device(ctx, kind, P, d, sections, stream, fill=0x5A):
    """tmx_inputs_value_batch_device on `stream` into a fresh device buffer (filled with `fill`: bytes the kernel leaves are seen)"""
    import torch
    lay = ctx.value_layout(kind, sections)
    out = torch.full((P * lay.bytes,), fill, dtype=torch.uint8, device=d[0].device)
    torch.cuda.synchronize(d[0].device)     # (the inputs and `out` were written on torch's stream; calls on different streams are ordered by the caller)
    ctx.inputs_value_batch_device(kind, P, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr() if d[2] is not None else None, out.data_ptr(), sections,
                                  stream=stream)
    torch.cuda.synchronize(d[0].device)
    return out.cpu().numpy().reshape(P, lay.bytes)


# ------------------------------------------------------------------------------------------------ 1. value fuzz
FUZZ_SEEDS = int(os.environ.get("TMX_FUZZ_VALUE_SEEDS", "32"))


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_value_fuzz(tmx, oracle, seed):
    """A mutated batch of test_fuzz_extended.py (random and extreme bytes, message / validator lengths, flag bytes, powers, keys,
    signatures) on one context with its chain id and skip_max: SEC_ALL cold, SEC_HINT warm, SEC_ALL warm through page-locked buffers both
    ways, SEC_ALL through the device entry point on a stream of its own -- each equal to the oracle's value byte for byte."""
    import torch
    from tendermintx_amd import _lib
    kind, n, proofs, targets, trusteds, chain_id, skip_max = _mutated_batch(seed)
    P = len(proofs) // 2336
    want = _want(oracle, kind, n, proofs, targets, trusteds, chain_id, skip_max)
    dev = torch.device("cuda", 0)
    with tmx.Context(n, chain_id, skip_max, max_batch=P) as ctx:
        laya, layh = ctx.value_layout(kind, _lib.SEC_ALL), ctx.value_layout(kind, _lib.SEC_HINT)
        got, _ = ctx.inputs_value_batch(kind, proofs, targets, trusteds, _lib.SEC_ALL)
        _assert_value(got, want, laya, kind, n, f"seed {seed} (kind {kind}, N {n}, {P} proofs): SEC_ALL cold")
        got, _ = ctx.inputs_value_batch(kind, proofs, targets, trusteds, _lib.SEC_HINT)
        _assert_value(got, want[:, :layh.bytes], layh, kind, n, f"seed {seed}: SEC_HINT warm")
        pins = _pinned(ctx, proofs, targets, trusteds)
        out = ctx.host_alloc(P * laya.bytes)
        try:
            out[:] = 0xA5
            got, _ = ctx.inputs_value_batch(kind, *pins, _lib.SEC_ALL, out=out)
            _assert_value(got, want, laya, kind, n, f"seed {seed}: SEC_ALL warm, page-locked in and out")
        finally:
            for a in [out] + [p for p in pins if p is not None]:
                ctx.host_free(a)
        st = torch.cuda.Stream(dev)
        got = _value_device(ctx, kind, P, _on_device(dev, proofs, targets, trusteds), _lib.SEC_ALL, st.cuda_stream)
        _assert_value(got, want, laya, kind, n, f"seed {seed}: SEC_ALL, device entry point on a side stream")


# ------------------------------------------------------------------------------------------------ 2. every schedule knob
@pytest.fixture(scope="module")
def knob_batch(oracle):
    """test_schedule_knobs_give_the_same_bits' batch: 20 proofs x 128 lanes (100 validators), one corrupted signature in proof 0"""
    from tendermintx_amd.synth import Workload
    n, P = 128, 20
    wl = Workload(0, n, P, 100, chain_id=CID, seed=4242, signed_permille=850)
    targets = bytearray(wl.targets)
    lane = next(l for l in range(n) if targets[l * 256 + 223] & 1)
    targets[lane * 256 + 40] ^= 0x10
    return wl.proofs, bytes(targets), wl.trusteds, lane, _want(oracle, 0, n, wl.proofs, bytes(targets), wl.trusteds)


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_value_under_every_schedule_knob(tmx, monkeypatch, knob_batch, knobs):
    """Every knob of test_schedule_knobs_give_the_same_bits changes a schedule, never a value: the typed value of its batch, SEC_ALL cold
    and warm, then the (0, 1), (0, 4) and (3, 15) slices on the same context, equals the oracle's, and the report packed in the fixed part
    names the corrupted lane of proof 0 and no other."""
    from tendermintx_amd import _lib
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)      # read at context creation
    proofs, targets, trusteds, lane, want = knob_batch
    n, P = 128, 20
    with tmx.Context(n, CID, max_batch=P) as ctx:
        lay = ctx.value_layout(0, _lib.SEC_ALL)
        for run in ("cold", "warm"):
            got, _ = ctx.inputs_value_batch(0, proofs, targets, trusteds, _lib.SEC_ALL)
            _assert_value(got, want, lay, 0, n, f"{knobs} {run}")
            reps = [_report(0, v) for v in got]
            assert [r.first_bad_sig for r in reps] == [lane] + [-1] * (P - 1) and not reps[0].all_ok, (knobs, run)
        for p0, p1 in ((0, 1), (0, 4), (3, 15)):
            got, _ = ctx.inputs_value_batch(0, proofs[p0 * 2336:p1 * 2336], targets[p0 * n * 256:p1 * n * 256], trusteds[p0 * n * 48:p1 * n * 48], _lib.SEC_ALL)
            _assert_value(got, want[p0:p1], lay, 0, n, f"{knobs} proofs {p0}..{p1}", proof_ids=range(p0, p1))
            assert [_report(0, v).first_bad_sig for v in got] == ([lane] if p0 == 0 else [-1]) + [-1] * (p1 - p0 - 1)


# ------------------------------------------------------------------------------------------------ 3. the batch bench.py times, and the throughput regime
def test_timed_workload_values(tmx, oracle):
    """The exact batch bench.py times (synth.bench_workload("survey8d", 128, 256): 32 768 lanes, so the verdict runs on the side stream
    and joins through ev_tail) as values: page-locked in and out as bench.py's t_value, SEC_HINT and SEC_ALL each on a context of its own,
    cold, warm, warm; then the device entry point, the batch with one bad signature in proof 5 (every proof of this batch passes, so only a
    failing verdict shows whether the packed reports wait for the verdict on the side stream) and one proof on the warm context.  Every byte
    equals the oracle's; `last_dedup` and the key- and set-cache counters prove that the cold call built the tables and the warm ones ran
    from the caches."""
    import torch
    from tendermintx_amd import _lib
    from tendermintx_amd.synth import bench_workload
    n, P = 128, 256
    wl = bench_workload("survey8d", n, P, seed=0x544D58)
    want = _want(oracle, 0, n, wl.proofs, wl.targets, wl.trusteds)
    assert all(_report(0, v).all_ok for v in want)
    dev = torch.device("cuda", 0)
    for sections in (_lib.SEC_HINT, _lib.SEC_ALL):
        with tmx.Context(n, CID, max_batch=P) as ctx:
            lay = ctx.value_layout(0, sections)
            pins = _pinned(ctx, wl.proofs, wl.targets, wl.trusteds)
            out = ctx.host_alloc(P * ctx.value_layout(0, _lib.SEC_ALL).bytes)
            try:
                for run in range(3):
                    out[:] = 0xA5
                    sc0 = ctx.set_cache_stats()
                    got, _ = ctx.inputs_value_batch(0, *pins, sections, out=out)
                    _assert_value(got, want[:, :lay.bytes], lay, 0, n, f"sections {sections} run {run}, page-locked")
                    st, sc = ctx.key_cache_stats(), ctx.set_cache_stats()
                    assert ctx.last_dedup() == (401, True), (sections, run)
                    if run == 0:
                        assert (st["last_new_keys"], st["last_built_keys"], st["last_hit_lanes"]) == (401, 401, 0)
                        assert sc["served"] + sc["computed"] == 2 * P and sc["computed"] >= 8     # (4 target + 4 trusted sets)
                    else:
                        assert (st["last_new_keys"], st["last_hit_keys"], st["last_hit_lanes"]) == (0, 401, n * P)
                        assert sc["served"] == sc0["served"] + 2 * P and sc["computed"] == sc0["computed"]
            finally:
                for a in [out] + pins:
                    ctx.host_free(a)
            if sections == _lib.SEC_ALL:
                stream = torch.cuda.current_stream(dev)
                got = _value_device(ctx, 0, P, _on_device(dev, wl.proofs, wl.targets, wl.trusteds), _lib.SEC_ALL, stream.cuda_stream)
                _assert_value(got, want, lay, 0, n, "device entry point, warm")
                bad, lane = _bad_signature(wl.targets, n, 5)
                want_bad = want.copy()
                want_bad[5] = _oracle_value(oracle, 0, wl.proofs[5 * 2336:6 * 2336], bad[5 * n * 256:6 * n * 256], wl.trusteds[5 * n * 48:6 * n * 48], n, CID,
                                            100800, True)[0]
                assert _report(0, want_bad[5]).first_bad_sig == lane and not _report(0, want_bad[5]).all_ok
                got = _value_device(ctx, 0, P, _on_device(dev, wl.proofs, bad, wl.trusteds), _lib.SEC_ALL, stream.cuda_stream)
                _assert_value(got, want_bad, lay, 0, n, "device entry point, warm, a bad signature in proof 5")
                got, _ = ctx.inputs_value_batch(0, wl.proofs[:2336], wl.targets[:256 * n], wl.trusteds[:48 * n], _lib.SEC_ALL)
                _assert_value(got, want[:1], lay, 0, n, "one proof, warm")
                row, _ = oracle.witness(0, wl.proofs[:2336], wl.targets[:256 * n], wl.trusteds[:48 * n], CID, 100800)
                hint = ctx.hint_elem_count(0)
                assert np.array_equal(expand_hint(_lib, 0, n, got[0], lay), row[:hint])
                assert np.array_equal(expand_derived(_lib, 0, n, got[0], lay), row[hint:])


def test_throughput_regime_values(tmx, oracle):
    """The throughput regime's schedule (from 512 proofs x 128: the row writers' settings, the split tail; 640 x 128 = 81 920 lanes) on the
    value path, which has no row writers: the bench workload at 640 proofs through the device entry point, cold, warm, and warm with two
    proofs over new validator sets (new keys) in front and a bad signature in the last proof -- every value vs the oracle."""
    import torch
    from tendermintx_amd import _lib
    from tendermintx_amd.synth import Workload, bench_workload
    n, P = 128, 640
    wl = bench_workload("survey8d", n, P, seed=0x544D58 + P)
    fresh = Workload(0, n, 2, 90, chain_id=CID, seed=31337 + P, signed_permille=950, n_sets=2)
    want = _want(oracle, 0, n, wl.proofs, wl.targets, wl.trusteds)
    mixed = (fresh.proofs + wl.proofs[2 * 2336:], _bad_signature(fresh.targets + wl.targets[2 * n * 256:], n, P - 1)[0], fresh.trusteds + wl.trusteds[2 * n * 48:])
    want_mixed = np.concatenate([_want(oracle, 0, n, fresh.proofs, fresh.targets, fresh.trusteds), want[2:-1],
                                 _oracle_value(oracle, 0, mixed[0][-2336:], mixed[1][-256 * n:], mixed[2][-48 * n:], n, CID, 100800, True)])
    assert not _report(0, want_mixed[-1]).all_ok
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    with tmx.Context(n, CID, max_batch=P) as ctx:
        lay = ctx.value_layout(0, _lib.SEC_ALL)
        d = _on_device(dev, wl.proofs, wl.targets, wl.trusteds)
        for run, (batch, w) in enumerate(((d, want), (d, want), (_on_device(dev, *mixed), want_mixed))):
            got = _value_device(ctx, 0, P, batch, _lib.SEC_ALL, stream.cuda_stream)
            _assert_value(got, w, lay, 0, n, f"{P} proofs, run {run}")


# ------------------------------------------------------------------------------------------------ 4. one context, many different calls
CALLS = ("value pageable", "value page-locked", "value device", "rows", "hint rows")


def _mixed_plan(n_calls=60, seed=606):
    """(first seed, glued batches, call kind, sections) of every call of test_one_context_many_value_and_row_calls"""
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(0, 20000)), int(rng.integers(0, 4)), CALLS[int(rng.integers(0, len(CALLS)))], int(rng.integers(0, 2)))
            for _ in range(n_calls)]


def _glued_batch(n, s0, extra):
    """up to four mutated batches of one kind at N = n glued together (as test_one_context_many_different_calls builds them)"""
    saved = test_fuzz_extended.NSET
    try:
        test_fuzz_extended.NSET = (n,)
        kind, _, proofs, targets, trusteds, _, _ = _mutated_batch(s0)
        for k in range(extra):
            for s1 in range(s0 + 1 + 50 * k, s0 + 50 * (k + 1)):
                k2, _, p2, t2, r2, _, _ = _mutated_batch(s1)
                if k2 == kind:
                    proofs, targets = proofs + p2, targets + t2
                    trusteds = trusteds + r2 if trusteds is not None else None
                    break
    finally:
        test_fuzz_extended.NSET = saved
    return kind, proofs, targets, trusteds


def test_one_context_many_value_and_row_calls(tmx, oracle):
    """State carried between calls of ONE context (the event that ends a batch, scratch buffers, the value staging buffer,
    the caches, the small-launch path vs the launch graph): 60 calls of random kind -- values through pageable and page-locked host
    buffers and through the device entry point on two alternating streams, SEC_HINT and SEC_ALL; element rows and hint-only rows -- on
    mutated batches of 1 .. 92 proofs x 64 lanes, each equal to the oracle.  Page-locked outputs fall on both sides of the 1 MiB up to
    which k_pack_value writes host memory itself."""
    import torch
    from tendermintx_amd import _lib
    n = 64
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    lanes, pinned_bytes, seen = set(), set(), set()
    n_dev = 0
    with tmx.Context(n, CID, 100800, max_batch=96) as ctx:
        for it, (s0, extra, call, sec) in enumerate(_mixed_plan()):
            kind, proofs, targets, trusteds = _glued_batch(n, s0, extra)
            P = len(proofs) // 2336
            lanes.add(P * n)
            seen.add(call)
            what = f"call {it} ({call}, kind {kind}, {P} proofs, seed {s0})"
            if call == "rows":
                _check_vs_oracle(tmx, oracle, kind, n, proofs, targets, trusteds, CID, ctx=ctx)
                continue
            if call == "hint rows":
                want, oreps = oracle.witness_batch(kind, P, proofs, targets, trusteds, n, CID, 100800, n_threads=THREADS)
                rows, reps = ctx.witness_batch_hint(kind, proofs, targets, trusteds)
                h = ctx.hint_elem_count(kind)
                assert np.array_equal(rows.astype(np.uint64), want[:, :h]) and reps == oreps, what
                continue
            sections = (_lib.SEC_HINT, _lib.SEC_ALL)[sec]
            lay = ctx.value_layout(kind, sections)
            want = _want(oracle, kind, n, proofs, targets, trusteds)[:, :lay.bytes]
            if call == "value pageable":
                got, _ = ctx.inputs_value_batch(kind, proofs, targets, trusteds, sections)
            elif call == "value page-locked":
                pins = _pinned(ctx, proofs, targets, trusteds)
                out = ctx.host_alloc(P * lay.bytes)
                try:
                    out[:] = 0xA5
                    got, _ = ctx.inputs_value_batch(kind, *pins, sections, out=out)
                    got = got.copy()
                finally:
                    for a in [out] + [p for p in pins if p is not None]:
                        ctx.host_free(a)
                pinned_bytes.add(P * lay.bytes)
            else:
                got = _value_device(ctx, kind, P, _on_device(dev, proofs, targets, trusteds), sections, streams[n_dev & 1].cuda_stream)
                n_dev += 1
            _assert_value(got, want, lay, kind, n, what)
    assert seen == set(CALLS) and n_dev >= 2
    assert min(lanes) <= 1536 and max(lanes) > 2048                                   # the small path and the launch graph
    assert min(pinned_bytes) <= 1 << 20 < max(pinned_bytes)                            # both sides of the direct-write limit


# ------------------------------------------------------------------------------------------------ 5. more than 65 535 proofs in one call
def test_value_batch_above_the_grid_y_limit(tmx, oracle):
    """k_pack_value puts the proof on grid.y, which holds at most 65 535: launch_pack_value launches the proofs above in chunks with their
    first proof `proof0`.  A step context with N = 2 takes 65 540 proofs: four distinct proofs repeated in order (4 does not divide 65 535,
    so a chunk that restarted at proof 0 would write the wrong proof's value -- or leave the last five unwritten), SEC_HINT through the host
    entry point and SEC_ALL through the device entry point: every proof's value equals its oracle value."""
    import torch
    from tendermintx_amd import _lib
    from tendermintx_amd.synth import Workload
    n, P, period = 2, 65540, 4
    wl = Workload(1, n, period, 2, chain_id=CID, seed=6553, signed_permille=1000, rounds=(0, 1, 2, 3))
    base = _oracle_value(oracle, 1, wl.proofs, wl.targets, None, n, CID, 100800, True)           # four oracle calls
    assert len({v.tobytes() for v in base}) == period
    reps = -(-P // period)
    proofs, targets = (wl.proofs * reps)[:P * 2336], (wl.targets * reps)[:P * n * 256]
    dev = torch.device("cuda", 0)

    def check(got, lay, what):
        assert got.shape == (P, lay.bytes), what
        for r in range(period):
            rows = got[r::period]
            _assert_value(rows, np.broadcast_to(base[r, :lay.bytes], rows.shape), lay, 1, n, what, proof_ids=range(r, P, period))

    with tmx.Context(n, CID, 100800, max_batch=P) as ctx:
        layh, laya = ctx.value_layout(1, _lib.SEC_HINT), ctx.value_layout(1, _lib.SEC_ALL)
        got, _ = ctx.inputs_value_batch(1, proofs, targets, None, _lib.SEC_HINT)
        check(got, layh, f"{P} proofs, SEC_HINT, host entry point")
        del got
        got = _value_device(ctx, 1, P, _on_device(dev, proofs, targets, None), _lib.SEC_ALL, torch.cuda.current_stream(dev).cuda_stream)
        check(got, laya, f"{P} proofs, SEC_ALL, device entry point")
