"""The one-workgroup-per-proof kernels above N = 128 against the CPU oracle, bit for bit.

launch_proof (kernels.hip) runs one of three instantiations of proof_body<NMAX>: k_proof_r168 (N <= 128), k_proof (N <= 256, 256
threads) and k_proof_wide (N <= 512, 512 threads).  A batch reaches it only above the small path's bound (1536 lanes; 2048 for N <= 32)
AND above the 2048 lanes up to which k_proof runs as role workgroups, so the batches here are the smallest that do: n_proofs * N just
above 2048.  `Context.last_proof_path()` says which launch ran, and every test asserts it: if a lane threshold moves, these tests fail
instead of sliding back onto the small path (the fix then is another proof count, not a dropped assertion).

What differs from the N <= 128 instantiation and is exercised here: per-lane loops of one to three trips over 256 / 512 threads, the
u96 tallies carried across four / eight waves, the LDS hash table of 2 * NMAX slots of the trusted-key match, the odd-node promotions of
the fixed-shape validator tree at N = 129 / 200 / 257 / 300, the set cache's slot size, the leaves-first branch, and beside k_proof the
whole classic launch graph (EdDSA chain, verdict / wide tail, row serializer) at these N."""
import os
import struct

import numpy as np
import pytest

import test_fuzz_extended
from test_fuzz_extended import _mutated_batch
from test_gpu_parity import _check_vs_oracle
from test_value_differential import _assert_value, _bad_signature, _on_device, _value_device, _want

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 8)
CID = b"celestia"
NONE, TINY, ROLES, R168, K256, WIDE = range(6)          # _lib.PROOF_PATH_* (test_abi_codec.py checks them against include/tmx.h)
PATH_NAMES = ("none", "tiny", "roles", "r168", "k256", "wide")
# (N, proofs, the path the batch must take): just above the roles bound on each kernel, the bound itself, and the small path at N = 512
TABLE = [(129, 16, K256), (200, 11, K256), (256, 9, K256), (256, 8, ROLES), (257, 8, WIDE), (300, 7, WIDE), (512, 5, WIDE), (512, 3, TINY)]
ROUNDS = (0, 3, 0, 2**40 + 7, 1)


@pytest.fixture(scope="module")
def tmx(built_lib):
    import tendermintx_amd
    from tendermintx_amd import _lib
    assert (_lib.PROOF_PATH_NONE, _lib.PROOF_PATH_TINY, _lib.PROOF_PATH_ROLES, _lib.PROOF_PATH_R168, _lib.PROOF_PATH_K256,
            _lib.PROOF_PATH_WIDE) == (NONE, TINY, ROLES, R168, K256, WIDE)
    return tendermintx_amd


class _PathChecked:
    """a context whose witness_batch asserts the proof path after EVERY call (what _check_vs_oracle calls on its `ctx`)"""

    def __init__(self, ctx, path):
        self.ctx, self.path, self.calls = ctx, path, 0

    def witness_batch(self, *args):
        out = self.ctx.witness_batch(*args)
        got = self.ctx.last_proof_path()
        assert got == self.path, f"call {self.calls}: proof path {PATH_NAMES[got]}, expected {PATH_NAMES[self.path]}"
        self.calls += 1
        return out


def _assert_rows(elems, want, what):
    if not np.array_equal(elems, want):
        bad = np.argwhere(elems != want)
        raise AssertionError(f"{what}: GPU != oracle at (proof, element) {bad[:10].tolist()} ({len(bad)} differences)")


# ------------------------------------------------------------------------------------------------ a. every kernel, skip and step
def _kernel_cases():
    cases = [(kind, n, P, n, path) for kind in (0, 1) for n, P, path in TABLE]
    seen = set()
    for n, P, path in TABLE:       # a set one short of full (skip) and one two thirds full (step), once per N
        if n not in seen:
            seen.add(n)
            cases += [(0, n, P, n - 1, path), (1, n, P, (2 * n) // 3, path)]
    return cases


@pytest.mark.parametrize("kind,n,P,nb,path", _kernel_cases(),
                         ids=[f"{('skip', 'step')[c[0]]}-N{c[1]}x{c[2]}-nb{c[3]}-{PATH_NAMES[c[4]]}" for c in _kernel_cases()])
def test_rows_equal_the_oracle_on_each_kernel(tmx, oracle, kind, n, P, nb, path):
    """Every row of the table, skip and step, full and partially filled sets, 90 % signing, non-zero rounds: cold, warm (key cache and set
    cache), then a batch whose first quarter comes from another workload (new keys and new sets beside resident ones).  The last proof of
    each batch has the R of its first signing lane flipped: its report names that lane (first_bad_sig through the N > 64 ballots of the
    verdict), every other report is clean.  The proof path is the table's after every call."""
    from tendermintx_amd.synth import Workload
    wl = Workload(kind, n, P, nb, chain_id=CID, seed=7000 + 10 * n + P + kind, signed_permille=900, rounds=ROUNDS, n_sets=2, ensure_two_thirds=True)
    targets, lane = _bad_signature(wl.targets, n, P - 1)
    k = max(1, P // 4)
    fresh = Workload(kind, n, k, nb, chain_id=CID, seed=9000 + 10 * n + P + kind, signed_permille=900, rounds=ROUNDS, n_sets=2, ensure_two_thirds=True)
    mixed = (fresh.proofs + wl.proofs[k * 2336:], fresh.targets + targets[k * n * 256:], fresh.trusteds + wl.trusteds[k * n * 48:] if kind == 0 else None)
    with tmx.Context(n, CID, max_batch=P) as raw:
        ctx = _PathChecked(raw, path)
        for batch, repeat in (((wl.proofs, targets, wl.trusteds), 2), (mixed, 1)):
            _, reps = _check_vs_oracle(tmx, oracle, kind, n, *batch, CID, ctx=ctx, threads=THREADS, repeat=repeat)
            assert [r["first_bad_sig"] for r in reps] == [-1] * (P - 1) + [lane]
            assert [r["all_ok"] for r in reps] == [True] * (P - 1) + [False]
        assert ctx.calls == 3


# ------------------------------------------------------------------------------------------------ b. tallies and the key match at their edges
def _vlen(power):
    """bytes of the marshalled validator (key field + power field as a varint, omitted when zero)"""
    return 36 + (1 + (power.bit_length() + 6) // 7 if power else 0)


def _edge_batch(n, P):
    """Six hand-made skip proofs over N = n lanes (+ pristine ones up to P), each an edge of the tallies or of the trusted-key match:
      0  every target and trusted power 2^63 - 1, everybody signed, the trusted set = the target set reversed (every trusted lane matches:
         the hash table holds N keys, both u96 totals are N * (2^63 - 1); the circuit's u64 sums overflow, and the reports say so)
      1  the signed power EXACTLY two thirds of the total (strict >: fails), decided by the power of lane n - 1 (the last wave)
      2  that power one unit smaller (passes)        3  one unit larger (fails)
      4  every target lane carries ONE key, which the trusted set holds once (a probe run of N equal keys)
      5  nb = 1 for the target set, nbt = N for the trusted set
    Returns (proofs, targets, trusteds)."""
    from tendermintx_amd.synth import Workload
    assert P >= 6
    wl = Workload(0, n, P, n, chain_id=CID, seed=31000 + n, signed_permille=1000, rounds=(0, 1))
    pr, t, r = bytearray(wl.proofs), bytearray(wl.targets), bytearray(wl.trusteds)

    def tpow(p, lane, v):
        o = (p * n + lane) * 256
        t[o + 224:o + 232] = struct.pack("<Q", v)
        t[o + 222] = _vlen(v)

    big = 2**63 - 1
    for lane in range(n):
        tpow(0, lane, big)
    for j in range(n):
        src, dst = (n - 1 - j) * 256, j * 48
        r[dst:dst + 32] = t[src:src + 32]
        r[dst + 32:dst + 40] = struct.pack("<Q", big)
        r[dst + 40] = _vlen(big)
    # lanes 0 .. n-2 hold w each, u of them did not sign, s did; lane n-1 did not sign and holds x:  3 * s*w == 2 * (s*w + u*w + x)
    # (w small enough that 3 * the signed sum and 2 * the total stay below 2^64: the circuit's u64 products wrap, voting.rs:91-105)
    w = 2**50
    u = (n - 1) // 3 - 1
    s = n - 1 - u
    x = (s - 2 * u) * w // 2
    assert 0 < x and 3 * s * w == 2 * (s * w + u * w + x) and 3 * s * w < 2**64
    for p, dx in ((1, 0), (2, -1), (3, 1)):
        for lane in range(n - 1):
            tpow(p, lane, w)
        for lane in range(1, 3 * u, 3):
            t[(p * n + lane) * 256 + 223] &= 0xFE
        assert sum(1 for lane in range(n) if not t[(p * n + lane) * 256 + 223] & 1) == u
        tpow(p, n - 1, x + dx)
        t[(p * n + n - 1) * 256 + 223] &= 0xFE
    key = bytes(r[(4 * n + 5) * 48:(4 * n + 5) * 48 + 32])
    assert sum(1 for j in range(n) if bytes(r[(4 * n + j) * 48:(4 * n + j) * 48 + 32]) == key) == 1
    for lane in range(n):
        t[(4 * n + lane) * 256:(4 * n + lane) * 256 + 32] = key
    pr[5 * 2336 + 56:5 * 2336 + 64] = struct.pack("<II", 1, n)
    return bytes(pr), bytes(t), bytes(r)


@pytest.mark.parametrize("n,P,path", [(256, 9, K256), (512, 6, WIDE)], ids=["N256x9-k256", "N512x6-wide"])
def test_tally_and_match_edges_across_waves(tmx, oracle, n, P, path):
    """_edge_batch on k_proof (four waves) and k_proof_wide (eight): rows and reports (all_ok, fail_mask, gt_target, gt_trusted, every
    other field) equal the oracle's, cold and warm.  The threshold verdicts are the ones strict > gives, so the oracle's verdicts are not
    a constant: some cases pass and some fail.  (N = 512 runs six proofs, one more than the table's five: one proof per case.)"""
    proofs, targets, trusteds = _edge_batch(n, P)
    with tmx.Context(n, CID, max_batch=P) as raw:
        ctx = _PathChecked(raw, path)
        _, reps = _check_vs_oracle(tmx, oracle, 0, n, proofs, targets, trusteds, CID, ctx=ctx, threads=THREADS, repeat=2)
    for p, r in enumerate(reps):
        print(f"N {n} proof {p}: all_ok {r['all_ok']} fail_mask {r['fail_mask']:#x} gt_target {r['gt_target']} gt_trusted {r['gt_trusted']}")
    assert [reps[p]["gt_target"] for p in (1, 2, 3)] == [False, True, False]
    assert any(r["gt_target"] for r in reps) and not all(r["gt_target"] for r in reps)


# ------------------------------------------------------------------------------------------------ c. the validator-set cache
@pytest.mark.parametrize("n,P,nb", [(200, 12, 150), (300, 8, 300)], ids=["N200x12", "N300x8"])
def test_set_cache_above_128(tmx, oracle, monkeypatch, n, P, nb):
    """test_key_cache.py::test_validator_set_cache at the slot sizes and tree sizes of N = 200 (k_proof) and N = 300 (k_proof_wide): the
    first call computes 2 P sets, the second is served 2 P, one flipped byte of one lane's power is one new set (`served` counts the
    proofs whose sets were all resident), every call equals the
    oracle and a context without the cache.  Then an 8-slot cache (TMX_SET_CACHE_SETS) and twelve calls over sixteen target sets that differ
    in one byte: slots are evicted and refilled, rows equal the oracle every time, and the counters stay consistent."""
    from tendermintx_amd.synth import Workload
    wl = Workload(0, n, P, nb, chain_id=CID, seed=9300 + n, signed_permille=900, n_sets=3)
    path = K256 if n <= 256 else WIDE
    want, oreps = oracle.witness_batch(0, P, wl.proofs, wl.targets, wl.trusteds, n, CID, 100800, n_threads=THREADS)
    t2 = bytearray(wl.targets)
    t2[(5 * n + 17) * 256 + 224] ^= 1
    want3, oreps3 = oracle.witness_batch(0, P, wl.proofs, bytes(t2), wl.trusteds, n, CID, 100800, n_threads=THREADS)
    with tmx.Context(n, CID, max_batch=P) as ctx:
        e1, r1 = ctx.witness_batch(0, wl.proofs, wl.targets, wl.trusteds)
        s1 = ctx.set_cache_stats()
        assert ctx.last_proof_path() == path
        assert s1["served"] == 0 and s1["computed"] == 2 * P and 1 <= s1["resident"] <= 2 * P and s1["inserted"] == s1["resident"]
        e2, r2 = ctx.witness_batch(0, wl.proofs, wl.targets, wl.trusteds)
        s2 = ctx.set_cache_stats()
        assert s2["served"] == 2 * P and s2["computed"] == s1["computed"] and s2["resident"] == s1["resident"]
        _assert_rows(e1, want, "first call")
        _assert_rows(e2, want, "second call (served)")
        assert r1 == oreps and r2 == oreps
        e3, r3 = ctx.witness_batch(0, wl.proofs, bytes(t2), wl.trusteds)
        s3 = ctx.set_cache_stats()
        assert s3["computed"] == s2["computed"] + 1 and s3["served"] == s2["served"] + 2 * (P - 1) and s3["resident"] == s2["resident"] + 1
        _assert_rows(e3, want3, "one power byte flipped in proof 5")
        assert r3 == oreps3 and ctx.last_proof_path() == path
        del e1, e2, e3
    monkeypatch.setenv("TMX_SET_CACHE", "0")
    with tmx.Context(n, CID, max_batch=P) as ctx:
        e4, r4 = ctx.witness_batch(0, wl.proofs, wl.targets, wl.trusteds)
        assert ctx.set_cache_stats()["computed"] == 0 and ctx.last_proof_path() == path
        _assert_rows(e4, want, "TMX_SET_CACHE=0")
        assert r4 == oreps
        del e4
    monkeypatch.delenv("TMX_SET_CACHE")
    monkeypatch.setenv("TMX_SET_CACHE_SETS", "8")
    one = Workload(0, n, P, nb, chain_id=CID, seed=9400 + n, signed_permille=900, n_sets=1)

    def variant(call):      # proof q of call `call`: target set (3 * call + q) % 16 = the base set with one power byte of lane v changed
        t = bytearray(one.targets)
        for q in range(P):
            v = (3 * call + q) % 16
            t[(q * n + v) * 256 + 224] ^= 1 + v
        return bytes(t)

    with tmx.Context(n, CID, max_batch=P) as ctx:
        assert ctx.set_cache_stats()["capacity"] == 8
        for call in range(12):
            t = variant(call)
            _check_vs_oracle(tmx, oracle, 0, n, one.proofs, t, one.trusteds, CID, ctx=ctx, threads=THREADS)
            s = ctx.set_cache_stats()
            assert s["resident"] == s["inserted"] - s["evicted"] <= s["capacity"], (call, s)
        assert s["evicted"] > 0 and s["inserted"] > 8 and s["computed"] > 0, s
        assert ctx.last_proof_path() == path


# ------------------------------------------------------------------------------------------------ d. the schedule knobs
KNOBS_300 = [{"TMX_LEAVES": "1"}, {"TMX_SCHEDULE": "warm"}, {"TMX_SCHEDULE": "cold"}, {"TMX_SET_CACHE": "0"}, {"TMX_HASH_FIRST": "1"},
             {"TMX_TAIL_WIDE": "0"}, {"TMX_TAIL_WIDE": "1"}]
TWO_WORKGROUPS = {"TMX_TINY": "0", "TMX_PROOF_ROLES": "0"}


@pytest.fixture(scope="module")
def knob_batches(oracle):
    """(inputs, oracle rows, oracle reports) of the 300 x 7 batch every knob runs and of the 129 x 2 batch, computed once"""
    from tendermintx_amd.synth import Workload
    out = {}
    for n, P, nb in ((300, 7, 271), (129, 2, 129)):
        wl = Workload(0, n, P, nb, chain_id=CID, seed=4300 + n, signed_permille=900, rounds=ROUNDS, n_sets=2)
        want, oreps = oracle.witness_batch(0, P, wl.proofs, wl.targets, wl.trusteds, n, CID, 100800, n_threads=THREADS)
        want.setflags(write=False)
        out[n] = (wl.proofs, wl.targets, wl.trusteds, want, oreps)
    return out


KNOB_CASES = [(k, 300, 7, WIDE) for k in KNOBS_300] + [(TWO_WORKGROUPS, 300, 2, WIDE), (TWO_WORKGROUPS, 129, 2, K256)]


@pytest.mark.parametrize("knobs,n,P,path", KNOB_CASES,
                         ids=[",".join(f"{a}={b}" for a, b in c[0].items()) + f"-N{c[1]}x{c[2]}-{PATH_NAMES[c[3]]}" for c in KNOB_CASES])
def test_knobs_above_128(tmx, monkeypatch, knob_batches, knobs, n, P, path):
    """A knob changes a schedule, never a value: the leaves-first branch of k_proof_wide (P.leaves_done), both forced schedules, no set
    cache, the hash role first, both forms of the verdict's tail -- skip, 300 x 7, cold and warm against one oracle result.  With the small
    path and the role workgroups both off, the first two proofs run the one-workgroup kernel as a two-workgroup grid: k_proof_wide at
    N = 300, k_proof at N = 129."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)      # read at context creation
    proofs, targets, trusteds, want, oreps = knob_batches[n]
    proofs, targets, trusteds = proofs[:P * 2336], targets[:P * n * 256], trusteds[:P * n * 48]
    with tmx.Context(n, CID, max_batch=P) as ctx:
        for run in ("cold", "warm"):
            elems, reps = ctx.witness_batch(0, proofs, targets, trusteds)
            got = ctx.last_proof_path()
            assert got == path, f"{knobs} {run}: proof path {PATH_NAMES[got]}, expected {PATH_NAMES[path]}"
            _assert_rows(elems, want[:P], f"{knobs} {run}")
            assert reps == oreps[:P], (knobs, run)


# ------------------------------------------------------------------------------------------------ e. typed values and hint rows
@pytest.mark.parametrize("kind,n,P,path", [(0, 256, 9, K256), (1, 300, 7, WIDE)], ids=["skip-N256x9", "step-N300x7"])
def test_typed_value_and_hint_rows_above_128(tmx, oracle, kind, n, P, path):
    """The typed value (k_pack_value over the records of k_proof / k_proof_wide, no row buffer): SEC_ALL cold, SEC_HINT warm, SEC_ALL
    through the device entry point on a side stream, each byte for byte the oracle's value (a failure names part, lane and byte); and the
    hint-only u32 rows against the first hint_elem_count elements of the oracle's rows."""
    import torch
    from tendermintx_amd import _lib
    from tendermintx_amd.synth import Workload
    wl = Workload(kind, n, P, n - 3, chain_id=CID, seed=5200 + n, signed_permille=900, rounds=ROUNDS, n_sets=2)
    want = _want(oracle, kind, n, wl.proofs, wl.targets, wl.trusteds)
    rows_want, oreps = oracle.witness_batch(kind, P, wl.proofs, wl.targets, wl.trusteds, n, CID, 100800, n_threads=THREADS)
    dev = torch.device("cuda", 0)
    what = f"kind {kind}, N {n}, {P} proofs"
    with tmx.Context(n, CID, max_batch=P) as ctx:
        laya, layh = ctx.value_layout(kind, _lib.SEC_ALL), ctx.value_layout(kind, _lib.SEC_HINT)
        got, _ = ctx.inputs_value_batch(kind, wl.proofs, wl.targets, wl.trusteds, _lib.SEC_ALL)
        assert ctx.last_proof_path() == path
        _assert_value(got, want, laya, kind, n, f"{what}: SEC_ALL cold")
        got, _ = ctx.inputs_value_batch(kind, wl.proofs, wl.targets, wl.trusteds, _lib.SEC_HINT)
        assert ctx.last_proof_path() == path
        _assert_value(got, want[:, :layh.bytes], layh, kind, n, f"{what}: SEC_HINT warm")
        st = torch.cuda.Stream(dev)
        got = _value_device(ctx, kind, P, _on_device(dev, wl.proofs, wl.targets, wl.trusteds), _lib.SEC_ALL, st.cuda_stream)
        assert ctx.last_proof_path() == path
        _assert_value(got, want, laya, kind, n, f"{what}: SEC_ALL, device entry point on a side stream")
        rows, reps = ctx.witness_batch_hint(kind, wl.proofs, wl.targets, wl.trusteds)
        assert ctx.last_proof_path() == path
        h = ctx.hint_elem_count(kind)
        assert rows.dtype == np.uint32
        _assert_rows(rows.astype(np.uint64), rows_want[:, :h], f"{what}: hint-only u32 rows")
        assert reps == oreps


# ------------------------------------------------------------------------------------------------ f. mutated batches
FUZZ_N = (200, 256, 300, 512)
FUZZ_MAX_LANES = 6144


def _glued_above_roles(n, s0):
    """_mutated_batch batches of one kind at N = n (seeds s0, s0 + 1, ...) glued until the lanes exceed the roles bound, cut at FUZZ_MAX_LANES;
    chain id and skip_max are the first batch's"""
    saved = test_fuzz_extended.NSET
    try:
        test_fuzz_extended.NSET = (n,)       # (NSET's default stays: it fixes the draws of every seeded test of that file)
        kind, _, proofs, targets, trusteds, chain_id, skip_max = _mutated_batch(s0)
        for s1 in range(s0 + 1, s0 + 400):
            if len(proofs) // 2336 * n > 2048:
                break
            k2, _, p2, t2, r2, _, _ = _mutated_batch(s1)
            if k2 == kind:
                proofs, targets = proofs + p2, targets + t2
                trusteds = trusteds + r2 if trusteds is not None else None
    finally:
        test_fuzz_extended.NSET = saved
    P = min(len(proofs) // 2336, FUZZ_MAX_LANES // n)
    assert P * n > 2048
    return kind, proofs[:P * 2336], targets[:P * n * 256], trusteds[:P * n * 48] if trusteds is not None else None, chain_id, skip_max


@pytest.mark.parametrize("seed", range(24))
def test_mutated_batches_above_128(tmx, oracle, seed):
    """Hostile inputs (test_fuzz_extended._mutated_batch: random and extreme bytes, lengths, flags, powers, duplicated and small-order keys,
    non-canonical scalars) on k_proof and k_proof_wide, six seeds per N: rows and reports equal the oracle's, cold and warm, whatever the
    verdicts are."""
    n = FUZZ_N[seed // 6]
    kind, proofs, targets, trusteds, chain_id, skip_max = _glued_above_roles(n, 300000 + 1000 * seed)
    P = len(proofs) // 2336
    with tmx.Context(n, chain_id, skip_max, max_batch=P) as raw:
        ctx = _PathChecked(raw, K256 if n <= 256 else WIDE)
        _check_vs_oracle(tmx, oracle, kind, n, proofs, targets, trusteds, chain_id, skip_max, ctx=ctx, threads=THREADS, repeat=2)
        assert ctx.calls == 2


# ------------------------------------------------------------------------------------------------ g. the shape BASELINE.md quotes
def test_n512_by_32_proofs(tmx, oracle):
    """BASELINE configs[4]'s batch shape: N = 512, 32 proofs (16 384 lanes), 400 validators, one cold and one warm call, every row and
    report against the oracle (0.55 GB of rows per call: compared run by run, each result freed before the next), every proof passes,
    k_proof_wide ran."""
    from tendermintx_amd.synth import Workload
    n, P = 512, 32
    wl = Workload(0, n, P, 400, chain_id=CID, seed=0x544D58 + n, signed_permille=900, n_sets=4, ensure_two_thirds=True)
    want, oreps = oracle.witness_batch(0, P, wl.proofs, wl.targets, wl.trusteds, n, CID, 100800, n_threads=THREADS)
    assert all(r["all_ok"] for r in oreps)
    with tmx.Context(n, CID, max_batch=P) as ctx:
        for run in ("cold", "warm"):
            elems, reps = ctx.witness_batch(0, wl.proofs, wl.targets, wl.trusteds)
            assert ctx.last_proof_path() == WIDE, run
            _assert_rows(elems, want, run)
            assert reps == oreps, run
            del elems
