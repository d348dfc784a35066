"""The FRI, DEEP, grinding and batch proofs at the shapes where their kernels change behaviour: wide oracles (Tier A) and the measured
full-size shape itself (Tier B).  The yardsticks are the independent ones of tests/test_fri.py, test_deep.py, test_pow.py and
test_batch_fri.py: tests/fri_model.py, deep_model.py, pow_model.py, batch_model.py over the CPU oracle in oracle/c; none calls libtmx.

Tier A -- thousands of columns on 2^7 .. 2^11 rows, device proofs word for word against the models.  What each shape is for, and the
constants of the sources that the geometry depends on (test_wide_shapes_hit_the_intended_geometry recomputes it and reads the constants out
of the sources, so a change to one of them fails there first and says that the shapes must move):

  * DEEP_ROWS = 8 (fri.hip) and the 4096 waves of launch_deep_eval: tiles = ceil(N / (64 DEEP_ROWS)), chunks = min(n_cols, 4096 / tiles),
    columns per chunk = ceil(n_cols / chunks).  k_deep_eval loops over more than one column per block only when n_cols tiles > 4096.
      params(7, 4608, ...)   N = 64:   1 tile,  2304 chunks of 2 columns
      params(8, 4099, ...)   N = 64:   1 tile,  2050 chunks, the last with ONE column; R = 8192 with 4093 padding rows; 4099 = 16 * 256 + 3
      params(11, 2100, ...)  N = 1024: 2 tiles, 1050 chunks of 2 columns
  * FRI_MAX_QUERIES = 256 (fri.h), the workgroup of k_fri_verify, and DEEP_Y_THREADS = 256 (fri.hip) of k_deep_y / k_batch_y: a thread's
    share of the Y sums strides the columns by 256 and multiplies its running power by alpha^256 only when n_cols > 256; the padding check
    strides R - n_cols rows the same way.
  * the batch shapes: bparams([8, 8, 6], [2500, 700, 2100], ...) has two oracles of equal size, so k_fri_combine<true> accumulates at alpha
    offset 2500, and two groups; bparams([11, 7], [2100, 4608], ..., pow_bits=6) makes the group that ENTERS a layer the wide one, with grinding.
  * the 64-block cap of launch_merkle_open (poseidon.hip): k_merkle_open's grid-stride loop runs a second time only above 64 * 256 = 16384
    columns; that shape, (3 | 4, 16389, 1), lives in tests/test_merkle_open.py (MERKLE_SHAPES and the query-by-query rejection test).

Tier B -- 256 proofs at N = 128 (tools/deep_bench.py, fri_bench.py, batch_bench.py: bench_workload("survey8d", 128, 256), blow-up 8, cap
height 4, arity 4, final_log_max 5, 28 queries): the 2^18-row, 4608-column SHA-512 oracle alone, and beside the 2304-column TREE, SHA256 and
HEADER oracles (FULL_SIZE of tests/test_batch_fri.py).  The Python provers cannot run there; the Python verifiers can, so the device proofs
are held against size-independent properties: the independent verifier accepts all 28 queries against the device's cap, zeta is the model
transcript's, the nonce satisfies the model's condition and is the smallest one (pow_model.search over the candidates below it: all 2^16
bits' worth is affordable, so the smallest-nonce form is what is asserted), spot columns' openings equal deep_model.evaluate over the
pre-LDE trace column and their queried row words equal oracle.lde of that column, tampered proofs get the model's verdicts.  At this size
k_deep_eval runs 64 tiles x 64 chunks of 72 columns on the SHA-512 oracle (36, 18 and 5 columns per chunk on TREE, SHA256 and HEADER): the
spot columns sit either side of the first chunk boundary.

Wall time on an MI355X, measured per test (GPU part: witness, trace rows, commits, proves, device verifies, downloads; Python part: the
model verifiers, deep_model.evaluate, oracle.lde, the nonce search):
  workload, witness and trace rows (module fixture)   GPU 0.6 - 0.8 s
  test_full_size_single_commit[fri]                    GPU 0.1 - 0.7 s (the first prove grows the scratch)   Python 0.5 s
  test_full_size_single_commit[deep]                   GPU 0.1 s   Python 1.1 s
  test_full_size_single_commit[deep-pow16]             GPU 0.1 s   Python 2.0 s   (the nonce search is about half of it)
  test_full_size_single_tampering                      GPU 0.3 s   Python 1.7 s
  test_full_size_commit_set                            GPU 1.0 - 1.5 s   Python 9.3 s

Tier B is about 20 s in all and the Python side dominates it (the verifiers' cost is per query and per column, not per row; the largest
single item is deep_model.evaluate over 2^15 trace rows, run for eight oracle / proof pairs in the set test).  Tier A, where the Python
provers run, is about 75 s in one process: 6.7 - 8.4 s per 11x2100 case, 1 - 2.2 s per 7x4608 / 8x4099 case (the first case of a process
pays some 10 s of start-up on top), 9.6 s for the wide batch proof with grinding, 2.5 and 3.9 s for the two tamper tests.  Whole suite with both tiers: -m gpu 821 passed, 1 skipped (needs two
GPUs) in 441 s; -m "not gpu" 344 passed in 118 s.
"""
import contextlib
import os
import re
import time

import numpy as np
import pytest

import batch_model as bm
import deep_model as dm
import fri_model as fm
import pow_model as pw
from batch_model import bparams
from test_batch_fri import FULL_SIZE, _bprove, _bverify, _commit, _want
from test_batch_fri import _tamper_cases as _batch_tamper_cases
from test_deep import _deep_tamper_cases
from test_fri import _down, _sentinel, _shift, _tree, _up, params
from test_merkle_open import _section_geom

P = fm.P
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tendermintx_amd", "csrc")

# ---- Tier A shapes
WIDE_SINGLE = [params(7, 4608, 2, 1, 2, 1, 6), params(8, 4099, 3, 2, 3, 1, 6), params(11, 2100, 3, 1, 4, 2, 8)]
WIDE_BATCH = [bparams([8, 8, 6], [2500, 700, 2100], 2, 1, 2, 1, 6), bparams([11, 7], [2100, 4608], 3, 1, 4, 2, 8, pow_bits=6)]
# (deep, pow_bits): plain FRI, DEEP, and one grinding variant of each
VARIANTS = [(0, 0), (1, 0), (0, 5), (1, 7)]
# the constants the geometry is derived from, as the sources state them
DEEP_ROWS, DEEP_EVAL_WAVES, FRI_MAX_QUERIES, DEEP_Y_THREADS, OPEN_BLOCK_CAP, OPEN_BLOCK = 8, 4096, 256, 256, 64, 256


def _deep_eval_geometry(log_sub, n_cols):
    """(tiles, chunks, columns per chunk, columns of the last chunk) of launch_deep_eval"""
    tiles = ((1 << log_sub) + 64 * DEEP_ROWS - 1) // (64 * DEEP_ROWS)
    chunks = min(n_cols, max(1, DEEP_EVAL_WAVES // tiles))
    per = (n_cols + chunks - 1) // chunks
    chunks = (n_cols + per - 1) // per
    return tiles, chunks, per, n_cols - (chunks - 1) * per


def _single_id(p):
    return f"{p['log_n']}x{p['n_cols']}"


def _batch_id(p):
    return "+".join(f"{m}x{n}" for m, n in zip(p["log_n"], p["n_cols"])) + (f"-pow{p['pow_bits']}" if p["pow_bits"] else "")


def _variant_id(v):
    return ("deep" if v[0] else "fri") + (f"-pow{v[1]}" if v[1] else "")


def _wide_columns(oracle, p, seed):
    """LDE'd random columns; column 0 is a constant whose words are stored non-canonically (w + p) at every third row"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, P, (p["n_cols"], 1 << (p["log_n"] - p["log_blowup"])), dtype=np.uint64)
    base[0] = 97531
    ext = oracle.lde(base, p["log_blowup"]).reshape(p["n_cols"], -1).copy()
    ext[0, ::3] += np.uint64(P)
    return ext


def _wide_batch_columns(oracle, p, seed):
    return [_wide_columns(oracle, dict(log_n=m, n_cols=n, log_blowup=p["log_blowup"]), seed + 7 * k)
            for k, (m, n) in enumerate(zip(p["log_n"], p["n_cols"]))]


def _model_prove(oracle, p, deep, bits, cols):
    """(proof words, degree flag, zeta or None, nonce or None) of the model that matches the variant"""
    if bits:
        out = pw.prove(oracle, p, bits, deep, cols, _shift())
        return out[0], out[1], (out[3] if deep else None), out[2]
    if deep:
        proof, deg, zeta = dm.prove(oracle, p, cols, _shift())
        return proof, deg, zeta, None
    proof, deg = fm.prove(oracle, p, cols, _shift())
    return proof, deg, None, None


def _model_verify(oracle, p, deep, bits, cap, proof):
    if bits:
        return pw.verify(oracle, p, bits, deep, cap, proof, _shift())
    return (dm if deep else fm).verify(oracle, p, cap, proof, _shift())


def _proof_words(p, deep, bits):
    return fm.layout(p)["words"] + (dm.openings_words(p["n_cols"]) if deep else 0) + (1 if bits else 0)


def _bump(proof, at):
    bad = proof.copy()
    bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
    return bad


def _wide_opening_cases(n_cols, off_open=0):
    """(name, word offset, new value or None = another residue) of the three cases of a wide openings section at proof[off_open:]: a column
    between 256 and 511 (a second stride of the verifier's Y sums), the last column, the padding word at row R - 1 (the last stride of
    the padding check; in plane 0 -- the existing generators alter plane 3)"""
    R = 1 << dm.log_r(n_cols)
    assert n_cols > 511 and R > n_cols
    return [("opening of column 300", off_open + R + 300, None), ("opening of the last column", off_open + n_cols - 1, None),
            ("padding word at R - 1", off_open + R - 1, 1)]


def _apply(proof, at, value):
    if value is None:
        return _bump(proof, at)
    bad = proof.copy()
    bad[at] = np.uint64(value)
    return bad


# ---- CPU
def test_wide_shapes_hit_the_intended_geometry():
    """the shapes against the constants they were chosen for, and the constants against the sources: whoever changes DEEP_ROWS, the 4096 of
    launch_deep_eval, FRI_MAX_QUERIES, DEEP_Y_THREADS or the 64-block cap of launch_merkle_open is told here that the shapes must move"""
    src = {name: open(os.path.join(CSRC, name)).read() for name in ("fri.hip", "fri.h", "poseidon.hip")}
    assert re.search(r"constexpr int DEEP_ROWS = %d;" % DEEP_ROWS, src["fri.hip"])
    assert re.search(r"std::max<uint64_t>\(1, %d / tiles\)" % DEEP_EVAL_WAVES, src["fri.hip"])
    assert re.search(r"constexpr int DEEP_Y_THREADS = %d;" % DEEP_Y_THREADS, src["fri.hip"])
    assert re.search(r"FRI_MAX_QUERIES = %d\b" % FRI_MAX_QUERIES, src["fri.h"])
    assert re.search(r"\(\(uint64_t\)n_cols \+ %d\) / %d, %d\)" % (OPEN_BLOCK - 1, OPEN_BLOCK, OPEN_BLOCK_CAP), src["poseidon.hip"])
    geo = [_deep_eval_geometry(p["log_n"] - p["log_blowup"], p["n_cols"]) for p in WIDE_SINGLE]
    assert geo == [(1, 2304, 2, 2), (1, 2050, 2, 1), (2, 1050, 2, 2)]
    p = WIDE_SINGLE[1]
    assert 1 << dm.log_r(p["n_cols"]) == 8192 and 8192 - p["n_cols"] == 4093 > FRI_MAX_QUERIES and p["n_cols"] % FRI_MAX_QUERIES == 3
    for p in WIDE_SINGLE:
        assert p["n_cols"] > 2 * max(FRI_MAX_QUERIES, DEEP_Y_THREADS) and p["n_queries"] <= FRI_MAX_QUERIES
    a, b = (bm.layout(p) for p in WIDE_BATCH)
    assert a["group_of"] == [0, 0, 1] and a["n_groups"] == 2 and WIDE_BATCH[0]["n_cols"][0] == 2500  # the accumulating combine's alpha offset
    assert b["group_of"] == [0, 1] and b["layer_enter"].count(1) == 1 and WIDE_BATCH[1]["n_cols"][1] > WIDE_BATCH[1]["n_cols"][0]
    for p in WIDE_BATCH:
        assert all(n > 2 * max(FRI_MAX_QUERIES, DEEP_Y_THREADS) for n in p["n_cols"])
    assert [_deep_eval_geometry(m - 1, n)[1:] for m, n in zip(WIDE_BATCH[1]["log_n"], WIDE_BATCH[1]["n_cols"])] == [(1050, 2, 2), (2304, 2, 2)]
    # the measured shape: 64 tiles x 64 chunks of 72 columns; 36, 18 and 5 columns per chunk on the smaller oracles
    full = [_deep_eval_geometry(m - 3, n) for m, n in zip(FULL_SIZE["log_n"], FULL_SIZE["n_cols"])]
    assert full == [(64, 64, 72, 72), (64, 64, 36, 36), (32, 128, 18, 18), (8, 461, 5, 4)]
    import test_merkle_open as tmo
    assert any(n > OPEN_BLOCK * OPEN_BLOCK_CAP for _, n, _ in tmo.MERKLE_SHAPES)


def test_models_prove_and_verify_wide_shapes(oracle):
    """no device: the models prove one wide single shape (DEEP with grinding, so all three single models run) and one wide batch shape,
    their own verifiers accept every query, and an altered opening of a column beyond 256 rejects every query"""
    p, bits = WIDE_SINGLE[0], 5
    cols = _wide_columns(oracle, p, 11)
    proof, deg, nonce, zeta = pw.prove(oracle, p, bits, 1, cols, _shift())
    cap = oracle.poseidon_merkle(cols.reshape(-1), p["log_n"], p["n_cols"], p["cap_height"])[-(1 << p["cap_height"]):]
    assert deg and zeta[1] and int(proof[-1]) == nonce and proof.size == _proof_words(p, 1, bits)
    assert all(pw.verify(oracle, p, bits, 1, cap, proof, _shift()))
    name, at, value = _wide_opening_cases(p["n_cols"])[0]
    assert not any(pw.verify(oracle, p, bits, 1, cap, _apply(proof, at, value), _shift())), name
    b = WIDE_BATCH[0]
    bcols = _wide_batch_columns(oracle, b, 12)
    bproof, bdeg, bzeta, bnonce = bm.prove(oracle, b, bcols, _shift())
    L = bm.layout(b)
    caps = [oracle.poseidon_merkle(np.ascontiguousarray(c).reshape(-1), m, n, h)[-(1 << h):].reshape(-1)
            for c, m, n, h in zip(bcols, b["log_n"], b["n_cols"], L["cap_height_of"])]
    assert bdeg and bzeta[1] and bnonce is None and bproof.size == L["words"]
    assert all(bm.verify(oracle, b, caps, bproof, _shift()))
    name, at, value = _wide_opening_cases(b["n_cols"][2], L["off_open"][2])[0]
    assert not any(bm.verify(oracle, b, caps, _apply(bproof, at, value), _shift())), name


# ---- GPU, Tier A
def _dev():
    import torch
    return torch.device("cuda", 0)


GUARD = 64


def _guarded(words):
    """a sentinel-filled buffer with GUARD words either side of the proof"""
    return _sentinel(words + 2 * GUARD)


def _unguard(buf, words):
    """the proof out of its buffer, after checking that the words around it are untouched"""
    import torch
    torch.cuda.synchronize(_dev())
    want = _sentinel(GUARD)
    assert torch.equal(buf[:GUARD], want) and torch.equal(buf[GUARD + words:], want)
    return buf[GUARD:GUARD + words].clone()


def _device_prove(ctx, p, deep, bits, d_cols, d_lv):
    words = _proof_words(p, deep, bits)
    buf = _guarded(words)
    at = buf[GUARD:].data_ptr()
    if bits:
        ctx.pow_prove_device(p, bits, deep, d_cols.data_ptr(), d_lv.data_ptr(), at, 0)
    elif deep:
        ctx.deep_prove_device(p, d_cols.data_ptr(), d_lv.data_ptr(), at, 0)
    else:
        ctx.fri_prove_device(p, d_cols.data_ptr(), d_lv.data_ptr(), at, 0)
    return _unguard(buf, words)


def _device_verify(ctx, p, deep, bits, d_cap, d_proof):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    if bits:
        ctx.pow_verify_device(p, bits, deep, d_cap.data_ptr(), d_proof.data_ptr(), ok.data_ptr(), 0)
    elif deep:
        ctx.deep_verify_device(p, d_cap.data_ptr(), d_proof.data_ptr(), ok.data_ptr(), 0)
    else:
        ctx.fri_verify_device(p, d_cap.data_ptr(), d_proof.data_ptr(), ok.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    return ok.cpu().numpy()


@pytest.fixture(scope="module")
def ctx(built_lib):
    import tendermintx_amd as tmx
    c = tmx.Context(4, b"celestia")
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=_variant_id)
@pytest.mark.parametrize("p", WIDE_SINGLE, ids=_single_id)
def test_wide_caller_columns_equal_the_model(ctx, oracle, p, variant):
    """Tier A, single oracle (the geometry of each shape: the module docstring): the device proof equals the model's word for word, the
    words around it stay, the degree flag, zeta and the nonce agree, and every query is accepted by the device verifier and by the model's"""
    deep, bits = variant
    ext = _wide_columns(oracle, p, p["log_n"] * 1009 + p["n_cols"] + 10 * deep + bits)
    d_cols = _up(ext)
    d_lv, d_cap = _tree(ctx, p, d_cols)
    d_proof = _device_prove(ctx, p, deep, bits, d_cols, d_lv)
    assert ctx.fri_last_degree_ok()
    got = _down(d_proof)
    want, deg, zeta, nonce = _model_prove(oracle, p, deep, bits, ext)
    assert deg and got.size == want.size
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    if deep:
        assert ctx.deep_last_zeta() == zeta
    if bits:
        assert ctx.pow_last()[0] == nonce == int(got[-1])
    ok = _device_verify(ctx, p, deep, bits, d_cap, d_proof)
    assert (ok == 1).all(), ok
    assert all(_model_verify(oracle, p, deep, bits, _down(d_cap), got))


@pytest.mark.gpu
@pytest.mark.parametrize("p", WIDE_BATCH, ids=_batch_id)
def test_wide_batch_proof_equals_the_model(ctx, oracle, p):
    """Tier A, several oracles (two of equal size and two groups; the wide oracle entering a layer, with grinding): the device proof
    equals the model's word for word, degree flag, zeta and nonce included, and every query verifies on the device and in the model"""
    cols = _wide_batch_columns(oracle, p, sum(p["n_cols"]))
    d_cols, d_lv, d_caps = _commit(ctx, p, cols)
    d_proof = _bprove(ctx, p, d_cols, d_lv)
    assert ctx.fri_last_degree_ok()
    got = _down(d_proof)
    want, deg, zeta, nonce = bm.prove(oracle, p, cols, _shift())
    assert deg and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert ctx.deep_last_zeta() == zeta
    if p["pow_bits"]:
        assert ctx.pow_last()[0] == nonce == int(got[-1])
    ok = _bverify(ctx, p, d_caps, d_proof)
    assert (ok == 1).all(), ok
    assert all(bm.verify(oracle, p, _down(d_caps), got, _shift()))


@pytest.mark.gpu
def test_wide_tampering_single(ctx, oracle):
    """the tamper cases of tests/test_deep.py on the 4608-column DEEP proof, and three that need the width: an opening of column 300, an
    opening of the last column, the padding word at row R - 1 = 8191.  The device verdict vector equals the model's in every case."""
    p = WIDE_SINGLE[0]
    ext = _wide_columns(oracle, p, 4242)
    d_cols = _up(ext)
    d_lv, d_cap = _tree(ctx, p, d_cols)
    proof = _down(_device_prove(ctx, p, 1, 0, d_cols, d_lv))
    cap = _down(d_cap)
    assert (_device_verify(ctx, p, 1, 0, d_cap, _up(proof)) == 1).all()
    cases = _deep_tamper_cases(p, proof)
    assert {"init row", "opening", "padding word", "layer row", "index"} <= {c[0] for c in cases}
    cases += [(name, _apply(proof, at, value), None) for name, at, value in _wide_opening_cases(p["n_cols"])]
    for name, bad, fails in cases:
        model = dm.verify(oracle, p, cap, bad, _shift())
        assert model == [not (fails is None or q in fails) for q in range(p["n_queries"])], name
        assert [bool(x) for x in _device_verify(ctx, p, 1, 0, d_cap, _up(bad))] == model, name


@pytest.mark.gpu
def test_wide_tampering_batch(ctx, oracle):
    """the tamper cases of tests/test_batch_fri.py on the [2500, 700, 2100]-column proof (3 queries: the model verifier's cost is per
    query), and the three wide cases on the last oracle, the one of the second group: the device verdicts equal the model's"""
    p = dict(WIDE_BATCH[0], n_queries=3)
    cols = _wide_batch_columns(oracle, p, 777)
    d_cols, d_lv, d_caps = _commit(ctx, p, cols)
    proof = _down(_bprove(ctx, p, d_cols, d_lv))
    caps = _down(d_caps)
    assert (_bverify(ctx, p, d_caps, _up(proof)) == 1).all()
    cases = _batch_tamper_cases(p, proof)
    assert {"oracle 1 row", "oracle 2 opening", "oracle 2 padding word", "layer row", "index"} <= {c[0] for c in cases}
    cases += [(name + " of oracle 2", _apply(proof, at, value), None)
              for name, at, value in _wide_opening_cases(p["n_cols"][2], bm.layout(p)["off_open"][2])]
    for name, bad, fails in cases:
        model = bm.verify(oracle, p, caps, bad, _shift())
        assert model == _want(p, fails), name
        assert [bool(x) for x in _bverify(ctx, p, d_caps, _up(bad))] == model, name


# ---- GPU, Tier B: 256 proofs at N = 128
FULL = dict(n=128, proofs=256, log_blowup=3, cap_height=4, arity_bits=4, final_log_max=5, n_queries=28, pow_bits=16)
SHA512, TREE, SHA256, HEADER = 2, 16, 4, 32  # TMX_TRACE_* section bits
FULL_ORDER = [SHA512, TREE, SHA256, HEADER]   # by decreasing rows, ties by ascending bit: the oracle order of FULL_SIZE


class _Clock:
    """wall time of a test split into its GPU part and its Python-verifier part; printed when the test ends"""

    def __init__(self, name):
        self.name, self.t = name, {"gpu": 0.0, "python": 0.0}

    @contextlib.contextmanager
    def part(self, which):
        import torch
        t0 = time.perf_counter()
        try:
            yield
        finally:
            if which == "gpu":
                torch.cuda.synchronize(_dev())
            self.t[which] += time.perf_counter() - t0

    def report(self):
        print(f"\n[tier B wall time] {self.name}: GPU part {self.t['gpu']:.1f} s, Python part {self.t['python']:.1f} s", flush=True)


@pytest.fixture(scope="module")
def full(built_lib):
    """the bench tools' workload, witness and trace rows, computed once: (context, trace block [proofs][trace words] on the device)"""
    import torch
    import tendermintx_amd as tmx
    from tendermintx_amd import _lib
    from tendermintx_amd.synth import bench_workload
    t0 = time.perf_counter()
    n, n_proofs = FULL["n"], FULL["proofs"]
    w = bench_workload("survey8d", n, n_proofs, seed=0x544D58)
    dev = _dev()
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    ctx = tmx.Context(n, b"celestia", 100800, device=0, max_batch=n_proofs)
    out = torch.empty(n_proofs * ctx.elem_stride(0), dtype=torch.int64, device=dev)
    rep = torch.empty(n_proofs * 64, dtype=torch.uint8, device=dev)
    tr = torch.zeros((n_proofs, ctx.trace_elem_count(0)), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(0, n_proofs, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(0, n_proofs, d[1].data_ptr(), d[2].data_ptr(), tr.data_ptr(), _lib.TRACE_ALL, 0)
    torch.cuda.synchronize(dev)
    del out, rep
    print(f"\n[tier B wall time] workload, witness and trace rows: GPU part {time.perf_counter() - t0:.1f} s", flush=True)
    yield ctx, tr
    ctx.close()
    del tr
    torch.cuda.empty_cache()


def _full_params(log_m, n_cols):
    return params(log_m, n_cols, FULL["cap_height"], FULL["log_blowup"], FULL["arity_bits"], FULL["final_log_max"], FULL["n_queries"])


def _commit_section(ctx, tr, section):
    """tmx_trace_commit_device of one section: (FRI parameters of the commit, the cap on the device)"""
    cap = _sentinel(4 << FULL["cap_height"])
    ctx.trace_commit_device(0, FULL["proofs"], section, FULL["log_blowup"], FULL["cap_height"], tr.data_ptr(), cap.data_ptr(), 0)
    log_m, n_cols, ch = ctx.trace_commit_last_shape()
    assert ch == FULL["cap_height"]
    return _full_params(log_m, n_cols), cap


def _spot_columns(log_m, n_cols):
    """8 columns: the first, the last, the two either side of the first k_deep_eval chunk boundary, and four in between"""
    per = _deep_eval_geometry(log_m - FULL["log_blowup"], n_cols)[2]
    assert 1 < per < n_cols // 4
    return sorted({0, per - 1, per, n_cols // 4 + 1, n_cols // 2 - 1, n_cols // 2, (3 * n_cols) // 4 + 5, n_cols - 1})


def _trace_columns(tr, section, log_m, pick):
    """the pre-LDE trace columns `pick` of a section, sliced out of the trace block ON THE DEVICE (natural rows, zero padded): column c is
    cell c % width of proof c // width (tmx_trace_commit_device's first stage)"""
    off, rows, width = _section_geom(0, FULL["n"], section)
    cols = np.zeros((len(pick), 1 << (log_m - FULL["log_blowup"])), dtype=np.uint64)
    for k, c in enumerate(pick):
        cols[k, :rows] = _down(tr[c // width, off:off + rows * width].view(rows, width)[:, c % width].contiguous())
    return cols


def _check_spot(oracle, section, tr, log_m, n_cols, zs, openings, indices, rows, want_openings=True):
    """openings: [(y0, y1)] per column of the proof; indices: the queried rows of THIS oracle; rows: [n_queries][n_cols] opened words"""
    pick = _spot_columns(log_m, n_cols)
    assert len(pick) >= 8
    cols = _trace_columns(tr, section, log_m, pick)
    assert cols.any()  # (not a block of zeros)
    if want_openings:
        ys = dm.evaluate(oracle, cols, 1, zs)
        assert [openings[c] for c in pick] == [tuple(y) for y in ys], section
    ext = oracle.lde(cols, FULL["log_blowup"]).reshape(len(pick), -1)
    for k, c in enumerate(pick):
        assert np.array_equal(rows[:, c], ext[k, indices]), (section, c)


def _full_tamper_cases(n_cols, n_queries, off_open, off_rows, off_paths, path_len):
    """(name, word offset, new value or None = another residue, queries that must fail or None = all)"""
    R = 1 << dm.log_r(n_cols)
    q_row, q_path = 5 % n_queries, 11 % n_queries
    return [("opening of the last column", off_open + 3 * R + n_cols - 1, None, None),
            ("row word of the last column", off_rows + q_row * n_cols + n_cols - 1, None, {q_row}),
            ("top path digest", off_paths + q_path * path_len * 4 + 4 * (path_len - 1) + 2, None, {q_path}),
            ("padding word at R - 1", off_open + 2 * R + R - 1, 1, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [(0, 0), (1, 0), (1, 16)], ids=_variant_id)
def test_full_size_single_commit(full, oracle, variant):
    """Tier B, the SHA-512 section alone (2^18 rows x 4608 columns): the FRI proof, the DEEP proof and the 16-bit grinding DEEP proof over
    tmx_trace_commit_device.  The degree flag is true; the matching model verifier accepts all 28 queries of the downloaded proof against
    the device's cap, and so does the device verifier; zeta is the one the model transcript draws from the parameters and the cap; the
    nonce is the smallest one that satisfies the model's condition (pow_model.search from 0 over the verifier's own grinding point).
    DEEP: the spot columns' openings equal deep_model.evaluate over the pre-LDE trace column; every variant: their 28 queried row words
    equal oracle.lde of that column."""
    ctx, tr = full
    deep, bits = variant
    clock = _Clock(f"single commit, {_variant_id(variant)}")
    with clock.part("gpu"):
        p, d_cap = _commit_section(ctx, tr, SHA512)
        assert (p["log_n"], p["n_cols"]) == (FULL_SIZE["log_n"][0], FULL_SIZE["n_cols"][0])
        words = _proof_words(p, deep, bits)
        buf = _guarded(words)
        if bits:
            ctx.trace_commit_pow_device(p, bits, deep, buf[GUARD:].data_ptr(), 0)
        elif deep:
            ctx.trace_commit_deep_device(p, buf[GUARD:].data_ptr(), 0)
        else:
            ctx.trace_commit_fri_device(p, buf[GUARD:].data_ptr(), 0)
        d_proof = _unguard(buf, words)
        assert ctx.fri_last_degree_ok() is True
        zeta = ctx.deep_last_zeta() if deep else None
        nonce = ctx.pow_last()[0] if bits else None
        ok = _device_verify(ctx, p, deep, bits, d_cap, d_proof)
        got, cap = _down(d_proof), _down(d_cap)
    assert (ok == 1).all(), ok
    with clock.part("python"):
        assert all(_model_verify(oracle, p, deep, bits, cap, got)) and p["n_queries"] == 28
        if deep:
            assert zeta == dm._start(oracle, p, cap)[1] and zeta[1] != 0
        if bits:
            assert nonce == int(got[-1])
            at = pw.grind_point(oracle, p, bits, deep, cap, got, _shift())
            assert pw.search(oracle, at, bits) == nonce  # the smallest satisfying nonce: every candidate below it was tried
        L = fm.layout(p)
        head = dm.openings_words(p["n_cols"]) if deep else 0
        idx = got[head + L["off_indices"]:head + L["off_indices"] + p["n_queries"]].astype(np.int64)
        rows = got[head + L["off_init_rows"]:head + L["off_init_rows"] + p["n_queries"] * p["n_cols"]].reshape(p["n_queries"], p["n_cols"])
        _check_spot(oracle, SHA512, tr, p["log_n"], p["n_cols"], dm.points(oracle, p, zeta) if deep else None,
                    dm.openings_of(p, got) if deep else None, idx, rows, want_openings=bool(deep))
    clock.report()


@pytest.mark.gpu
def test_full_size_single_tampering(full, oracle):
    """Tier B: an opening of the last column, a row word of the last column, the top path digest of one query and the padding word at row
    R - 1 of the full-size DEEP proof: the device verdicts equal the model's, which are the expected ones"""
    ctx, tr = full
    clock = _Clock("single commit, tampering")
    with clock.part("gpu"):
        p, d_cap = _commit_section(ctx, tr, SHA512)
        d_proof = _sentinel(dm.proof_words(p))
        ctx.trace_commit_deep_device(p, d_proof.data_ptr(), 0)
        proof, cap = _down(d_proof), _down(d_cap)
    L = fm.layout(p)
    head = dm.openings_words(p["n_cols"])
    for name, at, value, fails in _full_tamper_cases(p["n_cols"], p["n_queries"], 0, head + L["off_init_rows"], head + L["off_init_paths"],
                                                     p["log_n"] - p["cap_height"]):
        bad = _apply(proof, at, value)
        with clock.part("python"):
            model = dm.verify(oracle, p, cap, bad, _shift())
        assert model == [not (fails is None or q in fails) for q in range(p["n_queries"])], name
        with clock.part("gpu"):
            device = _device_verify(ctx, p, 1, 0, d_cap, _up(bad))
        assert [bool(x) for x in device] == model, name
    clock.report()


@pytest.mark.gpu
def test_full_size_commit_set(full, oracle):
    """Tier B, SHA512 + TREE + SHA256 + HEADER side by side (tmx_trace_commit_set_device), proved without and with 16 bits of grinding: the
    shape is FULL_SIZE; every cap equals the single commit's cap of that section; batch_model.verify and the device verifier accept all
    28 queries of both proofs; zeta is the model transcript's; the spot columns' openings and queried row words of EVERY oracle are
    deep_model.evaluate's and oracle.lde's, in both proofs; a second prove (after the four single commits) gives identical words; the four tamper cases
    on TREE, a non-first oracle, get the model's verdicts"""
    import torch
    ctx, tr = full
    clock = _Clock("commit set")
    n_or, cap_w = len(FULL_ORDER), 4 << FULL["cap_height"]
    with clock.part("gpu"):
        d_caps = _sentinel(n_or * cap_w)
        ctx.trace_commit_set_device(0, FULL["proofs"], sum(FULL_ORDER), FULL["log_blowup"], FULL["cap_height"], tr.data_ptr(), d_caps.data_ptr(), 0)
        shape, section_of = ctx.trace_commit_set_shape()
        assert section_of == FULL_ORDER
        p = dict(shape, arity_bits=FULL["arity_bits"], final_log_max=FULL["final_log_max"], n_queries=FULL["n_queries"], pow_bits=0)
        assert p == FULL_SIZE
        pg = dict(p, pow_bits=FULL["pow_bits"])
        L, Lg = bm.layout(p), bm.layout(pg)
        proofs, oks, zetas = [], [], []
        for q, lay in ((p, L), (pg, Lg)):
            buf = _guarded(lay["words"])
            ctx.trace_commit_set_prove_device(q, buf[GUARD:].data_ptr(), 0)
            proofs.append(_unguard(buf, lay["words"]))
            assert ctx.fri_last_degree_ok() is True
            zetas.append(ctx.deep_last_zeta())
            oks.append(_bverify(ctx, q, d_caps, proofs[-1]))
        nonce = ctx.pow_last()[0]
        for k, sec in enumerate(FULL_ORDER):  # the single commits: the same caps, section by section
            _, cap = _commit_section(ctx, tr, sec)
            torch.cuda.synchronize(_dev())
            assert torch.equal(cap, d_caps[k * cap_w:(k + 1) * cap_w]), sec
        again = _sentinel(L["words"])
        ctx.trace_commit_set_prove_device(p, again.data_ptr(), 0)  # (the single commits left the set intact)
        torch.cuda.synchronize(_dev())
        assert torch.equal(again, proofs[0])
        del again
        got, got_g, caps = _down(proofs[0]), _down(proofs[1]), _down(d_caps)
    assert (oks[0] == 1).all() and (oks[1] == 1).all(), oks
    with clock.part("python"):
        assert all(bm.verify(oracle, p, caps, got, _shift())) and all(bm.verify(oracle, pg, caps, got_g, _shift()))
        cap_list = [caps[k * cap_w:(k + 1) * cap_w] for k in range(n_or)]
        # (pow_bits is one of the scalars the transcript starts from: the two proofs have different zetas, openings and indices)
        assert zetas[0] == bm._start(oracle, p, cap_list)[1] and zetas[1] == bm._start(oracle, pg, cap_list)[1] and zetas[0] != zetas[1]
        assert nonce == int(got_g[Lg["off_nonce"]]) < P
        for k, sec in enumerate(FULL_ORDER):
            m, n = p["log_n"][k], p["n_cols"][k]
            for q, proof, lay, zeta in ((p, got, L, zetas[0]), (pg, got_g, Lg, zetas[1])):
                idx = (proof[lay["off_indices"]:lay["off_indices"] + 28] % np.uint64(1 << m)).astype(np.int64)
                rows = proof[lay["off_init_rows"][k]:lay["off_init_rows"][k] + 28 * n].reshape(28, n)
                _check_spot(oracle, sec, tr, m, n, bm._points(oracle, q, k, zeta), bm.openings_of(q, proof, k), idx, rows)
    k = 1  # TREE: 2^18 rows like SHA512, so the same group, behind alpha offset 4608
    for name, at, value, fails in _full_tamper_cases(p["n_cols"][k], 28, L["off_open"][k], L["off_init_rows"][k], L["off_init_paths"][k],
                                                     p["log_n"][k] - L["cap_height_of"][k]):
        bad = _apply(got, at, value)
        with clock.part("python"):
            model = bm.verify(oracle, p, caps, bad, _shift())
        assert model == _want(p, fails), name
        with clock.part("gpu"):
            device = _bverify(ctx, p, d_caps, _up(bad))
        assert [bool(x) for x in device] == model, name
    clock.report()
