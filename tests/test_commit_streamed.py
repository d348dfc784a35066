"""Streamed members of a commit set (include/tmx.h "streamed members of a commit set"): tmx_trace_commit_set_bytes,
tmx_trace_commit_set_streamed_device, and tmx_trace_commit_set_prove_device over a set that has them.  The yardstick is the RESIDENT set of
the same sections, which tests/test_batch_fri.py and tests/test_proof_shapes.py tie to tests/batch_model.py: caps, shape and every proof
word of a streamed set must equal the resident set's.  At full size (256 proofs, N = 128, blow-up 8), where a resident set with the
ladders does not fit the card, the five-section proof is held against the models directly.

Wall time of the full-size tests on one MI355X, as _Clock prints it (pytest -s):
  workload, witness and trace rows                      GPU 0.9 s (2.3 s with the workload's synthesis)
  test_full_size_one_section_both_ways                  GPU 0.4 s   Python 0.0 s
  test_full_size_five_sections_with_the_ladders         GPU 2.7 s   Python 16.5 s
The GPU tests of this file: 4 s at the small shapes, 23 s at full size; the model verification of both proofs stays in."""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest

import batch_model as bm
import deep_model as dm
import fri_model as fm
from test_batch_fri import _bverify, _want
from test_fri import _down, _sentinel, _shift, _up
from test_merkle_open import _section_geom, _trace_rows

P = fm.P
BAD_ARG = -1
LADDERS, SHA512, SHA256, TREE, HEADER = 1, 2, 4, 16, 32  # TMX_TRACE_* section bits
TABLES = (LADDERS, SHA512, SHA256, TREE, HEADER)
ALL = sum(TABLES)


# ---- CPU
@pytest.mark.parametrize("width", [9, 195, 260])
@pytest.mark.parametrize("chunk", [8, 24, 64])
def test_chunked_sponge_equals_hash_no_pad(width, chunk):
    """(1) the rule the streamed commit rests on: an overwrite-mode sponge that absorbs a row in chunks of a multiple of eight columns,
    its 12-word state carried from chunk to chunk, ends in hash_no_pad's digest (195 and 260 end in a short block)"""
    import poseidon_model as pm
    pos = pm.Poseidon()
    rng = np.random.default_rng(width * 100 + chunk)
    row = [int(x) % P for x in rng.integers(0, 2**63, width, dtype=np.uint64)]
    state = [0] * 12
    for c0 in range(0, width, chunk):
        part = row[c0:c0 + chunk]            # one chunk: what the device has of the row at a time
        assert len(part) % 8 == 0 or c0 + chunk >= width
        for off in range(0, len(part), 8):
            block = part[off:off + 8]
            state = pos.permute(block + state[len(block):])
    assert state[:4] == pos.hash_no_pad(row)
    if width % 8:  # a boundary off the multiple of eight gives another digest: the rule is needed
        cut = 12 if width > 12 else 4
        s = [0] * 12
        for part in (row[:cut], row[cut:]):
            for off in range(0, len(part), 8):
                block = part[off:off + 8]
                s = pos.permute(block + s[len(block):])
        assert s[:4] != pos.hash_no_pad(row)


def _digests(log_n, cap_height):
    return sum(1 << (log_n - k) for k in range(log_n - cap_height + 1))


def _shape(lib, kind, n_max, section):
    log_n, width = C.c_uint32(), C.c_uint32()
    assert lib.tmx_trace_commit_shape(kind, n_max, section, C.byref(log_n), C.byref(width)) == 0
    return log_n.value, width.value


def _resident_bytes(lib, kind, n_max, n_proofs, sections, log_blowup, cap_height):
    """cols + lde + levels per member, plus twice the largest extended member (tmx_trace_commit_set_device's rule)"""
    want = lde_max = 0
    for sec in TABLES:
        if sections & sec:
            log_n, width = _shape(lib, kind, n_max, sec)
            n_cols, log_m = n_proofs * width, log_n + log_blowup
            lde = (n_cols << log_m) * 8
            want += (n_cols << log_n) * 8 + lde + _digests(log_m, min(cap_height, log_m)) * 32
            lde_max = max(lde_max, lde)
    return want + 2 * lde_max


def test_bytes_formula(built_lib):
    """(2) host only: streamed = 0 is the resident formula; streaming the ladders at the full-size parameters saves at least their extended
    columns; bad arguments give 0"""
    from tendermintx_amd.context import trace_commit_set_bytes as nbytes
    for kind, n_max, n_proofs, sections, lb, cap in ((0, 4, 3, ALL, 3, 2), (1, 4, 2, SHA512 | HEADER, 2, 1), (0, 128, 256, ALL, 3, 4),
                                                     (0, 128, 256, ALL - LADDERS, 3, 4), (0, 32, 2, LADDERS, 1, 0)):
        for chunk in (8, 512):
            assert nbytes(kind, n_max, n_proofs, sections, 0, chunk, lb, cap) == _resident_bytes(built_lib, kind, n_max, n_proofs, sections, lb, cap)
    resident = nbytes(0, 128, 256, ALL, 0, 512, 3, 4)
    log_n, width = _shape(built_lib, 0, 128, LADDERS)
    assert (log_n, 256 * width) == (16, 16640)
    ext = ((256 * width) << (log_n + 3)) * 8
    for chunk in (256, 512, 1024, 2048):
        streamed = nbytes(0, 128, 256, ALL, LADDERS, chunk, 3, 4)
        assert 0 < streamed <= resident - ext, (chunk, streamed, resident)
    # a member that fits one chunk stays resident: the figure is the resident one
    assert nbytes(0, 4, 1, SHA256, SHA256, 16, 3, 2) == nbytes(0, 4, 1, SHA256, 0, 16, 3, 2)
    assert nbytes(0, 4, 3, ALL, ALL, 8, 3, 2) < nbytes(0, 4, 3, ALL, 0, 8, 3, 2)
    for sections, streamed, chunk in ((ALL, LADDERS, 0), (ALL, LADDERS, 12), (ALL, LADDERS, 4), (SHA512, LADDERS, 8), (SHA512, SHA512 | TREE, 8),
                                      (0, 0, 8), (8, 0, 8), (ALL | 64, 0, 8)):
        assert nbytes(0, 4, 3, sections, streamed, chunk, 3, 2) == 0, (sections, streamed, chunk)
    assert nbytes(0, 4, 0, ALL, 0, 8, 3, 2) == 0 and nbytes(0, 4, 3, ALL, 0, 8, 3, 99) == 0


# ---- GPU, small shapes: skip, N = 4, blow-up 8
def _dev():
    import torch
    return torch.device("cuda", 0)


GUARD = 64
KIND, N, LOG_BLOWUP, CAP_H = 0, 4, 3, 2
BIG = 1 << 20


def _guarded(words):
    return _sentinel(words + 2 * GUARD)


def _unguard(buf, words):
    """the proof out of its buffer, after checking that the words around it are untouched"""
    import torch
    torch.cuda.synchronize(_dev())
    want = _sentinel(GUARD)
    assert torch.equal(buf[:GUARD], want) and torch.equal(buf[GUARD + words:], want)
    return buf[GUARD:GUARD + words].clone()


def _n_tables(sections):
    return sum(1 for sec in TABLES if sections & sec)


def _commit(ctx, tr, n_proofs, sections, streamed, chunk, cap_h=CAP_H):
    """streamed is None: the resident entry point.  (caps on the device, shape, section_of)"""
    import torch
    d_caps = _sentinel(_n_tables(sections) * (4 << cap_h))
    if streamed is None:
        ctx.trace_commit_set_device(KIND, n_proofs, sections, LOG_BLOWUP, cap_h, tr.data_ptr(), d_caps.data_ptr(), 0)
    else:
        ctx.trace_commit_set_streamed_device(KIND, n_proofs, sections, streamed, chunk, LOG_BLOWUP, cap_h, tr.data_ptr(), d_caps.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    shape, section_of = ctx.trace_commit_set_shape()
    return d_caps, shape, section_of


def _prove(ctx, p):
    words = bm.layout(p)["words"]
    buf = _guarded(words)
    ctx.trace_commit_set_prove_device(p, buf[GUARD:].data_ptr(), 0)
    return _unguard(buf, words)


@pytest.mark.gpu
@pytest.mark.parametrize("n_proofs", [1, 3])
def test_streamed_caps_equal_the_resident_caps(built_lib, n_proofs):
    """(3) every row table alone (streamed: itself) and the set of five (streamed: all; the ladders only), chunks of 8, 24, 64 and 2^20
    columns (the last: nothing is wide enough to stream): caps and shape are tmx_trace_commit_set_device's word for word.  With three
    proofs the ladders have 195 columns: every chunk size leaves a short last block"""
    import torch
    import tendermintx_amd as tmx
    with tmx.Context(N, b"celestia", max_batch=n_proofs) as ctx:
        tr = _trace_rows(ctx, KIND, N, n_proofs, 4100 + n_proofs)
        cases = [(sec, sec) for sec in TABLES] + [(ALL, ALL), (ALL, LADDERS)]
        for sections, streamed in cases:
            want = _commit(ctx, tr, n_proofs, sections, None, 0)
            if sections == ALL:
                assert want[2] == [HEADER, LADDERS, SHA512, TREE, SHA256] and want[1]["log_n"] == [15, 14, 13, 13, 12]
                assert want[1]["n_cols"][1] == 65 * n_proofs
            for chunk in (8, 24, 64, BIG):
                got = _commit(ctx, tr, n_proofs, sections, streamed, chunk)
                assert torch.equal(got[0], want[0]), (sections, streamed, chunk)
                assert got[1:] == want[1:], (sections, streamed, chunk)
        got = _commit(ctx, tr, n_proofs, ALL, 0, 8)  # streamed = 0: the resident call
        assert torch.equal(got[0], want[0]) and got[1:] == want[1:]


PROOF_CASES = [(ALL, ALL), (ALL, LADDERS), (LADDERS | SHA512, LADDERS), (LADDERS | SHA512, LADDERS | SHA512), (SHA512 | TREE, TREE),
               (SHA512 | TREE, SHA512), (SHA512 | TREE, SHA512 | TREE)]


@pytest.mark.gpu
@pytest.mark.parametrize("pow_bits", [0, 8])
@pytest.mark.parametrize("chunk", [8, 64])
def test_streamed_proofs_equal_the_resident_proofs(built_lib, oracle, chunk, pow_bits):
    """(4) the five-section set (all streamed; the ladders only: a streamed oracle that is not the largest), LADDERS + SHA512, and
    SHA512 + TREE three ways (TREE streamed: added to a resident oracle's sum; SHA512 streamed: it opens the group; both): the proof of the
    streamed set equals the resident set's word for word, guard words intact, zeta equal, the degree flag true, every query accepted; a
    second prove gives the same words, also with a single tmx_trace_commit_device in between.  Once, the context's NTT domain is changed
    between commit and prove: the streamed prove still extends under the set's domain and equals the resident prove of the same sequence"""
    import torch
    import tendermintx_amd as tmx
    n_proofs = 3
    root7, shift7 = oracle.G7_DOMAIN
    with tmx.Context(N, b"celestia", max_batch=n_proofs) as ctx:
        tr = _trace_rows(ctx, KIND, N, n_proofs, 4200)
        for sections, streamed in PROOF_CASES:
            moved = (sections, streamed) == (ALL, LADDERS) and chunk == 8
            d_caps, shape, order = _commit(ctx, tr, n_proofs, sections, None, 0)
            p = dict(shape, arity_bits=2, final_log_max=2, n_queries=12, pow_bits=pow_bits)
            if moved:
                ctx.ntt_set_domain(root7, shift7)
            want = _prove(ctx, p)
            want_zeta = ctx.deep_last_zeta()
            if moved:
                ctx.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
            assert (_bverify(ctx, p, d_caps, want) == 1).all()
            got_caps, got_shape, got_order = _commit(ctx, tr, n_proofs, sections, streamed, chunk)
            assert torch.equal(got_caps, d_caps) and (got_shape, got_order) == (shape, order)
            if moved:
                ctx.ntt_set_domain(root7, shift7)
            got = _prove(ctx, p)
            assert ctx.fri_last_degree_ok() is True and ctx.deep_last_zeta() == want_zeta
            if moved:
                ctx.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
            diff = torch.nonzero(got != want).flatten()[:10].tolist()
            assert not diff, (sections, streamed, diff, bm.layout(p))
            ok = _bverify(ctx, p, got_caps, got)
            assert (ok == 1).all(), ok
            again = _prove(ctx, p)
            assert torch.equal(again, got)
            cap = _sentinel(4 << CAP_H)
            ctx.trace_commit_device(KIND, n_proofs, SHA256, LOG_BLOWUP, CAP_H, tr.data_ptr(), cap.data_ptr(), 0)  # a resident single commit in between
            again = _prove(ctx, p)
            assert torch.equal(again, got), (sections, streamed)


@pytest.mark.gpu
def test_streamed_validation(built_lib):
    """(5) bad chunk_cols / streamed: TMX_ERR_BAD_ARG with a message, nothing written to d_caps, and the previous set is gone"""
    import torch
    import tendermintx_amd as tmx
    from tendermintx_amd._lib import TmxError
    with tmx.Context(N, b"celestia", max_batch=2) as ctx:
        tr = _trace_rows(ctx, KIND, N, 2, 4300)
        for sections, streamed, chunk in ((ALL, LADDERS, 0), (ALL, LADDERS, 12), (ALL, LADDERS, 4), (ALL, 0, 0), (SHA512, LADDERS, 8),
                                          (SHA512 | TREE, SHA512 | SHA256, 8), (ALL, 8, 8), (ALL, 64, 8)):
            _commit(ctx, tr, 2, SHA512 | TREE, TREE, 8)  # a set to lose
            d_caps = _sentinel(5 * (4 << CAP_H))
            with pytest.raises(TmxError) as e:
                ctx.trace_commit_set_streamed_device(KIND, 2, sections, streamed, chunk, LOG_BLOWUP, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
            torch.cuda.synchronize(_dev())
            assert e.value.status == BAD_ARG and ("chunk_cols" in str(e.value) or "streamed" in str(e.value)), e.value
            assert torch.equal(d_caps, _sentinel(5 * (4 << CAP_H)))
            with pytest.raises(TmxError) as e:
                ctx.trace_commit_set_shape()
            assert e.value.status == BAD_ARG and "no commit set" in str(e.value)


# ---- GPU, full size: 256 proofs at N = 128 (the recipe of tests/test_proof_shapes.py's `full` fixture)
FULL = dict(n=128, proofs=256, log_blowup=3, cap_height=4, arity_bits=4, final_log_max=5, n_queries=28, pow_bits=16)
FULL_ORDER = [LADDERS, SHA512, TREE, SHA256, HEADER]  # by decreasing rows, ties by ascending bit
FULL_CHUNK = 512
DEEP_ROWS, DEEP_EVAL_WAVES = 8, 4096  # launch_deep_eval's geometry, as the sources state it


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
        print(f"\n[streamed wall time] {self.name}: GPU part {self.t['gpu']:.1f} s, Python part {self.t['python']:.1f} s", flush=True)


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
    print(f"\n[streamed wall time] workload, witness and trace rows: GPU part {time.perf_counter() - t0:.1f} s", flush=True)
    yield ctx, tr
    ctx.close()
    del tr
    torch.cuda.empty_cache()


def _full_commit(ctx, tr, sections, streamed):
    d_caps = _sentinel(_n_tables(sections) * (4 << FULL["cap_height"]))
    if streamed is None:
        ctx.trace_commit_set_device(0, FULL["proofs"], sections, FULL["log_blowup"], FULL["cap_height"], tr.data_ptr(), d_caps.data_ptr(), 0)
    else:
        ctx.trace_commit_set_streamed_device(0, FULL["proofs"], sections, streamed, FULL_CHUNK, FULL["log_blowup"], FULL["cap_height"], tr.data_ptr(),
                                             d_caps.data_ptr(), 0)
    shape, section_of = ctx.trace_commit_set_shape()
    p = dict(shape, arity_bits=FULL["arity_bits"], final_log_max=FULL["final_log_max"], n_queries=FULL["n_queries"], pow_bits=0)
    return d_caps, p, section_of


@pytest.mark.gpu
def test_full_size_one_section_both_ways(full):
    """(6) SHA-512 at full size (4608 columns of 2^18 extended rows: it fits resident) as a one-member set, resident and streamed in
    chunks of 512 columns: caps equal, proofs equal word for word"""
    import torch
    ctx, tr = full
    clock = _Clock("SHA-512 both ways")
    with clock.part("gpu"):
        caps_r, p, order = _full_commit(ctx, tr, SHA512, None)
        assert (p["log_n"], p["n_cols"], order) == ([18], [4608], [SHA512])
        want = _prove(ctx, p)
        zeta = ctx.deep_last_zeta()
        caps_s, p_s, order_s = _full_commit(ctx, tr, SHA512, SHA512)
        torch.cuda.synchronize(_dev())
        assert torch.equal(caps_s, caps_r) and (p_s, order_s) == (p, order)
        got = _prove(ctx, p)
        assert ctx.fri_last_degree_ok() is True and ctx.deep_last_zeta() == zeta
        diff = torch.nonzero(got != want).flatten()[:10].tolist()
        assert not diff, (diff, bm.layout(p))
        assert (_bverify(ctx, p, caps_s, got) == 1).all()
    clock.report()


def _deep_eval_per(log_sub, n_cols):
    """columns per chunk of launch_deep_eval"""
    tiles = ((1 << log_sub) + 64 * DEEP_ROWS - 1) // (64 * DEEP_ROWS)
    chunks = min(n_cols, max(1, DEEP_EVAL_WAVES // tiles))
    return (n_cols + chunks - 1) // chunks


def _ladder_spots(log_m, n_cols):
    """8 columns: the first, the last, both sides of a streaming chunk boundary, both sides of a k_deep_eval chunk boundary, two in between"""
    per = _deep_eval_per(log_m - FULL["log_blowup"], n_cols)
    assert 1 < per < n_cols // 4
    at = per * ((n_cols // 3) // per + 1)  # a k_deep_eval boundary away from the streaming boundary below
    pick = sorted({0, 7 * FULL_CHUNK - 1, 7 * FULL_CHUNK, at - 1, at, n_cols // 2 + 3, (3 * n_cols) // 4 + 5, n_cols - 1})
    assert len(pick) == 8 and pick[-1] == n_cols - 1
    return pick


def _trace_columns(tr, section, log_m, pick):
    """the pre-LDE trace columns `pick` of a section, sliced out of the trace block on the device (natural rows, zero padded): column c is
    cell c % width of proof c // width"""
    off, rows, width = _section_geom(0, FULL["n"], section)
    cols = np.zeros((len(pick), 1 << (log_m - FULL["log_blowup"])), dtype=np.uint64)
    for k, c in enumerate(pick):
        cols[k, :rows] = _down(tr[c // width, off:off + rows * width].view(rows, width)[:, c % width].contiguous())
    return cols


def _apply(proof, at, value):
    bad = proof.copy()
    bad[at] = np.uint64((int(bad[at]) % P + 1) % P if value is None else value)
    return bad


@pytest.mark.gpu
def test_full_size_five_sections_with_the_ladders(full, oracle):
    """(7) all five row tables of the full-size trace in ONE proof, the ladders (16 640 columns of 2^19 extended rows) streamed in chunks of
    512 columns.  tmx_trace_commit_set_bytes says what is saved: the streamed figure must be below the card's free memory; where the
    resident one is too, that half is skipped with a message (measured on a 288-GiB MI355X with the trace block and the scratch of the test
    before it allocated: streamed 46.6 GiB, resident 221.5 GiB, 239.1 GiB free -- the resident set would have fitted, narrowly).  The
    oracle order is LADDERS, SHA512, TREE, SHA256, HEADER; proved without and with 16 bits of grinding: the device verifier and
    batch_model.verify accept all 28 queries of both proofs; zeta is the model transcript's; eight spot columns of the ladders have
    deep_model.evaluate's openings and oracle.lde's queried words; the four resident members' caps are their single commits'; a second prove
    gives the same words; four tamper cases on the ladders oracle get the model's verdicts"""
    import torch
    from tendermintx_amd.context import trace_commit_set_bytes as nbytes
    ctx, tr = full
    clock = _Clock("five sections, ladders streamed")
    cap_w = 4 << FULL["cap_height"]
    args = (0, FULL["n"], FULL["proofs"], ALL)
    need_s = nbytes(*args, LADDERS, FULL_CHUNK, FULL["log_blowup"], FULL["cap_height"])
    need_r = nbytes(*args, 0, FULL_CHUNK, FULL["log_blowup"], FULL["cap_height"])
    torch.cuda.empty_cache()
    free_b, total_b = torch.cuda.mem_get_info(_dev())
    print(f"\n[streamed] five sections: streamed {need_s / 2**30:.1f} GiB, resident {need_r / 2**30:.1f} GiB, free {free_b / 2**30:.1f} of "
          f"{total_b / 2**30:.1f} GiB", flush=True)
    assert 0 < need_s < free_b, (need_s, free_b)
    if need_r <= free_b:  # (a larger card: the feature is a saving there, not a necessity)
        print("[streamed] the resident five-section set would fit this card: that half of the reason is skipped", flush=True)
    else:
        assert need_r > free_b >= need_s
    with clock.part("gpu"):
        d_caps, p, order = _full_commit(ctx, tr, ALL, LADDERS)
        assert order == FULL_ORDER and p["log_n"] == [19, 18, 18, 17, 15] and p["n_cols"] == [16640, 4608, 2304, 2304, 2304]
        pg = dict(p, pow_bits=FULL["pow_bits"])
        L, Lg = bm.layout(p), bm.layout(pg)
        proofs, oks, zetas = [], [], []
        for q in (p, pg):
            proofs.append(_prove(ctx, q))
            assert ctx.fri_last_degree_ok() is True
            zetas.append(ctx.deep_last_zeta())
            oks.append(_bverify(ctx, q, d_caps, proofs[-1]))
        nonce = ctx.pow_last()[0]
        for k, sec in enumerate(FULL_ORDER):  # the single commits of the four resident members: the same caps
            if sec == LADDERS:
                continue
            cap = _sentinel(cap_w)
            ctx.trace_commit_device(0, FULL["proofs"], sec, FULL["log_blowup"], FULL["cap_height"], tr.data_ptr(), cap.data_ptr(), 0)
            torch.cuda.synchronize(_dev())
            assert torch.equal(cap, d_caps[k * cap_w:(k + 1) * cap_w]), sec
        again = _prove(ctx, p)  # (the single commits left the set intact)
        assert torch.equal(again, proofs[0])
        del again
        got, got_g, caps = _down(proofs[0]), _down(proofs[1]), _down(d_caps)
    assert (oks[0] == 1).all() and (oks[1] == 1).all(), oks
    with clock.part("python"):
        assert all(bm.verify(oracle, p, caps, got, _shift())) and all(bm.verify(oracle, pg, caps, got_g, _shift()))
        cap_list = [caps[k * cap_w:(k + 1) * cap_w] for k in range(5)]
        assert zetas[0] == bm._start(oracle, p, cap_list)[1] and zetas[1] == bm._start(oracle, pg, cap_list)[1] and zetas[0] != zetas[1]
        assert nonce == int(got_g[Lg["off_nonce"]]) < P
        m, n = p["log_n"][0], p["n_cols"][0]
        pick = _ladder_spots(m, n)
        cols = _trace_columns(tr, LADDERS, m, pick)
        assert all(c.any() for c in cols)
        ext = oracle.lde(cols, FULL["log_blowup"]).reshape(len(pick), -1)
        for q, proof, lay, zeta in ((p, got, L, zetas[0]), (pg, got_g, Lg, zetas[1])):
            idx = (proof[lay["off_indices"]:lay["off_indices"] + 28] % np.uint64(1 << m)).astype(np.int64)
            rows = proof[lay["off_init_rows"][0]:lay["off_init_rows"][0] + 28 * n].reshape(28, n)
            openings = bm.openings_of(q, proof, 0)
            ys = dm.evaluate(oracle, cols, 1, bm._points(oracle, q, 0, zeta))
            assert [openings[c] for c in pick] == [tuple(y) for y in ys]
            for k, c in enumerate(pick):
                assert np.array_equal(rows[:, c], ext[k, idx]), c
    R = 1 << dm.log_r(n)
    path_len = m - L["cap_height_of"][0]
    assert R > n
    for name, at, value, fails in (("opening of the last ladder column", L["off_open"][0] + 3 * R + n - 1, None, None),
                                   ("row word of the last ladder column", L["off_init_rows"][0] + 5 * n + n - 1, None, {5}),
                                   ("top path digest", L["off_init_paths"][0] + 11 * path_len * 4 + 4 * (path_len - 1) + 2, None, {11}),
                                   ("padding word at R - 1", L["off_open"][0] + 2 * R + R - 1, 1, None)):
        bad = _apply(got, at, value)
        with clock.part("python"):
            model = bm.verify(oracle, p, caps, bad, _shift())
        assert model == _want(p, fails), name
        with clock.part("gpu"):
            device = _bverify(ctx, p, d_caps, _up(bad))
        assert [bool(x) for x in device] == model, name
    clock.report()
