"""Streamed helpers of the SHA-512 sets (include/tmx.h "streamed helpers of the SHA-512 sets"): the host-only
tmx_trace_commit_set_air_sha512_streamed_bytes, the set-level tmx_trace_commit_set_air_sha512_streamed_device of constraint sets 7, 8 and 9
on TMX_TRACE_SHA512, and tmx_trace_commit_set_air_sha512_scratch_bytes.  The promise is that of every streamed member: for any valid chunk
size the caps, gamma, the set's shape and every word of the proof equal the resident call's.  The yardsticks are the resident calls
themselves and, for the pieces, the three existing models run on sub-arrays and one constant of F_p^2 (tests/sha_streamed_model.py's
arithmetic).  The fixtures and the plumbing are those of tests/test_sha512_air.py and its siblings and of tests/test_sha_streamed.py."""
import numpy as np
import pytest

import batch_model as bm
import fri_model as fm
import sha512_air_model as s7
import sha512_init_model as s9
import sha512_sched_model as s8
import sha_streamed_model as st
import test_sha512_air as t7
import test_sha512_init as t9
import test_sha512_sched as t8
from test_fri import _down, _sentinel, _shift, _up
from test_sha512_air import step2  # noqa: F401  (a fixture)
from test_sha_air import BAD_ARG, GUARD, _dev, _guarded, _refused

P = fm.P
SHA512, SHA256, HEADER = 2, 4, 32
HELPER_ID = {7: 32768, 8: 131072, 9: 524288}   # section ids of the helpers; a quotient's is twice its helper's
SET_OF = {sec << q: s for s, sec in HELPER_ID.items() for q in (0, 1)}
W = 18
MODELS = {7: s7, 8: s8, 9: s9}
HC = {7: s7.HELPER_COLS, 8: s8.HELPER_COLS, 9: s9.HELPER_COLS}
CONSTRAINTS = {7: 628, 8: 234, 9: 673}
CAP_H = 2
SETS = (7, 8, 9)
CAPACITY = -4


# ---- CPU
def test_symbols_and_wrappers_exist(built_lib):
    """the three new entry points are in the built library and bound in _lib.py; context.py wraps the set-level call, the scratch bytes and,
    at module level, the bytes function"""
    from tendermintx_amd import context
    for name in ("tmx_trace_commit_set_air_sha512_streamed_bytes", "tmx_trace_commit_set_air_sha512_streamed_device",
                 "tmx_trace_commit_set_air_sha512_scratch_bytes"):
        assert getattr(built_lib, name).argtypes, name
    assert callable(context.Context.trace_commit_set_air_sha512_streamed_device)
    assert callable(context.Context.trace_commit_set_air_sha512_scratch_bytes)
    assert callable(context.trace_commit_set_air_sha512_streamed_bytes)
    assert (HC, {s: m.CONSTRAINTS for s, m in MODELS.items()}) == ({7: 599, 8: 230, 9: 629}, CONSTRAINTS)


def _digests(log_m, h):
    return sum(1 << (log_m - k) for k in range(log_m - h + 1))


def _bytes_formula(set_id, log_m, log_blowup, cap_height, n_proofs, chunk_proofs):
    """(scratch, LDE scratch) in bytes, written from the layout in include/tmx.h: pre-LDE helper | helper levels | quotient | quotient
    levels | sponge states [12][M] | chunk [chunk_proofs helper_cols][M], and twice one chunk; resident (one chunk holds everything):
    (hc P (N + M) + 2 M) 8 + two trees, the LDE extending one proof's helper at a time"""
    hc, M, N = HC[set_id], 1 << log_m, 1 << (log_m - log_blowup)
    trees = 2 * _digests(log_m, min(cap_height, log_m)) * 32
    if chunk_proofs >= n_proofs:
        return (hc * n_proofs * (N + M) + 2 * M) * 8 + trees, 2 * hc * M * 8
    chunk = chunk_proofs * hc * M
    return (hc * n_proofs * N + 2 * M + 12 * M + chunk) * 8 + trees, 2 * chunk * 8


SHAPES = [(10, 1, 2, 19, 8), (12, 3, 4, 9, 8), (18, 3, 4, 256, 8)]   # (log_m, log_blowup, cap_height, n_proofs, chunk_proofs)


@pytest.mark.parametrize("set_id", SETS)
def test_bytes_equal_the_formula(built_lib, set_id):
    """the set-level tests' shape, the blow-up-8 shape and the product's (T.2 at N = 128: M = 2^18, 256 proofs) in chunks of 8 proofs, set 8
    also in chunks of 4 and 12; a chunk that holds every proof gives the resident call's bytes"""
    from tendermintx_amd.context import trace_commit_set_air_sha512_streamed_bytes as nbytes
    for log_m, lb, cap_h, n, chunk in SHAPES:
        for ch in (chunk,) + ((4, 12) if set_id == 8 else ()):
            got = nbytes(set_id, log_m, lb, cap_h, n, ch)
            assert got[0] and got == _bytes_formula(set_id, log_m, lb, cap_h, n, ch), (log_m, ch)
        resident = ((HC[set_id] * n * ((1 << log_m - lb) + (1 << log_m)) + (2 << log_m)) * 8 + 2 * _digests(log_m, cap_h) * 32,
                    2 * HC[set_id] * 8 << log_m)
        for ch in (-(-n // 8) * 8, 1 << 20):   # (the smallest chunk the rule takes that holds every proof: 24, 16, 256)
            assert nbytes(set_id, log_m, lb, cap_h, n, ch) == resident, (log_m, ch)


def test_bytes_refusals_and_the_point_of_streaming(built_lib):
    """0 for constraint_set 3, 6 and 10, chunk_proofs = 0, 4 x 599, 4 x 629 and 2 x 230 columns (no multiples of 8), log_blowup 0 and 7,
    64 and 2^19 rows, no proof, and more than 2^24 helper columns, one case each; the multiples the chunk rule does take.  At the product's
    size the scratch and the LDE's scratch of each set are below a quarter of the resident bytes: the formula gives 0.19 - 0.20, so the
    bound has room and is no measurement"""
    from tendermintx_amd.context import trace_commit_set_air_sha512_streamed_bytes as nbytes
    for args in ((3, 18, 3, 4, 256, 8), (6, 18, 3, 4, 256, 8), (10, 18, 3, 4, 256, 8), (7, 18, 3, 4, 256, 0), (7, 18, 3, 4, 256, 4),
                 (9, 18, 3, 4, 256, 4), (8, 18, 3, 4, 256, 2), (7, 18, 0, 4, 256, 8), (7, 18, 7, 4, 256, 8), (7, 9, 3, 4, 256, 8),
                 (7, 22, 3, 4, 256, 8), (7, 18, 3, 4, 0, 8), (7, 18, 3, 4, (1 << 24) // 599 + 1, 8), (8, 18, 3, 4, (1 << 24) // 230 + 1, 8),
                 (9, 18, 3, 4, (1 << 24) // 629 + 1, 8)):
        assert nbytes(*args) == (0, 0), args
    for set_id, chunk in ((7, 8), (7, 24), (9, 16), (8, 4), (8, 12), (8, 8)):
        assert nbytes(set_id, 21, 3, 4, 256, chunk)[0] > 0 and nbytes(set_id, 10, 3, 4, 1, chunk)[0] > 0, (set_id, chunk)
    assert nbytes(7, 18, 3, 4, (1 << 24) // 599, 8)[0] > 0
    for set_id in SETS:
        resident = nbytes(set_id, 18, 3, 4, 256, 256)[0]
        ratio = sum(nbytes(set_id, 18, 3, 4, 256, 8)) / resident
        assert 0.18 < ratio < 0.25, (set_id, ratio)
    streamed = [nbytes(s, 18, 3, 4, 256, 8) for s in SETS]
    for got, about in zip([x[0] for x in streamed] + [max(x[1] for x in streamed)], (50.3e9, 19.3e9, 52.8e9, 21.1e9)):
        assert abs(got - about) < 0.1e9, (got, about)   # (DESIGN.md's table: the helper columns, and 0.06 GB of states and trees)
    assert 875e9 < sum(nbytes(s, 18, 3, 4, 256, 256)[0] for s in SETS) < 885e9


def _pext(oracle, set_id, N, lb):
    pre = np.asarray(MODELS[set_id].periodic(N))
    return oracle.lde(pre.reshape(-1, N), lb)


@pytest.mark.parametrize("set_id", SETS)
def test_pieces_of_the_model_sum_to_the_whole(oracle, step2, set_id):
    """T.2 of step N = 2 (N = 512, two proofs), blow-up 2: the model's quotient of proof 0 alone plus gamma^C times its quotient of proof 1
    alone (C = 628, 234, 673) is its quotient of both, word for word, added in both orders; neither piece is zero or the whole"""
    m, lb = MODELS[set_id], 1
    N, n_proofs = step2.shape[1], step2.shape[0] // W
    assert (N, n_proofs, m.CONSTRAINTS) == (512, 2, CONSTRAINTS[set_id])
    log_n = 9 + lb
    ext, hext, pext = oracle.lde(step2, lb), oracle.lde(m.helper(step2, n_proofs), lb), _pext(oracle, set_id, N, lb)
    g = (0x0123456789ABCDEF % P, 0xFEDCBA9876543210 % P)
    want = m.quotient(oracle, log_n, lb, n_proofs, ext, hext, pext, _shift(), g)
    hc = HC[set_id]
    pieces = [st.scale(m.quotient(oracle, log_n, lb, 1, ext[p * W:(p + 1) * W], hext[p * hc:(p + 1) * hc], pext, _shift(), g),
                       st.e_pow(g, CONSTRAINTS[set_id] * p)) for p in range(n_proofs)]
    assert all(x.any() and not np.array_equal(x, want) for x in pieces)
    assert np.array_equal(st.add(pieces[0], pieces[1]), want) and np.array_equal(st.add(pieces[1], pieces[0]), want)


# ---- GPU: the set level
N_PROOFS, LB = 19, 1
CW = 4 << CAP_H


class _Sets:
    """one context and one batch of trace rows at step N = 2 (T.2 has 2^9 rows), nineteen proofs; run() commits a fresh set SHA512 | HEADER
    over the first n_proofs of them, makes the given set-level calls on SHA512 -- (set id, chunk_proofs or None for the resident call) --
    and proves; results are kept by their calls"""

    def __init__(self, n_proofs=N_PROOFS):
        import tendermintx_amd as tmx
        from test_merkle_open import _trace_rows
        self.c = tmx.Context(2, b"celestia", max_batch=n_proofs)
        self.tr = _trace_rows(self.c, 1, 2, n_proofs, 9300)
        self.kept = {}

    def commit(self, n_proofs=N_PROOFS, lb=LB, sections=SHA512 | HEADER):
        """{section: its cap on the device}"""
        n = bin(sections).count("1")
        buf = _sentinel(n * CW + 2 * GUARD)
        d_caps = buf[GUARD:GUARD + n * CW]
        self.c.trace_commit_set_device(1, n_proofs, sections, lb, CAP_H, self.tr.data_ptr(), d_caps.data_ptr(), 0)
        _guards_intact(buf)
        return {sec: d_caps[CW * i:CW * (i + 1)] for i, sec in enumerate(self.c.trace_commit_set_shape()[1])}

    def call(self, set_id, chunk, d_cap_h, d_cap_q):
        c = self.c
        if chunk is None:
            {7: c.trace_commit_set_air_sha512_device, 8: c.trace_commit_set_air_sha512_sched_device,
             9: c.trace_commit_set_air_sha512_init_device}[set_id](SHA512, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
        else:
            c.trace_commit_set_air_sha512_streamed_device(set_id, SHA512, chunk, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)

    def pair(self, set_id, chunk):
        """the call with each cap between guard words; (d_cap_h, d_cap_q)"""
        import torch
        bufs = [_sentinel(CW + 2 * GUARD) for _ in range(2)]
        caps = [b[GUARD:GUARD + CW] for b in bufs]
        self.call(set_id, chunk, *caps)
        torch.cuda.synchronize(_dev())
        for b in bufs:
            _guards_intact(b)
        return tuple(caps)

    def prove(self):
        """(params, section_of, proof words) of one proof over the set as it stands; the proof sits between guard words"""
        c = self.c
        shape, order = c.trace_commit_set_shape()
        p = dict(shape, arity_bits=2, final_log_max=2, n_queries=6, pow_bits=0)
        proof = _guarded(bm.layout(p)["words"], lambda o: c.trace_commit_set_prove_device(p, o, 0))
        assert c.fri_last_degree_ok() is True
        return p, order, _down(proof)

    def verify(self, p, order, words, table_caps, pairs):
        """pairs: {set id: (d_cap_h, d_cap_q)}; (caps in oracle order, {"batch": verdicts, set id: (verdicts, verdicts with that set's
        quotient opening bumped)}), under the context's CURRENT domain"""
        import torch
        c = self.c
        caps = [table_caps[sec] if sec in table_caps else pairs[SET_OF[sec]][int(sec not in HELPER_ID.values())] for sec in order]
        all_caps = torch.cat(caps)
        L, kt = bm.layout(p), order.index(SHA512)
        verdicts = {"batch": t7._verdicts(c, p, 0, all_caps, words, batch_only=True)}
        for set_id in pairs:
            kh = order.index(HELPER_ID[set_id])
            check = {7: lambda w: t7._verdicts(c, p, kt, all_caps, w), 8: lambda w: t8._verdicts(c, p, kt, kh, all_caps, w),
                     9: lambda w: t9._verdicts(c, p, kt, kh, all_caps, w)}[set_id]
            verdicts[set_id] = (check(words), check(t9._bumped(words, L["off_open"][kh + 1])))
        return _down(all_caps), verdicts

    def run(self, calls, between=lambda when: None, n_proofs=N_PROOFS, lb=LB):
        """between("calls") runs behind the commit, between("prove") behind the calls, between("verify") behind the prove"""
        key = (tuple(calls), n_proofs, lb)
        if key in self.kept and between("cached") is None:
            return self.kept[key]
        table_caps = self.commit(n_proofs, lb)
        pairs, gammas = {}, {}
        between("calls")
        for set_id, chunk in calls:
            pairs[set_id] = self.pair(set_id, chunk)
            gammas[set_id] = self.c.air_last_gamma()
        between("prove")
        p, order, proof = self.prove()
        between("verify")
        caps, verdicts = self.verify(p, order, proof, table_caps, pairs)
        out = dict(p=p, order=order, caps=caps, proof=proof, verdicts=verdicts, gammas=gammas)
        if between("cached") is None:
            self.kept[key] = out
        return out


def _guards_intact(buf):
    import torch
    want = _sentinel(GUARD)
    assert torch.equal(buf[:GUARD], want) and torch.equal(buf[-GUARD:], want)


@pytest.fixture(scope="module")
def sets(built_lib):
    s = _Sets()
    yield s
    s.c.close()


def _same(a, b):
    assert a["order"] == b["order"] and a["p"] == b["p"] and a["gammas"] == b["gammas"]
    assert np.array_equal(a["caps"], b["caps"])
    diff = np.flatnonzero(a["proof"] != b["proof"])[:10]
    assert not len(diff), (diff, bm.layout(a["p"]))


def _accepted(r):
    assert all(r["verdicts"]["batch"])
    for key, both in r["verdicts"].items():
        if key != "batch":
            good, bad = both
            assert all(good) and not any(bad), key


@pytest.mark.gpu
@pytest.mark.parametrize("set_id", SETS)
def test_streamed_set_level_call_equals_the_resident_call(sets, set_id):
    """T.2 of step N = 2 (N = 2^9), nineteen proofs, blow-up 2: streamed in chunks of 8 proofs (8 + 8 + 3) and of 16 (16 + 3), set 8 also of
    4 (4 x 4 + 3) and 12 (12 + 7), and with chunk_proofs = 24 (one chunk: the resident path), against the resident call: the same d_cap_h,
    d_cap_q, gamma, shape and proof word for word, the degree flag true; the set's device verifier and tmx_batch_verify_device accept
    every query; with the quotient's opening bumped the set's verifier rejects every query.  A piece behind the first reads its own
    proofs' eighteen table columns: a table pointer advanced by another width gives other words in every run with a second piece"""
    want = sets.run([(set_id, None)])
    assert want["order"][want["order"].index(SHA512) + 1:][:2] == [HELPER_ID[set_id], 2 * HELPER_ID[set_id]]
    assert want["p"]["n_cols"][want["order"].index(HELPER_ID[set_id])] == N_PROOFS * HC[set_id]
    _accepted(want)
    for chunk in (8, 16, 24) + ((4, 12) if set_id == 8 else ()):
        got = sets.run([(set_id, chunk)])
        _same(got, want)
        _accepted(got)


@pytest.mark.gpu
def test_three_streamed_sets_equal_three_resident_sets(sets):
    """all three sets streamed in the call order 9-7-8 (chunks of 8, 16 and 4 proofs) against all three resident in the order 7-8-9: the
    same eight oracles [HEADER, SHA512, H7, Q7, H8, Q8, H9, Q9] (19 x 1458 streamed helper columns in one proof), caps and proof; all
    three verifiers accept"""
    want = sets.run([(7, None), (8, None), (9, None)])
    got = sets.run([(9, 8), (7, 16), (8, 4)])
    at = got["order"].index(SHA512)
    assert len(got["order"]) == 8 and got["order"][at:at + 7] == [SHA512, 32768, 65536, 131072, 262144, 524288, 1048576]
    assert sum(got["p"]["n_cols"][at + k] for k in (1, 3, 5)) == N_PROOFS * 1458
    _same(got, want)
    _accepted(got)
    assert sorted(k for k in got["verdicts"] if k != "batch") == [7, 8, 9]


@pytest.mark.gpu
def test_resident_and_streamed_pairs_on_the_section(sets):
    """set 7 resident and set 8 streamed equals both resident; so does set 9 streamed in front of set 7 resident"""
    want = sets.run([(7, None), (8, None)])
    got = sets.run([(7, None), (8, 12)])
    _same(got, want)
    _accepted(got)
    want = sets.run([(7, None), (9, None)])
    got = sets.run([(9, 16), (7, None)])
    _same(got, want)
    _accepted(got)


@pytest.mark.gpu
@pytest.mark.parametrize("set_id", SETS)
def test_the_domain_moved_between_the_commit_and_the_calls(sets, oracle, set_id):
    """tmx_ntt_set_domain between the commit and the streamed call, back behind the call and moved again in front of the prove: the call
    extends the chunks AND the set's preprocessed planes under the set's domain and so does the prove, so the words are those of the
    unmoved resident run; and the context's domain is what the caller set -- the same column extends to the same words right after the
    moves, behind the call and behind the prove, and to other words once the caller sets the default back (under which the verifiers
    then accept)"""
    import torch
    c = sets.c
    want = sets.run([(set_id, None)])
    col, outs = _up(np.arange(1, 65, dtype=np.uint64)), {}

    def probe(name):
        outs[name] = _sentinel(128)
        c.lde_device(6, 1, 1, col.data_ptr(), outs[name].data_ptr(), 0)

    def between(when):
        if when == "cached":
            return False  # (never kept: this run is not the plain one)
        if when == "calls":
            c.ntt_set_domain(*oracle.G7_DOMAIN)
            probe("moved")
        elif when == "prove":
            probe("behind the call")
            c.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
            c.ntt_set_domain(*oracle.G7_DOMAIN)
        else:
            probe("behind the prove")
            c.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
            probe("default")

    try:
        got = sets.run([(set_id, 8)], between)
    finally:
        c.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
    torch.cuda.synchronize(_dev())
    assert torch.equal(outs["moved"], outs["behind the call"]) and torch.equal(outs["moved"], outs["behind the prove"])
    assert not torch.equal(outs["moved"], outs["default"])
    _same(got, want)
    _accepted(got)


@pytest.mark.gpu
@pytest.mark.parametrize("set_id", SETS)
def test_streamed_as_the_first_call_of_a_fresh_context(built_lib, set_id):
    """a context of its own per set whose FIRST set-level call is the streamed one (nine proofs in chunks of 8 and, set 8, of 4): no
    resident call has left the set's preprocessed planes in the context's scratch, so the streamed branch has to fill and extend them
    itself.  The set's verifier accepts; the resident call behind it, on a fresh set, gives the same caps, gamma and proof words"""
    s = _Sets(9)
    try:
        got = s.run([(set_id, 4 if set_id == 8 else 8)], n_proofs=9)
        _accepted(got)
        want = s.run([(set_id, None)], n_proofs=9)
        _same(got, want)
        _accepted(want)
    finally:
        s.c.close()


@pytest.mark.gpu
def test_blowup_8_and_a_last_piece_of_one_proof(sets):
    """blow-up 8, nine proofs, set 9 in chunks of 8 (8 + 1: the last piece is one proof in a chunk buffer sized for eight): the resident
    call's words, and the verifiers accept"""
    want = sets.run([(9, None)], n_proofs=9, lb=3)
    got = sets.run([(9, 8)], n_proofs=9, lb=3)
    assert got["p"]["log_blowup"] == 3 and got["p"]["log_n"][got["order"].index(SHA512)] == 12
    _same(got, want)
    _accepted(got)


@pytest.mark.gpu
def test_streamed_then_resident_then_streamed_on_one_context(sets):
    """a streamed call of set 9, then a fresh set and the resident call on the same context, then streamed again twice: the scratch of
    that set is sized exactly by a streamed call (tmx_trace_commit_set_air_sha512_scratch_bytes equals the bytes function; released and
    allocated anew behind a resident one and between two chunk sizes) and is at least the resident formula behind a resident one; the
    same words each time.  Free device memory behind each call is printed, not asserted: other processes may allocate on the same card"""
    import torch
    from tendermintx_amd.context import trace_commit_set_air_sha512_streamed_bytes as nbytes
    c = sets.c
    want = sets.run([(9, None)])
    log_m, free = 9 + LB, []
    for chunk in (8, None, 8, 16):
        table_caps = sets.commit()
        pair = sets.pair(9, chunk)
        free.append(torch.cuda.mem_get_info(_dev())[0] >> 20)
        held = c.trace_commit_set_air_sha512_scratch_bytes(9, SHA512)
        if chunk is None:
            assert held >= nbytes(9, log_m, LB, CAP_H, N_PROOFS, N_PROOFS)[0]
        else:
            assert held == nbytes(9, log_m, LB, CAP_H, N_PROOFS, chunk)[0] == _bytes_formula(9, log_m, LB, CAP_H, N_PROOFS, chunk)[0]
        assert c.trace_commit_set_air_sha512_scratch_bytes(9, HEADER) == 0 and c.trace_commit_set_air_sha512_scratch_bytes(6, SHA512) == 0
        assert c.trace_commit_set_air_sha512_scratch_bytes(10, SHA512) == 0
        p, order, proof = sets.prove()
        caps, _ = sets.verify(p, order, proof, table_caps, {9: pair})
        assert np.array_equal(caps, want["caps"]) and np.array_equal(proof, want["proof"]), chunk
    print(f"\n[sha512-streamed] MiB free behind the calls (chunk 8, resident, chunk 8, chunk 16): {free}")


@pytest.mark.gpu
def test_a_second_call_behind_a_streamed_pair_is_refused(sets):
    """behind a pair whose helper IS streamed (19 proofs in chunks of 4), a second call of that set is refused in either form, and the
    set's shape stays; another set's pair is still taken"""
    c = sets.c
    sets.commit()
    a, b, d_cap_h, d_cap_q = (_sentinel(CW) for _ in range(4))
    sets.call(8, 4, a, b)
    before = c.trace_commit_set_shape()
    assert before[1] == [HEADER, SHA512, 131072, 262144]
    for chunk in (4, 8, 24, None):
        assert "already" in _refused(lambda: sets.call(8, chunk, d_cap_h, d_cap_q), d_cap_h, d_cap_q)
    assert c.trace_commit_set_shape() == before
    sets.call(7, None, a, b)
    assert c.trace_commit_set_shape()[1] == [HEADER, SHA512, 32768, 65536, 131072, 262144]


@pytest.mark.gpu
def test_set_level_refusals(built_lib):
    """no set, constraint_set 3, 6 and 10, a section other than TMX_TRACE_SHA512 or one that is absent, null caps, chunk_proofs 0, 4 for
    sets 7 and 9, 2 for set 8, a streamed table member, a second call in either form, a full set: TMX_ERR_BAD_ARG, nothing written, the
    shape as it was"""
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    kind, n, n_proofs, lb = 1, 2, 2, 1
    with tmx.Context(n, b"celestia", max_batch=n_proofs) as c:
        tr = _trace_rows(c, kind, n, n_proofs, 9300)
        d_caps, d_cap_h, d_cap_q = _sentinel(3 * CW), _sentinel(CW), _sentinel(CW)
        call = lambda s, sec=SHA512, chunk=8, h=d_cap_h.data_ptr(), q=d_cap_q.data_ptr(): (
            lambda: c.trace_commit_set_air_sha512_streamed_device(s, sec, chunk, h, q, 0))
        commit = lambda secs=SHA512 | HEADER: c.trace_commit_set_device(kind, n_proofs, secs, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        assert "no commit set" in _refused(call(7), d_cap_h, d_cap_q)
        commit()
        before = c.trace_commit_set_shape()
        for s in (3, 6, 10):
            assert "7, 8 or 9" in _refused(call(s), d_cap_h, d_cap_q)
        for sec in (HEADER, SHA256, 1, 32768, 524288, 0):
            assert "TMX_TRACE_SHA512" in _refused(call(7, sec), d_cap_h, d_cap_q)
        for fn in (call(7, h=None), call(8, q=None), call(7, chunk=0), call(8, chunk=0), call(9, chunk=0), call(7, chunk=4), call(9, chunk=4),
                   call(8, chunk=2), call(8, chunk=6)):
            _refused(fn, d_cap_h, d_cap_q)
        assert c.trace_commit_set_shape() == before
        a, b = _sentinel(CW), _sentinel(CW)
        c.trace_commit_set_air_sha512_streamed_device(9, SHA512, 8, a.data_ptr(), b.data_ptr(), 0)   # (one chunk: the resident form)
        assert "already" in _refused(call(9), d_cap_h, d_cap_q)
        assert "already" in _refused(lambda: c.trace_commit_set_air_sha512_init_device(SHA512, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0),
                                     d_cap_h, d_cap_q)
        assert c.trace_commit_set_shape()[1] == [HEADER, SHA512, 524288, 1048576]
        commit(HEADER)
        before = c.trace_commit_set_shape()
        assert "does not hold" in _refused(call(7), d_cap_h, d_cap_q)
        assert c.trace_commit_set_shape() == before
        commit(SHA512 | SHA256 | HEADER)
        c.trace_commit_set_air_sha512_streamed_device(8, SHA512, 4, a.data_ptr(), b.data_ptr(), 0)
        c.trace_commit_set_air_sha512_streamed_device(7, SHA512, 8, a.data_ptr(), b.data_ptr(), 0)
        full = c.trace_commit_set_shape()
        assert len(full[1]) == 7
        assert "room" in _refused(call(9), d_cap_h, d_cap_q)  # (seven oracles: no room for a pair)
        assert c.trace_commit_set_shape() == full
        c.trace_commit_set_streamed_device(kind, n_proofs, SHA512 | HEADER, SHA512, 8, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        before = c.trace_commit_set_shape()
        for s in SETS:
            assert "streamed" in _refused(call(s), d_cap_h, d_cap_q)
            assert c.trace_commit_set_shape() == before


@pytest.mark.gpu
def test_capacity_counts_the_ldes_scratch(built_lib):
    """a shape whose formula exceeds the card's whole memory, so the refusal needs nothing held: T.2 of step N = 2 alone, 800 proofs,
    blow-up 64 (M = 2^15; the committed table is 3.8 GB), set 9 in chunks of 792 proofs -- a chunk of 131 GB, scratch + LDE scratch 394 GB.
    TMX_ERR_CAPACITY, the message counts the LDE's scratch, nothing written, the shape as it was, no scratch held.  Then a small set of
    the first nine proofs on the same context: the streamed call is taken and holds what the bytes function says"""
    import tendermintx_amd as tmx
    import torch
    from tendermintx_amd._lib import TmxError
    from tendermintx_amd.context import trace_commit_set_air_sha512_streamed_bytes as nbytes
    from test_merkle_open import _trace_rows
    kind, n, n_proofs, lb, chunk = 1, 2, 800, 6, 792
    with tmx.Context(n, b"celestia", max_batch=n_proofs) as c:
        tr = _trace_rows(c, kind, n, n_proofs, 9300)
        d_caps, d_cap_h, d_cap_q = _sentinel(2 * CW), _sentinel(CW), _sentinel(CW)
        c.trace_commit_set_device(kind, n_proofs, SHA512, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        before = c.trace_commit_set_shape()
        assert before[1] == [SHA512] and before[0]["log_n"] == [9 + lb]
        scratch, lde = nbytes(9, 9 + lb, lb, CAP_H, n_proofs, chunk)
        assert lde == 2 * chunk * 629 * 8 << 15
        # (the call compares with free memory plus the LDE scratch the context holds: at most twice the extended table behind this commit)
        total, table = torch.cuda.mem_get_info(_dev())[1], n_proofs * W * 8 << 15
        assert scratch + lde > total + 2 * table, (scratch, lde, total)
        caps = [d_cap_h.clone(), d_cap_q.clone()]
        with pytest.raises(TmxError) as e:
            c.trace_commit_set_air_sha512_streamed_device(9, SHA512, chunk, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        assert e.value.status == CAPACITY != BAD_ARG and f"{(scratch + lde) >> 20} MiB of scratch, the LDE's own included" in str(e.value), e.value
        assert torch.equal(d_cap_h, caps[0]) and torch.equal(d_cap_q, caps[1]) and c.trace_commit_set_shape() == before
        assert c.trace_commit_set_air_sha512_scratch_bytes(9, SHA512) == 0
        c.trace_commit_set_device(kind, 9, SHA512 | HEADER, 1, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        c.trace_commit_set_air_sha512_streamed_device(9, SHA512, 8, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        assert c.trace_commit_set_air_sha512_scratch_bytes(9, SHA512) == nbytes(9, 10, 1, CAP_H, 9, 8)[0]
        assert c.trace_commit_set_shape()[1] == [HEADER, SHA512, 524288, 1048576]
