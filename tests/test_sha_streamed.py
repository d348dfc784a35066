"""Streamed helpers of the SHA-256 sets (include/tmx.h "streamed helpers of the SHA-256 sets"): the three range calls
tmx_air_sha256_quotient_range_device, _sched_quotient_range_device, _init_quotient_range_device, the host-only
tmx_trace_commit_set_air_sha256_streamed_bytes and the set-level tmx_trace_commit_set_air_sha256_streamed_device.  The promise is that of
every streamed member: for any valid chunk size the caps, gamma, the set's shape and every word of the proof equal the resident call's.
The yardsticks are the resident calls themselves and tests/sha_streamed_model.py, which is the three existing models run on sub-arrays and
one constant of F_p^2.  The fixtures and the plumbing are those of tests/test_sha_air.py and its siblings."""
import numpy as np
import pytest

import batch_model as bm
import fri_model as fm
import sha_air_model as sm
import sha_init_model as si
import sha_sched_model as ss
import sha_streamed_model as st
import test_sha_air as tsa
import test_sha_init as tsi
import test_sha_sched as tss
from test_fri import _down, _sentinel, _shift, _up
from test_sha_air import ctx, skip4, step2, step3  # noqa: F401  (fixtures)
from test_sha_air import GUARD, _random_ext, _refused, _tree
from test_sha_air_shapes import _tiled, live_blocks  # noqa: F401  (live_blocks: a fixture)

P = fm.P
SHA256, TREE, HEADER = 4, 16, 32
HELPER_ID = {3: 128, 4: 512, 5: 2048}   # section ids of the helpers; a quotient's is twice its helper's
W = 9
HC = {3: sm.HELPER_COLS, 4: ss.HELPER_COLS, 5: si.HELPER_COLS}
CONSTRAINTS = {3: 315, 4: 117, 5: 337}
CAP_H = 2
SETS = (3, 4, 5)


# ---- CPU
def test_symbols_and_wrappers_exist(built_lib):
    """the five new entry points are in the built library and bound in _lib.py; context.py wraps the set-level call and the bytes function,
    and the three quotient wrappers take proof_range and accumulate"""
    import inspect
    from tendermintx_amd import context
    for name in ("tmx_air_sha256_quotient_range_device", "tmx_air_sha256_sched_quotient_range_device",
                 "tmx_air_sha256_init_quotient_range_device", "tmx_trace_commit_set_air_sha256_streamed_bytes",
                 "tmx_trace_commit_set_air_sha256_streamed_device"):
        assert getattr(built_lib, name).argtypes, name
    assert callable(context.Context.trace_commit_set_air_sha256_streamed_device)
    assert callable(context.trace_commit_set_air_sha256_streamed_bytes)
    for name in ("air_sha256_quotient_device", "air_sha256_sched_quotient_device", "air_sha256_init_quotient_device"):
        params = inspect.signature(getattr(context.Context, name)).parameters
        assert params["proof_range"].default is None and params["accumulate"].default == 0, name


def _digests(log_m, h):
    return sum(1 << (log_m - k) for k in range(log_m - h + 1))


def _bytes_formula(set_id, log_m, log_blowup, cap_height, n_proofs, chunk_proofs):
    """(scratch, LDE scratch) in bytes, written from the layout in include/tmx.h: pre-LDE helper | helper levels | quotient | quotient
    levels | sponge states [12][M] | chunk [chunk_proofs helper_cols][M]; resident (one chunk holds everything): DESIGN.md's
    (hc P (N + M) + 2 M) 8 + two trees, the LDE extending one proof's helper at a time"""
    hc, M, N = HC[set_id], 1 << log_m, 1 << (log_m - log_blowup)
    trees = 2 * _digests(log_m, min(cap_height, log_m)) * 32
    if chunk_proofs >= n_proofs:
        return (hc * n_proofs * (N + M) + 2 * M) * 8 + trees, 2 * hc * M * 8
    chunk = chunk_proofs * hc * M
    return (hc * n_proofs * N + 2 * M + 12 * M + chunk) * 8 + trees, 2 * chunk * 8


@pytest.mark.parametrize("set_id", SETS)
def test_bytes_equal_the_formula(built_lib, set_id):
    """HEADER, T.3 and TREE at 256 proofs and blow-up 8 (log_m = 15, 17, 18) with chunks of 8 and 16 proofs, a chunk that holds all 256
    (the resident formula), and the smallest table with one proof"""
    from tendermintx_amd.context import trace_commit_set_air_sha256_streamed_bytes as nbytes
    for log_m in (15, 17, 18):
        for chunk in (8, 16, 256, 1 << 20):
            assert nbytes(set_id, log_m, 3, CAP_H, 256, chunk) == _bytes_formula(set_id, log_m, 3, CAP_H, 256, chunk), (log_m, chunk)
    for chunk in (8, 16):
        assert nbytes(set_id, 8, 2, CAP_H, 1, chunk) == _bytes_formula(set_id, 8, 2, CAP_H, 1, chunk)
        assert nbytes(set_id, 8, 2, 30, 1, chunk) == _bytes_formula(set_id, 8, 2, 30, 1, chunk)  # (cap_height is capped at log_m)


def test_bytes_refusals_and_the_point_of_streaming(built_lib):
    """0 for a set outside 3 - 5, chunk_proofs = 0, 3 x 300 and 4 x 115 columns (no multiples of 8) and the shapes the quotient calls
    refuse; chunk_proofs is even for set 3 and a multiple of 8 for sets 4 and 5.  TREE under set 3 in chunks of 8 needs less than HEADER
    and T.3 together need resident; all three pairs of TREE need about 49 GB of helper columns where the resident calls need about 441 GB
    (181 + 69 + 190)"""
    from tendermintx_amd.context import trace_commit_set_air_sha256_streamed_bytes as nbytes
    for args in ((2, 15, 3, CAP_H, 256, 8), (6, 15, 3, CAP_H, 256, 8), (3, 15, 3, CAP_H, 256, 0), (3, 15, 3, CAP_H, 256, 3),
                 (4, 15, 3, CAP_H, 256, 4), (5, 15, 3, CAP_H, 256, 4), (4, 15, 3, CAP_H, 256, 12), (3, 15, 0, CAP_H, 256, 8),
                 (3, 15, 7, CAP_H, 256, 8), (3, 8, 3, CAP_H, 1, 8), (3, 15, 3, CAP_H, 0, 8), (3, 15, 3, CAP_H, (1 << 24) // 300 + 1, 8)):
        assert nbytes(*args) == (0, 0), args
    for set_id, chunk in ((3, 2), (3, 6), (4, 8), (5, 24)):
        assert nbytes(set_id, 15, 3, CAP_H, 256, chunk)[0] > 0
    tree = sum(nbytes(3, 18, 3, CAP_H, 256, 8))
    assert tree < nbytes(3, 15, 3, CAP_H, 256, 256)[0] + nbytes(3, 17, 3, CAP_H, 256, 256)[0]
    pre = sum(HC[s] * 256 * (1 << 15) * 8 for s in SETS)
    resident = sum(nbytes(s, 18, 3, CAP_H, 256, 256)[0] for s in SETS)
    assert 48e9 < pre < 50e9 and 435e9 < resident < 445e9
    streamed = [nbytes(s, 18, 3, CAP_H, 256, 8) for s in SETS]  # (the three scratches side by side, ONE LDE scratch: the largest)
    assert sum(x[0] for x in streamed) + max(x[1] for x in streamed) < resident // 5


def _helper(set_id, table, n_proofs, chain):
    return si.helper(table, n_proofs, chain) if set_id == 5 else st.MODELS[set_id].helper(table, n_proofs)


@pytest.mark.parametrize("set_id,N,chain", [(3, 64, 0), (4, 64, 0), (5, 64, 0), (5, 128, 1)])
def test_pieces_of_the_model_sum_to_the_whole(oracle, live_blocks, set_id, N, chain):
    """N = 64 (and N = 128 under chain = 1), blow-up 2, five proofs of tiled honest tables: the pieces [0, 2) and [2, 5) of the model sum
    to the existing model's quotient of all five, word for word"""
    n_proofs, lb = 5, 1
    log_n = N.bit_length() - 1 + lb
    table = _tiled(live_blocks, N, n_proofs)
    ext, hext = oracle.lde(table, lb), oracle.lde(_helper(set_id, table, n_proofs, chain), lb)
    g = (0x0123456789ABCDEF % P, 0xFEDCBA9876543210 % P)
    want = st.whole(set_id, oracle, log_n, lb, n_proofs, chain, ext, hext, _shift(), g)
    a = st.piece(set_id, oracle, log_n, lb, chain, 0, 2, ext, hext, _shift(), g)
    b = st.piece(set_id, oracle, log_n, lb, chain, 2, 5, ext, hext, _shift(), g)
    assert a.any() and b.any() and not np.array_equal(a, want)
    assert np.array_equal(st.add(a, b), want)


# ---- GPU: the range calls
def _quotient_call(ctx, set_id):
    return {3: ctx.air_sha256_quotient_device, 4: ctx.air_sha256_sched_quotient_device, 5: ctx.air_sha256_init_quotient_device}[set_id]


def _call(ctx, set_id, log_n, lb, n_proofs, chain, ptrs, **kw):
    mode = (chain,) if set_id == 5 else ()
    _quotient_call(ctx, set_id)(log_n, lb, CAP_H, n_proofs, *mode, *ptrs, 0, **kw)


def _between_guards(words):
    """a buffer that holds `words` alone between two blocks of guard words"""
    buf = _sentinel(len(words) + 2 * GUARD)
    buf[GUARD:GUARD + len(words)] = _up(words)
    return buf


def _guards_intact(buf):
    import torch
    want = _sentinel(GUARD)
    return torch.equal(buf[:GUARD], want) and torch.equal(buf[-GUARD:], want)


RANGE_SHAPES = [(s, 6, 1, 5, 0) for s in SETS] + [(s, 6, 3, 17, 0) for s in SETS] + [(5, 7, 1, 3, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("set_id,log_rows,log_blowup,n_proofs,chain", RANGE_SHAPES)
def test_pieces_equal_the_whole_call(ctx, oracle, set_id, log_rows, log_blowup, n_proofs, chain):
    """random extended columns.  The pieces 2 + 3 of five proofs, 8 + 8 + 1 of seventeen (1 + 2 of three under chain = 1), ascending and
    descending, each piece's helper in a buffer of its own that holds only that piece's columns between guard words: d_quot equals the
    whole call's words, and at the first shape the model's, piece by piece; the first piece (accumulate = 0) overwrites a sentinel-filled
    d_quot; a single piece [0, n_proofs) equals the existing call; gamma is the whole call's after every piece; all guards intact"""
    import torch
    hc, log_n = HC[set_id], log_rows + log_blowup
    M = 1 << log_n
    rng = np.random.default_rng(11000 + 1000 * set_id + 100 * log_rows + 10 * log_blowup + n_proofs)
    ext, hext = _random_ext(rng, n_proofs * W, log_n), _random_ext(rng, n_proofs * hc, log_n)
    d_cols, d_hcols = _up(ext), _up(hext)
    _, d_cap = _tree(ctx, d_cols, log_n, n_proofs * W)
    _, d_cap_h = _tree(ctx, d_hcols, log_n, n_proofs * hc)
    caps = [d_cap.data_ptr(), d_cap_h.data_ptr()]
    whole = _sentinel(2 * M + 2 * GUARD)
    _call(ctx, set_id, log_n, log_blowup, n_proofs, chain, [d_cols.data_ptr(), d_hcols.data_ptr(), *caps, whole[GUARD:].data_ptr()])
    g = ctx.air_last_gamma()
    assert _guards_intact(whole)
    want = whole[GUARD:GUARD + 2 * M]
    cuts = {5: [0, 2, 5], 17: [0, 8, 16, 17], 3: [0, 1, 3]}[n_proofs]
    pieces = list(zip(cuts[:-1], cuts[1:]))
    first_shape = (log_rows, log_blowup, n_proofs) == (6, 1, 5)
    for order in (pieces, pieces[::-1], [(0, n_proofs)]):
        out = _sentinel(2 * M + 2 * GUARD)
        model = None
        for k, (lo, hi) in enumerate(order):
            piece = _between_guards(hext[lo * hc:hi * hc].reshape(-1))
            _call(ctx, set_id, log_n, log_blowup, n_proofs, chain, [d_cols.data_ptr(), piece[GUARD:].data_ptr(), *caps, out[GUARD:].data_ptr()],
                  proof_range=(lo, hi), accumulate=int(k > 0))
            torch.cuda.synchronize(tsa._dev())
            assert ctx.air_last_gamma() == g
            assert _guards_intact(piece) and _guards_intact(out)
            if first_shape:
                part = st.piece(set_id, oracle, log_n, log_blowup, chain, lo, hi, ext, hext, _shift(), g)
                model = part if model is None else st.add(model, part)
                assert np.array_equal(_down(out[GUARD:GUARD + 2 * M]), model), (order, lo, hi)
        diff = torch.nonzero(out[GUARD:GUARD + 2 * M] != want).flatten()[:10].tolist()
        assert not diff, (order, diff)


@pytest.mark.gpu
@pytest.mark.parametrize("set_id", SETS)
def test_each_rule_of_the_range_calls(ctx, set_id):
    """an empty range, a reversed one, proof_hi > n_proofs, accumulate > 1, and the whole call's rules (blow-up, rows, n_proofs, the mode,
    every null pointer), each on its own: TMX_ERR_BAD_ARG before anything is enqueued, d_quot untouched"""
    log_n, lb, n = 8, 1, 3
    hc = HC[set_id]
    bufs = [_sentinel((n * W) << log_n), _sentinel((n * hc) << log_n), _sentinel(4 << CAP_H), _sentinel(4 << CAP_H), _sentinel(2 << log_n)]
    ptrs = [b.data_ptr() for b in bufs]
    q = lambda rng, acc=0, ln=log_n, b=lb, np_=n, ch=0, a=ptrs: (
        lambda: _call(ctx, set_id, ln, b, np_, ch, a, proof_range=rng, accumulate=acc))
    for fn in (q((1, 1)), q((2, 1)), q((0, n + 1)), q((n, n + 1)), q((0, 1), acc=2), q((0, 1), b=0), q((0, 1), b=7), q((0, 1), ln=6),
               q((0, 1), ln=29, b=2), q((0, 0), np_=0), q((0, 1), np_=(1 << 24) // hc + 1)):
        _refused(fn, bufs[4])
    if set_id == 5:
        _refused(q((0, 1), ch=2), bufs[4])
        _refused(q((0, 1), ln=7, b=1, ch=1), bufs[4])
    for k in range(5):
        _refused(q((0, 1), a=ptrs[:k] + [None] + ptrs[k + 1:]), bufs[4])
        _refused(q((0, 1), acc=1, a=ptrs[:k] + [None] + ptrs[k + 1:]), bufs[4])


# ---- GPU: the set level
N_PROOFS, LB = 19, 1
CW = 4 << CAP_H
CHAIN = {SHA256: 0, HEADER: 1}


class _Sets:
    """one context and one batch of trace rows at step N = 2, nineteen proofs; run() commits a fresh set SHA256 | HEADER, makes the given
    set-level calls -- (set id, section, chunk_proofs or None for the resident call) -- and proves; results are kept by their calls"""

    def __init__(self):
        import tendermintx_amd as tmx
        from test_merkle_open import _trace_rows
        self.c = tmx.Context(2, b"celestia", max_batch=N_PROOFS)
        self.tr = _trace_rows(self.c, 1, 2, N_PROOFS, 9300)
        self.kept = {}

    def commit(self):
        d_caps = _sentinel(2 * CW)
        self.c.trace_commit_set_device(1, N_PROOFS, SHA256 | HEADER, LB, CAP_H, self.tr.data_ptr(), d_caps.data_ptr(), 0)
        return d_caps

    def call(self, set_id, section, chunk, d_cap_h, d_cap_q):
        c = self.c
        if chunk is None:
            {3: c.trace_commit_set_air_sha256_device, 4: c.trace_commit_set_air_sha256_sched_device,
             5: c.trace_commit_set_air_sha256_init_device}[set_id](section, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
        else:
            c.trace_commit_set_air_sha256_streamed_device(set_id, section, chunk, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)

    def prove(self):
        """(params, section_of, proof words) of one proof over the set as it stands"""
        c = self.c
        shape, order = c.trace_commit_set_shape()
        p = dict(shape, arity_bits=2, final_log_max=2, n_queries=6, pow_bits=0)
        proof = tsa._guarded(bm.layout(p)["words"], lambda o: c.trace_commit_set_prove_device(p, o, 0))
        assert c.fri_last_degree_ok() is True
        return p, order, _down(proof)

    def verify(self, p, order, words, d_caps, pairs):
        """pairs: {(section, set id): (d_cap_h, d_cap_q)}; (caps in oracle order, {"batch": verdicts, pair: (verdicts, verdicts with that
        pair's quotient opening bumped)}), under the context's CURRENT domain"""
        import torch
        c = self.c
        table_cap = {HEADER: d_caps[:CW], SHA256: d_caps[CW:]}
        caps, where, table, k_table = [], {}, None, None
        for k, sec in enumerate(order):
            if sec in table_cap:
                table, k_table = sec, k
                caps.append(table_cap[sec])
                continue
            set_id = {128: 3, 256: 3, 512: 4, 1024: 4, 2048: 5, 4096: 5}[sec]
            is_q = sec in (256, 1024, 4096)
            caps.append(pairs[(table, set_id)][int(is_q)])
            if not is_q:
                where[(table, set_id)] = (k_table, k)
        all_caps = torch.cat(caps)
        L = bm.layout(p)
        verdicts = {"batch": tsa._verdicts(c, p, 0, all_caps, words, batch_only=True)}
        for (section, set_id), (kt, kh) in where.items():
            check = {3: lambda w: tsa._verdicts(c, p, kt, all_caps, w), 4: lambda w: tss._verdicts(c, p, kt, kh, all_caps, w),
                     5: lambda w: tsi._verdicts(c, p, kt, kh, CHAIN[section], all_caps, w)}[set_id]
            verdicts[(section, set_id)] = (check(words), check(tsi._bumped(words, L["off_open"][kh + 1])))
        return _down(all_caps), verdicts

    def run(self, calls, between=lambda when: None):
        """between("calls") runs behind the commit, between("prove") behind the calls, between("verify") behind the prove"""
        key = tuple(calls)
        if key in self.kept and between("cached") is None:
            return self.kept[key]
        d_caps = self.commit()
        pairs, gammas = {}, {}
        between("calls")
        for set_id, section, chunk in calls:
            pairs[(section, set_id)] = (_sentinel(CW), _sentinel(CW))
            self.call(set_id, section, chunk, *pairs[(section, set_id)])
            gammas[(section, set_id)] = self.c.air_last_gamma()
        between("prove")
        p, order, proof = self.prove()
        between("verify")
        caps, verdicts = self.verify(p, order, proof, d_caps, pairs)
        out = dict(p=p, order=order, caps=caps, proof=proof, verdicts=verdicts, gammas=gammas)
        if between("cached") is None:
            self.kept[key] = out
        return out


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
@pytest.mark.parametrize("section", [SHA256, HEADER])
@pytest.mark.parametrize("set_id", SETS)
def test_streamed_set_level_call_equals_the_resident_call(sets, set_id, section):
    """SHA256 (chain 0, N = 2^7) and HEADER (chain 1, N = 2^12), nineteen proofs, blow-up 2: streamed in chunks of 8 proofs (8 + 8 + 3) and
    of 16 (16 + 3), and with chunk_proofs = 24 (one chunk: the resident path), against the resident call: the same d_cap_h, d_cap_q,
    gamma, shape and proof word for word; the set's device verifier and tmx_batch_verify_device accept every query; with the quotient's
    opening bumped the set's verifier rejects every query"""
    want = sets.run([(set_id, section, None)])
    assert want["order"][want["order"].index(section) + 1:][:2] == [HELPER_ID[set_id], 2 * HELPER_ID[set_id]]
    _accepted(want)
    for chunk in (8, 16, 24):
        got = sets.run([(set_id, section, chunk)])
        _same(got, want)
        _accepted(got)


@pytest.mark.gpu
def test_three_streamed_sets_equal_three_resident_sets(sets):
    """all three sets streamed on HEADER in the call order 5-3-4 (chunks of 8, 16 and 8 proofs) against all three resident in the order
    3-4-5: the same eight oracles [HEADER, H3, Q3, H4, Q4, H5, Q5, SHA256], caps and proof; all three verifiers accept"""
    want = sets.run([(3, HEADER, None), (4, HEADER, None), (5, HEADER, None)])
    got = sets.run([(5, HEADER, 8), (3, HEADER, 16), (4, HEADER, 8)])
    assert got["order"] == [HEADER, 128, 256, 512, 1024, 2048, 4096, SHA256]
    _same(got, want)
    _accepted(got)
    assert sorted(k for k in got["verdicts"] if k != "batch") == [(HEADER, 3), (HEADER, 4), (HEADER, 5)]


@pytest.mark.gpu
def test_resident_and_streamed_pairs_on_one_section(sets):
    """set 3 resident and set 4 streamed on SHA256 equals both resident"""
    want = sets.run([(3, SHA256, None), (4, SHA256, None)])
    got = sets.run([(3, SHA256, None), (4, SHA256, 8)])
    _same(got, want)
    _accepted(got)


@pytest.mark.gpu
def test_the_domain_moved_between_the_commit_and_the_calls(sets, oracle):
    """tmx_ntt_set_domain between the commit and the streamed call, back behind the call and moved again in front of the prove: the call
    and the prove extend under the set's domain, so the words are those of the unmoved resident run; and the context's domain is what the
    caller set -- the same column extends to the same words right after the moves, behind the call and behind the prove, and to other
    words once the caller sets the default back (under which the verifiers then accept)"""
    import torch
    c = sets.c
    want = sets.run([(5, HEADER, None)])
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
        got = sets.run([(5, HEADER, 8)], between)
    finally:
        c.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
    torch.cuda.synchronize(tsa._dev())
    assert torch.equal(outs["moved"], outs["behind the call"]) and torch.equal(outs["moved"], outs["behind the prove"])
    assert not torch.equal(outs["moved"], outs["default"])
    _same(got, want)
    _accepted(got)


@pytest.mark.gpu
def test_streamed_then_resident_then_streamed_on_one_context(sets):
    """a streamed call, then a fresh set and the resident call on the same context and section, then streamed again twice: the scratch of
    that set and section is sized exactly by a streamed call (released and allocated anew behind a resident one, and between two chunk
    sizes) and grown by a resident one; the same words each time.  Free device memory behind each call is printed, not asserted: other
    processes may allocate on the same card"""
    import torch
    want = sets.run([(3, HEADER, None)])
    free = []
    for chunk in (8, None, 8, 16):
        d_caps = sets.commit()
        pair = (_sentinel(CW), _sentinel(CW))
        sets.call(3, HEADER, chunk, *pair)
        torch.cuda.synchronize(tsa._dev())
        free.append(torch.cuda.mem_get_info(tsa._dev())[0] >> 20)
        p, order, proof = sets.prove()
        caps, _ = sets.verify(p, order, proof, d_caps, {(HEADER, 3): pair})
        assert np.array_equal(caps, want["caps"]) and np.array_equal(proof, want["proof"]), chunk
    print(f"\n[sha-streamed] MiB free behind the calls (chunk 8, resident, chunk 8, chunk 16): {free}")


@pytest.mark.gpu
def test_a_second_call_behind_a_streamed_pair_is_refused(sets):
    """behind a pair whose helper IS streamed (19 proofs in chunks of 8), a second call on that section is refused in either form, and the
    set's shape stays; the same set's pair on the other section is still taken"""
    c = sets.c
    sets.commit()
    a, b, d_cap_h, d_cap_q = (_sentinel(CW) for _ in range(4))
    sets.call(4, HEADER, 8, a, b)
    before = c.trace_commit_set_shape()
    assert before[1] == [HEADER, 512, 1024, SHA256]
    for chunk in (8, 16, 24, None):
        assert "already" in _refused(lambda: sets.call(4, HEADER, chunk, d_cap_h, d_cap_q), d_cap_h, d_cap_q)
    assert c.trace_commit_set_shape() == before
    sets.call(4, SHA256, None, a, b)
    assert c.trace_commit_set_shape()[1] == [HEADER, 512, 1024, SHA256, 512, 1024]


@pytest.mark.gpu
def test_set_level_refusals(built_lib):
    """no set, constraint_set 2 or 6, a section that is no SHA-256 table or is absent, null caps, chunk_proofs 0, 3 for set 3, 4 for set 4,
    a streamed table member, a second call on the section in either form, a full set: TMX_ERR_BAD_ARG, nothing written, the shape as it was"""
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    kind, n, n_proofs, lb = 1, 2, 2, 1
    with tmx.Context(n, b"celestia", max_batch=n_proofs) as c:
        tr = _trace_rows(c, kind, n, n_proofs, 9300)
        d_caps, d_cap_h, d_cap_q = _sentinel(2 * CW), _sentinel(CW), _sentinel(CW)
        call = lambda s, sec, chunk=1 << 3, h=d_cap_h.data_ptr(), q=d_cap_q.data_ptr(): (
            lambda: c.trace_commit_set_air_sha256_streamed_device(s, sec, chunk, h, q, 0))
        assert "no commit set" in _refused(call(3, HEADER), d_cap_h, d_cap_q)
        c.trace_commit_set_device(kind, n_proofs, SHA256 | HEADER, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        before = c.trace_commit_set_shape()
        for fn in (call(2, HEADER), call(6, HEADER), call(3, TREE), call(3, 1), call(3, 128), call(4, 0), call(5, 4096),
                   call(3, HEADER, h=None), call(3, HEADER, q=None), call(3, HEADER, 0), call(4, HEADER, 0), call(5, HEADER, 0),
                   call(3, HEADER, 3), call(4, HEADER, 4), call(5, HEADER, 4)):
            _refused(fn, d_cap_h, d_cap_q)
        assert c.trace_commit_set_shape() == before
        a, b = _sentinel(CW), _sentinel(CW)
        c.trace_commit_set_air_sha256_streamed_device(5, SHA256, 8, a.data_ptr(), b.data_ptr(), 0)   # (one chunk: the resident form)
        assert "already" in _refused(call(5, SHA256, 1 << 3), d_cap_h, d_cap_q)
        c.trace_commit_set_air_sha256_streamed_device(4, HEADER, 8, a.data_ptr(), b.data_ptr(), 0)
        c.trace_commit_set_air_sha256_streamed_device(3, HEADER, 2, a.data_ptr(), b.data_ptr(), 0)
        assert "already" in _refused(call(4, HEADER), d_cap_h, d_cap_q)
        assert "already" in _refused(lambda: c.trace_commit_set_air_sha256_sched_device(HEADER, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0),
                                     d_cap_h, d_cap_q)
        assert "already" in _refused(call(3, HEADER, 2), d_cap_h, d_cap_q)
        assert c.trace_commit_set_shape()[1] == [HEADER, 128, 256, 512, 1024, SHA256, 2048, 4096]
        assert "room" in _refused(call(5, HEADER), d_cap_h, d_cap_q)  # (eight oracles: a full set)
        c.trace_commit_set_streamed_device(kind, n_proofs, SHA256 | HEADER, HEADER, 8, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        for s in SETS:
            assert "streamed" in _refused(call(s, HEADER), d_cap_h, d_cap_q)
