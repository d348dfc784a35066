"""The streamed helpers of the SHA-256 sets (include/tmx.h "streamed helpers of the SHA-256 sets") at every shape they branch on and at the
shape of the workload: the piece forms k_air_{sha,sched,init}_quotient<AIR_FORM_PIECE | AIR_FORM_PIECE_ACC> with a large first proof, at
blow-up 64, N = 2048, cap heights 0 and "the leaf level", on extreme words and onto words the CALLER left in d_quot; the set-level
tmx_trace_commit_set_air_sha256_streamed_device on TREE (T.5: chain = 1 with live second blocks), at blow-up 4 and 8, cap heights 0, 4 and
12, at every chunk edge, beside a streamed TABLE member in one prove, and across sizes on one context.  The yardsticks stay what they are:
tests/sha_air_model.py, sha_sched_model.py, sha_init_model.py and sha_streamed_model.py over tests/batch_model.py, word for word, and the
resident calls.  No tolerances: uint64 words, verdict lists and guard words are compared for equality.  The fixtures and the plumbing are
those of tests/test_sha_air.py and its siblings; docs/kernels.md "the piece forms and the streamed call: which test reaches which shape"
is the map."""
import os
import re

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
import test_sha_streamed as tst
from test_fri import _down, _sentinel, _shift, _up
from test_sha_air import ctx  # noqa: F401  (a fixture)
from test_sha_air import GUARD, _cap, _random_ext, _refused, _tree
from test_sha_air_shapes import EDGE_WORDS, FILLS
from test_sha_streamed import _accepted, _between_guards, _bytes_formula, _guards_intact, _same

P = fm.P
SHA512, SHA256, TREE, HEADER = 2, 4, 16, 32
H3, Q3, H4, Q4, H5, Q5 = 128, 256, 512, 1024, 2048, 4096
W = 9
HC = tst.HC
SETS = (3, 4, 5)
CHAIN = tsi.CHAIN
SET_OF = {H3: 3, Q3: 3, H4: 4, Q4: 4, H5: 5, Q5: 5}
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- CPU
def test_the_scratch_accessor_exists(built_lib):
    """tmx_trace_commit_set_air_sha256_scratch_bytes is in the built library, bound in _lib.py and wrapped in context.py"""
    from tendermintx_amd.context import Context
    assert built_lib.tmx_trace_commit_set_air_sha256_scratch_bytes.argtypes
    assert callable(Context.trace_commit_set_air_sha256_scratch_bytes)


def test_the_map_names_tests_that_exist():
    """every test id of this file that docs/kernels.md names is a test of this file, and every GPU test of this file is named there"""
    text = open(os.path.join(HERE, "..", "docs", "kernels.md")).read()
    named = set(re.findall(r"test_sha_streamed_shapes\.py::(test_\w+)", text))
    assert len(named) >= 10
    here = {k for k, v in globals().items() if k.startswith("test_") and callable(v)}
    assert named <= here, named - here
    gpu = {k for k in here if any(m.name == "gpu" for m in getattr(globals()[k], "pytestmark", []))}
    assert gpu <= named, gpu - named


@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("set_id,chain", [(3, 0), (4, 0), (5, 0), (5, 1)])
def test_model_pieces_of_extreme_words_sum_to_the_whole(oracle, set_id, chain, fill):
    """N = 128, blow-up 2, two proofs of the four fills: the models' pieces [0, 1) and [1, 2) sum to the models' whole quotient, which is
    canonical and not zero -- the reference alone satisfies what the GPU tests below assert"""
    log_n, lb, n_proofs = 8, 1, 2
    rng = np.random.default_rng(12000 + set_id)
    ext, hext = FILLS[fill](rng, (n_proofs * W, 1 << log_n)), FILLS[fill](rng, (n_proofs * HC[set_id], 1 << log_n))
    g = (0x0123456789ABCDEF % P, 0xFEDCBA9876543210 % P)
    want = st.whole(set_id, oracle, log_n, lb, n_proofs, chain, ext, hext, _shift(), g)
    a = st.piece(set_id, oracle, log_n, lb, chain, 0, 1, ext, hext, _shift(), g)
    b = st.piece(set_id, oracle, log_n, lb, chain, 1, 2, ext, hext, _shift(), g)
    assert want.any() and int(want.max()) < P
    assert np.array_equal(st.add(a, b), want)


# ---- GPU: the range calls
def _qcall(ctx, set_id, log_n, lb, cap_h, n_proofs, chain, ptrs, **kw):
    mode = (chain,) if set_id == 5 else ()
    tst._quotient_call(ctx, set_id)(log_n, lb, cap_h, n_proofs, *mode, *ptrs, 0, **kw)


def _model_gamma(oracle, set_id, log_n, lb, cap_h, n_proofs, chain, cap, cap_helper):
    mode = (chain,) if set_id == 5 else ()
    return st.MODELS[set_id].gamma(oracle, log_n, lb, cap_h, n_proofs, *mode, cap, cap_helper)


class _Range:
    """extended table and helper columns on the device, both caps, and the WHOLE call's words and gamma; pieces() runs range calls over
    helper buffers that hold one piece each between guard words"""

    def __init__(self, ctx, set_id, log_n, lb, cap_h, n_proofs, chain, ext, hext):
        import torch
        self.ctx, self.args, self.hc, self.M = ctx, (set_id, log_n, lb, cap_h, n_proofs, chain), HC[set_id], 1 << log_n
        self.ext, self.hext = ext, hext
        self.d_cols, d_hcols = _up(ext), _up(hext)
        self.trees = (_tree(ctx, self.d_cols, log_n, n_proofs * W, cap_h), _tree(ctx, d_hcols, log_n, n_proofs * self.hc, cap_h))
        self.caps = [t[1].data_ptr() for t in self.trees]
        whole = _sentinel(2 * self.M + 2 * GUARD)
        _qcall(ctx, *self.args, [self.d_cols.data_ptr(), d_hcols.data_ptr(), *self.caps, whole[GUARD:].data_ptr()])
        torch.cuda.synchronize(tsa._dev())
        self.g = ctx.air_last_gamma()
        assert _guards_intact(whole)
        self.whole = _down(whole[GUARD:GUARD + 2 * self.M])
        self.bufs = {}

    def model_gamma(self, oracle):
        set_id, log_n, lb, cap_h, n_proofs, chain = self.args
        return _model_gamma(oracle, set_id, log_n, lb, cap_h, n_proofs, chain, _down(self.trees[0][1]), _down(self.trees[1][1]))

    def model_whole(self, oracle):
        set_id, log_n, lb, _, n_proofs, chain = self.args
        return st.whole(set_id, oracle, log_n, lb, n_proofs, chain, self.ext, self.hext, _shift(), self.g)

    def model_piece(self, oracle, lo, hi):
        set_id, log_n, lb, _, _, chain = self.args
        return st.piece(set_id, oracle, log_n, lb, chain, lo, hi, self.ext, self.hext, _shift(), self.g)

    def pieces(self, order, prefill=None, first_accumulates=False):
        """the range calls of `order` in turn into one d_quot between guard words (sentinel-filled, or holding `prefill`); the first with
        accumulate = 0 unless first_accumulates; gamma is the whole call's after every piece and every guard is intact"""
        import torch
        out = _sentinel(2 * self.M + 2 * GUARD) if prefill is None else _between_guards(prefill)
        for k, (lo, hi) in enumerate(order):
            if (lo, hi) not in self.bufs:
                self.bufs[(lo, hi)] = _between_guards(self.hext[lo * self.hc:hi * self.hc].reshape(-1))
            piece = self.bufs[(lo, hi)]
            _qcall(self.ctx, *self.args, [self.d_cols.data_ptr(), piece[GUARD:].data_ptr(), *self.caps, out[GUARD:].data_ptr()],
                   proof_range=(lo, hi), accumulate=int(k > 0 or first_accumulates))
            torch.cuda.synchronize(tsa._dev())
            assert self.ctx.air_last_gamma() == self.g, (lo, hi)
            assert _guards_intact(piece) and _guards_intact(out), (lo, hi)
        return _down(out[GUARD:GUARD + 2 * self.M])


def _equal(got, want, what):
    diff = np.flatnonzero(got != want)[:10]
    assert not len(diff), (what, diff.tolist())


MANY = 259  # first = 256 and 258: the weight's exponent C first passes 2^16 for every set (315 x 256 = 80640)


@pytest.mark.gpu
@pytest.mark.parametrize("set_id", SETS)
def test_pieces_with_a_large_first_proof(ctx, oracle, set_id):
    """N = 64, blow-up 2, 259 proofs of random columns (the helpers of sets 3 and 5 are about 83 MB extended): the pieces [0, 256),
    [256, 258) and [258, 259), ascending and descending, leave the whole call's words; [256, 258) and [258, 259), each alone with
    accumulate = 0 onto a sentinel-filled d_quot, equal sha_streamed_model.piece word for word -- the weight gamma^(C first) with
    C first up to 337 x 258, the table read from proof `first` on.  gamma is the whole call's after every piece"""
    log_n, lb, cap_h = 7, 1, 2
    rng = np.random.default_rng(13000 + set_id)
    r = _Range(ctx, set_id, log_n, lb, cap_h, MANY, 0, _random_ext(rng, MANY * W, log_n), _random_ext(rng, MANY * HC[set_id], log_n))
    assert r.g == r.model_gamma(oracle)
    cuts = [(0, 256), (256, 258), (258, 259)]
    for order in (cuts, cuts[::-1]):
        _equal(r.pieces(order), r.whole, order)
    for lo, hi in cuts[1:]:
        _equal(r.pieces([(lo, hi)]), r.model_piece(oracle, lo, hi), (lo, hi))


GEOMETRY = ([(s, 6, 6, 2, 0) for s in SETS] + [(5, 7, 6, 2, 1)] + [(3, 11, 2, 2, 0), (4, 11, 2, 2, 0), (5, 11, 2, 2, 1)]
            + [(s, 6, 1, h, 0) for s in SETS for h in (0, 7)])


@pytest.mark.gpu
@pytest.mark.parametrize("set_id,log_rows,log_blowup,cap_height,chain", GEOMETRY)
def test_pieces_at_every_table_geometry(ctx, oracle, set_id, log_rows, log_blowup, cap_height, chain):
    """two proofs of random columns in the pieces [0, 1) + [1, 2), both orders, against the whole call and against the model's whole
    quotient (gamma against the model's too): blow-up 64 at N = 64 (4096-entry S / K / F tables) and, for set 5 with chain = 1, at
    N = 128 (the 8192-entry D_s table; a shape no whole call ran at either); N = 2048 at blow-up 4, set 5 chained; N = 64 at blow-up 2
    with cap height 0 and with cap height 7, where the cap is the whole leaf level and gamma absorbs 2 x 512 words"""
    log_n = log_rows + log_blowup
    rng = np.random.default_rng(14000 + 1000 * set_id + 100 * log_rows + 10 * log_blowup + cap_height)
    r = _Range(ctx, set_id, log_n, log_blowup, cap_height, 2, chain, _random_ext(rng, 2 * W, log_n), _random_ext(rng, 2 * HC[set_id], log_n))
    assert r.g == r.model_gamma(oracle)
    _equal(r.whole, r.model_whole(oracle), "the whole call against the model")
    for order in ([(0, 1), (1, 2)], [(1, 2), (0, 1)]):
        _equal(r.pieces(order), r.whole, order)


def _filled(fill, set_id, log_n, n_proofs):
    rng = np.random.default_rng(15000 + 10 * log_n + set_id)
    return FILLS[fill](rng, (n_proofs * W, 1 << log_n)), FILLS[fill](rng, (n_proofs * HC[set_id], 1 << log_n))


@pytest.mark.gpu
@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("set_id,N,log_blowup,n_proofs,chain", [(4, 64, 3, 2, 0), (5, 64, 3, 2, 0), (4, 128, 4, 1, 0), (5, 128, 4, 1, 1)])
def test_quotient_of_extreme_words_in_sets_4_and_5(ctx, oracle, set_id, N, log_blowup, n_proofs, chain, fill):
    """what test_sha_air_shapes.test_quotient_of_extreme_words_equals_the_model does for set 3: every word p - 1, every word 2^64 - 1,
    random non-canonical words and random edge words as table and helper columns through the lazy gamma sums of sets 4 and 5 (set 5
    chained at N = 128): the whole call's words and gamma equal the model's"""
    log_n = N.bit_length() - 1 + log_blowup
    ext, hext = _filled(fill, set_id, log_n, n_proofs)
    r = _Range(ctx, set_id, log_n, log_blowup, 2, n_proofs, chain, ext, hext)
    assert r.g == r.model_gamma(oracle)
    want = r.model_whole(oracle)
    assert want.any() and int(want.max()) < P
    _equal(r.whole, want, fill)


@pytest.mark.gpu
@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("set_id", SETS)
def test_pieces_of_extreme_words(ctx, oracle, set_id, fill):
    """the same fills in piece form at N = 64, blow-up 8, two proofs: [0, 1), then [1, 2) accumulated, equal the whole call's words and the
    model's; the first piece alone equals the model's piece"""
    log_n, lb = 9, 3
    ext, hext = _filled(fill, set_id, log_n, 2)
    r = _Range(ctx, set_id, log_n, lb, 2, 2, 0, ext, hext)
    want = r.model_whole(oracle)
    assert want.any() and int(want.max()) < P
    _equal(r.whole, want, "the whole call against the model")
    _equal(r.pieces([(0, 1)]), r.model_piece(oracle, 0, 1), "the first piece")
    _equal(r.pieces([(0, 1), (1, 2)]), want, fill)


@pytest.mark.gpu
@pytest.mark.parametrize("set_id", SETS)
def test_accumulating_onto_the_callers_words(ctx, oracle, set_id):
    """N = 64, blow-up 2, three proofs; d_quot holds a seeded choice of edge words (0, p - 1, p, p + 1, 2^64 - 1 ...) that the CALLER put
    there, and the single piece [0, 3) runs with accumulate = 1: "added to what d_quot holds and written canonical" -- every word is
    below p and equals sha_streamed_model.add(prefill, whole)"""
    log_n, lb, n_proofs = 7, 1, 3
    rng = np.random.default_rng(16000 + set_id)
    r = _Range(ctx, set_id, log_n, lb, 2, n_proofs, 0, _random_ext(rng, n_proofs * W, log_n), _random_ext(rng, n_proofs * HC[set_id], log_n))
    whole = r.model_whole(oracle)
    _equal(r.whole, whole, "the whole call against the model")
    prefill = rng.choice(EDGE_WORDS, 2 << log_n)
    assert set(int(x) for x in EDGE_WORDS) == set(int(x) for x in prefill)  # (every edge word occurs)
    got = r.pieces([(0, n_proofs)], prefill=prefill, first_accumulates=True)
    assert int(got.max()) < P
    _equal(got, st.add(prefill, whole), "prefill + whole")


# ---- GPU: the set level
class _Sets:
    """one context and one batch of step trace rows; run() commits a fresh set of `sections` over the first n_proofs proofs (members of the
    mask `streamed` through tmx_trace_commit_set_streamed_device), makes the given set-level calls -- (set id, section, chunk_proofs or
    None for the resident call) -- proves and verifies.  Results are kept by their arguments.  The parametrised sibling of
    test_sha_streamed._Sets"""

    def __init__(self, n, max_proofs, seed):
        import tendermintx_amd as tmx
        from test_merkle_open import _trace_rows
        self.n, self.max_proofs = n, max_proofs
        self.c = tmx.Context(n, b"celestia", max_batch=max_proofs)
        self.tr = _trace_rows(self.c, 1, n, max_proofs, seed)
        self.kept = {}

    def tables(self, section, n_proofs):
        """[9 n_proofs][rows padded to a power of two] pre-LDE columns of `section` from the device's trace rows"""
        off, rows, width = tsa._section_geom(1, self.n, section)
        assert width == W
        table = np.zeros((n_proofs * W, 1 << max(6, (rows - 1).bit_length())), dtype=np.uint64)
        for q, full in enumerate(_down(self.tr)[:n_proofs]):
            table[q * W:(q + 1) * W, :rows] = full[off:off + rows * W].reshape(rows, W).T
        return table

    def commit(self, sections, n_proofs, lb, cap_h, streamed=0, chunk_cols=8):
        """{section: its cap on the device}; the caps between guard words"""
        import torch
        c = self.c
        room = bin(sections).count("1") * (4 << cap_h)
        buf = _sentinel(room + 2 * GUARD)
        if streamed:
            c.trace_commit_set_streamed_device(1, n_proofs, sections, streamed, chunk_cols, lb, cap_h, self.tr.data_ptr(), buf[GUARD:].data_ptr(), 0)
        else:
            c.trace_commit_set_device(1, n_proofs, sections, lb, cap_h, self.tr.data_ptr(), buf[GUARD:].data_ptr(), 0)
        torch.cuda.synchronize(tsa._dev())
        shape, order = c.trace_commit_set_shape()
        widths = [4 << min(cap_h, ln) for ln in shape["log_n"]]
        used = GUARD + sum(widths)
        assert torch.equal(buf[:GUARD], _sentinel(GUARD)) and torch.equal(buf[used:], _sentinel(len(buf) - used))
        out, at = {}, GUARD
        for sec, w in zip(order, widths):
            out[sec] = buf[at:at + w]
            at += w
        return out

    def call(self, set_id, section, chunk, width):
        """(d_cap_h, d_cap_q) of one set-level call, each written between guard words"""
        import torch
        c = self.c
        bufs = (_sentinel(width + 2 * GUARD), _sentinel(width + 2 * GUARD))
        ptrs = [b[GUARD:].data_ptr() for b in bufs]
        if chunk is None:
            {3: c.trace_commit_set_air_sha256_device, 4: c.trace_commit_set_air_sha256_sched_device,
             5: c.trace_commit_set_air_sha256_init_device}[set_id](section, *ptrs, 0)
        else:
            c.trace_commit_set_air_sha256_streamed_device(set_id, section, chunk, *ptrs, 0)
        torch.cuda.synchronize(tsa._dev())
        assert _guards_intact(bufs[0]) and _guards_intact(bufs[1])
        return tuple(b[GUARD:GUARD + width] for b in bufs)

    def prove(self, n_queries):
        c = self.c
        shape, order = c.trace_commit_set_shape()
        p = dict(shape, arity_bits=2, final_log_max=2, n_queries=n_queries, pow_bits=0)
        proof = tsa._guarded(bm.layout(p)["words"], lambda o: c.trace_commit_set_prove_device(p, o, 0))
        assert c.fri_last_degree_ok() is True
        return p, order, _down(proof)

    def verify(self, p, order, words, table_cap, pairs):
        """(all caps on the device in oracle order, {"batch": verdicts, (section, set id): (verdicts, verdicts with that pair's quotient
        opening bumped)})"""
        import torch
        c = self.c
        caps, where, table, k_table = [], {}, None, None
        for k, sec in enumerate(order):
            if sec in table_cap:
                table, k_table = sec, k
                caps.append(table_cap[sec])
                continue
            set_id, is_q = SET_OF[sec], sec in (Q3, Q4, Q5)
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
        return all_caps, verdicts

    def run(self, sections, n_proofs, lb, cap_h, calls, streamed=0, chunk_cols=8, n_queries=6, fresh=False):
        key = (sections, n_proofs, lb, cap_h, tuple(calls), streamed, chunk_cols, n_queries)
        if key in self.kept and not fresh:
            return self.kept[key]
        table_cap = self.commit(sections, n_proofs, lb, cap_h, streamed, chunk_cols)
        pairs, gammas, scratch = {}, {}, {}
        for set_id, section, chunk in calls:
            pairs[(section, set_id)] = self.call(set_id, section, chunk, len(table_cap[section]))
            gammas[(section, set_id)] = self.c.air_last_gamma()
            scratch[(section, set_id)] = self.c.trace_commit_set_air_sha256_scratch_bytes(set_id, section)
        p, order, proof = self.prove(n_queries)
        all_caps, verdicts = self.verify(p, order, proof, table_cap, pairs)
        out = dict(p=p, order=order, caps=_down(all_caps), d_caps=all_caps, proof=proof, verdicts=verdicts, gammas=gammas, scratch=scratch)
        self.kept[key] = out
        return out


@pytest.fixture(scope="module")
def tree_sets(built_lib):
    """step N = 3, ten proofs: TREE has 512 rows (padding, zero blocks and chained second blocks), SHA256 256, SHA512 512"""
    s = _Sets(3, 10, 9900)
    yield s
    s.c.close()


@pytest.fixture(scope="module")
def sha_sets(built_lib):
    """step N = 2, seventeen proofs: SHA256 has 128 rows, HEADER 4096"""
    s = _Sets(2, 17, 9300)
    yield s
    s.c.close()


def _nbytes(set_id, r, section, n_proofs, chunk):
    from tendermintx_amd.context import trace_commit_set_air_sha256_streamed_bytes as nbytes
    log_m = r["p"]["log_n"][r["order"].index(section)]
    return nbytes(set_id, log_m, r["p"]["log_blowup"], r["p"]["cap_height"], n_proofs, chunk)


TREE_SHAPE = (TREE | SHA256, 10, 2, 2)  # (sections, proofs, log_blowup, cap height)


@pytest.mark.gpu
def test_tree_rows_are_not_degenerate(tree_sets):
    """the T.5 rows the tests below stream: set 3's LIVE and set 5's LV columns (the models' helpers of the device's trace rows) are
    neither all one nor all zero, and live SECOND blocks occur -- set 5's chained sum is not trivial on them, as it is on HEADER"""
    table = tree_sets.tables(TREE, 10)
    assert table.shape == (90, 512)
    live = sm.helper(table, 10)[sm.HLIVE::sm.HELPER_COLS]
    lv = si.helper(table, 10, 1)[si.HLV::si.HELPER_COLS]
    for col in (live, lv):
        assert col.any() and not col.all() and int(col.max()) == 1
    blocks = lv.reshape(10, -1, 64)[:, :, 0]
    assert blocks[:, 1::2].any() and not blocks[:, 1::2].all()


@pytest.mark.gpu
@pytest.mark.parametrize("set_id", SETS)
def test_streamed_call_on_the_tree_table_equals_the_resident_call(tree_sets, set_id):
    """step N = 3, TREE | SHA256, ten proofs, blow-up 4, cap height 2; the set's call on TREE (set 5 with chain = 1) streamed in chunks of 8
    proofs (8 + 2), and for set 3 in chunks of 2, against the resident call: the same d_cap_h, d_cap_q, gamma, shape and order and every
    proof word; the set's device verifier and tmx_batch_verify_device accept every query; with the quotient's opening bumped every query
    is rejected; the streamed scratch is exactly what _streamed_bytes says"""
    want = tree_sets.run(*TREE_SHAPE, [(set_id, TREE, None)])
    assert want["order"] == [TREE, tst.HELPER_ID[set_id], 2 * tst.HELPER_ID[set_id], SHA256] and want["p"]["log_n"] == [11, 11, 11, 10]
    _accepted(want)
    for chunk in ((8, 2) if set_id == 3 else (8,)):
        got = tree_sets.run(*TREE_SHAPE, [(set_id, TREE, chunk)], fresh=True)
        _same(got, want)
        _accepted(got)
        assert got["scratch"][(TREE, set_id)] == _nbytes(set_id, got, TREE, 10, chunk)[0]


@pytest.mark.gpu
def test_three_streamed_sets_on_the_tree_table(tree_sets):
    """all three sets streamed on TREE in the call order 5-3-4 (chunks of 8, 2 and 8 proofs) against all three resident in the order
    3-4-5: the eight oracles [TREE, H3, Q3, H4, Q4, H5, Q5, SHA256] are a full set; the same caps, gammas and proof; all verifiers accept"""
    want = tree_sets.run(*TREE_SHAPE, [(3, TREE, None), (4, TREE, None), (5, TREE, None)])
    got = tree_sets.run(*TREE_SHAPE, [(5, TREE, 8), (3, TREE, 2), (4, TREE, 8)])
    assert got["order"] == [TREE, H3, Q3, H4, Q4, H5, Q5, SHA256]
    _same(got, want)
    _accepted(want)
    _accepted(got)
    assert sorted(k for k in got["verdicts"] if k != "batch") == [(TREE, 3), (TREE, 4), (TREE, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("set_id", [4, 5])
def test_sets_4_and_5_on_the_tree_table_against_the_models(tree_sets, oracle, set_id):
    """the twin of test_sha_air_shapes.test_set_level_on_the_tree_table: step N = 3, two proofs, blow-up 2, the resident call of set 4 and
    of set 5 (chain = 1) on TREE: the table's cap, the helper's cap (through the device's Poseidon tree over the MODEL's helper words),
    gamma and the quotient's cap against the model; one proof over the four oracles: the device's verdicts equal the model verifier's (all
    accept), and a bumped helper opening is rejected by both.  With the streamed tests above this ties the streamed TREE words to the models"""
    from test_merkle_open import _oracle_ext
    n_proofs, lb, cap_h, cw = 2, 1, 2, 4 << 2
    m, hc, chain = st.MODELS[set_id], HC[set_id], (1,) if set_id == 5 else ()
    r = tree_sets.run(TREE | SHA256, n_proofs, lb, cap_h, [(set_id, TREE, None)], n_queries=3)
    p, caps, got, c = r["p"], r["caps"], r["proof"], tree_sets.c
    assert r["order"] == [TREE, tst.HELPER_ID[set_id], 2 * tst.HELPER_ID[set_id], SHA256]
    assert p["log_n"] == [9 + lb] * 3 + [8 + lb] and p["n_cols"] == [W * n_proofs, hc * n_proofs, 2, W * n_proofs]
    e, lm, nc = _oracle_ext(oracle, 1, 3, _down(tree_sets.tr)[:n_proofs], TREE, lb)
    assert (lm, nc) == (9 + lb, W * n_proofs)
    ext = e.reshape(nc, -1)
    table = tree_sets.tables(TREE, n_proofs)
    help_ = m.helper(table, n_proofs, *chain)
    hext = oracle.lde(help_, lb)
    assert np.array_equal(caps[:cw], _cap(oracle, ext, lm))
    assert np.array_equal(caps[cw:2 * cw], _down(_tree(c, _up(hext), lm, n_proofs * hc)[1]))
    g = m.gamma(oracle, lm, lb, cap_h, n_proofs, *chain, caps[:cw], caps[cw:2 * cw])
    assert r["gammas"][(TREE, set_id)] == g
    quot = m.quotient(oracle, lm, lb, n_proofs, *chain, ext, hext, _shift(), g)
    assert np.array_equal(caps[2 * cw:3 * cw], _cap(oracle, quot.reshape(2, -1), lm))
    device = (lambda w: tss._verdicts(c, p, 0, 1, r["d_caps"], w)) if set_id == 4 else (lambda w: tsi._verdicts(c, p, 0, 1, 1, r["d_caps"], w))
    model = m.verify(oracle, p, 0, 1, *chain, caps, got, _shift())
    assert all(model) and device(got) == model
    bad = tsi._bumped(got, bm.layout(p)["off_open"][1] + hc + (ss.HQ + 4 if set_id == 4 else si.HLV))
    assert not m.identity(oracle, p, 0, 1, *chain, caps, bad)  # (so the model verifier rejects every query whatever the batch proof says)
    assert device(bad) == [False] * p["n_queries"]


# (the set's other table, log_blowup, cap height, proofs, chunk_proofs): blow-up 8 and 4, cap heights 0, 4 and 12 (SHA256's tree has 10 levels
# at blow-up 8: the cap is its leaf level), two full chunks with `last` on a chunk boundary, a last chunk of one proof, one chunk that holds
# everything.  Beside cap height 12 stands SHA512 (2^12 extended rows, just enough for the cap): the transcript is one lane, and HEADER's
# 2^15 rows would double the 4096-digest caps it absorbs per prove and per verifier
EDGES = [(HEADER, 3, 0, 16, 8), (HEADER, 2, 4, 16, 8), (SHA512, 3, 12, 16, 8), (HEADER, 1, 2, 17, 16), (HEADER, 1, 2, 16, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("other,log_blowup,cap_height,n_proofs,chunk", EDGES)
@pytest.mark.parametrize("set_id", SETS)
def test_streamed_call_at_every_blowup_cap_and_chunk_edge(sha_sets, set_id, other, log_blowup, cap_height, n_proofs, chunk):
    """step N = 2, SHA256 | HEADER (SHA256 | SHA512 under cap height 12), the set's call on SHA256 (N = 128) streamed against resident, by the equalities of the TREE test.  With
    16 proofs every helper's column total is a multiple of 8.  chunk_proofs == n_proofs takes the resident path: _streamed_bytes returns
    the resident formula and the scratch holds at least that; every other case leaves exactly the streamed bytes"""
    shape = (SHA256 | other, n_proofs, log_blowup, cap_height)
    want = sha_sets.run(*shape, [(set_id, SHA256, None)])
    _accepted(want)
    assert want["p"]["log_n"][want["order"].index(SHA256)] == 7 + log_blowup
    got = sha_sets.run(*shape, [(set_id, SHA256, chunk)], fresh=True)
    _same(got, want)
    _accepted(got)
    log_m = 7 + log_blowup
    nbytes = _nbytes(set_id, got, SHA256, n_proofs, chunk)
    assert nbytes == _bytes_formula(set_id, log_m, log_blowup, cap_height, n_proofs, chunk)
    if chunk >= n_proofs:
        resident = (HC[set_id] * n_proofs * ((1 << 7) + (1 << log_m)) + (2 << log_m)) * 8 + 2 * tst._digests(log_m, min(cap_height, log_m)) * 32
        assert nbytes[0] == resident and got["scratch"][(SHA256, set_id)] >= resident
    else:
        assert got["scratch"][(SHA256, set_id)] == nbytes[0] < _nbytes(set_id, got, SHA256, n_proofs, 1 << 20)[0]


@pytest.mark.gpu
def test_set_3_in_eight_chunks_of_two(sha_sets):
    """set 3 on SHA256, 16 proofs in chunks of 2: eight chunks, the sponge states carried across seven seams"""
    shape = (SHA256 | HEADER, 16, 1, 2)
    want = sha_sets.run(*shape, [(3, SHA256, None)])
    got = sha_sets.run(*shape, [(3, SHA256, 2)], fresh=True)
    _same(got, want)
    _accepted(got)
    assert got["scratch"][(SHA256, 3)] == _nbytes(3, got, SHA256, 16, 2)[0]


@pytest.mark.gpu
def test_a_streamed_table_member_beside_streamed_helpers(tree_sets):
    """step N = 3, SHA512 | TREE, ten proofs, blow-up 2: SHA512 streamed through tmx_trace_commit_set_streamed_device (chunks of 8 columns:
    the set's shared chunk buffer) and sets 3, 4 and 5 streamed on TREE (chunks of 2, 8 and 8 proofs: a chunk buffer each) in ONE prove
    over a full set of eight oracles, against the set committed resident with the three resident calls: the shape, every cap and every
    proof word are equal and all verifiers accept; the helpers' scratches are the chunked form's bytes; a call on the streamed SHA512
    member stays refused"""
    shape = (SHA512 | TREE, 10, 1, 2)
    want = tree_sets.run(*shape, [(3, TREE, None), (4, TREE, None), (5, TREE, None)])
    calls = [(3, TREE, 2), (4, TREE, 8), (5, TREE, 8)]
    got = tree_sets.run(*shape, calls, streamed=SHA512, chunk_cols=8, fresh=True)
    assert got["order"] == [SHA512, TREE, H3, Q3, H4, Q4, H5, Q5] and got["p"]["n_cols"][0] == 180
    _same(got, want)
    _accepted(want)
    _accepted(got)
    for set_id, _, chunk in calls:
        assert got["scratch"][(TREE, set_id)] == _nbytes(set_id, got, TREE, 10, chunk)[0] < want["scratch"][(TREE, set_id)]
    c = tree_sets.c
    tree_sets.commit(SHA512 | TREE, 10, 1, 2, streamed=SHA512, chunk_cols=8)
    a, b = _sentinel(16), _sentinel(16)
    for set_id in SETS:
        _refused(lambda: c.trace_commit_set_air_sha256_streamed_device(set_id, SHA512, 8, a.data_ptr(), b.data_ptr(), 0), a, b)
    assert c.trace_commit_set_shape()[1] == [SHA512, TREE]
    tree_sets.commit(SHA512 | TREE, 10, 1, 2, streamed=TREE, chunk_cols=8)
    for set_id in SETS:
        assert "streamed" in _refused(lambda: c.trace_commit_set_air_sha256_streamed_device(set_id, TREE, 8, a.data_ptr(), b.data_ptr(), 0), a, b)


@pytest.mark.gpu
def test_scratch_across_sizes_on_one_context(tree_sets):
    """one context (max_batch 10), set 3 on TREE in chunks of 2: a streamed call at ten proofs, then a fresh set at four proofs streamed
    with the same chunk -- the exact-size rule releases the scratch and allocates the smaller one -- then ten again; each run's words are
    that size's resident words"""
    sizes = {}
    for n_proofs in (10, 4, 10):
        shape = (TREE | SHA256, n_proofs, 1, 2)
        want = tree_sets.run(*shape, [(3, TREE, None)])
        got = tree_sets.run(*shape, [(3, TREE, 2)], fresh=True)
        _same(got, want)
        _accepted(got)
        sizes[n_proofs] = got["scratch"][(TREE, 3)]
        assert sizes[n_proofs] == _nbytes(3, got, TREE, n_proofs, 2)[0]
    assert sizes[4] < sizes[10]
