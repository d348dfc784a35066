"""Constraint sets 1 and 2 (the ladders' 33 + 32 constraints: the first twelve kernels of air.hip and the air_* host path of api.cpp) at
every grid shape, table size and row value they branch on; docs/kernels.md "Sets 1 and 2, the ladders' constraints: which test reaches
which shape" is the map.  The yardsticks are tests/test_air.py's and tests/test_air_boundary.py's: air_model.py, air_boundary_model.py and
batch_model.py.  Device words equal the model's word for word, verdicts verdict for verdict, every device output sits between guard
words; there is no tolerance anywhere.  The CPU part keeps the references honest: the models' uint64 path against plain Python integers
on the extreme fills, and the honest tables of the verifier tests -- tilings of the CPU oracle's real 256-row ladders -- against the
constraints as integers and against the degree bound."""
import time

import numpy as np
import pytest

import air_boundary_model as abm
import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import test_air as ta
import test_air_boundary as tab
from batch_model import bparams
from fri_model import e_add, e_mul, e_scale, e_sub
from test_fri import _down, _sentinel, _shift, _up

P = fm.P
W, PW = am.WIDTH, abm.PUB_WIDTH
CAP_H, GUARD, E2E = ta.CAP_H, ta.GUARD, ta.E2E
_dev, _refused = ta._dev, ta._refused
ZETA = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)

EDGE_WORDS = np.array([0, 1, P - 1, P, P + 1, (1 << 64) - 1, (1 << 32) - 1, 1 << 32, 1 << 63], dtype=np.uint64)
FILLS = {
    "all p - 1": lambda rng, shape: np.full(shape, P - 1, dtype=np.uint64),
    "all 2^64 - 1": lambda rng, shape: np.full(shape, (1 << 64) - 1, dtype=np.uint64),
    "random in [p, 2^64)": lambda rng, shape: rng.integers(P, 1 << 64, shape, dtype=np.uint64),
    "edge words": lambda rng, shape: rng.choice(EDGE_WORDS, shape),
}


# ---- the two models behind one signature (boundary: set 2)
def _gamma(oracle, boundary, log_n, log_blowup, cap_height, n_proofs, cap, pub):
    if boundary:
        return abm.gamma(oracle, log_n, log_blowup, cap_height, n_proofs, cap, pub)
    return am.gamma(oracle, log_n, log_blowup, cap_height, n_proofs, cap)


def _model(oracle, boundary, log_n, log_blowup, n_proofs, ext, pub, g, proofs=None):
    if boundary:
        return abm.quotient(oracle, log_n, log_blowup, n_proofs, ext, pub, _shift(), g, proofs=proofs)
    return am.quotient(oracle, log_n, log_blowup, n_proofs, ext, _shift(), g, proofs=proofs)


def _model_verdicts(oracle, boundary, p, k_trace, caps, proof, pub):
    """[ok and holds] per query.  Where the identity fails that is False for every query whatever batch_model.verify says, so its time
    over thousands of columns is only spent on a proof whose identity holds"""
    if boundary:
        if not abm.identity(oracle, p, k_trace, caps, proof, pub):
            return [False] * p["n_queries"]
        return abm.verify(oracle, p, k_trace, caps, proof, _shift(), pub)
    if not am.identity(oracle, p, k_trace, caps, proof):
        return [False] * p["n_queries"]
    return am.verify(oracle, p, k_trace, caps, proof, _shift())


def _plain_quotient(oracle, boundary, log_n, log_blowup, n_proofs, cols, pub, g):
    """the header's definition in plain Python integers, point by point: no numpy arithmetic and no uint64 anywhere behind the first line
    of each block, Pub_gamma by Horner on the coefficients of the V_k formed here"""
    M, B = 1 << log_n, 1 << log_blowup
    N = M // B
    K, C = N // 256, 65 if boundary else 33
    cols = [[int(x) % P for x in col] for col in np.asarray(cols).reshape(n_proofs * W, M)]
    gpow = [(1, 0)]
    for _ in range(C * n_proofs + 1):
        gpow.append(e_mul(gpow[-1], g))
    inv = lambda a: pow(a, P - 2, P)
    if boundary:
        words = [[int(x) % P for x in col] for col in np.asarray(pub).reshape(n_proofs * PW, K)]
        V = []
        for k in range(K):
            v = (0, 0)
            for p in range(n_proofs):
                for l in range(16):
                    v = e_add(v, e_scale(gpow[65 * p + 33 + l], words[PW * p + l][k]))
                v = e_add(v, e_scale(gpow[65 * p + 57], words[PW * p + 16][(k + 1) % K]))
            V.append(v)
        coefs = abm.pub_coefficients(oracle, log_n, log_blowup, V)
    w, om, x = oracle.gl_root(log_n), am.omega_256_inv(oracle, log_n), _shift() % P
    out = [[], []]
    for i in range(M):
        S, Z, nx = (pow(x, N // 256, P) - om) % P, (pow(x, N, P) - 1) % P, (i + B) % M
        t, u = (0, 0), (0, 0)
        for p in range(n_proofs):
            c = cols[p * W:(p + 1) * W]
            bit = c[am.BIT][i]
            terms = [(bit * bit - bit) % P]
            terms += [(c[am.NXT + l][i] - c[am.DBL + l][i] - bit * (c[am.ADD + l][i] - c[am.DBL + l][i])) % P for l in range(16)]
            terms += [S * (c[am.ACC + l][nx] - c[am.NXT + l][i]) % P for l in range(16)]
            for j, v in enumerate(terms):
                t = e_add(t, e_scale(gpow[C * p + j], v))
            if boundary:
                for j, v in enumerate([c[am.NXT + l][i] for l in range(16)] + [c[am.ACC + l][nx] for l in range(16)]):
                    u = e_add(u, e_scale(gpow[C * p + 33 + j], v))
        q = e_scale(t, inv(Z))
        if boundary:
            px = [0, 0]
            for k in (0, 1):
                for cf in reversed(coefs[k]):
                    px[k] = (px[k] * x + cf) % P
            q = e_add(q, e_scale(e_sub(u, tuple(px)), inv(S)))
        out[0].append(q[0])
        out[1].append(q[1])
        x = x * w % P
    return np.array(out[0] + out[1], dtype=np.uint64)


# ---- CPU: the models' uint64 path on the extreme fills
@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("set_no", [1, 2])
def test_model_on_extreme_words_equals_plain_integers(oracle, set_no, fill):
    """the reference of the extreme-word tests below, at the smallest shape of each set (N = 256 resp. 512, one proof, blow-up 2): the
    models' quotient of columns (and a public table) of all p - 1, all 2^64 - 1, random words in [p, 2^64) and random edge words equals the
    definition evaluated in plain Python integers; every word of it is canonical"""
    boundary = set_no == 2
    log_rows, lb, n_proofs = 9 if boundary else 8, 1, 1
    log_n = log_rows + lb
    rng = np.random.default_rng(11900 + set_no)
    ext = FILLS[fill](rng, (n_proofs * W, 1 << log_n))
    pub = FILLS[fill](rng, (n_proofs * PW, 1 << (log_rows - 8))) if boundary else None
    assert ext.dtype == np.uint64 and (fill == "edge words" or int(ext.min()) >= P - 1)
    want = _plain_quotient(oracle, boundary, log_n, lb, n_proofs, ext, pub, ZETA)
    got = _model(oracle, boundary, log_n, lb, n_proofs, ext, pub, ZETA)
    assert got.dtype == np.uint64 and int(got.max()) < P and got.any()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


# ---- CPU: honest tables as tilings of the CPU oracle's real ladders
@pytest.fixture(scope="module")
def pool(oracle):
    """(rows [n + 1][65][256], public columns [n + 1][17]): the distinct live 256-row ladders of the step N = 2 and skip N = 4 fixtures of
    test_air_boundary.py with their Level-1 end points and live = 1; the last entry (index -1) is the dead ladder: all zero, live = 0"""
    rows, pubs, seen = [], [], set()
    for kind, n, seed in ((1, 2, 5200), (0, 4, 5100)):
        table, pub = tab._tables(oracle, kind, n, 2, seed)
        for p in range(2):
            for k in range(table.shape[1] // 256):
                lad, col = table[p * W:(p + 1) * W, 256 * k:256 * k + 256], pub[p * PW:(p + 1) * PW, k]
                if int(col[16]) and lad.tobytes() not in seen:
                    seen.add(lad.tobytes())
                    rows.append(lad.copy())
                    pubs.append(col.copy())
    assert len(rows) >= 12, len(rows)
    rows.append(np.zeros((W, 256), dtype=np.uint64))
    pubs.append(np.zeros(PW, dtype=np.uint64))
    return np.stack(rows), np.stack(pubs)


def _draw(rng, pool, K, n_proofs, dead=(), live=()):
    """[n_proofs][K] pool indices, about one in seven of them -1 (the dead ladder); dead: (proof, ladder) pairs forced dead; live: proofs
    without a dead ladder.  Along the ladders the drawing repeats with no period that divides 256"""
    n_live = pool[0].shape[0] - 1
    seq = rng.integers(0, n_live, (n_proofs, K))
    seq[rng.random(seq.shape) < 1 / 7] = -1
    for p in live:
        seq[p] = rng.integers(0, n_live, K)
    for p, k in dead:
        seq[p, k] = -1
    d = 1
    while d <= 256 and d < K:
        assert (seq != np.roll(seq, d, axis=1)).any(), d
        d *= 2
    return seq


def _tiling(pool, seq):
    """(pre-LDE columns [65 P][256 K], the public table [17 P][K] that belongs to them) of a drawing, by index arrays"""
    rows, pubs = pool
    n_proofs, K = seq.shape
    table = np.ascontiguousarray(rows[seq].transpose(0, 2, 1, 3)).reshape(n_proofs * W, K * 256)
    pub = np.ascontiguousarray(pubs[seq].transpose(0, 2, 1)).reshape(n_proofs * PW, K)
    return table, pub


def _holds_as_integers(table, pub, boundary):
    """set 1's 33 constraints on every row (the chain on every row but a ladder's last), and with `boundary` set 2's 32 on every ladder's
    last row against pub: nxt is the end point, the next row's acc -- the next ladder's first, the table's first behind the last -- is
    (0, live of that ladder): as integer identities, no reduction mod p"""
    assert int(table.max()) < 1 << 32
    t = table.astype(np.int64)
    last = np.arange(table.shape[1]) % 256 == 255
    for p in range(table.shape[0] // W):
        c = t[p * W:(p + 1) * W]
        bit, acc, dbl, add, nxt = c[am.BIT], c[am.ACC:am.ACC + 16], c[am.DBL:am.DBL + 16], c[am.ADD:am.ADD + 16], c[am.NXT:am.NXT + 16]
        assert not (bit * bit - bit).any() and not (nxt - dbl - bit * (add - dbl)).any()
        follow = np.roll(acc, -1, axis=1)
        assert not (follow - nxt)[:, ~last].any()
        if boundary:
            q = pub[p * PW:(p + 1) * PW].astype(np.int64)
            want = np.zeros_like(q[:16])
            want[8] = np.roll(q[16], -1)
            assert np.array_equal(nxt[:, last], q[:16]) and np.array_equal(follow[:, last], want)
            assert np.array_equal(q[16], q[:16].any(axis=0).astype(np.int64))


@pytest.mark.parametrize("set_no,K,n_proofs,log_blowup,dead", [(1, 1, 2, 2, ()), (2, 2, 2, 2, ((1, 0),)), (2, 16, 1, 1, ((0, 15),))])
def test_tilings_are_honest_tables(oracle, pool, set_no, K, n_proofs, log_blowup, dead):
    """K = 1 (set 1: one ladder, the only unselected row is seam and wrap-around at once), K = 2 with ladder 0 of one proof dead and K = 16
    with ladder K - 1 dead (set 2): the tiling satisfies every constraint as an integer identity, its model quotient interpolates to degree
    <= N - 2 in both planes, the identity holds at a zeta outside the base field (Horner on the coefficients) and fails for a bumped
    quotient value; under set 2 it also fails for one changed public word"""
    boundary = set_no == 2
    seq = _draw(np.random.default_rng(12000 + K), pool, K, n_proofs, dead=dead, live=[0] if K < 16 else [])
    table, pub = _tiling(pool, seq)
    assert (seq == -1).sum() >= len(dead) and (seq >= 0).any()
    _holds_as_integers(table, pub, boundary)
    N = table.shape[1]
    log_n = N.bit_length() - 1 + log_blowup
    ext = oracle.lde(table, log_blowup)
    g = _gamma(oracle, boundary, log_n, log_blowup, CAP_H, n_proofs, ta._cap(oracle, ext, log_n), pub)
    quot = _model(oracle, boundary, log_n, log_blowup, n_proofs, ext, pub, g)
    deg = ta._degrees(oracle, quot)
    print(f"\n[air shapes] set {set_no}, K = {K}: N = {N}, quotient degrees {deg}")
    assert -1 < max(deg) <= N - 2
    M = 1 << log_n
    zs = (ZETA, fm.e_scale(ZETA, oracle.gl_root(log_n - log_blowup)))
    ys = dm.evaluate(oracle, table, 1, zs)
    u = [am.horner(am.coefficients(oracle, quot[k * M:(k + 1) * M], _shift()), ZETA) for k in (0, 1)]
    t0, t1 = [tuple(y[0]) for y in ys], [tuple(y[1]) for y in ys]
    args = (oracle, log_n, log_blowup, n_proofs)
    if boundary:
        assert abm.identity_at(*args, t0, t1, u[0], u[1], ZETA, g, pub)
        assert not abm.identity_at(*args, t0, t1, fm.e_add(u[0], (1, 0)), u[1], ZETA, g, pub)
        bad = pub.copy()
        bad[5, K - 1] ^= np.uint64(1)
        assert not abm.identity_at(*args, t0, t1, u[0], u[1], ZETA, g, bad)
    else:
        assert am.identity_at(*args, t0, t1, u[0], u[1], ZETA, g)
        assert not am.identity_at(*args, t0, t1, fm.e_add(u[0], (1, 0)), u[1], ZETA, g)


# ---- GPU
@pytest.fixture(scope="module")
def ctx(built_lib):
    import tendermintx_amd as tmx
    c = tmx.Context(4, b"celestia")
    yield c
    c.close()


def _quotient_dev(ctx, boundary, log_n, log_blowup, n_proofs, d_cols, d_cap, d_pub=None, pieces=None, cap_height=CAP_H, onto=None):
    """the device quotient (a device tensor) between two sentinel blocks that must stay untouched.  pieces: [(lo, hi)] fed in order, the
    first overwriting and the others accumulating; onto: words the CALLER leaves in d_quot, onto which every piece accumulates"""
    import torch
    words = 2 << log_n
    buf = _sentinel(words + 2 * GUARD)
    if onto is not None:
        buf[GUARD:GUARD + words] = _up(onto)
    out = buf[GUARD:].data_ptr()

    def call(**kw):
        if boundary:
            ctx.air_ladder_boundary_quotient_device(log_n, log_blowup, cap_height, n_proofs, d_cols.data_ptr(), d_cap.data_ptr(), d_pub.data_ptr(),
                                                    out, 0, **kw)
        else:
            ctx.air_ladder_quotient_device(log_n, log_blowup, cap_height, n_proofs, d_cols.data_ptr(), d_cap.data_ptr(), out, 0, **kw)

    if pieces is None:
        call()
    else:
        for k, r in enumerate(pieces):
            call(proof_range=r, accumulate=k > 0 or onto is not None)
    torch.cuda.synchronize(_dev())
    want = _sentinel(GUARD)
    assert torch.equal(buf[:GUARD], want) and torch.equal(buf[GUARD + words:], want)
    return buf[GUARD:GUARD + words].clone()


def _quotient(*a, **kw):
    return _down(_quotient_dev(*a, **kw))


def _same(got, want, what=""):
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:10])


# A.  (set, log2 of the trace rows N, proofs, log_blowup, cap height): N = 256 (set 2: 512), where the selector index i mod 256 B is the
# whole domain; blow-up 2 and 64 (1 and 64 workgroups of the tables kernels, ZINV filled up to the first SEL word, SEL / SINV of 16 384
# entries); a Horner chain over 17 proofs; K = 16.  At blow-up 64 the cap is the root, at one of them also the whole leaf level
GEOMETRY = [(1, 8, 1, 1, CAP_H), (1, 8, 2, 6, 0), (1, 8, 2, 6, 14), (1, 9, 1, 6, 0), (1, 8, 17, 1, CAP_H), (1, 12, 1, 1, CAP_H),
            (2, 9, 1, 1, CAP_H), (2, 9, 2, 6, 0), (2, 10, 1, 6, 0), (2, 9, 17, 1, CAP_H), (2, 12, 1, 1, CAP_H)]


@pytest.mark.gpu
@pytest.mark.parametrize("set_no,log_rows,n_proofs,log_blowup,cap_height", GEOMETRY)
def test_quotient_at_every_table_geometry(ctx, oracle, set_no, log_rows, n_proofs, log_blowup, cap_height):
    """random full-degree, non-satisfying columns (set 2: and a random public table): d_quot and gamma equal the model's word for word,
    whole and, where there are two proofs or more, in two pieces fed in both orders; gamma after every call is the whole call's"""
    boundary = set_no == 2
    log_n = log_rows + log_blowup
    rng = np.random.default_rng(11000 + 1000 * set_no + 37 * log_n + n_proofs + cap_height)
    ext = ta._random_ext(rng, log_n, n_proofs)
    pub = tab._random_pub(rng, n_proofs, 1 << (log_rows - 8)) if boundary else None
    d_cols, d_pub = _up(ext), _up(pub) if boundary else None
    _, d_cap = ta._tree(ctx, d_cols, log_n, n_proofs * W, cap_height)
    assert d_cap.numel() == 4 << min(cap_height, log_n)
    args = (ctx, boundary, log_n, log_blowup, n_proofs, d_cols, d_cap, d_pub)
    got = _quotient(*args, cap_height=cap_height)
    g = _gamma(oracle, boundary, log_n, log_blowup, cap_height, n_proofs, _down(d_cap), pub)
    assert ctx.air_last_gamma() == g
    want = _model(oracle, boundary, log_n, log_blowup, n_proofs, ext, pub, g)
    _same(got, want, "whole")
    if n_proofs > 1:
        cut = max(1, n_proofs // 3)
        for pieces in ([(0, cut), (cut, n_proofs)], [(cut, n_proofs), (0, cut)]):
            _same(_quotient(*args, pieces=pieces, cap_height=cap_height), want, pieces)
            assert ctx.air_last_gamma() == g


# B.
@pytest.mark.gpu
@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("set_no", [1, 2])
def test_quotient_of_extreme_words_equals_the_model(ctx, oracle, set_no, fill):
    """columns (set 2: and a public table) of all p - 1, all 2^64 - 1, random words in [p, 2^64) and random edge words, two proofs at
    N = 256 (set 2: 512) and blow-up 8: gl_canon on every load, the lazy sums a0 / b0 / w0 at their largest and gl_mul(sel, b0) on a
    non-canonical b0.  Whole and as [0, 1) then [1, 2)"""
    boundary = set_no == 2
    log_rows, n_proofs, lb = 9 if boundary else 8, 2, 3
    log_n = log_rows + lb
    rng = np.random.default_rng(11200 + set_no)
    ext = FILLS[fill](rng, (n_proofs * W, 1 << log_n))
    pub = FILLS[fill](rng, (n_proofs * PW, 1 << (log_rows - 8))) if boundary else None
    assert ext.dtype == np.uint64 and (fill == "edge words" or int(ext.min()) >= P - 1)
    d_cols, d_pub = _up(ext), _up(pub) if boundary else None
    _, d_cap = ta._tree(ctx, d_cols, log_n, n_proofs * W)
    args = (ctx, boundary, log_n, lb, n_proofs, d_cols, d_cap, d_pub)
    got = _quotient(*args)
    g = _gamma(oracle, boundary, log_n, lb, CAP_H, n_proofs, _down(d_cap), pub)
    assert ctx.air_last_gamma() == g
    want = _model(oracle, boundary, log_n, lb, n_proofs, ext, pub, g)
    _same(got, want, "whole")
    _same(_quotient(*args, pieces=[(0, 1), (1, 2)]), want, "pieces")


# C.
@pytest.mark.gpu
@pytest.mark.parametrize("set_no", [1, 2])
def test_accumulating_onto_the_callers_words(ctx, oracle, set_no):
    """the single piece [0, 3) with accumulate = 1 onto a d_quot the caller filled with 0, 1, p - 1, p, p + 1, 2^64 - 1, 2^32 - 1, 2^32,
    2^63, cycled: the output is (the caller's words mod p) + the model's quotient, every word canonical"""
    boundary = set_no == 2
    log_rows, n_proofs, lb = 9 if boundary else 8, 3, 1
    log_n = log_rows + lb
    rng = np.random.default_rng(11300 + set_no)
    ext = ta._random_ext(rng, log_n, n_proofs)
    pub = tab._random_pub(rng, n_proofs, 1 << (log_rows - 8)) if boundary else None
    d_cols, d_pub = _up(ext), _up(pub) if boundary else None
    _, d_cap = ta._tree(ctx, d_cols, log_n, n_proofs * W)
    onto = np.resize(EDGE_WORDS, 2 << log_n)
    got = _quotient(ctx, boundary, log_n, lb, n_proofs, d_cols, d_cap, d_pub, pieces=[(0, n_proofs)], onto=onto)
    g = _gamma(oracle, boundary, log_n, lb, CAP_H, n_proofs, _down(d_cap), pub)
    assert ctx.air_last_gamma() == g
    model = _model(oracle, boundary, log_n, lb, n_proofs, ext, pub, g)
    want = np.array([(int(a) % P + int(b)) % P for a, b in zip(onto, model)], dtype=np.uint64)
    assert int(got.max()) < P
    _same(got, want)
    assert not np.array_equal(got, model)


# D.
MANY = 259


@pytest.mark.gpu
@pytest.mark.parametrize("set_no", [1, 2])
def test_pieces_that_start_at_proof_256_and_above(ctx, oracle, set_no):
    """259 proofs at N = 256 (set 2: 512) and blow-up 2, 16 835 columns: [0, 256) + [256, 258) + [258, 259) ascending and descending equal
    the whole call word for word (the piece weights gamma^(33 first), gamma^(65 first) with first = 256 and 258; a Horner chain over 259
    proofs); [256, 259) and [258, 259) alone equal the model's pieces, under set 2 the model's pieces of an all-zero public table: a piece
    without proof 0 carries no Pub_gamma term"""
    boundary = set_no == 2
    log_rows, lb = 9 if boundary else 8, 1
    log_n = log_rows + lb
    rng = np.random.default_rng(11400 + set_no)
    ext = ta._random_ext(rng, log_n, MANY)
    pub = tab._random_pub(rng, MANY, 1 << (log_rows - 8)) if boundary else None
    d_cols, d_pub = _up(ext), _up(pub) if boundary else None
    _, d_cap = ta._tree(ctx, d_cols, log_n, MANY * W)
    args = (ctx, boundary, log_n, lb, MANY, d_cols, d_cap, d_pub)
    whole = _quotient(*args)
    g = _gamma(oracle, boundary, log_n, lb, CAP_H, MANY, _down(d_cap), pub)
    assert ctx.air_last_gamma() == g
    pieces = [(0, 256), (256, 258), (258, MANY)]
    for order in (pieces, pieces[::-1]):
        _same(_quotient(*args, pieces=order), whole, order)
        assert ctx.air_last_gamma() == g
    none = np.zeros_like(pub) if boundary else None
    for lo in (256, 258):
        want = _model(oracle, boundary, log_n, lb, MANY, ext, none, g, proofs=range(lo, MANY))
        _same(_quotient(*args, pieces=[(lo, MANY)]), want, lo)
    # the three model pieces behind proof 256 are what the whole call adds to the first piece
    first = _quotient(*args, pieces=[(0, 256)])
    tail = _model(oracle, boundary, log_n, lb, MANY, ext, none, g, proofs=range(256, MANY))
    _same(whole, np.array([(int(a) + int(b)) % P for a, b in zip(first, tail)], dtype=np.uint64), "first + tail")


# E.  (log2 of the trace rows, proofs, log_blowup): K = 16, 64, 128 (threads of the one-workgroup transform without an element), 512 (two
# trips of the j += 256 loops, half = 256), 1024 (log_a = 2) and 2048 (log_a = 1)
PUBLIC_SHAPES = [(12, 3, 1), (14, 1, 2), (15, 1, 1), (17, 2, 1), (18, 1, 1), (19, 1, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs,log_blowup", PUBLIC_SHAPES)
def test_public_side_at_every_k_regime(ctx, oracle, log_rows, n_proofs, log_blowup):
    """test_air_boundary.py's construction: the quotient of all-zero columns is - Pub_gamma(x_i) / S(x_i) exactly, so every word of
    k_air_public_combine / _coefs / _extend is seen through it.  The random public table has a third of its words in [p, 2^64), live
    flags 0 at ladders 0 and K - 1 in the first proof and 1 there in the last (the (k + 1) mod K wrap); with one proof the two ladders get
    0 and 1"""
    import torch
    log_n, K = log_rows + log_blowup, 1 << (log_rows - 8)
    rng = np.random.default_rng(11500 + log_rows)
    pub = tab._random_pub(rng, n_proofs, K)
    high = rng.random(pub.shape) < 1 / 3
    pub[high] = rng.integers(P, 1 << 64, int(high.sum()), dtype=np.uint64)
    pub[16, 0], pub[16, K - 1] = 0, 0 if n_proofs > 1 else 1
    pub[PW * (n_proofs - 1) + 16, K - 1] = 1
    if n_proofs > 1:
        pub[PW * (n_proofs - 1) + 16, 0] = 1
    assert int(pub.max()) >= P
    d_cols = torch.zeros(((n_proofs * W) << log_n,), dtype=torch.int64, device=_dev())
    d_cap, d_pub = _up(rng.integers(0, P, 4 << CAP_H, dtype=np.uint64)), _up(pub)
    got = _quotient(ctx, True, log_n, log_blowup, n_proofs, d_cols, d_cap, d_pub)
    del d_cols
    g = abm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _down(d_cap), pub)
    assert ctx.air_last_gamma() == g
    M, B = 1 << log_n, 1 << log_blowup
    ext = abm.pub_on_coset(oracle, log_n, abm.pub_coefficients(oracle, log_n, log_blowup, abm.combine(pub, g)), _shift())
    w, om, x = oracle.gl_root(log_n), am.omega_256_inv(oracle, log_n), _shift() % P
    sinv = []
    for _ in range(256 * B):
        sinv.append(pow((pow(x, K, P) - om) % P, P - 2, P))
        x = x * w % P
    sinv = np.array(sinv * (M // (256 * B)), dtype=object)
    for k in (0, 1):
        want = (P - ext[k].astype(object) % P * sinv % P) % P
        have = got[k * M:(k + 1) * M].astype(object)
        assert np.array_equal(have, want), (k, np.flatnonzero(have != want)[:10])


# F.  (kind, N, proofs): K = 2; ten ladders in K = 16 and six padding ladders; one full workgroup per proof; 516 lanes
GATHER = [(1, 1, 3), (0, 5, 2), (0, 128, 3), (1, 2, 129)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,n_proofs", GATHER)
def test_gather_of_crafted_rows_equals_the_model(built_lib, kind, n, n_proofs):
    """element rows of random 64-bit words, a third of them in [p, 2^64), with four planted end points: sixteen words 0 (live 0), sixteen
    words p (they reduce to 0: live 0), all p but one word 1 and all 0 but one word p + 1 (live 1).  The device's table equals the model's
    table of the same rows reduced mod p, guard words intact, and it does not change when every word outside D.1b's span changes: all the
    kernel reads lies inside [d1b_start, d1b_start + 99 N) of a row"""
    import tendermintx_amd as tmx
    with tmx.Context(n, tab.CID, max_batch=n_proofs) as c:
        stride, start = c.elem_stride(kind), abm.d1b_start(kind, n)
        log_k, n_cols = c.air_ladder_public_shape(kind, n_proofs)
        assert start + 99 * n <= stride and 2 * n <= 1 << log_k and n_cols == PW * n_proofs
        rng = np.random.default_rng(11600 + n)
        rows = rng.integers(0, 1 << 64, (n_proofs, stride), dtype=np.uint64)
        high = rng.random(rows.shape) < 1 / 3
        rows[high] = rng.integers(P, 1 << 64, int(high.sum()), dtype=np.uint64)
        slots = [(p, k) for p in range(n_proofs) for k in range(2 * n)]
        planted = [slots[0], slots[len(slots) // 3], slots[2 * len(slots) // 3], slots[-1]]
        assert len(set(planted)) == 4
        at = lambda k: start + 99 * (k >> 1) + 40 + 16 * (k & 1)
        for (p, k), words in zip(planted, ([0] * 16, [P] * 16, [P] * 11 + [1] + [P] * 4, [0] * 3 + [P + 1] + [0] * 12)):
            rows[p, at(k):at(k) + 16] = np.array(words, dtype=np.uint64)
        _, got = tab._gather(c, kind, n_proofs, _up(rows))
        want = abm.public_table(kind, n, list(rows % np.uint64(P)), log_k)
        assert got.shape == want.shape == (n_cols, 1 << log_k)
        _same(got.reshape(-1), want.reshape(-1))
        assert int(got.max()) < P and not got[:, 2 * n:].any()
        assert [int(got[PW * p + 16, k]) for p, k in planted] == [0, 0, 1, 1]
        assert not got[PW * planted[1][0]:PW * planted[1][0] + 17, planted[1][1]].any()
        assert int(got[PW * planted[3][0]:PW * planted[3][0] + 16, planted[3][1]].sum()) == 1
        assert got[16::PW, :2 * n].sum() == 2 * n * n_proofs - 2
        outside = np.ones(stride, dtype=bool)
        outside[start:start + 99 * n] = False
        assert outside[start - 1] and outside[start + 99 * n:].all()
        other = rows.copy()
        other[:, outside] ^= np.uint64(0x5555555555555555)
        _, again = tab._gather(c, kind, n_proofs, _up(other))
        _same(again.reshape(-1), got.reshape(-1), "words outside D.1b")


# G.  the verifiers on honest tilings
def _chain(ctx, boundary, table, pub, log_blowup, n_queries, front=None):
    """the caller-level chain of test_air.py's _e2e on the device alone: LDE, trees, the quotient of set 1 or 2, one batch proof over
    [(front,) trace, quotient].  Returns (params, d_caps, proof words, gamma, d_ext, d_quot); front: extended columns of an unrelated oracle"""
    import torch
    n_cols, log_rows = table.shape[0], table.shape[1].bit_length() - 1
    log_n, n_proofs = log_rows + log_blowup, table.shape[0] // W
    d_ext, d_table = _sentinel(n_cols << log_n), _up(table)
    ctx.lde_device(log_rows, log_blowup, n_cols, d_table.data_ptr(), d_ext.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    del d_table
    d_lv_t, d_cap_t = ta._tree(ctx, d_ext, log_n, n_cols)
    d_quot = _quotient_dev(ctx, boundary, log_n, log_blowup, n_proofs, d_ext, d_cap_t, _up(pub) if boundary else None)
    gamma = ctx.air_last_gamma()
    d_lv_q, d_cap_q = ta._tree(ctx, d_quot, log_n, 2)
    cols, levels, caps, sizes, widths = [d_ext, d_quot], [d_lv_t, d_lv_q], [d_cap_t, d_cap_q], [log_n, log_n], [n_cols, 2]
    if front is not None:
        d_front, log_f = _up(front), front.shape[1].bit_length() - 1
        d_lv_f, d_cap_f = ta._tree(ctx, d_front, log_f, front.shape[0])
        cols, levels, caps, sizes, widths = [d_front] + cols, [d_lv_f] + levels, [d_cap_f] + caps, [log_f] + sizes, [front.shape[0]] + widths
    p = bparams(sizes, widths, CAP_H, log_blowup, E2E["arity_bits"], E2E["final_log_max"], n_queries)
    words = bm.layout(p)["words"]
    buf = _sentinel(words + 2 * GUARD)
    ctx.batch_prove_device(p, [c.data_ptr() for c in cols], [l.data_ptr() for l in levels], buf[GUARD:].data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(buf[:GUARD], _sentinel(GUARD)) and torch.equal(buf[GUARD + words:], _sentinel(GUARD))
    assert ctx.fri_last_degree_ok() is True
    return p, torch.cat(caps), _down(buf[GUARD:GUARD + words].clone()), gamma, d_ext, d_quot


def _verdicts(ctx, boundary, p, k_trace, d_caps, proof, pub):
    return tab._verdicts(ctx, p, k_trace, d_caps, proof, pub) if boundary else ta._verdicts(ctx, p, k_trace, d_caps, proof)


def _bumped(proof, at):
    bad = proof.copy()
    bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("set_no", [1, 2])
def test_one_proof_at_log_sub_8_and_9(ctx, oracle, pool, set_no):
    """set 1 at N = 256 (zero squarings of zeta, one ladder: the only unselected row is seam and wrap-around at once) and set 2 at N = 512
    (one squaring, K = 2, the second ladder dead), one proof: the device quotient and gamma equal the model's, the quotient has degree
    <= N - 2, every verdict equals the model verifier's (all accept), and a bumped trace opening at zeta, at zeta omega and a bumped
    quotient opening are rejected verdict for verdict"""
    boundary = set_no == 2
    K = 2 if boundary else 1
    seq = _draw(np.random.default_rng(12200 + K), pool, K, 1, dead=((0, 1),) if boundary else (), live=[0])
    table, pub = _tiling(pool, seq)
    lb = E2E["log_blowup"]
    p, d_caps, got, gamma, d_ext, d_quot = _chain(ctx, boundary, table, pub, lb, E2E["n_queries"])
    log_n, caps, N = p["log_n"][0], _down(d_caps), table.shape[1]
    assert log_n - lb == 7 + set_no
    ext = oracle.lde(table, lb)
    _same(_down(d_ext), ext.reshape(-1), "lde")
    assert gamma == _gamma(oracle, boundary, log_n, lb, CAP_H, 1, caps[:4 << CAP_H], pub)
    quot = _down(d_quot)
    _same(quot, _model(oracle, boundary, log_n, lb, 1, ext, pub, gamma), "quotient")
    assert -1 < max(ta._degrees(oracle, quot)) <= N - 2
    model = _model_verdicts(oracle, boundary, p, 0, caps, got, pub)
    assert all(model) and _verdicts(ctx, boundary, p, 0, d_caps, got, pub) == model
    L, R = bm.layout(p), 1 << dm.log_r(p["n_cols"][0])
    for name, at in (("nxt at zeta", L["off_open"][0] + am.NXT + 2), ("acc at zeta omega", L["off_open"][0] + 2 * R + am.ACC + 8),
                     ("quotient", L["off_open"][1] + 1)):
        bad = _bumped(got, at)
        model = _model_verdicts(oracle, boundary, p, 0, caps, bad, pub)
        assert not any(model), name
        assert _verdicts(ctx, boundary, p, 0, d_caps, bad, pub) == model, name


CROWD = 257  # one proof more than the check kernels have threads: thread 0 takes proofs 0 and 256


def _crowd(ctx, oracle, pool, boundary):
    """the chain with 257 proofs at N = 256 (set 2: 512), blow-up 2, two queries.  The proofs whose openings the tests change hold no dead
    ladder, so none of them drops out of the sum by being zero"""
    K = 2 if boundary else 1
    seq = _draw(np.random.default_rng(12300 + K), pool, K, CROWD, live=[0, 1, 200, 255, 256])
    assert (seq == -1).any() and len(np.unique(seq)) >= 13
    table, pub = _tiling(pool, seq)
    p, d_caps, got, gamma, _, _ = _chain(ctx, boundary, table, pub, 1, 2)
    caps = _down(d_caps)
    assert gamma == _gamma(oracle, boundary, p["log_n"][0], 1, CAP_H, CROWD, caps[:4 << CAP_H], pub)
    return p, d_caps, caps, got, pub


@pytest.fixture(scope="module")
def crowd1(ctx, oracle, pool):
    return _crowd(ctx, oracle, pool, False)


@pytest.fixture(scope="module")
def crowd2(ctx, oracle, pool):
    return _crowd(ctx, oracle, pool, True)


@pytest.mark.gpu
@pytest.mark.parametrize("set_no", [1, 2])
def test_257_proofs_are_accepted(request, ctx, oracle, set_no):
    """every thread of the check kernel contributes to the LDS reduction and thread 0's proof loop takes a second trip: the device accepts
    every query, as the model verifier does"""
    p, d_caps, caps, got, pub = request.getfixturevalue(f"crowd{set_no}")
    assert p["n_cols"] == [CROWD * W, 2] and p["log_n"] == [8 + set_no] * 2
    model = _model_verdicts(oracle, set_no == 2, p, 0, caps, got, pub)
    assert all(model) and _verdicts(ctx, set_no == 2, p, 0, d_caps, got, pub) == model


@pytest.mark.gpu
@pytest.mark.parametrize("proof_no", [0, 1, 200, 255, 256])
@pytest.mark.parametrize("set_no", [1, 2])
def test_257_proofs_with_one_changed_opening_are_rejected(request, ctx, oracle, set_no, proof_no):
    """one trace opening at zeta bumped in proof 0, 1, 200, 255 or 256 (the last one thread 0's second trip): rejected on every query by
    the device and by the model (a reduction step that drops a thread, a wrong gamma^(33 p) / gamma^(65 p) or a proof loop that stops after
    one trip would keep some of them accepted)"""
    p, d_caps, caps, got, pub = request.getfixturevalue(f"crowd{set_no}")
    bad = _bumped(got, bm.layout(p)["off_open"][0] + proof_no * W + am.NXT + 2)
    model = _model_verdicts(oracle, set_no == 2, p, 0, caps, bad, pub)
    assert not any(model)
    assert _verdicts(ctx, set_no == 2, p, 0, d_caps, bad, pub) == model


@pytest.mark.gpu
def test_257_proofs_with_a_changed_public_word_are_rejected(ctx, oracle, crowd2):
    """set 2: one end word, then the live flag, of proof 256 changed in the verifier's public table: every query rejected by both"""
    p, d_caps, caps, got, pub = crowd2
    for row in (3, 16):
        bad = pub.copy()
        bad[PW * 256 + row, 1] ^= np.uint64(1)
        assert not abm.identity(oracle, p, 0, caps, got, bad), row
        assert not any(_verdicts(ctx, True, p, 0, d_caps, got, bad)), row


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,dead", [(17, 0), (20, -1)])
def test_set_2_verifier_at_k_512_and_4096(ctx, oracle, pool, log_rows, dead):
    """K = 512 and K = 4096 (one proof, blow-up 2, two queries): the barycentric block of k_air_ladder_boundary_check with 2 and with all
    16 slots per thread occupied -- pre[m], the back-substitution across slots, y *= stride -- on an honest tiling that repeats with no
    period dividing 256, ladder 0 dead at K = 512 and ladder K - 1 dead at K = 4096.  The device accepts every query, as the model's
    identity (gamma, the barycentric Pub_gamma(zeta)) and batch_model's verifier do; one changed end word at a ladder k >= K - 256 and
    one flipped live flag there are rejected by the device and the model's identity.  (The table is built with index arrays, not per
    row; the quotient's words are compared with the model at the sizes of the tests above.)"""
    t0 = time.perf_counter()
    K = 1 << (log_rows - 8)
    seq = _draw(np.random.default_rng(12400 + log_rows), pool, K, 1, dead=((0, dead % K),))
    assert len(np.unique(seq[0, K - 256:])) >= 13
    table, pub = _tiling(pool, seq)
    p, d_caps, got, gamma, d_ext, d_quot = _chain(ctx, True, table, pub, 1, 2)
    del table, d_ext, d_quot
    caps = _down(d_caps)
    assert gamma == abm.gamma(oracle, log_rows + 1, 1, CAP_H, 1, caps[:4 << CAP_H], pub)
    assert abm.identity(oracle, p, 0, caps, got, pub) and all(bm.verify(oracle, p, caps, got, _shift()))
    assert all(_verdicts(ctx, True, p, 0, d_caps, got, pub))
    for name, row, k in (("end word", 11, K - 251), ("live flag", 16, K - 2)):
        bad = pub.copy()
        bad[row, k] ^= np.uint64(1)
        assert not abm.identity(oracle, p, 0, caps, got, bad), name
        assert not any(_verdicts(ctx, True, p, 0, d_caps, got, bad)), name
    print(f"\n[air shapes] set 2 at K = {K}: {time.perf_counter() - t0:.1f} s")


@pytest.mark.gpu
def test_set_1_verifier_after_nine_squarings(ctx, oracle, pool):
    """set 1 at N = 2^17 (k_air_ladder_check squares zeta nine times before S(zeta)), one proof, blow-up 2, two queries: accepted by the
    device and the model verifier; a bumped acc opening at zeta omega is rejected by both"""
    seq = _draw(np.random.default_rng(12500), pool, 512, 1)
    table, pub = _tiling(pool, seq)
    p, d_caps, got, gamma, d_ext, d_quot = _chain(ctx, False, table, None, 1, 2)
    del table, d_ext, d_quot
    caps = _down(d_caps)
    assert gamma == am.gamma(oracle, 18, 1, CAP_H, 1, caps[:4 << CAP_H])
    model = _model_verdicts(oracle, False, p, 0, caps, got, None)
    assert all(model) and _verdicts(ctx, False, p, 0, d_caps, got, None) == model
    R = 1 << dm.log_r(W)
    bad = _bumped(got, bm.layout(p)["off_open"][0] + 2 * R + am.ACC + 3)
    model = _model_verdicts(oracle, False, p, 0, caps, bad, None)
    assert not any(model) and _verdicts(ctx, False, p, 0, d_caps, bad, None) == model


@pytest.mark.gpu
@pytest.mark.parametrize("set_no", [1, 2])
def test_the_ladders_behind_another_oracle(ctx, oracle, pool, set_no):
    """k_trace = 1: a low-degree random oracle of 3 columns and log_n + 1 in front of [ladders, quotient] (two proofs, K = 2), so that
    L.off_open[1], G.o_cap_at[1] and G.o_log_r[1] (log_r 8 behind an oracle of log_r 2) are what the verifier must read.  The verdicts
    equal the model's with k_trace = 1 (all accept), a bumped trace opening is rejected by both, and k_trace = 0 on the same proof is
    refused by both verifiers with nothing written"""
    import torch
    boundary = set_no == 2
    seq = _draw(np.random.default_rng(12600 + set_no), pool, 2, 2, dead=((1, 1),), live=[0])
    table, pub = _tiling(pool, seq)
    lb = E2E["log_blowup"]
    front = oracle.lde(np.random.default_rng(12700).integers(0, P, (3, 2 * table.shape[1]), dtype=np.uint64), lb)
    p, d_caps, got, gamma, _, _ = _chain(ctx, boundary, table, pub, lb, E2E["n_queries"], front=front)
    assert p["log_n"] == [12, 11, 11] and p["n_cols"] == [3, 2 * W, 2]
    assert dm.log_r(3) == 2 and dm.log_r(2 * W) == 8
    caps = _down(d_caps)
    model = _model_verdicts(oracle, boundary, p, 1, caps, got, pub)
    assert all(model) and _verdicts(ctx, boundary, p, 1, d_caps, got, pub) == model
    bad = _bumped(got, bm.layout(p)["off_open"][1] + W + am.NXT + 2)
    model = _model_verdicts(oracle, boundary, p, 1, caps, bad, pub)
    assert not any(model) and _verdicts(ctx, boundary, p, 1, d_caps, bad, pub) == model
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    d_got, d_pub = _up(got), _up(pub)
    _refused(lambda: ctx.air_verify_device(p, 0, d_caps.data_ptr(), d_got.data_ptr(), ok.data_ptr(), 0), ok)
    _refused(lambda: ctx.air_boundary_verify_device(p, 0, d_caps.data_ptr(), d_got.data_ptr(), d_pub.data_ptr(), ok.data_ptr(), 0), ok)
