"""The SHA-512 table's link to Level-1 (include/tmx.h "the SHA-512 table's link to Level-1", constraint set 10):
tmx_air_sha512_public_shape, tmx_air_sha512_public_device, tmx_air_sha512_link_helper_device, tmx_air_sha512_link_quotient_device /
_range_device, tmx_air_sha512_link_verify_device, tmx_trace_commit_set_air_sha512_link_device and the calls that show the planes and the
public side on their own.  The yardstick is tests/sha512_link_model.py on top of tests/batch_model.py: device words must equal the model's
word for word and every verdict of the device verifier must equal the model verifier's.  The CPU part ties the model to the claim: the public table
is built from the ELEMENT rows only (Level 1: H.2 and the digest of D.1a) and equals, for every block of T.2, what the trace rows say -- the
sixteen message words, CV plus the last-round state written out with plain integers, the liveness pattern -- and hashlib.sha512 of the
reassembled messages; all 115 constraints hold on those rows as integer identities, the model quotient is a polynomial of degree N - 2, and
the two changes constraint sets 7 + 8 + 9 accept (tests/test_sha512_init.py records them) break it.  The fixtures are those of
tests/test_sha512_air.py (the same workloads and seeds) with the oracle's element rows beside them, and a batch with a lane that did not
sign."""
import hashlib

import numpy as np
import pytest

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha512_link_model as lm
import test_sha512_init as t9
from batch_model import bparams
from test_fri import _down, _sentinel, _shift, _up
from test_sha512_air import _columns, _word
from test_sha_air import GUARD, _cap, _degrees, _dev, _guarded, _random_ext, _refused, _tree

P = lm.P
W, PW, HC = lm.WIDTH, lm.PUB_WIDTH, lm.HELPER_COLS
IV512, M64, M32 = lm.IV512, lm.M64, lm.M32
CID, SKIP_MAX = b"celestia", 100800
CAP_H, LB = 2, 2  # blow-up 4 in the CPU tests
SHA512, SHA256, HEADER, H9, Q9, HELPER, QUOTIENT = 2, 4, 32, 524288, 1048576, 2097152, 4194304
FLAGS, SIGNED = 223, 1  # the flags byte of a 256-byte validator record and its `signed` bit
LENGTHS = [0, 47, 48, 63, 64, 124, 200]  # message lengths at which the block count, the 80 byte and the length field move; 200 is clamped


def _workload(kind, n, n_proofs, seed, unsign=()):
    """a synthetic batch; unsign: (proof, lane) pairs whose `signed` flag is cleared afterwards, key, signature and message left in place"""
    from tendermintx_amd.synth import Workload
    wl = Workload(kind, n, n_proofs, n, chain_id=CID, seed=seed, signed_permille=900)
    targets = bytearray(wl.targets)
    for p, i in unsign:
        at = (p * n + i) * 256 + FLAGS
        assert targets[at] & SIGNED  # (the lane signed: clearing the flag leaves a real triple in a lane that is hashed on the dummy one)
        targets[at] &= ~SIGNED & 0xFF
    return wl.proofs, bytes(targets), wl.trusteds if kind == 0 else b""


def _fixture(oracle, kind, n, n_proofs, seed, unsign=()):
    """(kind, n, T.2 pre-LDE columns [18 n_proofs][N], element rows, the model's public table)"""
    proofs, targets, trusteds = _workload(kind, n, n_proofs, seed, unsign)
    fulls, elems = [], []
    for p in range(n_proofs):
        pr, t = proofs[p * 2336:(p + 1) * 2336], targets[p * n * 256:(p + 1) * n * 256]
        r = trusteds[p * n * 48:(p + 1) * n * 48] if kind == 0 else None
        fulls.append(oracle.trace(kind, pr, t, r, n))
        elems.append(oracle.witness(kind, pr, t, r, CID, SKIP_MAX)[0])
    table = _columns(fulls, kind, n)
    return kind, n, table, elems, lm.public_table(kind, n, elems, lm.log_k(table.shape[1].bit_length() - 1), oracle.dummy())


@pytest.fixture(scope="module")
def skip4(oracle):
    return _fixture(oracle, 0, 4, 2, 8100)


@pytest.fixture(scope="module")
def step2(oracle):
    return _fixture(oracle, 1, 2, 2, 8200)


@pytest.fixture(scope="module")
def step3(oracle):
    return _fixture(oracle, 1, 3, 2, 8300)


@pytest.fixture(scope="module")
def unsigned3(oracle):
    """step N = 3 with lane 1 of proof 0 and lane 2 of proof 1 not signing: a live first block in front of a zero second block"""
    return _fixture(oracle, 1, 3, 2, 8300, unsign=((0, 1), (1, 2)))


def _cases(skip4, step2, step3, unsigned3):
    return (("skip4", skip4), ("step2", step2), ("step3", step3), ("unsigned3", unsigned3))


# ---- CPU: the model against the claim
def test_public_table_from_the_element_rows_is_what_the_rows_hash(oracle, skip4, step2, step3, unsigned3):
    """the link itself.  For every block slot of T.2 of skip N = 4, step N = 2, step N = 3 and the batch with lanes that did not sign, two
    proofs each, the table gathered from the ELEMENT rows holds: w[k][t] = the table's W at row 80 k + t (the partial last slot included); lv
    = the liveness of the rows; dig = CV + the last-round state of the lane's last live block, plain integers (CV the IV, or the IV plus the
    first block's last-round state); and every digest equals hashlib.sha512 of the reassembled message"""
    two_blocks = one_block = n_unsigned = 0
    for name, (kind, n, table, elems, pub) in _cases(skip4, step2, step3, unsigned3):
        N = table.shape[1]
        slots, K = -(-N // 80), pub.shape[1]
        assert pub.shape == (PW * len(elems), K) and K >= slots > 2 * n and int(pub.max()) < 1 << 32 and N % 80
        for p, row in enumerate(elems):
            t, u = table[p * W:(p + 1) * W], pub[p * PW:(p + 1) * PW]
            assert not u[:, slots:].any()
            for k in range(slots):
                rows = min(80, N - 80 * k)
                for l in (0, 1):
                    want = [int(x) for x in t[lm.W_ + l, 80 * k:80 * k + min(16, rows)]]
                    assert [int(x) for x in u[lm.PW_W + l:lm.PW_W + 32:2, k]][:len(want)] == want, (name, p, k, l)
                assert int(u[lm.PW_LV, k]) == int(t[:, 80 * k].any()), (name, p, k)
            msgs = lm.messages(n, row, oracle.dummy())
            for i, m in enumerate(msgs):
                signed = int(row[lm.H2 + lm.H2_LANE * i + lm.H2_SIGNED])
                n_unsigned += 1 - signed
                n_blocks = len(lm.pad(m)) // 128
                assert (int(u[lm.PW_LV, 2 * i]), int(u[lm.PW_LV, 2 * i + 1])) == (1, n_blocks - 1) and (signed or n_blocks == 1)
                one_block, two_blocks = one_block + (n_blocks == 1), two_blocks + (n_blocks == 2)
                state = lambda r: [_word(t, c, r) for c in range(lm.A_, W, 2)]
                cv = list(IV512)
                if n_blocks == 2:
                    cv = [(a + b) & M64 for a, b in zip(cv, state(160 * i + 79))]
                digest = [(a + b) & M64 for a, b in zip(cv, state(160 * i + 80 * n_blocks - 1))]
                last = 2 * i + n_blocks - 1
                got = [int(u[lm.PW_DIG + 2 * j, last]) | int(u[lm.PW_DIG + 2 * j + 1, last]) << 32 for j in range(8)]
                assert got == digest, (name, p, i)
                assert b"".join(x.to_bytes(8, "big") for x in got) == hashlib.sha512(m).digest(), (name, p, i)
                if n_blocks == 2:
                    assert not u[lm.PW_DIG:lm.PW_DIG + 16, 2 * i].any()
                else:
                    assert not u[:, 2 * i + 1].any()
    print(f"\n[sha512-link] lanes of two blocks {two_blocks}, of one block {one_block}, lanes that did not sign {n_unsigned}")
    assert two_blocks and one_block and n_unsigned >= 2


def _synthetic_rows(kind, n, stride, lengths, seed=12000):
    """element rows that hold nothing but what the gather reads: per proof lane i signs a random message of lengths[p][i] bytes (all 124
    message bytes are random: those behind the length must not count) under a random key and R, and D.1a holds hashlib's digest of
    R | A | M[: min(length, 124)]"""
    import sha_public_model as sp
    rng = np.random.default_rng(seed)
    rows = np.zeros((len(lengths), stride), dtype=np.uint64)
    bits = lambda data: [(b >> (7 - k)) & 1 for b in data for k in range(8)]
    for p, per_lane in enumerate(lengths):
        for i, length in enumerate(per_lane):
            pk, r, msg = (bytes(rng.integers(0, 256, c, dtype=np.uint8)) for c in (32, 32, 124))
            v = lm.H2 + lm.H2_LANE * i
            rows[p, v + lm.H2_PK:v + lm.H2_PK + 256] = bits(pk)
            rows[p, v + lm.H2_R:v + lm.H2_R + 256] = bits(r)
            rows[p, v + lm.H2_MSG:v + lm.H2_MSG + 992] = bits(msg)
            rows[p, v + lm.H2_MLEN], rows[p, v + lm.H2_SIGNED] = length, 1
            d = sp.Layout(kind, n).d1a + lm.D1A_LANE * i + lm.D1A_DIGEST
            rows[p, d:d + 512] = bits(hashlib.sha512(r + pk + msg[:min(length, 124)]).digest())
    return rows


def _check_padding(pub, rows, n, dummy):
    """the statement of the padding test on a public table of _synthetic_rows"""
    for p, row in enumerate(rows):
        u = pub[p * PW:(p + 1) * PW]
        for i in range(n):
            length = min(int(row[lm.H2 + lm.H2_LANE * i + lm.H2_MLEN]), 124)
            m = lm.lane_message(row, i, dummy)
            assert len(m) == 64 + length
            n_blocks = 2 if length >= 48 else 1
            got = b"".join((int(u[lm.PW_W + 2 * t + 1, k]) << 32 | int(u[lm.PW_W + 2 * t, k])).to_bytes(8, "big")
                           for k in range(2 * i, 2 * i + n_blocks) for t in range(16))
            assert got[:len(m)] == m and got[len(m)] == 0x80 and not any(got[len(m) + 1:-2]), (p, i, length)
            assert int.from_bytes(got[-16:], "big") == 8 * len(m)
            assert [int(x) for x in u[lm.PW_LV, 2 * i:2 * i + 2]] == [1, n_blocks - 1] and (n_blocks == 2 or not u[:, 2 * i + 1].any())
            # the words are a real SHA-512 input: compressing them from the IV gives the digest the row carries
            t, digest = t9._hash_lane(m)
            assert digest == hashlib.sha512(m).digest()
            for k in range(n_blocks):
                assert [int(x) for x in u[lm.PW_W:lm.PW_W + 32:2, 2 * i + k]] == [int(x) for x in t[lm.W_, 80 * k:80 * k + 16]]
            last = 2 * i + n_blocks - 1
            assert b"".join((int(u[lm.PW_DIG + 2 * j + 1, last]) << 32 | int(u[lm.PW_DIG + 2 * j, last])).to_bytes(8, "big") for j in range(8)) == digest


PAD_N = 4  # lanes per proof in the padding test: two proofs hold the seven lengths and one more


def test_padding_at_the_lengths_where_it_moves(oracle):
    """message lengths 0, 47, 48, 63, 64, 124 and 200 (clamped to 124) on rows that hold nothing else: 47 is the last length of one block;
    at 63 the 80 byte is the last byte of block 0 and at 64 the first of block 1; the 128-bit length closes the last block; the bytes of
    message[124] behind the length do not count"""
    import sha_public_model as sp
    lengths = [LENGTHS[:PAD_N], LENGTHS[PAD_N:] + [31]]
    rows = _synthetic_rows(1, PAD_N, sp.Layout(1, PAD_N).d + 2000 * PAD_N, lengths)
    pub = lm.public_table(1, PAD_N, list(rows), lm.log_k(10), oracle.dummy())
    _check_padding(pub, rows, PAD_N, oracle.dummy())


def test_rows_satisfy_the_constraints_as_integers(skip4, step2, step3, unsigned3):
    """all 115 constraints hold as integer identities (no reduction mod p) on every row of T.2 of the four batches, rows cyclic, with every
    helper value below 2^32; both carry bits occur; zero blocks, unused second blocks, the partial last slot and the wrap row satisfy them"""
    cdl = cdh = 0
    for name, (kind, n, table, elems, pub) in _cases(skip4, step2, step3, unsigned3):
        n_proofs = len(elems)
        help_ = lm.helper(table, pub, n_proofs)
        assert help_.shape == (n_proofs * HC, table.shape[1]) and int(help_.max()) < 1 << 32
        for p in range(n_proofs):
            t, h, u = table[p * W:(p + 1) * W], help_[p * HC:(p + 1) * HC], pub[p * PW:(p + 1) * PW]
            res = lm.integer_residuals(t, h, u)
            assert len(res) == lm.CONSTRAINTS
            for j, c in enumerate(res):
                assert not c.any(), (name, p, j, np.flatnonzero(c)[:4])
            cdl, cdh = cdl + int(h[lm.HCD:lm.HCD + 16:2].sum()), cdh + int(h[lm.HCD + 1:lm.HCD + 16:2].sum())
            # DG on the last row of a lane's last live block is the public digest
            ends = np.flatnonzero(u[lm.PW_DIG:lm.PW_DIG + 16].any(axis=0))
            assert ends.size == n and np.array_equal(h[lm.HDG:lm.HDG + 16, 80 * ends + 79], u[lm.PW_DIG:lm.PW_DIG + 16, ends])
    assert cdl and cdh


def test_the_planes_have_full_degree(oracle):
    """STA, CHN, SEL, E79 and MSG interpolate to degree N - 1 at N = 128 .. 1024: no subgroup selector fits the 80-row blocks; the wrap row
    is ON in STA; the model's barycentric values of the planes and of a public row vector at a zeta outside the base field equal Horner on
    the interpolated coefficients"""
    for log_rows in (7, 8, 9, 10):
        N = 1 << log_rows
        for name, col in zip(("STA", "CHN", "SEL", "E79", "MSG"), lm.periodic(N)):
            assert am.degree(am.coefficients(oracle, col, 1)) == N - 1, (log_rows, name)
        assert lm.periodic(N)[0][N - 1] == 1 and not lm.periodic(N, wrap=False)[0][N - 1]
    zeta = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)
    assert lm.periodic_at(oracle, 7, zeta) == [am.horner(am.coefficients(oracle, c, 1), zeta) for c in lm.periodic(128)]
    rng = np.random.default_rng(12300)
    V = [rng.integers(0, P, 128, dtype=np.uint64) for _ in (0, 1)]
    a, b = (am.horner(am.coefficients(oracle, v, 1), zeta) for v in V)
    assert lm.public_at(oracle, 7, V, zeta) == fm.e_add(a, fm.e_mul((0, 1), b))


def _model_quotient(oracle, table, help_, pub, wrap=True):
    """(gamma, planar quotient) of pre-LDE columns of whole proofs at blow-up 4"""
    n_proofs, log_n = table.shape[0] // W, table.shape[1].bit_length() - 1 + LB
    ext, hext = oracle.lde(table, LB), oracle.lde(help_, LB)
    pext = oracle.lde(lm.periodic(table.shape[1], wrap), LB)
    g = lm.gamma(oracle, log_n, LB, CAP_H, n_proofs, _cap(oracle, ext, log_n), _cap(oracle, hext, log_n), pub)
    return g, lm.quotient(oracle, log_n, LB, n_proofs, ext, hext, pext, pub, _shift(), g, wrap=wrap)


def _degree10(oracle, t, h, u, wrap=True):
    return max(_degrees(oracle, _model_quotient(oracle, t, h, u, wrap)[1]))


def test_quotient_is_a_polynomial_of_degree_n_minus_2(oracle, step2, unsigned3):
    """T.2 of step N = 2 (two proofs, N = 512) and of the batch with lanes that did not sign, blow-up 4: the model quotient -- the 115
    constraints per proof under gamma, less the ONE public polynomial Pub_gamma, over x^N - 1 -- interpolates to degree exactly N - 2"""
    for kind, n, table, elems, pub in (step2, unsigned3):
        N = table.shape[1]
        g, quot = _model_quotient(oracle, table, lm.helper(table, pub, len(elems)), pub)
        deg = _degrees(oracle, quot)
        print(f"\n[sha512-link] T.2 of step N = {n}: N = {N}, quotient degrees {deg}")
        assert max(deg) == N - 2 and g[1] != 0


def test_the_identity_holds_at_zeta(oracle, step2):
    """T.2 of step N = 2, proof 0 alone, blow-up 4: the identity holds at a zeta outside the base field -- table, helper and quotient
    evaluated there by Horner on their coefficients, the planes and Pub_gamma barycentrically over the N rows, Pub_gamma equal to Horner on
    the coefficients interpolated through V; it fails after bumping u_0, a table or helper opening, a plane or Pub_gamma(zeta), and under
    another public word"""
    _, _, table, _, pub = step2
    table, pub = table[:W], pub[:PW]
    N, log_n = table.shape[1], 9 + LB
    help_ = lm.helper(table, pub, 1)
    g, quot = _model_quotient(oracle, table, help_, pub)
    M = 1 << log_n
    zeta = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)
    zs = (zeta, fm.e_scale(zeta, oracle.gl_root(9)))
    yt, yh = dm.evaluate(oracle, table, 1, zs), dm.evaluate(oracle, help_, 1, zs)
    u = [am.horner(am.coefficients(oracle, quot[k * M:(k + 1) * M], _shift()), zeta) for k in (0, 1)]
    t0, t1, h0, h1 = [tuple(y[0]) for y in yt], [tuple(y[1]) for y in yt], [tuple(y[0]) for y in yh], [tuple(y[1]) for y in yh]
    planes = lm.periodic_at(oracle, 9, zeta)
    V = lm.combine(pub, N, g)
    pubz = lm.public_at(oracle, 9, V, zeta)
    a, b = (am.horner(am.coefficients(oracle, np.array([int(x) for x in v], dtype=np.uint64), 1), zeta) for v in V)
    assert pubz == fm.e_add(a, fm.e_mul((0, 1), b)) and pubz != (0, 0)
    ident = lambda t0=t0, t1=t1, h0=h0, h1=h1, u0=u[0], planes=planes, pubz=pubz, pub=pub: lm.identity_at(
        oracle, log_n, LB, 1, t0, t1, h0, h1, u0, u[1], zeta, g, pub, planes, pubz)
    assert ident() and lm.identity_at(oracle, log_n, LB, 1, t0, t1, h0, h1, u[0], u[1], zeta, g, pub)
    bump = lambda v, at: v[:at] + [fm.e_add(v[at], (0, 1))] + v[at + 1:]
    assert not ident(u0=fm.e_add(u[0], (1, 0))) and not ident(pubz=fm.e_add(pubz, (1, 0)))
    assert not ident(t0=bump(t0, lm.W_ + 1)) and not ident(t0=bump(t0, lm.A_ + 5)) and not ident(h0=bump(h0, lm.HCH + 6)) and not ident(h1=bump(h1, lm.HCV + 3))
    for k in range(5):
        assert not ident(planes=bump(planes, k)), k
    other = pub.copy()
    other[lm.PW_W + 4, 0] ^= np.uint64(2)
    assert not lm.identity_at(oracle, log_n, LB, 1, t0, t1, h0, h1, u[0], u[1], zeta, g, other, planes)


W3_RERUN, ZERO_SECOND = "W_3 changed with everything behind it re-run", "a live second block replaced by zeros"
DETECTED = [W3_RERUN, ZERO_SECOND, "one changed public message limb", "one changed digest limb", "a flipped lv", "a flipped carry bit on a digest row",
            "a changed CV limb mid-block"]


def _changed(table, pub, kind):
    """(table, helper, public table) of ONE proof after a single change of `kind`; lane 1 (rows 160 .. 319) of T.2 of step N = 2 has two
    live blocks.  The helper is the honest one of the changed table unless the change is the helper's"""
    t, u = table[:W].copy(), pub[:PW].copy()
    r0 = 160
    assert t[:, r0].any() and t[:, r0 + 80].any()
    if kind == W3_RERUN:
        w16 = [_word(t, lm.W_, r0 + k) for k in range(16)]
        w16[3] ^= 1 << 40
        for k, x in enumerate(t9._schedule(w16)):
            t9._put(t, lm.W_, r0 + k, x)
        t9._run_lane(t, r0, IV512)
    elif kind == ZERO_SECOND:
        t[:, r0 + 80:r0 + 160] = 0
    elif kind == "one changed public message limb":
        u[lm.PW_W + 2 * 5 + 1, 2] ^= np.uint64(1 << 7)
    elif kind == "one changed digest limb":
        u[lm.PW_DIG + 2 * 6, 3] ^= np.uint64(1 << 30)
    elif kind == "a flipped lv":
        u[lm.PW_LV, 3] = 0
    h = lm.helper(t, u, 1)
    if kind == "a flipped carry bit on a digest row":
        h[lm.HCD + 2 * 4 + 1, r0 + 159] ^= np.uint64(1)
    elif kind == "a changed CV limb mid-block":
        h[lm.HCV + 2 * 2, r0 + 40] ^= np.uint64(1 << 3)
    return t, h, u


@pytest.mark.parametrize("kind", DETECTED)
def test_one_change_breaks_the_degree(oracle, step2, kind):
    """the detected kinds, on T.2 of step N = 2 (one proof): the quotient no longer interpolates to degree < N.  The first two are the
    changes tests/test_sha512_init.py records as unseen by sets 7 + 8 + 9: the model quotients of those sets of the SAME rows keep degree
    N - 2 -- the hole this set closes.  A changed public word or a flipped lv also moves the helper (lv decides CV) and gamma"""
    _, _, table, _, pub = step2
    N = table.shape[1]
    t, h, u = _changed(table, pub, kind)
    assert (t != table[:W]).sum() + (u != pub[:PW]).sum() + (h != lm.helper(table[:W], pub[:PW], 1)).sum() >= 1
    assert any(c.any() for c in lm.integer_residuals(t, h, u))
    deg = _degree10(oracle, t, h, u)
    print(f"\n[sha512-link] {kind}: quotient degree {deg}, N = {N}")
    assert deg >= N
    if kind in (W3_RERUN, ZERO_SECOND):
        d7, d8, d9 = t9._degree7(oracle, t), t9._degree8(oracle, t), t9._degree9(oracle, t)
        print(f"[sha512-link] {kind}: the quotient degrees of sets 7, 8 and 9 are {d7}, {d8}, {d9}")
        assert max(d7, d8, d9) <= N - 2


def test_the_wrap_row_is_what_ties_row_0_to_the_iv(oracle, step2):
    """the lane at row 0 re-run from another start state, with the helper a prover would commit for it (CV of slot 0 = that state) and the
    digest that run ends in claimed as public: every constraint but STA's on the wrap row N - 1 holds, so with an STA that is 0 there the
    quotient keeps degree N - 2 -- a digest that is not SHA-512 of the public message would pass -- and with the explicit wrap it does not"""
    _, _, table, _, pub = step2
    N = table.shape[1]
    t, u = table[:W].copy(), pub[:PW].copy()
    assert t[:, 0].any() and t[:, 80].any()
    bad = [x ^ (1 << (5 + 7 * j)) for j, x in enumerate(IV512)]
    t9._run_lane(t, 0, bad)
    # (the second block ran from IV + state, the chaining value set 9 states; the helper's chain starts from `bad`: run it from there)
    first = [(a + b) & M64 for a, b in zip(bad, [_word(t, c, 79) for c in range(lm.A_, W, 2)])]
    t9._run_block(t, 80, first)
    for j, (a, b) in enumerate(zip(first, [_word(t, c, 159) for c in range(lm.A_, W, 2)])):
        u[lm.PW_DIG + 2 * j, 1], u[lm.PW_DIG + 2 * j + 1, 1] = ((a + b) & M64) & M32, ((a + b) & M64) >> 32
    h = lm.helper(t, u, 1, start0=bad)
    res = lm.integer_residuals(t, h, u)
    broken = [j for j, c in enumerate(res) if c.any()]
    assert broken and all(lm.JSTA <= j < lm.JSTA + 16 for j in broken) and all(np.flatnonzero(res[j]).tolist() == [N - 1] for j in broken)
    assert not any(c.any() for c in lm.integer_residuals(t, h, u, wrap=False))
    assert _degree10(oracle, t, h, u, wrap=False) <= N - 2
    assert _degree10(oracle, t, h, u) >= N


def test_symbols_and_wrappers_exist(built_lib):
    """the new entry points are in the built library, bound in _lib.py and wrapped in context.py; the shape call against the table shapes
    of tmx_trace_commit_shape and its refusals; the model's offsets against the library's hint count"""
    import sha_public_model as sp
    from tendermintx_amd import _lib, context
    from tendermintx_amd._lib import TmxError
    from tendermintx_amd.context import Context
    for name in ("tmx_air_sha512_public_shape", "tmx_air_sha512_public_device", "tmx_air_sha512_link_helper_device",
                 "tmx_air_sha512_link_quotient_device", "tmx_air_sha512_link_quotient_range_device", "tmx_air_sha512_link_verify_device",
                 "tmx_trace_commit_set_air_sha512_link_device", "tmx_air_sha512_link_periodic_device", "tmx_air_sha512_link_periodic_eval_device",
                 "tmx_air_sha512_link_public_side_device", "tmx_air_sha512_link_public_eval_device"):
        assert getattr(built_lib, name).argtypes, name
        if "range" not in name:  # (the range call is the wrapper's proof_range / accumulate path)
            assert callable(getattr(Context, name[4:])), name
    assert (_lib.AIR_SHA512_PUBLIC_WIDTH, _lib.AIR_SHA512_LINK_HELPER_COLS, _lib.AIR_SHA512_LINK_CONSTRAINTS) == (PW, HC, lm.CONSTRAINTS)
    assert (_lib.TRACE_SHA512_LINK_HELPER, _lib.TRACE_SHA512_LINK_QUOTIENT) == (HELPER, QUOTIENT) == (2097152, 4194304)
    shape = context.air_sha512_public_shape
    # N = 512 rows: 7 slots (6 whole, 1 partial) -> 8; N = 1024: 13 -> 16; N = 2^15 (n_max = 128): 410 -> 512; N = 256: 4
    assert shape(1, 2, 2) == (3, 98) and shape(0, 4, 2) == (4, 98) and shape(1, 3, 1) == (3, 49) and shape(0, 128, 256) == (9, 49 * 256)
    assert shape(1, 1, 1) == (2, 49)
    for n in (1, 2, 3, 4, 128):
        assert shape(0, n, 1)[0] == lm.log_k(max(6, (160 * n - 1).bit_length()))
    for args in ((2, 4, 1), (0, 0, 1), (0, 4, 0), (0, 4, (1 << 24) // HC + 1)):
        with pytest.raises(TmxError):
            shape(*args)
    for kind, n in ((0, 4), (1, 3), (0, 128)):
        assert sp.Layout(kind, n).d == int(built_lib.tmx_hint_elem_count(kind, n))


# ---- GPU
@pytest.fixture(scope="module")
def ctx(built_lib):
    import tendermintx_amd as tmx
    c = tmx.Context(2, CID, max_batch=2)
    yield c
    c.close()


def _gather(c, kind, n_proofs, d_rows):
    log_k, n_cols = c.air_sha512_public_shape(kind, n_proofs)
    d_pub = _guarded(n_cols << log_k, lambda out: c.air_sha512_public_device(kind, n_proofs, d_rows.data_ptr(), out, 0))
    return d_pub, _down(d_pub).reshape(n_cols, 1 << log_k)


def _device_rows(c, kind, n, n_proofs, seed, unsign=()):
    """(element rows [P][stride], trace rows [P][elems]) of one synthetic batch, as tmx_witness_batch_device and tmx_trace_rows_device leave
    them on the device"""
    import torch
    dev = _dev()
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None for b in _workload(kind, n, n_proofs, seed, unsign)]
    out = torch.zeros((n_proofs, c.elem_stride(kind)), dtype=torch.int64, device=dev)
    rep = torch.zeros(n_proofs * 64, dtype=torch.uint8, device=dev)
    r = d[2].data_ptr() if d[2] is not None else None
    c.witness_batch_device(kind, n_proofs, d[0].data_ptr(), d[1].data_ptr(), r, out.data_ptr(), rep.data_ptr(), 0)
    tr = torch.zeros((n_proofs, c.trace_elem_count(kind)), dtype=torch.int64, device=dev)
    c.trace_rows_device(kind, n_proofs, d[1].data_ptr(), r, tr.data_ptr(), 63, 0)
    torch.cuda.synchronize(dev)
    return out, tr


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,seed,unsign", [(0, 4, 8100, ()), (1, 2, 8200, ()), (1, 3, 8300, ()), (1, 3, 8300, ((0, 1), (1, 2)))])
def test_gather_equals_the_model(built_lib, oracle, kind, n, seed, unsign):
    """tmx_air_sha512_public_device on the rows tmx_witness_batch_device left, skip N = 4, step N = 2, step N = 3 and the batch with lanes
    that did not sign, two proofs: every word equals the model's table built from the same rows, guard words intact; and the link on the
    device's own rows -- w[k][t] is the W of row 80 k + t of the trace rows tmx_trace_rows_device wrote from the context's Level-1 scratch,
    lv their liveness, and DG of the model helper on a lane's last live row is the public digest"""
    import tendermintx_amd as tmx
    n_proofs = 2
    with tmx.Context(n, CID, max_batch=n_proofs) as c:
        d_rows, d_trace = _device_rows(c, kind, n, n_proofs, seed, unsign)
        rows = _down(d_rows).reshape(n_proofs, -1)
        _, got = _gather(c, kind, n_proofs, d_rows)
        log_k, n_cols = c.air_sha512_public_shape(kind, n_proofs)
        want = lm.public_table(kind, n, list(rows), log_k, oracle.dummy())
        assert got.shape == want.shape == (PW * n_proofs, 1 << log_k)
        assert np.array_equal(got, want), np.argwhere(got != want)[:10]
        table = _columns(list(_down(d_trace).reshape(n_proofs, -1)), kind, n)
        N = table.shape[1]
        help_ = lm.helper(table, got, n_proofs)
        for p in range(n_proofs):
            t, u, h = table[p * W:(p + 1) * W], got[p * PW:(p + 1) * PW], help_[p * HC:(p + 1) * HC]
            blocks = t[:, :160 * n].reshape(W, 2 * n, 80)
            for l in (0, 1):
                assert np.array_equal(u[lm.PW_W + l:lm.PW_W + 32:2, :2 * n], blocks[lm.W_ + l, :, :16].T), (p, l)
            assert np.array_equal(u[lm.PW_LV, :2 * n], blocks[:, :, 0].any(axis=0).astype(np.uint64)) and not u[:, 2 * n:].any()
            ends = np.flatnonzero(u[lm.PW_DIG:lm.PW_DIG + 16].any(axis=0))
            assert ends.size == n and np.array_equal(h[lm.HDG:lm.HDG + 16, 80 * ends + 79], u[lm.PW_DIG:lm.PW_DIG + 16, ends])
            one_block = int((u[lm.PW_LV, 0:2 * n:2] > u[lm.PW_LV, 1:2 * n:2]).sum())
            assert one_block >= sum(1 for q, _ in unsign if q == p)


@pytest.mark.gpu
def test_gather_pads_at_the_lengths_where_it_moves(built_lib, oracle):
    """the padding test's rows on the device (n_max = 4, two proofs): the model's table word for word, and the statement of the padding
    itself on the DEVICE's words"""
    import tendermintx_amd as tmx
    with tmx.Context(PAD_N, CID, max_batch=2) as c:
        rows = _synthetic_rows(1, PAD_N, c.elem_stride(1), [LENGTHS[:PAD_N], LENGTHS[PAD_N:] + [31]])
        _, got = _gather(c, 1, 2, _up(rows))
        assert np.array_equal(got, lm.public_table(1, PAD_N, list(rows), lm.log_k(10), oracle.dummy()))
        _check_padding(got, rows, PAD_N, oracle.dummy())


def _device_helper(ctx, table, pub):
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    d_table, d_pub = _up(table), _up(pub)
    return _guarded((n_proofs * HC) << log_rows,
                    lambda out: ctx.air_sha512_link_helper_device(log_rows, n_proofs, d_table.data_ptr(), d_pub.data_ptr(), out, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs", [(7, 1), (7, 3), (9, 3), (10, 2), (8, 257)])
def test_helper_of_random_tables_equals_the_model(ctx, log_rows, n_proofs):
    """random 64-bit table words and random lv -- clear, 1, a word whose low 32 bits are zero (clear), a word above 2^32 with low bits
    (set), on every slot, the partial last one and the padding included: the helper equals the model's word for word, guard words intact.
    log_rows 7 is one block and a partial one (the slot behind the partial one is slot 0); 257 proofs cross every power-of-two grid edge"""
    rng = np.random.default_rng(12100 + 100 * log_rows + n_proofs)
    R = 1 << log_rows
    K = 1 << lm.log_k(log_rows)
    table = rng.integers(0, 1 << 64, (n_proofs * W, R), dtype=np.uint64)
    pub = rng.integers(0, 1 << 32, (n_proofs * PW, K), dtype=np.uint64)
    kinds = np.array([0, 1, 1 << 32, (5 << 32) | 7], dtype=np.uint64)
    pub[lm.PW_LV::PW] = kinds[rng.integers(0, 4, (n_proofs, K))]
    pub[lm.PW_LV, :2] = 1  # (proof 0 begins with a live block in front of a live one, whatever was drawn)
    got = _down(_device_helper(ctx, table, pub)).reshape(n_proofs * HC, -1)
    want = lm.helper(table, pub, n_proofs)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    assert int(want.max()) < 1 << 32 and want[lm.HCD:lm.HCD + 16:2].any() and want[lm.HCD + 1:lm.HCD + 16:2].any()
    assert want[lm.HLN, :80].all() and np.array_equal(want[lm.HCH:lm.HCH + 16, :80], want[lm.HDG:lm.HDG + 16, :80])
    # the wrap on its own: LN of the last slot is lv of slot 0 of the SAME proof
    for p in (0, n_proofs - 1):
        assert int(want[p * HC + lm.HLN, R - 1]) == lm._flag(pub[p * PW + lm.PW_LV, 0])


@pytest.mark.gpu
def test_helper_of_real_rows_equals_the_model(ctx, skip4, unsigned3):
    """the real T.2 rows of skip N = 4 (1024 rows) and of the batch with lanes that did not sign (512 rows) under their own public tables:
    the model's words -- all 115 constraints hold on them (the CPU test above)"""
    for kind, n, table, elems, pub in (skip4, unsigned3):
        got = _down(_device_helper(ctx, table, pub)).reshape(len(elems) * HC, -1)
        assert np.array_equal(got, lm.helper(table, pub, len(elems)))


@pytest.mark.gpu
def test_each_validation_rule(ctx):
    """every rule of the two device calls on its own: TMX_ERR_BAD_ARG before anything is enqueued, nothing written"""
    d_table, d_pub, d_help = _sentinel(W << 7), _sentinel(PW << 1), _sentinel(HC << 7)
    hp = lambda lr, n, t=d_table.data_ptr(), u=d_pub.data_ptr(), o=d_help.data_ptr(): (lambda: ctx.air_sha512_link_helper_device(lr, n, t, u, o, 0))
    for fn in (hp(6, 1), hp(19, 1), hp(7, 0), hp(7, (1 << 24) // HC + 1), hp(7, 1, t=None), hp(7, 1, u=None), hp(7, 1, o=None)):
        _refused(fn, d_help)
    rows, pub = _sentinel(16), _sentinel(16)
    g = lambda kind, n, r=rows.data_ptr(), u=pub.data_ptr(): (lambda: ctx.air_sha512_public_device(kind, n, r, u, 0))
    for fn in (g(2, 1), g(0, 0), g(0, (1 << 24) // HC + 1), g(0, 1, r=None), g(0, 1, u=None)):
        _refused(fn, pub)


# ---- GPU: the planes and the public side
def _periodic(ctx, log_rows, log_blowup):
    import torch
    N, M = 1 << log_rows, 1 << (log_rows + log_blowup)
    d_pre, d_ext = _sentinel(5 * N + GUARD), _sentinel(5 * M + GUARD)
    ctx.air_sha512_link_periodic_device(log_rows, log_blowup, d_pre.data_ptr(), d_ext.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(d_pre[5 * N:], _sentinel(GUARD)) and torch.equal(d_ext[5 * M:], _sentinel(GUARD))
    return _down(d_pre[:5 * N]).reshape(5, N), _down(d_ext[:5 * M]).reshape(5, M)


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,log_blowup", [(7, 1), (9, 3), (10, 1)])
def test_the_planes_and_their_extension(ctx, oracle, log_rows, log_blowup):
    """STA, CHN, SEL, E79, MSG before the LDE (planar, 5 << log_rows words, nothing behind them) and extended under the context's domain,
    against the model and the CPU oracle's LDE"""
    pre, ext = _periodic(ctx, log_rows, log_blowup)
    want = lm.periodic(1 << log_rows)
    assert np.array_equal(pre, want) and np.array_equal(ext, oracle.lde(want, log_blowup))


def _bary(ctx, log_rows, zeta_words, v=None):
    """the words of tmx_air_sha512_link_periodic_eval_device (11) or, with V, of tmx_air_sha512_link_public_eval_device (3) at the two words
    of zeta as given; the words behind them stay untouched"""
    import torch
    n = 11 if v is None else 3
    d_zeta, d_out = _up(np.array(zeta_words, dtype=np.uint64)), _sentinel(n + GUARD)
    if v is None:
        ctx.air_sha512_link_periodic_eval_device(log_rows, d_zeta.data_ptr(), d_out.data_ptr(), 0)
    else:
        ctx.air_sha512_link_public_eval_device(log_rows, v.data_ptr(), d_zeta.data_ptr(), d_out.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(d_out[n:], _sentinel(GUARD))
    return [int(x) for x in _down(d_out[:n])]


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows", [7, 10, 15, 18])
def test_the_planes_and_pub_at_zeta_equal_the_model(ctx, oracle, log_rows):
    """the five planes and Pub_gamma -- from a random V with a few non-canonical words -- at a random zeta of F_p^2 over N = 128 (half a
    workgroup), 1024 (one), 2^15 (32 workgroups, the full size) and 2^18 (64 workgroups, four batches per thread): the kernels' values equal
    the model's barycentric sums, no zero denominator"""
    rng = np.random.default_rng(12500 + log_rows)
    N = 1 << log_rows
    zeta = tuple(int(x) for x in rng.integers(1, P, 2, dtype=np.uint64))
    assert _bary(ctx, log_rows, zeta) == [x for v in lm.periodic_at(oracle, log_rows, zeta) for x in v] + [0]
    V = rng.integers(0, P, (2, N), dtype=np.uint64)
    V[:, ::3] = 0  # (most rows carry no public term)
    V[0, 5], V[1, N - 1] = np.uint64(P), np.uint64(P + 3)
    assert _bary(ctx, log_rows, zeta, _up(V)) == list(lm.public_at(oracle, log_rows, [V[0] % np.uint64(P), V[1] % np.uint64(P)], zeta)) + [0]


@pytest.mark.gpu
@pytest.mark.parametrize("r", [5, 1029, 1359])
def test_zero_denominators_are_flagged_in_every_slot_and_workgroup(ctx, oracle, r):
    """zeta = (omega^r, 0) at N = 4096 (four workgroups, T = 1024 threads, thread g takes the rows g + 1024 m as slot m): r = 5 is slot 0 of
    workgroup 0, r = 1029 slot 1 of workgroup 0, r = 1359 slot 1 of workgroup 1 -- both kernels raise their flag; one step off the domain
    neither does, and a small evaluation behind a flagged one folds no stale flag"""
    om = oracle.gl_root(12)
    assert (r % 1024 // 256, r // 1024) in ((0, 0), (0, 1), (1, 1))
    V = _up(np.random.default_rng(12600).integers(0, P, (2, 4096), dtype=np.uint64))
    assert _bary(ctx, 12, (pow(om, r, P), 0))[10] == 1 and _bary(ctx, 12, (pow(om, r, P), 0), V)[2] == 1
    assert _bary(ctx, 12, (pow(om, r, P), 1))[10] == 0 and _bary(ctx, 12, (pow(om, r, P), 1), V)[2] == 0
    assert _bary(ctx, 9, (pow(om, r, P), 0))[10] == 0 and _bary(ctx, 9, (pow(om, r, P), 0), V[:1024])[2] == 0


def _random_pub(rng, n_proofs, log_rows):
    """random public words below 2^32 on every slot, the padding included; a few above 2^32 and non-canonical"""
    pub = rng.integers(0, 1 << 32, (n_proofs * PW, 1 << lm.log_k(log_rows)), dtype=np.uint64)
    pub[lm.PW_LV::PW] &= np.uint64(1)
    pub[3, 0], pub[lm.PW_DIG + 1, 1] = np.uint64(P + 5), np.uint64((7 << 32) | 9)
    return pub


SHAPES = [(7, 1, 1), (9, 3, 3), (10, 1, 2)]  # (log N, log blow-up, proofs); N = 128 is one block and a partial one


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,log_blowup,n_proofs", SHAPES)
def test_v_and_the_extended_pub_equal_the_model(ctx, oracle, log_rows, log_blowup, n_proofs):
    """V_r under a given gamma (Horner over the proofs, one lane per row) and Pub_gamma on the coset, from random public words: the model's
    words, guard words intact"""
    import torch
    rng = np.random.default_rng(12700 + 10 * log_rows + n_proofs)
    N, M = 1 << log_rows, 1 << (log_rows + log_blowup)
    pub = _random_pub(rng, n_proofs, log_rows)
    g = tuple(int(x) for x in rng.integers(1, P, 2, dtype=np.uint64))
    d_v, d_ext, d_pub, d_g = _sentinel(2 * N + GUARD), _sentinel(2 * M + GUARD), _up(pub), _up(np.array(g, dtype=np.uint64))
    ctx.air_sha512_link_public_side_device(log_rows, log_blowup, n_proofs, d_pub.data_ptr(), d_g.data_ptr(), d_v.data_ptr(), d_ext.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(d_v[2 * N:], _sentinel(GUARD)) and torch.equal(d_ext[2 * M:], _sentinel(GUARD))
    want = np.array([[int(x) for x in v] for v in lm.combine(pub, N, g)], dtype=np.uint64)
    assert np.array_equal(_down(d_v[:2 * N]).reshape(2, N), want) and want.any(axis=1).all()
    assert np.array_equal(_down(d_ext[:2 * M]).reshape(2, M), lm.public_extended(oracle, log_rows + log_blowup, log_blowup, pub, g))


# ---- GPU: the quotient
def _device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, d_pub, cap_height=CAP_H, **kw):
    return _guarded(2 << log_n, lambda out: ctx.air_sha512_link_quotient_device(log_n, log_blowup, cap_height, n_proofs, d_cols.data_ptr(),
                                                                               d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(),
                                                                               d_pub.data_ptr(), out, 0, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,log_blowup,n_proofs", SHAPES)
def test_quotient_of_random_columns_equals_the_model(ctx, oracle, log_rows, log_blowup, n_proofs):
    """random table, helper and public words (a few non-canonical): the definition is pointwise, so gamma and d_quot equal the model word
    for word -- whole, and through the range call as [1, P) written + [0, 1) accumulated and in the other order (the piece that starts at
    proof 0 carries the public polynomial); guard words intact"""
    import torch
    log_n = log_rows + log_blowup
    rng = np.random.default_rng(12800 + 100 * log_n + 10 * log_blowup + n_proofs)
    ext, hext = _random_ext(rng, n_proofs * W, log_n), _random_ext(rng, n_proofs * HC, log_n)
    pub = _random_pub(rng, n_proofs, log_rows)
    d_cols, d_hcols, d_pub = _up(ext), _up(hext), _up(pub)
    _, d_cap = _tree(ctx, d_cols, log_n, n_proofs * W)
    _, d_cap_h = _tree(ctx, d_hcols, log_n, n_proofs * HC)
    got = _down(_device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, d_pub))
    g = lm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _down(d_cap), _down(d_cap_h), pub)
    assert ctx.air_last_gamma() == g
    pext = oracle.lde(lm.periodic(1 << log_rows), log_blowup)
    want = lm.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, pext, pub, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    pieces, words = ([(1, n_proofs), (0, 1)] if n_proofs > 1 else [(0, 1)]), 2 << log_n
    for order in (pieces, pieces[::-1]):
        buf = _sentinel(words + 2 * GUARD)
        for k, (lo, hi) in enumerate(order):
            d_piece = d_hcols[(lo * HC) << log_n:]
            ctx.air_sha512_link_quotient_device(log_n, log_blowup, CAP_H, n_proofs, d_cols.data_ptr(), d_piece.data_ptr(), d_cap.data_ptr(),
                                                d_cap_h.data_ptr(), d_pub.data_ptr(), buf[GUARD:].data_ptr(), 0, proof_range=(lo, hi),
                                                accumulate=int(k > 0))
        torch.cuda.synchronize(_dev())
        assert np.array_equal(_down(buf[GUARD:GUARD + words]), want), order
        assert torch.equal(buf[:GUARD], _sentinel(GUARD)) and torch.equal(buf[GUARD + words:], _sentinel(GUARD)), order


# ---- GPU: the chain and the verifiers
def _chain(ctx, oracle, table, pub, log_blowup, q_override=None, n_queries=6, others=()):
    """caller-level chain: helper -> LDE -> caps -> quotient -> one batch proof over [table, H10, Q10].  others: (position, extended
    columns) of further oracles.  Returns a dict: the params, the caps on the device, the proof words, kt, gamma, the extended columns"""
    import torch
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    log_n = log_rows + log_blowup

    def lde(d_pre, n):
        d_out = _sentinel(n << log_n)
        ctx.lde_device(log_rows, log_blowup, n, d_pre.data_ptr(), d_out.data_ptr(), 0)
        return d_out
    d_pub = _up(pub)
    d_ext = lde(_up(table), n_proofs * W)
    d_lv_t, d_cap_t = _tree(ctx, d_ext, log_n, n_proofs * W)
    d_h = lde(_device_helper(ctx, table, pub), n_proofs * HC)
    d_lv_h, d_cap_h = _tree(ctx, d_h, log_n, n_proofs * HC)
    gamma = None
    if q_override is None:
        d_q = _device_quotient(ctx, log_n, log_blowup, n_proofs, d_ext, d_h, d_cap_t, d_cap_h, d_pub)
        gamma = ctx.air_last_gamma()
    else:
        d_q = _up(q_override)
    d_lv_q, d_cap_q = _tree(ctx, d_q, log_n, 2)
    members = [(d_ext, d_lv_t, d_cap_t, n_proofs * W), (d_h, d_lv_h, d_cap_h, n_proofs * HC), (d_q, d_lv_q, d_cap_q, 2)]
    log_ns = [log_n] * 3
    for at, e in others:
        d_o, lo = _up(e), e.shape[1].bit_length() - 1
        d_lv_o, d_cap_o = _tree(ctx, d_o, lo, e.shape[0])
        members.insert(at, (d_o, d_lv_o, d_cap_o, e.shape[0]))
        log_ns.insert(at, lo)
    kt = next(k for k, m in enumerate(members) if m[0] is d_ext)
    p = bparams(log_ns, [m[3] for m in members], CAP_H, log_blowup, 2, 2, n_queries)
    proof = _guarded(bm.layout(p)["words"], lambda o: ctx.batch_prove_device(p, [m[0].data_ptr() for m in members], [m[1].data_ptr() for m in members], o, 0))
    return dict(p=p, d_caps=torch.cat([m[2] for m in members]), proof=_down(proof), kt=kt, gamma=gamma, ext=_down(d_ext).reshape(n_proofs * W, -1),
                hext=_down(d_h).reshape(n_proofs * HC, -1), quot=_down(d_q))


def _verdicts(ctx, p, k_trace, k_helper, d_caps, proof, pub):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    d_proof, d_pub = _up(proof), _up(pub)  # (both held until the call has run)
    ctx.air_sha512_link_verify_device(p, k_trace, k_helper, d_caps.data_ptr(), d_proof.data_ptr(), d_pub.data_ptr(), ok.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    out = ok.cpu().numpy()
    assert ((out == 0) | (out == 1)).all(), out
    return [bool(x) for x in out]


@pytest.mark.gpu
def test_real_rows_through_the_caller_level_chain(ctx, oracle, step2):
    """[table, H10, Q10] of T.2 of step N = 2 (two proofs, N = 512, blow-up 2) in one batch proof: helper, gamma and quotient equal the
    model's and the quotient has degree N - 2; the device verifier accepts every query, as the model does; it rejects a proof with one
    bumped table, helper or quotient opening on every query, and the honest proof under one changed public word, as the model's identity
    fails"""
    _, _, table, _, pub = step2
    lb, n_proofs = 1, 2
    c = _chain(ctx, oracle, table, pub, lb)
    assert ctx.fri_last_degree_ok() is True
    p, d_caps, got = c["p"], c["d_caps"], c["proof"]
    assert p["n_cols"] == [n_proofs * W, n_proofs * HC, 2] and c["kt"] == 0
    log_n, caps, cw = p["log_n"][0], _down(d_caps), 4 << CAP_H
    assert np.array_equal(c["hext"], oracle.lde(lm.helper(table, pub, n_proofs), lb))
    g = lm.gamma(oracle, log_n, lb, CAP_H, n_proofs, caps[:cw], caps[cw:2 * cw], pub)
    assert c["gamma"] == g
    pext = oracle.lde(lm.periodic(table.shape[1]), lb)
    assert np.array_equal(c["quot"], lm.quotient(oracle, log_n, lb, n_proofs, c["ext"], c["hext"], pext, pub, _shift(), g))
    assert max(_degrees(oracle, c["quot"])) == table.shape[1] - 2
    model = lm.verify(oracle, p, 0, 1, caps, got, _shift(), pub)
    assert all(model) and _verdicts(ctx, p, 0, 1, d_caps, got, pub) == model
    L = bm.layout(p)
    RH = 1 << dm.log_r(p["n_cols"][1])
    for name, at in (("quotient opening", L["off_open"][2] + 1), ("helper opening at zeta", L["off_open"][1] + lm.HDG + 5),
                     ("helper opening at zeta omega", L["off_open"][1] + 2 * RH + HC + lm.HCV + 1),
                     ("table opening at zeta", L["off_open"][0] + W + lm.W_ + 1)):
        bad = t9._bumped(got, at)
        assert not lm.identity(oracle, p, 0, 1, caps, bad, pub), name
        assert _verdicts(ctx, p, 0, 1, d_caps, bad, pub) == [False] * p["n_queries"], name
    other = pub.copy()
    other[PW + lm.PW_DIG + 3, 2] ^= np.uint64(1)
    assert not lm.identity(oracle, p, 0, 1, caps, got, other)
    assert _verdicts(ctx, p, 0, 1, d_caps, got, other) == [False] * p["n_queries"]


@pytest.mark.gpu
def test_the_changed_w3_passes_sets_7_8_and_9_and_fails_set_10_on_the_device(ctx, oracle, step2):
    """the test that carries the feature.  The table whose lane 1 has W_3 changed with the schedule, the rounds and the second block re-run
    from it, under the honest helpers of the changed table: over [table, H7, Q7, H8, Q8, H9, Q9] THE DEVICE VERIFIERS OF SETS 7, 8 AND 9
    ACCEPT every query; over [table, H10, Q10] with the honest public table and a zero (low-degree) quotient SET 10'S REJECTS every one,
    as the models do"""
    _, _, table, _, pub = step2
    t, _, _ = _changed(table, pub, W3_RERUN)
    log_n = 9 + 1
    c = t9._chain(ctx, oracle, t, 1)
    p, d_caps, got = c["p"], c["d_caps"], c["proof"]
    n = p["n_queries"]
    assert t9._verdicts(ctx, p, 0, None, d_caps, got, which="7") == [True] * n and t9._verdicts(ctx, p, 0, 3, d_caps, got, which="8") == [True] * n
    assert t9._verdicts(ctx, p, 0, 5, d_caps, got) == [True] * n
    c = _chain(ctx, oracle, t, pub[:PW], 1, q_override=np.zeros(2 << log_n, dtype=np.uint64))
    p, d_caps, got = c["p"], c["d_caps"], c["proof"]
    assert all(t9._verdicts(ctx, p, 0, None, d_caps, got, which="0"))
    assert not lm.identity(oracle, p, 0, 1, _down(d_caps), got, pub[:PW])
    assert _verdicts(ctx, p, 0, 1, d_caps, got, pub[:PW]) == [False] * n


@pytest.mark.gpu
def test_257_proofs_through_the_check_kernel(ctx, oracle, step2):
    """N = 128, 257 proofs (one more than k_air_sha512_link_check has threads: thread 0 takes proofs 0 and 256): the first block of the live
    lanes of T.2 of step N = 2 in turn as a one-block table (lv = 1, 0; its digest IV + state: the rows of the partial slot are zero), every
    seventh proof zero, blow-up 2, two queries: the device accepts every query as the model's identity does; a helper opening bumped in
    proof 256 and a table opening in proof 255 are rejected"""
    _, _, src, _, _ = step2
    many = 257
    lanes = [src[q * W:(q + 1) * W, 160 * b:160 * b + 80] for q in range(src.shape[0] // W) for b in range(2)]
    table = np.zeros((many * W, 128), dtype=np.uint64)
    pub = np.zeros((many * PW, 2), dtype=np.uint64)
    for q in range(many):
        if q % 7 != 6:
            t = lanes[q % len(lanes)]
            table[q * W:(q + 1) * W, :80] = t
            u = pub[q * PW:(q + 1) * PW]
            u[lm.PW_W:lm.PW_W + 32:2, 0], u[lm.PW_W + 1:lm.PW_W + 32:2, 0], u[lm.PW_LV, 0] = t[lm.W_, :16], t[lm.W_ + 1, :16], 1
            for j in range(8):
                d = (IV512[j] + _word(t, lm.A_ + 2 * j, 79)) & M64
                u[lm.PW_DIG + 2 * j, 0], u[lm.PW_DIG + 2 * j + 1, 0] = d & M32, d >> 32
    assert not any(c.any() for c in lm.integer_residuals(table[:W], lm.helper(table[:W], pub[:PW], 1), pub[:PW]))
    c = _chain(ctx, oracle, table, pub, 1, n_queries=2)
    assert ctx.fri_last_degree_ok() is True
    p, d_caps, got, caps = c["p"], c["d_caps"], c["proof"], _down(c["d_caps"])
    assert lm.identity(oracle, p, 0, 1, caps, got, pub)
    assert _verdicts(ctx, p, 0, 1, d_caps, got, pub) == [True, True]
    L = bm.layout(p)
    for at in (L["off_open"][1] + 256 * HC + lm.HDG + 3, L["off_open"][0] + 255 * W + lm.A_ + 4):
        bad = t9._bumped(got, at)
        assert not lm.identity(oracle, p, 0, 1, caps, bad, pub)
        assert _verdicts(ctx, p, 0, 1, d_caps, bad, pub) == [False, False]


# ---- GPU: the set level
@pytest.fixture(scope="module")
def device_set(ctx):
    """(trace rows, T.2 columns, the device's public table and its host copy) of two step N = 2 proofs on the device"""
    d_rows, d_trace = _device_rows(ctx, 1, 2, 2, 9300)
    d_pub, pub = _gather(ctx, 1, 2, d_rows)
    return d_trace, _columns(list(_down(d_trace).reshape(2, -1)), 1, 2), d_pub, pub


def _set_round(c, tr, d_pub, calls, sections=SHA512 | HEADER, queries=6, lb=1):
    """commit `sections` of two step proofs, the air calls of `calls` ("9": set 9's, "X": set 10's) on SHA512 in that order, one proof.
    Returns (params, the sections in oracle order, the caps in that order on the device, proof words, {set: gamma})"""
    import torch
    cw = 4 << CAP_H
    d_caps = _sentinel(bin(sections).count("1") * cw)
    own = {s: _sentinel(cw) for s in (H9, Q9, HELPER, QUOTIENT)}
    c.trace_commit_set_device(1, 2, sections, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
    _, order0 = c.trace_commit_set_shape()
    gammas = {}
    for s in calls:
        if s == "9":
            c.trace_commit_set_air_sha512_init_device(SHA512, own[H9].data_ptr(), own[Q9].data_ptr(), 0)
        else:
            c.trace_commit_set_air_sha512_link_device(SHA512, d_pub.data_ptr(), own[HELPER].data_ptr(), own[QUOTIENT].data_ptr(), 0)
        gammas[s] = c.air_last_gamma()
    shape, order = c.trace_commit_set_shape()
    p = dict(shape, arity_bits=2, final_log_max=2, n_queries=queries, pow_bits=0)
    proof = _down(_guarded(bm.layout(p)["words"], lambda out: c.trace_commit_set_prove_device(p, out, 0)))
    assert c.fri_last_degree_ok() is True
    caps_of = {s: d_caps[cw * i:cw * (i + 1)] for i, s in enumerate(order0)}
    caps_of.update(own)
    return p, order, torch.cat([caps_of[s] for s in order]), proof, gammas


@pytest.mark.gpu
def test_set_level_alone_and_beside_set_9(ctx, oracle, device_set):
    """a set SHA512 | HEADER of two step N = 2 proofs.  Set 10's call alone: the shape [HEADER, SHA512, 2097152, 4194304]; caps, gamma and
    proof words equal the caller-level chain's over the same columns (the header table as one more oracle); the device verifier accepts,
    as the model's identity holds, and rejects under a changed public word.  Beside set 9's pair in both call orders: [.., 524288, 1048576,
    2097152, 4194304] either way, with the same caps, gammas and proof words, and set 10's caps and gamma those of the call alone"""
    import torch
    from test_merkle_open import _oracle_ext
    tr, table, d_pub, pub = device_set
    lb, cw = 1, 4 << CAP_H
    p, order, d_caps, proof, gammas = _set_round(ctx, tr, d_pub, "X")
    assert order == [HEADER, SHA512, HELPER, QUOTIENT]
    assert p["log_n"][1:] == [9 + lb] * 3 and p["n_cols"][1:] == [W * 2, HC * 2, 2]
    e, _, nc = _oracle_ext(oracle, 1, 2, _down(tr), HEADER, lb)
    ch = _chain(ctx, oracle, table, pub, lb, others=[(0, e.reshape(nc, -1))])
    assert {key: ch["p"][key] for key in ("log_n", "n_cols")} == {key: p[key] for key in ("log_n", "n_cols")} and ch["kt"] == 1
    assert gammas["X"] == ch["gamma"] and torch.equal(d_caps, ch["d_caps"]) and np.array_equal(proof, ch["proof"])
    assert lm.identity(oracle, p, 1, 2, _down(d_caps), proof, pub)
    assert _verdicts(ctx, p, 1, 2, d_caps, proof, pub) == [True] * 6
    other = pub.copy()
    other[lm.PW_W + 9, 1] ^= np.uint64(4)
    assert _verdicts(ctx, p, 1, 2, d_caps, proof, other) == [False] * 6
    a = _set_round(ctx, tr, d_pub, "9X")
    assert a[1] == [HEADER, SHA512, H9, Q9, HELPER, QUOTIENT]
    b = _set_round(ctx, tr, d_pub, "X9")
    assert b[1] == a[1] and b[0] == a[0] and torch.equal(b[2], a[2]) and np.array_equal(b[3], a[3]) and b[4] == a[4]
    assert torch.equal(a[2][4 * cw:], d_caps[2 * cw:]) and a[4]["X"] == gammas["X"]
    assert _verdicts(ctx, a[0], 1, 4, a[2], a[3], pub) == [True] * 6
    assert t9._verdicts(ctx, a[0], 1, 2, a[2], a[3]) == [True] * 6


@pytest.mark.gpu
def test_set_level_refusals_and_the_eight_oracle_limit(ctx, device_set):
    """the set-level call takes TMX_TRACE_SHA512 alone, a resident member only, refuses a second call on the section and a null pointer,
    each with nothing enqueued and the set as it was; the streamed SHA-512 call keeps refusing constraint_set = 10; behind the pairs of
    sets 7, 8 and 9 (seven oracles) there is no room for set 10's pair: TMX_BATCH_MAX_ORACLES stays 8"""
    c, (tr, _, d_pub, _) = ctx, device_set
    lb, cw = 1, 4 << CAP_H
    d_caps, d_cap_h, d_cap_q = _sentinel(2 * cw), _sentinel(cw), _sentinel(cw)
    air = lambda sec, u=d_pub.data_ptr(), h=d_cap_h.data_ptr(), q=d_cap_q.data_ptr(): (lambda: c.trace_commit_set_air_sha512_link_device(sec, u, h, q, 0))
    commit = lambda secs=SHA512 | HEADER: c.trace_commit_set_device(1, 2, secs, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
    commit()
    before = c.trace_commit_set_shape()
    for sec in (HEADER, SHA256, 1, H9, HELPER):
        assert "TMX_TRACE_SHA512" in _refused(air(sec), d_cap_h, d_cap_q)
    for fn in (air(SHA512, u=None), air(SHA512, h=None), air(SHA512, q=None)):
        _refused(fn, d_cap_h, d_cap_q)
    _refused(lambda: c.trace_commit_set_air_sha512_streamed_device(10, SHA512, 8, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0), d_cap_h, d_cap_q)
    assert c.trace_commit_set_shape() == before
    air(SHA512)()
    after = c.trace_commit_set_shape()
    assert after[1] == [HEADER, SHA512, HELPER, QUOTIENT]
    assert "already" in _refused(air(SHA512), d_cap_h, d_cap_q)
    assert c.trace_commit_set_shape() == after
    commit(HEADER)
    assert "does not hold" in _refused(air(SHA512), d_cap_h, d_cap_q)
    c.trace_commit_set_streamed_device(1, 2, SHA512 | HEADER, SHA512, 8, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
    assert "streamed" in _refused(air(SHA512), d_cap_h, d_cap_q)
    commit(SHA512)
    c.trace_commit_set_air_sha512_device(SHA512, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
    c.trace_commit_set_air_sha512_sched_device(SHA512, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
    c.trace_commit_set_air_sha512_init_device(SHA512, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
    full = c.trace_commit_set_shape()
    assert len(full[1]) == 7
    assert "room" in _refused(air(SHA512), d_cap_h, d_cap_q)
    assert c.trace_commit_set_shape() == full


@pytest.mark.gpu
def test_each_validation_rule_of_the_quotient_and_the_verifier(ctx):
    """every rule on its own: TMX_ERR_BAD_ARG before anything is enqueued, nothing written.  FRI's rules on log_n and log_blowup;
    7 <= log_n - log_blowup <= 18; n_proofs >= 1; 65 n_proofs <= 2^24; a range inside n_proofs; accumulate <= 1; no null pointer"""
    log_n, lb = 8, 1
    bufs = {k: _sentinel(n) for k, n in (("cols", W << log_n), ("h", HC << log_n), ("cap", 16), ("cap_h", 16), ("pub", PW << 1), ("q", 2 << log_n))}
    ptr = {k: v.data_ptr() for k, v in bufs.items()}

    def q(log_n=log_n, lb=lb, n=1, rng=None, acc=0, **null):
        a = {k: (None if k in null else v) for k, v in ptr.items()}
        return lambda: ctx.air_sha512_link_quotient_device(log_n, lb, CAP_H, n, a["cols"], a["h"], a["cap"], a["cap_h"], a["pub"], a["q"], 0,
                                                           proof_range=rng, accumulate=acc)
    for fn in (q(lb=0), q(lb=7, log_n=14), q(log_n=7), q(log_n=20, lb=1), q(n=0), q(n=(1 << 24) // HC + 1), q(rng=(1, 1)), q(rng=(0, 2)), q(acc=2),
               q(cols=0), q(h=0), q(cap=0), q(cap_h=0), q(pub=0), q(q=0)):
        _refused(fn, bufs["q"])
    p = bparams([log_n] * 3, [W, HC, 2], CAP_H, lb, 2, 2, 2)
    proof, caps, ok = _sentinel(bm.layout(p)["words"]), _sentinel(3 * 16), _sentinel(2)
    v = lambda kt=0, kh=1, pp=p, u=ptr["pub"]: (lambda: ctx.air_sha512_link_verify_device(pp, kt, kh, caps.data_ptr(), proof.data_ptr(), u, ok.data_ptr(), 0))
    for fn in (v(kh=0), v(kh=2), v(kt=1, kh=2), v(u=None), v(pp=bparams([log_n] * 3, [W, HC + 1, 2], CAP_H, lb, 2, 2, 2)),
               v(pp=bparams([log_n] * 3, [W, HC, 3], CAP_H, lb, 2, 2, 2)), v(pp=bparams([log_n, log_n, log_n + 1], [W, HC, 2], CAP_H, lb, 2, 2, 2))):
        _refused(fn, ok)
