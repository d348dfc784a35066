"""The public table and the helper oracle of the SHA-256 tables' link to Level-1 (include/tmx.h "the SHA-256 tables' link to Level-1",
constraint set 6): tmx_air_sha256_public_shape, tmx_air_sha256_public_device, tmx_air_sha256_link_helper_device,
tmx_air_sha256_link_quotient_device / _range_device, tmx_air_sha256_link_verify_device, tmx_trace_commit_set_air_sha256_link_device.  The yardstick is tests/sha_public_model.py on
top of tests/batch_model.py: device words must equal the model's word for word and every verdict of the device verifier must equal the
model verifier's.  The CPU part ties the model to the claim: the public table
is built from the ELEMENT rows only (Level 1: H and D) and equals, for every block of T.3, T.5 and T.6, what the trace rows say -- the
sixteen message words, IV plus the last-round states written out with plain integers, the liveness pattern -- and hashlib.sha256 of the
reassembled messages; all 50 constraints hold on those rows as integer identities.  The fixtures are those of tests/test_sha_air.py
(the same workloads and seeds) with the oracle's element rows beside them."""
import hashlib

import numpy as np
import pytest

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha_init_model as si
import sha_public_model as sp
import test_sha_air as tsa
import test_sha_init as tsi
from batch_model import bparams
from test_fri import _down, _sentinel, _shift, _up
from test_merkle_open import _section_geom
from test_sha_air import ctx  # noqa: F401  (fixture)
from test_sha_air import _guarded, _refused

SHA256, TREE, HEADER = 4, 16, 32
P = fm.P
W, PW, HC = sp.WIDTH, sp.PUB_WIDTH, sp.HELPER_COLS
CID, SKIP_MAX = b"celestia", 100800
PER = {SHA256: 1, TREE: 2, HEADER: 2}  # blocks of the table per hash


def _workload(kind, n, n_proofs, seed):
    from tendermintx_amd.synth import Workload
    return Workload(kind, n, n_proofs, n, chain_id=CID, seed=seed, signed_permille=900)


def _records(wl, kind, n, p):
    return (wl.proofs[p * 2336:(p + 1) * 2336], wl.targets[p * n * 256:(p + 1) * n * 256],
            wl.trusteds[p * n * 48:(p + 1) * n * 48] if kind == 0 else None)


def _fixture(oracle, kind, n, n_proofs, seed):
    """(kind, n, {section: pre-LDE columns [9 n_proofs][2^log_rows]}, element rows, {section: model public table})"""
    wl = _workload(kind, n, n_proofs, seed)
    fulls, elems = [], []
    for p in range(n_proofs):
        pr, t, r = _records(wl, kind, n, p)
        fulls.append(oracle.trace(kind, pr, t, r, n))
        elems.append(oracle.witness(kind, pr, t, r, CID, SKIP_MAX)[0])
    tables, pubs = {}, {}
    for sec in (SHA256, TREE, HEADER):
        off, rows, width = _section_geom(kind, n, sec)
        assert width == W and rows % 64 == 0
        cols = np.zeros((n_proofs * W, 1 << max(6, (rows - 1).bit_length())), dtype=np.uint64)
        for p, full in enumerate(fulls):
            cols[p * W:(p + 1) * W, :rows] = full[off:off + rows * W].reshape(rows, W).T
        tables[sec] = cols
        pubs[sec] = sp.public_table(kind, n, sec, elems, (cols.shape[1] // 64).bit_length() - 1)
    return kind, n, tables, elems, pubs


@pytest.fixture(scope="module")
def skip4(oracle):
    return _fixture(oracle, 0, 4, 2, 8100)


@pytest.fixture(scope="module")
def step2(oracle):
    return _fixture(oracle, 1, 2, 2, 8200)


@pytest.fixture(scope="module")
def step3(oracle):
    return _fixture(oracle, 1, 3, 2, 8300)


# ---- CPU: the model against the claim
def test_public_table_from_the_element_rows_is_what_the_rows_hash(skip4, step2, step3):
    """the link itself.  For every block of T.3, T.5 and T.6 of skip N = 4, step N = 2 and step N = 3, two proofs each, the table gathered
    from the ELEMENT rows holds: w[k][t] = the table's W at row 64 k + t; dig = IV + the last-round state of the hash's last live block
    (through the chaining value of a two-block hash), plain integers; new / chn = the liveness pattern of the rows; every digest also equals
    hashlib.sha256 of the reassembled message.  Start blocks, chained blocks, zero blocks and live first blocks followed by a zero second
    block all occur, in the counts tests/test_sha_init.py prints for the same workloads"""
    n_start = n_chained = n_zero = n_live_zero = n_hashlib = 0
    for name, (kind, n, tables, elems, pubs) in (("skip4", skip4), ("step2", step2), ("step3", step3)):
        for sec, table in tables.items():
            pub, per, K = pubs[sec], PER[sec], table.shape[1] // 64
            assert pub.shape == (PW * len(elems), K) and int(pub.max()) < 1 << 32
            for p, row in enumerate(elems):
                t, u = table[p * W:(p + 1) * W], pub[p * PW:(p + 1) * PW]
                live = t.reshape(W, -1, 64).any(axis=(0, 2))
                second = np.arange(K) % per == 1
                assert np.array_equal(u[sp.PW_NEW], (live & ~second).astype(np.uint64)), (name, sec, p)
                assert np.array_equal(u[sp.PW_CHN], (live & second).astype(np.uint64)), (name, sec, p)
                n_start, n_chained, n_zero = n_start + int((live & ~second).sum()), n_chained + int((live & second).sum()), n_zero + int((~live).sum())
                if per == 2:
                    n_live_zero += int((live[0::2] & ~live[1::2]).sum())
                for k in range(K):
                    assert [int(x) for x in u[sp.PW_W:sp.PW_W + 16, k]] == [int(x) for x in t[0, 64 * k:64 * k + 16]], (name, sec, p, k)
                    if not live[k]:
                        assert not u[:, k].any()
                        continue
                    is_last = not (per == 2 and not second[k] and live[k + 1])
                    cv = sp.IV if not second[k] else [(v + int(s)) & sp.MASK for v, s in zip(sp.IV, t[1:, 64 * k - 1])]
                    digest = [(c + int(s)) & sp.MASK for c, s in zip(cv, t[1:, 64 * k + 63])]
                    assert [int(x) for x in u[sp.PW_DIG:sp.PW_DIG + 8, k]] == (digest if is_last else [0] * 8), (name, sec, p, k)
                msgs = sp.messages(kind, n, sec, row)
                assert per * len(msgs) <= K
                for i, m in enumerate(msgs):
                    if m is None:
                        assert not live[per * i:per * i + per].any()
                        continue
                    k = per * i + (1 if len(m) + 9 > 64 else 0)
                    want = hashlib.sha256(m).digest()
                    assert b"".join(int(x).to_bytes(4, "big") for x in u[sp.PW_DIG:sp.PW_DIG + 8, k]) == want, (name, sec, p, i)
                    n_hashlib += 1
    print(f"\n[sha-link] start blocks {n_start}, chained blocks {n_chained}, zero blocks {n_zero}, live first blocks before a zero second block "
          f"{n_live_zero}; {n_hashlib} digests against hashlib")
    assert (n_start, n_chained, n_zero, n_live_zero) == (184, 134, 146, 24) and n_hashlib == n_start


def test_rows_satisfy_the_constraints_as_integers(skip4, step2, step3):
    """all 50 constraints hold as integer identities (no reduction mod p) on T.3, T.5 and T.6 of the three workloads, rows cyclic; every
    helper value is below 2^32; CD = 1 occurs; dead blocks, promoted slots, unused second blocks and the zero padding satisfy them with
    their flags clear"""
    carries = 0
    for name, (kind, n, tables, elems, pubs) in (("skip4", skip4), ("step2", step2), ("step3", step3)):
        for sec, table in tables.items():
            n_proofs = len(elems)
            help_ = sp.helper(table, pubs[sec], n_proofs)
            assert help_.shape == (n_proofs * HC, table.shape[1]) and int(help_.max()) < 1 << 32
            for p in range(n_proofs):
                res = sp.integer_residuals(table[p * W:(p + 1) * W], help_[p * HC:(p + 1) * HC], pubs[sec][p * PW:(p + 1) * PW])
                assert len(res) == sp.CONSTRAINTS - 1 + 16
                for j, c in enumerate(res):
                    assert not c.any(), (name, sec, p, j, np.flatnonzero(c)[:4])
                carries += int(help_[p * HC + sp.HCD:p * HC + sp.HCD + 8].sum())
                dead = ~table[p * W:(p + 1) * W].reshape(W, -1, 64).any(axis=(0, 2))
                assert not help_[p * HC:p * HC + sp.HCHN].reshape(sp.HCHN, -1, 64)[:, dead].any()
    assert carries


def test_a_changed_word_breaks_an_integer_identity(step3):
    """the residuals see what set 6 is for: one changed public w word, digest word, new or chn flag, a table W word among the first sixteen
    of a block, and a last-round state each leave some constraint non-zero -- the helper regenerated from the changed inputs"""
    kind, n, tables, elems, pubs = step3
    table, pub = tables[TREE][:W].copy(), pubs[TREE][:PW].copy()
    live = np.flatnonzero(pub[sp.PW_CHN])
    k = int(live[0])  # a chained block: its digest is set, block k - 1 starts the hash
    broken = lambda t, u: any(c.any() for c in sp.integer_residuals(t, sp.helper(t, u, 1), u))
    assert not broken(table, pub)
    for col, kk in ((sp.PW_W + 5, k), (sp.PW_DIG + 2, k), (sp.PW_NEW, k - 1), (sp.PW_CHN, k)):
        bad = pub.copy()
        bad[col, kk] ^= np.uint64(1)
        assert broken(table, bad), (col, kk)
    for c, r in ((0, 64 * k + 5), (3, 64 * k + 63), (3, 64 * k - 1)):
        bad = table.copy()
        bad[c, r] ^= np.uint64(1 << 9)
        assert broken(bad, pub), (c, r)
    bad = table.copy()
    bad[0, 64 * k + 16] ^= np.uint64(1)  # (W_16 is the schedule's: set 4, not this set)
    assert not broken(bad, pub)


LB = 2  # blow-up 4 in the CPU tests
CAP_H = 2


def _model_quotient(oracle, table, help_, pub, log_blowup=LB):
    """(extended table, extended helper, gamma, planar quotient) of pre-LDE columns and a public table"""
    n_proofs, log_n = table.shape[0] // W, table.shape[1].bit_length() - 1 + log_blowup
    ext, hext = oracle.lde(table, log_blowup), oracle.lde(help_, log_blowup)
    g = sp.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, tsa._cap(oracle, ext, log_n), tsa._cap(oracle, hext, log_n), pub)
    return ext, hext, g, sp.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, pub, _shift(), g)


@pytest.mark.parametrize("which", ["T.3 of skip N = 4", "T.5 of step N = 3"])
def test_quotient_is_a_polynomial_of_degree_below_n(oracle, skip4, step3, which):
    """two proofs, blow-up 4: the model quotient of the honest tables under the public table from the element rows interpolates to degree
    < N in both planes (N - 2 expected), and the identity holds at a zeta outside the base field; it fails after bumping u_0, a table
    opening, a helper opening on either side, or one public word.  The seventeen barycentric sums are the interpolants the quotient
    used: PQ(zeta) equals Horner on the coefficients"""
    fx, sec = (skip4, SHA256) if which.startswith("T.3") else (step3, TREE)
    table, pub = fx[2][sec], fx[4][sec]
    N = table.shape[1]
    assert N == 512
    log_n, n_proofs = N.bit_length() - 1 + LB, table.shape[0] // W
    help_ = sp.helper(table, pub, n_proofs)
    ext, hext, g, quot = _model_quotient(oracle, table, help_, pub)
    deg = tsa._degrees(oracle, quot)
    print(f"\n[sha-link] {which}: N = {N}, quotient degrees {deg}")
    assert max(deg) < N and g[1] != 0
    M = 1 << log_n
    zeta = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)
    zs = (zeta, fm.e_scale(zeta, oracle.gl_root(log_n - LB)))
    yt, yh = dm.evaluate(oracle, table, 1, zs), dm.evaluate(oracle, help_, 1, zs)
    u = [am.horner(am.coefficients(oracle, quot[k * M:(k + 1) * M], _shift()), zeta) for k in (0, 1)]
    t0, t1, h0, h1 = [tuple(y[0]) for y in yt], [tuple(y[1]) for y in yt], [tuple(y[0]) for y in yh], [tuple(y[1]) for y in yh]
    ident = lambda t0=t0, t1=t1, h0=h0, h1=h1, u0=u[0], pub=pub: sp.identity_at(oracle, log_n, LB, n_proofs, t0, t1, h0, h1, u0, u[1], zeta, g, pub)
    assert ident()
    assert not ident(u0=fm.e_add(u[0], (1, 0)))
    bump = lambda v, at: v[:at] + [fm.e_add(v[at], (0, 1))] + v[at + 1:]
    assert not ident(t0=bump(t0, W + 4)) and not ident(t0=bump(t0, 0))
    assert not ident(h0=bump(h0, sp.HDG + 7)) and not ident(h1=bump(h1, HC + sp.HCV + 2))
    for col, k in ((sp.PW_W + 9, 1), (sp.PW_DIG + 1, 0), (PW + sp.PW_NEW, 0), (sp.PW_CHN, 1)):
        bad = pub.copy()
        bad[col, k] ^= np.uint64(1)
        assert not ident(pub=bad), (col, k)
    V = sp.combine(pub, g)
    want = (0, 0)
    K, om = len(V[0]), sp.omega(oracle, log_n, LB)
    zk = dm.e_pow(zeta, K)
    for v, off in zip(V, sp.OFFSETS):
        c = sp.coefficients(oracle, log_n, LB, v, off)
        pz = fm.e_add(am.horner(c[0], zeta), fm.e_mul((0, 1), am.horner(c[1], zeta)))
        want = fm.e_add(want, fm.e_mul(pz, dm.e_inv(((zk[0] - pow(om, off * K, P)) % P, zk[1]))))
    assert sp.public_at(oracle, log_n, LB, pub, g, zeta) == want


RERUN_W5, ZERO_SECOND = tsi.RERUN_W5, "T.5: a live second block replaced by zeros, the helper regenerated"
DETECTED = [RERUN_W5, ZERO_SECOND, "one changed public w word", "one changed digest word", "a flipped new", "a flipped chn",
            "a flipped CD bit on a digest row", "a changed CV_3 mid-block"]


def _tampered(skip4, step3, kind):
    """(honest table, table, helper, public table, whether the table changed) of ONE proof after a single change of `kind`: the two table
    tamperings tests/test_sha_init.py records as unseen (its own rows), else T.5 of step N = 3"""
    if kind == RERUN_W5:
        table, pub = skip4[2][SHA256][:W], skip4[4][SHA256][:PW]
        t = tsi._tampered(table, None, kind)[0]
        return table, t, sp.helper(t, pub, 1), pub, True
    table, pub = step3[2][TREE][:W], step3[4][TREE][:PW].copy()
    if kind == ZERO_SECOND:
        t = tsi._tampered(None, table, kind)[0]
        return table, t, sp.helper(t, pub, 1), pub, True
    k = int(np.flatnonzero(pub[sp.PW_CHN])[0])  # a chained block: block k - 1 starts its hash, the digest stands on block k
    if kind.startswith("one changed") or kind.startswith("a flipped n") or kind.startswith("a flipped chn"):
        col, kk = {"one changed public w word": (sp.PW_W + 5, k), "one changed digest word": (sp.PW_DIG + 2, k), "a flipped new": (sp.PW_NEW, k - 1),
                   "a flipped chn": (sp.PW_CHN, k)}[kind]
        pub[col, kk] ^= np.uint64(1)
        return table, table, sp.helper(table, pub, 1), pub, False  # (the helper from the changed flags: the prover's best)
    h = sp.helper(table, pub, 1)
    if kind == "a flipped CD bit on a digest row":
        h[sp.HCD + 2, 64 * k + 63] ^= np.uint64(1)
    elif kind == "a changed CV_3 mid-block":
        h[sp.HCV + 3, 64 * k + 29] += np.uint64(1)
    else:
        raise KeyError(kind)
    return table, table, h, pub, False


@pytest.mark.parametrize("kind", DETECTED)
def test_one_change_breaks_the_degree(oracle, skip4, step3, kind):
    """the detected kinds (one proof, blow-up 4): the quotient no longer interpolates to degree < N.  The first two are the holes
    tests/test_sha_init.py records -- the rows come from its `_tampered` -- and the model quotients of sets 3, 4 and 5 of the same rows
    stay below N.  NOT seen by sets 3 - 6 together, recorded here so that nobody mistakes the claim: LIVE / LV of sets 3 and 5 against
    the public flags (a block that set 6 holds live and sets 3 and 5 hold dead is constrained by neither side's round or start
    constraints); SHA-512; the ladders' curve arithmetic and limb ranges; a T.5 slot whose right child is not enabled (Level-1 holds L
    there, not the hash: the honest rows do not link); and there is no range argument for DG on chain rows -- the identities are
    integer identities far below p and the digest is pinned to a public word below 2^32, so the digest is right mod 2^32 provided set 3
    range-checks s_j"""
    table, t, h, pub, table_changed = _tampered(skip4, step3, kind)
    N = table.shape[1]
    assert np.array_equal(t, table) != table_changed
    deg = tsa._degrees(oracle, _model_quotient(oracle, t, h, pub)[3])
    print(f"\n[sha-link] {kind}: quotient degrees {deg}, N = {N}")
    assert max(deg) >= N
    if table_changed:
        assert kind in tsi.UNDETECTED and (t != table).sum() > 8
        chain = 0 if kind == RERUN_W5 else 1
        d5 = max(tsa._degrees(oracle, tsi._model_quotient(oracle, t, si.helper(t, 1, chain), chain)[3]))
        d3, d4 = tsi._degrees_under_sets_3_and_4(oracle, t)
        print(f"[sha-link] the same rows under set 3: degree {d3}, set 4: {d4}, set 5: {d5}")
        assert max(d3, d4, d5) < N


def test_model_uint64_path_equals_python_integers_and_pieces_add_up(oracle):
    """one whole quotient of random columns (three proofs, N = 128, blow-up 2) through the uint64 field and through Python integers; the
    pieces [0, 2) + [2, 3) and, in the other order, [1, 3) + [0, 1) add up to the whole mod p"""
    rng = np.random.default_rng(11900)
    n_proofs, log_n, lb = 3, 8, 1
    ext = rng.integers(0, 1 << 64, (n_proofs * W, 256), dtype=np.uint64)
    hext = rng.integers(0, 1 << 64, (n_proofs * HC, 256), dtype=np.uint64)
    pub = rng.integers(0, P, (n_proofs * PW, 2), dtype=np.uint64)
    g = (0x0123456789ABCDEF % P, 0xFEDCBA9876543210 % P)
    q = lambda **kw: sp.quotient(oracle, log_n, lb, n_proofs, ext, hext, pub, _shift(), g, **kw)
    whole = q()
    assert np.array_equal(whole, q(ints=True))
    add = lambda a, b: ((a.astype(object) + b.astype(object)) % P).astype(np.uint64)
    assert np.array_equal(add(q(proofs=range(0, 2)), q(proofs=range(2, 3))), whole)
    assert np.array_equal(add(q(proofs=range(1, 3)), q(proofs=range(0, 1))), whole)


def test_a_slot_with_a_disabled_right_child_does_not_link(oracle):
    """the limit of the T.5 link, pinned: step N = 4 with nb = 3, one proof.  Lane 3 is not enabled, so Level-1 holds L in the slot over
    the leaves 2 and 3 (`both enabled ? hash : L`) while the rows hash the pair: the public digest of that slot -- the slot's node, as the
    gather reads it -- is the left leaf hash and not IV + the last-round state.  The digest constraints 40 .. 47 fail there as integer
    identities on that slot's digest row alone, and the model quotient of the HONEST rows has degree >= N.  The message words link on
    every slot (the slot above hashes its children as Level-1 holds them) and the full slot over the leaves 0 and 1 links.  Set 6 is for
    full trees (nb >= N)"""
    from tendermintx_amd.synth import Workload
    kind, n = 1, 4
    wl = Workload(kind, n, 1, 3, chain_id=CID, seed=8400, signed_permille=900)
    pr, t, r = _records(wl, kind, n, 0)
    full, row = oracle.trace(kind, pr, t, r, n), oracle.witness(kind, pr, t, r, CID, SKIP_MAX)[0]
    off, rows, _ = _section_geom(kind, n, TREE)
    table = np.zeros((W, 512), dtype=np.uint64)
    table[:, :rows] = full[off:off + rows * W].reshape(rows, W).T
    pub = sp.public_table(kind, n, TREE, [row], 3)
    L = sp.Layout(kind, n)
    assert [int(x) for x in pub[sp.PW_DIG:sp.PW_DIG + 8, 3]] == sp._words(row, L.d1a + 1136 * 2 + 368)  # (slot 1's node is leaf 2's hash)
    res = sp.integer_residuals(table, sp.helper(table, pub, 1), pub)
    broken = sorted({j for j, c in enumerate(res) if c.any()})
    print(f"\n[sha-link] nb = 3 of N = 4: residuals broken at {broken}")
    assert set(range(40, 48)) <= set(broken) and not set(broken) & set(range(40))
    assert np.flatnonzero(res[40]).tolist() == [64 * 3 + 63]  # (only the disabled slot's digest row; slot 0 links)
    assert not any(j >= 48 for j in broken)  # (the slot above hashes its children as Level-1 holds them: its message words link)
    deg = tsa._degrees(oracle, _model_quotient(oracle, table, sp.helper(table, pub, 1), pub, 1)[3])
    assert max(deg) >= 512, deg


def test_symbols_and_wrappers_exist(built_lib):
    """the new entry points are in the built library, bound in _lib.py and wrapped in context.py; the shape call against the table
    shapes of tmx_trace_commit_shape, its refusals, and the model's section starts against the library's hint count"""
    from tendermintx_amd import _lib, context
    from tendermintx_amd.context import Context
    from tendermintx_amd._lib import TmxError
    for name in ("tmx_air_sha256_public_shape", "tmx_air_sha256_public_device", "tmx_air_sha256_link_helper_device",
                 "tmx_air_sha256_link_quotient_device", "tmx_air_sha256_link_quotient_range_device", "tmx_air_sha256_link_verify_device",
                 "tmx_trace_commit_set_air_sha256_link_device"):
        assert getattr(built_lib, name).argtypes, name
        if "range" not in name:  # (the range call is the wrapper's proof_range / accumulate path)
            assert callable(getattr(Context, name[4:])), name
    assert (_lib.AIR_SHA256_PUBLIC_WIDTH, _lib.AIR_SHA256_LINK_HELPER_COLS, _lib.AIR_SHA256_LINK_CONSTRAINTS) == (PW, HC, sp.CONSTRAINTS)
    assert (_lib.TRACE_SHA256_LINK_HELPER, _lib.TRACE_SHA256_LINK_QUOTIENT) == (8192, 16384)
    shape = context.air_sha256_public_shape
    assert shape(0, SHA256, 4, 2) == (3, 52) and shape(0, TREE, 4, 2) == (4, 52) and shape(0, HEADER, 4, 1) == (6, 26)
    assert shape(1, SHA256, 3, 2) == (2, 52) and shape(1, TREE, 3, 5) == (3, 130) and shape(1, HEADER, 2, 2) == (6, 52)
    assert shape(0, SHA256, 128, 256) == (8, 26 * 256) and shape(0, TREE, 128, 256) == (9, 26 * 256)
    # refused: no SHA-256 table, a bad kind, no proofs, one block only (T.3 of step N = 1), no tree at N = 1, 33 n_proofs > 2^24
    for args in ((0, 1, 4, 1), (0, 2, 4, 1), (0, 8, 4, 1), (0, 64, 4, 1), (2, SHA256, 4, 1), (0, SHA256, 4, 0), (1, SHA256, 1, 1), (1, TREE, 1, 1),
                 (0, SHA256, 4, (1 << 24) // HC + 1)):
        with pytest.raises(TmxError):
            shape(*args)
    for kind, n in ((0, 4), (1, 3), (0, 128)):
        assert sp.Layout(kind, n).d == int(built_lib.tmx_hint_elem_count(kind, n))


# ---- GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


def _device_rows(c, kind, n, n_proofs, seed):
    """(element rows [P][stride], trace rows [P][elems]) of one synthetic batch, as tmx_witness_batch_device and tmx_trace_rows_device leave
    them on the device"""
    from test_air_boundary import _witness_rows
    return _witness_rows(c, kind, n, n_proofs, seed)


def _gather(c, kind, section, n_proofs, d_rows):
    log_k, n_cols = c.air_sha256_public_shape(kind, section, n_proofs)
    d_pub = _guarded(n_cols << log_k, lambda out: c.air_sha256_public_device(kind, section, n_proofs, d_rows.data_ptr(), out, 0))
    return d_pub, _down(d_pub).reshape(n_cols, 1 << log_k)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [(0, 4), (1, 3)])
def test_gather_equals_the_model(built_lib, kind, n):
    """tmx_air_sha256_public_device on the rows tmx_witness_batch_device left, all three sections of skip N = 4 and step N = 3, two proofs:
    every word equals the model's table built from the same rows, guard words intact; and the link on the device's own rows -- w[k][t] is
    the W of row 64 k + t of the trace rows tmx_trace_rows_device wrote from the context's Level-1 scratch, new / chn their liveness"""
    import tendermintx_amd as tmx
    n_proofs = 2
    with tmx.Context(n, CID, max_batch=n_proofs) as c:
        d_rows, d_trace = _device_rows(c, kind, n, n_proofs, 8100 + n)
        rows, trace = _down(d_rows).reshape(n_proofs, -1), _down(d_trace).reshape(n_proofs, -1)
        for sec in (SHA256, TREE, HEADER):
            _, got = _gather(c, kind, sec, n_proofs, d_rows)
            log_k, n_cols = c.air_sha256_public_shape(kind, sec, n_proofs)
            want = sp.public_table(kind, n, sec, list(rows), log_k)
            assert got.shape == want.shape == (PW * n_proofs, 1 << log_k)
            assert np.array_equal(got, want), (sec, np.argwhere(got != want)[:10])
            off, n_rows, width = _section_geom(kind, n, sec)
            for p in range(n_proofs):
                t = trace[p, off:off + n_rows * W].reshape(n_rows, W)
                blocks = t.reshape(-1, 64, W)
                live = blocks.any(axis=(1, 2))
                u = got[p * PW:(p + 1) * PW]
                assert np.array_equal(u[sp.PW_W:sp.PW_W + 16, :len(blocks)].T, blocks[:, :16, 0]), (sec, p)
                assert np.array_equal((u[sp.PW_NEW] + u[sp.PW_CHN])[:len(blocks)], live.astype(np.uint64)) and not u[:, len(blocks):].any()
                assert live.any() and u[sp.PW_DIG:sp.PW_DIG + 8].any()


def _device_helper(ctx, table, pub):
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    d_table, d_pub = _up(table), _up(pub)
    return _guarded((n_proofs * HC) << log_rows,
                    lambda out: ctx.air_sha256_link_helper_device(log_rows, n_proofs, d_table.data_ptr(), d_pub.data_ptr(), out, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs", [(7, 1), (7, 3), (8, 257), (12, 1)])
def test_helper_of_random_tables_equals_the_model(ctx, log_rows, n_proofs):
    """random 64-bit table words and random flags -- clear, 1, a word whose low 32 bits are zero (clear), a word above 2^32 with low bits
    (set), new and chn both set (new wins): the helper equals the model's word for word, guard words intact.  log_rows 7 is the smallest
    shape (K = 2: the block behind the last is block 0), 257 proofs cross every power-of-two grid edge, log_rows 12 has K = 64"""
    rng = np.random.default_rng(11000 + 100 * log_rows + n_proofs)
    R = 1 << log_rows
    table = rng.integers(0, 1 << 64, (n_proofs * W, R), dtype=np.uint64)
    pub = rng.integers(0, 1 << 32, (n_proofs * PW, R // 64), dtype=np.uint64)
    kinds = np.array([0, 1, 1 << 32, (5 << 32) | 7], dtype=np.uint64)
    for col in (sp.PW_NEW, sp.PW_CHN):
        pub[col::PW] = kinds[rng.integers(0, 4, (n_proofs, R // 64))]
    pub[sp.PW_NEW, :2], pub[sp.PW_CHN, :2] = (1, 0), (0, 1)  # (proof 0 begins with a two-block hash whatever was drawn: CHN = 1, then 0)
    got = _down(_device_helper(ctx, table, pub)).reshape(n_proofs * HC, -1)
    want = sp.helper(table, pub, n_proofs)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    assert int(want.max()) < 1 << 32 and want[sp.HCD::HC].any()
    assert want[sp.HCHN, :64].all() and np.array_equal(want[sp.HCH:sp.HCH + 8, :64], want[sp.HDG:sp.HDG + 8, :64])
    assert not want[sp.HCHN, 64:128].any() and not want[sp.HCH:sp.HCH + 8, 64:128].any()
    assert [int(x) for x in want[sp.HCV:sp.HCV + 8, 64]] == [(v + (int(x) & sp.MASK)) & sp.MASK for v, x in zip(sp.IV, table[1:W, 63])]
    # the wrap on its own: the last block's CHN is chn of block 0 of the SAME proof, block 0's chained CV reads the proof's last row
    for p in (0, n_proofs - 1):
        assert int(want[p * HC + sp.HCHN, R - 1]) == sp._flag(pub[p * PW + sp.PW_CHN, 0])
        if not sp._flag(pub[p * PW + sp.PW_NEW, 0]) and sp._flag(pub[p * PW + sp.PW_CHN, 0]):
            assert int(want[p * HC + sp.HCV + 2, 0]) == (sp.IV[2] + (int(table[p * W + 3, R - 1]) & sp.MASK)) & sp.MASK


@pytest.mark.gpu
def test_helper_of_real_rows_equals_the_model(ctx, step3, skip4):
    """the real T.5 rows of step N = 3 (512 rows with padding, a promoted slot and chained second blocks) and the real T.6 rows of skip
    N = 4 (4096 rows; live first blocks followed by a zero second block) under their own public tables: the model's words, all 50
    constraints on them (the CPU test above) -- and DG on the last row of a hash's last live block is the public digest"""
    for (kind, n, tables, elems, pubs), sec in ((step3, TREE), (skip4, HEADER)):
        table, pub = tables[sec], pubs[sec]
        n_proofs = len(elems)
        got = _down(_device_helper(ctx, table, pub)).reshape(n_proofs * HC, -1)
        assert np.array_equal(got, sp.helper(table, pub, n_proofs))
        for p in range(n_proofs):
            u, h = pub[p * PW:(p + 1) * PW], got[p * HC:(p + 1) * HC]
            ends = np.flatnonzero(u[sp.PW_DIG:sp.PW_DIG + 8].any(axis=0))
            assert ends.size and np.array_equal(h[sp.HDG:sp.HDG + 8, 64 * ends + 63], u[sp.PW_DIG:sp.PW_DIG + 8, ends])


@pytest.mark.gpu
def test_each_validation_rule(ctx):
    """every rule of the two device calls on its own: TMX_ERR_BAD_ARG before anything is enqueued, nothing written"""
    d_table, d_pub, d_help = _sentinel(W << 7), _sentinel(PW << 1), _sentinel(HC << 7)
    hp = lambda lr, n, t=d_table.data_ptr(), u=d_pub.data_ptr(), o=d_help.data_ptr(): (lambda: ctx.air_sha256_link_helper_device(lr, n, t, u, o, 0))
    for fn in (hp(6, 1), hp(19, 1), hp(7, 0), hp(7, (1 << 24) // HC + 1), hp(7, 1, t=None), hp(7, 1, u=None), hp(7, 1, o=None)):
        _refused(fn, d_help)
    rows, pub = _sentinel(16), _sentinel(16)
    g = lambda kind, sec, n, r=rows.data_ptr(), u=pub.data_ptr(): (lambda: ctx.air_sha256_public_device(kind, sec, n, r, u, 0))
    for fn in (g(2, SHA256, 1), g(0, 1, 1), g(0, 2, 1), g(0, 8, 1), g(0, 128, 1), g(0, SHA256 | TREE, 1), g(0, SHA256, 0), g(0, TREE, (1 << 24) // HC + 1),
               g(0, SHA256, 1, r=None), g(0, SHA256, 1, u=None)):
        _refused(fn, pub)


def _device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, d_pub, cap_height=CAP_H, pieces=None):
    """the device quotient between guards; pieces: [(lo, hi)] fed in order, the first written and the others accumulated"""
    a = (log_n, log_blowup, cap_height, n_proofs, d_cols.data_ptr(), d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(), d_pub.data_ptr())

    def run(out):
        if pieces is None:
            ctx.air_sha256_link_quotient_device(*a, out, 0)
        else:
            for k, r in enumerate(pieces):
                ctx.air_sha256_link_quotient_device(*a, out, 0, proof_range=r, accumulate=int(k > 0))
    return _guarded(2 << log_n, run)


@pytest.mark.gpu
@pytest.mark.parametrize("log_k,log_blowup,n_proofs", [(1, 1, 2), (3, 3, 1), (6, 1, 3), (9, 3, 1), (12, 1, 1)])
def test_public_chain_equals_the_model(ctx, oracle, log_k, log_blowup, n_proofs):
    """K = 2, 8, 64, 512 and 2^12 (the LDS limit of the size-K transform), blow-up 2 and 8: gamma with the public digest, V, the seventeen
    coefficient vectors, extensions and their fold, seen through the quotient of all-zero table and helper columns, which is - PQ(x_i)
    exactly: every word equals the model's.  The random public words are canonical; flags of any value: the definition is pointwise"""
    log_n = 6 + log_k + log_blowup
    rng = np.random.default_rng(11100 + 10 * log_k + log_blowup)
    pub = rng.integers(0, P, (PW * n_proofs, 1 << log_k), dtype=np.uint64)
    zt, zh = np.zeros((n_proofs * W, 1 << log_n), dtype=np.uint64), np.zeros((n_proofs * HC, 1 << log_n), dtype=np.uint64)
    d_cols, d_hcols, d_pub = _up(zt), _up(zh), _up(pub)
    _, d_cap = tsa._tree(ctx, d_cols, log_n, n_proofs * W)
    _, d_cap_h = tsa._tree(ctx, d_hcols, log_n, n_proofs * HC)
    got = _down(_device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, d_pub))
    g = sp.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _down(d_cap), _down(d_cap_h), pub)
    assert ctx.air_last_gamma() == g
    pq = sp.public_quotient(oracle, log_n, log_blowup, pub, _shift(), g)
    want = np.array([(P - int(x)) % P for x in pq[0]] + [(P - int(x)) % P for x in pq[1]], dtype=np.uint64)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    other = pub.copy()
    other[5, 1] ^= np.uint64(1)  # (one public word: another digest, another gamma)
    assert sp.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _down(d_cap), _down(d_cap_h), other) != g


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,log_blowup,n_proofs,cap_height", [(7, 1, 1, 0), (7, 3, 3, 2), (10, 2, 1, 2), (10, 1, 3, 2)])
def test_quotient_of_random_columns_equals_the_model(ctx, oracle, log_rows, log_blowup, n_proofs, cap_height):
    """N = 128 (K = 2, the smallest shape) and N = 1024, one and three proofs, random table, helper and public words (a few columns
    non-canonical): the definition is pointwise, so d_quot and gamma equal the model word for word, guard words intact; with three proofs
    also in two pieces in both orders, [0, 2) + [2, 3) and [1, 3) + [0, 1): the same words"""
    log_n = log_rows + log_blowup
    rng = np.random.default_rng(11200 + 100 * log_rows + 10 * log_blowup + n_proofs)
    ext, hext = tsa._random_ext(rng, n_proofs * W, log_n), tsa._random_ext(rng, n_proofs * HC, log_n)
    pub = rng.integers(0, P, (PW * n_proofs, 1 << (log_rows - 6)), dtype=np.uint64)
    d_cols, d_hcols, d_pub = _up(ext), _up(hext), _up(pub)
    _, d_cap = tsa._tree(ctx, d_cols, log_n, n_proofs * W, cap_height)
    _, d_cap_h = tsa._tree(ctx, d_hcols, log_n, n_proofs * HC, cap_height)
    args = (ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, d_pub, cap_height)
    got = _down(_device_quotient(*args))
    g = sp.gamma(oracle, log_n, log_blowup, cap_height, n_proofs, _down(d_cap), _down(d_cap_h), pub)
    assert ctx.air_last_gamma() == g
    want = sp.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, pub, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    if n_proofs == 3:
        d_tail = _up(hext[2 * HC:])  # (a piece's helper columns alone, as the range call takes them)
        for pieces, bufs in (([(0, 2), (2, 3)], (d_hcols, d_tail)), ([(1, 3), (0, 1)], (_up(hext[HC:]), d_hcols))):
            a = (log_n, log_blowup, cap_height, n_proofs, d_cols.data_ptr())
            b = (d_cap.data_ptr(), d_cap_h.data_ptr(), d_pub.data_ptr())

            def run(out, pieces=pieces, bufs=bufs):
                for k, (r, h) in enumerate(zip(pieces, bufs)):
                    ctx.air_sha256_link_quotient_device(*a, h.data_ptr(), *b, out, 0, proof_range=r, accumulate=int(k > 0))
            assert np.array_equal(_down(_guarded(2 << log_n, run)), want), pieces


def _chain(ctx, oracle, table, pub, log_blowup, quot_override=None, n_queries=6):
    """caller-level chain: helper -> LDE -> caps -> quotient -> one batch proof over [table, helper, quotient].  Returns (params, d_caps,
    proof words, extended table, extended helper, quotient words)"""
    import torch
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    log_n = log_rows + log_blowup
    d_help, d_pub = _device_helper(ctx, table, pub), _up(pub)
    d_ext, d_hext = _sentinel((n_proofs * W) << log_n), _sentinel((n_proofs * HC) << log_n)
    ctx.lde_device(log_rows, log_blowup, n_proofs * W, _up(table).data_ptr(), d_ext.data_ptr(), 0)
    ctx.lde_device(log_rows, log_blowup, n_proofs * HC, d_help.data_ptr(), d_hext.data_ptr(), 0)
    d_lv_t, d_cap_t = tsa._tree(ctx, d_ext, log_n, n_proofs * W)
    d_lv_h, d_cap_h = tsa._tree(ctx, d_hext, log_n, n_proofs * HC)
    d_quot = (_device_quotient(ctx, log_n, log_blowup, n_proofs, d_ext, d_hext, d_cap_t, d_cap_h, d_pub) if quot_override is None
              else _up(quot_override))
    d_lv_q, d_cap_q = tsa._tree(ctx, d_quot, log_n, 2)
    p = bparams([log_n] * 3, [n_proofs * W, n_proofs * HC, 2], CAP_H, log_blowup, 2, 2, n_queries)
    proof = _guarded(bm.layout(p)["words"], lambda out: ctx.batch_prove_device(p, [d.data_ptr() for d in (d_ext, d_hext, d_quot)],
                                                                               [d.data_ptr() for d in (d_lv_t, d_lv_h, d_lv_q)], out, 0))
    return (p, torch.cat([d_cap_t, d_cap_h, d_cap_q]), _down(proof), _down(d_ext).reshape(n_proofs * W, -1),
            _down(d_hext).reshape(n_proofs * HC, -1), _down(d_quot))


def _verdicts(ctx, p, k_trace, k_helper, d_caps, proof, pub):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    d_proof, d_pub = _up(proof), _up(pub)  # (both held until the call has run)
    ctx.air_sha256_link_verify_device(p, k_trace, k_helper, d_caps.data_ptr(), d_proof.data_ptr(), d_pub.data_ptr(), ok.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    out = ok.cpu().numpy()
    assert ((out == 0) | (out == 1)).all(), out
    return [bool(x) for x in out]


@pytest.mark.gpu
def test_real_rows_through_the_caller_level_chain(ctx, oracle, step3):
    """helper -> LDE -> caps -> quotient -> tmx_batch_prove_device -> tmx_air_sha256_link_verify_device on the real T.5 rows of step N = 3
    under the public table from the element rows, blow-up 2: the quotient and gamma equal the model's and the quotient has degree < N;
    every verdict equals the model verifier's (all accept); a proof with one bumped table, helper or quotient opening is rejected on every
    query, and so is the honest proof under a public table with one changed word (a w word, a digest word, a flag)"""
    kind, n, tables, elems, pubs = step3
    table, pub, lb = tables[TREE], pubs[TREE], 1
    n_proofs = len(elems)
    p, d_caps, got, ext, hext, quot = _chain(ctx, oracle, table, pub, lb)
    assert ctx.fri_last_degree_ok() is True
    log_n, caps, cw = p["log_n"][0], _down(d_caps), 4 << CAP_H
    assert np.array_equal(hext, oracle.lde(sp.helper(table, pub, n_proofs), lb))
    g = sp.gamma(oracle, log_n, lb, CAP_H, n_proofs, caps[:cw], caps[cw:2 * cw], pub)
    assert np.array_equal(quot, sp.quotient(oracle, log_n, lb, n_proofs, ext, hext, pub, _shift(), g))
    assert max(tsa._degrees(oracle, quot)) < table.shape[1]
    model = sp.verify(oracle, p, 0, 1, caps, got, _shift(), pub)
    assert all(model) and _verdicts(ctx, p, 0, 1, d_caps, got, pub) == model
    L = bm.layout(p)
    RT, RH = 1 << dm.log_r(p["n_cols"][0]), 1 << dm.log_r(p["n_cols"][1])
    for name, at in (("quotient opening", L["off_open"][2] + 1), ("helper opening at zeta", L["off_open"][1] + sp.HDG + 3),
                     ("helper opening at zeta omega", L["off_open"][1] + 2 * RH + HC + sp.HCV + 1),
                     ("table opening at zeta", L["off_open"][0] + 4), ("table W at zeta", L["off_open"][0] + W)):
        bad = got.copy()
        bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
        assert not sp.identity(oracle, p, 0, 1, caps, bad, pub), name
        model = sp.verify(oracle, p, 0, 1, caps, bad, _shift(), pub)
        assert not any(model) and _verdicts(ctx, p, 0, 1, d_caps, bad, pub) == model, name
    k = int(np.flatnonzero(pub[sp.PW_CHN])[0])
    for col, kk in ((sp.PW_W + 5, k), (PW + sp.PW_DIG + 2, k), (sp.PW_NEW, k - 1)):
        other = pub.copy()
        other[col, kk] ^= np.uint64(1)
        model = sp.verify(oracle, p, 0, 1, caps, got, _shift(), other)
        assert not any(model) and _verdicts(ctx, p, 0, 1, d_caps, got, other) == model, (col, kk)


@pytest.mark.gpu
def test_the_rerun_from_w5_is_rejected_and_sets_3_to_5_still_accept_it(ctx, oracle, skip4):
    """the T.3 table re-run from a changed W_5 (the kind tests/test_sha_init.py records as unseen by sets 3 + 4 + 5), one proof, blow-up 4,
    with its HONEST quotients: set 6's chain under the public table from the element rows clears every verdict, as the model does -- the
    quotient is no polynomial of degree < N -- while the chains of sets 3, 4 and 5 over the same rows accept every query"""
    import test_sha_sched as tss
    table, t, h, pub, _ = _tampered(skip4, None, RERUN_W5)
    p, d_caps, got, _, _, quot = _chain(ctx, oracle, t, pub, 2)
    assert max(tsa._degrees(oracle, quot)) >= table.shape[1]
    model = sp.verify(oracle, p, 0, 1, _down(d_caps), got, _shift(), pub)
    assert not any(model) and _verdicts(ctx, p, 0, 1, d_caps, got, pub) == model
    p3, d_caps3, got3, _, _, _ = tsa._chain(ctx, oracle, t, 2)
    assert all(tsa._verdicts(ctx, p3, 0, d_caps3, got3))
    p4, d_caps4, got4, _, _, _ = tss._chain(ctx, oracle, t, 2)
    assert all(tss._verdicts(ctx, p4, 0, 1, d_caps4, got4))
    p5, d_caps5, got5, _, _, _ = tsi._chain(ctx, oracle, t, 0, 2)
    assert all(tsi._verdicts(ctx, p5, 0, 1, 0, d_caps5, got5))


@pytest.mark.gpu
def test_zero_quotient_for_a_tampered_table(ctx, oracle, skip4):
    """a zero (low-degree) quotient committed for the same re-run table: the batch proof is fine and the identity fails -- every verdict is
    cleared by k_air_link_check alone, as in the model"""
    _, t, h, pub, _ = _tampered(skip4, None, RERUN_W5)
    log_n = t.shape[1].bit_length() - 1 + 1
    p, d_caps, got, _, _, _ = _chain(ctx, oracle, t, pub, 1, quot_override=np.zeros(2 << log_n, dtype=np.uint64))
    assert all(tsa._verdicts(ctx, p, 0, d_caps, got, batch_only=True))
    model = sp.verify(oracle, p, 0, 1, _down(d_caps), got, _shift(), pub)
    assert not any(model) and _verdicts(ctx, p, 0, 1, d_caps, got, pub) == model


@pytest.mark.gpu
def test_257_proofs_through_the_check_kernel(ctx, oracle, step3):
    """N = 128, 257 proofs (one more than k_air_link_check has threads: thread 0 takes proofs 0 and 256) -- the two-block hashes of T.5 of
    step N = 3 in turn with their own public blocks, every seventh proof zero with its flags clear --, blow-up 2, two queries: the device
    accepts every query as the model's identity does; one helper opening bumped in proof 256 and a table opening in proof 255 are rejected"""
    kind, n, tables, elems, pubs = step3
    t5, u5, many = tables[TREE], pubs[TREE], 257
    pairs, ppub = [], []
    for p in range(len(elems)):
        for i in range(t5.shape[1] // 128):
            if u5[p * PW + sp.PW_CHN, 2 * i + 1]:
                pairs.append(t5[p * W:(p + 1) * W, 128 * i:128 * i + 128])
                ppub.append(u5[p * PW:(p + 1) * PW, 2 * i:2 * i + 2])
    assert pairs
    table, pub = np.zeros((many * W, 128), dtype=np.uint64), np.zeros((many * PW, 2), dtype=np.uint64)
    for q in range(many):
        if q % 7 != 6:
            table[q * W:(q + 1) * W], pub[q * PW:(q + 1) * PW] = pairs[q % len(pairs)], ppub[q % len(pairs)]
    p, d_caps, got, ext, hext, _ = _chain(ctx, oracle, table, pub, 1, n_queries=2)
    assert ctx.fri_last_degree_ok() is True
    caps = _down(d_caps)
    assert sp.identity(oracle, p, 0, 1, caps, got, pub)
    assert _verdicts(ctx, p, 0, 1, d_caps, got, pub) == [True, True]
    L = bm.layout(p)
    for at in (L["off_open"][1] + 256 * HC + sp.HDG + 3, L["off_open"][0] + 255 * W + 4):
        bad = got.copy()
        bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
        assert not sp.identity(oracle, p, 0, 1, caps, bad, pub)
        assert _verdicts(ctx, p, 0, 1, d_caps, bad, pub) == [False, False]


@pytest.mark.gpu
def test_each_validation_rule_of_the_quotient_and_the_verifier(ctx):
    """every rule of the quotient calls and of the verifier on its own: TMX_ERR_BAD_ARG before anything is enqueued, nothing written.
    7 <= log_n - log_blowup <= 18 as set 2 restricts its K; 33 n_proofs <= 2^24; a range inside n_proofs; accumulate <= 1; no null pointer;
    the verifier: column counts 9 k / 33 k / 2, equal log_n, k_trace < k_helper, k_helper + 1 inside the proof, d_pub set"""
    import torch
    log_n, lb = 8, 1
    d_cols, d_hcols, d_pub = _sentinel(W << log_n), _sentinel(HC << log_n), _sentinel(PW << 1)
    d_cap, d_cap_h, d_quot = _sentinel(4 << CAP_H), _sentinel(4 << CAP_H), _sentinel(2 << log_n)
    ptrs = [d_cols.data_ptr(), d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(), d_pub.data_ptr(), d_quot.data_ptr()]
    q = lambda ln, b, n, a=ptrs, **kw: (lambda: ctx.air_sha256_link_quotient_device(ln, b, CAP_H, n, *a, 0, **kw))
    for fn in (q(log_n, 0, 1), q(log_n, 7, 1), q(2, 2, 1), q(29, 2, 1), q(7, 1, 1), q(6, 1, 1), q(20, 1, 1), q(log_n, lb, 0), q(log_n, lb, (1 << 24) // HC + 1),
               q(log_n, lb, 2, proof_range=(1, 1)), q(log_n, lb, 2, proof_range=(1, 3)), q(log_n, lb, 2, proof_range=(0, 1), accumulate=2)):
        _refused(fn, d_quot)
    for k in range(6):
        _refused(q(log_n, lb, 1, ptrs[:k] + [None] + ptrs[k + 1:]), d_quot)
    ok, caps, proof = torch.full((4,), 7, dtype=torch.int32, device=_dev()), _sentinel(256), _sentinel(1 << 16)
    v = lambda p, kt, kh, u=d_pub.data_ptr(): (lambda: ctx.air_sha256_link_verify_device(p, kt, kh, caps.data_ptr(), proof.data_ptr(), u, ok.data_ptr(), 0))
    good = bparams([8, 8, 8], [W, HC, 2], CAP_H, lb, 2, 2, 4)
    for p, kt, kh in ((good, 0, 2), (good, 0, 0), (good, 1, 1), (good, 1, 0), (dict(good, n_cols=[W + 1, HC, 2]), 0, 1),
                      (dict(good, n_cols=[W, HC + 1, 2]), 0, 1), (dict(good, n_cols=[W, 315, 2]), 0, 1), (dict(good, n_cols=[2 * W, HC, 2]), 0, 1),
                      (dict(good, n_cols=[W, HC, 3]), 0, 1), (dict(good, log_n=[8, 8, 7]), 0, 1), (dict(good, log_n=[8, 7, 8]), 0, 1),
                      (bparams([7, 7, 7], [W, HC, 2], CAP_H, lb, 2, 2, 4), 0, 1), (dict(good, arity_bits=0), 0, 1),
                      (bparams([8, 8], [W, HC], CAP_H, lb, 2, 2, 4), 0, 1)):
        _refused(v(p, kt, kh), ok)
    assert "d_pub" in _refused(v(good, 0, 1, u=None), ok)


# ---- the set level
H5, Q5, H6, Q6 = 2048, 4096, 8192, 16384


@pytest.fixture(scope="module")
def header_sets(built_lib, oracle):
    """a set SHA256 + HEADER at step N = 2, two proofs, three ways: set 6 alone on HEADER, then sets 5 and 6 in the call orders 5-6 and
    6-5.  Per way: (params, section_of, caps of every oracle in order, proof words, verdicts, gammas); and the public table the device
    gathered from the element rows of the same batch"""
    import torch
    import tendermintx_amd as tmx
    kind, n, n_proofs, lb = 1, 2, 2, 1
    cw = 4 << CAP_H
    out = {}
    with tmx.Context(n, CID, max_batch=n_proofs) as c:
        d_rows, tr = _device_rows(c, kind, n, n_proofs, 9300)
        d_pub, pub = _gather(c, kind, HEADER, n_proofs, d_rows)
        out["pub"], out["traces"] = pub, _down(tr).reshape(n_proofs, -1)
        calls = {"5": lambda h, q: c.trace_commit_set_air_sha256_init_device(HEADER, h, q, 0),
                 "6": lambda h, q: c.trace_commit_set_air_sha256_link_device(HEADER, d_pub.data_ptr(), h, q, 0)}
        for way in ("6", "56", "65"):
            d_caps = _sentinel(2 * cw)
            c.trace_commit_set_device(kind, n_proofs, SHA256 | HEADER, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
            pair, gammas = {}, {}
            for s in way:
                pair[s] = (_sentinel(cw), _sentinel(cw))
                calls[s](pair[s][0].data_ptr(), pair[s][1].data_ptr())
                gammas[s] = c.air_last_gamma()
            shape, order = c.trace_commit_set_shape()
            p = dict(shape, arity_bits=2, final_log_max=2, n_queries=6, pow_bits=0)
            proof = _guarded(bm.layout(p)["words"], lambda o: c.trace_commit_set_prove_device(p, o, 0))
            assert c.fri_last_degree_ok() is True
            all_caps = torch.cat([d_caps[:cw]] + [x for s in sorted(way) for x in pair[s]] + [d_caps[cw:]])
            k6 = order.index(H6)
            got = _down(proof)
            v = dict(link=_verdicts(c, p, 0, k6, all_caps, got, pub), batch=tsa._verdicts(c, p, 0, all_caps, got, batch_only=True))
            if "5" in way:
                v["init"] = tsi._verdicts(c, p, 0, order.index(H5), 1, all_caps, got)
            bad = got.copy()
            at = bm.layout(p)["off_open"][k6 + 1]
            bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
            v["bad"] = _verdicts(c, p, 0, k6, all_caps, bad, pub)
            other = pub.copy()
            other[sp.PW_W + 3, 0] ^= np.uint64(1)
            v["other_pub"] = _verdicts(c, p, 0, k6, all_caps, got, other)
            if way == "6":  # the model's helper cap through the device's tree, as tests/test_sha_init.py does
                off, rows, _ = _section_geom(kind, n, HEADER)
                table = np.zeros((n_proofs * W, 1 << 12), dtype=np.uint64)
                for q, full in enumerate(out["traces"]):
                    table[q * W:(q + 1) * W, :rows] = full[off:off + rows * W].reshape(rows, W).T
                hext = oracle.lde(sp.helper(table, pub, n_proofs), lb)
                out["cap_h_model"] = _down(tsa._tree(c, _up(hext), 12 + lb, n_proofs * HC)[1])
            out[way] = dict(p=p, order=order, caps=_down(all_caps), proof=got, verdicts=v, gammas=gammas)
    return out


@pytest.mark.gpu
def test_set_level_with_set_6_alone(oracle, header_sets):
    """three oracles behind each other -- section_of ends 32, 8192, 16384 with SHA256 behind --, the helper's cap (the model's helper of the
    device's rows and the gathered public table) and gamma against the model, the device verifier and the model's on the proof over the
    four oracles (all accept; a bumped quotient opening and a changed public word reject), tmx_batch_verify_device against
    tests/batch_model.py"""
    s, lb, n_proofs, cw, pub = header_sets["6"], 1, 2, 4 << CAP_H, header_sets["pub"]
    assert s["order"] == [HEADER, H6, Q6, SHA256]
    assert s["p"]["log_n"] == [12 + lb] * 3 + [7 + lb] and s["p"]["n_cols"] == [W * n_proofs, HC * n_proofs, 2, W * n_proofs]
    caps = s["caps"]
    assert np.array_equal(caps[cw:2 * cw], header_sets["cap_h_model"])
    assert s["gammas"]["6"] == sp.gamma(oracle, 12 + lb, lb, CAP_H, n_proofs, caps[:cw], caps[cw:2 * cw], pub)
    assert s["verdicts"]["batch"] == bm.verify(oracle, s["p"], caps, s["proof"], _shift())
    model = sp.verify(oracle, s["p"], 0, 1, caps, s["proof"], _shift(), pub)
    assert all(model) and s["verdicts"]["link"] == model
    assert not any(s["verdicts"]["bad"]) and not any(s["verdicts"]["other_pub"])


@pytest.mark.gpu
def test_set_level_in_both_orders_with_set_5(oracle, header_sets):
    """the call orders 5-6 and 6-5 both end as table, H5, Q5, H6, Q6, SHA256: the same section_of, the same caps, gammas and proof word
    for word; set 6's caps are those of the set with set 6 alone; the set-5 and set-6 device verifiers accept that proof, both model
    identities hold, and tmx_batch_verify_device equals tests/batch_model.py"""
    a, b, alone, cw, pub = header_sets["56"], header_sets["65"], header_sets["6"], 4 << CAP_H, header_sets["pub"]
    assert a["order"] == b["order"] == [HEADER, H5, Q5, H6, Q6, SHA256]
    assert a["p"] == b["p"] and a["p"]["n_cols"][:5] == [2 * W, 2 * si.HELPER_COLS, 2, 2 * HC, 2]
    assert np.array_equal(a["caps"], b["caps"]) and np.array_equal(a["proof"], b["proof"]) and a["gammas"] == b["gammas"]
    assert np.array_equal(a["caps"][3 * cw:5 * cw], alone["caps"][cw:3 * cw]) and a["gammas"]["6"] == alone["gammas"]["6"]
    for s in (a, b):
        v = s["verdicts"]
        assert all(v["link"]) and all(v["init"]) and all(v["batch"]) and not any(v["bad"]) and not any(v["other_pub"])
    assert a["verdicts"]["batch"] == bm.verify(oracle, a["p"], a["caps"], a["proof"], _shift())
    assert sp.identity(oracle, a["p"], 0, 3, a["caps"], a["proof"], pub) and si.identity(oracle, a["p"], 0, 1, 1, a["caps"], a["proof"])


@pytest.mark.gpu
def test_set_level_refusals(built_lib):
    """before a set, a section that is no SHA-256 table, an absent section, null pointers, a second call (behind the table and behind set
    5's pair), a set with no room for two more oracles -- a section that carries sets 3 + 4 + 5 has seven oracles: the 8-oracle refusal
    --, a streamed member: TMX_ERR_BAD_ARG, nothing written, the set's shape as it was"""
    import tendermintx_amd as tmx
    kind, n, n_proofs, lb = 1, 2, 2, 1
    cw = 4 << CAP_H
    with tmx.Context(n, CID, max_batch=n_proofs) as c:
        d_rows, tr = _device_rows(c, kind, n, n_proofs, 9300)
        pubs = {sec: _gather(c, kind, sec, n_proofs, d_rows)[0] for sec in (SHA256, HEADER)}
        d_caps, d_cap_h, d_cap_q = _sentinel(2 * cw), _sentinel(cw), _sentinel(cw)
        link = lambda sec, u=None: (lambda: c.trace_commit_set_air_sha256_link_device(sec, (u or pubs.get(sec, pubs[HEADER])).data_ptr(),
                                                                                       d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0))
        assert "no commit set" in _refused(link(HEADER), d_cap_h, d_cap_q)
        c.trace_commit_set_device(kind, n_proofs, SHA256 | HEADER, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        before = c.trace_commit_set_shape()
        for sec in (TREE, 1, H5, H6, Q6, 0):
            _refused(link(sec), d_cap_h, d_cap_q)
        u = pubs[HEADER].data_ptr()
        _refused(lambda: c.trace_commit_set_air_sha256_link_device(HEADER, None, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0), d_cap_h, d_cap_q)
        _refused(lambda: c.trace_commit_set_air_sha256_link_device(HEADER, u, None, d_cap_q.data_ptr(), 0), d_cap_q)
        _refused(lambda: c.trace_commit_set_air_sha256_link_device(HEADER, u, d_cap_h.data_ptr(), None, 0), d_cap_h)
        assert c.trace_commit_set_shape() == before
        a, b = _sentinel(cw), _sentinel(cw)
        c.trace_commit_set_air_sha256_link_device(SHA256, pubs[SHA256].data_ptr(), a.data_ptr(), b.data_ptr(), 0)
        assert c.trace_commit_set_shape()[1] == [HEADER, SHA256, H6, Q6]
        assert "already" in _refused(link(SHA256), d_cap_h, d_cap_q)
        c.trace_commit_set_air_sha256_init_device(SHA256, a.data_ptr(), b.data_ptr(), 0)
        assert c.trace_commit_set_shape()[1] == [HEADER, SHA256, H5, Q5, H6, Q6]
        assert "already" in _refused(link(SHA256), d_cap_h, d_cap_q)
        c.trace_commit_set_air_sha256_sched_device(SHA256, a.data_ptr(), b.data_ptr(), 0)
        assert len(c.trace_commit_set_shape()[1]) == 8
        assert "room" in _refused(link(HEADER), d_cap_h, d_cap_q)  # (eight oracles: a full set)
        # sets 3 + 4 + 5 on one section are seven oracles: set 6's pair is refused by the same rule
        c.trace_commit_set_device(kind, n_proofs, HEADER, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        for call in (c.trace_commit_set_air_sha256_device, c.trace_commit_set_air_sha256_sched_device, c.trace_commit_set_air_sha256_init_device):
            call(HEADER, a.data_ptr(), b.data_ptr(), 0)
        assert len(c.trace_commit_set_shape()[1]) == 7
        assert "room" in _refused(link(HEADER), d_cap_h, d_cap_q)
        c.trace_commit_set_streamed_device(kind, n_proofs, SHA256 | HEADER, HEADER, 8, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        assert "streamed" in _refused(link(HEADER), d_cap_h, d_cap_q)
