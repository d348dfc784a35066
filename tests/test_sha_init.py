"""The block starts of the SHA-256 tables (include/tmx.h "the block starts of the SHA-256 tables", constraint set 5):
tmx_air_sha256_init_helper_device, tmx_air_sha256_init_quotient_device, tmx_air_sha256_init_verify_device,
tmx_trace_commit_set_air_sha256_init_device.  The yardstick is tests/sha_init_model.py on top of tests/batch_model.py: device words must
equal the model's word for word and every verdict of the device verifier must equal the model verifier's.  The CPU part ties the model to
the claim: on the CPU oracle's T.3, T.5 and T.6 rows all 337 constraints hold as integer identities and round 0 from the IV or from the
chaining value is written out with plain integer SHA-256; the quotient is a polynomial of degree < N, and one change of a detected kind --
the re-run from a changed row-0 state that sets 3 and 4 do not see among them -- makes it one of degree >= N; the kinds that sets 3, 4 and
5 together still do NOT see are recorded next to them.  The fixtures and the plumbing are those of tests/test_sha_air.py."""
import numpy as np
import pytest

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha_air_model as sm
import sha_init_model as si
import sha_sched_model as ss
import test_sha_air as tsa
import test_sha_sched as tss
from batch_model import bparams
from test_fri import _down, _sentinel, _shift, _up
from test_sha_air import ctx, skip4, step2, step3  # noqa: F401  (fixtures)
from test_sha_air import _cap, _degrees, _guarded, _random_ext, _refused, _tree

P = fm.P
SHA256, TREE, HEADER = 4, 16, 32
H3, Q3, H4, Q4, H5, Q5 = 128, 256, 512, 1024, 2048, 4096
W, HC, HC3, HC4 = si.WIDTH, si.HELPER_COLS, sm.HELPER_COLS, ss.HELPER_COLS
CAP_H = 2
LB = 2  # blow-up 4 in the CPU tests
CHAIN = {SHA256: 0, TREE: 1, HEADER: 1}  # T.3 hashes are single blocks; T.5 and T.6 hashes are pairs of blocks on 128-row boundaries


def _carries(h):
    return h[si.HCA] + 2 * h[si.HCA + 1] + 4 * h[si.HCA + 2], h[si.HCE] + 2 * h[si.HCE + 1] + 4 * h[si.HCE + 2]


# ---- CPU: the model against the claim
def test_rows_satisfy_the_constraints_as_integers(skip4, step2, step3):
    """all 337 constraints hold as integer identities (no reduction mod p) on T.3, T.5 and T.6 of skip N = 4, step N = 2 and step N = 3,
    rows cyclic: the unselected ones on every row, the start ones on every start row, the chain ones on every chain row; every helper
    value is below 2^32; start, chained and zero blocks occur, and a live first block followed by a zero second block; the largest carries
    are printed.  On EVERY boundary row round 0 is also written out with plain integer SHA-256 (sha_air_model.sha_round), from the IV or from
    IV + the state of the row: that ties the model to the hash and not to itself"""
    n_start = n_chained = n_zero = n_live_zero = rows_checked = ca_max = ce_max = 0
    for name, tables in (("skip4", skip4), ("step2", step2), ("step3", step3)):
        for sec, table in tables.items():
            chain, n_proofs, R = CHAIN[sec], table.shape[0] // W, table.shape[1]
            assert int(table.max()) < 1 << 32
            help_ = si.helper(table, n_proofs, chain)
            assert help_.shape == (n_proofs * HC, R) and int(help_.max()) < 1 << 32
            for p in range(n_proofs):
                t, h = table[p * W:(p + 1) * W], help_[p * HC:(p + 1) * HC]
                for j, c in enumerate(si.integer_residuals(t, h, chain)):
                    assert not c.any(), (name, sec, p, j, np.flatnonzero(c)[:4])
                live = t.reshape(W, -1, 64).any(axis=(0, 2))
                assert np.array_equal(h[si.HLV].reshape(-1, 64), np.repeat(live[:, None], 64, axis=1).astype(np.uint64))
                second = np.arange(live.size) % 2 == 1 if chain else np.zeros(live.size, dtype=bool)
                n_zero += int((~live).sum())
                n_chained += int((live & second).sum())
                n_start += int((live & ~second).sum())
                if chain:
                    n_live_zero += int((live[0::2] & ~live[1::2]).sum())
                    assert not (~live[0::2] & live[1::2]).any()  # (no second block without its first)
                ca, ce = _carries(h)
                ca_max, ce_max = max(ca_max, int(ca.max())), max(ce_max, int(ce.max()))
                inner = [r for r in range(R) if not si.boundary_row(r)]
                assert not ca[inner].any() and not ce[inner].any()
                rows = [[int(x) for x in t[:, r]] for r in range(R)]
                for r in range(63, R, 64):  # round 0 of the next block, written out
                    nxt = rows[(r + 1) % R]
                    if not live[((r + 1) % R) // 64]:
                        assert not any(nxt)
                        continue
                    state = [(v + s) & si.MASK for v, s in zip(si.IV, rows[r][1:])] if si.chain_row(r, chain) else si.IV
                    assert nxt[1:] == sm.sha_round(state, nxt[0], 0), (name, sec, p, r)
                    rows_checked += 1
    print(f"\n[sha-init] start blocks {n_start}, chained blocks {n_chained}, zero blocks {n_zero}, live first blocks before a zero second block "
          f"{n_live_zero}; round 0 written out on {rows_checked} rows; largest carries a {ca_max} e {ce_max}")
    assert n_start and n_chained and n_zero and n_live_zero and rows_checked
    assert ca_max <= 6 and ce_max <= 5


@pytest.mark.parametrize("chain", [0, 1])
def test_model_uint64_path_equals_python_integers(oracle, chain):
    """one whole quotient of random columns through the uint64 field and through Python integers, in both modes"""
    rng = np.random.default_rng(9900 + chain)
    ext, hext = rng.integers(0, 1 << 64, (W, 256), dtype=np.uint64), rng.integers(0, 1 << 64, (HC, 256), dtype=np.uint64)
    g = (0x0123456789ABCDEF % P, 0xFEDCBA9876543210 % P)
    assert np.array_equal(si.quotient(oracle, 8, 1, 1, chain, ext, hext, _shift(), g),
                          si.quotient(oracle, 8, 1, 1, chain, ext, hext, _shift(), g, ints=True))


def _model_quotient(oracle, table, help_, chain, log_blowup=LB):
    """(extended table, extended helper, gamma, planar quotient) of pre-LDE columns"""
    n_proofs, log_n = table.shape[0] // W, table.shape[1].bit_length() - 1 + log_blowup
    ext, hext = oracle.lde(table, log_blowup), oracle.lde(help_, log_blowup)
    g = si.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, chain, _cap(oracle, ext, log_n), _cap(oracle, hext, log_n))
    return ext, hext, g, si.quotient(oracle, log_n, log_blowup, n_proofs, chain, ext, hext, _shift(), g)


@pytest.mark.parametrize("which", ["T.3 of skip N = 4", "T.5 of step N = 3"])
def test_quotient_is_a_polynomial_of_degree_below_n(oracle, skip4, step3, which):
    """two proofs, blow-up 4: the model quotient of the honest tables interpolates to degree < N in both planes, and the identity holds at a
    zeta outside the base field; it fails after bumping u_0, a table opening at zeta, one at zeta omega, or a helper opening on either side"""
    table, chain = (skip4[SHA256], 0) if which.startswith("T.3") else (step3[TREE], 1)
    N = table.shape[1]
    assert N == 512
    log_n, n_proofs = N.bit_length() - 1 + LB, table.shape[0] // W
    help_ = si.helper(table, n_proofs, chain)
    ext, hext, g, quot = _model_quotient(oracle, table, help_, chain)
    deg = _degrees(oracle, quot)
    print(f"\n[sha-init] {which}: N = {N}, quotient degrees {deg}")
    assert max(deg) < N and g[1] != 0
    M = 1 << log_n
    zeta = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)
    zs = (zeta, fm.e_scale(zeta, oracle.gl_root(log_n - LB)))
    yt, yh = dm.evaluate(oracle, table, 1, zs), dm.evaluate(oracle, help_, 1, zs)
    u = [am.horner(am.coefficients(oracle, quot[k * M:(k + 1) * M], _shift()), zeta) for k in (0, 1)]
    t0, t1, h0, h1 = [tuple(y[0]) for y in yt], [tuple(y[1]) for y in yt], [tuple(y[0]) for y in yh], [tuple(y[1]) for y in yh]
    ident = lambda t0=t0, t1=t1, h0=h0, h1=h1, u0=u[0]: si.identity_at(oracle, log_n, LB, n_proofs, chain, t0, t1, h0, h1, u0, u[1], zeta, g)
    assert ident()
    assert not ident(u0=fm.e_add(u[0], (1, 0)))
    bump = lambda v, at: v[:at] + [fm.e_add(v[at], (0, 1))] + v[at + 1:]
    assert not ident(t0=bump(t0, W + si.A_)) and not ident(t1=bump(t1, si.W_))
    assert not ident(h0=bump(h0, si.HV + 7)) and not ident(h1=bump(h1, HC + si.HLV))


RERUN = "a block re-run from a changed row-0 state"
RERUN_W5 = "a block re-run from a changed W_5, schedule and rounds recomputed"


def _pair(table):
    """the first rows (r0 of the first block, r0 + 64 of the second) of a hash of proof 0's chained table whose two blocks are both live"""
    live = table[:W].reshape(W, -1, 64).any(axis=(0, 2))
    both = np.flatnonzero(live[0::2] & live[1::2])
    r0 = 128 * int(both[len(both) // 2])
    return r0, r0 + 64


def _tampered(skip_table, tree_table, kind):
    """(table, init helper, chain) of ONE proof after a single change of `kind`: T.3 of skip N = 4, or T.5 of step N = 3 where it says so"""
    if kind in (RERUN, RERUN_W5):
        t = (tsa._tampered(skip_table, kind) if kind == RERUN else tss._tampered(skip_table, kind))[0]
        return t, si.helper(t, 1, 0), 0
    in_tree = kind.startswith("T.5")
    t, chain = (tree_table if in_tree else skip_table)[:W].copy(), int(in_tree)
    if in_tree:
        first, second = _pair(t)
    else:
        first = tsa._mid_row(t)[1]
    if kind == "d of a row 0 changed alone":
        t[si.D_, first] ^= np.uint64(1 << 17)
        return t, si.helper(t, 1, chain), chain
    if kind == "T.5: f of a chained block's row 0 changed":
        t[si.F_, second] ^= np.uint64(1 << 4)
        return t, si.helper(t, 1, chain), chain
    if kind == "T.5: h of a first block's row 63 changed, the helper regenerated":
        t[si.H_, first + 63] ^= np.uint64(1 << 21)
        return t, si.helper(t, 1, chain), chain
    if kind == "T.5: a live second block replaced by zeros, the helper regenerated":
        t[:, second:second + 64] = 0
        return t, si.helper(t, 1, chain), chain
    h = si.helper(t, 1, chain)
    if kind == "T.5: a flipped CZ bit on a chain row":
        h[si.HCZ + 2, first + 63] ^= np.uint64(1)
    elif kind == "LV cleared on row 0 of a live block":
        assert h[si.HLV, first] == 1
        h[si.HLV, first] = 0
    elif kind == "T.5: a changed PZ_3 on a chain row":
        h[si.HPZ + 3, first + 63] += np.uint64(1)
    else:
        raise KeyError(kind)
    return t, h, chain


DETECTED = [RERUN, "d of a row 0 changed alone", "T.5: f of a chained block's row 0 changed",
            "T.5: h of a first block's row 63 changed, the helper regenerated", "T.5: a flipped CZ bit on a chain row",
            "LV cleared on row 0 of a live block", "T.5: a changed PZ_3 on a chain row"]
UNDETECTED = [RERUN_W5, "T.5: a live second block replaced by zeros, the helper regenerated"]


def _degrees_under_sets_3_and_4(oracle, t):
    return (max(_degrees(oracle, tsa._model_quotient(oracle, t, sm.helper(t, 1))[3])),
            max(_degrees(oracle, tss._model_quotient(oracle, t, ss.helper(t, 1))[3])))


@pytest.mark.parametrize("kind", DETECTED)
def test_one_change_breaks_the_degree(oracle, skip4, step3, kind):
    """the detected kinds (one proof): the quotient no longer interpolates to degree < N.  The first is the hole that tests/test_sha_air.py
    and tests/test_sha_sched.py both record: the rows come from test_sha_air's `_tampered`, and set 3's and set 4's own model quotients of
    them stay below N"""
    t, h, chain = _tampered(skip4[SHA256], step3[TREE], kind)
    table = (step3[TREE] if chain else skip4[SHA256])[:W]
    assert (t != table).sum() + (h != si.helper(table, 1, chain)).sum() >= 1
    deg = _degrees(oracle, _model_quotient(oracle, t, h, chain)[3])
    print(f"\n[sha-init] {kind}: quotient degrees {deg}, N = {table.shape[1]}")
    assert max(deg) >= table.shape[1]
    if kind == RERUN:
        assert kind in tsa.UNDETECTED and kind in tss.UNDETECTED and (t != table).sum() > 8
        d3, d4 = _degrees_under_sets_3_and_4(oracle, t)
        print(f"[sha-init] the same rows under set 3: degree {d3}, under set 4: degree {d4}")
        assert d3 < table.shape[1] and d4 < table.shape[1]


@pytest.mark.parametrize("kind", UNDETECTED)
def test_kinds_the_constraints_do_not_see(oracle, skip4, step3, kind):
    """recorded so that nobody mistakes the claim.  NOT proved by sets 3 + 4 + 5: the first sixteen W of a block against Level-1 (a block
    re-run consistently, schedule AND rounds, from a changed W_5 keeps all three quotients low-degree); LV against anything public (a live
    second block of a T.5 hash replaced by a zero block goes unseen: the set cannot know that a second block was due); the digest against
    Level-1; SHA-512; the ladders' curve arithmetic and limb ranges"""
    t, h, chain = _tampered(skip4[SHA256], step3[TREE], kind)
    table = (step3[TREE] if chain else skip4[SHA256])[:W]
    assert (t != table).sum() > 8
    assert max(_degrees(oracle, _model_quotient(oracle, t, h, chain)[3])) < table.shape[1]
    d3, d4 = _degrees_under_sets_3_and_4(oracle, t)
    assert d3 < table.shape[1] and d4 < table.shape[1]


def test_symbols_and_wrappers_exist(built_lib):
    """the new entry points are in the built library, bound in _lib.py and wrapped in context.py"""
    from tendermintx_amd import _lib
    from tendermintx_amd.context import Context
    for name in ("tmx_air_sha256_init_helper_device", "tmx_air_sha256_init_quotient_device", "tmx_air_sha256_init_verify_device",
                 "tmx_trace_commit_set_air_sha256_init_device"):
        assert getattr(built_lib, name).argtypes, name
        assert callable(getattr(Context, name[4:])), name
    assert (_lib.AIR_SHA256_INIT_HELPER_COLS, _lib.AIR_SHA256_INIT_CONSTRAINTS) == (HC, si.CONSTRAINTS)
    assert (_lib.TRACE_SHA256_INIT_HELPER, _lib.TRACE_SHA256_INIT_QUOTIENT) == (H5, Q5)


# ---- GPU
def _device_helper(ctx, table, chain):
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    d_table = _up(table)
    return _guarded((n_proofs * HC) << log_rows,
                    lambda out: ctx.air_sha256_init_helper_device(log_rows, n_proofs, chain, d_table.data_ptr(), out, 0))


def _helper_equals_the_model(ctx, table, chain):
    n_proofs = table.shape[0] // W
    got = _down(_device_helper(ctx, table, chain)).reshape(n_proofs * HC, -1)
    want = si.helper(table, n_proofs, chain)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs,chain", [(6, 1, 0), (7, 1, 1), (7, 3, 1), (8, 257, 0), (12, 1, 1)])
def test_helper_of_random_tables_equals_the_model(ctx, log_rows, n_proofs, chain):
    """random 64-bit words, the last block of the last proof zeroed where there is more than one (LV = 0 occurs, and LV' = 0 on the row in
    front of it): the helper equals the model's word for word, guard words intact.  log_rows 6 is the smallest table, a single block whose
    only boundary is the wrap; log_rows 7 is the smallest chained shape, one chain row and one wrap; 257 proofs cross every power-of-two
    grid edge.  The wrap is looked at on its own: the last row's PZ carries LV of row 0 of the SAME proof"""
    rng = np.random.default_rng(10000 + 100 * log_rows + 10 * n_proofs + chain)
    R = 1 << log_rows
    table = rng.integers(0, 1 << 64, (n_proofs * W, R), dtype=np.uint64)
    if R > 64:
        table[(n_proofs - 1) * W:, R - 64:] = 0
    want = _helper_equals_the_model(ctx, table, chain)
    for p in (0, n_proofs - 1):
        t = table[p * W:(p + 1) * W]
        lv0 = int(t[:, 0].any())
        assert int(want[p * HC + si.HLV, 0]) == lv0
        assert int(want[p * HC + si.HPZ + 5, R - 1]) == lv0 * ((si.IV[5] + (int(t[si.F_, R - 1]) & si.MASK)) & si.MASK)
    ca = want[si.HCA::HC] + 2 * want[si.HCA + 1::HC] + 4 * want[si.HCA + 2::HC]
    ce = want[si.HCE::HC] + 2 * want[si.HCE + 1::HC] + 4 * want[si.HCE + 2::HC]
    print(f"\n[sha-init] log_rows {log_rows}, {n_proofs} proofs, chain {chain}: largest carries a {int(ca.max())} e {int(ce.max())}")
    assert int(ca.max()) <= 6 and int(ce.max()) <= 5
    inner = [r for r in range(R) if not si.boundary_row(r)]
    assert not ca[:, inner].any() and not ce[:, inner].any()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["T.5 of step N = 3", "T.6 of step N = 2"])
def test_helper_of_real_rows_equals_the_model(ctx, step2, step3, which):
    """the real T.5 rows of step N = 3 (512 rows with padding, zero blocks and chained second blocks) and the real T.6 rows of step N = 2
    (4096 rows; they hold the live first blocks followed by a zero second block)"""
    table = step3[TREE] if which.startswith("T.5") else step2[HEADER]
    assert which.startswith("T.5") or table.shape[1] == 4096
    _helper_equals_the_model(ctx, table, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [0, 1])
@pytest.mark.parametrize("word", [0xFFFFFFFF, 0])
def test_helper_of_constant_tables(ctx, word, chain):
    """every operand 0xFFFFFFFF under random high words: Sigma0, Sigma1, Ch and Maj of all-ones words are all-ones words, every CZ is 1 and
    PZ_j = IV_j - 1, so the two sums follow from the definition with plain integers -- on a start row (IV_7 + K_0) + 5 (2^32 - 1) and
    (IV_3 + IV_7 + K_0) + 3 (2^32 - 1), on a chain row with PZ_7 and PZ_3 + PZ_7 in place of the IV words; the carries the device gives
    are those, printed.  An all-zero table gives an all-zero helper but for CZ, which is 0 too: IV_j < 2^32"""
    rng = np.random.default_rng(10100)
    table = np.zeros((2 * W, 256), dtype=np.uint64)
    if word:
        table = rng.integers(0, 1 << 64, (2 * W, 256), dtype=np.uint64) | np.uint64(word)
    want = _helper_equals_the_model(ctx, table, chain)
    if not word:
        assert not want.any()
        return
    ones, pz = 0xFFFFFFFF, [(v + 0xFFFFFFFF) & si.MASK for v in si.IV]
    carry = {False: ((si.IV[7] + si.K0 + 5 * ones) >> 32, (si.IV[3] + si.IV[7] + si.K0 + 3 * ones) >> 32),
             True: ((pz[7] + si.K0 + 5 * ones) >> 32, (pz[3] + pz[7] + si.K0 + 3 * ones) >> 32)}
    print(f"\n[sha-init] all-ones table, chain {chain}: carries (a, e) on a start row {carry[False]}, on a chain row {carry[True]}")
    for p in range(2):
        ca, ce = _carries(want[p * HC:(p + 1) * HC])
        for r in range(256):
            a, e = carry[si.chain_row(r, chain)] if si.boundary_row(r) else (0, 0)
            assert (int(ca[r]), int(ce[r])) == (a, e), (p, r)
        assert want[p * HC + si.HCZ:p * HC + si.HCZ + 8].all() and want[p * HC + si.HLV].all()
        assert [int(x) for x in want[p * HC + si.HPZ:p * HC + si.HPZ + 8, 5]] == pz


def _device_quotient(ctx, log_n, log_blowup, n_proofs, chain, d_cols, d_hcols, d_cap, d_cap_h, cap_height=CAP_H):
    return _guarded(2 << log_n, lambda out: ctx.air_sha256_init_quotient_device(log_n, log_blowup, cap_height, n_proofs, chain, d_cols.data_ptr(),
                                                                               d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(), out, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,log_blowup,n_proofs,cap_height,chain", [(6, 1, 1, 0, 0), (6, 3, 17, 2, 0), (6, 6, 1, 2, 0), (7, 1, 3, 2, 1),
                                                                           (7, 3, 1, 0, 1), (10, 2, 2, 2, 1)])
def test_quotient_of_random_columns_equals_the_model(ctx, oracle, log_rows, log_blowup, n_proofs, cap_height, chain):
    """N = 64 (one block: D_s' period is the whole domain), N = 128 (the smallest chained shape) and N = 1024, random table and helper
    columns: the definition is pointwise, so d_quot and gamma equal the model word for word, guard words intact; on the same caps the
    other mode draws another gamma"""
    log_n = log_rows + log_blowup
    rng = np.random.default_rng(10200 + 100 * log_rows + 10 * log_blowup + n_proofs)
    ext, hext = _random_ext(rng, n_proofs * W, log_n), _random_ext(rng, n_proofs * HC, log_n)
    d_cols, d_hcols = _up(ext), _up(hext)
    _, d_cap = _tree(ctx, d_cols, log_n, n_proofs * W, cap_height)
    _, d_cap_h = _tree(ctx, d_hcols, log_n, n_proofs * HC, cap_height)
    got = _down(_device_quotient(ctx, log_n, log_blowup, n_proofs, chain, d_cols, d_hcols, d_cap, d_cap_h, cap_height))
    g = si.gamma(oracle, log_n, log_blowup, cap_height, n_proofs, chain, _down(d_cap), _down(d_cap_h))
    assert ctx.air_last_gamma() == g
    want = si.quotient(oracle, log_n, log_blowup, n_proofs, chain, ext, hext, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    if log_rows >= 7:  # (both modes take this shape)
        other = si.gamma(oracle, log_n, log_blowup, cap_height, n_proofs, 1 - chain, _down(d_cap), _down(d_cap_h))
        _device_quotient(ctx, log_n, log_blowup, n_proofs, 1 - chain, d_cols, d_hcols, d_cap, d_cap_h, cap_height)
        assert ctx.air_last_gamma() == other and other != g


def _chain(ctx, oracle, table, chain, log_blowup, quot_override=None, n_queries=6):
    """caller-level chain: helper -> LDE -> caps -> quotient -> one batch proof over [table, helper, quotient].  Returns (params, d_caps,
    proof words, extended table, extended helper, quotient words)"""
    import torch
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    log_n = log_rows + log_blowup
    d_help = _device_helper(ctx, table, chain)
    d_ext, d_hext = _sentinel((n_proofs * W) << log_n), _sentinel((n_proofs * HC) << log_n)
    ctx.lde_device(log_rows, log_blowup, n_proofs * W, _up(table).data_ptr(), d_ext.data_ptr(), 0)
    ctx.lde_device(log_rows, log_blowup, n_proofs * HC, d_help.data_ptr(), d_hext.data_ptr(), 0)
    d_lv_t, d_cap_t = _tree(ctx, d_ext, log_n, n_proofs * W)
    d_lv_h, d_cap_h = _tree(ctx, d_hext, log_n, n_proofs * HC)
    d_quot = (_device_quotient(ctx, log_n, log_blowup, n_proofs, chain, d_ext, d_hext, d_cap_t, d_cap_h) if quot_override is None
              else _up(quot_override))
    d_lv_q, d_cap_q = _tree(ctx, d_quot, log_n, 2)
    p = bparams([log_n] * 3, [n_proofs * W, n_proofs * HC, 2], CAP_H, log_blowup, 2, 2, n_queries)
    proof = _guarded(bm.layout(p)["words"], lambda out: ctx.batch_prove_device(p, [d.data_ptr() for d in (d_ext, d_hext, d_quot)],
                                                                               [d.data_ptr() for d in (d_lv_t, d_lv_h, d_lv_q)], out, 0))
    return (p, torch.cat([d_cap_t, d_cap_h, d_cap_q]), _down(proof), _down(d_ext).reshape(n_proofs * W, -1),
            _down(d_hext).reshape(n_proofs * HC, -1), _down(d_quot))


def _verdicts(ctx, p, k_trace, k_helper, chain, d_caps, proof):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=tsa._dev())
    ctx.air_sha256_init_verify_device(p, k_trace, k_helper, chain, d_caps.data_ptr(), _up(proof).data_ptr(), ok.data_ptr(), 0)
    torch.cuda.synchronize(tsa._dev())
    out = ok.cpu().numpy()
    assert ((out == 0) | (out == 1)).all(), out
    return [bool(x) for x in out]


def _bumped(proof, at):
    bad = proof.copy()
    bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("which,log_blowup", [("T.3 of skip N = 4", 2), ("T.5 of step N = 3", 1)])
def test_real_tables_through_the_caller_level_chain(ctx, oracle, skip4, step3, which, log_blowup):
    """helper -> LDE -> caps -> quotient -> tmx_batch_prove_device -> tmx_air_sha256_init_verify_device on the real T.3 (chain 0) and T.5
    (chain 1) rows: the quotient and gamma equal the model's and the quotient has degree < N; every verdict equals the model verifier's
    (all accept); a proof with one bumped table, helper or quotient opening is rejected on every query; the other mode rejects the proof"""
    table, chain = (skip4[SHA256], 0) if which.startswith("T.3") else (step3[TREE], 1)
    n_proofs = table.shape[0] // W
    p, d_caps, got, ext, hext, quot = _chain(ctx, oracle, table, chain, log_blowup)
    assert ctx.fri_last_degree_ok() is True
    log_n, caps, cw = p["log_n"][0], _down(d_caps), 4 << CAP_H
    assert np.array_equal(hext, oracle.lde(si.helper(table, n_proofs, chain), log_blowup))
    g = si.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, chain, caps[:cw], caps[cw:2 * cw])
    assert np.array_equal(quot, si.quotient(oracle, log_n, log_blowup, n_proofs, chain, ext, hext, _shift(), g))
    assert max(_degrees(oracle, quot)) < table.shape[1]
    model = si.verify(oracle, p, 0, 1, chain, caps, got, _shift())
    assert all(model) and _verdicts(ctx, p, 0, 1, chain, d_caps, got) == model
    other = si.verify(oracle, p, 0, 1, 1 - chain, caps, got, _shift())
    assert not any(other) and _verdicts(ctx, p, 0, 1, 1 - chain, d_caps, got) == other
    L = bm.layout(p)
    RT, RH = 1 << dm.log_r(p["n_cols"][0]), 1 << dm.log_r(p["n_cols"][1])
    for name, at in (("quotient opening", L["off_open"][2] + 1), ("helper opening at zeta", L["off_open"][1] + si.HD + 9),
                     ("helper opening at zeta omega", L["off_open"][1] + 2 * RH + HC + si.HLV),
                     ("table opening at zeta", L["off_open"][0] + si.A_), ("table opening at zeta omega", L["off_open"][0] + 2 * RT + si.W_)):
        bad = _bumped(got, at)
        assert not si.identity(oracle, p, 0, 1, chain, caps, bad), name
        model = si.verify(oracle, p, 0, 1, chain, caps, bad, _shift())
        assert not any(model), name
        assert _verdicts(ctx, p, 0, 1, chain, d_caps, bad) == model, name


@pytest.mark.gpu
def test_the_rerun_from_row_0_is_rejected_and_sets_3_and_4_still_accept_it(ctx, oracle, skip4):
    """the table re-run from a changed row-0 state (the kind tests/test_sha_air.py and tests/test_sha_sched.py record as undetected), one
    proof, blow-up 4, with its HONEST quotients: set 5's chain clears every verdict, as the model does -- the quotient is no polynomial of
    degree < N, so the proof over it fails -- while set 3's and set 4's chains over the same rows with their own helpers accept every query"""
    table = skip4[SHA256][:W]
    t, _, chain = _tampered(skip4[SHA256], None, RERUN)
    p, d_caps, got, _, _, quot = _chain(ctx, oracle, t, chain, 2)
    assert max(_degrees(oracle, quot)) >= table.shape[1]
    model = si.verify(oracle, p, 0, 1, chain, _down(d_caps), got, _shift())
    assert not any(model) and _verdicts(ctx, p, 0, 1, chain, d_caps, got) == model
    p3, d_caps3, got3, _, _, _ = tsa._chain(ctx, oracle, t, 2)
    assert all(tsa._verdicts(ctx, p3, 0, d_caps3, got3))
    p4, d_caps4, got4, _, _, _ = tss._chain(ctx, oracle, t, 2)
    assert all(tss._verdicts(ctx, p4, 0, 1, d_caps4, got4))


@pytest.mark.gpu
def test_zero_quotient_for_a_tampered_table(ctx, oracle, skip4):
    """a zero (low-degree) quotient committed for the same re-run table: the batch proof is fine and the identity fails -- every verdict is
    cleared by k_air_init_check alone, as in the model"""
    t, _, chain = _tampered(skip4[SHA256], None, RERUN)
    log_n = t.shape[1].bit_length() - 1 + 1
    p, d_caps, got, _, _, _ = _chain(ctx, oracle, t, chain, 1, quot_override=np.zeros(2 << log_n, dtype=np.uint64))
    assert all(tsa._verdicts(ctx, p, 0, d_caps, got, batch_only=True))
    model = si.verify(oracle, p, 0, 1, chain, _down(d_caps), got, _shift())
    assert not any(model) and _verdicts(ctx, p, 0, 1, chain, d_caps, got) == model


MANY = 257  # one proof more than k_air_init_check has threads: thread 0 takes proofs 0 and 256


@pytest.mark.gpu
def test_257_proofs_through_the_check_kernel(ctx, oracle, step3):
    """N = 128, chain 1, 257 proofs (the hashes of T.5 of step N = 3 in turn -- pairs of live blocks, live first blocks with a zero second
    one -- every seventh proof zero), blow-up 2, two queries: the device accepts every query as the model does; one helper opening bumped in
    proof 256, one in proof 200 and a table opening in proof 255 are each rejected"""
    t5 = step3[TREE]
    pairs = np.concatenate([t5[p * W:(p + 1) * W].reshape(W, -1, 128).transpose(1, 0, 2) for p in range(t5.shape[0] // W)])
    pairs = pairs[pairs.any(axis=(1, 2))]
    table = np.zeros((MANY * W, 128), dtype=np.uint64)
    for q in range(MANY):
        if q % 7 != 6:
            table[q * W:(q + 1) * W] = pairs[q % len(pairs)]
    p, d_caps, got, ext, hext, _ = _chain(ctx, oracle, table, 1, 1, n_queries=2)
    assert ctx.fri_last_degree_ok() is True
    assert np.array_equal(hext, oracle.lde(si.helper(table, MANY, 1), 1))
    caps = _down(d_caps)
    assert si.identity(oracle, p, 0, 1, 1, caps, got)
    assert _verdicts(ctx, p, 0, 1, 1, d_caps, got) == [True, True]
    L = bm.layout(p)
    for at in (L["off_open"][1] + 256 * HC + si.HU1 + 3, L["off_open"][1] + 200 * HC + si.HPZ + 2, L["off_open"][0] + 255 * W + si.D_):
        bad = _bumped(got, at)
        assert not si.identity(oracle, p, 0, 1, 1, caps, bad)
        assert _verdicts(ctx, p, 0, 1, 1, d_caps, bad) == [False, False]


# ---- the set level
@pytest.fixture(scope="module")
def header_sets(built_lib, oracle):
    """a set SHA256 + HEADER at step N = 2, two proofs (the shape of test_sha_air.test_set_level_on_the_header_table), four ways: set 5
    alone on HEADER, then sets 3, 4 and 5 in the call orders 5-3-4, 3-5-4 and 3-4-5.  Per way: (shape, section_of, caps of every oracle in
    order, proof words, verdicts)"""
    import torch
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    kind, n, n_proofs, lb = 1, 2, 2, 1
    cw = 4 << CAP_H
    out = {}
    with tmx.Context(n, b"celestia", max_batch=n_proofs) as c:
        tr = _trace_rows(c, kind, n, n_proofs, 9300)
        out["traces"] = _down(tr)
        calls = {"3": c.trace_commit_set_air_sha256_device, "4": c.trace_commit_set_air_sha256_sched_device,
                 "5": c.trace_commit_set_air_sha256_init_device}
        for way in ("5", "534", "354", "345"):
            d_caps = _sentinel(2 * cw)
            c.trace_commit_set_device(kind, n_proofs, SHA256 | HEADER, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
            pair, gammas = {}, {}
            for s in way:
                pair[s] = (_sentinel(cw), _sentinel(cw))
                calls[s](HEADER, pair[s][0].data_ptr(), pair[s][1].data_ptr(), 0)
                gammas[s] = c.air_last_gamma()
            shape, order = c.trace_commit_set_shape()
            p = dict(shape, arity_bits=2, final_log_max=2, n_queries=6, pow_bits=0)
            proof = _guarded(bm.layout(p)["words"], lambda o: c.trace_commit_set_prove_device(p, o, 0))
            assert c.fri_last_degree_ok() is True
            all_caps = torch.cat([d_caps[:cw]] + [x for s in sorted(way) for x in pair[s]] + [d_caps[cw:]])
            k5 = order.index(H5)
            v = dict(init=_verdicts(c, p, 0, k5, 1, all_caps, _down(proof)), batch=tsa._verdicts(c, p, 0, all_caps, _down(proof), batch_only=True))
            if "3" in way:
                v["sha"] = tsa._verdicts(c, p, 0, all_caps, _down(proof))
                v["sched"] = tss._verdicts(c, p, 0, order.index(H4), all_caps, _down(proof))
            bad = _bumped(_down(proof), bm.layout(p)["off_open"][k5 + 1])
            v["bad"] = _verdicts(c, p, 0, k5, 1, all_caps, bad)
            if way == "5":  # the model's helper cap through the device's tree, as tests/test_sha_air.py does
                off, rows, _ = tsa._section_geom(kind, n, HEADER)
                table = np.zeros((n_proofs * W, 1 << 12), dtype=np.uint64)
                for q, full in enumerate(out["traces"]):
                    table[q * W:(q + 1) * W, :rows] = full[off:off + rows * W].reshape(rows, W).T
                out["hext"] = oracle.lde(si.helper(table, n_proofs, 1), lb)
                out["cap_h_model"] = _down(_tree(c, _up(out["hext"]), 12 + lb, n_proofs * HC)[1])
            out[way] = dict(p=p, order=order, caps=_down(all_caps), proof=_down(proof), verdicts=v, gammas=gammas)
    return out


@pytest.mark.gpu
def test_set_level_with_set_5_alone(oracle, header_sets):
    """three oracles behind each other -- section_of ends 32, 2048, 4096 with SHA256 behind -- the helper's cap, gamma (chain = 1 for
    HEADER) and the quotient's cap against the model, the device verifier and the model's on the proof over the four oracles,
    tmx_batch_verify_device against tests/batch_model.py"""
    from test_merkle_open import _oracle_ext
    s, lb, n_proofs, cw = header_sets["5"], 1, 2, 4 << CAP_H
    assert s["order"] == [HEADER, H5, Q5, SHA256]
    assert s["p"]["log_n"] == [12 + lb] * 3 + [7 + lb] and s["p"]["n_cols"] == [W * n_proofs, HC * n_proofs, 2, W * n_proofs]
    caps = s["caps"]
    e, lm, nc = _oracle_ext(oracle, 1, 2, header_sets["traces"], HEADER, lb)
    ext = e.reshape(nc, -1)
    assert np.array_equal(caps[:cw], _cap(oracle, ext, lm))
    assert np.array_equal(caps[cw:2 * cw], header_sets["cap_h_model"])
    g = si.gamma(oracle, lm, lb, CAP_H, n_proofs, 1, caps[:cw], caps[cw:2 * cw])
    assert s["gammas"]["5"] == g
    quot = si.quotient(oracle, lm, lb, n_proofs, 1, ext, header_sets["hext"], _shift(), g)
    assert np.array_equal(caps[2 * cw:3 * cw], _cap(oracle, quot.reshape(2, -1), lm))
    assert s["verdicts"]["batch"] == bm.verify(oracle, s["p"], caps, s["proof"], _shift())
    model = si.verify(oracle, s["p"], 0, 1, 1, caps, s["proof"], _shift())
    assert all(model) and s["verdicts"]["init"] == model and not any(s["verdicts"]["bad"])


@pytest.mark.gpu
def test_set_level_in_three_orders_with_sets_3_and_4(oracle, header_sets):
    """the call orders 5-3-4, 3-5-4 and 3-4-5 all end as table, H3, Q3, H4, Q4, H5, Q5, SHA256: the same section_of, the same caps and
    the same proof word for word; set 5's caps are those of the set with set 5 alone; the set-3, set-4 and set-5 device verifiers accept
    that proof, all three model identities hold, and tmx_batch_verify_device equals tests/batch_model.py"""
    a, b, c, alone, cw = header_sets["534"], header_sets["354"], header_sets["345"], header_sets["5"], 4 << CAP_H
    assert a["order"] == b["order"] == c["order"] == [HEADER, H3, Q3, H4, Q4, H5, Q5, SHA256]
    assert a["p"] == b["p"] == c["p"] and a["p"]["n_cols"][:7] == [2 * W, 2 * HC3, 2, 2 * HC4, 2, 2 * HC, 2]
    for s in (b, c):
        assert np.array_equal(a["caps"], s["caps"]) and np.array_equal(a["proof"], s["proof"])
        assert a["gammas"] == s["gammas"]
    assert np.array_equal(a["caps"][5 * cw:7 * cw], alone["caps"][cw:3 * cw]) and a["gammas"]["5"] == alone["gammas"]["5"]
    for s in (a, b, c):
        v = s["verdicts"]
        assert all(v["sha"]) and all(v["sched"]) and all(v["init"]) and all(v["batch"]) and not any(v["bad"])
    assert a["verdicts"]["batch"] == bm.verify(oracle, a["p"], a["caps"], a["proof"], _shift())
    assert si.identity(oracle, a["p"], 0, 5, 1, a["caps"], a["proof"]) and ss.identity(oracle, a["p"], 0, 3, a["caps"], a["proof"])
    assert sm.identity(oracle, a["p"], 0, a["caps"], a["proof"])


@pytest.mark.gpu
def test_set_level_refusals(built_lib):
    """before a set, a section that is no SHA-256 table, an absent section, null caps, a second call (behind the table, and behind set 3's
    and set 4's pairs), a streamed member: TMX_ERR_BAD_ARG, nothing written, the set's shape as it was"""
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    kind, n, n_proofs, lb = 1, 2, 2, 1
    cw = 4 << CAP_H
    with tmx.Context(n, b"celestia", max_batch=n_proofs) as c:
        tr = _trace_rows(c, kind, n, n_proofs, 9300)
        d_caps, d_cap_h, d_cap_q = _sentinel(2 * cw), _sentinel(cw), _sentinel(cw)
        air = lambda sec: (lambda: c.trace_commit_set_air_sha256_init_device(sec, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0))
        assert "no commit set" in _refused(air(HEADER), d_cap_h, d_cap_q)
        c.trace_commit_set_device(kind, n_proofs, SHA256 | HEADER, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        before = c.trace_commit_set_shape()
        for sec in (TREE, 1, H3, H4, H5, Q5, 0):
            _refused(air(sec), d_cap_h, d_cap_q)
        _refused(lambda: c.trace_commit_set_air_sha256_init_device(HEADER, None, d_cap_q.data_ptr(), 0), d_cap_q)
        _refused(lambda: c.trace_commit_set_air_sha256_init_device(HEADER, d_cap_h.data_ptr(), None, 0), d_cap_h)
        assert c.trace_commit_set_shape() == before
        a, b = _sentinel(cw), _sentinel(cw)
        c.trace_commit_set_air_sha256_init_device(SHA256, a.data_ptr(), b.data_ptr(), 0)
        assert c.trace_commit_set_shape()[1] == [HEADER, SHA256, H5, Q5]
        assert "already" in _refused(air(SHA256), d_cap_h, d_cap_q)
        c.trace_commit_set_air_sha256_sched_device(SHA256, a.data_ptr(), b.data_ptr(), 0)
        assert c.trace_commit_set_shape()[1] == [HEADER, SHA256, H4, Q4, H5, Q5]
        assert "already" in _refused(air(SHA256), d_cap_h, d_cap_q)
        c.trace_commit_set_air_sha256_device(SHA256, a.data_ptr(), b.data_ptr(), 0)
        assert c.trace_commit_set_shape()[1] == [HEADER, SHA256, H3, Q3, H4, Q4, H5, Q5]
        assert "already" in _refused(air(SHA256), d_cap_h, d_cap_q)
        assert "room" in _refused(air(HEADER), d_cap_h, d_cap_q)  # (eight oracles: a full set)
        c.trace_commit_set_streamed_device(kind, n_proofs, SHA256 | HEADER, HEADER, 8, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        assert "streamed" in _refused(air(HEADER), d_cap_h, d_cap_q)


@pytest.mark.gpu
def test_a_full_set_is_refused(built_lib):
    """all five tables and the ladders' quotient are six oracles; one block-start pair makes eight; a second pair would exceed eight"""
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    cw = 4 << CAP_H
    with tmx.Context(4, b"celestia", max_batch=1) as c:
        tr = _trace_rows(c, 0, 4, 1, 9400)
        d_caps, d_cap_h, d_cap_q = _sentinel(5 * cw), _sentinel(cw), _sentinel(cw)
        c.trace_commit_set_device(0, 1, 1 | 2 | SHA256 | TREE | HEADER, 1, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        c.trace_commit_set_air_device(d_cap_q.data_ptr(), 0)
        c.trace_commit_set_air_sha256_init_device(TREE, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
        _, order = c.trace_commit_set_shape()
        assert len(order) == 8 and order[order.index(TREE) + 1:order.index(TREE) + 3] == [H5, Q5]
        assert "room" in _refused(lambda: c.trace_commit_set_air_sha256_init_device(SHA256, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0),
                                  d_cap_h, d_cap_q)


@pytest.mark.gpu
def test_each_validation_rule(ctx):
    """every rule of the three caller-level calls on its own: TMX_ERR_BAD_ARG before anything is enqueued, nothing written.  They are set
    4's rules with 315 n_proofs <= 2^24, and: chain > 1 is refused; chain = 1 with fewer than 128 rows is refused"""
    import torch
    log_n, lb = 8, 1
    d_cols, d_hcols = _sentinel(W << log_n), _sentinel(HC << log_n)
    d_cap, d_cap_h, d_quot = _sentinel(4 << CAP_H), _sentinel(4 << CAP_H), _sentinel(2 << log_n)
    ptrs = [d_cols.data_ptr(), d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(), d_quot.data_ptr()]
    q = lambda ln, b, n, ch=0, a=ptrs: (lambda: ctx.air_sha256_init_quotient_device(ln, b, CAP_H, n, ch, *a, 0))
    for fn in (q(log_n, 0, 1), q(log_n, 7, 1), q(2, 2, 1), q(29, 2, 1), q(6, 1, 1), q(11, 6, 1), q(log_n, lb, 0), q(log_n, lb, (1 << 24) // HC + 1),
               q(log_n, lb, 1, ch=2), q(7, 1, 1, ch=1), q(9, 3, 1, ch=1)):
        _refused(fn, d_quot)
    for k in range(5):
        _refused(q(log_n, lb, 1, 1, ptrs[:k] + [None] + ptrs[k + 1:]), d_quot)
    d_table, d_help = _sentinel(W << 7), _sentinel(HC << 7)
    hp = lambda lr, n, ch=0, t=d_table.data_ptr(), o=d_help.data_ptr(): (lambda: ctx.air_sha256_init_helper_device(lr, n, ch, t, o, 0))
    for fn in (hp(5, 1), hp(28, 1), hp(7, 0), hp(7, (1 << 24) // HC + 1), hp(7, 1, t=None), hp(7, 1, o=None), hp(7, 1, ch=2), hp(6, 1, ch=1)):
        _refused(fn, d_help)
    # the verifier: column counts 9 k / 315 k / 2, equal log_n, k_trace < k_helper, k_helper + 1 inside the proof, the mode
    ok, caps, proof = torch.full((4,), 7, dtype=torch.int32, device=tsa._dev()), _sentinel(256), _sentinel(1 << 16)
    v = lambda p, kt, kh, ch=0: (lambda: ctx.air_sha256_init_verify_device(p, kt, kh, ch, caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0))
    good = bparams([8, 8, 8], [W, HC, 2], CAP_H, lb, 2, 2, 4)
    for p, kt, kh in ((good, 0, 2), (good, 0, 0), (good, 1, 1), (good, 1, 0), (dict(good, n_cols=[W + 1, HC, 2]), 0, 1),
                      (dict(good, n_cols=[W, HC + 1, 2]), 0, 1), (dict(good, n_cols=[W, HC3, 2]), 0, 1), (dict(good, n_cols=[2 * W, HC, 2]), 0, 1),
                      (dict(good, n_cols=[W, HC, 3]), 0, 1), (dict(good, log_n=[8, 8, 7]), 0, 1), (dict(good, log_n=[8, 7, 8]), 0, 1),
                      (bparams([6, 6, 6], [W, HC, 2], CAP_H, lb, 2, 2, 4), 0, 1), (dict(good, arity_bits=0), 0, 1),
                      (bparams([8, 8], [W, HC], CAP_H, lb, 2, 2, 4), 0, 1)):
        _refused(v(p, kt, kh), ok)
    _refused(v(good, 0, 1, ch=2), ok)
    _refused(v(bparams([7, 7, 7], [W, HC, 2], CAP_H, lb, 2, 2, 4), 0, 1, ch=1), ok)
