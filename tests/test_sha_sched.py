"""The message schedule of the SHA-256 tables (include/tmx.h "the message schedule of the SHA-256 tables", constraint set 4):
tmx_air_sha256_sched_helper_device, tmx_air_sha256_sched_quotient_device, tmx_air_sha256_sched_verify_device,
tmx_trace_commit_set_air_sha256_sched_device.  The yardstick is tests/sha_sched_model.py on top of tests/batch_model.py: device words must
equal the model's word for word and every verdict of the device verifier must equal the model verifier's.  The CPU part ties the model to
the claim: on the CPU oracle's T.3, T.5 and T.6 rows all 117 constraints hold as integer identities, the quotient is a polynomial of
degree < N, and one change of a detected kind -- the re-run from a changed W_t, t >= 16, that set 3 alone does not see among them -- makes
it one of degree >= N; the kinds that sets 3 and 4 together still do NOT see are recorded next to them.  The fixtures and the plumbing
are those of tests/test_sha_air.py."""
import numpy as np
import pytest

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha_air_model as sm
import sha_sched_model as ss
import test_sha_air as tsa
from batch_model import bparams
from test_fri import _down, _sentinel, _shift, _up
from test_sha_air import ctx, skip4, step2, step3  # noqa: F401  (fixtures)
from test_sha_air import _cap, _degrees, _guarded, _random_ext, _refused, _tree

P = fm.P
SHA256, TREE, HEADER = 4, 16, 32
H3, Q3, H4, Q4 = 128, 256, 512, 1024
W, HC, HC3 = ss.WIDTH, ss.HELPER_COLS, sm.HELPER_COLS
CAP_H = 2
LB = 2  # blow-up 4 in the CPU tests


# ---- CPU: the model against the claim
def test_rows_satisfy_the_constraints_as_integers(skip4, step2, step3):
    """all 117 constraints hold as integer identities (no reduction mod p) on every row of T.3, T.5 and T.6 of skip N = 4, step N = 2 and
    step N = 3, rows cyclic; every helper value is below 2^34; the largest carry is printed and is at most 3; the selected constraint holds
    -- W(r + 1) + 2^32 CW(r) = Q_15(r) -- on every row with r mod 64 in 15 .. 62, of live and of zero blocks"""
    cw_max = rows_checked = 0
    for name, tables in (("skip4", skip4), ("step2", step2), ("step3", step3)):
        for sec, table in tables.items():
            n_proofs = table.shape[0] // W
            help_ = ss.helper(table, n_proofs)
            assert help_.shape == (n_proofs * HC, table.shape[1]) and int(help_.max()) < 1 << 34
            for p in range(n_proofs):
                t, h = table[p * W:(p + 1) * W], help_[p * HC:(p + 1) * HC]
                for j, c in enumerate(ss.integer_residuals(t, h)):
                    assert not c.any(), (name, sec, p, j, np.flatnonzero(c)[:4])
                cw = h[ss.HCW] + 2 * h[ss.HCW + 1]
                cw_max = max(cw_max, int(cw.max()))
                rows = np.array([r for r in range(t.shape[1]) if ss.schedule_row(r)])
                assert np.array_equal(t[ss.W_][rows + 1] + (cw[rows] << np.uint64(32)), h[ss.HQ + 15][rows])
                w = [int(x) for x in t[ss.W_]]
                for r in rows[::7]:  # the recurrence itself, written out
                    assert w[r + 1] == (ss.small_sigma1(w[r - 1]) + w[r - 6] + ss.small_sigma0(w[r - 14]) + w[r - 15]) & ss.MASK
                rows_checked += len(rows)
    print(f"\n[sha-sched] {rows_checked} schedule rows, largest carry {cw_max}")
    assert rows_checked and cw_max <= 3


def test_model_uint64_path_equals_python_integers(oracle):
    """one whole quotient of random columns through the uint64 field and through Python integers"""
    rng = np.random.default_rng(9500)
    ext, hext = rng.integers(0, 1 << 64, (W, 256), dtype=np.uint64), rng.integers(0, 1 << 64, (HC, 256), dtype=np.uint64)
    g = (0x0123456789ABCDEF % P, 0xFEDCBA9876543210 % P)
    assert np.array_equal(ss.quotient(oracle, 8, 1, 1, ext, hext, _shift(), g), ss.quotient(oracle, 8, 1, 1, ext, hext, _shift(), g, ints=True))


def _model_quotient(oracle, table, help_, log_blowup=LB):
    """(extended table, extended helper, gamma, planar quotient) of pre-LDE columns"""
    n_proofs, log_n = table.shape[0] // W, table.shape[1].bit_length() - 1 + log_blowup
    ext, hext = oracle.lde(table, log_blowup), oracle.lde(help_, log_blowup)
    g = ss.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _cap(oracle, ext, log_n), _cap(oracle, hext, log_n))
    return ext, hext, g, ss.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, _shift(), g)


@pytest.mark.parametrize("which", ["T.3 of skip N = 4", "T.5 of step N = 3"])
def test_quotient_is_a_polynomial_of_degree_below_n(oracle, skip4, step3, which):
    """two proofs, blow-up 4: the model quotient of the honest tables interpolates to degree < N in both planes (expected N - 2), and the
    identity holds at a zeta outside the base field; it fails after bumping u_0, a table opening or a helper opening"""
    table = skip4[SHA256] if which.startswith("T.3") else step3[TREE]
    N = table.shape[1]
    assert N == 512
    log_n, n_proofs = N.bit_length() - 1 + LB, table.shape[0] // W
    help_ = ss.helper(table, n_proofs)
    ext, hext, g, quot = _model_quotient(oracle, table, help_)
    deg = _degrees(oracle, quot)
    print(f"\n[sha-sched] {which}: N = {N}, quotient degrees {deg}")
    assert max(deg) < N and g[1] != 0
    M = 1 << log_n
    zeta = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)
    zs = (zeta, fm.e_scale(zeta, oracle.gl_root(log_n - LB)))
    yt, yh = dm.evaluate(oracle, table, 1, zs), dm.evaluate(oracle, help_, 1, zs)
    u = [am.horner(am.coefficients(oracle, quot[k * M:(k + 1) * M], _shift()), zeta) for k in (0, 1)]
    t0, t1, h0, h1 = [tuple(y[0]) for y in yt], [tuple(y[1]) for y in yt], [tuple(y[0]) for y in yh], [tuple(y[1]) for y in yh]
    ident = lambda t0=t0, t1=t1, h0=h0, h1=h1, u0=u[0]: ss.identity_at(oracle, log_n, LB, n_proofs, t0, t1, h0, h1, u0, u[1], zeta, g)
    assert ident()
    assert not ident(u0=fm.e_add(u[0], (1, 0)))
    bump = lambda v, at: v[:at] + [fm.e_add(v[at], (0, 1))] + v[at + 1:]
    assert not ident(t0=bump(t0, W + ss.W_)) and not ident(t1=bump(t1, ss.W_))
    assert not ident(h0=bump(h0, ss.HX1 + 7)) and not ident(h1=bump(h1, HC + ss.HQ + 4))


def _reschedule(t, r0):
    """W_16 .. W_63 of the block at r0 recomputed from its first sixteen words"""
    w = [int(x) for x in t[ss.W_, r0:r0 + 16]]
    for i in range(16, 64):
        w.append((ss.small_sigma1(w[i - 2]) + w[i - 7] + ss.small_sigma0(w[i - 15]) + w[i - 16]) & ss.MASK)
    t[ss.W_, r0:r0 + 64] = np.array(w, dtype=np.uint64)


RERUN = "a block re-run from a changed W_t, t >= 16"


def _tampered(table, kind):
    """(table, schedule helper) of ONE proof after a single change of `kind`"""
    t = table[:W].copy()
    r, r0 = tsa._mid_row(t)
    if kind in (RERUN, "a block re-run from a changed row-0 state"):
        t = tsa._tampered(table, kind)[0]
        return t, ss.helper(t, 1)
    if kind == "one W_t (t >= 16) changed alone":
        t[ss.W_, r0 + 20] ^= np.uint64(1 << 3)
        return t, ss.helper(t, 1)
    if kind == "a block re-run from a changed W_5, schedule and rounds recomputed":
        t[ss.W_, r0 + 5] ^= np.uint64(1 << 11)
        _reschedule(t, r0)
        t = tsa._rerun(t, r0, r0 + 5, r0 + 63)
        return t, ss.helper(t, 1)
    h = ss.helper(t, 1)
    if kind == "a flipped WB bit":
        h[ss.HWB + 5, r] ^= np.uint64(1)
    elif kind == "a flipped carry bit":
        h[ss.HCW, r] ^= np.uint64(1)
    elif kind == "a changed Q_9 on one row":
        h[ss.HQ + 9, r] += np.uint64(1)
    else:
        raise KeyError(kind)
    return t, h


DETECTED = [RERUN, "one W_t (t >= 16) changed alone", "a flipped WB bit", "a flipped carry bit", "a changed Q_9 on one row"]
UNDETECTED = ["a block re-run from a changed W_5, schedule and rounds recomputed", "a block re-run from a changed row-0 state"]


@pytest.mark.parametrize("kind", DETECTED)
def test_one_change_breaks_the_degree(oracle, skip4, kind):
    """the detected kinds, on T.3 of skip N = 4 (one proof): the quotient no longer interpolates to degree < N.  The first is the hole
    tests/test_sha_air.py records for set 3: the rows come from its `_tampered`, and set 3's own model quotient of them stays below N"""
    table = skip4[SHA256][:W]
    t, h = _tampered(table, kind)
    assert (t != table).sum() + (h != ss.helper(table, 1)).sum() >= 1
    deg = _degrees(oracle, _model_quotient(oracle, t, h)[3])
    print(f"\n[sha-sched] {kind}: quotient degrees {deg}, N = {table.shape[1]}")
    assert max(deg) >= table.shape[1]
    if kind == RERUN:
        assert kind in tsa.UNDETECTED and (t != table).sum() > 8
        deg3 = _degrees(oracle, tsa._model_quotient(oracle, t, sm.helper(t, 1))[3])
        print(f"[sha-sched] the same rows under set 3: quotient degrees {deg3}")
        assert max(deg3) < table.shape[1]


@pytest.mark.parametrize("kind", UNDETECTED)
def test_kinds_the_constraints_do_not_see(oracle, skip4, kind):
    """recorded so that nobody mistakes the claim: the first sixteen W against Level-1 and row 0 against the IV are in neither set -- a
    block re-run consistently (schedule AND rounds) from a changed W_5 or from a changed row-0 state keeps both quotients low-degree"""
    table = skip4[SHA256][:W]
    t, h = _tampered(table, kind)
    assert (t != table).sum() > 8
    assert max(_degrees(oracle, _model_quotient(oracle, t, h)[3])) < table.shape[1]
    assert max(_degrees(oracle, tsa._model_quotient(oracle, t, sm.helper(t, 1))[3])) < table.shape[1]


def test_symbols_and_wrappers_exist(built_lib):
    """the new entry points are in the built library, bound in _lib.py and wrapped in context.py"""
    from tendermintx_amd import _lib
    from tendermintx_amd.context import Context
    for name in ("tmx_air_sha256_sched_helper_device", "tmx_air_sha256_sched_quotient_device", "tmx_air_sha256_sched_verify_device",
                 "tmx_trace_commit_set_air_sha256_sched_device"):
        assert getattr(built_lib, name).argtypes, name
        assert callable(getattr(Context, name[4:])), name
    assert (_lib.AIR_SHA256_SCHED_HELPER_COLS, _lib.AIR_SHA256_SCHED_CONSTRAINTS) == (HC, ss.CONSTRAINTS)
    assert (_lib.TRACE_SHA256_SCHED_HELPER, _lib.TRACE_SHA256_SCHED_QUOTIENT) == (H4, Q4)


# ---- GPU
def _device_helper(ctx, table):
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    d_table = _up(table)
    return _guarded((n_proofs * HC) << log_rows, lambda out: ctx.air_sha256_sched_helper_device(log_rows, n_proofs, d_table.data_ptr(), out, 0))


def _helper_equals_the_model(ctx, table):
    n_proofs = table.shape[0] // W
    got = _down(_device_helper(ctx, table)).reshape(n_proofs * HC, -1)
    want = ss.helper(table, n_proofs)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs", [(6, 1), (6, 3), (8, 257), (12, 1)])
def test_helper_of_random_tables_equals_the_model(ctx, log_rows, n_proofs):
    """random 64-bit words: the helper equals the model's word for word, guard words intact; the wrap rows are looked at on their own: row
    0's Q_1 comes from the last row of the SAME proof"""
    rng = np.random.default_rng(9600 + 10 * log_rows + n_proofs)
    table = rng.integers(0, 1 << 64, (n_proofs * W, 1 << log_rows), dtype=np.uint64)
    want = _helper_equals_the_model(ctx, table)
    for p in (0, n_proofs - 1):
        w = table[p * W + ss.W_] & np.uint64(ss.MASK)
        assert int(want[p * HC + ss.HQ + 1, 0]) == int(w[-1]) + ss.small_sigma0(int(w[0]))
    cw = want[ss.HCW::HC] + 2 * want[ss.HCW + 1::HC]
    print(f"\n[sha-sched] log_rows {log_rows}, {n_proofs} proofs: largest carry {int(cw.max())}")
    assert int(cw.max()) == 3 or (n_proofs << log_rows) < 1024  # (four uniform words reach 3 * 2^32 once in 24 rows)
    assert not cw[:, [r for r in range(1 << log_rows) if not ss.schedule_row(r)]].any()


@pytest.mark.gpu
def test_helper_of_real_tree_rows_equals_the_model(ctx, step3):
    """the real T.5 rows of step N = 3 (two proofs, 512 rows with padding, zero blocks and chained second blocks)"""
    _helper_equals_the_model(ctx, step3[TREE])


@pytest.mark.gpu
@pytest.mark.parametrize("word", [0xFFFFFFFF, 0])
def test_helper_of_constant_tables(ctx, word):
    """W all 0xFFFFFFFF under random high words and in random other columns: the largest W there is, on every row.  Its carry follows from
    the definition: Q_15 = 2 (2^32 - 1) + sigma0(0xFFFFFFFF) + sigma1(0xFFFFFFFF) = 2 (2^32 - 1) + 0x1FFFFFFF + 0x003FFFFF, so CW = 2 on
    every schedule row and 0 elsewhere (the shifts of sigma0 and sigma1 clear the top bits: a constant table cannot reach 3; the random
    tables above do).  An all-zero table gives an all-zero helper"""
    rng = np.random.default_rng(9700)
    table = np.zeros((2 * W, 128), dtype=np.uint64)
    if word:
        table = rng.integers(0, 1 << 64, (2 * W, 128), dtype=np.uint64)
        table[ss.W_::W] |= np.uint64(word)
    carry = (2 * word + ss.small_sigma0(word) + ss.small_sigma1(word)) >> 32
    assert carry == (2 if word else 0)
    want = _helper_equals_the_model(ctx, table)
    cw = (want[ss.HCW::HC] + 2 * want[ss.HCW + 1::HC]).reshape(2, 128)
    assert np.array_equal(cw, np.tile(np.array([carry if ss.schedule_row(r) else 0 for r in range(128)], dtype=np.uint64), (2, 1)))
    assert word or not want.any()


def _device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, cap_height=CAP_H):
    return _guarded(2 << log_n, lambda out: ctx.air_sha256_sched_quotient_device(log_n, log_blowup, cap_height, n_proofs, d_cols.data_ptr(),
                                                                                d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(), out, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,log_blowup,n_proofs,cap_height", [(6, 1, 1, 0), (6, 1, 3, 2), (6, 3, 1, 2), (6, 3, 17, 0), (6, 6, 1, 2),
                                                                     (10, 1, 2, 2)])
def test_quotient_of_random_columns_equals_the_model(ctx, oracle, log_rows, log_blowup, n_proofs, cap_height):
    """N = 64 (one block: F's period is the whole domain) and N = 1024, random table and helper columns: the definition is pointwise, so
    d_quot and gamma equal the model word for word, guard words intact"""
    log_n = log_rows + log_blowup
    rng = np.random.default_rng(9800 + 100 * log_rows + 10 * log_blowup + n_proofs)
    ext, hext = _random_ext(rng, n_proofs * W, log_n), _random_ext(rng, n_proofs * HC, log_n)
    d_cols, d_hcols = _up(ext), _up(hext)
    _, d_cap = _tree(ctx, d_cols, log_n, n_proofs * W, cap_height)
    _, d_cap_h = _tree(ctx, d_hcols, log_n, n_proofs * HC, cap_height)
    got = _down(_device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, cap_height))
    g = ss.gamma(oracle, log_n, log_blowup, cap_height, n_proofs, _down(d_cap), _down(d_cap_h))
    assert ctx.air_last_gamma() == g
    want = ss.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


def _chain(ctx, oracle, table, log_blowup, quot_override=None, n_queries=6):
    """caller-level chain: helper -> LDE -> caps -> quotient -> one batch proof over [table, helper, quotient].  Returns (params, d_caps,
    proof words, extended table, extended helper, quotient words)"""
    import torch
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    log_n = log_rows + log_blowup
    d_help = _device_helper(ctx, table)
    d_ext, d_hext = _sentinel((n_proofs * W) << log_n), _sentinel((n_proofs * HC) << log_n)
    ctx.lde_device(log_rows, log_blowup, n_proofs * W, _up(table).data_ptr(), d_ext.data_ptr(), 0)
    ctx.lde_device(log_rows, log_blowup, n_proofs * HC, d_help.data_ptr(), d_hext.data_ptr(), 0)
    d_lv_t, d_cap_t = _tree(ctx, d_ext, log_n, n_proofs * W)
    d_lv_h, d_cap_h = _tree(ctx, d_hext, log_n, n_proofs * HC)
    d_quot = _device_quotient(ctx, log_n, log_blowup, n_proofs, d_ext, d_hext, d_cap_t, d_cap_h) if quot_override is None else _up(quot_override)
    d_lv_q, d_cap_q = _tree(ctx, d_quot, log_n, 2)
    p = bparams([log_n] * 3, [n_proofs * W, n_proofs * HC, 2], CAP_H, log_blowup, 2, 2, n_queries)
    proof = _guarded(bm.layout(p)["words"], lambda out: ctx.batch_prove_device(p, [d.data_ptr() for d in (d_ext, d_hext, d_quot)],
                                                                               [d.data_ptr() for d in (d_lv_t, d_lv_h, d_lv_q)], out, 0))
    return (p, torch.cat([d_cap_t, d_cap_h, d_cap_q]), _down(proof), _down(d_ext).reshape(n_proofs * W, -1),
            _down(d_hext).reshape(n_proofs * HC, -1), _down(d_quot))


def _verdicts(ctx, p, k_trace, k_helper, d_caps, proof):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=tsa._dev())
    ctx.air_sha256_sched_verify_device(p, k_trace, k_helper, d_caps.data_ptr(), _up(proof).data_ptr(), ok.data_ptr(), 0)
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
    """helper -> LDE -> caps -> quotient -> tmx_batch_prove_device -> tmx_air_sha256_sched_verify_device on the real T.3 and T.5 rows: the
    quotient and gamma equal the model's and the quotient has degree < N; every verdict equals the model verifier's (all accept); a proof
    with one bumped quotient or helper opening is rejected on every query"""
    table = skip4[SHA256] if which.startswith("T.3") else step3[TREE]
    n_proofs = table.shape[0] // W
    p, d_caps, got, ext, hext, quot = _chain(ctx, oracle, table, log_blowup)
    assert ctx.fri_last_degree_ok() is True
    log_n, caps, cw = p["log_n"][0], _down(d_caps), 4 << CAP_H
    assert np.array_equal(hext, oracle.lde(ss.helper(table, n_proofs), log_blowup))
    g = ss.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, caps[:cw], caps[cw:2 * cw])
    assert np.array_equal(quot, ss.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, _shift(), g))
    assert max(_degrees(oracle, quot)) < table.shape[1]
    model = ss.verify(oracle, p, 0, 1, caps, got, _shift())
    assert all(model) and _verdicts(ctx, p, 0, 1, d_caps, got) == model
    L = bm.layout(p)
    RH = 1 << dm.log_r(p["n_cols"][1])
    for name, at in (("quotient opening", L["off_open"][2] + 1), ("helper opening at zeta", L["off_open"][1] + ss.HX0 + 9),
                     ("helper opening at zeta omega", L["off_open"][1] + 2 * RH + HC + ss.HQ + 15),
                     ("table opening at zeta", L["off_open"][0] + ss.W_)):
        bad = _bumped(got, at)
        assert not ss.identity(oracle, p, 0, 1, caps, bad), name
        model = ss.verify(oracle, p, 0, 1, caps, bad, _shift())
        assert not any(model), name
        assert _verdicts(ctx, p, 0, 1, d_caps, bad) == model, name


@pytest.mark.gpu
def test_the_rerun_from_w20_is_rejected_and_set_3_still_accepts_it(ctx, oracle, skip4):
    """the table re-run from a changed W_20 (tests/test_sha_air.py's undetected kind), one proof, blow-up 4, with its HONEST quotients: set
    4's chain clears every verdict, as the model does -- the quotient is no polynomial of degree < N, so the proof over it fails -- while
    set 3's chain over the same rows with set 3's own helper still accepts every query"""
    table = skip4[SHA256][:W]
    t, _ = _tampered(table, RERUN)
    p, d_caps, got, _, _, quot = _chain(ctx, oracle, t, 2)
    assert max(_degrees(oracle, quot)) >= t.shape[1]
    model = ss.verify(oracle, p, 0, 1, _down(d_caps), got, _shift())
    assert not any(model) and _verdicts(ctx, p, 0, 1, d_caps, got) == model
    p3, d_caps3, got3, _, _, _ = tsa._chain(ctx, oracle, t, 2)
    assert all(tsa._verdicts(ctx, p3, 0, d_caps3, got3))


@pytest.mark.gpu
def test_zero_quotient_for_a_tampered_table(ctx, oracle, skip4):
    """a zero (low-degree) quotient committed for the same re-run table: the batch proof is fine and the identity fails -- every verdict is
    cleared by k_air_sched_check alone, as in the model"""
    t, _ = _tampered(skip4[SHA256][:W], RERUN)
    log_n = t.shape[1].bit_length() - 1 + 1
    p, d_caps, got, _, _, _ = _chain(ctx, oracle, t, 1, quot_override=np.zeros(2 << log_n, dtype=np.uint64))
    assert all(tsa._verdicts(ctx, p, 0, d_caps, got, batch_only=True))
    model = ss.verify(oracle, p, 0, 1, _down(d_caps), got, _shift())
    assert not any(model) and _verdicts(ctx, p, 0, 1, d_caps, got) == model


MANY = 257  # one proof more than k_air_sched_check has threads: thread 0 takes proofs 0 and 256


@pytest.mark.gpu
def test_257_proofs_through_the_check_kernel(ctx, oracle, skip4, step3):
    """N = 64, 257 proofs (the live blocks of the fixtures in turn, every seventh proof zero), blow-up 2, two queries: the device accepts
    every query as the model does; one helper opening bumped in proof 256, one in proof 200 and the table's in proof 255 are each rejected"""
    blocks = np.concatenate([t[p * W:(p + 1) * W].reshape(W, -1, 64).transpose(1, 0, 2) for t in (skip4[SHA256], step3[TREE])
                             for p in range(t.shape[0] // W)])
    blocks = blocks[blocks.any(axis=(1, 2))]
    table = np.zeros((MANY * W, 64), dtype=np.uint64)
    for q in range(MANY):
        if q % 7 != 6:
            table[q * W:(q + 1) * W] = blocks[q % len(blocks)]
    p, d_caps, got, ext, hext, _ = _chain(ctx, oracle, table, 1, n_queries=2)
    assert ctx.fri_last_degree_ok() is True
    assert np.array_equal(hext, oracle.lde(ss.helper(table, MANY), 1))
    caps = _down(d_caps)
    assert ss.identity(oracle, p, 0, 1, caps, got)
    assert _verdicts(ctx, p, 0, 1, d_caps, got) == [True, True]
    L = bm.layout(p)
    for at in (L["off_open"][1] + 256 * HC + ss.HX1 + 3, L["off_open"][1] + 200 * HC + ss.HQ + 2, L["off_open"][0] + 255 * W + ss.W_):
        bad = _bumped(got, at)
        assert not ss.identity(oracle, p, 0, 1, caps, bad)
        assert _verdicts(ctx, p, 0, 1, d_caps, bad) == [False, False]


# ---- the set level
@pytest.fixture(scope="module")
def header_sets(built_lib, oracle):
    """a set SHA256 + HEADER at step N = 2, two proofs (the shape of test_sha_air.test_set_level_on_the_header_table), three ways: set 4
    alone on HEADER, set 3 then set 4, set 4 then set 3.  Per way: (shape, section_of, caps of every oracle in order, proof words, verdicts)"""
    import torch
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    kind, n, n_proofs, lb = 1, 2, 2, 1
    cw = 4 << CAP_H
    out = {}
    with tmx.Context(n, b"celestia", max_batch=n_proofs) as c:
        tr = _trace_rows(c, kind, n, n_proofs, 9300)
        out["traces"] = _down(tr)
        for way in ("4", "34", "43"):
            d_caps = _sentinel(2 * cw)
            c.trace_commit_set_device(kind, n_proofs, SHA256 | HEADER, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
            pair, gammas = {}, {}
            for s in way:
                pair[s] = (_sentinel(cw), _sentinel(cw))
                call = c.trace_commit_set_air_sha256_device if s == "3" else c.trace_commit_set_air_sha256_sched_device
                call(HEADER, pair[s][0].data_ptr(), pair[s][1].data_ptr(), 0)
                gammas[s] = c.air_last_gamma()
            shape, order = c.trace_commit_set_shape()
            p = dict(shape, arity_bits=2, final_log_max=2, n_queries=6, pow_bits=0)
            proof = _guarded(bm.layout(p)["words"], lambda o: c.trace_commit_set_prove_device(p, o, 0))
            assert c.fri_last_degree_ok() is True
            all_caps = torch.cat([d_caps[:cw]] + [x for s in sorted(way) for x in pair[s]] + [d_caps[cw:]])
            k4 = order.index(H4)
            v = dict(sched=_verdicts(c, p, 0, k4, all_caps, _down(proof)), batch=tsa._verdicts(c, p, 0, all_caps, _down(proof), batch_only=True))
            if "3" in way:
                v["sha"] = tsa._verdicts(c, p, 0, all_caps, _down(proof))
            bad = _bumped(_down(proof), bm.layout(p)["off_open"][k4 + 1])
            v["bad"] = _verdicts(c, p, 0, k4, all_caps, bad)
            if way == "4":  # the model's helper cap through the device's tree, as tests/test_sha_air.py does
                off, rows, _ = tsa._section_geom(kind, n, HEADER)
                table = np.zeros((n_proofs * W, 1 << 12), dtype=np.uint64)
                for q, full in enumerate(out["traces"]):
                    table[q * W:(q + 1) * W, :rows] = full[off:off + rows * W].reshape(rows, W).T
                out["hext"] = oracle.lde(ss.helper(table, n_proofs), lb)
                out["cap_h_model"] = _down(_tree(c, _up(out["hext"]), 12 + lb, n_proofs * HC)[1])
            out[way] = dict(p=p, order=order, caps=_down(all_caps), proof=_down(proof), verdicts=v, gammas=gammas)
    return out


@pytest.mark.gpu
def test_set_level_with_set_4_alone(oracle, header_sets):
    """three oracles behind each other -- section_of ends 32, 512, 1024 with SHA256 behind -- the helper's cap, gamma and the quotient's
    cap against the model, the device verifier and the model's on the proof over the four oracles, tmx_batch_verify_device against
    tests/batch_model.py"""
    from test_merkle_open import _oracle_ext
    s, lb, n_proofs, cw = header_sets["4"], 1, 2, 4 << CAP_H
    assert s["order"] == [HEADER, H4, Q4, SHA256]
    assert s["p"]["log_n"] == [12 + lb] * 3 + [7 + lb] and s["p"]["n_cols"] == [W * n_proofs, HC * n_proofs, 2, W * n_proofs]
    caps = s["caps"]
    e, lm, nc = _oracle_ext(oracle, 1, 2, header_sets["traces"], HEADER, lb)
    ext = e.reshape(nc, -1)
    assert np.array_equal(caps[:cw], _cap(oracle, ext, lm))
    assert np.array_equal(caps[cw:2 * cw], header_sets["cap_h_model"])
    g = ss.gamma(oracle, lm, lb, CAP_H, n_proofs, caps[:cw], caps[cw:2 * cw])
    assert s["gammas"]["4"] == g
    quot = ss.quotient(oracle, lm, lb, n_proofs, ext, header_sets["hext"], _shift(), g)
    assert np.array_equal(caps[2 * cw:3 * cw], _cap(oracle, quot.reshape(2, -1), lm))
    assert s["verdicts"]["batch"] == bm.verify(oracle, s["p"], caps, s["proof"], _shift())
    model = ss.verify(oracle, s["p"], 0, 1, caps, s["proof"], _shift())
    assert all(model) and s["verdicts"]["sched"] == model and not any(s["verdicts"]["bad"])


@pytest.mark.gpu
def test_set_level_in_both_orders_with_set_3(oracle, header_sets):
    """set 3 then set 4 and set 4 then set 3 end as table, H3, Q3, H4, Q4, SHA256: the same section_of, the same caps and the same proof word
    for word; set 4's caps are those of the set with set 4 alone; both device verifiers accept it, both model identities hold, and
    tmx_batch_verify_device equals tests/batch_model.py"""
    a, b, alone, cw = header_sets["34"], header_sets["43"], header_sets["4"], 4 << CAP_H
    assert a["order"] == b["order"] == [HEADER, H3, Q3, H4, Q4, SHA256]
    assert a["p"] == b["p"] and a["p"]["n_cols"][:5] == [2 * W, 2 * HC3, 2, 2 * HC, 2]
    assert np.array_equal(a["caps"], b["caps"]) and np.array_equal(a["proof"], b["proof"])
    assert np.array_equal(a["caps"][3 * cw:5 * cw], alone["caps"][cw:3 * cw]) and a["gammas"]["4"] == b["gammas"]["4"] == alone["gammas"]["4"]
    for s in (a, b):
        assert all(s["verdicts"]["sha"]) and all(s["verdicts"]["sched"]) and all(s["verdicts"]["batch"]) and not any(s["verdicts"]["bad"])
    assert a["verdicts"]["batch"] == bm.verify(oracle, a["p"], a["caps"], a["proof"], _shift())
    assert ss.identity(oracle, a["p"], 0, 3, a["caps"], a["proof"]) and sm.identity(oracle, a["p"], 0, a["caps"], a["proof"])


@pytest.mark.gpu
def test_set_level_refusals(built_lib):
    """before a set, a section that is no SHA-256 table, an absent section, null caps, a second call (behind the table and behind set 3's
    pair), a streamed member: TMX_ERR_BAD_ARG, nothing written, the set's shape as it was"""
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    kind, n, n_proofs, lb = 1, 2, 2, 1
    cw = 4 << CAP_H
    with tmx.Context(n, b"celestia", max_batch=n_proofs) as c:
        tr = _trace_rows(c, kind, n, n_proofs, 9300)
        d_caps, d_cap_h, d_cap_q = _sentinel(2 * cw), _sentinel(cw), _sentinel(cw)
        air = lambda sec: (lambda: c.trace_commit_set_air_sha256_sched_device(sec, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0))
        assert "no commit set" in _refused(air(HEADER), d_cap_h, d_cap_q)
        c.trace_commit_set_device(kind, n_proofs, SHA256 | HEADER, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        before = c.trace_commit_set_shape()
        for sec in (TREE, 1, H3, H4, Q4, 0):
            _refused(air(sec), d_cap_h, d_cap_q)
        _refused(lambda: c.trace_commit_set_air_sha256_sched_device(HEADER, None, d_cap_q.data_ptr(), 0), d_cap_q)
        _refused(lambda: c.trace_commit_set_air_sha256_sched_device(HEADER, d_cap_h.data_ptr(), None, 0), d_cap_h)
        assert c.trace_commit_set_shape() == before
        a, b = _sentinel(cw), _sentinel(cw)
        c.trace_commit_set_air_sha256_sched_device(SHA256, a.data_ptr(), b.data_ptr(), 0)
        assert c.trace_commit_set_shape()[1] == [HEADER, SHA256, H4, Q4]
        assert "already" in _refused(air(SHA256), d_cap_h, d_cap_q)
        c.trace_commit_set_air_sha256_device(SHA256, a.data_ptr(), b.data_ptr(), 0)
        assert c.trace_commit_set_shape()[1] == [HEADER, SHA256, H3, Q3, H4, Q4]
        assert "already" in _refused(air(SHA256), d_cap_h, d_cap_q)
        c.trace_commit_set_streamed_device(kind, n_proofs, SHA256 | HEADER, HEADER, 8, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        assert "streamed" in _refused(air(HEADER), d_cap_h, d_cap_q)


@pytest.mark.gpu
def test_a_full_set_is_refused(built_lib):
    """all five tables and the ladders' quotient are six oracles; one schedule pair makes eight; a second pair would exceed eight"""
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    cw = 4 << CAP_H
    with tmx.Context(4, b"celestia", max_batch=1) as c:
        tr = _trace_rows(c, 0, 4, 1, 9400)
        d_caps, d_cap_h, d_cap_q = _sentinel(5 * cw), _sentinel(cw), _sentinel(cw)
        c.trace_commit_set_device(0, 1, 1 | 2 | SHA256 | TREE | HEADER, 1, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        c.trace_commit_set_air_device(d_cap_q.data_ptr(), 0)
        c.trace_commit_set_air_sha256_sched_device(TREE, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
        _, order = c.trace_commit_set_shape()
        assert len(order) == 8 and order[order.index(TREE) + 1:order.index(TREE) + 3] == [H4, Q4]
        assert "room" in _refused(lambda: c.trace_commit_set_air_sha256_sched_device(SHA256, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0),
                                  d_cap_h, d_cap_q)


@pytest.mark.gpu
def test_each_validation_rule(ctx):
    """every rule of the three caller-level calls on its own: TMX_ERR_BAD_ARG before anything is enqueued, nothing written"""
    import torch
    log_n, lb = 8, 1
    d_cols, d_hcols = _sentinel(W << log_n), _sentinel(HC << log_n)
    d_cap, d_cap_h, d_quot = _sentinel(4 << CAP_H), _sentinel(4 << CAP_H), _sentinel(2 << log_n)
    ptrs = [d_cols.data_ptr(), d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(), d_quot.data_ptr()]
    q = lambda ln, b, n, a=ptrs: (lambda: ctx.air_sha256_sched_quotient_device(ln, b, CAP_H, n, *a, 0))
    for fn in (q(log_n, 0, 1), q(log_n, 7, 1), q(2, 2, 1), q(29, 2, 1), q(6, 1, 1), q(11, 6, 1), q(log_n, lb, 0), q(log_n, lb, (1 << 24) // HC + 1)):
        _refused(fn, d_quot)
    for k in range(5):
        _refused(q(log_n, lb, 1, ptrs[:k] + [None] + ptrs[k + 1:]), d_quot)
    d_table, d_help = _sentinel(W << 7), _sentinel(HC << 7)
    hp = lambda lr, n, t=d_table.data_ptr(), o=d_help.data_ptr(): (lambda: ctx.air_sha256_sched_helper_device(lr, n, t, o, 0))
    for fn in (hp(5, 1), hp(28, 1), hp(7, 0), hp(7, (1 << 24) // HC + 1), hp(7, 1, t=None), hp(7, 1, o=None)):
        _refused(fn, d_help)
    # the verifier: column counts 9 k / 115 k / 2, equal log_n, k_trace < k_helper, k_helper + 1 inside the proof
    ok, caps, proof = torch.full((4,), 7, dtype=torch.int32, device=tsa._dev()), _sentinel(256), _sentinel(1 << 16)
    v = lambda p, kt, kh: (lambda: ctx.air_sha256_sched_verify_device(p, kt, kh, caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0))
    good = bparams([8, 8, 8], [W, HC, 2], CAP_H, lb, 2, 2, 4)
    for p, kt, kh in ((good, 0, 2), (good, 0, 0), (good, 1, 1), (good, 1, 0), (dict(good, n_cols=[W + 1, HC, 2]), 0, 1),
                      (dict(good, n_cols=[W, HC + 1, 2]), 0, 1), (dict(good, n_cols=[W, HC3, 2]), 0, 1), (dict(good, n_cols=[2 * W, HC, 2]), 0, 1),
                      (dict(good, n_cols=[W, HC, 3]), 0, 1), (dict(good, log_n=[8, 8, 7]), 0, 1), (dict(good, log_n=[8, 7, 8]), 0, 1),
                      (bparams([6, 6, 6], [W, HC, 2], CAP_H, lb, 2, 2, 4), 0, 1), (dict(good, arity_bits=0), 0, 1),
                      (bparams([8, 8], [W, HC], CAP_H, lb, 2, 2, 4), 0, 1)):
        _refused(v(p, kt, kh), ok)
