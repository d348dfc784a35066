"""The message schedule of the SHA-512 table (include/tmx.h "the message schedule of the SHA-512 table", constraint set 8):
tmx_air_sha512_sched_helper_device, tmx_air_sha512_sched_quotient_device and its range form, tmx_air_sha512_sched_verify_device,
tmx_trace_commit_set_air_sha512_sched_device, and the two calls that show the preprocessed column SCH on its own.  The yardstick is
tests/sha512_sched_model.py on top of tests/batch_model.py: device words must equal the model's word for word and every verdict of the
device verifier must equal the model verifier's.  The CPU part ties the model itself to the claim: on the CPU oracle's T.2 rows all 234
constraints hold as integer identities and W_16 .. W_79 of every live block are the schedule of its first sixteen words, the quotient is a
polynomial of degree <= N - 2, one change of a detected kind makes it one of degree >= N -- among them the block re-run from a changed W_20
that set 7 alone accepts --, and the kind sets 7 + 8 do NOT see is recorded next to them."""
import hashlib

import numpy as np
import pytest

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha512_air_model as s7
import sha512_sched_model as sm
import test_sha512_air as t7
from batch_model import bparams
from test_fri import _down, _sentinel, _shift, _up
from test_sha512_air import IV512, _mid_row, _tampered, _word, device_rows, skip4, step2, step3  # noqa: F401
from test_sha_air import GUARD, _cap, _degrees, _dev, _guarded, _random_ext, _refused, _tree
from test_sha_air_shapes import FILLS

P = fm.P
SHA512, SHA256, HEADER = 2, 4, 32
H7, Q7, HELPER, QUOTIENT = 32768, 65536, 131072, 262144
W, HC, HC7 = sm.WIDTH, sm.HELPER_COLS, s7.HELPER_COLS
CAP_H = 2
LB = 2  # blow-up 4 in the CPU tests
RERUN = "a block re-run from a changed W_t, t >= 16"


def _schedule(w16):
    """W_0 .. W_79 in plain integers from the sixteen message words"""
    w = list(w16)
    for k in range(16, 80):
        w.append((sm.small_sigma1(w[k - 2]) + w[k - 7] + sm.small_sigma0(w[k - 15]) + w[k - 16]) & sm.M64)
    return w


# ---- CPU
def test_rows_satisfy_the_constraints_as_integers(skip4, step2, step3):
    """all 234 constraints hold as integer identities (no reduction mod p) on every row of T.2 of skip N = 4, step N = 2 and step N = 3, with
    every helper value below 2^34 and every bit column in {0, 1}; the largest CL and CH are printed and stay <= 3; for every live block
    W_16 .. W_79 recomputed in plain integers from W_0 .. W_15 equal the table"""
    live_blocks = zero_blocks = 0
    cmax = [0, 0]
    bits = list(range(sm.HWB, sm.HG0)) + list(range(sm.HCL, sm.HELPER_COLS))
    for name, table in (("skip4", skip4), ("step2", step2), ("step3", step3)):
        n_proofs, N = table.shape[0] // W, table.shape[1]
        help_ = sm.helper(table, n_proofs)
        assert help_.shape == (n_proofs * HC, N) and int(help_.max()) < 1 << 34
        for p in range(n_proofs):
            t, h = table[p * W:(p + 1) * W], help_[p * HC:(p + 1) * HC]
            assert int(h[bits].max()) <= 1
            for j, c in enumerate(sm.integer_residuals(t, h)):
                assert not c.any(), (name, p, j, np.flatnonzero(c)[:4])
            for b in range(N // 80):
                r0 = 80 * b
                nonzero = bool(t[:, r0].any())
                live_blocks, zero_blocks = live_blocks + nonzero, zero_blocks + (not nonzero)
                if nonzero:
                    w = _schedule([_word(t, sm.W_, r0 + k) for k in range(16)])
                    assert [_word(t, sm.W_, r0 + k) for k in range(80)] == w, (name, p, b)
            cmax[0] = max(cmax[0], int((h[sm.HCL] + 2 * h[sm.HCL + 1]).max()))
            cmax[1] = max(cmax[1], int((h[sm.HCH] + 2 * h[sm.HCH + 1]).max()))
    print(f"\n[sha512-sched] live blocks {live_blocks}, zero blocks {zero_blocks}, largest carries CL {cmax[0]} CH {cmax[1]}")
    assert live_blocks and zero_blocks and max(cmax) <= 3


def test_schedule_model_against_hashlib():
    """the plain sigma0 / sigma1 the test above leans on are SHA-512's: one padded block, scheduled by them and compressed by the round
    function of tests/sha512_air_model.py, against hashlib"""
    msg = b"abc"
    block = msg + b"\x80" + bytes(128 - len(msg) - 1 - 16) + (8 * len(msg)).to_bytes(16, "big")
    w = _schedule([int.from_bytes(block[8 * k:8 * k + 8], "big") for k in range(16)])
    state = list(IV512)
    for k in range(80):
        state = s7.sha_round(state, w[k], k)
    digest = b"".join(((a + b) & sm.M64).to_bytes(8, "big") for a, b in zip(IV512, state))
    assert digest == hashlib.sha512(msg).digest()


def test_sch_has_full_degree_and_barycentric_equals_horner(oracle):
    """SCH interpolates to degree N - 1 = 127 at N = 128, which is why no subgroup selector stands in for it; the model's barycentric
    SCH(zeta) at a zeta outside the base field equals Horner on the interpolated coefficients; the wrap row is off at every size"""
    zeta = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)
    col = sm.periodic(128)
    coef = am.coefficients(oracle, col, 1)
    assert am.degree(coef) == 127
    assert sm.sch_at(oracle, 7, zeta) == am.horner(coef, zeta)
    for log_rows in range(7, 19):
        N = 1 << log_rows
        sch = sm.periodic(N)
        assert sch[N - 1] == 0 and (N - 1) % 80 == {3: 47, 0: 15, 1: 31, 2: 63}[log_rows % 4]
        assert sch[:80].tolist() == [0] * 15 + [1] * 64 + [0] and int(sch.sum()) == 64 * (N // 80) + (N - 1) % 80 - 15


def _model_quotient(oracle, table, help_, log_blowup=LB, pre=None):
    """(extended table, extended helper, gamma, planar quotient) of pre-LDE columns"""
    n_proofs, log_n = table.shape[0] // W, table.shape[1].bit_length() - 1 + log_blowup
    ext, hext = oracle.lde(table, log_blowup), oracle.lde(help_, log_blowup)
    pext = oracle.lde((sm.periodic(table.shape[1]) if pre is None else pre).reshape(1, -1), log_blowup)
    g = sm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _cap(oracle, ext, log_n), _cap(oracle, hext, log_n))
    return ext, hext, g, sm.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, pext, _shift(), g)


def test_quotient_is_a_polynomial_of_degree_at_most_n_minus_2(oracle, step2):
    """T.2 of step N = 2 (one proof, N = 512), blow-up 4: the model quotient interpolates to degree <= N - 2 in both planes, and the
    identity holds at a zeta outside the base field -- table, helper and quotient evaluated there by Horner on their coefficients, SCH
    barycentrically; it fails after bumping u_0, a table opening (W_lo at zeta, W_hi at zeta omega) or a helper opening (an X1 bit, QH_9 at
    zeta omega)"""
    table = step2[:W]
    N = table.shape[1]
    assert N == 512
    log_n, n_proofs = 9 + LB, 1
    help_ = sm.helper(table, n_proofs)
    ext, hext, g, quot = _model_quotient(oracle, table, help_)
    deg = _degrees(oracle, quot)
    print(f"\n[sha512-sched] T.2 of step N = 2: N = {N}, quotient degrees {deg}")
    assert max(deg) <= N - 2 and g[1] != 0
    M = 1 << log_n
    zeta = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)
    zs = (zeta, fm.e_scale(zeta, oracle.gl_root(log_n - LB)))
    yt, yh = dm.evaluate(oracle, table, 1, zs), dm.evaluate(oracle, help_, 1, zs)
    u = [am.horner(am.coefficients(oracle, quot[k * M:(k + 1) * M], _shift()), zeta) for k in (0, 1)]
    t0, t1, h0, h1 = [tuple(y[0]) for y in yt], [tuple(y[1]) for y in yt], [tuple(y[0]) for y in yh], [tuple(y[1]) for y in yh]
    pre = sm.sch_at(oracle, 9, zeta)
    ident = lambda t0=t0, t1=t1, h0=h0, h1=h1, u0=u[0]: sm.identity_at(oracle, log_n, LB, n_proofs, t0, t1, h0, h1, u0, u[1], zeta, g, pre)
    assert ident()
    assert not ident(u0=fm.e_add(u[0], (1, 0)))
    bump = lambda v, at: v[:at] + [fm.e_add(v[at], (0, 1))] + v[at + 1:]
    assert not ident(t0=bump(t0, sm.W_)) and not ident(t1=bump(t1, sm.W_ + 1))
    assert not ident(h0=bump(h0, sm.HX1 + 40)) and not ident(h1=bump(h1, sm.HQH + 9))


def test_model_quotient_in_integers_equals_the_uint64_field(oracle):
    """the model's two arithmetics agree on random, non-satisfying columns with a few non-canonical words (N = 128, blow-up 2, two
    proofs): Python integers in object arrays against the vectorised uint64 field the GPU tests are compared with"""
    log_n, lb, n_proofs = 8, 1, 2
    rng = np.random.default_rng(10050)
    ext, hext = _random_ext(rng, n_proofs * W, log_n), _random_ext(rng, n_proofs * HC, log_n)
    pext = oracle.lde(sm.periodic(128).reshape(1, -1), lb)
    g = (0x0123456789ABCDEF % P, 0x0FEDCBA987654321 % P)
    fast = sm.quotient(oracle, log_n, lb, n_proofs, ext, hext, pext, _shift(), g)
    assert np.array_equal(fast, sm.quotient(oracle, log_n, lb, n_proofs, ext, hext, pext, _shift(), g, ints=True))


def _changed(table, kind):
    """(table, helper, SCH) of ONE proof after a single change of `kind`"""
    t = table[:W].copy()
    r, r0 = _mid_row(t)
    sch = sm.periodic(t.shape[1])
    if kind == "a changed W_lo, t >= 16":
        t[sm.W_, r] ^= np.uint64(1 << 9)
        return t, sm.helper(t, 1), sch
    if kind == "a changed W_hi, t >= 16":
        t[sm.W_ + 1, r] ^= np.uint64(1 << 9)
        return t, sm.helper(t, 1), sch
    h = sm.helper(t, 1)
    if kind == "a flipped WB bit":
        h[sm.HWB + 37, r] ^= np.uint64(1)
    elif kind == "a flipped X0 bit":
        h[sm.HX0 + 12, r] ^= np.uint64(1)
    elif kind == "a changed G1_hi":
        h[sm.HG1 + 1, r] ^= np.uint64(1 << 5)
    elif kind == "a changed QL_7":
        h[sm.HQL + 7, r] += np.uint64(1)
    elif kind == "a flipped CL bit":
        h[sm.HCL, r] ^= np.uint64(1)
    elif kind == "a flipped CH bit":
        h[sm.HCH + 1, r] ^= np.uint64(1)
    elif kind == "SCH left 1 on row N - 1":
        sch[-1] = 1
    elif kind == "SCH left 1 on the last row of a block":
        sch[r0 + 79] = 1
    else:
        raise KeyError(kind)
    return t, h, sch


DETECTED = ["a changed W_lo, t >= 16", "a changed W_hi, t >= 16", "a flipped WB bit", "a flipped X0 bit", "a changed G1_hi", "a changed QL_7",
            "a flipped CL bit", "a flipped CH bit", "SCH left 1 on row N - 1", "SCH left 1 on the last row of a block"]


@pytest.mark.parametrize("kind", DETECTED)
def test_one_change_breaks_the_degree(oracle, step2, kind):
    """the detected kinds, on T.2 of step N = 2 (one proof): the first two change W on row 37 of a live block and regenerate the helper from
    the changed table, the next six change the helper alone, the last two leave SCH on where it must be off -- at the wrap row, behind which
    row 0 is W_0 of a live block, and on the last row of a live block, behind which stands W_0 of the next.  The quotient no longer
    interpolates to degree < N"""
    table = step2[:W]
    t, h, sch = _changed(table, kind)
    assert (t != table).sum() + (h != sm.helper(table, 1)).sum() + (sch != sm.periodic(table.shape[1])).sum() >= 1
    deg = _degrees(oracle, _model_quotient(oracle, t, h, pre=sch)[3])
    print(f"\n[sha512-sched] {kind}: quotient degrees {deg}, N = {table.shape[1]}")
    assert max(deg) >= table.shape[1]


def test_the_rerun_block_set_7_accepts_is_rejected(oracle, step2):
    """the kind tests/test_sha512_air.py records as unseen by set 7: a block re-run consistently through the round function from a changed
    W_20.  Set 7's model quotient of that table still has degree <= N - 2; set 8's, with its helper regenerated from the tampered table, has
    degree >= N: the pair of facts side by side"""
    table = step2[:W]
    t, h7, pre7 = _tampered(table, RERUN)
    N = table.shape[1]
    assert (t != table).sum() > 8
    deg7 = _degrees(oracle, t7._model_quotient(oracle, t, h7, pre=pre7)[3])
    deg8 = _degrees(oracle, _model_quotient(oracle, t, sm.helper(t, 1))[3])
    print(f"\n[sha512-sched] {RERUN}: set 7's quotient degrees {deg7}, set 8's {deg8}, N = {N}")
    assert max(deg7) <= N - 2 and max(deg8) >= N


def test_kinds_sets_7_and_8_do_not_see(oracle, step2):
    """recorded so that nobody mistakes the claim: the message is not linked to anything public -- W_3 of a live block changed and
    W_16 .. W_79 recomputed from it keeps set 8's quotient at degree <= N - 2 (the state columns are not set 8's concern)"""
    table = step2[:W]
    t = table.copy()
    _, r0 = _mid_row(t)
    w16 = [_word(t, sm.W_, r0 + k) for k in range(16)]
    w16[3] ^= 1 << 40
    for k, x in enumerate(_schedule(w16)):
        t[sm.W_, r0 + k], t[sm.W_ + 1, r0 + k] = x & sm.M32, x >> 32
    assert (t != table).sum() > 64
    assert max(_degrees(oracle, _model_quotient(oracle, t, sm.helper(t, 1))[3])) <= table.shape[1] - 2


def test_symbols_and_wrappers_exist(built_lib):
    """the new entry points are in the built library, bound in _lib.py and wrapped in context.py; the four constants are the model's"""
    from tendermintx_amd import _lib
    from tendermintx_amd.context import Context
    for name in ("tmx_air_sha512_sched_helper_device", "tmx_air_sha512_sched_quotient_device", "tmx_air_sha512_sched_quotient_range_device",
                 "tmx_air_sha512_sched_verify_device", "tmx_trace_commit_set_air_sha512_sched_device", "tmx_air_sha512_sched_periodic_device",
                 "tmx_air_sha512_sched_periodic_eval_device"):
        assert getattr(built_lib, name).argtypes, name
    for name in ("air_sha512_sched_helper_device", "air_sha512_sched_quotient_device", "air_sha512_sched_verify_device",
                 "trace_commit_set_air_sha512_sched_device", "air_sha512_sched_periodic_device", "air_sha512_sched_periodic_eval_device"):
        assert callable(getattr(Context, name)), name
    assert (_lib.AIR_SHA512_SCHED_HELPER_COLS, _lib.AIR_SHA512_SCHED_CONSTRAINTS) == (HC, sm.CONSTRAINTS)
    assert (_lib.TRACE_SHA512_SCHED_HELPER, _lib.TRACE_SHA512_SCHED_QUOTIENT) == (HELPER, QUOTIENT)


# ---- GPU
@pytest.fixture(scope="module")
def ctx(built_lib):
    import tendermintx_amd as tmx
    c = tmx.Context(2, b"celestia", max_batch=2)
    yield c
    c.close()


def _device_helper(ctx, table):
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    d_table = _up(table)
    return _guarded((n_proofs * HC) << log_rows, lambda out: ctx.air_sha512_sched_helper_device(log_rows, n_proofs, d_table.data_ptr(), out, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs", [(7, 1), (7, 3), (8, 1), (8, 3), (9, 1), (9, 3), (10, 1), (10, 3), (7, 257)])
def test_helper_of_random_tables_equals_the_model(ctx, log_rows, n_proofs):
    """random tables of full 64-bit words (the operands are the low 32 bits) at the four residues of (N - 1) mod 80 -- at N = 256 the wrap
    row sits on the first index where SCH could be 1 --, one and three proofs (3 x 128 lanes end in a partial workgroup) and 257 proofs: the
    helper equals the model's word for word, so the sixteen-row window wraps inside its own proof; guard words intact"""
    rng = np.random.default_rng(10100 + 10 * log_rows + n_proofs)
    table = rng.integers(0, 1 << 64, (n_proofs * W, 1 << log_rows), dtype=np.uint64)
    got = _down(_device_helper(ctx, table)).reshape(n_proofs * HC, -1)
    want = sm.helper(table, n_proofs)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    carries = want[sm.HCL::HC] + 2 * want[sm.HCL + 1::HC], want[sm.HCH::HC] + 2 * want[sm.HCH + 1::HC]
    assert all(int(c.max()) == 3 and not c[:, -1].any() and not c[:, :15].any() for c in carries)


@pytest.mark.gpu
def test_helper_of_the_devices_own_rows_equals_the_model(ctx, device_rows):
    """T.2 of two step N = 2 proofs as tmx_trace_rows_device writes it (512 rows: live and zero blocks, padding)"""
    table = device_rows[1]
    assert table.shape == (2 * W, 512) and table.any()
    got = _down(_device_helper(ctx, table)).reshape(-1, 512)
    assert np.array_equal(got, sm.helper(table, 2))


def _periodic(ctx, log_rows, log_blowup):
    import torch
    N, M = 1 << log_rows, 1 << (log_rows + log_blowup)
    d_pre, d_ext = _sentinel(N + GUARD), _sentinel(M + GUARD)
    ctx.air_sha512_sched_periodic_device(log_rows, log_blowup, d_pre.data_ptr(), d_ext.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(d_pre[N:], _sentinel(GUARD)) and torch.equal(d_ext[M:], _sentinel(GUARD))
    return _down(d_pre[:N]), _down(d_ext[:M])


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,log_blowup", [(7, 1), (7, 6), (8, 2), (9, 3)])
def test_sch_and_its_extension(ctx, oracle, log_rows, log_blowup):
    """SCH before the LDE (1 << log_rows words, nothing behind them) and extended under the context's domain, against the model and the
    CPU oracle's LDE"""
    pre, ext = _periodic(ctx, log_rows, log_blowup)
    want = sm.periodic(1 << log_rows)
    assert np.array_equal(pre, want) and np.array_equal(ext, oracle.lde(want.reshape(1, -1), log_blowup).reshape(-1))


@pytest.mark.gpu
def test_sch_extends_under_the_current_domain(ctx, oracle):
    """after tmx_ntt_set_domain (g = 7) SCH is extended under that domain: the CPU oracle's LDE under it, which differs from the default
    domain's; the column before the LDE does not depend on the domain"""
    log_rows, lb = 8, 2
    want = sm.periodic(1 << log_rows).reshape(1, -1)
    default = oracle.lde(want, lb).reshape(-1)
    try:
        ctx.ntt_set_domain(*oracle.G7_DOMAIN)
        oracle.ntt_set_domain(*oracle.G7_DOMAIN)
        pre, ext = _periodic(ctx, log_rows, lb)
        moved = oracle.lde(want, lb).reshape(-1)
    finally:
        ctx.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
        oracle.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
    assert np.array_equal(pre, want[0]) and np.array_equal(ext, moved) and not np.array_equal(moved, default)
    assert np.array_equal(_periodic(ctx, log_rows, lb)[1], default)


def _bary(ctx, log_rows, zeta_words):
    """the three words of tmx_air_sha512_sched_periodic_eval_device at the two words of zeta as given; the words behind them stay untouched"""
    import torch
    d_zeta, d_out = _up(np.array(zeta_words, dtype=np.uint64)), _sentinel(3 + GUARD)
    ctx.air_sha512_sched_periodic_eval_device(log_rows, d_zeta.data_ptr(), d_out.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(d_out[3:], _sentinel(GUARD))
    return [int(x) for x in _down(d_out[:3])]


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows", [7, 8, 9, 10, 15, 18])
def test_sch_at_zeta_equals_the_model(ctx, oracle, log_rows):
    """SCH at a random zeta of F_p^2 over N = 128 (half a workgroup), 256, 512, 1024 (one), 2^15 (32 workgroups, the full size) and 2^18
    (64 workgroups, four batches per thread): the kernel's value equals the model's barycentric sum, no zero denominator"""
    rng = np.random.default_rng(10500 + log_rows)
    zeta = tuple(int(x) for x in rng.integers(1, P, 2, dtype=np.uint64))
    assert _bary(ctx, log_rows, zeta) == list(sm.sch_at(oracle, log_rows, zeta)) + [0]


@pytest.mark.gpu
def test_sch_at_zeta_flags_and_non_canonical_words(ctx, oracle):
    """N = 4096: four workgroups of 256 threads, row r in workgroup (r mod 1024) / 256.  zeta = omega^5 (the first workgroup) and
    omega^4095 (the last) raise the flag; (omega^5, 1) is no root: no flag; the words (z0 + p, z1 + p) give the three words of (z0, z1),
    at an honest point and at a root; a small evaluation behind a flagged one folds no stale flag"""
    om = oracle.gl_root(12)
    assert _bary(ctx, 12, (pow(om, 5, P), 0))[2] == 1 and _bary(ctx, 12, (pow(om, 4095, P), 0))[2] == 1
    near = (pow(om, 5, P), 1)
    assert _bary(ctx, 12, near) == list(sm.sch_at(oracle, 12, near)) + [0]
    z = (0x12345678, 0x7ABCDEF1)
    want = list(sm.sch_at(oracle, 12, z)) + [0]
    assert _bary(ctx, 12, z) == want and _bary(ctx, 12, (z[0] + P, z[1] + P)) == want
    assert _bary(ctx, 12, (1 + P, P))[2] == 1  # (omega^0 = 1, 0) in non-canonical words
    assert _bary(ctx, 9, z) == list(sm.sch_at(oracle, 9, z)) + [0]


def _device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, cap_height=CAP_H, **kw):
    return _guarded(2 << log_n, lambda out: ctx.air_sha512_sched_quotient_device(log_n, log_blowup, cap_height, n_proofs, d_cols.data_ptr(),
                                                                                d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(), out, 0, **kw))


def _quotient_equals_the_model(ctx, oracle, log_n, log_blowup, n_proofs, ext, hext):
    """uploads, caps, the whole quotient and gamma against the model; returns (device columns, device helper columns, the two caps, the
    model's quotient)"""
    d_cols, d_hcols = _up(ext), _up(hext)
    _, d_cap = _tree(ctx, d_cols, log_n, n_proofs * W)
    _, d_cap_h = _tree(ctx, d_hcols, log_n, n_proofs * HC)
    got = _down(_device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h))
    g = sm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _down(d_cap), _down(d_cap_h))
    assert ctx.air_last_gamma() == g
    pext = oracle.lde(sm.periodic(1 << (log_n - log_blowup)).reshape(1, -1), log_blowup)
    want = sm.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, pext, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    return d_cols, d_hcols, d_cap, d_cap_h, want


@pytest.mark.gpu
@pytest.mark.parametrize("N,log_blowup,n_proofs", [(128, 1, 1), (128, 6, 2), (512, 3, 3), (1024, 1, 3)])
def test_quotient_of_random_columns_equals_the_model(ctx, oracle, N, log_blowup, n_proofs):
    """random table and helper columns (a few words non-canonical): the definition is pointwise, so gamma and d_quot equal the model word
    for word -- whole, and through the range call in two pieces in both orders (a written first piece and an accumulated second: [0, 1)
    then the rest, and the rest then [0, 1)); guard words intact"""
    import torch
    log_n = N.bit_length() - 1 + log_blowup
    rng = np.random.default_rng(10200 + 100 * log_n + 10 * log_blowup + n_proofs)
    ext, hext = _random_ext(rng, n_proofs * W, log_n), _random_ext(rng, n_proofs * HC, log_n)
    d_cols, d_hcols, d_cap, d_cap_h, want = _quotient_equals_the_model(ctx, oracle, log_n, log_blowup, n_proofs, ext, hext)
    pieces, words = ([(0, 1), (1, n_proofs)] if n_proofs > 1 else [(0, 1)]), 2 << log_n
    for order in (pieces, pieces[::-1]):
        buf = _sentinel(words + 2 * GUARD)
        for k, (lo, hi) in enumerate(order):
            d_piece = d_hcols[(lo * HC) << log_n:]
            ctx.air_sha512_sched_quotient_device(log_n, log_blowup, CAP_H, n_proofs, d_cols.data_ptr(), d_piece.data_ptr(), d_cap.data_ptr(),
                                                 d_cap_h.data_ptr(), buf[GUARD:].data_ptr(), 0, proof_range=(lo, hi), accumulate=int(k > 0))
        torch.cuda.synchronize(_dev())
        assert np.array_equal(_down(buf[GUARD:GUARD + words]), want), order
        assert torch.equal(buf[:GUARD], _sentinel(GUARD)) and torch.equal(buf[GUARD + words:], _sentinel(GUARD)), order


@pytest.mark.gpu
@pytest.mark.parametrize("fill", ["all p - 1", "all 2^64 - 1"])
def test_quotient_of_extreme_words_equals_the_model(ctx, oracle, fill):
    """the inputs the NTT's lazy arithmetic is tested with, as table and helper columns of set 8's sums (32-step dbl_add, scale(carry,
    2^32), 234 accumulated terms): every word p - 1 and every word 2^64 - 1, at N = 128, blow-up 8, two proofs"""
    log_n, lb, n_proofs = 10, 3, 2
    rng = np.random.default_rng(10800)
    ext, hext = FILLS[fill](rng, (n_proofs * W, 1 << log_n)), FILLS[fill](rng, (n_proofs * HC, 1 << log_n))
    assert ext.dtype == np.uint64 and int(ext.min()) >= P - 1
    _quotient_equals_the_model(ctx, oracle, log_n, lb, n_proofs, ext, hext)


# ---- GPU: the chain and the verifiers
def _chain(ctx, oracle, table, log_blowup, with7=True, q8_override=None, n_queries=6, others=()):
    """caller-level chain: both helpers -> LDE -> caps -> both quotients -> one batch proof over [table, H7, Q7, H8, Q8] (with7 = False:
    [table, H8, Q8]).  others: (position, extended columns [n][2^log_n]) of further oracles.  Returns a dict: the params p, the caps on the
    device, the proof words, k7 / k8 (set 7's and set 8's helper index; the table's is kt), the two gammas, and set 8's extended helper and
    quotient words"""
    import torch
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    log_n = log_rows + log_blowup

    def lde(d_pre, n):
        d_out = _sentinel(n << log_n)
        ctx.lde_device(log_rows, log_blowup, n, d_pre.data_ptr(), d_out.data_ptr(), 0)
        return d_out
    d_ext = lde(_up(table), n_proofs * W)
    d_lv_t, d_cap_t = _tree(ctx, d_ext, log_n, n_proofs * W)
    members, out = [(d_ext, d_lv_t, d_cap_t, n_proofs * W)], {}
    if with7:
        d_h7 = lde(t7._device_helper(ctx, table), n_proofs * HC7)
        d_lv, d_cap_h7 = _tree(ctx, d_h7, log_n, n_proofs * HC7)
        d_q7 = t7._device_quotient(ctx, log_n, log_blowup, n_proofs, d_ext, d_h7, d_cap_t, d_cap_h7)
        out["gamma7"] = ctx.air_last_gamma()
        d_lv_q, d_cap_q7 = _tree(ctx, d_q7, log_n, 2)
        members += [(d_h7, d_lv, d_cap_h7, n_proofs * HC7), (d_q7, d_lv_q, d_cap_q7, 2)]
    d_h8 = lde(_device_helper(ctx, table), n_proofs * HC)
    d_lv, d_cap_h8 = _tree(ctx, d_h8, log_n, n_proofs * HC)
    if q8_override is None:
        d_q8 = _device_quotient(ctx, log_n, log_blowup, n_proofs, d_ext, d_h8, d_cap_t, d_cap_h8)
        out["gamma8"] = ctx.air_last_gamma()
    else:
        d_q8 = _up(q8_override)
    d_lv_q, d_cap_q8 = _tree(ctx, d_q8, log_n, 2)
    members += [(d_h8, d_lv, d_cap_h8, n_proofs * HC), (d_q8, d_lv_q, d_cap_q8, 2)]
    log_ns = [log_n] * len(members)
    for at, e in others:
        d_o, lo = _up(e), e.shape[1].bit_length() - 1
        d_lv_o, d_cap_o = _tree(ctx, d_o, lo, e.shape[0])
        members.insert(at, (d_o, d_lv_o, d_cap_o, e.shape[0]))
        log_ns.insert(at, lo)
    kt = next(k for k, m in enumerate(members) if m[0] is d_ext)
    p = bparams(log_ns, [m[3] for m in members], CAP_H, log_blowup, 2, 2, n_queries)
    proof = _guarded(bm.layout(p)["words"], lambda o: ctx.batch_prove_device(p, [m[0].data_ptr() for m in members], [m[1].data_ptr() for m in members], o, 0))
    out.update(p=p, d_caps=torch.cat([m[2] for m in members]), proof=_down(proof), kt=kt, k7=kt + 1 if with7 else None, k8=kt + (3 if with7 else 1),
               ext=_down(d_ext).reshape(n_proofs * W, -1), hext=_down(d_h8).reshape(n_proofs * HC, -1), quot=_down(d_q8))
    return out


def _verdicts(ctx, p, k_trace, k_helper, d_caps, proof, which=8):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    if which == 8:
        ctx.air_sha512_sched_verify_device(p, k_trace, k_helper, d_caps.data_ptr(), _up(proof).data_ptr(), ok.data_ptr(), 0)
    elif which == 7:
        ctx.air_sha512_verify_device(p, k_trace, d_caps.data_ptr(), _up(proof).data_ptr(), ok.data_ptr(), 0)
    else:
        ctx.batch_verify_device(p, d_caps.data_ptr(), _up(proof).data_ptr(), ok.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    out = ok.cpu().numpy()
    assert ((out == 0) | (out == 1)).all(), out
    return [bool(x) for x in out]


def _bumped(proof, at):
    bad = proof.copy()
    bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
    return bad


@pytest.mark.gpu
def test_real_rows_through_the_caller_level_chain(ctx, oracle, step2):
    """five oracles [table, H7, Q7, H8, Q8] of T.2 of step N = 2 (two proofs, N = 512, blow-up 2) in one batch proof: set 8's helper,
    gamma and quotient equal the model's and the quotient has degree <= N - 2; both device verifiers accept every query, as both models
    do; set 8's verifier rejects a proof with one bumped table, helper or quotient opening on every query, as the model's identity fails"""
    table, lb = step2, 1
    n_proofs = table.shape[0] // W
    c = _chain(ctx, oracle, table, lb)
    assert ctx.fri_last_degree_ok() is True
    p, d_caps, got = c["p"], c["d_caps"], c["proof"]
    assert p["n_cols"] == [n_proofs * W, n_proofs * HC7, 2, n_proofs * HC, 2] and (c["kt"], c["k7"], c["k8"]) == (0, 1, 3)
    log_n, caps, cw = p["log_n"][0], _down(d_caps), 4 << CAP_H
    assert np.array_equal(c["hext"], oracle.lde(sm.helper(table, n_proofs), lb))
    g = sm.gamma(oracle, log_n, lb, CAP_H, n_proofs, caps[:cw], caps[3 * cw:4 * cw])
    assert c["gamma8"] == g and c["gamma7"] == s7.gamma(oracle, log_n, lb, CAP_H, n_proofs, caps[:cw], caps[cw:2 * cw])
    pext = oracle.lde(sm.periodic(table.shape[1]).reshape(1, -1), lb)
    assert np.array_equal(c["quot"], sm.quotient(oracle, log_n, lb, n_proofs, c["ext"], c["hext"], pext, _shift(), g))
    assert max(_degrees(oracle, c["quot"])) <= table.shape[1] - 2
    model8 = sm.verify(oracle, p, 0, 3, caps, got, _shift())
    assert all(model8) and s7.identity(oracle, p, 0, caps, got)
    assert _verdicts(ctx, p, 0, 3, d_caps, got) == model8 and _verdicts(ctx, p, 0, None, d_caps, got, which=7) == model8
    assert all(_verdicts(ctx, p, 0, None, d_caps, got, which=0))
    L = bm.layout(p)
    RH = 1 << dm.log_r(p["n_cols"][3])
    for name, at in (("quotient opening", L["off_open"][4] + 1), ("helper opening at zeta", L["off_open"][3] + sm.HX1 + 41),
                     ("helper opening at zeta omega", L["off_open"][3] + 2 * RH + HC + sm.HQH + 9),
                     ("table opening at zeta", L["off_open"][0] + W + sm.W_ + 1)):
        bad = _bumped(got, at)
        assert not sm.identity(oracle, p, 0, 3, caps, bad), name
        assert _verdicts(ctx, p, 0, 3, d_caps, bad) == [False] * p["n_queries"], name


@pytest.mark.gpu
def test_the_rerun_block_passes_set_7_and_fails_set_8_on_the_device(ctx, oracle, step2):
    """the table re-run from a changed W_20 with the honest helpers of the changed table, set 7's own quotient and a zero (low-degree)
    quotient for set 8: the batch proof is fine and SET 7'S DEVICE VERIFIER ACCEPTS every query, SET 8'S REJECTS every one, as the two
    models do"""
    t, _, _ = _tampered(step2[:W], RERUN)
    log_n = 9 + 1
    c = _chain(ctx, oracle, t, 1, q8_override=np.zeros(2 << log_n, dtype=np.uint64))
    p, d_caps, got, caps = c["p"], c["d_caps"], c["proof"], _down(c["d_caps"])
    assert all(_verdicts(ctx, p, 0, None, d_caps, got, which=0))
    assert s7.identity(oracle, p, 0, caps, got) and not sm.identity(oracle, p, 0, 3, caps, got)
    assert _verdicts(ctx, p, 0, None, d_caps, got, which=7) == [True] * p["n_queries"]
    assert _verdicts(ctx, p, 0, 3, d_caps, got) == [False] * p["n_queries"]


@pytest.mark.gpu
def test_257_proofs_through_the_check_kernel(ctx, oracle, step2):
    """N = 128, 257 proofs (one more than k_air_sha512_check<Sha512Sched> has threads: thread 0 takes proofs 0 and 256) -- the live first blocks
    of T.2 of step N = 2 in turn, 48 rows of padding behind each, every seventh proof zero --, blow-up 2, two queries, [table, H8, Q8]:
    the device accepts every query as the model's identity does; a helper opening bumped in proof 256 and a table opening in proof 255
    are rejected"""
    many = 257
    blocks = [step2[q * W:(q + 1) * W, 80 * b:80 * b + 80] for q in range(step2.shape[0] // W) for b in range(0, step2.shape[1] // 80, 2)
              if step2[q * W:(q + 1) * W, 80 * b].any()]
    assert blocks
    table = np.zeros((many * W, 128), dtype=np.uint64)
    for q in range(many):
        if q % 7 != 6:
            table[q * W:(q + 1) * W, :80] = blocks[q % len(blocks)]
    c = _chain(ctx, oracle, table, 1, with7=False, n_queries=2)
    assert ctx.fri_last_degree_ok() is True
    p, d_caps, got, caps = c["p"], c["d_caps"], c["proof"], _down(c["d_caps"])
    assert sm.identity(oracle, p, 0, 1, caps, got)
    assert _verdicts(ctx, p, 0, 1, d_caps, got) == [True, True]
    L = bm.layout(p)
    for at in (L["off_open"][1] + 256 * HC + sm.HG1 + 1, L["off_open"][0] + 255 * W + sm.W_):
        bad = _bumped(got, at)
        assert not sm.identity(oracle, p, 0, 1, caps, bad)
        assert _verdicts(ctx, p, 0, 1, d_caps, bad) == [False, False]


# ---- GPU: the set level
def _set_round(c, kind, n_proofs, lb, tr, calls, sections=SHA512 | HEADER, queries=6):
    """commit `sections`, the air calls of `calls` ("7": set 7's, "8": set 8's, on SHA512) in that order, one proof.  Returns (params, the
    sections in oracle order, the caps in that order on the device, proof words, {set: gamma})"""
    import torch
    cw = 4 << CAP_H
    d_caps = _sentinel(bin(sections).count("1") * cw)
    own = {s: _sentinel(cw) for s in (H7, Q7, HELPER, QUOTIENT)}
    c.trace_commit_set_device(kind, n_proofs, sections, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
    _, order0 = c.trace_commit_set_shape()
    gammas = {}
    for s in calls:
        if s == "7":
            c.trace_commit_set_air_sha512_device(SHA512, own[H7].data_ptr(), own[Q7].data_ptr(), 0)
        else:
            c.trace_commit_set_air_sha512_sched_device(SHA512, own[HELPER].data_ptr(), own[QUOTIENT].data_ptr(), 0)
        gammas[s] = c.air_last_gamma()
    shape, order = c.trace_commit_set_shape()
    p = dict(shape, arity_bits=2, final_log_max=2, n_queries=queries, pow_bits=0)
    proof = _down(_guarded(bm.layout(p)["words"], lambda out: c.trace_commit_set_prove_device(p, out, 0)))
    assert c.fri_last_degree_ok() is True
    caps_of = {s: d_caps[cw * i:cw * (i + 1)] for i, s in enumerate(order0)}
    caps_of.update(own)
    return p, order, torch.cat([caps_of[s] for s in order]), proof, gammas


@pytest.mark.gpu
def test_set_level_in_both_call_orders(ctx, oracle, device_rows):
    """a set SHA512 | HEADER of two step N = 2 proofs: set 7's call then set 8's, and on a second set set 8's then set 7's.  Both shapes end
    [HEADER, SHA512, 32768, 65536, 131072, 262144]; caps, both gammas and proof words are equal between the two orders and equal to the
    caller-level chain's over the same columns (the header table as one more oracle); both device verifiers accept, as both models'
    identities hold; set 7's caps with set 8 present equal those of a set without it"""
    import torch
    from test_merkle_open import _oracle_ext
    c, (tr, table) = ctx, device_rows
    kind, n, n_proofs, lb = 1, 2, 2, 1
    cw = 4 << CAP_H
    a = _set_round(c, kind, n_proofs, lb, tr, "78")
    b = _set_round(c, kind, n_proofs, lb, tr, "87")
    p, order, d_caps, proof, gammas = a
    assert order == [HEADER, SHA512, H7, Q7, HELPER, QUOTIENT] and b[1] == order and b[0] == p
    assert p["log_n"][1:] == [9 + lb] * 5 and p["n_cols"][1:] == [W * n_proofs, HC7 * n_proofs, 2, HC * n_proofs, 2]
    assert torch.equal(b[2], d_caps) and np.array_equal(b[3], proof) and b[4] == gammas
    e, lm, nc = _oracle_ext(oracle, kind, n, _down(tr), HEADER, lb)
    ch = _chain(c, oracle, table, lb, others=[(0, e.reshape(nc, -1))])
    assert {key: ch["p"][key] for key in ("log_n", "n_cols")} == {key: p[key] for key in ("log_n", "n_cols")} and (ch["kt"], ch["k8"]) == (1, 4)
    assert gammas == {"7": ch["gamma7"], "8": ch["gamma8"]} and torch.equal(d_caps, ch["d_caps"])
    assert np.array_equal(proof, ch["proof"])
    caps = _down(d_caps)
    assert _verdicts(c, p, 1, 4, d_caps, proof) == [True] * 6 and _verdicts(c, p, 1, None, d_caps, proof, which=7) == [True] * 6
    assert sm.identity(oracle, p, 1, 4, caps, proof) and s7.identity(oracle, p, 1, caps, proof)
    assert not any(_verdicts(c, p, 1, 4, d_caps, _bumped(proof, bm.layout(p)["off_open"][5])))
    only7 = _set_round(c, kind, n_proofs, lb, tr, "7")
    assert only7[1] == order[:4] and torch.equal(only7[2], d_caps[:4 * cw]) and only7[4]["7"] == gammas["7"]
    only8 = _set_round(c, kind, n_proofs, lb, tr, "8")
    assert only8[1] == order[:2] + order[4:] and torch.equal(only8[2][2 * cw:], d_caps[4 * cw:]) and only8[4]["8"] == gammas["8"]
    assert _verdicts(c, only8[0], 1, 2, only8[2], only8[3]) == [True] * 6


@pytest.mark.gpu
def test_set_level_refusals(ctx, device_rows):
    """the set-level call takes TMX_TRACE_SHA512 alone, a resident member only, refuses a second call on the section and null caps, each
    with nothing enqueued and the set as it was; set 7's call behind set 8's is still fine; the streamed call refuses constraint_set = 8"""
    c, (tr, _) = ctx, device_rows
    kind, n_proofs, lb = 1, 2, 1
    cw = 4 << CAP_H
    d_caps, d_cap_h, d_cap_q = _sentinel(2 * cw), _sentinel(cw), _sentinel(cw)
    air = lambda sec: (lambda: c.trace_commit_set_air_sha512_sched_device(sec, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0))
    commit = lambda secs=SHA512 | HEADER: c.trace_commit_set_device(kind, n_proofs, secs, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
    commit()
    before = c.trace_commit_set_shape()
    for sec in (HEADER, SHA256, 1, H7, HELPER):
        assert "TMX_TRACE_SHA512" in _refused(air(sec), d_cap_h, d_cap_q)
    _refused(lambda: c.trace_commit_set_air_sha512_sched_device(SHA512, None, d_cap_q.data_ptr(), 0), d_cap_q)
    _refused(lambda: c.trace_commit_set_air_sha512_sched_device(SHA512, d_cap_h.data_ptr(), None, 0), d_cap_h)
    _refused(lambda: c.trace_commit_set_air_sha256_streamed_device(8, SHA512, 8, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0), d_cap_h, d_cap_q)
    assert c.trace_commit_set_shape() == before
    air(SHA512)()
    after = c.trace_commit_set_shape()
    assert after[1] == [HEADER, SHA512, HELPER, QUOTIENT]
    assert "already" in _refused(air(SHA512), d_cap_h, d_cap_q)
    assert c.trace_commit_set_shape() == after
    commit(HEADER)
    assert "does not hold" in _refused(air(SHA512), d_cap_h, d_cap_q)
    c.trace_commit_set_streamed_device(kind, n_proofs, SHA512 | HEADER, SHA512, 8, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
    assert "streamed" in _refused(air(SHA512), d_cap_h, d_cap_q)


@pytest.mark.gpu
def test_a_full_set_is_refused(built_lib):
    """all five tables, the ladders' quotient and one SHA-256 pair make eight oracles: set 8's pair has no room, and the set stays as it was"""
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    cw = 4 << CAP_H
    with tmx.Context(4, b"celestia", max_batch=1) as c:
        tr = _trace_rows(c, 0, 4, 1, 10400)
        d_caps, d_cap_h, d_cap_q = _sentinel(5 * cw), _sentinel(cw), _sentinel(cw)
        c.trace_commit_set_device(0, 1, 1 | SHA512 | SHA256 | 16 | HEADER, 1, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        c.trace_commit_set_air_device(d_cap_q.data_ptr(), 0)
        c.trace_commit_set_air_sha256_device(16, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
        before = c.trace_commit_set_shape()
        assert len(before[1]) == 8
        assert "room" in _refused(lambda: c.trace_commit_set_air_sha512_sched_device(SHA512, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0), d_cap_h,
                                  d_cap_q)
        assert c.trace_commit_set_shape() == before


@pytest.mark.gpu
def test_each_validation_rule(ctx):
    """every rule on its own: TMX_ERR_BAD_ARG before anything is enqueued, nothing written.  FRI's rules on log_n and log_blowup;
    7 <= log_n - log_blowup <= 18; n_proofs >= 1; 230 n_proofs <= 2^24; a range inside n_proofs; accumulate <= 1; no null pointer; the
    verifier: k_helper > k_trace, column counts 18 k / 230 k / 2, equal log_n, both oracles inside the proof"""
    import torch
    log_n, lb = 9, 1
    d_cols, d_hcols = _sentinel(W << log_n), _sentinel(HC << log_n)
    d_cap, d_cap_h, d_quot = _sentinel(4 << CAP_H), _sentinel(4 << CAP_H), _sentinel(2 << log_n)
    ptrs = [d_cols.data_ptr(), d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(), d_quot.data_ptr()]
    q = lambda ln, b, n, a=ptrs, **kw: (lambda: ctx.air_sha512_sched_quotient_device(ln, b, CAP_H, n, *a, 0, **kw))
    for fn in (q(log_n, 0, 1), q(log_n, 7, 1), q(2, 2, 1), q(29, 2, 1), q(7, 1, 1), q(20, 1, 1), q(log_n, lb, 0), q(log_n, lb, (1 << 24) // HC + 1),
               q(log_n, lb, 2, proof_range=(1, 1)), q(log_n, lb, 2, proof_range=(1, 3)), q(log_n, lb, 2, proof_range=(0, 1), accumulate=2)):
        _refused(fn, d_quot)
    for k in range(5):
        _refused(q(log_n, lb, 1, ptrs[:k] + [None] + ptrs[k + 1:]), d_quot)
    d_table, d_help = _sentinel(W << 7), _sentinel(HC << 7)
    hp = lambda lr, n, t=d_table.data_ptr(), o=d_help.data_ptr(): (lambda: ctx.air_sha512_sched_helper_device(lr, n, t, o, 0))
    for fn in (hp(6, 1), hp(19, 1), hp(7, 0), hp(7, (1 << 24) // HC + 1), hp(7, 1, t=None), hp(7, 1, o=None)):
        _refused(fn, d_help)
    d_pre, d_out = _sentinel(1 << 8), _sentinel(8)
    for fn in (lambda: ctx.air_sha512_sched_periodic_device(6, 1, d_pre.data_ptr(), d_pre.data_ptr(), 0),
               lambda: ctx.air_sha512_sched_periodic_device(19, 1, d_pre.data_ptr(), d_pre.data_ptr(), 0),
               lambda: ctx.air_sha512_sched_periodic_device(7, 1, None, d_pre.data_ptr(), 0),
               lambda: ctx.air_sha512_sched_periodic_device(7, 1, d_pre.data_ptr(), None, 0),
               lambda: ctx.air_sha512_sched_periodic_eval_device(6, d_pre.data_ptr(), d_out.data_ptr(), 0),
               lambda: ctx.air_sha512_sched_periodic_eval_device(19, d_pre.data_ptr(), d_out.data_ptr(), 0),
               lambda: ctx.air_sha512_sched_periodic_eval_device(7, None, d_out.data_ptr(), 0),
               lambda: ctx.air_sha512_sched_periodic_eval_device(7, d_pre.data_ptr(), None, 0)):
        _refused(fn, d_pre, d_out)
    # the verifier
    ok, caps, proof = torch.full((4,), 7, dtype=torch.int32, device=_dev()), _sentinel(256), _sentinel(1 << 17)
    v = lambda p, kt, kh: (lambda: ctx.air_sha512_sched_verify_device(p, kt, kh, caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0))
    good = bparams([9, 9, 9], [W, HC, 2], CAP_H, lb, 2, 2, 4)
    for p, kt, kh in ((good, 1, 1), (good, 1, 0), (good, 0, 0), (good, 0, 2), (dict(good, n_cols=[W + 1, HC, 2]), 0, 1),
                      (dict(good, n_cols=[9, HC, 2]), 0, 1), (dict(good, n_cols=[W, HC + 1, 2]), 0, 1), (dict(good, n_cols=[2 * W, HC, 2]), 0, 1),
                      (dict(good, n_cols=[W, HC, 3]), 0, 1), (dict(good, log_n=[9, 9, 8]), 0, 1), (dict(good, log_n=[9, 8, 9]), 0, 1),
                      (bparams([7, 7, 7], [W, HC, 2], CAP_H, lb, 2, 2, 4), 0, 1), (dict(good, arity_bits=0), 0, 1),
                      (bparams([9, 9], [W, HC], CAP_H, lb, 2, 2, 4), 0, 1)):
        _refused(v(p, kt, kh), ok)


# ---- GPU: the scratch
@pytest.mark.gpu
def test_growth_and_reuse_of_the_scratch_and_interleaving_with_set_7(oracle):
    """one fresh context (its set-8 scratch starts unallocated): a caller-level set-8 quotient at (N, blow-up) = (128, 2) allocates it, one at
    (2048, 4) grows it (the scratch is synchronised, freed and allocated anew), a small one after the large one runs in the larger scratch;
    then set-7 and set-8 quotient calls interleaved on one stream without a synchronisation between them: each set's words are those of
    its call alone, all of them the model's"""
    import torch
    import tendermintx_amd as tmx
    import test_sha512_air_shapes as t7s
    rng = np.random.default_rng(10940)
    with tmx.Context(2, b"celestia", max_batch=2) as c:
        small = (8, 1, 1, _random_ext(rng, W, 8), _random_ext(rng, HC, 8))
        _quotient_equals_the_model(c, oracle, *small)
        _quotient_equals_the_model(c, oracle, 13, 2, 1, _random_ext(rng, W, 13), _random_ext(rng, HC, 13))
        d_cols, d_h8, d_cap, d_cap_h8, want8 = _quotient_equals_the_model(c, oracle, *small)
        h7 = _random_ext(rng, HC7, 8)
        _, d_h7, _, d_cap_h7, want7 = t7s._quotient_equals_the_model(c, oracle, 8, 1, 1, CAP_H, small[3], h7)
        words = 2 << 8
        bufs = [_sentinel(words + 2 * GUARD) for _ in range(4)]
        for k, buf in enumerate(bufs):
            call, d_h, d_ch = ((c.air_sha512_quotient_device, d_h7, d_cap_h7), (c.air_sha512_sched_quotient_device, d_h8, d_cap_h8))[k % 2]
            call(8, 1, CAP_H, 1, d_cols.data_ptr(), d_h.data_ptr(), d_cap.data_ptr(), d_ch.data_ptr(), buf[GUARD:].data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        for k, buf in enumerate(bufs):
            assert np.array_equal(_down(buf[GUARD:GUARD + words]), (want7, want8)[k % 2]), k
            assert torch.equal(buf[:GUARD], _sentinel(GUARD)) and torch.equal(buf[GUARD + words:], _sentinel(GUARD)), k
