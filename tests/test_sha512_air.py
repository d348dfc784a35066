"""The round constraints of the SHA-512 table (include/tmx.h "the round constraints of the SHA-512 table", constraint set 7):
tmx_air_sha512_helper_device, tmx_air_sha512_quotient_device and its range form, tmx_air_sha512_verify_device,
tmx_trace_commit_set_air_sha512_device, and the two calls that show the preprocessed columns on their own.  The yardstick is
tests/sha512_air_model.py on top of tests/batch_model.py: device words must equal the model's word for word and every verdict of the device
verifier must equal the model verifier's.  The CPU part ties the model itself to the claim: on the CPU oracle's T.2 rows all 628 constraints
hold as integer identities and the rows are a real SHA-512 compression of their first sixteen W words, the quotient is a polynomial of degree
<= N - 2, and one change of a detected kind makes it one of degree >= N; the kind the set does NOT see is recorded next to them."""
import hashlib

import numpy as np
import pytest

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha512_air_model as sm
from batch_model import bparams
from test_fri import _down, _sentinel, _shift, _up
from test_merkle_open import _section_geom
from test_sha_air import _cap, _degrees, _dev, _guarded, _random_ext, _refused, _tree

P = fm.P
SHA512, SHA256, HEADER, HELPER, QUOTIENT = 2, 4, 32, 32768, 65536
W, HC = sm.WIDTH, sm.HELPER_COLS
CAP_H = 2
LB = 2  # blow-up 4 in the CPU tests
IV512 = [0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1, 0x510e527fade682d1, 0x9b05688c2b3e6c1f,
         0x1f83d9abfb41bd6b, 0x5be0cd19137e2179]


def _columns(fulls, kind, n):
    """[18 n_proofs][2^log_rows] pre-LDE columns of T.2 from trace blocks (zero padded to a power of two, as the commit pipeline pads them)"""
    off, rows, width = _section_geom(kind, n, SHA512)
    assert width == W and rows == 160 * n
    cols = np.zeros((len(fulls) * W, 1 << (rows - 1).bit_length()), dtype=np.uint64)
    for p, full in enumerate(fulls):
        cols[p * W:(p + 1) * W, :rows] = np.asarray(full[off:off + rows * W], dtype=np.uint64).reshape(rows, W).T
    return cols


def _t2(oracle, kind, n, n_proofs, seed):
    from tendermintx_amd.synth import Workload
    wl = Workload(kind, n, n_proofs, n, chain_id=b"celestia", seed=seed, signed_permille=900)
    fulls = []
    for p in range(n_proofs):
        t = wl.targets[p * n * 256:(p + 1) * n * 256]
        r = wl.trusteds[p * n * 48:(p + 1) * n * 48] if kind == 0 else None
        fulls.append(oracle.trace(kind, wl.proofs[p * 2336:(p + 1) * 2336], t, r, n))
    return _columns(fulls, kind, n)


@pytest.fixture(scope="module")
def skip4(oracle):
    return _t2(oracle, 0, 4, 2, 8100)


@pytest.fixture(scope="module")
def step2(oracle):
    return _t2(oracle, 1, 2, 2, 8200)


@pytest.fixture(scope="module")
def step3(oracle):
    return _t2(oracle, 1, 3, 2, 8300)


def _word(t, c, r):
    return int(t[c, r]) | int(t[c + 1, r]) << 32


def test_rows_satisfy_the_constraints_as_integers(skip4, step2, step3):
    """all 628 constraints hold as integer identities (no reduction mod p) on every row of T.2 of skip N = 4, step N = 2 and step N = 3, with
    every table and helper value below 2^32; live and all-zero blocks both occur and LIVE is "row 0 of the block is not all zero"; the
    largest carries are printed and stay within the bounds the summand counts give (a: 6, e: 5).  Every live FIRST block is fed through a
    plain-integer SHA-512 compression: W_16 .. W_79 recomputed from W_0 .. W_15, the state chain from the IV, every row compared."""
    live_blocks = zero_blocks = 0
    cmax = [0, 0, 0, 0]
    s0 = lambda x: sm.rotr(x, 1) ^ sm.rotr(x, 8) ^ (x >> 7)
    s1 = lambda x: sm.rotr(x, 19) ^ sm.rotr(x, 61) ^ (x >> 6)
    for name, table in (("skip4", skip4), ("step2", step2), ("step3", step3)):
        assert int(table.max()) < 1 << 32
        n_proofs, N = table.shape[0] // W, table.shape[1]
        assert N % 80 and (N - 1) % 80 != 79
        help_ = sm.helper(table, n_proofs)
        assert help_.shape == (n_proofs * HC, N) and int(help_.max()) < 1 << 32
        for p in range(n_proofs):
            t, h = table[p * W:(p + 1) * W], help_[p * HC:(p + 1) * HC]
            for j, c in enumerate(sm.integer_residuals(t, h)):
                assert not c.any(), (name, p, j, np.flatnonzero(c)[:4])
            for b in range(N // 80):
                r0 = 80 * b
                nonzero = bool(t[:, r0].any())
                assert (h[sm.HLIVE, r0:r0 + 80] == int(nonzero)).all()
                assert nonzero == bool(t[:, r0:r0 + 80].any())
                live_blocks, zero_blocks = live_blocks + nonzero, zero_blocks + (not nonzero)
                if nonzero and b % 2 == 0:
                    w = [_word(t, sm.W_, r0 + k) for k in range(16)]
                    for k in range(16, 80):
                        w.append((s1(w[k - 2]) + w[k - 7] + s0(w[k - 15]) + w[k - 16]) & sm.M64)
                    state = list(IV512)
                    for k in range(80):
                        state = sm.sha_round(state, w[k], k)
                        assert _word(t, sm.W_, r0 + k) == w[k], (name, p, b, k)
                        assert [_word(t, c, r0 + k) for c in range(sm.A_, W, 2)] == state, (name, p, b, k)
            assert not h[sm.HLIVE, 80 * (N // 80):].any()
            for k, at in enumerate((sm.HCAL, sm.HCAH, sm.HCEL, sm.HCEH)):
                cmax[k] = max(cmax[k], int((h[at] + 2 * h[at + 1] + 4 * h[at + 2]).max()))
    print(f"\n[sha512-air] live blocks {live_blocks}, zero blocks {zero_blocks}, largest carries CAL {cmax[0]} CAH {cmax[1]} CEL {cmax[2]} CEH {cmax[3]}")
    assert live_blocks and zero_blocks and max(cmax[:2]) <= 6 and max(cmax[2:]) <= 5


def test_compression_model_against_hashlib():
    """the plain-integer round function the test above leans on is SHA-512: one padded block against hashlib"""
    msg = b"abc"
    block = msg + b"\x80" + bytes(128 - len(msg) - 1 - 16) + (8 * len(msg)).to_bytes(16, "big")
    w = [int.from_bytes(block[8 * k:8 * k + 8], "big") for k in range(16)]
    for k in range(16, 80):
        w.append(((sm.rotr(w[k - 2], 19) ^ sm.rotr(w[k - 2], 61) ^ (w[k - 2] >> 6)) + w[k - 7]
                  + (sm.rotr(w[k - 15], 1) ^ sm.rotr(w[k - 15], 8) ^ (w[k - 15] >> 7)) + w[k - 16]) & sm.M64)
    state = list(IV512)
    for k in range(80):
        state = sm.sha_round(state, w[k], k)
    digest = b"".join(((a + b) & sm.M64).to_bytes(8, "big") for a, b in zip(IV512, state))
    assert digest == hashlib.sha512(msg).digest()


def test_barycentric_values_equal_horner_on_the_coefficients(oracle):
    """the model's barycentric SEL, KLO, KHI at a zeta outside the base field against Horner on the interpolated coefficients (N = 128); the
    three polynomials have full degree N - 1, which is why no subgroup selector stands in for them"""
    zeta = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)
    cols = sm.periodic(128)
    coefs = [am.coefficients(oracle, c, 1) for c in cols]
    assert [am.degree(c) for c in coefs] == [127] * 3
    assert sm.barycentric(oracle, 7, zeta) == [am.horner(c, zeta) for c in coefs]


def _model_quotient(oracle, table, help_, log_blowup=LB, pre=None):
    """(extended table, extended helper, gamma, planar quotient) of pre-LDE columns"""
    n_proofs, log_n = table.shape[0] // W, table.shape[1].bit_length() - 1 + log_blowup
    ext, hext = oracle.lde(table, log_blowup), oracle.lde(help_, log_blowup)
    pext = oracle.lde(sm.periodic(table.shape[1]) if pre is None else pre, log_blowup)
    g = sm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _cap(oracle, ext, log_n), _cap(oracle, hext, log_n))
    return ext, hext, g, sm.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, pext, _shift(), g)


def test_quotient_is_a_polynomial_of_degree_at_most_n_minus_2(oracle, step2):
    """T.2 of step N = 2 (one proof, N = 512: live first blocks, zero second blocks, 192 rows of padding and a partial block at the end),
    blow-up 4: the model quotient interpolates to degree <= N - 2 in both planes, and the identity holds at a zeta outside the base field
    -- table, helper and quotient evaluated there by Horner on their coefficients, SEL, KLO, KHI barycentrically; it fails after bumping
    u_0, a table opening or a helper opening"""
    table = step2[:W]
    N = table.shape[1]
    assert N == 512
    log_n, n_proofs = 9 + LB, 1
    help_ = sm.helper(table, n_proofs)
    ext, hext, g, quot = _model_quotient(oracle, table, help_)
    deg = _degrees(oracle, quot)
    print(f"\n[sha512-air] T.2 of step N = 2: N = {N}, quotient degrees {deg}")
    assert max(deg) <= N - 2 and g[1] != 0
    M = 1 << log_n
    zeta = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)
    zs = (zeta, fm.e_scale(zeta, oracle.gl_root(log_n - LB)))
    yt, yh = dm.evaluate(oracle, table, 1, zs), dm.evaluate(oracle, help_, 1, zs)
    u = [am.horner(am.coefficients(oracle, quot[k * M:(k + 1) * M], _shift()), zeta) for k in (0, 1)]
    t0, t1, h0, h1 = [tuple(y[0]) for y in yt], [tuple(y[1]) for y in yt], [tuple(y[0]) for y in yh], [tuple(y[1]) for y in yh]
    pre = sm.barycentric(oracle, 9, zeta)
    ident = lambda t0=t0, t1=t1, h0=h0, h1=h1, u0=u[0]: sm.identity_at(oracle, log_n, LB, n_proofs, t0, t1, h0, h1, u0, u[1], zeta, g, pre)
    assert ident()
    assert not ident(u0=fm.e_add(u[0], (1, 0)))
    bump = lambda v, at: v[:at] + [fm.e_add(v[at], (0, 1))] + v[at + 1:]
    assert not ident(t0=bump(t0, sm.D_ + 1)) and not ident(t1=bump(t1, sm.W_))
    assert not ident(h0=bump(h0, sm.HV + 40)) and not ident(h1=bump(h1, sm.HKL + 1))


def _mid_row(table):
    """a row in the middle of a live block of proof 0's table, and that block's first row"""
    live = [b for b in range(table.shape[1] // 80) if table[:W, 80 * b].any()]
    b = live[len(live) // 2]
    return 80 * b + 37, 80 * b


def _rerun(table, r0, first, last):
    """rows first .. last of the block at r0 recomputed from row first - 1 with the round function, the W column as it stands"""
    t = table.copy()
    state = [_word(t, c, first - 1) for c in range(sm.A_, W, 2)]
    for r in range(first, last + 1):
        state = sm.sha_round(state, _word(t, sm.W_, r), r - r0)
        for k, x in enumerate(state):
            t[sm.A_ + 2 * k, r], t[sm.A_ + 2 * k + 1, r] = x & sm.M32, x >> 32
    return t


def _tampered(table, kind):
    """(table, helper, preprocessed columns) of ONE proof after a single change of `kind`"""
    t = table[:W].copy()
    r, r0 = _mid_row(t)
    pre = sm.periodic(t.shape[1])
    if kind == "a changed a_lo":
        t[sm.A_, r] ^= np.uint64(1 << 9)
        return t, sm.helper(t, 1), pre
    if kind == "a changed a_hi":
        t[sm.A_ + 1, r] ^= np.uint64(1 << 9)
        return t, sm.helper(t, 1), pre
    h = sm.helper(t, 1)
    if kind == "a flipped helper bit":
        h[sm.HE + 37, r] ^= np.uint64(1)
    elif kind == "a changed CAL bit":
        h[sm.HCAL, r] ^= np.uint64(1)
    elif kind == "a changed CAH bit":
        h[sm.HCAH + 1, r] ^= np.uint64(1)
    elif kind == "LIVE flipped on one row":
        h[sm.HLIVE, r] ^= np.uint64(1)
    elif kind == "SEL left 1 on row N - 1":
        pre[0, -1] = 1
    elif kind == "a block re-run from a changed W_t, t >= 16":
        t[sm.W_ + 1, r0 + 20] ^= np.uint64(1 << 3)
        t = _rerun(t, r0, r0 + 20, r0 + 79)
        h = sm.helper(t, 1)
    else:
        raise KeyError(kind)
    return t, h, pre


DETECTED = ["a changed a_lo", "a changed a_hi", "a flipped helper bit", "a changed CAL bit", "a changed CAH bit", "LIVE flipped on one row",
            "SEL left 1 on row N - 1"]
UNDETECTED = ["a block re-run from a changed W_t, t >= 16"]


@pytest.mark.parametrize("kind", DETECTED)
def test_one_change_breaks_the_degree(oracle, step2, kind):
    """the detected kinds, on T.2 of step N = 2 (one proof): the first two change the table mid-block and regenerate the helper from it, the
    next four change the helper alone, the last leaves SEL on at the wrap row -- row N - 1 is zero padding but row 0 is a live row, so
    the shift constraints fail there: the reason the wrap row is switched off.  The quotient no longer interpolates to degree < N"""
    table = step2[:W]
    t, h, pre = _tampered(table, kind)
    assert (t != table).sum() + (h != sm.helper(table, 1)).sum() + (pre != sm.periodic(table.shape[1])).sum() >= 1
    deg = _degrees(oracle, _model_quotient(oracle, t, h, pre=pre)[3])
    print(f"\n[sha512-air] {kind}: quotient degrees {deg}, N = {table.shape[1]}")
    assert max(deg) >= table.shape[1]


@pytest.mark.parametrize("kind", UNDETECTED)
def test_kinds_the_constraints_do_not_see(oracle, step2, kind):
    """recorded so that nobody mistakes the claim: the message schedule is not in the set -- a block re-run consistently with the round
    function from a changed W_t (t >= 16) keeps the quotient at degree <= N - 2"""
    table = step2[:W]
    t, h, pre = _tampered(table, kind)
    assert (t != table).sum() > 8
    assert max(_degrees(oracle, _model_quotient(oracle, t, h, pre=pre)[3])) <= table.shape[1] - 2


def test_symbols_and_wrappers_exist(built_lib):
    """the new entry points are in the built library, bound in _lib.py and wrapped in context.py"""
    from tendermintx_amd import _lib
    from tendermintx_amd.context import Context
    for name in ("tmx_air_sha512_helper_device", "tmx_air_sha512_quotient_device", "tmx_air_sha512_quotient_range_device",
                 "tmx_air_sha512_verify_device", "tmx_trace_commit_set_air_sha512_device", "tmx_air_sha512_periodic_device",
                 "tmx_air_sha512_periodic_eval_device"):
        assert getattr(built_lib, name).argtypes, name
    for name in ("air_sha512_helper_device", "air_sha512_quotient_device", "air_sha512_verify_device", "trace_commit_set_air_sha512_device",
                 "air_sha512_periodic_device", "air_sha512_periodic_eval_device"):
        assert callable(getattr(Context, name)), name
    assert (_lib.AIR_SHA512_HELPER_COLS, _lib.AIR_SHA512_CONSTRAINTS) == (HC, sm.CONSTRAINTS)
    assert (_lib.TRACE_SHA512_HELPER, _lib.TRACE_SHA512_QUOTIENT) == (HELPER, QUOTIENT)


# ---- GPU
@pytest.fixture(scope="module")
def ctx(built_lib):
    import tendermintx_amd as tmx
    c = tmx.Context(2, b"celestia", max_batch=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device_rows(ctx):
    """(trace rows on the device, T.2 columns from them) of two step N = 2 proofs"""
    from test_merkle_open import _trace_rows
    tr = _trace_rows(ctx, 1, 2, 2, 9300)
    return tr, _columns(list(_down(tr)), 1, 2)


def _device_helper(ctx, table):
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    d_table = _up(table)
    return _guarded((n_proofs * HC) << log_rows, lambda out: ctx.air_sha512_helper_device(log_rows, n_proofs, d_table.data_ptr(), out, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows", [7, 9, 10])
@pytest.mark.parametrize("n_proofs", [1, 3])
def test_helper_of_random_tables_equals_the_model(ctx, log_rows, n_proofs):
    """random 64-bit words (words above 2^32: only the low halves count; a nonzero partial block at the end; one block of the last proof
    zeroed in its low halves so that LIVE = 0 occurs): the helper equals the model's word for word, guard words intact"""
    rng = np.random.default_rng(9100 + 10 * log_rows + n_proofs)
    table = rng.integers(0, 1 << 64, (n_proofs * W, 1 << log_rows), dtype=np.uint64)
    table[(n_proofs - 1) * W:, 80] &= np.uint64(0xFFFFFFFF00000000)
    got = _down(_device_helper(ctx, table)).reshape(n_proofs * HC, -1)
    want = sm.helper(table, n_proofs)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    assert not want[(n_proofs - 1) * HC + sm.HLIVE, 80:160].any() and want[sm.HLIVE, :80].all()
    assert log_rows == 7 or want[sm.HLIVE, -1] == 1  # (the partial block at the end is live; at 128 rows it is the zeroed one)


@pytest.mark.gpu
def test_helper_of_the_devices_own_rows_equals_the_model(ctx, device_rows):
    """T.2 of two step N = 2 proofs as tmx_trace_rows_device writes it (512 rows: live and zero blocks, padding)"""
    table = device_rows[1]
    assert table.shape == (2 * W, 512) and table.any()
    got = _down(_device_helper(ctx, table)).reshape(-1, 512)
    assert np.array_equal(got, sm.helper(table, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,log_blowup", [(7, 1), (7, 3), (9, 1), (9, 3)])
def test_preprocessed_columns_and_their_extensions(ctx, oracle, log_rows, log_blowup):
    """SEL, KLO, KHI before the LDE and extended at blow-up 2 and 8 under the context's domain, against the model and the CPU oracle's LDE"""
    import torch
    N, M = 1 << log_rows, 1 << (log_rows + log_blowup)
    d_pre, d_ext = _sentinel(3 * N + 64), _sentinel(3 * M + 64)
    ctx.air_sha512_periodic_device(log_rows, log_blowup, d_pre.data_ptr(), d_ext.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(d_pre[3 * N:], _sentinel(3 * N + 64)[3 * N:]) and torch.equal(d_ext[3 * M:], _sentinel(3 * M + 64)[3 * M:])
    pre = sm.periodic(N)
    assert np.array_equal(_down(d_pre[:3 * N]).reshape(3, N), pre)
    assert np.array_equal(_down(d_ext[:3 * M]).reshape(3, M), oracle.lde(pre, log_blowup))
    assert pre[0].sum() == N - N // 80 - 1 and pre[0, N - 1] == 0 and pre[0, 79] == 0 and pre[0, 80] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows", [7, 9, 10, 15, 18])
def test_barycentric_values_equal_the_model(ctx, oracle, log_rows):
    """SEL, KLO, KHI at a random zeta of F_p^2 over N = 128 (half a workgroup), 512, 1024 (one), 2^15 (32 workgroups, the full size) and
    2^18 (64 workgroups, four batches per thread): the kernel's three values equal the model's barycentric sums, no zero denominator"""
    import torch
    rng = np.random.default_rng(9500 + log_rows)
    zeta = tuple(int(x) for x in rng.integers(1, P, 2, dtype=np.uint64))
    d_zeta, d_out = _up(np.array(zeta, dtype=np.uint64)), _sentinel(7 + 64)
    ctx.air_sha512_periodic_eval_device(log_rows, d_zeta.data_ptr(), d_out.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    got = [int(x) for x in _down(d_out[:7])]
    assert torch.equal(d_out[7:], _sentinel(7 + 64)[7:])
    want = sm.barycentric(oracle, log_rows, zeta)
    assert got == [w[k] for w in want for k in (0, 1)] + [0]


@pytest.mark.gpu
def test_barycentric_zero_denominator_is_flagged(ctx, oracle):
    """zeta = omega_N^5 lies on the trace domain: the kernel raises its flag (the verifier then clears every verdict)"""
    import torch
    d_zeta, d_out = _up(np.array([pow(oracle.gl_root(9), 5, P), 0], dtype=np.uint64)), _sentinel(7)
    ctx.air_sha512_periodic_eval_device(9, d_zeta.data_ptr(), d_out.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert int(_down(d_out)[6]) == 1


def _device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, cap_height=CAP_H, **kw):
    return _guarded(2 << log_n, lambda out: ctx.air_sha512_quotient_device(log_n, log_blowup, cap_height, n_proofs, d_cols.data_ptr(),
                                                                          d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(), out, 0, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,log_blowup,n_proofs", [(9, 1, 1), (9, 3, 3), (10, 1, 3), (10, 3, 1)])
def test_quotient_of_random_columns_equals_the_model(ctx, oracle, log_rows, log_blowup, n_proofs):
    """N = 512 and 1024, blow-up 2 and 8, one and three proofs, random table and helper columns (a few words non-canonical): the definition
    is pointwise, so gamma and d_quot equal the model word for word -- whole, and through the range call in two pieces in both orders (a
    written first piece and an accumulated second: [0, 1) then the rest, and the rest then [0, 1)); guard words intact"""
    import torch
    log_n = log_rows + log_blowup
    rng = np.random.default_rng(9200 + 100 * log_rows + 10 * log_blowup + n_proofs)
    ext, hext = _random_ext(rng, n_proofs * W, log_n), _random_ext(rng, n_proofs * HC, log_n)
    d_cols, d_hcols = _up(ext), _up(hext)
    _, d_cap = _tree(ctx, d_cols, log_n, n_proofs * W)
    _, d_cap_h = _tree(ctx, d_hcols, log_n, n_proofs * HC)
    got = _down(_device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h))
    g = sm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _down(d_cap), _down(d_cap_h))
    assert ctx.air_last_gamma() == g
    pext = oracle.lde(sm.periodic(1 << log_rows), log_blowup)
    want = sm.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, pext, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    pieces = [(0, 1), (1, n_proofs)] if n_proofs > 1 else [(0, 1)]
    for order in (pieces, pieces[::-1]):
        d_quot = _sentinel((2 << log_n) + 64)
        for k, (lo, hi) in enumerate(order):
            d_piece = d_hcols[(lo * HC) << log_n:]
            ctx.air_sha512_quotient_device(log_n, log_blowup, CAP_H, n_proofs, d_cols.data_ptr(), d_piece.data_ptr(), d_cap.data_ptr(),
                                           d_cap_h.data_ptr(), d_quot.data_ptr(), 0, proof_range=(lo, hi), accumulate=int(k > 0))
        torch.cuda.synchronize(_dev())
        assert np.array_equal(_down(d_quot[:2 << log_n]), want), order
        assert torch.equal(d_quot[2 << log_n:], _sentinel((2 << log_n) + 64)[2 << log_n:])


def _chain(ctx, oracle, table, log_blowup, quot_override=None, n_queries=6, others=()):
    """caller-level chain: helper -> LDE -> caps -> quotient -> one batch proof over [table, helper, quotient].  Returns (params, d_caps,
    proof words, extended table, extended helper, quotient words).  others: (position, extended columns [n][2^log_n]) of further oracles"""
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
    gamma = ctx.air_last_gamma() if quot_override is None else None
    d_lv_q, d_cap_q = _tree(ctx, d_quot, log_n, 2)
    log_ns, n_cols = [log_n] * 3, [n_proofs * W, n_proofs * HC, 2]
    d_cols, d_lvs, d_caps = [d_ext, d_hext, d_quot], [d_lv_t, d_lv_h, d_lv_q], [d_cap_t, d_cap_h, d_cap_q]
    for at, e in others:
        d_o = _up(e)
        lo = e.shape[1].bit_length() - 1
        d_lv_o, d_cap_o = _tree(ctx, d_o, lo, e.shape[0])
        log_ns.insert(at, lo), n_cols.insert(at, e.shape[0]), d_cols.insert(at, d_o), d_lvs.insert(at, d_lv_o), d_caps.insert(at, d_cap_o)
    p = bparams(log_ns, n_cols, CAP_H, log_blowup, 2, 2, n_queries)
    words = bm.layout(p)["words"]
    proof = _guarded(words, lambda out: ctx.batch_prove_device(p, [d.data_ptr() for d in d_cols], [d.data_ptr() for d in d_lvs], out, 0))
    return (p, torch.cat(d_caps), _down(proof), _down(d_ext).reshape(n_proofs * W, -1), _down(d_hext).reshape(n_proofs * HC, -1), _down(d_quot),
            gamma)


def _verdicts(ctx, p, k_trace, d_caps, proof, batch_only=False, sha256=False):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    if batch_only:
        ctx.batch_verify_device(p, d_caps.data_ptr(), _up(proof).data_ptr(), ok.data_ptr(), 0)
    elif sha256:
        ctx.air_sha256_verify_device(p, k_trace, d_caps.data_ptr(), _up(proof).data_ptr(), ok.data_ptr(), 0)
    else:
        ctx.air_sha512_verify_device(p, k_trace, d_caps.data_ptr(), _up(proof).data_ptr(), ok.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    out = ok.cpu().numpy()
    assert ((out == 0) | (out == 1)).all(), out
    return [bool(x) for x in out]


@pytest.mark.gpu
def test_real_rows_through_the_caller_level_chain(ctx, oracle, step2):
    """commit table -> helper -> LDE -> caps -> quotient -> tmx_batch_prove_device -> tmx_air_sha512_verify_device on T.2 of step N = 2 (two
    proofs, N = 512, blow-up 2): the quotient and gamma equal the model's and the quotient has degree <= N - 2; every verdict equals the
    model verifier's (all accept); a proof with one bumped table, helper or quotient opening is rejected on every query, by the device as by
    the model; the plain tmx_batch_verify_device still accepts the honest proof"""
    table, lb = step2, 1
    n_proofs = table.shape[0] // W
    p, d_caps, got, ext, hext, quot, gamma = _chain(ctx, oracle, table, lb)
    assert ctx.fri_last_degree_ok() is True
    log_n, caps, cw = p["log_n"][0], _down(d_caps), 4 << CAP_H
    assert np.array_equal(hext, oracle.lde(sm.helper(table, n_proofs), lb))
    g = sm.gamma(oracle, log_n, lb, CAP_H, n_proofs, caps[:cw], caps[cw:2 * cw])
    assert gamma == g
    pext = oracle.lde(sm.periodic(table.shape[1]), lb)
    assert np.array_equal(quot, sm.quotient(oracle, log_n, lb, n_proofs, ext, hext, pext, _shift(), g))
    assert max(_degrees(oracle, quot)) <= table.shape[1] - 2
    model = sm.verify(oracle, p, 0, caps, got, _shift())
    assert all(model) and _verdicts(ctx, p, 0, d_caps, got) == model
    assert all(_verdicts(ctx, p, 0, d_caps, got, batch_only=True))
    L = bm.layout(p)
    RH = 1 << dm.log_r(p["n_cols"][1])
    for name, at in (("quotient opening", L["off_open"][2] + 1), ("helper opening at zeta", L["off_open"][1] + sm.HE + 41),
                     ("helper opening at zeta omega", L["off_open"][1] + 2 * RH + HC + sm.HKL + 1),
                     ("table opening at zeta", L["off_open"][0] + W + sm.D_ + 1)):
        bad = got.copy()
        bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
        assert not sm.identity(oracle, p, 0, caps, bad), name
        model = sm.verify(oracle, p, 0, caps, bad, _shift())
        assert not any(model), name
        assert _verdicts(ctx, p, 0, d_caps, bad) == model, name


@pytest.mark.gpu
def test_zero_quotient_for_a_table_with_a_changed_a_hi(ctx, oracle, step2):
    """a zero (low-degree) quotient committed for a table with one changed a_hi and the honest helper of the changed table: the batch proof is
    fine -- tmx_batch_verify_device accepts every query -- and the identity fails: tmx_air_sha512_verify_device rejects every one, as the
    model does"""
    table = step2[:W].copy()
    table[sm.A_ + 1, _mid_row(table)[0]] ^= np.uint64(1 << 20)
    log_n = 9 + 1
    p, d_caps, got, _, _, _, _ = _chain(ctx, oracle, table, 1, quot_override=np.zeros(2 << log_n, dtype=np.uint64))
    caps = _down(d_caps)
    assert all(_verdicts(ctx, p, 0, d_caps, got, batch_only=True))
    model = sm.verify(oracle, p, 0, caps, got, _shift())
    assert not any(model) and _verdicts(ctx, p, 0, d_caps, got) == model


@pytest.mark.gpu
def test_257_proofs_through_the_check_kernel(ctx, oracle, step2):
    """N = 128, 257 proofs (one more than k_air_sha512_check<Sha512Round> has threads: thread 0 takes proofs 0 and 256) -- the live first blocks of T.2
    of step N = 2 in turn, 48 rows of padding behind each, every seventh proof zero --, blow-up 2, two queries: the device accepts every
    query as the model's identity does; a helper opening bumped in proof 256 and a table opening in proof 255 are rejected"""
    many = 257
    blocks = [step2[q * W:(q + 1) * W, 80 * b:80 * b + 80] for q in range(step2.shape[0] // W) for b in range(0, step2.shape[1] // 80, 2)
              if step2[q * W:(q + 1) * W, 80 * b].any()]
    assert blocks
    table = np.zeros((many * W, 128), dtype=np.uint64)
    for q in range(many):
        if q % 7 != 6:
            table[q * W:(q + 1) * W, :80] = blocks[q % len(blocks)]
    p, d_caps, got, _, _, _, _ = _chain(ctx, oracle, table, 1, n_queries=2)
    assert ctx.fri_last_degree_ok() is True
    caps = _down(d_caps)
    assert sm.identity(oracle, p, 0, caps, got)
    assert _verdicts(ctx, p, 0, d_caps, got) == [True, True]
    L = bm.layout(p)
    for at in (L["off_open"][1] + 256 * HC + sm.HS1 + 1, L["off_open"][0] + 255 * W + sm.E_):
        bad = got.copy()
        bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
        assert not sm.identity(oracle, p, 0, caps, bad)
        assert _verdicts(ctx, p, 0, d_caps, bad) == [False, False]


@pytest.mark.gpu
def test_set_level_on_the_sha512_table(ctx, oracle, device_rows):
    """a set SHA512 | HEADER at step N = 2, two proofs; the air call on SHA512: the pair sits directly behind the table with the two new ids;
    caps, gamma and proof words equal the caller-level chain's on the same columns (the header table as one more oracle); the device
    verifier accepts; the same set with tmx_trace_commit_set_air_sha256_device on HEADER works in both call orders; the refusals"""
    import torch
    from test_merkle_open import _oracle_ext
    c, (tr, table) = ctx, device_rows
    kind, n, n_proofs, lb = 1, 2, 2, 1
    cw = 4 << CAP_H
    d_caps, d_cap_h, d_cap_q = _sentinel(2 * cw), _sentinel(cw), _sentinel(cw)
    air = lambda sec: (lambda: c.trace_commit_set_air_sha512_device(sec, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0))
    commit = lambda secs=SHA512 | HEADER: c.trace_commit_set_device(kind, n_proofs, secs, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
    commit()
    shape0, order0 = c.trace_commit_set_shape()
    assert sorted(order0) == [SHA512, HEADER]
    # refusals on the fresh set: a section that is not SHA512 (present or not), null caps
    for sec in (HEADER, SHA256, 1, HELPER):
        assert "TMX_TRACE_SHA512" in _refused(air(sec), d_cap_h, d_cap_q)
    _refused(lambda: c.trace_commit_set_air_sha512_device(SHA512, None, d_cap_q.data_ptr(), 0), d_cap_q)
    _refused(lambda: c.trace_commit_set_air_sha512_device(SHA512, d_cap_h.data_ptr(), None, 0), d_cap_h)
    assert c.trace_commit_set_shape() == (shape0, order0)
    air(SHA512)()
    gamma = c.air_last_gamma()
    shape, order = c.trace_commit_set_shape()
    k = order.index(SHA512)
    assert order[k:k + 3] == [SHA512, HELPER, QUOTIENT] and sorted(order) == sorted([SHA512, HELPER, QUOTIENT, HEADER])
    assert shape["log_n"][k:k + 3] == [9 + lb] * 3 and shape["n_cols"][k:k + 3] == [W * n_proofs, HC * n_proofs, 2]
    assert "already" in _refused(air(SHA512), d_cap_h, d_cap_q)  # a second call on the section
    assert c.trace_commit_set_shape() == (shape, order)
    p = dict(shape, arity_bits=2, final_log_max=2, n_queries=6, pow_bits=0)
    after = _guarded(bm.layout(p)["words"], lambda out: c.trace_commit_set_prove_device(p, out, 0))
    assert c.fri_last_degree_ok() is True
    kh = order.index(HEADER)
    caps_of = {SHA512: d_caps[cw * order0.index(SHA512):][:cw], HEADER: d_caps[cw * order0.index(HEADER):][:cw], HELPER: d_cap_h, QUOTIENT: d_cap_q}
    all_caps = torch.cat([caps_of[s] for s in order])
    # the caller-level chain on the same columns, the header table's extended columns as one more oracle at its place
    e, lm, nc = _oracle_ext(oracle, kind, n, _down(tr), HEADER, lb)
    p2, d_caps2, proof2, _, _, _, gamma2 = _chain(c, oracle, table, lb, others=[(kh, e.reshape(nc, -1))])
    assert {key: p2[key] for key in ("log_n", "n_cols")} == {key: p[key] for key in ("log_n", "n_cols")}
    assert gamma == gamma2 and torch.equal(all_caps, d_caps2)
    assert np.array_equal(_down(after), proof2)
    assert _verdicts(c, p, k, all_caps, _down(after)) == [True] * 6
    assert sm.identity(oracle, p, k, _down(all_caps), _down(after))
    bad = _down(after).copy()
    at = bm.layout(p)["off_open"][k + 2]
    bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
    assert not any(_verdicts(c, p, k, all_caps, bad))
    # set 3's call on HEADER behind set 7's, then a fresh set with the two calls the other way round: the same set either way
    d_h3, d_q3, d_h7, d_q7 = (_sentinel(cw) for _ in range(4))
    c.trace_commit_set_air_sha256_device(HEADER, d_h3.data_ptr(), d_q3.data_ptr(), 0)
    shape_a, order_a = c.trace_commit_set_shape()
    pa = dict(shape_a, arity_bits=2, final_log_max=2, n_queries=6, pow_bits=0)
    proof_a = _guarded(bm.layout(pa)["words"], lambda out: c.trace_commit_set_prove_device(pa, out, 0))
    caps_of.update({128: d_h3, 256: d_q3})
    caps_a = torch.cat([caps_of[s] for s in order_a])
    assert all(_verdicts(c, pa, order_a.index(SHA512), caps_a, _down(proof_a)))
    assert all(_verdicts(c, pa, order_a.index(HEADER), caps_a, _down(proof_a), sha256=True))
    commit()
    c.trace_commit_set_air_sha256_device(HEADER, d_h3.data_ptr(), d_q3.data_ptr(), 0)
    c.trace_commit_set_air_sha512_device(SHA512, d_h7.data_ptr(), d_q7.data_ptr(), 0)
    assert c.trace_commit_set_shape() == (shape_a, order_a)
    assert torch.equal(d_h7, d_cap_h) and torch.equal(d_q7, d_cap_q)
    proof_b = _guarded(bm.layout(pa)["words"], lambda out: c.trace_commit_set_prove_device(pa, out, 0))
    assert torch.equal(proof_b, proof_a)
    # an absent section, a streamed section
    commit(HEADER)
    assert "does not hold" in _refused(air(SHA512), d_cap_h, d_cap_q)
    c.trace_commit_set_streamed_device(kind, n_proofs, SHA512 | HEADER, SHA512, 8, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
    assert "streamed" in _refused(air(SHA512), d_cap_h, d_cap_q)


@pytest.mark.gpu
def test_a_full_set_is_refused(built_lib):
    """all five tables, the ladders' quotient and one SHA-256 pair make eight oracles: set 7's pair has no room, and the set stays as it was"""
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    cw = 4 << CAP_H
    with tmx.Context(4, b"celestia", max_batch=1) as c:
        tr = _trace_rows(c, 0, 4, 1, 9400)
        d_caps, d_cap_h, d_cap_q = _sentinel(5 * cw), _sentinel(cw), _sentinel(cw)
        c.trace_commit_set_device(0, 1, 1 | SHA512 | SHA256 | 16 | HEADER, 1, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        c.trace_commit_set_air_device(d_cap_q.data_ptr(), 0)
        c.trace_commit_set_air_sha256_device(16, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
        before = c.trace_commit_set_shape()
        assert len(before[1]) == 8
        assert "room" in _refused(lambda: c.trace_commit_set_air_sha512_device(SHA512, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0), d_cap_h, d_cap_q)
        assert c.trace_commit_set_shape() == before


@pytest.mark.gpu
def test_each_validation_rule(ctx):
    """every rule on its own: TMX_ERR_BAD_ARG before anything is enqueued, nothing written.  7 <= log_n - log_blowup <= 18; 599 n_proofs <=
    2^24; a range inside n_proofs; accumulate <= 1; no null pointer; the verifier: column counts 18 k / 599 k / 2, equal log_n, all three
    oracles inside the proof; the streamed call keeps refusing every constraint set but 3, 4 and 5"""
    import torch
    log_n, lb = 9, 1
    d_cols, d_hcols = _sentinel(W << log_n), _sentinel(HC << log_n)
    d_cap, d_cap_h, d_quot = _sentinel(4 << CAP_H), _sentinel(4 << CAP_H), _sentinel(2 << log_n)
    ptrs = [d_cols.data_ptr(), d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(), d_quot.data_ptr()]
    q = lambda ln, b, n, a=ptrs, **kw: (lambda: ctx.air_sha512_quotient_device(ln, b, CAP_H, n, *a, 0, **kw))
    for fn in (q(log_n, 0, 1), q(log_n, 7, 1), q(2, 2, 1), q(29, 2, 1), q(7, 1, 1), q(20, 1, 1), q(log_n, lb, 0), q(log_n, lb, (1 << 24) // HC + 1),
               q(log_n, lb, 2, proof_range=(1, 1)), q(log_n, lb, 2, proof_range=(1, 3)), q(log_n, lb, 2, proof_range=(0, 1), accumulate=2)):
        _refused(fn, d_quot)
    for k in range(5):
        _refused(q(log_n, lb, 1, ptrs[:k] + [None] + ptrs[k + 1:]), d_quot)
    d_table, d_help = _sentinel(W << 7), _sentinel(HC << 7)
    hp = lambda lr, n, t=d_table.data_ptr(), o=d_help.data_ptr(): (lambda: ctx.air_sha512_helper_device(lr, n, t, o, 0))
    for fn in (hp(6, 1), hp(19, 1), hp(7, 0), hp(7, (1 << 24) // HC + 1), hp(7, 1, t=None), hp(7, 1, o=None)):
        _refused(fn, d_help)
    d_pre, d_out = _sentinel(3 << 8), _sentinel(8)
    for fn in (lambda: ctx.air_sha512_periodic_device(6, 1, d_pre.data_ptr(), d_pre.data_ptr(), 0),
               lambda: ctx.air_sha512_periodic_device(19, 1, d_pre.data_ptr(), d_pre.data_ptr(), 0),
               lambda: ctx.air_sha512_periodic_device(7, 1, None, d_pre.data_ptr(), 0),
               lambda: ctx.air_sha512_periodic_device(7, 1, d_pre.data_ptr(), None, 0),
               lambda: ctx.air_sha512_periodic_eval_device(6, d_pre.data_ptr(), d_out.data_ptr(), 0),
               lambda: ctx.air_sha512_periodic_eval_device(19, d_pre.data_ptr(), d_out.data_ptr(), 0),
               lambda: ctx.air_sha512_periodic_eval_device(7, None, d_out.data_ptr(), 0),
               lambda: ctx.air_sha512_periodic_eval_device(7, d_pre.data_ptr(), None, 0)):
        _refused(fn, d_pre, d_out)
    # the verifier
    ok, caps, proof = torch.full((4,), 7, dtype=torch.int32, device=_dev()), _sentinel(256), _sentinel(1 << 17)
    v = lambda p, k: (lambda: ctx.air_sha512_verify_device(p, k, caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0))
    good = bparams([9, 9, 9], [W, HC, 2], CAP_H, lb, 2, 2, 4)
    for p, k in ((good, 1), (dict(good, n_cols=[W + 1, HC, 2]), 0), (dict(good, n_cols=[9, HC, 2]), 0), (dict(good, n_cols=[W, HC + 1, 2]), 0),
                 (dict(good, n_cols=[2 * W, HC, 2]), 0), (dict(good, n_cols=[W, HC, 3]), 0), (dict(good, log_n=[9, 9, 8]), 0),
                 (bparams([7, 7, 7], [W, HC, 2], CAP_H, lb, 2, 2, 4), 0), (dict(good, arity_bits=0), 0),
                 (bparams([9, 9], [W, HC], CAP_H, lb, 2, 2, 4), 0)):
        _refused(v(p, k), ok)
    d_c = _sentinel(8 << CAP_H)
    _refused(lambda: ctx.trace_commit_set_air_sha256_streamed_device(7, SHA512, 8, d_c.data_ptr(), d_c.data_ptr(), 0), d_c)
