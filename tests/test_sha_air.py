"""The round constraints of the SHA-256 tables (include/tmx.h "the round constraints of the SHA-256 tables", constraint set 3):
tmx_air_sha256_helper_device, tmx_air_sha256_quotient_device, tmx_air_sha256_verify_device, tmx_trace_commit_set_air_sha256_device.  The
yardstick is tests/sha_air_model.py (the helper, gamma, the quotient point by point, the identity at zeta) on top of tests/batch_model.py:
device words must equal the model's word for word and every verdict of the device verifier must equal the model verifier's.  The CPU part
ties the model itself to the claim: on the CPU oracle's T.3, T.5 and T.6 rows all 315 constraints hold as integer identities, the quotient
is a polynomial of degree < N, and one change of a detected kind makes it one of degree >= N; the kinds the set does NOT see are recorded
next to them."""
import numpy as np
import pytest

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha_air_model as sm
from batch_model import bparams
from test_fri import _down, _sentinel, _shift, _up
from test_merkle_open import _section_geom

P = fm.P
BAD_ARG = -1
SHA256, TREE, HEADER, HELPER, QUOTIENT = 4, 16, 32, 128, 256
W, HC = sm.WIDTH, sm.HELPER_COLS
CAP_H = 2


# ---- the CPU oracle's SHA-256 tables
def _sha_tables(oracle, kind, n, n_proofs, seed):
    """{section: [9 n_proofs][2^log_rows] pre-LDE columns} of T.3, T.5 and T.6 of n_proofs synthetic proofs from the CPU oracle (zero padded
    to a power of two, as the commit pipeline pads them)"""
    from tendermintx_amd.synth import Workload
    wl = Workload(kind, n, n_proofs, n, chain_id=b"celestia", seed=seed, signed_permille=900)
    out = {}
    fulls = []
    for p in range(n_proofs):
        t = wl.targets[p * n * 256:(p + 1) * n * 256]
        r = wl.trusteds[p * n * 48:(p + 1) * n * 48] if kind == 0 else None
        fulls.append(oracle.trace(kind, wl.proofs[p * 2336:(p + 1) * 2336], t, r, n))
    for sec in (SHA256, TREE, HEADER):
        off, rows, width = _section_geom(kind, n, sec)
        assert width == W and rows % 64 == 0
        cols = np.zeros((n_proofs * W, 1 << max(6, (rows - 1).bit_length())), dtype=np.uint64)
        for p, full in enumerate(fulls):
            cols[p * W:(p + 1) * W, :rows] = full[off:off + rows * W].reshape(rows, W).T
        out[sec] = cols
    return out


@pytest.fixture(scope="module")
def skip4(oracle):
    return _sha_tables(oracle, 0, 4, 2, 8100)


@pytest.fixture(scope="module")
def step2(oracle):
    return _sha_tables(oracle, 1, 2, 2, 8200)


@pytest.fixture(scope="module")
def step3(oracle):
    return _sha_tables(oracle, 1, 3, 2, 8300)


def test_rows_satisfy_the_constraints_as_integers(skip4, step2, step3):
    """all 315 constraints hold as integer identities (no reduction mod p) on every row of T.3, T.5 and T.6 of skip N = 4, step N = 2 and
    step N = 3, the selected ones on every row but the last of a block; every value is below 2^32; live and all-zero blocks both occur; the
    model helper's LIVE is "the block is not all zero"; the largest carries are printed"""
    live_blocks = zero_blocks = 0
    ca_max = ce_max = 0
    for name, tables in (("skip4", skip4), ("step2", step2), ("step3", step3)):
        for sec, table in tables.items():
            assert int(table.max()) < 1 << 32
            n_proofs = table.shape[0] // W
            help_ = sm.helper(table, n_proofs)
            assert help_.shape == (n_proofs * HC, table.shape[1]) and int(help_.max()) < 1 << 32
            for p in range(n_proofs):
                t, h = table[p * W:(p + 1) * W], help_[p * HC:(p + 1) * HC]
                res = sm.integer_residuals(t, h)
                for j, c in enumerate(res):
                    assert not c.any(), (name, sec, p, j, np.flatnonzero(c)[:4])
                blocks = t.reshape(W, -1, 64)
                nonzero = blocks.any(axis=(0, 2))
                assert np.array_equal(h[sm.HLIVE].reshape(-1, 64), np.repeat(nonzero[:, None], 64, axis=1).astype(np.uint64))
                live_blocks += int(nonzero.sum())
                zero_blocks += int((~nonzero).sum())
                ca = h[sm.HCA] + 2 * h[sm.HCA + 1] + 4 * h[sm.HCA + 2]
                ce = h[sm.HCE] + 2 * h[sm.HCE + 1] + 4 * h[sm.HCE + 2]
                ca_max, ce_max = max(ca_max, int(ca.max())), max(ce_max, int(ce.max()))
    print(f"\n[sha-air] live blocks {live_blocks}, zero blocks {zero_blocks}, largest carries a {ca_max} e {ce_max}")
    assert live_blocks and zero_blocks and ca_max <= 6 and ce_max <= 5


def test_model_field_arithmetic_equals_python_integers(oracle):
    """the model's uint64 field (sha_air_model._mulv and friends) against Python integers: edge values and random ones, and one whole
    quotient of random columns both ways"""
    rng = np.random.default_rng(9000)
    edge = np.array([0, 1, 2, P - 1, P - 2, 1 << 32, (1 << 32) - 1, (1 << 32) + 1, P >> 1, 0xFFFFFFFF00000000], dtype=np.uint64)
    a = np.concatenate([np.repeat(edge, edge.size), rng.integers(0, P, 4000, dtype=np.uint64)])
    b = np.concatenate([np.tile(edge, edge.size), rng.integers(0, P, 4000, dtype=np.uint64)])
    ai, bi = [int(x) for x in a], [int(x) for x in b]
    with np.errstate(over="ignore"):
        assert [int(x) for x in sm._mulv(a, b)] == [x * y % P for x, y in zip(ai, bi)]
        assert [int(x) for x in sm._addv(a, b)] == [(x + y) % P for x, y in zip(ai, bi)]
        assert [int(x) for x in sm._subv(a, b)] == [(x - y) % P for x, y in zip(ai, bi)]
        assert [int(x) for x in sm._mulv(a, np.uint64(P - 1))] == [x * (P - 1) % P for x in ai]
    ext, hext = rng.integers(0, 1 << 64, (W, 256), dtype=np.uint64), rng.integers(0, 1 << 64, (HC, 256), dtype=np.uint64)
    g = (0x0123456789ABCDEF % P, 0xFEDCBA9876543210 % P)
    assert np.array_equal(sm.quotient(oracle, 8, 1, 1, ext, hext, _shift(), g), sm.quotient(oracle, 8, 1, 1, ext, hext, _shift(), g, ints=True))


LB = 2  # blow-up 4 in the CPU tests


def _cap(oracle, ext, log_n, cap_height=CAP_H):
    h = min(cap_height, log_n)
    return oracle.poseidon_merkle(np.ascontiguousarray(ext).reshape(-1), log_n, ext.shape[0], h)[-(1 << h):].reshape(-1)


def _model_quotient(oracle, table, help_, log_blowup=LB):
    """(extended table, extended helper, gamma, planar quotient) of pre-LDE columns"""
    n_proofs, log_n = table.shape[0] // W, table.shape[1].bit_length() - 1 + log_blowup
    ext, hext = oracle.lde(table, log_blowup), oracle.lde(help_, log_blowup)
    g = sm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _cap(oracle, ext, log_n), _cap(oracle, hext, log_n))
    return ext, hext, g, sm.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, _shift(), g)


def _degrees(oracle, quot):
    M = quot.size // 2
    return [am.degree(am.coefficients(oracle, quot[k * M:(k + 1) * M], _shift())) for k in (0, 1)]


@pytest.mark.parametrize("which", ["T.3 of skip N = 4", "T.5 of step N = 3"])
def test_quotient_is_a_polynomial_of_degree_below_n(oracle, skip4, step3, which):
    """two proofs, blow-up 4: the model quotient of the honest tables (512 rows; T.5 with padding, zero blocks and chained second blocks)
    interpolates to degree < N in both planes, and the identity holds at a zeta outside the base field -- table, helper and quotient
    polynomials evaluated there by Horner on their coefficients; it fails after bumping u_0, a table opening or a helper opening"""
    table = skip4[SHA256] if which.startswith("T.3") else step3[TREE]
    N = table.shape[1]
    assert N == 512
    log_n, n_proofs = N.bit_length() - 1 + LB, table.shape[0] // W
    help_ = sm.helper(table, n_proofs)
    ext, hext, g, quot = _model_quotient(oracle, table, help_)
    deg = _degrees(oracle, quot)
    print(f"\n[sha-air] {which}: N = {N}, quotient degrees {deg}")
    assert max(deg) < N and g[1] != 0
    M = 1 << log_n
    zeta = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)
    zs = (zeta, fm.e_scale(zeta, oracle.gl_root(log_n - LB)))
    yt, yh = dm.evaluate(oracle, table, 1, zs), dm.evaluate(oracle, help_, 1, zs)
    u = [am.horner(am.coefficients(oracle, quot[k * M:(k + 1) * M], _shift()), zeta) for k in (0, 1)]
    t0, t1, h0, h1 = [tuple(y[0]) for y in yt], [tuple(y[1]) for y in yt], [tuple(y[0]) for y in yh], [tuple(y[1]) for y in yh]
    ident = lambda t0=t0, t1=t1, h0=h0, h1=h1, u0=u[0]: sm.identity_at(oracle, log_n, LB, n_proofs, t0, t1, h0, h1, u0, u[1], zeta, g)
    assert ident()
    assert not ident(u0=fm.e_add(u[0], (1, 0)))
    bump = lambda v, at: v[:at] + [fm.e_add(v[at], (0, 1))] + v[at + 1:]
    assert not ident(t0=bump(t0, W + sm.D_)) and not ident(t1=bump(t1, sm.W_))
    assert not ident(h0=bump(h0, sm.HV + 7)) and not ident(h1=bump(h1, HC + sm.HKL))


def _mid_row(table):
    """a row in the middle of a live block of proof 0's table, and that block's first row"""
    live = np.flatnonzero(table[:W].reshape(W, -1, 64).any(axis=(0, 2)))
    b = int(live[len(live) // 2])
    return 64 * b + 29, 64 * b


def _rerun(table, r0, first, last):
    """rows first .. last of the block at r0 recomputed from row first - 1 with the round function, the W column as it stands"""
    t = table.copy()
    state = [int(t[c, first - 1]) for c in range(1, 9)]
    for r in range(first, last + 1):
        state = sm.sha_round(state, int(t[sm.W_, r]), r - r0)
        t[1:9, r] = state
    return t


def _tampered(table, kind):
    """(table, helper) of ONE proof after a single change of `kind`"""
    t = table[:W].copy()
    r, r0 = _mid_row(t)
    if kind == "a changed a":
        t[sm.A_, r] ^= np.uint64(1 << 9)
        return t, sm.helper(t, 1)
    if kind == "a changed W":
        t[sm.W_, r] ^= np.uint64(1 << 20)
        return t, sm.helper(t, 1)
    h = sm.helper(t, 1)
    if kind == "a flipped helper bit":
        h[sm.HE + 5, r] ^= np.uint64(1)
    elif kind == "a changed carry bit":
        h[sm.HCA, r] ^= np.uint64(1)
    elif kind == "LIVE flipped on one row":
        h[sm.HLIVE, r] ^= np.uint64(1)
    elif kind == "a block re-run from a changed W_t, t >= 16":
        t[sm.W_, r0 + 20] ^= np.uint64(1 << 3)
        t = _rerun(t, r0, r0 + 20, r0 + 63)
        h = sm.helper(t, 1)
    elif kind == "a block re-run from a changed row-0 state":
        t[sm.C_, r0] ^= np.uint64(1 << 17)
        t = _rerun(t, r0, r0 + 1, r0 + 63)
        h = sm.helper(t, 1)
    else:
        raise KeyError(kind)
    return t, h


DETECTED = ["a changed a", "a changed W", "a flipped helper bit", "a changed carry bit", "LIVE flipped on one row"]
UNDETECTED = ["a block re-run from a changed W_t, t >= 16", "a block re-run from a changed row-0 state"]


@pytest.mark.parametrize("kind", DETECTED)
def test_one_change_breaks_the_degree(oracle, skip4, kind):
    """the detected kinds, on T.3 of skip N = 4 (one proof): the first two change the table mid-block and regenerate the helper from it, the
    others change the helper alone; the quotient no longer interpolates to degree < N"""
    table = skip4[SHA256][:W]
    t, h = _tampered(table, kind)
    assert (t != table).sum() + (h != sm.helper(table, 1)).sum() >= 1
    deg = _degrees(oracle, _model_quotient(oracle, t, h)[3])
    print(f"\n[sha-air] {kind}: quotient degrees {deg}, N = {table.shape[1]}")
    assert max(deg) >= table.shape[1]


@pytest.mark.parametrize("kind", UNDETECTED)
def test_kinds_the_constraints_do_not_see(oracle, skip4, kind):
    """recorded so that nobody mistakes the claim: the message schedule and row 0 against the IV are not in the set -- a block re-run
    consistently with the round function from a changed W_t (t >= 16) or from a changed row-0 state keeps the quotient low-degree"""
    table = skip4[SHA256][:W]
    t, h = _tampered(table, kind)
    assert (t != table).sum() > 8
    assert max(_degrees(oracle, _model_quotient(oracle, t, h)[3])) < table.shape[1]


def test_symbols_and_wrappers_exist(built_lib):
    """the new entry points are in the built library, bound in _lib.py and wrapped in context.py"""
    from tendermintx_amd import _lib
    from tendermintx_amd.context import Context
    for name in ("tmx_air_sha256_helper_device", "tmx_air_sha256_quotient_device", "tmx_air_sha256_verify_device",
                 "tmx_trace_commit_set_air_sha256_device"):
        assert getattr(built_lib, name).argtypes, name
        assert callable(getattr(Context, name[4:])), name
    assert (_lib.AIR_SHA256_HELPER_COLS, _lib.AIR_SHA256_CONSTRAINTS) == (HC, sm.CONSTRAINTS)
    assert (_lib.TRACE_SHA256_HELPER, _lib.TRACE_SHA256_QUOTIENT) == (HELPER, QUOTIENT)


# ---- GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


GUARD = 64


@pytest.fixture(scope="module")
def ctx(built_lib):
    import tendermintx_amd as tmx
    c = tmx.Context(4, b"celestia")
    yield c
    c.close()


def _guarded(words, fn):
    """fn(pointer) writes `words` words between two sentinel blocks that must stay untouched; returns the words"""
    import torch
    buf = _sentinel(words + 2 * GUARD)
    fn(buf[GUARD:].data_ptr())
    torch.cuda.synchronize(_dev())
    want = _sentinel(GUARD)
    assert torch.equal(buf[:GUARD], want) and torch.equal(buf[GUARD + words:], want)
    return buf[GUARD:GUARD + words].clone()


def _device_helper(ctx, table):
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    d_table = _up(table)
    return _guarded((n_proofs * HC) << log_rows, lambda out: ctx.air_sha256_helper_device(log_rows, n_proofs, d_table.data_ptr(), out, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("n_proofs", [1, 3])
def test_helper_of_random_tables_equals_the_model(ctx, n_proofs):
    """random 64-bit words (two blocks of 64 rows per proof; one block of one proof zeroed so that LIVE = 0 occurs): the helper equals the
    model's word for word, guard words intact"""
    rng = np.random.default_rng(9100 + n_proofs)
    table = rng.integers(0, 1 << 64, (n_proofs * W, 128), dtype=np.uint64)
    table[(n_proofs - 1) * W:, 64:] = 0
    got = _down(_device_helper(ctx, table)).reshape(n_proofs * HC, -1)
    want = sm.helper(table, n_proofs)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    live = np.ones((n_proofs, 128), dtype=np.uint64)
    live[-1, 64:] = 0
    assert np.array_equal(want[sm.HLIVE::HC], live)


@pytest.mark.gpu
def test_helper_of_real_tree_rows_equals_the_model(ctx, step3):
    """the real T.5 rows of step N = 3 (two proofs, 512 rows with padding, zero blocks and chained second blocks)"""
    table = step3[TREE]
    got = _down(_device_helper(ctx, table)).reshape(-1, table.shape[1])
    assert np.array_equal(got, sm.helper(table, table.shape[0] // W))


def _tree(ctx, d_cols, log_n, n_cols, cap_height=CAP_H):
    """(levels, cap) on the device"""
    h = min(cap_height, log_n)
    d_lv = _sentinel(4 * ctx.poseidon_merkle_digests(log_n, h))
    ctx.poseidon_merkle_device(log_n, n_cols, d_cols.data_ptr(), h, d_lv.data_ptr(), 0)
    return d_lv, d_lv[-(4 << h):]


def _device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, cap_height=CAP_H):
    return _guarded(2 << log_n, lambda out: ctx.air_sha256_quotient_device(log_n, log_blowup, cap_height, n_proofs, d_cols.data_ptr(),
                                                                          d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(), out, 0))


def _random_ext(rng, n_cols, log_n):
    """random words, non-satisfying and of full degree; a few of them non-canonical"""
    ext = rng.integers(0, P, (n_cols, 1 << log_n), dtype=np.uint64)
    ext[0, ::5] = rng.integers(0, 1 << 31, ext[0, ::5].size, dtype=np.uint64) + np.uint64(P)
    ext[n_cols - 1, 1::7] = np.uint64(P)
    return ext


@pytest.mark.gpu
@pytest.mark.parametrize("log_blowup,n_proofs,cap_height", [(1, 1, 0), (1, 3, 2), (3, 1, 2), (3, 3, 0)])
def test_quotient_of_random_columns_equals_the_model(ctx, oracle, log_blowup, n_proofs, cap_height):
    """N = 128 (two blocks: the smallest shape with a seam and the wrap-around), random table and helper columns: the definition is
    pointwise, so d_quot and gamma equal the model word for word, guard words intact"""
    log_n = 7 + log_blowup
    rng = np.random.default_rng(9200 + 10 * log_blowup + n_proofs)
    ext, hext = _random_ext(rng, n_proofs * W, log_n), _random_ext(rng, n_proofs * HC, log_n)
    d_cols, d_hcols = _up(ext), _up(hext)
    _, d_cap = _tree(ctx, d_cols, log_n, n_proofs * W, cap_height)
    _, d_cap_h = _tree(ctx, d_hcols, log_n, n_proofs * HC, cap_height)
    got = _down(_device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, cap_height))
    g = sm.gamma(oracle, log_n, log_blowup, cap_height, n_proofs, _down(d_cap), _down(d_cap_h))
    assert ctx.air_last_gamma() == g
    want = sm.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


def _chain(ctx, oracle, table, log_blowup, quot_override=None, n_queries=6, front=None):
    """caller-level chain: helper -> LDE -> caps -> quotient -> one batch proof over [table, helper, quotient].  Returns (params, d_caps,
    proof words, extended table, extended helper, quotient words).  front: the extended columns [n][2^(log_n + 1)] of one more oracle that
    goes in front of the table (the table is then oracle 1)"""
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
    log_ns, n_cols = [log_n] * 3, [n_proofs * W, n_proofs * HC, 2]
    d_cols, d_lvs, d_caps = [d_ext, d_hext, d_quot], [d_lv_t, d_lv_h, d_lv_q], [d_cap_t, d_cap_h, d_cap_q]
    if front is not None:
        d_front = _up(front)
        d_lv_f, d_cap_f = _tree(ctx, d_front, log_n + 1, front.shape[0])
        log_ns, n_cols = [log_n + 1] + log_ns, [front.shape[0]] + n_cols
        d_cols, d_lvs, d_caps = [d_front] + d_cols, [d_lv_f] + d_lvs, [d_cap_f] + d_caps
    p = bparams(log_ns, n_cols, CAP_H, log_blowup, 2, 2, n_queries)
    words = bm.layout(p)["words"]
    proof = _guarded(words, lambda out: ctx.batch_prove_device(p, [d.data_ptr() for d in d_cols], [d.data_ptr() for d in d_lvs], out, 0))
    return (p, torch.cat(d_caps), _down(proof), _down(d_ext).reshape(n_proofs * W, -1), _down(d_hext).reshape(n_proofs * HC, -1), _down(d_quot))


def _verdicts(ctx, p, k_trace, d_caps, proof, batch_only=False):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    if batch_only:
        ctx.batch_verify_device(p, d_caps.data_ptr(), _up(proof).data_ptr(), ok.data_ptr(), 0)
    else:
        ctx.air_sha256_verify_device(p, k_trace, d_caps.data_ptr(), _up(proof).data_ptr(), ok.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    out = ok.cpu().numpy()
    assert ((out == 0) | (out == 1)).all(), out
    return [bool(x) for x in out]


@pytest.mark.gpu
@pytest.mark.parametrize("which,log_blowup", [("T.3 of skip N = 4", 2), ("T.5 of step N = 3", 1)])
def test_real_tables_through_the_caller_level_chain(ctx, oracle, skip4, step3, which, log_blowup):
    """helper -> LDE -> caps -> quotient -> tmx_batch_prove_device -> tmx_air_sha256_verify_device on the real T.3 and T.5 rows: the quotient
    and gamma equal the model's and the quotient has degree < N; every verdict equals the model verifier's (all accept); a proof with one
    bumped quotient or helper opening is rejected on every query; the plain tmx_batch_verify_device still accepts the honest proof"""
    table = skip4[SHA256] if which.startswith("T.3") else step3[TREE]
    n_proofs = table.shape[0] // W
    p, d_caps, got, ext, hext, quot = _chain(ctx, oracle, table, log_blowup)
    assert ctx.fri_last_degree_ok() is True
    log_n, caps, cw = p["log_n"][0], _down(d_caps), 4 << CAP_H
    assert np.array_equal(hext, oracle.lde(sm.helper(table, n_proofs), log_blowup))
    g = sm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, caps[:cw], caps[cw:2 * cw])
    assert np.array_equal(quot, sm.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, _shift(), g))
    assert max(_degrees(oracle, quot)) < table.shape[1]
    model = sm.verify(oracle, p, 0, caps, got, _shift())
    assert all(model) and _verdicts(ctx, p, 0, d_caps, got) == model
    assert all(_verdicts(ctx, p, 0, d_caps, got, batch_only=True))
    L = bm.layout(p)
    RH = 1 << dm.log_r(p["n_cols"][1])
    for name, at in (("quotient opening", L["off_open"][2] + 1), ("helper opening at zeta", L["off_open"][1] + sm.HE + 9),
                     ("helper opening at zeta omega", L["off_open"][1] + 2 * RH + sm.HKL), ("table opening at zeta", L["off_open"][0] + sm.D_)):
        bad = got.copy()
        bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
        assert not sm.identity(oracle, p, 0, caps, bad), name
        model = sm.verify(oracle, p, 0, caps, bad, _shift())
        assert not any(model), name
        assert _verdicts(ctx, p, 0, d_caps, bad) == model, name


@pytest.mark.gpu
def test_zero_quotient_for_a_tampered_table(ctx, oracle, skip4):
    """a zero (low-degree) quotient committed for a table with one changed W: the batch proof is fine -- tmx_batch_verify_device accepts every
    query -- and the identity fails: tmx_air_sha256_verify_device rejects every one, as the model does"""
    table = skip4[SHA256][:W].copy()
    table[sm.W_, _mid_row(table)[0]] ^= np.uint64(1 << 20)
    log_n = table.shape[1].bit_length() - 1 + 1
    p, d_caps, got, _, _, _ = _chain(ctx, oracle, table, 1, quot_override=np.zeros(2 << log_n, dtype=np.uint64))
    caps = _down(d_caps)
    assert all(_verdicts(ctx, p, 0, d_caps, got, batch_only=True))
    model = sm.verify(oracle, p, 0, caps, got, _shift())
    assert not any(model) and _verdicts(ctx, p, 0, d_caps, got) == model


def _refused(fn, *outs):
    import torch
    from tendermintx_amd._lib import TmxError
    before = [o.clone() for o in outs]
    with pytest.raises(TmxError) as e:
        fn()
    torch.cuda.synchronize(_dev())
    assert e.value.status == BAD_ARG, e.value
    for a, b in zip(outs, before):
        assert torch.equal(a, b)
    return str(e.value)


@pytest.mark.gpu
def test_set_level_on_the_header_table(built_lib, oracle):
    """a set SHA256 + HEADER at step N = 2, two proofs; the air call on HEADER: the shape, the section ids, both caps against the model, one
    proof over the four oracles, the device verifier and the model's; the refusals; a set without the call proves what it proved"""
    import torch
    import tendermintx_amd as tmx
    from test_merkle_open import _oracle_ext, _trace_rows
    kind, n, n_proofs, lb = 1, 2, 2, 1
    cw = 4 << CAP_H
    with tmx.Context(n, b"celestia", max_batch=n_proofs) as c:
        tr = _trace_rows(c, kind, n, n_proofs, 9300)
        d_caps, d_cap_h, d_cap_q = _sentinel(2 * cw), _sentinel(cw), _sentinel(cw)
        air = lambda sec: (lambda: c.trace_commit_set_air_sha256_device(sec, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0))
        assert "no commit set" in _refused(air(HEADER), d_cap_h, d_cap_q)
        commit = lambda: c.trace_commit_set_device(kind, n_proofs, SHA256 | HEADER, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        commit()
        shape0, order0 = c.trace_commit_set_shape()
        assert order0 == [HEADER, SHA256] and shape0["log_n"] == [12 + lb, 7 + lb]
        p0 = dict(shape0, arity_bits=2, final_log_max=2, n_queries=6, pow_bits=0)
        before = _sentinel(bm.layout(p0)["words"])
        c.trace_commit_set_prove_device(p0, before.data_ptr(), 0)
        # refusals on the fresh set: an absent section, a section that is no SHA-256 table, null caps
        _refused(air(TREE), d_cap_h, d_cap_q)
        _refused(air(1), d_cap_h, d_cap_q)
        _refused(air(HELPER), d_cap_h, d_cap_q)
        _refused(lambda: c.trace_commit_set_air_sha256_device(HEADER, None, d_cap_q.data_ptr(), 0), d_cap_q)
        _refused(lambda: c.trace_commit_set_air_sha256_device(HEADER, d_cap_h.data_ptr(), None, 0), d_cap_h)
        air(HEADER)()
        gamma = c.air_last_gamma()
        shape, order = c.trace_commit_set_shape()
        assert order == [HEADER, HELPER, QUOTIENT, SHA256]
        assert shape["log_n"] == [12 + lb] * 3 + [7 + lb] and shape["n_cols"] == [W * n_proofs, HC * n_proofs, 2, W * n_proofs]
        _refused(air(HEADER), d_cap_h, d_cap_q)  # a second call on the same section
        p = dict(shape, arity_bits=2, final_log_max=2, n_queries=6, pow_bits=0)
        words = bm.layout(p)["words"]
        after = _guarded(words, lambda out: c.trace_commit_set_prove_device(p, out, 0))
        assert c.fri_last_degree_ok() is True
        all_caps = torch.cat([d_caps[:cw], d_cap_h, d_cap_q, d_caps[cw:]])
        caps_h, got = _down(all_caps), _down(after)
        # the model: the header table from the device's trace rows, its helper, both caps, gamma, the quotient and its cap
        traces = _down(tr)
        e, lm, nc = _oracle_ext(oracle, kind, n, traces, HEADER, lb)
        ext = e.reshape(nc, -1)
        off, rows, width = _section_geom(kind, n, HEADER)
        table = np.zeros((n_proofs * W, 1 << (lm - lb)), dtype=np.uint64)
        for q, full in enumerate(traces):
            table[q * W:(q + 1) * W, :rows] = full[off:off + rows * W].reshape(rows, W).T
        hext = oracle.lde(sm.helper(table, n_proofs), lb)
        # (the helper's cap through the device's Poseidon tree over the MODEL's helper words: the CPU oracle takes half a minute for 600
        # columns of 2^13 rows, and tmx_poseidon_merkle_device is tied to it word for word in tests/test_poseidon_gpu.py)
        assert np.array_equal(caps_h[:cw], _cap(oracle, ext, lm))
        assert np.array_equal(caps_h[cw:2 * cw], _down(_tree(c, _up(hext), lm, n_proofs * HC)[1]))
        assert gamma == sm.gamma(oracle, lm, lb, CAP_H, n_proofs, caps_h[:cw], caps_h[cw:2 * cw])
        quot = sm.quotient(oracle, lm, lb, n_proofs, ext, hext, _shift(), gamma)
        assert np.array_equal(caps_h[2 * cw:3 * cw], _cap(oracle, quot.reshape(2, -1), lm))
        model = sm.verify(oracle, p, 0, caps_h, got, _shift())
        assert all(model) and _verdicts(c, p, 0, all_caps, got) == model
        bad = got.copy()
        at = bm.layout(p)["off_open"][2]
        bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
        assert not any(_verdicts(c, p, 0, all_caps, bad)) and not sm.identity(oracle, p, 0, caps_h, bad)
        # the other SHA-256 member takes the call too: six oracles; a third pair would exceed eight
        d_cap_h2, d_cap_q2 = _sentinel(cw), _sentinel(cw)
        c.trace_commit_set_air_sha256_device(SHA256, d_cap_h2.data_ptr(), d_cap_q2.data_ptr(), 0)
        shape2, order2 = c.trace_commit_set_shape()
        assert order2 == [HEADER, HELPER, QUOTIENT, SHA256, HELPER, QUOTIENT]
        p2 = dict(shape2, arity_bits=2, final_log_max=2, n_queries=6, pow_bits=0)
        proof2 = _guarded(bm.layout(p2)["words"], lambda out: c.trace_commit_set_prove_device(p2, out, 0))
        caps2 = torch.cat([all_caps, d_cap_h2, d_cap_q2])
        assert all(_verdicts(c, p2, 0, caps2, _down(proof2))) and all(_verdicts(c, p2, 3, caps2, _down(proof2)))
        assert sm.identity(oracle, p2, 3, _down(caps2), _down(proof2))
        # a streamed member is refused; a fresh set without the call proves what the set proved before the call
        c.trace_commit_set_streamed_device(kind, n_proofs, SHA256 | HEADER, HEADER, 8, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        assert "streamed" in _refused(air(HEADER), d_cap_h, d_cap_q)
        commit()
        assert c.trace_commit_set_shape() == (shape0, order0)
        fresh = _sentinel(bm.layout(p0)["words"])
        c.trace_commit_set_prove_device(p0, fresh.data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        assert torch.equal(fresh, before)


@pytest.mark.gpu
def test_a_full_set_is_refused(built_lib):
    """all five tables and the ladders' quotient are six oracles; one SHA-256 pair makes eight; a second pair would exceed eight"""
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    cw = 4 << CAP_H
    with tmx.Context(4, b"celestia", max_batch=1) as c:
        tr = _trace_rows(c, 0, 4, 1, 9400)
        d_caps, d_cap_h, d_cap_q = _sentinel(5 * cw), _sentinel(cw), _sentinel(cw)
        c.trace_commit_set_device(0, 1, 1 | 2 | SHA256 | TREE | HEADER, 1, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        c.trace_commit_set_air_device(d_cap_q.data_ptr(), 0)  # the ladders' call coexists
        c.trace_commit_set_air_sha256_device(TREE, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
        shape, order = c.trace_commit_set_shape()
        assert len(order) == 8 and order[order.index(TREE) + 1:order.index(TREE) + 3] == [HELPER, QUOTIENT] and order[order.index(1) + 1] == 64
        assert "room" in _refused(lambda: c.trace_commit_set_air_sha256_device(SHA256, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0), d_cap_h, d_cap_q)


@pytest.mark.gpu
def test_each_validation_rule(ctx):
    """every rule on its own: TMX_ERR_BAD_ARG before anything is enqueued, nothing written"""
    import torch
    log_n, lb = 8, 1
    d_cols, d_hcols = _sentinel(W << log_n), _sentinel(HC << log_n)
    d_cap, d_cap_h, d_quot = _sentinel(4 << CAP_H), _sentinel(4 << CAP_H), _sentinel(2 << log_n)
    ptrs = [d_cols.data_ptr(), d_hcols.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(), d_quot.data_ptr()]
    q = lambda ln, b, n, a=ptrs: (lambda: ctx.air_sha256_quotient_device(ln, b, CAP_H, n, *a, 0))
    for fn in (q(log_n, 0, 1), q(log_n, 7, 1), q(2, 2, 1), q(29, 2, 1), q(6, 1, 1), q(11, 6, 1), q(log_n, lb, 0), q(log_n, lb, (1 << 24) // HC + 1)):
        _refused(fn, d_quot)
    for k in range(5):
        _refused(q(log_n, lb, 1, ptrs[:k] + [None] + ptrs[k + 1:]), d_quot)
    d_table, d_help = _sentinel(W << 7), _sentinel(HC << 7)
    hp = lambda lr, n, t=d_table.data_ptr(), o=d_help.data_ptr(): (lambda: ctx.air_sha256_helper_device(lr, n, t, o, 0))
    for fn in (hp(5, 1), hp(28, 1), hp(7, 0), hp(7, (1 << 24) // HC + 1), hp(7, 1, t=None), hp(7, 1, o=None)):
        _refused(fn, d_help)
    # the verifier: column counts 9 k / 300 k / 2, equal log_n, all three inside the proof
    ok, caps, proof = torch.full((4,), 7, dtype=torch.int32, device=_dev()), _sentinel(256), _sentinel(1 << 16)
    v = lambda p, k: (lambda: ctx.air_sha256_verify_device(p, k, caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0))
    good = bparams([8, 8, 8], [W, HC, 2], CAP_H, lb, 2, 2, 4)
    for p, k in ((good, 1), (dict(good, n_cols=[W + 1, HC, 2]), 0), (dict(good, n_cols=[W, HC + 1, 2]), 0), (dict(good, n_cols=[2 * W, HC, 2]), 0),
                 (dict(good, n_cols=[W, HC, 3]), 0), (dict(good, log_n=[8, 8, 7]), 0), (bparams([6, 6, 6], [W, HC, 2], CAP_H, lb, 2, 2, 4), 0),
                 (dict(good, arity_bits=0), 0), (bparams([8, 8], [W, HC], CAP_H, lb, 2, 2, 4), 0)):
        _refused(v(p, k), ok)
