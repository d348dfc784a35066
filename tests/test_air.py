"""The constraint quotient of the ladder rows (include/tmx.h "the constraint quotient of the ladder rows"): tmx_air_ladder_quotient_device,
tmx_air_ladder_quotient_range_device, tmx_air_last_gamma, tmx_air_verify_device, tmx_trace_commit_set_air_device.  The yardstick is
tests/air_model.py (gamma, the quotient point by point, the identity at zeta) on top of tests/batch_model.py: device words must equal the
model's word for word and every verdict of the device verifier must equal the model verifier's.  The CPU part ties the model itself to the
claim: on the CPU oracle's ladder rows the quotient is a polynomial of degree < N, and one changed cell of a detected kind makes it one of
degree >= N; the kinds the 33 constraints do NOT see are recorded next to them."""
import numpy as np
import pytest

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
from batch_model import bparams
from test_fri import _down, _sentinel, _shift, _up

P = fm.P
BAD_ARG = -1
LADDERS, SHA512, SHA256, TREE, HEADER, QUOTIENT = 1, 2, 4, 16, 32, 64
ALL = LADDERS | SHA512 | SHA256 | TREE | HEADER
W = am.WIDTH


# ---- the CPU oracle's ladder rows
def _ladder_table(oracle, kind, n, n_proofs, seed):
    """the pre-LDE ladder columns of n_proofs synthetic proofs from the CPU oracle: [65 n_proofs][2 n 256] words (row-major rows of 65 in
    the trace block, include/tmx.h "Level-2 trace rows")"""
    from tendermintx_amd.synth import Workload
    wl = Workload(kind, n, n_proofs, n, chain_id=b"celestia", seed=seed, signed_permille=900)
    rows = 2 * n * 256
    cols = np.zeros((n_proofs * W, rows), dtype=np.uint64)
    for p in range(n_proofs):
        t = wl.targets[p * n * 256:(p + 1) * n * 256]
        r = wl.trusteds[p * n * 48:(p + 1) * n * 48] if kind == 0 else None
        full = oracle.trace(kind, wl.proofs[p * 2336:(p + 1) * 2336], t, r, n)
        cols[p * W:(p + 1) * W] = full[:rows * W].reshape(rows, W).T
    return cols


@pytest.fixture(scope="module")
def skip_table(oracle):
    return _ladder_table(oracle, 0, 4, 2, 5100)  # skip, N = 4, two proofs: 130 columns of 2^11 rows


@pytest.fixture(scope="module")
def step_table(oracle):
    return _ladder_table(oracle, 1, 2, 2, 5200)  # step, N = 2, two proofs: 130 columns of 2^10 rows


CAP_H = 2


def _cap(oracle, ext, log_n, cap_height=CAP_H):
    h = min(cap_height, log_n)
    return oracle.poseidon_merkle(np.ascontiguousarray(ext).reshape(-1), log_n, ext.shape[0], h)[-(1 << h):].reshape(-1)


def _model_quotient(oracle, table, log_blowup):
    """(extended columns, cap, gamma, planar quotient) of a pre-LDE table"""
    n_proofs, log_n = table.shape[0] // W, table.shape[1].bit_length() - 1 + log_blowup
    ext = oracle.lde(table, log_blowup)
    cap = _cap(oracle, ext, log_n)
    g = am.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, cap)
    return ext, cap, g, am.quotient(oracle, log_n, log_blowup, n_proofs, ext, _shift(), g)


def _degrees(oracle, quot):
    M = quot.size // 2
    return [am.degree(am.coefficients(oracle, quot[k * M:(k + 1) * M], _shift())) for k in (0, 1)]


def test_rows_satisfy_the_constraints_limb_for_limb(skip_table, step_table):
    """all 33 constraints hold as integer identities on every ladder row of the oracle's tables (no reduction mod p needed: every value is
    below 2^32), the chain on every row but the last of a ladder"""
    for table in (skip_table, step_table):
        assert int(table.max()) < 1 << 32
        t = table.astype(object)
        for p in range(table.shape[0] // W):
            c = t[p * W:(p + 1) * W]
            assert not ((c[am.BIT] * c[am.BIT] - c[am.BIT]) != 0).any()
            for l in range(am.LIMBS):
                assert not ((c[am.NXT + l] - c[am.DBL + l] - c[am.BIT] * (c[am.ADD + l] - c[am.DBL + l])) != 0).any()
                chain = np.roll(c[am.ACC + l], -1) - c[am.NXT + l]
                assert not chain[np.arange(chain.size) % 256 != 255].any()
        assert (table[am.BIT] == 1).any() and (table[am.BIT] == 0).any()


@pytest.mark.parametrize("which", ["skip", "step"])
def test_quotient_is_a_polynomial_of_degree_below_n(oracle, skip_table, step_table, which):
    """the model quotient of the honest tables interpolates to degree < N in both planes (measured: N - 2), and the identity holds at a point
    outside the base field: trace and quotient polynomials evaluated there by Horner on their coefficients"""
    table = skip_table if which == "skip" else step_table
    log_blowup = 2
    N = table.shape[1]
    log_n, n_proofs = N.bit_length() - 1 + log_blowup, table.shape[0] // W
    ext, cap, g, quot = _model_quotient(oracle, table, log_blowup)
    deg = _degrees(oracle, quot)
    print(f"\n[air] {which}: N = {N}, quotient degrees {deg}")
    assert max(deg) < N and g[1] != 0
    M = 1 << log_n
    zeta = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)
    zs = (zeta, fm.e_scale(zeta, oracle.gl_root(log_n - log_blowup)))
    ys = dm.evaluate(oracle, table, 1, zs)  # (inverse NTT on the trace domain, Horner)
    u = [am.horner(am.coefficients(oracle, quot[k * M:(k + 1) * M], _shift()), zeta) for k in (0, 1)]
    t0, t1 = [tuple(y[0]) for y in ys], [tuple(y[1]) for y in ys]
    assert am.identity_at(oracle, log_n, log_blowup, n_proofs, t0, t1, u[0], u[1], zeta, g)
    assert not am.identity_at(oracle, log_n, log_blowup, n_proofs, t0, t1, fm.e_add(u[0], (1, 0)), u[1], zeta, g)
    t0[am.NXT + 3] = fm.e_add(t0[am.NXT + 3], (0, 1))
    assert not am.identity_at(oracle, log_n, log_blowup, n_proofs, t0, t1, u[0], u[1], zeta, g)


def _spots(table):
    """rows of proof 0's table inside a live ladder: one with bit = 0 and one with bit = 1, neither the first nor the last of a ladder"""
    bit = table[am.BIT]
    mid = (np.arange(bit.size) % 256 != 0) & (np.arange(bit.size) % 256 != 255)
    r0, r1 = np.flatnonzero(mid & (bit == 0) & (table[am.DBL] != 0)), np.flatnonzero(mid & (bit == 1))
    return int(r0[len(r0) // 2]), int(r1[len(r1) // 2])


def _changed(table, col, row, value=None):
    bad = table.copy()
    bad[col, row] = np.uint64(int(bad[col, row]) ^ 1) if value is None else np.uint64(value)
    return bad


DETECTED = ["bit -> 2", "nxt limb", "acc limb at r >= 1", "dbl where bit = 0", "add where bit = 1"]
UNDETECTED = ["acc at r = 0", "dbl where bit = 1", "add where bit = 0"]


def _one_cell(table, kind):
    r0, r1 = _spots(table)
    return {"bit -> 2": lambda: _changed(table, am.BIT, r1, 2),
            "nxt limb": lambda: _changed(table, am.NXT + 5, r0),
            "acc limb at r >= 1": lambda: _changed(table, am.ACC + 9, r1),
            "dbl where bit = 0": lambda: _changed(table, am.DBL + 2, r0),
            "add where bit = 1": lambda: _changed(table, am.ADD + 12, r1),
            "acc at r = 0": lambda: _changed(table, am.ACC + 9, 256 * (r1 // 256)),
            "dbl where bit = 1": lambda: _changed(table, am.DBL + 2, r1),
            "add where bit = 0": lambda: _changed(table, am.ADD + 12, r0)}[kind]()


@pytest.mark.parametrize("kind", DETECTED)
def test_one_changed_cell_breaks_the_degree(oracle, step_table, kind):
    """the detected kinds: one changed cell of the first proof's table and the quotient no longer interpolates to degree < N"""
    table = step_table[:W]
    bad = _one_cell(table, kind)
    assert (bad != table).sum() == 1
    deg = _degrees(oracle, _model_quotient(oracle, bad, 2)[3])
    print(f"\n[air] {kind}: quotient degrees {deg}, N = {table.shape[1]}")
    assert max(deg) >= table.shape[1]


@pytest.mark.parametrize("kind", UNDETECTED)
def test_kinds_the_constraints_do_not_see(oracle, step_table, kind):
    """recorded so that nobody mistakes the claim: the accumulator of a ladder's first row (the boundary is not in the set), dbl where the
    bit selects add and add where it selects dbl (the curve arithmetic is not in the set) can change and the quotient stays low-degree"""
    table = step_table[:W]
    bad = _one_cell(table, kind)
    assert (bad != table).sum() == 1
    assert max(_degrees(oracle, _model_quotient(oracle, bad, 2)[3])) < table.shape[1]


def test_model_pieces_add_up(oracle, step_table):
    """the piece form of the model: proofs [0, 1) plus proofs [1, 2) is the whole sum"""
    ext, cap, g, quot = _model_quotient(oracle, step_table, 2)
    parts = [am.quotient(oracle, 12, 2, 2, ext, _shift(), g, proofs=r) for r in (range(0, 1), range(1, 2))]
    assert np.array_equal((parts[0].astype(object) + parts[1].astype(object)) % P, quot.astype(object))
    assert parts[1].any()


def test_symbols_and_wrappers_exist(built_lib):
    """the new entry points are in the built library, bound in _lib.py and wrapped in context.py"""
    from tendermintx_amd import _lib
    from tendermintx_amd.context import Context
    for name in ("tmx_air_ladder_quotient_device", "tmx_air_ladder_quotient_range_device", "tmx_air_last_gamma", "tmx_air_verify_device",
                 "tmx_trace_commit_set_air_device"):
        assert getattr(built_lib, name).argtypes, name
    for name in ("air_ladder_quotient_device", "air_last_gamma", "air_verify_device", "trace_commit_set_air_device"):
        assert callable(getattr(Context, name)), name
    assert _lib.TRACE_LADDERS_QUOTIENT == QUOTIENT


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


def _tree(ctx, d_cols, log_n, n_cols, cap_height=CAP_H):
    """(levels, cap) on the device"""
    h = min(cap_height, log_n)
    d_lv = _sentinel(4 * ctx.poseidon_merkle_digests(log_n, h))
    ctx.poseidon_merkle_device(log_n, n_cols, d_cols.data_ptr(), h, d_lv.data_ptr(), 0)
    return d_lv, d_lv[-(4 << h):]


def _quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_cap, pieces=None, cap_height=CAP_H):
    """the device quotient between two sentinel blocks that must stay untouched; pieces: [(lo, hi)] fed in order, accumulating"""
    import torch
    words = 2 << log_n
    buf = _sentinel(words + 2 * GUARD)
    out = buf[GUARD:].data_ptr()
    if pieces is None:
        ctx.air_ladder_quotient_device(log_n, log_blowup, cap_height, n_proofs, d_cols.data_ptr(), d_cap.data_ptr(), out, 0)
    else:
        for k, r in enumerate(pieces):
            ctx.air_ladder_quotient_device(log_n, log_blowup, cap_height, n_proofs, d_cols.data_ptr(), d_cap.data_ptr(), out, 0, proof_range=r,
                                           accumulate=k > 0)
    torch.cuda.synchronize(_dev())
    want = _sentinel(GUARD)
    assert torch.equal(buf[:GUARD], want) and torch.equal(buf[GUARD + words:], want)
    return buf[GUARD:GUARD + words].clone()


def _random_ext(rng, log_n, n_proofs):
    """random words, non-satisfying and of full degree; a few of them non-canonical (w + p for small w)"""
    ext = rng.integers(0, P, (n_proofs * W, 1 << log_n), dtype=np.uint64)
    ext[0, ::5] = rng.integers(0, 1 << 31, ext[0, ::5].size, dtype=np.uint64) + np.uint64(P)
    ext[W - 1, 1::7] = np.uint64(P)
    return ext


# (log2 of the trace rows, proofs, log_blowup): 2^8 .. 2^11 rows, 1 .. 40 proofs, blow-up 4 and 8
RANDOM_SHAPES = [(8, 40, 2), (8, 1, 3), (9, 7, 3), (10, 3, 2), (11, 1, 3), (11, 2, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs,log_blowup", RANDOM_SHAPES)
def test_quotient_of_random_columns_equals_the_model(ctx, oracle, log_rows, n_proofs, log_blowup):
    """the definition is pointwise: on random (non-satisfying) columns d_quot and gamma equal the model word for word, guard words intact,
    whole and fed in two pieces"""
    log_n = log_rows + log_blowup
    ext = _random_ext(np.random.default_rng(6100 + log_n * 41 + n_proofs), log_n, n_proofs)
    d_cols = _up(ext)
    _, d_cap = _tree(ctx, d_cols, log_n, n_proofs * W)
    got = _down(_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_cap))
    g = am.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _down(d_cap))
    assert ctx.air_last_gamma() == g
    want = am.quotient(oracle, log_n, log_blowup, n_proofs, ext, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    cut = max(1, n_proofs // 3)
    pieces = [(0, cut), (cut, n_proofs)] if n_proofs > 1 else [(0, 1)]
    again = _down(_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_cap, pieces=pieces))
    assert np.array_equal(again, want), np.flatnonzero(again != want)[:10]
    if n_proofs > 1:  # one piece alone is the model's piece
        part = _down(_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_cap, pieces=[(cut, n_proofs)]))
        assert np.array_equal(part, am.quotient(oracle, log_n, log_blowup, n_proofs, ext, _shift(), g, proofs=range(cut, n_proofs)))


@pytest.mark.gpu
@pytest.mark.parametrize("which,log_blowup", [("step", 2), ("skip", 3)])
def test_quotient_of_real_ladders_equals_the_model(ctx, oracle, skip_table, step_table, which, log_blowup):
    """real ladders at 2^10 (step, N = 2) and 2^11 (skip, N = 4) rows, extended on the device: d_quot and gamma equal the model's, whole
    and in two pieces, and the quotient interpolates to degree < N"""
    import torch
    table = skip_table if which == "skip" else step_table
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    log_n = log_rows + log_blowup
    d_ext = _sentinel(table.shape[0] << log_n)
    ctx.lde_device(log_rows, log_blowup, table.shape[0], _up(table).data_ptr(), d_ext.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    ext = oracle.lde(table, log_blowup)
    assert np.array_equal(_down(d_ext).reshape(ext.shape), ext)
    _, d_cap = _tree(ctx, d_ext, log_n, n_proofs * W)
    got = _down(_quotient(ctx, log_n, log_blowup, n_proofs, d_ext, d_cap))
    g = am.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _down(d_cap))
    assert ctx.air_last_gamma() == g
    want = am.quotient(oracle, log_n, log_blowup, n_proofs, ext, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    again = _down(_quotient(ctx, log_n, log_blowup, n_proofs, d_ext, d_cap, pieces=[(0, 1), (1, 2)]))
    assert np.array_equal(again, want)
    assert max(_degrees(oracle, got)) < table.shape[1]


E2E = dict(log_blowup=2, arity_bits=2, final_log_max=2, n_queries=6)


def _e2e(ctx, oracle, table, quot_override=None):
    """caller-level chain: LDE, trees, quotient, one batch proof over [trace, quotient].  Returns (params, d_caps, device proof words,
    extended columns, quotient words)"""
    import torch
    log_blowup = E2E["log_blowup"]
    n_cols, log_rows = table.shape[0], table.shape[1].bit_length() - 1
    log_n, n_proofs = log_rows + log_blowup, table.shape[0] // W
    d_ext = _sentinel(n_cols << log_n)
    ctx.lde_device(log_rows, log_blowup, n_cols, _up(table).data_ptr(), d_ext.data_ptr(), 0)
    d_lv_t, d_cap_t = _tree(ctx, d_ext, log_n, n_cols)
    if quot_override is None:
        d_quot = _quotient(ctx, log_n, log_blowup, n_proofs, d_ext, d_cap_t)
    else:
        d_quot = _up(quot_override)
    d_lv_q, d_cap_q = _tree(ctx, d_quot, log_n, 2)
    p = bparams([log_n, log_n], [n_cols, 2], CAP_H, log_blowup, E2E["arity_bits"], E2E["final_log_max"], E2E["n_queries"])
    words = bm.layout(p)["words"]
    buf = _sentinel(words + 2 * GUARD)
    ctx.batch_prove_device(p, [d_ext.data_ptr(), d_quot.data_ptr()], [d_lv_t.data_ptr(), d_lv_q.data_ptr()], buf[GUARD:].data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(buf[:GUARD], _sentinel(GUARD)) and torch.equal(buf[GUARD + words:], _sentinel(GUARD))
    return p, torch.cat([d_cap_t, d_cap_q]), _down(buf[GUARD:GUARD + words].clone()), _down(d_ext).reshape(n_cols, -1), _down(d_quot)


def _verdicts(ctx, p, k_trace, d_caps, proof, batch_only=False):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    if batch_only:
        ctx.batch_verify_device(p, d_caps.data_ptr(), _up(proof).data_ptr(), ok.data_ptr(), 0)
    else:
        ctx.air_verify_device(p, k_trace, d_caps.data_ptr(), _up(proof).data_ptr(), ok.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    out = ok.cpu().numpy()
    assert ((out == 0) | (out == 1)).all(), out
    return [bool(x) for x in out]


@pytest.mark.gpu
def test_caller_level_end_to_end(ctx, oracle, step_table):
    """LDE, trees, quotient, batch prove over [trace, quotient]: the proof equals batch_model.prove on the model's quotient word for word,
    tmx_air_verify_device accepts every query and so does the model; a bumped trace opening or quotient opening is rejected by every query"""
    p, d_caps, got, ext, quot = _e2e(ctx, oracle, step_table)
    log_n, n_proofs = p["log_n"][0], step_table.shape[0] // W
    caps = _down(d_caps)
    g = am.gamma(oracle, log_n, p["log_blowup"], CAP_H, n_proofs, caps[:4 << CAP_H])
    want_q = am.quotient(oracle, log_n, p["log_blowup"], n_proofs, ext, _shift(), g)
    assert np.array_equal(quot, want_q)
    want, deg, zeta, _ = bm.prove(oracle, p, [ext, want_q.reshape(2, -1)], _shift())
    assert deg and ctx.fri_last_degree_ok() is True and ctx.deep_last_zeta() == zeta
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert am.identity(oracle, p, 0, caps, got)
    assert all(am.verify(oracle, p, 0, caps, got, _shift()))
    assert all(_verdicts(ctx, p, 0, d_caps, got))
    L = bm.layout(p)
    R = 1 << dm.log_r(p["n_cols"][0])
    for name, at in (("trace opening at zeta", L["off_open"][0] + am.NXT + 2), ("trace opening at zeta omega", L["off_open"][0] + 2 * R + W + am.ACC),
                     ("quotient opening", L["off_open"][1] + 1)):
        bad = got.copy()
        bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
        assert not am.identity(oracle, p, 0, caps, bad), name
        model = am.verify(oracle, p, 0, caps, bad, _shift())
        assert not any(model), name
        assert _verdicts(ctx, p, 0, d_caps, bad) == model, name


@pytest.mark.gpu
def test_tampered_trace_proved_honestly(ctx, oracle, step_table):
    """a tampered trace (bit -> 2 in one cell) with its honest quotient: the quotient has degree >= N, so the degree flag is 0 and not all
    queries are accepted; the verdicts are the model's query by query"""
    bad = step_table.copy()
    bad[:W] = _one_cell(step_table[:W], "bit -> 2")
    p, d_caps, got, ext, quot = _e2e(ctx, oracle, bad)
    assert ctx.fri_last_degree_ok() is False
    caps = _down(d_caps)
    n_proofs = bad.shape[0] // W
    g = am.gamma(oracle, p["log_n"][0], p["log_blowup"], CAP_H, n_proofs, caps[:4 << CAP_H])
    want_q = am.quotient(oracle, p["log_n"][0], p["log_blowup"], n_proofs, ext, _shift(), g)
    assert np.array_equal(quot, want_q) and max(_degrees(oracle, quot)) >= bad.shape[1]
    want, deg, _, _ = bm.prove(oracle, p, [ext, want_q.reshape(2, -1)], _shift())
    assert deg is False and np.array_equal(got, want)
    model = am.verify(oracle, p, 0, caps, got, _shift())
    device = _verdicts(ctx, p, 0, d_caps, got)
    print(f"\n[air] tampered trace, honest quotient: device verdicts {device}")
    assert device == model and not all(device)


@pytest.mark.gpu
def test_zero_quotient_for_a_tampered_trace(ctx, oracle, step_table):
    """a zero (low-degree) quotient committed for a tampered trace: the batch proof is fine -- tmx_batch_verify_device accepts every query --
    and the identity fails: tmx_air_verify_device rejects every one, as the model does"""
    bad = step_table.copy()
    bad[:W] = _one_cell(step_table[:W], "nxt limb")
    log_n = bad.shape[1].bit_length() - 1 + E2E["log_blowup"]
    p, d_caps, got, ext, quot = _e2e(ctx, oracle, bad, quot_override=np.zeros(2 << log_n, dtype=np.uint64))
    assert ctx.fri_last_degree_ok() is True
    caps = _down(d_caps)
    assert all(_verdicts(ctx, p, 0, d_caps, got, batch_only=True)) and all(bm.verify(oracle, p, caps, got, _shift()))
    assert not am.identity(oracle, p, 0, caps, got)
    model = am.verify(oracle, p, 0, caps, got, _shift())
    device = _verdicts(ctx, p, 0, d_caps, got)
    assert device == model and not any(device)


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
def test_each_validation_rule(ctx):
    """every rule on its own: TMX_ERR_BAD_ARG before anything is enqueued, nothing written"""
    import torch
    log_n, lb, n_proofs = 10, 2, 1
    d_cols = _sentinel((n_proofs * W) << log_n)
    d_cap, d_quot = _sentinel(4 << CAP_H), _sentinel(2 << log_n)
    ptrs = (d_cols.data_ptr(), d_cap.data_ptr(), d_quot.data_ptr(), 0)
    q = lambda ln, b, n, **kw: (lambda: ctx.air_ladder_quotient_device(ln, b, CAP_H, n, *ptrs, **kw))
    for fn in (q(log_n, 0, 1), q(log_n, 7, 1), q(2, 2, 1), q(29, 2, 1), q(9, 2, 1), q(13, 6, 1), q(log_n, lb, 0), q(log_n, lb, (1 << 24) // W + 1),
               q(log_n, lb, 1, proof_range=(0, 0)), q(log_n, lb, 1, proof_range=(1, 1)), q(log_n, lb, 1, proof_range=(0, 2)),
               q(log_n, lb, 1, proof_range=(0, 1), accumulate=2)):
        _refused(fn, d_quot)
    assert "d_cols" in _refused(lambda: ctx.air_ladder_quotient_device(log_n, lb, CAP_H, 1, None, d_cap.data_ptr(), d_quot.data_ptr(), 0), d_quot)
    # the verifier: oracle k_trace a multiple of 65 columns, oracle k_trace + 1 the same log_n and 2 columns, both inside the proof
    ok, caps, proof = torch.full((4,), 7, dtype=torch.int32, device=_dev()), _sentinel(64), _sentinel(1 << 16)
    v = lambda p, k: (lambda: ctx.air_verify_device(p, k, caps.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0))
    good = bparams([10, 10], [W, 2], CAP_H, lb, 2, 2, 4)
    for p, k in ((good, 1), (dict(good, n_cols=[W + 1, 2]), 0), (dict(good, n_cols=[W, 3]), 0), (dict(good, log_n=[10, 9]), 0),
                 (bparams([9, 9], [W, 2], CAP_H, lb, 2, 2, 4), 0), (dict(good, arity_bits=0), 0), (bparams([10], [W], CAP_H, lb, 2, 2, 4), 0)):
        _refused(v(p, k), ok)


def _set_case(built_lib, oracle, kind, n, n_proofs, sections, streamed, chunk, log_blowup=3, model=False, queries=6):
    """set, (prove), air, shape, prove, verify on one context; returns everything comparable: (caps, cap_q, proof before, proof after,
    params after)"""
    import torch
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    with tmx.Context(n, b"celestia", max_batch=n_proofs) as c:
        tr = _trace_rows(c, kind, n, n_proofs, 7300 + n + n_proofs)
        n_tab = bin(sections).count("1")
        d_caps = _sentinel(n_tab * (4 << CAP_H))
        commit = lambda: (c.trace_commit_set_device(kind, n_proofs, sections, log_blowup, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0) if streamed is None
                          else c.trace_commit_set_streamed_device(kind, n_proofs, sections, streamed, chunk, log_blowup, CAP_H, tr.data_ptr(),
                                                                  d_caps.data_ptr(), 0))
        commit()
        shape0, order0 = c.trace_commit_set_shape()
        p0 = dict(shape0, arity_bits=2, final_log_max=2, n_queries=queries, pow_bits=0)
        before = _sentinel(bm.layout(p0)["words"])
        c.trace_commit_set_prove_device(p0, before.data_ptr(), 0)
        d_cap_q = _sentinel(4 << CAP_H)
        c.trace_commit_set_air_device(d_cap_q.data_ptr(), 0)
        gamma = c.air_last_gamma()
        shape, order = c.trace_commit_set_shape()
        kt = order.index(LADDERS)
        assert order == order0[:kt + 1] + [QUOTIENT] + order0[kt + 1:]
        assert shape["log_n"] == shape0["log_n"][:kt + 1] + [shape0["log_n"][kt]] + shape0["log_n"][kt + 1:]
        assert shape["n_cols"] == shape0["n_cols"][:kt + 1] + [2] + shape0["n_cols"][kt + 1:] and shape["n_cols"][kt] == W * n_proofs
        _refused(lambda: c.trace_commit_set_air_device(d_cap_q.data_ptr(), 0), d_cap_q)  # a second call on the same set
        p = dict(shape, arity_bits=2, final_log_max=2, n_queries=queries, pow_bits=0)
        words = bm.layout(p)["words"]
        buf = _sentinel(words + 2 * GUARD)
        c.trace_commit_set_prove_device(p, buf[GUARD:].data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        assert torch.equal(buf[:GUARD], _sentinel(GUARD)) and torch.equal(buf[GUARD + words:], _sentinel(GUARD))
        after = buf[GUARD:GUARD + words].clone()
        assert c.fri_last_degree_ok() is True
        cw = 4 << CAP_H
        all_caps = torch.cat([d_caps[:(kt + 1) * cw], d_cap_q, d_caps[(kt + 1) * cw:]])
        assert all(_verdicts(c, p, kt, all_caps, _down(after)))
        caps_h, got = _down(all_caps), _down(after)
        assert gamma == am.gamma(oracle, p["log_n"][kt], log_blowup, CAP_H, n_proofs, caps_h[kt * cw:(kt + 1) * cw])
        assert am.identity(oracle, p, kt, caps_h, got)
        # a fresh set without the air call proves what the set proved before the call: nothing existing changed
        commit()
        assert c.trace_commit_set_shape() == (shape0, order0)
        fresh = _sentinel(bm.layout(p0)["words"])
        c.trace_commit_set_prove_device(p0, fresh.data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        assert torch.equal(fresh, before)
        if model:
            from test_merkle_open import _oracle_ext
            traces = _down(tr)
            ext = []
            for k, sec in enumerate(order):
                if sec == QUOTIENT:
                    ext.append(am.quotient(oracle, p["log_n"][kt], log_blowup, n_proofs, ext[kt], _shift(), gamma).reshape(2, -1))
                    continue
                e, lm, nc = _oracle_ext(oracle, kind, n, traces, sec, log_blowup)
                assert (lm, nc) == (p["log_n"][k], p["n_cols"][k])
                ext.append(e.reshape(nc, -1))
            want, deg, _, _ = bm.prove(oracle, p, ext, _shift())
            assert deg and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
            want0, _, _, _ = bm.prove(oracle, p0, [e for e, sec in zip(ext, order) if sec != QUOTIENT], _shift())
            assert np.array_equal(_down(before), want0)
            assert all(am.verify(oracle, p, kt, caps_h, got, _shift()))
        return _down(d_caps), _down(d_cap_q), _down(before), got, p


@pytest.mark.gpu
def test_set_of_the_ladders_alone_equals_the_model(built_lib, oracle):
    """a set of LADDERS alone (step, N = 2, two proofs): set, air, shape, prove, verify; the proof before the air call and the proof of the
    enlarged set equal batch_model.prove (the latter on the model's quotient); the model verifier and the identity accept"""
    caps, cap_q, before, after, p = _set_case(built_lib, oracle, 1, 2, 2, LADDERS, None, 0, log_blowup=2, model=True)
    assert p["log_n"] == [12, 12] and p["n_cols"] == [2 * W, 2]


@pytest.mark.gpu
def test_set_of_all_five_tables_resident_and_streamed(built_lib, oracle):
    """all five tables (skip, N = 4, nine proofs: 585 ladder columns), the ladders resident and streamed in chunks of 72 (one proof per
    chunk), 136 (two) and 520 (eight, then one) columns: caps, quotient cap and both proofs equal word for word; tmx_air_verify_device and
    the model's identity accept (inside _set_case); a prove before the air call is what a set without the call proves"""
    want = _set_case(built_lib, oracle, 0, 4, 9, ALL, None, 0)
    assert want[4]["n_cols"][want[4]["log_n"].index(14)] == 9 * W
    for chunk in (72, 136, 520):
        got = _set_case(built_lib, oracle, 0, 4, 9, ALL, LADDERS, chunk)
        for a, b, name in zip(got[:4], want[:4], ("caps", "quotient cap", "proof before", "proof after")):
            assert np.array_equal(a, b), (chunk, name, np.flatnonzero(a != b)[:10])
        assert got[4] == want[4]
    alone = _set_case(built_lib, oracle, 0, 4, 9, LADDERS, LADDERS, 136)
    assert np.array_equal(alone[1], want[1])  # (gamma and the quotient depend on the ladders alone)


@pytest.mark.gpu
def test_set_level_refusals(built_lib):
    """no set; a set without the ladders; a streamed ladders member with chunk_cols < 65: TMX_ERR_BAD_ARG, nothing written, the set intact"""
    import torch
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    with tmx.Context(4, b"celestia", max_batch=2) as c:
        d_cap_q = _sentinel(4 << CAP_H)
        assert "no commit set" in _refused(lambda: c.trace_commit_set_air_device(d_cap_q.data_ptr(), 0), d_cap_q)
        tr = _trace_rows(c, 0, 4, 2, 7400)
        caps = _sentinel(5 * (4 << CAP_H))
        c.trace_commit_set_device(0, 2, SHA512 | TREE, 3, CAP_H, tr.data_ptr(), caps.data_ptr(), 0)
        assert "LADDERS" in _refused(lambda: c.trace_commit_set_air_device(d_cap_q.data_ptr(), 0), d_cap_q)
        c.trace_commit_set_streamed_device(0, 2, ALL, LADDERS, 64, 3, CAP_H, tr.data_ptr(), caps.data_ptr(), 0)
        assert "chunk_cols" in _refused(lambda: c.trace_commit_set_air_device(d_cap_q.data_ptr(), 0), d_cap_q)
        shape, order = c.trace_commit_set_shape()
        assert QUOTIENT not in order and len(order) == 5
        assert "d_cap_q" in _refused(lambda: c.trace_commit_set_air_device(None, 0))


# ---- GPU, full size: 256 proofs at N = 128, the ladders streamed (tests/test_commit_streamed.py's fixture and memory rule)
from test_commit_streamed import FULL, FULL_CHUNK, FULL_ORDER, full  # noqa: E402,F401


@pytest.mark.gpu
def test_full_size_five_tables_with_the_quotient(full, oracle):
    """256 proofs x N = 128, blow-up 8: all five tables with the ladders (16 640 columns of 2^19 extended rows) streamed in chunks of 512
    columns (7 proofs per chunk), the quotient, one proof over the six oracles, the device verifier, the model's verifier and the identity.
    The memory rule is test_commit_streamed's: the streamed set must fit the card's free memory"""
    import torch
    from tendermintx_amd.context import trace_commit_set_bytes as nbytes
    ctx, tr = full
    need = nbytes(0, FULL["n"], FULL["proofs"], ALL, LADDERS, FULL_CHUNK, FULL["log_blowup"], FULL["cap_height"]) + (2 << 19) * 8 * 3
    torch.cuda.empty_cache()
    free_b, total_b = torch.cuda.mem_get_info(_dev())
    print(f"\n[air] full size: streamed set + quotient {need / 2**30:.1f} GiB, free {free_b / 2**30:.1f} of {total_b / 2**30:.1f} GiB", flush=True)
    assert 0 < need < free_b, (need, free_b)
    cw = 4 << FULL["cap_height"]
    d_caps = _sentinel(5 * cw)
    ctx.trace_commit_set_streamed_device(0, FULL["proofs"], ALL, LADDERS, FULL_CHUNK, FULL["log_blowup"], FULL["cap_height"], tr.data_ptr(),
                                         d_caps.data_ptr(), 0)
    d_cap_q = _sentinel(cw)
    ctx.trace_commit_set_air_device(d_cap_q.data_ptr(), 0)
    gamma = ctx.air_last_gamma()
    shape, order = ctx.trace_commit_set_shape()
    assert order == [LADDERS, QUOTIENT] + FULL_ORDER[1:] and shape["log_n"] == [19, 19, 18, 18, 17, 15]
    assert shape["n_cols"] == [16640, 2, 4608, 2304, 2304, 2304]
    p = dict(shape, arity_bits=FULL["arity_bits"], final_log_max=FULL["final_log_max"], n_queries=FULL["n_queries"], pow_bits=0)
    d_proof = _sentinel(bm.layout(p)["words"])
    ctx.trace_commit_set_prove_device(p, d_proof.data_ptr(), 0)
    assert ctx.fri_last_degree_ok() is True
    all_caps = torch.cat([d_caps[:cw], d_cap_q, d_caps[cw:]])
    got, caps = _down(d_proof), _down(all_caps)
    assert all(_verdicts(ctx, p, 0, all_caps, got))
    assert gamma == am.gamma(oracle, 19, FULL["log_blowup"], FULL["cap_height"], FULL["proofs"], caps[:cw])
    assert am.identity(oracle, p, 0, caps, got)
    assert all(bm.verify(oracle, p, caps, got, _shift()))
    bad = got.copy()
    at = bm.layout(p)["off_open"][1]
    bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
    assert not any(_verdicts(ctx, p, 0, all_caps, bad)) and not am.identity(oracle, p, 0, caps, bad)
