"""Constraint set 2 of the ladder rows (include/tmx.h "the boundary constraints of the ladder rows"): tmx_air_ladder_public_shape,
tmx_air_ladder_public_device, tmx_air_ladder_boundary_quotient_device / _range_device, tmx_air_boundary_verify_device,
tmx_trace_commit_set_air_boundary_device.  The yardstick is tests/air_boundary_model.py on top of air_model.py and batch_model.py: device
words must equal the model's word for word (everything is exact field arithmetic: no tolerance anywhere).  The CPU part ties the model to
the claim on the CPU oracle's rows: the public table built from the ELEMENT rows (Level 1, D.1b) is what the ladders end in, the quotient is
a polynomial of degree < N, and a changed first accumulator, a consistent change on a ladder's last row, a changed public word or a flipped
live flag -- none of which set 1 sees -- makes it one of degree >= N.  What set 2 still does not see is recorded next to that."""
import numpy as np
import pytest

import air_boundary_model as abm
import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import test_air as ta
from batch_model import bparams
from test_fri import _down, _sentinel, _shift, _up

P = fm.P
BAD_ARG = -1
LADDERS, SHA512, SHA256, TREE, HEADER, QUOTIENT = 1, 2, 4, 16, 32, 64
ALL = LADDERS | SHA512 | SHA256 | TREE | HEADER
W, PW = am.WIDTH, abm.PUB_WIDTH
CAP_H = ta.CAP_H
CID, SKIP_MAX = b"celestia", 100800


# ---- the CPU oracle's ladder rows and element rows
def _tables(oracle, kind, n, n_proofs, seed, permille=900):
    """(pre-LDE ladder columns [65 n_proofs][2^log_rows], zero rows behind a proof's own; the public table from the oracle's ELEMENT rows)"""
    from tendermintx_amd.synth import Workload
    wl = Workload(kind, n, n_proofs, n, chain_id=CID, seed=seed, signed_permille=permille)
    rows = 2 * n * 256
    log_rows = (rows - 1).bit_length()
    cols, elems = np.zeros((n_proofs * W, 1 << log_rows), dtype=np.uint64), []
    for p in range(n_proofs):
        t = wl.targets[p * n * 256:(p + 1) * n * 256]
        r = wl.trusteds[p * n * 48:(p + 1) * n * 48] if kind == 0 else None
        pr = wl.proofs[p * 2336:(p + 1) * 2336]
        full = oracle.trace(kind, pr, t, r, n)
        cols[p * W:(p + 1) * W, :rows] = full[:rows * W].reshape(rows, W).T
        elems.append(oracle.witness(kind, pr, t, r, CID, SKIP_MAX)[0])
    return cols, abm.public_table(kind, n, elems, log_rows - 8)


@pytest.fixture(scope="module")
def skip4(oracle):
    return _tables(oracle, 0, 4, 2, 5100)  # skip, N = 4, two proofs: 2^11 rows, K = 8


@pytest.fixture(scope="module")
def step2(oracle):
    return _tables(oracle, 1, 2, 2, 5200)  # step, N = 2, two proofs: 2^10 rows, K = 4


@pytest.fixture(scope="module")
def step3(oracle):
    return _tables(oracle, 1, 3, 2, 5300, permille=500)  # step, N = 3: 1536 rows in 2^11, K = 8 with two all-zero padding ladders


def _pick(request, which):
    return request.getfixturevalue({"skip": "skip4", "step": "step2", "step3": "step3"}[which])


def _model_quotient(oracle, table, pub, log_blowup, parts=False):
    """(extended columns, cap, gamma, planar quotient) of a pre-LDE table and a public table"""
    n_proofs, log_n = table.shape[0] // W, table.shape[1].bit_length() - 1 + log_blowup
    ext = oracle.lde(table, log_blowup)
    cap = ta._cap(oracle, ext, log_n)
    g = abm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, cap, pub)
    return ext, cap, g, abm.quotient(oracle, log_n, log_blowup, n_proofs, ext, pub, _shift(), g, parts=parts)


def _deg2(oracle, table, pub):
    return max(ta._degrees(oracle, _model_quotient(oracle, table, pub, 2)[3]))


def _deg1(oracle, table):
    return max(ta._degrees(oracle, ta._model_quotient(oracle, table, 2)[3]))


@pytest.mark.parametrize("which", ["skip", "step", "step3"])
def test_public_table_is_where_the_ladders_end(request, which):
    """the Level-1 tie: the table built from the element rows (D.1b: sB, hA per lane), not from the trace, holds for every proof and ladder
    the trace's nxt at row 255 word for word, and live is acc_0.y limb 0; padding ladders are zero in both"""
    table, pub = _pick(request, which)
    K = table.shape[1] // 256
    assert pub.shape == (PW * (table.shape[0] // W), K)
    lives = 0
    for p in range(table.shape[0] // W):
        for k in range(K):
            for l in range(am.LIMBS):
                assert pub[PW * p + l, k] == table[p * W + am.NXT + l, 256 * k + 255], (p, k, l)
            live = int(pub[PW * p + 16, k])
            assert live == int(pub[PW * p:PW * p + 16, k].any())
            assert [int(table[p * W + am.ACC + l, 256 * k]) for l in range(am.LIMBS)] == [0] * 8 + [live] + [0] * 7, (p, k)
            lives += live
            if not live:
                assert not table[p * W:(p + 1) * W, 256 * k:256 * k + 256].any()
    assert lives >= K // 2
    if which == "step3":
        assert not pub[:, 6:].any() and pub[16, :6].all()


@pytest.mark.parametrize("which", ["skip", "step", "step3"])
def test_quotient_is_a_polynomial_of_degree_below_n(request, oracle, which):
    """both planes of the model quotient interpolate to degree < N (the boundary part alone too), and the identity holds at a zeta outside
    the base field: trace and quotient polynomials evaluated there by Horner on their coefficients"""
    table, pub = _pick(request, which)
    log_blowup, N = 2, table.shape[1]
    log_n, n_proofs = N.bit_length() - 1 + log_blowup, table.shape[0] // W
    ext, cap, g, (qm, qb) = _model_quotient(oracle, table, pub, log_blowup, parts=True)
    quot = ((qm.astype(object) + qb.astype(object)) % P).astype(np.uint64)
    assert np.array_equal(quot, abm.quotient(oracle, log_n, log_blowup, n_proofs, ext, pub, _shift(), g))
    deg, deg_b = ta._degrees(oracle, quot), ta._degrees(oracle, qb)
    print(f"\n[air2] {which}: N = {N}, K = {N // 256}, quotient degrees {deg}, boundary part {deg_b}")
    assert max(deg) < N and max(deg_b) < N and g[1] != 0
    assert g != am.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, cap)
    M = 1 << log_n
    zeta = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321 % P)
    zs = (zeta, fm.e_scale(zeta, oracle.gl_root(log_n - log_blowup)))
    ys = dm.evaluate(oracle, table, 1, zs)
    u = [am.horner(am.coefficients(oracle, quot[k * M:(k + 1) * M], _shift()), zeta) for k in (0, 1)]
    t0, t1 = [tuple(y[0]) for y in ys], [tuple(y[1]) for y in ys]
    args = (oracle, log_n, log_blowup, n_proofs)
    assert abm.identity_at(*args, t0, t1, u[0], u[1], zeta, g, pub)
    assert not abm.identity_at(*args, t0, t1, fm.e_add(u[0], (1, 0)), u[1], zeta, g, pub)
    bad = pub.copy()
    bad[3, 1] ^= np.uint64(1)
    assert not abm.identity_at(*args, t0, t1, u[0], u[1], zeta, g, bad)
    # Pub_gamma by the barycentric formula is the interpolant the quotient used: compare at zeta with Horner on its coefficients
    V = abm.combine(pub, g)
    c = abm.pub_coefficients(oracle, log_n, log_blowup, V)
    hz = fm.e_add(am.horner(c[0], zeta), fm.e_mul((0, 1), am.horner(c[1], zeta)))
    assert abm.pub_at(oracle, log_n, log_blowup, V, zeta) == hz
    y = abm.y_points(oracle, log_n, log_blowup, len(V))
    for k in (0, len(V) - 1):
        assert (am.horner(c[0], (y[k], 0))[0], am.horner(c[1], (y[k], 0))[0]) == V[k]


def _last_row(table, bit):
    """(proof, row): a row 255 of a live ladder with that bit"""
    for p in range(table.shape[0] // W):
        for k in range(table.shape[1] // 256):
            r = 256 * k + 255
            if int(table[p * W + am.BIT, r]) == bit and table[p * W + am.NXT:p * W + am.NXT + 16, r].any():
                return p, r
    raise AssertionError(f"no live ladder ends on bit {bit}")


def _tamper(table, pub, kind):
    """(table, pub) with one change of that kind"""
    table, pub = table.copy(), pub.copy()
    if kind == "acc at r = 0":
        return ta._one_cell(table[:W], kind) if table.shape[0] == W else np.concatenate([ta._one_cell(table[:W], kind), table[W:]]), pub
    if kind in ("dbl and nxt at row 255 where bit = 0", "add and nxt at row 255 where bit = 1"):
        p, r = _last_row(table, 0 if kind.startswith("dbl") else 1)
        src = am.DBL if kind.startswith("dbl") else am.ADD
        v = np.uint64(int(table[p * W + src + 4, r]) ^ 1)
        table[p * W + src + 4, r] = v
        table[p * W + am.NXT + 4, r] = v
        return table, pub
    if kind == "one end word of pub":
        pub[PW + 11, 2] ^= np.uint64(1)
        return table, pub
    assert kind == "one flipped live"
    pub[16, 1] ^= np.uint64(1)
    return table, pub


ROW_KINDS = ["acc at r = 0", "dbl and nxt at row 255 where bit = 0", "add and nxt at row 255 where bit = 1"]
PUB_KINDS = ["one end word of pub", "one flipped live"]


@pytest.mark.parametrize("kind", ROW_KINDS + PUB_KINDS)
def test_one_change_breaks_the_degree(oracle, step2, kind):
    """each of these alone: the set-2 quotient no longer interpolates to degree < N.  The three row kinds leave set 1's quotient low-degree
    (air_model, the same table): that difference is what set 2 adds"""
    table, pub = step2
    bad_t, bad_p = _tamper(table, pub, kind)
    assert (bad_t != table).sum() == (0 if kind in PUB_KINDS else 1 if kind == "acc at r = 0" else 2) and (bad_p != pub).sum() == (kind in PUB_KINDS)
    N = table.shape[1]
    if kind in ROW_KINDS:
        for p in range(bad_t.shape[0] // W):  # the change is consistent: set 1's row constraints still hold limb for limb
            c = bad_t[p * W:(p + 1) * W].astype(object)
            for l in range(am.LIMBS):
                assert not ((c[am.NXT + l] - c[am.DBL + l] - c[am.BIT] * (c[am.ADD + l] - c[am.DBL + l])) != 0).any()
        assert _deg1(oracle, bad_t) < N
    deg = _deg2(oracle, bad_t, bad_p)
    print(f"\n[air2] {kind}: set-2 quotient degree {deg}, N = {N}")
    assert deg >= N


@pytest.mark.parametrize("kind", ["dbl where bit = 1", "add where bit = 0"])
def test_kinds_set_2_still_does_not_see(oracle, step2, kind):
    """recorded so that nobody mistakes the claim: mid-ladder, dbl where the bit selects add and add where it selects dbl can change and the
    set-2 quotient stays low-degree -- the curve arithmetic is in neither set"""
    table, pub = step2
    bad = np.concatenate([ta._one_cell(table[:W], kind), table[W:]])
    assert (bad != table).sum() == 1
    assert _deg2(oracle, bad, pub) < table.shape[1]


def test_zeroed_ladder(oracle, step2):
    """a ladder zeroed by hand with live = 0 and a zero end point satisfies set 2; the same rows with live = 1 do not"""
    table, pub = step2
    table, pub = table.copy(), pub.copy()
    table[:W, 256:512] = 0
    pub[:PW, 1] = 0
    assert _deg2(oracle, table, pub) < table.shape[1]
    pub[16, 1] = 1
    assert _deg2(oracle, table, pub) >= table.shape[1]


def test_model_pieces_add_up(oracle, step2):
    """proofs [0, 1) plus proofs [1, 2) is the whole sum, and the public term sits in the piece with proof 0 only: the other piece is the
    same whatever the table says"""
    table, pub = step2
    ext, cap, g, quot = _model_quotient(oracle, table, pub, 2)
    parts = [abm.quotient(oracle, 12, 2, 2, ext, pub, _shift(), g, proofs=r) for r in (range(0, 1), range(1, 2))]
    assert np.array_equal((parts[0].astype(object) + parts[1].astype(object)) % P, quot.astype(object))
    other = np.zeros_like(pub)
    assert np.array_equal(abm.quotient(oracle, 12, 2, 2, ext, other, _shift(), g, proofs=range(1, 2)), parts[1])
    assert not np.array_equal(abm.quotient(oracle, 12, 2, 2, ext, other, _shift(), g, proofs=range(0, 1)), parts[0])


def test_symbols_and_wrappers_exist(built_lib):
    """the new entry points are in the built library (hipcc --offload-arch=gfx950), bound in _lib.py and wrapped in context.py"""
    from tendermintx_amd import context
    from tendermintx_amd.context import Context
    for name in ("tmx_air_ladder_public_shape", "tmx_air_ladder_public_device", "tmx_air_ladder_boundary_quotient_device",
                 "tmx_air_ladder_boundary_quotient_range_device", "tmx_air_boundary_verify_device", "tmx_trace_commit_set_air_boundary_device"):
        assert getattr(built_lib, name).argtypes, name
    for name in ("air_ladder_public_shape", "air_ladder_public_device", "air_ladder_boundary_quotient_device", "air_boundary_verify_device",
                 "trace_commit_set_air_boundary_device"):
        assert callable(getattr(Context, name)), name
    assert context.air_ladder_public_shape(0, 4, 2) == (3, 34) and context.air_ladder_public_shape(1, 3, 1) == (3, 17)
    assert context.air_ladder_public_shape(1, 2, 5) == (2, 85) and context.air_ladder_public_shape(0, 128, 256) == (8, 4352)
    from tendermintx_amd._lib import TmxError
    for args in ((0, 4, 0), (2, 4, 1)):
        with pytest.raises(TmxError):
            context.air_ladder_public_shape(*args)
    for kind, n in ((0, 4), (1, 3), (0, 128)):  # the model's D.1b offset is the library's
        assert abm.d1b_start(kind, n) == int(built_lib.tmx_hint_elem_count(kind, n)) + 1136 * n


# ---- GPU
_dev = ta._dev
GUARD = ta.GUARD


@pytest.fixture(scope="module")
def ctx(built_lib):
    import tendermintx_amd as tmx
    c = tmx.Context(4, b"celestia")
    yield c
    c.close()


def _quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_cap, d_pub, pieces=None):
    """the device quotient between two sentinel blocks that must stay untouched; pieces: [(lo, hi)] fed in order, accumulating"""
    import torch
    words = 2 << log_n
    buf = _sentinel(words + 2 * GUARD)
    out = buf[GUARD:].data_ptr()
    a = (log_n, log_blowup, CAP_H, n_proofs, d_cols.data_ptr(), d_cap.data_ptr(), d_pub.data_ptr(), out, 0)
    if pieces is None:
        ctx.air_ladder_boundary_quotient_device(*a)
    else:
        for k, r in enumerate(pieces):
            ctx.air_ladder_boundary_quotient_device(*a, proof_range=r, accumulate=k > 0)
    torch.cuda.synchronize(_dev())
    want = _sentinel(GUARD)
    assert torch.equal(buf[:GUARD], want) and torch.equal(buf[GUARD + words:], want)
    return buf[GUARD:GUARD + words].clone()


def _random_pub(rng, n_proofs, K):
    """random canonical words (no curve point, live flags of any value: the definition is pointwise)"""
    return rng.integers(0, P, (PW * n_proofs, K), dtype=np.uint64)


def _witness_rows(ctx, kind, n, n_proofs, seed, trace=True):
    """(element rows [P][stride], trace rows or None) of one synthetic batch on the device"""
    import torch
    from tendermintx_amd.synth import Workload
    wl = Workload(kind, n, n_proofs, n - 1 if n > 4 else n, chain_id=CID, seed=seed, signed_permille=900)
    dev = _dev()
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None for b in (wl.proofs, wl.targets, wl.trusteds if kind == 0 else b"")]
    out = torch.zeros((n_proofs, ctx.elem_stride(kind)), dtype=torch.int64, device=dev)
    rep = torch.zeros(n_proofs * 64, dtype=torch.uint8, device=dev)
    r = d[2].data_ptr() if d[2] is not None else None
    ctx.witness_batch_device(kind, n_proofs, d[0].data_ptr(), d[1].data_ptr(), r, out.data_ptr(), rep.data_ptr(), 0)
    tr = None
    if trace:
        tr = torch.zeros((n_proofs, ctx.trace_elem_count(kind)), dtype=torch.int64, device=dev)
        ctx.trace_rows_device(kind, n_proofs, d[1].data_ptr(), r, tr.data_ptr(), 63, 0)
    torch.cuda.synchronize(dev)
    return out, tr


def _gather(ctx, kind, n_proofs, d_rows):
    """the device's public table between guards: (device tensor, host [17 P][K])"""
    import torch
    log_k, n_cols = ctx.air_ladder_public_shape(kind, n_proofs)
    words = n_cols << log_k
    buf = _sentinel(words + 2 * GUARD)
    ctx.air_ladder_public_device(kind, n_proofs, d_rows.data_ptr(), buf[GUARD:].data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(buf[:GUARD], _sentinel(GUARD)) and torch.equal(buf[GUARD + words:], _sentinel(GUARD))
    d_pub = buf[GUARD:GUARD + words].clone()
    return d_pub, _down(d_pub).reshape(n_cols, 1 << log_k)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,n_proofs", [(0, 4, 3), (1, 3, 2), (1, 2, 5)])
def test_gather_equals_the_model(built_lib, kind, n, n_proofs):
    """tmx_air_ladder_public_device on the rows tmx_witness_batch_device left equals the model's table built from the same rows (u64, row
    stride tmx_elem_stride, D.1b), guard words intact; step N = 3 has two padding ladders"""
    import tendermintx_amd as tmx
    with tmx.Context(n, CID, max_batch=n_proofs) as c:
        d_rows, _ = _witness_rows(c, kind, n, n_proofs, 8100 + n, trace=False)
        d_pub, got = _gather(c, kind, n_proofs, d_rows)
        rows = _down(d_rows).reshape(n_proofs, -1)
        log_k, n_cols = c.air_ladder_public_shape(kind, n_proofs)
        want = abm.public_table(kind, n, list(rows), log_k)
        assert got.shape == want.shape == (PW * n_proofs, 1 << log_k) and np.array_equal(got, want)
        assert want[16::PW, :2 * n].all() and not want[:, 2 * n:].any()


# (log2 of the trace rows, proofs, log_blowup): K = 2, 8, 256 and 2^12
PUBLIC_SHAPES = [(9, 3, 2), (11, 40, 3), (16, 2, 1), (20, 1, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs,log_blowup", PUBLIC_SHAPES)
def test_public_side_equals_the_model(ctx, oracle, log_rows, n_proofs, log_blowup):
    """V_k, Pub_gamma on the coset and gamma for K in {2, 8, 256, 2^12}, seen through the quotient of all-zero columns, which is
    - Pub_gamma(x_i) / S(x_i) exactly: every word equals the model's, and Pub_gamma on the coset with it (S has no zero there)"""
    log_n, K = log_rows + log_blowup, 1 << (log_rows - 8)
    rng = np.random.default_rng(8200 + log_rows)
    pub = _random_pub(rng, n_proofs, K)
    import torch
    d_cols = torch.zeros(((n_proofs * W) << log_n,), dtype=torch.int64, device=_dev())
    d_cap, d_pub = _up(rng.integers(0, P, 4 << CAP_H, dtype=np.uint64)), _up(pub)
    got = _down(_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_cap, d_pub))
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
        assert np.array_equal(got[k * M:(k + 1) * M].astype(object), want), (k, np.flatnonzero(got[k * M:(k + 1) * M].astype(object) != want)[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs,log_blowup", [(9, 40, 2), (9, 1, 3), (10, 7, 3), (10, 3, 2), (11, 1, 3), (11, 2, 2)])
def test_quotient_of_random_columns_equals_the_model(ctx, oracle, log_rows, n_proofs, log_blowup):
    """the definition is pointwise: on random (non-satisfying) columns and a random public table d_quot and gamma equal the model word for
    word, guard words intact, whole, in two pieces and in three; one piece alone is the model's piece (test_air.py's RANDOM_SHAPES with the
    2^8-row shapes at 2^9: set 2 needs two ladders)"""
    log_n = log_rows + log_blowup
    rng = np.random.default_rng(8300 + log_n * 41 + n_proofs)
    ext, pub = ta._random_ext(rng, log_n, n_proofs), _random_pub(rng, n_proofs, 1 << (log_rows - 8))
    pub[0, 0] = np.uint64(P)  # (a non-canonical word: taken mod p)
    d_cols, d_pub = _up(ext), _up(pub)
    _, d_cap = ta._tree(ctx, d_cols, log_n, n_proofs * W)
    got = _down(_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_cap, d_pub))
    g = abm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _down(d_cap), pub)
    assert ctx.air_last_gamma() == g
    want = abm.quotient(oracle, log_n, log_blowup, n_proofs, ext, pub, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    cut = max(1, n_proofs // 3)
    splits = [[(0, cut), (cut, n_proofs)]] if n_proofs > 1 else [[(0, 1)]]
    if n_proofs > 2:
        splits.append([(0, cut), (cut, cut + 1), (cut + 1, n_proofs)])
        splits.append([(cut, n_proofs), (0, cut)])  # (the piece with proof 0 need not come first)
    for pieces in splits:
        again = _down(_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_cap, d_pub, pieces=pieces))
        assert np.array_equal(again, want), (pieces, np.flatnonzero(again != want)[:10])
    if n_proofs > 1:
        part = _down(_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_cap, d_pub, pieces=[(cut, n_proofs)]))
        assert np.array_equal(part, abm.quotient(oracle, log_n, log_blowup, n_proofs, ext, pub, _shift(), g, proofs=range(cut, n_proofs)))


@pytest.mark.gpu
@pytest.mark.parametrize("which,log_blowup", [("step", 2), ("skip", 3), ("step3", 2)])
def test_quotient_of_real_ladders_equals_the_model(request, ctx, oracle, which, log_blowup):
    """real ladders and their Level-1 table, extended on the device: d_quot and gamma equal the model's, whole and in two pieces, and the
    quotient interpolates to degree < N"""
    import torch
    table, pub = _pick(request, which)
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    log_n = log_rows + log_blowup
    d_ext = _sentinel(table.shape[0] << log_n)
    ctx.lde_device(log_rows, log_blowup, table.shape[0], _up(table).data_ptr(), d_ext.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    ext = oracle.lde(table, log_blowup)
    assert np.array_equal(_down(d_ext).reshape(ext.shape), ext)
    _, d_cap = ta._tree(ctx, d_ext, log_n, n_proofs * W)
    d_pub = _up(pub)
    got = _down(_quotient(ctx, log_n, log_blowup, n_proofs, d_ext, d_cap, d_pub))
    g = abm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, _down(d_cap), pub)
    assert ctx.air_last_gamma() == g
    want = abm.quotient(oracle, log_n, log_blowup, n_proofs, ext, pub, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    again = _down(_quotient(ctx, log_n, log_blowup, n_proofs, d_ext, d_cap, d_pub, pieces=[(0, 1), (1, 2)]))
    assert np.array_equal(again, want)
    assert max(ta._degrees(oracle, got)) < table.shape[1]


E2E = ta.E2E


def _e2e(ctx, oracle, table, pub, quot_override=None):
    """caller-level chain: LDE, trees, set-2 quotient, one batch proof over [trace, quotient].  Returns (params, d_caps, device proof
    words, extended columns, quotient words)"""
    import torch
    log_blowup = E2E["log_blowup"]
    n_cols, log_rows = table.shape[0], table.shape[1].bit_length() - 1
    log_n, n_proofs = log_rows + log_blowup, table.shape[0] // W
    d_ext = _sentinel(n_cols << log_n)
    ctx.lde_device(log_rows, log_blowup, n_cols, _up(table).data_ptr(), d_ext.data_ptr(), 0)
    d_lv_t, d_cap_t = ta._tree(ctx, d_ext, log_n, n_cols)
    d_quot = _quotient(ctx, log_n, log_blowup, n_proofs, d_ext, d_cap_t, _up(pub)) if quot_override is None else _up(quot_override)
    d_lv_q, d_cap_q = ta._tree(ctx, d_quot, log_n, 2)
    p = bparams([log_n, log_n], [n_cols, 2], CAP_H, log_blowup, E2E["arity_bits"], E2E["final_log_max"], E2E["n_queries"])
    words = bm.layout(p)["words"]
    buf = _sentinel(words + 2 * GUARD)
    ctx.batch_prove_device(p, [d_ext.data_ptr(), d_quot.data_ptr()], [d_lv_t.data_ptr(), d_lv_q.data_ptr()], buf[GUARD:].data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(buf[:GUARD], _sentinel(GUARD)) and torch.equal(buf[GUARD + words:], _sentinel(GUARD))
    return p, torch.cat([d_cap_t, d_cap_q]), _down(buf[GUARD:GUARD + words].clone()), _down(d_ext).reshape(n_cols, -1), _down(d_quot)


def _verdicts(ctx, p, k_trace, d_caps, proof, pub):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    d_proof, d_pub = _up(proof), _up(pub)  # (both kept until the call has run)
    ctx.air_boundary_verify_device(p, k_trace, d_caps.data_ptr(), d_proof.data_ptr(), d_pub.data_ptr(), ok.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    out = ok.cpu().numpy()
    assert ((out == 0) | (out == 1)).all(), out
    return [bool(x) for x in out]


@pytest.mark.gpu
def test_caller_level_end_to_end(ctx, oracle, step2):
    """LDE, trees, set-2 quotient, batch prove over [trace, quotient]: the proof equals batch_model.prove on the model's quotient word for
    word; tmx_air_boundary_verify_device and the model verifier accept every query; with one changed public word or one flipped live flag
    every query is rejected, by both; set 1's verifier rejects the set-2 quotient"""
    table, pub = step2
    p, d_caps, got, ext, quot = _e2e(ctx, oracle, table, pub)
    log_n, n_proofs = p["log_n"][0], table.shape[0] // W
    caps = _down(d_caps)
    g = abm.gamma(oracle, log_n, p["log_blowup"], CAP_H, n_proofs, caps[:4 << CAP_H], pub)
    want_q = abm.quotient(oracle, log_n, p["log_blowup"], n_proofs, ext, pub, _shift(), g)
    assert np.array_equal(quot, want_q)
    want, deg, zeta, _ = bm.prove(oracle, p, [ext, want_q.reshape(2, -1)], _shift())
    assert deg and ctx.fri_last_degree_ok() is True and ctx.deep_last_zeta() == zeta
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert abm.identity(oracle, p, 0, caps, got, pub)
    assert all(abm.verify(oracle, p, 0, caps, got, _shift(), pub))
    assert all(_verdicts(ctx, p, 0, d_caps, got, pub))
    assert not any(ta._verdicts(ctx, p, 0, d_caps, got)) and not am.identity(oracle, p, 0, caps, got)
    for kind in PUB_KINDS:
        _, bad = _tamper(table, pub, kind)
        assert not abm.identity(oracle, p, 0, caps, got, bad), kind
        assert not any(abm.verify(oracle, p, 0, caps, got, _shift(), bad)), kind
        assert not any(_verdicts(ctx, p, 0, d_caps, got, bad)), kind
    L = bm.layout(p)
    R = 1 << dm.log_r(p["n_cols"][0])
    for name, at in (("nxt opening at zeta", L["off_open"][0] + am.NXT + 2), ("acc opening at zeta omega", L["off_open"][0] + 2 * R + W + am.ACC + 8),
                     ("quotient opening", L["off_open"][1] + 1)):
        bad = got.copy()
        bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
        model = abm.verify(oracle, p, 0, caps, bad, _shift(), pub)
        assert not any(model), name
        assert _verdicts(ctx, p, 0, d_caps, bad, pub) == model, name


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ROW_KINDS)
def test_tampered_trace_proved_honestly(ctx, oracle, step2, kind):
    """a trace with a changed acc_0 (or a consistent change on a ladder's last row) and its honest set-2 quotient: the quotient has degree
    >= N, so the degree flag is 0 and not every query is accepted; the device's verdicts are the model's query by query"""
    table, pub = step2
    bad, _ = _tamper(table, pub, kind)
    p, d_caps, got, ext, quot = _e2e(ctx, oracle, bad, pub)
    assert ctx.fri_last_degree_ok() is False
    caps = _down(d_caps)
    n_proofs = bad.shape[0] // W
    g = abm.gamma(oracle, p["log_n"][0], p["log_blowup"], CAP_H, n_proofs, caps[:4 << CAP_H], pub)
    want_q = abm.quotient(oracle, p["log_n"][0], p["log_blowup"], n_proofs, ext, pub, _shift(), g)
    assert np.array_equal(quot, want_q) and max(ta._degrees(oracle, quot)) >= bad.shape[1]
    want, deg, _, _ = bm.prove(oracle, p, [ext, want_q.reshape(2, -1)], _shift())
    assert deg is False and np.array_equal(got, want)
    model = abm.verify(oracle, p, 0, caps, got, _shift(), pub)
    device = _verdicts(ctx, p, 0, d_caps, got, pub)
    print(f"\n[air2] {kind}, honest quotient: device verdicts {device}")
    assert device == model and not all(device)


@pytest.mark.gpu
def test_zero_quotient_for_a_tampered_trace(ctx, oracle, step2):
    """a zero (low-degree) quotient committed for a trace with a changed acc_0: the batch proof is fine -- tmx_batch_verify_device accepts
    every query -- and the identity fails: tmx_air_boundary_verify_device rejects every one, as the model does"""
    table, pub = step2
    bad, _ = _tamper(table, pub, "acc at r = 0")
    log_n = bad.shape[1].bit_length() - 1 + E2E["log_blowup"]
    p, d_caps, got, ext, quot = _e2e(ctx, oracle, bad, pub, quot_override=np.zeros(2 << log_n, dtype=np.uint64))
    assert ctx.fri_last_degree_ok() is True
    caps = _down(d_caps)
    assert all(ta._verdicts(ctx, p, 0, d_caps, got, batch_only=True)) and all(bm.verify(oracle, p, caps, got, _shift()))
    assert not abm.identity(oracle, p, 0, caps, got, pub)
    model = abm.verify(oracle, p, 0, caps, got, _shift(), pub)
    device = _verdicts(ctx, p, 0, d_caps, got, pub)
    assert device == model and not any(device)


_refused = ta._refused


@pytest.mark.gpu
def test_each_validation_rule(ctx):
    """every rule on its own: TMX_ERR_BAD_ARG before anything is enqueued, nothing written"""
    import torch
    log_n, lb, n_proofs = 11, 2, 1
    d_cols = _sentinel((n_proofs * W) << log_n)
    d_cap, d_quot, d_pub = _sentinel(4 << CAP_H), _sentinel(2 << log_n), _sentinel(PW << 1)
    ptrs = (d_cols.data_ptr(), d_cap.data_ptr(), d_pub.data_ptr(), d_quot.data_ptr(), 0)
    q = lambda ln, b, n, **kw: (lambda: ctx.air_ladder_boundary_quotient_device(ln, b, CAP_H, n, *ptrs, **kw))
    for fn in (q(log_n, 0, 1), q(log_n, 7, 1), q(2, 2, 1), q(29, 2, 1), q(10, 2, 1), q(14, 6, 1), q(23, 2, 1), q(log_n, lb, 0),
               q(log_n, lb, (1 << 24) // W + 1), q(log_n, lb, 1, proof_range=(0, 0)), q(log_n, lb, 1, proof_range=(1, 1)),
               q(log_n, lb, 1, proof_range=(0, 2)), q(log_n, lb, 1, proof_range=(0, 1), accumulate=2)):
        _refused(fn, d_quot)
    for k in range(4):
        a = [d_cols.data_ptr(), d_cap.data_ptr(), d_pub.data_ptr(), d_quot.data_ptr()]
        a[k] = None
        assert "d_pub" in _refused(lambda: ctx.air_ladder_boundary_quotient_device(log_n, lb, CAP_H, 1, *a, 0), d_quot)
    ok, caps, proof = torch.full((4,), 7, dtype=torch.int32, device=_dev()), _sentinel(64), _sentinel(1 << 16)
    v = lambda p, k, pub=d_pub: (lambda: ctx.air_boundary_verify_device(p, k, caps.data_ptr(), proof.data_ptr(), pub.data_ptr() if pub is not None else None,
                                                                        ok.data_ptr(), 0))
    good = bparams([11, 11], [W, 2], CAP_H, lb, 2, 2, 4)
    for p, k in ((good, 1), (dict(good, n_cols=[W + 1, 2]), 0), (dict(good, n_cols=[W, 3]), 0), (dict(good, log_n=[11, 10]), 0),
                 (bparams([10, 10], [W, 2], CAP_H, lb, 2, 2, 4), 0), (dict(good, arity_bits=0), 0), (bparams([11], [W], CAP_H, lb, 2, 2, 4), 0)):
        _refused(v(p, k), ok)
    assert "d_pub" in _refused(v(good, 0, None), ok)
    rows, pub = _sentinel(16), _sentinel(16)
    for fn in (lambda: ctx.air_ladder_public_device(2, 1, rows.data_ptr(), pub.data_ptr(), 0),
               lambda: ctx.air_ladder_public_device(0, 0, rows.data_ptr(), pub.data_ptr(), 0),
               lambda: ctx.air_ladder_public_device(0, 1, None, pub.data_ptr(), 0), lambda: ctx.air_ladder_public_device(0, 1, rows.data_ptr(), None, 0)):
        _refused(fn, pub)


def _set_case(built_lib, oracle, kind, n, n_proofs, sections, streamed, chunk, log_blowup=3, model=False, queries=6):
    """set, gather, air (set 2), shape, prove, verify on one context; returns everything comparable: (caps, cap_q, proof, params, pub)"""
    import torch
    import tendermintx_amd as tmx
    with tmx.Context(n, CID, max_batch=n_proofs) as c:
        d_rows, tr = _witness_rows(c, kind, n, n_proofs, 8400 + n + n_proofs)
        d_pub, pub = _gather(c, kind, n_proofs, d_rows)
        n_tab = bin(sections).count("1")
        d_caps = _sentinel(n_tab * (4 << CAP_H))
        if streamed is None:
            c.trace_commit_set_device(kind, n_proofs, sections, log_blowup, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        else:
            c.trace_commit_set_streamed_device(kind, n_proofs, sections, streamed, chunk, log_blowup, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        shape0, order0 = c.trace_commit_set_shape()
        d_cap_q = _sentinel(4 << CAP_H)
        c.trace_commit_set_air_boundary_device(d_pub.data_ptr(), d_cap_q.data_ptr(), 0)
        gamma = c.air_last_gamma()
        shape, order = c.trace_commit_set_shape()
        kt = order.index(LADDERS)
        assert order == order0[:kt + 1] + [QUOTIENT] + order0[kt + 1:]
        assert shape["n_cols"] == shape0["n_cols"][:kt + 1] + [2] + shape0["n_cols"][kt + 1:] and shape["n_cols"][kt] == W * n_proofs
        # the two set-level calls exclude each other: whichever comes second is refused
        assert "already holds" in _refused(lambda: c.trace_commit_set_air_device(d_cap_q.data_ptr(), 0), d_cap_q)
        assert "already holds" in _refused(lambda: c.trace_commit_set_air_boundary_device(d_pub.data_ptr(), d_cap_q.data_ptr(), 0), d_cap_q)
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
        caps_h, got = _down(all_caps), _down(after)
        assert all(_verdicts(c, p, kt, all_caps, got, pub))
        assert not any(_verdicts(c, p, kt, all_caps, got, _tamper(pub, pub, "one flipped live")[1]))
        assert gamma == abm.gamma(oracle, p["log_n"][kt], log_blowup, CAP_H, n_proofs, caps_h[kt * cw:(kt + 1) * cw], pub)
        assert abm.identity(oracle, p, kt, caps_h, got, pub)
        if model:
            from test_merkle_open import _oracle_ext
            traces = _down(tr)
            ext = []
            for k, sec in enumerate(order):
                if sec == QUOTIENT:
                    ext.append(abm.quotient(oracle, p["log_n"][kt], log_blowup, n_proofs, ext[kt], pub, _shift(), gamma).reshape(2, -1))
                    continue
                e, lm, nc = _oracle_ext(oracle, kind, n, traces, sec, log_blowup)
                assert (lm, nc) == (p["log_n"][k], p["n_cols"][k])
                ext.append(e.reshape(nc, -1))
            want, deg, _, _ = bm.prove(oracle, p, ext, _shift())
            assert deg and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
            assert all(abm.verify(oracle, p, kt, caps_h, got, _shift(), pub))
        # the set-1 call on a fresh set still works after a set-2 call on the context, and refuses a set-2 call behind it
        if streamed is None:
            c.trace_commit_set_device(kind, n_proofs, sections, log_blowup, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
            c.trace_commit_set_air_device(d_cap_q.data_ptr(), 0)
            assert "already holds" in _refused(lambda: c.trace_commit_set_air_boundary_device(d_pub.data_ptr(), d_cap_q.data_ptr(), 0), d_cap_q)
        return _down(d_caps), caps_h[(kt + 1) * cw:(kt + 2) * cw], got, p, pub


@pytest.mark.gpu
def test_set_of_the_ladders_alone_equals_the_model(built_lib, oracle):
    """a set of LADDERS alone (step, N = 2, two proofs): gather, set, air, shape, prove, verify; the proof of the enlarged set equals
    batch_model.prove on the model's set-2 quotient; the model verifier and the identity accept"""
    caps, cap_q, after, p, pub = _set_case(built_lib, oracle, 1, 2, 2, LADDERS, None, 0, log_blowup=2, model=True)
    assert p["log_n"] == [12, 12] and p["n_cols"] == [2 * W, 2]


@pytest.mark.gpu
def test_set_of_all_five_tables_resident_and_streamed(built_lib, oracle):
    """all five tables (skip, N = 4, nine proofs: 585 ladder columns), the ladders resident and streamed in chunks of 72 (65 columns = one
    proof per chunk) and 200 (195 columns = three proofs): caps, quotient cap and every proof word equal; the ladders alone give the same
    quotient cap"""
    want = _set_case(built_lib, oracle, 0, 4, 9, ALL, None, 0)
    assert want[3]["n_cols"][want[3]["log_n"].index(14)] == 9 * W
    for chunk in (72, 200):
        got = _set_case(built_lib, oracle, 0, 4, 9, ALL, LADDERS, chunk)
        for a, b, name in zip(got[:3], want[:3], ("caps", "quotient cap", "proof")):
            assert np.array_equal(a, b), (chunk, name, np.flatnonzero(a != b)[:10])
        assert got[3] == want[3] and np.array_equal(got[4], want[4])
    for streamed, chunk in ((None, 0), (LADDERS, 200)):
        alone = _set_case(built_lib, oracle, 0, 4, 9, LADDERS, streamed, chunk)
        assert np.array_equal(alone[1], want[1])  # (gamma and the quotient depend on the ladders and the table alone)


@pytest.mark.gpu
def test_set_level_refusals(built_lib):
    """no set; a set without the ladders; a streamed ladders member with chunk_cols < 65; null pointers: TMX_ERR_BAD_ARG, nothing written,
    the set intact"""
    import tendermintx_amd as tmx
    with tmx.Context(4, CID, max_batch=2) as c:
        d_cap_q, d_pub = _sentinel(4 << CAP_H), _sentinel(2 * PW * 8)
        air = lambda pub=d_pub, cap=d_cap_q: (lambda: c.trace_commit_set_air_boundary_device(pub.data_ptr() if pub is not None else None,
                                                                                             cap.data_ptr() if cap is not None else None, 0))
        assert "no commit set" in _refused(air(), d_cap_q)
        d_rows, tr = _witness_rows(c, 0, 4, 2, 8500)
        caps = _sentinel(5 * (4 << CAP_H))
        c.trace_commit_set_device(0, 2, SHA512 | TREE, 3, CAP_H, tr.data_ptr(), caps.data_ptr(), 0)
        assert "LADDERS" in _refused(air(), d_cap_q)
        c.trace_commit_set_streamed_device(0, 2, ALL, LADDERS, 64, 3, CAP_H, tr.data_ptr(), caps.data_ptr(), 0)
        assert "chunk_cols" in _refused(air(), d_cap_q)
        shape, order = c.trace_commit_set_shape()
        assert QUOTIENT not in order and len(order) == 5
        assert "d_cap_q" in _refused(air(cap=None))
        assert "d_pub" in _refused(air(pub=None), d_cap_q)


# ---- GPU, full size: 256 proofs at N = 128, the ladders streamed (tests/test_commit_streamed.py's fixture and memory rule)
from test_commit_streamed import FULL, FULL_CHUNK, FULL_ORDER, full  # noqa: E402,F401


@pytest.mark.gpu
def test_full_size_five_tables_with_the_boundary_quotient(full, oracle):
    """256 proofs x N = 128, blow-up 8: the public table (4352 columns of K = 256) gathered from a witness batch of the same inputs, all
    five tables with the ladders streamed in chunks of 512 columns, the set-2 quotient, one proof over the six oracles: all 28 queries are
    accepted by the device verifier and by the model's verifier and identity; one flipped live flag rejects every one"""
    import torch
    from tendermintx_amd.context import trace_commit_set_bytes as nbytes
    ctx, tr = full
    M = 1 << 19
    need = nbytes(0, FULL["n"], FULL["proofs"], ALL, LADDERS, FULL_CHUNK, FULL["log_blowup"], FULL["cap_height"]) + (2 * M) * 8 * 4
    torch.cuda.empty_cache()
    free_b, total_b = torch.cuda.mem_get_info(_dev())
    print(f"\n[air2] full size: streamed set + quotient {need / 2**30:.1f} GiB, free {free_b / 2**30:.1f} of {total_b / 2**30:.1f} GiB", flush=True)
    assert 0 < need < free_b, (need, free_b)
    d_pub, pub = _full_pub(ctx)
    assert pub.shape == (PW * FULL["proofs"], 256) and pub[16::PW].sum() > 128 * FULL["proofs"] and int(pub.max()) < 1 << 32
    cw = 4 << FULL["cap_height"]
    d_caps = _sentinel(5 * cw)
    ctx.trace_commit_set_streamed_device(0, FULL["proofs"], ALL, LADDERS, FULL_CHUNK, FULL["log_blowup"], FULL["cap_height"], tr.data_ptr(),
                                         d_caps.data_ptr(), 0)
    d_cap_q = _sentinel(cw)
    ctx.trace_commit_set_air_boundary_device(d_pub.data_ptr(), d_cap_q.data_ptr(), 0)
    gamma = ctx.air_last_gamma()
    shape, order = ctx.trace_commit_set_shape()
    assert order == [LADDERS, QUOTIENT] + FULL_ORDER[1:] and shape["log_n"] == [19, 19, 18, 18, 17, 15]
    assert shape["n_cols"] == [16640, 2, 4608, 2304, 2304, 2304]
    p = dict(shape, arity_bits=FULL["arity_bits"], final_log_max=FULL["final_log_max"], n_queries=FULL["n_queries"], pow_bits=0)
    assert p["n_queries"] == 28
    d_proof = _sentinel(bm.layout(p)["words"])
    ctx.trace_commit_set_prove_device(p, d_proof.data_ptr(), 0)
    assert ctx.fri_last_degree_ok() is True
    all_caps = torch.cat([d_caps[:cw], d_cap_q, d_caps[cw:]])
    got, caps = _down(d_proof), _down(all_caps)

    def verdicts(table):
        ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
        d_table = _up(table)
        ctx.air_boundary_verify_device(p, 0, all_caps.data_ptr(), d_proof.data_ptr(), d_table.data_ptr(), ok.data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        return [int(x) for x in ok.cpu().numpy()]

    assert verdicts(pub) == [1] * 28
    assert gamma == abm.gamma(oracle, 19, FULL["log_blowup"], FULL["cap_height"], FULL["proofs"], caps[:cw], pub)
    assert abm.identity(oracle, p, 0, caps, got, pub)
    assert all(bm.verify(oracle, p, caps, got, _shift()))
    bad = pub.copy()
    bad[PW * 200 + 16, 77] ^= np.uint64(1)
    assert verdicts(bad) == [0] * 28 and not abm.identity(oracle, p, 0, caps, got, bad)


def _full_pub(ctx):
    """the public table of the full-size fixture's batch: the fixture keeps the trace rows only, so the witness batch of the same workload
    runs once more (same inputs, same values) and its element rows are gathered on the device"""
    import torch
    from tendermintx_amd.synth import bench_workload
    n, n_proofs = FULL["n"], FULL["proofs"]
    w = bench_workload("survey8d", n, n_proofs, seed=0x544D58)
    dev = _dev()
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (w.proofs, w.targets, w.trusteds)]
    out = torch.empty(n_proofs * ctx.elem_stride(0), dtype=torch.int64, device=dev)
    rep = torch.empty(n_proofs * 64, dtype=torch.uint8, device=dev)
    ctx.witness_batch_device(0, n_proofs, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), rep.data_ptr(), 0)
    torch.cuda.synchronize(dev)
    return _gather(ctx, 0, n_proofs, out)
