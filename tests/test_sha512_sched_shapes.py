"""The set-8 kernels (tendermintx_amd/csrc/air.hip k_air_sha512_sched_helper, k_air_sha512_periodic<Sha512Sched>, k_air_sha512_periodic_eval<Sha512Sched>,
k_air_sha512_tables<Sha512Sched>, k_air_sha512_quotient<Sha512Sched, FORM>, k_air_sha512_check<Sha512Sched>) and their host paths (api.cpp sha_pass, sha_verify_call,
sha_set_call under SHA_SETS[5] and SHA8_PERIODIC, sha512_scratch on d_air8) at every shape and row value they branch on: a high-limb carry
that exists through the low limb's carry alone (and one that needs all of CL = 3, not its low bit), all sixteen (CL, CH) pairs, the carry
columns on SCH-off rows under operands that would carry, a verifier that folds 2, 4 and 32 rows of the barycentric kernel's `part`, the
rows-per-thread regimes of that kernel and a zero denominator in every batch slot, in a workgroup other than 0 and on SCH-on rows, N = 256
(the wrap row on t = 15), 17 proofs, cap height 0, three pieces in three orders, the extreme words of the lazy field arithmetic, the sizes of
the openings planes, the set of openings the identity reads, the skip kind, set 1 beside set 8, a moved NTT domain, and a verifier call as the
first set-8 call of a context.  The yardstick stays tests/sha512_sched_model.py on tests/batch_model.py: device words equal the model's word
for word, every device verdict equals the model's, guard words stay intact.  The helpers and fixtures are those of tests/test_sha512_sched.py,
tests/test_sha512_air_shapes.py, tests/test_sha_air_shapes.py and tests/test_sha_air.py; docs/kernels.md "set 8: which test reaches which
shape" is the map."""
import functools

import numpy as np
import pytest

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha512_sched_model as sm
from batch_model import bparams
from test_fri import _down, _sentinel, _shift, _up
from test_sha512_air import _columns
from test_sha512_air_shapes import step2_rows  # noqa: F401
from test_sha512_sched import (CAP_H, HC, HEADER, HELPER, QUOTIENT, SHA512, W, _bary, _chain, _device_helper, _device_quotient,  # noqa: F401
                               _model_quotient, _periodic, _schedule, _verdicts, ctx)
from test_sha_air import GUARD, _cap, _degrees, _dev, _guarded, _random_ext, _tree
from test_sha_air_shapes import FILLS, _bumped, _Remembering

P = fm.P
BLOCK, M32, M64 = sm.BLOCK, sm.M32, sm.M64


# ---- honest tables of any size
def _block(w16, rng):
    """[18][80]: W_0 .. W_79 of the sixteen message words in lo / hi limbs; the sixteen columns set 8 does not speak about hold random 32-bit
    words, so that a kernel reading the wrong column is seen"""
    b = rng.integers(0, 1 << 32, (W, BLOCK), dtype=np.uint64)
    w = _schedule(w16)
    b[sm.W_], b[sm.W_ + 1] = [x & M32 for x in w], [x >> 32 for x in w]
    return b


def _slots(n_blocks):
    """the places of a tiling that are not zero blocks"""
    return [g for g in range(n_blocks) if g % 7 != 6]


def _tiled(N, n_proofs, planted=()):
    """[18 n_proofs][N] pre-LDE columns: random honest blocks, every seventh block of the tiling all zero; the rows behind the last full
    block (N is no multiple of 80) hold the first rows of an honest block in even proofs and zeros in odd ones; `planted` blocks take the
    first places that are not zero blocks.  A block's transitions 15 -> 16 .. 78 -> 79 are honest and SCH is off on every other row, so
    every tiling satisfies the set."""
    rng = np.random.default_rng(11000 + N + n_proofs)
    rand16 = lambda: [int(x) for x in rng.integers(0, 1 << 64, 16, dtype=np.uint64)]
    nb, tail = divmod(N, BLOCK)
    table = np.zeros((n_proofs * W, N), dtype=np.uint64)
    slots = _slots(n_proofs * nb)
    assert len(planted) <= len(slots)
    for k, g in enumerate(slots):
        p, b = divmod(g, nb)
        table[p * W:(p + 1) * W, BLOCK * b:BLOCK * b + BLOCK] = planted[k] if k < len(planted) else _block(rand16(), rng)
    for p in range(0, n_proofs, 2):
        table[p * W:(p + 1) * W, BLOCK * nb:] = _block(rand16(), rng)[:, :tail]
    return table


def _carries(help_):
    """(CL, CH) as [n_proofs][N] values"""
    return help_[sm.HCL::HC] + 2 * help_[sm.HCL + 1::HC], help_[sm.HCH::HC] + 2 * help_[sm.HCH + 1::HC]


def _on(N):
    return sm.periodic(N).astype(bool)


@pytest.mark.parametrize("N,n_proofs", [(128, 5), (2048, 1)])
def test_tiled_tables_satisfy_the_constraints_as_integers(N, n_proofs):
    """the tiling at N = 128 (one full block and a 48-row partial one per proof, honest in proofs 0, 2, 4 and zero in 1, 3) and N = 2048
    (25 full blocks, three of them zero, and a 48-row partial one): all 234 constraints are integer identities on every row"""
    table = _tiled(N, n_proofs)
    help_ = sm.helper(table, n_proofs)
    assert table[sm.W_, -1] and (n_proofs == 1 or not table[W:2 * W, BLOCK * (N // BLOCK):].any())
    assert N == 128 or not table[:, 6 * BLOCK:7 * BLOCK].any()
    for p in range(n_proofs):
        for j, c in enumerate(sm.integer_residuals(table[p * W:(p + 1) * W], help_[p * HC:(p + 1) * HC])):
            assert not c.any(), (p, j, np.flatnonzero(c)[:4])


def test_tiled_quotient_has_degree_at_most_n_minus_2_and_the_identity_holds(oracle):
    """N = 128, 3 proofs, blow-up 4: the model quotient interpolates to degree <= N - 2 in both planes; the identity holds on a
    tests/batch_model.py proof over [table, helper, quotient] and fails after one helper opening of proof 2 is bumped"""
    N, n_proofs, lb = 128, 3, 2
    oracle = _Remembering(oracle)
    table = _tiled(N, n_proofs)
    ext, hext, g, quot = _model_quotient(oracle, table, sm.helper(table, n_proofs), lb)
    deg = _degrees(oracle, quot)
    print(f"\n[sha512-sched shapes] N = {N}, {n_proofs} proofs: quotient degrees {deg}")
    assert max(deg) <= N - 2
    log_n = 7 + lb
    p = bparams([log_n] * 3, [n_proofs * W, n_proofs * HC, 2], CAP_H, lb, 2, 2, 1)
    cols = [ext, hext, quot.reshape(2, -1)]
    caps = np.concatenate([_cap(oracle, c, log_n) for c in cols])
    proof, degree_ok, _, _ = bm.prove(oracle, p, cols, _shift())
    assert degree_ok and sm.identity(oracle, p, 0, 1, caps, proof)
    at = bm.layout(p)["off_open"][1] + 2 * HC + sm.HX1 + 41
    proof[at] = np.uint64((int(proof[at]) + 1) % P)
    assert not sm.identity(oracle, p, 0, 1, caps, proof)


# ---- the edge blocks of the helper's definition
def _pairs(w16):
    """the (CL, CH) of the rows t = 15 .. 78 of one block in plain integers, from the schedule's four summands per limb (not the model)"""
    w = _schedule(w16)
    out = []
    for t in range(16, BLOCK):
        terms = (w[t - 16], sm.small_sigma0(w[t - 15]), w[t - 7], sm.small_sigma1(w[t - 2]))
        cl = sum(x & M32 for x in terms) >> 32
        out.append((cl, (sum(x >> 32 for x in terms) + cl) >> 32))
    return out


A_AT, B_AT, ONES_AT, ONE_AT, HIGH_AT = range(5)


@functools.lru_cache(maxsize=None)
def _edge_blocks(high_bits=True):
    """honest blocks [18][80] of chosen message words (w[1] = w[14] = 0 and the others 0 unless given), in this order:
    A: w[0] = 2^64 - 1, w[9] = 1 -- on row 15 the low limbs sum to 2^32 (CL = 1) and the high limbs to 2^32 - 1, so CH = 1 through CL alone;
    B: w[0].lo = w[9].lo = 0xFFFFFFFF, w[1] and w[14] searched with a seeded generator so that sigma0's and sigma1's low limbs lift the low
    sum to 3 * 2^32 or more (CL = 3), w[9].hi = 0xFFFFFFFF and w[0].hi chosen so that the high limbs sum to 2 * 2^32 - 3: CH = 2 under the
    full CL = 3 and 1 under its low bit alone or without it;
    all sixteen words 2^64 - 1; w[0] = 1 alone (every carry of row 15 is 0 on an SCH-on row); high_bits: an honest random block whose two W
    limbs carry random bits above bit 31 in the stored words (for helper-only tables: the operands are the low 32 bits);
    then random honest blocks, taken while one of the sixteen (CL, CH) pairs is still missing from the rows of the blocks so far"""
    rng = np.random.default_rng(11100)
    rand64 = lambda: int(rng.integers(0, 1 << 64, dtype=np.uint64))
    words = lambda given: [given.get(k, 0) for k in range(16)]
    while True:
        w1, w14 = rand64(), rand64()
        s0, s1 = sm.small_sigma0(w1), sm.small_sigma1(w14)
        if (s0 & M32) + (s1 & M32) >= (1 << 32) + 2 and (s0 >> 32) + (s1 >> 32) <= (1 << 32) - 2:
            break
    w0_hi = (1 << 33) - 3 - (M32 + (s0 >> 32) + (s1 >> 32))
    assert 0 <= w0_hi <= M32
    w16s = [words({0: M64, 9: 1}), words({0: w0_hi << 32 | M32, 1: w1, 9: M64, 14: w14}), [M64] * 16, words({0: 1})]
    out = [_block(w16, rng) for w16 in w16s]
    seen = {pair for w16 in w16s for pair in _pairs(w16)}
    if high_bits:
        high = _block([rand64() for _ in range(16)], rng)
        high[sm.W_:sm.W_ + 2] |= rng.integers(1, 1 << 32, (2, BLOCK), dtype=np.uint64) << np.uint64(32)
        out.append(high)
    while len(seen) < 16:
        w16 = [rand64() for _ in range(16)]
        if set(_pairs(w16)) - seen:
            seen |= set(_pairs(w16))
            out.append(_block(w16, rng))
    assert len(out) <= 24
    return tuple(out)


def _carry_facts(table, help_):
    """from a table [18 p][N] and its helper: (the set of (CL, CH) pairs on SCH-on rows, the largest carry bit on an SCH-off row, the
    number of SCH-on rows where CH differs from the high-limb sum's own carry (QH_15 >> 32) & 3: the carry-in from the low limb decides)"""
    on = _on(table.shape[1])
    cl, ch = _carries(help_)
    own = (help_[sm.HQH + 15::HC] >> np.uint64(32)) & np.uint64(3)
    pairs = {(int(a), int(b)) for a, b in zip(cl[:, on].reshape(-1), ch[:, on].reshape(-1))}
    off = int(max(help_[c::HC][:, ~on].max() for c in range(sm.HCL, HC)))
    return pairs, off, int((own != ch)[:, on].sum())


def _row_15(help_, p, block):
    """(CL, CH, the high-limb sum's own carry) on row 15 of a block of proof p"""
    cl, ch = _carries(help_)
    r = BLOCK * block + 15
    return int(cl[p, r]), int(ch[p, r]), int(help_[p * HC + sm.HQH + 15, r] >> np.uint64(32)) & 3


def _wrap_on_15(edges, rng=None):
    """N = 256, one proof, whose 16-row tail is the first rows of block A: the wrap row N - 1 is t = 15 under operands that would carry"""
    table = _tiled(256, 1) if rng is None else rng.integers(0, 1 << 64, (W, 256), dtype=np.uint64)
    table[:, 240:] = edges[A_AT][:, :16]
    return table


def test_edge_blocks_reach_the_carries_they_claim():
    """the edge blocks in one 2048-row proof (the first places of the tiling that are not zero blocks), by the model: row 15 of block A
    gives (CL, CH) = (1, 1) with the high-limb sum's own carry 0, row 15 of block B (3, 2) with the high-limb sum's own carry 1, row 15
    of the all-ones block CL = 3 and of the w[0] = 1 block (0, 0); every one of the sixteen (CL, CH) pairs occurs; all four carry bits are 0
    on every SCH-off row, also on row N - 1 of an N = 256 table whose tail is the first 16 rows of block A (there QL_15 >> 32 is 1 and
    (CL, CH) = (0, 0)); CH differs from the high-limb sum's own carry on at least 2 SCH-on rows, so the reference alone shows that the
    carry-in matters; the plain-integer pairs of _pairs are the model's"""
    edges = _edge_blocks()
    N, slots = 2048, _slots(25)
    table = _tiled(N, 1, edges)
    help_ = sm.helper(table, 1)
    at = lambda k: slots[k]
    assert _row_15(help_, 0, at(A_AT)) == (1, 1, 0) and _row_15(help_, 0, at(B_AT)) == (3, 2, 1)
    assert _row_15(help_, 0, at(ONES_AT))[0] == 3 and _row_15(help_, 0, at(ONE_AT))[:2] == (0, 0)
    assert int(table[sm.W_, BLOCK * at(HIGH_AT):BLOCK * at(HIGH_AT) + BLOCK].min()) >> 32
    pairs, off, decisive = _carry_facts(table, help_)
    print(f"\n[sha512-sched shapes] {len(edges)} edge blocks; {len(pairs)} (CL, CH) pairs; the carry-in decides CH on {decisive} rows")
    assert pairs == {(a, b) for a in range(4) for b in range(4)} and off == 0 and decisive >= 2
    cl, ch = _carries(help_)
    for k in (A_AT, B_AT):
        w16 = [int(table[sm.W_, BLOCK * at(k) + j]) | int(table[sm.W_ + 1, BLOCK * at(k) + j]) << 32 for j in range(16)]
        r0 = BLOCK * at(k) + 15
        assert _pairs(w16) == [(int(a), int(b)) for a, b in zip(cl[0, r0:r0 + 64], ch[0, r0:r0 + 64])]
    small = _wrap_on_15(edges)
    hs = sm.helper(small, 1)
    assert int(hs[sm.HQL + 15, 255]) >> 32 == 1 and _carry_facts(small, hs)[1] == 0 and not hs[sm.HCL:, 255].any()
    for j, c in enumerate(sm.integer_residuals(small, hs)):
        assert not c.any(), j
    honest = _tiled(N, 1, _edge_blocks(high_bits=False))
    for j, c in enumerate(sm.integer_residuals(honest, sm.helper(honest, 1))):
        assert not c.any(), j


# ---- GPU: the helper
@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs", [(7, 5), (8, 1), (11, 2), (12, 1)])
def test_helper_at_every_grid_shape_equals_the_model(ctx, log_rows, n_proofs):
    """random 64-bit words at 128 rows x 5 proofs (the grid's last workgroup half filled), 256 rows (one workgroup; the wrap row is t = 15),
    2048 x 2 and 4096.  At (7, 5) blocks A, B, all-ones, w[0] = 1 and the high-bits block are block 0 of proofs 0 .. 4; at (11, 2) every
    edge block is planted; at (8, 1) the 16-row tail is block A's first rows.  The helper equals the model's word for word, guard words
    intact, and the DEVICE's words show the carry facts: all four carry bits 0 on every SCH-off row; where planted, (1, 1) on row 15 of A
    with the high-limb sum's own carry 0, (3, 2) on row 15 of B with its own carry 1, and the carry-in decisive on at least 2 rows; at
    (11, 2) all sixteen (CL, CH) pairs; at (8, 1) (0, 0) on row N - 1 while QL_15 >> 32 is 1 there"""
    rng = np.random.default_rng(11200 + 10 * log_rows + n_proofs)
    N = 1 << log_rows
    nb = N // BLOCK
    table = rng.integers(0, 1 << 64, (n_proofs * W, N), dtype=np.uint64)
    edges = _edge_blocks()
    where = []
    if (log_rows, n_proofs) == (7, 5):
        where = [(p, 0) for p in range(5)]
    elif (log_rows, n_proofs) == (11, 2):
        where = [divmod(g, nb) for g in range(len(edges))]
    elif log_rows == 8:
        table = _wrap_on_15(edges, rng)
    for (p, b), block in zip(where, edges):
        table[p * W:(p + 1) * W, BLOCK * b:BLOCK * b + BLOCK] = block
    got = _down(_device_helper(ctx, table)).reshape(n_proofs * HC, -1)
    want = sm.helper(table, n_proofs)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    pairs, off, decisive = _carry_facts(table, got)
    print(f"\n[sha512-sched shapes] helper ({log_rows}, {n_proofs}): {len(pairs)} (CL, CH) pairs, largest carry bit on an SCH-off row {off}, "
          f"carry-in decisive on {decisive} rows")
    assert off == 0
    if where:
        assert _row_15(got, *where[A_AT]) == (1, 1, 0) and _row_15(got, *where[B_AT]) == (3, 2, 1) and decisive >= 2
        assert _row_15(got, *where[ONES_AT])[0] == 3 and _row_15(got, *where[ONE_AT])[:2] == (0, 0)
    if log_rows == 11:
        assert pairs == {(a, b) for a in range(4) for b in range(4)}
    if log_rows == 8:
        assert int(got[sm.HQL + 15, 255]) >> 32 == 1 and not got[sm.HCL:, 255].any()


# ---- GPU: SCH and the barycentric kernel
@pytest.mark.gpu
def test_sch_and_its_extension_at_2048_rows(ctx, oracle):
    """N = 2048 (eight workgroups of k_air_sha512_periodic<Sha512Sched>), blow-up 2, against the model and the CPU oracle's LDE; the column sum is
    the number of SCH-on rows counted from r mod 80 alone"""
    pre, ext = _periodic(ctx, 11, 1)
    want = sm.periodic(2048)
    assert np.array_equal(pre, want) and np.array_equal(ext, oracle.lde(want.reshape(1, -1), 1).reshape(-1))
    assert int(pre.sum()) == sum(1 for r in range(2048) if 15 <= r % 80 <= 78 and r != 2047) == 64 * 25 + 32


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows", [11, 12, 16, 17])
def test_sch_at_zeta_at_every_regime(ctx, oracle, log_rows):
    """N = 2048 (the first two-workgroup shape), 4096 (four workgroups; the shape of the zero-denominator tests below), 2^16 (64 workgroups,
    exactly one batch of four rows per thread) and 2^17 (two batches): the value equals the model's barycentric sum, no flag"""
    rng = np.random.default_rng(11300 + log_rows)
    zeta = tuple(int(x) for x in rng.integers(1, P, 2, dtype=np.uint64))
    assert _bary(ctx, log_rows, zeta) == list(sm.sch_at(oracle, log_rows, zeta)) + [0]


# r -> (batch slot, workgroup, SCH-on) at N = 4096: four workgroups, T = 1024 threads, thread g takes the rows g + 1024 m as slot m
ROOTS_12 = {1029: (1, 0, True), 2053: (2, 0, True), 3077: (3, 0, True), 300: (0, 1, True), 20: (0, 0, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("r", list(ROOTS_12))
def test_sch_at_zeta_zero_denominator_in_every_slot_and_workgroup(ctx, oracle, r):
    """zeta = (omega^r, 0) at N = 4096 for r = 1029, 2053, 3077 (thread 5, slots 1, 2, 3), 300 (workgroup 1: the flag reaches the fold
    through that workgroup's row of `part` alone) and 20 (workgroup 0, slot 0), every one an SCH-on row: the flag is raised"""
    assert (r // 1024, r % 1024 // 256, bool(sm.periodic(4096)[r])) == ROOTS_12[r]
    assert _bary(ctx, 12, (pow(oracle.gl_root(12), r, P), 0))[2] == 1


@pytest.mark.gpu
def test_sch_at_zeta_near_miss_and_a_small_evaluation_after_large_ones(ctx, oracle):
    """zeta = (omega^1029, 1) has the c0 of a root and is none: no flag, the value is the model's.  Then N = 2^18 fills all 64 rows of
    `part`, a flagged zeta at N = 4096 writes four of them, one with the flag, and an honest zeta at N = 512 writes row 0 alone: its result
    is the model's with flag 0 -- no stale row and no stale flag is folded"""
    near = (pow(oracle.gl_root(12), 1029, P), 1)
    assert _bary(ctx, 12, near) == list(sm.sch_at(oracle, 12, near)) + [0]
    rng = np.random.default_rng(11350)
    big = _bary(ctx, 18, tuple(int(x) for x in rng.integers(1, P, 2, dtype=np.uint64)))
    assert big[2] == 0 and all(big[:2])
    assert _bary(ctx, 12, (pow(oracle.gl_root(12), 300, P), 0))[2] == 1
    zeta = tuple(int(x) for x in rng.integers(1, P, 2, dtype=np.uint64))
    assert _bary(ctx, 9, zeta) == list(sm.sch_at(oracle, 9, zeta)) + [0]


# ---- GPU: the quotient of arbitrary columns
def _quotient_equals_the_model(ctx, oracle, log_n, log_blowup, n_proofs, cap_height, ext, hext):
    """uploads, caps, the whole quotient and gamma against the model; returns (device columns, device helper columns, the two caps, the
    model's quotient)"""
    d_cols, d_hcols = _up(ext), _up(hext)
    _, d_cap = _tree(ctx, d_cols, log_n, n_proofs * W, cap_height)
    _, d_cap_h = _tree(ctx, d_hcols, log_n, n_proofs * HC, cap_height)
    got = _down(_device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, cap_height))
    g = sm.gamma(oracle, log_n, log_blowup, cap_height, n_proofs, _down(d_cap), _down(d_cap_h))
    assert ctx.air_last_gamma() == g
    pext = oracle.lde(sm.periodic(1 << (log_n - log_blowup)).reshape(1, -1), log_blowup)
    want = sm.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, pext, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    return d_cols, d_hcols, d_cap, d_cap_h, want


@pytest.mark.gpu
@pytest.mark.parametrize("N,log_blowup,n_proofs,cap_height", [(128, 3, 17, 2), (256, 4, 3, 2), (256, 5, 1, 2), (128, 1, 1, 0), (2048, 1, 2, 2)])
def test_quotient_of_random_columns_at_every_table_size(ctx, oracle, N, log_blowup, n_proofs, cap_height):
    """random full-degree columns: a Horner chain by gamma^234 over 17 proofs, N = 256 (the wrap row N - 1 on t = 15) under blow-up 16 and
    32, cap height 0, N = 2048: d_quot and gamma equal the model word for word, guard words intact"""
    log_n = N.bit_length() - 1 + log_blowup
    rng = np.random.default_rng(11400 + 100 * log_n + 10 * log_blowup + n_proofs)
    _quotient_equals_the_model(ctx, oracle, log_n, log_blowup, n_proofs, cap_height, _random_ext(rng, n_proofs * W, log_n),
                               _random_ext(rng, n_proofs * HC, log_n))


@pytest.mark.gpu
def test_quotient_in_three_pieces_in_three_orders(ctx, oracle):
    """3 proofs at N = 256, blow-up 4, through the range call one proof at a time in the orders 0-1-2, 2-0-1 and 1-2-0: the first piece of
    an order writes (also one that does not start at proof 0), the two later ones accumulate (PIECE_ACC twice, `first` = 1 and 2 in
    gamma^(234 first)); each order equals the whole quotient, guard words intact"""
    import torch
    lb, n_proofs = 2, 3
    log_n = 8 + lb
    rng = np.random.default_rng(11450)
    ext, hext = _random_ext(rng, n_proofs * W, log_n), _random_ext(rng, n_proofs * HC, log_n)
    d_cols, d_hcols, d_cap, d_cap_h, want = _quotient_equals_the_model(ctx, oracle, log_n, lb, n_proofs, CAP_H, ext, hext)
    words = 2 << log_n
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        buf = _sentinel(words + 2 * GUARD)
        for k, lo in enumerate(order):
            d_piece = d_hcols[(lo * HC) << log_n:]
            ctx.air_sha512_sched_quotient_device(log_n, lb, CAP_H, n_proofs, d_cols.data_ptr(), d_piece.data_ptr(), d_cap.data_ptr(),
                                                 d_cap_h.data_ptr(), buf[GUARD:].data_ptr(), 0, proof_range=(lo, lo + 1), accumulate=int(k > 0))
        torch.cuda.synchronize(_dev())
        assert np.array_equal(_down(buf[GUARD:GUARD + words]), want), order
        assert torch.equal(buf[:GUARD], _sentinel(GUARD)) and torch.equal(buf[GUARD + words:], _sentinel(GUARD)), order


@pytest.mark.gpu
@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("N,log_blowup,n_proofs", [(128, 3, 2), (256, 4, 1)])
def test_quotient_of_extreme_words_equals_the_model(ctx, oracle, N, log_blowup, n_proofs, fill):
    """the inputs the NTT's lazy arithmetic is tested with, as table and helper columns of set 8's sums (32-step dbl_add, scale(carry,
    2^32), 234 accumulated terms): every word p - 1, every word 2^64 - 1, random non-canonical words, and a random choice of edge words"""
    log_n = N.bit_length() - 1 + log_blowup
    rng = np.random.default_rng(11500 + log_n)
    ext, hext = FILLS[fill](rng, (n_proofs * W, 1 << log_n)), FILLS[fill](rng, (n_proofs * HC, 1 << log_n))
    assert ext.dtype == np.uint64 and (fill == "edge words" or int(ext.min()) >= P - 1)
    _quotient_equals_the_model(ctx, oracle, log_n, log_blowup, n_proofs, CAP_H, ext, hext)


# ---- GPU: the chain and the verifier
def _prime(ctx):
    """an evaluation over 2^18 rows on the same context: all 64 rows of `part` then hold nonzero words, so a fold over the wrong number of
    rows or with the wrong row stride cannot hide behind a zeroed allocation"""
    out = _bary(ctx, 18, (0x0123456789ABCDEF % P, 0x0FEDCBA987654321 % P))
    assert out[2] == 0 and all(out[:2])


def _model_verdicts(oracle, p, caps, proof):
    """sha512_sched_model.verify with [table, H8, Q8]: [ok and holds].  Where the identity fails that is False for every query whatever
    batch_model.verify says, so its time is only spent on a proof whose identity holds"""
    if not sm.identity(oracle, p, 0, 1, caps, proof):
        return [False] * p["n_queries"]
    return sm.verify(oracle, p, 0, 1, caps, proof, _shift())


def _open_at(p):
    """{kind: word offset of column 0} of the openings of [table, H8, Q8]: column c at zeta is word c of a section, at zeta omega word
    2 R + c, R the section's row count"""
    L = bm.layout(p)
    ot, oh, oq = L["off_open"][:3]
    return {"table at zeta": ot, "table at zeta omega": ot + (2 << dm.log_r(p["n_cols"][0])), "helper at zeta": oh,
            "helper at zeta omega": oh + (2 << dm.log_r(p["n_cols"][1])), "quotient": oq}


@pytest.mark.gpu
@pytest.mark.parametrize("N,log_blowup,n_proofs", [(2048, 1, 2), (4096, 2, 1)])
def test_tiled_tables_through_the_caller_level_chain(ctx, oracle, N, log_blowup, n_proofs):
    """[table, H8, Q8] at N = 2048 (k_air_sha512_check<Sha512Sched> folds two rows of `part`) and N = 4096 (four), the edge blocks inside, after
    an evaluation that left all 64 rows nonzero: helper, gamma and quotient equal the model's, the quotient has degree <= N - 2, every
    verdict equals the model verifier's (all accept), and a proof with one bumped opening -- the last proof's W_lo at zeta, an X1 bit at
    zeta, QH_9 at zeta omega, the quotient's u_1 -- is rejected on every query by the device and the model"""
    _prime(ctx)
    table = _tiled(N, n_proofs, _edge_blocks(high_bits=False))
    c = _chain(ctx, oracle, table, log_blowup, with7=False, n_queries=3)
    assert ctx.fri_last_degree_ok() is True
    p, d_caps, got, caps = c["p"], c["d_caps"], c["proof"], _down(c["d_caps"])
    log_n, cw = p["log_n"][0], 4 << CAP_H
    help_ = sm.helper(table, n_proofs)
    assert len(_carry_facts(table, help_)[0]) == 16 and np.array_equal(c["hext"], oracle.lde(help_, log_blowup))
    g = sm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, caps[:cw], caps[cw:2 * cw])
    assert c["gamma8"] == g
    pext = oracle.lde(sm.periodic(N).reshape(1, -1), log_blowup)
    assert np.array_equal(c["quot"], sm.quotient(oracle, log_n, log_blowup, n_proofs, c["ext"], c["hext"], pext, _shift(), g))
    assert max(_degrees(oracle, c["quot"])) <= N - 2
    model = sm.verify(oracle, p, 0, 1, caps, got, _shift())
    assert all(model) and _verdicts(ctx, p, 0, 1, d_caps, got) == model
    at, last = _open_at(p), n_proofs - 1
    for name, word in (("table at zeta", last * W + sm.W_), ("helper at zeta", last * HC + sm.HX1 + 41),
                       ("helper at zeta omega", last * HC + sm.HQH + 9), ("quotient", 1)):
        bad = _bumped(got, at[name] + word)
        model = _model_verdicts(oracle, p, caps, bad)
        assert not any(model) and _verdicts(ctx, p, 0, 1, d_caps, bad) == model, name


def _chain_on_device(ctx, table, log_blowup, n_queries):
    """the chain [table, H8, Q8] with nothing downloaded but the caps and the proof: (params, d_caps, proof words)"""
    import torch
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    log_n = log_rows + log_blowup
    d_table, d_help = _up(table), _device_helper(ctx, table)
    d_ext, d_hext = _sentinel((n_proofs * W) << log_n), _sentinel((n_proofs * HC) << log_n)
    ctx.lde_device(log_rows, log_blowup, n_proofs * W, d_table.data_ptr(), d_ext.data_ptr(), 0)
    ctx.lde_device(log_rows, log_blowup, n_proofs * HC, d_help.data_ptr(), d_hext.data_ptr(), 0)
    d_lv_t, d_cap_t = _tree(ctx, d_ext, log_n, n_proofs * W)
    d_lv_h, d_cap_h = _tree(ctx, d_hext, log_n, n_proofs * HC)
    d_quot = _device_quotient(ctx, log_n, log_blowup, n_proofs, d_ext, d_hext, d_cap_t, d_cap_h)
    d_lv_q, d_cap_q = _tree(ctx, d_quot, log_n, 2)
    p = bparams([log_n] * 3, [n_proofs * W, n_proofs * HC, 2], CAP_H, log_blowup, 2, 2, n_queries)
    d_cols, d_lvs = [d_ext, d_hext, d_quot], [d_lv_t, d_lv_h, d_lv_q]
    proof = _guarded(bm.layout(p)["words"], lambda out: ctx.batch_prove_device(p, [d.data_ptr() for d in d_cols], [d.data_ptr() for d in d_lvs], out, 0))
    assert ctx.fri_last_degree_ok() is True
    return p, torch.cat([d_cap_t, d_cap_h, d_cap_q]), _down(proof)


@pytest.mark.gpu
def test_full_size_table_through_the_check_kernel(ctx, oracle):
    """N = 2^15, the real size of T.2 (409 full blocks; k_air_sha512_check<Sha512Sched> folds 32 rows of `part`, primed by a 2^18 evaluation),
    blow-up 2, one proof, two queries; the extended helper (121 MB) never leaves the device.  The model's identity, which needs the caps
    and the openings alone, holds and the device accepts both queries; a bumped table opening and a bumped helper opening fail the identity
    and are rejected on both queries"""
    _prime(ctx)
    table = _tiled(1 << 15, 1, _edge_blocks(high_bits=False))
    p, d_caps, got = _chain_on_device(ctx, table, 1, 2)
    caps = _down(d_caps)
    assert sm.identity(oracle, p, 0, 1, caps, got)
    assert _verdicts(ctx, p, 0, 1, d_caps, got) == [True, True]
    at = _open_at(p)
    for word in (at["table at zeta omega"] + sm.W_ + 1, at["helper at zeta"] + sm.HG1):
        bad = _bumped(got, word)
        assert not sm.identity(oracle, p, 0, 1, caps, bad)
        assert _verdicts(ctx, p, 0, 1, d_caps, bad) == [False, False]


# n_proofs -> (log_r of the table's openings plane, log_r of the helper's)
PLANES = {4: (7, 10), 5: (7, 11), 7: (7, 11), 8: (8, 11), 9: (8, 12)}


@pytest.mark.gpu
@pytest.mark.parametrize("n_proofs", list(PLANES))
def test_openings_planes_of_4_to_9_proofs(ctx, oracle, n_proofs):
    """N = 128, blow-up 2, two queries: the table's openings plane grows between 7 and 8 proofs (126 -> 128, 144 -> 256 rows), the
    helper's between 4 and 5 (920 -> 1024, 1150 -> 2048) and between 8 and 9 (1840 -> 2048, 2070 -> 4096), ZetaView's strides: the honest
    proof is accepted, a bump in the last proof's last helper column and one in its W_hi are rejected, as the model's identity has it"""
    _prime(ctx)
    p, d_caps, got = _chain_on_device(ctx, _tiled(128, n_proofs), 1, 2)
    assert (dm.log_r(p["n_cols"][0]), dm.log_r(p["n_cols"][1])) == PLANES[n_proofs]
    caps = _down(d_caps)
    assert sm.identity(oracle, p, 0, 1, caps, got) and _verdicts(ctx, p, 0, 1, d_caps, got) == [True, True]
    at = _open_at(p)
    for word in (at["helper at zeta"] + n_proofs * HC - 1, at["table at zeta"] + (n_proofs - 1) * W + sm.W_ + 1):
        bad = _bumped(got, word)
        assert not sm.identity(oracle, p, 0, 1, caps, bad)
        assert _verdicts(ctx, p, 0, 1, d_caps, bad) == [False, False]


# What the identity does NOT read, written out from include/tmx.h "the message schedule of the SHA-512 table": of the table it reads W_lo
# and W_hi alone, at both points; of the helper all 230 columns at zeta, and at zeta omega G0, G1 (192 .. 195) and QL_k, QH_k (196 .. 225)
NOT_READ = ({("table at zeta", c) for c in range(2, 18)} | {("table at zeta omega", c) for c in range(2, 18)}
            | {("helper at zeta omega", c) for c in [*range(0, 192), 226, 227, 228, 229]})


@pytest.mark.gpu
def test_which_openings_the_identity_reads(ctx, oracle):
    """N = 128, two proofs, blow-up 2: each of the 36 table openings and the 460 helper openings of proof 1 (every column at zeta and at
    zeta omega) bumped in turn.  For every bump the device verdicts equal the model verifier's (all reject: a changed opening fails the
    batch proof even where the identity does not read it), and the set of bumps after which the model's identity still holds is exactly
    NOT_READ: the sixteen columns that are not W at both points, and WB, X0, X1, CL, CH at zeta omega"""
    _prime(ctx)
    p, d_caps, got = _chain_on_device(ctx, _tiled(128, 2), 1, 2)
    caps = _down(d_caps)
    assert sm.identity(oracle, p, 0, 1, caps, got) and _verdicts(ctx, p, 0, 1, d_caps, got) == [True, True]
    at = _open_at(p)
    bumps = [(where, c) for where, n in (("table at zeta", W), ("table at zeta omega", W), ("helper at zeta", HC), ("helper at zeta omega", HC))
             for c in range(n)]
    holds = set()
    for where, c in bumps:
        bad = _bumped(got, at[where] + (HC if where.startswith("helper") else W) + c)
        if sm.identity(oracle, p, 0, 1, caps, bad):
            holds.add((where, c))
            model = sm.verify(oracle, p, 0, 1, caps, bad, _shift())
        else:
            model = [False, False]
        assert _verdicts(ctx, p, 0, 1, d_caps, bad) == model, (where, c)
    print(f"\n[sha512-sched shapes] {len(bumps)} bumps, the identity still holds after {len(holds)} of them")
    assert holds == NOT_READ and len(NOT_READ) == 16 + 16 + 196


# ---- GPU: the set level and the scratch
LADDERS, LADDERS_QUOTIENT = 1, 64


def _set_round(c, kind, n_proofs, lb, tr, sections=SHA512, queries=3, before=None, after=None, calls="8"):
    """commit `sections`, before(), the air calls of `calls` ("1": the ladders', "8": set 8's on SHA512) in that order, after(), one
    proof.  Returns (params, the sections in oracle order, the caps in that order on the device, proof words, set 8's gamma)"""
    import torch
    cw = 4 << CAP_H
    d_caps = _sentinel(bin(sections).count("1") * cw)
    d_cap_q1, d_cap_h, d_cap_q = _sentinel(cw), _sentinel(cw), _sentinel(cw)
    c.trace_commit_set_device(kind, n_proofs, sections, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
    _, order0 = c.trace_commit_set_shape()
    gamma = None
    try:
        if before:
            before()
        for s in calls:
            if s == "1":
                c.trace_commit_set_air_device(d_cap_q1.data_ptr(), 0)
            else:
                c.trace_commit_set_air_sha512_sched_device(SHA512, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
                gamma = c.air_last_gamma()
    finally:
        if after:
            after()
    shape, order = c.trace_commit_set_shape()
    k = order.index(SHA512)
    assert order[k:k + 3] == [SHA512, HELPER, QUOTIENT] and shape["n_cols"][k:k + 3] == [n_proofs * W, n_proofs * HC, 2]
    p = dict(shape, arity_bits=2, final_log_max=2, n_queries=queries, pow_bits=0)
    proof = _down(_guarded(bm.layout(p)["words"], lambda out: c.trace_commit_set_prove_device(p, out, 0)))
    assert c.fri_last_degree_ok() is True
    caps_of = {s: d_caps[cw * i:cw * (i + 1)] for i, s in enumerate(order0)}
    caps_of.update({HELPER: d_cap_h, QUOTIENT: d_cap_q, LADDERS_QUOTIENT: d_cap_q1})
    return p, order, torch.cat([caps_of[s] for s in order]), proof, gamma


def _set_8_holds(c, oracle, p, order, d_caps, proof):
    """the device verifier accepts every query, the model's identity holds, and a bumped quotient opening is rejected on every query"""
    k = order.index(SHA512)
    assert _verdicts(c, p, k, k + 1, d_caps, proof) == [True] * p["n_queries"]
    assert sm.identity(oracle, p, k, k + 1, _down(d_caps), proof)
    bad = _bumped(proof, bm.layout(p)["off_open"][k + 2])
    assert not any(_verdicts(c, p, k, k + 1, d_caps, bad))
    return bad


@pytest.mark.gpu
def test_set_level_on_the_skip_kind(built_lib, oracle):
    """kind 0, N = 4 (T.2 has 640 rows, so N = 1024), blow-up 4, a set SHA512 | HEADER on a two-proof context with one proof and then
    two: caps, gamma and proof words equal the caller-level chain's on the same columns (the header table as one more oracle); the device
    verifier accepts and rejects a bumped quotient opening"""
    import torch
    import tendermintx_amd as tmx
    from test_merkle_open import _oracle_ext, _trace_rows
    kind, n, lb = 0, 4, 2
    with tmx.Context(n, b"celestia", max_batch=2) as c:
        tr = _trace_rows(c, kind, n, 2, 11610)
        traces = _down(tr)
        for n_proofs in (1, 2):
            p, order, d_caps, proof, gamma = _set_round(c, kind, n_proofs, lb, tr, SHA512 | HEADER)
            k, kh = order.index(SHA512), order.index(HEADER)
            assert p["log_n"][k] == 10 + lb and sorted(order) == sorted([SHA512, HELPER, QUOTIENT, HEADER])
            table = _columns(list(traces[:n_proofs]), kind, n)
            e, lm, nc = _oracle_ext(oracle, kind, n, traces[:n_proofs], HEADER, lb)
            ch = _chain(c, oracle, table, lb, with7=False, n_queries=3, others=[(kh, e.reshape(nc, -1))])
            assert {key: ch["p"][key] for key in ("log_n", "n_cols")} == {key: p[key] for key in ("log_n", "n_cols")}
            assert gamma == ch["gamma8"] and torch.equal(d_caps, ch["d_caps"]), n_proofs
            assert np.array_equal(proof, ch["proof"]), n_proofs
            _set_8_holds(c, oracle, p, order, d_caps, proof)


@pytest.mark.gpu
def test_the_ladders_quotient_beside_set_8(built_lib, oracle):
    """a set LADDERS | SHA512 of skip N = 4, one proof, blow-up 2: set 8's tables live inside set 1's table scratch, so the two air calls
    are made in both orders on fresh commits.  Both orders give the same shape, caps and proof words; the ladders' verifier and set 8's
    both accept; a bumped set-8 quotient opening fails set 8's verifier and identity and leaves the ladders' identity holding"""
    import torch
    import tendermintx_amd as tmx
    import test_air as ta
    from test_merkle_open import _trace_rows
    with tmx.Context(4, b"celestia", max_batch=1) as c:
        tr = _trace_rows(c, 0, 4, 1, 11620)
        runs = [_set_round(c, 0, 1, 1, tr, LADDERS | SHA512, calls=way) for way in ("18", "81")]
        (p, order, d_caps, proof, gamma), (p_b, order_b, d_caps_b, proof_b, gamma_b) = runs
        assert (p, order, gamma) == (p_b, order_b, gamma_b) and torch.equal(d_caps, d_caps_b) and np.array_equal(proof, proof_b)
        kl, k = order.index(LADDERS), order.index(SHA512)
        assert order[kl + 1] == LADDERS_QUOTIENT and len(order) == 5
        caps = _down(d_caps)
        assert all(ta._verdicts(c, p, kl, d_caps, proof)) and am.identity(oracle, p, kl, caps, proof)
        bad = _set_8_holds(c, oracle, p, order, d_caps, proof)
        assert not sm.identity(oracle, p, k, k + 1, caps, bad) and am.identity(oracle, p, kl, caps, bad)


@pytest.mark.gpu
def test_the_domain_moved_between_the_commit_and_the_call(step2_rows, oracle):
    """tmx_ntt_set_domain (g = 7) between the commit and set 8's call, the default back behind the call: the helper AND the SCH plane are
    extended under the set's domain, so caps, gamma and proof equal the unmoved run's and the verifier accepts"""
    import torch
    c, tr = step2_rows
    want = _set_round(c, 1, 2, 1, tr)
    try:
        got = _set_round(c, 1, 2, 1, tr, before=lambda: c.ntt_set_domain(*oracle.G7_DOMAIN), after=lambda: c.ntt_set_domain(*oracle.PLONKY2_DOMAIN))
    finally:
        c.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
    assert got[:2] == want[:2] and got[4] == want[4]
    assert torch.equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    _set_8_holds(c, oracle, *got[:4])


@pytest.mark.gpu
def test_a_verifier_call_first_on_a_fresh_context(ctx, oracle):
    """a proof over [table, H8, Q8] at N = 2048 (two rows of `part`) made on the module's context; then on a fresh context, whose d_air8
    is unallocated: the verifier first (sha512_scratch allocates the rows of `part` alone), a caller-level quotient at (128, 2) that grows
    d_air8 (freed and allocated anew) and equals the model, and the verifier again.  Every verdict equals the model's: the honest proof
    accepted on every query, one with a bumped helper opening rejected, before and after the growth"""
    import tendermintx_amd as tmx
    table = _tiled(2048, 1, _edge_blocks(high_bits=False))
    p, d_caps, got = _chain_on_device(ctx, table, 1, 2)
    caps = _down(d_caps)
    bad = _bumped(got, _open_at(p)["helper at zeta omega"] + sm.HQL + 15)
    honest, broken = _model_verdicts(oracle, p, caps, got), _model_verdicts(oracle, p, caps, bad)
    assert honest == [True, True] and broken == [False, False]
    rng = np.random.default_rng(11640)
    with tmx.Context(2, b"celestia", max_batch=2) as c:
        assert _verdicts(c, p, 0, 1, d_caps, got) == honest and _verdicts(c, p, 0, 1, d_caps, bad) == broken
        _quotient_equals_the_model(c, oracle, 8, 1, 1, CAP_H, _random_ext(rng, W, 8), _random_ext(rng, HC, 8))
        assert _verdicts(c, p, 0, 1, d_caps, got) == honest and _verdicts(c, p, 0, 1, d_caps, bad) == broken


@pytest.mark.gpu
def test_a_set_of_the_moved_domain_called_from_the_default_one(step2_rows, oracle):
    """the other way round: the set committed under g = 7, the context put back to the default domain between the commit and set 8's call
    and to g = 7 again behind it.  SCH is extended under the SET's domain (a plane extended under the default one is no low-degree column
    on that set's coset): the degree flag holds, caps, gamma and proof equal those of the run that stays under g = 7 throughout, and the
    verifier, under g = 7, accepts as the model's identity holds"""
    import torch
    c, tr = step2_rows
    try:
        c.ntt_set_domain(*oracle.G7_DOMAIN)
        oracle.ntt_set_domain(*oracle.G7_DOMAIN)
        want = _set_round(c, 1, 2, 1, tr)
        got = _set_round(c, 1, 2, 1, tr, before=lambda: c.ntt_set_domain(*oracle.PLONKY2_DOMAIN), after=lambda: c.ntt_set_domain(*oracle.G7_DOMAIN))
        assert got[:2] == want[:2] and got[4] == want[4]
        assert torch.equal(got[2], want[2]) and np.array_equal(got[3], want[3])
        _set_8_holds(c, oracle, *got[:4])
    finally:
        c.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
        oracle.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
