"""The set-7 kernels (tendermintx_amd/csrc/air.hip k_air_sha512_helper, k_air_sha512_periodic<Sha512Round>, k_air_sha512_periodic_eval<Sha512Round>, k_air_sha512_tables<Sha512Round>,
k_air_sha512_quotient<Sha512Round, FORM>, k_air_sha512_check<Sha512Round>) and their host paths (api.cpp sha_pass, sha_verify_call, sha_set_call under has_periodic,
sha512_scratch) at every shape and row value they branch on: a verifier that folds 2, 4 and 32 rows of the barycentric kernel's `part`,
the rows-per-thread regimes of that kernel and a zero denominator in every batch slot and in workgroups other than 0, LIVE from each of the
eighteen limbs alone, the extreme carries and the carry columns on SEL-off rows, N = 128 and blow-up 64 in the quotient, three pieces in
three orders, the extreme words of the lazy field arithmetic, the set of openings the identity reads, 7 and 8 proofs' openings planes,
k_trace = 1, the skip kind, set 1 beside set 7, a moved NTT domain, and growth and reuse of d_air7 on one context.  The yardstick stays
tests/sha512_air_model.py on tests/batch_model.py: device words equal the model's word for word, every device verdict equals the model's,
guard words stay intact.  The helpers and fixtures are those of tests/test_sha512_air.py and tests/test_sha_air.py; docs/kernels.md "set 7:
which test reaches which shape" is the map."""
import numpy as np
import pytest

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha512_air_model as sm
from batch_model import bparams
from test_fri import _down, _sentinel, _shift, _up
from test_sha512_air import (CAP_H, HC, HEADER, HELPER, QUOTIENT, SHA512, W, _chain, _columns, _device_helper, _device_quotient,  # noqa: F401
                             _model_quotient, _verdicts, ctx, skip4, step2, step3)
from test_sha_air import GUARD, _cap, _degrees, _dev, _guarded, _random_ext, _refused, _tree
from test_sha_air_shapes import FILLS, _bumped, _openings, _Remembering

P = fm.P
BLOCK = sm.BLOCK


# ---- honest tables of any size
@pytest.fixture(scope="module")
def live_blocks(skip4, step2, step3):
    """[n][18][80]: every 80-row block of the CPU oracle's T.2 rows (skip N = 4, step N = 2, step N = 3, two proofs each) whose first row
    is not zero"""
    out = []
    for table in (skip4, step2, step3):
        for p in range(table.shape[0] // W):
            t = table[p * W:(p + 1) * W]
            out += [t[:, BLOCK * b:BLOCK * b + BLOCK] for b in range(t.shape[1] // BLOCK) if t[:, BLOCK * b].any()]
    out = np.stack(out)
    assert len(out) >= 8 and int(out.max()) < 1 << 32
    return out


def _tiled(live_blocks, N, n_proofs):
    """[18 n_proofs][N] pre-LDE columns: the live blocks in turn, every seventh block of the tiling all zero; the rows behind the last full
    block (N is no multiple of 80) hold the first rows of a live block in even proofs and zero padding in odd ones.  A block's 79
    transitions are honest and the seam rows and row N - 1 are unselected, so every tiling satisfies the set."""
    nb, tail = divmod(N, BLOCK)
    table = np.zeros((n_proofs * W, N), dtype=np.uint64)
    for g in range(n_proofs * nb):
        if g % 7 != 6:
            p, b = divmod(g, nb)
            table[p * W:(p + 1) * W, BLOCK * b:BLOCK * b + BLOCK] = live_blocks[(g - g // 7) % len(live_blocks)]
    for p in range(0, n_proofs, 2):
        table[p * W:(p + 1) * W, BLOCK * nb:] = live_blocks[(p + 3) % len(live_blocks)][:, :tail]
    return table


@pytest.mark.parametrize("N,n_proofs", [(128, 5), (2048, 1)])
def test_tiled_tables_satisfy_the_constraints_as_integers(live_blocks, N, n_proofs):
    """the tiling at N = 128 (one full block and a 48-row partial one per proof, live in proofs 0, 2, 4 and zero in 1, 3) and N = 2048
    (25 full blocks, three of them zero, and a live 48-row partial one): all 628 constraints are integer identities on every row"""
    print(f"\n[sha512-air shapes] {len(live_blocks)} live blocks")
    table = _tiled(live_blocks, N, n_proofs)
    help_ = sm.helper(table, n_proofs)
    live = help_[sm.HLIVE::HC]
    assert live[0, -1] == 1 and (live[:, -1] == 0).any() == (n_proofs > 1) and (N == 128 or not live[0, :BLOCK * (N // BLOCK)].all())
    for p in range(n_proofs):
        for j, c in enumerate(sm.integer_residuals(table[p * W:(p + 1) * W], help_[p * HC:(p + 1) * HC])):
            assert not c.any(), (p, j, np.flatnonzero(c)[:4])


def test_tiled_quotient_has_degree_at_most_n_minus_2_and_the_identity_holds(oracle, live_blocks):
    """N = 128, 3 proofs, blow-up 4: the model quotient interpolates to degree <= N - 2 in both planes; the identity holds on a
    tests/batch_model.py proof over [table, helper, quotient] and fails after one helper opening of proof 2 is bumped"""
    N, n_proofs, lb = 128, 3, 2
    oracle = _Remembering(oracle)
    table = _tiled(live_blocks, N, n_proofs)
    ext, hext, g, quot = _model_quotient(oracle, table, sm.helper(table, n_proofs), lb)
    deg = _degrees(oracle, quot)
    print(f"\n[sha512-air shapes] N = {N}, {n_proofs} proofs: quotient degrees {deg}")
    assert max(deg) <= N - 2
    log_n = 7 + lb
    p = bparams([log_n] * 3, [n_proofs * W, n_proofs * HC, 2], CAP_H, lb, 2, 2, 1)
    cols = [ext, hext, quot.reshape(2, -1)]
    caps = np.concatenate([_cap(oracle, c, log_n) for c in cols])
    proof, degree_ok, _, _ = bm.prove(oracle, p, cols, _shift())
    assert degree_ok and sm.identity(oracle, p, 0, caps, proof)
    at = bm.layout(p)["off_open"][1] + 2 * HC + sm.HE + 41
    proof[at] = np.uint64((int(proof[at]) + 1) % P)
    assert not sm.identity(oracle, p, 0, caps, proof)


# ---- the edge blocks of the helper's definition
N_EDGE, ONES = 23, 20  # (ONES: the all-ones block's place in the list)


def _edge_blocks(rng):
    """[(block [18][80], LIVE)] x 23: eighteen blocks whose first row is nonzero in the low half of exactly limb c, c = 0 .. 17, under
    random high halves and random rows below (LIVE = 1: each limb alone raises it); a first row nonzero only in high halves (LIVE = 0); a
    block nonzero only below its first row (LIVE = 0); all low halves 0xFFFFFFFF under random high halves (every word of the round is
    2^64 - 1: the largest carries); a live block whose operands are all zero except W_0 = 1 (every carry 0 on a live row); and a block
    whose only nonzero word is h of row 0, chosen so that both high-limb sums of that row are 2^32 - 1 before the low limb's carry comes
    in and both low-limb sums carry 1 (CAH = CEH = 1 through CAL and CEL alone: in the all-ones block a high-limb sum reaches its
    carry with or without the one from below, and under random words the two differ once in 2^30 rows)"""
    hi = np.uint64(0xFFFFFFFF00000000)
    rand = lambda: rng.integers(0, 1 << 64, (W, BLOCK), dtype=np.uint64)
    out = []
    for c in range(W):
        b = rand()
        b[:, 0] &= hi
        b[c, 0] |= np.uint64(1 << (c + 3))
        out.append((b, 1))
    high_only = rand()
    high_only[:, 0] = (high_only[:, 0] & hi) | np.uint64(1 << 32)
    below = rand()
    below[:, 0] = 0
    ones = rand() | np.uint64(0xFFFFFFFF)
    w0 = np.zeros((W, BLOCK), dtype=np.uint64)
    w0[sm.W_, 0] = 1
    carry_in = np.zeros((W, BLOCK), dtype=np.uint64)
    carry_in[sm.H_, 0], carry_in[sm.H_ + 1, 0] = 0xFFFFFFFF, 0xFFFFFFFF - (sm.K512[1] >> 32)
    out += [(high_only, 0), (below, 0), (ones, 1), (w0, 1), (carry_in, 1)]
    assert len(out) == N_EDGE and out[ONES][0] is ones
    return out


def _carry_edges(help_):
    """(largest of CAL and CAH, largest of CEL and CEH, smallest carry on a SEL-on row of a live block, largest carry on a SEL-off row)"""
    sel = sm.periodic(help_.shape[1])[0].astype(bool)
    c = np.stack([help_[at::HC] + 2 * help_[at + 1::HC] + 4 * help_[at + 2::HC] for at in (sm.HCAL, sm.HCAH, sm.HCEL, sm.HCEH)])
    on = help_[sm.HLIVE::HC].astype(bool) & sel
    return int(c[:2].max()), int(c[2:].max()), int(c[:, on].min()), int(c[:, :, ~sel].max())


def test_edge_blocks_reach_the_carry_extremes():
    """the 23 edge blocks as blocks 0 .. 22 of one proof of 2048 rows, random blocks behind them and the first rows of the all-ones block
    as the partial block (so row N - 1 and the seam row 79 of the all-ones block stand under operands that would carry): LIVE is the
    expected one, max(CAL, CAH) = 6, max(CEL, CEH) = 5, the smallest carry on a SEL-on row of a live block is 0, and all twelve carry
    bits are 0 on every SEL-off row; on row 0 of the carry-in block all four carries are 1 and the high-limb sums are 2^32 - 1 without
    the carry from below"""
    rng = np.random.default_rng(9900)
    edges = _edge_blocks(rng)
    N, nb = 2048, 2048 // BLOCK
    table = rng.integers(0, 1 << 64, (W, N), dtype=np.uint64)
    live = np.ones(nb + 1, dtype=np.uint64)
    for b, (block, lv) in enumerate(edges):
        table[:, BLOCK * b:BLOCK * b + BLOCK] = block
        live[b] = lv
    table[:, BLOCK * nb:] = edges[ONES][0][:, :N - BLOCK * nb]
    help_ = sm.helper(table, 1)
    assert np.array_equal(help_[sm.HLIVE], np.repeat(live, BLOCK)[:N]) and int((live == 0).sum()) == 2
    assert _carry_edges(help_) == (6, 5, 0, 0)
    ones_at, carry_at = BLOCK * ONES, BLOCK * (N_EDGE - 1)
    assert help_[sm.HCAL:sm.HCAL + 12, ones_at + 78].any() and not help_[sm.HCAL:sm.HCAL + 12, ones_at + 79].any()
    assert [int(help_[at + k, carry_at]) for at in (sm.HCAL, sm.HCAH, sm.HCEL, sm.HCEH) for k in range(3)] == [1, 0, 0] * 4
    assert int(table[sm.H_ + 1, carry_at]) + (sm.K512[1] >> 32) == 0xFFFFFFFF and not table[sm.W_:sm.H_, carry_at:carry_at + 2].any()


# ---- GPU: the helper
@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs", [(7, 3), (7, 5), (7, 257), (8, 1), (11, 2), (12, 1)])
def test_helper_at_every_grid_shape_equals_the_model(ctx, log_rows, n_proofs):
    """random 64-bit words from 128 rows per proof (the grid's last workgroup half filled at 3 and 5 proofs, 129 workgroups at 257) over
    256 rows (one workgroup; the real size of step N = 1) to 4096; at log_rows >= 11 the even blocks and the last full block of every proof
    are zero.  At (7, 5) the five edge blocks that are not one-limb blocks are block 0 of proofs 0 .. 4 and the all-ones block's first rows
    the partial block of proof 0; at (11, 2) all 23 are planted, the all-ones rows again as a partial block.  The helper equals the model's
    word for word, guard words intact; the LIVE column is the expected one; the carry bits are 0 on every SEL-off row, and where the edge
    blocks are planted CA = 6, CE = 5 and a carry of 0 on a live SEL-on row occur in the device's words"""
    rng = np.random.default_rng(9500 + 10 * log_rows + n_proofs)
    N = 1 << log_rows
    nb = N // BLOCK
    table = rng.integers(0, 1 << 64, (n_proofs * W, N), dtype=np.uint64)
    live = np.ones((n_proofs, nb + 1), dtype=np.uint64)

    def put(p, b, block, lv):
        table[p * W:(p + 1) * W, BLOCK * b:BLOCK * b + BLOCK] = block
        live[p, b] = lv
    if log_rows >= 11:
        for p in range(n_proofs):
            for b in [*range(0, nb, 2), nb - 1]:
                put(p, b, 0, 0)
    planted = (log_rows, n_proofs) in ((7, 5), (11, 2))
    if planted:
        edges = _edge_blocks(rng)
        ones = edges[ONES][0]
        if log_rows == 7:
            where, edges, tail_of = [(p, 0) for p in range(5)], edges[W:], 0
        else:
            where, tail_of = [(0, b) for b in range(13)] + [(1, b) for b in range(5, 15)], 1
        assert len(where) == len(edges)
        for (p, b), (block, lv) in zip(where, edges):
            put(p, b, block, lv)
        table[tail_of * W:(tail_of + 1) * W, BLOCK * nb:] = ones[:, :N - BLOCK * nb]
    got = _down(_device_helper(ctx, table)).reshape(n_proofs * HC, -1)
    want = sm.helper(table, n_proofs)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    expected = np.repeat(live, BLOCK, axis=1)[:, :N]
    assert np.array_equal(want[sm.HLIVE::HC], expected) and np.array_equal(got[sm.HLIVE::HC], expected)
    edges_seen = _carry_edges(got)
    print(f"\n[sha512-air shapes] helper ({log_rows}, {n_proofs}): {int((live == 0).sum())} of {live.size} blocks with LIVE = 0, carries {edges_seen}")
    assert edges_seen[3] == 0 and (not planted or edges_seen == (6, 5, 0, 0))


# ---- GPU: the preprocessed columns
def _periodic(ctx, log_rows, log_blowup):
    import torch
    N, M = 1 << log_rows, 1 << (log_rows + log_blowup)
    d_pre, d_ext = _sentinel(3 * N + GUARD), _sentinel(3 * M + GUARD)
    ctx.air_sha512_periodic_device(log_rows, log_blowup, d_pre.data_ptr(), d_ext.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(d_pre[3 * N:], _sentinel(GUARD)) and torch.equal(d_ext[3 * M:], _sentinel(GUARD))
    return _down(d_pre[:3 * N]).reshape(3, N), _down(d_ext[:3 * M]).reshape(3, M)


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,log_blowup", [(7, 6), (8, 2), (11, 1)])
def test_preprocessed_columns_at_the_edge_sizes(ctx, oracle, log_rows, log_blowup):
    """SEL, KLO, KHI at N = 128 under blow-up 64, N = 256 (one workgroup of k_air_sha512_periodic<Sha512Round> exactly) and N = 2048 (eight), against the
    model and the CPU oracle's LDE"""
    pre, ext = _periodic(ctx, log_rows, log_blowup)
    want = sm.periodic(1 << log_rows)
    assert np.array_equal(pre, want) and np.array_equal(ext, oracle.lde(want, log_blowup))
    N = 1 << log_rows
    assert want[0].sum() == N - N // BLOCK - 1


@pytest.mark.gpu
def test_preprocessed_columns_extend_under_the_current_domain(ctx, oracle):
    """after tmx_ntt_set_domain (g = 7) the three planes are extended under that domain: the CPU oracle's LDE under it, which differs from
    the default domain's; the columns before the LDE do not depend on the domain"""
    log_rows, lb = 8, 2
    want = sm.periodic(1 << log_rows)
    default = oracle.lde(want, lb)
    try:
        ctx.ntt_set_domain(*oracle.G7_DOMAIN)
        oracle.ntt_set_domain(*oracle.G7_DOMAIN)
        pre, ext = _periodic(ctx, log_rows, lb)
        moved = oracle.lde(want, lb)
    finally:
        ctx.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
        oracle.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
    assert np.array_equal(pre, want) and np.array_equal(ext, moved) and not np.array_equal(moved, default)
    assert np.array_equal(_periodic(ctx, log_rows, lb)[1], default)


# ---- GPU: the barycentric kernel
def _bary(ctx, log_rows, zeta_words):
    """the seven words of tmx_air_sha512_periodic_eval_device at the two words of zeta as given; the words behind them stay untouched"""
    import torch
    d_zeta, d_out = _up(np.array(zeta_words, dtype=np.uint64)), _sentinel(7 + GUARD)
    ctx.air_sha512_periodic_eval_device(log_rows, d_zeta.data_ptr(), d_out.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(d_out[7:], _sentinel(GUARD))
    return [int(x) for x in _down(d_out[:7])]


def _bary_model(oracle, log_rows, zeta):
    return [w[k] for w in sm.barycentric(oracle, log_rows, zeta) for k in (0, 1)] + [0]


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows", [8, 11, 12, 16, 17])
def test_barycentric_values_at_every_regime(ctx, oracle, log_rows):
    """N = 256 (one workgroup, one row per thread: batch slots 1 - 3 all out of range), 2048 (the first two-workgroup shape), 4096 (four
    workgroups; the shape of the zero-denominator tests below), 2^16 (64 workgroups, exactly one batch of four rows per thread) and 2^17
    (two batches): the three values equal the model's barycentric sums, no flag"""
    rng = np.random.default_rng(9600 + log_rows)
    zeta = tuple(int(x) for x in rng.integers(1, P, 2, dtype=np.uint64))
    assert _bary(ctx, log_rows, zeta) == _bary_model(oracle, log_rows, zeta)


ROOTS_12 = {"row 0": 0, "slot 1": 5 + 1024, "slot 2": 5 + 2 * 1024, "slot 3": 5 + 3 * 1024, "workgroup 1, slot 0": 300, "row N - 1": 4095}


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(ROOTS_12))
def test_barycentric_zero_denominator_in_every_slot_and_workgroup(ctx, oracle, which):
    """N = 4096: four workgroups, T = 1024 threads, thread g takes the rows g, g + 1024, g + 2048, g + 3072 as the four slots of one
    batch.  zeta = (omega^r, 0) for r = 0 (workgroup 0, slot 0), 1029, 2053, 3077 (thread 5, slots 1, 2, 3), 300 (workgroup 1: the flag
    reaches the fold through that workgroup's part[6] alone) and 4095 (workgroup 3, slot 3): the flag is raised for each"""
    r = ROOTS_12[which]
    assert (r // 1024, r % 1024 // 256) == {"row 0": (0, 0), "slot 1": (1, 0), "slot 2": (2, 0), "slot 3": (3, 0), "workgroup 1, slot 0": (0, 1),
                                            "row N - 1": (3, 3)}[which]
    assert _bary(ctx, 12, (pow(oracle.gl_root(12), r, P), 0))[6] == 1


@pytest.mark.gpu
def test_barycentric_near_miss_and_non_canonical_zeta(ctx, oracle):
    """zeta = (omega^1029, 1) has the c0 of a root and is none: no flag, the three values are the model's.  The words (z0 + p, z1 + p) of a
    zeta with z0, z1 < 2^31 give the same seven words as (z0, z1), at an honest point and at a root"""
    near = (pow(oracle.gl_root(12), 5 + 1024, P), 1)
    assert _bary(ctx, 12, near) == _bary_model(oracle, 12, near)
    z = (0x12345678, 0x7ABCDEF1)
    want = _bary_model(oracle, 12, z)
    assert _bary(ctx, 12, z) == want and _bary(ctx, 12, (z[0] + P, z[1] + P)) == want
    assert _bary(ctx, 12, (1 + P, P))[6] == 1  # (omega^0 = 1, 0) in non-canonical words


@pytest.mark.gpu
def test_barycentric_small_evaluation_after_a_64_part_one(ctx, oracle):
    """N = 2^18 fills all 64 rows of `part`; the flagged zeta at N = 4096 then writes four of them, one with the flag; an honest zeta at
    N = 512 writes row 0 alone: its result is the model's with flag 0 -- no stale row and no stale flag is folded"""
    rng = np.random.default_rng(9650)
    big = _bary(ctx, 18, tuple(int(x) for x in rng.integers(1, P, 2, dtype=np.uint64)))
    assert big[6] == 0 and all(big[:6])
    assert _bary(ctx, 12, (pow(oracle.gl_root(12), 300, P), 0))[6] == 1
    zeta = tuple(int(x) for x in rng.integers(1, P, 2, dtype=np.uint64))
    assert _bary(ctx, 9, zeta) == _bary_model(oracle, 9, zeta)


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
    pext = oracle.lde(sm.periodic(1 << (log_n - log_blowup)), log_blowup)
    want = sm.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, pext, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    return d_cols, d_hcols, d_cap, d_cap_h, want


@pytest.mark.gpu
@pytest.mark.parametrize("N,log_blowup,n_proofs,cap_height", [(128, 1, 1, 0), (128, 6, 2, 2), (128, 3, 17, 2), (256, 4, 3, 2), (256, 5, 1, 2),
                                                              (2048, 2, 1, 2), (128, 1, 1, 9)])
def test_quotient_of_random_columns_at_every_table_size(ctx, oracle, N, log_blowup, n_proofs, cap_height):
    """random full-degree columns: N = 128 (the smallest table) up to N = 2048, blow-up 64 (all 64 entries of the 1 / (x^N - 1) table, the
    bound of AIR7_TAB_WORDS), a Horner chain over 17 proofs, cap height 0 and a cap that is the whole leaf level (gamma absorbs 2 x 1024
    words): d_quot and gamma equal the model word for word, guard words intact"""
    log_n = N.bit_length() - 1 + log_blowup
    rng = np.random.default_rng(9700 + 100 * log_n + 10 * log_blowup + n_proofs)
    _quotient_equals_the_model(ctx, oracle, log_n, log_blowup, n_proofs, cap_height, _random_ext(rng, n_proofs * W, log_n),
                               _random_ext(rng, n_proofs * HC, log_n))


@pytest.mark.gpu
def test_quotient_in_three_pieces_in_three_orders(ctx, oracle):
    """5 proofs at N = 256, blow-up 4, through the range call as [0, 2), [2, 3), [3, 5) -- a middle piece, and `first` = 2 and 3 in
    gamma^(628 first) -- in the orders 0-1-2, 2-0-1 and 1-2-0: the first piece of an order writes (also one that does not start at proof 0),
    the later ones accumulate; each order equals the whole quotient, guard words intact"""
    import torch
    N, lb, n_proofs = 256, 2, 5
    log_n = 8 + lb
    rng = np.random.default_rng(9750)
    ext, hext = _random_ext(rng, n_proofs * W, log_n), _random_ext(rng, n_proofs * HC, log_n)
    d_cols, d_hcols, d_cap, d_cap_h, want = _quotient_equals_the_model(ctx, oracle, log_n, lb, n_proofs, CAP_H, ext, hext)
    pieces, words = [(0, 2), (2, 3), (3, 5)], 2 << log_n
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        buf = _sentinel(words + 2 * GUARD)
        for k, (lo, hi) in enumerate(pieces[j] for j in order):
            d_piece = d_hcols[(lo * HC) << log_n:]
            ctx.air_sha512_quotient_device(log_n, lb, CAP_H, n_proofs, d_cols.data_ptr(), d_piece.data_ptr(), d_cap.data_ptr(), d_cap_h.data_ptr(),
                                           buf[GUARD:].data_ptr(), 0, proof_range=(lo, hi), accumulate=int(k > 0))
        torch.cuda.synchronize(_dev())
        assert np.array_equal(_down(buf[GUARD:GUARD + words]), want), order
        assert torch.equal(buf[:GUARD], _sentinel(GUARD)) and torch.equal(buf[GUARD + words:], _sentinel(GUARD)), order


@pytest.mark.gpu
@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("N,log_blowup,n_proofs", [(128, 3, 2), (256, 4, 1)])
def test_quotient_of_extreme_words_equals_the_model(ctx, oracle, N, log_blowup, n_proofs, fill):
    """the inputs the NTT's lazy arithmetic is tested with, as table and helper columns of set 7's sums (32-step dbl_add, scale(carry,
    2^32), 628 accumulated terms): every word p - 1, every word 2^64 - 1, random non-canonical words, and a random choice of edge words"""
    log_n = N.bit_length() - 1 + log_blowup
    rng = np.random.default_rng(9800 + log_n)
    ext, hext = FILLS[fill](rng, (n_proofs * W, 1 << log_n)), FILLS[fill](rng, (n_proofs * HC, 1 << log_n))
    assert ext.dtype == np.uint64 and (fill == "edge words" or int(ext.min()) >= P - 1)
    _quotient_equals_the_model(ctx, oracle, log_n, log_blowup, n_proofs, CAP_H, ext, hext)


# ---- GPU: the chain and the verifier
def _prime(ctx):
    """an evaluation over 2^18 rows on the same context: all 64 rows of `part` then hold nonzero words, so a fold over the wrong number of
    rows cannot hide behind a zeroed allocation"""
    out = _bary(ctx, 18, (0x0123456789ABCDEF % P, 0x0FEDCBA987654321 % P))
    assert out[6] == 0 and all(out[:6])


def _model_verdicts(oracle, p, k_trace, caps, proof):
    """sha512_air_model.verify: [ok and holds].  Where the identity fails that is False for every query whatever batch_model.verify says,
    so its time is only spent on a proof whose identity holds"""
    if not sm.identity(oracle, p, k_trace, caps, proof):
        return [False] * p["n_queries"]
    return sm.verify(oracle, p, k_trace, caps, proof, _shift())


@pytest.mark.gpu
@pytest.mark.parametrize("N,log_blowup,n_proofs", [(128, 6, 1), (2048, 1, 2), (4096, 2, 1)])
def test_tiled_tables_through_the_caller_level_chain(ctx, oracle, live_blocks, N, log_blowup, n_proofs):
    """N = 128 under blow-up 64, N = 2048 (k_air_sha512_check<Sha512Round> folds two rows of `part`) and N = 4096 (four), after an evaluation that left
    all 64 rows nonzero: the quotient has degree <= N - 2, every verdict equals the model verifier's (all accept), the plain batch verifier
    accepts, and a proof with one bumped helper opening of the last proof is rejected on every query by the device and the model"""
    _prime(ctx)
    table = _tiled(live_blocks, N, n_proofs)
    p, d_caps, got, _, _, quot, _ = _chain(ctx, oracle, table, log_blowup)
    assert ctx.fri_last_degree_ok() is True
    caps = _down(d_caps)
    assert max(_degrees(oracle, quot)) <= N - 2
    model = sm.verify(oracle, p, 0, caps, got, _shift())
    assert all(model) and _verdicts(ctx, p, 0, d_caps, got) == model
    assert all(_verdicts(ctx, p, 0, d_caps, got, batch_only=True))
    _, oh, _, _ = _openings(p)
    bad = _bumped(got, oh + (n_proofs - 1) * HC + sm.HU1 + 3)
    model = _model_verdicts(oracle, p, 0, caps, bad)
    assert not any(model) and _verdicts(ctx, p, 0, d_caps, bad) == model


def _chain_on_device(ctx, table, log_blowup, n_queries):
    """tests/test_sha512_air.py's _chain with nothing downloaded but the caps and the proof: (params, d_caps, proof words)"""
    import torch
    n_proofs, log_rows = table.shape[0] // W, table.shape[1].bit_length() - 1
    log_n = log_rows + log_blowup
    d_help = _device_helper(ctx, table)
    d_ext, d_hext = _sentinel((n_proofs * W) << log_n), _sentinel((n_proofs * HC) << log_n)
    ctx.lde_device(log_rows, log_blowup, n_proofs * W, _up(table).data_ptr(), d_ext.data_ptr(), 0)
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
def test_full_size_table_through_the_check_kernel(ctx, oracle, live_blocks):
    """N = 2^15, the real size of T.2 (409 full blocks; k_air_sha512_check<Sha512Round> folds 32 rows of `part`), blow-up 2, one proof, two queries; the
    extended helper (314 MB) never leaves the device.  tests/sha512_air_model.py's identity, which needs the caps and the openings alone,
    holds, the device accepts both queries and the plain batch verifier does; a bumped table opening and a bumped helper opening fail
    the identity and are rejected on both queries.  (0.4 s on the MI355X.)"""
    _prime(ctx)
    table = _tiled(live_blocks, 1 << 15, 1)
    p, d_caps, got = _chain_on_device(ctx, table, 1, 2)
    caps = _down(d_caps)
    assert sm.identity(oracle, p, 0, caps, got)
    assert _verdicts(ctx, p, 0, d_caps, got) == [True, True]
    assert _verdicts(ctx, p, 0, d_caps, got, batch_only=True) == [True, True]
    ot, oh, _, _ = _openings(p)
    for at in (ot + sm.E_ + 1, oh + sm.HMAJ):
        bad = _bumped(got, at)
        assert not sm.identity(oracle, p, 0, caps, bad)
        assert _verdicts(ctx, p, 0, d_caps, bad) == [False, False]


@pytest.mark.gpu
@pytest.mark.parametrize("n_proofs", [7, 8])
def test_openings_planes_of_7_and_8_proofs(ctx, oracle, live_blocks, n_proofs):
    """N = 128, blow-up 2, two queries: 7 proofs are 126 table columns, just under a 128-row openings plane, 8 proofs are 144, the next
    plane size (ZetaView's strides): the honest proof is accepted, a bump in the last proof's last table column and one in its last
    helper column are rejected, as the model's identity has it"""
    _prime(ctx)
    p, d_caps, got = _chain_on_device(ctx, _tiled(live_blocks, 128, n_proofs), 1, 2)
    assert dm.log_r(p["n_cols"][0]) == (7 if n_proofs == 7 else 8)
    caps = _down(d_caps)
    assert sm.identity(oracle, p, 0, caps, got) and _verdicts(ctx, p, 0, d_caps, got) == [True, True]
    ot, oh, _, _ = _openings(p)
    for at in (ot + n_proofs * W - 1, oh + n_proofs * HC - 1):
        bad = _bumped(got, at)
        assert not sm.identity(oracle, p, 0, caps, bad)
        assert _verdicts(ctx, p, 0, d_caps, bad) == [False, False]


# one column per group of the helper, and what the constraints read of the table: (where, column)
READ_SET_BUMPS = ([("table at zeta", c) for c in range(W)] + [("table at zeta omega", c) for c in range(W)]
                  + [("helper at zeta", c) for c in (sm.HA + 5, sm.HB + 63, sm.HC + 32, sm.HE, sm.HF + 31, sm.HG + 40, sm.HU0 + 7, sm.HU1 + 50,
                                                    sm.HV + 33, sm.HS0, sm.HS1 + 1, sm.HCH, sm.HMAJ + 1, sm.HLIVE, sm.HKL, sm.HCAL, sm.HCAH + 1,
                                                    sm.HCEL + 2, sm.HCEH)]
                  + [("helper at zeta omega", c) for c in (sm.HLIVE, sm.HKL, sm.HKL + 1, sm.HA + 5)])
# the bumps after which the identity still holds: W enters through the next row alone, the helper's bits through the current row alone
NOT_READ = {("table at zeta", sm.W_), ("table at zeta", sm.W_ + 1), ("helper at zeta omega", sm.HA + 5)}


@pytest.mark.gpu
def test_which_openings_the_identity_reads(ctx, oracle, live_blocks):
    """N = 128, one proof, blow-up 2: each of the 36 table openings (18 columns at zeta and at zeta omega), one helper column per group at
    zeta and LIVE, KL_lo, KL_hi and one A bit at zeta omega bumped in turn.  For every bump the device verdicts equal the model
    verifier's (all reject: a changed opening fails the batch proof even where the identity does not read it), and the set of bumps after
    which the model's identity still holds is exactly NOT_READ: W at zeta and the helper's A bit at zeta omega"""
    _prime(ctx)
    p, d_caps, got = _chain_on_device(ctx, _tiled(live_blocks, 128, 1), 1, 2)
    caps = _down(d_caps)
    assert sm.identity(oracle, p, 0, caps, got) and _verdicts(ctx, p, 0, d_caps, got) == [True, True]
    ot, oh, _, RH = _openings(p)
    RT = 1 << dm.log_r(p["n_cols"][0])
    base = {"table at zeta": ot, "table at zeta omega": ot + 2 * RT, "helper at zeta": oh, "helper at zeta omega": oh + 2 * RH}
    holds = set()
    for where, c in READ_SET_BUMPS:
        bad = _bumped(got, base[where] + c)
        if sm.identity(oracle, p, 0, caps, bad):
            holds.add((where, c))
            model = sm.verify(oracle, p, 0, caps, bad, _shift())
        else:
            model = [False, False]
        assert _verdicts(ctx, p, 0, d_caps, bad) == model, (where, c)
    print(f"\n[sha512-air shapes] {len(READ_SET_BUMPS)} bumps, the identity still holds after {sorted(holds)}")
    assert holds == NOT_READ


@pytest.mark.gpu
def test_the_table_behind_another_oracle(ctx, oracle, live_blocks):
    """k_trace = 1, N = 128, two proofs: a low-degree random oracle of 3 columns and log_n + 1 in front of the table, so that the openings
    of table, helper and quotient sit behind another oracle's.  The verdicts equal the model's with k_trace = 1 (all accept), a bumped
    helper opening is rejected by both, and k_trace = 0 on the same proof is refused with nothing written"""
    import torch
    _prime(ctx)
    N, n_proofs, lb = 128, 2, 1
    table = _tiled(live_blocks, N, n_proofs)
    rng = np.random.default_rng(9850)
    front = oracle.lde(rng.integers(0, P, (3, 2 * N), dtype=np.uint64), lb)
    p, d_caps, got, _, _, _, _ = _chain(ctx, oracle, table, lb, others=[(0, front)])
    assert ctx.fri_last_degree_ok() is True
    assert p["log_n"] == [9, 8, 8, 8] and p["n_cols"] == [3, n_proofs * W, n_proofs * HC, 2]
    caps = _down(d_caps)
    model = sm.verify(oracle, p, 1, caps, got, _shift())
    assert all(model) and _verdicts(ctx, p, 1, d_caps, got) == model
    assert all(_verdicts(ctx, p, 1, d_caps, got, batch_only=True))
    _, oh, _, _ = _openings(p, 1)
    bad = _bumped(got, oh + HC + sm.HMAJ)
    model = _model_verdicts(oracle, p, 1, caps, bad)
    assert not any(model) and _verdicts(ctx, p, 1, d_caps, bad) == model
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    d_got = _up(got)
    _refused(lambda: ctx.air_sha512_verify_device(p, 0, d_caps.data_ptr(), d_got.data_ptr(), ok.data_ptr(), 0), ok)


# ---- GPU: the set level and the scratch
LADDERS, LADDERS_QUOTIENT = 1, 64


def _set_round(c, kind, n_proofs, lb, tr, sections=SHA512, queries=3, before=None, after=None, calls="7"):
    """commit `sections`, before(), the air calls of `calls` ("1": the ladders', "7": set 7's on SHA512) in that order, after(), one
    proof.  Returns (params, the sections in oracle order, the caps in that order on the device, proof words, set 7's gamma)"""
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
                c.trace_commit_set_air_sha512_device(SHA512, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
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


def _set_7_holds(c, oracle, p, order, d_caps, proof):
    """the device verifier accepts every query, the model's identity holds, and a bumped quotient opening is rejected on every query"""
    k = order.index(SHA512)
    assert _verdicts(c, p, k, d_caps, proof) == [True] * p["n_queries"]
    assert sm.identity(oracle, p, k, _down(d_caps), proof)
    bad = _bumped(proof, bm.layout(p)["off_open"][k + 2])
    assert not any(_verdicts(c, p, k, d_caps, bad))
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
        tr = _trace_rows(c, kind, n, 2, 9910)
        traces = _down(tr)
        for n_proofs in (1, 2):
            p, order, d_caps, proof, gamma = _set_round(c, kind, n_proofs, lb, tr, SHA512 | HEADER)
            k, kh = order.index(SHA512), order.index(HEADER)
            assert p["log_n"][k] == 10 + lb and sorted(order) == sorted([SHA512, HELPER, QUOTIENT, HEADER])
            table = _columns(list(traces[:n_proofs]), kind, n)
            e, lm, nc = _oracle_ext(oracle, kind, n, traces[:n_proofs], HEADER, lb)
            p2, d_caps2, proof2, _, _, _, gamma2 = _chain(c, oracle, table, lb, n_queries=3, others=[(kh, e.reshape(nc, -1))])
            assert {key: p2[key] for key in ("log_n", "n_cols")} == {key: p[key] for key in ("log_n", "n_cols")}
            assert gamma == gamma2 and torch.equal(d_caps, d_caps2), n_proofs
            assert np.array_equal(proof, proof2), n_proofs
            _set_7_holds(c, oracle, p, order, d_caps, proof)


@pytest.mark.gpu
def test_the_ladders_quotient_beside_set_7(built_lib, oracle):
    """a set LADDERS | SHA512 of skip N = 4, one proof, blow-up 2: set 7's tables live inside set 1's table scratch, so the two air calls
    are made in both orders on fresh commits.  Both orders give the same shape, caps and proof words; the ladders' verifier and set 7's
    both accept; a bumped set-7 quotient opening fails set 7's verifier and identity and leaves the ladders' identity holding"""
    import torch
    import tendermintx_amd as tmx
    import test_air as ta
    from test_merkle_open import _trace_rows
    with tmx.Context(4, b"celestia", max_batch=1) as c:
        tr = _trace_rows(c, 0, 4, 1, 9920)
        runs = [_set_round(c, 0, 1, 1, tr, LADDERS | SHA512, calls=way) for way in ("17", "71")]
        (p, order, d_caps, proof, gamma), (p_b, order_b, d_caps_b, proof_b, gamma_b) = runs
        assert (p, order, gamma) == (p_b, order_b, gamma_b) and torch.equal(d_caps, d_caps_b) and np.array_equal(proof, proof_b)
        kl = order.index(LADDERS)
        assert order[kl + 1] == LADDERS_QUOTIENT and len(order) == 5
        caps = _down(d_caps)
        assert all(ta._verdicts(c, p, kl, d_caps, proof)) and am.identity(oracle, p, kl, caps, proof)
        bad = _set_7_holds(c, oracle, p, order, d_caps, proof)
        assert not sm.identity(oracle, p, order.index(SHA512), caps, bad) and am.identity(oracle, p, kl, caps, bad)


@pytest.fixture(scope="module")
def step2_rows(built_lib):
    """a two-proof context of step N = 2 of its own (its d_air7 starts unallocated) and two proofs' trace rows"""
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    with tmx.Context(2, b"celestia", max_batch=2) as c:
        yield c, _trace_rows(c, 1, 2, 2, 9930)


@pytest.mark.gpu
def test_the_domain_moved_between_the_commit_and_the_call(step2_rows, oracle):
    """tmx_ntt_set_domain (g = 7) between the commit and set 7's call, the default back behind the call: the helper AND the three
    preprocessed planes are extended under the set's domain, so caps, gamma and proof equal the unmoved run's and the verifier accepts"""
    import torch
    c, tr = step2_rows
    want = _set_round(c, 1, 2, 1, tr)
    try:
        got = _set_round(c, 1, 2, 1, tr, before=lambda: c.ntt_set_domain(*oracle.G7_DOMAIN), after=lambda: c.ntt_set_domain(*oracle.PLONKY2_DOMAIN))
    finally:
        c.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
    assert got[:2] == want[:2] and got[4] == want[4]
    assert torch.equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    _set_7_holds(c, oracle, *got[:4])


@pytest.mark.gpu
def test_growth_and_reuse_of_the_scratch_on_one_context(oracle):
    """one fresh context: a caller-level quotient at (N, blow-up) = (128, 2) allocates d_air7; round A (set level, one proof of step
    N = 2) grows it; a caller-level quotient at (2048, 4) grows it again (sha512_scratch synchronises, frees and reallocates); round A's
    proof is verified again and accepted; round B (two proofs) and round C (one proof again) follow in the larger scratch.  Both
    caller-level quotients equal the model; every round satisfies the device verifier and the model identity; round C equals round A
    word for word"""
    import torch
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    rng = np.random.default_rng(9940)
    with tmx.Context(2, b"celestia", max_batch=2) as c:
        tr = _trace_rows(c, 1, 2, 2, 9941)
        _quotient_equals_the_model(c, oracle, 8, 1, 1, CAP_H, _random_ext(rng, W, 8), _random_ext(rng, HC, 8))
        a = _set_round(c, 1, 1, 1, tr)
        _set_7_holds(c, oracle, *a[:4])
        _quotient_equals_the_model(c, oracle, 13, 2, 1, CAP_H, _random_ext(rng, W, 13), _random_ext(rng, HC, 13))
        _set_7_holds(c, oracle, *a[:4])
        b = _set_round(c, 1, 2, 1, tr)
        _set_7_holds(c, oracle, *b[:4])
        cc = _set_round(c, 1, 1, 1, tr)
        _set_7_holds(c, oracle, *cc[:4])
        assert cc[:2] == a[:2] and cc[4] == a[4] and torch.equal(cc[2], a[2]) and np.array_equal(cc[3], a[3])
        assert b[0]["n_cols"][:3] == [2 * W, 2 * HC, 2]
