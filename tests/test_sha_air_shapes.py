"""The set-3 kernels (tendermintx_amd/csrc/air.hip k_air_sha_helper, k_air_sha_tables, k_air_sha_quotient, k_air_sha_check, k_air_sha_gamma) at
every shape they branch on: more proofs than k_air_sha_check has threads, N = 64 (no squaring of zeta, the seam row is the wrap-around) and
N = 1024 / 2048, blow-up up to 6 (sixteen workgroups of k_air_sha_tables, 4096-entry S / K tables), partly filled helper workgroups, the
edge words of the helper's definition, the extreme words of the lazy field arithmetic, k_trace = 1 and the set-level call on T.5.  The
yardstick stays tests/sha_air_model.py on tests/batch_model.py: device words equal the model's word for word, every device verdict equals
the model verifier's, guard words stay intact.  The helpers and fixtures are those of tests/test_sha_air.py; docs/kernels.md "set 3: which
test reaches which shape" is the map."""
import hashlib

import numpy as np
import pytest

import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha_air_model as sm
from batch_model import bparams
from test_fri import _down, _sentinel, _shift, _up
from test_sha_air import (BAD_ARG, CAP_H, HC, HEADER, HELPER, QUOTIENT, SHA256, TREE, W, _cap, _chain, _degrees, _dev, _device_helper,  # noqa: F401
                          _device_quotient, _guarded, _model_quotient, _random_ext, _refused, _tree, _verdicts, ctx, skip4, step2, step3)

P = fm.P


# ---- honest tables of any size
@pytest.fixture(scope="module")
def live_blocks(skip4, step2, step3):
    """[n][9][64]: every 64-row block of the CPU oracle's T.3, T.5 and T.6 rows (skip N = 4, step N = 2, step N = 3, two proofs each) that
    is not all zero"""
    out = []
    for tables in (skip4, step2, step3):
        for sec in (SHA256, TREE, HEADER):
            t = tables[sec]
            for p in range(t.shape[0] // W):
                blocks = t[p * W:(p + 1) * W].reshape(W, -1, 64).transpose(1, 0, 2)
                out.append(blocks[blocks.any(axis=(1, 2))])
    out = np.concatenate(out)
    assert len(out) >= 100 and out[:, :, 0].any(axis=1).all()  # (a live block's first row is not zero: LIVE sees it)
    return out


def _tiled(live_blocks, N, n_proofs):
    """[9 n_proofs][N] pre-LDE columns: the live blocks in turn, every seventh block of the tiling (with N = 64: every seventh proof) all zero.
    A block's 63 transitions are honest and the seam and wrap-around rows are unselected, so every tiling satisfies the set."""
    assert N % 64 == 0
    nb = N // 64
    table = np.zeros((n_proofs * W, N), dtype=np.uint64)
    for g in range(n_proofs * nb):
        if g % 7 != 6:
            p, b = divmod(g, nb)
            table[p * W:(p + 1) * W, 64 * b:64 * b + 64] = live_blocks[(g - g // 7) % len(live_blocks)]
    return table


@pytest.mark.parametrize("N,n_proofs", [(64, 5), (1024, 1)])
def test_tiled_tables_satisfy_the_constraints_as_integers(live_blocks, N, n_proofs):
    """the tiling at N = 64 (one block per proof) and N = 1024 (sixteen blocks, two of them zero): all 315 constraints are integer identities
    on every row of every proof"""
    print(f"\n[sha-air shapes] {len(live_blocks)} live blocks")
    table = _tiled(live_blocks, N, n_proofs)
    help_ = sm.helper(table, n_proofs)
    live = help_[sm.HLIVE::HC]
    assert live.any() and (N == 64 or not live.all())
    for p in range(n_proofs):
        for j, c in enumerate(sm.integer_residuals(table[p * W:(p + 1) * W], help_[p * HC:(p + 1) * HC])):
            assert not c.any(), (p, j, np.flatnonzero(c)[:4])


class _Remembering:
    """the CPU oracle with its Poseidon trees remembered per input: the tree over 6000 helper columns takes seconds, and the model's gamma,
    the caps and batch_model.prove each ask for it"""

    def __init__(self, oracle):
        self._oracle, self._trees = oracle, {}

    def __getattr__(self, name):
        return getattr(self._oracle, name)

    def poseidon_merkle(self, cols, log_n, n_cols, cap_height):
        key = (hashlib.sha256(np.ascontiguousarray(cols, dtype=np.uint64).tobytes()).digest(), log_n, n_cols, cap_height)
        if key not in self._trees:
            self._trees[key] = self._oracle.poseidon_merkle(cols, log_n, n_cols, cap_height)
        return self._trees[key].copy()


def test_tiled_quotient_has_degree_below_n_and_the_identity_holds(oracle, live_blocks):
    """N = 64, 20 proofs (proofs 6 and 13 zero), blow-up 4: the model quotient interpolates to degree < N in both planes; the identity holds
    on a tests/batch_model.py proof over [table, helper, quotient] and fails after one helper opening of proof 19 is bumped"""
    N, n_proofs, lb = 64, 20, 2
    oracle = _Remembering(oracle)
    table = _tiled(live_blocks, N, n_proofs)
    ext, hext, g, quot = _model_quotient(oracle, table, sm.helper(table, n_proofs), lb)
    deg = _degrees(oracle, quot)
    print(f"\n[sha-air shapes] N = {N}, {n_proofs} proofs: quotient degrees {deg}")
    assert max(deg) < N
    log_n = 6 + lb
    p = bparams([log_n] * 3, [n_proofs * W, n_proofs * HC, 2], CAP_H, lb, 2, 2, 1)
    cols = [ext, hext, quot.reshape(2, -1)]
    caps = np.concatenate([_cap(oracle, c, log_n) for c in cols])
    proof, degree_ok, _, _ = bm.prove(oracle, p, cols, _shift())
    assert degree_ok and sm.identity(oracle, p, 0, caps, proof)
    at = bm.layout(p)["off_open"][1] + 19 * HC + sm.HE + 9
    proof[at] = np.uint64((int(proof[at]) + 1) % P)
    assert not sm.identity(oracle, p, 0, caps, proof)


# ---- GPU: the helper
def _edge_blocks(rng):
    """[(block [9][64], LIVE)]: a first row that is nonzero in the high 32 bits of one word only (LIVE = 1 while every operand is 0), a
    block that is nonzero only below its first row (LIVE = 0), all low words 0xFFFFFFFF under random high words (the largest carries)"""
    high_only = np.zeros((W, 64), dtype=np.uint64)
    high_only[sm.H_, 0] = np.uint64(1 << 32)
    below = rng.integers(0, 1 << 64, (W, 64), dtype=np.uint64)
    below[:, 0] = 0
    ones = rng.integers(0, 1 << 64, (W, 64), dtype=np.uint64) | np.uint64(0xFFFFFFFF)
    return [(high_only, 1), (below, 0), (ones, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs", [(6, 1), (6, 3), (6, 5), (6, 257), (11, 2), (12, 1)])
def test_helper_at_every_grid_shape_equals_the_model(ctx, log_rows, n_proofs):
    """random 64-bit words from one block per proof (the grid's last workgroup partly filled at 3 and 5 proofs, 65 workgroups at 257) to 64
    blocks per proof; at log_rows >= 11 the even blocks and the last block of every proof are zero; at (6, 5) and (11, 2) the three edge
    blocks are planted.  The helper equals the model's word for word, guard words intact; the LIVE column is the expected one, and where
    the all-ones block is planted the carries CA = 6 and CE = 5 occur"""
    rng = np.random.default_rng(9500 + 10 * log_rows + n_proofs)
    nb = 1 << (log_rows - 6)
    table = rng.integers(0, 1 << 64, (n_proofs * W, 64 * nb), dtype=np.uint64)
    live = np.ones((n_proofs, nb), dtype=np.uint64)

    def put(p, b, block, lv):
        table[p * W:(p + 1) * W, 64 * b:64 * b + 64] = block
        live[p, b] = lv
    if log_rows >= 11:
        for p in range(n_proofs):
            for b in [*range(0, nb, 2), nb - 1]:
                put(p, b, 0, 0)
    planted = (log_rows, n_proofs) in ((6, 5), (11, 2))
    if planted:
        where = [(1, 0), (2, 0), (4, 0)] if log_rows == 6 else [(0, 1), (0, 29), (1, 31)]  # ((1, 31): a zeroed last block becomes the all-ones one)
        for (p, b), (block, lv) in zip(where, _edge_blocks(rng)):
            put(p, b, block, lv)
    got = _down(_device_helper(ctx, table)).reshape(n_proofs * HC, -1)
    want = sm.helper(table, n_proofs)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    assert np.array_equal(want[sm.HLIVE::HC], np.repeat(live, 64, axis=1))
    assert np.array_equal(got[sm.HLIVE::HC], np.repeat(live, 64, axis=1))
    if planted:
        ca = want[sm.HCA::HC] + 2 * want[sm.HCA + 1::HC] + 4 * want[sm.HCA + 2::HC]
        ce = want[sm.HCE::HC] + 2 * want[sm.HCE + 1::HC] + 4 * want[sm.HCE + 2::HC]
        assert int(ca.max()) == 6 and int(ce.max()) == 5


# ---- GPU: the quotient of arbitrary columns
def _quotient_equals_the_model(ctx, oracle, log_n, log_blowup, n_proofs, cap_height, ext, hext):
    d_cols, d_hcols = _up(ext), _up(hext)
    _, d_cap = _tree(ctx, d_cols, log_n, n_proofs * W, cap_height)
    _, d_cap_h = _tree(ctx, d_hcols, log_n, n_proofs * HC, cap_height)
    got = _down(_device_quotient(ctx, log_n, log_blowup, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, cap_height))
    g = sm.gamma(oracle, log_n, log_blowup, cap_height, n_proofs, _down(d_cap), _down(d_cap_h))
    assert ctx.air_last_gamma() == g
    want = sm.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("N,log_blowup,n_proofs,cap_height", [(64, 1, 1, 0), (64, 6, 2, 2), (64, 3, 17, 2), (128, 4, 3, 2), (256, 5, 1, 0),
                                                              (2048, 2, 1, 2), (64, 1, 1, 7)])
def test_quotient_of_random_columns_at_every_table_size(ctx, oracle, N, log_blowup, n_proofs, cap_height):
    """random full-degree columns: N = 64 (the S / K period is the whole domain) up to N = 2048, blow-up up to 6 (sixteen workgroups of
    k_air_sha_tables, 4096-entry tables), a Horner chain over 17 proofs, and a cap that is the whole leaf level (gamma absorbs 2 x 512 words):
    d_quot and gamma equal the model word for word, guard words intact"""
    log_n = N.bit_length() - 1 + log_blowup
    rng = np.random.default_rng(9600 + 100 * log_n + 10 * log_blowup + n_proofs)
    _quotient_equals_the_model(ctx, oracle, log_n, log_blowup, n_proofs, cap_height, _random_ext(rng, n_proofs * W, log_n),
                               _random_ext(rng, n_proofs * HC, log_n))


EDGE_WORDS = np.array([0, 1, P - 1, P, P + 1, (1 << 64) - 1, (1 << 32) - 1, 1 << 32, 1 << 63], dtype=np.uint64)
FILLS = {
    "all p - 1": lambda rng, shape: np.full(shape, P - 1, dtype=np.uint64),
    "all 2^64 - 1": lambda rng, shape: np.full(shape, (1 << 64) - 1, dtype=np.uint64),
    "random in [p, 2^64)": lambda rng, shape: rng.integers(P, 1 << 64, shape, dtype=np.uint64),
    "edge words": lambda rng, shape: rng.choice(EDGE_WORDS, shape),
}


@pytest.mark.gpu
@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("N,log_blowup,n_proofs", [(64, 3, 2), (128, 4, 1)])
def test_quotient_of_extreme_words_equals_the_model(ctx, oracle, N, log_blowup, n_proofs, fill):
    """the inputs the NTT's lazy arithmetic is tested with, as table and helper columns: every word p - 1, every word 2^64 - 1, random
    non-canonical words, and a random choice of edge words"""
    log_n = N.bit_length() - 1 + log_blowup
    rng = np.random.default_rng(9700 + log_n)
    ext, hext = FILLS[fill](rng, (n_proofs * W, 1 << log_n)), FILLS[fill](rng, (n_proofs * HC, 1 << log_n))
    assert ext.dtype == np.uint64 and (fill == "edge words" or int(ext.min()) >= P - 1)
    _quotient_equals_the_model(ctx, oracle, log_n, log_blowup, n_proofs, CAP_H, ext, hext)


# ---- GPU: the chain and the identity
def _bumped(proof, at):
    bad = proof.copy()
    bad[at] = np.uint64((int(bad[at]) % P + 1) % P)
    return bad


def _model_verdicts(oracle, p, k_trace, caps, proof):
    """sha_air_model.verify: [ok and holds].  Where the identity fails that is False for every query whatever batch_model.verify says, so its
    seconds per query over tens of thousands of columns are only spent on a proof whose identity holds"""
    if not sm.identity(oracle, p, k_trace, caps, proof):
        return [False] * p["n_queries"]
    return sm.verify(oracle, p, k_trace, caps, proof, _shift())


def _openings(p, k_trace=0):
    """(the word offsets of the table's, the helper's and the quotient's openings sections, the helper section's row count R): column c at
    zeta is word c of a section, at zeta omega word 2 R + c"""
    L = bm.layout(p)
    return L["off_open"][k_trace], L["off_open"][k_trace + 1], L["off_open"][k_trace + 2], 1 << dm.log_r(p["n_cols"][k_trace + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("N,log_blowup,n_proofs", [(64, 1, 1), (1024, 2, 2)])
def test_tiled_tables_through_the_caller_level_chain(ctx, oracle, live_blocks, N, log_blowup, n_proofs):
    """N = 64 (k_air_sha_check squares zeta zero times; one block, so the only unselected row is seam and wrap-around at once) and N = 1024
    (four squarings, 32 blocks of which four are zero): the helper, the quotient and gamma equal the model's, the quotient has degree < N,
    every verdict equals the model verifier's (all accept), the plain batch verifier accepts, and a proof with one bumped opening of each
    kind is rejected on every query by the device and the model"""
    table = _tiled(live_blocks, N, n_proofs)
    p, d_caps, got, ext, hext, quot = _chain(ctx, oracle, table, log_blowup)
    assert ctx.fri_last_degree_ok() is True
    log_n, caps, cw = p["log_n"][0], _down(d_caps), 4 << CAP_H
    assert np.array_equal(hext, oracle.lde(sm.helper(table, n_proofs), log_blowup))
    g = sm.gamma(oracle, log_n, log_blowup, CAP_H, n_proofs, caps[:cw], caps[cw:2 * cw])
    assert np.array_equal(quot, sm.quotient(oracle, log_n, log_blowup, n_proofs, ext, hext, _shift(), g))
    assert max(_degrees(oracle, quot)) < N
    model = sm.verify(oracle, p, 0, caps, got, _shift())
    assert all(model) and _verdicts(ctx, p, 0, d_caps, got) == model
    assert all(_verdicts(ctx, p, 0, d_caps, got, batch_only=True))
    ot, oh, oq, RH = _openings(p)
    last = n_proofs - 1
    for name, at in (("quotient opening", oq + 1), ("helper opening at zeta", oh + last * HC + sm.HE + 9),
                     ("helper KL at zeta omega", oh + 2 * RH + last * HC + sm.HKL), ("table opening at zeta", ot + last * W + sm.D_)):
        bad = _bumped(got, at)
        model = _model_verdicts(oracle, p, 0, caps, bad)
        assert not any(model), name
        assert _verdicts(ctx, p, 0, d_caps, bad) == model, name


MANY = 257  # one proof more than k_air_sha_check has threads: thread 0 takes proofs 0 and 256


@pytest.fixture(scope="module")
def many(ctx, oracle, live_blocks):
    """the chain at N = 64 with 257 proofs, blow-up 2, two queries (a 79 MB extended helper).  The helper's and the table's caps are the
    device's Poseidon tree over words that equal the model's (asserted here), as in test_set_level_on_the_header_table; the quotient is the
    device's own -- the identity holding on it is the tie, the kernel's words are compared in the quotient tests above"""
    table = _tiled(live_blocks, 64, MANY)
    p, d_caps, got, ext, hext, _ = _chain(ctx, oracle, table, 1, n_queries=2)
    assert ctx.fri_last_degree_ok() is True
    assert np.array_equal(ext, oracle.lde(table, 1))
    assert np.array_equal(hext, oracle.lde(sm.helper(table, MANY), 1))
    return p, d_caps, _down(d_caps), got


@pytest.mark.gpu
def test_257_proofs_are_accepted(ctx, oracle, many):
    """every thread of k_air_sha_check contributes to the LDS reduction and thread 0's proof loop takes a second trip: the device accepts
    every query, as the model verifier and the plain batch verifier do"""
    p, d_caps, caps, got = many
    assert p["n_cols"] == [MANY * W, MANY * HC, 2] and p["log_n"] == [7] * 3
    model = sm.verify(oracle, p, 0, caps, got, _shift())
    assert all(model) and _verdicts(ctx, p, 0, d_caps, got) == model
    assert all(_verdicts(ctx, p, 0, d_caps, got, batch_only=True))


@pytest.mark.gpu
@pytest.mark.parametrize("what,proof_no", [("table", 0), ("table", 255), ("table", 256), ("helper", 1), ("helper", 200), ("helper", 256),
                                           ("helper KL at zeta omega", 256), ("quotient", None)])
def test_257_proofs_with_one_changed_opening_are_rejected(ctx, oracle, many, what, proof_no):
    """one opening changed -- the table's at zeta in proofs 0, 255 and 256, the helper's at zeta in proofs 1, 200 and 256, the helper's KL at
    zeta omega in proof 256, the quotient's: rejected on every query by the device and by the model (a reduction step that drops a thread,
    a wrong gamma^(315 p) or a proof loop that stops after one trip would keep some of them accepted)"""
    p, d_caps, caps, got = many
    ot, oh, oq, RH = _openings(p)
    at = {"table": lambda: ot + proof_no * W + sm.E_, "helper": lambda: oh + proof_no * HC + sm.HU1 + 3,
          "helper KL at zeta omega": lambda: oh + 2 * RH + proof_no * HC + sm.HKL, "quotient": lambda: oq + 2}[what]()
    bad = _bumped(got, at)
    model = _model_verdicts(oracle, p, 0, caps, bad)
    assert not any(model)
    assert _verdicts(ctx, p, 0, d_caps, bad) == model


@pytest.mark.gpu
def test_the_table_behind_another_oracle(ctx, oracle, live_blocks):
    """k_trace = 1, N = 64, two proofs: a low-degree random oracle of 3 columns and log_n + 1 in front of the table, so that the openings
    of table, helper and quotient sit behind another oracle's (log_r 2 in front of log_r 5 and 10).  The verdicts equal the model's with
    k_trace = 1 (all accept), a bumped helper opening is rejected by both, and k_trace = 0 on the same proof is refused with nothing written"""
    import torch
    N, n_proofs, lb = 64, 2, 1
    table = _tiled(live_blocks, N, n_proofs)
    rng = np.random.default_rng(9800)
    front = oracle.lde(rng.integers(0, P, (3, 2 * N), dtype=np.uint64), lb)
    p, d_caps, got, _, _, _ = _chain(ctx, oracle, table, lb, front=front)
    assert ctx.fri_last_degree_ok() is True
    assert p["log_n"] == [8, 7, 7, 7] and p["n_cols"] == [3, n_proofs * W, n_proofs * HC, 2]
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
    _refused(lambda: ctx.air_sha256_verify_device(p, 0, d_caps.data_ptr(), d_got.data_ptr(), ok.data_ptr(), 0), ok)


# ---- GPU: the set-level call on T.5
@pytest.mark.gpu
def test_set_level_on_the_tree_table(built_lib, oracle):
    """a set TREE + SHA256 at step N = 3, two proofs, blow-up 2; the air call on TREE (T.5: padding, zero blocks and chained second blocks):
    the shape and the section ids, the table's and the helper's caps, gamma and the quotient's cap against the model, one proof over the
    four oracles, the device verifier's verdicts and the model's.  (The helper's cap through the device's Poseidon tree over the MODEL's
    helper words, as in test_set_level_on_the_header_table.)"""
    import torch
    import tendermintx_amd as tmx
    from test_merkle_open import _oracle_ext, _section_geom, _trace_rows
    kind, n, n_proofs, lb = 1, 3, 2, 1
    cw = 4 << CAP_H
    with tmx.Context(n, b"celestia", max_batch=n_proofs) as c:
        tr = _trace_rows(c, kind, n, n_proofs, 9900)
        d_caps, d_cap_h, d_cap_q = _sentinel(2 * cw), _sentinel(cw), _sentinel(cw)
        c.trace_commit_set_device(kind, n_proofs, SHA256 | TREE, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
        shape0, order0 = c.trace_commit_set_shape()
        assert order0 == [TREE, SHA256] and shape0["log_n"] == [9 + lb, 8 + lb]
        c.trace_commit_set_air_sha256_device(TREE, d_cap_h.data_ptr(), d_cap_q.data_ptr(), 0)
        gamma = c.air_last_gamma()
        shape, order = c.trace_commit_set_shape()
        assert order == [TREE, HELPER, QUOTIENT, SHA256]
        assert shape["log_n"] == [9 + lb] * 3 + [8 + lb] and shape["n_cols"] == [W * n_proofs, HC * n_proofs, 2, W * n_proofs]
        p = dict(shape, arity_bits=2, final_log_max=2, n_queries=3, pow_bits=0)
        proof = _guarded(bm.layout(p)["words"], lambda out: c.trace_commit_set_prove_device(p, out, 0))
        assert c.fri_last_degree_ok() is True
        all_caps = torch.cat([d_caps[:cw], d_cap_h, d_cap_q, d_caps[cw:]])
        caps_h, got = _down(all_caps), _down(proof)
        # the model: the tree table from the device's trace rows, its helper, both caps, gamma, the quotient and its cap
        traces = _down(tr)
        e, lm, nc = _oracle_ext(oracle, kind, n, traces, TREE, lb)
        assert (lm, nc) == (9 + lb, W * n_proofs)
        ext = e.reshape(nc, -1)
        off, rows, width = _section_geom(kind, n, TREE)
        table = np.zeros((n_proofs * W, 1 << (lm - lb)), dtype=np.uint64)
        for q, full in enumerate(traces):
            table[q * W:(q + 1) * W, :rows] = full[off:off + rows * W].reshape(rows, W).T
        live = sm.helper(table, n_proofs)[sm.HLIVE::HC]
        assert live.any() and not live.all()
        hext = oracle.lde(sm.helper(table, n_proofs), lb)
        assert np.array_equal(caps_h[:cw], _cap(oracle, ext, lm))
        assert np.array_equal(caps_h[cw:2 * cw], _down(_tree(c, _up(hext), lm, n_proofs * HC)[1]))
        assert gamma == sm.gamma(oracle, lm, lb, CAP_H, n_proofs, caps_h[:cw], caps_h[cw:2 * cw])
        quot = sm.quotient(oracle, lm, lb, n_proofs, ext, hext, _shift(), gamma)
        assert np.array_equal(caps_h[2 * cw:3 * cw], _cap(oracle, quot.reshape(2, -1), lm))
        model = sm.verify(oracle, p, 0, caps_h, got, _shift())
        assert all(model) and _verdicts(c, p, 0, all_caps, got) == model
        bad = _bumped(got, bm.layout(p)["off_open"][1] + HC + sm.HLIVE)
        model = _model_verdicts(oracle, p, 0, caps_h, bad)
        assert not any(model) and _verdicts(c, p, 0, all_caps, bad) == model
