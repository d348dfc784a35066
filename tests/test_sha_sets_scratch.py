"""The scratch of the set-level calls of constraint sets 3, 4 and 5 (tmx_trace_commit_set_air_sha256_device, _sched_device, _init_device):
one buffer per (set, table), grown on demand and reused by later calls.  ONE context takes all three tables in turn, each through three
commits -- one proof (the buffers are allocated), two proofs (all three grow), one proof again (they are larger than needed and reused) --
with the three calls in a different order every time.  Every round ends as table, H3, Q3, H4, Q4, H5, Q5; the proof over the seven
oracles satisfies all three device verifiers and all three model identities; a bumped quotient opening fails its own set alone; and the
third round equals the first word for word.  The buffers of an earlier table stay allocated while a later one is proved, so two
(set, table) pairs that shared a buffer would show as a changed proof or a rejected query.  What the helpers, caps, gammas and quotients
ARE is compared against the models in tests/test_sha_air.py, tests/test_sha_sched.py and tests/test_sha_init.py, whose plumbing this
file uses."""
import numpy as np
import pytest

import batch_model as bm
import sha_air_model as sm
import sha_init_model as si
import sha_sched_model as ss
import test_sha_air as tsa
import test_sha_init as tsi
import test_sha_sched as tss
from test_fri import _down, _sentinel, _shift

SHA256, TREE, HEADER = 4, 16, 32
H3, Q3, H4, Q4, H5, Q5 = 128, 256, 512, 1024, 2048, 4096
CAP_H, LB = 2, 1
KIND, N, MAX_BATCH = 0, 4, 2  # the shape of test_a_full_set_is_refused: it holds all three tables


@pytest.fixture(scope="module")
def shared(built_lib):
    """the one context and two proofs' trace rows; the one-proof rounds commit the first of them"""
    import tendermintx_amd as tmx
    from test_merkle_open import _trace_rows
    with tmx.Context(N, b"celestia", max_batch=MAX_BATCH) as c:
        yield c, _trace_rows(c, KIND, N, MAX_BATCH, 9500)


def _round(c, oracle, tr, section, n_proofs, way):
    """commit `section` alone (a one-section mask is a legal set), the three calls in the order `way`, one proof, every check; returns
    (caps of the seven oracles in order, proof words)"""
    import torch
    cw, chain = 4 << CAP_H, tsi.CHAIN[section]
    calls = {"3": c.trace_commit_set_air_sha256_device, "4": c.trace_commit_set_air_sha256_sched_device,
             "5": c.trace_commit_set_air_sha256_init_device}
    d_cap_t = _sentinel(cw)
    c.trace_commit_set_device(KIND, n_proofs, section, LB, CAP_H, tr.data_ptr(), d_cap_t.data_ptr(), 0)
    pair = {}
    for s in way:
        pair[s] = (_sentinel(cw), _sentinel(cw))
        calls[s](section, pair[s][0].data_ptr(), pair[s][1].data_ptr(), 0)
    shape, order = c.trace_commit_set_shape()
    assert order == [section, H3, Q3, H4, Q4, H5, Q5], (section, n_proofs, way)
    assert shape["n_cols"] == [n_proofs * k for k in (sm.WIDTH, sm.HELPER_COLS)] + [2, n_proofs * ss.HELPER_COLS, 2, n_proofs * si.HELPER_COLS, 2]
    p = dict(shape, arity_bits=2, final_log_max=2, n_queries=6, pow_bits=0)
    proof = _down(tsa._guarded(bm.layout(p)["words"], lambda out: c.trace_commit_set_prove_device(p, out, 0)))
    assert c.fri_last_degree_ok() is True
    d_caps = torch.cat([d_cap_t] + [x for s in "345" for x in pair[s]])
    caps = _down(d_caps)
    verdicts = {"3": lambda w: tsa._verdicts(c, p, 0, d_caps, w), "4": lambda w: tss._verdicts(c, p, 0, 3, d_caps, w),
                "5": lambda w: tsi._verdicts(c, p, 0, 5, chain, d_caps, w)}
    identity = {"3": lambda w: sm.identity(oracle, p, 0, caps, w), "4": lambda w: ss.identity(oracle, p, 0, 3, caps, w),
                "5": lambda w: si.identity(oracle, p, 0, 5, chain, caps, w)}
    for s in "345":
        assert all(verdicts[s](proof)), (section, n_proofs, way, s)
        assert identity[s](proof), (section, n_proofs, way, s)
    assert tsa._verdicts(c, p, 0, d_caps, proof, batch_only=True) == bm.verify(oracle, p, caps, proof, _shift())
    L = bm.layout(p)
    for s, k_quot in (("3", 2), ("4", 4), ("5", 6)):  # one word of that set's quotient openings: its verifier and its identity alone
        bad = tsi._bumped(proof, L["off_open"][k_quot])
        assert not any(verdicts[s](bad)), (section, n_proofs, way, s)
        assert [bool(identity[t](bad)) for t in "345"] == [t != s for t in "345"], (section, n_proofs, way, s)
    return caps, proof


@pytest.mark.gpu
@pytest.mark.parametrize("section", [SHA256, TREE, HEADER])
def test_three_commits_per_table_on_one_context(shared, oracle, section):
    """one proof with the calls in the order 5, 3, 4; two proofs (the grow path of the three buffers of this table) in the order 3, 4, 5;
    one proof again (the buffers reused) in the order 4, 5, 3: the caps of all seven oracles and the proof equal the first round's"""
    c, tr = shared
    caps1, proof1 = _round(c, oracle, tr, section, 1, "534")
    _round(c, oracle, tr, section, 2, "345")
    caps3, proof3 = _round(c, oracle, tr, section, 1, "453")
    assert np.array_equal(caps1, caps3) and np.array_equal(proof1, proof3)
