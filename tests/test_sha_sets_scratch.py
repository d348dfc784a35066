"""The scratch of the set-level calls of constraint sets 3, 4 and 5 (tmx_trace_commit_set_air_sha256_device, _sched_device, _init_device):
one buffer per (set, table), grown on demand and reused by later calls.  ONE context takes all three tables in turn, each through three
commits -- one proof (the buffers are allocated), two proofs (all three grow), one proof again (they are larger than needed and reused) --
with the three calls in a different order every time.  Every round ends as table, H3, Q3, H4, Q4, H5, Q5; the proof over the seven
oracles satisfies all three device verifiers and all three model identities; a bumped quotient opening fails its own set alone; and the
third round equals the first word for word.  The buffers of an earlier table stay allocated while a later one is proved, so two
(set, table) pairs that shared a buffer would show as a changed proof or a rejected query.  What the helpers, caps, gammas and quotients
ARE is compared against the models in tests/test_sha_air.py, tests/test_sha_sched.py and tests/test_sha_init.py, whose plumbing this
file uses.  Row 3 of the same table, constraint set 6's (tmx_trace_commit_set_air_sha256_link_device), goes through the same three commits
beside set 5 on a context of its own, under the public tables the device gathers (tests/test_sha_public.py).
Row 4, constraint set 7's, and its d_air7: tests/test_sha512_air_shapes.py test_growth_and_reuse_of_the_scratch_on_one_context."""
import numpy as np
import pytest

import batch_model as bm
import sha_air_model as sm
import sha_init_model as si
import sha_public_model as sl
import sha_sched_model as ss
import test_sha_air as tsa
import test_sha_init as tsi
import test_sha_public as tsl
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


# ---- row 3 of the same scratch table: constraint set 6 (tmx_trace_commit_set_air_sha256_link_device), beside set 5
H6, Q6 = 8192, 16384


@pytest.fixture(scope="module")
def linked(built_lib):
    """one more context of the same shape with two proofs' element and trace rows, and the public tables the device gathers from the
    element rows: {(section, n_proofs): (device table, host table)} (the one-proof table is that of the first proof)"""
    import tendermintx_amd as tmx
    with tmx.Context(N, tsl.CID, max_batch=MAX_BATCH) as c:
        d_rows, tr = tsl._device_rows(c, KIND, N, MAX_BATCH, 9600)
        pubs = {(sec, k): tsl._gather(c, KIND, sec, k, d_rows) for sec in (SHA256, TREE, HEADER) for k in (1, 2)}
        yield c, tr, pubs


def _round_6(c, oracle, tr, pubs, section, n_proofs, way):
    """commit `section` alone, the calls of `way` ("5" and "6") in that order, one proof; set 6's part as _set_6_holds of
    tests/test_sha_public_shapes.py has it; returns (set 6's two caps, its gamma)"""
    import torch
    cw = 4 << CAP_H
    d_pub, pub = pubs[section, n_proofs]
    calls = {"5": lambda h, q: c.trace_commit_set_air_sha256_init_device(section, h, q, 0),
             "6": lambda h, q: c.trace_commit_set_air_sha256_link_device(section, d_pub.data_ptr(), h, q, 0)}
    d_cap_t = _sentinel(cw)
    c.trace_commit_set_device(KIND, n_proofs, section, LB, CAP_H, tr.data_ptr(), d_cap_t.data_ptr(), 0)
    pair, gamma = {}, None
    for s in way:
        pair[s] = (_sentinel(cw), _sentinel(cw))
        calls[s](pair[s][0].data_ptr(), pair[s][1].data_ptr())
        if s == "6":
            gamma = c.air_last_gamma()
    shape, order = c.trace_commit_set_shape()
    assert order == [section] + ([H5, Q5] if "5" in way else []) + [H6, Q6], (section, n_proofs, way)
    k6 = order.index(H6)
    assert shape["n_cols"][k6:] == [n_proofs * sl.HELPER_COLS, 2] and shape["log_n"] == [shape["log_n"][0]] * len(order)
    p = dict(shape, arity_bits=2, final_log_max=2, n_queries=3, pow_bits=0)
    proof = _down(tsa._guarded(bm.layout(p)["words"], lambda out: c.trace_commit_set_prove_device(p, out, 0)))
    assert c.fri_last_degree_ok() is True
    d_caps = torch.cat([d_cap_t] + [x for s in sorted(way) for x in pair[s]])
    caps = _down(d_caps)
    cap_h6, cap_q6 = caps[k6 * cw:(k6 + 1) * cw], caps[(k6 + 1) * cw:]
    assert gamma == sl.gamma(oracle, p["log_n"][0], LB, CAP_H, n_proofs, caps[:cw], cap_h6, pub), (section, n_proofs, way)
    batch = bm.verify(oracle, p, caps, proof, _shift())
    assert tsa._verdicts(c, p, 0, d_caps, proof, batch_only=True) == [bool(x) for x in batch] and all(batch)
    assert sl.identity(oracle, p, 0, k6, caps, proof, pub), (section, n_proofs, way)
    assert tsl._verdicts(c, p, 0, k6, d_caps, proof, pub) == [True] * p["n_queries"], (section, n_proofs, way)
    bad = tsi._bumped(proof, bm.layout(p)["off_open"][k6 + 1])
    assert not any(tsl._verdicts(c, p, 0, k6, d_caps, bad, pub)), (section, n_proofs, way)
    return cap_h6.copy(), cap_q6.copy(), gamma


@pytest.mark.gpu
@pytest.mark.parametrize("section", [SHA256, TREE, HEADER])
def test_three_commits_of_set_6_per_table_on_one_context(linked, oracle, section):
    """one proof with the calls in the order 6, 5 (the row-3 buffer of this table is allocated); two proofs in the order 5, 6 (it grows);
    one proof with set 6 alone (it is larger than needed and reused).  Every round's proof satisfies set 6's device verifier and the
    model identity under the gathered public table and is rejected on a bumped quotient opening; set 6's two caps and gamma in the third
    round equal the first round's word for word"""
    c, tr, pubs = linked
    first = _round_6(c, oracle, tr, pubs, section, 1, "65")
    _round_6(c, oracle, tr, pubs, section, 2, "56")
    third = _round_6(c, oracle, tr, pubs, section, 1, "6")
    assert np.array_equal(first[0], third[0]) and np.array_equal(first[1], third[1]) and first[2] == third[2]
