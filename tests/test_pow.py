"""Proof-of-work grinding on the FRI and DEEP proofs (include/tmx.h "proof of work"): tmx_pow_proof_words, tmx_pow_prove_device,
tmx_trace_commit_pow_device, tmx_pow_verify_device, tmx_pow_last.  The yardstick is tests/pow_model.py, the model of the header's
definition over tests/fri_model.py and tests/deep_model.py: device proofs must equal the model's word for word (the nonce is the SMALLEST
one, so the proof is a function of its inputs), and every verdict of the device verifier must equal the model verifier's.  No test
reaches the search bound 2^(pow_bits + 6): it cannot be reached with honest inputs."""
import ctypes as C

import numpy as np
import pytest

import deep_model as dm
import fri_model as fm
import pow_model as pw
from test_deep import _deep_tamper_cases
from test_fri import _down, _low_degree_cols, _sentinel, _shift, _tamper_cases, _tree, _up, params
from test_merkle_open import _oracle_ext, _trace_rows

P = fm.P
BAD_ARG = -1

# the caller-column shapes of tests/test_fri.py (plain FRI) and tests/test_deep.py (DEEP), written out
FRI_SHAPES = [params(6, 3, 2, 2, 2, 5, 4), params(9, 5, 1, 2, 3, 1, 7), params(8, 4, 3, 1, 1, 2, 5), params(10, 9, 6, 2, 4, 0, 3),
              params(12, 64, 4, 3, 4, 5, 28), params(9, 1, 2, 3, 3, 2, 16), params(10, 3, 4, 2, 2, 3, 9), params(7, 4, 1, 1, 4, 2, 12),
              params(11, 9, 3, 3, 4, 4, 30)]
DEEP_SHAPES = [params(6, 3, 2, 2, 2, 5, 4), params(9, 5, 1, 2, 3, 1, 7), params(8, 4, 3, 1, 1, 2, 5), params(10, 9, 6, 2, 4, 0, 3),
               params(9, 1, 2, 3, 3, 2, 16), params(7, 1, 7, 3, 2, 0, 1), params(11, 64, 4, 3, 4, 5, 28), params(12, 2, 0, 1, 3, 3, 40)]
CALLER_CASES = [(deep, p, bits) for deep, shapes in ((0, FRI_SHAPES), (1, DEEP_SHAPES)) for p in shapes for bits in (1, 4, 8, 12)]
CALLER_CASES += [(0, FRI_SHAPES[1], 16), (1, DEEP_SHAPES[2], 16)]


def _case_id(case):
    deep, p, bits = case
    return f"{'deep' if deep else 'fri'}-{p['log_n']}x{p['n_cols']}q{p['n_queries']}-pow{bits}"


def _pow_words(p, bits, deep):
    from tendermintx_amd import _lib
    pp = _lib.PowParams(fri=_lib.FriParams(**{k: int(v) for k, v in p.items()}), pow_bits=bits, deep=deep)
    return int(_lib.lib().tmx_pow_proof_words(C.byref(pp)))


def _cap_of(oracle, p, cols):
    return oracle.poseidon_merkle(np.ascontiguousarray(cols).reshape(-1), p["log_n"], p["n_cols"], p["cap_height"])[-(1 << p["cap_height"]):]


def _plain_tampers(p, deep, body):
    """the tamper cases of tests/test_fri.py / tests/test_deep.py on the part of a grinding proof in front of its nonce"""
    return _deep_tamper_cases(p, body) if deep else _tamper_cases(p, body)


# ---- CPU
@pytest.mark.parametrize("deep", [0, 1])
def test_proof_words_equal_the_model(built_lib, deep):
    from tendermintx_amd.context import pow_proof_words
    for p in FRI_SHAPES + DEEP_SHAPES + [params(28, 4608, 4, 3, 4, 5, 28), params(5, 3, 0, 4, 1, 8, 2)]:
        for bits in (1, 7, 16, 24):
            want = fm.layout(p)["words"] + 1 + (dm.openings_words(p["n_cols"]) if deep else 0)
            assert _pow_words(p, bits, deep) == pow_proof_words(p, bits, deep) == pw.proof_words(p, deep) == want


@pytest.mark.parametrize("field,value", [("pow_bits", 0), ("pow_bits", 25), ("deep", 2), ("log_blowup", 0), ("log_blowup", 7), ("log_n", 3),
                                         ("log_n", 29), ("n_cols", 0), ("cap_height", 11), ("arity_bits", 0), ("arity_bits", 5),
                                         ("final_log_max", 9), ("n_queries", 0), ("n_queries", 257), ("reserved", 1),
                                         ("n_cols", (1 << 24) + 1)])
def test_proof_words_refuse_each_rule(built_lib, field, value):
    """each rule on its own: the base parameters are accepted for both proofs, the broken ones answer 0 (n_cols above 2^24 only for the
    DEEP proof, whose rule it is) and the Python wrapper raises BAD_ARG"""
    from tendermintx_amd._lib import TmxError
    from tendermintx_amd.context import pow_proof_words
    base = dict(params(10, 4, 2, 3, 2, 4, 8), reserved=0)
    for deep in (0, 1):
        assert _pow_words(base, 16, deep) == pw.proof_words(base, deep)
        p, bits, dp = dict(base), 16, deep
        if field == "pow_bits":
            bits = value
        elif field == "deep":
            dp = value
        else:
            p[field] = value
        if field == "n_cols" and value > (1 << 24) and not deep:
            assert _pow_words(p, bits, dp) == pw.proof_words(p, 0)
            continue
        assert _pow_words(p, bits, dp) == 0
        with pytest.raises(TmxError) as e:
            pow_proof_words(p, bits, dp)
        assert e.value.status == BAD_ARG


@pytest.mark.parametrize("deep", [0, 1])
@pytest.mark.parametrize("bits", [1, 5, 12])
def test_model_checks_itself(oracle, bits, deep):
    """the model's own proof verifies; no candidate below the nonce satisfies the condition; the proof is rejected under pow_bits + 1 and
    pow_bits - 1; the next larger satisfying nonce in its place rejects every query (the indices move); nonce + p rejects.  Against the
    plain proof of the same inputs: every word in front of the indices is equal (the transcript is unchanged up to the final
    coefficients), the indices are not."""
    rng = np.random.default_rng(31 + bits + 100 * deep)
    p = params(8, 5, 2, 2, 2, 1, 8)
    shift = _shift()
    cols = _low_degree_cols(oracle, rng, p)
    cap = _cap_of(oracle, p, cols)
    proof, deg_ok, nonce = pw.prove(oracle, p, bits, deep, cols, shift)[:3]
    assert deg_ok and proof.size == pw.proof_words(p, deep) and int(proof[-1]) == nonce < 1 << (bits + pw.SLACK_BITS)
    assert all(pw.verify(oracle, p, bits, deep, cap, proof, shift))
    at = pw.grind_point(oracle, p, bits, deep, cap, proof, shift)
    rs = pw.candidates(oracle, at, 0, nonce + 1)
    assert pw.satisfies(rs[nonce], bits) and not any(pw.satisfies(r, bits) for r in rs[:nonce])
    assert not any(pw.verify(oracle, p, bits + 1, deep, cap, proof, shift))
    if bits > 1:
        assert not any(pw.verify(oracle, p, bits - 1, deep, cap, proof, shift))
    nxt = pw.search(oracle, at, bits, nonce + 1)
    assert nonce < nxt < pw.GAVE_UP
    for word in (nxt, nonce + P):
        bad = proof.copy()
        bad[-1] = np.uint64(word)
        assert not any(pw.verify(oracle, p, bits, deep, cap, bad, shift)), word
    plain = (dm if deep else fm).prove(oracle, p, cols, shift)[0]
    L = fm.layout(p)
    head = (dm.openings_words(p["n_cols"]) if deep else 0) + L["off_indices"]
    assert np.array_equal(proof[:head], plain[:head])
    assert not np.array_equal(proof[head:head + p["n_queries"]], plain[head:head + p["n_queries"]])
    # the plain verifier on the proof without its nonce: a different transcript; a query gets through only where it draws the same index
    same = [bool(a == b) for a, b in zip(proof[head:head + p["n_queries"]], plain[head:head + p["n_queries"]])]
    assert (dm if deep else fm).verify(oracle, p, cap, proof[:-1], shift) == same and not all(same)


# ---- GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


def _pprove(ctx, p, bits, deep, d_cols, d_lv, stream=0):
    d_proof = _sentinel(pw.proof_words(p, deep))
    ctx.pow_prove_device(p, bits, deep, d_cols.data_ptr(), d_lv.data_ptr(), d_proof.data_ptr(), stream)
    return d_proof


def _pverify(ctx, p, bits, deep, d_cap, d_proof, stream=0):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    ctx.pow_verify_device(p, bits, deep, d_cap.data_ptr(), d_proof.data_ptr(), ok.data_ptr(), stream)
    torch.cuda.synchronize(_dev())
    return ok.cpu().numpy()


def _plain_verify(ctx, p, deep, d_cap, d_proof):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    (ctx.deep_verify_device if deep else ctx.fri_verify_device)(p, d_cap.data_ptr(), d_proof.data_ptr(), ok.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    return ok.cpu().numpy()


@pytest.fixture(scope="module")
def ctx(built_lib):
    import tendermintx_amd as tmx
    c = tmx.Context(4, b"celestia")
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CALLER_CASES, ids=_case_id)
def test_caller_columns_equal_the_model(ctx, oracle, case):
    """LDE'd random columns with non-canonical words w + p in column 0 (a constant): the device proof equals the model's word for word,
    tmx_pow_last's nonce is the proof's last word and the model's, every query verifies on the device and in the model"""
    deep, p, bits = case
    rng = np.random.default_rng(p["log_n"] * 137 + p["n_cols"] + bits)
    n = 1 << (p["log_n"] - p["log_blowup"])
    base = rng.integers(0, P, (p["n_cols"], n), dtype=np.uint64)
    base[0] = 2468
    ext = oracle.lde(base, p["log_blowup"]).reshape(p["n_cols"], -1).copy()
    ext[0, ::3] += np.uint64(P)
    d_cols = _up(ext)
    d_lv, d_cap = _tree(ctx, p, d_cols)
    d_proof = _pprove(ctx, p, bits, deep, d_cols, d_lv)
    nonce, tried = ctx.pow_last()
    assert ctx.fri_last_degree_ok()
    got = _down(d_proof)
    want, deg, want_nonce = pw.prove(oracle, p, bits, deep, ext, _shift())[:3]
    assert deg and nonce == int(got[-1]) == want_nonce and nonce < tried <= 1 << (bits + pw.SLACK_BITS), (nonce, want_nonce, tried)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert (_pverify(ctx, p, bits, deep, d_cap, d_proof) == 1).all()
    assert all(pw.verify(oracle, p, bits, deep, _down(d_cap), got, _shift()))


@pytest.mark.gpu
@pytest.mark.parametrize("deep", [0, 1])
@pytest.mark.parametrize("kind,n,P_,sections", [(0, 4, 3, (1, 2, 4, 16, 32)), (1, 4, 2, (2, 32)), (0, 32, 2, (2, 4, 16))])
def test_last_commit_equals_the_model(built_lib, oracle, kind, n, P_, sections, deep):
    """trace rows -> tmx_trace_commit_device -> tmx_trace_commit_pow_device: the model's proof over the oracle chain's extension, one
    pow_bits per section; it verifies; the commit's openings after the prove equal those before it"""
    import torch
    import tendermintx_amd as tmx
    log_blowup, cap_h = 3, 2
    with tmx.Context(n, b"celestia", max_batch=P_) as ctx:
        tr = _trace_rows(ctx, kind, n, P_, 1300 + n + kind)
        traces = _down(tr)
        for k, sec in enumerate(sections):
            bits = (3, 9, 6, 11, 2)[k]
            cap = _sentinel(4 << cap_h)
            ctx.trace_commit_device(kind, P_, sec, log_blowup, cap_h, tr.data_ptr(), cap.data_ptr(), 0)
            log_m, n_cols, _ = ctx.trace_commit_last_shape()
            p = params(log_m, n_cols, cap_h, log_blowup, 1 + sec % 4, 2, 12)
            idx = [0, 5, (1 << log_m) - 1, 77 % (1 << log_m)]
            before = _sentinel(len(idx) * n_cols), _sentinel(len(idx) * (log_m - cap_h) * 4)
            ctx.trace_commit_open_device(idx, before[0].data_ptr(), before[1].data_ptr(), 0)
            d_proof = _sentinel(pw.proof_words(p, deep))
            ctx.trace_commit_pow_device(p, bits, deep, d_proof.data_ptr(), 0)
            nonce, _ = ctx.pow_last()
            after = _sentinel(len(idx) * n_cols), _sentinel(len(idx) * (log_m - cap_h) * 4)
            ctx.trace_commit_open_device(idx, after[0].data_ptr(), after[1].data_ptr(), 0)
            ok = _pverify(ctx, p, bits, deep, cap, d_proof)
            assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]), sec
            assert (ok == 1).all(), (sec, ok)
            assert ctx.fri_last_degree_ok(), sec
            ext, lm, nc = _oracle_ext(oracle, kind, n, traces, sec, log_blowup)
            assert (lm, nc) == (log_m, n_cols)
            want, deg, want_nonce = pw.prove(oracle, p, bits, deep, ext.reshape(nc, -1), _shift())[:3]
            got = _down(d_proof)
            assert deg and nonce == want_nonce and np.array_equal(got, want), (sec, nonce, want_nonce, np.flatnonzero(got != want)[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("bits,deep,p", [(20, 0, params(8, 3, 1, 1, 1, 2, 8)), (20, 1, params(9, 6, 2, 2, 2, 1, 8)),
                                         (24, 0, params(9, 6, 2, 2, 2, 1, 8)), (24, 1, params(8, 3, 1, 1, 1, 2, 8))],
                         ids=lambda v: str(v) if not isinstance(v, dict) else f"{v['log_n']}x{v['n_cols']}")
def test_long_searches(ctx, oracle, bits, deep, p):
    """20 and 24 bits, device search only: the device verifier accepts every query, the model's verifier accepts the same proof (one
    permutation, no search), and the search stayed inside its bound"""
    rng = np.random.default_rng(bits * 7 + deep)
    d_cols = _up(_low_degree_cols(oracle, rng, p))
    d_lv, d_cap = _tree(ctx, p, d_cols)
    d_proof = _pprove(ctx, p, bits, deep, d_cols, d_lv)
    nonce, tried = ctx.pow_last()
    got = _down(d_proof)
    print(f"pow_bits {bits} deep {deep}: nonce {nonce}, tried {tried}")
    assert nonce == int(got[-1]) and nonce < tried <= 1 << (bits + pw.SLACK_BITS)
    assert (_pverify(ctx, p, bits, deep, d_cap, d_proof) == 1).all()
    assert all(pw.verify(oracle, p, bits, deep, _down(d_cap), got, _shift()))


@pytest.mark.gpu
@pytest.mark.parametrize("deep", [0, 1])
@pytest.mark.parametrize("p", [params(9, 6, 2, 2, 2, 1, 8), params(8, 3, 1, 1, 1, 2, 8), params(10, 20, 3, 3, 4, 2, 8)],
                         ids=lambda v: f"{v['log_n']}x{v['n_cols']}")
def test_tampering_query_by_query(ctx, oracle, p, deep):
    """the nonce altered (+- 1, + p, 2^64 - 1), the proof verified under pow_bits +- 1, a grinding proof without its nonce given to the
    plain verifier, a plain proof with a word appended given to the grinding verifier: every query fails.  The tamper cases of
    tests/test_fri.py / tests/test_deep.py on a grinding proof: the queries the model rejects, and only those.  Device verdicts equal the
    model's in every case."""
    bits = 6
    rng = np.random.default_rng(29 + p["log_n"] + deep)
    d_cols = _up(_low_degree_cols(oracle, rng, p))
    d_lv, d_cap = _tree(ctx, p, d_cols)
    proof = _down(_pprove(ctx, p, bits, deep, d_cols, d_lv))
    cap, shift = _down(d_cap), _shift()
    nonce = int(proof[-1])
    assert (_pverify(ctx, p, bits, deep, d_cap, _up(proof)) == 1).all()
    for name, word in (("nonce + 1", nonce + 1), ("nonce - 1", (nonce - 1) % 2**64), ("nonce + p", nonce + P), ("nonce 2^64 - 1", 2**64 - 1)):
        bad = proof.copy()
        bad[-1] = np.uint64(word)
        assert (_pverify(ctx, p, bits, deep, d_cap, _up(bad)) == 0).all(), name
        assert not any(pw.verify(oracle, p, bits, deep, cap, bad, shift)), name
    for other in (bits + 1, bits - 1):
        assert (_pverify(ctx, p, other, deep, d_cap, _up(proof)) == 0).all(), other
        assert not any(pw.verify(oracle, p, other, deep, cap, proof, shift)), other
    assert (_plain_verify(ctx, p, deep, d_cap, _up(proof[:-1])) == 0).all()
    assert not any((dm if deep else fm).verify(oracle, p, cap, proof[:-1], shift))
    d_plain = _sentinel(pw.proof_words(p, deep) - 1)
    (ctx.deep_prove_device if deep else ctx.fri_prove_device)(p, d_cols.data_ptr(), d_lv.data_ptr(), d_plain.data_ptr(), 0)
    plain = _down(d_plain)
    assert (_plain_verify(ctx, p, deep, d_cap, d_plain) == 1).all()
    for word in (0, nonce):
        padded = np.concatenate([plain, np.array([word], dtype=np.uint64)])
        assert (_pverify(ctx, p, bits, deep, d_cap, _up(padded)) == 0).all(), word
        assert not any(pw.verify(oracle, p, bits, deep, cap, padded, shift)), word
    cases = _plain_tampers(p, deep, proof[:-1])
    assert {"init row", "index", "final coefficient"} <= {c[0] for c in cases}
    for name, bad, fails in cases:
        bad = np.concatenate([bad, proof[-1:]])
        want = np.array([0 if (fails is None or q in fails) else 1 for q in range(p["n_queries"])])
        assert np.array_equal(_pverify(ctx, p, bits, deep, d_cap, _up(bad)), want), name
        assert pw.verify(oracle, p, bits, deep, cap, bad, shift) == [bool(x) for x in want], name
    bad_cap = cap.copy()
    bad_cap[5] = np.uint64((int(bad_cap[5]) + 1) % P)
    assert (_pverify(ctx, p, bits, deep, _up(bad_cap), _up(proof)) == 0).all()
    assert not any(pw.verify(oracle, p, bits, deep, bad_cap, proof, shift))


@pytest.mark.gpu
@pytest.mark.parametrize("deep", [0, 1])
def test_injected_constants_and_domain(built_lib, oracle, deep):
    """injected Poseidon constants and the g = 7 domain: the search runs the context's CURRENT permutation, so the proof equals the model
    under the same tables and domain; verified under the default constants it is rejected on every query"""
    import poseidon_model as pm
    import tendermintx_amd as tmx
    rng = np.random.default_rng(79 + deep)
    rc = [int(x) % P for x in rng.integers(0, 2**63, 360, dtype=np.uint64)]
    p, bits = params(9, 5, 2, 2, 3, 2, 12), 10
    root, shift = oracle.G7_DOMAIN
    with tmx.Context(4, b"celestia") as ctx:
        ctx.poseidon_set_constants(rc, pm.MDS_CIRC, pm.MDS_DIAG)
        ctx.ntt_set_domain(root, shift)
        try:
            oracle.poseidon_set_constants(rc, pm.MDS_CIRC, pm.MDS_DIAG)
            oracle.ntt_set_domain(root, shift)
            cols = _low_degree_cols(oracle, rng, p)
            d_cols = _up(cols)
            d_lv, d_cap = _tree(ctx, p, d_cols)
            d_proof = _pprove(ctx, p, bits, deep, d_cols, d_lv)
            want, deg, want_nonce = pw.prove(oracle, p, bits, deep, cols, shift)[:3]
            assert deg and ctx.fri_last_degree_ok() and ctx.pow_last()[0] == want_nonce
            assert np.array_equal(_down(d_proof), want)
            assert (_pverify(ctx, p, bits, deep, d_cap, d_proof) == 1).all()
        finally:
            oracle.poseidon_set_constants(pm.grain_constants(), pm.MDS_CIRC, pm.MDS_DIAG)
            oracle.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
        ctx.poseidon_set_constants(pm.grain_constants(), pm.MDS_CIRC, pm.MDS_DIAG)
        assert (_pverify(ctx, p, bits, deep, d_cap, d_proof) == 0).all()


@pytest.mark.gpu
def test_lifecycle_and_arguments(built_lib, oracle):
    """every refusal leaves sentinel-filled buffers unchanged: the grinding prove over the last commit on a fresh context and on a shape
    mismatch, and every validation rule (pow_bits 0 and 25, deep 2, the inherited ones) at each entry point; tmx_pow_last is refused
    before any prove and after a plain prove; after a grinding prove tmx_fri_last_degree_ok, tmx_fri_last_ms and (deep) tmx_deep_last_zeta
    answer"""
    import torch
    import tendermintx_amd as tmx
    from tendermintx_amd._lib import TmxError
    kind, n, P_, log_blowup, cap_h = 1, 4, 2, 2, 1

    def refused(fn, *outs):
        before = [o.clone() for o in outs]
        with pytest.raises(TmxError) as e:
            fn()
        torch.cuda.synchronize(_dev())
        assert e.value.status == BAD_ARG, e.value
        for a, b in zip(outs, before):
            assert torch.equal(a, b)
        return str(e.value)

    with tmx.Context(n, b"celestia", max_batch=P_) as ctx:
        proof = _sentinel(1 << 16)
        p0 = params(9, 18, cap_h, log_blowup, 2, 2, 8)
        for deep in (0, 1):
            assert "no commit" in refused(lambda: ctx.trace_commit_pow_device(p0, 8, deep, proof.data_ptr(), 0), proof)
        refused(lambda: ctx.pow_last())
        tr = _trace_rows(ctx, kind, n, P_, 930)
        cap = _sentinel(4 << cap_h)
        ctx.trace_commit_device(kind, P_, 2, log_blowup, cap_h, tr.data_ptr(), cap.data_ptr(), 0)
        log_m, n_cols, _ = ctx.trace_commit_last_shape()
        p = params(log_m, n_cols, cap_h, log_blowup, 2, 2, 8)
        for field, delta in (("log_n", -1), ("n_cols", 1), ("cap_height", 1), ("log_blowup", 1)):
            refused(lambda: ctx.trace_commit_pow_device(dict(p, **{field: p[field] + delta}), 8, 0, proof.data_ptr(), 0), proof)
        ok = torch.full((8,), 7, dtype=torch.int32, device=_dev())
        rules = [(p, 0, 0), (p, 25, 1), (p, 8, 2)]
        rules += [(dict(p, **{f: v}), 8, d) for d in (0, 1) for f, v in (("log_blowup", 0), ("log_n", 29), ("arity_bits", 5), ("n_queries", 257),
                                                                          ("final_log_max", 9), ("cap_height", log_m + 1), ("n_cols", 0),
                                                                          ("reserved", 1))]
        rules.append((dict(p, n_cols=(1 << 24) + 1), 8, 1))
        for bad, bits, deep in rules:
            refused(lambda: ctx.trace_commit_pow_device(bad, bits, deep, proof.data_ptr(), 0), proof)
            refused(lambda: ctx.pow_prove_device(bad, bits, deep, proof.data_ptr(), proof.data_ptr(), proof.data_ptr(), 0), proof)
            refused(lambda: ctx.pow_verify_device(bad, bits, deep, cap.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0), ok)
        refused(lambda: ctx.pow_last())
        ctx.trace_commit_fri_device(p, proof.data_ptr(), 0)
        refused(lambda: ctx.pow_last())
        for deep in (0, 1):
            ctx.trace_commit_pow_device(p, 8, deep, proof.data_ptr(), 0)
            nonce, tried = ctx.pow_last()
            assert (_pverify(ctx, p, 8, deep, cap, proof) == 1).all() and ctx.fri_last_degree_ok()
            assert nonce == int(_down(proof)[pw.proof_words(p, deep) - 1]) and nonce < tried <= 1 << 14
            ms = ctx.fri_last_ms()
            assert set(ms) == {"combine", "layers", "final", "openings"} and all(v >= 0 for v in ms.values())
            if deep:
                assert ctx.deep_last_zeta()[1] != 0
            else:
                refused(lambda: ctx.deep_last_zeta())
        ctx.trace_commit_deep_device(p, proof.data_ptr(), 0)
        refused(lambda: ctx.pow_last())


@pytest.mark.gpu
def test_stream_ordering(built_lib):
    """commit -> grinding DEEP -> grinding FRI -> verify on one non-default stream with no host synchronisation between them: every
    result equals the same call run alone on the default stream"""
    import torch
    import tendermintx_amd as tmx
    kind, n, P_, sec, log_blowup, cap_h = 0, 4, 3, 16, 3, 2
    with tmx.Context(n, b"celestia", max_batch=P_) as ctx:
        tr = _trace_rows(ctx, kind, n, P_, 987)
        cap = _sentinel(4 << cap_h)
        ctx.trace_commit_device(kind, P_, sec, log_blowup, cap_h, tr.data_ptr(), cap.data_ptr(), 0)
        log_m, n_cols, _ = ctx.trace_commit_last_shape()
        p1 = params(log_m, n_cols, cap_h, log_blowup, 3, 2, 16)
        p2 = params(log_m, n_cols, cap_h, log_blowup, 2, 1, 9)
        alone = [_sentinel(pw.proof_words(p1, 1)), _sentinel(pw.proof_words(p2, 0))]
        ctx.trace_commit_pow_device(p1, 10, 1, alone[0].data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        ctx.trace_commit_pow_device(p2, 7, 0, alone[1].data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        s = torch.cuda.Stream(_dev())
        cap_s = _sentinel(4 << cap_h)
        got = [_sentinel(pw.proof_words(p1, 1)), _sentinel(pw.proof_words(p2, 0))]
        ok = torch.full((p2["n_queries"],), 7, dtype=torch.int32, device=_dev())
        torch.cuda.synchronize(_dev())
        with torch.cuda.stream(s):
            ctx.trace_commit_device(kind, P_, sec, log_blowup, cap_h, tr.data_ptr(), cap_s.data_ptr(), s.cuda_stream)
            ctx.trace_commit_pow_device(p1, 10, 1, got[0].data_ptr(), s.cuda_stream)
            ctx.trace_commit_pow_device(p2, 7, 0, got[1].data_ptr(), s.cuda_stream)
            ctx.pow_verify_device(p2, 7, 0, cap_s.data_ptr(), got[1].data_ptr(), ok.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert torch.equal(cap, cap_s)
        for a, b in zip(alone, got):
            assert torch.equal(a, b)
        assert (ok.cpu().numpy() == 1).all()
        assert ctx.pow_last()[0] == int(_down(got[1])[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("deep", [0, 1])
def test_plain_grinding_plain(ctx, oracle, deep):
    """a plain prove, a grinding prove and a plain prove again on one context: the first and third proofs are equal word for word"""
    import torch
    p = params(10, 9, 3, 2, 3, 2, 10)
    rng = np.random.default_rng(97 + deep)
    d_cols = _up(_low_degree_cols(oracle, rng, p))
    d_lv, d_cap = _tree(ctx, p, d_cols)
    plain = ctx.deep_prove_device if deep else ctx.fri_prove_device
    first, third = _sentinel(pw.proof_words(p, deep) - 1), _sentinel(pw.proof_words(p, deep) - 1)
    plain(p, d_cols.data_ptr(), d_lv.data_ptr(), first.data_ptr(), 0)
    mid = _pprove(ctx, p, 9, deep, d_cols, d_lv)
    plain(p, d_cols.data_ptr(), d_lv.data_ptr(), third.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    assert torch.equal(first, third)
    assert (_plain_verify(ctx, p, deep, d_cap, third) == 1).all() and (_pverify(ctx, p, 9, deep, d_cap, mid) == 1).all()
    head = (dm.openings_words(p["n_cols"]) if deep else 0) + fm.layout(p)["off_indices"]
    assert torch.equal(first[:head], mid[:head]) and not torch.equal(first[head:head + p["n_queries"]], mid[head:head + p["n_queries"]])
