"""Out-of-domain openings with DEEP-FRI (include/tmx.h "out-of-domain openings"): tmx_deep_openings_words, tmx_deep_prove_device,
tmx_trace_commit_deep_device, tmx_deep_verify_device, tmx_deep_last_zeta.  The yardstick is tests/deep_model.py, a pure-Python model whose
openings come from interpolation and Horner, not from the barycentric form the device uses: device proofs must equal the model's word for
word, and every verdict of the device verifier must equal the model verifier's."""
import numpy as np
import pytest

import deep_model as dm
import fri_model as fm
from test_fri import _down, _low_degree_cols, _sentinel, _shift, _tamper_cases, _tree, _up, params
from test_merkle_open import _oracle_ext, _section_geom, _trace_rows

P = fm.P
BAD_ARG = -1


def _horner(coef, z):
    acc = (0, 0)
    for c in reversed(coef):
        acc = fm.e_add(fm.e_mul(acc, z), (int(c) % P, 0))
    return acc


def _ext_from_coefs(oracle, coef, log_blowup, shift):
    """columns of the polynomials with these coefficients ([n_cols][N]) evaluated on shift <gl_root(log N + log_blowup)>"""
    n_cols, N = coef.shape
    M = N << log_blowup
    scaled = np.zeros((n_cols, M), dtype=np.uint64)
    for c in range(n_cols):
        scaled[c, :N] = [int(x) * pow(shift, k, P) % P for k, x in enumerate(coef[c])]
    return oracle.ntt(scaled)


def _with_section(sec, fri_part):
    return np.concatenate([sec, fri_part])


def _deep_tamper_cases(p, proof):
    """(name, tampered proof, queries that must fail or None = all): the FRI part's cases of tests/test_fri.py, an opening, a padding word"""
    R = 1 << dm.log_r(p["n_cols"])
    sec, fri_part = proof[:4 * R], proof[4 * R:]
    out = [(name, _with_section(sec, bad), fails) for name, bad, fails in _tamper_cases(p, fri_part)]
    bad = proof.copy()
    bad[2 * R + p["n_cols"] - 1] = np.uint64((int(bad[2 * R + p["n_cols"] - 1]) + 1) % P)
    out.append(("opening", bad, None))
    if R > p["n_cols"]:
        bad = proof.copy()
        bad[3 * R + R - 1] = np.uint64(1)
        out.append(("padding word", bad, None))
    return out


# ---- CPU
@pytest.mark.parametrize("n_cols", [1, 3, 4, 9, 4608, 1 << 24])
def test_openings_words_equal_the_model(built_lib, n_cols):
    from tendermintx_amd.context import deep_openings_words
    assert deep_openings_words(n_cols) == dm.openings_words(n_cols) == 4 << max(0, (n_cols - 1).bit_length())


@pytest.mark.parametrize("n_cols", [0, (1 << 24) + 1, 1 << 30, 0xFFFFFFFF])
def test_openings_words_refuse(built_lib, n_cols):
    from tendermintx_amd.context import deep_openings_words
    assert deep_openings_words(n_cols) == 0


def test_proof_words_equal_the_model(built_lib):
    from tendermintx_amd.context import deep_proof_words
    for p in (params(9, 5, 1, 2, 3, 1, 7), params(6, 3, 2, 2, 2, 5, 4), params(28, 4608, 4, 3, 4, 5, 28)):
        assert deep_proof_words(p) == dm.proof_words(p)


@pytest.mark.parametrize("field,value", [("log_blowup", 0), ("log_blowup", 7), ("log_n", 3), ("log_n", 29), ("n_cols", 0), ("n_cols", (1 << 24) + 1),
                                         ("cap_height", 11), ("arity_bits", 0), ("arity_bits", 5), ("final_log_max", 9), ("n_queries", 0),
                                         ("n_queries", 257), ("reserved", 1)])
def test_proof_words_refuse_each_rule(built_lib, field, value):
    """each validation rule on its own, host side (the device entry points are checked rule by rule in the lifecycle test): the DEEP proof
    size is refused for every rule of FRI plus n_cols <= 2^24, while the base parameters are accepted"""
    from tendermintx_amd.context import deep_proof_words
    from tendermintx_amd._lib import TmxError
    p = dict(params(10, 4, 2, 3, 2, 4, 8), reserved=0)
    assert deep_proof_words(p) == dm.proof_words(p)
    p[field] = value
    with pytest.raises(TmxError) as e:
        deep_proof_words(p)
    assert e.value.status == BAD_ARG


def test_model_checks_itself(oracle):
    """the model's honest proof verifies; its openings equal Horner on polynomials built from known coefficients; a changed opening or
    padding word rejects every query; an opening stored as y + p still verifies; a changed row rejects only its own query"""
    rng = np.random.default_rng(13)
    p = params(8, 5, 2, 2, 2, 1, 8)
    N, shift = 1 << (p["log_n"] - p["log_blowup"]), _shift()
    coef = rng.integers(0, P, (p["n_cols"], N), dtype=np.uint64)
    coef[0, 1:] = 0
    coef[0, 0] = 12345  # a constant column: its openings are (12345, 0)
    cols = _ext_from_coefs(oracle, coef, p["log_blowup"], shift)
    proof, deg_ok, zeta = dm.prove(oracle, p, cols, shift)
    cap = oracle.poseidon_merkle(cols.reshape(-1), p["log_n"], p["n_cols"], p["cap_height"])[-(1 << p["cap_height"]):]
    assert deg_ok and all(dm.verify(oracle, p, cap, proof, shift))
    zs = dm.points(oracle, p, zeta)
    assert dm.openings_of(p, proof) == [(_horner(coef[c], zs[0]), _horner(coef[c], zs[1])) for c in range(p["n_cols"])]
    for name, bad, fails in _deep_tamper_cases(p, proof):
        want = [not (fails is None or q in fails) for q in range(p["n_queries"])]
        assert dm.verify(oracle, p, cap, bad, shift) == want, name
    R = 1 << dm.log_r(p["n_cols"])
    alt = proof.copy()
    assert int(alt[R]) == 0 and int(alt[0]) == 12345
    alt[R] = np.uint64(P)
    alt[0] = np.uint64(12345 + P)
    assert all(dm.verify(oracle, p, cap, alt, shift))
    assert not any(fm.verify(oracle, p, cap, proof[4 * R:], shift))  # the FRI verifier on the FRI part: a different transcript


# ---- GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


def _dprove(ctx, p, d_cols, d_lv, stream=0):
    d_proof = _sentinel(dm.proof_words(p))
    ctx.deep_prove_device(p, d_cols.data_ptr(), d_lv.data_ptr(), d_proof.data_ptr(), stream)
    return d_proof


def _dverify(ctx, p, d_cap, d_proof, stream=0, fri=False):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    (ctx.fri_verify_device if fri else ctx.deep_verify_device)(p, d_cap.data_ptr(), d_proof.data_ptr(), ok.data_ptr(), stream)
    torch.cuda.synchronize(_dev())
    return ok.cpu().numpy()


@pytest.fixture(scope="module")
def ctx(built_lib):
    import tendermintx_amd as tmx
    c = tmx.Context(4, b"celestia")
    yield c
    c.close()


# n_cols 1, 3, 5, 9 and powers of two; zero layers (6, 3, ...); arities 1 .. 4
CALLER_GRID = [params(6, 3, 2, 2, 2, 5, 4), params(9, 5, 1, 2, 3, 1, 7), params(8, 4, 3, 1, 1, 2, 5), params(10, 9, 6, 2, 4, 0, 3),
               params(9, 1, 2, 3, 3, 2, 16), params(7, 1, 7, 3, 2, 0, 1), params(11, 64, 4, 3, 4, 5, 28), params(12, 2, 0, 1, 3, 3, 40)]


@pytest.mark.gpu
@pytest.mark.parametrize("p", CALLER_GRID)
def test_caller_columns_equal_the_model(ctx, oracle, p):
    """(1) LDE'd random columns with non-canonical words w + p in column 0 (a constant): the device proof equals the model's word for word,
    every query verifies on the device and in the model, and zeta is the model's"""
    rng = np.random.default_rng(p["log_n"] * 131 + p["n_cols"])
    n = 1 << (p["log_n"] - p["log_blowup"])
    base = rng.integers(0, P, (p["n_cols"], n), dtype=np.uint64)
    base[0] = 4321
    ext = oracle.lde(base, p["log_blowup"]).reshape(p["n_cols"], -1).copy()
    ext[0, ::3] += np.uint64(P)
    d_cols = _up(ext)
    d_lv, d_cap = _tree(ctx, p, d_cols)
    d_proof = _dprove(ctx, p, d_cols, d_lv)
    assert ctx.fri_last_degree_ok()
    want, deg, zeta = dm.prove(oracle, p, ext, _shift())
    got = _down(d_proof)
    assert deg and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert ctx.deep_last_zeta() == zeta
    assert (_dverify(ctx, p, d_cap, d_proof) == 1).all()
    assert all(dm.verify(oracle, p, _down(d_cap), got, _shift()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,P_,sections", [(0, 4, 3, (1, 2, 4, 16, 32)), (1, 4, 2, (2, 32)), (0, 32, 2, (2, 4, 16))])
def test_last_commit_equals_the_model(built_lib, oracle, kind, n, P_, sections):
    """(2) trace rows -> tmx_trace_commit_device -> tmx_trace_commit_deep_device: the model's proof over the oracle chain's extension; it
    verifies; the commit's openings and a plain FRI proof taken after the DEEP prove equal those taken before it.  (3) the openings equal the
    oracle's trace-column polynomials (interpolated from the pre-LDE columns) at the tmx_deep_last_zeta() points."""
    import torch
    import tendermintx_amd as tmx
    log_blowup, cap_h = 3, 2
    with tmx.Context(n, b"celestia", max_batch=P_) as ctx:
        tr = _trace_rows(ctx, kind, n, P_, 700 + n + kind)
        traces = _down(tr)
        for sec in sections:
            cap = _sentinel(4 << cap_h)
            ctx.trace_commit_device(kind, P_, sec, log_blowup, cap_h, tr.data_ptr(), cap.data_ptr(), 0)
            log_m, n_cols, _ = ctx.trace_commit_last_shape()
            p = params(log_m, n_cols, cap_h, log_blowup, 1 + sec % 4, 2, 12)
            idx = [0, 5, (1 << log_m) - 1, 77 % (1 << log_m)]
            opened = [_sentinel(len(idx) * n_cols), _sentinel(len(idx) * (log_m - cap_h) * 4)]
            ctx.trace_commit_open_device(idx, opened[0].data_ptr(), opened[1].data_ptr(), 0)
            fri_before = _sentinel(fm.layout(p)["words"])
            ctx.trace_commit_fri_device(p, fri_before.data_ptr(), 0)
            d_proof = _sentinel(dm.proof_words(p))
            ctx.trace_commit_deep_device(p, d_proof.data_ptr(), 0)
            zeta = ctx.deep_last_zeta()
            assert ctx.fri_last_degree_ok(), sec
            after = [_sentinel(len(idx) * n_cols), _sentinel(len(idx) * (log_m - cap_h) * 4)]
            ctx.trace_commit_open_device(idx, after[0].data_ptr(), after[1].data_ptr(), 0)
            fri_after = _sentinel(fm.layout(p)["words"])
            ctx.trace_commit_fri_device(p, fri_after.data_ptr(), 0)
            ok = _dverify(ctx, p, cap, d_proof)
            torch.cuda.synchronize(_dev())
            assert torch.equal(opened[0], after[0]) and torch.equal(opened[1], after[1]), sec
            assert torch.equal(fri_before, fri_after), sec
            assert (ok == 1).all(), (sec, ok)
            ext, lm, nc = _oracle_ext(oracle, kind, n, traces, sec, log_blowup)
            assert (lm, nc) == (log_m, n_cols)
            want, deg, wz = dm.prove(oracle, p, ext.reshape(nc, -1), _shift())
            got = _down(d_proof)
            assert deg and wz == zeta and np.array_equal(got, want), (sec, np.flatnonzero(got != want)[:10])
            # (3) the trace columns themselves (natural rows, zero padded), interpolated on the trace domain
            off, rows, width = _section_geom(kind, n, sec)
            cols = np.zeros((nc, 1 << (log_m - log_blowup)), dtype=np.uint64)
            for q, full in enumerate(traces):
                cols[q * width:(q + 1) * width, :rows] = full[off:off + rows * width].reshape(rows, width).T
            pick = sorted({0, nc // 2, nc - 1})
            zs = dm.points(oracle, p, zeta)
            assert [dm.openings_of(p, got)[c] for c in pick] == [tuple(y) for y in dm.evaluate(oracle, cols[pick], 1, zs)], sec


@pytest.mark.gpu
@pytest.mark.parametrize("p", [params(9, 6, 2, 2, 2, 1, 8), params(8, 3, 1, 1, 1, 2, 8), params(10, 20, 3, 3, 4, 2, 8)])
def test_tampering_query_by_query(ctx, oracle, p):
    """(4) an opening, a padding word, a layer cap, a final coefficient or the commit cap altered: every query fails; one word of one
    query's initial row / initial path / layer row / layer path / index: only that query.  The model verifier agrees in every case, and the
    plain FRI verifier rejects every query of the DEEP proof's FRI part."""
    rng = np.random.default_rng(19 + p["log_n"])
    d_cols = _up(_low_degree_cols(oracle, rng, p))
    d_lv, d_cap = _tree(ctx, p, d_cols)
    proof = _down(_dprove(ctx, p, d_cols, d_lv))
    cap = _down(d_cap)
    assert (_dverify(ctx, p, d_cap, _up(proof)) == 1).all()
    cases = _deep_tamper_cases(p, proof)
    assert "padding word" in [c[0] for c in cases]
    for name, bad, fails in cases:
        want = np.array([0 if (fails is None or q in fails) else 1 for q in range(p["n_queries"])])
        assert np.array_equal(_dverify(ctx, p, d_cap, _up(bad)), want), name
        assert dm.verify(oracle, p, cap, bad, _shift()) == [bool(x) for x in want], name
    bad_cap = cap.copy()
    bad_cap[5] = np.uint64((int(bad_cap[5]) + 1) % P)
    assert (_dverify(ctx, p, _up(bad_cap), _up(proof)) == 0).all()
    assert not any(dm.verify(oracle, p, bad_cap, proof, _shift()))
    R = 1 << dm.log_r(p["n_cols"])
    assert (_dverify(ctx, p, d_cap, _up(proof[4 * R:]), fri=True) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("p", [params(9, 3, 2, 3, 2, 2, 10), params(8, 2, 1, 1, 3, 0, 10)])
def test_degree_edge(ctx, oracle, p):
    """(5) a column of degree exactly N: the degree flag is 0 and the proof still equals the model's"""
    rng = np.random.default_rng(67)
    M, N = 1 << p["log_n"], 1 << (p["log_n"] - p["log_blowup"])
    coef = np.zeros((p["n_cols"], M), dtype=np.uint64)
    coef[:, :N + 1] = rng.integers(1, P, (p["n_cols"], N + 1), dtype=np.uint64)
    cols = _ext_from_coefs(oracle, coef, 0, _shift())
    d_cols = _up(cols)
    d_lv, _ = _tree(ctx, p, d_cols)
    d_proof = _dprove(ctx, p, d_cols, d_lv)
    assert ctx.fri_last_degree_ok() is False
    want, deg, _ = dm.prove(oracle, p, cols, _shift())
    assert not deg and np.array_equal(_down(d_proof), want)


@pytest.mark.gpu
def test_injected_constants_and_domain(built_lib, oracle):
    """(6) injected Poseidon constants and the g = 7 domain: the proof equals the model under the same tables and domain; after the
    constants change, the old proof fails verification on every query"""
    import poseidon_model as pm
    import tendermintx_amd as tmx
    rng = np.random.default_rng(73)
    rc = [int(x) % P for x in rng.integers(0, 2**63, 360, dtype=np.uint64)]
    p = params(9, 5, 2, 2, 3, 2, 12)
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
            d_proof = _dprove(ctx, p, d_cols, d_lv)
            want, deg, _ = dm.prove(oracle, p, cols, shift)
            assert deg and ctx.fri_last_degree_ok()
            assert np.array_equal(_down(d_proof), want)
            assert (_dverify(ctx, p, d_cap, d_proof) == 1).all()
        finally:
            oracle.poseidon_set_constants(pm.grain_constants(), pm.MDS_CIRC, pm.MDS_DIAG)
            oracle.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
        ctx.poseidon_set_constants(pm.grain_constants(), pm.MDS_CIRC, pm.MDS_DIAG)
        assert (_dverify(ctx, p, d_cap, d_proof) == 0).all()


@pytest.mark.gpu
def test_lifecycle_and_arguments(built_lib, oracle):
    """(7) DEEP over the last commit is refused on a fresh context, after a failed commit and on a shape mismatch; every validation rule
    (n_cols <= 2^24 included) is refused by each entry point; refused calls leave a sentinel-filled proof untouched; tmx_deep_last_zeta is
    refused with no prove and after a plain FRI prove"""
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
        assert "no commit" in refused(lambda: ctx.trace_commit_deep_device(p0, proof.data_ptr(), 0), proof)
        refused(lambda: ctx.deep_last_zeta())
        tr = _trace_rows(ctx, kind, n, P_, 910)
        cap = _sentinel(4 << cap_h)
        ctx.trace_commit_device(kind, P_, 2, log_blowup, cap_h, tr.data_ptr(), cap.data_ptr(), 0)
        log_m, n_cols, _ = ctx.trace_commit_last_shape()
        p = params(log_m, n_cols, cap_h, log_blowup, 2, 2, 8)
        for field, delta in (("log_n", -1), ("n_cols", 1), ("cap_height", 1), ("log_blowup", 1)):
            refused(lambda: ctx.trace_commit_deep_device(dict(p, **{field: p[field] + delta}), proof.data_ptr(), 0), proof)
        ok = torch.full((8,), 7, dtype=torch.int32, device=_dev())
        for field, value in (("log_blowup", 0), ("log_blowup", 7), ("log_n", 29), ("arity_bits", 0), ("arity_bits", 5), ("n_queries", 0),
                             ("n_queries", 257), ("final_log_max", 9), ("cap_height", log_m + 1), ("n_cols", 0), ("n_cols", (1 << 24) + 1),
                             ("reserved", 1)):
            bad = dict(p, **{field: value})
            refused(lambda: ctx.trace_commit_deep_device(bad, proof.data_ptr(), 0), proof)
            refused(lambda: ctx.deep_prove_device(bad, proof.data_ptr(), proof.data_ptr(), proof.data_ptr(), 0), proof)
            refused(lambda: ctx.deep_verify_device(bad, cap.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0), ok)
        ctx.trace_commit_deep_device(p, proof.data_ptr(), 0)
        assert (_dverify(ctx, p, cap, proof) == 1).all() and ctx.fri_last_degree_ok()
        z = ctx.deep_last_zeta()
        assert z[1] != 0
        fri_proof = _sentinel(fm.layout(p)["words"])
        ctx.trace_commit_fri_device(p, fri_proof.data_ptr(), 0)
        refused(lambda: ctx.deep_last_zeta())
        cap2 = _sentinel(4 << cap_h)
        with pytest.raises(TmxError):
            ctx.trace_commit_device(kind, P_, 8, log_blowup, cap_h, tr.data_ptr(), cap2.data_ptr(), 0)  # not a row table
        fresh = _sentinel(1 << 16)
        refused(lambda: ctx.trace_commit_deep_device(p, fresh.data_ptr(), 0), fresh)


@pytest.mark.gpu
def test_stream_ordering(built_lib):
    """(8) commit -> DEEP -> plain FRI -> DEEP on one non-default stream with no host synchronisation between them: every result equals the
    same call run alone on the default stream"""
    import torch
    import tendermintx_amd as tmx
    kind, n, P_, sec, log_blowup, cap_h = 0, 4, 3, 16, 3, 2
    with tmx.Context(n, b"celestia", max_batch=P_) as ctx:
        tr = _trace_rows(ctx, kind, n, P_, 977)
        cap = _sentinel(4 << cap_h)
        ctx.trace_commit_device(kind, P_, sec, log_blowup, cap_h, tr.data_ptr(), cap.data_ptr(), 0)
        log_m, n_cols, _ = ctx.trace_commit_last_shape()
        p1 = params(log_m, n_cols, cap_h, log_blowup, 3, 2, 16)
        p2 = params(log_m, n_cols, cap_h, log_blowup, 2, 1, 9)
        alone = [_sentinel(dm.proof_words(p1)), _sentinel(fm.layout(p2)["words"]), _sentinel(dm.proof_words(p2))]
        ctx.trace_commit_deep_device(p1, alone[0].data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        ctx.trace_commit_fri_device(p2, alone[1].data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        ctx.trace_commit_deep_device(p2, alone[2].data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        s = torch.cuda.Stream(_dev())
        cap_s = _sentinel(4 << cap_h)
        got = [_sentinel(dm.proof_words(p1)), _sentinel(fm.layout(p2)["words"]), _sentinel(dm.proof_words(p2))]
        ok = torch.full((p2["n_queries"],), 7, dtype=torch.int32, device=_dev())
        torch.cuda.synchronize(_dev())
        with torch.cuda.stream(s):
            ctx.trace_commit_device(kind, P_, sec, log_blowup, cap_h, tr.data_ptr(), cap_s.data_ptr(), s.cuda_stream)
            ctx.trace_commit_deep_device(p1, got[0].data_ptr(), s.cuda_stream)
            ctx.trace_commit_fri_device(p2, got[1].data_ptr(), s.cuda_stream)
            ctx.trace_commit_deep_device(p2, got[2].data_ptr(), s.cuda_stream)
            ctx.deep_verify_device(p2, cap_s.data_ptr(), got[2].data_ptr(), ok.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert torch.equal(cap, cap_s)
        for a, b in zip(alone, got):
            assert torch.equal(a, b)
        assert (ok.cpu().numpy() == 1).all()
        ms = ctx.fri_last_ms()
        assert set(ms) == {"combine", "layers", "final", "openings"} and all(v >= 0 for v in ms.values())
