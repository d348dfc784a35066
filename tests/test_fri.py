"""The batched FRI low-degree proof (include/tmx.h "a batched FRI low-degree proof"): tmx_fri_layout_of, tmx_fri_prove_device,
tmx_trace_commit_fri_device, tmx_fri_verify_device.  The yardstick is tests/fri_model.py, a pure-Python model over the CPU oracle: device
proofs must equal the model's word for word, and every verdict of the device verifier must equal the model verifier's.  Parity unpinned
against plonky2 (natural row order, no salt, injectable constants, the project's own transcript)."""
import numpy as np
import pytest

import fri_model as fm
from test_merkle_open import _oracle_ext, _trace_rows

P = fm.P
BAD_ARG = -1


def params(log_n, n_cols, cap_height, log_blowup, arity_bits, final_log_max, n_queries):
    return dict(log_n=log_n, n_cols=n_cols, cap_height=cap_height, log_blowup=log_blowup, arity_bits=arity_bits, final_log_max=final_log_max,
                n_queries=n_queries)


# zero layers; an uneven last arity; a_l = 2; cap_height above a layer's leaf log; arities 1 .. 4
LAYOUT_GRID = [params(6, 3, 2, 2, 2, 5, 4), params(9, 5, 1, 2, 3, 1, 7), params(8, 4, 3, 1, 1, 2, 5), params(10, 9, 6, 2, 4, 0, 3),
               params(12, 64, 4, 3, 4, 5, 28), params(7, 1, 7, 3, 2, 0, 1), params(11, 2, 0, 1, 3, 3, 256), params(28, 4608, 4, 3, 4, 5, 28),
               params(5, 3, 0, 4, 1, 8, 2)]


def _shift():
    import oracle_c
    return oracle_c.PLONKY2_DOMAIN[1]


def _low_degree_cols(oracle, rng, p):
    n = 1 << (p["log_n"] - p["log_blowup"])
    return oracle.lde(rng.integers(0, P, (p["n_cols"], n), dtype=np.uint64), p["log_blowup"])


# ---- CPU
@pytest.mark.parametrize("p", LAYOUT_GRID)
def test_layout_equals_the_model(built_lib, p):
    from tendermintx_amd.context import fri_layout
    assert fri_layout(p) == fm.layout(p)


def test_layout_grid_covers_the_edges():
    lay = [fm.layout(p) for p in LAYOUT_GRID]
    assert any(L["n_layers"] == 0 for L in lay)
    assert any(L["layer_bits"] and L["layer_bits"][-1] < p["arity_bits"] for p, L in zip(LAYOUT_GRID, lay))
    assert any(1 in L["layer_bits"] for L in lay)
    lg = lambda p, L, l: p["log_n"] - sum(L["layer_bits"][:l + 1])
    assert any(p["cap_height"] > lg(p, L, l) for p, L in zip(LAYOUT_GRID, lay) for l in range(L["n_layers"]))


@pytest.mark.parametrize("field,value", [("log_blowup", 0), ("log_blowup", 7), ("log_n", 3), ("log_n", 29), ("n_cols", 0), ("cap_height", 11),
                                         ("arity_bits", 0), ("arity_bits", 5), ("final_log_max", 9), ("final_log_max", None), ("n_queries", 0),
                                         ("n_queries", 257), ("reserved", 1)])
def test_layout_refuses_each_rule(built_lib, field, value):
    """each validation rule on its own (base: log_n 10, log_blowup 3; the None case breaks only final_log_max + log_blowup <= 12:
    final_log_max 8 with log_blowup 5)"""
    import ctypes as C
    from tendermintx_amd import _lib
    p = dict(params(10, 4, 2, 3, 2, 4, 8), reserved=0)
    if value is None:
        p["log_blowup"] = 5
        value = 8
    assert built_lib.tmx_fri_layout_of(C.byref(_lib.FriParams(**p)), C.byref(_lib.FriLayout())) == 0
    p[field] = value
    assert built_lib.tmx_fri_layout_of(C.byref(_lib.FriParams(**p)), C.byref(_lib.FriLayout())) == BAD_ARG


def _tamper_cases(p, proof, q_row=1, q_path=2, q_lrow=3, q_lpath=4, q_idx=5):
    """(name, tampered proof or None, tampered cap?, queries that must fail or None = all)"""
    L = fm.layout(p)
    nq, nc = p["n_queries"], p["n_cols"]
    bump = lambda a, at: (a.__setitem__(at, np.uint64((int(a[at]) % P + 1) % P)), a)[1]
    out = [("init row", bump(proof.copy(), L["off_init_rows"] + q_row * nc + nc - 1), {q_row})]
    pl0 = p["log_n"] - p["cap_height"]
    if pl0:
        out.append(("init path", bump(proof.copy(), L["off_init_paths"] + q_path * pl0 * 4 + 4 * (pl0 // 2) + 1), {q_path}))
    if L["n_layers"]:
        a = 1 << L["layer_bits"][0]
        out.append(("layer row", bump(proof.copy(), L["off_rows"][0] + q_lrow * 2 * a + a + 1), {q_lrow}))
        lg = p["log_n"] - L["layer_bits"][0]
        pl = lg - L["layer_cap_height"][0]
        if pl:
            out.append(("layer path", bump(proof.copy(), L["off_paths"][0] + q_lpath * pl * 4 + 2), {q_lpath}))
        out.append(("layer cap", bump(proof.copy(), L["off_caps"][-1] + 3), None))
    bad = proof.copy()
    bad[L["off_indices"] + q_idx] = np.uint64((int(bad[L["off_indices"] + q_idx]) + 1) % (1 << p["log_n"]))
    out.append(("index", bad, {q_idx}))
    out.append(("final coefficient", bump(proof.copy(), L["off_final"] + 1), None))
    return out


def test_model_checks_itself(oracle):
    """the model's honest proof of LDE'd random columns verifies; each tampering class is rejected (only its query, or all); columns of too
    high a degree are rejected on every query"""
    rng = np.random.default_rng(5)
    p = params(8, 5, 2, 2, 2, 1, 8)
    cols = _low_degree_cols(oracle, rng, p)
    proof, deg_ok = fm.prove(oracle, p, cols, _shift())
    cap = oracle.poseidon_merkle(cols.reshape(-1), p["log_n"], p["n_cols"], p["cap_height"])[-(1 << p["cap_height"]):]
    assert deg_ok and all(fm.verify(oracle, p, cap, proof, _shift()))
    for name, bad, fails in _tamper_cases(p, proof):
        got = fm.verify(oracle, p, cap, bad, _shift())
        want = [not (fails is None or q in fails) for q in range(p["n_queries"])]
        assert got == want, name
    bad_cap = cap.copy()
    bad_cap[0, 0] ^= np.uint64(1)
    assert not any(fm.verify(oracle, p, bad_cap, proof, _shift()))
    high = rng.integers(0, P, (p["n_cols"], 1 << p["log_n"]), dtype=np.uint64)
    hp, hdeg = fm.prove(oracle, p, high, _shift())
    hcap = oracle.poseidon_merkle(high.reshape(-1), p["log_n"], p["n_cols"], p["cap_height"])[-(1 << p["cap_height"]):]
    assert not hdeg and not any(fm.verify(oracle, p, hcap, hp, _shift()))


# ---- GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1).view(np.int64)).to(_dev())


def _down(t):
    return t.cpu().numpy().view(np.uint64)


def _sentinel(n):
    import torch
    return torch.full((n,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=_dev())


def _tree(ctx, p, d_cols):
    d_lv = _sentinel(4 * ctx.poseidon_merkle_digests(p["log_n"], p["cap_height"]))
    ctx.poseidon_merkle_device(p["log_n"], p["n_cols"], d_cols.data_ptr(), p["cap_height"], d_lv.data_ptr(), 0)
    return d_lv, d_lv[-(4 << p["cap_height"]):]


def _prove(ctx, p, d_cols, d_lv, stream=0):
    d_proof = _sentinel(fm.layout(p)["words"])
    ctx.fri_prove_device(p, d_cols.data_ptr(), d_lv.data_ptr(), d_proof.data_ptr(), stream)
    return d_proof


def _verify(ctx, p, d_cap, d_proof, stream=0):
    import torch
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    ctx.fri_verify_device(p, d_cap.data_ptr(), d_proof.data_ptr(), ok.data_ptr(), stream)
    torch.cuda.synchronize(_dev())
    return ok.cpu().numpy()


@pytest.fixture(scope="module")
def ctx(built_lib):
    import tendermintx_amd as tmx
    c = tmx.Context(4, b"celestia")
    yield c
    c.close()


CALLER_GRID = LAYOUT_GRID[:5] + [params(9, 1, 2, 3, 3, 2, 16), params(10, 3, 4, 2, 2, 3, 9), params(7, 4, 1, 1, 4, 2, 12),
                                 params(11, 9, 3, 3, 4, 4, 30)]


@pytest.mark.gpu
@pytest.mark.parametrize("p", CALLER_GRID)
def test_caller_columns_equal_the_model(ctx, oracle, p):
    """(3) tmx_lde_goldilocks_device output (with non-canonical words w + p in column 0, a constant polynomial) and its tree: the device
    proof equals the model's word for word, every query verifies on the device and in the model"""
    import torch
    rng = np.random.default_rng(p["log_n"] * 100 + p["n_cols"])
    n = 1 << (p["log_n"] - p["log_blowup"])
    base = rng.integers(0, P, (p["n_cols"], n), dtype=np.uint64)
    base[0] = 12345
    d_ext = _sentinel(p["n_cols"] << p["log_n"])
    ctx.lde_device(p["log_n"] - p["log_blowup"], p["log_blowup"], p["n_cols"], _up(base).data_ptr(), d_ext.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    ext = _down(d_ext).reshape(p["n_cols"], -1).copy()
    assert np.array_equal(ext, oracle.lde(base, p["log_blowup"]))
    ext[0, ::3] += np.uint64(P)  # the same residues, stored non-canonically
    d_cols = _up(ext)
    d_lv, d_cap = _tree(ctx, p, d_cols)
    d_proof = _prove(ctx, p, d_cols, d_lv)
    assert ctx.fri_last_degree_ok()
    want, deg = fm.prove(oracle, p, ext, _shift())
    got = _down(d_proof)
    assert deg and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert (_verify(ctx, p, d_cap, d_proof) == 1).all()
    assert all(fm.verify(oracle, p, _down(d_cap), got, _shift()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,P_,sections", [(0, 4, 3, (1, 2, 4, 16, 32)), (1, 4, 2, (2, 32)), (0, 32, 2, (2, 4, 16))])
def test_last_commit_equals_the_model(built_lib, oracle, kind, n, P_, sections):
    """(4) trace rows -> tmx_trace_commit_device -> tmx_trace_commit_fri_device: the model's proof over the oracle chain's extension, it
    verifies, and the commit's openings after the FRI equal those before it"""
    import torch
    import tendermintx_amd as tmx
    log_blowup, cap_h = 3, 2
    with tmx.Context(n, b"celestia", max_batch=P_) as ctx:
        tr = _trace_rows(ctx, kind, n, P_, 500 + n + kind)
        traces = _down(tr)
        for sec in sections:
            cap = _sentinel(4 << cap_h)
            ctx.trace_commit_device(kind, P_, sec, log_blowup, cap_h, tr.data_ptr(), cap.data_ptr(), 0)
            log_m, n_cols, _ = ctx.trace_commit_last_shape()
            p = params(log_m, n_cols, cap_h, log_blowup, 2 + sec % 3, 2, 12)
            idx = [0, 5, (1 << log_m) - 1, 77 % (1 << log_m)]
            before = _sentinel(len(idx) * n_cols), _sentinel(len(idx) * (log_m - cap_h) * 4)
            ctx.trace_commit_open_device(idx, before[0].data_ptr(), before[1].data_ptr(), 0)
            d_proof = _sentinel(fm.layout(p)["words"])
            ctx.trace_commit_fri_device(p, d_proof.data_ptr(), 0)
            after = _sentinel(len(idx) * n_cols), _sentinel(len(idx) * (log_m - cap_h) * 4)
            ctx.trace_commit_open_device(idx, after[0].data_ptr(), after[1].data_ptr(), 0)
            ok = _verify(ctx, p, cap, d_proof)
            torch.cuda.synchronize(_dev())
            assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]), sec
            assert (ok == 1).all(), (sec, ok)
            assert ctx.fri_last_degree_ok()
            ext, lm, nc = _oracle_ext(oracle, kind, n, traces, sec, log_blowup)
            assert (lm, nc) == (log_m, n_cols)
            want, deg = fm.prove(oracle, p, ext.reshape(nc, -1), _shift())
            assert deg and np.array_equal(_down(d_proof), want), sec


@pytest.mark.gpu
@pytest.mark.parametrize("p", [params(9, 6, 2, 2, 2, 1, 8), params(8, 3, 1, 1, 1, 2, 8), params(10, 20, 3, 3, 4, 2, 8)])
def test_tampering_query_by_query(ctx, oracle, p):
    """(5) one word of one query's initial row / initial path / layer row / layer path / index: only that query fails; a layer cap, a
    final coefficient or the commit cap altered: every query fails.  The model verifier agrees in every case."""
    rng = np.random.default_rng(9 + p["log_n"])
    d_cols = _up(_low_degree_cols(oracle, rng, p))
    d_lv, d_cap = _tree(ctx, p, d_cols)
    proof = _down(_prove(ctx, p, d_cols, d_lv))
    cap = _down(d_cap)
    assert (_verify(ctx, p, d_cap, _up(proof)) == 1).all()
    for name, bad, fails in _tamper_cases(p, proof):
        want = np.array([0 if (fails is None or q in fails) else 1 for q in range(p["n_queries"])])
        assert np.array_equal(_verify(ctx, p, d_cap, _up(bad)), want), name
        assert fm.verify(oracle, p, cap, bad, _shift()) == [bool(x) for x in want], name
    bad_cap = cap.copy()
    bad_cap[5] = np.uint64((int(bad_cap[5]) + 1) % P)
    assert (_verify(ctx, p, _up(bad_cap), _up(proof)) == 0).all()
    assert not any(fm.verify(oracle, p, bad_cap, proof, _shift()))


@pytest.mark.gpu
@pytest.mark.parametrize("p", [params(9, 3, 2, 3, 2, 2, 10), params(8, 2, 1, 1, 3, 0, 10)])
def test_degree_edge(ctx, oracle, p):
    """(6) degree 2^(log_n - log_blowup) - 1: degree_ok and every query accepted; degree 2^(log_n - log_blowup): neither"""
    rng = np.random.default_rng(61)
    M, D = 1 << p["log_n"], 1 << (p["log_n"] - p["log_blowup"])
    shift = _shift()
    for deg, good in ((D - 1, True), (D, False)):
        coef = np.zeros((p["n_cols"], M), dtype=np.uint64)
        coef[:, :deg + 1] = rng.integers(1, P, (p["n_cols"], deg + 1), dtype=np.uint64)
        scaled = np.array([[int(c) * pow(shift, k, P) % P for k, c in enumerate(row)] for row in coef], dtype=np.uint64)
        cols = oracle.ntt(scaled)
        d_cols = _up(cols)
        d_lv, d_cap = _tree(ctx, p, d_cols)
        d_proof = _prove(ctx, p, d_cols, d_lv)
        assert ctx.fri_last_degree_ok() == good, deg
        ok = _verify(ctx, p, d_cap, d_proof)
        assert (ok == (1 if good else 0)).all(), (deg, ok)
        want, wdeg = fm.prove(oracle, p, cols, shift)
        assert wdeg == good and np.array_equal(_down(d_proof), want)


@pytest.mark.gpu
def test_injected_constants_and_domain(built_lib, oracle):
    """(7) injected Poseidon constants and the g = 7 domain: the proof equals the model under the same tables and domain; after the
    constants change, the old proof fails verification on every query"""
    import poseidon_model as pm
    import tendermintx_amd as tmx
    rng = np.random.default_rng(71)
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
            d_proof = _prove(ctx, p, d_cols, d_lv)
            want, deg = fm.prove(oracle, p, cols, shift)
            assert deg and ctx.fri_last_degree_ok()
            assert np.array_equal(_down(d_proof), want)
            assert (_verify(ctx, p, d_cap, d_proof) == 1).all()
        finally:
            oracle.poseidon_set_constants(pm.grain_constants(), pm.MDS_CIRC, pm.MDS_DIAG)
            oracle.ntt_set_domain(*oracle.PLONKY2_DOMAIN)
        ctx.poseidon_set_constants(pm.grain_constants(), pm.MDS_CIRC, pm.MDS_DIAG)
        assert (_verify(ctx, p, d_cap, d_proof) == 0).all()


@pytest.mark.gpu
def test_lifecycle_and_arguments(built_lib, oracle):
    """(8) FRI over the last commit is refused on a fresh context, after a failed commit and on a shape mismatch; refused calls (these and
    every validation rule) leave a sentinel-filled proof untouched"""
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
        assert "no commit" in refused(lambda: ctx.trace_commit_fri_device(p0, proof.data_ptr(), 0), proof)
        refused(lambda: ctx.fri_last_degree_ok())
        tr = _trace_rows(ctx, kind, n, P_, 900)
        cap = _sentinel(4 << cap_h)
        ctx.trace_commit_device(kind, P_, 2, log_blowup, cap_h, tr.data_ptr(), cap.data_ptr(), 0)
        log_m, n_cols, _ = ctx.trace_commit_last_shape()
        p = params(log_m, n_cols, cap_h, log_blowup, 2, 2, 8)
        for field, delta in (("log_n", -1), ("n_cols", 1), ("cap_height", 1), ("log_blowup", 1)):
            refused(lambda: ctx.trace_commit_fri_device(dict(p, **{field: p[field] + delta}), proof.data_ptr(), 0), proof)
        for field, value in (("log_blowup", 0), ("arity_bits", 5), ("n_queries", 257), ("final_log_max", 9), ("cap_height", log_m + 1), ("n_cols", 0)):
            refused(lambda: ctx.trace_commit_fri_device(dict(p, **{field: value}), proof.data_ptr(), 0), proof)
            refused(lambda: ctx.fri_prove_device(dict(p, **{field: value}), proof.data_ptr(), proof.data_ptr(), proof.data_ptr(), 0), proof)
        ok = torch.full((8,), 7, dtype=torch.int32, device=_dev())
        refused(lambda: ctx.fri_verify_device(dict(p, reserved=1), cap.data_ptr(), proof.data_ptr(), ok.data_ptr(), 0), ok)
        ctx.trace_commit_fri_device(p, proof.data_ptr(), 0)
        assert (_verify(ctx, p, cap, proof) == 1).all() and ctx.fri_last_degree_ok()
        cap2 = _sentinel(4 << cap_h)
        with pytest.raises(TmxError):
            ctx.trace_commit_device(kind, P_, 8, log_blowup, cap_h, tr.data_ptr(), cap2.data_ptr(), 0)  # not a row table
        fresh = _sentinel(1 << 16)
        refused(lambda: ctx.trace_commit_fri_device(p, fresh.data_ptr(), 0), fresh)


@pytest.mark.gpu
def test_stream_ordering_and_determinism(ctx, oracle):
    """(9) prove then verify on a non-default stream with no host sync between them; two proves of the same input are identical"""
    import torch
    p = params(12, 64, 4, 3, 4, 5, 28)
    rng = np.random.default_rng(91)
    cols = _low_degree_cols(oracle, rng, p)
    d_cols = _up(cols)
    d_lv, d_cap = _tree(ctx, p, d_cols)
    torch.cuda.synchronize(_dev())
    s = torch.cuda.Stream(_dev())
    words = fm.layout(p)["words"]
    a, b = _sentinel(words), _sentinel(words)
    ok = torch.full((p["n_queries"],), 7, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize(_dev())
    with torch.cuda.stream(s):
        ctx.fri_prove_device(p, d_cols.data_ptr(), d_lv.data_ptr(), a.data_ptr(), s.cuda_stream)
        ctx.fri_verify_device(p, d_cap.data_ptr(), a.data_ptr(), ok.data_ptr(), s.cuda_stream)
        ctx.fri_prove_device(p, d_cols.data_ptr(), d_lv.data_ptr(), b.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert (ok.cpu().numpy() == 1).all()
    assert torch.equal(a, b)
    ms = ctx.fri_last_ms()
    assert set(ms) == {"combine", "layers", "final", "openings"} and all(v >= 0 for v in ms.values())
    want, _ = fm.prove(oracle, p, cols, _shift())
    assert np.array_equal(_down(a), want)
