"""Openings of the Poseidon Merkle commitment (include/tmx.h "openings of a Poseidon Merkle tree"): rows + paths out of caller trees
(tmx_poseidon_merkle_open_device) and out of the context's last commit (tmx_trace_commit_open_device), and their check on the device
(tmx_poseidon_merkle_verify_device).  Expected values come from the CPU oracle under oracle/c -- rows are slices of the columns (or of
tmxo_lde's extension), paths are slices of tmxo_poseidon_merkle's levels -- and every opening also goes through the host-side reference
verifier below (tmxo_poseidon_hash_no_pad / tmxo_poseidon_two_to_one), which is itself checked on the CPU to accept oracle openings and
reject tampered ones.  Parity unpinned against plonky2, as for the commit: natural row order, no salt, injectable constants."""
import ctypes as C

import numpy as np
import pytest

P = 2**64 - 2**32 + 1
BAD_ARG = -1
# (3, 16389, 1): above the 64 blocks x 256 threads that launch_merkle_open gives a query's columns (poseidon.hip), so k_merkle_open's
# grid-stride loop runs a second time for columns 16384 .. 16388
MERKLE_SHAPES = [(3, 3, 0), (4, 4, 2), (6, 5, 1), (8, 8, 4), (10, 9, 0), (9, 20, 3), (12, 135, 4), (5, 300, 5), (3, 16389, 1)]


# ---- the host-side reference verifier (the yardstick of every device result below)
def _olib(oracle):
    L = oracle.lib()
    L.tmxo_poseidon_hash_no_pad.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.tmxo_poseidon_hash_no_pad.restype = None
    L.tmxo_poseidon_two_to_one.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.tmxo_poseidon_two_to_one.restype = None
    return L


def ref_leaf(L, row):
    row = np.ascontiguousarray(row, dtype=np.uint64)
    if row.size <= 4:
        return np.array([int(x) % P for x in row] + [0] * (4 - row.size), dtype=np.uint64)
    out = np.zeros(4, dtype=np.uint64)
    L.tmxo_poseidon_hash_no_pad(row.ctypes.data, row.size, out.ctypes.data)
    return out


def ref_verify(L, cap, index, row, path):
    """cap: [2^cap_height][4], path: [path_len][4] (bottom-up) -> True iff the opening of leaf `index` leads to its cap digest"""
    cur = ref_leaf(L, row)
    path = np.ascontiguousarray(path, dtype=np.uint64).reshape(-1, 4)
    for lvl in range(path.shape[0]):
        sib = np.ascontiguousarray(path[lvl])
        left, right = (sib, cur) if (index >> lvl) & 1 else (cur, sib)
        nxt = np.zeros(4, dtype=np.uint64)
        L.tmxo_poseidon_two_to_one(left.ctypes.data, right.ctypes.data, nxt.ctypes.data)
        cur = nxt
    return bool(np.array_equal(cur, np.asarray(cap, dtype=np.uint64).reshape(-1, 4)[index >> path.shape[0]]))


def level_offset(log_n, lvl):
    return sum(1 << (log_n - k) for k in range(lvl))


def oracle_opening(levels, cols, log_n, n_cols, cap_height, index):
    """(row, path) of leaf `index` sliced out of column-major cols and tmxo_poseidon_merkle's levels"""
    row = np.asarray(cols, dtype=np.uint64).reshape(n_cols, 1 << log_n)[:, index].copy()
    path = np.array([levels[level_offset(log_n, lvl) + ((index >> lvl) ^ 1)] for lvl in range(log_n - cap_height)], dtype=np.uint64).reshape(-1, 4)
    return row, path


def query_indices(rng, log_n, k=13):
    n = 1 << log_n
    idx = [0, n - 1] + [int(x) for x in rng.integers(0, n, k)]
    return idx + [idx[2], 0, n - 1]  # duplicates


def _cols(rng, log_n, n_cols):
    cols = rng.integers(0, 2**64, n_cols << log_n, dtype=np.uint64)
    cols[:4] = [P - 1, P, 2**64 - 1, P + 5]  # non-canonical words (and their canonical neighbours) in the first rows of column 0
    return cols


# ---- CPU
def test_path_len(built_lib):
    L = built_lib
    for log_n, cap in ((10, 4), (14, 4), (5, 0), (6, 6), (0, 0), (30, 0), (30, 30)):
        assert L.tmx_poseidon_merkle_path_len(log_n, cap) == log_n - cap
    assert L.tmx_poseidon_merkle_path_len(3, 4) == 0   # cap above the tree: no shape
    assert L.tmx_poseidon_merkle_path_len(31, 0) == 0  # beyond the trees tmx_poseidon_merkle_device builds


@pytest.mark.parametrize("log_n,n_cols,cap", [(3, 3, 0), (4, 4, 2), (6, 5, 1), (5, 9, 5), (7, 20, 3)])
def test_reference_verifier_accepts_oracle_openings_and_rejects_tampered(oracle, log_n, n_cols, cap):
    L = _olib(oracle)
    rng = np.random.default_rng(77 + 100 * log_n + n_cols)
    cols = _cols(rng, log_n, n_cols)
    levels = oracle.poseidon_merkle(cols, log_n, n_cols, cap)
    cap_d = levels[-(1 << cap):]
    for i in query_indices(rng, log_n, 6):
        row, path = oracle_opening(levels, cols, log_n, n_cols, cap, i)
        assert np.array_equal(ref_leaf(L, row), levels[i])
        assert ref_verify(L, cap_d, i, row, path), i
        bad = row.copy()
        bad[n_cols - 1] = (int(bad[n_cols - 1]) % P + 1) % P
        assert not ref_verify(L, cap_d, i, bad, path)
        if int(row[0]) % P < 2**32 - 1:  # the same residue is the same leaf
            same = row.copy()
            same[0] = int(row[0]) % P + P
            assert ref_verify(L, cap_d, i, same, path)
        if path.size:
            bp = path.copy()
            bp[-1, 1] = (int(bp[-1, 1]) + 1) % P
            assert not ref_verify(L, cap_d, i, row, bp)
            assert not ref_verify(L, cap_d, i ^ 1, row, path) or np.array_equal(row, oracle_opening(levels, cols, log_n, n_cols, cap, i ^ 1)[0])
        bc = cap_d.copy()
        bc[i >> (log_n - cap), 3] ^= np.uint64(1)
        assert not ref_verify(L, bc, i, row, path)


# ---- GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(_dev())


def _down(t):
    return t.cpu().numpy().view(np.uint64)


def _sentinel(*shape):
    import torch
    return torch.full(shape, -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=_dev())


def _verify(ctx, log_n, n_cols, cap, d_cap, idx, d_rows, d_paths):
    import torch
    ok = torch.full((len(idx),), 7, dtype=torch.int32, device=_dev())
    ctx.poseidon_merkle_verify_device(log_n, n_cols, cap, d_cap.data_ptr(), idx, d_rows.data_ptr(), d_paths.data_ptr() if d_paths is not None else None,
                                      ok.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    return ok.cpu().numpy()


@pytest.fixture(scope="module")
def ctx(built_lib):
    import tendermintx_amd as tmx
    c = tmx.Context(4, b"celestia")
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,n_cols,cap", MERKLE_SHAPES)
def test_standalone_openings_are_oracle_slices_and_verify(ctx, oracle, log_n, n_cols, cap):
    """(1) rows bit for bit, paths = the oracle's level entries; (2) every opening passes the reference verifier and the device verifier"""
    import torch
    L = _olib(oracle)
    rng = np.random.default_rng(1000 * log_n + n_cols)
    cols = _cols(rng, log_n, n_cols)
    d_cols = _up(cols)
    nd = ctx.poseidon_merkle_digests(log_n, cap)
    d_lv = _sentinel(nd, 4)
    ctx.poseidon_merkle_device(log_n, n_cols, d_cols.data_ptr(), cap, d_lv.data_ptr(), 0)
    idx = query_indices(rng, log_n)
    pl = ctx.poseidon_merkle_path_len(log_n, cap)
    assert pl == log_n - cap
    d_rows, d_paths = _sentinel(len(idx), n_cols), _sentinel(len(idx), max(pl, 1), 4)
    ctx.poseidon_merkle_open_device(log_n, n_cols, d_cols.data_ptr(), cap, d_lv.data_ptr(), np.array(idx, dtype=np.uint64), d_rows.data_ptr(),
                                    d_paths.data_ptr(), 0)
    torch.cuda.synchronize(_dev())
    rows, paths = _down(d_rows), _down(d_paths)
    levels = oracle.poseidon_merkle(cols, log_n, n_cols, cap)
    cap_d = levels[-(1 << cap):]
    for q, i in enumerate(idx):
        row, path = oracle_opening(levels, cols, log_n, n_cols, cap, i)
        assert np.array_equal(rows[q], row), (q, i)
        if pl:
            assert np.array_equal(paths[q], path), (q, i)
        else:
            assert (paths[q] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()  # nothing written where there is no path
        assert ref_verify(L, cap_d, i, rows[q], paths[q][:pl]), (q, i)
    d_cap = d_lv[nd - (1 << cap):]
    assert np.array_equal(_down(d_cap), cap_d)
    assert (_verify(ctx, log_n, n_cols, cap, d_cap, idx, d_rows, d_paths) == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,n_cols,cap", [(9, 20, 3), (4, 4, 2), (6, 5, 1), (8, 300, 2), (4, 16389, 1)])
def test_verifier_rejects_query_by_query(ctx, oracle, log_n, n_cols, cap):
    """(3) in one mixed batch, only the tampered queries report 0: a row element to another residue, one word of one sibling, the indices
    of two queries with different rows swapped, one word of the cap (every query under that cap digest)"""
    L = _olib(oracle)
    rng = np.random.default_rng(31 * log_n + n_cols)
    cols = _cols(rng, log_n, n_cols)
    d_cols = _up(cols)
    nd, pl = ctx.poseidon_merkle_digests(log_n, cap), log_n - cap
    d_lv = _sentinel(nd, 4)
    ctx.poseidon_merkle_device(log_n, n_cols, d_cols.data_ptr(), cap, d_lv.data_ptr(), 0)
    idx = [int(x) for x in rng.choice(1 << log_n, 16, replace=False)]
    d_rows, d_paths = _sentinel(16, n_cols), _sentinel(16, pl, 4)
    ctx.poseidon_merkle_open_device(log_n, n_cols, d_cols.data_ptr(), cap, d_lv.data_ptr(), idx, d_rows.data_ptr(), d_paths.data_ptr(), 0)
    d_cap = d_lv[nd - (1 << cap):].clone()
    rows, paths, cap_h = _down(d_rows), _down(d_paths), _down(d_cap).reshape(-1, 4)
    assert (_verify(ctx, log_n, n_cols, cap, d_cap, idx, d_rows, d_paths) == 1).all()

    def run(rows_t, paths_t, idx_t, cap_t, tampered):
        want = np.array([0 if q in tampered else 1 for q in range(16)], dtype=np.int32)
        ref = np.array([ref_verify(L, cap_t, idx_t[q], rows_t[q], paths_t[q]) for q in range(16)], dtype=np.int32)
        assert np.array_equal(ref, want), ("reference verifier", ref, want)
        got = _verify(ctx, log_n, n_cols, cap, _up(cap_t), idx_t, _up(rows_t), _up(paths_t))
        assert np.array_equal(got, want), (got, want)

    r = rows.copy()
    r[3, n_cols // 2] = (int(r[3, n_cols // 2]) % P + 12345) % P
    run(r, paths, idx, cap_h, {3})
    last = rows.copy()  # the last column: above 16384 columns, one that k_merkle_open copies in a later pass of its loop
    last[9, n_cols - 1] = (int(last[9, n_cols - 1]) % P + 1) % P
    run(last, paths, idx, cap_h, {9})
    p_ = paths.copy()
    p_[7, pl // 2, 2] = (int(p_[7, pl // 2, 2]) + 1) % P
    run(rows, p_, idx, cap_h, {7})
    assert not np.array_equal(rows[10], rows[11])
    sw = list(idx)
    sw[10], sw[11] = sw[11], sw[10]
    run(rows, paths, sw, cap_h, {10, 11})
    c_ = cap_h.copy()
    slot = idx[5] >> pl
    c_[slot, 1] = (int(c_[slot, 1]) + 1) % P
    run(rows, paths, idx, c_, {q for q in range(16) if idx[q] >> pl == slot})
    # all four at once
    run(r, p_, sw, c_, {3, 7, 10, 11} | {q for q in range(16) if idx[q] >> pl == slot})


def _section_geom(kind, n, section):
    """(offset, rows, width) of one row table inside a proof's trace block (include/tmx.h tmx_trace_rows_device)"""
    sets = 2 if kind == 0 else 1
    tn, sz = 0, n
    while sz > 1:
        sz = (sz + 1) // 2
        tn += sz
    o512 = n * 2 * 256 * 65
    o256 = o512 + n * 2 * 80 * 18
    otree = o256 + sets * n * 64 * 9 + (n * n if kind == 0 else 0)
    return {1: (0, 2 * n * 256, 65), 2: (o512, 2 * n * 80, 18), 4: (o256, sets * n * 64, 9), 16: (otree, sets * tn * 128, 9),
            32: (otree + sets * tn * 1152, (4 if kind == 0 else 5) * 5 * 128, 9)}[section]


def _oracle_ext(oracle, kind, n, traces, section, log_blowup):
    """the extended columns of the CPU chain (tests/test_commit_pipeline.py): trace blocks -> section columns -> tmxo_lde"""
    off, rows, width = _section_geom(kind, n, section)
    log_n = max(6, (rows - 1).bit_length())
    cols = np.zeros((len(traces) * width, 1 << log_n), dtype=np.uint64)
    for p, full in enumerate(traces):
        cols[p * width:(p + 1) * width, :rows] = full[off:off + rows * width].reshape(rows, width).T
    return np.ascontiguousarray(oracle.lde(cols, log_blowup)).reshape(-1), log_n + log_blowup, len(traces) * width


def _trace_rows(ctx, kind, n, P, seed):
    import torch
    from tendermintx_amd.synth import Workload
    wl = Workload(kind, n, P, n - 1 if n > 4 else n, chain_id=b"celestia", seed=seed, signed_permille=900)
    dev = _dev()
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None for b in (wl.proofs, wl.targets, wl.trusteds if kind == 0 else b"")]
    out = torch.zeros((P, ctx.elem_stride(kind)), dtype=torch.int64, device=dev)
    rep = torch.zeros(P * 64, dtype=torch.uint8, device=dev)
    tr = torch.zeros((P, ctx.trace_elem_count(kind)), dtype=torch.int64, device=dev)
    ctx.witness_batch_device(kind, P, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr() if d[2] is not None else None, out.data_ptr(), rep.data_ptr(), 0)
    ctx.trace_rows_device(kind, P, d[1].data_ptr(), d[2].data_ptr() if d[2] is not None else None, tr.data_ptr(), 63, 0)
    torch.cuda.synchronize(dev)
    return tr


def _commit_open_verify(ctx, kind, sec, P, log_blowup, cap_h, tr, idx_fn):
    """commit -> last shape -> open -> device verify against the returned cap; returns the host copies"""
    import torch
    cap = _sentinel(1 << cap_h, 4)
    ctx.trace_commit_device(kind, P, sec, log_blowup, cap_h, tr.data_ptr(), cap.data_ptr(), 0)
    log_m, n_cols, ch = ctx.trace_commit_last_shape()
    idx = idx_fn(log_m)
    pl = log_m - ch
    d_rows, d_paths = _sentinel(len(idx), n_cols), _sentinel(len(idx), pl, 4)
    ctx.trace_commit_open_device(idx, d_rows.data_ptr(), d_paths.data_ptr(), 0)
    ok = _verify(ctx, log_m, n_cols, ch, cap, idx, d_rows, d_paths)
    torch.cuda.synchronize(_dev())
    return dict(shape=(log_m, n_cols, ch), idx=idx, rows=_down(d_rows), paths=_down(d_paths), cap=_down(cap), ok=ok)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,P,sections", [(0, 4, 3, (1, 2, 4, 16, 32)), (1, 4, 2, (2, 32)), (0, 32, 2, (2, 4, 16))])
def test_commit_openings_equal_the_oracle_chain(built_lib, oracle, kind, n, P, sections):
    """(4) trace rows -> tmx_trace_commit_device -> tmx_trace_commit_open_device: rows = the rows of tmxo_lde's extension, paths = the levels
    of tmxo_poseidon_merkle over it, every opening verifies against the commit's cap; the last shape is (log_n + log_blowup, P * width, cap)"""
    import tendermintx_amd as tmx
    L = _olib(oracle)
    log_blowup, cap_h = 3, 2
    rng = np.random.default_rng(7 + n + kind)
    got = {}
    with tmx.Context(n, b"celestia", max_batch=P) as ctx:
        tr = _trace_rows(ctx, kind, n, P, 500 + n + kind)
        for sec in sections:
            got[sec] = _commit_open_verify(ctx, kind, sec, P, log_blowup, cap_h, tr, lambda lm: query_indices(rng, lm, 29))
        traces = _down(tr)
    for sec in sections:
        g = got[sec]
        off, rows, width = _section_geom(kind, n, sec)
        ext, log_m, n_cols = _oracle_ext(oracle, kind, n, traces, sec, log_blowup)
        assert g["shape"] == (max(6, (rows - 1).bit_length()) + log_blowup, P * width, cap_h)
        assert (log_m, n_cols) == g["shape"][:2]
        levels = oracle.poseidon_merkle(ext, log_m, n_cols, cap_h)
        assert np.array_equal(g["cap"], levels[-(1 << cap_h):])
        assert (g["ok"] == 1).all(), (sec, g["ok"])
        for q, i in enumerate(g["idx"]):
            row, path = oracle_opening(levels, ext, log_m, n_cols, cap_h, i)
            assert np.array_equal(g["rows"][q], row), (sec, q, i)
            assert np.array_equal(g["paths"][q], path), (sec, q, i)
            if q < 4:
                assert ref_verify(L, g["cap"], i, g["rows"][q], g["paths"][q])


@pytest.mark.gpu
def test_open_lifecycle_and_argument_errors(built_lib, oracle):
    """(5) no commit yet / an index >= 2^log_m / n_queries == 0 / a failed commit: TMX_ERR_BAD_ARG and the outputs untouched; after two
    commits of different sections the open serves the second"""
    import torch
    import tendermintx_amd as tmx
    from tendermintx_amd._lib import TmxError
    kind, n, P, log_blowup, cap_h = 1, 4, 2, 2, 1

    def refused(fn, *outs):
        before = [o.clone() for o in outs]
        with pytest.raises(TmxError) as e:
            fn()
        torch.cuda.synchronize(_dev())
        assert e.value.status == BAD_ARG, e.value
        for a, b in zip(outs, before):
            assert torch.equal(a, b)
        return str(e.value)

    with tmx.Context(n, b"celestia", max_batch=P) as ctx:
        rows, paths = _sentinel(4, 64), _sentinel(4, 16, 4)
        msg = refused(lambda: ctx.trace_commit_open_device([0], rows.data_ptr(), paths.data_ptr(), 0), rows, paths)
        assert "no commit" in msg
        refused(lambda: ctx.trace_commit_last_shape())
        tr = _trace_rows(ctx, kind, n, P, 900)
        first = _commit_open_verify(ctx, kind, 2, P, log_blowup, cap_h, tr, lambda lm: [0, 5, (1 << lm) - 1])
        second = _commit_open_verify(ctx, kind, 32, P, log_blowup, cap_h, tr, lambda lm: [0, 5, (1 << lm) - 1])
        log_m, n_cols, _ = second["shape"]
        assert first["shape"] != second["shape"] and (first["ok"] == 1).all() and (second["ok"] == 1).all()
        d_rows, d_paths = _sentinel(3, n_cols), _sentinel(3, log_m - cap_h, 4)
        refused(lambda: ctx.trace_commit_open_device([0, 1 << log_m, 2], d_rows.data_ptr(), d_paths.data_ptr(), 0), d_rows, d_paths)
        refused(lambda: ctx.trace_commit_open_device([], d_rows.data_ptr(), d_paths.data_ptr(), 0), d_rows, d_paths)
        # the standalone calls validate the same way
        d_cols = _up(np.arange(n_cols << 4, dtype=np.uint64))
        d_lv = _sentinel(ctx.poseidon_merkle_digests(4, 1), 4)
        ctx.poseidon_merkle_device(4, n_cols, d_cols.data_ptr(), 1, d_lv.data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        refused(lambda: ctx.poseidon_merkle_open_device(4, n_cols, d_cols.data_ptr(), 1, d_lv.data_ptr(), [3, 16], d_rows.data_ptr(), d_paths.data_ptr(), 0),
                d_rows, d_paths)
        refused(lambda: ctx.poseidon_merkle_open_device(4, n_cols, d_cols.data_ptr(), 1, d_lv.data_ptr(), [], d_rows.data_ptr(), d_paths.data_ptr(), 0),
                d_rows, d_paths)
        ok = torch.full((2,), 7, dtype=torch.int32, device=_dev())
        cap = d_lv[-2:]
        refused(lambda: ctx.poseidon_merkle_verify_device(4, n_cols, 1, cap.data_ptr(), [1, 1 << 4], d_rows.data_ptr(), d_paths.data_ptr(), ok.data_ptr(), 0), ok)
        refused(lambda: ctx.poseidon_merkle_verify_device(4, n_cols, 1, cap.data_ptr(), [], d_rows.data_ptr(), d_paths.data_ptr(), ok.data_ptr(), 0), ok)
        # the open after the two commits serves the second: its rows are the oracle extension of section 32
        ext, lm, nc = _oracle_ext(oracle, kind, n, _down(tr), 32, log_blowup)
        assert (lm, nc) == (log_m, n_cols) and ctx.trace_commit_last_shape() == second["shape"]
        ctx.trace_commit_open_device([7, 0], d_rows.data_ptr(), d_paths.data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        got = _down(d_rows)
        assert np.array_equal(got[0], ext.reshape(nc, 1 << lm)[:, 7]) and np.array_equal(got[1], ext.reshape(nc, 1 << lm)[:, 0])
        # a commit that fails leaves nothing to open
        cap2 = _sentinel(2, 4)
        with pytest.raises(TmxError):
            ctx.trace_commit_device(kind, P, 8, log_blowup, cap_h, tr.data_ptr(), cap2.data_ptr(), 0)  # the N x N bits are not a row table
        refused(lambda: ctx.trace_commit_open_device([0], d_rows.data_ptr(), d_paths.data_ptr(), 0), d_rows, d_paths)
        refused(lambda: ctx.trace_commit_last_shape())


@pytest.mark.gpu
def test_injected_constants_open_and_verify_under_their_own_tables(built_lib, oracle):
    """(6) commit, open and verify under tmx_poseidon_set_constants tables (the merged-round, the 32-bit-limb and the general MDS forms): all
    queries pass and the cap is the oracle's under the same tables; a context with the default constants rejects every one of them"""
    import torch
    import poseidon_model as pm
    import tendermintx_amd as tmx
    kind, n, n_proofs, log_blowup, cap_h = 1, 4, 2, 1, 2
    rng = np.random.default_rng(66)
    big = lambda k: [int(x) % P for x in rng.integers(0, 2**63, k, dtype=np.uint64)]
    rc = big(360)
    tables = [(rc, pm.MDS_CIRC, pm.MDS_DIAG), (rc, [65535] * 12, [65535] * 12), (rc, big(12), big(12))]
    with tmx.Context(n, b"celestia", max_batch=n_proofs) as plain:
        for t, (r, circ, diag) in enumerate(tables):
            with tmx.Context(n, b"celestia", max_batch=n_proofs) as ctx:
                ctx.poseidon_set_constants(r, circ, diag)
                # (the commit hashes any rows: random words below 2^32 stand in for a trace)
                tr = _up(rng.integers(0, 2**32, (n_proofs, ctx.trace_elem_count(kind)), dtype=np.uint64))
                g = _commit_open_verify(ctx, kind, 32, n_proofs, log_blowup, cap_h, tr, lambda lm: query_indices(rng, lm, 9))
                assert (g["ok"] == 1).all(), (t, g["ok"])
                ext, log_m, n_cols = _oracle_ext(oracle, kind, n, _down(tr), 32, log_blowup)
                try:
                    oracle.poseidon_set_constants(r, circ, diag)
                    levels = oracle.poseidon_merkle(ext, log_m, n_cols, cap_h)
                finally:
                    oracle.poseidon_set_constants(pm.grain_constants(), pm.MDS_CIRC, pm.MDS_DIAG)
                assert np.array_equal(g["cap"], levels[-(1 << cap_h):]), t
                assert np.array_equal(g["paths"][0], oracle_opening(levels, ext, log_m, n_cols, cap_h, g["idx"][0])[1])
                ok = _verify(plain, log_m, n_cols, cap_h, _up(g["cap"]), g["idx"], _up(g["rows"]), _up(g["paths"]))
                assert (ok == 0).all(), (t, ok)
                assert (_verify(ctx, log_m, n_cols, cap_h, _up(g["cap"]), g["idx"], _up(g["rows"]), _up(g["paths"])) == 1).all()
        torch.cuda.synchronize(_dev())
