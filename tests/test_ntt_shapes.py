"""The Goldilocks NTT / coset LDE (ntt.hip, the ntt_* host path of api.cpp) at every shape and branch it has, word for word against
oracle/c/tmxo_ntt.c under BOTH domains (plonky2's constants and g = 7: the load permutations kinv = 1 / 15 and 5 / 11 of the forward /
inverse transform): every two-pass split 2^12 .. 2^22, the one-pass fixed tiles with the column counts that just fill, overflow and miss
them, extreme words through the large kernels, every host branch of the LDE in its fused and its padded form (TMX_LDE_FUSED=0), the
context's caches across domain changes, scratch growth on a side stream.  The CPU part pins the oracle at those sizes against direct sums
in Python integers.  docs/kernels.md "NTT and coset LDE: which test reaches which shape" lists what reaches what."""
import contextlib

import numpy as np
import pytest

P = 2**64 - 2**32 + 1
EDGE = [0, 1, P - 1, P, 2**64 - 1]
DOMAINS = ["plonky2", "g7"]


def _dom(oc, name):
    return oc.PLONKY2_DOMAIN if name == "plonky2" else oc.G7_DOMAIN


@contextlib.contextmanager
def _domain(oc, dom, *ctxs):
    """The oracle and the given contexts under (root, shift); the default domain again afterwards, whatever happened."""
    try:
        oc.ntt_set_domain(*dom)
        for c in ctxs:
            c.ntt_set_domain(*dom)
        yield
    finally:
        oc.ntt_set_domain(*oc.PLONKY2_DOMAIN)
        for c in ctxs:
            c.ntt_set_domain(*oc.PLONKY2_DOMAIN)


def _rand(rng, shape):
    """Random words in [0, 2^64) -- most of them canonical, 2^-32 of them not -- behind the edge words 0, 1, p - 1, p, 2^64 - 1."""
    a = rng.integers(0, 2**64, size=shape, dtype=np.uint64)
    flat = a.reshape(-1)
    k = min(len(EDGE), flat.size)
    flat[:k] = EDGE[:k]
    return a


def _root(dom, log_n):
    return pow(dom[0], 1 << (32 - log_n), P)


# ---- CPU: the oracle itself at the sizes the GPU tests lean on it (tests/test_ntt_oracle.py has the O(n^2) DFT up to 2^7 only) ------------
def _sparse(rng, n, k, canonical=False):
    pos = rng.choice(n, size=min(k, n), replace=False)
    col = np.zeros(n, dtype=np.uint64)
    col[pos] = rng.integers(0, P if canonical else 2**64, size=pos.size, dtype=np.uint64)
    if not canonical:
        col[pos[: len(EDGE)]] = EDGE[: pos.size]
    return col, [int(i) for i in pos]


@pytest.mark.parametrize("log_n", [19, 20, 21, 22])
@pytest.mark.parametrize("domain", DOMAINS)
def test_oracle_ntt_equals_the_direct_sum_at_full_size(oracle, domain, log_n):
    """64 non-zero words at random positions: 32 sampled outputs of the oracle's forward and inverse transform against
    sum x_i omega^(+-ij) (/ n) in Python integers."""
    oc, dom = oracle, _dom(oracle, domain)
    rng = np.random.default_rng(9000 + log_n)
    n = 1 << log_n
    x, pos = _sparse(rng, n, 64)
    idx = [0, 1, n // 2, n - 1] + [int(j) for j in rng.integers(0, n, size=28)]
    w = _root(dom, log_n)
    n_inv = pow(n, P - 2, P)
    with _domain(oc, dom):
        fwd, inv = oc.ntt(x), oc.ntt(x, inverse=True)
    for j in idx:
        wj, wj_inv = pow(w, j, P), pow(w, n - j, P)
        assert int(fwd[j]) == sum(int(x[i]) * pow(wj, i, P) for i in pos) % P, (log_n, j)
        assert int(inv[j]) == sum(int(x[i]) * pow(wj_inv, i, P) for i in pos) * n_inv % P, (log_n, j)


@pytest.mark.parametrize("log_n,log_blowup", [(18, 3), (11, 11), (5, 17)])
@pytest.mark.parametrize("domain", DOMAINS)
def test_oracle_lde_evaluates_a_sparse_polynomial_on_the_coset(oracle, domain, log_n, log_blowup):
    """x = the values of a sparse polynomial c on the subgroup: 32 sampled words of the oracle's LDE against sum c_i (shift omega_M^j)^i."""
    oc, dom = oracle, _dom(oracle, domain)
    rng = np.random.default_rng(9100 + log_n)
    n, m = 1 << log_n, 1 << (log_n + log_blowup)
    c, pos = _sparse(rng, n, 64 if n > 64 else n // 2, canonical=True)
    c[n - 1] = P - 1          # the top coefficient is always there
    pos = sorted(set(pos) | {n - 1})
    idx = [0, 1, m // 2, m - 1] + [int(j) for j in rng.integers(0, m, size=28)]
    wm = _root(dom, log_n + log_blowup)
    with _domain(oc, dom):
        ext = oc.lde(oc.ntt(c), log_blowup)
    for j in idx:
        pt = dom[1] * pow(wm, j, P) % P
        assert int(ext[j]) == sum(int(c[i]) * pow(pt, i, P) for i in pos) % P, (log_n, log_blowup, j)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def _to_host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream0(torch):
    return torch.cuda.current_stream().cuda_stream


def _ntt(torch, ctx, d_in, log_n, cols, inverse, d_out=None):
    out = torch.empty_like(d_in) if d_out is None else d_out
    ctx.ntt_device(log_n, cols, d_in.data_ptr(), out.data_ptr(), inverse, _stream0(torch))
    return out


def _lde(torch, ctx, x, log_n, log_blowup, cols):
    d = _to_dev(torch, x)
    out = torch.empty((cols, 1 << (log_n + log_blowup)), dtype=torch.int64, device="cuda:0")
    ctx.lde_device(log_n, log_blowup, cols, d.data_ptr(), out.data_ptr(), _stream0(torch))
    torch.cuda.synchronize()
    return _to_host(out)


@pytest.fixture(scope="module")
def env(oracle, built_lib):
    import torch
    import tendermintx_amd as tmx
    ctx = tmx.Context(4, b"celestia", max_batch=1)
    yield torch, ctx, oracle
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", range(12, 23))
@pytest.mark.parametrize("domain", DOMAINS)
def test_every_two_pass_split_is_bit_exact(env, domain, log_n):
    """k_ntt_tile<6,6> .. <11,3> as pass A (strided in and out, the matrix on the way out) and pass B (contiguous in, transposed out),
    tiles of 2^12, 2^13 and 2^14 elements: the forward transform against the oracle, the inverse of that on the device against x mod p;
    at 2^13 and 2^20 one forward transform in place."""
    torch, ctx, oc = env
    cols = 3 if log_n <= 18 else 2 if log_n <= 20 else 1
    x = _rand(np.random.default_rng(1200 + log_n), (cols, 1 << log_n))
    with _domain(oc, _dom(oc, domain), ctx):
        want = oc.ntt(x)
        d = _to_dev(torch, x)
        fwd = _ntt(torch, ctx, d, log_n, cols, False)
        back = _ntt(torch, ctx, fwd, log_n, cols, True)
        torch.cuda.synchronize()
        assert np.array_equal(_to_host(fwd), want), (log_n, "forward")
        assert np.array_equal(_to_host(back), x % np.uint64(P)), (log_n, "inverse of the forward result")
        if log_n in (13, 20):
            _ntt(torch, ctx, d, log_n, cols, False, d_out=d)
            torch.cuda.synchronize()
            assert np.array_equal(_to_host(d), want), (log_n, "in place")


ONE_PASS = [(log_n, (1 << (12 - log_n)) + d) for log_n in range(4, 12) for d in (0, 1, -1)] + [(0, 4097), (1, 2049), (3, 513), (2, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,cols", ONE_PASS)
@pytest.mark.parametrize("domain", DOMAINS)
def test_one_pass_fixed_tiles_and_their_neighbours(env, domain, log_n, cols):
    """C = 2^(12 - log_n) columns are one full fixed tile k_ntt_tile<log_n, 12 - log_n> in the contiguous mapping (TH >= L up to 2^8), C + 1
    a second tile with one live sub-transform (FULL = false), C - 1 the generic kernel with a partly filled tile; below 2^4 the generic
    kernel runs whole tiles of 2^12 elements and more than one of them."""
    torch, ctx, oc = env
    x = _rand(np.random.default_rng(200 * log_n + cols), (cols, 1 << log_n))
    with _domain(oc, _dom(oc, domain), ctx):
        d = _to_dev(torch, x)
        for inverse in (False, True):
            out = _ntt(torch, ctx, d, log_n, cols, inverse)
            torch.cuda.synchronize()
            assert np.array_equal(_to_host(out), oc.ntt(x, inverse=inverse)), (log_n, cols, inverse)


@pytest.mark.gpu
@pytest.mark.parametrize("fill", ["all_ones", "p_minus_1", "above_p", "extremes"])
@pytest.mark.parametrize("log_n", [19, 21])
def test_extreme_words_through_the_large_kernels(env, log_n, fill):
    """The fills of test_ntt_noncanonical_and_extreme_inputs through <10,3>, <9,3> (2^19) and <11,3>, <10,3> (2^21) under g = 7."""
    torch, ctx, oc = env
    n = 1 << log_n
    rng = np.random.default_rng(7000 + log_n)
    if fill == "all_ones":
        x = np.full((1, n), 2**64 - 1, dtype=np.uint64)
    elif fill == "p_minus_1":
        x = np.full((1, n), P - 1, dtype=np.uint64)
    elif fill == "above_p":
        x = rng.integers(P, 2**64, size=(1, n), dtype=np.uint64, endpoint=False)
    else:
        x = rng.choice(np.array([0, 1, P - 1, P, P + 1, 2**64 - 1, 2**32 - 1, 2**32, 2**63], dtype=np.uint64), size=(1, n))
    with _domain(oc, oc.G7_DOMAIN, ctx):
        d = _to_dev(torch, x)
        for inverse in (False, True):
            out = _ntt(torch, ctx, d, log_n, 1, inverse)
            torch.cuda.synchronize()
            assert np.array_equal(_to_host(out), oc.ntt(x, inverse=inverse)), (fill, inverse)


LDE_CASES = [(5, 3, 9), (8, 3, 16),                              # fused, one pass in both halves
             (9, 4, 3), (11, 1, 2), (11, 8, 1),                  # fused, one-pass inverse into a two-pass forward: j_nonzero = N >> b
             (12, 2, 3), (14, 3, 2), (18, 3, 1), (19, 3, 1),     # fused, two passes in both halves: the scale vector on pass B
             (6, 6, 3), (11, 11, 1),                             # fused, log_n == b_fwd: j_nonzero = 1
             (5, 7, 3), (10, 12, 1), (5, 17, 1),                 # padded, log_n < b_fwd: k_lde_expand
             (5, 0, 3), (13, 0, 2)]                              # blow-up 0: the values on the coset itself
LDE_FUSED_ONLY = {(19, 3, 1), (10, 12, 1), (5, 17, 1)}          # full-size rows the TMX_LDE_FUSED=0 pass leaves to (18, 3, 1) and (11, 11, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,log_blowup,cols", LDE_CASES)
@pytest.mark.parametrize("domain", DOMAINS)
def test_lde_every_host_branch(env, monkeypatch, domain, log_n, log_blowup, cols):
    """Random columns through every branch of tmx_lde_goldilocks_device, then the same call with TMX_LDE_FUSED=0 (read on every call): the
    padded form through k_lde_expand gives the same words.  Blow-up 0 is accepted and returns the column's values on the coset."""
    torch, ctx, oc = env
    monkeypatch.delenv("TMX_LDE_FUSED", raising=False)
    x = _rand(np.random.default_rng(5000 + 50 * log_n + log_blowup), (cols, 1 << log_n))
    with _domain(oc, _dom(oc, domain), ctx):
        want = oc.lde(x, log_blowup)
        assert np.array_equal(_lde(torch, ctx, x, log_n, log_blowup, cols), want), "fused where the split allows it"
        if (log_n, log_blowup, cols) not in LDE_FUSED_ONLY:
            monkeypatch.setenv("TMX_LDE_FUSED", "0")
            assert np.array_equal(_lde(torch, ctx, x, log_n, log_blowup, cols), want), "TMX_LDE_FUSED=0"


def _cache_inputs():
    rng = np.random.default_rng(4242)
    return [_rand(rng, (2, 1 << 13)), _rand(rng, (1, 1 << 19)), _rand(rng, (2, 1 << 12)), _rand(rng, (2, 1 << 9))]


def _cache_device(torch, ctx, xs):
    """NTT forward and inverse at 2^13 x 2 and 2^19 x 1, LDE (12, 2, 2) and (9, 4, 2): [four transforms], [two extensions]"""
    ntts = []
    for x, log_n in ((xs[0], 13), (xs[1], 19)):
        d = _to_dev(torch, x)
        outs = [_ntt(torch, ctx, d, log_n, x.shape[0], inverse) for inverse in (False, True)]
        torch.cuda.synchronize()
        ntts += [_to_host(o) for o in outs]
    return ntts, [_lde(torch, ctx, xs[2], 12, 2, 2), _lde(torch, ctx, xs[3], 9, 4, 2)]


def _cache_oracle(oc, xs):
    return ([oc.ntt(xs[0]), oc.ntt(xs[0], inverse=True), oc.ntt(xs[1]), oc.ntt(xs[1], inverse=True)],
            [oc.lde(xs[2], 2), oc.lde(xs[3], 4)])


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.gpu
def test_caches_across_domain_changes_on_one_context(oracle, built_lib):
    """d_ntt_w, both d_ntt_m and d_lde_s built under one domain must not serve the next: a new root drops all three, a new shift alone the
    scale vectors only, the values already in force nothing; a refused domain leaves the one in force usable."""
    import torch
    import tendermintx_amd as tmx
    oc = oracle
    xs = _cache_inputs()
    root7 = oc.G7_DOMAIN[0]
    with tmx.Context(4, b"celestia", max_batch=1) as ctx:
        try:
            # 1. the default domain: tables at 2^9, 2^12, 2^13, 2^14, 2^19, matrices at 2^12 (inverse), 2^13, 2^14 (forward), 2^19, scale vectors
            ntt1, lde1 = _cache_device(torch, ctx, xs)
            w_ntt, w_lde = _cache_oracle(oc, xs)
            assert _same(ntt1, w_ntt) and _same(lde1, w_lde)
            # 2. g = 7: another root and another shift
            ctx.ntt_set_domain(*oc.G7_DOMAIN)
            oc.ntt_set_domain(*oc.G7_DOMAIN)
            ntt2, lde2 = _cache_device(torch, ctx, xs)
            w_ntt, w_lde = _cache_oracle(oc, xs)
            assert _same(ntt2, w_ntt) and _same(lde2, w_lde)
            assert not np.array_equal(ntt2[0], ntt1[0])
            with pytest.raises(tmx.TmxError):
                ctx.ntt_set_domain(5, 7)          # 5 is not a primitive 2^32-th root of unity: g = 7 stays in force
            assert np.array_equal(_lde(torch, ctx, xs[2], 12, 2, 2), w_lde[0])
            # 3. the same root, another shift: the transforms keep their words, the extensions move to the new coset
            ctx.ntt_set_domain(root7, 3)
            oc.ntt_set_domain(root7, 3)
            ntt3, lde3 = _cache_device(torch, ctx, xs)
            assert _same(ntt3, ntt2)
            assert _same(lde3, [oc.lde(xs[2], 2), oc.lde(xs[3], 4)])
            assert not np.array_equal(lde3[0], lde2[0]) and not np.array_equal(lde3[1], lde2[1])
            # 4. back to the default domain: the words of step 1
            ctx.ntt_set_domain(*oc.PLONKY2_DOMAIN)
            oc.ntt_set_domain(*oc.PLONKY2_DOMAIN)
            ntt4, lde4 = _cache_device(torch, ctx, xs)
            assert _same(ntt4, ntt1) and _same(lde4, lde1)
            # 5. the values already in force: nothing is dropped, nothing goes stale
            ctx.ntt_set_domain(*oc.PLONKY2_DOMAIN)
            ntt5, lde5 = _cache_device(torch, ctx, xs)
            assert _same(ntt5, ntt1) and _same(lde5, lde1)
        finally:
            ctx.ntt_set_domain(*oc.PLONKY2_DOMAIN)
            oc.ntt_set_domain(*oc.PLONKY2_DOMAIN)


@pytest.mark.gpu
@pytest.mark.parametrize("domain", DOMAINS)
def test_scratch_growth_on_a_side_stream(oracle, built_lib, domain):
    """A fresh context on a non-default stream (the first-use table, matrix and scale-vector builds happen there): 2^12 x 1, 2^14 x 8, LDE
    (12, 3, 4) and 2^12 x 1 again with no host synchronisation between them -- d_ntt_tmp is reallocated twice under work in flight."""
    import torch
    import tendermintx_amd as tmx
    oc = oracle
    rng = np.random.default_rng(616)
    a, b, c = _rand(rng, (1, 1 << 12)), _rand(rng, (8, 1 << 14)), _rand(rng, (4, 1 << 12))
    with tmx.Context(4, b"celestia", max_batch=1) as ctx, _domain(oc, _dom(oc, domain), ctx):
        da, db, dc = _to_dev(torch, a), _to_dev(torch, b), _to_dev(torch, c)
        oa, ob, oa2 = torch.empty_like(da), torch.empty_like(db), torch.empty_like(da)
        olde = torch.empty((4, 1 << 15), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        assert side.cuda_stream != 0
        s = side.cuda_stream
        ctx.ntt_device(12, 1, da.data_ptr(), oa.data_ptr(), False, s)
        ctx.ntt_device(14, 8, db.data_ptr(), ob.data_ptr(), False, s)
        ctx.lde_device(12, 3, 4, dc.data_ptr(), olde.data_ptr(), s)
        ctx.ntt_device(12, 1, da.data_ptr(), oa2.data_ptr(), True, s)
        side.synchronize()
        assert np.array_equal(_to_host(oa), oc.ntt(a))
        assert np.array_equal(_to_host(ob), oc.ntt(b))
        assert np.array_equal(_to_host(olde), oc.lde(c, 3))
        assert np.array_equal(_to_host(oa2), oc.ntt(a, inverse=True))


@pytest.mark.gpu
def test_zero_columns_leave_the_output_alone(env):
    torch, ctx, oc = env
    d = _to_dev(torch, _rand(np.random.default_rng(3), (1, 32)))
    out = torch.full((64,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
    ctx.ntt_device(5, 0, d.data_ptr(), out.data_ptr(), False, _stream0(torch))
    ctx.ntt_device(5, 0, d.data_ptr(), out.data_ptr(), True, _stream0(torch))
    ctx.lde_device(5, 1, 0, d.data_ptr(), out.data_ptr(), _stream0(torch))
    torch.cuda.synchronize()
    assert (_to_host(out) == 0x5A5A5A5A5A5A5A5A).all()
