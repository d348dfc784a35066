"""A pure-Python model of constraint set 2 of the ladder rows (include/tmx.h "the boundary constraints of the ladder rows"), written from the
header text and independent of libtmx: the public table from Level-1 element rows, its digest, gamma, V_k, Pub_gamma, the quotient point by
point and in pieces, the identity at zeta and `verify` = tests/batch_model.py's verifier and that identity.  Built on air_model's and
fri_model's helpers.  The yardstick of tests/test_air_boundary.py (not collected by pytest).  Parity unpinned against plonky2."""
import numpy as np

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
from air_model import ACC, ADD, BIT, DBL, LIMBS, NXT, WIDTH
from fri_model import P, e_add, e_mul, e_scale, e_sub

CONSTRAINTS, MAIN, PUB_WIDTH, SET_ID = 65, 33, 17, 2
W_NXT, W_ACC, W_LIVE = 33, 49, 57  # weights' offsets inside a proof's 65; live is the target of acc limb 8 (y limb 0)


# ---- the public table
def d1b_start(kind, n):
    """first element of section D.1b in an element row (docs/witness_layout.md: H, then D.1a = 1136 per lane)"""
    return (1776 * n + 5320 if kind == 0 else 1517 * n + 6919) + 1136 * n


def public_table(kind, n, rows, log_k):
    """rows: one element row per proof.  [17 n_proofs][K] words: D.1b of lane i is 99 elements, sB.x sB.y hA.x hA.y at 40 .. 71"""
    K = 1 << log_k
    assert 2 * n <= K
    pub = np.zeros((PUB_WIDTH * len(rows), K), dtype=np.uint64)
    for p, row in enumerate(rows):
        for i in range(n):
            at = d1b_start(kind, n) + 99 * i + 40
            for k in (0, 1):
                words = np.asarray(row[at + 16 * k:at + 16 * k + 16], dtype=np.uint64)
                pub[PUB_WIDTH * p:PUB_WIDTH * p + 16, 2 * i + k] = words
                pub[PUB_WIDTH * p + 16, 2 * i + k] = 1 if words.any() else 0
    return pub


def digest(oracle, pub):
    """the Poseidon Merkle root (cap height 0) of pub as a column-major oracle of log2 K rows"""
    pub = np.asarray(pub, dtype=np.uint64)
    log_k = pub.shape[1].bit_length() - 1
    return oracle.poseidon_merkle(np.ascontiguousarray(pub).reshape(-1), log_k, pub.shape[0], 0)[-1].reshape(-1)


def gamma(oracle, log_n, log_blowup, cap_height, n_proofs, cap, pub):
    """2^33, the set id 2, log_n, log_blowup, cap_height, n_proofs, the trace cap, the public digest; drawn again while gamma.c1 == 0"""
    ch = fm.Challenger(oracle)
    ch.observe(1 << 33)
    for v in (SET_ID, log_n, log_blowup, cap_height, n_proofs):
        ch.observe(v)
    cap = np.asarray(cap, dtype=np.uint64).reshape(-1)
    assert cap.size == 4 << min(cap_height, log_n)
    ch.observe_all(cap)
    d = digest(oracle, pub)
    assert d.size == 4
    ch.observe_all(d)
    while True:
        g = ch.ext()
        if g[1]:
            return g


def combine(pub, g):
    """V_k = sum_p [sum_l gamma^(65 p + 33 + l) pub[17 p + l][k] + gamma^(65 p + 57) pub[17 p + 16][(k + 1) mod K]]"""
    pub = np.asarray(pub, dtype=np.uint64)
    n_proofs, K = pub.shape[0] // PUB_WIDTH, pub.shape[1]
    V = [(0, 0)] * K
    for p in range(n_proofs):
        gp = [dm.e_pow(g, CONSTRAINTS * p + W_NXT + l) for l in range(LIMBS)]
        gl = dm.e_pow(g, CONSTRAINTS * p + W_LIVE)
        for k in range(K):
            v = V[k]
            for l in range(LIMBS):
                v = e_add(v, e_scale(gp[l], int(pub[PUB_WIDTH * p + l, k]) % P))
            V[k] = e_add(v, e_scale(gl, int(pub[PUB_WIDTH * p + 16, (k + 1) % K]) % P))
    return V


def y_points(oracle, log_n, log_blowup, K):
    """y_k = omega^(256 k + 255), omega = omega_N = w^B"""
    om = pow(oracle.gl_root(log_n), 1 << log_blowup, P)
    return [pow(om, 256 * k + 255, P) for k in range(K)]


def pub_coefficients(oracle, log_n, log_blowup, V):
    """the two planes' coefficients of Pub_gamma (degree < K): V_k = sum_j (c_j omega^(255 j)) omega_K^(j k), so c_j = d_j omega^(-255 j) with
    d the inverse transform of V on the K-subgroup"""
    K = len(V)
    log_k = K.bit_length() - 1
    om = pow(oracle.gl_root(log_n), 1 << log_blowup, P)
    assert oracle.gl_root(log_k) == pow(om, 256, P)  # omega_K = omega^256: the CPU transform's root of that size
    f = pow(pow(om, 255, P), P - 2, P)
    out = []
    for plane in (0, 1):
        d = oracle.ntt(np.array([v[plane] for v in V], dtype=np.uint64), inverse=True)
        c, fk = [], 1
        for x in d:
            c.append(int(x) * fk % P)
            fk = fk * f % P
        out.append(c)
    return out


def pub_on_coset(oracle, log_n, coefs, shift):
    """Pub_gamma at x_i = shift w^i, i < 2^log_n: the two planes"""
    M = 1 << log_n
    out = []
    for c in coefs:
        a, sk = np.zeros(M, dtype=np.uint64), 1
        for j, x in enumerate(c):
            a[j] = x * sk % P
            sk = sk * (shift % P) % P
        out.append(oracle.ntt(a))
    return out


def pub_at(oracle, log_n, log_blowup, V, z):
    """Pub_gamma(z) = S(z) / (K omega_256^-1) sum_k V_k y_k / (z - y_k) for z outside the base field"""
    K = len(V)
    ys = y_points(oracle, log_n, log_blowup, K)
    om = am.omega_256_inv(oracle, log_n)
    zk = dm.e_pow(z, K)
    S = ((zk[0] - om) % P, zk[1])
    acc = (0, 0)
    for v, y in zip(V, ys):
        acc = e_add(acc, e_mul(e_scale(v, y), dm.e_inv(((z[0] - y) % P, z[1]))))
    return e_mul(e_scale(S, pow(K * om % P, P - 2, P)), acc)


# ---- the quotient
def _obj(v):
    return np.array([int(x) % P for x in np.asarray(v, dtype=np.uint64).reshape(-1)], dtype=object)


def quotient(oracle, log_n, log_blowup, n_proofs, cols, pub, shift, g, proofs=None, parts=False):
    """cols: [65 n_proofs][2^log_n] words on the coset; the planar quotient (2 << log_n canonical words).  proofs: a range of proof indices
    (the piece form; the piece that holds proof 0 carries - Pub_gamma / S).  parts: (main part, boundary part) instead of their sum"""
    M, B = 1 << log_n, 1 << log_blowup
    N = M // B
    K = N // 256
    assert 2 <= K <= 4096
    cols = np.asarray(cols, dtype=np.uint64).reshape(n_proofs * WIDTH, M)
    w = oracle.gl_root(log_n)
    xs = [shift % P]
    for _ in range(M - 1):
        xs.append(xs[-1] * w % P)
    zinv = np.array([pow((pow(x, N, P) - 1) % P, P - 2, P) for x in xs[:B]] * (M // B), dtype=object)
    om = am.omega_256_inv(oracle, log_n)
    period = 256 * B
    S = np.array([(pow(x, K, P) - om) % P for x in xs[:period]] * (M // period), dtype=object)
    sinv = np.array([pow(int(s), P - 2, P) for s in S[:period]] * (M // period), dtype=object)
    q = [np.zeros(M, dtype=object), np.zeros(M, dtype=object)]
    b = [np.zeros(M, dtype=object), np.zeros(M, dtype=object)]
    rng = range(n_proofs) if proofs is None else proofs
    for p in rng:
        gp = dm.e_pow(g, CONSTRAINTS * p)
        c = [_obj(col) for col in cols[p * WIDTH:(p + 1) * WIDTH]]
        bit = c[BIT]
        terms = [(bit * bit - bit) % P]
        terms += [(c[NXT + l] - c[DBL + l] - bit * (c[ADD + l] - c[DBL + l])) % P for l in range(LIMBS)]
        terms += [S * ((np.roll(c[ACC + l], -B) - c[NXT + l]) % P) % P for l in range(LIMBS)]
        for t in terms:
            q[0], q[1] = (q[0] + gp[0] * t) % P, (q[1] + gp[1] * t) % P
            gp = e_mul(gp, g)
        for t in [c[NXT + l] for l in range(LIMBS)] + [np.roll(c[ACC + l], -B) for l in range(LIMBS)]:
            b[0], b[1] = (b[0] + gp[0] * t) % P, (b[1] + gp[1] * t) % P
            gp = e_mul(gp, g)
    if 0 in rng:
        ext = pub_on_coset(oracle, log_n, pub_coefficients(oracle, log_n, log_blowup, combine(pub, g)), shift)
        b = [(b[k] - _obj(ext[k])) % P for k in (0, 1)]
    q = [q[k] * zinv % P for k in (0, 1)]
    b = [b[k] * sinv % P for k in (0, 1)]
    flat = lambda v: np.array([int(x) for x in v[0]] + [int(x) for x in v[1]], dtype=np.uint64)
    if parts:
        return flat(q), flat(b)
    return flat([(q[k] + b[k]) % P for k in (0, 1)])


# ---- the identity
def identity_at(oracle, log_n, log_blowup, n_proofs, t0, t1, u0, u1, zeta, g, pub):
    """S(zeta) main + Z (bsum - Pub_gamma(zeta)) == (u_0 + X u_1) Z S(zeta), Z = zeta^N - 1"""
    N = 1 << (log_n - log_blowup)
    K = N // 256
    zk = dm.e_pow(zeta, K)
    S = ((zk[0] - am.omega_256_inv(oracle, log_n)) % P, zk[1])
    zn = dm.e_pow(zeta, N)
    Z = ((zn[0] - 1) % P, zn[1])
    main, bsum = (0, 0), (0, 0)
    for p in range(n_proofs):
        o, gp = p * WIDTH, dm.e_pow(g, CONSTRAINTS * p)
        bit = t0[o + BIT]
        terms = [e_sub(e_mul(bit, bit), bit)]
        terms += [e_sub(e_sub(t0[o + NXT + l], t0[o + DBL + l]), e_mul(bit, e_sub(t0[o + ADD + l], t0[o + DBL + l]))) for l in range(LIMBS)]
        terms += [e_mul(S, e_sub(t1[o + ACC + l], t0[o + NXT + l])) for l in range(LIMBS)]
        for t in terms:
            main = e_add(main, e_mul(gp, t))
            gp = e_mul(gp, g)
        for t in [t0[o + NXT + l] for l in range(LIMBS)] + [t1[o + ACC + l] for l in range(LIMBS)]:
            bsum = e_add(bsum, e_mul(gp, t))
            gp = e_mul(gp, g)
    pub_z = pub_at(oracle, log_n, log_blowup, combine(pub, g), zeta)
    q = ((u0[0] + 7 * u1[1]) % P, (u0[1] + u1[0]) % P)
    lhs = e_add(e_mul(S, main), e_mul(Z, e_sub(bsum, pub_z)))
    return lhs == e_mul(q, e_mul(Z, S))


def identity(oracle, p, k_trace, caps, proof, pub):
    """the set-2 identity from the openings blocks of oracle k_trace (the ladders) and k_trace + 1 (the quotient) of a batch proof"""
    caps = am._caps_list(p, caps)
    log_n, n_cols = p["log_n"][k_trace], p["n_cols"][k_trace]
    assert n_cols % WIDTH == 0 and p["log_n"][k_trace + 1] == log_n and p["n_cols"][k_trace + 1] == 2
    n_proofs = n_cols // WIDTH
    _, zeta = bm._start(oracle, p, caps)
    g = gamma(oracle, log_n, p["log_blowup"], p["cap_height"], n_proofs, caps[k_trace], pub)
    yt, yq = bm.openings_of(p, proof, k_trace), bm.openings_of(p, proof, k_trace + 1)
    return identity_at(oracle, log_n, p["log_blowup"], n_proofs, [y[0] for y in yt], [y[1] for y in yt], yq[0][0], yq[1][0], zeta, g, pub)


def verify(oracle, p, k_trace, caps, proof, shift, pub):
    """[ok] per query: batch_model.verify and the set-2 identity (a failed identity rejects every query)"""
    holds = identity(oracle, p, k_trace, caps, proof, pub)
    return [bool(ok and holds) for ok in bm.verify(oracle, p, caps, proof, shift)]
