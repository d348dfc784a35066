"""A pure-Python model of the ladder rows' constraint quotient (include/tmx.h "the constraint quotient of the ladder rows"), written from
the header text and independent of libtmx: gamma from a fresh duplex over the trace cap, the quotient point by point over the extended
columns, the identity at zeta from a batch proof's openings, and `verify` = tests/batch_model.py's verifier and that identity.  Built on
fri_model's field helpers and duplex; the quotient is vectorised over the rows with numpy object arrays of Python integers.  The yardstick
of tests/test_air.py (not collected by pytest).  Parity unpinned against plonky2, like the feature itself."""
import numpy as np

import batch_model as bm
import deep_model as dm
import fri_model as fm
from fri_model import P, e_add, e_mul, e_scale, e_sub

WIDTH, CONSTRAINTS, LIMBS = 65, 33, 16
BIT, ACC, DBL, ADD, NXT = 0, 1, 17, 33, 49
SET_ID = 1


def gamma(oracle, log_n, log_blowup, cap_height, n_proofs, cap):
    """2^33, the set id, log_n, log_blowup, cap_height, n_proofs, the trace cap; drawn again while gamma.c1 == 0"""
    ch = fm.Challenger(oracle)
    ch.observe(1 << 33)
    for v in (SET_ID, log_n, log_blowup, cap_height, n_proofs):
        ch.observe(v)
    cap = np.asarray(cap, dtype=np.uint64).reshape(-1)
    assert cap.size == 4 << min(cap_height, log_n)
    ch.observe_all(cap)
    while True:
        g = ch.ext()
        if g[1]:
            return g


def omega_256_inv(oracle, log_n):
    """omega_256 = omega_N^(N/256) = w^(M/256)"""
    return pow(pow(oracle.gl_root(log_n), 1 << (log_n - 8), P), P - 2, P)


def _obj(v):
    return np.array([int(x) % P for x in np.asarray(v, dtype=np.uint64).reshape(-1)], dtype=object)


def quotient(oracle, log_n, log_blowup, n_proofs, cols, shift, g, proofs=None):
    """cols: [65 n_proofs][2^log_n] words on the coset shift <gl_root(log_n)>; the planar quotient (2 << log_n canonical words).  proofs: a
    range of proof indices to sum over (default: all) -- the piece form."""
    M, B = 1 << log_n, 1 << log_blowup
    N = M // B
    cols = np.asarray(cols, dtype=np.uint64).reshape(n_proofs * WIDTH, M)
    w = oracle.gl_root(log_n)
    xs = [shift % P]
    for _ in range(M - 1):
        xs.append(xs[-1] * w % P)
    zinv = np.array([pow((pow(x, N, P) - 1) % P, P - 2, P) for x in xs[:B]] * (M // B), dtype=object)
    om = omega_256_inv(oracle, log_n)
    period = min(M, 256 * B)
    S = np.array([(pow(x, N // 256, P) - om) % P for x in xs[:period]] * (M // period), dtype=object)
    q0, q1 = np.zeros(M, dtype=object), np.zeros(M, dtype=object)
    for p in (range(n_proofs) if proofs is None else proofs):
        gp = dm.e_pow(g, CONSTRAINTS * p)
        c = [_obj(col) for col in cols[p * WIDTH:(p + 1) * WIDTH]]
        bit = c[BIT]
        terms = [(bit * bit - bit) % P]
        terms += [(c[NXT + l] - c[DBL + l] - bit * (c[ADD + l] - c[DBL + l])) % P for l in range(LIMBS)]
        terms += [S * ((np.roll(c[ACC + l], -B) - c[NXT + l]) % P) % P for l in range(LIMBS)]
        for t in terms:
            q0 = (q0 + gp[0] * t) % P
            q1 = (q1 + gp[1] * t) % P
            gp = e_mul(gp, g)
    q0, q1 = q0 * zinv % P, q1 * zinv % P
    return np.array([int(x) for x in q0] + [int(x) for x in q1], dtype=np.uint64)


def constraint_sum(oracle, log_n, log_blowup, n_proofs, t0, t1, zeta, g):
    """sum gamma^(33 p + j) C_(p,j)(t^0, t^1; zeta) over F_p^2: t0[c], t1[c] the value of column c at zeta and at zeta omega_N"""
    N = 1 << (log_n - log_blowup)
    zp = dm.e_pow(zeta, N // 256)
    S = ((zp[0] - omega_256_inv(oracle, log_n)) % P, zp[1])
    acc, gp = (0, 0), (1, 0)
    for p in range(n_proofs):
        o = p * WIDTH
        bit = t0[o + BIT]
        terms = [e_sub(e_mul(bit, bit), bit)]
        terms += [e_sub(e_sub(t0[o + NXT + l], t0[o + DBL + l]), e_mul(bit, e_sub(t0[o + ADD + l], t0[o + DBL + l]))) for l in range(LIMBS)]
        terms += [e_mul(S, e_sub(t1[o + ACC + l], t0[o + NXT + l])) for l in range(LIMBS)]
        for t in terms:
            acc = e_add(acc, e_mul(gp, t))
            gp = e_mul(gp, g)
    return acc


def identity_at(oracle, log_n, log_blowup, n_proofs, t0, t1, u0, u1, zeta, g):
    """sum gamma^i C_i == (u_0 + X u_1) (zeta^N - 1), X (a, b) = (7 b, a)"""
    zn = dm.e_pow(zeta, 1 << (log_n - log_blowup))
    q = ((u0[0] + 7 * u1[1]) % P, (u0[1] + u1[0]) % P)
    return constraint_sum(oracle, log_n, log_blowup, n_proofs, t0, t1, zeta, g) == e_mul(q, ((zn[0] - 1) % P, zn[1]))


def _caps_list(p, caps):
    if isinstance(caps, (list, tuple)):
        return [np.asarray(c, dtype=np.uint64).reshape(-1) for c in caps]
    L = bm.layout(p)
    flat, out, at = np.asarray(caps, dtype=np.uint64).reshape(-1), [], 0
    for h in L["cap_height_of"]:
        out.append(flat[at:at + (4 << h)])
        at += 4 << h
    return out


def identity(oracle, p, k_trace, caps, proof):
    """the identity from the openings blocks of oracle k_trace (the ladders) and k_trace + 1 (the quotient) of a batch proof"""
    caps = _caps_list(p, caps)
    log_n, n_cols = p["log_n"][k_trace], p["n_cols"][k_trace]
    assert n_cols % WIDTH == 0 and p["log_n"][k_trace + 1] == log_n and p["n_cols"][k_trace + 1] == 2
    n_proofs = n_cols // WIDTH
    _, zeta = bm._start(oracle, p, caps)
    g = gamma(oracle, log_n, p["log_blowup"], p["cap_height"], n_proofs, caps[k_trace])
    yt, yq = bm.openings_of(p, proof, k_trace), bm.openings_of(p, proof, k_trace + 1)
    return identity_at(oracle, log_n, p["log_blowup"], n_proofs, [y[0] for y in yt], [y[1] for y in yt], yq[0][0], yq[1][0], zeta, g)


def verify(oracle, p, k_trace, caps, proof, shift):
    """[ok] per query: batch_model.verify and the identity (a failed identity rejects every query)"""
    holds = identity(oracle, p, k_trace, caps, proof)
    return [bool(ok and holds) for ok in bm.verify(oracle, p, caps, proof, shift)]


def coefficients(oracle, plane, shift):
    """the coefficients of the polynomial with these values on shift <gl_root(log len)>"""
    c = oracle.ntt(np.asarray(plane, dtype=np.uint64), inverse=True)
    s_inv, sk, out = pow(shift % P, P - 2, P), 1, []
    for x in c:
        out.append(int(x) * sk % P)
        sk = sk * s_inv % P
    return out


def degree(coefs):
    """of a list of base-field coefficients; -1 for the zero polynomial"""
    for k in range(len(coefs) - 1, -1, -1):
        if coefs[k]:
            return k
    return -1


def horner(coefs, z):
    acc = (0, 0)
    for c in reversed(coefs):
        acc = e_add(e_mul(acc, z), (c, 0))
    return acc
