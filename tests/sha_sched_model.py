"""A pure-Python model of the SHA-256 tables' message-schedule constraints (include/tmx.h "the message schedule of the SHA-256 tables",
constraint set 4), written from the header text and independent of libtmx: the helper oracle (the bits of W, the two xor rows, sigma0 and
sigma1 as words, the schedule sum as a pipeline of fifteen columns, two carry bits), gamma from a fresh duplex over the table cap and the
helper cap, the quotient point by point over the extended columns, the identity at zeta from a batch proof's openings, and `verify` =
tests/batch_model.py's verifier and that identity, with the helper's oracle index explicit.  A sibling of tests/sha_air_model.py, whose
field helpers it imports; the 117 constraints are written ONCE (`_constraints`) over an abstract field.  The yardstick of
tests/test_sha_sched.py (not collected by pytest).  Parity unpinned against plonky2, like the feature."""
import numpy as np

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha_air_model as sm
from fri_model import P, e_add, e_mul
from sha_air_model import _Field, _addv, _base, _ext, _mulv, _obj, _vec, omega_64

WIDTH, HELPER_COLS, CONSTRAINTS = 9, 115, 117
SET_ID = 4
W_ = 0  # the table's W column inside a proof
HWB, HX0, HX1, HG0, HG1, HQ, HCW = 0, 32, 64, 96, 97, 97, 113  # the helper's columns; Q_k at HQ + k, k = 1 .. 15
JCW, JWORD, JX0, JX1, JG0, JG1, JQ, JNEXT = 32, 34, 35, 67, 99, 100, 100, 116  # constraint indices; Q_k's at JQ + k
MASK = 0xFFFFFFFF
_U = np.uint64


def small_sigma0(w):
    return sm.rotr(w, 7) ^ sm.rotr(w, 18) ^ (w >> 3)


def small_sigma1(w):
    return sm.rotr(w, 17) ^ sm.rotr(w, 19) ^ (w >> 10)


def schedule_row(r):
    """F's support: the NEXT row is a schedule row (W_t, t = r mod 64 + 1 in 16 .. 63)"""
    return 15 <= r % 64 <= 62


# ---- the helper oracle
def helper(table, n_proofs):
    """table: [9 n_proofs][R] words (pre-LDE, any 64-bit words: W is the low 32 bits of column 0); the helper [115 n_proofs][R].  Rows are
    cyclic inside one proof.  Vectorised over the rows with numpy uint64 (every intermediate stays below 2^34)."""
    table = np.asarray(table, dtype=np.uint64).reshape(n_proofs * WIDTH, -1)
    R = table.shape[1]
    assert R % 64 == 0
    out = np.zeros((n_proofs * HELPER_COLS, R), dtype=np.uint64)
    bit = lambda x, i: (x >> _U(i % 32)) & _U(1)
    rot = lambda x, n: ((x >> _U(n)) | (x << _U(32 - n))) & _U(MASK)
    sched = np.array([schedule_row(r) for r in range(R)], dtype=np.uint64)
    for p in range(n_proofs):
        w = table[p * WIDTH + W_] & _U(MASK)
        o = out[p * HELPER_COLS:(p + 1) * HELPER_COLS]
        for i in range(32):
            o[HWB + i] = bit(w, i)
            o[HX0 + i] = bit(w, i + 7) ^ bit(w, i + 18)
            o[HX1 + i] = bit(w, i + 17) ^ bit(w, i + 19)
        g0 = rot(w, 7) ^ rot(w, 18) ^ (w >> _U(3))
        g1 = rot(w, 17) ^ rot(w, 19) ^ (w >> _U(10))
        o[HG0], o[HG1] = g0, g1
        o[HQ + 1] = np.roll(w, 1) + g0
        for k in range(2, 16):
            o[HQ + k] = np.roll(o[HQ + k - 1], 1) + (w if k == 9 else 0) + (g1 if k == 14 else 0)
        cw = ((o[HQ + 15] >> _U(32)) & _U(3)) * sched
        o[HCW], o[HCW + 1] = cw & _U(1), cw >> _U(1)
    return out


# ---- the 117 constraints over an abstract field
def _constraints(f, t, tn, h, hn, F):
    """the 117 constraints of one proof: t[c], h[c] the table's and the helper's columns at x, tn, hn at omega x; F the value of the
    selector polynomial (the next row is a schedule row) at x"""
    add, sub, mul, k = f.add, f.sub, f.mul, f.k
    two = k(2)
    boolean = lambda x: sub(mul(x, x), x)
    xor = lambda x, y: sub(add(x, y), mul(two, mul(x, y)))

    def word(bits):
        acc = k(0)
        for i in range(31, -1, -1):
            acc = add(mul(acc, two), bits[i])
        return acc
    wb = lambda i: h[HWB + i % 32]
    out = [boolean(h[HWB + i]) for i in range(32)]
    out += [boolean(h[HCW]), boolean(h[HCW + 1])]
    out.append(sub(t[W_], word([h[HWB + i] for i in range(32)])))
    out += [sub(h[HX0 + i], xor(wb(i + 7), wb(i + 18))) for i in range(32)]
    out += [sub(h[HX1 + i], xor(wb(i + 17), wb(i + 19))) for i in range(32)]
    out.append(sub(h[HG0], word([xor(h[HX0 + i], wb(i + 3)) if i < 29 else h[HX0 + i] for i in range(32)])))
    out.append(sub(h[HG1], word([xor(h[HX1 + i], wb(i + 10)) if i < 22 else h[HX1 + i] for i in range(32)])))
    out.append(sub(hn[HQ + 1], add(t[W_], hn[HG0])))
    for q in range(2, 16):
        rhs = h[HQ + q - 1]
        if q == 9:
            rhs = add(rhs, tn[W_])
        if q == 14:
            rhs = add(rhs, hn[HG1])
        out.append(sub(hn[HQ + q], rhs))
    carry = mul(k(1 << 32), add(h[HCW], mul(two, h[HCW + 1])))
    out.append(mul(F, sub(add(tn[W_], carry), h[HQ + 15])))
    assert len(out) == CONSTRAINTS
    return out


def integer_residuals(table, help_):
    """the 117 constraints of ONE proof as integer expressions (no reduction mod p) on pre-LDE rows, rows cyclic; F = 1 on the rows with
    r mod 64 in 15 .. 62 and 0 elsewhere.  Returns [117][R] Python integers as object arrays."""
    f = _Field()
    f.add, f.sub, f.mul, f.k = (lambda a, b: a + b), (lambda a, b: a - b), (lambda a, b: a * b), (lambda c: c)
    t = [np.array([int(x) for x in col], dtype=object) for col in np.asarray(table, dtype=np.uint64).reshape(WIDTH, -1)]
    h = [np.array([int(x) for x in col], dtype=object) for col in np.asarray(help_, dtype=np.uint64).reshape(HELPER_COLS, -1)]
    R = t[0].size
    F = np.array([1 if schedule_row(r) else 0 for r in range(R)], dtype=object)
    return _constraints(f, t, [np.roll(c, -1) for c in t], h, [np.roll(c, -1) for c in h], F)


# ---- gamma, the tables on the coset, the quotient
def gamma(oracle, log_n, log_blowup, cap_height, n_proofs, cap, cap_helper):
    """2^33, the set id 4, log_n, log_blowup, cap_height, n_proofs, the table cap, the helper cap; drawn again while gamma.c1 == 0"""
    chal = fm.Challenger(oracle)
    chal.observe(1 << 33)
    for v in (SET_ID, log_n, log_blowup, cap_height, n_proofs):
        chal.observe(v)
    for c in (cap, cap_helper):
        c = np.asarray(c, dtype=np.uint64).reshape(-1)
        assert c.size == 4 << min(cap_height, log_n)
        chal.observe_all(c)
    while True:
        g = chal.ext()
        if g[1]:
            return g


def f_coefficients(oracle, log_n):
    """P_F: degree < 64, P_F(omega_64^t) = 1 for 15 <= t <= 62 and 0 otherwise (an inverse transform written out)"""
    om_inv, n_inv = pow(omega_64(oracle, log_n), P - 2, P), pow(64, P - 2, P)
    return [sum(pow(om_inv, j * t, P) for t in range(15, 63)) * n_inv % P for j in range(64)]


def quotient(oracle, log_n, log_blowup, n_proofs, cols, hcols, shift, g, ints=False):
    """cols [9 n_proofs][M], hcols [115 n_proofs][M] words on the coset shift <gl_root(log_n)>; the planar quotient (2 M canonical words).
    ints: with Python integers in object arrays instead of the uint64 field (slow; the cross-check of the two)"""
    M, B = 1 << log_n, 1 << log_blowup
    N = M // B
    cols = np.asarray(cols, dtype=np.uint64).reshape(n_proofs * WIDTH, M)
    hcols = np.asarray(hcols, dtype=np.uint64).reshape(n_proofs * HELPER_COLS, M)
    w = oracle.gl_root(log_n)
    xs = [shift % P]
    for _ in range(M - 1):
        xs.append(xs[-1] * w % P)
    pf = f_coefficients(oracle, log_n)
    period = min(M, 64 * B)
    ys = [pow(x, N // 64, P) for x in xs[:period]]
    dt = object if ints else np.uint64
    zinv = np.array([pow((pow(x, N, P) - 1) % P, P - 2, P) for x in xs[:B]] * (M // B), dtype=dt)
    F = np.array([am.horner(pf, (y, 0))[0] for y in ys] * (M // period), dtype=dt)
    f = _base() if ints else _vec()
    canon = _obj if ints else (lambda v: np.asarray(v, dtype=np.uint64) % _U(P))
    q0, q1 = np.zeros(M, dtype=dt), np.zeros(M, dtype=dt)
    gp = (1, 0)
    with np.errstate(over="ignore"):
        for p in range(n_proofs):
            t = [canon(c) for c in cols[p * WIDTH:(p + 1) * WIDTH]]
            h = [canon(c) for c in hcols[p * HELPER_COLS:(p + 1) * HELPER_COLS]]
            for term in _constraints(f, t, [np.roll(c, -B) for c in t], h, [np.roll(c, -B) for c in h], F):
                if ints:
                    term = term % P
                    q0, q1 = q0 + gp[0] * term, q1 + gp[1] * term
                else:
                    q0, q1 = _addv(q0, _mulv(term, _U(gp[0]))), _addv(q1, _mulv(term, _U(gp[1])))
                gp = e_mul(gp, g)
        q0, q1 = (q0 % P * zinv % P, q1 % P * zinv % P) if ints else (_mulv(q0, zinv), _mulv(q1, zinv))
    return np.array([int(x) for x in q0] + [int(x) for x in q1], dtype=np.uint64)


# ---- the identity at zeta
def constraint_sum(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, zeta, g):
    """sum gamma^(117 p + j) C_(p,j) over F_p^2 from the openings at zeta (t0, h0) and zeta omega_N (t1, h1)"""
    N = 1 << (log_n - log_blowup)
    F = am.horner(f_coefficients(oracle, log_n), dm.e_pow(zeta, N // 64))
    f = _ext()
    acc, gp = (0, 0), (1, 0)
    for p in range(n_proofs):
        a, b = p * WIDTH, p * HELPER_COLS
        for term in _constraints(f, t0[a:a + WIDTH], t1[a:a + WIDTH], h0[b:b + HELPER_COLS], h1[b:b + HELPER_COLS], F):
            acc = e_add(acc, e_mul(gp, term))
            gp = e_mul(gp, g)
    return acc


def identity_at(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, u0, u1, zeta, g):
    """sum gamma^i C_i == (u_0 + X u_1) (zeta^N - 1), X (a, b) = (7 b, a)"""
    zn = dm.e_pow(zeta, 1 << (log_n - log_blowup))
    q = ((u0[0] + 7 * u1[1]) % P, (u0[1] + u1[0]) % P)
    return constraint_sum(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, zeta, g) == e_mul(q, ((zn[0] - 1) % P, zn[1]))


def identity(oracle, p, k_trace, k_helper, caps, proof):
    """the identity from the openings blocks of oracle k_trace (the table), k_helper (the helper) and k_helper + 1 (the quotient)"""
    caps = am._caps_list(p, caps)
    log_n, n_cols = p["log_n"][k_trace], p["n_cols"][k_trace]
    assert n_cols % WIDTH == 0 and k_helper > k_trace
    n_proofs = n_cols // WIDTH
    assert p["log_n"][k_helper] == log_n and p["n_cols"][k_helper] == HELPER_COLS * n_proofs
    assert p["log_n"][k_helper + 1] == log_n and p["n_cols"][k_helper + 1] == 2
    _, zeta = bm._start(oracle, p, caps)
    g = gamma(oracle, log_n, p["log_blowup"], p["cap_height"], n_proofs, caps[k_trace], caps[k_helper])
    yt, yh, yq = (bm.openings_of(p, proof, k) for k in (k_trace, k_helper, k_helper + 1))
    return identity_at(oracle, log_n, p["log_blowup"], n_proofs, [y[0] for y in yt], [y[1] for y in yt], [y[0] for y in yh], [y[1] for y in yh],
                       yq[0][0], yq[1][0], zeta, g)


def verify(oracle, p, k_trace, k_helper, caps, proof, shift):
    """[ok] per query: batch_model.verify and the identity (a failed identity rejects every query)"""
    holds = identity(oracle, p, k_trace, k_helper, caps, proof)
    return [bool(ok and holds) for ok in bm.verify(oracle, p, caps, proof, shift)]
