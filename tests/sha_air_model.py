"""A pure-Python model of the SHA-256 tables' round constraints (include/tmx.h "the round constraints of the SHA-256 tables", constraint
set 3), written from the header text and independent of libtmx: the helper oracle of bits, gamma from a fresh duplex over the table cap and
the helper cap, the quotient point by point over the extended columns, the identity at zeta from a batch proof's openings, and `verify` =
tests/batch_model.py's verifier and that identity.  A sibling of tests/air_model.py, built on the same field helpers and duplex; the 315
constraints are written ONCE (`_constraints`) over an abstract field, used with numpy object arrays of Python integers on the coset and with
F_p^2 pairs at zeta.  The yardstick of tests/test_sha_air.py (not collected by pytest).  Parity unpinned against plonky2, like the feature."""
import numpy as np

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
from fri_model import P, e_add, e_mul, e_sub

WIDTH, HELPER_COLS, CONSTRAINTS = 9, 300, 315
SET_ID = 3
W_, A_, B_, C_, D_, E_, F_, G_, H_ = range(9)  # the table's columns inside a proof
HA, HB, HC, HE, HF, HG, HU0, HU1, HV = 0, 32, 64, 96, 128, 160, 192, 224, 256  # the helper's bit groups
HS0, HS1, HCH, HMAJ, HLIVE, HKL, HCA, HCE = 288, 289, 290, 291, 292, 293, 294, 297
MASK = 0xFFFFFFFF

K256 = [
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
    0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
    0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]


def rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & MASK


def sigma0(a):
    return rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)


def sigma1(e):
    return rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)


def ch(e, f, g):
    return (e & f) ^ (~e & g & MASK)


def maj(a, b, c):
    return (a & b) ^ (a & c) ^ (b & c)


def sha_round(state, w, t):
    """the state (a .. h) after round t from the state before it and W_t"""
    a, b, c, d, e, f, g, h = state
    t1 = h + sigma1(e) + ch(e, f, g) + K256[t] + w
    t2 = sigma0(a) + maj(a, b, c)
    return [(t1 + t2) & MASK, a, b, c, (d + t1) & MASK, e, f, g]


# ---- the helper oracle
def helper(table, n_proofs):
    """table: [9 n_proofs][R] words (pre-LDE, any 64-bit words: the operands are their low 32 bits); the helper [300 n_proofs][R].
    Vectorised over the rows with numpy uint64 (every intermediate stays below 2^35)."""
    table = np.asarray(table, dtype=np.uint64).reshape(n_proofs * WIDTH, -1)
    R = table.shape[1]
    assert R % 64 == 0
    u = np.uint64
    out = np.zeros((n_proofs * HELPER_COLS, R), dtype=np.uint64)
    bit = lambda x, i: (x >> u(i % 32)) & u(1)
    rot = lambda x, n: ((x >> u(n)) | (x << u(32 - n))) & u(MASK)
    r = np.arange(R)
    k_row = np.array(K256, dtype=np.uint64)[r % 64]
    for p in range(n_proofs):
        full = table[p * WIDTH:(p + 1) * WIDTH]
        w = full & u(MASK)
        o = out[p * HELPER_COLS:(p + 1) * HELPER_COLS]
        a, b, c, e, f, g = w[A_], w[B_], w[C_], w[E_], w[F_], w[G_]
        for i in range(32):
            o[HA + i], o[HB + i], o[HC + i], o[HE + i], o[HF + i], o[HG + i] = bit(a, i), bit(b, i), bit(c, i), bit(e, i), bit(f, i), bit(g, i)
            o[HU0 + i] = bit(a, i + 2) ^ bit(a, i + 13)
            o[HU1 + i] = bit(e, i + 6) ^ bit(e, i + 11)
            o[HV + i] = bit(a, i) & bit(b, i)
        s0, s1 = rot(a, 2) ^ rot(a, 13) ^ rot(a, 22), rot(e, 6) ^ rot(e, 11) ^ rot(e, 25)
        c_, m = (e & f) ^ (~e & g & u(MASK)), (a & b) ^ (a & c) ^ (b & c)
        live = (full[:, r - r % 64] != 0).any(axis=0).astype(np.uint64)
        kl = live * k_row
        o[HS0], o[HS1], o[HCH], o[HMAJ], o[HLIVE], o[HKL] = s0, s1, c_, m, live, kl
        inner = r % 64 != 63
        t1 = w[H_] + s1 + c_ + np.roll(kl, -1) + np.roll(w[W_], -1)
        ca, ce = ((t1 + s0 + m) >> u(32)) & u(7), ((w[D_] + t1) >> u(32)) & u(7)
        for k in range(3):
            o[HCA + k], o[HCE + k] = ((ca >> u(k)) & u(1)) * inner, ((ce >> u(k)) & u(1)) * inner
    return out


# ---- the 315 constraints over an abstract field
class _Field:
    """add, sub, mul on elements; k(c) an element from a base-field constant"""


def _base():
    """Python integers (in numpy object arrays): sums and differences are left unreduced, products reduced -- the caller reduces at the end"""
    f = _Field()
    f.add, f.sub, f.mul = (lambda a, b: a + b), (lambda a, b: a - b), (lambda a, b: a * b % P)
    f.k = lambda c: c % P
    return f


_U = np.uint64
_M32, _P64 = _U(0xFFFFFFFF), _U(P)


def _addv(a, b):
    """canonical uint64 arrays: 2^64 = 2^32 - 1 (mod p) after a wrap"""
    s = a + b
    s = np.where(s < a, s + _M32, s)
    return np.where(s >= _P64, s - _P64, s)


def _subv(a, b):
    return np.where(a < b, a - b + _P64, a - b)


def _mulv(a, b):
    """the 128-bit product from four 32 x 32 products, then x = lo + 2^64 hi_lo + 2^96 hi_hi = lo + (2^32 - 1) hi_lo - hi_hi (mod p)"""
    a0, a1, b0, b1 = a & _M32, a >> _U(32), b & _M32, b >> _U(32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = p01 + (p00 >> _U(32))
    mid2 = p10 + (mid & _M32)
    lo = (mid2 << _U(32)) | (p00 & _M32)
    hi = p11 + (mid >> _U(32)) + (mid2 >> _U(32))
    hi_lo, hi_hi = hi & _M32, hi >> _U(32)
    t = np.where(lo < hi_hi, lo - hi_hi - _M32, lo - hi_hi)
    r = t + hi_lo * _M32
    r = np.where(r < t, r + _M32, r)
    return np.where(r >= _P64, r - _P64, r)


def _vec():
    """canonical numpy uint64 arrays (the quotient over a whole coset; checked against Python integers in tests/test_sha_air.py)"""
    f = _Field()
    f.add, f.sub, f.mul, f.k = _addv, _subv, _mulv, (lambda c: _U(c % P))
    return f


def _ext():
    f = _Field()
    f.add, f.sub, f.mul, f.k = e_add, e_sub, e_mul, (lambda c: (c % P, 0))
    return f


def _constraints(f, t, tn, h, hn, S, K):
    """the 315 constraints of one proof: t[c], h[c] the table's and the helper's columns at x, tn, hn at omega x; S and K the values of the
    selector and of the round-constant polynomial at x"""
    add, sub, mul, k = f.add, f.sub, f.mul, f.k
    two = k(2)
    boolean = lambda x: sub(mul(x, x), x)
    xor = lambda x, y: sub(add(x, y), mul(two, mul(x, y)))

    def word(bits):
        acc = k(0)
        for i in range(31, -1, -1):
            acc = add(mul(acc, two), bits[i])
        return acc
    out = [boolean(h[c]) for c in range(192)]
    out += [boolean(h[c]) for c in range(HCA, HCA + 6)]
    out.append(boolean(h[HLIVE]))
    for col, at in ((A_, HA), (B_, HB), (C_, HC), (E_, HE), (F_, HF), (G_, HG)):
        out.append(sub(t[col], word([h[at + i] for i in range(32)])))
    Ab, Bb, Cb = (lambda i: h[HA + i % 32]), (lambda i: h[HB + i % 32]), (lambda i: h[HC + i % 32])
    Eb, Fb, Gb = (lambda i: h[HE + i % 32]), (lambda i: h[HF + i % 32]), (lambda i: h[HG + i % 32])
    out += [sub(h[HU0 + i], xor(Ab(i + 2), Ab(i + 13))) for i in range(32)]
    out += [sub(h[HU1 + i], xor(Eb(i + 6), Eb(i + 11))) for i in range(32)]
    out += [sub(h[HV + i], mul(Ab(i), Bb(i))) for i in range(32)]
    out.append(sub(h[HS0], word([xor(h[HU0 + i], Ab(i + 22)) for i in range(32)])))
    out.append(sub(h[HS1], word([xor(h[HU1 + i], Eb(i + 25)) for i in range(32)])))
    out.append(sub(h[HCH], word([add(Gb(i), mul(Eb(i), sub(Fb(i), Gb(i)))) for i in range(32)])))
    out.append(sub(h[HMAJ], word([add(h[HV + i], mul(Cb(i), sub(add(Ab(i), Bb(i)), mul(two, h[HV + i])))) for i in range(32)])))
    out.append(sub(h[HKL], mul(h[HLIVE], K)))
    for nxt, cur in ((B_, A_), (C_, B_), (D_, C_), (F_, E_), (G_, F_), (H_, G_)):
        out.append(mul(S, sub(tn[nxt], t[cur])))
    out.append(mul(S, sub(hn[HLIVE], h[HLIVE])))
    c32 = lambda at: mul(k(1 << 32), add(h[at], add(mul(two, h[at + 1]), mul(k(4), h[at + 2]))))
    t1 = add(add(add(t[H_], h[HS1]), add(h[HCH], hn[HKL])), tn[W_])
    out.append(mul(S, sub(add(tn[A_], c32(HCA)), add(t1, add(h[HS0], h[HMAJ])))))
    out.append(mul(S, sub(add(tn[E_], c32(HCE)), add(t[D_], t1))))
    assert len(out) == CONSTRAINTS
    return out


def integer_residuals(table, help_):
    """the 315 constraints of ONE proof as integer expressions (no reduction mod p) on pre-LDE rows; the selected ones are set to zero on the
    rows r = 63 mod 64; K = K256[r mod 64].  Returns [315][R] Python integers as object arrays."""
    f = _Field()
    f.add, f.sub, f.mul, f.k = (lambda a, b: a + b), (lambda a, b: a - b), (lambda a, b: a * b), (lambda c: c)
    t = [np.array([int(x) for x in col], dtype=object) for col in np.asarray(table, dtype=np.uint64).reshape(WIDTH, -1)]
    h = [np.array([int(x) for x in col], dtype=object) for col in np.asarray(help_, dtype=np.uint64).reshape(HELPER_COLS, -1)]
    R = t[0].size
    S = np.array([0 if r % 64 == 63 else 1 for r in range(R)], dtype=object)
    K = np.array([K256[r % 64] for r in range(R)], dtype=object)
    return _constraints(f, t, [np.roll(c, -1) for c in t], h, [np.roll(c, -1) for c in h], S, K)


# ---- gamma, the tables on the coset, the quotient
def gamma(oracle, log_n, log_blowup, cap_height, n_proofs, cap, cap_helper):
    """2^33, the set id 3, log_n, log_blowup, cap_height, n_proofs, the table cap, the helper cap; drawn again while gamma.c1 == 0"""
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


def omega_64(oracle, log_n):
    """omega_64 = omega_N^(N/64) = w^(M/64)"""
    return pow(oracle.gl_root(log_n), 1 << (log_n - 6), P)


def k_coefficients(oracle, log_n):
    """P_K: degree < 64, P_K(omega_64^t) = K256[t] (an inverse transform written out)"""
    om_inv, n_inv = pow(omega_64(oracle, log_n), P - 2, P), pow(64, P - 2, P)
    return [sum(K256[t] * pow(om_inv, j * t, P) for t in range(64)) * n_inv % P for j in range(64)]


def _obj(v):
    return np.array([int(x) % P for x in np.asarray(v, dtype=np.uint64).reshape(-1)], dtype=object)


def quotient(oracle, log_n, log_blowup, n_proofs, cols, hcols, shift, g, ints=False):
    """cols [9 n_proofs][M], hcols [300 n_proofs][M] words on the coset shift <gl_root(log_n)>; the planar quotient (2 M canonical words).
    ints: with Python integers in object arrays instead of the uint64 field above (slow; the cross-check of the two)"""
    M, B = 1 << log_n, 1 << log_blowup
    N = M // B
    cols = np.asarray(cols, dtype=np.uint64).reshape(n_proofs * WIDTH, M)
    hcols = np.asarray(hcols, dtype=np.uint64).reshape(n_proofs * HELPER_COLS, M)
    w = oracle.gl_root(log_n)
    xs = [shift % P]
    for _ in range(M - 1):
        xs.append(xs[-1] * w % P)
    om_inv, pk = pow(omega_64(oracle, log_n), P - 2, P), k_coefficients(oracle, log_n)
    period = min(M, 64 * B)
    ys = [pow(x, N // 64, P) for x in xs[:period]]
    dt = object if ints else np.uint64
    zinv = np.array([pow((pow(x, N, P) - 1) % P, P - 2, P) for x in xs[:B]] * (M // B), dtype=dt)
    S = np.array([(y - om_inv) % P for y in ys] * (M // period), dtype=dt)
    K = np.array([am.horner(pk, (y, 0))[0] for y in ys] * (M // period), dtype=dt)
    f = _base() if ints else _vec()
    canon = _obj if ints else (lambda v: np.asarray(v, dtype=np.uint64) % _P64)
    q0, q1 = np.zeros(M, dtype=dt), np.zeros(M, dtype=dt)
    gp = (1, 0)
    with np.errstate(over="ignore"):
        for p in range(n_proofs):
            t = [canon(c) for c in cols[p * WIDTH:(p + 1) * WIDTH]]
            h = [canon(c) for c in hcols[p * HELPER_COLS:(p + 1) * HELPER_COLS]]
            for term in _constraints(f, t, [np.roll(c, -B) for c in t], h, [np.roll(c, -B) for c in h], S, K):
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
    """sum gamma^(315 p + j) C_(p,j) over F_p^2 from the openings at zeta (t0, h0) and zeta omega_N (t1, h1)"""
    N = 1 << (log_n - log_blowup)
    y = dm.e_pow(zeta, N // 64)
    S = ((y[0] - pow(omega_64(oracle, log_n), P - 2, P)) % P, y[1])
    K = am.horner(k_coefficients(oracle, log_n), y)
    f = _ext()
    acc, gp = (0, 0), (1, 0)
    for p in range(n_proofs):
        a, b = p * WIDTH, p * HELPER_COLS
        for term in _constraints(f, t0[a:a + WIDTH], t1[a:a + WIDTH], h0[b:b + HELPER_COLS], h1[b:b + HELPER_COLS], S, K):
            acc = e_add(acc, e_mul(gp, term))
            gp = e_mul(gp, g)
    return acc


def identity_at(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, u0, u1, zeta, g):
    """sum gamma^i C_i == (u_0 + X u_1) (zeta^N - 1), X (a, b) = (7 b, a)"""
    zn = dm.e_pow(zeta, 1 << (log_n - log_blowup))
    q = ((u0[0] + 7 * u1[1]) % P, (u0[1] + u1[0]) % P)
    return constraint_sum(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, zeta, g) == e_mul(q, ((zn[0] - 1) % P, zn[1]))


def identity(oracle, p, k_trace, caps, proof):
    """the identity from the openings blocks of oracle k_trace (the table), k_trace + 1 (the helper) and k_trace + 2 (the quotient)"""
    caps = am._caps_list(p, caps)
    log_n, n_cols = p["log_n"][k_trace], p["n_cols"][k_trace]
    assert n_cols % WIDTH == 0
    n_proofs = n_cols // WIDTH
    assert p["log_n"][k_trace + 1] == log_n and p["n_cols"][k_trace + 1] == HELPER_COLS * n_proofs
    assert p["log_n"][k_trace + 2] == log_n and p["n_cols"][k_trace + 2] == 2
    _, zeta = bm._start(oracle, p, caps)
    g = gamma(oracle, log_n, p["log_blowup"], p["cap_height"], n_proofs, caps[k_trace], caps[k_trace + 1])
    yt, yh, yq = (bm.openings_of(p, proof, k_trace + d) for d in range(3))
    return identity_at(oracle, log_n, p["log_blowup"], n_proofs, [y[0] for y in yt], [y[1] for y in yt], [y[0] for y in yh], [y[1] for y in yh],
                       yq[0][0], yq[1][0], zeta, g)


def verify(oracle, p, k_trace, caps, proof, shift):
    """[ok] per query: batch_model.verify and the identity (a failed identity rejects every query)"""
    holds = identity(oracle, p, k_trace, caps, proof)
    return [bool(ok and holds) for ok in bm.verify(oracle, p, caps, proof, shift)]
