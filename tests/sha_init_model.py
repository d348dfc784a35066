"""A pure-Python model of the SHA-256 tables' block-start constraints (include/tmx.h "the block starts of the SHA-256 tables", constraint
set 5), written from the header text and independent of libtmx: the helper oracle (the bits of b, c, d, f, g, h of a row -- six of the
eight words a block starts from stand in its row 0 -- the xor rows, Sigma0, Sigma1, Ch and Maj as words, LV, the feed-forward words PZ with
their carry bits CZ, and the carry bits of the two round-0 sums), gamma from a fresh duplex over the table cap and the helper cap with the
mode in the first observed word, the quotient point by point over the extended columns with its two selector denominators, the
division-free identity at zeta from a batch proof's openings, and `verify` = tests/batch_model.py's verifier and that identity.  A sibling
of tests/sha_sched_model.py; the 337 constraints are written ONCE (`_constraints`) over an abstract field.  The yardstick of
tests/test_sha_init.py (not collected by pytest).  Parity unpinned against plonky2, like the feature."""
import numpy as np

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha_air_model as sm
from fri_model import P, e_add, e_mul, e_sub
from sha_air_model import _Field, _addv, _base, _ext, _mulv, _obj, _vec, omega_64

WIDTH, HELPER_COLS, CONSTRAINTS = 9, 315, 337
SET_ID = 5
W_, A_, B_, C_, D_, E_, F_, G_, H_ = range(9)  # the table's columns inside a proof; the state column s_j is column 1 + j
HB, HC, HD, HF, HG, HH, HU0, HU1, HV = 0, 32, 64, 96, 128, 160, 192, 224, 256  # the helper's bit groups
HS0, HS1, HCH, HMAJ, HLV, HPZ, HCZ, HCA, HCE = 288, 289, 290, 291, 292, 293, 301, 309, 312
JCZ, JCARRY, JLV, JWORD, JU0, JU1, JV, JS0, JS1, JCH, JMAJ, JPZ, JSTART, JCHAIN = 192, 200, 206, 207, 213, 245, 277, 309, 310, 311, 312, 313, 321, 329
MASK = 0xFFFFFFFF
IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]
K0 = sm.K256[0]
SHIFTED = ((B_, 0), (C_, 1), (D_, 2), (F_, 4), (G_, 5), (H_, 6))  # (the column x of the next row, the j of the word H_j it must equal)
_U = np.uint64


def boundary_row(r):
    return r % 64 == 63


def chain_row(r, chain):
    """the next row continues a hash: the second block of a pair on a 128-row boundary"""
    return bool(chain) and r % 128 == 63


def start_row(r, chain):
    return boundary_row(r) and not chain_row(r, chain)


# ---- the helper oracle
def helper(table, n_proofs, chain):
    """table: [9 n_proofs][R] words (pre-LDE, any 64-bit words: the operands are their low 32 bits); the helper [315 n_proofs][R].  Rows
    are cyclic inside one proof.  Vectorised over the rows with numpy uint64 (every intermediate stays below 2^35)."""
    table = np.asarray(table, dtype=np.uint64).reshape(n_proofs * WIDTH, -1)
    R = table.shape[1]
    assert chain in (0, 1) and R % (128 if chain else 64) == 0
    out = np.zeros((n_proofs * HELPER_COLS, R), dtype=np.uint64)
    bit = lambda x, i: (x >> _U(i % 32)) & _U(1)
    rot = lambda x, n: ((x >> _U(n)) | (x << _U(32 - n))) & _U(MASK)
    nxt = lambda v: np.roll(v, -1)
    r = np.arange(R)
    bound = np.array([boundary_row(x) for x in r], dtype=np.uint64)
    chained = np.array([chain_row(x, chain) for x in r], dtype=bool)
    for p in range(n_proofs):
        full = table[p * WIDTH:(p + 1) * WIDTH]
        w = full & _U(MASK)
        o = out[p * HELPER_COLS:(p + 1) * HELPER_COLS]
        b, c, d, f, g, h = w[B_], w[C_], w[D_], w[F_], w[G_], w[H_]
        for i in range(32):
            o[HB + i], o[HC + i], o[HD + i], o[HF + i], o[HG + i], o[HH + i] = bit(b, i), bit(c, i), bit(d, i), bit(f, i), bit(g, i), bit(h, i)
            o[HU0 + i] = bit(b, i + 2) ^ bit(b, i + 13)
            o[HU1 + i] = bit(f, i + 6) ^ bit(f, i + 11)
            o[HV + i] = bit(b, i) & bit(c, i)
        s0, s1 = rot(b, 2) ^ rot(b, 13) ^ rot(b, 22), rot(f, 6) ^ rot(f, 11) ^ rot(f, 25)
        c_, m = (f & g) ^ (~f & h & _U(MASK)), (b & c) ^ (b & d) ^ (c & d)
        live = (full[:, r - r % 64] != 0).any(axis=0).astype(np.uint64)
        lvn = nxt(live)
        o[HS0], o[HS1], o[HCH], o[HMAJ], o[HLV] = s0, s1, c_, m, live
        for j in range(8):
            s = _U(IV[j]) + w[1 + j]
            o[HPZ + j], o[HCZ + j] = lvn * (s & _U(MASK)), s >> _U(32)
        t1 = nxt(s1) + nxt(c_) + nxt(w[W_]) + _U(K0) * lvn
        a_sum = np.where(chained, o[HPZ + 7], _U(IV[7]) * lvn) + t1 + nxt(s0) + nxt(m)
        e_sum = np.where(chained, o[HPZ + 3] + o[HPZ + 7], _U(IV[3] + IV[7]) * lvn) + t1
        ca, ce = (a_sum >> _U(32)) & _U(7), (e_sum >> _U(32)) & _U(7)
        for k in range(3):
            o[HCA + k], o[HCE + k] = ((ca >> _U(k)) & _U(1)) * bound, ((ce >> _U(k)) & _U(1)) * bound
    return out


# ---- the 337 constraints over an abstract field
def _constraints(f, t, tn, h, hn):
    """the 337 constraints of one proof WITHOUT their selectors: t[c], h[c] the table's and the helper's columns at x, tn, hn at omega x.
    Returns (the 321 unselected ones, the 8 linear forms of the start rows, the 8 of the chain rows)"""
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
    out += [boolean(h[HCZ + j]) for j in range(8)]
    out += [boolean(h[c]) for c in range(HCA, HCA + 6)]
    out.append(boolean(h[HLV]))
    for col, at in ((B_, HB), (C_, HC), (D_, HD), (F_, HF), (G_, HG), (H_, HH)):
        out.append(sub(t[col], word([h[at + i] for i in range(32)])))
    Bb, Cb, Db = (lambda i: h[HB + i % 32]), (lambda i: h[HC + i % 32]), (lambda i: h[HD + i % 32])
    Fb, Gb, Hb = (lambda i: h[HF + i % 32]), (lambda i: h[HG + i % 32]), (lambda i: h[HH + i % 32])
    out += [sub(h[HU0 + i], xor(Bb(i + 2), Bb(i + 13))) for i in range(32)]
    out += [sub(h[HU1 + i], xor(Fb(i + 6), Fb(i + 11))) for i in range(32)]
    out += [sub(h[HV + i], mul(Bb(i), Cb(i))) for i in range(32)]
    out.append(sub(h[HS0], word([xor(h[HU0 + i], Bb(i + 22)) for i in range(32)])))
    out.append(sub(h[HS1], word([xor(h[HU1 + i], Fb(i + 25)) for i in range(32)])))
    out.append(sub(h[HCH], word([add(Hb(i), mul(Fb(i), sub(Gb(i), Hb(i)))) for i in range(32)])))
    out.append(sub(h[HMAJ], word([add(h[HV + i], mul(Db(i), sub(add(Bb(i), Cb(i)), mul(two, h[HV + i])))) for i in range(32)])))
    lvn, c32 = hn[HLV], k(1 << 32)
    for j in range(8):
        out.append(sub(h[HPZ + j], mul(lvn, sub(add(k(IV[j]), t[1 + j]), mul(c32, h[HCZ + j])))))
    assert len(out) == JSTART
    carry = lambda at: mul(c32, add(h[at], add(mul(two, h[at + 1]), mul(k(4), h[at + 2]))))
    t1 = add(add(hn[HS1], hn[HCH]), tn[W_])  # (without the chaining words and K_0)
    t2 = add(hn[HS0], hn[HMAJ])
    lk = lambda c: mul(k(c), lvn)
    start = [sub(tn[x], lk(IV[j])) for x, j in SHIFTED]
    start.append(sub(add(tn[A_], carry(HCA)), add(lk(IV[7] + K0), add(t1, t2))))
    start.append(sub(add(tn[E_], carry(HCE)), add(lk(IV[3] + IV[7] + K0), t1)))
    chain = [sub(tn[x], h[HPZ + j]) for x, j in SHIFTED]
    chain.append(sub(add(tn[A_], carry(HCA)), add(add(h[HPZ + 7], lk(K0)), add(t1, t2))))
    chain.append(sub(add(tn[E_], carry(HCE)), add(add(h[HPZ + 3], h[HPZ + 7]), add(lk(K0), t1))))
    assert len(out) + len(start) + len(chain) == CONSTRAINTS
    return out, start, chain


def integer_residuals(table, help_, chain):
    """the 337 constraints of ONE proof as integer expressions (no reduction mod p) on pre-LDE rows, rows cyclic; the start ones are set to
    zero off the start rows, the chain ones off the chain rows.  Returns [337][R] Python integers as object arrays."""
    f = _Field()
    f.add, f.sub, f.mul, f.k = (lambda a, b: a + b), (lambda a, b: a - b), (lambda a, b: a * b), (lambda c: c)
    t = [np.array([int(x) for x in col], dtype=object) for col in np.asarray(table, dtype=np.uint64).reshape(WIDTH, -1)]
    h = [np.array([int(x) for x in col], dtype=object) for col in np.asarray(help_, dtype=np.uint64).reshape(HELPER_COLS, -1)]
    R = t[0].size
    es = np.array([1 if start_row(r, chain) else 0 for r in range(R)], dtype=object)
    ec = np.array([1 if chain_row(r, chain) else 0 for r in range(R)], dtype=object)
    plain, start, chained = _constraints(f, t, [np.roll(c, -1) for c in t], h, [np.roll(c, -1) for c in h])
    return plain + [es * c for c in start] + [ec * c for c in chained]


# ---- gamma, the tables on the coset, the quotient
def gamma(oracle, log_n, log_blowup, cap_height, n_proofs, chain, cap, cap_helper):
    """2^33, the set id 5 with the mode in bit 8, log_n, log_blowup, cap_height, n_proofs, the table cap, the helper cap; drawn again while
    gamma.c1 == 0"""
    chal = fm.Challenger(oracle)
    chal.observe(1 << 33)
    for v in (SET_ID | chain << 8, log_n, log_blowup, cap_height, n_proofs):
        chal.observe(v)
    for c in (cap, cap_helper):
        c = np.asarray(c, dtype=np.uint64).reshape(-1)
        assert c.size == 4 << min(cap_height, log_n)
        chal.observe_all(c)
    while True:
        g = chal.ext()
        if g[1]:
            return g


def rho(oracle, log_n):
    """omega_128^-1, omega_128 = omega_N^(N/128) = w^(M/128)"""
    return pow(pow(oracle.gl_root(log_n), 1 << (log_n - 7), P), P - 2, P)


def quotient(oracle, log_n, log_blowup, n_proofs, chain, cols, hcols, shift, g, ints=False):
    """cols [9 n_proofs][M], hcols [315 n_proofs][M] words on the coset shift <gl_root(log_n)>; the planar quotient (2 M canonical words):
    the unselected constraints over x^N - 1, the start forms over D_s, the chain forms over D_c.
    ints: with Python integers in object arrays instead of the uint64 field (slow; the cross-check of the two)"""
    M, B = 1 << log_n, 1 << log_blowup
    N = M // B
    assert chain in (0, 1) and N >= (128 if chain else 64)
    cols = np.asarray(cols, dtype=np.uint64).reshape(n_proofs * WIDTH, M)
    hcols = np.asarray(hcols, dtype=np.uint64).reshape(n_proofs * HELPER_COLS, M)
    w = oracle.gl_root(log_n)
    xs = [shift % P]
    for _ in range(M - 1):
        xs.append(xs[-1] * w % P)
    inv = lambda v: pow(v % P, P - 2, P)
    dt = object if ints else np.uint64
    zinv = np.array([inv(pow(x, N, P) - 1) for x in xs[:B]] * (M // B), dtype=dt)
    if chain:
        period, ro = min(M, 128 * B), rho(oracle, log_n)
        zs = [pow(x, N // 128, P) for x in xs[:period]]
        dsinv = np.array([inv(z - ro) for z in zs] * (M // period), dtype=dt)
        dcinv = np.array([inv(z + ro) for z in zs] * (M // period), dtype=dt)
    else:
        period, om_inv = min(M, 64 * B), pow(omega_64(oracle, log_n), P - 2, P)
        dsinv = np.array([inv(pow(x, N // 64, P) - om_inv) for x in xs[:period]] * (M // period), dtype=dt)
        dcinv = np.zeros(M, dtype=dt)  # E_c = 0
    f = _base() if ints else _vec()
    canon = _obj if ints else (lambda v: np.asarray(v, dtype=np.uint64) % _U(P))
    zero = lambda: np.zeros(M, dtype=dt)
    acc = [[zero(), zero()] for _ in range(3)]  # the gamma sums of the unselected, the start and the chain part
    gp = (1, 0)
    with np.errstate(over="ignore"):
        for p in range(n_proofs):
            t = [canon(c) for c in cols[p * WIDTH:(p + 1) * WIDTH]]
            h = [canon(c) for c in hcols[p * HELPER_COLS:(p + 1) * HELPER_COLS]]
            for part, terms in zip(acc, _constraints(f, t, [np.roll(c, -B) for c in t], h, [np.roll(c, -B) for c in h])):
                for term in terms:
                    if ints:
                        term = term % P
                        part[0], part[1] = part[0] + gp[0] * term, part[1] + gp[1] * term
                    else:
                        part[0], part[1] = _addv(part[0], _mulv(term, _U(gp[0]))), _addv(part[1], _mulv(term, _U(gp[1])))
                    gp = e_mul(gp, g)
        q = []
        for k in (0, 1):
            if ints:
                q.append((acc[0][k] % P * zinv + acc[1][k] % P * dsinv + acc[2][k] % P * dcinv) % P)
            else:
                q.append(_addv(_addv(_mulv(acc[0][k], zinv), _mulv(acc[1][k], dsinv)), _mulv(acc[2][k], dcinv)))
    return np.array([int(x) for x in q[0]] + [int(x) for x in q[1]], dtype=np.uint64)


# ---- the identity at zeta
def constraint_sums(n_proofs, t0, t1, h0, h1, g):
    """the three sums of gamma^(337 p + j) C_(p,j) over F_p^2 (unselected, start, chain) from the openings at zeta (t0, h0) and zeta omega_N
    (t1, h1)"""
    f = _ext()
    acc, gp = [(0, 0)] * 3, (1, 0)
    for p in range(n_proofs):
        a, b = p * WIDTH, p * HELPER_COLS
        parts = _constraints(f, t0[a:a + WIDTH], t1[a:a + WIDTH], h0[b:b + HELPER_COLS], h1[b:b + HELPER_COLS])
        for k, terms in enumerate(parts):
            for term in terms:
                acc[k] = e_add(acc[k], e_mul(gp, term))
                gp = e_mul(gp, g)
    return acc


def identity_at(oracle, log_n, log_blowup, n_proofs, chain, t0, t1, h0, h1, u0, u1, zeta, g):
    """division-free: S sum_unselected + (zeta^N - 1) (D_c sum_start + D_s sum_chain) == (u_0 + X u_1) (zeta^N - 1) S with S = D_s D_c under
    chain = 1; S sum_unselected + (zeta^N - 1) sum_start == (u_0 + X u_1) (zeta^N - 1) S under chain = 0; X (a, b) = (7 b, a)"""
    N = 1 << (log_n - log_blowup)
    zn = dm.e_pow(zeta, N)
    zn1 = ((zn[0] - 1) % P, zn[1])
    q = ((u0[0] + 7 * u1[1]) % P, (u0[1] + u1[0]) % P)
    plain, start, chained = constraint_sums(n_proofs, t0, t1, h0, h1, g)
    if chain:
        z, ro = dm.e_pow(zeta, N // 128), rho(oracle, log_n)
        ds, dc = ((z[0] - ro) % P, z[1]), ((z[0] + ro) % P, z[1])
        S = e_mul(ds, dc)
        sel = e_add(e_mul(dc, start), e_mul(ds, chained))
    else:
        y = dm.e_pow(zeta, N // 64)
        S = ((y[0] - pow(omega_64(oracle, log_n), P - 2, P)) % P, y[1])
        sel = start
    return e_add(e_mul(S, plain), e_mul(zn1, sel)) == e_mul(e_mul(q, zn1), S)


def identity(oracle, p, k_trace, k_helper, chain, caps, proof):
    """the identity from the openings blocks of oracle k_trace (the table), k_helper (the helper) and k_helper + 1 (the quotient)"""
    caps = am._caps_list(p, caps)
    log_n, n_cols = p["log_n"][k_trace], p["n_cols"][k_trace]
    assert n_cols % WIDTH == 0 and k_helper > k_trace
    n_proofs = n_cols // WIDTH
    assert p["log_n"][k_helper] == log_n and p["n_cols"][k_helper] == HELPER_COLS * n_proofs
    assert p["log_n"][k_helper + 1] == log_n and p["n_cols"][k_helper + 1] == 2
    _, zeta = bm._start(oracle, p, caps)
    g = gamma(oracle, log_n, p["log_blowup"], p["cap_height"], n_proofs, chain, caps[k_trace], caps[k_helper])
    yt, yh, yq = (bm.openings_of(p, proof, k) for k in (k_trace, k_helper, k_helper + 1))
    return identity_at(oracle, log_n, p["log_blowup"], n_proofs, chain, [y[0] for y in yt], [y[1] for y in yt], [y[0] for y in yh],
                       [y[1] for y in yh], yq[0][0], yq[1][0], zeta, g)


def verify(oracle, p, k_trace, k_helper, chain, caps, proof, shift):
    """[ok] per query: batch_model.verify and the identity (a failed identity rejects every query)"""
    holds = identity(oracle, p, k_trace, k_helper, chain, caps, proof)
    return [bool(ok and holds) for ok in bm.verify(oracle, p, caps, proof, shift)]
