"""A pure-Python model of the public side of constraint set 6 of the SHA-256 tables (include/tmx.h "the SHA-256 tables' link to Level-1"),
written from the header text and independent of libtmx: the public table of T.3, T.5 and T.6 gathered from Level-1 ELEMENT rows
(docs/witness_layout.md: H and D; bytes are eight big-endian bit elements), the 33-column helper oracle, the 50 constraints as integer identities
on the rows and over an abstract field, the public digest, gamma, the seventeen public polynomials, the quotient point by point and in
pieces, the identity at zeta and `verify` = tests/batch_model.py's verifier and that identity.  Built on tests/batch_model.py and on the
helpers of tests/air_boundary_model.py's kind.  The yardstick of tests/test_sha_public.py (not collected by pytest).  Parity unpinned
against plonky2."""
import numpy as np

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha_air_model as sm
from fri_model import P, e_add, e_mul, e_sub
from sha_air_model import WIDTH

SHA256, TREE, HEADER = 4, 16, 32
PUB_WIDTH, HELPER_COLS, CONSTRAINTS, SET_ID = 26, 33, 50, 6
PW_W, PW_DIG, PW_NEW, PW_CHN = 0, 16, 24, 25  # columns inside a proof's 26
HCV, HDG, HCD, HCH, HCHN = 0, 8, 16, 24, 32  # helper columns inside a proof's 33
MASK = 0xFFFFFFFF
IV = [0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19]


# ---- the element rows
def tree_slots(n):
    """slots of the fixed-shape validator tree, every level (promoted odd nodes included)"""
    c = 0
    while n > 1:
        n = (n + 1) // 2
        c += n
    return c


class Layout:
    """first elements of the sections of an element row that the gather reads (docs/witness_layout.md)"""

    def __init__(self, kind, n):
        skip = kind == 0
        self.kind, self.n, self.tn = kind, n, tree_slots(n)
        self.h2 = 256  # ValidatorVariable[N], 1517 each: validator_byte_length at 1515
        self.h3 = 256 + 1517 * n  # nb, round, then the proof structs
        self.aunts = [self.h3 + 3, self.h3 + 1444, self.h3 + 2471, self.h3 + (3768 if skip else 3767)] + ([] if skip else [self.h3 + 5367])
        self.cid_len, self.cid = self.h3 + 1027, self.h3 + 1028
        self.h_len = self.h3 + 2468
        self.leaf = [None, None, self.h3 + 3495, self.h3 + (4792 if skip else 4791)] + ([] if skip else [self.h3 + 6391])
        self.leaf_bytes = [52, 11, 34, 34 if skip else 72] + ([] if skip else [34])
        self.h4 = self.h3 + 5064  # skip: ValidatorHashFieldVariable[N], 259 each: validator_byte_length at 258
        self.d = 1776 * n + 5320 if skip else 1517 * n + 6919
        self.d1a = self.d  # 1136 per lane: marshalled 368, leaf hash 256
        self.d2a = self.d + 1235 * n  # skip, 624 per lane
        self.d3 = self.d + (1865 if skip else 1235) * n
        self.d4 = self.d3 + 256 * self.tn
        self.d5 = self.d3 + (2 if skip else 1) * 256 * self.tn
        self.d5_proof = [self.d5, self.d5 + 1368, self.d5 + 2648, self.d5 + 3928] + ([] if skip else [self.d5 + 5208])
        self.d5_hleaf = self.d5 + 1280


PATH_INDEX = {0: [1, 2, 7, 7], 1: [1, 2, 7, 4, 8]}  # leaf index of each header proof: path bits LSB-first


def _byte(row, at):
    v = 0
    for b in range(8):
        v = (v << 1) | (int(row[at + b]) & 1)
    return v


def _bytes(row, at, count):
    return [_byte(row, at + 8 * k) for k in range(count)]


def _blocks(msg, length):
    """the SHA padding of msg[:length] (length <= 119): one or two blocks of sixteen big-endian words"""
    m = list(msg[:length]) + [0x80]
    n_blocks = 2 if length + 9 > 64 else 1
    m += [0] * (64 * n_blocks - 4 - len(m)) + list((8 * length).to_bytes(4, "big"))
    return [[int.from_bytes(bytes(m[64 * b + 4 * t:64 * b + 4 * t + 4]), "big") for t in range(16)] for b in range(n_blocks)]


def _words(row, at):
    """a 32-byte digest as eight big-endian words"""
    return [int.from_bytes(bytes(_bytes(row, at + 32 * j, 4)), "big") for j in range(8)]


def section_hashes(kind, n, section, row):
    """[(message bytes or None, digest words)] of the section's hashes in table order, from one element row; None is a zero hash.  Also
    whether a hash owns two blocks of the table"""
    L = Layout(kind, n)
    sets = 2 if kind == 0 else 1
    out = []
    if section == SHA256:
        for s in range(sets):
            for i in range(n):
                lane = (L.d2a + 624 * i) if s else (L.d1a + 1136 * i)
                vlen = min(int(row[L.h4 + 259 * i + 258] if s else row[L.h2 + 1517 * i + 1515]), 46)
                out.append(([0] + _bytes(row, lane, vlen), _words(row, lane + 368)))
        return out, 1
    if section == TREE:
        for s in range(sets):
            nodes = L.d4 if s else L.d3
            sz, first, prev_first, level = n, 0, 0, 0
            while sz > 1:
                nx = (sz + 1) // 2
                for rem in range(nx):
                    if 2 * rem + 1 >= sz:  # the promoted odd node: no hash
                        out.append((None, None))
                        continue
                    if level == 0:
                        step = 624 if s else 1136
                        l = (L.d2a if s else L.d1a) + step * 2 * rem + 368
                    else:
                        step = 256
                        l = nodes + 256 * (prev_first + 2 * rem)
                    out.append(([1] + _bytes(row, l, 32) + _bytes(row, l + step, 32), _words(row, nodes + 256 * (first + rem))))
                prev_first, first, sz, level = first, first + nx, nx, level + 1
        return out, 2
    assert section == HEADER
    for q in range(4 if kind == 0 else 5):
        if q == 0:
            msg, length = [0] + _bytes(row, L.cid, 52) + [0] * 27, min(int(row[L.cid_len]), 79) + 1
        elif q == 1:
            msg, length = _bytes(row, L.d5_hleaf, 11) + [0] * 69, min(int(row[L.h_len]), 79) + 1
        else:
            msg, length = [0] + _bytes(row, L.leaf[q], L.leaf_bytes[q]), L.leaf_bytes[q] + 1
        out.append((msg[:length], _words(row, L.d5_proof[q])))
        for k in range(4):
            cur, aunt = _bytes(row, L.d5_proof[q] + 256 * k, 32), _bytes(row, L.aunts[q] + 256 * k, 32)
            right = (PATH_INDEX[kind][q] >> k) & 1  # the running hash is the right child
            out.append(([1] + (aunt + cur if right else cur + aunt), _words(row, L.d5_proof[q] + 256 * (k + 1))))
    return out, 2


def public_table(kind, n, section, rows, log_k):
    """rows: one element row per proof.  [26 n_proofs][K] words: per block the sixteen message words, the digest on the last live block of
    a hash, new and chn.  Blocks behind the section's own are padding: all zero"""
    K = 1 << log_k
    pub = np.zeros((PUB_WIDTH * len(rows), K), dtype=np.uint64)
    for p, row in enumerate(rows):
        hashes, per = section_hashes(kind, n, section, row)
        assert per * len(hashes) <= K
        o = PUB_WIDTH * p
        for i, (msg, dig) in enumerate(hashes):
            if msg is None:
                continue
            blocks = _blocks(msg, len(msg))
            assert len(blocks) <= per
            for b, words in enumerate(blocks):
                k = per * i + b
                pub[o + PW_W:o + PW_W + 16, k] = words
                pub[o + (PW_CHN if b else PW_NEW), k] = 1
            pub[o + PW_DIG:o + PW_DIG + 8, per * i + len(blocks) - 1] = dig
    return pub


def messages(kind, n, section, row):
    """the reassembled message bytes of every hash of the section (None: a zero hash), for hashlib"""
    return [None if m is None else bytes(m) for m, _ in section_hashes(kind, n, section, row)[0]]


# ---- the helper oracle
def _flag(word):
    return 1 if int(word) & MASK else 0


def helper(table, pub, n_proofs):
    """table: [9 n_proofs][R] pre-LDE words, pub: [26 n_proofs][R / 64].  [33 n_proofs][R] words; operands are the low 32 bits, a flag is set
    when its low 32 bits are not zero (new before chn)"""
    table, pub = np.asarray(table, dtype=np.uint64), np.asarray(pub, dtype=np.uint64)
    R = table.shape[1]
    K = R // 64
    assert table.shape[0] == n_proofs * WIDTH and pub.shape == (n_proofs * PUB_WIDTH, K)
    out = np.zeros((n_proofs * HELPER_COLS, R), dtype=np.uint64)
    for p in range(n_proofs):
        t, o = table[p * WIDTH:(p + 1) * WIDTH], p * HELPER_COLS
        for k in range(K):
            new, chn = _flag(pub[p * PUB_WIDTH + PW_NEW, k]), _flag(pub[p * PUB_WIDTH + PW_CHN, k])
            chn_next = _flag(pub[p * PUB_WIDTH + PW_CHN, (k + 1) % K])
            prev = (64 * k - 1) % R
            for j in range(8):
                cv = IV[j] if new else ((IV[j] + (int(t[1 + j, prev]) & MASK)) & MASK if chn else 0)
                s = (t[1 + j, 64 * k:64 * k + 64] & np.uint64(MASK)) + np.uint64(cv)
                out[o + HCV + j, 64 * k:64 * k + 64] = cv
                out[o + HDG + j, 64 * k:64 * k + 64] = s & np.uint64(MASK)
                out[o + HCD + j, 64 * k:64 * k + 64] = s >> np.uint64(32)
                if chn_next:
                    out[o + HCH + j, 64 * k:64 * k + 64] = s & np.uint64(MASK)
            out[o + HCHN, 64 * k:64 * k + 64] = chn_next
    return out


def integer_residuals(table, help_, pub):
    """ONE proof: the 50 constraints as integer arrays over the rows (no reduction mod p), rows cyclic; the selected ones are zero off
    their rows by construction (the selector written as a 0 / 1 mask), 24 .. 31 on every row but the last of a block.  Constraint 49 is
    returned as its sixteen parts"""
    t = [[int(x) for x in c] for c in np.asarray(table, dtype=np.uint64)]
    h = [[int(x) for x in c] for c in np.asarray(help_, dtype=np.uint64)]
    pub = np.asarray(pub, dtype=np.uint64)
    R = len(t[0])
    K = R // 64
    assert pub.shape == (PUB_WIDTH, K)
    rows = range(R)
    nxt = lambda c: c[1:] + c[:1]
    last = [1 if r % 64 == 63 else 0 for r in rows]
    blk = [r // 64 for r in rows]
    pw = lambda col, shift: [int(pub[col, (blk[r] + shift) % K]) for r in rows]
    new_next, chn_next = pw(PW_NEW, 1), pw(PW_CHN, 1)
    res = []
    res += [[h[HCD + j][r] ** 2 - h[HCD + j][r] for r in rows] for j in range(8)]
    res += [[h[HDG + j][r] + (h[HCD + j][r] << 32) - h[HCV + j][r] - t[1 + j][r] for r in rows] for j in range(8)]
    res += [[h[HCH + j][r] - h[HCHN][r] * h[HDG + j][r] for r in rows] for j in range(8)]
    cvn = [nxt(h[HCV + j]) for j in range(8)]  # (shifted once per column, not once per row: 2^15 rows take seconds, not minutes)
    res += [[(1 - last[r]) * (cvn[j][r] - h[HCV + j][r]) for r in rows] for j in range(8)]
    res += [[last[r] * (cvn[j][r] - h[HCH + j][r] - IV[j] * new_next[r]) for r in rows] for j in range(8)]
    res += [[last[r] * (h[HDG + j][r] - h[HCH + j][r] - int(pub[PW_DIG + j, blk[r]])) for r in rows] for j in range(8)]
    res += [[last[r] * (h[HCHN][r] - chn_next[r]) for r in rows]]
    res += [[(t[0][r] - int(pub[PW_W + tt, blk[r]])) if r % 64 == tt else 0 for r in rows] for tt in range(16)]
    return [np.array(c, dtype=object) for c in res]


# ---- the 50 constraints over an abstract field (sha_air_model's field policies), their column parts
def _constraints(f, t, tn, h, hn, S):
    """(the 32 unselected constraints -- 24 .. 31 carry the factor S --, the column parts of the 17 constraints selected by T, W): what
    the public polynomials are subtracted from is left to the caller"""
    c32 = f.k(1 << 32)
    plain = [f.sub(f.mul(h[HCD + j], h[HCD + j]), h[HCD + j]) for j in range(8)]
    plain += [f.sub(f.add(h[HDG + j], f.mul(c32, h[HCD + j])), f.add(h[HCV + j], t[1 + j])) for j in range(8)]
    plain += [f.sub(h[HCH + j], f.mul(h[HCHN], h[HDG + j])) for j in range(8)]
    plain += [f.mul(S, f.sub(hn[HCV + j], h[HCV + j])) for j in range(8)]
    sel = [f.sub(hn[HCV + j], h[HCH + j]) for j in range(8)]
    sel += [f.sub(h[HDG + j], h[HCH + j]) for j in range(8)]
    sel.append(h[HCHN])
    return plain, sel, t[0]


# ---- gamma and the public side
def digest(oracle, pub):
    """the Poseidon Merkle root (cap height 0) of pub as a column-major oracle of log2 K rows"""
    pub = np.asarray(pub, dtype=np.uint64)
    log_k = pub.shape[1].bit_length() - 1
    return oracle.poseidon_merkle(np.ascontiguousarray(pub).reshape(-1), log_k, pub.shape[0], 0)[-1].reshape(-1)


def gamma(oracle, log_n, log_blowup, cap_height, n_proofs, cap, cap_helper, pub):
    """2^33, the set id 6, log_n, log_blowup, cap_height, n_proofs, the table cap, the helper cap, the public digest; drawn again while
    gamma.c1 == 0"""
    chal = fm.Challenger(oracle)
    chal.observe(1 << 33)
    for v in (SET_ID, log_n, log_blowup, cap_height, n_proofs):
        chal.observe(v)
    for c in (cap, cap_helper):
        c = np.asarray(c, dtype=np.uint64).reshape(-1)
        assert c.size == 4 << min(cap_height, log_n)
        chal.observe_all(c)
    d = digest(oracle, pub)
    assert d.size == 4
    chal.observe_all(d)
    while True:
        g = chal.ext()
        if g[1]:
            return g


def combine(pub, g):
    """the seventeen value vectors under gamma: [V63, V^0 .. V^15], each K elements of F_p^2.
    V63_k = sum_p [sum_j gamma^(50 p + 32 + j) IV_j new_p[(k + 1) % K] + sum_j gamma^(50 p + 40 + j) dig_p[k][j] + gamma^(50 p + 48) chn_p[(k + 1) % K]],
    V^t_k = sum_p gamma^(50 p + 49) w_p[k][t]"""
    pub = np.asarray(pub, dtype=np.uint64)
    n_proofs, K = pub.shape[0] // PUB_WIDTH, pub.shape[1]
    V = [[(0, 0)] * K for _ in range(17)]
    for p in range(n_proofs):
        o = PUB_WIDTH * p
        gw = [dm.e_pow(g, CONSTRAINTS * p + j) for j in range(CONSTRAINTS)]
        g_new = (0, 0)
        for j in range(8):
            g_new = e_add(g_new, fm.e_scale(gw[32 + j], IV[j]))
        for k in range(K):
            v = e_add(fm.e_scale(g_new, int(pub[o + PW_NEW, (k + 1) % K]) % P), fm.e_scale(gw[48], int(pub[o + PW_CHN, (k + 1) % K]) % P))
            for j in range(8):
                v = e_add(v, fm.e_scale(gw[40 + j], int(pub[o + PW_DIG + j, k]) % P))
            V[0][k] = e_add(V[0][k], v)
            for t in range(16):
                V[1 + t][k] = e_add(V[1 + t][k], fm.e_scale(gw[49], int(pub[o + PW_W + t, k]) % P))
    return V


OFFSETS = [63] + list(range(16))  # the row inside a block of each of the seventeen cosets


def omega(oracle, log_n, log_blowup):
    return pow(oracle.gl_root(log_n), 1 << log_blowup, P)


def coefficients(oracle, log_n, log_blowup, V, off):
    """the two planes' coefficients of the polynomial of degree < K through V_k at omega^(64 k + off): V_k = sum_j (c_j omega^(off j))
    omega_K^(j k), so c_j = d_j omega^(-off j) with d the inverse transform of V on the K-subgroup"""
    K = len(V)
    om = omega(oracle, log_n, log_blowup)
    assert oracle.gl_root(K.bit_length() - 1) == pow(om, 64, P)  # omega_K = omega^64: the CPU transform's root of that size
    f = pow(pow(om, off, P), P - 2, P)
    out = []
    for plane in (0, 1):
        d = oracle.ntt(np.array([v[plane] for v in V], dtype=np.uint64), inverse=True)
        c, fk = [], 1
        for x in d:
            c.append(int(x) * fk % P)
            fk = fk * f % P
        out.append(c)
    return out


def _on_coset(oracle, log_n, coefs, shift):
    M = 1 << log_n
    out = []
    for c in coefs:
        a, sk = np.zeros(M, dtype=np.uint64), 1
        for j, x in enumerate(c):
            a[j] = x * sk % P
            sk = sk * (shift % P) % P
        out.append(oracle.ntt(a))
    return out


def _obj(v):
    return np.array([int(x) % P for x in np.asarray(v, dtype=np.uint64).reshape(-1)], dtype=object)


def _divisors(oracle, log_n, log_blowup, shift):
    """(1 / (x^N - 1), S, 1 / S, [1 / D_t]) on the coset as object arrays; S = x^K - omega_64^-1, D_t = x^K - omega_64^t (period 64 B)"""
    M, B = 1 << log_n, 1 << log_blowup
    N = M // B
    K = N // 64
    w = oracle.gl_root(log_n)
    xs = [shift % P]
    for _ in range(M - 1):
        xs.append(xs[-1] * w % P)
    inv = lambda v: pow(v % P, P - 2, P)
    om64 = pow(omega(oracle, log_n, log_blowup), K, P)
    period = 64 * B
    zk = [pow(x, K, P) for x in xs[:period]]
    rep = lambda v: np.array(v * (M // len(v)), dtype=object)
    zinv = rep([inv(pow(x, N, P) - 1) for x in xs[:B]])
    S = rep([(z - pow(om64, 63, P)) % P for z in zk])
    sinv = rep([inv(z - pow(om64, 63, P)) for z in zk])
    dinv = [rep([inv(z - pow(om64, t, P)) for z in zk]) for t in range(16)]
    return zinv, S, sinv, dinv


def public_quotient(oracle, log_n, log_blowup, pub, shift, g):
    """PQ(x_i) = P63(x_i) / S(x_i) + sum_t P_t(x_i) / D_t(x_i) on the coset: the two planes as object arrays"""
    _, _, sinv, dinv = _divisors(oracle, log_n, log_blowup, shift)
    V = combine(pub, g)
    pq = [np.zeros(1 << log_n, dtype=object) for _ in (0, 1)]
    for v, off, d in zip(V, OFFSETS, [sinv] + dinv):
        ext = _on_coset(oracle, log_n, coefficients(oracle, log_n, log_blowup, v, off), shift)
        for k in (0, 1):
            pq[k] = (pq[k] + _obj(ext[k]) * d) % P
    return pq


def quotient(oracle, log_n, log_blowup, n_proofs, cols, hcols, pub, shift, g, proofs=None, ints=False):
    """cols [9 n_proofs][M], hcols [33 n_proofs][M] words on the coset shift <gl_root(log_n)>, pub [26 n_proofs][K]; the planar quotient
    (2 M canonical words): the unselected constraints over x^N - 1, the column parts of 32 .. 48 over S, W times sum_t 1 / D_t, less PQ.
    proofs: a range of proof indices (the piece form; the piece that holds proof 0 carries - PQ).  ints: the constraint sums with Python
    integers in object arrays instead of the uint64 field (the cross-check of the two)"""
    M, B = 1 << log_n, 1 << log_blowup
    K = M // B // 64
    assert 2 <= K <= 4096
    cols = np.asarray(cols, dtype=np.uint64).reshape(n_proofs * WIDTH, M)
    hcols = np.asarray(hcols, dtype=np.uint64).reshape(n_proofs * HELPER_COLS, M)
    zinv, S, sinv, dinv = _divisors(oracle, log_n, log_blowup, shift)
    dsum = sum(dinv) % P
    f = sm._base() if ints else sm._vec()
    canon = _obj if ints else (lambda v: np.asarray(v, dtype=np.uint64) % sm._U(P))
    Sf = S if ints else S.astype(np.uint64)
    acc = [[np.zeros(M, dtype=object), np.zeros(M, dtype=object)] for _ in range(3)]
    rng = range(n_proofs) if proofs is None else proofs
    with np.errstate(over="ignore"):
        for p in rng:
            gp = dm.e_pow(g, CONSTRAINTS * p)
            t = [canon(c) for c in cols[p * WIDTH:(p + 1) * WIDTH]]
            h = [canon(c) for c in hcols[p * HELPER_COLS:(p + 1) * HELPER_COLS]]
            plain, sel, wcol = _constraints(f, t, [np.roll(c, -B) for c in t], h, [np.roll(c, -B) for c in h], Sf)
            for part, terms in zip(acc, (plain, sel, [wcol])):
                for term in terms:
                    term = _obj_any(term)
                    part[0], part[1] = (part[0] + gp[0] * term) % P, (part[1] + gp[1] * term) % P
                    gp = e_mul(gp, g)
    q = [(acc[0][k] * zinv + acc[1][k] * sinv + acc[2][k] * dsum) % P for k in (0, 1)]
    if 0 in rng:
        pq = public_quotient(oracle, log_n, log_blowup, pub, shift, g)
        q = [(q[k] - pq[k]) % P for k in (0, 1)]
    return np.array([int(x) for x in q[0]] + [int(x) for x in q[1]], dtype=np.uint64)


def _obj_any(v):
    return np.array([int(x) % P for x in v], dtype=object)


# ---- the identity at zeta
def public_at(oracle, log_n, log_blowup, pub, g, zeta):
    """PQ(zeta) = sum over the seventeen cosets of 1 / (K y_0^K) sum_k V_k y_k / (zeta - y_k), or None on a zero denominator"""
    K = np.asarray(pub).shape[1]
    om = omega(oracle, log_n, log_blowup)
    total = (0, 0)
    for v, off in zip(combine(pub, g), OFFSETS):
        y0 = pow(om, off, P)
        acc = (0, 0)
        for k in range(K):
            y = y0 * pow(om, 64 * k, P) % P
            d = ((zeta[0] - y) % P, zeta[1])
            if d == (0, 0):
                return None
            acc = e_add(acc, e_mul(fm.e_scale(v[k], y), dm.e_inv(d)))
        total = e_add(total, fm.e_scale(acc, pow(K * pow(y0, K, P) % P, P - 2, P)))
    return total


def identity_at(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, u0, u1, zeta, g, pub):
    """sum_unselected + (zeta^N - 1) (sum_selected / S + sum_W sum_t 1 / D_t - PQ(zeta)) == (u_0 + X u_1) (zeta^N - 1); a zero denominator
    fails it; X (a, b) = (7 b, a)"""
    N = 1 << (log_n - log_blowup)
    K = N // 64
    om64 = pow(omega(oracle, log_n, log_blowup), K, P)
    zk, zn = dm.e_pow(zeta, K), dm.e_pow(zeta, N)
    Z = ((zn[0] - 1) % P, zn[1])
    S = ((zk[0] - pow(om64, 63, P)) % P, zk[1])
    D = [((zk[0] - pow(om64, t, P)) % P, zk[1]) for t in range(16)]
    pq = public_at(oracle, log_n, log_blowup, pub, g, zeta)
    if pq is None or S == (0, 0) or (0, 0) in D:
        return False
    f = sm._ext()
    acc, gp = [(0, 0)] * 3, None
    for p in range(n_proofs):
        a, b = p * WIDTH, p * HELPER_COLS
        gp = dm.e_pow(g, CONSTRAINTS * p)
        parts = _constraints(f, t0[a:a + WIDTH], t1[a:a + WIDTH], h0[b:b + HELPER_COLS], h1[b:b + HELPER_COLS], S)
        for k, terms in enumerate((parts[0], parts[1], [parts[2]])):
            for term in terms:
                acc[k] = e_add(acc[k], e_mul(gp, term))
                gp = e_mul(gp, g)
    dsum = (0, 0)
    for d in D:
        dsum = e_add(dsum, dm.e_inv(d))
    inner = e_sub(e_add(e_mul(acc[1], dm.e_inv(S)), e_mul(acc[2], dsum)), pq)
    q = ((u0[0] + 7 * u1[1]) % P, (u0[1] + u1[0]) % P)
    return e_add(acc[0], e_mul(Z, inner)) == e_mul(q, Z)


def identity(oracle, p, k_trace, k_helper, caps, proof, pub):
    """the identity from the openings blocks of oracle k_trace (the table), k_helper (the helper) and k_helper + 1 (the quotient)"""
    caps = am._caps_list(p, caps)
    log_n, n_cols = p["log_n"][k_trace], p["n_cols"][k_trace]
    assert n_cols % WIDTH == 0 and k_helper > k_trace
    n_proofs = n_cols // WIDTH
    assert p["log_n"][k_helper] == log_n and p["n_cols"][k_helper] == HELPER_COLS * n_proofs
    assert p["log_n"][k_helper + 1] == log_n and p["n_cols"][k_helper + 1] == 2
    _, zeta = bm._start(oracle, p, caps)
    g = gamma(oracle, log_n, p["log_blowup"], p["cap_height"], n_proofs, caps[k_trace], caps[k_helper], pub)
    yt, yh, yq = (bm.openings_of(p, proof, k) for k in (k_trace, k_helper, k_helper + 1))
    return identity_at(oracle, log_n, p["log_blowup"], n_proofs, [y[0] for y in yt], [y[1] for y in yt], [y[0] for y in yh],
                       [y[1] for y in yh], yq[0][0], yq[1][0], zeta, g, pub)


def verify(oracle, p, k_trace, k_helper, caps, proof, shift, pub):
    """[ok] per query: batch_model.verify and the identity (a failed identity rejects every query)"""
    holds = identity(oracle, p, k_trace, k_helper, caps, proof, pub)
    return [bool(ok and holds) for ok in bm.verify(oracle, p, caps, proof, shift)]
