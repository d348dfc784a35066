"""A pure-Python model of the SHA-512 table's block-start constraints (include/tmx.h "the block starts of the SHA-512 table", constraint
set 9), written from the header text and independent of libtmx: the two preprocessed columns STA and CHN of full degree, the helper oracle
of 629 columns (the bits of b, c, d, f, g, h, the xor and and rows, the four round words as limbs, LV, the chaining words PZ with their
carry bits, the carries of the two round-0 sums), gamma from a fresh duplex over the table cap and the helper cap, the quotient point by
point over the extended columns, the identity at zeta from a batch proof's openings, and `verify` = tests/batch_model.py's verifier and
that identity, with the helper's oracle index explicit.  A sibling of tests/sha_init_model.py on 64-bit words in lo / hi limbs; it reuses
the field helpers of tests/sha_air_model.py and `barycentric` of tests/sha512_air_model.py; the 673 constraints are written ONCE
(`_constraints`) over an abstract field.  The yardstick of tests/test_sha512_init.py (not collected by pytest).  Parity unpinned against
plonky2, like the feature."""
import numpy as np

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha512_air_model as s7
import sha_air_model as sm
from fri_model import P, e_add, e_mul

WIDTH, HELPER_COLS, CONSTRAINTS = 18, 629, 673
SET_ID = 9
BLOCK, LANE = 80, 160
W_, A_, B_, C_, D_, E_, F_, G_, H_ = range(0, 18, 2)  # the table's columns inside a proof: the low limb; the high limb is the next one
HB, HC, HD, HF, HG, HH, HU0, HU1, HV = range(0, 576, 64)  # the helper's bit groups
HS0, HS1, HCH, HMAJ, HLV, HPZ, HCZ, HCAL, HCAH, HCEL, HCEH = 576, 578, 580, 582, 584, 585, 601, 617, 620, 623, 626  # PZ_j, CZ_j at + 2 j + limb
JCZ, JCARRY, JLV, JWORD, JU0, JU1, JV, JS0, JS1, JCH, JMAJ, JPZ, JSTART, JCHAIN = 384, 400, 412, 413, 425, 489, 553, 617, 619, 621, 623, 625, 641, 657
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1
IV512 = [0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1, 0x510e527fade682d1, 0x9b05688c2b3e6c1f,
         0x1f83d9abfb41bd6b, 0x5be0cd19137e2179]
K0 = 0x428a2f98d728ae22
_U = np.uint64


def limb(x, l):
    return (x >> 32) & M32 if l else x & M32


def round0(start, w0):
    """the state after round 0 (row 0 of a block) from the eight words the block starts from"""
    return s7.sha_round(list(start), w0, 0)


# ---- the preprocessed columns
def periodic(N, wrap=True):
    """[2][N]: STA (1 where the next row is row 0 of a first block: r mod 160 = 159, and the wrap row N - 1, switched ON explicitly), CHN
    (1 where r mod 160 = 79).  wrap = False: STA without the wrap row, the column a test shows to be wrong"""
    assert (N - 1) % LANE in (127, 95, 31, 63)
    r = np.arange(N)
    sta = (r % LANE == LANE - 1) | ((r == N - 1) & wrap)
    return np.stack([sta.astype(np.uint64), (r % LANE == BLOCK - 1).astype(np.uint64)])


# ---- the helper oracle
def helper(table, n_proofs):
    """table: [18 n_proofs][N] words (pre-LDE, any 64-bit words: the operands are their low 32 bits); the helper [629 n_proofs][N].  Rows
    are cyclic inside one proof.  Vectorised over the rows with numpy uint64 (every limb sum stays below 2^35)."""
    table = np.asarray(table, dtype=np.uint64).reshape(n_proofs * WIDTH, -1)
    N = table.shape[1]
    out = np.zeros((n_proofs * HELPER_COLS, N), dtype=np.uint64)
    bit = lambda x, i: (x >> _U(i % 64)) & _U(1)
    rot = lambda x, n: (x >> _U(n)) | (x << _U(64 - n))
    lo, hi = (lambda x: x & _U(M32)), (lambda x: x >> _U(32))
    nxt = lambda x: np.roll(x, -1)
    r = np.arange(N)
    sta, chn = periodic(N)
    edge = sta | chn
    for p in range(n_proofs):
        lim = table[p * WIDTH:(p + 1) * WIDTH] & _U(M32)
        word = lambda c: lim[c] | (lim[c + 1] << _U(32))
        o = out[p * HELPER_COLS:(p + 1) * HELPER_COLS]
        b, c, d, f, g, h = word(B_), word(C_), word(D_), word(F_), word(G_), word(H_)
        for i in range(64):
            o[HB + i], o[HC + i], o[HD + i], o[HF + i], o[HG + i], o[HH + i] = bit(b, i), bit(c, i), bit(d, i), bit(f, i), bit(g, i), bit(h, i)
            o[HU0 + i] = bit(b, i + 28) ^ bit(b, i + 34)
            o[HU1 + i] = bit(f, i + 14) ^ bit(f, i + 18)
            o[HV + i] = bit(b, i) & bit(c, i)
        s0, s1 = rot(b, 28) ^ rot(b, 34) ^ rot(b, 39), rot(f, 14) ^ rot(f, 18) ^ rot(f, 41)
        c_, m = (f & g) ^ (~f & h), (b & c) ^ (b & d) ^ (c & d)
        for at, x in ((HS0, s0), (HS1, s1), (HCH, c_), (HMAJ, m)):
            o[at], o[at + 1] = lo(x), hi(x)
        lv = (lim[:, r - r % BLOCK] != 0).any(axis=0).astype(np.uint64)
        lvn = nxt(lv)
        o[HLV] = lv
        for j in range(8):
            s_lo = _U(limb(IV512[j], 0)) + lim[A_ + 2 * j]
            czl = s_lo >> _U(32)
            s_hi = _U(limb(IV512[j], 1)) + lim[A_ + 2 * j + 1] + czl
            o[HPZ + 2 * j], o[HPZ + 2 * j + 1] = lvn * lo(s_lo), lvn * lo(s_hi)
            o[HCZ + 2 * j], o[HCZ + 2 * j + 1] = czl, s_hi >> _U(32)
        # the two round-0 sums of the next row's block: from IV LV' on a start row, from PZ on a chain row
        pz = lambda j, l: o[HPZ + 2 * j + l]
        carry = {}
        for l in (0, 1):
            h7 = np.where(chn == 1, pz(7, l), lvn * _U(limb(IV512[7], l)))
            h3 = np.where(chn == 1, pz(3, l), lvn * _U(limb(IV512[3], l)))
            t1 = nxt(o[HS1 + l]) + nxt(o[HCH + l]) + nxt(lim[W_ + l]) + lvn * _U(limb(K0, l))
            ca = h7 + t1 + nxt(o[HS0 + l]) + nxt(o[HMAJ + l]) + (carry["a", 0] if l else _U(0))
            ce = h3 + h7 + t1 + (carry["e", 0] if l else _U(0))
            carry["a", l], carry["e", l] = ((ca >> _U(32)) & _U(7)) * edge, ((ce >> _U(32)) & _U(7)) * edge
        for at, x in ((HCAL, carry["a", 0]), (HCAH, carry["a", 1]), (HCEL, carry["e", 0]), (HCEH, carry["e", 1])):
            for k in range(3):
                o[at + k] = (x >> _U(k)) & _U(1)
    return out


# ---- the 673 constraints over an abstract field (the fields are tests/sha_air_model.py's)
def _constraints(f, t, tn, h, hn, STA, CHN):
    """the 673 constraints of one proof: t[c], h[c] the table's and the helper's columns at x, tn, hn at omega x; STA, CHN the values of
    the two preprocessed columns at x"""
    add, sub, mul, k = f.add, f.sub, f.mul, f.k
    two, c32 = k(2), k(1 << 32)
    boolean = lambda x: sub(mul(x, x), x)
    xor = lambda x, y: sub(add(x, y), mul(two, mul(x, y)))

    def word(bits):
        acc = k(0)
        for i in range(31, -1, -1):
            acc = add(mul(acc, two), bits[i])
        return acc
    limbs = lambda bits: [word([bits(32 * l + i) for i in range(32)]) for l in (0, 1)]
    Bb, Cb, Db = (lambda i: h[HB + i % 64]), (lambda i: h[HC + i % 64]), (lambda i: h[HD + i % 64])
    Fb, Gb, Hb = (lambda i: h[HF + i % 64]), (lambda i: h[HG + i % 64]), (lambda i: h[HH + i % 64])
    out = [boolean(h[c]) for c in range(384)]
    out += [boolean(h[c]) for c in range(HCZ, HCZ + 16)]
    out += [boolean(h[c]) for c in range(HCAL, HCAL + 12)]
    out.append(boolean(h[HLV]))
    for col, bits in ((B_, Bb), (C_, Cb), (D_, Db), (F_, Fb), (G_, Gb), (H_, Hb)):
        out += [sub(t[col + l], w) for l, w in enumerate(limbs(bits))]
    out += [sub(h[HU0 + i], xor(Bb(i + 28), Bb(i + 34))) for i in range(64)]
    out += [sub(h[HU1 + i], xor(Fb(i + 14), Fb(i + 18))) for i in range(64)]
    out += [sub(h[HV + i], mul(Bb(i), Cb(i))) for i in range(64)]
    out += [sub(h[HS0 + l], w) for l, w in enumerate(limbs(lambda j: xor(h[HU0 + j], Bb(j + 39))))]
    out += [sub(h[HS1 + l], w) for l, w in enumerate(limbs(lambda j: xor(h[HU1 + j], Fb(j + 41))))]
    out += [sub(h[HCH + l], w) for l, w in enumerate(limbs(lambda j: add(Hb(j), mul(Fb(j), sub(Gb(j), Hb(j))))))]
    out += [sub(h[HMAJ + l], w) for l, w in
            enumerate(limbs(lambda j: add(h[HV + j], mul(Db(j), sub(add(Bb(j), Cb(j)), mul(two, h[HV + j]))))))]
    LVn = hn[HLV]
    for j in range(8):
        for l in (0, 1):
            s = sub(add(t[A_ + 2 * j + l], k(limb(IV512[j], l))), mul(c32, h[HCZ + 2 * j + l]))
            if l:
                s = add(s, h[HCZ + 2 * j])
            out.append(sub(h[HPZ + 2 * j + l], mul(LVn, s)))
    val = lambda at: add(h[at], add(mul(two, h[at + 1]), mul(k(4), h[at + 2])))
    ca, ce = (val(HCAL), val(HCAH)), (val(HCEL), val(HCEH))
    six = (0, 1, 2, 4, 5, 6)
    # the selected forms: the next row's limbs against IV LV' (start rows) and against PZ (chain rows)
    t1 = [add(add(hn[HS1 + l], hn[HCH + l]), tn[W_ + l]) for l in (0, 1)]
    t12 = [add(t1[l], add(hn[HS0 + l], hn[HMAJ + l])) for l in (0, 1)]
    an = [add(tn[A_], mul(c32, ca[0])), sub(add(tn[A_ + 1], mul(c32, ca[1])), ca[0])]
    en = [add(tn[E_], mul(c32, ce[0])), sub(add(tn[E_ + 1], mul(c32, ce[1])), ce[0])]
    for SELD, h7, h3, x_of in (
            (STA, [mul(LVn, k(limb(IV512[7], l))) for l in (0, 1)], [mul(LVn, k(limb(IV512[3], l))) for l in (0, 1)],
             lambda j, l: mul(LVn, k(limb(IV512[j], l)))),
            (CHN, [h[HPZ + 14 + l] for l in (0, 1)], [h[HPZ + 6 + l] for l in (0, 1)], lambda j, l: h[HPZ + 2 * j + l])):
        for j in six:
            for l in (0, 1):
                out.append(mul(SELD, sub(tn[B_ + 2 * j + l], x_of(j, l))))
        kl = [mul(LVn, k(limb(K0, l))) for l in (0, 1)]
        out += [mul(SELD, sub(an[l], add(add(h7[l], kl[l]), t12[l]))) for l in (0, 1)]
        out += [mul(SELD, sub(en[l], add(add(h3[l], h7[l]), add(kl[l], t1[l])))) for l in (0, 1)]
    assert len(out) == CONSTRAINTS
    return out


def integer_residuals(table, help_, pre=None):
    """the 673 constraints of ONE proof as integer expressions (no reduction mod p) on pre-LDE rows, rows cyclic, STA and CHN at their row
    values (pre: other columns [2][N] in their place).  Returns [673][N] Python integers as object arrays."""
    f = sm._Field()
    f.add, f.sub, f.mul, f.k = (lambda a, b: a + b), (lambda a, b: a - b), (lambda a, b: a * b), (lambda c: c)
    ints = lambda m, w: [np.array([int(x) for x in col], dtype=object) for col in np.asarray(m, dtype=np.uint64).reshape(w, -1)]
    t, h = ints(table, WIDTH), ints(help_, HELPER_COLS)
    STA, CHN = ints(periodic(t[0].size) if pre is None else pre, 2)
    return _constraints(f, t, [np.roll(c, -1) for c in t], h, [np.roll(c, -1) for c in h], STA, CHN)


# ---- gamma, the quotient
def gamma(oracle, log_n, log_blowup, cap_height, n_proofs, cap, cap_helper):
    """2^33, the set id 9, log_n, log_blowup, cap_height, n_proofs, the table cap, the helper cap; drawn again while gamma.c1 == 0.  STA
    and CHN are functions of log_n - log_blowup and are not observed"""
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


def quotient(oracle, log_n, log_blowup, n_proofs, cols, hcols, pext, shift, g, ints=False):
    """cols [18 n_proofs][M], hcols [629 n_proofs][M], pext [2][M] (the extended STA and CHN) words on the coset shift <gl_root(log_n)>;
    the planar quotient (2 M canonical words).  ints: with Python integers in object arrays instead of the uint64 field (slow; the
    cross-check)"""
    M, B = 1 << log_n, 1 << log_blowup
    N = M // B
    cols = np.asarray(cols, dtype=np.uint64).reshape(n_proofs * WIDTH, M)
    hcols = np.asarray(hcols, dtype=np.uint64).reshape(n_proofs * HELPER_COLS, M)
    pext = np.asarray(pext, dtype=np.uint64).reshape(2, M)
    w = oracle.gl_root(log_n)
    xs = [shift % P]
    for _ in range(B - 1):
        xs.append(xs[-1] * w % P)
    dt = object if ints else np.uint64
    zinv = np.array([pow((pow(x, N, P) - 1) % P, P - 2, P) for x in xs] * (M // B), dtype=dt)
    f = sm._base() if ints else sm._vec()
    canon = sm._obj if ints else (lambda v: np.asarray(v, dtype=np.uint64) % sm._P64)
    STA, CHN = canon(pext[0]), canon(pext[1])
    q0, q1 = np.zeros(M, dtype=dt), np.zeros(M, dtype=dt)
    gp = (1, 0)
    with np.errstate(over="ignore"):
        for p in range(n_proofs):
            t = [canon(c) for c in cols[p * WIDTH:(p + 1) * WIDTH]]
            h = [canon(c) for c in hcols[p * HELPER_COLS:(p + 1) * HELPER_COLS]]
            for term in _constraints(f, t, [np.roll(c, -B) for c in t], h, [np.roll(c, -B) for c in h], STA, CHN):
                if ints:
                    term = term % P
                    q0, q1 = q0 + gp[0] * term, q1 + gp[1] * term
                else:
                    q0, q1 = sm._addv(q0, sm._mulv(term, sm._U(gp[0]))), sm._addv(q1, sm._mulv(term, sm._U(gp[1])))
                gp = e_mul(gp, g)
        q0, q1 = (q0 % P * zinv % P, q1 % P * zinv % P) if ints else (sm._mulv(q0, zinv), sm._mulv(q1, zinv))
    return np.array([int(x) for x in q0] + [int(x) for x in q1], dtype=np.uint64)


# ---- STA and CHN at zeta
def periodic_at(oracle, log_rows, zeta):
    """[STA(zeta), CHN(zeta)], barycentric over the N rows (tests/sha512_air_model.py's sum over two columns)"""
    return s7.barycentric(oracle, log_rows, zeta, list(periodic(1 << log_rows)))


# ---- the identity at zeta
def constraint_sum(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, zeta, g, pre=None):
    """sum gamma^(673 p + j) C_(p,j) over F_p^2 from the openings at zeta (t0, h0) and zeta omega_N (t1, h1); pre: (STA, CHN) at zeta"""
    STA, CHN = periodic_at(oracle, log_n - log_blowup, zeta) if pre is None else pre
    f = sm._ext()
    acc, gp = (0, 0), (1, 0)
    for p in range(n_proofs):
        a, b = p * WIDTH, p * HELPER_COLS
        for term in _constraints(f, t0[a:a + WIDTH], t1[a:a + WIDTH], h0[b:b + HELPER_COLS], h1[b:b + HELPER_COLS], STA, CHN):
            acc = e_add(acc, e_mul(gp, term))
            gp = e_mul(gp, g)
    return acc


def identity_at(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, u0, u1, zeta, g, pre=None):
    """sum gamma^i C_i == (u_0 + X u_1) (zeta^N - 1), X (a, b) = (7 b, a)"""
    zn = dm.e_pow(zeta, 1 << (log_n - log_blowup))
    q = ((u0[0] + 7 * u1[1]) % P, (u0[1] + u1[0]) % P)
    return constraint_sum(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, zeta, g, pre) == e_mul(q, ((zn[0] - 1) % P, zn[1]))


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
