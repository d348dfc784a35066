"""A pure-Python model of the SHA-512 table's round constraints (include/tmx.h "the round constraints of the SHA-512 table", constraint
set 7), written from the header text and independent of libtmx: the three preprocessed columns SEL, KLO and KHI of full degree, the helper
oracle of 599 columns, the 628 constraints, gamma from a fresh duplex over the table cap and the helper cap, the quotient point by point
over the extended columns, the barycentric values of the preprocessed columns at zeta, the identity at zeta from a batch proof's openings,
and `verify` = tests/batch_model.py's verifier and that identity.  A sibling of tests/sha_air_model.py, built on its field helpers; the 628
constraints are written ONCE (`_constraints`) over an abstract field.  The yardstick of tests/test_sha512_air.py (not collected by pytest).
Parity unpinned against plonky2, like the feature."""
import numpy as np

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha_air_model as sm
from fri_model import P, e_add, e_mul, e_sub

WIDTH, HELPER_COLS, CONSTRAINTS = 18, 599, 628
SET_ID = 7
BLOCK = 80
W_, A_, B_, C_, D_, E_, F_, G_, H_ = range(0, 18, 2)  # the low limb's column inside a proof; the high limb is the next one
HA, HB, HC, HE, HF, HG, HU0, HU1, HV = range(0, 576, 64)  # the helper's bit groups
HS0, HS1, HCH, HMAJ, HLIVE, HKL, HCAL, HCAH, HCEL, HCEH = 576, 578, 580, 582, 584, 585, 587, 590, 593, 596
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1


def _icbrt(n):
    x = 1 << -(-n.bit_length() // 3)
    while True:
        y = (2 * x + n // (x * x)) // 3
        if y >= x:
            return x
        x = y


def _primes(n):
    out, c = [], 2
    while len(out) < n:
        if all(c % q for q in out):
            out.append(c)
        c += 1
    return out


# the first 64 bits of the fractional parts of the cube roots of the first eighty primes (FIPS 180-4, 4.2.3)
K512 = [_icbrt(q << 192) & M64 for q in _primes(80)]
assert K512[0] == 0x428a2f98d728ae22 and K512[79] == 0x6c44198c4a475817


def rotr(x, n):
    return ((x >> n) | (x << (64 - n))) & M64


def sigma0(a):
    return rotr(a, 28) ^ rotr(a, 34) ^ rotr(a, 39)


def sigma1(e):
    return rotr(e, 14) ^ rotr(e, 18) ^ rotr(e, 41)


def ch(e, f, g):
    return (e & f) ^ (~e & g & M64)


def maj(a, b, c):
    return (a & b) ^ (a & c) ^ (b & c)


def sha_round(state, w, t):
    """the state (a .. h, 64-bit words) after round t from the state before it and W_t"""
    a, b, c, d, e, f, g, h = state
    t1 = h + sigma1(e) + ch(e, f, g) + K512[t] + w
    t2 = sigma0(a) + maj(a, b, c)
    return [(t1 + t2) & M64, a, b, c, (d + t1) & M64, e, f, g]


# ---- the preprocessed columns
def periodic(N):
    """[3][N]: SEL (0 on the last row of every 80-row block and on row N - 1), KLO, KHI (the limbs of K512[r mod 80] on every row)"""
    assert (N - 1) % BLOCK != BLOCK - 1
    r = np.arange(N)
    k = np.array(K512, dtype=np.uint64)[r % BLOCK]
    sel = ((r % BLOCK != BLOCK - 1) & (r != N - 1)).astype(np.uint64)
    return np.stack([sel, k & np.uint64(M32), k >> np.uint64(32)])


# ---- the helper oracle
def helper(table, n_proofs):
    """table: [18 n_proofs][N] words (pre-LDE, any 64-bit words: the operands are their low 32 bits); the helper [599 n_proofs][N].
    Vectorised over the rows with numpy uint64 (every limb sum stays below 2^35)."""
    table = np.asarray(table, dtype=np.uint64).reshape(n_proofs * WIDTH, -1)
    N = table.shape[1]
    u = np.uint64
    out = np.zeros((n_proofs * HELPER_COLS, N), dtype=np.uint64)
    bit = lambda x, i: (x >> u(i % 64)) & u(1)
    rot = lambda x, n: (x >> u(n)) | (x << u(64 - n))
    r = np.arange(N)
    sel, klo, khi = periodic(N)
    k_row = klo | (khi << u(32))
    for p in range(n_proofs):
        lim = table[p * WIDTH:(p + 1) * WIDTH] & u(M32)
        word = lambda c: lim[c] | (lim[c + 1] << u(32))
        o = out[p * HELPER_COLS:(p + 1) * HELPER_COLS]
        a, b, c, e, f, g = word(A_), word(B_), word(C_), word(E_), word(F_), word(G_)
        for i in range(64):
            o[HA + i], o[HB + i], o[HC + i], o[HE + i], o[HF + i], o[HG + i] = bit(a, i), bit(b, i), bit(c, i), bit(e, i), bit(f, i), bit(g, i)
            o[HU0 + i] = bit(a, i + 28) ^ bit(a, i + 34)
            o[HU1 + i] = bit(e, i + 14) ^ bit(e, i + 18)
            o[HV + i] = bit(a, i) & bit(b, i)
        s0, s1 = rot(a, 28) ^ rot(a, 34) ^ rot(a, 39), rot(e, 14) ^ rot(e, 18) ^ rot(e, 41)
        c_, m = (e & f) ^ (~e & g), (a & b) ^ (a & c) ^ (b & c)
        live = (lim[:, r - r % BLOCK] != 0).any(axis=0).astype(np.uint64)
        kl = live * k_row
        lo, hi = (lambda x: x & u(M32)), (lambda x: x >> u(32))
        for at, x in ((HS0, s0), (HS1, s1), (HCH, c_), (HMAJ, m)):
            o[at], o[at + 1] = lo(x), hi(x)
        o[HLIVE], o[HKL], o[HKL + 1] = live, lo(kl), hi(kl)
        nxt = lambda x: np.roll(x, -1)
        t1_lo = lim[H_] + lo(s1) + lo(c_) + nxt(lo(kl)) + nxt(lim[W_])
        t1_hi = lim[H_ + 1] + hi(s1) + hi(c_) + nxt(hi(kl)) + nxt(lim[W_ + 1])
        cal = ((t1_lo + lo(s0) + lo(m)) >> u(32)) & u(7)
        cah = ((t1_hi + hi(s0) + hi(m) + cal) >> u(32)) & u(7)
        cel = ((t1_lo + lim[D_]) >> u(32)) & u(7)
        ceh = ((t1_hi + lim[D_ + 1] + cel) >> u(32)) & u(7)
        for at, x in ((HCAL, cal), (HCAH, cah), (HCEL, cel), (HCEH, ceh)):
            for k in range(3):
                o[at + k] = ((x >> u(k)) & u(1)) * sel
    return out


# ---- the 628 constraints over an abstract field (the fields are tests/sha_air_model.py's)
def _constraints(f, t, tn, h, hn, SEL, KLO, KHI):
    """the 628 constraints of one proof: t[c], h[c] the table's and the helper's columns at x, tn, hn at omega x; SEL, KLO, KHI the values of
    the three preprocessed columns at x"""
    add, sub, mul, k = f.add, f.sub, f.mul, f.k
    two = k(2)
    boolean = lambda x: sub(mul(x, x), x)
    xor = lambda x, y: sub(add(x, y), mul(two, mul(x, y)))

    def word(bits):
        acc = k(0)
        for i in range(31, -1, -1):
            acc = add(mul(acc, two), bits[i])
        return acc
    limbs = lambda bits: [word([bits(32 * l + i) for i in range(32)]) for l in (0, 1)]
    out = [boolean(h[c]) for c in range(384)]
    out += [boolean(h[c]) for c in range(HCAL, HCAL + 12)]
    out.append(boolean(h[HLIVE]))
    Ab, Bb, Cb = (lambda i: h[HA + i % 64]), (lambda i: h[HB + i % 64]), (lambda i: h[HC + i % 64])
    Eb, Fb, Gb = (lambda i: h[HE + i % 64]), (lambda i: h[HF + i % 64]), (lambda i: h[HG + i % 64])
    for col, bits in ((A_, Ab), (B_, Bb), (C_, Cb), (E_, Eb), (F_, Fb), (G_, Gb)):
        out += [sub(t[col + l], w) for l, w in enumerate(limbs(bits))]
    out += [sub(h[HU0 + i], xor(Ab(i + 28), Ab(i + 34))) for i in range(64)]
    out += [sub(h[HU1 + i], xor(Eb(i + 14), Eb(i + 18))) for i in range(64)]
    out += [sub(h[HV + i], mul(Ab(i), Bb(i))) for i in range(64)]
    for at, bits in ((HS0, lambda i: xor(h[HU0 + i], Ab(i + 39))), (HS1, lambda i: xor(h[HU1 + i], Eb(i + 41))),
                     (HCH, lambda i: add(Gb(i), mul(Eb(i), sub(Fb(i), Gb(i))))),
                     (HMAJ, lambda i: add(h[HV + i], mul(Cb(i), sub(add(Ab(i), Bb(i)), mul(two, h[HV + i])))))):
        out += [sub(h[at + l], w) for l, w in enumerate(limbs(bits))]
    out.append(sub(h[HKL], mul(h[HLIVE], KLO)))
    out.append(sub(h[HKL + 1], mul(h[HLIVE], KHI)))
    for nxt, cur in ((B_, A_), (C_, B_), (D_, C_), (F_, E_), (G_, F_), (H_, G_)):
        out += [mul(SEL, sub(tn[nxt + l], t[cur + l])) for l in (0, 1)]
    out.append(mul(SEL, sub(hn[HLIVE], h[HLIVE])))
    val = lambda at: add(h[at], add(mul(two, h[at + 1]), mul(k(4), h[at + 2])))
    c32 = lambda at: mul(k(1 << 32), val(at))
    t1 = [add(add(add(t[H_ + l], h[HS1 + l]), add(h[HCH + l], hn[HKL + l])), tn[W_ + l]) for l in (0, 1)]
    out.append(mul(SEL, sub(add(tn[A_], c32(HCAL)), add(t1[0], add(h[HS0], h[HMAJ])))))
    out.append(mul(SEL, sub(sub(add(tn[A_ + 1], c32(HCAH)), add(t1[1], add(h[HS0 + 1], h[HMAJ + 1]))), val(HCAL))))
    out.append(mul(SEL, sub(add(tn[E_], c32(HCEL)), add(t[D_], t1[0]))))
    out.append(mul(SEL, sub(sub(add(tn[E_ + 1], c32(HCEH)), add(t[D_ + 1], t1[1])), val(HCEL))))
    assert len(out) == CONSTRAINTS
    return out


def integer_residuals(table, help_):
    """the 628 constraints of ONE proof as integer expressions (no reduction mod p) on pre-LDE rows, the preprocessed columns at their row
    values.  Returns [628][N] Python integers as object arrays."""
    f = sm._Field()
    f.add, f.sub, f.mul, f.k = (lambda a, b: a + b), (lambda a, b: a - b), (lambda a, b: a * b), (lambda c: c)
    ints = lambda m, w: [np.array([int(x) for x in col], dtype=object) for col in np.asarray(m, dtype=np.uint64).reshape(w, -1)]
    t, h = ints(table, WIDTH), ints(help_, HELPER_COLS)
    sel, klo, khi = ints(periodic(t[0].size), 3)
    return _constraints(f, t, [np.roll(c, -1) for c in t], h, [np.roll(c, -1) for c in h], sel, klo, khi)


# ---- gamma, the quotient
def gamma(oracle, log_n, log_blowup, cap_height, n_proofs, cap, cap_helper):
    """2^33, the set id 7, log_n, log_blowup, cap_height, n_proofs, the table cap, the helper cap; drawn again while gamma.c1 == 0.  The
    preprocessed columns are a function of log_n - log_blowup and are not observed"""
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
    """cols [18 n_proofs][M], hcols [599 n_proofs][M], pext [3][M] (the extended preprocessed columns) words on the coset shift
    <gl_root(log_n)>; the planar quotient (2 M canonical words).  ints: with Python integers in object arrays (slow; the cross-check)"""
    M, B = 1 << log_n, 1 << log_blowup
    N = M // B
    cols = np.asarray(cols, dtype=np.uint64).reshape(n_proofs * WIDTH, M)
    hcols = np.asarray(hcols, dtype=np.uint64).reshape(n_proofs * HELPER_COLS, M)
    pext = np.asarray(pext, dtype=np.uint64).reshape(3, M)
    w = oracle.gl_root(log_n)
    xs = [shift % P]
    for _ in range(B - 1):
        xs.append(xs[-1] * w % P)
    dt = object if ints else np.uint64
    zinv = np.array([pow((pow(x, N, P) - 1) % P, P - 2, P) for x in xs] * (M // B), dtype=dt)
    f = sm._base() if ints else sm._vec()
    canon = sm._obj if ints else (lambda v: np.asarray(v, dtype=np.uint64) % sm._P64)
    SEL, KLO, KHI = (canon(c) for c in pext)
    q0, q1 = np.zeros(M, dtype=dt), np.zeros(M, dtype=dt)
    gp = (1, 0)
    with np.errstate(over="ignore"):
        for p in range(n_proofs):
            t = [canon(c) for c in cols[p * WIDTH:(p + 1) * WIDTH]]
            h = [canon(c) for c in hcols[p * HELPER_COLS:(p + 1) * HELPER_COLS]]
            for term in _constraints(f, t, [np.roll(c, -B) for c in t], h, [np.roll(c, -B) for c in h], SEL, KLO, KHI):
                if ints:
                    term = term % P
                    q0, q1 = q0 + gp[0] * term, q1 + gp[1] * term
                else:
                    q0, q1 = sm._addv(q0, sm._mulv(term, sm._U(gp[0]))), sm._addv(q1, sm._mulv(term, sm._U(gp[1])))
                gp = e_mul(gp, g)
        q0, q1 = (q0 % P * zinv % P, q1 % P * zinv % P) if ints else (sm._mulv(q0, zinv), sm._mulv(q1, zinv))
    return np.array([int(x) for x in q0] + [int(x) for x in q1], dtype=np.uint64)


# ---- the preprocessed columns at zeta
def barycentric(oracle, log_rows, zeta, cols=None):
    """[P(zeta)] of the polynomials of degree < N through the columns (default: the three preprocessed ones) on <omega_N>:
    P(zeta) = (zeta^N - 1) / N  sum_r v_r omega^r / (zeta - omega^r), the N inversions batched into one"""
    N = 1 << log_rows
    cols = periodic(N) if cols is None else cols
    om = oracle.gl_root(log_rows)
    pts, den, pre, run, x = [], [], [], (1, 0), 1
    for _ in range(N):
        d = ((zeta[0] - x) % P, zeta[1])
        assert d != (0, 0)
        pts.append(x)
        den.append(d)
        pre.append(run)
        run = e_mul(run, d)
        x = x * om % P
    inv = dm.e_inv(run)
    sums = [(0, 0)] * len(cols)
    for r in range(N - 1, -1, -1):
        di = e_mul(inv, pre[r])
        inv = e_mul(inv, den[r])
        di = fm.e_scale(di, pts[r])
        sums = [e_add(s, fm.e_scale(di, int(c[r]))) if c[r] else s for s, c in zip(sums, cols)]
    zn = dm.e_pow(zeta, N)
    lead = fm.e_scale(((zn[0] - 1) % P, zn[1]), pow(N, P - 2, P))
    return [e_mul(lead, s) for s in sums]


# ---- the identity at zeta
def constraint_sum(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, zeta, g, pre=None):
    """sum gamma^(628 p + j) C_(p,j) over F_p^2 from the openings at zeta (t0, h0) and zeta omega_N (t1, h1); pre: (SEL, KLO, KHI) at zeta"""
    SEL, KLO, KHI = barycentric(oracle, log_n - log_blowup, zeta) if pre is None else pre
    f = sm._ext()
    acc, gp = (0, 0), (1, 0)
    for p in range(n_proofs):
        a, b = p * WIDTH, p * HELPER_COLS
        for term in _constraints(f, t0[a:a + WIDTH], t1[a:a + WIDTH], h0[b:b + HELPER_COLS], h1[b:b + HELPER_COLS], SEL, KLO, KHI):
            acc = e_add(acc, e_mul(gp, term))
            gp = e_mul(gp, g)
    return acc


def identity_at(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, u0, u1, zeta, g, pre=None):
    """sum gamma^i C_i == (u_0 + X u_1) (zeta^N - 1), X (a, b) = (7 b, a)"""
    zn = dm.e_pow(zeta, 1 << (log_n - log_blowup))
    q = ((u0[0] + 7 * u1[1]) % P, (u0[1] + u1[0]) % P)
    return constraint_sum(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, zeta, g, pre) == e_mul(q, ((zn[0] - 1) % P, zn[1]))


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
