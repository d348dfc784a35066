"""A pure-Python model of the SHA-512 table's message-schedule constraints (include/tmx.h "the message schedule of the SHA-512 table",
constraint set 8), written from the header text and independent of libtmx: the preprocessed column SCH of full degree, the helper oracle
(the bits of W, the two xor rows, sigma0 and sigma1 as limbs, the schedule sum as one carry-free pipeline of fifteen columns per limb, two
carry bits per limb), gamma from a fresh duplex over the table cap and the helper cap, the quotient point by point over the extended
columns, the identity at zeta from a batch proof's openings, and `verify` = tests/batch_model.py's verifier and that identity, with the
helper's oracle index explicit.  A sibling of tests/sha_sched_model.py on 64-bit words in lo / hi limbs; it reuses the field helpers of
tests/sha_air_model.py and `barycentric` of tests/sha512_air_model.py; the 234 constraints are written ONCE (`_constraints`) over an
abstract field.  The yardstick of tests/test_sha512_sched.py (not collected by pytest).  Parity unpinned against plonky2, like the feature."""
import numpy as np

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha512_air_model as s7
import sha_air_model as sm
from fri_model import P, e_add, e_mul

WIDTH, HELPER_COLS, CONSTRAINTS = 18, 230, 234
SET_ID = 8
BLOCK = 80
W_ = 0  # the table's W column inside a proof: the low limb; the high limb is the next one
HWB, HX0, HX1, HG0, HG1, HQL, HQH, HCL, HCH = 0, 64, 128, 192, 194, 195, 210, 226, 228  # the helper's columns; QL_k at HQL + k, QH_k at HQH + k
JCARRY, JWORD, JX0, JX1, JG0, JG1, JQL, JQH, JNEXT = 64, 68, 70, 134, 198, 200, 201, 216, 232  # constraint indices; QL_k's at JQL + k
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1
_U = np.uint64


def small_sigma0(w):
    return s7.rotr(w, 1) ^ s7.rotr(w, 8) ^ (w >> 7)


def small_sigma1(w):
    return s7.rotr(w, 19) ^ s7.rotr(w, 61) ^ (w >> 6)


def schedule_row(r, N):
    """SCH's support: the NEXT row is a schedule row of the same block (W_t, t = r mod 80 + 1 in 16 .. 79), and r is not the wrap row"""
    return 15 <= r % BLOCK <= BLOCK - 2 and r != N - 1


# ---- the preprocessed column
def periodic(N):
    """[N]: SCH.  (N - 1) mod 80 always lies in 15 .. 78, so the wrap row is switched off explicitly"""
    assert 15 <= (N - 1) % BLOCK <= BLOCK - 2
    return np.array([schedule_row(r, N) for r in range(N)], dtype=np.uint64)


# ---- the helper oracle
def helper(table, n_proofs):
    """table: [18 n_proofs][N] words (pre-LDE, any 64-bit words: the operands are the low 32 bits of columns 0 and 1); the helper
    [230 n_proofs][N].  Rows are cyclic inside one proof.  Vectorised over the rows with numpy uint64 (every limb sum stays below 2^34)."""
    table = np.asarray(table, dtype=np.uint64).reshape(n_proofs * WIDTH, -1)
    N = table.shape[1]
    out = np.zeros((n_proofs * HELPER_COLS, N), dtype=np.uint64)
    bit = lambda x, i: (x >> _U(i % 64)) & _U(1)
    rot = lambda x, n: (x >> _U(n)) | (x << _U(64 - n))
    lo, hi = (lambda x: x & _U(M32)), (lambda x: x >> _U(32))
    sch = periodic(N)
    for p in range(n_proofs):
        w_lo, w_hi = table[p * WIDTH + W_] & _U(M32), table[p * WIDTH + W_ + 1] & _U(M32)
        w = w_lo | (w_hi << _U(32))
        o = out[p * HELPER_COLS:(p + 1) * HELPER_COLS]
        for i in range(64):
            o[HWB + i] = bit(w, i)
            o[HX0 + i] = bit(w, i + 1) ^ bit(w, i + 8)
            o[HX1 + i] = bit(w, i + 19) ^ bit(w, i + 61)
        g0 = rot(w, 1) ^ rot(w, 8) ^ (w >> _U(7))
        g1 = rot(w, 19) ^ rot(w, 61) ^ (w >> _U(6))
        o[HG0], o[HG0 + 1], o[HG1], o[HG1 + 1] = lo(g0), hi(g0), lo(g1), hi(g1)
        for at, wl, l in ((HQL, w_lo, 0), (HQH, w_hi, 1)):
            o[at + 1] = np.roll(wl, 1) + o[HG0 + l]
            for k in range(2, 16):
                o[at + k] = np.roll(o[at + k - 1], 1) + (wl if k == 9 else 0) + (o[HG1 + l] if k == 14 else 0)
        cl = ((o[HQL + 15] >> _U(32)) & _U(3)) * sch
        ch = (((o[HQH + 15] + cl) >> _U(32)) & _U(3)) * sch
        o[HCL], o[HCL + 1], o[HCH], o[HCH + 1] = cl & _U(1), cl >> _U(1), ch & _U(1), ch >> _U(1)
    return out


# ---- the 234 constraints over an abstract field (the fields are tests/sha_air_model.py's)
def _constraints(f, t, tn, h, hn, SCH):
    """the 234 constraints of one proof: t[c], h[c] the table's and the helper's columns at x, tn, hn at omega x; SCH the value of the
    preprocessed column at x"""
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
    wb = lambda i: h[HWB + i % 64]
    out = [boolean(h[HWB + i]) for i in range(64)]
    out += [boolean(h[c]) for c in (HCL, HCL + 1, HCH, HCH + 1)]
    out += [sub(t[W_ + l], w) for l, w in enumerate(limbs(wb))]
    out += [sub(h[HX0 + i], xor(wb(i + 1), wb(i + 8))) for i in range(64)]
    out += [sub(h[HX1 + i], xor(wb(i + 19), wb(i + 61))) for i in range(64)]
    out += [sub(h[HG0 + l], w) for l, w in enumerate(limbs(lambda j: xor(h[HX0 + j], wb(j + 7)) if j < 57 else h[HX0 + j]))]
    out += [sub(h[HG1 + l], w) for l, w in enumerate(limbs(lambda j: xor(h[HX1 + j], wb(j + 6)) if j < 58 else h[HX1 + j]))]
    for at, l in ((HQL, 0), (HQH, 1)):
        out.append(sub(hn[at + 1], add(t[W_ + l], hn[HG0 + l])))
        for q in range(2, 16):
            rhs = h[at + q - 1]
            if q == 9:
                rhs = add(rhs, tn[W_ + l])
            if q == 14:
                rhs = add(rhs, hn[HG1 + l])
            out.append(sub(hn[at + q], rhs))
    val = lambda at: add(h[at], mul(two, h[at + 1]))
    c32 = lambda at: mul(k(1 << 32), val(at))
    out.append(mul(SCH, sub(add(tn[W_], c32(HCL)), h[HQL + 15])))
    out.append(mul(SCH, sub(sub(add(tn[W_ + 1], c32(HCH)), h[HQH + 15]), val(HCL))))
    assert len(out) == CONSTRAINTS
    return out


def integer_residuals(table, help_, sch=None):
    """the 234 constraints of ONE proof as integer expressions (no reduction mod p) on pre-LDE rows, rows cyclic, SCH at its row values
    (sch: another column in its place).  Returns [234][N] Python integers as object arrays."""
    f = sm._Field()
    f.add, f.sub, f.mul, f.k = (lambda a, b: a + b), (lambda a, b: a - b), (lambda a, b: a * b), (lambda c: c)
    ints = lambda m, w: [np.array([int(x) for x in col], dtype=object) for col in np.asarray(m, dtype=np.uint64).reshape(w, -1)]
    t, h = ints(table, WIDTH), ints(help_, HELPER_COLS)
    SCH = ints(periodic(t[0].size) if sch is None else sch, 1)[0]
    return _constraints(f, t, [np.roll(c, -1) for c in t], h, [np.roll(c, -1) for c in h], SCH)


# ---- gamma, the quotient
def gamma(oracle, log_n, log_blowup, cap_height, n_proofs, cap, cap_helper):
    """2^33, the set id 8, log_n, log_blowup, cap_height, n_proofs, the table cap, the helper cap; drawn again while gamma.c1 == 0.  SCH is
    a function of log_n - log_blowup and is not observed"""
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
    """cols [18 n_proofs][M], hcols [230 n_proofs][M], pext [M] (the extended SCH) words on the coset shift <gl_root(log_n)>; the planar
    quotient (2 M canonical words).  ints: with Python integers in object arrays instead of the uint64 field (slow; the cross-check)"""
    M, B = 1 << log_n, 1 << log_blowup
    N = M // B
    cols = np.asarray(cols, dtype=np.uint64).reshape(n_proofs * WIDTH, M)
    hcols = np.asarray(hcols, dtype=np.uint64).reshape(n_proofs * HELPER_COLS, M)
    pext = np.asarray(pext, dtype=np.uint64).reshape(M)
    w = oracle.gl_root(log_n)
    xs = [shift % P]
    for _ in range(B - 1):
        xs.append(xs[-1] * w % P)
    dt = object if ints else np.uint64
    zinv = np.array([pow((pow(x, N, P) - 1) % P, P - 2, P) for x in xs] * (M // B), dtype=dt)
    f = sm._base() if ints else sm._vec()
    canon = sm._obj if ints else (lambda v: np.asarray(v, dtype=np.uint64) % sm._P64)
    SCH = canon(pext)
    q0, q1 = np.zeros(M, dtype=dt), np.zeros(M, dtype=dt)
    gp = (1, 0)
    with np.errstate(over="ignore"):
        for p in range(n_proofs):
            t = [canon(c) for c in cols[p * WIDTH:(p + 1) * WIDTH]]
            h = [canon(c) for c in hcols[p * HELPER_COLS:(p + 1) * HELPER_COLS]]
            for term in _constraints(f, t, [np.roll(c, -B) for c in t], h, [np.roll(c, -B) for c in h], SCH):
                if ints:
                    term = term % P
                    q0, q1 = q0 + gp[0] * term, q1 + gp[1] * term
                else:
                    q0, q1 = sm._addv(q0, sm._mulv(term, sm._U(gp[0]))), sm._addv(q1, sm._mulv(term, sm._U(gp[1])))
                gp = e_mul(gp, g)
        q0, q1 = (q0 % P * zinv % P, q1 % P * zinv % P) if ints else (sm._mulv(q0, zinv), sm._mulv(q1, zinv))
    return np.array([int(x) for x in q0] + [int(x) for x in q1], dtype=np.uint64)


# ---- SCH at zeta
def sch_at(oracle, log_rows, zeta):
    """SCH(zeta), barycentric over the N rows (tests/sha512_air_model.py's sum over one column)"""
    return s7.barycentric(oracle, log_rows, zeta, [periodic(1 << log_rows)])[0]


# ---- the identity at zeta
def constraint_sum(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, zeta, g, pre=None):
    """sum gamma^(234 p + j) C_(p,j) over F_p^2 from the openings at zeta (t0, h0) and zeta omega_N (t1, h1); pre: SCH at zeta"""
    SCH = sch_at(oracle, log_n - log_blowup, zeta) if pre is None else pre
    f = sm._ext()
    acc, gp = (0, 0), (1, 0)
    for p in range(n_proofs):
        a, b = p * WIDTH, p * HELPER_COLS
        for term in _constraints(f, t0[a:a + WIDTH], t1[a:a + WIDTH], h0[b:b + HELPER_COLS], h1[b:b + HELPER_COLS], SCH):
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
