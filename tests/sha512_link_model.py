"""A pure-Python model of constraint set 10, the SHA-512 table's link to Level-1 (include/tmx.h "the SHA-512 table's link to Level-1"),
written from the header text and independent of libtmx: the public table of T.2 gathered from Level-1 ELEMENT rows (docs/witness_layout.md:
H.2 and the digest of D.1a; bytes are eight big-endian bit elements), the 65-column helper oracle, the five preprocessed planes, the 115
constraints written ONCE over an abstract field (`_constraints`: integer identities on the rows, the uint64 field on a coset), the public
side as one row vector V_r under gamma, and the quotient point by point.  A sibling of tests/sha_public_model.py on 64-bit words in lo / hi
limbs and 80-row blocks; it reuses the field helpers of tests/sha_air_model.py.  The yardstick of tests/test_sha512_link.py (not collected
by pytest).  Parity unpinned against plonky2, like the feature."""
import numpy as np

import air_model as am
import batch_model as bm
import deep_model as dm
import fri_model as fm
import sha512_air_model as s7
import sha512_init_model as s9
import sha_air_model as sm
import sha_public_model as sp
from fri_model import P, e_add, e_mul

WIDTH, PUB_WIDTH, HELPER_COLS, CONSTRAINTS, SET_ID = 18, 49, 65, 115, 10
PW_W, PW_DIG, PW_LV = 0, 32, 48  # columns inside a proof's 49 (a word's low limb first)
HCV, HDG, HCD, HLN, HCH = 0, 16, 32, 48, 49  # helper columns inside a proof's 65 (word j at + 2 j, + 2 j + 1)
# constraint indices inside a proof's 115 (a family's member 2 j + limb): the families from JLVN on carry a public term
JCD, JSUM, JCH, JSEL, JCHN, JSTA, JLVN, JDIG, JMSG = 0, 16, 32, 48, 64, 80, 96, 97, 113
BLOCK, LANE = 80, 160
W_, A_ = 0, 2  # the table's columns: W and the state word a (low limbs)
M32, M64, IV512 = s9.M32, s9.M64, s9.IV512
H2, H2_LANE, H2_PK, H2_R, H2_MSG, H2_MLEN, H2_SIGNED = 256, 1517, 0, 256, 520, 1512, 1516  # ValidatorVariable[N] and the fields inside one
D1A_LANE, D1A_DIGEST = 1136, 624  # a lane of D.1a and the 512 digest bits inside it
_U = np.uint64
limb = s9.limb


def log_k(log_rows):
    """log2 of the public table's rows: ceil(N / 80) slots -- the partial last one counts -- padded to a power of two"""
    return (-(-(1 << log_rows) // BLOCK) - 1).bit_length()


# ---- the element rows
def pad(msg):
    """SHA-512 padding: 80, zeros, the 128-bit bit length; whole 128-byte blocks"""
    return bytes(msg) + b"\x80" + bytes(-(len(msg) + 17) % 128) + (8 * len(msg)).to_bytes(16, "big")


def lane_message(row, i, dummy):
    """R | A | M of lane i as T.2 hashes it: the lane's own triple with the length clamped to 124 if it signed, else the dummy triple (dummy
    = (public key, signature) of plonky2x: dummy R, dummy key, 32 zero bytes)"""
    v = H2 + H2_LANE * i
    if int(row[v + H2_SIGNED]) & M32:
        mlen = min(int(row[v + H2_MLEN]), 124)
        return bytes(sp._bytes(row, v + H2_R, 32) + sp._bytes(row, v + H2_PK, 32) + sp._bytes(row, v + H2_MSG, mlen))
    return bytes(dummy[1][:32]) + bytes(dummy[0]) + bytes(32)


def messages(n, row, dummy):
    return [lane_message(row, i, dummy) for i in range(n)]


def lane_digest(kind, n, row, i):
    """the eight digest words of lane i from D.1a"""
    at = sp.Layout(kind, n).d1a + D1A_LANE * i + D1A_DIGEST
    return [int.from_bytes(bytes(sp._bytes(row, at + 64 * j, 8)), "big") for j in range(8)]


def public_table(kind, n, rows, lk, dummy):
    """rows: one element row per proof.  [49 n_proofs][2^lk] words: per slot k = (lane k / 2, block k mod 2) the sixteen message words, the
    digest on the last live block of the lane, lv.  Slots of lanes >= n (the partial last slot, the padding) are zero"""
    K = 1 << lk
    assert 2 * n <= K
    pub = np.zeros((PUB_WIDTH * len(rows), K), dtype=np.uint64)
    for p, row in enumerate(rows):
        o = PUB_WIDTH * p
        for i in range(n):
            padded = pad(lane_message(row, i, dummy))
            n_blocks = len(padded) // 128
            assert n_blocks in (1, 2)
            for b in range(n_blocks):
                k = 2 * i + b
                for t in range(16):
                    w = int.from_bytes(padded[128 * b + 8 * t:128 * b + 8 * t + 8], "big")
                    pub[o + PW_W + 2 * t, k], pub[o + PW_W + 2 * t + 1, k] = limb(w, 0), limb(w, 1)
                pub[o + PW_LV, k] = 1
            for j, w in enumerate(lane_digest(kind, n, row, i)):
                pub[o + PW_DIG + 2 * j, 2 * i + n_blocks - 1], pub[o + PW_DIG + 2 * j + 1, 2 * i + n_blocks - 1] = limb(w, 0), limb(w, 1)
    return pub


# ---- the helper oracle
def _flag(word):
    return 1 if int(word) & M32 else 0


def next_slot(k, N):
    """the slot of the row behind slot k's last row, cyclic inside the proof"""
    return k + 1 if BLOCK * (k + 1) < N else 0


def helper(table, pub, n_proofs, start0=None):
    """table: [18 n_proofs][N] pre-LDE words, pub: [49 n_proofs][2^log_k(N)].  [65 n_proofs][N] words; operands are the low 32 bits, lv is
    set when its low 32 bits are not zero.  start0: eight words that stand in for the IV in slot 0 -- NOT the helper the header states: the
    one a prover would commit who wants a first block that starts elsewhere (the test of the wrap row)"""
    table, pub = np.asarray(table, dtype=np.uint64), np.asarray(pub, dtype=np.uint64)
    N = table.shape[1]
    slots = -(-N // BLOCK)
    assert table.shape[0] == n_proofs * WIDTH and pub.shape == (n_proofs * PUB_WIDTH, 1 << log_k(N.bit_length() - 1))
    out = np.zeros((n_proofs * HELPER_COLS, N), dtype=np.uint64)
    for p in range(n_proofs):
        lim, o = table[p * WIDTH:(p + 1) * WIDTH] & _U(M32), p * HELPER_COLS
        lv = [_flag(x) for x in pub[p * PUB_WIDTH + PW_LV]]
        for k in range(slots):
            rows = slice(BLOCK * k, min(BLOCK * k + BLOCK, N))
            ln = lv[next_slot(k, N)]
            for j in range(8):
                word = lambda r: int(lim[A_ + 2 * j, r]) | int(lim[A_ + 2 * j + 1, r]) << 32
                first = lambda kk: start0[j] if start0 is not None and kk == 0 else IV512[j]
                if not lv[k]:
                    cv = 0
                elif k % 2 == 0:
                    cv = first(k)
                else:
                    cv = (lv[k - 1] * first(k - 1) + word(BLOCK * k - 1)) & M64
                lo = lim[A_ + 2 * j, rows] + _U(limb(cv, 0))
                hi = lim[A_ + 2 * j + 1, rows] + _U(limb(cv, 1)) + (lo >> _U(32))
                out[o + HCV + 2 * j, rows], out[o + HCV + 2 * j + 1, rows] = limb(cv, 0), limb(cv, 1)
                out[o + HDG + 2 * j, rows], out[o + HDG + 2 * j + 1, rows] = lo & _U(M32), hi & _U(M32)
                out[o + HCD + 2 * j, rows], out[o + HCD + 2 * j + 1, rows] = lo >> _U(32), hi >> _U(32)
                if ln:
                    out[o + HCH + 2 * j, rows], out[o + HCH + 2 * j + 1, rows] = lo & _U(M32), hi & _U(M32)
            out[o + HLN, rows] = ln
    return out


# ---- the preprocessed planes
def periodic(N, wrap=True):
    """[5][N]: STA (1 where r mod 160 = 159 and, switched on explicitly, on the wrap row N - 1), CHN (1 where r mod 160 = 79), SEL (set 7's: 0
    on the last row of every block and on row N - 1), E79 (1 where r mod 80 = 79), MSG (1 where r mod 80 < 16).  wrap = False: STA without
    the wrap row, the plane a test shows to be wrong"""
    assert (N - 1) % LANE in (127, 95, 31, 63)
    r = np.arange(N)
    sel = (r % BLOCK != BLOCK - 1) & (r != N - 1)
    sta = (r % LANE == LANE - 1) | ((r == N - 1) & wrap)
    return np.stack([x.astype(np.uint64) for x in (sta, r % LANE == BLOCK - 1, sel, r % BLOCK == BLOCK - 1, r % BLOCK < 16)])


# ---- the 115 constraints over an abstract field: the column parts; the public terms are subtracted by the caller
def _constraints(f, t, tn, h, hn, STA, CHN, SEL, E79, MSG):
    add, sub, mul, k = f.add, f.sub, f.mul, f.k
    c32 = k(1 << 32)
    out = [None] * CONSTRAINTS
    LN = h[HLN]
    for j in range(8):
        for l in (0, 1):
            c = 2 * j + l
            CV, DG, CD, CH, CVn, s = h[HCV + c], h[HDG + c], h[HCD + c], h[HCH + c], hn[HCV + c], t[A_ + c]
            out[JCD + c] = sub(mul(CD, CD), CD)
            total = sub(add(DG, mul(c32, CD)), add(CV, s))
            out[JSUM + c] = sub(total, h[HCD + c - 1]) if l else total
            out[JCH + c] = sub(CH, mul(LN, DG))
            out[JSEL + c] = mul(SEL, sub(CVn, CV))
            out[JCHN + c] = mul(CHN, sub(CVn, CH))
            out[JSTA + c] = mul(STA, sub(CVn, mul(k(limb(IV512[j], l)), LN)))
            out[JDIG + c] = sub(mul(E79, DG), mul(CHN, CH))
    out[JLVN] = mul(add(CHN, STA), LN)
    out[JMSG], out[JMSG + 1] = mul(MSG, t[W_]), mul(MSG, t[W_ + 1])
    return out


def public_rows(pub, N, wrap=True):
    """ONE proof: {constraint index: [N] integers}, the public term of each constraint that has one, as a value per row -- lv of the next
    slot on the rows where CHN + STA is on; dig of the row's slot on rows r mod 80 = 79; w[k][t] on rows 80 k + t, t < 16"""
    pub = np.asarray(pub, dtype=np.uint64)
    assert pub.shape == (PUB_WIDTH, 1 << log_k(N.bit_length() - 1))
    sta, chn, _, e79, msg = periodic(N, wrap)
    out = {j: np.zeros(N, dtype=object) for j in range(JLVN, CONSTRAINTS)}
    for r in range(N):
        k = r // BLOCK
        if sta[r] or chn[r]:
            out[JLVN][r] = int(pub[PW_LV, next_slot(k, N)])
        if e79[r]:
            for c in range(16):
                out[JDIG + c][r] = int(pub[PW_DIG + c, k])
        if msg[r]:
            for l in (0, 1):
                out[JMSG + l][r] = int(pub[PW_W + 2 * (r % BLOCK) + l, k])
    return out


def integer_residuals(table, help_, pub, wrap=True):
    """ONE proof: the 115 constraints as integer arrays over the rows (no reduction mod p), rows cyclic, the planes at their row values"""
    f = sm._Field()
    f.add, f.sub, f.mul, f.k = (lambda a, b: a + b), (lambda a, b: a - b), (lambda a, b: a * b), (lambda c: c)
    ints = lambda m, w: [np.array([int(x) for x in col], dtype=object) for col in np.asarray(m, dtype=np.uint64).reshape(w, -1)]
    t, h = ints(table, WIDTH), ints(help_, HELPER_COLS)
    N = t[0].size
    res = _constraints(f, t, [np.roll(c, -1) for c in t], h, [np.roll(c, -1) for c in h], *ints(periodic(N, wrap), 5))
    for j, v in public_rows(pub, N, wrap).items():
        res[j] = res[j] - v
    return res


# ---- gamma and the public side
def gamma(oracle, log_n, log_blowup, cap_height, n_proofs, cap, cap_helper, pub):
    """set 6's rule with the set id 10: 2^33, 10, log_n, log_blowup, cap_height, n_proofs, the table cap, the helper cap, the Poseidon Merkle
    root (cap height 0) of pub as a column-major oracle; drawn again while gamma.c1 == 0"""
    chal = fm.Challenger(oracle)
    chal.observe(1 << 33)
    for v in (SET_ID, log_n, log_blowup, cap_height, n_proofs):
        chal.observe(v)
    for c in (cap, cap_helper):
        c = np.asarray(c, dtype=np.uint64).reshape(-1)
        assert c.size == 4 << min(cap_height, log_n)
        chal.observe_all(c)
    chal.observe_all(sp.digest(oracle, pub))
    while True:
        g = chal.ext()
        if g[1]:
            return g


def combine(pub, N, g, wrap=True):
    """V_r = sum_p sum_j gamma^(115 p + j) (the public term of constraint j of proof p on row r): two planes of N integers mod p"""
    pub = np.asarray(pub, dtype=np.uint64)
    n_proofs = pub.shape[0] // PUB_WIDTH
    V = [np.zeros(N, dtype=object), np.zeros(N, dtype=object)]
    for p in range(n_proofs):
        for j, v in public_rows(pub[p * PUB_WIDTH:(p + 1) * PUB_WIDTH], N, wrap).items():
            gw = dm.e_pow(g, CONSTRAINTS * p + j)
            V[0], V[1] = (V[0] + gw[0] * v) % P, (V[1] + gw[1] * v) % P
    return V


def public_extended(oracle, log_n, log_blowup, pub, g, wrap=True):
    """Pub_gamma on the coset: the polynomial of degree < N through V_r on <omega_N>, two planes of M words"""
    N = 1 << (log_n - log_blowup)
    V = combine(pub, N, g, wrap)
    return oracle.lde(np.array([[int(x) for x in v] for v in V], dtype=np.uint64), log_blowup)


def quotient(oracle, log_n, log_blowup, n_proofs, cols, hcols, pext, pub, shift, g, proofs=None, wrap=True):
    """cols [18 n_proofs][M], hcols [65 n_proofs][M], pext [5][M] (the extended planes) words on the coset shift <gl_root(log_n)>, pub
    [49 n_proofs][K]; the planar quotient (2 M canonical words) = (sum_p sum_j gamma^(115 p + j) C_(p,j) - Pub_gamma) / (x^N - 1).
    proofs: a range of proof indices (the piece form; the piece that holds proof 0 carries - Pub_gamma); wrap = False: the public rows of an STA without the wrap row, to go with such planes in pext"""
    M, B = 1 << log_n, 1 << log_blowup
    N = M // B
    cols = np.asarray(cols, dtype=np.uint64).reshape(n_proofs * WIDTH, M)
    hcols = np.asarray(hcols, dtype=np.uint64).reshape(n_proofs * HELPER_COLS, M)
    w = oracle.gl_root(log_n)
    xs = [shift % P]
    for _ in range(B - 1):
        xs.append(xs[-1] * w % P)
    zinv = np.array([pow((pow(x, N, P) - 1) % P, P - 2, P) for x in xs] * (M // B), dtype=np.uint64)
    f = sm._vec()
    canon = lambda v: np.asarray(v, dtype=np.uint64) % sm._P64
    planes = [canon(c) for c in np.asarray(pext, dtype=np.uint64).reshape(5, M)]
    q0, q1 = np.zeros(M, dtype=np.uint64), np.zeros(M, dtype=np.uint64)
    rng = range(n_proofs) if proofs is None else proofs
    with np.errstate(over="ignore"):
        for p in rng:
            gp = dm.e_pow(g, CONSTRAINTS * p)
            t = [canon(c) for c in cols[p * WIDTH:(p + 1) * WIDTH]]
            h = [canon(c) for c in hcols[p * HELPER_COLS:(p + 1) * HELPER_COLS]]
            for term in _constraints(f, t, [np.roll(c, -B) for c in t], h, [np.roll(c, -B) for c in h], *planes):
                q0, q1 = sm._addv(q0, sm._mulv(term, sm._U(gp[0]))), sm._addv(q1, sm._mulv(term, sm._U(gp[1])))
                gp = e_mul(gp, g)
        if 0 in rng:
            pe = public_extended(oracle, log_n, log_blowup, pub, g, wrap)
            q0, q1 = sm._subv(q0, canon(pe[0])), sm._subv(q1, canon(pe[1]))
        q0, q1 = sm._mulv(q0, zinv), sm._mulv(q1, zinv)
    return np.array([int(x) for x in q0] + [int(x) for x in q1], dtype=np.uint64)


# ---- the identity at zeta
def periodic_at(oracle, log_rows, zeta):
    """the five planes at zeta, barycentric over the N rows"""
    return s7.barycentric(oracle, log_rows, zeta, cols=periodic(1 << log_rows))


def public_at(oracle, log_rows, V, zeta):
    """Pub_gamma(zeta) from the two planes of V: A(zeta) + X B(zeta), X (a, b) = (7 b, a)"""
    a, b = s7.barycentric(oracle, log_rows, zeta, cols=[[int(x) for x in v] for v in V])
    return e_add(a, e_mul((0, 1), b))


def constraint_sum(oracle, n_proofs, t0, t1, h0, h1, g, planes):
    """sum gamma^(115 p + j) C_(p,j) over F_p^2 from the openings at zeta (t0, h0) and zeta omega_N (t1, h1): the column parts"""
    f = sm._ext()
    acc = (0, 0)
    for p in range(n_proofs):
        a, b = p * WIDTH, p * HELPER_COLS
        gp = dm.e_pow(g, CONSTRAINTS * p)
        for term in _constraints(f, t0[a:a + WIDTH], t1[a:a + WIDTH], h0[b:b + HELPER_COLS], h1[b:b + HELPER_COLS], *planes):
            acc = e_add(acc, e_mul(gp, term))
            gp = e_mul(gp, g)
    return acc


def identity_at(oracle, log_n, log_blowup, n_proofs, t0, t1, h0, h1, u0, u1, zeta, g, pub, planes=None, pubz=None):
    """sum gamma^i C_i - Pub_gamma(zeta) == (u_0 + X u_1) (zeta^N - 1); the planes and Pub_gamma at zeta barycentric over the N rows"""
    log_rows = log_n - log_blowup
    planes = periodic_at(oracle, log_rows, zeta) if planes is None else planes
    pubz = public_at(oracle, log_rows, combine(pub, 1 << log_rows, g), zeta) if pubz is None else pubz
    zn = dm.e_pow(zeta, 1 << log_rows)
    q = ((u0[0] + 7 * u1[1]) % P, (u0[1] + u1[0]) % P)
    return fm.e_sub(constraint_sum(oracle, n_proofs, t0, t1, h0, h1, g, planes), pubz) == e_mul(q, ((zn[0] - 1) % P, zn[1]))


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
    return [ok and holds for ok in bm.verify(oracle, p, caps, proof, shift)]
