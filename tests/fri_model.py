"""A pure-Python model of the batched FRI proof (include/tmx.h "a batched FRI low-degree proof"), written from the mathematics of the header
and independent of libtmx: F_p^2 = F_p[X] / (X^2 - 7) in Python integers; hashing, trees and transforms from the CPU oracle (oracle_c:
poseidon_permute, poseidon_merkle, ntt, gl_root).  The prover folds whole layers with the radix-2 definition; the verifier folds single
leaves.  The yardstick of tests/test_fri.py (not collected by pytest).  Parity unpinned against plonky2, like the feature itself."""
import numpy as np

P = 2**64 - 2**32 + 1
NONRESIDUE = 7
INV2 = (P + 1) // 2
PARAM_NAMES = ("log_n", "n_cols", "cap_height", "log_blowup", "arity_bits", "final_log_max", "n_queries")


def e_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def e_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def e_mul(a, b):
    return ((a[0] * b[0] + NONRESIDUE * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def e_scale(a, s):
    return (a[0] * s % P, a[1] * s % P)


def layout(p):
    """the schedule and offsets of the proof (u64 words), as tmx_fri_layout_of defines them"""
    d = p["log_n"] - p["log_blowup"]
    bits = []
    while d > p["final_log_max"]:
        b = min(p["arity_bits"], d - p["final_log_max"])
        bits.append(b)
        d -= b
    L = {"n_layers": len(bits), "final_log": d, "layer_bits": bits, "layer_cap_height": [], "off_caps": [], "off_rows": [], "off_paths": []}
    w, lg = 0, p["log_n"]
    for b in bits:
        lg -= b
        L["layer_cap_height"].append(min(p["cap_height"], lg))
        L["off_caps"].append(w)
        w += 4 << L["layer_cap_height"][-1]
    nq, nc = p["n_queries"], p["n_cols"]
    L["off_final"] = w; w += 2 << d
    L["off_indices"] = w; w += nq
    L["off_init_rows"] = w; w += nq * nc
    L["off_init_paths"] = w; w += nq * (p["log_n"] - p["cap_height"]) * 4
    lg = p["log_n"]
    for l, b in enumerate(bits):
        lg -= b
        L["off_rows"].append(w); w += nq * (2 << b)
        L["off_paths"].append(w); w += nq * (lg - L["layer_cap_height"][l]) * 4
    L["words"] = w
    return L


class Challenger:
    """the duplex of the header's transcript: observe / duplex / challenge (the LAST output word first)"""

    def __init__(self, oracle):
        self.oracle, self.state, self.inp, self.out = oracle, [0] * 12, [], []

    def observe(self, x):
        self.out = []
        self.inp.append(int(x) % P)
        if len(self.inp) == 8:
            self.duplex()

    def observe_all(self, xs):
        for x in np.asarray(xs, dtype=np.uint64).reshape(-1):
            self.observe(int(x))

    def duplex(self):
        self.state[:len(self.inp)] = self.inp
        self.inp = []
        self.state = [int(x) % P for x in self.oracle.poseidon_permute(np.array(self.state, dtype=np.uint64))[0]]
        self.out = self.state[:8]

    def challenge(self):
        if self.inp or not self.out:
            self.duplex()
        return self.out.pop()

    def ext(self):
        return (self.challenge(), self.challenge())


def fold(vals, xs, beta):
    """one radix-2 fold: vals[k] = f(xs[k]) with xs[k + h] = -xs[k]; returns the values of g at xs[k]^2 and those points"""
    h = len(vals) // 2
    out = []
    for k in range(h):
        s, d = e_add(vals[k], vals[k + h]), e_sub(vals[k], vals[k + h])
        out.append(e_scale(e_add(s, e_scale(e_mul(beta, d), pow(xs[k], P - 2, P))), INV2))
    return out, [x * x % P for x in xs[:h]]


def level_offset(log_n, lvl):
    return sum(1 << (log_n - k) for k in range(lvl))


def _path(levels, log_n, cap_height, i):
    return [int(w) for lvl in range(log_n - cap_height) for w in levels[level_offset(log_n, lvl) + ((i >> lvl) ^ 1)]]


def _start(oracle, p, cap):
    ch = Challenger(oracle)
    for name in PARAM_NAMES:
        ch.observe(p[name])
    ch.observe_all(cap)
    return ch


def _final_eval(coefs, x):
    acc = (0, 0)
    for c in reversed(coefs):
        acc = e_add(e_scale(acc, x), c)
    return acc


def prove(oracle, p, cols, shift):
    """cols: [n_cols][2^log_n] words on the coset shift <gl_root(log_n)> (the oracle's current domain).  Returns (proof words, degree_ok)."""
    L = layout(p)
    log_n, n_cols, nq = p["log_n"], p["n_cols"], p["n_queries"]
    M = 1 << log_n
    cols = np.ascontiguousarray(cols, dtype=np.uint64).reshape(n_cols, M)
    levels = oracle.poseidon_merkle(cols.reshape(-1), log_n, n_cols, p["cap_height"])
    proof = [0] * L["words"]
    ch = _start(oracle, p, levels[-(1 << p["cap_height"]):])
    alpha = ch.ext()
    apow = [(1, 0)]
    for _ in range(n_cols - 1):
        apow.append(e_mul(apow[-1], alpha))
    cv = np.array([[int(w) % P for w in col] for col in cols], dtype=object)
    f0 = list((np.array([a[0] for a in apow], dtype=object)[:, None] * cv).sum(axis=0) % P)
    f1 = list((np.array([a[1] for a in apow], dtype=object)[:, None] * cv).sum(axis=0) % P)
    vals = [(int(a), int(b)) for a, b in zip(f0, f1)]
    xs = [shift * pow(oracle.gl_root(log_n), i, P) % P for i in range(M)]
    layers = []
    lg = log_n
    for l, b in enumerate(L["layer_bits"]):
        lg -= b
        h = L["layer_cap_height"][l]
        mat = np.array([v[0] for v in vals] + [v[1] for v in vals], dtype=np.uint64)  # planar = [2a][M_(l+1)] column-major
        lv = oracle.poseidon_merkle(mat, lg, 2 << b, h)
        cap = lv[-(1 << h):].reshape(-1)
        proof[L["off_caps"][l]:L["off_caps"][l] + cap.size] = [int(w) for w in cap]
        ch.observe_all(cap)
        beta = ch.ext()
        layers.append((lg, b, h, mat, lv))
        for _ in range(b):
            vals, xs = fold(vals, xs, beta)
            beta = e_mul(beta, beta)
    ML = len(vals)
    planes = [oracle.ntt(np.array([v[k] for v in vals], dtype=np.uint64), inverse=True) for k in (0, 1)]
    s_inv = pow(xs[0], P - 2, P)  # xs[0] = s_L
    coefs = [(int(planes[0][k]) * pow(s_inv, k, P) % P, int(planes[1][k]) * pow(s_inv, k, P) % P) for k in range(ML)]
    nf = 1 << L["final_log"]
    degree_ok = all(c == (0, 0) for c in coefs[nf:])
    for k in range(nf):
        proof[L["off_final"] + 2 * k:L["off_final"] + 2 * k + 2] = coefs[k]
        ch.observe(coefs[k][0])
        ch.observe(coefs[k][1])
    idx = [ch.challenge() % M for _ in range(nq)]
    proof[L["off_indices"]:L["off_indices"] + nq] = idx
    pl0 = log_n - p["cap_height"]
    for q, i in enumerate(idx):
        proof[L["off_init_rows"] + q * n_cols:L["off_init_rows"] + (q + 1) * n_cols] = [int(w) for w in cols[:, i]]
        proof[L["off_init_paths"] + q * pl0 * 4:L["off_init_paths"] + (q + 1) * pl0 * 4] = _path(levels, log_n, p["cap_height"], i)
        for l, (lg, b, h, mat, lv) in enumerate(layers):
            r, a = i & ((1 << lg) - 1), 1 << b
            row = [int(w) for w in mat.reshape(2 * a, 1 << lg)[:, r]]
            proof[L["off_rows"][l] + q * 2 * a:L["off_rows"][l] + (q + 1) * 2 * a] = row
            pl = lg - h
            proof[L["off_paths"][l] + q * pl * 4:L["off_paths"][l] + (q + 1) * pl * 4] = _path(lv, lg, h, r)
            i = r
    return np.array(proof, dtype=np.uint64), degree_ok


def _leaf(oracle, row):
    row = [int(w) % P for w in row]
    if len(row) <= 4:
        return row + [0] * (4 - len(row))
    st = [0] * 12
    for k in range(0, len(row), 8):
        chunk = row[k:k + 8]
        st[:len(chunk)] = chunk
        st = [int(x) % P for x in oracle.poseidon_permute(np.array(st, dtype=np.uint64))[0]]
    return st[:4]


def merkle_ok(oracle, row, path, i, cap):
    cur = _leaf(oracle, row)
    path = [int(w) for w in np.asarray(path, dtype=np.uint64).reshape(-1)]
    for lvl in range(len(path) // 4):
        sib = path[4 * lvl:4 * lvl + 4]
        st = (sib + cur if (i >> lvl) & 1 else cur + sib) + [0] * 4
        cur = [int(x) % P for x in oracle.poseidon_permute(np.array(st, dtype=np.uint64))[0][:4]]
    cap = [int(w) for w in np.asarray(cap, dtype=np.uint64).reshape(-1)]
    at = 4 * (i >> (len(path) // 4))
    return cur == cap[at:at + 4]


def verify(oracle, p, cap, proof, shift):
    """[ok] per query of `proof` against the commit cap (words), on the coset shift <gl_root(log_n)>"""
    L = layout(p)
    proof = [int(w) for w in np.asarray(proof, dtype=np.uint64)]
    log_n, n_cols, nq = p["log_n"], p["n_cols"], p["n_queries"]
    ch = _start(oracle, p, cap)
    alpha = ch.ext()
    betas = []
    for l in range(L["n_layers"]):
        o = L["off_caps"][l]
        ch.observe_all(np.array(proof[o:o + (4 << L["layer_cap_height"][l])], dtype=np.uint64))
        betas.append(ch.ext())
    nf = 1 << L["final_log"]
    fin = proof[L["off_final"]:L["off_final"] + 2 * nf]
    for w in fin:
        ch.observe(w)
    coefs = [(fin[2 * k] % P, fin[2 * k + 1] % P) for k in range(nf)]
    idx = [ch.challenge() % (1 << log_n) for _ in range(nq)]
    w0 = oracle.gl_root(log_n)
    pl0 = log_n - p["cap_height"]
    res = []
    for q in range(nq):
        i = idx[q]
        ok = proof[L["off_indices"] + q] == i
        row = proof[L["off_init_rows"] + q * n_cols:L["off_init_rows"] + (q + 1) * n_cols]
        ok = merkle_ok(oracle, row, proof[L["off_init_paths"] + q * pl0 * 4:L["off_init_paths"] + (q + 1) * pl0 * 4], i, cap) and ok
        v, ap = (0, 0), (1, 0)
        for w in row:
            v = e_add(v, e_scale(ap, w % P))
            ap = e_mul(ap, alpha)
        s, w, lg = shift % P, w0, log_n
        for l, b in enumerate(L["layer_bits"]):
            a, lgn = 1 << b, lg - b
            h = L["layer_cap_height"][l]
            r, j = i & ((1 << lgn) - 1), i >> lgn
            lr = proof[L["off_rows"][l] + q * 2 * a:L["off_rows"][l] + (q + 1) * 2 * a]
            ok = ok and (lr[j] % P, lr[a + j] % P) == v
            pl = lgn - h
            o = L["off_caps"][l]
            ok = merkle_ok(oracle, lr, proof[L["off_paths"][l] + q * pl * 4:L["off_paths"][l] + (q + 1) * pl * 4], r,
                           proof[o:o + (4 << h)]) and ok
            vals = [(lr[k] % P, lr[a + k] % P) for k in range(a)]
            xs = [s * pow(w, r + k * (1 << lgn), P) % P for k in range(a)]
            beta = betas[l]
            for _ in range(b):
                vals, xs = fold(vals, xs, beta)
                beta = e_mul(beta, beta)
            v = vals[0]
            s, w, i, lg = pow(s, a, P), pow(w, a, P), r, lgn
        res.append(bool(ok and _final_eval(coefs, s * pow(w, i, P) % P) == v))
    return res
