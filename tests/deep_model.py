"""A pure-Python model of the DEEP proof (include/tmx.h "out-of-domain openings"), written from the mathematics of the header and independent
of libtmx.  It reuses tests/fri_model.py's helpers (Challenger, fold, layout, merkle_ok, _path, _final_eval) without changing them.  The
openings are computed independently of the barycentric form the device uses: an inverse NTT of the subset (oracle.ntt), coefficient k times
s^-k, then Horner in F_p^2.  The yardstick of tests/test_deep.py (not collected by pytest)."""
import numpy as np

from fri_model import (P, PARAM_NAMES, Challenger, _final_eval, _path, e_add, e_mul, e_scale, e_sub, fold, layout,  # noqa: F401
                       merkle_ok)

MAX_COLS = 1 << 24


def log_r(n_cols):
    return max(0, (n_cols - 1).bit_length())


def openings_words(n_cols):
    """tmx_deep_openings_words"""
    return 0 if n_cols == 0 or n_cols > MAX_COLS else 4 << log_r(n_cols)


def proof_words(p):
    return openings_words(p["n_cols"]) + layout(p)["words"]


def e_inv(a):
    n = (a[0] * a[0] - 7 * a[1] * a[1]) % P
    ni = pow(n, P - 2, P)
    return (a[0] * ni % P, -a[1] * ni % P)


def e_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = e_mul(r, a)
        a = e_mul(a, a)
        e >>= 1
    return r


def _canon(a):
    a = np.asarray(a, dtype=np.uint64)
    return np.where(a >= np.uint64(P), a - np.uint64(P), a)


def _start(oracle, p, cap):
    """the DEEP start: parameters, the point count 2, the commit cap; zeta drawn again while zeta.c1 == 0"""
    ch = Challenger(oracle)
    for name in PARAM_NAMES:
        ch.observe(p[name])
    ch.observe(2)
    ch.observe_all(cap)
    while True:
        z = ch.ext()
        if z[1]:
            return ch, z


def points(oracle, p, zeta):
    """z_0 = zeta, z_1 = zeta omega_N"""
    omega = oracle.gl_root(p["log_n"] - p["log_blowup"])
    return zeta, e_scale(zeta, omega)


def evaluate(oracle, sub, s, zs):
    """sub: [n_cols][N] words, the values of each column on s <omega_N>; returns [n_cols][len(zs)] values in F_p^2 of the polynomial of degree
    < N through them: inverse NTT, coefficient k times s^-k, Horner (vectorized over the columns)"""
    sub = _canon(np.atleast_2d(sub))
    n_cols, N = sub.shape
    coef = np.array(oracle.ntt(sub, inverse=True), dtype=object).reshape(n_cols, N)
    s_inv = pow(s % P, P - 2, P)
    scale = np.array([pow(s_inv, k, P) for k in range(N)], dtype=object)
    coef = coef * scale[None, :] % P
    out = []
    for z in zs:
        a0 = np.zeros(n_cols, dtype=object)
        a1 = np.zeros(n_cols, dtype=object)
        for k in range(N - 1, -1, -1):
            a0, a1 = (a0 * z[0] + 7 * a1 * z[1] + coef[:, k]) % P, (a0 * z[1] + a1 * z[0]) % P
        out.append([(int(x), int(y)) for x, y in zip(a0, a1)])
    return [list(t) for t in zip(*out)]


def openings_section(ys, n_cols):
    """the planar section: y_(.,0).c0, y_(.,0).c1, y_(.,1).c0, y_(.,1).c1, R rows each, zero padding"""
    R = 1 << log_r(n_cols)
    sec = np.zeros(4 * R, dtype=np.uint64)
    for c, (y0, y1) in enumerate(ys):
        sec[c], sec[R + c], sec[2 * R + c], sec[3 * R + c] = y0[0], y0[1], y1[0], y1[1]
    return sec


def openings_of(p, proof):
    """[(y0, y1)] per column, words taken mod p, from a proof's openings section"""
    R = 1 << log_r(p["n_cols"])
    w = [int(x) % P for x in np.asarray(proof, dtype=np.uint64)[:4 * R]]
    return [((w[c], w[R + c]), (w[2 * R + c], w[3 * R + c])) for c in range(p["n_cols"])]


def openings_root(oracle, p, section):
    return oracle.poseidon_merkle(_canon(section), log_r(p["n_cols"]), 4, 0)[-1]


def _ysum(ys, alpha, k):
    acc, ap = (0, 0), (1, 0)
    for y in ys:
        acc = e_add(acc, e_mul(ap, y[k]))
        ap = e_mul(ap, alpha)
    return acc, ap


def layer0(F, x, zs, Y, alpha_n):
    """(F - Y_0) / (x - z_0) + alpha^n (F - Y_1) / (x - z_1)"""
    q0 = e_mul(e_sub(F, Y[0]), e_inv(((x - zs[0][0]) % P, -zs[0][1] % P)))
    q1 = e_mul(e_sub(F, Y[1]), e_inv(((x - zs[1][0]) % P, -zs[1][1] % P)))
    return e_add(q0, e_mul(alpha_n, q1))


def prove(oracle, p, cols, shift):
    """cols: [n_cols][2^log_n] words on the coset shift <gl_root(log_n)> (the oracle's current domain).  Returns (proof words, degree_ok,
    zeta)."""
    L = layout(p)
    log_n, n_cols, nq = p["log_n"], p["n_cols"], p["n_queries"]
    M, B = 1 << log_n, 1 << p["log_blowup"]
    cols = np.ascontiguousarray(cols, dtype=np.uint64).reshape(n_cols, M)
    levels = oracle.poseidon_merkle(cols.reshape(-1), log_n, n_cols, p["cap_height"])
    ch, zeta = _start(oracle, p, levels[-(1 << p["cap_height"]):])
    zs = points(oracle, p, zeta)
    ys = evaluate(oracle, cols[:, ::B], shift, zs)
    sec = openings_section(ys, n_cols)
    ch.observe_all(openings_root(oracle, p, sec))
    alpha = ch.ext()
    Y0, _ = _ysum(ys, alpha, 0)
    Y1, alpha_n = _ysum(ys, alpha, 1)
    apow = [(1, 0)]
    for _ in range(n_cols - 1):
        apow.append(e_mul(apow[-1], alpha))
    cv = np.array([[int(w) % P for w in col] for col in cols], dtype=object)
    f0 = list((np.array([a[0] for a in apow], dtype=object)[:, None] * cv).sum(axis=0) % P)
    f1 = list((np.array([a[1] for a in apow], dtype=object)[:, None] * cv).sum(axis=0) % P)
    xs = [shift * pow(oracle.gl_root(log_n), i, P) % P for i in range(M)]
    vals = [layer0((int(a), int(b)), x, zs, (Y0, Y1), alpha_n) for a, b, x in zip(f0, f1, xs)]
    proof = [0] * L["words"]
    layers = []
    lg = log_n
    for l, b in enumerate(L["layer_bits"]):
        lg -= b
        h = L["layer_cap_height"][l]
        mat = np.array([v[0] for v in vals] + [v[1] for v in vals], dtype=np.uint64)
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
    s_inv = pow(xs[0], P - 2, P)
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
            proof[L["off_rows"][l] + q * 2 * a:L["off_rows"][l] + (q + 1) * 2 * a] = [int(w) for w in mat.reshape(2 * a, 1 << lg)[:, r]]
            pl = lg - h
            proof[L["off_paths"][l] + q * pl * 4:L["off_paths"][l] + (q + 1) * pl * 4] = _path(lv, lg, h, r)
            i = r
    return np.concatenate([sec, np.array(proof, dtype=np.uint64)]), degree_ok, zeta


def verify(oracle, p, cap, proof, shift):
    """[ok] per query of the DEEP proof against the commit cap (words), on the coset shift <gl_root(log_n)>"""
    L = layout(p)
    log_n, n_cols, nq = p["log_n"], p["n_cols"], p["n_queries"]
    R = 1 << log_r(n_cols)
    raw = np.asarray(proof, dtype=np.uint64)
    sec = raw[:4 * R]
    pad_ok = not any(int(sec[k * R + r]) for k in range(4) for r in range(n_cols, R))
    proof = [int(w) for w in raw[4 * R:]]
    ch, zeta = _start(oracle, p, cap)
    zs = points(oracle, p, zeta)
    ch.observe_all(openings_root(oracle, p, sec))
    alpha = ch.ext()
    ys = openings_of(p, raw)
    Y0, _ = _ysum(ys, alpha, 0)
    Y1, alpha_n = _ysum(ys, alpha, 1)
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
        ok = pad_ok and proof[L["off_indices"] + q] == i
        row = proof[L["off_init_rows"] + q * n_cols:L["off_init_rows"] + (q + 1) * n_cols]
        ok = merkle_ok(oracle, row, proof[L["off_init_paths"] + q * pl0 * 4:L["off_init_paths"] + (q + 1) * pl0 * 4], i, cap) and ok
        v, ap = (0, 0), (1, 0)
        for w in row:
            v = e_add(v, e_scale(ap, w % P))
            ap = e_mul(ap, alpha)
        v = layer0(v, shift * pow(w0, i, P) % P, zs, (Y0, Y1), alpha_n)
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
