"""A pure-Python model of the mixed-size batch proof (include/tmx.h "one DEEP-FRI proof over several oracles"), written from the header text
and independent of libtmx.  It is built on tests/fri_model.py (duplex, folds, Merkle checks), tests/deep_model.py (openings by interpolation
and Horner, the planar openings section, the layer-0 quotient) and tests/pow_model.py (the nonce search), none of which it changes.  The
prover folds whole layers with the radix-2 definition and adds a group to the folded layer index for index; the verifier folds single
leaves.  The yardstick of tests/test_batch_fri.py (not collected by pytest)."""
import numpy as np

import deep_model as dm
import fri_model as fm
import pow_model as pm
from fri_model import P, e_add, e_mul, e_scale

MAX_ORACLES = 8
SCALARS = ("log_blowup", "cap_height", "arity_bits", "final_log_max", "n_queries", "pow_bits")


def bparams(log_n, n_cols, cap_height, log_blowup, arity_bits, final_log_max, n_queries, pow_bits=0):
    return dict(log_n=list(log_n), n_cols=list(n_cols), cap_height=cap_height, log_blowup=log_blowup, arity_bits=arity_bits,
                final_log_max=final_log_max, n_queries=n_queries, pow_bits=pow_bits)


def layout(p):
    """the schedule and offsets of the proof (u64 words), as tmx_batch_layout_of defines them"""
    log_n, n_cols, nq = p["log_n"], p["n_cols"], p["n_queries"]
    K = len(log_n)
    sizes = sorted(set(log_n), reverse=True)
    group = [sizes.index(m) for m in log_n]
    cap_h = [min(p["cap_height"], m) for m in log_n]
    bits, enter = [], []
    d = log_n[0] - p["log_blowup"]
    for g in range(len(sizes) - 1):
        gap = sizes[g] - sizes[g + 1]
        while gap > 0:
            b = min(p["arity_bits"], gap)
            bits.append(b)
            enter.append(0)
            gap -= b
            d -= b
        enter[-1] = g + 1
    while d > p["final_log_max"]:
        b = min(p["arity_bits"], d - p["final_log_max"])
        bits.append(b)
        enter.append(0)
        d -= b
    L = {"n_layers": len(bits), "final_log": d, "n_groups": len(sizes), "layer_bits": bits, "layer_cap_height": [], "layer_enter": enter,
         "group_of": group, "cap_height_of": cap_h, "off_open": [], "off_caps": [], "off_init_rows": [], "off_init_paths": [],
         "off_rows": [], "off_paths": []}
    w = 0
    for k in range(K):
        L["off_open"].append(w)
        w += dm.openings_words(n_cols[k])
    lg = log_n[0]
    for b in bits:
        lg -= b
        L["layer_cap_height"].append(min(p["cap_height"], lg))
        L["off_caps"].append(w)
        w += 4 << L["layer_cap_height"][-1]
    L["off_final"] = w; w += 2 << d
    L["off_indices"] = w; w += nq
    for k in range(K):
        L["off_init_rows"].append(w); w += nq * n_cols[k]
        L["off_init_paths"].append(w); w += nq * (log_n[k] - cap_h[k]) * 4
    lg = log_n[0]
    for l, b in enumerate(bits):
        lg -= b
        L["off_rows"].append(w); w += nq * (2 << b)
        L["off_paths"].append(w); w += nq * (lg - L["layer_cap_height"][l]) * 4
    L["off_nonce"] = w
    L["words"] = w + (1 if p["pow_bits"] else 0)
    return L


def _start(oracle, p, caps):
    """2^32 + K, the six scalars, the (log_n_k, n_cols_k) pairs, the word 2, the K caps; zeta drawn again while zeta.c1 == 0"""
    ch = fm.Challenger(oracle)
    ch.observe((1 << 32) + len(p["log_n"]))
    for name in SCALARS:
        ch.observe(p[name])
    for m, n in zip(p["log_n"], p["n_cols"]):
        ch.observe(m)
        ch.observe(n)
    ch.observe(2)
    for cap in caps:
        ch.observe_all(cap)
    while True:
        z = ch.ext()
        if z[1]:
            return ch, z


def _points(oracle, p, k, zeta):
    return zeta, e_scale(zeta, oracle.gl_root(p["log_n"][k] - p["log_blowup"]))


def _sub(p, k):
    return dict(log_n=p["log_n"][k], n_cols=p["n_cols"][k], log_blowup=p["log_blowup"])


def _grind(oracle, ch, pow_bits, nonce=None):
    """the proof-of-work steps 1 - 3 on the live duplex; returns (nonce, r)"""
    ch.observe(pow_bits)
    if nonce is None:
        nonce = pm.search(oracle, ch, pow_bits)
    ch.observe(nonce)
    return nonce, ch.challenge()


def _quotients(oracle, p, k, F, zs, Y, alpha_c, shift, rows=None):
    """Q_k at the rows `rows` (default: all) of oracle k's own domain s w_k^i from the values F of F_k there"""
    wk = oracle.gl_root(p["log_n"][k])
    rows = range(1 << p["log_n"][k]) if rows is None else rows
    return [dm.layer0(f, shift * pow(wk, i, P) % P, zs, Y, alpha_c) for f, i in zip(F, rows)]


def prove(oracle, p, cols, shift):
    """cols[k]: [n_cols_k][2^log_n_k] words on the coset shift <gl_root(log_n_k)>.  Returns (proof words, degree_ok, zeta, nonce or None)."""
    L = layout(p)
    K, nq, B = len(p["log_n"]), p["n_queries"], 1 << p["log_blowup"]
    C = sum(p["n_cols"])
    cols = [np.ascontiguousarray(c, dtype=np.uint64).reshape(p["n_cols"][k], 1 << p["log_n"][k]) for k, c in enumerate(cols)]
    levels = [oracle.poseidon_merkle(cols[k].reshape(-1), p["log_n"][k], p["n_cols"][k], L["cap_height_of"][k]) for k in range(K)]
    ch, zeta = _start(oracle, p, [levels[k][-(1 << L["cap_height_of"][k]):] for k in range(K)])
    proof = [0] * L["words"]
    ys, secs = [], []
    for k in range(K):
        ys.append(dm.evaluate(oracle, cols[k][:, ::B], shift, _points(oracle, p, k, zeta)))
        secs.append(dm.openings_section(ys[k], p["n_cols"][k]))
        proof[L["off_open"][k]:L["off_open"][k] + secs[k].size] = [int(w) for w in secs[k]]
    for k in range(K):
        ch.observe_all(dm.openings_root(oracle, _sub(p, k), secs[k]))
    alpha = ch.ext()
    apow = [(1, 0)]
    for _ in range(C):
        apow.append(e_mul(apow[-1], alpha))
    Q = [None] * L["n_groups"]
    off = 0
    for k in range(K):
        n = p["n_cols"][k]
        ap = apow[off:off + n]
        cv = np.array([[int(w) % P for w in col] for col in cols[k]], dtype=object)
        f0 = (np.array([a[0] for a in ap], dtype=object)[:, None] * cv).sum(axis=0) % P
        f1 = (np.array([a[1] for a in ap], dtype=object)[:, None] * cv).sum(axis=0) % P
        Y = [(0, 0), (0, 0)]
        for c, y in enumerate(ys[k]):
            Y = [e_add(Y[j], e_mul(ap[c], y[j])) for j in (0, 1)]
        q = _quotients(oracle, p, k, [(int(a), int(b)) for a, b in zip(f0, f1)], _points(oracle, p, k, zeta), Y, apow[C], shift)
        g = L["group_of"][k]
        Q[g] = q if Q[g] is None else [e_add(a, b) for a, b in zip(Q[g], q)]
        off += n
    vals = Q[0]
    xs = [shift * pow(oracle.gl_root(p["log_n"][0]), i, P) % P for i in range(1 << p["log_n"][0])]
    layers = []
    lg = p["log_n"][0]
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
            vals, xs = fm.fold(vals, xs, beta)
            beta = e_mul(beta, beta)
        if L["layer_enter"][l]:  # (beta is beta_l^(a_l) here: the first power the fold did not use)
            vals = [e_add(v, e_mul(beta, q)) for v, q in zip(vals, Q[L["layer_enter"][l]])]
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
    nonce = None
    if p["pow_bits"]:
        nonce, _ = _grind(oracle, ch, p["pow_bits"])
        proof[L["off_nonce"]] = nonce
    idx = [ch.challenge() % (1 << p["log_n"][0]) for _ in range(nq)]
    proof[L["off_indices"]:L["off_indices"] + nq] = idx
    for q, i0 in enumerate(idx):
        for k in range(K):
            n, m, h = p["n_cols"][k], p["log_n"][k], L["cap_height_of"][k]
            i, pl = i0 % (1 << m), m - h
            proof[L["off_init_rows"][k] + q * n:L["off_init_rows"][k] + (q + 1) * n] = [int(w) for w in cols[k][:, i]]
            proof[L["off_init_paths"][k] + q * pl * 4:L["off_init_paths"][k] + (q + 1) * pl * 4] = fm._path(levels[k], m, h, i)
        i = i0
        for l, (lg, b, h, mat, lv) in enumerate(layers):
            r, a = i & ((1 << lg) - 1), 1 << b
            proof[L["off_rows"][l] + q * 2 * a:L["off_rows"][l] + (q + 1) * 2 * a] = [int(w) for w in mat.reshape(2 * a, 1 << lg)[:, r]]
            pl = lg - h
            proof[L["off_paths"][l] + q * pl * 4:L["off_paths"][l] + (q + 1) * pl * 4] = fm._path(lv, lg, h, r)
            i = r
    return np.array(proof, dtype=np.uint64), degree_ok, zeta, nonce


def openings_of(p, proof, k):
    """[(y0, y1)] per column of oracle k, words taken mod p"""
    o = layout(p)["off_open"][k]
    return dm.openings_of(_sub(p, k), np.asarray(proof, dtype=np.uint64)[o:])


def verify(oracle, p, caps, proof, shift):
    """[ok] per query against the K caps (a list of word arrays, or their concatenation)"""
    L = layout(p)
    K, nq = len(p["log_n"]), p["n_queries"]
    C = sum(p["n_cols"])
    if not isinstance(caps, (list, tuple)):
        flat, caps, at = np.asarray(caps, dtype=np.uint64).reshape(-1), [], 0
        for k in range(K):
            caps.append(flat[at:at + (4 << L["cap_height_of"][k])])
            at += 4 << L["cap_height_of"][k]
    raw = np.asarray(proof, dtype=np.uint64)
    assert raw.size == L["words"]
    proof = [int(w) for w in raw]
    ch, zeta = _start(oracle, p, caps)
    all_ok = True
    ys = []
    for k in range(K):
        n, o = p["n_cols"][k], L["off_open"][k]
        R = 1 << dm.log_r(n)
        sec = raw[o:o + 4 * R]
        all_ok = all_ok and not any(int(sec[j * R + r]) for j in range(4) for r in range(n, R))
        ch.observe_all(dm.openings_root(oracle, _sub(p, k), sec))
        ys.append(dm.openings_of(_sub(p, k), sec))
    alpha = ch.ext()
    apow = [(1, 0)]
    for _ in range(C):
        apow.append(e_mul(apow[-1], alpha))
    offs = [sum(p["n_cols"][:k]) for k in range(K)]
    Y = []
    for k in range(K):
        y = [(0, 0), (0, 0)]
        for c, yc in enumerate(ys[k]):
            y = [e_add(y[j], e_mul(apow[offs[k] + c], yc[j])) for j in (0, 1)]
        Y.append(y)
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
    if p["pow_bits"]:
        nonce = proof[L["off_nonce"]]
        _, r = _grind(oracle, ch, p["pow_bits"], nonce)
        all_ok = all_ok and nonce < P and pm.satisfies(r, p["pow_bits"])
    idx = [ch.challenge() % (1 << p["log_n"][0]) for _ in range(nq)]
    res = []
    for q in range(nq):
        i = idx[q]
        ok = all_ok and proof[L["off_indices"] + q] == i
        Q = [(0, 0)] * L["n_groups"]
        for k in range(K):
            n, m, h = p["n_cols"][k], p["log_n"][k], L["cap_height_of"][k]
            ik, pl = i % (1 << m), m - h
            row = proof[L["off_init_rows"][k] + q * n:L["off_init_rows"][k] + (q + 1) * n]
            path = proof[L["off_init_paths"][k] + q * pl * 4:L["off_init_paths"][k] + (q + 1) * pl * 4]
            ok = fm.merkle_ok(oracle, row, path, ik, caps[k]) and ok
            F = (0, 0)
            for c, w in enumerate(row):
                F = e_add(F, e_scale(apow[offs[k] + c], w % P))
            g = L["group_of"][k]
            Q[g] = e_add(Q[g], _quotients(oracle, p, k, [F], _points(oracle, p, k, zeta), Y[k], apow[C], shift, [ik])[0])
        v = Q[0]
        s, w, lg = shift % P, oracle.gl_root(p["log_n"][0]), p["log_n"][0]
        for l, b in enumerate(L["layer_bits"]):
            a, lgn = 1 << b, lg - b
            h = L["layer_cap_height"][l]
            r, j = i & ((1 << lgn) - 1), i >> lgn
            lr = proof[L["off_rows"][l] + q * 2 * a:L["off_rows"][l] + (q + 1) * 2 * a]
            ok = ok and (lr[j] % P, lr[a + j] % P) == v
            pl = lgn - h
            o = L["off_caps"][l]
            ok = fm.merkle_ok(oracle, lr, proof[L["off_paths"][l] + q * pl * 4:L["off_paths"][l] + (q + 1) * pl * 4], r, proof[o:o + (4 << h)]) and ok
            vals = [(lr[k] % P, lr[a + k] % P) for k in range(a)]
            xs = [s * pow(w, r + k * (1 << lgn), P) % P for k in range(a)]
            beta = betas[l]
            for _ in range(b):
                vals, xs = fm.fold(vals, xs, beta)
                beta = e_mul(beta, beta)
            v = vals[0]
            if L["layer_enter"][l]:
                v = e_add(v, e_mul(beta, Q[L["layer_enter"][l]]))
            s, w, i, lg = pow(s, a, P), pow(w, a, P), r, lgn
        res.append(bool(ok and fm._final_eval(coefs, s * pow(w, i, P) % P) == v))
    return res
