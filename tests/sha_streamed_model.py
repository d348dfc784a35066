"""Pieces of the model quotients of constraint sets 3, 4 and 5 (include/tmx.h "streamed helpers of the SHA-256 sets").  A piece over the
proofs [lo, hi) of a table is gamma^(C lo) times the EXISTING model's quotient over the sub-arrays of those proofs -- the model of the
whole call, run on fewer proofs, and one constant of F_p^2.  Nothing of tests/sha_air_model.py, sha_sched_model.py or sha_init_model.py
is changed or re-derived here; the sum of the pieces of a partition of [0, n_proofs) is the whole quotient because the weights
gamma^(C p + j) = gamma^(C lo) gamma^(C (p - lo) + j) factor and the divisors do not depend on the proof."""
import numpy as np

import fri_model as fm
import sha_air_model as sm
import sha_init_model as si
import sha_sched_model as ss

P = fm.P
MODELS = {3: sm, 4: ss, 5: si}


def e_pow(g, e):
    out, base = (1, 0), g
    while e:
        if e & 1:
            out = fm.e_mul(out, base)
        base = fm.e_mul(base, base)
        e >>= 1
    return out


def scale(quot, c):
    """the planar F_p^2 column `quot` (2 M words) times the constant c of F_p^2, canonical"""
    M = len(quot) // 2
    prod = [fm.e_mul((int(quot[i]) % P, int(quot[M + i]) % P), c) for i in range(M)]
    return np.array([v[0] for v in prod] + [v[1] for v in prod], dtype=np.uint64)


def add(a, b):
    """the sum of two planar columns, canonical"""
    return np.array([(int(x) % P + int(y) % P) % P for x, y in zip(a, b)], dtype=np.uint64)


def whole(set_id, oracle, log_n, log_blowup, n_proofs, chain, cols, hcols, shift, g):
    """the existing model's quotient (set 5 alone has a mode)"""
    m = MODELS[set_id]
    if set_id == 5:
        return m.quotient(oracle, log_n, log_blowup, n_proofs, chain, cols, hcols, shift, g)
    assert chain == 0
    return m.quotient(oracle, log_n, log_blowup, n_proofs, cols, hcols, shift, g)


def piece(set_id, oracle, log_n, log_blowup, chain, lo, hi, cols, hcols, shift, g):
    """cols [9 n_proofs][M] and hcols [helper_cols n_proofs][M] of the WHOLE table; the piece of the proofs [lo, hi)"""
    m = MODELS[set_id]
    cols, hcols = np.asarray(cols).reshape(-1, 1 << log_n), np.asarray(hcols).reshape(-1, 1 << log_n)
    sub = whole(set_id, oracle, log_n, log_blowup, hi - lo, chain, cols[lo * m.WIDTH:hi * m.WIDTH], hcols[lo * m.HELPER_COLS:hi * m.HELPER_COLS],
                shift, g)
    return scale(sub, e_pow(g, m.CONSTRAINTS * lo))
