"""A pure-Python model of the proof-of-work (grinding) variants of the FRI and DEEP proofs (include/tmx.h "proof of work"), written from the
header text and independent of libtmx.  It reuses tests/fri_model.py and tests/deep_model.py without changing them: their provers and
verifiers run as they are, over a Challenger that inserts the grinding steps (observe pow_bits, the nonce, the consumed challenge r)
between the last final coefficient and the first query index, which is where the header puts them.  The search runs the CPU oracle's
batched poseidon_permute in blocks, lowest candidate first.  The yardstick of tests/test_pow.py (not collected by pytest)."""
import contextlib

import numpy as np

import deep_model as dm
import fri_model as fm

P = fm.P
MAX_BITS, SLACK_BITS = 24, 6
GAVE_UP = 2**64 - 1
BLOCK = 4096


def proof_words(p, deep):
    """tmx_pow_proof_words for parameters that validate"""
    return fm.layout(p)["words"] + 1 + (dm.openings_words(p["n_cols"]) if deep else 0)


def observed_before_grinding(p, deep):
    """how many words the plain transcript observes up to and including the final coefficients: the seven parameters (DEEP: and the point
    count), the commit cap, (DEEP: the openings root), every layer cap, the final coefficients"""
    L = fm.layout(p)
    return 7 + (4 << p["cap_height"]) + sum(4 << h for h in L["layer_cap_height"]) + (2 << L["final_log"]) + (5 if deep else 0)


def satisfies(r, pow_bits):
    return r < 1 << (64 - pow_bits)


def candidates(oracle, ch, lo, hi):
    """r for every candidate nonce in [lo, hi) on a copy of the duplex `ch` (after observe(pow_bits)): observe(n), challenge() is ONE
    permutation of the state with the pending input words and n written over its first words; challenge() pops output word 7"""
    st = np.array(ch.state, dtype=np.uint64)
    k = len(ch.inp)
    assert k < 8
    st[:k] = ch.inp
    states = np.tile(st, (hi - lo, 1))
    states[:, k] = np.arange(lo, hi, dtype=np.uint64)
    return [int(x) % P for x in oracle.poseidon_permute(states)[:, 7]]


def search(oracle, ch, pow_bits, start=0):
    """the smallest satisfying nonce >= start, below the bound 2^(pow_bits + 6); GAVE_UP if there is none"""
    bound = 1 << (pow_bits + SLACK_BITS)
    lo = start
    while lo < bound:
        hi = min(lo + BLOCK, bound)
        for n, r in zip(range(lo, hi), candidates(oracle, ch, lo, hi)):
            if satisfies(r, pow_bits):
                return n
        lo = hi
    return GAVE_UP


_Plain = fm.Challenger


class GrindChallenger(_Plain):
    """fri_model's duplex, with the grinding steps run in front of the first challenge() that follows observation number `grind_at`.
    nonce None: search for it (the prover); else use the given word (the verifier).  Afterwards .nonce and .r hold what was used."""

    def __init__(self, oracle, pow_bits, grind_at, nonce=None):
        super().__init__(oracle)
        self.pow_bits, self.grind_at, self.nonce, self.r = pow_bits, grind_at, nonce, None
        self.n_obs, self.grinding, self.pre = 0, False, None

    def observe(self, x):
        if not self.grinding:
            self.n_obs += 1
        super().observe(x)

    def challenge(self):
        if self.r is None and not self.grinding and self.n_obs == self.grind_at:
            self.grinding = True
            self.observe(self.pow_bits)
            self.pre = _Plain(self.oracle)  # a copy of the duplex at the point of the search
            self.pre.state, self.pre.inp = list(self.state), list(self.inp)
            if self.nonce is None:
                self.nonce = search(self.oracle, self, self.pow_bits)
            self.observe(self.nonce)
            self.r = super().challenge()
            self.grinding = False
        return super().challenge()


@contextlib.contextmanager
def _transcript(pow_bits, grind_at, nonce):
    """the models' provers and verifiers build their Challenger by name: for the length of one call that name yields a GrindChallenger"""
    made = []

    def factory(oracle):
        made.append(GrindChallenger(oracle, pow_bits, grind_at, nonce))
        return made[-1]

    saved = fm.Challenger, dm.Challenger
    fm.Challenger = dm.Challenger = factory
    try:
        yield made
    finally:
        fm.Challenger, dm.Challenger = saved


def prove(oracle, p, pow_bits, deep, cols, shift):
    """Returns (proof words, degree_ok, nonce); deep: also zeta as a fourth value"""
    with _transcript(pow_bits, observed_before_grinding(p, deep), None) as made:
        out = (dm if deep else fm).prove(oracle, p, cols, shift)
    (ch,) = made
    assert ch.r is not None and ch.n_obs == ch.grind_at
    proof = np.concatenate([out[0], np.array([ch.nonce], dtype=np.uint64)])
    return (proof, out[1], ch.nonce) + tuple(out[2:])


def verify(oracle, p, pow_bits, deep, cap, proof, shift):
    """[ok] per query of the grinding proof against the commit cap (one permutation for the nonce, no search)"""
    proof = np.asarray(proof, dtype=np.uint64)
    assert proof.size == proof_words(p, deep)
    nonce = int(proof[-1])
    with _transcript(pow_bits, observed_before_grinding(p, deep), nonce) as made:
        res = (dm if deep else fm).verify(oracle, p, cap, proof[:-1], shift)
    (ch,) = made
    assert ch.r is not None
    pow_ok = nonce < P and satisfies(ch.r, pow_bits)
    return [bool(ok and pow_ok) for ok in res]


def grind_point(oracle, p, pow_bits, deep, cap, proof, shift):
    """the duplex after observe(pow_bits) as the verifier of `proof` reaches it: what candidates() and search() start from"""
    proof = np.asarray(proof, dtype=np.uint64)
    with _transcript(pow_bits, observed_before_grinding(p, deep), int(proof[-1])) as made:
        (dm if deep else fm).verify(oracle, p, cap, proof[:-1], shift)
    return made[0].pre
