"""The set-6 kernels (tendermintx_amd/csrc/air.hip k_air_sha_public_gather, k_air_link_helper, k_air_link_tables, k_air_link_combine,
k_air_link_fold, k_air_link_quotient<FORM>, k_air_link_check; poseidon.hip k_air_link_gamma) at every shape and row value they branch on:
the gather's SHA padding at every length the packed records can hold, its tree walk at odd N and two validator sets, every offset of its
geometry on rows of random bits, more than two workgroups; the gather against the trace writer's own padding on edited records; the
verifier's barycentric sums at K = 256, 512 and 4096; blow-up 64; pieces that start at proof 256 and above; public words at or above p;
the set-level call on a skip section and beside sets 3 and 4.  The yardsticks stay tests/sha_public_model.py on tests/batch_model.py and
hashlib: device words equal the model's word for word, every device verdict equals the model verifier's, guard words stay intact.  The
helpers and fixtures are those of tests/test_sha_public.py, tests/test_sha_air.py and tests/test_sha_air_shapes.py; docs/kernels.md "set 6:
which test reaches which shape" is the map."""
import hashlib
import os
import re

import numpy as np
import pytest

import batch_model as bm
import fri_model as fm
import sha_air_model as sm
import sha_public_model as sp
import sha_sched_model as ss
import test_sha_air as tsa
import test_sha_public as tsp
import test_sha_sched as tss
from test_fri import _down, _sentinel, _shift, _up
from test_merkle_open import _section_geom
from test_sha_air import ctx  # noqa: F401  (a fixture)
from test_sha_air import _guarded, _random_ext, _tree
from test_sha_air_shapes import _bumped
from test_sha_public import skip4, step3  # noqa: F401  (fixtures)

P = fm.P
SHA256, TREE, HEADER = 4, 16, 32
H3, Q3, H4, Q4, H6, Q6 = 128, 256, 512, 1024, 8192, 16384
W, PW, HC = sp.WIDTH, sp.PUB_WIDTH, sp.HELPER_COLS
CID, CAP_H = tsp.CID, tsp.CAP_H
HERE = os.path.dirname(os.path.abspath(__file__))
M32 = 0xFFFFFFFF


# ---- a plain SHA-256 compression, written here: the check of the gathered blocks that does not go through the model's padding
K256 = [0x428A2F98, 0x71374491, 0xB5C0FBCF, 0xE9B5DBA5, 0x3956C25B, 0x59F111F1, 0x923F82A4, 0xAB1C5ED5, 0xD807AA98, 0x12835B01, 0x243185BE,
        0x550C7DC3, 0x72BE5D74, 0x80DEB1FE, 0x9BDC06A7, 0xC19BF174, 0xE49B69C1, 0xEFBE4786, 0x0FC19DC6, 0x240CA1CC, 0x2DE92C6F, 0x4A7484AA,
        0x5CB0A9DC, 0x76F988DA, 0x983E5152, 0xA831C66D, 0xB00327C8, 0xBF597FC7, 0xC6E00BF3, 0xD5A79147, 0x06CA6351, 0x14292967, 0x27B70A85,
        0x2E1B2138, 0x4D2C6DFC, 0x53380D13, 0x650A7354, 0x766A0ABB, 0x81C2C92E, 0x92722C85, 0xA2BFE8A1, 0xA81A664B, 0xC24B8B70, 0xC76C51A3,
        0xD192E819, 0xD6990624, 0xF40E3585, 0x106AA070, 0x19A4C116, 0x1E376C08, 0x2748774C, 0x34B0BCB5, 0x391C0CB3, 0x4ED8AA4A, 0x5B9CCA4F,
        0x682E6FF3, 0x748F82EE, 0x78A5636F, 0x84C87814, 0x8CC70208, 0x90BEFFFA, 0xA4506CEB, 0xBEF9A3F7, 0xC67178F2]


def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def _compress(state, words):
    w = [int(x) for x in words]
    assert len(w) == 16 and max(w) <= M32
    for t in range(16, 64):
        s0 = _rotr(w[t - 15], 7) ^ _rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = _rotr(w[t - 2], 17) ^ _rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & M32)
    a, b, c, d, e, f, g, h = state
    for t in range(64):
        t1 = (h + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & g & M32)) + K256[t] + w[t]) & M32
        t2 = ((_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        a, b, c, d, e, f, g, h = (t1 + t2) & M32, a, b, c, (d + t1) & M32, e, f, g
    return [(x + y) & M32 for x, y in zip(state, (a, b, c, d, e, f, g, h))]


def test_the_map_names_tests_that_exist():
    """every test id of this file that docs/kernels.md names is a test of this file, and every GPU test of this file is named there"""
    text = open(os.path.join(HERE, "..", "docs", "kernels.md")).read()
    named = set(re.findall(r"test_sha_public_shapes\.py::(test_\w+)", text))
    assert len(named) >= 10
    here = {k for k, v in globals().items() if k.startswith("test_") and callable(v)}
    assert named <= here, named - here
    gpu = {k for k in here if any(m.name == "gpu" for m in getattr(globals()[k], "pytestmark", []))}
    assert gpu <= named, gpu - named


# ---- A: the gather on crafted element rows
VLENS = (0, 1, 45, 46, 47, 255)  # validator_byte_length: a u8 of the packed record; the message is 00 | min(vlen, 46) bytes
ENC_LENS = (0, 1, 10, 11, 52, 53, 54, 55, 56, 62, 63, 64, 78, 79, 80, (1 << 32) - 1)  # u32 fields; the leaf is min(len, 79) + 1 bytes
SHAPES = [(1, 2), (0, 5), (1, 6), (1, 7), (0, 9)]  # (kind, n)


def _crafted_rows(lib, kind, n, n_proofs, seed):
    """[n_proofs][elem_stride] element rows of random bits -- a wrong offset reads other bytes -- with the length elements set: every H.2
    lane's (and, skip, every H.4 lane's) validator_byte_length from VLENS, shifted per lane, the encoded chain-id and height lengths from
    ENC_LENS in two phases.  All inside what the packed record holds (u8, u32)"""
    stride = int(lib.tmx_elem_stride(kind, n))
    L = sp.Layout(kind, n)
    assert stride >= L.d5_proof[-1] + 256 * 5
    rows = np.random.default_rng(seed).integers(0, 2, (n_proofs, stride), dtype=np.uint64)
    for p in range(n_proofs):
        for i in range(n):
            rows[p, L.h2 + 1517 * i + 1515] = VLENS[(p + i) % 6]
            if kind == 0:
                rows[p, L.h4 + 259 * i + 258] = VLENS[(p + 2 * i + 3) % 6]
        rows[p, L.cid_len] = ENC_LENS[p % 16]
        rows[p, L.h_len] = ENC_LENS[(p + 5) % 16]
    return rows


def _check_table(kind, n, sec, rows, pub):
    """what every public table must satisfy whoever built it, independently of the model's padding: per hash with a message the blocks,
    compressed with _compress from the IV -- block 0 where new is set, block 1 where chn is set -- give hashlib.sha256(message); the
    digest columns hold the row's 32 digest bytes on the last live block only; a zero hash is all zero.  Returns the counts (hashes
    compressed, two-block hashes, two-block leaves among the variable-length leaves, promoted slots, zero blocks)"""
    n_hash = n_two = n_two_leaf = n_promoted = 0
    K = pub.shape[1]
    for p, row in enumerate(rows):
        u = pub[p * PW:(p + 1) * PW]
        hashes, per = sp.section_hashes(kind, n, sec, row)
        msgs = sp.messages(kind, n, sec, row)
        assert len(hashes) == len(msgs) and per * len(msgs) <= K
        for i, m in enumerate(msgs):
            blocks = u[:, per * i:per * i + per]
            if m is None:
                n_promoted += 1
                assert not blocks.any(), (sec, p, i)
                continue
            two = len(m) + 9 > 64
            assert two <= (per == 2)
            assert int(blocks[sp.PW_NEW, 0]) == 1 and int(blocks[sp.PW_CHN, 0]) == 0, (sec, p, i)
            state = _compress(sp.IV, blocks[sp.PW_W:sp.PW_W + 16, 0])
            if per == 2:
                assert int(blocks[sp.PW_NEW, 1]) == 0 and int(blocks[sp.PW_CHN, 1]) == int(two), (sec, p, i, len(m))
                if blocks[sp.PW_CHN, 1]:
                    state = _compress(state, blocks[sp.PW_W:sp.PW_W + 16, 1])
                else:
                    assert not blocks[:, 1].any(), (sec, p, i)
            assert b"".join(x.to_bytes(4, "big") for x in state) == hashlib.sha256(m).digest(), (sec, p, i, len(m))
            last = int(two)
            assert [int(x) for x in blocks[sp.PW_DIG:sp.PW_DIG + 8, last]] == hashes[i][1], (sec, p, i)
            assert two == 0 or not blocks[sp.PW_DIG:sp.PW_DIG + 8, 0].any(), (sec, p, i)
            n_hash, n_two = n_hash + 1, n_two + int(two)
            if sec == HEADER and i % 5 == 0 and i // 5 < 2:
                n_two_leaf += int(two)
        assert not u[:, per * len(msgs):].any()
    live = pub[sp.PW_NEW::PW] + pub[sp.PW_CHN::PW]
    assert int(live.max()) == 1
    return n_hash, n_two, n_two_leaf, n_promoted, int((live == 0).sum())


def _check_counts(kind, n, sec, n_proofs, log_k, counts):
    """the case did not pass by having nothing to check"""
    n_hash, n_two, n_two_leaf, n_promoted, n_zero = counts
    assert n_hash > 0
    if sec == HEADER:  # the leaf lengths 56 .. 80 take two blocks, and so do the path nodes
        assert n_two_leaf >= (6 if n_proofs >= 16 else 1) and n_two > n_two_leaf
    if sec == TREE:
        odd_levels, sz = 0, n
        while sz > 1:
            odd_levels, sz = odd_levels + sz % 2, (sz + 1) // 2
        assert n_two == n_hash and n_promoted == (2 if kind == 0 else 1) * odd_levels * n_proofs
        assert (n_promoted > 0) == (n in (5, 6, 7, 9))
    if sec == SHA256:
        assert n_two == 0
    assert (n_zero > 0) == ((n_proofs << log_k) > n_hash + n_two)
    assert sec != TREE or n == 2 or n_zero > 0


def _log_k(lib, kind, sec, n, n_proofs):
    from tendermintx_amd.context import air_sha256_public_shape
    log_k, n_cols = air_sha256_public_shape(kind, sec, n, n_proofs, lib)
    assert n_cols == PW * n_proofs
    return log_k


@pytest.mark.parametrize("kind,n", SHAPES)
def test_model_table_of_crafted_rows_hashes_to_hashlib(built_lib, kind, n):
    """the CPU twin of test_gather_of_crafted_rows_equals_the_model, with the model's table in place of the device's: seventeen rows of
    random bits per (kind, N), every validator_byte_length of {0, 1, 45, 46, 47, 255} and every encoded length of {0, 1, 10, 11, 52 .. 56,
    62 .. 64, 78 .. 80, 2^32 - 1}: every hash of T.3, T.5 and T.6 compresses to hashlib's digest of the reassembled message -- the
    two-block leaf from length 55 on, 0x80 on the last byte of block 0 (63) and on the first of block 1 (64), the exact fit at 55 (the
    leaf is then 56 bytes: two blocks; 54 gives the 55-byte one-block fit), the clamps at 46 and 79, lengths 0 and 1.  A length element above
    its field's range (u8, u32) is not crafted: the kernel takes the low 32 bits of the element and the model the whole word, and no
    witness produces such a row, so nothing is asserted there"""
    n_proofs, total = 17, [0, 0]
    rows = _crafted_rows(built_lib, kind, n, n_proofs, 17000 + 10 * n + kind)
    for sec in (SHA256, TREE, HEADER):
        log_k = _log_k(built_lib, kind, sec, n, n_proofs)
        counts = _check_table(kind, n, sec, rows, sp.public_table(kind, n, sec, list(rows), log_k))
        _check_counts(kind, n, sec, n_proofs, log_k, counts)
        total = [total[0] + counts[0], total[1] + counts[1]]
    print(f"\n[sha-link shapes] kind {kind}, N = {n}: {total[0]} hashes against hashlib, {total[1]} of them two-block")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,n_proofs", [(k, n, 17) for k, n in SHAPES] + [(1, 2, 257)])
def test_gather_of_crafted_rows_equals_the_model(built_lib, kind, n, n_proofs):
    """tmx_air_sha256_public_device on the crafted rows of the CPU twin (the call takes any row pointer): all three sections of step N = 2,
    6, 7 and skip N = 5, 9 -- promoted slots at several levels, two validator sets beside an odd N -- with 17 proofs, and T.3 of step N = 2
    with 257 proofs (514 lanes: a partly filled third workgroup).  Every word equals sp.public_table's, guard words intact; and the same
    independent checks as the twin on the DEVICE's words: _compress of the gathered blocks is hashlib's digest of the message, the digest
    columns are the row's digest bytes on the last live block only; two-block leaves, promoted slots and zero blocks occur where the
    shape has them.  Every offset of AirShaPublicGeom is read inside random bits: a wrong one gives other bytes.  (A length element above
    u8 / u32 is not crafted, as the twin's docstring says)"""
    import tendermintx_amd as tmx
    rows = _crafted_rows(built_lib, kind, n, n_proofs, 17000 + 10 * n + kind)
    with tmx.Context(n, CID, max_batch=2) as c:
        assert c.elem_stride(kind) == rows.shape[1]
        d_rows = _up(rows.reshape(-1))
        for sec in ((SHA256,) if n_proofs == 257 else (SHA256, TREE, HEADER)):
            log_k, _ = c.air_sha256_public_shape(kind, sec, n_proofs)
            _, got = tsp._gather(c, kind, sec, n_proofs, d_rows)
            want = sp.public_table(kind, n, sec, list(rows), log_k)
            assert got.shape == want.shape == (PW * n_proofs, 1 << log_k)
            assert np.array_equal(got, want), (sec, np.argwhere(got != want)[:10])
            _check_counts(kind, n, sec, n_proofs, log_k, _check_table(kind, n, sec, rows, got))


# ---- B: the gather against the trace writer on edited records
EDITED_LENS = (54, 55, 56, 63, 64, 79, 80, 255)
PR_STRIDE, PR_OFF_HDR_A, VR_STRIDE, VR_OFF_VLEN, HR_STRIDE, HR_OFF_VLEN = 2336, 64, 256, 222, 48, 40  # csrc/layout.h, include/tmx.h


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [(0, 4), (1, 3)])
def test_gather_equals_the_trace_writer_on_edited_records(built_lib, kind, n):
    """the two independent padding codes against each other where they can differ: k_air_sha_public_gather (from the element rows) and
    k_trace_sha256 / k_trace_sha256x2 (from the packed records and the Level-1 scratch).  Eight proofs of a synthetic batch with the packed
    records raw-edited before upload: the encoded chain-id and height lengths of header A (leaf_len[1], leaf_len[2]: the bytes k_proof
    copies to PF_OFF_CIDLEN and PF_OFF_HLEN) become 54, 55, 56, 63, 64, 79, 80 and 255, one per proof, the two in different phases; the
    validator_byte_length of some lanes (VR_OFF_VLEN, skip: HR_OFF_VLEN) becomes 0, 47 and 255.  (The packed field is a u8: 255 is the
    largest value above the clamp that a record can hold, 300 does not fit.)  tmx_witness_batch_device and tmx_trace_rows_device as
    test_air_boundary._witness_rows runs them; the verdicts fail on chain id, height or sign-bytes and are not asserted.  The gathered
    w[k][t] is the W of row 64 k + t of the device's trace rows, new + chn their liveness, in all three sections; the element rows carry
    the edited lengths; and the table is the model's"""
    import torch
    import tendermintx_amd as tmx
    from tendermintx_amd.synth import Workload
    n_proofs = 8
    wl = Workload(kind, n, n_proofs, n, chain_id=CID, seed=17500 + n, signed_permille=900)
    proofs, targets = bytearray(wl.proofs), bytearray(wl.targets)
    trusteds = bytearray(wl.trusteds) if kind == 0 else None
    vl = (0, 47, 255)
    for p in range(n_proofs):
        proofs[p * PR_STRIDE + PR_OFF_HDR_A + 1] = EDITED_LENS[p]
        proofs[p * PR_STRIDE + PR_OFF_HDR_A + 2] = EDITED_LENS[(p + 3) % 8]
        targets[(p * n + p % n) * VR_STRIDE + VR_OFF_VLEN] = vl[p % 3]
        if kind == 0:
            trusteds[(p * n + (p + 1) % n) * HR_STRIDE + HR_OFF_VLEN] = vl[(p + 1) % 3]
    dev = tsa._dev()
    d = [torch.frombuffer(b, dtype=torch.uint8).to(dev) if b is not None else None for b in (proofs, targets, trusteds)]
    r = d[2].data_ptr() if d[2] is not None else None
    with tmx.Context(n, CID, max_batch=n_proofs) as c:
        d_rows = torch.zeros((n_proofs, c.elem_stride(kind)), dtype=torch.int64, device=dev)
        rep = torch.zeros(n_proofs * 64, dtype=torch.uint8, device=dev)
        c.witness_batch_device(kind, n_proofs, d[0].data_ptr(), d[1].data_ptr(), r, d_rows.data_ptr(), rep.data_ptr(), 0)
        d_trace = torch.zeros((n_proofs, c.trace_elem_count(kind)), dtype=torch.int64, device=dev)
        c.trace_rows_device(kind, n_proofs, d[1].data_ptr(), r, d_trace.data_ptr(), 63, 0)
        torch.cuda.synchronize(dev)
        rows, trace = _down(d_rows).reshape(n_proofs, -1), _down(d_trace).reshape(n_proofs, -1)
        L = sp.Layout(kind, n)
        assert [int(x) for x in rows[:, L.cid_len]] == list(EDITED_LENS)  # (the witness call neither refuses nor ignores the edits)
        assert [int(x) for x in rows[:, L.h_len]] == [EDITED_LENS[(p + 3) % 8] for p in range(n_proofs)]
        assert [int(rows[p, L.h2 + 1517 * (p % n) + 1515]) for p in range(n_proofs)] == [vl[p % 3] for p in range(n_proofs)]
        n_two_leaf = 0
        for sec in (SHA256, TREE, HEADER):
            _, got = tsp._gather(c, kind, sec, n_proofs, d_rows)
            log_k, _ = c.air_sha256_public_shape(kind, sec, n_proofs)
            want = sp.public_table(kind, n, sec, list(rows), log_k)
            assert np.array_equal(got, want), (sec, np.argwhere(got != want)[:10])
            off, n_rows, width = _section_geom(kind, n, sec)
            assert width == W
            for p in range(n_proofs):
                blocks = trace[p, off:off + n_rows * W].reshape(-1, 64, W)
                live = blocks.any(axis=(1, 2))
                u = got[p * PW:(p + 1) * PW]
                diff = np.argwhere(u[sp.PW_W:sp.PW_W + 16, :len(blocks)].T != blocks[:, :16, 0])
                assert not len(diff), (sec, p, diff[:8].tolist())
                assert np.array_equal((u[sp.PW_NEW] + u[sp.PW_CHN])[:len(blocks)], live.astype(np.uint64)), (sec, p)
                assert not u[:, len(blocks):].any() and live.any()
                if sec == HEADER:
                    n_two_leaf += int(u[sp.PW_CHN, 1]) + int(u[sp.PW_CHN, 11])  # (the second blocks of the chain-id and height leaves)
        assert n_two_leaf == 14  # (lengths 55 .. 255 of both leaves: seven of eight proofs each)


# ---- C: the verifier at K = 256, 512 and 4096
@pytest.fixture(scope="module")
def whole_hashes(skip4, step3):
    """[(table blocks [9][64 b], public blocks [26][b])], b = 1 or 2: every hash of the CPU oracle's T.3, T.5 and T.6 rows of skip N = 4
    and step N = 3 (two proofs each) with its own public blocks"""
    out = []
    for kind, n, tables, elems, pubs in (skip4, step3):
        for sec in (SHA256, TREE, HEADER):
            per = tsp.PER[sec]
            for p in range(len(elems)):
                t, u = tables[sec][p * W:(p + 1) * W], pubs[sec][p * PW:(p + 1) * PW]
                for k in range(0, u.shape[1], per):
                    if not u[sp.PW_NEW, k]:
                        continue
                    b = 2 if per == 2 and u[sp.PW_CHN, k + 1] else 1
                    out.append((t[:, 64 * k:64 * (k + b)].copy(), u[:, k:k + b].copy()))
    assert sum(len(u[0]) == 1 for _, u in out) >= 20 and sum(len(u[0]) == 2 for _, u in out) >= 20
    return out


def _tiling(whole_hashes, K, n_proofs, seed):
    """(table [9 n_proofs][64 K], pub [26 n_proofs][K]): whole hashes in a seeded order, a zero block in place of every fifth draw.
    Set 6's constraints are local to a block and the flags of the next one (cyclic), so every concatenation of whole hashes and zero
    blocks satisfies them"""
    rng = np.random.default_rng(seed)
    table, pub = np.zeros((n_proofs * W, 64 * K), dtype=np.uint64), np.zeros((n_proofs * PW, K), dtype=np.uint64)
    order, at = rng.permutation(len(whole_hashes)), 0
    for p in range(n_proofs):
        k = 0
        while k < K:
            t, u = whole_hashes[order[at % len(order)]]
            at += 1
            b = u.shape[1]
            if k + b > K:  # (one block left: the next one-block hash takes it)
                continue
            if at % 5 == 0 and k < K - min(8, K // 4):  # (none among a proof's last blocks, eight at most: its last block is live)
                k += 1
                continue
            table[p * W:(p + 1) * W, 64 * k:64 * (k + b)], pub[p * PW:(p + 1) * PW, k:k + b] = t, u
            k += b
    return table, pub


def _tiling_is_fit(pub):
    """live and zero blocks, one- and two-block hashes, and beyond block 256 no period that divides 256"""
    K = pub.shape[1]
    new, chn = pub[sp.PW_NEW::PW], pub[sp.PW_CHN::PW]
    assert new.any() and chn.any() and (new + chn == 0).any() and int((new + chn).max()) == 1
    assert ((new[:, :-1] == 1) & (chn[:, 1:] == 0)).any()  # (a one-block hash)
    if K > 256:
        assert (pub[:, :256] != pub[:, 256:512]).any(axis=1).sum() >= 20
    return int((new + chn)[:, 256:].sum())


@pytest.mark.parametrize("K", [16, 512])
def test_tilings_satisfy_the_constraints_as_integers(whole_hashes, K):
    """the tilings the chains below prove, at K = 16 and K = 512, one proof: all 50 constraints are integer identities on every row (the
    wrap-around from the last block to block 0 included), under the helper of the tiled table and the tiled public blocks"""
    table, pub = _tiling(whole_hashes, K, 1, 17600 + K)
    _tiling_is_fit(pub)
    res = sp.integer_residuals(table, sp.helper(table, pub, 1), pub)
    assert len(res) == sp.CONSTRAINTS - 1 + 16
    for j, c in enumerate(res):
        assert not c.any(), (K, j, np.flatnonzero(c)[:4])


def _model_verdicts(oracle, p, caps, proof, pub):
    """sp.verify, without running tests/batch_model.py's verifier where the identity alone decides"""
    if not sp.identity(oracle, p, 0, 1, caps, proof, pub):
        return [False] * p["n_queries"]
    return [bool(ok) for ok in bm.verify(oracle, p, caps, proof, _shift())]


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs,n_queries", [(14, 1, 2), (15, 2, 4), (18, 1, 2)])
def test_tilings_through_the_verifier_at_k_256_512_and_4096(ctx, oracle, whole_hashes, log_rows, n_proofs, n_queries):
    """k_air_link_check's barycentric sums beyond round m = 0: thread t takes the blocks k = t, t + 256, ... of every coset, one round at
    K = 256 (the last K with one), two at K = 512 (what T.5 has at N = 128) and sixteen at K = 4096.  An honest tiling through the
    caller-level chain (helper, LDE, caps, quotient, batch proof, tmx_air_sha256_link_verify_device), blow-up 2: the proof is of low
    degree, the model identity holds and every device verdict equals the model verifier's -- all accept, which a wrong PQ(zeta) in any
    round would not allow; one bumped helper opening and a public table with one changed word at a block k >= 256 (K = 256: at its last
    live block) reject every query, as the model does.  The public vectors do not repeat with a period that divides 256"""
    K = 1 << (log_rows - 6)
    table, pub = _tiling(whole_hashes, K, n_proofs, 17700 + log_rows)
    beyond = _tiling_is_fit(pub)
    assert (beyond > 0) == (K > 256)
    p, d_caps, got, _, _, _ = tsp._chain(ctx, oracle, table, pub, 1, n_queries=n_queries)
    assert ctx.fri_last_degree_ok() is True
    caps = _down(d_caps)
    assert sp.identity(oracle, p, 0, 1, caps, got, pub)
    model = _model_verdicts(oracle, p, caps, got, pub)
    assert all(model) and tsp._verdicts(ctx, p, 0, 1, d_caps, got, pub) == model
    bad = _bumped(got, bm.layout(p)["off_open"][1] + (n_proofs - 1) * HC + sp.HDG + 3)
    assert not sp.identity(oracle, p, 0, 1, caps, bad, pub)
    assert tsp._verdicts(ctx, p, 0, 1, d_caps, bad, pub) == [False] * n_queries
    k = K - 1 - int(np.flatnonzero((pub[sp.PW_NEW] + pub[sp.PW_CHN])[::-1])[0])  # the last live block of proof 0
    assert k >= min(256, K - 8)
    for col in (sp.PW_W + 7, sp.PW_DIG + 4 if pub[sp.PW_DIG:sp.PW_DIG + 8, k].any() else sp.PW_W + 2):
        other = pub.copy()
        other[col, k] ^= np.uint64(1)
        assert not sp.identity(oracle, p, 0, 1, caps, got, other)
        assert tsp._verdicts(ctx, p, 0, 1, d_caps, got, other) == [False] * n_queries, (col, k)


# ---- D: blow-up 64
@pytest.mark.gpu
@pytest.mark.parametrize("log_rows,n_proofs", [(7, 3), (10, 1)])
def test_quotient_of_random_columns_at_blowup_64(ctx, oracle, log_rows, n_proofs):
    """test_sha_public.test_quotient_of_random_columns_equals_the_model's comparison at log_blowup 6, the largest the call accepts: every
    selector table of AIR6_PER_MAX = 4096 entries filled to its last word by sixteen workgroups of k_air_link_tables.  Quotient and gamma
    word for word; three proofs also in two pieces, both orders"""
    tsp.test_quotient_of_random_columns_equals_the_model(ctx, oracle, log_rows, 6, n_proofs, CAP_H)


@pytest.mark.gpu
@pytest.mark.parametrize("log_k", [1, 6])
def test_public_chain_at_blowup_64(ctx, oracle, log_k):
    """test_sha_public.test_public_chain_equals_the_model's comparison at log_blowup 6: K = 2 and K = 64 public blocks through gamma, V,
    the seventeen extensions and their fold by the 4096-entry 1 / S and 1 / D_t tables"""
    tsp.test_public_chain_equals_the_model(ctx, oracle, log_k, 6, 1)


# ---- E: pieces that start at proof 256 and above
MANY = 259


@pytest.mark.gpu
def test_pieces_that_start_at_proof_256_and_above(ctx, oracle):
    """N = 128, blow-up 2, 259 proofs of random extended columns: the whole call equals the model (gamma too); the pieces [0, 256) +
    [256, 259), [258, 259) + [0, 258) and [256, 259) + [0, 256), each helper piece in a buffer of its own, leave the whole call's words;
    [256, 259) and [258, 259) alone equal the model's pieces -- gpow[51] = gamma^(50 first) with first = 256 and 258, the table read from
    proof `first` on"""
    log_n, lb = 8, 1
    rng = np.random.default_rng(17800)
    ext, hext = _random_ext(rng, MANY * W, log_n), _random_ext(rng, MANY * HC, log_n)
    pub = rng.integers(0, P, (PW * MANY, 2), dtype=np.uint64)
    d_cols, d_hcols, d_pub = _up(ext), _up(hext), _up(pub)
    _, d_cap = _tree(ctx, d_cols, log_n, MANY * W)
    _, d_cap_h = _tree(ctx, d_hcols, log_n, MANY * HC)
    whole = _down(tsp._device_quotient(ctx, log_n, lb, MANY, d_cols, d_hcols, d_cap, d_cap_h, d_pub))
    g = sp.gamma(oracle, log_n, lb, CAP_H, MANY, _down(d_cap), _down(d_cap_h), pub)
    assert ctx.air_last_gamma() == g
    want = sp.quotient(oracle, log_n, lb, MANY, ext, hext, pub, _shift(), g)
    assert np.array_equal(whole, want), np.flatnonzero(whole != want)[:10]
    a = (log_n, lb, CAP_H, MANY, d_cols.data_ptr())
    b = (d_cap.data_ptr(), d_cap_h.data_ptr(), d_pub.data_ptr())
    bufs = {}

    def pieces(order):
        def run(out):
            for k, (lo, hi) in enumerate(order):
                if (lo, hi) not in bufs:
                    bufs[(lo, hi)] = _up(hext[lo * HC:hi * HC])
                ctx.air_sha256_link_quotient_device(*a, bufs[(lo, hi)].data_ptr(), *b, out, 0, proof_range=(lo, hi), accumulate=int(k > 0))
                assert ctx.air_last_gamma() == g
        return _down(_guarded(2 << log_n, run))
    for order in ([(0, 256), (256, 259)], [(258, 259), (0, 258)], [(256, 259), (0, 256)]):
        got = pieces(order)
        assert np.array_equal(got, whole), (order, np.flatnonzero(got != whole)[:10])
    for lo, hi in ((256, 259), (258, 259)):
        got, piece = pieces([(lo, hi)]), sp.quotient(oracle, log_n, lb, MANY, ext, hext, pub, _shift(), g, proofs=range(lo, hi))
        assert np.array_equal(got, piece), ((lo, hi), np.flatnonzero(got != piece)[:10])


# ---- F: public words at or above p
def _lifted(rng, pub):
    """pub with about a third of its words drawn from [p, 2^64): every flag column, one w and one digest column of every proof whole"""
    lift = rng.random(pub.shape) < 0.3
    for col in (sp.PW_NEW, sp.PW_CHN, sp.PW_W + 3, sp.PW_DIG + 2):
        lift[col::PW] = True
    out = pub.copy()
    out[lift] = rng.integers(P, 1 << 64, int(lift.sum()), dtype=np.uint64, endpoint=False)
    assert int(out[sp.PW_NEW::PW].min()) >= P and int(out[sp.PW_CHN::PW].min()) >= P
    return out, int(lift.sum())


@pytest.mark.gpu
def test_quotient_under_public_words_at_or_above_p(ctx, oracle):
    """include/tmx.h: the quotient is "defined for any columns and any pub".  N = 128, blow-up 2, three proofs of random columns and a
    public table with a third of its words in [p, 2^64) -- both flag columns, w_3 and dig_2 of every proof whole: quotient and gamma
    equal the model's, which reduces pub in `combine` and hashes the words as given through the oracle's Poseidon.  Device and oracle
    agree on the digest of such words: the permutation works mod p, so a word and the word + p absorb alike
    (tmx_poseidon_merkle_device documents no reduction of its own and needs none).  A table and the table reduced mod p are therefore
    ONE public input: the same digest, gamma, V and quotient words, on the device as in the model"""
    log_rows, lb, n_proofs = 7, 1, 3
    log_n = log_rows + lb
    rng = np.random.default_rng(17900)
    ext, hext = _random_ext(rng, n_proofs * W, log_n), _random_ext(rng, n_proofs * HC, log_n)
    pub, n_lifted = _lifted(rng, rng.integers(0, P, (PW * n_proofs, 2), dtype=np.uint64))
    assert 3 * n_lifted >= pub.size and (pub < np.uint64(P)).any()
    d_cols, d_hcols, d_pub = _up(ext), _up(hext), _up(pub)
    _, d_cap = _tree(ctx, d_cols, log_n, n_proofs * W)
    _, d_cap_h = _tree(ctx, d_hcols, log_n, n_proofs * HC)
    got = _down(tsp._device_quotient(ctx, log_n, lb, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, d_pub))
    g = sp.gamma(oracle, log_n, lb, CAP_H, n_proofs, _down(d_cap), _down(d_cap_h), pub)
    assert ctx.air_last_gamma() == g
    want = sp.quotient(oracle, log_n, lb, n_proofs, ext, hext, pub, _shift(), g)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    reduced = pub % np.uint64(P)  # (the canonical table is the same public input: the same digest and gamma, the same V)
    assert sp.gamma(oracle, log_n, lb, CAP_H, n_proofs, _down(d_cap), _down(d_cap_h), reduced) == g
    assert sp.combine(reduced, g) == sp.combine(pub, g)
    d_reduced = _up(reduced)
    again = _down(tsp._device_quotient(ctx, log_n, lb, n_proofs, d_cols, d_hcols, d_cap, d_cap_h, d_reduced))
    assert ctx.air_last_gamma() == g and np.array_equal(again, want)


@pytest.mark.gpu
def test_verifier_under_public_words_at_or_above_p(ctx, oracle, whole_hashes):
    """one chain (N = 128: a two-block hash per proof, two proofs, blow-up 2) under a public table whose words are the honest ones plus p
    where that fits in 64 bits -- every w and digest word below 2^32 - 1 and every SET flag; a clear flag stays 0, since the helper's rule
    "set when the low 32 bits are not zero" would read p as set.  k_air_link_combine and k_air_link_check reduce what they read: the
    verdicts equal the model's, all accept; under one changed non-canonical word every query is rejected"""
    two = [h for h in whole_hashes if h[1].shape[1] == 2]
    table, honest = np.concatenate([two[0][0], two[5][0]]), np.concatenate([two[0][1], two[5][1]])
    pub = honest.copy()
    lift = (honest < np.uint64(M32))
    lift[sp.PW_NEW::PW] = honest[sp.PW_NEW::PW] == 1
    lift[sp.PW_CHN::PW] = honest[sp.PW_CHN::PW] == 1
    pub[lift] += np.uint64(P)
    assert 2 * int(lift.sum()) > pub.size and np.array_equal(pub % np.uint64(P), honest)
    p, d_caps, got, _, _, _ = tsp._chain(ctx, oracle, table, pub, 1, n_queries=3)
    assert ctx.fri_last_degree_ok() is True
    caps = _down(d_caps)
    model = _model_verdicts(oracle, p, caps, got, pub)
    assert all(model) and tsp._verdicts(ctx, p, 0, 1, d_caps, got, pub) == model
    other = pub.copy()
    other[PW + sp.PW_W + 9, 1] += np.uint64(1)
    assert int(other[PW + sp.PW_W + 9, 1]) >= P and not sp.identity(oracle, p, 0, 1, caps, got, other)
    assert tsp._verdicts(ctx, p, 0, 1, d_caps, got, other) == [False] * 3


# ---- G: the set-level call on a skip section and beside sets 3 and 4
WAYS = {"6t": [(6, TREE)], "36t": [(3, TREE), (6, TREE)], "63t": [(6, TREE), (3, TREE)], "6s": [(6, SHA256)], "46s": [(4, SHA256), (6, SHA256)]}
HELPER_OF = {3: H3, 4: H4, 6: H6}


@pytest.fixture(scope="module")
def skip_sets(built_lib, oracle):
    """a set SHA256 + TREE at skip N = 4 (two validator sets: T.5 has K = 16, T.3 K = 8), two proofs, blow-up 2, under the public tables the
    device gathered from the element rows of the same batch; per way of WAYS: (params, section_of, caps in oracle order, proof words,
    gammas, verdicts), and the model's helper cap through the device's tree for the two ways with set 6 alone"""
    import torch
    import tendermintx_amd as tmx
    kind, n, n_proofs, lb = 0, 4, 2, 1
    cw = 4 << CAP_H
    out = {}
    with tmx.Context(n, CID, max_batch=n_proofs) as c:
        d_rows, tr = tsp._device_rows(c, kind, n, n_proofs, 9400)
        d_pubs, pubs = {}, {}
        for sec in (SHA256, TREE):
            d_pubs[sec], pubs[sec] = tsp._gather(c, kind, sec, n_proofs, d_rows)
        traces = _down(tr).reshape(n_proofs, -1)
        out["pubs"] = pubs
        calls = {3: lambda sec, h, q: c.trace_commit_set_air_sha256_device(sec, h, q, 0),
                 4: lambda sec, h, q: c.trace_commit_set_air_sha256_sched_device(sec, h, q, 0),
                 6: lambda sec, h, q: c.trace_commit_set_air_sha256_link_device(sec, d_pubs[sec].data_ptr(), h, q, 0)}
        for way, todo in WAYS.items():
            d_caps = _sentinel(2 * cw)
            c.trace_commit_set_device(kind, n_proofs, SHA256 | TREE, lb, CAP_H, tr.data_ptr(), d_caps.data_ptr(), 0)
            assert c.trace_commit_set_shape()[1] == [TREE, SHA256]
            cap_of, gammas = {TREE: d_caps[:cw], SHA256: d_caps[cw:]}, {}
            for set_id, sec in todo:
                cap_of[HELPER_OF[set_id]], cap_of[2 * HELPER_OF[set_id]] = _sentinel(cw), _sentinel(cw)
                calls[set_id](sec, cap_of[HELPER_OF[set_id]].data_ptr(), cap_of[2 * HELPER_OF[set_id]].data_ptr())
                gammas[set_id] = c.air_last_gamma()
            shape, order = c.trace_commit_set_shape()
            p = dict(shape, arity_bits=2, final_log_max=2, n_queries=3, pow_bits=0)
            proof = _guarded(bm.layout(p)["words"], lambda o: c.trace_commit_set_prove_device(p, o, 0))
            assert c.fri_last_degree_ok() is True
            all_caps = torch.cat([cap_of[sec] for sec in order])
            got, sec = _down(proof), todo[0][1]
            kt, k6, pub = order.index(sec), order.index(H6), pubs[sec]
            v = dict(link=tsp._verdicts(c, p, kt, k6, all_caps, got, pub), batch=tsa._verdicts(c, p, 0, all_caps, got, batch_only=True))
            if H3 in order:
                v["round"] = tsa._verdicts(c, p, kt, all_caps, got)
            if H4 in order:
                v["sched"] = tss._verdicts(c, p, kt, order.index(H4), all_caps, got)
            v["bad"] = tsp._verdicts(c, p, kt, k6, all_caps, _bumped(got, bm.layout(p)["off_open"][k6 + 1]), pub)
            other = pub.copy()
            other[PW + sp.PW_W + 3, 2] ^= np.uint64(1)
            v["other_pub"] = tsp._verdicts(c, p, kt, k6, all_caps, got, other)
            s = dict(p=p, order=order, caps=_down(all_caps), proof=got, verdicts=v, gammas=gammas, kt=kt, k6=k6)
            if len(todo) == 1:  # the model's helper of the device's rows under the gathered table, through the device's tree
                off, rows, _ = _section_geom(kind, n, sec)
                log_rows = p["log_n"][kt] - lb
                table = np.zeros((n_proofs * W, 1 << log_rows), dtype=np.uint64)
                for q, full in enumerate(traces):
                    table[q * W:(q + 1) * W, :rows] = full[off:off + rows * W].reshape(rows, W).T
                hext = oracle.lde(sp.helper(table, pub, n_proofs), lb)
                s["cap_h_model"] = _down(_tree(c, _up(hext), log_rows + lb, n_proofs * HC)[1])
            out[way] = s
    return out


def _caps_of(s, k):
    cw = 4 << CAP_H
    return s["caps"][k * cw:(k + 1) * cw]


def _set_6_holds(oracle, s, pub, n_proofs=2, lb=1):
    """set 6's part of a way: the helper's cap position, gamma, the device verifier against the model's, both rejections"""
    kt, k6, p = s["kt"], s["k6"], s["p"]
    assert p["n_cols"][k6:k6 + 2] == [HC * n_proofs, 2] and p["log_n"][k6] == p["log_n"][k6 + 1] == p["log_n"][kt]
    assert s["gammas"][6] == sp.gamma(oracle, p["log_n"][kt], lb, CAP_H, n_proofs, _caps_of(s, kt), _caps_of(s, k6), pub)
    batch = bm.verify(oracle, p, s["caps"], s["proof"], _shift())
    assert s["verdicts"]["batch"] == [bool(x) for x in batch] and all(batch)
    assert sp.identity(oracle, p, kt, k6, s["caps"], s["proof"], pub)  # (with `batch`: sp.verify accepts every query)
    assert s["verdicts"]["link"] == [True] * p["n_queries"]
    assert not any(s["verdicts"]["bad"]) and not any(s["verdicts"]["other_pub"])


@pytest.mark.gpu
def test_set_level_on_the_tree_table_of_a_skip_section(oracle, skip_sets):
    """set 6 alone on TREE of skip N = 4: two validator sets, K = 16 (the slots of both sets live, the padding zero); section_of ends
    16, 8192, 16384 with SHA256 behind; the helper's cap is the model's helper of the device's rows under the gathered table through the
    device's tree; gamma, the device verifier and the model's (all accept), tmx_batch_verify_device against tests/batch_model.py; a bumped
    quotient opening and a changed public word reject"""
    s, pub = skip_sets["6t"], skip_sets["pubs"][TREE]
    assert s["order"] == [TREE, H6, Q6, SHA256] and s["p"]["log_n"] == [11, 11, 11, 10]
    assert s["p"]["n_cols"] == [2 * W, 2 * HC, 2, 2 * W]
    live = (pub[sp.PW_NEW] + pub[sp.PW_CHN]).reshape(-1, 2)[:, 0]
    assert pub.shape == (2 * PW, 16) and live.tolist() == [1, 1, 1, 1, 1, 1, 0, 0]  # (three slots per set, two sets)
    assert np.array_equal(_caps_of(s, 1), s["cap_h_model"])
    _set_6_holds(oracle, s, pub)


@pytest.mark.gpu
def test_set_level_on_the_tree_table_beside_set_3_in_both_orders(oracle, skip_sets):
    """the call orders 3-6 and 6-3 on TREE both end as TREE, H3, Q3, H6, Q6, SHA256: the same section_of, caps, gammas and proof word for
    word; set 6's caps and gamma are those of the set with set 6 alone; the device verifiers of sets 3 and 6 accept that proof and equal
    their models; set 6 rejects a bumped quotient opening and a changed public word"""
    a, b, alone, pub = skip_sets["36t"], skip_sets["63t"], skip_sets["6t"], skip_sets["pubs"][TREE]
    assert a["order"] == b["order"] == [TREE, H3, Q3, H6, Q6, SHA256]
    assert a["p"] == b["p"] and a["p"]["n_cols"][:5] == [2 * W, 2 * sm.HELPER_COLS, 2, 2 * HC, 2]
    assert np.array_equal(a["caps"], b["caps"]) and np.array_equal(a["proof"], b["proof"]) and a["gammas"] == b["gammas"]
    assert np.array_equal(_caps_of(a, 3), _caps_of(alone, 1)) and np.array_equal(_caps_of(a, 4), _caps_of(alone, 2))
    assert a["gammas"][6] == alone["gammas"][6]
    for s in (a, b):
        _set_6_holds(oracle, s, pub)
        assert s["verdicts"]["round"] == [True] * 3
    assert sm.identity(oracle, a["p"], 0, a["caps"], a["proof"])


@pytest.mark.gpu
def test_set_level_on_t3_beside_set_4(oracle, skip_sets):
    """set 6 on T.3 (SHA256 of skip N = 4: eight one-block hashes, K = 8) alone and behind set 4: TREE, SHA256, H4, Q4, H6, Q6; set 6's caps
    and gamma are those of the set with set 6 alone, the helper's cap the model's; the device verifiers of sets 4 and 6 accept and equal
    their models; set 6 rejects a bumped quotient opening and a changed public word"""
    s, alone, pub = skip_sets["46s"], skip_sets["6s"], skip_sets["pubs"][SHA256]
    assert alone["order"] == [TREE, SHA256, H6, Q6] and s["order"] == [TREE, SHA256, H4, Q4, H6, Q6]
    assert pub.shape == (2 * PW, 8) and pub[sp.PW_NEW::PW].all() and not pub[sp.PW_CHN::PW].any()
    assert np.array_equal(_caps_of(alone, 2), alone["cap_h_model"])
    assert np.array_equal(_caps_of(s, 4), _caps_of(alone, 2)) and np.array_equal(_caps_of(s, 5), _caps_of(alone, 3))
    assert s["gammas"][6] == alone["gammas"][6]
    _set_6_holds(oracle, alone, pub)
    _set_6_holds(oracle, s, pub)
    assert s["verdicts"]["sched"] == [True] * 3 and ss.identity(oracle, s["p"], 1, 2, s["caps"], s["proof"])
