"""Level-2 trace rows (tmx_trace_rows_device) after every producer of the Level-1 records they read, at every schedule and size.

The trace does not read the batch's inputs alone: the ladders take h, A and the decode flag from the EdDSA lane records, T.5 hashes the
leaf values and the validator-tree nodes, T.6 the proof records -- all of them what the LAST witness call left in the context.  On the
launch-graph path those records come from stores of their own (k_ed_fin writes the D.1b row words and the lane record apart, k_ed_dedup
copies the dummy record, the validator-set cache copies leaf values and nodes), so rows that are bit-exact there say nothing about the
records.  test_trace.py and the commit / open / FRI / DEEP chains build their rows after one cold call on a fresh context, all of them on
the small path (k_tiny); this module covers the rest:

- the small path, the N <= 32 bound of 2048 lanes, the launch graph (compacted, from the set cache, without it), the fused rows, the
  throughput regime and a launch of more than 8192 distinct keys; skip at N = 128, step and odd N at launch-graph sizes;
- every schedule knob of test_gpu_parity.py;
- every witness entry point that sets the batch the trace reads;
- section masks, a prefix of the batch, the ladder segmentation (in child processes: those knobs are read once per process);
- stream order without host syncs, refusals that write nothing, and the cap of one commit over the rows.

Every case runs cold, then warm on the same context with the batch's proofs in another order, so that a record left stale by the warm
call's producer differs from what the trace must read.  A proof's rows depend on its own records alone: the oracle traces V distinct
proofs per (kind, N) once (thread pool: its C calls release the GIL), batches repeat them (which also gives key- and set-cache hits inside
a batch), and the rows are compared on the device."""
import os
import struct
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_commit_pipeline import _section_geom
from test_gpu_parity import KNOBS

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 8)
CID = b"celestia"
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -1          # what the rows hold before the trace: an element the trace never writes (every value is < 2^32)


@pytest.fixture(scope="module")
def tmx(built_lib):
    import tendermintx_amd
    return tendermintx_amd


def _dev():
    import torch
    return torch.device("cuda", 0)


# ---- the variants: distinct proofs whose rows the oracle generates once
def _signed_lanes(targets, n):
    return [i for i in range(n) if targets[i * 256 + 223] & 1]


def _variant_inputs(kind, n, seed):
    """14 distinct proofs of one kind at VALIDATOR_SET_SIZE_MAX n: eight over two full validator sets (90 % signing), six over two sets of
    nb < n (70 % signing), with the edges of test_trace.py and the others where a record producer could go wrong."""
    from tendermintx_amd.synth import Workload
    nb = n - n // 4 - 1
    full = Workload(kind, n, 8, n, chain_id=CID, seed=seed, signed_permille=900, rounds=(0, 2), n_sets=2)
    part = Workload(kind, n, 6, nb, chain_id=CID, seed=seed + 1, signed_permille=700, n_sets=2)
    proofs, targets, trusteds = [], [], []
    for wl, P in ((full, 8), (part, 6)):
        for p in range(P):
            proofs.append(wl.proofs[p * 2336:(p + 1) * 2336])
            targets.append(bytearray(wl.targets[p * n * 256:(p + 1) * n * 256]))
            trusteds.append(bytearray(wl.trusteds[p * n * 48:(p + 1) * n * 48]) if kind == 0 else None)
    lane = lambda v, k: _signed_lanes(targets[v], n)[k]
    targets[1][1 * 256:1 * 256 + 32] = (2).to_bytes(32, "little")                 # an undecodable public key: zero ladders
    targets[2][lane(2, 0) * 256 + 40] ^= 0x10                                      # corrupted R of a lane that signed: a failing signature
    targets[3][lane(3, 1) * 256 + 64 + 31] |= 0xF0                                 # s >= 2^252 (non-canonical, still a ladder)
    targets[4][5 * 256 + 224:5 * 256 + 232] = struct.pack("<Q", 2**63 + 5)         # a power with bit 63 set
    targets[5][lane(5, 2) * 256 + 32:lane(5, 2) * 256 + 64] = bytes([1] + [0] * 31)  # R = the identity (small order)
    targets[9][2 * 256:2 * 256 + 32] = bytes([1] + [0] * 31)                       # a small-order key in a set of nb < n
    targets[10][lane(10, 0) * 256 + 40] ^= 0x01                                    # a failing signature in a set of nb < n
    if kind == 0:
        trusteds[6][4 * 48:4 * 48 + 32] = targets[6][lane(6, 3) * 256:lane(6, 3) * 256 + 32]   # a signing key in both sets, explicitly
        trusteds[11][0:32] = targets[11][0:32]
        trusteds[12][3 * 48 + 32:3 * 48 + 40] = struct.pack("<Q", 2**63 + 1)      # the trusted set's power with bit 63 set
    else:
        targets[6][(n - 1) * 256 + 224:(n - 1) * 256 + 232] = struct.pack("<Q", 2**63 + 1)
    return proofs, [bytes(t) for t in targets], [bytes(r) if r is not None else None for r in trusteds]


def _oracle_rows(oracle, kind, n, inputs, which):
    """{variant: the oracle's rows} for the variants `which` (thread pool: the C calls release the GIL)"""
    proofs, targets, trusteds = inputs
    with ThreadPoolExecutor(THREADS) as ex:
        return dict(zip(which, ex.map(lambda v: oracle.trace(kind, proofs[v], targets[v], trusteds[v], n), which)))


class Variants:
    """Distinct proofs of one (kind, n) and the oracle rows of all or some of them: on the host ({variant: rows}) and on the device
    ([V, te] int64, zero where a variant has none)."""

    def __init__(self, kind, n, inputs, rows):
        import torch
        self.kind, self.n = kind, n
        self.proofs, self.targets, self.trusteds = inputs
        self.V = len(self.proofs)
        self.rows = rows
        self.want = torch.zeros((self.V, next(iter(rows.values())).size), dtype=torch.int64, device=_dev())
        for v, r in rows.items():
            self.want[v] = torch.from_numpy(r.view(np.int64)).to(_dev())

    def batch(self, idx):
        return (b"".join(self.proofs[v] for v in idx), b"".join(self.targets[v] for v in idx),
                b"".join(self.trusteds[v] for v in idx) if self.kind == 0 else None)

    def upload(self, idx):
        import torch
        return [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(_dev()) if b else None for b in self.batch(idx)]


_VARIANTS = {}


def _seed(kind, n):
    return 9100 + 31 * n + kind


def _variants(oracle, kind, n):
    if (kind, n) not in _VARIANTS:
        inputs = _variant_inputs(kind, n, _seed(kind, n))
        _VARIANTS[(kind, n)] = Variants(kind, n, inputs, _oracle_rows(oracle, kind, n, inputs, range(len(inputs[0]))))
    return _VARIANTS[(kind, n)]


def _order(V, P, run):
    """proof p of a batch -> variant: run 0 cycles through the variants, run 1 (the warm call) rotates each cycle by 1 .. V - 1, so that
    every proof position holds another proof than in the call before"""
    if run == 0:
        return [p % V for p in range(P)]
    return [(p + 1 + (p // V) % (V - 1)) % V for p in range(P)]


# ---- where an element lives
def _where(kind, n, e):
    off1, _, w1 = _section_geom(kind, n, 1)
    off2, _, w2 = _section_geom(kind, n, 2)
    off4, rows4, w4 = _section_geom(kind, n, 4)
    off16, _, _ = _section_geom(kind, n, 16)
    off32, _, _ = _section_geom(kind, n, 32)
    sets = 2 if kind == 0 else 1
    tn = (off32 - off16) // (sets * 1152)
    if e < off2:
        r, c = divmod(e - off1, w1)
        lk, row = divmod(r, 256)
        return f"ladders lane {lk // 2} ladder {'h*A' if lk & 1 else 's*B'} row {row} element {c}"
    if e < off4:
        r, c = divmod(e - off2, w2)
        lb, row = divmod(r, 80)
        return f"SHA-512 lane {lb // 2} block {lb & 1} round {row} element {c}"
    if e < off4 + rows4 * w4:
        r, c = divmod(e - off4, w4)
        sl, row = divmod(r, 64)
        return f"SHA-256 set {sl // n} lane {sl % n} round {row} element {c}"
    if e < off16:
        i, j = divmod(e - off4 - rows4 * w4, n)
        return f"N x N target lane {i} trusted lane {j}"
    if e < off32:
        node, r = divmod(e - off16, 1152)
        return f"tree set {node // tn} node slot {node % tn} row {r // 9} element {r % 9}"
    item, r = divmod(e - off32, 1152)
    return f"header proof {item // 5} hash {item % 5} row {r // 9} element {r % 9}"


def _compare(tr, V, idx, what, proofs=None, span=None):
    """tr: [P, te] int64 on the device; proof p must hold the oracle rows of variant idx[p] -- every proof or those in `proofs`, elements
    [a, b) = span or all"""
    import torch
    dev = _dev()
    a, b = span or (0, V.want.shape[1])
    sel = list(range(len(idx))) if proofs is None else list(proofs)
    for c0 in range(0, len(sel), 16):
        ps = sel[c0:c0 + 16]
        got = tr[torch.tensor(ps, device=dev)][:, a:b]
        ne = got != V.want[torch.tensor([idx[p] for p in ps], device=dev)][:, a:b]
        if bool(ne.any()):
            bad = ne.any(1).nonzero().flatten().tolist()
            k = bad[0]
            e = int(ne[k].nonzero()[0])
            p = ps[k]
            raise AssertionError(f"{what}: proof {p} (variant {idx[p]}) {_where(V.kind, V.n, a + e)}: got {int(got[k, e]) & (2**64 - 1):#x}, "
                                 f"want {int(V.want[idx[p], a + e]) & (2**64 - 1):#x}; {int(ne.sum())} elements differ, in proofs "
                                 f"{[ps[j] for j in bad][:8]}")


def _check_rows(oracle, V, tr, idx, proofs):
    """the constraint checker on a few proofs' device rows"""
    def one(p):
        v = idx[p]
        return p, oracle.trace_check(V.kind, V.proofs[v], V.targets[v], V.trusteds[v], V.n, tr[p].cpu().numpy().view(np.uint64))
    with ThreadPoolExecutor(THREADS) as ex:
        for p, rc in ex.map(one, proofs):
            assert rc == 0, (p, rc)


# ---- one witness call + the trace
def _ptr(t):
    return t.data_ptr() if t is not None else None


def _witness(ctx, V, idx, d, entry="device", stream=0):
    """the Level-1 call of one of the entry points the trace accepts; returns the buffers it writes (alive until the caller syncs)"""
    import torch
    from tendermintx_amd import _lib
    kind, P, dev = V.kind, len(idx), _dev()
    if entry == "host":
        ctx.witness_batch(kind, *V.batch(idx))
        return ()
    if entry == "value":
        out = torch.empty(P * ctx.value_layout(kind).bytes, dtype=torch.uint8, device=dev)
        ctx.inputs_value_batch_device(kind, P, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), out.data_ptr(), _lib.SEC_HINT, stream)
        return (out,)
    out = torch.empty((P, ctx.elem_stride(kind)), dtype=torch.int64, device=dev)
    rep = torch.empty(P * 64, dtype=torch.uint8, device=dev)
    if entry == "hint":
        ctx.witness_batch_device_sections(kind, P, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), out.data_ptr(), rep.data_ptr(), _lib.SEC_HINT, stream)
    else:
        assert entry == "device"
        ctx.witness_batch_device(kind, P, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), out.data_ptr(), rep.data_ptr(), stream)
    return out, rep


def _trace(ctx, V, idx, tr, entry="device"):
    """witness + trace of the batch idx into tr ([>= P, te] int64, reset to the sentinel first) on the HIP default stream; synchronizes"""
    import torch
    d = V.upload(idx)
    tr.fill_(SENTINEL)
    torch.cuda.synchronize(_dev())
    keep = _witness(ctx, V, idx, d, entry)
    ctx.trace_rows_device(V.kind, len(idx), _ptr(d[1]), _ptr(d[2]), tr.data_ptr(), 63, 0)
    torch.cuda.synchronize(_dev())
    del keep


def _rows(ctx, kind, P):
    import torch
    return torch.empty((P, ctx.trace_elem_count(kind)), dtype=torch.int64, device=_dev())


def _cold_warm(tmx, oracle, kind, n, P, what, entry="device", check=()):
    """the batch cold on a fresh context, then warm (another proof order) on the same one; returns the context's set-cache stats"""
    V = _variants(oracle, kind, n)
    with tmx.Context(n, CID, max_batch=P) as ctx:
        tr = _rows(ctx, kind, P)
        for run in range(2):
            idx = _order(V.V, P, run)
            _trace(ctx, V, idx, tr, entry)
            _compare(tr, V, idx, f"{what} run {run}")
            if check and run == 1:
                _check_rows(oracle, V, tr, idx, check)
        return ctx.set_cache_stats()


# ---- sizes and paths
@pytest.mark.parametrize("P", [4, 12])
def test_small_path_n128(tmx, oracle, P):
    _cold_warm(tmx, oracle, 0, 128, P, f"small path {P} x 128", check=(0, P - 1))


@pytest.mark.parametrize("P", [64, 65])
def test_the_2048_lane_bound_at_n32(tmx, oracle, P):
    """64 proofs x 32 lanes are the last small launch, 65 the first launch graph at this N"""
    _cold_warm(tmx, oracle, 0, 32, P, f"{P} x 32")


@pytest.mark.parametrize("kind,n,P", [(1, 128, 20), (1, 33, 80), (0, 100, 24)])
def test_launch_graph_step_and_odd_n(tmx, oracle, kind, n, P):
    _cold_warm(tmx, oracle, kind, n, P, f"kind {kind} {P} x {n}", check=(1,))


@pytest.mark.parametrize("env", [{}, {"TMX_HASH_FIRST": "0"}, {"TMX_SET_CACHE": "0"}], ids=["default", "compacted", "no-set-cache"])
def test_launch_graph_n128(tmx, oracle, monkeypatch, env):
    """24 proofs x 128: the launch graph; the warm call takes every validator set from the set cache (its all-hit copies of leaf values and
    tree nodes), unless the cache is off; TMX_HASH_FIRST=0 opens the chain with the dedup, which compacts the lanes that signed"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    st = _cold_warm(tmx, oracle, 0, 128, 24, f"launch graph {env}", check=(0, 23))
    if env.get("TMX_SET_CACHE") == "0":
        assert st["served"] == 0
    else:
        assert st["served"] > 0, st


def test_fused_rows_warm_140(tmx, oracle, monkeypatch):
    monkeypatch.setenv("TMX_FUSED_ROWS", "4:2")
    _cold_warm(tmx, oracle, 0, 128, 140, "fused rows 140 x 128")


def test_throughput_regime_640(tmx, oracle):
    """640 proofs x 128 = 81 920 lanes (api.cpp THROUGHPUT_LANES): 26 GB of rows"""
    _cold_warm(tmx, oracle, 0, 128, 640, "throughput 640 x 128", check=(0, 639))


def test_many_distinct_keys(tmx, oracle):
    """More than 8192 distinct keys in one launch (k_ed_keys one key per thread, h*A in the quad form): 68 proofs x 128, each over a
    validator set of its own, so nothing repeats -- a fixed sample of proofs against the oracle, cold and then warm with the batch rotated"""
    from tendermintx_amd.synth import Workload
    n, P = 128, 68
    wl = Workload(0, n, P, n, chain_id=CID, seed=8192, signed_permille=1000, n_sets=P)
    targets = bytearray(wl.targets)
    targets[1 * 256:1 * 256 + 32] = (2).to_bytes(32, "little")            # proof 0: an undecodable key
    targets[(33 * n + 7) * 256 + 40] ^= 0x10                              # proof 33: a failing signature
    targets[((P - 1) * n + 3) * 256 + 64 + 31] |= 0xF0                    # the last proof: s >= 2^252
    inputs = ([wl.proofs[p * 2336:(p + 1) * 2336] for p in range(P)], [bytes(targets[p * n * 256:(p + 1) * n * 256]) for p in range(P)],
              [wl.trusteds[p * n * 48:(p + 1) * n * 48] for p in range(P)])
    rng = np.random.default_rng(68)
    sample = sorted({0, 33, P - 1, *rng.choice(np.arange(1, P - 1), 13, replace=False).tolist()})
    V = Variants(0, n, inputs, _oracle_rows(oracle, 0, n, inputs, sample))
    with tmx.Context(n, CID, max_batch=P) as ctx:
        tr = _rows(ctx, 0, P)
        for run in range(2):
            idx = [(p + run) % P for p in range(P)]
            _trace(ctx, V, idx, tr)
            if run == 0:
                assert ctx.last_dedup()[0] > 8192
            _compare(tr, V, idx, f"distinct keys run {run}", proofs=[p for p in range(P) if idx[p] in V.rows])
        _check_rows(oracle, V, tr, idx, [idx.index(0), idx.index(P - 1)])


# ---- every schedule knob
@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_schedule_knobs(tmx, oracle, monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)      # read at context creation
    _cold_warm(tmx, oracle, 0, 128, 20, f"knobs {knobs}")


# ---- the entry points before the trace
@pytest.mark.parametrize("entry", ["device", "hint", "host", "value"])
@pytest.mark.parametrize("P", [4, 24])
def test_entry_points(tmx, oracle, entry, P):
    _cold_warm(tmx, oracle, 0, 128, P, f"{entry} {P} x 128", entry=entry)


# ---- trace options
def test_section_masks_and_prefix(tmx, oracle):
    """every single section, 1|2, 62 (no ladders: the other sections on the caller's stream) and 63 after one witness call of the launch
    graph: the selected sections equal the oracle, the others keep the sentinel; then a prefix of the batch"""
    import torch
    V = _variants(oracle, 0, 128)
    P = 24
    geo = {s: _section_geom(0, 128, s) for s in (1, 2, 4, 16, 32)}
    te = V.want.shape[1]
    span = {s: (o, o + r * w) for s, (o, r, w) in geo.items()}
    span[8] = (span[4][1], geo[16][0])
    assert span[32][1] == te
    idx = _order(V.V, P, 1)
    with tmx.Context(128, CID, max_batch=P) as ctx:
        tr = _rows(ctx, 0, P)
        d = V.upload(idx)
        keep = _witness(ctx, V, idx, d)
        torch.cuda.synchronize(_dev())
        for mask in (1, 2, 4, 8, 16, 32, 3, 62, 63):
            tr.fill_(SENTINEL)
            ctx.trace_rows_device(0, P, _ptr(d[1]), _ptr(d[2]), tr.data_ptr(), mask, 0)
            torch.cuda.synchronize(_dev())
            for s, (a, b) in span.items():
                if mask & s:
                    _compare(tr, V, idx, f"mask {mask} section {s}", span=(a, b))
                else:
                    assert bool((tr[:, a:b] == SENTINEL).all()), (mask, s)
        tr.fill_(SENTINEL)
        ctx.trace_rows_device(0, P - 5, _ptr(d[1]), _ptr(d[2]), tr.data_ptr(), 63, 0)
        torch.cuda.synchronize(_dev())
        assert bool((tr[P - 5:] == SENTINEL).all())
        _compare(tr, V, idx, "prefix", proofs=range(P - 5))
        del keep


_CHILD = r"""
import sys
sys.path[:0] = [{tests!r}, {root!r}, {oracle!r}]
import numpy as np
import tendermintx_amd as tmx
import test_trace_paths as m
want = np.load({path!r})
V = m.Variants(0, 32, m._variant_inputs(0, 32, m._seed(0, 32)), dict(enumerate(want)))
with tmx.Context(32, m.CID, max_batch=65) as ctx:
    tr = m._rows(ctx, 0, 65)
    for run in range(2):
        idx = m._order(V.V, 65, run)
        m._trace(ctx, V, idx, tr)
        m._compare(tr, V, idx, "run %d" % run)
print("ok")
"""


@pytest.mark.parametrize("segs,rows", [(1, 64), (4, 32), (8, 8), (16, 64)])
def test_ladder_segments_and_rows_per_thread(tmx, oracle, tmp_path, segs, rows):
    """TMX_TRACE_SEGS / TMX_TRACE_ROWS are read once per process: each pairing in a child process of its own, 65 proofs x 32"""
    from conftest import ROOT
    V = _variants(oracle, 0, 32)
    path = str(tmp_path / "want.npy")
    np.save(path, np.stack([V.rows[v] for v in range(V.V)]))
    code = _CHILD.format(tests=HERE, root=ROOT, oracle=os.path.join(ROOT, "oracle", "py"), path=path)
    env = dict(os.environ, TMX_TRACE_SEGS=str(segs), TMX_TRACE_ROWS=str(rows))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- ordering and lifecycle
@pytest.mark.parametrize("P", [4, 24])
def test_two_batches_on_one_stream_without_a_sync(tmx, oracle, P):
    """witness A, trace A, witness B, trace B on a non-default stream, no host sync in between, each trace followed by a comparison queued
    on the same stream: both traces equal the oracle when that stream reaches them (the trace's work on side streams -- pass 2, the other
    sections -- and the witness kernels on side streams are joined back into the caller's stream, not waited for by a sync)"""
    import torch
    V = _variants(oracle, 0, 128)
    a, b = _order(V.V, P, 0), _order(V.V, P, 1)
    dev = _dev()
    st = torch.cuda.Stream(dev)
    with tmx.Context(128, CID, max_batch=P) as ctx:
        tra, trb = _rows(ctx, 0, P), _rows(ctx, 0, P)
        da, db = V.upload(a), V.upload(b)
        wa, wb = V.want[torch.tensor(a, device=dev)], V.want[torch.tensor(b, device=dev)]
        tra.fill_(SENTINEL)
        trb.fill_(SENTINEL)
        torch.cuda.synchronize(dev)
        ka = _witness(ctx, V, a, da, stream=st.cuda_stream)
        ctx.trace_rows_device(0, P, _ptr(da[1]), _ptr(da[2]), tra.data_ptr(), 63, st.cuda_stream)
        with torch.cuda.stream(st):
            oka = (tra == wa).all(1)
        kb = _witness(ctx, V, b, db, stream=st.cuda_stream)
        ctx.trace_rows_device(0, P, _ptr(db[1]), _ptr(db[2]), trb.data_ptr(), 63, st.cuda_stream)
        with torch.cuda.stream(st):
            okb = (trb == wb).all(1)
        st.synchronize()
        _compare(tra, V, a, "trace A")
        _compare(trb, V, b, "trace B")
        assert bool(oka.all()) and bool(okb.all()), ("rows not complete when the caller's stream reached them", oka.tolist(), okb.tolist())
        del ka, kb


def test_refusals_write_nothing(tmx, oracle):
    """the trace refuses (TMX_ERR_BAD_ARG) and writes nothing before any witness call, for another kind and for more proofs than the last
    call; a witness call refused before it enqueues anything (n_proofs > max_batch) leaves the previous batch traceable"""
    import torch
    V = _variants(oracle, 0, 32)
    P = 8
    idx = _order(V.V, P, 1)
    with tmx.Context(32, CID, max_batch=P + 4) as ctx:
        tr = _rows(ctx, 0, P + 4)
        d = V.upload(idx)
        tr.fill_(SENTINEL)
        torch.cuda.synchronize(_dev())

        def refused(kind, n_proofs):
            with pytest.raises(tmx.TmxError) as e:
                ctx.trace_rows_device(kind, n_proofs, _ptr(d[1]), _ptr(d[2]), tr.data_ptr(), 63, 0)
            torch.cuda.synchronize(_dev())
            assert e.value.status == -1 and bool((tr == SENTINEL).all()), (kind, n_proofs, e.value)

        refused(0, P)
        keep = _witness(ctx, V, idx, d)
        refused(1, P)
        refused(0, P + 1)
        big = V.upload(_order(V.V, P + 5, 0))
        with pytest.raises(tmx.TmxError):
            ctx.witness_batch_device(0, P + 5, _ptr(big[0]), _ptr(big[1]), _ptr(big[2]), 0, 0, 0)
        ctx.trace_rows_device(0, P, _ptr(d[1]), _ptr(d[2]), tr.data_ptr(), 63, 0)
        torch.cuda.synchronize(_dev())
        _compare(tr, V, idx, "after a refused witness call")
        assert bool((tr[P:] == SENTINEL).all())
        del keep


# ---- one commit over launch-graph rows
def test_header_cap_after_the_launch_graph(tmx, oracle):
    """the commit pipeline's cap of the header section (T.6) of the 24-proof launch-graph batch equals the oracle chain's
    (test_commit_pipeline.py) over the oracle's rows"""
    import torch
    V = _variants(oracle, 0, 128)
    P, sec, log_blowup, cap_h = 24, 32, 1, 2
    idx = _order(V.V, P, 1)
    with tmx.Context(128, CID, max_batch=P) as ctx:
        tr = _rows(ctx, 0, P)
        _trace(ctx, V, idx, tr)
        _compare(tr, V, idx, "header cap rows")
        cap = torch.zeros(4 << cap_h, dtype=torch.int64, device=_dev())
        ctx.trace_commit_device(0, P, sec, log_blowup, cap_h, tr.data_ptr(), cap.data_ptr(), 0)
        torch.cuda.synchronize(_dev())
        got = cap.cpu().numpy().view(np.uint64).reshape(-1, 4)
    off, rows, width = _section_geom(0, 128, sec)
    log_n = max(6, (rows - 1).bit_length())
    cols = np.zeros((P * width, 1 << log_n), dtype=np.uint64)
    for p in range(P):
        cols[p * width:(p + 1) * width, :rows] = V.rows[idx[p]][off:off + rows * width].reshape(rows, width).T
    ext = oracle.lde(cols, log_blowup)
    levels = oracle.poseidon_merkle(ext.reshape(-1), log_n + log_blowup, P * width, cap_h)
    assert np.array_equal(got, levels[-(1 << cap_h):])
