"""One rank of the world-2 opening run on a single GPU (tests/test_commit_open_world2.py starts two of these, as tests/test_world2_one_gpu.py
does with rank_worker.py): after tmx_trace_commit_sharded_device every rank opens ITS shard's tree (tmx_trace_commit_open_device), checks the
rows against the CPU oracle chain over its own proofs and verifies the openings on the device against slot `rank` of the gathered caps; with
n_total = 1 the rank with the empty shard has nothing to open (TMX_ERR_BAD_ARG).  Writes "ok" or a traceback to <outdir>/rank<r>.txt.
TEST INFRASTRUCTURE.  usage: open_worker.py <rank> <world> <outdir>"""
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle", "py"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from rank_worker import bootstrap_id, section_geom  # noqa: E402


def main():
    rank, world, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    import numpy as np
    import torch
    import oracle_c as oc
    import tendermintx_amd as tmx
    from tendermintx_amd import _lib, sharding
    from tendermintx_amd._lib import TmxError
    from tendermintx_amd.synth import Workload
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    uid = bootstrap_id(rank, outdir)
    log = []
    kind, n, P, sec, log_blowup, cap_h = 1, 4, 3, _lib.TRACE_SHA512, 2, 2
    wl = Workload(kind, n, P, n, chain_id=b"celestia", seed=2024, signed_permille=900)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (wl.proofs, wl.targets)]
    off, rows, width = section_geom(kind, n, sec)
    log_m = max(6, (rows - 1).bit_length()) + log_blowup
    with tmx.Context(n, b"celestia", device=0, max_batch=P) as ctx:
        # every rank computes the rows of the whole batch locally; the sharded commit takes its own proofs' rows out of them
        out = torch.zeros((P, ctx.elem_stride(kind)), dtype=torch.int64, device=dev)
        rep = torch.zeros(P * 64, dtype=torch.uint8, device=dev)
        tr = torch.zeros((P, ctx.trace_elem_count(kind)), dtype=torch.int64, device=dev)
        ctx.witness_batch_device(kind, P, d[0].data_ptr(), d[1].data_ptr(), None, out.data_ptr(), rep.data_ptr(), 0)
        ctx.trace_rows_device(kind, P, d[1].data_ptr(), None, tr.data_ptr(), _lib.TRACE_ALL, 0)
        torch.cuda.synchronize(dev)
        trh = tr.cpu().numpy().view(np.uint64)
        for p in range(P):
            pr, tg = wl.proofs[2336 * p:2336 * (p + 1)], wl.targets[256 * n * p:256 * n * (p + 1)]
            assert np.array_equal(trh[p], oc.trace(kind, pr, tg, None, n)), f"trace rows of proof {p} differ from the oracle's"
        ctx.comm_create(uid, rank, world)
        for n_total in (P, 1):
            lo, hi = sharding.shard_range(n_total, rank, world)
            caps = torch.zeros((world, 4 << cap_h), dtype=torch.int64, device=dev)
            ctx.trace_commit_sharded_device(kind, n_total, sec, log_blowup, cap_h, tr.data_ptr(), caps.data_ptr(), stream=0)
            torch.cuda.synchronize(dev)
            if hi == lo:
                sentinel = torch.full((2, 4), 77, dtype=torch.int64, device=dev)
                for call in (lambda: ctx.trace_commit_open_device([0, 1], sentinel.data_ptr(), sentinel.data_ptr(), 0), ctx.trace_commit_last_shape):
                    try:
                        call()
                        raise AssertionError("an empty shard opened something")
                    except TmxError as e:
                        assert e.status == -1, e
                torch.cuda.synchronize(dev)
                assert (sentinel.cpu().numpy() == 77).all()
                log.append(f"n_total={n_total}: empty shard, nothing to open")
                continue
            assert ctx.trace_commit_last_shape() == (log_m, (hi - lo) * width, cap_h)
            n_cols = (hi - lo) * width
            rng = np.random.default_rng(rank + 10 * n_total)
            idx = [0, (1 << log_m) - 1] + [int(x) for x in rng.integers(0, 1 << log_m, 14)]
            d_rows = torch.zeros((len(idx), n_cols), dtype=torch.int64, device=dev)
            d_paths = torch.zeros((len(idx), log_m - cap_h, 4), dtype=torch.int64, device=dev)
            ctx.trace_commit_open_device(idx, d_rows.data_ptr(), d_paths.data_ptr(), 0)
            ok = torch.zeros(len(idx), dtype=torch.int32, device=dev)
            ctx.poseidon_merkle_verify_device(log_m, n_cols, cap_h, caps[rank].data_ptr(), idx, d_rows.data_ptr(), d_paths.data_ptr(), ok.data_ptr(), 0)
            torch.cuda.synchronize(dev)
            assert (ok.cpu().numpy() == 1).all(), f"openings of rank {rank} against cap slot {rank}: {ok.cpu().numpy()}"
            cols = np.zeros((n_cols, 1 << (log_m - log_blowup)), dtype=np.uint64)
            for j, p in enumerate(range(lo, hi)):
                cols[j * width:(j + 1) * width, :rows] = trh[p][off:off + rows * width].reshape(rows, width).T
            ext = np.ascontiguousarray(oc.lde(cols, log_blowup)).reshape(n_cols, 1 << log_m)
            got = d_rows.cpu().numpy().view(np.uint64)
            for q, i in enumerate(idx):
                assert np.array_equal(got[q], ext[:, i]), f"row {i} of rank {rank}'s tree differs from the oracle chain"
            if world > 1:  # another rank's cap does not take this rank's openings
                other = (rank + 1) % world
                ctx.poseidon_merkle_verify_device(log_m, n_cols, cap_h, caps[other].data_ptr(), idx, d_rows.data_ptr(), d_paths.data_ptr(), ok.data_ptr(), 0)
                torch.cuda.synchronize(dev)
                assert (ok.cpu().numpy() == 0).all()
            log.append(f"n_total={n_total}: shard [{lo},{hi}) opened, {len(idx)} queries verified against cap slot {rank}")
    return log


if __name__ == "__main__":
    rank, outdir = int(sys.argv[1]), sys.argv[3]
    try:
        msg = "ok\n" + "\n".join(main())
    except BaseException:
        msg = "FAIL\n" + traceback.format_exc()
    with open(os.path.join(outdir, f"rank{rank}.txt"), "w") as f:
        f.write(msg)
    sys.exit(0 if msg.startswith("ok") else 1)
