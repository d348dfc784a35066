"""Openings of a proof-sharded commit at world = 2 on one GPU, through the stand-in RCCL of tests/fake_rccl (the pattern of
tests/test_world2_one_gpu.py): each rank opens the tree of its own proofs after tmx_trace_commit_sharded_device and verifies the openings
against slot `rank` of the gathered caps; a rank with an empty shard has nothing to open (tests/fake_rccl/open_worker.py)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

HERE = os.path.join(ROOT, "tests", "fake_rccl")


@pytest.mark.gpu
def test_each_rank_opens_its_own_shard(built_lib, oracle, tmp_path):
    so = str(tmp_path / "libfake_rccl.so")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "fake_rccl.c")])
    run_dir = tmp_path / "ranks"
    run_dir.mkdir()
    env = dict(os.environ, TMX_RCCL_LIB=so, FAKE_RCCL_DIR=str(run_dir), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "open_worker.py"), str(r), "2", str(run_dir)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r in range(2):
        path = run_dir / f"rank{r}.txt"
        res = path.read_text() if path.exists() else "FAIL\n(no result file)"
        assert res.startswith("ok"), f"rank {r}:\n{res}\n--- output ---\n{outs[r][-3000:]}"
        print(f"rank {r}: " + " | ".join(res.split("\n")[1:]))
    # P = 3 over two ranks: both open; n_total = 1: exactly one rank has an empty shard
    res = [(run_dir / f"rank{r}.txt").read_text() for r in range(2)]
    assert all("n_total=3: shard" in x for x in res)
    assert sum("n_total=1: empty shard" in x for x in res) == 1
