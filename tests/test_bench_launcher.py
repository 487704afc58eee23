"""bench.py --gpus N from a bare shell (missing 1): the script starts its own ranks as a fresh child under
torch.distributed.run, hands its arguments on unchanged and leaves with the child's exit code.  CPU only: on this box
the ranks stop at "needs an MI355X", which is exactly the relay being tested."""
import os
import subprocess
import sys

from conftest import ROOT

sys.path.insert(0, ROOT)


def test_launcher_command_relays_every_argument():
    import bench
    argv = ["--gpus", "4", "--steps", "7", "--warmup", "2", "--backend", "gloo", "--no-full-run", "--config", "c4"]
    cmd = bench.launcher_command(argv, 4, 29511)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29511"
    k = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[k + 1:] == argv                       # the script's own arguments, in order, after the script
    assert 1024 < bench.free_port() < 65536


def test_bare_gpus_flag_starts_the_ranks_and_relays_their_exit_code():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("a GPU is present: the GPU rehearsal covers this (tools/gloo2_rehearsal.sh)")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "2",
                        "--warmup", "1", "--no-full-run"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert "starting 2 ranks" in p.stderr and "--nproc-per-node 2" in p.stderr
    assert "needs an MI355X" in p.stderr              # the ranks ran bench.py with WORLD_SIZE set and said why they stop
    assert p.returncode != 0                          # ... and their failure is the launcher's exit code


def test_dump_outputs_writes_float_arrays_of_fixed_rows(tmp_path):
    """--dump-outputs: float32 stays float32, indices become float64, the sampled codebook rows are the same on every call,
    and the 64 MB bound is enforced before anything is written"""
    import numpy as np
    import pytest
    import bench
    rows = bench.sample_rows(65536, 512)
    assert len(rows) * 512 * 4 <= bench.DUMP_ROWS_BYTES and np.array_equal(rows, bench.sample_rows(65536, 512))
    assert np.all(np.diff(rows) > 0) and rows[-1] < 65536
    assert np.array_equal(bench.sample_rows(1000, 128), np.arange(1000))
    bench.dump_outputs(str(tmp_path / "d"), {"winner_index": np.arange(7, dtype=np.int64), "codebook": np.ones((3, 4), np.float32)})
    assert np.load(tmp_path / "d" / "winner_index.npy").dtype == np.float64
    assert np.load(tmp_path / "d" / "codebook.npy").dtype == np.float32
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_BYTES // 4 + 1, np.float32)})
    assert not (tmp_path / "big").exists()


def test_timed_batches_gives_exactly_the_steps_asked_for():
    """--steps K times exactly K batches: the wanted ones where they are distinct, the next free ones where several steps
    want the same batch, every batch (some more than once) when K exceeds the schedule's batches"""
    import bench
    assert bench.timed_batches([0, 3, 7, 9], 10) == [0, 3, 7, 9]
    assert bench.timed_batches([0, 0, 1, 1, 2], 10) == [0, 1, 2, 3, 4]
    assert bench.timed_batches([0, 8, 9, 9, 9], 10) == [0, 6, 7, 8, 9]
    for nb in (1, 7, 444):
        for K in (1, 2, nb, nb + 1, 3 * nb + 2):
            wanted = [(k * nb) // max(K, 1) for k in range(K)]
            got = bench.timed_batches(wanted, nb)
            assert len(got) == K and all(0 <= j < nb for j in got) and got == sorted(got)
            assert len(set(got)) == min(K, nb)
