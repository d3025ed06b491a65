"""GPU: a plain `bench.py` run end to end at a small size: it times exactly --steps steps,
measures nothing beside the headline, and --dump-outputs writes the records its last timed
step produced -- checked against the oracle over the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_steps_records(tmp_path):
    import bench
    import oracle
    import rxg
    steps, warmup, n = 3, 2, 5000  # 5 launches over the 2 rotating batches: the last reads batch 0
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--frames", str(n), "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    (line,) = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0
    assert line["counters"]["rx"] == steps * n and line["counters_ok"] is True  # the timed steps, no more
    assert line["full"] is False and line["legs"] == {} and line["cpu_baseline"] is None
    assert line["roofline"]["kernel_us_per_launch_pairs_rank0_median"] is None
    assert line["dumped_outputs"] == {"dir": str(tmp_path), "records": [n, 2], "sampled": False}
    got = np.load(tmp_path / "records.npy")
    cnt = np.load(tmp_path / "counters.npy")
    assert got.dtype == np.float64 and got.shape == (n, 2) and cnt.dtype == np.float64
    assert [int(c) for c in cnt] == [line["counters"][k] for k in rxg.COUNTERS]

    # the same batch again (the bench's seeds), through the oracle
    with rxg.Engine(device=0, max_batch=1 << 16, max_bytes=64 << 20) as eng:
        wl = bench.Workload(eng, "c3_1500B_1Kflows", n, bench.shard_seed(0x5EED0001, 0), rxg.REC8)
        b = wl.batches[(warmup + steps - 1) % wl.copies]
        arena = b["arena"].download(np.uint8, b["arena_bytes"])
        off = b["off64"].download(np.uint32, n)
        lens = b["len"].download(np.uint16, n)
        wl.free()
    tcb, live = rxg.synthetic_tcb_table(1000)
    exp, _ = oracle.rx_batch(arena, off, lens, tcb, live)
    exp8 = rxg.rec8_pack(exp["c"])
    assert np.array_equal(got[:, 0], exp8["w0"].astype(np.float64))
    assert np.array_equal(got[:, 1], exp8["w1"].astype(np.float64))
    assert (exp["c"]["verdict"] == rxg.V_DISPATCH).all()  # every frame an exact hit, as counters_ok says
