"""CPU: the replay's staleness rule (dpdk-tcpipstack_amd/csrc/rxg_replaylog.h) against
its model.  tests/replaylog_check.cpp plays rxg_rx_replay's packet loop over the real rxg::ReplayLog
and rxg::WriteSet, with both classifiers replaced by a lookup of the frame's record at the table's
epoch, for every set of tests/replay_sel_cases.py on a default and a RXG_CFG_REPLAY_ON_DEVICE
context; asserted equal to Case.sim: per frame the epoch whose record its handler saw, every launch
as (burst, list), and the four rxg_replay_stats figures.  The program's two direct cases (two
tuples sharing a filter_hash, one written; a packet fixed at write s against writes <= s and a later
one) need no model.  Built plain and under ASan/UBSan (g++; nothing of the library is linked, the
HIP headers only supply the vector types of rxg_common.h); every frame is a heap block of its own
length, so a read past a short frame is an error there."""
import os
import struct
import subprocess

import numpy as np
import pytest

import replay_sel_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpdk-tcpipstack_amd", "csrc")
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
SANS = {"plain": [], "san": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
MAGIC = 0x31435052
HEAD = 54


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """san -> the program built that way, on first use."""
    d, built = tmp_path_factory.mktemp("replaylog_check"), {}

    def get(san):
        if san not in built:
            exe = d / ("replaylog_check_" + san)
            subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SANS[san],
                            "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-isystem",
                            ROCM_INC, os.path.join(ROOT, "tests", "replaylog_check.cpp"), "-o", str(exe)], check=True)
            built[san] = str(exe)
        return built[san]

    return get


def case_file(c: rc.Case, on_device: bool) -> bytes:
    sim = c.sim(on_device)
    nep = len(c.epochs)
    assert [i for i, _ in sim.touches] == sorted(c.writers) and len(sim.touches) + 1 == nep
    out = [struct.pack("<6I", MAGIC, c.n, len(c.bursts), nep, len(sim.touches), int(on_device)),
           np.array(c.lens, dtype="<u2").tobytes(),
           b"".join(f[:HEAD].ljust(HEAD, b"\0") for f in c.frames),
           np.array(c.bursts, dtype="<u4").tobytes()]
    for e in range(nep):
        recs = np.ascontiguousarray(c.cls(e))
        assert recs.dtype.itemsize == 16 and len(recs) == c.n
        out.append(recs.tobytes())
    for i, t in sim.touches:
        out.append(struct.pack("<5I", i, int(t.all), int(t.pass2), len(t.keys), len(t.listen)))
        out.append(np.array(t.keys, dtype="<u4").reshape(-1, 3).tobytes())
        out.append(np.array(t.listen, dtype="<i4").tobytes())
    return b"".join(out)


def run(exe, arg):
    r = subprocess.run([exe, str(arg)], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout


@pytest.mark.parametrize("san", list(SANS))
def test_direct_cases(exes, san):
    assert "direct ok" in run(exes(san), "direct")


@pytest.mark.parametrize("san", list(SANS))
@pytest.mark.parametrize("name", rc.ALL)
def test_log_equals_model(exes, tmp_path, name, san):
    c = rc.get(name)
    for on_device in (False, True):
        sim = c.sim(on_device)
        path = tmp_path / ("case_%d.bin" % on_device)
        path.write_bytes(case_file(c, on_device))
        seen, launches, stats = None, [], None
        for line in run(exes(san), path).splitlines():
            w = line.split()
            if w[0] == "seen":
                seen = [int(x) for x in w[1:]]
            elif w[0] == "launch":
                launches.append((int(w[1]), [int(x) for x in w[2:]]))
            elif w[0] == "stats":
                stats = dict(zip(("marked", "host_fixups", "device_fixups", "device_launches"), map(int, w[1:])))
        assert seen == sim.seen, (name, on_device)
        assert launches == sim.launches, (name, on_device)
        assert stats == sim.stats, (name, on_device, stats, sim.stats)


def test_every_set_is_run():
    """Every set of the cases module is in test_log_equals_model's parametrisation, once per build."""
    marks = [m for m in test_log_equals_model.pytestmark if m.name == "parametrize"]
    by_arg = {m.args[0]: list(m.args[1]) for m in marks}
    assert sorted(by_arg["name"]) == sorted(n for v in rc.NAMES.values() for n in v) and len(set(by_arg["name"])) == len(rc.ALL)
    assert by_arg["san"] == ["plain", "san"]
