"""CPU: what a replay hands out (dpdk-tcpipstack_amd/csrc/rxg_attached.h) against its
model.  tests/attached_check.cpp plays a script of attach, replay and take calls over the real
rxg::ReplayAttached and rxg::RcvWindow (with the real rxg::ReplayLog, rxg::WriteSet and
rxg::TcbMirror beside them) and prints every answer; asserted equal, line by line, to what the model
of tests/attached_cases.py answers for the same script: the prebuilt resets' slot and bytes, the
options' record, the summary and packet, the train and position, the ACK's frame, and the
receive window's takes.  Every set asserts on itself that it reaches the edges it is named for.
Built plain and under ASan/UBSan (g++; of the library only the stand-alone rxg_txresetid.cpp is
compiled in, the HIP headers only supply the vector types of rxg_common.h); every attached array is a
heap block of exactly its own length, so an index past an attachment's end is an error there."""
import os
import subprocess

import pytest

import attached_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpdk-tcpipstack_amd", "csrc")
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
SANS = {"plain": [], "san": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """san -> the program built that way, on first use."""
    d, built = tmp_path_factory.mktemp("attached_check"), {}

    def get(san):
        if san not in built:
            exe = d / ("attached_check_" + san)
            subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SANS[san],
                            "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-isystem",
                            ROCM_INC, os.path.join(ROOT, "tests", "attached_check.cpp"),
                            os.path.join(CSRC, "rxg_txresetid.cpp"), "-o", str(exe)], check=True)
            built[san] = str(exe)
        return built[san]

    return get


@pytest.mark.parametrize("san", list(SANS))
@pytest.mark.parametrize("name", ac.ALL)
def test_answers_equal_model(exes, tmp_path, name, san):
    script, want = ac.build(name)
    path = tmp_path / "script.txt"
    path.write_text(script)
    r = subprocess.run([exes(san), str(path)], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = r.stdout.splitlines()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, "answer %d" % k, g, w)
    assert len(got) == len(want)


def test_every_set_is_run():
    """Every set of the cases module is in test_answers_equal_model's parametrisation, once per build."""
    marks = [m for m in test_answers_equal_model.pytestmark if m.name == "parametrize"]
    by_arg = {m.args[0]: list(m.args[1]) for m in marks}
    assert sorted(by_arg["name"]) == sorted(ac.SETS) and len(set(by_arg["name"])) == len(ac.ALL)
    assert by_arg["san"] == ["plain", "san"]
