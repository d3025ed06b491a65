"""CPU: the order of device-table writes against the kernels that read the tables
(dpdk-tcpipstack_amd/csrc/rxg_tablesync.h).  tests/tablesync_check.cpp drives
rxg::TableSync and the real mirrors (rxg_mirror.h) against a recording device that knows which
operation is ordered before which, and asserts after every step: writes before later readers,
readers before later writes, patch and table buffers idle before they are rewritten or freed,
carried lists short and free of duplicate words, the device tables equal to the mirrors, and
the event a stream or the server waits for recorded after the carrying launch.  Built plain and
under ASan/UBSan (g++; the HIP headers only supply the vector types of rxg_common.h)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpdk-tcpipstack_amd", "csrc")
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]])
def test_table_write_ordering(tmp_path, san):
    exe = tmp_path / "tablesync_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *san, "-D__HIP_PLATFORM_AMD__",
                    "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-isystem", ROCM_INC,
                    os.path.join(ROOT, "tests", "tablesync_check.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "tablesync ok" in r.stdout, r.stdout + r.stderr
