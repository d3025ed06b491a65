"""GPU: rxg_tx_plan_dev on the deterministic sets of tests/txplan_cases.py -- send counts on both
sides of every tile and scan-round edge, slice-edge segment counts, flags, wraps, 64-bit offsets,
option blocks, refused sends, `cap` and the NULL arguments -- with every byte of segs, first,
next_seq and count compared to what the shipped host planner gives (tests/test_gpu_txplan.py:
run)."""
import pytest

import txplan_cases as tc
from test_gpu_txplan import run

pytestmark = pytest.mark.gpu

CASES = tc.all_cases()
LARGE = [c["name"] for c in CASES if tc.size_of(c) > tc.SMALL]
assert sorted(LARGE) == sorted(["big_alone", "big_between", "bytes_2^32-1", "one_segment_sends_2^16+1"] +
                               [f"round_{n}" for n in tc.ROUND_COUNTS])


def test_small_sets(engine):
    """Every set of at most 2^15 sends and segments, one call each."""
    ran = 0
    for c in CASES:
        if c["name"] not in LARGE:
            run(engine, c)
            ran += 1
    assert ran == len(CASES) - len(LARGE) > 40


@pytest.mark.parametrize("name", LARGE)
def test_large_sets(engine, name):
    """The sets that cross a scan round, a slice count of 2^14 and 2^32 bytes (up to 32 MiB of
    descriptors compared)."""
    run(engine, next(c for c in CASES if c["name"] == name))
