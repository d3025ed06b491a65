"""CPU: rxg_tx_plan_count (the segment count of a cut, the `n` of the build that follows
rxg_tx_plan_dev) against the shipped planners' return values, and rxg_dev_tx_plan at the C
boundary."""
import ctypes as C

import numpy as np
import pytest

import rxg

EINVAL = 22
MSS = 1460


@pytest.fixture(scope="module")
def lib():
    return rxg.load_library()


def table(seed=1):
    """Six valid blocks (len 0, 4, 8, 12, 28, 40) with garbage around `len`."""
    raw = np.random.default_rng(seed).integers(0, 256, (6, 48), dtype=np.uint8)
    raw[:, 0] = [0, 4, 8, 12, 28, 40]
    return np.ascontiguousarray(raw).view(rxg.TX_OPT_DTYPE).reshape(-1)


def random_sends(r, n, mss):
    raw = r.integers(0, 256, (n, 40), dtype=np.uint8)
    s = np.ascontiguousarray(raw).view(rxg.TX_SEND_DTYPE).reshape(-1)
    s["bytes"] = np.where(r.random(n) < 0.5, r.choice([0, 1, mss - 1, mss, mss + 1, 5 * mss, 70000], n),
                          r.integers(0, 200000, n))
    return s


def count(lib, sends, mss, so, opts, nopts=None):
    return lib.rxg_tx_plan_count(sends.ctypes.data if len(sends) else None, len(sends), mss,
                                 None if so is None else so.ctypes.data, opts.ctypes.data if len(opts) else None,
                                 len(opts) if nopts is None else nopts)


def plan(lib, sends, mss, so, opts, cap=1 << 16):
    out = np.zeros(cap, rxg.TX_SEG_DTYPE)
    return lib.rxg_tx_plan_opt(sends.ctypes.data if len(sends) else None, len(sends), mss,
                               None if so is None else so.ctypes.data, opts.ctypes.data if len(opts) else None,
                               len(opts), out.ctypes.data, cap, None)


def test_symbol_and_layout(lib):
    assert hasattr(lib, "rxg_tx_plan_count") and hasattr(lib, "rxg_tx_plan_dev")
    assert C.sizeof(rxg.DevTxPlan) == 80
    assert [(f, getattr(rxg.DevTxPlan, f).offset) for f, _ in rxg.DevTxPlan._fields_] == [
        ("sends", 0), ("nsends", 8), ("mss", 12), ("send_opt", 16), ("opts", 24), ("nopts", 32), ("pad", 36),
        ("segs", 40), ("cap", 48), ("first", 56), ("next_seq", 64), ("count", 72)]


def test_count_equals_the_planners_return_on_seeded_sets(lib):
    opts = table()
    checked = blocked = 0
    for seed in range(300):
        r = np.random.default_rng(seed)
        mss = int(r.choice([1, 41, 536, MSS, 9000, rxg.TX_MAX_DATA]))
        n = int(r.integers(0, 40))
        s = random_sends(r, n, mss)
        if seed % 5 == 0:
            s["bytes"] = r.integers(0, 1 << 16, n)
        if mss <= 41:  # (the planner's output of a set stays within plan()'s cap)
            s["bytes"] %= 3000
        for so in (None, r.integers(0, 2 if mss == 1 else len(opts) + 1, n).astype(np.uint32)):  # (O < mss)
            want = plan(lib, s, mss, so, opts, cap=1 << 18)
            assert want >= n
            before = (s.tobytes(), opts.tobytes())
            assert count(lib, s, mss, so, opts) == want, (seed, so is None)
            assert (s.tobytes(), opts.tobytes()) == before
            checked += 1
            blocked += so is not None and bool((so > 0).any())
    assert checked == 600 and blocked > 250
    # the wrapper of the binding
    s = random_sends(np.random.default_rng(7), 9, MSS)
    so = np.arange(9, dtype=np.uint32) % 7
    assert rxg.tx_plan_count(s, MSS, so, opts) == len(rxg.tx_plan_opt(s, MSS, so, opts)[0])
    assert rxg.tx_plan_count(s, MSS) == len(rxg.tx_plan(s, MSS)[0])
    # a count past 2^32: 2^10 sends of 2^32 - 1 bytes at mss 1
    big = np.zeros(1 << 10, rxg.TX_SEND_DTYPE)
    big["bytes"] = 0xFFFFFFFF
    assert rxg.tx_plan_count(big, 1) == (1 << 10) * 0xFFFFFFFF


def test_einval_cases_are_the_planners(lib):
    opts = table()
    bad = opts.copy()
    bad["len"][1], bad["len"][2] = 44, 6
    two = random_sends(np.random.default_rng(3), 2, MSS)
    cases = [
        (two, 0, None, opts, None), (two, rxg.TX_MAX_DATA + 1, None, opts, None),      # mss
        (two, 0, np.array([0, 0], np.uint32), opts, None),
        (two, MSS, np.array([0, 7], np.uint32), opts, None),                           # past nopts
        (two, MSS, np.array([1, 0], np.uint32), opts, 0),                              # nopts 0
        (two, MSS, np.array([2, 0], np.uint32), bad, None),                            # len 44
        (two, MSS, np.array([0, 3], np.uint32), bad, None),                            # len 6
        (two, 40, np.array([0, 6], np.uint32), opts, None),                            # mss == O
        (two, 12, np.array([5, 0], np.uint32), opts, None),                            # mss < O
    ]
    for s, mss, so, o, nopts in cases:
        want = plan(lib, s, mss, so, o) if nopts is None else \
            lib.rxg_tx_plan_opt(s.ctypes.data, 2, mss, so.ctypes.data, o.ctypes.data, nopts,
                                np.zeros(64, rxg.TX_SEG_DTYPE).ctypes.data, 64, None)
        assert want == -EINVAL
        assert count(lib, s, mss, so, o, nopts) == -EINVAL, (mss, so, nopts)
    so = np.array([1, 2], np.uint32)
    # a block named with a NULL table, NULL sends
    assert lib.rxg_tx_plan_count(two.ctypes.data, 2, MSS, so.ctypes.data, None, 6) == -EINVAL
    assert lib.rxg_tx_plan_count(None, 2, MSS, None, None, 0) == -EINVAL
    # not errors: no sends; a bad block nobody names; mss == O + 1
    assert lib.rxg_tx_plan_count(None, 0, MSS, None, None, 0) == 0
    assert count(lib, two, MSS, np.array([1, 4], np.uint32), bad) == plan(lib, two, MSS, np.array([1, 4], np.uint32), bad)
    assert count(lib, two, 41, np.array([6, 6], np.uint32), opts) == int(np.maximum(two["bytes"], 1).sum())
    with pytest.raises(rxg.RxgError):
        rxg.tx_plan_count(two, MSS, [7, 0], opts)
