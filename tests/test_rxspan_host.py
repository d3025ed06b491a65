"""The receive-span case builders (rxspan_cases.py) against the CPU oracle and the pure-Python
checksum restatement (pktgen.py), frame by frame: the inputs of test_gpu_rxspan.py are what
they claim to be, and the oracle the GPU is compared with agrees with a second restatement on
every cell of the grid.  No GPU."""
import numpy as np
import pytest

import oracle
import pktgen
import rxspan_cases as cases


def _oracle(rows, frames):
    arena, off, lens = pktgen.pack_arena(frames)
    tcb, live = pktgen.table_arrays(rows)
    exp, cnt = oracle.rx_batch(arena, off, lens, tcb, live)
    return exp, cnt, (arena, off, lens)


def _check_against_python(frames, exp):
    """The oracle's two checksum fields are the Python restatement's, frame by frame (a frame
    that is not TCP is dropped before the TCP checksum, ip.c:36-39: its record holds 0)."""
    assert all(f[12:14] == b"\x08\x00" for f in frames)
    ip = np.array([pktgen.ip_checksum_of(f) for f in frames], dtype=np.uint16)
    tcp = np.array([pktgen.tcp_checksum_of(f) if f[23] == 6 else 0 for f in frames], dtype=np.uint16)
    for name, want in (("ip_cksum", ip), ("tcp_cksum", tcp)):
        bad = np.nonzero(exp["c"][name] != want)[0]
        assert len(bad) == 0, (f"oracle {name} differs from the Python restatement at {len(bad)} frames, first "
                               f"{cases.describe(frames[int(bad[0])])}: {exp['c'][name][bad[0]]:#06x} != {want[bad[0]]:#06x}")


@pytest.fixture(scope="module")
def grid():
    rows, frames = cases.span_grid()
    exp, cnt, packed = _oracle(rows, frames)
    return rows, frames, exp, packed


def test_grid_shape():
    """The recipe: per class the lengths at its ends and around every multiple of 16, per length
    the 19 total_length values that fit; one burst of the session engine."""
    rows, frames = cases.span_grid()
    nbytes = sum((len(f) + 63) // 64 * 64 for f in frames)
    print(f"span grid: {len(frames)} frames, {sum(map(len, frames))} bytes, {nbytes} in the pool")
    assert len(frames) <= 1 << 16 and nbytes <= 64 << 20
    assert cases.grid_lengths(0) == [63, 64]
    assert cases.grid_lengths(4) == [513, 514, 527, 528, 529, 543, 544, 545, 559, 560, 561, 575, 576]
    assert cases.grid_total_lengths(100) == [0, 1, 19, 20, 21, 33, 34, 35, 39, 40, 41, 69, 70, 71, 85, 86, 87, 102, 65535]
    for k, (lo, hi, _lpf) in enumerate(cases.CLASSES):
        ls = cases.grid_lengths(k)
        assert ls[0] == (63 if k == 0 else lo) and ls[-1] == hi
        assert all(cases.class_of(x) == k for x in ls)
        assert {m + d for m in range(64, hi + 1, 16) if m >= lo for d in (-1, 0, 1) if lo <= m + d <= hi} <= set(ls)
    by = cases.class_slices(frames)
    assert sorted(by) == list(range(len(cases.CLASSES)))
    for k, fs in by.items():
        assert {len(f) for f in fs} == set(cases.grid_lengths(k))
        for f in fs:
            assert cases.total_length_of(f) in cases.grid_total_lengths(len(f))
    # deterministic: a second build gives the same bytes
    cases._span_grid.cache_clear()
    assert cases.span_grid()[1] == frames


def test_grid_oracle_against_python(grid):
    rows, frames, exp, _ = grid
    _check_against_python(frames, exp)
    assert (exp["c"]["verdict"] <= 2).all()  # every frame reaches the TCP checksum


def test_grid_checksums_verify_where_the_field_is_in_the_span(grid):
    rows, frames, exp, _ = grid
    c = exp["c"]
    assert (c["ip_cksum"] == 0).all(), f"{(c['ip_cksum'] != 0).sum()} grid frames with a bad ip checksum"
    inside = np.array([min(len(f), max(34, 14 + cases.total_length_of(f))) >= 52 for f in frames])
    ok = c["tcp_cksum"] == 0
    print(f"span grid: {len(frames)} frames, {(~inside).sum()} with the checksum field outside the span, "
          f"{(np.array([cases.tcp_end_of(f) < len(f) for f in frames])).sum()} with tcp_end < len")
    bad = np.nonzero(ok != inside)[0]
    assert len(bad) == 0, f"{len(bad)} frames, first {cases.describe(frames[int(bad[0])])}: tcp_cksum {c['tcp_cksum'][bad[0]]:#06x}"
    assert ((c["flags"] & 2) != 0).tolist() == inside.tolist()  # RXG_F_TCP_OK follows


def test_grid_interleaved_is_the_same_set_with_mixed_rounds():
    rows, frames = cases.span_grid()
    rows2, inter = cases.span_grid_interleaved()
    assert rows2 == rows and sorted(inter) == sorted(frames) and inter != frames
    assert [cases.class_of(len(f)) for f in inter] == [cases.class_of(len(f)) for f in frames]
    # as generated the rounds of the streaming classes are mostly uniform; interleaved every
    # class but jumbo (one frame per round) has rounds holding both kinds
    assert cases.mixed_round_classes(inter) >= set(range(cases.JUMBO))
    nmixed = {k: 0 for k in range(cases.JUMBO)}
    for k, fs in cases.rounds_of(inter):
        if k != cases.JUMBO and len({cases.tcp_end_of(f) < len(f) for f in fs}) == 2:
            nmixed[k] += 1
    print("mixed rounds per class:", nmixed)
    assert all(v >= 1 for v in nmixed.values())
    uniform = sum(1 for k, fs in cases.rounds_of(frames) if len({cases.tcp_end_of(f) < len(f) for f in fs}) == 1)
    assert uniform > 1000


def test_small_layouts():
    rows, all_small, mixed = cases.small_layouts()
    assert len(all_small) == len(mixed) == 4096
    small = {f for f in cases.span_grid()[1] if len(f) <= 64}
    assert len(small) == 33 and small == set(all_small) and small <= set(mixed)
    for s in range(0, 4096, 64):
        assert max(map(len, all_small[s:s + 64])) <= 64 < max(map(len, mixed[s:s + 64]))


def test_grid_tx_oracle_reproduces_python_checksums(grid):
    """oracle.tx_batch over the grid with both fields zeroed gives back the frames as the Python
    functions filled them (every grid frame holds both fields), and touches nothing else."""
    rows, frames, _, (arena, off, lens) = grid
    zarena, zoff, zlens = pktgen.pack_arena([cases.zeroed_fields(f) for f in frames])
    assert np.array_equal(zoff, off) and np.array_equal(zlens, lens) and not np.array_equal(zarena, arena)
    got = oracle.tx_batch(zarena, zoff, zlens)
    if got.tobytes() != arena.tobytes():
        bad = np.nonzero(got != arena)[0]
        slot = int(bad[0]) // 64
        i = int(np.searchsorted(off, slot, side="right")) - 1
        raise AssertionError(f"tx oracle differs at {len(bad)} bytes, first in {cases.describe(frames[i])}, "
                             f"byte {int(bad[0]) - int(off[i]) * 64}")


@pytest.mark.parametrize("shorten", [0, 40])
def test_flip_set_rules(shorten):
    """One flipped bit changes one 16-bit word by +-1 or +-256, never 0x0000 into 0xFFFF, so the
    folded sum always changes: p in 14..33 -> ip_cksum != 0; p in [26, tcp_end) -> tcp_cksum
    differs from the baseline's, so != 0 wherever the baseline verifies; p >= tcp_end -> both
    fields as the baseline's."""
    rows, frames, base_of = cases.flip_set(shorten)
    exp, _, _ = _oracle(rows, frames)
    print(f"flip set (total_length - {shorten}): {len(frames)} frames, {sum(map(len, frames))} bytes")
    assert len(frames) == sum(n - 14 + 1 for n in cases.FLIP_LENGTHS)
    _check_against_python(frames, exp)
    cases.check_flip_rules(frames, base_of, exp["c"], shorten)


def test_extreme_set():
    rows, frames, kinds = cases.extreme_set()
    exp, _, _ = _oracle(rows, frames)
    _check_against_python(frames, exp)
    c = exp["c"]
    assert {len(f) for f, k in zip(frames, kinds) if k.startswith("fill")} == {9018, 65535}
    for i, (f, k) in enumerate(zip(frames, kinds)):
        assert c["ip_cksum"][i] == 0, (k, cases.describe(f))
        if k != "fill":
            assert c["tcp_cksum"][i] == 0, (k, cases.describe(f))
        if k.startswith("fill"):
            body = set(f[34:50] + f[52:])
            assert body in ({0xFF}, {0x00})
        if k == "tcp_0000":
            assert f[50:52] == b"\0\0" and frames[i + 1][50:52] == b"\xff\xff" and kinds[i + 1] == "tcp_ffff"
            assert frames[i + 1][:50] == f[:50] and frames[i + 1][52:] == f[52:]
        if k == "ip_0000":
            assert f[24:26] == b"\0\0" and frames[i + 1][24:26] == b"\xff\xff" and kinds[i + 1] == "ip_ffff"
    per_class = {cases.class_of(len(f)) for f, k in zip(frames, kinds) if k == "tcp_0000"}
    assert per_class == set(range(len(cases.CLASSES)))
    # the largest sum met: 0xFF from 34 to the end of a 65535-byte frame
    big = [f for f, k in zip(frames, kinds) if k == "fill" and len(f) == 65535 and f[60] == 0xFF]
    assert len(big) == 2 and {cases.tcp_end_of(f) for f in big} == {65535}
    # tx generate over the zeroed-field copies: the verifying members come back as they were
    valid = [f for f, k in zip(frames, kinds) if k not in ("fill", "tcp_ffff", "ip_ffff")]
    zarena, off, lens = pktgen.pack_arena([cases.zeroed_fields(f) for f in valid])
    assert oracle.tx_batch(zarena, off, lens).tobytes() == pktgen.pack_arena(valid)[0].tobytes()
