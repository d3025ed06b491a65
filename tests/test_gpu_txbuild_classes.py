"""GPU: rxg_tx_build_dev in every size class and under a capped grid.  test_gpu_txbuild.py
draws its lengths from txbuild_ref.LENGTHS, which reach the classes of 0, 4, 32 and 64 lanes
per frame only, and runs on the occupancy grid, where a wave sees one slice.  Here: both ends
of all six classes (txbuild_ref.CLASS_LENGTHS), slices of one class and of all six, a grid of
1 and 2 workgroups whose waves take several slices, checksums at their extreme values, and
segments at the payload's two ends.  As there, every expectation is the model's
(txbuild_ref.build), every pool is pre-filled and compared whole, byte for byte."""
import numpy as np
import pytest

import rxg
import txbuild_ref as ref
from test_gpu_txbuild import FILL, _peer_tcbs, explain, run

pytestmark = pytest.mark.gpu

SMALL_MAX = 2731  # lengths stay at or below this except where a test says otherwise
ONE_PER_CLASS = [7, 139, 331, 715, 1483, 2731]


@pytest.fixture(scope="module")
def flows():
    return ref.make_flows(8)


@pytest.fixture(scope="module")
def payload():
    return np.random.default_rng(41).integers(0, 256, 1 << 17, dtype=np.uint8)


def check(eng, payload, flows, segs, off, nslots, lens, what="", model=None, **kw):
    """One build on `eng` against the model's (`model`: ref.build's result where several
    engines share it): len, the whole pool, stats.  Returns the pool."""
    stats0 = kw.get("stats0", (0, 0))
    pbytes = kw.get("payload_bytes", len(payload))
    nflows = kw.get("nflows", len(flows))
    want, wlen, wstats = model or ref.build(payload[:pbytes], flows[:nflows], segs, off, nslots, fill=FILL)
    got, glen, gstats = run(eng, payload, flows, segs, nslots, off64=off, **kw)
    assert np.array_equal(glen, wlen), what
    assert np.array_equal(got, want), what + " " + explain(got, want, off, lens)
    assert [int(x) for x in gstats] == [int(wstats[0]) + stats0[0], int(wstats[1]) + stats0[1]], what
    return got


def classes_of(lens):
    return [ref.lanes_per_frame(x) for x in lens]


# ------------------------------------------------ a. class ends x source alignment ---
@pytest.fixture(scope="module")
def class_case(flows, payload):
    """CLASS_LENGTHS x the 16 source alignments, packed back to back in a random order."""
    lens = np.repeat(ref.CLASS_LENGTHS, 16)
    r = np.random.default_rng(42)
    base = r.integers(0, (len(payload) - SMALL_MAX - 16) // 16, len(lens)) * 16
    segs = ref.make_segs(lens, base + np.tile(np.arange(16), len(ref.CLASS_LENGTHS)), len(flows), seed=43)
    off, nslots = ref.packed_offsets(lens, r.permutation(len(lens)))
    return lens, segs, off, nslots + 2


def test_class_ends_and_alignments_byte_exact(engine, flows, payload, class_case):
    lens, segs, off, nslots = class_case
    assert set(classes_of(lens)) == set(ref.CLASSES)
    for L in ref.CLASS_LENGTHS:
        assert sorted(int(s) % 16 for s in segs["src_off"][lens == L]) == list(range(16)), L
    check(engine, payload, flows, segs, off, nslots, lens)
    assert len(lens) == 16 * len(ref.CLASS_LENGTHS)


# ------------------------------------------------ b. uniform and ragged slices ---
def draw_in_class(r, cls, n):
    """n lengths of one class, its two ends among them (and nothing else above SMALL_MAX)."""
    lo, hi = ref.CLASS_RANGE[cls]
    lens = r.integers(lo, min(hi, SMALL_MAX) + 1, n)
    if n >= 2:
        at = r.choice(n, 2, replace=False)
        lens[at[0]], lens[at[1]] = lo, hi
    return lens


@pytest.mark.parametrize("cls", ref.CLASSES)
def test_slices_of_one_class(engine, flows, payload, cls):
    """Two full slices of one class (no lane compaction) and a partial one."""
    r = np.random.default_rng(50 + cls)
    lens = np.concatenate([draw_in_class(r, cls, 64), draw_in_class(r, cls, 64), draw_in_class(r, cls, 17)])
    n = len(lens)
    assert n == 64 + 64 + 17 and set(classes_of(lens)) == {cls}
    segs = ref.make_segs(lens, r.integers(0, len(payload) - rxg.TX_MAX_DATA, n), len(flows), seed=60 + cls)
    off, nslots = ref.packed_offsets(lens, r.permutation(n))
    check(engine, payload, flows, segs, off, nslots + 1, lens)


def test_one_slice_of_all_six_classes(engine, flows, payload):
    """Per-class counts that end inside a round of 64 / LPF frames, lanes interleaved."""
    counts = {64: 1, 32: 3, 16: 5, 8: 9, 4: 17, 0: 29}
    r = np.random.default_rng(70)
    lens = np.concatenate([draw_in_class(r, c, k) for c, k in counts.items()])
    lens[0] = SMALL_MAX  # the one class-64 frame
    lens = lens[r.permutation(64)]
    cl = classes_of(lens)
    assert len(lens) == 64 and {c: cl.count(c) for c in counts} == counts
    assert sum(a != b for a, b in zip(cl, cl[1:])) > 32  # interleaved, not sorted
    segs = ref.make_segs(lens, r.integers(0, len(payload) - SMALL_MAX, 64), len(flows), seed=71)
    off, nslots = ref.packed_offsets(lens, r.permutation(64))
    check(engine, payload, flows, segs, off, nslots + 1, lens)


# ------------------------------------------------ c. capped grid ---
@pytest.fixture(scope="module")
def grids(engine):
    """Contexts whose launches are capped at 1 and 2 workgroups, and the occupancy grid."""
    e1, e2 = rxg.Engine(device=0, max_blocks=1), rxg.Engine(device=0, max_blocks=2)
    yield [("max_blocks 1", e1), ("max_blocks 2", e2), ("occupancy grid", engine)]
    e1.close()
    e2.close()


def test_capped_grid_several_slices_per_wave(grids, payload):
    """805 segments on 4 waves (max_blocks 1: wave 0 takes slices 0, 4, 8, 12, the others
    three), on 8 and on the occupancy grid: the same pool, the model's."""
    flows = ref.make_flows(9)  # one entry more than the bound passed
    nflows, pbytes = 8, 40000  # and payload past the bound passed
    n = 64 * 4 * 3 + 37
    r = np.random.default_rng(80)
    lens = r.choice(ref.CLASS_LENGTHS, n)
    hist = [sorted(classes_of(lens[s * 64:s * 64 + 64])) for s in range(13)]
    assert all(hist[s] != hist[s + 4] for s in range(9)) and all(hist[s] != hist[s + 8] for s in range(5))
    segs = ref.make_segs(lens, r.integers(0, pbytes - SMALL_MAX, n), nflows, seed=81)
    off, nslots = ref.packed_offsets(lens, r.permutation(n))  # (slots by the lengths before the skips)
    # skipped descriptors in the first, second, third and fourth slice of a wave of 4
    bad_flow = [64 * 1 + 3, 64 * 9 + 5, n - 1]
    bad_len = [0, 64 * 8 + 17, 64 * 6 + 63]
    bad_off = [64 * 2 + 1, 64 * 10 + 33, 64 * 3, 64 * 11 + 63]
    edge = [64 * 4 + 9, 64 * 12 + 2]  # src_off + data_len == payload_bytes exactly: built
    segs["flow"][bad_flow] = nflows
    segs["data_len"][bad_len] = rxg.TX_MAX_DATA + 1
    for i in bad_off:
        segs["src_off"][i] = pbytes + 1 - int(segs["data_len"][i])
    for i in edge:
        segs["src_off"][i] = pbytes - int(segs["data_len"][i])
    skipped = sorted(bad_flow + bad_len + bad_off)
    assert len(set(skipped + edge)) == 12 and len(payload) >= pbytes + (64 << 10)
    model = ref.build(payload[:pbytes], flows[:nflows], segs, off, nslots + 1, fill=FILL)
    _, wlen, wstats = model
    assert sorted(np.nonzero(wlen == 0)[0]) == skipped and list(wstats) == [n - 10, 10]
    pools = []
    for name, eng in grids:
        got = check(eng, payload, flows, segs, off, nslots + 1, lens, name, model, nflows=nflows,
                    payload_bytes=pbytes, stats0=(5, 7))
        for i in skipped:
            a = int(off[i]) * 64
            assert (got[a:a + int(ref.slots_of(lens[i:i + 1])[0]) * 64] == FILL).all(), (name, i)
        pools.append(got)
    assert np.array_equal(pools[0], pools[1]) and np.array_equal(pools[0], pools[2])


def test_capped_grid_pure_acks(grids, flows):
    """2561 segments without data at one slot each: 41 slices on 8 waves."""
    n = 64 * 8 * 5 + 1
    lens = np.zeros(n, dtype=np.int64)
    segs = ref.make_segs(lens, np.zeros(n, dtype=np.int64), len(flows), seed=85)
    off = (3 + np.arange(n)).astype(np.uint32)
    want, wlen, _ = ref.build(np.zeros(16, np.uint8), flows, segs, off, n + 5, fill=FILL)
    for name, eng in grids[1:]:
        got, glen, gstats = run(eng, np.zeros(16, np.uint8), flows, segs, n + 5, slot0=3, stride64=1, stats0=(5, 7))
        assert np.array_equal(glen, wlen), name
        assert np.array_equal(got, want), name + " " + explain(got, want, off, lens)
        assert list(gstats) == [5 + n, 7], name


# ------------------------------------------------ d. checksum extremes ---
@pytest.mark.parametrize("inside,outside", [(0xFF, 0x00), (0x00, 0xFF)])
def test_segment_bytes_against_their_surroundings(engine, flows, inside, outside):
    """Every segment's bytes are `inside`, every other byte of the payload `outside`: 0xFF
    inside drives each 16-bit add to its largest value; 0x00 inside shows any byte taken from
    outside [src_off, src_off + L) in the frame's padding and in its checksum."""
    lens = np.repeat(ref.CLASS_LENGTHS, 16)
    align = np.tile(np.arange(16), len(ref.CLASS_LENGTHS))
    so, cursor = [], 0
    for L, a in zip(lens, align):
        so.append(cursor + 32 + int(a))
        cursor += 32 + (int(a) + int(L) + 15) // 16 * 16 + 32
    payload = np.full(cursor, outside, np.uint8)
    for L, o in zip(lens, so):
        payload[o:o + int(L)] = inside
    assert sum(1 for o in so if o % 16 < 6) and sum(1 for o in so if o % 16 >= 6)
    segs = ref.make_segs(lens, np.array(so), len(flows), seed=90 + inside)
    off, nslots = ref.packed_offsets(lens, np.random.default_rng(91).permutation(len(lens)))
    check(engine, payload, flows, segs, off, nslots + 1, lens)


def test_largest_sum(engine, flows):
    """RXG_TX_MAX_DATA bytes of 0xFF, at a source alignment on either side of 6, one of them
    under header fields of all ones."""
    lens = np.array([rxg.TX_MAX_DATA, rxg.TX_MAX_DATA])
    payload = np.full(rxg.TX_MAX_DATA + 16, 0xFF, np.uint8)
    segs = ref.make_segs(lens, np.array([3, 9]), len(flows), seed=95)
    segs["seq"][1], segs["ack"][1], segs["win_raw"][1] = 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFF
    segs["ip_id"][1], segs["tcp_flags"][1] = 0xFFFF, 0xFF
    off, nslots = ref.packed_offsets(lens)
    check(engine, payload, flows, segs, off, nslots + 1, lens)


def test_stored_checksums_of_zero(engine, flows):
    """One segment per class whose stored TCP checksum is 0x0000 (the folded sum 0xFFFF), and
    one whose IP header checksum is.  Found on the host: with the free 16-bit word (a payload
    word, ip_id) zero the stored checksum is the complement of the folded sum S of the rest,
    and S + ~S = 0xFFFF in one's complement, so the word wanted is that checksum's two bytes."""
    lens = np.array([10] + ONE_PER_CLASS[1:] + [331])
    n = len(lens)
    assert classes_of(lens[:6]) == ref.CLASSES
    payload = np.random.default_rng(96).integers(0, 256, n * 4096, dtype=np.uint8)
    so = np.arange(n) * 4096 + (5 * np.arange(n) + 1) % 16
    word = [int(o) + ((int(L) - 3) & ~1) for o, L in zip(so[:6], lens[:6])]  # an even payload offset, both bytes inside
    segs = ref.make_segs(lens, so, len(flows), seed=97)
    off, nslots = ref.packed_offsets(lens)
    for w in word:
        payload[w:w + 2] = 0
    segs["ip_id"][6] = 0
    pool, _, _ = ref.build(payload, flows, segs, off, nslots, fill=FILL)
    for i, w in enumerate(word):
        payload[w:w + 2] = pool[int(off[i]) * 64 + 50:int(off[i]) * 64 + 52]
    a = int(off[6]) * 64
    segs["ip_id"][6] = int(pool[a + 24]) | int(pool[a + 25]) << 8  # stored without a byte swap
    want, _, _ = ref.build(payload, flows, segs, off, nslots, fill=FILL)
    for i in range(6):
        assert not want[int(off[i]) * 64 + 50:int(off[i]) * 64 + 52].any(), i
    assert not want[a + 24:a + 26].any()
    check(engine, payload, flows, segs, off, nslots, lens)


# ------------------------------------------------ e. payload ends ---
def test_segments_at_the_payload_start(engine, flows):
    """src_off 0..15: the source chunk before the segment's first lies before the payload."""
    lens = np.repeat(ONE_PER_CLASS, 16)
    assert classes_of(ONE_PER_CLASS) == ref.CLASSES
    payload = np.random.default_rng(100).integers(0, 256, 4096, dtype=np.uint8)
    segs = ref.make_segs(lens, np.tile(np.arange(16), len(ONE_PER_CLASS)), len(flows), seed=101)
    off, nslots = ref.packed_offsets(lens, np.random.default_rng(102).permutation(len(lens)))
    check(engine, payload, flows, segs, off, nslots + 1, lens)


@pytest.mark.parametrize("pbytes", [4096, 4097, 4107])
def test_segments_ending_at_payload_bytes(engine, flows, pbytes):
    """Segments of every class length ending exactly at payload_bytes (data_len 0: src_off ==
    payload_bytes, built per include/rxg.h), the buffer's bytes from there to its end 0xEE, a
    value the payload does not hold: none of them may show in a frame."""
    assert pbytes % 16 in (0, 1, 11)
    data = np.random.default_rng(pbytes).integers(0, 256, pbytes, dtype=np.uint8)
    data[data == 0xEE] = 0x11
    buf = np.concatenate([data, np.full(16 - pbytes % 16, 0xEE, np.uint8)])
    assert len(buf) % 16 == 0 and len(buf) > pbytes
    lens = np.array(ref.CLASS_LENGTHS)
    segs = ref.make_segs(lens, pbytes - lens, len(flows), seed=pbytes + 1)
    assert int(segs["src_off"][0]) == pbytes and int(segs["data_len"][0]) == 0
    off, nslots = ref.packed_offsets(lens)
    got = check(engine, buf, flows, segs, off, nslots + 1, lens, payload_bytes=pbytes)
    for i, L in enumerate(lens):  # said on its own: the payload bytes are the source's last L
        a = int(off[i]) * 64 + 54
        assert np.array_equal(got[a:a + L], data[pbytes - L:]), i


# ------------------------------------------------ f. through the shipped receive path ---
def test_class_frames_through_rx_and_tx_cksum(engine, flows, payload, class_case):
    lens, segs, off, nslots = class_case
    pool = check(engine, payload, flows, segs, off, nslots, lens)
    flen = (54 + lens).astype(np.uint16)
    with rxg.Engine(device=0) as peer:
        peer.tcb_load(_peer_tcbs(flows), np.ones(len(flows), np.uint8))
        recs = peer.rx_arena(pool, off, flen, rxg.REC48)
    assert (recs["c"]["verdict"] == rxg.V_DISPATCH).all()
    assert (recs["c"]["flags"] & (rxg.F_IP_OK | rxg.F_TCP_OK) == rxg.F_IP_OK | rxg.F_TCP_OK).all()
    assert (recs["c"]["ip_cksum"] == 0).all() and (recs["c"]["tcp_cksum"] == 0).all()
    assert np.array_equal(recs["c"]["tcb_idx"], segs["flow"].astype(np.int32))
    assert np.array_equal(recs["c"]["datalen"], lens.astype(np.int32))
    assert np.array_equal(recs["seq"], segs["seq"]) and np.array_equal(recs["ack"], segs["ack"])
    again = engine.tx_arena(pool, off, flen)
    assert np.array_equal(again, pool)
