"""CPU: the sets of tests/txbuild_opt_cases.py hold what they claim, asserted on the sets
themselves in forms no change of seed alters, and the model they are compared with
(txbuild_opt_ref.build) stands at every block length: its frames verify through the rx oracle
and the received-option model for O = 0, 4, .. 40, the four lengths the earlier tests never
built among them."""
import functools

import numpy as np
import pytest

import oracle
import rxg
import rxopt_ref
import txbuild_opt_cases as cases
import txbuild_opt_ref as oref

HDR = 54
ALL = oref.ALL_OPT_LENS
MAXD = rxg.TX_MAX_DATA


@functools.lru_cache(maxsize=None)
def get(name, *a):
    return getattr(cases, name)(*a)


@functools.lru_cache(maxsize=None)
def model(name, *a):
    return get(name, *a).model()


def geometry(c):
    """Per descriptor: O (-1: skipped for its block), data_len, src_off, H + L."""
    ol = c.opt_len()
    dl = c.segs["data_len"].astype(np.int64)
    return ol, dl, c.segs["src_off"].astype(np.int64), HDR + ol + dl


def frame(c, pool, i, n=None):
    a = int(c.off64[i]) * 64
    return pool[a:a + (n if n is not None else (int(HDR + c.opt_len()[i] + c.segs["data_len"][i]) + 63) // 64 * 64)]


def test_every_block_length_and_the_old_list_unchanged():
    assert list(ALL) == list(range(0, 44, 4))
    assert oref.OPT_LENS == [0, 4, 8, 12, 16, 28, 40] and set(oref.OPT_LENS) < set(ALL)
    t = cases.table()
    assert [int(t[cases.block_of(O) - 1]["len"]) for O in ALL] == list(ALL)


# ------------------------------------------------------------------------- masks ---
@pytest.mark.parametrize("O", ALL)
def test_masks_grid_is_complete(O):
    c = get("masks", O)
    ol, dl, so, hl = geometry(c)
    assert (ol == O).all() and len(dl) == 256 + 49 * 16
    g = slice(0, 256)
    # the smallest streamed frames: two lines, with data, every residue at every shift once
    assert ((hl[g] > 64) & (hl[g] <= 128) & (dl[g] >= 1)).all()
    pairs = set(zip((hl[g] % 16).tolist(), ((so[g] + 10 - O) % 16).tolist()))
    assert pairs == {(r, s) for r in range(16) for s in range(16)}
    for r in range(16):  # no smaller frame with data has the residue
        mine = hl[g][hl[g] % 16 == r]
        assert len(set(mine.tolist())) == 1 and not [x for x in range(max(65, HDR + O + 1), int(mine[0])) if x % 16 == r]
    # every data_len 0..48 at every source alignment
    assert sorted(zip(dl[256:].tolist(), (so[256:] % 16).tolist())) == [(L, a) for L in range(49) for a in range(16)]
    assert int(hl.max()) <= 192 == c.labels["stride64"] * 64
    one_line = hl[256:] <= 64
    assert one_line.sum() == (16 * (11 - O) if O <= 8 else 0)           # the whole one-line class
    assert ((dl[256:] == 0) & ~one_line).sum() == (16 if O >= 12 else 0)  # streamed without data
    if O == 0:  # with no block at all and with the block of no bytes, at every alignment
        for k in (0, 1):
            assert set((so[c.segs["reserved"] == k] % 16).tolist()) == set(range(16))
    else:
        assert (c.segs["reserved"] == cases.block_of(O)).all()
    assert int((so + dl).max()) <= len(c.payload)


def test_masks_put_both_masks_in_one_chunk_in_every_combination():
    """hb = H - 16 c bytes of chunk c are dropped, vb = H + L - 16 c kept; c = H // 16 is the
    chunk with the last option bytes.  With both inside one chunk (vb < 16) every pair of
    dwords they end in occurs for c = 3, 4 and 5, at all 16 alignments."""
    seen = {3: {}, 4: {}, 5: {}}
    for O in ALL:
        c = get("masks", O)
        _, dl, so, hl = geometry(c)
        H = HDR + O
        ch = H // 16
        assert ch == (3 if O <= 8 else 4 if O <= 24 else 5)
        hb = H - 16 * ch
        assert hb in (2, 6, 10, 14) and hb // 4 == {3: (O + 4) // 4, 4: (O - 12) // 4, 5: (O - 28) // 4}[ch]
        ce = hl // 16                                       # the chunk of the first byte past the payload
        for L, a, e in zip(dl.tolist(), (so % 16).tolist(), ce.tolist()):
            if e == ch:
                seen[ch].setdefault((hb // 4, (H + L - 16 * ch) // 4), set()).add(a)
        # the payload's last byte in that chunk, the next, the one after; and across a line edge
        last = (hl[dl > 0] - 1) // 16
        assert {0, 1, 2} <= set((last - ch).tolist())
        first_line, last_line = H // 64, (hl[dl > 0] - 1) // 64
        if O <= 8 or O >= 28:
            assert (last_line > first_line).any() and (last_line == first_line).any()
        for L in range(0, 16 - hb):                         # every length that keeps both masks in the chunk
            assert set((so[dl == L] % 16).tolist()) == set(range(16))
    for ch, lowest in ((3, 1), (4, 0), (5, 0)):             # (H = 50 does not exist: chunk 3 drops 6 bytes at least)
        want = {(h, v) for h in range(lowest, 4) for v in range(h, 4)}
        assert set(seen[ch]) == want, ch
        assert all(a == set(range(16)) for a in seen[ch].values())


# ------------------------------------------------------------------- class_edges ---
def test_class_edges_lengths_alignments_and_the_shared_slice():
    c = get("class_edges")
    ol, dl, so, hl = geometry(c)
    assert np.array_equal(ol, c.labels["O"]) and set(ol.tolist()) == set(ALL)
    for O in ALL:
        mine = np.nonzero(ol[64:] == O)[0] + 64
        for L in oref.payload_lengths(O):
            al = sorted((so[mine][dl[mine] == L] % 16).tolist())
            assert al == (list(range(16)) if L <= 300 else cases.LONG_ALIGN), (O, L)
        assert set(dl[mine].tolist()) == set(oref.payload_lengths(O))
        # both sides of the one-line edge and of every class edge
        cl = {cases.cls_of(O, L) for L in dl[mine].tolist()}
        assert cl == ({0, 4, 8, 16, 32, 64} if O <= 8 else {4, 8, 16, 32, 64})
        for E in (64, 256, 512, 1024, 2048):
            if E - HDR - O >= 0:
                assert {E - HDR - O, E - HDR - O + 1} <= set(dl[mine].tolist())
    # slice 0: one data_len under O = 16, 20 and 24 on both sides of a class edge
    for E in cases.EDGES:
        rows = [i for i in range(64) if dl[i] == E - 74 and ol[i] in (16, 20, 24)]
        assert len(rows) == 3 * len(cases.EDGE_ALIGN)
        by_o = {O: {int(hl[i]) for i in rows if ol[i] == O} for O in (16, 20, 24)}
        assert by_o == {16: {E - 4}, 20: {E}, 24: {E + 4}}
        assert cases.cls_of(16, E - 74) == cases.cls_of(20, E - 74) != cases.cls_of(24, E - 74)
    # the blocks are real options: the received-option model reads them back without complaint
    t = c.opts
    for O in ALL:
        b = bytes(t[cases.block_of(O) - 1]["bytes"][:O])
        assert b == cases.REAL_OPTIONS[O]
        f = bytes(46) + bytes([(5 + O // 4) << 4]) + bytes(7) + b
        rec = rxopt_ref.parse(f)
        assert rec["opt_len"] == O and not rec["flags"] & (rxg.O_MALFORMED | rxg.O_CUT | rxg.O_BAD_DOFF | rxg.O_OTHER)
    kinds = 0
    for O in ALL:
        kinds |= rxopt_ref.parse(bytes(46) + bytes([(5 + O // 4) << 4]) + bytes(7) + cases.REAL_OPTIONS[O])["flags"]
    assert kinds == rxg.O_PARSED | rxg.O_MSS | rxg.O_WSCALE | rxg.O_SACK_PERM | rxg.O_SACK | rxg.O_TS


def test_model_frames_of_every_block_length_verify_through_the_rx_oracle():
    c = get("class_edges")
    pool, flen, stats = model("class_edges")
    ol, dl, so, hl = geometry(c)
    n = len(dl)
    assert list(stats) == [n, 0] and np.array_equal(flen, hl)
    recs, _ = oracle.rx_batch(pool, c.off64, flen, cases.peer_tcbs(c.flows), np.ones(len(c.flows), np.uint8))
    assert (recs["c"]["ip_cksum"] == 0).all() and (recs["c"]["tcp_cksum"] == 0).all()
    assert (recs["c"]["verdict"] == rxg.V_DISPATCH).all() and (recs["c"]["tcb_idx"] == c.segs["flow"]).all()
    assert (recs["c"]["datalen"] == dl).all()
    assert np.array_equal(recs["data_off"], ((5 + ol // 4) << 4).astype(np.uint8))
    for i in range(n):  # the option bytes and the payload stand where rxg.h says
        f, O, L, o = frame(c, pool, i), int(ol[i]), int(dl[i]), int(so[i])
        assert bytes(f[HDR:HDR + O]) == cases.REAL_OPTIONS[O]
        assert np.array_equal(f[HDR + O:HDR + O + L], c.payload[o:o + L]) and not f[HDR + O + L:].any()


# ------------------------------------------------------------------------ slices ---
def classes(c, rows):
    ol, dl, _, _ = geometry(c)
    return [cases.cls_of(ol[i], dl[i]) if not c.labels["skipped"][i] else -1 for i in rows]


@pytest.mark.parametrize("cls", cases.CLASSES)
def test_slices_of_one_class(cls):
    c = get("slices", cls)
    ol, dl, _, hl = geometry(c)
    assert len(dl) == 64 + 64 + 17 and c.labels["names"] == ["full", "full", "17"]
    assert set(classes(c, range(len(dl)))) == {cls} and not c.labels["skipped"].any()
    allowed = [O for O in ALL if (cls or O <= 8)]
    lo, hi = cases.HL_RANGE[cls]
    for s in (slice(0, 64), slice(64, 128), slice(128, 145)):
        assert set(ol[s].tolist()) == set(allowed)          # O mixed inside the class
        assert int(hl[s].max()) == hi                       # the class's upper end ...
        assert ((hl[s] == lo) | (dl[s] == 0)).any()         # ... and its lower end, or a frame without data
    if cls == 0:
        assert set(c.segs["reserved"][ol == 0].tolist()) == {0, 1}
    if cls == 4:
        assert ((dl == 0) & (ol >= 12)).any()               # streamed without data
    assert int(dl.max()) <= cases.SMALL_MAX


def test_slices_all_histograms_blocks_and_skips():
    c = get("slices_all")
    ol, dl, _, hl = geometry(c)
    names = c.labels["names"]
    n = len(dl)
    assert n == 64 * 16 + 17 and len(names) == 17 and names[-1] == "17"
    assert len(c.opts) == cases.K_PAST >= 65 and c.nopts == cases.K_LAST
    for s, name in enumerate(names):
        rows = range(64 * s, min(n, 64 * s + 64))
        cl = classes(c, rows)
        kk = c.segs["reserved"][rows.start:rows.stop]
        if name.startswith("class"):
            assert set(cl) == {int(name.split()[1])}
        elif name == "six":
            assert {k: cl.count(k) for k in cases.SIX_COUNTS} == cases.SIX_COUNTS
            assert sum(a != b for a, b in zip(cl, cl[1:])) > 32  # interleaved, not sorted
        elif name == "different blocks":
            assert sorted(kk.tolist()) == list(range(12, 76))
            assert set(ol[rows.start:rows.stop].tolist()) == set(ALL[1:])
        elif name == "same block":
            assert (kk == c.nopts).all() and len(set(cl)) >= 3
        elif name == "skips":
            skipped = [i - rows.start for i in rows if c.labels["skipped"][i]]
            assert skipped == sorted(cases.SKIP_LANES) == [0, 31, 32, 63]
            a = rows.start
            assert int(kk[0]) == c.nopts + 1 and int(c.opts[kk[0] - 1]["len"]) % 4 == 0  # a good block past the bound
            assert int(c.opts[kk[31] - 1]["len"]) == 44 and int(c.opts[kk[32] - 1]["len"]) == 6
            assert int(dl[a + 63]) == MAXD - int(ol[a + 63]) + 1 and int(ol[a + 63]) == 40
            assert int(c.segs["src_off"][a + 63]) + int(dl[a + 63]) <= len(c.payload)  # skipped for its length alone
            assert len(set(cl) - {-1}) == 6
        else:
            assert len(rows) == 17 and len(set(cl)) >= 4
    assert int(c.labels["skipped"].sum()) == 4
    keep = ~c.labels["skipped"]
    assert int(dl[keep].max()) <= cases.SMALL_MAX
    pool, flen, stats = model("slices_all")
    assert list(stats) == [n - 4, 4] and (flen[~keep] == 0).all() and np.array_equal(flen[keep], hl[keep])
    for i in np.nonzero(~keep)[0]:
        assert (frame(c, pool, i, 64) == cases.FILL).all()


# ------------------------------------------------------------------ surroundings ---
@pytest.mark.parametrize("inside,outside", cases.FORMS)
@pytest.mark.parametrize("O", ALL)
def test_surroundings_show_every_byte_from_outside(inside, outside, O):
    c = get("surroundings", inside, outside, O)
    ol, dl, so, hl = geometry(c)
    assert (ol == O).all()
    want = cases.CLASSES if O <= 8 else cases.CLASSES[1:]
    assert [cases.cls_of(O, L) for L in cases.one_per_class(O)] == want
    for L in cases.one_per_class(O):
        assert sorted((so[dl == L] % 16).tolist()) == list(range(16))
    own = np.zeros(len(c.payload), bool)
    for o, L in zip(so.tolist(), dl.tolist()):
        assert not own[o - 64:o + L + 64].any()             # 64 bytes of the other value around every segment
        own[o:o + L] = True
    assert (c.payload[own] == inside).all() and (c.payload[~own] == outside).all()
    raw = c.opts.view(np.uint8).reshape(-1, 48)
    for k, x in enumerate(ALL):
        assert raw[k, 0] == x and (raw[k, 6:6 + x] == inside).all()
        assert (raw[k, 1:6] == outside).all() and (raw[k, 6 + x:] == outside).all()
    pool, _, _ = model("surroundings", inside, outside, O)
    for i in range(len(dl)):
        f = frame(c, pool, i)
        assert (f[HDR:int(hl[i])] == inside).all() and not f[int(hl[i]):].any()


def test_single_option_bytes_show_alone():
    c = get("single_bytes")
    pool, flen, stats = model("single_bytes")
    assert list(stats) == [41, 0] and (flen == HDR + 40 + 21).all() and not c.payload.any()
    raw = c.opts.view(np.uint8).reshape(-1, 48)
    assert (raw[:, 0] == 40).all() and (raw[:, 1:6] == 0xFF).all() and (raw[:, 46:] == 0xFF).all()
    zero = frame(c, pool, 0)
    assert not zero[HDR:].any()
    for j in range(40):
        assert np.count_nonzero(raw[1 + j, 6:46]) == 1 and raw[1 + j, 6 + j] == 0xFF
        f = frame(c, pool, 1 + j)
        diff = set(np.nonzero(f != zero)[0].tolist())
        assert HDR + j in diff and diff <= {50, 51, HDR + j}, j
        assert diff & {50, 51}


# ------------------------------------------------------------------ payload ends ---
@pytest.mark.parametrize("O", ALL)
def test_payload_starts_reach_before_the_buffer(O):
    c = get("payload_starts", O)
    ol, dl, so, _ = geometry(c)
    assert (ol == O).all()
    for L in cases.one_per_class(O):
        assert sorted(so[dl == L].tolist()) == list(range(16))
    base = (so - 6 - O) // 16 * 16                          # the first source chunk of frame chunk 3
    assert int(base.min()) == -((6 + O + 15) // 16 * 16) >= -48 and (base < 0).sum() >= len(cases.one_per_class(O))
    if O == 40:
        assert int(base.min()) == -48


@pytest.mark.parametrize("pbytes", cases.END_BYTES)
def test_payload_ends_are_where_they_claim(pbytes):
    c = get("payload_ends", pbytes)
    ol, dl, so, hl = geometry(c)
    assert pbytes % 16 in (0, 1, 11) and c.payload_bytes == pbytes
    assert (so + dl == pbytes).all()
    assert len(c.payload) % 16 == 0 and len(c.payload) > pbytes and (c.payload[pbytes:] == cases.SLACK).all()
    for O in ALL:
        assert sorted(dl[ol == O].tolist()) == oref.payload_lengths(O)
    # data_len 0 at src_off == payload_bytes, one line and streamed
    for O, cls in ((0, 0), (8, 0), (12, 4), (40, 4)):
        at = np.nonzero((ol == O) & (dl == 0))[0]
        assert len(at) == 1 and int(so[at[0]]) == pbytes and cases.cls_of(O, 0) == cls
    # no 0xEE can come from the data or the option bytes: none stands behind a model frame's headers
    assert not (c.payload[:pbytes] == cases.SLACK).any()
    pool, flen, stats = model("payload_ends", pbytes)
    assert list(stats) == [len(dl), 0]
    for i in range(len(dl)):
        f = frame(c, pool, i)
        assert not (f[HDR:] == cases.SLACK).any()
        assert np.array_equal(f[HDR + int(ol[i]):int(hl[i])], c.payload[pbytes - int(dl[i]):pbytes])


@pytest.mark.parametrize("O", ALL[1:])
def test_longest_segments_on_both_sides_of_the_shifts_zero(O):
    c = get("longest", O)
    ol, dl, so, hl = geometry(c)
    assert (ol == O).all() and (dl == MAXD - O).all() and (hl == 65535).all()
    assert [int(x) for x in (so + 10 - O) % 16] == [0, 5]
    assert int((so + dl).max()) <= len(c.payload)
    assert list(c.model()[2]) == [2, 0]


# --------------------------------------------------------------------- checksums ---
def test_checksums_store_the_promised_values():
    c = get("checksums")
    pool, flen, stats = model("checksums")
    ol, dl, so, hl = geometry(c)
    assert list(stats) == [9, 0] and np.array_equal(flen, hl)
    for i, (cls, O, w) in enumerate(cases.ZERO_TCP):
        f = frame(c, pool, i)
        assert not f[50:52].any() and cases.cls_of(ol[i], dl[i]) == cls and int(ol[i]) == O
        assert w % 2 == 0 and HDR <= w and w + 2 <= HDR + O and w // 16 == {8: 3, 24: 4, 40: 5}[O]
        assert f[w:w + 2].any()                             # the word did the work
        assert cases.tcp_sum32(f, int(hl[i])) % 0xFFFF == 0
    assert [x[0] for x in cases.ZERO_TCP] == cases.CLASSES
    f = frame(c, pool, cases.I_IP)
    assert not f[24:26].any() and int(ol[cases.I_IP]) == 20
    f = frame(c, pool, cases.I_MAX)
    assert int(hl[cases.I_MAX]) == 65535 and int(ol[cases.I_MAX]) == 40
    ones = np.r_[0:12, 18:20, 26:46, 47:50, HDR:65535]      # every field a caller sets, options, payload
    assert (f[ones] == 0xFF).all()
    sums = [cases.tcp_sum32(frame(c, pool, i), int(hl[i])) for i in range(9)]
    assert sums[cases.I_MAX] == max(sums) > (65535 - 34 - 4) // 2 * 0xFFFF
    s = sums[cases.I_CARRY]
    assert (s & 0xFFFF) + (s >> 16) > 0xFFFF                # one fold leaves a carry
    assert not any((x & 0xFFFF) + (x >> 16) > 0xFFFF for x in sums[:cases.I_IP])
    # the oracle's fields are the complement of these sums
    for i in range(9):
        f = frame(c, pool, i)
        assert (sums[i] + int(f[50]) + (int(f[51]) << 8)) % 0xFFFF == 0


# ------------------------------------------------------------------- pool limits ---
ALL_CASES = ([("masks", O) for O in ALL] + [("class_edges",), ("slices_all",), ("single_bytes",), ("checksums",)] +
             [("slices", k) for k in cases.CLASSES] + [("surroundings", i, o, O) for i, o in cases.FORMS for O in ALL] +
             [("payload_starts", O) for O in ALL] + [("payload_ends", p) for p in cases.END_BYTES] +
             [("longest", O) for O in ALL[1:]])


def test_no_pool_exceeds_the_fixture_limit():
    for key in ALL_CASES:
        c = get(*key)
        assert c.nslots * 64 <= cases.LIMIT, (key, c.nslots * 64)
        assert len(c.off64) == len(c.segs) and int(c.off64.max()) < c.nslots
        assert len(set(c.off64.tolist())) == len(c.off64)   # a slot of its own for every descriptor
