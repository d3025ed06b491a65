"""GPU: the replay's selected re-classification (rxg_rx_replay's reclassify(): rx_kernel<16, kDescSel,
false, false> through a selection list) on the deterministic edge sets of tests/replay_sel_cases.py
(sizes, holes, classes, waves, rewrites, trunc, forms, checks; tests/test_replay_sel_cases_host.py
holds what each set covers).

Per set and context kind: the table is loaded, the burst run in the set's form, and every burst
replayed with handlers that record what they saw; a writer frame's tcpswitch makes its one write.
Asserted: per packet what the handlers saw (("switch", idx, state), ("rst",), free; tcpnopcb
separates the two reset verdicts; with the checksum verify, the frees and tcpchecksumerror; with the
ARP mirror, the add_mac order); engine.counters() equal to the epochs' summed oracle counters (which
carries the REF_NULLSLOT and hit-counter corrections computed from the fix records); the difference
of replay_stats() before and after equal to the model's four figures, an equality against the model
and never against the library's own output; and the device table after the replay, by a burst of
the set's first frames against the final rows.

Contexts are made here: default, RXG_CFG_REPLAY_ON_DEVICE, and RXG_CFG_REPLAY_ON_DEVICE with
max_blocks 1 and 2 (waves; classes/ahead, whose look-aheads only a capped grid meets).  Every device
pool ends in 16 KiB of fill, and every record buffer is exactly the burst's.

What this cannot see: datalen and IP_OK of a fix record reach no handler and no counter, so a
re-classification that got only those wrong passes."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle
import pktgen
import replay_sel_cases as rc
import rxg

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def contexts():
    """(on_device, max_blocks) -> a context of its own, made on first use, closed at the module's end."""
    engines = {}

    def get(on_device, max_blocks):
        key = (on_device, max_blocks)
        if key not in engines:
            engines[key] = rxg.Engine(device=0, max_batch=1 << 15, max_bytes=16 << 20, max_blocks=max_blocks,
                                       flags=rxg.CFG_REPLAY_ON_DEVICE if on_device else 0)
        return engines[key]

    try:
        yield get
    finally:
        for e in engines.values():
            e.close()
        engines.clear()


def _slots(f):
    return (len(f) + 63) // 64


def _list_pool(frames, order):
    """Frames in `order` in one pool, POOL_TAIL bytes of fill behind the last."""
    idx = {"fwd": list(range(len(frames))), "rev": list(range(len(frames) - 1, -1, -1))}.get(order)
    if idx is None:
        idx = list(range(len(frames)))
        random.Random(5).shuffle(idx)
    off, pos = np.zeros(len(frames), dtype=np.uint32), 0
    for i in idx:
        off[i] = pos
        pos += _slots(frames[i])
    pool = np.full(pos * 64 + rc.POOL_TAIL, rc.FILL, dtype=np.uint8)
    for i, f in enumerate(frames):
        pool[int(off[i]) * 64:int(off[i]) * 64 + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return pool, off


def _run_bursts(eng, c, keep):
    """The case's bursts in its form; returns per burst its records as the kernel wrote them."""
    fr, kind = c.frames, c.kind
    dt = rxg.rec_dtype(kind)
    if c.form == "host":
        assert len(c.bursts) == 1
        return [eng.rx_burst(fr, kind)]
    lens = np.array(c.lens, dtype=np.uint16)
    dl = eng.to_device(lens)
    outs = [eng.alloc((hi - lo) * kind) for lo, hi in c.bursts]
    keep += [dl] + outs
    if c.form in ("dev", "multi"):
        pool, off = _list_pool(fr, c.order)
        da, do = eng.to_device(pool), eng.to_device(off)
        keep += [da, do]
        if c.form == "dev":
            eng.rx_burst_dev(da.ptr, do.ptr, dl.ptr, c.n, outs[0].ptr, kind)
        else:
            eng.rx_bursts_dev(da.ptr, [(do.ptr + 4 * lo, dl.ptr + 2 * lo, hi - lo, o.ptr)
                                       for (lo, hi), o in zip(c.bursts, outs)], kind)
    else:      # strided, smulti: frame i of the pool at slot slot0 + i * stride64, slot0 > 0
        stride, slot0 = max(_slots(f) for f in fr), 3
        pool = np.full((slot0 + c.n * stride) * 64 + rc.POOL_TAIL, rc.FILL, dtype=np.uint8)
        for i, f in enumerate(fr):
            o = (slot0 + i * stride) * 64
            pool[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
        da = eng.to_device(pool)
        keep.append(da)
        eng.rx_bursts_strided_dev(da.ptr, stride, [(slot0 + lo * stride, dl.ptr + 2 * lo, hi - lo, o.ptr)
                                                   for (lo, hi), o in zip(c.bursts, outs)], kind)
    eng.sync()
    return [o.download(dt, hi - lo) for (lo, hi), o in zip(c.bursts, outs)]


def run_case(eng, c, on_device):
    sim = c.sim(on_device)
    exp, ecnt, erows = c.expect
    fr = c.frames
    eng.tcb_load(*pktgen.table_arrays(rc.ROWS))
    eng.tcb_sync()
    if c.checks:
        eng.arp_load(c.known_sources)
    else:
        eng.arp_disable()
    table = rc.Table(rc.ROWS)
    bufs = [C.create_string_buffer(f, max(len(f), 64)) for f in fr]
    addr = {C.addressof(b): i for i, b in enumerate(bufs)}
    got, learned, wrote = [None] * c.n, [], []

    def free_mbuf(u, m):
        if got[addr[m]] is None:
            got[addr[m]] = ("free",)

    def rst(u, ip, tcp):
        got[addr[ip - 14]] = ("rst",)

    def tcpswitch(u, idx, st, tcp, ip, m):
        i = addr[m]
        got[i] = ("switch", idx, st)
        if i in c.writers:
            rc.apply_writer(table, c.writers[i], eng)
            wrote.append(i)
        return 0

    def add_mac(u, ip, mac):
        learned.append(ip)
        return 1

    nopcb, cksum = C.c_int(0), C.c_int(0)
    ops = rxg.HandoffOps(None, rxg.HANDOFF_FREE(free_mbuf), rxg.HANDOFF_ARP_IN(), rxg.HANDOFF_GET_MAC(),
                         rxg.HANDOFF_ADD_MAC(add_mac) if c.checks else rxg.HANDOFF_ADD_MAC(),
                         rxg.HANDOFF_SEND_RESET(rst), rxg.HANDOFF_ON_SEGMENT(), rxg.HANDOFF_TCPSWITCH(tcpswitch))
    ops.tcpnopcb = C.pointer(nopcb)
    ops.tcpchecksumerror = C.pointer(cksum)
    if c.checks:
        ops.flags = rxg.OPS_VERIFY_TCP_CKSUM
    lib = rxg.load_library()
    keep = []
    try:
        eng.counters_reset()
        before = eng.replay_stats()
        recs = _run_bursts(eng, c, keep)
        for (lo, hi), r in zip(c.bursts, recs):
            ptrs = (C.c_void_p * (hi - lo))(*[C.addressof(b) for b in bufs[lo:hi]])
            rc_ = lib.rxg_rx_replay(eng.ctx, C.byref(ops), ptrs, ptrs, r.ctypes.data, hi - lo, c.kind)
            assert rc_ == 0, lib.rxg_last_error()
        after = eng.replay_stats()
        counters = eng.counters()
        # the device table after the replay: the set's first frames against the final rows
        if c.checks:
            eng.arp_disable()
        probe = [f for f in fr[:320] if len(f) >= 54]
        want, _ = oracle.rx_batch(*pktgen.pack_arena(probe), *pktgen.table_arrays(erows))
        table_now = eng.rx_burst(probe, rxg.REC48)
    finally:
        for d in keep:
            d.free()
    delta = {k: after[k] - before[k] for k in after}
    print(c.name, "device" if on_device else "default", "stats", delta, "model", sim.stats)
    assert delta == sim.stats
    assert wrote == sorted(c.writers)
    e_nopcb = e_cksum = 0
    for i, r in enumerate(exp):
        v = int(r["verdict"])
        if c.checks_drop(i):
            e_cksum += 1
            want_i = ("free",)
        elif v == rxg.V_DISPATCH:
            want_i = ("switch", int(r["tcb_idx"]), int(r["state"]))
        elif v in (rxg.V_RST_NOPCB, rxg.V_RST_LISTEN_NONSYN):
            e_nopcb += v == rxg.V_RST_NOPCB
            want_i = ("rst",)
        else:
            want_i = ("free",)
        assert got[i] == want_i, (c.name, i, c.specs[i], got[i], want_i)
    assert (nopcb.value, cksum.value) == (e_nopcb, e_cksum)
    assert table.rows == erows
    assert counters.tolist() == ecnt.tolist()
    assert table_now.tobytes() == want.tobytes()
    if c.checks:      # ip.c:30-32: the first TCP sighting of every source the mirror did not hold
        seen, order = set(c.known_sources), []
        for i, r in enumerate(exp):
            src = int.from_bytes(fr[i][26:30], "big")
            if int(r["verdict"]) in rc.TCP_VERDICTS and src not in seen:
                seen.add(src)
                order.append(src)
        assert learned == order and order


CASES = [(n, od, mb) for n in rc.ALL for od, mb in rc.contexts(rc.get(n))]


@pytest.mark.parametrize("name,on_device,max_blocks", CASES,
                         ids=[f"{n}-{'device' if od else 'default'}{mb or ''}" for n, od, mb in CASES])
def test_replay_selection_edges(contexts, name, on_device, max_blocks):
    run_case(contexts(on_device, max_blocks), rc.get(name), on_device)
