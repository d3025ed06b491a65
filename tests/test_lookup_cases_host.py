"""CPU: the sets of tests/lookup_cases.py hold what they claim.  tests/lookup_check.cpp (the host
mirror of csrc/rxg_mirror.h, built stand-alone with the host sanitizers) says where every key
sits and what every lookup reads; the claims are held against that in forms that are true for any
insertion order of TcbMirror::rebuild, and every frame set is run through the oracle."""
import collections
import functools
import os
import subprocess

import numpy as np
import pytest

import lookup_cases as lc
import oracle
import pktgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpdk-tcpipstack_amd", "csrc")
EXE = os.path.join(ROOT, "dpdk-tcpipstack_amd", "build", "lookup_check")

F_IP_OK, F_TCP_OK, F_LISTEN, F_NULLSLOT, F_TRUNC = 1, 2, 4, 8, 16   # include/rxg.h
T = collections.namedtuple("T", "nb hash home found probed crossed idx state listen")
A = collections.namedtuple("A", "nb hash home found probed crossed hit")


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "lookup_check.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("rxg_mirror.h", "rxg_common.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *san,
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, src, "-o", EXE], check=True)
    return EXE


def run_check(exe, tmp_path, text):
    """{(kind, phase): [answers]}, moves."""
    p = tmp_path / "lookup.in"
    p.write_text(text)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    r = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120, env=env)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1].startswith("ok") and not r.stderr.strip(), r.stdout[-400:] + r.stderr
    out = collections.defaultdict(list)
    for ln in lines[:-1]:
        w = ln.split()
        out[w[0], int(w[1])].append((T if w[0] == "T" else A)(*map(int, w[3:])))
    return out, int(lines[-1].split()[2])


ALL_TABLES = lc.launched_tables() + [lc.cache_table()]


@pytest.fixture(scope="module")
def answers(exe, tmp_path_factory):
    """table name -> (answers before the table's writes, after them, moves)."""
    d = tmp_path_factory.mktemp("lookup")
    out = {}
    for t in ALL_TABLES:
        a, moves = run_check(exe, d, lc.check_file_text(t))
        out[t.name] = (a["T", 0], a["T", 1] if t.ops else a["T", 0], moves)
    return out


def test_hashes_equal_the_programs(exe, tmp_path):
    f = lc.Finder(0, start=77)
    qs = [lc._q(f"k{h}", f.take(0, 1, dport=(80 + 37 * h) & 0xFFFF)[0], None, None) for h in range(2500)]
    qs += [lc.ZERO_Q, lc.Q("ones", lc.M32, 65535, 65535, lc.M32, None, None)]
    ips = [0, 1, lc.M32] + [pktgen.ip4(10, 200, i >> 8, i & 255) for i in range(3000)]
    t = lc.Table("hashes", [], qs, 1)
    a, _ = run_check(exe, tmp_path, lc.check_file_text(t, arp=dict(known=[], later=[]), arp_queries=ips))
    assert len(qs) > 2000 and [x.hash for x in a["T", 0]] == [lc.tuple_hash(*lc.key_of(q)) for q in qs]
    assert [x.hash for x in a["A", 0]] == [lc.arp_hash(ip) for ip in ips]


@pytest.mark.parametrize("t", ALL_TABLES, ids=lambda t: t.name)
def test_table_sizes_and_labels(answers, t):
    before, after, _ = answers[t.name]
    assert {x.nb for x in before + after} == {t.nb} and lc.tcb_nb(len(t.loaded_keys())) == t.nb
    for q, x in zip(t.queries, after):
        assert x.home == lc.home_of(q, t.nb - 1)
        if q.kind is not None:
            assert (x.found >= 0) == (q.kind == "found"), q
        if q.walk is not None:
            assert (x.probed >= 2) == q.walk, (q, x)
        if x.found < 0 and x.probed >= 2:  # a walking miss ends at a bucket with a free slot
            assert x.probed == lc.miss_probes(t.occ, x.home) and t.occ[(x.home + x.probed - 1) % t.nb] < 4


def _dist(x, nb):
    return (x.found - x.home) % nb


def test_coverage_claims(answers):
    found = [(x, t.nb) for t in ALL_TABLES for x in answers[t.name][1] if x.found >= 0]
    missing = [x for t in ALL_TABLES for x in answers[t.name][1] if x.found < 0]
    assert {0, 1, 2, 3} <= {_dist(x, nb) for x, nb in found}
    assert any(x.crossed for x, _ in found) and any(x.crossed for x in missing)
    # said per table, in forms no insertion order changes: a bucket holds four keys, so fourteen
    # keys with one home sit at distances 0, 1, 2, 3, and ten of them beyond the home bucket
    c16 = lc.cluster16()
    a16 = dict(zip([q.label for q in c16.queries], answers["cluster16"][1]))
    h14 = [a16[f"h14_{i}"] for i in range(14)]
    assert sorted(_dist(x, 16) for x in h14) == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 2
    assert sum(x.crossed for x in h14) == 6
    assert [(a16[k].found, a16[k].probed) for k in ("h15a", "h15b", "h0a", "h0b", "h1", "h2")] == \
        [(1, 3), (1, 3), (2, 3), (2, 3), (2, 2), (2, 1)]
    assert [a16[f"miss{h}_{k}"].probed for h, k in ((14, "listen"), (15, "nopcb"), (0, "listen"), (1, "nopcb"),
                                                     (2, "listen"), (6, "listen"))] == [6, 5, 4, 3, 2, 1]
    tw = dict(zip([q.label for q in lc.tiny_wrap().queries], answers["tiny_wrap"][1]))
    for k in ("miss1_listen", "miss1_nopcb"):
        assert (tw[k].home, tw[k].probed, tw[k].crossed, tw[k].found) == (1, 2, 1, -1)
    assert tw["miss1_listen"].listen == 1 and tw["miss1_nopcb"].idx == -1 and tw["miss0_listen"].probed == 1
    for live in (True, False):
        t = lc.zero_tuple(live, True)
        z = answers[t.name][1][-1]
        assert t.queries[-1].label == "zero" and z.probed == 4 and (z.found >= 0) == live and z.hash == lc.tuple_hash(0, 0, 0)
        assert not live or _dist(z, 8) == 3
        t = lc.zero_tuple(live, False)
        z = answers[t.name][1][-1]
        assert z.probed == 1 and (z.found >= 0) == live and 0 < t.occ[z.home] < 4
    d = dict(zip([q.label for q in lc.duplicates().queries], zip(*answers["duplicates"][:2])))
    assert d["dup"][0].idx == 1 and d["dup"][1].idx == 3 and d["dup"][1].state == 5


def test_removals_move_keys_across_the_end(answers):
    t = lc.cluster16_removed()
    before, after, moves = answers[t.name]
    base = answers["cluster16"][1]   # the table before the removals (cluster16's own upserts made)
    assert moves > 0
    moved = [(q.label, b.found, a.found) for q, b, a in zip(t.queries, base, after) if b.found >= 0 and a.found >= 0
             and b.found != a.found]
    assert moved and any(b <= 2 and a >= 14 for _, b, a in moved), moved
    gone = [a for q, a in zip(t.queries, after) if q.label in ("h14_5", "h14_7", "h14_8", "h14_11")]
    assert all(a.found < 0 and a.listen == 1 for a in gone)


def _walk_bits(t, ans, burst):
    by_key = {lc.key_of(q): x.probed >= 2 for q, x in zip(t.queries, ans)}
    return [{lane for lane, e in enumerate(sl) if by_key[lc.key_of(e[0])]} for sl in burst]


@pytest.mark.parametrize("t", [t for t in lc.launched_tables() if "lane_walkers" in lc.layouts(t)], ids=lambda t: t.name)
def test_lane_walkers_walk_on_the_stated_lanes_only(answers, t):
    burst, lanes = lc.lane_walkers(t)
    assert _walk_bits(t, answers[t.name][1], burst) == lanes
    assert [sorted(s) for s in lanes[:7]] == [[x] for x in lc.WALKER_LANES]
    assert lanes[7:] == [set(range(64)), set(range(0, 64, 2)), set(range(1, 64, 2)), set(range(32)), set(range(32, 64))]
    ans = dict(zip([lc.key_of(q) for q in t.queries], answers[t.name][1]))
    for sl, ls in zip(burst[7:], lanes[7:]):  # walkers of one slice differ in length and result
        w = [ans[lc.key_of(sl[lane][0])] for lane in ls]
        if t.name == "cluster16":
            assert {1, 2, 3} <= {x.probed - 1 for x in w}
            assert {(True, 0, True), (False, 1, True), (False, 0, False)} <= {(x.found >= 0, x.listen, x.idx >= 0) for x in w}
    if t.name == "cluster16":
        w = [ans[lc.key_of(q)] for q in t.walkers]
        assert {1, 2, 3} <= {x.probed - 1 for x in w}
        assert {(x.found >= 0, x.listen, x.idx >= 0) for x in w} == {(True, 0, True), (False, 1, True), (False, 0, False)}
    for t2burst in lc.partial(t):
        last = t2burst[-1]
        assert len(last) in lc.PARTIAL_SIZES and ans[lc.key_of(last[-1][0])].probed >= 2


def test_lane_rotation_puts_every_tuple_on_every_lane(answers):
    t = lc.rotation64()
    burst = lc.lane_rotation(t)
    assert len(burst) == 64 and len({lc.key_of(q) for q in t.queries}) == 64
    for lane in range(64):
        assert len({lc.key_of(sl[lane][0]) for sl in burst}) == 64
    x = answers[t.name][1]
    assert len({a.idx for a in x}) == 64 and all(a.found >= 0 for a in x)
    assert {0, 1, 2, 3} <= {_dist(a, 32) for a in x} and sum(a.crossed for a in x) == 6


def test_one_bit_variants_differ_in_one_bit_of_one_word():
    steps = lc.cache_steps()
    names = [n for n, _ in steps]
    t = lc.cache_table()
    keys = lc.distinct_keys(t.final_rows)
    seen = set()
    for i, (name, sl) in enumerate(steps):
        if not name.startswith("onebit_"):
            continue
        _, word, what = name.split("_")
        assert names[i - 1] == f"base_before_{word}_{what}"
        for (q, _), (p, _) in zip(sl, steps[i - 1][1]):
            diff = [a ^ b for a, b in zip(lc.key_of(q), lc.key_of(p))]
            w = {"sport": 0, "dport": 0, "dst": 1, "src": 2}[word]
            assert bin(diff[w]).count("1") == 1 and all(d == 0 for k, d in enumerate(diff) if k != w), (name, q)
            assert (diff[w] >> 16 != 0) == (word == "dport") or w != 0
            if p.kind == "found":  # the other tuple is in the table under another index, or absent
                assert (lc.key_of(q) in keys) == (what == "present"), (name, q)
        seen.add((word, what))
    assert len(seen) == 8
    for lane in (0, 37, 63):
        sl, base = dict(steps)[f"all_but_{lane}"], dict(steps)["base"]
        assert [k for k in range(64) if sl[k] != base[k]] == [lane]


class Sets:
    """Every frame set of the module, with the oracle's records: (name, table, frames, exp, cnt)."""

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def all():
        out = []
        for t in lc.launched_tables():
            for lname, bursts in lc.layouts(t).items():
                for form in lc.FORMS:
                    for b, burst in enumerate(bursts):
                        out.append((f"{t.name}/{lname}{b}/{form}", t, lc.burst_frames(burst, form)))
            if t.name.startswith("zero"):
                for form in lc.FORMS:
                    st = lc.cache_stream(4, lc.zero_steps(t))
                    out.append((f"{t.name}/zero_stream/{form}", t, lc.burst_frames(st, form, lc.stream_small_fn(4))))
        for nw in (4, 12):
            for form in lc.FORMS:
                out.append((f"cache_stream{nw}/{form}", lc.cache_table(),
                            lc.burst_frames(lc.cache_stream(nw), form, lc.stream_small_fn(nw))))
        res = []
        for name, t, frames in out:
            arena, off, lens = pktgen.pack_arena(frames)
            tcb, live = pktgen.table_arrays(t.final_rows)
            exp, cnt = oracle.rx_batch(arena, off, lens, tcb, live)
            res.append((name, t, frames, exp, cnt))
        return res


def test_sizes_of_the_forms():
    n = 0
    for name, _, frames, _, _ in Sets.all():
        ls = {len(f) for f in frames}
        form = name.rsplit("/", 1)[1]
        if form == "small":
            assert max(ls) <= 64, name
        elif form == "class":   # (the streams' truncated frames are 40 bytes in every form)
            assert 65 <= min(ls - {40}) and max(ls) <= 128 and (40 not in ls or "cache_stream" in name), name
        else:
            assert min(ls) <= 64 and max(ls) > 64, name
        n += len(frames)
    print(f"{len(Sets.all())} sets, {n} frames")
    assert 20000 <= n <= 400000


def test_oracle_agrees_with_the_mirror_on_every_frame(answers):
    verdicts, flags = set(), 0
    for name, t, frames, exp, _ in Sets.all():
        ans = {lc.key_of(q): x for q, x in zip(t.queries, answers[t.name][1])}
        c = exp["c"]
        verdicts |= set(c["verdict"].tolist())
        flags |= int(np.bitwise_or.reduce(c["flags"]))
        for i, f in enumerate(frames):
            if c["verdict"][i] > 2 or len(f) < 54:   # no TCP segment / (truncated: checked by the GPU tests)
                continue
            key = (int.from_bytes(f[36:38], "big") << 16 | int.from_bytes(f[34:36], "big"),
                   int.from_bytes(f[30:34], "little"), int.from_bytes(f[26:30], "big"))
            x = ans.get(key)
            if x is None:
                continue   # (a one-bit variant: not among the table's queries)
            assert (int(c["tcb_idx"][i]), int(c["state"][i]), int(bool(c["flags"][i] & F_LISTEN))) == \
                (x.idx, x.state, x.listen), (name, i, c[i], x)
    assert verdicts == {0, 1, 2, 3, 4, 5}
    assert flags & 0x1F == F_IP_OK | F_TCP_OK | F_LISTEN | F_NULLSLOT | F_TRUNC


def test_kinds_are_what_the_oracle_answers():
    for name, t, frames, exp, _ in Sets.all():
        if "every_query" not in name or not name.endswith("small"):
            continue
        by_key = {lc.key_of(q): q for q in t.queries}
        c = exp["c"]
        for i, f in enumerate(frames):
            q = by_key[(int.from_bytes(f[36:38], "big") << 16 | int.from_bytes(f[34:36], "big"),
                        int.from_bytes(f[30:34], "little"), int.from_bytes(f[26:30], "big"))]
            fl = int(c["flags"][i])
            got = "nopcb" if c["tcb_idx"][i] < 0 else "found" if not fl & F_LISTEN else \
                "listen_null" if fl & F_NULLSLOT else "listen"
            assert q.kind is None or got == q.kind, (name, q, c[i])


@pytest.mark.parametrize("nb,zero", [(4, False), (4, True), (16, False), (16, True)])
def test_arp_cluster(exe, tmp_path, nb, zero):
    a = lc.arp_cluster(nb, zero)
    burst, lanes = lc.arp_burst(a)
    ips = sorted({e[0].src for sl in burst for e in sl})
    ans, _ = run_check(exe, tmp_path, lc.check_file_text(arp=a, arp_queries=ips))
    x0 = dict(zip(ips, ans["A", 0]))
    assert {x.nb for x in x0.values()} == {nb}
    assert [{lane for lane, e in enumerate(sl) if x0[e[0].src].probed >= 2} for sl in burst] == lanes
    w = [x0[ip] for ip in a["walk_found"] + a["walk_miss"]]
    assert all(x.crossed and x.home == nb - 1 for x in w) and {x.hit for x in w} == {0, 1}
    assert all(x0[ip].hit == (ip in a["known"]) for ip in ips) and x0[0].hit == int(zero) and x0[0].probed == 0
    if a["later"]:
        x1 = dict(zip(ips, ans["A", 1]))
        assert all(x1[ip].hit and x1[ip].probed >= 2 and not x0[ip].hit for ip in a["later"])
        assert all(x1[ip].hit == (ip in a["known"] + a["later"]) for ip in ips)
