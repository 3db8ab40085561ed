"""Flow expiry (nsd_flow_expire_device, nsd_flow_expire, nsd_flow_expire_cpu,
nsd_pcap_flows_expire): the rules of include/netsniff_dissect.h "flow expiry"
against a model that shares no code with the product - expire_model splits the
{key: [flags, pkts, bytes, first, last]} dict that test_flows.model makes, with
the rules written out - and hand-written answers.  Every comparison is exact.

CPU tests run nsd_flow_expire_cpu over flow rows.  GPU tests run the kernels
(init / split / clear / reinsert) into poisoned outputs and a poisoned
workspace, and then look at the rebuilt table through the entries that existed
before: export, a further update, conversations.
"""
import numpy as np
import pytest

import edge_cases as E
import nsd
import nsd_testlib as T
import test_conversations as C
import test_flows as F
from nsd_testlib import device_fill  # noqa: F401  (fixture: nsd_set_debug_fill(0xA5) around each test)

PAIRED = 1
U64_MAX = (1 << 64) - 1
ST_EXPIRED = 6
IPV4, TCP, UDP = F.IPV4, F.TCP, F.UDP
V4 = F.V4


# ---- the model ----------------------------------------------------------------
def reverse(k):
    src, dst, sport, dport, l3, l4 = k
    return (dst, src, dport, sport, l3, l4)


def qualifies(flows, k, before, flags):
    """The header's rule for one flow of the dict."""
    if not flows[k][4] < before:
        return False
    rk = reverse(k)
    if flags & PAIRED and rk != k and rk in flows:
        return flows[rk][4] < before
    return True


def expire_model(flows, before, flags=0):
    """(expired dict, remaining dict) with room for every qualifying flow."""
    gone = {k: v for k, v in flows.items() if qualifies(flows, k, before, flags)}
    return gone, {k: v for k, v in flows.items() if k not in gone}


def merge(into, more):
    """What a further update does to a table: `more` accumulated into `into`."""
    out = {k: list(v) for k, v in into.items()}
    for k, v in more.items():
        if k in out:
            o = out[k]
            out[k] = [o[0] | v[0], o[1] + v[1], o[2] + v[2], min(o[3], v[3]), max(o[4], v[4])]
        else:
            out[k] = list(v)
    return out


def by_first(m):
    return F.sorted_model(m)


def rows_list(flows):
    return [[k, v] for k, v in F.rows_of(flows)]


def make_rows(items):
    """[(key, [flags, pkts, bytes, first, last])] -> FLOW_DTYPE rows in that order."""
    rows = np.zeros(len(items), dtype=nsd.FLOW_DTYPE)
    for r, (k, v) in zip(rows, items):
        r["src"], r["dst"] = np.frombuffer(k[0], np.uint8), np.frombuffer(k[1], np.uint8)
        r["sport"], r["dport"], r["l3"], r["l4"] = k[2:]
        r["tcp_flags"], r["pkts"], r["bytes"], r["first"], r["last"] = v
    return rows


# ---- CPU: known answers ---------------------------------------------------------
def known_rows():
    A, B, Cc, D, Ee, Ff, G, H, S = (V4(0x0A000001 + j) for j in range(9))
    return [
        ((A, B, 1111, 2222, IPV4, UDP), [0, 3, 300, 0, 10]),         # 0 A -> B: idle
        ((B, A, 2222, 1111, IPV4, UDP), [0, 2, 200, 1, 50]),         # 1 B -> A: live
        ((Cc, D, 10, 20, IPV4, TCP), [0x12, 4, 400, 2, 5]),          # 2 C -> D: idle
        ((D, Cc, 20, 10, IPV4, TCP), [0x10, 1, 100, 3, 8]),          # 3 D -> C: idle
        ((Ee, Ff, 5, 6, IPV4, UDP), [0, 1, 60, 4, 4]),               # 4 idle, no reverse
        ((S, S, 9999, 9999, IPV4, UDP), [0, 2, 92, 6, 7]),           # 5 idle, its own reverse
        ((G, H, 500, 600, IPV4, TCP), [0x02, 1, 54, 9, 9]),          # 6 TCP G -> H: idle
        ((H, G, 600, 500, IPV4, UDP), [0, 1, 54, 11, 90]),           # 7 UDP H -> G: live, not its pair
        ((Ff, Ee, 7, 5, IPV4, UDP), [0, 1, 60, 12, 30]),             # 8 live; ports differ from 4's reverse
    ]


def test_known_answers():
    R = known_rows()
    rows = make_rows(R)
    as_list = lambda idx: [[R[j][0], R[j][1]] for j in idx]   # noqa: E731
    # before = 30: last < 30 is idle
    rest, gone, q = nsd.flow_expire_cpu(rows, 30)
    assert q == 6 and rows_list(gone) == as_list([0, 2, 3, 4, 5, 6]) and rows_list(rest) == as_list([1, 7, 8])
    # PAIRED: A -> B stays with its live reverse; C <-> D leave together; the
    # others have no reverse in the table (7 is UDP, 6 TCP) or are their own
    rest, gone, q = nsd.flow_expire_cpu(rows, 30, PAIRED)
    assert q == 5 and rows_list(gone) == as_list([2, 3, 4, 5, 6]) and rows_list(rest) == as_list([0, 1, 7, 8])
    # `last` itself is not below `before`
    rest, gone, q = nsd.flow_expire_cpu(rows, 8)
    assert q == 3 and rows_list(gone) == as_list([2, 4, 5])
    rest, gone, q = nsd.flow_expire_cpu(rows, 8, PAIRED)             # D -> C (last 8) keeps C -> D
    assert q == 2 and rows_list(gone) == as_list([4, 5]) and len(rest) == 7
    # the edges of `before`
    rest, gone, q = nsd.flow_expire_cpu(rows, 0, PAIRED)
    assert q == 0 and len(gone) == 0 and rows_list(rest) == as_list(range(9))
    for flags in (0, PAIRED):
        rest, gone, q = nsd.flow_expire_cpu(rows, U64_MAX, flags)
        assert q == 9 and len(rest) == 0 and rows_list(gone) == as_list(range(9))
    # the cap: the first `max` qualifying rows in input order, the others stay
    rest, gone, q = nsd.flow_expire_cpu(rows, 30, 0, max_flows=2)
    assert q == 6 and rows_list(gone) == as_list([0, 2]) and rows_list(rest) == as_list([1, 3, 4, 5, 6, 7, 8])
    rest, gone, q = nsd.flow_expire_cpu(rows, 30, 0, max_flows=0)
    assert q == 6 and len(gone) == 0 and rows_list(rest) == as_list(range(9))
    # the model reads the same rows the same way
    m = dict((k, v) for k, v in R)
    for before, flags, want in ((30, 0, [0, 2, 3, 4, 5, 6]), (30, PAIRED, [2, 3, 4, 5, 6]), (8, PAIRED, [4, 5])):
        assert by_first(expire_model(m, before, flags)[0]) == as_list(want)


def cpu_rows(name):
    if name == "few37":
        frames, desc, rec, ext = F.few37()[:4]
    elif name == "many":
        frames, desc, rec, ext = F.cached("many:300x5", lambda: F.many_flows(1500, 300))[:4]
    else:
        frames, desc, rec, ext = C.talk_batch(4096, 50)
    flows, _ = nsd.flow_cpu(frames, desc, rec, ext, base=100)
    return flows, F.model(frames, desc, rec, ext, base=100)[0]


@pytest.mark.parametrize("flags", [0, PAIRED])
@pytest.mark.parametrize("name", ["few37", "many", "talk"])
def test_expire_cpu_matches_model(name, flags):
    flows, m = cpu_rows(name)
    assert dict(F.rows_of(flows)) == m
    shuffled = flows[np.random.RandomState(5).permutation(len(flows))]
    lasts = sorted(v[4] for v in m.values())
    for before in (0, lasts[len(lasts) // 2], U64_MAX):
        gone, stay = expire_model(m, before, flags)
        if before == lasts[len(lasts) // 2]:
            assert 0 < len(gone) < len(m)
            if name == "talk" and flags:
                assert len(gone) < len(expire_model(m, before, 0)[0])    # pairs held back
        for rows in (flows, shuffled):
            rest, exp, q = nsd.flow_expire_cpu(rows, before, flags)
            order = [k for k, _ in F.rows_of(rows)]
            assert q == len(gone)
            assert rows_list(exp) == [[k, m[k]] for k in order if k in gone]
            assert rows_list(rest) == [[k, m[k]] for k in order if k in stay]
            if len(gone) > 1:
                cap = len(gone) - 1
                rest, exp, q = nsd.flow_expire_cpu(rows, before, flags, max_flows=cap)
                taken = [k for k in order if k in gone][:cap]
                assert q == len(gone) and rows_list(exp) == [[k, m[k]] for k in taken]
                assert rows_list(rest) == [[k, m[k]] for k in order if k not in taken]
                assert dict(F.rows_of(exp)) | dict(F.rows_of(rest)) == m


def test_arguments():
    assert (nsd.FLOW_EXPIRE_PAIRED, nsd.FLOW_ST_EXPIRED) == (1, 6)
    L = nsd.lib()
    rows = make_rows(known_rows())
    out = np.zeros(9, dtype=nsd.FLOW_DTYPE)
    rem = np.zeros(1, dtype=np.uint64)
    cpu = lambda *a: L.nsd_flow_expire_cpu(*a)   # noqa: E731
    assert cpu(rows.ctypes.data, 9, 30, 2, out.ctypes.data, 9, rem.ctypes.data) == -1      # NSD_ERR_ARG: a flag bit
    assert cpu(rows.ctypes.data, 9, 30, 0xFFFFFFFE, out.ctypes.data, 9, rem.ctypes.data) == -1
    assert cpu(None, 9, 30, 0, out.ctypes.data, 9, rem.ctypes.data) == -1
    assert cpu(rows.ctypes.data, 9, 30, 0, None, 9, rem.ctypes.data) == -1
    assert cpu(rows.ctypes.data, 9, 30, 0, out.ctypes.data, 9, None) == -1
    assert cpu(None, 0, 30, 0, None, 0, rem.ctypes.data) == 0 and int(rem[0]) == 0
    assert cpu(rows.ctypes.data, 9, 30, 0, None, 0, rem.ctypes.data) == 6 and int(rem[0]) == 9
    # table entries validate before anything is launched
    assert L.nsd_flow_expire_workspace_bytes(None) == 0
    for flags in (0, 1, 2):
        assert L.nsd_flow_expire_device(None, 5, flags, None, 0, None, None, None) == -1
        assert L.nsd_flow_expire(None, 5, flags, None, 0, None) == -1
    sink = nsd.FLOW_SINK(lambda rows, n, user: 0)
    assert L.nsd_pcap_flows_expire(None, 0, None, None, 256, 512, 0, sink, None) == -1
    assert L.nsd_pcap_flows_expire(b"/nonexistent.pcap", 0, None, None, 256, 512, 0, sink, None) == -1


def test_expire_device_entries_fail_loudly_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(nsd.NsdError):
        nsd.FlowTable(16).expire(5)
    with pytest.raises(nsd.NsdError):
        nsd.FlowTable(16).expire_device(5)
    # the host rules need none
    rest, gone, q = nsd.flow_expire_cpu(make_rows(known_rows()), 30)
    assert (len(rest), len(gone), q) == (3, 6, 6)


# ---- GPU --------------------------------------------------------------------------
def expire_checked(table, before, flags, cap):
    """expire_device into poisoned outputs and a poisoned workspace: exactly
    d_count[0] <= cap rows written, the bytes after them still poison, no
    written row all poison.  (rows sorted by first, [removed, qualified])."""
    import torch
    buf = torch.full(((cap + 1) * nsd.FLOW_BYTES,), T.FILL, dtype=torch.uint8, device="cuda")
    count = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    ws = torch.full((nsd.lib().nsd_flow_expire_workspace_bytes(table.h),), T.FILL, dtype=torch.uint8, device="cuda")
    assert ws.numel() == 2048 + 80 * table.slots
    table.expire_device(before, flags, max_flows=cap, flows=buf, count=count, workspace=ws)
    torch.cuda.synchronize()
    c = [int(x) for x in count.cpu()]
    k = c[0]
    assert 0 <= k <= cap and k == min(c[1], cap), c
    host = buf.cpu().numpy()
    assert (host[k * nsd.FLOW_BYTES:] == T.FILL).all(), "bytes past the last row were written"
    assert not (host[:k * nsd.FLOW_BYTES].reshape(k, nsd.FLOW_BYTES) == T.FILL).all(axis=1).any()
    rows = host[:k * nsd.FLOW_BYTES].view(nsd.FLOW_DTYPE)
    return rows[np.argsort(rows["first"], kind="stable")], c


def assert_table(table, want, what=""):
    """The table's export (poisoned buffer) is the dict `want`; the stats."""
    flows, stats, count = F.export_checked(table, table.slots)
    assert count == len(want), what
    assert rows_list(flows) == by_first(want), what
    st = [int(x) for x in stats]
    assert st[F.ST_FLOWS] == len(want) and st[7] == 0, what
    return st


def batch_model(name, make):
    frames, desc, rec, ext, m, st = F.cached(name, make)
    return frames, desc, m, st


@pytest.mark.gpu
def test_broken_probe_chains(device_fill):
    """16 flows in 16 slots: every probe chain runs through slots of other
    flows and round the table's end.  Half of them leave; the same batch again
    must find every survivor (doubled counts) and put every expired flow in as
    a new one.  Emptying the slots in place loses survivors behind them."""
    frames, desc, m, st0 = batch_model("small16", lambda: F.many_flows(16 * 9, 16))
    t = nsd.FlowTable(8)
    assert t.slots == 16 and len(m) == 16
    F.feed(t, frames, desc)
    before = sorted(v[4] for v in m.values())[8]
    gone, stay = expire_model(m, before)
    assert len(gone) == 8 == len(stay)
    rows, c = expire_checked(t, before, 0, 16)
    assert c == [8, 8] and rows_list(rows) == by_first(gone)
    st = assert_table(t, stay, "after the expiry")
    assert st[ST_EXPIRED] == 8 and st[:5] == st0[:5]
    F.feed(t, frames, desc, base=1000)
    again = {k: v[:3] + [v[3] + 1000, v[4] + 1000] for k, v in m.items()}
    want = merge(stay, again)
    assert sum(1 for k in stay if want[k][1] == 2 * m[k][1] and want[k][3] == m[k][3]) == 8
    assert sum(1 for k in gone if want[k] == again[k]) == 8
    st = assert_table(t, want, "after the second update")
    assert st[F.ST_FLOWS] == 16 and st[F.ST_FULL] == 0 and st[ST_EXPIRED] == 8
    assert st[F.ST_PKTS] == st[F.ST_KEYED] == 2 * 16 * 9
    t.close()


@pytest.mark.gpu
def test_formerly_full_table(device_fill):
    """40 flows into 16 slots, everything expired, then 16 other flows: all
    enter, FULL is what it was."""
    lens = [1 + (j * 7) % 23 for j in range(40)]
    frames, desc, m, _ = batch_model("small40", lambda: F.many_flows(0, 40, lens=lens))
    t = nsd.FlowTable(8)
    F.feed(t, frames, desc)
    flows, stats, count = F.export_checked(t, 64)
    held = dict(F.rows_of(flows))
    full = int(stats[F.ST_FULL])
    assert count == 16 and full == sum(v[1] for k, v in m.items() if k not in held) > 0
    rows, c = expire_checked(t, U64_MAX, 0, 16)
    assert c == [16, 16] and rows_list(rows) == by_first(held)
    st = assert_table(t, {}, "emptied")
    assert st[ST_EXPIRED] == 16 and st[F.ST_FULL] == full

    def others():
        return T.batch_from_packets([E.eth(0x0800) + E.ipv4(17, 8, src=0x0E000000 + i % 16) + E.udp(7000 + i % 16, 53)
                                     for i in range(16 * 3)])
    frames2, desc2, m2, _ = batch_model("other16", others)
    assert len(m2) == 16 and not set(m2) & set(m)
    F.feed(t, frames2, desc2, base=5000)
    st = assert_table(t, {k: v[:3] + [v[3] + 5000, v[4] + 5000] for k, v in m2.items()}, "the other flows")
    assert st[F.ST_FLOWS] == 16 and st[F.ST_FULL] == full and st[ST_EXPIRED] == 16
    t.close()


@pytest.mark.gpu
def test_no_stale_counters(device_fill):
    """Expire everything, then one update: the rows of the same update on a
    table just created (pkts / bytes / last / flags start at 0, first at
    UINT64_MAX in every slot)."""
    frames, desc, rec, ext, m, _ = F.few37()
    t, fresh = nsd.FlowTable(64), nsd.FlowTable(64)
    F.feed(t, frames, desc)
    st0 = assert_table(t, m)
    rows, c = expire_checked(t, U64_MAX, PAIRED, 64)
    assert c == [37, 37] and rows_list(rows) == by_first(m)
    F.feed(t, frames, desc[:1000], base=7)
    F.feed(fresh, frames, desc[:1000], base=7)
    want = F.model(frames, desc[:1000], rec[:1000], ext, base=7)[0]
    st = assert_table(t, want, "after expire-all")
    stf = assert_table(fresh, want, "fresh")
    assert st[ST_EXPIRED] == 37 and stf[ST_EXPIRED] == 0
    assert [a - b for a, b in zip(st[:5], st0[:5])] == stf[:5]       # the cumulative words went on counting
    t.close()
    fresh.close()


def reply_to(p, ids, offs):
    """(packet p with the addresses and ports of its flow key the other way
    round, p's address and port bytes), or None for a packet without an IP
    layer or cut inside those bytes."""
    l3 = next((k for k, x in enumerate(ids) if x in (F.IPV4, F.IPV6)), None)
    if l3 is None:
        return None
    o, n = (offs[l3] + 12, 4) if ids[l3] == F.IPV4 else (offs[l3] + 8, 16)
    ports = ids[-1] in (TCP, UDP, F.DCCP)
    o4 = offs[-1]
    if o + 2 * n > len(p) or (ports and o4 + 4 > len(p)):
        return None
    q = bytearray(p)
    q[o:o + n], q[o + n:o + 2 * n] = p[o + n:o + 2 * n], p[o:o + n]
    if ports:
        q[o4:o4 + 2], q[o4 + 2:o4 + 4] = p[o4 + 2:o4 + 4], p[o4:o4 + 2]
    return bytes(q), p[o:o + 2 * n] + (p[o4:o4 + 4] if ports else b"")


def with_replies(name, n):
    """The first n packets of a test_flows batch, every other packet of every
    third flow (in the order the flows appear) followed by a reply to it."""
    def make():
        frames, desc, rec, ext = (F.syn("ipv6x", 4097) if name == "ipv6x" else F.few37(4097))[:4]
        offs, caps = T.desc_off(desc), T.desc_caplen(desc)
        seen, pkts = {}, []
        for i in range(n):
            p = bytes(frames[offs[i]:offs[i] + caps[i]])
            pkts.append(p)
            ids, lo = F.chain_of(rec, ext, i)
            r = None if int(rec[i]["nflags"]) & 0x20 else reply_to(p, ids, lo)
            if r is None:
                continue
            flow = seen.setdefault((ids[-1], r[1]), [len(seen), 0])
            if flow[0] % 3 == 0 and flow[1] % 2 == 0:
                pkts.append(r[0])                                     # (every other packet: the lasts of a pair differ)
            flow[1] += 1
        return T.batch_from_packets(pkts)
    return batch_model(f"replies:{name}:{n}", make)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, PAIRED])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("name", ["ipv6x", "few37"])
def test_device_matches_model(device_fill, name, n, flags):
    """Flow counts either side of a wave and of a block, half of the flows
    idle, a third of them with a reverse in the table."""
    frames, desc, m, st0 = with_replies(name, n)
    if n > 1:
        assert any(reverse(k) in m and reverse(k) != k for k in m)
    t = nsd.FlowTable(2 * n)
    F.feed(t, frames, desc)
    before = sorted(v[4] for v in m.values())[len(m) // 2] + (n == 1)
    gone, stay = expire_model(m, before, flags)
    assert gone and len(gone) <= len(expire_model(m, before, 0)[0])
    rows, c = expire_checked(t, before, flags, len(m))
    assert c == [len(gone), len(gone)], f"{name} n={n}"
    assert rows_list(rows) == by_first(gone), f"{name} n={n}"
    st = assert_table(t, stay, f"{name} n={n}")
    assert st[ST_EXPIRED] == len(gone) and st[:5] == st0[:5]
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, PAIRED])
def test_before_and_max_at_their_edges(device_fill, flags):
    frames, desc, rec, ext = C.talk_batch(4097, 20)
    m, st0 = F.model(frames, desc, rec, ext)
    mid = sorted(v[4] for v in m.values())[len(m) // 2]
    gone, stay = expire_model(m, mid, flags)
    q = len(gone)
    assert q > 3
    t = nsd.FlowTable(64)
    F.feed(t, frames, desc)
    # before = 0 and max = 0: the table as it was, bit for bit
    first = F.export_checked(t, t.slots)
    for before, cap, want in ((0, 64, [0, 0]), (mid, 0, [0, q]), (U64_MAX, 0, [0, len(m)])):
        rows, c = expire_checked(t, before, flags, cap)
        assert c == want and len(rows) == 0
        again = F.export_checked(t, t.slots)
        assert again[0].tobytes() == first[0].tobytes() and list(again[1]) == list(first[1]) == st0
    # max below the qualifying flows: max rows leave, the others stay for the next call
    for cap in (q - 1, 1):
        t.reset()
        F.feed(t, frames, desc)
        rows, c = expire_checked(t, mid, flags, cap)
        assert c == [cap, q] and len(rows) == cap
        took = dict(F.rows_of(rows))
        assert len(took) == cap and all(k in gone and gone[k] == v for k, v in took.items())
        st = assert_table(t, {k: v for k, v in m.items() if k not in took}, f"max={cap}")
        assert st[ST_EXPIRED] == cap
        rows2, c2 = expire_checked(t, mid, flags, 64)
        took2 = dict(F.rows_of(rows2))
        assert c2 == [q - cap, q - cap] and not set(took) & set(took2) and took | took2 == gone
        st = assert_table(t, stay, f"max={cap}, second call")
        assert st[ST_EXPIRED] == q and st[:5] == st0[:5]
    # the host entry: rows in order, the stats after the call
    t.reset()
    F.feed(t, frames, desc)
    rows, n, stats = t.expire(mid, flags, max_flows=q - 1)
    assert n == q and len(rows) == q - 1 and all(k in gone and gone[k] == v for k, v in F.rows_of(rows))
    assert [int(r["first"]) for r in rows] == sorted(int(r["first"]) for r in rows)
    assert int(stats[F.ST_FLOWS]) == len(m) - (q - 1) and int(stats[ST_EXPIRED]) == q - 1
    rows, n, stats = t.expire(mid, flags)
    assert n == 1 == len(rows) and int(stats[F.ST_FLOWS]) == len(stay) and int(stats[ST_EXPIRED]) == q
    assert_table(t, stay, "host entry")
    t.close()


@pytest.mark.gpu
def test_conversations_after_a_rebuild(device_fill):
    frames, desc, rec, ext = C.talk_batch(4097, 1500)
    m, _ = F.model(frames, desc, rec, ext)
    t = nsd.FlowTable(4096)
    F.feed(t, frames, desc)
    mid = sorted(v[4] for v in m.values())[len(m) // 2]
    gone, stay = expire_model(m, mid, PAIRED)
    rows, c = expire_checked(t, mid, PAIRED, len(m))
    assert c == [len(gone), len(gone)] and len(gone) > 100 and len(stay) > 100
    flows, _ = t.export()
    assert dict(F.rows_of(flows)) == stay
    cpu = nsd.conv_cpu(flows, nsd.CONV_BY_BYTES)
    want = C.conv_rows_of(cpu)
    assert any(v[4] for _, v in want) and want == C.ordered(C.conv_model(stay), nsd.CONV_BY_BYTES)
    for k in (9, C.ALL):
        C.assert_topk(t, nsd.CONV_BY_BYTES, k, want, "rebuilt")
    t.close()


@pytest.mark.gpu
def test_captured_chain_replays(device_fill):
    """reset + walk + update + expire + export captured once on one stream (a
    linear chain), replayed over two input contents with the outputs and both
    workspaces poisoned before each replay: the header is zeroed by the chain."""
    import torch
    n, cut = 1500, 1480   # (every flow talks to the end: about two thirds have no packet among the last 20)
    batches = [C.talk(n, 21, seed=1), C.talk(n, 33, seed=2)]
    size = max(len(f) for f, _ in batches)
    frames = torch.zeros(size, dtype=torch.uint8, device="cuda")
    desc = torch.zeros(n, dtype=torch.int64, device="cuda")
    rec = torch.empty(n * nsd.REC_BYTES, dtype=torch.uint8, device="cuda")
    ext = torch.empty(nsd.ext_pool_words(n), dtype=torch.int32, device="cuda")
    used = torch.zeros(1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(nsd.NCOUNTERS, dtype=torch.int64, device="cuda")
    ws = torch.empty(nsd.lib().nsd_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    t = nsd.FlowTable(128)
    gone_buf = torch.empty(129 * nsd.FLOW_BYTES, dtype=torch.uint8, device="cuda")
    gone_count = torch.zeros(2, dtype=torch.int32, device="cuda")
    ews = torch.empty(nsd.lib().nsd_flow_expire_workspace_bytes(t.h), dtype=torch.uint8, device="cuda")
    out = torch.empty(129 * nsd.FLOW_BYTES, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    stats = torch.zeros(nsd.FLOW_NSTATS, dtype=torch.int64, device="cuda")

    def chain():
        used.zero_()
        t.reset()
        nsd.dissect_device(frames, desc, mode=T.PRINT_NORM, rec=rec, ext=ext, ext_used=used, counters=cnt,
                           workspace=ws)
        t.update(frames, desc, rec, ext)
        t.expire_device(cut, PAIRED, max_flows=128, flows=gone_buf, count=gone_count, workspace=ews)
        t.export_device(max_flows=128, flows=out, count=count, stats=stats)

    def load(j):
        f, d = batches[j]
        frames.zero_()
        frames[:len(f)].copy_(torch.from_numpy(f))
        desc.copy_(torch.from_numpy(d.view(np.int64)))

    load(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    for j in (1, 0):
        load(j)
        for x in (rec, ext, ws, out, gone_buf, gone_count, ews):
            x.view(torch.uint8).fill_(T.FILL)
        g.replay()
        torch.cuda.synchronize()
        f, d = batches[j]
        orec, oext, _, _ = T.oracle_records(f, d)
        m, st = F.model(f, d, orec, oext)
        gone, stay = expire_model(m, cut, PAIRED)
        assert 3 < len(gone) < len(expire_model(m, cut, 0)[0]) and stay
        assert [int(x) for x in gone_count.cpu()] == [len(gone), len(gone)], f"replay {j}"
        host = gone_buf.cpu().numpy()
        assert (host[len(gone) * nsd.FLOW_BYTES:] == T.FILL).all()
        rows = host[:len(gone) * nsd.FLOW_BYTES].view(nsd.FLOW_DTYPE)
        assert rows_list(rows[np.argsort(rows["first"])]) == by_first(gone), f"replay {j}"
        c = int(count.cpu()[0])
        host = out.cpu().numpy()
        assert c == len(stay) and (host[c * nsd.FLOW_BYTES:] == T.FILL).all()
        rows = host[:c * nsd.FLOW_BYTES].view(nsd.FLOW_DTYPE)
        assert rows_list(rows[np.argsort(rows["first"])]) == by_first(stay), f"replay {j}"
        got = [int(x) for x in stats.cpu().numpy().view(np.uint64)]
        assert got == st[:5] + [len(stay), len(gone), 0]
    t.close()


def capture_packets():
    """3,000 packets of 100 endpoint pairs (200 flows) in six stretches of 500:
    stretch s talks over pairs 25 (s % 4) .. 25 (s % 4) + 24, so the pairs of
    the first two stretches are quiet for 1,500 packets (750 of the TCP half)
    and return.  UDP and TCP, both directions."""
    rng = np.random.RandomState(21)
    pkts = []
    for i in range(3000):
        p = 25 * ((i // 500) % 4) + int(rng.randint(25))
        back = bool(rng.randint(2))
        pay = bytes(int(rng.randint(0, 30)))
        a, b, pa, pb = 0x0A030000 + p, 0xC0AA0000 + p, 3000 + p, 443
        if back:
            a, b, pa, pb = b, a, pb, pa
        if p % 2:
            q = E.eth(0x0800) + E.ipv4(6, 20 + len(pay), src=a, dst=b) + E.tcp(pa, pb, flags=1 << int(rng.randint(6))) + pay
        else:
            q = E.eth(0x0800) + E.ipv4(17, 8 + len(pay), src=a, dst=b) + E.udp(pa, pb, payload=pay)
        pkts.append(q)
    return pkts


@pytest.mark.gpu
@pytest.mark.parametrize("filtered,flags", [(False, 0), (True, 0), (False, PAIRED), (True, PAIRED)])
def test_pcap_flows_expire(device_fill, tmp_path, filtered, flags):
    """A capture file through nsd_pcap_flows_expire(every = 256, idle = 512)
    against the same loop in Python: chunks of 256 records, the filter, the
    dict update, the expiry at fed - idle; the sink's rows call by call."""
    every, idle = 256, 512
    pkts = capture_packets()
    assert max(len(p) for p in pkts) < 200
    path = str(tmp_path / "quiet.pcap")
    T.write_pcap(path, pkts)
    frames, desc = T.batch_from_packets(pkts)
    rec, ext, _, _ = T.oracle_records(frames, desc)
    prog = nsd.BpfProgram(np.array(F.TCP_ONLY, dtype=nsd.BPF_INSN)) if filtered else None
    keep = np.array([not filtered or p[23] == 6 for p in pkts])
    assert len(F.model(frames, desc, rec, ext)[0]) == 200
    # the model's loop
    table, sunk, fed = {}, [], 0
    for lo in range(0, len(pkts), every):
        idx = np.arange(lo, min(lo + every, len(pkts)))
        idx = idx[keep[idx]]
        table = merge(table, F.model(frames, desc[idx], rec[idx], ext, base=fed)[0])
        fed += len(idx)
        if fed > idle:
            gone, table = expire_model(table, fed - idle, flags)
            if gone:
                sunk.append(by_first(gone))
    assert len(sunk) >= 4 and sum(len(s) for s in sunk) > len(table) > 0
    # some flows went quiet, left, and came back as new flows
    keys = [k for s in sunk for k, _ in s] + list(table)
    assert len(set(keys)) + 10 < len(keys)
    t = nsd.FlowTable(512)
    got_fed, calls = nsd.pcap_flows_expire(path, t, every, idle, flags, prog=prog)
    assert got_fed == fed == int(keep.sum())
    assert [rows_list(c) for c in calls] == sunk
    flows, stats = t.export()
    assert rows_list(flows) == by_first(table)
    st = [int(x) for x in stats]
    assert st[F.ST_FLOWS] == len(table) and st[ST_EXPIRED] == sum(len(s) for s in sunk) and st[F.ST_FULL] == 0
    total = sum(int(c["pkts"].sum()) for c in calls) + int(flows["pkts"].sum())
    assert total == st[F.ST_KEYED] == fed
    # nsd_pcap_flows over the same file: what it gave before there was expiry
    plain = nsd.FlowTable(512)
    assert nsd.pcap_flows(path, plain, prog=prog) == fed
    want, want_st = F.model(frames, desc[keep], rec[keep], ext)
    pflows, pstats = plain.export()
    F.assert_flows(pflows, pstats, want, want_st, "nsd_pcap_flows")
    # a sink that refuses ends the loop
    t.reset()
    refuse = nsd.FLOW_SINK(lambda rows, n, user: 1)
    rc = nsd.lib().nsd_pcap_flows_expire(path.encode(), T.PRINT_NORM, prog.h if prog else None, t.h, every, idle, flags,
                                         refuse, None)
    assert rc == -1
    for x in (t, plain):
        x.close()
    if prog is not None:
        prog.close()
