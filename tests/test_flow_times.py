"""Capture timestamps in the flow table (nsd_flow_create_timed and the *_ts
entries): the rules of include/netsniff_dissect.h "flow times" against a model
that shares no code with the product - the {key: [flags, pkts, bytes, first,
last]} dict of test_flows.model extended by t_first, t_last (min / max of the
timestamps of the flow's counted packets), split and paired in Python - and
hand-written answers.  Every comparison is exact.

CPU tests run nsd_flow_cpu_ts / nsd_flow_expire_cpu_ts / nsd_conv_cpu_ts.  GPU
tests run every timed kernel instantiation (update, export, expire split /
reinsert under both criteria, conv_gather) into poisoned outputs and
workspaces.
"""
import struct

import numpy as np
import pytest

import edge_cases as E
import nsd
import nsd_testlib as T
import test_conversations as C
import test_flow_expire as X
import test_flows as F
from nsd_testlib import device_fill  # noqa: F401  (fixture: nsd_set_debug_fill(0xA5) around each test)

PAIRED = 1
U64_MAX = (1 << 64) - 1
ST_EXPIRED = 6
IPV4, TCP, UDP = F.IPV4, F.TCP, F.UDP
V4 = F.V4
ERR_ARG = -1


# ---- the model ----------------------------------------------------------------
def stamps(n, seed, extremes=True):
    """n timestamps in no order (seeded), spread over 2^40 ns (any 32-bit
    truncation shows), with 0 and 2^64 - 1 among them when there is room."""
    rng = np.random.RandomState(seed)
    ts = np.uint64(1_700_000_000_000_000_000) + rng.randint(0, 1 << 40, size=n).astype(np.uint64)
    if extremes and n >= 3:
        ts[n // 3] = 0
        ts[(2 * n) // 3] = U64_MAX
    assert n < 3 or int(ts.max()) - int(ts.min()) > 1 << 33
    return ts


_keys = {}


def packet_keys(name, frames, desc, rec, ext):
    """The flow key of each packet (None: not keyed), built once per batch."""
    if name not in _keys:
        _keys[name] = [next(iter(F.model(frames, desc[i:i + 1], rec[i:i + 1], ext)[0]), None)
                       for i in range(len(desc))]
    return _keys[name]


def model_ts(frames, desc, rec, ext, ts, keys, idx=None, base=0):
    """{key: [flags, pkts, bytes, first, last, t_first, t_last]} and the stats
    over the packets idx (default all), which count as base, base + 1, ..."""
    idx = np.arange(len(desc)) if idx is None else np.asarray(idx, dtype=np.int64)
    m, st = F.model(frames, desc[idx], rec[idx], ext, base=base)
    out = {k: v + [U64_MAX, 0] for k, v in m.items()}
    for i in idx:
        k = keys[i]
        if k is not None:
            o, t = out[k], int(ts[i])
            o[5], o[6] = min(o[5], t), max(o[6], t)
    return out, st


def merge_ts(into, more):
    """What a further update does to a timed table."""
    out = {k: list(v) for k, v in into.items()}
    for k, v in more.items():
        if k in out:
            o = out[k]
            out[k] = [o[0] | v[0], o[1] + v[1], o[2] + v[2], min(o[3], v[3]), max(o[4], v[4]), min(o[5], v[5]),
                      max(o[6], v[6])]
        else:
            out[k] = list(v)
    return out


def expire_model(flows, before, flags=0, by_time=True):
    """(expired, remaining): a flow qualifies when its t_last (by_time) or its
    last is below `before`; PAIRED: and its reverse's, when that is in the table."""
    j = 6 if by_time else 4

    def idle(k):
        if not flows[k][j] < before:
            return False
        rk = X.reverse(k)
        if flags & PAIRED and rk != k and rk in flows:
            return flows[rk][j] < before
        return True
    gone = {k: v for k, v in flows.items() if idle(k)}
    return gone, {k: v for k, v in flows.items() if k not in gone}


def conv_model_ts(flows):
    """conv_model with the times: [(originator key, [..., first, last, t_first, t_last])]."""
    plain = dict(C.conv_model({k: v[:5] for k, v in flows.items()}))
    out = []
    for k, v in plain.items():
        rk = X.reverse(k)
        w = flows.get(rk) if rk != k else None
        f = flows[k]
        out.append((k, v + ([min(f[5], w[5]), max(f[6], w[6])] if w is not None else [f[5], f[6]])))
    return out


def rows_of(flows):
    """FLOWT_DTYPE rows -> [[key, [flags, pkts, bytes, first, last, t_first, t_last]]] in the rows' order."""
    assert flows.dtype == nsd.FLOWT_DTYPE
    return [[k, v + [int(f["t_first"]), int(f["t_last"])]] for (k, v), f in zip(F.rows_of(flows), flows)]


def conv_rows_of(conv):
    assert conv.dtype == nsd.CONVT_DTYPE
    return [(k, v + [int(c["t_first"]), int(c["t_last"])]) for (k, v), c in zip(C.conv_rows_of(conv), conv)]


def by_first(m):
    return sorted(([k, v] for k, v in m.items()), key=lambda kv: kv[1][3])


def make_rows(items):
    """[(key, [flags, pkts, bytes, first, last, t_first, t_last])] -> FLOWT_DTYPE rows in that order."""
    rows = np.zeros(len(items), dtype=nsd.FLOWT_DTYPE)
    for r, (k, v) in zip(rows, items):
        r["src"], r["dst"] = np.frombuffer(k[0], np.uint8), np.frombuffer(k[1], np.uint8)
        r["sport"], r["dport"], r["l3"], r["l4"] = k[2:]
        r["tcp_flags"], r["pkts"], r["bytes"], r["first"], r["last"], r["t_first"], r["t_last"] = v
    return rows


# ---- CPU: known answers ---------------------------------------------------------
def test_layout():
    assert nsd.FLOWT_DTYPE.itemsize == nsd.FLOWT_BYTES == 88 and nsd.CONVT_DTYPE.itemsize == nsd.CONVT_BYTES == 104
    assert nsd.FLOWT_DTYPE.fields["t_first"][1] == 72 and nsd.CONVT_DTYPE.fields["t_first"][1] == 88
    for name in nsd.FLOW_DTYPE.names:
        assert nsd.FLOWT_DTYPE.fields[name] == nsd.FLOW_DTYPE.fields[name]
    for name in nsd.CONV_DTYPE.names:
        assert nsd.CONVT_DTYPE.fields[name] == nsd.CONV_DTYPE.fields[name]


def test_flow_cpu_ts_known_answers():
    A, B, Cc, D = 0x0A000001, 0x0A000002, 0x0A000003, 0x0A000004
    u = lambda a, b, s, d: E.eth(0x0800) + E.ipv4(17, 12, src=a, dst=b) + E.udp(s, d, payload=b"abcd")   # noqa: E731
    P = [u(A, B, 1, 2), u(A, B, 1, 2), u(A, B, 1, 2),          # 0..2  timestamps descending
         u(B, A, 2, 1), u(B, A, 2, 1),                         # 3, 4  equal timestamps
         u(Cc, D, 5, 6), u(Cc, D, 5, 6),                       # 5, 6  0 and 2^64 - 1
         E.eth(0x0806) + bytes(28)]                            # 7     ARP: not counted, gives no time
    ts = np.array([300, 200, 100, 500, 500, 0, U64_MAX, 7], dtype=np.uint64)
    frames, desc = T.batch_from_packets(P)
    rec, ext, _, _ = T.oracle_records(frames, desc)
    flows, stats = nsd.flow_cpu_ts(frames, desc, rec, ts, ext, base=10)
    n = len(P[0])
    assert rows_of(flows) == [
        [(V4(A), V4(B), 1, 2, IPV4, UDP), [0, 3, 3 * n, 10, 12, 100, 300]],
        [(V4(B), V4(A), 2, 1, IPV4, UDP), [0, 2, 2 * n, 13, 14, 500, 500]],
        [(V4(Cc), V4(D), 5, 6, IPV4, UDP), [0, 2, 2 * n, 15, 16, 0, U64_MAX]],
    ]
    assert [int(x) for x in stats] == [8, 7, 1, 0, 0, 3, 0, 0]
    # the order of the packets does not matter to the times
    perm = np.array([6, 2, 4, 0, 7, 5, 1, 3])
    f2, d2 = T.batch_from_packets([P[i] for i in perm])
    r2, e2, _, _ = T.oracle_records(f2, d2)
    again, _ = nsd.flow_cpu_ts(f2, d2, r2, ts[perm], e2)
    assert sorted((k, v[5:]) for k, v in rows_of(again)) == sorted((k, v[5:]) for k, v in rows_of(flows))
    # the plain rows are the same rows without the times
    plain, pstats = nsd.flow_cpu(frames, desc, rec, ext, base=10)
    assert F.rows_of(plain) == [(k, v[:5]) for k, v in rows_of(flows)] and list(pstats) == list(stats)
    # the model reads the same packets the same way
    keys = packet_keys("known", frames, desc, rec, ext)
    assert by_first(model_ts(frames, desc, rec, ext, ts, keys, base=10)[0]) == rows_of(flows)


def known_rows():
    A, B, Cc, D, Ee, Ff, G, H = (V4(0x0A000001 + j) for j in range(8))
    return [
        ((A, B, 1111, 2222, IPV4, UDP), [0, 3, 300, 0, 10, 50, 900]),       # 0 idle by index (before 30), live by time (500)
        ((B, A, 2222, 1111, IPV4, UDP), [0, 2, 200, 1, 50, 60, 100]),       # 1 live by index, idle by time
        ((Cc, D, 10, 20, IPV4, TCP), [0x12, 4, 400, 2, 5, 70, 499]),        # 2 idle either way
        ((D, Cc, 20, 10, IPV4, TCP), [0x10, 1, 100, 3, 8, 80, 500]),        # 3 t_last == before_ns: stays
        ((Ee, Ff, 5, 6, IPV4, UDP), [0, 1, 60, 4, 4, 0, 0]),                # 4 t_last 0, no reverse
        ((G, H, 7, 8, IPV4, UDP), [0, 1, 60, 5, 60, 90, U64_MAX]),          # 5 t_last 2^64 - 1: never below `before`
    ]


def test_expire_cpu_ts_known_answers():
    R = known_rows()
    rows = make_rows(R)
    pick = lambda idx: [[R[j][0], R[j][1]] for j in idx]   # noqa: E731
    rest, gone, q = nsd.flow_expire_cpu_ts(rows, 500)
    assert q == 3 and rows_of(gone) == pick([1, 2, 4]) and rows_of(rest) == pick([0, 3, 5])
    # PAIRED: B -> A stays with its live reverse, C -> D with D -> C whose t_last is not below 500
    rest, gone, q = nsd.flow_expire_cpu_ts(rows, 500, PAIRED)
    assert q == 1 and rows_of(gone) == pick([4]) and rows_of(rest) == pick([0, 1, 2, 3, 5])
    rest, gone, q = nsd.flow_expire_cpu_ts(rows, 501, PAIRED)
    assert q == 3 and rows_of(gone) == pick([2, 3, 4])
    # the index criterion over the same rows is another rule: there A -> B is the idle direction
    plain = np.zeros(len(rows), dtype=nsd.FLOW_DTYPE)
    for name in nsd.FLOW_DTYPE.names:
        plain[name] = rows[name]
    rest, gone, q = nsd.flow_expire_cpu(plain, 30)
    assert q == 4 and [k for k, _ in F.rows_of(gone)] == [R[j][0] for j in (0, 2, 3, 4)]
    rest, gone, q = nsd.flow_expire_cpu(plain, 30, PAIRED)
    assert q == 3 and [k for k, _ in F.rows_of(gone)] == [R[j][0] for j in (2, 3, 4)]
    # the edges of before_ns
    for flags in (0, PAIRED):
        rest, gone, q = nsd.flow_expire_cpu_ts(rows, 0, flags)
        assert q == 0 and len(gone) == 0 and rows_of(rest) == pick(range(6))
        rest, gone, q = nsd.flow_expire_cpu_ts(rows, U64_MAX, flags)
        assert q == 5 and rows_of(gone) == pick(range(5)) and rows_of(rest) == pick([5])
    rest, gone, q = nsd.flow_expire_cpu_ts(rows, 1)
    assert q == 1 and rows_of(gone) == pick([4])
    # the cap and max = 0
    rest, gone, q = nsd.flow_expire_cpu_ts(rows, 500, 0, max_flows=2)
    assert q == 3 and rows_of(gone) == pick([1, 2]) and rows_of(rest) == pick([0, 3, 4, 5])
    rest, gone, q = nsd.flow_expire_cpu_ts(rows, 500, 0, max_flows=0)
    assert q == 3 and len(gone) == 0 and rows_of(rest) == pick(range(6))
    # the model reads the same rows the same way
    m = dict(R)
    for before, flags, want in ((500, 0, [1, 2, 4]), (500, PAIRED, [4]), (501, PAIRED, [2, 3, 4]), (U64_MAX, 0, range(5))):
        assert by_first(expire_model(m, before, flags)[0]) == pick(want)
    assert by_first(expire_model(m, 30, PAIRED, by_time=False)[0]) == pick([2, 3, 4])


def test_conv_cpu_ts_known_answers():
    R = known_rows()
    conv = nsd.conv_cpu_ts(make_rows(R), nsd.CONV_BY_FIRST)
    want = [
        (R[0][0], [0, 0, 3, 300, 2, 200, 0, 50, 50, 900]),             # A <-> B: min t_first, max t_last
        (R[2][0], [0x12, 0x10, 4, 400, 1, 100, 2, 8, 70, 500]),
        (R[4][0], [0, 0, 1, 60, 0, 0, 4, 4, 0, 0]),                    # one direction only: its own times
        (R[5][0], [0, 0, 1, 60, 0, 0, 5, 60, 90, U64_MAX]),
    ]
    assert conv_rows_of(conv) == want
    assert sorted(conv_model_ts(dict(R)), key=C.order_key(0)) == want
    by_bytes = nsd.conv_cpu_ts(make_rows(R), nsd.CONV_BY_BYTES, max_conv=2)
    assert conv_rows_of(by_bytes) == want[:2]
    # the same pairs as the plain entry gives
    plain = np.zeros(len(R), dtype=nsd.FLOW_DTYPE)
    for name in nsd.FLOW_DTYPE.names:
        plain[name] = make_rows(R)[name]
    assert C.conv_rows_of(nsd.conv_cpu(plain, nsd.CONV_BY_FIRST)) == [(k, v[:8]) for k, v in want]


def cpu_batch(name):
    if name == "few37":
        return F.few37()[:4]
    if name == "many":
        return F.cached("many:300x5", lambda: F.many_flows(1500, 300))[:4]
    return F.syn("ipv6x")[:4]


@pytest.mark.parametrize("name", ["few37", "many", "ipv6x"])
def test_flow_cpu_ts_matches_model(name):
    frames, desc, rec, ext = cpu_batch(name)
    ts = stamps(len(desc), 11)
    assert (np.diff(ts.astype(np.float64)) < 0).any()                 # not monotonic
    keys = packet_keys(name, frames, desc, rec, ext)
    want, want_st = model_ts(frames, desc, rec, ext, ts, keys, base=5)
    flows, stats = nsd.flow_cpu_ts(frames, desc, rec, ts, ext, base=5)
    assert rows_of(flows) == by_first(want) and [int(x) for x in stats] == want_st
    assert any(v[5] == 0 for v in want.values()) and any(v[6] == U64_MAX for v in want.values())
    # expiry and pairing over these rows
    mid = sorted(v[6] for v in want.values())[len(want) // 2]
    for flags in (0, PAIRED):
        gone, stay = expire_model(want, mid, flags)
        rest, exp, q = nsd.flow_expire_cpu_ts(flows, mid, flags)
        assert q == len(gone) and rows_of(exp) == by_first(gone) and rows_of(rest) == by_first(stay)
    conv = nsd.conv_cpu_ts(flows, nsd.CONV_BY_BYTES)
    assert conv_rows_of(conv) == sorted(conv_model_ts(want), key=C.order_key(nsd.CONV_BY_BYTES))


def test_arguments_cpu():
    L = nsd.lib()
    assert L.nsd_flow_create_timed(0) is None and L.nsd_flow_is_timed(None) == 0
    assert L.nsd_flow_update_device_ts(None, None, None, 1, None, None, 0, None, 0, None) == ERR_ARG
    assert L.nsd_flow_export_device_ts(None, None, 0, None, None, None) == ERR_ARG
    assert L.nsd_flow_export_ts(None, None, 0, None) == ERR_ARG
    assert L.nsd_flow_conv_device_ts(None, 0, 0, None, None, None, None) == ERR_ARG
    assert L.nsd_flow_conversations_ts(None, 0, 0, None, None) == ERR_ARG
    for flags in (0, 1, 2):
        assert L.nsd_flow_expire_device_ts(None, 5, flags, None, 0, None, None, None) == ERR_ARG
        assert L.nsd_flow_expire_ts(None, 5, flags, None, 0, None) == ERR_ARG
    rows = make_rows(known_rows())
    out = np.zeros(6, dtype=nsd.FLOWT_DTYPE)
    rem = np.zeros(1, dtype=np.uint64)
    cpu = L.nsd_flow_expire_cpu_ts
    assert cpu(rows.ctypes.data, 6, 500, 2, out.ctypes.data, 6, rem.ctypes.data) == ERR_ARG      # a flag bit
    assert cpu(None, 6, 500, 0, out.ctypes.data, 6, rem.ctypes.data) == ERR_ARG
    assert cpu(rows.ctypes.data, 6, 500, 0, None, 6, rem.ctypes.data) == ERR_ARG
    assert cpu(rows.ctypes.data, 6, 500, 0, out.ctypes.data, 6, None) == ERR_ARG
    assert cpu(rows.ctypes.data, 6, 500, 0, None, 0, rem.ctypes.data) == 3 and int(rem[0]) == 6
    assert L.nsd_flow_cpu_ts(None, None, 3, None, None, None, 0, None, 0, None) == ERR_ARG
    assert L.nsd_flow_cpu_ts(None, None, 0, None, None, None, 0, None, 0, None) == 0
    frames, desc = T.batch_from_packets([E.eth(0x0800) + E.ipv4(17, 8) + E.udp()])
    rec, ext, _, _ = T.oracle_records(frames, desc)
    one = np.zeros(1, dtype=nsd.FLOWT_DTYPE)
    assert L.nsd_flow_cpu_ts(frames.ctypes.data, desc.ctypes.data, 1, rec.ctypes.data, None, None, 0, one.ctypes.data, 1,
                             None) == ERR_ARG                                                  # no timestamps
    assert L.nsd_conv_cpu_ts(None, 3, 0, None, 0) == ERR_ARG and L.nsd_conv_cpu_ts(rows.ctypes.data, 6, 3, None, 0) == ERR_ARG
    sink = nsd.FLOW_SINK(lambda rows, n, user: 0)
    assert L.nsd_pcap_flows_expire_ts(None, 0, None, None, 256, 512, 0, sink, None) == ERR_ARG
    assert L.nsd_pcap_flows_expire_ts(b"/nonexistent.pcap", 0, None, None, 256, 512, 0, sink, None) == ERR_ARG


def test_timed_device_entries_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(nsd.NsdError):
        nsd.FlowTable(16, timed=True)
    # the host rules need none
    rest, gone, q = nsd.flow_expire_cpu_ts(make_rows(known_rows()), 500)
    assert (len(rest), len(gone), q) == (3, 3, 3)


# ---- GPU --------------------------------------------------------------------------
def ts_dev(ts):
    import torch
    return torch.from_numpy(np.ascontiguousarray(ts).view(np.int64)).cuda()


def feed(table, frames, desc, ts, base=0):
    """walk + timed update of one host batch on the current stream."""
    f, d = F.to_dev(frames, desc)
    rec, ext, _, _ = nsd.dissect_device(f, d, mode=T.PRINT_NORM)
    t = ts_dev(ts)
    table.update(f, d, rec, ext, base=base, ts=t)
    return f, d, rec, ext, t


def export_checked(table, cap):
    """export_device_ts into a poisoned buffer: exactly count rows written,
    the rest still poison.  (rows sorted by first, stats, count)."""
    import torch
    B = nsd.FLOWT_BYTES
    buf = torch.full(((cap + 1) * B,), T.FILL, dtype=torch.uint8, device="cuda")
    _, count, stats = table.export_device_ts(max_flows=cap, flows=buf)
    torch.cuda.synchronize()
    count = int(count.cpu()[0])
    host = buf.cpu().numpy()
    k = min(count, cap)
    assert (host[k * B:] == T.FILL).all(), "rows past the count were written"
    assert not (host[:k * B].reshape(k, B) == T.FILL).all(axis=1).any()
    rows = host[:k * B].view(nsd.FLOWT_DTYPE)
    return rows[np.argsort(rows["first"], kind="stable")], stats.cpu().numpy().view(np.uint64), count


def assert_table(table, want, what=""):
    flows, stats, count = export_checked(table, table.slots)
    assert count == len(want), what
    assert rows_of(flows) == by_first(want), what
    st = [int(x) for x in stats]
    assert st[F.ST_FLOWS] == len(want) and st[7] == 0, what
    return st


def expire_checked(table, before, flags, cap, by_time=True):
    """expire_device_ts (or, by_time=False, the index entry with 72-byte rows)
    into poisoned outputs and a poisoned workspace of the timed size."""
    import torch
    B, dt = (nsd.FLOWT_BYTES, nsd.FLOWT_DTYPE) if by_time else (nsd.FLOW_BYTES, nsd.FLOW_DTYPE)
    buf = torch.full(((cap + 1) * B,), T.FILL, dtype=torch.uint8, device="cuda")
    count = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    ws = torch.full((nsd.lib().nsd_flow_expire_workspace_bytes(table.h),), T.FILL, dtype=torch.uint8, device="cuda")
    assert ws.numel() == 2048 + 96 * table.slots
    call = table.expire_device_ts if by_time else table.expire_device
    call(before, flags, max_flows=cap, flows=buf, count=count, workspace=ws)
    torch.cuda.synchronize()
    c = [int(x) for x in count.cpu()]
    k = c[0]
    assert 0 <= k <= cap and k == min(c[1], cap), c
    host = buf.cpu().numpy()
    assert (host[k * B:] == T.FILL).all(), "bytes past the last row were written"
    assert not (host[:k * B].reshape(k, B) == T.FILL).all(axis=1).any()
    rows = host[:k * B].view(dt)
    return rows[np.argsort(rows["first"], kind="stable")], c


def batch(name):
    """(frames, desc, rec, ext, keys) of a named batch, built once."""
    if name == "ipv6x":
        b = F.syn("ipv6x", 4097)[:4]
    elif name == "few37":
        b = F.few37(4097)[:4]
    elif name.startswith("many16k:"):
        nf = int(name.split(":")[1])
        b = F.cached(name, lambda: F.many_flows(16384, nf))[:4]
    elif name == "small16":
        b = F.cached("small16", lambda: F.many_flows(16 * 9, 16))[:4]
    elif name == "small40":
        lens = [1 + (j * 7) % 23 for j in range(40)]
        b = F.cached("small40", lambda: F.many_flows(0, 40, lens=lens))[:4]
    else:
        n, pairs = (int(x) for x in name.split(":")[1:])
        b = C.talk_batch(n, pairs)
    return b + (packet_keys(name, *b),)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("name", ["ipv6x", "few37"])
def test_update_export_matches_model(device_fill, name, n):
    frames, desc, rec, ext, keys = batch(name)
    ts = stamps(n, 100 + n)
    want, want_st = model_ts(frames, desc[:n], rec[:n], ext, ts, keys)
    t = nsd.FlowTable(n, timed=True)
    assert nsd.lib().nsd_flow_is_timed(t.h) == 1
    feed(t, frames, desc[:n], ts)
    flows, stats, count = export_checked(t, n)
    assert count == len(want), f"{name} n={n}"
    assert rows_of(flows) == by_first(want), f"{name} n={n}"
    assert [int(x) for x in stats] == want_st
    # the 72-byte export of a timed table: the same rows without the times
    plain, pstats, _ = F.export_checked(t, n)
    assert F.rows_of(plain) == [(k, v[:5]) for k, v in by_first(want)] and list(pstats) == list(stats)
    host, hstats = t.export_ts()
    assert rows_of(host) == by_first(want) and list(hstats) == list(stats)
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("nflows", [3, 8192])
def test_both_aggregation_paths(device_fill, nflows, cap):
    """16,384 packets in 3 flows: every packet through the block's LDS entries.
    In 8,192 flows over 512 entries a block: most entries are taken by another
    slot and the times go to the table packet by packet.  (cap = 3 caps the
    walk that makes the records; the flow kernels size their own grids.)"""
    frames, desc, rec, ext, keys = batch(f"many16k:{nflows}")
    ts = stamps(len(desc), 9)
    want, want_st = model_ts(frames, desc, rec, ext, ts, keys)
    assert len(want) == nflows
    prev = nsd.set_grid_cap(cap)
    try:
        t = nsd.FlowTable(8192, timed=True)
        feed(t, frames, desc, ts)
        flows, stats, count = export_checked(t, 8192)
    finally:
        nsd.set_grid_cap(prev)
    assert count == nflows and rows_of(flows) == by_first(want) and [int(x) for x in stats] == want_st
    t.close()


@pytest.mark.gpu
def test_accumulation_over_updates_and_reset(device_fill):
    frames, desc, rec, ext, keys = batch("few37")
    n1, n2 = 1000, 2111
    ts = stamps(n2, 5, extremes=False)
    ts[n1:] = ts[n1:] - np.uint64(1 << 41)                    # the second batch lies wholly before the first
    assert int(ts[n1:].max()) < int(ts[:n1].min())
    a, _ = model_ts(frames, desc, rec, ext, ts, keys, idx=np.arange(n1))
    b, _ = model_ts(frames, desc, rec, ext, ts, keys, idx=np.arange(n1, n2), base=n1)
    want = merge_ts(a, b)
    assert all(want[k][5] == b[k][5] < a[k][5] and want[k][6] == a[k][6] for k in a if k in b) and len(want) == 37
    t = nsd.FlowTable(64, timed=True)
    keep = [feed(t, frames, desc[:n1], ts[:n1]), feed(t, frames, desc[n1:n2], ts[n1:], base=n1)]
    assert_table(t, want, "two updates")
    whole, st = model_ts(frames, desc[:n2], rec[:n2], ext, ts, keys)
    assert whole == want
    t.reset()
    assert_table(t, {}, "reset")
    ts2 = stamps(500, 6)
    keep.append(feed(t, frames, desc[:500], ts2))
    assert_table(t, model_ts(frames, desc[:500], rec[:500], ext, ts2, keys)[0], "after reset")
    t.close()


@pytest.mark.gpu
def test_small_table_fills(device_fill):
    """create_timed(4): 8 slots, 40 flows.  Eight come back, each whole and with
    its own times; the packets of the others are FULL and give no time."""
    frames, desc, rec, ext, keys = batch("small40")
    ts = stamps(len(desc), 12)
    want, want_st = model_ts(frames, desc, rec, ext, ts, keys)
    t = nsd.FlowTable(4, timed=True)
    assert t.slots == 8
    feed(t, frames, desc, ts)
    flows, stats, count = export_checked(t, 64)
    got = dict((k, v) for k, v in rows_of(flows))
    assert count == 8 and len(got) == 8
    for k, v in got.items():
        assert want[k] == v, k
    st = [int(x) for x in stats]
    assert st[F.ST_FULL] == sum(v[1] for k, v in want.items() if k not in got) and st[F.ST_FLOWS] == 8
    assert st[F.ST_PKTS] == st[F.ST_KEYED] == len(desc)
    t.close()


@pytest.mark.gpu
def test_time_expiry_broken_probe_chains(device_fill):
    """16 flows in 16 slots, half of them leave by time: the survivors move
    with their times, and a further update accumulates into them."""
    frames, desc, rec, ext, keys = batch("small16")
    ts = stamps(len(desc), 13, extremes=False)
    m, st0 = model_ts(frames, desc, rec, ext, ts, keys)
    t = nsd.FlowTable(8, timed=True)
    assert t.slots == 16 and len(m) == 16
    feed(t, frames, desc, ts)
    before = sorted(v[6] for v in m.values())[8]
    gone, stay = expire_model(m, before)
    assert len(gone) == 8 == len(stay) and gone != expire_model(m, sorted(v[4] for v in m.values())[8], by_time=False)[0]
    rows, c = expire_checked(t, before, 0, 16)
    assert c == [8, 8] and rows_of(rows) == by_first(gone)
    st = assert_table(t, stay, "after the expiry")
    assert st[ST_EXPIRED] == 8 and st[:5] == st0[:5]
    ts2 = stamps(len(desc), 14)
    feed(t, frames, desc, ts2, base=1000)
    want = merge_ts(stay, model_ts(frames, desc, rec, ext, ts2, keys, base=1000)[0])
    st = assert_table(t, want, "after the second update")
    assert st[F.ST_FLOWS] == 16 and st[F.ST_FULL] == 0 and st[ST_EXPIRED] == 8
    t.close()


@pytest.mark.gpu
def test_time_expiry_formerly_full_table(device_fill):
    frames, desc, rec, ext, keys = batch("small40")
    ts = stamps(len(desc), 15, extremes=False)
    m, _ = model_ts(frames, desc, rec, ext, ts, keys)
    t = nsd.FlowTable(8, timed=True)
    feed(t, frames, desc, ts)
    flows, stats, count = export_checked(t, 64)
    held = dict((k, v) for k, v in rows_of(flows))
    full = int(stats[F.ST_FULL])
    assert count == 16 and full > 0 and all(m[k] == v for k, v in held.items())
    rows, c = expire_checked(t, U64_MAX, 0, 16)
    assert c == [16, 16] and rows_of(rows) == by_first(held)
    st = assert_table(t, {}, "emptied")
    assert st[ST_EXPIRED] == 16 and st[F.ST_FULL] == full
    f2, d2, r2, e2 = F.cached("other16", lambda: T.batch_from_packets(
        [E.eth(0x0800) + E.ipv4(17, 8, src=0x0E000000 + i % 16) + E.udp(7000 + i % 16, 53) for i in range(16 * 3)]))[:4]
    ts2 = stamps(len(d2), 16)
    m2, _ = model_ts(f2, d2, r2, e2, ts2, packet_keys("other16", f2, d2, r2, e2), base=5000)
    feed(t, f2, d2, ts2, base=5000)
    st = assert_table(t, m2, "the other flows")
    assert st[F.ST_FLOWS] == 16 and st[F.ST_FULL] == full and st[ST_EXPIRED] == 16
    t.close()


@pytest.mark.gpu
def test_no_stale_times(device_fill):
    """Expire everything, then one update with later and earlier timestamps
    than before: every flow's times are its own (freed slots hold UINT64_MAX / 0)."""
    frames, desc, rec, ext, keys = batch("few37")
    ts = stamps(4097, 17, extremes=False)
    t = nsd.FlowTable(64, timed=True)
    feed(t, frames, desc, ts)
    m, _ = model_ts(frames, desc, rec, ext, ts, keys)
    rows, c = expire_checked(t, U64_MAX, PAIRED, 64)
    assert c == [37, 37] and rows_of(rows) == by_first(m)
    ts2 = np.uint64(1_700_000_300_000_000_000) + np.arange(1000, dtype=np.uint64)   # inside the old range of every flow
    assert all(v[5] < int(ts2.min()) and int(ts2.max()) < v[6] for v in m.values())
    feed(t, frames, desc[:1000], ts2, base=7)
    want = model_ts(frames, desc[:1000], rec[:1000], ext, ts2, keys, base=7)[0]
    st = assert_table(t, want, "after expire-all")
    assert st[ST_EXPIRED] == 37
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, PAIRED])
def test_before_and_max_at_their_edges(device_fill, flags):
    frames, desc, rec, ext, keys = batch("talk:4097:20")
    ts = stamps(4097, 18, extremes=False)
    ts[:] = np.sort(ts)[::-1]                                  # time runs against the index
    m, st0 = model_ts(frames, desc, rec, ext, ts, keys)
    mid = sorted(v[6] for v in m.values())[len(m) // 2]
    gone, stay = expire_model(m, mid, flags)
    q = len(gone)
    assert q > 3 and set(gone) != set(expire_model(m, sorted(v[4] for v in m.values())[len(m) // 2], flags, False)[0])
    t = nsd.FlowTable(64, timed=True)
    feed(t, frames, desc, ts)
    first = export_checked(t, t.slots)
    for before, cap, want in ((0, 64, [0, 0]), (mid, 0, [0, q]), (U64_MAX, 0, [0, len(m)])):
        rows, c = expire_checked(t, before, flags, cap)
        assert c == want and len(rows) == 0
        again = export_checked(t, t.slots)
        assert again[0].tobytes() == first[0].tobytes() and list(again[1]) == list(first[1]) == st0
    for cap in (q - 1, 1):
        t.reset()
        feed(t, frames, desc, ts)
        rows, c = expire_checked(t, mid, flags, cap)
        assert c == [cap, q] and len(rows) == cap
        took = dict((k, v) for k, v in rows_of(rows))
        assert len(took) == cap and all(k in gone and gone[k] == v for k, v in took.items())
        st = assert_table(t, {k: v for k, v in m.items() if k not in took}, f"max={cap}")
        assert st[ST_EXPIRED] == cap
        rows2, c2 = expire_checked(t, mid, flags, 64)
        took2 = dict((k, v) for k, v in rows_of(rows2))
        assert c2 == [q - cap, q - cap] and not set(took) & set(took2) and {**took, **took2} == gone
        st = assert_table(t, stay, f"max={cap}, second call")
        assert st[ST_EXPIRED] == q and st[:5] == st0[:5]
    # the host entry, then a further update into the survivors
    t.reset()
    feed(t, frames, desc, ts)
    rows, n, stats = t.expire_ts(mid, flags, max_flows=q - 1)
    assert n == q and len(rows) == q - 1 and all(k in gone and gone[k] == v for k, v in rows_of(rows))
    assert [int(r["first"]) for r in rows] == sorted(int(r["first"]) for r in rows)
    rows, n, stats = t.expire_ts(mid, flags)
    assert n == 1 == len(rows) and int(stats[F.ST_FLOWS]) == len(stay) and int(stats[ST_EXPIRED]) == q
    assert_table(t, stay, "host entry")
    ts2 = stamps(500, 19)
    feed(t, frames, desc[:500], ts2, base=9000)
    assert_table(t, merge_ts(stay, model_ts(frames, desc[:500], rec[:500], ext, ts2, keys, base=9000)[0]), "update after")
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, PAIRED])
def test_index_expiry_on_a_timed_table(device_fill, flags):
    """nsd_flow_expire_device (criterion `last`, 72-byte rows) on a timed
    table: the survivors keep their times through the rebuild."""
    frames, desc, rec, ext, keys = batch("talk:4097:20")
    ts = stamps(4097, 20)
    m, st0 = model_ts(frames, desc, rec, ext, ts, keys)
    mid = sorted(v[4] for v in m.values())[len(m) // 2]
    gone, stay = expire_model(m, mid, flags, by_time=False)
    assert gone and stay
    t = nsd.FlowTable(64, timed=True)
    feed(t, frames, desc, ts)
    rows, c = expire_checked(t, mid, flags, 64, by_time=False)
    assert c == [len(gone), len(gone)]
    assert [[k, v] for k, v in F.rows_of(rows)] == [[k, v[:5]] for k, v in by_first(gone)]
    st = assert_table(t, stay, "survivors")
    assert st[ST_EXPIRED] == len(gone)
    hrows, n, _ = t.expire(U64_MAX, flags)
    assert n == len(stay) and [[k, v] for k, v in F.rows_of(hrows)] == [[k, v[:5]] for k, v in by_first(stay)]
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("by", ["first", "bytes", "pkts"])
def test_conversations_ts(device_fill, by):
    import torch
    frames, desc, rec, ext, keys = batch("talk:4096:50")
    ts = stamps(4096, 21)
    m, _ = model_ts(frames, desc, rec, ext, ts, keys)
    want = sorted(conv_model_ts(m), key=C.order_key(C.BY[by]))
    assert any(v[4] == 0 for _, v in want) and any(v[4] for _, v in want)      # one-directional ones too
    t = nsd.FlowTable(256, timed=True)
    feed(t, frames, desc, ts)
    B = nsd.CONVT_BYTES
    for k in (0, 1, 7, C.ALL):
        kk = min(k, len(want))
        buf = torch.full(((kk + 1) * B,), T.FILL, dtype=torch.uint8, device="cuda")
        count = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        ws = torch.full((nsd.lib().nsd_flow_conv_workspace_bytes(t.h),), T.FILL, dtype=torch.uint8, device="cuda")
        t.conversations_device_ts(C.BY[by], k, conv=buf, count=count, workspace=ws)
        torch.cuda.synchronize()
        assert [int(x) for x in count.cpu()] == [kk, len(want)]
        host = buf.cpu().numpy()
        assert (host[kk * B:] == T.FILL).all()
        got = sorted(conv_rows_of(host[:kk * B].view(nsd.CONVT_DTYPE)), key=C.order_key(C.BY[by]))
        assert got == want[:kk], f"{by} k={k}"
        conv, _ = t.conversations_ts(C.BY[by], None if k == C.ALL else k)
        assert conv_rows_of(conv) == want[:kk]
        plain, _ = t.conversations(C.BY[by], None if k == C.ALL else k)
        assert C.conv_rows_of(plain) == [(key, v[:8]) for key, v in want[:kk]]
    t.close()


@pytest.mark.gpu
def test_captured_chain_replays(device_fill):
    """reset + walk + update_ts + expire_device_ts + export_device_ts captured
    once on one stream, replayed over two input contents with the outputs and
    workspaces poisoned before each replay."""
    import torch
    n = 1500
    batches = [C.talk(n, 21, seed=1), C.talk(n, 33, seed=2)]
    # time drifts forward with the index (2^30 ns a packet, jitter of two packets): about
    # two thirds of the flows have no packet after the cut, 20 packets before the end
    t0 = np.uint64(1_700_000_000_000_000_000)
    tss = [t0 + (np.arange(n, dtype=np.uint64) << np.uint64(30)) +
           np.random.RandomState(s).randint(0, 1 << 31, size=n).astype(np.uint64) for s in (31, 32)]
    cut = int(t0) + (1480 << 30)
    size = max(len(f) for f, _ in batches)
    frames = torch.zeros(size, dtype=torch.uint8, device="cuda")
    desc = torch.zeros(n, dtype=torch.int64, device="cuda")
    tsd = torch.zeros(n, dtype=torch.int64, device="cuda")
    rec = torch.empty(n * nsd.REC_BYTES, dtype=torch.uint8, device="cuda")
    ext = torch.empty(nsd.ext_pool_words(n), dtype=torch.int32, device="cuda")
    used = torch.zeros(1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(nsd.NCOUNTERS, dtype=torch.int64, device="cuda")
    ws = torch.empty(nsd.lib().nsd_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    t = nsd.FlowTable(128, timed=True)
    B = nsd.FLOWT_BYTES
    gone_buf = torch.empty(129 * B, dtype=torch.uint8, device="cuda")
    gone_count = torch.zeros(2, dtype=torch.int32, device="cuda")
    ews = torch.empty(nsd.lib().nsd_flow_expire_workspace_bytes(t.h), dtype=torch.uint8, device="cuda")
    out = torch.empty(129 * B, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    stats = torch.zeros(nsd.FLOW_NSTATS, dtype=torch.int64, device="cuda")

    def chain():
        used.zero_()
        t.reset()
        nsd.dissect_device(frames, desc, mode=T.PRINT_NORM, rec=rec, ext=ext, ext_used=used, counters=cnt,
                           workspace=ws)
        t.update(frames, desc, rec, ext, ts=tsd)
        t.expire_device_ts(cut, PAIRED, max_flows=128, flows=gone_buf, count=gone_count, workspace=ews)
        t.export_device_ts(max_flows=128, flows=out, count=count, stats=stats)

    def load(j):
        f, d = batches[j]
        frames.zero_()
        frames[:len(f)].copy_(torch.from_numpy(f))
        desc.copy_(torch.from_numpy(d.view(np.int64)))
        tsd.copy_(torch.from_numpy(tss[j].view(np.int64)))

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
        m, st = model_ts(f, d, orec, oext, tss[j], packet_keys(f"talkcap:{j}", f, d, orec, oext))
        gone, stay = expire_model(m, cut, PAIRED)
        assert gone and stay
        assert [int(x) for x in gone_count.cpu()] == [len(gone), len(gone)], f"replay {j}"
        host = gone_buf.cpu().numpy()
        assert (host[len(gone) * B:] == T.FILL).all()
        rows = host[:len(gone) * B].view(nsd.FLOWT_DTYPE)
        assert rows_of(rows[np.argsort(rows["first"])]) == by_first(gone), f"replay {j}"
        c = int(count.cpu()[0])
        host = out.cpu().numpy()
        assert c == len(stay) and (host[c * B:] == T.FILL).all()
        rows = host[:c * B].view(nsd.FLOWT_DTYPE)
        assert rows_of(rows[np.argsort(rows["first"])]) == by_first(stay), f"replay {j}"
        got = [int(x) for x in stats.cpu().numpy().view(np.uint64)]
        assert got == st[:5] + [len(stay), len(gone), 0]
    t.close()


@pytest.mark.gpu
def test_argument_errors_on_tables(device_fill):
    import torch
    frames, desc, rec, ext, keys = batch("few37")
    f, d = F.to_dev(frames, desc[:64])
    drec, dext, _, _ = nsd.dissect_device(f, d, mode=T.PRINT_NORM)
    ts = torch.zeros(65, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L = nsd.lib()
    timed, plain = nsd.FlowTable(64, timed=True), nsd.FlowTable(64)
    assert L.nsd_flow_is_timed(timed.h) == 1 and L.nsd_flow_is_timed(plain.h) == 0
    s = torch.cuda.current_stream().cuda_stream
    upd = lambda t: L.nsd_flow_update_device(t.h, f.data_ptr(), d.data_ptr(), 64, drec.data_ptr(), dext.data_ptr(),   # noqa: E731
                                             dext.numel(), 0, s)
    upd_ts = lambda t, p: L.nsd_flow_update_device_ts(t.h, f.data_ptr(), d.data_ptr(), 64, drec.data_ptr(),          # noqa: E731
                                                      dext.data_ptr(), dext.numel(), p, 0, s)
    assert upd(timed) == ERR_ARG and upd_ts(plain, ts.data_ptr()) == ERR_ARG
    assert upd_ts(timed, None) == ERR_ARG and upd_ts(timed, ts.data_ptr() + 4) == ERR_ARG
    buf = torch.empty(64 * nsd.CONVT_BYTES, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = torch.zeros(8, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(L.nsd_flow_expire_workspace_bytes(timed.h), L.nsd_flow_conv_workspace_bytes(timed.h)),
                     dtype=torch.uint8, device="cuda")
    a = (buf.data_ptr(), cnt.data_ptr(), st.data_ptr(), ws.data_ptr())
    assert L.nsd_flow_export_device_ts(plain.h, a[0], 64, a[1], a[2], s) == ERR_ARG
    assert L.nsd_flow_conv_device_ts(plain.h, 0, 64, a[0], a[1], a[3], s) == ERR_ARG
    assert L.nsd_flow_expire_device_ts(plain.h, 5, 0, a[0], 64, a[1], a[3], s) == ERR_ARG
    assert L.nsd_flow_expire_device_ts(timed.h, 5, 2, a[0], 64, a[1], a[3], s) == ERR_ARG        # bad flags
    assert L.nsd_flow_expire_device_ts(timed.h, 5, 0, a[0] + 4, 64, a[1], a[3], s) == ERR_ARG
    host = np.zeros(64, dtype=nsd.CONVT_DTYPE)
    assert L.nsd_flow_export_ts(plain.h, host.ctypes.data, 64, None) == ERR_ARG
    assert L.nsd_flow_conversations_ts(plain.h, 0, 64, host.ctypes.data, None) == ERR_ARG
    assert L.nsd_flow_expire_ts(plain.h, 5, 0, host.ctypes.data, 64, None) == ERR_ARG
    sink = nsd.FLOW_SINK(lambda rows, n, user: 0)
    assert L.nsd_pcap_flows_expire_ts(b"/nonexistent.pcap", 0, None, plain.h, 256, 512, 0, sink, None) == ERR_ARG
    # nothing was launched: both tables are still empty
    torch.cuda.synchronize()
    assert_table(timed, {})
    assert F.export_checked(plain, 64)[2] == 0
    # and the accepted forms work
    assert upd_ts(timed, ts.data_ptr()) == 0 and upd(plain) == 0
    torch.cuda.synchronize()
    assert export_checked(timed, 64)[2] == F.export_checked(plain, 64)[2] > 0
    timed.close()
    plain.close()


@pytest.mark.gpu
def test_plain_tables_untouched(device_fill):
    """A table of nsd_flow_create: the workspace size, update / export /
    expire, rows bit-identical to nsd_flow_cpu's."""
    frames, desc, rec, ext = F.few37()[:4]
    cflows, cstats = nsd.flow_cpu(frames, desc, rec, ext)
    t = nsd.FlowTable(64)
    assert not t.timed and nsd.lib().nsd_flow_expire_workspace_bytes(t.h) == 2048 + 80 * t.slots
    F.feed(t, frames, desc)
    flows, stats, count = F.export_checked(t, 64)
    assert count == 37 and flows.tobytes() == cflows.tobytes() and list(stats) == list(cstats)
    mid = int(np.sort(cflows["last"])[18])
    rest, gone, q = nsd.flow_expire_cpu(cflows, mid)
    rows, c = X.expire_checked(t, mid, 0, 64)
    assert c == [q, q] and rows.tobytes() == gone.tobytes()
    flows, _, _ = F.export_checked(t, 64)
    assert flows.tobytes() == rest.tobytes()
    t.close()


# ---- capture files ------------------------------------------------------------------
NSEC_MAGIC, USEC_MAGIC = 0xA1B23C4D, 0xA1B2C3D4


def write_pcap_ts(path, pkts, ts, magic):
    """A little-endian pcap whose record i carries ts[i] = (sec, frac)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<IHHiIII", magic, 2, 4, 0, 0, 65535, 1))
        for p, (sec, frac) in zip(pkts, ts):
            f.write(struct.pack("<IIII", sec, frac, len(p), len(p)))
            f.write(bytes(p))


def capture(magic, n=600, big_at=250):
    """n packets of 24 endpoint pairs in three stretches (pairs 0..11, 12..23,
    0..11 again), UDP and TCP both ways, record times mostly ascending by
    about 1 ms with every fifth record stepping back; record `big_at` is a UDP
    packet of 70,000 bytes.  (packets, ts_ns u64, (sec, frac) per record)."""
    rng = np.random.RandomState(41)
    pkts, recs = [], []
    tick = 1_000_000_000 * 1_700_000_000
    for i in range(n):
        p = 12 * ((i // 200) % 2) + int(rng.randint(12))
        back = bool(rng.randint(2))
        pay = bytes(int(rng.randint(0, 30)))
        a, b, pa, pb = 0x0A030000 + p, 0xC0AA0000 + p, 3000 + p, 443
        if back:
            a, b, pa, pb = b, a, pb, pa
        if i == big_at:
            q = E.eth(0x0800) + E.ipv4(17, 8 + 20, src=0x0A0300FE, dst=0xC0AA00FE) + E.udp(9, 9, payload=bytes(20))
            q += bytes(70000 - len(q))
        elif p % 2:
            q = E.eth(0x0800) + E.ipv4(6, 20 + len(pay), src=a, dst=b) + E.tcp(pa, pb, flags=1 << int(rng.randint(6))) + pay
        else:
            q = E.eth(0x0800) + E.ipv4(17, 8 + len(pay), src=a, dst=b) + E.udp(pa, pb, payload=pay)
        pkts.append(q)
        tick += int(rng.randint(500_000, 1_500_000))
        at = tick - (3_000_000 if i % 5 == 4 else 0)
        at -= at % 1000                                         # whole microseconds: the same instants under both magics
        recs.append((at // 1_000_000_000, at % 1_000_000_000 if magic == NSEC_MAGIC else at % 1_000_000_000 // 1000))
    ts = np.array([s * 1_000_000_000 + (f if magic == NSEC_MAGIC else f * 1000) for s, f in recs], dtype=np.uint64)
    assert (np.diff(ts.astype(np.int64)) < 0).any()
    return pkts, ts, recs


def capture_model(pkts):
    """(frames, full desc, rec, ext, keys): each packet keyed from its first
    65535 bytes, counted with its whole length."""
    frames, desc = T.batch_from_packets([p[:F.MAX_CAPLEN] for p in pkts])
    rec, ext, _, _ = T.oracle_records(frames, desc)
    full = desc.copy()
    for i, p in enumerate(pkts):
        full[i] = T.desc_pack(int(T.desc_off(desc)[i]), len(p))
    return frames, full, rec, ext, packet_keys(f"capture:{len(pkts)}", frames, full, rec, ext)


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("magic", [USEC_MAGIC, NSEC_MAGIC])
def test_pcap_flows_into_a_timed_table(device_fill, tmp_path, magic, filtered):
    pkts, ts, recs = capture(magic)
    path = str(tmp_path / "times.pcap")
    write_pcap_ts(path, pkts, recs, magic)
    frames, desc, rec, ext, keys = capture_model(pkts)
    prog = nsd.BpfProgram(np.array(F.TCP_ONLY, dtype=nsd.BPF_INSN)) if filtered else None
    keep = np.array([not filtered or p[23] == 6 for p in pkts])
    idx = np.flatnonzero(keep)
    want, want_st = model_ts(frames, desc, rec, ext, ts, keys, idx=idx)
    assert filtered or any(v[2] >= 70000 for v in want.values())
    t = nsd.FlowTable(256, timed=True)
    assert nsd.pcap_flows(path, t, prog=prog) == len(idx)
    flows, stats = t.export_ts()
    assert rows_of(flows) == by_first(want) and [int(x) for x in stats] == want_st
    t.close()
    if prog is not None:
        prog.close()


@pytest.mark.gpu
@pytest.mark.parametrize("filtered,flags", [(False, 0), (True, 0), (False, PAIRED), (True, PAIRED)])
@pytest.mark.parametrize("every", [1, 64, 1000])
def test_pcap_flows_expire_ts(device_fill, tmp_path, every, filtered, flags):
    """nsd_pcap_flows_expire_ts against the same loop in Python: batches of
    `every` records (the record above 65,535 bytes ends the batch before it and
    is one of its own), the filter, the dict update, now = the largest
    timestamp fed, the expiry at now - idle_ns; the sink's rows call by call."""
    magic = NSEC_MAGIC if every == 64 else USEC_MAGIC
    idle_ns = 60_000_000                                         # 60 ms: a stretch is about 200 ms
    pkts, ts, recs = capture(magic)
    path = str(tmp_path / "quiet.pcap")
    write_pcap_ts(path, pkts, recs, magic)
    frames, desc, rec, ext, keys = capture_model(pkts)
    prog = nsd.BpfProgram(np.array(F.TCP_ONLY, dtype=nsd.BPF_INSN)) if filtered else None
    keep = np.array([not filtered or p[23] == 6 for p in pkts])
    big = [len(p) > F.MAX_CAPLEN for p in pkts]
    table, sunk, fed, now, i = {}, [], 0, 0, 0
    while i < len(pkts):
        j = i + 1
        if not big[i]:
            while j < len(pkts) and j - i < every and not big[j]:
                j += 1
        idx = [x for x in range(i, j) if keep[x]]
        i = j
        if idx:
            table = merge_ts(table, model_ts(frames, desc, rec, ext, ts, keys, idx=idx, base=fed)[0])
            fed += len(idx)
            now = max(now, max(int(ts[x]) for x in idx))
        if now > idle_ns:
            gone, table = expire_model(table, now - idle_ns, flags)
            if gone:
                sunk.append(by_first(gone))
    assert len(sunk) >= 2 and table
    keys_seen = [k for s in sunk for k, _ in s] + list(table)
    assert len(set(keys_seen)) < len(keys_seen)                  # some flows left and came back
    t = nsd.FlowTable(256, timed=True)
    got_fed, calls = nsd.pcap_flows_expire_ts(path, t, every, idle_ns, flags, prog=prog)
    assert got_fed == fed == int(keep.sum())
    assert [rows_of(c) for c in calls] == sunk
    flows, stats = t.export_ts()
    assert rows_of(flows) == by_first(table)
    st = [int(x) for x in stats]
    assert st[F.ST_FLOWS] == len(table) and st[ST_EXPIRED] == sum(len(s) for s in sunk) and st[F.ST_FULL] == 0
    # a sink that refuses ends the loop
    t.reset()
    refuse = nsd.FLOW_SINK(lambda rows, n, user: 1)
    rc = nsd.lib().nsd_pcap_flows_expire_ts(path.encode(), T.PRINT_NORM, prog.h if prog else None, t.h, every, idle_ns,
                                            flags, refuse, None)
    assert rc == ERR_ARG
    t.close()
    if prog is not None:
        prog.close()
