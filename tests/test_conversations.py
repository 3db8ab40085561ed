"""Conversations and top-k from the flow table (nsd_flow_conv_device,
nsd_flow_conversations, nsd_conv_cpu): the pairing and order rules of
include/netsniff_dissect.h "conversations" against a model that shares no
code with the product - conv_model pairs the {key: [flags, pkts, bytes,
first, last]} dict that test_flows.model makes and orders with sorted() - and
hand-written answers.

CPU tests run nsd_flow_cpu -> nsd_conv_cpu; GPU tests run the kernels (pair /
hist / scan / gather) into poisoned outputs and compare the returned set after
sorting it with the model's order (the device's row order is unspecified).
"""
import os

import numpy as np
import pytest

import edge_cases as E
import nsd
import nsd_testlib as T
import test_flows as F
from nsd_testlib import device_fill  # noqa: F401  (fixture: nsd_set_debug_fill(0xA5) around each test)

BY = {"first": 0, "bytes": 1, "pkts": 2}
ALL = 0xFFFFFFFF


# ---- the model ----------------------------------------------------------------
def key_bytes(k):
    """The 40 key bytes of nsd_flow as they lie in memory."""
    src, dst, sport, dport, l3, l4 = k
    return src + dst + sport.to_bytes(2, "little") + dport.to_bytes(2, "little") + bytes([l3, l4, 0, 0])


def conv_model(flows):
    """{key: [flags, pkts, bytes, first, last]} -> [(originator key, [flags_src,
    flags_dst, pkts_src, bytes_src, pkts_dst, bytes_dst, first, last])]."""
    out = []
    for k, v in flows.items():
        src, dst, sport, dport, l3, l4 = k
        rk = (dst, src, dport, sport, l3, l4)
        w = flows.get(rk) if rk != k else None
        if w is None:
            out.append((k, [v[0], 0, v[1], v[2], 0, 0, v[3], v[4]]))
        elif (v[3], key_bytes(k)) < (w[3], key_bytes(rk)):
            out.append((k, [v[0], w[0], v[1], v[2], w[1], w[2], min(v[3], w[3]), max(v[4], w[4])]))
    return out


def order_key(by):
    if by == BY["first"]:
        return lambda kv: kv[1][6]
    if by == BY["bytes"]:
        return lambda kv: (-(kv[1][3] + kv[1][5]), kv[1][6])
    return lambda kv: (-(kv[1][2] + kv[1][4]), kv[1][6])


def ordered(rows, by):
    return sorted(rows, key=order_key(by))


def conv_rows_of(conv):
    """CONV_DTYPE rows -> [(key, [...])] like conv_model's, in the rows' order."""
    return [((bytes(c["src"]), bytes(c["dst"]), int(c["sport"]), int(c["dport"]), int(c["l3"]), int(c["l4"])),
             [int(c["tcp_flags_src"]), int(c["tcp_flags_dst"]), int(c["pkts_src"]), int(c["bytes_src"]),
              int(c["pkts_dst"]), int(c["bytes_dst"]), int(c["first"]), int(c["last"])])
            for c in conv]


def flow_dict(flows):
    return dict(F.rows_of(flows))


def talk(n, npairs, seed=11):
    """n packets drawn at random (seeded) from npairs endpoint pairs, each
    packet going either way at random: IPv4 / UDP, IPv4 / TCP with varying
    flag bits, IPv6 / UDP and ICMPv4 echo / reply, payloads of varying length;
    pair 0 is a flow that is its own reverse."""
    rng = np.random.RandomState(seed)
    pkts = []
    for i in range(n):
        p = int(rng.randint(npairs))
        back = bool(rng.randint(2))
        pay = bytes(int(rng.randint(0, 40)))
        a, b = 0x0A020000 + p, 0xC0A90000 + p
        pa, pb = 2000 + (p & 0x3FFF), 53
        if back:
            a, b, pa, pb = b, a, pb, pa
        kind = p % 4
        if p == 0:
            q = E.eth(0x0800) + E.ipv4(17, 8 + len(pay), src=0x7F000001, dst=0x7F000001) + E.udp(7777, 7777, payload=pay)
        elif kind == 0:
            q = E.eth(0x0800) + E.ipv4(17, 8 + len(pay), src=a, dst=b) + E.udp(pa, pb, payload=pay)
        elif kind == 1:
            q = E.eth(0x0800) + E.ipv4(6, 20 + len(pay), src=a, dst=b) + E.tcp(pa, pb, flags=1 << int(rng.randint(6))) + pay
        elif kind == 2:
            s6 = bytes.fromhex("20010db80000000000000000") + E.be32(a)
            d6 = bytes.fromhex("20010db80000000000000000") + E.be32(b)
            q = E.eth(0x86DD) + E.ipv6(17, 8 + len(pay), src=s6, dst=d6) + E.udp(pa, pb, payload=pay)
        else:
            q = E.eth(0x0800) + E.ipv4(1, 8 + len(pay), src=a, dst=b) + E.icmp(typ=0 if back else 8, payload=pay)
        pkts.append(q)
    return T.batch_from_packets(pkts)


_cache = {}


def cached(name, make):
    """(frames, desc, oracle rec, oracle ext), built once."""
    if name not in _cache:
        frames, desc = make()
        rec, ext, _, _ = T.oracle_records(frames, desc)
        _cache[name] = (frames, desc, rec, ext)
    return _cache[name]


def talk_batch(n, npairs):
    return cached(f"talk:{n}:{npairs}", lambda: talk(n, npairs))


# ---- CPU: known answers ---------------------------------------------------------
V4 = F.V4
IPV4, IPV6, TCP, UDP, ICMP4 = F.IPV4, F.IPV6, F.TCP, F.UDP, F.ICMP4


def known_packets():
    u = lambda s, d, pay=b"abcd": E.udp(s, d, payload=pay)   # noqa: E731
    v4 = lambda proto, n, s, d, **kw: E.eth(0x0800) + E.ipv4(proto, n, src=s, dst=d, **kw)   # noqa: E731
    A, B, C, D, G, H, I, J, K, L, S = (0x0A000101, 0xC0A80001, 0x0A000102, 0xC0A80002, 0x0A000103, 0xC0A80003,
                                       0x0A000104, 0xC0A80004, 0x0A000105, 0xC0A80005, 0x0A000106)
    P = [
        v4(17, 12, A, B) + u(1111, 2222),                     # 0  A -> B UDP
        v4(17, 12, A, B) + u(1111, 2222),                     # 1  A -> B
        v4(17, 12, B, A) + u(2222, 1111),                     # 2  B -> A
        v4(17, 12, D, C) + u(4444, 3333),                     # 3  the reply D -> C seen first
        v4(17, 12, C, D) + u(3333, 4444),                     # 4  C -> D
        v4(6, 20, A, B) + E.tcp(1000, 80, flags=0x02),        # 5  SYN
        v4(6, 20, B, A) + E.tcp(80, 1000, flags=0x12),        # 6  SYN|ACK back
        v4(6, 20, G, H) + E.tcp(500, 600, flags=0x10),        # 7  TCP G -> H
        v4(17, 20, H, G) + u(600, 500, bytes(12)),            # 8  UDP H -> G: no pair; 54 bytes like 7
        v4(17, 12, S, S) + u(9999, 9999),                     # 9  its own reverse
        v4(17, 12, S, S) + u(9999, 9999),                     # 10
        v4(1, 8, I, J) + E.icmp(typ=8),                       # 11 echo
        v4(1, 8, J, I) + E.icmp(typ=0),                       # 12 reply
        v4(6, 20, K, L, frag=0x0010) + E.tcp(flags=0x3F),     # 13 a later fragment
        v4(6, 20, L, K, frag=0x0020) + E.tcp(flags=0x3F),     # 14 one back
        E.eth(0x86DD) + E.ipv6(17, 12, src=F.S6, dst=F.D6) + u(40, 50),   # 15 IPv6
        E.eth(0x86DD) + E.ipv6(17, 12, src=F.D6, dst=F.S6) + u(50, 40),   # 16 back
        E.eth(0x0806) + bytes(28),                            # 17 ARP
    ]
    b = 1000   # base
    want = [   # in BY_FIRST order
        ((V4(A), V4(B), 1111, 2222, IPV4, UDP), [0, 0, 2, 92, 1, 46, b + 0, b + 2]),
        ((V4(D), V4(C), 4444, 3333, IPV4, UDP), [0, 0, 1, 46, 1, 46, b + 3, b + 4]),
        ((V4(A), V4(B), 1000, 80, IPV4, TCP), [0x02, 0x12, 1, 54, 1, 54, b + 5, b + 6]),
        ((V4(G), V4(H), 500, 600, IPV4, TCP), [0x10, 0, 1, 54, 0, 0, b + 7, b + 7]),
        ((V4(H), V4(G), 600, 500, IPV4, UDP), [0, 0, 1, 54, 0, 0, b + 8, b + 8]),
        ((V4(S), V4(S), 9999, 9999, IPV4, UDP), [0, 0, 2, 92, 0, 0, b + 9, b + 10]),
        ((V4(I), V4(J), 0, 0, IPV4, ICMP4), [0, 0, 1, 42, 1, 42, b + 11, b + 12]),
        ((V4(K), V4(L), 0, 0, IPV4, TCP), [0, 0, 1, 54, 1, 54, b + 13, b + 14]),
        ((F.S6, F.D6, 40, 50, IPV6, UDP), [0, 0, 1, 66, 1, 66, b + 15, b + 16]),
    ]
    # totals 138 92 108 54 54 92 84 108 132 bytes, 3 2 2 1 1 2 2 2 2 packets: equal
    # bytes (2 / 7, 1 / 5, 3 / 4) fall back on `first`
    orders = {"first": list(range(9)), "bytes": [0, 8, 2, 7, 1, 5, 6, 3, 4], "pkts": [0, 1, 2, 5, 6, 7, 8, 3, 4]}
    return P, b, want, orders


def test_known_answers():
    P, base, want, orders = known_packets()
    assert [len(p) for p in P[:17]] == [46] * 5 + [54] * 4 + [46] * 2 + [42] * 2 + [54] * 2 + [66] * 2
    frames, desc = T.batch_from_packets(P)
    rec, ext, _, _ = T.oracle_records(frames, desc)
    flows, stats = nsd.flow_cpu(frames, desc, rec, ext, base=base)
    assert len(flows) == 15 and int(stats[F.ST_NOIP]) == 1          # ARP makes no row
    for name, perm in orders.items():
        got = conv_rows_of(nsd.conv_cpu(flows, BY[name]))
        assert got == [want[j] for j in perm], name
        # the model reads the same flows the same way
        assert ordered(conv_model(flow_dict(flows)), BY[name]) == got, name


@pytest.mark.parametrize("by", sorted(BY))
def test_conv_cpu_matches_model(by):
    frames, desc, rec, ext = talk_batch(4096, 50)
    base = (1 << 33) + 7
    flows, _ = nsd.flow_cpu(frames, desc, rec, ext, base=base)
    m = F.model(frames, desc, rec, ext, base=base)[0]
    assert flow_dict(flows) == m
    want = ordered(conv_model(m), BY[by])
    kinds = {k[5] for k, _ in want}
    assert 50 <= len(want) < len(flows) and kinds == {TCP, UDP, ICMP4}
    assert sum(1 for _, v in want if v[4]) >= 40 and any(k[4] == IPV6 for k, _ in want)
    assert any(k[0] == k[1] and k[2] == k[3] for k, _ in want)      # the flow that is its own reverse, once
    assert conv_rows_of(nsd.conv_cpu(flows, BY[by])) == want
    shuffled = flows[np.random.RandomState(5).permutation(len(flows))]
    assert conv_rows_of(nsd.conv_cpu(shuffled, BY[by])) == want
    assert conv_rows_of(nsd.conv_cpu(shuffled, BY[by], max_conv=7)) == want[:7]
    assert len(nsd.conv_cpu(flows[:0], BY[by])) == 0


def test_arguments():
    assert nsd.CONV_DTYPE.itemsize == 88 == nsd.CONV_BYTES and nsd.CONV_DTYPE.fields["pkts_src"][1] == 40
    assert (nsd.CONV_BY_FIRST, nsd.CONV_BY_BYTES, nsd.CONV_BY_PKTS) == (0, 1, 2)
    L = nsd.lib()
    assert L.nsd_flow_conv_workspace_bytes(None) == 0
    for by in (0, 3, -1):
        assert L.nsd_flow_conv_device(None, by, 0, None, None, None, None) == -1      # NSD_ERR_ARG
        assert L.nsd_flow_conversations(None, by, 0, None, None) == -1
    row = np.zeros(2, dtype=nsd.FLOW_DTYPE)
    out = np.zeros(2, dtype=nsd.CONV_DTYPE)
    for by in (3, -1):
        assert L.nsd_conv_cpu(row.ctypes.data, 1, by, out.ctypes.data, 2) == -1
    assert L.nsd_conv_cpu(None, 2, 0, out.ctypes.data, 2) == -1
    assert L.nsd_conv_cpu(row.ctypes.data, 1, 0, None, 2) == -1
    assert L.nsd_conv_cpu(None, 0, 0, None, 0) == 0
    assert L.nsd_conv_cpu(row.ctypes.data, 1, 0, None, 0) == 1


def test_flow_table_still_raises_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(nsd.NsdError):
        nsd.FlowTable(16)


# ---- GPU --------------------------------------------------------------------------
def conv_checked(table, by, k, total):
    """conversations_device into poisoned outputs (and a poisoned workspace):
    d_count == [min(k, total), total], exactly that many rows written, the
    bytes after them still poison, no written row all poison.  The rows."""
    import torch
    rows = min(k, total)
    buf = torch.full(((rows + 1) * nsd.CONV_BYTES,), T.FILL, dtype=torch.uint8, device="cuda")
    count = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    ws = torch.full((nsd.lib().nsd_flow_conv_workspace_bytes(table.h),), T.FILL, dtype=torch.uint8, device="cuda")
    table.conversations_device(by, k, conv=buf, count=count, workspace=ws)
    torch.cuda.synchronize()
    assert [int(x) for x in count.cpu()] == [rows, total], (by, k)
    host = buf.cpu().numpy()
    assert (host[rows * nsd.CONV_BYTES:] == T.FILL).all(), "bytes past the last row were written"
    assert not (host[:rows * nsd.CONV_BYTES].reshape(rows, nsd.CONV_BYTES) == T.FILL).all(axis=1).any()
    return host[:rows * nsd.CONV_BYTES].view(nsd.CONV_DTYPE)


def assert_topk(table, by, k, want_all, what=""):
    """The returned set is the first k of the model's order."""
    got = conv_checked(table, by, k, len(want_all))
    assert ordered(conv_rows_of(got), by) == ordered(want_all, by)[:k], f"{what} by={by} k={k}"


# (max_flows, packets, endpoint pairs): 2 slots and one flow, 16 slots, 128
# slots, 8,192 slots (32 blocks of the pair kernel; with 1,500 pairs more
# candidates than one block of the histogram / gather takes)
SHAPES = [(1, 1, 1), (8, 63, 3), (8, 64, 3), (8, 65, 3), (64, 65, 20), (64, 4097, 20), (4096, 63, 1500),
          (4096, 4097, 1500)]


@pytest.mark.gpu
@pytest.mark.parametrize("by", sorted(BY))
@pytest.mark.parametrize("max_flows,n,npairs", SHAPES)
def test_device_matches_model(device_fill, max_flows, n, npairs, by):
    frames, desc, rec, ext = talk_batch(4097, npairs)
    m, st = F.model(frames, desc[:n], rec[:n], ext)
    want = conv_model(m)
    t = nsd.FlowTable(max_flows)
    assert t.slots >= 2 * len(m) or len(m) == 1
    F.feed(t, frames, desc[:n])
    total = len(want)
    for k in sorted({total, ALL, (total + 1) // 2, 1}):
        assert_topk(t, BY[by], k, want, f"{max_flows}/{n}/{npairs}")
    _, stats = t.export()
    assert [int(x) for x in stats] == st                             # the table was only read
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("by", sorted(BY))
def test_k_at_its_edges(device_fill, by):
    """300 flows of two packets each, lengths j % 5: every row ties on packets
    and 60 at a time on bytes, so `first` alone decides inside a group."""
    frames, desc, rec, ext = cached("many300", lambda: F.many_flows(600, 300))
    want = conv_model(F.model(frames, desc, rec, ext)[0])
    total = len(want)
    assert total == 300 and len({v[3] for _, v in want}) == 5
    t = nsd.FlowTable(512)
    F.feed(t, frames, desc)
    for k in (0, 1, 137, total - 1, total, total + 1, ALL):
        assert_topk(t, BY[by], k, want)
    t.close()


@pytest.mark.gpu
def test_high_key_digits(device_fill):
    """Byte counts either side of 2^32 and `first` values up to 2^56: every
    digit of the sort key is decided, not only the low ones.  X and Y are
    8,192 descriptors of one 65,535-byte frame each (536,862,720 bytes an
    update); X is fed 8 times, Y 9 times: Y = 4,831,764,480 > 2^32 > X =
    4,294,901,760, and Y's low 32 bits are the smaller."""
    import torch
    big = lambda src: (E.eth(0x0800) + E.ipv4(17, 65501, src=src, dst=0xC0A80909) +   # noqa: E731
                       E.udp(5000, 6000, payload=bytes(65493)))
    small = lambda src: E.eth(0x0800) + E.ipv4(17, 12, src=src, dst=0xC0A80909) + E.udp(5000, 6000, payload=b"abcd")   # noqa: E731
    X, Y, Z, W = 0x0A0A0001, 0x0A0A0002, 0x0A0A0003, 0x0A0A0004
    t = nsd.FlowTable(16)
    for src, times, base0 in ((X, 8, 0), (Y, 9, 100000)):
        frames, desc = T.batch_from_packets([big(src)])
        assert int(T.desc_caplen(desc)[0]) == 65535
        f, d = F.to_dev(frames, np.repeat(desc, 8192))
        rec, ext, _, _ = nsd.dissect_device(f, d, mode=T.PRINT_NORM)
        for u in range(times):
            t.update(f, d, rec, ext, base=base0 + 10000 * u)
    for src, base in ((Z, (1 << 56) + 5), (W, 1 << 40)):
        F.feed(t, *T.batch_from_packets([small(src)]), base=base)
    torch.cuda.synchronize()
    DST = F.V4(0xC0A80909)
    row = lambda src, pkts, nbytes, first, last: ((F.V4(src), DST, 5000, 6000, IPV4, UDP),   # noqa: E731
                                                  [0, 0, pkts, nbytes, 0, 0, first, last])
    rx = row(X, 8 * 8192, 8 * 8192 * 65535, 0, 70000 + 8191)
    ry = row(Y, 9 * 8192, 9 * 8192 * 65535, 100000, 180000 + 8191)
    rz = row(Z, 1, 46, (1 << 56) + 5, (1 << 56) + 5)
    rw = row(W, 1, 46, 1 << 40, 1 << 40)
    assert ry[1][3] == 4831764480 > 1 << 32 > rx[1][3] == 4294901760 and ry[1][3] & 0xFFFFFFFF < rx[1][3] & 0xFFFFFFFF
    for by, order in ((BY["bytes"], [ry, rx, rw, rz]), (BY["pkts"], [ry, rx, rw, rz]), (BY["first"], [rx, ry, rw, rz])):
        for k in (1, 2, 3, 4):
            got = conv_checked(t, by, k, 4)
            assert ordered(conv_rows_of(got), by) == order[:k], (by, k)
    t.close()


def both_ways(lens):
    """lens[j] packets of flow j and as many of its reverse, shuffled (seeded)."""
    order = [(j, back) for j, c in enumerate(lens) for back in (0, 1) for _ in range(c)]
    np.random.RandomState(9).shuffle(order)
    pkts = []
    for j, back in order:
        a, b, pa, pb = 0x0B000000 + j, 0xC0A80A0A, 5000, 6000 + j
        if back:
            a, b, pa, pb = b, a, pb, pa
        pkts.append(E.eth(0x0800) + E.ipv4(17, 8 + (j % 5), src=a, dst=b) + E.udp(pa, pb, payload=bytes(j % 5)))
    return T.batch_from_packets(pkts)


@pytest.mark.gpu
def test_full_table(device_fill):
    """40 flows in both directions into max_flows = 8: 16 slots, none left
    EMPTY, so the reverse probe of a flow whose reverse was dropped as FULL ends
    by its bound.  The conversations are the model's over what the table
    holds."""
    frames, desc, rec, ext = cached("both40", lambda: both_ways([1 + (j * 7) % 23 for j in range(40)]))
    t = nsd.FlowTable(8)
    assert t.slots == 16
    F.feed(t, frames, desc)
    flows, stats = t.export()
    assert len(flows) == 16 and int(stats[F.ST_FULL]) > 0
    held = flow_dict(flows)
    want = conv_model(held)
    assert 8 <= len(want) <= 16
    for by in BY.values():
        assert_topk(t, by, ALL, want)
        assert_topk(t, by, 3, want)
        host, _ = t.conversations(by)
        assert conv_rows_of(host) == ordered(want, by)
    t.close()


@pytest.mark.gpu
def test_accumulation_and_reset(device_fill):
    """Requests, conversations, then the replies: the _dst columns fill in and
    the order changes; after a reset nothing is written."""
    import torch

    def make():
        req = [E.eth(0x0800) + E.ipv4(17, 8 + 4 * j, src=0x0D000000 + j, dst=0xC0A80B0B) +
               E.udp(1000 + j, 53, payload=bytes(4 * j)) for j in range(12)]
        rep = [E.eth(0x0800) + E.ipv4(17, 8 + 300 - 20 * j, src=0xC0A80B0B, dst=0x0D000000 + j) +
               E.udp(53, 1000 + j, payload=bytes(300 - 20 * j)) for j in range(0, 12, 2)]
        return T.batch_from_packets(req + rep)
    frames, desc, rec, ext = cached("reqrep", make)
    t = nsd.FlowTable(64)
    F.feed(t, frames, desc[:12])
    one = conv_model(F.model(frames, desc[:12], rec[:12], ext)[0])
    assert len(one) == 12 and not any(v[4] for _, v in one)
    for by in BY.values():
        assert_topk(t, by, ALL, one, "requests")
        assert_topk(t, by, 5, one, "requests")
    F.feed(t, frames, desc[12:], base=12)
    two = conv_model(F.model(frames, desc, rec, ext)[0])
    assert len(two) == 12 and sum(1 for _, v in two if v[4]) == 6
    assert ordered(one, BY["bytes"])[0][0] != ordered(two, BY["bytes"])[0][0]
    for by in BY.values():
        assert_topk(t, by, ALL, two, "with replies")
        assert_topk(t, by, 5, two, "with replies")
    t.reset()
    for k in (0, 5, ALL):
        got = conv_checked(t, BY["bytes"], k, 0)
        assert len(got) == 0
    torch.cuda.synchronize()
    t.close()


@pytest.mark.gpu
def test_captured_chain_replays(device_fill):
    """reset + walk + update + conversations_device captured once on one stream
    (a linear chain), replayed over two input contents with the outputs
    poisoned before each replay."""
    import torch
    n, k = 1500, 9
    batches = [talk(n, 21, seed=1), talk(n, 33, seed=2)]
    size = max(len(f) for f, _ in batches)
    frames = torch.zeros(size, dtype=torch.uint8, device="cuda")
    desc = torch.zeros(n, dtype=torch.int64, device="cuda")
    rec = torch.empty(n * nsd.REC_BYTES, dtype=torch.uint8, device="cuda")
    ext = torch.empty(nsd.ext_pool_words(n), dtype=torch.int32, device="cuda")
    used = torch.zeros(1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(nsd.NCOUNTERS, dtype=torch.int64, device="cuda")
    ws = torch.empty(nsd.lib().nsd_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    t = nsd.FlowTable(128)
    out = torch.empty((k + 1) * nsd.CONV_BYTES, dtype=torch.uint8, device="cuda")
    count = torch.zeros(2, dtype=torch.int32, device="cuda")
    cws = torch.empty(nsd.lib().nsd_flow_conv_workspace_bytes(t.h), dtype=torch.uint8, device="cuda")

    def chain():
        used.zero_()
        t.reset()
        nsd.dissect_device(frames, desc, mode=T.PRINT_NORM, rec=rec, ext=ext, ext_used=used, counters=cnt,
                           workspace=ws)
        t.update(frames, desc, rec, ext)
        t.conversations_device(nsd.CONV_BY_BYTES, k, conv=out, count=count, workspace=cws)

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
        for x in (rec, ext, ws, out, cws, count):
            x.view(torch.uint8).fill_(T.FILL)
        g.replay()
        torch.cuda.synchronize()
        f, d = batches[j]
        orec, oext, _, _ = T.oracle_records(f, d)
        want = ordered(conv_model(F.model(f, d, orec, oext)[0]), BY["bytes"])
        assert len(want) > k
        assert [int(x) for x in count.cpu()] == [k, len(want)]
        host = out.cpu().numpy()
        assert (host[k * nsd.CONV_BYTES:] == T.FILL).all()
        rows = host[:k * nsd.CONV_BYTES].view(nsd.CONV_DTYPE)
        assert ordered(conv_rows_of(rows), BY["bytes"]) == want[:k], f"replay {j}"
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("by", sorted(BY))
def test_host_entry_on_a_capture(device_fill, by):
    """pcap -> nsd_pcap_flows -> nsd_flow_conversations: rows in order, equal
    to nsd_conv_cpu over the table's export and to the model."""
    path = os.path.join(T.GOLDEN, "leaves.pcap")
    t = nsd.FlowTable(1024)
    fed = nsd.pcap_flows(path, t)
    flows, fstats = t.export()
    assert fed > 0 and len(flows) > 3
    cpu = nsd.conv_cpu(flows, BY[by])
    want = ordered(conv_model(flow_dict(flows)), BY[by])
    assert conv_rows_of(cpu) == want
    for k in (None, 3, 0, len(want) + 5):
        conv, stats = t.conversations(BY[by], k)
        assert conv.tobytes() == cpu[:k].tobytes(), k
        assert list(stats) == list(fstats)
    t.close()
