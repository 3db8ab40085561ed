"""Flow table over dissected batches (nsd_flow_*): the key rules of
include/netsniff_dissect.h "flow table" against a model that shares no code
with the product - a dict over the CPU restatement's records
(T.oracle_records) and the frame bytes - and hand-written answers.

CPU tests run nsd_flow_cpu (the host aggregation over the shared key
function); GPU tests run the kernels (update / commit / export / reset),
compared after sorting by `first` (the device's export order is unspecified).
"""
import os

import numpy as np
import pytest

import edge_cases as E
import nsd
import nsd_testlib as T
from nsd_testlib import device_fill  # noqa: F401  (fixture: nsd_set_debug_fill(0xA5) around each test)

IPV4, IPV6, TCP, UDP, DCCP, ICMP4, ICMP6 = 7, 8, 21, 22, 23, 10, 11
ST_PKTS, ST_KEYED, ST_NOIP, ST_SKIPPED, ST_FULL, ST_FLOWS = range(6)
MAX_CAPLEN = 65535


# ---- the model ----------------------------------------------------------------
def chain_of(rec, ext, i):
    """(ids, offsets) of record i, from the inline form or its ext entry."""
    r = rec[i]
    nl = int(r["nflags"]) & 7
    if nl == 7:
        slot = int.from_bytes(bytes(r["off2"][:4]), "little")
        cnt = int(ext[slot + 1]) & 0xFFFF
        words = [int(w) for w in ext[slot + 4: slot + 4 + cnt]]
        return [w & 0xFF for w in words], [w >> 16 for w in words]
    ids = [(int(r["chain"]) >> (5 * k)) & 31 for k in range(nl)]
    return ids, [0] + [2 * int(r["off2"][k]) for k in range(nl - 1)]


def outside_pool(rec, ext, i, ext_words):
    """The header's rule for a pool of ext_words words: an ext-form record
    whose entry header, or whose layer words, end past the pool."""
    r = rec[i]
    if int(r["nflags"]) & 7 != 7:
        return False
    slot = int.from_bytes(bytes(r["off2"][:4]), "little")
    if slot + 4 > ext_words:
        return True
    return slot + 4 + min(int(ext[slot + 1]) & 0xFFFF, 64) > ext_words


def model(frames, desc, rec, ext, base=0, ext_words=None):
    """{key: [flags, pkts, bytes, first, last]} and the stats, by the rules of
    the header; key = (src16, dst16, sport, dport, l3, l4).  ext_words: the
    size of the pool given (default: it holds every entry)."""
    flows, st = {}, [0] * 8
    offs, caps = T.desc_off(desc), T.desc_caplen(desc)
    for i in range(len(desc)):
        st[ST_PKTS] += 1
        if int(rec[i]["nflags"]) & 0x20 or (ext_words is not None and outside_pool(rec, ext, i, ext_words)):
            st[ST_SKIPPED] += 1
            continue
        pkt = bytes(frames[offs[i]:offs[i] + min(int(caps[i]), MAX_CAPLEN)])
        at = lambda o, n=1: (pkt[o:o + n] + bytes(n))[:n]                # noqa: E731  (zeros past caplen)
        ids, lo = chain_of(rec, ext, i)
        l3 = next((k for k, x in enumerate(ids) if x in (IPV4, IPV6)), None)
        if l3 is None:
            st[ST_NOIP] += 1
            continue
        st[ST_KEYED] += 1
        o = lo[l3]
        later = False
        if ids[l3] == IPV4:
            src, dst = at(o + 12, 4) + bytes(12), at(o + 16, 4) + bytes(12)
            later = int.from_bytes(at(o + 6, 2), "big") & 0x1FFF != 0
        else:
            src, dst = at(o + 8, 16), at(o + 24, 16)
        l4, o4 = ids[-1], lo[-1]
        sport = dport = flags = 0
        if l4 in (TCP, UDP, DCCP) and not later:
            sport, dport = int.from_bytes(at(o4, 2), "big"), int.from_bytes(at(o4 + 2, 2), "big")
            flags = at(o4 + 13)[0] if l4 == TCP else 0
        f = flows.setdefault((src, dst, sport, dport, ids[l3], l4), [0, 0, 0, base + i, base + i])
        f[0] |= flags
        f[1] += 1
        f[2] += int(caps[i])
        f[4] = base + i
    st[ST_FLOWS] = len(flows)
    return flows, st


def rows_of(flows):
    """FLOW_DTYPE rows -> [(key, [flags, pkts, bytes, first, last])] in the rows' order."""
    assert not flows["rsvd"].any()
    return [((bytes(f["src"]), bytes(f["dst"]), int(f["sport"]), int(f["dport"]), int(f["l3"]), int(f["l4"])),
             [int(f["tcp_flags"]), int(f["pkts"]), int(f["bytes"]), int(f["first"]), int(f["last"])])
            for f in flows]


def sorted_model(m):
    return sorted(([k, v] for k, v in m.items()), key=lambda kv: kv[1][3])


def assert_flows(flows, stats, want, want_st, what=""):
    got = [[k, v] for k, v in rows_of(flows)]
    assert [v[3] for _, v in got] == sorted(v[3] for _, v in got), f"{what}: not sorted by first"
    assert got == sorted_model(want), what
    assert [int(x) for x in stats] == want_st, what


def few_flows(n, nflows, seed=7):
    """n packets drawn at random (seeded) from nflows flows: IPv4 / UDP,
    IPv4 / TCP with varying flag bits, IPv6 / UDP and ICMPv4, payloads of
    varying length."""
    rng = np.random.RandomState(seed)
    pkts = []
    for i in range(n):
        f = int(rng.randint(nflows))
        pay = bytes(int(rng.randint(0, 40)))
        kind = f % 4
        if kind == 0:
            p = E.eth(0x0800) + E.ipv4(17, 8 + len(pay), src=0x0A010000 + f) + E.udp(2000 + f, 53, payload=pay)
        elif kind == 1:
            p = E.eth(0x0800) + E.ipv4(6, 20 + len(pay), src=0x0A010000 + f) + \
                E.tcp(3000 + f, 443, flags=1 << int(rng.randint(6))) + pay
        elif kind == 2:
            src = bytes.fromhex("20010db80000000000000000") + E.be32(f)
            p = E.eth(0x86DD) + E.ipv6(17, 8 + len(pay), src=src) + E.udp(4000 + f, 123, payload=pay)
        else:
            p = E.eth(0x0800) + E.ipv4(1, 8 + len(pay), dst=0xC0A80100 + f) + E.icmp(payload=pay)
        pkts.append(p)
    return T.batch_from_packets(pkts)


def many_flows(n, nflows, lens=None):
    """n IPv4 / UDP packets over nflows flows, packet i in flow i % nflows
    (or, with lens, lens[j] packets of flow j, all shuffled with a seed)."""
    if lens is not None:
        order = [j for j, c in enumerate(lens) for _ in range(c)]
        rng = np.random.RandomState(3)
        rng.shuffle(order)
    else:
        order = [i % nflows for i in range(n)]
    pkts = [E.eth(0x0800) + E.ipv4(17, 8 + (j % 5), src=0x0B000000 + j) + E.udp(5000, 6000 + (j & 0xFFF),
                                                                                  payload=bytes(j % 5))
            for j in order]
    return T.batch_from_packets(pkts)


_cache = {}


def cached(name, make, mode=T.PRINT_NORM):
    """(frames, desc, oracle rec, oracle ext, model flows, model stats), built once."""
    if name not in _cache:
        frames, desc = make()
        rec, ext, _, _ = T.oracle_records(frames, desc, mode=mode)
        _cache[name] = (frames, desc, rec, ext) + model(frames, desc, rec, ext)
    return _cache[name]


SYN = {"udp64": T.SYN_UDP64, "imix": T.SYN_IMIX, "ipv6x": T.SYN_IPV6X}


def syn(name, n=4096):
    return cached(f"{name}:{n}", lambda: T.make_batch(SYN[name], n))


def few37(n=4096):
    return cached(f"few37:{n}", lambda: few_flows(n, 37))


# ---- CPU: known answers ---------------------------------------------------------
V4 = lambda a: E.be32(a) + bytes(12)   # noqa: E731
S6 = bytes.fromhex("20010db8000000000000000000000001")
D6 = bytes.fromhex("fe800000000000000000000000000002")
DST4 = V4(0xC0A80001)


def known_packets():
    """[(packet, expected key or None)] written out by hand."""
    P = []
    u = lambda s, d=53: E.udp(s, d, payload=b"abcd")   # noqa: E731
    ip = lambda proto, n, src, **kw: E.ipv4(proto, n, src=src, **kw)   # noqa: E731
    # 0, 1: IPv4 / UDP, one flow of two packets
    k_udp = (V4(0x0A000101), DST4, 1111, 2222, IPV4, UDP)
    P.append((E.eth(0x0800) + ip(17, 12, 0x0A000101) + u(1111, 2222), k_udp))
    P.append((E.eth(0x0800) + ip(17, 12, 0x0A000101) + u(1111, 2222) + b"trailer", k_udp))
    # 2, 3: IPv4 / TCP, SYN then ACK: flags 0x02 | 0x10
    k_tcp = (V4(0x0A000102), DST4, 80, 443, IPV4, TCP)
    P.append((E.eth(0x0800) + ip(6, 20, 0x0A000102) + E.tcp(flags=0x02), k_tcp))
    P.append((E.eth(0x0800) + ip(6, 20, 0x0A000102) + E.tcp(flags=0x10), k_tcp))
    # 4: 802.1Q, 5: QinQ in front
    P.append((E.eth(0x8100) + E.be16(10) + E.be16(0x0800) + ip(17, 12, 0x0A000103) + u(1),
              (V4(0x0A000103), DST4, 1, 53, IPV4, UDP)))
    P.append((E.eth(0x88a8) + E.be16(100) + E.be16(0x8100) + E.be16(5) + E.be16(0x0800) + ip(17, 12, 0x0A000104) +
              u(2), (V4(0x0A000104), DST4, 2, 53, IPV4, UDP)))
    # 6: MPLS
    P.append((E.eth(0x8847) + E.be32((100 << 12) | (1 << 8) | 64) + ip(17, 12, 0x0A000105) + u(3),
              (V4(0x0A000105), DST4, 3, 53, IPV4, UDP)))
    # 7: IPv6 / UDP
    P.append((E.eth(0x86DD) + E.ipv6(17, 12) + u(4), (S6, D6, 4, 53, IPV6, UDP)))
    # 8: IPv6 + 7 destination-option headers + TCP: 10 layers, the ext-pool form
    chain = b"".join(bytes([60 if k < 6 else 6, 0]) + bytes(6) for k in range(7))
    P.append((E.eth(0x86DD) + E.ipv6(60, len(chain) + 20) + chain + E.tcp(5, 6, flags=0x11),
              (S6, D6, 5, 6, IPV6, TCP)))
    # 9: IPv4 / 41 / IPv6 / UDP: outer IPv4 addresses, the UDP's ports
    P.append((E.eth(0x0800) + ip(41, 40 + 12, 0x0A000106) + E.ipv6(17, 12) + u(7),
              (V4(0x0A000106), DST4, 7, 53, IPV4, UDP)))
    # 10: ICMPv4, 11: ICMPv6 (ports 0)
    P.append((E.eth(0x0800) + ip(1, 8, 0x0A000107) + E.icmp(), (V4(0x0A000107), DST4, 0, 0, IPV4, ICMP4)))
    P.append((E.eth(0x86DD) + E.ipv6(58, 8) + bytes([128, 0]) + E.be16(0x1234) + E.be32(1),
              (S6, D6, 0, 0, IPV6, ICMP6)))
    # 12: a later IPv4 fragment carrying "TCP": dispatched to tcp, ports 0, flags 0
    P.append((E.eth(0x0800) + ip(6, 20, 0x0A000108, frag=0x0010) + E.tcp(flags=0x3F),
              (V4(0x0A000108), DST4, 0, 0, IPV4, TCP)))
    # 13: ARP: no IP layer
    P.append((E.eth(0x0806) + bytes(28), None))
    # 14: UDP cut two bytes into its header: sport read, dport zero
    P.append((E.eth(0x0800) + ip(17, 8, 0x0A000109) + E.udp(7777, 8888)[:2],
              (V4(0x0A000109), DST4, 7777, 0, IPV4, UDP)))
    return P


def test_known_answers():
    P = known_packets()
    frames, desc = T.batch_from_packets([p for p, _ in P])
    rec, ext, _, _ = T.oracle_records(frames, desc)
    assert int(rec[8]["nflags"]) & 7 == 7 and not int(rec[8]["nflags"]) & 0x20    # the ext form
    flows, stats = nsd.flow_cpu(frames, desc, rec, ext, base=1000)
    L = [len(p) for p, _ in P]
    want = [
        (P[0][1], [0, 2, L[0] + L[1], 1000, 1001]),
        (P[2][1], [0x12, 2, L[2] + L[3], 1002, 1003]),
        (P[4][1], [0, 1, L[4], 1004, 1004]),
        (P[5][1], [0, 1, L[5], 1005, 1005]),
        (P[6][1], [0, 1, L[6], 1006, 1006]),
        (P[7][1], [0, 1, L[7], 1007, 1007]),
        (P[8][1], [0x11, 1, L[8], 1008, 1008]),
        (P[9][1], [0, 1, L[9], 1009, 1009]),
        (P[10][1], [0, 1, L[10], 1010, 1010]),
        (P[11][1], [0, 1, L[11], 1011, 1011]),
        (P[12][1], [0, 1, L[12], 1012, 1012]),
        (P[14][1], [0, 1, L[14], 1014, 1014]),
    ]
    assert rows_of(flows) == want
    assert [int(x) for x in stats] == [15, 14, 1, 0, 0, 12, 0, 0]
    # the model reads the same packets the same way
    assert sorted_model(model(frames, desc, rec, ext, base=1000)[0]) == [[k, v] for k, v in want]


def test_known_answers_cooked():
    """LINKTYPE_LINUX_SLL: the chain starts at the SLL head (no bytes), the
    IP header at offset 0."""
    pay = [E.ipv4(17, 12, src=0x0A000201) + E.udp(9, 10, payload=b"abcd"),
           E.ipv6(6, 20) + E.tcp(11, 12, flags=0x04),
           E.ipv4(17, 12, src=0x0A000201) + E.udp(9, 10, payload=b"efgh"),
           bytes(28)]
    sll = np.zeros(4, dtype=nsd.SLL_DTYPE)
    sll["family"], sll["hatype"], sll["halen"] = 17, 1, 6
    sll["protocol"] = [0x0800, 0x86DD, 0x0800, 0x0806]
    frames, desc = T.batch_from_packets(pay)
    rec, ext, _, _ = T.oracle_records(frames, desc, linktype=nsd.LINKTYPE_LINUX_SLL, sll=sll)
    flows, stats = nsd.flow_cpu(frames, desc, rec, ext)
    assert rows_of(flows) == [
        ((V4(0x0A000201), DST4, 9, 10, IPV4, UDP), [0, 2, len(pay[0]) + len(pay[2]), 0, 2]),
        ((S6, D6, 11, 12, IPV6, TCP), [0x04, 1, len(pay[1]), 1, 1]),
    ]
    assert [int(x) for x in stats] == [4, 3, 1, 0, 0, 2, 0, 0]


def test_overflow_records_are_skipped():
    """A chain past 64 layers (NSD_F_OVERFLOW) is counted, not keyed."""
    deep = E.eth(0x8100) + (E.be16(7) + E.be16(0x8100)) * 70 + E.be16(7) + E.be16(0x0800) + E.ipv4(17, 8) + E.udp()
    frames, desc = T.batch_from_packets([deep, E.eth(0x0800) + E.ipv4(17, 8) + E.udp()])
    rec, ext, _, _ = T.oracle_records(frames, desc)
    assert int(rec[0]["nflags"]) & 0x20
    flows, stats = nsd.flow_cpu(frames, desc, rec, ext)
    assert len(flows) == 1 and int(flows[0]["first"]) == 1
    assert [int(x) for x in stats] == [2, 1, 0, 1, 0, 1, 0, 0]


@pytest.mark.parametrize("name", ["udp64", "imix", "ipv6x", "few37"])
def test_flow_cpu_matches_model(name):
    frames, desc, rec, ext, want, want_st = few37() if name == "few37" else syn(name)
    if name == "ipv6x":
        assert int(((rec["nflags"] & 7) == 7).sum()) == 1710 and not (rec["nflags"] & 0x20).any()
    if name == "few37":
        assert len(want) == 37
    flows, stats = nsd.flow_cpu(frames, desc, rec, ext, base=5)
    want5 = {k: v[:3] + [v[3] + 5, v[4] + 5] for k, v in want.items()}
    assert_flows(flows, stats, want5, want_st, name)


def test_flow_cpu_output_cap_and_arguments():
    frames, desc, rec, ext, want, _ = few37()
    flows, stats = nsd.flow_cpu(frames, desc, rec, ext, max_flows=5)
    assert [[k, v] for k, v in rows_of(flows)] == sorted_model(want)[:5] and int(stats[ST_FLOWS]) == 37
    L = nsd.lib()
    assert L.nsd_flow_cpu(None, None, 3, None, None, 0, None, 0, None) == -1      # NSD_ERR_ARG
    assert L.nsd_flow_cpu(None, None, 0, None, None, 0, None, 0, None) == 0
    assert nsd.FLOW_DTYPE.itemsize == 72 and nsd.FLOW_DTYPE.fields["pkts"][1] == 40
    # table entries validate before anything is launched
    assert L.nsd_flow_create(0) is None
    assert L.nsd_flow_reset(None, None) == -1 and L.nsd_flow_slots(None) == 0
    assert L.nsd_flow_update_device(None, None, None, 1, None, None, 0, 0, None) == -1
    assert L.nsd_flow_export_device(None, None, 0, None, None, None) == -1
    assert L.nsd_flow_export(None, None, 0, None) == -1
    assert L.nsd_pcap_flows(None, 0, None, None) == -1


def test_flow_device_entries_fail_loudly_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(nsd.NsdError):
        nsd.FlowTable(16)
    frames, desc = T.batch_from_packets([E.eth(0x0800) + E.ipv4(17, 8) + E.udp()])
    with pytest.raises(nsd.NsdError):
        nsd.flow_batch(frames, desc)


# ---- GPU --------------------------------------------------------------------------
def to_dev(frames, desc):
    import torch
    return torch.from_numpy(frames).cuda(), torch.from_numpy(desc.view(np.int64)).cuda()


def feed(table, frames, desc, base=0):
    """walk + update of one host batch on the current stream."""
    f, d = to_dev(frames, desc)
    rec, ext, _, _ = nsd.dissect_device(f, d, mode=T.PRINT_NORM)
    table.update(f, d, rec, ext, base=base)
    return f, d, rec, ext


def export_checked(table, cap):
    """The table's rows (sorted by first) and stats through export_device
    into a poisoned buffer: exactly count rows written, the next still poison."""
    import torch
    buf = torch.full(((cap + 1) * nsd.FLOW_BYTES,), T.FILL, dtype=torch.uint8, device="cuda")
    _, count, stats = table.export_device(max_flows=cap, flows=buf)
    torch.cuda.synchronize()
    count = int(count.cpu()[0])
    host = buf.cpu().numpy()
    k = min(count, cap)
    assert (host[k * nsd.FLOW_BYTES:] == T.FILL).all(), "rows past the count were written"
    rows = host[:k * nsd.FLOW_BYTES].view(nsd.FLOW_DTYPE)
    assert not (host[:k * nsd.FLOW_BYTES].reshape(k, nsd.FLOW_BYTES) == T.FILL).all(axis=1).any()
    return rows[np.argsort(rows["first"], kind="stable")], stats.cpu().numpy().view(np.uint64), count


def sub(batch, n):
    """The first n packets of a cached batch and their model."""
    frames, desc, rec, ext = batch[:4]
    return (frames, desc[:n]) + model(frames, desc[:n], rec[:n], ext)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("name", ["ipv6x", "few37"])
def test_device_matches_model(device_fill, name, n):
    frames, desc, want, want_st = sub(syn("ipv6x", 4097) if name == "ipv6x" else few37(4097), n)
    t = nsd.FlowTable(n)
    feed(t, frames, desc)
    flows, stats, count = export_checked(t, n)
    assert count == len(want)
    assert_flows(flows, stats, want, want_st, f"{name} n={n}")
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nflows", [3, 8192])
def test_contention_and_spread(device_fill, nflows):
    """8,192 packets in 3 flows (most lanes of every wave on one slot) and in
    8,192 flows into max_flows = 8192."""
    frames, desc, rec, ext, want, want_st = cached(f"many:{nflows}", lambda: many_flows(8192, nflows))
    assert len(want) == nflows
    t = nsd.FlowTable(8192)
    feed(t, frames, desc)
    flows, stats, count = export_checked(t, 8192)
    assert count == nflows
    assert_flows(flows, stats, want, want_st)
    t.close()


@pytest.mark.gpu
def test_small_table_wraps_and_fills(device_fill):
    """max_flows = 8: 16 slots.  16 flows all fit (probe chains wrap round the
    table's end); of 40 flows exactly 16 come back, each whole, and FULL is the
    packet total of the other 24."""
    frames, desc, rec, ext, want, want_st = cached("small16", lambda: many_flows(16 * 9, 16))
    t = nsd.FlowTable(8)
    assert t.slots == 16
    feed(t, frames, desc)
    flows, stats, count = export_checked(t, 16)
    assert count == 16
    assert_flows(flows, stats, want, want_st)
    lens = [1 + (j * 7) % 23 for j in range(40)]
    frames, desc, rec, ext, want, want_st = cached("small40", lambda: many_flows(0, 40, lens=lens))
    assert len(want) == 40 and sorted(v[1] for v in want.values()) == sorted(lens)
    t.reset()
    feed(t, frames, desc)
    flows, stats, count = export_checked(t, 64)
    got = dict(rows_of(flows))
    assert count == 16 and len(got) == 16
    for k, v in got.items():
        assert want[k] == v, k                       # wholly in the table
    dropped = sum(v[1] for k, v in want.items() if k not in got)
    st = [int(x) for x in stats]
    assert st[ST_FULL] == dropped and st[ST_FLOWS] == 16
    assert st[ST_PKTS] == st[ST_KEYED] == sum(lens)
    t.close()


@pytest.mark.gpu
def test_accumulation_over_updates_and_reset(device_fill):
    """One batch as three updates with their base values equals one update;
    flows 0..9 appear only in parts one and three (the stored-key path meets
    the new-in-this-launch path); reset + update equals a fresh table."""
    def make():
        a = [j % 30 for j in range(1000)]
        b = [10 + j % 20 for j in range(1111)]
        c = [j % 35 for j in range(900)]
        pk = [E.eth(0x0800) + E.ipv4(6, 20, src=0x0C000000 + j) + E.tcp(100 + j, 200, flags=1 << (i % 5))
              for i, j in enumerate(a + b + c)]
        return T.batch_from_packets(pk)
    frames, desc, rec, ext, want, want_st = cached("three", make)
    assert len(want) == 35
    t = nsd.FlowTable(64)
    keep = []
    for lo, hi in ((0, 1000), (1000, 2111), (2111, 3011)):
        keep.append(feed(t, frames, desc[lo:hi], base=lo))
    flows, stats, _ = export_checked(t, 64)
    assert_flows(flows, stats, want, want_st, "three updates")
    host, hstats = t.export()
    assert_flows(host, hstats, want, want_st, "host export")
    one = nsd.FlowTable(64)
    feed(one, frames, desc)
    flows, stats, _ = export_checked(one, 64)
    assert_flows(flows, stats, want, want_st, "one update")
    t.reset()
    feed(t, frames, desc[:1000], base=0)
    w, ws = model(frames, desc[:1000], rec[:1000], ext)
    flows, stats, _ = export_checked(t, 64)
    assert_flows(flows, stats, w, ws, "after reset")
    t.close()
    one.close()


@pytest.mark.gpu
def test_captured_chain_replays(device_fill):
    """reset + walk + update + export captured once on one stream (a linear
    chain), replayed over two input contents."""
    import torch
    n = 1500
    batches = [few_flows(n, 21, seed=1), few_flows(n, 33, seed=2)]
    size = max(len(f) for f, _ in batches)
    frames = torch.zeros(size, dtype=torch.uint8, device="cuda")
    desc = torch.zeros(n, dtype=torch.int64, device="cuda")
    rec = torch.empty(n * nsd.REC_BYTES, dtype=torch.uint8, device="cuda")
    ext = torch.empty(nsd.ext_pool_words(n), dtype=torch.int32, device="cuda")
    used = torch.zeros(1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(nsd.NCOUNTERS, dtype=torch.int64, device="cuda")
    ws = torch.empty(nsd.lib().nsd_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    out = torch.empty(65 * nsd.FLOW_BYTES, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    stats = torch.zeros(nsd.FLOW_NSTATS, dtype=torch.int64, device="cuda")
    t = nsd.FlowTable(64)

    def chain():
        used.zero_()
        t.reset()
        nsd.dissect_device(frames, desc, mode=T.PRINT_NORM, rec=rec, ext=ext, ext_used=used, counters=cnt,
                           workspace=ws)
        t.update(frames, desc, rec, ext)
        t.export_device(max_flows=64, flows=out, count=count, stats=stats)

    def load(k):
        f, d = batches[k]
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
    for k in (1, 0):
        load(k)
        for x in (rec, ext, ws, out):
            x.view(torch.uint8).fill_(T.FILL)
        g.replay()
        torch.cuda.synchronize()
        f, d = batches[k]
        orec, oext, _, _ = T.oracle_records(f, d)
        want, want_st = model(f, d, orec, oext)
        c = int(count.cpu()[0])
        host = out.cpu().numpy()
        assert c == len(want) and (host[c * nsd.FLOW_BYTES:] == T.FILL).all()
        rows = host[:c * nsd.FLOW_BYTES].view(nsd.FLOW_DTYPE)
        assert_flows(rows[np.argsort(rows["first"])], stats.cpu().numpy().view(np.uint64), want, want_st, f"replay {k}")
    t.close()


TCP_ONLY = [(0x28, 0, 0, 12), (0x15, 0, 3, 0x0800), (0x30, 0, 0, 23), (0x15, 0, 1, 6), (0x06, 0, 0, 0xFFFF),
            (0x06, 0, 0, 0)]   # untagged IPv4 with protocol 6


@pytest.mark.gpu
def test_filter_walk_flows(device_fill):
    """The compacted output of BpfProgram.filter_device feeds the walk and the
    update: the flows of the accepted packets."""
    import torch
    frames, desc, rec, ext = few37()[:4]
    prog = nsd.BpfProgram(np.array(TCP_ONLY, dtype=nsd.BPF_INSN))
    f, d = to_dev(frames, desc)
    verdict, kept, count = prog.filter_device(f, d, compact=True)
    torch.cuda.synchronize()
    m = int(count.cpu()[0])
    v = verdict.cpu().numpy() != 0
    offs, caps = T.desc_off(desc), T.desc_caplen(desc)
    ref = np.array([caps[i] >= 24 and bytes(frames[offs[i] + 12:offs[i] + 14]) == b"\x08\x00" and
                    frames[offs[i] + 23] == 6 for i in range(len(desc))])
    assert 0 < m < len(desc) and (v == ref).all() and m == int(ref.sum())
    kd = kept[:m].contiguous()
    drec, dext, _, _ = nsd.dissect_device(f, kd, mode=T.PRINT_NORM)
    t = nsd.FlowTable(64)
    t.update(f, kd, drec, dext)
    flows, stats, _ = export_checked(t, 64)
    want, want_st = model(frames, desc[ref], rec[ref], ext)
    assert all(k[5] == TCP for k in want)
    assert_flows(flows, stats, want, want_st)
    t.close()
    prog.close()


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("name", ["big", "leaves"])
def test_pcap_flows(device_fill, name, filtered):
    """A capture file through nsd_pcap_flows, with and without a filter: the
    model over the file's (accepted) packets; a record above 65535 bytes
    (big.pcap's second) is keyed from its first 65535 and counts them all."""
    path = os.path.join(T.GOLDEN, name + ".pcap")
    lt, pkts = T.read_pcap(path)
    assert lt == 1
    prog = None
    if filtered:
        # IPv6 only: ethertype 0x86DD
        prog = nsd.BpfProgram(np.array([(0x28, 0, 0, 12), (0x15, 0, 1, 0x86DD), (0x06, 0, 0, 0xFFFF), (0x06, 0, 0, 0)],
                                       dtype=nsd.BPF_INSN))
        pkts = [p for p in pkts if p[12:14] == b"\x86\xdd"]
    frames, desc = T.batch_from_packets([p[:MAX_CAPLEN] for p in pkts])
    rec, ext, _, _ = T.oracle_records(frames, desc)
    full = desc.copy()
    for i, p in enumerate(pkts):
        full[i] = T.desc_pack(int(T.desc_off(desc)[i]), len(p))
    # (the model cuts each packet at 65535 bytes for the key and sums the whole caplen)
    want, want_st = model(frames, full, rec, ext)
    t = nsd.FlowTable(1024)
    assert nsd.pcap_flows(path, t, prog=prog) == len(pkts)
    flows, stats = t.export()
    assert_flows(flows, stats, want, want_st, name)
    t.close()
    if prog is not None:
        prog.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ipv6x", "few37"])
def test_flow_batch_equals_flow_cpu(device_fill, name):
    frames, desc, rec, ext = (syn("ipv6x") if name == "ipv6x" else few37())[:4]
    flows, stats = nsd.flow_batch(frames, desc)
    cflows, cstats = nsd.flow_cpu(frames, desc, rec, ext)
    assert rows_of(flows) == rows_of(cflows)
    assert list(stats) == list(cstats)
