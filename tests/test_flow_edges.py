"""The flow key on hostile input: truncated frames, the edge / leaf / fuzz
corpora the walk is pinned on, frames at odd addresses, PRINT_LESS records,
cooked batches, an L4 layer past byte 510 and a pool shorter than the records'
slots - the paths of flow_key() (nsd_flow.h) that the well-formed traffic of
test_flows / test_flow_expire / test_flow_times / test_conversations never
reaches: the zero-fill at and past caplen (also inside le32 / le64), the
later-fragment rule, the inline against the ext-pool form, the doubled off2
offsets, and "an ext entry outside the pool is SKIPPED".

The model is test_flows.model over the CPU restatement's records and the frame
bytes (no code shared with the product); rows and all eight stats compare
exactly.  A census over the oracle's records keeps the corpora from going
bland: each test asserts that its corpus still holds the cases it is for.

CPU tests run nsd_flow_cpu (nsd_flow_cpu.cpp, the host form of the shared key
function); GPU tests run the device walk and the update kernels (plain and
timed, nsd_flow_table.h) and export through poisoned buffers.
"""
import numpy as np
import pytest

import edge_cases as E
import fuzz_cases
import leaf_cases
import nsd
import nsd_testlib as T
import test_flow_times as TS
import test_flows as F
from nsd_testlib import device_fill  # noqa: F401  (fixture: nsd_set_debug_fill(0xA5) around each test)

IPV4, IPV6, TCP, UDP, DCCP = F.IPV4, F.IPV6, F.TCP, F.UDP, F.DCCP
MODES = {"norm": T.PRINT_NORM, "less": T.PRINT_LESS}
CORPORA = ["cuts", "edge+leaf", "mutants", "far"]
FAR_HDR = (2048, 512)          # destination-options header sizes: L4 at 14 + 40 + these
EXT_HDR = 4                    # NSD_EXT_HDR_WORDS


# ---- the corpora ------------------------------------------------------------------
def far_packets():
    """IPv6 + one destination-options header of 2048 / 512 bytes + UDP: the L4
    layer starts at byte 2102 / 566, past what off2 (2 * 255) can say, so the
    record takes the ext form with three layers' worth of chain.  Each whole
    packet, then the same cut one, two and three bytes into the UDP ports."""
    out = []
    for j, size in enumerate(FAR_HDR):
        opts = bytes([17, size // 8 - 1]) + bytes(size - 2)                            # Pad1 options
        src = bytes.fromhex("20010db80000000000000000000000f0")[:15] + bytes([0xF0 + j])
        p = E.eth(0x86DD) + E.ipv6(60, size + 12, src=src) + opts + E.udp(0x1234 + j, 0x5678, payload=b"abcd")
        l4 = 14 + 40 + size
        out += [p] + [p[:l4 + c] for c in (1, 2, 3)]
    return out


_pkts = {}


def packets(name):
    if name not in _pkts:
        if name == "cuts":
            p = [q[:c] for q, _ in F.known_packets() for c in range(len(q) + 1)]
            assert len(p) == 894
        elif name == "edge+leaf":
            p = E.cases() + leaf_cases.cases(600)
        elif name == "mutants":
            p = fuzz_cases.mutants(4096, seed=3)
        else:
            p = far_packets()
        _pkts[name] = p
    return _pkts[name]


def batch(name, align=16, mode="norm"):
    """(frames, desc, oracle rec, oracle ext, model flows, model stats), built once."""
    return F.cached(f"edges:{name}:{align}:{mode}", lambda: T.batch_from_packets(packets(name), align=align),
                    mode=MODES[mode])


def layers(rec, ext, i):
    """(ids, offsets, index of the L3 layer or None) of a record that is not OVERFLOW."""
    ids, lo = F.chain_of(rec, ext, i)
    return ids, lo, next((k for k, x in enumerate(ids) if x in (IPV4, IPV6)), None)


def census(frames, desc, rec, ext):
    """What a corpus holds for the key, from the oracle's records alone:
    [packets whose caplen lies strictly inside the L3 address bytes (IPv4 header
    bytes 12..20, IPv6 8..40), packets whose caplen lies inside the L4 key bytes
    (l4off <= caplen < l4off + 14 for TCP, + 4 for UDP and DCCP), keyed records
    in the ext form, keyed later IPv4 fragments (caplen >= the header's byte 8,
    so the fragment offset was captured)]."""
    offs, caps = T.desc_off(desc), T.desc_caplen(desc)
    inside_l3 = inside_l4 = ext_form = later = 0
    for i in range(len(desc)):
        nf = int(rec[i]["nflags"])
        if nf & 0x20:
            continue
        ids, lo, l3 = layers(rec, ext, i)
        if l3 is None:
            continue
        c, o = int(caps[i]), lo[l3]
        a0, a1 = (o + 12, o + 20) if ids[l3] == IPV4 else (o + 8, o + 40)
        inside_l3 += a0 < c < a1
        n4 = {TCP: 14, UDP: 4, DCCP: 4}.get(ids[-1])
        inside_l4 += n4 is not None and lo[-1] <= c < lo[-1] + n4
        ext_form += nf & 7 == 7
        if ids[l3] == IPV4 and c >= o + 8:
            later += int.from_bytes(bytes(frames[offs[i] + o + 6:offs[i] + o + 8]), "big") & 0x1FFF != 0
    return [inside_l3, inside_l4, ext_form, later]


FLOORS = {"cuts": [150, 80, 40, 30], "mutants": [80, 20, 400, 200]}


def check_census(name, frames, desc, rec, ext, mode="norm"):
    """The corpus still holds what the test is for (the floors are those of
    the PRINT_NORM records)."""
    if name in FLOORS and mode == "norm":
        got = census(frames, desc, rec, ext)
        assert all(g >= f for g, f in zip(got, FLOORS[name])), f"{name}: census {got} below {FLOORS[name]}"
    if name == "far" and mode == "norm":
        for j, size in enumerate(FAR_HDR):
            i = 4 * j
            assert int(rec[i]["nflags"]) & 0x27 == 7, "a far packet's record is not in the ext form"
            ids, lo, l3 = layers(rec, ext, i)
            assert ids[l3] == IPV6 and ids[-1] == UDP and lo[-1] == 14 + 40 + size > 510


# ---- CPU ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cuts", "mutants"])
def test_corpus_census(name):
    """The measured census (cuts 170 / 87 / 45 / 33, mutants 99 / 24 / 451 /
    266) stays above its floors at either alignment."""
    for align in (16, 1):
        frames, desc, rec, ext = batch(name, align)[:4]
        check_census(name, frames, desc, rec, ext)


def test_far_packets_are_in_ext_form():
    frames, desc, rec, ext, want, st = batch("far")
    check_census("far", frames, desc, rec, ext)
    # the whole packets' ports, and each cut: sport's high byte, sport, sport (dport's high byte is zero-filled)
    ports = sorted((k[2], k[3]) for k in want)
    assert ports == sorted([(0x1234, 0x5678), (0x1200, 0), (0x1234, 0), (0x1234, 0x5600),
                            (0x1235, 0x5678), (0x1200, 0), (0x1235, 0), (0x1235, 0x5600)])
    assert st[:4] == [8, 8, 0, 0]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("align", [16, 1])
@pytest.mark.parametrize("name", CORPORA)
def test_flow_cpu_matches_model(name, align, mode):
    frames, desc, rec, ext, want, want_st = batch(name, align, mode)
    check_census(name, frames, desc, rec, ext, mode)
    flows, stats = nsd.flow_cpu(frames, desc, rec, ext)
    F.assert_flows(flows, stats, want, want_st, f"{name} align={align} {mode}")
    # the timed host form: a packet that is not keyed lends no timestamp
    ts = TS.stamps(len(desc), 41)
    keys = TS.packet_keys(f"edges:{name}:{align}:{mode}", frames, desc, rec, ext)
    want_ts, _ = TS.model_ts(frames, desc, rec, ext, ts, keys)
    tflows, tstats = nsd.flow_cpu_ts(frames, desc, rec, ts, ext)
    assert TS.rows_of(tflows) == TS.by_first(want_ts) and [int(x) for x in tstats] == want_st


def test_less_records_give_other_flows():
    """PRINT_LESS is no repeat of PRINT_NORM: some chains end elsewhere, and
    with the last layer the flows differ."""
    for name in ("edge+leaf", "mutants"):
        less, norm = batch(name, 16, "less"), batch(name, 16, "norm")
        assert (less[2]["chain"] != norm[2]["chain"]).any() and less[4] != norm[4], name


def test_model_short_pool():
    """The model's own rule for a short pool, on a hand-made case: packet 8 of
    known_packets() is the one ext entry (10 layers: words 0..13 of its 20)."""
    frames, desc = T.batch_from_packets([p for p, _ in F.known_packets()])
    rec, ext, _, _ = T.oracle_records(frames, desc)
    whole, st = F.model(frames, desc, rec, ext)
    assert F.model(frames, desc, rec, ext, ext_words=len(ext)) == (whole, st)
    assert F.model(frames, desc, rec, ext, ext_words=14) == (whole, st)            # the layer words just fit
    for words in (13, 4, 3, 0):
        m, s = F.model(frames, desc, rec, ext, ext_words=words)
        assert s[F.ST_SKIPPED] == 1 and s[F.ST_KEYED] == st[F.ST_KEYED] - 1, words
        assert m == {k: v for k, v in whole.items() if v[3] != 8}


# ---- GPU ---------------------------------------------------------------------------
def walk_and_update(table, frames, desc, mode, ts=None, ext_words=None):
    f, d = F.to_dev(frames, desc)
    rec, ext, _, _ = nsd.dissect_device(f, d, mode=MODES[mode])
    table.update(f, d, rec, ext, ts=None if ts is None else TS.ts_dev(ts))
    return f, d, rec, ext


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("align", [16, 1])
@pytest.mark.parametrize("name", CORPORA)
def test_device_matches_model(device_fill, name, align, mode):
    frames, desc, rec, ext, want, want_st = batch(name, align, mode)
    check_census(name, frames, desc, rec, ext, mode)
    n = len(desc)
    t = nsd.FlowTable(n)                            # max_flows = the packets: nothing is FULL
    walk_and_update(t, frames, desc, mode)
    flows, stats, count = F.export_checked(t, n)
    assert count == len(want)
    F.assert_flows(flows, stats, want, want_st, f"{name} align={align} {mode}")
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("align", [16, 1])
@pytest.mark.parametrize("name", CORPORA)
def test_timed_device_matches_model(device_fill, name, align, mode):
    """t_first / t_last per flow over timestamps in no order: a packet that is
    NOIP or SKIPPED lends none of its own."""
    frames, desc, rec, ext, _, want_st = batch(name, align, mode)
    n = len(desc)
    keys = TS.packet_keys(f"edges:{name}:{align}:{mode}", frames, desc, rec, ext)
    ts = TS.stamps(n, 43)
    unkeyed = [i for i, k in enumerate(keys) if k is None]
    assert unkeyed or name == "far"
    ts[unkeyed[0::2]], ts[unkeyed[1::2]] = 0, TS.U64_MAX          # what must not show in any flow next to it
    want, _ = TS.model_ts(frames, desc, rec, ext, ts, keys)
    t = nsd.FlowTable(n, timed=True)
    walk_and_update(t, frames, desc, mode, ts=ts)
    flows, stats, count = TS.export_checked(t, n)
    assert count == len(want)
    assert TS.rows_of(flows) == TS.by_first(want), f"{name} align={align} {mode}"
    assert [int(x) for x in stats] == want_st
    t.close()


def cooked_batch():
    """test_flows.test_known_answers_cooked's four payloads and every prefix of
    each, with the sockaddr_ll that names its protocol."""
    pay = [E.ipv4(17, 12, src=0x0A000201) + E.udp(9, 10, payload=b"abcd"),
           E.ipv6(6, 20) + E.tcp(11, 12, flags=0x04),
           E.ipv4(17, 12, src=0x0A000201) + E.udp(9, 10, payload=b"efgh"),
           bytes(28)]
    proto = [0x0800, 0x86DD, 0x0800, 0x0806]
    pkts, protos = [], []
    for p, pr in zip(pay, proto):
        cuts = [p] + [p[:c] for c in range(len(p))]
        pkts += cuts
        protos += [pr] * len(cuts)
    sll = np.zeros(len(pkts), dtype=nsd.SLL_DTYPE)
    sll["family"], sll["hatype"], sll["halen"] = 17, 1, 6
    sll["protocol"] = protos
    return pkts, sll, [len(p) for p in pay]


@pytest.mark.gpu
@pytest.mark.parametrize("align", [16, 1])
def test_cooked_batch_on_device(device_fill, align):
    """LINKTYPE_LINUX_SLL walked on the device: the chain starts at the SLL
    head, which has no bytes, so the IP header is at offset 0 of the frame."""
    import torch
    pkts, sll, lens = cooked_batch()
    frames, desc = T.batch_from_packets(pkts, align=align)
    orec, oext, _, _ = T.oracle_records(frames, desc, linktype=nsd.LINKTYPE_LINUX_SLL, sll=sll)
    want, want_st = F.model(frames, desc, orec, oext)
    first = [0, lens[0] + 1, lens[0] + lens[1] + 2]                       # the whole IP packets
    for i in first:
        ids, lo, l3 = layers(orec, oext, i)
        assert l3 is not None and lo[l3] == 0, "the cooked IP header is not at offset 0"
    whole = F.rows_of(nsd.flow_cpu(frames, desc[first], orec[first], oext)[0])
    assert [k for k, _ in whole] == [(F.V4(0x0A000201), F.DST4, 9, 10, IPV4, UDP), (F.S6, F.D6, 11, 12, IPV6, TCP)]
    assert want_st[F.ST_NOIP] >= 29 and want_st[F.ST_KEYED] > 80 and len(want) >= 15
    rec, ext, _ = nsd.entry_batch(frames, desc, linktype=nsd.LINKTYPE_LINUX_SLL, sll=sll)
    f, d = F.to_dev(frames, desc)
    drec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    dext = torch.from_numpy(ext.view(np.int32).copy()).cuda() if len(ext) else None
    t = nsd.FlowTable(len(desc))
    t.update(f, d, drec, dext)
    flows, stats, count = F.export_checked(t, len(desc))
    assert count == len(want)
    F.assert_flows(flows, stats, want, want_st, f"cooked align={align}")
    t.close()


def pool_entries(rec, ext):
    """[(slot, nlayers)] of the ext-form records that are not OVERFLOW, by slot."""
    out = []
    for i in np.nonzero(((rec["nflags"] & 7) == 7) & ((rec["nflags"] & 0x20) == 0))[0]:
        slot = int.from_bytes(bytes(rec[i]["off2"][:4]), "little")
        out.append((slot, int(ext[slot + 1]) & 0xFFFF))
    return sorted(out)


def pool_cuts(rec, ext):
    """Three pool sizes from the entry boundaries of a pool: between two
    entries, inside an entry's header, inside an entry's layer words."""
    ent = pool_entries(rec, ext)
    assert len(ent) >= 9
    a, b, c = ent[len(ent) // 3], ent[len(ent) // 2], ent[(2 * len(ent)) // 3]
    assert c[1] >= 2
    return {"between": a[0], "header": b[0] + 2, "layers": c[0] + EXT_HDR + c[1] - 1}



@pytest.mark.gpu
@pytest.mark.parametrize("where", ["between", "header", "layers"])
@pytest.mark.parametrize("source", ["device", "oracle"])
def test_short_pool(device_fill, source, where):
    """The update is given a prefix of the walk's pool: the records whose
    entries leave it are SKIPPED, every other packet counts as before.
    source = device: the device walk's records and pool (its entry order is its
    own, so the cut points come from the entries of the pool that is cut);
    oracle: the restatement's records and pool handed to the update."""
    import torch
    frames, desc, orec, oext, whole, whole_st = batch("mutants")
    f, d = F.to_dev(frames, desc)
    if source == "device":
        drec, dext, used, _ = nsd.dissect_device(f, d, mode=T.PRINT_NORM)
        torch.cuda.synchronize()
        rec = drec.cpu().numpy().view(nsd.REC_DTYPE)
        ext = dext.cpu().numpy().view(np.uint32)
        assert F.model(frames, desc, rec, ext) == (whole, whole_st)          # the same chains, slot for slot its own
    else:
        rec, ext = orec, oext
        drec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        dext = torch.from_numpy(ext.view(np.int32).copy()).cuda()
    words = pool_cuts(rec, ext)[where]
    want, want_st = F.model(frames, desc, rec, ext, ext_words=words)
    ent = pool_entries(rec, ext)
    gone = [e for e in ent if e[0] + EXT_HDR > words or e[0] + EXT_HDR + min(e[1], 64) > words]
    assert want_st[F.ST_SKIPPED] == whole_st[F.ST_SKIPPED] + len(gone) and 0 < len(gone) < len(ent)
    if where == "header":
        assert any(e[0] < words < e[0] + EXT_HDR for e in gone)
    if where == "layers":
        assert any(e[0] + EXT_HDR < words < e[0] + EXT_HDR + e[1] for e in gone)
    if where == "between":
        assert any(e[0] == words for e in gone)
    t = nsd.FlowTable(len(desc))
    t.update(f, d, drec, dext[:words])
    flows, stats, count = F.export_checked(t, len(desc))
    assert count == len(want)
    F.assert_flows(flows, stats, want, want_st, f"{source} pool cut {where} at {words}")
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ["cuts", "mutants"])
def test_flow_batch_equals_flow_cpu(device_fill, name, mode):
    frames, desc, rec, ext = batch(name, 16, mode)[:4]
    flows, stats = nsd.flow_batch(frames, desc, mode=MODES[mode])
    cflows, cstats = nsd.flow_cpu(frames, desc, rec, ext)
    assert F.rows_of(flows) == F.rows_of(cflows)
    assert list(stats) == list(cstats)
