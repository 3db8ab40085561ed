"""pcap replay front end (nsd_pcap.cpp the reader, nsd_replay.cpp the replay
that drives it; read_pcap netsniff-ng.c:640-770, pcap_io.h record formats,
pcap_sg.c reader).

CPU: the reader against the committed pcaps (tiny = C1, edge) in every record
format the reference reads (usec / nsec / Kuznetzov / Borkmann magics, both
byte orders, the *_LL form of SLL files), batch splitting and the end-of-replay
rules.  GPU: the whole `--in` loop (reader -> [device BPF] -> pipelined
device walk -> formatter -> [tprintf wrap]) reproduces the golden text the
reference's parser objects printed for the same files."""
import os
import struct

import numpy as np
import pytest

import nsd
import nsd_testlib as T
from nsd_testlib import device_fill  # noqa: F401  (fixture: nsd_set_debug_fill(0xA5) around each test)
import test_golden as TG

G = T.GOLDEN


def packets_of(path, **kw):
    lt, batches = nsd.pcap_read(path, **kw)
    out = []
    for frames, desc, wl, ts in batches:
        for d in desc:
            d = int(d)
            off, cl = d & 0xFFFFFFFFFF, d >> 40
            assert off % 16 == 0
            out.append(bytes(frames[off:off + cl]))
    return lt, out, batches


def rewrite(pkts, path, magic=0xA1B2C3D4, endian="<", linktype=1, rec_extra=b"", ll=False):
    """Write pkts in a given pcap record format (pcap_io.h:43-116)."""
    with open(path, "wb") as f:
        f.write(struct.pack(endian + "IHHiIII", magic, 2, 4, 0, 0, 65535, linktype))
        for i, p in enumerate(pkts):
            cooked = bytes(range(16)) if ll else b""
            f.write(struct.pack(endian + "IIII", 1000 + i, 7 * i, len(p) + len(cooked), len(p) + 3))
            f.write(rec_extra + cooked + bytes(p))


@pytest.mark.parametrize("name", ["tiny", "edge"])
def test_reader_matches_pcap(name):
    lt, want = T.read_pcap(os.path.join(G, name + ".pcap"))
    got_lt, got, batches = packets_of(os.path.join(G, name + ".pcap"))
    # the replay ends at the first zero-length record (pcap_sg_read /
    # pcap_mm_read return -EINVAL, read_pcap leaves its loop)
    if b"" in want:
        want = want[:want.index(b"")]
        assert name == "edge" and want
    assert got_lt == lt and got == want
    # the frames after the last one are zero (NSD_FRAME_PAD)
    frames, desc = batches[-1][0], batches[-1][1]
    end = int(desc[-1]) & 0xFFFFFFFFFF
    end += int(desc[-1]) >> 40
    assert not frames[end:end + 64].any()


@pytest.mark.parametrize("fmt", ["usec_be", "nsec", "nsec_be", "kuz", "bkm", "bkm_be", "sll", "sll_be"])
def test_reader_record_formats(tmp_path, fmt):
    pkts = [p for p in T.read_pcap(os.path.join(G, "edge.pcap"))[1] if p][:40]
    path = str(tmp_path / "f.pcap")
    spec = {
        "usec_be": dict(endian=">"),
        "nsec": dict(magic=0xA1B23C4D),
        "nsec_be": dict(magic=0xA1B23C4D, endian=">"),
        "kuz": dict(magic=0xA1B2CD34, rec_extra=bytes(8)),
        "bkm": dict(magic=0xA1E2CB12, rec_extra=bytes(8)),
        "bkm_be": dict(magic=0xA1E2CB12, endian=">", rec_extra=bytes(8)),
        "sll": dict(linktype=113, ll=True),
        "sll_be": dict(linktype=113, ll=True, endian=">"),
    }[fmt]
    rewrite(pkts, path, **spec)
    lt, got, batches = packets_of(path)
    want_lt = spec.get("linktype", 1)
    if spec.get("endian") == ">":
        want_lt = int.from_bytes(want_lt.to_bytes(4, "big"), "little")   # passed as stored
    assert lt == want_lt
    assert got == pkts
    wl = np.concatenate([b[2] for b in batches])
    ts = np.concatenate([b[3] for b in batches])
    assert list(wl) == [len(p) + 3 for p in pkts]
    nsec = fmt.startswith("nsec") or fmt.startswith("bkm")
    assert list(ts) == [(1000 + i) * 10**9 + 7 * i * (1 if nsec else 1000) for i in range(len(pkts))]


def test_reader_stops_before_oversized_record(tmp_path):
    """A record longer than a batch carries (65535 < caplen <= 1 MiB) ends the
    batch before it; as the next record it is reported as NSD_ERR_CAPLEN
    (the replay dissects it through the per-packet path), not as the end."""
    _, pkts = T.read_pcap(os.path.join(G, "big.pcap"))
    assert len(pkts[1]) == 70000
    L = nsd.lib()
    h = L.nsd_pcap_open(os.path.join(G, "big.pcap").encode())
    try:
        frames = np.zeros(1 << 20, dtype=np.uint8)
        desc = np.zeros(16, dtype=np.uint64)
        n = L.nsd_pcap_read_batch(h, frames.ctypes.data, frames.nbytes, desc.ctypes.data, 16, None, None)
        assert n == 1
        n = L.nsd_pcap_read_batch(h, frames.ctypes.data, frames.nbytes, desc.ctypes.data, 16, None, None)
        assert n == -3                                  # NSD_ERR_CAPLEN, the record is not consumed
    finally:
        L.nsd_pcap_close(h)


def test_reader_batches_and_end_rules(tmp_path):
    pkts = [p for p in T.read_pcap(os.path.join(G, "edge.pcap"))[1] if p]
    full = str(tmp_path / "full.pcap")
    T.write_pcap(full, pkts)
    # small buffers split the file into several batches, in order
    lt, got, batches = packets_of(full, cap=4096, max_n=7)
    assert got == pkts and len(batches) > 1 and all(len(b[1]) <= 7 for b in batches)
    # a zero-length record ends the replay (pcap_sg_read -EINVAL), as does a
    # truncated last record
    path = str(tmp_path / "z.pcap")
    rewrite(pkts[:5] + [b""] + pkts[5:9], path)
    assert packets_of(path)[1] == pkts[:5]
    data = open(full, "rb").read()
    path2 = str(tmp_path / "t.pcap")
    open(path2, "wb").write(data[:-3])
    assert packets_of(path2)[1] == pkts[:-1]
    # bad magic / version
    bad = str(tmp_path / "b.pcap")
    open(bad, "wb").write(b"\x00" * 24)
    with pytest.raises(nsd.NsdError):
        nsd.pcap_read(bad)


def _fifo_feed(path, data):
    """A named pipe at `path` that a thread fills with `data` (the reader's
    read() path: a non-regular file is not mapped)."""
    import threading
    os.mkfifo(path)

    def feed():
        with open(path, "wb") as f:
            f.write(data)
    t = threading.Thread(target=feed, daemon=True)
    t.start()
    return t


def test_reader_mapped_and_read_paths_agree(tmp_path, monkeypatch):
    """A regular file is mapped, anything else read with read() (or any file
    with NSD_PCAP_MMAP=0): the same records, frame header fields and
    sockaddr_ll from both, including the end rules (a zero-length record, a
    truncated last record) and a named pipe."""
    pkts = [p for p in T.read_pcap(os.path.join(G, "edge.pcap"))[1] if p]
    full = str(tmp_path / "full.pcap")
    T.write_pcap(full, pkts)
    z = str(tmp_path / "z.pcap")
    rewrite(pkts[:5] + [b""] + pkts[5:9], z)
    t = str(tmp_path / "t.pcap")
    open(t, "wb").write(open(full, "rb").read()[:-3])
    files = [full, z, t] + [os.path.join(G, f) for f in sorted(os.listdir(G)) if f.startswith("fh_") and
                            f.endswith(".pcap")]
    for f in files:
        mapped = nsd.pcap_frame_hdrs(f)
        monkeypatch.setenv("NSD_PCAP_MMAP", "0")
        read = nsd.pcap_frame_hdrs(f)
        monkeypatch.delenv("NSD_PCAP_MMAP")
        assert mapped[0] == read[0] and mapped[1] == read[1], f
        assert np.array_equal(mapped[2], read[2]) and np.array_equal(mapped[3], read[3]), f
        assert packets_of(f, cap=4096, max_n=7)[1] == mapped[1]
    fifo = str(tmp_path / "p.pcap")
    th = _fifo_feed(fifo, open(full, "rb").read())
    got = nsd.pcap_frame_hdrs(fifo)
    th.join(10)
    ref = nsd.pcap_frame_hdrs(full)
    assert got[1] == ref[1] and np.array_equal(got[2], ref[2])


def _walk(path):
    """The record walk one header at a time (read_batch's end rule): each
    record's (header offset, caplen)."""
    data = open(path, "rb").read()
    magic = struct.unpack_from("<I", data, 0)[0]
    sw = magic not in (0xA1B2C3D4, 0xA1B23C4D, 0xA1B2CD34, 0xA1E2CB12)
    m = struct.unpack_from(">I" if sw else "<I", data, 0)[0]
    lt = struct.unpack_from(">I" if sw else "<I", data, 20)[0]
    hs, extra = (24, 0) if m in (0xA1B2CD34, 0xA1E2CB12) else ((32, 16) if lt in (113, 253) else (16, 0))
    out, pos = [], 24
    while len(data) - pos >= hs:
        cl = (struct.unpack_from(">I" if sw else "<I", data, pos + 8)[0] - extra) & 0xFFFFFFFF
        if cl == 0 or cl > 1 << 20 or len(data) - pos - hs < cl:
            break
        out.append((pos, cl))
        pos += hs + cl
    return out


def _decoys(n, seed):
    """Frames whose payloads hold runs of pcap-looking record headers (a
    capture of a pcap transfer): guessed walks start inside them."""
    rng = np.random.default_rng(seed)
    pkts = []
    for i in range(n):
        body = b""
        for _ in range(int(rng.integers(0, 40))):
            cl = int(rng.integers(1, 24))
            body += struct.pack("<IIII", i, int(rng.integers(0, 999999)), cl, cl) + rng.bytes(cl)
        pkts.append(rng.bytes(int(rng.integers(0, 20))) + body + rng.bytes(int(rng.integers(0, 64))))
    return [p if p else b"x" for p in pkts]


def test_record_index_is_the_walk(tmp_path):
    """The replay reader's record index (windows cut into chunks walked from
    guessed record starts, spliced onto the exact walk) gives the walk's
    records exactly, for any window and chunk count: record formats, the
    end rules (a zero-length record, a truncated last record, a caplen past
    the 1 MiB buffer), records longer than a window, and payloads full of
    decoy headers."""
    pkts = [p for p in T.read_pcap(os.path.join(G, "edge.pcap"))[1] if p]
    files = []
    f = str(tmp_path / "full.pcap")
    T.write_pcap(f, pkts)
    files.append(f)
    z = str(tmp_path / "z.pcap")
    rewrite(pkts[:5] + [b""] + pkts[5:9], z)
    t = str(tmp_path / "t.pcap")
    open(t, "wb").write(open(f, "rb").read()[:-3])
    files += [z, t]
    for fmt, spec in {"be": dict(endian=">"), "nsec": dict(magic=0xA1B23C4D),
                      "kuz": dict(magic=0xA1B2CD34, rec_extra=bytes(8)),
                      "bkm_be": dict(magic=0xA1E2CB12, endian=">", rec_extra=bytes(8)),
                      "sll": dict(linktype=113, ll=True)}.items():
        g = str(tmp_path / (fmt + ".pcap"))
        rewrite(pkts[:60], g, **spec)
        files.append(g)
    d = str(tmp_path / "decoys.pcap")
    T.write_pcap(d, _decoys(400, 7))
    files.append(d)
    bigf = str(tmp_path / "big.pcap")
    T.write_pcap(bigf, pkts[:3] + [bytes(70000)] + pkts[3:20] + [bytes(1 << 20)] + pkts[20:30])
    files.append(bigf)
    over = str(tmp_path / "over.pcap")
    T.write_pcap(over, pkts[:10] + [bytes((1 << 20) + 1)] + pkts[10:20])
    files.append(over)
    files += [os.path.join(G, n) for n in sorted(os.listdir(G)) if n.endswith(".pcap")]
    for path in files:
        want = _walk(path)
        for window in (1, 7, 100, 999, 4096, 1 << 20, 0):
            for chunks in (1, 2, 3, 5, 17):
                off, cap = nsd.pcap_index(path, window, chunks)
                got = list(zip(off.tolist(), cap.tolist()))
                assert got == want, (path, window, chunks)
    with pytest.raises(nsd.NsdError):
        nsd.pcap_index(str(tmp_path / "missing.pcap"))


MODES = [T.PRINT_NORM, T.PRINT_LESS, T.PRINT_HEX, T.PRINT_ASCII, T.PRINT_HEX_ASCII]


def replayable(name, mode, tmp_path):
    """The committed pcap minus its zero-length records (they end the
    reference's replay).  A chain longer than the device record's layer
    budget (edge.pcap #92) stays: the replay renders its record through the
    per-packet path.  Returns (path, kept indices)."""
    lt, pkts = T.read_pcap(os.path.join(G, name + ".pcap"))
    keep = [i for i in range(len(pkts)) if pkts[i]]
    path = str(tmp_path / (name + ".pcap"))
    T.write_pcap(path, [pkts[i] for i in keep], linktype=lt)
    return path, keep


def frame_lines(path, mode, accepted=None, read=None):
    """show_frame_hdr's line per replayed record (restated, pinned against
    the reference's pcap code in test_frame_hdr.py); with `accepted` (record
    indexes a filter passes) only theirs, counted among themselves.  `read`:
    the file's (linktype, packets) when the batch reader cannot give them (a
    record above NSD_MAX_CAPLEN)."""
    lt, pkts = read if read is not None else nsd.pcap_frame_hdrs(path)[:2]
    fh, sll, _ = T.oracle_pcap_meta(path)
    idx = range(len(fh)) if accepted is None else accepted
    return [T.oracle_frame_hdr(fh[i], sll[i], pkts[i], linktype=lt, mode=mode, count=k + 1)
            for k, i in enumerate(idx)]


@pytest.mark.gpu
@pytest.mark.usefixtures("device_fill")
@pytest.mark.parametrize("mode", MODES)
def test_replay_edge_matches_golden(tmp_path, mode):
    """`--in edge.pcap` end to end on the device: every record's frame header
    line, then the text the reference's parser objects print for it
    (tiny / big / leaves / the record-format fixtures: test_frame_hdr.py,
    whole texts of the reference's read_pcap loop)."""
    gold = TG.load_golden(f"edge.m{mode}.w65535")
    path, keep = replayable("edge", mode, tmp_path)
    cnt = np.zeros(nsd.NCOUNTERS, dtype=np.uint64)
    n, text = nsd.replay_pcap(path, mode=mode, counters=cnt, threads=1, cols=65535)
    assert n == len(keep)
    fl = frame_lines(path, mode)
    assert text == b"".join(fl[k] + gold[i] for k, i in enumerate(keep))
    assert int(cnt[nsd.CNT_PKTS]) == len(keep)


@pytest.mark.gpu
@pytest.mark.usefixtures("device_fill")
def test_replay_read_paths(tmp_path, monkeypatch):
    """The replay's two readers give the same text: the mapped file (record
    index and bodies on the pool, several pool sizes and index windows), the
    read() path (NSD_PCAP_MMAP=0) and a named pipe."""
    path, keep = replayable("edge", T.PRINT_NORM, tmp_path)
    pkts = [p for p in T.read_pcap(path)[1]]
    big = str(tmp_path / "big.pcap")
    T.write_pcap(big, pkts * 600)   # > one 65536-record batch
    decoys = str(tmp_path / "decoys.pcap")
    T.write_pcap(decoys, _decoys(3000, 11))   # guessed index walks start in payloads
    for pth in (decoys, path, big):
        monkeypatch.setenv("NSD_PCAP_MMAP", "0")
        n0, ref = nsd.replay_pcap(pth, mode=T.PRINT_NORM, threads=1)
        monkeypatch.delenv("NSD_PCAP_MMAP")
        assert nsd.replay_pcap(pth, mode=T.PRINT_NORM, threads=1) == (n0, ref)
        for th in (2, 5, 16):
            assert nsd.replay_pcap(pth, mode=T.PRINT_NORM, threads=th) == (n0, ref)
        monkeypatch.setenv("NSD_PCAP_MMAP", "0")
        assert nsd.replay_pcap(pth, mode=T.PRINT_NORM, threads=4) == (n0, ref)
        monkeypatch.delenv("NSD_PCAP_MMAP")
        # record index windows of a few records (many windows, each built on
        # the pool while the one before is scanned, batches cut at windows)
        for w in ("777", "65536"):
            monkeypatch.setenv("NSD_PCAP_IX_WINDOW", w)
            assert nsd.replay_pcap(pth, mode=T.PRINT_NORM, threads=5) == (n0, ref)
        monkeypatch.delenv("NSD_PCAP_IX_WINDOW")
    fifo = str(tmp_path / "p.pcap")
    t = _fifo_feed(fifo, open(big, "rb").read())
    assert nsd.replay_pcap(fifo, mode=T.PRINT_NORM, threads=4) == (n0, ref)
    t.join(10)


@pytest.mark.gpu
@pytest.mark.usefixtures("device_fill")
def test_concurrent_replays(tmp_path):
    """Two replays at once in one process (ctypes drops the GIL): one takes
    the cached staging and device pipe, the other builds its own set; both
    print exactly what a replay alone prints, and the next replay after them
    too."""
    import threading
    path, keep = replayable("edge", T.PRINT_NORM, tmp_path)
    pkts = [p for p in T.read_pcap(path)[1]]
    big = str(tmp_path / "big.pcap")
    T.write_pcap(big, pkts * 900)
    want = {pth: nsd.replay_pcap(pth, mode=T.PRINT_NORM, threads=4) for pth in (path, big)}
    got = {}

    def run(k, pth):
        got[k] = nsd.replay_pcap(pth, mode=T.PRINT_NORM, threads=4)

    for _ in range(3):
        ts = [threading.Thread(target=run, args=(k, pth)) for k, pth in enumerate((big, big, path))]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        assert got[0] == want[big] and got[1] == want[big] and got[2] == want[path]
    assert nsd.replay_pcap(big, mode=T.PRINT_NORM, threads=4) == want[big]


@pytest.mark.gpu
@pytest.mark.usefixtures("device_fill")
@pytest.mark.parametrize("mode", [T.PRINT_NORM, T.PRINT_LESS])
def test_replay_wrapped_and_filtered(tmp_path, mode):
    """80-column tprintf wrap over the replay stream, and a BPF filter in
    front (only the accepted records print, in file order)."""
    _, pkts = T.read_pcap(os.path.join(G, "edge.pcap"))
    path, keep = replayable("edge", mode, tmp_path)
    unwrapped = TG.load_golden(f"edge.m{mode}.w65535")
    n, text = nsd.replay_pcap(path, mode=mode, cols=80)
    fl = frame_lines(path, mode)
    state, want = 0, b""
    for k, i in enumerate(keep):
        w, state = nsd.tprintf_wrap(fl[k] + unwrapped[i], cols=80, state=state)
        want += w
    assert n == len(keep) and text == want
    # bpfc.8 "IPv4 TCP" program: ldh [12]; jeq #0x800 ...; ldb [23]; jeq #6; ret #-1; ret #0
    prog = np.array([(0x28, 0, 0, 12), (0x15, 0, 3, 0x800), (0x30, 0, 0, 23), (0x15, 0, 1, 6),
                     (0x06, 0, 0, 0xFFFFFFFF), (0x06, 0, 0, 0)], dtype=nsd.BPF_INSN)
    bp = nsd.BpfProgram(prog)
    acc = [i for i in keep if len(pkts[i]) >= 24 and pkts[i][12:14] == b"\x08\x00" and pkts[i][23] == 6]
    assert acc
    n, text = nsd.replay_pcap(path, mode=mode, prog=bp)
    # the packet counter counts the records the filter passes (netsniff-ng.c:723-730)
    fl = frame_lines(path, mode, accepted=[keep.index(i) for i in acc])
    assert n == len(acc) and text == b"".join(fl[k] + unwrapped[i] for k, i in enumerate(acc))


@pytest.mark.gpu
@pytest.mark.usefixtures("device_fill")
@pytest.mark.parametrize("key,cfg", [("udp64", T.SYN_UDP64), ("imix", T.SYN_IMIX), ("ipv6x", T.SYN_IPV6X)])
@pytest.mark.parametrize("mode", [T.PRINT_NORM, T.PRINT_LESS])
def test_replay_prefix_digest(tmp_path, key, cfg, mode):
    """64K-packet synthetic pcaps (C2/C3/C4 prefixes) replayed through the
    device with 8 formatting threads: the text's SHA-256 equals the digest of
    the reference's read_pcap loop over the same file (nsref -f: frame
    headers + the parser objects' text; tests/golden/prefix.json)."""
    import hashlib
    import json
    with open(os.path.join(G, "prefix.json")) as f:
        want = json.load(f)[f"{key}:m{mode}"]["replay_text_sha256"]
    path = str(tmp_path / f"{key}.pcap")
    T.synth().nsd_synth_pcap(cfg, T.SEED, 0, 65536, path.encode())
    n, text = nsd.replay_pcap(path, mode=mode, threads=8)
    assert n == 65536
    assert hashlib.sha256(text).hexdigest() == want


def write_ll_pcap(path, pkts, slls, endian="<", magic=0xA1B2C3D4):
    """A LINKTYPE_LINUX_SLL file: each record = pcap_pkthdr + struct pcap_ll
    (pkttype, hatype, len, addr[8], protocol; big-endian fields,
    pcap_io.h:63-69, 171-180 sockaddr_to_ll) + the packet."""
    with open(path, "wb") as f:
        f.write(struct.pack(endian + "IHHiIII", magic, 2, 4, 0, 0, 65535, 113))
        for i, (p, s) in enumerate(zip(pkts, slls)):
            ll = struct.pack(">HHH8s", int(s["pkttype"]), int(s["hatype"]), int(s["halen"]),
                             bytes(s["addr"])) + struct.pack(">H", int(s["protocol"]))
            f.write(struct.pack(endian + "IIII", 1000 + i, i, len(p) + 16, len(p) + 16))
            f.write(ll + bytes(p))


def as_read(slls):
    """The sockaddr_ll read_pcap hands the dissector for those records:
    ll_to_sockaddr fills pkttype / hatype / halen / protocol / addr; family
    and ifindex stay as memset (netsniff-ng.c:672)."""
    r = np.zeros(len(slls), dtype=nsd.SLL_DTYPE)
    for f in ("protocol", "hatype", "pkttype", "halen", "addr"):
        r[f] = slls[f]
    return r


@pytest.mark.parametrize("endian", ["<", ">"])
def test_reader_sll_cooked_headers(tmp_path, endian):
    import test_sll as TS
    cases = TS.sll_cases()
    pkts = [p for p, _ in cases]
    slls = np.array([s for _, s in cases], dtype=nsd.SLL_DTYPE)
    path = str(tmp_path / "ll.pcap")
    write_ll_pcap(path, pkts, slls, endian=endian)
    lt, batches = nsd.pcap_read(path, sll=True, max_n=50)
    assert len(batches) > 1
    got = np.concatenate([b[4] for b in batches]).astype(nsd.SLL_DTYPE)   # concatenate canonicalises byte order
    assert got.tobytes() == as_read(slls).tobytes()
    got_pkts = []
    for b in batches:
        for d in b[1]:
            d = int(d)
            got_pkts.append(bytes(b[0][d & 0xFFFFFFFFFF:(d & 0xFFFFFFFFFF) + (d >> 40)]))
    assert got_pkts == pkts
    # other record forms: zeros (fm.s_ll as memset)
    plain = str(tmp_path / "plain.pcap")
    T.write_pcap(plain, pkts[:9])
    _, b2 = nsd.pcap_read(plain, sll=True)
    assert not b2[0][4].tobytes().strip(b"\0")


@pytest.mark.gpu
@pytest.mark.usefixtures("device_fill")
@pytest.mark.parametrize("mode", [T.PRINT_NORM, T.PRINT_LESS])
def test_replay_sll_file(tmp_path, mode):
    """`--in` an SLL capture: each record's cooked header reaches the SLL
    head as its sockaddr_ll; the text equals the restatement's per packet
    (netlink-continued packets left out: nlmsg is outside the path)."""
    import test_sll as TS
    cases = [c for c in TS.sll_cases() if int(c[1]["hatype"]) != 824]
    pkts = [p for p, _ in cases]
    slls = np.array([s for _, s in cases], dtype=nsd.SLL_DTYPE)
    path = str(tmp_path / "ll.pcap")
    write_ll_pcap(path, pkts, slls)
    frames, desc = T.batch_from_packets(pkts)
    ora = T.oracle_text_packets(frames, desc, linktype=nsd.LINKTYPE_LINUX_SLL, mode=mode, sll=as_read(slls))
    orec, oext, ocnt, _ = T.oracle_records(frames, desc, linktype=nsd.LINKTYPE_LINUX_SLL, mode=mode,
                                           sll=as_read(slls))
    # leaves the restatement does not render as text (ARP / LLDP bodies):
    # the product renderer's text over the oracle's records (pinned against
    # the reference objects in test_golden / test_sll)
    fmt, rc = nsd.format_batch(frames, desc, orec, oext, mode=mode, linktype=nsd.LINKTYPE_LINUX_SLL,
                               sll=as_read(slls))
    assert not any(rc)
    fl = frame_lines(path, mode)
    want = b"".join(fl[i] + (fmt[i] if u else t) for i, (t, u) in enumerate(ora))
    assert sum(u for _, u in ora) < len(ora) // 2
    cnt = np.zeros(nsd.NCOUNTERS, dtype=np.uint64)
    n, text = nsd.replay_pcap(path, mode=mode, counters=cnt)
    assert n == len(pkts)
    assert text == want
    assert np.array_equal(cnt, ocnt)


def _records(data, hdrsize, endian, ll=False):
    """Split a pcap body into raw records (header + bytes; an *_LL record's
    caplen counts its cooked header)."""
    out, pos = [], 24
    base = hdrsize - 16 if ll else hdrsize
    while pos + hdrsize <= len(data):
        cl = struct.unpack_from(endian + "I", data, pos + 8)[0]
        out.append(data[pos:pos + base + cl])
        pos += base + cl
    return out


@pytest.mark.gpu
@pytest.mark.usefixtures("device_fill")
@pytest.mark.parametrize("fmt", ["usec", "usec_be", "nsec", "kuz", "bkm_be", "sll", "sll_be"])
def test_replay_pcap_out(tmp_path, fmt):
    """`--in a.pcap --out b.pcap`: pcap_generic_push_fhdr's header for the
    replayed file (stored magic, 2.4, thiszone / sigfigs 0, snaplen 65535,
    link type swapped once more for swapped magics), then every record that
    passed the filter exactly as read; the text is unchanged by the
    write-out."""
    import test_bpf as TB
    pkts = [p for p in T.read_pcap(os.path.join(G, "edge.pcap"))[1] if p]
    spec = {
        "usec": dict(), "usec_be": dict(endian=">"), "nsec": dict(magic=0xA1B23C4D),
        "kuz": dict(magic=0xA1B2CD34, rec_extra=bytes(8)),
        "bkm_be": dict(magic=0xA1E2CB12, endian=">", rec_extra=bytes(8)),
        "sll": dict(linktype=113, ll=True), "sll_be": dict(linktype=113, ll=True, endian=">"),
    }[fmt]
    src = str(tmp_path / "in.pcap")
    rewrite(pkts, src, **spec)
    data = open(src, "rb").read()
    endian = spec.get("endian", "<")
    hdrsize = 24 if "rec_extra" in spec else 32 if spec.get("ll") else 16
    lt = spec.get("linktype", 1)
    stored_lt = struct.unpack("<I", struct.pack(endian + "I", lt))[0]          # as read natively
    out_lt = stored_lt if endian == "<" else int.from_bytes(stored_lt.to_bytes(4, "little"), "big")
    # (pcap_prepare_header stores swab(as-read) natively: a swapped file gets
    # its link type in host order, a reference quirk kept here)
    want_hdr = data[:16] + struct.pack(endian + "I", 65535) + struct.pack("<I", out_lt)
    if fmt == "sll_be":
        # a swapped SLL file's magic is remapped to swab32(*_MAGIC_LL), which
        # pcap_magic_is_swapped does not know (pcap_io.h:307-320, 895-909): the
        # header is written unswapped, the link type as stored
        want_hdr = data[:4] + struct.pack("<HH", 2, 4) + bytes(8) + struct.pack("<I", 65535) + data[20:24]
    assert data[8:16] == bytes(8)
    recs = _records(data, hdrsize, endian, ll=spec.get("ll", False))
    assert len(recs) == len(pkts)
    dst = str(tmp_path / "out.pcap")
    n, text = nsd.replay_pcap(src, mode=T.PRINT_NORM, pcap_out=dst)
    assert n == len(pkts)
    assert open(dst, "rb").read() == want_hdr + b"".join(recs)
    assert text == nsd.replay_pcap(src, mode=T.PRINT_NORM)[1]
    if fmt in ("usec", "sll"):
        # with the filter: only the accepted records, in file order
        prog = nsd.BpfProgram(TB.P_TCP)
        frames, desc = T.batch_from_packets(pkts)
        keep = TB.oracle_batch(TB.P_TCP, frames, desc) != 0
        assert 0 < keep.sum() < len(pkts)
        n2, _ = nsd.replay_pcap(src, mode=T.PRINT_NORM, prog=prog, pcap_out=dst)
        assert n2 == keep.sum()
        assert open(dst, "rb").read() == want_hdr + b"".join(r for r, k in zip(recs, keep) if k)


def _replay_bounded(**kw):
    """nsd.replay_pcap on a thread joined with a timeout (a hang fails the
    test instead of stalling it): the call's result, or the NsdError it
    raised."""
    import threading
    out = {}

    def run():
        try:
            out["ret"] = nsd.replay_pcap(**kw)
        except nsd.NsdError as e:
            out["err"] = e

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(60)
    assert not t.is_alive(), "the replay did not return"
    return out


def _edge_golden_text(path, keep, mode):
    """The text test_replay_edge_matches_golden expects for replayable("edge")."""
    gold = TG.load_golden(f"edge.m{mode}.w65535")
    fl = frame_lines(path, mode)
    return b"".join(fl[k] + gold[i] for k, i in enumerate(keep))


@pytest.mark.gpu
@pytest.mark.usefixtures("device_fill")
@pytest.mark.parametrize("cols", [0, 80])
def test_replay_text_write_error_then_recovery(tmp_path, cols):
    """The text output fails (out_fd on /dev/full; cols=0 the writev path,
    cols=80 the wrap path): the replay returns a negative status (no hang:
    reader, pool and writer all wind down), and the next replay, which
    rebuilds the cached staging dropped on the error, prints the golden text."""
    path, keep = replayable("edge", T.PRINT_NORM, tmp_path)
    fd = os.open("/dev/full", os.O_WRONLY)
    try:
        out = _replay_bounded(path=path, mode=T.PRINT_NORM, cols=cols, threads=1, out_fd=fd)
    finally:
        os.close(fd)
    assert "err" in out and "ret" not in out
    n, text = nsd.replay_pcap(path, mode=T.PRINT_NORM, threads=1, cols=65535)
    assert n == len(keep) and text == _edge_golden_text(path, keep, T.PRINT_NORM)


@pytest.mark.gpu
@pytest.mark.usefixtures("device_fill")
def test_replay_pcap_out_write_error(tmp_path):
    """The `--out` file cannot be written (/dev/full): NsdError, and the next
    replay is correct."""
    path, keep = replayable("edge", T.PRINT_NORM, tmp_path)
    out = _replay_bounded(path=path, mode=T.PRINT_NORM, threads=1, pcap_out="/dev/full")
    assert "err" in out and "ret" not in out
    n, text = nsd.replay_pcap(path, mode=T.PRINT_NORM, threads=1, cols=65535)
    assert n == len(keep) and text == _edge_golden_text(path, keep, T.PRINT_NORM)


@pytest.mark.gpu
@pytest.mark.usefixtures("device_fill")
def test_replay_big_filtered_pcap_out(tmp_path):
    """Records above NSD_MAX_CAPLEN (big.pcap) with a filter and `--out`: the
    over-long records go one by one through the filter and the per-packet
    path, between the batches; only the accepted records print (counted among
    themselves) and reach the written pcap, bytes as in the source."""
    mode = T.PRINT_NORM
    src = os.path.join(G, "big.pcap")
    _, pkts = T.read_pcap(src)
    # IPv6 only: ethertype 0x86DD (test_pcap_flows' program)
    prog = nsd.BpfProgram(np.array([(0x28, 0, 0, 12), (0x15, 0, 1, 0x86DD), (0x06, 0, 0, 0xFFFF), (0x06, 0, 0, 0)],
                                   dtype=nsd.BPF_INSN))
    acc = [i for i, p in enumerate(pkts) if p[12:14] == b"\x86\xdd"]
    assert acc and len(acc) < len(pkts) and any(len(pkts[i]) > 65535 for i in acc)
    gold = TG.load_golden(f"big.m{mode}.w65535")
    fl = frame_lines(src, mode, accepted=acc, read=(1, pkts))
    # (the restated lines over this file are the reference's: its whole replay text)
    assert b"".join(a + b for a, b in zip(frame_lines(src, mode, read=(1, pkts)), gold)) == \
        b"".join(TG.load_golden(f"big.fh.m{mode}.w65535"))
    dst = str(tmp_path / "out.pcap")
    # (cols as the golden's: the over-long payload lines wrap at 65535 columns)
    n, text = nsd.replay_pcap(src, mode=mode, prog=prog, cols=65535, pcap_out=dst)
    prog.close()
    assert n == len(acc) and text == b"".join(fl[k] + gold[i] for k, i in enumerate(acc))
    data = open(src, "rb").read()
    recs = _records(data, 16, "<")
    assert len(recs) == len(pkts)
    want_hdr = data[:16] + struct.pack("<II", 65535, 1)
    assert open(dst, "rb").read() == want_hdr + b"".join(recs[i] for i in acc)
