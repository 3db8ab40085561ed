"""The split schedule's fast kernel with a shared tail (fast_tiles: a static
front, the last rounds' tiles handed out at run time from per-stream heads):
device records against the CPU oracle, both record forms, NORM and LESS, at
small grids so that a small batch has many rounds and a real tail.  Every
case forces the split schedule (its own fixture instead of `schedule_small`,
whose other parameters run the fused kernel) and checks with
nsd_last_tail_shared that the launch it compares drew tickets, so a library
that fell back to static tiles fails here.  The share threshold is crossed at
grid caps 1 and 3; the cap of 8 is covered by the plain batches."""
import ctypes

import numpy as np
import pytest

import edge_cases
import nsd
import nsd_testlib as T
import test_device_parity as P
from nsd_testlib import device_fill  # noqa: F401  (fixture: nsd_set_debug_fill(0xA5) around each test)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("device_fill")]

MODES = [T.PRINT_NORM, T.PRINT_LESS]
WAVES = 4


@pytest.fixture(autouse=True)
def split_schedule():
    prev = nsd.set_schedule(nsd.SCHED_SPLIT)
    yield
    nsd.set_schedule(prev)
    nsd.set_grid_cap(0)


def _tail_rounds(n, grid):
    """The rounds the launcher shares for n packets at this grid cap (0: static)."""
    L = nsd.lib()
    L.nsd_launch_workspace_layout.restype = ctypes.c_int
    L.nsd_launch_workspace_layout.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_uint64)]
    out = (ctypes.c_uint64 * 20)()
    assert L.nsd_launch_workspace_layout(n, grid, 1, out) == 0
    return int(out[18])


def _shared():
    """Whether the last launch's fast kernel shared its tail."""
    L = nsd.lib()
    L.nsd_last_tail_shared.restype = ctypes.c_int
    return bool(L.nsd_last_tail_shared())


_ORACLE = {}


def _oracle(key, frames, desc, mode):
    """The oracle's records, pool and counters of a batch, computed once."""
    k = (key, mode)
    if k not in _ORACLE:
        orec, oext, ocnt, _ = T.oracle_records(frames, desc, mode=mode)
        for a in (orec, oext, ocnt):
            a.setflags(write=False)
        _ORACLE[k] = (orec, oext, ocnt)
    return _ORACLE[k]


def _upload(frames, desc):
    import torch
    return torch.from_numpy(frames.copy()).cuda(), torch.from_numpy(desc.view(np.int64).copy()).cuda()


def _same_full(out, ora):
    rec, ext, used, cnt = out
    orec, oext, ocnt = ora
    drec = rec.cpu().numpy().view(nsd.REC_DTYPE)
    dext = ext.cpu().numpy().view(np.uint32)[:int(used.item())]
    P.assert_same_records(drec, orec, dext, oext)
    c = cnt.cpu().numpy().view(np.uint64)
    assert c[nsd.CNT_LISTOVF] == 0
    assert np.array_equal(c, ocnt), f"counters differ: {nsd.unpack_counters(c)} vs {nsd.unpack_counters(ocnt)}"


def _same_compact(out, ora):
    """test_device_parity._compare_compact against an oracle computed before."""
    crec, ext, used, cnt = out
    orec, oext, ocnt = ora
    n = len(orec)
    got = crec.cpu().numpy().view(nsd.CREC_DTYPE)[:n]
    dpool = ext.cpu().numpy().view(np.uint32)[:n + int(used.item())]
    want, wpool = nsd.compact_of(orec, oext)
    for fld in ("ip_csum", "nflags", "nlayers"):
        bad = np.nonzero(got[fld] != want[fld])[0]
        assert len(bad) == 0, f"{fld} differs at {bad[:10]}"
    deep = ((want["nflags"] & 7) == 7) & (want["nlayers"] == 0)
    assert np.array_equal(got["chain"][~deep], want["chain"][~deep]), "chain ids differ"
    leaf = (want["nflags"] & nsd.F_LEAF_END) != 0
    side = (want["nlayers"] != 0) | (leaf & ~deep)
    assert np.array_equal(dpool[:n][side], wpool[:n][side]), "side words differ"
    for i in np.nonzero(deep)[0]:
        if want[i]["chain"] == 0xFFFFFFFF:
            assert got[i]["chain"] == 0xFFFFFFFF
            continue
        gp, gids, goffs = nsd.ext_entry(dpool, int(got[i]["chain"]))
        _, oids, _ = nsd.ext_entry(wpool, int(want[i]["chain"]))
        assert gp == i and gids == oids and not any(goffs), f"ext chain differs at {i}"
    c = cnt.cpu().numpy().view(np.uint64)
    assert c[nsd.CNT_LISTOVF] == 0
    assert np.array_equal(c, ocnt), f"counters differ: {nsd.unpack_counters(c)} vs {nsd.unpack_counters(ocnt)}"


def _check_both(key, frames, desc, mode, grid):
    import torch
    ora = _oracle(key, frames, desc, mode)
    f, d = _upload(frames, desc)
    nsd.set_grid_cap(grid)
    want = _tail_rounds(len(desc), grid) > 0
    full = nsd.dissect_device(f, d, mode=mode)
    assert _shared() == want
    comp = nsd.dissect_device_compact(f, d, mode=mode)
    assert _shared() == want
    torch.cuda.synchronize()
    assert nsd.last_schedule() == "split"
    _same_full(full, ora)
    _same_compact(comp, ora)


_UDP = {}


def _udp(n, seed=T.SEED):
    if (n, seed) not in _UDP:
        frames, desc = T.make_batch(T.SYN_UDP64, n, seed=seed)
        frames.setflags(write=False)
        desc.setflags(write=False)
        _UDP[(n, seed)] = (frames, desc)
    return _UDP[(n, seed)]


@pytest.mark.parametrize("grid", [1, 3, 8])
@pytest.mark.parametrize("n", [64 * 2048, 64 * 2048 + 17])
@pytest.mark.parametrize("mode", MODES)
def test_plain_batches_at_small_grids(mode, n, grid):
    """2,048 tiles over 4, 12 and 32 waves (512, 171 and 64 rounds, the last
    half of them shared), and the same with a partial last tile, which lies
    in the shared tail."""
    assert _tail_rounds(n, grid) > 0
    frames, desc = _udp(n)
    _check_both(("udp", n), frames, desc, mode, grid)


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("share", [15, 16, 17])
@pytest.mark.parametrize("mode", MODES)
def test_share_threshold(mode, share, grid):
    """A wave's share of 15 tiles runs the static loop, 16 and 17 share their
    tail; each with whole tiles and with a partial last one."""
    for extra in (0, 17):
        n = 64 * WAVES * grid * (share - (1 if extra else 0)) + extra
        assert (_tail_rounds(n, grid) > 0) == (share >= 16)
        frames, desc = _udp(n)
        _check_both(("udp", n), frames, desc, mode, grid)


_FULL = {}


def _full_lists(kind, n):
    """n packets that each add a list entry: long IPv6 extension chains (as
    test_device_parity._split_tail_batch's: every one deferred from the
    front), or ICMPv4 messages that run past the 64-byte window (every one
    leaves a remainder at the back), good and bad sums."""
    if (kind, n) not in _FULL:
        E = edge_cases
        if kind == "chains":
            base = P._long_chains(512, seed=23)
        else:
            base = []
            for k in range(256):
                body = bytes((7 * k + 3 * j) & 255 for j in range(40 + (k * 13) % 300))
                msg = E.icmp(payload=body, good=k % 3 != 0)
                base.append(E.eth(0x0800) + E.ipv4(1, len(msg)) + msg)
        pkts = (base * (n // len(base) + 1))[:n]
        frames, desc = T.batch_from_packets(pkts, align=2)
        _FULL[(kind, n)] = (frames, desc)
    return _FULL[(kind, n)]


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("kind", ["chains", "icmp"])
@pytest.mark.parametrize("mode", MODES)
def test_full_lists(mode, kind, grid):
    """Every packet adds an entry to its wave's list, so the lists fill as
    fast as they can: a wave that runs ahead stops asking once its list has
    no room for the tiles it holds and one more (the room rule), and no list
    is overrun (NSD_CNT_LISTOVF stays 0, counters equal the oracle's)."""
    n = 64 * WAVES * 3 * 20 + 17      # 20 rounds at 12 waves, 60 at 4
    assert _tail_rounds(n, grid) > 0
    frames, desc = _full_lists(kind, n)
    orec, _, ocnt = _oracle((kind, n), frames, desc, mode)
    if kind == "chains":
        assert (orec["data_off"] > 64).all()
    elif mode == T.PRINT_NORM:
        assert ocnt[nsd.CNT_ICMP_BAD] > n // 4
    _check_both((kind, n), frames, desc, mode, grid)


def test_counter_reset_between_launches():
    """Three launches on one stream with different sizes and grids, the debug
    fill on: each finds the heads and the blocks' count zeroed by the one
    before (a head left over would skip tiles: records would keep the fill)."""
    import torch
    runs = [(64 * 2048 + 17, 8), (64 * WAVES * 3 * 17, 3), (64 * 2048, 1), (64 * 1024 + 5, 3)]
    outs = []
    for n, grid in runs:
        assert _tail_rounds(n, grid) > 0
        frames, desc = _udp(n)
        f, d = _upload(frames, desc)
        nsd.set_grid_cap(grid)
        outs.append((nsd.dissect_device_compact(f, d, mode=T.PRINT_NORM), f, d))
        assert _shared()
    torch.cuda.synchronize()
    for (n, grid), (out, _, _) in zip(runs, outs):
        frames, desc = _udp(n)
        _same_compact(out, _oracle(("udp", n), frames, desc, T.PRINT_NORM))


def test_streams_have_their_own_heads():
    """Two streams, each with its own workspace and batch, launched in turn
    without a wait between them; one synchronise at the end."""
    import torch
    dev = torch.device("cuda", 0)
    nsd.set_grid_cap(8)
    jobs = []
    for k, n in enumerate((64 * 2048 + 17, 64 * 1536)):
        assert _tail_rounds(n, 8) > 0
        frames, desc = _udp(n, seed=T.SEED + 1 + k)
        f, d = _upload(frames, desc)
        ws = torch.empty(nsd.lib().nsd_workspace_bytes(n), dtype=torch.uint8, device=dev)
        jobs.append((torch.cuda.Stream(), n, T.SEED + 1 + k, f, d, ws, []))
    torch.cuda.synchronize()
    for _ in range(3):
        for s, n, seed, f, d, ws, outs in jobs:
            with torch.cuda.stream(s):
                outs.append(nsd.dissect_device_compact(f, d, mode=T.PRINT_NORM, workspace=ws))
                assert _shared()
    torch.cuda.synchronize()
    for s, n, seed, f, d, ws, outs in jobs:
        frames, desc = _udp(n, seed=seed)
        ora = _oracle(("udp", n, seed), frames, desc, T.PRINT_NORM)
        for out in outs:
            _same_compact(out, ora)


@pytest.mark.parametrize("compact", [False, True])
def test_graph_replay_between_shared_launches(compact):
    """One captured launch (static tiles: a graph replays fixed arguments)
    replayed three times over changed frames, with launches that share their
    tail on the same stream before and after it."""
    import torch
    n = 64 * 512
    nsd.set_grid_cap(3)
    assert _tail_rounds(n, 3) > 0
    dev = torch.device("cuda", 0)
    batches = [_udp(n, seed=T.SEED + 10 + k) for k in range(3)]
    cap = max(len(f) for f, _ in batches)
    frames = torch.zeros(cap, dtype=torch.uint8, device=dev)
    desc = torch.zeros(n, dtype=torch.int64, device=dev)
    rb = nsd.CREC_BYTES if compact else nsd.REC_BYTES
    rec = torch.empty(n * rb, dtype=torch.uint8, device=dev)
    ext = torch.empty(nsd.ext_pool_words(n), dtype=torch.int32, device=dev)
    used = torch.zeros(1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(nsd.NCOUNTERS, dtype=torch.int64, device=dev)
    ws = torch.empty(nsd.lib().nsd_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def walk():
        used.zero_()
        cnt.zero_()
        if compact:
            nsd.dissect_device_compact(frames, desc, mode=T.PRINT_NORM, crec=rec, ext=ext, ext_used=used,
                                       counters=cnt, workspace=ws)
        else:
            nsd.dissect_device(frames, desc, mode=T.PRINT_NORM, rec=rec, ext=ext, ext_used=used, counters=cnt,
                               workspace=ws)

    def load(k):
        f, d = batches[k]
        frames.zero_()
        frames[:len(f)].copy_(torch.from_numpy(f.copy()))
        desc.copy_(torch.from_numpy(d.view(np.int64).copy()))

    def check(k):
        f, d = batches[k]
        ora = _oracle(("udp", n, T.SEED + 10 + k), f, d, T.PRINT_NORM)
        (_same_compact if compact else _same_full)((rec, ext, used, cnt), ora)

    load(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        walk()   # outside the capture: a launch with a shared tail on this stream
        assert _shared()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    check(0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        walk()
        assert not _shared()
    for k in range(3):
        load(k)
        for t in (rec, ext, ws):
            t.view(torch.uint8).fill_(T.FILL)
        g.replay()
        torch.cuda.synchronize()
        check(k)
    load(1)
    walk()   # and one with a shared tail again
    assert _shared()
    torch.cuda.synchronize()
    check(1)
