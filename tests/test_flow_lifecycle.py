"""The flow table through random sequences of every kind of event - update,
expiry (by index and by time, plain and PAIRED, capped and not), conversations,
export, reset - against a model that runs alongside: the {key: [...]} dicts of
test_flows.model / test_flow_times.model_ts, merged, split and paired in Python
by the models of test_flow_expire / test_flow_times / test_conversations.
After every event the table is exported through a poisoned buffer and compared
with the model, rows and all eight stats, exactly.

Where the header leaves the outcome to the table (which new flows enter a
table that fills, which qualifying flows leave when `max` is below their
number) the model follows the table's choice after checking that it was legal.

One driver serves two tables: the device table, and a stand-in built from the
model that makes a legal choice of its own.  The stand-in runs on any host; it
shows that each seed's sequence reaches every situation the test is for (a
flow dropped as FULL that enters later, a flow that expires and returns, an
expiry cut by `max` and then an update, ...), and it runs the driver's own
checks.  The GPU tests assert the same coverage of the device's run.
"""
import numpy as np
import pytest

import edge_cases as E
import nsd
import nsd_testlib as T
import test_conversations as C
import test_flow_expire as X
import test_flow_times as TS
import test_flows as F
from nsd_testlib import device_fill  # noqa: F401  (fixture: nsd_set_debug_fill(0xA5) around each test)

PAIRED = 1
U64_MAX = (1 << 64) - 1
ST_EXPIRED = 6
NOPS = 40
T0 = 1_700_000_000_000_000_000
SEEDS = [5, 8, 27]           # chosen so that the stand-in reaches every situation at least twice, either way it picks
SIZES = [8, 32]                # max_flows: 16 and 64 slots
MUST_SIZES = (1, 64, 65, 600)  # batch sizes every sequence has: one packet, a wave, a wave and one, above 512
SITUATIONS = ["full_update", "dropped_then_in", "expired_then_back", "partial_expiry", "cut_then_update",
              "paired_hold", "conv_after_rebuilds"]


# ---- traffic ------------------------------------------------------------------------
class Traffic:
    """Packets of a pool of about 3 * slots unidirectional flows (IPv4 / UDP,
    IPv4 / TCP with varying flag bits, IPv6 / UDP; the reverse of a flow is in
    the pool with probability one half), drawn with a skewed popularity: the
    head of the pool is in every batch, most of the tail shows once.  One
    packet in fifty is ARP (never keyed)."""

    def __init__(self, rng, slots):
        self.rng = rng
        pool, j = [], 0
        while len(pool) < 3 * slots:
            kind, a, b, pa, pb = j % 3, 0x0A400000 + j, 0xC0A84000 + j, 1024 + j, (53, 443, 123)[j % 3]
            pool.append((kind, a, b, pa, pb))
            if rng.randint(2):
                pool.append((kind, b, a, pb, pa))
            j += 1
        order = rng.permutation(len(pool))
        self.pool = [pool[i] for i in order]
        w = 1.0 / (1.0 + np.arange(len(pool))) ** 1.5
        self.cum = np.cumsum(w / w.sum())

    def packet(self):
        rng = self.rng
        if rng.randint(50) == 0:
            return E.eth(0x0806) + bytes(28)
        kind, a, b, pa, pb = self.pool[min(int(np.searchsorted(self.cum, rng.rand())), len(self.pool) - 1)]
        pay = bytes(int(rng.randint(0, 30)))
        if kind == 0:
            return E.eth(0x0800) + E.ipv4(17, 8 + len(pay), src=a, dst=b) + E.udp(pa, pb, payload=pay)
        if kind == 1:
            return E.eth(0x0800) + E.ipv4(6, 20 + len(pay), src=a, dst=b) + E.tcp(pa, pb, flags=1 << int(rng.randint(6))) + pay
        pre = bytes.fromhex("20010db80000000000000000")
        return E.eth(0x86DD) + E.ipv6(17, 8 + len(pay), src=pre + E.be32(a), dst=pre + E.be32(b)) + E.udp(pa, pb, payload=pay)


class Batch:
    """n packets counted from `base`, their oracle records, 64-bit timestamps
    that rise with the index but not packet by packet (a jitter of eight
    packets' worth), and what they add to a table: `more` and the stats."""

    def __init__(self, traffic, n, base, timed):
        rng = traffic.rng
        self.n, self.base = n, base
        self.frames, self.desc = T.batch_from_packets([traffic.packet() for _ in range(n)])
        self.rec, self.ext, _, _ = T.oracle_records(self.frames, self.desc)
        self.ts = (np.uint64(T0) + ((np.uint64(base) + np.arange(n, dtype=np.uint64)) << np.uint64(20)) +
                   rng.randint(0, 8 << 20, size=n).astype(np.uint64))
        if timed:
            keys = [next(iter(F.model(self.frames, self.desc[i:i + 1], self.rec[i:i + 1], self.ext)[0]), None)
                    for i in range(n)]
            self.more, self.st = TS.model_ts(self.frames, self.desc, self.rec, self.ext, self.ts, keys, base=base)
        else:
            self.more, self.st = F.model(self.frames, self.desc, self.rec, self.ext, base=base)


# ---- the two tables -------------------------------------------------------------------
class Device:
    """The device table behind the driver's calls; every output goes through a
    poisoned buffer (the *_checked helpers of the feature tests)."""

    def __init__(self, max_flows, timed):
        self.t = nsd.FlowTable(max_flows, timed=timed)
        self.timed, self.slots, self.keep = timed, self.t.slots, None

    def update(self, b):
        f, d = F.to_dev(b.frames, b.desc)
        rec, ext, _, _ = nsd.dissect_device(f, d, mode=T.PRINT_NORM)
        ts = TS.ts_dev(b.ts) if self.timed else None
        self.t.update(f, d, rec, ext, base=b.base, ts=ts)
        self.keep = (f, d, rec, ext, ts)                 # (alive until snapshot() has synchronised)

    def rows(self, flows):
        return TS.rows_of(flows) if flows.dtype == nsd.FLOWT_DTYPE else X.rows_list(flows)

    def snapshot(self):
        flows, stats, count = (TS if self.timed else F).export_checked(self.t, self.slots)
        assert count == len(flows)
        return self.rows(flows), [int(x) for x in stats]

    def export(self, form):
        if form == "device":
            return self.snapshot()
        flows, stats = self.t.export_ts() if form == "host_ts" else self.t.export()
        return self.rows(flows), [int(x) for x in stats]

    def expire(self, before, flags, cap, by_time, host):
        """([[key, values]] removed, sorted by first; [removed, qualified])"""
        if host:
            flows, q, _ = self.t.expire_ts(before, flags, max_flows=cap) if by_time else self.t.expire(before, flags, max_flows=cap)
            return self.rows(flows), [len(flows), q]
        if self.timed:
            flows, c = TS.expire_checked(self.t, before, flags, cap, by_time=by_time)
        else:
            flows, c = X.expire_checked(self.t, before, flags, cap)
        return self.rows(flows), c

    def conversations(self, by, k, form, total):
        """The rows in the model's form; the device forms' in the model's order
        (theirs is unspecified), the host forms' as they came."""
        ts = form.endswith("_ts")
        if form.startswith("host"):
            conv, _ = (self.t.conversations_ts if ts else self.t.conversations)(by, k)
            return TS.conv_rows_of(conv) if ts else C.conv_rows_of(conv)
        if not ts:
            return C.ordered(C.conv_rows_of(C.conv_checked(self.t, by, k, total)), by)
        import torch
        B, rows = nsd.CONVT_BYTES, min(k, total)
        buf = torch.full(((rows + 1) * B,), T.FILL, dtype=torch.uint8, device="cuda")
        count = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        ws = torch.full((nsd.lib().nsd_flow_conv_workspace_bytes(self.t.h),), T.FILL, dtype=torch.uint8, device="cuda")
        self.t.conversations_device_ts(by, k, conv=buf, count=count, workspace=ws)
        torch.cuda.synchronize()
        assert [int(x) for x in count.cpu()] == [rows, total], (by, k)
        host = buf.cpu().numpy()
        assert (host[rows * B:] == T.FILL).all(), "bytes past the last row were written"
        assert not (host[:rows * B].reshape(rows, B) == T.FILL).all(axis=1).any()
        return C.ordered(TS.conv_rows_of(host[:rows * B].view(nsd.CONVT_DTYPE)), by)

    def reset(self):
        self.t.reset()

    def close(self):
        self.t.close()


class StandIn:
    """A table made of the models, for hosts without a GPU: it takes the new
    flows of an update in the order of their `first` (pick = 0) or against it
    (pick = -1) while it has slots, and on a capped expiry the qualifying flows
    from the same end.  Any such choice is legal."""

    def __init__(self, max_flows, timed, pick=0):
        self.timed, self.pick = timed, pick
        self.slots = 1 << (2 * max_flows - 1).bit_length()
        self.reset()

    def reset(self):
        self.m, self.st = {}, [0] * 8

    def update(self, b):
        known = {k: v for k, v in b.more.items() if k in self.m}
        new = TS.by_first({k: v for k, v in b.more.items() if k not in self.m})
        if self.pick:
            new.reverse()
        room = self.slots - len(self.m)
        self.m = (TS.merge_ts if self.timed else X.merge)(self.m, {**known, **{k: v for k, v in new[:room]}})
        for j in range(4):
            self.st[j] += b.st[j]
        self.st[F.ST_FULL] += sum(v[1] for _, v in new[room:])
        self.st[F.ST_FLOWS] = len(self.m)

    def snapshot(self):
        return TS.by_first(self.m), list(self.st)

    def export(self, form):
        rows, st = self.snapshot()
        return ([[k, v[:5]] for k, v in rows] if form == "host" else rows), st

    def expire(self, before, flags, cap, by_time, host):
        gone, _ = TS.expire_model(self.m, before, flags, by_time)
        rows = TS.by_first(gone)
        took = (rows[max(0, len(rows) - cap):] if self.pick else rows[:cap]) if cap else []
        for k, _ in took:
            del self.m[k]
        self.st[F.ST_FLOWS] = len(self.m)
        self.st[ST_EXPIRED] += len(took)
        return ([[k, v if by_time else v[:5]] for k, v in took]), [len(took), len(gone)]

    def conversations(self, by, k, form, total):
        if form.endswith("_ts"):
            return C.ordered(TS.conv_model_ts(self.m), by)[:k]
        return C.ordered(C.conv_model({key: v[:5] for key, v in self.m.items()}), by)[:k]

    def close(self):
        pass


# ---- the driver -----------------------------------------------------------------------
def schedule(rng):
    """NOPS op kinds and the sizes of the updates among them: the first op is
    an update, MUST_SIZES come first among the sizes (shuffled), the others are
    1..700."""
    kinds = ["update"] + list(rng.choice(["update", "expire", "conv", "export", "reset"], size=NOPS - 1,
                                         p=[0.38, 0.32, 0.18, 0.09, 0.03]))
    sizes = [int(x) for x in rng.permutation(MUST_SIZES)] + [int(rng.randint(1, 701)) for _ in range(NOPS)]
    return kinds, sizes


def run_sequence(table, seed, max_flows, timed):
    """Drives `table` through the seed's sequence; after every op the table's
    export is the model.  Returns how often each situation was reached and the
    update sizes used.  The random numbers drawn do not depend on what the
    table chose, so every table sees the same ops; an expiry's `before`, flags
    and `max` lean towards a situation that has not been reached yet when the
    model's state offers it."""
    rng = np.random.RandomState(1000 * seed + max_flows)
    traffic = Traffic(rng, table.slots)
    kinds, sizes = schedule(rng)
    merge = TS.merge_ts if timed else X.merge
    m, st = {}, [0] * 8                          # the model: the flows in the table, its stats
    hit = dict.fromkeys(SITUATIONS, 0)
    dropped, expired_first = set(), {}           # keys once dropped as FULL; key -> `first` when it expired
    cut_pending, rebuilds, base, used = False, 0, 0, []

    def check(what):
        rows, got_st = table.snapshot()
        assert len({k for k, _ in rows}) == len(rows), f"{what}: a key twice in the table"
        assert rows == TS.by_first(m), what
        assert got_st == st, f"{what}: stats {got_st}, model {st}"

    for op, kind in enumerate(kinds):
        what = f"seed {seed} max_flows {max_flows} op {op} {kind}"
        if kind == "update":
            n = sizes[len(used)]
            used.append(n)
            b = Batch(traffic, n, base, timed)
            base += n + int(rng.randint(0, 3))
            table.update(b)
            rows, got_st = table.snapshot()
            got = {k: v for k, v in rows}
            assert len(got) == len(rows), f"{what}: a key twice in the table"
            known = {k: v for k, v in b.more.items() if k in m}
            new_in = {k: v for k, v in b.more.items() if k not in m and k in got}
            absent = {k: v for k, v in b.more.items() if k not in m and k not in got}
            for k, v in new_in.items():          # in with all its packets of this batch
                assert got[k] == v, f"{what}: a new flow is in the table with other counters than the batch's"
            if absent:                           # allowed only when no slot is left
                assert len(got) == table.slots, f"{what}: flows dropped as FULL from a table with free slots"
                hit["full_update"] += 1
            hit["dropped_then_in"] += sum(1 for k in new_in if k in dropped)
            hit["expired_then_back"] += sum(1 for k, v in new_in.items() if k in expired_first and v[3] > expired_first[k])
            dropped = (dropped | set(absent)) - set(new_in)
            for k in new_in:
                expired_first.pop(k, None)
            if cut_pending:
                hit["cut_then_update"] += 1
                cut_pending = False
            m = merge(m, {**known, **new_in})
            for j in range(4):
                st[j] += b.st[j]
            st[F.ST_FULL] += sum(v[1] for v in absent.values())
            st[F.ST_FLOWS] = len(m)
            assert rows == TS.by_first(m), what
            assert got_st == st, f"{what}: stats {got_st}, model {st}"
        elif kind == "expire":
            by_time = timed and bool(rng.randint(2))
            flags = PAIRED if rng.randint(2) else 0
            host = bool(rng.randint(3) == 0)
            lasts = sorted(v[6 if by_time else 4] for v in m.values())
            q = rng.choice([0.3, 0.5, 0.8, 2.0, -1.0], p=[0.3, 0.3, 0.25, 0.1, 0.05])
            bump, u = int(rng.randint(2)), rng.rand()        # (drawn whatever the table holds)
            cap_kind = rng.choice(["zero", "below", "enough"], p=[0.12, 0.38, 0.5])
            before = 0 if q < 0 else U64_MAX if q > 1 or not lasts else lasts[int(q * len(lasts))] + bump
            if not hit["paired_hold"]:
                # not reached yet: the first `before` among the model's lasts at which a reverse holds a flow back
                held = [x + 1 for x in lasts if len(TS.expire_model(m, x + 1, PAIRED, by_time)[0]) <
                        len(TS.expire_model(m, x + 1, 0, by_time)[0])]
                if held:
                    before, flags = held[int(u * len(held))], PAIRED
                    cap_kind = "enough" if cap_kind == "zero" else cap_kind
            gone, stay = TS.expire_model(m, before, flags, by_time)
            plain_gone, _ = TS.expire_model(m, before, 0, by_time)
            if not hit["cut_then_update"] and not cut_pending and len(gone) >= 2 and cap_kind == "enough":
                cap_kind = "below"                           # not reached yet either
            cap = 0 if cap_kind == "zero" else table.slots if cap_kind == "enough" or len(gone) < 2 else \
                [1, len(gone) // 2, len(gone) - 1][int(u * 3)]
            rows, c = table.expire(before, flags, cap, by_time, host)
            width = 7 if by_time else 5
            took = {k: v for k, v in rows}
            assert c == [min(cap, len(gone)), len(gone)] and len(took) == len(rows) == c[0], what
            assert [v[3] for _, v in rows] == sorted(v[3] for _, v in rows), what
            for k, v in took.items():            # a subset of the qualifying flows, each as the model has it
                assert k in gone and gone[k][:width] == v, what
            if cap >= len(gone):
                assert set(took) == set(gone), what
            if flags and cap and len(gone) < len(plain_gone):
                hit["paired_hold"] += 1
            if took and len(took) < len(m):
                hit["partial_expiry"] += 1
            if 0 < cap < len(gone):
                cut_pending = True
            rebuilds += bool(took)
            for k, v in took.items():
                expired_first[k] = v[3]
            m = {k: v for k, v in m.items() if k not in took}
            st[F.ST_FLOWS] = len(m)
            st[ST_EXPIRED] += len(took)
            check(what)
        elif kind == "conv":
            by = int(rng.randint(3))
            form = ["device", "host"][int(rng.randint(2))] + ("_ts" if timed and rng.randint(3) else "")
            want = C.ordered(TS.conv_model_ts(m) if form.endswith("_ts") else C.conv_model({k: v[:5] for k, v in m.items()}), by)
            total = len(want)
            k = int(rng.choice([0, 1, (total + 1) // 2, total, total + 3]))
            got = table.conversations(by, k, form, total)
            assert got == want[:k], f"{what} by={by} k={k} {form}"
            if rebuilds >= 2 and total:
                hit["conv_after_rebuilds"] += 1
            check(what)                          # the table was only read
        elif kind == "export":
            form = ["device", "host", "host_ts"][int(rng.randint(3 if timed else 2))]
            rows, got_st = table.export(form)
            want = TS.by_first(m)
            assert rows == ([[k, v[:5]] for k, v in want] if form == "host" else want) and got_st == st, f"{what} {form}"
            check(what)
        else:
            table.reset()
            m, st = {}, [0] * 8
            dropped, expired_first, cut_pending, rebuilds = set(), {}, False, 0
            check(what)
    return hit, used


def assert_coverage(hit, used, floor=1):
    assert all(hit[s] >= floor for s in SITUATIONS), f"situations not reached: {hit}"
    assert set(MUST_SIZES) <= set(used) and max(used) > 512, used


# ---- CPU: the sequences reach every situation, whatever the table chooses -------------
@pytest.mark.parametrize("max_flows", SIZES)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("timed", [False, True], ids=["plain", "timed"])
def test_sequences_reach_every_situation(timed, seed, max_flows):
    """With a stand-in table that takes new / expiring flows from either end
    of their order, every situation is reached at least twice: the device's
    own legal choices have room to differ."""
    for pick in (0, -1):
        table = StandIn(max_flows, timed, pick)
        assert table.slots == 2 * max_flows
        hit, used = run_sequence(table, seed, max_flows, timed)
        assert_coverage(hit, used, floor=2)


def test_driver_refuses_an_illegal_choice():
    """The driver's checks are no formality: a stand-in that loses a packet of
    a new flow, drops a flow while slots are free, or removes a flow that does
    not qualify, fails."""
    class LosesAPacket(StandIn):
        def update(self, b):
            super().update(b)
            k = next(iter(self.m))
            self.m[k] = [self.m[k][0], self.m[k][1] + 1] + self.m[k][2:]

    class DropsEarly(StandIn):
        def update(self, b):
            self.slots -= 1
            super().update(b)
            self.slots += 1

    class TakesTheWrongFlow(StandIn):
        def expire(self, before, flags, cap, by_time, host):
            rows, c = super().expire(before, flags, cap, by_time, host)
            if self.m and c[1] < len(self.m) + c[0]:
                k = next(iter(self.m))
                rows = TS.by_first({**dict((key, v) for key, v in rows), k: self.m.pop(k)[:5]})
                c = [c[0] + 1, c[1] + 1]
            return rows, c

    for bad, why in ((LosesAPacket, "other counters than the batch's"), (DropsEarly, "a table with free slots"),
                     (TakesTheWrongFlow, "expire")):
        with pytest.raises(AssertionError, match=why):
            run_sequence(bad(8, False), SEEDS[0], 8, False)


# ---- GPU ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("max_flows", SIZES)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("timed", [False, True], ids=["plain", "timed"])
def test_random_life_cycle(device_fill, timed, seed, max_flows):
    table = Device(max_flows, timed)
    assert table.slots == 2 * max_flows
    try:
        hit, used = run_sequence(table, seed, max_flows, timed)
    finally:
        table.close()
    assert_coverage(hit, used)


@pytest.mark.gpu
def test_captured_chain_replays(device_fill):
    """reset + walk + update + expire + update + conversations + export
    captured once on one stream (a linear chain) and replayed over three input
    contents, with every output and workspace poisoned before each replay.
    The second update feeds the same records again, counted from n: the flows
    the expiry removed return as new ones, the survivors accumulate."""
    import torch
    n, cut = 1500, 1480
    batches = [C.talk(n, 21, seed=1), C.talk(n, 33, seed=2), C.talk(n, 27, seed=3)]
    size = max(len(f) for f, _ in batches)
    frames = torch.zeros(size, dtype=torch.uint8, device="cuda")
    desc = torch.zeros(n, dtype=torch.int64, device="cuda")
    rec = torch.empty(n * nsd.REC_BYTES, dtype=torch.uint8, device="cuda")
    ext = torch.empty(nsd.ext_pool_words(n), dtype=torch.int32, device="cuda")
    used = torch.zeros(1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(nsd.NCOUNTERS, dtype=torch.int64, device="cuda")
    ws = torch.empty(nsd.lib().nsd_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    t = nsd.FlowTable(128)
    L = nsd.lib()
    gone_buf = torch.empty(129 * nsd.FLOW_BYTES, dtype=torch.uint8, device="cuda")
    gone_count = torch.zeros(2, dtype=torch.int32, device="cuda")
    ews = torch.empty(L.nsd_flow_expire_workspace_bytes(t.h), dtype=torch.uint8, device="cuda")
    conv_buf = torch.empty((t.slots + 1) * nsd.CONV_BYTES, dtype=torch.uint8, device="cuda")
    conv_count = torch.zeros(2, dtype=torch.int32, device="cuda")
    cws = torch.empty(L.nsd_flow_conv_workspace_bytes(t.h), dtype=torch.uint8, device="cuda")
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
        t.update(frames, desc, rec, ext, base=n)
        t.conversations_device(nsd.CONV_BY_BYTES, C.ALL, conv=conv_buf, count=conv_count, workspace=cws)
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
    for j in (1, 2, 0):
        load(j)
        for x in (rec, ext, ws, out, gone_buf, gone_count, ews, conv_buf, conv_count, cws):
            x.view(torch.uint8).fill_(T.FILL)
        g.replay()
        torch.cuda.synchronize()
        f, d = batches[j]
        orec, oext, _, _ = T.oracle_records(f, d)
        m, st = F.model(f, d, orec, oext)
        gone, stay = X.expire_model(m, cut, PAIRED)
        assert 3 < len(gone) < len(X.expire_model(m, cut, 0)[0]) and stay
        again = F.model(f, d, orec, oext, base=n)[0]
        want = X.merge(stay, again)
        assert all(want[k] == again[k] for k in gone) and all(want[k][1] == 2 * m[k][1] for k in stay)
        assert [int(x) for x in gone_count.cpu()] == [len(gone), len(gone)], f"replay {j}"
        host = gone_buf.cpu().numpy()
        assert (host[len(gone) * nsd.FLOW_BYTES:] == T.FILL).all()
        rows = host[:len(gone) * nsd.FLOW_BYTES].view(nsd.FLOW_DTYPE)
        assert X.rows_list(rows[np.argsort(rows["first"])]) == X.by_first(gone), f"replay {j}"
        convs = C.ordered(C.conv_model(want), nsd.CONV_BY_BYTES)
        assert [int(x) for x in conv_count.cpu()] == [len(convs), len(convs)], f"replay {j}"
        host = conv_buf.cpu().numpy()
        assert (host[len(convs) * nsd.CONV_BYTES:] == T.FILL).all()
        got = C.conv_rows_of(host[:len(convs) * nsd.CONV_BYTES].view(nsd.CONV_DTYPE))
        assert C.ordered(got, nsd.CONV_BY_BYTES) == convs, f"replay {j}"
        c = int(count.cpu()[0])
        host = out.cpu().numpy()
        assert c == len(want) and (host[c * nsd.FLOW_BYTES:] == T.FILL).all()
        rows = host[:c * nsd.FLOW_BYTES].view(nsd.FLOW_DTYPE)
        assert X.rows_list(rows[np.argsort(rows["first"])]) == X.by_first(want), f"replay {j}"
        got = [int(x) for x in stats.cpu().numpy().view(np.uint64)]
        assert got == [2 * x for x in st[:5]] + [len(want), len(gone), 0], f"replay {j}"
    t.close()
