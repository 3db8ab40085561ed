"""flowbench.py - timing of the flow table's update (update + commit kernels)
beside the batch walk that feeds it.  Not the benchmark (bench.py is).

  python tools/flowbench.py [--packets N] [--steps K] [--warmup W] [--out DIR]

Four GPU steps, one child process per workload, each under its own time
limit; the first that fails ends the run (nothing more is started on the
GPU after a fault or a timeout):

  udp64   C2: 16,777,216 x 64 B Eth/IPv4/UDP, source address 10.0.0.0 | i
  imix    C3: IMIX Eth/[VLAN]/IPv4/{TCP,UDP,ICMP}
  ipv6x   C4: IPv6 + 0..6 extension headers
  heavy   C2's frames with the source address drawn from 1,024 values,
          skewed (value = floor(1024 * u^3), u uniform): heavy hitters

C2 / C3 / C4 are the worst case for inserts (almost every packet is its own
flow); `heavy` is the worst case for contention on a row.

Per workload, with HIP events around each call on one resident batch and a
2^25-slot table, alternating the three inside one process:
  walk_ms     the batch walk (16-byte records), the yardstick
  fresh       update of a table just reset (every flow is an insert)
  warm        update of a table that already holds the batch's flows
Rates are packets over the median time; bytes_per_packet is what an update has to move at
least (model below), achieved_GBps that over the median.

tools/flowbench_conv.py is a further leg on the same tables: conversations /
top-k (nsd_flow_conv_device) beside a whole-table export and host sort.

The result (one JSON object per workload and a merged flowbench.json) goes
to --out (default bench_out/flowbench).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "netsniff-ng_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = ["udp64", "imix", "ipv6x", "heavy"]
SLOTS_LOG2 = 25


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def update_bytes_per_packet(counters, n):
    """The bytes one update must move per packet at the least: the packet's
    descriptor (8) and record (16), the header bytes of its key (IPv4: 8
    address + 2 fragment + 4 port bytes + 1 flag byte = 15; IPv6: 32 + 4 + 1 =
    37), and in the table its state word (4), the 40-byte key (compared, or
    written by the commit) and the 36 bytes of counters it adds to."""
    v4, v6 = int(counters[7]), int(counters[8])
    key = (15 * v4 + 37 * v6) / max(n, 1)
    return 8 + 16 + key + 4 + 40 + 36


def workload_batch(name, n, dev):
    """(frames, desc) of one workload on the device (the table in the module's docstring)."""
    import numpy as np
    import torch
    import nsd_testlib as T
    cfg = {"udp64": T.SYN_UDP64, "imix": T.SYN_IMIX, "ipv6x": T.SYN_IPV6X, "heavy": T.SYN_UDP64}[name]
    frames, desc, hdesc = T.make_device_batch(cfg, n, device=dev)
    if name == "heavy":
        assert (T.desc_caplen(hdesc) == 64).all() and (np.diff(T.desc_off(hdesc)) == 64).all()
        g = torch.Generator(device=dev)
        g.manual_seed(0x5EED)
        flow = (torch.rand(n, device=dev, generator=g) ** 3 * 1024).to(torch.int64).clamp_(0, 1023)
        v = frames[:n * 64].view(n, 64)
        v[:, 26], v[:, 27] = 10, 0
        v[:, 28], v[:, 29] = (flow >> 8).to(torch.uint8), (flow & 255).to(torch.uint8)
        v[:, 34], v[:, 35] = 4, 0        # (C2's source port varies with i: one port for all)
        del flow, v
    return frames, desc


def run_one(args):
    import numpy as np
    import torch
    import nsd
    import nsd_testlib as T
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n = args.packets
    frames, desc = workload_batch(args.one, n, dev)
    L = nsd.lib()
    rec = torch.empty(n * nsd.REC_BYTES, dtype=torch.uint8, device=dev)
    ext = torch.empty(nsd.ext_pool_words(n) if args.one == "ipv6x" else 1 << 20, dtype=torch.int32, device=dev)
    used = torch.zeros(1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(nsd.NCOUNTERS, dtype=torch.int64, device=dev)
    ws = torch.empty(L.nsd_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def walk():
        nsd.dissect_device(frames, desc, mode=nsd.PRINT_NORM, rec=rec, ext=ext, ext_used=used, counters=cnt,
                           workspace=ws)

    def timed(fn):
        if fn is walk:   # (a fresh pool and counters, outside the timed span)
            used.zero_()
            cnt.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    table = nsd.FlowTable(1 << (SLOTS_LOG2 - 1))
    assert table.slots == 1 << SLOTS_LOG2
    update = lambda: table.update(frames, desc, rec, ext)   # noqa: E731
    timed(walk)
    counters = cnt.cpu().numpy().view(np.uint64).copy()
    assert int(counters[nsd.CNT_OVERFLOW]) == 0, "ext pool too small for the workload"
    bpp = update_bytes_per_packet(counters, n)
    res = {"workload": args.one, "packets": n, "slots": table.slots, "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "library": L.nsd_build_info().decode(),
           "bytes_per_packet": round(bpp, 2)}
    times = {"fresh": [], "warm": []}
    walk_ms, stats = [], None
    for step in range(args.warmup + args.steps):
        w = timed(walk)
        table.reset()
        fresh = timed(update)
        if step == 0:
            # what one update leaves in the table
            _, c, st = table.export_device(max_flows=0, flows=rec)
            torch.cuda.synchronize()
            stats = [int(x) for x in st.cpu().numpy().view(np.uint64)] + [int(c.cpu()[0])]
            continue
        warm = timed(update)
        if step >= args.warmup:
            walk_ms.append(w)
            times["fresh"].append(fresh)
            times["warm"].append(warm)
    assert stats[0] == n and stats[1] + stats[2] + stats[3] == n and stats[4] == 0 and stats[5] == stats[-1], stats
    wm = median(walk_ms)
    res["stats"] = dict(zip(["pkts", "keyed", "noip", "skipped", "full", "flows"], stats[:6]))
    res["walk_ms"] = {"median": round(wm, 4), "min": round(min(walk_ms), 4), "max": round(max(walk_ms), 4),
                      "Mpkt_s": round(n / wm / 1e3, 1)}
    for kind in ("fresh", "warm"):
        xs = times[kind]
        m = median(xs)
        res[kind] = {"median_ms": round(m, 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
                     "Mpkt_s": round(n / m / 1e3, 1), "achieved_GBps": round(n * bpp / m / 1e6, 1),
                     "ratio_to_walk": round(m / wm, 2)}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"flowbench_{args.one}.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
    table.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "flowbench"))
    ap.add_argument("--limit", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--one", default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if args.warmup < 1:
        ap.error("--warmup must be at least 1")
    if args.one:
        return run_one(args)
    merged = {}
    for w in args.workloads.split(","):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, "-u", os.path.abspath(__file__), "--one", w,
               "--packets", str(args.packets), "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--out", args.out]
        print("+", " ".join(cmd), flush=True)
        r = subprocess.run(cmd)
        if r.returncode != 0:
            print(f"flowbench: step {w} ended with status {r.returncode}; stopping", flush=True)
            return r.returncode
        with open(os.path.join(args.out, f"flowbench_{w}.json")) as f:
            merged[w] = json.load(f)
    with open(os.path.join(args.out, "flowbench.json"), "w") as f:
        json.dump(merged, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
