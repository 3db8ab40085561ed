"""flowbench_conv.py - timing of conversations / top-k from the flow table
(nsd_flow_conv_device) beside what gave the same answer before it existed:
nsd_flow_export of the whole table plus a host sort.  A leg of flowbench.py
(its workloads, its table); not the benchmark (bench.py is).

  python tools/flowbench_conv.py [--packets N] [--steps K] [--warmup W] [--out DIR]

One child process per workload, each under its own time limit; the first that
fails ends the run (nothing more is started on the GPU after a fault or a
timeout):

  udp64   C2 fresh: 16,777,216 flows in a 2^25-slot table
  heavy   C2's frames in 1,024 flows, skewed

Per workload, on a table that holds one update of the batch:
  conv    nsd_flow_conv_device by bytes for k = 0 (init + pair + a gather
          that writes nothing: what pairing costs), k = 1,024 (pair + the
          radix select + gather) and k = all (pair + gather of every row),
          and by first for k = 1,024; HIP events around the call, medians over
          --steps.  Launches = the kernels the call enqueues.
  export  nsd_flow_export of the whole table (device pack, copy to the host,
          sort by first) and a host sort of the rows by bytes, by the host's
          clock (the call ends in a synchronise); at most 3 repetitions, it
          takes seconds.  It does not pair the directions, so it is a lower
          bound of what a user had to do.
The k = 1,024 rows are checked against the export (the 1,024 largest byte
counts, no reverse flows in these workloads).

The result (one JSON object per workload and a merged flowbench_conv.json)
goes to --out (default bench_out/flowbench).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "netsniff-ng_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = ["udp64", "heavy"]
SLOTS_LOG2 = 25
ALL = 0xFFFFFFFF


def stat(xs, digits=4):
    s = sorted(xs)
    return {"median_ms": round(s[len(s) // 2], digits), "min_ms": round(s[0], digits), "max_ms": round(s[-1], digits)}


def run_one(args):
    import numpy as np
    import torch
    import nsd
    from flowbench import workload_batch
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n = args.packets
    frames, desc = workload_batch(args.one, n, dev)
    L = nsd.lib()
    rec, ext, _, _ = nsd.dissect_device(frames, desc, mode=nsd.PRINT_NORM)
    table = nsd.FlowTable(1 << (SLOTS_LOG2 - 1))
    assert table.slots == 1 << SLOTS_LOG2
    table.update(frames, desc, rec, ext)
    torch.cuda.synchronize()
    del rec, ext, frames, desc
    # the yardstick first: it also gives the answer to check against
    reps = min(args.steps, 3)
    export_ms, sort_ms, flows = [], [], None
    for _ in range(reps):
        del flows
        t0 = time.perf_counter()
        flows, stats = table.export()
        t1 = time.perf_counter()
        order = np.lexsort((flows["first"], -flows["bytes"].astype(np.int64)))
        t2 = time.perf_counter()
        export_ms.append((t1 - t0) * 1e3)
        sort_ms.append((t2 - t1) * 1e3)
    nflows = len(flows)
    assert nflows == int(stats[nsd.FLOW_ST_FLOWS]) and int(stats[nsd.FLOW_ST_FULL]) == 0
    top = flows[order[:1024]]
    res = {"workload": args.one, "packets": n, "slots": table.slots, "flows": nflows, "steps": args.steps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "library": L.nsd_build_info().decode(),
           "workspace_bytes": int(L.nsd_flow_conv_workspace_bytes(table.h)),
           "export_and_sort": {"repetitions": reps, "export": stat(export_ms, 1), "host_sort_by_bytes": stat(sort_ms, 1),
                               "total_median_ms": round(stat(export_ms, 1)["median_ms"] +
                                                        stat(sort_ms, 1)["median_ms"], 1)}}
    del flows, order
    ws = torch.empty(res["workspace_bytes"], dtype=torch.uint8, device=dev)
    out = torch.empty(nflows * nsd.CONV_BYTES, dtype=torch.uint8, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)

    def timed(by, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        table.conversations_device(by, k, conv=out, count=count, workspace=ws)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    legs = [("bytes_k0", nsd.CONV_BY_BYTES, 0, 3), ("bytes_k1024", nsd.CONV_BY_BYTES, 1024, 35),
            ("bytes_all", nsd.CONV_BY_BYTES, ALL, 3), ("first_k1024", nsd.CONV_BY_FIRST, 1024, 19)]
    times = {name: [] for name, _, _, _ in legs}
    for step in range(args.warmup + args.steps):
        for name, by, k, _ in legs:     # alternating, in one process
            ms = timed(by, k)
            if step >= args.warmup:
                times[name].append(ms)
            if step == 0:
                c = [int(x) for x in count.cpu()]
                assert c == [min(k, nflows), nflows], (name, c)
                if name == "bytes_k1024":
                    rows = out[:c[0] * nsd.CONV_BYTES].cpu().numpy().view(nsd.CONV_DTYPE)
                    rows = rows[np.lexsort((rows["first"], -rows["bytes_src"].astype(np.int64)))]
                    for f in ("src", "sport", "bytes_src", "pkts_src", "first", "last"):
                        assert np.array_equal(rows[f], top[{"bytes_src": "bytes", "pkts_src": "pkts"}.get(f, f)]), f
                    assert not rows["pkts_dst"].any()
    res["conv"] = {name: dict(stat(times[name]), k="all" if k == ALL else k, launches=launches)
                   for name, _, k, launches in legs}
    res["speedup_top1024_over_export_and_sort"] = round(
        res["export_and_sort"]["total_median_ms"] / res["conv"]["bytes_k1024"]["median_ms"], 1)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"flowbench_conv_{args.one}.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
    table.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "flowbench"))
    ap.add_argument("--limit", type=int, default=400, help="seconds each GPU step may take")
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
            print(f"flowbench_conv: step {w} ended with status {r.returncode}; stopping", flush=True)
            return r.returncode
        with open(os.path.join(args.out, f"flowbench_conv_{w}.json")) as f:
            merged[w] = json.load(f)
    with open(os.path.join(args.out, "flowbench_conv.json"), "w") as f:
        json.dump(merged, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
