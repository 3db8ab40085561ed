"""flowbench_expire.py - timing of flow expiry (nsd_flow_expire_device: the
table rebuilt from its survivors) beside what freed slots before it existed:
nsd_flow_export of the whole table plus nsd_flow_reset.  A leg of flowbench.py
(its workloads, its table); not the benchmark (bench.py is).

  python tools/flowbench_expire.py [--packets N] [--steps K] [--warmup W] [--out DIR]

One child process per workload, each under its own time limit; the first that
fails ends the run (nothing more is started on the GPU after a fault or a
timeout):

  udp64   C2 fresh: 16,777,216 flows in a 2^25-slot table
  heavy   C2's frames in 1,024 flows, skewed

Per workload, on a table that holds one update of the batch:
  expire  nsd_flow_expire_device with `before` set so that 0 %, 50 % and 100 %
          of the flows qualify (0, the median `last` of the table's rows,
          UINT64_MAX), room for every row; HIP events around the call, medians
          over --steps after --warmup rounds, the legs alternating in one
          process.  Before every timed call the table is restored by reset +
          update, outside the timed span.  The counts of the first round are
          checked against the exported rows.
  export  the yardstick: nsd_flow_export of the whole table (device pack, copy
          to the host, sort by first) by the host's clock, at most 3
          repetitions, plus nsd_flow_reset (HIP events): what emptied a table
          before, every flow leaving.
  update  beside them, one flow_update of the batch into the table just reset
          (HIP events): what refilling costs.

The result (one JSON object per workload and a merged flowbench_expire.json)
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
U64_MAX = (1 << 64) - 1


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

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def update():
        table.update(frames, desc, rec, ext)

    update()
    torch.cuda.synchronize()
    # the yardstick first: its rows also give the thresholds and the counts to check
    reps = min(args.steps, 3)
    export_ms, flows = [], None
    for _ in range(reps):
        del flows
        t0 = time.perf_counter()
        flows, stats = table.export()
        export_ms.append((time.perf_counter() - t0) * 1e3)
    nflows = len(flows)
    assert nflows == int(stats[nsd.FLOW_ST_FLOWS]) and int(stats[nsd.FLOW_ST_FULL]) == 0
    last = np.sort(flows["last"])
    half = int(last[nflows // 2])
    legs = [("expire_0pct", 0, 0), ("expire_50pct", half, int(np.searchsorted(last, half, side="left"))),
            ("expire_100pct", U64_MAX, nflows)]
    del flows, last
    res = {"workload": args.one, "packets": n, "slots": table.slots, "flows": nflows, "steps": args.steps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "library": L.nsd_build_info().decode(),
           "workspace_bytes": int(L.nsd_flow_expire_workspace_bytes(table.h)), "launches": 4}
    ws = torch.empty(res["workspace_bytes"], dtype=torch.uint8, device=dev)
    out = torch.empty(nflows * nsd.FLOW_BYTES, dtype=torch.uint8, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    times = {name: [] for name, _, _ in legs}
    reset_ms, update_ms = [], []
    for step in range(args.warmup + args.steps):
        for name, before, want in legs:     # alternating, in one process
            r = timed(table.reset)
            u = timed(update)
            ms = timed(lambda: table.expire_device(before, 0, flows=out, count=count, workspace=ws))
            if step >= args.warmup:
                times[name].append(ms)
                reset_ms.append(r)
                update_ms.append(u)
            if step == 0:
                c = [int(x) for x in count.cpu()]
                assert c == [want, want], (name, c)
                _, _, st = table.export_device(max_flows=0)
                st = [int(x) for x in st.cpu()]
                assert st[nsd.FLOW_ST_FLOWS] == nflows - want and st[nsd.FLOW_ST_EXPIRED] == want, (name, st)
    res["expire"] = {name: dict(stat(times[name]), qualifying=want) for name, _, want in legs}
    res["yardstick"] = {"export": dict(stat(export_ms, 1), repetitions=reps), "reset": stat(reset_ms),
                        "export_plus_reset_median_ms": round(stat(export_ms, 1)["median_ms"] +
                                                             stat(reset_ms)["median_ms"], 1),
                        "update_after_reset": stat(update_ms)}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"flowbench_expire_{args.one}.json"), "w") as f:
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
            print(f"flowbench_expire: step {w} ended with status {r.returncode}; stopping", flush=True)
            return r.returncode
        with open(os.path.join(args.out, f"flowbench_expire_{w}.json")) as f:
            merged[w] = json.load(f)
    with open(os.path.join(args.out, "flowbench_expire.json"), "w") as f:
        json.dump(merged, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
