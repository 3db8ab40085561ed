"""flowbench_ts.py - timing of the timed flow table (nsd_flow_create_timed and
the *_ts entries: capture timestamps kept per flow) beside the plain table, leg
by leg, on flowbench.py's workloads.  Not the benchmark (bench.py is).

  python tools/flowbench_ts.py [--packets N] [--steps K] [--warmup W] [--out DIR]
                               [--lib PATH --untimed-only] [--tag NAME]

One child process per workload, each under its own time limit; the first that
fails ends the run (nothing more is started on the GPU after a fault or a
timeout):

  udp64   C2 fresh: 16,777,216 flows in a 2^25-slot table
  heavy   C2's frames in 1,024 flows, skewed

Per workload and per kind of table (plain, timed), HIP events around each call,
medians over --steps after --warmup rounds, the kinds and legs alternating in
one process:
  update         flow_update + flow_commit of the batch into the table just reset
  export         nsd_flow_export_device[_ts] of every row (72 / 88 bytes each)
  conversations  nsd_flow_conv_device[_ts], BY_BYTES, k = 64
  expire         nsd_flow_expire_device[_ts] with `before` set so that 0 %, 50 %
                 and 100 % of the flows qualify (the median `last` / t_last of
                 the exported rows), room for every row; the table restored by
                 reset + update before every timed call
The counts of the first round are checked.

--lib PATH --untimed-only runs the plain legs against another build of the
library (one without the timed entries will do): the no-regression comparison
of the untimed update takes the parent commit's library twice and this tree's
once in one session.  The result (one JSON object per workload and a merged
flowbench_ts[_TAG].json) goes to --out (default bench_out/flowbench).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "netsniff-ng_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = ["udp64", "heavy"]
SLOTS_LOG2 = 25
U64_MAX = (1 << 64) - 1
CONV_K = 64


def stat(xs, digits=4):
    s = sorted(xs)
    return {"median_ms": round(s[len(s) // 2], digits), "min_ms": round(s[0], digits), "max_ms": round(s[-1], digits)}


def run_one(args):
    import torch
    import nsd
    if args.lib:
        nsd.LIB_PATH = os.path.abspath(args.lib)
    from flowbench import workload_batch
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n = args.packets
    frames, desc = workload_batch(args.one, n, dev)
    L = nsd.lib()
    rec, ext, _, _ = nsd.dissect_device(frames, desc, mode=nsd.PRINT_NORM)
    # a microsecond a packet from an epoch in 2023, jitter of a millisecond: not monotonic
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    ts = (1_700_000_000_000_000_000 + torch.arange(n, dtype=torch.int64, device=dev) * 1000 +
          torch.randint(0, 1 << 20, (n,), dtype=torch.int64, device=dev, generator=g))
    kinds = ["plain"] if args.untimed_only else ["plain", "timed"]
    tables = {k: nsd.FlowTable(1 << (SLOTS_LOG2 - 1), **({"timed": True} if k == "timed" else {})) for k in kinds}
    assert all(t.slots == 1 << SLOTS_LOG2 for t in tables.values())

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def update(kind):
        if kind == "timed":
            tables[kind].update(frames, desc, rec, ext, ts=ts)
        else:
            tables[kind].update(frames, desc, rec, ext)

    res = {"workload": args.one, "packets": n, "slots": 1 << SLOTS_LOG2, "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "library": L.nsd_build_info().decode(), "kinds": {}}
    # the rows once per kind: the flow count, the thresholds and the counts to check
    plan = {}
    for kind in kinds:
        t = tables[kind]
        update(kind)
        _, c, st = t.export_device(max_flows=0)
        nflows = int(c.cpu()[0])
        row = nsd.FLOWT_BYTES if kind == "timed" else nsd.FLOW_BYTES
        out = torch.empty(nflows * row, dtype=torch.uint8, device=dev)
        (t.export_device_ts if kind == "timed" else t.export_device)(flows=out)
        col = out.view(torch.int64).view(nflows, row // 8)[:, 10 if kind == "timed" else 8]
        half = int(col.sort().values[nflows // 2])
        below = int((col < half).sum())
        del col
        ws = torch.empty(max(int(L.nsd_flow_expire_workspace_bytes(t.h)), int(L.nsd_flow_conv_workspace_bytes(t.h))),
                         dtype=torch.uint8, device=dev)
        conv = torch.empty(CONV_K * (nsd.CONVT_BYTES if kind == "timed" else nsd.CONV_BYTES), dtype=torch.uint8,
                           device=dev)
        plan[kind] = {"nflows": nflows, "out": out, "ws": ws, "conv": conv,
                      "count": torch.zeros(2, dtype=torch.int32, device=dev),
                      "legs": [("expire_0pct", 0, 0), ("expire_50pct", half, below), ("expire_100pct", U64_MAX, nflows)]}
        res["kinds"][kind] = {"flows": nflows, "row_bytes": row,
                              "expire_workspace_bytes": int(L.nsd_flow_expire_workspace_bytes(t.h))}
    times = {kind: {} for kind in kinds}
    for step in range(args.warmup + args.steps):
        for kind in kinds:          # alternating, in one process
            t, p = tables[kind], plan[kind]
            sample = {}
            for j, (name, before, want) in enumerate(p["legs"]):
                timed(t.reset)
                u = timed(lambda: update(kind))
                if j == 0:
                    sample["update"] = u
                call = t.expire_device_ts if kind == "timed" else t.expire_device
                sample[name] = timed(lambda: call(before, 0, flows=p["out"], count=p["count"], workspace=p["ws"]))
                if step == 0:
                    c = [int(x) for x in p["count"].cpu()]
                    assert c == [want, want], (kind, name, c)
            timed(t.reset)
            timed(lambda: update(kind))
            exp = t.export_device_ts if kind == "timed" else t.export_device
            sample["export"] = timed(lambda: exp(flows=p["out"], count=p["count"][:1]))
            cv = t.conversations_device_ts if kind == "timed" else t.conversations_device
            sample["conversations"] = timed(lambda: cv(nsd.CONV_BY_BYTES, CONV_K, conv=p["conv"], count=p["count"],
                                                       workspace=p["ws"]))
            if step >= args.warmup:
                for name, ms in sample.items():
                    times[kind].setdefault(name, []).append(ms)
    for kind in kinds:
        res["kinds"][kind].update({name: stat(v) for name, v in times[kind].items()})
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"flowbench_ts{args.tag}_{args.one}.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
    for t in tables.values():
        t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "flowbench"))
    ap.add_argument("--limit", type=int, default=400, help="seconds each GPU step may take")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--lib", default=None, help="another build of libnsdissect.so to measure")
    ap.add_argument("--untimed-only", action="store_true", help="only the plain table's legs")
    ap.add_argument("--tag", default="", help="suffix of the output files' names")
    ap.add_argument("--one", default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if args.warmup < 1:
        ap.error("--warmup must be at least 1")
    if args.tag and not args.tag.startswith("_"):
        args.tag = "_" + args.tag
    if args.one:
        return run_one(args)
    merged = {}
    for w in args.workloads.split(","):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, "-u", os.path.abspath(__file__), "--one", w,
               "--packets", str(args.packets), "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--out", args.out] + (["--lib", args.lib] if args.lib else []) + \
              (["--untimed-only"] if args.untimed_only else []) + (["--tag", args.tag] if args.tag else [])
        print("+", " ".join(cmd), flush=True)
        r = subprocess.run(cmd)
        if r.returncode != 0:
            print(f"flowbench_ts: step {w} ended with status {r.returncode}; stopping", flush=True)
            return r.returncode
        with open(os.path.join(args.out, f"flowbench_ts{args.tag}_{w}.json")) as f:
            merged[w] = json.load(f)
    with open(os.path.join(args.out, f"flowbench_ts{args.tag}.json"), "w") as f:
        json.dump(merged, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
