"""kbench.py - development timing of the dissect kernel alone: K launches over
one resident synthetic batch per config, kernel ms from HIP events (no
result checks: experiment variants that skip a phase run through it too).
Not the benchmark (bench.py is).

  python tools/kbench.py --configs udp64,imix,ipv6x --steps 10 [--lib path]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "netsniff-ng_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def timeline_report(key, buf, NW=16384):
    """The per-wave stamps of one dissect_fast launch (KB_DBG) as text."""
    a = buf.reshape(5, NW).astype(np.int64)
    # the last launch's waves alone (an earlier launch on a larger grid leaves
    # its stamps in the slots past this grid's): a launch lasts well under 1 ms
    nw = int(np.count_nonzero(a[0] > a[0].max() - 100000))
    assert np.all(a[0][:nw] > a[0].max() - 100000)
    st, en, be, hw, t78 = (a[k][:nw] for k in range(5))
    t0 = st.min()
    us = lambda x: (x - t0) / 100.0   # noqa: E731
    s, e, bl, m = us(st), us(en), us(be), us(t78)
    xcc = hw & 15
    hid = hw >> 8
    cu = (xcc << 8) | (((hid >> 13) & 3) << 5) | (((hid >> 12) & 1) << 4) | ((hid >> 8) & 15)
    grp = (np.arange(nw) // 4) % 8
    wv = np.arange(nw) % 4
    q = lambda x: " ".join(f"{np.percentile(x, p):.1f}" for p in (0, 10, 50, 90, 100))   # noqa: E731
    L = [f"{key} waves {nw}, CUs {len(np.unique(cu))}, XCDs {len(np.unique(xcc))} (us from the first wave's start; p0 p10 p50 p90 p100)",
         f"  wave start      {q(s)}",
         f"  7/8 of share    {q(m[t78 > 0]) if (t78 > 0).any() else '-'}   ({int((t78 > 0).sum())} waves: the mark is a static tile's)",
         f"  fast_tiles end  {q(e)}   mean {e.mean():.1f}",
         f"  block end       {q(bl)}",
         "  by XCD (XCC_ID): waves, fast_tiles end mean / max, block%8 labels seen"]
    for x in np.unique(xcc):
        k = xcc == x
        L.append(f"    xcd {x}: {int(k.sum()):4d}  {e[k].mean():.1f} / {e[k].max():.1f}  labels {sorted(set(grp[k].tolist()))}")
    cm = np.array([e[cu == c].mean() for c in np.unique(cu)])
    cx = np.array([e[cu == c].max() for c in np.unique(cu)])
    L.append(f"  by CU: mean end {q(cm)}; max end {q(cx)}; waves per CU {sorted(set(int((cu == c).sum()) for c in np.unique(cu)))}")
    L.append(f"  by wave in block: mean end {[round(float(e[wv == w].mean()), 1) for w in range(4)]}")
    blk = e[:nw - nw % 4].reshape(-1, 4)
    L.append(f"  within-block spread mean {np.mean(blk.max(1) - blk.min(1)):.1f}, first / second half of the grid mean end "
             f"{e[:nw // 2].mean():.1f} / {e[nw // 2:].mean():.1f}")
    # a wave's pace before and after its 7/8 mark (us per 1/8 share): waves
    # that speed up as others end would mean the tail is bandwidth-bound
    ok = t78 > 0
    if ok.sum() >= nw // 2:
        front = (m[ok] - s[ok]) / 7.0
        back = e[ok] - m[ok]
        L.append(f"  us per eighth of a share: front {q(front)}; last eighth {q(back)}")
        late = e[ok] >= np.percentile(e[ok], 90)
        L.append(f"  the latest tenth of the waves: front {front[late].mean():.2f}, last eighth {back[late].mean():.2f}; "
                 f"the earliest tenth: front {front[e[ok] <= np.percentile(e[ok], 10)].mean():.2f}, "
                 f"last eighth {back[e[ok] <= np.percentile(e[ok], 10)].mean():.2f}")
    # balanced end: the waves' tile phases at their own pace, work shared
    # perfectly (the mean end), against the actual last end
    L.append(f"  last fast_tiles end {e.max():.1f}, mean {e.mean():.1f}: a perfectly balanced tile phase would end "
             f"{e.max() - e.mean():.1f} us ({100 * (e.max() - e.mean()) / bl.max():.1f} % of the launch) sooner at the waves' own pace")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="udp64,imix,ipv6x")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--grid", type=int, default=0)
    ap.add_argument("--records", default="both", choices=["compact", "full", "both"])
    ap.add_argument("--sched", default="adaptive", choices=["adaptive", "split", "fused"],
                    help="kernel schedule (nsd_set_schedule)")
    ap.add_argument("--bpf", action="store_true", help="also time the device BPF filter (bench.bpf_bench: "
                    "verdicts, and with the compaction, whose accepted count it checks)")
    ap.add_argument("--dbg-out", default=os.path.join(ROOT, "bench_out", "var"),
                    help="where KB_DBG keeps the stamps it read (dbg_<config>_rec<bytes>.npy)")
    ap.add_argument("--lib", default=None, help="a variant libnsdissect.so (tools/build_variant.sh) "
                    "loaded instead of the in-tree one (dev tools only; the product loads its own)")
    args = ap.parse_args()
    import nsd
    if args.lib:
        nsd.LIB_PATH = os.path.abspath(args.lib)
    print(f"library {os.path.relpath(nsd.LIB_PATH, ROOT)} schedule {args.sched}", flush=True)
    nsd.set_schedule({"adaptive": nsd.SCHED_ADAPTIVE, "split": nsd.SCHED_SPLIT, "fused": nsd.SCHED_FUSED}[args.sched])
    import bench
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    forms = {"compact": [True], "full": [False], "both": [False, True]}[args.records]
    for key in args.configs.split(","):
        for compact in forms:
            b = bench.Batch(key, args.packets, 0, 1, dev, compact=compact)
            if args.bpf:
                r = bench.bpf_bench(b, args.steps, args.warmup)
                print(f"{key:6s} bpf kernel_ms={r['kernel_ms']:.4f} compact_ms={r['compact_ms']:.4f} "
                      f"frac={r['roofline']['frac']} accepted={r['accepted']}", flush=True)
            ms = bench.time_steps(b, args.mode, args.steps, args.warmup, 0 if compact else args.grid)
            cnt = b.counters.cpu().numpy().view(np.uint64)
            r = b.roofline(ms)
            print(f"{key:6s} rec{b.rec_b:<2d} {nsd.last_schedule()} kernel_ms={ms:.4f} frac={r['frac'] if r else None} "
                  f"read_frac={r['read_frac'] if r else None} pkts_counted={int(cnt[32])}", flush=True)
            if os.environ.get("KB_ENDS"):
                # counters 56..61 of an instrumented variant (a timeline patch):
                # ~min / max of block start, wave tile-phase end, block end
                # (s_memrealtime, 100 MHz), one more launch with zeroed counters
                b.counters.zero_()
                b.step(args.mode, 0 if compact else args.grid, zero=False)
                b.sync()
                c = b.counters.cpu().numpy().view(np.uint64)
                inv = lambda x: int(~np.uint64(x))   # noqa: E731
                t0 = inv(c[56])
                us = lambda t: round((t - t0) / 100.0, 1)   # noqa: E731
                print(f"{key:6s} timeline_us start {us(t0)}..{us(int(c[57]))} tiles_end {us(inv(c[58]))}.."
                      f"{us(int(c[59]))} block_end {us(inv(c[60]))}..{us(int(c[61]))}", flush=True)
                if os.environ.get("KB_ENDS") == "xcd":
                    print(f"{key:6s} per-group (block * 4 / grid: dispatch round) last tile-phase end {[us(int(x)) for x in c[40:48]]} "
                          f"last block end {[us(int(x)) for x in c[48:56]]}", flush=True)
            if os.environ.get("KB_DBG"):
                # a timing variant (tools/variants/timeline.patch: g_dbg,
                # nsd_dbg_read) of dissect_fast: per wave, s_memrealtime at its
                # start, one tile before 7/8 of its share, at the end of fast_tiles
                # and at the block's end, and XCC_ID | HW_ID << 8.  One more
                # launch, then the spread by XCD, CU and wave, and when a
                # perfectly balanced launch would end.
                import ctypes
                b.step(args.mode, 0 if compact else args.grid, zero=False)
                b.sync()
                NW = 16384
                buf = np.zeros(5 * NW, dtype=np.uint64)
                assert nsd.lib().nsd_dbg_read(ctypes.c_void_p(buf.ctypes.data)) == 0
                out = args.dbg_out
                os.makedirs(out, exist_ok=True)
                np.save(os.path.join(out, f"dbg_{key}_rec{b.rec_b}.npy"), buf)
                print(timeline_report(key, buf), flush=True)
            b.free()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
