"""bench.py's line fields that need no GPU: the roofline's algorithmic bytes,
line floor and traffic ratios from the committed goldens (wsum.json,
lines.json), the CPU baseline's shape (the reference's objects as `value`),
the library's source provenance, what a plain run leaves to --full, and
--dump-outputs (its records on the GPU)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import nsd  # noqa: E402
import nsd_testlib as T  # noqa: E402


def _fake_batch(key, n=1 << 24):
    b = object.__new__(bench.Batch)
    b.key, b.n_shard, b.shards, b.n, b.compact, b.rec_b = key, n, 1, n, True, bench.CREC_B
    b.wsum = bench.wsum_for(key, n, 0)
    b.lines = bench.lines_for(key, n, 0)
    return b


def test_roofline_line_floor():
    n = 1 << 24
    for key in ("udp64", "imix", "ipv6x"):
        b = _fake_batch(key)
        assert b.wsum is not None and b.lines is not None, key
        floor = 128 * b.lines + 8 * n
        traffic = {"read_bytes": 1.1 * floor, "write_bytes": 2.0 * 8 * n, "bytes_per_launch": 1.1 * floor + 16 * n}
        r = b.roofline(1.0, traffic, None, {"gbs": 7000.0})
        assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == bench.HBM_PEAK_GBS
        alg = 8 * n + b.wsum + 8 * n
        assert abs(r["achieved"] - alg / 1e-3 / 1e9) < 0.1
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
        assert r["line_floor_bytes_per_pkt"]["read"] == round(floor / n, 2)
        assert r["traffic_vs_line_floor"] == {"read": 1.1, "write": 2.0}
        assert r["line_floor_bytes_per_pkt"]["read"] >= r["bytes_per_pkt"]["read"] - 1e-9, key
    # C2: 64-byte frames, two to a line: the floor is the algorithmic bytes
    assert _fake_batch("udp64").lines * 128 == 64 * n
    # a shard the tables do not hold gives no floor
    assert bench.lines_for("imix", 1000, 0) is None


def test_golden_counters_cover_c5():
    want = bench.golden_counters("imix", 1 << 24, 8)
    assert want is not None and int(want[nsd.CNT_PKTS]) == 8 << 24


def test_library_info_names_its_sources():
    info = bench.library_info()
    assert info["source_matches_tree"] and info["source_sha256_16"] == nsd.source_hash()
    assert info["build"].endswith(info["source_sha256_16"])
    assert len(info["sha256_16"]) == 16 and int(info["sha256_16"], 16) >= 0


EXTRAS = ("no_cpu", "no_e2e", "no_bpf", "no_replay", "no_legs", "no_pmc")


def test_plain_run_takes_only_the_headline():
    """Without --full every leg beside the headline is off; --full turns them
    on and the --no-* switches take single ones out again."""
    plain = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not plain.full and plain.steps == 7 and all(getattr(plain, k) for k in EXTRAS)
    full = bench.parse_args(["--full"])
    assert full.full and not any(getattr(full, k) for k in EXTRAS)
    some = bench.parse_args(["--full", "--no-cpu", "--no-pmc"])
    assert [k for k in EXTRAS if getattr(some, k)] == ["no_cpu", "no_pmc"]


def test_plain_line_and_counter_dump_host(tmp_path):
    """A plain run's line (host walk in place of the kernels): the headline
    fields, none of --full's legs, and --dump-outputs writes the counters the
    timed steps returned (= the oracle's x steps)."""
    n, steps = 3000, 3
    args = bench.parse_args(["--gpus", "1", "--config", "imix", "--packets", str(n), "--steps", str(steps),
                             "--warmup", "1", "--dump-outputs", str(tmp_path / "d")])
    line = bench.run(args, 0, 1, "cpu", engine="host")
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["unit"] == "Mpkt/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8"
    assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3) / 1e6) <= 0.02 * line["value"] + 0.01
    for k in ("legs", "other_records", "cpu_baseline", "end_to_end", "replay", "bpf_filter"):
        assert line[k] is None, k
    frames, desc = T.make_batch(T.SYN_IMIX, n)
    _, _, want, _ = T.oracle_records(frames, desc)
    got = np.load(tmp_path / "d" / "counters.npy")
    assert got.dtype == np.float64 and np.array_equal(got, (want * np.uint64(steps)).astype(np.float64))
    assert sorted(os.listdir(tmp_path / "d")) == ["counters.npy"]


@pytest.mark.gpu
@pytest.mark.parametrize("key,cfg,n,records", [("ipv6x", T.SYN_IPV6X, 20001, "compact"),
                                               ("imix", T.SYN_IMIX, 20001, "full"),
                                               ("udp64", T.SYN_UDP64, bench.DUMP_RECORDS + 4097, "compact")])
def test_dump_outputs_device(tmp_path, key, cfg, n, records):
    """--dump-outputs after a plain run on the GPU: the dumped records are the
    oracle's for the sampled packets (a batch past DUMP_RECORDS is sampled,
    the same packets every run), the counters the oracle's x steps, and a
    second run with the same arguments dumps the same arrays."""
    import torch
    steps = 2
    dumps = []
    for d in ("a", "b"):
        args = bench.parse_args(["--gpus", "1", "--config", key, "--packets", str(n), "--steps", str(steps),
                                 "--warmup", "1", "--records", records, "--dump-outputs", str(tmp_path / d)])
        line = bench.run(args, 0, 1, torch.device("cuda", 0), "device")
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["legs"] is None
        dumps.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = dumps
    assert sorted(a) == ["counters", "ext_used", "record_index", "records"]
    for name in a:
        assert a[name].dtype == np.float64 and np.array_equal(a[name], b[name]), name
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    idx = a["record_index"].astype(np.int64)
    assert len(idx) == len(a["records"]) and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert len(idx) == n if n <= bench.DUMP_RECORDS else bench.DUMP_RECORDS // 2 < len(idx) <= bench.DUMP_RECORDS
    frames, desc = T.make_batch(cfg, n)
    _, _, cnt, _ = T.oracle_records(frames, desc)
    launches = steps if a["ext_used"][0] == 0 else 1   # (pool words taken: timed launch by launch)
    assert np.array_equal(a["counters"], (cnt * np.uint64(launches)).astype(np.float64))
    orec, oext, _, _ = T.oracle_records(frames, desc[idx])
    rows = a["records"]
    if records == "compact":
        want, pool = nsd.compact_of(orec, oext)
        entry = ((want["nflags"] & 7) == 7) & (want["nlayers"] == 0) & ((want["nflags"] & nsd.F_OVERFLOW) == 0)
        side = (want["nlayers"] != 0) | (((want["nflags"] & 7) != 7) & ((want["nflags"] & nsd.F_LEAF_END) != 0))
        assert rows.shape[1] == 6
        assert np.array_equal(rows[:, 0], np.where(entry, -1.0, want["chain"].astype(np.float64)))
        for col, fld in ((1, "ip_csum"), (2, "nflags"), (3, "nlayers")):
            assert np.array_equal(rows[:, col], want[fld].astype(np.float64)), fld
        assert np.array_equal(rows[:, 4], np.where(side, pool[:len(idx)], 0).astype(np.float64))
        if key == "ipv6x":
            assert (want["nlayers"] != 0).any()   # the config reaches the side-word form
    else:
        entry = ((orec["nflags"] & 7) == 7) & ((orec["nflags"] & nsd.F_OVERFLOW) == 0)
        assert rows.shape[1] == 11
        for col, fld in enumerate(("chain", "data_off", "tail_off", "ip_csum", "nflags")):
            assert np.array_equal(rows[:, col], orec[fld].astype(np.float64)), fld
        assert np.all(rows[entry, 5:9] == -1)
    # an entry's layer count, resolved through the pool on both sides
    nl = np.zeros(len(idx))
    for i in np.nonzero(entry)[0]:
        slot = int(orec["off2"][i, :4].copy().view("<u4")[0])
        if slot != 0xFFFFFFFF:
            nl[i] = len(nsd.ext_entry(oext, slot)[1])
    assert np.array_equal(rows[:, -1], nl)


def test_cpu_baseline_value_is_the_reference(monkeypatch):
    """`cpu_baseline.value` is the reference's own objects on the 16-CPU
    share (kind "reference"); the restatement sits beside it as `port`;
    without the reference's objects the port's rate is the value."""
    monkeypatch.setattr(bench, "cpu_rate", lambda cfg, n, th, sec, text: (2.0 if text else 30.0, n, sec))
    monkeypatch.setattr(bench, "ref_harness_rate",
                        lambda cfg, key, n=0, frames=True: {"value": 0.1, "cores": 1, "kind": "reference"})
    monkeypatch.setattr(bench, "ref_harness_all_cores",
                        lambda cfg, key, procs, rate1, seconds=8.0: {"value": 1.5, "cores": procs, "kind": "reference",
                                                                     "sample": f"{key} x{procs}"})
    c = bench.cpu_baseline("udp64", 0.01)
    assert c["kind"] == "reference" and c["value"] == 1.5 and c["cores"] == min(bench.cpu_info()[2], 16)
    assert c["port"]["kind"] == "port" and c["port"]["value"] == 2.0
    assert set(c["reference_harness_all_cores"]) >= {"udp64", "imix"}
    monkeypatch.setattr(bench, "ref_harness_all_cores", lambda *a, **k: None)
    c = bench.cpu_baseline("imix", 0.01)
    assert c["kind"] == "port" and c["value"] == 2.0 and "reference_error" in c
    np.testing.assert_equal(c["text_16threads"]["value"], 2.0)
