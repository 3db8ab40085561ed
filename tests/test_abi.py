"""C ABI checks that need no GPU: the product library loads, exports every
entry point declared in include/netsniff_dissect.h, and its pure-host parts
(formatter, wrap, lookups) behave; device calls fail loudly without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import nsd
import nsd_testlib as T

HDR = os.path.join(T.ROOT, "include", "netsniff_dissect.h")


def declared_functions():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"^\s*(?:[a-z_][\w\s\*]*?)\b([a-z_]\w*)\s*\(", src, flags=re.M)
    return sorted({n for n in names if n not in ("if", "return", "sizeof")})


def test_header_declares_abi():
    decl = set(declared_functions())
    assert set(nsd.ABI_SYMBOLS) <= decl, set(nsd.ABI_SYMBOLS) - decl


def test_library_exports_every_declared_symbol():
    lib = nsd.lib()
    for name in declared_functions():
        assert hasattr(lib, name), f"libnsdissect.so does not export {name}"


def test_record_layout_matches_header():
    assert nsd.REC_DTYPE.itemsize == 16 and nsd.BPF_INSN.itemsize == 8
    assert nsd.ext_words(6) == 20 and nsd.ext_words(16) == 20 and nsd.ext_words(17) == 68
    assert nsd.REC_DTYPE.fields["nflags"][1] == 10 and nsd.REC_DTYPE.fields["off2"][1] == 11


def test_version_and_device_count():
    assert b"netsniff" in nsd.lib().nsd_version()
    assert nsd.lib().nsd_device_count() >= 0


def test_record_ring_knob():
    """nsd_set_record_ring: 0 adaptive / 1 on / 2 off, returns the previous
    setting, refuses anything else (NSD_ERR_ARG)."""
    prev = nsd.set_record_ring(nsd.RING_OFF)
    try:
        assert nsd.set_record_ring(nsd.RING_ON) == nsd.RING_OFF
        assert nsd.set_record_ring(nsd.RING_ADAPTIVE) == nsd.RING_ON
        for bad in (-1, 3):
            with pytest.raises(ValueError):
                nsd.set_record_ring(bad)
    finally:
        nsd.set_record_ring(prev)


def test_debug_fill_returns_previous_value():
    """nsd_set_debug_fill: -1 off (the default) or a byte 0..255; each call
    returns the value the one before it set."""
    L = nsd.lib()
    prev = L.nsd_set_debug_fill(0xA5)
    try:
        assert prev == -1                              # off by default
        assert L.nsd_set_debug_fill(0) == 0xA5
        assert L.nsd_set_debug_fill(255) == 0
        assert L.nsd_set_debug_fill(-1) == 255
        assert nsd.set_debug_fill(0x5A) == -1          # the binding's wrapper
        assert nsd.set_debug_fill(-1) == 0x5A
    finally:
        L.nsd_set_debug_fill(prev)


def test_debug_fill_rejects_other_arguments():
    """Anything but -1..255 is NSD_ERR_ARG and leaves the setting as it was;
    the wrapper raises before the call."""
    L = nsd.lib()
    prev = L.nsd_set_debug_fill(7)
    try:
        for bad in (-2, 256, 0x1A5, -(1 << 31), (1 << 31) - 1):
            assert L.nsd_set_debug_fill(bad) == -1     # NSD_ERR_ARG
            with pytest.raises(ValueError):
                nsd.set_debug_fill(bad)
        assert L.nsd_set_debug_fill(7) == 7            # still set
    finally:
        L.nsd_set_debug_fill(prev)


def test_library_carries_the_tree_source_hash():
    """The library names the sources it was built from (nsd_build_info's
    `sources` hash, the Makefile's SRCHASH) and they are this tree's: what
    a bench line's `library` reports and the test fixture rebuilds on."""
    info = nsd.lib().nsd_build_info().decode()
    assert re.search(r"; sources [0-9a-f]{16}$", info), info
    assert info.endswith(nsd.source_hash()) and nsd.built_source_hash() == nsd.source_hash()


def test_device_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    frames, desc = T.batch_from_packets([b"\x00" * 64])
    with pytest.raises(nsd.NsdError):
        nsd.entry_batch(frames, desc)


def test_replay_fails_loudly_without_gpu(tmp_path):
    """`--in` through the library needs the device walk: without a GPU the
    replay reports an error (no CPU fallback), the pcap reader alone works."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    path = str(tmp_path / "x.pcap")
    T.write_pcap(path, [b"\x00" * 64] * 3)
    assert len(nsd.pcap_frame_hdrs(path)[1]) == 3
    with pytest.raises(nsd.NsdError):
        nsd.replay_pcap(path)


def test_format_rejects_inconsistent_record():
    frames, desc = T.make_batch(T.SYN_UDP64, 4)
    rec, ext, _, _ = T.oracle_records(frames, desc)
    bad = rec.copy()
    bad["data_off"] += 2               # claims a cursor the bytes do not give
    _, rc = nsd.format_batch(frames, desc, bad, ext)
    assert (rc != 0).all()
    bad = rec.copy()
    bad["off2"][:, 1] += 1             # wrong UDP layer start
    _, rc = nsd.format_batch(frames, desc, bad, ext)
    assert (rc != 0).all()


def test_wrap_basics():
    out, st = nsd.tprintf_wrap(b"x" * 100 + b"\n", cols=80)
    assert out == b"x" * 75 + b"\n   " + b"x" * 25 + b"\n"
    assert st == 0
    # wrap point on spaces/commas: they are dropped
    out, _ = nsd.tprintf_wrap(b"a" * 75 + b" , b\n", cols=80)
    assert out == b"a" * 75 + b"\n   b\n"
    # colour sequences suppress wrapping until closed
    s = b"\033[1m" + b"y" * 90 + b"\033[0m\n"
    out, _ = nsd.tprintf_wrap(s, cols=80)
    assert out.count(b"\n   ") == 1


# The flow table's Python front end as callers know it: every public FlowTable
# method and the module functions beside it, with the parameters and defaults
# of commit 93356fb (before the plain / _ts pairs were folded into shared
# bodies).  Literal strings on purpose: nothing here is read from nsd.py.
_FLOWTABLE_SIGNATURES = {
    "__init__": "(self, max_flows, timed=False)",
    "close": "(self)",
    "conversations": "(self, by=1, k=None)",
    "conversations_device": "(self, by, k, conv=None, count=None, workspace=None, stream=None)",
    "conversations_device_ts": "(self, by, k, conv=None, count=None, workspace=None, stream=None)",
    "conversations_ts": "(self, by=1, k=None)",
    "expire": "(self, before, flags=0, max_flows=None)",
    "expire_device": "(self, before, flags=0, max_flows=None, flows=None, count=None, workspace=None, stream=None)",
    "expire_device_ts": "(self, before_ns, flags=0, max_flows=None, flows=None, count=None, workspace=None, stream=None)",
    "expire_ts": "(self, before_ns, flags=0, max_flows=None)",
    "export": "(self, max_flows=None)",
    "export_device": "(self, max_flows=None, flows=None, count=None, stats=None, stream=None)",
    "export_device_ts": "(self, max_flows=None, flows=None, count=None, stats=None, stream=None)",
    "export_ts": "(self, max_flows=None)",
    "reset": "(self, stream=None)",
    "update": "(self, frames, desc, rec, ext=None, base=0, n=None, stream=None, ts=None)",
}
_FLOW_FUNCTION_SIGNATURES = {
    "flow_batch": "(frames, desc, mode=0, linktype=1, max_flows=None)",
    "flow_cpu": "(frames, desc, rec, ext=None, base=0, max_flows=None)",
    "flow_cpu_ts": "(frames, desc, rec, ts, ext=None, base=0, max_flows=None)",
    "conv_cpu": "(flows, by=0, max_conv=None)",
    "conv_cpu_ts": "(flows, by=0, max_conv=None)",
    "flow_expire_cpu": "(flows, before, flags=0, max_flows=None)",
    "flow_expire_cpu_ts": "(flows, before_ns, flags=0, max_flows=None)",
    "pcap_flows": "(path, table, mode=0, prog=None)",
    "pcap_flows_expire": "(path, table, every, idle, flags=0, mode=0, prog=None)",
    "pcap_flows_expire_ts": "(path, table, every, idle_ns, flags=0, mode=0, prog=None)",
}


def test_flow_front_end_signatures_pinned():
    import inspect
    public = {name for name, member in vars(nsd.FlowTable).items()
              if callable(member) and (not name.startswith("_") or name == "__init__")}
    assert public == set(_FLOWTABLE_SIGNATURES)
    for name, sig in _FLOWTABLE_SIGNATURES.items():
        assert str(inspect.signature(getattr(nsd.FlowTable, name))) == sig, name
    for name, sig in _FLOW_FUNCTION_SIGNATURES.items():
        assert str(inspect.signature(getattr(nsd, name))) == sig, name
    # the row sizes the folded bodies take from the dtypes are the ABI's
    assert (nsd.FLOW_DTYPE.itemsize, nsd.FLOWT_DTYPE.itemsize) == (nsd.FLOW_BYTES, nsd.FLOWT_BYTES) == (72, 88)
    assert (nsd.CONV_DTYPE.itemsize, nsd.CONVT_DTYPE.itemsize) == (nsd.CONV_BYTES, nsd.CONVT_BYTES) == (88, 104)
