"""CPU: the C ABI of the keyed hash bursts' witness -- net2_sha2_burst_stats
(launches by form: one datagram per lane, or the one-launch small-burst form,
which the _mc calls now take too) is declared in include/net2/packet.h beside
net2_sha2_burst_limits, exported, bound by _lib, and is host state: it needs
no device.  No kernel is launched here."""
import ctypes
import os
import re
import subprocess
import sys

from ilias_net2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "net2_sha2_burst_stats"


def test_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "net2", "packet.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"\bint\s+net2_sha2_burst_stats\s*\(\s*uint64_t\s*\*\s*lane_launches"
                     r"\s*,\s*uint64_t\s*\*\s*wave_launches\s*\)\s*;", src)
    assert decl
    # beside net2_sha2_burst_limits: the next declaration after it
    lim = re.search(r"\bint\s+net2_sha2_burst_limits\s*\([^)]*\)\s*;", src)
    assert lim and src[lim.end():decl.start()].strip() == ""
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, NAME)
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    assert _lib.lib().net2_sha2_burst_stats.argtypes == args


def test_a_build_without_it_is_refused(tmp_path):
    """bind() refuses a library that lacks the entry point."""
    import pytest
    src = tmp_path / "old.c"
    src.write_text("".join(f"int {n}(void) {{ return 1; }}\n"
                           for n in _lib.SIGNATURES if n != NAME))
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    with pytest.raises(ImportError) as ei:
        _lib.bind(ctypes.CDLL(str(so)))
    assert NAME in str(ei.value)


def test_null_pointers_and_the_python_wrapper():
    from ilias_net2_amd import conn_burst
    L = _lib.lib()
    lane, wave = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.net2_sha2_burst_stats(None, None) == 0
    assert L.net2_sha2_burst_stats(ctypes.byref(lane), None) == 0
    assert L.net2_sha2_burst_stats(None, ctypes.byref(wave)) == 0
    assert conn_burst.burst_stats() == (lane.value, wave.value)
    # the limits change nothing that is counted
    try:
        assert L.net2_sha2_burst_limits(1 << 30, 0) == 0
        assert conn_burst.burst_stats() == (lane.value, wave.value)
    finally:
        L.net2_sha2_burst_limits(-1, -1)


def test_no_device_needed_and_starts_at_zero():
    """A process that sees no device and has launched nothing counts
    nothing, whatever it set: the library loaded in a child of its own, every
    device hidden from it."""
    code = (
        "import ctypes, sys\n"
        "L = ctypes.CDLL(sys.argv[1])\n"
        "L.net2_sha2_burst_limits.argtypes = [ctypes.c_int64, ctypes.c_int64]\n"
        "a, b = ctypes.c_uint64(9), ctypes.c_uint64(9)\n"
        "rc = [L.net2_sha2_burst_limits(1 << 30, -1), L.net2_sha2_burst_limits(-1, -1),\n"
        "      L.net2_sha2_burst_stats(None, None),\n"
        "      L.net2_sha2_burst_stats(ctypes.byref(a), ctypes.byref(b))]\n"
        "print('STATS', rc, a.value, b.value)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH], env=env,
                       capture_output=True, text=True, timeout=300)
    assert "STATS [0, 0, 0, 0] 0 0" in r.stdout, r.stdout + r.stderr
