"""CPU: the C ABI of the encrypt bursts' two forms -- net2_aes_encrypt_limits
(the size threshold between four lanes and one lane per datagram) and
net2_aes_encrypt_stats (launches by form) are declared in
include/net2/packet.h, exported, bound by _lib, and are host state: they need
no device.  No kernel is launched here."""
import ctypes
import os
import re
import subprocess
import sys

from ilias_net2_amd import _lib, cipher_burst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("net2_aes_encrypt_limits", "net2_aes_encrypt_stats")


def test_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "net2", "packet.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+net2_aes_encrypt_limits\s*\(\s*int64_t\s+quad_max\s*\)\s*;",
                     src)
    assert re.search(r"\bint\s+net2_aes_encrypt_stats\s*\(\s*uint64_t\s*\*\s*lane_launches"
                     r"\s*,\s*uint64_t\s*\*\s*quad_launches\s*\)\s*;", src)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["net2_aes_encrypt_limits"] == (ctypes.c_int, [ctypes.c_int64])
    res, args = _lib.SIGNATURES["net2_aes_encrypt_stats"]
    assert res is ctypes.c_int and len(args) == 2
    assert all(a is ctypes.POINTER(ctypes.c_uint64) for a in args)


def test_a_build_without_them_is_refused(tmp_path):
    """bind() refuses a library that lacks the two entry points."""
    import pytest
    src = tmp_path / "old.c"
    src.write_text("".join(f"int {n}(void) {{ return 1; }}\n"
                           for n in _lib.SIGNATURES if n not in NAMES))
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    with pytest.raises(ImportError) as ei:
        _lib.bind(ctypes.CDLL(str(so)))
    assert all(n in str(ei.value) for n in NAMES)


def test_limits_need_no_device_and_always_return_zero():
    L = _lib.lib()
    try:
        for v in (0, 1, 1 << 30, (1 << 63) - 1, -1, -(1 << 63)):
            assert L.net2_aes_encrypt_limits(v) == 0, v
        assert cipher_burst.encrypt_limits(0) is None
    finally:
        L.net2_aes_encrypt_limits(-1)
    # either pointer may be NULL
    lane, quad = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.net2_aes_encrypt_stats(None, None) == 0
    assert L.net2_aes_encrypt_stats(ctypes.byref(lane), None) == 0
    assert L.net2_aes_encrypt_stats(None, ctypes.byref(quad)) == 0
    assert set(cipher_burst.encrypt_stats()) == {"lane_launches", "quad_launches"}
    assert cipher_burst.encrypt_stats() == {"lane_launches": lane.value,
                                            "quad_launches": quad.value}
    # the decrypt bursts' calls keep their two counters
    assert set(cipher_burst.stats()) == {"lane_launches", "wave_launches"}


def test_stats_start_at_zero():
    """A process that has launched nothing counts nothing, whatever it set:
    the library loaded in a child of its own."""
    code = (
        "import ctypes, sys\n"
        "L = ctypes.CDLL(sys.argv[1])\n"
        "L.net2_aes_encrypt_limits.argtypes = [ctypes.c_int64]\n"
        "a, b = ctypes.c_uint64(9), ctypes.c_uint64(9)\n"
        "rc = [L.net2_aes_encrypt_limits(1 << 30), L.net2_aes_encrypt_limits(-1),\n"
        "      L.net2_aes_encrypt_stats(ctypes.byref(a), ctypes.byref(b))]\n"
        "print('STATS', rc, a.value, b.value)\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH],
                       capture_output=True, text=True, timeout=300)
    assert "STATS [0, 0, 0] 0 0" in r.stdout, r.stdout + r.stderr
