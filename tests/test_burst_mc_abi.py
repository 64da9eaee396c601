"""CPU: the device key table and the multi-connection burst calls
(include/net2/packet.h: net2_burst_keytab_*, net2_packet_*_burst_mc) are
exported and bound, and their argument checks come before the device check,
as check_burst_args' do.  No kernel is launched here."""
import ctypes
import errno

from ilias_net2_amd import _lib

NAMES = ("net2_burst_keytab_create", "net2_burst_keytab_destroy",
         "net2_burst_keytab_set_rx", "net2_burst_keytab_set_tx",
         "net2_burst_keytab_clear", "net2_packet_decode_burst_mc",
         "net2_packet_encode_burst_mc")


def test_symbols_exported_and_bound():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        fn = getattr(L, name)
        res, args = _lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_keytab_create_argument_errors_precede_the_device_check():
    L = _lib.lib()
    tab = ctypes.c_void_p(0x1234)
    # an unkeyed row, the nil row, a row past the registry, no slots
    for alg, slots in ((_lib.SHA512, 4), (_lib.NIL, 4), (7, 4), (-1, 4),
                       (_lib.HMAC_SHA512, 0)):
        assert L.net2_burst_keytab_create(alg, slots, ctypes.byref(tab)) == errno.EINVAL
        assert not tab.value          # and no table is handed out
        tab.value = 0x1234
    assert L.net2_burst_keytab_create(_lib.HMAC_SHA256, 4, None) == errno.EINVAL
    # a well-formed request reaches the device check (or a device)
    rc = L.net2_burst_keytab_create(_lib.HMAC_SHA256, 4, ctypes.byref(tab))
    if _lib.device_count() == 0:
        assert rc == errno.ENODEV and not tab.value
    else:
        assert rc == 0 and tab.value
        L.net2_burst_keytab_destroy(tab)


def test_null_table_is_einval():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert L.net2_packet_decode_burst_mc(None, p, 16, p, p, p, 1, p, p, p, p, p,
                                         4096, None) == errno.EINVAL
    assert L.net2_packet_encode_burst_mc(None, p, p, p, p, p, p, 1, p, p, 4096,
                                         None) == errno.EINVAL
    key = b"k" * 64
    keys = _lib.BurstRxKeys(6, ctypes.cast(ctypes.c_char_p(key), ctypes.c_void_p),
                            64, 1, None, 0, 0, 0, 0)
    assert L.net2_burst_keytab_set_rx(None, 0, ctypes.byref(keys), None) == errno.EINVAL
    assert L.net2_burst_keytab_set_tx(None, 0, key, 64, 1, None) == errno.EINVAL
    assert L.net2_burst_keytab_clear(None, 0, None) == errno.EINVAL
    L.net2_burst_keytab_destroy(None)         # a no-op


def test_noconn_code_is_declared():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "net2", "packet.h")).read()
    assert "#define NET2_PBURST_NOCONN\t5" in hdr
    from ilias_net2_amd import conn_burst
    assert conn_burst.NOCONN == 5
