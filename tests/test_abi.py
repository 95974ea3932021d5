"""CPU-side checks of the drop-in boundary: libdeft4g.so loads, exports every symbol include/deft4g.h
declares, and refuses to work without a GPU (no CPU fallback)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import deft4j_amd
    return deft4j_amd.load_library()


def test_header_symbols_are_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "deft4g.h")).read()
    names = sorted(set(re.findall(r"\b(d4g_[a-z_0-9]+)\s*\(", hdr)))
    assert len(names) >= 14
    for n in names:
        assert getattr(lib, n) is not None, n
    import deft4j_amd
    assert sorted(deft4j_amd.EXPORTS) == names


def test_no_cpu_fallback_without_a_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import deft4j_amd
    rc = lib.d4g_init(0)
    assert rc < 0
    assert b"no CPU fallback" in lib.d4g_last_error() or b"device" in lib.d4g_last_error()
    with pytest.raises(RuntimeError):
        deft4j_amd.Deft.optimiseDeflateStream(b"\x03\x00")
    with pytest.raises(RuntimeError):
        deft4j_amd.zopfli_streams([b"abc"], 3)           # the Zopfli encoder has no CPU path either
    # the raw entry points also refuse
    arr = (ctypes.c_char_p * 1)(b"\x03\x00")
    lens = (ctypes.c_size_t * 1)(2)
    assert not lib.d4g_batch_create(1, arr, lens)


def test_product_library_does_not_link_the_oracle():
    out = os.popen("nm -D --defined-only %s" % os.path.join(ROOT, "deft4j_amd", "libdeft4g.so")).read()
    assert "oracle_" not in out
    src = "".join(open(os.path.join(ROOT, "deft4j_amd", "csrc", f)).read() for f in os.listdir(os.path.join(ROOT, "deft4j_amd", "csrc")))
    assert "oracle" not in src.lower() or "deft_oracle" not in src
    py = open(os.path.join(ROOT, "deft4j_amd", "__init__.py")).read() + open(os.path.join(ROOT, "deft4j_amd", "shard.py")).read()
    assert "oracle" not in py


def test_jni_shim_and_java_binding_match_the_header():
    """jni/deft4g_jni.c and java/.../NativeDeft.java cannot be compiled here (no JDK), so keep them honest textually:
    every d4g_ function the shim calls is declared in include/deft4g.h, and every native method of NativeDeft has its
    Java_..._NativeDeft_<name> definition in the shim."""
    hdr = open(os.path.join(ROOT, "include", "deft4g.h")).read()
    shim = open(os.path.join(ROOT, "jni", "deft4g_jni.c")).read()
    java = open(os.path.join(ROOT, "java", "com", "github", "NeRdTheNed", "deft4j", "NativeDeft.java")).read()
    declared = set(re.findall(r"\b(d4g_[a-z_0-9]+)\s*\(", hdr))
    for f in set(re.findall(r"\b(d4g_[a-z_0-9]+)\s*\(", shim)):
        assert f in declared, f
    natives = re.findall(r"native\s+[\w\[\]]+\s+(\w+)\s*\(", java)
    assert len(natives) >= 6
    for m in natives:
        assert "JFN(%s)" % m in shim, m


def test_device_entry_points_refuse_before_init(lib):
    """d4g_init never succeeds without a GPU.  Every entry point that needs the device and takes no batch (and those that
    take one, given NULL: the library check comes first) returns D4G_ERR_NODEVICE with its message, the batch creators a
    NULL batch; the one-shot calls leave their result arrays "unchanged" (deft4g.h)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import abi_calls
    from deft4j_amd import d4g_encoder_spec, d4g_encoder_spec_level
    lib.d4g_debug_fused_stats.restype = ctypes.c_int
    lib.d4g_debug_fused_stats.argtypes = [ctypes.c_void_p]
    data = [b"\x03\x00", b"abc"]
    n = len(data)
    arr = (ctypes.c_char_p * n)(*data)
    lens = (ctypes.c_size_t * n)(*map(len, data))
    spec = (d4g_encoder_spec * 1)(d4g_encoder_spec(0, 0, 0))
    spec_level = (d4g_encoder_spec_level * 1)(d4g_encoder_spec_level(0, 0, 0, 6))
    nodevice = b"d4g_init has not succeeded"

    def refused(call, want=nodevice):
        assert lib.d4g_batch_stats(None, None) == -2          # some other message first
        rc = call()
        assert lib.d4g_last_error() == want
        return rc

    assert refused(lambda: lib.d4g_batch_create(n, arr, lens)) is None
    assert refused(lambda: lib.d4g_batch_create_encode(n, arr, lens, 1, spec)) is None
    assert refused(lambda: lib.d4g_batch_create_encode_level(n, arr, lens, 1, spec_level)) is None
    assert refused(lambda: lib.d4g_batch_create_on(0, n, arr, lens), b"no such context (d4g_init_devices)") is None
    for name, (call, slots, check) in abi_calls.one_shot_calls(lib, data).items():
        assert refused(call) == -1, name
        assert slots.unchanged(**check), name
    out, olen, consumed, status, bits = ctypes.c_void_p(0xdead), ctypes.c_size_t(777), ctypes.c_size_t(0), ctypes.c_int32(99), ctypes.c_int64(0)
    assert refused(lambda: lib.d4g_inflate(data[0], 2, ctypes.byref(out), ctypes.byref(olen), ctypes.byref(consumed), ctypes.byref(status))) == -1
    assert out.value is None and olen.value == 0
    assert refused(lambda: lib.d4g_size_bits_fallback(data[0], 2, ctypes.byref(bits))) == -1
    u16 = (ctypes.c_uint16 * 8)()
    u32 = (ctypes.c_uint32 * 19)(*range(19))
    i32 = (ctypes.c_int32 * 1)()
    assert refused(lambda: lib.d4g_debug_zopfli_table(b"abc", 3, 0, u16, u16, None)) == -1
    assert refused(lambda: lib.d4g_debug_zopfli_code_lengths(u32, 4, 15, u32)) == -1
    assert refused(lambda: lib.d4g_debug_cl_tree_lengths(u32, 1, u32, i32)) == -1
    assert refused(lambda: abi_calls.pack_header_call(lib)) == -1
    assert refused(lambda: lib.d4g_debug_fused_stats((ctypes.c_int64 * 64)())) == -1
    assert refused(lambda: lib.d4g_batch_run(None, 1)) == -1
    assert refused(lambda: lib.d4g_batch_run_encode(None, 0, 0)) == -1
    assert refused(lambda: lib.d4g_batch_parse(None)) == -1
    assert refused(lambda: lib.d4g_batch_run_recompress(None, 1, 20, 1)) == -1
