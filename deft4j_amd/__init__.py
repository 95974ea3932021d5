"""deft4j_amd — host-side mirror of deft4j's optimiser API over libdeft4g.so (HIP, gfx950).

The Java reference (NeRdTheNed/deft4j) exposes
    Deft.optimiseDeflateStream(byte[], boolean)            B/Deft.java:21-34
    Deft.getSizeBitsFallback(byte[])                       B/Deft.java:48-54
    DeflateStream.parse / optimise / getSizeBits / getUncompressedData / asBytes
                                                           B/deflate/DeflateStream.java:68-182,496,652
    DeflateFilesContainer.optimise(List<DeflateStream>, boolean)   K/DeflateFilesContainer.java:18-43
(B/ = deft4j-base/src/main/java/com/github/NeRdTheNed/deft4j/, K/ = deft4j-container/...).
This module keeps those names, argument meanings and the "fall back to the original bytes"
error behaviour, and forwards every call to the C ABI declared in include/deft4g.h.  There
is no CPU path here: importing works anywhere, but any call raises RuntimeError unless the
HIP library is built and a GPU is present.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdeft4g.so")

_lib = None
_ready = False


class d4g_stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("ms_upload", "ms_parse", "ms_optimise", "ms_merge", "ms_write", "ms_total")] + \
               [(n, ctypes.c_int64) for n in ("n_streams", "n_blocks", "n_tokens", "bytes_in", "bytes_decoded", "bytes_out",
                                              "rounds", "kernel_launches", "search_bytes_algorithmic")] + \
               [("ms_search_kernels", ctypes.c_double), ("ms_parse_kernels", ctypes.c_double)] + \
               [(n, ctypes.c_int64) for n in ("scan_candidates", "scan_confirmed", "exact_probes", "jump_rounds")] + \
               [("ms_state_kernels", ctypes.c_double), ("state_launches", ctypes.c_int64), ("state_tokens_per_round", ctypes.c_int64),
                ("state_bytes_per_round", ctypes.c_int64), ("search_lanes", ctypes.c_int64), ("ms_checksum_kernels", ctypes.c_double),
                ("ms_lz_sort", ctypes.c_double), ("ms_lz_parse", ctypes.c_double), ("ms_lz_emit", ctypes.c_double),
                ("lz_parse_passes", ctypes.c_int64), ("lz_chunks_rerun", ctypes.c_int64), ("lz_symbols", ctypes.c_int64),
                ("ms_recompress_encode", ctypes.c_double), ("ms_recompress_encode_front", ctypes.c_double),
                ("ms_recompress_encode_search", ctypes.c_double), ("ms_recompress_reoptimise", ctypes.c_double),
                ("recompress_outputs", ctypes.c_int64), ("recompress_outputs_pruned", ctypes.c_int64),
                ("ms_zopfli_table", ctypes.c_double), ("ms_zopfli_split", ctypes.c_double), ("ms_zopfli_squeeze", ctypes.c_double),
                ("ms_zopfli_emit", ctypes.c_double), ("zopfli_blocks", ctypes.c_int64), ("zopfli_position_iterations", ctypes.c_int64),
                ("rounds_fused", ctypes.c_int64), ("fused_fallbacks", ctypes.c_int64), ("rounds_cluster", ctypes.c_int64),
                ("ms_verify", ctypes.c_double), ("ms_verify_kernels", ctypes.c_double), ("verify_streams", ctypes.c_int64), ("verify_bytes", ctypes.c_int64),
                ("copy_segments", ctypes.c_int64), ("copy_rounds", ctypes.c_int64),
                ("recover_streams", ctypes.c_int64), ("recover_bytes", ctypes.c_int64), ("ms_recover", ctypes.c_double),
                ("ms_recover_kernels", ctypes.c_double),
                ("fused_fallbacks_mid", ctypes.c_int64), ("fused_relaunches", ctypes.c_int64), ("cluster_fallbacks", ctypes.c_int64),
                ("scan_kept", ctypes.c_int64), ("dict_streams", ctypes.c_int64), ("dict_bytes", ctypes.c_int64)]


class d4g_encoder_spec(ctypes.Structure):
    _fields_ = [("input", ctypes.c_int32), ("encoder", ctypes.c_int32), ("strategy", ctypes.c_int32)]


class d4g_encoder_spec_level(ctypes.Structure):
    _fields_ = [("input", ctypes.c_int32), ("encoder", ctypes.c_int32), ("strategy", ctypes.c_int32), ("level", ctypes.c_int32)]


class d4g_block_info(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int32), ("bfinal", ctypes.c_int32)] + \
               [(n, ctypes.c_int64) for n in ("bit_pos", "size_bits", "header_bits", "tokens", "decoded_len")]


class d4g_found_stream(ctypes.Structure):
    _fields_ = [("file", ctypes.c_int32), ("kind", ctypes.c_int32)] + \
               [(n, ctypes.c_int64) for n in ("offset", "payload_offset", "payload_len", "total_len", "decoded_len", "size_bits")] + \
               [("crc32", ctypes.c_uint32), ("adler32", ctypes.c_uint32), ("n_blocks", ctypes.c_int32), ("dictionary", ctypes.c_int32)]


class d4g_find_options(ctypes.Structure):
    _fields_ = [("kinds", ctypes.c_int32), ("reserved", ctypes.c_int32), ("min_decoded", ctypes.c_int64)]


class d4g_find_stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("bytes_scanned", "header_candidates", "first_block_ok", "parsed", "confirmed", "reported",
                                              "kernel_launches")] + [("ms_total", ctypes.c_double), ("ms_kernels", ctypes.c_double)]


FOUND_ZLIB, FOUND_GZIP = 1, 2                               # D4G_FOUND_*
FOUND_KIND_NAMES = {1: "zlib", 2: "gzip"}


class d4g_parse_error(ctypes.Structure):
    _fields_ = [("reason", ctypes.c_int32), ("block", ctypes.c_int32)] + \
               [(n, ctypes.c_int64) for n in ("block_bit_pos", "bit_pos", "decoded_offset", "value")]


# D4G_PARSE_*: why a stream did not parse (d4g_batch_parse_error)
PARSE_OK, PARSE_EOF, PARSE_BLOCK_TYPE, PARSE_STORED_LENGTHS, PARSE_CODE_LENGTHS, PARSE_LITLEN_SYMBOL, PARSE_DIST_SYMBOL, \
    PARSE_DISTANCE_TOO_FAR = range(8)
PARSE_REASON_NAMES = {0: "OK", 1: "EOF", 2: "BLOCK_TYPE", 3: "STORED_LENGTHS", 4: "CODE_LENGTHS", 5: "LITLEN_SYMBOL", 6: "DIST_SYMBOL",
                      7: "DISTANCE_TOO_FAR"}

VERIFY_OK, VERIFY_SKIPPED, VERIFY_PARSE, VERIFY_SIZE, VERIFY_LENGTH, VERIFY_BYTES = 0, 1, -1, -2, -3, -4     # D4G_VERIFY_*
VERDICT_NAMES = {0: "OK", 1: "SKIPPED", -1: "PARSE", -2: "SIZE", -3: "LENGTH", -4: "BYTES"}
BLOCK_TYPE_NAMES = ("STORED", "FIXED", "DYNAMIC")           # DeflateBlockType, as printBlockInfo prints it

ENC_JVM, ENC_JZLIB = 0, 1                                   # D4G_ENC_*: JavaCompressor / JZLibCompressor
STRATEGY_DEFAULT, STRATEGY_FILTERED, STRATEGY_HUFFMAN_ONLY = 0, 1, 2
STRATEGY_RLE, STRATEGY_FIXED = 3, 4                         # zlib's Z_RLE / Z_FIXED (the level entry points only)

EXPORTS = ["d4g_init", "d4g_shutdown", "d4g_last_error", "d4g_batch_create", "d4g_batch_run", "d4g_batch_stream_result",
           "d4g_batch_copy_output", "d4g_batch_copy_decoded", "d4g_batch_checksums", "d4g_batch_parse", "d4g_batch_stats", "d4g_batch_destroy", "d4g_optimise_streams",
           "d4g_size_bits_fallback", "d4g_inflate", "d4g_free", "d4g_batch_create_encode", "d4g_batch_run_encode", "d4g_deflate_streams",
           "d4g_compress", "d4g_recompress_streams", "d4g_batch_run_recompress", "d4g_batch_recompress_result", "d4g_zopfli_streams",
           "d4g_debug_zopfli_table", "d4g_debug_zopfli_code_lengths", "d4g_debug_cl_tree_lengths", "d4g_debug_pack_header", "d4g_init_devices", "d4g_device_count", "d4g_set_device",
           "d4g_batch_create_on", "d4g_optimise_streams_sharded", "d4g_batch_create_encode_level", "d4g_deflate_streams_level",
           "d4g_batch_verify", "d4g_batch_verify_result", "d4g_verify_streams", "d4g_debug_batch_poke_output", "d4g_batch_block_info", "d4g_debug_verify_compare",
           "d4g_debug_device_blocks", "d4g_debug_batch_bins", "d4g_batch_parse_error", "d4g_diagnose_streams", "d4g_parse_reason_name",
           "d4g_find_streams", "d4g_batch_recover", "d4g_batch_copy_recovered", "d4g_recover_streams",
           "d4g_batch_create_dict", "d4g_batch_create_dict_on", "d4g_inflate_dict", "d4g_find_streams_dict",
           "d4g_batch_create_encode_dict", "d4g_deflate_streams_dict"]


def load_library(path=None):
    """Load libdeft4g.so and declare the prototypes of include/deft4g.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("D4G_LIB") or LIB_PATH   # D4G_LIB: development builds of the same library
    if not os.path.exists(p):
        raise RuntimeError("libdeft4g.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'`; "
                           "there is no CPU fallback" % p)
    L = ctypes.CDLL(p)
    L.d4g_init.restype = ctypes.c_int
    L.d4g_init.argtypes = [ctypes.c_int]
    L.d4g_shutdown.restype = None
    L.d4g_last_error.restype = ctypes.c_char_p
    L.d4g_batch_create.restype = ctypes.c_void_p
    L.d4g_batch_create.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t)]
    L.d4g_batch_run.restype = ctypes.c_int
    L.d4g_batch_run.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.d4g_batch_stream_result.restype = ctypes.c_int
    L.d4g_batch_stream_result.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32),
                                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_size_t),
                                          ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int64)]
    L.d4g_batch_copy_output.restype = ctypes.c_int
    L.d4g_batch_copy_output.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    L.d4g_batch_copy_decoded.restype = ctypes.c_int
    L.d4g_batch_copy_decoded.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.POINTER(ctypes.c_size_t)]
    L.d4g_batch_checksums.restype = ctypes.c_int
    L.d4g_batch_checksums.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                      ctypes.POINTER(ctypes.c_int64)]
    L.d4g_batch_parse.restype = ctypes.c_int
    L.d4g_batch_parse.argtypes = [ctypes.c_void_p]
    L.d4g_batch_stats.restype = ctypes.c_int
    L.d4g_batch_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(d4g_stats)]
    L.d4g_batch_destroy.restype = None
    L.d4g_batch_destroy.argtypes = [ctypes.c_void_p]
    L.d4g_free.restype = None
    L.d4g_free.argtypes = [ctypes.c_void_p]
    L.d4g_optimise_streams.restype = ctypes.c_int
    L.d4g_optimise_streams.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                       ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)]
    L.d4g_size_bits_fallback.restype = ctypes.c_int
    L.d4g_size_bits_fallback.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64)]
    L.d4g_inflate.restype = ctypes.c_int
    L.d4g_inflate.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p),
                              ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t),
                              ctypes.POINTER(ctypes.c_int32)]
    L.d4g_batch_create_encode.restype = ctypes.c_void_p
    L.d4g_batch_create_encode.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                                          ctypes.POINTER(d4g_encoder_spec)]
    L.d4g_batch_run_encode.restype = ctypes.c_int
    L.d4g_batch_run_encode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.d4g_deflate_streams.restype = ctypes.c_int
    L.d4g_deflate_streams.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    L.d4g_batch_create_encode_level.restype = ctypes.c_void_p
    L.d4g_batch_create_encode_level.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                                                ctypes.POINTER(d4g_encoder_spec_level)]
    L.d4g_deflate_streams_level.restype = ctypes.c_int
    L.d4g_deflate_streams_level.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    L.d4g_zopfli_streams.restype = ctypes.c_int
    L.d4g_zopfli_streams.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    L.d4g_debug_zopfli_table.restype = ctypes.c_int
    L.d4g_debug_zopfli_table.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.d4g_debug_zopfli_code_lengths.restype = ctypes.c_int
    L.d4g_debug_zopfli_code_lengths.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]
    L.d4g_debug_cl_tree_lengths.restype = ctypes.c_int
    L.d4g_debug_cl_tree_lengths.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    # (d4g_debug_pack_header, a test hook, gets its prototype where the tests call it — tests/abi_calls.py: a build of the
    # library from before the hook existed, as an A/B series loads through D4G_LIB, has no such symbol to declare)
    L.d4g_compress.restype = ctypes.c_int
    L.d4g_compress.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                               ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32)]
    L.d4g_batch_run_recompress.restype = ctypes.c_int
    L.d4g_batch_run_recompress.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.d4g_batch_recompress_result.restype = ctypes.c_int
    L.d4g_batch_recompress_result.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)]
    L.d4g_recompress_streams.restype = ctypes.c_int
    L.d4g_recompress_streams.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                         ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)]
    L.d4g_init_devices.restype = ctypes.c_int
    L.d4g_init_devices.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.d4g_device_count.restype = ctypes.c_int
    L.d4g_set_device.restype = ctypes.c_int
    L.d4g_set_device.argtypes = [ctypes.c_int]
    L.d4g_batch_create_on.restype = ctypes.c_void_p
    L.d4g_batch_create_on.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t)]
    L.d4g_optimise_streams_sharded.restype = ctypes.c_int
    L.d4g_optimise_streams_sharded.argtypes = L.d4g_optimise_streams.argtypes
    L.d4g_batch_verify.restype = ctypes.c_int
    L.d4g_batch_verify.argtypes = [ctypes.c_void_p]
    L.d4g_batch_verify_result.restype = ctypes.c_int
    L.d4g_batch_verify_result.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)]
    L.d4g_verify_streams.restype = ctypes.c_int
    L.d4g_verify_streams.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_char_p),
                                     ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)]
    L.d4g_debug_batch_poke_output.restype = ctypes.c_int
    L.d4g_debug_batch_poke_output.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint8]
    L.d4g_debug_verify_compare.restype = ctypes.c_int
    L.d4g_debug_verify_compare.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64)]
    L.d4g_debug_device_blocks.restype = ctypes.c_int
    L.d4g_debug_device_blocks.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    L.d4g_batch_block_info.restype = ctypes.c_int
    L.d4g_batch_block_info.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(d4g_block_info), ctypes.c_size_t,
                                       ctypes.POINTER(ctypes.c_size_t)]
    L.d4g_batch_parse_error.restype = ctypes.c_int
    L.d4g_batch_parse_error.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(d4g_parse_error)]
    L.d4g_diagnose_streams.restype = ctypes.c_int
    L.d4g_diagnose_streams.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(d4g_parse_error)]
    L.d4g_parse_reason_name.restype = ctypes.c_char_p
    L.d4g_parse_reason_name.argtypes = [ctypes.c_int]
    L.d4g_find_streams.restype = ctypes.c_int
    L.d4g_find_streams.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(d4g_find_options),
                                   ctypes.POINTER(ctypes.POINTER(d4g_found_stream)), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(d4g_find_stats)]
    L.d4g_batch_recover.restype = ctypes.c_int
    L.d4g_batch_recover.argtypes = [ctypes.c_void_p]
    L.d4g_batch_copy_recovered.restype = ctypes.c_int
    L.d4g_batch_copy_recovered.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.d4g_recover_streams.restype = ctypes.c_int
    L.d4g_recover_streams.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(d4g_parse_error)]
    if hasattr(L, "d4g_batch_create_dict"):   # (preset dictionaries: a build from before them, loaded through D4G_LIB, has no such symbols)
        dict_args = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32)]
        L.d4g_batch_create_dict.restype = ctypes.c_void_p
        L.d4g_batch_create_dict.argtypes = L.d4g_batch_create.argtypes + dict_args
        L.d4g_batch_create_dict_on.restype = ctypes.c_void_p
        L.d4g_batch_create_dict_on.argtypes = L.d4g_batch_create_on.argtypes + dict_args
        L.d4g_inflate_dict.restype = ctypes.c_int
        L.d4g_inflate_dict.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p),
                                       ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32)]
        L.d4g_find_streams_dict.restype = ctypes.c_int
        L.d4g_find_streams_dict.argtypes = L.d4g_find_streams.argtypes[:4] + dict_args[:3] + L.d4g_find_streams.argtypes[4:]
    if hasattr(L, "d4g_batch_create_encode_dict"):   # (the encoder's preset dictionaries: likewise)
        dict_args = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32)]
        L.d4g_batch_create_encode_dict.restype = ctypes.c_void_p
        L.d4g_batch_create_encode_dict.argtypes = L.d4g_batch_create_encode_level.argtypes[:3] + dict_args + L.d4g_batch_create_encode_level.argtypes[3:]
        L.d4g_deflate_streams_dict.restype = ctypes.c_int
        L.d4g_deflate_streams_dict.argtypes = L.d4g_deflate_streams_level.argtypes[:6] + dict_args + L.d4g_deflate_streams_level.argtypes[6:]
    if path is None:
        _lib = L
    return L


def init(device_index=None, lib=None):
    """d4g_init: one process per GPU.  Defaults to LOCAL_RANK (torch.distributed launch) or 0."""
    global _ready
    L = lib or load_library()
    if device_index is None:
        device_index = int(os.environ.get("LOCAL_RANK", "0"))
    rc = L.d4g_init(device_index)
    if rc != 0:
        raise RuntimeError("d4g_init(%d) failed: %s" % (device_index, L.d4g_last_error().decode()))
    if lib is None:
        _ready = True
    return L


def init_devices(devices, lib=None):
    """d4g_init_devices: one process driving several GPUs — context k = devices[k] (a device may appear twice)."""
    global _ready
    L = lib or load_library()
    arr = (ctypes.c_int * len(devices))(*devices)
    rc = L.d4g_init_devices(len(devices), arr)
    if rc != 0:
        raise RuntimeError("d4g_init_devices(%r) failed: %s" % (list(devices), L.d4g_last_error().decode()))
    if lib is None:
        _ready = True
    return L


def optimise_streams_sharded(streams, merge_blocks=True, lib=None):
    """d4g_optimise_streams_sharded: the list over every initialised context.  -> (outputs, saved_bits, status) with
    outputs[i] = None when stream i keeps its original bytes."""
    L = lib or _need()
    n = len(streams)
    keep = [bytes(s) for s in streams]
    arr = (ctypes.c_char_p * n)(*keep)
    lens = (ctypes.c_size_t * n)(*[len(s) for s in keep])
    out = (ctypes.c_void_p * n)()
    olen = (ctypes.c_size_t * n)()
    saved = (ctypes.c_int64 * n)()
    status = (ctypes.c_int32 * n)()
    rc = L.d4g_optimise_streams_sharded(n, arr, lens, 1 if merge_blocks else 0, out, olen, saved, status)
    if rc != 0:
        raise RuntimeError("d4g_optimise_streams_sharded: " + L.d4g_last_error().decode())
    res = []
    for i in range(n):
        if out[i]:
            res.append(ctypes.string_at(out[i], olen[i]))
            L.d4g_free(out[i])
        else:
            res.append(None)
    return res, list(saved), list(status)


def _need():
    if not _ready:
        init()
    return _lib


def _parse_error_dict(e):
    d = {k: getattr(e, k) for k, _ in d4g_parse_error._fields_}
    d["reason_name"] = PARSE_REASON_NAMES.get(e.reason, "UNKNOWN")
    return d


def _dictionary_args(n, dictionaries, dictionary_of):
    """The preset-dictionary arguments of Batch and its kin -> (dictionaries as a list of bytes, index per stream with -1 for
    none).  `dictionaries` is one bytes object, applied to all n streams, or a list that goes with `dictionary_of`: per stream
    an index into it, or None."""
    if isinstance(dictionaries, (bytes, bytearray, memoryview)):
        if dictionary_of is not None:
            raise ValueError("dictionary_of goes with a list of dictionaries")
        return [bytes(dictionaries)], [0] * n
    dicts = [bytes(d) for d in dictionaries]
    if dictionary_of is None:
        raise ValueError("a list of dictionaries needs dictionary_of: per stream an index into it, or None")
    if len(dictionary_of) != n:
        raise ValueError("dictionary_of has one entry per stream")
    return dicts, [-1 if k is None else int(k) for k in dictionary_of]


def _dictionary_arrays(dicts):
    nd = len(dicts)
    return (ctypes.c_char_p * max(1, nd))(*dicts), (ctypes.c_size_t * max(1, nd))(*[len(d) for d in dicts])


class Batch:
    """A list of independent raw DEFLATE streams resident in HBM (d4g_batch_*).  dictionaries / dictionary_of: the preset
    dictionaries the streams were written against (zlib's zdict=, d4g_batch_create_dict) — one bytes object for all
    streams, or a list and per stream an index into it or None."""

    def __init__(self, streams, lib=None, context=None, dictionaries=None, dictionary_of=None):
        self.L = lib or _need()
        self.n = len(streams)
        self._keep = [bytes(s) for s in streams]
        arr = (ctypes.c_char_p * self.n)(*self._keep)
        lens = (ctypes.c_size_t * self.n)(*[len(s) for s in self._keep])
        what = "d4g_batch_create: "
        if dictionaries is not None:
            dicts, of = _dictionary_args(self.n, dictionaries, dictionary_of)
            darr, dlens = _dictionary_arrays(dicts)
            ofarr = (ctypes.c_int32 * max(1, self.n))(*of)
            what = "d4g_batch_create_dict: "
            if context is None:
                self.h = self.L.d4g_batch_create_dict(self.n, arr, lens, len(dicts), darr, dlens, ofarr)
            else:
                self.h = self.L.d4g_batch_create_dict_on(context, self.n, arr, lens, len(dicts), darr, dlens, ofarr)
        elif dictionary_of is not None:
            raise ValueError("dictionary_of without dictionaries")
        elif context is None:
            self.h = self.L.d4g_batch_create(self.n, arr, lens)
        else:   # d4g_batch_create_on: the batch lives on that context (device) whichever thread calls with it
            self.h = self.L.d4g_batch_create_on(context, self.n, arr, lens)
        if not self.h:
            raise RuntimeError(what + self.L.d4g_last_error().decode())

    def run(self, merge_blocks=True):
        rc = self.L.d4g_batch_run(self.h, 1 if merge_blocks else 0)
        if rc != 0:
            raise RuntimeError("d4g_batch_run: " + self.L.d4g_last_error().decode())
        return self

    def run_recompress(self, mode=1, merge_blocks=True, iter=20):   # noqa: A002
        """CMDUtil.optimise's per-stream loop on the resident streams (d4g_batch_run_recompress)."""
        rc = self.L.d4g_batch_run_recompress(self.h, mode, iter, 1 if merge_blocks else 0)
        if rc != 0:
            raise RuntimeError("d4g_batch_run_recompress: " + self.L.d4g_last_error().decode())
        return self

    def recompress_result(self, i):
        """-> (grafted, recompress_saved_bits)"""
        g = ctypes.c_int32()
        r = ctypes.c_int64()
        self.L.d4g_batch_recompress_result(self.h, i, ctypes.byref(g), ctypes.byref(r))
        return bool(g.value), r.value

    def result(self, i):
        """-> dict(status, saved_bits, out_len, consumed, size_bits_in)"""
        st = ctypes.c_int32()
        sv = ctypes.c_int64()
        ol = ctypes.c_size_t()
        co = ctypes.c_size_t()
        sb = ctypes.c_int64()
        rc = self.L.d4g_batch_stream_result(self.h, i, ctypes.byref(st), ctypes.byref(sv), ctypes.byref(ol),
                                            ctypes.byref(co), ctypes.byref(sb))
        if rc != 0:
            raise RuntimeError(self.L.d4g_last_error().decode())
        return dict(status=st.value, saved_bits=sv.value, out_len=ol.value, consumed=co.value, size_bits_in=sb.value)

    def output(self, i):
        """DeflateStream.asBytes() of stream i (the re-serialised stream, whether or not bits were saved)."""
        r = self.result(i)
        buf = ctypes.create_string_buffer(max(1, r["out_len"]))
        rc = self.L.d4g_batch_copy_output(self.h, i, buf, r["out_len"])
        if rc != 0:
            raise RuntimeError(self.L.d4g_last_error().decode())
        return buf.raw[:r["out_len"]]

    def decoded(self, i):
        n = ctypes.c_size_t()
        rc = self.L.d4g_batch_copy_decoded(self.h, i, None, 0, ctypes.byref(n))
        if rc != 0:
            raise RuntimeError(self.L.d4g_last_error().decode())
        buf = ctypes.create_string_buffer(max(1, n.value))
        rc = self.L.d4g_batch_copy_decoded(self.h, i, buf, n.value, ctypes.byref(n))
        if rc != 0:
            raise RuntimeError(self.L.d4g_last_error().decode())
        return buf.raw[:n.value]

    def parse(self):
        """DeflateStream.parse for every stream (no optimisation); decoded bytes and checksums become available."""
        rc = self.L.d4g_batch_parse(self.h)
        if rc != 0:
            raise RuntimeError("d4g_batch_parse: " + self.L.d4g_last_error().decode())
        return self

    def checksums(self, i):
        """-> (crc32, adler32, isize) of stream i's decoded bytes, computed on the device."""
        c = ctypes.c_uint32()
        a = ctypes.c_uint32()
        n = ctypes.c_int64()
        rc = self.L.d4g_batch_checksums(self.h, i, ctypes.byref(c), ctypes.byref(a), ctypes.byref(n))
        if rc != 0:
            raise RuntimeError(self.L.d4g_last_error().decode())
        return c.value, a.value, n.value

    def verify(self):
        """d4g_batch_verify: every stream the library wrote is parsed again in HBM and its decoded bytes compared on the device
        with the input's.  -> list of {"verdict", "first_mismatch"} (VERIFY_*; see include/deft4g.h)."""
        rc = self.L.d4g_batch_verify(self.h)
        if rc != 0:
            raise RuntimeError("d4g_batch_verify: " + self.L.d4g_last_error().decode())
        res = []
        for i in range(self.n):
            v = ctypes.c_int32()
            f = ctypes.c_int64()
            if self.L.d4g_batch_verify_result(self.h, i, ctypes.byref(v), ctypes.byref(f)) != 0:
                raise RuntimeError(self.L.d4g_last_error().decode())
            res.append({"verdict": v.value, "first_mismatch": f.value})
        return res

    def block_info(self, i, final=False):
        """d4g_batch_block_info -> list of dict(type, bfinal, bit_pos, size_bits, header_bits, tokens, decoded_len), positions and
        sizes as DeflateStream.printBlockInfo counts them."""
        n = ctypes.c_size_t()
        rc = self.L.d4g_batch_block_info(self.h, i, 1 if final else 0, None, 0, ctypes.byref(n))
        if rc != 0:
            raise RuntimeError("d4g_batch_block_info: " + self.L.d4g_last_error().decode())
        arr = (d4g_block_info * max(1, n.value))()
        rc = self.L.d4g_batch_block_info(self.h, i, 1 if final else 0, arr, n.value, ctypes.byref(n))
        if rc != 0:
            raise RuntimeError("d4g_batch_block_info: " + self.L.d4g_last_error().decode())
        return [{k: getattr(arr[j], k) for k, _ in d4g_block_info._fields_} for j in range(n.value)]

    def parse_error(self, i):
        """d4g_batch_parse_error: why stream i did not parse -> dict(reason, reason_name, block, block_bit_pos, bit_pos,
        decoded_offset, value); reason PARSE_OK (and -1 everywhere else) for a stream that parsed."""
        e = d4g_parse_error()
        rc = self.L.d4g_batch_parse_error(self.h, i, ctypes.byref(e))
        if rc != 0:
            raise RuntimeError("d4g_batch_parse_error: " + self.L.d4g_last_error().decode())
        return _parse_error_dict(e)

    def recover(self):
        """d4g_batch_recover: decode what precedes the first failure of every failed stream (once; recovered() asks by itself)."""
        rc = self.L.d4g_batch_recover(self.h)
        if rc != 0:
            raise RuntimeError("d4g_batch_recover: " + self.L.d4g_last_error().decode())
        return self

    def recovered(self, i):
        """d4g_batch_copy_recovered: the bytes of stream i that decode before its first failure — parse_error(i)["decoded_offset"]
        of them; the whole decoded stream where it parsed."""
        n = ctypes.c_size_t()
        rc = self.L.d4g_batch_copy_recovered(self.h, i, None, 0, ctypes.byref(n))
        if rc != 0:
            raise RuntimeError("d4g_batch_copy_recovered: " + self.L.d4g_last_error().decode())
        buf = ctypes.create_string_buffer(max(1, n.value))
        rc = self.L.d4g_batch_copy_recovered(self.h, i, buf, n.value, ctypes.byref(n))
        if rc != 0:
            raise RuntimeError("d4g_batch_copy_recovered: " + self.L.d4g_last_error().decode())
        return buf.raw[:n.value]

    def locate(self, i, offset, final=True):
        """Decoded byte `offset` of stream i -> (block index, byte within that block), by the stream's block list."""
        at = 0
        blocks = self.block_info(i, final)
        for k, b in enumerate(blocks):
            if offset < at + b["decoded_len"]:
                return k, offset - at
            at += b["decoded_len"]
        return len(blocks), offset - at

    def poke_output(self, i, byte_offset, xor_mask):
        """Test hook (d4g_debug_batch_poke_output): flips bits of stream i's final output in HBM."""
        rc = self.L.d4g_debug_batch_poke_output(self.h, i, byte_offset, xor_mask)
        if rc != 0:
            raise RuntimeError("d4g_debug_batch_poke_output: " + self.L.d4g_last_error().decode())

    def debug_bins(self, block):
        """Test hook (d4g_debug_batch_bins): device block `block`'s static bin statistics -> dict(table: 29 rows of 320,
        masks: 29 rows of mask words, records: (x, y, z, w) per back-reference record, n_blocks).  Parses a batch that has not
        run; RuntimeError for a block without a table.  (The prototype is declared here: a build of the library from
        before the hook existed, as an A/B series loads through D4G_LIB, has no such symbol.)"""
        f = self.L.d4g_debug_batch_bins
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                      ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
        mw, nr, nb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        if f(self.h, block, None, None, 0, None, 0, ctypes.byref(mw), ctypes.byref(nr), ctypes.byref(nb)) != 0:
            raise RuntimeError("d4g_debug_batch_bins: " + self.L.d4g_last_error().decode())
        table = (ctypes.c_uint32 * (29 * 320))()
        masks = (ctypes.c_uint64 * max(1, 29 * mw.value))()
        recs = (ctypes.c_uint32 * max(1, 4 * nr.value))()
        if f(self.h, block, table, masks, 29 * mw.value, recs, nr.value, ctypes.byref(mw), ctypes.byref(nr), ctypes.byref(nb)) != 0:
            raise RuntimeError("d4g_debug_batch_bins: " + self.L.d4g_last_error().decode())
        return {"table": [list(table[r * 320:(r + 1) * 320]) for r in range(29)],
                "masks": [list(masks[r * mw.value:(r + 1) * mw.value]) for r in range(29)],
                "records": [tuple(recs[4 * r:4 * r + 4]) for r in range(nr.value)], "n_blocks": nb.value}

    def stats(self):
        st = d4g_stats()
        self.L.d4g_batch_stats(self.h, ctypes.byref(st))
        return {k: getattr(st, k) for k, _ in d4g_stats._fields_}

    def close(self):
        if self.h:
            self.L.d4g_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EncodeBatch(Batch):
    """Streams produced by the LZ77 encoder kernels (d4g_batch_create_encode): one output per (input, encoder, strategy)
    spec — the Compressor objects of C/CompressionUtil.java:44-78.  run(optimise=False) leaves the encoder's output as it
    is (SingleCompressor.compressSingle); optimise=True also applies Deft.optimiseDeflateStream to every output.
    A spec may also be (input, encoder, strategy, level) — zlib levels -1, 1..9 (d4g_batch_create_encode_level); a
    3-tuple next to those means level 9.
    dictionaries / dictionary_of: preset dictionaries of the INPUTS (zlib's zdict=, d4g_batch_create_encode_dict), in
    Batch's convention — one bytes object for all inputs, or a list and per input an index into it or None."""

    def __init__(self, inputs, specs, lib=None, dictionaries=None, dictionary_of=None):  # noqa: super().__init__ deliberately not called: a different constructor
        self.L = lib or _need()
        self.n = len(specs)
        self._keep = [bytes(s) for s in inputs]
        nin = len(self._keep)
        arr = (ctypes.c_char_p * max(1, nin))(*self._keep)
        lens = (ctypes.c_size_t * max(1, nin))(*[len(s) for s in self._keep])
        if dictionaries is not None:
            dicts, of = _dictionary_args(nin, dictionaries, dictionary_of)
            darr, dlens = _dictionary_arrays(dicts)
            ofarr = (ctypes.c_int32 * max(1, nin))(*of)
            sp = (d4g_encoder_spec_level * max(1, self.n))(*[d4g_encoder_spec_level(*(tuple(t) + (9,) * (4 - len(t)))) for t in specs])
            self.h = self.L.d4g_batch_create_encode_dict(nin, arr, lens, len(dicts), darr, dlens, ofarr, self.n, sp)
            what = "d4g_batch_create_encode_dict: "
        elif dictionary_of is not None:
            raise ValueError("dictionary_of without dictionaries")
        elif any(len(t) == 4 for t in specs):
            sp = (d4g_encoder_spec_level * max(1, self.n))(*[d4g_encoder_spec_level(*(tuple(t) + (9,) * (4 - len(t)))) for t in specs])
            self.h = self.L.d4g_batch_create_encode_level(nin, arr, lens, self.n, sp)
            what = "d4g_batch_create_encode_level: "
        else:
            sp = (d4g_encoder_spec * max(1, self.n))(*[d4g_encoder_spec(*t) for t in specs])
            self.h = self.L.d4g_batch_create_encode(nin, arr, lens, self.n, sp)
            what = "d4g_batch_create_encode: "
        if not self.h:
            raise RuntimeError(what + self.L.d4g_last_error().decode())

    def run(self, optimise=False, merge_blocks=True):
        rc = self.L.d4g_batch_run_encode(self.h, 1 if optimise else 0, 1 if merge_blocks else 0)
        if rc != 0:
            raise RuntimeError("d4g_batch_run_encode: " + self.L.d4g_last_error().decode())
        return self


def deflate_streams(inputs, encoder=ENC_JVM, strategy=STRATEGY_DEFAULT, lib=None, level=9, dictionaries=None, dictionary_of=None):
    """SingleCompressor.compressSingle for every input (d4g_deflate_streams); at another zlib level (-1, 1..9) or with
    STRATEGY_RLE / STRATEGY_FIXED through d4g_deflate_streams_level; with preset dictionaries (Batch's convention, per
    input) through d4g_deflate_streams_dict."""
    L = lib or _need()
    n = len(inputs)
    keep = [bytes(s) for s in inputs]
    arr = (ctypes.c_char_p * max(1, n))(*keep)
    lens = (ctypes.c_size_t * max(1, n))(*[len(s) for s in keep])
    out = (ctypes.c_void_p * max(1, n))()
    olen = (ctypes.c_size_t * max(1, n))()
    if dictionaries is not None:
        dicts, of = _dictionary_args(n, dictionaries, dictionary_of)
        darr, dlens = _dictionary_arrays(dicts)
        ofarr = (ctypes.c_int32 * max(1, n))(*of)
        rc = L.d4g_deflate_streams_dict(n, arr, lens, encoder, level, strategy, len(dicts), darr, dlens, ofarr, out, olen)
        what = "d4g_deflate_streams_dict: "
    elif dictionary_of is not None:
        raise ValueError("dictionary_of without dictionaries")
    elif level == 9 and strategy in (STRATEGY_DEFAULT, STRATEGY_FILTERED, STRATEGY_HUFFMAN_ONLY):
        rc, what = L.d4g_deflate_streams(n, arr, lens, encoder, strategy, out, olen), "d4g_deflate_streams: "
    else:
        rc, what = L.d4g_deflate_streams_level(n, arr, lens, encoder, level, strategy, out, olen), "d4g_deflate_streams_level: "
    if rc != 0:
        raise RuntimeError(what + L.d4g_last_error().decode())
    res = []
    for i in range(n):
        res.append(ctypes.string_at(out[i], olen[i]))
        L.d4g_free(out[i])
    return res


def zlib_streams(inputs, level=9, strategy=STRATEGY_DEFAULT, dictionaries=None, dictionary_of=None, lib=None):
    """Complete zlib streams (RFC 1950) of the inputs, as zlib 1.2.11's deflateInit2(level, Z_DEFLATED, 15, 8, strategy) [+
    deflateSetDictionary] writes them: CMF FLG [DICTID] payload ADLER32.  The payload is the encoder's, the trailer the
    device checksum of the batch; FLEVEL follows zlib's rule and DICTID is the Adler-32 of the whole dictionary as passed."""
    import zlib
    n = len(inputs)
    dicts, of = ([], [-1] * n) if dictionaries is None else _dictionary_args(n, dictionaries, dictionary_of)
    if dictionaries is None and dictionary_of is not None:
        raise ValueError("dictionary_of without dictionaries")
    b = EncodeBatch(inputs, [(i, ENC_JVM, strategy, level) for i in range(n)], lib=lib, dictionaries=dictionaries, dictionary_of=dictionary_of)
    try:
        b.run(False)
        lv = 6 if level == -1 else level
        flevel = 0 if (strategy >= STRATEGY_HUFFMAN_ONLY or lv < 2) else 1 if lv < 6 else 2 if lv == 6 else 3
        res = []
        for i in range(n):
            d = dicts[of[i]] if of[i] >= 0 else b""
            head = 0x7800 | (flevel << 6) | (0x20 if d else 0)
            head += 31 - head % 31
            res.append(head.to_bytes(2, "big") + (zlib.adler32(d).to_bytes(4, "big") if d else b"") + b.output(i) +
                       b.checksums(i)[1].to_bytes(4, "big"))
        return res
    finally:
        b.close()


def verify_streams(a, b, lib=None):
    """d4g_verify_streams: do the raw DEFLATE streams a[i] and b[i] decode to the same bytes?  Both sides are parsed and
    compared on the device.  -> list of {"verdict", "first_mismatch"}."""
    L = lib or _need()
    n = len(a)
    if len(b) != n:
        raise ValueError("verify_streams: two lists of the same length")
    ka, kb = [bytes(s) for s in a], [bytes(s) for s in b]
    arr_a = (ctypes.c_char_p * max(1, n))(*ka)
    len_a = (ctypes.c_size_t * max(1, n))(*[len(s) for s in ka])
    arr_b = (ctypes.c_char_p * max(1, n))(*kb)
    len_b = (ctypes.c_size_t * max(1, n))(*[len(s) for s in kb])
    v = (ctypes.c_int32 * max(1, n))()
    f = (ctypes.c_int64 * max(1, n))()
    rc = L.d4g_verify_streams(n, arr_a, len_a, arr_b, len_b, v, f)
    if rc != 0:
        raise RuntimeError("d4g_verify_streams: " + L.d4g_last_error().decode())
    return [{"verdict": v[i], "first_mismatch": f[i]} for i in range(n)]


def diagnose_streams(streams, lib=None, dictionaries=None, dictionary_of=None):
    """d4g_diagnose_streams: parse every raw DEFLATE stream and say where and why it fails -> list of the dicts of
    Batch.parse_error (reason PARSE_OK for the streams that parse).  With preset dictionaries (as Batch takes them) the same
    through a batch of its own."""
    if dictionaries is not None:
        b = Batch(streams, lib=lib, dictionaries=dictionaries, dictionary_of=dictionary_of).parse()
        try:
            return [b.parse_error(i) for i in range(b.n)]
        finally:
            b.close()
    L = lib or _need()
    n = len(streams)
    keep = [bytes(s) for s in streams]
    arr = (ctypes.c_char_p * max(1, n))(*keep)
    lens = (ctypes.c_size_t * max(1, n))(*[len(s) for s in keep])
    out = (d4g_parse_error * max(1, n))()
    rc = L.d4g_diagnose_streams(n, arr, lens, out)
    if rc != 0:
        raise RuntimeError("d4g_diagnose_streams: " + L.d4g_last_error().decode())
    return [_parse_error_dict(out[i]) for i in range(n)]


def recover_streams(streams, lib=None, dictionaries=None, dictionary_of=None):
    """d4g_recover_streams: inflate every raw DEFLATE stream as far as it goes -> list of (bytes, the dict of Batch.parse_error);
    a stream that parses gives all its bytes and reason PARSE_OK, one that does not the decoded_offset bytes before its first
    failure.  With preset dictionaries (as Batch takes them) the same through a batch of its own."""
    if dictionaries is not None:
        b = Batch(streams, lib=lib, dictionaries=dictionaries, dictionary_of=dictionary_of).parse()
        try:
            return [(b.recovered(i), b.parse_error(i)) for i in range(b.n)]
        finally:
            b.close()
    L = lib or _need()
    n = len(streams)
    keep = [bytes(s) for s in streams]
    arr = (ctypes.c_char_p * max(1, n))(*keep)
    lens = (ctypes.c_size_t * max(1, n))(*[len(s) for s in keep])
    out = (ctypes.c_void_p * max(1, n))()
    olen = (ctypes.c_size_t * max(1, n))()
    why = (d4g_parse_error * max(1, n))()
    rc = L.d4g_recover_streams(n, arr, lens, out, olen, why)
    if rc != 0:
        raise RuntimeError("d4g_recover_streams: " + L.d4g_last_error().decode())
    res = []
    for i in range(n):
        res.append((ctypes.string_at(out[i], olen[i]), _parse_error_dict(why[i])))
        L.d4g_free(out[i])
    return res


def inflate(data, dictionary=None, lib=None):
    """d4g_inflate / d4g_inflate_dict: the decoded bytes of one raw DEFLATE stream, optionally written against a preset
    dictionary -> (bytes or None when it does not parse, bytes consumed)."""
    L = lib or _need()
    data = bytes(data)
    out = ctypes.c_void_p()
    ol = ctypes.c_size_t()
    co = ctypes.c_size_t()
    st = ctypes.c_int32()
    if dictionary is None:
        rc = L.d4g_inflate(data, len(data), ctypes.byref(out), ctypes.byref(ol), ctypes.byref(co), ctypes.byref(st))
    else:
        d = bytes(dictionary)
        rc = L.d4g_inflate_dict(data, len(data), d, len(d), ctypes.byref(out), ctypes.byref(ol), ctypes.byref(co), ctypes.byref(st))
    if rc != 0:
        raise RuntimeError("d4g_inflate: " + L.d4g_last_error().decode())
    if st.value < 0:
        return None, co.value
    res = ctypes.string_at(out.value, ol.value)
    L.d4g_free(out)
    return res, co.value


def find_streams(files, kinds=0, min_decoded=0, lib=None, stats=False, dictionaries=None):
    """d4g_find_streams: the zlib and gzip streams embedded in files whose layout is not known (include/deft4g.h states what
    counts as one).  kinds: OR of 1 << FOUND_ZLIB / 1 << FOUND_GZIP, 0 = both.  -> one list per file, in offset order, of
    dict(file, kind, kind_name, offset, payload_offset, payload_len, total_len, decoded_len, size_bits, crc32, adler32,
    n_blocks); with stats=True also the dict of d4g_find_stats.  dictionaries: a list of preset dictionaries
    (d4g_find_streams_dict) — zlib headers with FDICT whose DICTID is the Adler-32 of one of them are streams too, and every
    dict then has a "dictionary" key: the index of the stream's dictionary, or None."""
    L = lib or _need()
    n = len(files)
    keep = [bytes(f) for f in files]
    arr = (ctypes.c_char_p * max(1, n))(*keep)
    lens = (ctypes.c_size_t * max(1, n))(*[len(f) for f in keep])
    opt = d4g_find_options(kinds, 0, min_decoded)
    found = ctypes.POINTER(d4g_found_stream)()
    nf = ctypes.c_size_t()
    st = d4g_find_stats()
    if dictionaries is None:
        rc = L.d4g_find_streams(n, arr, lens, ctypes.byref(opt), ctypes.byref(found), ctypes.byref(nf), ctypes.byref(st))
    else:
        dicts = [bytes(d) for d in dictionaries]
        darr, dlens = _dictionary_arrays(dicts)
        rc = L.d4g_find_streams_dict(n, arr, lens, ctypes.byref(opt), len(dicts), darr, dlens, ctypes.byref(found), ctypes.byref(nf), ctypes.byref(st))
    if rc != 0:
        raise RuntimeError("d4g_find_streams: " + L.d4g_last_error().decode())
    res = [[] for _ in range(n)]
    for k in range(nf.value):
        d = {name: getattr(found[k], name) for name, _ in d4g_found_stream._fields_ if name != "dictionary"}
        if dictionaries is not None:
            d["dictionary"] = found[k].dictionary - 1 if found[k].dictionary > 0 else None
        d["kind_name"] = FOUND_KIND_NAMES.get(d["kind"], "unknown")
        res[d["file"]].append(d)
    if nf.value:
        L.d4g_free(found)
    if stats:
        return res, {name: getattr(st, name) for name, _ in d4g_find_stats._fields_}
    return res


ZOPFLI_SPLIT_FIRST, ZOPFLI_SPLIT_LAST, ZOPFLI_SPLIT_NONE = 0, 1, 2     # Options.BlockSplitting (CafeUndZopfli) / blocksplitting[last] (jzopfli)


def zopfli_streams(inputs, iterations=20, splitting=ZOPFLI_SPLIT_FIRST, max_blocks=15, master_block=8 << 20, lib=None):
    """MultiCafeUndZopfliCompressor / MultiJZopfliCompressor.compressWithOptions for every input (d4g_zopfli_streams)."""
    L = lib or _need()
    n = len(inputs)
    keep = [bytes(s) for s in inputs]
    arr = (ctypes.c_char_p * max(1, n))(*keep)
    lens = (ctypes.c_size_t * max(1, n))(*[len(s) for s in keep])
    out = (ctypes.c_void_p * max(1, n))()
    olen = (ctypes.c_size_t * max(1, n))()
    rc = L.d4g_zopfli_streams(n, arr, lens, iterations, splitting, max_blocks, master_block, out, olen)
    if rc != 0:
        raise RuntimeError("d4g_zopfli_streams: " + L.d4g_last_error().decode())
    res = []
    for i in range(n):
        res.append(ctypes.string_at(out[i], olen[i]))
        L.d4g_free(out[i])
    return res


MODE_NONE, MODE_CHEAP, MODE_ZOPFLI, MODE_ZOPFLI_EXTENSIVE, MODE_ZOPFLI_VERY_EXTENSIVE = range(5)   # M/Optimise.java RecompressMode


class CompressionUtil:
    """C/CompressionUtil.java as CMDUtil configures it (M/CMDUtil.java:44-50): the compressor list of a recompress
    mode, every output through Deft.optimiseDeflateStream, strict minimum by parsed bit size in list order."""

    def __init__(self, mode=MODE_CHEAP, iter=20, mergeBlocks=True, lib=None):   # noqa: A002 (the reference's name)
        self.mode, self.iter, self.mergeBlocks, self._lib = mode, iter, mergeBlocks, lib
        self.last_winner = None

    def compress_many(self, buffers):
        L = self._lib or _need()
        n = len(buffers)
        keep = [bytes(b) for b in buffers]
        arr = (ctypes.c_char_p * max(1, n))(*keep)
        lens = (ctypes.c_size_t * max(1, n))(*[len(b) for b in keep])
        out = (ctypes.c_void_p * max(1, n))()
        olen = (ctypes.c_size_t * max(1, n))()
        win = (ctypes.c_int32 * max(1, n))()
        rc = L.d4g_compress(n, arr, lens, self.mode, self.iter, 1 if self.mergeBlocks else 0, out, olen, win)
        if rc != 0:
            raise IOError("Unable to compress data: " + L.d4g_last_error().decode())   # CompressionUtil.java:177-179
        res = []
        for i in range(n):
            res.append(ctypes.string_at(out[i], olen[i]))
            L.d4g_free(out[i])
        self.last_winner = list(win[:n])
        return res

    def compress(self, uncompressedData, threaded=False):
        """-> the smallest optimised stream (CompressionUtil.compress :106-182).  `threaded` is accepted and ignored:
        the result is the list-order one, which the reference's threaded path only matches when no sizes tie."""
        return self.compress_many([uncompressedData])[0]


def recompress_streams(streams, mode=MODE_CHEAP, mergeBlocks=True, iter=20, lib=None):   # noqa: A002
    """CMDUtil.optimise's per-stream work (M/CMDUtil.java:70-105) for a list of raw deflate streams.
    -> list of dict(status, saved_bits, recompress_saved, out) — out is None unless status == 0 (changed)."""
    L = lib or _need()
    n = len(streams)
    keep = [bytes(b) for b in streams]
    arr = (ctypes.c_char_p * max(1, n))(*keep)
    lens = (ctypes.c_size_t * max(1, n))(*[len(b) for b in keep])
    out = (ctypes.c_void_p * max(1, n))()
    olen = (ctypes.c_size_t * max(1, n))()
    sv = (ctypes.c_int64 * max(1, n))()
    rs = (ctypes.c_int64 * max(1, n))()
    st = (ctypes.c_int32 * max(1, n))()
    rc = L.d4g_recompress_streams(n, arr, lens, mode, iter, 1 if mergeBlocks else 0, out, olen, sv, rs, st)
    if rc != 0:
        raise RuntimeError("d4g_recompress_streams: " + L.d4g_last_error().decode())
    res = []
    for i in range(n):
        data = None
        if out[i]:
            data = ctypes.string_at(out[i], olen[i])
            L.d4g_free(out[i])
        res.append(dict(status=st[i], saved_bits=sv[i], recompress_saved=rs[i], out=data))
    return res


class Deft:
    """Static façade — B/Deft.java."""

    @staticmethod
    def optimiseDeflateStream(original, mergeBlocks=True):
        """Returns new bytes iff the stream parses and bits were saved; otherwise the SAME object it was given."""
        b = Batch([original]).run(mergeBlocks)
        try:
            if b.result(0)["status"] == 0:
                return b.output(0)
            return original
        finally:
            b.close()

    @staticmethod
    def getSizeBitsFallback(deflateStream, lib=None):
        L = lib or _need()
        bits = ctypes.c_int64()
        rc = L.d4g_size_bits_fallback(bytes(deflateStream), len(deflateStream), ctypes.byref(bits))
        if rc != 0:
            raise RuntimeError(L.d4g_last_error().decode())
        return bits.value


class DeflateStream:
    """Object API — B/deflate/DeflateStream.java (parse / optimise / getSizeBits / getUncompressedData / asBytes)."""
    DEFAULT_NAME = "unnamed stream"

    def __init__(self, name=None, lib=None):
        self.name = name or self.DEFAULT_NAME
        self._lib = lib
        self._data = None
        self._batch = None
        self._parsed = None
        self._dictionary = None

    def getName(self):
        return self.name

    def parse(self, data, dictionary=None):
        """-> bool.  `consumed` gives the bytes DeflateStream.parse(InputStream) reads (K/GZFile.java:84 relies on it).
        dictionary: the preset dictionary the stream was written against; optimise() and printBlockInfo() then use it too."""
        self._data = bytes(data)
        self._dictionary = None if dictionary is None else bytes(dictionary)
        self.close()
        self._parsed, self.consumed = inflate(self._data, self._dictionary, self._lib)
        return self._parsed is not None

    def getUncompressedData(self):
        return self._parsed

    def printBlockInfo(self):
        """DeflateStream.printBlockInfo (:35-51): the reference's text, for the stream as it stands (after optimise(): the
        optimised stream)."""
        b, own = self._batch, False
        if b is None:
            if self._parsed is None:
                raise RuntimeError("printBlockInfo() on a stream that did not parse")
            b, own = Batch([self._data], lib=self._lib, dictionaries=self._dictionary).parse(), True
        try:
            info = b.block_info(0, final=not own)
        finally:
            if own:
                b.close()
        lines = "".join("\nBlock %d position %d size %d type %s" % (k, bi["bit_pos"], bi["size_bits"], BLOCK_TYPE_NAMES[bi["type"]])
                        for k, bi in enumerate(info))
        return "Stream name: " + self.name + "\nBlock info:" + lines + "\nTotal blocks: %d" % len(info)

    def getSizeBits(self):
        if self._batch is not None:
            r = self._batch.result(0)
            return r["size_bits_in"] - r["saved_bits"]
        if self._dictionary is not None:   # (getSizeBitsFallback knows no dictionary)
            b = Batch([self._data], lib=self._lib, dictionaries=self._dictionary).parse()
            try:
                r = b.result(0)
                return r["size_bits_in"] if r["status"] >= 0 else len(self._data) * 8
            finally:
                b.close()
        return Deft.getSizeBitsFallback(self._data, self._lib)

    def optimise(self, mergeBlocks=True):
        """-> bits saved (DeflateStream.optimise(boolean), :496)."""
        self.close()
        self._batch = Batch([self._data], lib=self._lib, dictionaries=self._dictionary).run(mergeBlocks)
        return self._batch.result(0)["saved_bits"]

    def asBytes(self):
        """DeflateStream.asBytes() (:652) = write(): the stream as it stands.  Before optimise() that is the parsed
        stream re-serialised unchanged: the bytes parse() consumed, with the padding bits of the last byte written as
        zeros (DeflateStream.write :143 pads with zero bits)."""
        if self._batch is not None:
            return self._batch.output(0)
        if self._parsed is None:
            raise RuntimeError("asBytes() on a stream that did not parse")
        out = bytearray(self._data[:self.consumed])
        rem = self.getSizeBits() % 8
        if rem and out:
            out[-1] &= (1 << rem) - 1
        return bytes(out)

    def close(self):
        if self._batch is not None:
            self._batch.close()
            self._batch = None


class DeflateFilesContainer:
    """K/DeflateFilesContainer.java:18-43 — the batch seam: independent streams, results in index order."""

    @staticmethod
    def optimise(streams, mergeBlocks=True, printer=None):
        """streams: list of raw deflate byte strings.  Returns (total bits saved, [output bytes or the original]).
        `printer`, when given, receives the transcript lines the reference prints (:31-40)."""
        b = Batch(streams).run(mergeBlocks)
        total = 0
        outs = []
        try:
            for i, s in enumerate(streams):
                r = b.result(i)
                saved = r["saved_bits"] if r["status"] >= 0 else 0
                if printer and saved > 0:
                    printer("%d bits saved in stream %d (%s)" % (saved, i, DeflateStream.DEFAULT_NAME))
                total += saved
                outs.append(b.output(i) if r["status"] >= 0 else s)
            if printer and total > 0:
                printer("Total bits saved %d" % total)
        finally:
            b.close()
        return total, outs
