"""ctypes binding of lib/libzd.so (C ABI in include/zd.h).

The decode path is the HIP library only: if it is missing this module raises
at import time — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("ZD_LIB_PATH") or os.path.join(_PKG, "lib", "libzd.so")

# status codes (include/zd.h)
OK = 0
STATUS_NAMES = {}


class ZdError(Exception):
    """A non-zero zd status.  `name` is the reference's error variant
    (parsing::Error, literals::Error, frame::Error, ...)."""

    def __init__(self, code: int, where: str = ""):
        self.code = code
        self.name = status_name(code)
        super().__init__(f"{self.name} ({code}){' in ' + where if where else ''}")


class FrameDesc(C.Structure):
    _fields_ = [("src_offset", C.c_uint64), ("src_size", C.c_uint64), ("content_size", C.c_uint64),
                ("window_size", C.c_uint64), ("dict_id", C.c_uint64), ("magic", C.c_uint32),
                ("kind", C.c_uint32), ("first_block", C.c_uint32), ("num_blocks", C.c_uint32),
                ("has_checksum", C.c_uint32), ("checksum", C.c_uint32)]


class BlockDesc(C.Structure):
    _fields_ = [("src_offset", C.c_uint64), ("block_size", C.c_uint32), ("type", C.c_uint8),
                ("last", C.c_uint8), ("rle_byte", C.c_uint8), ("_pad", C.c_uint8)]


class PlanInfo(C.Structure):
    _fields_ = [("nframes", C.c_uint64), ("nblocks", C.c_uint64), ("ncompressed", C.c_uint64),
                ("src_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("out_exact", C.c_uint64),
                ("workspace_bytes", C.c_uint64), ("nsequences", C.c_uint64), ("nliterals", C.c_uint64),
                ("index_status", C.c_int32), ("executors", C.c_uint32), ("host_ns", C.c_uint64),
                ("device_ns", C.c_uint64), ("walk_serial_bytes", C.c_uint64),
                ("io_h2d_ns", C.c_uint64), ("io_decode_ns", C.c_uint64), ("io_d2h_ns", C.c_uint64),
                ("error_key", C.c_uint64), ("replans", C.c_uint64),
                ("fused_redo_frames", C.c_uint64), ("device_descriptors", C.c_uint64)]


class GatherResult(C.Structure):
    _fields_ = [("total_len", C.c_uint64), ("status", C.c_int32), ("failed_rank", C.c_int32),
                ("first_error_frame", C.c_int64)]


class BatchInfo(C.Structure):
    _fields_ = [("nchunks", C.c_uint64), ("gathered_bytes", C.c_uint64), ("nblocks", C.c_uint64),
                ("nsequences", C.c_uint64), ("workspace_bytes", C.c_uint64), ("executors", C.c_uint32),
                ("device_built", C.c_uint32), ("gather_ns", C.c_uint64), ("walk_ns", C.c_uint64),
                ("host_ns", C.c_uint64), ("upload_ns", C.c_uint64)]


class BatchInfoEx(BatchInfo):
    """zd_batch_info as include/zd.h has it now (zd_batch_info_get_sized fills
    it; BatchInfo is the 80 bytes zd_batch_info_get writes)."""
    _fields_ = [("prefix_bytes_total", C.c_uint64)]


class BatchInfo2(BatchInfoEx):
    """zd_batch_info2: what zd_batch_info_get_sized writes behind zd_batch_info
    when the caller's size covers it."""
    _fields_ = [("k4j_chunks", C.c_uint64)]


class SeekableInfo(C.Structure):
    """zd_seekable_info"""
    _fields_ = [("nframes", C.c_uint64), ("content_bytes", C.c_uint64), ("compressed_bytes", C.c_uint64),
                ("table_bytes", C.c_uint64), ("has_checksums", C.c_uint32), ("max_frame_content", C.c_uint32)]


class SeekReadInfo(C.Structure):
    """zd_seek_read_info"""
    _fields_ = [("nranges", C.c_uint64), ("frames_decoded", C.c_uint64), ("frames_in_place", C.c_uint64),
                ("staged_bytes", C.c_uint64), ("copy_pieces", C.c_uint64), ("batch", BatchInfo2)]


class SeekReadInfo2(SeekReadInfo):
    """zd_seek_read_info2: what zd_seek_read_info_get_sized writes behind
    zd_seek_read_info when the caller's size covers it."""
    _fields_ = [("read_flags", C.c_uint64), ("verify_entries", C.c_uint64)]


class MultiInfo(C.Structure):
    """zd_multi_info"""
    _fields_ = [("nchunks", C.c_uint64), ("frames", C.c_uint64), ("frames_in_place", C.c_uint64),
                ("staged_frames", C.c_uint64), ("staged_bytes", C.c_uint64), ("copy_pieces", C.c_uint64),
                ("batch", BatchInfo2)]


COMM_ID_BYTES = 128

# every entry point declared in include/zd.h: name -> (restype, argtypes)
_u8p, _sz, _szp, _vp = C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p
SIGNATURES = {
    "zd_status_name": (C.c_char_p, [C.c_int]),
    "zd_route": (C.c_int, [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32,
                           C.POINTER(C.c_uint32)]),
    "zd_abi_version": (C.c_int, []),
    "zd_trim_cache": (None, []),
    "zd_frames_index": (C.c_int, [_vp, _sz, C.POINTER(FrameDesc), _sz, _szp, C.POINTER(BlockDesc), _sz, _szp, _szp]),
    "zd_plan_create": (C.c_int, [_vp, _sz, C.c_uint32, C.POINTER(_vp)]),
    "zd_plan_create_device": (C.c_int, [_vp, _sz, C.c_uint32, _vp, C.POINTER(_vp)]),
    "zd_plan_info_get": (C.c_int, [_vp, C.POINTER(PlanInfo)]),
    "zd_plan_destroy": (None, [_vp]),
    "zd_decode_async": (C.c_int, [_vp, _vp, _vp, _sz, _vp]),
    "zd_plan_results": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    "zd_plan_checksums": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "zd_plan_set_profiling": (C.c_int, [_vp, C.c_int]),
    "zd_plan_k1_fallbacks": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "zd_plan_kernel_times": (C.c_int, [_vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]),
    "zd_decompress": (C.c_int, [_vp, _sz, _vp, _sz, _szp, C.c_uint32]),
    "zd_plan_decompress": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "zd_dict_create": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "zd_dict_destroy": (None, [_vp]),
    "zd_dict_info": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                               C.POINTER(C.c_int)]),
    "zd_plan_create_dict": (C.c_int, [_vp, _sz, C.c_uint32, _vp, C.POINTER(_vp)]),
    "zd_decompress_dict": (C.c_int, [_vp, _sz, _vp, _sz, _szp, C.c_uint32, _vp]),
    "zd_dict_set_create": (C.c_int, [C.POINTER(_vp), _sz, C.c_int, C.POINTER(_vp)]),
    "zd_dict_set_destroy": (None, [_vp]),
    "zd_dict_set_info": (C.c_int, [_vp, _szp, C.POINTER(C.c_int)]),
    "zd_plan_create_dicts": (C.c_int, [_vp, _sz, C.c_uint32, _vp, C.POINTER(_vp)]),
    "zd_decompress_dicts": (C.c_int, [_vp, _sz, _vp, _sz, _szp, C.c_uint32, _vp]),
    "zd_batch_create_dicts": (C.c_int, [C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp), C.POINTER(C.c_uint64),
                                        _sz, C.c_uint32, _vp, _vp, C.POINTER(_vp)]),
    "zd_batch_create": (C.c_int, [C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp), C.POINTER(C.c_uint64), _sz,
                                  C.c_uint32, _vp, _vp, C.POINTER(_vp)]),
    "zd_batch_create_device": (C.c_int, [_vp, _vp, _vp, _vp, _sz, C.c_uint32, _vp, _vp, C.POINTER(_vp)]),
    "zd_batch_create_device_dicts": (C.c_int, [_vp, _vp, _vp, _vp, _sz, C.c_uint32, _vp, _vp, C.POINTER(_vp)]),
    "zd_batch_create_prefix": (C.c_int, [C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp), C.POINTER(C.c_uint64),
                                         C.POINTER(_vp), C.POINTER(C.c_uint64), _sz, C.c_uint32, _vp,
                                         C.POINTER(_vp)]),
    "zd_batch_create_device_prefix": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, C.c_uint32, _vp, C.POINTER(_vp)]),
    "zd_batch_create_chain": (C.c_int, [C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp), C.POINTER(C.c_uint64),
                                        C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(C.c_int64), _sz, C.c_uint32,
                                        _vp, C.POINTER(_vp)]),
    "zd_batch_create_device_chain": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, C.c_uint32, _vp,
                                               C.POINTER(_vp)]),
    "zd_batch_chain_info": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "zd_chunk_sizes_device": (C.c_int, [_vp, _vp, _sz, C.c_uint32, _vp, _vp, _vp, _vp]),
    "zd_batch_create_device_packed": (C.c_int, [_vp, _vp, _sz, C.c_uint32, C.c_uint32, _vp, _vp, C.POINTER(_vp)]),
    "zd_batch_create_device_packed_dicts": (C.c_int, [_vp, _vp, _sz, C.c_uint32, C.c_uint32, _vp, _vp,
                                                      C.POINTER(_vp)]),
    "zd_batch_output_layout": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(_vp), C.POINTER(_vp)]),
    "zd_batch_bind_output": (C.c_int, [_vp, _vp, C.c_uint64]),
    "zd_batch_info_get": (C.c_int, [_vp, C.POINTER(BatchInfo)]),
    "zd_batch_info_get_sized": (C.c_int, [_vp, C.POINTER(BatchInfoEx), _sz]),
    "zd_batch_decode_async": (C.c_int, [_vp, _vp]),
    "zd_batch_device_results": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "zd_batch_device_checksums": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "zd_batch_results": (C.c_int, [_vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), _sz,
                                   C.POINTER(C.c_uint64)]),
    "zd_batch_checksums": (C.c_int, [_vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "zd_batch_destroy": (None, [_vp]),
    "zd_seekable_open_device": (C.c_int, [_vp, _sz, _vp, C.POINTER(_vp)]),
    "zd_seekable_info_get": (C.c_int, [_vp, C.POINTER(SeekableInfo)]),
    "zd_seekable_table": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "zd_seekable_close": (None, [_vp]),
    "zd_seekable_read_create": (C.c_int, [_vp, _vp, _vp, _vp, _sz, C.c_uint32, _vp, C.POINTER(_vp)]),
    "zd_seek_read_decode_async": (C.c_int, [_vp, _vp]),
    "zd_seek_read_finish_async": (C.c_int, [_vp, _vp]),
    "zd_seek_read_device_results": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "zd_seek_read_results": (C.c_int, [_vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), _sz,
                                       C.POINTER(C.c_uint64)]),
    "zd_seek_read_info_get": (C.c_int, [_vp, C.POINTER(SeekReadInfo)]),
    "zd_seekable_read_create_ex": (C.c_int, [_vp, _vp, _vp, _vp, _sz, C.c_uint32, C.c_uint32, _vp, C.POINTER(_vp)]),
    "zd_seek_read_device_verdicts": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                                               C.POINTER(C.c_uint64)]),
    "zd_seek_read_info_get_sized": (C.c_int, [_vp, C.POINTER(SeekReadInfo), _sz]),
    "zd_seek_read_destroy": (None, [_vp]),
    "zd_multi_create_device": (C.c_int, [_vp, _vp, _vp, _vp, _sz, C.c_uint32, _vp, _vp, _vp, C.POINTER(_vp)]),
    "zd_multi_decode_async": (C.c_int, [_vp, _vp]),
    "zd_multi_finish_async": (C.c_int, [_vp, _vp]),
    "zd_multi_device_results": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "zd_multi_results": (C.c_int, [_vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), _sz,
                                   C.POINTER(C.c_uint64)]),
    "zd_multi_device_frames": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "zd_multi_info_get_sized": (C.c_int, [_vp, C.POINTER(MultiInfo), _sz]),
    "zd_multi_destroy": (None, [_vp]),
    "zd_context_new": (C.c_int, [C.c_uint64, C.POINTER(_vp)]),
    "zd_context_free": (None, [_vp]),
    "zd_block_decode": (C.c_int, [_vp, _vp, _sz, _szp, C.POINTER(C.c_int)]),
    "zd_execute_sequences": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                       _sz, _vp, _sz]),
    "zd_context_decoded": (C.c_int, [_vp, _vp, _sz, _szp]),
    "zd_context_offsets": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "zd_shard_partition": (C.c_int, [C.POINTER(C.c_uint64), _sz, C.c_int, _szp]),
    "zd_shard_range": (C.c_int, [_vp, _sz, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "zd_plan_frame_outputs": (C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                        C.c_size_t, C.POINTER(C.c_size_t)]),
    "zd_comm_unique_id": (C.c_int, [_vp]),
    "zd_comm_create": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "zd_comm_destroy": (None, [_vp]),
    "zd_comm_buffers": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "zd_gather_layout": (C.c_int, [C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.POINTER(GatherResult)]),
    "zd_comm_gather": (C.c_int, [_vp, _vp, C.c_uint64, C.c_int32, C.c_int64, _vp, C.c_uint64,
                                 C.POINTER(GatherResult), _vp]),
    "zd_decode_sharded": (C.c_int, [_vp, _vp, _sz, C.c_uint32, _vp, C.c_uint64, C.POINTER(GatherResult), _vp]),
    "zd_decode_sharded_at": (C.c_int, [_vp, _vp, _sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, _vp,
                                       C.c_uint64, C.POINTER(GatherResult), _vp]),
    "zd_shard_cuts": (C.c_int, [_vp, _sz, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "zd_shard_range_at": (C.c_int, [_vp, _sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int, C.c_int,
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint64)]),
}

_lib = None


def _one_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64
    (soname libamdhip64.so.7, loaded as torch/lib/libamdhip64.so), and libzd's
    dependency on libamdhip64.so.7 binds to whichever copy is loaded first;
    loading libzd before torch would leave torch a second runtime that finds
    no GPU.  So torch's copy goes in first -- by path, without importing torch
    (which costs seconds): a later `import torch` then maps the same file and
    shares it.  With no torch installed, libzd takes ROCm's own runtime."""
    import sys
    if "torch" in sys.modules:
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    for d in spec.submodule_search_locations:
        rt = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(rt):
            C.CDLL(rt, mode=C.RTLD_GLOBAL)
            return


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built: run `make -C zstd-decompressor_amd` "
                              "(or __graft_entry__.build()); there is no CPU fallback")
        _one_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def status_name(code: int) -> str:
    return lib().zd_status_name(code).decode()


def check(code: int, where: str = ""):
    if code != OK:
        raise ZdError(code, where)
    return code


def buf(data):
    """(pointer, length) for a bytes-like object without copying when possible."""
    if isinstance(data, (bytes, bytearray, memoryview)):
        mv = memoryview(data).cast("B")
        n = mv.nbytes
        if n == 0:
            return None, 0, None
        if isinstance(data, bytes):
            keep = C.c_char_p(data)
            return C.cast(keep, C.c_void_p), n, keep
        arr = (C.c_uint8 * n).from_buffer(mv if not mv.readonly else bytearray(mv))
        return C.cast(arr, C.c_void_p), n, arr
    raise TypeError("bytes-like object required")

def buf_from(data: bytes, off: int):
    """(pointer, length, keep) for data[off:] of a bytes object, without the
    copy a slice makes (Frame.parse on a parser's remaining bytes: a 100 MB
    input cost ~10 ms a frame in slicing alone)."""
    n = len(data) - off
    if n <= 0:
        return None, 0, None
    keep = C.c_char_p(data)
    return C.c_void_p(C.cast(keep, C.c_void_p).value + off), n, keep


def take(arr, n: int) -> bytes:
    """The first n bytes of a ctypes byte array, one memcpy (a buffer view:
    C.string_at's size is a C int, and a ctypes slice goes element by element)."""
    return bytes(memoryview(arr).cast("B")[:n])


# status codes mirrored from include/zd.h
NOT_ENOUGH_BYTES, NOT_ENOUGH_BITS, MAX_READABLE_BITS_EXCEEDED = -1, -2, -3
EMPTY_INPUT_DATA, NULL_BYTE, EMPTY_SLICE = -4, -5, -6
LARGE_ACCURACY_LOG, CORRUPTED_TABLE, SEQUENCE_CODE_MAX_EXCEEDED = -12, -13, -14
HUFFMAN_DECODER_MISSING, CORRUPTED_STREAMS_SIZE = -20, -21
SEQ_RESERVED_SET, NO_PREVIOUS_DECODER = -30, -31
CTX_WINDOW_SIZE_TOO_BIG, NULL_OFFSET, IMPOSSIBLE_VALUE = -40, -41, -42
RESERVED_BLOCK_TYPE = -50
UNRECOGNIZED_MAGIC, FRAME_RESERVED_SET, MISSING_CHECKSUM, WINDOW_SIZE_TOO_BIG = -60, -61, -64, -66
REF_PANIC, OUT_OF_DOMAIN, DST_TOO_SMALL, INVALID_ARG, HIP, NO_MEMORY, NOT_DECODED = -90, -91, -92, -93, -94, -95, -96
DICT_CORRUPTED, DICT_MISMATCH = -98, -99
CHECKSUM_WRONG = -100  # F_VERIFY_CHECKSUM: the frame decoded, its bytes do not hash to its Content_Checksum
SEEK_TABLE = -101      # a seekable archive's table contradicts itself or the archive; a frame of another length
DICT_SET_MAX = 4096    # ZD_DICT_SET_MAX
CHAIN_MAX_DEPTH = 255  # ZD_CHAIN_MAX_DEPTH: in-batch ancestors a chunk of a chain batch may have
F_SKIPPABLE = 1
F_BLOCK_PARALLEL = 2   # every frame with a compressed block -> K4J (block-parallel execute); prefix batches too
F_FRAME_SERIAL = 4     # no frame -> K4J
F_SEQ_ONE_LANE = 8     # K3 one lane per block instead of four (K3Q)
F_NO_FUSE = 32         # K3 then K4 as two launches in few-frame plans (no zd_k_fused)
F_K1_LANES = 64        # K1's sequence half on serial lanes in plans of <= 16,384 tables
F_J_ONE_ROUND = 128    # test switch: K4J pointer jumping cut to one round of one hop
F_SEQ_NO_LATENCY = 256 # K3Q instead of the one-block-per-wave K3L in plans of few blocks
F_K1_SPLIT = 512       # K1 as a parse pass and a build pass in a plan of any size
F_VERIFY_CHECKSUM = 1024  # Content_Checksums verified inside the decode launch (zd_k_verify): CHECKSUM_WRONG
F_LONG_WINDOW = 2048   # accept a Window_Size up to 2 GiB (default: the reference's 8 MiB limit)
F_CHAIN_BLOCK_PARALLEL = 4096  # a chain batch (parents=): frames with a compressed block -> K4J, level by level
F_AUTO_EXECUTOR = 8192  # a prefix or chain batch: each chunk's executor by rule (include/zd.h ZD_AUTO_*)
SEEK_RFC = 4           # zd_seekable_read_create_ex read_flags: the inner batch decodes with F_RFC
SEEK_VERIFY_TABLE = 1  # zd_seekable_read_create_ex read_flags: the seek table's Checksums verified inside the launch
SIZES_DICT = 1         # zd_chunk_sizes_device: the chunks will be decoded with a dictionary or set
F_RFC = 16384           # frames decode as RFC 8878 / libzstd have them (default: the reference's decoder, D1-D3, D8)
F_DICT_BLOCK_PARALLEL = 32768  # a dictionary / set plan or batch: frames may run on K4J (with F_BLOCK_PARALLEL every
                               # frame with a compressed block, with F_FRAME_SERIAL none, else by the ZD_AUTO_* rule)
SIZES_RFC = 16384       # zd_chunk_sizes_device: the chunks will be decoded with F_RFC (the same bit)
SIZES_MULTI_FRAME = 8    # zd_chunk_sizes_device: the chunks may hold several frames (a MultiFrameBatch will decode them)
SIZES_LONG_WINDOW = 2048  # zd_chunk_sizes_device: the chunks will be decoded with F_LONG_WINDOW (the same bit)
EXEC_FUSED, EXEC_K4F, EXEC_K4J = 1, 2, 4  # zd_plan_info.executors bits (include/zd.h ZD_EXEC_*)
