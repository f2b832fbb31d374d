"""ctypes binding of libzstd's dictionary calls (1.4.8 in this image), beside
corpus/libzstd.py: the dictionary trainer, and compression / decompression
with a dictionary.

Used only to make dictionary-compressed test frames and as the independent
RFC 8878 decoder their expected bytes come from.  Never on the product's
decode path.
"""
from __future__ import annotations

import ctypes as C

from . import libzstd

_bound = False


def lib():
    global _bound
    L = libzstd.lib()
    if not _bound:
        L.ZDICT_trainFromBuffer.restype = C.c_size_t
        L.ZDICT_trainFromBuffer.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t), C.c_uint]
        L.ZDICT_isError.restype = C.c_uint
        L.ZDICT_isError.argtypes = [C.c_size_t]
        L.ZDICT_getErrorName.restype = C.c_char_p
        L.ZDICT_getErrorName.argtypes = [C.c_size_t]
        L.ZDICT_getDictID.restype = C.c_uint
        L.ZDICT_getDictID.argtypes = [C.c_void_p, C.c_size_t]
        L.ZSTD_compress_usingDict.restype = C.c_size_t
        L.ZSTD_compress_usingDict.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_size_t, C.c_int]
        L.ZSTD_createDCtx.restype = C.c_void_p
        L.ZSTD_freeDCtx.argtypes = [C.c_void_p]
        L.ZSTD_decompress_usingDict.restype = C.c_size_t
        L.ZSTD_decompress_usingDict.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                C.c_void_p, C.c_size_t]
        # (the parameter API with a dictionary: a Content_Checksum, no Frame_Content_Size)
        L.ZSTD_CCtx_loadDictionary.restype = C.c_size_t
        L.ZSTD_CCtx_loadDictionary.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        # (a prefix: raw content for one frame, ZSTD_dct_rawContent)
        L.ZSTD_CCtx_refPrefix.restype = C.c_size_t
        L.ZSTD_CCtx_refPrefix.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.ZSTD_DCtx_refPrefix.restype = C.c_size_t
        L.ZSTD_DCtx_refPrefix.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.ZSTD_decompressDCtx.restype = C.c_size_t
        L.ZSTD_decompressDCtx.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        _bound = True
    return L


def train(samples, capacity: int) -> bytes:
    """ZDICT_trainFromBuffer: a formatted dictionary of at most `capacity`
    bytes from the sample records."""
    L = lib()
    blob = b"".join(samples)
    sizes = (C.c_size_t * len(samples))(*[len(s) for s in samples])
    dst = C.create_string_buffer(capacity)
    n = L.ZDICT_trainFromBuffer(dst, capacity, blob, sizes, len(samples))
    if L.ZDICT_isError(n):
        raise RuntimeError(L.ZDICT_getErrorName(n).decode())
    return dst.raw[:n]


def dict_id(dictionary: bytes) -> int:
    """ZDICT_getDictID: the ID of a formatted dictionary, 0 for raw content."""
    return lib().ZDICT_getDictID(dictionary, len(dictionary))


def compress(data: bytes, dictionary: bytes, level: int = 3, checksum: bool = False,
             content_size: bool = True) -> bytes:
    """One frame compressed against `dictionary` (formatted or raw content):
    ZSTD_compress_usingDict, or the parameter API with the dictionary loaded
    when a Content_Checksum or a frame without Frame_Content_Size is asked
    for (ZSTD_compress_usingDict takes neither)."""
    L = lib()
    cap = L.ZSTD_compressBound(len(data))
    dst = C.create_string_buffer(cap)
    cctx = L.ZSTD_createCCtx()
    try:
        if not checksum and content_size:
            n = libzstd._chk(L.ZSTD_compress_usingDict(cctx, dst, cap, data, len(data), dictionary, len(dictionary),
                                                       level))
        else:
            libzstd._chk(L.ZSTD_CCtx_setParameter(cctx, libzstd.ZSTD_c_compressionLevel, level))
            libzstd._chk(L.ZSTD_CCtx_setParameter(cctx, libzstd.ZSTD_c_checksumFlag, int(checksum)))
            libzstd._chk(L.ZSTD_CCtx_setParameter(cctx, libzstd.ZSTD_c_contentSizeFlag, int(content_size)))
            libzstd._chk(L.ZSTD_CCtx_loadDictionary(cctx, dictionary, len(dictionary)))
            n = libzstd._chk(L.ZSTD_compress2(cctx, dst, cap, data, len(data)))
    finally:
        L.ZSTD_freeCCtx(cctx)
    return dst.raw[:n]


def decompress(frame: bytes, dictionary: bytes, size: int) -> bytes:
    """ZSTD_decompress_usingDict of one frame (or several) into `size` bytes
    at most; raises RuntimeError with libzstd's message on failure."""
    L = lib()
    dst = C.create_string_buffer(max(size, 1))
    dctx = L.ZSTD_createDCtx()
    try:
        n = libzstd._chk(L.ZSTD_decompress_usingDict(dctx, dst, size, frame, len(frame), dictionary, len(dictionary)))
    finally:
        L.ZSTD_freeDCtx(dctx)
    return dst.raw[:n]


def prefix_compress(data: bytes, prefix: bytes, level: int = 3, checksum: bool = False,
                    content_size: bool = True) -> bytes:
    """One frame compressed against `prefix` as raw content, whatever its first
    bytes (ZSTD_CCtx_refPrefix + ZSTD_compress2: what `zstd --patch-from` does)."""
    L = lib()
    cap = L.ZSTD_compressBound(len(data))
    dst = C.create_string_buffer(cap)
    cctx = L.ZSTD_createCCtx()
    try:
        libzstd._chk(L.ZSTD_CCtx_setParameter(cctx, libzstd.ZSTD_c_compressionLevel, level))
        libzstd._chk(L.ZSTD_CCtx_setParameter(cctx, libzstd.ZSTD_c_checksumFlag, int(checksum)))
        libzstd._chk(L.ZSTD_CCtx_setParameter(cctx, libzstd.ZSTD_c_contentSizeFlag, int(content_size)))
        libzstd._chk(L.ZSTD_CCtx_refPrefix(cctx, prefix, len(prefix)))
        n = libzstd._chk(L.ZSTD_compress2(cctx, dst, cap, data, len(data)))
    finally:
        L.ZSTD_freeCCtx(cctx)
    return dst.raw[:n]


def prefix_decompress(frame: bytes, prefix: bytes, size: int) -> bytes:
    """ZSTD_DCtx_refPrefix + ZSTD_decompressDCtx of one frame into `size`
    bytes at most; raises RuntimeError with libzstd's message on failure."""
    L = lib()
    dst = C.create_string_buffer(max(size, 1))
    dctx = L.ZSTD_createDCtx()
    try:
        libzstd._chk(L.ZSTD_DCtx_refPrefix(dctx, prefix, len(prefix)))
        n = libzstd._chk(L.ZSTD_decompressDCtx(dctx, dst, size, frame, len(frame)))
    finally:
        L.ZSTD_freeDCtx(dctx)
    return dst.raw[:n]
