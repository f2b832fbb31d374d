"""Batches whose chunks hold several concatenated zstd frames (zd_multi_*,
include/zd.h).

    b = MultiFrameBatch(src_ptrs, src_sizes, dst_ptrs, dst_caps)
    b.decode_async(); statuses, lengths = b.results()
    statuses, lengths = decode_multi(srcs, dsts)          # lists of uint8 device tensors

A chunk is any zstd payload: `cat a.zst b.zst`, pzstd output, a message
written by a streaming compressor that closes a frame at every flush.  It is
cut on the GPU into sub-chunks of one frame each, which an ordinary
device-built batch decodes: frames that carry a Frame_Content_Size decode in
place, one behind the other; every frame behind the first one without it
decodes into a staging buffer and is copied behind the bytes before it.  A
chunk's status is its first failing frame's.  Limits: no prefix, chain or
packed multi-frame batches; the destinations are fixed at creation; one lane
walks a chunk's headers at creation, so one huge multi-frame file belongs in
Plan.from_device.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from .seekable import _read_device, _stream


class MultiFrameBatch:
    """zd_multi: src_ptrs / src_sizes / dst_ptrs / dst_caps are lists (uploaded,
    as SeekableArchive.reader uploads its ranges) or contiguous int64 / uint64
    device tensors of one entry a chunk; they may be released when this
    returns, and so may the sources.  dictionary: a Dictionary or a
    DictionarySet.  flags: a Batch's (F_SKIPPABLE is INVALID_ARG).  A bad entry
    (a NULL address with a non-zero count) fails its own chunk with
    INVALID_ARG; overlapping destinations are the caller's duty.  stream (here
    and in every method): a HIP stream handle; 0: torch's current stream."""

    def __init__(self, src_ptrs, src_sizes, dst_ptrs, dst_caps, flags: int = 0, dictionary=None, stream=0):
        from .batch import DictionarySet, _device_arrays
        self._h = None
        if dictionary is not None and not getattr(dictionary, "_h", None):
            raise ValueError("the %s is closed" % type(dictionary).__name__)
        n, addr, keep = _device_arrays((src_ptrs, src_sizes, dst_ptrs, dst_caps), None)
        is_set = isinstance(dictionary, DictionarySet)
        h = C.c_void_p()
        _lib.check(_lib.lib().zd_multi_create_device(
            *[C.c_void_p(a) for a in addr], n, flags,
            dictionary._h if dictionary is not None and not is_set else None,
            dictionary._h if is_set else None, C.c_void_p(_stream(stream or None)), C.byref(h)),
            "zd_multi_create_device")
        self._h = h
        self.nchunks = n
        self._keep = dictionary
        self.info = _lib.MultiInfo()
        _lib.check(_lib.lib().zd_multi_info_get_sized(h, C.byref(self.info), C.sizeof(self.info)),
                   "zd_multi_info_get_sized")

    def decode_async(self, stream=0):
        """The inner batch's decode, the join pass, the staged frames' copy: no
        allocation, no host synchronisation; may be called again."""
        _lib.check(_lib.lib().zd_multi_decode_async(self._h, C.c_void_p(_stream(stream or None))),
                   "zd_multi_decode_async")

    def finish_async(self, stream=0):
        """The join and copy passes alone (zd_multi_finish_async)."""
        _lib.check(_lib.lib().zd_multi_finish_async(self._h, C.c_void_p(_stream(stream or None))),
                   "zd_multi_finish_async")

    def device_results(self):
        """(device address of the int32 statuses, device address of the uint64
        lengths), one entry a chunk: final behind what decode_async queued."""
        st, ln = C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().zd_multi_device_results(self._h, C.byref(st), C.byref(ln)), "zd_multi_device_results")
        return st.value or 0, ln.value or 0

    def results(self, stream=0):
        """(statuses, lengths) per chunk, after waiting for `stream`; a
        block-parallel frame that did not converge is decoded again first."""
        n = self.nchunks
        st = (C.c_int32 * max(n, 1))()
        ln = (C.c_uint64 * max(n, 1))()
        bad = C.c_uint64()
        _lib.check(_lib.lib().zd_multi_results(self._h, C.c_void_p(_stream(stream or None)), st, ln, n, C.byref(bad)),
                   "zd_multi_results")
        return list(st)[:n], list(ln)[:n]

    def frames(self, stream=0):
        """(first, statuses, lengths) as lists, after waiting for `stream`:
        chunk i's frames (its sub-chunks) are first[i] .. first[i + 1) of the
        two per-frame lists, the inner batch's results."""
        import torch
        first, st, ln = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().zd_multi_device_frames(self._h, C.byref(first), C.byref(st), C.byref(ln)),
                   "zd_multi_device_frames")
        (torch.cuda.ExternalStream(int(stream)) if stream else torch.cuda.current_stream()).synchronize()
        n = self.nchunks
        if not n:
            return [0], [], []
        f = self.info.frames
        return (_read_device(first.value, C.c_uint64, n + 1), _read_device(st.value, C.c_int32, f),
                _read_device(ln.value, C.c_uint64, f))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().zd_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_multi(srcs, dsts, flags: int = 0, dictionary=None):
    """Decode uint8 device tensors srcs[i] (one chunk of any number of frames
    each) into dsts[i] on torch's current stream: (statuses, lengths)."""
    import torch
    if len(srcs) != len(dsts):
        raise ValueError("srcs and dsts differ in length")
    for t in list(srcs) + list(dsts):
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("contiguous uint8 device tensors required")
    b = MultiFrameBatch([t.data_ptr() if t.numel() else 0 for t in srcs], [t.numel() for t in srcs],
                        [t.data_ptr() if t.numel() else 0 for t in dsts], [t.numel() for t in dsts],
                        flags=flags, dictionary=dictionary)
    try:
        b.decode_async()
        return b.results()
    finally:
        b.close()
