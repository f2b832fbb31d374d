"""Random access: byte ranges of a zstd seekable archive that lies on the
device (zd_seekable_*, include/zd.h).

    a = SeekableArchive(tensor_or_bytes)
    t = a.read(off, length)                      # a uint8 device tensor
    r = a.reader(offsets, lengths)               # many ranges, one launch
    r.decode_async(); statuses, lengths = r.results(); r.outputs

A seekable archive is a multi-frame .zst that ends with a skippable frame
holding a seek table; every needed entry is decoded once per launch, a frame
wholly inside one range at that range's own destination.  Limits: no
dictionary, prefix or chain reads; the seek table's own checksums are exposed
(`table()`), not verified; a reader's destinations are fixed at creation.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import ZdError


def _stream(stream):
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return int(stream)


class SeekableArchive:
    """zd_seekable: an open archive.  `archive` is a contiguous uint8 device
    tensor holding exactly the archive (any alignment, no padding), or bytes,
    which are uploaded.  The tensor must stay unchanged until close(): it is read
    here and whenever a reader is made, never by a decode."""

    def __init__(self, archive, stream=None):
        import torch
        if isinstance(archive, (bytes, bytearray, memoryview)):
            dev = torch.device("cuda", torch.cuda.current_device())
            host = torch.frombuffer(bytearray(archive), dtype=torch.uint8) if len(archive) else \
                torch.empty(0, dtype=torch.uint8)
            archive = host.to(dev)
        if not (isinstance(archive, torch.Tensor) and archive.is_cuda and archive.is_contiguous()
                and archive.dtype == torch.uint8 and archive.dim() == 1):
            raise ValueError("a contiguous 1-D uint8 device tensor or bytes required")
        self._archive = archive
        self._h = None
        h = C.c_void_p()
        _lib.check(_lib.lib().zd_seekable_open_device(C.c_void_p(archive.data_ptr() if archive.numel() else 0),
                                                      archive.numel(), C.c_void_p(_stream(stream)), C.byref(h)),
                   "zd_seekable_open_device")
        self._h = h
        self.info = _lib.SeekableInfo()
        _lib.check(_lib.lib().zd_seekable_info_get(h, C.byref(self.info)), "zd_seekable_info_get")
        self.nframes = self.info.nframes
        self.content_size = self.info.content_bytes
        self.has_checksums = bool(self.info.has_checksums)

    def table(self):
        """(c_off, d_off, checksum): device addresses of the table's arrays --
        uint64[nframes + 1] twice, uint32[nframes] or 0 without checksums --
        owned by the archive."""
        self._open()
        c, d, k = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().zd_seekable_table(self._h, C.byref(c), C.byref(d), C.byref(k)), "zd_seekable_table")
        return c.value or 0, d.value or 0, k.value or 0

    def _open(self):
        if not getattr(self, "_h", None):
            raise ValueError("the SeekableArchive is closed")

    def reader(self, offsets, lengths, dsts=None, flags: int = 0, stream=None):
        """zd_seekable_read_create: a SeekReader over ranges [offsets[i],
        offsets[i] + lengths[i]) of the content, clamped to its end.  offsets /
        lengths: lists, or contiguous int64 / uint64 device tensors.  dsts:
        None (one uint8 tensor of the clamped length is allocated per range:
        `.outputs`), a list of uint8 device tensors / device addresses / None,
        or a device tensor of addresses; range i is written at dsts[i]."""
        import torch
        from .batch import _device_arrays
        self._open()
        dev = self._archive.device
        outputs = None
        if dsts is None:
            offs = offsets.cpu().tolist() if isinstance(offsets, torch.Tensor) else list(offsets)
            lens = lengths.cpu().tolist() if isinstance(lengths, torch.Tensor) else list(lengths)
            total = self.content_size
            outputs = [torch.empty(max(0, min(int(n), total - int(o))), dtype=torch.uint8, device=dev)
                       for o, n in zip(offs, lens)]
            dsts = outputs
        keep_dst = dsts
        if isinstance(dsts, (list, tuple)):
            dsts = [(d.data_ptr() if d.numel() else 0) if isinstance(d, torch.Tensor) else int(d or 0) for d in dsts]
        n, addr, keep = _device_arrays((offsets, lengths, dsts), None)
        s = _stream(stream)
        h = C.c_void_p()
        _lib.check(_lib.lib().zd_seekable_read_create(self._h, C.c_void_p(addr[0]), C.c_void_p(addr[1]),
                                                      C.c_void_p(addr[2]), n, flags, C.c_void_p(s), C.byref(h)),
                   "zd_seekable_read_create")
        return SeekReader(h, n, outputs, keep_dst, self)

    def read(self, off: int, length: int, flags: int = 0):
        """Content bytes [off, off + length), clamped to the content's end, as a
        uint8 device tensor.  Raises ZdError with the range's status."""
        r = self.reader([off], [length], flags=flags)
        try:
            r.decode_async()
            st, ln = r.results()
            if st[0] != 0:
                raise ZdError(st[0], "SeekableArchive.read")
            return r.outputs[0][:ln[0]]
        finally:
            r.close()

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().zd_seekable_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SeekReader:
    """zd_seek_read: R ranges of an archive, decoded by one launch.  Made by
    SeekableArchive.reader."""

    def __init__(self, h, nranges, outputs, keep, archive):
        self._h = h
        self.nranges = nranges
        self.outputs = outputs
        self._keep = (keep, archive._archive)
        self.info = _lib.SeekReadInfo()
        _lib.check(_lib.lib().zd_seek_read_info_get(h, C.byref(self.info)), "zd_seek_read_info_get")

    def decode_async(self, stream=None):
        """The inner batch's decode, the staged frames' copy, the result pass: no
        allocation, no host synchronisation; may be called again."""
        _lib.check(_lib.lib().zd_seek_read_decode_async(self._h, C.c_void_p(_stream(stream))),
                   "zd_seek_read_decode_async")

    def device_results(self):
        """(device address of the int32 statuses, device address of the uint64 lengths)."""
        st, ln = C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().zd_seek_read_device_results(self._h, C.byref(st), C.byref(ln)),
                   "zd_seek_read_device_results")
        return st.value or 0, ln.value or 0

    def results(self, stream=None):
        """(statuses, lengths) per range, after waiting for `stream`."""
        n = self.nranges
        st = (C.c_int32 * max(n, 1))()
        ln = (C.c_uint64 * max(n, 1))()
        bad = C.c_uint64()
        _lib.check(_lib.lib().zd_seek_read_results(self._h, C.c_void_p(_stream(stream)), st, ln, n, C.byref(bad)),
                   "zd_seek_read_results")
        return list(st)[:n], list(ln)[:n]

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().zd_seek_read_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
