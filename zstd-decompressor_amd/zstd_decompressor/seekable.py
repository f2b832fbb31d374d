"""Random access: byte ranges of a zstd seekable archive that lies on the
device (zd_seekable_*, include/zd.h).

    a = SeekableArchive(tensor_or_bytes)
    t = a.read(off, length)                      # a uint8 device tensor
    r = a.reader(offsets, lengths)               # many ranges, one launch
    r.decode_async(); statuses, lengths = r.results(); r.outputs
    t = a.read(off, length, verify_table=True)   # the table's checksums enforced
    bad_entries, statuses = a.verify_all()       # the archive's `zstd -t`

A seekable archive is a multi-frame .zst that ends with a skippable frame
holding a seek table; every needed entry is decoded once per launch, a frame
wholly inside one range at that range's own destination.  verify_table=True
(ZD_SEEK_VERIFY_TABLE) compares the seek table's Checksum -- the low 32 bits
of XXH64 of the entry's decoded bytes -- of every needed entry inside the
launch: a range over an entry that differs ends CHECKSUM_WRONG, and
`verdicts()` names the entries.  An archive without checksums refuses the
option.  Limits: no dictionary, prefix or chain reads; a reader's destinations
are fixed at creation.
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


def _read_device(d_ptr: int, ctype, n: int):
    """n words of ctype at a device address, as a list (a blocking hipMemcpy of
    the HIP runtime the process already runs, as batch._read_u64)."""
    import os
    import torch
    if not n or not d_ptr:
        return []
    rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = C.CDLL(rt if os.path.exists(rt) else "libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    words = (ctype * n)()
    if hip.hipMemcpy(words, C.c_void_p(d_ptr), C.sizeof(ctype) * n, 2) != 0:     # hipMemcpyDeviceToHost
        raise ZdError(_lib.HIP, "hipMemcpy")
    return list(words)


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

    def reader(self, offsets, lengths, dsts=None, flags: int = 0, stream=None, verify_table: bool = False):
        """zd_seekable_read_create_ex: a SeekReader over ranges [offsets[i],
        offsets[i] + lengths[i]) of the content, clamped to its end.  offsets /
        lengths: lists, or contiguous int64 / uint64 device tensors.  dsts:
        None (one uint8 tensor of the clamped length is allocated per range:
        `.outputs`), a list of uint8 device tensors / device addresses / None,
        or a device tensor of addresses; range i is written at dsts[i].
        verify_table: every launch compares the table's Checksum of every
        needed entry (ZD_SEEK_VERIFY_TABLE); ZdError INVALID_ARG on an archive
        without checksums.  _lib.F_RFC in flags reaches the inner batch as the
        read option ZD_SEEK_RFC (the C call rejects the plan flag's bit)."""
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
        _lib.check(_lib.lib().zd_seekable_read_create_ex(self._h, C.c_void_p(addr[0]), C.c_void_p(addr[1]),
                                                         C.c_void_p(addr[2]), n, flags & ~_lib.F_RFC,
                                                         (_lib.SEEK_VERIFY_TABLE if verify_table else 0) |
                                                         (_lib.SEEK_RFC if flags & _lib.F_RFC else 0),
                                                         C.c_void_p(s), C.byref(h)),
                   "zd_seekable_read_create_ex")
        return SeekReader(h, n, outputs, keep_dst, self)

    def read(self, off: int, length: int, flags: int = 0, verify_table: bool = False):
        """Content bytes [off, off + length), clamped to the content's end, as a
        uint8 device tensor.  Raises ZdError with the range's status; with
        verify_table, CHECKSUM_WRONG for an entry whose bytes do not hash to
        the table's Checksum, and the error's `entries` lists those entries."""
        r = self.reader([off], [length], flags=flags, verify_table=verify_table)
        try:
            r.decode_async()
            st, ln = r.results()
            if st[0] != 0:
                e = ZdError(st[0], "SeekableArchive.read")
                e.entries = [f for f, ok in zip(*r.verdicts()[:2]) if ok == 0] if verify_table else []
                raise e
            return r.outputs[0][:ln[0]]
        finally:
            r.close()

    def verify_all(self, slab_bytes: int = 1 << 28, flags: int = 0):
        """The archive's `zstd -t`: verified reads of content bytes [k slab,
        (k + 1) slab) into one scratch tensor, every entry decoded and its
        table Checksum compared.  Returns (entries, statuses): the sorted
        indices of the entries that failed -- a verdict of 0 is CHECKSUM_WRONG;
        an entry of a failed range that was not compared is read once more
        alone, and that range's status is the entry's -- and their statuses.
        ValueError on an archive without checksums."""
        import torch
        from .batch import _read_u64
        self._open()
        if not self.has_checksums:
            raise ValueError("the archive's seek table carries no checksums")
        if slab_bytes <= 0:
            raise ValueError("slab_bytes must be positive")
        total, bad = self.content_size, {}
        slab = min(slab_bytes, max(total, 1))
        scratch = torch.empty(slab, dtype=torch.uint8, device=self._archive.device)
        suspects = set()
        for o in range(0, total, slab):
            r = self.reader([o], [slab], [scratch], flags=flags, verify_table=True)
            try:
                r.decode_async()
                st, _ = r.results()
                for f, ok, _h in zip(*r.verdicts()):
                    if ok == 0:
                        bad[f] = _lib.CHECKSUM_WRONG
                    elif ok < 0 and st[0] != 0:
                        suspects.add(f)
            finally:
                r.close()
        suspects -= set(bad)
        if suspects:
            d_off = _read_u64(self.table()[1], self.nframes + 1)
            for f in sorted(suspects):
                n = d_off[f + 1] - d_off[f]
                if n > scratch.numel():
                    scratch = torch.empty(n, dtype=torch.uint8, device=self._archive.device)
                r = self.reader([d_off[f]], [n], [scratch], flags=flags, verify_table=True)
                try:
                    r.decode_async()
                    st, _ = r.results()
                    if st[0] != 0:
                        bad[f] = st[0]
                finally:
                    r.close()
        entries = sorted(bad)
        return entries, [bad[f] for f in entries]

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
        self.info = _lib.SeekReadInfo2()
        _lib.check(_lib.lib().zd_seek_read_info_get_sized(h, C.cast(C.byref(self.info), C.POINTER(_lib.SeekReadInfo)),
                                                          C.sizeof(self.info)), "zd_seek_read_info_get_sized")

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

    def device_verdicts(self):
        """(device address of the uint32 entry indices, of the int8 verdicts, of
        the uint32 computed checksums, n): a verify_table reader's per-entry
        arrays, indexed by the inner batch's chunk and owned by the reader;
        (0, 0, 0, 0) for a reader made without the option."""
        e, ok, h32 = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = C.c_uint64()
        _lib.check(_lib.lib().zd_seek_read_device_verdicts(self._h, C.byref(e), C.byref(ok), C.byref(h32),
                                                           C.byref(n)), "zd_seek_read_device_verdicts")
        return e.value or 0, ok.value or 0, h32.value or 0, n.value

    def verdicts(self, stream=None):
        """(entries, ok, hash32) as lists, after waiting for `stream`: for every
        needed entry its index in the table, 1 / 0 / -1 (its bytes hash to the
        table's Checksum / they differ / not compared: it did not decode to
        its Decompressed_Size) and the computed low 32 bits of XXH64 (0 when
        not compared)."""
        import torch
        e, ok, h32, n = self.device_verdicts()
        (torch.cuda.current_stream() if stream is None else torch.cuda.ExternalStream(int(stream))).synchronize()
        return _read_device(e, C.c_uint32, n), _read_device(ok, C.c_int8, n), _read_device(h32, C.c_uint32, n)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().zd_seek_read_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
