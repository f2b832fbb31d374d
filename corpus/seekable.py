"""Writer of zstd SEEKABLE archives, for tests, timing scripts and examples.

A seekable archive is an ordinary multi-frame .zst whose last frame is a
skippable frame holding a seek table (restated from the published format
description; zstd-decompressor_amd/csrc/zd_seek.h reads the same layout):

    entries ... | 5E 2A 4D 18 | Frame_Size u32 | nframes x entry | footer
    entry  = Compressed_Size u32, Decompressed_Size u32 [, Checksum u32]
    footer = Number_Of_Frames u32, descriptor u8 (bit 7: checksums), B1 EA 92 8F

Checksum is the low 32 bits of XXH64 of the entry's decoded bytes.  The frames
come from the system libzstd (corpus/libzstd.py).  Files from zstd's own
seekable tools have not been compared with these.
"""
from __future__ import annotations

import struct

from . import libzstd

SKIPPABLE_MAGIC = 0x184D2A5E
SEEKABLE_MAGIC = 0x8F92EAB1
XXH64_EMPTY_LOW32 = 0x51D8E999      # XXH64("", seed 0) = 0xEF46DB3751D8E999


def skippable_frame(payload: bytes = b"") -> bytes:
    """A skippable frame (magic 0x184D2A50) around payload."""
    return struct.pack("<II", 0x184D2A50, len(payload)) + payload


def seek_table(entries, checksums: bool = False) -> bytes:
    """The seek table's frame for entries of (compressed, decompressed[, checksum])."""
    body = b"".join(struct.pack("<III", e[0], e[1], e[2]) if checksums else struct.pack("<II", e[0], e[1])
                    for e in entries)
    footer = struct.pack("<IBI", len(entries), 0x80 if checksums else 0, SEEKABLE_MAGIC)
    return struct.pack("<II", SKIPPABLE_MAGIC, len(body) + len(footer)) + body + footer


def _sizes(total: int, frame_bytes):
    if isinstance(frame_bytes, int):
        if frame_bytes <= 0:
            raise ValueError("frame_bytes must be positive")
        return [min(frame_bytes, total - o) for o in range(0, total, frame_bytes)]
    sizes = list(frame_bytes)
    if sum(sizes) != total:
        raise ValueError("the entries' sizes must add up to len(data)")
    return sizes


def _flag(which, i: int) -> bool:
    if callable(which):
        return bool(which(i))
    if isinstance(which, (list, tuple, set, frozenset)):
        return i in which
    return bool(which)


def write_seekable_parts(data: bytes, frame_bytes, level: int = 3, checksums: bool = False, frame_checksums=False):
    """(entries' bytes, table rows): entry i's bytes and (compressed,
    decompressed, checksum).  frame_bytes: one size for every entry (the last
    one shorter), or the list of the entries' content sizes, where 0 makes an
    entry of one skippable frame and no zstd frame.  frame_checksums: True, or
    a set / predicate of entry indices whose frames carry a Content_Checksum."""
    parts, rows = [], []
    o = 0
    for i, z in enumerate(_sizes(len(data), frame_bytes)):
        chunk = data[o:o + z]
        o += z
        if z == 0:
            c, ck = skippable_frame(b"seek"), XXH64_EMPTY_LOW32
        else:
            own = _flag(frame_checksums, i)
            c = libzstd.compress(chunk, level, checksum=own)
            ck = 0
            if checksums:
                # (a frame's Content_Checksum is the same 32 bits)
                withsum = c if own else libzstd.compress(chunk, level, checksum=True)
                ck = struct.unpack("<I", withsum[-4:])[0]
        parts.append(c)
        rows.append((len(c), z, ck))
    return parts, rows


def write_seekable(data: bytes, frame_bytes, level: int = 3, checksums: bool = False, frame_checksums=False) -> bytes:
    """data as a seekable archive of entries of frame_bytes content bytes each
    (see write_seekable_parts), the seek table with or without checksums."""
    parts, rows = write_seekable_parts(data, frame_bytes, level, checksums, frame_checksums)
    return b"".join(parts) + seek_table(rows, checksums)
