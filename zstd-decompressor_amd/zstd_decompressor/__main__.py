"""Command line, mirroring the reference CLI (src/main.rs:7-60):

    python -m zstd_decompressor FILE [-i/--info] [-o/--output FILE] [-p/--print-skippable] [-D DICT]... [--verify] [--long]
    python -m zstd_decompressor FILE --patch-from OLD -o FILE [--long]
    python -m zstd_decompressor FILE --range OFF:LEN [-o FILE] [--verify] [--verify-table] [--long]
    python -m zstd_decompressor FILE --verify-table [--verify] [--long]

Decodes every frame of FILE on the GPU (the HIP pipeline behind zd_decompress)
and writes the concatenated output to stdout or --output.  As in the
reference: skippable frames are dropped unless -p; the first failing frame
ends the run with its error (exit status 1, nothing written); the output must
be UTF-8 (the reference's `String::from_utf8(res).unwrap()` panics otherwise:
exit status 101).  --info prints one line per frame instead (the reference
prints the parsed frames with `{:#x?}`).  Extra, beyond the reference:
--check-checksums verifies Content_Checksum (XXH64) on the GPU and reports
mismatches on stderr (the reference computes and never enforces it);
--verify enforces it inside the decode launch: a frame whose bytes do not hash
to its Content_Checksum ends the run with `Error: frame N: ChecksumWrong`
(exit status 1), as `zstd -d` fails such a file;
-D DICT decodes every frame with the dictionary file DICT (formatted or raw
content), as zstd's own -D does; -D given several times makes a dictionary
set: every frame decodes with the dictionary its Dictionary_ID names, a frame
without an ID with the one raw-content file if there is one, else the first.
When some frame's Frame_Content_Size is at least 2 MiB (--patch-from's
threshold below) the plan is created with F_DICT_BLOCK_PARALLEL, so that its
frames of several blocks decode block-parallel; the output is the same.
--patch-from OLD decodes FILE, one frame made by `zstd --patch-from OLD`,
against the bytes of OLD as its prefix (raw content, whatever they start
with): a prefix batch of one chunk with OLD uploaded.  The output is written
as bytes (a patched file need not be text); a failure prints the chunk's
status name and exits with status 1.  Not together with -D.  A frame whose
Frame_Content_Size is at least 2 MiB (16 blocks of 128 KiB, the block count
from which a plain plan sends a frame to the block-parallel executor) is
decoded block-parallel (F_BLOCK_PARALLEL); a smaller one, or one without a
Frame_Content_Size, on the streaming executor.
--range OFF:LEN reads content bytes [OFF, OFF + LEN) of FILE, a zstd seekable
archive (a multi-frame file that ends with a seek table), decoding only the
entries the range touches; the range is clamped to the content's end and
written as bytes.  A file without a seek table is an error message and exit
status 1.  Not together with -D or --patch-from.
--verify-table with --range compares the seek table's checksum of every entry
the range touches inside the launch: an entry whose decoded bytes do not hash
to it ends the run with `Error: entry N: ChecksumWrong` (exit status 1), and
an archive whose table carries no checksums is an error.  --verify-table
without --range decodes every entry of the archive and compares it (as
`zstd -t` tests a file): one `Error: entry N: <status>` line per bad entry on
stderr, exit status 1 when there is one, nothing written.  --verify keeps its
meaning: the frames' own Content_Checksums.
--long accepts frames whose Window_Size is up to 2 GiB (F_LONG_WINDOW; the
default is the reference's 8 MiB limit): what `zstd --long` and `zstd
--patch-from` write for inputs past 8 MiB.
--rfc decodes frames as RFC 8878 and libzstd have them (F_RFC; the default is
the reference's decoder, which fails on a compressed block without sequences
and on some Huffman weight totals, and miscounts more than 32,511 sequences).
"""
from __future__ import annotations

import argparse
import sys

from . import _lib
from .batch import Dictionary, DictionarySet, Plan, chunk_sizes, decode_tensors, frames_index

# --patch-from: a frame of at least this Frame_Content_Size goes to the block-parallel executor (K4J_MIN_BLOCKS
# blocks of 128 KiB, zd_plan.h: the plain plans' own threshold in bytes the command line can see)
PATCH_BLOCK_PARALLEL_BYTES = 16 * (128 << 10)


def _plan_flags(a) -> int:
    """--verify, --long and --rfc as plan flags"""
    return ((_lib.F_VERIFY_CHECKSUM if a.verify else 0) | (_lib.F_LONG_WINDOW if a.long_window else 0) |
            (_lib.F_RFC if a.rfc else 0))


def _info(data: bytes) -> int:
    frames, blocks, st, _ = frames_index(data)
    for f in frames:
        if f["kind"] == 1:
            print(f"SkippableFrame(Skippable {{ magic: {f['magic']:#x}, data: {f['src_size'] - 8:#x} bytes }})")
            continue
        bs = blocks[f["first_block"]: f["first_block"] + f["num_blocks"]]
        kinds = ["Raw", "RLE", "Compressed"]
        cs = None if f["content_size"] == (1 << 64) - 1 else f["content_size"]
        did = None if f["dict_id"] == (1 << 64) - 1 else f["dict_id"]
        blist = ", ".join("%s(%#x)" % (kinds[b["type"]], b["block_size"]) for b in bs)
        chk = hex(f["checksum"]) if f["has_checksum"] else None
        print(f"ZStandardFrame(ZStandard {{ header: Header {{ content_checksum_flag: {bool(f['has_checksum'])}, "
              f"window_size: {f['window_size']:#x}, dictionnary_id: {did}, content_size: {cs} }}, "
              f"blocks: [{blist}], checksum: {chk} }})")
    if st != 0:
        print(f"Error: {_lib.status_name(st)}", file=sys.stderr)
        return 1
    return 0


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="zstd_decompressor", description="ZStandard decoder on MI355X (HIP)")
    ap.add_argument("filename", help="ZStandard file input, decompress it and output to stdout")
    ap.add_argument("-i", "--info", action="store_true", help="Dump information about frames instead of the output")
    ap.add_argument("-o", "--output", metavar="filename", help="Output to given file (overwriting) instead of stdout")
    ap.add_argument("-p", "--print-skippable", action="store_true", help="Output Skippable frames as well")
    ap.add_argument("--check-checksums", action="store_true",
                    help="verify Content_Checksum (XXH64) on the GPU; mismatches go to stderr (not in the reference)")
    ap.add_argument("--verify", action="store_true",
                    help="fail a frame whose decoded bytes do not match its Content_Checksum, as zstd -d does "
                         "(not in the reference)")
    ap.add_argument("-D", dest="dictionary", metavar="dict", action="append",
                    help="decode with this dictionary file, as zstd -D; repeat it for a set of dictionaries, "
                         "each frame choosing by its Dictionary_ID (not in the reference)")
    ap.add_argument("--patch-from", dest="patch_from", metavar="old",
                    help="decode the one frame of the input against this file as its prefix, as zstd --patch-from "
                         "(not in the reference; not together with -D)")
    ap.add_argument("--long", dest="long_window", action="store_true",
                    help="accept frames whose Window_Size is up to 2 GiB (default: 8 MiB, the reference's limit), "
                         "as written by zstd --long and by --patch-from on large files (not in the reference)")
    ap.add_argument("--rfc", action="store_true",
                    help="decode frames as RFC 8878 and libzstd have them, where the default keeps the reference's "
                         "departures from the format (not in the reference)")
    ap.add_argument("--range", dest="byte_range", metavar="OFF:LEN",
                    help="read LEN content bytes from offset OFF of a zstd seekable archive, decoding only the "
                         "entries they lie in (not in the reference; not together with -D or --patch-from)")
    ap.add_argument("--verify-table", dest="verify_table", action="store_true",
                    help="a zstd seekable archive: compare every decoded entry with its checksum in the seek table; "
                         "with --range the entries the range touches, without it the whole archive (not in the "
                         "reference)")
    return ap


def _range(a, data: bytes) -> int:
    """--range OFF:LEN: one range of a seekable archive, written as bytes."""
    from .seekable import SeekableArchive
    try:
        off, length = (int(v, 0) for v in a.byte_range.split(":"))
        if off < 0 or length < 0:
            raise ValueError
    except ValueError:
        print("Error: --range takes OFF:LEN, two non-negative integers", file=sys.stderr)
        return 2
    try:
        arc = SeekableArchive(data)
    except _lib.ZdError as e:
        print(f"Error: not a seekable archive: {e.name}", file=sys.stderr)
        return 1
    flags = _plan_flags(a)
    try:
        out = bytes(arc.read(off, length, flags=flags, verify_table=a.verify_table).cpu().numpy().tobytes())
    except _lib.ZdError as e:
        if a.verify_table and e.code == _lib.INVALID_ARG and not arc.has_checksums:
            print("Error: --verify-table: the seek table carries no checksums", file=sys.stderr)
        elif getattr(e, "entries", None):
            print(f"Error: entry {e.entries[0]}: {e.name}", file=sys.stderr)
        else:
            print(f"Error: {e.name}", file=sys.stderr)
        return 1
    finally:
        arc.close()
    if a.output:
        with open(a.output, "wb") as fo:
            fo.write(out)
    else:
        sys.stdout.buffer.write(out)
        sys.stdout.buffer.flush()
    return 0


def _verify_table(a, data: bytes) -> int:
    """--verify-table without --range: every entry of a seekable archive decoded
    and compared with the table's Checksum, one line per bad entry."""
    from .seekable import SeekableArchive
    try:
        arc = SeekableArchive(data)
    except _lib.ZdError as e:
        print(f"Error: not a seekable archive: {e.name}", file=sys.stderr)
        return 1
    try:
        flags = _plan_flags(a)
        entries, statuses = arc.verify_all(flags=flags)
    except ValueError as e:
        print(f"Error: --verify-table: {e}", file=sys.stderr)
        return 1
    finally:
        arc.close()
    for f, st in zip(entries, statuses):
        print(f"Error: entry {f}: {_lib.status_name(st)}", file=sys.stderr)
    return 1 if entries else 0


def _patch(a, data: bytes) -> int:
    """FILE against OLD: one chunk of a prefix batch, sized by the frame's own
    Frame_Content_Size, else by 128 KiB per block (what a batch reserves)."""
    import torch
    old = open(a.patch_from, "rb").read()
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else torch.empty(0, dtype=torch.uint8, device=dev)
    d_src = up(data)
    cap, fcs = 0, None
    if a.long_window:
        # (the host index takes no flags: the device's size query walks the chunk under the long limit, and as a
        # prefix batch walks it: an empty Raw literals section is accepted)
        sizes, _, exact = chunk_sizes([d_src.data_ptr()], [len(data)], dictionary=True, long_window=True, rfc=a.rfc)
        cap = int(sizes.cpu()[0])
        fcs = cap if int(exact.cpu()[0]) else None
    else:
        frames, blocks, st, _ = frames_index(data)
        for f in frames:
            if f["kind"] == 1:
                continue
            cs = f["content_size"]
            fcs = cs if cs != (1 << 64) - 1 else None
            cap = max(cap, cs if fcs is not None else (128 << 10) * max(f["num_blocks"], 1))
    d_dst = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    flags = _plan_flags(a)
    if fcs is not None and fcs >= PATCH_BLOCK_PARALLEL_BYTES:
        flags |= _lib.F_BLOCK_PARALLEL
    status, length = decode_tensors([d_src], [d_dst], flags=flags, prefixes=[up(old)])
    if status[0] != 0:
        print(f"Error: {_lib.status_name(status[0])}", file=sys.stderr)
        return 1
    out = bytes(d_dst[:length[0]].cpu().numpy().tobytes())
    if a.output:
        with open(a.output, "wb") as fo:
            fo.write(out)
    else:
        sys.stdout.buffer.write(out)
        sys.stdout.buffer.flush()
    return 0


def _dictionary(paths):
    """One -D: that Dictionary, as ever.  Several: a DictionarySet whose
    fallback is the one raw-content file, else the first."""
    ds = [Dictionary(open(p, "rb").read()) for p in paths]
    if len(ds) == 1:
        return ds[0]
    raw = [i for i, d in enumerate(ds) if d.raw_content]
    return DictionarySet(ds, fallback=raw[0] if len(raw) == 1 else 0)


def main(argv=None) -> int:
    a = _parser().parse_args(argv)
    data = open(a.filename, "rb").read()
    if a.info:
        return _info(data)
    if a.patch_from:
        if a.dictionary or a.byte_range is not None:
            print("Error: --patch-from and -D / --range exclude one another" if a.byte_range is not None else
                  "Error: --patch-from and -D exclude one another", file=sys.stderr)
            return 2
        return _patch(a, data)
    if a.byte_range is not None:
        if a.dictionary:
            print("Error: --range and -D exclude one another", file=sys.stderr)
            return 2
        return _range(a, data)
    if a.verify_table:
        if a.dictionary:
            print("Error: --verify-table and -D exclude one another", file=sys.stderr)
            return 2
        return _verify_table(a, data)
    import torch
    try:
        dictionary = _dictionary(a.dictionary) if a.dictionary else None
    except _lib.ZdError as e:
        print(f"Error: dictionary: {e.name}", file=sys.stderr)
        return 1
    flags = _plan_flags(a)
    if dictionary is not None:
        # a frame of --patch-from's threshold behind a dictionary: the plan may send its frames to the
        # block-parallel executor, each by the library's rule (the same bytes either way)
        sized = [f["content_size"] for f in frames_index(data)[0] if f["kind"] != 1]
        if any(cs != (1 << 64) - 1 and cs >= PATCH_BLOCK_PARALLEL_BYTES for cs in sized):
            flags |= _lib.F_DICT_BLOCK_PARALLEL
    plan = Plan(data, a.print_skippable,
                flags,
                dictionary=dictionary)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_src = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
    if data:
        d_src[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    cap = max(int(plan.info.out_bytes), 1)
    d_dst = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), cap, s)
    st, total, _, _, first = plan.results(d_dst.data_ptr(), s)
    if st != 0:
        print(f"Error: frame {first}: {_lib.status_name(st)}", file=sys.stderr)
        return 1
    if a.check_checksums:
        ok, _ = plan.checksums(d_dst.data_ptr(), s)
        for i, v in enumerate(ok):
            if v == 0:
                print(f"Warning: Bad checksum ! (frame {i})", file=sys.stderr)
    out = bytes(d_dst[:total].cpu().numpy().tobytes())
    try:
        text = out.decode("utf-8")
    except UnicodeDecodeError as e:
        print(f"thread 'main' panicked: called `Result::unwrap()` on an `Err` value: FromUtf8Error {{ {e} }}",
              file=sys.stderr)
        return 101
    if a.output:
        with open(a.output, "w", encoding="utf-8", newline="") as fo:
            fo.write(text)
    else:
        sys.stdout.write(text)
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
