"""MI355X-native mirror of the `zstd_decompressor` crate API
(AchilleBailly/zstd-decompressor, zstd-decompressor/src/lib.rs:2-9).

Module map (reference -> here):
  parsing.rs          -> parsing       ForwardByteParser, FrameIterator entry
  frame.rs            -> frame         Frame, ZStandard, Skippable, Header, FrameIterator
  block.rs            -> block         Block.parse / Block.decode(ctx)
  decoding_context.rs -> decoding_context  DecodingContext (GPU-resident)
  decoders/, literals.rs, sequences.rs -> HIP kernels behind the C ABI (include/zd.h)
Batch API (the hot path): batch.decompress / batch.Plan; batch.Batch for
scattered device chunks with per-chunk buffers and statuses; batch.chunk_sizes /
Batch.packed / batch.decompress_tensors when the decoded sizes are not known;
seekable.SeekableArchive for byte ranges of a seekable archive on the device;
multi.MultiFrameBatch / multi.decode_multi for chunks of several concatenated frames.
"""
from . import _lib
from ._lib import ZdError
from .parsing import ForwardByteParser
from .frame import Frame, FrameIterator, Header, Skippable, ZStandard, MAX_WIN_SIZE
from .block import Block
from .decoding_context import DecodingContext
from .batch import (Batch, Dictionary, DictionarySet, Plan, chunk_sizes, decode_tensors, decompress,
                    decompress_tensors, frames_index)
from .seekable import SeekableArchive, SeekReader
from .multi import MultiFrameBatch, decode_multi

__all__ = ["ZdError", "ForwardByteParser", "Frame", "FrameIterator", "Header", "Skippable", "ZStandard",
           "MAX_WIN_SIZE", "Block", "DecodingContext", "Batch", "Dictionary", "DictionarySet",
           "Plan", "chunk_sizes", "decode_tensors", "decompress", "decompress_tensors",
           "frames_index", "SeekableArchive", "SeekReader", "MultiFrameBatch", "decode_multi"]
