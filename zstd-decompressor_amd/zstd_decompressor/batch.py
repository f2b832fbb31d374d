"""Batch decode over the C ABI — the hot path.

`decompress` mirrors the CLI loop (src/main.rs:43-58) on host buffers;
`Plan` keeps input/output in HBM (torch tensors or raw device pointers) and is
what bench.py times; `Batch` decodes N chunks held at N device addresses, each
into its own device buffer with its own status (zd_batch, include/zd.h).
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import ZdError, FrameDesc, BlockDesc, PlanInfo


def frames_index(data: bytes, max_frames: int = 0):
    """zd_frames_index: ([frame dicts], [block dicts], status, consumed)."""
    L = _lib.lib()
    p, n, keep = _lib.buf(data)
    nf, nb, cons = C.c_size_t(), C.c_size_t(), C.c_size_t()
    L.zd_frames_index(p, n, None, 0, C.byref(nf), None, 0, C.byref(nb), C.byref(cons))
    fa = (FrameDesc * max(nf.value, 1))()
    ba = (BlockDesc * max(nb.value, 1))()
    st = L.zd_frames_index(p, n, fa, nf.value, C.byref(nf), ba, nb.value, C.byref(nb), C.byref(cons))
    frames = [{k: getattr(fa[i], k) for k, _ in FrameDesc._fields_} for i in range(nf.value)]
    blocks = [{k: getattr(ba[i], k) for k, _ in BlockDesc._fields_ if k != "_pad"} for i in range(nb.value)]
    return frames, blocks, st, cons.value


def run_plan(plan, p, n):
    """(status, output): zd_plan_decompress into a buffer sized from the plan;
    again with the size it reports when the output came out larger (a frame
    that decodes past its declared size is re-planned inside the call).  The
    output is read back with one memcpy (_lib.take), not an element-wise
    ctypes slice (seconds per 100 MB)."""
    L = _lib.lib()
    cap = max(plan.info.out_bytes, 1)
    for _ in range(2):
        out = (C.c_uint8 * cap)()
        ol = C.c_size_t()
        st = L.zd_plan_decompress(plan._h, p, n, out, cap, C.byref(ol))
        if st in (_lib.HIP, _lib.INVALID_ARG, _lib.NO_MEMORY):
            _lib.check(st, "zd_plan_decompress")
        if ol.value <= cap:
            break
        cap = ol.value
    return st, _lib.take(out, min(ol.value, cap))


class Dictionary:
    """zd_dict: a zstd dictionary (RFC 8878 5) on the current device, formatted
    (magic 0xEC30A437: ID, entropy tables, repeat offsets, content) or raw
    content (any other bytes).  Pass it to Plan / decompress /
    decompress_status as `dictionary=`; plans made with it keep it alive, so
    close() before they are closed is fine."""

    def __init__(self, data: bytes):
        L = _lib.lib()
        p, n, keep = _lib.buf(data)
        h = C.c_void_p()
        _lib.check(L.zd_dict_create(p, n, C.byref(h)), "zd_dict_create")
        self._h = h
        did, size, raw = C.c_uint32(), C.c_uint64(), C.c_int()
        rep = (C.c_uint64 * 3)()
        _lib.check(L.zd_dict_info(h, C.byref(did), C.byref(size), rep, C.byref(raw)), "zd_dict_info")
        self.dict_id, self.content_size = did.value, size.value
        self.repeat_offsets, self.raw_content = tuple(rep), bool(raw.value)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().zd_dict_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DictionarySet:
    """zd_dict_set: many dictionaries for one plan or batch, each frame
    choosing its own by the Dictionary_ID in its header.  dictionaries: open
    Dictionary objects with distinct IDs; fallback: index of the one for frames
    without an ID (a raw-content dictionary can only be that one), or -1: such
    frames decode with no dictionary.  Accepted wherever `dictionary=` is.  The
    set keeps its dictionaries' device data alive, plans and batches keep the
    set: close() in any order."""

    def __init__(self, dictionaries, fallback: int = 0):
        ds = list(dictionaries)
        for d in ds:
            if not isinstance(d, Dictionary):
                raise TypeError("Dictionary objects required")
        arr = (C.c_void_p * max(len(ds), 1))(*[d._h.value if d._h else None for d in ds])   # (a closed Dictionary: NULL, ZD_E_INVALID_ARG)
        h = C.c_void_p()
        _lib.check(_lib.lib().zd_dict_set_create(arr, len(ds), fallback, C.byref(h)), "zd_dict_set_create")
        self._h = h
        self.dict_ids = tuple(d.dict_id for d in ds)
        self.fallback = fallback

    def __len__(self):
        return len(self.dict_ids)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().zd_dict_set_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _decompress(data: bytes, flags: int, dictionary=None):
    """One plan (the host walk once) and zd_plan_decompress — what
    zd_decompress does, with the plan's output size read first."""
    p, n, keep = _lib.buf(data)
    plan = Plan(data, bool(flags & _lib.F_SKIPPABLE), flags & ~_lib.F_SKIPPABLE, dictionary=dictionary)
    try:
        return run_plan(plan, p, n)
    finally:
        plan.close()


def decompress(data: bytes, print_skippable: bool = False, dictionary=None, verify: bool = False,
               rfc: bool = False, flags: int = 0) -> bytes:
    """Decode every frame of `data` on the GPU (host in, host out);
    dictionary: a Dictionary every frame decodes with, or a DictionarySet;
    verify: a frame whose bytes do not hash to its Content_Checksum raises
    ZdError(CHECKSUM_WRONG), as libzstd fails such a frame; rfc: frames decode
    as RFC 8878 and libzstd have them (F_RFC), where the default is the
    reference's decoder, which fails or corrupts some frames libzstd writes;
    flags: extra plan flags, such as _lib.F_DICT_BLOCK_PARALLEL with
    dictionary= (large frames behind a dictionary on the block-parallel
    executor; the same bytes)."""
    flags |= ((_lib.F_SKIPPABLE if print_skippable else 0) | (_lib.F_VERIFY_CHECKSUM if verify else 0) |
              (_lib.F_RFC if rfc else 0))
    st, out = _decompress(data, flags, dictionary)
    _lib.check(st, "zd_decompress")
    return out


KEY_NONE = (1 << 64) - 1
PH_PARSE = 0


def decode_keyed(data: bytes, flags: int = 0):
    """(status, output of the frames before the first failure, error key):
    one plan and zd_plan_decompress; the key's phase (key >> 62: 0 parse, 1
    decode, 3 a limit) tells a table-description error, which the reference
    raises in Frame::parse, from an execution error it raises in decode."""
    plan = Plan(data, bool(flags & _lib.F_SKIPPABLE), flags & ~_lib.F_SKIPPABLE)
    try:
        p, n, keep = _lib.buf(data)
        st, out = run_plan(plan, p, n)
        return st, out, plan.refresh_info().error_key
    finally:
        plan.close()


def decompress_status(data: bytes, print_skippable: bool = False, flags: int = 0, dictionary=None):
    """(status, output of the frames before the first failure).  flags: extra
    zd_plan flags (_lib.F_BLOCK_PARALLEL / F_FRAME_SERIAL pick the executor);
    dictionary: a Dictionary every frame decodes with, or a DictionarySet."""
    return _decompress(data, (_lib.F_SKIPPABLE if print_skippable else 0) | flags, dictionary)


class Plan:
    """zd_plan: host index + device workspace for one byte range of frames."""

    def __init__(self, data: bytes, print_skippable: bool = False, flags: int = 0, dictionary=None):
        L = _lib.lib()
        self._data = data
        p, n, self._keep = _lib.buf(data)
        h = C.c_void_p()
        f = (_lib.F_SKIPPABLE if print_skippable else 0) | flags
        if dictionary is None:
            _lib.check(L.zd_plan_create(p, n, f, C.byref(h)), "zd_plan_create")
        else:
            if not getattr(dictionary, "_h", None):
                raise ValueError("the %s is closed" % type(dictionary).__name__)
            if isinstance(dictionary, DictionarySet):
                _lib.check(L.zd_plan_create_dicts(p, n, f, dictionary._h, C.byref(h)), "zd_plan_create_dicts")
            else:
                _lib.check(L.zd_plan_create_dict(p, n, f, dictionary._h, C.byref(h)), "zd_plan_create_dict")
        self._h = h
        self.info = PlanInfo()
        _lib.check(L.zd_plan_info_get(h, C.byref(self.info)), "zd_plan_info_get")

    @classmethod
    def from_device(cls, d_src: int, n: int, print_skippable: bool = False, flags: int = 0, stream: int = 0):
        """zd_plan_create_device: the same plan for n bytes resident in HBM at d_src
        (readable for n + 16 bytes); the frame/block header walk runs on the GPU."""
        self = cls.__new__(cls)
        L = _lib.lib()
        self._data, self._keep = None, None
        h = C.c_void_p()
        _lib.check(L.zd_plan_create_device(C.c_void_p(d_src), n, (_lib.F_SKIPPABLE if print_skippable else 0) | flags,
                                           C.c_void_p(stream), C.byref(h)), "zd_plan_create_device")
        self._h = h
        self.info = PlanInfo()
        _lib.check(L.zd_plan_info_get(h, C.byref(self.info)), "zd_plan_info_get")
        return self

    def set_profiling(self, on=True):
        """zd_plan_set_profiling: True / 1 every kernel timed one after another,
        2 the pipeline as it runs with events around its dominant launch, 0 off."""
        _lib.check(_lib.lib().zd_plan_set_profiling(self._h, int(on)))

    def refresh_info(self):
        """zd_plan_info again (the fields of the last decode / results)."""
        _lib.check(_lib.lib().zd_plan_info_get(self._h, C.byref(self.info)), "zd_plan_info_get")
        return self.info

    def decode_async(self, d_src: int, d_dst: int, dst_cap: int, stream: int = 0):
        """Launch the pipeline; pointers/stream are integers (e.g. tensor.data_ptr(),
        torch.cuda.current_stream().cuda_stream)."""
        _lib.check(_lib.lib().zd_decode_async(self._h, C.c_void_p(d_src), C.c_void_p(d_dst), dst_cap,
                                              C.c_void_p(stream)), "zd_decode_async")

    def results(self, d_dst: int, stream: int = 0):
        """(status, total_len, per-frame statuses, per-frame lengths, first error frame)."""
        nf = self.info.nframes
        st_arr = (C.c_int32 * max(nf, 1))()
        ln_arr = (C.c_uint64 * max(nf, 1))()
        total, first = C.c_uint64(), C.c_int32()
        st = _lib.lib().zd_plan_results(self._h, C.c_void_p(d_dst), C.c_void_p(stream), st_arr, ln_arr,
                                        C.byref(total), C.byref(first))
        if st in (_lib.HIP, _lib.INVALID_ARG):
            _lib.check(st, "zd_plan_results")
        return st, total.value, list(st_arr)[:nf], list(ln_arr)[:nf], first.value

    def checksums(self, d_dst: int, stream: int = 0):
        """After results(): (ok per frame: 1 match / 0 mismatch / -1 none, XXH64 digests),
        computed on the GPU (zd_plan_checksums; an extra, the reference never enforces it)."""
        nf = self.info.nframes
        ok = (C.c_int32 * max(nf, 1))()
        h = (C.c_uint64 * max(nf, 1))()
        _lib.check(_lib.lib().zd_plan_checksums(self._h, C.c_void_p(d_dst), C.c_void_p(stream), ok, h),
                   "zd_plan_checksums")
        return list(ok)[:nf], list(h)[:nf]

    def kernel_times(self):
        names = (C.c_char_p * 8)()
        ms = (C.c_float * 8)()
        n = C.c_int()
        _lib.check(_lib.lib().zd_plan_kernel_times(self._h, names, ms, 8, C.byref(n)))
        return {names[i].decode(): ms[i] for i in range(n.value)}

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().zd_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _u64_array(values, n: int):
    """n integers as a ctypes uint64 array (array.array packs a list far faster
    than ctypes' own constructor: 65,536 chunks in a millisecond or two)."""
    import array
    try:
        a = array.array("Q", values)                            # plain ints
    except TypeError:
        a = array.array("Q", [int(v or 0) for v in values])     # None for a null pointer, numpy scalars
    return (C.c_uint64 * n).from_buffer(a) if n else (C.c_uint64 * 1)()


def _device_arrays(arrs, nchunks, lists=True):
    """(n, device addresses, tensors to keep) of per-chunk arrays given as
    contiguous 1-D int64 / uint64 device tensors, device addresses (with
    nchunks), or (unless lists=False) Python lists, which are uploaded as one
    int64 tensor each (the upload is waited for, so the arrays are readable on
    any stream)."""
    n, addr, keep, uploaded = nchunks, [], [], False
    for a in arrs:
        if isinstance(a, int):
            addr.append(a)
            continue
        import torch
        if lists and isinstance(a, (list, tuple)):
            a = torch.tensor([int(v or 0) for v in a], dtype=torch.int64,
                             device=torch.device("cuda", torch.cuda.current_device()))
            uploaded = True
        if not (isinstance(a, torch.Tensor) and a.is_cuda and a.is_contiguous() and a.dim() == 1
                and a.dtype in (torch.int64, torch.uint64)):
            raise ValueError("contiguous 1-D int64 / uint64 device tensors%s required"
                             % (", device addresses or lists" if lists else ", or device addresses,"))
        if n is None:
            n = a.numel()
        if a.numel() != n:
            raise ValueError("the arrays and nchunks differ in length")
        addr.append(a.data_ptr() if n else 0)
        keep.append(a)
    if n is None:
        raise ValueError("nchunks is required when every array is a raw address")
    if uploaded:
        torch.cuda.current_stream().synchronize()
    return n, addr, keep


def chunk_sizes(src_ptrs, src_sizes, nchunks=None, dictionary: bool = False, stream=None, long_window: bool = False,
                rfc: bool = False, multi_frame: bool = False):
    """zd_chunk_sizes_device: what each chunk needs of its destination, asked
    on the device.  src_ptrs / src_sizes as in Batch.from_device (device
    tensors, or addresses with `nchunks`).  Returns three device tensors
    (sizes int64, statuses int32, exact uint8): a chunk's reserve (its usable
    Frame_Content_Size, exact 1, else 128 KiB per compressed block + its raw
    and RLE blocks, exact 0; 0 for a failing or empty chunk) and the status of
    its header walk.  dictionary=True when the chunks will be decoded with a
    Dictionary or DictionarySet, long_window=True when with F_LONG_WINDOW (a
    Window_Size up to 2 GiB is then no failure), rfc=True when with F_RFC (the
    walk reads section headers as that flag does), multi_frame=True when by a
    MultiFrameBatch (a chunk may then hold several frames: the sum of its
    sub-chunks' reserves, exact when all of them are, the first failing
    sub-chunk's status).  The kernel is queued on
    `stream` (torch's current stream by default) and nothing is synchronised."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    n, addr, keep = _device_arrays((src_ptrs, src_sizes), nchunks)
    dev = keep[0].device if keep else torch.device("cuda", torch.cuda.current_device())
    sizes = torch.empty(n, dtype=torch.int64, device=dev)
    statuses = torch.empty(n, dtype=torch.int32, device=dev)
    exact = torch.empty(n, dtype=torch.uint8, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr() if n else 0)
    _lib.check(_lib.lib().zd_chunk_sizes_device(C.c_void_p(addr[0]), C.c_void_p(addr[1]), n,
                                                (_lib.SIZES_DICT if dictionary else 0) |
                                                (_lib.SIZES_LONG_WINDOW if long_window else 0) |
                                                (_lib.SIZES_RFC if rfc else 0) |
                                                (_lib.SIZES_MULTI_FRAME if multi_frame else 0), ptr(sizes), ptr(statuses),
                                                ptr(exact), C.c_void_p(stream)), "zd_chunk_sizes_device")
    return sizes, statuses, exact


def _batch_info(h):
    info = _lib.BatchInfo2()
    _lib.check(_lib.lib().zd_batch_info_get_sized(h, C.byref(info), C.sizeof(info)), "zd_batch_info_get_sized")
    return info


def _with_dictionary(name, dictionary):
    """(entry point, handle) for a batch made with `dictionary`: `name` with
    a Dictionary's handle or None, name + "_dicts" with a DictionarySet's.  A
    closed dictionary or set is a ValueError."""
    if dictionary is None:
        return name, None
    if not getattr(dictionary, "_h", None):
        raise ValueError("the %s is closed" % type(dictionary).__name__)
    return (name + "_dicts" if isinstance(dictionary, DictionarySet) else name), dictionary._h


class Batch:
    """zd_batch: N independently compressed chunks at N device addresses, each
    decoded into its own device buffer with its own status (dictionary: a
    Dictionary every chunk decodes with, or a DictionarySet; prefixes: a pair
    (ptrs, sizes), chunk i decodes against the sizes[i] bytes at device address
    ptrs[i] -- its own raw-content prefix, as ZSTD_DCtx_refPrefix gives a frame;
    size 0, address None or 0: no prefix.  Prefixes are read by decode_async
    where they lie, must stay valid while the batch lives and must not overlap
    a destination; not together with dictionary=; parents: a delta chain,
    zd_batch_create_chain -- parents[i] is -1, or the index of the chunk whose
    decoded output OF THE SAME LAUNCH is chunk i's prefix (its prefix size must
    then be 0; prefixes may be None when no chunk has an external one).  A chunk
    behind a failed ancestor is NOT_DECODED; `chain_info` gives the levels).
    flags: with prefixes= or parents=, _lib.F_AUTO_EXECUTOR routes each chunk's
    frame on its own (large frames to the block-parallel executor, the rest to
    the streaming one); `info.k4j_chunks` counts the former in any batch.
    With dictionary=, _lib.F_DICT_BLOCK_PARALLEL lets frames run on the
    block-parallel executor: all with a compressed block under
    F_BLOCK_PARALLEL, none under F_FRAME_SERIAL, else by the same rule.

    src_ptrs / dst_ptrs are device addresses (integers, e.g. tensor.data_ptr()),
    src_sizes / dst_caps byte counts.  A chunk holds one zstd frame (skippable
    frames around it are skipped).  The sources are copied at creation (they
    need no padding and may be released afterwards); the destinations must
    stay valid while the batch decodes."""

    def __init__(self, src_ptrs, src_sizes, dst_ptrs, dst_caps, flags: int = 0, dictionary=None, stream: int = 0,
                 prefixes=None, parents=None):
        n = len(src_ptrs)
        if not (len(src_sizes) == len(dst_ptrs) == len(dst_caps) == n):
            raise ValueError("src_ptrs, src_sizes, dst_ptrs and dst_caps differ in length")
        name, dh = _with_dictionary("zd_batch_create", dictionary)
        if (prefixes is not None or parents is not None) and dictionary is not None:
            raise ValueError("prefixes= / parents= and dictionary= exclude one another")
        sp, ss, dp, dc = (_u64_array(v, n) for v in (src_ptrs, src_sizes, dst_ptrs, dst_caps))
        vpp = C.POINTER(C.c_void_p)
        pp = ps = None
        if prefixes is not None:
            pptrs, psizes = prefixes
            if not (len(pptrs) == len(psizes) == n):
                raise ValueError("the prefixes and the chunks differ in length")
            pp, ps = _u64_array(pptrs, n), _u64_array(psizes, n)
        if parents is not None:
            # a chain batch (zd_batch_create_chain): parents[i] = -1, or the chunk whose output of the
            # same launch is chunk i's prefix
            if len(parents) != n:
                raise ValueError("the parents and the chunks differ in length")
            import array
            pa = array.array("q", [int(v) for v in parents])
            par = (C.c_int64 * n).from_buffer(pa) if n else (C.c_int64 * 1)()
            self._create("zd_batch_create_chain", n, C.cast(sp, vpp), ss, C.cast(dp, vpp), dc,
                         C.cast(pp, vpp) if pp is not None else None, ps, par, n, flags, C.c_void_p(stream))
        elif prefixes is not None:
            self._create("zd_batch_create_prefix", n, C.cast(sp, vpp), ss, C.cast(dp, vpp), dc, C.cast(pp, vpp), ps,
                         n, flags, C.c_void_p(stream))
        else:
            self._create(name, n, C.cast(sp, vpp), ss, C.cast(dp, vpp), dc, n, flags, dh, C.c_void_p(stream))

    def _create(self, name, n, *args):
        """Calls the zd_batch_create* entry point `name` (the handle it
        returns is its last argument, added here) and takes the batch over."""
        h = C.c_void_p()
        _lib.check(getattr(_lib.lib(), name)(*args, C.byref(h)), name)
        self._h = h
        self.nchunks = n
        self.info = _batch_info(h)

    @classmethod
    def from_device(cls, src_ptrs, src_sizes, dst_ptrs, dst_caps, nchunks=None, flags: int = 0, dictionary=None,
                    stream: int = 0, prefixes=None, parents=None):
        """zd_batch_create_device: the same batch from a chunk table that is on
        the device.  Each of the four arrays is a contiguous int64 / uint64
        device tensor of one entry a chunk, or the device address of such an
        array (an integer) with `nchunks` given; they must be readable on
        `stream` and may be released when this returns.  Layout, walk, capacity
        checks and descriptors are built on the GPU.  A bad entry (a NULL
        address with a non-zero count) fails its own chunk with INVALID_ARG
        instead of the call, and overlapping destinations are not checked: the
        caller keeps them disjoint.  `.info.device_built` is 1.
        prefixes: a pair (ptrs, sizes) of two more such arrays, chunk i's own
        prefix (zd_batch_create_device_prefix; not together with dictionary=);
        a NULL prefix address with a non-zero size fails its own chunk, and
        keeping prefixes and destinations apart is the caller's duty.
        parents: one more such array, int64 (zd_batch_create_device_chain; with
        or without prefixes=): chunk i's parent in the batch, or -1.  A bad
        entry, a cycle or a chain deeper than 255 fails its own chunks with
        INVALID_ARG."""
        if (prefixes is not None or parents is not None) and dictionary is not None:
            raise ValueError("prefixes= / parents= and dictionary= exclude one another")
        arrs = (src_ptrs, src_sizes, dst_ptrs, dst_caps) + (tuple(prefixes) if prefixes is not None else ())
        if len(arrs) not in (4, 6):
            raise ValueError("prefixes is a pair (ptrs, sizes)")
        if parents is not None:
            arrs = arrs + (parents,)
        n, addr, keep = _device_arrays(arrs, nchunks, lists=False)
        name, dh = _with_dictionary("zd_batch_create_device", dictionary)
        self = cls.__new__(cls)
        ptrs = [C.c_void_p(a) for a in addr]
        if parents is not None:
            if prefixes is None:
                ptrs[4:4] = [None, None]
            self._create("zd_batch_create_device_chain", n, *ptrs, n, flags, C.c_void_p(stream))
        elif prefixes is not None:
            self._create("zd_batch_create_device_prefix", n, *ptrs, n, flags, C.c_void_p(stream))
        else:
            self._create(name, n, *ptrs, n, flags, dh, C.c_void_p(stream))
        return self

    @classmethod
    def packed(cls, src_ptrs, src_sizes, nchunks=None, align: int = 16, flags: int = 0, dictionary=None,
               stream: int = 0):
        """zd_batch_create_device_packed: a batch made from sources only, which
        lays its outputs out itself in one buffer.  src_ptrs / src_sizes as in
        from_device (device tensors, or addresses with `nchunks`); Python lists
        are uploaded as one int64 tensor each.  Chunk i's capacity is its
        reserve (chunk_sizes) and its place a multiple of `align` (a power of
        two up to 4096) from the buffer's base: `.out_bytes` is the buffer's
        size, output_layout() the two device arrays, bind_output() gives the
        buffer.  A frame without a usable Frame_Content_Size gets its bound, so
        there is slack after it: results() tells the lengths."""
        n, addr, keep = _device_arrays((src_ptrs, src_sizes), nchunks)
        name, dh = _with_dictionary("zd_batch_create_device_packed", dictionary)
        self = cls.__new__(cls)
        self._create(name, n, C.c_void_p(addr[0]), C.c_void_p(addr[1]), n, align, flags, dh, C.c_void_p(stream))
        ob = C.c_uint64()
        _lib.check(_lib.lib().zd_batch_output_layout(self._h, C.byref(ob), None, None), "zd_batch_output_layout")
        self.out_bytes = ob.value
        return self

    @property
    def chain_info(self):
        """zd_batch_chain_info: (levels, links) of a batch made with parents= --
        the chain's levels (1 when no chunk has a parent) and the chunks with a
        parent.  ZdError(INVALID_ARG) on any other batch."""
        lv, ln = C.c_uint32(), C.c_uint64()
        _lib.check(_lib.lib().zd_batch_chain_info(self._h, C.byref(lv), C.byref(ln)), "zd_batch_chain_info")
        return lv.value, ln.value

    def output_layout(self):
        """A packed batch's (device address of the uint64 offsets, device address
        of the uint64 capacities), nchunks entries each, owned by the batch."""
        off, cap = C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().zd_batch_output_layout(self._h, None, C.byref(off), C.byref(cap)),
                   "zd_batch_output_layout")
        return off.value or 0, cap.value or 0

    def bind_output(self, out, cap=None):
        """zd_batch_bind_output: the packed batch decodes into `out`, a
        contiguous uint8 device tensor or a device address with `cap` bytes.
        Takes effect at the next decode_async; call results() / checksums() of
        a decode before binding another buffer."""
        if isinstance(out, int):
            if cap is None:
                raise ValueError("cap is required with a raw address")
            ptr = out
        else:
            import torch
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8):
                raise ValueError("a contiguous uint8 device tensor, or a device address with cap, required")
            ptr = out.data_ptr() if out.numel() else 0
            if cap is None:
                cap = out.numel()
            elif cap > out.numel():
                raise ValueError("cap exceeds the tensor")
        _lib.check(_lib.lib().zd_batch_bind_output(self._h, C.c_void_p(ptr), cap), "zd_batch_bind_output")

    def decode_async(self, stream: int = 0):
        """Launch the decode of every chunk (no allocation, no host synchronisation)."""
        _lib.check(_lib.lib().zd_batch_decode_async(self._h, C.c_void_p(stream)), "zd_batch_decode_async")

    def device_results(self):
        """(device address of the int32 statuses, device address of the uint64
        lengths): written by the last kernel decode_async queues."""
        st, ln = C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().zd_batch_device_results(self._h, C.byref(st), C.byref(ln)), "zd_batch_device_results")
        return st.value or 0, ln.value or 0

    def device_checksums(self):
        """(device address of the uint64 XXH64 digests, device address of the
        int8 ok values: 1 match / 0 mismatch / -1 none or not decoded) of a
        batch made with _lib.F_VERIFY_CHECKSUM: written by the verification
        pass decode_async queues before the result arrays."""
        h, ok = C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().zd_batch_device_checksums(self._h, C.byref(h), C.byref(ok)),
                   "zd_batch_device_checksums")
        return h.value or 0, ok.value or 0

    def results(self, stream: int = 0):
        """(statuses, lengths) per chunk, after waiting for `stream`."""
        n = self.nchunks
        st = (C.c_int32 * max(n, 1))()
        ln = (C.c_uint64 * max(n, 1))()
        bad = C.c_uint64()
        _lib.check(_lib.lib().zd_batch_results(self._h, C.c_void_p(stream), st, ln, n, C.byref(bad)),
                   "zd_batch_results")
        return list(st)[:n], list(ln)[:n]

    def checksums(self, stream: int = 0):
        """(ok per chunk: 1 match / 0 mismatch / -1 none or not decoded, XXH64 digests)."""
        n = self.nchunks
        ok = (C.c_int32 * max(n, 1))()
        h = (C.c_uint64 * max(n, 1))()
        _lib.check(_lib.lib().zd_batch_checksums(self._h, C.c_void_p(stream), ok, h), "zd_batch_checksums")
        return list(ok)[:n], list(h)[:n]

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().zd_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_tensors(srcs, dsts, dictionary=None, flags: int = 0, prefixes=None, parents=None):
    """Decode uint8 device tensors srcs[i] (one chunk each) into dsts[i] on
    torch's current stream: (statuses, lengths).  prefixes: one entry a chunk,
    a uint8 device tensor (the chunk's own prefix, read in place) or None.
    parents: one entry a chunk, -1 or the index of the chunk whose output of
    this decode is the chunk's prefix (a delta chain; Batch parents=)."""
    import torch
    if len(srcs) != len(dsts):
        raise ValueError("srcs and dsts differ in length")
    if prefixes is not None and len(prefixes) != len(srcs):
        raise ValueError("srcs and prefixes differ in length")
    for t in list(srcs) + list(dsts) + [p for p in (prefixes or ()) if p is not None]:
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("contiguous uint8 device tensors required")
    stream = torch.cuda.current_stream().cuda_stream
    pfx = None
    if prefixes is not None:
        pfx = ([p.data_ptr() if p is not None and p.numel() else 0 for p in prefixes],
               [p.numel() if p is not None else 0 for p in prefixes])
    b = Batch([t.data_ptr() if t.numel() else 0 for t in srcs], [t.numel() for t in srcs],
              [t.data_ptr() if t.numel() else 0 for t in dsts], [t.numel() for t in dsts],
              flags=flags, dictionary=dictionary, stream=stream, prefixes=pfx, parents=parents)
    try:
        b.decode_async(stream)
        return b.results(stream)
    finally:
        b.close()


def _read_u64(d_ptr: int, n: int):
    """n uint64 words at a device address, as a list (a blocking hipMemcpy of
    the HIP runtime the process already runs: torch's own, else the system's)."""
    import os
    import torch
    if not n:
        return []
    rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = C.CDLL(rt if os.path.exists(rt) else "libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    words = (C.c_uint64 * n)()
    if hip.hipMemcpy(words, C.c_void_p(d_ptr), 8 * n, 2) != 0:     # hipMemcpyDeviceToHost
        raise ZdError(_lib.HIP, "hipMemcpy")
    return list(words)


def decompress_tensors(srcs, dictionary=None, flags: int = 0, align: int = 16):
    """Decode uint8 device tensors srcs[i] (one chunk each) without knowing
    their sizes: a packed batch (Batch.packed) over them, one uint8 tensor of
    its out_bytes, the decode on torch's current stream.  Returns (outs,
    statuses): outs[i] is a view of chunk i's decoded bytes in that tensor at
    the chunk's offset (a multiple of `align`), empty for a failing chunk."""
    import torch
    for t in srcs:
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("contiguous uint8 device tensors required")
    n = len(srcs)
    dev = srcs[0].device if n else torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    b = Batch.packed([t.data_ptr() if t.numel() else 0 for t in srcs], [t.numel() for t in srcs], align=align,
                     flags=flags, dictionary=dictionary, stream=stream)
    try:
        out = torch.empty(b.out_bytes, dtype=torch.uint8, device=dev)
        b.bind_output(out)
        b.decode_async(stream)
        statuses, lengths = b.results(stream)
        offs = _read_u64(b.output_layout()[0], n)
        outs = [out[offs[i]:offs[i] + lengths[i]] for i in range(n)]
        return outs, statuses
    finally:
        b.close()
