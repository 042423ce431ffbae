"""xz_amd -- MI355X-native LZMA2 Block encoder (Python plumbing over the C ABI).

The product is ``libxz_amd.so`` (HIP kernels for gfx950 + plain-C host layer,
see include/xz_amd.h).  This module only binds it with ctypes and uses torch
for device memory, streams and torch.distributed.  There is no CPU fallback:
if the library or a GPU is missing the calls raise.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("XZ_AMD_LIB") or os.path.join(_HERE, "libxz_amd.so")   # env override: A/B builds

CHECK_NONE, CHECK_CRC32, CHECK_CRC64, CHECK_SHA256 = 0, 1, 4, 10
MF_HC3, MF_HC4, MF_BT4 = 0x03, 0x04, 0x14
PRESET_EXTREME = 0x80000000
SPAN_WHOLE_BLOCK = 0xFFFFFFFF
SPAN_DEFAULT = 0
SPAN_AUTO = 1
F_BLOCKS_ONLY = 1
F_SEGMENTS = 2
F_KEEP_RESUME = 4
F_VERIFY = 8
F_REPAIR = 16
F_SINGLE = 32
F_AUTO_DELTA = 64
AUTO_DELTA_DISTANCES = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32)     # candidates of the automatic delta filter, 0 = none
DEBUG_DELTA_HIST, DEBUG_DELTA_DIST = 19, 20
F_AUTO_BCJ = 128
F_AUTO_LCLP = 256
DEBUG_LCLP_HIST, DEBUG_LCLP_PROPS = 23, 24
AUTO_BCJ_KINDS = (4, 0x0A)           # candidates of the automatic BCJ filter: x86, ARM64 (.xz filter ids)
AUTO_BCJ_BUCKETS = 4096
DEBUG_BCJ_HIST, DEBUG_BCJ_KIND = 21, 22
VSTEPS = ("none", "grammar", "decode", "check", "compare")     # XZAMD_VSTEP_*
NO_BLOCK = 0xFFFFFFFFFFFFFFFF
BCJ_X86 = 4
BCJ_ARM64 = 0x0A
BCJ_RISCV = 0x0B
BCJ_POWERPC, BCJ_IA64, BCJ_ARM, BCJ_ARMTHUMB, BCJ_SPARC = 5, 6, 7, 8, 9


def filter_delta(dist):
    """xzamd_lzma_options.bcj value of a delta filter (dist 1..256) in front of LZMA2."""
    return 3 | ((dist - 1) << 8)



class LzmaOptions(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "dict_size", "lc", "lp", "pb", "mode", "nice_len", "mf", "depth",
        "gpu_mf", "gpu_nice_len", "gpu_depth", "span_size", "gpu_sa_window", "gpu_parser", "bcj",
        "gpu_sa_depth", "span_cost", "span_bits", "enc_span_bits", "bcj2", "bcj3", "part_iters")]


class Stats(C.Structure):
    _fields_ = [("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("blocks", C.c_uint64),
                ("spans", C.c_uint64), ("batches", C.c_uint64), ("blocks_stored", C.c_uint64),
                ("ms_chains", C.c_float), ("ms_encode", C.c_float), ("ms_crc", C.c_float),
                ("ms_assemble", C.c_float), ("ms_total", C.c_float), ("encode_launches", C.c_uint32),
                ("ms_find", C.c_float), ("span_size", C.c_uint32), ("ms_find_overlapped", C.c_float),
                ("span_cost_used", C.c_uint32), ("ms_plan", C.c_float), ("wave_slots", C.c_uint32),
                ("enc_spans", C.c_uint64), ("ms_seed", C.c_float), ("ms_parse", C.c_float), ("ms_code", C.c_float), ("ms_iter1", C.c_float),
                ("ms_verify", C.c_float), ("batches_ahead", C.c_uint32)]


class VerifyReport(C.Structure):
    """xzamd_verify_report: what the last verification of a context found."""
    _fields_ = [("units", C.c_uint64), ("blocks", C.c_uint64), ("records_used", C.c_uint64), ("first_bad_block", C.c_uint64),
                ("mismatching_words", C.c_uint64), ("table_used", C.c_uint32), ("first_bad_step", C.c_uint32),
                ("ms_verify", C.c_float), ("reserved_", C.c_uint32)]


class RepairReport(C.Structure):
    """xzamd_repair_report: what the last repair of a context did."""
    _fields_ = [("blocks", C.c_uint64), ("blocks_bad", C.c_uint64), ("blocks_reencoded", C.c_uint64),
                ("blocks_stored", C.c_uint64), ("size_before", C.c_uint64), ("size_after", C.c_uint64),
                ("passes", C.c_uint32), ("ms_repair", C.c_float), ("ms_verify_passes", C.c_float),
                ("ms_reencode", C.c_float), ("ms_splice", C.c_float), ("reserved_", C.c_uint32)]


class ForwardReport(C.Structure):
    """xzamd_forward_report: how far a forward decode read and why it stopped."""
    _fields_ = [(n, C.c_uint64) for n in ("streams", "blocks", "blocks_delivered", "consumed", "stop_offset")] + \
               [(n, C.c_uint32) for n in ("stop", "code", "step", "reserved_")]


FWD_CONCATENATED = 1
FWD_END, FWD_TRUNCATED, FWD_DEFECT, FWD_OUT_FULL = 1, 2, 3, 4


class BlockInfo(C.Structure):
    _fields_ = [("unpadded_size", C.c_uint64), ("uncompressed_size", C.c_uint64),
                ("out_offset", C.c_uint64), ("total_size", C.c_uint64)]


class XzStream(C.Structure):
    """xzamd_xz_stream: one Stream of an .xz file."""
    _fields_ = [(n, C.c_uint64) for n in ("offset", "size", "padding", "first_block", "block_count",
                                          "uncompressed_offset", "uncompressed_size")] + \
               [("check", C.c_uint32), ("reserved_", C.c_uint32)]


class XzBlock(C.Structure):
    """xzamd_xz_block: one Block of an .xz file."""
    _fields_ = [(n, C.c_uint64) for n in ("header_offset", "unpadded_size", "total_size", "uncompressed_size",
                                          "uncompressed_offset")] + \
               [("stream", C.c_uint32), ("filter_count", C.c_uint32), ("filter_ids", C.c_uint32 * 4)]


_lib = None


def lib():
    """Load libxz_amd.so (built in-tree by ``make -C xz_amd/csrc`` / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C xz_amd/csrc` "
                "(there is no CPU fallback for the encoder)")
        try:
            # torch brings its own copy of the HIP runtime; when libxz_amd.so (linked against /opt/rocm) is
            # loaded first, a later `import torch` puts a second runtime into the process and device
            # initialisation fails.  Loading torch first makes the linker reuse its runtime for ours.
            import torch  # noqa: F401
        except ImportError:
            pass
        l = C.CDLL(LIB_PATH)
        l.xzamd_lzma_preset.argtypes = [C.POINTER(LzmaOptions), C.c_uint32]
        l.xzamd_mt_block_size.restype = C.c_uint64
        l.xzamd_mt_block_size.argtypes = [C.POINTER(LzmaOptions)]
        l.xzamd_block_buffer_bound.restype = C.c_uint64
        l.xzamd_block_buffer_bound.argtypes = [C.c_uint64]
        l.xzamd_stream_buffer_bound.restype = C.c_uint64
        l.xzamd_stream_buffer_bound.argtypes = [C.c_uint64, C.c_uint64]
        l.xzamd_ctx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        l.xzamd_ctx_destroy.argtypes = [C.c_void_p]
        l.xzamd_ctx_set_batch_bytes.argtypes = [C.c_void_p, C.c_uint64]
        l.xzamd_last_error.restype = C.c_char_p
        l.xzamd_last_error.argtypes = [C.c_void_p]
        l.xzamd_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        l.xzamd_stream_encode_device.argtypes = [
            C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(LzmaOptions), C.c_int,
            C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(BlockInfo),
            C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        l.xzamd_frame_header.restype = C.c_uint64
        l.xzamd_frame_header.argtypes = [C.c_void_p, C.c_int]
        l.xzamd_frame_index_footer.restype = C.c_uint64
        l.xzamd_frame_index_footer.argtypes = [C.c_void_p, C.c_uint64, C.c_int,
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64]
        l.xzamd_stream_decode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                 C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                                 C.POINTER(C.c_uint64), C.c_void_p]
        if hasattr(l, "xzamd_file_index_host"):         # an older library (XZ_AMD_LIB, A/B runs) lacks the file entries
            idx_args = [C.c_void_p, C.c_uint64, C.POINTER(XzStream), C.c_uint64, C.POINTER(C.c_uint64),
                        C.POINTER(XzBlock), C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
            l.xzamd_file_index_host.argtypes = idx_args
            l.xzamd_file_index_device.argtypes = [C.c_void_p] + idx_args
            l.xzamd_file_decode_device.argtypes = l.xzamd_stream_decode_device.argtypes
            l.xzamd_file_decode_range_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                                         C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                                         C.POINTER(C.c_uint64), C.c_void_p]
            l.xzamd_debug_file_counters_.restype = None
            l.xzamd_debug_file_counters_.argtypes = [C.POINTER(C.c_uint64)]
        if hasattr(l, "xzamd_file_decode_forward_device"):   # (an older library lacks the forward reader)
            l.xzamd_file_decode_forward_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64,
                                                           C.POINTER(C.c_uint64), C.POINTER(ForwardReport), C.c_void_p]
            l.xzamd_debug_forward_counters_.restype = None
            l.xzamd_debug_forward_counters_.argtypes = [C.POINTER(C.c_uint64)]
        if hasattr(l, "xzamd_crc32_combine"):           # (an older library lacks the single-Block encoder)
            l.xzamd_crc32_combine.restype = C.c_uint32
            l.xzamd_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
            l.xzamd_crc64_combine.restype = C.c_uint64
            l.xzamd_crc64_combine.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
        if hasattr(l, "xzamd_stream_verify_device"):    # (an older library lacks the verified encode)
            l.xzamd_stream_verify_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                     C.POINTER(VerifyReport), C.c_void_p]
            l.xzamd_get_verify_report.restype = None
            l.xzamd_get_verify_report.argtypes = [C.c_void_p, C.POINTER(VerifyReport)]
            l.xzamd_debug_resume_poke_.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32]
            l.xzamd_debug_resume_peek_.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        if hasattr(l, "xzamd_stream_repair_device"):    # (an older library lacks the per-Block verification and the repair)
            l.xzamd_stream_verify_blocks_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                            C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                                            C.POINTER(VerifyReport), C.c_void_p]
            l.xzamd_stream_repair_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                                     C.POINTER(LzmaOptions), C.POINTER(C.c_uint64),
                                                     C.POINTER(RepairReport), C.c_void_p]
            l.xzamd_get_repair_report.restype = None
            l.xzamd_get_repair_report.argtypes = [C.c_void_p, C.POINTER(RepairReport)]
        if hasattr(l, "xzamd_chains_repair_device"):    # (an older library lacks the bare chunk chains)
            l.xzamd_chains_verify_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(BlockInfo), C.c_uint64,
                                                     C.POINTER(LzmaOptions), C.c_int, C.c_void_p, C.c_uint64,
                                                     C.c_void_p, C.c_uint64, C.POINTER(VerifyReport), C.c_void_p]
            l.xzamd_chains_repair_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(BlockInfo),
                                                     C.c_uint64, C.POINTER(LzmaOptions), C.c_int, C.c_void_p, C.c_uint64,
                                                     C.POINTER(C.c_uint64), C.POINTER(RepairReport), C.c_void_p]
        if hasattr(l, "xzamd_auto_delta_device"):       # (an older library lacks the automatic delta filter)
            l.xzamd_auto_delta_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32),
                                                  C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        if hasattr(l, "xzamd_auto_lclp_device"):        # (an older library lacks the automatic literal context)
            l.xzamd_auto_lclp_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                                 C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        if hasattr(l, "xzamd_auto_bcj_device"):         # (an older library lacks the automatic BCJ filter)
            l.xzamd_auto_bcj_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32),
                                                C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        l.xzamd_debug_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
        l.xzamd_trace_enable.argtypes = [C.c_void_p, C.c_uint32]
        l.xzamd_trace_read.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        l.xzamd_corpus_lorem.argtypes = [C.c_void_p, C.c_uint64]
        l.xzamd_corpus_text.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int]
        l.xzamd_corpus_tar.restype = C.c_uint64
        l.xzamd_corpus_tar.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64]
        l.xzamd_version.restype = C.c_char_p
        _lib = l
    return _lib


def preset_options(preset, span_size=SPAN_DEFAULT):
    o = LzmaOptions()
    if lib().xzamd_lzma_preset(C.byref(o), preset) != 0:
        raise ValueError(f"invalid preset {preset:#x}")
    o.span_size = span_size
    return o


def mt_block_size(opts):
    return lib().xzamd_mt_block_size(C.byref(opts))


def corpus_lorem(n):
    import numpy as np
    a = np.empty(n, dtype=np.uint8)
    lib().xzamd_corpus_lorem(a.ctypes.data, n)
    return a


def corpus_text(n, seed=1, threads=0):
    import numpy as np
    if threads <= 0:
        threads = min(64, os.cpu_count() or 1)
    a = np.empty(n, dtype=np.uint8)
    lib().xzamd_corpus_text(a.ctypes.data, n, seed, threads)
    return a


TAR_ROOTS = "/opt/rocm/include:/usr/include:/usr/lib/python3:/usr/lib/python3.10"


def corpus_tar(n, roots=TAR_ROOTS, seed=1):
    """ustar stream of the box's source trees, cycled to n bytes."""
    import numpy as np
    a = np.empty(n, dtype=np.uint8)
    if lib().xzamd_corpus_tar(a.ctypes.data, n, roots.encode(), seed) == 0:
        raise RuntimeError(f"no readable files under {roots}")
    return a


class XzAmdError(RuntimeError):
    """`code` = the XZAMD_* / lzma_ret value of the failed call, where there is one."""

    def __init__(self, msg, code=None, partial=None, report=None):
        super().__init__(msg)
        self.code = code
        self.partial = partial      # decode_forward: the bytes in front of the defect
        self.report = report        # ... and its report


def _stream_dict(s):
    return {n: getattr(s, n) for n in ("offset", "size", "padding", "first_block", "block_count", "uncompressed_offset",
                                       "uncompressed_size", "check")}


def _block_dict(b):
    d = {n: getattr(b, n) for n in ("header_offset", "unpadded_size", "total_size", "uncompressed_size",
                                    "uncompressed_offset", "stream")}
    d["filter_ids"] = tuple(b.filter_ids[: b.filter_count])
    return d


def _file_index(call, what, detail):
    """Both variants of xzamd_file_index_*: ask for the counts, then for the lists.  Returns (streams, blocks,
    uncompressed size), Streams and Blocks as dicts named like the fields of xzamd_xz_stream / xzamd_xz_block."""
    ns, nb, usz = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = call(None, 0, C.byref(ns), None, 0, C.byref(nb), C.byref(usz))
    if rc not in (0, 10):
        raise XzAmdError(f"{what} failed ({rc})" + detail(), rc)
    streams, blocks = (XzStream * max(ns.value, 1))(), (XzBlock * max(nb.value, 1))()
    rc = call(streams, ns.value, C.byref(ns), blocks, nb.value, C.byref(nb), C.byref(usz))
    if rc != 0:
        raise XzAmdError(f"{what} failed ({rc})" + detail(), rc)
    return ([_stream_dict(s) for s in streams[: ns.value]], [_block_dict(b) for b in blocks[: nb.value]], usz.value)


def crc32_combine(crc_a, crc_b, len_b):
    """CRC32 of A || B from crc32(A), crc32(B) and len(B) (xzamd_crc32_combine): how the single-Block encoder makes the
    Check of a Block from the Checks of its segments."""
    return lib().xzamd_crc32_combine(crc_a, crc_b, len_b)


def crc64_combine(crc_a, crc_b, len_b):
    """The same for the CRC64 of the .xz format (xzamd_crc64_combine)."""
    return lib().xzamd_crc64_combine(crc_a, crc_b, len_b)


def file_index(xz_bytes):
    """Streams and Blocks of an .xz file held in host memory (bytes): xz --list.  Validates all framing of the file
    (Stream Headers / Footers / Padding, Indexes, Block Headers and Padding); needs no GPU.  Returns (streams, blocks,
    uncompressed size)."""
    buf = bytes(xz_bytes)
    f = lib().xzamd_file_index_host
    return _file_index(lambda *a: f(buf, len(buf), *a), "xzamd_file_index_host", lambda: "")


class Encoder:
    """One GPU context. ``encode`` takes/returns CUDA uint8 tensors (torch owns the memory)."""

    def __init__(self, device=None):
        import torch
        if not torch.cuda.is_available():
            raise XzAmdError("no GPU visible: the xz_amd encoder has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._ctx = C.c_void_p()
        rc = lib().xzamd_ctx_create(C.byref(self._ctx), self.device.index)
        if rc != 0:
            raise XzAmdError(f"xzamd_ctx_create failed: {rc}")

    def close(self):
        if self._ctx:
            lib().xzamd_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_batch_bytes(self, n):
        if lib().xzamd_ctx_set_batch_bytes(self._ctx, n) != 0:
            raise ValueError("batch bytes out of range")

    def stats(self):
        s = Stats()
        lib().xzamd_get_stats(self._ctx, C.byref(s))
        return s

    def encode(self, data, opts=None, preset=6, block_size=0, check=CHECK_CRC64,
               span_size=None, blocks_only=False, out=None, verify=False, keep_resume=False, flags=0, repair=False,
               single=False, auto_delta=False, auto_bcj=False, auto_lclp=False):
        """Encode a CUDA uint8 tensor into an .xz Stream (CUDA uint8 tensor).

        Returns (out_tensor_view, block_infos). Runs on torch's current stream.

        keep_resume: the context keeps the resume table of this encode (one record per encode span) for `verify`.
        verify: verified encode -- the finished Stream is decoded on the device, span-parallel with that table, and
        compared with `data` before the call returns; a defect raises XzAmdError with code 9 (`.stream` = the Stream
        as written, `verify_report()` = the details).  `flags`: further XZAMD_F_* bits.
        repair: verified and repaired encode (XZAMD_F_REPAIR) -- every Block the device decoder rejects is re-encoded and
        spliced in before the call returns; `repair_report()` says what happened, the block infos are those of the
        repaired Stream.  Allowed with blocks_only.
        single: the single-Block Stream of lzma_stream_encoder (XZAMD_F_SINGLE), coded in segments of `block_size` bytes;
        the block infos describe the segments (offset and length of each chunk chain inside the Stream, its CRC in
        unpadded_size).  Combinable with verify, keep_resume and repair, which then act on the segments' chains;
        Checks none / CRC32 / CRC64, no filter in front of LZMA2.
        auto_delta: every Block gets the delta filter the device picks for it from byte histograms, or none
        (XZAMD_F_AUTO_DELTA); for the chain {LZMA2} only, not with single or repair.
        auto_bcj: every Block gets the BCJ filter (x86 or ARM64) the device picks for it from the entropy of its call
        operands, or none (XZAMD_F_AUTO_BCJ); the same restrictions.  With auto_delta too a Block takes the BCJ filter when
        that rule fires, else what the delta rule says.
        auto_lclp: every Block is parsed and coded with the literal context (lc, lp) the device picks for it from a joint
        histogram of its bytes -- never more literal coders than opts.lc + opts.lp, pb stays (XZAMD_F_AUTO_LCLP); with
        any filter chain and with auto_delta / auto_bcj (the statistic is taken behind the filters), not with single or repair.

        Every XzAmdError raised here carries `code` (the XZAMD_* value; it used to be None for encode failures) and
        `stream` (what was written: empty unless the failure is a verification defect).
        """
        import torch
        assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()
        if opts is None:
            opts = preset_options(preset)
        if span_size is not None:
            opts.span_size = span_size
        n = data.numel()
        bs = block_size if block_size else mt_block_size(opts)
        cap = lib().xzamd_stream_buffer_bound(n, bs)
        if out is None or out.numel() < cap:
            out = torch.empty(cap, dtype=torch.uint8, device=data.device)
        nblocks = (n + bs - 1) // bs
        binfo = (BlockInfo * max(nblocks, 1))()
        out_size = C.c_uint64(0)
        nb = C.c_uint64(0)
        cur = torch.cuda.current_stream(data.device)
        stream = cur.cuda_stream
        if stream == 0:
            # The C ABI reads a NULL stream as "the context's own (non-blocking) stream", which is not ordered
            # after work queued on torch's legacy default stream: make the input final first.  The library
            # synchronises its stream before it returns, so the output is ordered for the caller either way.
            cur.synchronize()
        rc = lib().xzamd_stream_encode_device(
            self._ctx, C.c_void_p(data.data_ptr()), n, bs, C.byref(opts), check,
            (F_BLOCKS_ONLY if blocks_only else 0) | (F_VERIFY if verify else 0) | (F_KEEP_RESUME if keep_resume else 0)
            | (F_REPAIR if repair else 0) | (F_SINGLE if single else 0) | (F_AUTO_DELTA if auto_delta else 0)
            | (F_AUTO_BCJ if auto_bcj else 0) | (F_AUTO_LCLP if auto_lclp else 0) | flags,
            C.c_void_p(out.data_ptr()), out.numel(),
            C.byref(out_size), binfo, max(nblocks, 1), C.byref(nb), C.c_void_p(stream))
        if rc != 0:
            err = XzAmdError(f"xzamd_stream_encode_device failed ({rc}): "
                             f"{lib().xzamd_last_error(self._ctx).decode()}", rc)
            err.stream = out[: out_size.value]
            raise err
        return out[: out_size.value], list(binfo)[: nb.value]

    def choose_lclp(self, data, block_size, lc=3, lp=0):
        """What encode(auto_lclp=True) of a job with (lc, lp) and no filter would pick for every Block of `block_size` bytes
        of `data` (CUDA uint8 tensor): the list of (lc, lp) pairs (xzamd_auto_lclp_device)."""
        import torch
        assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()
        n = data.numel()
        cap = max((n + block_size - 1) // block_size, 1) if block_size else 1
        props = (C.c_uint32 * cap)()
        nb = C.c_uint64(0)
        torch.cuda.current_stream(data.device).synchronize()
        rc = lib().xzamd_auto_lclp_device(self._ctx, C.c_void_p(data.data_ptr()), n, block_size, lc, lp, props, cap,
                                          C.byref(nb), None)
        if rc != 0:
            raise XzAmdError(f"xzamd_auto_lclp_device failed ({rc}): {lib().xzamd_last_error(self._ctx).decode()}", rc)
        return [(v & 255, v >> 8) for v in list(props)[: nb.value]]

    def lclp_stats(self, nblocks):
        """The joint histograms and choices the last choose_lclp / encode(auto_lclp=True) of this context left for the
        `nblocks` Blocks of its last batch: (uint32 array [nblocks, 8, 8, 256] indexed [offset & 7][byte in front >> 5][byte],
        list of (lc, lp))."""
        import numpy as np
        hist = np.zeros((nblocks, 8, 8, 256), dtype=np.uint32)
        props = np.zeros(nblocks, dtype=np.uint32)
        for what, a in ((DEBUG_LCLP_HIST, hist), (DEBUG_LCLP_PROPS, props)):
            rc = lib().xzamd_debug_fetch(self._ctx, what, C.c_void_p(a.ctypes.data), a.nbytes)
            if rc != 0:
                raise XzAmdError(f"xzamd_debug_fetch({what}) failed ({rc})", rc)
        return hist, [(int(v) & 255, int(v) >> 8) for v in props]

    def choose_delta(self, data, block_size):
        """What encode(auto_delta=True) would pick for every Block of `block_size` bytes of `data` (CUDA uint8 tensor): the
        list of delta distances, 0 = no filter (xzamd_auto_delta_device)."""
        import torch
        assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()
        n = data.numel()
        cap = max((n + block_size - 1) // block_size, 1) if block_size else 1
        dist = (C.c_uint32 * cap)()
        nb = C.c_uint64(0)
        torch.cuda.current_stream(data.device).synchronize()
        rc = lib().xzamd_auto_delta_device(self._ctx, C.c_void_p(data.data_ptr()), n, block_size, dist, cap, C.byref(nb), None)
        if rc != 0:
            raise XzAmdError(f"xzamd_auto_delta_device failed ({rc}): {lib().xzamd_last_error(self._ctx).decode()}", rc)
        return list(dist)[: nb.value]

    def delta_histograms(self, nblocks):
        """The histograms and choices the last choose_delta / encode(auto_delta=True) of this context left for the
        `nblocks` Blocks of its last batch: (uint32 array [nblocks, 11, 256] in the order of AUTO_DELTA_DISTANCES,
        uint32 array [nblocks])."""
        import numpy as np
        hist = np.zeros((nblocks, len(AUTO_DELTA_DISTANCES), 256), dtype=np.uint32)
        dist = np.zeros(nblocks, dtype=np.uint32)
        for what, a in ((DEBUG_DELTA_HIST, hist), (DEBUG_DELTA_DIST, dist)):
            rc = lib().xzamd_debug_fetch(self._ctx, what, C.c_void_p(a.ctypes.data), a.nbytes)
            if rc != 0:
                raise XzAmdError(f"xzamd_debug_fetch({what}) failed ({rc})", rc)
        return hist, dist

    def choose_bcj(self, data, block_size):
        """What encode(auto_bcj=True) would pick for every Block of `block_size` bytes of `data` (CUDA uint8 tensor): the
        list of filter ids (BCJ_X86, BCJ_ARM64), 0 = no filter (xzamd_auto_bcj_device)."""
        import torch
        assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()
        n = data.numel()
        cap = max((n + block_size - 1) // block_size, 1) if block_size else 1
        kind = (C.c_uint32 * cap)()
        nb = C.c_uint64(0)
        torch.cuda.current_stream(data.device).synchronize()
        rc = lib().xzamd_auto_bcj_device(self._ctx, C.c_void_p(data.data_ptr()), n, block_size, kind, cap, C.byref(nb), None)
        if rc != 0:
            raise XzAmdError(f"xzamd_auto_bcj_device failed ({rc}): {lib().xzamd_last_error(self._ctx).decode()}", rc)
        return list(kind)[: nb.value]

    def bcj_histograms(self, nblocks):
        """What the last choose_bcj / encode(auto_bcj=True) of this context left for the `nblocks` Blocks of its last batch:
        (uint32 array [nblocks, 2, 2, 4096]: per candidate of AUTO_BCJ_KINDS the histogram of the operands as stored and
        made absolute, uint32 array [nblocks, 2] of site counts, uint32 array [nblocks] of chosen filter ids)."""
        import numpy as np
        words = len(AUTO_BCJ_KINDS) * 2 * AUTO_BCJ_BUCKETS
        both = np.zeros(nblocks * (words + len(AUTO_BCJ_KINDS)), dtype=np.uint32)
        kind = np.zeros(nblocks, dtype=np.uint32)
        for what, a in ((DEBUG_BCJ_HIST, both), (DEBUG_BCJ_KIND, kind)):
            rc = lib().xzamd_debug_fetch(self._ctx, what, C.c_void_p(a.ctypes.data), a.nbytes)
            if rc != 0:
                raise XzAmdError(f"xzamd_debug_fetch({what}) failed ({rc})", rc)
        hist = both[: nblocks * words].reshape(nblocks, len(AUTO_BCJ_KINDS), 2, AUTO_BCJ_BUCKETS)
        return hist, both[nblocks * words:].reshape(nblocks, len(AUTO_BCJ_KINDS)), kind

    def verify_report(self):
        """The report of this context's last verification (`verify`, or an encode with verify=True) as a dict named like
        the fields of xzamd_verify_report; first_bad_step as one of VSTEPS, first_bad_block None when there is none."""
        r = VerifyReport()
        lib().xzamd_get_verify_report(self._ctx, C.byref(r))
        d = {n: getattr(r, n) for n in ("units", "blocks", "records_used", "mismatching_words", "ms_verify")}
        d["table_used"] = bool(r.table_used)
        d["first_bad_block"] = None if r.first_bad_block == NO_BLOCK else r.first_bad_block
        d["first_bad_step"] = VSTEPS[r.first_bad_step] if r.first_bad_step < len(VSTEPS) else str(r.first_bad_step)
        return d

    def verify(self, xz, original):
        """Verify an .xz Stream against its original (CUDA uint8 tensors): device decode with the units of the resume
        table kept by the last encode(keep_resume=True) of this context when it fits, Checks, comparison.  Returns the
        report (`verify_report`); a defect raises XzAmdError with code 9."""
        import torch
        for t in (xz, original):
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.device == xz.device
        torch.cuda.current_stream(xz.device).synchronize()
        rc = lib().xzamd_stream_verify_device(self._ctx, C.c_void_p(xz.data_ptr()), xz.numel(),
                                              C.c_void_p(original.data_ptr()), original.numel(), None, None)
        if rc != 0:
            raise XzAmdError(f"xzamd_stream_verify_device failed ({rc})" + self._detail(), rc)
        return self.verify_report()

    def verify_blocks(self, xz, original=None):
        """Per-Block verification of an .xz Stream (CUDA uint8 tensor), against `original` when given (else grammar,
        decode and Check only): one step name of VSTEPS per Block, "none" = good.  Bad Blocks do not raise; a damaged
        Stream Header, Footer or Index does.  `verify_report()` has the details."""
        import torch
        for t in (xz,) + ((original,) if original is not None else ()):
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.device == xz.device
        torch.cuda.current_stream(xz.device).synchronize()
        f = lib().xzamd_stream_verify_blocks_device
        nb = C.c_uint64(0)
        args = (self._ctx, C.c_void_p(xz.data_ptr()), xz.numel(),
                C.c_void_p(original.data_ptr()) if original is not None else None,
                original.numel() if original is not None else 0)
        rc = f(*args, None, 0, C.byref(nb), None, None)
        if rc not in (0, 10):
            raise XzAmdError(f"xzamd_stream_verify_blocks_device failed ({rc})" + self._detail(), rc)
        steps = (C.c_uint8 * max(nb.value, 1))()
        rc = f(*args, steps, nb.value, C.byref(nb), None, None)
        if rc not in (0, 9):
            raise XzAmdError(f"xzamd_stream_verify_blocks_device failed ({rc})" + self._detail(), rc)
        if rc == 9 and not any(steps[: nb.value]):
            raise XzAmdError("xzamd_stream_verify_blocks_device failed (9)" + self._detail(), rc)
        return [VSTEPS[v] if v < len(VSTEPS) else str(v) for v in steps[: nb.value]]

    def _chain_args(self, chains, block_infos, original, opts, preset):
        import torch
        for t in (chains,) + ((original,) if original is not None else ()):
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.device == chains.device
        if opts is None:
            opts = preset_options(preset)
        n = len(block_infos)
        binfo = (BlockInfo * max(n, 1))()
        for i, b in enumerate(block_infos):
            binfo[i].unpadded_size, binfo[i].uncompressed_size = b.unpadded_size, b.uncompressed_size
            binfo[i].out_offset, binfo[i].total_size = b.out_offset, b.total_size
        torch.cuda.current_stream(chains.device).synchronize()
        return opts, n, binfo

    def verify_chains(self, chains, block_infos, original=None, opts=None, preset=6, check=CHECK_CRC64):
        """Per-segment verification of bare chunk chains: `chains` (CUDA uint8 tensor) and `block_infos` as
        encode(flags=F_SEGMENTS) returns them -- out_offset / total_size name a chain inside `chains`, unpadded_size is the
        segment's CRC.  Against `original` when given.  One step name of VSTEPS per segment, "none" = good; bad segments do
        not raise.  `verify_report()` has the details."""
        opts, n, binfo = self._chain_args(chains, block_infos, original, opts, preset)
        steps = (C.c_uint8 * max(n, 1))()
        rc = lib().xzamd_chains_verify_device(self._ctx, C.c_void_p(chains.data_ptr()), chains.numel(), binfo, n,
                                              C.byref(opts), check,
                                              C.c_void_p(original.data_ptr()) if original is not None else None,
                                              original.numel() if original is not None else 0, steps, n, None, None)
        if rc not in (0, 9) or (rc == 9 and not any(steps[:n])):
            raise XzAmdError(f"xzamd_chains_verify_device failed ({rc})" + self._detail(), rc)
        return [VSTEPS[v] if v < len(VSTEPS) else str(v) for v in steps[:n]]

    def repair_chains(self, buf, size, block_infos, original, opts=None, preset=6, check=CHECK_CRC64):
        """Repair, in place, the chunk chains in the first `size` bytes of the CUDA uint8 tensor `buf` (its capacity: the
        whole tensor): the segments the device decoder rejects are re-encoded from `original` and spliced in, the chains
        behind them move.  All or nothing: an XzAmdError (code 10 when `buf` is too small, with `.new_size`) leaves chains
        and block infos as they were (`.block_infos`: what the library left in its table).  Returns (view of the repaired chains, the rewritten block infos, report dict)."""
        assert 0 <= size <= buf.numel()
        opts, n, binfo = self._chain_args(buf, block_infos, original, opts, preset)
        ns = C.c_uint64(0)
        rc = lib().xzamd_chains_repair_device(self._ctx, C.c_void_p(buf.data_ptr()), size, buf.numel(), binfo, n,
                                              C.byref(opts), check, C.c_void_p(original.data_ptr()), original.numel(),
                                              C.byref(ns), None, None)
        if rc != 0:
            err = XzAmdError(f"xzamd_chains_repair_device failed ({rc})" + self._detail(), rc)
            err.new_size = ns.value
            err.block_infos = list(binfo)[:n]
            raise err
        return buf[: ns.value], list(binfo)[:n], self.repair_report()

    def repair_report(self):
        """The report of this context's last repair (`repair`, or an encode with repair=True) as a dict named like the
        fields of xzamd_repair_report."""
        r = RepairReport()
        lib().xzamd_get_repair_report(self._ctx, C.byref(r))
        return {n: getattr(r, n) for n, _ in RepairReport._fields_ if n != "reserved_"}

    def repair(self, buf, size, original, opts=None, preset=6):
        """Repair, in place, the .xz Stream in the first `size` bytes of the CUDA uint8 tensor `buf` (its capacity: the
        whole tensor) against `original`: the Blocks the device decoder rejects are re-encoded with `opts` and spliced
        in.  All or nothing: an XzAmdError (code 10 when `buf` is too small, with `.new_size` = what is needed) leaves
        the Stream as it was.  Returns (view of the repaired Stream, report dict)."""
        import torch
        for t in (buf, original):
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.device == buf.device
        assert 0 <= size <= buf.numel()
        if opts is None:
            opts = preset_options(preset)
        torch.cuda.current_stream(buf.device).synchronize()
        ns = C.c_uint64(0)
        rc = lib().xzamd_stream_repair_device(self._ctx, C.c_void_p(buf.data_ptr()), size, buf.numel(),
                                              C.c_void_p(original.data_ptr()), original.numel(), C.byref(opts),
                                              C.byref(ns), None, None)
        if rc != 0:
            err = XzAmdError(f"xzamd_stream_repair_device failed ({rc})" + self._detail(), rc)
            err.new_size = ns.value
            raise err
        return buf[: ns.value], self.repair_report()

    def debug_resume_records(self):
        """Test instrumentation: records of the kept resume table (0: none kept)."""
        n = C.c_uint32(0)
        lib().xzamd_debug_resume_peek_(self._ctx, 0, None, C.byref(n))
        return n.value

    def debug_resume_peek(self, record):
        """Test instrumentation: header of a record of the kept table as a dict (block, upos, lc, lp, pb, kind, state, rep)."""
        h = (C.c_uint32 * 8)()
        rc = lib().xzamd_debug_resume_peek_(self._ctx, record, h, None)
        if rc != 0:
            raise XzAmdError(f"resume_peek({record}) failed: {rc}", rc)
        return {"block": h[0], "upos": h[1], "lc": h[2] & 0xFF, "lp": (h[2] >> 8) & 0xFF, "pb": (h[2] >> 16) & 0xFF,
                "kind": h[2] >> 24, "state": h[3], "rep": tuple(h[4:8])}

    def debug_resume_poke(self, record, field, value=0):
        """Test instrumentation: overwrite a field of a record of the kept table: "upos", "kind", "state", or "model"
        (all 1024s)."""
        rc = lib().xzamd_debug_resume_poke_(self._ctx, record, ("upos", "kind", "state", "model").index(field), value)
        if rc != 0:
            raise XzAmdError(f"resume_poke({record}, {field}) failed: {rc}", rc)

    def decode(self, xz, out_cap, expected=None):
        """Decode an .xz Stream held in a CUDA uint8 tensor on the device: the chains {LZMA2} and {up to three of BCJ |
        delta, LZMA2} (a BCJ filter with a non-zero start offset is declined).  With `expected` (CUDA uint8 tensor of
        the original data) it is a span-parallel verification decode.  Returns (decoded tensor view, nblocks)."""
        import torch
        assert xz.is_cuda and xz.dtype == torch.uint8 and xz.is_contiguous()
        if expected is not None:
            assert (expected.is_cuda and expected.dtype == torch.uint8 and expected.is_contiguous()
                    and expected.device == xz.device), "expected: contiguous CUDA uint8 tensor on the Stream's device"
        out = torch.empty(max(out_cap, 1), dtype=torch.uint8, device=xz.device)
        osz, mm, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        torch.cuda.current_stream(xz.device).synchronize()
        rc = lib().xzamd_stream_decode_device(
            self._ctx, C.c_void_p(xz.data_ptr()), xz.numel(), C.c_void_p(out.data_ptr()), out_cap, C.byref(osz),
            C.c_void_p(expected.data_ptr()) if expected is not None else None,
            expected.numel() if expected is not None else 0, C.byref(mm), C.byref(nb), None)
        if rc != 0:
            raise XzAmdError(f"xzamd_stream_decode_device failed ({rc}): {lib().xzamd_last_error(self._ctx).decode()}"
                             + (f" [{mm.value} mismatching words]" if mm.value else ""), rc)
        return out[: osz.value], nb.value

    def _detail(self):
        return ": " + lib().xzamd_last_error(self._ctx).decode()

    def file_index(self, xz):
        """Streams and Blocks of an .xz file held in a CUDA uint8 tensor: `file_index` with the Block Headers parsed on
        the device (one thread per Block)."""
        import torch
        assert xz.is_cuda and xz.dtype == torch.uint8 and xz.is_contiguous()
        torch.cuda.current_stream(xz.device).synchronize()
        f = lib().xzamd_file_index_device
        return _file_index(lambda *a: f(self._ctx, C.c_void_p(xz.data_ptr()), xz.numel(), *a), "xzamd_file_index_device",
                           self._detail)

    def decode_file(self, xz, out_cap, expected=None):
        """`decode` for a whole .xz file: any number of Streams, each followed by Stream Padding.  Returns (decoded
        tensor view, Blocks of all Streams)."""
        import torch
        assert xz.is_cuda and xz.dtype == torch.uint8 and xz.is_contiguous()
        if expected is not None:
            assert (expected.is_cuda and expected.dtype == torch.uint8 and expected.is_contiguous()
                    and expected.device == xz.device), "expected: contiguous CUDA uint8 tensor on the file's device"
        out = torch.empty(max(out_cap, 1), dtype=torch.uint8, device=xz.device)
        osz, mm, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        torch.cuda.current_stream(xz.device).synchronize()
        rc = lib().xzamd_file_decode_device(
            self._ctx, C.c_void_p(xz.data_ptr()), xz.numel(), C.c_void_p(out.data_ptr()), out_cap, C.byref(osz),
            C.c_void_p(expected.data_ptr()) if expected is not None else None,
            expected.numel() if expected is not None else 0, C.byref(mm), C.byref(nb), None)
        if rc != 0:
            raise XzAmdError(f"xzamd_file_decode_device failed ({rc})" + self._detail()
                             + (f" [{mm.value} mismatching words]" if mm.value else ""), rc)
        return out[: osz.value], nb.value

    def decode_range(self, xz, offset, length):
        """Uncompressed bytes [offset, offset + length) of an .xz file, clipped at its end like pread; only the Blocks
        that hold them are decoded (and their Checks verified).  Returns (tensor of the bytes, Blocks decoded)."""
        import torch
        assert xz.is_cuda and xz.dtype == torch.uint8 and xz.is_contiguous()
        out = torch.empty(max(length, 1), dtype=torch.uint8, device=xz.device)
        osz, nb = C.c_uint64(0), C.c_uint64(0)
        torch.cuda.current_stream(xz.device).synchronize()
        rc = lib().xzamd_file_decode_range_device(
            self._ctx, C.c_void_p(xz.data_ptr()), xz.numel(), offset, length, C.c_void_p(out.data_ptr()), length,
            C.byref(osz), C.byref(nb), None)
        if rc != 0:
            raise XzAmdError(f"xzamd_file_decode_range_device failed ({rc})" + self._detail(), rc)
        return out[: osz.value], nb.value

    def decode_forward(self, xz, out_cap, concatenated=True):
        """Decode an .xz file held in a CUDA uint8 tensor from its front, without its Index (xzamd_file_decode_forward_device):
        a truncated file, or one damaged in or behind a Block, gives every whole good Block in front of the damage.
        Returns (decoded tensor view, report dict: the fields of xzamd_forward_report).  A truncated input and an output
        that does not fit are no exceptions: report["code"] is then XZAMD_BUF_ERROR (10) and report["stop"] tells which.
        Any other code raises XzAmdError, whose .partial / .report carry the bytes in front of the defect and the report."""
        import torch
        assert xz.is_cuda and xz.dtype == torch.uint8 and xz.is_contiguous()
        out = torch.empty(max(out_cap, 1), dtype=torch.uint8, device=xz.device)
        osz, rp = C.c_uint64(0), ForwardReport()
        torch.cuda.current_stream(xz.device).synchronize()
        rc = lib().xzamd_file_decode_forward_device(
            self._ctx, C.c_void_p(xz.data_ptr()) if xz.numel() else None, xz.numel(), FWD_CONCATENATED if concatenated else 0,
            C.c_void_p(out.data_ptr()), out_cap, C.byref(osz), C.byref(rp), None)
        report = {n: getattr(rp, n) for n in ("streams", "blocks", "blocks_delivered", "consumed", "stop_offset", "stop", "step")}
        report["code"] = rc
        if rc not in (0, 10):
            raise XzAmdError(f"xzamd_file_decode_forward_device failed ({rc})" + self._detail(), rc, out[: osz.value], report)
        return out[: osz.value], report

    @staticmethod
    def debug_forward_counters():
        """Counts of the last decode_forward (test instrumentation): (device-to-host reads, kernel-launch calls, Blocks
        delivered, walk launches)."""
        a = (C.c_uint64 * 4)()
        lib().xzamd_debug_forward_counters_(a)
        return tuple(a)

    # debug hooks used by the parity tests
    @staticmethod
    def debug_file_counters():
        """Counts of the last file call on a file in device memory (test instrumentation): (device-to-host reads,
        kernel-launch calls, Blocks decoded)."""
        a = (C.c_uint64 * 3)()
        lib().xzamd_debug_file_counters_(a)
        return tuple(a)

    @staticmethod
    def debug_decode_counters():
        """Process-wide counts of the device decoder (test instrumentation): (temporary buffers allocated for inverse
        filters, inverse-stage calls, forward-filter launches of verification decodes)."""
        a = (C.c_uint64 * 3)()
        f = lib().xzamd_debug_decode_counters_        # bound here: an older library (XZ_AMD_LIB, A/B runs) lacks it
        f.restype, f.argtypes = None, [C.POINTER(C.c_uint64)]
        f(a)
        return tuple(a)

    @staticmethod
    def debug_decode_units():
        """The last decode launch of the process (test instrumentation): (units, Blocks, split mode of the unit scan: 0 = a
        unit per Block, 1 = verification units at state resets, 2 = plain units at dictionary resets)."""
        a = (C.c_uint64 * 3)()
        f = lib().xzamd_debug_decode_units_
        f.restype, f.argtypes = None, [C.POINTER(C.c_uint64)]
        f(a)
        return tuple(a)

    def debug_fetch(self, what, count, dtype="uint32"):
        """Copy a work buffer of the last batch to the host: 1 = suffix order, 2 = position -> slot,
        3 = match-list records (8 x u32 per position), 4 = their u16 lengths."""
        import numpy as np
        buf = np.zeros(count, dtype=dtype)
        rc = lib().xzamd_debug_fetch(self._ctx, what, C.c_void_p(buf.ctypes.data), C.c_uint64(buf.nbytes))
        if rc != 0:
            raise XzAmdError(f"debug_fetch({what}) failed: {rc}")
        return buf

    def trace_enable(self, cap):
        if lib().xzamd_trace_enable(self._ctx, cap) != 0:
            raise XzAmdError("trace_enable failed")

    def trace_read(self, cap):
        import numpy as np
        buf = np.zeros((cap, 4), dtype=np.uint32)
        cnt = C.c_uint32(0)
        if lib().xzamd_trace_read(self._ctx, buf.ctypes.data, cap, C.byref(cnt)) != 0:
            raise XzAmdError("trace_read failed")
        return buf[: min(cnt.value, cap)], cnt.value
