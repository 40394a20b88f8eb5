"""ctypes binding over the C ABI of libzpaq_hip.so (include/zpaq_hip.h).

This is plumbing only: every compute call goes to the HIP library.  There is no
Python or CPU fallback -- if the shared library is missing, or no GPU is
present, the calls raise ZpqError.
"""
import atexit
import ctypes as C
import os
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FLAG_PP = 1
FLAG_GENERIC = 2
FLAG_LANES = 8
FLAG_VMPIPE = 16
FLAG_LINESTORE = 32                          # a request: k_rows / k_lanes with the large ICM / ISSE tables on the compact line store
SET_LANES = 1                                # zpq_blockset_create_ex / zpq_blockset_capacity_ex
SET_PIPE = 4
SET_WAVES = 16
SET_VMWAVES = 64
SET_CHUNKS = 128
_LIB = None
# Handle lifetime on the Python side (the C side tolerates any destroy order as well, include/zpaq_hip.h): every live
# Context, Block and PinnedArray is tracked; Context.close() closes its blocks first; at interpreter exit everything
# still alive is closed in that order by ONE atexit hook (registered when the library is loaded, i.e. after torch's own
# hooks, so it runs before them and before any runtime is torn down) and from then on __del__ does nothing: a
# destructor that runs during interpreter finalisation must not call into HIP any more.
_LIVE_CTX = weakref.WeakSet()
_LIVE_PINNED = weakref.WeakSet()
_FINALIZING = False


def _shutdown():
    global _FINALIZING
    for ctx in list(_LIVE_CTX):
        try:
            ctx.close()
        except Exception:  # noqa: BLE001
            pass
    for arr in list(_LIVE_PINNED):
        try:
            arr.free()
        except Exception:  # noqa: BLE001
            pass
    _FINALIZING = True


class ZpqError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        super().__init__("%s: %s (%d)" % (what, status_string(code), code))


def lib_path():
    # ZPQ_LIB_PATH: another build of the same library (kernel experiments, tools/variant.sh)
    return os.environ.get("ZPQ_LIB_PATH") or os.path.join(HERE, "lib", "libzpaq_hip.so")


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise ZpqError(-1, "libzpaq_hip.so is not built (run __graft_entry__.build() or make -C zpaq-v_amd/csrc)")
    # PyTorch-ROCm ships its own HIP runtime; a process that maps this library (and with it the system's libamdhip64) BEFORE
    # torch ends up with two runtimes and the second one to initialise sees no device (measured: build() then smoke() in one
    # process).  Where torch is there -- it is on every box this harness runs on -- its runtime is mapped first, always.
    try:
        import torch  # noqa: F401
    except Exception:  # noqa: BLE001
        pass
    L = C.CDLL(p)
    vp, u8p, u32, i32, u64 = C.c_void_p, C.c_char_p, C.c_uint32, C.c_int, C.c_uint64
    L.zpq_level_header.argtypes = [i32, vp, i32, vp, vp, vp, vp]
    L.zpq_scan_header.argtypes = [u8p, i32, vp, vp, vp]
    L.zpq_model_create.argtypes = [u8p, i32, i32, i32, i32, vp]
    L.zpq_model_create_level.argtypes = [i32, vp]
    L.zpq_model_destroy.argtypes = [vp]
    L.zpq_model_ncomp.argtypes = [vp]
    L.zpq_model_state_bytes.argtypes = [vp]
    L.zpq_model_state_bytes.restype = u64
    L.zpq_model_has_fast_path.argtypes = [vp]
    L.zpq_ctx_create.argtypes = [i32, vp]
    L.zpq_ctx_destroy.argtypes = [vp]
    L.zpq_ctx_sync.argtypes = [vp]
    L.zpq_ctx_stream.argtypes = [vp]
    L.zpq_ctx_stream.restype = vp
    L.zpq_ctx_set_state_budget.argtypes = [vp, u64]
    L.zpq_ctx_set_max_block_bytes.argtypes = [vp, u64]
    L.zpq_ctx_last_slots.argtypes = [vp]
    L.zpq_ctx_last_host_transfer.argtypes = [vp]
    L.zpq_ctx_last_host_transfer.restype = C.c_uint
    L.zpq_ctx_last_line_store.argtypes = [vp]
    L.zpq_ctx_last_line_store.restype = C.c_uint
    L.zpq_ctx_resident_capacity.argtypes = [vp, vp, u32]
    L.zpq_ctx_last_kernel_ms.argtypes = [vp]
    L.zpq_ctx_last_kernel_ms.restype = C.c_float
    L.zpq_ctx_last_kernel_name.argtypes = [vp]
    L.zpq_ctx_last_kernel_name.restype = C.c_char_p
    enc = [vp, vp, i32, vp, vp, u32, vp, vp, vp, vp]
    dec = [vp, vp, i32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    L.zpq_encode_blocks.argtypes = enc
    L.zpq_encode_blocks_dev.argtypes = enc
    L.zpq_decode_blocks.argtypes = dec
    L.zpq_decode_blocks_dev.argtypes = dec
    L.zpq_host_alloc.argtypes = [C.c_size_t]
    L.zpq_host_alloc.restype = vp
    L.zpq_host_free.argtypes = [vp]
    L.zpq_encode_blocks_multi.argtypes = [vp, i32, vp, i32, vp, vp, u32, vp, vp, vp, vp]
    L.zpq_decode_blocks_multi.argtypes = [vp, i32, vp, i32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    L.zpq_sha1_blocks.argtypes = [vp, i32, vp, vp, vp]
    L.zpq_sha1_blocks_dev.argtypes = [vp, i32, vp, vp, vp]
    L.zpq_sha1_ranges_dev.argtypes = [vp, i32, vp, vp, vp, vp]
    L.zpq_ctx_device.argtypes = [vp]
    L.zpq_gather_dev.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.zpq_block_create.argtypes = [vp, vp, vp]
    L.zpq_block_destroy.argtypes = [vp]
    L.zpq_block_encode_segment.argtypes = [vp, u8p, C.c_size_t, u32, vp, C.c_size_t, vp]
    L.zpq_block_decode_segment.argtypes = [vp, u8p, C.c_size_t, u32, vp, C.c_size_t, vp, vp, vp, vp]
    L.zpq_blockset_create.argtypes = [vp, vp, i32, u64, vp]
    L.zpq_blockset_destroy.argtypes = [vp]
    L.zpq_blockset_capacity.argtypes = [vp, vp, u64]
    L.zpq_blockset_create_ex.argtypes = [vp, vp, i32, u64, u32, vp]
    L.zpq_blockset_capacity_ex.argtypes = [vp, vp, u64, u32]
    L.zpq_blockset_flags.argtypes = [vp]
    L.zpq_blockset_flags.restype = u32
    L.zpq_lanes_store_applies.argtypes = [vp, u32]
    L.zpq_lanes_store_slot_bytes.argtypes = [vp, u32]
    L.zpq_lanes_store_slot_bytes.restype = u64
    L.zpq_blockset_lanes_applies.argtypes = [vp]
    L.zpq_blockset_pipe_applies.argtypes = [vp]
    L.zpq_blockset_waves_applies.argtypes = [vp]
    L.zpq_blockset_vmwaves_applies.argtypes = [vp]
    L.zpq_blockset_resolve_flags.argtypes = [vp, u32]
    L.zpq_blockset_encode_segments.argtypes = [vp, i32, vp, vp, vp, u32, vp, vp, vp, vp]
    L.zpq_blockset_decode_segments.argtypes = [vp, i32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "zpq_blockset_encode_chunks"):           # (a ZPQ_LIB_PATH build from before chunked coding lacks the three)
        L.zpq_blockset_encode_chunks.argtypes = [vp, i32, vp, vp, vp, u32, vp, vp, vp, vp, vp]
        L.zpq_blockset_decode_chunks.argtypes = [vp, i32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.zpq_blockset_member_open.argtypes = [vp, i32]
    L.zpq_tables.argtypes = [vp, vp]
    L.zpq_tables_ex.argtypes = [vp, vp, vp]
    L.zpq_debug_contexts.argtypes = [vp, vp, u8p, C.c_size_t, vp]
    L.zpq_debug_encode_trace.argtypes = [vp, vp, u8p, C.c_size_t, u32, vp, C.c_size_t, vp, vp, C.c_size_t]
    if hasattr(L, "zpq_debug_pool_residue"):               # (a ZPQ_LIB_PATH build from before the dirty-line log lacks it)
        L.zpq_debug_pool_residue.argtypes = [vp, i32, vp]
    if hasattr(L, "zpq_debug_dlog_counts"):
        L.zpq_debug_dlog_counts.argtypes = [vp, i32, vp]
    L.zpq_status_string.argtypes = [i32]
    L.zpq_status_string.restype = C.c_char_p
    L.zpq_version.restype = C.c_char_p
    _LIB = L
    atexit.register(_shutdown)
    return L


def status_string(code):
    try:
        return lib().zpq_status_string(code).decode()
    except Exception:
        return "?"


def _ck(rc, what):
    if rc != 0:
        raise ZpqError(rc, what)


def tables_ex():
    """dt[1024], dt2k[256], ns[1024] as the library builds them (zpq_tables_ex)."""
    dt = np.zeros(1024, dtype=np.int32)
    dt2k = np.zeros(256, dtype=np.int32)
    ns = np.zeros(1024, dtype=np.uint8)
    _ck(lib().zpq_tables_ex(dt.ctypes.data, dt2k.ctypes.data, ns.ctypes.data), "zpq_tables_ex")
    return dt, dt2k, ns


def level_header(level):
    """get_compression_level(level).hcomp (reference zpaq/levels.v:26-36)."""
    buf = C.create_string_buffer(256)
    n = C.c_int()
    _ck(lib().zpq_level_header(level, buf, 256, C.byref(n), None, None, None), "zpq_level_header")
    return buf.raw[:n.value]


def scan_header(hdr):
    """cend, hbegin, hend as Compressor.start_block derives them (compressor.v:96-145)."""
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    _ck(lib().zpq_scan_header(hdr, len(hdr), C.byref(a), C.byref(b), C.byref(c)), "zpq_scan_header")
    return a.value, b.value, c.value


class Model:
    def __init__(self, header=None, level=None, offsets=None):
        self.h = C.c_void_p()
        if header is None:
            header = level_header(level)
        self.header = bytes(header)
        self.offsets = tuple(offsets) if offsets else scan_header(self.header)
        _ck(lib().zpq_model_create(self.header, len(self.header), *self.offsets, C.byref(self.h)),
            "zpq_model_create")

    def close(self):
        if getattr(self, "h", None) and _LIB is not None:
            _LIB.zpq_model_destroy(self.h)                 # (a Block built on the model keeps it alive: it is refcounted)
            self.h = None

    def __del__(self):
        if not _FINALIZING:
            self.close()

    @property
    def ncomp(self):
        return lib().zpq_model_ncomp(self.h)

    @property
    def state_bytes(self):
        return lib().zpq_model_state_bytes(self.h)

    @property
    def has_fast_path(self):
        return bool(lib().zpq_model_has_fast_path(self.h))

    def lanes_store_applies(self, cap_lines):
        """Would FLAG_LINESTORE be honoured for this model on a line store of cap_lines lines (host logic, no device)?"""
        return bool(lib().zpq_lanes_store_applies(self.h, cap_lines))

    def lanes_store_slot_bytes(self, cap_lines):
        """Bytes of one block's slot under FLAG_LINESTORE at that capacity, 0 where the store does not apply."""
        return lib().zpq_lanes_store_slot_bytes(self.h, cap_lines)


class PinnedArray:
    """A numpy view over page-locked, device-visible host memory (zpq_host_alloc): what a front end should hand
    to the host-pointer batch calls so that transfers are plain DMA and outputs are packed by the GPU."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = lib().zpq_host_alloc(max(self.nbytes, 1))
        if not self.ptr:
            raise ZpqError(-6, "zpq_host_alloc")
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(self.nbytes, 1)).from_address(self.ptr))[:self.nbytes]
        _LIVE_PINNED.add(self)

    def free(self):
        if getattr(self, "ptr", None) and _LIB is not None:
            self.array = None
            _LIB.zpq_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        if not _FINALIZING:
            self.free()


def _offsets(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    if len(lengths):
        off[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64))
    return off


# fn(*head, in, in_off, flags, out, out_off, results...): the batch, _multi and block-set calls differ in `head` alone
def _enc_raw(fn, head, nblocks, in_ptr, in_off, flags, out_ptr, out_off):
    in_off, out_off = np.ascontiguousarray(in_off, dtype=np.uint64), np.ascontiguousarray(out_off, dtype=np.uint64)
    assert len(in_off) == nblocks + 1 and len(out_off) == nblocks + 1
    out_len = np.full(nblocks, 0xABCDEF, dtype=np.uint32)
    status = np.full(nblocks, -99, dtype=np.int32)
    rc = fn(*head, in_ptr, in_off.ctypes.data, flags, out_ptr, out_off.ctypes.data, out_len.ctypes.data,
            status.ctypes.data)
    return rc, out_len, status


def _dec_raw(fn, head, nblocks, in_ptr, in_off, flags, out_ptr, out_off):
    in_off, out_off = np.ascontiguousarray(in_off, dtype=np.uint64), np.ascontiguousarray(out_off, dtype=np.uint64)
    assert len(in_off) == nblocks + 1 and len(out_off) == nblocks + 1
    r = [np.full(nblocks, 0xABCDEF, dtype=np.uint32) for _ in range(4)]
    status = np.full(nblocks, -99, dtype=np.int32)
    rc = fn(*head, in_ptr, in_off.ctypes.data, flags, out_ptr, out_off.ctypes.data, r[0].ctypes.data,
            r[1].ctypes.data, r[2].ctypes.data, r[3].ctypes.data, status.ctypes.data)
    return rc, r[0], r[1], r[2], r[3], status


def _ctx_array(ctxs):
    return (C.c_void_p * len(ctxs))(*[c.h for c in ctxs]), len(ctxs)


def encode_blocks_multi(ctxs, model, nblocks, in_ptr, in_off, flags, out_ptr, out_off):
    """zpq_encode_blocks_multi over the Contexts `ctxs` (one may be listed several times) on caller buffers.
    Returns (rc, out_len, status)."""
    return _enc_raw(lib().zpq_encode_blocks_multi, _ctx_array(ctxs) + (model.h, nblocks), nblocks, in_ptr, in_off, flags, out_ptr, out_off)


def decode_blocks_multi(ctxs, model, nblocks, in_ptr, in_off, flags, out_ptr, out_off):
    """zpq_decode_blocks_multi likewise.  Returns (rc, out_len, consumed, final_code, first_byte, status)."""
    return _dec_raw(lib().zpq_decode_blocks_multi, _ctx_array(ctxs) + (model.h, nblocks), nblocks, in_ptr, in_off, flags, out_ptr, out_off)


class Context:
    """One GPU (zpq_ctx).  Batch helpers take/return Python bytes for tests; the
    *_dev forms take raw device pointers (e.g. torch tensors' data_ptr())."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        self._children = weakref.WeakSet()                 # Blocks (and front-end handles) living on this ctx
        _ck(lib().zpq_ctx_create(device, C.byref(self.h)), "zpq_ctx_create")
        _LIVE_CTX.add(self)

    def close(self):
        """Destroy the ctx; whatever still lives on it is closed first."""
        for child in list(getattr(self, "_children", ())):
            try:
                child.close()
            except Exception:  # noqa: BLE001
                pass
        if getattr(self, "h", None) and _LIB is not None:
            _LIB.zpq_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        if not _FINALIZING:
            self.close()

    def sync(self):
        _ck(lib().zpq_ctx_sync(self.h), "zpq_ctx_sync")

    @property
    def stream(self):
        return lib().zpq_ctx_stream(self.h)

    @property
    def last_kernel_ms(self):
        return lib().zpq_ctx_last_kernel_ms(self.h)

    @property
    def last_kernel_name(self):
        return lib().zpq_ctx_last_kernel_name(self.h).decode()

    @property
    def last_slots(self):
        return lib().zpq_ctx_last_slots(self.h)

    @property
    def last_host_transfer(self):
        """What the host pipeline did with the last host-pointer batch: bit 0 striped upload, bit 1 early download,
        bits 8 and up the number of rounds (zpq_ctx_last_host_transfer)."""
        return lib().zpq_ctx_last_host_transfer(self.h)

    @property
    def last_line_store(self):
        """Lines per hash table of the compact line store the last launch ran with (0 = dense tables)."""
        return lib().zpq_ctx_last_line_store(self.h)

    def resident_capacity(self, model, flags=FLAG_PP):
        """Blocks of `model` one launch keeps resident on this GPU (zpq_ctx_resident_capacity)."""
        n = lib().zpq_ctx_resident_capacity(self.h, model.h, flags)
        if n < 0:
            raise ZpqError(n, "zpq_ctx_resident_capacity")
        return n

    def blockset_capacity(self, model, max_member_bytes=0, lanes=False, pipe=False, waves=False, vmwaves=False):
        """Members one BlockSet of `model` may hold on this GPU (zpq_blockset_capacity_ex; lanes / pipe / waves / vmwaves: with
        SET_LANES / SET_PIPE / SET_LANES | SET_WAVES / SET_LANES | SET_VMWAVES requested)."""
        n = lib().zpq_blockset_capacity_ex(self.h, model.h, max_member_bytes, _set_flags(lanes, pipe, waves, vmwaves))
        if n < 0:
            raise ZpqError(n, "zpq_blockset_capacity")
        return n

    def encode_blocks(self, model, blocks, flags=FLAG_PP, cap=None):
        nb = len(blocks)
        in_off = _offsets([len(b) for b in blocks])
        src = np.frombuffer(b"".join(blocks) + b"\0", dtype=np.uint8)
        caps = [cap if cap is not None else len(b) * 17 + 4096 for b in blocks]
        out_off = _offsets(caps)
        out = np.zeros(int(out_off[-1]) + 1, dtype=np.uint8)
        out_len = np.zeros(nb, dtype=np.uint32)
        status = np.zeros(nb, dtype=np.int32)
        _ck(lib().zpq_encode_blocks(self.h, model.h, nb, src.ctypes.data, in_off.ctypes.data, flags,
                                    out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data,
                                    status.ctypes.data), "zpq_encode_blocks")
        res = []
        for i in range(nb):
            o = int(out_off[i])
            res.append(out[o:o + min(int(out_len[i]), caps[i])].tobytes())
        return res, status, out_len

    def sha1_blocks(self, blocks):
        """SHA-1 of each byte string, one message per GPU lane (zpq_sha1_blocks; sha1.v:6-146)."""
        nb = len(blocks)
        in_off = _offsets([len(b) for b in blocks])
        src = np.frombuffer(b"".join(blocks) + b"\0", dtype=np.uint8)
        out = np.zeros(20 * nb + 1, dtype=np.uint8)
        _ck(lib().zpq_sha1_blocks(self.h, nb, src.ctypes.data, in_off.ctypes.data, out.ctypes.data), "zpq_sha1_blocks")
        return [out[20 * i:20 * i + 20].tobytes() for i in range(nb)]

    def sha1_blocks_dev(self, nblocks, d_in, d_in_off, d_out20):
        _ck(lib().zpq_sha1_blocks_dev(self.h, nblocks, d_in, d_in_off, d_out20), "zpq_sha1_blocks_dev")

    def decode_blocks(self, model, coded, cap, flags=FLAG_PP):
        nb = len(coded)
        in_off = _offsets([len(b) for b in coded])
        src = np.frombuffer(b"".join(coded) + b"\0", dtype=np.uint8)
        out_off = _offsets([cap] * nb)
        out = np.zeros(int(out_off[-1]) + 1, dtype=np.uint8)
        out_len = np.zeros(nb, dtype=np.uint32)
        consumed = np.zeros(nb, dtype=np.uint32)
        code = np.zeros(nb, dtype=np.uint32)
        first = np.zeros(nb, dtype=np.uint32)
        status = np.zeros(nb, dtype=np.int32)
        _ck(lib().zpq_decode_blocks(self.h, model.h, nb, src.ctypes.data, in_off.ctypes.data, flags,
                                    out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data,
                                    consumed.ctypes.data, code.ctypes.data, first.ctypes.data,
                                    status.ctypes.data), "zpq_decode_blocks")
        res = []
        for i in range(nb):
            o = int(out_off[i])
            res.append(out[o:o + min(int(out_len[i]), cap)].tobytes())
        return res, status, consumed, code, first

    def encode_blocks_dev(self, model, nblocks, d_in, d_in_off, flags, d_out, d_out_off, d_out_len, d_status):
        _ck(lib().zpq_encode_blocks_dev(self.h, model.h, nblocks, d_in, d_in_off, flags, d_out, d_out_off,
                                        d_out_len, d_status), "zpq_encode_blocks_dev")

    def decode_blocks_dev(self, model, nblocks, d_in, d_in_off, flags, d_out, d_out_off, d_out_len,
                          d_consumed, d_code, d_first, d_status):
        _ck(lib().zpq_decode_blocks_dev(self.h, model.h, nblocks, d_in, d_in_off, flags, d_out, d_out_off,
                                        d_out_len, d_consumed, d_code, d_first, d_status),
            "zpq_decode_blocks_dev")

    # ---- raw forms: the caller's own buffers and offsets (any window of them), nothing raised -- rc comes back first
    def encode_blocks_raw(self, model, nblocks, in_ptr, in_off, flags, out_ptr, out_off):
        """zpq_encode_blocks on caller buffers: in_ptr / out_ptr are host addresses, in_off / out_off uint64 arrays of
        nblocks + 1 entries (in_off[0] and out_off[0] need not be 0).  Returns (rc, out_len, status)."""
        return _enc_raw(lib().zpq_encode_blocks, (self.h, model.h, nblocks), nblocks, in_ptr, in_off, flags, out_ptr, out_off)

    def decode_blocks_raw(self, model, nblocks, in_ptr, in_off, flags, out_ptr, out_off):
        """zpq_decode_blocks likewise.  Returns (rc, out_len, consumed, final_code, first_byte, status)."""
        return _dec_raw(lib().zpq_decode_blocks, (self.h, model.h, nblocks), nblocks, in_ptr, in_off, flags, out_ptr, out_off)

    def sha1_blocks_raw(self, nblocks, in_ptr, in_off):
        """zpq_sha1_blocks on a caller buffer and offsets.  Returns (rc, the digests)."""
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        out = np.zeros(20 * nblocks + 1, dtype=np.uint8)
        rc = lib().zpq_sha1_blocks(self.h, nblocks, in_ptr, in_off.ctypes.data, out.ctypes.data)
        return rc, [out[20 * i:20 * i + 20].tobytes() for i in range(nblocks)]

    def sha1_ranges_dev(self, nranges, d_in, d_begin, d_end, d_out20):
        _ck(lib().zpq_sha1_ranges_dev(self.h, nranges, d_in, d_begin, d_end, d_out20), "zpq_sha1_ranges_dev")

    def gather_dev(self, nblocks, d_src, d_src_off, d_len, d_dst, d_dst_off):
        _ck(lib().zpq_gather_dev(self.h, nblocks, d_src, d_src_off, d_len, d_dst, d_dst_off), "zpq_gather_dev")

    def debug_pool_residue(self, nslots):
        """Apply the dirty-line logs' clear to the pool's first `nslots` slots; the non-zero 16-byte words left (0 = the logs
        name every dirty line).  ZpqError unless the last launches left valid logs for that many slots."""
        count = C.c_uint64(0)
        _ck(lib().zpq_debug_pool_residue(self.h, nslots, C.byref(count)), "zpq_debug_pool_residue")
        return int(count.value)

    def debug_dlog_counts(self, nslots):
        """The dirty-line logs' counts of the pool's first `nslots` slots, [nslots, 3], as the last launch left them (nothing
        is cleared).  ZpqError unless the last launches left valid logs for that many slots."""
        counts = np.zeros((nslots, 3), dtype=np.uint32)
        _ck(lib().zpq_debug_dlog_counts(self.h, nslots, counts.ctypes.data), "zpq_debug_dlog_counts")
        return counts

    def debug_contexts(self, model, data):
        n = model.ncomp
        out = np.zeros(max(1, len(data) * n), dtype=np.uint32)
        _ck(lib().zpq_debug_contexts(self.h, model.h, data, len(data), out.ctypes.data), "zpq_debug_contexts")
        return out[:len(data) * n].reshape(len(data), n)

    def debug_encode_trace(self, model, data, ntrace, flags=FLAG_PP):
        cap = len(data) * 17 + 4096
        out = C.create_string_buffer(cap)
        olen = C.c_size_t()
        tr = np.zeros(ntrace, dtype=np.int32)
        _ck(lib().zpq_debug_encode_trace(self.h, model.h, data, len(data), flags, out, cap, C.byref(olen),
                                         tr.ctypes.data, ntrace), "zpq_debug_encode_trace")
        return out.raw[:olen.value], tr


class Block:
    """One ZPAQ block whose model state persists across segments (zpq_block)."""

    def __init__(self, ctx, model):
        self.ctx, self.model = ctx, model
        self.h = C.c_void_p()
        _ck(lib().zpq_block_create(ctx.h, model.h, C.byref(self.h)), "zpq_block_create")
        ctx._children.add(self)

    def close(self):
        if getattr(self, "h", None) and _LIB is not None:
            _LIB.zpq_block_destroy(self.h)
            self.h = None

    def __del__(self):
        if not _FINALIZING:
            self.close()

    def encode_segment(self, data, flags=FLAG_PP, cap=None):
        cap = cap if cap is not None else len(data) * 17 + 4096
        out = C.create_string_buffer(cap)
        olen = C.c_size_t()
        _ck(lib().zpq_block_encode_segment(self.h, data, len(data), flags, out, cap, C.byref(olen)),
            "zpq_block_encode_segment")
        return out.raw[:olen.value]

    def decode_segment(self, coded, cap, flags=FLAG_PP):
        out = C.create_string_buffer(max(cap, 1))
        olen, cons = C.c_size_t(), C.c_size_t()
        code, first = C.c_uint32(), C.c_uint32()
        _ck(lib().zpq_block_decode_segment(self.h, coded, len(coded), flags, out, cap, C.byref(olen),
                                           C.byref(cons), C.byref(code), C.byref(first)),
            "zpq_block_decode_segment")
        return out.raw[:olen.value], cons.value, code.value, first.value


def _set_flags(lanes, pipe, waves, vmwaves=False, chunks=False):
    return ((SET_LANES if lanes or waves or vmwaves or chunks else 0) | (SET_PIPE if pipe else 0) | (SET_WAVES if waves else 0)
            | (SET_VMWAVES if vmwaves else 0) | (SET_CHUNKS if chunks else 0))


class BlockSet:
    """N ZPAQ blocks whose model state persists across segments, coded a segment of each per call (zpq_blockset):
    every call is one launch for all listed members.  `members` = distinct member indices in any order (None =
    0 .. n-1); a member whose segment failed keeps reporting that status.  lanes=True requests the lane-per-component
    kernels for a model no chain kernel takes (ZPQ_SET_LANES: one launch per call instead of one per member); the
    read-only `lanes` tells whether the library honoured it.  pipe=True requests the wave-pipelined encoder for a chain
    model (ZPQ_SET_PIPE: encode calls with at least 12 live members; same coded bytes); read-only `pipe` likewise.
    waves=True requests, with lanes, the wave-per-component kernels (ZPQ_SET_LANES | ZPQ_SET_WAVES: k_wset / k_wsetd for a
    model both take; same coded bytes); read-only `waves` likewise.  vmwaves=True requests, with lanes, the same for a
    model whose HCOMP program is not the shipped hash chain (ZPQ_SET_LANES | ZPQ_SET_VMWAVES: k_vset / k_vsetd, with a wave
    that runs the ZPAQL interpreter; same coded bytes); read-only `vmwaves` likewise.  No model gets both.  chunks=True requests,
    with lanes, that encode_chunks / decode_chunks code such a set, on k_rows / k_lanes (ZPQ_SET_LANES | ZPQ_SET_CHUNKS; without
    it they raise ZPQ_E_ARG on a lanes set); read-only `chunks` likewise."""

    def __init__(self, ctx, model, nmembers, max_member_bytes=0, lanes=False, pipe=False, waves=False, vmwaves=False, chunks=False):
        self.ctx, self.model, self.nmembers = ctx, model, nmembers
        self.h = C.c_void_p()
        _ck(lib().zpq_blockset_create_ex(ctx.h, model.h, nmembers, max_member_bytes,
                                         _set_flags(lanes, pipe, waves, vmwaves, chunks), C.byref(self.h)),
            "zpq_blockset_create")
        self._lanes = bool(lib().zpq_blockset_flags(self.h) & SET_LANES)
        self._pipe = bool(lib().zpq_blockset_flags(self.h) & SET_PIPE)
        self._waves = bool(lib().zpq_blockset_flags(self.h) & SET_WAVES)
        self._vmwaves = bool(lib().zpq_blockset_flags(self.h) & SET_VMWAVES)
        self._chunks = bool(lib().zpq_blockset_flags(self.h) & SET_CHUNKS)
        ctx._children.add(self)

    @property
    def lanes(self):
        return self._lanes

    @property
    def pipe(self):
        return self._pipe

    @property
    def waves(self):
        return self._waves

    @property
    def vmwaves(self):
        return self._vmwaves

    @property
    def chunks(self):
        return self._chunks

    def close(self):
        if getattr(self, "h", None) and _LIB is not None:
            _LIB.zpq_blockset_destroy(self.h)
            self.h = None

    def __del__(self):
        if not _FINALIZING:
            self.close()

    @staticmethod
    def _members(members, n):
        if members is None:
            return None, None
        arr = np.asarray(members, dtype=np.int32)
        assert len(arr) == n
        return arr, arr.ctypes.data

    def encode_segments(self, segments, members=None, flags=FLAG_PP, cap=None):
        n = len(segments)
        keep, mp = self._members(members, n)
        in_off = _offsets([len(b) for b in segments])
        src = np.frombuffer(b"".join(segments) + b"\0", dtype=np.uint8)
        if isinstance(cap, (list, tuple)):                 # one output capacity per segment
            caps = [int(x) for x in cap]
        else:
            caps = [cap if cap is not None else len(b) * 17 + 4096 for b in segments]
        out_off = _offsets(caps)
        out = np.zeros(int(out_off[-1]) + 1, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint32)
        status = np.zeros(n, dtype=np.int32)
        _ck(lib().zpq_blockset_encode_segments(self.h, n, mp, src.ctypes.data, in_off.ctypes.data, flags, out.ctypes.data,
                                               out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data),
            "zpq_blockset_encode_segments")
        res = [out[int(out_off[i]):int(out_off[i]) + min(int(out_len[i]), caps[i])].tobytes() for i in range(n)]
        return res, status, out_len

    def encode_segments_raw(self, members, in_ptr, in_off, flags, out_ptr, out_off):
        """zpq_blockset_encode_segments on caller buffers and offsets (any window).  Returns (rc, out_len, status)."""
        keep, mp = self._members(members, len(in_off) - 1)
        return _enc_raw(lib().zpq_blockset_encode_segments, (self.h, len(in_off) - 1, mp), len(in_off) - 1, in_ptr, in_off,
                        flags, out_ptr, out_off)

    def decode_segments_raw(self, members, in_ptr, in_off, flags, out_ptr, out_off):
        """zpq_blockset_decode_segments likewise.  Returns (rc, out_len, consumed, final_code, first_byte, status)."""
        keep, mp = self._members(members, len(in_off) - 1)
        return _dec_raw(lib().zpq_blockset_decode_segments, (self.h, len(in_off) - 1, mp), len(in_off) - 1, in_ptr, in_off,
                        flags, out_ptr, out_off)

    def decode_segments(self, coded, cap, members=None, flags=FLAG_PP):
        n = len(coded)
        keep, mp = self._members(members, n)
        in_off = _offsets([len(b) for b in coded])
        src = np.frombuffer(b"".join(coded) + b"\0", dtype=np.uint8)
        out_off = _offsets([cap] * n)
        out = np.zeros(int(out_off[-1]) + 1, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint32)
        consumed = np.zeros(n, dtype=np.uint32)
        code = np.zeros(n, dtype=np.uint32)
        first = np.zeros(n, dtype=np.uint32)
        status = np.zeros(n, dtype=np.int32)
        _ck(lib().zpq_blockset_decode_segments(self.h, n, mp, src.ctypes.data, in_off.ctypes.data, flags, out.ctypes.data,
                                               out_off.ctypes.data, out_len.ctypes.data, consumed.ctypes.data,
                                               code.ctypes.data, first.ctypes.data, status.ctypes.data),
            "zpq_blockset_decode_segments")
        res = [out[int(out_off[i]):int(out_off[i]) + min(int(out_len[i]), cap)].tobytes() for i in range(n)]
        return res, status, consumed, code, first

    def member_open(self, m):
        """Is member m's segment open, i.e. did a chunk call leave it unfinished (zpq_blockset_member_open)?"""
        rc = lib().zpq_blockset_member_open(self.h, m)
        if rc < 0:
            raise ZpqError(rc, "zpq_blockset_member_open")
        return bool(rc)

    def encode_chunks(self, chunks, more, members=None, flags=FLAG_PP, cap=None):
        """zpq_blockset_encode_chunks: the next piece of each listed member's segment; more[i] true = the segment goes on
        after it (None = every chunk ends its segment).  A segment's pieces joined are what encode_segments gives for the
        whole of it.  Returns (coded, status, out_len)."""
        n = len(chunks)
        keep, mp = self._members(members, n)
        in_off = _offsets([len(b) for b in chunks])
        src = np.frombuffer(b"".join(chunks) + b"\0", dtype=np.uint8)
        if isinstance(cap, (list, tuple)):                 # one output capacity per chunk
            caps = [int(x) for x in cap]
        else:
            caps = [cap if cap is not None else len(b) * 17 + 4096 for b in chunks]
        out_off = _offsets(caps)
        out = np.zeros(int(out_off[-1]) + 1, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint32)
        status = np.zeros(n, dtype=np.int32)
        mo = None if more is None else np.asarray([1 if x else 0 for x in more], dtype=np.uint8)
        assert mo is None or len(mo) == n
        _ck(lib().zpq_blockset_encode_chunks(self.h, n, mp, src.ctypes.data, in_off.ctypes.data, flags,
                                             None if mo is None else mo.ctypes.data, out.ctypes.data, out_off.ctypes.data,
                                             out_len.ctypes.data, status.ctypes.data),
            "zpq_blockset_encode_chunks")
        res = [out[int(out_off[i]):int(out_off[i]) + min(int(out_len[i]), caps[i])].tobytes() for i in range(n)]
        return res, status, out_len

    def decode_chunks(self, coded, cap, members=None, flags=FLAG_PP):
        """zpq_blockset_decode_chunks: up to cap (one number, or one per member) more bytes of each listed member's segment
        from coded[i], the coded bytes from where the member's decoder stands on.  A decoder whose slab is full pauses
        (open[i] = 1) instead of overflowing.  Returns (bytes, status, consumed, final_code, first_byte, open)."""
        n = len(coded)
        keep, mp = self._members(members, n)
        in_off = _offsets([len(b) for b in coded])
        src = np.frombuffer(b"".join(coded) + b"\0", dtype=np.uint8)
        caps = [int(x) for x in cap] if isinstance(cap, (list, tuple)) else [int(cap)] * n
        out_off = _offsets(caps)
        out = np.zeros(int(out_off[-1]) + 1, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint32)
        consumed = np.zeros(n, dtype=np.uint32)
        code = np.zeros(n, dtype=np.uint32)
        first = np.zeros(n, dtype=np.uint32)
        opened = np.zeros(n, dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        _ck(lib().zpq_blockset_decode_chunks(self.h, n, mp, src.ctypes.data, in_off.ctypes.data, flags, out.ctypes.data,
                                             out_off.ctypes.data, out_len.ctypes.data, consumed.ctypes.data,
                                             code.ctypes.data, first.ctypes.data, opened.ctypes.data, status.ctypes.data),
            "zpq_blockset_decode_chunks")
        res = [out[int(out_off[i]):int(out_off[i]) + min(int(out_len[i]), caps[i])].tobytes() for i in range(n)]
        return res, status, consumed, code, first, opened

    def encode_chunks_raw(self, members, in_ptr, in_off, flags, more, out_ptr, out_off):
        """zpq_blockset_encode_chunks on caller buffers and offsets (any window).  Returns (rc, out_len, status)."""
        n = len(in_off) - 1
        keep, mp = self._members(members, n)
        mo = None if more is None else np.asarray([1 if x else 0 for x in more], dtype=np.uint8)
        fn = lib().zpq_blockset_encode_chunks
        return _enc_raw(lambda *a: fn(*a[:6], None if mo is None else mo.ctypes.data, *a[6:]), (self.h, n, mp), n, in_ptr,
                        in_off, flags, out_ptr, out_off)

    def decode_chunks_raw(self, members, in_ptr, in_off, flags, out_ptr, out_off):
        """zpq_blockset_decode_chunks likewise.  Returns (rc, out_len, consumed, final_code, first_byte, status, open)."""
        n = len(in_off) - 1
        keep, mp = self._members(members, n)
        opened = np.full(n, 0xEE, dtype=np.uint8)
        fn = lib().zpq_blockset_decode_chunks
        return _dec_raw(lambda *a: fn(*a[:-1], opened.ctypes.data, a[-1]), (self.h, n, mp), n, in_ptr, in_off, flags,
                        out_ptr, out_off) + (opened,)
