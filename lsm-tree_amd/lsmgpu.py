"""ctypes binding of lsm-tree_amd/liblsmgpu.so (include/lsmgpu.h) for tests and bench.

Device memory comes from torch CUDA tensors (plumbing only).  Every call goes
through the C ABI; there is no CPU fallback: importing this module on a box
without the built library raises, and calls without a GPU fail loudly.

The functions' signatures are not written down here: lib() types every entry
point from its prototype in include/lsmgpu.h (EXPORTED_SYMBOLS: their names in
header order), so a new entry point is declared in the header and listed in
exports.map, nowhere else.  Only the structs are mirrored (the Lsm* classes;
tests/test_abi.py holds them to the header).  Every wrapper takes its
temporary workspace from _workspace and reads device values back through
_read_back, which keep both sound on a caller's side stream.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

HERE = Path(__file__).resolve().parent
# LSMGPU_LIB: diagnostic override (tuning sweeps load variant builds of the same library)
LIB_PATH = Path(os.environ.get("LSMGPU_LIB", HERE / "liblsmgpu.so"))

LSM_HEADER_LEN = 33
LSM_TRAILER_LEN = 31
LSM_INPUT_PADDING = 64

STATUS = {0: "OK", 1: "BAD_MAGIC", 2: "BAD_TYPE", 3: "HDR_CKSUM", 4: "CKSUM", 5: "PARSE", 6: "OVERFLOW",
          7: "TYPE_MISMATCH", 8: "TRUNCATED", 9: "UNSUPPORTED", 10: "BAD_ARG", 11: "HIP_ERROR",
          12: "DECOMPRESS", 13: "INCOMPLETE"}
BLOCK_DATA, BLOCK_INDEX, BLOCK_FILTER, BLOCK_META = 0, 1, 2, 3


class LsmItems(C.Structure):
    _fields_ = [("keys", C.c_void_p), ("key_off", C.c_void_p), ("vals", C.c_void_p), ("val_off", C.c_void_p),
                ("seqno", C.c_void_p), ("vtype", C.c_void_p), ("handle_off", C.c_void_p),
                ("handle_size", C.c_void_p), ("n_items", C.c_uint64)]


class LsmItems32(C.Structure):  # lsm_items32: u32 key / value offsets (lsm_encode_blocks32)
    _fields_ = [("keys", C.c_void_p), ("key_off", C.c_void_p), ("vals", C.c_void_p), ("val_off", C.c_void_p),
                ("seqno", C.c_void_p), ("vtype", C.c_void_p), ("handle_off", C.c_void_p),
                ("handle_size", C.c_void_p), ("n_items", C.c_uint64)]


class LsmParsed(C.Structure):
    _fields_ = [("seqno", C.c_void_p), ("key_off", C.c_void_p), ("val_off", C.c_void_p), ("val_len", C.c_void_p),
                ("key_len", C.c_void_p), ("prefix_len", C.c_void_p), ("vtype", C.c_void_p),
                ("handle_off", C.c_void_p)]


class LsmParsed16(C.Structure):
    _fields_ = [("seqno", C.c_void_p), ("key_off", C.c_void_p), ("val_off", C.c_void_p), ("val_len", C.c_void_p),
                ("key_len", C.c_void_p), ("prefix_len", C.c_void_p), ("vtype", C.c_void_p)]


class LsmBlockParams(C.Structure):
    _fields_ = [("restart_interval", C.c_uint8), ("block_type", C.c_uint8), ("compression", C.c_uint8),
                ("reserved", C.c_uint8), ("hash_ratio", C.c_float), ("flags", C.c_uint32)]


class LsmPointResult(C.Structure):
    _fields_ = [("item", C.c_void_p), ("seqno", C.c_void_p), ("val_off", C.c_void_p), ("val_len", C.c_void_p),
                ("vtype", C.c_void_p)]


class LsmDecodeTuning(C.Structure):
    _fields_ = [("blocks_per_wave", C.c_uint32), ("stage_bytes", C.c_uint32), ("tile_items", C.c_uint32),
                ("flags", C.c_uint32)]


class LsmTableScan(C.Structure):
    _fields_ = [("tli_off", C.c_uint64), ("tli_size", C.c_uint32), ("two_level", C.c_uint32),
                ("global_seqno", C.c_uint64), ("block_count", C.c_uint64)]


class LsmRangeResult(C.Structure):
    _fields_ = [("first_block_off", C.c_void_p), ("first_block_size", C.c_void_p), ("first_item", C.c_void_p),
                ("last_block_off", C.c_void_p), ("last_block_size", C.c_void_p), ("last_item", C.c_void_p),
                ("first_block", C.c_void_p), ("last_block", C.c_void_p)]


class LsmRangePositions(C.Structure):  # lsm_range_positions: lsm_table_range's outputs, read by lsm_table_range_rows
    _fields_ = [("outcome", C.c_void_p), ("status", C.c_void_p), ("first_block", C.c_void_p),
                ("first_item", C.c_void_p), ("last_block", C.c_void_p), ("last_item", C.c_void_p)]


class LsmTableFrames(C.Structure):  # lsm_table_frames: a table's data blocks as inflated frames (table_frames)
    _fields_ = [("stored_off", C.c_void_p), ("frames", C.c_void_p), ("frame_off", C.c_void_p),
                ("frame_status", C.c_void_p), ("frames_len", C.c_uint64), ("n_blocks", C.c_uint32)]


ABI_VERSION = 7
DECODE_ITEM_START_VALID = 1
# lsm_decode_tuning.flags / lsm_block_params.flags: take the workspace pool (explicit opt-in)
DECODE_HUGE_POOL = 4
ENCODE_HUGE_POOL = 1
ENCODE_RUN_PLAN = 2
# Mean block size (bytes) from which the wrappers hand the workspace pool for
# blocks spread over the GPU (blocks > 72 KiB decode, > 96 KiB images encode).
HUGE_AUTO_MEAN = 32 << 10
DECODE_PAYLOAD_VERIFIED = 2


class LsmError(RuntimeError):
    pass


def build():
    import subprocess
    subprocess.run(["make", "-s", "-C", str(HERE), "-j8"], check=True)


_lib = None


_C_SCALARS = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float,
              **{f"{u}int{b}_t": getattr(C, f"c_{u}int{b}") for u in ("", "u") for b in (8, 16, 32, 64)}}
_C_STRUCTS = {"lsm_items": LsmItems, "lsm_items32": LsmItems32, "lsm_parsed_items": LsmParsed,
              "lsm_parsed_items16": LsmParsed16, "lsm_block_params": LsmBlockParams,
              "lsm_point_result": LsmPointResult, "lsm_decode_tuning": LsmDecodeTuning,
              "lsm_table_scan": LsmTableScan, "lsm_range_result": LsmRangeResult,
              "lsm_range_positions": LsmRangePositions}


def _prototypes():
    """{name: (return type, [parameter types])} of every function include/lsmgpu.h declares, as C
    type strings, in header order."""
    text = re.sub(r"/\*.*?\*/", "", (HERE.parent / "include" / "lsmgpu.h").read_text(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"^(\w[\w \*]*?)\s*\b(lsm_\w+)\s*\(([^()]*)\)\s*;", text, re.M):
        params = [] if params.strip() == "void" else params.split(",")
        protos[name] = (ret, [re.sub(r"\w+\s*$", "", p) for p in params])  # (the type: all but the name)
    return protos


PROTOTYPES = _prototypes()
EXPORTED_SYMBOLS = list(PROTOTYPES)


def _c_type(name, ctype, ret=False):
    """The ctypes type of one parameter (ret: of the return value) of prototype `name`: a scalar,
    POINTER(the mirrored Structure), c_char_p for a returned const char*, c_void_p for every other
    pointer to a known type.  Anything else is an LsmError: the binding does not guess."""
    m = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*", ctype)
    base, ptr = m.groups() if m else (None, None)
    if base in _C_SCALARS and not ptr:
        return _C_SCALARS[base]
    if base in _C_STRUCTS and ptr:
        return C.POINTER(_C_STRUCTS[base])
    if base == "char" and ptr and ret:
        return C.c_char_p
    if (base == "void" or base in _C_SCALARS) and ptr:
        return C.c_void_p
    raise LsmError(f"{name}: no ctypes mapping for the C type {ctype.strip()!r} in include/lsmgpu.h")


def lib():
    """The loaded library, every function the header declares typed from its prototype.  A symbol
    the library lacks is skipped: LSMGPU_LIB may name a variant built from an earlier tree."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise LsmError(f"{LIB_PATH} not built: run `make -C {HERE}` (or __graft_entry__.build())")
        L = C.CDLL(str(LIB_PATH))
        for name, (ret, params) in PROTOTYPES.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.restype = _c_type(name, ret, ret=True)
                fn.argtypes = [_c_type(name, p) for p in params]
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise LsmError(f"{what} failed: {STATUS.get(rc, rc)} {lib().lsm_last_error().decode()}")


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise LsmError("no GPU visible: the lsmgpu product path has no CPU fallback")
    return torch


def _stream(stream):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _workspace(nbytes, device, stream=None):
    """A call's temporary workspace: uint8 [nbytes] on `device`, recorded on the stream the call
    launches on (`stream`, else the device's current one), so that the caching allocator hands
    the bytes on only to work queued after the kernels that use them."""
    torch = _torch()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    if ws.is_cuda:
        ws.record_stream(stream if stream is not None else torch.cuda.current_stream(ws.device))
    return ws


def _read_back(t, stream=None):
    """A device tensor's values on the host (tolist()), read after the work queued on `stream`:
    the copy runs on the current stream, which does not wait for a side stream by itself."""
    if stream is not None:
        stream.synchronize()
    return t.cpu().tolist()


ITEM_FIELDS = ("keys", "key_off", "vals", "val_off", "seqno", "vtype")


def _items_struct(items, fields=ITEM_FIELDS, cls=LsmItems):
    """The lsm_items (cls: LsmItems or LsmItems32) over those of `fields` an items dict holds, the
    others NULL, n_items from seqno.  Returns (struct, held): an empty tensor has no address and
    the library wants its arrays non-NULL, so one element stands in, kept alive by `held`."""
    it, held = cls(n_items=items["seqno"].numel()), []
    for f in fields:
        t = items.get(f)
        if t is not None and t.numel() == 0:
            t = t.new_zeros(1)
            held.append(t)
        setattr(it, f, t.data_ptr() if t is not None else None)
    return it, held


def _items_view(dst, rows=None):
    """The six lsm_items tensors of dst; rows: the per-row arrays trimmed to that many rows."""
    items = {f: dst[f] for f in ITEM_FIELDS}
    if rows is not None:
        items.update(key_off=dst["key_off"][:rows + 1], val_off=dst["val_off"][:rows + 1],
                     seqno=dst["seqno"][:rows], vtype=dst["vtype"][:rows])
    return items


def _parsed_struct(out, cls=LsmParsed):
    """The lsm_parsed_items (cls=LsmParsed16: lsm_parsed_items16) over a decode output dict; fields
    it does not hold are NULL (not written)."""
    return cls(*(_ptr(out.get(f)) for f, _ in cls._fields_))


def _table_struct(table, global_seqno=0, block_count=0):
    """The lsm_table_scan of a table dict (tli_off, tli_size, optionally two_level)."""
    return LsmTableScan(table["tli_off"], table["tli_size"], int(bool(table.get("two_level", False))),
                        global_seqno & (2 ** 64 - 1), block_count)


def _file_len(table, other_end=0):
    """table["file_len"], else the end of the TLI (or of another region that ends later)."""
    return table.get("file_len", max(table["tli_off"] + table["tli_size"], other_end))


def padded_bytes(n, device="cuda"):
    """uint8 device buffer of n bytes + LSM_INPUT_PADDING slack (16-aligned by the allocator)."""
    torch = _torch()
    buf = torch.zeros(n + LSM_INPUT_PADDING, dtype=torch.uint8, device=device)
    return buf


def to_device_bytes(data, device="cuda"):
    """Host bytes / numpy uint8 -> padded device buffer (first len bytes valid)."""
    import numpy as np
    torch = _torch()
    a = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, np.uint8)
    buf = padded_bytes(len(a), device)
    if len(a):
        buf[:len(a)].copy_(torch.from_numpy(a.copy()))
    return buf


PARSED_FIELDS = (("seqno", "int64"), ("key_off", "int32"), ("val_off", "int32"), ("val_len", "int32"),
                 ("key_len", "int16"), ("prefix_len", "int16"), ("vtype", "uint8"), ("handle_off", "int64"))
# lsm_parsed_items16: 16-bit payload offsets and lengths, 19 B/item (no handle_off)
PARSED16_FIELDS = (("seqno", "int64"), ("key_off", "int16"), ("val_off", "int16"), ("val_len", "int16"),
                   ("key_len", "int16"), ("prefix_len", "int16"), ("vtype", "uint8"))


class Decoder:
    """Reusable decode context: holds the workspace for up to n_blocks."""

    def __init__(self, device="cuda"):
        self.device = device
        self.ws = None

    def workspace(self, n_blocks, blocks_bytes=0):
        """Workspace for n_blocks; with blocks_bytes (the batch buffer's size) it
        includes the pool that spreads blocks > 72 KiB over the whole GPU.  The
        cached buffer is returned viewed at exactly the size this call needs:
        the library turns the pool on from the size it is handed (lsmgpu.h), so
        bytes grown by an earlier pool call must not reach a pool=False call."""
        torch = _torch()
        need = (lib().lsm_decode_workspace_size_ex(n_blocks, blocks_bytes) if blocks_bytes
                else lib().lsm_decode_workspace_size(n_blocks))
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        return self.ws[:need]

    def alloc_outputs(self, item_cap, n_blocks, fields=None, compact=False):
        torch = _torch()
        spec = PARSED16_FIELDS if compact else PARSED_FIELDS
        fields = fields or [f for f, _ in spec]
        out = {}
        for f, dt in spec:
            if f in fields:
                out[f] = torch.empty(max(item_cap, 1), dtype=getattr(torch, dt), device=self.device)
        out["item_start"] = torch.empty(n_blocks + 1, dtype=torch.int32, device=self.device)
        out["status"] = torch.empty(max(n_blocks, 1), dtype=torch.int32, device=self.device)
        return out

    def decode(self, blocks, block_off, n_blocks, out, item_cap, expect_type=-1, tuning=None, stream=None,
               compact=False, pool=None, workspace_bytes=None, blocks_bytes=None):
        """Enqueue lsm_decode_blocks (compact: lsm_decode_blocks16 into 16-bit
        offset arrays from alloc_outputs(..., compact=True)).  blocks: uint8 cuda
        (padded); block_off: int64 cuda [n+1].  pool=True: the workspace carries
        the pool that spreads blocks > 72 KiB over the GPU; False: the base
        workspace only (those blocks on one workgroup each); None (default): the
        pool when the batch's mean block is 32 KiB or more (its kernels cost a few
        microseconds per call even with no such block); workspace_bytes: pass
        exactly that much workspace (tests of a pool too small for the batch);
        blocks_bytes: the batch's size where it is a small part of `blocks` (an
        arena addressed by large offsets), default blocks.numel()."""
        if blocks_bytes is None:
            blocks_bytes = blocks.numel()
        if pool is None:
            pool = blocks_bytes >= HUGE_AUTO_MEAN * max(n_blocks, 1)
        if tuning is None and os.environ.get("LSMGPU_DECODE_TUNING"):  # diagnostic override
            tuning = tuple(int(x, 0) for x in os.environ["LSMGPU_DECODE_TUNING"].split(","))
        ws = self.workspace(n_blocks, blocks_bytes if pool else 0)
        if workspace_bytes is not None:
            ws = _workspace(max(workspace_bytes, 1), self.device, stream)[:workspace_bytes]
        if pool:  # the pool is an explicit opt-in (LSM_DECODE_HUGE_POOL), never implied by the size
            tuning = tuple(tuning or (0, 0, 0))
            tuning = tuning[:3] + ((tuning[3] if len(tuning) > 3 else 0) | DECODE_HUGE_POOL,)
        # (blocks_per_wave, stage_bytes, tile_items[, flags])
        t = C.byref(LsmDecodeTuning(*tuning)) if tuning is not None else None
        args = (_ptr(blocks), _ptr(block_off), n_blocks, expect_type)
        tail = (item_cap, _ptr(out["item_start"]), _ptr(out["status"]), _ptr(ws), ws.numel())
        if compact:
            for f, dt in PARSED16_FIELDS:
                if f in out and out[f].element_size() != C.sizeof(C.c_uint64 if dt == "int64" else
                                                                  C.c_uint16 if dt == "int16" else C.c_uint8):
                    raise LsmError(f"compact decode: field {f} must be {dt}")
            ps = _parsed_struct(out, LsmParsed16)
            _check(lib().lsm_decode_blocks16(*args, C.byref(ps), *tail, t, _stream(stream)), "lsm_decode_blocks16")
            return out
        ps = _parsed_struct(out)
        if t is not None:
            rc = lib().lsm_decode_blocks_tuned(*args, C.byref(ps), *tail, t, _stream(stream))
        else:
            rc = lib().lsm_decode_blocks(*args, C.byref(ps), *tail, _stream(stream))
        _check(rc, "lsm_decode_blocks")
        return out


def decode_blocks(blocks, block_off, n_blocks=None, expect_type=-1, item_cap=None, fields=None, tuning=None,
                  compact=False, pool=None, workspace_bytes=None, blocks_bytes=None):
    """Convenience: decode device blocks, returns dict of device tensors
    (compact: the 19 B/item lsm_parsed_items16 layout).  blocks_bytes: the
    batch's size where it is a small part of `blocks`, default blocks.numel()."""
    n_blocks = (block_off.numel() - 1) if n_blocks is None else n_blocks
    if item_cap is None:
        item_cap = (blocks.numel() if blocks_bytes is None else blocks_bytes) // 3 + 1
    d = Decoder(blocks.device)
    out = d.alloc_outputs(item_cap, n_blocks, fields, compact)
    return d.decode(blocks, block_off, n_blocks, out, item_cap, expect_type, tuning, compact=compact, pool=pool,
                    workspace_bytes=workspace_bytes, blocks_bytes=blocks_bytes)


class Encoder:
    def __init__(self, device="cuda"):
        self.device = device
        self.ws = None

    def encode(self, items, starts, n_blocks, restart_interval=16, hash_ratio=0.0, block_type=BLOCK_DATA,
               out=None, stream=None, pool=None, workspace_bytes=None, run_plan=False):
        """items: dict of cuda tensors keys(u8, padded) key_off(i64 n+1) vals(u8, padded) val_off(i64 n+1)
        seqno(i64) vtype(u8) [handle_off(i64) handle_size(i32)]; starts: int32 cuda [n_blocks+1].
        key_off / val_off as int32 tensors (arenas < 4 GiB): lsm_encode_blocks32 (u32 offsets).
        pool=False: the base workspace only (blocks > 96 KiB on one workgroup each);
        None (default): the pool when the output bound averages 32 KiB per block or more;
        workspace_bytes: pass exactly that much workspace (tests of a pool too small)."""
        torch = _torch()
        n_items = items["seqno"].numel()
        off32 = items["key_off"].element_size() == 4
        if off32 and "val_off" in items and items["val_off"].element_size() != 4:
            raise LsmError("key_off and val_off must have the same width")
        # (index-form items carry no values: the value fields then alias the keys)
        it, held = _items_struct({"vals": items["keys"], "val_off": items["key_off"], **items},
                                 ITEM_FIELDS + ("handle_off", "handle_size"), LsmItems32 if off32 else LsmItems)
        params = LsmBlockParams(restart_interval, block_type, 0, 0, hash_ratio, 0)
        key_bytes = int(items["keys"].numel())
        val_bytes = int(items["vals"].numel()) if "vals" in items else 0
        bound = lib().lsm_encode_bound(n_items, n_blocks, key_bytes, val_bytes, C.byref(params))
        if pool is None:
            pool = bound >= HUGE_AUTO_MEAN * max(n_blocks, 1)
        if pool:  # the pool is an explicit opt-in (LSM_ENCODE_HUGE_POOL), never implied by the size
            params.flags = ENCODE_HUGE_POOL
        if run_plan:  # LSM_ENCODE_RUN_PLAN (the library also takes it by itself for long blocks)
            params.flags |= ENCODE_RUN_PLAN
        need = (lib().lsm_encode_workspace_size_ex(n_items, n_blocks, bound) if pool
                else lib().lsm_encode_workspace_size(n_items, n_blocks))
        if workspace_bytes is not None:
            need = workspace_bytes
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        if out is None or out["buf"].numel() < bound:
            out = {"buf": torch.empty(bound + LSM_INPUT_PADDING, dtype=torch.uint8, device=self.device),
                   "block_off": torch.empty(n_blocks + 1, dtype=torch.int64, device=self.device),
                   "status": torch.empty(max(n_blocks, 1), dtype=torch.int32, device=self.device)}
        fn = lib().lsm_encode_blocks32 if off32 else lib().lsm_encode_blocks
        rc = fn(C.byref(it), _ptr(starts), n_blocks, C.byref(params), _ptr(out["buf"]), bound,
                _ptr(out["block_off"]), _ptr(out["status"]), _ptr(self.ws), need, _stream(stream))
        _check(rc, "lsm_encode_blocks32" if off32 else "lsm_encode_blocks")
        return out


def xxh3_128_batch(data, off, n):
    torch = _torch()
    out = torch.empty(2 * max(n, 1), dtype=torch.int64, device=data.device)
    _check(lib().lsm_xxh3_128_batch(_ptr(data), _ptr(off), n, _ptr(out), _stream(None)), "lsm_xxh3_128_batch")
    return out


def _point_result(out):
    """The LsmPointResult over an output dict's item/seqno/val_off/val_len/vtype tensors."""
    return LsmPointResult(*(_ptr(out[f]) for f in ("item", "seqno", "val_off", "val_len", "vtype")))


def point_read(blocks, block_off, n_blocks, query_block, needles, needle_off, snapshot, stream=None):
    """Batched DataBlock::point_read (data_block/mod.rs:412-472).  All inputs cuda
    tensors: blocks uint8 (padded), block_off int64 [n_blocks+1], query_block
    int32 [n], needles uint8 (padded arena), needle_off int64 [n+1], snapshot
    int64 [n].  Returns dict item/seqno/val_off/val_len/vtype/status (item -1 = None)."""
    torch = _torch()
    n = int(query_block.numel())
    dev = blocks.device
    out = {"item": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
           "seqno": torch.zeros(max(n, 1), dtype=torch.int64, device=dev),
           "val_off": torch.zeros(max(n, 1), dtype=torch.int32, device=dev),
           "val_len": torch.zeros(max(n, 1), dtype=torch.int32, device=dev),
           "vtype": torch.zeros(max(n, 1), dtype=torch.uint8, device=dev),
           "status": torch.empty(max(n, 1), dtype=torch.int32, device=dev)}
    res = _point_result(out)
    _check(lib().lsm_point_read_blocks(_ptr(blocks), _ptr(block_off), n_blocks, _ptr(query_block), _ptr(needles),
                                       _ptr(needle_off), _ptr(snapshot), n, C.byref(res), _ptr(out["status"]),
                                       _stream(stream)), "lsm_point_read_blocks")
    return out


GET_NONE, GET_SEQNO_SKIP, GET_FILTERED, GET_NO_BLOCK, GET_MISS, GET_HIT = range(6)
TABLE_GET_FIELDS = (("item", "int32"), ("seqno", "int64"), ("val_off", "int32"), ("val_len", "int32"),
                    ("vtype", "uint8"), ("block_off", "int64"), ("block_size", "int32"), ("outcome", "uint8"),
                    ("status", "int32"))


def _frames_struct(frames):
    """The lsm_table_frames of a view dict (table_frames' result, or one built by hand: stored_off,
    frames, frame_off, n_blocks, frames_len and an optional status)."""
    return LsmTableFrames(_ptr(frames["stored_off"]), _ptr(frames["frames"]), _ptr(frames["frame_off"]),
                          _ptr(frames.get("status")), int(frames["frames_len"]), int(frames["n_blocks"]))


def table_get(file, table, needles, needle_off, snapshot, key_hash=None, active=None, filter=None, lowest_seqno=0,
              global_seqno=0, stream=None, out=None, frames=None):
    """Batched Table::get (src/table/mod.rs:229-340) on a table file image: file = padded uint8
    cuda tensor; table = dict with tli_off, tli_size, two_level (write_table's result with
    two_level added; an optional file_len, else the end of the TLI / filter region); needles uint8
    (padded arena), needle_off int64 [n+1], snapshot int64 [n]; key_hash int64 [n] (xxh3_64 of each
    needle) or None; active uint8 [n] or None; filter = (off, size) of the filter block or None.
    Returns dict of cuda tensors item/seqno/val_off/val_len/vtype/block_off/block_size/outcome
    (GET_*)/status; item -1 = no hit, the value of a hit is
    file[block_off + 33 + val_off : ... + val_len].  out: such a dict to write into (rows of
    inactive queries keep what it holds), e.g. the result of the previous, newer table.
    frames: table_frames' view of an LZ4 table (lsm_table_get_framed): block_off / block_size are
    the stored handle, the result gains block (int32: the handle's ordinal in frames["stored_off"])
    and the value of a hit is frames["frames"][frame_off[block] + 33 + val_off : ... + val_len].
    No host synchronisation."""
    torch = _torch()
    n = int(snapshot.numel())
    dev = file.device
    if out is None:
        out = {f: torch.zeros(max(n, 1), dtype=getattr(torch, dt), device=dev) for f, dt in TABLE_GET_FIELDS}
    f_off, f_size = filter if filter is not None else (0, 0)
    t = _table_struct(table, global_seqno)
    res = _point_result(out)
    args = (_ptr(file), _file_len(table, f_off + f_size), C.byref(t), f_off, f_size, lowest_seqno, _ptr(needles),
            _ptr(needle_off), _ptr(snapshot), _ptr(key_hash), _ptr(active), n, C.byref(res), _ptr(out["block_off"]),
            _ptr(out["block_size"]), _ptr(out["outcome"]), _ptr(out["status"]))
    if frames is None:
        _check(lib().lsm_table_get(*args, _stream(stream)), "lsm_table_get")
        return out
    if "block" not in out:
        out["block"] = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    view = _frames_struct(frames)
    _check(lib().lsm_table_get_framed(*args, C.byref(view), _ptr(out["block"]), _stream(stream)),
           "lsm_table_get_framed")
    return out


SEEK_LO, SEEK_HI, SEEK_LO_EXCLUSIVE, SEEK_HI_EXCLUSIVE = 1, 2, 4, 8

RANGE_NONE, RANGE_NO_BLOCK, RANGE_EMPTY, RANGE_ROWS = range(4)
TABLE_RANGE_FIELDS = (("first_block_off", "int64"), ("first_block_size", "int32"), ("first_item", "int32"),
                      ("last_block_off", "int64"), ("last_block_size", "int32"), ("last_item", "int32"),
                      ("first_block", "int32"), ("last_block", "int32"), ("outcome", "uint8"), ("status", "int32"))


def table_range(file, table, lo, lo_off, hi, hi_off, flags, scan=None, out=None, stream=None, frames=None):
    """Batched Table::range bounds (src/table/mod.rs:391-422, the forward drain of
    src/table/iter.rs:94-293) on a table file image: file = padded uint8 cuda tensor; table = dict
    with tli_off, tli_size, two_level (and an optional file_len, else the end of the TLI); lo / hi
    uint8 padded arenas with int64 [n+1] offsets and flags uint8 [n] (SEEK_* bits) as seek().
    Returns dict of cuda tensors first_block_off / first_block_size / first_item (the first row:
    its block's handle and its index in the block), last_* (the last row, inclusive), outcome
    (RANGE_*) and status; rows whose outcome is not RANGE_ROWS keep what the tensors held.
    out: such a dict to write into.  scan: a dict holding block_off (the table's data-block offsets,
    int64 [n_blocks + 1], n_blocks taken from scan["n_blocks"] when that is an int) and item_start,
    as scan_table returns: first_block / last_block are then the two blocks' ordinals, and
    row_first / row_end the row window [item_start[first_block] + first_item,
    item_start[last_block] + last_item + 1) of the scan, 0 / 0 where the outcome is not RANGE_ROWS.
    frames: table_frames' view of an LZ4 table (lsm_table_range_framed): the handles are the stored
    ones, first_block / last_block their ordinals in frames["stored_off"] (scan's block_off is not
    read; its item_start still gives the row window), the items index the decompressed blocks.
    No host synchronisation."""
    torch = _torch()
    n = int(flags.numel())
    dev = file.device
    if out is None:
        out = {f: torch.zeros(max(n, 1), dtype=getattr(torch, dt), device=dev) for f, dt in TABLE_RANGE_FIELDS}
    t = _table_struct(table)
    block_off, n_blocks = None, 0
    if scan is not None:
        block_off = scan["block_off"]
        nb = scan.get("n_blocks")
        n_blocks = nb if isinstance(nb, int) else int(block_off.numel()) - 1
    res = LsmRangeResult(*(_ptr(out[f]) if block_off is not None or frames is not None or not f.endswith("_block")
                           else None for f, _ in TABLE_RANGE_FIELDS[:8]))
    head = (_ptr(file), _file_len(table), C.byref(t), _ptr(lo), _ptr(lo_off), _ptr(hi), _ptr(hi_off), _ptr(flags), n)
    tail = (C.byref(res), _ptr(out["outcome"]), _ptr(out["status"]), _stream(stream))
    if frames is None:
        _check(lib().lsm_table_range(*head, _ptr(block_off), n_blocks, *tail), "lsm_table_range")
    else:
        view = _frames_struct(frames)
        _check(lib().lsm_table_range_framed(*head, C.byref(view), *tail), "lsm_table_range_framed")
    if scan is not None:
        rows = out["outcome"][:n] == RANGE_ROWS
        start = scan["item_start"].to(torch.int64)
        # (rows the kernel left alone may hold anything: gather at 0 there)
        fb = torch.where(rows, out["first_block"][:n].to(torch.int64), 0).clamp_(0, start.numel() - 1)
        lb = torch.where(rows, out["last_block"][:n].to(torch.int64), 0).clamp_(0, start.numel() - 1)
        zero = torch.zeros((), dtype=torch.int64, device=dev)
        out["row_first"] = torch.where(rows, start[fb] + out["first_item"][:n], zero)
        out["row_end"] = torch.where(rows, start[lb] + out["last_item"][:n] + 1, zero)
    return out


def table_block_offsets(file, table, data_off=0):
    """The data-block offsets of a table (int64 cuda [n_blocks + 1], what table_range takes as
    scan["block_off"] and table_range_rows as block_off) from its block index alone, for a reader
    that never scanned the table: the TLI's entries, or, when table["two_level"], the entries of
    the partitions the TLI names, decoded as index blocks (decode_blocks, which verifies them).
    table as table_range takes it.  Raises LsmError when an index block does not decode or the
    handles are not contiguous from data_off (default 0: the layout a scan reads back to back; a
    table laid further into a larger image gives the offset of its first data block).
    Synchronises."""
    import numpy as np
    torch = _torch()
    dev = file.device
    file_len = _file_len(table)

    def entries(handles):
        """[(off, size)] of index blocks -> the handles their entries hold, in order."""
        out, i = [], 0
        while i < len(handles):  # one decode per run of blocks that lie back to back
            j = i + 1
            while j < len(handles) and handles[j][0] == handles[j - 1][0] + handles[j - 1][1]:
                j += 1
            run = handles[i:j]
            if any(size < LSM_HEADER_LEN for _, size in run) or run[-1][0] + run[-1][1] > file_len:
                raise LsmError("table_block_offsets: an index block's handle does not lie in the file")
            off = torch.tensor([h[0] for h in run] + [run[-1][0] + run[-1][1]], dtype=torch.int64, device=dev)
            cap = sum(size for _, size in run) // 5 + len(run)  # (an index record takes 5 bytes or more)
            d = decode_blocks(file, off, len(run), expect_type=BLOCK_INDEX, item_cap=cap,
                              fields=["handle_off", "val_len"], blocks_bytes=sum(size for _, size in run))
            status = d["status"][:len(run)].cpu().numpy()
            if status.any():
                raise LsmError(f"table_block_offsets: index block status {STATUS.get(int(status.max()), '?')}")
            n = int(d["item_start"][len(run)].item())
            out += zip(d["handle_off"][:n].cpu().tolist(), d["val_len"][:n].cpu().numpy().view(np.uint32).tolist())
            i = j
        return out

    handles = entries([(table["tli_off"], table["tli_size"])])
    if table.get("two_level", False):
        handles = entries(handles)
    off = np.full(len(handles) + 1, data_off, np.int64)
    for i, (o, size) in enumerate(handles):
        if o != off[i]:
            raise LsmError(f"table_block_offsets: data block {i} at {o}, not contiguous from {data_off}")
        off[i + 1] = o + size
    if off[-1] > file_len:
        raise LsmError("table_block_offsets: the data blocks end past the file")
    return torch.from_numpy(off).to(dev)


RANGE_ROWS_AUTO_PAIRS = 1 << 22


def table_range_rows(file, table, positions, block_off, base=None, into=None, caps=None, stream=None,
                     n_queries=None, frames=None):
    """lsm_table_range_rows_plan + lsm_table_range_rows: the rows between the positions of
    table_range, as item runs.  file / table as table_range (table["global_seqno"], default 0, is
    added to every seqno); positions: the dict table_range(..., scan={"block_off": block_off})
    returned (outcome, status, first_block, first_item, last_block, last_item are read);
    block_off: the table's data-block offsets, int64 cuda [n_blocks + 1] (scan_table's,
    write_table's or table_block_offsets'); n_queries: default the positions' length.
    Returns the device lsm_items dict (keys, key_off, vals, val_off, seqno, vtype; padded arenas)
    that merge_runs takes, plus run_start (int64 [n + 1]: run q is the rows
    [run_start[q], run_start[q+1]), absolute), row_status (int32 [n]), end (int64 [3]: base plus
    this call's {rows, key bytes, value bytes}), need (int64 [4]: {pairs, rows, key bytes, value
    bytes}), result and plan_result (int32 [1]: LSM_OK / LSM_OVERFLOW of the rows call and of the
    plan).  base: device int64 [3] cursor the rows are appended at (None = zeros; needs `into`).
    caps = (pairs, rows, key bytes, value bytes[, items]), in need's order: the call's block_cap
    and row_cap and the outputs' capacities; no host synchronisation, nothing trimmed.  into: an
    items dict (as this call or materialize_items returned it) to append to in place; its
    capacities are its tensors' (the arenas' less LSM_INPUT_PADDING) unless caps narrows them.
    caps=None: a sizing plan with row_cap 0 and block_cap n_queries x n_blocks runs first and
    need is read back once, the only host synchronisation (above RANGE_ROWS_AUTO_PAIRS possible
    pairs the pair count is read back first, by itself); without `into` the outputs are
    allocated for need and trimmed to the rows.
    frames: table_frames' view of an LZ4 table (lsm_table_range_rows_plan_framed /
    lsm_table_range_rows_framed): block b is frame b, positions are table_range(..., frames=frames)'s;
    file and block_off are not read (block_off may be None)."""
    torch = _torch()
    dev = file.device
    n = int(positions["outcome"].numel()) if n_queries is None else int(n_queries)
    t = _table_struct(table, table.get("global_seqno", 0))
    ps = LsmRangePositions(*(_ptr(positions[f]) for f, _ in LsmRangePositions._fields_))
    if base is not None and into is None:
        raise LsmError("table_range_rows: a base needs `into` (the outputs it already fills)")
    st = _stream(stream)
    if frames is None:
        n_blocks = int(block_off.numel()) - 1
        plan_fn, rows_fn = "lsm_table_range_rows_plan", "lsm_table_range_rows"
        head = (_ptr(file), _file_len(table), C.byref(t), _ptr(block_off), n_blocks, C.byref(ps), n)  # both calls'
    else:
        n_blocks = int(frames["n_blocks"])
        view = _frames_struct(frames)
        plan_fn, rows_fn = "lsm_table_range_rows_plan_framed", "lsm_table_range_rows_framed"
        head = (C.byref(t), C.byref(view), C.byref(ps), n)
    run_start = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    row_status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    end = torch.zeros(3, dtype=torch.int64, device=dev)
    need = torch.zeros(4, dtype=torch.int64, device=dev)
    result = torch.zeros(1, dtype=torch.int32, device=dev)
    plan_result = torch.zeros(1, dtype=torch.int32, device=dev)

    def plan(block_cap, row_cap):
        ws = _workspace(lib().lsm_table_range_rows_workspace_size(n, block_cap, row_cap), dev, stream)
        _check(getattr(lib(), plan_fn)(*head, block_cap, row_cap, _ptr(base), _ptr(run_start), _ptr(end), _ptr(need),
                                       _ptr(row_status), _ptr(plan_result), _ptr(ws), ws.numel(), st), plan_fn)
        return ws

    trim = None
    explicit = caps is not None
    if caps is None:
        bound = n * n_blocks
        if bound > RANGE_ROWS_AUTO_PAIRS:
            plan(0, 0)
            bound = _read_back(need, stream)[0]
        plan(bound, 0)
        pairs, rows, key_bytes, val_bytes = _read_back(need, stream)
        caps = (pairs, rows, key_bytes, val_bytes)
        if into is None:
            trim = rows
    block_cap, row_cap = int(caps[0]), int(caps[1])
    if into is not None:
        dst = into
        item_cap = into["seqno"].numel()
        key_cap, val_cap = into["keys"].numel() - LSM_INPUT_PADDING, into["vals"].numel() - LSM_INPUT_PADDING
        if explicit:
            key_cap, val_cap = min(key_cap, int(caps[2])), min(val_cap, int(caps[3]))
            if len(caps) > 4:
                item_cap = min(item_cap, int(caps[4]))
    else:
        item_cap = int(caps[4]) if len(caps) > 4 else row_cap
        key_cap, val_cap = int(caps[2]), int(caps[3])
        dst = _mi_alloc(dev, item_cap, key_cap, val_cap)
    ws = plan(block_cap, row_cap)
    _check(getattr(lib(), rows_fn)(*head, block_cap, row_cap, _ptr(base), _ptr(end), _ptr(ws), ws.numel(),
                                   _ptr(dst["key_off"]), _ptr(dst["val_off"]), _ptr(dst["keys"]), key_cap,
                                   _ptr(dst["vals"]), val_cap, _ptr(dst["seqno"]), _ptr(dst["vtype"]), item_cap,
                                   _ptr(result), st), rows_fn)
    items = _items_view(dst, trim)
    items.update(run_start=run_start, row_status=row_status[:n], end=end, need=need, result=result,
                 plan_result=plan_result)
    return items


def seek(blocks, block_off, n_blocks, query_block, lo, lo_off, hi, hi_off, flags, stream=None):
    """Batched data_block::Iter::seek / seek_upper (+ exclusive) (data_block/iter.rs:37-176).
    All inputs cuda tensors: blocks uint8 (padded), block_off int64 [n_blocks+1], query_block
    int32 [n], lo / hi uint8 padded arenas with int64 [n+1] offsets, flags uint8 [n]
    (SEEK_* bits).  Returns dict first/end (int32: item range in block order), found
    (uint8: bit 0 lower, bit 1 upper seek's return value), status."""
    torch = _torch()
    n = int(query_block.numel())
    dev = blocks.device
    out = {"first": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
           "end": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
           "found": torch.empty(max(n, 1), dtype=torch.uint8, device=dev),
           "status": torch.empty(max(n, 1), dtype=torch.int32, device=dev)}
    _check(lib().lsm_seek_blocks(_ptr(blocks), _ptr(block_off), n_blocks, _ptr(query_block), _ptr(lo), _ptr(lo_off),
                                 _ptr(hi), _ptr(hi_off), _ptr(flags), n, _ptr(out["first"]), _ptr(out["end"]),
                                 _ptr(out["found"]), _ptr(out["status"]), _stream(stream)), "lsm_seek_blocks")
    return out


def xxh3_128_file(data, length=None, offset=0, stream=None):
    """Whole-file xxh3_128 (ChecksummedWriter digest) of data[offset .. offset+length)
    (uint8 cuda tensor, readable 16 B past the end) -> (low, high) as Python ints."""
    torch = _torch()
    length = data.numel() - offset if length is None else length
    ws = _workspace(max(lib().lsm_xxh3_128_file_workspace_size(length), 256), data.device, stream)
    out = torch.zeros(2, dtype=torch.int64, device=data.device)
    _check(lib().lsm_xxh3_128_file(C.c_void_p(data.data_ptr() + offset), length, _ptr(out), _ptr(ws), ws.numel(),
                                   _stream(stream)), "lsm_xxh3_128_file")
    lo, hi = (x & (2 ** 64 - 1) for x in _read_back(out, stream))
    return lo, hi


class ChecksummedWriter:
    """The running whole-file checksum of an SST writer (ChecksummedWriter,
    src/checksum.rs:59-96) with its state in device memory: write(data) feeds
    the next bytes (ChecksummedWriter::write, checksum.rs:92-95),
    checksum() is Xxh3Default::digest128 of everything written so far, as
    (low, high) Python ints (synchronises; the state is kept, writes may go on).
    Any split of the file into writes gives the one-shot xxh3_128.

    Every call runs on one stream, fixed at construction (`stream`, else the
    stream current then).  write() first makes that stream wait for the
    caller's current stream (where `data` was produced); checksum() waits for
    the digest on that stream before reading it back."""

    def __init__(self, device=None, stream=None):
        torch = _torch()
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.stream):
            self.state = torch.empty(lib().lsm_xxh3_128_stream_state_size(), dtype=torch.uint8, device=self.device)
            self._ws = torch.empty(0, dtype=torch.uint8, device=self.device)
        self.bytes_written = 0
        _check(lib().lsm_xxh3_128_stream_init(_ptr(self.state), _stream(self.stream)), "lsm_xxh3_128_stream_init")

    def write(self, data, length=None, offset=0):
        """Feed data[offset .. offset + length) (uint8 cuda tensor, readable 16 B past the end)."""
        torch = _torch()
        length = data.numel() - offset if length is None else length
        cur = torch.cuda.current_stream(self.device)
        if cur != self.stream:
            self.stream.wait_stream(cur)           # data may still be being written on the caller's stream
            data.record_stream(self.stream)        # and must outlive the update queued below
        need = lib().lsm_xxh3_128_stream_workspace_size(length)
        if self._ws.numel() < need:
            # (allocated and freed on self.stream: the caching allocator reuses the old
            # workspace only for work queued after the updates that read it)
            with torch.cuda.stream(self.stream):
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        _check(lib().lsm_xxh3_128_stream_update(_ptr(self.state), C.c_void_p(data.data_ptr() + offset), length,
                                                _ptr(self._ws), self._ws.numel(), _stream(self.stream)),
               "lsm_xxh3_128_stream_update")
        self.bytes_written += length
        return length

    def checksum(self):
        torch = _torch()
        with torch.cuda.stream(self.stream):
            out = torch.zeros(2, dtype=torch.int64, device=self.device)
        _check(lib().lsm_xxh3_128_stream_digest(_ptr(self.state), _ptr(out), _stream(self.stream)),
               "lsm_xxh3_128_stream_digest")
        lo, hi = (x & (2 ** 64 - 1) for x in _read_back(out, self.stream))
        return lo, hi


class ChecksummedWriterSet:
    """n running whole-file checksums advanced together: one ChecksummedWriter
    (src/checksum.rs:59-96) per table of a flush or compaction that rotates
    through several tables (MultiWriter, src/table/multi_writer.rs:181-257).
    write(data, off) feeds state i the bytes data[off[i] .. off[i+1]) for every
    i in one launch sequence (lsm_xxh3_128_stream_update_batch); checksums()
    returns every digest as (low, high) pairs.  Same stream rules as
    ChecksummedWriter."""

    def __init__(self, n, device=None, stream=None):
        torch = _torch()
        self.n = n
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        size = lib().lsm_xxh3_128_stream_state_size()
        with torch.cuda.stream(self.stream):
            self.states = torch.empty(max(n, 1) * size, dtype=torch.uint8, device=self.device)
            self.status = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
            self._ws = torch.empty(0, dtype=torch.uint8, device=self.device)
        _check(lib().lsm_xxh3_128_stream_init_batch(_ptr(self.states), n, _stream(self.stream)),
               "lsm_xxh3_128_stream_init_batch")

    def write(self, data, off, total_len=None):
        """data: uint8 cuda tensor (readable 16 B past each range); off: int64 cuda
        tensor [n+1]; total_len >= off[n] - off[0] (default: data.numel())."""
        torch = _torch()
        total_len = data.numel() if total_len is None else total_len
        cur = torch.cuda.current_stream(self.device)
        if cur != self.stream:
            self.stream.wait_stream(cur)
            data.record_stream(self.stream)
            off.record_stream(self.stream)
        need = lib().lsm_xxh3_128_stream_batch_workspace_size(self.n, total_len)
        if self._ws.numel() < need:
            with torch.cuda.stream(self.stream):
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        _check(lib().lsm_xxh3_128_stream_update_batch(_ptr(self.states), self.n, _ptr(data), _ptr(off), total_len,
                                                      _ptr(self.status), _ptr(self._ws), self._ws.numel(),
                                                      _stream(self.stream)), "lsm_xxh3_128_stream_update_batch")
        return self.status

    def checksums(self):
        torch = _torch()
        with torch.cuda.stream(self.stream):
            out = torch.zeros(2 * max(self.n, 1), dtype=torch.int64, device=self.device)
        _check(lib().lsm_xxh3_128_stream_digest_batch(_ptr(self.states), self.n, _ptr(out), _stream(self.stream)),
               "lsm_xxh3_128_stream_digest_batch")
        v = [x & (2 ** 64 - 1) for x in _read_back(out, self.stream)]
        return [(v[2 * i], v[2 * i + 1]) for i in range(self.n)]


BLOOM_BITS_PER_KEY, BLOOM_FP_RATE, BLOOM_BAD_FILTER = 0, 1, 0xFF


def bloom_shape(n, bpk=None, fpr=None):
    """BloomConstructionPolicy::{BitsPerKey, FalsePositiveRate}.init(n) -> (m, k)
    (src/table/filter/mod.rs:25-34).  Host-only."""
    m, k = C.c_uint64(), C.c_uint64()
    policy, value = (BLOOM_BITS_PER_KEY, bpk) if bpk is not None else (BLOOM_FP_RATE, fpr)
    _check(lib().lsm_bloom_shape(n, policy, value, C.byref(m), C.byref(k)), "lsm_bloom_shape")
    return m.value, k.value


def hash64_keys(keys, key_off, n=None, stream=None):
    """xxh3_64 of each key (FullFilterWriter::register_key, writer/filter/full.rs:47-50):
    keys = padded uint8 cuda tensor, key_off = int64 cuda tensor [n+1] -> int64 cuda [n]."""
    torch = _torch()
    n = key_off.numel() - 1 if n is None else n
    out = torch.empty(max(n, 1), dtype=torch.int64, device=keys.device)
    _check(lib().lsm_hash64_keys(_ptr(keys), _ptr(key_off), n, _ptr(out), _stream(stream)), "lsm_hash64_keys")
    return out[:n]


def bloom_build(hashes, m, k, stream=None):
    """Standard Bloom filter image (Builder::set_with_hash + build, standard_bloom/builder.rs)
    of int64 cuda hashes -> uint8 cuda tensor of lsm_bloom_filter_size(m) bytes."""
    torch = _torch()
    size = lib().lsm_bloom_filter_size(m)
    buf = torch.empty((size + 3) // 4 * 4, dtype=torch.uint8, device=hashes.device)
    _check(lib().lsm_bloom_build(_ptr(hashes), hashes.numel(), m, k, _ptr(buf), buf.numel(), _stream(stream)),
           "lsm_bloom_build")
    return buf[:size]


def bloom_contains(filt, hashes, stream=None):
    """contains_hash per hash (standard_bloom/mod.rs:100-120) -> uint8 cuda [n]: 1, 0 or BLOOM_BAD_FILTER."""
    torch = _torch()
    out = torch.empty(max(hashes.numel(), 1), dtype=torch.uint8, device=hashes.device)
    _check(lib().lsm_bloom_contains(_ptr(filt), filt.numel(), _ptr(hashes), hashes.numel(), _ptr(out),
                                    _stream(stream)), "lsm_bloom_contains")
    return out[:hashes.numel()]


# Default cap on a header's uncompressed_length (the plan sizes the output from
# verified headers only, but a crafted header per block could still ask for
# this much): the writer's largest data-block target is 4 MiB
# (writer/mod.rs:195-198) and a block overshoots its target by its last item
# (mod.rs:284-290), so 4 MiB + 64 KiB covers tables of items < 64 KiB; pass a
# larger max_block_bytes for tables with larger items.
LZ4_MAX_BLOCK = (4 << 20) + (64 << 10)


def lz4_decompress_blocks(blocks, block_off, n_blocks=None, max_block_bytes=LZ4_MAX_BLOCK, stream=None):
    """Block::from_reader with CompressionType::Lz4 over a batch (block/mod.rs:87-128):
    blocks = padded uint8 cuda tensor of on-disk blocks, block_off = int64 cuda [n+1].
    Output sizes come from lsm_lz4_plan_output: each VERIFIED header's
    uncompressed_length (a block whose header fails gets 0 bytes and reports the
    header error; one above max_block_bytes reports OVERFLOW).
    Returns (out uint8 cuda, out_off int64 cuda [n+1], status int32 cuda [n])."""
    torch = _torch()
    n = block_off.numel() - 1 if n_blocks is None else n_blocks
    dev = blocks.device
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        pws = _workspace(lib().lsm_lz4_plan_workspace_size(n), dev, stream)
        _check(lib().lsm_lz4_plan_output(_ptr(blocks), _ptr(block_off), n, max_block_bytes, _ptr(out_off), _ptr(pws),
                                         pws.numel(), _stream(stream)), "lsm_lz4_plan_output")
    total = _read_back(out_off[-1], stream) if n else 0
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    ws = _workspace(lib().lsm_lz4_workspace_size(n), dev, stream)
    _check(lib().lsm_lz4_decompress_blocks(_ptr(blocks), _ptr(block_off), n, _ptr(out), _ptr(out_off),
                                           _ptr(status), _ptr(ws), ws.numel(), _stream(stream)),
           "lsm_lz4_decompress_blocks")
    return out, out_off, status[:n]


def decode_lz4_blocks(blocks, block_off, n_blocks=None, expect_type=-1, item_cap=None, fields=None,
                      max_block_bytes=LZ4_MAX_BLOCK, stream=None, frames_cap=None):
    """LZ4 blocks end to end: Block::from_reader(Lz4) then DataBlock::new + iter
    (block/mod.rs:104-118, data_block/mod.rs:335,476).  lsm_lz4_plan_framed ->
    lsm_lz4_decompress_framed (frames = Header' || decompressed payload) ->
    lsm_decode_blocks_tuned(frames, LSM_DECODE_PAYLOAD_VERIFIED).  Returns the decode
    output dict (payload-relative offsets into each frame's payload) plus "frames",
    "frame_off" and "status" = the decompress status where it is not OK, else the
    decode status ("decode_status": the decode's own statuses: a block whose
    decompression failed has an all-zero frame header, so it is BAD_MAGIC there
    even without the merge).  frames_cap (bytes): size the frame arena without
    reading the plan back (no host sync; every block whose header verifies reports
    LSM_OVERFLOW when the frames do not fit, and item_cap defaults to frames_cap // 3)."""
    torch = _torch()
    n = block_off.numel() - 1 if n_blocks is None else n_blocks
    dev = blocks.device
    frame_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        pws = _workspace(lib().lsm_lz4_plan_workspace_size(n), dev, stream)
        if frames_cap is not None:
            _check(lib().lsm_lz4_plan_capped(_ptr(blocks), _ptr(block_off), n, max_block_bytes, 1, frames_cap,
                                             _ptr(frame_off), _ptr(pws), pws.numel(), _stream(stream)),
                   "lsm_lz4_plan_capped")
        else:
            _check(lib().lsm_lz4_plan_framed(_ptr(blocks), _ptr(block_off), n, max_block_bytes, _ptr(frame_off),
                                             _ptr(pws), pws.numel(), _stream(stream)), "lsm_lz4_plan_framed")
    if frames_cap is not None:
        total = frames_cap
    else:
        total = _read_back(frame_off[-1], stream) if n else 0
    frames = padded_bytes(total, dev)
    zst = _workspace(4 * max(n, 1), dev, stream).view(torch.int32)  # (the decompress statuses: not returned)
    ws = _workspace(lib().lsm_lz4_workspace_size(n), dev, stream)
    _check(lib().lsm_lz4_decompress_framed(_ptr(blocks), _ptr(block_off), n, _ptr(frames), _ptr(frame_off),
                                           _ptr(zst), _ptr(ws), ws.numel(), _stream(stream)),
           "lsm_lz4_decompress_framed")
    if item_cap is None:
        item_cap = total // 3 + 1
    d = Decoder(dev)
    out = d.alloc_outputs(item_cap, n, fields)
    d.decode(frames, frame_off, n, out, item_cap, expect_type,
             tuning=(0, 0, 0, DECODE_PAYLOAD_VERIFIED), stream=stream)
    with torch.cuda.stream(stream):  # (the merge of the statuses follows the decode on its stream)
        out["decode_status"] = out["status"].clone()  # (what a caller sees without the merge below)
        out["status"] = torch.where(zst[:max(n, 1)] != 0, zst[:max(n, 1)], out["status"])
    out["frames"], out["frame_off"] = frames, frame_off
    return out


def table_frames(file, table, block_off=None, max_block_bytes=LZ4_MAX_BLOCK, stream=None):
    """The view the framed readers take of an LZ4 table (lsm_table_frames): every data block of
    the table inflated once, a fully populated block cache of one table.  file / table as
    table_get; block_off: the data blocks' stored offsets, int64 cuda [n_blocks + 1] (write_table's
    block_off; default table_block_offsets(file, table)).  lsm_lz4_plan_framed and
    lsm_lz4_decompress_framed run over them; the plan's total is read back to size the arena (the
    one host synchronisation).  Returns dict(stored_off, frames (padded uint8), frame_off (int64
    [n_blocks + 1]), status (int32 [n_blocks], the decompress statuses), n_blocks, frames_len), what
    table_get / table_range / table_range_rows take as frames= and range_read as a table's
    "frames".  A table whose data blocks are not LZ4 yields non-OK statuses."""
    torch = _torch()
    if block_off is None:
        block_off = table_block_offsets(file, table)
    n = int(block_off.numel()) - 1
    dev = file.device
    frame_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        pws = _workspace(lib().lsm_lz4_plan_workspace_size(n), dev, stream)
        _check(lib().lsm_lz4_plan_framed(_ptr(file), _ptr(block_off), n, max_block_bytes, _ptr(frame_off), _ptr(pws),
                                         pws.numel(), _stream(stream)), "lsm_lz4_plan_framed")
    total = _read_back(frame_off[-1], stream) if n else 0
    frames = padded_bytes(total, dev)
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    ws = _workspace(lib().lsm_lz4_workspace_size(n), dev, stream)
    _check(lib().lsm_lz4_decompress_framed(_ptr(file), _ptr(block_off), n, _ptr(frames), _ptr(frame_off),
                                           _ptr(status), _ptr(ws), ws.numel(), _stream(stream)),
           "lsm_lz4_decompress_framed")
    return {"stored_off": block_off, "frames": frames, "frame_off": frame_off, "status": status[:n], "n_blocks": n,
            "frames_len": total}


def lz4_compress_blocks(blocks, block_off, n_blocks=None, in_status=None, out_cap=None, stream=None,
                        blocks_bytes=None):
    """Block::write_into with CompressionType::Lz4 over a batch (block/mod.rs:60-74):
    blocks = padded uint8 cuda tensor of uncompressed blocks as Encoder.encode wrote them,
    block_off = int64 cuda [n+1], in_status = the encoder's status (or None).  Each block
    becomes Header' || LZ4 stream of its payload, packed from offset 0.  out_cap defaults to
    lsm_lz4_compress_bound of the input buffer (of blocks_bytes, where the batch is a small
    part of `blocks`), which cannot overflow.  No host
    synchronisation.  Returns dict(buf: uint8 cuda, padded by LSM_INPUT_PADDING so it feeds
    decode_lz4_blocks; block_off: int64 cuda [n+1]; status: int32 cuda [n])."""
    torch = _torch()
    n = block_off.numel() - 1 if n_blocks is None else n_blocks
    dev = blocks.device
    if blocks_bytes is None:
        blocks_bytes = blocks.numel()  # (an upper bound of block_off[n] - block_off[0]: no read-back)
    if out_cap is None:
        out_cap = int(lib().lsm_lz4_compress_bound(blocks_bytes, n))
    buf = padded_bytes(out_cap, dev)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    ws = _workspace(lib().lsm_lz4_compress_workspace_size(n, blocks_bytes), dev, stream)
    _check(lib().lsm_lz4_compress_blocks(_ptr(blocks), _ptr(block_off), n, _ptr(in_status), _ptr(buf), out_cap,
                                         _ptr(out_off), _ptr(status), _ptr(ws), ws.numel(), _stream(stream)),
           "lsm_lz4_compress_blocks")
    return {"buf": buf, "block_off": out_off, "status": status[:n]}


def materialize_keys(blocks, block_off, n_blocks, out, n_items=None, stream=None, key_cap=None):
    """DataBlockParsedItem::materialize (data_block/mod.rs:296-315) of decode output `out`
    (dict from decode_blocks / scan_table) -> (keys uint8 cuda arena, key_off int64 cuda
    [n_items+1]); values stay (val_off, val_len) sub-slices of each payload.
    key_cap (bytes): no host sync (n_items defaults to the parsed arrays' capacity,
    lsm_materialize_keys_capped); returns (keys, key_off, result) with result a
    device int32 [1]: LSM_OK, or LSM_OVERFLOW when the keys exceed key_cap (none written)."""
    torch = _torch()
    dev = blocks.device
    if n_items is None:
        n_items = out["key_off"].numel() if key_cap is not None else _read_back(out["item_start"][n_blocks], stream)
    key_off = torch.zeros(n_items + 1, dtype=torch.int64, device=dev)
    ps = _parsed_struct(out)
    ws = _workspace(lib().lsm_materialize_workspace_size(n_items), dev, stream)
    args = (_ptr(blocks), _ptr(block_off), n_blocks, _ptr(out["item_start"]), _ptr(out["status"]), C.byref(ps), n_items)
    _check(lib().lsm_materialize_plan(*args, _ptr(key_off), _ptr(ws), ws.numel(), _stream(stream)),
           "lsm_materialize_plan")
    if key_cap is not None:
        keys = padded_bytes(key_cap, dev)
        result = torch.empty(1, dtype=torch.int32, device=dev)
        _check(lib().lsm_materialize_keys_capped(*args, _ptr(key_off), _ptr(keys), key_cap, _ptr(result),
                                                 _stream(stream)), "lsm_materialize_keys_capped")
        return keys, key_off, result
    total = _read_back(key_off[-1], stream) if n_items else 0
    keys = padded_bytes(total, dev)
    _check(lib().lsm_materialize_keys(*args, _ptr(key_off), _ptr(keys), _stream(stream)), "lsm_materialize_keys")
    return keys, key_off


def scan_table(file, file_len, tli_off, tli_size, two_level=False, global_seqno=0, block_count=0, cap_blocks=None,
               item_cap=None, fields=None, stream=None, sync=True, data_blocks_hint=0, index_blocks_hint=0):
    """Scanner over a table file image (scanner.rs:24-92): file = padded uint8 cuda tensor.
    Returns dict: table_status (int), n_blocks (int), block_off (int64 cuda [n+1]),
    the parsed fields, item_start and status (as decode_blocks).
    sync=False: lsm_scan_table_async (no host synchronisation): table_status and
    n_blocks are device int32 / uint32 tensors of one element, block_off holds
    cap_blocks + 1 entries (data_blocks_hint bounds the data decode, e.g. block_count;
    index_blocks_hint the partitions of a two-level index, e.g. tli_size // 4)."""
    torch = _torch()
    dev = file.device
    if cap_blocks is None:
        cap_blocks = max(1, file_len // 33)
    if item_cap is None:
        item_cap = file_len // 3 + 1
    out = Decoder(dev).alloc_outputs(item_cap, cap_blocks, fields)
    block_off = torch.zeros(cap_blocks + 1, dtype=torch.int64, device=dev)
    ws = _workspace(lib().lsm_scan_workspace_size(cap_blocks), dev, stream)
    ps = _parsed_struct(out)
    t = _table_struct({"tli_off": tli_off, "tli_size": tli_size, "two_level": two_level}, global_seqno, block_count)
    if not sync:
        d_nb = torch.zeros(1, dtype=torch.int32, device=dev)
        d_ts = torch.zeros(1, dtype=torch.int32, device=dev)
        _check(lib().lsm_scan_table_async(_ptr(file), file_len, C.byref(t), _ptr(block_off), cap_blocks,
                                          index_blocks_hint, data_blocks_hint, C.byref(ps), item_cap, _ptr(out["item_start"]),
                                          _ptr(out["status"]), _ptr(d_nb), _ptr(d_ts), _ptr(ws), ws.numel(),
                                          _stream(stream)), "lsm_scan_table_async")
        out["table_status"], out["n_blocks"], out["block_off"] = d_ts, d_nb, block_off
        return out
    nb, tst = C.c_uint32(), C.c_int32()
    _check(lib().lsm_scan_table(_ptr(file), file_len, C.byref(t), _ptr(block_off), cap_blocks, C.byref(ps), item_cap,
                                _ptr(out["item_start"]), _ptr(out["status"]), C.byref(nb), C.byref(tst), _ptr(ws),
                                ws.numel(), _stream(stream)), "lsm_scan_table")
    out["table_status"], out["n_blocks"] = int(tst.value), int(nb.value)
    out["block_off"] = block_off[:nb.value + 1]
    return out


def cut_blocks(key_off, val_off, block_size):
    """Host-side Writer chunking (numpy uint64 [n+1] arrays) -> numpy uint32 starts."""
    import numpy as np
    key_off = np.ascontiguousarray(key_off, np.uint64)
    val_off = np.ascontiguousarray(val_off, np.uint64)
    n = len(key_off) - 1
    starts = np.zeros(n + 2, np.uint32)
    nb = lib().lsm_cut_blocks(key_off.ctypes.data, val_off.ctypes.data, n, block_size, starts.ctypes.data, n + 1)
    return starts[:nb + 1].copy()


# Items per tile of lsm_cut_blocks_device (kCutTile, csrc/table_write.hip): tests size their inputs from it.
CUT_TILE_ITEMS = 16384


def cut_blocks_device(items_or_offsets, block_size, n_items=None, extra=0, stream=None):
    """lsm_cut_blocks_device: the writer's cut rule on device offsets.  items_or_offsets: a device
    lsm_items dict (key_off, val_off), or a (key_off, val_off) pair of int64 cuda tensors [cap + 1]
    (val_off None: the weight is the key length + extra, the index partitions' rule).
    n_items: None (every item of the arrays), an int, or a device int64 [1] count such as
    merge_runs' n_out (the arrays are then only the capacity).  Reads back one 16-byte record
    (block count and status) and returns the device int32 starts [n_blocks + 1]."""
    torch = _torch()
    if isinstance(items_or_offsets, dict):
        key_off, val_off = items_or_offsets["key_off"], items_or_offsets.get("val_off")
    else:
        key_off, val_off = items_or_offsets
    dev = key_off.device
    cap = key_off.numel() - 1
    d_n = None
    if hasattr(n_items, "data_ptr"):
        d_n = n_items
    elif n_items is not None:
        cap = int(n_items)
    starts = torch.empty(cap + 1, dtype=torch.int32, device=dev)
    res = torch.empty(2, dtype=torch.int64, device=dev)  # [n_blocks, status]
    ws = _workspace(lib().lsm_cut_workspace_size(cap), dev, stream)
    _check(lib().lsm_cut_blocks_device(_ptr(key_off), _ptr(val_off), cap, _ptr(d_n), extra, block_size,
                                       _ptr(starts), max(cap, 1), _ptr(res[0:]), _ptr(res[1:]), _ptr(ws),
                                       ws.numel(), _stream(stream)), "lsm_cut_blocks_device")
    nb, status = _read_back(res, stream)
    _check(status & 0xFFFFFFFF, "lsm_cut_blocks_device (device status)")
    return starts[:nb + 1]


def index_entries(items, starts, block_off, n_blocks, base_offset=0, key_cap=None, stream=None):
    """lsm_index_entries: the KeyedBlockHandles of an encoded batch as a device index-form lsm_items
    dict (keys, key_off, seqno, handle_off, handle_size) for Encoder.encode(block_type=BLOCK_INDEX),
    plus result (device int32 [1]: LSM_OK, or LSM_OVERFLOW when the keys exceed key_cap).  items:
    device dict (keys padded, key_off, seqno); starts / block_off as Encoder.encode took / returned
    them.  key_cap defaults to the items' key arena, which always suffices.  No host synchronisation."""
    torch = _torch()
    dev = items["keys"].device
    if key_cap is None:
        key_cap = items["keys"].numel()
    it, held = _items_struct(items, ("keys", "key_off", "seqno"))
    out = {"keys": torch.zeros(key_cap + LSM_INPUT_PADDING, dtype=torch.uint8, device=dev),
           "key_off": torch.empty(n_blocks + 1, dtype=torch.int64, device=dev),
           "seqno": torch.empty(n_blocks, dtype=torch.int64, device=dev),
           "handle_off": torch.empty(n_blocks, dtype=torch.int64, device=dev),
           "handle_size": torch.empty(n_blocks, dtype=torch.int32, device=dev),
           "result": torch.empty(1, dtype=torch.int32, device=dev)}
    ws = _workspace(lib().lsm_index_entries_workspace_size(n_blocks), dev, stream)
    _check(lib().lsm_index_entries(C.byref(it), _ptr(starts), _ptr(block_off), n_blocks, base_offset,
                                   _ptr(out["keys"]), key_cap, _ptr(out["key_off"]), _ptr(out["seqno"]),
                                   _ptr(out["handle_off"]), _ptr(out["handle_size"]), _ptr(out["result"]), _ptr(ws),
                                   ws.numel(), _stream(stream)), "lsm_index_entries")
    return out


def write_table(items, block_size=4096, restart_interval=16, hash_ratio=0.0, two_level=False, partition_size=4096,
                handle_overhead=48, n_items=None, compression=None):
    """The data and block-index regions of a table file, built on the device: what
    pyoracle.table_write builds on the host (Writer::write / spill_block, writer/mod.rs:243-343;
    FullIndexWriter::finish, writer/index/full.rs:55-69; PartitionedIndexWriter,
    writer/index/partitioned.rs:54-201).  items: device lsm_items dict (keys and vals padded);
    n_items: None, an int, or a device count such as merge_runs' n_out (the arrays are then the
    capacity; no offset array is downloaded).  handle_overhead stands for
    size_of::<KeyedBlockHandle>() in the partition cut (buffered size per handle = end key length
    + handle_overhead), which the reference does not pin; the scan does not depend on where
    partitions are cut.  Only scalars are read back: the block counts, the item count and the
    region ends.  The filter, meta, TOC and trailer regions are not written.
    compression: None, or "lz4" = the default data_block_compression_policy below level 0
    (config/mod.rs:275-283): the data blocks are encoded, then compressed
    (lz4_compress_blocks), and the index is built over the compressed offsets; the index
    partitions and the TLI stay uncompressed (index_block_compression_policy: None).
    Returns dict(file: uint8 cuda tensor (a view of a padded buffer), tli_off, tli_size,
    index_off, data_len, block_count, block_off (data blocks as stored, int64 cuda),
    starts (int32 cuda), compression)."""
    torch = _torch()
    if compression not in (None, "lz4"):
        raise LsmError(f"write_table: compression {compression!r} (None or \"lz4\")")
    dev = items["keys"].device
    starts = cut_blocks_device(items, block_size, n_items=n_items)
    nb = starts.numel() - 1
    if nb == 0:
        raise LsmError("write_table: no items")
    n = int(starts[nb].item())
    items = dict(items, key_off=items["key_off"][:n + 1], val_off=items["val_off"][:n + 1],
                 seqno=items["seqno"][:n], vtype=items["vtype"][:n])
    items.pop("handle_off", None)
    items.pop("handle_size", None)

    def encode(it, st, count, **kw):
        enc = Encoder(dev).encode(it, st, count, **kw)
        end = int(enc["block_off"][count].item())
        if not bool((enc["status"][:count] == 0).all().item()):
            raise LsmError("write_table: a block failed to encode")
        return enc, end

    def one_block(count):
        return torch.tensor([0, count], dtype=torch.int32, device=dev)

    data, data_len = encode(items, starts, nb, restart_interval=restart_interval, hash_ratio=hash_ratio)
    if compression == "lz4":
        data = lz4_compress_blocks(data["buf"], data["block_off"], nb, in_status=data["status"])
        data_len = int(data["block_off"][nb].item())
        if not bool((data["status"][:nb] == 0).all().item()):
            raise LsmError("write_table: a block failed to compress")
    handles = index_entries(items, starts, data["block_off"], nb)
    pieces = [data["buf"][:data_len]]
    index_off = data_len
    if two_level:
        pstarts = cut_blocks_device((handles["key_off"], None), partition_size, extra=handle_overhead)
        n_parts = pstarts.numel() - 1
        parts, region_len = encode(handles, pstarts, n_parts, block_type=BLOCK_INDEX)
        pieces.append(parts["buf"][:region_len])
        handles = index_entries(handles, pstarts, parts["block_off"], n_parts, base_offset=index_off)
        tli, tli_size = encode(handles, one_block(n_parts), 1, block_type=BLOCK_INDEX)
        tli_off = index_off + region_len
    else:
        tli, tli_size = encode(handles, one_block(nb), 1, block_type=BLOCK_INDEX)
        tli_off = index_off
    pieces.append(tli["buf"][:tli_size])
    total = tli_off + tli_size
    file = padded_bytes(total, dev)
    torch.cat(pieces, out=file[:total])
    return {"file": file[:total], "tli_off": tli_off, "tli_size": tli_size, "index_off": index_off,
            "data_len": data_len, "block_count": nb, "block_off": data["block_off"][:nb + 1], "starts": starts,
            "compression": compression}


def items_to_device(items_np, device="cuda", off32=False):
    """pyoracle.Items-like numpy SoA -> dict of padded cuda tensors for Encoder.encode
    (off32: int32 key / value offsets, encoded through lsm_encode_blocks32)."""
    import numpy as np
    torch = _torch()
    d = {"keys": to_device_bytes(items_np.keys, device), "vals": to_device_bytes(items_np.vals, device)}
    ot = np.int32 if off32 else np.int64
    if off32 and (int(items_np.key_off[-1]) >= 1 << 32 or int(items_np.val_off[-1]) >= 1 << 32):
        raise LsmError("off32: arenas of 4 GiB or more need the u64 offsets")
    d["key_off"] = torch.from_numpy(items_np.key_off.astype(np.uint32 if off32 else np.int64).view(ot)).to(device)
    d["val_off"] = torch.from_numpy(items_np.val_off.astype(np.uint32 if off32 else np.int64).view(ot)).to(device)
    d["seqno"] = torch.from_numpy(items_np.seqno.view(np.int64)).to(device)
    d["vtype"] = torch.from_numpy(items_np.vtype).to(device)
    d["handle_off"] = torch.from_numpy(items_np.handle_off.view(np.int64)).to(device)
    d["handle_size"] = torch.from_numpy(items_np.handle_size.view(np.int32)).to(device)
    return d


MERGE_MAX_RUNS, MERGE_EVICT_TOMBSTONES, MERGE_ZERO_SEQNOS = 64, 1, 2


def _run_start(items, run_start):
    """run_start as an int64 tensor on the items' device (a host sequence is uploaded)."""
    if hasattr(run_start, "data_ptr"):
        return run_start
    torch = _torch()
    return torch.tensor(list(run_start), dtype=torch.int64, device=items["keys"].device)


def _merge_io(items, tail, tail_len, n_status):
    """What lsm_merge_runs and lsm_merge_read share: (the input lsm_items, its stand-ins to keep
    alive, the output dict).  The outputs are sized for the input and listed in the order both
    calls take them: the items-shaped arrays, src, the int64 [tail_len] array named `tail`
    (n_out / group_start), status (int32 [n_status])."""
    torch = _torch()
    dev = items["keys"].device
    it, held = _items_struct(items)
    n = it.n_items
    out = {"keys": torch.empty(items["keys"].numel() + LSM_INPUT_PADDING, dtype=torch.uint8, device=dev),
           "key_off": torch.empty(n + 1, dtype=torch.int64, device=dev),
           "vals": torch.empty(items["vals"].numel() + LSM_INPUT_PADDING, dtype=torch.uint8, device=dev),
           "val_off": torch.empty(n + 1, dtype=torch.int64, device=dev),
           "seqno": torch.empty(max(n, 1), dtype=torch.int64, device=dev),
           "vtype": torch.empty(max(n, 1), dtype=torch.uint8, device=dev),
           "src": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
           tail: torch.empty(tail_len, dtype=torch.int64, device=dev),
           "status": torch.empty(max(n_status, 1), dtype=torch.int32, device=dev)}
    return it, held, out


def merge_runs(items, run_start, gc_seqno_threshold=0, evict_tombstones=False, zero_seqnos=False, stream=None):
    """CompactionStream::new(Merger::new(runs), gc_seqno_threshold).evict_tombstones(..).zero_seqnos(..)
    (merge.rs:34-100, compaction/stream.rs:46-221) on the device.  items: device dict as
    items_to_device returns it, every run back to back; run_start: int64 cuda [n_runs + 1] (or a
    host sequence).  Returns a device dict of the same keys (keys, key_off, vals, val_off, seqno,
    vtype, sized for the input: the first n_out items / n_out + 1 offsets are defined) plus
    src (int32: input index of each output item), n_out (int64 [1], on the device) and status
    (int32 [n_runs]).  No host synchronisation."""
    run_start = _run_start(items, run_start)
    n_runs = max(run_start.numel() - 1, 0)
    it, held, out = _merge_io(items, "n_out", 1, n_runs)
    ws = _workspace(lib().lsm_merge_workspace_size(it.n_items, n_runs), run_start.device, stream)
    flags = (MERGE_EVICT_TOMBSTONES if evict_tombstones else 0) | (MERGE_ZERO_SEQNOS if zero_seqnos else 0)
    _check(lib().lsm_merge_runs(C.byref(it), _ptr(run_start), n_runs, gc_seqno_threshold & (2 ** 64 - 1), flags,
                                *map(_ptr, out.values()), _ptr(ws), ws.numel(), _stream(stream)), "lsm_merge_runs")
    return out


MERGE_READ_KEEP_TOMBSTONES = 1


def merge_read(items, run_start, n_groups, n_sources, snapshot, group_seqno=None, in_status=None,
               keep_tombstones=False, stream=None):
    """The snapshot read of n_groups queries over n_sources sources each (TreeIter::create_range,
    range.rs:99-235: seqno_filter per source, Merger, MvccStream, the tombstone filter) on the
    device.  items: device lsm_items dict, every run back to back; run_start: int64 cuda
    [n_sources * n_groups + 1] (or a host sequence), run s * n_groups + g = source s of group g.
    snapshot: an item is visible iff seqno < snapshot; group_seqno (int64 cuda [n_groups]) gives
    every group its own.  in_status: int32 cuda [n_sources * n_groups], table_range_rows'
    row_status of every run.  keep_tombstones: the kept tombstones stay in the output.
    Returns merge_runs' dict with group_start (int64 [n_groups + 1]: group g's rows are
    [group_start[g], group_start[g + 1])) in place of n_out, and status of [n_groups].
    No host synchronisation."""
    run_start = _run_start(items, run_start)
    it, held, out = _merge_io(items, "group_start", n_groups + 1, n_groups)
    ws = _workspace(lib().lsm_merge_read_workspace_size(it.n_items, n_groups, n_sources), run_start.device, stream)
    flags = MERGE_READ_KEEP_TOMBSTONES if keep_tombstones else 0
    _check(lib().lsm_merge_read(C.byref(it), _ptr(run_start), n_groups, n_sources, snapshot & (2 ** 64 - 1),
                                _ptr(group_seqno), _ptr(in_status), flags, *map(_ptr, out.values()), _ptr(ws),
                                ws.numel(), _stream(stream)), "lsm_merge_read")
    out["status"] = out["status"][:n_groups]
    return out


def range_read(tables, lo, lo_off, hi, hi_off, flags, snapshot, group_seqno=None, keep_tombstones=False,
               stream=None):
    """Tree::range(range, seqno) for a batch of ranges over several tables on the device:
    table_range -> table_range_rows per table, each appended at the previous one's cursor, then
    merge_read with the tables as sources (tables[0] is the lowest source: of equal (key, seqno)
    its row comes first) and the rows calls' row_status as in_status.  tables: dicts as
    table_range takes them, with file (padded uint8 cuda tensor), block_off (int64 cuda
    [n_blocks + 1]) and optionally global_seqno: what write_table returns.  A table whose data
    blocks are LZ4 also carries frames (table_frames' view of it) and is read through the framed
    calls, so one read can mix LZ4 and plain tables.  lo / lo_off / hi /
    hi_off / flags: the bounds of the n ranges, as table_range.  Returns merge_read's dict
    (n_groups = n, n_sources = len(tables)) plus row_status (int32 [len(tables) * n]).
    One host synchronisation: the rows calls' sizes are read back to size the arenas."""
    torch = _torch()
    dev = flags.device
    n, n_src = int(flags.numel()), len(tables)
    positions, needs = [], []
    for t in tables:
        nb = int(t["block_off"].numel()) - 1
        start = t.get("starts")
        if start is None:  # (only table_range's row window reads it, which is not used here)
            start = torch.zeros(nb + 1, dtype=torch.int32, device=dev)
        pos = table_range(t["file"], t, lo, lo_off, hi, hi_off, flags,
                          scan={"block_off": t["block_off"], "n_blocks": nb, "item_start": start}, stream=stream,
                          frames=t.get("frames"))
        positions.append(pos)
        # a plan with no room for rows: its need sizes the real call (pairs beyond the cap: only need[0] counts)
        cap = min(n * nb, RANGE_ROWS_AUTO_PAIRS)
        needs.append((cap, table_range_rows(t["file"], t, pos, t["block_off"], caps=(cap, 0, 0, 0), stream=stream,
                                            n_queries=n, frames=t.get("frames"))["need"]))
    needs = [(cap, _read_back(need, stream)) for cap, need in needs]
    for s, (cap, need) in enumerate(needs):
        if need[0] > cap:
            t = tables[s]
            again = table_range_rows(t["file"], t, positions[s], t["block_off"], caps=(need[0], 0, 0, 0),
                                     stream=stream, n_queries=n, frames=t.get("frames"))["need"]
            needs[s] = (need[0], _read_back(again, stream))
    rows, key_bytes, val_bytes = (sum(need[k] for _, need in needs) for k in (1, 2, 3))
    dst = _mi_alloc(dev, rows, key_bytes, val_bytes)
    cursor, run_start, row_status = None, [], []
    for s, t in enumerate(tables):
        need = needs[s][1]
        res = table_range_rows(t["file"], t, positions[s], t["block_off"], base=cursor, into=dst,
                               caps=(need[0], need[1], key_bytes, val_bytes), stream=stream, n_queries=n,
                               frames=t.get("frames"))
        cursor = res["end"]
        run_start.append(res["run_start"][:n] if s + 1 < n_src else res["run_start"])
        row_status.append(res["row_status"])
    row_status = torch.cat(row_status)
    out = merge_read(_items_view(dst, rows), torch.cat(run_start), n, n_src, snapshot, group_seqno=group_seqno,
                     in_status=row_status, keep_tombstones=keep_tombstones, stream=stream)
    out["row_status"] = row_status
    return out


def _mi_args(blocks, block_off, n_blocks, out):
    """The leading arguments lsm_materialize_items_plan and lsm_materialize_items share (and the
    struct they point into, which the caller keeps alive)."""
    ps = _parsed_struct(out)
    d_nb = n_blocks if hasattr(n_blocks, "data_ptr") else None
    nb = out["item_start"].numel() - 1 if d_nb is not None else int(n_blocks)
    return (_ptr(blocks), _ptr(block_off), nb, _ptr(d_nb), _ptr(out["item_start"]), _ptr(out["status"]),
            C.byref(ps), out["key_off"].numel()), ps


def _mi_plan(args, base, dst, item_cap, end, result, stream):
    ws = _workspace(lib().lsm_materialize_items_workspace_size(args[7]), end.device, stream)
    _check(lib().lsm_materialize_items_plan(*args, _ptr(base), _ptr(dst["key_off"]), _ptr(dst["val_off"]), item_cap,
                                            _ptr(end), _ptr(result), _ptr(ws), ws.numel(), _stream(stream)),
           "lsm_materialize_items_plan")


def _mi_gather(args, base, end, dst, caps, result, stream):
    _check(lib().lsm_materialize_items(*args, _ptr(base), _ptr(end), _ptr(dst["key_off"]), _ptr(dst["val_off"]),
                                       _ptr(dst["keys"]), caps[1], _ptr(dst["vals"]), caps[2], _ptr(dst["seqno"]),
                                       _ptr(dst["vtype"]), caps[0], _ptr(result), _stream(stream)),
           "lsm_materialize_items")


def _mi_alloc(dev, item_cap, key_cap=None, val_cap=None):
    torch = _torch()
    d = {"key_off": torch.zeros(item_cap + 1, dtype=torch.int64, device=dev),
         "val_off": torch.zeros(item_cap + 1, dtype=torch.int64, device=dev),
         "seqno": torch.zeros(max(item_cap, 1), dtype=torch.int64, device=dev),
         "vtype": torch.zeros(max(item_cap, 1), dtype=torch.uint8, device=dev)}
    if key_cap is not None:
        d["keys"], d["vals"] = padded_bytes(key_cap, dev), padded_bytes(val_cap, dev)
    return d


def materialize_items(blocks, block_off, n_blocks, out, base=None, into=None, caps=None, stream=None, end=None):
    """lsm_materialize_items_plan + lsm_materialize_items: decode output `out` (dict from
    decode_blocks / decode_lz4_blocks / scan_table over `blocks`) -> the device lsm_items dict
    (keys, key_off, vals, val_off, seqno, vtype) that merge_runs and Encoder.encode take, plus
    end (device int64 [3]: base + this table's {rows, key bytes, value bytes}), result and
    plan_result (device int32 [1]: LSM_OK / LSM_OVERFLOW of the gather and of the plan).
    n_blocks: an int, or the device count scan_table(sync=False) leaves.  base: device int64 [3]
    cursor the rows are appended at (None = zeros); end: where to write the advanced cursor, e.g.
    the next row of a cursor array (None = a fresh tensor).
    Neither into nor caps: the arenas are sized from the plan (one read-back of `end`) and the
    returned tensors are trimmed to the rows.  caps = (items, key bytes, value bytes): outputs
    of that capacity, no host synchronisation, nothing trimmed.  into: an items dict (as this
    call returned it) to append to in place; its capacities are its tensors' (the arenas' less
    LSM_INPUT_PADDING) unless caps narrows them."""
    torch = _torch()
    dev = blocks.device
    args, ps = _mi_args(blocks, block_off, n_blocks, out)
    if end is None:
        end = torch.zeros(3, dtype=torch.int64, device=dev)
    result = torch.zeros(1, dtype=torch.int32, device=dev)
    plan_result = torch.zeros(1, dtype=torch.int32, device=dev)
    trim = None
    if into is not None:
        dst = into
        if caps is None:
            caps = (into["seqno"].numel(), into["keys"].numel() - LSM_INPUT_PADDING,
                    into["vals"].numel() - LSM_INPUT_PADDING)
        _mi_plan(args, base, dst, caps[0], end, plan_result, stream)
    elif caps is not None:
        dst = _mi_alloc(dev, *caps)
        _mi_plan(args, base, dst, caps[0], end, plan_result, stream)
    else:
        if base is not None:
            raise LsmError("materialize_items: a base needs `into` or `caps` (the outputs it already fills)")
        dst = _mi_alloc(dev, args[7])
        _mi_plan(args, None, dst, args[7], end, plan_result, stream)
        trim, key_cap, val_cap = _read_back(end, stream)
        dst["keys"], dst["vals"] = padded_bytes(key_cap, dev), padded_bytes(val_cap, dev)
        caps = (args[7], key_cap, val_cap)
    _mi_gather(args, base, end, dst, caps, result, stream)
    items = _items_view(dst, trim)
    items.update(end=end, result=result, plan_result=plan_result)
    return items


def tables_to_runs(tables, stream=None):
    """Several decoded tables -> one merge-ready lsm_items dict, run after run: tables is a list
    of (blocks, block_off, n_blocks, out) as materialize_items takes them.  The cursor
    (int64 [n_tables + 1][3]) is chained on the device: table t + 1 is appended where table t
    ended; only its last row (three scalars) is read back, to size the arenas and trim the
    views.  Returns (items, run_start): items also holds result (device int32 [n_tables], the
    gathers' LSM_OK / LSM_OVERFLOW); run_start is the device int64 [n_tables + 1] merge_runs takes."""
    torch = _torch()
    dev = tables[0][0].device
    nt = len(tables)
    cursor = torch.zeros((nt + 1, 3), dtype=torch.int64, device=dev)
    calls = [_mi_args(*t) for t in tables]
    item_cap = sum(a[7] for a, _ in calls)
    dst = _mi_alloc(dev, item_cap)
    plan_result = torch.zeros(nt, dtype=torch.int32, device=dev)
    result = torch.zeros(nt, dtype=torch.int32, device=dev)
    for t, (a, _) in enumerate(calls):
        _mi_plan(a, cursor[t], dst, item_cap, cursor[t + 1], plan_result[t:], stream)
    n, key_cap, val_cap = _read_back(cursor[nt], stream)
    dst["keys"], dst["vals"] = padded_bytes(key_cap, dev), padded_bytes(val_cap, dev)
    for t, (a, _) in enumerate(calls):
        _mi_gather(a, cursor[t], cursor[t + 1], dst, (item_cap, key_cap, val_cap), result[t:], stream)
    items = dict(_items_view(dst, n), result=result, plan_result=plan_result)
    return items, cursor[:, 0].contiguous()


def decoded_to_items(blocks, block_off, n_blocks, out, keys, key_off):
    """Decoder output -> encoder input: `out` from decode_blocks / scan_table over `blocks`
    (block_off int64 cuda [n_blocks + 1]) plus materialize_keys' (keys, key_off) -> the device
    lsm_items dict Encoder.encode and merge_runs take.  Keys as materialized; values gathered
    from block_off[b] + 33 + val_off, val_len into a packed, padded arena.  Torch ops only
    (an index tensor per value byte and a host read-back: kept as an independent check of
    materialize_items / tables_to_runs, the HIP path a pipeline uses)."""
    torch = _torch()
    dev = blocks.device
    n = key_off.numel() - 1
    starts = out["item_start"][:n_blocks + 1].to(torch.int64) & 0xFFFFFFFF
    counts = starts[1:] - starts[:-1]
    base = torch.repeat_interleave(block_off[:n_blocks].to(torch.int64) + LSM_HEADER_LEN, counts, output_size=n)
    vlen = out["val_len"][:n].to(torch.int64) & 0xFFFFFFFF
    vsrc = base + (out["val_off"][:n].to(torch.int64) & 0xFFFFFFFF)
    val_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(vlen, 0, out=val_off[1:])
    total = int(val_off[-1].item()) if n else 0
    vals = padded_bytes(total, dev)
    if total:
        item = torch.repeat_interleave(torch.arange(n, device=dev), vlen, output_size=total)
        pos = torch.arange(total, device=dev) - val_off[item]
        vals[:total] = blocks[vsrc[item] + pos]
    return {"keys": keys, "key_off": key_off, "vals": vals, "val_off": val_off,
            "seqno": out["seqno"][:n].contiguous(), "vtype": out["vtype"][:n].contiguous()}


def shard_blocks(block_off, world):
    """Split n blocks into `world` contiguous shards of about equal BYTES
    (blocks are independent, so shards need no exchange).
    block_off: host array-like of n+1 offsets.  Returns world+1 block indices
    b[0]=0 <= b[1] <= ... <= b[world]=n; rank r decodes blocks [b[r], b[r+1])."""
    import numpy as np
    off = np.asarray(block_off, dtype=np.uint64)
    n = len(off) - 1
    total = int(off[-1] - off[0])
    bounds = [0]
    for r in range(1, world):
        target = int(off[0]) + total * r // world
        b = int(np.searchsorted(off[:n], np.uint64(target), side="left"))
        bounds.append(max(bounds[-1], min(b, n)))
    bounds.append(n)
    return bounds


def shard_items(starts, key_off, val_off, world):
    """Encode-side split: `world` contiguous block ranges,
    cut only at block boundaries, of about equal key + value BYTES.
    starts: host [n_blocks+1] item starts; key_off / val_off: host [n_items+1].
    Returns world+1 block indices (as shard_blocks)."""
    import numpy as np
    st = np.asarray(starts, dtype=np.int64)
    w = np.asarray(key_off, dtype=np.uint64)[st] + np.asarray(val_off, dtype=np.uint64)[st]
    return shard_blocks(w, world)


def _dev_items(items, i0, i1, device):
    """Items [i0, i1) of a host SoA (pyoracle.Items layout) as rebased, padded device tensors."""
    import numpy as np
    torch = _torch()
    k0, k1 = int(items.key_off[i0]), int(items.key_off[i1])
    v0, v1 = int(items.val_off[i0]), int(items.val_off[i1])
    d = {"keys": to_device_bytes(items.keys[k0:k1], device), "vals": to_device_bytes(items.vals[v0:v1], device)}
    d["key_off"] = torch.from_numpy((items.key_off[i0:i1 + 1] - np.uint64(k0)).astype(np.int64)).to(device)
    d["val_off"] = torch.from_numpy((items.val_off[i0:i1 + 1] - np.uint64(v0)).astype(np.int64)).to(device)
    d["seqno"] = torch.from_numpy(np.ascontiguousarray(items.seqno[i0:i1]).view(np.int64)).to(device)
    d["vtype"] = torch.from_numpy(np.ascontiguousarray(items.vtype[i0:i1])).to(device)
    d["handle_off"] = torch.from_numpy(np.ascontiguousarray(items.handle_off[i0:i1]).view(np.int64)).to(device)
    d["handle_size"] = torch.from_numpy(np.ascontiguousarray(items.handle_size[i0:i1]).view(np.int32)).to(device)
    return d


def _pinned(arr):
    """A host numpy array copied into page-locked memory (torch tensor; the copy
    runs in numpy, which releases the GIL for it)."""
    import numpy as np
    torch = _torch()
    a = np.ascontiguousarray(arr)
    t = torch.empty(a.nbytes, dtype=torch.uint8, pin_memory=True)
    if a.nbytes:
        np.copyto(t.numpy(), a.view(np.uint8).reshape(-1))
    return t


def _run_shards(jobs, worker):
    """One host thread per shard (each drives its own device and stream; the
    library calls and torch copies release the GIL), with a barrier for the one
    exchange step.  worker(k, job, barrier) -> result; a failing shard aborts
    the barrier so no other shard waits forever, and its exception is raised."""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    if not jobs:
        return []
    barrier = threading.Barrier(len(jobs))

    def run(k):
        try:
            return worker(k, jobs[k], barrier)
        except BaseException:
            barrier.abort()
            raise
    with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        futs = [ex.submit(run, k) for k in range(len(jobs))]
        return [f.result() for f in futs]


def encode_sharded(items, starts, devices, restart_interval=16, hash_ratio=0.0, block_type=BLOCK_DATA):
    """Single-process multi-device encode:
    the blocks of a host write buffer (pyoracle.Items layout, starts [n+1]) are
    split into len(devices) contiguous shards at block cuts (shard_items).  One
    host thread per shard: it stages the shard's items in pinned memory, copies
    them to its device on its own stream, encodes there and reads back the
    shard's block offsets; the one exchange step is the exclusive scan of the
    shards' byte totals (a barrier across the threads), after which every
    thread copies its blocks asynchronously into its place in one pinned packed
    buffer.  Shards overlap end to end (no blocking copy serialises them).
    Returns (packed bytes, block_off [n+1], status [n]) as host numpy arrays,
    equal to a single-device encode."""
    import numpy as np
    torch = _torch()
    starts = np.asarray(starts, dtype=np.int64)
    n_blocks = len(starts) - 1
    bounds = shard_items(starts, items.key_off, items.val_off, len(devices))
    jobs = [(dev, bounds[r], bounds[r + 1]) for r, dev in enumerate(devices) if bounds[r + 1] > bounds[r]]
    totals = [0] * len(jobs)
    shared = {}

    def worker(k, job, barrier):
        dev, b0, b1 = job
        dev = torch.device("cuda", dev) if isinstance(dev, int) else torch.device(dev)
        torch.cuda.set_device(dev)
        i0, i1 = int(starts[b0]), int(starts[b1])
        k0, k1 = int(items.key_off[i0]), int(items.key_off[i1])
        v0, v1 = int(items.val_off[i0]), int(items.val_off[i1])
        host = {"keys": _pinned(items.keys[k0:k1]), "vals": _pinned(items.vals[v0:v1]),
                "key_off": _pinned((items.key_off[i0:i1 + 1] - np.uint64(k0)).astype(np.int64)),
                "val_off": _pinned((items.val_off[i0:i1 + 1] - np.uint64(v0)).astype(np.int64)),
                "seqno": _pinned(items.seqno[i0:i1]), "vtype": _pinned(items.vtype[i0:i1]),
                "starts": _pinned((starts[b0:b1 + 1] - i0).astype(np.int32))}
        if items.handle_off is not None:
            host["handle_off"] = _pinned(items.handle_off[i0:i1])
            host["handle_size"] = _pinned(items.handle_size[i0:i1])
        st = torch.cuda.Stream(dev)
        nb = b1 - b0
        with torch.cuda.stream(st):
            d = {}
            for name, dt in (("keys", torch.uint8), ("vals", torch.uint8), ("key_off", torch.int64),
                             ("val_off", torch.int64), ("seqno", torch.int64), ("vtype", torch.uint8),
                             ("handle_off", torch.int64), ("handle_size", torch.int32)):
                if name not in host:
                    continue
                h = host[name].view(dt)
                if name in ("keys", "vals"):
                    t = padded_bytes(h.numel(), dev)
                    t[:h.numel()].copy_(h, non_blocking=True)
                else:
                    t = torch.empty(h.numel(), dtype=dt, device=dev)
                    t.copy_(h, non_blocking=True)
                d[name] = t
            d_starts = torch.empty(nb + 1, dtype=torch.int32, device=dev)
            d_starts.copy_(host["starts"].view(torch.int32), non_blocking=True)
            enc = Encoder(dev).encode(d, d_starts, nb, restart_interval, hash_ratio, block_type, stream=st)
            off_h = torch.empty(nb + 1, dtype=torch.int64, pin_memory=True)
            st_h = torch.empty(nb, dtype=torch.int32, pin_memory=True)
            off_h.copy_(enc["block_off"][:nb + 1], non_blocking=True)
            st_h.copy_(enc["status"][:nb], non_blocking=True)
        st.synchronize()
        totals[k] = int(off_h[-1])
        barrier.wait()  # exchange: every shard's byte total is known
        if k == 0:
            shared["packed"] = torch.empty(sum(totals), dtype=torch.uint8, pin_memory=True)
        barrier.wait()
        base = sum(totals[:k])
        with torch.cuda.stream(st):
            if totals[k]:
                shared["packed"][base:base + totals[k]].copy_(enc["buf"][:totals[k]], non_blocking=True)
        st.synchronize()
        off = off_h.numpy().view(np.uint64)
        return off[1:] + np.uint64(base), st_h.numpy().copy()

    res = _run_shards(jobs, worker)
    packed = shared["packed"].numpy() if jobs else np.zeros(0, np.uint8)
    block_off = np.concatenate([np.zeros(1, np.uint64)] + [r[0] for r in res])
    status = np.concatenate([r[1] for r in res]) if res else np.zeros(0, np.int32)
    assert len(block_off) == n_blocks + 1
    return packed, block_off, status


def decode_sharded(blocks, block_off, devices, expect_type=-1, fields=None):
    """Single-process multi-device decode: the on-disk blocks
    of a host buffer (e.g. an mmap'd SST's data section; block_off [n+1]) are
    split into len(devices) byte-balanced contiguous shards (shard_blocks).  One
    host thread per shard stages its bytes in pinned memory, copies them to its
    device on its own stream and decodes there; after the exchange step (the
    exclusive scan of the shards' item totals, a barrier across the threads)
    each thread copies its rows asynchronously into one pinned gather buffer
    per field, item_start rebased.  Returns host numpy arrays: every requested
    field, item_start [n+1] and status [n]."""
    import numpy as np
    torch = _torch()
    boff = np.asarray(block_off, dtype=np.uint64)
    data = np.frombuffer(blocks, np.uint8) if isinstance(blocks, (bytes, bytearray, memoryview)) else \
        np.asarray(blocks, np.uint8)
    n_blocks = len(boff) - 1
    bounds = shard_blocks(boff, len(devices))
    fields = fields or [f for f, _ in PARSED_FIELDS]
    jobs = [(dev, bounds[r], bounds[r + 1]) for r, dev in enumerate(devices) if bounds[r + 1] > bounds[r]]
    counts = [0] * len(jobs)
    shared = {}

    def worker(k, job, barrier):
        dev, b0, b1 = job
        dev = torch.device("cuda", dev) if isinstance(dev, int) else torch.device(dev)
        torch.cuda.set_device(dev)
        o0, o1 = int(boff[b0]), int(boff[b1])
        nb = b1 - b0
        hb = _pinned(data[o0:o1])
        ho = _pinned((boff[b0:b1 + 1] - np.uint64(o0)).astype(np.int64))
        st = torch.cuda.Stream(dev)
        cap = (o1 - o0) // 3 + 1
        with torch.cuda.stream(st):
            d_blocks = padded_bytes(o1 - o0, dev)
            d_blocks[:o1 - o0].copy_(hb, non_blocking=True)
            d_off = torch.empty(nb + 1, dtype=torch.int64, device=dev)
            d_off.copy_(ho.view(torch.int64), non_blocking=True)
            dec = Decoder(dev)
            out = dec.alloc_outputs(cap, nb, fields)
            dec.decode(d_blocks, d_off, nb, out, cap, expect_type, stream=st)
            ist_h = torch.empty(nb + 1, dtype=torch.int32, pin_memory=True)
            st_h = torch.empty(nb, dtype=torch.int32, pin_memory=True)
            ist_h.copy_(out["item_start"][:nb + 1], non_blocking=True)
            st_h.copy_(out["status"][:nb], non_blocking=True)
        st.synchronize()
        ist = ist_h.numpy().view(np.uint32).astype(np.int64)
        counts[k] = int(ist[-1])
        barrier.wait()  # exchange: every shard's item total is known
        if k == 0:
            tot = sum(counts)
            shared.update({f: torch.empty(max(tot, 1), dtype=out[f].dtype, pin_memory=True) for f in fields})
        barrier.wait()
        base = sum(counts[:k])
        with torch.cuda.stream(st):
            if counts[k]:
                for f in fields:
                    shared[f][base:base + counts[k]].copy_(out[f][:counts[k]], non_blocking=True)
        st.synchronize()
        return ist[1:] + base, st_h.numpy().copy()

    res_sh = _run_shards(jobs, worker)
    total = sum(counts)
    res = {f: (shared[f][:total].numpy() if jobs else np.zeros(0)) for f in fields}
    res["item_start"] = np.concatenate([np.zeros(1, np.int64)] + [r[0] for r in res_sh])
    res["status"] = np.concatenate([r[1] for r in res_sh]) if res_sh else np.zeros(0, np.int32)
    assert len(res["item_start"]) == n_blocks + 1
    return res
