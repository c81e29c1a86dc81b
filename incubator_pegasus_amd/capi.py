"""ctypes binding for the rrdb engine C-ABI (include/rrdb_engine.h).

The same binding drives either backend .so:
  - incubator_pegasus_amd/csrc/librrdb_hip.so  (the product, MI355X/gfx950)
  - oracle/liboracle.so                        (CPU restatement; tests only)

Mirrors the reference's read-service request/response shapes
(reference src/server/pegasus_read_service.h:54-68, idl/rrdb.thrift:185-345).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional

# status codes (rocksdb::Status::Code, v8.5.3)
OK = 0
NOT_FOUND = 1
CORRUPTION = 2
INVALID_ARGUMENT = 4
INCOMPLETE = 7
TRY_AGAIN = 13  # a check_and_mutate / check_and_set whose check did not pass

# filter types (idl/rrdb.thrift:27-33)
FT_NO_FILTER = 0
FT_MATCH_ANYWHERE = 1
FT_MATCH_PREFIX = 2
FT_MATCH_POSTFIX = 3

KIND_PUT = 0
KIND_DELETE = 1

SCAN_COMPLETED = -1


class _CSlice(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_uint8)), ("len", C.c_uint64)]


class _Slice(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_uint8)), ("len", C.c_uint64)]


class _Result(C.Structure):
    _fields_ = [
        ("error", C.c_int32),
        ("count", C.c_uint64),
        ("context_id", C.c_int64),
        ("i64", C.c_int64),
        ("keys", C.POINTER(_Slice)),
        ("values", C.POINTER(_Slice)),
        ("expire_ts", C.POINTER(C.c_int32)),
        ("group_counts", C.POINTER(C.c_uint64)),
        ("group_errors", C.POINTER(C.c_int32)),
        ("dev_keys", C.c_void_p),
        ("dev_key_offs", C.c_void_p),
        ("dev_vals", C.c_void_p),
        ("dev_val_offs", C.c_void_p),
        ("_arena", C.c_void_p),
    ]


class _MultiGetRequest(C.Structure):
    _fields_ = [
        ("hash_key", _CSlice),
        ("start_sortkey", _CSlice),
        ("stop_sortkey", _CSlice),
        ("start_inclusive", C.c_uint8),
        ("stop_inclusive", C.c_uint8),
        ("max_kv_count", C.c_int32),
        ("max_kv_size", C.c_int32),
        ("no_value", C.c_uint8),
        ("reverse", C.c_uint8),
        ("sort_key_filter_type", C.c_int32),
        ("sort_key_filter_pattern", _CSlice),
        ("n_sort_keys", C.c_uint64),
        ("sort_keys", C.POINTER(C.c_uint8)),
        ("sort_key_offs", C.POINTER(C.c_uint64)),
        ("on_device_out", C.c_uint8),
    ]


class _ScanRequest(C.Structure):
    _fields_ = [
        ("start_key", _CSlice),
        ("stop_key", _CSlice),
        ("start_inclusive", C.c_uint8),
        ("stop_inclusive", C.c_uint8),
        ("batch_size", C.c_int32),
        ("no_value", C.c_uint8),
        ("hash_key_filter_type", C.c_int32),
        ("hash_key_filter_pattern", _CSlice),
        ("sort_key_filter_type", C.c_int32),
        ("sort_key_filter_pattern", _CSlice),
        ("full_scan", C.c_uint8),
        ("validate_partition_hash", C.c_uint8),
        ("return_expire_ts", C.c_uint8),
        ("only_return_count", C.c_uint8),
        ("on_device_out", C.c_uint8),
    ]


class _CompactOptions(C.Structure):
    _fields_ = [("target_level", C.c_int32), ("bottommost_force", C.c_uint8),
                ("keep_inputs", C.c_uint8)]


class _CompactStats(C.Structure):
    _fields_ = [
        ("input_records", C.c_uint64),
        ("output_records", C.c_uint64),
        ("expired", C.c_uint64),
        ("filtered", C.c_uint64),
        ("tombstones", C.c_uint64),
        ("shadowed", C.c_uint64),
        ("output_bytes", C.c_uint64),
    ]


class _SplitStats(C.Structure):
    _fields_ = [
        ("input_records", C.c_uint64),
        ("parent_records", C.c_uint64),
        ("child_records", C.c_uint64),
        ("dropped_records", C.c_uint64),
        ("parent_bytes", C.c_uint64),
        ("child_bytes", C.c_uint64),
        ("runs_in", C.c_uint64),
        ("parent_runs", C.c_uint64),
        ("child_runs", C.c_uint64),
        ("parent_unpruned_runs", C.c_uint64),
    ]


class _WriteBatchStats(C.Structure):
    _fields_ = [
        ("input_ops", C.c_uint64),
        ("output_records", C.c_uint64),
        ("superseded", C.c_uint64),
        ("puts", C.c_uint64),
        ("removes", C.c_uint64),
        ("key_bytes", C.c_uint64),
        ("value_bytes", C.c_uint64),
    ]


class _IncrBatchStats(C.Structure):
    _fields_ = [
        ("input_ops", C.c_uint64),
        ("applied", C.c_uint64),
        ("failed_parse", C.c_uint64),
        ("failed_range", C.c_uint64),
        ("output_records", C.c_uint64),
        ("key_bytes", C.c_uint64),
        ("value_bytes", C.c_uint64),
    ]


class _TimetagBatchStats(C.Structure):
    _fields_ = [
        ("input_ops", C.c_uint64),
        ("applied", C.c_uint64),
        ("ignored", C.c_uint64),
        ("output_records", C.c_uint64),
        ("superseded", C.c_uint64),
        ("puts", C.c_uint64),
        ("removes", C.c_uint64),
        ("key_bytes", C.c_uint64),
        ("value_bytes", C.c_uint64),
    ]


class _CasBatchStats(C.Structure):
    _fields_ = [
        ("input_ops", C.c_uint64),
        ("passed", C.c_uint64),
        ("failed_check", C.c_uint64),
        ("failed_invalid", C.c_uint64),
        ("malformed", C.c_uint64),
        ("mutations_applied", C.c_uint64),
        ("output_records", C.c_uint64),
        ("puts", C.c_uint64),
        ("removes", C.c_uint64),
        ("key_bytes", C.c_uint64),
        ("value_bytes", C.c_uint64),
    ]


class _CompactRoute(C.Structure):
    _fields_ = [("rank", C.c_int32), ("emit", C.c_int32)]


# rrdb_compact_route values (include/rrdb_engine_ext.h)
ROUTE_NONE = -1
ROUTE_RANK_GLOBAL, ROUTE_RANK_LDS, ROUTE_RANK_LDST, ROUTE_RANK_GRP = 0, 1, 3, 4
ROUTE_EMIT_RANK, ROUTE_EMIT_INPUT, ROUTE_EMIT_CHUNKED, ROUTE_EMIT_CHUNKED_FIXED = 0, 1, 2, 3


class _MultiGetLane(C.Structure):
    _fields_ = [("lane", C.c_int32), ("fused_first", C.c_int32), ("tail_read", C.c_int32),
                ("batch_device_out", C.c_int32), ("batch_fused", C.c_uint64),
                ("batch_fallback", C.c_uint64)]


# rrdb_multi_get_lane values (include/rrdb_engine_ext.h)
MG_LANE_NONE, MG_LANE_POINT_LIST, MG_LANE_SERVER, MG_LANE_GRAPH, MG_LANE_SMALL, \
    MG_LANE_GENERAL = 0, 1, 2, 3, 4, 5


@dataclass
class MultiGetLane:
    lane: int = 0
    fused_first: int = 0
    tail_read: int = 0
    batch_device_out: int = 0
    batch_fused: int = 0
    batch_fallback: int = 0


class _ViewRoute(C.Structure):
    _fields_ = [("rank", C.c_int32), ("bound_levels", C.c_int32), ("n_groups", C.c_uint64),
                ("window_records", C.c_uint64), ("visible", C.c_uint64)]


@dataclass
class ViewRoute:
    rank: int = ROUTE_NONE
    bound_levels: int = 0
    n_groups: int = 0
    window_records: int = 0
    visible: int = 0


@dataclass
class IncrBatchStats:
    input_ops: int = 0
    applied: int = 0
    failed_parse: int = 0
    failed_range: int = 0
    output_records: int = 0
    key_bytes: int = 0
    value_bytes: int = 0


@dataclass
class TimetagBatchStats:
    input_ops: int = 0
    applied: int = 0
    ignored: int = 0
    output_records: int = 0
    superseded: int = 0
    puts: int = 0
    removes: int = 0
    key_bytes: int = 0
    value_bytes: int = 0


@dataclass
class CasBatchStats:
    input_ops: int = 0
    passed: int = 0
    failed_check: int = 0
    failed_invalid: int = 0
    malformed: int = 0
    mutations_applied: int = 0
    output_records: int = 0
    puts: int = 0
    removes: int = 0
    key_bytes: int = 0
    value_bytes: int = 0


# cas_check_type (idl/rrdb.thrift), the check_type of a check_and_mutate op
CT_NO_CHECK, CT_VALUE_NOT_EXIST, CT_VALUE_NOT_EXIST_OR_EMPTY, CT_VALUE_EXIST, \
    CT_VALUE_NOT_EMPTY = 0, 1, 2, 3, 4
CT_VALUE_MATCH_ANYWHERE, CT_VALUE_MATCH_PREFIX, CT_VALUE_MATCH_POSTFIX = 5, 6, 7
CT_VALUE_BYTES_LESS, CT_VALUE_BYTES_LESS_OR_EQUAL, CT_VALUE_BYTES_EQUAL, \
    CT_VALUE_BYTES_GREATER_OR_EQUAL, CT_VALUE_BYTES_GREATER = 8, 9, 10, 11, 12
CT_VALUE_INT_LESS, CT_VALUE_INT_LESS_OR_EQUAL, CT_VALUE_INT_EQUAL, \
    CT_VALUE_INT_GREATER_OR_EQUAL, CT_VALUE_INT_GREATER = 13, 14, 15, 16, 17


def _cslice(b: bytes, keep: list) -> _CSlice:
    """Build a _CSlice over a copy of b; the backing buffer is appended to
    `keep`, which the caller must hold alive across the C call (struct field
    assignment copies the slice by value, so the slice itself cannot own the
    buffer)."""
    if not b:
        return _CSlice(None, 0)
    buf = (C.c_uint8 * len(b)).from_buffer_copy(b)
    keep.append(buf)
    return _CSlice(C.cast(buf, C.POINTER(C.c_uint8)), len(b))


def _read_slice(s: _Slice) -> bytes:
    if s.len == 0:
        return b""
    return C.string_at(s.data, s.len)


@dataclass
class ScanResult:
    error: int
    context_id: int
    kvs: list  # [(key, value)]
    kv_count: Optional[int] = None  # only_return_count
    expire_ts: Optional[list] = None
    dev: Optional[dict] = None  # device-resident output descriptors


@dataclass
class CompactStats:
    input_records: int = 0
    output_records: int = 0
    expired: int = 0
    filtered: int = 0
    tombstones: int = 0
    shadowed: int = 0
    output_bytes: int = 0


@dataclass
class SplitStats:
    input_records: int = 0
    parent_records: int = 0
    child_records: int = 0
    dropped_records: int = 0
    parent_bytes: int = 0
    child_bytes: int = 0
    runs_in: int = 0
    parent_runs: int = 0
    child_runs: int = 0
    parent_unpruned_runs: int = 0


@dataclass
class WriteBatchStats:
    input_ops: int = 0
    output_records: int = 0
    superseded: int = 0
    puts: int = 0
    removes: int = 0
    key_bytes: int = 0
    value_bytes: int = 0


class RrdbLib:
    """One loaded engine .so."""

    def __init__(self, so_path: str):
        self.path = os.path.abspath(so_path)
        self._lib = C.CDLL(self.path)
        L = self._lib
        L.rrdb_open.restype = C.c_void_p
        L.rrdb_open.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        L.rrdb_close.argtypes = [C.c_void_p]
        L.rrdb_backend.restype = C.c_char_p
        L.rrdb_set_envs.restype = C.c_int32
        L.rrdb_set_envs.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int32]
        L.rrdb_set_partition_version.restype = C.c_int32
        L.rrdb_set_partition_version.argtypes = [C.c_void_p, C.c_int32]
        L.rrdb_ingest_run.restype = C.c_int32
        L.rrdb_ingest_run.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.rrdb_get.restype = C.c_int32
        L.rrdb_get.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(_Result)]
        L.rrdb_ttl.restype = C.c_int32
        L.rrdb_ttl.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(_Result)]
        L.rrdb_sortkey_count.restype = C.c_int32
        L.rrdb_sortkey_count.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(_Result)]
        L.rrdb_batch_get.restype = C.c_int32
        L.rrdb_batch_get.argtypes = [
            C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(_Result)]
        L.rrdb_multi_get.restype = C.c_int32
        L.rrdb_multi_get.argtypes = [C.c_void_p, C.POINTER(_MultiGetRequest), C.c_uint32, C.POINTER(_Result)]
        L.rrdb_scan_open.restype = C.c_int32
        L.rrdb_scan_open.argtypes = [C.c_void_p, C.POINTER(_ScanRequest), C.c_uint32, C.POINTER(_Result)]
        L.rrdb_scan_count_begin.restype = C.c_int32
        L.rrdb_scan_count_begin.argtypes = [C.c_void_p, C.POINTER(_ScanRequest), C.c_uint32]
        L.rrdb_scan_count_finish.restype = C.c_int32
        L.rrdb_scan_count_finish.argtypes = [C.c_void_p, C.POINTER(_Result)]
        L.rrdb_scan_next.restype = C.c_int32
        L.rrdb_scan_next.argtypes = [C.c_void_p, C.c_int64, C.c_uint32, C.POINTER(_Result)]
        L.rrdb_clear_scanner.argtypes = [C.c_void_p, C.c_int64]
        L.rrdb_manual_compact.restype = C.c_int32
        L.rrdb_manual_compact.argtypes = [
            C.c_void_p, C.POINTER(_CompactOptions), C.c_uint32, C.POINTER(_CompactStats)]
        L.rrdb_manual_compact_begin.restype = C.c_int32
        L.rrdb_manual_compact_begin.argtypes = [
            C.c_void_p, C.POINTER(_CompactOptions), C.c_uint32]
        L.rrdb_manual_compact_finish.restype = C.c_int32
        L.rrdb_manual_compact_finish.argtypes = [C.c_void_p, C.POINTER(_CompactStats)]
        L.rrdb_phase_ms.restype = C.c_double
        L.rrdb_phase_ms.argtypes = [C.c_void_p, C.c_char_p]
        L.rrdb_put.restype = C.c_int32
        L.rrdb_put.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64,
                               C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32]
        L.rrdb_remove.restype = C.c_int32
        L.rrdb_remove.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
        L.rrdb_flush.restype = C.c_int32
        L.rrdb_flush.argtypes = [C.c_void_p]
        L.rrdb_memtable_entries.restype = C.c_uint64
        L.rrdb_memtable_entries.argtypes = [C.c_void_p]
        L.rrdb_checkpoint.restype = C.c_int32
        L.rrdb_checkpoint.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
        L.rrdb_restore.restype = C.c_int32
        L.rrdb_restore.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
        L.rrdb_multi_get_batch.restype = C.c_int32
        L.rrdb_multi_get_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                           C.POINTER(_MultiGetRequest), C.c_uint32,
                                           C.POINTER(_Result)]
        L.rrdb_num_runs.restype = C.c_uint64
        L.rrdb_num_runs.argtypes = [C.c_void_p]
        L.rrdb_num_records.restype = C.c_uint64
        L.rrdb_num_records.argtypes = [C.c_void_p]
        L.rrdb_free_result.argtypes = [C.POINTER(_Result)]
        # engine-only extensions (include/rrdb_engine_ext.h): bound only when
        # the loaded library exports them (the CPU oracle does not)
        self.has_window_compact = all(
            hasattr(L, n) for n in ("rrdb_compact_runs", "rrdb_auto_compact"))
        if self.has_window_compact:
            L.rrdb_compact_runs.restype = C.c_int32
            L.rrdb_compact_runs.argtypes = [
                C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(_CompactStats)]
            L.rrdb_auto_compact.restype = C.c_int32
            L.rrdb_auto_compact.argtypes = [
                C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                C.POINTER(_CompactStats)]
        self.has_split = hasattr(L, "rrdb_split")
        if self.has_split:
            L.rrdb_split.restype = C.c_int32
            L.rrdb_split.argtypes = [
                C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(_SplitStats)]
        self.has_write_batch = hasattr(L, "rrdb_write_batch")
        if self.has_write_batch:
            L.rrdb_write_batch.restype = C.c_int32
            L.rrdb_write_batch.argtypes = [
                C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(_WriteBatchStats)]
        self.has_incr_batch = hasattr(L, "rrdb_incr_batch")
        if self.has_incr_batch:
            L.rrdb_incr_batch.restype = C.c_int32
            L.rrdb_incr_batch.argtypes = [
                C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(_IncrBatchStats)]
        self.has_write_batch_timetag = hasattr(L, "rrdb_write_batch_timetag")
        if self.has_write_batch_timetag:
            L.rrdb_write_batch_timetag.restype = C.c_int32
            L.rrdb_write_batch_timetag.argtypes = (
                [C.c_void_p, C.c_uint64] + [C.c_void_p] * 8 +
                [C.c_uint32, C.c_void_p, C.POINTER(_TimetagBatchStats)])
        self.has_check_and_mutate_batch = hasattr(L, "rrdb_check_and_mutate_batch")
        if self.has_check_and_mutate_batch:
            L.rrdb_check_and_mutate_batch.restype = C.c_int32
            L.rrdb_check_and_mutate_batch.argtypes = (
                [C.c_void_p, C.c_uint64] + [C.c_void_p] * 13 +
                [C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(_Result),
                 C.POINTER(_CasBatchStats)])
        self.has_compact_route = hasattr(L, "rrdb_last_compact_route")
        if self.has_compact_route:
            L.rrdb_last_compact_route.restype = C.c_int32
            L.rrdb_last_compact_route.argtypes = [C.c_void_p, C.POINTER(_CompactRoute)]
        self.has_multi_get_lane = hasattr(L, "rrdb_last_multi_get_lane")
        if self.has_multi_get_lane:
            L.rrdb_last_multi_get_lane.restype = C.c_int32
            L.rrdb_last_multi_get_lane.argtypes = [C.c_void_p, C.POINTER(_MultiGetLane)]
        self.has_view_route = hasattr(L, "rrdb_last_view_route")
        if self.has_view_route:
            L.rrdb_last_view_route.restype = C.c_int32
            L.rrdb_last_view_route.argtypes = [C.c_void_p, C.POINTER(_ViewRoute)]

    @property
    def backend(self) -> str:
        return self._lib.rrdb_backend().decode()

    def open(self, app_id: int, pidx: int, gpu_id: int) -> "RrdbPartition":
        h = self._lib.rrdb_open(app_id, pidx, gpu_id)
        if not h:
            raise RuntimeError(f"rrdb_open failed (backend={self.backend}, gpu_id={gpu_id})")
        return RrdbPartition(self, h)


def _pack(items):
    """list[bytes] -> (packed buffer, offsets u64 array)"""
    import numpy as np

    offs = np.zeros(len(items) + 1, dtype=np.uint64)
    total = 0
    for i, b in enumerate(items):
        total += len(b)
        offs[i + 1] = total
    buf = b"".join(items)
    return np.frombuffer(bytearray(buf), dtype=np.uint8), offs


class RrdbPartition:
    def __init__(self, lib: RrdbLib, handle):
        self.lib = lib
        self._L = lib._lib
        self._h = handle

    def close(self):
        if self._h:
            self._L.rrdb_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_envs(self, envs: dict):
        n = len(envs)
        keys = (C.c_char_p * n)(*[k.encode() for k in envs])
        vals = (C.c_char_p * n)(*[str(v).encode() for v in envs.values()])
        return self._L.rrdb_set_envs(self._h, keys, vals, n)

    def set_partition_version(self, pv: int):
        return self._L.rrdb_set_partition_version(self._h, pv)

    def ingest_run_arrays(self, keys_u8, key_offs_u64, vals_u8, val_offs_u64, seq_kind_u64):
        """Ingest from packed numpy arrays (zero python-loop path for bench)."""
        import numpy as np

        for a, dt in ((keys_u8, np.uint8), (key_offs_u64, np.uint64), (vals_u8, np.uint8),
                      (val_offs_u64, np.uint64), (seq_kind_u64, np.uint64)):
            assert a.dtype == dt and a.flags["C_CONTIGUOUS"], (a.dtype, dt)
        n = len(seq_kind_u64)
        st = self._L.rrdb_ingest_run(
            self._h,
            keys_u8.ctypes.data_as(C.c_void_p),
            key_offs_u64.ctypes.data_as(C.c_void_p),
            vals_u8.ctypes.data_as(C.c_void_p),
            val_offs_u64.ctypes.data_as(C.c_void_p),
            seq_kind_u64.ctypes.data_as(C.c_void_p),
            n,
        )
        if st != OK:
            raise RuntimeError(f"rrdb_ingest_run failed: status {st}")
        return st

    def ingest_run(self, records):
        """records: list of (raw_key: bytes, raw_value: bytes, seqno: int, kind: int),
        already sorted by raw_key ascending."""
        keys, koffs = _pack([r[0] for r in records])
        vals, voffs = _pack([r[1] for r in records])
        import numpy as np

        sk = np.array([(r[2] << 1) | r[3] for r in records], dtype=np.uint64)
        return self.ingest_run_arrays(keys, koffs, vals, voffs, sk)

    def num_runs(self):
        return self._L.rrdb_num_runs(self._h)

    def num_records(self):
        return self._L.rrdb_num_records(self._h)

    def _call_result(self, fn, *args):
        res = _Result()
        fn(self._h, *args, C.byref(res))
        return res

    def get(self, raw_key: bytes, epoch_now: int):
        res = self._call_result(self._L.rrdb_get, raw_key, len(raw_key), epoch_now)
        try:
            if res.error != OK:
                return res.error, None
            return OK, _read_slice(res.values[0])
        finally:
            self._L.rrdb_free_result(C.byref(res))

    def ttl(self, raw_key: bytes, epoch_now: int):
        res = self._call_result(self._L.rrdb_ttl, raw_key, len(raw_key), epoch_now)
        try:
            return res.error, (res.i64 if res.error == OK else None)
        finally:
            self._L.rrdb_free_result(C.byref(res))

    def sortkey_count(self, hash_key: bytes, epoch_now: int):
        res = self._call_result(self._L.rrdb_sortkey_count, hash_key, len(hash_key), epoch_now)
        try:
            return res.error, res.i64
        finally:
            self._L.rrdb_free_result(C.byref(res))

    def batch_get(self, raw_keys, epoch_now: int):
        keys, offs = _pack(raw_keys)
        res = _Result()
        self._L.rrdb_batch_get(
            self._h, len(raw_keys), keys.ctypes.data_as(C.c_void_p),
            offs.ctypes.data_as(C.c_void_p), epoch_now, C.byref(res))
        try:
            kvs = [(_read_slice(res.keys[i]), _read_slice(res.values[i]))
                   for i in range(res.count)]
            return res.error, kvs
        finally:
            self._L.rrdb_free_result(C.byref(res))

    def multi_get(self, hash_key: bytes, epoch_now: int, *, start_sortkey=b"", stop_sortkey=b"",
                  start_inclusive=True, stop_inclusive=False, max_kv_count=-1, max_kv_size=-1,
                  no_value=False, reverse=False, sort_key_filter_type=FT_NO_FILTER,
                  sort_key_filter_pattern=b"", sort_keys=None):
        keep = []
        req = _MultiGetRequest()
        req.hash_key = _cslice(hash_key, keep)
        req.start_sortkey = _cslice(start_sortkey, keep)
        req.stop_sortkey = _cslice(stop_sortkey, keep)
        req.start_inclusive = 1 if start_inclusive else 0
        req.stop_inclusive = 1 if stop_inclusive else 0
        req.max_kv_count = max_kv_count
        req.max_kv_size = max_kv_size
        req.no_value = 1 if no_value else 0
        req.reverse = 1 if reverse else 0
        req.sort_key_filter_type = sort_key_filter_type
        req.sort_key_filter_pattern = _cslice(sort_key_filter_pattern, keep)
        if sort_keys:
            sk, offs = _pack(sort_keys)
            req.n_sort_keys = len(sort_keys)
            req.sort_keys = sk.ctypes.data_as(C.POINTER(C.c_uint8))
            req.sort_key_offs = offs.ctypes.data_as(C.POINTER(C.c_uint64))
            keep += [sk, offs]
        res = _Result()
        self._L.rrdb_multi_get(self._h, C.byref(req), epoch_now, C.byref(res))
        del keep
        try:
            kvs = [(_read_slice(res.keys[i]), _read_slice(res.values[i]))
                   for i in range(res.count)]
            return res.error, kvs
        finally:
            self._L.rrdb_free_result(C.byref(res))

    def multi_get_batch(self, hash_keys, epoch_now: int, **shared_kwargs):
        """N full-range (or shared-shape) multi_gets in one call; returns
        (error, [per-request (error, [(sortkey, value), ...])])."""
        keep = []
        req = _MultiGetRequest()
        req.hash_key = _CSlice(None, 0)
        req.start_sortkey = _cslice(shared_kwargs.get("start_sortkey", b""), keep)
        req.stop_sortkey = _cslice(shared_kwargs.get("stop_sortkey", b""), keep)
        req.start_inclusive = 1 if shared_kwargs.get("start_inclusive", True) else 0
        req.stop_inclusive = 1 if shared_kwargs.get("stop_inclusive", False) else 0
        req.max_kv_count = shared_kwargs.get("max_kv_count", -1)
        req.max_kv_size = shared_kwargs.get("max_kv_size", -1)
        req.no_value = 1 if shared_kwargs.get("no_value", False) else 0
        req.reverse = 1 if shared_kwargs.get("reverse", False) else 0
        req.sort_key_filter_type = shared_kwargs.get("sort_key_filter_type", FT_NO_FILTER)
        req.sort_key_filter_pattern = _cslice(
            shared_kwargs.get("sort_key_filter_pattern", b""), keep)
        hks, offs = _pack(hash_keys)
        res = _Result()
        self._L.rrdb_multi_get_batch(self._h, len(hash_keys),
                                     hks.ctypes.data_as(C.c_void_p),
                                     offs.ctypes.data_as(C.c_void_p), C.byref(req), epoch_now,
                                     C.byref(res))
        del keep
        try:
            if res.error != OK:
                return res.error, []
            groups = []
            m = 0
            for i in range(len(hash_keys)):
                n = res.group_counts[i]
                kvs = [(_read_slice(res.keys[m + j]), _read_slice(res.values[m + j]))
                       for j in range(n)]
                m += n
                groups.append((res.group_errors[i], kvs))
            return OK, groups
        finally:
            self._L.rrdb_free_result(C.byref(res))

    def _scan_result(self, res: _Result, only_return_count, return_expire_ts, on_device):
        kvs = []
        ets = None
        dev = None
        if on_device:
            dev = dict(count=res.count, dev_keys=res.dev_keys, dev_key_offs=res.dev_key_offs,
                       dev_vals=res.dev_vals, dev_val_offs=res.dev_val_offs)
        elif not only_return_count:
            kvs = [(_read_slice(res.keys[i]), _read_slice(res.values[i]))
                   for i in range(res.count)]
            if return_expire_ts and res.expire_ts:
                ets = [res.expire_ts[i] for i in range(res.count)]
        return ScanResult(error=res.error, context_id=res.context_id, kvs=kvs,
                          kv_count=(res.i64 if only_return_count else None), expire_ts=ets,
                          dev=dev)

    def scan_open(self, start_key: bytes, stop_key: bytes, epoch_now: int, *,
                  start_inclusive=True, stop_inclusive=False, batch_size=-1, no_value=False,
                  hash_key_filter_type=FT_NO_FILTER, hash_key_filter_pattern=b"",
                  sort_key_filter_type=FT_NO_FILTER, sort_key_filter_pattern=b"",
                  full_scan=False, validate_partition_hash=True, return_expire_ts=False,
                  only_return_count=False, on_device_out=False) -> ScanResult:
        keep = []
        req = _ScanRequest()
        req.start_key = _cslice(start_key, keep)
        req.stop_key = _cslice(stop_key, keep)
        req.start_inclusive = 1 if start_inclusive else 0
        req.stop_inclusive = 1 if stop_inclusive else 0
        req.batch_size = batch_size
        req.no_value = 1 if no_value else 0
        req.hash_key_filter_type = hash_key_filter_type
        req.hash_key_filter_pattern = _cslice(hash_key_filter_pattern, keep)
        req.sort_key_filter_type = sort_key_filter_type
        req.sort_key_filter_pattern = _cslice(sort_key_filter_pattern, keep)
        req.full_scan = 1 if full_scan else 0
        req.validate_partition_hash = 1 if validate_partition_hash else 0
        req.return_expire_ts = 1 if return_expire_ts else 0
        req.only_return_count = 1 if only_return_count else 0
        req.on_device_out = 1 if on_device_out else 0
        res = _Result()
        self._L.rrdb_scan_open(self._h, C.byref(req), epoch_now, C.byref(res))
        try:
            out = self._scan_result(res, only_return_count, return_expire_ts, on_device_out)
            if out.context_id != SCAN_COMPLETED:
                # flags follow the parked context (ids change on every batch)
                self._scan_flags = getattr(self, "_scan_flags", {})
                self._scan_flags[out.context_id] = (only_return_count, return_expire_ts,
                                                    on_device_out)
            return out
        finally:
            self._L.rrdb_free_result(C.byref(res))

    def scan_count_begin(self, start_key: bytes, stop_key: bytes, epoch_now: int, *,
                         stop_inclusive=False, batch_size=2**31 - 1,
                         hash_key_filter_type=FT_NO_FILTER, hash_key_filter_pattern=b"",
                         sort_key_filter_type=FT_NO_FILTER, sort_key_filter_pattern=b"",
                         validate_partition_hash=True):
        """Submit a fused pipelined count scan; returns the C status.
        kInvalidArgument = shape unsupported -> fall back to scan_open."""
        keep = []
        req = _ScanRequest()
        req.start_key = _cslice(start_key, keep)
        req.stop_key = _cslice(stop_key, keep)
        req.start_inclusive = 1
        req.stop_inclusive = 1 if stop_inclusive else 0
        req.batch_size = batch_size
        req.no_value = 1
        req.hash_key_filter_type = hash_key_filter_type
        req.hash_key_filter_pattern = _cslice(hash_key_filter_pattern, keep)
        req.sort_key_filter_type = sort_key_filter_type
        req.sort_key_filter_pattern = _cslice(sort_key_filter_pattern, keep)
        req.full_scan = 1
        req.validate_partition_hash = 1 if validate_partition_hash else 0
        req.return_expire_ts = 0
        req.only_return_count = 1
        req.on_device_out = 0
        rc = self._L.rrdb_scan_count_begin(self._h, C.byref(req), epoch_now)
        del keep
        return rc

    def scan_count_finish(self):
        """(error, count) for a submitted scan_count_begin."""
        res = _Result()
        self._L.rrdb_scan_count_finish(self._h, C.byref(res))
        try:
            return res.error, res.i64
        finally:
            self._L.rrdb_free_result(C.byref(res))

    def scan_next(self, context_id: int, epoch_now: int) -> ScanResult:
        res = _Result()
        self._L.rrdb_scan_next(self._h, context_id, epoch_now, C.byref(res))
        try:
            flags = getattr(self, "_scan_flags", {})
            orc, ret, dev = flags.pop(context_id, (False, False, False))
            out = self._scan_result(res, orc, ret, dev)
            if out.context_id != SCAN_COMPLETED and out.error == OK:
                flags[out.context_id] = (orc, ret, dev)
            return out
        finally:
            self._L.rrdb_free_result(C.byref(res))

    def clear_scanner(self, context_id: int):
        self._L.rrdb_clear_scanner(self._h, context_id)

    def phase_ms(self, phase: str) -> float:
        return self._L.rrdb_phase_ms(self._h, phase.encode())

    # ---- write path (§8(f)1) ----
    def put(self, hash_key: bytes, sort_key: bytes, value: bytes, expire_ts: int = 0,
            epoch_now: int = 0):
        """epoch_now = the write's clock; with a default_ttl table env and
        expire_ts 0, the stored expire becomes epoch_now + default_ttl at
        WRITE time (rocksdb_wrapper.cpp:280-286)."""
        return self._L.rrdb_put(self._h, hash_key, len(hash_key), sort_key, len(sort_key),
                                value, len(value), expire_ts, epoch_now)

    def remove(self, hash_key: bytes, sort_key: bytes):
        return self._L.rrdb_remove(self._h, hash_key, len(hash_key), sort_key, len(sort_key))

    def flush(self):
        return self._L.rrdb_flush(self._h)

    def memtable_entries(self):
        return self._L.rrdb_memtable_entries(self._h)

    # ---- checkpoint (§8(f)2) ----
    def checkpoint(self, directory: str, decree: int):
        return self._L.rrdb_checkpoint(self._h, directory.encode(), decree)

    def restore(self, directory: str, decree: int):
        return self._L.rrdb_restore(self._h, directory.encode(), decree)

    def manual_compact(self, epoch_now: int, *, target_level=-1, bottommost_force=True,
                       keep_inputs=False):
        opts = _CompactOptions(target_level, 1 if bottommost_force else 0,
                               1 if keep_inputs else 0)
        st = _CompactStats()
        err = self._L.rrdb_manual_compact(self._h, C.byref(opts), epoch_now, C.byref(st))
        stats = CompactStats(**{f[0]: getattr(st, f[0]) for f in _CompactStats._fields_})
        return err, stats

    def manual_compact_begin(self, epoch_now: int, *, target_level=-1, bottommost_force=True,
                             keep_inputs=False):
        """Submit the compaction's merge phase without blocking; pair with
        manual_compact_finish.  The pipelined-partitions seam
        (include/rrdb_engine.h)."""
        opts = _CompactOptions(target_level, 1 if bottommost_force else 0,
                               1 if keep_inputs else 0)
        return self._L.rrdb_manual_compact_begin(self._h, C.byref(opts), epoch_now)

    def manual_compact_finish(self, epoch_now: int = 0):
        st = _CompactStats()
        err = self._L.rrdb_manual_compact_finish(self._h, C.byref(st))
        stats = CompactStats(**{f[0]: getattr(st, f[0]) for f in _CompactStats._fields_})
        return err, stats

    # ---- window (minor) compaction: engine-only (include/rrdb_engine_ext.h) ----
    def _need_window_compact(self, what: str):
        if not self.lib.has_window_compact:
            raise RuntimeError(
                f"{what}: backend {self.lib.backend!r} ({self.lib.path}) does not export "
                "rrdb_compact_runs/rrdb_auto_compact (engine-only extensions)")

    def compact_runs(self, first: int, n: int, epoch_now: int):
        """Merge runs [first, first+n) (0 = oldest) into one run in their
        place; bottommost iff first == 0.  Returns (err, CompactStats), like
        manual_compact."""
        self._need_window_compact("compact_runs")
        st = _CompactStats()
        err = self._L.rrdb_compact_runs(self._h, first, n, epoch_now, C.byref(st))
        stats = CompactStats(**{f[0]: getattr(st, f[0]) for f in _CompactStats._fields_})
        return err, stats

    def auto_compact(self, epoch_now: int):
        """Background-compaction tick.  Returns (err, first, n, CompactStats);
        n == 0 means nothing was compacted."""
        self._need_window_compact("auto_compact")
        st = _CompactStats()
        first, n = C.c_uint64(0), C.c_uint64(0)
        err = self._L.rrdb_auto_compact(self._h, epoch_now, C.byref(first), C.byref(n),
                                        C.byref(st))
        stats = CompactStats(**{f[0]: getattr(st, f[0]) for f in _CompactStats._fields_})
        return err, first.value, n.value, stats

    # ---- compaction route: engine-only (include/rrdb_engine_ext.h) ----
    def last_compact_route(self):
        """(rank, emit) of the last compaction pass on this handle: the
        ROUTE_RANK_* / ROUTE_EMIT_* values, ROUTE_NONE where no kernel ran."""
        if not self.lib.has_compact_route:
            raise RuntimeError(
                f"last_compact_route: backend {self.lib.backend!r} ({self.lib.path}) does not "
                "export rrdb_last_compact_route (engine-only extension)")
        rt = _CompactRoute()
        err = self._L.rrdb_last_compact_route(self._h, C.byref(rt))
        if err != OK:
            raise RuntimeError(f"rrdb_last_compact_route failed: status {err}")
        return rt.rank, rt.emit

    # ---- multi_get lane: engine-only (include/rrdb_engine_ext.h) ----
    def last_multi_get_lane(self) -> MultiGetLane:
        """Which serving lane the last multi_get on this handle took (the
        MG_LANE_* values), whether a fused lane handed it back first, whether
        the response needed the second device read, and the fused / fallback
        split of the last multi_get_batch."""
        if not self.lib.has_multi_get_lane:
            raise RuntimeError(
                f"last_multi_get_lane: backend {self.lib.backend!r} ({self.lib.path}) does not "
                "export rrdb_last_multi_get_lane (engine-only extension)")
        ln = _MultiGetLane()
        err = self._L.rrdb_last_multi_get_lane(self._h, C.byref(ln))
        if err != OK:
            raise RuntimeError(f"rrdb_last_multi_get_lane failed: status {err}")
        return MultiGetLane(**{f[0]: getattr(ln, f[0]) for f in _MultiGetLane._fields_})

    # ---- view route: engine-only (include/rrdb_engine_ext.h) ----
    def last_view_route(self) -> ViewRoute:
        """Which rank kernel built the last read view on this handle (the
        ROUTE_RANK_* values, ROUTE_NONE for an empty range), through how many
        bound-table levels, over how many groups and records, and how many
        rows the view holds."""
        if not self.lib.has_view_route:
            raise RuntimeError(
                f"last_view_route: backend {self.lib.backend!r} ({self.lib.path}) does not "
                "export rrdb_last_view_route (engine-only extension)")
        rt = _ViewRoute()
        err = self._L.rrdb_last_view_route(self._h, C.byref(rt))
        if err != OK:
            raise RuntimeError(f"rrdb_last_view_route failed: status {err}")
        return ViewRoute(**{f[0]: getattr(rt, f[0]) for f in _ViewRoute._fields_})

    # ---- partition split: engine-only (include/rrdb_engine_ext.h) ----
    def split(self, child: "RrdbPartition", new_partition_count: int):
        """Split this partition (p of N) on the device into itself and `child`
        (p + N, an empty handle on the same GPU), new_partition_count = 2N.
        Returns (err, SplitStats), like manual_compact."""
        if not self.lib.has_split:
            raise RuntimeError(
                f"split: backend {self.lib.backend!r} ({self.lib.path}) does not export "
                "rrdb_split (engine-only extension)")
        if child.lib is not self.lib:
            raise RuntimeError("split: parent and child must come from the same library")
        st = _SplitStats()
        err = self._L.rrdb_split(self._h, child._h, new_partition_count, C.byref(st))
        stats = SplitStats(**{f[0]: getattr(st, f[0]) for f in _SplitStats._fields_})
        return err, stats

    # ---- batched writes: engine-only (include/rrdb_engine_ext.h) ----
    def _need_write_batch(self):
        if not self.lib.has_write_batch:
            raise RuntimeError(
                f"write_batch: backend {self.lib.backend!r} ({self.lib.path}) does not export "
                "rrdb_write_batch (engine-only extension)")

    def write_batch_arrays(self, keys_u8, key_offs_u64, vals_u8, val_offs_u64, expire_u32,
                           kinds_u8, epoch_now: int = 0):
        """write_batch from packed numpy arrays (no python loop; the bench and
        the rejection tests, which hand in malformed arrays, use it)."""
        import numpy as np

        self._need_write_batch()
        for a, dt in ((keys_u8, np.uint8), (key_offs_u64, np.uint64), (vals_u8, np.uint8),
                      (val_offs_u64, np.uint64), (expire_u32, np.uint32), (kinds_u8, np.uint8)):
            assert a.dtype == dt and a.flags["C_CONTIGUOUS"], (a.dtype, dt)
        st = _WriteBatchStats()
        err = self._L.rrdb_write_batch(
            self._h, len(kinds_u8),
            keys_u8.ctypes.data_as(C.c_void_p), key_offs_u64.ctypes.data_as(C.c_void_p),
            vals_u8.ctypes.data_as(C.c_void_p), val_offs_u64.ctypes.data_as(C.c_void_p),
            expire_u32.ctypes.data_as(C.c_void_p), kinds_u8.ctypes.data_as(C.c_void_p),
            epoch_now, C.byref(st))
        stats = WriteBatchStats(**{f[0]: getattr(st, f[0]) for f in _WriteBatchStats._fields_})
        return err, stats

    def write_batch(self, ops, epoch_now: int = 0):
        """Apply `ops`, a list of (full_key, value_or_None, expire_ts) in
        commit order (None = remove; duplicate keys allowed, the last op on a
        key wins), as one new run sorted and deduplicated on the device.
        Returns (err, WriteBatchStats)."""
        import numpy as np

        self._need_write_batch()
        keys, koffs = _pack([o[0] for o in ops])
        vals, voffs = _pack([o[1] if o[1] is not None else b"" for o in ops])
        expire = np.array([o[2] if o[1] is not None else 0 for o in ops], dtype=np.uint32)
        kinds = np.array([0 if o[1] is not None else 1 for o in ops], dtype=np.uint8)
        return self.write_batch_arrays(keys, koffs, vals, voffs, expire, kinds, epoch_now)

    # ---- batched counter increments: engine-only (include/rrdb_engine_ext.h) ----
    def _need_incr_batch(self):
        if not self.lib.has_incr_batch:
            raise RuntimeError(
                f"incr_batch: backend {self.lib.backend!r} ({self.lib.path}) does not export "
                "rrdb_incr_batch (engine-only extension)")

    def incr_batch_arrays(self, keys_u8, key_offs_u64, increments_i64, expire_i32,
                          epoch_now: int = 0):
        """incr_batch from packed numpy arrays (no python loop; the bench and
        the rejection tests, which hand in malformed arrays, use it).
        expire_i32 may be None (every directive 0).  Returns
        (err, new_values int64 array, errors int32 array, IncrBatchStats)."""
        import numpy as np

        self._need_incr_batch()
        for a, dt in ((keys_u8, np.uint8), (key_offs_u64, np.uint64),
                      (increments_i64, np.int64), (expire_i32, np.int32)):
            assert a is None or (a.dtype == dt and a.flags["C_CONTIGUOUS"]), (a.dtype, dt)
        n = len(increments_i64)
        new_values = np.zeros(n, dtype=np.int64)
        errors = np.zeros(n, dtype=np.int32)
        st = _IncrBatchStats()
        err = self._L.rrdb_incr_batch(
            self._h, n,
            keys_u8.ctypes.data_as(C.c_void_p), key_offs_u64.ctypes.data_as(C.c_void_p),
            increments_i64.ctypes.data_as(C.c_void_p),
            None if expire_i32 is None else expire_i32.ctypes.data_as(C.c_void_p),
            epoch_now, new_values.ctypes.data_as(C.c_void_p),
            errors.ctypes.data_as(C.c_void_p), C.byref(st))
        stats = IncrBatchStats(**{f[0]: getattr(st, f[0]) for f in _IncrBatchStats._fields_})
        return err, new_values, errors, stats

    def incr_batch(self, ops, epoch_now: int = 0):
        """Apply `ops`, a list of (full_key, increment, expire_directive) in
        commit order (duplicate keys allowed: each op sees the ones before
        it), as the reference's incr would, one after the other, on the
        device.  Returns (err, new_values, errors, IncrBatchStats) with the
        per-op results as python lists."""
        import numpy as np

        self._need_incr_batch()
        keys, koffs = _pack([o[0] for o in ops])
        inc = np.array([o[1] for o in ops], dtype=np.int64)
        expire = np.array([o[2] for o in ops], dtype=np.int32)
        err, nv, er, stats = self.incr_batch_arrays(keys, koffs, inc, expire, epoch_now)
        return err, [int(x) for x in nv], [int(x) for x in er], stats

    # ---- batched writes with timetags: engine-only (include/rrdb_engine_ext.h) ----
    def _need_write_batch_timetag(self):
        if not self.lib.has_write_batch_timetag:
            raise RuntimeError(
                f"write_batch_timetag: backend {self.lib.backend!r} ({self.lib.path}) does not "
                "export rrdb_write_batch_timetag (engine-only extension)")

    def write_batch_timetag_arrays(self, keys_u8, key_offs_u64, vals_u8, val_offs_u64,
                                   expire_u32, kinds_u8, timetags_u64, verify_u8,
                                   epoch_now: int = 0):
        """write_batch_timetag from packed numpy arrays (no python loop; the
        bench and the rejection tests, which hand in malformed arrays, use it).
        timetags_u64 and verify_u8 may be None (all zero).  Returns
        (err, applied uint8 array, TimetagBatchStats)."""
        import numpy as np

        self._need_write_batch_timetag()
        for a, dt in ((keys_u8, np.uint8), (key_offs_u64, np.uint64), (vals_u8, np.uint8),
                      (val_offs_u64, np.uint64), (expire_u32, np.uint32), (kinds_u8, np.uint8),
                      (timetags_u64, np.uint64), (verify_u8, np.uint8)):
            assert a is None or (a.dtype == dt and a.flags["C_CONTIGUOUS"]), (a.dtype, dt)
        n = len(kinds_u8)
        applied = np.zeros(n, dtype=np.uint8)
        st = _TimetagBatchStats()
        err = self._L.rrdb_write_batch_timetag(
            self._h, n,
            keys_u8.ctypes.data_as(C.c_void_p), key_offs_u64.ctypes.data_as(C.c_void_p),
            vals_u8.ctypes.data_as(C.c_void_p), val_offs_u64.ctypes.data_as(C.c_void_p),
            expire_u32.ctypes.data_as(C.c_void_p), kinds_u8.ctypes.data_as(C.c_void_p),
            None if timetags_u64 is None else timetags_u64.ctypes.data_as(C.c_void_p),
            None if verify_u8 is None else verify_u8.ctypes.data_as(C.c_void_p),
            epoch_now, applied.ctypes.data_as(C.c_void_p), C.byref(st))
        stats = TimetagBatchStats(**{f[0]: getattr(st, f[0])
                                     for f in _TimetagBatchStats._fields_})
        return err, applied, stats

    def write_batch_timetag(self, ops, epoch_now: int = 0):
        """Apply `ops`, a list of (full_key, value_or_None, expire_ts, timetag,
        verify) in commit order (None = remove; duplicate keys allowed: each
        op sees the ones before it), as the reference's duplicate handler
        would, one after the other, on the device.  A verified PUT is dropped
        when the stored record is live and its timetag is not smaller.
        Returns (err, applied_list, TimetagBatchStats)."""
        import numpy as np

        self._need_write_batch_timetag()
        keys, koffs = _pack([o[0] for o in ops])
        vals, voffs = _pack([o[1] if o[1] is not None else b"" for o in ops])
        expire = np.array([o[2] if o[1] is not None else 0 for o in ops], dtype=np.uint32)
        kinds = np.array([0 if o[1] is not None else 1 for o in ops], dtype=np.uint8)
        timetags = np.array([o[3] for o in ops], dtype=np.uint64)
        verify = np.array([1 if o[4] else 0 for o in ops], dtype=np.uint8)
        err, ap, stats = self.write_batch_timetag_arrays(keys, koffs, vals, voffs, expire, kinds,
                                                         timetags, verify, epoch_now)
        return err, [int(x) for x in ap], stats

    # ---- batched check-and-mutate: engine-only (include/rrdb_engine_ext.h) ----
    def _need_check_and_mutate_batch(self):
        if not self.lib.has_check_and_mutate_batch:
            raise RuntimeError(
                f"check_and_mutate_batch: backend {self.lib.backend!r} ({self.lib.path}) does "
                "not export rrdb_check_and_mutate_batch (engine-only extension)")

    def check_and_mutate_batch_arrays(self, check_keys_u8, check_key_offs_u64, check_types_i32,
                                      operands_u8, operand_offs_u64, mut_offs_u64, mut_keys_u8,
                                      mut_key_offs_u64, mut_vals_u8, mut_val_offs_u64,
                                      mut_expire_u32, mut_kinds_u8, return_u8,
                                      epoch_now: int = 0, *, want_errors=True,
                                      want_exist=True, want_values=True, want_stats=True):
        """check_and_mutate_batch from packed numpy arrays (no python loop; the
        bench and the rejection tests, which hand in malformed arrays, use
        it).  Any array may be None (passed as NULL); mut_expire_u32 = None
        means every expire_ts is 0 and return_u8 = None means no check value
        is asked for.  The want_* switches pass NULL for that output.  The C
        call takes the mutation count from mut_offs[n]; a mut_offs[n] that
        differs from len(mut_kinds_u8) is refused here as kInvalidArgument.
        Returns (err, errors int32 array, check_exist uint8 array,
        check_values list[bytes], CasBatchStats); an output that was not asked
        for is None."""
        import numpy as np

        self._need_check_and_mutate_batch()
        for a, dt in ((check_keys_u8, np.uint8), (check_key_offs_u64, np.uint64),
                      (check_types_i32, np.int32), (operands_u8, np.uint8),
                      (operand_offs_u64, np.uint64), (mut_offs_u64, np.uint64),
                      (mut_keys_u8, np.uint8), (mut_key_offs_u64, np.uint64),
                      (mut_vals_u8, np.uint8), (mut_val_offs_u64, np.uint64),
                      (mut_expire_u32, np.uint32), (mut_kinds_u8, np.uint8),
                      (return_u8, np.uint8)):
            assert a is None or (a.dtype == dt and a.flags["C_CONTIGUOUS"]), (a.dtype, dt)
        n = next(len(a) - d for a, d in ((check_types_i32, 0), (check_key_offs_u64, 1),
                                         (operand_offs_u64, 1), (mut_offs_u64, 1))
                 if a is not None)
        if (mut_offs_u64 is not None and mut_kinds_u8 is not None
                and len(mut_offs_u64) == n + 1 and int(mut_offs_u64[n]) != len(mut_kinds_u8)):
            return INVALID_ARGUMENT, None, None, None, CasBatchStats()

        def ptr(a):
            return None if a is None else a.ctypes.data_as(C.c_void_p)

        errors = np.zeros(n, dtype=np.int32) if want_errors else None
        exist = np.zeros(n, dtype=np.uint8) if want_exist else None
        res = _Result() if want_values else None
        st = _CasBatchStats() if want_stats else None
        err = self._L.rrdb_check_and_mutate_batch(
            self._h, n, ptr(check_keys_u8), ptr(check_key_offs_u64), ptr(check_types_i32),
            ptr(operands_u8), ptr(operand_offs_u64), ptr(mut_offs_u64), ptr(mut_keys_u8),
            ptr(mut_key_offs_u64), ptr(mut_vals_u8), ptr(mut_val_offs_u64), ptr(mut_expire_u32),
            ptr(mut_kinds_u8), ptr(return_u8), epoch_now, ptr(errors), ptr(exist),
            C.byref(res) if res is not None else None, C.byref(st) if st is not None else None)
        values = None
        if res is not None:
            try:
                if err == OK and res.count:
                    values = [_read_slice(res.values[i]) for i in range(res.count)]
                elif err == OK:
                    values = []
            finally:
                self._L.rrdb_free_result(C.byref(res))
        stats = None if st is None else CasBatchStats(
            **{f[0]: getattr(st, f[0]) for f in _CasBatchStats._fields_})
        return err, errors, exist, values, stats

    @staticmethod
    def pack_check_and_mutate_ops(ops):
        """ops -> the thirteen input arrays of check_and_mutate_batch_arrays."""
        import numpy as np

        ck, ckoffs = _pack([o[0] for o in ops])
        types = np.array([o[1] for o in ops], dtype=np.int32)
        opd, opoffs = _pack([o[2] for o in ops])
        muts = [m for o in ops for m in o[3]]
        moffs = np.zeros(len(ops) + 1, dtype=np.uint64)
        moffs[1:] = np.cumsum([len(o[3]) for o in ops], dtype=np.uint64)
        mk, mkoffs = _pack([m[0] for m in muts])
        mv, mvoffs = _pack([m[1] if m[1] is not None else b"" for m in muts])
        mexp = np.array([m[2] if m[1] is not None else 0 for m in muts], dtype=np.uint32)
        kinds = np.array([(m[3] if len(m) > 3 else (0 if m[1] is not None else 1))
                          for m in muts], dtype=np.uint8)
        ret = np.array([1 if o[4] else 0 for o in ops], dtype=np.uint8)
        return ck, ckoffs, types, opd, opoffs, moffs, mk, mkoffs, mv, mvoffs, mexp, kinds, ret

    def check_and_mutate_batch(self, ops, epoch_now: int = 0):
        """Check and apply `ops`, a list of (check_key, check_type, operand,
        [(key, value_or_None, expire_ts), ...], return_check_value) in commit
        order (None = remove; duplicate keys allowed: each op sees the ones
        before it), as the reference's check_and_mutate would, one after the
        other, on the device.  A mutation may carry a fourth element, its raw
        kind byte.  Returns (err, errors, check_exist, check_values,
        CasBatchStats) with the per-op results as python lists."""
        self._need_check_and_mutate_batch()
        if not ops:
            return OK, [], [], [], CasBatchStats()
        err, er, ex, vals, stats = self.check_and_mutate_batch_arrays(
            *self.pack_check_and_mutate_ops(ops), epoch_now)
        if err != OK:
            return err, None, None, None, stats
        return err, [int(x) for x in er], [bool(x) for x in ex], vals, stats

    def check_and_set_batch(self, ops, epoch_now: int = 0):
        """check_and_set: `ops` is a list of (check_key, check_type, operand,
        set_key, set_value, set_expire_ts, return_check_value); set_key equal
        to check_key is set_diff_sort_key == false.  One PUT mutation per op."""
        return self.check_and_mutate_batch(
            [(o[0], o[1], o[2], [(o[3], o[4], o[5])], o[6]) for o in ops], epoch_now)
