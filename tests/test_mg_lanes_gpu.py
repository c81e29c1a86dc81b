"""GPU parity for the multi_get serving lanes at their size and run-count
limits: the HIP engine against the CPU oracle, byte for byte, on the case
table of tests/mg_lane_cases.py (tests/test_mg_lanes_model.py pins the oracle
and the table on the CPU).

  - every single-request case under the server, graph and plain settings: the
    result, the lane rrdb_last_multi_get_lane names, and the hand-back and
    tail-read flags the case's tier predicts.  A lane that silently switched
    itself off fails here;
  - the server lane's device buffer across a tail read, a small request and
    another large one;
  - every batch case: engine == oracle == the engine's own per-request loop,
    and the fused / fallback split the table predicts;
  - the device-resident output of the batch and of the scan, copied back with
    hipMemcpy and decoded region by region;
  - handles with 32, 33, 64 and 65 runs: every read, a manual compaction under
    each engine.rank_mode with its stats and route, every read again.
"""
import ctypes as C

import numpy as np
import pytest

import mg_lane_cases as MC
from incubator_pegasus_amd.capi import (MG_LANE_GENERAL, MG_LANE_NONE, OK,
                                        ROUTE_RANK_GRP, ROUTE_RANK_LDS, SCAN_COMPLETED,
                                        _MultiGetRequest, _Result, _ScanRequest, _cslice, _pack)
from mg_lane_cases import NOW
from pymodel import Model
from test_mg_lanes_model import ITER_COUNT_ENV, rc_reads
from test_scan_differential import _drain_batches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trio(oracle_lib, hip_lib):
    runs = MC.build_runs()
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    for r in runs:
        o.ingest_run(r)
        g.ingest_run(r)
    yield runs, o, g
    o.close()
    g.close()


@pytest.fixture(scope="module")
def want_single(trio):
    """the oracle's answer to every single-request case, computed once"""
    _, o, _ = trio
    return {c.name: o.multi_get(c.hk, NOW, **c.kw) for c in MC.SINGLE_CASES}


def _lane(g):
    r = g.last_multi_get_lane()
    return r.lane, r.fused_first, r.tail_read


# ---------------- single requests ----------------

@pytest.mark.parametrize("setting", sorted(MC.LANE_SETTINGS))
def test_single_cases_bytes_and_lane(trio, want_single, setting):
    _, _, g = trio
    g.set_envs(MC.LANE_SETTINGS[setting])
    for c in MC.SINGLE_CASES:
        got = g.multi_get(c.hk, NOW, **c.kw)
        lane = _lane(g)
        assert got == want_single[c.name], (setting, c.name)
        assert lane == MC.expected_lane(c, setting), (setting, c.name)
    # the two adjacent request sizes flip the lane; nothing else differs
    by = {c.name: c for c in MC.SINGLE_CASES}
    flip = []
    for name in ("req-graph-max", "req-graph-max+1"):
        g.multi_get(by[name].hk, NOW, **by[name].kw)
        flip.append(_lane(g)[0])
    assert flip == [MC.FUSED_LANE[setting], MC.FUSED_LANE["small"]]


def test_server_buffer_across_tail_reads(trio, want_single):
    """The resident server writes every response into one device buffer and
    the host reads a large one from it while the kernel is still running:
    a small request and another large one after a tail read see their own
    bytes only."""
    _, _, g = trio
    g.set_envs(MC.LANE_SETTINGS["server"])
    by = {c.name: c for c in MC.SINGLE_CASES}
    order = ["bigfit", "ordinary", "k100", "one-prefix", "v65535", "bigfit-rev", "miss",
             "many-prefix+1", "sk65535", "k100-cut", "many-prefix-1", "bigfit"]
    for rep in range(2):
        for name in order:
            c = by[name]
            assert g.multi_get(c.hk, NOW, **c.kw) == want_single[name], (rep, name)
            assert _lane(g) == MC.expected_lane(c, "server"), (rep, name)


@pytest.mark.parametrize("setting", sorted(MC.LANE_SETTINGS))
def test_prefix_clamp_cases(oracle_lib, hip_lib, setting):
    """A sort-key prefix filter clamps both ends of the range before a lane
    sees it.  Two overlapping runs, no compaction, an iteration cap that the
    clamped walk just fits: engine == oracle == model on every case, on a
    fused lane and, for the hashkey with the over-long row, on the general one."""
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    try:
        m = Model()
        for r in MC.pfx_runs():
            o.ingest_run(r)
            g.ingest_run(r)
            m.ingest(r)
        g.set_envs(MC.LANE_SETTINGS[setting])
        fused = MC.FUSED_LANE[setting]
        for cap in (MC.PFX_ITER_CAP, MC.MG_ITER_COUNT):
            o.set_envs({ITER_COUNT_ENV: str(cap)})
            g.set_envs({ITER_COUNT_ENV: str(cap)})
            for hk, lane in ((MC.PFX_HK, (fused, MG_LANE_NONE, 0)),
                             (MC.PFX_HK_WIDE, (MG_LANE_GENERAL, fused, 0))):
                for name, kw in MC.PFX_CASES.items():
                    want = m.multi_get(hk, NOW, engine_max_iter=cap, **kw)
                    assert want[0] == OK and len(want[1]) >= MC.PFX_ITERATED - 2
                    assert o.multi_get(hk, NOW, **kw) == want, (cap, hk, name)
                    assert g.multi_get(hk, NOW, **kw) == want, (cap, hk, name)
                    assert _lane(g) == lane, (cap, hk, name)
        assert g.num_runs() == 2
    finally:
        o.close()
        g.close()


# ---------------- batch ----------------

def _predicted_fallbacks(runs, reqs, kw, want):
    return sum(MC.batch_falls_back(runs, h, kw, r[1]) for h, r in zip(reqs, want))


@pytest.mark.parametrize("variant", sorted(MC.BATCH_VARIANTS))
def test_batch_cases(trio, variant):
    runs, o, g = trio
    kw = MC.BATCH_VARIANTS[variant]
    reqs = MC.batch_requests()
    # the per-request loop runs on the server lane for one variant, so that
    # the batch retires a live resident kernel, and on the plain lane otherwise
    g.set_envs(MC.LANE_SETTINGS["server" if variant == "default" else "small"])
    g.multi_get(MC.ORDINARY[0], NOW)
    before = _lane(g)
    werr, want = o.multi_get_batch(reqs, NOW, **kw)
    err, got = g.multi_get_batch(reqs, NOW, **kw)
    rep = g.last_multi_get_lane()
    assert err == werr == OK
    for h, a, b in zip(reqs, got, want):
        assert a == b, (variant, h[:16])
    fb = _predicted_fallbacks(runs, reqs, kw, want)
    assert (rep.batch_fused, rep.batch_fallback, rep.batch_device_out) == \
        (len(reqs) - fb, fb, 0)
    assert (rep.lane, rep.fused_first, rep.tail_read) == before  # a batch leaves these
    singles = [g.multi_get(h, NOW, **kw) for h in reqs]
    for h, a, b in zip(reqs, singles, want):
        assert a == b, (variant, h[:16])


def test_batch_of_one(trio):
    runs, o, g = trio
    for h in MC.BATCH_SPECIAL + [MC.ORDINARY[5]]:
        want = o.multi_get_batch([h], NOW)
        assert g.multi_get_batch([h], NOW) == want, h[:16]
        rep = g.last_multi_get_lane()
        fb = int(MC.batch_falls_back(runs, h, {}, want[1][0][1]))
        assert (rep.batch_fused, rep.batch_fallback) == (1 - fb, fb), h[:16]


# ---------------- device-resident output ----------------

_hip = None


def _d2h(ptr, n):
    """n bytes of device memory, through hipMemcpy"""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.restype = C.c_int
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    if n == 0:
        return b""
    assert ptr
    buf = (C.c_uint8 * n)()
    assert _hip.hipMemcpy(buf, C.c_void_p(ptr), n, 2) == 0  # hipMemcpyDeviceToHost
    return bytes(buf)


def _u64s(raw):
    return [int(x) for x in np.frombuffer(raw, dtype=np.uint64)]


def _batch_device_out(g, hks, **kw):
    """rrdb_multi_get_batch with on_device_out: (error, [(error, rows) per
    request] decoded from the device buffers or None when they were not
    delivered, region offsets)"""
    keep = []
    req = _MultiGetRequest()
    req.start_inclusive = 1
    req.max_kv_count = kw.get("max_kv_count", -1)
    req.max_kv_size = kw.get("max_kv_size", -1)
    req.no_value = 1 if kw.get("no_value") else 0
    req.reverse = 1 if kw.get("reverse") else 0
    req.sort_key_filter_type = kw.get("sort_key_filter_type", 0)
    req.sort_key_filter_pattern = _cslice(kw.get("sort_key_filter_pattern", b""), keep)
    req.on_device_out = 1
    blob, offs = _pack(hks)
    res = _Result()
    g._L.rrdb_multi_get_batch(g._h, len(hks), blob.ctypes.data_as(C.c_void_p),
                              offs.ctypes.data_as(C.c_void_p), C.byref(req), NOW, C.byref(res))
    try:
        if res.error != OK or not res.dev_vals:
            return res.error, None, None
        n = len(hks)
        poff = _u64s(_d2h(res.dev_val_offs, (n + 1) * 8))
        packed = _d2h(res.dev_vals, poff[n])
        groups = []
        for i in range(n):
            m = res.group_counts[i]
            region = packed[poff[i]:poff[i + 1]]
            assert len(region) >= 16 * (m + 1)
            koff = _u64s(region[:8 * (m + 1)])
            voff = _u64s(region[8 * (m + 1):16 * (m + 1)])
            kb = region[16 * (m + 1):16 * (m + 1) + koff[m]]
            vb = region[16 * (m + 1) + koff[m]:]
            assert len(vb) == voff[m] and koff[0] == voff[0] == 0
            groups.append((res.group_errors[i],
                           [(kb[koff[j]:koff[j + 1]], vb[voff[j]:voff[j + 1]])
                            for j in range(m)]))
        assert res.count == sum(len(r) for _, r in groups)
        return OK, groups, poff
    finally:
        g._L.rrdb_free_result(C.byref(res))


@pytest.mark.parametrize("variant", ["default", "no_value", "count3", "reverse"])
def test_batch_device_out_bytes(trio, variant):
    _, o, g = trio
    kw = MC.BATCH_VARIANTS[variant]
    reqs = MC.DEVICE_OUT_REQUESTS
    werr, want = o.multi_get_batch(reqs, NOW, **kw)
    err, got, poff = _batch_device_out(g, reqs, **kw)
    rep = g.last_multi_get_lane()
    assert err == werr == OK and got is not None
    assert (rep.batch_fused, rep.batch_fallback, rep.batch_device_out) == (len(reqs), 0, 1)
    for h, a, b in zip(reqs, got, want):
        assert a == b, (variant, h[:16])
    assert got == g.multi_get_batch(reqs, NOW, **kw)[1]  # the host-marshalled result
    assert got[reqs.index(MC.MISS)] == (OK, [])           # a request with zero rows
    assert sum(1 for x in poff[:-1] if x % 8) > 10        # regions off the 8-byte grid
    assert poff[0] == 0 and poff == sorted(poff)


def test_batch_device_out_needs_every_request_fused(trio):
    """one request that the kernel hands back keeps the whole batch on the
    host path: nothing is delivered on the device and the report says so"""
    _, o, g = trio
    reqs = MC.DEVICE_OUT_REQUESTS[:10] + [b"b64k1"] + MC.DEVICE_OUT_REQUESTS[10:20]
    err, got, _ = _batch_device_out(g, reqs)
    rep = g.last_multi_get_lane()
    assert err == OK and got is None
    assert (rep.batch_fused, rep.batch_fallback, rep.batch_device_out) == (len(reqs) - 1, 1, 0)
    assert g.multi_get_batch(reqs, NOW) == o.multi_get_batch(reqs, NOW)


def _scan_pages_device_out(g, kw):
    """pages of a scan with on_device_out, decoded from the device buffers"""
    keep = []
    req = _ScanRequest()
    req.start_key = _cslice(kw["start_key"], keep)
    req.stop_key = _cslice(kw["stop_key"], keep)
    req.start_inclusive = 1
    req.stop_inclusive = 0
    req.batch_size = kw["batch_size"]
    req.no_value = 1 if kw["no_value"] else 0
    req.validate_partition_hash = 0
    req.on_device_out = 1
    pages = []
    res = _Result()
    g._L.rrdb_scan_open(g._h, C.byref(req), NOW, C.byref(res))
    while True:
        try:
            assert res.error == OK
            n = res.count
            kvs = []
            if n:
                koff = _u64s(_d2h(res.dev_key_offs, (n + 1) * 8))
                voff = _u64s(_d2h(res.dev_val_offs, (n + 1) * 8))
                assert koff[0] == voff[0] == 0
                kb = _d2h(res.dev_keys, koff[n])
                vb = _d2h(res.dev_vals, voff[n])
                kvs = [(kb[koff[j]:koff[j + 1]], vb[voff[j]:voff[j + 1]]) for j in range(n)]
            pages.append(kvs)
            ctx = res.context_id
        finally:
            g._L.rrdb_free_result(C.byref(res))
        if ctx == SCAN_COMPLETED:
            return pages
        res = _Result()
        g._L.rrdb_scan_next(g._h, ctx, NOW, C.byref(res))


@pytest.mark.parametrize("case", range(len(MC.SCAN_CASES)))
def test_scan_device_out_bytes(trio, case):
    _, o, g = trio
    kw = MC.SCAN_CASES[case]
    err, want = _drain_batches(o, kw, 1000)
    assert err == OK
    assert _drain_batches(g, kw, 1000) == (OK, want)
    assert _scan_pages_device_out(g, kw) == [b[0] for b in want]


# ---------------- run-count handles ----------------

def _count_scan(p):
    """(fused?, error, count) of a full count scan"""
    if p.scan_count_begin(b"\x00\x00", b"\xff\xff", NOW, validate_partition_hash=False) == OK:
        return (True,) + tuple(p.scan_count_finish())
    res = p.scan_open(b"\x00\x00", b"\xff\xff", NOW, only_return_count=True, full_scan=True,
                      batch_size=2**31 - 1, validate_partition_hash=False)
    return False, res.error, res.kv_count


def _check_reads(o, g, shape, n_runs, count_fused):
    want = rc_reads(o, shape)
    hks = MC.rc_hashkeys(shape) + [b"absent"]
    for setting in sorted(MC.LANE_SETTINGS):
        g.set_envs(MC.LANE_SETTINGS[setting])
        assert rc_reads(g, shape) == want, setting
        # rc_reads ends on a scan; the last multi_get decides the report
        g.multi_get(hks[0], NOW)
        fused = MC.FUSED_LANE[setting]
        assert _lane(g) == ((fused, MG_LANE_NONE, 0) if n_runs <= MC.RRDB_MAX_RUNS
                            else (MG_LANE_GENERAL, MG_LANE_NONE, 0)), setting
    for kw in MC.RC_MULTI_GETS.values():
        if kw.get("start_sortkey"):
            continue  # the batch takes no sortkey bounds
        assert g.multi_get_batch(hks, NOW, **kw) == o.multi_get_batch(hks, NOW, **kw)
        rep = g.last_multi_get_lane()
        assert (rep.batch_fused, rep.batch_fallback) == \
            ((len(hks), 0) if n_runs <= MC.RRDB_MAX_RUNS else (0, len(hks)))
    got, exp = _count_scan(g), _count_scan(o)
    assert got[1:] == exp[1:] and got[1] == OK
    assert got[0] == count_fused


@pytest.mark.parametrize("mode", ["grp", "ldst", "lds", "global"])
@pytest.mark.parametrize("n_runs", MC.RUN_COUNTS)
@pytest.mark.parametrize("shape", ["fixed", "var"])
def test_run_count_handles(oracle_lib, hip_lib, shape, n_runs, mode):
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    try:
        g.set_envs({"engine.rank_mode": mode})
        for r in MC.rc_runs(shape, n_runs):
            o.ingest_run(r)
            g.ingest_run(r)
        assert g.num_runs() == o.num_runs() == n_runs
        # the fused count scan runs on the group rank only
        _check_reads(o, g, shape, n_runs,
                     mode == "grp" and shape == "fixed" and n_runs <= MC.LDST_MAXR)
        assert g.manual_compact(NOW) == o.manual_compact(NOW)
        route = g.last_compact_route()[0]
        assert route == MC.expected_rank_route(shape, n_runs, mode)
        if n_runs > MC.LDST_MAXR:
            assert route != ROUTE_RANK_GRP
        if n_runs > MC.RRDB_MAX_RUNS:
            assert route != ROUTE_RANK_LDS
        assert g.num_runs() == 1
        _check_reads(o, g, shape, 1, True)
    finally:
        o.close()
        g.close()
