"""Shared case table for the multi_get serving lanes at their size and
run-count limits (tests/test_mg_lanes_model.py on the CPU,
tests/test_mg_lanes_gpu.py on the device).

One device function (mg_core, kernels.hip) answers a range multi_get behind
four lanes: the plain k_multi_get_small launch, the captured graph, the
resident mailbox server and k_multi_get_batch.  The lanes differ in how the
request goes in and how the response comes back, and each of those has size
tiers.  This module builds one small multi-run data set and, per tier, the
smallest request that crosses into it.  The constants below mirror
engine_common.h / engine.cpp; test_constants_have_not_drifted parses the two
files and fails when one of them moves.

Response tiers (a response blob is 16*(m+1) + kb + vb bytes for m rows with kb
sortkey bytes and vb user-data bytes):
  prefix    blob <= MG_OUT_PREFIX: it came back with the header
  tail      MG_OUT_PREFIX < blob <= MG_BLOB_BYTES: a second device read
  over_blob blob > MG_BLOB_BYTES: the fused lane hands back, general path
  over_row  a sortkey or a user datum above 65535 bytes: likewise
  over_rows more than MG_MAX_ROWS candidate records in the range: likewise
Request tiers (in_n = start key + stop key, with the extra NUL of an inclusive
stop, + filter pattern):
  graph     sizeof(MgGraphHdr) + in_n <= MG_GRAPH_IN: server and graph lanes
  pinned    in_n <= MG_IN_CAP: the pinned upload of the plain lane
  giant     above: pageable per-piece uploads
"""
import ctypes as C
from collections import namedtuple

from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import (FT_MATCH_ANYWHERE, FT_MATCH_POSTFIX, FT_MATCH_PREFIX,
                                        FT_NO_FILTER, MG_LANE_GENERAL, MG_LANE_GRAPH,
                                        MG_LANE_NONE, MG_LANE_SERVER, MG_LANE_SMALL,
                                        ROUTE_RANK_GLOBAL, ROUTE_RANK_GRP, ROUTE_RANK_LDS,
                                        ROUTE_RANK_LDST)

NOW = 1000

# ---- mirrored from engine_common.h / engine.cpp / kernels.hip ----
RRDB_MAX_RUNS = 64
LDST_MAXR = 32
MG_MAX_ROWS = 4096
MG_SCRATCH_BYTES = 1 << 20
MG_BLOB_BYTES = 2 * MG_SCRATCH_BYTES + 2 * (MG_MAX_ROWS + 1) * 8
MG_GRAPH_IN = 4096
MG_IN_CAP = 64 << 10
MG_OUT_PREFIX = 16 << 10
BLOB_STRIDE = 64 << 10   # rrdb_multi_get_batch: response bytes per request
BATCH_HK_MAX = 4096      # k_multi_get_batch stages [u16][hashkey] in LDS
ROW_MAX = 0xFFFF         # mg_core keeps row lengths in 16 bits
MG_ITER_COUNT = 3000     # rocksdb.multi_get_max_iteration_count default


class MgGraphHdr(C.Structure):
    """struct MgGraphHdr (engine_common.h): the request header of the graph
    and server lanes.  Mirrored so that sizeof comes from the layout."""
    _fields_ = [("start_len", C.c_uint32), ("stop_len", C.c_uint32),
                ("sk_pat_len", C.c_uint32),
                ("start_inclusive", C.c_uint8), ("stop_inclusive", C.c_uint8),
                ("reverse", C.c_uint8), ("no_value", C.c_uint8),
                ("max_kv_count", C.c_uint32), ("max_iteration_count", C.c_uint32),
                ("max_iteration_size", C.c_int64),
                ("sk_ft", C.c_int32),
                ("epoch_now", C.c_uint32), ("data_version", C.c_uint32),
                ("hash_key_skip", C.c_uint64)]


GRAPH_IN_MAX = MG_GRAPH_IN - C.sizeof(MgGraphHdr)  # largest in_n of the graph tier

# ---- the data set ----
N_DATA_RUNS = 4  # run 3 holds none of the sized hashkeys: the prefix bloom skips it
H_DEAD, H_GONE, H_LATE = b"\x01dead", b"\x01gone", b"\x01late"


def body_bytes(hk, i, n):
    """n bytes that depend on the hashkey, the row and the position"""
    off = (i * 37 + sum(hk[:8]) + len(hk)) % 251
    ramp = bytes(range(1, 252))
    return (ramp * ((off + n) // 251 + 1))[off:off + n]


def spread(hk, rows):
    """The physical records [(run, key, value, kind)] under which a full-range
    multi_get of hk returns exactly `rows` [(sortkey, body)], laid over runs
    0..2: row 0 shadows an older version, row 1 is a put over an older
    tombstone, every fifth row carries an unexpired TTL, and three hidden
    sortkeys add a tombstone over a put, an expired put, and an expired put
    over a live one."""
    out = []

    def put(run, sk, body, exp=0):
        out.append((run, D.generate_key(hk, sk), D.encode_value(body, exp, 0, 1), 0))

    def tomb(run, sk):
        out.append((run, D.generate_key(hk, sk), b"", 1))

    assert not {H_DEAD, H_GONE, H_LATE} & {sk for sk, _ in rows}
    for j, (sk, body) in enumerate(rows):
        if j == 0:
            put(0, sk, b"old")
            put(2, sk, body)
        elif j == 1:
            tomb(0, sk)
            put(1, sk, body)
        else:
            put(j % 3, sk, body, NOW + 100 if j % 5 == 4 else 0)
    put(0, H_DEAD, b"dead")
    tomb(2, H_DEAD)
    put(1, H_GONE, b"gone", 500)
    put(0, H_LATE, b"live")
    put(2, H_LATE, b"late", 500)
    return out


def hidden_records(n_rows):
    """physical records of spread() beyond one per row"""
    return 5 + (1 if n_rows >= 1 else 0) + (1 if n_rows >= 2 else 0)


def sized_rows(hk, blob, n, sk_len=4):
    """n rows whose response blob is exactly `blob` bytes"""
    sks = [b"s%0*d" % (sk_len - 1, i) for i in range(n)]
    vb = blob - 16 * (n + 1) - sum(len(s) for s in sks)
    assert vb >= 0
    base, extra = divmod(vb, n)
    rows = [(sk, body_bytes(hk, i, base + (1 if i < extra else 0))) for i, sk in enumerate(sks)]
    assert max(len(b) for _, b in rows) <= ROW_MAX
    return rows


def blob_bytes(kvs):
    """the response blob of a multi_get result, as the engine sizes it"""
    if not kvs:
        return 0
    return 16 * (len(kvs) + 1) + sum(len(k) + len(v) for k, v in kvs)


# hashkey -> visible rows of the full range
SIZED = {}
for _name, _blob in (("pm", MG_OUT_PREFIX - 1), ("pe", MG_OUT_PREFIX), ("pp", MG_OUT_PREFIX + 1)):
    SIZED[b"one-" + _name.encode()] = sized_rows(b"one-" + _name.encode(), _blob, 1)
    SIZED[b"many-" + _name.encode()] = sized_rows(b"many-" + _name.encode(), _blob, 100)
SIZED[b"k100"] = sized_rows(b"k100", 100 << 10, 10)
SIZED[b"bigfit"] = sized_rows(b"bigfit", MG_BLOB_BYTES, 33)
SIZED[b"bigover"] = sized_rows(b"bigover", MG_BLOB_BYTES + 1, 33)
SIZED[b"v65535"] = [(b"s000", body_bytes(b"v65535", 0, 65535))]
SIZED[b"v65536"] = [(b"s000", body_bytes(b"v65536", 0, 65536))]
SIZED[b"sk65535"] = [(body_bytes(b"sk65535", 1, 65535), b"small")]
SIZED[b"sk65536"] = [(body_bytes(b"sk65536", 1, 65536), b"small")]
SIZED[b"rows4096"] = [(b"r%05d" % i, b"%d" % i) for i in range(MG_MAX_ROWS - 7)]
SIZED[b"rows4097"] = [(b"r%05d" % i, b"%d" % i) for i in range(MG_MAX_ROWS - 6)]
SIZED[b"b64k"] = sized_rows(b"b64k", BLOB_STRIDE, 1)
SIZED[b"b64k1"] = sized_rows(b"b64k1", BLOB_STRIDE + 1, 1)
# request tiers: rows between long start and stop sortkeys
REQ_HK = b"reqhk"
SIZED[REQ_HK] = [(b"b%d" % i, b"req%d" % i) for i in range(6)]
HK_CAP = b"C" * (MG_IN_CAP // 2 - 2)      # in_n == MG_IN_CAP
HK_CAP1 = b"D" * (MG_IN_CAP // 2 - 1)     # in_n == MG_IN_CAP + 2
HK_GIANT = b"G" * 33000
for _hk in (HK_CAP, HK_CAP1, HK_GIANT):
    SIZED[_hk] = [(b"g%d" % i, b"giant%d" % i) for i in range(4)]
# batch: hashkey lengths and 0xFF endings
HK_L1, HK_L4096, HK_L4097 = b"k", b"L" * BATCH_HK_MAX, b"M" * (BATCH_HK_MAX + 1)
HK_FF = [b"\xff", b"a\xff\xff", b"\xff" * 255, b"\xff" * 256]
for _hk in [HK_L1, HK_L4096, HK_L4097] + HK_FF:
    SIZED[_hk] = [(b"f%d" % i, b"ff%d-" % i + _hk[:3]) for i in range(3)]
# neighbours right after the 0xFF hashkeys' stop keys: a next-blob that stops
# short, or does not carry, lets these rows into the range or loses the range
SIZED[b"\xff\x00"] = [(b"n0", b"after-ff")]
SIZED[b"a\xff\xff\x00"] = [(b"n0", b"after-aff")]
SIZED[b"b"] = [(b"n0", b"after-a")]
ORDINARY = [b"u%03d" % i for i in range(280)]
for _i, _hk in enumerate(ORDINARY):
    SIZED[_hk] = [(b"k%d" % j, body_bytes(_hk, j, 3 + (_i * 5 + j * 3) % 11))
                  for j in range(2 + _i % 4)]
MISS = b"nohk"
assert MISS not in SIZED


def build_runs():
    """[run0..run3], each a sorted list of (key, value, seq, kind); newer runs
    carry higher sequence numbers"""
    per_run = [dict() for _ in range(N_DATA_RUNS)]
    for hk, rows in SIZED.items():
        for run, key, val, kind in spread(hk, rows):
            assert key not in per_run[run]
            per_run[run][key] = (val, kind)
    # run 3: hashkeys of its own only
    for i in range(5):
        per_run[3][D.generate_key(b"zz-only-%d" % i, b"s")] = (D.encode_value(b"z", 0, 0, 1), 0)
    runs = []
    for r, recs in enumerate(per_run):
        runs.append([(k, recs[k][0], r * 10_000_000 + i + 1, recs[k][1])
                     for i, k in enumerate(sorted(recs))])
    return runs


# ---- the engine's view of a request, restated ----

def request_bounds(hk, kw):
    """(start, stop_excl, pattern) as multi_get_locked builds them"""
    assert kw.get("sort_key_filter_type", FT_NO_FILTER) != FT_MATCH_PREFIX
    start = D.generate_key(hk, kw.get("start_sortkey", b""))
    if kw.get("stop_sortkey", b""):
        stop = D.generate_key(hk, kw["stop_sortkey"])
        if kw.get("stop_inclusive", False):
            stop += b"\x00"
    else:
        stop = D.generate_next_blob(hk)
    return start, stop, kw.get("sort_key_filter_pattern", b"")


def in_n(hk, kw):
    return sum(len(x) for x in request_bounds(hk, kw))


def _filter_ok(ft, pat, sk):
    if ft == FT_NO_FILTER or not pat:
        return True
    if len(sk) < len(pat):
        return False
    if ft == FT_MATCH_ANYWHERE:
        return pat in sk
    return sk.endswith(pat) if ft == FT_MATCH_POSTFIX else sk.startswith(pat)


def candidates(runs, hk, kw):
    """(physical records in the range over all runs, whether a visible,
    unexpired, filter-passing row among them is too long for 16 bits)"""
    start, stop, pat = request_bounds(hk, kw)
    assert kw.get("start_inclusive", True)
    ft = kw.get("sort_key_filter_type", FT_NO_FILTER)
    n, newest = 0, {}
    for run in runs:
        for k, v, _, kind in run:
            if start <= k < stop:
                n += 1
                newest[k] = (v, kind)  # later runs overwrite
    oversize = False
    for k, (v, kind) in newest.items():
        if kind == 1:
            continue
        exp = D.decode_value(v, 1)[0]
        sk = k[2 + len(hk):]
        if (0 < exp <= NOW) or not _filter_ok(ft, pat, sk):
            continue
        if len(sk) > ROW_MAX or len(v) - D.value_header_len(1) > ROW_MAX:
            oversize = True
    return n, oversize


def response_tier(runs, hk, kw, kvs, blob_cap=MG_BLOB_BYTES):
    n, oversize = candidates(runs, hk, kw)
    if n > MG_MAX_ROWS:
        return "over_rows"
    if oversize:
        return "over_row"
    blob = blob_bytes(kvs)
    if blob > blob_cap:
        return "over_blob"
    return "tail" if blob > MG_OUT_PREFIX else "prefix"


def request_tier(hk, kw):
    n = in_n(hk, kw)
    return "graph" if n <= GRAPH_IN_MAX else ("pinned" if n <= MG_IN_CAP else "giant")


# ---- single-request cases ----
Case = namedtuple("Case", "name hk kw resp req")


def _single_cases():
    cs = []

    def add(name, hk, resp, req="graph", **kw):
        cs.append(Case(name, hk, kw, resp, req))

    for n in ("one", "many"):
        add(n + "-prefix-1", n.encode() + b"-pm", "prefix")
        add(n + "-prefix", n.encode() + b"-pe", "prefix")
        add(n + "-prefix+1", n.encode() + b"-pp", "tail")
        add(n + "-prefix+1-rev", n.encode() + b"-pp", "tail", reverse=True)
    large = [("k100", b"k100", "tail"), ("bigfit", b"bigfit", "tail"),
             ("bigover", b"bigover", "over_blob"), ("v65535", b"v65535", "tail"),
             ("v65536", b"v65536", "over_row"), ("sk65535", b"sk65535", "tail"),
             ("sk65536", b"sk65536", "over_row")]
    for name, hk, resp in large:
        add(name, hk, resp)
        add(name + "-rev", hk, resp, reverse=True)
        # no_value empties the values: only rows that are themselves too long
        # (checked before no_value applies) and the 64 KiB of sortkey stay large
        nv = resp if resp == "over_row" or hk == b"sk65535" else "prefix"
        add(name + "-novalue", hk, nv, no_value=True)
    # a size cap that stops inside the large hashkey: INCOMPLETE and a tail read
    add("k100-cut", b"k100", "tail", max_kv_size=50_000)
    add("k100-cut-rev", b"k100", "tail", max_kv_size=50_000, reverse=True)
    add("bigfit-cut", b"bigfit", "tail", max_kv_size=1_000_000)
    add("rows4096", b"rows4096", "tail")
    add("rows4097", b"rows4097", "over_rows")
    add("rows4097-rev", b"rows4097", "over_rows", reverse=True)
    add("miss", MISS, "prefix")
    add("ordinary", ORDINARY[7], "prefix")
    # request tiers: start + stop + pattern land exactly on the graph limit
    fixed = len(D.generate_key(REQ_HK)) * 2 + 1 + 1  # two prefixes, the NUL, the pattern
    l1 = 2000
    l2 = GRAPH_IN_MAX - fixed - l1
    rq = dict(start_sortkey=b"a" * l1, stop_inclusive=True,
              sort_key_filter_type=FT_MATCH_ANYWHERE, sort_key_filter_pattern=b"b")
    add("req-graph-max", REQ_HK, "prefix", "graph", stop_sortkey=b"c" * l2, **rq)
    add("req-graph-max+1", REQ_HK, "prefix", "pinned", stop_sortkey=b"c" * (l2 + 1), **rq)
    add("req-in-cap", HK_CAP, "prefix", "pinned")
    add("req-in-cap+2", HK_CAP1, "prefix", "giant")
    add("req-giant", HK_GIANT, "prefix", "giant")
    add("req-giant-rev", HK_GIANT, "prefix", "giant", reverse=True)
    return cs


SINGLE_CASES = _single_cases()
LANE_SETTINGS = {
    "server": {"engine.mg_persist": "on", "engine.mg_graph": "on"},
    "graph": {"engine.mg_persist": "off", "engine.mg_graph": "on"},
    "small": {"engine.mg_persist": "off", "engine.mg_graph": "off"},
}
FUSED_LANE = {"server": MG_LANE_SERVER, "graph": MG_LANE_GRAPH, "small": MG_LANE_SMALL}


def expected_lane(case, setting, n_runs=N_DATA_RUNS):
    """(lane, fused_first, tail_read) rrdb_last_multi_get_lane must report"""
    if n_runs == 0 or n_runs > RRDB_MAX_RUNS:
        return MG_LANE_GENERAL, MG_LANE_NONE, 0
    fused = FUSED_LANE[setting] if case.req == "graph" else MG_LANE_SMALL
    if case.resp in ("prefix", "tail"):
        return fused, MG_LANE_NONE, int(case.resp == "tail")
    return MG_LANE_GENERAL, fused, 0


# ---- batch cases ----
BATCH_SPECIAL = ([b"", HK_L1, HK_L4096, HK_L4097] + HK_FF +
                 [b"b64k", b"b64k1", b"rows4097", MISS, b"v65536", b"k100", b"a", b"\xff\xff"])
BATCH_VARIANTS = {
    "default": {},
    "reverse": dict(reverse=True),
    "no_value": dict(no_value=True),
    "count3": dict(max_kv_count=3),
    "size20": dict(max_kv_size=20),
    "postfix": dict(sort_key_filter_type=FT_MATCH_POSTFIX, sort_key_filter_pattern=b"3"),
}


def batch_requests():
    """~300 hashkeys: the special ones mixed in among ordinary ones"""
    reqs = list(ORDINARY)
    for i, hk in enumerate(BATCH_SPECIAL):
        reqs.insert(5 + i * 17, hk)
    return reqs


def batch_falls_back(runs, hk, kw, kvs):
    """does k_multi_get_batch hand this request to the per-request path?"""
    if len(hk) == 0 or len(hk) > BATCH_HK_MAX:
        return True
    return response_tier(runs, hk, kw, kvs, BLOB_STRIDE) not in ("prefix", "tail")


# every request here is answered by the batch kernel, so device-out delivers;
# body lengths are odd, so the packed regions do not start on 8-byte bounds
DEVICE_OUT_REQUESTS = ORDINARY[:40] + [MISS] + HK_FF + ORDINARY[40:60] + [b"b64k", HK_L4096]

# ---- run-count handles ----
RUN_COUNTS = (LDST_MAXR, LDST_MAXR + 1, RRDB_MAX_RUNS, RRDB_MAX_RUNS + 1)
RC_KEYS = 10
RC_FIXED_HK = b"hk0000"
RC_VAR_HKS = (b"a", b"bb", b"ccc")


def rc_key(shape, i):
    if shape == "fixed":  # 16-byte keys that share their first 8 bytes: word-probe eligible
        return D.generate_key(RC_FIXED_HK, b"s%07d" % i)
    return D.generate_key(RC_VAR_HKS[i % 3], b"v" * (i % 4) + b"%d" % i)


def rc_hashkeys(shape):
    return [RC_FIXED_HK] if shape == "fixed" else list(RC_VAR_HKS)


def rc_runs(shape, n_runs):
    """n_runs runs of three records over RC_KEYS keys: run r puts key r, buries
    key r+3 under a tombstone and puts key r+6 (expired TTL when r % 4 == 0,
    live TTL when r % 4 == 1).  Every key moves between put and tombstone as
    the run index grows, so what is visible depends on the newest runs."""
    runs = []
    for r in range(n_runs):
        exp = 500 if r % 4 == 0 else (NOW + 50 if r % 4 == 1 else 0)
        recs = {
            rc_key(shape, r % RC_KEYS): (D.encode_value(b"p%d" % r, 0, 0, 1), 0),
            rc_key(shape, (r + 3) % RC_KEYS): (b"", 1),
            rc_key(shape, (r + 6) % RC_KEYS): (D.encode_value(b"q%d" % r, exp, 0, 1), 0),
        }
        runs.append([(k, recs[k][0], r * 100 + i + 1, recs[k][1])
                     for i, k in enumerate(sorted(recs))])
    return runs


def expected_rank_route(shape, n_runs, mode):
    """the rank kernel rrdb_last_compact_route must report for a manual
    compaction of rc_runs(shape, n_runs) under engine.rank_mode = mode"""
    if mode == "lds":
        return ROUTE_RANK_LDS if n_runs <= RRDB_MAX_RUNS else ROUTE_RANK_GLOBAL
    if mode == "grp" and shape == "fixed" and n_runs <= LDST_MAXR:
        return ROUTE_RANK_GRP
    if mode == "ldst" and shape == "fixed":
        return ROUTE_RANK_LDST  # above LDST_MAXR the fallback is inside the kernel
    return ROUTE_RANK_GLOBAL


# reads of a run-count handle
RC_MULTI_GETS = {
    "full": {},
    "rev": dict(reverse=True),
    "count2": dict(max_kv_count=2),
    "range": dict(start_sortkey=b"s0000002", stop_sortkey=b"s0000007", stop_inclusive=True),
}
RC_SCAN = dict(start_key=b"\x00\x00", stop_key=b"\xff\xff", batch_size=3)

# ---- the sort-key prefix filter's clamp of both ends of the range ----
# A prefix filter narrows [start, stop) to the keys that carry the prefix
# before any lane sees the range (on_multi_get:558-578).  The filter itself
# hides what a missing clamp lets in, so rows alone do not show it: the
# iteration cap does.  The walk over a clamped range ends at the prefix's last
# key; over an unclamped one it goes on into the filtered keys behind it
# (forward), or starts among them (reverse), and runs into the cap.
PFX = b"p"
PFX_HK, PFX_HK_WIDE = b"pfx", b"pfx-wide"  # the second holds a row over ROW_MAX: general lane
PFX_BEFORE = [b"a%d" % i for i in range(4)]
PFX_IN = [b"p"] + [b"p%d" % i for i in range(9)] + [b"p\xff"]  # b"p" is the clamped start itself
PFX_AFTER = [b"q"] + [b"q%d" % i for i in range(4)] + [b"z"]    # b"q" is the clamped stop itself
PFX_ITERATED = len(PFX_IN) - 1          # p1's newest version is a tombstone
PFX_ITER_CAP = PFX_ITERATED + 2         # the clamped walk fits; two keys further does not


def pfx_runs():
    """two runs with overlapping keys: run 0 puts every sortkey of both
    hashkeys, run 1 lays newer puts over both bounds and tombstones, an
    expired and a live TTL over keys inside and outside the prefix"""
    run0, run1 = {}, {}
    for hk in (PFX_HK, PFX_HK_WIDE):
        for sk in PFX_BEFORE + PFX_IN + PFX_AFTER:
            run0[D.generate_key(hk, sk)] = (D.encode_value(b"old-" + sk, 0, 0, 1), 0)
        wide = body_bytes(hk, 8, ROW_MAX + 1) if hk == PFX_HK_WIDE else b"narrow"
        newer = {b"p": b"new-p", b"q": b"new-q", b"a1": b"new-a1", b"p8": wide}
        for sk, body in newer.items():
            run1[D.generate_key(hk, sk)] = (D.encode_value(body, 0, 0, 1), 0)
        for sk in (b"p1", b"q1"):
            run1[D.generate_key(hk, sk)] = (b"", 1)
        run1[D.generate_key(hk, b"p2")] = (D.encode_value(b"dead", 500, 0, 1), 0)
        run1[D.generate_key(hk, b"p3")] = (D.encode_value(b"ttl", NOW + 100, 0, 1), 0)
    return [[(k, recs[k][0], r * 1000 + i + 1, recs[k][1]) for i, k in enumerate(sorted(recs))]
            for r, recs in enumerate((run0, run1))]


def _pfx_cases():
    """a bound exactly on an existing key at each end, forward and reverse.
    whole_hashkey and its reverse are the ones that tell a missing stop clamp:
    the other shapes' own stop keys end the walk inside PFX_ITER_CAP anyway."""
    shapes = {
        "whole_hashkey": {},
        "start_on_bound_excl": dict(start_sortkey=b"p", start_inclusive=False),
        "stop_on_bound_incl": dict(stop_sortkey=b"q", stop_inclusive=True),
        "around": dict(start_sortkey=b"a2", stop_sortkey=b"q2", stop_inclusive=True),
    }
    flt = dict(sort_key_filter_type=FT_MATCH_PREFIX, sort_key_filter_pattern=PFX)
    return {name + ("-rev" if rev else ""): dict(kw, reverse=rev, **flt)
            for name, kw in shapes.items() for rev in (False, True)}


PFX_CASES = _pfx_cases()

# ---- scans (the device-resident output is read back on these) ----
SCAN_CASES = [dict(start_key=D.generate_key(b"u000"), stop_key=D.generate_key(b"u060"),
                   batch_size=bs, no_value=nv)
              for bs in (8, 1000) for nv in (False, True)]
SCAN_CASES.append(dict(start_key=b"\x00\x00", stop_key=b"\xff\xff", batch_size=1000,
                       no_value=False))
