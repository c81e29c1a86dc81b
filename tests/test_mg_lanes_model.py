"""The case table of tests/mg_lane_cases.py on the CPU: no GPU.

  - the CPU oracle against the independent Python restatement
    (tests/pymodel.py) on every case: multi_get, the batch as N singles, scan,
    and the reads and compaction stats of the run-count handles.  The GPU file
    compares the engine with the oracle; this pins the oracle.
  - test_cases_are_what_they_claim: from the oracle's own results, every case
    lands in the tier its name says and every tier has a case.
  - test_constants_have_not_drifted: the limits the case table mirrors are the
    ones in engine_common.h, engine.cpp and kernels.hip.
"""
import ctypes as C
import os
import re

import pytest

import mg_lane_cases as MC
from conftest import REPO
from incubator_pegasus_amd.capi import INCOMPLETE, OK
from mg_lane_cases import NOW
from pymodel import Model
from test_minor_compact_model import stats_dict
from test_scan_differential import _drain_batches

CSRC = os.path.join(REPO, "incubator_pegasus_amd", "csrc")


class CachedModel(Model):
    """pymodel.Model over a data set that no longer changes: the whole-table
    visible list, which every multi_get rebuilds, is built once."""

    def visible_items(self, lo=None, hi=None, lo_incl=True, hi_incl=False):
        key = (lo, hi, lo_incl, hi_incl)
        if key != (None, None, True, True):
            return Model.visible_items(self, lo, hi, lo_incl, hi_incl)
        if getattr(self, "_all", None) is None:
            self._all = Model.visible_items(self, None, None, True, True)
        return self._all


@pytest.fixture(scope="module")
def data(oracle_lib):
    runs = MC.build_runs()
    o = oracle_lib.open(1, 0, -1)
    m = CachedModel()
    for r in runs:
        o.ingest_run(r)
        m.ingest(r)
    yield runs, o, m
    o.close()


# ---------------- the oracle against the model ----------------

def test_multi_get_oracle_vs_model(data):
    _, o, m = data
    for c in MC.SINGLE_CASES:
        assert o.multi_get(c.hk, NOW, **c.kw) == m.multi_get(c.hk, NOW, **c.kw), c.name


@pytest.mark.parametrize("variant", sorted(MC.BATCH_VARIANTS))
def test_batch_oracle_vs_singles_vs_model(data, variant):
    _, o, m = data
    kw = MC.BATCH_VARIANTS[variant]
    reqs = MC.batch_requests()
    err, groups = o.multi_get_batch(reqs, NOW, **kw)
    assert err == OK and len(groups) == len(reqs)
    for hk, got in zip(reqs, groups):
        single = o.multi_get(hk, NOW, **kw)
        assert got == single, hk[:16]
        assert single == m.multi_get(hk, NOW, **kw), hk[:16]


@pytest.mark.parametrize("case", range(len(MC.SCAN_CASES)))
def test_scan_oracle_vs_model(data, case):
    _, o, m = data
    kw = MC.SCAN_CASES[case]
    assert _drain_batches(o, kw, 1000) == m.scan(NOW, max_iteration_count=1000,
                                                 validate_hash_req=False, **kw)


def rc_reads(p, shape):
    """every read of a run-count handle, in one comparable value"""
    keys = [MC.rc_key(shape, i) for i in range(MC.RC_KEYS + 2)]
    hks = MC.rc_hashkeys(shape) + [b"absent"]
    out = {"get": [p.get(k, NOW) for k in keys], "ttl": [p.ttl(k, NOW) for k in keys],
           "batch_get": p.batch_get(keys, NOW),
           "sortkey_count": [p.sortkey_count(hk, NOW) for hk in hks]}
    for name, kw in MC.RC_MULTI_GETS.items():
        out["multi_get-" + name] = [p.multi_get(hk, NOW, **kw) for hk in hks]
    out["scan"] = _drain_batches(p, MC.RC_SCAN, 1000)
    return out


def model_rc_reads(m, shape):
    keys = [MC.rc_key(shape, i) for i in range(MC.RC_KEYS + 2)]
    hks = MC.rc_hashkeys(shape) + [b"absent"]
    out = {"get": [m.get(k, NOW) for k in keys], "ttl": [m.ttl(k, NOW) for k in keys],
           "batch_get": m.batch_get(keys, NOW),
           "sortkey_count": [(OK, m.sortkey_count(hk, NOW)) for hk in hks]}
    for name, kw in MC.RC_MULTI_GETS.items():
        out["multi_get-" + name] = [m.multi_get(hk, NOW, **kw) for hk in hks]
    out["scan"] = m.scan(NOW, max_iteration_count=1000, validate_hash_req=False, **MC.RC_SCAN)
    return out


@pytest.mark.parametrize("n_runs", MC.RUN_COUNTS)
@pytest.mark.parametrize("shape", ["fixed", "var"])
def test_run_count_handles_oracle_vs_model(oracle_lib, shape, n_runs):
    o = oracle_lib.open(1, 0, -1)
    try:
        m = Model()
        for r in MC.rc_runs(shape, n_runs):
            o.ingest_run(r)
            m.ingest(r)
        assert o.num_runs() == n_runs
        assert rc_reads(o, shape) == model_rc_reads(m, shape)
        err, st = o.manual_compact(NOW)
        assert err == OK and stats_dict(st) == m.compact_full(NOW)[1]
        assert rc_reads(o, shape) == model_rc_reads(m, shape)
    finally:
        o.close()


ITER_COUNT_ENV = "rocksdb.multi_get_max_iteration_count"


def test_prefix_clamp_oracle_vs_model(oracle_lib):
    """the prefix-clamp cases: the oracle against the model, and the cases
    are what they claim: under PFX_ITER_CAP a walk over the clamped range
    completes with every row of the prefix, keys lie behind the prefix for a
    longer walk to run into, and the cap is tight enough to tell"""
    runs = MC.pfx_runs()
    assert len(runs) == 2 and all(len(r) <= 200 for r in runs)
    assert {k for k, _, _, _ in runs[0]} > {k for k, _, _, _ in runs[1]}  # overlapping keys
    o = oracle_lib.open(1, 0, -1)
    try:
        m = Model()
        for r in runs:
            o.ingest_run(r)
            m.ingest(r)
        for hk in (MC.PFX_HK, MC.PFX_HK_WIDE):
            rows = m.multi_get(hk, NOW, **MC.PFX_CASES["whole_hashkey"])[1]
            assert len(rows) == MC.PFX_ITERATED - 1  # all but the expired one
            assert rows[0][0] == MC.PFX and rows[-1][0] == MC.PFX_IN[-1]
            assert len(m.multi_get(hk, NOW, start_sortkey=b"q")[1]) > 2  # behind the prefix
            for cap in (MC.PFX_ITER_CAP, MC.MG_ITER_COUNT):
                o.set_envs({ITER_COUNT_ENV: str(cap)})
                for name, kw in MC.PFX_CASES.items():
                    want = m.multi_get(hk, NOW, engine_max_iter=cap, **kw)
                    assert o.multi_get(hk, NOW, **kw) == want, (hk, cap, name)
                    excl = name.startswith("start_on_bound_excl")
                    assert want == (OK, rows[1:] if excl else rows), (hk, cap, name)
            # the cap is what tells: one short of it, the walk no longer fits
            short = m.multi_get(hk, NOW, engine_max_iter=MC.PFX_ITERATED - 1,
                                **MC.PFX_CASES["whole_hashkey"])
            assert short[0] == INCOMPLETE
        wide = m.multi_get(MC.PFX_HK_WIDE, NOW, **MC.PFX_CASES["whole_hashkey"])[1]
        assert max(len(v) for _, v in wide) == MC.ROW_MAX + 1
    finally:
        o.close()


# ---------------- the cases are what their names say ----------------

def test_cases_are_what_they_claim(data):
    runs, o, _ = data
    assert len(runs) == MC.N_DATA_RUNS >= 4
    # every sized hashkey lies in runs 0, 1 and 2 and not in run 3
    for hk in MC.SIZED:
        lo, hi = MC.D.generate_key(hk), MC.D.generate_next_blob(hk)
        present = [any(lo <= k < hi for k, _, _, _ in run) for run in runs]
        assert present == [True, True, True, False], hk[:16]
    # what spread() hides and shows, on one hashkey
    hk = MC.ORDINARY[3]
    err, kvs = o.multi_get(hk, NOW)
    assert (err, kvs) == (OK, MC.SIZED[hk]) and len(kvs) == 5
    assert MC.candidates(runs, hk, {})[0] == len(kvs) + MC.hidden_records(len(kvs))
    for sk in (MC.H_DEAD, MC.H_GONE, MC.H_LATE):
        assert o.get(MC.D.generate_key(hk, sk), NOW)[0] != OK
    assert o.ttl(MC.D.generate_key(hk, kvs[4][0]), NOW) == (OK, 100)

    # single requests: response tier, request tier, and the exact sizes
    seen = set()
    blobs = {}
    for c in MC.SINGLE_CASES:
        err, kvs = o.multi_get(c.hk, NOW, **c.kw)
        assert err in (OK, INCOMPLETE), c.name
        assert MC.response_tier(runs, c.hk, c.kw, kvs) == c.resp, c.name
        assert MC.request_tier(c.hk, c.kw) == c.req, c.name
        blobs[c.name] = (MC.blob_bytes(kvs), err, len(kvs))
        seen.add((c.resp, c.req))
    P, B = MC.MG_OUT_PREFIX, MC.MG_BLOB_BYTES
    for n in ("one", "many"):
        assert [blobs[n + s][0] for s in ("-prefix-1", "-prefix", "-prefix+1")] == \
            [P - 1, P, P + 1]
        assert blobs[n + "-prefix"][2] == (1 if n == "one" else 100)
    assert abs(blobs["k100"][0] - (100 << 10)) < 64
    assert blobs["bigfit"][0] == B and blobs["bigover"][0] == B + 1
    assert blobs["bigfit"][2] in range(33, 36)
    assert blobs["bigfit"][0] < (30 << 20)  # the iteration-size cap is far away
    assert blobs["v65535"][0] == 32 + 4 + 65535 and blobs["v65536"][0] == 32 + 4 + 65536
    assert blobs["sk65535"][0] == 32 + 65535 + 5 and blobs["sk65536"][0] == 32 + 65536 + 5
    for name in ("k100", "bigfit", "bigover", "v65535"):
        assert blobs[name + "-novalue"][0] <= P, name
        assert blobs[name + "-rev"] == blobs[name], name
    for name in ("k100-cut", "k100-cut-rev", "bigfit-cut"):
        blob, err, m = blobs[name]
        assert err == INCOMPLETE and blob > P and 0 < m < blobs[name.split("-")[0]][2], name
    assert MC.candidates(runs, b"rows4096", {})[0] == MC.MG_MAX_ROWS
    assert MC.candidates(runs, b"rows4097", {})[0] == MC.MG_MAX_ROWS + 1
    # the iteration cap cuts it; the two expired hidden rows are iterated too
    assert blobs["rows4096"][1:] == (INCOMPLETE, MC.MG_ITER_COUNT - 2)
    assert blobs["miss"] == (0, OK, 0)
    by = {c.name: c for c in MC.SINGLE_CASES}
    hdr = C.sizeof(MC.MgGraphHdr)
    assert hdr + MC.in_n(by["req-graph-max"].hk, by["req-graph-max"].kw) == MC.MG_GRAPH_IN
    assert hdr + MC.in_n(by["req-graph-max+1"].hk, by["req-graph-max+1"].kw) == \
        MC.MG_GRAPH_IN + 1
    assert MC.in_n(MC.HK_CAP, {}) == MC.MG_IN_CAP and MC.in_n(MC.HK_CAP1, {}) == MC.MG_IN_CAP + 2
    assert MC.in_n(MC.HK_GIANT, {}) > MC.MG_IN_CAP
    for name in ("req-graph-max", "req-graph-max+1", "req-in-cap", "req-in-cap+2", "req-giant"):
        assert blobs[name][1] == OK and blobs[name][2] > 0, name
    # every tier has a case, and the three request tiers meet a prefix response
    assert {r for r, _ in seen} == {"prefix", "tail", "over_blob", "over_row", "over_rows"}
    assert {q for r, q in seen if r == "prefix"} == {"graph", "pinned", "giant"}
    # the lane table: each fused lane is expected somewhere, with and without
    # a tail read, and each is expected to hand back somewhere
    exp = {(s,) + MC.expected_lane(c, s) for c in MC.SINGLE_CASES for s in MC.LANE_SETTINGS}
    for s, lane in MC.FUSED_LANE.items():
        assert (s, lane, MC.MG_LANE_NONE, 0) in exp and (s, lane, MC.MG_LANE_NONE, 1) in exp
        assert (s, MC.MG_LANE_GENERAL, lane, 0) in exp

    # batch: the special hashkeys, and what each variant must do
    reqs = MC.batch_requests()
    assert 290 <= len(reqs) <= 310 and len(set(reqs)) == len(reqs)
    assert {len(h) for h in reqs} >= {0, 1, MC.BATCH_HK_MAX, MC.BATCH_HK_MAX + 1, 255, 256}
    for h in MC.HK_FF:
        assert h.endswith(b"\xff") and o.multi_get(h, NOW) == (OK, MC.SIZED[h])
    assert MC.D.generate_next_blob(b"\xff" * 255) == b"\x01"  # the carry reaches the length
    assert MC.D.generate_next_blob(b"\xff" * 256) == b"\x01\x01"
    assert MC.blob_bytes(o.multi_get(b"b64k", NOW)[1]) == MC.BLOB_STRIDE
    assert MC.blob_bytes(o.multi_get(b"b64k1", NOW)[1]) == MC.BLOB_STRIDE + 1
    for variant, kw in MC.BATCH_VARIANTS.items():
        res = [o.multi_get(h, NOW, **kw) for h in reqs]
        fb = [MC.batch_falls_back(runs, h, kw, r[1]) for h, r in zip(reqs, res)]
        assert 3 <= sum(fb) <= 12, variant
        # fallbacks lie among fused requests, not at one end
        idx = [i for i, f in enumerate(fb) if f]
        assert idx[0] > 0 and idx[-1] < len(reqs) - 1 and idx[-1] - idx[0] > 100, variant
        full = [o.multi_get(h, NOW) for h in reqs]
        if variant in ("count3", "size20"):
            cut = [r for r, f in zip(res, full) if r[0] == INCOMPLETE and 0 < len(r[1]) < len(f[1])]
            assert len(cut) > 50, variant
        if variant == "postfix":
            assert any(0 < len(r[1]) < len(f[1]) for r, f in zip(res, full))
            assert all(k.endswith(b"3") for r in res for k, _ in r[1])
    fb = {h: MC.batch_falls_back(runs, h, {}, o.multi_get(h, NOW)[1]) for h in reqs}
    assert [h for h in MC.BATCH_SPECIAL if fb[h]] == \
        [b"", MC.HK_L4097, b"b64k1", b"rows4097", b"v65536", b"k100"]
    # device-out: all fused, a zero-row request, regions off the 8-byte grid
    dres = [o.multi_get(h, NOW) for h in MC.DEVICE_OUT_REQUESTS]
    assert not any(MC.batch_falls_back(runs, h, {}, r[1])
                   for h, r in zip(MC.DEVICE_OUT_REQUESTS, dres))
    assert dres[MC.DEVICE_OUT_REQUESTS.index(MC.MISS)] == (OK, [])
    off, offs = 0, []
    for _, kvs in dres:
        offs.append(off)
        off += 16 * (len(kvs) + 1) + sum(len(k) + len(v) for k, v in kvs)
    assert sum(1 for x in offs if x % 8) > 10

    # scan cases: more than one page, and a page that is not full
    for kw in MC.SCAN_CASES:
        err, batches = _drain_batches(o, kw, 1000)
        assert err == OK and sum(len(b[0]) for b in batches) > 0
        if 0 < kw["batch_size"] < 100:
            assert len(batches) > 3 and len(batches[-1][0]) not in (0, kw["batch_size"])

    # run-count handles: the counts straddle both limits; keys cross the
    # newest run, as a put over older records and as a tombstone over a put
    assert MC.RUN_COUNTS == (MC.LDST_MAXR, MC.LDST_MAXR + 1, MC.RRDB_MAX_RUNS,
                             MC.RRDB_MAX_RUNS + 1)
    for shape in ("fixed", "var"):
        for n in MC.RUN_COUNTS:
            rr = MC.rc_runs(shape, n)
            assert len(rr) == n and all(3 <= len(r) <= 4 for r in rr)
            lens = {len(k) for r in rr for k, _, _, _ in r}
            assert (lens == {16}) if shape == "fixed" else (len(lens) > 2)
            if shape == "fixed":
                assert len({k[:8] for r in rr for k, _, _, _ in r}) == 1
            older = {}
            for r in rr[:-1]:
                for k, _, _, kind in r:
                    older[k] = kind
            last = {k: kind for k, _, _, kind in rr[-1]}
            assert any(kind == 0 and k in older for k, kind in last.items())
            assert any(kind == 1 and older.get(k) == 0 for k, kind in last.items())
    routes = {(s, n, md): MC.expected_rank_route(s, n, md) for s in ("fixed", "var")
              for n in MC.RUN_COUNTS for md in ("grp", "ldst", "lds", "global")}
    assert routes[("fixed", MC.LDST_MAXR, "grp")] == MC.ROUTE_RANK_GRP
    assert routes[("fixed", MC.LDST_MAXR + 1, "grp")] != MC.ROUTE_RANK_GRP
    assert routes[("fixed", MC.RRDB_MAX_RUNS, "lds")] == MC.ROUTE_RANK_LDS
    assert all(v != MC.ROUTE_RANK_LDS for (s, n, md), v in routes.items()
               if n > MC.RRDB_MAX_RUNS)


# ---------------- the mirrored constants ----------------

def _c_int(expr, names):
    expr = re.sub(r"\b(\d+)(?:ull|ul|u|ll)\b", r"\1", expr.strip().rstrip(";"))
    assert re.fullmatch(r"[\w\s()<>*+\-]+", expr), expr
    return int(eval(expr, {"__builtins__": {}}, dict(names)))  # arithmetic on mirrored names


def test_constants_have_not_drifted():
    common = open(os.path.join(CSRC, "engine_common.h")).read()
    engine = open(os.path.join(CSRC, "engine.cpp")).read()
    kernels = open(os.path.join(CSRC, "kernels.hip")).read()
    names = {}
    for name in ("RRDB_MAX_RUNS", "LDST_MAXR", "MG_MAX_ROWS", "MG_SCRATCH_BYTES",
                 "MG_BLOB_BYTES", "MG_GRAPH_IN"):
        m = re.search(r"^#define\s+%s\s+(.+?)\s*(?:/\*.*)?$" % name, common, re.M)
        assert m, name
        names[name] = _c_int(m.group(1), names)
        assert names[name] == getattr(MC, name), name
    for name in ("MG_IN_CAP", "MG_OUT_PREFIX"):
        m = re.search(r"static constexpr uint64_t %s = ([^;]+);" % name, engine)
        assert m and _c_int(m.group(1), names) == getattr(MC, name), name
    m = re.findall(r"const uint64_t BLOB_STRIDE = ([^;]+);", engine)
    assert len(m) == 1 and _c_int(m[0], names) == MC.BLOB_STRIDE
    # the batch kernel's staged hashkey and the server's copy of the prefix size
    assert re.search(r"s_start\[2 \+ %d\], s_stop\[2 \+ %d\]" % ((MC.BATCH_HK_MAX,) * 2), kernels)
    assert re.search(r"hl == 0 \|\| hl > %d\b" % MC.BATCH_HK_MAX, kernels)
    assert "kl - hash_key_skip > 0xFFFF || vl - hdr > 0xFFFF" in kernels
    assert re.search(r"uint8_t resp\[32 \+ \(16 << 10\)\];", common)
    assert re.search(r"mg_max_iter_count = %d\b" % MC.MG_ITER_COUNT, engine)
    # struct MgGraphHdr, field by field
    body = re.search(r"struct MgGraphHdr \{(.*?)\};", common, re.S).group(1)
    ctype = {"uint32_t": C.c_uint32, "uint8_t": C.c_uint8, "int64_t": C.c_int64,
             "int32_t": C.c_int32, "uint64_t": C.c_uint64}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            t, rest = decl.split(None, 1)
            fields += [(n.strip(), ctype[t]) for n in rest.split(",")]
    assert fields == list(MC.MgGraphHdr._fields_)
    assert MC.GRAPH_IN_MAX == MC.MG_GRAPH_IN - C.sizeof(MC.MgGraphHdr) > 0
    # the lane numbering, as capi.py mirrors it
    ext = open(os.path.join(REPO, "include", "rrdb_engine_ext.h")).read()
    from incubator_pegasus_amd import capi
    for name in ("NONE", "POINT_LIST", "SERVER", "GRAPH", "SMALL", "GENERAL"):
        assert re.search(r"\bRRDB_MG_LANE_%s\s*=\s*%d\b" % (name, getattr(capi, "MG_LANE_" + name)),
                         ext), name
    struct = re.search(r"typedef struct \{([^}]*)\} rrdb_multi_get_lane;", ext).group(1)
    decl = re.findall(r"\b(int32_t|uint64_t)\s+(\w+);", struct)
    assert [(n, ctype[t]) for t, n in decl] == list(capi._MultiGetLane._fields_)

