"""The multi-run read view on every rank route and on bounded ranges.

Every read here happens before any compaction, so build_view (engine.cpp)
merges several runs: k_bounds, then k_rank_grp<1>, k_rank_ldst or k_rank (the
last two with no bound table, one level or two), then k_visible, the prefix
sum and k_gather.  tests/read_view_cases.py builds the data sets and ranges
that hand those kernels what a compaction never does: windows with lo != 0 and
hi < n, empty windows, an anchor run chosen per window, more groups than
launch_rank_grp_view has workgroups, a bound table on the read side.

Each read is compared three ways, byte for byte: engine == CPU oracle == a
plain dict merge of the input runs (keys, values, expire_ts, errors, context
ids).  After every engine read that builds a view, rrdb_last_view_route must
report the route, the table levels, the group count, the window size and the
row count that the case module restates from the data, so a view that
silently took another kernel fails here.  tests/test_read_view_model.py
checks on the CPU that the cases have the shapes their names claim.
"""
import pytest

import read_view_cases as RV
from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import (FT_MATCH_PREFIX, MG_LANE_GENERAL, OK, ROUTE_NONE,
                                        ROUTE_RANK_GLOBAL, ROUTE_RANK_GRP, ROUTE_RANK_LDST)
from read_view_cases import FIRST, LAST, NOW, Range
from rule_tables import open_part

pytestmark = pytest.mark.gpu

BIG = 2**31 - 1
ONE_WINDOW = {"rocksdb.max_iteration_count": str(BIG)}
MG_UNCAPPED = {"rocksdb.multi_get_max_iteration_count": str(BIG),
               "rocksdb.multi_get_max_iteration_size": str(BIG)}
RANK = {"grp": ROUTE_RANK_GRP, "ldst": ROUTE_RANK_LDST, "global": ROUTE_RANK_GLOBAL,
        "lds": ROUTE_RANK_GLOBAL}
FULL = Range("full", FIRST, LAST, True, False)

_ORACLE, _REF = {}, {}


@pytest.fixture(scope="module")
def reference(oracle_lib):
    """the oracle's answer to (data set, settings, read), computed once and
    shared by the engine configurations; fn runs the read on a handle"""
    def get(name, envs, key, fn):
        ekey = (name, tuple(sorted(envs.items())))
        if ekey + (key,) not in _REF:
            if ekey not in _ORACLE:
                o = open_part(oracle_lib)
                o.set_envs(envs)
                RV.ingest(o, name)
                _ORACLE[ekey] = o
            _REF[ekey + (key,)] = fn(_ORACLE[ekey])
        return _REF[ekey + (key,)]

    yield get
    for o in _ORACLE.values():
        o.close()
    _ORACLE.clear()
    _REF.clear()


def engine_of(hip_lib, name, mode, envs=None):
    g = open_part(hip_lib)
    g.set_envs(dict(envs or {}, **{"engine.rank_mode": mode}))
    RV.ingest(g, name)
    return g


def check_scan(g, reference, name, envs, rg, route, want=None, **kw):
    """one scan of the range on the engine: its batches equal the oracle's,
    their rows the dict merge's, and the view took `route` (None: the handler
    returned before it built one, and the report kept its value)"""
    before = g.last_view_route()
    got = RV.scan_batches(g, rg, **kw)
    ref = reference(name, envs, (rg, tuple(sorted(kw.items()))),
                    lambda o: RV.scan_batches(o, rg, **kw))
    assert len(got) == len(ref), (rg.name, kw)
    for n, (a, b) in enumerate(zip(got, ref)):
        assert a == b, (rg.name, kw, "batch %d" % n)
    assert g.last_view_route() == (before if route is None else route), (rg.name, kw)
    assert all(b[0] == OK for b in got) and got[-1][1] == -1
    if want is None:
        want = RV.expected_rows(name, rg)
    if kw.get("only_return_count"):
        assert sum(b[4] for b in got) == len(want), rg.name
    elif kw.get("return_expire_ts"):
        assert RV.rows_of_batches(got) == want, rg.name
    else:
        value = (lambda v: b"") if kw.get("no_value") else (lambda v: v)
        assert [kv for b in got for kv in b[2]] == [(k, value(v)) for k, v, _ in want], rg.name
    return got


# ---- the data sets --------------------------------------------------------

@pytest.mark.parametrize("name", list(RV.DATA))
def test_data_set_ingests(hip_lib, name):
    """the generated runs are valid tables for the engine (sorted, one run per
    ingest), nothing is merged before the first read, and no view was built.
    Run first, this also builds each data set once for the tests below."""
    runs = RV.runs_of(name)
    RV.merged(name)
    g = engine_of(hip_lib, name, "grp")
    try:
        assert g.num_runs() == len(runs) > 1
        assert g.num_records() == sum(len(r) for r in runs)
        assert g.last_view_route() == RV.ViewRoute(ROUTE_NONE, 0, 0, 0, 0)
    finally:
        g.close()


# ---- bounded ranges on the four rank modes --------------------------------

SLICES = 4  # the range table is dealt over this many test cases per mode


@pytest.mark.parametrize("part", list(range(SLICES)) + ["full"])
@pytest.mark.parametrize("mode", ["grp", "ldst", "global", "lds"])
def test_bounded_ranges(oracle_lib, hip_lib, reference, mode, part):
    """every range of the table through a paged scan, a one-window scan and a
    count.  grp: MODE 1 of k_rank_grp with lo != 0, the previous-segment test
    against s_lo, empty segments, the anchor run of the window; ldst: the
    no-table fallback inside k_rank_ldst; global and lds: k_rank.  (The full
    range, some 1800 pages of 7 rows, is a case of its own.)"""
    ranges = [rg for rg in RV.bounded_ranges() if (rg.name == "full") == (part == "full")]
    if part != "full":
        ranges = ranges[part::SLICES]
    g = engine_of(hip_lib, "bounded", mode)
    try:
        assert g.last_view_route().rank == ROUTE_NONE  # no view yet
        for rg in ranges:
            route = RV.scan_route("bounded", mode, rg)
            if route is not None:
                assert route.rank == (RANK[mode] if route.window_records else ROUTE_NONE)
                assert route.bound_levels == 0
            check_scan(g, reference, "bounded", {}, rg, route, batch_size=7,
                       return_expire_ts=True)
        g.set_envs(ONE_WINDOW)
        for rg in ranges:
            route = RV.scan_route("bounded", mode, rg)
            got = check_scan(g, reference, "bounded", ONE_WINDOW, rg, route, batch_size=BIG,
                             return_expire_ts=True)
            assert len(got) == 1
            got = check_scan(g, reference, "bounded", ONE_WINDOW, rg, route, batch_size=BIG,
                             only_return_count=True)
            assert len(got) == 1
    finally:
        g.close()


# ---- sortkey_count and the general lane of multi_get ----------------------

@pytest.mark.parametrize("part", range(SLICES))
@pytest.mark.parametrize("mode", ["grp", "ldst"])
def test_bounded32_count_and_general_multi_get(oracle_lib, hip_lib, reference, mode, part):
    """32-byte keys under one hashkey: sortkey_count builds the view of the
    hashkey, and a range multi_get over more than MG_MAX_ROWS candidate rows
    is handed back by the fused lane and builds a bounded one."""
    name = "bounded32"
    g = engine_of(hip_lib, name, mode)
    try:
        g.set_envs(MG_UNCAPPED)
        full = RV.expected_rows(name, FULL)
        got = g.sortkey_count(RV.HK32, NOW)
        assert got == reference(name, MG_UNCAPPED, "count",
                                lambda o: o.sortkey_count(RV.HK32, NOW)) == (OK, len(full))
        stop = D.generate_next_blob(RV.HK32)
        route = RV.expected_route(name, mode, D.generate_key(RV.HK32), stop)
        assert g.last_view_route() == route and route.rank == RANK[mode]
        for rg in RV.mg_ranges()[part::SLICES]:
            sr = RV.mg_scan_range(rg)
            want = [(k[18:], v) for k, v, _ in RV.expected_rows(name, sr)]
            route = RV.expected_route(name, mode, sr.start, RV.stop_excl(sr))
            assert route.rank == RANK[mode] and route.window_records > 4096
            for reverse in (False, True):
                kw = dict(start_sortkey=rg.start, stop_sortkey=rg.stop,
                          start_inclusive=rg.start_inclusive, stop_inclusive=rg.stop_inclusive,
                          reverse=reverse)
                got = g.multi_get(RV.HK32, NOW, **kw)
                ref = reference(name, MG_UNCAPPED, ("mg", rg, reverse),
                                lambda o: o.multi_get(RV.HK32, NOW, **kw))
                assert got == ref == (OK, want), (rg.name, reverse)
                assert g.last_multi_get_lane().lane == MG_LANE_GENERAL, rg.name
                assert g.last_view_route() == route, (rg.name, reverse)
        # the same ranges as scans: full keys, 32-byte stride
        for rg in RV.bounded_ranges(32)[part::3 * SLICES]:
            check_scan(g, reference, name, MG_UNCAPPED, rg, RV.scan_route(name, mode, rg),
                       batch_size=7, return_expire_ts=True)
    finally:
        g.close()


# ---- more groups than workgroups ------------------------------------------

def _mvg_engine(hip_lib):
    g = engine_of(hip_lib, "many_view_groups", "grp")
    g.set_envs(ONE_WINDOW)
    return g


def _mvg_route(rg):
    route = RV.scan_route("many_view_groups", "grp", rg)
    assert route.rank == ROUTE_RANK_GRP
    return route


def test_many_view_groups_full_drain(oracle_lib, hip_lib, reference):
    """3685 groups on 3584 workgroups: the first 101 workgroups rank a second
    group, and those second groups hold the overwritten ids, the tombstones
    and the boundary-split key sets.  One window: the prefix sum and the
    cutoff run over more than 4096 entries."""
    g = _mvg_engine(hip_lib)
    try:
        route = _mvg_route(FULL)
        assert RV.GRP_VIEW_BLOCKS < route.n_groups == RV.MVG_GROUPS
        got = check_scan(g, reference, "many_view_groups", ONE_WINDOW, FULL, route,
                         batch_size=BIG)
        assert len(got) == 1 and len(got[0][2]) > 100_000
    finally:
        g.close()


def test_many_view_groups_paged_expire_ts(oracle_lib, hip_lib, reference):
    g = _mvg_engine(hip_lib)
    try:
        got = check_scan(g, reference, "many_view_groups", ONE_WINDOW, FULL, _mvg_route(FULL),
                         batch_size=1000, return_expire_ts=True)
        assert len(got) > 100
    finally:
        g.close()


@pytest.mark.parametrize("which", ["late", "long_3", "long_50"])
def test_many_view_groups_bounded_ranges(oracle_lib, hip_lib, reference, which):
    """ranges that start at a key every run holds: six inside the groups a
    workgroup ranks second, two that leave more than GRP_VIEW_BLOCKS groups in
    a window whose lo is not 0"""
    ranges = [rg for rg in RV.mvg_ranges() if rg.name.startswith(which)]
    assert len(ranges) == (6 if which == "late" else 1)
    g = _mvg_engine(hip_lib)
    try:
        for rg in ranges:
            route = _mvg_route(rg)
            assert (route.n_groups > RV.GRP_VIEW_BLOCKS) == (which != "late")
            check_scan(g, reference, "many_view_groups", ONE_WINDOW, rg, route, batch_size=BIG,
                       return_expire_ts=True)
    finally:
        g.close()


# ---- the bound table on the read side -------------------------------------

BT_CONFIGS = [("ldst", 5, 2), ("ldst", 8, 1), ("global", 5, 2), ("global", 8, 1), ("grp", 5, 0)]


# one drained range per test case: the full range, the window that starts just
# before the cluster, the six above the threshold, the three just under it
BT_RANGES = ["full", "before"] + ["over%d" % n for n in range(6)] + \
    ["under%d" % n for n in range(3)]


def _bt_range(which):
    over, under, _ = RV.bt_fixed_ranges()
    table = dict({"full": FULL, "before": RV.bt_before_cluster_range()},
                 **{"over%d" % n: rg for n, rg in enumerate(over)},
                 **{"under%d" % n: rg for n, rg in enumerate(under)})
    assert sorted(table) == sorted(BT_RANGES)
    return table[which]


@pytest.mark.parametrize("which", BT_RANGES)
@pytest.mark.parametrize("mode,shift,levels", BT_CONFIGS,
                         ids=["%s-bt%d" % c[:2] for c in BT_CONFIGS])
def test_bt_fixed(oracle_lib, hip_lib, reference, mode, shift, levels, which):
    """windows above VIEW_BT_MIN_RECORDS: k_rank_ldst stages through a one- or
    two-level table (one block over LDST_CAP, blocks across both run
    boundaries), k_rank searches through it, the group rank takes none; just
    under the threshold the same kernels run without a table.  Every range is
    drained in one window."""
    name = "bt_fixed"
    rg = _bt_range(which)
    under = which.startswith("under")
    g = engine_of(hip_lib, name, mode, {"engine.bt_shift": str(shift)})
    try:
        g.set_envs(ONE_WINDOW)
        route = RV.scan_route(name, mode, rg, shift)
        assert (route.rank, route.bound_levels) == (RANK[mode], 0 if under else levels)
        assert (route.window_records > RV.VIEW_BT_MIN_RECORDS) == (not under)
        got = check_scan(g, reference, name, ONE_WINDOW, rg, route, batch_size=BIG,
                         return_expire_ts=True)
        assert len(got) == 1 and len(got[0][2]) > 80_000
    finally:
        g.close()


@pytest.mark.parametrize("read", ["rows", "no_value", "hash_key_prefix"])
def test_bt_var_variable_length_keys(oracle_lib, hip_lib, reference, read):
    """no tail words: the default mode falls to k_rank, whose table and
    searches read whole keys through koff (several hashkey lengths, keys that
    are strict prefixes of keys in other runs)"""
    name = "bt_var"
    g = open_part(hip_lib)
    try:
        g.set_envs(ONE_WINDOW)
        RV.ingest(g, name)
        route = RV.expected_route(name, "grp", FIRST, LAST)
        assert (route.rank, route.bound_levels) == (ROUTE_RANK_GLOBAL, 2)
        if read == "rows":
            check_scan(g, reference, name, ONE_WINDOW, FULL, route, batch_size=BIG,
                       return_expire_ts=True)
        elif read == "no_value":
            check_scan(g, reference, name, ONE_WINDOW, FULL, route, batch_size=BIG,
                       no_value=True)
        else:
            want = [r for r in RV.expected_rows(name, FULL)
                    if D.restore_key(r[0])[0].startswith(RV.BT_VAR_PREFIX)]
            clamp = RV.expected_route(name, "grp", D.generate_key(RV.BT_VAR_PREFIX), LAST)
            got = check_scan(g, reference, name, ONE_WINDOW, FULL, clamp, want=want,
                             batch_size=BIG, hash_key_filter_type=FT_MATCH_PREFIX,
                             hash_key_filter_pattern=RV.BT_VAR_PREFIX)
            assert len(got[0][2]) == len(want) > 1000
    finally:
        g.close()


@pytest.mark.parametrize("mode", ["ldst", "global"])
def test_route_boundary(oracle_lib, hip_lib, reference, mode):
    """a window of exactly VIEW_BT_MIN_RECORDS records takes no table, one
    record more takes one, and both return the same rows where they overlap"""
    name = "bt_fixed"
    _, _, edge = RV.bt_fixed_ranges()
    g = engine_of(hip_lib, name, mode)
    try:
        g.set_envs(ONE_WINDOW)
        rows = []
        for rg, total in zip(edge, (RV.VIEW_BT_MIN_RECORDS, RV.VIEW_BT_MIN_RECORDS + 1)):
            route = RV.scan_route(name, mode, rg)
            assert route.window_records == total and route.rank == RANK[mode]
            got = check_scan(g, reference, name, ONE_WINDOW, rg, route, batch_size=BIG,
                             return_expire_ts=True)
            rows.append(RV.rows_of_batches(got))
            levels = g.last_view_route().bound_levels
            assert levels == 0 if total == RV.VIEW_BT_MIN_RECORDS else levels >= 1
        lo, hi = max(e.start for e in edge), min(e.stop for e in edge)
        a, b = ([r for r in rs if lo <= r[0] < hi] for rs in rows)
        assert a == b and len(a) > 80_000
    finally:
        g.close()
