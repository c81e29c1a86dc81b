"""The cases of tests/read_view_cases.py on the CPU: no GPU.

  - the CPU oracle against a plain dict merge of the input runs (the highest
    run wins per key, tombstones and expired rows go, sorted, sliced by the
    range) on every data set and range, and tests/pymodel.py as a third voice
    on the two small sets.  The GPU file compares the engine with both; this
    pins them to one another first.
  - the cases are what they claim: every named range has the property its
    name states and every data set the shape the GPU tests rely on, from the
    data alone, so that a later edit of the data cannot hollow them out.
  - test_constants_have_not_drifted: the limits the case module mirrors are
    the ones in engine_common.h, kernels.hip and engine.cpp.
"""
import os
import re

import pytest

import read_view_cases as RV
from conftest import REPO
from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import (FT_MATCH_PREFIX, OK, ROUTE_NONE, ROUTE_RANK_GLOBAL,
                                        ROUTE_RANK_GRP, ROUTE_RANK_LDST)
from pymodel import Model
from read_view_cases import LAST, FIRST, NOW, Range
from rule_tables import open_part

CSRC = os.path.join(REPO, "incubator_pegasus_amd", "csrc")
BIG = 2**31 - 1

_ORACLES = {}


@pytest.fixture(scope="module")
def oracles(oracle_lib):
    """one oracle handle per data set, ingested on first use"""
    def get(name):
        if name not in _ORACLES:
            o = open_part(oracle_lib)
            o.set_envs({"rocksdb.max_iteration_count": str(BIG),
                        "rocksdb.multi_get_max_iteration_count": str(BIG),
                        "rocksdb.multi_get_max_iteration_size": str(BIG)})
            RV.ingest(o, name)
            _ORACLES[name] = o
        return _ORACLES[name]

    yield get
    for o in _ORACLES.values():
        o.close()
    _ORACLES.clear()


def _oracle_rows(o, rg):
    batches = RV.scan_batches(o, rg, batch_size=BIG, return_expire_ts=True)
    assert [b[:2] for b in batches] == [(OK, -1)], rg.name
    return RV.rows_of_batches(batches)


# ---------------- the oracle against the dict merge ----------------

@pytest.mark.parametrize("name,klen", [("bounded", 18), ("bounded32", 32)])
def test_bounded_oracle_vs_merge_vs_model(oracles, name, klen):
    o = oracles(name)
    m = Model()
    for run in RV.runs_of(name):
        m.ingest(run)
    m.visible_items = _cached_visible(m)
    for rg in RV.bounded_ranges(klen):
        want = RV.expected_rows(name, rg)
        assert _oracle_rows(o, rg) == want, rg.name
        err, batches = m.scan(NOW, start_key=rg.start, stop_key=rg.stop,
                              start_inclusive=rg.start_inclusive,
                              stop_inclusive=rg.stop_inclusive, batch_size=BIG,
                              max_iteration_count=BIG, validate_hash_req=False,
                              return_expire_ts=True)
        assert err == OK and len(batches) == 1
        assert [(k, v, e) for (k, v), e in zip(batches[0][0], batches[0][1] or [])] == want, \
            rg.name
        # paged: the batches add up to the same rows
        paged = RV.scan_batches(o, rg, batch_size=7, return_expire_ts=True)
        assert RV.rows_of_batches(paged) == want, rg.name
        count = RV.scan_batches(o, rg, batch_size=BIG, only_return_count=True)
        assert [(b[0], b[1], b[4]) for b in count] == [(OK, -1, len(want))], rg.name


def _cached_visible(model):
    """pymodel's visible list of the whole table, built once, sliced per call"""
    import bisect

    rows = Model.visible_items(model)
    keys = [k for k, _ in rows]

    def visible_items(lo=None, hi=None, lo_incl=True, hi_incl=False):
        a = 0 if lo is None else (bisect.bisect_left if lo_incl else bisect.bisect_right)(keys, lo)
        z = len(keys) if hi is None else \
            (bisect.bisect_right if hi_incl else bisect.bisect_left)(keys, hi)
        return rows[a:z]

    return visible_items


def test_bounded32_multi_get_and_count_oracle_vs_merge(oracles):
    o = oracles("bounded32")
    full = RV.expected_rows("bounded32", Range("full", FIRST, LAST, True, False))
    assert o.sortkey_count(RV.HK32, NOW) == (OK, len(full))
    for rg in RV.mg_ranges():
        want = [(k[18:], v) for k, v, _ in RV.expected_rows("bounded32", RV.mg_scan_range(rg))]
        for reverse in (False, True):
            got = o.multi_get(RV.HK32, NOW, start_sortkey=rg.start, stop_sortkey=rg.stop,
                              start_inclusive=rg.start_inclusive,
                              stop_inclusive=rg.stop_inclusive, reverse=reverse)
            assert got == (OK, want), (rg.name, reverse)


@pytest.mark.parametrize("name", ["many_view_groups", "bt_fixed", "bt_var"])
def test_large_sets_oracle_vs_merge(oracles, name):
    o = oracles(name)
    ranges = [Range("full", FIRST, LAST, True, False)]
    if name == "many_view_groups":
        ranges += RV.mvg_ranges()
    elif name == "bt_fixed":
        over, under, edge = RV.bt_fixed_ranges()
        ranges += over[:2] + under[:1] + edge
    for rg in ranges:
        assert _oracle_rows(o, rg) == RV.expected_rows(name, rg), rg.name
    if name == "bt_var":
        rg = Range("full", FIRST, LAST, True, False)
        want = RV.expected_rows(name, rg)
        got = RV.scan_batches(o, rg, batch_size=BIG, no_value=True)
        assert got[0][2] == [(k, b"") for k, _, _ in want]
        got = RV.scan_batches(o, rg, batch_size=BIG, hash_key_filter_type=FT_MATCH_PREFIX,
                              hash_key_filter_pattern=RV.BT_VAR_PREFIX)
        want = [(k, v) for k, v, _ in want if D.restore_key(k)[0].startswith(RV.BT_VAR_PREFIX)]
        assert got[0][2] == want and len(want) > 1000


# ---------------- the cases are what they claim ----------------

def _win(name, rg):
    return RV.windows(RV.keys_of(name), rg.start, RV.stop_excl(rg))


@pytest.mark.parametrize("name,klen", [("bounded", 18), ("bounded32", 32)])
def test_bounded_cases_are_what_they_claim(name, klen):
    runs, keys = RV.runs_of(name), RV.keys_of(name)
    assert len(runs) == RV.BOUNDED_R and all(len(k[0]) == klen for k in keys)
    assert 10_000 <= sum(len(r) for r in runs) <= 15_000
    assert all(max(len(v) for _, v, _, _ in run) == 12 + RV.USER_LEN for run in runs)
    n = [len(k) for k in keys]
    assert RV.anchor_run([0] * 8, n) == RV.BOUNDED_ANCHOR_RUN == 3  # in the middle
    # the full view: staged groups, one group over GRP_CAP
    sizes = RV.group_sizes(keys, [0] * 8, n)
    assert len(sizes) == 41 and sum(sizes) == sum(n) and sizes[-1] == 1
    assert sizes[RV.G_OVER] > RV.GRP_CAP and sum(s > RV.GRP_CAP for s in sizes) == 1
    assert sizes[RV.G_STAGED] == 128 + 300 and sizes[16] == 128 + 1900 <= RV.GRP_CAP
    P = RV.placement_keys(klen)
    for g in RV.BOUNDED_DUPS:
        assert RV.in_every_run(name, RV.key_of(RV.anchor_id(g), klen))
    assert RV.in_every_run(name, P["dup"]) and not RV.newest_is_tombstone(name, P["dup"])
    assert RV.in_every_run(name, P["tomb"]) and RV.newest_is_tombstone(name, P["tomb"])
    # the tombstone buries older puts, and an expired put hides live ones
    assert all(run[keys[r].index(P["tomb"])][3] == 0 for r, run in enumerate(runs[:7]))
    dead = RV.key_of(RV.anchor_id(12), klen)
    assert D.decode_value(runs[7][keys[7].index(dead)][1])[0] == NOW - 10
    for kind in ("anchor", "anchor_prev", "anchor_next"):
        assert P[kind] in keys[3] and sum(P[kind] in k for k in keys) == 1
    assert not any(P[kind] in k for k in keys for kind in ("anchor_below", "anchor_above"))
    merged = RV.merged(name)
    assert any(kind == 1 for _, _, kind in merged)
    assert any(kind == 0 and 0 < D.decode_value(v)[0] <= NOW for _, v, kind in merged)
    assert len(merged) < sum(n) - 500  # overwritten versions

    R = {rg.name: rg for rg in RV.bounded_ranges(klen)}
    assert len(R) == len(RV.bounded_ranges(klen))
    for kind in P:
        for rg, key in ((R["start_%s_incl" % kind], "start"), (R["start_%s_excl" % kind], "start"),
                        (R["stop_%s_incl" % kind], "stop"), (R["stop_%s_excl" % kind], "stop")):
            assert getattr(rg, key) == P[kind]
            lo, hi = _win(name, rg)
            assert sum(hi) - sum(lo) > 300 and min(lo) > 0
        assert R["start_%s_excl" % kind].start_inclusive is False
        assert R["stop_%s_incl" % kind].stop_inclusive is True
    # an exclusive start at a key whose newest version is a tombstone: the
    # view's first row is another key, and nothing may be skipped
    rg = R["start_tomb_excl"]
    rows = RV.expected_rows(name, rg)
    assert rows and rows[0][0] > P["tomb"]
    assert rows == RV.expected_rows(name, rg._replace(start_inclusive=True))
    assert len(RV.expected_rows(name, R["start_dup_incl"])) == \
        len(RV.expected_rows(name, R["start_dup_excl"])) + 1
    assert len(RV.expected_rows(name, R["stop_dup_incl"])) == \
        len(RV.expected_rows(name, R["stop_dup_excl"])) + 1
    assert RV.expected_rows(name, R["stop_tomb_incl"]) == RV.expected_rows(name, R["stop_tomb_excl"])
    # points and empties
    assert len(RV.expected_rows(name, R["point_anchor_incl"])) == 1
    assert len(RV.expected_rows(name, R["point_dup_incl"])) == 1
    for nm in ("point_tomb_incl", "point_anchor_below_incl", "before_first", "beyond_last",
               "after_last", "reversed", "point_anchor_excl", "point_dup_open"):
        assert RV.expected_rows(name, R[nm]) == [], nm
    for nm in ("point_anchor_excl", "point_anchor_open", "reversed"):
        assert RV.range_is_empty(R[nm]) and RV.scan_route(name, "grp", R[nm]) is None
    for nm in ("before_first", "beyond_last", "point_anchor_below_incl"):
        assert RV.scan_route(name, "grp", R[nm]).rank == ROUTE_NONE, nm
    assert RV.scan_route(name, "grp", R["after_last"]).window_records == 1
    assert len(RV.expected_rows(name, R["up_to_first"])) == 1
    assert RV.scan_route(name, "grp", R["from_last"]).window_records == 1
    # groups and windows
    lo, hi = _win(name, R["inside_staged_group"])
    assert RV.group_sizes(keys, [0] * 8, n)[RV.G_STAGED] > sum(hi) - sum(lo) > 100
    assert min(lo) > 0 and max(RV.group_sizes(keys, lo, hi)) <= RV.GRP_CAP
    lo, hi = _win(name, R["inside_oversized_group"])
    bounds = RV.group_bounds(keys, [0] * 8, n)
    assert all(bounds[RV.G_OVER][q] <= lo[q] and hi[q] <= bounds[RV.G_OVER + 1][q]
               for q in range(8))
    assert sum(hi) - sum(lo) > 1500
    lo, hi = _win(name, R["oversized_group_in_window"])
    sizes = RV.group_sizes(keys, lo, hi)
    assert RV.anchor_run(lo, hi) == 3 and min(lo) > 0
    assert len(sizes) == 3 and sizes[1] > RV.GRP_CAP and sizes[0] <= RV.GRP_CAP
    for nm, q0 in (("newest_run_anchors", 7), ("oldest_run_anchors", 0)):
        lo, hi = _win(name, R[nm])
        assert RV.anchor_run(lo, hi) == q0 and hi[q0] - lo[q0] == 300
        assert sum(h == l for l, h in zip(lo, hi)) >= 2  # empty windows
        assert len(RV.group_sizes(keys, lo, hi)) == 3
    lo, hi = _win(name, R["two_groups_dup_to_tomb"])
    assert RV.group_sizes(keys, lo, hi)[:2] == [128 + 7, 128]
    # the routes of the four modes
    for rg in RV.bounded_ranges(klen):
        if RV.range_is_empty(rg):
            continue
        lo, hi = _win(name, rg)
        total = sum(hi) - sum(lo)
        for mode, rank in (("grp", ROUTE_RANK_GRP), ("ldst", ROUTE_RANK_LDST),
                           ("global", ROUTE_RANK_GLOBAL), ("lds", ROUTE_RANK_GLOBAL)):
            rt = RV.scan_route(name, mode, rg)
            assert rt.window_records == total and rt.bound_levels == 0
            assert rt.rank == (rank if total else ROUTE_NONE)
            assert rt.n_groups == (len(RV.group_sizes(keys, lo, hi))
                                   if total and mode == "grp" else 0)
            assert rt.visible == len({k for k, _, kind in RV.merged(name)
                                      if kind == 0 and rg.start <= k < RV.stop_excl(rg)})


def test_mg_ranges_are_what_they_claim():
    from mg_lane_cases import MG_MAX_ROWS

    names = [rg.name for rg in RV.mg_ranges()]
    assert len(set(names)) == len(names) >= 16
    for rg in RV.mg_ranges():
        sr = RV.mg_scan_range(rg)
        lo, hi = RV.windows(RV.keys_of("bounded32"), sr.start, RV.stop_excl(sr))
        assert sum(hi) - sum(lo) > MG_MAX_ROWS, rg.name  # the fused lanes hand it back
        if rg.name not in ("whole_hashkey", "start_first_incl", "start_first_excl"):
            assert sum(lo) > 0 or sum(hi) < sum(len(k) for k in RV.keys_of("bounded32"))
    tomb = RV.placement_keys(32)["tomb"][18:]
    assert {rg.stop for rg in RV.mg_ranges() if rg.name.startswith("stop_tomb")} == {tomb}


def test_many_view_groups_is_what_it_claims():
    keys = RV.keys_of("many_view_groups")
    n = [len(k) for k in keys]
    assert len(keys) == RV.MVG_R == 32 and RV.gs_of(32) == 5
    assert RV.anchor_run([0] * 32, n) == RV.MVG_ANCHOR_RUN
    assert n[16] == RV.GRP_VIEW_BLOCKS * 32 + 32 * 100 + 1
    assert max(n[:16] + n[17:]) < 1000 and 110_000 < sum(n) < 130_000
    bounds = RV.group_bounds(keys, [0] * 32, n)
    sizes = [sum(b1) - sum(b0) for b0, b1 in zip(bounds, bounds[1:])]
    assert RV.GRP_VIEW_BLOCKS < len(sizes) == RV.MVG_GROUPS < 2 * RV.GRP_VIEW_BLOCKS
    assert max(sizes) <= RV.GRP_CAP
    shadowed = split = 0
    for g in range(RV.GRP_VIEW_BLOCKS, len(sizes)):
        mine = [k for q in range(32) for k in keys[q][bounds[g][q]:bounds[g + 1][q]]]
        shadowed += len(set(mine)) < len(mine)
        # the anchor key's newer versions closed the previous group
        first = keys[16][bounds[g][16]]
        split += any(bounds[g][q] > 0 and keys[q][bounds[g][q] - 1] == first
                     for q in range(17, 32))
    assert shadowed >= 50 and split >= 5
    late = RV.merged("many_view_groups")
    cut = RV.mvg_key(RV.GRP_VIEW_BLOCKS)
    assert any(kind == 1 for k, _, kind in late if k >= cut)
    ranges = RV.mvg_ranges()
    assert len(ranges) == 8
    for rg in ranges:
        assert RV.in_every_run("many_view_groups", rg.start)
        lo, hi = _win("many_view_groups", rg)
        rt = RV.scan_route("many_view_groups", "grp", rg)
        assert rt.rank == ROUTE_RANK_GRP and min(lo) > 0
        if rg.name.startswith("late"):
            assert rg.start >= cut and rg.stop > rg.start and rt.n_groups >= 2
        else:
            assert rt.n_groups > RV.GRP_VIEW_BLOCKS


def test_bt_fixed_is_what_it_claims():
    keys = RV.keys_of("bt_fixed")
    n = [len(k) for k in keys]
    assert tuple(n) == RV.BT_SIZES and all(x % 256 for x in n)
    assert sum(n) > RV.VIEW_BT_MIN_RECORDS and (max(n) >> 11) > 8
    # blocks straddle both run boundaries
    assert n[0] % RV.BLOCK and (n[0] + n[1]) % RV.BLOCK
    merged = RV.merged("bt_fixed")
    assert 0.08 < (sum(n) - len(merged)) / len(merged) < 0.12
    dels = sum(r[3] for run in RV.runs_of("bt_fixed") for r in run)
    assert 0.02 < dels / sum(n) < 0.04
    # the cluster: consecutive keys of run 2 between two neighbours of run 0
    i = keys[0].index(RV.key_of(RV.bt_id(RV.BT_J0)))
    assert keys[0][i + 1] == RV.key_of(RV.bt_id(RV.BT_J0 + 1))
    a, z = (RV.bisect.bisect_left(keys[2], keys[0][i + x]) for x in (0, 1))
    assert z - a == RV.BT_CLUSTER and keys[2][a] == RV.bt_cluster_key(0)
    assert RV.bisect.bisect_left(keys[1], keys[0][i]) == RV.bisect.bisect_left(keys[1],
                                                                               keys[0][i + 1])
    for shift, levels in ((5, 2), (8, 1)):
        totals = RV.ldst_block_totals(keys, [0] * 3, n, shift)
        assert len(totals) == (sum(n) + 255) // 256
        assert sum(t > RV.LDST_CAP for t in totals) >= 1
        assert sum(t <= RV.LDST_CAP for t in totals) >= 0.9 * len(totals)
        assert min(totals) == 0  # inside the cluster the other runs hold nothing
        assert RV.bound_levels([0] * 3, n, shift) == levels
    over, under, edge = RV.bt_fixed_ranges()
    assert len(over) == 6 and len(under) == 3 and len(edge) == 2
    cl0, cl1 = RV.bt_cluster_key(0), RV.bt_cluster_key(RV.BT_CLUSTER - 1)
    for rg in over + under + edge:
        assert cl0 <= rg.start <= cl1
    for rg in over:
        for mode, rank in (("ldst", ROUTE_RANK_LDST), ("global", ROUTE_RANK_GLOBAL)):
            for shift, levels in ((5, 2), (8, 1)):
                rt = RV.scan_route("bt_fixed", mode, rg, shift)
                assert (rt.rank, rt.bound_levels) == (rank, levels)
                assert rt.window_records > RV.VIEW_BT_MIN_RECORDS
        rt = RV.scan_route("bt_fixed", "grp", rg)
        assert (rt.rank, rt.bound_levels) == (ROUTE_RANK_GRP, 0) and rt.n_groups > 100
    # a block across a run boundary wants the end of the third run for its
    # first records and the start for its last: over the cap as well.  In a
    # window that starts inside the cluster these are the only ones (run 0's
    # first record lies beyond the cluster); the full range and the window
    # that starts just before the cluster, with lo != 0, have the block of
    # run 0 that spans the cluster too
    def over_cap(rg, shift):
        lo, hi = _win("bt_fixed", rg)
        totals = RV.ldst_block_totals(keys, lo, hi, shift)
        assert sum(t <= RV.LDST_CAP for t in totals) >= 0.9 * len(totals)
        ends = (hi[0] - lo[0], hi[0] - lo[0] + hi[1] - lo[1])
        straddle = {e // RV.BLOCK for e in ends if e % RV.BLOCK}
        assert len(straddle) == 2
        return {b for b, t in enumerate(totals) if t > RV.LDST_CAP}, straddle

    for shift in (5, 8):
        got, straddle = over_cap(over[0], shift)
        assert got == straddle
        for rg in (Range("full", FIRST, LAST, True, False), RV.bt_before_cluster_range()):
            got, straddle = over_cap(rg, shift)
            assert got > straddle and min(got) == 0
    lo, hi = _win("bt_fixed", RV.bt_before_cluster_range())
    assert min(lo) > 0 and sum(hi) - sum(lo) > RV.VIEW_BT_MIN_RECORDS
    for rg in under:
        rt = RV.scan_route("bt_fixed", "ldst", rg)
        assert rt.bound_levels == 0 and rt.rank == ROUTE_RANK_LDST
        assert RV.VIEW_BT_MIN_RECORDS - 300 < rt.window_records < RV.VIEW_BT_MIN_RECORDS
    assert [RV.scan_route("bt_fixed", "ldst", rg).window_records for rg in edge] == \
        [RV.VIEW_BT_MIN_RECORDS, RV.VIEW_BT_MIN_RECORDS + 1]
    assert [RV.scan_route("bt_fixed", "ldst", rg).bound_levels for rg in edge] == [0, 2]
    a, b = (RV.expected_rows("bt_fixed", rg) for rg in edge)
    assert len(set(a) & set(b)) > 80_000


def test_bt_var_is_what_it_claims():
    keys = RV.keys_of("bt_var")
    n = [len(k) for k in keys]
    assert len(keys) == 4 and sum(n) > RV.VIEW_BT_MIN_RECORDS and (max(n) >> 11) > 8
    lens = {len(k) for ks in keys for k in ks}
    assert len(lens) > 10
    assert {len(D.restore_key(k)[0]) for k in keys[0]} == {6, 8, 12}
    # a key and a strict prefix of it, in different runs
    where = {}
    for r, ks in enumerate(keys):
        for k in ks:
            where.setdefault(k, set()).add(r)
    pairs = [(k, k2) for k in where if k.endswith(b"pre")
             for k2 in (k + b"\x00", k + b"fix", k + b"\xff") if k2 in where]
    assert len(pairs) == RV.BT_VAR_PAIRS
    assert all(where[a].isdisjoint(where[b]) for a, b in pairs)
    assert max(len(v) for run in RV.runs_of("bt_var") for _, v, _, _ in run) <= 12 + 16
    rt = RV.expected_route("bt_var", "grp", FIRST, LAST)
    assert (rt.rank, rt.bound_levels, rt.n_groups) == (ROUTE_RANK_GLOBAL, 2, 0)
    clamp = D.generate_key(RV.BT_VAR_PREFIX)
    assert RV.expected_route("bt_var", "grp", clamp, LAST) == rt  # the filter's start clamp


# ---------------- the mirrored constants ----------------

def test_constants_have_not_drifted():
    common = open(os.path.join(CSRC, "engine_common.h")).read()
    kernels = open(os.path.join(CSRC, "kernels.hip")).read()
    engine = open(os.path.join(CSRC, "engine.cpp")).read()

    def define(src, name):
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, src, re.M)
        assert m, name
        return int(m.group(1))

    for name in ("VIEW_BT_MIN_RECORDS", "GRP_VIEW_BLOCKS", "GRP_CAP", "GRP_TARGET", "LDST_MAXR"):
        assert define(common, name) == getattr(RV, name), name
    for name in ("LDST_CAP", "BLOCK", "WAVE"):
        assert define(kernels, name) == getattr(RV, name), name
    # the names are what build_view and the view launch use: build_view hands
    # the threshold to prepare_rank, which compares the window with it
    view = engine[engine.index("DevView build_view("):]
    assert re.search(r"prepare_rank\(dr, 0, R, [^;]*\bVIEW_BT_MIN_RECORDS, true\);", view)
    assert "if (total > bt_min_records)" in engine
    launch = kernels[kernels.index("void launch_rank_grp_view("):]
    launch = launch[:launch.index("k_rank_grp<1>")]
    assert "blocks > GRP_VIEW_BLOCKS" in launch and "blocks = GRP_VIEW_BLOCKS" in launch
    assert re.search(r"int bt_shift = %d;" % RV.BT_SHIFT_DEFAULT, engine)
    assert "int cshift = bt_shift + 6;" in engine and "(wmax >> cshift) > 8" in engine
    # gs_of restates grp_shift, which build_anchors and the count scan call
    assert "while ((1ull << (gs + 1)) * (uint64_t)R <= GRP_TARGET && gs < 8)" in engine
    assert [RV.gs_of(R) for R in (2, 3, 8, 32)] == [8, 8, 7, 5]
    # the route numbering and the report's layout, as capi.py mirrors them
    ext = open(os.path.join(REPO, "include", "rrdb_engine_ext.h")).read()
    from incubator_pegasus_amd import capi
    for name in ("NONE", "RANK_GLOBAL", "RANK_LDST", "RANK_GRP"):
        assert re.search(r"\bRRDB_ROUTE_%s\s*=\s*%d\b" % (name, getattr(capi, "ROUTE_" + name)),
                         ext), name
    struct = re.search(r"typedef struct \{([^}]*)\} rrdb_view_route;", ext).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = [tuple(d.split()) for d in struct.split(";") if d.strip()]
    ctype = {"int32_t": capi.C.c_int32, "uint64_t": capi.C.c_uint64}
    assert [(n, ctype[t]) for t, n in fields] == list(capi._ViewRoute._fields_)
