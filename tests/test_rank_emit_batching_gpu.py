"""The batched loads of the group rank (k_rank_grp) and of the fused
fixed-stride emit (k_emit_fixed_fused) at the sizes where their schedules
change.

The rank kernel stages a group flat: thread t owns staged positions
t + 256 k, k < ceil(gsize / 256) <= 8, and loads the tail and meta words of all
of them before it waits (incubator_pegasus_amd/csrc/grp_stage.h).  The emit
copies 16-byte chunks in batches of EMIT_COPY_DEPTH * 256 with a remainder
loop, and other strides a row per thread (emit_tile.h).  The run records both
kernels read come from a table in LDS.

Every case ingests the same seeded runs into the CPU oracle and the engine,
compacts both, and compares the stats, a full scan of keys, values and expire
timestamps, and sampled point gets, byte for byte, and checks the route.

Placing a group: the anchor run (the largest) gives a group 2^gs of its
records, the other runs whatever they hold between the same anchor keys.  The
anchor run holds the ids a * SP; a group's other records get ids strictly
between its first two anchor ids, so the case fixes each group's size.
group_sizes() restates the engine's anchor rule, and the CPU test at the end
checks every case's claimed sizes with it.

The CPU half also runs tools/grp_stage_check.cpp as __graft_entry__.build()
built it.
"""
import bisect
import json
import os
import random
import subprocess

import pytest

from conftest import REPO
from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import (OK, ROUTE_EMIT_CHUNKED, ROUTE_EMIT_CHUNKED_FIXED,
                                        ROUTE_NONE, ROUTE_RANK_GLOBAL, ROUTE_RANK_GRP)
from rule_tables import SMT_PREFIX, open_part, ops_json, pattern_rule
from test_fused_emit_gpu import NOW, T, ingest, make_value, rows_of
from test_fused_emit_gpu import build_runs as plan_runs
from test_fused_emit_gpu import make_key as plan_key
from test_grp_rank import _count_fused_or_fallback, _drain
from test_minor_compact_gpu import _same_full_compact, _window_case
from test_minor_compact_model import build_model, delete_rule_env, fixed_key, stats_dict

gpu = pytest.mark.gpu

SP = 4096            # id spacing of the anchor run's keys
GRP_CAP = 2048       # staged group size limit (8 slots of 256)
COPY_BATCH = 4 * 256  # EMIT_COPY_DEPTH * EMIT_THREADS chunks per full batch


def gs_of(R):
    """build_anchors (engine.cpp): log2 of the anchor records per group"""
    gs = 4
    while (1 << (gs + 1)) * R <= 1024 and gs < 8:
        gs += 1
    return gs


def key_of(i, klen=18):
    """tail-word eligible keys: only the last 8 bytes vary (i < 10^8)"""
    if klen == 18:
        return D.generate_key(b"u:%014d" % i, b"")
    return D.generate_key(b"u:" + b"0" * 14, b"s%013d" % i)  # 32 bytes


def grouped_runs(R, n_anchor, extras, anchor_run=0, seed=1, klen=18, user_len=100, version=1,
                 kinds=("put",) * 16 + ("ttl", "ttl", "dead", "del"), boundary_dups=(),
                 vary_len=False, sp=SP):
    """R record lists, oldest first.  Run `anchor_run` holds ids a * SP for
    a < n_anchor (SP = sp here).  extras[g] is a count, dealt round-robin over the other
    runs, or a list of R - 1 counts, one per other run in run order: that many
    records with ids between the first two anchor ids of group g; about one in
    eight of them repeats an id another run already holds there (an
    overwritten version).  Every other run also holds one id between anchors
    0 and 1, so no run is empty.  boundary_dups: groups whose first anchor key
    every other run holds too (an equal-key set split at the group boundary).
    """
    G = 1 << gs_of(R)
    rnd = random.Random(seed * 7919 + R)
    others = [r for r in range(R) if r != anchor_run]
    ids = [set() for _ in range(R)]
    assert n_anchor * sp < 10**8  # beyond 8 digits the keys lose their tail-word eligibility
    ids[anchor_run] = {a * sp for a in range(n_anchor)}
    for s, r in enumerate(others):
        ids[r].add(1 + s)
    for g, spec in sorted(extras.items()):
        counts = spec if isinstance(spec, list) else \
            [spec // len(others) + (s < spec % len(others)) for s in range(len(others))]
        assert len(counts) == len(others) and sum(counts) + R < sp
        base = g * G * sp + (R if g == 0 else 1)
        used, nxt = [], 0
        for s, c in enumerate(counts):
            mine = set()
            dups = rnd.sample(used, min(c // 8, len(used)))
            mine.update(dups)
            while len(mine) < c:
                mine.add(base + nxt)
                used.append(base + nxt)
                nxt += 1
            ids[others[s]].update(mine)
    for g in boundary_dups:
        for r in others:
            ids[r].add(g * G * sp)
    runs = []
    for r in range(R):
        recs = []
        for n, i in enumerate(sorted(ids[r])):
            seq = r * 10_000_000 + n + 1  # a newer run's seqnos lie above the older run's
            what = "put" if n == 0 else rnd.choice(kinds)  # every run has a PUT stride
            ulen = user_len + (i % 5 if vary_len else 0)
            expire = {"ttl": NOW + 500, "dead": NOW - 10}.get(what, 0)
            val = b"" if what == "del" else make_value(i, seq, ulen, expire, version)
            recs.append((key_of(i, klen), val, seq, 1 if what == "del" else 0))
        runs.append(recs)
    return runs


def group_sizes(runs):
    """k_anchor_rows restated: run q's boundary for group g is the first
    record not below the anchor key, and for runs newer than the anchor run
    the first above it (equal keys in newer runs rank before the anchor)"""
    R = len(runs)
    gs = gs_of(R)
    q0 = max(range(R), key=lambda r: (len(runs[r]), -r))
    keys = [[rec[0] for rec in run] for run in runs]
    n_groups = max(1, (len(keys[q0]) + (1 << gs) - 1) >> gs)
    bounds = [[0] * R]
    for g in range(1, n_groups):
        k = keys[q0][g << gs]
        bounds.append([g << gs if q == q0 else
                       (bisect.bisect_right if q > q0 else bisect.bisect_left)(keys[q], k)
                       for q in range(R)])
    bounds.append([len(k) for k in keys])
    return [sum(b1) - sum(b0) for b0, b1 in zip(bounds, bounds[1:])]


# ---- the data sets --------------------------------------------------------

def _slots_extras():
    """R = 8, gs = 7: one group of each staged size the slot schedule turns
    on, the fallback size, and the empty / lopsided segment shapes"""
    G = 128
    ex = {1: 255 - G, 2: 256 - G, 3: 257 - G, 4: 1024 - G, 5: 1793 - G, 6: 2047 - G,
          7: 2048 - G, 8: 2049 - G}
    ex[9] = [0, 0, 300, 0, 0, 0, 0]      # 6 of 8 runs hold nothing here
    ex[10] = [0, 0, 0, 0, 1500, 0, 0]    # one run supplies all but 2^gs
    return ex


SLOT_SIZES = {1: 255, 2: 256, 3: 257, 4: 1024, 5: 1793, 6: 2047, 7: 2048, 8: 2049,
              9: 128 + 300, 10: 128 + 1500}
SLOTS_N_ANCHOR = 40 * 128 + 1  # the last group is one record


def slots_runs(**kw):
    return grouped_runs(8, SLOTS_N_ANCHOR, _slots_extras(), **kw)


def run_count_runs(R):
    G = 1 << gs_of(R)
    return grouped_runs(R, 12 * G + 1, {1: 200, 2: 777, 4: 1500, 5: [1] + [0] * (R - 2)},
                        anchor_run=R // 2, seed=R)


def boundary_runs():
    """anchor run in the middle: older and newer runs hold the boundary keys"""
    return grouped_runs(8, 10 * 128 + 1, {1: 100, 2: 300, 3: 40},
                        anchor_run=3, seed=5, boundary_dups=(1, 2, 3, 4, 7))


MANY_GROUPS = 640  # over 256 workgroups, the smallest grid the engine accepts


def many_groups_runs():
    return grouped_runs(8, MANY_GROUPS * 128, {g: 40 + g % 90 for g in range(1, MANY_GROUPS, 3)},
                        seed=6, sp=1024)


MANY_GROUPS_R32 = 2560  # R = 32, gs = 5: ten groups per workgroup at 256 workgroups


def many_groups_r32_runs():
    return grouped_runs(32, MANY_GROUPS_R32 * 32,
                        {g: 10 + g % 50 for g in range(1, MANY_GROUPS_R32, 3)}, anchor_run=16,
                        seed=7, sp=1024)


DATA = {
    "slots": slots_runs,
    "boundary": boundary_runs,
    "many_groups": many_groups_runs,
    "many_groups_r32": many_groups_r32_runs,
    "all_put": lambda: slots_runs(kinds=("put",), seed=8),
    "var_len": lambda: slots_runs(vary_len=True, seed=9),
    "k32": lambda: slots_runs(klen=32, user_len=20, seed=10),
    **{"r%d" % R: (lambda R=R: run_count_runs(R)) for R in (2, 3, 8, 31, 32, 33)},
    **{"v%d" % v: (lambda v=v: slots_runs(version=v, seed=20 + v)) for v in (0, 2)},
}
_RUNS = {}


def runs_of(name):
    if name not in _RUNS:
        _RUNS[name] = DATA[name]()
    return _RUNS[name]


def probe_keys(runs):
    ks = sorted({rec[0] for run in runs for rec in run})
    return ks[::max(1, len(ks) // 60)] + ks[-3:] + [key_of(99_999_999)]


_REF = {}


def compact_reference(oracle_lib, name, runs, envs):
    """the oracle's answer to a case, computed once"""
    key = (name, json.dumps(envs, sort_keys=True))
    if key not in _REF:
        o = open_part(oracle_lib)
        try:
            if envs:
                o.set_envs(envs)
            ingest(o, runs)
            err, so = o.manual_compact(NOW)
            assert err == OK
            probes = probe_keys(runs)
            _REF[key] = (stats_dict(so), rows_of(o), probes, [o.get(k, 0) for k in probes])
        finally:
            o.close()
    return _REF[key]


def check_compact(oracle_lib, hip_lib, name, runs, envs=None, rank=ROUTE_RANK_GRP,
                  emit=ROUTE_EMIT_CHUNKED_FIXED, engine_envs=None):
    stats, rows, probes, gets = compact_reference(oracle_lib, name, runs, envs or {})
    g = open_part(hip_lib)
    try:
        g.set_envs(dict(envs or {}, **(engine_envs or {})))
        ingest(g, runs)
        err, sg = g.manual_compact(NOW)
        assert err == OK
        assert g.last_compact_route() == (rank, emit if rows else ROUTE_NONE)
        assert stats_dict(sg) == stats
        assert rows_of(g) == rows
        assert [g.get(k, 0) for k in probes] == gets
    finally:
        g.close()
    return stats, rows


# ---- rank staging ---------------------------------------------------------

@gpu
def test_staging_slots_empty_and_lopsided_segments(oracle_lib, hip_lib):
    """gsize 1, 255, 256, 257, 1024, 1793, 2047, 2048 and the 2049 fallback;
    a group 6 of 8 runs skip; a group one other run fills"""
    stats, rows = check_compact(oracle_lib, hip_lib, "slots", runs_of("slots"))
    assert stats["shadowed"] > 0 and stats["tombstones"] > 0 and stats["expired"] > 0


@gpu
@pytest.mark.parametrize("R", [2, 3, 8, 31, 32])
def test_run_counts(oracle_lib, hip_lib, R):
    check_compact(oracle_lib, hip_lib, "r%d" % R, runs_of("r%d" % R))


@gpu
def test_33_runs_take_the_global_rank(oracle_lib, hip_lib):
    check_compact(oracle_lib, hip_lib, "r33", runs_of("r33"), rank=ROUTE_RANK_GLOBAL)


@gpu
def test_boundary_shadow_through_the_run_table(oracle_lib, hip_lib):
    stats, _ = check_compact(oracle_lib, hip_lib, "boundary", runs_of("boundary"))
    assert stats["shadowed"] >= 5 * 7  # each boundary key: one survivor of 8 versions


@gpu
@pytest.mark.parametrize("name,blocks", [("many_groups", 256), ("many_groups", 300),
                                         ("many_groups_r32", 256)])
def test_many_groups_per_workgroup(oracle_lib, hip_lib, name, blocks):
    """engine.grp_blocks takes no less than 256, so the groups are many: 640
    groups of 8 runs on 256 and 300 workgroups (two or three groups each) and
    2560 groups of 32 runs on 256 (ten each).  One run table serves all of a
    workgroup's groups, and the register-held meta words are replaced group
    after group."""
    check_compact(oracle_lib, hip_lib, name, runs_of(name),
                  engine_envs={"engine.grp_blocks": str(blocks)})


# ---- value length ---------------------------------------------------------

@gpu
def test_all_put_runs(oracle_lib, hip_lib):
    stats, _ = check_compact(oracle_lib, hip_lib, "all_put", runs_of("all_put"))
    assert stats["tombstones"] == 0


@gpu
def test_variable_value_lengths_keep_their_sizes(oracle_lib, hip_lib):
    """no shared PUT stride: the per-row-size emit, fed by the rank kernel's
    value lengths"""
    check_compact(oracle_lib, hip_lib, "var_len", runs_of("var_len"), emit=ROUTE_EMIT_CHUNKED)


@gpu
def test_non_bottommost_window_keeps_and_converts_tombstones(oracle_lib, hip_lib):
    m = build_model(fixed_key, 5, 1500, seed=41, universe=3000)
    ops, mop = delete_rule_env(b"u:00000000001")
    m.user_ops = [mop]
    g, b, st = _window_case(hip_lib, oracle_lib, m, 1, 4,
                            envs={"user_specified_compaction": ops})
    try:
        assert g.last_compact_route()[0] == ROUTE_RANK_GRP
        # an upper window drops nothing but shadowed versions: its tombstones are
        # emitted (and not tallied), the PUTs the rule or a TTL removes become
        # tombstones; _window_case compared every read with the oracle's
        assert st["tombstones"] == 0 and st["filtered"] > 0 and st["expired"] > 0
        assert any(kd == 1 for run in m.runs[1:] for _, _, kd in run.values())
        _same_full_compact(g, b)
    finally:
        g.close()
        b.close()


# ---- filters --------------------------------------------------------------

@gpu
def test_default_ttl_rewrite(oracle_lib, hip_lib):
    check_compact(oracle_lib, hip_lib, "slots", runs_of("slots"), envs={"default_ttl": "5000"})


@gpu
@pytest.mark.parametrize("version", [0, 1, 2])
def test_rules_read_keys_through_the_table(oracle_lib, hip_lib, version):
    """ids 1M..2M are deleted by hashkey prefix, ids below 1M get a new TTL"""
    ops = ops_json([
        ("COT_DELETE", "", [pattern_rule("hashkey", b"u:00000001", SMT_PREFIX)]),
        ("COT_UPDATE_TTL", {"type": "UTOT_FROM_NOW", "value": 1234},
         [pattern_rule("hashkey", b"u:00000000", SMT_PREFIX)])])
    name = "slots" if version == 1 else "v%d" % version
    stats, rows = check_compact(
        oracle_lib, hip_lib, name, runs_of(name),
        envs={"pegasus.data_version": str(version), "user_specified_compaction": ops})
    assert stats["filtered"] > 0
    assert any(e == NOW + 1234 for _, _, e in rows)


# ---- the other modes of the rank kernel -----------------------------------

def _pair(oracle_lib, hip_lib, runs, envs, pidx=0):
    o = oracle_lib.open(1, pidx, -1)
    g = hip_lib.open(1, pidx, 0)
    for p in (o, g):
        p.set_envs(envs)
        ingest(p, runs)
    return o, g


@gpu
def test_scan_view_on_the_slot_groups(oracle_lib, hip_lib):
    """a full drain builds the view with the MODE 1 kernel"""
    o, g = _pair(oracle_lib, hip_lib, runs_of("slots"), {})
    try:
        want = _drain(o, NOW, validate_partition_hash=False)
        assert len(want) > 10_000
        assert _drain(g, NOW, validate_partition_hash=False) == want
    finally:
        o.close()
        g.close()


@gpu
@pytest.mark.parametrize("validate", [False, True])
def test_fused_count_on_the_slot_groups(oracle_lib, hip_lib, validate):
    """MODE 2 stages the meta words at once; with hash validation it reads
    key bytes through the table"""
    envs = {"rocksdb.max_iteration_count": str(2**31 - 1)}
    if validate:
        envs["replica.split.validate_partition_hash"] = "true"
    o, g = _pair(oracle_lib, hip_lib, runs_of("slots"), envs, pidx=2 if validate else 0)
    try:
        if validate:
            for p in (o, g):
                p.set_partition_version(3)
        co, _ = _count_fused_or_fallback(o, NOW, validate_partition_hash=validate)
        cg, fused = _count_fused_or_fallback(g, NOW, validate_partition_hash=validate)
        assert fused, "expected the fused count on an eligible table"
        assert cg == co and cg > 0
        if validate:
            cu, _ = _count_fused_or_fallback(g, NOW, validate_partition_hash=False)
            assert cg < cu  # the mask really filtered
    finally:
        o.close()
        g.close()


# ---- emit remainders ------------------------------------------------------

def _tile(kept, fill="dead"):
    """one tile of T ranks whose first `kept` are kept"""
    return ["put"] * kept + [fill] * (T - kept)


# name -> (plan, value user bytes): value stride = 12 + user bytes, chunks per
# row = stride / 16; the chunk count of the first tile is in the name
EMIT_PLANS = {
    "tile_of_0": (["put"] * 5 + ["dead"] * (2 * T + 50) + ["ttl"] * 5, 4),
    "chunks_1": (_tile(1) + ["put"] * 3, 4),
    "chunks_batch_minus_1": (_tile(COPY_BATCH - 1, "del") + ["put"], 4),
    "chunks_batch_last_tile_of_1": (_tile(COPY_BATCH) + ["put"], 4),
    "chunks_batch_plus_1": (_tile(205) + ["ttl"] * 3, 68),       # 5 chunks per row
    "chunks_two_batches_plus_1": (_tile(683) + ["put"] * 9, 36),  # 3 chunks per row
    "rows_v19": (_tile(700) + ["ttl"] * 333, 7),                  # no 16-byte chunks
    "nothing_kept": (["dead", "del"] * 600, 4),
}
EMIT_CASES = [(n, 18) for n in EMIT_PLANS] + [("chunks_batch_plus_1", 32), ("rows_v19", 32)]


@gpu
@pytest.mark.parametrize("rewrite", [False, True], ids=["plain", "rewrite"])
@pytest.mark.parametrize("name,klen", EMIT_CASES, ids=["%s-k%d" % c for c in EMIT_CASES])
def test_emit_remainders(oracle_lib, hip_lib, name, klen, rewrite):
    plan, user_len = EMIT_PLANS[name]
    key = "emit-%s-k%d" % (name, klen)
    if key not in _RUNS:
        _RUNS[key] = plan_runs(plan, klen, user_len)
    # 32-byte keys of that helper differ in their hashkeys: no tail words, global rank
    stats, rows = check_compact(oracle_lib, hip_lib, key, _RUNS[key],
                                envs={"default_ttl": "5000"} if rewrite else None,
                                rank=ROUTE_RANK_GRP if klen == 18 else ROUTE_RANK_GLOBAL)
    assert len(rows) == sum(w in ("put", "ttl") for w in plan)
    if rewrite and rows:
        assert any(e == NOW + 5000 for _, _, e in rows)


# key stride 32: the key span is a chunk copy of two chunks per row, so its chunk
# count is even; name -> kept ranks of the first tile
KEY32_KEPT = {"key_chunks_batch_minus_2": COPY_BATCH // 2 - 1, "key_chunks_batch": COPY_BATCH // 2,
              "key_chunks_batch_plus_2": COPY_BATCH // 2 + 1, "key_chunks_two_batches": COPY_BATCH}


def key32_runs(kept):
    """the plan helper's runs under 32-byte keys that keep their tail words
    (one hashkey, the id in the sortkey), so the group rank feeds the emit"""
    runs = plan_runs(_tile(kept) + ["ttl"] * 3, 32, 7)
    return [[(key_of(int(k[4:18]), 32), v, seq, kind) for k, v, seq, kind in run]
            for run in runs]


@gpu
@pytest.mark.parametrize("name", list(KEY32_KEPT))
def test_key_span_chunk_batches(oracle_lib, hip_lib, name):
    """the batch edges of the chunked KEY copy; the 19-byte values move row by row"""
    key = "emit-" + name
    if key not in _RUNS:
        _RUNS[key] = key32_runs(KEY32_KEPT[name])
    _, rows = check_compact(oracle_lib, hip_lib, key, _RUNS[key])
    assert len(rows) == KEY32_KEPT[name] + 3 and all(len(k) == 32 for k, _, _ in rows)


@gpu
def test_32_byte_keys_on_both_routes(oracle_lib, hip_lib):
    """key stride 32 (two chunks per key) and value stride 32 under the group rank"""
    check_compact(oracle_lib, hip_lib, "k32", runs_of("k32"))


# ---- CPU half -------------------------------------------------------------

def test_cases_are_what_they_claim():
    """group sizes and chunk counts from the data alone (no GPU)"""
    assert [gs_of(R) for R in (2, 3, 8, 31, 32)] == [8, 8, 7, 5, 5]
    for name in ("slots", "all_put", "var_len", "k32", "v0", "v2"):
        sizes = group_sizes(runs_of(name))
        assert len(sizes) == 41 and sizes[-1] == 1
        assert sizes[0] == 128 + 7
        for g, want in SLOT_SIZES.items():
            assert sizes[g] == want, (name, g)
        assert all(s == 128 for s in sizes[11:-1])
    runs = runs_of("slots")
    G = 128
    for g, others_with_keys in ((9, 1), (10, 1)):
        lo, hi = key_of(g * G * SP), key_of((g + 1) * G * SP)
        holders = sum(any(lo <= rec[0] < hi for rec in run) for run in runs)
        assert holders == 1 + others_with_keys
    assert len({len(r[1]) for run in runs_of("var_len") for r in run if r[3] == 0}) > 1
    assert all(r[3] == 0 for run in runs_of("all_put") for r in run)
    for R in (2, 3, 8, 31, 32):
        runs = runs_of("r%d" % R)
        sizes = group_sizes(runs)
        G = 1 << gs_of(R)
        assert len(runs) == R and len(sizes) == 13
        assert sizes[1] == G + 200 and sizes[2] == G + 777 and sizes[4] == G + 1500
        assert sizes[5] == G + 1 and sizes[3] == G and sizes[-1] == 1
        assert max(range(R), key=lambda r: len(runs[r])) == R // 2
    assert len(runs_of("r33")) == 33
    # the boundary keys sit in every run, on both sides of the anchor run
    runs = runs_of("boundary")
    for g in (1, 2, 3, 4, 7):
        assert all(any(rec[0] == key_of(g * 128 * SP) for rec in run) for run in runs)
    sizes = group_sizes(runs)
    assert sum(sizes) == sum(len(r) for r in runs)
    # newer runs' boundary versions close the previous group, older ones open the next
    assert sizes[0] == 128 + 7 + 4 and sizes[4] == 128 + 3 + 0
    sizes = group_sizes(runs_of("many_groups"))
    assert len(sizes) == MANY_GROUPS and MANY_GROUPS > 2 * 256
    assert max(sizes) <= GRP_CAP and sizes[1] == 128 + 41
    sizes = group_sizes(runs_of("many_groups_r32"))
    assert len(sizes) == MANY_GROUPS_R32 == 10 * 256 and len(runs_of("many_groups_r32")) == 32
    assert max(sizes) <= GRP_CAP and sizes[1] == 32 + 11 and sizes[2] == 32
    for name, (plan, user_len) in EMIT_PLANS.items():
        assert (12 + user_len) % 16 == 0 or name == "rows_v19"
    chunks = {n: sum(w in ("put", "ttl") for w in p[:T]) * ((12 + u) // 16)
              for n, (p, u) in EMIT_PLANS.items() if n != "rows_v19"}
    assert chunks == {"tile_of_0": 5, "chunks_1": 1, "chunks_batch_minus_1": COPY_BATCH - 1,
                      "chunks_batch_last_tile_of_1": COPY_BATCH,
                      "chunks_batch_plus_1": COPY_BATCH + 1,
                      "chunks_two_batches_plus_1": 2 * COPY_BATCH + 1, "nothing_kept": 0}
    plan = EMIT_PLANS["tile_of_0"][0]
    assert not {"put", "ttl"} & set(plan[T:2 * T])  # a tile of 0 chunks among kept rows
    assert len(EMIT_PLANS["chunks_batch_last_tile_of_1"][0]) == T + 1
    assert len(plan_key(0, 32)) == len(key_of(0, 32)) == 32 and len(key_of(0)) == 18
    assert [2 * k for k in KEY32_KEPT.values()] == [COPY_BATCH - 2, COPY_BATCH, COPY_BATCH + 2,
                                                    2 * COPY_BATCH]
    runs = key32_runs(3)
    assert sum(len(r) for r in runs) == T + 3 and max(KEY32_KEPT.values()) <= T
    assert sorted(r[0] for run in runs for r in run) == [key_of(i, 32) for i in range(T + 3)]


def test_grp_stage_check_program():
    """tools/grp_stage_check.cpp (the staging map and the copy schedule
    against brute-force loops), as built by __graft_entry__.build()"""
    exe = os.path.join(REPO, "bin", "grp_stage_check")
    assert os.path.exists(exe), "bin/grp_stage_check not built (run __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "grp_stage_check OK" in r.stdout, r.stderr
