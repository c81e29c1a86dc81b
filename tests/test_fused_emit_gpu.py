"""The fused all-fixed-stride compaction emit at its tile edges.

When every run shares one key stride and one PUT-value stride, a bottommost
chunked pass counts the keep flags per tile of T = 1024 merged ranks
(k_keep_tile_counts), scans the counts in one workgroup, 256 per pass
(k_keep_tile_scan), and one kernel per tile scans its flags, writes the row
columns and copies the tile's key and value spans (k_emit_fixed_fused; the
indexing is incubator_pegasus_amd/csrc/emit_tile.h).

Every case ingests the same seeded runs into the CPU oracle and the engine,
compacts both, and compares the stats, a full scan of keys, values and expire
timestamps, and point gets, byte for byte.  The merged rank of a record is its
position in key order (versions of one key are neighbours), so a case places
its dropped ranks exactly: a tombstone, or a PUT that expired before NOW, is a
dropped rank of its own; an overwritten older version is a shadowed one.

The CPU half runs tools/emit_tile_check.cpp as __graft_entry__.build() built it.
"""
import os
import random
import subprocess

import pytest

from conftest import REPO
from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import (OK, ROUTE_EMIT_CHUNKED_FIXED, ROUTE_NONE,
                                        SCAN_COMPLETED)
from rule_tables import SMT_PREFIX, open_part, ops_json, pattern_rule
from test_minor_compact_model import stats_dict

gpu = pytest.mark.gpu

NOW = 100_000
T = 1024          # EMIT_TILE
SCAN_PASS = 256   # EMIT_SCAN_PASS
N_RUNS = 3


def make_key(i: int, klen: int) -> bytes:
    """18 bytes: 16-byte hashkey, empty sortkey.  32 bytes: a 14-byte sortkey
    behind it.  Key order is index order."""
    assert klen in (18, 32)
    return D.generate_key(b"u:%014d" % i, b"" if klen == 18 else b"s%013d" % i)


def make_value(i: int, seq: int, user_len: int, expire: int, version: int = 1) -> bytes:
    body = (b"v%d-%d|" % (i, seq)).ljust(user_len, b".")[:user_len]
    return D.encode_value(body, expire, seq, version)


def build_runs(plan, klen, user_len, version=1):
    """plan: one entry per key index, in key order:
         "put"   a live PUT            -> one kept rank
         "ttl"   a live PUT with a TTL -> one kept rank
         "dead"  a PUT expired at NOW  -> one dropped rank
         "del"   a tombstone, no value -> one dropped rank
         "over"  a live PUT over an older PUT in an older run -> one kept and
                 one shadowed rank
       Returns N_RUNS sorted record lists, oldest first; seqnos grow with the
       run, so the newer run wins."""
    rnd = random.Random(len(plan) * 31 + klen + user_len)
    runs = [[] for _ in range(N_RUNS)]

    def add(r, i, kind, expire):
        seq = r * 10_000_000 + i + 1
        val = b"" if kind else make_value(i, seq, user_len, expire, version)
        runs[r].append((make_key(i, klen), val, seq, kind))

    for i, what in enumerate(plan):
        r = rnd.randrange(N_RUNS)
        if what == "over":
            r = rnd.randrange(1, N_RUNS)
            add(rnd.randrange(r), i, 0, 0)
        add(r, i, 1 if what == "del" else 0,
            {"ttl": NOW + 500, "dead": NOW - 10}.get(what, 0))
    return [r for r in runs if r]


def total_records(plan):
    return len(plan) + sum(w == "over" for w in plan)


def random_plan(total, seed, p_over=0.08):
    """`total` input records exactly: kept, expired, deleted, overwritten"""
    rnd = random.Random(seed)
    plan = []
    left = total
    while left:
        x = rnd.random()
        if x < p_over and left >= 2:
            plan.append("over")
            left -= 2
            continue
        plan.append("del" if x < 0.2 else "dead" if x < 0.3 else "ttl" if x < 0.5 else "put")
        left -= 1
    assert total_records(plan) == total
    return plan


def dropped_tile_plan():
    """more than 2T consecutive dropped ranks: wherever the tiles fall, one of
    them keeps nothing; kept rows on both sides of the block"""
    plan = random_plan(T + 5, 3, p_over=0)
    plan += ["del" if i % 3 else "dead" for i in range(2 * T + 7)]
    plan += random_plan(T + 9, 4, p_over=0)
    return plan


PLANS = {
    "t_minus_1": lambda: random_plan(T - 1, 11),
    "t": lambda: random_plan(T, 12),
    "t_plus_1": lambda: random_plan(T + 1, 13),
    "two_t_plus_3": lambda: random_plan(2 * T + 3, 14),
    "tile_dropped": dropped_tile_plan,
    # (every run needs a PUT to have a PUT-value stride: most drops are "dead")
    "first_only": lambda: ["put"] + ["dead" if i % 4 else "del" for i in range(2 * T + 2)],
    "last_only": lambda: ["dead"] * (2 * T + 2) + ["put"],
    "all_dropped": lambda: ["del", "dead"] * (T + 1),
    # more tiles than one pass of the one-workgroup scan covers, and a last
    # pass that is not full
    "scan_passes": lambda: random_plan((SCAN_PASS + 3) * T + 5, 15),
}
# (name, plan, key bytes, user bytes): value stride = 12 + user bytes
CASES = [(name, name, 18, 100) for name in PLANS if name != "scan_passes"]
CASES += [
    ("scan_passes", "scan_passes", 18, 4),        # 16-byte values
    ("k18_v19", "two_t_plus_3", 18, 7),           # neither stride a multiple of 16
    ("k32_v16", "two_t_plus_3", 32, 4),           # both
    ("k32_v19", "two_t_plus_3", 32, 7),
]


def rows_of(part):
    """full scan at epoch 0 (nothing TTL-hidden) -> [(key, value, expire_ts)]"""
    out = []
    res = part.scan_open(b"\x00\x00", b"\xff\xff", 0, batch_size=50_000, return_expire_ts=True,
                         validate_partition_hash=False)
    while True:
        assert res.error == OK
        out.extend((k, v, e) for (k, v), e in zip(res.kvs, res.expire_ts or []))
        if res.context_id == SCAN_COMPLETED:
            return out
        res = part.scan_next(res.context_id, 0)


def ingest(part, runs):
    for run in runs:
        part.ingest_run(run)


_REF = {}


def reference(oracle_lib, name, plan_name, klen, user_len):
    """the runs of a case and the oracle's answer to them, computed once"""
    if name not in _REF:
        plan = PLANS[plan_name]()
        runs = build_runs(plan, klen, user_len)
        o = open_part(oracle_lib)
        try:
            ingest(o, runs)
            err, so = o.manual_compact(NOW)
            assert err == OK
            rows = rows_of(o)
            probes = sample_keys(plan, klen)
            gets = [o.get(k, 0) for k in probes]
        finally:
            o.close()
        kept = sum(w in ("put", "ttl", "over") for w in plan)
        assert so.input_records == total_records(plan)
        assert so.output_records == len(rows) == kept
        _REF[name] = (runs, stats_dict(so), rows, probes, gets)
    return _REF[name]


def sample_keys(plan, klen):
    """first, last, the tile edges and a stride through the rest, kept or not"""
    n = len(plan)
    idx = {0, n - 1, n // 2} | set(range(0, n, max(1, n // 40)))
    idx |= {i for e in (T, 2 * T) for i in (e - 1, e, e + 1) if i < n}
    return [make_key(i, klen) for i in sorted(idx)]


def check_against(g, ref):
    _, _, rows, probes, gets = ref
    assert rows_of(g) == rows
    assert [g.get(k, 0) for k in probes] == gets


@gpu
@pytest.mark.parametrize("name,plan_name,klen,user_len", CASES, ids=[c[0] for c in CASES])
def test_fused_emit_case(oracle_lib, hip_lib, name, plan_name, klen, user_len):
    ref = reference(oracle_lib, name, plan_name, klen, user_len)
    runs, stats, rows = ref[:3]
    g = open_part(hip_lib)
    try:
        ingest(g, runs)
        err, sg = g.manual_compact(NOW)
        assert err == OK
        if rows:
            assert g.last_compact_route()[1] == ROUTE_EMIT_CHUNKED_FIXED
            assert g.num_runs() == 1
        else:
            # n_out == 0: nothing to emit and no output run
            assert g.last_compact_route()[1] == ROUTE_NONE
            assert g.num_runs() == 0 and g.num_records() == 0
        assert stats_dict(sg) == stats
        check_against(g, ref)
    finally:
        g.close()


def test_cases_are_what_they_claim():
    """the shapes the cases are named for, from the plans alone (no GPU)"""
    for name, want in (("t_minus_1", T - 1), ("t", T), ("t_plus_1", T + 1),
                       ("two_t_plus_3", 2 * T + 3)):
        assert total_records(PLANS[name]()) == want
    for name in ("t_minus_1", "t", "t_plus_1", "two_t_plus_3", "scan_passes"):
        assert {"put", "ttl", "dead", "del", "over"} == set(PLANS[name]())
    plan = PLANS["tile_dropped"]()
    run = best = 0
    for w in plan:
        run = run + 1 if w in ("del", "dead") else 0
        best = max(best, run)
    assert best >= 2 * T and "over" not in plan
    assert "put" in plan[:T + 5] and "put" in plan[-(T + 9):]
    for name, kept_at in (("first_only", 0), ("last_only", -1)):
        plan = PLANS[name]()
        assert len(plan) == 2 * T + 3 and plan[kept_at] == "put"
        assert sum(w in ("put", "ttl", "over") for w in plan) == 1
    assert not {"put", "ttl", "over"} & set(PLANS["all_dropped"]())
    tiles = -(-total_records(PLANS["scan_passes"]()) // T)
    assert tiles > SCAN_PASS and tiles % SCAN_PASS != 0
    strides = {(c[2], 12 + c[3]) for c in CASES}
    assert {k % 16 == 0 for k, _ in strides} == {True, False}
    assert {v % 16 == 0 for _, v in strides} == {True, False}
    assert any(k == 18 for k, _ in strides)


@gpu
def test_keep_inputs_pass_repeats(oracle_lib, hip_lib):
    """begin/finish with keep_inputs, twice on one handle, as the benchmark
    repeats its passes: each reports the full pass and leaves the inputs; a
    plain pass then produces the same run."""
    ref = reference(oracle_lib, "two_t_plus_3", "two_t_plus_3", 18, 100)
    runs, stats = ref[:2]
    g = open_part(hip_lib)
    try:
        ingest(g, runs)
        for _ in range(2):
            assert g.manual_compact_begin(NOW, keep_inputs=True) == OK
            err, sg = g.manual_compact_finish()
            assert err == OK
            assert g.last_compact_route()[1] == ROUTE_EMIT_CHUNKED_FIXED
            assert stats_dict(sg) == stats
            assert g.num_runs() == len(runs)
        err, sg = g.manual_compact(NOW)
        assert err == OK and stats_dict(sg) == stats
        assert g.last_compact_route()[1] == ROUTE_EMIT_CHUNKED_FIXED
        check_against(g, ref)
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("version", [0, 1, 2])
def test_rewrite_mode(oracle_lib, hip_lib, version):
    """default_ttl plus an update-TTL rule at T + 1 records, all kept: output
    row r is key r, so rows 0, T - 1 and T — the first and last row of a tile
    and the only row of the next — are rewritten.  Keys with i % 7 == 3 carry
    their own TTL and, beyond the rule's prefix (keys 0..9), are copied untouched."""
    n = T + 1
    ttl, bump = 5000, 1234
    ops = ops_json([("COT_UPDATE_TTL", {"type": "UTOT_FROM_NOW", "value": bump},
                     [pattern_rule("hashkey", b"u:" + b"0" * 13, SMT_PREFIX)])])
    runs = [[] for _ in range(2)]
    for i in range(n):
        expire = NOW + 500 if i % 7 == 3 else 0
        seq = (i % 2) * 10_000_000 + i + 1  # a newer run's seqnos lie above the older run's
        runs[i % 2].append((make_key(i, 18), make_value(i, seq, 100, expire, version), seq, 0))
    got = []
    for lib in (oracle_lib, hip_lib):
        p = open_part(lib)
        try:
            p.set_envs({"pegasus.data_version": str(version), "default_ttl": str(ttl),
                        "user_specified_compaction": ops})
            ingest(p, runs)
            err, st = p.manual_compact(NOW)
            assert err == OK
            if lib is hip_lib:
                assert p.last_compact_route()[1] == ROUTE_EMIT_CHUNKED_FIXED
            got.append((stats_dict(st), rows_of(p),
                        [p.get(make_key(i, 18), 0) for i in (0, 3, 9, 11, 17, T - 1, T)]))
        finally:
            p.close()
    want, have = got
    rows = want[1]
    assert len(rows) == n and want[0]["output_records"] == n
    # the oracle's rows are what the case claims before the engine is compared
    for r in (0, 9):
        assert rows[r][2] == NOW + bump      # the rule's prefix: indices 0..9
    for r in (11, T - 1, T):
        assert rows[r][2] == NOW + ttl       # default_ttl alone
    assert rows[3][2] == NOW + bump and rows[17][2] == NOW + 500
    assert have[0] == want[0]
    assert have[1] == rows
    assert have[2] == want[2]
    assert all(st == OK for st, _ in have[2])


def test_emit_tile_check_program():
    """tools/emit_tile_check.cpp (the emit's indexing header against
    brute-force loops), as built by __graft_entry__.build()"""
    exe = os.path.join(REPO, "bin", "emit_tile_check")
    if not os.path.exists(exe):
        pytest.skip("bin/emit_tile_check not built (run __graft_entry__.build())")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "emit_tile_check OK" in r.stdout, r.stderr
