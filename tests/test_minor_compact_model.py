"""Window (minor) compaction: the independent model and its CPU checks.

`merge_window` restates what a compaction over runs [first, first+n) must
produce (include/rrdb_engine_ext.h, DESIGN.md "Minor compaction").  It reuses
tests/pymodel.py's Model._filter — the KeyWithTTLCompactionFilter restatement
— unmodified.  Bottommost (first == 0): tombstones and filter-removed PUTs
vanish, as in Model.compact_full.  Otherwise only shadowed versions vanish: a
tombstone stays, and a PUT the filter removes becomes a tombstone with its own
seqno and an empty value (rocksdb CompactionIterator: Decision::kRemove ->
kTypeDeletion unless the key cannot exist beyond the output level).

The CPU oracle has no window compaction, so parity is physical: ingest the
runs before the window, the model's merged run and the runs after it into a
second oracle handle ("oracle B").  These tests pin the model itself against
the oracle; tests/test_minor_compact_gpu.py then pins the engine against
oracle B.
"""
import ctypes
import json
import os
import random
import re

import pytest

from conftest import HIP_SO, REPO
from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import OK, SCAN_COMPLETED
from pymodel import Model

NOW = 100_000
STAT_FIELDS = ("input_records", "output_records", "expired", "filtered", "tombstones",
               "shadowed", "output_bytes")


# ---------------- the model ----------------

def merge_window(model: Model, first: int, n: int, now: int):
    """Merge model.runs[first:first+n] -> (merged run dict, stats dict).
    Does not modify the model."""
    window = model.runs[first:first + n]
    bottommost = first == 0
    stats = dict.fromkeys(STAT_FIELDS, 0)
    newest = {}
    for run in window:
        stats["input_records"] += len(run)
        for k, (v, s, kd) in run.items():
            if k in newest:
                stats["shadowed"] += 1
            if k not in newest or s > newest[k][1]:
                newest[k] = (v, s, kd)
    out = {}
    for k in sorted(newest):
        v, s, kd = newest[k]
        if kd == 1:
            if bottommost:
                stats["tombstones"] += 1
                continue
            rec = (v, s, 1)  # kept verbatim
        else:
            reason, newv = model._filter(k, v, now)
            if reason is None:
                rec = (newv if newv is not None else v, s, 0)
            else:
                stats[reason] += 1
                if bottommost:
                    continue
                rec = (b"", s, 1)  # converted: the older version stays hidden
        out[k] = rec
        stats["output_records"] += 1
        stats["output_bytes"] += len(k) + len(rec[0])
    return out, stats


def apply_window(model: Model, first: int, n: int, now: int):
    """Window-compact the model in place; returns the stats dict."""
    merged, stats = merge_window(model, first, n, now)
    model.runs[first:first + n] = [merged] if merged else []
    return stats


def ingest_model(part, model: Model):
    """Ingest every run of the model, oldest first (the physical layout)."""
    for run in model.runs:
        part.ingest_run([(k, v, s, kd) for k, (v, s, kd) in sorted(run.items())])


def stats_dict(cs):
    return {f: getattr(cs, f) for f in STAT_FIELDS}


# ---------------- seeded data ----------------

def fixed_key(i: int) -> bytes:
    """18-byte key: 16-byte hashkey, empty sortkey; every key shares the
    first 10+ bytes, so runs are tail-word (group rank) eligible."""
    return D.generate_key(b"u:%014d" % i, b"")


def mixed_key(i: int) -> bytes:
    """keys of several lengths: the general (non tail-word) kernels"""
    hk = b"hk" + b"x" * (i % 3) + b"%d" % (i % 7)
    return D.generate_key(hk, b"s%0*d" % (3 + i % 4, i))


def build_model(keyfn, n_runs, per_run, seed, now=NOW, universe=None, p_del=0.15,
                p_ttl=0.3, fixed_vlen=False):
    """n_runs runs of per_run records sampled from one key universe, so keys
    recur across runs (overwrites), with tombstones and TTLs of which some
    are already expired at `now`.  fixed_vlen: every record, tombstones
    included, stores a 32-byte value (a tombstone's bytes are never read, but
    a window pass must carry them over verbatim)."""
    rnd = random.Random(seed)
    universe = universe or per_run * 2
    m = Model()
    seq = 1
    for _ in range(n_runs):
        recs = []
        for i in sorted(rnd.sample(range(universe), per_run)):
            if rnd.random() < p_del:
                recs.append((keyfn(i), b"\x00" * 32 if fixed_vlen else b"", seq, 1))
            else:
                ets = 0
                if rnd.random() < p_ttl:
                    ets = now - 10 if rnd.random() < 0.5 else now + 500
                body = b"v%d-%d" % (i, seq)
                recs.append((keyfn(i), D.encode_value(body.ljust(20, b".") if fixed_vlen
                                                      else body, ets, 0, 1), seq, 0))
            seq += 1
        recs.sort()
        m.ingest(recs)
    return m


def delete_rule_env(hashkey_prefix: bytes):
    """(engine env value, model op) of a user delete op on a hashkey prefix"""
    ops = {"ops": [{"type": "COT_DELETE", "params": "", "rules": [
        {"type": "FRT_HASHKEY_PATTERN",
         "params": json.dumps({"pattern": hashkey_prefix.decode(),
                               "match_type": "SMT_MATCH_PREFIX"})}]}]}
    mop = dict(type="delete", rules=[dict(type="hashkey", pattern=hashkey_prefix,
                                          match_type="prefix")])
    return json.dumps(ops), mop


def drain(part, now, **kw):
    """paged full scan -> [(key, value, expire_ts)]"""
    out = []
    res = part.scan_open(b"\x00\x00", b"\xff\xff", now, batch_size=97,
                         return_expire_ts=True, validate_partition_hash=False, **kw)
    while True:
        assert res.error == OK
        out.extend((k, v, e) for (k, v), e in zip(res.kvs, res.expire_ts or []))
        if res.context_id == SCAN_COMPLETED:
            return out
        res = part.scan_next(res.context_id, now)


def hash_keys_of(model: Model):
    return sorted({D.restore_key(k)[0] for run in model.runs for k in run})


# ---------------- CPU tests ----------------

@pytest.mark.parametrize("keyfn", [fixed_key, mixed_key])
def test_window_model_all_runs_equals_oracle_manual_compact(oracle_lib, keyfn):
    m = build_model(keyfn, 4, 300, seed=11)
    ops_json, mop = delete_rule_env(b"u:0000000000001" if keyfn is fixed_key else b"hkx")
    m.default_ttl = 700
    m.user_ops = [mop]
    a = oracle_lib.open(1, 0, -1)
    b = oracle_lib.open(1, 0, -1)
    try:
        a.set_envs({"default_ttl": "700", "user_specified_compaction": ops_json})
        ingest_model(a, m)
        err, sa = a.manual_compact(NOW)
        assert err == OK
        merged, sm = merge_window(m, 0, len(m.runs), NOW)
        assert sm == stats_dict(sa)
        assert sm["filtered"] > 0 and sm["expired"] > 0 and sm["tombstones"] > 0
        assert all(kd == 0 for _, _, kd in merged.values())
        apply_window(m, 0, 4, NOW)
        ingest_model(b, m)
        for now in (NOW, NOW + 600):
            assert drain(a, now) == drain(b, now)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("keyfn", [fixed_key, mixed_key])
def test_upper_window_is_read_invariant_without_rules(oracle_lib, keyfn):
    """No rules, default_ttl 0: a compaction may not change any read.  Oracle
    A holds the runs uncompacted, oracle B the model-merged window [1,4)."""
    m = build_model(keyfn, 4, 300, seed=12)
    a = oracle_lib.open(1, 0, -1)
    b = oracle_lib.open(1, 0, -1)
    try:
        ingest_model(a, m)
        keys = sorted({k for run in m.runs for k in run})
        hks = hash_keys_of(m)
        st = apply_window(m, 1, 3, NOW)
        assert st["tombstones"] == 0 and st["expired"] > 0
        assert st["input_records"] == st["output_records"] + st["shadowed"]
        assert any(kd == 1 and v == b"" for v, _, kd in m.runs[1].values())
        ingest_model(b, m)
        assert (a.num_runs(), b.num_runs()) == (4, 2)
        for now in (NOW, NOW + 600):
            for k in keys + [fixed_key(10**9), mixed_key(10**9)]:
                assert a.get(k, now) == b.get(k, now)
                assert a.ttl(k, now) == b.ttl(k, now)
            for hk in hks[:40]:
                assert a.sortkey_count(hk, now) == b.sortkey_count(hk, now)
                assert a.multi_get(hk, now) == b.multi_get(hk, now)
                assert a.multi_get(hk, now, reverse=True, max_kv_count=3) == \
                    b.multi_get(hk, now, reverse=True, max_kv_count=3)
            assert drain(a, now) == drain(b, now)
    finally:
        a.close()
        b.close()


def test_ext_header_and_exports():
    ext = open(os.path.join(REPO, "include", "rrdb_engine_ext.h")).read()
    base = open(os.path.join(REPO, "include", "rrdb_engine.h")).read()
    names = ("rrdb_compact_runs", "rrdb_auto_compact")
    for nm in names:
        assert re.search(r"\bint32_t\s+%s\s*\(" % nm, ext), nm
        assert not re.search(r"\b%s\s*\(" % nm, base), nm
    assert '#include "rrdb_engine.h"' in ext
    if not os.path.exists(HIP_SO):
        pytest.skip("librrdb_hip.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(HIP_SO)
    assert all(hasattr(lib, nm) for nm in names)


def test_oracle_backend_raises(oracle_part):
    assert not oracle_part.lib.has_window_compact
    with pytest.raises(RuntimeError, match="rrdb_compact_runs"):
        oracle_part.compact_runs(0, 1, NOW)
    with pytest.raises(RuntimeError, match="rrdb_compact_runs"):
        oracle_part.auto_compact(NOW)
