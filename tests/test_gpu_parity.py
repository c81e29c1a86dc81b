"""GPU parity: the HIP engine (librrdb_hip.so, the product) against the CPU
oracle (the checker) on identical seeded inputs, through the same C-ABI.

Bit-exactness bar: query results and surviving-key sets must
match byte for byte — keys, values, expire headers, status codes, counts.
"""
import json
import random

import pytest

from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import (FT_MATCH_ANYWHERE, FT_MATCH_PREFIX,
                                        FT_MATCH_POSTFIX, FT_NO_FILTER, INCOMPLETE,
                                        NOT_FOUND, OK, ROUTE_RANK_GLOBAL, ROUTE_RANK_LDS,
                                        ROUTE_RANK_LDST, SCAN_COMPLETED)

pytestmark = pytest.mark.gpu


@pytest.fixture()
def pair(oracle_lib, hip_lib):
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    yield o, g
    o.close()
    g.close()


def _mk_records(rnd, n_keys, with_sortkeys=False, ttl_frac=0.2, now=1000):
    recs = []
    for i in range(n_keys):
        hk = f"hk{rnd.randrange(max(1, n_keys // 2)):05d}".encode()
        sk = f"sk{rnd.randrange(5):02d}".encode() if with_sortkeys else b""
        expire = 0
        r = rnd.random()
        if r < ttl_frac / 2:
            expire = rnd.randrange(1, now + 1)
        elif r < ttl_frac:
            expire = now + rnd.randrange(1, 10000)
        val = D.encode_value(f"value-{i}-".encode() * rnd.randrange(1, 4), expire, i + 1, 1)
        kind = 1 if rnd.random() < 0.1 else 0
        recs.append((D.generate_key(hk, sk), val if kind == 0 else b"\x00" * 12, kind))
    return recs


def _ingest_pair(o, g, runs):
    seq = 1
    all_keys = []
    for run in runs:
        run = sorted({k: (v, kind) for k, v, kind in run}.items())
        records = []
        for key, (v, kind) in run:
            records.append((key, v, seq, kind))
            all_keys.append(key)
            seq += 1
        o.ingest_run(records)
        g.ingest_run(records)
    return sorted(set(all_keys))


def _rand_runs(rnd, n_runs, keys_per_run, **kw):
    return [_mk_records(rnd, keys_per_run, **kw) for _ in range(n_runs)]


@pytest.mark.parametrize("seed", range(4))
def test_get_parity(pair, seed):
    o, g = pair
    rnd = random.Random(seed)
    now = 1000
    keys = _ingest_pair(o, g, _rand_runs(rnd, rnd.randrange(1, 6), 50, now=now))
    probes = keys + [D.generate_key(b"miss", str(i).encode()) for i in range(5)]
    for k in probes:
        assert o.get(k, now) == g.get(k, now), k
        assert o.ttl(k, now) == g.ttl(k, now), k


@pytest.mark.parametrize("seed", range(3))
def test_batch_get_parity(pair, seed):
    o, g = pair
    rnd = random.Random(50 + seed)
    now = 1000
    keys = _ingest_pair(o, g, _rand_runs(rnd, 4, 60, now=now))
    probes = list(keys)
    rnd.shuffle(probes)
    probes += [D.generate_key(b"nope", b"x")]
    assert o.batch_get(probes, now) == g.batch_get(probes, now)


@pytest.mark.parametrize("seed", range(3))
def test_sortkey_count_parity(pair, seed):
    o, g = pair
    rnd = random.Random(80 + seed)
    now = 1000
    keys = _ingest_pair(o, g, _rand_runs(rnd, 3, 60, with_sortkeys=True, now=now))
    hks = sorted({D.restore_key(k)[0] for k in keys})
    for hk in hks[:10] + [b"absent"]:
        assert o.sortkey_count(hk, now) == g.sortkey_count(hk, now), hk


@pytest.mark.parametrize("seed", range(3))
def test_multi_get_parity(pair, seed):
    o, g = pair
    rnd = random.Random(120 + seed)
    now = 1000
    keys = _ingest_pair(o, g, _rand_runs(rnd, 3, 80, with_sortkeys=True, now=now))
    hks = sorted({D.restore_key(k)[0] for k in keys})
    for hk in hks[:8]:
        for kwargs in [
            dict(),
            dict(start_sortkey=b"sk01", stop_sortkey=b"sk03", stop_inclusive=True),
            dict(start_sortkey=b"sk01", start_inclusive=False),
            dict(sort_key_filter_type=FT_MATCH_PREFIX, sort_key_filter_pattern=b"sk0"),
            dict(sort_key_filter_type=FT_MATCH_ANYWHERE, sort_key_filter_pattern=b"k0"),
            dict(sort_key_filter_type=FT_MATCH_POSTFIX, sort_key_filter_pattern=b"2"),
            dict(reverse=True),
            dict(max_kv_count=2),
            dict(max_kv_count=2, reverse=True),
            dict(no_value=True),
            dict(start_sortkey=b"sk04", stop_sortkey=b"sk01"),
            dict(sort_keys=[b"sk01", b"sk00", b"skxx"]),
            dict(sort_keys=[b"sk00", b"sk01", b"sk02"], max_kv_count=1),
        ]:
            assert o.multi_get(hk, now, **kwargs) == g.multi_get(hk, now, **kwargs), (hk, kwargs)


def _drain(part, now, **kw):
    out, counts = [], 0
    res = part.scan_open(b"\x00\x00", b"\xff\xff", now, **kw)
    assert res.error == OK
    out.extend(res.kvs)
    ets = list(res.expire_ts or [])
    if res.kv_count is not None:
        counts += res.kv_count
    while res.context_id != SCAN_COMPLETED:
        res = part.scan_next(res.context_id, now)
        assert res.error == OK
        out.extend(res.kvs)
        ets.extend(res.expire_ts or [])
        if res.kv_count is not None:
            counts += res.kv_count
    return out, counts, ets


@pytest.mark.parametrize("seed", range(3))
def test_scan_parity(pair, seed):
    o, g = pair
    rnd = random.Random(200 + seed)
    now = 1000
    _ingest_pair(o, g, _rand_runs(rnd, 4, 80, with_sortkeys=True, now=now))
    for kw in [
        dict(batch_size=13, validate_partition_hash=False),
        dict(batch_size=7, only_return_count=True, validate_partition_hash=False),
        dict(batch_size=1000, no_value=True, validate_partition_hash=False),
        dict(batch_size=17, return_expire_ts=True, validate_partition_hash=False),
        dict(batch_size=11, hash_key_filter_type=FT_MATCH_PREFIX,
             hash_key_filter_pattern=b"hk0", validate_partition_hash=False),
        dict(batch_size=9, sort_key_filter_type=FT_MATCH_POSTFIX,
             sort_key_filter_pattern=b"1", validate_partition_hash=False),
    ]:
        assert _drain(o, now, **kw) == _drain(g, now, **kw), kw


def test_scan_bounds_parity(pair):
    o, g = pair
    now = 1000
    hk = b"bhk"
    recs = [(D.generate_key(hk, f"k{i}".encode()), D.encode_value(b"v", 0, i + 1, 1), i + 1, 0)
            for i in range(5)]
    o.ingest_run(recs)
    g.ingest_run(recs)
    K = lambda sk: D.generate_key(hk, sk)
    for start, stop, si, pi in [
        (K(b"k1"), K(b"k3"), True, True), (K(b"k1"), K(b"k3"), True, False),
        (K(b"k1"), K(b"k3"), False, True), (K(b"k1"), K(b"k3"), False, False),
        (K(b"k2"), K(b"k2"), True, True), (K(b"k2"), K(b"k2"), True, False),
        (K(b"k4"), K(b"k0"), True, True),
    ]:
        ro = o.scan_open(start, stop, now, start_inclusive=si, stop_inclusive=pi,
                         validate_partition_hash=False)
        rg = g.scan_open(start, stop, now, start_inclusive=si, stop_inclusive=pi,
                         validate_partition_hash=False)
        assert (ro.error, ro.kvs, ro.context_id) == (rg.error, rg.kvs, rg.context_id)


def test_scan_hash_validation_parity(oracle_lib, hip_lib):
    now = 1000
    mask = 3
    for pidx in (0, 2):
        o = oracle_lib.open(1, pidx, -1)
        g = hip_lib.open(1, pidx, 0)
        try:
            for p in (o, g):
                p.set_envs({"replica.split.validate_partition_hash": "true"})
                p.set_partition_version(mask)
            recs = [(D.generate_key(f"h{i:03d}".encode(), b""),
                     D.encode_value(b"v", 0, i + 1, 1), i + 1, 0) for i in range(64)]
            o.ingest_run(recs)
            g.ingest_run(recs)
            ro = o.scan_open(b"\x00\x00", b"\xff\xff", now)
            rg = g.scan_open(b"\x00\x00", b"\xff\xff", now)
            assert ro.kvs == rg.kvs and len(rg.kvs) > 0
        finally:
            o.close()
            g.close()


@pytest.mark.parametrize("seed", range(3))
def test_compact_parity(pair, seed):
    o, g = pair
    rnd = random.Random(300 + seed)
    now = 5000
    _ingest_pair(o, g, _rand_runs(rnd, 5, 70, with_sortkeys=True, now=now))
    ops_json = json.dumps({"ops": [
        {"type": "COT_DELETE", "params": "", "rules": [
            {"type": "FRT_SORTKEY_PATTERN",
             "params": json.dumps({"pattern": "sk01", "match_type": "SMT_MATCH_PREFIX"})}]},
        {"type": "COT_UPDATE_TTL",
         "params": json.dumps({"type": "UTOT_FROM_NOW", "value": 777}),
         "rules": [
            {"type": "FRT_HASHKEY_PATTERN",
             "params": json.dumps({"pattern": "hk000", "match_type": "SMT_MATCH_PREFIX"})}]},
    ]})
    envs = {"default_ttl": "4242", "user_specified_compaction": ops_json}
    o.set_envs(envs)
    g.set_envs(envs)
    eo, so = o.manual_compact(now)
    eg, sg = g.manual_compact(now)
    assert eo == eg == OK
    assert (so.input_records, so.output_records, so.expired, so.filtered, so.tombstones,
            so.shadowed, so.output_bytes) == \
           (sg.input_records, sg.output_records, sg.expired, sg.filtered, sg.tombstones,
            sg.shadowed, sg.output_bytes)
    # surviving content identical (scan with values + expire headers)
    assert _drain(o, 0, return_expire_ts=True, validate_partition_hash=False) == \
           _drain(g, 0, return_expire_ts=True, validate_partition_hash=False)


def test_compact_then_reads_parity(pair):
    """compact twice (idempotence) then keep reading."""
    o, g = pair
    rnd = random.Random(999)
    now = 1000
    keys = _ingest_pair(o, g, _rand_runs(rnd, 4, 50, with_sortkeys=True, now=now))
    for p in (o, g):
        p.manual_compact(now)
    s1o = o.manual_compact(now)
    s1g = g.manual_compact(now)
    assert s1o == s1g  # second compact: no shadowed, no tombstones
    for k in keys[:40]:
        assert o.get(k, now) == g.get(k, now)
    # ingest more on top of the compacted run
    extra = [(D.generate_key(b"zz-new", str(i).encode()),
              D.encode_value(b"nv", 0, 0, 1), 10_000 + i, 0) for i in range(5)]
    o.ingest_run(extra)
    g.ingest_run(extra)
    for k, _, _, _ in extra:
        assert o.get(k, now) == g.get(k, now)


def test_backend_identity(hip_lib):
    assert hip_lib.backend == "hip-gfx950"


def test_device_resident_scan_output(pair):
    """engine extension: on_device_out leaves kv bytes in HBM and returns
    device pointers + the count; count must match the host-copy path."""
    o, g = pair
    now = 1000
    recs = [(D.generate_key(b"dev", f"s{i:03d}".encode()),
             D.encode_value(b"v" * 20, 0, i + 1, 1), i + 1, 0) for i in range(100)]
    o.ingest_run(recs)
    g.ingest_run(recs)
    res = g.scan_open(b"\x00\x00", b"\xff\xff", now, batch_size=1000,
                      validate_partition_hash=False, on_device_out=True)
    assert res.error == OK and res.dev is not None
    assert res.dev["count"] == 100
    assert res.dev["dev_keys"] and res.dev["dev_vals"]


@pytest.mark.parametrize("version", [0, 1, 2])
def test_value_schema_versions_parity(oracle_lib, hip_lib, version):
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    try:
        now = 1000
        for p in (o, g):
            p.set_envs({"pegasus.data_version": str(version)})
        recs = [(D.generate_key(b"vk", f"s{i}".encode()),
                 D.encode_value(f"val{i}".encode(), now + 50 if i == 0 else 0, 7, version),
                 i + 1, 0) for i in range(5)]
        o.ingest_run(recs)
        g.ingest_run(recs)
        for k, _, _, _ in recs:
            assert o.get(k, now) == g.get(k, now)
            assert o.ttl(k, now) == g.ttl(k, now)
        ro = o.scan_open(b"\x00\x00", b"\xff\xff", now, validate_partition_hash=False,
                         return_expire_ts=True)
        rg = g.scan_open(b"\x00\x00", b"\xff\xff", now, validate_partition_hash=False,
                         return_expire_ts=True)
        assert (ro.kvs, ro.expire_ts) == (rg.kvs, rg.expire_ts)
        assert o.manual_compact(now)[1] == g.manual_compact(now)[1]
    finally:
        o.close()
        g.close()


def test_env_caps_parity(oracle_lib, hip_lib):
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    try:
        now = 100
        recs = [(D.generate_key(b"caps", f"s{i:04d}".encode()),
                 D.encode_value(b"v", 0, i + 1, 1), i + 1, 0) for i in range(60)]
        for p in (o, g):
            p.ingest_run(recs)
            p.set_envs({"rocksdb.max_iteration_count": "13",
                        "rocksdb.multi_get_max_iteration_count": "9"})
        assert o.multi_get(b"caps", now) == g.multi_get(b"caps", now)
        assert _drain(o, now, batch_size=1000, validate_partition_hash=False) == \
               _drain(g, now, batch_size=1000, validate_partition_hash=False)
    finally:
        o.close()
        g.close()


def test_compact_stale_split_parity(oracle_lib, hip_lib):
    mask, pidx = 3, 1
    o = oracle_lib.open(1, pidx, -1)
    g = hip_lib.open(1, pidx, 0)
    try:
        recs = [(D.generate_key(f"sp{i:03d}".encode(), b""),
                 D.encode_value(b"v", 0, i + 1, 1), i + 1, 0) for i in range(64)]
        for p in (o, g):
            p.set_envs({"replica.split.validate_partition_hash": "true"})
            p.set_partition_version(mask)
            p.ingest_run(recs)
        so = o.manual_compact(100)
        sg = g.manual_compact(100)
        assert so == sg
        assert _drain(o, 100, validate_partition_hash=False) == \
               _drain(g, 100, validate_partition_hash=False)
    finally:
        o.close()
        g.close()


def test_default_ttl_v2_parity(oracle_lib, hip_lib):
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    try:
        now = 7000
        raw = D.generate_key(b"v2k", b"")
        for p in (o, g):
            p.set_envs({"pegasus.data_version": "2", "default_ttl": "100"})
            p.ingest_run([(raw, D.encode_value(b"data", 0, 5, 2), 1, 0)])
            p.manual_compact(now)
        assert o.ttl(raw, now) == g.ttl(raw, now) == (OK, 100)
        assert o.get(raw, now) == g.get(raw, now)
    finally:
        o.close()
        g.close()


def test_multi_get_fused_fallback_boundary(oracle_lib, hip_lib):
    """ranges around MG_MAX_ROWS (4096) cross between the fused single-launch
    path and the general view path — results must be identical (and the
    3000-iteration limiter cap applies either way)."""
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    try:
        now = 100
        hk = b"bighk"
        recs = [(D.generate_key(hk, f"s{i:05d}".encode()),
                 D.encode_value(f"v{i}".encode(), 0, i + 1, 1), i + 1, 0)
                for i in range(5000)]
        o.ingest_run(recs)
        g.ingest_run(recs)
        for kwargs in [
            dict(),  # 5000 rows -> fallback, caps at 3000 iterations -> INCOMPLETE
            dict(start_sortkey=b"s00100", stop_sortkey=b"s04000"),  # ~3900 rows
            dict(start_sortkey=b"s00100", stop_sortkey=b"s04196"),  # = 4096 rows
            dict(start_sortkey=b"s00000", stop_sortkey=b"s04000", reverse=True),
            dict(start_sortkey=b"s01000", stop_sortkey=b"s01100"),  # fused
        ]:
            ro = o.multi_get(hk, now, **kwargs)
            rg = g.multi_get(hk, now, **kwargs)
            assert ro == rg, kwargs
    finally:
        o.close()
        g.close()


@pytest.mark.parametrize("seed", range(2))
def test_compact_parity_lds_rank(oracle_lib, hip_lib, seed):
    """LDS-staged block rank (engine.rank_mode=lds) must match the oracle
    exactly, including heavy-skew fallback windows."""
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    try:
        g.set_envs({"engine.rank_mode": "lds"})
        rnd = random.Random(700 + seed)
        now = 5000
        _ingest_pair(o, g, _rand_runs(rnd, 5, 400, with_sortkeys=True, now=now))
        # skewed extra run: many records under one hashkey (stresses windows)
        skew = [(D.generate_key(b"zskew", f"s{i:05d}".encode()),
                 D.encode_value(b"sv", 0, 100_000 + i, 1), 100_000 + i, 0)
                for i in range(3000)]
        o.ingest_run(skew)
        g.ingest_run(skew)
        so = o.manual_compact(now)
        sg = g.manual_compact(now)
        assert g.last_compact_route()[0] == ROUTE_RANK_LDS
        assert so == sg
        assert _drain(o, now, validate_partition_hash=False) == \
               _drain(g, now, validate_partition_hash=False)
    finally:
        o.close()
        g.close()


def test_scale_parity_1m(oracle_lib, hip_lib):
    """Parity at bench-generator scale (1M keys, 8 runs + overlay): compaction
    stats must match the oracle AND the survivor count predicted analytically
    from the generator's splitmix selections (a size-independent property per
    the measurement contract — the full-size check that small differential
    tests can't give)."""
    import numpy as np

    from incubator_pegasus_amd import data as D2

    n_keys, n_runs, seed = 1_000_000, 8, D2.DEFAULT_SEED + 123
    runs = D2.build_point_table_runs(n_keys, n_runs, seed=seed, dup_fraction=0.10,
                                     delete_fraction=0.02)
    # analytic survivor count: overlay deletes kill their keys; everything
    # else survives (no TTL in this config)
    ids = np.arange(n_keys, dtype=np.uint64)
    h = D2.splitmix64(ids + np.uint64(seed))
    dup_sel = (D2.splitmix64(h) % np.uint64(1000)).astype(np.float64) / 1000.0
    # replicate the generator's float expression exactly: 0.10 + 0.02 is
    # 0.12000000000000001, which INCLUDES dup_sel == 0.120
    n_deleted = int(((dup_sel >= 0.10) & (dup_sel < 0.10 + 0.02)).sum())
    expected_survivors = n_keys - n_deleted

    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    try:
        for part in (o, g):
            for r in runs:
                part.ingest_run_arrays(np.ascontiguousarray(r["keys"]), r["koff"],
                                       np.ascontiguousarray(r["vals"]), r["voff"], r["sk"])
        now = 1000
        # spot reads pre-compaction
        probe_ids = D2.zipfian_ids(200, n_keys, seed=seed)
        probes = [bytes(k) for k in D2.make_raw_keys(probe_ids)]
        for k in probes:
            assert o.get(k, now) == g.get(k, now)
        # full-scan count parity
        for part in (o, g):
            part.set_envs({"rocksdb.max_iteration_count": str(2**31 - 1)})
        ro = o.scan_open(b"\x00\x00", b"\xff\xff", now, only_return_count=True,
                         validate_partition_hash=False, batch_size=2**31 - 1)
        rg = g.scan_open(b"\x00\x00", b"\xff\xff", now, only_return_count=True,
                         validate_partition_hash=False, batch_size=2**31 - 1)
        assert ro.kv_count == rg.kv_count == expected_survivors
        # compaction stats parity + analytic check
        so = o.manual_compact(now)
        sg = g.manual_compact(now)
        assert so == sg
        assert sg[1].output_records == expected_survivors
        assert sg[1].tombstones == n_deleted
        # post-compaction spot reads
        for k in probes[:50]:
            assert o.get(k, now) == g.get(k, now)
    finally:
        o.close()
        g.close()


def test_bloom_filter_parity_and_toggle(oracle_lib, hip_lib):
    """§8(f)3: per-run bloom filters are lossless — gets agree with the
    oracle (no blooms) for hits and misses, with the filter on and off."""
    import random as _r

    rnd = _r.Random(31)
    now = 1000
    for filt in ("common", "none"):
        o = oracle_lib.open(1, 0, -1)
        g = hip_lib.open(1, 0, 0)
        try:
            g.set_envs({"rocksdb.filter_type": filt})
            keys = _ingest_pair(o, g, _rand_runs(rnd, 5, 80, now=now))
            probes = keys + [D.generate_key(f"miss{i}".encode(), b"") for i in range(40)]
            for k in probes:
                assert o.get(k, now) == g.get(k, now), (filt, k)
            st_o = o.batch_get(probes, now)
            st_g = g.batch_get(probes, now)
            assert st_o == st_g
            # write path + compact rebuild blooms and stay correct
            g.put(b"bloomk", b"s", b"v")
            o.put(b"bloomk", b"s", b"v")
            assert o.get(D.generate_key(b"bloomk", b"s"), now) == \
                   g.get(D.generate_key(b"bloomk", b"s"), now)
            o.manual_compact(now)
            g.manual_compact(now)
            for k in probes[:60]:
                assert o.get(k, now) == g.get(k, now), (filt, "post-compact", k)
        finally:
            o.close()
            g.close()


def test_mixed_op_soak(oracle_lib, hip_lib, tmp_path):
    """Randomized interleaving of every ABI surface (writes, flush, ingest,
    gets, multi_gets, scans with paging, sortkey_count, compaction,
    checkpoint/restore, env flips) — engine must track the oracle through
    400 operations."""
    import random as _r

    rnd = _r.Random(20260915)
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    live_keys = set()
    now = 1000
    seq = [1_000_000]  # ingest seqno space above write seqnos

    def hk(i):
        return f"soak{i:03d}".encode()

    def sk(i):
        return f"s{i:02d}".encode()

    try:
        for step in range(400):
            op = rnd.randrange(100)
            if op < 35:  # put
                h, s = hk(rnd.randrange(40)), sk(rnd.randrange(8))
                v = f"v{step}".encode() * rnd.randrange(1, 4)
                exp = 0 if rnd.random() < 0.9 else now + rnd.randrange(1, 50)
                for p in (o, g):
                    p.put(h, s, v, exp)
                live_keys.add((h, s))
            elif op < 45:  # remove
                h, s = hk(rnd.randrange(40)), sk(rnd.randrange(8))
                for p in (o, g):
                    p.remove(h, s)
            elif op < 50:  # flush
                for p in (o, g):
                    p.flush()
            elif op < 60:  # point get parity
                h, s = hk(rnd.randrange(40)), sk(rnd.randrange(8))
                assert o.get(D.generate_key(h, s), now) == g.get(D.generate_key(h, s), now)
            elif op < 70:  # multi_get parity
                h = hk(rnd.randrange(40))
                kw = {}
                if rnd.random() < 0.3:
                    kw = dict(reverse=True)
                elif rnd.random() < 0.3:
                    kw = dict(sort_key_filter_type=FT_MATCH_PREFIX,
                              sort_key_filter_pattern=b"s0")
                assert o.multi_get(h, now, **kw) == g.multi_get(h, now, **kw)
            elif op < 78:  # sortkey_count
                h = hk(rnd.randrange(40))
                assert o.sortkey_count(h, now) == g.sortkey_count(h, now)
            elif op < 86:  # paged scan parity
                bs = rnd.choice([3, 17, 1000])
                assert _drain(o, now, batch_size=bs, validate_partition_hash=False) == \
                       _drain(g, now, batch_size=bs, validate_partition_hash=False)
            elif op < 92:  # compact (occasionally with default_ttl)
                envs = {"default_ttl": str(rnd.choice([0, 1234]))}
                for p in (o, g):
                    p.set_envs(envs)
                assert o.manual_compact(now) == g.manual_compact(now)
            elif op < 96:  # ingest a pre-built run
                n = rnd.randrange(1, 20)
                ks = sorted({D.generate_key(hk(rnd.randrange(40)), sk(rnd.randrange(8)))
                             for _ in range(n)})
                # seqnos must stay above the write-path floor, which each
                # put/remove advances; jump well past anything allocated so far
                seq[0] = max(seq[0], 1_000_000 + step * 10_000)
                recs = []
                for k in ks:
                    seq[0] += 1
                    recs.append((k, D.encode_value(f"ing{step}".encode(), 0, 0, 1), seq[0], 0))
                for p in (o, g):
                    p.ingest_run(recs)
            else:  # checkpoint round-trip spot check
                d = str(tmp_path / f"ck{step}")
                assert o.checkpoint(d, step) == 0
                # checkpoint flushes the memtable: do it on BOTH handles so
                # flush-point-dependent compact stats keep comparing equal
                # (see tools/soak.py / tools/stress_mixed.py)
                assert g.checkpoint(str(tmp_path / f"ckg{step}"), step) == 0
                o2 = oracle_lib.open(1, 0, -1)
                g2 = hip_lib.open(1, 0, 0)
                try:
                    assert o2.restore(d, step) == 0
                    assert g2.restore(d, step) == 0
                    assert _drain(o2, now, validate_partition_hash=False) == \
                           _drain(g2, now, validate_partition_hash=False)
                finally:
                    o2.close()
                    g2.close()
        # final full comparison
        assert _drain(o, now, validate_partition_hash=False, return_expire_ts=True) == \
               _drain(g, now, validate_partition_hash=False, return_expire_ts=True)
    finally:
        o.close()
        g.close()


def test_multi_get_batch_parity(oracle_lib, hip_lib):
    """Batched multi_get == N single multi_gets, on both backends, including
    shapes that force the engine's per-request fallback."""
    import random as _r

    rnd = _r.Random(77)
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    try:
        now = 1000
        hks = [f"bmg{i:03d}".encode() for i in range(50)]
        seq = 1
        recs = {}
        for hk in hks:
            for s in range(rnd.randrange(0, 12)):
                expire = 0 if rnd.random() < 0.8 else (now - 1 if rnd.random() < 0.5 else now + 50)
                recs[D.generate_key(hk, f"s{s:02d}".encode())] = \
                    D.encode_value(f"{hk}{s}".encode(), expire, seq, 1)
        records = []
        for k in sorted(recs):
            records.append((k, recs[k], seq, 0))
            seq += 1
        o.ingest_run(records)
        g.ingest_run(records)
        ask = hks + [b"bmg-missing", b"bmg0"]  # misses included
        for kwargs in [
            dict(),
            dict(no_value=True),
            dict(reverse=True),
            dict(max_kv_count=3),
            dict(sort_key_filter_type=FT_MATCH_POSTFIX, sort_key_filter_pattern=b"1"),
            dict(start_sortkey=b"s02"),  # engine falls back per request
        ]:
            eo, go_ = o.multi_get_batch(ask, now, **kwargs), g.multi_get_batch(ask, now, **kwargs)
            assert eo == go_, kwargs
            # and equals the per-request loop
            err, groups = go_
            for hk, (gerr, kvs) in zip(ask, groups):
                assert (gerr, kvs) == g.multi_get(hk, now, **kwargs), (hk, kwargs)
    finally:
        o.close()
        g.close()


def test_prefix_skip_edge_queries(pair):
    """Runs whose keys share a long (>=8B) prefix engage the device
    prefix-skip search path; queries that diverge inside, fall short of, or
    exactly equal the shared prefix must take the fallback compare and still
    match the oracle bit for bit."""
    o, g = pair
    now = 1000
    # hashkeys "commonprefix-NNNN" -> every raw key shares >=14 leading bytes
    hks = [f"commonprefix-{i:04d}".encode() for i in range(64)]
    seq = 1
    records = []
    for i, hk in enumerate(hks):
        records.append((D.generate_key(hk, b""), D.encode_value(b"v%d" % i, 0, i + 1, 1), seq, 0))
        seq += 1
    records.sort()
    o.ingest_run(records)
    g.ingest_run(records)
    # second run: varying sortkey lengths -> variable stride, shared prefix;
    # exercises the offset-pair search branch with prefix skip
    records2 = []
    for i, hk in enumerate(hks[:32]):
        sk = b"s" * (i % 5)
        records2.append((D.generate_key(hk, sk), D.encode_value(b"w%d" % i, 0, 0, 1), seq, 0))
        seq += 1
    records2.sort()
    o.ingest_run(records2)
    g.ingest_run(records2)
    probes = (
        [D.generate_key(hk, b"") for hk in hks]       # shares prefix (skip path)
        + [D.generate_key(b"commonprefiy", b""),      # diverges after 8B
           D.generate_key(b"aommonprefix-0000", b""), # diverges in first word, below
           D.generate_key(b"zommonprefix-0000", b""), # diverges in first word, above
           D.generate_key(b"common", b""),            # shorter than the prefix
           D.generate_key(b"commonprefix-", b""),     # exactly the shared hashkey stem
           D.generate_key(b"commonprefix-0031", b"x")]  # longer than a run key
    )
    for k in probes:
        assert o.get(k, now) == g.get(k, now), k
    assert o.batch_get(probes, now) == g.batch_get(probes, now)
    for hk in [b"commonprefix-0005", b"common", b"zommonprefix"]:
        assert o.sortkey_count(hk, now) == g.sortkey_count(hk, now), hk
    o.manual_compact(now)
    g.manual_compact(now)
    assert o.num_records() == g.num_records()
    for k in probes:
        assert o.get(k, now) == g.get(k, now), k


@pytest.mark.parametrize("n_keys", [2_000, 300_000])
def test_compact_parity_ldst_rank(oracle_lib, hip_lib, n_keys):
    """LDS tail-word rank (engine.rank_mode=ldst) must match the oracle
    bit-exactly on eligible (uniform fixed-width, shared-prefix) tables —
    at 2K records the kernel takes its internal no-bound-table fallback, at
    300K it runs the staged path proper.  Mixed-width tables (covered by
    test_compact_parity_lds_rank's shapes) dispatch back to the standard
    kernel at the host."""
    import numpy as np

    from incubator_pegasus_amd import data as D2

    runs = D2.build_point_table_runs(n_keys, 6, seed=D2.DEFAULT_SEED + 77,
                                     dup_fraction=0.12, delete_fraction=0.03,
                                     ttl_fraction=0.05, ttl_expire_ts=500)
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    try:
        g.set_envs({"engine.rank_mode": "ldst"})
        for part in (o, g):
            for r in runs:
                part.ingest_run_arrays(np.ascontiguousarray(r["keys"]), r["koff"],
                                       np.ascontiguousarray(r["vals"]), r["voff"], r["sk"])
        now = 1000
        so = o.manual_compact(now)
        sg = g.manual_compact(now)
        assert g.last_compact_route()[0] == ROUTE_RANK_LDST
        assert so == sg
        assert o.num_records() == g.num_records()
        probe_ids = D2.zipfian_ids(300, n_keys, seed=7)
        for k in [bytes(x) for x in D2.make_raw_keys(probe_ids)]:
            assert o.get(k, now) == g.get(k, now), k
        assert _drain(o, now, validate_partition_hash=False) == \
               _drain(g, now, validate_partition_hash=False)
    finally:
        o.close()
        g.close()


def test_ldst_fallback_branches(oracle_lib, hip_lib):
    """Two ldst dispatch branches the main suite doesn't reach: more runs
    than the kernel stages (R > 16 -> in-kernel fallback to global probes)
    and uniform-width runs whose prefixes differ across runs (host
    eligibility check fails -> standard kernel)."""
    now = 1000
    # (a) 18 eligible runs: kernel launches staged variant, falls back inside
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    try:
        g.set_envs({"engine.rank_mode": "ldst"})
        seq = 1
        for run in range(18):
            recs = []
            for i in range(40):
                k = D.generate_key(f"fb{(run * 7 + i * 3) % 120:04d}".encode(), b"")
                recs.append((k, D.encode_value(b"v%d" % run, 0, seq, 1), seq, 0))
                seq += 1
            recs = sorted({k: r for k, *r in [(k, k, v, s, kd) for k, v, s, kd in recs]}.items())
            recs = [(k, v, s, kd) for k, (_, v, s, kd) in recs]
            o.ingest_run(recs)
            g.ingest_run(recs)
        assert o.manual_compact(now) == g.manual_compact(now)
        assert g.last_compact_route()[0] == ROUTE_RANK_LDST  # the fallback is in the kernel
        assert _drain(o, now, validate_partition_hash=False) == \
               _drain(g, now, validate_partition_hash=False)
    finally:
        o.close()
        g.close()
    # (b) same fixed width, different cross-run prefixes: host falls back
    o = oracle_lib.open(1, 0, -1)
    g = hip_lib.open(1, 0, 0)
    try:
        g.set_envs({"engine.rank_mode": "ldst"})
        seq = 1
        for pfx in (b"aaaaaaaaaa", b"bbbbbbbbbb", b"cccccccccc"):
            recs = []
            for i in range(50):
                k = D.generate_key(pfx + b"%04d" % i, b"")
                recs.append((k, D.encode_value(b"w", 0, seq, 1), seq, 0))
                seq += 1
            o.ingest_run(recs)
            g.ingest_run(recs)
        for i in (0, 7, 49):
            for pfx in (b"aaaaaaaaaa", b"bbbbbbbbbb", b"cccccccccc"):
                k = D.generate_key(pfx + b"%04d" % i, b"")
                assert o.get(k, now) == g.get(k, now), k
        assert o.manual_compact(now) == g.manual_compact(now)
        assert g.last_compact_route()[0] == ROUTE_RANK_GLOBAL
        assert _drain(o, now, validate_partition_hash=False) == \
               _drain(g, now, validate_partition_hash=False)
    finally:
        o.close()
        g.close()


def test_split_compact_pipeline_parity(oracle_lib, hip_lib):
    """begin() on several partitions then finish() on each (the bench's
    pipelined pattern) must produce the same stats and surviving data as
    one-shot compacts against the oracle."""
    import numpy as np

    from incubator_pegasus_amd import data as D2

    now = 1000
    parts = []
    try:
        for p in range(4):
            o = oracle_lib.open(1, p, -1)
            g = hip_lib.open(1, p, 0)
            runs = D2.build_point_table_runs(120_000 + p * 17, 5, seed=D2.DEFAULT_SEED + p,
                                             dup_fraction=0.1, delete_fraction=0.02,
                                             ttl_fraction=0.04, ttl_expire_ts=500)
            for r in runs:
                for eng in (o, g):
                    eng.ingest_run_arrays(np.ascontiguousarray(r["keys"]), r["koff"],
                                          np.ascontiguousarray(r["vals"]), r["voff"], r["sk"])
            parts.append((o, g))
        for o, g in parts:
            assert g.manual_compact_begin(now) == 0
        for o, g in parts:
            so = o.manual_compact(now)
            sg = g.manual_compact_finish()
            assert so == sg
            assert o.num_records() == g.num_records()
            probe_ids = D2.zipfian_ids(100, 120_000, seed=5)
            for k in [bytes(x) for x in D2.make_raw_keys(probe_ids)]:
                assert o.get(k, now) == g.get(k, now), k
    finally:
        for o, g in parts:
            o.close()
            g.close()
