"""GPU parity for batched writes with timetags, rrdb_write_batch_timetag
(include/rrdb_engine_ext.h).

The CPU oracle has no such call.  The expected results are the model's
(tests/test_timetag_batch_model.py, which proves it on the CPU against a
literal restatement of the reference and against the oracle's reads); the
expected state is an oracle handle prepared like the engine's that then
ingested the model's run.  Physical parity goes through checkpoints, which
both backends write in one format.  The sequence floor is compared with the
model's, not the oracle's: rrdb_ingest_run sets its own floor to the largest
seqno + 1, and the batch spends a seqno on every op, ignored ones included.
"""
import ctypes as C

import numpy as np
import pytest

from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import INVALID_ARGUMENT, OK, _pack
from test_minor_compact_model import stats_dict
from test_timetag_batch_model import (CASE_PARAMS, CHAIN_LENGTHS, CHAIN_PATTERNS,
                                      STAT_FIELDS, T, chain_ops, env_ttl, env_version, gen_tt,
                                      ingest_model_run, open_prepared, timetag_model)
from test_write_batch_model import NOW, read_checkpoint
from test_write_batch_model import STAT_FIELDS as WB_STAT_FIELDS

pytestmark = pytest.mark.gpu

PHASES = ("wbt_sort", "wbt_lookup", "wbt_apply", "wbt_emit", "wbt_total", "wbt_stage",
          "wbt_upload")


def _stats(st):
    return {f: getattr(st, f) for f in STAT_FIELDS}


def _same_checkpoint(g, o, tmp_path, tag="a"):
    """every run and the manifest fields but the floor, engine against oracle;
    returns the engine's manifest"""
    mg, rg = read_checkpoint(g, tmp_path / ("g" + tag))
    mo, ro = read_checkpoint(o, tmp_path / ("o" + tag))
    assert {k: v for k, v in mg.items() if k != "next_seq_floor"} == \
           {k: v for k, v in mo.items() if k != "next_seq_floor"}
    assert len(rg) == len(ro)
    for i, (a, b) in enumerate(zip(rg, ro)):
        for col in ("n", "sk", "koff", "voff", "keys", "vals"):
            assert a[col] == b[col], "run %d column %s differs" % (i, col)
    return mg


def _same_point_reads(g, o, keys, now):
    assert g.batch_get(keys, now) == o.batch_get(keys, now)
    for k in keys:
        assert g.ttl(k, now) == o.ttl(k, now), k


def _check_against_model(g, o, floor, layers, ops, envs, now, tmp_path, compact=True):
    """one batch on g; o is the oracle prepared alike"""
    err, applied, st = g.write_batch_timetag(ops, now)
    assert err == OK
    want_applied, want_stats, run, new_floor = timetag_model(
        layers, ops, floor, env_version(envs), env_ttl(envs), now)
    assert applied == want_applied
    assert _stats(st) == want_stats
    ingest_model_run(o, run)
    assert g.memtable_entries() == 0
    assert g.num_runs() == o.num_runs()
    assert g.num_records() == o.num_records()
    man = _same_checkpoint(g, o, tmp_path)
    assert man["next_seq_floor"] == new_floor == floor + len(ops)
    keys = sorted({op[0] for op in ops})
    _same_point_reads(g, o, keys, now)
    if compact:
        (eg, sg), (eo, so) = g.manual_compact(now), o.manual_compact(now)
        assert eg == eo == OK
        assert stats_dict(sg) == stats_dict(so)
        _same_checkpoint(g, o, tmp_path, "b")
    return st


# 1 the cases -----------------------------------------------------------------

@pytest.mark.parametrize("case,n", CASE_PARAMS)
def test_batch_equals_the_sequence(hip_lib, oracle_lib, tmp_path, case, n):
    _, gen, envs, now = case
    layers, ops = gen(n)
    g, floor = open_prepared(hip_lib, 0, envs, layers, now)
    o, _ = open_prepared(oracle_lib, -1, envs, layers, now)
    try:
        _check_against_model(g, o, floor, layers, ops, envs, now, tmp_path)
        for ph in PHASES:
            assert g.phase_ms(ph) >= 0.0, ph
    finally:
        g.close()
        o.close()


# 2 one key: the lane walk, the wave walk and its fallback --------------------

@pytest.mark.parametrize("pattern", CHAIN_PATTERNS)
@pytest.mark.parametrize("length", CHAIN_LENGTHS)
def test_one_key_chain(hip_lib, oracle_lib, tmp_path, pattern, length):
    """the default threshold, one that sends every chain to a wave and one
    that keeps every chain on a lane give the model's results"""
    ops = chain_ops(pattern, length)
    k = ops[0][0]
    base = [{k: (b"base", 0, 20)}, {}] if pattern == "mix" else [{}]
    for lane_max in (None, 4, 4096):
        g, floor = open_prepared(hip_lib, 0, {}, base, NOW)
        o, _ = open_prepared(oracle_lib, -1, {}, base, NOW)
        try:
            if lane_max is not None:
                assert g.set_envs({"engine.wbt_lane_max": str(lane_max)}) == OK
            want_applied, want_stats, run, _ = timetag_model(base, ops, floor, 1, 0, NOW)
            if pattern == "rising":
                assert want_applied == [1] * length
            if pattern == "falling":
                assert want_applied == [1] + [0] * (length - 1)
            err, applied, st = g.write_batch_timetag(ops, NOW)
            assert err == OK
            assert applied == want_applied, lane_max
            assert _stats(st) == want_stats, lane_max
            ingest_model_run(o, run)
            man = _same_checkpoint(g, o, tmp_path, "l%s" % lane_max)
            assert man["next_seq_floor"] == floor + length
            assert g.get(k, NOW) == o.get(k, NOW)
        finally:
            g.close()
            o.close()


# 3 the relation to rrdb_write_batch -------------------------------------------

@pytest.mark.parametrize("n", [T + 1, 3 * T + 7])
def test_null_timetags_and_verify_is_write_batch(hip_lib, tmp_path, n):
    layers, ops = gen_tt(n, 51, weights=(0.3, 0.7, 0.0))
    plain = [op[:3] for op in ops]
    a, floor = open_prepared(hip_lib, 0, {}, layers, NOW)
    b, _ = open_prepared(hip_lib, 0, {}, layers, NOW)
    try:
        keys, koffs = _pack([o[0] for o in plain])
        vals, voffs = _pack([o[1] if o[1] is not None else b"" for o in plain])
        expire = np.array([o[2] if o[1] is not None else 0 for o in plain], dtype=np.uint32)
        kinds = np.array([0 if o[1] is not None else 1 for o in plain], dtype=np.uint8)
        err, applied, st = a.write_batch_timetag_arrays(keys, koffs, vals, voffs, expire, kinds,
                                                        None, None, NOW)
        assert err == OK and applied.tolist() == [1] * n
        err, wst = b.write_batch(plain, NOW)
        assert err == OK
        assert {f: getattr(st, f) for f in WB_STAT_FIELDS} == \
               {f: getattr(wst, f) for f in WB_STAT_FIELDS}
        assert (st.applied, st.ignored) == (n, 0)
        ca, cb = read_checkpoint(a, tmp_path / "a"), read_checkpoint(b, tmp_path / "b")
        assert ca == cb and ca[0]["next_seq_floor"] == floor + n
        # applied and stats may be NULL as well
        rc = a._L.rrdb_write_batch_timetag(
            a._h, n, *[x.ctypes.data_as(C.c_void_p)
                       for x in (keys, koffs, vals, voffs, expire, kinds)],
            None, None, NOW, None, None)
        assert rc == OK and a.num_runs() == b.num_runs() + 1
    finally:
        a.close()
        b.close()


# 4 nothing applied, pending entries --------------------------------------------

def test_everything_ignored_adds_no_run(hip_lib, tmp_path):
    keys = [D.generate_key(b"ign", b"%05d" % i) for i in range(T + 1)]
    layers = [{k: (b"stored", 0, 1000 + i) for i, k in enumerate(keys)}, {}]
    ops = [(k, b"stale", 0, 1000 + i - (i % 2), 1) for i, k in enumerate(keys)]
    ops += ops[:40]  # a chain of two on some keys
    g, floor = open_prepared(hip_lib, 0, {}, layers, NOW)
    try:
        before = read_checkpoint(g, tmp_path / "before")
        err, applied, st = g.write_batch_timetag(ops, NOW)
        assert err == OK
        assert applied == [0] * len(ops)
        assert _stats(st) == dict(input_ops=len(ops), applied=0, ignored=len(ops),
                                  output_records=0, superseded=0, puts=0, removes=0,
                                  key_bytes=0, value_bytes=0)
        after = read_checkpoint(g, tmp_path / "after")
        assert after[1] == before[1] and after[0]["n_runs"] == before[0]["n_runs"] == 1
        assert after[0]["next_seq_floor"] == floor + len(ops)
        assert g.get(keys[0], NOW) == (OK, b"stored")
    finally:
        g.close()


def test_pending_memtable_entries_are_flushed_first(hip_lib):
    """a record rrdb_put wrote carries timetag 0: a verified PUT with timetag 1
    beats it, one with timetag 0 loses against it"""
    ka, kb = D.generate_key(b"pend", b"a"), D.generate_key(b"pend", b"b")
    g = hip_lib.open(1, 0, 0)
    try:
        assert g.put(b"pend", b"a", b"put-a", 0, NOW) == OK
        assert g.put(b"pend", b"b", b"put-b", 0, NOW) == OK
        assert g.memtable_entries() == 2 and g.num_runs() == 0
        err, applied, st = g.write_batch_timetag([(ka, b"dup-a", 0, 1, 1), (kb, b"dup-b", 0, 0, 1)],
                                                 NOW)
        assert err == OK and applied == [1, 0]
        assert (st.applied, st.ignored, st.output_records) == (1, 1, 1)
        assert g.memtable_entries() == 0 and g.num_runs() == 2
        assert g.get(ka, NOW) == (OK, b"dup-a")
        assert g.get(kb, NOW) == (OK, b"put-b")
    finally:
        g.close()


# 5 rejections ----------------------------------------------------------------

def _arrays(ops):
    keys, koffs = _pack([op[0] for op in ops])
    vals, voffs = _pack([op[1] if op[1] is not None else b"" for op in ops])
    return [keys, koffs, vals, voffs,
            np.array([op[2] for op in ops], dtype=np.uint32),
            np.array([0 if op[1] is not None else 1 for op in ops], dtype=np.uint8),
            np.array([op[3] for op in ops], dtype=np.uint64),
            np.array([op[4] for op in ops], dtype=np.uint8)]


def _bad_inputs():
    """rrdb_write_batch's malformed inputs (tests/test_write_batch_gpu.py)"""
    good = [(D.generate_key(b"hk%d" % i, b"s"), b"v%d" % i, 0, 5 + i, i % 2) for i in range(6)]

    def edit(col, idx, value):
        a = _arrays(good)
        a[col][idx] = value
        return a

    def with_key(k):
        return _arrays(good[:3] + [(k, b"v", 0, 9, 1)] + good[3:])

    return {
        "key_offs-start": edit(1, 0, 1),
        "key_offs-decrease": edit(1, 3, 2),
        "val_offs-start": edit(3, 0, 1),
        "val_offs-decrease": edit(3, 4, 1),
        "key-empty": with_key(b""),
        "key-one-byte": with_key(b"\x00"),
        "hklen-beyond-key": with_key(b"\x00\x05abc"),
        "hklen-ffff": with_key(b"\xff\xff" + b"h" * 0xFFFF + b"s"),
        "kind-2": edit(5, 2, 2),
    }


def test_rejections_leave_the_handle_alone(hip_lib, oracle_lib, tmp_path):
    """p has pending memtable entries that a rejected call must not flush; q
    has none, so its checkpoint can be taken after every rejection"""
    layers, ops = gen_tt(300, 81)
    p, _ = open_prepared(hip_lib, 0, {}, layers, NOW)
    q, floor = open_prepared(hip_lib, 0, {}, layers[:2] + [{}], NOW)
    o, _ = open_prepared(oracle_lib, -1, {}, layers[:2] + [{}], NOW)
    try:
        before_p = (p.num_runs(), p.num_records(), p.memtable_entries())
        assert before_p[2] == len(layers[2]) > 0
        before_q = read_checkpoint(q, tmp_path / "q0")
        shape_q = (q.num_runs(), q.memtable_entries())
        tag = [0]

        def unchanged(name):
            assert (p.num_runs(), p.num_records(), p.memtable_entries()) == before_p, name
            assert (q.num_runs(), q.memtable_entries()) == shape_q, name
            tag[0] += 1
            assert read_checkpoint(q, tmp_path / ("q%d" % tag[0])) == before_q, name

        for name, arrays in _bad_inputs().items():
            for h in (p, q):
                err, _, st = h.write_batch_timetag_arrays(*arrays, NOW)
                assert err == INVALID_ARGUMENT, name
                assert _stats(st) == dict.fromkeys(STAT_FIELDS, 0), name
            unchanged(name)
        # more ops than the 32-bit index carries: refused before any array is read
        a = _arrays(ops[:4])
        for h in (p, q):
            rc = h._L.rrdb_write_batch_timetag(
                h._h, 2**31, *[x.ctypes.data_as(C.c_void_p) for x in a], NOW, None, None)
            assert rc == INVALID_ARGUMENT
        unchanged("2^31 ops")
        for h in (p, q):
            assert h.scan_count_begin(b"\x00\x00", b"\xff\xff", NOW,
                                      validate_partition_hash=False) == OK
        # (the count scan's begin has flushed p's memtable: compare from here)
        before_p = (p.num_runs(), p.num_records(), p.memtable_entries())
        for h in (p, q):
            assert h.write_batch_timetag(ops, NOW)[0] == INVALID_ARGUMENT
        assert (p.num_runs(), p.num_records(), p.memtable_entries()) == before_p
        for h in (p, q):
            assert h.scan_count_finish()[0] == OK
            assert h.manual_compact_begin(NOW) == OK
            assert h.write_batch_timetag(ops, NOW)[0] == INVALID_ARGUMENT
        assert (p.num_runs(), p.num_records(), p.memtable_entries()) == before_p
        assert (q.num_runs(), q.memtable_entries()) == shape_q
        for h in (p, q):
            assert h.manual_compact_finish()[0] == OK
        assert o.manual_compact(NOW)[0] == OK
        # the next accepted batch takes the seqnos the rejected ones left alone.
        # The compaction dropped tombstones and expired records, which reads as
        # before: the model still takes the layers.
        _check_against_model(q, o, floor, layers[:2] + [{}], ops, {}, NOW, tmp_path,
                             compact=False)
    finally:
        p.close()
        q.close()
        o.close()


def test_empty_batch_does_nothing(hip_lib):
    g = hip_lib.open(1, 0, 0)
    try:
        assert g.put(b"hk", b"sk", b"1", 0, 0) == OK
        err, applied, st = g.write_batch_timetag([], NOW)
        assert err == OK and applied == []
        assert _stats(st) == dict.fromkeys(STAT_FIELDS, 0)
        assert g.num_runs() == 0 and g.memtable_entries() == 1
    finally:
        g.close()

