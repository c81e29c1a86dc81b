"""GPU parity for batched counter increments, rrdb_incr_batch
(include/rrdb_engine_ext.h).

The CPU oracle has no incr call: the expected state is the oracle driven by
the contract's sequence (flush; per op get + ttl, and a put on success; flush)
through tests/test_incr_batch_model.py's drive_sequence, which explains its
two handles.  Physical parity goes through checkpoints, which both backends
write in one format.  The case lists live in the model file, which proves every
one of them against the oracle on the CPU; every case runs at T + 1 and
3T + 7 ops, the smallest sizes that cross the sort's tile and merge boundaries.
"""
import ctypes as C

import numpy as np
import pytest

from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import INVALID_ARGUMENT, OK, _pack
from test_incr_batch_model import (CASE_PARAMS, CASES, INT64_MAX, INT64_MIN, STAT_FIELDS, T,
                                   drive_sequence, env_ttl, env_version, gen_hot_key,
                                   gen_mixed_fail, gen_ttl, incr_model, open_prepared, overlay)
from test_minor_compact_model import stats_dict
from test_write_batch_gpu import _same_checkpoint
from test_write_batch_model import NOW, read_checkpoint

pytestmark = pytest.mark.gpu

PHASES = ("incr_sort", "incr_lookup", "incr_apply", "incr_emit", "incr_total")


def _stats(st):
    return {f: getattr(st, f) for f in STAT_FIELDS}


def _trio(hip_lib, oracle_lib, envs, layers, now):
    """the engine, and the oracle's reader and state handles, prepared alike"""
    g, floor = open_prepared(hip_lib, 0, envs, layers, now)
    reader, _ = open_prepared(oracle_lib, -1, envs, layers, now)
    state, _ = open_prepared(oracle_lib, -1, envs, layers, now)
    return g, reader, state, floor


def _same_point_reads(g, o, keys, now):
    assert g.batch_get(keys, now) == o.batch_get(keys, now)
    for k in keys:
        assert g.ttl(k, now) == o.ttl(k, now), k


# 1 the cases -----------------------------------------------------------------

@pytest.mark.parametrize("case,n", CASE_PARAMS)
def test_batch_equals_the_sequence(hip_lib, oracle_lib, tmp_path, case, n):
    _, gen, envs, now = case
    layers, ops = gen(n)
    g, reader, state, floor = _trio(hip_lib, oracle_lib, envs, layers, now)
    try:
        err, new_values, errors, st = g.incr_batch(ops, now)
        assert err == OK
        want_v, want_e = drive_sequence(reader, state, ops, now)
        assert new_values == want_v
        assert errors == want_e
        _, _, want_stats, run, new_floor = incr_model(
            overlay(layers, env_ttl(envs), now), ops, floor, env_version(envs), env_ttl(envs),
            now)
        assert _stats(st) == want_stats
        assert g.memtable_entries() == 0
        assert g.num_runs() == state.num_runs()
        assert g.num_records() == state.num_records()
        man = _same_checkpoint(g, state, tmp_path)
        assert man["next_seq_floor"] == new_floor
        for ph in PHASES:
            assert g.phase_ms(ph) >= 0.0, ph
        keys = sorted({op[0] for op in ops})
        _same_point_reads(g, state, keys, now)
        (eg, sg), (eo, so) = g.manual_compact(now), state.manual_compact(now)
        assert eg == eo == OK
        assert stats_dict(sg) == stats_dict(so)
        _same_checkpoint(g, state, tmp_path, "b")
    finally:
        g.close()
        reader.close()
        state.close()


@pytest.mark.parametrize("n", [T + 1, 3 * T + 7])
def test_one_key_results_are_the_running_sums(hip_lib, n):
    k = D.generate_key(b"only", b"one")
    incs = [(i * 7919) % 2001 - 1000 for i in range(n)]
    g = hip_lib.open(1, 0, 0)
    try:
        assert g.put(b"only", b"one", b"0x7fffffff", 0, NOW) == OK  # pending: flushed first
        err, new_values, errors, st = g.incr_batch([(k, v, 0) for v in incs], NOW)
        assert err == OK and errors == [OK] * n
        assert new_values == list(np.cumsum(np.array(incs, dtype=np.int64)) + 0x7FFFFFFF)
        assert (st.applied, st.output_records, st.failed_parse, st.failed_range) == (n, 1, 0, 0)
        assert g.num_runs() == 2
        assert g.get(k, NOW) == (OK, b"%d" % new_values[-1])
    finally:
        g.close()


def test_range_edges_spelled_out(hip_lib):
    """the issue's four chains, expected values written down by hand"""
    ka, kb, kc = (D.generate_key(b"edge", s) for s in (b"a", b"b", b"c"))
    g = hip_lib.open(1, 0, 0)
    try:
        for sk, v in ((b"a", INT64_MAX - 1), (b"b", INT64_MIN), (b"c", -1)):
            assert g.put(b"edge", sk, b"%d" % v, 0, NOW) == OK
        ops = [(ka, 1, 0), (kb, -1, 0), (ka, 1, 0), (kc, INT64_MIN, 0), (ka, -5, 0), (kb, 1, 0),
               (ka, 10, 0)]
        err, nv, er, st = g.incr_batch(ops, NOW)
        assert err == OK
        assert nv == [INT64_MAX, INT64_MIN, INT64_MAX, -1, INT64_MAX - 5, INT64_MIN + 1,
                      INT64_MAX - 5]
        assert er == [OK, INVALID_ARGUMENT, INVALID_ARGUMENT, INVALID_ARGUMENT, OK, OK,
                      INVALID_ARGUMENT]
        assert (st.applied, st.failed_range, st.failed_parse, st.output_records) == (3, 4, 0, 2)
        assert g.get(ka, NOW) == (OK, b"%d" % (INT64_MAX - 5))
        assert g.get(kc, NOW) == (OK, b"-1")
    finally:
        g.close()


# 2 no run, seqnos, split batches ---------------------------------------------

def test_all_ops_fail_adds_no_run(hip_lib, oracle_lib, tmp_path):
    _, gen, envs, now = [c for c in CASES if c[0] == "all-fail"][0]
    layers, ops = gen(T + 1)
    g, floor = open_prepared(hip_lib, 0, envs, layers, now)
    try:
        before = read_checkpoint(g, tmp_path / "before")
        runs = g.num_runs()
        err, nv, er, st = g.incr_batch(ops, now)
        assert err == OK
        assert nv == [0] * len(ops) and er == [INVALID_ARGUMENT] * len(ops)
        assert (st.applied, st.failed_parse, st.output_records, st.key_bytes) == \
               (0, len(ops), 0, 0)
        assert g.num_runs() == runs
        after = read_checkpoint(g, tmp_path / "after")
        assert after == before and after[0]["next_seq_floor"] == floor
    finally:
        g.close()


def test_failed_ops_take_no_seqno_and_a_later_remove_wins(hip_lib, oracle_lib, tmp_path):
    layers, ops = gen_mixed_fail(T + 1, 61)
    g, reader, state, floor = _trio(hip_lib, oracle_lib, {}, layers, NOW)
    try:
        err, nv, er, st = g.incr_batch(ops, NOW)
        assert err == OK
        assert (nv, er) == drive_sequence(reader, state, ops, NOW)
        assert 0 < st.applied < len(ops) and st.applied == er.count(OK)
        man = _same_checkpoint(g, state, tmp_path)
        assert man["next_seq_floor"] == floor + st.applied
        # the newest run's seqnos are exactly floor .. floor + applied - 1, no gaps beyond
        sk = np.frombuffer(read_checkpoint(g, tmp_path / "sk")[1][-1]["sk"], dtype=np.uint64)
        assert int(sk.min() >> 1) >= floor and int(sk.max() >> 1) == floor + st.applied - 1
        # a remove issued afterwards gets the next seqno and outranks the counter
        written = [op[0] for op, e in zip(ops, er) if e == OK]
        victim = written[-1]
        assert g.get(victim, NOW)[0] == OK
        assert g.write_batch([(victim, None, 0)])[0] == OK
        hk, sk_ = D.restore_key(victim)
        assert state.remove(hk, sk_) == OK and state.flush() == OK
        assert g.get(victim, NOW)[0] != OK
        _same_checkpoint(g, state, tmp_path, "b")
    finally:
        g.close()
        reader.close()
        state.close()


@pytest.mark.parametrize("name,gen,cut", [
    ("hot-key", lambda: gen_hot_key(T + 1, 71), 777),
    ("ttl", lambda: gen_ttl(T + 1, 72), 1200),
    ("mixed-fail", lambda: gen_mixed_fail(3 * T + 7, 73), 2 * T + 5),
])
def test_split_batch_gives_the_same_results(hip_lib, oracle_lib, tmp_path, name, gen, cut):
    layers, ops = gen()
    one, _ = open_prepared(hip_lib, 0, {}, layers, NOW)
    two, _ = open_prepared(hip_lib, 0, {}, layers, NOW)
    try:
        err, nv, er, _ = one.incr_batch(ops, NOW)
        assert err == OK
        e1, nv1, er1, s1 = two.incr_batch(ops[:cut], NOW)
        e2, nv2, er2, s2 = two.incr_batch(ops[cut:], NOW)
        assert e1 == e2 == OK
        assert nv1 + nv2 == nv and er1 + er2 == er
        keys = sorted({op[0] for op in ops})
        _same_point_reads(two, one, keys, NOW)
        m1, _ = read_checkpoint(one, tmp_path / "one")
        m2, _ = read_checkpoint(two, tmp_path / "two")
        assert m1["next_seq_floor"] == m2["next_seq_floor"]
        assert m2["n_runs"] == m1["n_runs"] + 1
    finally:
        one.close()
        two.close()


def test_empty_batch_does_nothing(hip_lib):
    g = hip_lib.open(1, 0, 0)
    try:
        assert g.put(b"hk", b"sk", b"1", 0, 0) == OK
        err, nv, er, st = g.incr_batch([], NOW)
        assert err == OK and nv == [] and er == []
        assert _stats(st) == dict.fromkeys(STAT_FIELDS, 0)
        assert g.num_runs() == 0 and g.memtable_entries() == 1
    finally:
        g.close()


def test_null_directives_and_null_outputs(hip_lib):
    """expire_ts_seconds, new_values and errors may all be NULL"""
    ops = [(D.generate_key(b"n", b"%d" % (i % 5)), i, 0) for i in range(40)]
    keys, koffs = _pack([o[0] for o in ops])
    inc = np.array([o[1] for o in ops], dtype=np.int64)
    a, b = hip_lib.open(1, 0, 0), hip_lib.open(1, 0, 0)
    try:
        err, nv, er, st = a.incr_batch_arrays(keys, koffs, inc, None, NOW)
        assert err == OK and st.applied == 40 and st.output_records == 5
        rc = b._L.rrdb_incr_batch(b._h, 40, keys.ctypes.data_as(C.c_void_p),
                                  koffs.ctypes.data_as(C.c_void_p),
                                  inc.ctypes.data_as(C.c_void_p), None, NOW, None, None, None)
        assert rc == OK
        probe = sorted({o[0] for o in ops})
        assert a.batch_get(probe, NOW) == b.batch_get(probe, NOW)
        assert a.get(probe[0], NOW) == (OK, b"%d" % sum(range(0, 40, 5)))
    finally:
        a.close()
        b.close()


# 3 rejections ----------------------------------------------------------------

def _arrays(ops):
    keys, koffs = _pack([op[0] for op in ops])
    return [keys, koffs, np.array([op[1] for op in ops], dtype=np.int64),
            np.array([op[2] for op in ops], dtype=np.int32)]


def _bad_inputs():
    good = [(D.generate_key(b"hk%d" % i, b"s"), i + 1, 0) for i in range(6)]

    def edit(col, idx, value):
        a = _arrays(good)
        a[col][idx] = value
        return a

    def with_key(k):
        return _arrays(good[:3] + [(k, 1, 0)] + good[3:])

    return {
        "key_offs-start": edit(1, 0, 1),
        "key_offs-decrease": edit(1, 3, 2),
        "key-empty": with_key(b""),
        "key-one-byte": with_key(b"\x00"),
        "hklen-beyond-key": with_key(b"\x00\x05abc"),
        "hklen-ffff": with_key(b"\xff\xff" + b"h" * 0xFFFF + b"s"),
    }


def _raw_call(g, n, a, stats=None):
    return g._L.rrdb_incr_batch(g._h, n, *[None if x is None else x.ctypes.data_as(C.c_void_p)
                                           for x in a], NOW, None, None, stats)


def test_rejections_leave_the_handle_alone(hip_lib, oracle_lib, tmp_path):
    """p has pending memtable entries that a rejected call must not flush; q
    has none, so its checkpoint can be taken after every rejection"""
    layers, ops = gen_hot_key(300, 81)
    pending = dict(layers[0])
    p, _ = open_prepared(hip_lib, 0, {}, [layers[0], pending], NOW)
    q, _ = open_prepared(hip_lib, 0, {}, layers, NOW)
    o, _ = open_prepared(oracle_lib, -1, {}, layers, NOW)
    try:
        before_p = (p.num_runs(), p.num_records(), p.memtable_entries())
        assert before_p[0] == 1 and before_p[2] == len(pending) > 0
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
                err, _, _, st = h.incr_batch_arrays(*arrays, NOW)
                assert err == INVALID_ARGUMENT, name
                assert _stats(st) == dict.fromkeys(STAT_FIELDS, 0), name
            unchanged(name)
        a = _arrays(ops[:4])
        for h in (p, q):
            # increments == NULL
            assert _raw_call(h, 4, [a[0], a[1], None, a[3]]) == INVALID_ARGUMENT
            # more ops than the 32-bit index carries: refused before any array is read
            assert _raw_call(h, 2**31, a) == INVALID_ARGUMENT
        unchanged("null-increments / 2^31 ops")
        for h in (p, q):
            assert h.scan_count_begin(b"\x00\x00", b"\xff\xff", NOW,
                                      validate_partition_hash=False) == OK
        # (the count scan's begin has flushed p's memtable: compare from here)
        before_p = (p.num_runs(), p.num_records(), p.memtable_entries())
        for h in (p, q):
            assert h.incr_batch(ops, NOW)[0] == INVALID_ARGUMENT
        assert (p.num_runs(), p.num_records(), p.memtable_entries()) == before_p
        for h in (p, q):
            assert h.scan_count_finish()[0] == OK
            assert h.manual_compact_begin(NOW) == OK
            assert h.incr_batch(ops, NOW)[0] == INVALID_ARGUMENT
        assert (p.num_runs(), p.num_records(), p.memtable_entries()) == before_p
        assert (q.num_runs(), q.memtable_entries()) == shape_q
        for h in (p, q):
            assert h.manual_compact_finish()[0] == OK
        assert o.manual_compact(NOW)[0] == OK
        # the next accepted batch takes the seqnos the rejected ones left alone
        reader, _ = open_prepared(oracle_lib, -1, {}, layers, NOW)
        try:
            err, nv, er, _ = q.incr_batch(ops, NOW)
            assert err == OK and (nv, er) == drive_sequence(reader, o, ops, NOW)
        finally:
            reader.close()
        _same_checkpoint(q, o, tmp_path)
    finally:
        p.close()
        q.close()
        o.close()
