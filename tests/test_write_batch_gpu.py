"""GPU parity for batched writes, rrdb_write_batch
(include/rrdb_engine_ext.h).

The CPU oracle has no batch call: the expected state is an oracle handle
driven through put / remove in the same order and then flush.  Physical parity
goes through checkpoints, which both backends write in one format: every
run_k.{keys,koff,vals,voff,sk} byte for byte and the MANIFEST's data_version,
next_seq_floor, n_runs and run lines.  The case lists and sizes live in
tests/test_write_batch_model.py, which pins them against the oracle on the CPU.
"""
import ctypes as C

import numpy as np
import pytest

from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import INVALID_ARGUMENT, OK, _pack
from test_minor_compact_model import stats_dict
from test_split_gpu import _open, _same_reads
from test_split_model import fixed_key, hash_keys_of
from test_write_batch_model import (CASE_PARAMS, NOW, STAT_FIELDS, T, apply_ops, batch_run,
                                    env_version, ops_dups, ops_fixed, read_checkpoint)

pytestmark = pytest.mark.gpu


def _pair(hip_lib, oracle_lib, envs=None):
    g, o = hip_lib.open(1, 0, 0), oracle_lib.open(1, 0, -1)
    if envs:
        assert g.set_envs(envs) == OK and o.set_envs(envs) == OK
    return g, o


def _same_checkpoint(g, o, tmp_path, tag="a"):
    """every run and the manifest fields, engine against oracle"""
    mg, rg = read_checkpoint(g, tmp_path / ("g" + tag))
    mo, ro = read_checkpoint(o, tmp_path / ("o" + tag))
    assert mg == mo
    assert len(rg) == len(ro)
    for i, (a, b) in enumerate(zip(rg, ro)):
        for col in ("n", "sk", "koff", "voff", "keys", "vals"):
            assert a[col] == b[col], "run %d column %s differs" % (i, col)
    return mg


def _stats(st):
    return {f: getattr(st, f) for f in STAT_FIELDS}


# 1 shapes --------------------------------------------------------------------

@pytest.mark.parametrize("case,n", CASE_PARAMS)
def test_batch_equals_put_remove_flush(hip_lib, oracle_lib, tmp_path, case, n):
    """one batch on a handle whose floor is 2 (a flushed memtable ahead of it)"""
    _, gen, _, envs, epoch_now = case
    ops = gen(n)
    g, o = _pair(hip_lib, oracle_lib, envs)
    try:
        for p in (g, o):
            assert p.put(b"before", b"a", b"x", 0, epoch_now) == OK
            assert p.remove(b"before", b"b") == OK
            assert p.flush() == OK
        err, st = g.write_batch(ops, epoch_now)
        assert err == OK
        apply_ops(o, ops, epoch_now)
        assert o.flush() == OK
        assert g.memtable_entries() == 0
        assert g.num_runs() == o.num_runs() == 2
        assert g.num_records() == o.num_records()
        man = _same_checkpoint(g, o, tmp_path)
        assert man["next_seq_floor"] == 2 + n
        _, want = batch_run(ops, 2, env_version(envs), int(envs.get("default_ttl", 0)),
                            epoch_now)
        assert _stats(st) == want
        for ph in ("wb_sort", "wb_emit", "wb_total"):
            assert g.phase_ms(ph) >= 0.0
        # the run serves reads like any other
        probe = [op[0] for op in ops[:: max(1, n // 50)]]
        assert g.batch_get(probe, NOW) == o.batch_get(probe, NOW)
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("n", [T + 1, 3 * T + 7])
def test_one_key_keeps_the_last_op(hip_lib, n):
    k = D.generate_key(b"only", b"one")
    g = hip_lib.open(1, 0, 0)
    try:
        err, st = g.write_batch([(k, b"v%d" % i, 0) for i in range(n)])
        assert err == OK
        assert (st.output_records, st.superseded, st.puts) == (1, n - 1, 1)
        assert g.get(k, NOW) == (OK, b"v%d" % (n - 1))
        # the next batch's first op is seqno n: it outranks the record above
        assert g.write_batch([(k, None, 0)])[0] == OK
        assert g.get(k, NOW)[0] != OK
    finally:
        g.close()


# 2 state ---------------------------------------------------------------------

def test_runs_and_memtable_before_the_batch(hip_lib, oracle_lib, tmp_path):
    """runs already ingested plus pending memtable entries: num_runs grows by
    two and the memtable's run is the older one"""
    g, o = _pair(hip_lib, oracle_lib)
    try:
        base = ops_fixed(300, 41)
        for p in (g, o):
            keys = sorted(k for k, _, _ in base[:200])
            p.ingest_run([(k, D.encode_value(b"old", 0, 0, 1), 1 + i, 0)
                          for i, k in enumerate(keys)])
            p.ingest_run([(k, D.encode_value(b"older2", 0, 0, 1), 1000 + i, 0)
                          for i, k in enumerate(keys[:50])])
            apply_ops(p, base[190:230])  # pending, not flushed
        assert g.num_runs() == 2 and g.memtable_entries() == 40
        batch = ops_dups(T + 5, 42) + base[100:300]
        err, st = g.write_batch(batch)
        assert err == OK
        assert o.flush() == OK
        apply_ops(o, batch)
        assert o.flush() == OK
        assert g.num_runs() == o.num_runs() == 4
        assert g.memtable_entries() == 0
        man = _same_checkpoint(g, o, tmp_path)
        assert man["run"][2][1] == 40 and man["run"][3][1] == st.output_records
        probe = [k for k, _, _ in base]
        assert g.batch_get(probe, NOW) == o.batch_get(probe, NOW)
    finally:
        g.close()
        o.close()


def _ttl_ops(ids, tag, seed):
    import random

    rnd = random.Random(seed)
    ops = []
    for i in ids:
        if rnd.random() < 0.2:
            ops.append((fixed_key(i), None, 0))
        else:
            ets = rnd.choice((0, 0, NOW - 10, NOW + 500))
            ops.append((fixed_key(i), b"%s-%d" % (tag, i), ets))
    rnd.shuffle(ops)
    return ops


def test_two_batches_then_every_read_and_a_compaction(hip_lib, oracle_lib, tmp_path):
    """the second batch overwrites half of the first; reads at NOW and LATER,
    full manual_compact stats, reads again"""
    g, o = _open(hip_lib, 0, 0), _open(oracle_lib, 0, -1)
    try:
        first = _ttl_ops(range(0, 600), b"a", 51)
        second = _ttl_ops(range(300, 900), b"b", 52)
        for ops in (first, second):
            assert g.write_batch(ops)[0] == OK
            apply_ops(o, ops)
            assert o.flush() == OK
        _same_checkpoint(g, o, tmp_path)
        keys = sorted({op[0] for op in first + second})
        hks = hash_keys_of([{k: 0} for k in keys])[:6]
        _same_reads(g, o, keys, hks, point_stride=7)
        (eg, sg), (eo, so) = g.manual_compact(NOW), o.manual_compact(NOW)
        assert eg == eo == OK
        assert stats_dict(sg) == stats_dict(so)
        _same_reads(g, o, keys, hks, point_stride=7)
        _same_checkpoint(g, o, tmp_path, "b")
    finally:
        g.close()
        o.close()


def test_auto_compact_after_batches_as_after_flushes(hip_lib, tmp_path):
    """the tick sees batch runs as it sees flushed runs: same pick, same
    stats, same resulting layout"""
    a, b = hip_lib.open(1, 0, 0), hip_lib.open(1, 0, 0)
    try:
        for r in range(4):
            ops = ops_dups(500 + 300 * r, 60 + r)
            assert a.write_batch(ops)[0] == OK
            apply_ops(b, ops)
            assert b.flush() == OK
            if r < 3:
                ta, tb = a.auto_compact(NOW), b.auto_compact(NOW)
                assert ta[:3] == tb[:3] == (OK, 0, 0)
        ta, tb = a.auto_compact(NOW), b.auto_compact(NOW)
        assert ta[0] == tb[0] == OK
        assert ta[1:3] == tb[1:3] and ta[2] >= 2
        assert stats_dict(ta[3]) == stats_dict(tb[3])
        assert a.num_runs() == b.num_runs()
        _same_checkpoint(a, b, tmp_path)
    finally:
        a.close()
        b.close()


def test_empty_batch_does_nothing(hip_lib, oracle_lib, tmp_path):
    g, o = _pair(hip_lib, oracle_lib)
    try:
        for p in (g, o):
            assert p.put(b"hk", b"sk", b"v", 0, 0) == OK
        err, st = g.write_batch([])
        assert err == OK and _stats(st) == dict.fromkeys(STAT_FIELDS, 0)
        assert g.num_runs() == 0 and g.memtable_entries() == 1
        ops = ops_fixed(70, 71)
        assert g.write_batch(ops)[0] == OK
        assert o.flush() == OK
        apply_ops(o, ops)
        assert o.flush() == OK
        assert _same_checkpoint(g, o, tmp_path)["next_seq_floor"] == 71
    finally:
        g.close()
        o.close()


# 3 rejections ----------------------------------------------------------------

def _arrays(ops):
    keys, koffs = _pack([op[0] for op in ops])
    vals, voffs = _pack([op[1] if op[1] is not None else b"" for op in ops])
    expire = np.array([op[2] for op in ops], dtype=np.uint32)
    kinds = np.array([0 if op[1] is not None else 1 for op in ops], dtype=np.uint8)
    return [keys, koffs, vals, voffs, expire, kinds]


def _bad_inputs():
    good = [(D.generate_key(b"hk%d" % i, b"s"), b"v%d" % i, 0) for i in range(6)]

    def edit(col, idx, value):
        a = _arrays(good)
        a[col][idx] = value
        return a

    def with_key(k):
        return _arrays(good[:3] + [(k, b"v", 0)] + good[3:])

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


def _snapshot(g):
    return g.num_runs(), g.num_records(), g.memtable_entries()


def test_rejections_leave_the_handle_alone(hip_lib, oracle_lib, tmp_path):
    g, o = _pair(hip_lib, oracle_lib)
    try:
        base = ops_fixed(100, 81)
        for p in (g, o):
            apply_ops(p, base[:60])
            assert p.flush() == OK
            apply_ops(p, base[60:])  # pending: a rejected batch must not flush it
        before = _snapshot(g)
        assert before[0] == 1 and before[2] == 40
        for name, arrays in _bad_inputs().items():
            err, st = g.write_batch_arrays(*arrays)
            assert err == INVALID_ARGUMENT, name
            assert _stats(st) == dict.fromkeys(STAT_FIELDS, 0), name
            assert _snapshot(g) == before, name
        # more ops than the 32-bit index carries: refused before any array is read
        a = _arrays(base[:4])
        err = g._L.rrdb_write_batch(g._h, 2**31, *[x.ctypes.data_as(C.c_void_p) for x in a],
                                    0, None)
        assert err == INVALID_ARGUMENT and _snapshot(g) == before
        # the next accepted batch takes the seqnos the rejected ones left alone
        ops = ops_dups(300, 82)
        assert g.write_batch(ops)[0] == OK
        assert o.flush() == OK
        apply_ops(o, ops)
        assert o.flush() == OK
        assert _same_checkpoint(g, o, tmp_path)["next_seq_floor"] == 400
    finally:
        g.close()
        o.close()


def test_rejected_while_a_split_operation_is_pending(hip_lib, oracle_lib, tmp_path):
    """a split compaction or a pipelined count scan pending on the handle"""
    g, o = _pair(hip_lib, oracle_lib)
    try:
        base = ops_fixed(200, 91)
        for p in (g, o):
            apply_ops(p, base)
            assert p.flush() == OK
        ops = ops_dups(100, 92)
        assert g.scan_count_begin(b"\x00\x00", b"\xff\xff", NOW,
                                  validate_partition_hash=False) == OK
        before = _snapshot(g)
        assert g.write_batch(ops)[0] == INVALID_ARGUMENT
        assert _snapshot(g) == before
        assert g.scan_count_finish() == (OK, 200)
        assert g.manual_compact_begin(NOW) == OK
        assert g.write_batch(ops)[0] == INVALID_ARGUMENT
        assert _snapshot(g) == before
        assert g.manual_compact_finish()[0] == OK
        assert o.manual_compact(NOW)[0] == OK
        assert g.write_batch(ops)[0] == OK
        apply_ops(o, ops)
        assert o.flush() == OK
        assert _same_checkpoint(g, o, tmp_path)["next_seq_floor"] == 300
    finally:
        g.close()
        o.close()
