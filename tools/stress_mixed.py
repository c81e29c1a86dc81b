#!/usr/bin/env python3
"""Mixed-operation GPU stress: randomized interleavings of every C-ABI
entry point on one handle — writes, batched writes (rrdb_write_batch, which
the oracle replays through put/remove), batched counter increments
(rrdb_incr_batch, which the oracle replays through get/ttl/put), batched
check-and-mutate ops (rrdb_check_and_mutate_batch, which the oracle replays
through get/ttl and the applied puts/removes), batched writes with timetags
(rrdb_write_batch_timetag, whose run the oracle ingests from a model), flushes,
point/range/batched reads with
the serving lanes forced on, pipelined count scans, paged scans, real
compactions, checkpoints and restores — cross-checked against the CPU
oracle driven with the same operation stream.  Complements tools/soak.py
(which focuses on compaction/read parity) with the round-2 surfaces.

Usage: python tools/stress_mixed.py [steps=600] [seed=11]
"""
import ctypes
import os
import random
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from incubator_pegasus_amd import data as D  # noqa: E402
from incubator_pegasus_amd.capi import OK, RrdbLib  # noqa: E402


_LIBC = ctypes.CDLL(None, use_errno=True)
_LIBC.strtoll.restype = ctypes.c_longlong
_LIBC.strtoll.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]


def buf2int64(s):
    """dsn::buf2int64: strtoll over the whole span, no range error"""
    buf = ctypes.create_string_buffer(s, len(s) + 1)
    end = ctypes.c_void_p()
    ctypes.set_errno(0)
    v = _LIBC.strtoll(buf, ctypes.byref(end), 0)
    if not s or end.value - ctypes.addressof(buf) != len(s) or ctypes.get_errno() != 0:
        return None
    return v


def replay_incr(o, ops, now):
    """the batch on the oracle: every base read before the first put (an
    oracle read flushes), then the reference's incr op by op on a shadow of
    the touched keys, its successful puts, one flush"""
    assert o.flush() == OK
    shadow = {}
    for k in {op[0] for op in ops}:
        e, val = o.get(k, now)
        if e == OK:
            _, ttl = o.ttl(k, now)
            shadow[k] = (val, now + ttl if ttl > 0 else 0)
    values, errors = [], []
    for k, inc, d in ops:
        old = shadow.get(k)
        if old is not None and 0 < old[1] <= now:
            old = None
        if old is None:
            new, ne = inc, (d if d > 0 else 0)
        else:
            new = inc
            if old[0]:
                cur = buf2int64(old[0])
                new = None if cur is None else cur + inc
                if new is None or not -2**63 <= new < 2**63:
                    values.append(0 if cur is None else cur)
                    errors.append(4)  # kInvalidArgument
                    continue
            ne = old[1] if d == 0 else (0 if d < 0 else d)
        hk, sk = D.restore_key(k)
        assert o.put(hk, sk, b"%d" % new, ne, now) == OK
        shadow[k] = (b"%d" % new, ne)
        values.append(new)
        errors.append(OK)
    assert o.flush() == OK
    return values, errors


def validate_check(ct, operand, exist, value):
    """the reference's validate_check: (passed, invalid_argument)"""
    if ct <= 4:
        return (True, not exist, not exist or not value, exist, exist and bool(value))[ct], False
    if not exist:
        return False, False
    if ct <= 7:
        if not operand:
            return True, False
        if len(value) < len(operand):
            return False, False
        return (operand in value, value.startswith(operand), value.endswith(operand))[ct - 5], False
    a, b = value, operand
    if ct >= 13:
        a, b = buf2int64(value), buf2int64(operand)
        if a is None or b is None:
            return False, True
    c = (a > b) - (a < b)
    return (c < 0, c <= 0, c == 0, c >= 0, c > 0)[(ct - 8) % 5], False


def replay_cas(o, ops, now):
    """the batch on the oracle: every check key read before the first write
    (an oracle read flushes), then the reference's check_and_mutate op by op
    on a shadow of the touched keys, the applied puts and removes, one flush"""
    assert o.flush() == OK
    shadow = {}
    for k in {op[0] for op in ops}:
        e, val = o.get(k, now)
        if e == OK:
            _, ttl = o.ttl(k, now)
            shadow[k] = (val, now + ttl if ttl > 0 else 0)
    errors, exists, values = [], [], []
    for ck, ct, operand, muts, ret in ops:
        if not muts or not 0 <= ct <= 17:
            errors.append(4)  # kInvalidArgument: a malformed op reads nothing
            exists.append(False)
            values.append(b"")
            continue
        old = shadow.get(ck)
        exist = old is not None and not 0 < old[1] <= now
        passed, invalid = validate_check(ct, operand, exist, old[0] if exist else b"")
        exists.append(exist)
        values.append(old[0] if exist and ret else b"")
        errors.append(OK if passed else (4 if invalid else 13))  # 13 = kTryAgain
        if passed:
            for k, v, ets in muts:
                hk, sk = D.restore_key(k)
                if v is None:
                    assert o.remove(hk, sk) == OK
                    shadow[k] = None
                else:
                    assert o.put(hk, sk, v, ets, now) == OK
                    shadow[k] = (v, ets)
    assert o.flush() == OK
    return errors, exists, values


def replay_timetag(o, ops, now, ckpt_dir, decree):
    """the batch on the oracle: no read returns a timetag, so the ops of this
    kind write theirs into the user bytes as well (b"t<timetag>:..."; no other
    writer's value starts with a t, and those store timetag 0).  The bases are
    read first, the ops walked by the rule of the header comment, and the
    model's run is ingested with seqnos from the oracle's own floor, which a
    checkpoint (it flushes, as the batch does) reports."""
    assert o.checkpoint(ckpt_dir, decree) == OK
    floor = None
    for line in open(os.path.join(ckpt_dir, "checkpoint.%d" % decree, "MANIFEST")):
        f = line.split()
        if f and f[0] == "next_seq_floor":
            floor = int(f[1])
    live = {}
    for k in {op[0] for op in ops}:
        e, val = o.get(k, now)
        if e == OK:
            live[k] = int(val[1:val.index(b":")]) if val.startswith(b"t") else 0
    applied, newest = [], {}
    for i, (k, v, ets, tt, verify) in enumerate(ops):
        if v is None:
            live.pop(k, None)
            newest[k] = (b"", floor + i, 1)
        else:
            if verify and k in live and live[k] >= tt:
                applied.append(0)
                continue
            if 0 < ets <= now:
                live.pop(k, None)
            else:
                live[k] = tt
            newest[k] = (D.encode_value(v, ets, tt, 1), floor + i, 0)
        applied.append(1)
    if newest:
        o.ingest_run([(k,) + newest[k] for k in sorted(newest)])
    return applied


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 600
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 11
    rnd = random.Random(seed)
    now = 1000
    hip = RrdbLib(os.path.join(REPO, "incubator_pegasus_amd", "csrc", "librrdb_hip.so"))
    orc = RrdbLib(os.path.join(REPO, "oracle", "liboracle.so"))
    g = hip.open(1, 0, 0)
    o = orc.open(1, 0, -1)
    envs = {"engine.mg_persist": "on",
            "rocksdb.max_iteration_count": str(2**31 - 1)}
    g.set_envs(envs)
    o.set_envs({"rocksdb.max_iteration_count": str(2**31 - 1)})
    checks = 0
    tmp = tempfile.mkdtemp(prefix="stress_ckpt_")
    tmp_o = tempfile.mkdtemp(prefix="stress_ckpt_o_")
    decree = 0
    for step in range(steps):
        op = rnd.randrange(14)
        if op == 13:  # batched writes with timetags: local and duplicated puts
            # and removes on the shared key space, a past expire now and then
            ops = []
            for _ in range(rnd.choice([1, 7, 300, 2049, 5000])):
                k = D.generate_key(b"hk%03d" % rnd.randrange(70), b"s%02d" % rnd.randrange(7))
                tt = rnd.randrange(0, 40)
                if rnd.random() < 0.15:
                    ops.append((k, None, 0, 0, 0))
                else:
                    ops.append((k, b"t%d:%d" % (tt, step), rnd.choice([0, 0, 0, now + 50, now - 1]),
                                tt, rnd.random() < 0.7))
            decree += 1
            err, applied, st = g.write_batch_timetag(ops, now)
            assert err == OK and st.input_ops == len(ops)
            assert applied == replay_timetag(o, ops, now, tmp_o, decree)
            assert st.applied == sum(applied)
            assert g.num_runs() == o.num_runs() and g.num_records() == o.num_records()
            checks += 1
        elif op == 12:  # batched check-and-mutate: every check type, lists of up
            # to three mutations on the check key's hashkey, now and then a
            # malformed op (an empty list, a check type out of range)
            ops = []
            for _ in range(rnd.choice([1, 7, 300, 2049, 5000])):
                hk = b"hk%03d" % rnd.randrange(70)
                muts = [(D.generate_key(hk, b"s%02d" % rnd.randrange(7)),
                         None if rnd.random() < 0.2 else rnd.choice([b"5", b"v7", b"0x10", b""]),
                         rnd.choice([0, 0, 0, now + 50, now - 1]))
                        for _ in range(rnd.choice([0, 1, 1, 1, 2, 3]))]
                ops.append((D.generate_key(hk, b"s%02d" % rnd.randrange(7)),
                            rnd.choice([-1, 18] + list(range(18)) * 3),
                            rnd.choice([b"", b"v", b"5", b"7", b"16", b"v7", b"b1"]), muts,
                            rnd.random() < 0.5))
            err, errors, exists, values, st = g.check_and_mutate_batch(ops, now)
            assert err == OK and st.input_ops == len(ops)
            assert (errors, exists, values) == replay_cas(o, ops, now)
            assert g.num_runs() == o.num_runs() and g.num_records() == o.num_records()
            checks += 1
        elif op == 11:  # batched increments: most stored values are no integers
            # (the op fails and writes nothing) until an incr has replaced them
            ops = [(D.generate_key(b"hk%03d" % rnd.randrange(70), b"s%02d" % rnd.randrange(7)),
                    rnd.choice([1, -1, 5, 2**62, -2**62]),
                    rnd.choice([0, 0, 0, -1, now + 50, now - 1]))
                   for _ in range(rnd.choice([1, 7, 300, 2049, 5000]))]
            err, values, errors, st = g.incr_batch(ops, now)
            assert err == OK and st.input_ops == len(ops)
            assert (values, errors) == replay_incr(o, ops, now)
            assert g.num_runs() == o.num_runs() and g.num_records() == o.num_records()
            checks += 1
        elif op == 10:  # batched write: the engine sorts and dedups it on the
            # device; the oracle takes the same ops one by one.  The batch
            # flushes the memtable ahead of itself and ends in a run of its
            # own, so the oracle flushes at those two points
            ops = []
            for _ in range(rnd.choice([1, 7, 300, 2049, 5000])):
                k = D.generate_key(b"hk%03d" % rnd.randrange(60), b"s%02d" % rnd.randrange(6))
                if rnd.random() < 0.15:
                    ops.append((k, None, 0))
                else:
                    ops.append((k, b"b%d-%d" % (step, len(ops)),
                                rnd.choice([0, 0, 0, now + 50])))
            err, st = g.write_batch(ops, now)
            assert err == OK and st.input_ops == len(ops)
            assert o.flush() == OK
            for k, v, ets in ops:
                hk, sk = D.restore_key(k)
                if v is None:
                    o.remove(hk, sk)
                else:
                    o.put(hk, sk, v, ets, now)
            assert o.flush() == OK
            assert g.num_runs() == o.num_runs() and g.num_records() == o.num_records()
            checks += 1
        elif op <= 1:  # writes
            for _ in range(rnd.randrange(1, 25)):
                hk = b"hk%03d" % rnd.randrange(60)
                sk = b"s%02d" % rnd.randrange(6)
                if rnd.random() < 0.15:
                    g.remove(hk, sk)
                    o.remove(hk, sk)
                else:
                    v = b"v%d" % step
                    ttl = rnd.choice([0, 0, 0, now + 50])
                    g.put(hk, sk, v, ttl, now)
                    o.put(hk, sk, v, ttl, now)
        elif op == 2:  # point gets
            for _ in range(8):
                k = D.generate_key(b"hk%03d" % rnd.randrange(70), b"s%02d" % rnd.randrange(7))
                assert g.get(k, now) == o.get(k, now), k
                checks += 1
        elif op == 3:  # multi_get burst (keeps the resident lane warm)
            hk = b"hk%03d" % rnd.randrange(70)
            kw = dict(reverse=rnd.random() < 0.3,
                      max_kv_count=rnd.choice([-1, 1, 3]))
            for _ in range(rnd.randrange(1, 6)):
                assert g.multi_get(hk, now, **kw) == o.multi_get(hk, now, **kw), (hk, kw)
                checks += 1
        elif op == 4:  # batched multi_get
            hks = [b"hk%03d" % rnd.randrange(70) for _ in range(16)]
            eg, gg = g.multi_get_batch(hks, now)
            eo, go = o.multi_get_batch(hks, now)
            assert (eg, gg) == (eo, go)
            checks += 1
        elif op == 5:  # pipelined count
            rc_g = g.scan_count_begin(b"\x00\x00", b"\xff\xff", now,
                                      validate_partition_hash=False)
            rc_o = o.scan_count_begin(b"\x00\x00", b"\xff\xff", now,
                                      validate_partition_hash=False)
            assert rc_g == rc_o == OK
            assert g.scan_count_finish() == o.scan_count_finish()
            checks += 1
        elif op == 6:  # paged scan
            rg = g.scan_open(b"\x00\x00", b"\xff\xff", now, batch_size=9,
                             validate_partition_hash=False)
            ro = o.scan_open(b"\x00\x00", b"\xff\xff", now, batch_size=9,
                             validate_partition_hash=False)
            assert rg.error == ro.error == OK
            assert rg.kvs == ro.kvs
            while rg.context_id != -1:
                assert ro.context_id != -1
                rg = g.scan_next(rg.context_id, now)
                ro = o.scan_next(ro.context_id, now)
                assert rg.error == ro.error == OK and rg.kvs == ro.kvs
            assert ro.context_id == -1
            checks += 1
        elif op == 7:  # real compaction
            assert g.manual_compact(now) == o.manual_compact(now)
            checks += 1
        elif op == 8 and g.num_records() > 0:  # checkpoint + cross restore
            # checkpoint BOTH handles: checkpoint flushes the memtable, and
            # flush-point-dependent compact stats (input_records/shadowed)
            # only compare when both sides saw the same flush boundaries
            decree += 1
            assert g.checkpoint(tmp, decree) == OK
            assert o.checkpoint(tmp_o, decree) == OK
            r = hip.open(1, 1, 0)
            ro_ = orc.open(1, 1, -1)
            try:
                assert r.restore(tmp, decree) == OK
                assert ro_.restore(tmp_o, decree) == OK
                k = D.generate_key(b"hk%03d" % rnd.randrange(60), b"s00")
                assert r.get(k, now) == g.get(k, now) == ro_.get(k, now)
            finally:
                r.close()
                ro_.close()
            checks += 1
        else:  # sortkey_count
            hk = b"hk%03d" % rnd.randrange(70)
            assert g.sortkey_count(hk, now) == o.sortkey_count(hk, now), hk
            checks += 1
    g.close()
    o.close()
    print(f"STRESS-MIXED OK: {steps} steps, {checks} parity checks")


if __name__ == "__main__":
    main()
