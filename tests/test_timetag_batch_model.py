"""Batched writes with timetags: the independent model, its case lists and its
CPU checks.

`timetag_model` restates rrdb_write_batch_timetag (include/rrdb_engine_ext.h,
DESIGN.md §3g) in Python on abstract key states: a key is dead, or live with a
timetag; a verified PUT is ignored when the key is live and its timetag is not
smaller; op i takes seqno floor + i; the last applied op of every key is the
record stored.

`restate` is the literal version: the reference's write_batch_put_ctx /
write_batch_delete (rocksdb_wrapper.cpp:129-183, :221-239) applied one op at a
time to a dict of raw value bytes, reading the timetag back out of the bytes
with data.decode_value before every verified PUT.  The model is proven against
it, and against an oracle handle: the layers and then the model's run go in
through rrdb_ingest_run, and get / ttl on every touched key must show the
restatement's view.  tests/test_timetag_batch_gpu.py pins the engine against
the model and against an oracle handle prepared the same way.

A layer is {key: (user data or None, expire_ts, timetag)}; layers[:-1] become
ingested runs, layers[-1] pending memtable entries written with rrdb_put /
rrdb_remove (which store timetag 0, whatever the layer says).
An op is (full_key, value_or_None, expire_ts, timetag, verify).
"""
import ctypes
import os
import random
import re
import struct
import subprocess

import pytest

from conftest import HIP_SO, REPO
from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import OK
from test_write_batch_model import NOW, T, _raw18, batch_run
from test_write_batch_model import STAT_FIELDS as WB_STAT_FIELDS

SIZES = [T + 1, 3 * T + 7]  # the smallest that cross the sort's tile and merge boundaries
STAT_FIELDS = ("input_ops", "applied", "ignored", "output_records", "superseded", "puts",
               "removes", "key_bytes", "value_bytes")
# the lane/wave threshold (32), the 64-op stride and the multi-stride staging (4 x 64)
CHAIN_LENGTHS = [32, 33, 64, 65, 257, T + 1]
CHAIN_PATTERNS = ["rising", "falling", "mix", "past-expire"]


# ---------------- the model ----------------

def generate_timetag(timestamp, cluster_id, deleted=False):
    """pegasus_value_schema.h:44-47; the engine only ever compares the result"""
    return (timestamp << 8) | (cluster_id << 1) | (1 if deleted else 0)


def _stored_expire(ets, default_ttl, now):
    return (now + default_ttl) & 0xFFFFFFFF if ets == 0 and default_ttl else ets


def base_states(layers, data_version, default_ttl, now):
    """{key: timetag} of the keys a read at `now` finds after prepare()"""
    newest = {}
    for j, layer in enumerate(layers):
        pending = j == len(layers) - 1
        for k, (v, ets, tt) in layer.items():
            if v is None:
                newest[k] = None
            elif pending:  # a put: write-time default_ttl, timetag 0
                newest[k] = (_stored_expire(ets, default_ttl, now), 0)
            else:
                newest[k] = (ets, tt if data_version >= 1 else 0)
    return {k: s[1] for k, s in newest.items() if s is not None and not 0 < s[0] <= now}


def timetag_model(layers, ops, floor, data_version=1, default_ttl=0, now=0):
    """Returns (applied, stats, run or None, new floor)."""
    live = base_states(layers, data_version, default_ttl, now)
    applied, newest = [], {}
    for i, (k, v, ets, tt, verify) in enumerate(ops):
        if v is None:
            live.pop(k, None)
            newest[k] = (b"", floor + i, 1)
        else:
            if verify and data_version >= 1 and k in live and live[k] >= tt:
                applied.append(0)
                continue
            ets = _stored_expire(ets, default_ttl, now)
            if 0 < ets <= now:
                live.pop(k, None)
            else:
                live[k] = tt
            newest[k] = (D.encode_value(v, ets, tt if data_version >= 1 else 0, data_version),
                         floor + i, 0)
        applied.append(1)
    keys = sorted(newest)
    koff, voff = [0], [0]
    for k in keys:
        koff.append(koff[-1] + len(k))
        voff.append(voff[-1] + len(newest[k][0]))
    run = None
    if keys:
        run = {
            "n": len(keys),
            "keys": b"".join(keys),
            "koff": struct.pack("<%dQ" % len(koff), *koff),
            "vals": b"".join(newest[k][0] for k in keys),
            "voff": struct.pack("<%dQ" % len(voff), *voff),
            "sk": struct.pack("<%dQ" % len(keys), *[(newest[k][1] << 1) | newest[k][2]
                                                    for k in keys]),
        }
    n_applied = sum(applied)
    puts = sum(1 for k in keys if newest[k][2] == 0)
    stats = dict(input_ops=len(ops), applied=n_applied, ignored=len(ops) - n_applied,
                 output_records=len(keys), superseded=n_applied - len(keys), puts=puts,
                 removes=len(keys) - puts, key_bytes=koff[-1], value_bytes=voff[-1])
    return applied, stats, run, floor + len(ops)


# ---------------- the literal restatement ----------------

def raw_overlay(layers, data_version, default_ttl, now):
    """{key: raw value bytes, or None for a tombstone} after prepare()"""
    db = {}
    for j, layer in enumerate(layers):
        pending = j == len(layers) - 1
        for k, (v, ets, tt) in layer.items():
            if v is None:
                db[k] = None
            elif pending:
                db[k] = D.encode_value(v, _stored_expire(ets, default_ttl, now), 0, data_version)
            else:
                db[k] = D.encode_value(v, ets, tt, data_version)
    return db


def restate(layers, ops, data_version, default_ttl, now):
    """write_batch_put_ctx / write_batch_delete, one op at a time, on raw
    bytes.  Returns (applied, db)."""
    db = raw_overlay(layers, data_version, default_ttl, now)
    applied = []
    for k, v, ets, tt, verify in ops:
        if v is None:
            db[k] = None  # write_batch_delete: no check
            applied.append(1)
            continue
        if verify and data_version >= 1:  # needs read-before-write
            raw = db.get(k)
            if raw is not None:  # found
                old_ets, old_tt, _ = D.decode_value(raw, data_version)
                if not 0 < old_ets <= now and old_tt >= tt:
                    applied.append(0)  # the reference's empty record
                    continue
        db[k] = D.encode_value(v, _stored_expire(ets, default_ttl, now), tt, data_version)
        applied.append(1)
    return applied, db


def view_of(db, data_version, now):
    """what get / ttl report for every key of db: {key: (user data, expire)}"""
    out = {}
    for k, raw in db.items():
        if raw is None:
            continue
        ets, _, user = D.decode_value(raw, data_version)
        if not 0 < ets <= now:
            out[k] = (user, ets)
    return out


# ---------------- driving a backend ----------------

def prepare(part, layers, data_version, now):
    """Returns the handle's sequence floor afterwards."""
    seq, floor = 1, 0
    for layer in layers[:-1]:
        recs = []
        for k in sorted(layer):
            v, ets, tt = layer[k]
            recs.append((k, b"" if v is None else D.encode_value(v, ets, tt, data_version), seq,
                         1 if v is None else 0))
            seq += 1
        if recs:
            part.ingest_run(recs)
            floor = seq
    for k, (v, ets, _) in layers[-1].items():
        hk, sk = D.restore_key(k)
        if v is None:
            assert part.remove(hk, sk) == OK
        else:
            assert part.put(hk, sk, v, ets, now) == OK
        floor += 1
    return floor


def env_version(envs):
    return int(envs.get("pegasus.data_version", 1))


def env_ttl(envs):
    return int(envs.get("default_ttl", 0))


def open_prepared(lib, gpu_id, envs, layers, now):
    p = lib.open(1, 0, gpu_id)
    if envs:
        assert p.set_envs(envs) == OK
    return p, prepare(p, layers, env_version(envs), now)


def ingest_model_run(part, run):
    """the model's run into a handle whose memtable has been flushed"""
    assert part.flush() == OK
    if run is None:
        return
    koff = struct.unpack("<%dQ" % (run["n"] + 1), run["koff"])
    voff = struct.unpack("<%dQ" % (run["n"] + 1), run["voff"])
    sk = struct.unpack("<%dQ" % run["n"], run["sk"])
    part.ingest_run([(run["keys"][koff[i]:koff[i + 1]], run["vals"][voff[i]:voff[i + 1]],
                      sk[i] >> 1, sk[i] & 1) for i in range(run["n"])])


# ---------------- the case lists ----------------
# a generator returns (layers, ops) for n ops.  Every one plants the same block
# of special keys, so that no case can pass empty (case_conditions), and fills
# the rest of the batch in its own way.

def keys_fixed(rnd, count):
    return _raw18(rnd.sample(range(10 * count + 100), count))


def keys_mixed(rnd, count):
    """key lengths from 3 bytes up, hashkey lengths 0..22"""
    out = []
    for j in rnd.sample(range(4 * count + 50), count):
        hl = j % 23
        hk = (b"h%d." % j).ljust(hl, b"x")[:hl] if hl else b""
        out.append(D.generate_key(hk, b"s%0*d" % (1 + j % 9, j)))
    return out


def keys_empty_hashkey(rnd, count):
    return [D.generate_key(b"", b"s%0*d" % (1 + j % 7, j))
            for j in rnd.sample(range(4 * count + 50), count)]


def gen_tt(n, seed, *, keyfn=keys_fixed, pool=lambda n: max(4, n // 4),
           weights=(0.15, 0.25, 0.60), tt_max=2000, vlen=lambda rnd: 20, expires=(0,),
           retry=0.0):
    """weights: DELETE, unverified PUT, verified PUT.  retry: the share of ops
    that repeat an earlier op of the batch as a verified write."""
    rnd = random.Random(seed)
    val = lambda: rnd.randbytes(vlen(rnd))  # noqa: E731
    keys = keyfn(rnd, pool(n) + 8)
    (k_new_ign, k_all_ign, k_tomb, k_expired, k_absent, k_past, k_pending,
     k_tie), pool_keys = keys[:8], keys[8:]
    r0, r1, mem = {}, {}, {}
    for j, k in enumerate(pool_keys):
        m = j % 5
        if m == 0:
            r0[k] = (val(), 0, rnd.randrange(1, tt_max))
        elif m == 1:  # the newer version decides
            r0[k] = (val(), 0, tt_max)
            r1[k] = (val(), NOW + 900, rnd.randrange(1, tt_max))
        elif m == 3:
            r1[k] = (val(), 0, rnd.randrange(1, tt_max))
            if j % 4 == 0:
                mem[k] = (val(), 0, 0)
        elif m == 4:
            r0[k] = (val(), 0, rnd.randrange(1, tt_max))
            if j % 2:
                r1[k] = (None, 0, 0)
    r0[k_new_ign] = (val(), 0, 50)
    r0[k_all_ign] = (val(), 0, 100)
    r0[k_tomb] = (val(), 0, 500)
    r1[k_tomb] = (None, 0, 0)
    r1[k_expired] = (val(), NOW - 5, 900)
    mem[k_pending] = (val(), 0, 0)
    r1[k_tie] = (val(), 0, generate_timetag(15, 1))
    planted = [
        (k_new_ign, val(), 0, 60, 1), (k_new_ign, val(), 0, 55, 1),   # applied, then ignored
        (k_all_ign, val(), 0, 90, 1), (k_all_ign, val(), 0, 100, 1),  # both ignored: no row
        (k_tomb, val(), 0, 1, 1),                                     # a tombstone is dead
        (k_expired, val(), 0, 1, 1),                                  # so is an expired base
        (k_absent, val(), 0, 0, 1),                                   # and an absent key
        (k_past, val(), NOW - 1, 1000, 0), (k_past, val(), 0, 5, 1),  # stored past: dead
        (k_pending, val(), 0, 0, 1), (k_pending, val(), 0, 1, 1),     # a put stores timetag 0
        (k_tie, val(), 0, generate_timetag(15, 2), 1),                # the cluster id decides
        (k_tie, val(), 0, generate_timetag(15, 2), 1),
    ]
    fill = []
    while len(fill) < n - len(planted):
        if fill and rnd.random() < retry:
            k, v, ets, tt, _ = rnd.choice(fill)
            if v is not None:
                fill.append((k, v, ets, tt, 1))  # the same write again
                continue
        k = rnd.choice(pool_keys)
        w = rnd.random()
        if w < weights[0]:
            fill.append((k, None, 0, 0, 0))
        else:
            fill.append((k, val(), rnd.choice(expires), rnd.randrange(tt_max),
                         0 if w < weights[0] + weights[1] else 1))
    slots = set(rnd.sample(range(n), len(planted)))
    ops, p, f = [], iter(planted), iter(fill)
    for i in range(n):
        ops.append(next(p) if i in slots else next(f))
    return [r0, r1, mem], ops


# (name, generator, handle envs, epoch_now of the call)
CASES = [
    ("uniform", lambda n: gen_tt(n, 11, pool=lambda n: 2 * n, weights=(0, 0.3, 0.7)), {}, NOW),
    ("duplicate-heavy", lambda n: gen_tt(n, 12, pool=lambda n: max(4, n // 40)), {}, NOW),
    ("kinds-mixed", lambda n: gen_tt(n, 13, weights=(0.3, 0.3, 0.4)), {}, NOW),
    ("equal-timetags", lambda n: gen_tt(n, 14, tt_max=40, retry=0.4), {}, NOW),
    ("past-expire", lambda n: gen_tt(n, 15, pool=lambda n: max(4, n // 6),
                                     expires=(0, NOW - 10, NOW, NOW + 500)), {}, NOW),
    ("default-ttl", lambda n: gen_tt(n, 16, expires=(0, 0, NOW + 500)),
     {"default_ttl": "777"}, NOW),
    ("data-version-0", lambda n: gen_tt(n, 17), {"pegasus.data_version": "0"}, NOW),
    ("data-version-2", lambda n: gen_tt(n, 18, expires=(0, NOW - 10, NOW + 500)),
     {"pegasus.data_version": "2"}, NOW),
    ("variable-lengths", lambda n: gen_tt(n, 19, keyfn=keys_mixed,
                                          vlen=lambda rnd: rnd.randrange(0, 200)), {}, NOW),
    ("empty-hashkey", lambda n: gen_tt(n, 20, keyfn=keys_empty_hashkey,
                                       vlen=lambda rnd: rnd.randrange(1, 40)), {}, NOW),
]
CASE_PARAMS = [pytest.param(c, n, id="%s-%d" % (c[0], n)) for c in CASES for n in SIZES]


def case_conditions(layers, ops, applied, now):
    """what every case must contain; `applied` is the model's on data version
    >= 1.  Returns the names of the conditions that do not hold."""
    by_key = {}
    for (k, *_), ap in zip(ops, applied):
        by_key.setdefault(k, []).append(ap)
    newest = {}
    for layer in layers:
        newest.update(layer)
    missing = []
    if not (0 < sum(applied) < len(applied)):
        missing.append("ignored > 0 and applied > 0")
    if not any(a[-1] == 0 and 1 in a for a in by_key.values()):
        missing.append("newest op ignored while an older op is applied")
    if not any(1 not in a for a in by_key.values()):
        missing.append("a key all of whose ops are ignored")
    if not any(k in newest and newest[k][0] is None for k in by_key):
        missing.append("a base that is a tombstone")
    if not any(k in newest and newest[k][0] is not None and 0 < newest[k][1] <= now
               for k in by_key):
        missing.append("a base that has expired")
    if not any(k not in newest for k in by_key):
        missing.append("an absent key")
    return missing


def chain_ops(pattern, length, seed=41):
    """one key, `length` ops, for the lane / wave walk"""
    rnd = random.Random(seed * 1000 + length)
    k = D.generate_key(b"chain", b"key")
    if pattern == "rising":  # every one is applied
        return [(k, b"r%d" % i, 0, 10 + i, 1) for i in range(length)]
    if pattern == "falling":  # only the first
        return [(k, b"f%d" % i, 0, 10 + length - i, 1) for i in range(length)]
    ops = []
    for i in range(length):
        w = rnd.random()
        if w < 0.05:
            ops.append((k, None, 0, 0, 0))
        elif w < 0.15:
            ops.append((k, b"u%d" % i, 0, rnd.randrange(100), 0))
        else:
            ops.append((k, b"v%d" % i, rnd.choice((0, NOW + 50)), rnd.randrange(100), 1))
    if pattern == "past-expire":
        # an unverified PUT with the largest timetag, stored already past: the
        # verified PUT behind it has a smaller one and is applied all the same
        at = length // 2
        ops[at] = (k, b"past", NOW - 1, 1 << 40, 0)
        ops[at + 1] = (k, b"after", 0, 3, 1)
    return ops


# ---------------- CPU checks ----------------

@pytest.mark.parametrize("case,n", CASE_PARAMS)
def test_model_matches_restatement_and_oracle(oracle_lib, case, n):
    """the model's applied flags equal the literal restatement's, and the
    model's run, ingested into an oracle handle on top of the layers, reads as
    the restatement's dict does"""
    _, gen, envs, now = case
    layers, ops = gen(n)
    assert len(ops) == n
    dv, ttl = env_version(envs), env_ttl(envs)
    o, floor = open_prepared(oracle_lib, -1, envs, layers, now)
    try:
        applied, stats, run, new_floor = timetag_model(layers, ops, floor, dv, ttl, now)
        want_applied, db = restate(layers, ops, dv, ttl, now)
        assert applied == want_applied
        assert new_floor == floor + n
        assert stats["input_ops"] == n == \
            stats["ignored"] + stats["superseded"] + stats["output_records"]
        assert stats["applied"] == sum(applied)
        ingest_model_run(o, run)
        view = view_of(db, dv, now)
        for k in sorted({op[0] for op in ops}):
            err, val = o.get(k, now)
            terr, t = o.ttl(k, now)
            if k in view:
                assert (err, val) == (OK, view[k][0]), k
                assert terr == OK and (now + t if t > 0 else 0) == view[k][1], k
            else:
                assert err != OK and terr != OK, k
    finally:
        o.close()


@pytest.mark.parametrize("case", [pytest.param(c, id=c[0]) for c in CASES])
def test_cases_reach_what_they_are_for(case):
    """no case passes empty.  Data version 0 verifies nothing, so "ignored > 0"
    cannot hold there: the conditions are checked on the same batch at version
    1, and version 0 itself must apply every op."""
    _, gen, envs, now = case
    for n in SIZES:
        layers, ops = gen(n)
        dv = env_version(envs)
        applied, *_ = timetag_model(layers, ops, 1, max(dv, 1), env_ttl(envs), now)
        assert case_conditions(layers, ops, applied, now) == []
        if dv == 0:
            applied0, st0, *_ = timetag_model(layers, ops, 1, 0, env_ttl(envs), now)
            assert applied0 == [1] * n and st0["ignored"] == 0


def test_zero_timetags_without_verify_is_the_write_batch():
    for name, gen, envs, now in CASES:
        layers, ops = gen(SIZES[0])
        plain = [(k, v, ets, 0, 0) for k, v, ets, _, _ in ops]
        dv, ttl = env_version(envs), env_ttl(envs)
        applied, stats, run, floor = timetag_model(layers, plain, 7, dv, ttl, now)
        want_run, want_stats = batch_run([op[:3] for op in plain], 7, dv, ttl, now)
        assert run == want_run, name
        assert {f: stats[f] for f in WB_STAT_FIELDS} == want_stats, name
        assert applied == [1] * len(plain) and floor == 7 + len(plain)


def _one_key(writes, data_version=1):
    k = D.generate_key(b"hk", b"sk")
    ops = [(k, v, 0, tt, verify) for v, tt, verify in writes]
    return k, ops, timetag_model([{}], ops, 0, data_version)


def test_reference_put_verify_timetag_vector():
    """rocksdb_wrapper_test.cpp:131-205, put_verify_timetag"""
    local = lambda ts: generate_timetag(ts, 1)  # noqa: E731
    remote = generate_timetag(15, 2)
    k, ops, (applied, st, run, floor) = _one_key([
        (b"value_10", local(10), 0),     # 1 local, timestamp 10, cluster 1: stored
        (b"value_15", local(15), 0),     # 2 local, timestamp 15: stored
        (b"value_15_r", remote, 1),      # 3 remote, timestamp 15, cluster 2, verified
        (b"value_15_r", remote, 1),      # 4 the same write again
        (b"value_16", local(16), 0),     # 5 local, timestamp 16
        (b"value_16", local(16), 0),     # 6 the same write again, unverified
    ])
    assert applied == [1, 1, 1, 0, 1, 1]
    assert remote > local(15)  # the cluster id breaks the tie
    assert run["vals"] == D.encode_value(b"value_16", 0, local(16), 1)
    assert struct.unpack("<Q", run["sk"]) == (5 << 1,)
    assert (st["ignored"], st["superseded"], st["output_records"], floor) == (1, 4, 1, 6)
    # up to step 4: the remote write is what is stored
    _, _, (applied, _, run, _) = _one_key([(b"value_10", local(10), 0), (b"value_15", local(15), 0),
                                           (b"value_15_r", remote, 1), (b"value_15_r", remote, 1)])
    assert applied == [1, 1, 1, 0]
    assert D.decode_value(run["vals"], 1) == (0, remote, b"value_15_r")


def test_version_0_vector():
    """verify_timetag_compatible_with_version_0: a verified PUT is applied and
    no timetag is stored"""
    _, _, (applied, st, run, _) = _one_key(
        [(b"a", generate_timetag(10, 1), 0), (b"b", generate_timetag(5, 2), 1)], data_version=0)
    assert applied == [1, 1] and st["ignored"] == 0
    assert run["vals"] == D.encode_value(b"b", 0, 0, 0) == b"\0\0\0\0b"


@pytest.mark.parametrize("length", CHAIN_LENGTHS)
def test_chains_are_what_their_names_say(length):
    for pattern in CHAIN_PATTERNS:
        ops = chain_ops(pattern, length)
        assert len(ops) == length
        applied, st, run, _ = timetag_model([{}], ops, 0, 1, 0, NOW)
        assert applied == restate([{}], ops, 1, 0, NOW)[0]
        if pattern == "rising":
            assert applied == [1] * length
        elif pattern == "falling":
            assert applied == [1] + [0] * (length - 1)
        else:
            assert 0 < st["ignored"] < length
            assert any(op[4] == 0 for op in ops)  # resets
        if pattern == "past-expire":
            at = length // 2
            assert ops[at][2] == NOW - 1 and applied[at:at + 2] == [1, 1]
            assert ops[at + 1][3] < ops[at][3]


# ---------------- plumbing ----------------

def test_binding_raises_without_the_symbol(oracle_lib):
    """the oracle does not export rrdb_write_batch_timetag: the binding says
    so and does not fall back to get + put"""
    assert oracle_lib.has_write_batch_timetag is False
    o = oracle_lib.open(1, 0, -1)
    try:
        with pytest.raises(RuntimeError, match="rrdb_write_batch_timetag"):
            o.write_batch_timetag([(D.generate_key(b"h", b"s"), b"v", 0, 1, 1)])
        assert o.num_runs() == 0 and o.memtable_entries() == 0
    finally:
        o.close()


def test_verify_check_program():
    """tools/tt_verify_check.cpp (tt_verify.h against a std::map restatement,
    and the staging function), as built by __graft_entry__.build()"""
    exe = os.path.join(REPO, "bin", "tt_verify_check")
    if not os.path.exists(exe):
        pytest.skip("bin/tt_verify_check not built (run __graft_entry__.build())")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "tt_verify_check OK" in r.stdout, r.stderr


def test_header_declares_write_batch_timetag():
    src = open(os.path.join(REPO, "include", "rrdb_engine_ext.h")).read()
    assert re.search(r"\bint32_t\s+rrdb_write_batch_timetag\s*\(", src)
    assert re.search(r"\}\s*rrdb_timetag_batch_stats\s*;", src)
    for f in STAT_FIELDS:
        assert re.search(r"\buint64_t\b[^;]*\b%s\b" % f, src), f


def test_hip_lib_exports_write_batch_timetag():
    if not os.path.exists(HIP_SO):
        pytest.skip("librrdb_hip.so not built (run __graft_entry__.build())")
    assert hasattr(ctypes.CDLL(HIP_SO), "rrdb_write_batch_timetag")

