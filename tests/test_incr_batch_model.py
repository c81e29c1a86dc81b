"""Batched counter increments: the independent model, its case lists and its
CPU checks.

`incr_model` restates rrdb_incr_batch (include/rrdb_engine_ext.h, DESIGN.md
§3e) in Python: the ops of a batch applied one after the other as the
reference's incr applies them (pegasus_write_service_impl.h:264-344), the k-th
successful op taking seqno floor + k, the last successful op of every key
stored as one PUT of the decimal text.

The CPU oracle has no incr call.  The expected state is an oracle driven
through calls it has, by the sequence of the contract: flush; per op a get and
a ttl to read and, on success, a put; flush.  The reference's reads see the
memtable without flushing it; the oracle's reads flush, which would leave one
run per op.  `drive_sequence` therefore uses two oracle handles prepared alike:
the reader takes the literal sequence (its reads and puts; its run layout is
of no interest), the state handle takes flush, the very same successful puts in
the same order, flush - what the sequence leaves behind where a read does not
flush.  tests/test_incr_batch_gpu.py pins the engine against that state handle.
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
from incubator_pegasus_amd.capi import INVALID_ARGUMENT, OK
from test_write_batch_model import NOW, T, _raw18, read_checkpoint

INT64_MAX, INT64_MIN = 2**63 - 1, -(2**63)
SIZES = [T + 1, 3 * T + 7]  # the smallest that cross the sort's tile and merge boundaries
STAT_FIELDS = ("input_ops", "applied", "failed_parse", "failed_range", "output_records",
               "key_bytes", "value_bytes")

# every string the issue lists, plus the 64-byte zero-padded number
TABLE = [b"0", b"-0", b"+7", b" 12", b"\t-3", b"1 ", b"0x1F", b"-0x10", b"0x", b"0777", b"09",
         b"00", b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808",
         b"-9223372036854775809", b"0x8000000000000000", b"1\0", b"abc", b"+", b"-", b" ",
         b"0b1", b"0" * 61 + b"123"]
NOT_INTEGERS = [b"1 ", b"0x", b"09", b"9223372036854775808", b"-9223372036854775809",
                b"0x8000000000000000", b"1\0", b"abc", b"+", b"-", b" ", b"0b1"]


# ---------------- the model ----------------

def parse_i64(b):
    """dsn::buf2int64: strtoll(s, &end, 0) in the C locale over the whole
    span; None when it does not convert, leaves bytes over or leaves int64"""
    i, n = 0, len(b)
    while i < n and b[i] in b" \t\n\v\f\r":
        i += 1
    neg = False
    if i < n and b[i] in b"+-":
        neg = b[i] == 0x2D
        i += 1
    base = 10
    if i < n and b[i] == 0x30:
        if i + 2 < n and b[i + 1] in b"xX" and b[i + 2] in b"0123456789abcdefABCDEF":
            base, i = 16, i + 2
        else:
            base = 8  # the 0 itself is the first digit
    if i == n:
        return None
    acc = 0
    for c in b[i:]:
        d = "0123456789abcdefghijklmnopqrstuvwxyz".find(chr(c).lower()) if c < 128 else -1
        if d < 0 or d >= base:
            return None
        acc = acc * base + d
    v = -acc if neg else acc
    return v if INT64_MIN <= v <= INT64_MAX else None


def overlay(layers, default_ttl, epoch_now):
    """what a read at epoch_now sees after prepare(): {key: (user data, expire)}"""
    state = {}
    for j, layer in enumerate(layers):
        for k, (v, ets) in layer.items():
            if j == len(layers) - 1 and v is not None and ets == 0 and default_ttl:
                ets = (epoch_now + default_ttl) & 0xFFFFFFFF  # a put, not an ingest
            state[k] = (v, ets)
    return {k: ve for k, ve in state.items()
            if ve[0] is not None and not (0 < ve[1] <= epoch_now)}


def incr_model(base, ops, floor, data_version=1, default_ttl=0, epoch_now=0):
    """base: overlay(); ops: [(full_key, increment, directive)] in commit
    order.  Returns (new_values, errors, stats, run or None, new floor)."""
    state = dict(base)
    new_values, errors, last = [], [], {}
    applied = fparse = frange = 0
    for k, inc, d in ops:
        old = state.get(k)
        if old is not None and 0 < old[1] <= epoch_now:
            old = None  # stored by an earlier op of this batch, already past
        if old is None:
            new, ne = inc, (d if d > 0 else 0)
        else:
            if len(old[0]) == 0:
                new = inc
            else:
                cur = parse_i64(old[0])
                if cur is None:
                    new_values.append(0)
                    errors.append(INVALID_ARGUMENT)
                    fparse += 1
                    continue
                new = cur + inc
                if not INT64_MIN <= new <= INT64_MAX:
                    new_values.append(cur)
                    errors.append(INVALID_ARGUMENT)
                    frange += 1
                    continue
            ne = old[1] if d == 0 else (0 if d < 0 else d)
        if ne == 0 and default_ttl:
            ne = (epoch_now + default_ttl) & 0xFFFFFFFF
        state[k] = (b"%d" % new, ne)
        last[k] = floor + applied
        applied += 1
        new_values.append(new)
        errors.append(OK)
    keys = sorted(last)
    vals = [D.encode_value(state[k][0], state[k][1], 0, data_version) for k in keys]
    koff, voff = [0], [0]
    for k, v in zip(keys, vals):
        koff.append(koff[-1] + len(k))
        voff.append(voff[-1] + len(v))
    run = None
    if keys:
        run = {
            "n": len(keys),
            "keys": b"".join(keys),
            "koff": struct.pack("<%dQ" % len(koff), *koff),
            "vals": b"".join(vals),
            "voff": struct.pack("<%dQ" % len(voff), *voff),
            "sk": struct.pack("<%dQ" % len(keys), *[last[k] << 1 for k in keys]),
        }
    stats = dict(input_ops=len(ops), applied=applied, failed_parse=fparse, failed_range=frange,
                 output_records=len(keys), key_bytes=koff[-1], value_bytes=voff[-1])
    return new_values, errors, stats, run, floor + applied


# ---------------- driving a backend ----------------

def prepare(part, layers, data_version, epoch_now):
    """layers[:-1] become ingested runs, layers[-1] pending memtable entries.
    Every layer is {key: (user data or None, expire_ts)}.  Returns the handle's
    sequence floor afterwards."""
    seq, floor = 1, 0
    for layer in layers[:-1]:
        recs = []
        for k in sorted(layer):
            v, ets = layer[k]
            recs.append((k, b"" if v is None else D.encode_value(v, ets, 0, data_version), seq,
                         1 if v is None else 0))
            seq += 1
        if recs:
            part.ingest_run(recs)
            floor = seq
    for k, (v, ets) in layers[-1].items():
        hk, sk = D.restore_key(k)
        if v is None:
            assert part.remove(hk, sk) == OK
        else:
            assert part.put(hk, sk, v, ets, epoch_now) == OK
        floor += 1
    return floor


def drive_sequence(reader, state, ops, epoch_now):
    """the contract's sequence through calls every backend has; see the module
    docstring for the two handles.  Returns (new_values, errors)."""
    new_values, errors = [], []
    assert state.flush() == OK
    for k, inc, d in ops:
        err, val = reader.get(k, epoch_now)
        if err != OK:
            new, ne = inc, (d if d > 0 else 0)
        else:
            terr, ttl = reader.ttl(k, epoch_now)
            assert terr == OK
            stored = epoch_now + ttl if ttl > 0 else 0
            if len(val) == 0:
                new = inc
            else:
                cur = parse_i64(val)
                if cur is None:
                    new_values.append(0)
                    errors.append(INVALID_ARGUMENT)
                    continue
                new = cur + inc
                if not INT64_MIN <= new <= INT64_MAX:
                    new_values.append(cur)
                    errors.append(INVALID_ARGUMENT)
                    continue
            ne = stored if d == 0 else (0 if d < 0 else d)
        hk, sk = D.restore_key(k)
        for p in (reader, state):
            assert p.put(hk, sk, b"%d" % new, ne, epoch_now) == OK
        new_values.append(new)
        errors.append(OK)
    assert state.flush() == OK
    return new_values, errors


# ---------------- the case lists ----------------
# a generator returns (layers, ops) for n ops

def _fresh(rnd, count, lo=0):
    return _raw18(rnd.sample(range(lo, lo + 10 * count + 100), count))


def _inc(rnd):
    return rnd.choice((1, 1, -1, 7, -300, 10**12, rnd.randrange(-10**6, 10**6)))


def gen_distinct_fixed(n, seed):
    rnd = random.Random(seed)
    return [{}], [(k, _inc(rnd), 0) for k in _fresh(rnd, n)]


def gen_distinct_mixed(n, seed):
    """key lengths from 3 bytes up, an empty hashkey among them"""
    rnd = random.Random(seed)
    ops = []
    for j in rnd.sample(range(4 * n), n):
        hl = j % 23
        hk = (b"h%d." % j).ljust(hl, b"x")[:hl] if hl else b""
        ops.append((D.generate_key(hk, b"s%0*d" % (1 + j % 9, j)), _inc(rnd), 0))
    return [{}], ops


def gen_one_key(n, seed, base=None):
    rnd = random.Random(seed)
    k = D.generate_key(b"only", b"one")
    layers = [{k: (base, 0)}, {}] if base is not None else [{}]
    return layers, [(k, rnd.randrange(-1000, 1000), 0) for _ in range(n)]


def gen_hot_key(n, seed):
    """half the ops on one key, between singletons and pairs; the hot key has
    a stored base"""
    rnd = random.Random(seed)
    hot = D.generate_key(b"hot", b"counter")
    cold = _fresh(rnd, n)
    ops, c = [], 0
    while len(ops) < n:
        ops.append((hot, _inc(rnd), 0))
        if len(ops) < n:
            k = cold[c]
            c += 1
            ops.append((k, _inc(rnd), 0))
            if rnd.random() < 0.3 and len(ops) + 1 < n:
                ops.insert(rnd.randrange(len(ops)), (k, _inc(rnd), 0))
    return [{hot: (b"1000000", 0)}, {}], ops[:n]


def gen_layers(n, seed):
    """bases spread over three ingested runs and a pending memtable: newest
    version wins, a tombstoned base, an expired base, an empty base with a
    TTL, and every TABLE string as a base with two or more ops on it"""
    rnd = random.Random(seed)
    keys = _fresh(rnd, 40 + len(TABLE))
    r0, r1, r2, mem = {}, {}, {}, {}
    for j, k in enumerate(keys[:32]):
        r0[k] = (b"%d" % (100 + j), 0)
        if j % 2:
            r1[k] = (b"%d" % (200 + j), NOW + 900 if j % 3 == 0 else 0)
        if j % 4 == 1:
            r2[k] = (b"%d" % (300 + j), 0)
        if j % 8 == 3:
            mem[k] = (b"%d" % (400 + j), 0)
    tomb_r, tomb_m, expired, empty_ttl, gone_old = keys[32:37]
    r0[tomb_r] = (b"5", 0)
    r2[tomb_r] = (None, 0)
    r1[tomb_m] = (b"6", 0)
    mem[tomb_m] = (None, 0)
    r1[expired] = (b"77", NOW - 5)
    r0[empty_ttl] = (b"12", 0)
    r2[empty_ttl] = (b"", NOW + 300)
    r0[gone_old] = (b"abc", 0)  # a non-integer that a newer integer hides
    mem[gone_old] = (b"9", NOW + 50)
    table_keys = keys[40:40 + len(TABLE)]
    for j, (k, s) in enumerate(zip(table_keys, TABLE)):
        (r0, r1, r2, mem)[j % 4][k] = (s, NOW + 1000 if j % 5 == 0 else 0)
    special = keys[:37] + table_keys
    ops = []
    for k in special:
        for _ in range(2 + rnd.randrange(3)):
            ops.append((k, _inc(rnd), 0))
    fresh = _fresh(rnd, n, lo=10**7)
    while len(ops) < n:
        ops.append((fresh[len(ops)], _inc(rnd), 0))
    ops = ops[:n]
    rnd.shuffle(ops)
    return [r0, r1, r2, mem], ops


def gen_range_edges(n, seed):
    rnd = random.Random(seed)
    keys = _fresh(rnd, 8)
    base = {keys[0]: (b"%d" % (INT64_MAX - 1), 0), keys[1]: (b"%d" % INT64_MIN, 0),
            keys[2]: (b"-1", 0), keys[3]: (b"%d" % (INT64_MAX - 100), 0),
            keys[4]: (b"%d" % (INT64_MIN + 3), 0), keys[5]: (b"0", 0)}
    chains = {
        keys[0]: [1, 1, -5, 10],
        keys[1]: [-1, 1],
        keys[2]: [INT64_MIN],
        # longer than a lane's walk: fine, then over the top, back down, fine again
        keys[3]: [1] * 90 + [50, 50, -500] + [3] * 120,
        keys[4]: [-1, -1, -1, -1, 5, -9, -1],
        # every prefix inside int64 by a hair, then INT64_MAX itself, then one more
        keys[5]: [INT64_MAX, -INT64_MAX, INT64_MIN, INT64_MAX, INT64_MAX, 1, 1, 1, -2],
        # no base: the first op sets it
        keys[6]: [INT64_MAX, 1, -1],
        keys[7]: [INT64_MIN, -1, 1],
    }
    return [base, {}], _interleave(rnd, chains, n, lambda i: 0)


def _interleave(rnd, chains, n, directive, fresh_lo=10**7):
    """the chains' ops in chain order, spread between ops on fresh keys"""
    total = sum(len(c) for c in chains.values())
    fresh = _fresh(rnd, max(1, n - total), lo=fresh_lo)
    slots = sorted(rnd.sample(range(n), total)) if total <= n else list(range(total))
    order = [k for k, c in chains.items() for _ in c]
    rnd.shuffle(order)
    cursor = {k: 0 for k in chains}
    ops, f, it = [], 0, iter(order)
    slot_set = set(slots)
    for i in range(max(n, total)):
        if i in slot_set:
            k = next(it)
            v = chains[k][cursor[k]]
            cursor[k] += 1
            ops.append((k, v[0], v[1]) if isinstance(v, tuple) else (k, v, directive(i)))
        else:
            ops.append((fresh[f], _inc(rnd), directive(i)))
            f += 1
    return ops[:n] if total <= n else ops


def gen_ttl(n, seed):
    """directives 0, -1 and > 0 along chains short and long; a positive one
    that is already past, so that the next op of the key starts over"""
    rnd = random.Random(seed)
    keys = _fresh(rnd, 6)
    base = {keys[0]: (b"10", NOW + 100), keys[1]: (b"20", 0), keys[2]: (b"", NOW + 40),
            keys[3]: (b"30", NOW + 70)}

    def dirs(count, past_every=0):
        out = []
        for j in range(count):
            d = rnd.choice((0, 0, 0, -1, NOW + 10 + j, NOW + 5000))
            if past_every and j % past_every == past_every - 1:
                d = rnd.choice((NOW, NOW - 3, 1))
            out.append((rnd.randrange(-50, 50), d))
        return out

    chains = {
        keys[0]: dirs(7),
        keys[1]: dirs(5, past_every=2),
        keys[2]: [(4, 0), (5, -1), (6, 0)],
        keys[3]: dirs(150),               # a wave's chain, associative all the way
        keys[4]: dirs(200, past_every=60),  # a wave's chain that resets on the way
        keys[5]: [(1, NOW - 1), (2, 0), (3, NOW + 9), (4, 0)],
    }
    mixed = lambda i: (0, 0, -1, NOW + 77, NOW - 7)[i % 5]  # noqa: E731
    return [base, {}], _interleave(rnd, chains, n, mixed)


def gen_all_fail(n, seed):
    """every key has a base that is no integer"""
    rnd = random.Random(seed)
    keys = _fresh(rnd, max(2, n // 3))
    bad = NOT_INTEGERS
    layer = {k: (bad[j % len(bad)], 0) for j, k in enumerate(keys)}
    hot = keys[0]  # long enough for the wave kernel
    return [layer, {}], [(hot if i % 4 == 0 else rnd.choice(keys), _inc(rnd), 0)
                         for i in range(n)]


def gen_mixed_fail(n, seed):
    """failed ops between successful ones: a third of the keys cannot parse,
    one counter sits at the top of the range"""
    rnd = random.Random(seed)
    keys = _fresh(rnd, max(3, n // 2))
    layer = {k: (b"1\0" if j % 3 == 0 else b"%d" % j, 0) for j, k in enumerate(keys[: n // 4])}
    layer[keys[-1]] = (b"%d" % (INT64_MAX - 2), 0)
    ops = [(keys[-1] if i % 50 == 0 else rnd.choice(keys), rnd.choice((1, 1, 2, -1)), 0)
           for i in range(n)]
    return [layer, {}], ops


# (name, generator, handle envs, epoch_now of the call)
CASES = [
    ("distinct-fixed", lambda n: gen_distinct_fixed(n, 11), {}, NOW),
    ("distinct-mixed", lambda n: gen_distinct_mixed(n, 12), {}, NOW),
    ("one-key", lambda n: gen_one_key(n, 13), {}, NOW),
    ("one-key-hex-base", lambda n: gen_one_key(n, 14, b" -0x10"), {}, NOW),
    ("hot-key", lambda n: gen_hot_key(n, 15), {}, NOW),
    ("layers", lambda n: gen_layers(n, 16), {}, NOW),
    ("range-edges", lambda n: gen_range_edges(n, 17), {}, NOW),
    ("ttl", lambda n: gen_ttl(n, 18), {}, NOW),
    ("ttl-default-ttl", lambda n: gen_ttl(n, 19), {"default_ttl": "777"}, NOW),
    ("ttl-data-version-0", lambda n: gen_ttl(n, 20), {"pegasus.data_version": "0"}, NOW),
    ("layers-data-version-2", lambda n: gen_layers(n, 21), {"pegasus.data_version": "2"}, NOW),
    ("ttl-data-version-2", lambda n: gen_ttl(n, 22),
     {"pegasus.data_version": "2", "default_ttl": "50"}, NOW),
    ("all-fail", lambda n: gen_all_fail(n, 23), {}, NOW),
    ("mixed-fail", lambda n: gen_mixed_fail(n, 24), {}, NOW),
]
CASE_PARAMS = [pytest.param(c, n, id="%s-%d" % (c[0], n)) for c in CASES for n in SIZES]


def env_version(envs):
    return int(envs.get("pegasus.data_version", 1))


def env_ttl(envs):
    return int(envs.get("default_ttl", 0))


def open_prepared(lib, gpu_id, envs, layers, epoch_now):
    p = lib.open(1, 0, gpu_id)
    if envs:
        assert p.set_envs(envs) == OK
    return p, prepare(p, layers, env_version(envs), epoch_now)


# ---------------- CPU checks ----------------

def _libc_parse(libc, s):
    buf = ctypes.create_string_buffer(s, len(s) + 1)
    end = ctypes.c_void_p()
    ctypes.set_errno(0)
    v = libc.strtoll(buf, ctypes.byref(end), 0)
    if end.value - ctypes.addressof(buf) != len(s) or ctypes.get_errno() != 0:
        return None
    return v


def test_parse_equals_libc_strtoll():
    libc = ctypes.CDLL(None, use_errno=True)
    libc.strtoll.restype = ctypes.c_longlong
    libc.strtoll.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    rnd = random.Random(31)
    alphabet = b" \t+-0123456789xXaAfF\0"
    strings = TABLE + [bytes(rnd.choice(alphabet) for _ in range(rnd.randrange(1, 22)))
                       for _ in range(2000)]
    for s in strings:
        assert parse_i64(s) == _libc_parse(libc, s), s
    # the table really holds both kinds
    assert parse_i64(b"0x1F") == 31 and parse_i64(b"-0x10") == -16 and parse_i64(b"0777") == 511
    assert parse_i64(TABLE[-1]) == 0o123 and len(TABLE[-1]) == 64
    assert [s for s in TABLE if parse_i64(s) is None] == NOT_INTEGERS


@pytest.mark.parametrize("case,n", CASE_PARAMS)
def test_model_matches_oracle_sequence(oracle_lib, tmp_path, case, n):
    """incr_model == the contract's sequence on the oracle: per-op results,
    stats, the run byte for byte and the floor"""
    _, gen, envs, now = case
    layers, ops = gen(n)
    assert len(ops) == n
    reader, _ = open_prepared(oracle_lib, -1, envs, layers, now)
    state, floor = open_prepared(oracle_lib, -1, envs, layers, now)
    try:
        runs_before = state.num_runs() + (1 if layers[-1] else 0)
        got_v, got_e = drive_sequence(reader, state, ops, now)
        man, runs = read_checkpoint(state, tmp_path)
    finally:
        reader.close()
        state.close()
    new_values, errors, stats, run, new_floor = incr_model(
        overlay(layers, env_ttl(envs), now), ops, floor, env_version(envs), env_ttl(envs), now)
    assert new_values == got_v and errors == got_e
    assert man["next_seq_floor"] == new_floor == floor + stats["applied"]
    assert man["n_runs"] == runs_before + (1 if run else 0)
    if run:
        assert runs[-1] == run
    assert stats["applied"] + stats["failed_parse"] + stats["failed_range"] == n
    assert stats["applied"] == errors.count(OK)


def test_cases_reach_what_they_are_for():
    """the generators really produce the situations their names promise"""
    by = {c[0]: c for c in CASES}

    def run(name, n=SIZES[0]):
        _, gen, envs, now = by[name]
        layers, ops = gen(n)
        return incr_model(overlay(layers, env_ttl(envs), now), ops, 1, env_version(envs),
                          env_ttl(envs), now)

    _, _, st, r, _ = run("all-fail")
    assert st["applied"] == 0 and st["failed_parse"] == SIZES[0] and r is None
    _, _, st, _, _ = run("range-edges")
    assert st["failed_range"] >= 8 and st["applied"] > SIZES[0] - 40
    _, _, st, _, _ = run("layers")
    assert st["failed_parse"] >= 2 * len(NOT_INTEGERS) and st["failed_range"] >= 1
    _, _, st, _, _ = run("mixed-fail")
    assert st["failed_parse"] > 50 and st["failed_range"] > 5 and st["applied"] > 1000
    nv, _, st, r, _ = run("one-key")
    assert st["output_records"] == 1 and st["applied"] == SIZES[0]
    _, ops = by["one-key"][1](SIZES[0])
    assert nv[-1] == sum(o[1] for o in ops)


def test_binding_raises_without_the_symbol(oracle_lib):
    """the oracle does not export rrdb_incr_batch: the binding says so and
    does not fall back to get + put"""
    assert oracle_lib.has_incr_batch is False
    o = oracle_lib.open(1, 0, -1)
    try:
        assert o.put(b"h", b"s", b"5", 0, 0) == OK
        with pytest.raises(RuntimeError, match="rrdb_incr_batch"):
            o.incr_batch([(D.generate_key(b"h", b"s"), 1, 0)])
        assert o.num_runs() == 0 and o.memtable_entries() == 1
    finally:
        o.close()


def test_num_check_program():
    """tools/incr_num_check.cpp (incr_num.h's parse and format against libc),
    as built by __graft_entry__.build()"""
    exe = os.path.join(REPO, "bin", "incr_num_check")
    if not os.path.exists(exe):
        pytest.skip("bin/incr_num_check not built (run __graft_entry__.build())")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "incr_num_check OK" in r.stdout, r.stderr


# ---------------- the two that fail before the change ----------------

def test_header_declares_incr_batch():
    src = open(os.path.join(REPO, "include", "rrdb_engine_ext.h")).read()
    assert re.search(r"\bint32_t\s+rrdb_incr_batch\s*\(", src)
    assert re.search(r"\}\s*rrdb_incr_batch_stats\s*;", src)
    for f in STAT_FIELDS:
        assert re.search(r"\buint64_t\b[^;]*\b%s\b" % f, src), f


def test_hip_lib_exports_incr_batch():
    if not os.path.exists(HIP_SO):
        pytest.skip("librrdb_hip.so not built (run __graft_entry__.build())")
    assert hasattr(ctypes.CDLL(HIP_SO), "rrdb_incr_batch")
