"""Batched writes: the independent model, its case lists and its CPU checks.

`batch_run` restates rrdb_write_batch (include/rrdb_engine_ext.h, DESIGN.md
§3d) in Python: op i of the batch gets seqno floor + i, a PUT value is encoded
with the handle's value header (timetag 0, write-time default_ttl), a remove is
a tombstone with an empty value; the run is the ops sorted by key ascending and
seqno descending, first of every equal-key group kept.

The CPU oracle has no batch call.  The expected state is an oracle handle
driven through put / remove in the same order and then flush; physical parity
goes through checkpoints, which both backends write in one format.  The tests
here pin the model (and so the case lists' expectations) against the oracle
that way; tests/test_write_batch_gpu.py pins the engine against the oracle.
"""
import ctypes
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import HIP_SO, REPO
from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import OK

WB_TILE = 2048  # engine_common.h; test_wb_tile_constant holds the two together
T = WB_TILE
NOW = 100_000  # test_split_model's clock: its LATER = NOW + 600 is past NOW + 500

# one tile and its edges; first merge pass and slice edges; an odd tile carried
# through a pass; a full power of two; six passes
SIZES = [1, 2, 3, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 7, 5 * T + 3, 8 * T,
         33 * T + 11]
VAR_SIZES = [65, T + 1, 3 * T + 7]
ONE_KEY_SIZES = [T + 1, 3 * T + 7]
STAT_FIELDS = ("input_ops", "output_records", "superseded", "puts", "removes", "key_bytes",
               "value_bytes")


# ---------------- the model ----------------

def batch_run(ops, floor, data_version=1, default_ttl=0, epoch_now=0):
    """ops: [(full_key, value_or_None, expire_ts)] in commit order.  Returns
    (run, stats): run = the five checkpoint columns as bytes plus n."""
    newest = {}
    for i, (k, v, ets) in enumerate(ops):
        if v is None:
            newest[k] = (b"", floor + i, 1)
        else:
            if ets == 0 and default_ttl:
                ets = (epoch_now + default_ttl) & 0xFFFFFFFF
            newest[k] = (D.encode_value(v, ets, 0, data_version), floor + i, 0)
    keys = sorted(newest)
    koff, voff = [0], [0]
    for k in keys:
        koff.append(koff[-1] + len(k))
        voff.append(voff[-1] + len(newest[k][0]))
    run = {
        "n": len(keys),
        "keys": b"".join(keys),
        "koff": struct.pack("<%dQ" % len(koff), *koff),
        "vals": b"".join(newest[k][0] for k in keys),
        "voff": struct.pack("<%dQ" % len(voff), *voff),
        "sk": struct.pack("<%dQ" % len(keys), *[(newest[k][1] << 1) | newest[k][2]
                                                for k in keys]),
    }
    puts = sum(1 for k in keys if newest[k][2] == 0)
    stats = dict(input_ops=len(ops), output_records=len(keys), superseded=len(ops) - len(keys),
                 puts=puts, removes=len(keys) - puts, key_bytes=koff[-1], value_bytes=voff[-1])
    return run, stats


def apply_ops(part, ops, epoch_now=0):
    """the batch through the one-record write path (any backend)"""
    for k, v, ets in ops:
        hk, sk = D.restore_key(k)
        if v is None:
            assert part.remove(hk, sk) == OK
        else:
            assert part.put(hk, sk, v, ets, epoch_now) == OK


def read_checkpoint(part, directory, decree=1):
    """checkpoint `part` and read it back: (manifest dict, [run column dict])"""
    assert part.checkpoint(str(directory), decree) == OK
    path = os.path.join(str(directory), "checkpoint.%d" % decree)
    man = {"run": []}
    for line in open(os.path.join(path, "MANIFEST")).read().splitlines():
        f = line.split()
        if f[0] in ("data_version", "next_seq_floor", "n_runs"):
            man[f[0]] = int(f[1])
        elif f[0] == "run":
            man["run"].append((int(f[1]), int(f[2])))
    runs = []
    for i, n in man["run"]:
        r = {"n": n}
        for ext in ("keys", "koff", "vals", "voff", "sk"):
            with open(os.path.join(path, "run_%d.%s" % (i, ext)), "rb") as fh:
                r[ext] = fh.read()
        runs.append(r)
    return man, runs


# ---------------- the case lists ----------------

def _raw18(ids):
    raw = D.make_raw_keys(np.asarray(ids, dtype=np.uint64))
    return [bytes(r) for r in raw]


def ops_fixed(n, seed, order="random", expire=False):
    """unique 18-byte keys, 100-byte values: the all-fixed-stride batch"""
    rnd = random.Random(seed)
    ids = rnd.sample(range(10 * n + 100), n)
    if order == "ascending":
        ids.sort()
    elif order == "descending":
        ids.sort(reverse=True)
    ets = [rnd.choice((0, NOW - 10, NOW + 500)) if expire else 0 for _ in ids]
    return [(k, rnd.randbytes(100), e) for k, e in zip(_raw18(ids), ets)]


def ops_dups(n, seed):
    """ids from n/4 distinct keys, puts and removes mixed: equal-key groups
    straddle tile and slice boundaries; a remove after a put and a put after a
    remove both occur"""
    rnd = random.Random(seed)
    keys = _raw18(rnd.sample(range(10 * n + 100), max(1, n // 4)))
    return [(rnd.choice(keys), None if rnd.random() < 0.3 else b"v%07d" % i, 0)
            for i in range(n)]


def ops_one_key(n, seed, last_is_put=True):
    rnd = random.Random(seed)
    k = D.generate_key(b"only", b"one")
    ops = [(k, None if rnd.random() < 0.3 else b"v%d" % i, 0) for i in range(n)]
    ops[-1] = (k, b"last" if last_is_put else None, 0)
    return ops


def ops_zero_pad(n, seed):
    """zero padding against true length, at and across the word boundary"""
    rnd = random.Random(seed)
    sks = [b"", b"\0", b"\0\0", b"s", b"s\0", b"s" + b"\0" * 9]
    keys = [D.generate_key(b"hk", s) for s in sks]
    return [(rnd.choice(keys), None if rnd.random() < 0.2 else b"z%d" % i, 0)
            for i in range(n)]


def ops_long_prefix(n, seed):
    """40-byte common hashkey, sortkeys that first differ after byte 30"""
    rnd = random.Random(seed)
    hk = b"H" * 40
    return [(D.generate_key(hk, b"p" * 30 + b"%06d" % rnd.randrange(2 * n)),
             b"v%d" % i, 0) for i in range(n)]


def ops_word_ties(n, seed):
    """sortkey = one of three 8-byte groups + 12 random bytes: every
    comparison inside a group ties in the sort word"""
    rnd = random.Random(seed)
    groups = [b"groupAAA", b"groupBBB", b"hroupCCC"]
    pool = [D.generate_key(b"g", rnd.choice(groups) + rnd.randbytes(12))
            for _ in range(max(1, (3 * n) // 4))]
    return [(rnd.choice(pool), None if rnd.random() < 0.1 else b"w%d" % i, 0)
            for i in range(n)]


def ops_empty_hashkey(n, seed):
    rnd = random.Random(seed)
    return [(D.generate_key(b"", b"s%0*d" % (1 + i % 7, rnd.randrange(n))), b"e%d" % i, 0)
            for i in range(n)]


def ops_hashkey_lengths(n, seed):
    """hashkey lengths 0..40 (a sortkey is always there), some removes"""
    rnd = random.Random(seed)
    ops = []
    for i in range(n):
        j = rnd.randrange(n)
        hl = j % 41
        hk = (b"h%d." % j).ljust(hl, b"x")[:hl]
        k = D.generate_key(hk, b"s%0*d" % (3 + j % 5, j))
        ops.append((k, None if rnd.random() < 0.15 else b"l%d" % i, 0))
    return ops


def ops_value_lengths(n, seed):
    """values of 0..300 bytes, the empty one included; unique 18-byte keys"""
    rnd = random.Random(seed)
    lens = [0, 1, 300] + [rnd.randrange(301) for _ in range(n)]
    return [(k, rnd.randbytes(lens[i]), 0)
            for i, k in enumerate(_raw18(rnd.sample(range(10 * n + 100), n)))]


def ops_all_remove(n, seed):
    rnd = random.Random(seed)
    return [(k, None, 0) for k in _raw18([rnd.randrange(n) for _ in range(n)])]


# (name, generator, sizes, handle envs, epoch_now of the write)
CASES = [
    ("fixed-random", lambda n: ops_fixed(n, 11), SIZES, {}, 0),
    ("fixed-ascending", lambda n: ops_fixed(n, 12, "ascending"), SIZES, {}, 0),
    ("fixed-descending", lambda n: ops_fixed(n, 13, "descending"), SIZES, {}, 0),
    ("dups", lambda n: ops_dups(n, 14), SIZES, {}, 0),
    ("one-key-put-last", lambda n: ops_one_key(n, 15, True), ONE_KEY_SIZES, {}, 0),
    ("one-key-remove-last", lambda n: ops_one_key(n, 16, False), ONE_KEY_SIZES, {}, 0),
    ("zero-pad", lambda n: ops_zero_pad(n, 17), VAR_SIZES, {}, 0),
    ("long-prefix", lambda n: ops_long_prefix(n, 18), VAR_SIZES, {}, 0),
    ("word-ties", lambda n: ops_word_ties(n, 19), VAR_SIZES, {}, 0),
    ("empty-hashkey", lambda n: ops_empty_hashkey(n, 20), VAR_SIZES, {}, 0),
    ("hashkey-lengths", lambda n: ops_hashkey_lengths(n, 21), VAR_SIZES, {}, 0),
    ("value-lengths", lambda n: ops_value_lengths(n, 22), VAR_SIZES, {}, 0),
    ("expire-ts", lambda n: ops_fixed(n, 23, expire=True), VAR_SIZES, {}, 0),
    ("default-ttl", lambda n: ops_fixed(n, 24, expire=True), VAR_SIZES,
     {"default_ttl": "777"}, NOW),
    ("data-version-0", lambda n: ops_dups(n, 25), VAR_SIZES, {"pegasus.data_version": "0"}, 0),
    ("data-version-2", lambda n: ops_dups(n, 26), VAR_SIZES, {"pegasus.data_version": "2"}, 0),
    ("data-version-2-fixed", lambda n: ops_fixed(n, 27), [T + 1],
     {"pegasus.data_version": "2"}, 0),
    ("all-remove", lambda n: ops_all_remove(n, 28), VAR_SIZES, {}, 0),
]
CASE_PARAMS = [pytest.param(c, n, id="%s-%d" % (c[0], n)) for c in CASES for n in c[2]]


def env_version(envs):
    return int(envs.get("pegasus.data_version", 1))


# ---------------- CPU checks ----------------

@pytest.mark.parametrize("case,n", CASE_PARAMS)
def test_model_matches_oracle_flush(oracle_lib, tmp_path, case, n):
    """batch_run == put/remove x n + flush on the oracle, byte for byte, with
    two memtable entries flushed ahead so the floor is not 0"""
    _, gen, _, envs, epoch_now = case
    ops = gen(n)
    o = oracle_lib.open(1, 0, -1)
    try:
        if envs:
            assert o.set_envs(envs) == OK
        assert o.put(b"before", b"a", b"x", 0, epoch_now) == OK
        assert o.remove(b"before", b"b") == OK
        assert o.flush() == OK
        apply_ops(o, ops, epoch_now)
        assert o.flush() == OK
        man, runs = read_checkpoint(o, tmp_path)
    finally:
        o.close()
    run, stats = batch_run(ops, 2, env_version(envs), int(envs.get("default_ttl", 0)), epoch_now)
    assert man["data_version"] == env_version(envs)
    assert man["next_seq_floor"] == 2 + n
    assert man["n_runs"] == 2 and man["run"] == [(0, 2), (1, run["n"])]
    assert runs[1] == run
    assert stats["output_records"] + stats["superseded"] == n
    assert stats["key_bytes"] == len(run["keys"]) and stats["value_bytes"] == len(run["vals"])


def test_model_newest_op_wins():
    k1, k2 = D.generate_key(b"a", b"1"), D.generate_key(b"a", b"2")
    run, st = batch_run([(k1, b"x", 0), (k2, None, 0), (k1, None, 0), (k2, b"y", 9)], 10)
    assert run["keys"] == k1 + k2
    assert struct.unpack("<2Q", run["sk"]) == ((12 << 1) | 1, (13 << 1) | 0)
    assert run["vals"] == D.encode_value(b"y", 9, 0, 1)
    assert st == dict(input_ops=4, output_records=2, superseded=2, puts=1, removes=1,
                      key_bytes=8, value_bytes=13)


def test_binding_raises_without_the_symbol(oracle_lib):
    """the oracle does not export rrdb_write_batch: the binding says so, as
    split() does, and does not fall back to put/remove"""
    assert oracle_lib.has_write_batch is False
    o = oracle_lib.open(1, 0, -1)
    try:
        with pytest.raises(RuntimeError, match="rrdb_write_batch"):
            o.write_batch([(D.generate_key(b"h", b"s"), b"v", 0)])
        assert o.num_runs() == 0 and o.memtable_entries() == 0
    finally:
        o.close()


def test_stage_check_program():
    """tools/wb_stage_check.cpp (malformed and valid batches through the host
    validation and staging code), as built by __graft_entry__.build()"""
    exe = os.path.join(REPO, "bin", "wb_stage_check")
    if not os.path.exists(exe):
        pytest.skip("bin/wb_stage_check not built (run __graft_entry__.build())")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "wb_stage_check OK" in r.stdout, r.stderr


# ---------------- the three that fail before the change ----------------

def test_header_declares_write_batch():
    src = open(os.path.join(REPO, "include", "rrdb_engine_ext.h")).read()
    assert re.search(r"\bint32_t\s+rrdb_write_batch\s*\(", src)
    assert "rrdb_write_batch_stats" in src


def test_hip_lib_exports_write_batch():
    if not os.path.exists(HIP_SO):
        pytest.skip("librrdb_hip.so not built (run __graft_entry__.build())")
    assert hasattr(ctypes.CDLL(HIP_SO), "rrdb_write_batch")


def test_wb_tile_constant():
    src = open(os.path.join(REPO, "incubator_pegasus_amd", "csrc", "engine_common.h")).read()
    m = re.search(r"^#define\s+WB_TILE\s+(\d+)\s*$", src, re.M)
    assert m, "WB_TILE is not defined in engine_common.h"
    assert int(m.group(1)) == WB_TILE
