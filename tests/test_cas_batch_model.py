"""Batched check-and-mutate: the independent model, its case lists and its CPU
checks.

`cas_model` restates rrdb_check_and_mutate_batch (include/rrdb_engine_ext.h,
DESIGN.md §3f) in Python: the ops of a batch applied one after the other as the
reference's check_and_mutate applies them (pegasus_write_service_impl.h:710-833,
validate_check at :1144-1270), the k-th applied mutation taking seqno
floor + k, the last applied mutation of every key stored.

The CPU oracle has no check_and_mutate call.  The expected state is an oracle
driven through calls it has, by the sequence of the contract: flush; per op a
get and, when the check passes, its puts and removes; flush.  As
tests/test_incr_batch_model.py explains, the oracle's reads flush where the
reference's do not, so `drive_sequence` uses two oracle handles prepared alike:
the reader takes the literal sequence, the state handle takes flush, the very
same applied writes in the same order, flush.  tests/test_cas_batch_gpu.py pins
the engine against that state handle.

An op is (check_key, check_type, operand, [(key, value_or_None, expire_ts), ...],
return_check_value); None = remove.  A mutation may carry a fourth element, its
raw kind byte, so that a case can hold a kind that is neither PUT nor DELETE.
Every generator takes the entry count E = ops + mutations it has to hit.
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
from incubator_pegasus_amd.capi import INVALID_ARGUMENT, OK, TRY_AGAIN
from test_incr_batch_model import (env_ttl, env_version, open_prepared, overlay, parse_i64)
from test_write_batch_model import NOW, T, read_checkpoint

SIZES = [T + 1, 3 * T + 7]  # entries: the smallest that cross the sort's tile and merge boundaries
STAT_FIELDS = ("input_ops", "passed", "failed_check", "failed_invalid", "malformed",
               "mutations_applied", "output_records", "puts", "removes", "key_bytes",
               "value_bytes")

(CT_NO_CHECK, CT_NOT_EXIST, CT_NOT_EXIST_OR_EMPTY, CT_EXIST, CT_NOT_EMPTY, CT_ANYWHERE, CT_PREFIX,
 CT_POSTFIX, CT_B_LT, CT_B_LE, CT_B_EQ, CT_B_GE, CT_B_GT, CT_I_LT, CT_I_LE, CT_I_EQ, CT_I_GE,
 CT_I_GT) = range(18)


# ---------------- the model ----------------

def validate_check(ct, operand, exist, value):
    """validate_check: (passed, invalid_argument)"""
    if ct == CT_NO_CHECK:
        return True, False
    if ct == CT_NOT_EXIST:
        return not exist, False
    if ct == CT_NOT_EXIST_OR_EMPTY:
        return (not exist) or len(value) == 0, False
    if ct == CT_EXIST:
        return exist, False
    if ct == CT_NOT_EMPTY:
        return exist and len(value) != 0, False
    if not exist:
        return False, False
    if ct in (CT_ANYWHERE, CT_PREFIX, CT_POSTFIX):
        if len(operand) == 0:
            return True, False
        if len(value) < len(operand):
            return False, False
        if ct == CT_ANYWHERE:
            return operand in value, False
        if ct == CT_PREFIX:
            return value.startswith(operand), False
        return value.endswith(operand), False
    if CT_B_LT <= ct <= CT_B_GT:
        a, b, rel = value, operand, ct - CT_B_LT  # bytes order: memcmp, then the shorter first
    else:
        a, b, rel = parse_i64(value), parse_i64(operand), ct - CT_I_LT
        if a is None or b is None:
            return False, True
    c = (a > b) - (a < b)
    return (c < 0, c <= 0, c == 0, c >= 0, c > 0)[rel], False


def kind_of(m):
    return m[3] if len(m) > 3 else (0 if m[1] is not None else 1)


def is_malformed(ct, muts):
    return len(muts) == 0 or any(kind_of(m) > 1 for m in muts) or not 0 <= ct <= 17


def cas_model(base, ops, floor, data_version=1, default_ttl=0, epoch_now=0):
    """base: overlay().  Returns (errors, check_exist, check_values, stats,
    run or None, new floor)."""
    state = dict(base)
    errors, exists, values, last = [], [], [], {}
    st = dict.fromkeys(STAT_FIELDS, 0)
    st["input_ops"] = len(ops)
    applied = 0
    for ck, ct, operand, muts, ret in ops:
        if is_malformed(ct, muts):
            errors.append(INVALID_ARGUMENT)
            exists.append(False)
            values.append(b"")
            st["malformed"] += 1
            continue
        old = state.get(ck)
        exist = old is not None and not 0 < old[1] <= epoch_now
        value = old[0] if exist else b""
        passed, invalid = validate_check(ct, operand, exist, value)
        exists.append(exist)
        values.append(value if ret and exist else b"")
        if not passed:
            errors.append(INVALID_ARGUMENT if invalid else TRY_AGAIN)
            st["failed_invalid" if invalid else "failed_check"] += 1
            continue
        errors.append(OK)
        st["passed"] += 1
        for m in muts:
            k, v, ets = m[:3]
            if v is None:
                state[k] = None
            else:
                if ets == 0 and default_ttl:
                    ets = (epoch_now + default_ttl) & 0xFFFFFFFF
                state[k] = (v, ets)
            last[k] = floor + applied
            applied += 1
    keys = sorted(last)
    vals = [b"" if state[k] is None else D.encode_value(state[k][0], state[k][1], 0, data_version)
            for k in keys]
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
            "sk": struct.pack("<%dQ" % len(keys),
                              *[(last[k] << 1) | (1 if state[k] is None else 0) for k in keys]),
        }
    st["mutations_applied"] = applied
    st["output_records"] = len(keys)
    st["removes"] = sum(1 for k in keys if state[k] is None)
    st["puts"] = len(keys) - st["removes"]
    st["key_bytes"], st["value_bytes"] = koff[-1], voff[-1]
    return errors, exists, values, st, run, floor + applied


def drive_sequence(reader, state, ops, epoch_now):
    """the contract's sequence through calls every backend has; see the module
    docstring for the two handles.  Returns (errors, check_exist, check_values)."""
    errors, exists, values = [], [], []
    assert state.flush() == OK
    for ck, ct, operand, muts, ret in ops:
        if is_malformed(ct, muts):
            errors.append(INVALID_ARGUMENT)
            exists.append(False)
            values.append(b"")
            continue
        err, val = reader.get(ck, epoch_now)
        exist = err == OK
        passed, invalid = validate_check(ct, operand, exist, val if exist else b"")
        exists.append(exist)
        values.append(val if ret and exist else b"")
        if not passed:
            errors.append(INVALID_ARGUMENT if invalid else TRY_AGAIN)
            continue
        for m in muts:
            hk, sk = D.restore_key(m[0])
            for p in (reader, state):
                if m[1] is None:
                    assert p.remove(hk, sk) == OK
                else:
                    assert p.put(hk, sk, m[1], m[2], epoch_now) == OK
        errors.append(OK)
    assert state.flush() == OK
    return errors, exists, values


def entries(ops):
    return sum(1 + len(o[3]) for o in ops)


# ---------------- the decision table ----------------
# validate_check by hand: one row per check type, one column per state of the
# check key; P = passes, F = kTryAgain, I = kInvalidArgument.

STATES = ("absent", "empty", "text", "integer", "non-integer", "expired", "tombstone")
STATE_VALUE = {"empty": b"", "text": b"hello", "integer": b"42", "non-integer": b"4x2"}
TABLE_OPERAND = {CT_ANYWHERE: b"x", CT_PREFIX: b"4", CT_POSTFIX: b"2"}  # 8..17: b"42", else b""
DECISIONS = [
    # absent empty text integer non-integer expired tombstone
    "PPPPPPP",  # 0 no check
    "PFFFFPP",  # 1 not exist
    "PPFFFPP",  # 2 not exist or empty
    "FPPPPFF",  # 3 exist
    "FFPPPFF",  # 4 not empty
    "FFFFPFF",  # 5 anywhere "x": only "4x2" holds one; "" is shorter than the operand
    "FFFPPFF",  # 6 prefix "4"
    "FFFPPFF",  # 7 postfix "2"
    "FPFFFFF",  # 8 bytes <  "42": "" is; "hello" and "4x2" are greater
    "FPFPFFF",  # 9 bytes <=
    "FFFPFFF",  # 10 bytes ==
    "FFPPPFF",  # 11 bytes >=
    "FFPFPFF",  # 12 bytes >
    "FIIFIFF",  # 13 int <  "42": "", "hello" and "4x2" are no integers
    "FIIPIFF",  # 14 int <=
    "FIIPIFF",  # 15 int ==
    "FIIPIFF",  # 16 int >=
    "FIIFIFF",  # 17 int >
]
# the stored value "42" against operands below, equal to and above it (hex 43),
# and one that is no integer: int <, <=, ==, >=, >
INT_ORDER = {b"41": "FFFPP", b" 42": "FPPPF", b"0x2B": "PPFFF", b"42 ": "IIIII", b"": "IIIII"}
VERDICT = {"P": OK, "F": TRY_AGAIN, "I": INVALID_ARGUMENT}


def table_operand(ct):
    return TABLE_OPERAND.get(ct, b"42" if ct >= CT_B_LT else b"")


def table_case():
    """the decision table as a batch: (layers, ops, expected errors), every
    cell on a hashkey of its own, the mutation on the check key"""
    run0, run1, ops, want = {}, {}, [], []
    for ct, row in enumerate(DECISIONS):
        for state, cell in zip(STATES, row):
            k = D.generate_key(b"t%02d-%s" % (ct, state.encode()), b"cell")
            if state in STATE_VALUE:
                run0[k] = (STATE_VALUE[state], 0)
            elif state == "expired":
                run0[k] = (b"42", NOW - 1)
            elif state == "tombstone":
                run0[k] = (b"42", 0)
                run1[k] = (None, 0)
            ops.append((k, ct, table_operand(ct), [(k, b"set", 0)], True))
            want.append(VERDICT[cell])
    for operand, row in INT_ORDER.items():
        for j, cell in enumerate(row):
            k = D.generate_key(b"io-%s-%d" % (operand.hex().encode(), j), b"cell")
            run0[k] = (b"42", 0)
            ops.append((k, CT_I_LT + j, operand, [(k, b"set", 0)], False))
            want.append(VERDICT[cell])
    return [run0, run1, {}], ops, want


# ---------------- the case lists ----------------
# a generator returns (layers, ops) with entries(ops) == E

def _build(rnd, E, make_op, max_muts):
    """ops from make_op(rnd, i, m) -> op with m mutations, until the entries
    add up to E exactly (never leaving a single entry over)"""
    ops, left = [], E
    while left:
        m = rnd.randrange(1, max_muts + 1)
        if left - 1 - m < 0:
            m = left - 1
        elif left - 1 - m == 1:
            m += 1
        op = make_op(rnd, len(ops), m)
        ops.append(op)
        left -= 1 + len(op[3])
        assert left != 1 and left >= 0
    return ops


def _puts(rnd, keys, m, i, expires=(0,)):
    return [(rnd.choice(keys), b"w%d.%d" % (i, j), rnd.choice(expires)) for j in range(m)]


RESIDENT = [None, b"", b"17", b"-5", b"0x1F", b"017", b"99999999999999999999", b"hello world",
            b"abcabc", b"17 ", b"A" * 100 + b"q" * 300 + b"Z"]
OPERANDS = [b"", b"17", b"0x11", b"abc", b"hello world and then some", b"q" * 300, b"zz", b"-5",
            b"hello", b"bc", b"1e3"]


def gen_all_types(E, seed):
    """distinct hashkeys, check types round-robin, every resident shape against
    every operand shape; check_and_set on the check key"""
    rnd = random.Random(seed)
    base = {}

    def make(rnd, i, m):
        hk = b"at%06d" % i
        ck = D.generate_key(hk, b"c")
        v = RESIDENT[(i // 18 + i) % len(RESIDENT)]
        if v is not None:
            base[ck] = (v, 0)
        operand = OPERANDS[(i // 7 + i) % len(OPERANDS)]
        return (ck, i % 18, operand, _puts(rnd, [ck], m, i), i % 3 == 0)

    ops = _build(rnd, E, make, 1)
    return [base, {}], ops


def gen_hot_hashkey(E, seed):
    """one hashkey, five sortkeys: the check on one, the mutations on others,
    so that a value set through B decides a later check on A and back"""
    rnd = random.Random(seed)
    keys = [D.generate_key(b"hot", s) for s in (b"a", b"b", b"c", b"d", b"e")]
    tokens = [b"t0", b"t1", b"t2"]

    def make(rnd, i, m):
        ck = rnd.choice(keys)
        ct, operand = rnd.choice(((CT_EXIST, b""), (CT_NOT_EXIST, b""), (CT_B_EQ, None),
                                  (CT_B_EQ, None), (CT_PREFIX, b"t")))
        if operand is None:
            operand = rnd.choice(tokens)
        others = [k for k in keys if k != ck]
        muts = [(rnd.choice(others), None if rnd.random() < 0.25 else rnd.choice(tokens), 0)
                for _ in range(m)]
        return (ck, ct, operand, muts, i % 2 == 0)

    return [{keys[0]: (b"t0", 0)}, {}], _build(rnd, E, make, 2)


def gen_lock(E, seed):
    """CT_VALUE_NOT_EXIST on a few lock keys over and over; an unconditional or
    an owner-checked DELETE in between releases them"""
    rnd = random.Random(seed)
    locks = [D.generate_key(b"lock%d" % j, b"owner") for j in range(3)]

    def make(rnd, i, m):
        k = rnd.choice(locks)
        r = rnd.random()
        if r < 0.2:
            return (k, CT_NO_CHECK, b"", [(k, None, 0)] * m, False)
        if r < 0.35:
            return (k, CT_B_EQ, b"owner%d" % rnd.randrange(max(0, i - 3), i + 1),
                    [(k, None, 0)] * m, True)
        return (k, CT_NOT_EXIST, b"", [(k, b"owner%d" % i, 0)] * m, True)

    return [{locks[1]: (b"owner0", 0)}, {}], _build(rnd, E, make, 1)


def gen_ttl(E, seed):
    """PUTs whose expire_ts is already past (a later check sees "not exist"),
    live TTLs, and resident records that have expired"""
    rnd = random.Random(seed)
    keys = [D.generate_key(b"ttl%d" % (j % 7), b"s%d" % (j // 7)) for j in range(21)]
    base = {k: (b"old%d" % j, (0, NOW - 5, NOW + 500)[j % 3]) for j, k in enumerate(keys[:12])}

    def make(rnd, i, m):
        ck = rnd.choice(keys)
        same_hk = [k for k in keys if D.restore_key(k)[0] == D.restore_key(ck)[0]]
        ct = rnd.choice((CT_EXIST, CT_EXIST, CT_NOT_EXIST, CT_NOT_EMPTY, CT_NO_CHECK))
        return (ck, ct, b"", _puts(rnd, same_hk, m, i, (0, 0, NOW - 5, NOW, NOW + 100, 1)),
                i % 2 == 1)

    return [base, {}], _build(rnd, E, make, 2)


def gen_layers(E, seed):
    """the newest version of a check key lies in one of three runs or in the
    pending memtable, with tombstones on top of older puts"""
    rnd = random.Random(seed)
    keys = [D.generate_key(b"ly%d" % (j % 11), b"s%d" % (j // 11)) for j in range(66)]
    r0, r1, r2, mem = {}, {}, {}, {}
    for j, k in enumerate(keys[:48]):
        r0[k] = (b"v0", 0)
        if j % 2:
            r1[k] = (b"v1", NOW + 900 if j % 3 == 0 else 0)
        if j % 4 == 1:
            r2[k] = (None, 0) if j % 8 == 1 else (b"v2", 0)
        if j % 8 == 3:
            mem[k] = (None, 0) if j % 16 == 3 else (b"v3", 0)

    def make(rnd, i, m):
        ck = rnd.choice(keys)
        ct, operand = rnd.choice(((CT_EXIST, b""), (CT_NOT_EXIST, b""),
                                  (CT_B_EQ, rnd.choice((b"v0", b"v1", b"v2", b"v3"))),
                                  (CT_B_GE, b"v1"), (CT_POSTFIX, b"1")))
        return (ck, ct, operand, [(ck, None if rnd.random() < 0.2 else b"n%d" % i, 0)] * m, True)

    return [r0, r1, r2, mem], _build(rnd, E, make, 1)


def gen_multi(E, seed):
    """lists of 1-6 mutations, puts and deletes, the same key twice in one
    list, on the check key and on other sortkeys"""
    rnd = random.Random(seed)
    n_hk = max(4, E // 40)

    def make(rnd, i, m):
        hk = b"mu%05d" % rnd.randrange(n_hk)
        keys = [D.generate_key(hk, b"s%d" % j) for j in range(4)]
        ck = keys[rnd.randrange(4)]
        ct = rnd.choice((CT_NO_CHECK, CT_EXIST, CT_NOT_EXIST, CT_NOT_EXIST, CT_NOT_EMPTY))
        muts = [(rnd.choice(keys), None if rnd.random() < 0.3 else b"m%d.%d" % (i, j) * (j + 1), 0)
                for j in range(m)]
        if m >= 2 and i % 3 == 0:
            muts[-1] = (muts[0][0], None if muts[0][1] is not None else b"again", 0)
        return (ck, ct, b"", muts, i % 4 == 0)

    return [{}], _build(rnd, E, make, 6)


def gen_malformed(E, seed):
    """empty lists, kinds that are neither PUT nor DELETE and check types
    outside 0..17, between good ops on the same keys"""
    rnd = random.Random(seed)
    n_hk = max(4, E // 30)
    ops, left, i = [], E, 0
    while left:
        hk = b"mf%05d" % rnd.randrange(n_hk)
        ck = D.generate_key(hk, b"s%d" % rnd.randrange(2))
        shape = i % 6 if left >= 4 else (5 if left != 1 else 0)
        if shape == 0:
            op = (ck, CT_NO_CHECK, b"", [], True)
        elif shape == 1:
            op = (ck, rnd.choice((-1, 18, 1000, -2**31)), b"", [(ck, b"never", 0)], True)
        elif shape == 2:
            op = (ck, CT_NO_CHECK, b"", [(ck, b"ok", 0, 0), (ck, b"bad kind", 0, 2)], True)
        else:
            op = (ck, rnd.choice((CT_NOT_EXIST, CT_EXIST, CT_NO_CHECK)), b"",
                  [(ck, None if rnd.random() < 0.3 else b"g%d" % i, 0)], True)
        ops.append(op)
        left -= 1 + len(op[3])
        i += 1
    return [{}], ops


def gen_int_invalid(E, seed):
    """int checks whose stored value or whose operand is no integer"""
    rnd = random.Random(seed)
    n_hk = max(4, E // 8)
    stored = [b"10", b"0x10", b"11", b"ten", b"-3", b"9223372036854775808", b"12", b""]
    base = {D.generate_key(b"ii%05d" % j, b"n"): (stored[j % len(stored)], 0)
            for j in range(n_hk)}

    def make(rnd, i, m):
        ck = D.generate_key(b"ii%05d" % rnd.randrange(n_hk), b"n")
        operand = rnd.choice((b"10", b"16", b"x", b" 11", b"11", b"-1", b"012", b"10"))
        return (ck, rnd.randrange(CT_I_LT, CT_I_GT + 1), operand,
                [(ck, rnd.choice((b"10", b"12", b"11", b"nan")), 0)] * m, True)

    return [base, {}], _build(rnd, E, make, 1)


def gen_all_fail(E, seed):
    """no check passes: CT_VALUE_EXIST on absent keys, CT_VALUE_NOT_EXIST on
    stored ones, an int check on text"""
    rnd = random.Random(seed)
    stored = {D.generate_key(b"af%04d" % j, b"s"): (b"text", 0) for j in range(50)}

    def make(rnd, i, m):
        if i % 3 == 0:
            k = D.generate_key(b"af-absent%d" % i, b"s")
            return (k, CT_EXIST, b"", _puts(rnd, [k], m, i), True)
        k = rnd.choice(sorted(stored))
        return (k, CT_NOT_EXIST if i % 3 == 1 else CT_I_EQ, b"7", _puts(rnd, [k], m, i), True)

    return [stored, {}], _build(rnd, E, make, 2)


def gen_empty_hashkey(E, seed):
    """hklen = 0: every key belongs to the one empty hashkey"""
    rnd = random.Random(seed)
    keys = [D.generate_key(b"", b"s%0*d" % (1 + j % 5, j)) for j in range(max(8, E // 6))]

    def make(rnd, i, m):
        ck = rnd.choice(keys)
        ct = rnd.choice((CT_NOT_EXIST, CT_EXIST, CT_NO_CHECK, CT_NOT_EXIST))
        return (ck, ct, b"", [(rnd.choice(keys), None if rnd.random() < 0.3 else b"e%d" % i, 0)
                              for _ in range(m)], i % 5 == 0)

    return [{keys[0]: (b"first", 0)}, {}], _build(rnd, E, make, 3)


# (name, generator, handle envs, epoch_now of the call)
CASES = [
    ("all-types", lambda E: gen_all_types(E, 111), {}, NOW),
    ("hot-hashkey", lambda E: gen_hot_hashkey(E, 112), {}, NOW),
    ("lock", lambda E: gen_lock(E, 113), {}, NOW),
    ("ttl", lambda E: gen_ttl(E, 114), {}, NOW),
    ("ttl-default-ttl", lambda E: gen_ttl(E, 115), {"default_ttl": "777"}, NOW),
    ("layers", lambda E: gen_layers(E, 116), {}, NOW),
    ("multi", lambda E: gen_multi(E, 117), {}, NOW),
    ("malformed", lambda E: gen_malformed(E, 118), {}, NOW),
    ("int-invalid", lambda E: gen_int_invalid(E, 119), {}, NOW),
    ("all-fail", lambda E: gen_all_fail(E, 120), {}, NOW),
    ("empty-hashkey", lambda E: gen_empty_hashkey(E, 121), {}, NOW),
    ("multi-data-version-0", lambda E: gen_multi(E, 122), {"pegasus.data_version": "0"}, NOW),
    ("ttl-data-version-0", lambda E: gen_ttl(E, 123), {"pegasus.data_version": "0"}, NOW),
    ("layers-data-version-2", lambda E: gen_layers(E, 124), {"pegasus.data_version": "2"}, NOW),
    ("ttl-data-version-2", lambda E: gen_ttl(E, 125),
     {"pegasus.data_version": "2", "default_ttl": "50"}, NOW),
]
CASE_PARAMS = [pytest.param(c, E, id="%s-%d" % (c[0], E)) for c in CASES for E in SIZES]


def model_of(case, E):
    """(layers, ops, floor-independent model results at floor 0)"""
    _, gen, envs, now = case
    layers, ops = gen(E)
    return layers, ops, cas_model(overlay(layers, env_ttl(envs), now), ops, 0, env_version(envs),
                                  env_ttl(envs), now)


# ---------------- CPU checks ----------------

def test_decision_table_by_hand():
    assert len(DECISIONS) == 18 and all(len(r) == len(STATES) for r in DECISIONS)
    for ct, row in enumerate(DECISIONS):
        for state, cell in zip(STATES, row):
            exist = state in STATE_VALUE
            passed, invalid = validate_check(ct, table_operand(ct), exist,
                                             STATE_VALUE.get(state, b""))
            got = "P" if passed else ("I" if invalid else "F")
            assert got == cell, (ct, state)
            assert not (passed and invalid)
    for operand, row in INT_ORDER.items():
        for j, cell in enumerate(row):
            passed, invalid = validate_check(CT_I_LT + j, operand, True, b"42")
            assert ("P" if passed else ("I" if invalid else "F")) == cell, (operand, j)
    # the rules the table's operands do not reach
    assert validate_check(CT_ANYWHERE, b"", True, b"") == (True, False)
    assert validate_check(CT_POSTFIX, b"abc", True, b"bc") == (False, False)
    assert validate_check(CT_ANYWHERE, b"q" * 300, True, b"A" + b"q" * 300 + b"Z") == (True, False)
    assert validate_check(CT_B_LT, b"ab\0", True, b"ab") == (True, False)
    assert validate_check(CT_B_GT, b"\x7f", True, b"\x80") == (True, False)  # unsigned bytes


def test_decision_table_through_the_model_and_the_oracle(oracle_lib):
    layers, ops, want = table_case()
    errors, exists, values, st, _, _ = cas_model(overlay(layers, 0, NOW), ops, 0, 1, 0, NOW)
    assert errors == want
    reader, _ = open_prepared(oracle_lib, -1, {}, layers, NOW)
    state, _ = open_prepared(oracle_lib, -1, {}, layers, NOW)
    try:
        assert drive_sequence(reader, state, ops, NOW) == (errors, exists, values)
    finally:
        reader.close()
        state.close()


@pytest.mark.parametrize("case,E", CASE_PARAMS)
def test_model_matches_oracle_sequence(oracle_lib, tmp_path, case, E):
    """cas_model == the contract's sequence on the oracle: per-op results, the
    run byte for byte and the floor"""
    _, gen, envs, now = case
    layers, ops = gen(E)
    assert entries(ops) == E
    reader, _ = open_prepared(oracle_lib, -1, envs, layers, now)
    state, floor = open_prepared(oracle_lib, -1, envs, layers, now)
    try:
        runs_before = state.num_runs() + (1 if layers[-1] else 0)
        got = drive_sequence(reader, state, ops, now)
        man, runs = read_checkpoint(state, tmp_path)
    finally:
        reader.close()
        state.close()
    errors, exists, values, st, run, new_floor = cas_model(
        overlay(layers, env_ttl(envs), now), ops, floor, env_version(envs), env_ttl(envs), now)
    assert (errors, exists, values) == got
    assert man["next_seq_floor"] == new_floor == floor + st["mutations_applied"]
    assert man["n_runs"] == runs_before + (1 if run else 0)
    if run:
        assert runs[-1] == run
    assert st["passed"] + st["failed_check"] + st["failed_invalid"] + st["malformed"] == len(ops)
    assert st["passed"] == errors.count(OK) and st["failed_check"] == errors.count(TRY_AGAIN)


@pytest.mark.parametrize("case,E", CASE_PARAMS)
def test_cases_do_not_degenerate(case, E):
    """in every case but all-fail at least a tenth of the ops pass and at least
    a tenth come back kTryAgain"""
    _, ops, (errors, exists, values, st, run, _) = model_of(case, E)
    n = len(ops)
    if case[0] == "all-fail":
        assert st["passed"] == 0 and run is None and st["failed_check"] and st["failed_invalid"]
        return
    assert 10 * st["passed"] >= n, st
    assert 10 * st["failed_check"] >= n, st


def test_cases_reach_what_they_are_for():
    by = {c[0]: c for c in CASES}
    E = SIZES[0]
    _, ops, (errors, exists, values, st, run, _) = model_of(by["malformed"], E)
    assert st["malformed"] * 3 >= len(ops) and st["mutations_applied"] == st["passed"]
    assert {o[1] for o in ops} & {-1, 18, 1000, -2**31} and any(not o[3] for o in ops)
    _, ops, (errors, _, _, st, _, _) = model_of(by["int-invalid"], E)
    assert st["failed_invalid"] * 5 >= len(ops)
    _, ops, (errors, exists, _, _, _, _) = model_of(by["ttl"], E)
    # a PUT of this batch that is already past, then a check that sees nothing
    stored, hit = {}, 0
    for (ck, _, _, muts, _), ex, er in zip(ops, exists, errors):
        if stored.get(ck) is not None and 0 < stored[ck] <= NOW:
            assert not ex
            hit += 1
        if er == OK:
            for k, v, ets in muts:
                stored[k] = ets if v is not None else None
    assert hit >= 5
    _, ops, (_, _, values, st, _, _) = model_of(by["multi"], E)
    assert max(len(o[3]) for o in ops) == 6 and st["removes"] and st["puts"]
    assert any(len({m[0] for m in o[3]}) < len(o[3]) for o in ops)
    _, ops, (_, _, values, _, _, _) = model_of(by["all-types"], E)
    assert {o[1] for o in ops} == set(range(18)) and any(len(v) > 300 for v in values)
    _, ops, _ = model_of(by["hot-hashkey"], E)
    assert len({D.restore_key(o[0])[0] for o in ops}) == 1
    assert all(m[0] != o[0] for o in ops for m in o[3])
    _, ops, _ = model_of(by["empty-hashkey"], E)
    assert all(o[0][:2] == b"\0\0" for o in ops)


def test_binding_raises_without_the_symbol(oracle_lib):
    """the oracle does not export rrdb_check_and_mutate_batch: the binding
    says so and does not fall back to get + put"""
    assert oracle_lib.has_check_and_mutate_batch is False
    o = oracle_lib.open(1, 0, -1)
    try:
        assert o.put(b"h", b"s", b"5", 0, 0) == OK
        k = D.generate_key(b"h", b"s")
        with pytest.raises(RuntimeError, match="rrdb_check_and_mutate_batch"):
            o.check_and_mutate_batch([(k, CT_EXIST, b"", [(k, b"6", 0)], True)])
        with pytest.raises(RuntimeError, match="rrdb_check_and_mutate_batch"):
            o.check_and_set_batch([(k, CT_EXIST, b"", k, b"6", 0, True)])
        assert o.num_runs() == 0 and o.memtable_entries() == 1
    finally:
        o.close()


def test_check_program():
    """tools/cas_check_check.cpp (cas_check.h against a std::string
    restatement, cas_stage.h over valid and malformed batches), as built by
    __graft_entry__.build()"""
    exe = os.path.join(REPO, "bin", "cas_check_check")
    if not os.path.exists(exe):
        pytest.skip("bin/cas_check_check not built (run __graft_entry__.build())")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "cas_check_check OK" in r.stdout, r.stderr


# ---------------- the two that fail before the change ----------------

def test_header_declares_check_and_mutate_batch():
    src = open(os.path.join(REPO, "include", "rrdb_engine_ext.h")).read()
    assert re.search(r"\bint32_t\s+rrdb_check_and_mutate_batch\s*\(", src)
    assert re.search(r"\}\s*rrdb_cas_batch_stats\s*;", src)
    assert re.search(r"\bRRDB_TRY_AGAIN\s*=\s*13\b", src)
    for f in STAT_FIELDS:
        assert re.search(r"\buint64_t\b[^;]*\b%s\b" % f, src), f


def test_hip_lib_exports_check_and_mutate_batch():
    if not os.path.exists(HIP_SO):
        pytest.skip("librrdb_hip.so not built (run __graft_entry__.build())")
    assert hasattr(ctypes.CDLL(HIP_SO), "rrdb_check_and_mutate_batch")
