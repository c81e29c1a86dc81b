"""Compaction-filter rule/op decision tables lifted from the reference tests:
  - src/server/test/compaction_filter_rule_test.cpp:32-135
    (hashkey/sortkey pattern matrices, ttl_range matrix)
  - src/server/test/compaction_operation_test.cpp:250-287 (ops JSON format)
Exercised through the oracle's pattern hook AND end-to-end through
rrdb_set_envs("user_specified_compaction") + rrdb_manual_compact.  The tables
and builders live in tests/rule_tables.py, shared with the device run of the
same rows (tests/test_rule_tables_gpu.py)."""
import ctypes
import json

from conftest import ORACLE_SO
from rule_tables import PATTERN_CASES, TTL_RANGE_CASES
from rule_tables import mk_rule as _mk_rule
from rule_tables import one_key_compact as _one_key_compact
from rule_tables import ops_json as _ops_json


def test_pattern_match_table():
    lib = ctypes.CDLL(ORACLE_SO)
    lib.orc_pattern_match.restype = ctypes.c_int
    lib.orc_pattern_match.argtypes = [
        ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64]
    for value, pat, mt, want in PATTERN_CASES:
        got = lib.orc_pattern_match(value, len(value), mt, pat, len(pat))
        assert bool(got) == want, (value, pat, mt)


def test_ttl_range_rule_matrix(oracle_lib):
    """ttl_range_rule::match (compaction_filter_rule.cpp:74-90) through a
    delete op — record dropped iff rule matches."""
    now = 1000000
    for start_ttl, stop_ttl, expire_ttl, want_match in TTL_RANGE_CASES:
        ops = _ops_json([("COT_DELETE", "",
                          [_mk_rule("FRT_TTL_RANGE",
                                    {"start_ttl": start_ttl, "stop_ttl": stop_ttl})])])
        expire = (expire_ttl + now) if expire_ttl else 0
        survived, _ = _one_key_compact(oracle_lib, ops, expire, now)
        assert survived == (not want_match), (start_ttl, stop_ttl, expire_ttl)


def test_delete_op_pattern_rules(oracle_lib):
    """delete_key::filter (compaction_operation.cpp:57-68): drops iff ALL rules match."""
    ops = _ops_json([("COT_DELETE", "", [
        _mk_rule("FRT_HASHKEY_PATTERN", {"pattern": "hash", "match_type": "SMT_MATCH_PREFIX"}),
        _mk_rule("FRT_SORTKEY_PATTERN", {"pattern": "key", "match_type": "SMT_MATCH_POSTFIX"}),
    ])])
    assert _one_key_compact(oracle_lib, ops, 0, 100)[0] is False  # both match -> dropped
    # second rule fails -> kept
    ops2 = _ops_json([("COT_DELETE", "", [
        _mk_rule("FRT_HASHKEY_PATTERN", {"pattern": "hash", "match_type": "SMT_MATCH_PREFIX"}),
        _mk_rule("FRT_SORTKEY_PATTERN", {"pattern": "nope", "match_type": "SMT_MATCH_POSTFIX"}),
    ])])
    assert _one_key_compact(oracle_lib, ops2, 0, 100)[0] is True


def test_update_ttl_ops(oracle_lib):
    """update_ttl::filter (compaction_operation.cpp:78-113)."""
    now = 500000
    rule = [_mk_rule("FRT_HASHKEY_PATTERN", {"pattern": "hash", "match_type": "SMT_MATCH_PREFIX"})]
    # UTOT_FROM_NOW: new expire = now + value
    ops = _ops_json([("COT_UPDATE_TTL", {"type": "UTOT_FROM_NOW", "value": 1234}, rule)])
    survived, new_expire = _one_key_compact(oracle_lib, ops, 0, now)
    assert survived and new_expire == now + 1234
    # UTOT_FROM_CURRENT on a no-ttl record: no-op
    ops = _ops_json([("COT_UPDATE_TTL", {"type": "UTOT_FROM_CURRENT", "value": 100}, rule)])
    survived, new_expire = _one_key_compact(oracle_lib, ops, 0, now)
    assert survived and new_expire is None
    # UTOT_FROM_CURRENT with existing ttl
    ops = _ops_json([("COT_UPDATE_TTL", {"type": "UTOT_FROM_CURRENT", "value": 100}, rule)])
    survived, new_expire = _one_key_compact(oracle_lib, ops, now + 50, now)
    assert survived and new_expire == now + 150
    # UTOT_TIMESTAMP: expire = value - epoch_begin(1451606400)
    ts = 1451606400 + 777777
    ops = _ops_json([("COT_UPDATE_TTL", {"type": "UTOT_TIMESTAMP", "value": ts}, rule)])
    survived, new_expire = _one_key_compact(oracle_lib, ops, 0, now)
    assert survived and new_expire == 777777


def test_default_ttl_rewrite(oracle_lib):
    """Filter:73-79: default_ttl applied to expire_ts==0 records during compaction."""
    now = 300000
    survived, new_expire = _one_key_compact(oracle_lib, None, 0, now,
                                            envs={"default_ttl": "5000"})
    assert survived and new_expire == now + 5000
    # record with own ttl is untouched
    survived, new_expire = _one_key_compact(oracle_lib, None, now + 99, now,
                                            envs={"default_ttl": "5000"})
    assert survived and new_expire == now + 99


def test_invalid_ops_json_means_no_ops(oracle_lib):
    """create_compaction_operations: bad json -> empty ops (cpp:165-169);
    ops with zero valid rules are skipped (:176-179)."""
    now = 1000
    # bad json: record survives
    assert _one_key_compact(oracle_lib, "not json at all", 0, now)[0] is True
    # delete op with only an invalid-typed rule: skipped -> survives
    ops = json.dumps({"ops": [{"type": "COT_DELETE", "params": "",
                               "rules": [{"type": "FRT_BOGUS", "params": "{}"}]}]})
    assert _one_key_compact(oracle_lib, ops, 0, now)[0] is True
    # rule params missing a required field -> rule invalid -> op skipped
    ops = json.dumps({"ops": [{"type": "COT_DELETE", "params": "", "rules": [
        {"type": "FRT_HASHKEY_PATTERN", "params": json.dumps({"pattern_xxx": "h", "match_type": "SMT_MATCH_PREFIX"})}]}]})
    assert _one_key_compact(oracle_lib, ops, 0, now)[0] is True


def test_op_order_first_delete_wins(oracle_lib):
    """ops applied in order; a matching delete drops immediately
    (key_ttl_compaction_filter.h:101-107)."""
    rule = [_mk_rule("FRT_HASHKEY_PATTERN", {"pattern": "hash", "match_type": "SMT_MATCH_PREFIX"})]
    ops = _ops_json([
        ("COT_DELETE", "", rule),
        ("COT_UPDATE_TTL", {"type": "UTOT_FROM_NOW", "value": 55}, rule),
    ])
    assert _one_key_compact(oracle_lib, ops, 0, 100)[0] is False
