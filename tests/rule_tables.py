"""Shared data for the compaction-filter rule tests: the decision tables
lifted from the reference's tests, the ops-JSON builders, the one-record
compaction they are run through, and the small multi-run layouts and rule sets
of the route matrix (tests/test_rule_tables_gpu.py).

Table sources:
  - src/server/test/compaction_filter_rule_test.cpp:32-135
    (hashkey/sortkey pattern matrices, ttl_range matrix)
  - src/server/test/compaction_operation_test.cpp:250-287 (ops JSON format)
"""
import json
import random
from collections import namedtuple

from incubator_pegasus_amd import data as D
from pymodel import Model, expire_of

SMT_ANYWHERE, SMT_PREFIX, SMT_POSTFIX, SMT_INVALID = 0, 1, 2, 3
SMT_NAMES = {SMT_ANYWHERE: "SMT_MATCH_ANYWHERE", SMT_PREFIX: "SMT_MATCH_PREFIX",
             SMT_POSTFIX: "SMT_MATCH_POSTFIX", SMT_INVALID: "SMT_INVALID"}

# compaction_filter_rule_test.cpp:40-57 (hashkey table; sortkey table is the
# same matrix over the sortkey, :75-92)
PATTERN_CASES = [
    (b"sortkey", b"", SMT_ANYWHERE, False),
    (b"hashkey", b"hashkey", SMT_ANYWHERE, True),
    (b"hashkey", b"shke", SMT_ANYWHERE, True),
    (b"hashkey", b"hash", SMT_ANYWHERE, True),
    (b"hashkey", b"key", SMT_ANYWHERE, True),
    (b"hashkey", b"sortkey", SMT_ANYWHERE, False),
    (b"hashkey", b"hashkey", SMT_PREFIX, True),
    (b"hashkey", b"hash", SMT_PREFIX, True),
    (b"hashkey", b"key", SMT_PREFIX, False),
    (b"hashkey", b"sortkey", SMT_PREFIX, False),
    (b"hashkey", b"hashkey", SMT_POSTFIX, True),
    (b"hashkey", b"hash", SMT_POSTFIX, False),
    (b"hashkey", b"key", SMT_POSTFIX, True),
    (b"hashkey", b"sortkey", SMT_POSTFIX, False),
    (b"hash", b"hashkey", SMT_POSTFIX, False),
    (b"hashkey", b"hashkey", SMT_INVALID, False),
]

# compaction_filter_rule_test.cpp:105-125: (start_ttl, stop_ttl, expire_ttl, match)
TTL_RANGE_CASES = [
    (100, 1000, 1100, False),
    (100, 1000, 500, True),
    (100, 1000, 20, False),
    (100, 1000, 0, False),
    (1000, 100, 1100, False),
    (1000, 100, 500, False),
    (1000, 100, 20, False),
    (1000, 100, 0, False),
    (0, 1000, 500, True),
    (1000, 0, 500, False),
    (0, 0, 0, True),
]


def mk_rule(rtype, params):
    return {"type": rtype, "params": json.dumps(params)}


def ops_json(ops):
    return json.dumps({"ops": [
        {"type": t, "params": json.dumps(p) if isinstance(p, dict) else p,
         "rules": rules} for t, p, rules in ops]})


def pattern_rule(part, pattern: bytes, match_type: int):
    """part: "hashkey" | "sortkey".  Pattern bytes travel as latin-1 text, so
    json.dumps writes every byte >= 0x80 as a \\u00XX escape."""
    return mk_rule("FRT_%s_PATTERN" % part.upper(),
                   {"pattern": pattern.decode("latin-1"), "match_type": SMT_NAMES[match_type]})


def ttl_rule(start_ttl, stop_ttl):
    return mk_rule("FRT_TTL_RANGE", {"start_ttl": start_ttl, "stop_ttl": stop_ttl})


def open_part(lib):
    """a fresh handle of either backend (the oracle takes no GPU)"""
    return lib.open(1, 0, -1 if lib.backend == "oracle-cpu" else 0)


def one_key_compact(lib, ops_json_text, value_expire, now, hash_key=b"hashkey",
                    sort_key=b"sortkey", envs=None, version=1):
    """Ingest a single record and compact; returns (survived, new_expire_ts)."""
    p = open_part(lib)
    try:
        if envs:
            p.set_envs(envs)
        if ops_json_text is not None:
            p.set_envs({"user_specified_compaction": ops_json_text})
        raw_key = D.generate_key(hash_key, sort_key)
        val = D.encode_value(b"payload", value_expire, 0, version)
        p.ingest_run([(raw_key, val, 10, 0)])
        err, stats = p.manual_compact(now)
        assert err == 0
        if stats.output_records == 0:
            return False, None
        st, got = p.get(raw_key, 0)  # epoch 0: nothing TTL-hidden at read time
        assert st == 0 and got == b"payload"
        st, ttl = p.ttl(raw_key, 0)
        # recover expire via ttl(+0): ttl == expire - 0 when expire>0 else -1
        return True, (None if ttl == -1 else ttl)
    finally:
        p.close()


# ---------------- ops JSON -> pymodel ops ----------------

_FRT = {"FRT_HASHKEY_PATTERN": "hashkey", "FRT_SORTKEY_PATTERN": "sortkey",
        "FRT_TTL_RANGE": "ttl_range"}
_SMT = {"SMT_MATCH_ANYWHERE": "anywhere", "SMT_MATCH_PREFIX": "prefix",
        "SMT_MATCH_POSTFIX": "postfix"}
_UTOT = {"UTOT_FROM_NOW": "from_now", "UTOT_FROM_CURRENT": "from_current",
         "UTOT_TIMESTAMP": "timestamp"}


def _is_int(x):
    return isinstance(x, int) and not isinstance(x, bool)


def model_ops(text):
    """create_compaction_operations (compaction_operation.cpp:162-186) for
    tests/pymodel.py: text that does not decode gives no ops; a rule of unknown
    type or whose params lack a field is skipped; an op without a valid rule,
    of unknown type, or (update_ttl) whose params lack type or value is
    skipped; an unknown UTOT type stays as an op that never applies."""
    try:
        root = json.loads(text)
    except ValueError:
        return []
    if not isinstance(root, dict) or not isinstance(root.get("ops"), list):
        return []
    out = []
    for jop in root["ops"]:
        if not isinstance(jop, dict):
            return []
        params = jop.get("params", "")
        if not isinstance(jop.get("type"), str) or not isinstance(params, str) \
                or not isinstance(jop.get("rules"), list):
            continue
        rules = []
        for jr in jop["rules"]:
            if not isinstance(jr, dict) or jr.get("type") not in _FRT \
                    or not isinstance(jr.get("params"), str):
                continue
            try:
                rp = json.loads(jr["params"])
            except ValueError:
                continue
            if not isinstance(rp, dict):
                continue
            kind = _FRT[jr["type"]]
            if kind == "ttl_range":
                if not _is_int(rp.get("start_ttl")) or not _is_int(rp.get("stop_ttl")):
                    continue
                rules.append(dict(type=kind, start_ttl=rp["start_ttl"], stop_ttl=rp["stop_ttl"]))
            else:
                if not isinstance(rp.get("pattern"), str) \
                        or not isinstance(rp.get("match_type"), str):
                    continue
                rules.append(dict(type=kind, pattern=rp["pattern"].encode("latin-1"),
                                  match_type=_SMT.get(rp["match_type"], "invalid")))
        if not rules:
            continue
        if jop["type"] == "COT_DELETE":
            out.append(dict(type="delete", rules=rules))
        elif jop["type"] == "COT_UPDATE_TTL":
            try:
                op = json.loads(params)
            except ValueError:
                continue
            if not isinstance(op, dict) or not isinstance(op.get("type"), str) \
                    or not _is_int(op.get("value")):
                continue
            out.append(dict(type="update_ttl", ut_type=_UTOT.get(op["type"], "invalid"),
                            value=op["value"], rules=rules))
    return out


# ---------------- layouts ----------------

NOW = 1_000_000
EPOCH_BEGIN = 1451606400  # pegasus::utils::epoch_begin, 2016-01-01 GMT
# the ttl_range rules below span [NOW + TTL_LO, NOW + TTL_HI]; the expire
# classes: none, already expired, on each bound exactly, inside, beyond
TTL_LO, TTL_HI = 100, 1000
EXPIRES = (0, 0, 0, NOW - 50, NOW + TTL_LO, NOW + TTL_HI, NOW + 500, NOW + 5000)

# Pattern vocabulary of a layout: (hashkey pattern, sortkey pattern) per role.
#   whole: equals one whole key part;  last: occurs in a key part only at its
#   last possible offset;  long: one byte longer than the longest key part,
#   made of bytes that do sit there in memory (the hashkey's over-long PREFIX
#   ends in the first sortkey byte, the sortkey's over-long POSTFIX starts
#   with the last hashkey byte), so an evaluator that forgets the length
#   check finds them.
Vocab = namedtuple("Vocab", "prefix postfix anywhere whole last long")
Layout = namedtuple("Layout", "name hashkeys sortkeys body vocab per_run")

_WORD_HK = [b"hkwxyz" + t for t in (b"ab07", b"ab19", b"abQ9", b"cd07", b"cdQ9", b"Q9cd",
                                   b"xaab", b"xa07", b"zzzz", b"07ab", b"a.b0", b"cdab")]
_WORD_SK = [b"s001", b"s002", b"s0Q9", b"t001", b"tQ9t", b"Q9s0", b"key1", b"1key", b"skey",
            b"zzzz"]
_WORD_VOCAB = Vocab(prefix=(b"hkwxyzab", b"s0"), postfix=(b"07", b"key"),
                    anywhere=(b"zcd", b"Q9"), whole=(b"hkwxyzab07", b"t001"),
                    last=(b"bQ9", b"0Q9"), long=(b"hkwxyzab07s", b"7s001"))

_VAR_HK = [b"h", b"hk", b"hash", b"hashkey", b"hashkeyQ9", b"xQ9hash", b"keyhash",
           b"a-much-longer-hashkey-07", b"sort", b"yek"]
_VAR_SK = [b"", b"s", b"sk", b"sort", b"sortkey", b"keysort", b"sortQ9", b"Q9sort",
           b"a-long-sortkey-0001", b"key", b"hash", b"xsortkeyx"]
_VAR_VOCAB = Vocab(prefix=(b"hash", b"sort"), postfix=(b"hash", b"sort"),
                   anywhere=(b"shke", b"ortk"), whole=(b"hashkey", b"sortkey"),
                   last=(b"yQ9", b"tQ9"),
                   long=(b"a-much-longer-hashkey-07s", b"ha-long-sortkey-0001"))

LAYOUTS = {
    # 16-byte keys: 2 length bytes + 10-byte hashkey + 4-byte sortkey.  The
    # shared first 8 bytes end inside the hashkey, so hashkey tail and sortkey
    # both vary in the tail word; every PUT value is 24 bytes.
    "word": Layout("word", _WORD_HK, _WORD_SK, lambda i, seq: b"r%011d" % seq, _WORD_VOCAB, 100),
    # the same keys with values of several lengths: tail-word rank, per-row emit
    "wordvar": Layout("wordvar", _WORD_HK, _WORD_SK, lambda i, seq: b"v" * (i % 5) + b"%d" % seq,
                      _WORD_VOCAB, 100),
    # hashkeys, sortkeys (one empty, one shorter than every pattern) and
    # values of several lengths
    "var": Layout("var", _VAR_HK, _VAR_SK, lambda i, seq: b"v" * (i % 7 * 3) + b"%d" % seq,
                  _VAR_VOCAB, 90),
}
N_RUNS = 3
P_TOMBSTONE = 0.06


def build_runs(layout_name, version=1):
    """N_RUNS overlapping sorted runs [(raw_key, raw_value, seq, kind)] drawn
    from the layout's hashkey x sortkey universe: keys recur across runs
    (shadowing), a few records are tombstones, expires come from EXPIRES."""
    lay = LAYOUTS[layout_name]
    rnd = random.Random("rule-tables-" + lay.name.replace("wordvar", "word"))
    universe = [(hk, sk) for hk in lay.hashkeys for sk in lay.sortkeys]
    runs, seq = [], 1
    for _ in range(N_RUNS):
        recs = []
        for i in sorted(rnd.sample(range(len(universe)), lay.per_run)):
            key = D.generate_key(*universe[i])
            ets = rnd.choice(EXPIRES)
            if rnd.random() < P_TOMBSTONE:
                recs.append((key, b"", seq, 1))
            else:
                recs.append((key, D.encode_value(lay.body(i, seq), ets, 0, version), seq, 0))
            seq += 1
        recs.sort()
        runs.append(recs)
    return runs


# ---------------- rule sets ----------------

# none: by construction no live record matches;  rewrite: the set rewrites
# expire headers of surviving records
RuleSet = namedtuple("RuleSet", "name ops default_ttl none rewrite")


def rule_sets(layout_name):
    """One user_specified_compaction value each (None = no ops), some with a
    default_ttl.  The patterns come from the layout's vocabulary."""
    v = LAYOUTS[layout_name].vocab
    HK, SK = 0, 1

    def rule(part, role, mt):
        return pattern_rule(("hashkey", "sortkey")[part], getattr(v, role)[part], mt)

    def delete(*rules):
        return ("COT_DELETE", "", list(rules))

    def update(ut_type, value, *rules):
        return ("COT_UPDATE_TTL", {"type": ut_type, "value": value}, list(rules))

    hk_pre = rule(HK, "prefix", SMT_PREFIX)
    sk_pre = rule(SK, "prefix", SMT_PREFIX)
    window = ttl_rule(TTL_LO, TTL_HI)
    sets = []

    def add(name, ops, default_ttl=0, none=False, rewrite=False):
        sets.append(RuleSet(name, ops_json(ops) if ops is not None else None, default_ttl,
                            none, rewrite))

    # each match type on each key part
    add("hk_prefix", [delete(hk_pre)])
    add("hk_postfix", [delete(rule(HK, "postfix", SMT_POSTFIX))])
    add("hk_anywhere", [delete(rule(HK, "anywhere", SMT_ANYWHERE))])
    add("sk_prefix", [delete(sk_pre)])
    add("sk_postfix", [delete(rule(SK, "postfix", SMT_POSTFIX))])
    add("sk_anywhere", [delete(rule(SK, "anywhere", SMT_ANYWHERE))])
    # a pattern equal to the whole key part, under every match type
    add("hk_whole_postfix", [delete(rule(HK, "whole", SMT_POSTFIX))])
    add("hk_whole_anywhere", [delete(rule(HK, "whole", SMT_ANYWHERE))])
    add("sk_whole_prefix", [delete(rule(SK, "whole", SMT_PREFIX))])
    add("sk_whole_postfix", [delete(rule(SK, "whole", SMT_POSTFIX))])
    # one byte longer than the longest key part
    add("hk_long_prefix", [delete(rule(HK, "long", SMT_PREFIX))], none=True)
    add("hk_long_anywhere", [delete(rule(HK, "long", SMT_ANYWHERE))], none=True)
    add("sk_long_postfix", [delete(rule(SK, "long", SMT_POSTFIX))], none=True)
    # the empty pattern matches nothing, whatever the match type
    add("hk_empty_anywhere", [delete(pattern_rule("hashkey", b"", SMT_ANYWHERE))], none=True)
    add("sk_empty_prefix", [delete(pattern_rule("sortkey", b"", SMT_PREFIX))], none=True)
    add("sk_empty_postfix", [delete(pattern_rule("sortkey", b"", SMT_POSTFIX))], none=True)
    # ANYWHERE that matches only at the last possible offset
    add("hk_anywhere_last", [delete(rule(HK, "last", SMT_ANYWHERE))])
    add("sk_anywhere_last", [delete(rule(SK, "last", SMT_ANYWHERE))])
    # ttl_range: the window, each bound on a record's expire exactly, start >
    # stop, the "no TTL" rule, and a stop whose 32-bit sum with now wraps
    add("ttl_window", [delete(window)])
    add("ttl_lower_bound_exact", [delete(ttl_rule(TTL_LO, TTL_LO))])
    add("ttl_upper_bound_exact", [delete(ttl_rule(TTL_HI, TTL_HI))])
    add("ttl_start_gt_stop", [delete(ttl_rule(TTL_HI, TTL_LO))], none=True)
    add("ttl_zero_zero", [delete(ttl_rule(0, 0))])
    add("ttl_stop_wraps", [delete(ttl_rule(TTL_LO, 0xFFFFFFFF))], none=True)
    # with default_ttl the rule sees the post-default expire: NOW + 500 is in
    # the window, so the records without a TTL go too
    add("ttl_window_default_ttl", [delete(window)], default_ttl=500)
    # all rules of an op must match
    add("two_rule_delete", [delete(hk_pre, sk_pre)])
    add("pattern_and_ttl_delete", [delete(rule(SK, "anywhere", SMT_ANYWHERE), window)])
    # update_ttl flavours
    add("default_ttl_only", None, default_ttl=700, rewrite=True)
    add("from_now", [update("UTOT_FROM_NOW", 1234, hk_pre)], rewrite=True)
    add("from_now_default_ttl", [update("UTOT_FROM_NOW", 1234, sk_pre)], default_ttl=700,
        rewrite=True)
    add("from_current", [update("UTOT_FROM_CURRENT", 77, hk_pre)], rewrite=True)
    add("from_current_default_ttl", [update("UTOT_FROM_CURRENT", 77, sk_pre)], default_ttl=700,
        rewrite=True)
    add("timestamp_future", [update("UTOT_TIMESTAMP", EPOCH_BEGIN + NOW + 7777, sk_pre)],
        rewrite=True)
    # lands in the past: the record is kept this pass, with the past timestamp
    add("timestamp_past", [update("UTOT_TIMESTAMP", EPOCH_BEGIN + NOW - 100, hk_pre)],
        rewrite=True)
    # the second op sees the expire as of loop entry, not the first's rewrite
    add("two_updates", [update("UTOT_FROM_NOW", 300, hk_pre),
                        update("UTOT_FROM_CURRENT", 50, hk_pre)], rewrite=True)
    # the delete's ttl_range sees the loop-entry expire as well
    add("delete_after_update", [update("UTOT_FROM_NOW", 300, hk_pre), delete(window),
                                delete(sk_pre)], rewrite=True)
    add("update_after_delete", [delete(sk_pre), update("UTOT_FROM_NOW", 300, hk_pre)],
        rewrite=True)
    return sets


REWRITING = [rs.name for rs in rule_sets("word") if rs.rewrite]


def make_model(layout_name, rs, version=1):
    m = Model(data_version=version)
    for run in build_runs(layout_name, version):
        m.ingest(run)
    m.default_ttl = rs.default_ttl
    m.user_ops = model_ops(rs.ops) if rs.ops is not None else []
    return m


def set_rule_envs(part, rs, version=1):
    """before any ingest: the data version decides the value header layout"""
    envs = {}
    if version != 1:
        envs["pegasus.data_version"] = str(version)
    if rs.default_ttl:
        envs["default_ttl"] = str(rs.default_ttl)
    if rs.ops is not None:
        envs["user_specified_compaction"] = rs.ops
    if envs:
        part.set_envs(envs)


def model_rows(surviving, version=1):
    """Model.compact_full's survivors as a full drain with return_expire_ts
    reports them: [(key, user data, expire_ts as int32)]"""
    hdr = D.value_header_len(version)
    rows = []
    for k in sorted(surviving):
        v = surviving[k][0]
        e = expire_of(v, version)
        rows.append((k, v[hdr:], e - (1 << 32) if e >= (1 << 31) else e))
    return rows
