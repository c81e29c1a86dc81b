"""A run holds the same thing whichever route built it.

The engine creates a run in five places ("run creation"):
  (a) ingest_run,
  (b) puts and removes followed by flush,
  (c) restore of a checkpoint,
  (d) a compaction's output: compact_runs(1, 1), the non-bottommost rewrite
      of one run, with an older one-record run below it,
  (e) a split's output: the side of a 2-way split that received the records,
      out of a parent run that also held the other side's.
For every shape below the same records go into an engine handle by each
route.  Each handle is compared with a CPU-oracle handle that plainly ingested
the records the route must have produced: run and record counts and every
read, then the full stats of a manual_compact and every read again.

The shapes are the sizes at which run creation can go wrong: one record (first
key == last key), two, a wave tile plus one, fixed-stride keys with and
without a shared prefix up to the last 8 bytes (tail words built / not built),
keys shorter than 8 bytes, variable strides, tombstones only (no PUT stride),
PUTs of one length mixed with tombstones (a PUT stride but no plain stride).
No record carries a TTL, so the non-bottommost pass of (d) converts nothing.
"""
import shutil
import tempfile

import pytest

from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import OK
from test_minor_compact_model import stats_dict
from test_split_gpu import _open, _same_reads
from test_split_model import NOW, key_hash

pytestmark = pytest.mark.gpu


# ---------------- shapes ----------------
# A shape is a list of rows (hashkey slot, hashkey length, sortkey, body);
# body None = tombstone.  Slots become real hashkeys per split side, so the
# same shape exists once with every key owned by partition 0 of 2 and once
# with every key owned by partition 1.

def _fixed(n, body=b"v" * 20, dead=lambda i: False):
    """16-byte keys under one 6-byte hashkey: all share the first 8 bytes"""
    return [(0, 6, b"s%07d" % i, None if dead(i) else body) for i in range(n)]


SHAPES = {
    "n1": _fixed(1),
    "n2": _fixed(2),
    "n65": _fixed(65),
    # first and last key differ only in the final 8 bytes: tail words
    "tails": _fixed(200),
    # 266-byte keys; hashkey lengths 1 and 256 put 0x00 / 0x01 into byte 0
    "no_tails": [(0, 1, b"t%0262d" % i, b"w" * 9) for i in range(40)] +
                [(1, 256, b"s%07d" % i, b"w" * 9) for i in range(40)],
    # 6-byte keys
    "short": [(0, 1, b"%03d" % i, b"x" * 5) for i in range(100)],
    "var": [(i % 7, 1 + i % 7 * 3, b"k%0*d" % (1 + i % 5, i), b"y" * (i % 13))
            for i in range(150)],
    "tombstones": _fixed(70, dead=lambda i: True),
    "puts_and_tombstones": _fixed(130, dead=lambda i: i % 3 == 1),
}


def _hashkeys(rows, side):
    """slot -> a hashkey of the slot's length owned by partition `side` of 2"""
    out, used = {}, set()
    for slot, hl, _, _ in rows:
        if slot in out:
            continue
        for j in range(100_000):
            hk = (b"%d" % j * hl)[:hl]
            if hk not in used and key_hash(D.generate_key(hk, b"")) & 1 == side:
                break
        else:
            raise AssertionError("no hashkey of length %d for side %d" % (hl, side))
        used.add(hk)
        out[slot] = hk
    return out


def records(rows, side, first_seq=1):
    """sorted [(key, encoded value, seq, kind)], seq = first_seq + position"""
    hks = _hashkeys(rows, side)
    kv = sorted((D.generate_key(hks[slot], sk), body) for slot, _, sk, body in rows)
    assert len({k for k, _ in kv}) == len(rows)
    return [(k, b"" if body is None else D.encode_value(body, 0, 0, 1), first_seq + i,
             int(body is None)) for i, (k, body) in enumerate(kv)]


def extra_record(recs):
    """an older record of a key that is not in recs: same hashkey and length
    as recs' first key, so a fixed-stride shape stays fixed-stride with it"""
    hk, sk = D.restore_key(recs[0][0])
    key = D.generate_key(hk, b"!" * len(sk))
    assert key not in {r[0] for r in recs}
    return (key, D.encode_value(b"old", 0, 0, 1), 0, 0)


def test_shapes_are_what_they_claim():
    """no GPU work: the properties the shapes are chosen for"""
    def strides(name, side=0):
        recs = records(SHAPES[name], side)
        keys = [r[0] for r in recs]
        return recs, keys, {len(k) for k in keys}, {len(r[1]) for r in recs}

    for name in ("n1", "n2", "n65", "tails"):
        recs, keys, kl, vl = strides(name)
        assert kl == {16} and vl == {32} and keys[0][:8] == keys[-1][:8]
    assert [len(SHAPES[n]) for n in ("n1", "n2", "n65")] == [1, 2, 65]
    recs, keys, kl, vl = strides("no_tails")
    assert kl == {266} and keys[0][0] == 0 and keys[-1][0] == 1
    assert strides("short")[2] == {6}
    recs, keys, kl, vl = strides("var")
    assert len(kl) > 3 and len(vl) > 3
    assert {r[3] for r in strides("tombstones")[0]} == {1}
    recs, keys, kl, vl = strides("puts_and_tombstones")
    assert kl == {16} and vl == {0, 32} and {r[3] for r in recs} == {0, 1}
    for name, rows in SHAPES.items():
        for side in (0, 1):
            assert all(key_hash(r[0]) & 1 == side for r in records(rows, side)), name


# ---------------- routes ----------------

class Routes:
    """every route's engine handle paired with its oracle handle"""

    def __init__(self, hip_lib, oracle_lib, rows, filter_type="common", child_filter_type=None,
                 only_split=False):
        self.hip, self.oracle = hip_lib, oracle_lib
        self.envs = {} if filter_type == "common" else {"rocksdb.filter_type": filter_type}
        self.child_envs = self.envs if child_filter_type is None else \
            {"rocksdb.filter_type": child_filter_type}
        self.handles, self.pairs = [], {}
        self.own = records(rows, 0)    # owned by partition 0 of 2
        self.other = records(rows, 1, first_seq=1 + len(rows))  # by partition 1
        self.tmp = tempfile.mkdtemp(prefix="run-creation-")
        try:
            if not only_split:
                self._host_routes()
                self._compaction_route()
            self._split_route()
        except BaseException:
            self.close()
            raise

    def _h(self, lib, pidx, pv=1, envs=None):
        h = _open(lib, pidx, 0 if lib is self.hip else -1, pv=pv)
        self.handles.append(h)
        envs = self.envs if envs is None else envs
        if envs:
            h.set_envs(envs)
        return h

    def _oracle(self, pidx, *runs):
        o = self._h(self.oracle, pidx)
        for run in runs:
            o.ingest_run(run)
        return o

    def _host_routes(self):
        a = self._h(self.hip, 0)
        a.ingest_run(self.own)
        self.pairs["ingest"] = (a, self._oracle(0, self.own), self.own)

        b = self._h(self.hip, 0)
        # writes take sequence numbers 0, 1, ...: a first write to the first
        # key, overwritten next, brings every record to its number in self.own
        hk, sk = D.restore_key(self.own[0][0])
        assert b.remove(hk, sk) == OK
        for key, value, _, kind in self.own:
            hk, sk = D.restore_key(key)
            if kind:
                assert b.remove(hk, sk) == OK
            else:
                assert b.put(hk, sk, D.decode_value(value, 1)[2], 0, NOW) == OK
        assert b.flush() == OK
        self.pairs["flush"] = (b, self._oracle(0, self.own), self.own)

        c = self._h(self.hip, 0)
        assert a.checkpoint(self.tmp, 1) == OK
        assert c.restore(self.tmp, 1) == OK
        self.pairs["restore"] = (c, self._oracle(0, self.own), self.own)

    def _compaction_route(self):
        old = [extra_record(self.own)]
        d = self._h(self.hip, 0)
        d.ingest_run(old)
        d.ingest_run(self.own)
        err, st = d.compact_runs(1, 1, NOW)
        n = len(self.own)
        assert err == OK
        assert (st.input_records, st.output_records, st.shadowed, st.expired, st.filtered) == \
            (n, n, 0, 0, 0)
        self.pairs["compaction"] = (d, self._oracle(0, old, self.own), old + self.own)

    def _split_route(self):
        p = self._h(self.hip, 0, pv=0)
        c = self._h(self.hip, 1, pv=None, envs=self.child_envs)
        p.ingest_run(sorted(self.own + self.other))
        err, st = p.split(c, 2)
        assert err == OK
        assert (st.parent_records, st.child_records, st.dropped_records,
                st.parent_unpruned_runs) == (len(self.own), len(self.other), 0, 0)
        self.pairs["split_parent"] = (p, self._oracle(0, self.own), self.own)
        self.pairs["split_child"] = (c, self._oracle(1, self.other), self.other)

    def check(self):
        for route, (g, o, recs) in self.pairs.items():
            keys = sorted(r[0] for r in recs)
            hks = sorted({D.restore_key(k)[0] for k in keys})[:4]
            assert g.num_records() == len(recs), route
            try:
                _same_reads(g, o, keys, hks, epochs=(NOW,))
                eg, sg = g.manual_compact(NOW)
                eo, so = o.manual_compact(NOW)
                assert eg == eo == OK
                print(route, stats_dict(sg))
                assert stats_dict(sg) == stats_dict(so)
                puts = sum(1 for r in recs if r[3] == 0)
                assert (so.input_records, so.output_records, so.tombstones) == \
                    (len(recs), puts, len(recs) - puts)
                _same_reads(g, o, keys, hks, epochs=(NOW,))
            except AssertionError as e:
                raise AssertionError("route %s: %s" % (route, e)) from e

    def close(self):
        for h in self.handles:
            h.close()
        shutil.rmtree(self.tmp, ignore_errors=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_route_builds_the_same_run(hip_lib, oracle_lib, shape):
    with Routes(hip_lib, oracle_lib, SHAPES[shape]) as r:
        assert list(r.pairs) == ["ingest", "flush", "restore", "compaction", "split_parent",
                                 "split_child"]
        r.check()


@pytest.mark.parametrize("shape", ["tails", "var", "puts_and_tombstones"])
def test_every_route_without_filters(hip_lib, oracle_lib, shape):
    """rocksdb.filter_type=none on every handle: runs carry no bloom columns"""
    with Routes(hip_lib, oracle_lib, SHAPES[shape], filter_type="none") as r:
        r.check()


@pytest.mark.parametrize("shape", ["tails", "var", "puts_and_tombstones"])
def test_split_child_without_filters(hip_lib, oracle_lib, shape):
    """the split builds the child's runs with the child's setting (none) while
    the parent keeps the default (common)"""
    with Routes(hip_lib, oracle_lib, SHAPES[shape], child_filter_type="none",
                only_split=True) as r:
        assert list(r.pairs) == ["split_parent", "split_child"]
        r.check()
