"""Shared cases for the multi-run read view (tests/test_read_view_model.py on
the CPU, tests/test_read_view_gpu.py on the device).

Every read that is no point lookup builds a view first (HipEngine::build_view,
engine.cpp): k_bounds cuts a window [lo, hi) out of every run, one of three
rank kernels orders the windows' records (k_rank_grp<1>, k_rank_ldst, k_rank,
the last two with or without a bound table of one or two levels), and
k_visible, a prefix sum and k_gather keep the newest versions that are no
tombstone.  A compaction ranks [0, n) of every run; only a bounded read hands
the rank kernels windows with lo != 0, empty windows and an anchor run chosen
per window.  This module builds the data sets and ranges that reach those
shapes before any compaction, and restates in plain Python what the engine
must then report through rrdb_last_view_route: the route, the group sizes of a
window and the per-block staged total of k_rank_ldst.  The constants mirror
engine_common.h / kernels.hip; test_constants_have_not_drifted parses them.

Nothing here is committed data: the sets are generated, every id is below
10^8 so that the 18- and 32-byte keys keep their tail words, and values carry
at most 16 user bytes.
"""
import bisect
import random
from collections import namedtuple

from incubator_pegasus_amd import data as D
from incubator_pegasus_amd.capi import (ROUTE_NONE, ROUTE_RANK_GLOBAL, ROUTE_RANK_GRP,
                                        ROUTE_RANK_LDST, ViewRoute)
from test_fused_emit_gpu import NOW, make_value
from test_rank_emit_batching_gpu import SP, grouped_runs, gs_of, key_of

# ---- mirrored from engine_common.h / kernels.hip ----
VIEW_BT_MIN_RECORDS = 100000  # a window above it gets a bound table (global, ldst)
GRP_VIEW_BLOCKS = 3584        # grid cap of launch_rank_grp_view
LDST_CAP = 3072               # tail words one k_rank_ldst workgroup stages
GRP_CAP = 2048                # largest staged group of k_rank_grp
GRP_TARGET = 1024
LDST_MAXR = 32
BLOCK = 256                   # records per k_rank_ldst workgroup
WAVE = 64
BT_SHIFT_DEFAULT = 5          # HipEngine::bt_shift

USER_LEN = 16
FIRST, LAST = b"\x00\x00", b"\xff\xff"
HK32 = b"u:" + b"0" * 14      # the one hashkey of the 32-byte keys

Range = namedtuple("Range", "name start stop start_inclusive stop_inclusive")


# ---- the data sets --------------------------------------------------------

BOUNDED_R = 8
BOUNDED_G = 1 << gs_of(BOUNDED_R)       # 128 anchor records per group
BOUNDED_ANCHOR_RUN = 3
BOUNDED_N_ANCHOR = 40 * BOUNDED_G + 1
G_STAGED, G_OVER, G_NEWEST, G_OLDEST = 2, 5, 9, 10
BOUNDED_DUPS = (1, 6, 11, 12, 20)
G_DUP, G_TOMB, G_PLAIN = 6, 11, 24      # boundary dup, its tombstoned kind, no dup
BOUNDED_EXTRAS = {
    G_STAGED: 300, 3: 1700, G_OVER: 2200, 8: 900,
    G_NEWEST: [0, 0, 0, 0, 0, 0, 300],  # only the newest run between two anchors
    G_OLDEST: [300, 0, 0, 0, 0, 0, 0],  # only the oldest
    15: 60, 16: 1900, 30: 500,
}


def anchor_id(g, j=0, G=BOUNDED_G, sp=SP):
    """id of the j-th anchor-run record of full-range group g"""
    return (g * G + j) * sp


def _set_kind(runs, r, key, what):
    """rewrite run r's version of `key` as a tombstone, a live or an expired put"""
    i = bisect.bisect_left([rec[0] for rec in runs[r]], key)
    k, _, seq, _ = runs[r][i]
    assert k == key
    if what == "del":
        runs[r][i] = (k, b"", seq, 1)
    else:
        expire = NOW - 10 if what == "dead" else 0
        runs[r][i] = (k, make_value(seq % 1000, seq, USER_LEN, expire), seq, 0)


def bounded_runs(klen=18):
    """8 runs, the anchor run (the largest) in the middle.  Group 5 is over
    GRP_CAP, groups 2, 3, 8, 16 and 30 are staged groups of several sizes,
    groups 9 and 10 hold records of one other run only (the newest, the
    oldest), the first anchor key of the BOUNDED_DUPS groups is in every run.
    Of those, group 11's newest version is a tombstone over seven puts and
    group 12's an expired put; group 6's is a live put."""
    runs = grouped_runs(BOUNDED_R, BOUNDED_N_ANCHOR, BOUNDED_EXTRAS,
                        anchor_run=BOUNDED_ANCHOR_RUN, seed=31 + klen, klen=klen,
                        user_len=USER_LEN, boundary_dups=BOUNDED_DUPS)
    for r in range(BOUNDED_R):
        _set_kind(runs, r, key_of(anchor_id(G_TOMB), klen), "del" if r == 7 else "put")
        _set_kind(runs, r, key_of(anchor_id(12), klen), "dead" if r == 7 else "put")
        _set_kind(runs, r, key_of(anchor_id(G_DUP), klen), "put")
    _set_kind(runs, BOUNDED_ANCHOR_RUN, key_of(anchor_id(G_PLAIN), klen), "put")
    return runs


MVG_R = 32
MVG_G = 1 << gs_of(MVG_R)               # 32
MVG_ANCHOR_RUN = 16
MVG_SP = 512
MVG_N_ANCHOR = GRP_VIEW_BLOCKS * MVG_G + MVG_G * 100 + 1
MVG_GROUPS = GRP_VIEW_BLOCKS + 101
MVG_DUPS = (3, 50) + tuple(range(GRP_VIEW_BLOCKS + 6, MVG_GROUPS - 2, 12))


def many_view_groups_runs():
    """R = 32: the anchor run holds GRP_VIEW_BLOCKS * 32 + 32 * 100 + 1
    records, so a full view has 3685 groups on 3584 workgroups and the first
    101 workgroups rank a second group.  Those second groups (3584 and up) hold
    the extras: three other runs supply 24, 20 and 16 records each, a few of
    them ids another run holds too, with tombstones and TTLs among them."""
    extras = {}
    for g in range(GRP_VIEW_BLOCKS + 1, MVG_GROUPS - 1):
        spec = [0] * (MVG_R - 1)
        for n, s in ((24, g % 31), (20, (g + 9) % 31), (16, (g + 20) % 31)):
            spec[s] = n
        extras[g] = spec
    return grouped_runs(MVG_R, MVG_N_ANCHOR, extras, anchor_run=MVG_ANCHOR_RUN, seed=77,
                        user_len=USER_LEN, boundary_dups=MVG_DUPS, sp=MVG_SP)


BT_SIZES = (40001, 35003, 30011)        # no multiple of 256, oldest first
BT_CLUSTER = 4000                       # ids of the newest run between two of the oldest
BT_STEP = 16                            # id spacing outside the cluster
BT_J0 = 150                             # the cluster follows the J0-th id
BT_N_IDS = (sum(BT_SIZES) - BT_CLUSTER) * 10 // 11  # distinct ids outside the cluster


def bt_id(j):
    return j * BT_STEP if j <= BT_J0 else j * BT_STEP + 4096


def bt_cluster_key(n):
    """the n-th key of the cluster, 0 <= n < BT_CLUSTER"""
    return key_of(bt_id(BT_J0) + 1 + n)


def bt_fixed_runs():
    """3 tail-word eligible runs of 40001 / 35003 / 30011 records, interleaved
    id by id.  About one id in ten is in two runs, 3% of the records are
    tombstones, 4% carry a TTL, half of them expired.  BT_CLUSTER consecutive
    ids of run 2 lie between two neighbouring ids of run 0: the k_rank_ldst
    block of run 0 that spans them would stage them all and falls back."""
    rnd = random.Random(4242)
    left = [BT_SIZES[0], BT_SIZES[1], BT_SIZES[2] - BT_CLUSTER]
    n_ids = BT_N_IDS
    slots = [r for r, n in enumerate(left) for _ in range(n)]
    rnd.shuffle(slots)
    # the cluster's neighbours belong to run 0 alone
    for j in (BT_J0, BT_J0 + 1):
        swap = slots.index(0, n_ids) if slots[j] != 0 else j
        slots[j], slots[swap] = slots[swap], slots[j]
    holders = [{slots[j]} for j in range(n_ids)]
    for r in slots[n_ids:]:
        while True:
            j = rnd.randrange(n_ids)
            if r not in holders[j] and j not in (BT_J0, BT_J0 + 1) and len(holders[j]) < 2:
                holders[j].add(r)
                break
    ids = [[] for _ in BT_SIZES]
    for j, hs in enumerate(holders):
        for r in hs:
            ids[r].append(bt_id(j))
    ids[2] += [bt_id(BT_J0) + 1 + n for n in range(BT_CLUSTER)]
    kinds = ("put",) * 93 + ("del",) * 3 + ("ttl",) * 2 + ("dead",) * 2
    runs = []
    for r, mine in enumerate(ids):
        recs = []
        for n, i in enumerate(sorted(mine)):
            seq = r * 10_000_000 + n + 1
            what = "put" if n == 0 else rnd.choice(kinds)
            expire = {"ttl": NOW + 500, "dead": NOW - 10}.get(what, 0)
            val = b"" if what == "del" else make_value(i, seq, USER_LEN, expire)
            recs.append((key_of(i), val, seq, 1 if what == "del" else 0))
        runs.append(recs)
    return runs


BT_VAR_HKS = (b"h%05d", b"hk%06d", b"hash-%07d")  # 6, 8 and 12 bytes
BT_VAR_N = 26500                                   # records per run, before the pairs
BT_VAR_PAIRS = 200


def bt_var_runs():
    """4 runs of variable-length keys (no tail words: k_rank and the table
    read whole keys through koff): three hashkey lengths, sortkeys of 0 to 9
    bytes, one key in ten in two runs, tombstones and TTLs, and BT_VAR_PAIRS
    pairs of sortkeys of which one is a strict prefix of the other, the two in
    different runs."""
    rnd = random.Random(99)
    per_run = [dict() for _ in range(4)]

    def put(r, key, i):
        what = rnd.choice(("put",) * 16 + ("ttl", "dead", "del", "del"))
        per_run[r][key] = (i, what)

    for i in range(4 * BT_VAR_N * 10 // 11):
        hk = BT_VAR_HKS[i % 3] % (i // 3)
        sk = (b"", b"s", b"s%d" % (i % 97), b"sortkey-%d" % (i % 7))[(i // 3) % 4]
        r = rnd.randrange(4)
        put(r, D.generate_key(hk, sk), i)
        if i % 10 == 0:
            put((r + 1 + rnd.randrange(3)) % 4, D.generate_key(hk, sk), i)
    for n in range(BT_VAR_PAIRS):
        hk = BT_VAR_HKS[n % 3] % (1000 + 17 * n)
        r = n % 4
        put(r, D.generate_key(hk, b"pre"), n)
        put((r + 1 + n % 3) % 4, D.generate_key(hk, b"pre" + (b"\x00", b"fix", b"\xff")[n % 3]), n)
    runs = []
    for r, recs in enumerate(per_run):
        out = []
        for n, key in enumerate(sorted(recs)):
            i, what = recs[key]
            seq = r * 10_000_000 + n + 1
            if n == 0:
                what = "put"
            expire = {"ttl": NOW + 500, "dead": NOW - 10}.get(what, 0)
            val = b"" if what == "del" else make_value(i, seq, 3 + i % 14, expire)
            out.append((key, val, seq, 1 if what == "del" else 0))
        runs.append(out)
    return runs


DATA = {
    "bounded": bounded_runs,
    "bounded32": lambda: bounded_runs(klen=32),
    "many_view_groups": many_view_groups_runs,
    "bt_fixed": bt_fixed_runs,
    "bt_var": bt_var_runs,
}
ELIGIBLE = {"bounded": True, "bounded32": True, "many_view_groups": True, "bt_fixed": True,
            "bt_var": False}
_RUNS, _KEYS = {}, {}


def runs_of(name):
    if name not in _RUNS:
        _RUNS[name] = DATA[name]()
    return _RUNS[name]


def keys_of(name):
    """the key list of every run (what the restatements bisect in)"""
    if name not in _KEYS:
        _KEYS[name] = [[rec[0] for rec in run] for run in runs_of(name)]
    return _KEYS[name]


def run_arrays(run):
    """a run as the numpy arrays of ingest_run_arrays"""
    import numpy as np

    from incubator_pegasus_amd.capi import _pack

    keys, koff = _pack([r[0] for r in run])
    vals, voff = _pack([r[1] for r in run])
    return keys, koff, vals, voff, np.array([(r[2] << 1) | r[3] for r in run], dtype=np.uint64)


# ---- the expectation: a plain dict merge ----------------------------------

_MERGED = {}


def merged(name):
    """sorted [(key, value, kind)] of the newest version of every key: the
    runs laid over one another, oldest first"""
    if name not in _MERGED:
        newest = {}
        for run in runs_of(name):
            for key, val, _, kind in run:
                newest[key] = (val, kind)
        _MERGED[name] = [(k,) + newest[k] for k in sorted(newest)]
    return _MERGED[name]


def range_is_empty(rg):
    """the handlers return before they build a view"""
    return rg.start > rg.stop or \
        (rg.start == rg.stop and not (rg.start_inclusive and rg.stop_inclusive))


_MERGED_KEYS, _ROWS = {}, {}


def merged_keys(name):
    if name not in _MERGED_KEYS:
        _MERGED_KEYS[name] = [r[0] for r in merged(name)]
    return _MERGED_KEYS[name]


def expected_rows(name, rg, now=NOW):
    """[(key, user data, expire_ts)] a scan of the range returns at `now`"""
    if (name, rg, now) not in _ROWS:
        _ROWS[name, rg, now] = _expected_rows(name, rg, now)
    return _ROWS[name, rg, now]


def _expected_rows(name, rg, now):
    if range_is_empty(rg):
        return []
    rows = merged(name)
    keys = merged_keys(name)
    lo = (bisect.bisect_left if rg.start_inclusive else bisect.bisect_right)(keys, rg.start)
    hi = (bisect.bisect_right if rg.stop_inclusive else bisect.bisect_left)(keys, rg.stop)
    out = []
    for key, val, kind in rows[lo:hi]:
        if kind == 1:
            continue
        expire, _, user = D.decode_value(val, 1)
        if 0 < expire <= now:
            continue
        out.append((key, user, expire))
    return out


# ---- build_view restated --------------------------------------------------

def stop_excl(rg):
    return rg.stop + b"\x00" if rg.stop_inclusive else rg.stop


def windows(keys, start, stop_x):
    """k_bounds: the window [lo, hi) of every run; stop_x None = unbounded"""
    lo = [bisect.bisect_left(k, start) for k in keys]
    hi = [len(k) if stop_x is None else bisect.bisect_left(k, stop_x) for k in keys]
    return lo, [max(h, l) for l, h in zip(lo, hi)]


def anchor_run(lo, hi):
    """build_anchors: the first run with the largest window"""
    return max(range(len(lo)), key=lambda r: (hi[r] - lo[r], -r))


def n_groups_of(lo, hi):
    gs = gs_of(len(lo))
    q0 = anchor_run(lo, hi)
    return max(1, (hi[q0] - lo[q0] + (1 << gs) - 1) >> gs)


def bound_levels(lo, hi, bt_shift):
    """build_bound_table: the coarse level is built only for a long window"""
    wmax = max(h - l for l, h in zip(lo, hi))
    return 2 if (wmax >> (bt_shift + 6)) > 8 else 1


def expected_route(name, mode, start, stop_x, bt_shift=BT_SHIFT_DEFAULT):
    """the ViewRoute rrdb_last_view_route must report after a view of
    [start, stop_x) under engine.rank_mode = mode"""
    keys = keys_of(name)
    R = len(keys)
    lo, hi = windows(keys, start, stop_x)
    total = sum(h - l for l, h in zip(lo, hi))
    if total == 0:
        return ViewRoute(ROUTE_NONE, 0, 0, 0, 0)
    k0 = bisect.bisect_left(merged_keys(name), start)
    k1 = len(merged(name)) if stop_x is None else bisect.bisect_left(merged_keys(name), stop_x)
    visible = sum(kind == 0 for _, _, kind in merged(name)[k0:k1])
    eligible = ELIGIBLE[name] and R > 1
    if mode == "grp" and eligible and R <= LDST_MAXR:
        return ViewRoute(ROUTE_RANK_GRP, 0, n_groups_of(lo, hi), total, visible)
    levels = bound_levels(lo, hi, bt_shift) if R > 1 and total > VIEW_BT_MIN_RECORDS else 0
    rank = ROUTE_RANK_LDST if mode == "ldst" and eligible else ROUTE_RANK_GLOBAL
    return ViewRoute(rank, levels, 0, total, visible)


def scan_route(name, mode, rg, bt_shift=BT_SHIFT_DEFAULT):
    """the report after rrdb_scan_open of the range; None when the handler
    returns before it builds a view (the report keeps its last value)"""
    if range_is_empty(rg):
        return None
    return expected_route(name, mode, rg.start, stop_excl(rg), bt_shift)


def group_bounds(keys, lo, hi):
    """k_anchor_rows restated for a window: row g is every run's boundary of
    group g.  The anchor key is the anchor run's record lo + g * 2^gs; run q's
    boundary is the first record of its window not below that key, and for
    runs newer than the anchor run the first above it."""
    R = len(keys)
    gs = gs_of(R)
    q0 = anchor_run(lo, hi)
    rows = [list(lo)]
    for g in range(1, n_groups_of(lo, hi)):
        i = lo[q0] + (g << gs)
        k = keys[q0][i]
        rows.append([i if q == q0 else
                     (bisect.bisect_right if q > q0 else bisect.bisect_left)(keys[q], k, lo[q],
                                                                              hi[q])
                     for q in range(R)])
    rows.append(list(hi))
    return rows


def group_sizes(keys, lo, hi):
    rows = group_bounds(keys, lo, hi)
    return [sum(b1) - sum(b0) for b0, b1 in zip(rows, rows[1:])]


def ldst_block_totals(keys, lo, hi, bt_shift):
    """k_rank_ldst restated: the tail words each 256-record block would stage.
    A record i of run r reads rows j and j + 1 of run r's bound table, j =
    (i - lo[r]) >> bt_shift; row j holds the place of run r's record
    lo[r] + (j << bt_shift) in every other run (after it in newer runs, before
    it in older ones) and the last row is hi.  A wave reduces the minimum of
    the row-j entries and the maximum of the row-j+1 entries of its records
    per other run q and, where that maximum is not 0, merges them into the
    block's window of q; the block stages the sum of its windows."""
    R = len(keys)
    wprefix = [0]
    for l, h in zip(lo, hi):
        wprefix.append(wprefix[-1] + h - l)
    total = wprefix[-1]
    memo = {}

    def row(r, j):
        if (r, j) not in memo:
            w = hi[r] - lo[r]
            i = lo[r] + (j << bt_shift)
            if j == (w >> bt_shift) + 1 or i >= hi[r]:
                memo[r, j] = list(hi)
            else:
                k = keys[r][i]
                memo[r, j] = [i if q == r else
                              (bisect.bisect_right if q > r else bisect.bisect_left)(
                                  keys[q], k, lo[q], hi[q]) for q in range(R)]
        return memo[r, j]

    totals = []
    for b0 in range(0, total, BLOCK):
        winlo, winhi = [None] * R, [0] * R
        for w0 in range(b0, min(b0 + BLOCK, total), WAVE):
            wl, wh = [None] * R, [0] * R
            t = w0
            while t < min(w0 + WAVE, total):
                r = bisect.bisect_right(wprefix, t) - 1
                t1 = min(w0 + WAVE, total, wprefix[r + 1])
                j_first = (t - wprefix[r]) >> bt_shift
                j_last = (t1 - 1 - wprefix[r]) >> bt_shift
                for q in range(R):
                    if q != r:
                        a, z = row(r, j_first)[q], row(r, j_last + 1)[q]
                        wl[q] = a if wl[q] is None else min(wl[q], a)
                        wh[q] = max(wh[q], z)
                t = t1
            for q in range(R):
                if wh[q] > 0:
                    winlo[q] = wl[q] if winlo[q] is None else min(winlo[q], wl[q])
                    winhi[q] = max(winhi[q], wh[q])
        totals.append(sum(winhi[q] - winlo[q] for q in range(R)
                          if winlo[q] is not None and winhi[q] > winlo[q]))
    return totals


def newest_is_tombstone(name, key):
    rows = merged(name)
    i = bisect.bisect_left(merged_keys(name), key)
    return i < len(rows) and rows[i][0] == key and rows[i][2] == 1


def in_every_run(name, key):
    return all(k[min(bisect.bisect_left(k, key), len(k) - 1)] == key for k in keys_of(name))


# ---- range cases of bounded / bounded32 -----------------------------------

def placement_keys(klen):
    """the kinds of key a range starts or stops at"""
    a = anchor_id(G_PLAIN)
    return {
        "anchor": key_of(a, klen),
        "anchor_prev": key_of(a - SP, klen),          # the anchor run's neighbours
        "anchor_next": key_of(a + SP, klen),
        "anchor_below": key_of(a - 1, klen),          # no record: just below and above
        "anchor_above": key_of(a + 1, klen),
        "dup": key_of(anchor_id(G_DUP), klen),        # in every run, newest a live put
        "tomb": key_of(anchor_id(G_TOMB), klen),      # in every run, newest a tombstone
    }


def bounded_ranges(klen=18):
    P = placement_keys(klen)
    out = []

    def add(name, start, stop, si=True, sti=False):
        out.append(Range(name, start, stop, si, sti))

    for kind, key in P.items():
        i = int(key[4:18]) if klen == 18 else int(key[19:32])
        for si in (True, False):
            # two and a half groups on from the start
            add("start_%s_%s" % (kind, "incl" if si else "excl"), key,
                key_of(i + 5 * BOUNDED_G * SP // 2, klen), si, False)
        for sti in (True, False):
            add("stop_%s_%s" % (kind, "incl" if sti else "excl"),
                key_of(i - 5 * BOUNDED_G * SP // 2 - 7, klen), key, True, sti)
    for kind in ("anchor", "dup", "tomb", "anchor_below"):
        add("point_%s_incl" % kind, P[kind], P[kind], True, True)
        add("point_%s_excl" % kind, P[kind], P[kind], True, False)
        add("point_%s_open" % kind, P[kind], P[kind], False, False)
    first = key_of(0, klen)
    last = key_of(anchor_id(0, BOUNDED_N_ANCHOR - 1), klen)
    add("before_first", FIRST, first, True, False)
    add("up_to_first", FIRST, first, True, True)
    add("after_last", last, LAST, False, False)
    add("from_last", last, LAST, True, False)
    add("beyond_last", key_of(anchor_id(0, BOUNDED_N_ANCHOR - 1) + 1, klen), LAST, True, False)
    add("reversed", P["anchor_next"], P["anchor"], True, True)
    base = anchor_id(G_STAGED) + 1
    add("inside_staged_group", key_of(base + 10, klen), key_of(base + 200, klen))
    base = anchor_id(G_OVER) + 1
    add("inside_oversized_group", key_of(base + 100, klen), key_of(base + 1900, klen))
    # the anchor run's window is the largest, and its second group of the
    # window is the oversized one: a group over GRP_CAP whose lo is not 0
    add("oversized_group_in_window", key_of(anchor_id(G_OVER - 1), klen),
        key_of(anchor_id(G_OVER + 2), klen))
    add("newest_run_anchors", key_of(anchor_id(G_NEWEST), klen),
        key_of(anchor_id(G_NEWEST, 1), klen), False, False)
    add("oldest_run_anchors", key_of(anchor_id(G_OLDEST), klen),
        key_of(anchor_id(G_OLDEST, 1), klen), False, False)
    add("two_groups_dup_to_tomb", P["dup"], key_of(anchor_id(G_DUP + 2), klen), False, True)
    add("full", FIRST, LAST)
    return out


def mg_ranges():
    """range multi_gets of bounded32's hashkey over more than MG_MAX_ROWS
    candidate records: (name, start_sortkey, stop_sortkey, start_inclusive,
    stop_inclusive).  The start keys sit in the first groups and the stop
    keys in the last, at the same kinds of key as the scan ranges."""
    def sk(i):
        return key_of(i, 32)[18:]

    far = anchor_id(38, 5)
    out = []
    for kind, i in (("anchor", anchor_id(1, 64)), ("anchor_above", anchor_id(1, 64) + 1),
                    ("dup", anchor_id(1)), ("first", 0)):
        for si in (True, False):
            out.append(Range("start_%s_%s" % (kind, "incl" if si else "excl"), sk(i), sk(far),
                             si, False))
    for kind, i in (("anchor", anchor_id(G_PLAIN)), ("dup", anchor_id(20)),
                    ("tomb", anchor_id(G_TOMB))):
        for sti in (True, False):
            out.append(Range("stop_%s_%s" % (kind, "incl" if sti else "excl"), sk(1), sk(i),
                             True, sti))
    out.append(Range("whole_hashkey", b"", b"", True, False))
    out.append(Range("tomb_to_end", sk(anchor_id(G_TOMB)), b"", True, False))
    return out


def mg_scan_range(rg):
    """the key range multi_get_locked turns a sortkey range into"""
    start = D.generate_key(HK32, rg.start)
    if rg.stop:
        return Range(rg.name, start, D.generate_key(HK32, rg.stop), rg.start_inclusive,
                     rg.stop_inclusive)
    return Range(rg.name, start, D.generate_next_blob(HK32), rg.start_inclusive, False)


# ---- ranges of many_view_groups -------------------------------------------

def mvg_key(g, j=0, off=0):
    return key_of(anchor_id(g, j, MVG_G, MVG_SP) + off)


def mvg_ranges():
    """8 ranges that start at a boundary-dup key: six start and stop inside
    groups beyond GRP_VIEW_BLOCKS, two start in the first groups and leave
    more than GRP_VIEW_BLOCKS groups in a window whose lo is not 0"""
    late = [g for g in MVG_DUPS if g >= GRP_VIEW_BLOCKS]
    out = []
    for n, g in enumerate(late[:6]):
        out.append(Range("late_%d" % g, mvg_key(g), mvg_key(g + 2 + n, 7, 3), n % 2 == 0,
                         n % 3 == 0))
    out.append(Range("long_3", mvg_key(3), mvg_key(MVG_GROUPS - 2, 9, 5), False, False))
    out.append(Range("long_50", mvg_key(50), LAST, True, False))
    return out


# ---- ranges of bt_fixed ---------------------------------------------------

def records_between(name, start, stop_x):
    lo, hi = windows(keys_of(name), start, stop_x)
    return sum(h - l for l, h in zip(lo, hi))


def stop_for_total(name, start, want):
    """an exclusive stop key that puts exactly `want` records of all runs in
    [start, stop), or None where the versions of one key straddle it"""
    cum = _cumulative(name)
    keys = [k for k, _ in cum]
    i = bisect.bisect_left(keys, start)
    before = cum[i - 1][1] if i else 0
    j = bisect.bisect_left([c for _, c in cum], before + want)
    if j >= len(cum) - 1 or cum[j][1] != before + want:
        return None
    return keys[j + 1]


_CUM = {}


def _cumulative(name):
    """[(key, records of all runs up to and including key)]"""
    if name not in _CUM:
        count = {}
        for ks in keys_of(name):
            for k in ks:
                count[k] = count.get(k, 0) + 1
        out, c = [], 0
        for k in sorted(count):
            c += count[k]
            out.append((k, c))
        _CUM[name] = out
    return _CUM[name]


def _window_of(name, start_keys, want):
    for start in start_keys:
        stop = stop_for_total(name, start, want)
        if stop is not None:
            return start, stop
    raise AssertionError("no range of %d records" % want)


_BT_RANGES = []


def bt_fixed_ranges():
    """(over, under, edge): six ranges above VIEW_BT_MIN_RECORDS that start
    inside the cluster, three just under it, and the two whose windows hold
    exactly VIEW_BT_MIN_RECORDS and VIEW_BT_MIN_RECORDS + 1 records"""
    if not _BT_RANGES:
        _BT_RANGES.append(_bt_fixed_ranges())
    return _BT_RANGES[0]


def _bt_fixed_ranges():
    end = key_of(bt_id(BT_N_IDS - 40))  # 40 ids before the last
    over = [Range("cluster_%d" % n, bt_cluster_key(n), stop, si, False)
            for n, stop, si in ((0, LAST, True), (1, LAST, False), (700, LAST, True),
                                (1999, end, False), (2600, end, True), (3100, LAST, False))]
    starts = [bt_cluster_key(n) for n in range(3500, BT_CLUSTER)]
    under = []
    for n, want in enumerate((VIEW_BT_MIN_RECORDS - 1, VIEW_BT_MIN_RECORDS - 37,
                              VIEW_BT_MIN_RECORDS - 256)):
        start, stop = _window_of("bt_fixed", starts[100 * n:], want)
        under.append(Range("under_%d" % want, start, stop, True, False))
    edge = []
    for want in (VIEW_BT_MIN_RECORDS, VIEW_BT_MIN_RECORDS + 1):
        start, stop = _window_of("bt_fixed", starts[50:], want)
        edge.append(Range("edge_%d" % want, start, stop, True, False))
    return over, under, edge


def bt_before_cluster_range():
    """starts 20 ids before the cluster: lo != 0 in every run, and run 0's
    block that spans the cluster is part of the window"""
    return Range("before_cluster", key_of(bt_id(BT_J0 - 20)), LAST, True, False)


BT_VAR_PREFIX = b"h0"  # hash-key prefix filter: the 6-byte hashkeys h0xxxx


# ---- reads, for either backend --------------------------------------------

_ARRAYS = {}


def ingest(part, name):
    if name not in _ARRAYS:
        _ARRAYS[name] = [run_arrays(run) for run in runs_of(name)]
    for arrays in _ARRAYS[name]:
        part.ingest_run_arrays(*arrays)


def scan_batches(part, rg, now=NOW, **kw):
    """every batch of a scan of the range: [(error, context id, kvs,
    expire_ts, kv_count)].  A parked context's id is given relative to the
    last id the handle issued before the scan (ids grow by one per park on
    both backends), -1 stands for completed."""
    from incubator_pegasus_amd.capi import OK, SCAN_COMPLETED

    base = getattr(part, "_rv_last_ctx", 0)
    res = part.scan_open(rg.start, rg.stop, now, start_inclusive=rg.start_inclusive,
                         stop_inclusive=rg.stop_inclusive, validate_partition_hash=False, **kw)
    out = []
    while True:
        done = res.context_id == SCAN_COMPLETED
        out.append((res.error, -1 if done else res.context_id - base, res.kvs, res.expire_ts,
                    res.kv_count))
        if done or res.error != OK:
            return out
        part._rv_last_ctx = res.context_id
        res = part.scan_next(res.context_id, now)


def rows_of_batches(batches):
    """[(key, value, expire_ts)] of a return_expire_ts scan's batches"""
    return [(k, v, e) for b in batches for (k, v), e in zip(b[2], b[3] or [])]
