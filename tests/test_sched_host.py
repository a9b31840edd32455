"""CPU tests of tests/sched_common.py: the checker of a dispatch order must accept what the builder's contract allows and nothing else, and the
host model shows which inputs the builder's trial loop could not fit before it was repaired."""
import numpy as np
import pytest

import sched_common as sc

TPR, TROWS = 7, 19                  # three tile rows in shares 0..2, two in the others
MAX_LG, SLOTS, MIN_QUOTA = 4, 16, 1


def _table():
    rng = np.random.default_rng(5)
    cost = rng.integers(1, 400, (TROWS, TPR)).astype(np.uint32)
    cost[0, 3] = 90000              # share 0: a tile the quota splits in 16 ...
    cost[8, 1] = 9000               # ... one it splits less ...
    cost[16, 5] = 2500
    return cost


@pytest.fixture(scope="module")
def good():
    cost = _table()
    cap = sc.per_share_of(TPR, TROWS) + 64
    shares = sc.model(cost, 0, cap, SLOTS, MIN_QUOTA, MAX_LG)
    words = sc.build_order(shares, cap, extra_words=8 * 32)
    return shares, cap, words


def _pos(words, k, cap, pred):
    """Positions in share k's list whose entry satisfies pred(col, row, lg, part)."""
    lst = words[:8 * cap].reshape(cap, 8)[:, k]
    return [p for p, e in enumerate(int(x) for x in lst)
            if e != sc.NONE and pred(e & 0xFFF, (e >> 12) & 0xFFF, (e >> 24) & 7, e >> 27)]


def test_the_model_splits_this_table_at_several_lg(good):
    shares, cap, _ = good
    h = sc.lg_histogram(shares)
    assert h[0] > 0 and h[4] > 0 and sum(1 for x in h[1:] if x) >= 2, h
    assert all(sh["fits"] and sh["nvalid"] <= cap for sh in shares)
    bins = {b for sh in shares for _, b in sh["tiles"].values()}
    assert len(bins) > 8, "the table must spread over bins, or the order test below tests nothing"


def test_checker_accepts_the_models_own_order(good):
    shares, cap, words = good
    assert sc.check_order(words, shares, cap) == []
    assert sc.check_order(words[:8 * cap], shares, cap) == []     # an order read back from a launch has no sentinel part


def test_checker_accepts_any_order_inside_a_bin(good):
    shares, cap, words = good
    w = words.copy()
    lst = w[:8 * cap].reshape(cap, 8)
    sh = shares[3]
    ps = _pos(w, 3, cap, lambda c, r, lg, p: lg == 0)
    same = [(a, b) for a in ps for b in ps if a < b and sh["tiles"][(int(lst[a, 3]) & 0xFFF, (int(lst[a, 3]) >> 12) & 0xFFF)][1] ==
            sh["tiles"][(int(lst[b, 3]) & 0xFFF, (int(lst[b, 3]) >> 12) & 0xFFF)][1]]
    assert same, "no two unsplit tiles of share 3 share a bin"
    a, b = same[0]
    lst[a, 3], lst[b, 3] = lst[b, 3], lst[a, 3]
    assert sc.check_order(w, shares, cap) == []


def _corrupt(kind, shares, cap, words):
    w = words.copy()
    lst = w[:8 * cap].reshape(cap, 8)          # a view: lst[pos, k]
    k = 0
    col0 = lst[:, k].copy()
    split = _pos(w, k, cap, lambda c, r, lg, p: lg > 0 and p == 1)[0]          # part 1 of the first split tile
    singles = _pos(w, k, cap, lambda c, r, lg, p: lg == 0)
    nvalid = shares[k]["nvalid"]
    bin_of = lambda p: shares[k]["tiles"][(int(col0[p]) & 0xFFF, (int(col0[p]) >> 12) & 0xFFF)][1]
    if kind == "drop a part":
        lst[split:nvalid - 1, k] = col0[split + 1:nvalid]
        lst[nvalid - 1, k] = sc.NONE
    elif kind == "duplicate a tile":
        lst[singles[1], k] = col0[singles[0]]
    elif kind == "swap two entries of different bins":
        a = singles[0]
        b = next(p for p in singles if bin_of(p) != bin_of(a))
        lst[a, k], lst[b, k] = col0[b], col0[a]
    elif kind == "mis-number a part":
        lst[split, k] = col0[split] ^ np.uint32(2 << 27)
    elif kind == "break a tile's run":
        lg = (int(col0[split]) >> 24) & 7
        after = split - 1 + (1 << lg)          # the first position behind the run
        lst[split, k], lst[after, k] = col0[after], col0[split]
    elif kind == "leave a hole before nvalid":
        lst[singles[2], k] = sc.NONE
    elif kind == "write one word past the cap":
        w[8 * cap] = sc.NONE
    elif kind == "write an entry past the cap":
        w[8 * cap + 5] = col0[0]
    elif kind == "an entry behind nvalid":
        lst[nvalid, k] = col0[singles[0]]
    elif kind == "a tile of another share":
        lst[singles[0], k] = lst[0, 1]
    elif kind == "a wrong lg":
        lst[singles[0], k] = col0[singles[0]] | np.uint32(1 << 24)
    else:
        raise KeyError(kind)
    return w


CORRUPTIONS = ["drop a part", "duplicate a tile", "swap two entries of different bins", "mis-number a part", "break a tile's run",
               "leave a hole before nvalid", "write one word past the cap", "write an entry past the cap", "an entry behind nvalid",
               "a tile of another share", "a wrong lg"]


@pytest.mark.parametrize("kind", CORRUPTIONS)
def test_checker_rejects(good, kind):
    shares, cap, words = good
    w = _corrupt(kind, shares, cap, words)
    assert not np.array_equal(w, words), "the corruption changed nothing"
    errs = sc.check_order(w, shares, cap)
    assert errs, f"{kind}: accepted"


def test_model_quota_rules():
    """The starting quota: sum / slots with a 64-bit sum, capped at 0x7FFFFFFF, raised to min_quota and to 1; lg is the smallest that brings
    a part under the quota; a share without tiles has no entries."""
    cost = np.full((3, 2), 0xFFFFFFFF, np.uint32)              # shares 0..2 hold two tiles each, their sum passes 32 bits
    sh = sc.model(cost, 0, 2 + 1024, 1, 1, 4)
    assert sh[0]["quota"] == 0x7FFFFFFF and sh[0]["nvalid"] == 4 and sh[3]["nvalid"] == 0 and sh[3]["tiles"] == {}
    sh = sc.model(np.zeros((1, 1), np.uint32), 0, 1, 512, 0, 4)
    assert sh[0]["quota"] == 1 and sh[0]["tiles"] == {(0, 0): (0, 0)}
    q = 1500
    cost = np.array([[q, q + 1, 2 * q + 1, 2 * q + 2, 16 * q + 15, 16 * q + 16, 1 << 31]], np.uint32)
    sh = sc.model(cost, 0, 7 + 1024, 1 << 30, q, 4)[0]
    assert sh["quota"] == q
    assert [sh["tiles"][(c, 0)][0] for c in range(7)] == [0, 1, 1, 2, 4, 4, 4]
    assert [sc.model(cost, 0, 7 + 1024, 1 << 30, q, m)[0]["tiles"][(6, 0)][0] for m in (0, 1, 2)] == [0, 1, 2]


def test_clamp_outliers_changes_the_scale_only():
    cost = np.full((32, 41), 100_000, np.uint32)               # 164 tiles per share
    cost[0, 0] = 100_000_000
    plain = sc.model(cost, 0, 164, 0, 1500, 4)[0]
    clamped = sc.model(cost, 1, 164, 0, 1500, 4)[0]
    assert plain["tiles"][(1, 0)][1] == 0 and plain["tiles"][(0, 0)][1] >= 254            # the outlier squeezes the rest into bin 0 (254: 255 / top is rounded)
    assert clamped["tiles"][(1, 0)][1] == 2 and clamped["tiles"][(0, 0)][1] == 255        # 16 x mean = 11.3 M: 1e5 * 255 / 11.3e6 = 2.2
    assert sc.model(cost, 1, 164, 0, 1500, 4)[1] == sc.model(cost, 0, 164, 0, 1500, 4)[1]  # a share without an outlier: the clamp is idle


def test_the_unrepaired_loop_does_not_fit_after_24_doublings():
    """min_quota 1, every cost 2^31, per_share_cap = per_share + 1.  The doubling reaches "never split" by itself once the quota passes 0x3FFFFFFF,
    so 24 trials are enough from any starting quota of 2^8 or more: with split_slots 512 a share's sum / 512 is millions and the old loop fits
    (asserted below, so that nobody looks for the defect there).  It takes a share whose sum / split_slots is below 2^7: then the 24th doubling
    still leaves a quota under 2^31, every tile is split at least in two, and the unrepaired loop goes on with more entries than the list
    holds.  The repaired loop ends at "never split" on the same inputs."""
    for tpr, trows, slots in sc.OVERFLOW_CASES:
        cost, cap = sc.overflow_table(tpr, trows)
        old = sc.model(cost, 0, cap, slots, 1, 4, fixed=False)
        new = sc.model(cost, 0, cap, slots, 1, 4, fixed=True)
        for k in range(8):
            if not old[k]["tiles"]:
                continue
            assert not old[k]["fits"] and old[k]["nvalid"] > cap and old[k]["quota"] < (1 << 31), (tpr, trows, slots, k, old[k]["quota"], old[k]["nvalid"])
            assert new[k]["fits"] and new[k]["quota"] == 0xFFFFFFFF and new[k]["nvalid"] == len(new[k]["tiles"]) <= cap
        assert sc.check_order(sc.build_order(new, cap, 64), new, cap) == []
    cost, cap = sc.overflow_table(41, 26)
    for max_lg in (4, 2, 1):
        assert all(sh["fits"] for sh in sc.model(cost, 0, cap, 512, 1, max_lg, fixed=False))


def test_edge_table_puts_the_quota_where_the_edges_are():
    """The table the GPU cases rely on: the model's quota of every share of the big tables is sc.QUOTA from the sum and from
    min_quota alike, and tiles fall on both sides of every quota << lg."""
    for tpr, trows in ((41, 26), (130, 17)):
        cost = sc.edge_table(tpr, trows)
        for min_quota in (1, 1500):
            shares = sc.model(cost, 0, sc.per_share_of(tpr, trows) + 1024, 512, min_quota, 4)
            assert all(sh["quota"] == sc.QUOTA for sh in shares if sh["tiles"]), [sh["quota"] for sh in shares]
            h = sc.lg_histogram(shares)
            assert all(x >= 8 for x in h), h


@pytest.mark.parametrize("values", sc.VALUES)
def test_value_tables_are_what_their_names_say(values):
    for tpr, trows in sc.SHAPES.values():
        c = sc.value_table(values, tpr, trows)
        assert c.shape == (trows, tpr) and c.dtype == np.uint32
        flat, total = c.reshape(-1), int(c.astype(np.uint64).sum())
        if values == "all zero":
            assert total == 0
        elif values == "all equal":
            assert len(set(flat.tolist())) == 1 and flat[0] > sc.QUOTA
        elif values == "all distinct":
            assert len(set(flat.tolist())) == flat.size
        elif values == "one tile holds 99 %" and flat.size > 1:
            assert int(flat.max()) * 100 == 99 * total
        elif values == ">= 2^31":
            assert flat.min() >= 1 << 31
        elif values == "total overflows 32 bits":
            if flat.size > 1:           # (one tile cannot: its cost is 32 bits)
                assert min(int(c[k::8].astype(np.uint64).sum()) for k in range(min(8, trows))) >= 1 << 32
