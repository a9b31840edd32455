"""A host model of the dispatch-order builder (wt_sched_build, csrc/whitted_trace.inc) and a checker of the order it writes.

The model states the CONTRACT of the builder, not its instruction order:

  share k (k = 0..7) holds the tiles whose tile row = k mod 8; per_share = ceil(trows / 8) * tpr is what a share can hold.
  split_slots == 0: no tile is split (every lg is 0).  Else
    quota = min(sum of the share's costs / split_slots, 0x7FFFFFFF)   [the sum is 64-bit], raised to min_quota, and to 1 if still 0;
    lg(c) = the smallest lg <= max_lg with (c >> lg) <= quota (max_lg if there is none); the quota doubles -- a quota above 0x3FFFFFFF
    becomes 0xFFFFFFFF, "never split" -- until the sum of 2^lg over the share's tiles is at most per_share_cap; after 24 quotas that did
    not fit it is 0xFFFFFFFF.
  bin(c) = min(uint(float32(c >> lg) * scale), 255), scale = 1 if top <= 255 else 255 / top in float32, top = float32(max(1, the largest
    c >> lg of the share)), with clamp_outliers (and a share that has tiles) cut to max(16 * float32(sum) / float32(count), 1).
  order[8 * pos + k], pos < per_share_cap: a tile's 2^lg entries column | row << 12 | lg << 24 | part << 27 at consecutive positions, parts
    0 .. 2^lg - 1 in that order; bins never increase along the list (the order inside a bin is free: the kernel takes positions with atomics);
    0xFFFFFFFF from the end of the entries to per_share_cap.

`fixed=False` models the loop as it was before it was repaired: at most 24 trials, and whatever quota the last doubling left, whether or not the
parts fit -- kept to show on the host which inputs made the scatter write past the list.
"""
import numpy as np

NONE = 0xFFFFFFFF
SENTINEL = 0xA5A5A5A5        # CLW_SCHED_SENTINEL (include/hip_wrap_ext.h): its lg field reads 5, so it is neither an entry nor NONE
f32 = np.float32


def per_share_of(tpr, trows):
    return ((trows + 7) // 8) * tpr


def entry(col, row, lg, part):
    return col | (row << 12) | (lg << 24) | (part << 27)


def _lgs(c, quota, max_lg):
    """lg of every cost of the uint64 array c (c >> l falls with l, so lg is the number of l < max_lg whose part is still above the quota)"""
    lg = np.zeros(c.shape, np.int64)
    for l in range(max_lg):
        lg += (c >> np.uint64(l)) > np.uint64(quota)
    return lg


def model_share(cost, k, clamp_outliers, per_share_cap, split_slots, min_quota, max_lg, fixed=True):
    """cost: uint32 [trows, tpr].  -> dict(tiles={(col, row): (lg, bin)}, quota, nvalid, fits) of share k."""
    cost = np.asarray(cost, np.uint32)
    rows = np.arange(k, cost.shape[0], 8)
    c = cost[rows].astype(np.uint64).reshape(-1)                # the share's costs, (row, column) order
    total = int(c.sum(dtype=object)) if c.size else 0           # exact: the kernel's sum is 64-bit and cannot overflow either
    entries = lambda q: int((1 << _lgs(c, q, max_lg)).sum())
    quota = 0xFFFFFFFF
    fits = True
    if split_slots != 0:
        quota = min(total // split_slots, 0x7FFFFFFF)
        quota = max(quota, min_quota)
        quota = max(quota, 1)
        trial = 0
        while True:
            fits = entries(quota) <= per_share_cap
            if fits:
                break
            trial += 1
            quota = 0xFFFFFFFF if quota > 0x3FFFFFFF else quota * 2
            if trial == 24:                     # 24 trials, then "never split", which always fits ...
                if fixed:
                    quota = 0xFFFFFFFF
                fits = entries(quota) <= per_share_cap      # ... the unrepaired loop: on with the untested quota
                break
    lgs = _lgs(c, quota, max_lg)
    part = (c >> lgs.astype(np.uint64)).astype(np.uint32)
    top = f32(max(1, int(part.max()) if c.size else 1))
    if clamp_outliers and c.size:
        mean16 = f32(f32(16.0) * f32(np.uint64(total))) / f32(c.size)
        top = min(top, max(f32(mean16), f32(1.0)))
    scale = f32(1.0) if top <= f32(255.0) else f32(255.0) / f32(top)
    bins = np.minimum(part.astype(f32) * scale, f32(255.0)).astype(np.int64)
    tpr = cost.shape[1]
    out = {(j % tpr, int(rows[j // tpr])): (int(lgs[j]), int(bins[j])) for j in range(c.size)}
    return dict(tiles=out, quota=quota, nvalid=int((1 << lgs).sum()), fits=fits)


def model(cost, clamp_outliers, per_share_cap, split_slots, min_quota, max_lg, fixed=True):
    return [model_share(cost, k, clamp_outliers, per_share_cap, split_slots, min_quota, max_lg, fixed) for k in range(8)]


def build_order(shares, per_share_cap, extra_words=0):
    """One order the contract accepts, from the model's prediction: bins descending, inside a bin the tiles in (row, column) order."""
    words = np.full(8 * per_share_cap + extra_words, SENTINEL, np.uint32)
    words[:8 * per_share_cap] = NONE
    for k, sh in enumerate(shares):
        pos = 0
        for (col, row), (lg, b) in sorted(sh["tiles"].items(), key=lambda t: (-t[1][1], t[0][1], t[0][0])):
            for q in range(1 << lg):
                words[8 * (pos + q) + k] = entry(col, row, lg, q)
            pos += 1 << lg
    return words


def check_order(words, shares, per_share_cap):
    """-> the list of what is wrong with `words` (8 * per_share_cap order words, then any number of words that must still hold the sentinel)
    as the order of the model's `shares`; empty = accepted."""
    words = np.asarray(words, np.uint32)
    errs = []
    if words.size < 8 * per_share_cap:
        return [f"{words.size} words are fewer than the {8 * per_share_cap} of the list"]
    beyond = np.nonzero(words[8 * per_share_cap:] != SENTINEL)[0]
    if beyond.size:
        errs.append(f"{beyond.size} words beyond the list were written, the first at word {8 * per_share_cap + int(beyond[0])}")
    lists = words[:8 * per_share_cap].reshape(per_share_cap, 8)
    for k, sh in enumerate(shares):
        lst = [int(x) for x in lists[:, k]]
        tiles, nvalid = sh["tiles"], sh["nvalid"]
        if nvalid > per_share_cap:
            errs.append(f"share {k}: the model's {nvalid} entries do not fit {per_share_cap}")
            continue
        seen, pos, last_bin = set(), 0, 255
        while pos < nvalid:
            e = lst[pos]
            if e == NONE:
                errs.append(f"share {k}: a hole at position {pos}, before the {nvalid} entries end")
                pos += 1
                continue
            col, row, lg, part = e & 0xFFF, (e >> 12) & 0xFFF, (e >> 24) & 7, e >> 27
            if (col, row) not in tiles:
                errs.append(f"share {k}: position {pos} holds {e:#x}, no tile of this share")
                pos += 1
                continue
            want_lg, b = tiles[(col, row)]
            if lg != want_lg:
                errs.append(f"share {k}: tile ({col}, {row}) at position {pos} has lg {lg}, the model {want_lg}")
            if (col, row) in seen:
                errs.append(f"share {k}: tile ({col}, {row}) is listed again at position {pos}")
            seen.add((col, row))
            run = [entry(col, row, want_lg, q) for q in range(1 << want_lg)]
            got = lst[pos:pos + len(run)]
            if pos + len(run) > nvalid or got != run:
                errs.append(f"share {k}: tile ({col}, {row}) at position {pos}: entries {[hex(x) for x in got]} are not its parts 0..{len(run) - 1} in a row")
                pos += 1
                continue
            if b > last_bin:
                errs.append(f"share {k}: tile ({col}, {row}) of bin {b} at position {pos} follows bin {last_bin}")
            last_bin = b
            pos += len(run)
        missing = set(tiles) - seen
        if missing:
            errs.append(f"share {k}: {len(missing)} tiles are missing, e.g. {sorted(missing)[0]}")
        tail = [p for p in range(nvalid, per_share_cap) if lst[p] != NONE]
        if tail:
            errs.append(f"share {k}: position {tail[0]} behind the {nvalid} entries holds {lst[tail[0]]:#x}")
    return errs


def lg_histogram(shares, max_lg=4):
    """How many tiles the model serves with 2^lg wavefronts, lg = 0..max_lg."""
    h = [0] * (max_lg + 1)
    for sh in shares:
        for lg, _ in sh["tiles"].values():
            h[lg] += 1
    return h


def order_lgs(words, per_share_cap):
    """The lg fields of the entries of an order."""
    w = np.asarray(words, np.uint32)[:8 * per_share_cap]
    w = w[w != NONE]
    return (w >> 24) & 7


# (tile columns, tile rows, split_slots) at which the trial loop, as it was, ran out of its 24 trials with parts that did not fit: every cost
# 2^31, min_quota 1, per_share_cap = per_share + 1 (tests/test_sched_host.py shows it with the model; the GPU runs the repaired kernel only)
OVERFLOW_CASES = [(1, 1, 1 << 31), (41, 26, 0xFFFFFFFF), (41, 8, 0x7FFFFFFF)]


def overflow_table(tpr, trows):
    return np.full((trows, tpr), 1 << 31, np.uint32), per_share_of(tpr, trows) + 1


# ---- synthetic cost tables for the builder (tests/test_gpu_dispatch.py; tests/test_sched_host.py holds them to what they promise)
SHAPES = {"1x1": (1, 1), "41x26": (41, 26), "5x3 (empty shares)": (5, 3), "130x17 (per_share 390)": (130, 17)}
QUOTA = 1500
EDGES = sorted({v for lg in range(5) for v in ((QUOTA << lg) - 1, QUOTA << lg, (QUOTA << lg) + 1, ((QUOTA + 1) << lg) - 1, (QUOTA + 1) << lg)} | {0, 1, QUOTA - 1})


def edge_table(tpr, trows, slots=512):
    """Every share holds the costs at and around quota << lg, lg = 0..4 (the last value whose part is still <= the quota, the first that is above),
    small costs elsewhere, and one balancing tile that brings the share's sum to slots * QUOTA + 7 -- so the quota is QUOTA whether it comes from
    the sum (min_quota 1) or from min_quota 1500.  A share too small for all of that holds the first edge values it has room for."""
    rng = np.random.default_rng(tpr * 1000 + trows)
    cost = rng.integers(0, 40, (trows, tpr)).astype(np.uint32)
    for k in range(min(8, trows)):
        rows = np.arange(k, trows, 8)
        idx = [(r, c) for r in rows for c in range(tpr)]
        order = rng.permutation(len(idx))
        for v, j in zip(EDGES, order[1:]):
            cost[idx[j]] = v
        if len(idx) > len(EDGES) + 1:
            r0 = idx[order[0]]
            cost[r0] = 0
            rest = int(cost[rows].astype(np.uint64).sum())
            assert slots * QUOTA + 7 - rest > 0
            cost[r0] = slots * QUOTA + 7 - rest
    return cost


def value_table(kind, tpr, trows):
    rng = np.random.default_rng(tpr * 131 + trows * 7 + len(kind))
    n = tpr * trows
    if kind == "all zero":
        c = np.zeros(n, np.uint32)
    elif kind == "all equal":
        c = np.full(n, 7000, np.uint32)
    elif kind == "all distinct":
        c = (rng.permutation(n).astype(np.uint32) * np.uint32(37) + np.uint32(1))
    elif kind == "one tile holds 99 %":
        c = rng.integers(50, 150, n).astype(np.uint32)
        c[n // 2] = 0
        c[n // 2] = 99 * int(c.sum()) if n > 1 else 123456
    elif kind == "around the quota":
        return edge_table(tpr, trows)
    elif kind == ">= 2^31":
        c = rng.integers(1 << 31, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        c[0] = 0xFFFFFFFF
        c[-1] = 1 << 31
    elif kind == "total overflows 32 bits":
        c = rng.integers(0, 1 << 27, n, dtype=np.uint64).astype(np.uint32)
        c[::3] = rng.integers(1 << 30, 3 << 30, len(c[::3]), dtype=np.uint64).astype(np.uint32)
        if n < 64:
            c[:] = 0xC0000000
    else:
        raise KeyError(kind)
    return c.reshape(trows, tpr)


VALUES = ["all zero", "all equal", "all distinct", "one tile holds 99 %", "around the quota", ">= 2^31", "total overflows 32 bits"]
