"""Shared by test_objects_host.py and test_gpu_objects.py: the visible-object table (include/hip_wrap_ext.h: clw_object_stat,
clw_host_object_stats) restated in numpy from the words of the header -- np.unique plus masks, not by calling the C model --, the fields and
rectangles both files run it on, and the census of which rule a case exercised.

The rules, for a range of width x rows pixels whose first row is row first_row of the frame, and a rectangle in FRAME pixels (None = all):
  1. the rectangle is clipped to the columns 0 .. width - 1 and the rows first_row .. first_row + rows - 1 (python integers: no overflow)
  2. an id is known if it is ID_NONE, or its kind (id >> 30) is 0..2 and its index (id & 0x3FFFFFFF) is below counts[kind]
  3. one record per distinct known id among the clipped pixels, ascending as uint32: pixels, inclusive box and coordinate sums in frame
     coordinates, the depths whose BIT PATTERNS are smallest / largest (0, 0 without depth)
  4. summary: objects = records, pixels = clipped pixels, foreign = clipped pixels whose id is not known"""
import itertools

import numpy as np

ID_NONE = 0xFFFFFFFF
U32 = np.uint32
OBJECT_STAT = np.dtype([("id", np.uint32), ("pixels", np.uint32), ("x0", np.uint32), ("y0", np.uint32), ("x1", np.uint32), ("y1", np.uint32),
                        ("depth_min", np.float32), ("depth_max", np.float32), ("sum_x", np.uint64), ("sum_y", np.uint64)])
FIELD_ORDER = ["id", "pixels", "x0", "y0", "x1", "y1", "depth_min", "depth_max", "sum_x", "sum_y"]

# the cases of the unit test (GPU) and of the host comparison: every size x first row x rectangle x field
SIZES = [(1, 1), (5, 3), (31, 7), (33, 9), (61, 43), (130, 17)]     # width x rows: one pixel, less than a tile, one short of / one beyond a 32 x 8 tile both ways, partial tiles, five tiles across
FIRST_ROWS = [0, 8, 13]
RECTS = ["whole", "null", "corner", "interior", "inside", "beyond", "huge", "below"]
FIELDS = ["one", "checker", "vstripes", "hstripes", "distinct", "kinds", "foreign"]
COUNTS = (8, 2, 3)                                                  # spheres, planes, lights of every field but "distinct"
# the two cases only 64-bit sums pass: (width, rows, first_row)
LARGE = [(8192, 160, 0), (8192, 8, 100000)]
# more than 512 tiles of 32 x 8 (17 x 33 = 561, partial at both edges): the reduce kernel's workgroups then walk a run of tiles each
RUN_SIZE, RUN_FIRST_ROW = (527, 261), 13
RUN_CASES = [(fname, rname) for fname in ("kinds", "foreign", "distinct", "hstripes") for rname in ("null", "inside")]


def make_id(kind, index):
    return U32((kind << 30) | index)


def rect_of(name, width, rows, first_row):
    """(x, y, width, height) in frame pixels, or None"""
    w, h, f = width, rows, first_row
    if name == "null":
        return None
    if name == "whole":
        return (0, f, w, h)
    if name == "corner":                        # one pixel: the last of the range
        return (w - 1, f + h - 1, 1, 1)
    if name == "interior":
        return (w // 2, f + h // 2, 1, 1)
    if name == "inside":                        # edges strictly inside tiles where the range has room for that
        x, y = min(3, w - 1), min(2, h - 1)
        return (x, f + y, max(1, w - x - 2), max(1, h - y - 1))
    if name == "beyond":                        # reaches beyond the frame to the right and below: clipped
        return (w // 3, f + h // 3, w, h + 5)
    if name == "huge":                          # x + width and y + height do not fit 32 bits; starts above the range when the range is a strip
        return (1 if w > 1 else 0, max(f - 3, 0), 0xFFFFFFFF, 0xFFFFFFFF)
    if name == "below":                         # entirely below the range: an empty table, not a refusal
        return (0, f + h, w, 4)
    raise KeyError(name)


def field(name, width, rows, seed=0):
    """-> (ids uint32 [rows, width], counts)"""
    rng = np.random.default_rng(1000 * seed + 7 * width + rows)
    yy, xx = np.mgrid[0:rows, 0:width]
    counts = COUNTS
    if name == "one":                           # one id everywhere: every workgroup hits one slot
        ids = np.full((rows, width), 5, U32)
    elif name == "checker":
        ids = np.where((xx + yy) % 2 == 0, make_id(0, 2), make_id(1, 1)).astype(U32)
    elif name == "vstripes":                    # one pixel wide
        ids = (xx % 7).astype(U32)
    elif name == "hstripes":
        ids = np.array([make_id(0, 0), make_id(1, 0), make_id(2, 2), U32(ID_NONE), make_id(0, 7)], U32)[yy % 5]
    elif name == "distinct":                    # a different id in every pixel
        ids = (yy * width + xx).astype(U32)
        counts = (width * rows, 0, 0)
    elif name == "kinds":                       # all three kinds and the sky
        pool = [make_id(0, i) for i in range(8)] + [make_id(1, i) for i in range(2)] + [make_id(2, i) for i in range(3)] + [U32(ID_NONE)]
        ids = np.array(pool, U32)[rng.integers(0, len(pool), (rows, width))]
    elif name == "foreign":                     # ids that are not known among known ones: index == count of each kind, kind 3 that is not ID_NONE
        pool = [make_id(0, 1), make_id(1, 1), make_id(2, 0), U32(ID_NONE),
                make_id(0, 8), make_id(0, 0x3FFFFFFF), make_id(1, 2), make_id(2, 3), make_id(3, 5), U32(ID_NONE - 1)]
        ids = np.array(pool, U32)[rng.integers(0, len(pool), (rows, width))]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(ids, U32), counts


def depth_field(width, rows, seed=0):
    """distinct positive depths, one of them +inf"""
    rng = np.random.default_rng(31 + seed + 13 * width + rows)
    d = ((1 + rng.permutation(width * rows)) * np.float32(0.37)).astype(np.float32)
    d[rng.integers(0, d.size)] = np.inf
    assert np.unique(d).size == d.size and (d > 0).all()
    return d.reshape(rows, width)


def model(ids, depth, width, rows, counts, first_row=0, rect=None):
    """-> (records OBJECT_STAT [objects], summary dict, census dict)"""
    ids = np.asarray(ids, U32).reshape(rows, width)
    x0, x1, y0, y1 = 0, width, first_row, first_row + rows
    clipped = False
    if rect is not None:
        rx, ry, rw, rh = (int(v) for v in rect)
        assert rw > 0 and rh > 0
        clipped = rx + rw > width or ry < first_row or ry + rh > first_row + rows
        x0, x1, y0, y1 = max(x0, rx), min(x1, rx + rw), max(y0, ry), min(y1, ry + rh)
    empty = np.zeros(0, OBJECT_STAT)
    if x0 >= x1 or y0 >= y1:
        return empty, dict(objects=0, pixels=0, foreign=0), census_of(empty, 0, clipped)
    sub = ids[y0 - first_row:y1 - first_row, x0:x1].reshape(-1)
    yy, xx = (a.reshape(-1).astype(np.uint64) for a in np.mgrid[y0:y1, x0:x1])
    kind, index = sub >> U32(30), sub & U32(0x3FFFFFFF)
    limit = np.array(list(counts) + [0], np.uint64)[kind]
    known = (sub == U32(ID_NONE)) | (index < limit)
    uniq, inv = np.unique(sub[known], return_inverse=True)
    out = np.zeros(uniq.size, OBJECT_STAT)
    out["id"] = uniq
    out["pixels"] = np.bincount(inv, minlength=uniq.size)
    kx, ky = xx[known], yy[known]
    for name, values, fold, start in (("x0", kx, np.minimum, 1 << 40), ("y0", ky, np.minimum, 1 << 40), ("x1", kx, np.maximum, 0), ("y1", ky, np.maximum, 0),
                                      ("sum_x", kx, np.add, 0), ("sum_y", ky, np.add, 0)):
        acc = np.full(uniq.size, start, np.uint64)
        fold.at(acc, inv, values)
        out[name] = acc
    if depth is not None:
        bits = np.ascontiguousarray(depth, np.float32).reshape(rows, width)[y0 - first_row:y1 - first_row, x0:x1].reshape(-1).view(U32)[known]
        lo, hi = np.full(uniq.size, 0xFFFFFFFF, U32), np.zeros(uniq.size, U32)
        np.minimum.at(lo, inv, bits)
        np.maximum.at(hi, inv, bits)
        out["depth_min"], out["depth_max"] = lo.view(np.float32), hi.view(np.float32)
    foreign = int((~known).sum())
    return out, dict(objects=int(uniq.size), pixels=int(sub.size), foreign=foreign), census_of(out, foreign, clipped)


def census_of(records, foreign, clipped):
    n = len(records)
    return dict(foreign_present=int(foreign > 0), foreign_absent=int(foreign == 0), clipped=int(clipped), unclipped=int(not clipped),
                empty=int(n == 0), not_empty=int(n > 0), one_record=int(n == 1), several_records=int(n > 1),
                over_1024_records=int(n > 1024), at_most_1024_records=int(n <= 1024))


def same_records(a, b):
    """np.array_equal on the raw 48-byte records: every field by its bits, depth included"""
    a, b = np.ascontiguousarray(a, OBJECT_STAT), np.ascontiguousarray(b, OBJECT_STAT)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def unit_cases(sizes=SIZES):
    """(width, rows, first_row, rect name, field name, with depth) of every case; depth is left out of one combination per size"""
    for (width, rows), first_row, rname, fname in itertools.product(sizes, FIRST_ROWS, RECTS, FIELDS):
        yield width, rows, first_row, rname, fname, not (fname == "checker" and first_row == 8)


def add_census(total, census):
    for k, v in census.items():
        total[k] = total.get(k, 0) + v
    return total


def assert_every_rule_fired_and_was_skipped(total):
    """no rule passes by never being asked: each held in some case of the run, and did not hold in another"""
    print("census of the run:", total)
    for k in ("foreign_present", "foreign_absent", "clipped", "unclipped", "empty", "not_empty", "one_record", "several_records",
              "over_1024_records", "at_most_1024_records"):
        assert total.get(k, 0) > 0, k
