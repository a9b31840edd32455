"""Shared by test_overlay_host.py and test_gpu_overlay.py: the selection overlay (include/hip_wrap_ext.h: clw_overlay, clw_host_overlay) restated
in numpy from the rules of the header -- not by calling the C model --, the id fields both files run it on, and the census of which rule fired.

The rules, for pixel p = (x, y) of a width x rows image; sel(p) = ids[p] is one of the listed words; pixels outside the image are absent:
  1. c = frame[p] & 0xFFFFFF
  2. EDGES:   the right neighbour (x + 1 < width) or the one below (y + 1 < rows) has another id -> c = edge_rgb
  3. FILL:    sel(p) -> every channel (c_ch * (256 - a) + t_ch * a + 128) >> 8
  4. OUTLINE: !sel(p) and some present q within `radius` in x and in y has sel(q) -> c = outline_rgb
  5. out[p] = c
`corrupt` names one deliberate mistake; the tests hold that the comparison rejects each:
  "inner"               the band inside the object instead of around it
  "no_round"            >> 8 without the + 128
  "outline_under_fill"  FILL applied after OUTLINE, in the implementation where that order matters: the whole dilated selection takes the
                        outline's colour and the object is left to the FILL that follows (without FILL, or below alpha 256, it shows)
  "fill_first"          FILL before EDGES: a selected boundary pixel loses its tint to the edge colour
  "fill_last"           rules 3 and 4 exchanged as they are written.  NOT a mistake: rule 3 changes selected pixels only and rule 4
                        unselected ones only, so the two commute -- the tests hold that this one is the model, bit for bit."""
import itertools

import numpy as np

OV_OUTLINE, OV_FILL, OV_EDGES = 1, 2, 4
ID_NONE = 0xFFFFFFFF
U32 = np.uint32

# the cases of the unit test (GPU) and of the host comparison: every size x radius x flag word x field x selection
SIZES = [(1, 1), (5, 3), (8, 8), (9, 9), (61, 43), (64, 16), (130, 17)]      # width x rows: one pixel, less than a tile, a tile's height, partial tiles, whole tiles, five tiles across
RADII = [1, 2, 3, 4]
FLAGS = [1, 2, 3, 4, 5, 6, 7]
FIELDS = ["noise3", "corners", "checker", "all", "none", "column"]
SELECTIONS = [1, 64]
ALPHAS = [96, 0, 256, 255, 1]
OUTLINE_RGB, FILL_RGB, EDGE_RGB = 0xFFFF00, 0x2060E0, 0x00FF40


def selection(count):
    """`count` distinct ids to select: a sphere first; with 64 of them a plane, a light, the sky and 60 more spheres, the first and the last of
    which the fields use"""
    if count == 1:
        return np.array([7], U32)
    ids = [7, (1 << 30) | 2, (2 << 30) | 1, ID_NONE] + list(range(100, 100 + count - 5)) + [3]
    assert len(ids) == count == len(set(ids))
    return np.array(ids, U32)


def unselected():
    """ids no selection above lists"""
    return np.array([0, 1, (1 << 30) | 0, (2 << 30) | 0, 0x7FFFFFFF], U32)


def field(name, width, rows, sel, seed=0):
    """An id channel [rows, width] of the named kind; `sel` = the selection it is made for"""
    rng = np.random.default_rng(1000 * seed + 7 * width + rows)
    a, z = sel[0], sel[-1]                      # a selected id: the first and the last word of the list
    off = unselected()
    yy, xx = np.mgrid[0:rows, 0:width]
    if name == "noise3":                        # three values, seeded: a selected one, and two that are not
        return np.array([z, off[0], off[2]], U32)[rng.integers(0, 3, (rows, width))]
    if name == "corners":                       # one selected pixel in each corner and in the centre
        ids = np.full((rows, width), off[1], U32)
        for y, x in ((0, 0), (0, width - 1), (rows - 1, 0), (rows - 1, width - 1), (rows // 2, width // 2)):
            ids[y, x] = a
        return ids
    if name == "checker":
        return np.where((xx + yy) % 2 == 0, a, off[3]).astype(U32)
    if name == "all":                           # every pixel selected, by every listed id in turn
        return sel[(xx + 3 * yy) % len(sel)].astype(U32)
    if name == "none":
        return off[(xx // 3 + yy // 2) % len(off)].astype(U32)
    if name == "column":                        # one pixel wide, all rows: column 32 opens the second 32-pixel tile and crosses every 8-row seam
        ids = np.full((rows, width), off[4], U32)
        ids[:, 32 if width > 33 else width // 2] = z
        return ids
    raise KeyError(name)


def frame_of(width, rows, seed=0):
    """A packed frame with a top byte that is not 0 (rule 1 drops it)"""
    rng = np.random.default_rng(77 + seed + 13 * width + rows)
    return rng.integers(0, 1 << 32, width * rows, dtype=np.uint64).astype(U32)


def _channels(c):
    return np.stack([(c >> U32(16)) & U32(255), (c >> U32(8)) & U32(255), c & U32(255)], -1).astype(np.uint32)


def _pack(ch):
    return (ch[..., 0] << U32(16)) | (ch[..., 1] << U32(8)) | ch[..., 2]


def near_selected(selected, radius):
    """[rows, width] bool: some present pixel within `radius` in x and in y is selected (the pixel itself included)"""
    rows, width = selected.shape
    padded = np.zeros((rows + 2 * radius, width + 2 * radius), bool)
    padded[radius:radius + rows, radius:radius + width] = selected
    near = np.zeros((rows, width), bool)
    for dy, dx in itertools.product(range(2 * radius + 1), repeat=2):
        near |= padded[dy:dy + rows, dx:dx + width]
    return near


def model(frame, ids, width, rows, flags, radius, outline_rgb, fill_rgb, alpha, edge_rgb, sel, corrupt=None):
    """-> (out uint32 [width * rows], census): the overlay by the rules above; census counts, per rule, the pixels it changed and the pixels it
    looked at and left alone"""
    assert flags in range(1, 8) and (not flags & OV_OUTLINE or 1 <= radius <= 4) and (not flags & OV_FILL or 0 <= alpha <= 256) and len(sel) <= 64
    frame = np.asarray(frame, U32).reshape(rows, width)
    ids = np.asarray(ids, U32).reshape(rows, width)
    selected = np.isin(ids, np.asarray(sel, U32)) if len(sel) else np.zeros((rows, width), bool)
    census = dict.fromkeys(("edge_drawn", "edge_flat", "edge_last_column_guard", "fill_drawn", "fill_unselected",
                            "outline_drawn", "outline_far", "outline_on_selected"), 0)
    c = frame & U32(0x00FFFFFF)

    def edges(c):
        differ = np.zeros((rows, width), bool)
        differ[:, :-1] |= ids[:, :-1] != ids[:, 1:]
        differ[:-1, :] |= ids[:-1, :] != ids[1:, :]
        census["edge_drawn"] = int(differ.sum())
        census["edge_flat"] = int((~differ).sum())
        # the last pixel of a row whose successor in memory -- the first pixel of the next row -- has another id, and that is not drawn: the x guard
        wrapped = np.zeros((rows, width), bool)
        wrapped[:-1, -1] = ids[:-1, -1] != ids[1:, 0]
        census["edge_last_column_guard"] = int((wrapped & ~differ).sum())
        return np.where(differ, U32(edge_rgb & 0xFFFFFF), c)

    def fill(c):
        a = np.uint32(alpha)
        ch = (_channels(c) * (np.uint32(256) - a) + _channels(np.full_like(c, fill_rgb & 0xFFFFFF)) * a + np.uint32(0 if corrupt == "no_round" else 128)) >> np.uint32(8)
        census["fill_drawn"] = int(selected.sum())
        census["fill_unselected"] = int((~selected).sum())
        return np.where(selected, _pack(ch).astype(U32), c)

    def outline(c):
        near = near_selected(selected, radius)
        band = near & ~selected
        if corrupt == "inner":                  # the band inside the object instead of around it
            band = selected & near_selected(~selected, radius)
        if corrupt == "outline_under_fill":     # the whole dilated selection painted, the object left to a FILL that comes afterwards
            band = near
        census["outline_drawn"] = int(band.sum())
        census["outline_far"] = int((~near).sum())
        census["outline_on_selected"] = int(selected.sum())
        return np.where(band, U32(outline_rgb & 0xFFFFFF), c)

    order = {None: (edges, fill, outline), "fill_last": (edges, outline, fill), "outline_under_fill": (edges, outline, fill),
             "fill_first": (fill, edges, outline)}.get(corrupt, (edges, fill, outline))
    on = {edges: flags & OV_EDGES, fill: flags & OV_FILL, outline: flags & OV_OUTLINE}
    for rule in order:
        if on[rule]:
            c = rule(c)
    return c.reshape(-1).astype(U32), census


def unit_cases(sizes=SIZES):
    """(width, rows, radius, flags, field name, selection, alpha) of every case, the alpha cycling through ALPHAS"""
    k = 0
    for (width, rows), radius, flags, name, count in itertools.product(sizes, RADII, FLAGS, FIELDS, SELECTIONS):
        yield width, rows, radius, flags, name, selection(count), ALPHAS[k % len(ALPHAS)]
        k += 1


def add_census(total, census):
    for k, v in census.items():
        total[k] = total.get(k, 0) + v
    return total


def assert_every_rule_fired_and_was_skipped(total):
    """no rule of the header passes by never being asked: each changed a pixel somewhere in the run, and left one alone"""
    print("census of the run:", total)
    for k in ("edge_drawn", "edge_flat", "edge_last_column_guard", "fill_drawn", "fill_unselected", "outline_drawn", "outline_far", "outline_on_selected"):
        assert total.get(k, 0) > 0, k
