"""Shared by test_ao_host.py and test_gpu_ao.py: the ambient occlusion pass (include/hip_wrap_ext.h: clw_ao, clw_host_ao_dirs, clw_host_ao_open,
clw_host_ao_resolve) restated in numpy -- the direction table in float64, the open-ray count in float32 with one rounding per operation, the
resolve in integers -- and the scenes and synthetic channels both test modules run.

Everything is compared for equality of bits, except the direction table against numpy: 1 float32 ulp per component, because two libms may
differ in the last bit of a double sine or cosine."""
import numpy as np

from example_gui_opencl_raytracer_amd import scene as S

AO_FILTER, AO_COMPOSE = 1, 2
KIND_PLANE, KIND_LIGHT, ID_NONE = 1 << 30, 2 << 30, 0xFFFFFFFF
RAYS = (1, 5, 32)
F = np.float32


# ---- (a) the direction table
def dirs_model(K):
    """float64 [16, K, 3] of the formulas, and its float32 rounding [16, K, 4]"""
    j = np.arange(16, dtype=np.float64)[:, None]
    i = np.arange(K, dtype=np.float64)[None, :]
    ji = np.arange(16)
    rev4 = (((ji & 1) << 3) | ((ji & 2) << 1) | ((ji & 4) >> 1) | ((ji & 8) >> 3)).astype(np.float64)[:, None]
    u1 = (i + (j + 0.5) / 16.0) / K
    s = i * 0.6180339887498949 + rev4 / 16.0
    u2 = s - np.floor(s)
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    l = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u1)], -1)
    l4 = np.zeros((16, K, 4), np.float32)
    l4[..., :3] = l.astype(np.float32)
    return l, l4


def ulps(a, b):
    """distance in float32 ulps between two arrays of finite floats of the same sign pattern (or zero)"""
    ka = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    kb = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    ka = np.where(ka < 0, -(ka & 0x7FFFFFFF), ka)
    kb = np.where(kb < 0, -(kb & 0x7FFFFFFF), kb)
    return np.abs(ka - kb)


# ---- (b) the open rays, float32, one rounding per operation, in the definition's order
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def open_model(point, normal, ids, width, rows, first_row, spheres, planes, K, radius, dirs4):
    """uint8 [width * rows]: the header's rules for every pixel; spheres / planes are scene record arrays (or None)"""
    n_px = width * rows
    o = np.ascontiguousarray(point, F).reshape(n_px, 3)
    n = np.ascontiguousarray(normal, F).reshape(n_px, 3)
    ids = np.ascontiguousarray(ids, np.uint32).reshape(n_px)
    ns, npl = (0 if spheres is None else len(spheres)), (0 if planes is None else len(planes))
    radius = F(radius)
    with np.errstate(all="ignore"):
        sg = np.copysign(F(1), n[:, 2])
        a = F(-1) / (sg + n[:, 2])
        b = n[:, 0] * n[:, 1] * a
        t = np.stack([F(1) + sg * n[:, 0] * n[:, 0] * a, sg * b, -sg * n[:, 0]], -1)
        u = np.stack([b, sg + n[:, 1] * n[:, 1] * a, -n[:, 1]], -1)
        x, y = np.arange(n_px) % width, np.arange(n_px) // width
        j = (x & 3) | (((first_row + y) & 3) << 2)
        l = np.ascontiguousarray(dirs4, F).reshape(16, K, 4)[j]                      # [n_px, K, 4]
        d = t[:, None, :] * l[:, :, 0:1] + u[:, None, :] * l[:, :, 1:2] + n[:, None, :] * l[:, :, 2:3]      # [n_px, K, 3]
        occluded = np.zeros((n_px, K), bool)
        A = _dot(d, d)
        for s in range(ns):
            c = np.asarray(spheres["origin"][s], F)
            r = F(spheres["radius"][s])
            q = np.abs(r * r)
            v = (o - c)[:, None, :]
            C = (_dot(v, v) - q)
            B = _dot(v, d)
            D = B * B + (-(A * C))
            sD = np.sqrt(D)
            t0 = (-B - sD) / A
            tt = np.where(t0 < 0, (-B + sD) / A, t0)
            occluded |= ~(D < 0) & ~(tt <= 0) & (tt <= radius)
        for p in range(npl):
            pn = np.asarray(planes["normal"][p], F)
            p0 = np.asarray(planes["point_in_plane"][p], F)
            num = _dot((p0 - o), pn[None, :])[:, None]
            B = _dot(d, pn[None, None, :])
            tt = num / B
            occluded |= ~(B == 0) & ~(tt <= 0) & (tt <= radius)
    kind, index = ids >> np.uint32(30), ids & np.uint32(0x3FFFFFFF)
    surface = ((kind == 0) & (index < ns)) | ((kind == 1) & (index < npl))
    return np.where(surface, K - occluded.sum(1), K).astype(np.uint8)


# ---- (c) the resolve, integers
def resolve_model(open_u8, ids, frame, width, rows, flags, K, strength):
    cnt = np.ascontiguousarray(open_u8, np.uint8).reshape(rows, width).astype(np.int64)
    idg = np.ascontiguousarray(ids, np.uint32).reshape(rows, width)
    if flags & AO_FILTER:
        S_, m = np.zeros((rows, width), np.int64), np.zeros((rows, width), np.int64)
        ys, xs = np.mgrid[0:rows, 0:width]
        for dy in (-2, -1, 0, 1):
            for dx in (-2, -1, 0, 1):
                qy, qx = ys + dy, xs + dx
                present = (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < width)
                qy, qx = np.clip(qy, 0, rows - 1), np.clip(qx, 0, width - 1)
                same = present & (idg[qy, qx] == idg)
                S_ += np.where(same, cnt[qy, qx], 0)
                m += same
    else:
        S_, m = cnt, np.ones((rows, width), np.int64)
    v = (255 * S_ + ((m * K) >> 1)) // (m * K)
    vs = 255 - (((255 - v) * strength + 128) >> 8)
    if flags & AO_COMPOSE:
        f = np.ascontiguousarray(frame, np.uint32).reshape(rows, width).astype(np.int64)
        out = np.zeros((rows, width), np.int64)
        for shift in (0, 8, 16):
            out |= ((((f >> shift) & 255) * vs + 127) // 255) << shift
    else:
        out = vs * 0x010101
    return out.astype(np.uint32).reshape(-1)


RESOLVE_SIZES = [(1, 1), (3, 2), (9, 9), (70, 17)]
STRENGTHS = (0, 1, 255, 256)


def id_field(name, width, rows):
    x, y = np.meshgrid(np.arange(width), np.arange(rows))
    if name == "constant":
        g = np.full((rows, width), 7)
    elif name == "checker":
        g = (x + y) & 1
    else:                      # "column": a new object every third column, one of them the sky
        g = np.where((x // 3) % 4 == 3, ID_NONE, KIND_PLANE | (x // 3))
    return g.astype(np.uint32).reshape(-1)


def resolve_inputs(width, rows, K, seed=0):
    rng = np.random.default_rng(1000 * width + rows + 7 * K + seed)
    return rng.integers(0, K + 1, width * rows).astype(np.uint8), rng.integers(0, 1 << 24, width * rows).astype(np.uint32)


def resolve_cases(sizes):
    """(width, rows, field name, flags, strength, K) of every combination the tests run"""
    return [(w, h, name, flags, strength, K) for (w, h) in sizes for name in ("constant", "checker", "column") for flags in range(4)
            for strength in STRENGTHS for K in RAYS]


# ---- scenes and synthetic channels
def small_scene(spheres=True, planes=True):
    """three spheres over a floor, and a slanted second plane whose normal is NOT unit (the basis takes it as stored)"""
    base = S.render_map_scene()
    sp = base.spheres[:3].copy()
    sp["origin"] = [(0.0, 1.0, 0.0), (1.6, 0.7, 0.4), (-0.9, 0.4, -1.1)]
    sp["radius"] = (1.0, 0.7, -0.4)                      # a negative radius is the sphere of its magnitude
    pl = base.planes[:2].copy()
    pl["normal"] = [(0.0, 1.0, 0.0), (-1.5, 0.5, 0.0)]
    pl["point_in_plane"] = [(0.0, 0.0, 0.0), (3.0, 0.0, 0.0)]
    return S.Scene(sp[:3 if spheres else 0], pl[:2 if planes else 0], base.lights)


def channels(scene, width, rows, seed, odd_normals=True):
    """Synthetic point / normal / id channels for a scene: points on the primitives (offset along the normal, as the primary-hit pass offsets
    them) and between them, normals from the primitive and from a random unit vector; a few sky, light and unknown ids; with `odd_normals`
    a zero and a NaN normal under surface ids.  -> (point [n, 3], normal [n, 3], ids [n])"""
    rng = np.random.default_rng(seed)
    n = width * rows
    sp, pl = scene.spheres, scene.planes
    ns, npl = len(sp), len(pl)
    point, normal, ids = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros(n, np.uint32)
    rnd = rng.normal(size=(n, 3))
    rnd = (rnd / np.linalg.norm(rnd, axis=1, keepdims=True)).astype(F)
    lo = sp["origin"].min(0) - 1 if ns else np.full(3, -3.0)
    hi = sp["origin"].max(0) + 1 if ns else np.full(3, 3.0)
    for p in range(n):
        mode = p % 4
        on_sphere = ns and (not npl or p % 3)
        if mode == 3:                                    # between the primitives
            point[p] = rng.uniform(lo, hi)
            normal[p] = rnd[p]
            ids[p] = int(rng.integers(ns)) if on_sphere else KIND_PLANE | int(rng.integers(npl))
        elif on_sphere:
            i = int(rng.integers(ns))
            nn = rnd[(p * 7 + 3) % n]
            point[p] = sp["origin"][i] + nn * np.abs(sp["radius"][i]) + nn * F(2e-4)
            normal[p] = nn if mode != 2 else rnd[p]
            ids[p] = i
        else:
            i = int(rng.integers(npl))
            pn = pl["normal"][i].astype(F)
            off = np.cross(pn, rnd[p]).astype(F) * F(rng.uniform(0, 3))
            point[p] = pl["point_in_plane"][i] + off + pn * F(2e-4)
            normal[p] = pn if mode != 2 else rnd[p]
            ids[p] = KIND_PLANE | i
    special = rng.permutation(n)[:min(n // 6, 12)]
    for k, p in enumerate(special):
        what = k % 6
        if what == 0:
            ids[p] = ID_NONE
        elif what == 1:
            ids[p] = KIND_LIGHT | 1
        elif what == 2:
            ids[p] = (3 << 30) | 5                       # an unknown word
        elif what == 3:
            ids[p] = (ns + 3) if (k // 6) % 2 else KIND_PLANE | (npl + 1)      # an index past the scene's count
        elif odd_normals and what == 4:
            normal[p] = 0
        elif odd_normals:
            normal[p] = (np.nan, 0.5, 0.5)
    return point, normal, ids
