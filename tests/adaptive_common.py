"""Shared by test_adaptive_host.py and test_gpu_adaptive.py: the numpy side of the definition of adaptive supersampling
(include/hip_wrap_ext.h, clw_ext_set_adaptive).

With factor n and threshold T, the contrast c(p) of pixel p of the packed 1-sample frame B of the launch range is the largest |ch(p) - ch(q)|
over R, G, B and the 4-neighbours q of p inside the range; p is flagged iff c(p) >= T; the range is cut into blocks of b x b pixels, b = 8 / n,
from its first row and column 0, and a block is refined iff one of its pixels is flagged (`refine_mask_np`).  The adaptive frame is the plain
supersampled frame in the refined blocks and B elsewhere (`composite`)."""
import numpy as np

from conftest import CAM
from render_common import rendering, same_floats, take


def contrast_np(xrgb, W, rows):
    """c(p) for every pixel -> int32 [rows, W]"""
    a = np.asarray(xrgb, np.uint32).reshape(rows, W)
    ch = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.int32)
    c = np.zeros((rows, W), np.int32)
    dx = np.abs(ch[:, 1:] - ch[:, :-1]).max(-1)          # between (x, x + 1)
    dy = np.abs(ch[1:] - ch[:-1]).max(-1)                # between (y, y + 1)
    c[:, 1:] = np.maximum(c[:, 1:], dx)
    c[:, :-1] = np.maximum(c[:, :-1], dx)
    c[1:] = np.maximum(c[1:], dy)
    c[:-1] = np.maximum(c[:-1], dy)
    return c


def refine_mask_np(xrgb, W, rows, n, T):
    """-> uint8 [ceil(rows / b), ceil(W / b)], b = 8 / n: 1 = the block holds a pixel whose contrast is >= T"""
    b = 8 // n
    flag = contrast_np(xrgb, W, rows) >= T
    br, bc = -(-rows // b), -(-W // b)
    pad = np.zeros((br * b, bc * b), bool)
    pad[:rows, :W] = flag
    return pad.reshape(br, b, bc, b).any((1, 3)).astype(np.uint8)


def pixel_mask(mask, W, rows, n):
    """the block mask spread over the pixels -> bool [rows * W]"""
    b = 8 // n
    return np.repeat(np.repeat(np.asarray(mask, bool), b, 0), b, 1)[:rows, :W].reshape(-1)


def composite(mask, W, rows, n, base, fine):
    """where(refined, plain supersampled frame, 1-sample frame), for packed [rows * W] or float [rows * W, 3] frames"""
    m = pixel_mask(mask, W, rows, n)
    return np.where(m if base.ndim == 1 else m[:, None], fine, base)


# ---- the adaptive launch and its check (api = the api module; `cam`: the view, conftest.CAM unless given)
def adaptive(R, sc, tex, sky, W, H, depth, strict, n, T, count=1, setup=None, cam=CAM, **kw):
    """`count` adaptive frames in a row from one renderer -> ([(packed, float, mask) ...], flags of the last trace launch)"""
    with rendering(R, sc, tex, sky, W, H, setup=setup, cam=cam, depth=depth, strict=strict, supersample=n, adaptive=T, **kw) as r:
        return take(r, count, extra=lambda r: r.w.read_refine_mask()), r.w.last_trace_flags()


def check_composite(api, ref, got, W, rows, n, T, what):
    """every frame of `got` == where(mask, fine, base) with mask = the host definition on the GPU's own base frame -> the mask"""
    bp, bf, fp, ff, _ = ref
    mask = api.refine_mask(bp, W, rows, n, T)
    want_p, want_f = composite(mask, W, rows, n, bp, fp), composite(mask, W, rows, n, bf, ff)
    for k, (p, f, m) in enumerate(got):
        print(f"{what} frame {k}: {mask.mean() * 100:.1f} % of {mask.size} blocks refined, {int((m != mask.reshape(-1)).sum())} mask bytes differ, "
              f"{int((p != want_p).sum())} packed pixels differ, {int((f.view(np.uint32) != want_f.view(np.uint32)).any(1).sum())} float")
        assert np.array_equal(m, mask.reshape(-1)), (what, k)
        assert np.array_equal(p, want_p), (what, k)
        assert same_floats(f, want_f), (what, k)
    return mask
