/* overlay_host.c -- THE definition of the selection overlay (include/hip_wrap_ext.h: clw_host_overlay), in integers only: the device pass
 * (wt_overlay, whitted_overlay.inc) is held to it bit for bit.  Written for reading, not for speed: one byte of "selected" per pixel, then
 * every pixel on its own, the rules in the header's order. */
#include "overlay_host.h"

#include <stdlib.h>

int wt_overlay_check(const clw_overlay* style, const uint32_t* sel, uint32_t count) {
    if (!style) return 0;
    if (style->flags == 0u || (style->flags & ~CLW_OV_ALL)) return 0;
    if ((style->flags & CLW_OV_OUTLINE) && (style->radius < 1u || style->radius > WT_OV_MAX_RADIUS)) return 0;
    if ((style->flags & CLW_OV_FILL) && style->fill_alpha > 256u) return 0;
    if (count > WT_OV_MAX_SEL || (count > 0u && !sel)) return 0;
    return 1;
}

static uint32_t blend(uint32_t c, uint32_t t, uint32_t a) {
    uint32_t out = 0u;
    for (int shift = 0; shift < 24; shift += 8) {
        const uint32_t cc = (c >> shift) & 255u, tc = (t >> shift) & 255u;
        out |= ((cc * (256u - a) + tc * a + 128u) >> 8) << shift;
    }
    return out;
}

int clw_host_overlay(const uint32_t* frame, const uint32_t* ids, uint32_t width, uint32_t rows, const clw_overlay* style, const uint32_t* sel,
                     uint32_t count, uint32_t* out) {
    if (!wt_overlay_check(style, sel, count) || width == 0u || rows == 0u || !frame || !ids || !out) return 0;
    const size_t n = (size_t)width * rows;
    uint8_t* selected = (uint8_t*)malloc(n);
    if (!selected) return 0;
    for (size_t p = 0; p < n; p++) {
        selected[p] = 0;
        for (uint32_t k = 0; k < count; k++) if (ids[p] == sel[k]) selected[p] = 1;
    }
    const uint32_t flags = style->flags, r = style->radius;
    for (uint32_t y = 0; y < rows; y++) {
        for (uint32_t x = 0; x < width; x++) {
            const size_t p = (size_t)y * width + x;
            uint32_t c = frame[p] & 0x00FFFFFFu;
            if (flags & CLW_OV_EDGES) {
                if ((x + 1u < width && ids[p] != ids[p + 1]) || (y + 1u < rows && ids[p] != ids[p + width])) c = style->edge_rgb & 0x00FFFFFFu;
            }
            if ((flags & CLW_OV_FILL) && selected[p]) c = blend(c, style->fill_rgb, style->fill_alpha);
            if ((flags & CLW_OV_OUTLINE) && !selected[p]) {
                const uint32_t x0 = x > r ? x - r : 0u, x1 = width - 1u - x > r ? x + r : width - 1u;
                const uint32_t y0 = y > r ? y - r : 0u, y1 = rows - 1u - y > r ? y + r : rows - 1u;
                int near = 0;
                for (uint32_t qy = y0; qy <= y1 && !near; qy++)
                    for (uint32_t qx = x0; qx <= x1; qx++)
                        if (selected[(size_t)qy * width + qx]) { near = 1; break; }
                if (near) c = style->outline_rgb & 0x00FFFFFFu;
            }
            out[p] = c;
        }
    }
    free(selected);
    return 1;
}
