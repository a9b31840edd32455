/* objects_host.c -- THE definition of the visible-object table (include/hip_wrap_ext.h: clw_host_object_stats, clw_host_merge_object_stats),
 * in integers only: the device pass (wt_objects_reduce + wt_objects_compact, whitted_objects.inc) is held to it bit for bit.  Written for
 * reading, not for speed: one record per possible id, every pixel of the clipped rectangle folded into its id's record in row order, then the
 * records that saw a pixel copied out in id order. */
#include "objects_host.h"

#include <stdlib.h>
#include <string.h>

int wt_objects_check(const void* ids, uint32_t width, uint32_t rows, uint32_t first_row, const clw_rect* rect, const uint32_t counts[3],
                     const void* summary) {
    if (!ids || !counts || !summary) return 0;
    if (width == 0u || rows == 0u) return 0;
    if (rect && (rect->width == 0u || rect->height == 0u)) return 0;
    if ((uint64_t)counts[0] + counts[1] + counts[2] + 1u > WT_OBJ_MAX_SLOTS) return 0;
    if ((uint64_t)width * rows >= WT_OBJ_MAX_PIXELS) return 0;
    if ((uint64_t)first_row + rows > 0x100000000ull) return 0;
    return 1;
}

int wt_objects_clip(uint32_t width, uint32_t rows, uint32_t first_row, const clw_rect* rect, uint32_t clip[4]) {
    uint64_t x0 = 0u, x1 = width, y0 = first_row, y1 = (uint64_t)first_row + rows;      /* [x0, x1) x [y0, y1) in frame pixels */
    clip[0] = clip[1] = clip[2] = clip[3] = 0u;
    if (rect) {
        const uint64_t rx1 = (uint64_t)rect->x + rect->width, ry1 = (uint64_t)rect->y + rect->height;
        if (rect->x > x0) x0 = rect->x;
        if (rect->y > y0) y0 = rect->y;
        if (rx1 < x1) x1 = rx1;
        if (ry1 < y1) y1 = ry1;
    }
    if (x0 >= x1 || y0 >= y1) return 0;
    clip[0] = (uint32_t)x0; clip[1] = (uint32_t)(y0 - first_row); clip[2] = (uint32_t)(x1 - x0); clip[3] = (uint32_t)(y1 - y0);
    return 1;
}

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* the record's place in id order: spheres, planes, lights, CLW_ID_NONE last; -1 = an id that is not known */
static int64_t slot_of(uint32_t id, const uint32_t counts[3]) {
    const uint32_t kind = id >> 30, index = id & 0x3FFFFFFFu;
    if (id == CLW_ID_NONE) return (int64_t)counts[0] + counts[1] + counts[2];
    if (kind > 2u || index >= counts[kind]) return -1;
    return (int64_t)index + (kind > 0u ? counts[0] : 0u) + (kind > 1u ? counts[1] : 0u);
}

int clw_host_object_stats(const uint32_t* ids, const float* depth, uint32_t width, uint32_t rows, uint32_t first_row, const clw_rect* rect,
                          const uint32_t counts[3], clw_object_stat* out, uint32_t capacity, clw_object_summary* summary) {
    if (!wt_objects_check(ids, width, rows, first_row, rect, counts, summary)) return 0;
    if (!out) capacity = 0u;
    clw_object_summary sum = {0u, 0u, 0u, 0u};
    uint32_t clip[4];
    if (!wt_objects_clip(width, rows, first_row, rect, clip)) { *summary = sum; return 1; }      /* the rectangle misses the range: an empty table */
    const size_t slots = (size_t)counts[0] + counts[1] + counts[2] + 1u;
    clw_object_stat* table = (clw_object_stat*)calloc(slots, sizeof *table);
    if (!table) return 0;
    for (uint32_t ly = clip[1]; ly < clip[1] + clip[3]; ly++) {
        for (uint32_t x = clip[0]; x < clip[0] + clip[2]; x++) {
            const size_t p = (size_t)ly * width + x;
            const uint32_t y = first_row + ly;
            const int64_t slot = slot_of(ids[p], counts);
            sum.pixels++;
            if (slot < 0) { sum.foreign++; continue; }
            clw_object_stat* s = &table[slot];
            const float d = depth ? depth[p] : 0.0f;
            if (s->pixels == 0u) {
                s->id = ids[p];
                s->x0 = s->x1 = x; s->y0 = s->y1 = y;
                s->depth_min = s->depth_max = d;
            }
            s->pixels++;
            if (x < s->x0) s->x0 = x;
            if (x > s->x1) s->x1 = x;
            if (y < s->y0) s->y0 = y;
            if (y > s->y1) s->y1 = y;
            if (bits_of(d) < bits_of(s->depth_min)) s->depth_min = d;
            if (bits_of(d) > bits_of(s->depth_max)) s->depth_max = d;
            s->sum_x += x; s->sum_y += y;
        }
    }
    for (size_t k = 0; k < slots; k++) {
        if (table[k].pixels == 0u) continue;
        if (sum.objects < capacity) out[sum.objects] = table[k];
        sum.objects++;
    }
    free(table);
    *summary = sum;
    return 1;
}

uint32_t clw_host_merge_object_stats(const clw_object_stat* a, uint32_t na, const clw_object_stat* b, uint32_t nb, clw_object_stat* out,
                                     uint32_t capacity) {
    uint32_t i = 0u, j = 0u, n = 0u;
    if (!a) na = 0u;
    if (!b) nb = 0u;
    if (!out) capacity = 0u;
    while (i < na || j < nb) {
        clw_object_stat s;
        if (j >= nb || (i < na && a[i].id < b[j].id)) s = a[i++];
        else if (i >= na || b[j].id < a[i].id) s = b[j++];
        else {      /* one object in both tables */
            const clw_object_stat* t = &b[j++];
            s = a[i++];
            s.pixels += t->pixels;
            if (t->x0 < s.x0) s.x0 = t->x0;
            if (t->y0 < s.y0) s.y0 = t->y0;
            if (t->x1 > s.x1) s.x1 = t->x1;
            if (t->y1 > s.y1) s.y1 = t->y1;
            if (bits_of(t->depth_min) < bits_of(s.depth_min)) s.depth_min = t->depth_min;
            if (bits_of(t->depth_max) > bits_of(s.depth_max)) s.depth_max = t->depth_max;
            s.sum_x += t->sum_x; s.sum_y += t->sum_y;
        }
        if (n < capacity) out[n] = s;
        n++;
    }
    return n;
}
