// pyr_walk_host: the register-walking pyrDown (stereo_visual_odometry_amd/csrc/svo_pyr_walk.hpp) run on the host, work item by work
// item, the way the threads of k_pyr_walk run it.  No GPU, no HIP: plain g++.
//
//   pyr_walk_host plan W H PAD ROWS
//       walks the load plan of one level (source W x H, ROWS destination rows per item) and prints one line of integers:
//       items fast_items loads outside_loads min_x max_x min_row max_row dst_uncovered dst_twice l0_uncovered l0_twice
//       (a load = one source byte an item reads; outside = a byte not inside the H rows of W bytes; dst / l0 = ownership of the
//       destination level's and of level 0's pixels: every one must belong to exactly one item)
//   pyr_walk_host run IN OUT W H STRIDE PAD LEVELS
//       IN: H rows of W bytes, STRIDE bytes apart (the last row W bytes long).  Builds level 0 (the copy the ingest form stores) and
//       LEVELS further levels, each from the one below, and writes them packed, one after the other, to OUT.  The caller's image is
//       placed twice: with its last byte flush against an inaccessible page, and with its first byte just behind one — a load
//       outside the image on either side ends the program with a fault instead of going unnoticed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include <vector>
#include "../../stereo_visual_odometry_amd/csrc/svo_pyr_walk.hpp"

template <bool INGEST>
static void level(const uint8_t* src, int ss, int w, int h, int pad, uint8_t* l0, int l0s, uint8_t* dst, int ds) {
    const PwPlan p = pw_plan(w, h, pad, INGEST ? PW_ROWS_INGEST : PW_ROWS);
    for (int i = 0; i < pw_items(p); i++) {
        const PwItem it = pw_item(p, i);
        const int rows = pw_item_rows(p, it);
        if (it.mode == PW_FAST) pw_walk<INGEST, PW_FAST>(src, ss, w, h, l0, l0s, dst, ds, p.w1, it.x0, it.y0, rows);
        else if (it.mode == PW_EDGE) pw_walk<INGEST, PW_EDGE>(src, ss, w, h, l0, l0s, dst, ds, p.w1, it.x0, it.y0, rows);
        else pw_walk<INGEST, PW_TINY>(src, ss, w, h, l0, l0s, dst, ds, p.w1, it.x0, it.y0, rows);
    }
}

static int plan(int w, int h, int pad, int walk) {
    const PwPlan p = pw_plan(w, h, pad, walk);
    long loads = 0, outside = 0; int fast = 0, min_x = 1 << 30, max_x = -(1 << 30), min_r = 1 << 30, max_r = -(1 << 30);
    std::vector<int> dst((size_t)p.w1 * p.h1, 0), l0((size_t)w * h, 0);
    for (int i = 0; i < pw_items(p); i++) {
        const PwItem it = pw_item(p, i);
        const int rows = pw_item_rows(p, it);
        fast += it.fast;
        for (int sy = 2 * it.y0 - 2; sy <= 2 * (it.y0 + rows - 1) + 2; sy++) {
            const int r = pw_reflect101(sy, h);
            for (int k = it.fast ? -3 : 0; k < (it.fast ? PW_LOAD : PW_SPAN); k++) {   // a fast item: the aligned dwords around its span, at any alignment of the row
                const int x = pw_span_byte(p, it, k);
                loads++; outside += x < 0 || x >= w || r < 0 || r >= h;
                if (x < min_x) min_x = x; if (x > max_x) max_x = x; if (r < min_r) min_r = r; if (r > max_r) max_r = r;
            }
        }
        for (int y = it.y0; y < it.y0 + rows; y++) {
            for (int j = 0; j < PW_VEC; j++) if (it.x0 + j >= 0 && it.x0 + j < p.w1) dst[(size_t)y * p.w1 + it.x0 + j]++;
            for (int sy = (y == 0 ? 0 : 2 * y + 1); sy <= 2 * y + 2; sy++)                 // level-0 rows the item stores
                if (sy < h) for (int j = 0; j < 2 * PW_VEC; j++) if (2 * it.x0 + j >= 0 && 2 * it.x0 + j < w) l0[(size_t)sy * w + 2 * it.x0 + j]++;
        }
    }
    long d0 = 0, d2 = 0, z0 = 0, z2 = 0;
    for (int v : dst) { d0 += v == 0; d2 += v > 1; }
    for (int v : l0) { z0 += v == 0; z2 += v > 1; }
    printf("%d %d %ld %ld %d %d %d %d %ld %ld %ld %ld\n", pw_items(p), fast, loads, outside, min_x, max_x, min_r, max_r, d0, d2, z0, z2);
    return 0;
}

// `extent` bytes between two inaccessible pages: flush against the page behind (end = true) or the page in front
static uint8_t* guarded(size_t extent, bool end) {
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE), body = (extent + pg - 1) / pg * pg;
    uint8_t* m = (uint8_t*)mmap(nullptr, body + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == MAP_FAILED) { perror("mmap"); exit(3); }
    mprotect(m, pg, PROT_NONE); mprotect(m + pg + body, pg, PROT_NONE);
    return end ? m + pg + body - extent : m + pg;
}

static int run(const char* in, const char* out, int w, int h, int stride, int pad, int levels) {
    const size_t extent = (size_t)(h - 1) * stride + w;
    std::vector<uint8_t> img(extent);
    FILE* f = fopen(in, "rb");
    if (!f || fread(img.data(), 1, extent, f) != extent) { fprintf(stderr, "cannot read %s\n", in); return 2; }
    fclose(f);
    std::vector<std::vector<uint8_t>> result[2];
    for (int side = 0; side < 2; side++) {
        uint8_t* src = guarded(extent, side == 0);
        memcpy(src, img.data(), extent);
        std::vector<std::vector<uint8_t>>& lv = result[side];
        lv.emplace_back((size_t)w * h, (uint8_t)0xA5);
        int cw = w, ch = h;
        for (int l = 1; l <= levels; l++) {
            const int nw = (cw + 1) / 2, nh = (ch + 1) / 2;
            lv.emplace_back((size_t)nw * nh, (uint8_t)0xA5);
            if (l == 1) level<true>(src, stride, cw, ch, pad, lv[0].data(), cw, lv[1].data(), nw);
            else level<false>(lv[l - 1].data(), cw, cw, ch, pad, nullptr, 0, lv[l].data(), nw);
            cw = nw; ch = nh;
        }
        if (levels == 0) for (int y = 0; y < h; y++) memcpy(&lv[0][(size_t)y * w], src + (size_t)y * stride, w);
    }
    if (result[0] != result[1]) { fprintf(stderr, "the two placements of the image give different levels\n"); return 4; }
    f = fopen(out, "wb");
    if (!f) return 2;
    for (const auto& l : result[0]) fwrite(l.data(), 1, l.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "plan")) return plan(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    if (argc == 9 && !strcmp(argv[1], "run")) return run(argv[2], argv[3], atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]));
    fprintf(stderr, "usage: pyr_walk_host plan W H PAD ROWS | run IN OUT W H STRIDE PAD LEVELS\n");
    return 2;
}
