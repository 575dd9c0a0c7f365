// svo_consolidate.hpp — the rules of the descriptor index's landmark consolidation (include/svo.h, "Landmark consolidation"): a
// call's refusals, which rows are members, the distance and the order behind the medoid, the gate and the arithmetic of the mean
// point, and the layout of the scratch.  Plain C++ that a host compiler takes as it is, like svo_retire.hpp and svo_fuse.hpp, so that
// a stand-alone host program (tests/cpp/consolidate_host.cpp) runs exactly the text the kernels (svo_kernels_consolidate.hip) and
// svo_match_api.hip run.  The medoid is integers only; the gate is f32 and the mean f64 with every operation rounded on its own (the
// translation units that include this are built with -ffp-contract=off).  The table of ids is retire's (svo_retire.hpp: its size,
// its hash, its probe order), the gate fusion's (svo_fuse.hpp: fuse_admits_axis).
#pragma once
#include "svo_fuse.hpp"
#include "svo_retire.hpp"

#if defined(__HIPCC__)
#define SVO_CONS_HD __host__ __device__
#else
#define SVO_CONS_HD
#endif

#define CONS_MAX_VIEWS 64                             // include/svo.h: SVO_CONSOLIDATE_MAX_VIEWS, the views of a group: a wave's lanes
#define CONS_DESC_WORDS 8                             // a descriptor as 32-bit words

// ---- a call's refusals.  The request is svo_consolidate_params field by field; row_hi = -1 is the index's size, as everywhere
struct ConsRequest { int32_t row_lo, row_hi, tag_lo, tag_hi; float radius; };
enum ConsRefusal { CONS_OK = 0, CONS_RANGE, CONS_RADIUS };
static inline ConsRefusal cons_check(ConsRequest& q, int size) {
    if (!fuse_span_ok(q.row_lo, q.row_hi, size)) return CONS_RANGE;
    if (!isfinite(q.radius) || q.radius < 0.f) return CONS_RADIUS;
    return CONS_OK;
}

// ---- rule 1: a row of the scope is a member when it has a point and its tag lies in the window
SVO_CONS_HD static inline bool cons_member(int32_t tag, int32_t tag_lo, int32_t tag_hi) { return retire_tag_selected(tag, tag_lo, tag_hi); }

// ---- rule 2: the views of a group of k members are its last cons_views(k)
SVO_CONS_HD static inline int32_t cons_views(int32_t k) { return k < CONS_MAX_VIEWS ? k : CONS_MAX_VIEWS; }

// ---- rule 3: the search's Hamming distance over 8 words, and the order of two views: the smaller sum, at equal sums the larger row
SVO_CONS_HD static inline int32_t cons_hamming(const uint32_t* a, const uint32_t* b) {
    int32_t d = 0;
    for (int w = 0; w < CONS_DESC_WORDS; w++) d += __builtin_popcount(a[w] ^ b[w]);
    return d;
}
SVO_CONS_HD static inline bool cons_better(int32_t sum_a, int32_t row_a, int32_t sum_b, int32_t row_b) {
    return sum_a < sum_b || (sum_a == sum_b && row_a > row_b);
}

// ---- rule 4: the gate between a view's point p and the medoid's q, and one coordinate of the mean of n_near >= 1 views
SVO_CONS_HD static inline bool cons_near(float px, float py, float pz, float qx, float qy, float qz, float radius) {
    return fuse_admits_axis(px, qx, radius) && fuse_admits_axis(py, qy, radius) && fuse_admits_axis(pz, qz, radius);
}
SVO_CONS_HD static inline float cons_mean(double sum, int32_t n_near) { return (float)(sum / (double)n_near); }

// Rules 3 and 4 for one group as a sequential program runs them: the views in ascending rows (n <= CONS_MAX_VIEWS of them), each a
// row number, 8 descriptor words and a point.  -> the view that is the medoid; xyz: rule 4's point; *n_far: the views not near.
static inline int32_t cons_group_plain(int32_t n, const int32_t* rows, const uint32_t* desc, const float* xyz_in, float radius, float* xyz, int32_t* n_far) {
    int32_t best = 0, best_sum = 0;
    for (int32_t i = 0; i < n; i++) {
        int32_t s = 0;
        for (int32_t j = 0; j < n; j++) s += cons_hamming(desc + CONS_DESC_WORDS * i, desc + CONS_DESC_WORDS * j);
        if (i == 0 || cons_better(s, rows[i], best_sum, rows[best])) { best = i; best_sum = s; }
    }
    const float* q = xyz_in + 3 * best;
    double sum[3] = {0.0, 0.0, 0.0};
    int32_t n_near = 0;
    for (int32_t j = 0; j < n; j++) {
        const float* p = xyz_in + 3 * j;
        if (!cons_near(p[0], p[1], p[2], q[0], q[1], q[2], radius)) continue;
        for (int c = 0; c < 3; c++) sum[c] = sum[c] + (double)p[c];
        n_near++;
    }
    for (int c = 0; c < 3; c++) xyz[c] = cons_mean(sum[c], n_near);
    *n_far = n - n_near;
    return best;
}

// ---- the scratch of one call, in the index's maintenance scratch, every part rounded up to 256 bytes (include/svo.h states `total`
// as the bound): retire's keep flags, ranks and block counts — before the ranks exist their room holds the groups' offsets into the
// member list, one more than the scope's rows, and the block counts' room the sums of that scan — then the table of latest rows,
// the members counted per slot, the member list (a row number per member, group after group) and the bounce buffer of one slab.
struct ConsLayout { size_t keep, rank, counts, table, count, list, bounce, total; };
static inline ConsLayout cons_layout(int32_t scope_rows, int32_t moving_rows, int32_t slab_rows) {
    ConsLayout l;
    const size_t m = (size_t)scope_rows, blocks = (m + RETIRE_BLOCK - 1) / RETIRE_BLOCK;
    const size_t slab = (size_t)(moving_rows < slab_rows ? moving_rows : slab_rows);
    const size_t slots = retire_table_slots(scope_rows);
    l.keep = 0; l.rank = retire_round(m);
    l.counts = l.rank + retire_round(4 * (m + 1));
    l.table = l.counts + retire_round(4 * (blocks + RETIRE_BLOCK + 1));
    l.count = l.table + retire_round(4 * slots);
    l.list = l.count + retire_round(4 * slots);
    l.bounce = l.list + retire_round(4 * m);
    l.total = l.bounce + retire_round(RETIRE_ROW_BYTES * slab);
    return l;
}
