// svo_pyr_walk.hpp — the register-walking pyrDown (k_pyr_walk, svo_kernels_img.hip): the work plan (which outputs a thread owns,
// which source bytes it loads) and the walk of one thread.  Written so that plain g++ compiles it too — the two device
// instructions it uses are restated for the host — and a host program (tests/cpp/pyr_walk_host.cpp) can run every work item of a
// level the way the kernel's threads do: the packed arithmetic and the load plan are checked without a GPU.
#pragma once
#include <stdint.h>
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

#define PW_VEC 8                       // consecutive outputs of a destination row a thread owns: one 8-byte store
#define PW_ROWS 8                      // destination rows it walks down, levels >= 2
#define PW_ROWS_INGEST 16              // and in the ingest form (level 1 from the caller's image: 3 of 35 source rows are loaded for the sums alone)
#define PW_SPAN (2 * PW_VEC + 4)       // source bytes of one row it needs: five dwords from column 2 x0 - 2
#define PW_LOAD (PW_SPAN + 4)          // bytes a fast vector loads: the six ALIGNED dwords that hold its span, wherever the row starts

// cv::borderInterpolate(i, n, BORDER_REFLECT_101) for any i (reflect101 of svo_kernels_img.hip)
__host__ __device__ inline int pw_reflect101(int i, int n) {
    if (n <= 1) return 0;
    while ((unsigned)i >= (unsigned)n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

// A destination level of w1 x h1 from a source of w x h (w1 = (w + 1) / 2, h1 = (h + 1) / 2) at border width pad.  Vector v of a
// row starts at x0 = PW_VEC v - (pad & 7): pixel (0, 0) of a stored level sits pad bytes behind a 16-byte boundary, so that origin
// makes the vector's store an aligned 8 bytes.  A vector is FAST where the aligned dwords around its PW_SPAN source bytes lie
// inside the source row whatever the row's own alignment (columns 2 x0 - 5 .. 2 x0 + 21 at the most) — vectors 1 .. n_fast: 16 + 8
// aligned bytes, shifted into place by the address's low bits.  Vector 0 and the last one to three are EDGE vectors: each of the
// five dwords is loaded from the nearest position inside the row (pw_edge_pos) and its bytes are put in place by one v_perm whose
// selector folds the columns (pw_edge_sel) — the only columns outside the row that an output inside the level needs are -2, -1, w
// and w + 1, and their mirror images lie in that dword.  Rows of fewer than four bytes (PW_TINY: never a level of the library) load
// reflected bytes one by one.  Work items: the fast vectors of all row groups first, then the others, so that a wave runs one form.
struct PwPlan { int w, h, w1, h1, c, nv, n_fast, rows, groups; };
enum { PW_FAST = 0, PW_EDGE = 1, PW_TINY = 2 };
struct PwItem { int x0, y0; bool fast; int mode; };
__host__ __device__ inline bool pw_fast(int x0, int w) { return 2 * x0 - 2 >= 3 && 2 * x0 - 2 + PW_LOAD <= w; }
__host__ __device__ inline PwPlan pw_plan(int w, int h, int pad, int rows) {
    PwPlan p;
    p.rows = rows;
    p.w = w; p.h = h; p.w1 = (w + 1) / 2; p.h1 = (h + 1) / 2; p.c = pad & 7;
    p.nv = (p.w1 + p.c + PW_VEC - 1) / PW_VEC;
    p.groups = (p.h1 + rows - 1) / rows;
    const int xl = (w - PW_LOAD + 2) / 2;                              // the largest x0 whose loads end inside the row: 2 x0 - 2 + PW_LOAD <= w
    const int vl = w >= PW_LOAD ? (xl + p.c) / PW_VEC : 0;             // the last fast vector; vector 0 (x0 <= 0) never is one, vector 1 starts at column >= 6
    p.n_fast = vl < p.nv ? vl : p.nv - 1;
    if (p.n_fast < 0) p.n_fast = 0;
    return p;
}
__host__ __device__ inline int pw_items(const PwPlan& p) { return p.nv * p.groups; }
__host__ __device__ inline PwItem pw_item(const PwPlan& p, int i) {
    const int nf = p.n_fast * p.groups;
    int v, g;
    if (i < nf) { g = i / p.n_fast; v = 1 + (i - g * p.n_fast); }
    else { const int ne = p.nv - p.n_fast, j = i - nf; g = j / ne; const int e = j - g * ne; v = e == 0 ? 0 : p.n_fast + e; }
    PwItem it;
    it.x0 = PW_VEC * v - p.c; it.y0 = p.rows * g;
    it.fast = pw_fast(it.x0, p.w);                                   // decided from the bytes, not from the item's place in the list
    it.mode = it.fast ? PW_FAST : p.w >= 4 ? PW_EDGE : PW_TINY;
    return it;
}
// the source rows an item loads: 2 y0 - 2 .. 2 (y0 + rows - 1) + 2, each at pw_reflect101(row, h)
__host__ __device__ inline int pw_item_rows(const PwPlan& p, const PwItem& it) { const int r = p.h1 - it.y0; return r < p.rows ? r : p.rows; }
// EDGE vectors: where the dword of span columns 4 k .. 4 k + 3 (row columns p = 2 x0 - 2 + 4 k ..) is loaded from, and the v_perm
// selector that puts the loaded bytes where the span wants them: span byte j takes the loaded byte that holds column
// reflect101(p + j), or some byte of the dword where that column is not in it (a column no output inside the level reads)
__host__ __device__ inline int pw_edge_pos(int p, int w) { return p < 0 ? 0 : p > w - 4 ? w - 4 : p; }
__host__ __device__ inline unsigned pw_edge_sel(int p, int w) {
    const int pc = pw_edge_pos(p, w);
    unsigned sel = 0;
    for (int j = 0; j < 4; j++) { int i = pw_reflect101(p + j, w) - pc; i = i < 0 ? 0 : i > 3 ? 3 : i; sel |= (unsigned)i << (8 * j); }
    return sel;
}
// the byte of a source row that column k (0 .. PW_SPAN - 1) of an item's span is loaded from; a fast item loads columns
// k = -3 .. PW_LOAD - 1 of it at the most (the aligned dwords around the span), as they lie
__host__ __device__ inline int pw_span_byte(const PwPlan& p, const PwItem& it, int k) {
    const int x = 2 * it.x0 - 2 + k;
    return it.mode == PW_FAST ? x : it.mode == PW_EDGE ? pw_edge_pos(x - (k & 3), p.w) + (k & 3) : pw_reflect101(x, p.w);
}

// ---- the walk itself (the kernel's comment in svo_kernels_img.hip says what it computes); host-compilable, like the plan ----
typedef unsigned short pw_u2 __attribute__((vector_size(4)));          // two 16-bit lanes: the arithmetic is v_pk_* on the device
struct __attribute__((packed, aligned(1))) PwUD { unsigned v; };       // a dword at any byte address
struct __attribute__((aligned(4))) PwUQ4 { unsigned v[4]; };           // 16 bytes at a 4-byte aligned address
struct __attribute__((aligned(8))) PwUD2 { unsigned x, y; };
struct __attribute__((aligned(4))) PwUD2a4 { unsigned x, y; };         // 8 bytes at a 4-byte aligned address
#if defined(__HIP_DEVICE_COMPILE__)
#define PW_UNROLL _Pragma("unroll")
#define PW_ROLLED _Pragma("unroll 1")
__device__ __forceinline__ unsigned pw_perm(unsigned hi, unsigned lo, unsigned sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
__device__ __forceinline__ unsigned pw_alignbyte(unsigned hi, unsigned lo, unsigned n) { return __builtin_amdgcn_alignbyte(hi, lo, n); }
__device__ __forceinline__ unsigned pw_alignbit(unsigned hi, unsigned lo, unsigned n) { return __builtin_amdgcn_alignbit(hi, lo, n); }
#else
#define PW_UNROLL
#define PW_ROLLED
// v_perm_b32, v_alignbyte_b32 and v_alignbit_b32 restated for the host: selector byte 0 .. 3 picks a byte of lo, 4 .. 7 of hi, 12 gives zero
inline unsigned pw_perm(unsigned hi, unsigned lo, unsigned sel) {
    const unsigned long long both = ((unsigned long long)hi << 32) | lo;
    unsigned r = 0;
    for (int k = 0; k < 4; k++) { const unsigned s = (sel >> (8 * k)) & 255u; r |= (s < 8 ? (unsigned)(both >> (8 * s)) & 255u : s >= 13 ? 255u : 0u) << (8 * k); }
    return r;
}
inline unsigned pw_alignbyte(unsigned hi, unsigned lo, unsigned n) { return (unsigned)(((((unsigned long long)hi) << 32) | lo) >> (8 * (n & 3))); }
inline unsigned pw_alignbit(unsigned hi, unsigned lo, unsigned n) { return (unsigned)(((((unsigned long long)hi) << 32) | lo) >> (n & 31)); }
#endif
#define PW_FN __host__ __device__ inline __attribute__((always_inline))
PW_FN pw_u2 pw_pair(unsigned v) { return __builtin_bit_cast(pw_u2, v); }
struct PwRow { unsigned s[PW_SPAN / 4]; };
struct PwEdge { unsigned sel[PW_SPAN / 4]; };                          // an EDGE vector's selectors: the same for every row
template <int MODE>
PW_FN PwEdge pw_edge(int sx, int w) {
    PwEdge e;
PW_UNROLL
    for (int k = 0; k < PW_SPAN / 4; k++) e.sel[k] = MODE == PW_EDGE ? pw_edge_sel(sx + 4 * k, w) : 0u;
    return e;
}
// a row's span from its byte offset ro inside src (a 32-bit offset beside the base: one address register)
template <int MODE>
PW_FN PwRow pw_load_row(const uint8_t* __restrict__ src, unsigned ro, int sx, int w, const PwEdge& e) {
    PwRow r;
    if constexpr (MODE == PW_FAST) {
        const unsigned mis = ((unsigned)(uintptr_t)src + ro + (unsigned)sx) & 3u, o = ro + (unsigned)sx - mis;   // the span starts mis bytes into an aligned dword
        const PwUQ4 a = *reinterpret_cast<const PwUQ4*>(src + o);
        const PwUD2a4 b = *reinterpret_cast<const PwUD2a4*>(src + (o + 16u));
        const unsigned sh = 8u * mis;
        r.s[0] = pw_alignbit(a.v[1], a.v[0], sh); r.s[1] = pw_alignbit(a.v[2], a.v[1], sh); r.s[2] = pw_alignbit(a.v[3], a.v[2], sh);
        r.s[3] = pw_alignbit(b.x, a.v[3], sh); r.s[4] = pw_alignbit(b.y, b.x, sh);
    } else if constexpr (MODE == PW_EDGE) {
PW_UNROLL
        for (int k = 0; k < PW_SPAN / 4; k++) {
            const unsigned d = reinterpret_cast<const PwUD*>(src + (ro + (unsigned)pw_edge_pos(sx + 4 * k, w)))->v;
            r.s[k] = pw_perm(d, d, e.sel[k]);
        }
    } else {
PW_UNROLL
        for (int k = 0; k < PW_SPAN / 4; k++) r.s[k] = 0;
PW_ROLLED
        for (int k = 0; k < PW_SPAN; k += 4) {                          // a dword per round, shifted in from the top: no indexed registers
            unsigned v = 0;
PW_UNROLL
            for (int j = 0; j < 4; j++) v |= (unsigned)src[ro + (unsigned)pw_reflect101(sx + k + j, w)] << (8 * j);
PW_UNROLL
            for (int q = 0; q + 1 < PW_SPAN / 4; q++) r.s[q] = r.s[q + 1];
            r.s[PW_SPAN / 4 - 1] = v;
        }
    }
    return r;
}
// the horizontal sums of the vector's outputs 2 K and 2 K + 1 as two 16-bit lanes: taps at span bytes 4 K + 0 .. 4 and 4 K + 2 .. 6
template <int K>
PW_FN pw_u2 pw_hpair(const PwRow& r) {
    const unsigned lo = r.s[K], hi = r.s[K + 1];
    const pw_u2 a = pw_pair(pw_perm(hi, lo, 0x0c020c00u)), b = pw_pair(pw_perm(hi, lo, 0x0c030c01u));
    const pw_u2 c = pw_pair(pw_perm(hi, lo, 0x0c040c02u)), e = pw_pair(pw_perm(hi, lo, 0x0c050c03u));
    const pw_u2 f = pw_pair(pw_perm(hi, lo, 0x0c060c04u));
    return (a + f) + (b + e) * (unsigned short)4 + c * (unsigned short)6;
}
PW_FN void pw_hrow(const PwRow& r, pw_u2 (&t)[PW_VEC / 2]) { t[0] = pw_hpair<0>(r); t[1] = pw_hpair<1>(r); t[2] = pw_hpair<2>(r); t[3] = pw_hpair<3>(r); }
// the level-0 bytes 2 x0 .. 2 x0 + 15 of a source row the thread holds (span bytes 2 .. 17)
template <bool FAST>
PW_FN void pw_store_l0(uint8_t* __restrict__ l0, int qo, const PwRow& r, int x, int w) {
    unsigned o[4];
PW_UNROLL
    for (int k = 0; k < 4; k++) o[k] = pw_alignbyte(r.s[k + 1], r.s[k], 2);
    if constexpr (FAST) { PwUQ4 u; u.v[0] = o[0]; u.v[1] = o[1]; u.v[2] = o[2]; u.v[3] = o[3]; *reinterpret_cast<PwUQ4*>(l0 + qo) = u; }
    else {
PW_UNROLL
        for (int j = 0; j < 16; j++) if ((unsigned)(x + j) < (unsigned)w) l0[qo + j] = (uint8_t)(o[j >> 2] >> (8 * (j & 3)));
    }
}
template <bool INGEST, int MODE>
PW_FN void pw_walk(const uint8_t* __restrict__ src, int ss, int w, int h, uint8_t* __restrict__ l0, int l0s,
                   uint8_t* __restrict__ dst, int ds, int w1, int x0, int y0, int rows) {
    constexpr bool FAST = MODE == PW_FAST;
    const int sx = 2 * x0 - 2;
    const PwEdge e = pw_edge<MODE>(sx, w);
    pw_u2 A[PW_VEC / 2], B[PW_VEC / 2], t[PW_VEC / 2];
    PwRow r = pw_load_row<MODE>(src, (unsigned)(pw_reflect101(2 * y0 - 2, h) * ss), sx, w, e);
    pw_hrow(r, A);
    r = pw_load_row<MODE>(src, (unsigned)(pw_reflect101(2 * y0 - 1, h) * ss), sx, w, e);
    pw_hrow(r, t);
PW_UNROLL
    for (int k = 0; k < PW_VEC / 2; k++) A[k] += t[k] * (unsigned short)4;
    r = pw_load_row<MODE>(src, (unsigned)(2 * y0 * ss), sx, w, e);          // row 2 y0 < h: the level has row y0
    if (INGEST && y0 == 0) pw_store_l0<FAST>(l0, 2 * x0, r, 2 * x0, w);
    pw_hrow(r, B);
PW_UNROLL
    for (int k = 0; k < PW_VEC / 2; k++) A[k] += B[k] * (unsigned short)6;
    unsigned dofs = (unsigned)(y0 * ds + x0);
PW_ROLLED
    for (int y = y0; y < y0 + rows; y++) {
        const int yo = 2 * y + 1, ye = 2 * y + 2;
        r = pw_load_row<MODE>(src, (unsigned)(pw_reflect101(yo, h) * ss), sx, w, e);
        if (INGEST && yo < h) pw_store_l0<FAST>(l0, yo * l0s + 2 * x0, r, 2 * x0, w);
        pw_hrow(r, t);
PW_UNROLL
        for (int k = 0; k < PW_VEC / 2; k++) { const pw_u2 o4 = t[k] * (unsigned short)4; A[k] += o4; B[k] += o4; }
        r = pw_load_row<MODE>(src, (unsigned)(pw_reflect101(ye, h) * ss), sx, w, e);
        if (INGEST && ye < h) pw_store_l0<FAST>(l0, ye * l0s + 2 * x0, r, 2 * x0, w);
        pw_hrow(r, t);
        unsigned o[PW_VEC / 2];
PW_UNROLL
        for (int k = 0; k < PW_VEC / 2; k++) {
            o[k] = __builtin_bit_cast(unsigned, (pw_u2)((A[k] + t[k] + (unsigned short)128) >> (unsigned short)8));   // bytes 0 and 2: two outputs
            A[k] = B[k] + t[k] * (unsigned short)6; B[k] = t[k];
        }
        PwUD2 v; v.x = pw_perm(o[1], o[0], 0x06040200u); v.y = pw_perm(o[3], o[2], 0x06040200u);
        if (FAST || (x0 >= 0 && x0 + PW_VEC <= w1)) *reinterpret_cast<PwUD2*>(dst + dofs) = v;
        else {
PW_UNROLL
            for (int j = 0; j < PW_VEC; j++) if ((unsigned)(x0 + j) < (unsigned)w1) dst[(int)dofs + j] = (uint8_t)((j < 4 ? v.x : v.y) >> (8 * (j & 3)));
        }
        dofs += ds;
    }
}
