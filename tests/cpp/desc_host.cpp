// The integer rules of the binary descriptors (stereo_visual_odometry_amd/csrc/svo_desc.hpp) — the text k_track_desc and
// k_describe_points run, compiled here for the host — in a stand-alone program: no GPU, no library, so it can be built with
// -fsanitize=address,undefined and run anywhere (tests/test_descriptor_host.py).
//   * the tables: C[k + 15] = -C[k], S[k + 15] = -S[k], S[7] = S[8], C[0] = 2^14; the pattern's bounds, a != b;
//   * the bin rule on the tie cases of include/svo.h (7, 22, 0), at the moments' extremes, and against a brute-force arg-max;
//   * desc_beats, the comparison the wave's butterfly reduction uses, gives desc_bin's answer in any order of the 30 bins;
//   * every pattern point, and every integer point of norm <= 13, rotated by every bin stays within +-13 (the kernel indexes a 27 x 27
//     plane with it), a rotation by bin 0 is the identity and by bin 15 the point reflection;
//   * the centre rule's rounding and clamp, and REFLECT_101's single reflection, at the ends of their ranges.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "../../stereo_visual_odometry_amd/csrc/svo_desc.hpp"

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

static int brute_bin(int32_t m10, int32_t m01) {
    int best = -1; int64_t top = 0;
    for (int k = SVO_DESC_BINS - 1; k >= 0; k--) {                    // downwards, >=: the smallest maximiser is the last one kept
        const int64_t s = (int64_t)m10 * SVO_DESC_COS[k] + (int64_t)m01 * SVO_DESC_SIN[k];
        if (best < 0 || s >= top) { top = s; best = k; }
    }
    return best;
}
// the bins in the order a butterfly over lanes visits them from lane `start`, reduced with desc_beats
static int butterfly_bin(int32_t m10, int32_t m01, int start) {
    int64_t top[64]; int bin[64];
    for (int l = 0; l < 64; l++) { bin[l] = l < SVO_DESC_BINS ? l : 64 + l; top[l] = desc_score(m10, m01, l < SVO_DESC_BINS ? l : 0); }
    for (int o = 32; o > 0; o >>= 1) {
        int64_t nt[64]; int nb[64];
        for (int l = 0; l < 64; l++) {
            nt[l] = top[l]; nb[l] = bin[l];
            if (desc_beats(top[l ^ o], bin[l ^ o], top[l], bin[l])) { nt[l] = top[l ^ o]; nb[l] = bin[l ^ o]; }
        }
        for (int l = 0; l < 64; l++) { top[l] = nt[l]; bin[l] = nb[l]; }
    }
    for (int l = 0; l < 64; l++) CHECK(bin[l] == bin[start]);
    return bin[start];
}

int main() {
    CHECK(SVO_DESC_COS[0] == 16384 && SVO_DESC_SIN[0] == 0 && SVO_DESC_SIN[7] == SVO_DESC_SIN[8]);
    for (int k = 0; k < 15; k++) CHECK(SVO_DESC_COS[k + 15] == -SVO_DESC_COS[k] && SVO_DESC_SIN[k + 15] == -SVO_DESC_SIN[k]);
    CHECK(sizeof(SVO_BRIEF_PATTERN) == 1024);
    for (int i = 0; i < SVO_BRIEF_TESTS; i++) {
        const int8_t* t = SVO_BRIEF_PATTERN + 4 * i;
        CHECK(t[0] * t[0] + t[1] * t[1] <= 169 && t[2] * t[2] + t[3] * t[3] <= 169);
        CHECK(t[0] != t[2] || t[1] != t[3]);
    }
    // the bin rule
    CHECK(desc_bin(0, 1) == 7 && desc_bin(0, 2000000) == 7);
    CHECK(desc_bin(0, -1) == 22 && desc_bin(0, -2000000) == 22);
    CHECK(desc_bin(0, 0) == 0);
    CHECK(desc_bin(1, 0) == 0 && desc_bin(-1, 0) == 15);
    const int32_t M = (1 << 21) - 1;
    const int32_t vals[] = {-M, -1000003, -4097, -17, -1, 0, 1, 3, 255, 65537, 1999999, M};
    for (int32_t a : vals) for (int32_t b : vals) {
        const int k = desc_bin(a, b);
        CHECK(k == brute_bin(a, b));
        CHECK(k == butterfly_bin(a, b, 0) && k == butterfly_bin(a, b, 41));
        if (a || b) CHECK(desc_bin(-a, -b) == (k + 15) % 30 || desc_score(a, b, k) == desc_score(a, b, (k + 1) % 30));   // a half turn, unless k's maximum is shared
    }
    for (int k = 0; k < SVO_DESC_BINS; k++) CHECK(desc_bin(SVO_DESC_COS[k], SVO_DESC_SIN[k]) == k);
    // the rotation
    int worst = 0;
    for (int b = 0; b < SVO_DESC_BINS; b++) {
        for (int i = 0; i < 2 * SVO_BRIEF_TESTS; i++) {
            int rx, ry;
            desc_rotate(SVO_BRIEF_PATTERN[2 * i], SVO_BRIEF_PATTERN[2 * i + 1], b, rx, ry);
            CHECK(rx >= -SVO_DESC_REACH && rx <= SVO_DESC_REACH && ry >= -SVO_DESC_REACH && ry <= SVO_DESC_REACH);
        }
        for (int y = -13; y <= 13; y++) for (int x = -13; x <= 13; x++) {
            if (x * x + y * y > 169) continue;
            int rx, ry;
            desc_rotate(x, y, b, rx, ry);
            CHECK(rx >= -13 && rx <= 13 && ry >= -13 && ry <= 13);
            const int m = (rx < 0 ? -rx : rx) > (ry < 0 ? -ry : ry) ? (rx < 0 ? -rx : rx) : (ry < 0 ? -ry : ry);
            worst = m > worst ? m : worst;
            if (b == 0) CHECK(rx == x && ry == y);
            if (b == 15) CHECK(rx == -x && ry == -y);
        }
    }
    CHECK(worst == 13);
    // the centre rule and the reflection
    CHECK(desc_centre(0.f, 64) == 0 && desc_centre(-3.7f, 64) == 0 && desc_centre(-0.6f, 64) == 0 && desc_centre(63.f, 64) == 63 && desc_centre(1e9f, 64) == 63);
    CHECK(desc_centre(10.5f, 64) == 11 && desc_centre(10.49f, 64) == 10 && desc_centre(0.49999997f, 64) == 1);      // 0.49999997f + 0.5f rounds to 1.0f in f32
    CHECK(desc_centre(62.5f, 64) == 63 && desc_centre(63.5f, 64) == 63);
    for (int n : {16, 17, 64}) {
        for (int i = -15; i < n + 15; i++) { const int r = desc_reflect(i, n); CHECK(r >= 0 && r < n); }
        CHECK(desc_reflect(-1, n) == 1 && desc_reflect(-15, n) == 15 && desc_reflect(n, n) == n - 2 && desc_reflect(n + 14, n) == n - 16 && desc_reflect(5, n) == 5);
    }
    if (fails == 0) std::printf("DESC HOST OK\n");
    return fails ? 1 : 0;
}
