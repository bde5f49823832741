// estep_scan_check.cpp - host check of the E-step's suffix sums of v (estep_body, em_lockstep.inc; no GPU needed).
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -o estep_scan_check tools/estep_scan_check.cpp && ./estep_scan_check
//
// estep_body needs, of each group of 64 bins, the four sums S(l) = v[l] + ... + v[63] that start at a 16-bin boundary
// (l = 0, 16, 32, 48).  It used to take them from a Hillis-Steele scan over the 64 lanes (steps 1, 2, 4, .. 32; in each
// step lane l adds the value of lane l + step if there is one).  It now builds the balanced tree T_r of each row of
// 16 lanes with row-local shifts (steps 1, 2, 4, 8; a lane whose source lies beyond the row adds +0.0) and combines the
// four row heads as S(48) = T3, S(32) = T2 + T3, S(16) = (T1 + T2) + T3, S(0) = (T0 + T1) + (T2 + T3).  This program
// restates both on the host and asserts that the four used lanes agree bit for bit, on random and adversarial groups
// (1e-100 next to 1e3, zeros, denormals, cancelling signs), and replays the carry chain over several groups.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static void hillis_steele(const double *v, double *out) {          // the old scan, all 64 lanes
    double a[64], b[64];
    std::memcpy(a, v, sizeof a);
    for (int step = 1; step < 64; step <<= 1) {
        for (int l = 0; l < 64; ++l) b[l] = (l + step < 64) ? a[l] + a[l + step] : a[l];
        std::memcpy(a, b, sizeof a);
    }
    std::memcpy(out, a, sizeof a);
}

static void four_trees(const double *v, double *s0, double *s16, double *s32, double *s48) {     // the new form
    double a[64], b[64];
    std::memcpy(a, v, sizeof a);
    for (int step = 1; step < 16; step <<= 1) {                   // d_row_shl<step>: row-local, +0.0 beyond the row
        for (int l = 0; l < 64; ++l) b[l] = a[l] + (((l & 15) + step < 16) ? a[l + step] : 0.0);
        std::memcpy(a, b, sizeof a);
    }
    const double T0 = a[0], T1 = a[16], T2 = a[32], T3 = a[48];
    const double S32 = T2 + T3;
    *s48 = T3;
    *s32 = S32;
    *s16 = (T1 + T2) + T3;
    *s0 = (T0 + T1) + S32;
}

static uint64_t bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, sizeof u);
    return u;
}

static int g_fail = 0;
static long g_groups = 0;
static void check_group(const double *v, const char *what) {
    double hs[64], s0, s16, s32, s48;
    hillis_steele(v, hs);
    four_trees(v, &s0, &s16, &s32, &s48);
    const double got[4] = {s0, s16, s32, s48};
    for (int r = 0; r < 4; ++r) {
        if (bits(hs[16 * r]) != bits(got[r])) {
            if (g_fail < 20) std::fprintf(stderr, "FAIL %s: S(%d) scan %a trees %a\n", what, 16 * r, hs[16 * r], got[r]);
            ++g_fail;
        }
    }
    ++g_groups;
}

int main() {
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    std::vector<double> v(64);
    // 1. random magnitudes over the whole exponent range of the values v takes (responsibility x read count)
    for (int it = 0; it < 20000; ++it) {
        for (auto &x : v) x = std::ldexp(uni(rng), (int)(rng() % 700) - 690);
        check_group(v.data(), "random exponents");
    }
    // 2. same magnitude: every addition rounds
    for (int it = 0; it < 20000; ++it) {
        for (auto &x : v) x = 1.0 + uni(rng);
        check_group(v.data(), "same magnitude");
    }
    // 3. adversarial: a tail of 1e-100 next to a head of 1e3, zeros, denormals, one value per group, cancelling signs
    const double pool[] = {0.0, 1e-100, 1e3, 4.9406564584124654e-324, 2.2250738585072014e-308, 1e-16, 1.0, 0.1, 1e300, -0.0};
    for (int it = 0; it < 40000; ++it) {
        const int kind = it % 4;
        for (int l = 0; l < 64; ++l) {
            double x = pool[rng() % 10];
            if (kind == 1) x = (l < (int)(rng() % 64)) ? 1e3 * uni(rng) : 1e-100 * uni(rng);
            if (kind == 2) x = (rng() % 8 == 0) ? pool[rng() % 10] : 0.0;
            if (kind == 3) x = ((rng() & 1) ? 1.0 : -1.0) * pool[rng() % 10];   // (v is never negative; the identity does not care)
            v[l] = x;
        }
        check_group(v.data(), "adversarial");
    }
    for (int one = 0; one < 64; ++one) {
        for (int l = 0; l < 64; ++l) v[l] = (l == one) ? 1e-100 : 0.0;
        check_group(v.data(), "single value");
        for (int l = 0; l < 64; ++l) v[l] = (l < one) ? 1e3 : 1e-100;
        check_group(v.data(), "head and tail");
    }
    // 4. the carry chain over several groups, last group first, as estep_body runs it: Vsuf[b] for every 16-bin boundary
    for (int it = 0; it < 2000; ++it) {
        const int groups = 1 + (int)(rng() % 17);
        std::vector<double> w(64 * groups);
        for (auto &x : w) x = (rng() % 5 == 0) ? 0.0 : std::ldexp(uni(rng), (int)(rng() % 400) - 390);
        double carry_a = 0.0, carry_b = 0.0;
        for (int g = groups - 1; g >= 0; --g) {
            double hs[64], s0, s16, s32, s48;
            hillis_steele(&w[64 * g], hs);
            four_trees(&w[64 * g], &s0, &s16, &s32, &s48);
            const double got[4] = {s0, s16, s32, s48};
            for (int r = 0; r < 4; ++r) {
                if (bits(carry_a + hs[16 * r]) != bits(carry_b + got[r])) {
                    if (g_fail < 20) std::fprintf(stderr, "FAIL carry chain: group %d row %d\n", g, r);
                    ++g_fail;
                }
            }
            carry_a += hs[0];
            carry_b += s0;
            ++g_groups;
        }
    }
    std::printf("estep_scan_check: %ld groups, %d mismatches\n", g_groups, g_fail);
    return g_fail ? 1 : 0;
}
