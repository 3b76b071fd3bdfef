// Host program that drives the stereo mix stage's host arithmetic (fish-tts_amd/csrc/fx_chain.h, the ms_* block: the region
// checks in their stated order and their place among the mix stage's, the region lookup, the pan table, the side selection)
// so that a build with -fsanitize=address,undefined sees any read or write past an array and any overflow.  No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/stereo_check.cpp -o stereo_check
// ms_pan - a binary search of the sorted table - against a walk over every region, at every edge of random tables whose
// arrays are sized exactly, so a region outside [0, R) is an error the sanitizer reports.
// Exit status 0 and "stereo_check: ok" when every expectation holds.
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../fish-tts_amd/csrc/fx_chain.h"

using namespace ft::chain;

static int failures = 0;
static char where[160] = "";
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (failures < 20) fprintf(stderr, "%s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, where); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static MsRegion region(long long a, long long e, int pan) {
    MsRegion g;
    g.a = a; g.e = e; g.pan = pan;
    return g;
}

static int walk(const std::vector<MsRegion>& reg, long long j) {
    for (const MsRegion& g : reg)
        if (g.a <= j && j < g.e) return g.pan;
    return 0;
}

static void lookup() {
    std::mt19937 rng(20241020u);
    for (int it = 0; it < 2000; ++it) {
        const long long n = it < 20 ? 1 + it : 1 + (long long)(rng() % 9000);
        std::vector<MsRegion> reg;
        long long at = 0;
        const unsigned dens = rng() % 4;          // one-frame regions that touch .. sparse long ones
        while (at < n && (long long)reg.size() < MS_MAX_REGIONS) {
            const long long a = at + (dens == 0 ? 0 : (long long)(rng() % (dens == 1 ? 2 : 300)));
            if (a >= n) break;
            const long long e = std::min(n, a + 1 + (dens == 0 ? 0 : (long long)(rng() % (dens == 3 ? 2000 : 5))));
            reg.push_back(region(a, e, (int)(rng() % 201) - 100));
            at = e;
        }
        snprintf(where, sizeof where, "it %d n %lld R %zu dens %u", it, n, reg.size(), dens);
        const MsTable t = {reg.data(), (long long)reg.size()};
        EXPECT(ms_check(t, n) == nullptr);
        for (const MsRegion& g : reg)
            for (long long j : {g.a - 1, g.a, g.e - 1, g.e}) EXPECT(ms_pan(t, j) == walk(reg, j));
        for (long long j : {-1LL, 0LL, n - 1, n, n + 5}) EXPECT(ms_pan(t, j) == walk(reg, j));
        for (int k = 0; k < 50; ++k) {
            const long long j = (long long)(rng() % (unsigned long long)(n + 2)) - 1;
            EXPECT(ms_pan(t, j) == walk(reg, j));
        }
    }
    const MsTable none;
    EXPECT(ms_check(none, 1) == nullptr && ms_pan(none, 0) == 0);
}

static void checks() {
    snprintf(where, sizeof where, "checks");
    std::vector<MsRegion> reg = {region(0, 4, -100), region(4, 5, 100), region(9, 10, 0)};
    MsTable t = {reg.data(), 3};
    EXPECT(ms_check(t, 10) == nullptr);
    EXPECT(strstr(ms_check(t, 9), "outside [0, n)"));                 // e > n
    MsTable null = {nullptr, 1};
    EXPECT(strstr(ms_check(null, 10), "null region table"));
    null.R = MS_MAX_REGIONS + 1;                                       // wrong twice: the null table is named
    EXPECT(strstr(ms_check(null, 10), "null region table"));
    MsTable many = {reg.data(), MS_MAX_REGIONS + 1}, negative = {reg.data(), -1};
    EXPECT(strstr(ms_check(many, 10), "R outside") && strstr(ms_check(negative, 10), "R outside"));   // before any region is read
    auto one = [&](long long a, long long e, int pan, int at) {
        std::vector<MsRegion> r = reg;
        r[(size_t)at] = region(a, e, pan);
        const MsTable q = {r.data(), 3};
        return ms_check(q, 10);
    };
    EXPECT(strstr(one(-1, 4, 0, 0), "out of order"));                  // a < 0
    EXPECT(strstr(one(2, 2, 0, 0), "out of order"));                   // empty
    EXPECT(strstr(one(3, 5, 0, 1), "out of order"));                   // overlaps the one before
    EXPECT(strstr(one(9, 11, 0, 2), "out of order"));                  // e > n
    EXPECT(strstr(one(4, 5, 101, 1), "pan outside") && strstr(one(4, 5, -101, 1), "pan outside"));
    EXPECT(one(4, 9, -100, 1) == nullptr);                             // touching on both sides
    EXPECT(strstr(one(3, 5, 101, 1), "out of order"));                 // wrong twice: the place comes first
    EXPECT(one(INT64_MAX - 1, INT64_MAX, 0, 2) != nullptr);            // no overflow on the way to the refusal
    // 4096 regions of one frame each
    std::vector<MsRegion> full;
    for (int r = 0; r < MS_MAX_REGIONS; ++r) full.push_back(region(r, r + 1, r % 201 - 100));
    const MsTable f = {full.data(), MS_MAX_REGIONS};
    EXPECT(ms_check(f, MS_MAX_REGIONS) == nullptr && ms_check(f, MS_MAX_REGIONS - 1) != nullptr);
    EXPECT(ms_pan(f, 0) == -100 && ms_pan(f, 4095) == 4095 % 201 - 100 && ms_pan(f, 4096) == 0);

    // among the mix stage's checks: behind the rate and n, before bed_loudness
    bool tl = true;
    MxArgs ok;
    ok.rate = 8000; ok.n = 10; ok.attack = 15; ok.release = 40;
    EXPECT(mx_check(ok, &tl, 1, &t) == nullptr && !tl);
    MxArgs a = ok;
    a.n = 9;
    EXPECT(strstr(mx_check(a, &tl, 1, &t), "outside [0, n)") && mx_check(a, &tl) == nullptr);
    a = ok;
    a.rate = 7999;
    EXPECT(strstr(mx_check(a, &tl, 1, &null), "sample rate"));
    a = ok;
    a.n = 0;
    EXPECT(strstr(mx_check(a, &tl, 1, &null), "n must"));
    a = ok;
    a.bed_loudness = -499;
    EXPECT(strstr(mx_check(a, &tl, 1, &null), "null region table") && strstr(mx_check(a, &tl, 1, &t), "bed_loudness"));
    a = ok;
    a.tail = MX_MAX_N;
    EXPECT(strstr(mx_check(a, &tl, 1, &null), "null region table") && !tl);
    EXPECT(strstr(mx_check(a, &tl, 1, &t), "2^28") && tl);
}

static void table() {
    snprintf(where, sizeof where, "table");
    float U[2 * MS_MAX_PAN + 1];
    for (float& u : U) u = -1.f;
    ms_gains(U);
    EXPECT(U[0] == 0.f && U[MS_MAX_PAN] == 1.f && U[2 * MS_MAX_PAN] == 1.f);
    for (int j = 1; j <= 2 * MS_MAX_PAN; ++j) EXPECT(U[j] >= U[j - 1] && U[j] <= 1.f);
    for (int j = 1; j < MS_MAX_PAN; ++j) {
        EXPECT(U[j] == (float)(std::sqrt(2.0) * std::sin(j * M_PI / 400.0)) && U[j] > 0.f && U[j] < 1.f);
        // constant power below the clamp: left^2 + right^2 = 2 for the unclamped pair (q = j - 100: right U[j], left sqrt2 cos)
        const double l = std::sqrt(2.0) * std::cos(j * M_PI / 400.0);
        EXPECT(std::fabs((double)U[j] * U[j] + l * l - 2.0) < 1e-6);
    }
    EXPECT(U[50] == (float)(std::sqrt(2.0) * std::sin(M_PI / 8.0)));
}

static void sides() {
    snprintf(where, sizeof where, "sides");
    MsSides s = ms_sides(-1, 2);
    EXPECT(s.ch[0] == 0 && s.ch[1] == 1 && !s.same);
    s = ms_sides(-1, 6);
    EXPECT(s.ch[0] == 0 && s.ch[1] == 1 && !s.same);
    s = ms_sides(-1, 1);
    EXPECT(s.ch[0] == 0 && s.ch[1] == 0 && s.same);
    s = ms_sides(4, 6);
    EXPECT(s.ch[0] == 4 && s.ch[1] == 4 && s.same);
    s = ms_sides(0, 2);
    EXPECT(s.ch[0] == 0 && s.ch[1] == 0 && s.same);
    for (int channels : {0, -3}) EXPECT(ms_sides(-1, channels).same);          // left to the intake to refuse
    for (int channel : {-2, 9, INT32_MIN, INT32_MAX}) {
        s = ms_sides(channel, 2);
        EXPECT(s.same && s.ch[0] == channel);                                  // ... as these are
    }
}

int main() {
    lookup();
    checks();
    table();
    sides();
    if (failures) {
        fprintf(stderr, "stereo_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("stereo_check: ok\n");
    return 0;
}
