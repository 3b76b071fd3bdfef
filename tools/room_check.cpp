// Host program that drives the room stage's host arithmetic (fish-tts_amd/csrc/fx_chain.h, the rm_* block: the send regions,
// the argument checks in their stated order, the impulse response's length at the output rate, L, f, the tail rule, N and the
// buffer sizes) so that a build with -fsanitize=address,undefined sees any read or write past an array and any overflow.
// No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/room_check.cpp -o room_check
// rm_send - a binary search over the sorted regions - against a table filled region by region, on random region sets whose
// arrays are sized exactly; rm_check over every refusal alone and in pairs (the earlier reason wins), at the limits and with
// values that would overflow on the way to a refusal; a walk of a host-side convolution over buffers of exactly rm_sizes'
// sizes with the kernel's index rule, so an index outside them is an error the sanitizer reports.
// Exit status 0 and "room_check: ok" when every expectation holds.
#include <stdint.h>
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

static void regions() {
    std::mt19937 rng(20240907u);
    for (int it = 0; it < 2000; ++it) {
        const long long n = it < 20 ? 1 + it : 1 + (long long)(rng() % 5000);
        const int send = (int)(rng() % 3) == 0 ? -1 : (int)(rng() % (RM_MAX_SEND + 1));
        std::vector<MsRegion> reg;
        std::vector<int> want((size_t)n, send);
        long long at = 0;
        while (at < n && reg.size() < 40) {
            const long long a = at + (long long)(rng() % 3 == 0 ? 0 : rng() % 50);      // they may touch
            if (a >= n) break;
            const long long e = std::min(n, a + 1 + (long long)(rng() % 200));
            const int s = (int)(rng() % 4) == 0 ? -1 : (int)(rng() % (RM_MAX_SEND + 1));
            reg.push_back(MsRegion{a, e, s, 0});
            for (long long j = a; j < e; ++j) want[(size_t)j] = s;
            at = e;
        }
        snprintf(where, sizeof where, "regions it %d n %lld R %zu", it, n, reg.size());
        const MsTable t = {reg.data(), (long long)reg.size()};
        EXPECT(rm_regions(t, n) == nullptr);
        for (long long j = 0; j < n; ++j) EXPECT(rm_send(t, j, send) == want[(size_t)j]);
        if (!reg.empty()) {
            std::vector<MsRegion> bad = reg;
            bad.back().e = n + 1;
            EXPECT(rm_regions(MsTable{bad.data(), (long long)bad.size()}, n) != nullptr);
            bad = reg;
            bad[0].pan = RM_MAX_SEND + 1;
            EXPECT(rm_regions(MsTable{bad.data(), (long long)bad.size()}, n) != nullptr);
            bad[0].pan = -2;
            EXPECT(rm_regions(MsTable{bad.data(), (long long)bad.size()}, n) != nullptr);
            bad = reg;
            bad[0].e = bad[0].a;
            EXPECT(rm_regions(MsTable{bad.data(), (long long)bad.size()}, n) != nullptr);
            if (reg.size() > 1) {
                bad = reg;
                std::swap(bad[0], bad[1]);
                EXPECT(rm_regions(MsTable{bad.data(), (long long)bad.size()}, n) != nullptr);
            }
        }
    }
    snprintf(where, sizeof where, "regions: the table itself");
    EXPECT(rm_regions(MsTable{nullptr, 0}, 1) == nullptr);
    EXPECT(rm_regions(MsTable{nullptr, 1}, 1) != nullptr);
    std::vector<MsRegion> many((size_t)MS_MAX_REGIONS + 1);
    for (size_t r = 0; r < many.size(); ++r) many[r] = MsRegion{(long long)r, (long long)r + 1, 0, 0};
    EXPECT(rm_regions(MsTable{many.data(), MS_MAX_REGIONS}, MS_MAX_REGIONS + 1) == nullptr);
    EXPECT(rm_regions(MsTable{many.data(), MS_MAX_REGIONS + 1}, MS_MAX_REGIONS + 1) != nullptr);
    EXPECT(rm_regions(MsTable{many.data(), -1}, 10) != nullptr);
}

static void checks() {
    snprintf(where, sizeof where, "checks");
    bool tl = true;
    RmPlan pl;
    RmArgs ok;
    ok.rate = 8000; ok.n = 100; ok.ir_rate = 44100; ok.ir_frames = 4410; ok.ir_channels = 2; ok.channel = 1;
    const MsTable none = {nullptr, 0};
    EXPECT(rm_check(ok, none, &tl, &pl) == nullptr && !tl);
    EXPECT(pl.nh == 800 && pl.L == 800 && pl.f == 0 && pl.tl == 799 && pl.N == 899 && !pl.send);
    const MsRegion bad_region = {5, 5, 0, 0};
    const MsTable bad_table = {&bad_region, 1};
    struct Bad { const char* word; void (*set)(RmArgs&); bool too_long; bool table; char field; };   // field: pairs that set one value are skipped
    const Bad BAD[] = {
        {"sample rate", [](RmArgs& a) { a.rate = 7999; }, false, false, 0},
        {"n must", [](RmArgs& a) { a.n = 0; }, false, false, 'n'},
        {"send region", [](RmArgs&) {}, false, true, 0},
        {"channel", [](RmArgs& a) { a.channel = 2; }, false, false, 0},
        {"normalize", [](RmArgs& a) { a.normalize = 2; }, false, false, 0},
        {"wet", [](RmArgs& a) { a.wet = RM_MAX_SEND + 1; }, false, false, 0},
        {"dry", [](RmArgs& a) { a.dry = -2; }, false, false, 0},
        {"send neither", [](RmArgs& a) { a.send = -2; }, false, false, 0},
        {"ceiling", [](RmArgs& a) { a.ceiling = -1; }, false, false, 0},
        {"offset must", [](RmArgs& a) { a.offset = -1; }, false, false, 'o'},
        {"length", [](RmArgs& a) { a.length = -1; }, false, false, 0},
        {"fade", [](RmArgs& a) { a.fade = -1; }, false, false, 0},
        {"predelay", [](RmArgs& a) { a.predelay = a.rate + 1LL; }, false, false, 0},
        {"tail must", [](RmArgs& a) { a.tail = -2; }, false, false, 't'},
        {"n exceeds", [](RmArgs& a) { a.n = MX_MAX_N + 1; }, true, false, 'n'},
        {"offset leaves", [](RmArgs& a) { a.offset = 800; }, false, false, 'o'},
        {"131072", [](RmArgs& a) { a.ir_frames = 44100LL * 20; }, true, false, 'o'},
        {"tail beyond", [](RmArgs& a) { a.tail = INT64_MAX; }, false, false, 't'},
        {"n + tail", [](RmArgs& a) { a.n = MX_MAX_N; }, true, false, 'n'},
    };
    const int NB = (int)(sizeof BAD / sizeof BAD[0]);
    for (int i = 0; i < NB; ++i) {
        RmArgs a = ok;
        BAD[i].set(a);
        bool table = BAD[i].table;
        const char* why = rm_check(a, table ? bad_table : none, &tl, &pl);
        snprintf(where, sizeof where, "checks %s", BAD[i].word);
        EXPECT(why && strstr(why, BAD[i].word) && tl == BAD[i].too_long);
        for (int j = i + 1; j < NB; ++j) {
            if (BAD[i].field && BAD[i].field == BAD[j].field) continue;
            RmArgs b = a;
            BAD[j].set(b);
            const char* both = rm_check(b, table || BAD[j].table ? bad_table : none, &tl, &pl);
            EXPECT(both && strstr(both, BAD[i].word));
        }
    }
    snprintf(where, sizeof where, "checks: limits");
    RmArgs a = ok;
    a.wet = a.dry = a.send = RM_MAX_SEND; a.normalize = 0; a.ceiling = 0; a.channel = -1; a.predelay = a.rate;
    a.fade = INT64_MAX; a.length = INT64_MAX; a.offset = 799;           // any fade, any length: the stage clamps them
    EXPECT(rm_check(a, none, &tl, &pl) == nullptr && pl.L == 1 && pl.f == 1 && pl.tl == 8000 && pl.N == 8100 && pl.send);
    a = ok;
    a.dry = -1; a.send = -1; a.length = 10; a.fade = 3; a.predelay = 7; a.tail = 16;
    EXPECT(rm_check(a, none, &tl, &pl) == nullptr && pl.L == 10 && pl.f == 3 && pl.tl == 16 && pl.N == 116 && pl.send);
    a.tail = 17;
    EXPECT(rm_check(a, none, &tl, &pl) != nullptr && !tl);
    a.tail = 0;
    EXPECT(rm_check(a, none, &tl, &pl) == nullptr && pl.N == 100);
    a = ok;
    a.ir_rate = 44100; a.rate = 44100; a.ir_frames = RM_MAX_L;          // exactly the cap
    EXPECT(rm_check(a, none, &tl, &pl) == nullptr && pl.L == RM_MAX_L);
    a.ir_frames = RM_MAX_L + 1;
    EXPECT(rm_check(a, none, &tl, &pl) != nullptr && tl);
    a.length = RM_MAX_L;                                                // ... and a length brings it back
    EXPECT(rm_check(a, none, &tl, &pl) == nullptr && pl.L == RM_MAX_L && pl.nh == RM_MAX_L + 1);
    a.n = MX_MAX_N - RM_MAX_L + 1;
    EXPECT(rm_check(a, none, &tl, &pl) == nullptr && pl.N == MX_MAX_N);
    a.n += 1;
    EXPECT(rm_check(a, none, &tl, &pl) != nullptr && tl);
    // an item the intake will refuse has no length: the checks that need one are passed over
    a = ok;
    a.ir_frames = 0; a.offset = INT64_MAX; a.tail = INT64_MAX;
    EXPECT(rm_check(a, none, &tl, &pl) == nullptr && pl.nh == -1);
    a.ir_frames = 10; a.ir_rate = 7000;
    EXPECT(rm_check(a, none, &tl, &pl) == nullptr && pl.nh == -1);
    a.ir_rate = 44100; a.ir_frames = INT64_MAX;                         // no overflow on the way
    EXPECT(rm_check(a, none, &tl, &pl) == nullptr && pl.nh == -1);
    // a given length (ft_room_plan)
    a = ok;
    a.nh = 5; a.ir_frames = 0;
    EXPECT(rm_check(a, none, &tl, &pl) == nullptr && pl.nh == 5 && pl.N == 104);
    EXPECT(rm_ir_len(48000, 1500, 16000) == 501 && rm_ir_len(44100, 700, 24000) == 381 && rm_ir_len(44100, 700, 44100) == 700);
}

// The kernel's index rule over host buffers of exactly rm_sizes' sizes: output i reads taps [0, L) and the sent programme at
// i - predelay - k where that lies in [0, n); integers, so the sums are exact and equal a plain convolution's.
static void walk() {
    std::mt19937 rng(7u);
    for (int it = 0; it < 60; ++it) {
        RmArgs a;
        a.rate = 8000; a.n = 1 + (long long)(rng() % 300); a.ir_rate = 44100; a.rate = 44100; a.ir_frames = 1 + (long long)(rng() % 90);
        a.offset = (long long)(rng() % (unsigned)a.ir_frames); a.length = (long long)(rng() % 40); a.predelay = (long long)(rng() % 20);
        a.send = it % 2 ? 100 : 0;
        bool tl;
        RmPlan pl;
        snprintf(where, sizeof where, "walk it %d", it);
        EXPECT(rm_check(a, MsTable{nullptr, 0}, &tl, &pl) == nullptr);
        if (it % 3 == 0) {
            a.tail = (long long)(rng() % (unsigned)(pl.tl + 1));
            EXPECT(rm_check(a, MsTable{nullptr, 0}, &tl, &pl) == nullptr);
        }
        const RmSizes z = rm_sizes(a, pl);
        EXPECT(z.x == (size_t)a.n && z.taps == (size_t)pl.L && z.y == (size_t)pl.N && z.blocks == (size_t)((pl.L + 255) / 256));
        EXPECT(z.xs == (pl.send ? (size_t)a.n : 0));
        std::vector<long long> x(z.x), h(z.taps), y(z.y, 0), full((size_t)(a.n + a.predelay + pl.L - 1), 0);
        std::vector<double> e(z.blocks, 0.0);
        for (auto& v : x) v = (long long)(rng() % 9) - 4;
        for (auto& v : h) v = (long long)(rng() % 3) - 1;
        for (long long k = 0; k < pl.L; ++k) e[(size_t)(k / 256)] += (double)(h[(size_t)k] * h[(size_t)k]);
        for (long long i = 0; i < pl.N; ++i)
            for (long long k = 0; k < pl.L; ++k) {
                const long long j = i - a.predelay - k;
                if (j >= 0 && j < a.n) y[(size_t)i] += h[(size_t)k] * x[(size_t)j];
            }
        for (long long j = 0; j < a.n; ++j)
            for (long long k = 0; k < pl.L; ++k) full[(size_t)(j + a.predelay + k)] += h[(size_t)k] * x[(size_t)j];
        for (long long i = 0; i < pl.N; ++i) EXPECT(y[(size_t)i] == full[(size_t)i]);
    }
}

int main() {
    regions();
    checks();
    walk();
    if (failures) {
        fprintf(stderr, "room_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("room_check: ok\n");
    return 0;
}
