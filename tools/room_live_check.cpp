// Host program that drives the live room stage's host arithmetic (fish-tts_amd/csrc/fx_chain.h, the rl_* block: the values of
// `begin`, a stream's counters, the bounds of its carry, the per-push checks in their stated order, the buffer sizes and the
// staging's pick of a sent sample) so that a build with -fsanitize=address,undefined sees any read or write past an array and
// any overflow.  No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/room_live_check.cpp -o room_live_check
// Random cuttings of random programmes: the pushes' counts sum to Room's N, every push emits exactly [n_in, n_in + n) and the
// final one the tail behind it, the carry never exceeds predelay + L - 1; a host-side stream over buffers of exactly
// rl_sizes' sizes - the push, its sent form, the output, two copies of the carry - walks the chain with the kernel's pick
// rule (rl_pick) and its roll, on integers, and must give the whole call's convolution with the regions moved to the
// timeline; a refused push changes no counter; the refusals alone and in pairs, the earlier reason winning.
// Exit status 0 and "room_live_check: ok" when every expectation holds.
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

static bool same(const RlStage& a, const RlStage& b) {
    return a.par == b.par && a.ended == b.ended && a.nin == b.nin && a.nout == b.nout && a.base == b.base &&
           a.s.hist == b.s.hist && a.s.tl == b.s.tl;
}

// The values of `begin`: rm_check's order, without n and the regions, the ceiling refused where rm_check judges it.
static void begin() {
    snprintf(where, sizeof where, "begin");
    bool tl = true;
    RmPlan pl;
    RmArgs ok;
    ok.rate = 8000; ok.ir_rate = 44100; ok.ir_frames = 4410; ok.ir_channels = 2; ok.channel = 1; ok.ceiling = 0;
    ok.n = -5;                                                            // (whatever it held: a stream has no n yet)
    const MsTable none = {nullptr, 0};
    EXPECT(rm_check(rl_begin_args(ok), none, &tl, &pl) == nullptr && !tl);
    EXPECT(pl.nh == 800 && pl.L == 800 && pl.tl == 799);
    const RlShape sh = rl_shape(ok, pl);
    EXPECT(sh.hist == 799 && sh.tl == 799);
    RmArgs a = ok;
    a.ceiling = 1;
    const char* why = rm_check(rl_begin_args(a), none, &tl, &pl);
    EXPECT(why && strstr(why, "ceiling must be 0 on a stream") && !tl);
    a.ceiling = 1; a.live = 0;                                            // the whole call keeps its ceiling
    a.n = 10;
    EXPECT(rm_check(a, none, &tl, &pl) == nullptr);
    a = ok; a.ceiling = 2;
    why = rm_check(rl_begin_args(a), none, &tl, &pl);
    EXPECT(why && strstr(why, "ceiling must be 0 or 1"));
    a = ok; a.ceiling = 1; a.send = -2;                                   // send is judged before the ceiling
    why = rm_check(rl_begin_args(a), none, &tl, &pl);
    EXPECT(why && strstr(why, "send neither"));
    a = ok; a.ceiling = 1; a.offset = -1;                                 // ... and the offset behind it
    why = rm_check(rl_begin_args(a), none, &tl, &pl);
    EXPECT(why && strstr(why, "ceiling must be 0 on a stream"));
    a = ok; a.predelay = 8000; a.tail = 3;
    EXPECT(rm_check(rl_begin_args(a), none, &tl, &pl) == nullptr);
    const RlShape s2 = rl_shape(a, pl);
    EXPECT(s2.hist == 8000 + 799 && s2.tl == 3);
    a = ok; a.ir_frames = 44100LL * 20;
    why = rm_check(rl_begin_args(a), none, &tl, &pl);
    EXPECT(why && strstr(why, "131072") && tl);
}

// One random stream: the counters, the carry bound and the integer chain over exactly sized buffers.
static void walk() {
    std::mt19937 rng(20241021u);
    for (int it = 0; it < 400; ++it) {
        const long long L = it % 7 == 0 ? 1 : 1 + (long long)(rng() % 70), predelay = it % 3 == 0 ? 0 : (long long)(rng() % 40);
        const long long hist = predelay + L - 1, tl = it % 4 == 0 ? (long long)(rng() % (unsigned)(hist + 1)) : hist;
        const long long n = it % 11 == 0 ? 0 : (long long)(rng() % 600);
        const int send = it % 5 == 0 ? -1 : it % 5 == 1 ? 3 : 0;
        snprintf(where, sizeof where, "walk it %d L %lld predelay %lld tl %lld n %lld", it, L, predelay, tl, n);
        std::vector<long long> x((size_t)n), h((size_t)L);
        for (auto& v : x) v = (long long)(rng() % 9) - 4;
        for (auto& v : h) v = (long long)(rng() % 5) - 2;
        // the cutting: pushes of random sizes, empty ones among them; the last one final (sometimes an empty one)
        std::vector<long long> cuts;
        for (long long at = 0; at < n;) {
            const unsigned kind = rng() % 6;
            const long long m = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? std::min(n - at, hist + 1 + (long long)(rng() % 50))
                                                                           : std::min(n - at, 1 + (long long)(rng() % 120));
            cuts.push_back(m);
            at += m;
        }
        if (cuts.empty() || rng() % 3 == 0) cuts.push_back(0);
        // every push's regions, relative to it, and the whole call's: the same sends on the timeline
        std::vector<int> want_send((size_t)n, send);
        RlStage st = RlStage::fresh(RlShape{hist, tl});
        std::vector<long long> carry[2] = {std::vector<long long>(rl_sizes(st, st.plan(0, false)).carry),
                                           std::vector<long long>(rl_sizes(st, st.plan(0, false)).carry)};
        std::vector<long long> got;
        long long at = 0, total = 0, largest = 0;
        std::vector<MsRegion> moved;
        for (size_t c = 0; c < cuts.size(); ++c) {
            const long long m = cuts[c];
            const bool final = c + 1 == cuts.size();
            std::vector<MsRegion> reg;
            for (long long a = 0; a < m && reg.size() < 6;) {
                a += rng() % 3 == 0 ? 0 : (long long)(rng() % 30);
                if (a >= m) break;
                const long long e = std::min(m, a + 1 + (long long)(rng() % 60));
                reg.push_back(MsRegion{a, e, rng() % 4 == 0 ? -1 : (int)(rng() % 4), 0});
                a = e;
            }
            const MsTable t = {reg.data(), (long long)reg.size()};
            for (const MsRegion& g : reg) {
                moved.push_back(rl_shift(g, at));
                for (long long j = g.a; j < g.e; ++j) want_send[(size_t)(at + j)] = g.pan;
            }
            bool state, too_long;
            const RlPlan p = st.plan(m, final);
            // a refused push in front of the right one: nothing moves
            const RlStage before = st;
            EXPECT(rl_check(st, m, t, final, p.out - 1, &state, &too_long) != nullptr || p.out == 0);
            EXPECT(rl_check(st, -1, t, final, p.out, &state, &too_long) != nullptr);
            EXPECT(same(st, before));
            EXPECT(rl_check(st, m, t, final, p.out, &state, &too_long) == nullptr && !state && !too_long);
            EXPECT(p.F0 == at && p.F1 == at + m && p.in == m && p.cb0 == st.base);
            EXPECT(p.out == (final ? m + tl : m) && p.end == p.F0 + p.out);
            EXPECT(p.F0 - p.cb0 <= hist && p.F0 - p.cb0 == std::min(at, hist));
            EXPECT(st.held(p) <= hist && (final || st.held(p) == std::min(p.F1, hist)));
            const RlSizes z = rl_sizes(st, p);
            EXPECT(z.carry == (size_t)std::max(hist, 1LL) && z.x >= (size_t)m && z.y >= (size_t)p.out);
            largest = std::max(largest, m);
            std::vector<long long> px(z.x, 0), pxs(z.xs, 0), py(z.y, 0);
            for (long long j = 0; j < m; ++j) {
                px[(size_t)j] = x[(size_t)(at + j)];
                const int s = rm_send(t, j, send);                        // push-relative, as rooml_send_kernel
                pxs[(size_t)j] = s < 0 ? 0 : px[(size_t)j] * (s + 1);     // (an integer stand-in for T[s])
            }
            const std::vector<long long>& cin = carry[st.par];
            std::vector<long long>& cout = carry[st.par ^ 1];
            for (long long i = p.F0; i < p.end; ++i) {
                long long acc = 0;
                for (long long k = 0; k < L; ++k) {
                    const RlPick q = rl_pick(p, i - predelay - k);
                    const long long v = q.buf == 0 ? cin.at((size_t)q.at) : pxs.at((size_t)q.at);   // loaded, then selected
                    acc += h[(size_t)k] * (q.taken ? v : 0);
                }
                py[(size_t)(i - p.F0)] = acc + (i < p.F1 ? 7 * px[(size_t)(i - p.F0)] : 0);
            }
            for (long long i = p.cb1; i < p.F1; ++i) {                    // the roll
                const RlPick q = rl_pick(p, i);
                EXPECT(q.taken);
                cout.at((size_t)(i - p.cb1)) = q.buf == 0 ? cin.at((size_t)q.at) : pxs.at((size_t)q.at);
            }
            got.insert(got.end(), py.begin(), py.begin() + p.out);
            st.commit(p);
            at += m;
            total += p.out;
            EXPECT(st.nin == at && st.nout == total && st.ended == final);
        }
        EXPECT(at == n && total == n + tl && (long long)got.size() == n + tl);
        bool state, too_long;
        const RlStage ended = st;
        const char* why = rl_check(st, 0, MsTable{nullptr, 0}, true, 1 << 20, &state, &too_long);
        EXPECT(why && state && same(st, ended));
        // the whole call: Room's N, the moved regions pass Room's check and give the same sends
        if (n >= 1) {
            EXPECT(rm_regions(MsTable{moved.data(), (long long)moved.size()}, n) == nullptr);
            for (long long j = 0; j < n; ++j) EXPECT(rm_send(MsTable{moved.data(), (long long)moved.size()}, j, send) == want_send[(size_t)j]);
        }
        for (long long i = 0; i < n + tl; ++i) {
            long long acc = 0;
            for (long long k = 0; k < L; ++k) {
                const long long j = i - predelay - k;
                if (j >= 0 && j < n) acc += h[(size_t)k] * (want_send[(size_t)j] < 0 ? 0 : x[(size_t)j] * (want_send[(size_t)j] + 1));
            }
            EXPECT(got[(size_t)i] == acc + (i < n ? 7 * x[(size_t)i] : 0));
        }
    }
}

// The refusals of a push alone and in pairs - the earlier reason wins - and the timeline's limit.
static void refusals() {
    snprintf(where, sizeof where, "refusals");
    RlStage st = RlStage::fresh(RlShape{99, 99});
    st.commit(st.plan(1000, false));
    const RlStage before = st;
    const MsRegion bad_region = {5, 5, 0, 0}, bad_send = {0, 4, RM_MAX_SEND + 1, 0}, outside = {0, 11, 0, 0}, fine = {0, 10, -1, 0};
    bool state, too_long;
    const char* why = rl_check(st, 10, MsTable{&fine, 1}, false, 10, &state, &too_long);
    EXPECT(why == nullptr);
    why = rl_check(st, -1, MsTable{&bad_region, 1}, false, 0, &state, &too_long);
    EXPECT(why && strstr(why, "n must") && !state && !too_long);
    why = rl_check(st, 10, MsTable{&bad_region, 1}, false, 0, &state, &too_long);
    EXPECT(why && strstr(why, "send region") && !state && !too_long);
    why = rl_check(st, 10, MsTable{&outside, 1}, false, 0, &state, &too_long);
    EXPECT(why && strstr(why, "send region"));
    why = rl_check(st, 10, MsTable{&bad_send, 1}, false, 0, &state, &too_long);
    EXPECT(why && strstr(why, "a send neither"));
    why = rl_check(st, 10, MsTable{nullptr, 1}, false, 0, &state, &too_long);
    EXPECT(why && strstr(why, "null region table"));
    why = rl_check(st, 10, MsTable{&fine, MS_MAX_REGIONS + 1}, false, 0, &state, &too_long);
    EXPECT(why && strstr(why, "R outside"));
    why = rl_check(st, MX_MAX_N, MsTable{&bad_region, 1}, false, 0, &state, &too_long);          // a region before the length
    EXPECT(why && strstr(why, "send region") && !too_long);
    why = rl_check(st, MX_MAX_N, MsTable{nullptr, 0}, false, 0, &state, &too_long);              // the length before the capacity
    EXPECT(why && too_long && !state);
    why = rl_check(st, MX_MAX_N - 1000 - 99, MsTable{nullptr, 0}, false, MX_MAX_N, &state, &too_long);   // exactly the limit
    EXPECT(why == nullptr);
    why = rl_check(st, MX_MAX_N - 1000 - 98, MsTable{nullptr, 0}, false, MX_MAX_N, &state, &too_long);
    EXPECT(why && too_long);
    why = rl_check(st, INT64_MAX, MsTable{nullptr, 0}, false, 0, &state, &too_long);             // no overflow on the way
    EXPECT(why && too_long);
    why = rl_check(st, 10, MsTable{nullptr, 0}, false, 9, &state, &too_long);
    EXPECT(why && strstr(why, "capacity") && !state && !too_long);
    why = rl_check(st, 10, MsTable{nullptr, 0}, true, 108, &state, &too_long);
    EXPECT(why && strstr(why, "capacity"));
    why = rl_check(st, 10, MsTable{nullptr, 0}, true, 109, &state, &too_long);
    EXPECT(why == nullptr);
    EXPECT(same(st, before));
    st.commit(st.plan(0, true));
    EXPECT(st.ended && st.nout == 1099);
    why = rl_check(st, -1, MsTable{&bad_region, 1}, false, 0, &state, &too_long);               // the state before everything
    EXPECT(why && state && !too_long);
    // an empty programme: the final push emits the tail alone, and a stream without history carries nothing
    RlStage e = RlStage::fresh(RlShape{0, 0});
    RlPlan p = e.plan(0, true);
    EXPECT(p.out == 0 && rl_sizes(e, p).carry == 1 && rl_sizes(e, p).x == 1 && rl_sizes(e, p).y == 1);
    e = RlStage::fresh(RlShape{12, 5});
    p = e.plan(0, true);
    EXPECT(p.out == 5 && p.F0 == 0 && p.end == 5 && p.cb1 == 0);
    for (long long g = -20; g < 20; ++g) EXPECT(!rl_pick(p, g).taken && rl_pick(p, g).at == 0);
}

int main() {
    begin();
    walk();
    refusals();
    if (failures) {
        fprintf(stderr, "room_live_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("room_live_check: ok\n");
    return 0;
}
