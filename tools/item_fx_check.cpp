// Host program that drives the planner of a join call with a chain per item (fish-tts_amd/csrc/item_fx.h: the order in
// which the chains are judged, every item's output length, the union of the call's tables and buffers) on arrays of exactly
// the stated sizes, so that a build with -fsanitize=address,undefined sees any read or write past them and any overflow.
// No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/item_fx_check.cpp -o item_fx_check
// Exit status 0 and "item_fx_check: ok" when every expectation holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <vector>

#include "../fish-tts_amd/csrc/item_fx.h"

using ft::chain::FxDesc;

static int failures = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);       \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static const int RATES[] = {44100, 16000, 48000, 8000, 22050};
static const int SPEEDS[] = {100, 50, 200, 80, 150, 125};
static const int CENTS[] = {0, 300, -200, 1200, -1200, 1};
static const int LEVELS[] = {0, -2300, -1600, -5000, -500};

// A chain the stage takes: a pair outside [0.5, 2] falls back to the plain pace.
static ft_item_fx good_fx() {
    ft_item_fx f{SPEEDS[rnd() % 6], CENTS[rnd() % 6], LEVELS[rnd() % 5]};
    if (!ft::chain::fx_plan(f.speed_pct, f.pitch_cents, nullptr)) f.speed_pct = 100;
    return f;
}

static void accepted() {
    for (int B = 1; B <= ft::JOIN_MAX_ITEMS; ++B) {       // heap arrays of exactly B entries
        const int rate = RATES[rnd() % 5], T = 1 + (int)(rnd() % 40), frame_len = B % 2 ? 32 : 2048;
        std::vector<ft_item_fx> fx(B);
        std::vector<FxDesc> d(B);
        std::vector<int32_t> lens(B);
        std::vector<int64_t> n(B);
        for (int b = 0; b < B; ++b) {
            fx[b] = good_fx();
            lens[b] = (int32_t)(rnd() % (unsigned)(T + 1));
        }
        const ft::ItemFxBad r = ft::item_fx_make(rate, fx.data(), B, d.data());
        EXPECT(r.bad == FxDesc::OK && r.item == -1);
        int64_t frames = -1, want_frames = 0;
        EXPECT(ft::item_fx_lens(d.data(), B, T, lens.data(), frame_len, n.data(), &frames) == nullptr);
        std::set<int> cents;
        int levelled = 0;
        size_t hops = 0;
        bool ps = false, ts = false;
        for (int b = 0; b < B; ++b) {
            want_frames += lens[b];
            // the item's length is that of a call with this one chain: ceil(100 n / pct), then ceil(n L / M)
            int L = 1, M = 1, K = 0;
            EXPECT(ft::chain::rs_design(rate, &L, &M, &K, nullptr) == nullptr);
            const long long t = ft::chain::ts_len(fx[b].speed_pct, (long long)lens[b] * frame_len);
            EXPECT(n[b] == (t * L + M - 1) / M);
            EXPECT(d[b].pct == fx[b].speed_pct && d[b].cents == fx[b].pitch_cents && d[b].level == fx[b].loudness && d[b].rate == rate);
            if (fx[b].pitch_cents) cents.insert(fx[b].pitch_cents);
            ps = ps || fx[b].pitch_cents != 0;
            ts = ts || fx[b].speed_pct != 100;
            if (fx[b].loudness) {
                ++levelled;
                hops += (size_t)((n[b] + rate / 10 - 1) / (rate / 10));
            }
        }
        EXPECT(frames == want_frames);
        const ft::ItemFxUnion u = ft::item_fx_union(d.data(), B, n.data());
        EXPECT(u.ncents == (int)cents.size() && u.ps == ps && u.ts == ts && u.rs == (rate != 44100));
        for (int k = 0; k < u.ncents; ++k) EXPECT(cents.count(u.cents[k]) == 1);
        EXPECT(u.levelled == levelled && u.hops == hops);
        for (int k = 0; k < u.levelled; ++k) {
            EXPECT(u.lv[k] >= 0 && u.lv[k] < B && fx[u.lv[k]].loudness != 0);
            EXPECT(k == 0 || u.lv[k] > u.lv[k - 1]);
        }
        const ft::ItemFxUnion v = ft::item_fx_union(d.data(), B, nullptr);       // without lengths: no hops, the rest the same
        EXPECT(v.hops == 0 && v.levelled == u.levelled && v.ncents == u.ncents && v.ps == u.ps && v.ts == u.ts && v.rs == u.rs);
        // lens null: T frames each
        EXPECT(ft::item_fx_lens(d.data(), B, T, nullptr, frame_len, n.data(), &frames) == nullptr && frames == (int64_t)B * T);
        // a length outside [0, T], anywhere
        const int at = (int)(rnd() % (unsigned)B);
        lens[at] = T + 1;
        EXPECT(ft::item_fx_lens(d.data(), B, T, lens.data(), frame_len, n.data(), nullptr) != nullptr);
        lens[at] = -1;
        EXPECT(ft::item_fx_lens(d.data(), B, T, lens.data(), frame_len, n.data(), nullptr) != nullptr);
    }
}

static void refused() {
    struct Case { ft_item_fx fx; FxDesc::Bad bad; };
    const Case cases[] = {{{49, 0, 0}, FxDesc::SPEED},       {{201, 0, 0}, FxDesc::SPEED},     {{100, 1201, 0}, FxDesc::CENTS},
                          {{100, -1201, 0}, FxDesc::CENTS},  {{200, -100, 0}, FxDesc::PAIR},   {{50, 100, 0}, FxDesc::PAIR},
                          {{100, 0, -400}, FxDesc::LEVEL},   {{100, 0, -5001}, FxDesc::LEVEL}, {{100, 0, 1}, FxDesc::LEVEL},
                          {{49, 1201, 1}, FxDesc::SPEED},    {{100, 1201, 1}, FxDesc::CENTS},  {{200, -100, 1}, FxDesc::PAIR}};
    for (const Case& c : cases) {
        for (int B = 1; B <= 9; ++B) {
            for (int at = 0; at < B; ++at) {
                std::vector<ft_item_fx> fx(B);
                std::vector<FxDesc> d(B);
                for (int b = 0; b < B; ++b) fx[b] = good_fx();
                fx[at] = c.fx;
                ft::ItemFxBad r = ft::item_fx_make(16000, fx.data(), B, d.data());
                EXPECT(r.bad == c.bad && r.item == at);
                // the first bad item is the one named
                if (at + 1 < B) {
                    fx[B - 1] = cases[0].fx;
                    r = ft::item_fx_make(16000, fx.data(), B, d.data());
                    EXPECT(r.bad == c.bad && r.item == at);
                }
                // the rate goes first, whatever the items hold
                for (int rate : {7999, 48001, 44101, 0, -1}) {
                    r = ft::item_fx_make(rate, fx.data(), B, d.data());
                    EXPECT(r.bad == FxDesc::RATE && r.item == -1 && r.why != nullptr);
                }
            }
        }
    }
    // no item at all: only the rate is judged, and nothing is read
    EXPECT(ft::item_fx_make(44100, nullptr, 0, nullptr).bad == FxDesc::OK);
    EXPECT(ft::item_fx_make(1, nullptr, 0, nullptr).bad == FxDesc::RATE);
}

int main() {
    accepted();
    refused();
    if (failures) {
        fprintf(stderr, "item_fx_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("item_fx_check: ok\n");
    return 0;
}
