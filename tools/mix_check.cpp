// Host program that drives the mix stage's host arithmetic (fish-tts_amd/csrc/fx_chain.h, the mx_* block: the hop and the
// timeline, the argument checks in their stated order, mx_duck and the gain table) so that a build with
// -fsanitize=address,undefined sees any read or write past an array and any overflow.  No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/mix_check.cpp -o mix_check
// mx_duck - one pass each way over the nearest active hop - against the rule as fishtts_hip.h writes it, a loop over every
// hop of both windows, on a few thousand random activity patterns (lengths 1 to 700 hops, windows 1 to 500, all depths'
// edge values); the arrays are sized exactly, so a node or a hop outside [0, Nh] is an error the sanitizer reports.
// Exit status 0 and "mix_check: ok" when every expectation holds.
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

// D_k as stated: the largest over every active hop of either window.
static std::vector<int> brute(const std::vector<unsigned char>& act, int depth, int Wa, int Wr) {
    const long long Nh = (long long)act.size();
    std::vector<int> D((size_t)Nh + 1, 0);
    for (long long k = 0; k <= Nh; ++k) {
        long long d = 0;
        for (long long h = k; h <= k + Wa - 1; ++h)
            if (h >= 0 && h < Nh && act[(size_t)h]) d = std::max(d, (long long)depth * (Wa - (h - k)) / Wa);
        for (long long h = k - Wr; h <= k - 1; ++h)
            if (h >= 0 && h < Nh && act[(size_t)h]) d = std::max(d, (long long)depth * (Wr - (k - 1 - h)) / Wr);
        D[(size_t)k] = (int)d;
    }
    return D;
}

static void duck() {
    std::mt19937 rng(20240611u);
    const int DEPTHS[] = {0, 1, 599, 1200, 5999, MX_MAX_DEPTH};
    const int WINS[] = {1, 2, 3, 15, 40, 499, MX_MAX_W};
    for (int it = 0; it < 3000; ++it) {
        const long long Nh = it < 40 ? 1 + it % 4 : 1 + (long long)(rng() % 700);
        const int depth = DEPTHS[rng() % 6], Wa = it % 3 ? WINS[rng() % 7] : 1 + (int)(rng() % MX_MAX_W);
        const int Wr = it % 5 ? WINS[rng() % 7] : 1 + (int)(rng() % MX_MAX_W);
        const unsigned dens = rng() % 5;          // all silent, sparse .. all active
        std::vector<unsigned char> act((size_t)Nh);
        for (auto& a : act) a = dens == 0 ? 0 : dens == 4 ? 1 : (rng() % (dens == 1 ? 60 : dens == 2 ? 8 : 2)) == 0;
        snprintf(where, sizeof where, "it %d Nh %lld depth %d Wa %d Wr %d dens %u", it, Nh, depth, Wa, Wr, dens);
        std::vector<int> D((size_t)Nh + 1, -1);
        mx_duck(act.data(), Nh, depth, Wa, Wr, D.data());
        const std::vector<int> want = brute(act, depth, Wa, Wr);
        EXPECT(D == want);
        for (long long h = 0; h < Nh; ++h)
            if (act[(size_t)h]) EXPECT(D[(size_t)h] == depth && D[(size_t)h + 1] == depth);   // both nodes of an active hop
        for (int d : D) EXPECT(d >= 0 && d <= depth);
    }
    // the statement's own example: one active hop, Wa = 4, Wr = 2, depth 1200
    std::vector<unsigned char> act(10, 0);
    act[5] = 1;
    std::vector<int> D(11, -1);
    mx_duck(act.data(), 10, 1200, 4, 2, D.data());
    EXPECT((D == std::vector<int>{0, 0, 300, 600, 900, 1200, 1200, 600, 0, 0, 0}));
}

static const char* judged(const MxArgs& a, bool* too_long) { return mx_check(a, too_long); }

static void checks() {
    snprintf(where, sizeof where, "checks");
    bool tl = true;
    MxArgs ok;
    ok.rate = 8000; ok.n = 1; ok.attack = 15; ok.release = 40;
    EXPECT(judged(ok, &tl) == nullptr && !tl);
    // each value alone, and the order: a call that is wrong twice is refused for the earlier reason
    struct Bad { const char* word; void (*set)(MxArgs&); bool too_long; };
    const Bad BAD[] = {
        {"sample rate", [](MxArgs& a) { a.rate = 7999; }, false},
        {"n must", [](MxArgs& a) { a.n = 0; }, false},
        {"bed_loudness", [](MxArgs& a) { a.bed_loudness = -499; }, false},
        {"depth", [](MxArgs& a) { a.depth = MX_MAX_DEPTH + 1; }, false},
        {"threshold", [](MxArgs& a) { a.threshold = -1e-9f; }, false},
        {"attack", [](MxArgs& a) { a.attack = 0; }, false},
        {"release", [](MxArgs& a) { a.release = MX_MAX_W + 1; }, false},
        {"lead", [](MxArgs& a) { a.lead = -1; }, false},
        {"tail", [](MxArgs& a) { a.tail = -1; }, false},
        {"fade_in", [](MxArgs& a) { a.fade_in = -1; }, false},
        {"fade_out", [](MxArgs& a) { a.fade_out = -1; }, false},
        {"offset", [](MxArgs& a) { a.offset = -1; }, false},
        {"loop", [](MxArgs& a) { a.loop = 2; }, false},
        {"2^28", [](MxArgs& a) { a.tail = MX_MAX_N; }, true},
    };
    const int NB = (int)(sizeof BAD / sizeof BAD[0]);
    for (int i = 0; i < NB; ++i) {
        MxArgs a = ok;
        BAD[i].set(a);
        const char* why = judged(a, &tl);
        EXPECT(why && strstr(why, BAD[i].word) && tl == BAD[i].too_long);
        for (int j = i + 1; j < NB; ++j) {
            MxArgs b = a;
            BAD[j].set(b);
            const char* both = judged(b, &tl);
            EXPECT(both && strstr(both, BAD[i].word));
        }
    }
    MxArgs a = ok;
    a.threshold = NAN;
    EXPECT(judged(a, &tl) != nullptr);
    a = ok;
    a.threshold = INFINITY; a.depth = 0; a.attack = a.release = MX_MAX_W; a.bed_loudness = -5000; a.loop = 1;
    a.fade_in = a.fade_out = a.offset = INT64_MAX;       // any length: the stage clamps them (f = min(fade, N / 2), offset mod nb)
    a.n = MX_MAX_N - 2; a.lead = a.tail = 1;
    EXPECT(judged(a, &tl) == nullptr);
    a.n = MX_MAX_N + 1; a.lead = a.tail = 0;
    EXPECT(judged(a, &tl) != nullptr && tl);
    a.n = 1; a.lead = INT64_MAX; a.tail = INT64_MAX;     // no overflow on the way to the refusal
    EXPECT(judged(a, &tl) != nullptr && tl);
    // the timeline
    const MxPlan p = mx_plan(8000, 161, 0, 0), q = mx_plan(44100, 1000, 441, 441), r = mx_plan(48000, MX_MAX_N, 0, 0);
    EXPECT(p.H == 160 && p.N == 161 && p.Nh == 2);
    EXPECT(q.H == 882 && q.N == 1882 && q.Nh == 3);
    EXPECT(r.H == 960 && r.Nh == (MX_MAX_N + 959) / 960);
    EXPECT(mx_hop(8000) == 160 && mx_hop(11025) == 220 && mx_hop(22050) == 441);
}

static void table() {
    snprintf(where, sizeof where, "table");
    std::vector<float> T((size_t)MX_MAX_DEPTH + 1, -1.f);
    mx_gains(T.data());
    EXPECT(T[0] == 1.f && T[2000] == 0.1f && T[4000] == 0.01f && T[6000] == 0.001f);
    for (int d = 1; d <= MX_MAX_DEPTH; ++d) EXPECT(T[(size_t)d] <= T[(size_t)d - 1] && T[(size_t)d] > 0.f);
}

int main() {
    duck();
    checks();
    table();
    if (failures) {
        fprintf(stderr, "mix_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("mix_check: ok\n");
    return 0;
}
