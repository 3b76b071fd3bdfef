// Host program that drives the live mix stage's host arithmetic (fish-tts_amd/csrc/fx_chain.h: ml_plan, MlStage) so that a build
// with -fsanitize=address,undefined sees any read or write past an array and any overflow.  No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/mix_live_check.cpp -o mix_live_check
// A stage is walked over random cuttings of a programme - empty pushes, an empty first and an empty final push among them - and
// every push is checked against the closed form of "Emission" in fishtts_hip.h, written out here on its own; the ranges a push
// names (new hops, duck nodes, hops of m and Q, limiter nodes, outputs, the two carries) are played on arrays sized exactly, each
// element written once and read only after it was written, so a range that is off by one is an error the sanitizer or an
// expectation reports.  Exit status 0 and "mix_live_check: ok" when every expectation holds.
#include <stdio.h>

#include <random>
#include <vector>

#include "../fish-tts_amd/csrc/fx_chain.h"

using namespace ft::chain;

static int failures = 0;
static char where[200] = "";
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (failures < 20) fprintf(stderr, "%s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, where); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

// "Emission", as the header writes it.
struct Closed { long long hops, ducks, mixed, limits, done; };
static Closed closed(const MlShape& s, long long n_in, bool final) {
    const long long F = s.lead + n_in;
    if (final) {
        const long long N = F + s.tail, Nh = (N + s.H - 1) / s.H;
        return Closed{Nh, Nh + 1, Nh, Nh + 1, N};
    }
    const long long W = F / s.H, E = s.lead + n_in + s.tail - s.fade_out;
    long long ducks = 0;                       // D_k is final for k <= W' - Wa
    for (long long k = 0; k <= W - s.Wa; ++k) ++ducks;
    const long long Wm = std::min(std::max(0LL, W - s.Wa), (E > 0 ? E : 0) / s.H);
    long long limits = 0;                      // L_k is final for k <= Wm - La
    for (long long k = 0; k <= Wm - ML_LA; ++k) ++limits;
    return Closed{W, ducks, Wm, limits, std::max(0LL, Wm - ML_LA) * s.H};
}

static void walk(std::mt19937& rng, int it) {
    static const int HOPS[] = {160, 320, 882, 960};
    MlShape s;
    s.H = HOPS[rng() % 4];
    s.Wa = it % 7 == 0 ? MX_MAX_W : 1 + (int)(rng() % 20);
    s.lead = rng() % 3 == 0 ? 0 : (long long)(rng() % (unsigned)(30 * s.H));
    s.tail = rng() % 3 == 0 ? 0 : (long long)(rng() % (unsigned)(8 * s.H));
    s.fade_out = rng() % 3 == 0 ? 0 : (long long)(rng() % (unsigned)(12 * s.H));
    if (it % 11 == 0) s.fade_out = ML_MAX_FADE;
    const long long n = it % 13 == 0 ? 0 : (long long)(rng() % (unsigned)((s.Wa + 40) * s.H));
    const long long N = s.lead + n + s.tail, Nh = (N + s.H - 1) / s.H;
    snprintf(where, sizeof where, "it %d H %d Wa %d lead %lld tail %lld fade_out %lld n %lld", it, s.H, s.Wa, s.lead, s.tail,
             s.fade_out, n);
    // what the device arrays would hold: 0 unknown, 1 written
    std::vector<unsigned char> act((size_t)Nh, 0), need((size_t)Nh, 0), D((size_t)Nh + 1, 0), L((size_t)Nh + 1, 0), m((size_t)N, 0),
        y((size_t)N, 0);
    MlStage st = MlStage::fresh(s);
    const long long bound = (long long)(s.Wa + ML_LA + 2) * s.H + std::max(0LL, s.fade_out - s.tail);
    long long fed = 0;
    bool final = false;
    int pushes = 0;
    while (!final) {
        long long k = 0;
        const unsigned kind = rng() % 6;
        if (pushes == 0 && it % 2 == 0) k = 0;                       // an empty first push
        else if (kind == 0) k = 0;
        else if (kind == 1) k = 1;
        else if (kind == 2) k = s.H;
        else k = (long long)(rng() % (unsigned)(5 * s.H + 1));
        k = std::min(k, n - fed);
        final = fed + k == n && (it % 3 != 0 || k == 0);               // (it % 3 == 0: the final push is an empty one)
        const MlPlan p = st.plan(k, final);
        const Closed c = closed(s, fed + k, final);
        EXPECT(p.in == k && p.hops == c.hops && p.ducks == c.ducks && p.mixed == c.mixed && p.limits == c.limits && p.done == c.done);
        EXPECT(p.out == c.done - st.done && p.out >= 0);
        EXPECT(p.hops >= st.hops && p.ducks >= st.ducks && p.mixed >= st.mixed && p.limits >= st.limits);
        EXPECT(p.F == s.lead + fed + k && (!final || p.N == N));
        // the carries: the programme from base on covers what the hops not yet mixed read; both are bounded
        EXPECT(p.base >= st.base && p.base <= p.F && p.base >= std::min(s.lead, p.F));
        if (!final) {
            EXPECT(p.base <= std::max(p.mixed * s.H, s.lead));
            EXPECT(p.F - p.done < bound);
            EXPECT(st.held_prog(p) < (long long)(s.Wa + 2) * s.H + std::max(0LL, s.fade_out - s.tail));
            EXPECT(st.held_mix(p) <= (long long)ML_LA * s.H && st.held_mix(p) >= 0);
            EXPECT(st.held(p) == st.held_prog(p) + st.held_mix(p));
        } else {
            EXPECT(st.held(p) == 0);
        }
        // the launches, in their order, on the exact arrays
        for (long long h = st.hops; h < p.hops; ++h) {               // mixl_hop_kernel: reads the programme of hop h
            EXPECT(h * s.H >= std::min(std::max(st.mixed * s.H, 0LL), h * s.H));
            EXPECT(final || (h + 1) * s.H <= p.F);
            EXPECT(!act.at((size_t)h));
            act.at((size_t)h) = 1;
        }
        for (long long q = st.ducks; q < p.ducks; ++q) {             // mixl_node_kernel: the window's flags
            for (long long h = q - 1; h <= q + s.Wa - 1; ++h)
                if (h >= 0 && h < Nh) EXPECT(h >= p.hops ? final : act.at((size_t)h) == 1);
            EXPECT(!final ? q + s.Wa - 1 < p.hops : true);
            EXPECT(!D.at((size_t)q));
            D.at((size_t)q) = 1;
        }
        for (long long h = st.mixed; h < p.mixed; ++h) {             // mixl_sample_kernel: both duck nodes, the programme
            EXPECT(D.at((size_t)h) == 1 && D.at((size_t)h + 1) == 1);
            const long long i0 = h * s.H, i1 = std::min(i0 + s.H, final ? N : i0 + s.H);
            EXPECT(final || i1 <= p.F);
            EXPECT(final || i1 <= s.lead + fed + k + s.tail - s.fade_out);     // below E
            EXPECT(std::max(i0, s.lead) >= std::min(st.base, std::max(i0, s.lead)));
            if (i1 > s.lead && i0 < p.F) EXPECT(std::max(i0, s.lead) >= st.base || st.base >= s.lead + fed);   // carried or new
            for (long long i = i0; i < i1; ++i) {
                EXPECT(!m.at((size_t)i));
                m.at((size_t)i) = 1;
            }
            EXPECT(!need.at((size_t)h));
            need.at((size_t)h) = 1;
        }
        for (long long q = st.limits; q < p.limits; ++q) {           // mixl_limit_kernel: the 30 hops around the node
            for (long long h = q - ML_LR; h <= q + ML_LA - 1; ++h)
                if (h >= 0 && h < Nh) EXPECT(need.at((size_t)h) == 1);
            EXPECT(!L.at((size_t)q));
            L.at((size_t)q) = 1;
        }
        for (long long i = st.done; i < p.done; ++i) {               // mixl_apply_kernel
            EXPECT(m.at((size_t)i) == 1 && L.at((size_t)(i / s.H)) == 1 && L.at((size_t)(i / s.H) + 1) == 1);
            EXPECT(!y.at((size_t)i));
            y.at((size_t)i) = 1;
        }
        if (!final)
            for (long long i = p.done; i < p.mixed * s.H; ++i) EXPECT(m.at((size_t)i) == 1);   // the m carry exists
        st.commit(p);
        fed += k;
        if (++pushes > 100000) { EXPECT(!"the walk does not end"); break; }
    }
    EXPECT(st.ended && st.done == N && st.nin == n);
    for (unsigned char v : y) EXPECT(v == 1);
    for (unsigned char v : L) EXPECT(v == 1);
    for (unsigned char v : D) EXPECT(v == 1);
}

static void examples() {
    snprintf(where, sizeof where, "examples");
    MlShape s;
    s.H = 882; s.Wa = 15;                                            // 44.1 kHz, the default attack
    EXPECT(ml_plan(s, 21 * 882 - 1, false).done == 0 && ml_plan(s, 21 * 882, false).done == 882);
    EXPECT(ml_plan(s, 22 * 882, false).done == 2 * 882);             // 15 + 5 hops behind the last whole one
    s.lead = 3 * 44100;                                              // a lead longer than the hold-back: out before any speech
    EXPECT(ml_plan(s, 0, false).done == (150 - 20) * 882 && ml_plan(s, 0, false).base == s.lead);
    s.fade_out = 44100;                                              // ... but not the samples that may lie in the fade-out
    EXPECT(ml_plan(s, 0, false).done == (100 - 5) * 882);
    s.tail = 44100;
    EXPECT(ml_plan(s, 0, false).done == (150 - 20) * 882);
    const MlPlan f = ml_plan(s, 1, true);
    EXPECT(f.N == 4 * 44100 + 1 && f.done == f.N && f.hops == 201 && f.limits == 202 && f.ducks == 202);
    MlShape z;
    z.H = 160; z.Wa = 1;
    const MlPlan e = ml_plan(z, 0, true);                            // nothing at all: one node, no sample
    EXPECT(e.N == 0 && e.hops == 0 && e.ducks == 1 && e.limits == 1 && e.done == 0);
    z.fade_out = INT64_MAX;                                          // no overflow on the way
    EXPECT(ml_plan(z, 1LL << 28, false).done == 0);
    bool tl = false;
    MxArgs a;
    a.rate = 8000; a.n = 0; a.attack = 15; a.release = 40;
    EXPECT(mx_check(a, &tl) != nullptr && mx_check(a, &tl, 0) == nullptr);   // an empty programme: the live stage alone
    a.n = -1;
    EXPECT(mx_check(a, &tl, 0) != nullptr && !tl);
}

int main() {
    std::mt19937 rng(20241019u);
    for (int it = 0; it < 4000; ++it) walk(rng, it);
    examples();
    if (failures) {
        fprintf(stderr, "mix_live_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("mix_live_check: ok\n");
    return 0;
}
