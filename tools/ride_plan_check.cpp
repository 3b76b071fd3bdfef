// Host program that drives the ride stage's host arithmetic (fish-tts_amd/csrc/fx_chain.h: rd_plan, RdStage and its place in
// StageChain / FxDesc) so that a build with -fsanitize=address,undefined sees any read or write past an array and any
// overflow.  No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ride_plan_check.cpp -o ride_plan_check
// Over five rates, stream lengths around every border of the emission rule and random ones, and random chunkings with empty
// chunks and a tail-only final:
//   every per-call count is >= 0 and the emitted samples sum to n; a stream holds back fewer than (RD_A + 1) H samples and
//   its carry base never moves backwards; hops, peaks and nodes after a call are those of rd_plan over the samples seen, so
//   the plan does not depend on the chunking; rd_plan agrees with the emission rule written out (ft_ride_plan's formula);
//   an absent stage passes its input on; FxDesc judges the target last and keeps the earlier verdicts.
// Exit status 0 and "ride_plan_check: ok" when every expectation holds.
#include <stdio.h>

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

static const int RATES[] = {8000, 11025, 16000, 44100, 48000};

// The emission rule as the header states it, on loose arithmetic.
static void rule(int H, long long n, bool final, long long* nodes, long long* out) {
    if (final) {
        *nodes = (n + H - 1) / H + 1;
        *out = n;
        return;
    }
    const long long w = n / H;
    *nodes = w >= RD_A ? w - RD_A + 1 : 0;
    *out = (w > RD_A ? w - RD_A : 0) * H;
}

static void walk(int rate, long long n, const std::vector<long long>& cuts) {
    FxDesc d;
    const char* why = nullptr;
    EXPECT(d.make(rate, 100, 0, 0, -1600, &why) == FxDesc::OK);
    StageChain c = d.fresh();
    const int H = lv_hop(rate);
    EXPECT(c.rd.target == -1600 && c.rd.H == H && c.rd.rate == rate && c.any());
    // what the device arrays of this stream would hold: written once each, in order
    std::vector<char> hop_done((size_t)(n / H) + 2, 0), node_done((size_t)(n / H) + 3, 0);
    long long seen = 0, emitted = 0;
    for (size_t j = 0; j <= cuts.size(); ++j) {
        const bool fin = j == cuts.size();
        const long long hi = fin ? n : std::min(n, cuts[j]), in = hi - seen;
        const ChainPlan p = c.plan(in, fin);
        snprintf(where, sizeof where, "rate %d n %lld call %zu in %lld", rate, n, j, in);
        EXPECT(p.rs.out == in && p.rd.in == in && p.rd.out >= 0);
        long long nodes = 0, out = 0;
        rule(H, seen + in, fin, &nodes, &out);
        EXPECT(p.rd.nodes == nodes && p.rd.out == out - emitted && p.rd.base == out);
        EXPECT(p.rd.hops == (seen + in) / H && p.rd.peaks == (fin ? (seen + in + H - 1) / H : (seen + in) / H));
        EXPECT(p.rd.base >= c.rd.base && p.rd.nodes >= c.rd.nodes && p.rd.peaks >= c.rd.peaks);
        EXPECT(c.rd.held(p.rd) < (long long)(RD_A + 1) * H && c.rd.held(p.rd) >= 0);
        // the hop pass starts LV_WARM_HOPS hops before a new hop: those samples are still carried
        if (p.rd.peaks > c.rd.peaks) EXPECT(std::max(0LL, (long long)(c.rd.peaks - LV_WARM_HOPS) * H) >= c.rd.base);
        // every emitted sample has both its nodes
        if (p.rd.out > 0) EXPECT((out - 1) / H + 1 < p.rd.nodes);
        for (int h = c.rd.peaks; h < p.rd.peaks; ++h) { EXPECT(!hop_done.at((size_t)h)); hop_done.at((size_t)h) = 1; }
        for (int k = c.rd.nodes; k < p.rd.nodes; ++k) { EXPECT(!node_done.at((size_t)k)); node_done.at((size_t)k) = 1; }
        c.commit(p);
        seen += in;
        emitted += p.rd.out;
        EXPECT(c.rd.nin == seen && c.rd.nout == emitted && c.seen == seen);
    }
    EXPECT(emitted == n && c.rd.nodes == (n + H - 1) / H + 1 && c.rd.base == n);
    const RdPlan whole = rd_plan(H, n, true);
    EXPECT(whole.nodes == c.rd.nodes && whole.hops == c.rd.hops && whole.peaks == c.rd.peaks && whole.out == n);
}

int main() {
    std::mt19937_64 rng(18);
    for (int rate : RATES) {
        const int H = lv_hop(rate);
        std::vector<long long> lens = {0, 1, H - 1, H, 4LL * H - 1, 4LL * H, (RD_A + 1LL) * H - 1, (RD_A + 1LL) * H, (RD_A + 1LL) * H + 1,
                                       133LL * H, 40LL * H + 17};
        for (int i = 0; i < 6; ++i) lens.push_back((long long)(rng() % (unsigned long long)(60LL * H)));
        for (long long n : lens) {
            walk(rate, n, {});
            std::vector<long long> hops, alt;
            for (long long at = H; at < n + H; at += H) hops.push_back(at);
            walk(rate, n, hops);
            for (long long at = 0, i = 0; at < n; ++i) { at += H + (i % 2 ? 1 : -1); alt.push_back(at); }
            walk(rate, n, alt);
            for (int rep = 0; rep < 8; ++rep) {
                std::vector<long long> cuts;
                const int k = 1 + (int)(rng() % 12);
                for (int i = 0; i < k; ++i) cuts.push_back((long long)(rng() % (unsigned long long)(n + 2)));
                std::sort(cuts.begin(), cuts.end());
                if (rep % 2) { cuts.push_back(cuts.back()); cuts.push_back(n + 5); cuts.push_back(n + 5); }   // empty chunks, a tail-only final
                walk(rate, n, cuts);
            }
        }
    }
    // an absent stage passes its input on and keeps no count
    {
        snprintf(where, sizeof where, "absent");
        RdStage r;
        const RdPlan p = r.plan(777, false);
        EXPECT(p.in == 777 && p.out == 777 && r.held(p) == 0);
        r.commit(p);
        EXPECT(r.nin == 0 && r.par == 0);
        FxDesc d;
        const char* why = nullptr;
        EXPECT(d.make(16000, 100, 0, 0, 0, &why) == FxDesc::OK && !d.fresh().any() && d.fresh().rd.target == 0);
    }
    // the target is judged last; the older overloads leave it unset
    {
        snprintf(where, sizeof where, "make");
        FxDesc d;
        const char* why = nullptr;
        EXPECT(rd_ok(0) && rd_ok(-5000) && rd_ok(-500) && !rd_ok(-5001) && !rd_ok(-499) && !rd_ok(1));
        EXPECT(d.make(16000, 100, 0, 0, -499, &why) == FxDesc::LIVE);
        EXPECT(d.make(7999, 100, 0, 0, -499, &why) == FxDesc::RATE);
        EXPECT(d.make(16000, 49, 0, 0, -499, &why) == FxDesc::SPEED);
        EXPECT(d.make(16000, 100, 0, -499, -499, &why) == FxDesc::LEVEL);
        EXPECT(d.make(16000, 125, 300, 0, -2300, &why) == FxDesc::OK && d.live == -2300 && d.any());
        EXPECT(d.make(16000, 125, 300, -2000, &why) == FxDesc::OK && d.live == 0 && d.level == -2000);
        EXPECT(d.make(44100, 100, 0, &why) == FxDesc::OK && d.live == 0 && !d.any());
        EXPECT((int)FxDesc::LIVE == 6 && (int)FxDesc::LEVEL == 5);
    }
    if (failures) {
        fprintf(stderr, "ride_plan_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("ride_plan_check: ok\n");
    return 0;
}
