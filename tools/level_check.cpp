// Host program that drives the level stage's host arithmetic (fish-tts_amd/csrc/fx_chain.h: the K-weighting design at any rate,
// the hop, the gates and the gain over given hop sums, and the judgement of a call's level in FxDesc) so that a build with
// -fsanitize=address,undefined sees any read or write past an array and any overflow.  No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/level_check.cpp -o level_check
//   every accepted rate: ten finite coefficients, both biquads stable (poles inside the unit circle: |a2| < 1 and
//   |a1| < 1 + a2), the hop floor(rate / 10); at 48000 the table of BS.1770;
//   hand-built hop sums: the absolute gate, the relative gate, the short-item rule, L = -inf -> gain 1 (silence, no samples,
//   a sum that is not finite), the ceiling, a target of 0;
//   FxDesc::make with a level: judged after the pair, the three-value form unchanged.
// Exit status 0 and "level_check: ok" when every expectation holds.
#include <stdio.h>

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

static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }

static void designs() {
    int rates = 0;
    for (int rate = RS_MIN_RATE; rate <= RS_MAX_RATE; ++rate) {
        int L, M, K;
        if (rs_design(rate, &L, &M, &K, nullptr)) continue;
        ++rates;
        snprintf(where, sizeof where, "rate %d", rate);
        double c[10];
        lv_design(rate, c);
        for (double v : c) EXPECT(std::isfinite(v));
        for (int q = 0; q < 2; ++q) {
            const double a1 = c[5 * q + 3], a2 = c[5 * q + 4];
            EXPECT(std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2);
        }
        EXPECT(c[5] == 1.0 && c[6] == -2.0 && c[7] == 1.0);
        EXPECT(lv_hop(rate) == rate / 10 && lv_hop(rate) >= 800);
    }
    EXPECT(rates > 100);
    snprintf(where, sizeof where, "48000 against BS.1770");
    const double want[10] = {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621};
    double c[10];
    lv_design(48000, c);
    for (int i = 0; i < 10; ++i) EXPECT(near(c[i], want[i], 1e-12));
}

// the block energy of a loudness l
static double energy(double l) { return std::pow(10.0, (l + 0.691) / 10.0); }

static void gates() {
    const int H = 4800;
    // seven whole hops of one energy: four blocks, all kept, L as put in
    {
        snprintf(where, sizeof where, "steady");
        std::vector<double> e(7, energy(-23.0) * H);
        const LvInfo r = lv_gain(e.data(), 7LL * H, H, 0.1f, -1600);
        EXPECT(r.blocks == 4 && r.gated == 4 && near(r.L, -23.0, 1e-9) && !r.capped);
        EXPECT(near(r.g, std::pow(10.0, 7.0 / 20.0), 1e-6) && r.p == 0.1f);
        const LvInfo m = lv_gain(e.data(), 7LL * H, H, 0.1f, 0);          // measure only
        EXPECT(m.g == 1.f && near(m.L, -23.0, 1e-9) && m.gated == 4);
        // a tail of 3 samples past the last whole hop counts for nothing
        e.push_back(1e6);
        const LvInfo t = lv_gain(e.data(), 7LL * H + 3, H, 0.1f, -1600);
        EXPECT(t.blocks == 4 && near(t.L, -23.0, 1e-9));
    }
    // the absolute gate: hops at -80 LUFS around four at -20: only blocks above -70 count
    {
        snprintf(where, sizeof where, "absolute gate");
        std::vector<double> e(12, energy(-80.0) * H);
        for (int h = 4; h < 8; ++h) e[h] = energy(-20.0) * H;
        const LvInfo r = lv_gain(e.data(), 12LL * H, H, 0.5f, -2000);
        EXPECT(r.blocks == 9);
        // blocks 1 .. 7 hold 1 2 3 4 3 2 1 loud hops (-26.0 and up): above -70; blocks 0 and 8 are at -80 and go.  The seven
        // average 16/28 of the loud energy (-22.43), and the relative gate 10 below that keeps them all
        EXPECT(r.gated == 7 && near(r.L, -20.0 + 10.0 * std::log10(16.0 / 28.0), 1e-4));
    }
    // the relative gate: a passage 15 dB down is cut, and L is the loud passage's
    {
        snprintf(where, sizeof where, "relative gate");
        std::vector<double> e(16, energy(-20.0) * H);
        for (int h = 8; h < 16; ++h) e[h] = energy(-35.0) * H;
        const LvInfo r = lv_gain(e.data(), 16LL * H, H, 0.5f, -2000);
        EXPECT(r.blocks == 13 && r.gated < 13 && r.gated >= 5 && r.L > -21.5 && r.L <= -20.0 + 1e-9);
    }
    // fewer than four whole hops: one block over everything the item has
    {
        snprintf(where, sizeof where, "short item");
        const long long n = 3LL * H + 17;
        std::vector<double> e = {1.0, 2.0, 3.0, 0.5};
        const LvInfo r = lv_gain(e.data(), n, H, 0.2f, -2000);
        EXPECT(r.blocks == 1 && r.gated == 1 && near(r.L, lv_lufs(6.5 / (double)n), 1e-12));
        const double one = 0.25;
        const LvInfo s = lv_gain(&one, 1, H, 0.5f, -2000);
        EXPECT(s.blocks == 1 && near(s.L, lv_lufs(0.25), 1e-12));
    }
    // nothing measured: the gain is exactly 1
    {
        snprintf(where, sizeof where, "nothing measured");
        std::vector<double> z(8, 0.0);
        LvInfo r = lv_gain(z.data(), 8LL * H, H, 0.f, -1600);
        EXPECT(r.L == -INFINITY && r.g == 1.f && r.blocks == 5 && r.gated == 0 && !r.capped);
        r = lv_gain(nullptr, 0, H, 0.f, -1600);
        EXPECT(r.L == -INFINITY && r.g == 1.f && r.blocks == 0);
        std::vector<double> q(8, energy(-90.0) * H);                       // below the absolute gate
        r = lv_gain(q.data(), 8LL * H, H, 1e-4f, -1600);
        EXPECT(r.L == -INFINITY && r.g == 1.f && r.gated == 0);
        std::vector<double> bad(8, energy(-20.0) * H);
        bad[3] = NAN;
        r = lv_gain(bad.data(), 8LL * H, H, 0.5f, -1600);
        EXPECT(r.L == -INFINITY && r.g == 1.f);
        bad[3] = INFINITY;
        r = lv_gain(bad.data(), 8LL * H, H, 0.5f, -1600);
        EXPECT(r.L == -INFINITY && r.g == 1.f);
    }
    // the ceiling: a peak of 0.9 at -30 LUFS cannot be raised to -10
    {
        snprintf(where, sizeof where, "ceiling");
        std::vector<double> e(8, energy(-30.0) * H);
        const LvInfo r = lv_gain(e.data(), 8LL * H, H, 0.9f, -1000);
        EXPECT(r.capped == 1 && r.g == (float)(lv_ceiling() / (double)0.9f) && (double)r.g * 0.9 <= lv_ceiling() * (1.0 + 1.2e-7));
        const LvInfo u = lv_gain(e.data(), 8LL * H, H, 0.9f, -4000);       // downwards it does not bind
        EXPECT(!u.capped && near(u.g, std::pow(10.0, -0.5), 1e-7));
        const LvInfo z = lv_gain(e.data(), 8LL * H, H, 0.f, -1000);        // no ceiling term without a peak
        EXPECT(!z.capped && near(z.g, 10.0, 1e-5));
    }
    EXPECT(near(lv_ceiling(), 0.8912509381337456, 1e-15));
}

static void judged() {
    snprintf(where, sizeof where, "FxDesc");
    const char* why = nullptr;
    FxDesc d;
    EXPECT(d.make(44100, 100, 0, &why) == FxDesc::OK && d.level == 0 && !d.any());
    EXPECT(d.make(16000, 100, 0, -1600, &why) == FxDesc::OK && d.level == -1600);
    EXPECT(d.make(44100, 100, 0, -5000, &why) == FxDesc::OK && d.make(44100, 100, 0, -500, &why) == FxDesc::OK);
    EXPECT(d.make(44100, 100, 0, -5001, &why) == FxDesc::LEVEL && d.make(44100, 100, 0, -499, &why) == FxDesc::LEVEL);
    EXPECT(d.make(44100, 100, 0, 1, &why) == FxDesc::LEVEL && d.make(44100, 100, 0, 1600, &why) == FxDesc::LEVEL);
    EXPECT(d.make(7000, 100, 0, 1, &why) == FxDesc::RATE && d.make(44100, 30, 0, 1, &why) == FxDesc::SPEED);
    EXPECT(d.make(44100, 100, 2000, 1, &why) == FxDesc::CENTS && d.make(44100, 200, -1200, 1, &why) == FxDesc::PAIR);
    EXPECT(lv_ok(0) && lv_ok(-5000) && lv_ok(-500) && !lv_ok(-5001) && !lv_ok(-499) && !lv_ok(100));
}

int main() {
    designs();
    gates();
    judged();
    if (failures) {
        fprintf(stderr, "level_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("level_check: ok\n");
    return 0;
}
