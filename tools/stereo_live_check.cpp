// Host program that drives the live stereo mix stage's host arithmetic (fish-tts_amd/csrc/fx_chain.h: mls_check, mls_shift,
// mls_words, mls_expand, mls_sizes, on MlStage and ml_plan) so that a build with -fsanitize=address,undefined sees any read or
// write past an array and any overflow.  No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/stereo_live_check.cpp -o stereo_live_check
// A stream is walked over random cuttings of a programme with random regions - cuts inside, at the start and at the end of a
// region, empty pushes, one-sample pushes - and every push is played on host buffers of exactly the sizes mls_sizes names, with
// the index arithmetic the kernels use (a buffer laid out by the timeline index minus a multiple of four; the staged push, the
// programme carry and the pan carry in two copies): the pan words expanded from the push's own regions, every frame of a newly
// mixed hop read from the carry or from the push with its pan beside it, the m staged and rolled with two values per frame,
// the carries written anew.  The programme sample and the pan every frame is mixed with must be the ones the whole programme
// and the concatenated regions give, whatever the cutting; every frame goes out once, in order.  The per-push region check is
// compared with the stated rule written out here.  Exit status 0 and "stereo_live_check: ok" when every expectation holds.
#include <stdio.h>

#include <random>
#include <vector>

#include "../fish-tts_amd/csrc/fx_chain.h"

using namespace ft::chain;

static int failures = 0;
static char where[240] = "";
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (failures < 20) fprintf(stderr, "%s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, where); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

// The stated rule for the regions of one push, on its own: 0 fine, else the number of the reason.
static int judge(const std::vector<MsRegion>& reg, long long R, bool null, long long n) {
    if (R > 0 && null) return 1;
    if (R < 0 || R > 4096) return 2;
    long long at = 0;
    for (long long r = 0; r < R; ++r) {
        const MsRegion& g = reg[(size_t)r];
        if (!(g.a >= at && g.a < g.e && g.e <= n)) return 3;
        if (g.pan < -100 || g.pan > 100) return 4;
        at = g.e;
    }
    return 0;
}
static int reason(const char* why) {
    if (!why) return 0;
    const std::string s = why;
    return s.find("null") != std::string::npos ? 1 : s.find("R outside") != std::string::npos ? 2 : s.find("out of order") != std::string::npos ? 3 : 4;
}

// Random sorted, disjoint regions over [0, n): some touch, some are one sample long, the last may end on n.
static std::vector<MsRegion> regions_over(std::mt19937& rng, long long n, int H) {
    std::vector<MsRegion> out;
    long long at = rng() % 3 == 0 ? 0 : (long long)(rng() % (unsigned)(H + 1));
    while (at < n && out.size() < 40) {
        const unsigned kind = rng() % 5;
        long long len = kind == 0 ? 1 : kind == 1 ? H : 1 + (long long)(rng() % (unsigned)(3 * H));
        if (rng() % 7 == 0) len = n - at;
        len = std::min(len, n - at);
        const int pan = rng() % 4 == 0 ? (rng() % 2 ? 100 : -100) : (int)(rng() % 201) - 100;
        out.push_back(MsRegion{at, at + len, pan, 0});
        at += len;
        if (rng() % 2) at += (long long)(rng() % (unsigned)(H / 2 + 1));   // else the next one touches
    }
    return out;
}

struct Buffers {
    std::vector<float> prog[2], mc[2];
    std::vector<unsigned char> pans[2];
};

static void walk(std::mt19937& rng, int it) {
    static const int HOPS[] = {160, 320, 882, 960};
    MlShape s;
    s.H = HOPS[rng() % 4];
    s.Wa = 1 + (int)(rng() % 6);
    s.lead = rng() % 3 == 0 ? 0 : (long long)(rng() % (unsigned)(12 * s.H));
    s.tail = rng() % 3 == 0 ? 0 : (long long)(rng() % (unsigned)(8 * s.H));
    s.fade_out = rng() % 3 == 0 ? 0 : (long long)(rng() % (unsigned)(10 * s.H));
    const long long n = it % 13 == 0 ? 0 : (long long)(rng() % (unsigned)((s.Wa + 25) * s.H));
    const long long N = s.lead + n + s.tail;
    snprintf(where, sizeof where, "it %d H %d Wa %d lead %lld tail %lld fade_out %lld n %lld", it, s.H, s.Wa, s.lead, s.tail,
             s.fade_out, n);
    const std::vector<MsRegion> all = regions_over(rng, n, s.H);
    const MsTable whole = {all.data(), (long long)all.size()};
    EXPECT(ms_check(whole, n) == nullptr);
    // the cuts: random, and at or one sample beside the edges of the regions
    std::vector<long long> cuts;
    for (const MsRegion& g : all)
        for (long long c : {g.a - 1, g.a, g.a + 1, g.e - 1, g.e, g.e + 1})
            if (c > 0 && c < n && rng() % 3 == 0) cuts.push_back(c);
    for (int j = (int)(rng() % 8); j > 0 && n > 1; --j) cuts.push_back(1 + (long long)(rng() % (unsigned)(n - 1)));
    if (it % 5 == 0 && n <= 2 * s.H)
        for (long long c = 1; c < n; ++c) cuts.push_back(c);         // one-sample pushes
    std::sort(cuts.begin(), cuts.end());
    cuts.push_back(n);
    if (it % 3 == 0) cuts.insert(cuts.begin(), 0);                   // an empty first push
    if (it % 4 == 0) cuts.push_back(n);                              // an empty final push (duplicates: empty pushes between)

    MlStage st = MlStage::fresh(s);
    Buffers b;
    for (int c = 0; c < 2; ++c) { b.prog[c].assign(4, -1.f); b.pans[c].assign(4, 255); b.mc[c].assign(8, -1.f); }
    std::vector<unsigned char> mixed_frames((size_t)N, 0);
    long long fed = 0, emitted = 0;
    for (size_t ci = 0; ci < cuts.size(); ++ci) {
        const long long k = cuts[ci] - fed;
        const bool final = ci + 1 == cuts.size();
        // the push's regions: the whole programme's, clipped to the push and shifted to its coordinates
        std::vector<MsRegion> reg;
        for (const MsRegion& g : all) {
            const long long a = std::max(g.a, fed), e = std::min(g.e, fed + k);
            if (a < e) reg.push_back(MsRegion{a - fed, e - fed, g.pan, 0});
        }
        const MsTable t = {reg.data(), (long long)reg.size()};
        EXPECT(mls_check(t, k) == nullptr);
        const long long F0 = s.lead + fed;
        for (const MsRegion& g : reg) {                              // back on the timeline they are pieces of the whole table
            const MsRegion u = mls_shift(g, F0);
            EXPECT(u.a >= F0 && u.e <= F0 + k && ms_pan(whole, u.a - s.lead) == g.pan && ms_pan(whole, u.e - 1 - s.lead) == g.pan);
        }
        const MlPlan p = st.plan(k, final);
        const MlsSizes z = mls_sizes(st, p, 2);
        const int r = st.par, w = st.par ^ 1, H = s.H;
        const long long F1 = p.F, cb0 = st.base, cb1 = p.base, mend0 = st.mixed * H, mend1 = final ? p.N : p.mixed * H;
        const long long xb = F0 & ~3LL, pib = cb0 & ~3LL, pob = cb1 & ~3LL, mb = mend0 & ~3LL, cib = st.done & ~3LL, cob = p.done & ~3LL;
        const long long Nend = final ? p.N : 1LL << 30;
        // the staged push and its pan words
        std::vector<float> x(z.x, -1.f), m(z.m, -1.f), y(z.y, -1.f);
        std::vector<unsigned char> q(z.q, 255);
        for (long long j = 0; j < k; ++j) x.at((size_t)(F0 - xb + j)) = (float)(fed + j);
        const long long words = mls_words(F0, k);
        EXPECT((words == 0) == (k == 0));
        if (k > 0) EXPECT(words * MLS_WORD >= F0 + k - xb && (words - 1) * MLS_WORD < F0 + k - xb);   // they cover [xb, F0 + k), no more
        for (long long wd = 0; wd < words; ++wd) {
            unsigned char out[MLS_WORD];
            mls_expand(t, F0, k, wd, out);
            for (int c = 0; c < MLS_WORD; ++c) q.at((size_t)(wd * MLS_WORD + c)) = out[c];
        }
        b.prog[w].assign(z.prog, -1.f);
        b.pans[w].assign(z.pans, 255);
        b.mc[w].assign(z.mc, -1.f);
        // mixl_prog / mixls_pan: the carry below F0, the push from there, nothing outside [cb0, F1)
        auto prog = [&](long long i, float* v, int* pan) {
            const bool old = i < F0;
            const long long lo = old ? cb0 : F0, hi = old ? F0 : F1, ab = old ? pib : xb;
            const long long ic = std::min(std::max(i, lo), std::max(hi - 1, lo));
            const float pv = old ? b.prog[r].at((size_t)(ic - ab)) : x.at((size_t)(ic - ab));
            const unsigned char qv = old ? b.pans[r].at((size_t)(ic - ab)) : q.at((size_t)(ic - ab));
            const bool in = i >= lo && i < hi;
            *v = in ? pv : -2.f;
            *pan = in ? (int)qv - MS_MAX_PAN : 0;
        };
        // mixls_sample_kernel: the frames of the newly mixed hops
        for (long long h = st.mixed; h < p.mixed; ++h) {
            const long long i0 = h * H, i1 = std::min(i0 + H, Nend);
            for (long long i = i0 & ~3LL; i < i1; i += 4) {
                const bool wholeg = i >= i0 && i + 3 < i1;
                if (wholeg && i >= F0 && i + 3 < F1) {               // 16 bytes of the push, 4 of its pans
                    EXPECT((i - xb) % 4 == 0);
                    (void)x.at((size_t)(i - xb + 3)); (void)q.at((size_t)(i - xb + 3));
                } else if (wholeg && i >= cb0 && i + 3 < F0) {       // ... of the carries
                    EXPECT((i - pib) % 4 == 0);
                    (void)b.prog[r].at((size_t)(i - pib + 3)); (void)b.pans[r].at((size_t)(i - pib + 3));
                }
                for (long long f = std::max(i, i0); f < std::min(i + 4, i1); ++f) {
                    float v; int pan;
                    prog(f, &v, &pan);
                    const long long j = f - s.lead;                  // the programme sample, if there is one
                    if (j >= 0 && j < n) {
                        EXPECT(final || j < fed + k);
                        EXPECT(v == (float)j && pan == ms_pan(whole, j));
                    } else {
                        EXPECT(v == -2.f && pan == 0);
                    }
                    EXPECT((i - mb) % 4 == 0 && f - mb >= 0);
                    m.at((size_t)(2 * (f - mb))) = (float)f;
                    m.at((size_t)(2 * (f - mb) + 1)) = -(float)f - 1.f;
                    EXPECT(!mixed_frames.at((size_t)f));
                    mixed_frames.at((size_t)f) = 1;
                }
            }
        }
        // mixls_apply_kernel: y, then the three carries
        auto mm = [&](long long i, int c) {
            const bool old = i < mend0;
            const long long lo = old ? st.done : mend0, hi = old ? mend0 : mend1, ab = old ? cib : mb;
            const long long ic = std::min(std::max(i, lo), std::max(hi - 1, lo));
            return old ? b.mc[r].at((size_t)(2 * (ic - ab) + c)) : m.at((size_t)(2 * (ic - ab) + c));
        };
        EXPECT(p.out == p.done - st.done && st.done == emitted);
        for (long long i = st.done; i < p.done; ++i) {
            y.at((size_t)(2 * (i - st.done))) = mm(i, 0);
            y.at((size_t)(2 * (i - st.done) + 1)) = mm(i, 1);
            EXPECT(y[(size_t)(2 * (i - st.done))] == (float)i && y[(size_t)(2 * (i - st.done) + 1)] == -(float)i - 1.f);
        }
        for (long long i = p.done; i < mend1; ++i)
            for (int c = 0; c < 2; ++c) b.mc[w].at((size_t)(2 * (i - cob) + c)) = mm(i, c);
        for (long long i = cb1; i < F1; ++i) {
            float v; int pan;
            prog(i, &v, &pan);
            b.prog[w].at((size_t)(i - pob)) = v;
            b.pans[w].at((size_t)(i - pob)) = (unsigned char)(pan + MS_MAX_PAN);
            EXPECT(v == (float)(i - s.lead) && pan == ms_pan(whole, i - s.lead));
        }
        emitted += p.out;
        st.commit(p);
        fed += k;
    }
    EXPECT(st.ended && emitted == N && fed == n);
    for (unsigned char v : mixed_frames) EXPECT(v == 1);
}

static void refusals(std::mt19937& rng) {
    snprintf(where, sizeof where, "refusals");
    for (int it = 0; it < 3000; ++it) {
        const long long n = it % 9 == 0 ? 0 : (long long)(rng() % 50);
        std::vector<MsRegion> reg;
        long long at = 0;
        const int R = (int)(rng() % 5);
        for (int r = 0; r < R; ++r) {                                // mostly in order, now and then bent
            const long long a = at + (long long)(rng() % 4) - (rng() % 9 == 0), e = a + (long long)(rng() % 12) + (rng() % 9 != 0);
            reg.push_back(MsRegion{a, e, rng() % 11 == 0 ? 101 - 202 * (int)(rng() % 2) : (int)(rng() % 201) - 100, 0});
            at = e;
        }
        const bool null = R > 0 && rng() % 17 == 0;
        const MsTable t = {null ? nullptr : reg.data(), R};
        EXPECT(reason(mls_check(t, n)) == judge(reg, R, null, n));
    }
    std::vector<MsRegion> many(4097);
    for (int r = 0; r < 4097; ++r) many[(size_t)r] = MsRegion{r, r + 1, 0, 0};
    EXPECT(mls_check(MsTable{many.data(), 4096}, 4096) == nullptr && reason(mls_check(MsTable{many.data(), 4097}, 5000)) == 2);
    EXPECT(reason(mls_check(MsTable{many.data(), 1}, 0)) == 3);      // a push of 0 samples takes R = 0
    EXPECT(mls_check(MsTable{nullptr, 0}, 0) == nullptr);
    EXPECT(mls_words(0, 0) == 0 && mls_words(3, 1) == 1 && mls_words(3, 13) == 1 && mls_words(3, 14) == 2 && mls_words(16, 16) == 1);
    // the regions sit behind the rate and n, before the mix parameters
    bool tl = false;
    MxArgs a;
    a.rate = 8000; a.n = 4; a.depth = -1;
    const MsRegion bad = {0, 5, 0, 0};
    const MsTable bt = {&bad, 1};
    EXPECT(reason(mx_check(a, &tl, 0, &bt)) == 3);
    a.n = -1;
    EXPECT(std::string(mx_check(a, &tl, 0, &bt)).find("n must") != std::string::npos);
}

int main() {
    std::mt19937 rng(20261020u);
    for (int it = 0; it < 1500; ++it) walk(rng, it);
    refusals(rng);
    if (failures) {
        fprintf(stderr, "stereo_live_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("stereo_live_check: ok\n");
    return 0;
}
