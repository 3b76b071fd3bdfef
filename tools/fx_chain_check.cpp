// Host program that drives the output chain's host arithmetic (fish-tts_amd/csrc/fx_chain.h: the filter designs, the rule
// for a (speed, cents) pair, what each stage emits after so many samples, and a stream's stage records from call to call)
// so that a build with -fsanitize=address,undefined sees any read or write past an array and any overflow.  No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/fx_chain_check.cpp -o fx_chain_check
// Over rates x speeds x cents (every combination fx_plan accepts), streams of up to 40 frames of 2048 samples in chunks of
// 1, 2, 5 and 17 frames and as one chunk, the final flag on the last chunk or as a call of no frames of its own:
//   every per-call count is >= 0; a stream's emitted samples sum to ft_resampled_len(rate, ft_timescaled_len(pct, n));
//   the time-scale carry never exceeds TS_CARRY; what a stream has emitted after n samples does not depend on the chunking;
//   the stage records agree call by call with the same walk written out on loose counters.
// Exit status 0 and "fx_chain_check: ok" when every expectation holds.
#include <stdio.h>

#include <array>
#include <map>
#include <vector>

#include "../fish-tts_amd/csrc/fx_chain.h"

using namespace ft::chain;

static int failures = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (failures < 20) fprintf(stderr, "%s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, where); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)
static char where[160] = "";

constexpr int FRAME = 2048;
static const int RATES[] = {8000, 16000, 22050, 24000, 44100, 48000};
static const int RATES_IN[] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 64000, 88200, 96000, 176400, 192000};
static const int SPEEDS[] = {50, 80, 100, 125, 200};
static const int CENTS[] = {-1200, -300, 0, 400, 1200};
static const int FRAMES[] = {1, 2, 5, 17, 40};
static const int CHUNKS[] = {1, 2, 5, 17, 0};   // frames per call; 0: the whole stream in one

// The walk over one stream's stages on loose counters, stage by stage: what the records have to reproduce.
struct Loose {
    const FxDesc* d;
    long long seen = 0, tin = 0, tout = 0, pin = 0, pout = 0, nin = 0, nout = 0;
    int tk = 0;
    // returns {time-scaled, pitched, resampled} samples of the call; *held: the time-scale carry after it
    std::array<long long, 3> call(long long n, bool fin, long long* held) {
        long long x = n, a = n, b, c;
        *held = 0;
        if (d->f.has_ts) {
            const TsPlan p = ts_plan(d->f.ts, tk, tin + n, fin);
            *held = tin + n - p.base;
            x = a = p.out - tout;
            tin += n; tout = p.out; tk = p.k1;
        }
        b = x;
        if (d->ps) {
            b = ps_ready(*d->ps, pin + x, fin, ts_len(d->pct, seen + n)) - pout;
            pin += x; pout += b;
        }
        c = b;
        if (d->K > 0) c = rs_ready(*d->rs, nin + b, fin) - nout;
        nin += b; nout += c;
        seen += n;
        return {a, b, c};
    }
};

static void tables() {
    snprintf(where, sizeof where, "tables");
    for (int rate : RATES) {
        int L = 0, M = 0, K = -1;
        std::vector<float> w;
        EXPECT(rs_design(rate, &L, &M, &K, &w) == nullptr);
        EXPECT(L >= 1 && L <= RS_MAX_L && (long long)L * RS_FI == (long long)M * rate);
        EXPECT((rate == RS_FI) == (K == 0) && K % 2 == 0 && w.size() == (size_t)(K ? L * K : 0));
        EXPECT((255L * M + L - 1) / L + K + 1 <= RS_LDS);
    }
    int L, M, K;
    EXPECT(rs_design(7999, &L, &M, &K, nullptr) && rs_design(48001, &L, &M, &K, nullptr) && rs_design(44101, &L, &M, &K, nullptr));
    // the intake direction (rs_design_in: a reference clip's rate to the codec's)
    for (int rate : RATES_IN) {
        int l = 0, m = 0, k = -1;
        std::vector<float> w;
        EXPECT(rs_design_in(rate, &l, &m, &k, &w) == nullptr);
        EXPECT(l >= 1 && l <= RS_MAX_L && (long long)l * rate == (long long)m * RS_FI);
        EXPECT((rate == RS_FI) == (k == 0) && k % 2 == 0 && k <= 292 && w.size() == (size_t)(k ? l * k : 0));
        EXPECT((255L * m + l - 1) / l + k + 1 <= 1404);
    }
    EXPECT(rs_design_in(7999, &L, &M, &K, nullptr) && rs_design_in(192001, &L, &M, &K, nullptr) &&
           rs_design_in(44099, &L, &M, &K, nullptr) && rs_design_in(47999, &L, &M, &K, nullptr));
    for (int cents : CENTS) {
        long long S = 0;
        std::vector<float> w;
        EXPECT(ps_design(cents, &S, &K, &w));
        EXPECT((cents == 0) == (K == 0) && K % 2 == 0 && w.size() == (size_t)(K ? (PS_PHASES + 1) * K : 0));
        EXPECT((cents == 0 && S == 1LL << PS_SHIFT) || (cents > 0 && S > 1LL << PS_SHIFT) || (cents < 0 && S < 1LL << PS_SHIFT));
    }
    long long S;
    EXPECT(!ps_design(1201, &S, &K, nullptr) && !ps_design(-1201, &S, &K, nullptr));
    EXPECT(!fx_plan(49, 0, nullptr) && !fx_plan(201, 0, nullptr) && !fx_plan(200, -1, nullptr) && !fx_plan(50, 1, nullptr));
    EXPECT(fx_plan(200, 1200, nullptr) && fx_plan(50, -1200, nullptr));
}

static void streams() {
    int combos = 0;
    for (int rate : RATES)
        for (int pct : SPEEDS)
            for (int cents : CENTS) {
                FxDesc d;
                const char* why = nullptr;
                const FxDesc::Bad bad = d.make(rate, pct, cents, &why);
                snprintf(where, sizeof where, "rate %d speed %d cents %d", rate, pct, cents);
                EXPECT((bad == FxDesc::OK) == fx_plan(pct, cents, nullptr));
                if (bad != FxDesc::OK) continue;
                ++combos;
                RsTab rt{d.L, d.M, d.K, nullptr};
                PsTab pt;
                EXPECT(ps_design(cents, &pt.S, &pt.K, nullptr));
                d.rs = &rt;
                if (cents != 0) d.ps = &pt;
                EXPECT(d.f.has_ts == ((long long)pct << PS_SHIFT != 100 * pt.S));
                EXPECT(d.any() == (rate != RS_FI || pct != 100 || cents != 0));
                for (int frames : FRAMES) {
                    const long long n = (long long)frames * FRAME, want = (ts_len(pct, n) * d.L + d.M - 1) / d.M;
                    EXPECT(d.out_len(n) == want && d.fresh().plan(n, true).rs.out == want);
                    std::map<long long, std::array<long long, 3>> at;   // emitted after so many samples, not final
                    for (int chunk : CHUNKS)
                        for (int own_final = 0; own_final < 2; ++own_final) {
                            snprintf(where, sizeof where, "rate %d speed %d cents %d frames %d chunk %d final %s", rate, pct, cents,
                                     frames, chunk, own_final ? "alone" : "on the last chunk");
                            StageChain c = d.fresh();
                            Loose ref{&d};
                            std::array<long long, 3> sum = {0, 0, 0};
                            int left = frames;
                            while (left > 0 || own_final == 1) {
                                const int T = left == 0 ? 0 : (chunk == 0 ? left : std::min(chunk, left));
                                const bool fin = own_final ? left == 0 : T == left;
                                const long long m = (long long)T * FRAME;
                                const ChainPlan p = c.plan(m, fin);
                                long long held = 0;
                                const std::array<long long, 3> r = ref.call(m, fin, &held);
                                EXPECT(p.ts.in == m && p.ps.in == p.ts.out && p.rs.in == p.ps.out);
                                EXPECT(p.ts.out >= 0 && p.ps.out >= 0 && p.rs.out >= 0 && p.ts.k1 >= c.ts.k && p.ts.base >= 0);
                                EXPECT(p.ts.out == r[0] && p.ps.out == r[1] && p.rs.out == r[2] && c.ts.held(p.ts) == held);
                                EXPECT(c.ts.held(p.ts) >= 0 && c.ts.held(p.ts) <= TS_CARRY);
                                const int par = c.rs.par;
                                c.commit(p);
                                EXPECT(c.rs.par == (par ^ 1) && c.seen == ref.seen && c.rs.nin == ref.nin && c.rs.nout == ref.nout);
                                sum[0] += p.ts.out; sum[1] += p.ps.out; sum[2] += p.rs.out;
                                left -= T;
                                if (!fin) {
                                    auto it = at.find(c.seen);
                                    if (it == at.end()) at.emplace(c.seen, sum);
                                    else EXPECT(it->second == sum);
                                } else break;
                            }
                            EXPECT(c.seen == n);
                            EXPECT(sum[0] == ts_len(d.f.has_ts ? d.f.ts : TsRate{}, n) && sum[1] == ts_len(pct, n) && sum[2] == want);
                        }
                }
            }
    snprintf(where, sizeof where, "combinations");
    EXPECT(combos > 100);
}

int main() {
    tables();
    streams();
    if (failures) {
        fprintf(stderr, "fx_chain_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("fx_chain_check: ok\n");
    return 0;
}
