// Host arithmetic of the output chain behind the codec (fishtts_hip.h: sample_rate, speed_pct, pitch_cents, loudness, live): the
// time-scale stage, then the pitch stage, then the resampler, then the level (whole items) or the ride stage (streams).  The filter designs, the rule that accepts a
// (speed, cents) pair, what each stage can emit after so many input samples, the bookkeeping of a stream's three stages from
// call to call, and the level stage's K-weighting design, gates and gain; behind the join, the mix stage's timeline, checks,
// duck and gain table (mx_*; tools/mix_check.cpp drives that block), the stereo mix stage's pan regions, pan table and bed
// sides (ms_*; tools/stereo_check.cpp), the live mix stage's emission (ml_*, MlStage; tools/mix_live_check.cpp), the live
// stereo mix stage's per-push regions, pan words and buffer sizes (mls_*; tools/stereo_live_check.cpp) and, between the join
// and the mix stages, the room stage's send regions, checks, lengths and buffer sizes (rm_*; tools/room_check.cpp), the live
// room stage's counters, carry bounds and per-push checks (rl_*; tools/room_live_check.cpp).
// Plain C++ without HIP, so that a host program can drive it under a sanitizer (tools/fx_chain_check.cpp).  The constants
// are those of the kernels (stage_kernels.h); codec.hip asserts that the two sets agree.
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace ft {
namespace chain {

constexpr int RS_FI = 44100, RS_MIN_RATE = 8000, RS_MAX_RATE = 48000, RS_MAX_L = 640, RS_LDS = 2048;
constexpr int TS_N = 1024, TS_HS = 512, TS_D = 384, TS_CARRY = TS_N + 2 * TS_D + 2 * TS_HS;
constexpr int TS_MIN_PCT = 50, TS_MAX_PCT = 200;
constexpr int PS_SHIFT = 20, PS_PHASES = 512, PS_MAX_CENTS = 1200;

struct RsTab { int L = 1, M = 1, K = 0; float* w = nullptr; };        // one output rate: [L][K] on the device
struct PsTab { long long S = 0; int K = 0; float* w = nullptr; };     // one cents value: [513][K] on the device

// ---- resampler (RsSeg, resample_kernel): filter design on the host in float64, a Kaiser-windowed sinc at the up-sampled
// rate L Fi cut off at 0.465 Fmin (pass band to 0.43 Fmin, stop band from 0.5 Fmin, Fmin = min(Fi, Fo)), designed for 75 dB.
// Tap t of phase p is the prototype at j = p + (K/2 - 1 - t) L up-sampled samples from the output instant, gain L (the
// zero-stuffed input).  Rates: integers in [8000, 48000] whose reduced L is at most 640; the codec's own rate has K = 0.
inline double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 500 && term > 1e-17 * sum; ++k) {
        term *= q / ((double)k * k);
        sum += term;
    }
    return sum;
}

// The design for any pair of rates: from Fi to Fo = Fi L / M, L = Fo / g, M = Fi / g, g = gcd(Fi, Fo); K = 0 when Fi == Fo.
// An error message (the caller says which rate is meant), or null; fills w ([L][K] float32) when non-null.
inline const char* rs_design_pair(int fi, int fo, int* L, int* M, int* K, std::vector<float>* w) {
    const int g = std::gcd(fi, fo), l = fo / g, m = fi / g;
    if (l > RS_MAX_L) return "sample rate: rate / gcd(rate, 44100) exceeds 640";
    *L = l;
    *M = m;
    *K = 0;
    if (fi == fo) return nullptr;
    const double A = 75.0, beta = 0.1102 * (A - 8.7), fmin = std::min(fi, fo);
    int k = (int)std::ceil((A - 7.95) / (2.285 * 2.0 * M_PI * 0.07) * fi / fmin);
    k += k & 1;
    if ((255L * m + l - 1) / l + k + 1 > RS_LDS) return "sample rate: filter window exceeds the resampler's LDS stage";
    *K = k;
    if (!w) return nullptr;
    const double fc = 0.465 * fmin / ((double)l * fi), half = 0.5 * k * l, ib = bessel_i0(beta);
    w->assign((size_t)l * k, 0.f);
    for (int p = 0; p < l; ++p)
        for (int t = 0; t < k; ++t) {
            const double j = p + (double)(k / 2 - 1 - t) * l, r = j / half, x = M_PI * 2.0 * fc * j;
            const double sinc = j == 0 ? 1.0 : std::sin(x) / x;
            (*w)[(size_t)p * k + t] = (float)(2.0 * fc * l * sinc * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / ib);
        }
    return nullptr;
}

// The output direction, Fi = 44100 and Fo = `rate`: validates `rate` (an error message, or null) and gives L, M, K; fills w
// ([L][K] float32) when non-null.
inline const char* rs_design(int rate, int* L, int* M, int* K, std::vector<float>* w) {
    if (rate < RS_MIN_RATE || rate > RS_MAX_RATE) return "sample rate outside [8000, 48000]";
    return rs_design_pair(RS_FI, rate, L, M, K, w);
}

// The intake direction (intake_kernel), Fi = `rate_in` and Fo = 44100: a reference clip brought to the codec's rate.  Rates:
// integers in [8000, 192000] whose reduced L = 44100 / gcd is at most 640 and whose window fits the LDS stage.
constexpr int RS_MAX_RATE_IN = 192000;
inline const char* rs_design_in(int rate_in, int* L, int* M, int* K, std::vector<float>* w) {
    if (rate_in < RS_MIN_RATE || rate_in > RS_MAX_RATE_IN) return "input sample rate outside [8000, 192000]";
    if (RS_FI / std::gcd(rate_in, RS_FI) > RS_MAX_L) return "input sample rate: 44100 / gcd(rate, 44100) exceeds 640";
    return rs_design_pair(rate_in, RS_FI, L, M, K, w);
}

// Outputs available after `nin` input samples: all of them at the end of the input (final), else those whose taps all
// lie within it (floor(n M / L) + K/2 < nin).
inline long long rs_ready(const RsTab& t, long long nin, bool final) {
    if (t.K == 0) return nin;
    const long long a = final ? nin : nin - t.K / 2;
    return a > 0 ? (a * t.L + t.M - 1) / t.M : 0;
}

// ---- time-scale stage (TsSeg, timescale_kernel; fishtts_hip.h states the algorithm)
inline bool ts_ok(int pct) { return pct >= TS_MIN_PCT && pct <= TS_MAX_PCT; }
// The stage runs at the rational rate num / den: pct / 100 for a speed alone, pct 2^20 / (100 S) under a pitch shift
// (k HS num stays below 2^52 for any stream within max_frames).
struct TsRate { long long num = 100, den = 100; };
inline long long ts_len(TsRate r, long long n) { return (n * r.den + r.num - 1) / r.num; }
inline long long ts_len(int pct, long long n) { return ts_len(TsRate{pct, 100}, n); }
inline long long ts_a(TsRate r, long long k) { return k * TS_HS * r.num / r.den; }
// Input samples frame k needs to have been seen: its search region ends at a_k + HS + D, its template (the continuation
// of frame k - 1) at most at a_{k-1} + D + N, which lies further on below speed 1.
inline long long ts_need(TsRate r, long long k) {
    return std::max(ts_a(r, k), k > 0 ? ts_a(r, k - 1) + TS_HS : 0) + TS_HS + TS_D;
}
struct TsPlan { int k1 = 0; long long out = 0, base = 0; };
// What a stream that has run k0 frames does once it has seen `nin` samples: frames [k0, k1), outputs below `out` final,
// input from `base` on kept for later frames.
inline TsPlan ts_plan(TsRate r, int k0, long long nin, bool final) {
    TsPlan p;
    if (final) {
        p.out = ts_len(r, nin);
        p.k1 = (int)((p.out + TS_HS - 1) / TS_HS) + 1;
        p.base = nin;
        return p;
    }
    p.k1 = k0;
    while (ts_need(r, p.k1) <= nin) ++p.k1;
    p.out = p.k1 > 0 ? (long long)(p.k1 - 1) * TS_HS : 0;
    p.base = ts_a(r, p.k1) - TS_HS - TS_D;
    if (p.k1 > 0) p.base = std::min(p.base, ts_a(r, p.k1 - 1) - TS_D);
    p.base = std::max(p.base, 0LL);
    return p;
}

// ---- pitch stage (PsSeg, pitch_kernel; fishtts_hip.h states it): the step S = llround(2^20 2^(cents / 1200)) and the
// [513][K] table, a Kaiser-windowed sinc designed in float64 with the resampler's constants (75 dB, transition 0.07), cut off
// at 0.465 min(1, 1 / r) cycles per input sample, r = S / 2^20; tap t of row p is the prototype at p / 512 + (K/2 - 1 - t).
inline bool ps_design(int cents, long long* S, int* K, std::vector<float>* w) {
    if (cents < -PS_MAX_CENTS || cents > PS_MAX_CENTS) return false;
    *S = std::llround(std::ldexp(std::exp2((double)cents / 1200.0), PS_SHIFT));
    *K = 0;
    if (cents == 0) return true;
    const double A = 75.0, beta = 0.1102 * (A - 8.7), r = std::ldexp((double)*S, -PS_SHIFT);
    int k = (int)std::ceil((A - 7.95) / (2.285 * 2.0 * M_PI * 0.07) * std::max(1.0, r));
    k += k & 1;
    *K = k;
    if (!w) return true;
    const double fc = 0.465 * std::min(1.0, 1.0 / r), half = 0.5 * k, ib = bessel_i0(beta);
    w->assign((size_t)(PS_PHASES + 1) * k, 0.f);
    for (int p = 0; p <= PS_PHASES; ++p)
        for (int t = 0; t < k; ++t) {
            const double tau = (double)p / PS_PHASES + (double)(k / 2 - 1 - t), q = tau / half, x = M_PI * 2.0 * fc * tau;
            const double sinc = tau == 0 ? 1.0 : std::sin(x) / x;
            (*w)[(size_t)p * k + t] = (float)(2.0 * fc * sinc * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - q * q))) / ib);
        }
    return true;
}

// The stages in front of the resampler for (speed_pct, cents): the time-scale stage's rate, absent at rate 1.  Accepted:
// cents in [-1200, 1200] and an effective rate speed_pct 2^20 / (100 S) in [0.5, 2].
struct FxPlan { TsRate ts; bool has_ts = false; long long S = 0; };
inline bool fx_plan(int pct, int cents, FxPlan* out) {
    FxPlan f;
    int k;
    if (!ts_ok(pct) || !ps_design(cents, &f.S, &k, nullptr)) return false;
    f.ts = TsRate{(long long)pct << PS_SHIFT, 100 * f.S};
    if (50 * f.S > f.ts.num || f.ts.num > 200 * f.S) return false;
    f.has_ts = f.ts.num != f.ts.den;
    if (cents == 0) f.ts = TsRate{pct, 100};   // the speed alone, as it always ran
    if (out) *out = f;
    return true;
}

// Outputs available after `nin` input samples: those whose taps all lie within them ((n S >> 20) + K/2 < nin); at the end of
// the input (final) all `total` of them.
inline long long ps_ready(const PsTab& t, long long nin, bool final, long long total) {
    if (final) return total;
    const long long a = nin - t.K / 2;
    return a > 0 ? ((a << PS_SHIFT) + t.S - 1) / t.S : 0;
}

// ---- level stage (level_filter_kernel, level_gain_kernel, level_scale_kernel; fishtts_hip.h states it): the K-weighting
// design at any rate, the hop, and the gates and the gain over given hop sums.  The target is in hundredths of a LUFS.
constexpr int LV_MIN = -5000, LV_MAX = -500, LV_WARM_HOPS = 2;
inline bool lv_ok(int target) { return target == 0 || (target >= LV_MIN && target <= LV_MAX); }
inline int lv_hop(int rate) { return rate / 10; }
inline double lv_ceiling() { return std::pow(10.0, -1.0 / 20.0); }      // -1 dBFS on the sample peak

// c = the shelf's b0 b1 b2 a1 a2, then the high-pass's: two biquads from the analogue prototypes of BS.1770, in float64.
inline void lv_design(int rate, double c[10]) {
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(M_PI * f0 / rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(M_PI * f0 / rate), d = 1.0 + K / Q + K * K;
        c[5] = 1.0;
        c[6] = -2.0;
        c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / d;
        c[9] = (1.0 - K / Q + K * K) / d;
    }
}

inline double lv_lufs(double E) { return -0.691 + 10.0 * std::log10(E); }

struct LvInfo { double L = -INFINITY; float p = 0.f, g = 1.f; int blocks = 0, gated = 0, capped = 0; };

// The stage's result for an item of n samples with hop H from its hop sums e[0 .. ceil(n / H)) (the last one over what is
// left of the item), its sample peak p and the target (0: measure only, the gain stays 1).
inline LvInfo lv_gain(const double* e, long long n, int H, float p, int target) {
    LvInfo r;
    r.p = p;
    if (n < 1 || H < 1) return r;
    const long long hops = n / H;
    std::vector<double> E;
    if (hops < 4) {
        double s = 0.0;
        for (long long h = 0; h < (n + H - 1) / H; ++h) s += e[h];
        E.push_back(s / (double)n);
    } else {
        for (long long j = 0; j + 3 < hops; ++j) E.push_back((e[j] + e[j + 1] + e[j + 2] + e[j + 3]) / (4.0 * H));
    }
    r.blocks = (int)E.size();
    double s = 0.0, all = 0.0;
    long long k = 0;
    for (double v : E) {
        all += v;
        if (lv_lufs(v) > -70.0) { s += v; ++k; }
    }
    if (!std::isfinite(all) || k == 0) return r;
    const double gamma = lv_lufs(s / (double)k) - 10.0;
    s = 0.0;
    k = 0;
    for (double v : E)
        if (lv_lufs(v) > -70.0 && lv_lufs(v) > gamma) { s += v; ++k; }
    if (k == 0) return r;
    r.gated = (int)k;
    r.L = lv_lufs(s / (double)k);
    if (target == 0) return r;
    double g = std::pow(10.0, ((double)target / 100.0 - r.L) / 20.0);
    if (p > 0.f && lv_ceiling() / (double)p < g) {
        g = lv_ceiling() / (double)p;
        r.capped = 1;
    }
    r.g = (float)g;
    return r;
}

// ---- ride stage (ride_hop_kernel, ride_node_kernel, ride_apply_kernel; fishtts_hip.h states it): a look-ahead gain rider
// behind the resampler of a stream.  Node k sits at sample k H; it is final once RD_A more whole hops have been seen (or at
// the end of the stream), and the samples below the last final node go out.  The target is the level stage's.
constexpr int RD_A = 10;              // look-ahead, hops
constexpr double RD_R = 0.5;          // slew, dB per hop
inline bool rd_ok(int target) { return lv_ok(target); }
// After `nin` samples at hop H: whole hops, hop peaks known, final nodes, final outputs (= the first sample still carried).
struct RdPlan { long long in = 0, out = 0, base = 0; int hops = 0, peaks = 0, nodes = 0; };
inline RdPlan rd_plan(int H, long long nin, bool final) {
    RdPlan p;
    p.hops = (int)(nin / H);
    if (final) {
        p.peaks = (int)((nin + H - 1) / H);
        p.nodes = p.peaks + 1;
        p.out = p.base = nin;
        return p;
    }
    p.peaks = p.hops;
    p.nodes = p.hops >= RD_A ? p.hops - RD_A + 1 : 0;
    p.out = p.base = (long long)std::max(0, p.hops - RD_A) * H;
    return p;
}

// ---- mix stage (mix_hop_kernel, mix_node_kernel, mix_kernel, mix_scale_kernel; fishtts_hip.h states it): a bed under a
// finished programme, lowered by a look-ahead sidechain gain that follows the programme's activity.  The hop (20 ms), the
// timeline, the argument checks in their stated order, the duck D_k (hundredths of a dB) from an activity array, the table.
constexpr int MX_MAX_DEPTH = 6000, MX_MAX_W = 500;
constexpr long long MX_MAX_N = 1LL << 28;
inline int mx_hop(int rate) { return rate / 50; }
struct MxPlan { long long N = 0, Nh = 0; int H = 1; };
// The timeline of n programme samples at `rate` with `lead` and `tail` (all judged by mx_check first).
inline MxPlan mx_plan(int rate, long long n, long long lead, long long tail) {
    MxPlan p;
    p.H = mx_hop(rate);
    p.N = lead + n + tail;
    p.Nh = (p.N + p.H - 1) / p.H;
    return p;
}
// The values of a call in the order every entry point judges them: null, or why not (*too_long: the refusal is a length).
struct MxArgs {
    int rate = RS_FI;
    long long n = 0;
    int bed_loudness = 0, depth = 0;
    float threshold = 0.f;
    int attack = 1, release = 1;
    long long lead = 0, tail = 0, fade_in = 0, fade_out = 0, offset = 0;
    int loop = 0;
};
// The stereo mix stage's pan regions (ft_pan_region; fishtts_hip.h: "Stereo mix"): sorted, disjoint, inside [0, n), pans in
// hundredths from -100 (hard left) to 100.  ms_check judges a table; ms_pan is q of programme sample j by binary search.
constexpr int MS_MAX_REGIONS = 4096, MS_MAX_PAN = 100;
struct MsRegion { long long a = 0, e = 0; int pan = 0, reserved = 0; };
struct MsTable { const MsRegion* reg = nullptr; long long R = 0; };
inline const char* ms_check(const MsTable& t, long long n) {
    if (t.R > 0 && !t.reg) return "a null region table with R > 0";
    if (t.R < 0 || t.R > MS_MAX_REGIONS) return "R outside [0, 4096] pan regions";
    long long at = 0;                         // the end of the region before
    for (long long r = 0; r < t.R; ++r) {
        const MsRegion& g = t.reg[r];
        if (g.a < at || g.a >= g.e || g.e > n) return "a pan region out of order or outside [0, n)";
        if (g.pan < -MS_MAX_PAN || g.pan > MS_MAX_PAN) return "a pan outside [-100, 100]";
        at = g.e;
    }
    return nullptr;
}
inline int ms_pan(const MsTable& t, long long j) {
    long long lo = 0, hi = t.R;               // the first region that ends behind j
    while (lo < hi) {
        const long long mid = (lo + hi) / 2;
        if (t.reg[mid].e > j) hi = mid; else lo = mid + 1;
    }
    return lo < t.R && t.reg[lo].a <= j ? t.reg[lo].pan : 0;
}
// U[j] = (float) min(1, sqrt(2) sin(j pi / 400)), j = 0 .. 200: float64 rounded once; U[0] = 0 and U[j] = 1 from the centre
// (j = 100) on by definition.  The right gain of pan q is U[100 + q], the left one U[100 - q].
inline void ms_gains(float* U) {
    for (int j = 0; j <= 2 * MS_MAX_PAN; ++j)
        U[j] = j == 0 ? 0.f : j >= MS_MAX_PAN ? 1.f : (float)std::min(1.0, std::sqrt(2.0) * std::sin((double)j * M_PI / 400.0));
}
// The channels of the bed's two sides: channel = -1 takes channels 0 and 1 (a mono file: 0 twice), channel = k takes k twice.
// Where both sides name one channel the bed is the mono bed of the mix stage with `channel` as it was given.
struct MsSides { int ch[2] = {0, 0}; bool same = true; };
inline MsSides ms_sides(int channel, int channels) {
    MsSides s;
    if (channel == -1) s.ch[1] = channels >= 2 ? 1 : 0;
    else s.ch[0] = s.ch[1] = channel;         // (a channel the intake refuses is refused there, as the mix stage's is)
    s.same = s.ch[0] == s.ch[1];
    return s;
}

// (min_n: 1 for the mix stage; 0 for the live mix stage, whose programme may be empty.  pans: the stereo mix stage's region
// table, judged behind the rate and n)
inline const char* mx_check(const MxArgs& a, bool* too_long, long long min_n = 1, const MsTable* pans = nullptr) {
    int L, M, K;
    *too_long = false;
    if (const char* e = rs_design(a.rate, &L, &M, &K, nullptr)) return e;
    if (a.n < min_n) return min_n >= 1 ? "n must be at least 1" : "n must be >= 0";
    if (pans)
        if (const char* e = ms_check(*pans, a.n)) return e;
    if (!lv_ok(a.bed_loudness)) return "bed_loudness neither 0 nor in [-5000, -500] hundredths of a LUFS";
    if (a.depth < 0 || a.depth > MX_MAX_DEPTH) return "depth outside [0, 6000] hundredths of a dB";
    if (!(a.threshold >= 0.f)) return "threshold must be >= 0";   // (refuses a NaN too)
    if (a.attack < 1 || a.attack > MX_MAX_W) return "attack outside [1, 500] hops";
    if (a.release < 1 || a.release > MX_MAX_W) return "release outside [1, 500] hops";
    if (a.lead < 0) return "lead must be >= 0";
    if (a.tail < 0) return "tail must be >= 0";
    if (a.fade_in < 0) return "fade_in must be >= 0";
    if (a.fade_out < 0) return "fade_out must be >= 0";
    if (a.offset < 0) return "offset must be >= 0";
    if (a.loop != 0 && a.loop != 1) return "loop must be 0 or 1";
    if (a.n > MX_MAX_N || a.lead > MX_MAX_N || a.tail > MX_MAX_N || a.lead + a.n + a.tail > MX_MAX_N) {
        *too_long = true;
        return "lead + n + tail exceeds 2^28 samples";
    }
    return nullptr;
}
// D_k for k = 0 .. Nh from act[0 .. Nh): the largest of 0, depth (Wa - (h - k)) / Wa over active h in [k, k + Wa - 1] and
// depth (Wr - (k - 1 - h)) / Wr over active h in [k - Wr, k - 1] (int64 divisions).  Both terms fall with the distance, so
// the nearest active hop on either side decides: one pass each way.
inline void mx_duck(const unsigned char* act, long long Nh, int depth, int Wa, int Wr, int* D) {
    long long near = -1;                      // the nearest active hop at or after k
    for (long long k = Nh; k >= 0; --k) {
        if (k < Nh && act[k]) near = k;
        D[k] = near >= 0 && near - k < Wa ? (int)((long long)depth * (Wa - (near - k)) / Wa) : 0;
    }
    near = -1;                                // the nearest active hop before k
    for (long long k = 0; k <= Nh; ++k) {
        if (k >= 1 && act[k - 1]) near = k - 1;
        if (near >= 0 && k - 1 - near < Wr) D[k] = std::max(D[k], (int)((long long)depth * (Wr - (k - 1 - near)) / Wr));
    }
}
// T[d] = (float) 10^(-d / 2000), d = 0 .. 6000: float64 rounded once; T[0] = 1.
inline void mx_gains(float* T) {
    for (int d = 0; d <= MX_MAX_DEPTH; ++d) T[d] = (float)std::pow(10.0, -(double)d / 2000.0);
}

// ---- live mix stage (mixl_*_kernel; fishtts_hip.h states it under "Live mix"): the mix stage on a stream, the one gain of
// its ceiling replaced by a look-ahead limiter over the hops' own peaks.  What is final after n_in programme samples - hops
// with their activity, duck nodes, hops with their m and Q, limiter nodes, outputs - in closed form (ml_plan), and the stage
// that walks a stream from push to push (MlStage; tools/mix_live_check.cpp drives both).
constexpr int ML_LA = 5, ML_LR = 25;                 // the limiter's attack and release, hops
constexpr long long ML_MAX_FADE = 1LL << 30;         // a fade counts as this at most: longer than any timeline (MX_MAX_N)
struct MlShape { int H = 1, Wa = 1; long long lead = 0, tail = 0, fade_out = 0; };
// Totals after n_in programme samples: F = lead + n_in; hops [0, hops) have their activity, nodes [0, ducks) their D_k, hops
// [0, mixed) their m and Q, nodes [0, limits) their L_k, samples [0, done) went out; the programme is carried from timeline
// sample `base` on.  in / out: what the call that led here took and emitted (MlStage::plan).
struct MlPlan { long long in = 0, out = 0, F = 0, N = 0, hops = 0, ducks = 0, mixed = 0, limits = 0, done = 0, base = 0; bool final = false; };
inline MlPlan ml_plan(const MlShape& s, long long n_in, bool final) {
    MlPlan p;
    p.final = final;
    p.F = s.lead + n_in;
    p.N = p.F + s.tail;
    if (final) {
        p.hops = p.mixed = (p.N + s.H - 1) / s.H;
        p.ducks = p.limits = p.hops + 1;
        p.done = p.N;
        p.base = p.F;
        return p;
    }
    const long long W = p.F / s.H, E = p.N - std::min(s.fade_out, ML_MAX_FADE);
    p.hops = W;
    p.ducks = std::max(0LL, W - s.Wa + 1);
    p.mixed = std::min(std::max(0LL, W - s.Wa), std::max(0LL, E) / s.H);
    p.limits = std::max(0LL, p.mixed - ML_LA + 1);
    p.done = std::max(0LL, p.mixed - ML_LA) * s.H;
    p.base = std::min(std::max(p.mixed * s.H, s.lead), p.F);
    return p;
}
// A stream of the stage.  The counters live here, on the host; on the device the stream carries the programme from `base` on
// and the m of [done, mixed H), two copies each (a push reads carry[par] and writes carry[par ^ 1]).
struct MlStage {
    MlShape s;
    int par = 0;
    bool ended = false;                        // the final push went through
    long long nin = 0, hops = 0, ducks = 0, mixed = 0, limits = 0, done = 0, base = 0;
    static MlStage fresh(const MlShape& shape) {
        MlStage m;
        m.s = shape;
        m.base = shape.lead;                   // nothing carried: the programme begins at `lead`
        return m;
    }
    MlPlan plan(long long n, bool final) const {
        MlPlan p = ml_plan(s, nin + n, final);
        p.in = n;
        p.out = p.done - done;
        return p;
    }
    // carried after the call: programme samples, below (Wa + 2) H + max(0, fade_out - tail), and samples of m, at most ML_LA H
    long long held_prog(const MlPlan& p) const { return p.F - p.base; }
    long long held_mix(const MlPlan& p) const { return p.final ? 0 : p.mixed * s.H - p.done; }
    long long held(const MlPlan& p) const { return held_prog(p) + held_mix(p); }
    void commit(const MlPlan& p) {
        nin += p.in; hops = p.hops; ducks = p.ducks; mixed = p.mixed; limits = p.limits; done = p.done; base = p.base;
        ended = p.final;
        par ^= 1;
    }
};

// ---- live stereo mix stage (mixls_*_kernel in stereo_kernels.h; fishtts_hip.h states it under "Live stereo mix"): the live
// mix stage with two channels out.  Its counters are MlStage's and its emission ml_plan's, in frames.  What it adds on the
// host: the regions of a push, relative to that push, judged by ms_check over the push's n; their place on the timeline (a
// push that begins at timeline sample F0 = lead + n_in puts its sample j at F0 + j); the pan bytes - pan + 100 per programme
// sample, 100 outside every region - which a push expands on the device and which roll beside the programme carry in the same
// layout (timeline index minus a multiple of four); and the sizes of the buffers a push touches, in elements, so that the
// stream and tools/stereo_live_check.cpp, which walks random cuttings over host buffers of exactly these sizes, agree.
constexpr int MLS_WORD = 16;                         // pan bytes one lane of the expansion writes, one 16-byte store
inline const char* mls_check(const MsTable& t, long long n) { return ms_check(t, n); }
inline MsRegion mls_shift(const MsRegion& g, long long F0) { return MsRegion{g.a + F0, g.e + F0, g.pan, 0}; }
// The 16-byte words of pan bytes a push of n samples from timeline sample F0 writes: they begin at xb = F0 rounded down to
// a multiple of four and cover [xb, F0 + n); bytes outside [F0, F0 + n) are written as the centre and never read.
inline long long mls_words(long long F0, long long n) {
    return n > 0 ? (F0 + n - (F0 & ~3LL) + MLS_WORD - 1) / MLS_WORD : 0;
}
// Word w of that expansion, as mixls_pan_kernel writes it: the regions are the push's own, relative to it.
inline void mls_expand(const MsTable& t, long long F0, long long n, long long w, unsigned char* out) {
    const long long xb = F0 & ~3LL;
    for (int k = 0; k < MLS_WORD; ++k) {
        const long long j = xb + w * MLS_WORD + k - F0;
        out[k] = (unsigned char)(MS_MAX_PAN + (j >= 0 && j < n ? ms_pan(t, j) : 0));
    }
}
// Elements a push needs in each buffer (the margins are the layout's: a buffer begins up to three elements before its first
// sample, and a 16-byte access may end up to three behind its last): the staged push and its pan bytes, the staged m and the
// output (floats, `ch` per frame), and the three carries the push writes (programme, pan bytes, m - `ch` floats per frame).
// ch: 2 for a stereo stream; 1 for a stream of the live mix stage, which has no pan bytes and leaves q and pans unused.
struct MlsSizes { size_t x = 0, q = 0, m = 0, y = 0, prog = 0, pans = 0, mc = 0; };
inline MlsSizes mls_sizes(const MlStage& st, const MlPlan& p, int ch) {
    MlsSizes z;
    const long long H = st.s.H, F0 = st.s.lead + st.nin, mend0 = st.mixed * H, mend1 = p.final ? p.N : p.mixed * H;
    z.x = (size_t)p.in + 8;
    z.q = (size_t)(mls_words(F0, p.in) * MLS_WORD) + 8;
    z.m = ch * ((size_t)(mend1 - mend0) + 8);
    z.y = ch * (size_t)p.out + 8;
    z.prog = (size_t)(p.F - p.base) + 4;
    z.pans = (size_t)(p.F - p.base) + 4;
    z.mc = ch * ((size_t)(mend1 - p.done) + 4);
    return z;
}

// ---- room stage (room_*_kernel in room_kernels.h; fishtts_hip.h states it under "Room"): a convolution reverb between the
// join and the mix stages.  The send regions (ft_send_region: the pan regions' layout and order rules, a send in the pan's
// place), the checks in their stated order, the impulse response's length at the output rate, L, f, the tail and N
// (tools/room_check.cpp drives this block).
constexpr int RM_MAX_L = 131072, RM_MAX_SEND = MX_MAX_DEPTH;
inline const char* rm_regions(const MsTable& t, long long n) {
    if (t.R > 0 && !t.reg) return "a null region table with R > 0";
    if (t.R < 0 || t.R > MS_MAX_REGIONS) return "R outside [0, 4096] send regions";
    long long at = 0;
    for (long long r = 0; r < t.R; ++r) {
        const MsRegion& g = t.reg[r];
        if (g.a < at || g.a >= g.e || g.e > n) return "a send region out of order or outside [0, n)";
        if (g.pan < -1 || g.pan > RM_MAX_SEND) return "a send neither -1 nor in [0, 6000] hundredths of a dB";
        at = g.e;
    }
    return nullptr;
}
// The send of programme sample j: its region's, `send` outside every region (ms_pan's search).
inline int rm_send(const MsTable& t, long long j, int send) {
    long long lo = 0, hi = t.R;
    while (lo < hi) {
        const long long mid = (lo + hi) / 2;
        if (t.reg[mid].e > j) hi = mid; else lo = mid + 1;
    }
    return lo < t.R && t.reg[lo].a <= j ? t.reg[lo].pan : send;
}
struct RmArgs {
    int rate = RS_FI;
    long long n = 0;
    int channel = -1, normalize = 1, wet = 0, dry = 0, send = 0, ceiling = 1;
    long long offset = 0, length = 0, fade = 0, predelay = 0, tail = -1;
    int ir_rate = RS_FI, ir_channels = 1;     // the impulse response's item
    long long ir_frames = 1;
    long long nh = -1;                         // >= 0: the response's length at the output rate, given (ft_room_plan)
    int live = 0;                              // a stream's begin (rl_begin_args): the ceiling must be 0
};
// The impulse response's samples at the output rate, as the intake and the resampler count them; -1 where the item's own
// checks (the intake's, which come last) will refuse it.
inline long long rm_ir_len(int ir_rate, long long ir_frames, int rate) {
    int L, M, K;
    if (ir_frames < 1 || ir_frames > (1LL << 30) || rs_design_in(ir_rate, &L, &M, &K, nullptr)) return -1;
    const long long n44 = (ir_frames * L + M - 1) / M;
    if (rs_design(rate, &L, &M, &K, nullptr)) return -1;
    return K > 0 ? (n44 * L + M - 1) / M : n44;
}
struct RmPlan { long long nh = 0, L = 0, f = 0, tl = 0, N = 0; bool send = false; };
// Null, or why not (*too_long: the refusal is a length); fills *pl.  The order is the header's.
inline const char* rm_check(const RmArgs& a, const MsTable& regs, bool* too_long, RmPlan* pl) {
    int L, M, K;
    *too_long = false;
    if (const char* e = rs_design(a.rate, &L, &M, &K, nullptr)) return e;
    if (a.n < 1) return "n must be at least 1";
    if (const char* e = rm_regions(regs, a.n)) return e;
    if (a.channel < -1 || a.channel >= a.ir_channels) return "channel outside [-1, channels)";
    if (a.normalize != 0 && a.normalize != 1) return "normalize must be 0 or 1";
    if (a.wet < 0 || a.wet > RM_MAX_SEND) return "wet outside [0, 6000] hundredths of a dB";
    if (a.dry < -1 || a.dry > RM_MAX_SEND) return "dry neither -1 nor in [0, 6000] hundredths of a dB";
    if (a.send < -1 || a.send > RM_MAX_SEND) return "send neither -1 nor in [0, 6000] hundredths of a dB";
    if (a.ceiling != 0 && a.ceiling != 1) return "ceiling must be 0 or 1";
    if (a.live && a.ceiling != 0) return "ceiling must be 0 on a stream: it has no whole-piece peak";
    if (a.offset < 0) return "offset must be >= 0";
    if (a.length < 0) return "length must be >= 0";
    if (a.fade < 0) return "fade must be >= 0";
    if (a.predelay < 0 || a.predelay > a.rate) return "predelay outside [0, sample_rate]";
    if (a.tail < -1) return "tail must be >= -1";
    if (a.n > MX_MAX_N) {
        *too_long = true;
        return "n exceeds 2^28 samples";
    }
    RmPlan p;
    p.nh = a.nh >= 0 ? a.nh : rm_ir_len(a.ir_rate, a.ir_frames, a.rate);
    p.send = regs.R > 0 || a.send != 0;
    if (p.nh < 0) {                            // the item is refused behind these checks, by the intake's own
        if (pl) *pl = p;
        return nullptr;
    }
    if (p.nh - a.offset < 1) return "offset leaves nothing of the impulse response";
    p.L = a.length == 0 ? p.nh - a.offset : std::min(a.length, p.nh - a.offset);
    if (p.L > RM_MAX_L) {
        *too_long = true;
        return "the impulse response exceeds 131072 taps: choose a length";
    }
    p.f = std::min(a.fade, p.L);
    p.tl = a.predelay + p.L - 1;
    if (a.tail > p.tl) return "tail beyond predelay + L - 1";
    if (a.tail >= 0) p.tl = a.tail;
    p.N = a.n + p.tl;
    if (p.N > MX_MAX_N) {
        *too_long = true;
        return "n + tail exceeds 2^28 samples";
    }
    if (pl) *pl = p;
    return nullptr;
}
// Elements of the stage's device buffers: the programme, the sent programme, t and hn, the block energies, the output.
struct RmSizes { size_t x = 0, xs = 0, taps = 0, blocks = 0, y = 0; };
inline RmSizes rm_sizes(const RmArgs& a, const RmPlan& p) {
    RmSizes z;
    z.x = (size_t)a.n;
    z.xs = p.send ? (size_t)a.n : 0;
    z.taps = (size_t)p.L;
    z.blocks = (size_t)((p.L + 255) / 256);
    z.y = (size_t)p.N;
    return z;
}

// ---- live room stage (rooml_*_kernel in room_kernels.h; fishtts_hip.h states it under "Live room"): the room stage on a
// stream.  The chain is causal - output i reads xs[i - predelay - k], k in [0, L) - so a push of n samples behind n_in
// earlier ones emits exactly the outputs [n_in, n_in + n), the final one the tail behind them, and the stream carries the
// last min(n_in, predelay + L - 1) sent samples.  The values of `begin` as rm_check judges them (no programme yet: n = 1
// stands in, and no n of a stream can then fail where rm_check looks at it), the counters of a stream, the bounds of its
// carry, the per-push checks in their order and the sizes of the buffers a push touches (tools/room_live_check.cpp drives
// this block over random cuttings).
inline RmArgs rl_begin_args(RmArgs a) {
    a.n = 1;
    a.live = 1;
    return a;
}
struct RlShape { long long hist = 0, tl = 0; };       // predelay + L - 1; the tail by Room's rule
inline RlShape rl_shape(const RmArgs& a, const RmPlan& p) { return RlShape{a.predelay + p.L - 1, p.tl}; }
// A push on the timeline: it brings the samples [F0, F1) and emits the outputs [F0, end); the carry read holds the sent
// samples [cb0, F0), the one written [cb1, F1) (nothing at the end of the stream).
struct RlPlan { long long in = 0, out = 0, F0 = 0, F1 = 0, end = 0, cb0 = 0, cb1 = 0; bool final = false; };
struct RlStage {
    RlShape s;
    int par = 0;                               // which copy of the carry is current
    bool ended = false;                        // the final push went through
    long long nin = 0, nout = 0, base = 0;     // samples taken, outputs emitted, the first sent sample carried
    static RlStage fresh(const RlShape& shape) {
        RlStage r;
        r.s = shape;
        return r;
    }
    RlPlan plan(long long n, bool final) const {
        RlPlan p;
        p.in = n;
        p.final = final;
        p.F0 = nin;
        p.F1 = nin + n;
        p.end = final ? p.F1 + s.tl : p.F1;
        p.out = p.end - nout;
        p.cb0 = base;
        p.cb1 = final ? p.F1 : std::max(0LL, p.F1 - s.hist);
        return p;
    }
    long long held(const RlPlan& p) const { return p.F1 - p.cb1; }   // carried after the call: at most hist
    void commit(const RlPlan& p) {
        nin = p.F1; nout = p.end; base = p.cb1;
        ended = p.final;
        par ^= 1;
    }
};
// A push judged, in the stated order: a push after the final one (*state), n, the regions - relative to the push, by
// rm_regions over its n - the timeline (*too_long), the capacity.  Null, or why not; nothing of the stage changes.
inline const char* rl_check(const RlStage& st, long long n, const MsTable& regs, bool final, long long capacity, bool* state,
                            bool* too_long) {
    *state = *too_long = false;
    if (st.ended) {
        *state = true;
        return "the stream has had its final push";
    }
    if (n < 0) return "n must be >= 0";
    if (const char* e = rm_regions(regs, n)) return e;
    if (n > MX_MAX_N || st.nin + n + st.s.tl > MX_MAX_N) {
        *too_long = true;
        return "n + tail exceeds 2^28 samples";
    }
    if (capacity < st.plan(n, final).out) return "capacity below what the push emits";
    return nullptr;
}
inline MsRegion rl_shift(const MsRegion& g, long long F0) { return MsRegion{g.a + F0, g.e + F0, g.pan, 0}; }
// Elements a push touches: the staged push and its sent form (one spare where the push is empty: the staging loads once and
// then selects), the output, and each copy of the carry, which a stream allocates once.
struct RlSizes { size_t x = 0, xs = 0, y = 0, carry = 0; };
inline RlSizes rl_sizes(const RlStage& st, const RlPlan& p) {
    RlSizes z;
    z.x = z.xs = (size_t)std::max(p.in, 1LL);
    z.y = (size_t)std::max(p.out, 1LL);
    z.carry = (size_t)std::max(st.s.hist, 1LL);
    return z;
}
// The sent sample at timeline index g as the chain's staging picks it: which buffer (0: the carry, 1: the push, -1: +0.0)
// and the element in it - clamped into the buffer even where the value is then not taken.
struct RlPick { int buf = -1; long long at = 0; bool taken = false; };
inline RlPick rl_pick(const RlPlan& p, long long g) {
    const bool old = g < p.F0;
    const long long lo = old ? p.cb0 : p.F0, hi = old ? p.F0 : p.F1;
    RlPick k;
    k.buf = old ? 0 : 1;
    k.at = std::min(std::max(g, lo), std::max(hi - 1, lo)) - lo;
    k.taken = g >= lo && g < hi;
    return k;
}

// ---- the stages of one waveform, in chain order.  A stage takes `in` more input samples in a call and emits `out`;
// plan() says how many (nothing changes), the caller builds the stage's segment from the record and the plan, and commit()
// advances the record once the call went through.  An absent stage passes its input on (out = in); its counters still run,
// the parity of its carry pair too.  A record with null carries and zero counters is a waveform decoded from zero state.
struct StagePlan { long long in = 0, out = 0, base = 0; int k1 = 0; };   // base, k1: the time-scale stage's (TsPlan)

struct TsStage {
    bool on = false;
    TsRate rate;
    float *carry[2] = {nullptr, nullptr}, *state[2] = {nullptr, nullptr};   // input a later frame still reads; state after the last frame
    int par = 0, k = 0;                        // which copy is current; frames run so far
    long long nin = 0, base = 0, nout = 0;     // input samples seen, first one carried, samples emitted
    StagePlan plan(long long n, bool final) const {
        if (!on) return StagePlan{n, n, 0, 0};
        const TsPlan p = ts_plan(rate, k, nin + n, final);
        return StagePlan{n, p.out - nout, p.base, p.k1};
    }
    long long held(const StagePlan& p) const { return on ? nin + p.in - p.base : 0; }   // carried after the call: at most TS_CARRY
    void commit(const StagePlan& p) {
        if (!on) return;
        nin += p.in; nout += p.out; base = p.base; k = p.k1; par ^= 1;
    }
};

struct PsStage {
    const PsTab* tab = nullptr;                // null: absent
    float* carry[2] = {nullptr, nullptr};      // its last K input samples
    int par = 0;
    long long nin = 0, nout = 0;
    // `total`: the outputs the stage gives in the end for the codec samples seen so far (it restores the caller's length)
    StagePlan plan(long long n, bool final, long long total) const {
        return StagePlan{n, tab ? ps_ready(*tab, nin + n, final, total) - nout : n, 0, 0};
    }
    void commit(const StagePlan& p) {
        if (!tab) return;
        nin += p.in; nout += p.out; par ^= 1;
    }
};

struct RsStage {
    const RsTab* tab = nullptr;                // null: absent (the codec's own rate)
    float* carry[2] = {nullptr, nullptr};      // its last K input samples
    int par = 0;
    long long nin = 0, nout = 0;
    StagePlan plan(long long n, bool final) const { return StagePlan{n, tab ? rs_ready(*tab, nin + n, final) - nout : n, 0, 0}; }
    void commit(const StagePlan& p) { nin += p.in; nout += p.out; par ^= 1; }
};

// The ride stage of a stream: `in` more samples, `out` emitted; hops, peaks and nodes are the totals after the call.
struct RdStage {
    int target = 0, rate = RS_FI, H = 1;       // target 0: absent; the output rate and its hop
    float* carry[2] = {nullptr, nullptr};      // the samples from `base` on (fewer than (RD_A + 1) H)
    double *e = nullptr, *v = nullptr;         // on the device, per stream: hop sums, v_k
    float *p = nullptr, *g = nullptr;          // hop peaks, nodes g_k
    int par = 0, hops = 0, peaks = 0, nodes = 0;
    long long nin = 0, nout = 0, base = 0;
    RdPlan plan(long long n, bool final) const {
        RdPlan q;
        if (target == 0) { q.in = q.out = n; return q; }
        q = rd_plan(H, nin + n, final);
        q.in = n;
        q.out -= nout;
        return q;
    }
    long long held(const RdPlan& q) const { return target != 0 ? nin + q.in - q.base : 0; }   // carried after the call: below (RD_A + 1) H
    void commit(const RdPlan& q) {
        if (target == 0) return;
        nin += q.in; nout += q.out; base = q.base; hops = q.hops; peaks = q.peaks; nodes = q.nodes; par ^= 1;
    }
};

struct ChainPlan { StagePlan ts, ps, rs; RdPlan rd; };
struct StageChain {
    TsStage ts;
    PsStage ps;
    RsStage rs;
    RdStage rd;
    int speed = 100;          // the caller's speed_pct: with the codec samples seen it fixes the pitch stage's output length
    long long seen = 0;       // codec samples taken so far
    bool any() const { return ts.on || ps.tab || rs.tab || rd.target != 0; }
    ChainPlan plan(long long n, bool final) const {
        ChainPlan p;
        p.ts = ts.plan(n, final);
        p.ps = ps.plan(p.ts.out, final, ts_len(speed, seen + n));
        p.rs = rs.plan(p.ps.out, final);
        p.rd = rd.plan(p.rs.out, final);
        return p;
    }
    void commit(const ChainPlan& p) {
        seen += p.ts.in;
        ts.commit(p.ts);
        ps.commit(p.ps);
        rs.commit(p.rs);
        rd.commit(p.rd);
    }
};

// A call's chain, resolved: which stages exist and at what rate.  make() judges the values as every entry point does
// (an error message, or null): the rate, then the speed, then the cents, then the pair, then the level, then the ride stage's
// target.  The device tables are filled in by
// the caller that holds the context (codec.hip: fx_prepare).
struct FxDesc {
    int rate = RS_FI, pct = 100, cents = 0, level = 0;   // level: the target in hundredths of a LUFS, 0: no level stage
    int live = 0;                     // the ride stage's target (a stream's), 0: no ride stage
    int L = 1, M = 1, K = 0;          // the resampler's (K = 0: the codec's own rate, no stage)
    FxPlan f;                         // f.has_ts: the time-scale stage exists (under a pitch shift it may not)
    const RsTab* rs = nullptr;        // set by the caller when K > 0
    const PsTab* ps = nullptr;        // set by the caller when cents != 0
    enum Bad { OK = 0, RATE, SPEED, CENTS, PAIR, LEVEL, LIVE };
    Bad make(int rate_, int pct_, int cents_, const char** why) { return make(rate_, pct_, cents_, 0, why); }
    Bad make(int rate_, int pct_, int cents_, int level_, int live_, const char** why) {
        const Bad b = make(rate_, pct_, cents_, level_, why);
        live = live_;
        return b != OK ? b : rd_ok(live) ? OK : LIVE;
    }
    Bad make(int rate_, int pct_, int cents_, int level_, const char** why) {
        rate = rate_; pct = pct_; cents = cents_; level = level_; live = 0;
        if ((*why = rs_design(rate, &L, &M, &K, nullptr))) return RATE;
        if (!ts_ok(pct)) return SPEED;
        if (cents < -PS_MAX_CENTS || cents > PS_MAX_CENTS) return CENTS;
        if (!fx_plan(pct, cents, &f)) return PAIR;
        return lv_ok(level) ? OK : LEVEL;
    }
    bool any() const { return K > 0 || f.has_ts || cents != 0 || live != 0; }
    // a waveform from zero state through this chain
    StageChain fresh() const {
        StageChain c;
        c.ts.on = f.has_ts;
        c.ts.rate = f.ts;
        c.ps.tab = ps;
        c.rs.tab = K > 0 ? rs : nullptr;
        c.speed = pct;
        c.rd.target = live;
        c.rd.rate = rate;
        c.rd.H = lv_hop(rate);
        return c;
    }
    // n_in codec samples -> after the time-scale and pitch stages -> after the resampler (ft_resampled_len of ft_timescaled_len)
    long long ts_out(long long n_in) const { return ts_len(pct, n_in); }
    long long out_len(long long n_in) const { return (ts_out(n_in) * L + M - 1) / M; }
};

}  // namespace chain
}  // namespace ft
