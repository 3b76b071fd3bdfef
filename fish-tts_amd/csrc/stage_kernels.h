// The output stages' kernels for gfx950, each behind the stage's statement: the resampler, the reference intake, the
// time-scale, pitch, join, level and ride stages, the mix and the live mix stage.  They work on f32 audio and share nothing
// with the codec model's kernels (codec_kernels.h); the stereo mix stages and the room stage build on them in
// stereo_kernels.h and room_kernels.h.  codec.hip launches these kernels; engine.hip includes the header too and launches
// none of them ("Kernel headers"), so a kernel added or changed here moves the AR engine's code: new
// stages go into a header of their own, as those two did.
#pragma once
#include <float.h>
#include <limits.h>

#include "common.h"

namespace ft {

// ---- polyphase FIR resampler (ft_codec_decode_at, ft_codec_stream_decode_many_at): from the codec rate Fi to Fo = Fi L / M.
// Output n is the value at input time n M / L (zero phase): with u = n M, i0 = u / L, p = u % L,
//   y[n] = sum_{t < K} w[p][t] * x[i0 - K/2 + 1 + t],
// summed in f32 in this order whatever the chunking and however many segments share the launch.  A segment is one stream's
// (or one utterance's) part of the call; it sits on blockIdx.z.  Input indices below the segment's first sample come from
// its carry (the K samples before it; none: zeros), indices past its last one are zeros (the final tail).  The block
// stages its outputs' input window in LDS: (255 M + L - 1) / L + K + 1 <= RS_LDS is checked with the table.
struct RsSeg {
    const float* x;          // input samples [nin, nin + n_in) (device; unused when n_in = 0)
    const float* w;          // [L][K]; null: the native rate, y = x
    const float* carry_rd;   // input samples [nin - K, nin); null: zeros
    float* carry_wr;         // receives input samples [nin + n_in - K, nin + n_in); null: not kept
    float* y;                // outputs [nout, nout + n_out)
    long long nin, nout;
    int n_in, n_out, L, M, K, pad;
};
constexpr int RS_THREADS = 256, RS_LDS = 2048;

__device__ inline float rs_in(const RsSeg& s, long long i) {
    if (i < s.nin) {
        const long long c = i - (s.nin - s.K);
        return s.carry_rd && c >= 0 ? s.carry_rd[c] : 0.f;
    }
    if (i < s.nin + s.n_in) return s.x[i - s.nin];
    return 0.f;
}

static __global__ __launch_bounds__(RS_THREADS) void resample_kernel(const RsSeg* segs) {
    __shared__ float xs[RS_LDS];
    const RsSeg s = segs[blockIdx.z];
    if (!s.w) {
        for (long i = (long)blockIdx.x * RS_THREADS + threadIdx.x; i < s.n_out; i += (long)gridDim.x * RS_THREADS) s.y[i] = s.x[i];
        return;
    }
    // the carry of the next call: a buffer this launch does not read (double-buffered by the caller)
    if (blockIdx.x == 0 && s.carry_wr) {
        const long long e = s.nin + s.n_in - s.K;
        for (int k = threadIdx.x; k < s.K; k += RS_THREADS) s.carry_wr[k] = rs_in(s, e + k);
    }
    const int h = s.K / 2;
    for (long b0 = (long)blockIdx.x * RS_THREADS; b0 < s.n_out; b0 += (long)gridDim.x * RS_THREADS) {
        const long long na = s.nout + b0, nb = s.nout + min((long)s.n_out, b0 + RS_THREADS) - 1;
        const long long ia = na * s.M / s.L - h + 1;
        const int span = (int)(nb * s.M / s.L + h - ia + 1);
        __syncthreads();
        for (int k = threadIdx.x; k < span && k < RS_LDS; k += RS_THREADS) xs[k] = rs_in(s, ia + k);
        __syncthreads();
        const long n = b0 + threadIdx.x;
        if (n < s.n_out) {
            const long long u = (s.nout + n) * s.M, i0 = u / s.L;
            const float* wp = s.w + (size_t)(u - i0 * s.L) * s.K;
            const float* xp = xs + (i0 - h + 1 - ia);
            float acc = 0.f;
            for (int t = 0; t < s.K; ++t) acc += wp[t] * xp[t];
            s.y[n] = acc;
        }
    }
}

// ---- reference intake (ft_codec_intake, ft_codec_encode_items; stated in fishtts_hip.h): the raw frames of a WAV - any of
// five sample formats, one to eight interleaved channels, any accepted rate - decoded, mixed down to mono and brought to
// the codec's rate in ONE launch for all clips of a call (the clip sits on blockIdx.z).  The launch has the shape of
// resample_kernel: a workgroup computes 256 consecutive outputs from an input window staged in LDS, the polyphase sum in
// float32 over t ascending; the difference is where the window comes from - each staged element is one frame, decoded and
// mixed from the clip's bytes, so no mono copy at the input rate ever exists.  (255 M + L - 1) / L + K + 1 <= RS_LDS is
// checked with the table (rs_design_in).
// Loads: a clip starts on a 16-byte boundary of the raw buffer, so every 2- and 4-byte sample is naturally aligned and is
// read with one load of its size; a 24-bit sample has no alignment at all and is read as three bytes.  Lane k of a wave
// stages frame ia + k: the lanes' addresses are C width bytes apart, so a wave's loads of one channel cover one contiguous
// run of 64 C width bytes, and the C loads of a lane hit the lines its neighbours just fetched.  A 30 s stereo 48 kHz clip
// is 5.8 MB, read K / 256 M/L + 1 times over (the windows of adjacent workgroups overlap by K frames) out of L2.
// The two counters are integer atomics, one pair per workgroup that saw something: every frame is counted by exactly one
// workgroup - the one whose outputs' centre taps start at it, frames [floor(na M / L), floor((nb + 1) M / L)) for outputs
// [na, nb], the last workgroup to the end of the clip - and those frames lie inside its window (M / L < 5 <= K / 2).
enum { IN_U8 = 0, IN_S16 = 1, IN_S24 = 2, IN_S32 = 3, IN_F32 = 4 };
struct IntakeSeg {
    const unsigned char* raw;     // n_frames frames of `channels` samples, interleaved, little-endian (device, 16-byte aligned)
    const float* w;               // [L][K]; null: the codec's own rate, y = m
    float* y;                     // n_out outputs
    unsigned long long* count;    // [2]: clipped, nonfinite (zeroed by the host before the launch)
    long long n_frames, n_out;
    int L, M, K, fmt, channels, channel;   // channel < 0: the mean of all channels
};
constexpr int IN_WIDTH[5] = {1, 2, 3, 4, 4};

// Sample `c` of frame `i` as a real number (exact in float64); `clip`, `bad`: the sample sits at an extreme code (f32:
// |v| >= 1), is not finite (and counts as 0).
__device__ inline double intake_sample(const IntakeSeg& s, long long i, int c, int& clip, int& bad) {
    const long long at = i * s.channels + c;
    switch (s.fmt) {
    case IN_U8: {
        const int v = s.raw[at];
        clip += v == 0 || v == 255;
        return (double)(v - 128) / 128.0;
    }
    case IN_S16: {
        const int v = ((const short*)s.raw)[at];
        clip += v == -32768 || v == 32767;
        return (double)v / 32768.0;
    }
    case IN_S24: {
        const unsigned char* q = s.raw + 3 * at;
        const int v = ((int)((unsigned)q[0] << 8 | (unsigned)q[1] << 16 | (unsigned)q[2] << 24)) >> 8;
        clip += v == -8388608 || v == 8388607;
        return (double)v / 8388608.0;
    }
    case IN_S32: {
        const int v = ((const int*)s.raw)[at];
        clip += v == INT_MIN || v == INT_MAX;
        return (double)v / 2147483648.0;
    }
    default: {
        const float v = ((const float*)s.raw)[at];
        if (!(fabsf(v) <= FLT_MAX)) {      // inf or NaN
            bad += 1;
            return 0.0;
        }
        clip += fabsf(v) >= 1.f;
        return (double)v;
    }
    }
}

// m[i]: the mono sample of frame i, zero outside the clip; `own`: this workgroup counts the frame.
__device__ inline float intake_mono(const IntakeSeg& s, long long i, bool own, int& clip, int& bad) {
    if (i < 0 || i >= s.n_frames) return 0.f;
    int cl = 0, bd = 0;
    float m;
    if (s.channel >= 0) {
        m = (float)intake_sample(s, i, s.channel, cl, bd);
    } else {
        double sum = 0.0;
        for (int c = 0; c < s.channels; ++c) sum += intake_sample(s, i, c, cl, bd);
        m = (float)(sum / (double)s.channels);
    }
    if (own) {
        clip += cl;
        bad += bd;
    }
    return m;
}

static __global__ __launch_bounds__(RS_THREADS) void intake_kernel(const IntakeSeg* segs) {
    __shared__ float xs[RS_LDS];
    __shared__ int tot[2];
    const IntakeSeg s = segs[blockIdx.z];
    int clip = 0, bad = 0;
    if (threadIdx.x < 2) tot[threadIdx.x] = 0;
    if (!s.w) {
        for (long long i = (long long)blockIdx.x * RS_THREADS + threadIdx.x; i < s.n_out; i += (long long)gridDim.x * RS_THREADS)
            s.y[i] = intake_mono(s, i, true, clip, bad);
    } else {
        const int h = s.K / 2;
        for (long long b0 = (long long)blockIdx.x * RS_THREADS; b0 < s.n_out; b0 += (long long)gridDim.x * RS_THREADS) {
            const long long na = b0, nb = min(s.n_out, b0 + RS_THREADS) - 1;
            const long long ia = na * s.M / s.L - h + 1;
            const int span = (int)(nb * s.M / s.L + h - ia + 1);
            const long long own_a = na * s.M / s.L, own_b = nb + 1 == s.n_out ? s.n_frames : (nb + 1) * s.M / s.L;
            __syncthreads();
            for (int k = threadIdx.x; k < span && k < RS_LDS; k += RS_THREADS)
                xs[k] = intake_mono(s, ia + k, ia + k >= own_a && ia + k < own_b, clip, bad);
            __syncthreads();
            const long long n = b0 + threadIdx.x;
            if (n < s.n_out) {
                const long long u = n * s.M, i0 = u / s.L;
                const float* wp = s.w + (size_t)(u - i0 * s.L) * s.K;
                const float* xp = xs + (i0 - h + 1 - ia);
                float acc = 0.f;
                for (int t = 0; t < s.K; ++t) acc += wp[t] * xp[t];
                s.y[n] = acc;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        clip += __shfl_xor(clip, o);
        bad += __shfl_xor(bad, o);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        if (clip) atomicAdd(&tot[0], clip);
        if (bad) atomicAdd(&tot[1], bad);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (tot[0]) atomicAdd(&s.count[0], (unsigned long long)tot[0]);
        if (tot[1]) atomicAdd(&s.count[1], (unsigned long long)tot[1]);
    }
}

// ---- WSOLA time-scale stage (ft_codec_decode_fx, ft_codec_stream_begin_fx; the algorithm is stated in fishtts_hip.h): at the
// codec rate, at the rational rate num / den (a speed alone: pct / 100; under a pitch shift pct 2^20 / (100 S), see PsSeg).
// Frame k lies at a_k = floor(k HS num / den); it reads x[s_k + i], i < N, with
// s_k = a_k - HS + d_k, and adds w[i] x[s_k + i] to output (k - 1) HS + i.  d_k in [-D, D] maximises the plain
// cross-correlation of the frame with the continuation of frame k - 1, x[s_{k-1} + HS + i]; the lowest d wins a tie.
// The frames of a segment depend on each other through d_{k-1}: one workgroup walks one segment's frames in order, the
// segments of a call sit on blockIdx.x.  Per frame the template (N floats) and the search region (N + 2 D floats) are staged
// in LDS; a thread holds four adjacent candidates in registers, so one 16-byte read of the region and one of the template
// (a broadcast) feed sixteen fused multiply-adds, each sum over i ascending.  The argmax is a wave, then a workgroup reduction
// over (value, index), the lower index winning on equal values.
// A stream's part of a call: input indices in [cbase_rd, nin) come from its carry, [nin, nin + n_in) from x, the rest is
// zero (before the first sample; past the last one in the final call - the host runs no frame earlier whose reads reach
// past the input seen).  It reads one copy of its carry and state (s_{k-1}, the HS half-overlapped outputs) and writes
// the other.
constexpr int TS_N = 1024, TS_HS = 512, TS_D = 384, TS_THREADS = 256;
constexpr int TS_REG = TS_N + 2 * TS_D, TS_CAND = 2 * TS_D + 1;
constexpr int TS_CARRY = TS_N + 2 * TS_D + 2 * TS_HS;   // most input samples a stream carries
constexpr int TS_STATE = TS_HS + 4;                     // floats of a state copy: the overlap, then s_{k-1} (an int)
struct TsSeg {
    const float* x;          // input samples [nin, nin + n_in) (device; unused when n_in = 0)
    const float* carry_rd;   // input samples [cbase_rd, nin); null: none
    float* carry_wr;         // receives input samples [cbase_wr, nin + n_in); null: not kept
    const float* st_rd;      // state after frame k0 - 1; null: a fresh input (k0 = 0)
    float* st_wr;            // state after frame k1 - 1; null: not kept
    float* y;                // outputs [emit0, emit0 + n_out)
    int* deltas;             // d_k of frames [k0, k1) (the test hook); null: not kept
    long long nin, cbase_rd, cbase_wr, emit0;
    long long num, den;      // the rate num / den: a_k = floor(k HS num / den) (a speed alone: pct / 100)
    int n_in, n_out, k0, k1, rsi, pad;   // rsi: host side only, the stream of the call whose next stage reads y
};

__device__ inline float ts_in(const TsSeg& s, long long i) {
    if (i < s.nin) return s.carry_rd && i >= s.cbase_rd ? s.carry_rd[i - s.cbase_rd] : 0.f;   // (i < 0: cbase_rd >= 0)
    if (i < s.nin + s.n_in) return s.x[i - s.nin];
    return 0.f;
}

static __global__ __launch_bounds__(TS_THREADS) void timescale_kernel(const TsSeg* segs, const float* win) {
    __shared__ __attribute__((aligned(16))) float tpl[TS_N];
    __shared__ __attribute__((aligned(16))) float reg[TS_REG + 8];   // 8 zeros behind it: the last thread's 16-byte reads
    __shared__ float ola[TS_HS];
    __shared__ float rv[TS_THREADS / 64];
    __shared__ int ri[TS_THREADS / 64];
    const TsSeg s = segs[blockIdx.x];
    const int t = threadIdx.x;
    for (int i = t; i < TS_HS; i += TS_THREADS) ola[i] = s.st_rd ? s.st_rd[i] : 0.f;   // thread t owns ola[t], ola[t + 256]
    if (t < 8) reg[TS_REG + t] = 0.f;
    int sprev = s.st_rd ? *reinterpret_cast<const int*>(s.st_rd + TS_HS) : 0;
    for (int k = s.k0; k < s.k1; ++k) {
        const long long a = (long long)k * TS_HS * s.num / s.den;
        __syncthreads();   // the frame before has read reg, rv, ri
        for (int i = t; i < TS_REG; i += TS_THREADS) reg[i] = ts_in(s, a - TS_HS - TS_D + i);
        int c = TS_D;      // d_0 = 0
        if (k > 0) {
            for (int i = t; i < TS_N; i += TS_THREADS) tpl[i] = ts_in(s, (long long)sprev + TS_HS + i);
            __syncthreads();
            float bv = -INFINITY;
            int bi = TS_CAND;
            const int cb = 4 * t;   // candidates cb .. cb + 3
            if (cb < TS_CAND) {
                const float4* R4 = reinterpret_cast<const float4*>(reg + cb);
                const float4* T4 = reinterpret_cast<const float4*>(tpl);
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                float4 lo = R4[0];
#pragma unroll 2
                for (int j = 0; j < TS_N / 4; ++j) {
                    const float4 hi = R4[j + 1], v = T4[j];
                    a0 = __builtin_fmaf(v.x, lo.x, a0); a1 = __builtin_fmaf(v.x, lo.y, a1); a2 = __builtin_fmaf(v.x, lo.z, a2); a3 = __builtin_fmaf(v.x, lo.w, a3);
                    a0 = __builtin_fmaf(v.y, lo.y, a0); a1 = __builtin_fmaf(v.y, lo.z, a1); a2 = __builtin_fmaf(v.y, lo.w, a2); a3 = __builtin_fmaf(v.y, hi.x, a3);
                    a0 = __builtin_fmaf(v.z, lo.z, a0); a1 = __builtin_fmaf(v.z, lo.w, a1); a2 = __builtin_fmaf(v.z, hi.x, a2); a3 = __builtin_fmaf(v.z, hi.y, a3);
                    a0 = __builtin_fmaf(v.w, lo.w, a0); a1 = __builtin_fmaf(v.w, hi.x, a1); a2 = __builtin_fmaf(v.w, hi.y, a2); a3 = __builtin_fmaf(v.w, hi.z, a3);
                    lo = hi;
                }
                const float av[4] = {a0, a1, a2, a3};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (cb + q < TS_CAND && av[q] > bv) { bv = av[q]; bi = cb + q; }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const float ov = __shfl_down(bv, off);
                const int oi = __shfl_down(bi, off);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if ((t & 63) == 0) { rv[t >> 6] = bv; ri[t >> 6] = bi; }
            __syncthreads();
            bv = rv[0];
            bi = ri[0];
#pragma unroll
            for (int w = 1; w < TS_THREADS / 64; ++w)
                if (rv[w] > bv || (rv[w] == bv && ri[w] < bi)) { bv = rv[w]; bi = ri[w]; }
            c = bi < TS_CAND ? bi : TS_D;   // (no finite sum: keep d = 0)
        } else {
            __syncthreads();
        }
        // overlap-add: outputs [(k - 1) HS, k HS) are final now; the second half waits for frame k + 1
        const long long p0 = (long long)(k - 1) * TS_HS - s.emit0;
        for (int i = t; i < TS_HS; i += TS_THREADS) {
            const float v = ola[i] + win[i] * reg[c + i];
            const long long p = p0 + i;
            if (k > 0 && p >= 0 && p < s.n_out) s.y[p] = v;
            ola[i] = win[i + TS_HS] * reg[c + i + TS_HS];
        }
        sprev = (int)(a - TS_HS) + c - TS_D;
        if (t == 0 && s.deltas) s.deltas[k - s.k0] = c - TS_D;
    }
    if (s.carry_wr) {
        const int n = (int)(s.nin + s.n_in - s.cbase_wr);
        for (int i = t; i < n && i < TS_CARRY; i += TS_THREADS) s.carry_wr[i] = ts_in(s, s.cbase_wr + i);
    }
    if (s.st_wr) {
        for (int i = t; i < TS_HS; i += TS_THREADS) s.st_wr[i] = ola[i];
        if (t == 0) *reinterpret_cast<int*>(s.st_wr + TS_HS) = sprev;
    }
}

// ---- pitch stage (ft_codec_decode_fxp, ft_codec_stream_begin_fxp; stated in fishtts_hip.h): an arbitrary-ratio resampler
// that reads its input faster by r = S / 2^20 and calls the result the same rate, behind a time-scale stage that stretched
// the waveform by r.  Output n is the input at time n S / 2^20: with u = n S, i0 = u >> 20, p = (u >> 11) & 511,
// f = (u & 2047) / 2048,
//   y[n] = sum_{t < K} ((1 - f) w[p][t] + f w[p + 1][t]) * x[i0 - K/2 + 1 + t],
// w [513][K] a Kaiser-windowed sinc at 512 phases per input sample (row 512: row 0 one tap on), linearly interpolated
// between adjacent rows; summed in f32 over t ascending whatever the chunking and however many segments share the launch.
// Segments, carry and the LDS stage as the resampler's: a block's 256 outputs span at most 255 * 2 + 2 inputs (r <= 2) plus
// K <= 134 taps, well inside RS_LDS.
struct PsSeg {
    const float* x;          // input samples [nin, nin + n_in) (device; unused when n_in = 0)
    const float* w;          // [513][K]
    const float* carry_rd;   // input samples [nin - K, nin); null: zeros
    float* carry_wr;         // receives input samples [nin + n_in - K, nin + n_in); null: not kept
    float* y;                // outputs [nout, nout + n_out)
    long long nin, nout, step;   // step: S
    int n_in, n_out, K, rsi;     // rsi: host side only, the stream of the call whose resampler segment reads y
};
constexpr int PS_SHIFT = 20, PS_PHASES = 512, PS_FRAC = 2048;

__device__ inline float ps_in(const PsSeg& s, long long i) {
    if (i < s.nin) {
        const long long c = i - (s.nin - s.K);
        return s.carry_rd && c >= 0 ? s.carry_rd[c] : 0.f;
    }
    if (i < s.nin + s.n_in) return s.x[i - s.nin];
    return 0.f;
}

static __global__ __launch_bounds__(RS_THREADS) void pitch_kernel(const PsSeg* segs) {
    __shared__ float xs[RS_LDS];
    const PsSeg s = segs[blockIdx.z];
    if (blockIdx.x == 0 && s.carry_wr) {
        const long long e = s.nin + s.n_in - s.K;
        for (int k = threadIdx.x; k < s.K; k += RS_THREADS) s.carry_wr[k] = ps_in(s, e + k);
    }
    const int h = s.K / 2;
    for (long b0 = (long)blockIdx.x * RS_THREADS; b0 < s.n_out; b0 += (long)gridDim.x * RS_THREADS) {
        const long long na = s.nout + b0, nb = s.nout + min((long)s.n_out, b0 + RS_THREADS) - 1;
        const long long ia = ((na * s.step) >> PS_SHIFT) - h + 1;
        const int span = (int)(((nb * s.step) >> PS_SHIFT) + h - ia + 1);
        __syncthreads();
        for (int k = threadIdx.x; k < span && k < RS_LDS; k += RS_THREADS) xs[k] = ps_in(s, ia + k);
        __syncthreads();
        const long n = b0 + threadIdx.x;
        if (n < s.n_out) {
            const long long u = (s.nout + n) * s.step, i0 = u >> PS_SHIFT;
            const int p = (int)(u >> 11) & (PS_PHASES - 1);
            const float f = (float)(int)(u & (PS_FRAC - 1)) / (float)PS_FRAC, g = 1.f - f;
            const float* w0 = s.w + (size_t)p * s.K;
            const float* w1 = w0 + s.K;
            const float* xp = xs + (i0 - h + 1 - ia);
            float acc = 0.f;
            for (int t = 0; t < s.K; ++t) acc += (g * w0[t] + f * w1[t]) * xp[t];
            s.y[n] = acc;
        }
    }
}

// ---- join stage (ft_codec_decode_join, ft_test_join; stated in fishtts_hip.h): the items of a call - whole utterances at
// the output rate, left on the device by the stages above - trimmed to their loud part, faded and laid out behind their
// gaps as one waveform.  Three launches whatever the number of items (the item is blockIdx.z of a device table):
//   join_edges_kernel     first / last loud window of every item: per thread over its samples (16-byte loads: the items
//                         lie on 16-byte boundaries of the input buffer), per wave by shuffles, per workgroup through
//                         LDS, then one atomicMin / atomicMax per workgroup that saw a loud sample (at most
//                         JOIN_EDGE_BLOCKS per item: at the default threshold nearly every wave sees one, and with
//                         one pair of atomics per wave on the same two words the launch took 56 us for 12 items of
//                         246 000 samples)
//   join_layout_kernel    one workgroup: cuts and fade lengths per item, then the running offsets (at most 64 items)
//   join_assemble_kernel  the output: 16-byte stores on the aligned groups of every item's destination range; the source
//                         offset a_b is arbitrary, so each lane loads its four samples with four 4-byte loads (lanes 16
//                         bytes apart: a wave's loads together cover one contiguous 1 KiB run); scalar stores on the up
//                         to three samples at either end
struct JoinItem {
    const float* x;            // the item's samples (device, 16-byte aligned)
    long long n, gap;          // samples; zeros in front of the piece (when something precedes it)
    int first, last;           // loud windows: the host sets INT_MAX / -1, join_edges_kernel reduces into them
    long long a, e, f, G, off; // join_layout_kernel: cut positions, fade length, the gap that counts, output offset of the gap
};
struct JoinTab {
    long long total;           // out: samples of the whole output
    long long cuts[2 * 64];    // out: (a_b, e_b) per item; `total` and `cuts` are what the host reads back
    int started, B;
    JoinItem it[64];
};
constexpr int JOIN_THREADS = 256, JOIN_EDGE_BLOCKS = 64;

__device__ inline void join_loud(float v, float thr, long long i, int hop, int& lo, int& hi) {
    if (fabsf(v) >= thr) {     // (false for a NaN)
        const int w = (int)(i / hop);
        lo = min(lo, w);
        hi = max(hi, w);
    }
}

static __global__ __launch_bounds__(JOIN_THREADS) void join_edges_kernel(JoinTab* tab, float thr, int hop) {
    JoinItem& it = tab->it[blockIdx.z];
    const long long n = it.n, n4 = n >> 2;
    const float4* x4 = (const float4*)it.x;
    int lo = INT_MAX, hi = -1;
    for (long long q = (long long)blockIdx.x * JOIN_THREADS + threadIdx.x; q < n4; q += (long long)gridDim.x * JOIN_THREADS) {
        const float4 v = x4[q];
        join_loud(v.x, thr, 4 * q, hop, lo, hi);
        join_loud(v.y, thr, 4 * q + 1, hop, lo, hi);
        join_loud(v.z, thr, 4 * q + 2, hop, lo, hi);
        join_loud(v.w, thr, 4 * q + 3, hop, lo, hi);
    }
    if (blockIdx.x == 0 && 4 * n4 + threadIdx.x < n) join_loud(it.x[4 * n4 + threadIdx.x], thr, 4 * n4 + threadIdx.x, hop, lo, hi);
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    __shared__ int wlo[JOIN_THREADS / 64], whi[JOIN_THREADS / 64];
    if ((threadIdx.x & 63) == 0) {
        wlo[threadIdx.x >> 6] = lo;
        whi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < JOIN_THREADS / 64; ++w) {
            lo = min(lo, wlo[w]);
            hi = max(hi, whi[w]);
        }
        if (hi >= 0) {      // all of an item's workgroups meet on these two words: one pair of atomics per workgroup
            atomicMin(&it.first, lo);
            atomicMax(&it.last, hi);
        }
    }
}

static __global__ __launch_bounds__(64) void join_layout_kernel(JoinTab* tab, int hop, int keep, int fade) {
    const int B = tab->B, b = threadIdx.x;
    if (b < B) {
        JoinItem& it = tab->it[b];
        long long a = 0, e = 0;
        if (it.last >= 0) {
            a = max(0LL, (long long)it.first * hop - keep);
            e = min(it.n, ((long long)it.last + 1) * hop + keep);
        }
        it.a = tab->cuts[2 * b] = a;
        it.e = tab->cuts[2 * b + 1] = e;
        it.f = min((long long)fade, (e - a) / 2);
    }
    __syncthreads();
    if (b == 0) {
        bool s = tab->started != 0;
        long long off = 0;
        for (int c = 0; c < B; ++c) {
            JoinItem& it = tab->it[c];
            const long long m = it.e - it.a, G = m > 0 && s ? it.gap : 0;
            it.G = G;
            it.off = off;
            off += G + m;
            s = s || m > 0;
        }
        tab->total = off;
    }
}

// Output sample d of an item's range [off, off + G + m): a zero of the gap, or piece sample i with its ramp.
__device__ inline float join_sample(const JoinItem& it, const float* x, long long m, double den, long long d) {
    const long long i = d - it.off - it.G;
    if (i < 0) return 0.f;
    float v = x[i];
    if (i < it.f) v = v * (float)((double)(2 * i + 1) / den);
    else if (i >= m - it.f) v = v * (float)((double)(2 * (m - 1 - i) + 1) / den);
    return v;
}

static __global__ __launch_bounds__(JOIN_THREADS) void join_assemble_kernel(const JoinTab* tab, float* y) {
    const JoinItem it = tab->it[blockIdx.z];
    const long long m = it.e - it.a, d0 = it.off, d1 = d0 + it.G + m;
    if (d1 == d0) return;
    const float* x = it.x + it.a;
    const double den = (double)(2 * it.f);
    // whole 16-byte groups [4 q0, 4 q1) of y inside [d0, d1); head [d0, hb) and tail [te, d1) hold at most 3 samples each
    const long long q0 = (d0 + 3) >> 2, q1 = d1 >> 2, hb = min(d1, 4 * q0), te = max(hb, 4 * q1);
    for (long long q = q0 + (long long)blockIdx.x * JOIN_THREADS + threadIdx.x; q < q1; q += (long long)gridDim.x * JOIN_THREADS) {
        float4 v;
        v.x = join_sample(it, x, m, den, 4 * q);
        v.y = join_sample(it, x, m, den, 4 * q + 1);
        v.z = join_sample(it, x, m, den, 4 * q + 2);
        v.w = join_sample(it, x, m, den, 4 * q + 3);
        ((float4*)y)[q] = v;
    }
    if (blockIdx.x == 0) {
        const long long t = threadIdx.x;
        if (d0 + t < hb) y[d0 + t] = join_sample(it, x, m, den, d0 + t);
        if (te + t < d1) y[te + t] = join_sample(it, x, m, den, te + t);
    }
}

// ---- level stage (ft_codec_loudness, ft_codec_decode_level, ft_codec_decode_join_level, ft_codec_decode_join_items; stated in
// fishtts_hip.h): the items
// of a call - whole utterances at the output rate, left on the device by the stages above - each measured (BS.1770
// integrated loudness, sample peak) and multiplied by one gain, in place.  Three launches whatever the number of items (the
// item is blockIdx.z of a device table):
//   level_filter_kernel   one lane per hop of H samples: it runs the two K-weighting biquads in float64 from zero state
//                         LV_WARM hops before its own (or from sample 0) and leaves the sum of z^2 and the peak of |x| over
//                         its hop.  No scan and no hand-over of state: the high-pass's double pole has decayed by e^-48
//                         over the 0.2 s of warm-up at every rate.  A lane's sum runs over its samples ascending, so the
//                         hop sums do not depend on the grid.  Lanes of a wave read streams H samples apart (each lane
//                         its own cache lines), 16 samples at a time, the next 16 loaded while these are filtered; the
//                         launch is bound by the serial recursion, 3 H steps per lane, not by memory.  One wave per
//                         workgroup, so that the waves of an item spread over the CUs.
//   level_gain_kernel     one workgroup per item: the peak, the 400 ms blocks from four hop sums each, the absolute and the
//                         relative gate, L and the gain.  Per-thread partial sums over blocks j = t, t + 256, ..., then
//                         added by thread 0 in thread order: the same bits on every call.
//   level_scale_kernel    x[i] = g x[i], one float32 multiply (not launched when the call only measures; an item without
//                         a target is left alone)
struct LevelItem {
    float* x;                  // the item's samples (device), levelled in place
    long long n;
    long long hop0;            // its first hop sum / hop peak in the two hop buffers
    double L;                  // out, in the layout of ft_level_info from here on: integrated loudness (-inf: nothing measured)
    float p, g;                // out: sample peak, gain
    int blocks, gated, capped; // out: 400 ms blocks, those that passed both gates, whether the ceiling bound the gain
    int target;                // in: the item's target in hundredths of a LUFS (0: measure only, the item is left as it is)
};
struct LevelTab {
    double c[10];              // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
    double ceiling;            // 10^(-1/20)
    int H, B, pad[2];          // hop; items (the target travels with the item: a call may level each toward its own)
    LevelItem it[64];
};
constexpr int LV_WARM = 2, LV_CHUNK = 16, LV_FILTER_THREADS = 64, LV_GAIN_THREADS = 256, LV_SCALE_THREADS = 256;

__device__ inline void level_load(const float* x, long long i, long long end, float* v) {
#pragma unroll
    for (int k = 0; k < LV_CHUNK; ++k) v[k] = i + k < end ? x[i + k] : 0.f;
}

static __global__ __launch_bounds__(LV_FILTER_THREADS) void level_filter_kernel(const LevelTab* tab, double* hops, float* peaks) {
    const LevelItem& it = tab->it[blockIdx.z];
    const long long n = it.n, H = tab->H, nh = (n + H - 1) / H;
    const double b0 = tab->c[0], b1 = tab->c[1], b2 = tab->c[2], a1 = tab->c[3], a2 = tab->c[4];
    const double d0 = tab->c[5], d1 = tab->c[6], d2 = tab->c[7], e1 = tab->c[8], e2 = tab->c[9];
    const float* x = it.x;
    for (long long h = (long long)blockIdx.x * LV_FILTER_THREADS + threadIdx.x; h < nh; h += (long long)gridDim.x * LV_FILTER_THREADS) {
        const long long s0 = h * H, s1 = min(n, s0 + H), w0 = max(0LL, s0 - LV_WARM * H);
        double u1 = 0.0, u2 = 0.0, v1 = 0.0, v2 = 0.0, acc = 0.0;   // the two filters' states (transposed direct form II)
        float pk = 0.f;
        float cur[LV_CHUNK], nxt[LV_CHUNK];
        level_load(x, w0, s1, cur);
        for (long long i = w0; i < s1; i += LV_CHUNK) {
            level_load(x, i + LV_CHUNK, s1, nxt);
#pragma unroll
            for (int k = 0; k < LV_CHUNK; ++k) {
                const long long q = i + k;
                const float xf = cur[k];
                const double xv = (double)xf;
                const double y = fma(b0, xv, u1);
                u1 = fma(b1, xv, fma(-a1, y, u2));
                u2 = fma(b2, xv, -a2 * y);
                const double z = fma(d0, y, v1);
                v1 = fma(d1, y, fma(-e1, z, v2));
                v2 = fma(d2, y, -e2 * z);
                if (q >= s0 && q < s1) {
                    acc = fma(z, z, acc);
                    pk = fmaxf(pk, fabsf(xf));
                }
                cur[k] = nxt[k];
            }
        }
        hops[it.hop0 + h] = acc;
        peaks[it.hop0 + h] = pk;
    }
}

// Block j of an item with `whole` whole hops: four hop sums, or (fewer than four whole hops) everything the item has.
__device__ inline double level_block(const double* e, long long j, long long whole, long long nh, long long n, int H) {
    if (whole >= 4) return (e[j] + e[j + 1] + e[j + 2] + e[j + 3]) / (4.0 * (double)H);
    double s = 0.0;
    for (long long h = 0; h < nh; ++h) s += e[h];
    return s / (double)n;
}
__device__ inline double level_lufs(double E) { return -0.691 + 10.0 * log10(E); }

static __global__ __launch_bounds__(LV_GAIN_THREADS) void level_gain_kernel(LevelTab* tab, const double* hops, const float* peaks) {
    LevelItem& it = tab->it[blockIdx.x];
    const int H = tab->H, t = threadIdx.x;
    const long long n = it.n, nh = (n + H - 1) / H, whole = n / H, nb = whole >= 4 ? whole - 3 : (n >= 1 ? 1 : 0);
    const double* e = hops + it.hop0;
    __shared__ double ssum[LV_GAIN_THREADS], sall[LV_GAIN_THREADS];
    __shared__ long long scnt[LV_GAIN_THREADS];
    __shared__ float spk[LV_GAIN_THREADS];
    __shared__ double gamma;
    __shared__ int live;
    float pk = 0.f;
    for (long long h = t; h < nh; h += LV_GAIN_THREADS) pk = fmaxf(pk, peaks[it.hop0 + h]);
    double s = 0.0, all = 0.0;
    long long k = 0;
    for (long long j = t; j < nb; j += LV_GAIN_THREADS) {
        const double E = level_block(e, j, whole, nh, n, H);
        all += E;
        if (level_lufs(E) > -70.0) { s += E; ++k; }
    }
    ssum[t] = s; sall[t] = all; scnt[t] = k; spk[t] = pk;
    __syncthreads();
    if (t == 0) {
        s = 0.0; all = 0.0; k = 0; pk = 0.f;
        for (int i = 0; i < LV_GAIN_THREADS; ++i) { s += ssum[i]; all += sall[i]; k += scnt[i]; pk = fmaxf(pk, spk[i]); }
        live = isfinite(all) && k > 0;
        gamma = live ? level_lufs(s / (double)k) - 10.0 : 0.0;
        it.L = -INFINITY; it.p = pk; it.g = 1.f; it.blocks = (int)nb; it.gated = 0; it.capped = 0;
    }
    __syncthreads();
    if (!live) return;
    const double gm = gamma;
    s = 0.0;
    k = 0;
    for (long long j = t; j < nb; j += LV_GAIN_THREADS) {
        const double E = level_block(e, j, whole, nh, n, H), l = level_lufs(E);
        if (l > -70.0 && l > gm) { s += E; ++k; }
    }
    __syncthreads();
    ssum[t] = s; scnt[t] = k;
    __syncthreads();
    if (t == 0) {
        s = 0.0; k = 0;
        for (int i = 0; i < LV_GAIN_THREADS; ++i) { s += ssum[i]; k += scnt[i]; }
        if (k > 0) {
            const double L = level_lufs(s / (double)k);
            it.L = L;
            it.gated = (int)k;
            if (it.target != 0) {
                double g = pow(10.0, ((double)it.target / 100.0 - L) / 20.0);
                const double p = (double)it.p;
                if (p > 0.0 && tab->ceiling / p < g) {
                    g = tab->ceiling / p;
                    it.capped = 1;
                }
                it.g = (float)g;
            }
        }
    }
}

static __global__ __launch_bounds__(LV_SCALE_THREADS) void level_scale_kernel(const LevelTab* tab) {
    const LevelItem& it = tab->it[blockIdx.z];
    if (it.target == 0) return;       // measured only
    const float g = it.g;
    float* x = it.x;
    for (long long i = (long long)blockIdx.x * LV_SCALE_THREADS + threadIdx.x; i < it.n; i += (long long)gridDim.x * LV_SCALE_THREADS)
        x[i] = g * x[i];
}

// ---- ride stage (ft_codec_stream_begin_live, ft_codec_ride; stated in fishtts_hip.h): a look-ahead gain rider behind the
// resampler of a stream, with carried state.  A call names one segment per stream (blockIdx.z of a device table; streams at
// different rates mix, so the filter and the hop travel with the segment).  Sample q of a stream lives in the carry copy
// the call reads (q < nin: cin[q - base]) or in the call's new samples (x[q - nin]).  Three launches whatever the number of
// streams:
//   ride_hop_kernel     the hops the new samples complete (at the end of a stream also the one cut short): one lane per hop
//                       with level_filter_kernel's arithmetic - both biquads in float64 from zero state LV_WARM hops earlier
//                       or at sample 0, the sum over the hop ascending - so a hop sum has the bits of the whole-waveform
//                       call.  A call completes few hops per stream; the streams lie on blockIdx.z, one wave per workgroup,
//                       so that they spread over the CUs.  The launch is bound by the recursion, 3 H steps per lane.
//   ride_node_kernel    one workgroup (one wave) per stream, the new nodes serially in k: the measure over the first m_k
//                       hops (blocks, both gates: per-thread partial sums over blocks j = t, t + 64, ..., added by thread 0
//                       in thread order - an order that depends on m_k alone), then slew, peak guard and the float32 node
//                       by thread 0.  A call brings a few nodes per stream and a measure has at most some 2000 blocks.
//   ride_apply_kernel   the emitted range times the interpolated gain, and the samples from the new base on rolled into the
//                       carry copy the call writes.  A segment without a target copies its samples (a stream without the
//                       stage in a call that has one).
struct RdSeg {
    const float* x;            // the call's new samples (device): what the stage in front gave
    const float* cin;          // carry read: samples [base, nin)
    float* cout;               // carry written: samples [base1, nin + n)
    float* y;                  // out: samples [out0, out1)
    double *e, *v;             // the stream's hop sums and v_k
    float *p, *g;              // its hop peaks and nodes
    double c[10];              // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 at the stream's rate
    double ceiling;            // 10^(-1/20)
    long long nin, base, base1, out0, out1;
    int n, H;                  // new samples; hop
    int h0, h1;                // hops to filter (h1: the peaks known after the call)
    int W;                     // whole hops after the call
    int k0, k1;                // nodes to compute
    int target;                // hundredths of a LUFS; 0: no stage, y = x
};
constexpr int RD_LOOK = 10, RD_HOP_THREADS = 64, RD_NODE_THREADS = 64, RD_APPLY_THREADS = 256;
constexpr double RD_SLEW = 0.5;

__device__ inline float ride_at(const RdSeg& g, long long q) { return q < g.nin ? g.cin[q - g.base] : g.x[q - g.nin]; }

__device__ inline void ride_load(const RdSeg& g, long long i, long long end, float* v) {
#pragma unroll
    for (int k = 0; k < LV_CHUNK; ++k) v[k] = i + k < end ? ride_at(g, i + k) : 0.f;
}

static __global__ __launch_bounds__(RD_HOP_THREADS) void ride_hop_kernel(const RdSeg* segs) {
    const RdSeg& g = segs[blockIdx.z];
    const long long h = (long long)g.h0 + (long long)blockIdx.x * RD_HOP_THREADS + threadIdx.x;
    if (h >= g.h1) return;
    const long long n = g.nin + g.n, H = g.H;
    const double b0 = g.c[0], b1 = g.c[1], b2 = g.c[2], a1 = g.c[3], a2 = g.c[4];
    const double d0 = g.c[5], d1 = g.c[6], d2 = g.c[7], e1 = g.c[8], e2 = g.c[9];
    const long long s0 = h * H, s1 = min(n, s0 + H), w0 = max(0LL, s0 - LV_WARM * H);
    double u1 = 0.0, u2 = 0.0, v1 = 0.0, v2 = 0.0, acc = 0.0;   // as level_filter_kernel
    float pk = 0.f;
    float cur[LV_CHUNK], nxt[LV_CHUNK];
    ride_load(g, w0, s1, cur);
    for (long long i = w0; i < s1; i += LV_CHUNK) {
        ride_load(g, i + LV_CHUNK, s1, nxt);
#pragma unroll
        for (int k = 0; k < LV_CHUNK; ++k) {
            const long long q = i + k;
            const float xf = cur[k];
            const double xv = (double)xf;
            const double y = fma(b0, xv, u1);
            u1 = fma(b1, xv, fma(-a1, y, u2));
            u2 = fma(b2, xv, -a2 * y);
            const double z = fma(d0, y, v1);
            v1 = fma(d1, y, fma(-e1, z, v2));
            v2 = fma(d2, y, -e2 * z);
            if (q >= s0 && q < s1) {
                acc = fma(z, z, acc);
                pk = fmaxf(pk, fabsf(xf));
            }
            cur[k] = nxt[k];
        }
    }
    g.e[h] = acc;
    g.p[h] = pk;
}

static __global__ __launch_bounds__(RD_NODE_THREADS) void ride_node_kernel(const RdSeg* segs) {
    const RdSeg& g = segs[blockIdx.x];
    const int H = g.H, t = threadIdx.x;
    const double* e = g.e;
    __shared__ double ssum[RD_NODE_THREADS], sall[RD_NODE_THREADS];
    __shared__ long long scnt[RD_NODE_THREADS];
    __shared__ double gamma;
    __shared__ int live;
    double vprev = g.k0 > 0 ? g.v[g.k0 - 1] : 0.0;      // thread 0's; v_{-1} = 0
    for (int k = g.k0; k < g.k1; ++k) {
        const long long m = min(k + RD_LOOK, g.W), nb = m >= 4 ? m - 3 : (m >= 1 ? 1 : 0), n = m * H;
        const int used = (int)min((long long)RD_NODE_THREADS, nb);
        double s = 0.0, all = 0.0;
        long long cnt = 0;
        for (long long j = t; j < nb; j += RD_NODE_THREADS) {
            const double E = level_block(e, j, m, m, n, H);
            all += E;
            if (level_lufs(E) > -70.0) { s += E; ++cnt; }
        }
        ssum[t] = s; sall[t] = all; scnt[t] = cnt;
        __syncthreads();
        if (t == 0) {
            s = 0.0; all = 0.0; cnt = 0;
            for (int i = 0; i < used; ++i) { s += ssum[i]; all += sall[i]; cnt += scnt[i]; }
            live = isfinite(all) && cnt > 0;
            gamma = live ? level_lufs(s / (double)cnt) - 10.0 : 0.0;
        }
        __syncthreads();
        const bool on = live != 0;
        const double gm = gamma;
        s = 0.0;
        cnt = 0;
        if (on)
            for (long long j = t; j < nb; j += RD_NODE_THREADS) {
                const double E = level_block(e, j, m, m, n, H), l = level_lufs(E);
                if (l > -70.0 && l > gm) { s += E; ++cnt; }
            }
        __syncthreads();
        ssum[t] = s; scnt[t] = cnt;
        __syncthreads();
        if (t == 0) {
            s = 0.0; cnt = 0;
            for (int i = 0; i < used; ++i) { s += ssum[i]; cnt += scnt[i]; }
            const double L = on && cnt > 0 ? level_lufs(s / (double)cnt) : -INFINITY;
            const double u = isfinite(L) ? (double)g.target / 100.0 - L : vprev;
            const double v = k == 0 ? u : fmin(fmax(u, vprev - RD_SLEW), vprev + RD_SLEW);
            const float q = fmaxf(k >= 1 && k - 1 < g.h1 ? g.p[k - 1] : 0.f, k < g.h1 ? g.p[k] : 0.f);
            const double cap = q > 0.f ? 20.0 * log10(g.ceiling / (double)q) : INFINITY;
            g.v[k] = v;
            g.g[k] = (float)pow(10.0, fmin(v, cap) / 20.0);
            vprev = v;
        }
        __syncthreads();
    }
}

static __global__ __launch_bounds__(RD_APPLY_THREADS) void ride_apply_kernel(const RdSeg* segs) {
    const RdSeg& g = segs[blockIdx.z];
    const long long step = (long long)gridDim.x * RD_APPLY_THREADS, t = (long long)blockIdx.x * RD_APPLY_THREADS + threadIdx.x;
    if (g.target == 0) {
        for (long long i = t; i < g.n; i += step) g.y[i] = g.x[i];
        return;
    }
    const float Hf = (float)g.H;
    for (long long i = g.out0 + t; i < g.out1; i += step) {
        const long long k = i / g.H;
        const float gk = g.g[k], w = (float)(i - k * g.H) / Hf;
        g.y[i - g.out0] = ride_at(g, i) * fmaf(w, g.g[k + 1] - gk, gk);
    }
    for (long long q = g.base1 + t; q < g.nin + g.n; q += step) g.cout[q - g.base1] = ride_at(g, q);
}

// ---- mix stage (ft_codec_mix; stated in fishtts_hip.h): a bed at the output rate under a finished programme.  The timeline
// has N = lead + n + tail samples (N <= 2^28: sample and hop indices fit 32 bits), s[i] = x[i - lead] inside the programme
// and 0 outside it.  Three launches, four when the ceiling binds:
//   mix_hop_kernel    one wave per hop of H samples: act[h] = some |s| of the hop is >= the threshold (never a NaN); the
//                     active hops are counted with one integer atomic per workgroup
//   mix_node_kernel   one lane per node k = 0 .. Nh: the nearest active hop in [k, k + Wa) and in [k - Wr, k) from the
//                     workgroup's window of flags staged in LDS (256 + Wa + Wr bytes), D_k and g_k = T[D_k]
//   mix_kernel        a workgroup per MX_SPAN samples, four per lane and step: 16-byte stores on the aligned groups of y,
//                     16-byte loads of the programme where `lead` is a multiple of 4 and the group lies inside it, of the
//                     bed where the group starts on a multiple of 4 of the bed and does not wrap; scalar loads elsewhere and
//                     on the last up to three samples.  Per workgroup the peak of |m|, one integer atomicMax on its bits
//                     (the values are not negative, so their bit patterns order as they do)
//   mix_scale_kernel  y times sg in place
struct MixOut { unsigned int pk; int active, dmax, pad; };
struct MixP {
    const float* x;            // programme, n samples (device, 16-byte aligned)
    const float* bed;          // bed at the output rate, nb samples (device, 16-byte aligned)
    const float* T;            // [6001]
    unsigned char* act;        // [Nh]
    int* D;                    // [Nh + 1]
    float* g;                  // [Nh + 1]
    float* y;                  // [N]
    MixOut* out;
    long long nb, off;         // off: `offset` (mod nb with loop, at most nb without)
    int N, n, lead, Nh, H, depth, Wa, Wr, f_in, f_out, loop;
    float thr;
};
constexpr int MX_THREADS = 256, MX_STEPS = 4, MX_SPAN = MX_THREADS * 4 * MX_STEPS, MX_MAX_WIN = 500;

static __global__ __launch_bounds__(MX_THREADS) void mix_hop_kernel(MixP p) {
    const int lane = threadIdx.x & 63, h = blockIdx.x * (MX_THREADS / 64) + (threadIdx.x >> 6);
    __shared__ int cnt[MX_THREADS / 64];
    int on = 0;
    if (h < p.Nh) {
        const int i0 = h * p.H, i1 = min(p.N, i0 + p.H);
        float pk = -1.f;                                   // (fmaxf passes a NaN by: a hop of NaNs stays below any threshold)
        for (int i = i0 + lane; i < i1; i += 64) {
            const int q = i - p.lead;
            if (q >= 0 && q < p.n) pk = fmaxf(pk, fabsf(p.x[q]));
            else pk = fmaxf(pk, 0.f);
        }
        for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o));
        on = pk >= p.thr;
        if (lane == 0) p.act[h] = (unsigned char)on;
    }
    if (lane == 0) cnt[threadIdx.x >> 6] = on;
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < MX_THREADS / 64; ++w) c += cnt[w];
        if (c > 0) atomicAdd(&p.out->active, c);
    }
}

static __global__ __launch_bounds__(MX_THREADS) void mix_node_kernel(MixP p) {
    __shared__ unsigned char win[MX_THREADS + 2 * MX_MAX_WIN];
    __shared__ int wmax[MX_THREADS / 64];
    const int k0 = blockIdx.x * MX_THREADS, lo = k0 - p.Wr, span = MX_THREADS + p.Wa + p.Wr;   // win[j] = act[lo + j]
    for (int j = threadIdx.x; j < span; j += MX_THREADS) {
        const int h = lo + j;
        win[j] = h >= 0 && h < p.Nh ? p.act[h] : 0;
    }
    __syncthreads();
    const int k = k0 + threadIdx.x;
    int d = 0;
    if (k <= p.Nh) {
        const unsigned char* w = win + (k - lo);           // w[j] = act[k + j]
        for (int j = 0; j < p.Wa; ++j)
            if (w[j]) { d = (int)((long long)p.depth * (p.Wa - j) / p.Wa); break; }
        for (int j = 0; j < p.Wr; ++j)
            if (w[-1 - j]) { d = max(d, (int)((long long)p.depth * (p.Wr - j) / p.Wr)); break; }
        p.D[k] = d;
        p.g[k] = p.T[d];
    }
    for (int o = 32; o > 0; o >>= 1) d = max(d, __shfl_xor(d, o));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MX_THREADS / 64; ++w) d = max(d, wmax[w]);
        if (d > 0) atomicMax(&p.out->dmax, d);
    }
}

__device__ inline float mix_prog(const MixP& p, int i) {
    const int q = i - p.lead;
    return q >= 0 && q < p.n ? p.x[q] : 0.f;
}

// Bed sample at position j = i + off of the bed (j >= 0).
__device__ inline float mix_bed(const MixP& p, long long j) {
    if (p.loop) return p.bed[j % p.nb];
    return j < p.nb ? p.bed[j] : 0.f;
}

// m[i] from s = s[i] and t = b(i): the fades, the duck, the sum, every operation rounded on its own.
__device__ inline float mix_sample(const MixP& p, int i, float s, float t) {
    const unsigned int k = (unsigned int)i / (unsigned int)p.H;
    const float gk = p.g[k], r = __fdiv_rn((float)(i - (int)k * p.H), (float)p.H);
    const float gd = fmaf(r, p.g[k + 1] - gk, gk);
    if (i < p.f_in) t = __fmul_rn(t, (float)((double)(2 * (long long)i + 1) / (double)(2 * (long long)p.f_in)));
    if (i >= p.N - p.f_out) t = __fmul_rn(t, (float)((double)(2 * (long long)(p.N - 1 - i) + 1) / (double)(2 * (long long)p.f_out)));
    return __fadd_rn(s, __fmul_rn(t, gd));
}

static __global__ __launch_bounds__(MX_THREADS) void mix_kernel(MixP p) {
    __shared__ float wpk[MX_THREADS / 64];
    const int N4 = p.N >> 2;
    const bool xal = (p.lead & 3) == 0;
    float pk = 0.f;
    for (int st = 0; st < MX_STEPS; ++st) {
        const int q = (blockIdx.x * MX_STEPS + st) * MX_THREADS + threadIdx.x, i = 4 * q;
        if (q >= N4) break;
        float4 s, t;
        const int a = i - p.lead;
        if (xal && a >= 0 && a + 3 < p.n) s = *(const float4*)(p.x + a);
        else s = make_float4(mix_prog(p, i), mix_prog(p, i + 1), mix_prog(p, i + 2), mix_prog(p, i + 3));
        long long j = (long long)i + p.off;
        if (p.loop) j %= p.nb;
        if ((j & 3) == 0 && j + 3 < p.nb) t = *(const float4*)(p.bed + j);
        else t = make_float4(mix_bed(p, j), mix_bed(p, j + 1), mix_bed(p, j + 2), mix_bed(p, j + 3));
        float4 m;
        m.x = mix_sample(p, i, s.x, t.x);
        m.y = mix_sample(p, i + 1, s.y, t.y);
        m.z = mix_sample(p, i + 2, s.z, t.z);
        m.w = mix_sample(p, i + 3, s.w, t.w);
        ((float4*)p.y)[q] = m;
        pk = fmaxf(pk, fmaxf(fmaxf(fabsf(m.x), fabsf(m.y)), fmaxf(fabsf(m.z), fabsf(m.w))));
    }
    // the up to three samples behind the last whole group: the workgroup that owns position N4
    if (4 * N4 < p.N && N4 / (MX_THREADS * MX_STEPS) == (int)blockIdx.x && threadIdx.x < p.N - 4 * N4) {
        const int i = 4 * N4 + threadIdx.x;
        const float m = mix_sample(p, i, mix_prog(p, i), mix_bed(p, (long long)i + p.off));
        p.y[i] = m;
        pk = fmaxf(pk, fabsf(m));
    }
    for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o));
    if ((threadIdx.x & 63) == 0) wpk[threadIdx.x >> 6] = pk;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MX_THREADS / 64; ++w) pk = fmaxf(pk, wpk[w]);
        if (pk > 0.f) atomicMax(&p.out->pk, __float_as_uint(pk));
    }
}

static __global__ __launch_bounds__(MX_THREADS) void mix_scale_kernel(float* y, int N, float sg) {
    const int N4 = N >> 2;
    for (int q = blockIdx.x * MX_THREADS + threadIdx.x; q < N4; q += gridDim.x * MX_THREADS) {
        float4 v = ((float4*)y)[q];
        v.x = __fmul_rn(v.x, sg); v.y = __fmul_rn(v.y, sg); v.z = __fmul_rn(v.z, sg); v.w = __fmul_rn(v.w, sg);
        ((float4*)y)[q] = v;
    }
    if (blockIdx.x == 0 && 4 * N4 + (int)threadIdx.x < N) y[4 * N4 + threadIdx.x] = __fmul_rn(y[4 * N4 + threadIdx.x], sg);
}

// ---- live mix stage (ft_codec_mix_stream_*, ft_codec_mix_live; stated in fishtts_hip.h under "Live mix"): the mix stage on a
// stream.  A push brings the programme samples of timeline [F0, F1); the stream carries the programme from cb0 on (pin) and the
// m of [out0, q0 H) that did not go out yet (cin), and the push writes both carries anew for its successor (pout from cb1,
// cout from out1).  Every sample buffer is laid out by the sample's timeline index minus a multiple of four (xb, pib, pob,
// mb, cib, cob: the first index rounded down), so a group of four samples that starts at a multiple of four lies on a
// 16-byte boundary in every one of them.  The per-hop arrays (act, D, g, need, L) are whole and indexed absolutely.  Five
// launches per push, whatever its size; a launch whose range is empty is left out:
//   mixl_hop_kernel     one wave per hop of [h0, h1): the activity flag, as mix_hop_kernel.  A sample comes from the carry
//                       or from the push: the lane picks the buffer and clamps the index, loads once and then selects
//                       between the value and zero - no branch per sample
//   mixl_node_kernel    one lane per duck node of [kd0, kd1): D_k and g_k from the flags of the workgroup's window in LDS,
//                       as mix_node_kernel (only hops below h1 exist so far)
//   mixl_sample_kernel  one workgroup per hop of [q0, q1), one group of four samples per lane (a hop has at most 960
//                       samples): mix_sample over the hop with 16-byte loads where a whole group lies in one buffer and
//                       16-byte stores of the whole groups; the hop's peak Q_h reduced in the workgroup; lane 0 then finds
//                       need_h by binary search over T
//   mixl_limit_kernel   one lane per limiter node of [kl0, kl1): L_k from the 30 hops around it
//   mixl_apply_kernel   y over [out0, out1), then the two carries rolled
// The integers a stream reports are kept in MixLiveOut by integer atomics, so no sum or max depends on an order.
struct MixLiveOut { unsigned int qmax; int active, dmax, lmax; };
struct MixLiveP {
    MixP m;                    // bed, T, act, D, g, nb, off, lead, H, depth, Wa, Wr, f_in, loop, thr as ft_codec_mix fills them;
                               // x: the push's samples; y: the m of hops [q0, q1); N, f_out: the timeline's once it has ended,
                               // else 2^30 and 0 (no sample that is final before the end lies in the fade-out)
    const float* pin;          // programme carry read: timeline [cb0, F0)
    float* pout;               // programme carry written: [cb1, F1)
    const float* cin;          // m carry read: [out0, q0 H)
    float* cout;               // m carry written: [out1, mend1)
    float* y;                  // out: [out0, out1)
    int* need;                 // [hops]
    int* L;                    // [hops + 1]
    MixLiveOut* out;
    int F0, F1, cb0, cb1;      // the push's samples; the first programme sample carried in, out
    int h0, h1, kd0, kd1, q0, q1, kl0, kl1, out0, out1;
    int mend1;                 // the end of the m known after the push: q1 H (at the end of the stream out1 = N: nothing rolls)
    int Nend;                  // samples that exist: N once the stream has ended, else 2^30
    int xb, pib, pob, mb, cib, cob;
    float cf;                  // (float) 10^(-1/20)
};
constexpr int ML_ATTACK = 5, ML_RELEASE = 25;

// s[i] for any i: the carry below F0, the push from there, zero outside [cb0, F1) - the lead, and the tail once it exists.
__device__ inline float mixl_prog(const MixLiveP& p, int i) {
    const bool old = i < p.F0;
    const float* src = old ? p.pin : p.m.x;
    const int lo = old ? p.cb0 : p.F0, hi = old ? p.F0 : p.F1, ab = old ? p.pib : p.xb;
    const int ic = min(max(i, lo), max(hi - 1, lo));       // (an empty range: lo, inside the buffer's margin)
    const float v = src[ic - ab];
    return i >= lo && i < hi ? v : 0.f;
}

// m[i] for i in [out0, mend1): the carry below q0 H, the push's hops from there.
__device__ inline float mixl_m(const MixLiveP& p, int i, int mend0) {
    const bool old = i < mend0;
    const float* src = old ? p.cin : p.m.y;
    const int lo = old ? p.out0 : mend0, hi = old ? mend0 : p.mend1, ab = old ? p.cib : p.mb;
    const int ic = min(max(i, lo), max(hi - 1, lo));
    return src[ic - ab];
}

static __global__ __launch_bounds__(MX_THREADS) void mixl_hop_kernel(MixLiveP p) {
    const int lane = threadIdx.x & 63, h = p.h0 + blockIdx.x * (MX_THREADS / 64) + (threadIdx.x >> 6);
    __shared__ int cnt[MX_THREADS / 64];
    int on = 0;
    if (h < p.h1) {
        const int i0 = h * p.m.H, i1 = min(p.Nend, i0 + p.m.H);
        float pk = -1.f;                                   // (as mix_hop_kernel: a hop of NaNs stays below any threshold)
        for (int i = i0 + lane; i < i1; i += 64) pk = fmaxf(pk, fabsf(mixl_prog(p, i)));
        for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o));
        on = pk >= p.m.thr;
        if (lane == 0) p.m.act[h] = (unsigned char)on;
    }
    if (lane == 0) cnt[threadIdx.x >> 6] = on;
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < MX_THREADS / 64; ++w) c += cnt[w];
        if (c > 0) atomicAdd(&p.out->active, c);
    }
}

static __global__ __launch_bounds__(MX_THREADS) void mixl_node_kernel(MixLiveP p) {
    __shared__ unsigned char win[MX_THREADS + 2 * MX_MAX_WIN];
    __shared__ int wmax[MX_THREADS / 64];
    const int Wa = p.m.Wa, Wr = p.m.Wr;
    const int k0 = p.kd0 + blockIdx.x * MX_THREADS, lo = k0 - Wr, span = MX_THREADS + Wa + Wr;   // win[j] = act[lo + j]
    for (int j = threadIdx.x; j < span; j += MX_THREADS) {
        const int h = lo + j;
        win[j] = h >= 0 && h < p.h1 ? p.m.act[h] : 0;
    }
    __syncthreads();
    const int k = k0 + threadIdx.x;
    int d = 0;
    if (k < p.kd1) {
        const unsigned char* w = win + (k - lo);           // w[j] = act[k + j]
        for (int j = 0; j < Wa; ++j)
            if (w[j]) { d = (int)((long long)p.m.depth * (Wa - j) / Wa); break; }
        for (int j = 0; j < Wr; ++j)
            if (w[-1 - j]) { d = max(d, (int)((long long)p.m.depth * (Wr - j) / Wr)); break; }
        p.m.D[k] = d;
        p.m.g[k] = p.m.T[d];
    }
    for (int o = 32; o > 0; o >>= 1) d = max(d, __shfl_xor(d, o));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MX_THREADS / 64; ++w) d = max(d, wmax[w]);
        if (d > 0) atomicMax(&p.out->dmax, d);
    }
}

static __global__ __launch_bounds__(MX_THREADS) void mixl_sample_kernel(MixLiveP p) {
    __shared__ float wpk[MX_THREADS / 64];
    const int h = p.q0 + blockIdx.x, i0 = h * p.m.H, i1 = min(i0 + p.m.H, p.Nend);
    const int i = (i0 & ~3) + 4 * (int)threadIdx.x;       // this lane's group: [i, i + 4), cut to the hop
    float pk = 0.f;
    if (i < i1) {
        const bool whole = i >= i0 && i + 3 < i1;
        float4 s, t;
        if (whole && i >= p.F0 && i + 3 < p.F1) s = *(const float4*)(p.m.x + (i - p.xb));
        else if (whole && i >= p.cb0 && i + 3 < p.F0) s = *(const float4*)(p.pin + (i - p.pib));
        else s = make_float4(mixl_prog(p, i), mixl_prog(p, i + 1), mixl_prog(p, i + 2), mixl_prog(p, i + 3));
        long long j = (long long)i + p.m.off;
        if (p.m.loop) j %= p.m.nb;
        if ((j & 3) == 0 && j + 3 < p.m.nb) t = *(const float4*)(p.m.bed + j);
        else t = make_float4(mix_bed(p.m, j), mix_bed(p.m, j + 1), mix_bed(p.m, j + 2), mix_bed(p.m, j + 3));
        if (whole) {
            float4 m;
            m.x = mix_sample(p.m, i, s.x, t.x);
            m.y = mix_sample(p.m, i + 1, s.y, t.y);
            m.z = mix_sample(p.m, i + 2, s.z, t.z);
            m.w = mix_sample(p.m, i + 3, s.w, t.w);
            *(float4*)(p.m.y + (i - p.mb)) = m;
            pk = fmaxf(fmaxf(fabsf(m.x), fabsf(m.y)), fmaxf(fabsf(m.z), fabsf(m.w)));   // (fmaxf passes a NaN by)
            pk = fmaxf(pk, 0.f);
        } else {                                           // the hop's first and last group: the samples inside it
            const float sv[4] = {s.x, s.y, s.z, s.w}, tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (i + c >= i0 && i + c < i1) {
                    const float m = mix_sample(p.m, i + c, sv[c], tv[c]);
                    p.m.y[i + c - p.mb] = m;
                    pk = fmaxf(pk, fabsf(m));
                }
        }
    }
    for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o));
    if ((threadIdx.x & 63) == 0) wpk[threadIdx.x >> 6] = pk;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MX_THREADS / 64; ++w) pk = fmaxf(pk, wpk[w]);
        // need_h: the smallest d with T[d] Q <= cf (T falls with d, so the test is monotone), 6000 when there is none
        int lo = 0, hi = 6000;
        if (__fmul_rn(p.m.T[hi], pk) <= p.cf)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (__fmul_rn(p.m.T[mid], pk) <= p.cf) hi = mid;
                else lo = mid + 1;
            }
        p.need[h] = hi;
        if (pk > 0.f) atomicMax(&p.out->qmax, __float_as_uint(pk));
    }
}

static __global__ __launch_bounds__(MX_THREADS) void mixl_limit_kernel(MixLiveP p) {
    __shared__ int wmax[MX_THREADS / 64];
    const int k = p.kl0 + blockIdx.x * MX_THREADS + threadIdx.x;
    int l = 0;
    if (k < p.kl1) {
        for (int j = 0; j < ML_ATTACK; ++j) {              // hops k .. k + La - 1
            const int h = k + j;
            if (h < p.q1) l = max(l, (int)((long long)p.need[h] * (ML_ATTACK - j) / ML_ATTACK));
        }
        for (int j = 0; j < ML_RELEASE; ++j) {             // hops k - 1 .. k - Lr
            const int h = k - 1 - j;
            if (h >= 0 && h < p.q1) l = max(l, (int)((long long)p.need[h] * (ML_RELEASE - j) / ML_RELEASE));
        }
        p.L[k] = l;
    }
    for (int o = 32; o > 0; o >>= 1) l = max(l, __shfl_xor(l, o));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = l;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MX_THREADS / 64; ++w) l = max(l, wmax[w]);
        if (l > 0) atomicMax(&p.out->lmax, l);
    }
}

static __global__ __launch_bounds__(MX_THREADS) void mixl_apply_kernel(MixLiveP p) {
    const int step = gridDim.x * MX_THREADS, t = blockIdx.x * MX_THREADS + threadIdx.x, H = p.m.H, mend0 = p.q0 * H;
    const float Hf = (float)H;
    for (int i = p.out0 + t; i < p.out1; i += step) {
        const int k = (int)((unsigned int)i / (unsigned int)H);
        const float lk = p.m.T[p.L[k]], r = __fdiv_rn((float)(i - k * H), Hf);
        p.y[i - p.out0] = __fmul_rn(mixl_m(p, i, mend0), fmaf(r, p.m.T[p.L[k + 1]] - lk, lk));
    }
    for (int i = p.out1 + t; i < p.mend1; i += step) p.cout[i - p.cob] = mixl_m(p, i, mend0);
    for (int i = p.cb1 + t; i < p.F1; i += step) p.pout[i - p.pob] = mixl_prog(p, i);
}

}  // namespace ft
