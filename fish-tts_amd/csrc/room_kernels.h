// The room stage's kernels (ft_codec_room; stated in fishtts_hip.h under "Room"): a convolution reverb behind the join, the
// programme convolved with an impulse response in direct form on the f32-input MFMA, whose result is a k-ordered f32 fmaf
// chain and can therefore be stated to the bit.  It builds on stage_kernels.h (mix_scale_kernel) and is included by codec.hip
// alone, behind stereo_kernels.h and for that header's reason: engine.hip sees neither, so nothing here moves the AR engine.
//   room_ir_kernel    one lane per block of 256 taps: t[k] = irF[offset + k] with the fade on the last f taps, and the block's
//                     energy e_b in float64, k ascending
//   room_gain_kernel  one workgroup: lane 0 adds the e_b ascending to E and rounds gn; every lane then writes hn = t gn
//   room_send_kernel  xs[i] = x[i] T[send of i]: the region of a sample by binary search (left out when no send is set)
//   room_conv_kernel  the chain, and behind it the sum with the dry signal and the workgroup's peak (below)
//   mix_scale_kernel  as it is, when the ceiling binds
// and the live room stage's (ft_codec_room_stream_*; "Live room"), behind them: rooml_send_kernel, rooml_conv_kernel - the same
// text as room_conv_kernel over another source of the sent programme - and rooml_roll_kernel.
#pragma once
#include "stage_kernels.h"

namespace ft {

constexpr int RM_BLOCK = 256;                  // taps per energy block
constexpr int RM_MAX_L = 131072;               // taps at most
constexpr int RM_WAVES = 4, RM_THREADS = 64 * RM_WAVES;
constexpr int RM_TILE = 1024;                  // outputs of a wave: one 32 x 32 accumulator
constexpr int RM_SPAN = RM_WAVES * RM_TILE;    // outputs of a workgroup
constexpr int RM_DC = 1024;                    // chain terms per LDS stage
constexpr int RM_STEP = 32;                    // chain terms per block of the inner loop: sixteen MFMAs (divides RM_DC)
constexpr int RM_XWIN = RM_SPAN - 32 + RM_DC;  // programme samples a stage reads
constexpr int RM_XLDS = RM_XWIN + (RM_XWIN >> 5) + 1;
constexpr int RM_HLDS = RM_DC + 32;
constexpr int RM_LAUNCH = 1 << 22;             // outputs per launch: 1024 workgroups, four waves per SIMD

struct RoomOut { unsigned int pk; int pad; double E; float gn; int pad2; };
struct RoomIrP {
    const float* ir;           // irF, nh samples
    float* t;                  // [L]
    float* hn;                 // [L]
    double* e;                 // [ceil(L / 256)]
    RoomOut* out;
    int L, f, normalize;
    long long offset;
};
struct RoomSendP {
    const float* x;
    float* xs;
    const float* T;            // [6001]
    const MixPan* reg;         // ft_send_region: `pan` holds the send
    int n, R, send;            // send: outside every region
};
struct RoomConvP {
    const float* xs;           // what the chain reads, n samples: x itself where no send is set
    const float* x;            // the dry signal, n samples
    const float* hn;           // [L]
    float* y;                  // [N]: y, or c for the test hook (raw != 0)
    RoomOut* out;
    int n, L, predelay, N, i0; // i0: the launch's first output
    int raw;
    float gd, gw;              // T[dry] (+0.0: no dry signal, the term is not formed), T[wet]
    int dry;
};

static __global__ __launch_bounds__(64) void room_ir_kernel(RoomIrP p) {
    const int b = blockIdx.x * 64 + threadIdx.x, k0 = b * RM_BLOCK;
    if (k0 >= p.L) return;
    const int k1 = min(p.L, k0 + RM_BLOCK);
    const double den = (double)(2 * (long long)p.f);
    double e = 0.0;
    for (int k = k0; k < k1; ++k) {
        float v = p.ir[p.offset + k];
        if (k >= p.L - p.f) v = __fmul_rn(v, (float)((double)(2 * (long long)(p.L - 1 - k) + 1) / den));
        p.t[k] = v;
        e = __dadd_rn(e, __dmul_rn((double)v, (double)v));
    }
    p.e[b] = e;
}

static __global__ __launch_bounds__(1024) void room_gain_kernel(RoomIrP p) {
    __shared__ float gs;
    if (threadIdx.x == 0) {
        const int nb = (p.L + RM_BLOCK - 1) / RM_BLOCK;
        double E = 0.0;
        for (int b = 0; b < nb; ++b) E = __dadd_rn(E, p.e[b]);
        const float gn = p.normalize ? (float)(1.0 / sqrt(E)) : 1.f;
        p.out->E = E;
        p.out->gn = gn;
        gs = gn;
    }
    __syncthreads();
    const float gn = gs;
    for (int k = threadIdx.x; k < p.L; k += 1024) p.hn[k] = __fmul_rn(p.t[k], gn);
}

// (one text for the whole call and for a stream's push, whose x, n and regions are the push's own: rooml_send_kernel)
__device__ __forceinline__ void room_send_body(RoomSendP p) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.n; i += gridDim.x * 256) {
        int lo = 0, hi = p.R;                              // the first region that ends behind i
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (p.reg[mid].e > i) hi = mid; else lo = mid + 1;
        }
        const int s = lo < p.R && p.reg[lo].a <= i ? p.reg[lo].pan : p.send;
        p.xs[i] = s < 0 ? 0.f : __fmul_rn(p.x[i], p.T[s]);
    }
}
static __global__ __launch_bounds__(256) void room_send_kernel(RoomSendP p) { room_send_body(p); }

// The chain as a Toeplitz product on v_mfma_f32_32x32x2_f32.  A wave owns 1024 consecutive outputs as a 32 x 32 tile,
// Y[r][c] = c[i0 + 32 r + c] = sum over d of xs[i0 + 32 r - d - predelay] hn[d + c], d = -31 .. L - 1 ascending, hn zero
// outside [0, L): with d ascending every output takes its taps k = d + c in ascending order, the MFMA adds its two k in
// order (the f32-input MFMA is a k-ordered fmaf chain), and one accumulator holds the chain from its first term to its last -
// nothing is split.  The terms with a zero tap add (+-0) to the chain: in front of it they leave +0.0, behind it they leave
// every value but -0.0, which the stage states as +0.0 anyway (the last addition below).
// With e = d + 31 the terms are staged RM_DC at a time: hq[e + c] = hn[e + c - 31] (RM_DC + 32 words) and the window of xs that
// the workgroup's four tiles read for those e (RM_XWIN words, zero outside [0, n)).  Lane (r, h) of a step reads A at word
// q = 1024 w + 32 r + RM_DC - 1 - h - e: a lane stride of 32 words, so word q lies at q + (q >> 5) and the 32 lanes of a half
// fall on 32 banks; B is read at e + h + c, consecutive.  Both reads are 4 bytes per lane and MFMA, far below what LDS gives.
// Every index is bounded by N + L + predelay + RM_SPAN < 2^29.
// The kernel's text is room_conv_body, over the source of the sent programme: RoomWhole for ft_codec_room - xs itself, n
// samples, output i at y[i] - and RoomLive for a stream's push (below).  Both kernels are this one text, so a stream gives
// the whole call's bits by construction; the source decides only where a word of the staging comes from, where an output
// lands and up to where the dry signal exists.
struct RoomWhole {
    const RoomConvP& p;
    __device__ __forceinline__ float at(int g) const { return g >= 0 && g < p.n ? p.xs[g] : 0.f; }
    __device__ __forceinline__ int rel(int i) const { return i; }
};

template <class Src>
__device__ __forceinline__ void room_conv_body(const RoomConvP& p, const Src& src) {
    using f32x16 = __attribute__((ext_vector_type(16))) float;
    __shared__ float lds[RM_XLDS + RM_HLDS + RM_WAVES];
    float* XL = lds;
    float* HL = lds + RM_XLDS;
    float* wpk = HL + RM_HLDS;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int I0 = p.i0 + blockIdx.x * RM_SPAN;
    const int terms = p.L + 31;
    f32x16 acc;
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (int s0 = 0; s0 < terms; s0 += RM_DC) {
        const int w0 = I0 + 31 - p.predelay - (s0 + RM_DC - 1);          // xs index of word 0
        __syncthreads();
        for (int q = threadIdx.x; q < RM_XWIN; q += RM_THREADS) {
            const int g = w0 + q;
            XL[q + (q >> 5)] = src.at(g);
        }
        for (int u = threadIdx.x; u < RM_HLDS; u += RM_THREADS) {
            const int k = s0 + u - 31;
            HL[u] = k >= 0 && k < p.L ? p.hn[k] : 0.f;
        }
        __syncthreads();
        // RM_STEP terms at a time, the next block's operands read while this block's MFMAs run (one wave per SIMD has nothing
        // else to hide the LDS latency behind); the count is rounded up to whole blocks - more zero taps behind the chain
        const int cnt = (min(RM_DC, terms - s0) + RM_STEP - 1) & ~(RM_STEP - 1);
        const int qb = RM_TILE * w + 32 * r + RM_DC - 1 - h;
        const float* hb = HL + h + r;
        float a[RM_STEP / 2], b[RM_STEP / 2], an[RM_STEP / 2] = {}, bn[RM_STEP / 2] = {};
#pragma unroll
        for (int j = 0; j < RM_STEP / 2; ++j) {
            const int q = qb - 2 * j;
            a[j] = XL[q + (q >> 5)];
            b[j] = hb[2 * j];
        }
        for (int e = 0; e < cnt; e += RM_STEP) {
            if (e + RM_STEP < cnt) {
#pragma unroll
                for (int j = 0; j < RM_STEP / 2; ++j) {
                    const int q = qb - e - RM_STEP - 2 * j;
                    an[j] = XL[q + (q >> 5)];
                    bn[j] = hb[e + RM_STEP + 2 * j];
                }
            }
#pragma unroll
            for (int j = 0; j < RM_STEP / 2; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < RM_STEP / 2; ++j) {
                a[j] = an[j];
                b[j] = bn[j];
            }
        }
    }
    float pk = 0.f;
    const int it = I0 + RM_TILE * w;
    for (int j = 0; j < 16; ++j) {
        const int row = (j & 3) + 8 * (j >> 2) + 4 * h, i = it + 32 * row + r;
        if (i < p.N) {
            const float c = __fadd_rn(acc[j], 0.f);
            float v = c;
            if (!p.raw) {
                const float wet = __fmul_rn(p.gw, c);
                const float dry = p.dry && i < p.n ? __fmul_rn(p.gd, p.x[src.rel(i)]) : 0.f;
                v = __fadd_rn(dry, wet);
            }
            p.y[src.rel(i)] = v;
            pk = fmaxf(pk, fabsf(v));
        }
    }
    for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o));
    if (lane == 0) wpk[w] = pk;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < RM_WAVES; ++v) pk = fmaxf(pk, wpk[v]);
        if (pk > 0.f) atomicMax(&p.out->pk, __float_as_uint(pk));
    }
}

static __global__ __launch_bounds__(RM_THREADS) void room_conv_kernel(RoomConvP p) { room_conv_body(p, RoomWhole{p}); }

// ---- live room stage (ft_codec_room_stream_*, ft_codec_room_live; stated in fishtts_hip.h under "Live room"): the room stage
// on a stream.  A push brings the samples of timeline [F0, F1) and emits the outputs [F0, F1), the final one up to N; the
// stream carries the sent samples [cb0, F0), cb0 = max(0, F0 - (predelay + L - 1)) - all that an output from F0 on reads
// below F0 - in two copies, one read and one written by a push.  Three launches per push, one with nothing to do left out:
//   rooml_send_kernel  xs of the push from its own regions: room_send_kernel's rule with push-relative indices (left out
//                      where the push has no region and rp->send = 0: its xs is x)
//   rooml_conv_kernel  room_conv_body over RoomLive: a word of the staging comes from the carry (timeline [cb0, F0)) or from
//                      the push ([F0, F1)) - the lane picks the buffer and clamps the index, loads once and selects between
//                      the value and +0.0, no branch per sample (mixl_prog's pattern); the dry signal is the push's x, and an
//                      output lands at its index in the push.  RoomConvP then holds n = F1, N = the end of the outputs, x
//                      and y the push's buffers, xs unused
//   rooml_roll_kernel  the carry [cb1, F1) for the next push, from the old one and the push's xs (nothing after the final
//                      push)
// The peak goes into the stream's own RoomOut by the same integer atomicMax.
struct RoomLive {
    const float* carry;        // sent samples [cb0, F0) (at least one element, read and not taken where the range is empty)
    const float* xs;           // sent samples [F0, F1) (the same)
    int cb0, F0, F1;
    __device__ __forceinline__ float at(int g) const {
        const bool old = g < F0;
        const float* s = old ? carry : xs;
        const int lo = old ? cb0 : F0, hi = old ? F0 : F1;
        const int ic = min(max(g, lo), max(hi - 1, lo));
        const float v = s[ic - lo];
        return g >= lo && g < hi ? v : 0.f;
    }
    __device__ __forceinline__ int rel(int i) const { return i - F0; }
};
struct RoomRollP {
    RoomLive src;
    float* out;                // the carry written: [cb1, F1)
    int cb1;
};

static __global__ __launch_bounds__(256) void rooml_send_kernel(RoomSendP p) { room_send_body(p); }

static __global__ __launch_bounds__(RM_THREADS) void rooml_conv_kernel(RoomConvP p, RoomLive src) { room_conv_body(p, src); }

static __global__ __launch_bounds__(256) void rooml_roll_kernel(RoomRollP p) {
    for (int i = p.cb1 + blockIdx.x * 256 + threadIdx.x; i < p.src.F1; i += gridDim.x * 256) p.out[i - p.cb1] = p.src.at(i);
}

}  // namespace ft
