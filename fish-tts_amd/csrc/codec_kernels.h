// DAC codec decode kernels for gfx950.  Activations are time-major [T][C] bf16 in HBM (the
// transformer's residual stream is f32); every convolution / linear layer is one "tap GEMM":
//     Y[t][n] = sum_tap sum_c X[t + off_tap][c] * W[tap][n][c]          (rows t + off < 0 read as 0)
// on bf16 MFMA (v_mfma_f32_16x16x32_bf16, f32 accumulate) with fused epilogues:
//   * Conv1d k=7 dilation d (vocoder.py:394-421): 7 taps, off = (kk-6)*d
//   * ConvTranspose1d k=2s stride s, right-trimmed (vocoder.py:432-455): N = s*Cout, 2 taps (0, -1),
//     the [T][s][Cout] result IS the [T*s][Cout] output
//   * Linear / 1x1 conv: one tap
// Snake (x + sin^2(ax)/a) is applied once per element in the producer's epilogue, never per tap.
#pragma once
#include <float.h>
#include <limits.h>

#include <algorithm>

#include "common.h"

namespace ft {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { ACT_NONE = 0, ACT_GELU = 1, ACT_SWIGLU = 2, ACT_TANH = 3 };

struct TapGemmP {
    const bf16_t* X;      // [B][T_in][ldx]
    long ldx, x_bstride;
    int T_in;
    int t_min;            // lowest readable row of X (0; negative in a streamed decode: rows [t_min, 0) hold the previous
                          // chunk's last rows instead of the causal zero padding)
    const bf16_t* W;      // [ntap][N][K]
    int ntap;
    int offs[8];
    int M, N, K;          // output rows per batch item, output columns, contraction per tap
    const float* bias;    // [n_mod] or null
    int n_mod;            // bias/alpha/gamma index = n % n_mod
    int act;
    const float* gamma;   // per-column scale (LayerScale / ConvNeXt gamma) or null
    const float* resid_f32;
    const bf16_t* resid_bf;
    long ldr, r_bstride;
    float* out_f32;
    bf16_t* out_bf;
    bf16_t* out_act;      // snake(v, alpha) or null
    const float* alpha;
    long ldo, o_bstride;
    int round_lin;      // round acc+bias to bf16 first (an nn.Linear output of a bf16 model; also the SwiGLU steps)
    int round_f32_out;  // out_f32 receives bf16-rounded values
    long ldw;           // skinny kernel: row stride of W in elements (0 = K, dense)
    // skinny kernel, fused RMSNorm (llama.py:172-177) of the X operand: X holds the un-normalised rows (exact bf16
    // copies of the residual stream), ss_in[row][b] the partial sums of squares the producer GEMM's blocks left
    // (ss_nblk partials per row, row stride ss_ld); ss_out: this GEMM's own partials of its f32 output rows
    const bf16_t* gain;
    const float* ss_in;
    float* ss_out;
    int ss_nblk, ss_ld;
    float eps;
    // batched streamed decode (ft_codec_stream_decode_many): blockIdx.z is one stream's chunk, seg[z] = {P, L, t0, nh}
    // (SegZ).  The chunk has M = T_in = L * seg_m rows; its X rows start at P * seg_m + z * seg_xg, its output and
    // residual rows at P * seg_m + z * seg_og (the gap rows between chunks hold carried halo rows).  null: one item.
    const int4* seg;
    int seg_m, seg_xg, seg_og;
    // (measured and removed: the RMSNorm of the OUTPUT rows by the block that finishes last - write-through stores, a
    // returning ticket atomic and the last block's trip to the memory side cost more than the ~5 us norm launch they
    // replaced: 4.67 against 3.54 ms per 32-row frame)
};

// The chunk of blockIdx.z in a batched streamed decode (the skinny kernel): M, T_in and the row bases of X / residual /
// outputs become the chunk's, so the per-element arithmetic is that of the same chunk decoded alone.  false: the block
// lies past the chunk.
__device__ __forceinline__ bool tap_segment(TapGemmP& p, int m0) {
    if (!p.seg) return true;
    const int4 s = p.seg[blockIdx.z];
    p.M = p.T_in = s.y * p.seg_m;
    if (m0 >= p.M) return false;
    const long xr = (long)s.x * p.seg_m + (long)blockIdx.z * p.seg_xg;
    const long orow = (long)s.x * p.seg_m + (long)blockIdx.z * p.seg_og;
    p.X += xr * p.ldx;
    if (p.resid_f32) p.resid_f32 += orow * p.ldr;
    if (p.resid_bf) p.resid_bf += orow * p.ldr;
    if (p.out_f32) p.out_f32 += orow * p.ldo;
    if (p.out_bf) p.out_bf += orow * p.ldo;
    if (p.out_act) p.out_act += orow * p.ldo;
    return true;
}

// The tap kernels keep p as it came (their lambdas capture it by reference: a modified copy lands in scratch) and read
// the item's rows and row bases from here: one batch item b (x / r / o_bstride) or the chunk of blockIdx.z (seg).
struct TapSeg { int M, T_in; size_t xo, ro, oo; };
__device__ __forceinline__ TapSeg tap_seg(const TapGemmP& p, int b) {
    if (!p.seg) return TapSeg{p.M, p.T_in, (size_t)b * p.x_bstride, (size_t)b * p.r_bstride, (size_t)b * p.o_bstride};
    const int4 s = p.seg[blockIdx.z];
    const long xr = (long)s.x * p.seg_m + (long)blockIdx.z * p.seg_xg;
    const long orow = (long)s.x * p.seg_m + (long)blockIdx.z * p.seg_og;
    const int M = s.y * p.seg_m;
    return TapSeg{M, M, (size_t)(xr * p.ldx), (size_t)(orow * p.ldr), (size_t)(orow * p.ldo)};
}

// The same for the row kernels of a batched streamed decode: seg[blockIdx.z] = {P, L, t0, nh} (frames [P, P + L) of the
// call, rope position t0, nh carried K/V rows); at a stage of m rows per frame the chunk's rows start at P * m + z * g.
// carry[(z * ncarry + ci) * 2 + {0, 1}]: the carry this chunk reads and the one it leaves for the next chunk.
struct SegZ {
    const int4* seg = nullptr;       // null: one item (the plain launch)
    bf16_t* const* carry = nullptr;
    int ncarry = 0, ci = 0;
    int m = 1, g = 0;
    __device__ __forceinline__ int4 get() const { return seg[blockIdx.z]; }
    __device__ __forceinline__ long row0(const int4& s) const { return (long)s.x * m + (long)blockIdx.z * g; }
    __device__ __forceinline__ bf16_t* carry_in() const { return carry[((long)blockIdx.z * ncarry + ci) * 2]; }
    __device__ __forceinline__ bf16_t* carry_out() const { return carry[((long)blockIdx.z * ncarry + ci) * 2 + 1]; }
};

// offs[] lives in the kernel arguments: a runtime index would force the whole struct into scratch
__device__ __forceinline__ int tap_off(const TapGemmP& p, int tap) {
    int o = p.offs[0];
#pragma unroll
    for (int t = 1; t < 8; ++t) o = (t == tap) ? p.offs[t] : o;
    return o;
}

__device__ __forceinline__ float snake_f(float v, float a) {
    // hardware sine (v_sin_f32 after the 1/2pi scaling): ~1e-6 absolute error, far below the bf16 step of the
    // value it is stored in; the argument is O(10) here
    const float s = __sinf(a * v);
    return v + (1.0f / (a + 1e-9f)) * (s * s);
}
__device__ __forceinline__ float gelu_f(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

template <int TM, int TN>
__device__ __forceinline__ void tapgemm_epilogue(const TapGemmP& p, f32x4 (&acc)[TM][TN], const int mw, const int nw,
                                                 const TapSeg& ts, const int fr, const int fq) {
    // epilogue: lane holds C[row = 4*fq + r][col = fr] of each 16x16 tile
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = nw + j * 16 + fr;
            const bool nv = n < p.N;
            const int nm = nv ? n % p.n_mod : 0;
            const float bias = (p.bias && nv) ? p.bias[nm] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = mw + i * 16 + fq * 4 + r;
                float v = acc[i][j][r] + bias;
                if (p.round_lin) v = round_bf16(v);
                if (p.act == ACT_SWIGLU) {
                    // columns (2i, 2i+1) = (gate, up): partner value sits in the neighbouring lane
                    const float other = dpp_f<DPP_XOR1>(v);
                    if ((fr & 1) == 0 && nv && t < ts.M) {
                        const float gate = v, up = other;
                        float sg = gate / (1.0f + expf(-gate));
                        if (p.round_lin) sg = round_bf16(sg);
                        const float o = sg * up;
                        const size_t oi = ts.oo + (size_t)t * p.ldo + (n >> 1);
                        if (p.out_bf) p.out_bf[oi] = f32_to_bf16_bits(o);
                        if (p.out_f32) p.out_f32[oi] = p.round_f32_out ? round_bf16(o) : o;
                    }
                    continue;
                }
                if (!nv || t >= ts.M) continue;
                if (p.act == ACT_GELU) v = gelu_f(v);
                else if (p.act == ACT_TANH) v = tanhf(v);
                if (p.gamma) v *= p.gamma[nm];
                const size_t ri = ts.ro + (size_t)t * p.ldr + n;
                if (p.resid_f32) v += p.resid_f32[ri];
                if (p.resid_bf) v += bf16_bits_to_f32(p.resid_bf[ri]);
                const size_t oi = ts.oo + (size_t)t * p.ldo + n;
                if (p.out_f32) p.out_f32[oi] = p.round_f32_out ? round_bf16(v) : v;
                if (p.out_bf) p.out_bf[oi] = f32_to_bf16_bits(v);
                if (p.out_act) p.out_act[oi] = f32_to_bf16_bits(snake_f(v, p.alpha[nm]));
            }
        }
    }
}

// Block tile BM x BN, BK = 32, 256 threads = 4 waves arranged WGM x WGN; each wave owns
// (BM/WGM) x (BN/WGN) as 16x16 MFMA tiles.  LDS rows are padded to 40 bf16 (80 B) so the 16-byte
// fragment reads of 16 consecutive rows spread over the banks.
template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(256) void tapgemm_kernel(TapGemmP p) {
    constexpr int BK = 32, LDS_LD = 40;
    constexpr int WM = BM / WGM, WN = BN / WGN;
    constexpr int TM = WM / 16, TN = WN / 16;
    __shared__ __attribute__((aligned(16))) bf16_t As[BM * LDS_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Bs[BN * LDS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN, b = p.seg ? 0 : blockIdx.z;
    const TapSeg ts = tap_seg(p, b);
    if (m0 >= ts.M) return;
    const bf16_t* X = p.X + ts.xo;
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;
    for (int tap = 0; tap < p.ntap; ++tap) {
        const int off = tap_off(p, tap);
        const bf16_t* Wt = p.W + (size_t)tap * p.N * p.K;
        for (int k0 = 0; k0 < p.K; k0 += BK) {
            // stage A (BM x 32) and B (BN x 32): 16-byte chunks, 4 per row
            for (int c = tid; c < BM * 4; c += 256) {
                const int r = c >> 2, q = c & 3;
                const int t = m0 + r + off;
                U4 v = U4{0u, 0u, 0u, 0u};
                if (m0 + r < ts.M && t >= p.t_min && t < ts.T_in)
                    v = *reinterpret_cast<const U4*>(X + (size_t)t * p.ldx + k0 + q * 8);
                *reinterpret_cast<U4*>(&As[r * LDS_LD + q * 8]) = v;
            }
            for (int c = tid; c < BN * 4; c += 256) {
                const int r = c >> 2, q = c & 3;
                U4 v = U4{0u, 0u, 0u, 0u};
                if (n0 + r < p.N) v = *reinterpret_cast<const U4*>(Wt + (size_t)(n0 + r) * p.K + k0 + q * 8);
                *reinterpret_cast<U4*>(&Bs[r * LDS_LD + q * 8]) = v;
            }
            __syncthreads();
            bf16x8 af[TM], bfr[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[i] = *reinterpret_cast<const bf16x8*>(&As[(wm * WM + i * 16 + fr) * LDS_LD + fq * 8]);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bfr[j] = *reinterpret_cast<const bf16x8*>(&Bs[(wn * WN + j * 16 + fr) * LDS_LD + fq * 8]);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            __syncthreads();
        }
    }
    tapgemm_epilogue<TM, TN>(p, acc, m0 + wm * WM, n0 + wn * WN, ts, fr, fq);
}

// Epilogue through LDS: the accumulators (column-per-lane) are transposed so that each lane finishes 8 consecutive
// columns of one row: 16-byte loads of the residual, 16-byte stores of every output (the late decoder stages are
// bandwidth-bound: 2-byte scattered stores were the bottleneck).  NWM passes of BM/NWM rows.
template <int BM, int BN, int TM, int TN, int NWM = 2, int NWN = 2>
__device__ __forceinline__ void tapgemm_epilogue_lds(const TapGemmP& p, f32x4 (&acc)[TM][TN], float* Cs, const int m0,
                                                     const int n0, const TapSeg& ts, const int wm, const int wn,
                                                     const int fr, const int fq) {
    constexpr int LDC = BN + 4;
    constexpr int WM = BM / NWM, WN = BN / NWN;
    constexpr int NTHR = 64 * NWM * NWN;
    const int tid = threadIdx.x;
#pragma unroll
    for (int pass = 0; pass < NWM; ++pass) {
        __syncthreads();
        if (wm == pass) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        Cs[(i * 16 + fq * 4 + r) * LDC + wn * WN + j * 16 + fr] = acc[i][j][r];
        }
        __syncthreads();
        for (int v = tid; v < WM * (BN / 8); v += NTHR) {
            const int row = v / (BN / 8), c8 = (v % (BN / 8)) * 8;
            const int t = m0 + pass * WM + row, n = n0 + c8;
            if (t >= ts.M || n >= p.N) continue;
            const int nm = n % p.n_mod;
            float x[8];
            const float4 c0 = *reinterpret_cast<const float4*>(&Cs[row * LDC + c8]);
            const float4 c1 = *reinterpret_cast<const float4*>(&Cs[row * LDC + c8 + 4]);
            x[0] = c0.x; x[1] = c0.y; x[2] = c0.z; x[3] = c0.w; x[4] = c1.x; x[5] = c1.y; x[6] = c1.z; x[7] = c1.w;
            if (p.bias) {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] += p.bias[nm + j];
            }
            if (p.round_lin) {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = round_bf16(x[j]);
            }
            if (p.act == ACT_GELU) {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = gelu_f(x[j]);
            } else if (p.act == ACT_TANH) {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = tanhf(x[j]);
            }
            if (p.gamma) {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] *= p.gamma[nm + j];
            }
            const size_t ri = ts.ro + (size_t)t * p.ldr + n;
            if (p.resid_f32) {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] += p.resid_f32[ri + j];
            }
            if (p.resid_bf) {
                float rv[8];
                Vec<bf16_t>::load(p.resid_bf + ri, rv);
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] += rv[j];
            }
            const size_t oi = ts.oo + (size_t)t * p.ldo + n;
            if (p.out_f32) {
#pragma unroll
                for (int j = 0; j < 8; ++j) p.out_f32[oi + j] = p.round_f32_out ? round_bf16(x[j]) : x[j];
            }
            if (p.out_bf) {
                U4 o;
                o.x = f32_to_bf16_bits(x[0]) | ((uint32_t)f32_to_bf16_bits(x[1]) << 16);
                o.y = f32_to_bf16_bits(x[2]) | ((uint32_t)f32_to_bf16_bits(x[3]) << 16);
                o.z = f32_to_bf16_bits(x[4]) | ((uint32_t)f32_to_bf16_bits(x[5]) << 16);
                o.w = f32_to_bf16_bits(x[6]) | ((uint32_t)f32_to_bf16_bits(x[7]) << 16);
                *reinterpret_cast<U4*>(p.out_bf + oi) = o;
            }
            if (p.out_act) {
                float y[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) y[j] = snake_f(x[j], p.alpha[nm + j]);
                U4 o;
                o.x = f32_to_bf16_bits(y[0]) | ((uint32_t)f32_to_bf16_bits(y[1]) << 16);
                o.y = f32_to_bf16_bits(y[2]) | ((uint32_t)f32_to_bf16_bits(y[3]) << 16);
                o.z = f32_to_bf16_bits(y[4]) | ((uint32_t)f32_to_bf16_bits(y[5]) << 16);
                o.w = f32_to_bf16_bits(y[6]) | ((uint32_t)f32_to_bf16_bits(y[7]) << 16);
                *reinterpret_cast<U4*>(p.out_act + oi) = o;
            }
        }
    }
}

// Pipelined variant for K % 64 == 0 (every layer of the real codec).  Per 64-channel chunk the A rows of the
// block *and its tap halo* (BM + max|off| rows) are staged once and shared by all taps; the B (weight) tile of
// the next tap is fetched into registers while the current one feeds the MFMAs and is written to the other LDS
// buffer afterwards: one barrier per (tap, chunk) step, 32 (BN=128) MFMAs per wave between barriers.
// NWM x NWN waves (default 2 x 2 = 256 threads).  The 8-wave 128-row tiles exist because the small tile is bound by the L2:
// a BM x BN tile reads (BM + BN) K bf16 per BM BN K MACs = BM BN / (BM + BN) flop per byte - 32 at 64 x 64, and 1024
// co-resident blocks re-reading their weight tiles at ~10-13 TB/s of L2 bandwidth is the 320-420 TFLOP/s the k = 7
// convolutions of the decoder ran at (12.8 % MFMA); 128 x 128 doubles it with the same waves per CU.
template <int BM, int BN, int BK, int NWM = 2, int NWN = 2>
__global__ __launch_bounds__(64 * NWM * NWN) void tapgemm64_kernel(TapGemmP p) {
    constexpr int NTHR = 64 * NWM * NWN;
    constexpr int LD = BK + 8;                      // LDS row stride (bf16): keeps 16-byte alignment, spreads banks
    constexpr int WM = BM / NWM, WN = BN / NWN;
    constexpr int TM = WM / 16, TN = WN / 16;
    static_assert(WM % 16 == 0 && WN % 16 == 0, "wave tile = whole 16 x 16 MFMA tiles");
    constexpr int MAXH = 56;                        // largest tap halo (k=7, dilation 9 -> 54)
    constexpr int QPR = BK / 8;                     // 16-byte chunks per tile row
    extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
    bf16_t* As = lds;                               // [(BM + MAXH)][LD]
    bf16_t* Bs0 = As + (BM + MAXH) * LD;            // [BN][LD] x 2
    bf16_t* Bs1 = Bs0 + BN * LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / NWN, wn = wave % NWN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN, b = p.seg ? 0 : blockIdx.z;
    const TapSeg ts = tap_seg(p, b);
    if (m0 >= ts.M) return;
    const bf16_t* X = p.X + ts.xo;
    int offmin = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) offmin = (t < p.ntap) ? min(offmin, p.offs[t]) : offmin;
    const int srows = BM - offmin;                  // stripe rows: t in [m0 + offmin, m0 + BM)
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;
    constexpr int BCH = (BN * QPR + NTHR - 1) / NTHR;     // 16-byte chunks of a B tile per thread
    // weight tiles are fetched TWO steps ahead into two named register sets (the MFMA work of one step is far
    // shorter than an L2 round trip)
    U4 bregA[BCH], bregB[BCH];
    auto load_b = [&](U4 (&breg)[BCH], int step) {
        const int tap = step % p.ntap, k0 = (step / p.ntap) * BK;
        const bf16_t* Wt = p.W + (size_t)tap * p.N * p.K;
#pragma unroll
        for (int u = 0; u < BCH; ++u) {
            const int c = tid + NTHR * u, r = c / QPR, q = c % QPR;
            breg[u] = (r < BN && n0 + r < p.N) ? *reinterpret_cast<const U4*>(Wt + (size_t)(n0 + r) * p.K + k0 + q * 8) : U4{0u, 0u, 0u, 0u};
        }
    };
    auto store_b = [&](const U4 (&breg)[BCH], bf16_t* Bs) {
#pragma unroll
        for (int u = 0; u < BCH; ++u) {
            const int c = tid + NTHR * u, r = c / QPR, q = c % QPR;
            if (r < BN) *reinterpret_cast<U4*>(&Bs[r * LD + q * 8]) = breg[u];
        }
    };
    const int nsteps = p.ntap * (p.K / BK);
    const int nchunks = p.K / BK;
    // the A stripe of the NEXT K chunk also travels in registers while this chunk's taps run (with one tap - linears,
    // 1x1 convs, the prompt GEMMs - its load latency would otherwise be exposed once per step)
    constexpr int ACH = ((BM + MAXH) * QPR + NTHR - 1) / NTHR;
    U4 areg[ACH];
    auto load_a = [&](int kc) {
#pragma unroll
        for (int u = 0; u < ACH; ++u) {
            const int c = tid + NTHR * u, r = c / QPR, q = c % QPR;
            const int t = m0 + offmin + r;
            areg[u] = (c < srows * QPR && t >= p.t_min && t < ts.T_in)
                          ? *reinterpret_cast<const U4*>(X + (size_t)t * p.ldx + kc * BK + q * 8) : U4{0u, 0u, 0u, 0u};
        }
    };
    load_a(0);
    auto do_step = [&](int step, U4 (&breg)[BCH], bf16_t* Bcur) {
        const int kc = step / p.ntap, tap = step % p.ntap;
        if (tap == 0) {
            // previous chunk's MFMAs are done (barrier at the end of its last step): restage the A stripe
#pragma unroll
            for (int u = 0; u < ACH; ++u) {
                const int c = tid + NTHR * u, r = c / QPR, q = c % QPR;
                if (c < srows * QPR) *reinterpret_cast<U4*>(&As[r * LD + q * 8]) = areg[u];
            }
            if (kc + 1 < nchunks) load_a(kc + 1);
        }
        store_b(breg, Bcur);
        __syncthreads();
        if (step + 2 < nsteps) load_b(breg, step + 2);  // in flight during two steps of MFMAs
        const int arow = tap_off(p, tap) - offmin;
#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk) {
            bf16x8 af[TM], bfr[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[i] = *reinterpret_cast<const bf16x8*>(&As[(arow + wm * WM + i * 16 + fr) * LD + kk * 32 + fq * 8]);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bfr[j] = *reinterpret_cast<const bf16x8*>(&Bcur[(wn * WN + j * 16 + fr) * LD + kk * 32 + fq * 8]);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        // the next step writes the OTHER B buffer; the A stripe is rewritten only at tap == 0 of the next chunk,
        // which must wait for every wave's reads of this chunk: barrier only then
        if (tap == p.ntap - 1) __syncthreads();
    };
    load_b(bregA, 0);
    if (nsteps > 1) load_b(bregB, 1);
    for (int step = 0; step < nsteps; step += 2) {
        do_step(step, bregA, Bs0);
        if (step + 1 < nsteps) do_step(step + 1, bregB, Bs1);
    }
    // vector epilogue whenever rows are 16-byte addressable (every real layer); SwiGLU pairs keep the lane epilogue
    const bool vec_ok = p.act != ACT_SWIGLU && (p.N % 8) == 0 && (p.n_mod % 8) == 0 && (p.ldo % 8) == 0 && (p.ldr % 8) == 0;
    if constexpr (TM * TN >= 16) {
        // 128x128: instantiating the lane epilogue here makes the compiler keep all 16 accumulator tiles in scratch for
        // the whole kernel (272 B/lane); the host selects this tile only for layers the vector epilogue covers
        tapgemm_epilogue_lds<BM, BN, TM, TN, NWM, NWN>(p, acc, reinterpret_cast<float*>(lds), m0, n0, ts, wm, wn, fr, fq);
    } else {
        if (vec_ok) tapgemm_epilogue_lds<BM, BN, TM, TN, NWM, NWN>(p, acc, reinterpret_cast<float*>(lds), m0, n0, ts, wm, wn, fr, fq);
        else tapgemm_epilogue<TM, TN>(p, acc, m0 + wm * WM, n0 + wn * WN, ts, fr, fq);
    }
}

// Plain Linear (one tap, no halo) on the same tiles, for the prompt pass: A and B tiles of DEPTH K-steps travel in registers
// at any time (the pipelined kernel above has its A stripe one step ahead only - enough behind seven taps, not for a
// linear: at 780 prompt rows every step waited ~2 us for its rows, 38 us per product).  Two LDS buffers, one barrier per
// step: step k's tiles are written to buffer k % 2 while buffer (k + 1) % 2 may still be read by waves one barrier behind.
template <int BM, int BN, int NWM, int NWN, int DEPTH, int MINW = 1>
__global__ __launch_bounds__(64 * NWM * NWN, MINW) void lingemm_kernel(TapGemmP p) {
    constexpr int BK = 64, NTHR = 64 * NWM * NWN, LD = BK + 8, QPR = BK / 8;
    constexpr int WM = BM / NWM, WN = BN / NWN, TM = WM / 16, TN = WN / 16;
    static_assert(WM % 16 == 0 && WN % 16 == 0 && DEPTH % 2 == 0, "whole MFMA tiles per wave; buffer parity follows the unrolled step");
    static_assert((BM * QPR) % NTHR == 0 && (BN * QPR) % NTHR == 0, "every thread moves whole 16-byte pieces of both tiles");
    constexpr int ACH = (BM * QPR) / NTHR, BCH = (BN * QPR) / NTHR;
    extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
    bf16_t* const A0 = lds;
    bf16_t* const B0 = lds + 2 * BM * LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / NWN, wn = wave % NWN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int fr = lane & 15, fq = lane >> 4;
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    U4 ar[DEPTH][ACH], br[DEPTH][BCH];
    auto load = [&](U4 (&a)[ACH], U4 (&b)[BCH], int step) {
        const int k0 = step * BK;
#pragma unroll
        for (int u = 0; u < ACH; ++u) {
            const int c = tid + NTHR * u, r = c / QPR, q = c % QPR;
            // rows past the end re-read the last row (their products are never stored): every load is unconditional, so the
            // counted waits of the pipeline stay exact (a predicated load costs a branch and a full drain per step)
            a[u] = *reinterpret_cast<const U4*>(p.X + (size_t)min(m0 + r, p.T_in - 1) * p.ldx + k0 + q * 8);
        }
#pragma unroll
        for (int u = 0; u < BCH; ++u) {
            const int c = tid + NTHR * u, r = c / QPR, q = c % QPR;
            b[u] = *reinterpret_cast<const U4*>(p.W + (size_t)min(n0 + r, p.N - 1) * p.K + k0 + q * 8);
        }
    };
    auto stage = [&](const U4 (&a)[ACH], const U4 (&b)[BCH], bf16_t* As, bf16_t* Bs) {
#pragma unroll
        for (int u = 0; u < ACH; ++u) {
            const int c = tid + NTHR * u, r = c / QPR, q = c % QPR;
            *reinterpret_cast<U4*>(&As[r * LD + q * 8]) = a[u];
        }
#pragma unroll
        for (int u = 0; u < BCH; ++u) {
            const int c = tid + NTHR * u, r = c / QPR, q = c % QPR;
            *reinterpret_cast<U4*>(&Bs[r * LD + q * 8]) = b[u];
        }
    };
    // K / 64 is a multiple of DEPTH (the host checks): no branch sits between a load and its use, and the loads past the end
    // re-read the last step's tiles, so the compiler's counted waits (vmcnt) never have to drain the pipeline
    const int nsteps = p.K / BK;
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) load(ar[d], br[d], d);
    for (int base = 0; base < nsteps; base += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            const int step = base + d;
            bf16_t* As = A0 + (d & 1) * BM * LD;
            bf16_t* Bs = B0 + (d & 1) * BN * LD;
            stage(ar[d], br[d], As, Bs);
            __syncthreads();
            load(ar[d], br[d], min(step + DEPTH, nsteps - 1));
#pragma unroll
            for (int kk = 0; kk < BK / 32; ++kk) {
                bf16x8 af[TM], bfr[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    af[i] = *reinterpret_cast<const bf16x8*>(&As[(wm * WM + i * 16 + fr) * LD + kk * 32 + fq * 8]);
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    bfr[j] = *reinterpret_cast<const bf16x8*>(&Bs[(wn * WN + j * 16 + fr) * LD + kk * 32 + fq * 8]);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    const bool vec_ok = p.act != ACT_SWIGLU && (p.N % 8) == 0 && (p.n_mod % 8) == 0 && (p.ldo % 8) == 0 && (p.ldr % 8) == 0;
    const TapSeg ts = tap_seg(p, 0);
    if (vec_ok) tapgemm_epilogue_lds<BM, BN, TM, TN, NWM, NWN>(p, acc, reinterpret_cast<float*>(lds), m0, n0, ts, wm, wn, fr, fq);
    else { __syncthreads(); tapgemm_epilogue<TM, TN>(p, acc, m0 + wm * WM, n0 + wn * WN, ts, fr, fq); }
}
template <int BM, int BN, int NWM>
constexpr size_t lingemm_lds_bytes() {
    return std::max((size_t)2 * (BM + BN) * (64 + 8) * 2, (size_t)(BM / NWM) * (BN + 4) * 4);
}

// ---- prompt-pass attention on the matrix cores (llama.py:229-283 with the causal mask of 437) -----------------------
// One block = 64 query positions of one query head (4 waves x 16 rows); K and V^T tiles of 32 cached positions are staged
// in LDS once per block and shared by the waves.  S = Q K^T and O += P V run on v_mfma_f32_16x16x32_bf16; the softmax is
// the online form in f32; P enters the second product as two bf16 planes (hi = bf16(p), lo = bf16(p - hi)), i.e. with
// f32-like precision, so the result follows the f32 SDPA of the reference up to summation order (one rounding at the end).
// Sums run in another order than the decode kernel's, so nothing pins it bit for bit: the launch alone is checked element by
// element against a float64 restatement (ft_test_pf_attn through engine.hip: pf_attn, tests/test_pf_kernels_gpu.py: y, the
// finished queries, the appended K / V rows, every other cache row unchanged with NaN patterns behind every sequence and in
// unused slots; NG = 4 and 2, HD = 128 and 64, prompt lengths on both sides of every query tile, of the 128- and 256-key pair
// steps and of the NG threshold, behind restored prefixes, alone and as a ragged pass over several slots), and whole prompt
// passes follow the oracle with the bf16 margin (tests/test_ar_gpu.py: test_prefill_gemm_paths_vs_oracle,
// test_ragged_prompt_pass_vs_oracle).
struct FlashP {
    const bf16_t* q;    // [S][H*hd] normalised + rotated queries
    const bf16_t* kc;   // [Hkv][n_slots][hd]
    const bf16_t* vc;
    bf16_t* y_bf;       // [S][H*hd]
    int S, H, Hkv, hd, n_slots, pos0;
    float scale;
    // ragged pass over the prompts of several slots (grid.z = sequence): seqs[z] = {first row, rows, first cache position,
    // slot}; q / y_bf rows are the concatenated prompts, kc / vc the layer's base pointers, cache_m_stride the elements
    // between slots.  Blocks past a sequence's last query tile leave at once.
    const int4* seqs;
    size_t cache_m_stride;
};
template <int HD, int NG>
__global__ __launch_bounds__(512) void flash_prefill_kernel(FlashP p) {
    constexpr int KT = 32;                  // keys per tile and key group
    constexpr int QW = 8 / NG;              // NG key groups of QW waves: group g takes keys [kt + 32 g, kt + 32 g + 32) of a step,
    constexpr int QROWS = 16 * QW;          // its waves 16 query rows each - a block covers QROWS query rows of one head
    static_assert(NG == 2 || NG == 4, "eight waves: 2 key groups x 64 query rows or 4 x 32");
    constexpr int LDK = HD + 8;             // K tile row stride (bf16)
    constexpr int LDV = KT + 8;             // V^T tile row stride
    constexpr int LDP = KT + 8;
    constexpr int NS = HD / 32;             // k-steps of Q K^T
    constexpr int NT = HD / 16;             // 16-wide output column tiles
    // The key groups walk the SAME query rows with their own online-softmax state and are merged once at the end: the
    // dependent chain of a block (a 780-position prompt: 26 tiles for the last query tile, the kernel's critical path with
    // fewer blocks than CUs) shrinks to 26 / NG steps of NG tiles side by side.
    constexpr int KS_N = KT * LDK, VT_N = HD * LDV, PS_N = 16 * LDP, XW = NT * 4 + 8;
    extern __shared__ __attribute__((aligned(16))) bf16_t smem_f[];      // flash_prefill_lds<HD, NG>() bytes
    static_assert((size_t)(NG * VT_N + 8 * 2 * PS_N) * sizeof(bf16_t) >= (size_t)(NG - 1) * QW * 64 * XW * sizeof(float), "the merge buffer reuses Vt + Ps");
    bf16_t (*Ks)[KS_N] = reinterpret_cast<bf16_t (*)[KS_N]>(smem_f);
    bf16_t (*Vt)[VT_N] = reinterpret_cast<bf16_t (*)[VT_N]>(smem_f + NG * KS_N);
    bf16_t (*Ps)[2][PS_N] = reinterpret_cast<bf16_t (*)[2][PS_N]>(smem_f + NG * KS_N + NG * VT_N);   // [8 waves]
    const int h = blockIdx.x, q0 = blockIdx.y * QROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = wave / QW, qw = wave % QW;            // key group, query sub-tile
    const int fr = lane & 15, fq = lane >> 4;
    const int G = p.H / p.Hkv, kvh = h / G;
    const bf16_t* kc = p.kc + (size_t)kvh * p.n_slots * HD;
    const bf16_t* vc = p.vc + (size_t)kvh * p.n_slots * HD;
    const bf16_t* qbase = p.q;
    bf16_t* ybase = p.y_bf;
    int S = p.S, pos0 = p.pos0;
    if (p.seqs) {
        const int4 sq = p.seqs[blockIdx.z];
        S = sq.y; pos0 = sq.z;
        if (q0 >= S) return;                               // the whole block: no barrier has been reached yet
        qbase += (size_t)sq.x * p.H * HD; ybase += (size_t)sq.x * p.H * HD;
        kc += (size_t)sq.w * p.cache_m_stride; vc += (size_t)sq.w * p.cache_m_stride;
    }
    // Q fragments of this wave's 16 rows (A operand: row = lane & 15, 8 consecutive d per lane)
    const int qrow = min(q0 + qw * 16 + fr, S - 1);
    bf16x8 qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s)
        qf[s] = *reinterpret_cast<const bf16x8*>(qbase + (size_t)qrow * p.H * HD + (size_t)h * HD + s * 32 + fq * 8);
    f32x4 O[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) O[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float mrun[4], lrun[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { mrun[r] = -INFINITY; lrun[r] = 0.f; }
    const int last_row = min(q0 + QROWS - 1, S - 1);
    const int kmax = pos0 + last_row;                    // last visible key of the block
    // K/V rows of a step (NG * KT keys) travel in registers TWO steps ahead of their use, in two named register sets; every
    // load is unconditional (rows past the last visible key re-read that key's row: they are masked below), so no branch sits
    // between a load and its use and the counted waits never drain the pipeline.  Each thread owns CPT 16-byte pieces.
    constexpr int CPT = NG * KT * (HD / 8) / 512;
    U4 kregA[CPT], vregA[CPT], kregB[CPT], vregB[CPT];
    auto fetch = [&](U4 (&kreg)[CPT], U4 (&vreg)[CPT], int kt) {
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const int c = tid + i * 512;
            const int kr = c / (HD / 8), d8 = (c % (HD / 8)) * 8;      // kr in [0, NG * KT)
            const int j = min(kt + kr, kmax);
            kreg[i] = *reinterpret_cast<const U4*>(kc + (size_t)j * HD + d8);
            vreg[i] = *reinterpret_cast<const U4*>(vc + (size_t)j * HD + d8);
        }
    };
    fetch(kregA, vregA, 0);
    fetch(kregB, vregB, NG * KT);
    // V^T in LDS: the 8-key group g of row d sits at group g ^ ((d / 8) & 3) - the 16 lanes that write one key of 16 different
    // 8-row bands then spread over four banks instead of one (their rows are 8 x LDV halfs = a multiple of 32 dwords apart)
    auto tile = [&](U4 (&kreg)[CPT], U4 (&vreg)[CPT], const int kt0) {
        __syncthreads();                                    // previous step fully consumed
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const int c = tid + i * 512;
            const int kr2 = c / (HD / 8), d8 = (c % (HD / 8)) * 8;
            const int g2 = kr2 / KT, kr = kr2 % KT;
            *reinterpret_cast<U4*>(&Ks[g2][kr * LDK + d8]) = kreg[i];
            const bf16_t* ve = reinterpret_cast<const bf16_t*>(&vreg[i]);
            const int col = (((kr >> 3) ^ ((d8 >> 3) & 3)) << 3) + (kr & 7);
#pragma unroll
            for (int e = 0; e < 8; ++e) Vt[g2][(d8 + e) * LDV + col] = ve[e];
        }
        __syncthreads();
        fetch(kreg, vreg, kt0 + 2 * NG * KT);
        const int kt = kt0 + grp * KT;                      // this group's keys
        // S = Q K^T for two 16-key sub-tiles: lane holds S[q = 4 fq + r][key = sub * 16 + fr]
        f32x4 sc[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            sc[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[grp][(sub * 16 + fr) * LDK + s * 32 + fq * 8]);
                sc[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[s], kf, sc[sub], 0, 0, 0);
            }
        }
        float pr[2][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qabs = pos0 + q0 + qw * 16 + fq * 4 + r;
            float s0 = sc[0][r] * p.scale, s1 = sc[1][r] * p.scale;
            if (kt + fr > qabs) s0 = -INFINITY;             // causal mask (also hides the rows re-read past the last key)
            if (kt + 16 + fr > qabs) s1 = -INFINITY;
            float mx = fmaxf(s0, s1);
            mx = fmaxf(mx, dpp_f<DPP_XOR1>(mx));
            mx = fmaxf(mx, dpp_f<DPP_XOR2>(mx));
            mx = fmaxf(mx, dpp_f<DPP_HALF_MIRROR>(mx));
            mx = fmaxf(mx, dpp_f<DPP_MIRROR>(mx));          // max over the row's 32 keys
            const float mn = fmaxf(mrun[r], mx);
            float corr = 1.f, p0 = 0.f, p1 = 0.f;
            if (mn > -INFINITY) {                           // rows past the prompt end may see nothing yet
                corr = expf(mrun[r] - mn);
                p0 = expf(s0 - mn);
                p1 = expf(s1 - mn);
            }
            mrun[r] = mn;
            lrun[r] = lrun[r] * corr + (p0 + p1);           // per-lane share of the row sum, reduced at the end
#pragma unroll
            for (int t = 0; t < NT; ++t) O[t][r] *= corr;
            pr[0][r] = p0; pr[1][r] = p1;
        }
        // P to the A-operand layout through this wave's LDS patch, split into two bf16 planes
        bf16_t* Ph = Ps[wave][0];
        bf16_t* Pl = Ps[wave][1];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = pr[sub][r];
                const bf16_t hi = f32_to_bf16_bits(v);
                const bf16_t lo = f32_to_bf16_bits(v - bf16_bits_to_f32(hi));
                Ph[(fq * 4 + r) * LDP + sub * 16 + fr] = hi;
                Pl[(fq * 4 + r) * LDP + sub * 16 + fr] = lo;
            }
        __syncthreads();
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(&Ph[fr * LDP + fq * 8]);
        const bf16x8 al = *reinterpret_cast<const bf16x8*>(&Pl[fr * LDP + fq * 8]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int d = t * 16 + fr;
            const bf16x8 vf = *reinterpret_cast<const bf16x8*>(&Vt[grp][d * LDV + ((fq ^ ((d >> 3) & 3)) << 3)]);
            O[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, vf, O[t], 0, 0, 0);
            O[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, vf, O[t], 0, 0, 0);
        }
    };
    // steps in pairs (one per register set); a tile wholly past the last visible key adds nothing (every score masked)
    for (int kt = 0; kt <= kmax; kt += 2 * NG * KT) {
        tile(kregA, vregA, kt);
        tile(kregB, vregB, kt + NG * KT);
    }
    // ---- merge of the two key groups: group 1 leaves (m, l, O) of its rows in LDS (the tile buffers are free now), group 0
    // rescales both to the common maximum and writes y
    __syncthreads();
    float* xbase = reinterpret_cast<float*>(smem_f + NG * KS_N);          // [NG - 1][QW][64 lanes][XW]
    if (grp > 0) {
        float* xch = xbase + ((size_t)((grp - 1) * QW + qw) * 64 + lane) * XW;
#pragma unroll
        for (int r = 0; r < 4; ++r) { xch[r] = mrun[r]; xch[4 + r] = lrun[r]; }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) xch[8 + t * 4 + r] = O[t][r];
    }
    __syncthreads();
    if (grp == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mn = mrun[r];
#pragma unroll
            for (int g = 1; g < NG; ++g) mn = fmaxf(mn, xbase[((size_t)((g - 1) * QW + qw) * 64 + lane) * XW + r]);
            const float c0 = mrun[r] > -INFINITY ? expf(mrun[r] - mn) : 0.f;
            float lsum = lrun[r] * c0;
            float cg[NG];
            cg[0] = c0;
#pragma unroll
            for (int g = 1; g < NG; ++g) {
                const float* xg = xbase + ((size_t)((g - 1) * QW + qw) * 64 + lane) * XW;
                cg[g] = xg[r] > -INFINITY ? expf(xg[r] - mn) : 0.f;
                lsum += xg[4 + r] * cg[g];
            }
            const float l = row16_sum(lsum);
            const int row = q0 + qw * 16 + fq * 4 + r;
            if (row < S) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    float o = O[t][r] * c0;
#pragma unroll
                    for (int g = 1; g < NG; ++g) o += xbase[((size_t)((g - 1) * QW + qw) * 64 + lane) * XW + 8 + t * 4 + r] * cg[g];
                    ybase[(size_t)row * p.H * HD + (size_t)h * HD + t * 16 + fr] = f32_to_bf16_bits(o / l);
                }
            }
        }
    }
}
template <int HD, int NG>
constexpr size_t flash_prefill_lds() { return (size_t)(NG * 32 * (HD + 8) + NG * HD * 40 + 8 * 2 * 16 * 40) * sizeof(bf16_t); }

// ---- skinny GEMM: few rows (prompt positions / lock-step utterances), weights streamed once ----------------------
// out[t][n] = sum_k X[t][k] W[n][k] for M <= 16*TS rows per block column.  The problem is weight-bandwidth bound,
// so the grid is cut along N only (16 weight rows per block => N/16 blocks) and the four waves of a block split K;
// fragments go straight from global memory into the MFMA operand registers (each lane's 16 bytes are one operand),
// the four partial tiles meet in LDS and are summed in wave order (deterministic).  Epilogue = the nn.Linear
// rounding points of the prefill (bias, rounded; residual add, rounded; SwiGLU on interleaved (gate, up) rows).
// Requires K % 128 == 0; act in {ACT_NONE, ACT_GELU, ACT_SWIGLU}; ntap == 1; one batch item (b = 0).
// XLDS: the X rows reach the MFMA operand registers through a per-wave LDS patch - loaded in full 256-byte row pieces
// (4 rows per load instruction) and re-read fragment-shaped with ds_read_b128 - instead of 16 rows x 64 bytes per load
// instruction straight from L2 (the per-CU address path was the limit of that form: tools/mb_skinny.hip).
constexpr int SKINNY_LDX = 136;   // LDS row stride of an X chunk (128 k + 8 pad, bf16): fragment reads spread over the banks
template <int TS, int NW>
constexpr size_t skinny_lds_bytes(bool xlds) {
    const size_t cs = (size_t)NW * TS * 16 * 17 * sizeof(float);
    const size_t xs = xlds ? (size_t)NW * TS * 16 * SKINNY_LDX * 2 : 0;
    return TS * 16 * sizeof(float) + (cs > xs ? cs : xs);
}
template <int TS, int NW, bool NORM, bool XLDS>
__global__ __launch_bounds__(NW * 64) void skinny_gemm_kernel(TapGemmP p) {
    constexpr int CH = 4;                          // k-steps (of 32) per register chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char skinny_smem[];
    float* inv_s = reinterpret_cast<float*>(skinny_smem);                                  // [TS*16]
    float (*Cs)[TS * 16][17] = reinterpret_cast<float (*)[TS * 16][17]>(skinny_smem + TS * 16 * sizeof(float));   // [NW]
    bf16_t* Xs = reinterpret_cast<bf16_t*>(skinny_smem + TS * 16 * sizeof(float));         // [NW][TS*16][SKINNY_LDX], aliases Cs
    const int kper = p.K / NW;                     // this wave's share of K (a multiple of 32)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * (16 * TS);
    if (!tap_segment(p, m0)) return;
    const int kw = wave * kper;
    const int nch = kper / (32 * CH);
    const int rem = (kper / 32) % CH;              // k-steps of a last partial chunk
    const bool nv = n0 + fr < p.N;
    const bf16_t* wrow = p.W + (size_t)(nv ? n0 + fr : 0) * (p.ldw ? p.ldw : p.K) + kw + fq * 8;
    const bf16_t* xrow[TS];
    bool tv[TS];
#pragma unroll
    for (int j = 0; j < TS; ++j) {
        const int t = m0 + j * 16 + fr;
        tv[j] = t < p.M;
        xrow[j] = p.X + (size_t)(tv[j] ? t : 0) * p.ldx + kw + fq * 8;
    }
    f32x4 acc[TS];
#pragma unroll
    for (int j = 0; j < TS; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const U4 zero = U4{0u, 0u, 0u, 0u};
    const bf16_t* grow = NORM ? p.gain + kw + fq * 8 : nullptr;
    auto load = [&](U4 (&w)[CH], U4 (&x)[TS][CH], U4 (&g)[CH], int k0, int steps) {
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            if (s < steps) {
                w[s] = nv ? *reinterpret_cast<const U4*>(wrow + k0 + s * 32) : zero;  // plain loads measured faster than nt here
                if constexpr (NORM) g[s] = *reinterpret_cast<const U4*>(grow + k0 + s * 32);
                if constexpr (!XLDS) {
#pragma unroll
                    for (int j = 0; j < TS; ++j) x[j][s] = tv[j] ? *reinterpret_cast<const U4*>(xrow[j] + k0 + s * 32) : zero;
                }
            }
        }
        if constexpr (XLDS) {
            // load instruction i = j*CH + s: rows 4i .. 4i+3 of the block column, 16 lanes x 16 B = one 256-byte row piece each
#pragma unroll
            for (int j = 0; j < TS; ++j)
#pragma unroll
                for (int s = 0; s < CH; ++s) {
                    const int row = (j * CH + s) * 4 + fq;
                    const bool ok = m0 + row < p.M && fr * 8 < steps * 32;
                    x[j][s] = ok ? *reinterpret_cast<const U4*>(p.X + (size_t)(m0 + row) * p.ldx + kw + k0 + fr * 8) : zero;
                }
        }
    };
    float inv[TS];
    if constexpr (NORM) {
        // 1/rms of every row of this block column from the producer's per-block partial sums of squares
        // one wave per row: its lanes fetch the row's partials in one coalesced load, DPP tree sum (fixed order)
        // (all of a wave's rows are fetched before the first reduction: one memory round trip, not one per row)
        constexpr int RPW = (TS * 16 + NW - 1) / NW;
        float ssr[RPW];
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            const int t = wave + i * NW, row = m0 + t;
            float ss = 0.f;
            if (t < TS * 16 && row < p.M)
                for (int b = lane; b < p.ss_nblk; b += 64) ss += p.ss_in[(size_t)row * p.ss_ld + b];
            ssr[i] = ss;
        }
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            const int t = wave + i * NW;
            const float ss = wave_sum(ssr[i]);
            if (t < TS * 16 && lane == 0) inv_s[t] = rsqrt_exact(ss / (float)p.K + p.eps);
        }
    }
    U4 wa[CH], wb[CH], xa[TS][CH], xb[TS][CH], ga[CH], gb[CH];
    if (nch > 0) load(wa, xa, ga, 0, CH);   // in flight while the norms are summed
    if constexpr (NORM) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TS; ++j) inv[j] = inv_s[j * 16 + fr];
    }
    bf16_t* xs_w = Xs + (size_t)wave * TS * 16 * SKINNY_LDX;   // this wave's patch
    auto compute = [&](const U4 (&w)[CH], const U4 (&x)[TS][CH], const U4 (&g)[CH], int steps) {
        if constexpr (XLDS) {
            // LDS operations of one wave execute in order: the fragment reads below see these writes without a barrier
#pragma unroll
            for (int j = 0; j < TS; ++j)
#pragma unroll
                for (int s = 0; s < CH; ++s)
                    *reinterpret_cast<U4*>(&xs_w[((j * CH + s) * 4 + fq) * SKINNY_LDX + fr * 8]) = x[j][s];
        }
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            if (s < steps) {
                bf16x8 b;
                __builtin_memcpy(&b, &w[s], 16);
                float gv[8];
                if constexpr (NORM) Vec<bf16_t>::unpack(g[s], gv);
#pragma unroll
                for (int j = 0; j < TS; ++j) {
                    bf16x8 a;
                    U4 xf;
                    if constexpr (XLDS) xf = *reinterpret_cast<const U4*>(&xs_w[(j * 16 + fr) * SKINNY_LDX + s * 32 + fq * 8]);
                    else xf = x[j][s];
                    if constexpr (NORM) {   // x -> round(round(x / rms) * gain), the two roundings of llama.py:172-177
                        float xv[8];
                        Vec<bf16_t>::unpack(xf, xv);
                        U4 o;
                        uint32_t* ow = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
                        for (int e = 0; e < 8; e += 2) {
                            const float y0 = round_bf16(xv[e] * inv[j]) * gv[e];
                            const float y1 = round_bf16(xv[e + 1] * inv[j]) * gv[e + 1];
                            ow[e >> 1] = (uint32_t)f32_to_bf16_bits(y0) | ((uint32_t)f32_to_bf16_bits(y1) << 16);
                        }
                        __builtin_memcpy(&a, &o, 16);
                    } else {
                        __builtin_memcpy(&a, &xf, 16);
                    }
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j], 0, 0, 0);
                }
            }
        }
    };
    for (int c = 0; c < nch; c += 2) {
        if (c + 1 < nch) load(wb, xb, gb, (c + 1) * 32 * CH, CH);
        compute(wa, xa, ga, CH);
        if (c + 2 < nch) load(wa, xa, ga, (c + 2) * 32 * CH, CH);
        if (c + 1 < nch) compute(wb, xb, gb, CH);
    }
    if (rem) {
        load(wa, xa, ga, nch * 32 * CH, rem);
        compute(wa, xa, ga, rem);
    }
    if constexpr (XLDS) __syncthreads();   // Cs aliases the X patches: every wave is done reading
    // lane holds C[token = j*16 + 4*fq + r][n = fr]
#pragma unroll
    for (int j = 0; j < TS; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) Cs[wave][j * 16 + fq * 4 + r][fr] = acc[j][r];
    __syncthreads();
    if (p.act == ACT_SWIGLU) {
        for (int e = tid; e < TS * 16 * 8; e += NW * 64) {
            const int row = e >> 3, c2 = (e & 7) * 2;
            const int t = m0 + row, n = n0 + c2;
            if (t >= p.M || n + 1 >= p.N) continue;
            float g = Cs[0][row][c2], u = Cs[0][row][c2 + 1];
#pragma unroll
            for (int w = 1; w < NW; ++w) { g += Cs[w][row][c2]; u += Cs[w][row][c2 + 1]; }
            if (p.bias) { g += p.bias[n % p.n_mod]; u += p.bias[(n + 1) % p.n_mod]; }
            if (p.round_lin) { g = round_bf16(g); u = round_bf16(u); }
            float sg = g / (1.0f + expf(-g));
            if (p.round_lin) sg = round_bf16(sg);
            const float o = sg * u;
            const size_t oi = (size_t)t * p.ldo + (n >> 1);
            if (p.out_bf) p.out_bf[oi] = f32_to_bf16_bits(o);
            if (p.out_f32) p.out_f32[oi] = p.round_f32_out ? round_bf16(o) : o;
        }
    } else {
        for (int e = tid; e < TS * 16 * 16; e += NW * 64) {
            const int row = e >> 4, c = e & 15;      // 16 consecutive lanes finish one row's 16 columns
            const int t = m0 + row, n = n0 + c;
            const bool ok = t < p.M && n < p.N;
            float stored = 0.f;
            if (ok) {
                float v = Cs[0][row][c];
#pragma unroll
                for (int w = 1; w < NW; ++w) v += Cs[w][row][c];
                if (p.bias) v += p.bias[n % p.n_mod];
                if (p.round_lin) v = round_bf16(v);
                if (p.act == ACT_GELU) v = gelu_f(v);                       // (codec: ConvNeXt pwconv1)
                if (p.gamma) v *= p.gamma[n % p.n_mod];                     // (codec: LayerScale / ConvNeXt gamma)
                if (p.resid_f32) v += p.resid_f32[(size_t)t * p.ldr + n];
                if (p.resid_bf) v += bf16_bits_to_f32(p.resid_bf[(size_t)t * p.ldr + n]);
                const size_t oi = (size_t)t * p.ldo + n;
                stored = p.round_f32_out ? round_bf16(v) : v;
                if (p.out_f32) p.out_f32[oi] = stored;
                if (p.out_bf) p.out_bf[oi] = f32_to_bf16_bits(v);
            }
            if (p.ss_out) {   // this block's share of the row's sum of squares, for the next GEMM's fused RMSNorm
                const float sq = row16_sum(stored * stored);
                if (c == 0 && t < p.M) p.ss_out[(size_t)t * p.ss_ld + blockIdx.x] = sq;
            }
        }
    }
}

// K split: 128-256 contraction steps per wave (one or two register chunks = a single memory round trip per wave)
static inline int skinny_waves(int N, int K, int TS) {
    if (TS < 4 && K % 384 == 0 && K / 12 >= 128) return 12;   // 3072 -> 12 x 256 (TS = 4 would spill registers)
    if (K % 256 == 0 && (K / 8 >= 256 || (N <= 2048 && K / 8 >= 128))) return 8;
    return 4;
}
template <int TS>
static inline void skinny_gemm_launch(const TapGemmP& p, int gy, hipStream_t st, int gz = 1) {
    const dim3 grid((p.N + 15) / 16, gy, gz);
    int nw = skinny_waves(p.N, p.K, TS);
    if (p.gain && TS == 4) nw = 4;   // the fused norm's extra registers: keep the 64-row variant off the spill edge
#define FT_SK(NWV, NORMV, XV)                                                                                       \
    do {                                                                                                              \
        constexpr size_t lds_ = skinny_lds_bytes<TS, NWV>(XV);                                                        \
        static DevOnce once_;                                                                                         \
        if (lds_ > 48 * 1024)                                                                                         \
            once_.run([] { hipFuncSetAttribute((const void*)skinny_gemm_kernel<TS, NWV, NORMV, XV>,                   \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_); });            \
        skinny_gemm_kernel<TS, NWV, NORMV, XV><<<grid, NWV * 64, lds_, st>>>(p);                                      \
    } while (0)
#define FT_SK_X(NWV, NORMV) FT_SK(NWV, NORMV, true)      /* X rows staged through LDS (the direct fragment loads were slower) */
    if (p.gain) {
        switch (nw) {
            case 12: FT_SK_X(12, true); break;
            case 8: FT_SK_X(8, true); break;
            default: FT_SK_X(4, true);
        }
    } else {
        switch (nw) {
            case 12: FT_SK_X(12, false); break;
            case 8: FT_SK_X(8, false); break;
            default: FT_SK_X(4, false);
        }
    }
#undef FT_SK_X
#undef FT_SK
}

// ---- residual vector quantiser decode (vocoder.py:800-811): x[t][:] = sum_i table_i[code_i[t]][:]
// table_i = out_proj_i(codebook_i) + bias_i, precomputed in f32 at load time.
struct RvqP {
    const int* codes;        // [B][ncb+1][T]
    const float* tables;     // semantic table [S0][D] followed by ncb tables [S][D]
    int ncb, S0, S, D, T;
    float* x;                // [B][T][D] f32
};
static __global__ __launch_bounds__(256) void rvq_gather_kernel(RvqP p) {
    const int t = blockIdx.x, b = blockIdx.y;
    const int* cd = p.codes + (size_t)b * (p.ncb + 1) * p.T;
    for (int d = threadIdx.x; d < p.D; d += 256) {
        int c0 = cd[t];
        c0 = c0 < 0 ? 0 : (c0 >= p.S0 ? p.S0 - 1 : c0);
        float zs = p.tables[(size_t)c0 * p.D + d];
        float zr = 0.f;
        for (int i = 0; i < p.ncb; ++i) {
            int c = cd[(size_t)(i + 1) * p.T + t];
            c = c < 0 ? 0 : (c >= p.S ? p.S - 1 : c);
            zr += p.tables[((size_t)p.S0 + (size_t)i * p.S + c) * p.D + d];
        }
        p.x[((size_t)b * p.T + t) * p.D + d] = zs + zr;
    }
}
static __global__ void rvq_table_kernel(const float* cb, const float* w, const float* bias, float* table, int S, int D, int cd) {
    // table[s][d] = sum_j w[d][j] * cb[s][j] + bias[d]
    const long n = (long)S * D;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int s = (int)(i / D), d = (int)(i % D);
        float a = 0.f;
        for (int j = 0; j < cd; ++j) a += w[(size_t)d * cd + j] * cb[(size_t)s * cd + j];
        table[i] = a + bias[d];
    }
}

// ---- RMSNorm over rows (vocoder.py:94-102), f32 in -> bf16 (and optionally f32) out
struct RowNormP {
    const float* x;
    const float* w;
    float eps;
    int D;
    bf16_t* out_bf;
    float* out_f32;
};
static __global__ __launch_bounds__(256) void rmsnorm_rows_kernel(RowNormP p) {
    __shared__ float red[4];
    const size_t row = blockIdx.x;
    const float* x = p.x + row * p.D;
    float ss = 0.f;
    for (int d = threadIdx.x; d < p.D; d += 256) ss = fmaf(x[d], x[d], ss);
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float inv = rsqrt_exact((((red[0] + red[1]) + red[2]) + red[3]) / (float)p.D + p.eps);
    for (int d = threadIdx.x; d < p.D; d += 256) {
        const float v = (x[d] * inv) * p.w[d];
        if (p.out_bf) p.out_bf[row * p.D + d] = f32_to_bf16_bits(v);
        if (p.out_f32) p.out_f32[row * p.D + d] = v;
    }
}

// ---- RoPE on the q and k thirds of a [T][3*H*hd] bf16 buffer, in place (vocoder.py:145-156)
static __global__ void rope_qk_kernel(bf16_t* qkv, const float* tab, int T, int H, int hd, int pos0 = 0, SegZ z = SegZ{}) {
    if (z.seg) {   // chunk z: its rows, its rope position
        const int4 s = z.get();
        qkv += z.row0(s) * 3 * H * hd;
        T = s.y;
        pos0 = s.z;
    }
    const int hp = hd >> 1;
    const long n = (long)T * 2 * H * hp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int pr = (int)(i % hp);
        const int h = (int)((i / hp) % (2 * H));  // q heads then k heads
        const int t = (int)(i / ((long)hp * 2 * H));
        bf16_t* v = qkv + (size_t)t * 3 * H * hd + (size_t)h * hd + 2 * pr;
        const float x0 = bf16_bits_to_f32(v[0]), x1 = bf16_bits_to_f32(v[1]);
        const float c = tab[((size_t)(t + pos0) * hp + pr) * 2], s = tab[((size_t)(t + pos0) * hp + pr) * 2 + 1];
        v[0] = f32_to_bf16_bits(x0 * c - x1 * s);
        v[1] = f32_to_bf16_bits(x1 * c + x0 * s);
    }
}

// ---- window-limited causal attention (vocoder.py:210-214 with the band mask of 325-332):
// one wave per (query t, head); lanes over keys for the scores, lanes over dims for P.V
struct WinAttnP {
    const bf16_t* qkv;  // [T][3*H*hd], q and k already rotated
    bf16_t* y;          // [T][H*hd]
    int T, H, hd, window;
    float scale;
    int t0;             // first query row (0; streamed decode: rows [0, t0) are the carried K/V of earlier chunks); y row = t - t0
    SegZ z;             // batched streamed decode: chunk z's qkv rows (carried rows in front) and its compact y rows
};
static __global__ __launch_bounds__(256) void window_attn_kernel(WinAttnP p) {
    __shared__ float q_s[4][128];
    __shared__ float p_s[4][512];   // window <= 512 (the encoder's transformer, vocoder.py:516)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (p.z.seg) {
        const int4 s = p.z.get();
        p.qkv += (p.z.row0(s) - s.w) * 3 * p.H * p.hd;
        p.y += (size_t)s.x * p.H * p.hd;
        p.T = s.w + s.y;
        p.t0 = s.w;
    }
    const long item = (long)blockIdx.x * 4 + wave;
    if (item >= (long)(p.T - p.t0) * p.H) return;
    const int t = p.t0 + (int)(item / p.H), h = (int)(item % p.H);
    const int hd = p.hd, ld = 3 * p.H * hd;
    const bf16_t* q = p.qkv + (size_t)t * ld + (size_t)h * hd;
    for (int d = lane; d < hd; d += 64) q_s[wave][d] = bf16_bits_to_f32(q[d]);
    __builtin_amdgcn_wave_barrier();
    const int j0 = max(0, t - p.window + 1);
    const int nk = t - j0 + 1;
    float mx = -INFINITY;
    for (int jj = lane; jj < nk; jj += 64) {
        const bf16_t* k = p.qkv + (size_t)(j0 + jj) * ld + (size_t)(p.H + h) * hd;
        float s = 0.f;
        for (int d = 0; d < hd; d += 8) {
            float kv[8];
            Vec<bf16_t>::load(k + d, kv);
#pragma unroll
            for (int e = 0; e < 8; ++e) s = fmaf(q_s[wave][d + e], kv[e], s);
        }
        s *= p.scale;
        p_s[wave][jj] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int jj = lane; jj < nk; jj += 64) {
        const float e = expf(p_s[wave][jj] - mx);
        p_s[wave][jj] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    __builtin_amdgcn_wave_barrier();
    for (int d = lane; d < hd; d += 64) {
        float o = 0.f;
        for (int jj = 0; jj < nk; ++jj)
            o = fmaf(p_s[wave][jj], bf16_bits_to_f32(p.qkv[(size_t)(j0 + jj) * ld + (size_t)(2 * p.H + h) * hd + d]), o);
        p.y[(size_t)(t - p.t0) * p.H * hd + (size_t)h * hd + d] = f32_to_bf16_bits(o / sum);
    }
}

// ---- ConvNeXt front half (vocoder.py:667-671): depthwise causal conv k=7 + LayerNorm(eps 1e-6)
struct DwLnP {
    const bf16_t* x;   // [T][C]
    const float* w;    // [C][7]
    const float* b;    // [C]
    const float* lw;
    const float* lb;
    int T, C;
    bf16_t* out;       // [T][C]
    int t_min;         // lowest readable row of x (as TapGemmP::t_min)
    SegZ z;            // batched streamed decode: chunk z's rows of x and out
};
static __global__ __launch_bounds__(256) void dwconv_ln_kernel(DwLnP p) {
    __shared__ float red[8];
    extern __shared__ float ybuf[];  // [C]
    const int t = blockIdx.x;
    if (p.z.seg) {
        const int4 s = p.z.get();
        if (t >= s.y * p.z.m) return;
        p.x += p.z.row0(s) * p.C;
        p.out += p.z.row0(s) * p.C;
    }
    float s1 = 0.f;
    for (int c = threadIdx.x; c < p.C; c += 256) {
        float a = p.b[c];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int tt = t - 6 + k;
            if (tt >= p.t_min) a = fmaf(p.w[c * 7 + k], bf16_bits_to_f32(p.x[(long)tt * p.C + c]), a);
        }
        ybuf[c] = a;
        s1 += a;
    }
    s1 = wave_sum(s1);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s1;
    __syncthreads();
    const float mean = (((red[0] + red[1]) + red[2]) + red[3]) / (float)p.C;
    float s2 = 0.f;
    for (int c = threadIdx.x; c < p.C; c += 256) { const float d = ybuf[c] - mean; s2 = fmaf(d, d, s2); }
    s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) red[4 + (threadIdx.x >> 6)] = s2;
    __syncthreads();
    const float var = (((red[4] + red[5]) + red[6]) + red[7]) / (float)p.C;
    const float inv = rsqrt_exact(var + 1e-6f);
    for (int c = threadIdx.x; c < p.C; c += 256)
        p.out[(size_t)t * p.C + c] = f32_to_bf16_bits((ybuf[c] - mean) * inv * p.lw[c] + p.lb[c]);
}

// ---- last layer (vocoder.py:631-635): conv k=7 C->1 on the snake'd input, tanh -> f32 audio
struct FinalConvP {
    const bf16_t* xs;  // [T][C]
    const float* w;    // [7][C]
    float bias;
    int T, C;
    float* audio;      // [T]
    int t_min;         // lowest readable row of xs (as TapGemmP::t_min)
    SegZ z;            // batched streamed decode: chunk z's rows of xs; its audio at P * m (chunks back to back)
};
static __global__ __launch_bounds__(256) void final_conv_tanh_kernel(FinalConvP p) {
    if (p.z.seg) {
        const int4 s = p.z.get();
        p.xs += p.z.row0(s) * p.C;
        p.audio += (long)s.x * p.z.m;
        p.T = s.y * p.z.m;
    }
    // 16 lanes per output sample, 16 samples per block step.  C % 8 == 0 and C <= 128: lane `sub` owns channels
    // 8 sub .. 8 sub + 7 - one 16-byte load per tap and sample, its 7 x 8 weights stay in registers (the first version read
    // 2-byte elements with a 32-byte stride: 150 us for 85 MB)
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
    if (p.C % 8 == 0 && p.C <= 128) {
        const bool on = sub * 8 < p.C;
        float wv[7][8];
#pragma unroll
        for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) wv[k][j] = on ? p.w[k * p.C + sub * 8 + j] : 0.f;
        for (long t = (long)blockIdx.x * 16 + grp; t < p.T; t += (long)gridDim.x * 16) {
            U4 x[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const long tt = t - 6 + k;
                x[k] = (on && tt >= p.t_min) ? *reinterpret_cast<const U4*>(p.xs + tt * p.C + sub * 8) : U4{0u, 0u, 0u, 0u};
            }
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                float xv[8];
                Vec<bf16_t>::unpack(x[k], xv);
#pragma unroll
                for (int j = 0; j < 8; ++j) a = fmaf(wv[k][j], xv[j], a);
            }
            a = row16_sum(a);
            if (sub == 0) p.audio[t] = tanhf(a + p.bias);
        }
        return;
    }
    for (long t = (long)blockIdx.x * 16 + grp; t < p.T; t += (long)gridDim.x * 16) {
        float a = 0.f;
        for (int k = 0; k < 7; ++k) {
            const long tt = t - 6 + k;
            if (tt < p.t_min) continue;
            for (int c = sub; c < p.C; c += 16) a = fmaf(p.w[k * p.C + c], bf16_bits_to_f32(p.xs[tt * p.C + c]), a);
        }
        a = row16_sum(a);
        if (sub == 0) p.audio[t] = tanhf(a + p.bias);
    }
}

// ---- weight repacks
static __global__ void pack_conv_kernel(const float* w, bf16_t* o, int Cout, int Cin, int k) {
    // [Cout][Cin][k] -> [k][Cout][Cin]
    const long n = (long)Cout * Cin * k;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int kk = (int)(i % k), ci = (int)((i / k) % Cin), co = (int)(i / ((long)k * Cin));
        o[((size_t)kk * Cout + co) * Cin + ci] = f32_to_bf16_bits(w[i]);
    }
}
static __global__ void pack_convT_kernel(const float* w, bf16_t* o, int Cin, int Cout, int k, int s) {
    // [Cin][Cout][k] -> [k/s taps][s*Cout][Cin]; tap j, column (r, co) <- w[ci][co][r + j*s]
    const long n = (long)Cin * Cout * k;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int kk = (int)(i % k), co = (int)((i / k) % Cout), ci = (int)(i / ((long)k * Cout));
        const int j = kk / s, r = kk % s;
        o[((size_t)j * s * Cout + (size_t)r * Cout + co) * Cin + ci] = f32_to_bf16_bits(w[i]);
    }
}
static __global__ void pack_rows_kernel(const float* w, bf16_t* o, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        o[i] = f32_to_bf16_bits(w[i]);
}
static __global__ void pack_interleave_kernel(const float* a, const float* b, bf16_t* o, long rows, long K) {
    const long n = rows * K;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / K, k = i % K;
        o[(2 * r) * K + k] = f32_to_bf16_bits(a[i]);
        o[(2 * r + 1) * K + k] = f32_to_bf16_bits(b[i]);
    }
}
// ---- encode side (DAC.encode, vocoder.py:885-904) ------------------------------------------------------------------
// strided causal conv (CausalConvNet with stride s, kernel k = taps*s, left pad k - s; vocoder.py:394-421) as a tap GEMM
// over the [T/s][s*Cin] view of the time-major input: [Cout][Cin][k] -> [taps][Cout][s*Cin],
// tap a (row offset a - (taps-1)), column jj*Cin + ci <- w[co][ci][a*s + jj]
static __global__ void pack_strided_conv_kernel(const float* w, bf16_t* o, int Cout, int Cin, int k, int s) {
    const long n = (long)Cout * Cin * k;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int kk = (int)(i % k), ci = (int)((i / k) % Cin), co = (int)(i / ((long)k * Cin));
        const int a = kk / s, jj = kk % s;
        o[((size_t)a * Cout + co) * ((size_t)s * Cin) + (size_t)jj * Cin + ci] = f32_to_bf16_bits(w[i]);
    }
}
// first encoder conv: 1 input channel, k = 7, causal (vocoder.py:552): raw output and the Snake'd copy the first
// residual unit reads
struct EncInP {
    const float* audio;  // [T]
    const float* w;      // [C][7]
    const float* b;      // [C]
    const float* alpha;  // [C]
    long T;
    int C;
    bf16_t* raw;         // [T][C]
    bf16_t* act;         // [T][C]
};
static __global__ __launch_bounds__(256) void enc_conv_in_kernel(EncInP p) {
    const long n = p.T * p.C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long t = i / p.C;
        const int c = (int)(i % p.C);
        float acc = p.b[c];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const long tt = t - 6 + j;
            if (tt >= 0) acc = fmaf(p.w[c * 7 + j], p.audio[tt], acc);
        }
        p.raw[i] = f32_to_bf16_bits(acc);
        p.act[i] = f32_to_bf16_bits(snake_f(acc, p.alpha[c]));
    }
}
static __global__ void snake_bf_rows_kernel(const bf16_t* x, const float* alpha, bf16_t* out, long n, int C) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = f32_to_bf16_bits(snake_f(bf16_bits_to_f32(x[i]), alpha[i % C]));
}
static __global__ void bf16_rows_to_f32_kernel(const bf16_t* x, float* out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = bf16_bits_to_f32(x[i]);
}
// L2-normalised codebook rows and their squared norms (dac VectorQuantize.decode_latents)
static __global__ void normalize_codebook_kernel(const float* cb, float* cbn, float* cn2, int N, int cd) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        float ss = 0.f;
        for (int c = 0; c < cd; ++c) ss += cb[(size_t)i * cd + c] * cb[(size_t)i * cd + c];
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);   // F.normalize eps
        float s2 = 0.f;
        for (int c = 0; c < cd; ++c) {
            const float v = cb[(size_t)i * cd + c] * inv;
            cbn[(size_t)i * cd + c] = v;
            s2 += v * v;
        }
        cn2[i] = s2;
    }
}
// Residual vector quantiser search (vocoder.py:765-779 + dac ResidualVectorQuantize.forward): per frame, for every
// codebook in turn: e = in_proj(residual); nearest codebook row by distance between the L2-normalised vectors
// (first index on ties, as torch.max); residual -= out_proj(codebook[idx]) (the folded decode table).  One block per frame.
struct RvqEncP {
    const float* z;       // [T][D]
    const float* inw;     // [R][cd][D]
    const float* inb;     // [R][cd]
    const float* cbn;     // normalised codebooks: [S0][cd] then (R-1) x [S][cd]
    const float* cn2;     // their squared norms, same order
    const float* tables;  // decode tables [S0][D] then (R-1) x [S][D]
    int R, S0, S, D, cd, T;
    int* codes;           // [R][T]
};
static __global__ __launch_bounds__(256) void rvq_encode_kernel(RvqEncP p) {
    extern __shared__ float res[];           // [D]
    __shared__ double part[4][16];
    __shared__ float e_s[16];
    __shared__ float bestv[4];
    __shared__ int besti[4];
    __shared__ int pick;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = p.D, cd = p.cd;
    for (int d = tid; d < D; d += 256) res[d] = p.z[(size_t)t * D + d];
    __syncthreads();
    for (int q = 0; q < p.R; ++q) {
        const float* W = p.inw + (size_t)q * cd * D;
        // the projection is accumulated in f64 (f32 operands): its f32 result is then the correctly rounded one at any width
        // (1024 at the real shapes), so an index can differ from an f32 evaluation only where that evaluation's own
        // accumulation error decides
        for (int c = 0; c < cd; ++c) {
            double a = 0.0;
            for (int d = tid; d < D; d += 256) a = fma((double)W[(size_t)c * D + d], (double)res[d], a);
            for (int sft = 32; sft >= 1; sft >>= 1) a += __shfl_xor(a, sft);
            if (lane == 0) part[wave][c] = a;
        }
        __syncthreads();
        if (tid < cd) e_s[tid] = (float)((((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]) + (double)p.inb[q * cd + tid]);
        __syncthreads();
        float nn = 0.f;
        for (int c = 0; c < cd; ++c) nn += e_s[c] * e_s[c];
        const float inv = 1.0f / fmaxf(sqrtf(nn), 1e-12f);
        float en[16];
        float l2 = 0.f;
        for (int c = 0; c < cd; ++c) { en[c] = e_s[c] * inv; l2 += en[c] * en[c]; }
        const int N = q == 0 ? p.S0 : p.S;
        const size_t off = q == 0 ? 0 : (size_t)p.S0 + (size_t)(q - 1) * p.S;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid; i < N; i += 256) {
            float dot = 0.f;
            for (int c = 0; c < cd; ++c) dot = fmaf(en[c], p.cbn[(off + i) * cd + c], dot);
            const float score = -((l2 - 2.0f * dot) + p.cn2[off + i]);
            if (score > bv) { bv = score; bi = i; }          // ascending i per thread: first maximum stays
        }
        for (int sft = 32; sft >= 1; sft >>= 1) {
            const float ov = __shfl_xor(bv, sft);
            const int oi = __shfl_xor(bi, sft);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { bestv[wave] = bv; besti[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            float v = bestv[0]; int ix = besti[0];
            for (int w = 1; w < 4; ++w) if (bestv[w] > v || (bestv[w] == v && besti[w] < ix)) { v = bestv[w]; ix = besti[w]; }
            pick = ix;
            p.codes[(size_t)q * p.T + t] = ix;
        }
        __syncthreads();
        const float* row = p.tables + (off + (size_t)pick) * D;
        for (int d = tid; d < D; d += 256) res[d] -= row[d];
        __syncthreads();
    }
}

static __global__ void snake_rows_kernel(const float* x, const float* alpha, bf16_t* out, long T, int C) {
    const long n = T * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = f32_to_bf16_bits(snake_f(x[i], alpha[i % C]));
}

// ---- streamed decode: carried context (ft_codec_stream_*)
// A causal convolution of halo H reads rows [-H, 0) of its input: the last H rows of the input of all earlier chunks.
// tail_roll_kernel (a) copies the carried rows in front of the chunk (x[-H .. 0)) and (b) leaves the carry of the NEXT chunk:
// the last H rows of (carried rows ++ this chunk's T rows).  16-byte pieces; C % 8 == 0.
static __global__ void tail_roll_kernel(bf16_t* x, const bf16_t* tail_in, bf16_t* tail_out, int T, int H, int C,
                                        SegZ z = SegZ{}) {
    if (z.seg) {   // chunk z: its rows, its stream's carry
        const int4 s = z.get();
        x += z.row0(s) * C;
        T = s.y * z.m;
        tail_in = z.carry_in();
        tail_out = z.carry_out();
    }
    const int per = C / 8;
    const long n = (long)H * per;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i / per), q = (int)(i % per);
        const U4 old = *reinterpret_cast<const U4*>(tail_in + (size_t)r * C + q * 8);
        *reinterpret_cast<U4*>(x + ((long)r - H) * C + q * 8) = old;
        const int src = r + T - H;          // row of the chunk that becomes carried row r (negative: still a carried row)
        const U4 nv = src >= 0 ? *reinterpret_cast<const U4*>(x + (long)src * C + q * 8)
                               : *reinterpret_cast<const U4*>(tail_in + (size_t)(r + T) * C + q * 8);
        *reinterpret_cast<U4*>(tail_out + (size_t)r * C + q * 8) = nv;
    }
}
// The K and V of the last nh rows before a chunk (window attention): kv_in [W1][2 * HD] -> rows [0, nh) of the qkv work
// buffer (its k and v thirds; carried rows sit at the END of kv_in), and the carry of the next chunk from rows
// [nh + T - nh2, nh + T) of the work buffer.  Two launches (the second reads what the GEMM wrote after the first).
// Batched (z.seg): qkv points at the row of chunk 0's first query row (SegZ rows), nh and the carry are chunk z's.
static __global__ void kv_carry_in_kernel(bf16_t* qkv, const bf16_t* kv_in, int nh, int W1, int HD, SegZ z = SegZ{}) {
    if (z.seg) {
        const int4 s = z.get();
        nh = s.w;
        qkv += (z.row0(s) - nh) * 3 * HD;
        kv_in = z.carry_in();
    }
    const int per = 2 * HD / 8;
    const long n = (long)nh * per;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i / per), q = (int)(i % per);
        *reinterpret_cast<U4*>(qkv + (size_t)r * 3 * HD + HD + q * 8) =
            *reinterpret_cast<const U4*>(kv_in + (size_t)(W1 - nh + r) * 2 * HD + q * 8);
    }
}
static __global__ void kv_carry_out_kernel(const bf16_t* qkv, bf16_t* kv_out, int rows, int nh2, int W1, int HD,
                                           SegZ z = SegZ{}) {
    if (z.seg) {
        const int4 s = z.get();
        qkv += (z.row0(s) - s.w) * 3 * HD;
        rows = s.w + s.y;
        nh2 = min(W1, rows);
        kv_out = z.carry_out();
    }
    const int per = 2 * HD / 8;
    const long n = (long)nh2 * per;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i / per), q = (int)(i % per);
        *reinterpret_cast<U4*>(kv_out + (size_t)(W1 - nh2 + r) * 2 * HD + q * 8) =
            *reinterpret_cast<const U4*>(qkv + (size_t)(rows - nh2 + r) * 3 * HD + HD + q * 8);
    }
}

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
