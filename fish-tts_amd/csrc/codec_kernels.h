// DAC codec model kernels for gfx950: what the decode and encode passes launch beside the tap GEMMs of gemm_kernels.h - the
// RVQ gather and search, RMSNorm, RoPE, the window attention, the ConvNeXt front half, the last layer, the weight repacks and
// the carried context of a streamed decode.  Activations are time-major [T][C] bf16 in HBM (the transformer's residual stream
// is f32).  The output stages behind the model live in stage_kernels.h.  codec.hip launches these kernels; engine.hip
// includes the header too and launches none of them ("Kernel headers": without them its own kernels move
// and the AR path measures slower), so a kernel added or changed here moves the AR engine's code.
#pragma once
#include "gemm_kernels.h"

namespace ft {

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

}  // namespace ft
