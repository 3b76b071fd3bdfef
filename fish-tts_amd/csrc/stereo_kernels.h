// The stereo mix stage's kernels (ft_codec_mix_stereo; stated in fishtts_hip.h under "Stereo mix"): mix_stereo_kernel and the
// two kernels of the pair level.  They build on codec_kernels.h - MixP, mix_prog, mix_sample, the level table - and are
// included behind it by codec.hip alone: engine.hip includes codec_kernels.h, so a kernel added there lands in the AR
// engine's code object as well and moves its kernels (measured: 0.7 % of bench.py's tokens per second; DESIGN section 8,
// "Stereo").
#pragma once
#include "codec_kernels.h"

namespace ft {

// ---- stereo mix stage (ft_codec_mix_stereo; stated in fishtts_hip.h under "Stereo mix"): the mix stage with the mono
// programme panned by regions and the bed's two sides kept apart, frames interleaved in y.  mix_hop_kernel and
// mix_node_kernel run as they are (the activity and the duck come from the mono programme), mix_scale_kernel over the 2 N
// floats, and in mix_kernel's place:
//   mix_stereo_kernel  a workgroup per MX_SPAN frames, four per lane and step, mix_kernel's loads (16 bytes of the programme
//                      and of either side under its conditions) and two 16-byte stores of y per four frames.  The regions
//                      that meet the span are found once per workgroup: lane 0 searches the sorted table for the first
//                      region that ends behind the span's first frame and the first that begins behind its last, the
//                      workgroup packs those (at most one per frame: 12 + 12 + 8 bits each) into LDS, and every lane then
//                      writes the pan of its 16 consecutive frames - one search of the packed words for the first of them,
//                      a walk over the rest - as bytes.  The sample loop reads four pans with one LDS load; the table U
//                      lies in LDS too.  The peak over both channels, one integer atomicMax per workgroup.
struct MixPan { long long a, e; int pan, reserved; };      // ft_pan_region
struct MixSP {
    MixP m;                    // as ft_codec_mix fills it: bed is side 0, y has 2 N floats; without a bed nb = 0 and loop = 0
    const float* bed1;         // side 1 (bed itself where both sides are one; device, 16-byte aligned)
    const MixPan* reg;         // [R], sorted and disjoint, in programme samples
    const float* U;            // [MS_PANS]
    int R;
};
constexpr int MS_PANS = 201, MS_CENTRE = 100;

// Side sample at position j of the bed (mix_bed for either side).
__device__ inline float mix_side(const MixP& p, const float* bed, long long j) {
    if (p.loop) return bed[j % p.nb];
    return j < p.nb ? bed[j] : 0.f;
}

static __global__ __launch_bounds__(MX_THREADS) void mix_stereo_kernel(MixSP sp) {
    const MixP& p = sp.m;
    __shared__ float wpk[MX_THREADS / 64];
    __shared__ float U[MS_PANS];
    __shared__ unsigned int seg[MX_SPAN];                  // first frame | last frame << 12 | (pan + 100) << 24, from `base`
    __shared__ __align__(16) unsigned char pan[MX_SPAN];   // pan + 100 per frame of the span
    __shared__ int found[2];
    const int base = blockIdx.x * MX_SPAN;
    const long long lo = (long long)base - p.lead, hi = lo + MX_SPAN;      // the span in programme samples
    if (threadIdx.x == 0) {
        int a = 0, b = sp.R;                               // the first region that ends behind lo
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (sp.reg[mid].e > lo) b = mid; else a = mid + 1;
        }
        found[0] = a;
        b = sp.R;                                          // the first region that begins at or behind hi
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (sp.reg[mid].a >= hi) b = mid; else a = mid + 1;
        }
        found[1] = a;
    }
    for (int j = threadIdx.x; j < MS_PANS; j += MX_THREADS) U[j] = sp.U[j];
    __syncthreads();
    const int r0 = found[0], C = found[1] - r0;            // C <= MX_SPAN: the regions are disjoint and each holds a frame of the span
    for (int c = threadIdx.x; c < C; c += MX_THREADS) {
        const MixPan g = sp.reg[r0 + c];
        const unsigned int f0 = (unsigned int)max(g.a - lo, 0LL), f1 = (unsigned int)(min(g.e - lo, (long long)MX_SPAN) - 1);
        seg[c] = f0 | f1 << 12 | (unsigned int)(g.pan + MS_CENTRE) << 24;
    }
    __syncthreads();
    {
        const unsigned int f0 = 16 * threadIdx.x;
        int c = 0, b = C;                                  // the first packed region whose last frame is at or behind f0
        while (c < b) {
            const int mid = (c + b) >> 1;
            if ((seg[mid] >> 12 & 4095u) >= f0) b = mid; else c = mid + 1;
        }
        unsigned int w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const unsigned int f = f0 + k;
            while (c < C && (seg[c] >> 12 & 4095u) < f) ++c;
            const unsigned int q = c < C && (seg[c] & 4095u) <= f ? seg[c] >> 24 : (unsigned int)MS_CENTRE;
            w[k >> 2] |= q << (8 * (k & 3));
        }
        ((uint4*)pan)[threadIdx.x] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
    const int N4 = p.N >> 2;
    const bool xal = (p.lead & 3) == 0, one = sp.bed1 == p.bed;
    float pk = 0.f;
    for (int st = 0; st < MX_STEPS; ++st) {
        const int q = (blockIdx.x * MX_STEPS + st) * MX_THREADS + threadIdx.x, i = 4 * q;
        if (q >= N4) break;
        float4 s, t0, t1;
        const int a = i - p.lead;
        if (xal && a >= 0 && a + 3 < p.n) s = *(const float4*)(p.x + a);
        else s = make_float4(mix_prog(p, i), mix_prog(p, i + 1), mix_prog(p, i + 2), mix_prog(p, i + 3));
        long long j = (long long)i + p.off;
        if (p.loop) j %= p.nb;
        const bool wide = (j & 3) == 0 && j + 3 < p.nb;
        if (wide) t0 = *(const float4*)(p.bed + j);
        else t0 = make_float4(mix_side(p, p.bed, j), mix_side(p, p.bed, j + 1), mix_side(p, p.bed, j + 2), mix_side(p, p.bed, j + 3));
        if (one) t1 = t0;
        else if (wide) t1 = *(const float4*)(sp.bed1 + j);
        else t1 = make_float4(mix_side(p, sp.bed1, j), mix_side(p, sp.bed1, j + 1), mix_side(p, sp.bed1, j + 2), mix_side(p, sp.bed1, j + 3));
        const unsigned int pq = *(const unsigned int*)(pan + (i - base));
        const unsigned int q0 = pq & 255u, q1 = pq >> 8 & 255u, q2 = pq >> 16 & 255u, q3 = pq >> 24;
        float4 m0, m1;                                     // frames i, i + 1 and i + 2, i + 3: left, right, left, right
        m0.x = mix_sample(p, i, __fmul_rn(s.x, U[2 * MS_CENTRE - q0]), t0.x);
        m0.y = mix_sample(p, i, __fmul_rn(s.x, U[q0]), t1.x);
        m0.z = mix_sample(p, i + 1, __fmul_rn(s.y, U[2 * MS_CENTRE - q1]), t0.y);
        m0.w = mix_sample(p, i + 1, __fmul_rn(s.y, U[q1]), t1.y);
        m1.x = mix_sample(p, i + 2, __fmul_rn(s.z, U[2 * MS_CENTRE - q2]), t0.z);
        m1.y = mix_sample(p, i + 2, __fmul_rn(s.z, U[q2]), t1.z);
        m1.z = mix_sample(p, i + 3, __fmul_rn(s.w, U[2 * MS_CENTRE - q3]), t0.w);
        m1.w = mix_sample(p, i + 3, __fmul_rn(s.w, U[q3]), t1.w);
        ((float4*)p.y)[2 * q] = m0;
        ((float4*)p.y)[2 * q + 1] = m1;
        pk = fmaxf(pk, fmaxf(fmaxf(fmaxf(fabsf(m0.x), fabsf(m0.y)), fmaxf(fabsf(m0.z), fabsf(m0.w))),
                             fmaxf(fmaxf(fabsf(m1.x), fabsf(m1.y)), fmaxf(fabsf(m1.z), fabsf(m1.w)))));
    }
    // the up to three frames behind the last whole group: the workgroup that owns position N4
    if (4 * N4 < p.N && N4 / (MX_THREADS * MX_STEPS) == (int)blockIdx.x && threadIdx.x < p.N - 4 * N4) {
        const int i = 4 * N4 + threadIdx.x;
        const unsigned int q = pan[i - base];
        const float s = mix_prog(p, i);
        const long long j = (long long)i + p.off;
        const float l = mix_sample(p, i, __fmul_rn(s, U[2 * MS_CENTRE - q]), mix_side(p, p.bed, j));
        const float r = mix_sample(p, i, __fmul_rn(s, U[q]), mix_side(p, sp.bed1, j));
        *(float2*)(p.y + 2 * (size_t)i) = make_float2(l, r);
        pk = fmaxf(pk, fmaxf(fabsf(l), fabsf(r)));
    }
    for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o));
    if ((threadIdx.x & 63) == 0) wpk[threadIdx.x >> 6] = pk;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MX_THREADS / 64; ++w) pk = fmaxf(pk, wpk[w]);
        if (pk > 0.f) atomicMax(&p.out->pk, __float_as_uint(pk));
    }
}

// The pair measure of the stereo mix stage's bed (fishtts_hip.h: "Stereo mix"), behind level_filter_kernel over the two sides
// as two items of n samples each, nh hops each, back to back in x, hops and peaks:
//   level_pair_kernel        e_h = e_h(side 0) + e_h(side 1), one float64 addition per hop, and the larger of the two hop
//                            peaks, left in side 0's hops; level_gain_kernel then runs over them as over one item of n samples
//   level_pair_scale_kernel  both sides times that one gain: item 0 of the table, 2 n samples from its x on
static __global__ __launch_bounds__(LV_SCALE_THREADS) void level_pair_kernel(double* hops, float* peaks, long long nh) {
    for (long long h = (long long)blockIdx.x * LV_SCALE_THREADS + threadIdx.x; h < nh; h += (long long)gridDim.x * LV_SCALE_THREADS) {
        hops[h] = hops[h] + hops[nh + h];
        peaks[h] = fmaxf(peaks[h], peaks[nh + h]);
    }
}

static __global__ __launch_bounds__(LV_SCALE_THREADS) void level_pair_scale_kernel(const LevelTab* tab) {
    const LevelItem& it = tab->it[0];
    const float g = it.g;
    float* x = it.x;
    for (long long i = (long long)blockIdx.x * LV_SCALE_THREADS + threadIdx.x; i < 2 * it.n; i += (long long)gridDim.x * LV_SCALE_THREADS)
        x[i] = g * x[i];
}

}  // namespace ft
