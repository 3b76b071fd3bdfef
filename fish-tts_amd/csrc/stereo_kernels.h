// The stereo mix stage's kernels (ft_codec_mix_stereo; stated in fishtts_hip.h under "Stereo mix"): mix_stereo_kernel and the
// two kernels of the pair level.  They build on stage_kernels.h - MixP, mix_prog, mix_sample, the level table - and are
// included behind it by codec.hip alone: engine.hip includes stage_kernels.h, so a kernel added there lands in the AR
// engine's code object as well and moves its kernels (measured: 0.7 % of bench.py's tokens per second; DESIGN section 8,
// "Stereo" and "Kernel headers").
#pragma once
#include "stage_kernels.h"

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

// ---- live stereo mix stage (ft_codec_mix_live_stereo, ft_codec_mix_stream_*_stereo; stated in fishtts_hip.h under "Live stereo
// mix"): the live mix stage with two channels out.  The programme and its carry stay mono and mixl_hop_kernel,
// mixl_node_kernel and mixl_limit_kernel run as they are over MixLiveSP::l; the staged m, the m carries and the output hold
// two floats per frame, so a group of four frames is 32 bytes and begins on a 32-byte boundary where it begins at a multiple of
// four.  Every programme sample has a pan byte (pan + 100) beside it: the push's bytes in qx, laid out like the push (by xb),
// the carried ones in qin / qout, laid out like the programme carry (by pib / pob), so a sample keeps its pan wherever the
// pushes were cut.  Six launches per push whatever its size and its R, a launch with nothing to do left out; three are new:
//   mixls_pan_kernel     one lane per 16 samples of the push from xb on: one binary search of the push's regions for the first
//                        of them, a walk over the rest, one 16-byte store (mix_stereo_kernel's expansion, into global memory)
//   mixls_sample_kernel  mixl_sample_kernel per hop with the pans: four frames per lane, 16-byte loads of the programme and
//                        of either side (the bed read once where both sides are one buffer), one 4-byte load of the pans
//                        where the group lies in one buffer, two 16-byte stores of m (left, right, left, right), Q_h over
//                        both channels reduced in the workgroup, need_h by lane 0; U in LDS
//   mixls_apply_kernel   y over [out0, out1), two frames per lane and one 16-byte store each, then the m carry, the programme
//                        carry and the pan carry rolled
struct MixLiveSP {
    MixLiveP l;                // as the live mix stage fills it; l.m.bed is side 0 (without a bed nb = 0 and loop = 0), l.m.y the
                               // m of hops [q0, q1), l.cin, l.cout and l.y with two floats per frame
    const float* bed1;         // side 1 (l.m.bed itself where both sides are one)
    const float* U;            // [MS_PANS]
    const MixPan* reg;         // [R]: the push's regions, relative to the push
    unsigned char* qx;         // pan bytes of the push: timeline [F0, F1) from xb on
    const unsigned char* qin;  // pan carry read: [cb0, F0) from pib on
    unsigned char* qout;       // pan carry written: [cb1, F1) from pob on
    int R, words;              // 16-byte words of qx
};

// pan + 100 of timeline sample i: mixl_prog's selection over the two byte buffers, the centre outside [cb0, F1).
__device__ inline unsigned int mixls_pan(const MixLiveSP& sp, int i) {
    const MixLiveP& p = sp.l;
    const bool old = i < p.F0;
    const unsigned char* src = old ? sp.qin : sp.qx;
    const int lo = old ? p.cb0 : p.F0, hi = old ? p.F0 : p.F1, ab = old ? p.pib : p.xb;
    const int ic = min(max(i, lo), max(hi - 1, lo));
    const unsigned int v = src[ic - ab];
    return i >= lo && i < hi ? v : (unsigned int)MS_CENTRE;
}

// (m_0, m_1)[i] for i in [out0, mend1): the carry below q0 H, the push's hops from there.
__device__ inline float2 mixls_m(const MixLiveP& p, int i, int mend0) {
    const bool old = i < mend0;
    const float* src = old ? p.cin : p.m.y;
    const int lo = old ? p.out0 : mend0, hi = old ? mend0 : p.mend1, ab = old ? p.cib : p.mb;
    const int ic = min(max(i, lo), max(hi - 1, lo));
    return *(const float2*)(src + 2 * (size_t)(ic - ab));
}

static __global__ __launch_bounds__(MX_THREADS) void mixls_pan_kernel(MixLiveSP sp) {
    const int w = blockIdx.x * MX_THREADS + threadIdx.x;
    if (w >= sp.words) return;
    const int n = sp.l.F1 - sp.l.F0, j0 = 16 * w - (sp.l.F0 - sp.l.xb);    // the word's first sample, relative to the push
    int c = 0, b = sp.R;                                   // the first region that ends behind j0
    while (c < b) {
        const int mid = (c + b) >> 1;
        if (sp.reg[mid].e > (long long)j0) b = mid; else c = mid + 1;
    }
    long long ga = 0, ge = 0;
    unsigned int gq = MS_CENTRE;
    if (c < sp.R) { const MixPan g = sp.reg[c]; ga = g.a; ge = g.e; gq = (unsigned int)(g.pan + MS_CENTRE); }
    unsigned int v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int j = j0 + k;
        if (c < sp.R && (long long)j >= ge) {              // (regions hold a sample each: one step reaches the next)
            ++c;
            if (c < sp.R) { const MixPan g = sp.reg[c]; ga = g.a; ge = g.e; gq = (unsigned int)(g.pan + MS_CENTRE); }
        }
        const unsigned int q = c < sp.R && j >= 0 && j < n && (long long)j >= ga && (long long)j < ge ? gq : (unsigned int)MS_CENTRE;
        v[k >> 2] |= q << (8 * (k & 3));
    }
    ((uint4*)sp.qx)[w] = make_uint4(v[0], v[1], v[2], v[3]);
}

static __global__ __launch_bounds__(MX_THREADS) void mixls_sample_kernel(MixLiveSP sp) {
    const MixLiveP& p = sp.l;
    __shared__ float wpk[MX_THREADS / 64];
    __shared__ float U[MS_PANS];
    for (int j = threadIdx.x; j < MS_PANS; j += MX_THREADS) U[j] = sp.U[j];
    __syncthreads();
    const int h = p.q0 + blockIdx.x, i0 = h * p.m.H, i1 = min(i0 + p.m.H, p.Nend);
    const int i = (i0 & ~3) + 4 * (int)threadIdx.x;       // this lane's group: [i, i + 4), cut to the hop
    const bool one = sp.bed1 == p.m.bed;
    float pk = 0.f;
    if (i < i1) {
        const bool whole = i >= i0 && i + 3 < i1;
        float4 s, t0, t1;
        unsigned int pq;
        if (whole && i >= p.F0 && i + 3 < p.F1) {
            s = *(const float4*)(p.m.x + (i - p.xb));
            pq = *(const unsigned int*)(sp.qx + (i - p.xb));
        } else if (whole && i >= p.cb0 && i + 3 < p.F0) {
            s = *(const float4*)(p.pin + (i - p.pib));
            pq = *(const unsigned int*)(sp.qin + (i - p.pib));
        } else {
            s = make_float4(mixl_prog(p, i), mixl_prog(p, i + 1), mixl_prog(p, i + 2), mixl_prog(p, i + 3));
            pq = mixls_pan(sp, i) | mixls_pan(sp, i + 1) << 8 | mixls_pan(sp, i + 2) << 16 | mixls_pan(sp, i + 3) << 24;
        }
        long long j = (long long)i + p.m.off;
        if (p.m.loop) j %= p.m.nb;
        const bool wide = (j & 3) == 0 && j + 3 < p.m.nb;
        if (wide) t0 = *(const float4*)(p.m.bed + j);
        else t0 = make_float4(mix_side(p.m, p.m.bed, j), mix_side(p.m, p.m.bed, j + 1), mix_side(p.m, p.m.bed, j + 2), mix_side(p.m, p.m.bed, j + 3));
        if (one) t1 = t0;
        else if (wide) t1 = *(const float4*)(sp.bed1 + j);
        else t1 = make_float4(mix_side(p.m, sp.bed1, j), mix_side(p.m, sp.bed1, j + 1), mix_side(p.m, sp.bed1, j + 2), mix_side(p.m, sp.bed1, j + 3));
        const unsigned int q0 = pq & 255u, q1 = pq >> 8 & 255u, q2 = pq >> 16 & 255u, q3 = pq >> 24;
        float* dst = p.m.y + 2 * (size_t)(i - p.mb);
        if (whole) {
            float4 m0, m1;                                 // frames i, i + 1 and i + 2, i + 3: left, right, left, right
            m0.x = mix_sample(p.m, i, __fmul_rn(s.x, U[2 * MS_CENTRE - q0]), t0.x);
            m0.y = mix_sample(p.m, i, __fmul_rn(s.x, U[q0]), t1.x);
            m0.z = mix_sample(p.m, i + 1, __fmul_rn(s.y, U[2 * MS_CENTRE - q1]), t0.y);
            m0.w = mix_sample(p.m, i + 1, __fmul_rn(s.y, U[q1]), t1.y);
            m1.x = mix_sample(p.m, i + 2, __fmul_rn(s.z, U[2 * MS_CENTRE - q2]), t0.z);
            m1.y = mix_sample(p.m, i + 2, __fmul_rn(s.z, U[q2]), t1.z);
            m1.z = mix_sample(p.m, i + 3, __fmul_rn(s.w, U[2 * MS_CENTRE - q3]), t0.w);
            m1.w = mix_sample(p.m, i + 3, __fmul_rn(s.w, U[q3]), t1.w);
            ((float4*)dst)[0] = m0;
            ((float4*)dst)[1] = m1;
            pk = fmaxf(fmaxf(fmaxf(fabsf(m0.x), fabsf(m0.y)), fmaxf(fabsf(m0.z), fabsf(m0.w))),
                       fmaxf(fmaxf(fabsf(m1.x), fabsf(m1.y)), fmaxf(fabsf(m1.z), fabsf(m1.w))));   // (fmaxf passes a NaN by)
            pk = fmaxf(pk, 0.f);
        } else {                                           // the hop's first and last group: the frames inside it
            const float sv[4] = {s.x, s.y, s.z, s.w}, av[4] = {t0.x, t0.y, t0.z, t0.w}, bv[4] = {t1.x, t1.y, t1.z, t1.w};
            const unsigned int qv[4] = {q0, q1, q2, q3};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (i + c >= i0 && i + c < i1) {
                    const float l = mix_sample(p.m, i + c, __fmul_rn(sv[c], U[2 * MS_CENTRE - qv[c]]), av[c]);
                    const float r = mix_sample(p.m, i + c, __fmul_rn(sv[c], U[qv[c]]), bv[c]);
                    *(float2*)(dst + 2 * c) = make_float2(l, r);
                    pk = fmaxf(pk, fmaxf(fabsf(l), fabsf(r)));
                }
        }
    }
    for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o));
    if ((threadIdx.x & 63) == 0) wpk[threadIdx.x >> 6] = pk;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MX_THREADS / 64; ++w) pk = fmaxf(pk, wpk[w]);
        // need_h as mixl_sample_kernel finds it, from the peak of both channels
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

static __global__ __launch_bounds__(MX_THREADS) void mixls_apply_kernel(MixLiveSP sp) {
    const MixLiveP& p = sp.l;
    const int step = gridDim.x * MX_THREADS, t = blockIdx.x * MX_THREADS + threadIdx.x, H = p.m.H, mend0 = p.q0 * H;
    const float Hf = (float)H;
    for (int i = p.out0 + 2 * t; i < p.out1; i += 2 * step) {              // frames i and i + 1: 16 bytes of y
        float f[2];
        float2 m[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int ii = min(i + c, p.out1 - 1), k = (int)((unsigned int)ii / (unsigned int)H);
            const float lk = p.m.T[p.L[k]], r = __fdiv_rn((float)(ii - k * H), Hf);
            f[c] = fmaf(r, p.m.T[p.L[k + 1]] - lk, lk);
            m[c] = mixls_m(p, ii, mend0);
        }
        float* dst = p.y + 2 * (size_t)(i - p.out0);
        const float2 a = make_float2(__fmul_rn(m[0].x, f[0]), __fmul_rn(m[0].y, f[0]));
        if (i + 1 < p.out1) *(float4*)dst = make_float4(a.x, a.y, __fmul_rn(m[1].x, f[1]), __fmul_rn(m[1].y, f[1]));
        else *(float2*)dst = a;
    }
    for (int i = p.out1 + t; i < p.mend1; i += step) *(float2*)(p.cout + 2 * (size_t)(i - p.cob)) = mixls_m(p, i, mend0);
    for (int i = p.cb1 + t; i < p.F1; i += step) {
        p.pout[i - p.pob] = mixl_prog(p, i);
        sp.qout[i - p.pob] = (unsigned char)mixls_pan(sp, i);
    }
}

}  // namespace ft
