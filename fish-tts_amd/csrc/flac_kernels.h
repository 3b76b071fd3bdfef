// The FLAC stage's kernels (fishtts_hip.h, "FLAC"; the host side of the stage is flac_plan.h, whose constexpr functions write
// the header bytes and CRC entries here as well).  Integer arithmetic only behind the one float32 product of the quantiser;
// integer atomics only (sums, ORs and XORs commute), so the stream does not depend on the order the lanes arrive in.
//   flac_analyse_kernel  one workgroup per (frame, signal): the exhaustive cost search -> one FlSig
//   flac_pack_kernel     one workgroup per frame: channel assignment, header, subframes, CRCs -> a worst-case-stride slot
//   flac_scan_kernel     one workgroup: exclusive scan over the frame lengths, min / max, the 42 stream-head bytes
//   flac_gather_kernel   one workgroup per frame: the slot to its place in the compact stream
// and the live FLAC stage's ("Live FLAC"), in front of those four on a stream's push:
//   flacl_stage_kernel   carry || push, quantised, to the int16 staging buffer; what no frame takes to the other carry copy
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flac_plan.h"

namespace ft {

constexpr int FL_THREADS = 256, FL_SCAN_THREADS = 1024;
constexpr int FL_NK = flac::FL_MAX_K + 1;                                  // k = 0 .. 14
constexpr int FL_FINE = 1 << flac::FL_MAX_P;                                // the most partitions
constexpr int FL_IMG_WORDS = (int)((flac::fl_frame_bound(flac::FL_MAX_B, 2) + 3) / 4) + 2;   // the largest frame, and slack for fl_put's pair

struct FlSig {                       // the decision for one signal of one frame
    unsigned int bits;               // the subframe's bits
    unsigned char kind;              // 0 CONSTANT, 1 VERBATIM, 2 + o FIXED o
    unsigned char P;                 // partition order (FIXED)
    unsigned char pad[2];
    unsigned char k[FL_FINE];        // Rice parameter per partition (FIXED)
};

struct FlacOut {
    long long total;                 // bytes of the stream, head included
    int frames, fmin, fmax;
    int kinds[flac::FL_KINDS];
    int assignments[flac::FL_ASSIGNMENTS];
    int overflow;                    // frames whose bits did not fit the LDS image or the slot (the stated bound forbids it: the
                                     // host refuses the call's result with FT_ERR_STATE when it is not 0)
};

struct FlacP {
    const void* x;                   // n frames of `channels` interleaved samples: float32 (fmt 0) or int16 (fmt 1)
    long long n;
    int fmt, channels, B, rate, F, nsig;
    FlSig* sig;                      // [F][nsig]
    unsigned char* slots;            // [F][stride]
    int stride;                      // a multiple of 4, at least the frame bound
    int* flen;                       // [F]
    long long* foff;                 // [F]
    unsigned char* stream;           // at least ft_flac_bound bytes
    FlacOut* out;
    long long f0;                    // the number of frame 0 (a stream's push: the frames emitted before it)
};

// p = (int) trunc(min(1, max(-1, x)) 32767.0f), one float32 product; a NaN gives 0.  int16 as it is.
__device__ __forceinline__ int fl_sample(const FlacP& p, long long idx) {
    if (p.fmt) return (int)((const short*)p.x)[idx];
    const float v = ((const float*)p.x)[idx];
    if (v != v) return 0;
    const float c = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);
    return (int)(c * 32767.0f);
}

// Signal sg of a frame at sample i: mono 0; stereo 0 L, 1 R, 2 M = (L + R) >> 1, 3 S = L - R.
__device__ __forceinline__ int fl_signal(const FlacP& p, long long i, int sg) {
    if (p.channels == 1) return fl_sample(p, i);
    const int l = sg == 1 ? 0 : fl_sample(p, 2 * i), r = sg == 0 ? 0 : fl_sample(p, 2 * i + 1);
    return sg == 0 ? l : sg == 1 ? r : sg == 2 ? (l + r) >> 1 : l - r;
}

// e_o[i] from the samples (i >= o), then u = 2e for e >= 0, else -2e - 1.  |e_4| <= 16 * 65535: int is enough.
__device__ __forceinline__ unsigned int fl_fold(const int* s, int i, int o) {
    int e = s[i];
    if (o == 1) e = s[i] - s[i - 1];
    else if (o == 2) e = s[i] - 2 * s[i - 1] + s[i - 2];
    else if (o == 3) e = s[i] - 3 * s[i - 1] + 3 * s[i - 2] - s[i - 3];
    else if (o == 4) e = s[i] - 4 * s[i - 1] + 6 * s[i - 2] - 4 * s[i - 3] + s[i - 4];
    return e >= 0 ? 2u * (unsigned int)e : 2u * (unsigned int)(-e) - 1u;
}

__global__ __launch_bounds__(FL_THREADS) void flac_analyse_kernel(FlacP p) {
    __shared__ int s[flac::FL_MAX_B];
    __shared__ unsigned long long S[FL_FINE * FL_NK];     // sum of (u >> k) per finest partition, merged upward in place
    __shared__ unsigned long long tot[flac::FL_MAX_P + 1];
    __shared__ int differs;
    const int t = threadIdx.x, f = blockIdx.x, sg = blockIdx.y;
    const long long i0 = (long long)f * p.B;
    const int bs = (int)(p.n - i0 < p.B ? p.n - i0 : p.B);
    const int w = sg == 3 ? 17 : 16;
    if (t == 0) differs = 0;
    for (int i = t; i < bs; i += FL_THREADS) s[i] = fl_signal(p, i0 + i, sg);
    __syncthreads();
    bool d = false;
    for (int i = t; i < bs; i += FL_THREADS) d = d || s[i] != s[0];
    if (d) atomicOr(&differs, 1);
    __syncthreads();

    const int tz = __builtin_ctz((unsigned int)bs), Pf = tz < flac::FL_MAX_P ? tz : flac::FL_MAX_P;
    const int np = 1 << Pf, lenf = bs >> Pf, per = FL_THREADS / np;      // `per` threads share a finest partition
    const int myj = t / per, mysub = t % per;

    // candidates in tie order: CONSTANT, FIXED by ascending o, VERBATIM; a later one must be strictly cheaper
    unsigned long long best = differs ? ~0ULL : (unsigned long long)(8 + w);
    int kind = 0, bestP = 0;
    unsigned char bestk = 0;
    for (int o = 0; o <= flac::FL_MAX_ORDER && o < bs; ++o) {
        for (int i = t; i < np * FL_NK; i += FL_THREADS) S[i] = 0;
        if (t <= flac::FL_MAX_P) tot[t] = 0;
        __syncthreads();
        unsigned int acc[FL_NK];
#pragma unroll
        for (int k = 0; k < FL_NK; ++k) acc[k] = 0;
        for (int q = mysub; q < lenf; q += per) {                        // at most 16 samples a thread: acc < 2^27
            const int i = myj * lenf + q;
            if (i < o) continue;                                         // the warm-up samples carry no residual
            const unsigned int u = fl_fold(s, i, o);
#pragma unroll
            for (int k = 0; k < FL_NK; ++k) acc[k] += u >> k;
        }
#pragma unroll
        for (int k = 0; k < FL_NK; ++k) atomicAdd(&S[myj * FL_NK + k], (unsigned long long)acc[k]);
        __syncthreads();
        unsigned long long obest = ~0ULL;
        int oP = 0;
        unsigned char ok = 0;
        for (int P = Pf; P >= 0; --P) {                                  // partition j of level P lies at j << (Pf - P)
            const int sh = Pf - P, count = 1 << P;
            const bool allowed = (bs >> P) > o;
            unsigned char myk = 0;
            if (allowed && t < count) {
                const unsigned long long m = (unsigned long long)((bs >> P) - (t == 0 ? o : 0));
                const unsigned long long* row = &S[(t << sh) * FL_NK];
                unsigned long long c = row[0] + m;
                for (int k = 1; k < FL_NK; ++k) {
                    const unsigned long long ck = row[k] + m * (unsigned long long)(k + 1);
                    if (ck < c) { c = ck; myk = (unsigned char)k; }      // ties to the smaller k
                }
                atomicAdd(&tot[P], c + 4);
            }
            __syncthreads();
            if (allowed && tot[P] <= obest) {                            // descending P: ties to the smaller P
                obest = tot[P];
                oP = P;
                ok = myk;
            }
            if (P > 0)
                for (int i = t; i < (count >> 1) * FL_NK; i += FL_THREADS) {
                    const int j = i / FL_NK, k = i % FL_NK;
                    S[((2 * j) << sh) * FL_NK + k] += S[((2 * j + 1) << sh) * FL_NK + k];
                }
            __syncthreads();
        }
        const unsigned long long bits = (unsigned long long)(8 + w * o + 6) + obest;
        if (bits < best) {
            best = bits;
            kind = 2 + o;
            bestP = oP;
            bestk = ok;
        }
    }
    const unsigned long long verbatim = 8ULL + (unsigned long long)w * (unsigned long long)bs;
    if (verbatim < best) {
        best = verbatim;
        kind = 1;
    }
    FlSig* out = &p.sig[(size_t)f * p.nsig + sg];
    if (t == 0) {
        out->bits = (unsigned int)best;
        out->kind = (unsigned char)kind;
        out->P = (unsigned char)(kind >= 2 ? bestP : 0);
        out->pad[0] = out->pad[1] = 0;
    }
    out->k[t] = kind >= 2 && t < (1 << bestP) ? bestk : (unsigned char)0;
}

// v (< 2^nb, nb in 1..32) at bit `bit` of an image whose words hold the stream's bits first-bit-highest.  The image starts
// zeroed, so ORs place a field whatever shares its words; a write past the image is dropped and marked in *over.
__device__ __forceinline__ void fl_put(unsigned int* img, int* over, unsigned int bit, int nb, unsigned int v) {
    const unsigned int wd = bit >> 5;
    const int room = 32 - (int)(bit & 31);
    if (wd + 1 >= (unsigned int)FL_IMG_WORDS) {
        *over = 1;
        return;
    }
    if (nb <= room) atomicOr(&img[wd], v << (room - nb));
    else {
        atomicOr(&img[wd], v >> (nb - room));
        atomicOr(&img[wd + 1], v << (32 - (nb - room)));
    }
}
__device__ __forceinline__ unsigned int fl_byte(const unsigned int* img, int b) { return (img[b >> 2] >> (24 - 8 * (b & 3))) & 0xFF; }

__global__ __launch_bounds__(FL_THREADS) void flac_pack_kernel(FlacP p) {
    __shared__ unsigned int img[FL_IMG_WORDS];
    __shared__ int s[flac::FL_MAX_B];
    __shared__ unsigned int ue[flac::FL_MAX_B];
    __shared__ unsigned int sc[FL_THREADS];
    __shared__ unsigned short tab[256];
    __shared__ unsigned char kk[FL_FINE];
    __shared__ unsigned char hdr[16];
    __shared__ int hlen, assignment, crc, over;
    const int t = threadIdx.x, f = blockIdx.x;
    const long long i0 = (long long)f * p.B;
    const int bs = (int)(p.n - i0 < p.B ? p.n - i0 : p.B);
    const FlSig* dec = &p.sig[(size_t)f * p.nsig];
    for (int i = t; i < FL_IMG_WORDS; i += FL_THREADS) img[i] = 0;
    tab[t] = flac::fl_crc16_entry(t);
    if (t == 0) {
        int a = 0;
        if (p.channels == 2) {                                           // 0001, 1000, 1001, 1010: ties go in that order
            const unsigned int lr = dec[0].bits + dec[1].bits, ls = dec[0].bits + dec[3].bits, sr = dec[3].bits + dec[1].bits,
                               ms = dec[2].bits + dec[3].bits;
            unsigned int m = lr;
            a = 1;
            if (ls < m) { m = ls; a = 8; }
            if (sr < m) { m = sr; a = 9; }
            if (ms < m) { m = ms; a = 10; }
        }
        assignment = a;
        crc = 0;
        over = 0;
        unsigned char h[flac::FL_HEADER_MAX];
        hlen = flac::fl_frame_header(h, bs, p.B, p.rate, a, (uint32_t)(p.f0 + f));
        for (int i = 0; i < hlen; ++i) hdr[i] = h[i];
    }
    __syncthreads();
    if (t < hlen) fl_put(img, &over, 8u * t, 8, hdr[t]);
    const int a = assignment;
    const int first = a == 9 ? 3 : a == 10 ? 2 : 0, second = a == 1 || a == 9 ? 1 : 3;
    unsigned int bit = 8u * hlen;
    for (int c = 0; c < p.channels; ++c) {
        const int sg = c == 0 ? first : second, w = sg == 3 ? 17 : 16;
        const FlSig* d = &dec[sg];
        const int kind = d->kind, o = kind >= 2 ? kind - 2 : 0, P = d->P;
        const unsigned int mask = (1u << w) - 1;
        __syncthreads();                                                 // the previous channel's s, ue, kk and sc are done with
        for (int i = t; i < bs; i += FL_THREADS) s[i] = fl_signal(p, i0 + i, sg);
        kk[t] = d->k[t];
        if (t == 0) {
            fl_put(img, &over, bit, 8, kind == 0 ? 0u : kind == 1 ? 2u : (unsigned int)((8 | o) << 1));
            atomicAdd(&p.out->kinds[kind], 1);
        }
        __syncthreads();
        if (kind == 0) {
            if (t == 0) fl_put(img, &over, bit + 8, w, (unsigned int)s[0] & mask);
        } else if (kind == 1) {
            for (int i = t; i < bs; i += FL_THREADS) fl_put(img, &over, bit + 8 + (unsigned int)i * w, w, (unsigned int)s[i] & mask);
        } else {
            if (t < o) fl_put(img, &over, bit + 8 + (unsigned int)t * w, w, (unsigned int)s[t] & mask);
            if (t == 0) fl_put(img, &over, bit + 8 + (unsigned int)o * w, 6, (unsigned int)P);        // method 00, then the order
            for (int i = t; i < bs; i += FL_THREADS) ue[i] = i < o ? 0u : fl_fold(s, i, o);
            __syncthreads();
            // a thread owns `chunk` consecutive samples: their code lengths, a scan over the threads, then the codes
            const int lenP = bs >> P, chunk = (bs + FL_THREADS - 1) / FL_THREADS;
            const int ia = t * chunk < bs ? t * chunk : bs, ie = ia + chunk < bs ? ia + chunk : bs;
            unsigned int mine = 0;
            for (int i = ia < o ? o : ia; i < ie; ++i) {
                const int part = i / lenP, k = kk[part];
                mine += (ue[i] >> k) + 1 + k + (i == (part == 0 ? o : part * lenP) ? 4 : 0);
            }
            sc[t] = mine;
            __syncthreads();
            for (int step = 1; step < FL_THREADS; step <<= 1) {          // inclusive scan over the threads' sums
                const unsigned int add = t >= step ? sc[t - step] : 0;
                __syncthreads();
                sc[t] += add;
                __syncthreads();
            }
            unsigned int at = bit + 8 + (unsigned int)o * w + 6 + sc[t] - mine;
            for (int i = ia < o ? o : ia; i < ie; ++i) {
                const int part = i / lenP, k = kk[part];
                if (i == (part == 0 ? o : part * lenP)) {
                    fl_put(img, &over, at, 4, (unsigned int)k);
                    at += 4;
                }
                const unsigned int u = ue[i], q = u >> k;                // q zeros are there already: the stop bit and k low bits
                fl_put(img, &over, at + q, 1 + k, (1u << k) | (u & ((1u << k) - 1)));
                at += q + 1 + k;
            }
        }
        bit += d->bits;
    }
    __syncthreads();
    // zero bits to the byte, then CRC-16 over the frame: each thread its run of bytes, joined by the CRC's linearity
    int nb = (int)((bit + 7) >> 3);
    const int limit = p.stride - 2 < (FL_IMG_WORDS - 2) * 4 ? p.stride - 2 : (FL_IMG_WORDS - 2) * 4;
    if (nb > limit) {                                                    // (the cheapest candidates are below the bound)
        nb = limit;
        if (t == 0) over = 1;
    }
    {
        const int chunk = (nb + FL_THREADS - 1) / FL_THREADS;
        const int ba = t * chunk < nb ? t * chunk : nb, be = ba + chunk < nb ? ba + chunk : nb;
        if (be > ba) {
            unsigned int c = 0;
            for (int b = ba; b < be; ++b) c = ((c << 8) & 0xFFFF) ^ tab[((c >> 8) ^ fl_byte(img, b)) & 0xFF];
            atomicXor(&crc, (int)flac::fl_crc16_shift((uint16_t)c, nb - be));
        }
    }
    __syncthreads();
    if (t == 0) {
        fl_put(img, &over, 8u * nb, 16, (unsigned int)crc & 0xFFFF);
        p.flen[f] = nb + 2;
        if (over) atomicAdd(&p.out->overflow, 1);
        atomicAdd(&p.out->assignments[a == 0 ? 0 : a == 1 ? 1 : a - 6], 1);
    }
    __syncthreads();
    unsigned int* slot = (unsigned int*)(p.slots + (size_t)f * p.stride);
    for (int i = t; i < (nb + 2 + 3) / 4; i += FL_THREADS) slot[i] = __builtin_bswap32(img[i]);
}

__global__ __launch_bounds__(FL_SCAN_THREADS) void flac_scan_kernel(FlacP p) {
    __shared__ long long sums[FL_SCAN_THREADS];
    __shared__ int fmin, fmax;
    const int t = threadIdx.x;
    const int chunk = (p.F + FL_SCAN_THREADS - 1) / FL_SCAN_THREADS;
    const int fa = (long long)t * chunk < p.F ? t * chunk : p.F, fe = fa + chunk < p.F ? fa + chunk : p.F;
    if (t == 0) {
        fmin = 0x7FFFFFFF;
        fmax = 0;
    }
    __syncthreads();
    long long mine = 0;
    int lo = 0x7FFFFFFF, hi = 0;
    for (int f = fa; f < fe; ++f) {
        const int v = p.flen[f];
        mine += v;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    sums[t] = mine;
    if (fe > fa) {
        atomicMin(&fmin, lo);
        atomicMax(&fmax, hi);
    }
    __syncthreads();
    for (int step = 1; step < FL_SCAN_THREADS; step <<= 1) {
        const long long add = t >= step ? sums[t - step] : 0;
        __syncthreads();
        sums[t] += add;
        __syncthreads();
    }
    long long at = sums[t] - mine;
    for (int f = fa; f < fe; ++f) {
        p.foff[f] = at;
        at += p.flen[f];
    }
    if (t == 0) {
        p.out->total = flac::FL_STREAM_HEAD + sums[FL_SCAN_THREADS - 1];
        p.out->frames = p.F;
        p.out->fmin = fmin;
        p.out->fmax = fmax;
        unsigned char head[flac::FL_STREAM_HEAD];
        flac::fl_stream_head(head, p.B, fmin, fmax, p.rate, p.channels, p.n);
        for (int i = 0; i < flac::FL_STREAM_HEAD; ++i) p.stream[i] = head[i];
    }
}

// A frame's bytes from its (4-byte aligned) slot to the compact stream: bytes up to the destination's next word, whole
// words put together from two of the slot's, bytes at the end.
__global__ __launch_bounds__(FL_THREADS) void flac_gather_kernel(FlacP p) {
    const int t = threadIdx.x, f = blockIdx.x, len = p.flen[f];
    const unsigned char* src = p.slots + (size_t)f * p.stride;
    unsigned char* dst = p.stream + flac::FL_STREAM_HEAD + p.foff[f];
    int head = (int)((4 - ((uintptr_t)dst & 3)) & 3);
    head = head < len ? head : len;
    const int words = (len - head) >> 2, tail = head + 4 * words;
    if (t < head) dst[t] = src[t];
    const unsigned int* s32 = (const unsigned int*)src;
    unsigned int* d32 = (unsigned int*)(dst + head);
    const int sh = 8 * head;                                             // the source runs `head` bytes ahead of a word
    for (int i = t; i < words; i += FL_THREADS) d32[i] = sh ? (s32[i] >> sh) | (s32[i + 1] << (32 - sh)) : s32[i];
    if (t < len - tail) dst[tail + t] = src[tail + t];
}

// ---- live FLAC stage: one launch over the T frames of carry || push, in int16 elements (T * channels of them).
struct FlacStageP {
    const short* carry_in;           // r frames, interleaved (the copy the push reads)
    short* carry_out;                // the other copy: the frames from `taken` on
    short* stage;                    // [T * channels], on an 8-byte boundary
    FlacP push;                      // x, fmt of the push's samples (fl_sample's arguments)
    long long r, T, taken;           // frames: the carry found, carry + push, those the emitted frames hold
};

// A thread owns four consecutive elements of the staging buffer, which begin at a multiple of four: each is read on its own
// (a 16-bit load from the carry, or fl_sample of the push - so any r and any T are served alike), the four go out in one
// 8-byte store where all four exist, and an element past `taken` goes to the other carry copy in a 16-bit store.
__global__ __launch_bounds__(FL_THREADS) void flacl_stage_kernel(FlacStageP q) {
    const long long E = q.T * q.push.channels, re = q.r * q.push.channels, te = q.taken * q.push.channels;
    const long long groups = (E + 3) >> 2;
    for (long long g = (long long)blockIdx.x * FL_THREADS + threadIdx.x; g < groups; g += (long long)gridDim.x * FL_THREADS) {
        const long long j0 = g << 2;
        short v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long j = j0 + u;
            v[u] = j >= E ? (short)0 : j < re ? q.carry_in[j] : (short)fl_sample(q.push, j - re);
            if (j < E && j >= te) q.carry_out[j - te] = v[u];
        }
        if (j0 + 4 <= E) {
            const uint2 w = {(unsigned int)(unsigned short)v[0] | ((unsigned int)(unsigned short)v[1] << 16),
                             (unsigned int)(unsigned short)v[2] | ((unsigned int)(unsigned short)v[3] << 16)};
            *(uint2*)(q.stage + j0) = w;
        } else {
            for (int u = 0; u < 4 && j0 + u < E; ++u) q.stage[j0 + u] = v[u];
        }
    }
}

}  // namespace ft
