// Host arithmetic of the FLAC stage (fishtts_hip.h, "FLAC"): the argument checks in their stated order, the frame count and the
// last frame's size, the frame header and STREAMINFO bytes, the format's number coding, both CRCs (entry by entry, so that a
// table is 256 calls) and the rule that joins the CRC-16 of two byte runs, and ft_flac_bound.  Plain C++ without HIP, so that a
// host program can drive it under a sanitizer (tools/flac_check.cpp).  Every function that writes stream bytes is constexpr: the
// kernels of flac_kernels.h call the same code, so the bytes the host program checks are the bytes the device writes.
#pragma once
#include <stdint.h>

#include "fx_chain.h"

namespace ft {
namespace flac {

constexpr long long FL_MAX_N = 1LL << 28;
constexpr int FL_MAX_K = 14, FL_MAX_P = 8, FL_MAX_ORDER = 4, FL_MAX_B = 4096;
constexpr int FL_STREAM_HEAD = 42;                       // fLaC, the block header, STREAMINFO
constexpr int FL_HEADER_MAX = 15;                        // 4 + a 6-byte number + 2 + 2 + CRC-8
constexpr int FL_KINDS = 7, FL_ASSIGNMENTS = 5;          // CONSTANT, VERBATIM, FIXED 0..4; 0000, 0001, 1000, 1001, 1010

// 1000..1100 for 256..4096; -1 for any other blocksize.
constexpr int fl_block_code(int B) {
    for (int c = 0; c < 5; ++c)
        if (B == 256 << c) return 8 + c;
    return -1;
}

constexpr long long fl_frames(long long n, int B) { return (n + B - 1) / B; }
constexpr int fl_last(long long n, int B) { return (int)(n - (fl_frames(n, B) - 1) * B); }

// The most bytes a frame of bs samples takes: the longest header, every subframe VERBATIM at 16 bits, CRC-16.
constexpr long long fl_frame_bound(int bs, int channels) { return FL_HEADER_MAX + (long long)channels * (1 + 2LL * bs) + 2; }

// ft_flac_bound: the all-VERBATIM stream with the longest frame headers; -1 for arguments the stage refuses.
constexpr long long fl_bound(long long n, int channels, int B) {
    if (n < 1 || n > FL_MAX_N || (channels != 1 && channels != 2) || fl_block_code(B) < 0) return -1;
    const long long F = fl_frames(n, B);
    return FL_STREAM_HEAD + F * (FL_HEADER_MAX + 2) + channels * (F + 2 * n);
}

struct FlArgs {
    int fmt = 0, channels = 1, rate = 44100, blocksize = 4096, reserved = 0;
    long long n = 0, capacity = 0;
};

// The checks behind the null pointers, in the stated order; null when the call stands.
inline const char* fl_check(const FlArgs& a, bool* too_long) {
    *too_long = false;
    if (a.fmt != 0 && a.fmt != 1) return "fmt is neither 0 (float32) nor 1 (int16)";
    if (a.channels != 1 && a.channels != 2) return "channels is neither 1 nor 2";
    int l = 1, m = 1, k = 0;
    if (const char* why = chain::rs_design(a.rate, &l, &m, &k, nullptr)) return why;
    if (fl_block_code(a.blocksize) < 0) return "blocksize is not 256, 512, 1024, 2048 or 4096";
    if (a.reserved != 0) return "the reserved field is not 0";
    if (a.n < 1) return "n < 1";
    if (a.n > FL_MAX_N) {
        *too_long = true;
        return "more than 2^28 frames of samples";
    }
    if (a.capacity < fl_bound(a.n, a.channels, a.blocksize)) return "capacity below ft_flac_bound";
    return nullptr;
}

// ---- CRCs: CRC-8 (poly 0x07) and CRC-16 (poly 0x8005), both init 0, not reflected, no final xor.
constexpr uint8_t fl_crc8_entry(int b) {
    unsigned c = (unsigned)b;
    for (int i = 0; i < 8; ++i) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
    return (uint8_t)c;
}
constexpr uint16_t fl_crc16_entry(int b) {
    unsigned c = (unsigned)b << 8;
    for (int i = 0; i < 8; ++i) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
    return (uint16_t)c;
}
constexpr uint8_t fl_crc8(const uint8_t* p, int n) {
    uint8_t c = 0;
    for (int i = 0; i < n; ++i) c = fl_crc8_entry(c ^ p[i]);
    return c;
}
constexpr uint16_t fl_crc16_step(uint16_t c, uint8_t b) { return (uint16_t)((c << 8) ^ fl_crc16_entry((c >> 8) ^ b)); }
constexpr uint16_t fl_crc16(const uint8_t* p, long long n) {
    uint16_t c = 0;
    for (long long i = 0; i < n; ++i) c = fl_crc16_step(c, p[i]);
    return c;
}
// With init 0 the CRC is linear: crc(A || B) = crc(A) x^(8 |B|) mod G  xor  crc(B).  a b mod G, G = x^16 + 0x8005:
constexpr uint16_t fl_gf_mul(uint16_t a, uint16_t b) {
    unsigned r = 0;
    for (int i = 15; i >= 0; --i) {
        r = (r & 0x8000) ? ((r << 1) ^ 0x8005) & 0xFFFF : (r << 1) & 0xFFFF;
        if ((b >> i) & 1) r ^= a;
    }
    return (uint16_t)r;
}
// crc x^(8 bytes) mod G: the CRC of a run followed by `bytes` bytes that are accounted for elsewhere.
constexpr uint16_t fl_crc16_shift(uint16_t crc, long long bytes) {
    uint16_t pw = 1, sq = 2;                             // x^0, x^1
    for (unsigned long long e = 8ULL * (unsigned long long)bytes; e; e >>= 1) {
        if (e & 1) pw = fl_gf_mul(pw, sq);
        sq = fl_gf_mul(sq, sq);
    }
    return fl_gf_mul(crc, pw);
}

// ---- the format's UTF-8-style number coding (up to 31 bits here): bytes written.
constexpr int fl_number(uint32_t v, uint8_t* out) {
    if (v < 0x80) {
        out[0] = (uint8_t)v;
        return 1;
    }
    int n = 2;
    while (n < 6 && (v >> (5 * n + 1))) ++n;             // n bytes hold 5 n + 1 bits: 11, 16, 21, 26, 31
    out[0] = (uint8_t)(((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1))));
    for (int i = 1; i < n; ++i) out[i] = (uint8_t)(0x80 | ((v >> (6 * (n - 1 - i))) & 0x3F));
    return n;
}

// 0100..1010 for the rates of the format's table, else 1101 (the rate in Hz behind the header, 16 bits).
constexpr int fl_rate_code(int rate) {
    switch (rate) {
        case 8000: return 4;
        case 16000: return 5;
        case 22050: return 6;
        case 24000: return 7;
        case 32000: return 8;
        case 44100: return 9;
        case 48000: return 10;
        default: return 13;
    }
}

// A frame's header, CRC-8 included, into out[FL_HEADER_MAX]; bytes written.  bs is the frame's own size, B the stream's.
constexpr int fl_frame_header(uint8_t* out, int bs, int B, int rate, int assignment, uint32_t number) {
    const int bcode = bs == B ? fl_block_code(B) : bs <= 256 ? 6 : 7, rcode = fl_rate_code(rate);
    int at = 0;
    out[at++] = 0xFF;
    out[at++] = 0xF8;
    out[at++] = (uint8_t)((bcode << 4) | rcode);
    out[at++] = (uint8_t)((assignment << 4) | (4 << 1));
    at += fl_number(number, out + at);
    if (bcode == 7) out[at++] = (uint8_t)((bs - 1) >> 8);
    if (bcode == 6 || bcode == 7) out[at++] = (uint8_t)((bs - 1) & 0xFF);
    if (rcode == 13) {
        out[at++] = (uint8_t)(rate >> 8);
        out[at++] = (uint8_t)(rate & 0xFF);
    }
    out[at] = fl_crc8(out, at);
    return at + 1;
}

// fLaC, the last-block header of a 34-byte STREAMINFO, STREAMINFO with the MD5 field zero: out[FL_STREAM_HEAD].
constexpr void fl_stream_head(uint8_t* out, int B, int fmin, int fmax, int rate, int channels, long long n) {
    const uint8_t head[8] = {0x66, 0x4C, 0x61, 0x43, 0x80, 0x00, 0x00, 0x22};
    for (int i = 0; i < 8; ++i) out[i] = head[i];
    out[8] = out[10] = (uint8_t)(B >> 8);
    out[9] = out[11] = (uint8_t)(B & 0xFF);
    for (int i = 0; i < 3; ++i) {
        out[12 + i] = (uint8_t)(fmin >> (16 - 8 * i));
        out[15 + i] = (uint8_t)(fmax >> (16 - 8 * i));
    }
    const unsigned long long v = ((unsigned long long)rate << 44) | ((unsigned long long)(channels - 1) << 41) | (15ULL << 36) |
                                 (unsigned long long)n;
    for (int i = 0; i < 8; ++i) out[18 + i] = (uint8_t)(v >> (56 - 8 * i));
    for (int i = 26; i < FL_STREAM_HEAD; ++i) out[i] = 0;
}

// ---- the live FLAC stage (fishtts_hip.h, "Live FLAC"): what a push emits, and a stream's host state with its checks.
constexpr long long FL_MAX_TOTAL = (1LL << 36) - 1;     // STREAMINFO's sample count

// One push of n frames behind `before` frames already taken: the carry r it finds, the frames it emits, the samples of the last
// of them, the samples those frames hold, the carry it leaves, and the byte bound of its frames (fl_bound without the 42).
struct FlPush {
    long long r = 0, T = 0, F = 0, taken = 0, keep = 0, bytes = 0;
    int last = 0;
};
constexpr FlPush fl_push_plan(int B, int channels, long long before, long long n, bool final) {
    FlPush p;
    p.r = before % B;
    p.T = p.r + n;
    p.F = final ? fl_frames(p.T, B) : p.T / B;
    p.taken = final ? p.T : p.F * B;
    p.keep = p.T - p.taken;
    p.last = p.F == 0 ? 0 : (int)(p.taken - (p.F - 1) * B);
    p.bytes = p.F * (FL_HEADER_MAX + 2) + channels * (p.F + 2 * p.taken);
    return p;
}

// ft_flac_stream_plan's refusals: 0 fine, 1 a bad argument, 2 too long.
constexpr int fl_push_refused(int B, int channels, long long before, long long n) {
    if (fl_block_code(B) < 0 || (channels != 1 && channels != 2) || before < 0 || n < 0) return 1;
    if (n > FL_MAX_N || before > FL_MAX_TOTAL || before + n > FL_MAX_TOTAL) return 2;
    return 0;
}

struct FlStream {
    int fmt = 0, channels = 1, rate = 44100, B = 4096;
    long long n_in = 0, F_done = 0, bytes = 0;           // samples taken, frames emitted, their bytes (without the 42)
    int fmin = 0, fmax = 0;                              // over the frames so far; 0 before the first
    int kinds[FL_KINDS] = {}, assignments[FL_ASSIGNMENTS] = {};
    int par = 0;                                         // the carry copy the next push reads
    bool ended = false;

    long long carry() const { return ended ? 0 : n_in - F_done * B; }
    FlPush plan(long long n, bool final) const { return fl_push_plan(B, channels, n_in, n, final); }
    // The counters behind a push that went through: its frames' bytes, smallest and largest, and counts.
    void commit(const FlPush& p, long long n, bool final, long long got, int lo, int hi, const int* k, const int* a) {
        n_in += n;
        if (p.F > 0) {
            fmin = F_done == 0 || lo < fmin ? lo : fmin;
            fmax = hi > fmax ? hi : fmax;
        }
        F_done += p.F;
        bytes += got;
        for (int i = 0; i < FL_KINDS; ++i) kinds[i] += k[i];
        for (int i = 0; i < FL_ASSIGNMENTS; ++i) assignments[i] += a[i];
        par ^= 1;
        ended = final;
    }
    // The 42 leading bytes from what is known: before the final push the format's "unknown" zeros for the smallest and largest
    // frame and for n, after it the real values.
    void head(uint8_t* out) const {
        if (ended) fl_stream_head(out, B, fmin, fmax, rate, channels, n_in);
        else fl_stream_head(out, B, 0, 0, rate, channels, 0);
    }
};

// `begin`'s checks behind the null pointers: fl_check's, in its order, without n and the capacity.
inline const char* fl_stream_begin_check(int fmt, int channels, int rate, int blocksize, int reserved) {
    FlArgs a;
    a.fmt = fmt; a.channels = channels; a.rate = rate; a.blocksize = blocksize; a.reserved = reserved;
    a.n = 1; a.capacity = 1LL << 40;
    bool too_long = false;
    return fl_check(a, &too_long);
}

// A push's checks in the stated order; null when the push stands.  `null_pointer`: the stream, out or n_bytes is null.
inline const char* fl_stream_check(const FlStream* s, bool null_pointer, bool x_null, long long n, bool final, long long capacity,
                                   bool* state, bool* too_long) {
    *state = *too_long = false;
    if (!s || null_pointer) return "a null pointer";
    if (n < 0) return "n < 0";
    if (x_null && n > 0) return "x is null with n > 0";
    if (s->ended) {
        *state = true;
        return "a push after the final one";
    }
    if (n > FL_MAX_N) {
        *too_long = true;
        return "more than 2^28 frames of samples in one push";
    }
    if (s->n_in + n > FL_MAX_TOTAL) {
        *too_long = true;
        return "more than 2^36 - 1 frames of samples in the stream";
    }
    if (capacity < s->plan(n, final).bytes) return "capacity below ft_flac_stream_plan's bound";
    return nullptr;
}

}  // namespace flac
}  // namespace ft
