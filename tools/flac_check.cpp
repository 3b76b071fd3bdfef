// Host program that drives the FLAC stage's host arithmetic (fish-tts_amd/csrc/flac_plan.h: the argument checks in their
// stated order, F and the last frame's size, the frame header and STREAMINFO bytes, the number coding, both CRCs and the
// rule that joins the CRC-16 of byte runs, ft_flac_bound) so that a build with -fsanitize=address,undefined sees any read or
// write past an array and any overflow.  No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/flac_check.cpp -o flac_check
// The arrays the functions write into are sized exactly (a header's FL_HEADER_MAX, the stream head's FL_STREAM_HEAD), so a
// byte too many is an error the sanitizer reports.
// Exit status 0 and "flac_check: ok" when every expectation holds.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../fish-tts_amd/csrc/flac_plan.h"

using namespace ft::flac;

static int failures = 0;
static char where[160] = "";
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (failures < 20) fprintf(stderr, "%s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, where); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static void checks() {
    snprintf(where, sizeof where, "checks");
    bool tl = true;
    FlArgs ok;
    ok.n = 1000; ok.capacity = fl_bound(1000, 1, 4096);
    EXPECT(fl_check(ok, &tl) == nullptr && !tl);
    struct Bad { const char* word; void (*set)(FlArgs&); bool too_long; char field; };   // pairs that set one field are skipped
    const Bad BAD[] = {
        {"fmt", [](FlArgs& a) { a.fmt = 2; }, false, 0},
        {"channels", [](FlArgs& a) { a.channels = 3; }, false, 0},
        {"sample rate", [](FlArgs& a) { a.rate = 7999; }, false, 0},
        {"blocksize", [](FlArgs& a) { a.blocksize = 4095; }, false, 0},
        {"reserved", [](FlArgs& a) { a.reserved = 1; }, false, 0},
        {"n < 1", [](FlArgs& a) { a.n = 0; }, false, 'n'},
        {"2^28", [](FlArgs& a) { a.n = FL_MAX_N + 1; }, true, 'n'},
        {"capacity", [](FlArgs& a) { a.capacity -= 1; }, false, 0},
    };
    const int NB = (int)(sizeof BAD / sizeof BAD[0]);
    for (int i = 0; i < NB; ++i) {
        FlArgs a = ok;
        BAD[i].set(a);
        const char* why = fl_check(a, &tl);
        snprintf(where, sizeof where, "checks %s", BAD[i].word);
        EXPECT(why && strstr(why, BAD[i].word) && tl == BAD[i].too_long);
        for (int j = i + 1; j < NB; ++j) {                      // the earlier reason wins
            if (BAD[i].field && BAD[i].field == BAD[j].field) continue;
            FlArgs b = a;
            BAD[j].set(b);
            const char* both = fl_check(b, &tl);
            EXPECT(both && strstr(both, BAD[i].word));
        }
    }
    snprintf(where, sizeof where, "checks: limits");
    FlArgs a = ok;
    a.n = FL_MAX_N; a.channels = 2; a.blocksize = 256; a.fmt = 1; a.rate = 48000; a.capacity = fl_bound(a.n, 2, 256);
    EXPECT(fl_check(a, &tl) == nullptr && !tl);
    a.capacity = INT64_MAX; a.rate = 8000;
    EXPECT(fl_check(a, &tl) == nullptr);
    a.n = INT64_MAX;
    EXPECT(fl_check(a, &tl) != nullptr && tl);
    a.n = INT64_MIN;
    EXPECT(fl_check(a, &tl) != nullptr && !tl);
    for (int B : {0, -256, 128, 255, 257, 8192, 4097, INT32_MAX, INT32_MIN}) EXPECT(fl_block_code(B) == -1);
    for (int c = 0; c < 5; ++c) EXPECT(fl_block_code(256 << c) == 8 + c);
}

static void frames_and_bound() {
    snprintf(where, sizeof where, "frames");
    EXPECT(fl_frames(1, 256) == 1 && fl_last(1, 256) == 1);
    EXPECT(fl_frames(256, 256) == 1 && fl_last(256, 256) == 256);
    EXPECT(fl_frames(257, 256) == 2 && fl_last(257, 256) == 1);
    EXPECT(fl_frames(2 * 256 + 255, 256) == 3 && fl_last(2 * 256 + 255, 256) == 255);
    EXPECT(fl_frames(1024 + 700, 1024) == 2 && fl_last(1024 + 700, 1024) == 700);
    EXPECT(fl_frames(FL_MAX_N, 256) == (1 << 20) && fl_last(FL_MAX_N, 256) == 256);
    EXPECT(fl_frames(FL_MAX_N, 4096) == (1 << 16) && fl_last(FL_MAX_N - 1, 4096) == 4095);
    snprintf(where, sizeof where, "bound");
    EXPECT(fl_bound(0, 1, 256) == -1 && fl_bound(1, 0, 256) == -1 && fl_bound(1, 3, 256) == -1 && fl_bound(1, 1, 100) == -1);
    EXPECT(fl_bound(FL_MAX_N + 1, 1, 256) == -1 && fl_bound(-5, 2, 4096) == -1);
    EXPECT(fl_bound(1, 1, 256) == 42 + 17 + 1 + 2);
    EXPECT(fl_bound(1, 2, 4096) == 42 + 17 + 2 + 4);
    EXPECT(fl_bound(257, 2, 256) == 42 + 2 * 19 + 4 * 257);
    EXPECT(fl_bound(FL_MAX_N, 2, 256) == 42 + (1LL << 20) * 19 + 4 * FL_MAX_N);
    // the bound is the frames' own bounds and the head: no frame's slot can outgrow it
    std::mt19937 rng(3u);
    for (int it = 0; it < 400; ++it) {
        const int B = 256 << (int)(rng() % 5), ch = 1 + (int)(rng() % 2);
        const long long n = 1 + (long long)(rng() % 20000);
        long long sum = FL_STREAM_HEAD;
        for (long long f = 0; f < fl_frames(n, B); ++f) sum += fl_frame_bound(f + 1 < fl_frames(n, B) ? B : fl_last(n, B), ch);
        EXPECT(sum == fl_bound(n, ch, B));
    }
}

static void numbers() {
    snprintf(where, sizeof where, "numbers");
    struct Case { uint32_t v; int n; uint8_t b[6]; };
    const Case CASES[] = {
        {0, 1, {0x00}},
        {127, 1, {0x7F}},
        {128, 2, {0xC2, 0x80}},
        {2047, 2, {0xDF, 0xBF}},
        {2048, 3, {0xE0, 0xA0, 0x80}},
        {65535, 3, {0xEF, 0xBF, 0xBF}},
        {65536, 4, {0xF0, 0x90, 0x80, 0x80}},
        {(1u << 20) - 1, 4, {0xF3, 0xBF, 0xBF, 0xBF}},
        {(1u << 21) - 1, 4, {0xF7, 0xBF, 0xBF, 0xBF}},
        {1u << 21, 5, {0xF8, 0x88, 0x80, 0x80, 0x80}},
        {(1u << 26) - 1, 5, {0xFB, 0xBF, 0xBF, 0xBF, 0xBF}},
        {1u << 26, 6, {0xFC, 0x84, 0x80, 0x80, 0x80, 0x80}},
        {0x7FFFFFFFu, 6, {0xFD, 0xBF, 0xBF, 0xBF, 0xBF, 0xBF}},
    };
    for (const Case& c : CASES) {
        std::vector<uint8_t> out((size_t)c.n);                  // exactly the bytes the number takes
        EXPECT(fl_number(c.v, out.data()) == c.n);
        EXPECT(memcmp(out.data(), c.b, (size_t)c.n) == 0);
    }
    // every length decodes back
    std::mt19937 rng(5u);
    for (int it = 0; it < 20000; ++it) {
        const uint32_t v = (uint32_t)rng() >> (1 + rng() % 31);
        uint8_t out[6];
        const int n = fl_number(v, out);
        uint32_t back = n == 1 ? out[0] : out[0] & (0x7Fu >> n);
        for (int i = 1; i < n; ++i) {
            EXPECT((out[i] & 0xC0) == 0x80);
            back = (back << 6) | (out[i] & 0x3Fu);
        }
        EXPECT(back == v);
    }
}

static void crcs() {
    snprintf(where, sizeof where, "crcs");
    const uint8_t* check = (const uint8_t*)"123456789";
    EXPECT(fl_crc8(check, 9) == 0xF4);
    EXPECT(fl_crc16(check, 9) == 0xFEE8);
    // the tables, entry by entry, against the bit-serial definition
    for (int b = 0; b < 256; ++b) {
        unsigned c8 = (unsigned)b, c16 = (unsigned)b << 8;
        for (int i = 0; i < 8; ++i) {
            c8 = ((c8 << 1) ^ ((c8 & 0x80) ? 0x107u : 0u)) & 0xFF;
            c16 = ((c16 << 1) ^ ((c16 & 0x8000) ? 0x18005u : 0u)) & 0xFFFF;
        }
        EXPECT(fl_crc8_entry(b) == c8 && fl_crc16_entry(b) == c16);
    }
    EXPECT(fl_crc8_entry(1) == 0x07 && fl_crc16_entry(1) == 0x8005 && fl_crc16_entry(255) == 0x0202);
    // joining runs: the rule flac_pack_kernel uses, for every way of cutting a frame into the threads' runs
    std::mt19937 rng(11u);
    for (int it = 0; it < 300; ++it) {
        const int nb = 1 + (int)(rng() % (it < 10 ? 20 : 17000)), threads = 256;
        std::vector<uint8_t> buf((size_t)nb);
        for (auto& v : buf) v = (uint8_t)rng();
        const int chunk = (nb + threads - 1) / threads;
        uint16_t joined = 0;
        for (int t = 0; t < threads; ++t) {
            const int ba = t * chunk < nb ? t * chunk : nb, be = ba + chunk < nb ? ba + chunk : nb;
            if (be > ba) joined ^= fl_crc16_shift(fl_crc16(buf.data() + ba, be - ba), nb - be);
        }
        snprintf(where, sizeof where, "crc join nb %d", nb);
        EXPECT(joined == fl_crc16(buf.data(), nb));
    }
    EXPECT(fl_crc16_shift(0x1234, 0) == 0x1234 && fl_gf_mul(1, 0xBEEF) == 0xBEEF && fl_gf_mul(0xBEEF, 1) == 0xBEEF);
}

static void headers() {
    snprintf(where, sizeof where, "headers");
    // RFC 9639's one-frame stereo example: blocksize 1 of a 4096 stream, 44100 Hz, (L, R), frame 0
    {
        uint8_t h[FL_HEADER_MAX];
        const uint8_t want[] = {0xFF, 0xF8, 0x69, 0x18, 0x00, 0x00, 0xBF};
        EXPECT(fl_frame_header(h, 1, 4096, 44100, 1, 0) == 7 && memcmp(h, want, 7) == 0);
        uint8_t head[FL_STREAM_HEAD];
        fl_stream_head(head, 4096, 15, 15, 44100, 2, 1);
        const uint8_t si[] = {0x66, 0x4C, 0x61, 0x43, 0x80, 0x00, 0x00, 0x22, 0x10, 0x00, 0x10, 0x00, 0x00, 0x00, 0x0F, 0x00, 0x00, 0x0F,
                              0x0A, 0xC4, 0x42, 0xF0, 0x00, 0x00, 0x00, 0x01};
        EXPECT(memcmp(head, si, sizeof si) == 0);
        for (int i = 26; i < FL_STREAM_HEAD; ++i) EXPECT(head[i] == 0);
        const uint8_t frame[] = {0xFF, 0xF8, 0x69, 0x18, 0x00, 0x00, 0xBF, 0x03, 0x58, 0xFD, 0x03, 0x12, 0x8B};
        EXPECT(fl_crc16(frame, sizeof frame) == 0xAA9A);
    }
    struct Case { int bs, B, rate, a; uint32_t number; int len; uint8_t b[FL_HEADER_MAX]; };
    const Case CASES[] = {
        {256, 256, 8000, 0, 5, 6, {0xFF, 0xF8, 0x84, 0x08, 0x05}},
        {4096, 4096, 48000, 10, 127, 6, {0xFF, 0xF8, 0xCA, 0xA8, 0x7F}},
        {255, 256, 16000, 8, 128, 8, {0xFF, 0xF8, 0x65, 0x88, 0xC2, 0x80, 0xFE}},
        {256, 1024, 22050, 9, 2, 7, {0xFF, 0xF8, 0x66, 0x98, 0x02, 0xFF}},
        {257, 1024, 24000, 1, 2048, 10, {0xFF, 0xF8, 0x77, 0x18, 0xE0, 0xA0, 0x80, 0x01, 0x00}},
        {700, 1024, 32000, 0, 1, 8, {0xFF, 0xF8, 0x78, 0x08, 0x01, 0x02, 0xBB}},
        {512, 512, 11025, 0, 0, 8, {0xFF, 0xF8, 0x9D, 0x08, 0x00, 0x2B, 0x11}},
        {4095, 4096, 12345, 1, 65536, 13, {0xFF, 0xF8, 0x7D, 0x18, 0xF0, 0x90, 0x80, 0x80, 0x0F, 0xFE, 0x30, 0x39}},
        {1, 256, 44100, 0, 0x7FFFFFFF, 12, {0xFF, 0xF8, 0x69, 0x08, 0xFD, 0xBF, 0xBF, 0xBF, 0xBF, 0xBF, 0x00}},
    };
    for (const Case& c : CASES) {
        snprintf(where, sizeof where, "header bs %d B %d rate %d", c.bs, c.B, c.rate);
        std::vector<uint8_t> h((size_t)c.len);                   // exactly the bytes the header takes
        EXPECT(fl_frame_header(h.data(), c.bs, c.B, c.rate, c.a, c.number) == c.len);
        EXPECT(memcmp(h.data(), c.b, (size_t)c.len - 1) == 0);
        EXPECT(h[(size_t)c.len - 1] == fl_crc8(h.data(), c.len - 1));
    }
    // the longest header there is fills FL_HEADER_MAX exactly
    uint8_t h[FL_HEADER_MAX];
    EXPECT(fl_frame_header(h, 4095, 4096, 12345, 1, 0x7FFFFFFF) == FL_HEADER_MAX);
    // STREAMINFO at the limits: 24-bit frame sizes, a 36-bit n above 2^28's own width is not needed, the rate's 20 bits
    uint8_t head[FL_STREAM_HEAD];
    fl_stream_head(head, 256, 0x010203, 0xFFFFFF, 48000, 1, FL_MAX_N);
    const uint8_t want[] = {0x01, 0x00, 0x01, 0x00, 0x01, 0x02, 0x03, 0xFF, 0xFF, 0xFF, 0x0B, 0xB8, 0x00, 0xF0, 0x10, 0x00, 0x00, 0x00};
    snprintf(where, sizeof where, "streaminfo");
    EXPECT(memcmp(head + 8, want, sizeof want) == 0);
}

int main() {
    checks();
    frames_and_bound();
    numbers();
    crcs();
    headers();
    if (failures) {
        fprintf(stderr, "flac_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("flac_check: ok\n");
    return 0;
}
