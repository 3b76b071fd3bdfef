// Host program that drives the live FLAC stage's host arithmetic (fish-tts_amd/csrc/flac_plan.h: fl_push_plan's emission rule,
// the stream's host state FlStream with its head bytes, the per-push checks in their stated order, the 2^36 - 1 limit) so that
// a build with -fsanitize=address,undefined sees any read or write past an array and any overflow.  No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/flac_stream_check.cpp -o flac_stream_check
// Exit status 0 and "flac_stream_check: ok" when every expectation holds.
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

static const int NO_KINDS[FL_KINDS] = {}, NO_ASSIGNMENTS[FL_ASSIGNMENTS] = {};

// One cutting of N samples: every push against the whole's frames.  A frame is taken to weigh 20 + its number bytes.
static void cutting(int B, int ch, long long N, const std::vector<long long>& cuts) {
    FlStream s;
    s.B = B; s.channels = ch;
    long long bytes = 0, frames = 0, bound = 0;
    for (size_t i = 0; i < cuts.size(); ++i) {
        const bool final = i + 1 == cuts.size();
        const long long n = cuts[i];
        EXPECT(s.carry() >= 0 && s.carry() < B);
        const FlPush p = s.plan(n, final);
        EXPECT(p.r == s.carry() && p.T == p.r + n);
        EXPECT(s.n_in - p.r == s.F_done * B);                               // the first emitted frame begins where the whole's does
        EXPECT(p.F == (final ? fl_frames(p.T, B) : p.T / B));
        EXPECT(p.keep >= 0 && p.keep < B && (!final || p.keep == 0) && p.taken + p.keep == p.T);
        if (p.F > 0) EXPECT(p.last == (final ? p.T - (p.F - 1) * B : B) && p.last >= 1 && p.last <= B);
        else EXPECT(p.bytes == 0 && p.taken == 0);
        long long sum = 0;                                                  // the bound is the frames' own bounds
        for (long long f = 0; f < p.F; ++f) sum += fl_frame_bound(f + 1 < p.F ? B : p.last, ch);
        EXPECT(sum == p.bytes);
        bool state = true, tl = true;
        EXPECT(fl_stream_check(&s, false, n == 0, n, final, p.bytes, &state, &tl) == nullptr && !state && !tl);
        if (p.bytes > 0) EXPECT(fl_stream_check(&s, false, false, n, final, p.bytes - 1, &state, &tl) != nullptr && !state && !tl);
        const long long got = 20 * p.F + (long long)i;
        s.commit(p, n, final, got, 20, 20 + (int)i, NO_KINDS, NO_ASSIGNMENTS);
        bytes += got;
        frames += p.F;
        bound += p.bytes;
        EXPECT(s.par == (int)((i + 1) & 1) && s.ended == final && s.F_done == frames && s.bytes == bytes);
    }
    EXPECT(s.n_in == N && s.carry() == 0);
    EXPECT(frames == (N > 0 ? fl_frames(N, B) : 0));
    if (N > 0 && N <= FL_MAX_N) EXPECT(bound <= fl_bound(N, ch, B) - FL_STREAM_HEAD && bound == fl_bound(N, ch, B) - FL_STREAM_HEAD);
    bool state = false, tl = false;
    EXPECT(fl_stream_check(&s, false, true, 0, true, 1 << 20, &state, &tl) != nullptr && state && !tl);
}

static void emission() {
    std::mt19937 rng(7u);
    for (int it = 0; it < 4000; ++it) {
        const int B = 256 << (int)(rng() % 5), ch = 1 + (int)(rng() % 2);
        const int pushes = 1 + (int)(rng() % 12);
        std::vector<long long> cuts((size_t)pushes);
        long long N = 0;
        for (auto& c : cuts) {
            const unsigned kind = rng() % 6;
            c = kind == 0 ? 0 : kind == 1 ? 1 + (long long)(rng() % 3) : kind == 2 ? B - 1 + (long long)(rng() % 3)
                : (long long)(rng() % (3u * (unsigned)B + 1));
            N += c;
        }
        snprintf(where, sizeof where, "cutting %d: B %d ch %d N %lld in %d", it, B, ch, N, pushes);
        cutting(B, ch, N, cuts);
    }
    snprintf(where, sizeof where, "cutting: fixed");
    cutting(256, 1, 0, {0});                                                // a stream of nothing: no frame, the head alone
    cutting(256, 2, 1, {1});
    cutting(256, 1, 256, {255, 1, 0});
    cutting(256, 1, 257, {256, 0, 1});
    cutting(4096, 2, 3 * 4096, {4096, 4096, 4096, 0});
    cutting(1024, 1, FL_MAX_N + 5, {5, FL_MAX_N});
    const FlPush p = fl_push_plan(256, 2, 255, 258, false);                 // r 255, T 513: two frames, one sample stays
    EXPECT(p.r == 255 && p.T == 513 && p.F == 2 && p.keep == 1 && p.last == 256 && p.bytes == 2 * 19 + 4 * 512);
    const FlPush q = fl_push_plan(256, 2, 255, 258, true);
    EXPECT(q.F == 3 && q.keep == 0 && q.last == 1 && q.bytes == 3 * 19 + 4 * 513);
}

static void refusals() {
    snprintf(where, sizeof where, "refusals");
    FlStream live, done;
    live.B = done.B = 256;
    done.ended = true;
    const long long big = INT64_MAX;
    bool st = true, tl = true;
    EXPECT(fl_stream_check(&live, false, false, 100, false, 0, &st, &tl) == nullptr && !st && !tl);   // no frame: no capacity needed
    // the stated order: each reason in front of every later one
    const char* why = fl_stream_check(nullptr, false, false, -1, false, 0, &st, &tl);
    EXPECT(why && strstr(why, "null pointer") && !st && !tl);
    why = fl_stream_check(&done, true, true, -1, false, 0, &st, &tl);
    EXPECT(why && strstr(why, "null pointer") && !st && !tl);
    why = fl_stream_check(&done, false, true, -1, false, 0, &st, &tl);
    EXPECT(why && strstr(why, "n < 0") && !st && !tl);
    why = fl_stream_check(&done, false, true, FL_MAX_N + 1, false, 0, &st, &tl);
    EXPECT(why && strstr(why, "x is null") && !st && !tl);
    why = fl_stream_check(&done, false, false, FL_MAX_N + 1, false, 0, &st, &tl);
    EXPECT(why && strstr(why, "after the final") && st && !tl);
    why = fl_stream_check(&live, false, false, FL_MAX_N + 1, false, 0, &st, &tl);
    EXPECT(why && strstr(why, "2^28") && !st && tl);
    why = fl_stream_check(&live, false, false, FL_MAX_N, false, 0, &st, &tl);
    EXPECT(why && strstr(why, "capacity") && !st && !tl);
    EXPECT(fl_stream_check(&live, false, false, FL_MAX_N, false, big, &st, &tl) == nullptr);
    EXPECT(fl_stream_check(&live, false, true, 0, true, 0, &st, &tl) == nullptr);                     // x may be null with n = 0
    // STREAMINFO's 36 bits
    snprintf(where, sizeof where, "2^36");
    FlStream far;
    far.B = 4096; far.channels = 2;
    far.n_in = FL_MAX_TOTAL - 10;
    far.F_done = far.n_in / 4096;
    EXPECT(fl_stream_check(&far, false, false, 10, true, big, &st, &tl) == nullptr && !tl);
    why = fl_stream_check(&far, false, false, 11, true, big, &st, &tl);
    EXPECT(why && strstr(why, "2^36") && tl && !st);
    why = fl_stream_check(&far, false, false, FL_MAX_N + 1, true, big, &st, &tl);
    EXPECT(why && strstr(why, "2^28") && tl);
    EXPECT(fl_push_refused(4096, 2, FL_MAX_TOTAL - 10, 10) == 0 && fl_push_refused(4096, 2, FL_MAX_TOTAL - 10, 11) == 2);
    EXPECT(fl_push_refused(4096, 2, FL_MAX_TOTAL, 0) == 0 && fl_push_refused(4096, 2, FL_MAX_TOTAL + 1, 0) == 2);
    EXPECT(fl_push_refused(4096, 2, INT64_MAX, 1) == 2 && fl_push_refused(4096, 2, 0, FL_MAX_N + 1) == 2);
    EXPECT(fl_push_refused(4095, 2, 0, 1) == 1 && fl_push_refused(256, 3, 0, 1) == 1 && fl_push_refused(256, 1, -1, 1) == 1 &&
           fl_push_refused(256, 1, 0, -1) == 1 && fl_push_refused(256, 1, 0, 0) == 0);
    const FlPush p = far.plan(10, true);                                    // the frame number at the far end fits fl_number's 31 bits
    EXPECT(far.F_done + p.F <= 0x7FFFFFFFLL);
    EXPECT(FL_MAX_TOTAL / 256 + 1 <= 0x7FFFFFFFLL);
    // begin's checks: fl_check's order without n and the capacity
    snprintf(where, sizeof where, "begin");
    EXPECT(fl_stream_begin_check(0, 1, 44100, 4096, 0) == nullptr && fl_stream_begin_check(1, 2, 8000, 256, 0) == nullptr);
    EXPECT(strstr(fl_stream_begin_check(2, 3, 7999, 100, 1), "fmt"));
    EXPECT(strstr(fl_stream_begin_check(0, 3, 7999, 100, 1), "channels"));
    EXPECT(strstr(fl_stream_begin_check(0, 2, 7999, 100, 1), "sample rate"));
    EXPECT(strstr(fl_stream_begin_check(0, 2, 44100, 100, 1), "blocksize"));
    EXPECT(strstr(fl_stream_begin_check(0, 2, 44100, 512, 1), "reserved"));
}

static void heads() {
    snprintf(where, sizeof where, "heads");
    FlStream s;
    s.B = 4096; s.channels = 2; s.rate = 44100;
    uint8_t head[FL_STREAM_HEAD];                                           // sized exactly
    const uint8_t unknown[FL_STREAM_HEAD] = {0x66, 0x4C, 0x61, 0x43, 0x80, 0x00, 0x00, 0x22, 0x10, 0x00, 0x10, 0x00, 0x00, 0x00, 0x00,
                                             0x00, 0x00, 0x00, 0x0A, 0xC4, 0x42, 0xF0, 0x00, 0x00, 0x00, 0x00};
    s.head(head);
    EXPECT(memcmp(head, unknown, sizeof unknown) == 0);
    int kinds[FL_KINDS] = {1, 0, 0, 2, 0, 0, 1}, as[FL_ASSIGNMENTS] = {0, 1, 0, 0, 1};
    s.commit(s.plan(4999, false), 4999, false, 700, 0x0123, 0x4567, kinds, as);
    EXPECT(s.F_done == 1 && s.carry() == 903 && s.fmin == 0x0123 && s.fmax == 0x4567);
    s.head(head);                                                           // still unknown: the stream has not ended
    EXPECT(memcmp(head, unknown, sizeof unknown) == 0);
    s.commit(s.plan(1, true), 1, true, 90, 0x0099, 0x0099, kinds, as);
    EXPECT(s.F_done == 2 && s.n_in == 5000 && s.carry() == 0 && s.bytes == 790 && s.fmin == 0x0099 && s.fmax == 0x4567);
    EXPECT(s.kinds[0] == 2 && s.kinds[3] == 4 && s.kinds[6] == 2 && s.assignments[1] == 2 && s.assignments[4] == 2 && s.assignments[0] == 0);
    const uint8_t known[FL_STREAM_HEAD] = {0x66, 0x4C, 0x61, 0x43, 0x80, 0x00, 0x00, 0x22, 0x10, 0x00, 0x10, 0x00, 0x00, 0x00, 0x99,
                                           0x00, 0x45, 0x67, 0x0A, 0xC4, 0x42, 0xF0, 0x00, 0x00, 0x13, 0x88};
    s.head(head);
    EXPECT(memcmp(head, known, sizeof known) == 0);
    FlStream m;                                                             // mono, 8 kHz, blocksize 256, ended with nothing
    m.B = 256; m.rate = 8000;
    const uint8_t mono[FL_STREAM_HEAD] = {0x66, 0x4C, 0x61, 0x43, 0x80, 0x00, 0x00, 0x22, 0x01, 0x00, 0x01, 0x00, 0x00, 0x00, 0x00,
                                          0x00, 0x00, 0x00, 0x01, 0xF4, 0x00, 0xF0, 0x00, 0x00, 0x00, 0x00};
    m.head(head);
    EXPECT(memcmp(head, mono, sizeof mono) == 0);
    m.commit(m.plan(0, true), 0, true, 0, 0, 0, NO_KINDS, NO_ASSIGNMENTS);
    m.head(head);
    EXPECT(m.ended && m.F_done == 0 && memcmp(head, mono, sizeof mono) == 0);
    FlStream e;                                                             // the 36-bit field filled
    e.B = 256; e.rate = 8000; e.n_in = FL_MAX_TOTAL; e.fmin = 1; e.fmax = 2; e.ended = true;
    e.head(head);
    const uint8_t full[8] = {0x01, 0xF4, 0x00, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
    EXPECT(memcmp(head + 18, full, 8) == 0 && head[14] == 1 && head[17] == 2);
}

int main() {
    emission();
    refusals();
    heads();
    if (failures) {
        fprintf(stderr, "flac_stream_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("flac_stream_check: ok\n");
    return 0;
}
