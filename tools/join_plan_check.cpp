// Host program that drives the join stage's planner (fish-tts_amd/csrc/join_plan.h: argument checks, capacity, the layout
// of the input buffer, the grouping of a document's items into calls) on arrays of exactly the stated sizes, so that a
// build with -fsanitize=address,undefined sees any read or write past them and any overflow.  No GPU, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/join_plan_check.cpp -o join_plan_check
// Exit status 0 and "join_plan_check: ok" when every expectation holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../fish-tts_amd/csrc/join_plan.h"

static int failures = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);       \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void checks() {
    const ft_join_params ok{0.1f, 220, 1323, 220};
    int64_t need = -1;
    for (int B = 1; B <= ft::JOIN_MAX_ITEMS; ++B) {       // heap arrays of exactly B entries
        std::vector<int64_t> n(B), gaps(B), off(B);
        int64_t sum = 0, in = 0;
        for (int b = 0; b < B; ++b) {
            n[b] = (int64_t)(rnd() % 5000);
            gaps[b] = (int64_t)(rnd() % 3);
            sum += n[b] + gaps[b];
            in += (n[b] + 3) / 4 * 4;
        }
        EXPECT(ft::join_check(B, n.data(), &ok, gaps.data(), 0, sum, &need) == nullptr && need == sum);
        EXPECT(ft::join_check(B, n.data(), &ok, gaps.data(), 1, sum + 1, &need) == nullptr);
        EXPECT(ft::join_check(B, n.data(), &ok, gaps.data(), 0, sum - 1, &need) != nullptr && need == sum);
        EXPECT(ft::join_offsets(B, n.data(), off.data()) == in);
        for (int b = 0; b < B; ++b) {
            EXPECT(off[b] % 4 == 0);
            EXPECT(b == 0 || off[b] >= off[b - 1] + n[b - 1]);
        }
        const int64_t keep = n[B - 1];
        n[B - 1] = -1;
        EXPECT(ft::join_check(B, n.data(), &ok, gaps.data(), 0, sum, &need) != nullptr);
        n[B - 1] = keep;
        gaps[B / 2] = -1;
        EXPECT(ft::join_check(B, n.data(), &ok, gaps.data(), 0, sum, &need) != nullptr);
    }
    int64_t n1[1] = {8}, g1[1] = {0};
    EXPECT(ft::join_check(0, n1, &ok, g1, 0, 100, &need) != nullptr);
    EXPECT(ft::join_check(65, n1, &ok, g1, 0, 100, &need) != nullptr);      // refused before n[1] is looked at
    EXPECT(ft::join_check(-1, n1, &ok, g1, 0, 100, nullptr) != nullptr);
    EXPECT(ft::join_check(1, nullptr, &ok, g1, 0, 100, &need) != nullptr);
    EXPECT(ft::join_check(1, n1, nullptr, g1, 0, 100, &need) != nullptr);
    EXPECT(ft::join_check(1, n1, &ok, nullptr, 0, 100, &need) != nullptr);
    EXPECT(ft::join_check(1, n1, &ok, g1, 2, 100, &need) != nullptr);
    EXPECT(ft::join_check(1, n1, &ok, g1, -1, 100, &need) != nullptr);
    EXPECT(ft::join_check(1, n1, &ok, g1, 0, 8, nullptr) == nullptr);
    const ft_join_params bad[] = {{-0.1f, 220, 0, 0}, {std::numeric_limits<float>::quiet_NaN(), 220, 0, 0}, {0.1f, 0, 0, 0},
                                  {0.1f, -1, 0, 0}, {0.1f, 1, -1, 0}, {0.1f, 1, 0, -1}};
    for (const ft_join_params& p : bad) EXPECT(ft::join_check(1, n1, &p, g1, 0, 100, &need) != nullptr);
    const ft_join_params edge{0.f, 1, 0, 0};
    EXPECT(ft::join_check(1, n1, &edge, g1, 0, 8, &need) == nullptr);
    // sums that would overflow or exceed the limit of one call are refused, not wrapped
    const int64_t big = std::numeric_limits<int64_t>::max();
    int64_t n2[2] = {big, big}, g2[2] = {big, big};
    EXPECT(ft::join_check(2, n2, &ok, g1, 0, big, &need) != nullptr);
    int64_t n3[2] = {ft::JOIN_MAX_SAMPLES, 1}, g3[2] = {0, 0};
    EXPECT(ft::join_check(2, n3, &ok, g3, 0, big, &need) != nullptr);
    EXPECT(ft::join_check(2, n3, &ok, g2, 0, big, &need) != nullptr);
    n3[1] = 0;
    EXPECT(ft::join_check(2, n3, &ok, g3, 0, big, &need) == nullptr && need == ft::JOIN_MAX_SAMPLES);
}

static void groups() {
    for (int round = 0; round < 2000; ++round) {
        const int n = (int)(rnd() % 200), max_frames = 1 + (int)(rnd() % 300);
        std::vector<int32_t> lens(n), ends(n);            // ends: exactly n entries (every item alone at the worst)
        for (int i = 0; i < n; ++i) lens[i] = (int32_t)(rnd() % (unsigned)(max_frames + 1));
        const int g = ft::join_groups(lens.data(), n, max_frames, ends.data());
        EXPECT(g >= 0 && g <= n && (n == 0) == (g == 0));
        int at = 0;
        for (int k = 0; k < g; ++k) {
            EXPECT(ends[k] > at && ends[k] - at <= ft::JOIN_MAX_ITEMS);
            int64_t frames = 0;
            for (int i = at; i < ends[k]; ++i) frames += lens[i];
            EXPECT(frames <= max_frames);
            // greedy: the next item would not have fitted
            if (k + 1 < g) EXPECT(ends[k] - at == ft::JOIN_MAX_ITEMS || frames + lens[ends[k]] > max_frames);
            at = ends[k];
        }
        EXPECT(at == n);
        if (n > 0) {
            const int i = (int)(rnd() % (unsigned)n);
            const int32_t keep = lens[i];
            lens[i] = max_frames + 1;
            EXPECT(ft::join_groups(lens.data(), n, max_frames, ends.data()) == -1);
            lens[i] = -1;
            EXPECT(ft::join_groups(lens.data(), n, max_frames, ends.data()) == -1);
            lens[i] = keep;
        }
    }
    std::vector<int32_t> zeros(130, 0), ends(130);
    EXPECT(ft::join_groups(zeros.data(), 130, 5, ends.data()) == 3 && ends[0] == 64 && ends[1] == 128 && ends[2] == 130);
    EXPECT(ft::join_groups(nullptr, 1, 5, ends.data()) == -1 && ft::join_groups(zeros.data(), 1, 5, nullptr) == -1);
    EXPECT(ft::join_groups(zeros.data(), -1, 5, ends.data()) == -1 && ft::join_groups(zeros.data(), 1, 0, ends.data()) == -1);
}

int main() {
    checks();
    groups();
    if (failures) {
        fprintf(stderr, "join_plan_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("join_plan_check: ok\n");
    return 0;
}
