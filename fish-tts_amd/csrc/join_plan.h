// Host-side planner of the join stage (fishtts_hip.h: ft_codec_decode_join, ft_join_groups; fishtts_hip_test.h:
// ft_test_join): the argument checks, the room a call needs, where the items lie in the stage's input buffer and how a
// document's items are grouped into calls.  Plain C++ without HIP, so that a host program can drive it under a sanitizer
// (tools/join_plan_check.cpp).
#pragma once
#include <stdint.h>

#include "../../include/fishtts_hip.h"

namespace ft {

constexpr int JOIN_MAX_ITEMS = 64;
constexpr int64_t JOIN_MAX_SAMPLES = (int64_t)1 << 28;   // items and gaps of one call together (1 GiB of float32)

// Null when the stage can run on B items of n[b] samples; else why not.  *need: sum(n) + sum(gaps), the room the output
// takes at most (set whenever the counts themselves are sound).
inline const char* join_check(int32_t B, const int64_t* n, const ft_join_params* jp, const int64_t* gaps, int32_t started,
                              int64_t capacity, int64_t* need) {
    if (need) *need = 0;
    if (B < 1 || B > JOIN_MAX_ITEMS) return "1 <= B <= 64 items";
    if (!n || !jp || !gaps) return "a null pointer";
    if (!(jp->threshold >= 0.f)) return "threshold must be >= 0";   // (refuses a NaN too)
    if (jp->hop < 1 || jp->keep < 0 || jp->fade < 0) return "hop >= 1, keep >= 0, fade >= 0";
    if (started != 0 && started != 1) return "started must be 0 or 1";
    int64_t sum = 0;
    for (int32_t b = 0; b < B; ++b) {
        if (n[b] < 0) return "a negative item length";
        if (gaps[b] < 0) return "a negative gap";
        if (n[b] > JOIN_MAX_SAMPLES || gaps[b] > JOIN_MAX_SAMPLES) return "more than 2^28 samples in one call";
        sum += n[b] + gaps[b];
        if (sum > JOIN_MAX_SAMPLES) return "more than 2^28 samples in one call";
    }
    if (need) *need = sum;
    if (capacity < sum) return "capacity below sum(out_lens) + sum(gaps)";
    return nullptr;
}

// Item b lies at off[b] of the stage's input buffer, every item on a 16-byte boundary; returns the floats that takes.
inline int64_t join_offsets(int32_t B, const int64_t* n, int64_t* off) {
    int64_t at = 0;
    for (int32_t b = 0; b < B; ++b) {
        off[b] = at;
        at += (n[b] + 3) & ~(int64_t)3;
    }
    return at;
}

// Consecutive items, lens[i] code frames each, grouped into calls of at most JOIN_MAX_ITEMS items and max_frames frames:
// ends[g] is one past the last item of group g.  Returns the number of groups; -1 for a negative length, an item longer than
// max_frames on its own or a bad argument.
inline int32_t join_groups(const int32_t* lens, int32_t n, int32_t max_frames, int32_t* ends) {
    if (n < 0 || max_frames < 1 || (n > 0 && (!lens || !ends))) return -1;
    int32_t g = 0, items = 0;
    int64_t frames = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (lens[i] < 0 || lens[i] > max_frames) return -1;
        if (items > 0 && (items == JOIN_MAX_ITEMS || frames + lens[i] > max_frames)) {
            ends[g++] = i;
            items = 0;
            frames = 0;
        }
        ++items;
        frames += lens[i];
    }
    if (items > 0) ends[g++] = n;
    return g;
}

}  // namespace ft
