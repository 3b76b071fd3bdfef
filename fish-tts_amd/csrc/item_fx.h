// Host-side planner of a join call whose items each bring their own output chain (fishtts_hip.h:
// ft_codec_decode_join_items): the order in which the chains are judged, every item's output length, and the union of what
// the call's chains need on the device - the distinct pitch tables, the buffers of the longest chain, the hop sums of the
// levelled items.  No new kernel stands behind the call: the stages are the existing ones (fx_chain.h), driven per item,
// and the level stage reads its target from the item.  Plain C++ without HIP, so that a host program can drive it under
// a sanitizer (tools/item_fx_check.cpp).
#pragma once
#include <stdint.h>

#include "../../include/fishtts_hip.h"
#include "fx_chain.h"
#include "join_plan.h"

namespace ft {

// What item_fx_make refused: the kind as FxDesc::make names it, the item (-1: the rate, which all items share), and the
// resampler design's own message for a rate.
struct ItemFxBad {
    chain::FxDesc::Bad bad = chain::FxDesc::OK;
    int item = -1;
    const char* why = nullptr;
};

// The chains of B items at one output rate: d[b] from fx[b].  The rate is judged first, then every item in order - speed,
// cents, pair, level, as FxDesc::make judges them.  d[0 .. B) is complete only when the result is OK.
inline ItemFxBad item_fx_make(int rate, const ft_item_fx* fx, int B, chain::FxDesc* d) {
    ItemFxBad r;
    chain::FxDesc probe;
    if ((r.bad = probe.make(rate, 100, 0, 0, &r.why)) != chain::FxDesc::OK) return r;
    for (int b = 0; b < B; ++b) {
        if ((r.bad = d[b].make(rate, fx[b].speed_pct, fx[b].pitch_cents, fx[b].loudness, &r.why)) != chain::FxDesc::OK) {
            r.item = b;
            return r;
        }
    }
    return r;
}

// Item b has lens[b] code frames (lens null: T each) of frame_len samples: n[b] = its own chain's output length, *frames the
// sum of the lengths.  Null, or why not: a length outside [0, T].
inline const char* item_fx_lens(const chain::FxDesc* d, int B, int T, const int32_t* lens, int frame_len, int64_t* n,
                                int64_t* frames) {
    int64_t sum = 0;
    for (int b = 0; b < B; ++b) {
        const int Tb = lens ? lens[b] : T;
        if (Tb < 0 || Tb > T) return "bad length";
        sum += Tb;
        n[b] = (int64_t)d[b].out_len((long long)Tb * frame_len);
    }
    if (frames) *frames = sum;
    return nullptr;
}

// The union of a call's chains.
struct ItemFxUnion {
    int cents[JOIN_MAX_ITEMS];     // the distinct non-zero cents values, in order of first use
    int ncents = 0;
    bool ps = false, ts = false, rs = false;   // some item has a pitch stage / a speed other than 100 / a resampler
    int levelled = 0;              // items with a level
    int lv[JOIN_MAX_ITEMS];        // their indices, ascending: the level stage's table holds these items only
    size_t hops = 0;               // hop sums of the levelled items together
};

// `n`: the items' output lengths, for the hop sums (null: not counted).
inline ItemFxUnion item_fx_union(const chain::FxDesc* d, int B, const int64_t* n) {
    ItemFxUnion u;
    for (int b = 0; b < B && b < JOIN_MAX_ITEMS; ++b) {
        if (d[b].cents != 0) {
            u.ps = true;
            int k = 0;
            while (k < u.ncents && u.cents[k] != d[b].cents) ++k;
            if (k == u.ncents) u.cents[u.ncents++] = d[b].cents;
        }
        u.ts = u.ts || d[b].pct != 100;
        u.rs = u.rs || d[b].K > 0;
        if (d[b].level != 0) {
            u.lv[u.levelled++] = b;
            const int H = chain::lv_hop(d[b].rate);
            if (n) u.hops += (size_t)((n[b] + H - 1) / H);
        }
    }
    return u;
}

}  // namespace ft
