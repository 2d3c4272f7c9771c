// rips_ladder.h -- the retry ladder of the Rips launchers (rips.hip) as plain data: no HIP, no context.
// A flavour (distance matrices, fused EEG windows, point clouds) has rungs r0 < r1 < ..., H1 class capacities in its own
// unit (matrices: u64 words, the other two: bits); `Rungs` holds the ones whose LDS layout fits and the index f of the
// first pass, chosen from tda_set_class_words.  F(r) is the first-pass kernel of a rung (one workgroup per window), R(r)
// the same capacity's kernel on the list of the flagged windows, T the last rung (class vectors in HBM, no capacity limit).
// THE RULE, for all three flavours (tda_set_retry_policy; tests/test_rips_ladder_model.py has the table):
//      AUTO         F(r_f), R(r_f+1), R(r_f+2), ..., T
//      FIRST_PASS   F(r_f)
//      ONLY               R(r_f+1), R(r_f+2), ..., T
//      ONE_STEP     F(r_f), R(r_f+1) if it exists; no T
//      LAST_RUNG    T
#pragma once

namespace rips_ladder {

enum Policy { AUTO = 0, FIRST_PASS = 1, ONLY = 2, ONE_STEP = 3, LAST_RUNG = 4 };       // the values of TDA_RETRY_*
const int MAX_RUNGS = 4;
struct Rungs { int n = 0; int cap[MAX_RUNGS] = {}; int first = 0; };         // available capacities, ascending; index of the first pass
struct Step { int cap; bool retry; };
struct Plan { int n = 0; Step step[MAX_RUNGS] = {}; bool last = false; };    // the steps, then T if `last`

inline Plan plan(int policy, const Rungs& r)
{
    const bool last_only = policy == LAST_RUNG;
    const bool do_first = policy != ONLY && !last_only;
    const bool do_ladder = policy != FIRST_PASS && !last_only;
    const bool one_step = policy == ONE_STEP;
    Plan p;
    if (do_first) p.step[p.n++] = Step{r.cap[r.first], false};
    const int end = !do_ladder ? 0 : (one_step && r.first + 2 < r.n) ? r.first + 2 : r.n;
    for (int i = r.first + 1; i < end; ++i) p.step[p.n++] = Step{r.cap[i], true};
    p.last = last_only || (do_ladder && !one_step);
    return p;
}

// Distance matrices: 1, 2, 4, 8 u64 words for n <= 64 (one vertex word) and a first pass of at most 4; 1, 2 words above.
// fits[i]: the layout of 1 << i words fits LDS (one word always runs).  The first pass is the widest rung that is
// available and not wider than the request (0, the fused kernel's 32 bits, counts as 1).
inline Rungs dm_rungs(int words, bool one_vertex_word, const bool fits[4])
{
    const int widest = one_vertex_word ? 8 : 2, widest_first = one_vertex_word ? 4 : 2;
    Rungs r;
    for (int i = 0; (1 << i) <= widest && (i == 0 || fits[i]); ++i) {
        if ((1 << i) <= words && (1 << i) <= widest_first) r.first = i;
        r.cap[r.n++] = 1 << i;
    }
    return r;
}
// Fused EEG windows: 32 bits (u32 x 1), then 64, 128, 512 (u64 x 1, 2, 8); words 0 -> 32, 1 -> 64, >= 2 -> 128.  No fit
// filter: a layout that does not fit is the launch's error.
inline Rungs eeg_rungs(int words)
{
    return Rungs{4, {32, 64, 128, 512}, words >= 2 ? 2 : words < 0 ? 0 : words};
}
// Point clouds: 32 bits (u32; a first pass only), 64 (u64 x 1) and, if its layout fits, 128 (u64 x 2); words 1 -> 32,
// 2 -> 64.
inline Rungs cloud_rungs(int words, bool fits128)
{
    return Rungs{fits128 ? 3 : 2, {32, 64, 128}, words == 1 ? 0 : 1};
}

}   // namespace rips_ladder
