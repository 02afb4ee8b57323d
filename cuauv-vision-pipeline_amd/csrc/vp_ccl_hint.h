// Which launches the two-level labelling queues behind its merge (ccl_two_level, vp_ccl.hip).  Plain C++ - no HIP types - so that the
// rule is checked without a GPU (tests/native/ccl_hint_main.cpp).
//
//   FULL  the crowded-frame kernels of vp_ccl3.inl: six launches that read the list of frames the merge handed over and leave at
//         once when it is empty;
//   LEAN  one launch in their place (k_ccl2_finish), which finishes a handed-over frame correctly but slowly.
//
// Both give the same results, so the choice costs time only.  It follows a hint: the number of frames the merge of an EARLIER call
// handed over, which the device leaves in a pinned word and the host reads without synchronising - possibly stale by any number of
// calls.  A cleaned mask is almost never crowded and crowded input comes in runs, so the rule leaves LEAN as soon as a hint says
// "crowded" and returns after CCL_HINT_QUIET consecutive quiet hints (the count vp_find_contours_* waits before it shrinks its
// capacities).
#pragma once

#define CCL_HINT_QUIET 32

enum { CCL_MODE_LEAN = 0, CCL_MODE_FULL = 1 };
enum { CCL_FORCE_AUTO = 0, CCL_FORCE_FULL = 1, CCL_FORCE_LEAN = 2 };   // VP_OPT_CCL_CROWDED

struct ccl_hint_state {
    int mode;                  // what the last decision was; a zero-filled state is a new context: LEAN
    int quiet;                 // consecutive hints of 0 read while in FULL
};

// The mode of the call at hand.  hint: the pinned word as read now; force: the override; chain_streams: LEAN is allowed only
// with one chain stream, the condition under which the crowded-frame kernels own the context's accumulator set (sub-batches on several
// streams would also share the one hint word).
// The state follows the hints whatever the override and the stream count say, so that either can change between calls.
static inline int ccl_hint_decide(ccl_hint_state& st, unsigned int hint, int force, int chain_streams)
{
    if (hint > 0u) {
        st.mode = CCL_MODE_FULL;
        st.quiet = 0;
    } else if (st.mode == CCL_MODE_FULL && ++st.quiet >= CCL_HINT_QUIET) {
        st.mode = CCL_MODE_LEAN;
        st.quiet = 0;
    }
    if (chain_streams != 1) return CCL_MODE_FULL;
    if (force == CCL_FORCE_FULL) return CCL_MODE_FULL;
    if (force == CCL_FORCE_LEAN) return CCL_MODE_LEAN;
    return st.mode;
}
