// lk_branches_emu.cpp -- TEST ONLY.  The CPU-emulator harness of tests/lk_branches.py: lk_fit_emu.cpp as it is (fe_track, lf_chain and
// the counter of iterations per level and kind of sum) and the second counter lk.hip keeps under VO_HOST_EMUL only: iterations that
// sampled the search window with iw11 = -1, the out-of-line case of blend7_cols behind the iteration's scalar branch.  Not a
// product path.
#include "lk_fit_emu.cpp"

extern "C" {

// iterations with iw11 = -1 since the last reset
long long lb_neg_iterations(int reset)
{
    const long long n = vo::g_lk_neg_iterations;
    if (reset)
        vo::g_lk_neg_iterations = 0;
    return n;
}
}
