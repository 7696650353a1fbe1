// pgw_loop_control.h -- the host's control flow of the surface-pressure loop (step_03_apply_to_era.py:182-319) in plain
// C++17: the reference's stopping rule, the number of passes the next launch carries, and the vector the latitude bands of
// a file exchange per launch.  No HIP and no pgw_ctx: pgw_capi.hip applies these to what it reads back from the device,
// tests/test_loop_control_host.py runs them on a CPU.
#pragma once
#include <math.h>

namespace pgw {

constexpr int LOOP_MAX_PASS = 8;       // passes of one launch at most (pgw_capi.hip asserts: = MULTI_MAX_PASS)

// The stopping rule, :186-189 and :308-319, fed one pass's max |err| at a time.
struct LoopControl {
    enum Verdict { CONTINUE, CONVERGED, NOT_CONVERGED };
    double thresh;
    int max_n_iter;
    int it = 1;                        // :188
    double *hist = nullptr;            // max |err| of pass 1, 2, ...: the first hist_len of them (null: not kept)
    int hist_len = 0;
    Verdict record(double err) {
        if (hist && it - 1 < hist_len) hist[it - 1] = err;
        it += 1;                                               // :313
        if (it > max_n_iter) return NOT_CONVERGED;             // :315-319: raised even when this pass met the threshold
        return !(err > thresh) ? CONVERGED : CONTINUE;         // :189  (NaN stops the loop too)
    }
    int n_iter() const { return it - 1; }                      // passes recorded
    int allowed() const { return max_n_iter - (it - 1); }      // passes it .. max_n_iter may still run
};

// Passes of the next launch of the multi-pass kernel.  The first launch carries the caller's guess (PGW_OPT_LOOP_GUESS;
// <= 0 counts as 1), a continuation launch 2; never more than the stopping rule still allows, never fewer than 1.
inline int launch_passes(bool first, int guess, int max_n_iter, int allowed) {
    int np = 2;
    if (first) {
        np = guess > LOOP_MAX_PASS ? LOOP_MAX_PASS : guess;
        if (np > max_n_iter) np = max_n_iter;
        if (np < 1) np = 1;
    }
    if (np > allowed) np = allowed;
    return np < 1 ? 1 : np;
}

// Who writes the final PS and QV once the loop has stopped.  The last pass of a launch of the multi-pass kernel may store the
// QV it forms below p_ref (PGW_OPT_QV_FROM_PASS), and with PGW_OPT_FINISH_IN_PASS it goes on to the first hybrid level and
// writes PS as well.  That is the file's result only when the very pass is the one whose max |err| met the threshold:
//   NOTHING      the storing pass finished its columns and is the converged one - no launch after the loop;
//   ABOVE_MARKS  it is the converged one but stopped where its scan stopped - the finalize kernel does the levels above;
//   ALL_LEVELS   every other stop - convergence in an earlier pass of the launch or in a pass that did not store, a finished
//                pass chosen on a NaN maximum (no valid column) - the finalize kernel runs over all levels and overwrites
//                what was speculated.
// Out of passes (NOT_CONVERGED) is the reference's error: nothing is finalized then, the caller returns it.
struct StoredPass {
    enum Final { NOTHING, ABOVE_MARKS, ALL_LEVELS };
    int k = -1;                        // index, within the launch being read back, of the pass that stored (-1: none did)
    bool finished = false;             // ... and walked on to the first hybrid level, PS written
    bool converged = false;            // the stopping rule chose that pass
    bool nan_stop = false;             // ... on a NaN maximum
    void launched(int k_, bool finished_) { k = k_; finished = k_ >= 0 && finished_; converged = nan_stop = false; }
    // pass `pass_k` of the launch got `verdict` from LoopControl::record(err)
    void decided(LoopControl::Verdict verdict, int pass_k, double err) {
        converged = verdict == LoopControl::CONVERGED && pass_k == k;
        nan_stop = err != err;
    }
    Final final_step() const {
        if (!converged) return ALL_LEVELS;
        if (!finished) return ABOVE_MARKS;
        return nan_stop ? ALL_LEVELS : NOTHING;
    }
};

// What the bands of a file exchange per launch (pgw_set_reduce_hook: element-wise MAX over the ranks):
// [status of the kernels before the loop | per pass: status, any-valid flag, max |err| (-inf: no valid column)].
struct BandVector {
    double v[1 + 3 * LOOP_MAX_PASS];
    static int length(int np) { return 1 + 3 * np; }
    void set_pre(int code) { v[0] = (double)code; }
    void set(int k, int code, bool valid, double max) { v[1 + 3 * k] = (double)code; v[2 + 3 * k] = valid ? 1.0 : 0.0; v[3 + 3 * k] = max; }
    int pre() const { return (int)v[0]; }
    int code(int k) const { return (int)v[1 + 3 * k]; }
    double err(int k) const { return v[2 + 3 * k] != 0.0 ? v[3 + 3 * k] : NAN; }   // NaN: xarray .max() of an all-NaN field
    void blank(int np) {               // a band with nothing to report: no status, no valid column
        set_pre(0);
        for (int k = 0; k < np; ++k) set(k, 0, false, -INFINITY);
    }
};

}  // namespace pgw
