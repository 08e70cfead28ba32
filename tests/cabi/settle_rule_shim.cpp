// Test-only C shim over ransac_with_homography_amd/csrc/rwh_settle.h (the native settle rule of rwh_ransac_run): the GPU work is
// two C callbacks, so tests/test_settle_rule_cpu.py can drive the very rule the library runs with synthetic tables through ctypes.
// Built by the test with g++ into its temporary directory; not part of librwh_hip.so.
#include <cstdint>

#include "rwh_settle.h"

extern "C" {

typedef int (*settle_shim_interval_fn)(const int* rows, int n, int* lo, int* hi, void* user);
typedef int (*settle_shim_settle_fn)(const int* rows, int n, int* cnt, void* user);

// k hypotheses: flags [k] (K1's), counts [k] (K2's raw counts).  Like rwh_ransac_run, the RWH_HYP_REPEATED rows are settled first
// (what the library does while the search runs), then rwh_settle::decide.  out [5]: winner, early, count, rounds, n_iv;
// slot [k]: settle order of every hypothesis (-1 = not settled).  Returns decide's status (a callback's nonzero status).
int settle_rule_run(int k, const uint8_t* flags, const int* counts, int need, int use_iv, int margin_cap,
                    settle_shim_interval_fn interval, settle_shim_settle_fn settle, void* user, int* out, int* slot) {
    rwh_settle::State st;
    st.pos.assign((size_t)k, -1);
    st.cnt.assign(counts, counts + k);
    std::vector<int> rows((size_t)k > 0 ? (size_t)k : 1);
    int n_rep = 0;
    for (int i = 0; i < k; ++i)
        if (flags[i] & RWH_HYP_REPEATED) rows[(size_t)n_rep++] = i;
    if (n_rep) {
        const int r = settle(rows.data(), n_rep, st.cnt.data(), user);
        if (r != 0) return r;
        for (int j = 0; j < n_rep; ++j) st.pos[(size_t)rows[(size_t)j]] = j;
        st.nset = n_rep;
    }
    rwh_settle::Outcome o;
    const int r = rwh_settle::decide(
        k, flags, need, use_iv != 0, margin_cap, rows.data(), st,
        [&](const int* rw, int n, int* lo, int* hi) { return interval(rw, n, lo, hi, user); },
        [&](const int* rw, int n, int* cnt) { return settle(rw, n, cnt, user); }, o);
    out[0] = o.winner; out[1] = o.early; out[2] = o.count; out[3] = o.rounds; out[4] = o.n_iv;
    for (int i = 0; i < k; ++i) slot[i] = st.pos[(size_t)i];
    return r;
}

}  // extern "C"
