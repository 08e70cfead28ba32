// rwh_settle.h: the DECISION part of the settle step of rwh_ransac_run (csrc/rwh_run.hip) -- which hypotheses get the reference's own
// solver, in which rounds, and the accept rules over the result.  Host-only C++17 (no HIP include, no HIP type): the GPU work comes in
// through two callables.  rwh_ransac_run calls `decide` directly; rwh_settle_decide (csrc/rwh_run.hip) exports it with C callbacks
// for ransac._settle_on_host (the step-by-step Python driver, the batched and sharded forms) and for the CPU suite
// (tests/test_settle_rule_cpu.py, on synthetic tables).  This file is the only place the rule is written.
//
// THE MODEL the 'fwd' interval rule is entitled to assume -- and all it assumes (stated in include/rwh.h and DESIGN.md too):
//   * a hypothesis without an always-bit (RWH_HYP_REPEATED / SINGULAR / DEGENERATE) has its reference count inside its count
//     interval [lo, hi] from rwh_score_interval, and K2's raw count is inside it too;
//   * an UNFLAGGED hypothesis (flags == 0) has its reference count within IV_NEAR / 2 of K2's raw count: what lets every unflagged
//     hypothesis more than IV_NEAR below min(best0, need) go without an interval (best0 = the best raw count of an UNFLAGGED
//     hypothesis; a non-candidate's reference count is then below best0's reference count and below `need`);
//   * an RWH_HYP_ILLCOND hypothesis's reference count is bounded only by its interval (its raw count places nothing);
//   * an always-bit hypothesis carries no information: it is always settled.
// Under the model the rule returns the reference's winner, early-exit flag and count (the accept rules of ransac.py:186-202 on the
// reference's counts of all k hypotheses), and the winner is either settled or has a point interval (lo == hi: K2's count and mask
// are the reference's).  'backward' / 'reproj' (use_iv false) keep the margin rule of rounds 2-3: every flagged hypothesis and every
// unflagged one within margin_of(best) of the best trustworthy count or within margin_of(need) of `need` is settled.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "rwh.h"

namespace rwh_settle {

static constexpr int IV_NEAR = 32;

// Margin around a decision count: min(cap, 3 + best / 16).  It shrinks with the count (a count of 17 cannot move by 8) and grows by
// at most 1 per 16 counts, so best - margin_of(best) is nondecreasing: a hypothesis inside the margin of a larger best is inside the
// margin of every smaller one -- what lets each shard of a sharded search settle on its own (sharded.gpu_score_slice).
inline int margin_of(int best, int cap) { const int v = 3 + (best > 0 ? best : 0) / 16; return v < cap ? v : cap; }

// The coordinate scale of rwh_score_interval's budget: the largest |entry| of pts_a (m x 2), at least 1; NaN if an entry is NaN.
inline double coord_scale(const float* pts_a, int m) {
    double c = 1.0;
    for (long long i = 0; i < 2ll * m; ++i) {
        const double v = pts_a[i] < 0 ? -(double)pts_a[i] : (double)pts_a[i];
        if (v != v) return v;
        if (v > c) c = v;
    }
    return c;
}

// Whether the 'fwd' interval rule may run at this scale: an Inf / NaN coordinate takes the margin rule (NaN < 1e30 is false).
inline bool intervals_usable(double coord_scale) { return coord_scale < 1e30; }

struct Outcome {
    int winner = -1, early = 0, count = 0;   // accept rules over the prefix the reference looks at; winner -1: no count above 0
    int rounds = 0, n_iv = 0;                // settle rounds run here, hypotheses given an interval
};

// Per-call state, owned by the caller (the library keeps it thread_local: its pages survive between calls).
//   cnt [k]: K2's raw counts in; a settled hypothesis's entry holds the reference's count (in and out)
//   pos [k]: slot of each settled hypothesis in the caller's tables, -1 = not settled (in and out); nset: slots in use (in and out)
//   lo, hi, act: scratch
struct State {
    std::vector<int> pos, cnt, lo, hi, act;
    int nset = 0;
};

// k hypotheses with K1's flags; rows: scratch of k ints handed to the callables (the library passes page-locked memory).
//   interval(const int* rows, int n, int* lo, int* hi) -> status: [lo, hi] of every listed row, written at lo[row], hi[row];
//   settle(const int* rows, int n, int* cnt) -> status: the reference's count of every listed row, written at cnt[row]; the rows
//     take slots st.nset .. st.nset + n - 1 (assigned here once the call returned 0).
// A nonzero status from a callable is returned as it is, with the state as far as it got.
template <class IntervalFn, class SettleFn>
int decide(int k, const uint8_t* flags, int need, bool use_iv, int margin_cap, int* rows, State& st, IntervalFn&& interval,
           SettleFn&& settle, Outcome& out) {
    out = Outcome();
    std::vector<int>&pos = st.pos, &cnt = st.cnt, &lo = st.lo, &hi = st.hi, &act = st.act;
    auto absorb = [&](int n_rows) {
        for (int j = 0; j < n_rows; ++j) pos[(size_t)rows[j]] = st.nset + j;
        st.nset += n_rows;
    };
    const unsigned always_bits = use_iv ? (RWH_HYP_REPEATED | RWH_HYP_SINGULAR | RWH_HYP_DEGENERATE) : 0xFFu;
    int end = k, st_ = 0;
    if (use_iv) {
        // ---- candidates: every RWH_HYP_ILLCOND sample that is not degenerate, every other hypothesis within IV_NEAR of best0 or
        // `need`; the others keep lo = hi = their raw count
        lo.assign(cnt.begin(), cnt.begin() + k);
        hi.assign(cnt.begin(), cnt.begin() + k);
        int best0 = 0;                  // over UNFLAGGED rows only: an RWH_HYP_ILLCOND raw count places nothing (a lower best0 only widens)
        for (int i = 0; i < k; ++i)
            if (flags[i] == 0 && cnt[(size_t)i] > best0) best0 = cnt[(size_t)i];
        const int near_lim = (best0 < need ? best0 : need) - IV_NEAR;      // cnt >= best0 - NEAR or cnt >= need - NEAR
        int n_iv = 0;
        for (int i = 0; i < k; ++i) {
            const unsigned f = flags[i];
            if (!(f & always_bits) && ((f & RWH_HYP_ILLCOND) || cnt[(size_t)i] >= near_lim) && pos[(size_t)i] < 0) rows[n_iv++] = i;
        }
        out.n_iv = n_iv;
        if (n_iv && (st_ = interval(static_cast<const int*>(rows), n_iv, lo.data(), hi.data())) != 0) return st_;

        // ---- rounds, active-list form: only a hypothesis that is not settled and either carries an always-bit or has an open
        // interval (lo < hi) can ever be taken: the ACTIVE list, a few thousand of 100 000.  Every other one is fixed for the whole
        // call: v[] = what it contributes to the running best (lo; 0 for an unsettled always-bit sample; the settled count once
        // settled -- kept in lo[]), `fs` = the first hypothesis that certainly exits.
        act.clear();
        int fs = k;
        for (int i = k - 1; i >= 0; --i) {
            const bool settled = pos[(size_t)i] >= 0, always = (flags[i] & always_bits) != 0;
            int v;
            if (settled) v = cnt[(size_t)i];
            else if (always) v = 0;
            else v = lo[(size_t)i];
            if ((settled || !always) && v >= need) fs = i;
            if (!settled && (always || lo[(size_t)i] < hi[(size_t)i])) act.push_back(i);
            lo[(size_t)i] = v;                                  // from here on lo[] is v[]
        }
        std::reverse(act.begin(), act.end());                   // ascending, like the margin rule's rows
        for (;;) {
            end = fs < k ? fs + 1 : k;
            int best = 0;
            for (int i = 0; i < end; ++i) best = lo[(size_t)i] > best ? lo[(size_t)i] : best;
            int n_rows = 0;
            size_t keep = 0;
            for (size_t a = 0; a < act.size(); ++a) {
                const int i = act[a];
                const bool take = i < end && ((flags[i] & always_bits) || hi[(size_t)i] >= best || hi[(size_t)i] >= need);
                if (take) rows[n_rows++] = i; else act[keep++] = i;
            }
            act.resize(keep);
            if (n_rows == 0) break;
            ++out.rounds;
            if ((st_ = settle(static_cast<const int*>(rows), n_rows, cnt.data())) != 0) return st_;
            absorb(n_rows);
            bool fs_lost = false;
            for (int j = 0; j < n_rows; ++j) {
                const int i = rows[j], c = cnt[(size_t)i];
                lo[(size_t)i] = c;
                fs_lost |= i == fs && c < need;
            }
            if (fs_lost) {                                      // (only when a count left its interval) the next sure exit after it
                int f = fs + 1;
                while (f < k && !((pos[(size_t)f] >= 0 || !(flags[f] & always_bits)) && lo[(size_t)f] >= need)) ++f;
                fs = f;
            }
            for (int j = 0; j < n_rows; ++j)
                if (cnt[(size_t)rows[j]] >= need && rows[j] < fs) fs = rows[j];
        }
    } else {
        // ---- the margin rule (rounds 2-3): `best` = a lower bound of the best count the reference sees in the prefix
        for (;;) {
            end = k;
            const int m_need = margin_of(need, margin_cap);
            for (int i = 0; i < k; ++i) {
                const bool sure = pos[(size_t)i] >= 0 ? cnt[(size_t)i] >= need : flags[i] == 0 && cnt[(size_t)i] >= need + m_need;
                if (sure) { end = i + 1; break; }
            }
            int best = 0;
            for (int i = 0; i < end; ++i) {
                const int v = pos[(size_t)i] >= 0 || flags[i] == 0 ? cnt[(size_t)i] : 0;
                if (v > best) best = v;
            }
            const int m_best = margin_of(best, margin_cap);
            int n_rows = 0;
            for (int i = 0; i < end; ++i) {
                if (pos[(size_t)i] >= 0) continue;
                if (flags[i] != 0 || cnt[(size_t)i] >= best - m_best || cnt[(size_t)i] >= need - m_need) rows[n_rows++] = i;
            }
            if (n_rows == 0) break;
            ++out.rounds;
            if ((st_ = settle(static_cast<const int*>(rows), n_rows, cnt.data())) != 0) return st_;
            absorb(n_rows);
        }
    }

    // ---- the accept rules (ransac.py:186-202) over the prefix the reference looks at ------------------------------------
    for (int i = 0; i < end; ++i)
        if (cnt[(size_t)i] >= need) { out.winner = i; out.early = 1; break; }
    if (out.winner < 0) {
        int bestc = 0;
        for (int i = 0; i < end; ++i)
            if (cnt[(size_t)i] > bestc) { bestc = cnt[(size_t)i]; out.winner = i; }    // strict >: the first index of the maximum
    }
    out.count = out.winner >= 0 ? cnt[(size_t)out.winner] : 0;
    return 0;
}

}  // namespace rwh_settle
