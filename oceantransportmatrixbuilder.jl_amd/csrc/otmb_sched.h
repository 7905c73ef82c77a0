// otmb_sched.h -- the schedule of a stepped cycle, host C++ alone (no HIP header: tests/test_schedule_header_host.py drives it from a
// stand-alone program): which slot step t takes and whether it blends, a blend's weights, the preconditioner blocks a call reserves, the
// cycle-mean's weights, what a failure's message says of its step, the lists of d and source blocks a step picks from, and what the
// scheduled calls refuse.  otmb_step.hip and otmb_periodic.hip hold no rule of their own.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

// The shift's diagonal part d: n values for every column (ld == 0, or p == null: none), or column c's own n values at p + c·ld (ld >= n):
// the per-column calls (otmb_op_*_dk).  percol: a column's preconditioner is its own.
struct SvD {
    const double *p;
    int64_t ld;
    bool percol() const { return p && ld != 0; }
};

// d as a list of blocks (otmb_op_*_season, include/otmb.h): nd = 0 (none), 1 (the block serves every step) or nslots (a block per slot), each
// n values (ldd == 0) or n x k (ldd >= n); D: a HOST array of nd pointers.  Every other call passes at most one block.
struct StD {
    int64_t nd;
    const double *const *D;
    int64_t ldd;
    SvD at(int64_t slot) const { return nd == 0 ? SvD{nullptr, 0} : SvD{D[nd == 1 ? 0 : slot], ldd}; }
    bool percol() const { return nd > 0 && ldd != 0 && D[0]; }
};

// The source blocks: a step on `slot` takes block at(slot) of nsrc (0: none; 1: block 0 on every step; nslots: the slot's), each n x k with
// the leading dimension lds; S: a HOST array of nsrc pointers; scale: nsteps·k HOST values (step t's source is s·scale[t·k + c]) or null.
struct StSrc {
    int64_t nsrc;
    const double *const *S;
    int64_t lds;
    const double *scale;
    const double *at(int64_t slot) const { return nsrc == 0 ? nullptr : S[nsrc == 1 ? 0 : slot]; }
};

// An explicit schedule (include/otmb.h): step t blends slots a[t] and b[t] with the weight w[t]; three HOST arrays.
struct StMix {
    const int64_t *a, *b;
    const double *w;
};
// What a schedule makes of step t: its slot when it is plain, or a blend (slot: the first of the two).
struct StStep {
    int64_t slot;
    bool blend;
};

// The schedule of a call: cyclic -- step t runs on slot (first_slot + t / substeps) mod nslots and never blends -- or explicit (listed): step
// t is plain on mix.a[t] (a == b or w == 0.0), plain on mix.b[t] (w == 1.0) or the blend (1 - w)·(slot a) + w·(slot b).
struct StSched {
    int64_t first_slot, substeps;
    bool listed;
    StMix mix;
    static StSched cyclic(int64_t first_slot, int64_t substeps) { return {first_slot, substeps, false, {nullptr, nullptr, nullptr}}; }
    static StSched list(const int64_t *a, const int64_t *b, const double *w) { return {0, 1, true, {a, b, w}}; }

    StStep at(int64_t t, int64_t nslots) const {
        if (!listed) return {(first_slot + t / substeps) % nslots, false};
        const int64_t a = mix.a[t], b = mix.b[t];
        const double w = mix.w[t];
        if (a == b || w == 0.0) return {a, false};
        if (w == 1.0) return {b, false};
        return {a, true};
    }
    // the weights of a blended step's two slots: wa = 1.0 - w for mix.a[t], wb = w for mix.b[t]
    void weights(int64_t t, double &wa, double &wb) const {
        wb = mix.w[t];
        wa = 1.0 - wb;
    }
    // the preconditioner blocks a call of nsteps steps keeps: one per distinct slot its plain steps visit, and one that every blended step
    // shares (blended: there is such a step)
    int64_t blocks(int64_t nsteps, int64_t nslots, bool &blended) const {
        std::vector<char> seen((size_t)nslots, 0);
        int64_t used = 0;
        blended = false;
        for (int64_t t = 0; t < nsteps; ++t) {
            const StStep s = at(t, nslots);
            if (s.blend)
                blended = true;
            else if (!seen[(size_t)s.slot]++)
                used += 1;
        }
        return used + (blended ? 1 : 0);
    }
    // The cycle-mean's weights, out[s] = acc_s / ncycle with acc over t ascending: a plain step adds 1.0 to its slot, a blended one wa to a,
    // then wb to b.  A cyclic schedule only ever adds 1.0, which is exact below 2^53: acc_s is the slot's visit count as a double, and the
    // quotient has the bits of (double)count / (double)ncycle.  A slot never visited gets +0.0.
    void mean_weights(int64_t ncycle, int64_t nslots, double *out) const {
        std::vector<double> acc((size_t)nslots, 0.0);
        for (int64_t t = 0; t < ncycle; ++t) {
            const StStep s = at(t, nslots);
            if (!s.blend) {
                acc[(size_t)s.slot] = acc[(size_t)s.slot] + 1.0;
            } else {
                double wa, wb;
                weights(t, wa, wb);
                acc[(size_t)mix.a[t]] = acc[(size_t)mix.a[t]] + wa;
                acc[(size_t)mix.b[t]] = acc[(size_t)mix.b[t]] + wb;
            }
        }
        for (int64_t s = 0; s < nslots; ++s) out[s] = acc[(size_t)s] / (double)ncycle;
    }
    // what a failure's message says of step t (slot: at(t).slot): the step and the slot(s) the schedule gave it
    std::string describe(int64_t t, int64_t slot) const {
        if (!listed) return " (step " + std::to_string(t) + ", slot " + std::to_string(slot) + ")";
        char w[40];
        snprintf(w, sizeof w, "%.17g", mix.w[t]);
        return " (step " + std::to_string(t) + ", slots " + std::to_string(mix.a[t]) + " and " + std::to_string(mix.b[t]) + ", weight " + w + ")";
    }
};

// sv_sched_complaint: the first complaint about a cyclic schedule's sub-steps and the source blocks of an operator of n rows and nslots
//                  slots, or null: what otmb_op_step_sched and otmb_op_periodic_sched add to the checks of the calls they extend.
static inline const char *sv_sched_complaint(int64_t n, int64_t nslots, int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds) {
    if (substeps < 1) return "substeps must be >= 1";
    if (nsrc != 0 && nsrc != 1 && nsrc != nslots) return "nsrc must be 0, 1 or the number of slots";
    if (nsrc > 0) {
        if (!S) return "S is null with nsrc > 0";
        for (int64_t j = 0; j < nsrc; ++j)
            if (!S[j]) return "a source block is null";
        if (lds < n) return "lds is smaller than the rows of S";
    }
    return nullptr;
}
// sv_interp_complaint: the same for an explicit schedule of `count` steps (otmb_op_*_interp, otmb_op_*_season): nsrc is 0 or 1 (per_slot: or
//                  the number of slots), then the complaints about the source above, then the three arrays -- none null, every slot one of
//                  the operator's, every weight finite and in [0, 1].  text: at least 160 chars of scratch for a message that names an entry.
static inline const char *sv_interp_complaint(int64_t n, int64_t nslots, int64_t count, const StMix &mix, int64_t nsrc, const double *const *S, int64_t lds,
                                              char *text, bool per_slot = false) {
    if (!per_slot && nsrc != 0 && nsrc != 1) return "nsrc must be 0 or 1 (a source per slot is not built with interpolation)";
    if (const char *more = sv_sched_complaint(n, nslots, 1, nsrc, S, lds)) return more;
    if (count > 0 && (!mix.a || !mix.b || !mix.w)) return "slot_a, slot_b or weight is null";
    for (int64_t t = 0; t < count; ++t) {
        for (const int64_t s : {mix.a[t], mix.b[t]})
            if (s < 0 || s >= nslots) {
                snprintf(text, 160, "step %lld: slot %lld is outside 0..%lld (otmb_op_set_slots)", (long long)t, (long long)s, (long long)nslots - 1);
                return text;
            }
        if (!std::isfinite(mix.w[t]) || mix.w[t] < 0.0 || mix.w[t] > 1.0) {
            snprintf(text, 160, "step %lld: the weight %g is not finite or outside [0, 1]", (long long)t, mix.w[t]);
            return text;
        }
    }
    return nullptr;
}
// sv_season_complaint: the first complaint about a list of d blocks, or null: what otmb_op_step_season and otmb_op_periodic_season add.
static inline const char *sv_season_complaint(int64_t n, int64_t nslots, int64_t nd, const double *const *D, int64_t ldd) {
    if (nd != 0 && nd != 1 && nd != nslots) return "nd must be 0, 1 or the number of slots";
    if (nd > 0) {
        if (!D) return "D is null with nd > 0";
        for (int64_t j = 0; j < nd; ++j)
            if (!D[j]) return "a d block is null";
        if (ldd != 0 && ldd < n) return "ldd must be 0 (the n values of a block serve every column) or >= n";
    }
    return nullptr;
}
