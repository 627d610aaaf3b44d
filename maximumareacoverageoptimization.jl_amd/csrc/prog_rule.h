// prog_rule.h — steps 3-7 of the progressive-barrier rule (DESIGN.md section 4 "Progressive barrier")
// as a record any subset of an iteration's candidates can compute alone and that merges exactly: host
// and device, no HIP runtime calls (the host compiler builds it as it is: tests/host/prog_rule_check.cpp).
//
// Candidate k of centre c has the global index g = c K + k. A candidate the chain did not evaluate
// carries the objective +inf; a NaN objective is counted as evaluated and selects nothing
// (prog_select_kernel, k_prog.h). Whatever the outcome, the new infeasible incumbent is chosen among
// the infeasible candidates with h <= h_new, and h_new is known before the poll except in the improving
// case, where it is max{h_y : h_y < I.h}: the set {y : h_y <= h_new} is then {y : h_y < I.h}, which does
// not depend on the maximum either. So a subset reports the minimum of (f, h, g) over both sets (keep:
// h <= I.h, or h <= h_max without an I; drop: h < I.h) beside the facts that decide the outcome, and the
// finish step picks one. Every field is a count, an OR, or a minimum / maximum under a total order with
// ties to the lower g: the merged record depends neither on the partition nor on the merge order.
#pragma once

#include <stdint.h>

#include "predicate.h"   // MAC_HD

#pragma clang fp contract(off)

namespace mac {

// The 64-byte record of an iteration's steps 3-7 (prog_select_kernel writes it; prog_finish returns it).
struct ProgRec {
    int64_t outcome;      // 0 dominating, 1 improving, 2 unsuccessful; bit 8: bestF replaces F
    double bestF_f;       // the best feasible candidate (bestF_g < 0: none)
    int64_t bestF_g;
    double newI_f;        // the new infeasible incumbent (newI_g = -1: none, -2: the old one)
    double newI_h;
    int64_t newI_g;
    double h_new;
    int64_t evaluated;    // candidates with an objective other than +inf
};
static_assert(sizeof(ProgRec) == 64, "one 64-byte record");

constexpr int64_t kProgNone = -1, kProgOld = -2;
constexpr int64_t kProgTagDone = (int64_t)1 << 62;   // ProgPart.tag: the loop ends at this iteration

MAC_HD bool prog_less2(double f, int64_t g, double f2, int64_t g2)
{
    return g >= 0 && (g2 < 0 || f < f2 || (f == f2 && g < g2));
}

MAC_HD bool prog_less3(double f, double h, int64_t g, double f2, double h2, int64_t g2)
{
    return g >= 0 && (g2 < 0 || f < f2 || (f == f2 && (h < h2 || (h == h2 && g < g2))));
}

// What every rank knows before the poll: the incumbents' values and the threshold.
struct ProgScalars {
    int32_t has_F, has_I;
    double F_f, I_f, I_h, h_max;
};

// The shard-partial record (include/maxcover.h mac_prog_part: the same 96 bytes).
struct ProgPart {
    int64_t tag;          // the 1-based iteration the record belongs to; bit 62: done
    int64_t evaluated;    // objectives other than +inf                                         (sum)
    double bestF_f;       // min (f, g) over h == 0 (bestF_g < 0: none)                         (prog_less2)
    int64_t bestF_g;
    int64_t dominates;    // an infeasible y with h <= I.h, f <= I.f, one strict (has_I only)   (OR)
    double h_below;       // max h over the infeasible y with h < I.h (has_I only; -1.0: none)  (max)
    double keep_f;        // min (f, h, g) over the infeasible y with h <= (has_I ? I.h : h_max) (prog_less3)
    double keep_h;
    int64_t keep_g;
    double drop_f;        // min (f, h, g) over the infeasible y with h < I.h (has_I only)      (prog_less3)
    double drop_h;
    int64_t drop_g;
};
static_assert(sizeof(ProgPart) == 96, "one 96-byte record");

MAC_HD ProgPart prog_part_empty(int64_t tag)
{
    const double inf = __builtin_inf();
    return ProgPart{tag, 0, inf, -1, 0, -1.0, inf, inf, -1, inf, inf, -1};
}

// One candidate (f, h) with the global index g >= 0 into the record.
MAC_HD void prog_part_fold(ProgPart& p, const ProgScalars& s, double f, double h, int64_t g)
{
    if (f == __builtin_inf()) return;   // not evaluated
    ++p.evaluated;
    if (f != f) return;
    if (h == 0.0) {
        if (prog_less2(f, g, p.bestF_f, p.bestF_g)) {
            p.bestF_f = f;
            p.bestF_g = g;
        }
    } else if (h > 0.0) {
        if (s.has_I) {
            p.dominates |= (h <= s.I_h && f <= s.I_f && (h < s.I_h || f < s.I_f)) ? 1 : 0;
            if (h < s.I_h) {
                if (h > p.h_below) p.h_below = h;
                if (prog_less3(f, h, g, p.drop_f, p.drop_h, p.drop_g)) {
                    p.drop_f = f;
                    p.drop_h = h;
                    p.drop_g = g;
                }
            }
        }
        if (h <= (s.has_I ? s.I_h : s.h_max) && prog_less3(f, h, g, p.keep_f, p.keep_h, p.keep_g)) {
            p.keep_f = f;
            p.keep_h = h;
            p.keep_g = g;
        }
    }
}

// a <- a merged with b (the tag stays a's: the callers compare tags)
MAC_HD void prog_part_merge(ProgPart& a, const ProgPart& b)
{
    a.evaluated += b.evaluated;
    if (prog_less2(b.bestF_f, b.bestF_g, a.bestF_f, a.bestF_g)) {
        a.bestF_f = b.bestF_f;
        a.bestF_g = b.bestF_g;
    }
    a.dominates |= b.dominates;
    a.h_below = b.h_below > a.h_below ? b.h_below : a.h_below;
    if (prog_less3(b.keep_f, b.keep_h, b.keep_g, a.keep_f, a.keep_h, a.keep_g)) {
        a.keep_f = b.keep_f;
        a.keep_h = b.keep_h;
        a.keep_g = b.keep_g;
    }
    if (prog_less3(b.drop_f, b.drop_h, b.drop_g, a.drop_f, a.drop_h, a.drop_g)) {
        a.drop_f = b.drop_f;
        a.drop_h = b.drop_h;
        a.drop_g = b.drop_g;
    }
}

// The iteration's record from the merged one: prog_select_kernel's, field for field.
MAC_HD ProgRec prog_finish(const ProgPart& p, const ProgScalars& s)
{
    const bool improves = p.bestF_g >= 0 && (!s.has_F || p.bestF_f < s.F_f);
    const bool dominating = improves || p.dominates != 0;
    const bool improving = !dominating && s.has_I && p.h_below > 0.0;
    const double h_new = improving ? p.h_below : (s.has_I ? s.I_h : s.h_max);
    double nf = improving ? p.drop_f : p.keep_f;
    double nh = improving ? p.drop_h : p.keep_h;
    int64_t ng = improving ? p.drop_g : p.keep_g;
    // the old I stays in the running when I.h <= h_new, and sorts before a candidate on a full tie
    if (s.has_I && s.I_h <= h_new && !(ng >= 0 && (nf < s.I_f || (nf == s.I_f && nh < s.I_h)))) {
        nf = s.I_f;
        nh = s.I_h;
        ng = kProgOld;
    }
    ProgRec r;
    r.outcome = (dominating ? 0 : improving ? 1 : 2) | (improves ? 256 : 0);
    r.bestF_f = p.bestF_f;
    r.bestF_g = p.bestF_g;
    r.newI_f = nf;
    r.newI_h = nh;
    r.newI_g = ng;
    r.h_new = h_new;
    r.evaluated = p.evaluated;
    return r;
}

// Whether the iteration was unsuccessful and left I as it was (no I before and none after counts): the
// next iteration's poll is then known beforehand — the same centres, ell - 1, the threshold I.h (h_max
// without an I) — which is what a rank polling ahead assumes.
MAC_HD bool prog_chains(const ProgRec& r, bool has_I)
{
    return (r.outcome & 255) == 2 && (r.newI_g == kProgOld || (!has_I && r.newI_g == kProgNone));
}

}  // namespace mac
