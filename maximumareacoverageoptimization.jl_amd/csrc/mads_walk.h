// mads_walk.h — the native MADS driver's arithmetic with no HIP runtime in it, shared by host and
// device code: the splitmix64 stream and the LTMADS entries the poll chains inline (k_prep.h CandSrc),
// and the host's side of a run (mads_driver.h): where an iteration's draws sit in the stream, its two
// permutations, the point a chosen candidate moves the incumbent to, and the acceptance rule. Builds
// with the host compiler alone for the CPU test (tests/test_mads_walk_host.py).
#pragma once

#include <stdint.h>

#include <vector>

#include "predicate.h"

#pragma clang fp contract(off)

namespace mac {

// splitmix64 stream value number `idx` (1-based) after `state` (workloads.SplitMix64).
MAC_HD uint64_t splitmix_at(uint64_t state, uint64_t idx)
{
    uint64_t z = state + idx * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

MAC_HD double splitmix_uniform_at(uint64_t state, uint64_t idx)
{
    return (double)(splitmix_at(state, idx) >> 11) * (1.0 / 9007199254740992.0);
}

// Entry (r, c) of the lower-triangular LTMADS matrix L drawn from the stream at `state`
// (workloads.ltmads_basis): diagonal sign(u_{r+1} < 0.5 ? -1 : 1) * 2^ell; strictly lower
// entries uniform integers in [-(2^ell - 1), 2^ell - 1] from stream values n + 1 + r(r-1)/2 + c
// (numpy's tril_indices order); zero above the diagonal.
MAC_HD double ltmads_entry(uint64_t state, int64_t n, int64_t b, int64_t r, int64_t c)
{
    if (r < c) return 0.0;
    if (r == c) return (splitmix_uniform_at(state, (uint64_t)r + 1) < 0.5 ? -1.0 : 1.0) * (double)b;
    const int64_t lo = -b + 1, span = 2 * b - 1;
    const double u = splitmix_uniform_at(state, (uint64_t)(n + 1 + r * (r - 1) / 2 + c));
    return (double)(lo + (int64_t)__builtin_floor(u * (double)span));
}

// Stable argsort of the next n stream values after stream position `first` - 1 (numpy
// argsort(kind="stable") of SplitMix64.next_u64(n)).
static inline void stream_permutation(uint64_t state, uint64_t first, int n, std::vector<int>& out)
{
    // A stable argsort of the keys, i.e. the order of the (key, index) pairs: bucketed by the
    // keys' top bits (uniform keys: O(n)), then insertion-sorted inside each bucket.
    int bits = 1;
    while ((1 << bits) < n && bits < 20) ++bits;
    const int nb = 1 << bits;
    std::vector<uint64_t> keys(n);
    std::vector<int> start(nb + 1, 0);
    for (int q = 0; q < n; ++q) {
        keys[q] = splitmix_at(state, first + (uint64_t)q);
        ++start[(keys[q] >> (64 - bits)) + 1];
    }
    for (int b = 0; b < nb; ++b) start[b + 1] += start[b];
    out.assign(n, 0);
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int q = 0; q < n; ++q) out[fill[keys[q] >> (64 - bits)]++] = q;  // ascending q per bucket
    for (int b = 0; b < nb; ++b) {
        for (int a = start[b] + 1; a < start[b + 1]; ++a) {
            const int v = out[a];
            int c = a - 1;
            while (c >= start[b] && keys[out[c]] > keys[v]) {  // strict: equal keys keep q order
                out[c + 1] = out[c];
                --c;
            }
            out[c + 1] = v;
        }
    }
}

// The stream of a run over n_p polled variables. An iteration takes ltmads_basis(n_p)'s draws after
// `state`: n_p diagonal signs, T strictly lower entries, then the keys of the row and of the column
// permutation, n_p each. The permutations do not depend on the poll's outcome, so any iteration's can
// be drawn ahead of time from its state alone.
struct MadsStream {
    uint64_t state = 0;   // the current iteration's
    int n_p = 0;
    uint64_t T() const { return (uint64_t)n_p * (uint64_t)(n_p - 1) / 2; }
    uint64_t per_iter() const { return (uint64_t)n_p + T() + 2 * (uint64_t)n_p; }
    uint64_t state_after(uint64_t k) const { return state + k * per_iter() * 0x9E3779B97F4A7C15ull; }
    void advance() { state = state_after(1); }
    // the permutations (rp, cp) of the iteration whose state is `at`
    void draw(uint64_t at, std::vector<int>& rp, std::vector<int>& cp) const
    {
        stream_permutation(at, (uint64_t)n_p + T() + 1, n_p, rp);
        stream_permutation(at, (uint64_t)n_p + T() + (uint64_t)n_p + 1, n_p, cp);
    }
};

// One poll of a run: the iteration's stream state, the mesh step b = 2^ell, the permutations (n_p
// each) and the mesh's granularity per variable (null: none). Candidate k < n_p is the centre plus
// column k of B = L[rp][:, cp], candidate k >= n_p the centre minus column k - n_p.
struct MadsPoll {
    uint64_t state;
    int n_p;
    int64_t b;
    const int* rp;
    const int* cp;
    const double* g;
};

// Candidate k of the poll p around the centre x (n doubles, the first n_p polled) into out (n doubles;
// out may be x itself). Variable v steps by the entry d, on a mesh by the one product g[v] * d (without
// a mesh d itself, not 1.0 * d: the device's CandSrc::step_m); the held variables are x's doubles copied.
static inline void mads_candidate(const MadsPoll& p, int64_t k, const double* x, int n, double* out)
{
    const bool plus = k < p.n_p;
    const int kk = plus ? (int)k : (int)k - p.n_p;
    for (int v = 0; v < p.n_p; ++v) {
        double d = ltmads_entry(p.state, p.n_p, p.b, p.rp[v], p.cp[kk]);
        if (p.g) d = p.g[v] * d;
        out[v] = plus ? x[v] + d : x[v] - d;
    }
    for (int v = p.n_p; v < n; ++v) out[v] = x[v];
}

// The plain acceptance rule on the poll's best (objective, index; index < 0: nothing feasible). A
// strictly better objective moves the incumbent x to that candidate and refines towards larger
// steps; anything else shrinks the mesh (ell < 0 ends the run). Returns whether x moved.
static inline bool mads_accept(const MadsPoll& p, double best_obj, int64_t best_idx, int ell_max, double* x, int n,
                               double& f, int& ell, int64_t& succ)
{
    if (best_idx >= 0 && best_obj < f) {
        mads_candidate(p, best_idx, x, n, x);
        f = best_obj;
        ell = ell + 1 < ell_max ? ell + 1 : ell_max;
        ++succ;
        return true;
    }
    --ell;
    return false;
}

}  // namespace mac
