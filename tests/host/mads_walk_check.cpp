// Host check of the native MADS driver's arithmetic (csrc/mads_walk.h) against a run of the Python
// stepper (TDM_STATIC_opt.PollStepper) recorded by tests/test_mads_walk_host.py: the stream's states,
// every iteration's permutations (and those drawn ahead), the point a chosen candidate moves the
// incumbent to and the acceptance rule, replayed from the recorded poll outcomes and compared byte for
// byte. Prints the counts and exits 0, or prints the first difference and exits 1 (2: a bad file).
// Built with g++ -ffp-contract=off; no GPU.
//
// The file, 8-byte words unless noted: n, n_p, has_g, ell0, ell_max, seed, records; x0[n], f0, g[n] (if
// has_g); per record: probes, per probe {ahead, rp[n_p], cp[n_p] (int32)} (the first has ahead = 0),
// best_obj, best_idx, then the state after the update: x[n], f, ell, stream state; at the end the
// successes and the iterations.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mads_walk.h"

namespace {

FILE* g_in = nullptr;

template <class T> void get(T* p, size_t count)
{
    if (std::fread(p, sizeof(T), count, g_in) != count) {
        std::printf("short file\n");
        std::exit(2);
    }
}
template <class T> T get()
{
    T v;
    get(&v, 1);
    return v;
}

[[noreturn]] void differ(int64_t rec, const char* what)
{
    std::printf("record %lld: %s differs\n", (long long)rec, what);
    std::exit(1);
}

template <class T> bool same(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2 || !(g_in = std::fopen(argv[1], "rb"))) {
        std::printf("usage: mads_walk_check <recorded run>\n");
        return 2;
    }
    const int64_t n = get<int64_t>(), n_p = get<int64_t>(), has_g = get<int64_t>();
    int ell = (int)get<int64_t>();
    const int ell_max = (int)get<int64_t>();
    mac::MadsStream stream{get<uint64_t>(), (int)n_p};
    const int64_t records = get<int64_t>();
    if (n < 1 || n_p < 1 || n_p > n || n > (1 << 20) || records < 0) return 2;
    std::vector<double> x(n), g(has_g ? n : 0), want_x(n), cand(n);
    get(x.data(), x.size());
    double f = get<double>();
    get(g.data(), g.size());
    int64_t succ = 0, it = 0, perms = 0;
    std::vector<int> rp, cp, rp0, cp0, want_rp(n_p), want_cp(n_p);
    for (int64_t rec = 0; rec < records; ++rec) {
        if (ell < 0) differ(rec, "the run's end (ell < 0)");
        const int64_t probes = get<int64_t>();
        for (int64_t q = 0; q < probes; ++q) {
            const int64_t ahead = get<int64_t>();
            get(want_rp.data(), want_rp.size());
            get(want_cp.data(), want_cp.size());
            if ((q == 0) != (ahead == 0)) return 2;
            stream.draw(stream.state_after((uint64_t)ahead), rp, cp);
            if (!same(rp, want_rp)) differ(rec, "rp");
            if (!same(cp, want_cp)) differ(rec, "cp");
            perms += 2;
            if (q == 0) {
                rp0 = rp;
                cp0 = cp;
            }
        }
        if (probes < 1) return 2;
        const double best_obj = get<double>();
        const int64_t best_idx = get<int64_t>();
        if (best_idx >= 2 * n_p) return 2;
        const mac::MadsPoll poll{stream.state, (int)n_p, (int64_t)1 << ell, rp0.data(), cp0.data(),
                                 has_g ? g.data() : nullptr};
        if (best_idx >= 0) mac::mads_candidate(poll, best_idx, x.data(), (int)n, cand.data());   // (out of place)
        const bool moved = mac::mads_accept(poll, best_obj, best_idx, ell_max, x.data(), (int)n, f, ell, succ);
        stream.advance();
        ++it;
        get(want_x.data(), want_x.size());
        const double want_f = get<double>();
        const int64_t want_ell = get<int64_t>();
        const uint64_t want_state = get<uint64_t>();
        if (!same(x, want_x)) differ(rec, "the incumbent");
        if (moved && !same(cand, x)) differ(rec, "the candidate written out of place");
        if (std::memcmp(&f, &want_f, sizeof f) != 0) differ(rec, "f");
        if (ell != want_ell) differ(rec, "ell");
        if (stream.state != want_state) differ(rec, "the stream state");
    }
    if (succ != get<int64_t>()) differ(records, "the successes");
    if (it != get<int64_t>()) differ(records, "the iterations");
    std::fclose(g_in);
    std::printf("records %lld permutations %lld successes %lld: ok\n", (long long)records, (long long)perms,
                (long long)succ);
    return 0;
}
