// prog_rule_check — csrc/prog_rule.h on the host compiler against a table of cases written by
// tests/test_prog_part_host.py: every case's candidates are folded shard by shard (prog_part_fold), the
// shard records merged in the order the file gives (prog_part_merge) and finished (prog_finish); the
// record must equal the expected ProgRec byte for byte. The merge is repeated in the reverse order and
// as a balanced tree, which must give the same 96 bytes.
//
// File (little endian, 8-byte words): n_cases; per case K, has_F, has_I, F_f, I_f, I_h, h_max, present[2],
// then per present centre K objectives and K h values, n_shards, per shard (lo, hi), the expected
// ProgRec (8 words), the expected chains flag.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "prog_rule.h"

using namespace mac;

static_assert(sizeof(ProgPart) == 96 && sizeof(ProgRec) == 64, "record sizes");

struct Reader {
    std::vector<unsigned char> buf;
    size_t at = 0;
    bool ok = true;
    template <class T> T get()
    {
        T v{};
        if (at + sizeof(T) > buf.size()) {
            ok = false;
            return v;
        }
        std::memcpy(&v, buf.data() + at, sizeof(T));
        at += sizeof(T);
        return v;
    }
    void doubles(std::vector<double>& out, size_t n)
    {
        out.assign(n, 0.0);
        if (at + 8 * n > buf.size()) {
            ok = false;
            return;
        }
        if (n) std::memcpy(out.data(), buf.data() + at, 8 * n);
        at += 8 * n;
    }
};

static ProgPart tree_merge(const std::vector<ProgPart>& v, size_t a, size_t b)
{
    if (b - a == 1) return v[a];
    const size_t mid = a + (b - a) / 2;
    ProgPart l = tree_merge(v, a, mid);
    const ProgPart r = tree_merge(v, mid, b);
    prog_part_merge(l, r);
    return l;
}

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: prog_rule_check FILE\n");
        return 2;
    }
    Reader rd;
    {
        FILE* fh = std::fopen(argv[1], "rb");
        if (!fh) {
            std::perror(argv[1]);
            return 2;
        }
        unsigned char tmp[1 << 16];
        size_t got;
        while ((got = std::fread(tmp, 1, sizeof tmp, fh)) > 0) rd.buf.insert(rd.buf.end(), tmp, tmp + got);
        std::fclose(fh);
    }
    // the empty record
    {
        const ProgPart e = prog_part_empty(7);
        const double inf = __builtin_inf();
        if (e.tag != 7 || e.evaluated != 0 || e.bestF_f != inf || e.bestF_g != -1 || e.dominates != 0 ||
            e.h_below != -1.0 || e.keep_f != inf || e.keep_h != inf || e.keep_g != -1 || e.drop_f != inf ||
            e.drop_h != inf || e.drop_g != -1) {
            std::printf("the empty record is not (0, +inf/-1, 0, -1.0, +inf/+inf/-1 twice)\n");
            return 1;
        }
    }
    const int64_t n_cases = rd.get<int64_t>();
    int64_t bad = 0, shards_total = 0;
    for (int64_t q = 0; q < n_cases && rd.ok; ++q) {
        const int64_t K = rd.get<int64_t>();
        ProgScalars sc{};
        sc.has_F = (int32_t)rd.get<int64_t>();
        sc.has_I = (int32_t)rd.get<int64_t>();
        sc.F_f = rd.get<double>();
        sc.I_f = rd.get<double>();
        sc.I_h = rd.get<double>();
        sc.h_max = rd.get<double>();
        int64_t present[2] = {rd.get<int64_t>(), 0};
        present[1] = rd.get<int64_t>();
        std::vector<double> obj[2], h[2];
        for (int c = 0; c < 2; ++c) {
            if (!present[c]) continue;
            rd.doubles(obj[c], (size_t)K);
            rd.doubles(h[c], (size_t)K);
        }
        const int64_t n_shards = rd.get<int64_t>();
        if (!rd.ok || n_shards < 1) break;
        std::vector<ProgPart> parts;
        for (int64_t s = 0; s < n_shards; ++s) {
            const int64_t lo = rd.get<int64_t>(), hi = rd.get<int64_t>();
            if (!rd.ok || lo < 0 || hi < lo || hi > K) {
                rd.ok = false;
                break;
            }
            ProgPart p = prog_part_empty(q + 1);
            for (int c = 0; c < 2; ++c) {
                if (!present[c]) continue;
                for (int64_t k = lo; k < hi; ++k) prog_part_fold(p, sc, obj[c][(size_t)k], h[c][(size_t)k], c * K + k);
            }
            parts.push_back(p);
        }
        ProgRec want;
        for (int w = 0; w < 8; ++w) {
            const int64_t v = rd.get<int64_t>();
            std::memcpy((char*)&want + 8 * w, &v, 8);
        }
        const int64_t want_chains = rd.get<int64_t>();
        if (!rd.ok) break;
        shards_total += n_shards;
        ProgPart fwd = parts[0];
        for (size_t s = 1; s < parts.size(); ++s) prog_part_merge(fwd, parts[s]);
        ProgPart rev = parts.back();
        for (size_t s = parts.size() - 1; s-- > 0;) prog_part_merge(rev, parts[s]);
        const ProgPart tree = tree_merge(parts, 0, parts.size());
        const ProgRec got = prog_finish(fwd, sc);
        const bool same_order = std::memcmp(&fwd, &rev, sizeof fwd) == 0 && std::memcmp(&fwd, &tree, sizeof fwd) == 0;
        const bool same_rec = std::memcmp(&got, &want, sizeof got) == 0;
        const bool same_chain = (prog_chains(got, sc.has_I != 0) ? 1 : 0) == want_chains;
        if (!same_order || !same_rec || !same_chain || fwd.tag != q + 1) {
            if (++bad <= 10)
                std::printf("case %lld (K %lld, %lld shards): order %d record %d chains %d; got (%lld, %g, %lld, %g, %g, "
                            "%lld, %g, %lld)\n",
                            (long long)q, (long long)K, (long long)n_shards, (int)same_order, (int)same_rec,
                            (int)same_chain, (long long)got.outcome, got.bestF_f, (long long)got.bestF_g, got.newI_f,
                            got.newI_h, (long long)got.newI_g, got.h_new, (long long)got.evaluated);
        }
    }
    if (!rd.ok || rd.at != rd.buf.size()) {
        std::printf("the file is truncated or has trailing bytes\n");
        return 1;
    }
    std::printf("cases %lld shards %lld bad %lld: %s\n", (long long)n_cases, (long long)shards_total, (long long)bad,
                bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
