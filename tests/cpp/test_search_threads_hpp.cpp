// The `const` search methods of the index classes of include/vq.hpp from several std::threads on ONE object each: one
// vq::FlatIndex, one vq::IVFFlatIndex and one vq::BinaryIndex shared by reference, every thread with its own queries, nq and
// topk, calling the plain and the masked overloads in turn.  `run in out` writes each thread's results for the driver
// (tests/test_cpp_search_threads.py) to compare with the numpy statements; a thread whose repeated call gives other bits
// than its first is reported here already.
//   in : u64 n, d, nq, nlist, nprobe, threads, then per thread u64 q0, nq_t, topk_t; f32 rows [n][d], f32 queries [nq][d],
//        u8 allowed [n], f32 coarse [nlist][d], u32 lists [n]
//   out: per thread, in thread order: flat, flat masked, ivfflat, ivfflat masked, binary -- each u32 idx [nq_t][topk_t],
//        f32 dist [nq_t][topk_t]
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "vq.hpp"

struct Hits {
    std::vector<std::uint32_t> idx;
    std::vector<float> dist;
    template <class R>
    static Hits of(const R &r) {
        return Hits{r.idx, r.dist};
    }
    bool same(const Hits &o) const {
        return idx == o.idx && dist.size() == o.dist.size() && !std::memcmp(dist.data(), o.dist.data(), dist.size() * 4);
    }
};

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[6];
    if (std::fread(h, 8, 6, in) != 6) return 2;
    const std::size_t n = h[0], d = h[1], nq = h[2], nlist = h[3], nprobe = h[4], threads = h[5];
    std::vector<std::uint64_t> per(3 * threads);
    std::vector<float> rows(n * d), queries(nq * d), coarse(nlist * d);
    std::vector<std::uint8_t> bytes(n);
    std::vector<std::uint32_t> lists(n);
    if (std::fread(per.data(), 8, per.size(), in) != per.size() || std::fread(rows.data(), 4, rows.size(), in) != rows.size() ||
        std::fread(queries.data(), 4, queries.size(), in) != queries.size() || std::fread(bytes.data(), 1, n, in) != n ||
        std::fread(coarse.data(), 4, coarse.size(), in) != coarse.size() || std::fread(lists.data(), 4, n, in) != n)
        return 2;
    std::fclose(in);
    std::vector<bool> allowed(n);
    for (std::size_t i = 0; i < n; ++i) allowed[i] = bytes[i] != 0;
    const std::vector<std::uint32_t> mask = vq::pack_row_mask(allowed);

    const vq::FlatIndex flat(rows.data(), n, d, vq::Distance(vq::Distance::Euclidean));
    vq::IVFFlatIndex ivf_build(coarse.data(), nlist, d, vq::Distance(vq::Distance::CosineDistance));
    ivf_build.add(lists.data(), rows.data(), n);
    const vq::IVFFlatIndex &ivf = ivf_build;  // the threads see the const methods only
    const vq::BinaryIndex bin(rows.data(), n, d, vq::BinaryQuantizer(0.0f, 0, 1), vq::Distance(vq::Distance::Manhattan));

    constexpr int kRounds = 6;
    std::vector<std::vector<Hits>> results(threads);
    std::vector<std::string> errors(threads);
    std::atomic<std::size_t> ready{0};
    std::vector<std::thread> pool;
    for (std::size_t t = 0; t < threads; ++t) {
        pool.emplace_back([&, t] {
            try {
                const float *q = queries.data() + per[3 * t] * d;
                const std::size_t nq_t = per[3 * t + 1], topk = per[3 * t + 2];
                ++ready;
                while (ready.load() < threads) std::this_thread::yield();  // all released together
                for (int r = 0; r < kRounds; ++r) {
                    std::vector<Hits> now;
                    now.push_back(Hits::of(flat.search(q, nq_t, topk)));
                    now.push_back(Hits::of(flat.search(q, nq_t, topk, mask.data())));
                    now.push_back(Hits::of(ivf.search(q, nq_t, topk, nprobe)));
                    now.push_back(Hits::of(ivf.search(q, nq_t, topk, nprobe, mask.data())));
                    now.push_back(Hits::of(bin.search(q, nq_t, topk)));
                    if (r == 0) {
                        results[t] = now;
                        continue;
                    }
                    for (std::size_t k = 0; k < now.size(); ++k)
                        if (!now[k].same(results[t][k]) && errors[t].empty())
                            errors[t] = "call " + std::to_string(k) + " of round " + std::to_string(r) + " differs from round 0";
                }
            } catch (const std::exception &e) {
                errors[t] = e.what();
                ++ready;  // (never holds the others back)
            }
        });
    }
    for (std::thread &th : pool) th.join();
    int fails = 0;
    for (std::size_t t = 0; t < threads; ++t)
        if (!errors[t].empty()) {
            std::printf("FAIL thread %zu: %s\n", t, errors[t].c_str());
            ++fails;
        }
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    for (std::size_t t = 0; t < threads && !fails; ++t)
        for (const Hits &r : results[t]) {
            std::fwrite(r.idx.data(), 4, r.idx.size(), out);
            std::fwrite(r.dist.data(), 4, r.dist.size(), out);
        }
    std::fclose(out);
    std::printf("RUN_%s backend=%s\n", fails ? "FAILED" : "OK", vq::get_simd_backend().c_str());
    return fails ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    std::fprintf(stderr, "usage: %s run in out\n", argv[0]);
    return 2;
}
