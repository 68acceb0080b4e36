// vq::FlatIndex of include/vq.hpp: `validate` checks the argument errors (no device needed -- they are thrown before
// the library is called); `run in out` searches and reranks the rows of `in` and writes the results for the driver
// (tests/test_cpp_knn.py) to compare with the numpy statement.
//   in : u64 n, u64 d, u64 nq, u64 topk, u64 c, f32 rows [n][d], f32 queries [nq][d], u32 cand [nq][c]
//   out: for each metric: u32 idx [nq][topk], f32 dist [nq][topk] of search, then of rerank (topk of c)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vq.hpp"

static int fails = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                   \
        }                                                              \
    } while (0)

template <class Fn>
static vq::VqError::Kind kind_of(Fn fn) {
    try {
        fn();
    } catch (const vq::VqError &e) {
        return e.kind;
    }
    return vq::VqError::Kind::FfiError;  // (no error: reported as a mismatch by the caller)
}

static int validate() {
    using K = vq::VqError::Kind;
    const std::vector<float> rows(12, 0.0f);
    EXPECT(kind_of([&] { vq::FlatIndex f(rows.data(), 0, 3); }) == K::EmptyInput);
    EXPECT(kind_of([&] { vq::FlatIndex f(rows.data(), 4, 0); }) == K::InvalidParameter);
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[5];
    if (std::fread(h, 8, 5, in) != 5) return 2;
    const std::size_t n = h[0], d = h[1], nq = h[2], topk = h[3], c = h[4];
    std::vector<float> rows(n * d), queries(nq * d);
    std::vector<std::uint32_t> cand(nq * c);
    if (std::fread(rows.data(), 4, rows.size(), in) != rows.size() || std::fread(queries.data(), 4, queries.size(), in) != queries.size() ||
        std::fread(cand.data(), 4, cand.size(), in) != cand.size())
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const vq::Distance::Kind metrics[] = {vq::Distance::SquaredEuclidean, vq::Distance::Euclidean, vq::Distance::Manhattan,
                                          vq::Distance::CosineDistance};
    for (vq::Distance::Kind m : metrics) {
        vq::FlatIndex f(rows.data(), n, d, vq::Distance(m));
        EXPECT(f.size() == n && f.dim() == d);
        const vq::FlatIndex::Result s = f.search(queries.data(), nq, topk);
        const vq::FlatIndex::Result r = f.rerank(queries.data(), nq, cand.data(), c, topk);
        EXPECT(kind_of([&] { f.search(queries.data(), nq, 0); }) == vq::VqError::Kind::InvalidParameter);
        std::vector<std::uint32_t> bad(cand);
        bad[0] = (std::uint32_t)n;
        EXPECT(kind_of([&] { f.rerank(queries.data(), nq, bad.data(), c, topk); }) == vq::VqError::Kind::InvalidParameter);
        for (const auto *res : {&s, &r}) {
            std::fwrite(res->idx.data(), 4, res->idx.size(), out);
            std::fwrite(res->dist.data(), 4, res->dist.size(), out);
        }
    }
    std::fclose(out);
    std::printf("RUN_%s backend=%s\n", fails ? "FAILED" : "OK", vq::get_simd_backend().c_str());
    return fails ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "validate")) return validate();
    if (argc >= 4 && !std::strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    std::fprintf(stderr, "usage: %s validate | run in out\n", argv[0]);
    return 2;
}
