// vq::BinaryIndex of include/vq.hpp: `validate` checks the argument errors (no device needed -- they are thrown before
// the library is called); `run in out` searches the rows of `in` and writes the results for the driver
// (tests/test_cpp_binary.py) to compare with the numpy statement.
//   in : u64 n, u64 d, u64 nq, u64 topk, f32 threshold, u32 low, u32 high, f32 rows [n][d], f32 queries [nq][d]
//   out: u32 packed words [n][W]; then for each metric (squared Euclidean, Euclidean, Manhattan): u32 idx [nq][topk],
//        f32 dist [nq][topk]
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
    const std::vector<float> rows(8200 * 2, 0.0f);
    const vq::BinaryQuantizer bq(0.0f, 0, 1);
    EXPECT(kind_of([&] { vq::BinaryIndex b(rows.data(), 0, 3); }) == K::EmptyInput);
    EXPECT(kind_of([&] { vq::BinaryIndex b(rows.data(), 2, 0); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::BinaryIndex b(rows.data(), 2, 8193); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::BinaryIndex b(rows.data(), 2, 4, bq, vq::Distance(vq::Distance::CosineDistance)); }) ==
           K::InvalidParameter);
    const std::vector<std::uint32_t> words = {1u << 5, 0u};
    EXPECT(kind_of([&] { vq::BinaryIndex b(words.data(), 2, 5, bq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::BinaryQuantizer q(0.0f, 3, 3); }) == K::InvalidParameter);
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[4];
    float thr = 0;
    std::uint32_t lh[2];
    if (std::fread(h, 8, 4, in) != 4 || std::fread(&thr, 4, 1, in) != 1 || std::fread(lh, 4, 2, in) != 2) return 2;
    const std::size_t n = h[0], d = h[1], nq = h[2], topk = h[3];
    std::vector<float> rows(n * d), queries(nq * d);
    if (std::fread(rows.data(), 4, rows.size(), in) != rows.size() || std::fread(queries.data(), 4, queries.size(), in) != queries.size())
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const vq::BinaryQuantizer bq(thr, (std::uint8_t)lh[0], (std::uint8_t)lh[1]);
    const vq::Distance::Kind metrics[] = {vq::Distance::SquaredEuclidean, vq::Distance::Euclidean, vq::Distance::Manhattan};
    bool first = true;
    for (vq::Distance::Kind m : metrics) {
        vq::BinaryIndex b(rows.data(), n, d, bq, vq::Distance(m));
        EXPECT(b.size() == n && b.dim() == d);
        if (first) {
            const std::vector<std::uint32_t> w = b.packed();
            std::fwrite(w.data(), 4, w.size(), out);
            const vq::BinaryIndex again(w.data(), n, d, bq, vq::Distance(m));
            EXPECT(again.packed() == w);
            first = false;
        }
        const vq::BinaryIndex::Result s = b.search(queries.data(), nq, topk);
        EXPECT(kind_of([&] { b.search(queries.data(), nq, 0); }) == vq::VqError::Kind::InvalidParameter);
        std::fwrite(s.idx.data(), 4, s.idx.size(), out);
        std::fwrite(s.dist.data(), 4, s.dist.size(), out);
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
