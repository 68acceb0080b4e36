// vq::ScalarIndex of include/vq.hpp: `validate` checks the argument errors (no device needed -- they are thrown before
// the library looks for one); `run in out` indexes the rows of `in` and writes the results for the driver
// (tests/test_cpp_sqindex.py) to compare with the numpy statement and with vq_amd.ScalarIndex.
//   in : u64 n, u64 d, u64 nq, u64 topk, u64 c, f32 min, f32 max, u32 levels, f32 rows [n][d], f32 queries [nq][d],
//        u32 candidates [nq][c]
//   out: u8 codes [n][d]; then for each metric (squared Euclidean, Euclidean, Manhattan, cosine): search u32 idx
//        [nq][topk], f32 dist [nq][topk], rerank u32 idx [nq][topk], f32 dist [nq][topk]
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
    const std::vector<float> rows(16, 0.0f);
    const std::vector<std::uint8_t> codes(16, 0);
    const vq::ScalarQuantizer sq(-1.0f, 1.0f, 256);
    EXPECT(kind_of([&] { vq::ScalarIndex s(rows.data(), 0, 3, sq); }) == K::EmptyInput);
    EXPECT(kind_of([&] { vq::ScalarIndex s(rows.data(), 2, 0, sq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::ScalarIndex s(codes.data(), 0, 3, sq); }) == K::EmptyInput);
    EXPECT(kind_of([&] { vq::ScalarIndex s(codes.data(), 2, 0, sq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::ScalarQuantizer q(1.0f, 1.0f, 256); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::ScalarQuantizer q(0.0f, 1.0f, 257); }) == K::InvalidParameter);
    // the C ABI keeps the quantizer's own text
    vqhip_sqindex *x = nullptr;
    EXPECT(vqhip_sqindex_create(0.0f, 1.0f, 1, codes.data(), 4, 4, VQHIP_EUCLIDEAN, &x) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(!std::strcmp(vqhip_last_error(), "Invalid parameter 'levels': must be at least 2"));
    EXPECT(x == nullptr);
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[5];
    float mm[2];
    std::uint32_t levels = 0;
    if (std::fread(h, 8, 5, in) != 5 || std::fread(mm, 4, 2, in) != 2 || std::fread(&levels, 4, 1, in) != 1) return 2;
    const std::size_t n = h[0], d = h[1], nq = h[2], topk = h[3], c = h[4];
    std::vector<float> rows(n * d), queries(nq * d);
    std::vector<std::uint32_t> cand(nq * c);
    if (std::fread(rows.data(), 4, rows.size(), in) != rows.size() ||
        std::fread(queries.data(), 4, queries.size(), in) != queries.size() || std::fread(cand.data(), 4, cand.size(), in) != cand.size())
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const vq::ScalarQuantizer sq(mm[0], mm[1], levels);
    const vq::Distance::Kind metrics[] = {vq::Distance::SquaredEuclidean, vq::Distance::Euclidean, vq::Distance::Manhattan,
                                          vq::Distance::CosineDistance};
    bool first = true;
    for (vq::Distance::Kind m : metrics) {
        const vq::ScalarIndex s(rows.data(), n, d, sq, vq::Distance(m));
        EXPECT(s.size() == n && s.dim() == d && s.quantizer().levels() == levels);
        const std::vector<std::uint8_t> codes = s.codes();
        if (first) {
            EXPECT(codes == sq.quantize(rows));
            std::fwrite(codes.data(), 1, codes.size(), out);
            first = false;
        }
        const vq::ScalarIndex again(codes.data(), n, d, sq, vq::Distance(m));
        const vq::ScalarIndex::Result r = s.search(queries.data(), nq, topk), r2 = again.search(queries, topk);
        EXPECT(r.idx == r2.idx && !std::memcmp(r.dist.data(), r2.dist.data(), r.dist.size() * 4));
        EXPECT(kind_of([&] { s.search(queries.data(), nq, 0); }) == vq::VqError::Kind::InvalidParameter);
        EXPECT(kind_of([&] { s.rerank(queries.data(), nq, cand.data(), c, c + 1); }) == vq::VqError::Kind::InvalidParameter);
        const vq::ScalarIndex::Result k = s.rerank(queries.data(), nq, cand.data(), c, topk);
        std::fwrite(r.idx.data(), 4, r.idx.size(), out);
        std::fwrite(r.dist.data(), 4, r.dist.size(), out);
        std::fwrite(k.idx.data(), 4, k.idx.size(), out);
        std::fwrite(k.dist.data(), 4, k.dist.size(), out);
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
