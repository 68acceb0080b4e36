// vq::AsymmetricBinaryIndex of include/vq.hpp: `validate` checks the argument errors (no device needed -- they are
// thrown before the library looks for one); `run in out` builds an index over the rows of `in`, searches, adds packed
// rows, removes rows and searches again, and writes the results for the driver (tests/test_cpp_abin.py) to compare with
// the numpy statement and with vq_amd.AsymmetricBinaryIndex.
//   in : u64 n, u64 d, u64 nq, u64 topk, u64 nadd, u64 nrem, f32 threshold, u32 low, u32 high, f32 rows [n][d],
//        f32 queries [nq][d], u32 added words [nadd][W], u32 removed ids [nrem]
//   out: for each metric (Euclidean, cosine): u32 words [n][W], search u32 idx [nq][topk], f32 dist [nq][topk]; then
//        after the add and the removal u64 n', u32 words [n'][W], search u32 idx [nq][topk], f32 dist [nq][topk]
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
    const std::vector<float> rows(80, 0.0f);
    const std::vector<std::uint8_t> codes(80, 0);
    std::vector<std::uint32_t> words(4, 0u);
    const vq::BinaryQuantizer bq(0.0f, 3, 200);
    EXPECT(kind_of([&] { vq::AsymmetricBinaryIndex a(rows.data(), 0, 3, bq); }) == K::EmptyInput);
    EXPECT(kind_of([&] { vq::AsymmetricBinaryIndex a(rows.data(), 2, 0, bq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::AsymmetricBinaryIndex a(rows.data(), 1, 8193, bq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::AsymmetricBinaryIndex a(codes.data(), 0, 3, bq); }) == K::EmptyInput);
    words[3] = 1u << 8;  // row 1 of two rows of 40 dimensions: bit 40, a pad bit
    EXPECT(kind_of([&] { vq::AsymmetricBinaryIndex a(words.data(), 2, 40, bq); }) == K::InvalidParameter);
    // the C ABI: cosine passes the metric check (a create without a device ends at VQHIP_ERR_NO_DEVICE, past every
    // argument check, or succeeds), an unknown metric and a pad bit do not
    vqhip_abin *x = nullptr;
    EXPECT(vqhip_abin_create(words.data(), VQHIP_BINARY_PACKED, 2, 40, 0.0f, 3, 200, VQHIP_COSINE, &x) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(std::strstr(vqhip_last_error(), "pad bit") != nullptr && x == nullptr);
    EXPECT(vqhip_abin_create(rows.data(), VQHIP_BINARY_F32, 2, 40, 0.0f, 3, 200, 9, &x) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(std::strstr(vqhip_last_error(), "metric") != nullptr && x == nullptr);
    const int rc = vqhip_abin_create(rows.data(), VQHIP_BINARY_F32, 2, 40, 0.0f, 3, 200, VQHIP_COSINE, &x);
    EXPECT(rc == VQHIP_OK || rc == VQHIP_ERR_NO_DEVICE);
    vqhip_abin_destroy(x);
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[6];
    float thr = 0;
    std::uint32_t lh[2];
    if (std::fread(h, 8, 6, in) != 6 || std::fread(&thr, 4, 1, in) != 1 || std::fread(lh, 4, 2, in) != 2) return 2;
    const std::size_t n = h[0], d = h[1], nq = h[2], topk = h[3], nadd = h[4], nrem = h[5], W = (d + 31) / 32;
    std::vector<float> rows(n * d), queries(nq * d);
    std::vector<std::uint32_t> added(nadd * W), gone(nrem);
    if (std::fread(rows.data(), 4, rows.size(), in) != rows.size() || std::fread(queries.data(), 4, queries.size(), in) != queries.size() ||
        std::fread(added.data(), 4, added.size(), in) != added.size() || std::fread(gone.data(), 4, gone.size(), in) != gone.size())
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const vq::BinaryQuantizer bq(thr, (std::uint8_t)lh[0], (std::uint8_t)lh[1]);
    const vq::Distance::Kind metrics[] = {vq::Distance::Euclidean, vq::Distance::CosineDistance};
    for (vq::Distance::Kind m : metrics) {
        vq::AsymmetricBinaryIndex a(rows.data(), n, d, bq, vq::Distance(m));
        EXPECT(a.size() == n && a.dim() == d && a.words_per_row() == W && a.quantizer().high() == lh[1]);
        const std::vector<std::uint32_t> words = a.packed();
        const vq::AsymmetricBinaryIndex twin(words.data(), n, d, bq, vq::Distance(m));
        const vq::AsymmetricBinaryIndex::Result r = a.search(queries.data(), nq, topk), r2 = twin.search(queries, topk);
        EXPECT(r.idx == r2.idx && !std::memcmp(r.dist.data(), r2.dist.data(), r.dist.size() * 4));
        EXPECT(kind_of([&] { a.search(queries.data(), nq, 0); }) == vq::VqError::Kind::InvalidParameter);
        std::fwrite(words.data(), 4, words.size(), out);
        std::fwrite(r.idx.data(), 4, r.idx.size(), out);
        std::fwrite(r.dist.data(), 4, r.dist.size(), out);
        const std::vector<std::uint32_t> ids = a.add_packed(added.data(), nadd);
        EXPECT(ids.size() == nadd && (nadd == 0 || (ids.front() == n && ids.back() == n + nadd - 1)));
        const std::vector<std::uint32_t> kept = a.remove_rows(gone);
        EXPECT(a.size() == kept.size() && kept.size() < n + nadd);
        const std::uint64_t left = a.size();
        const std::vector<std::uint32_t> after = a.packed();
        const vq::AsymmetricBinaryIndex::Result s = a.search(queries.data(), nq, topk);
        std::fwrite(&left, 8, 1, out);
        std::fwrite(after.data(), 4, after.size(), out);
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
