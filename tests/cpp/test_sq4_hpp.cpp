// vq::Scalar4Index of include/vq.hpp: `validate` checks the argument errors (no device needed -- they are thrown before
// the library looks for one); `run in out` builds an index over the rows of `in`, searches, adds packed rows, removes
// rows and searches again, and writes the results for the driver (tests/test_cpp_sq4.py) to compare with the numpy
// statement and with vq_amd.Scalar4Index.
//   in : u64 n, u64 d, u64 nq, u64 topk, u64 nadd, u64 nrem, f32 min, f32 max, u32 levels, f32 rows [n][d],
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
    std::vector<std::uint8_t> codes(66, 0);
    std::vector<std::uint32_t> words(10, 0u);
    const vq::ScalarQuantizer sq(-1.0f, 1.0f, 16);
    EXPECT(kind_of([&] { vq::Scalar4Index a(rows.data(), 0, 3, sq); }) == K::EmptyInput);
    EXPECT(kind_of([&] { vq::Scalar4Index a(rows.data(), 2, 0, sq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::Scalar4Index a(codes.data(), 0, 3, sq); }) == K::EmptyInput);
    EXPECT(kind_of([&] { vq::Scalar4Index a(rows.data(), 2, 33, vq::ScalarQuantizer(-1.0f, 1.0f, 17)); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::Scalar4Index a(rows.data(), 2, 33, vq::ScalarQuantizer(-1.0f, 1.0f, 256)); }) == K::InvalidParameter);
    codes[65] = 16;
    EXPECT(kind_of([&] { vq::Scalar4Index a(codes.data(), 2, 33, sq); }) == K::InvalidParameter);
    words[9] = 1u << 4;  // row 1 of two rows of 33 dimensions: dimension 33, a pad nibble
    EXPECT(kind_of([&] { vq::Scalar4Index a(words.data(), 2, 33, sq); }) == K::InvalidParameter);
    // the C ABI's host forms: the same three refused with their texts, an unknown metric too; every metric passes (a
    // create without a device ends at VQHIP_ERR_NO_DEVICE, past every argument check, or succeeds)
    vqhip_sq4index *x = nullptr;
    EXPECT(vqhip_sq4index_create(-1.0f, 1.0f, 16, words.data(), VQHIP_SQ4_PACKED, 2, 33, VQHIP_COSINE, &x) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(std::strstr(vqhip_last_error(), "pad nibble") != nullptr && x == nullptr);
    EXPECT(vqhip_sq4index_create(-1.0f, 1.0f, 16, codes.data(), VQHIP_SQ4_U8, 2, 33, VQHIP_COSINE, &x) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(std::strstr(vqhip_last_error(), "code 16") != nullptr && x == nullptr);
    EXPECT(vqhip_sq4index_create(-1.0f, 1.0f, 17, rows.data(), VQHIP_SQ4_F32, 2, 33, VQHIP_COSINE, &x) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(std::strstr(vqhip_last_error(), "levels 17: a 4-bit index holds at most 16") != nullptr && x == nullptr);
    EXPECT(vqhip_sq4index_create(-1.0f, 1.0f, 16, rows.data(), VQHIP_SQ4_F32, 2, 33, 9, &x) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(std::strstr(vqhip_last_error(), "metric") != nullptr && x == nullptr);
    const int rc = vqhip_sq4index_create(-1.0f, 1.0f, 16, rows.data(), VQHIP_SQ4_F32, 2, 33, VQHIP_COSINE, &x);
    EXPECT(rc == VQHIP_OK || rc == VQHIP_ERR_NO_DEVICE);
    vqhip_sq4index_destroy(x);
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[6];
    float mm[2];
    std::uint32_t levels = 0;
    if (std::fread(h, 8, 6, in) != 6 || std::fread(mm, 4, 2, in) != 2 || std::fread(&levels, 4, 1, in) != 1) return 2;
    const std::size_t n = h[0], d = h[1], nq = h[2], topk = h[3], nadd = h[4], nrem = h[5], W = (d + 7) / 8;
    std::vector<float> rows(n * d), queries(nq * d);
    std::vector<std::uint32_t> added(nadd * W), gone(nrem);
    if (std::fread(rows.data(), 4, rows.size(), in) != rows.size() || std::fread(queries.data(), 4, queries.size(), in) != queries.size() ||
        std::fread(added.data(), 4, added.size(), in) != added.size() || std::fread(gone.data(), 4, gone.size(), in) != gone.size())
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const vq::ScalarQuantizer sq(mm[0], mm[1], levels);
    const vq::Distance::Kind metrics[] = {vq::Distance::Euclidean, vq::Distance::CosineDistance};
    for (vq::Distance::Kind m : metrics) {
        vq::Scalar4Index a(rows.data(), n, d, sq, vq::Distance(m));
        EXPECT(a.size() == n && a.dim() == d && a.words_per_row() == W && a.quantizer().levels() == levels);
        const std::vector<std::uint32_t> words = a.packed();
        const std::vector<std::uint8_t> codes = a.codes();
        EXPECT(codes == sq.quantize(rows));
        const vq::Scalar4Index twin(words.data(), n, d, sq, vq::Distance(m)), bytes(codes.data(), n, d, sq, vq::Distance(m));
        const vq::ScalarIndex eight(codes.data(), n, d, sq, vq::Distance(m));
        const vq::Scalar4Index::Result r = a.search(queries.data(), nq, topk), r2 = twin.search(queries, topk), r3 = bytes.search(queries, topk);
        const vq::ScalarIndex::Result r8 = eight.search(queries, topk);
        EXPECT(r.idx == r2.idx && !std::memcmp(r.dist.data(), r2.dist.data(), r.dist.size() * 4));
        EXPECT(r.idx == r3.idx && !std::memcmp(r.dist.data(), r3.dist.data(), r.dist.size() * 4));
        EXPECT(r.idx == r8.idx && !std::memcmp(r.dist.data(), r8.dist.data(), r.dist.size() * 4));
        EXPECT(bytes.packed() == words);
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
        const vq::Scalar4Index::Result s = a.search(queries.data(), nq, topk);
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
