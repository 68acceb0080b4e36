// vq::IVFBinaryIndex of include/vq.hpp: `validate` checks the argument errors and the host-only calls (construction,
// add_packed, add_codes, packed, list sizes: no device needed); `run in out` searches the index of `in` and writes the
// results for the driver (tests/test_cpp_ivfbin.py) to compare with the numpy statement.
//   in : u64 nlist, u64 dim, u64 n, u64 nq, u64 topk, u64 nprobe, f32 threshold, u32 low, u32 high, f32 coarse [nlist][dim],
//        u32 list ids [n], u32 words [n][W], u8 codes [n][dim], f32 rows [n][dim], f32 queries [nq][dim]; the first n / 3
//        rows are added as words, the next n / 3 as codes, the others as rows
//   out: u32 words [n][W] of the index, then for each reported metric (squared Euclidean, Euclidean, Manhattan; the
//        probe under Euclidean, Manhattan, cosine in turn): u32 probe [nq][nprobe], u32 idx [nq][topk], f32 dist [nq][topk]
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
    const std::vector<float> coarse(4 * 8192, 0.0f);
    const vq::BinaryQuantizer bq(0.25f, 3, 200);
    const vq::Distance cosine(vq::Distance::CosineDistance), manhattan(vq::Distance::Manhattan);
    EXPECT(kind_of([&] { vq::IVFBinaryIndex ix(coarse.data(), 0, 37, bq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::IVFBinaryIndex ix(coarse.data(), 65537, 37, bq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::IVFBinaryIndex ix(coarse.data(), 4, 0, bq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::IVFBinaryIndex ix(coarse.data(), 4, 8193, bq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::IVFBinaryIndex ix(coarse.data(), 4, 37, bq, cosine); }) == K::InvalidParameter);
    vq::IVFBinaryIndex wide(coarse.data(), 4, 8192, bq, manhattan, cosine);  // cosine probes
    EXPECT(wide.size() == 0 && wide.words_per_row() == 256 && wide.packed().empty());
    EXPECT(!std::strcmp(wide.distance_metric(), "manhattan") && !std::strcmp(wide.coarse_distance_metric(), "cosine"));
    vq::IVFBinaryIndex dflt(coarse.data(), 4, 37);
    EXPECT(!std::strcmp(dflt.distance_metric(), "manhattan") && !std::strcmp(dflt.coarse_distance_metric(), "euclidean"));
    EXPECT(dflt.quantizer().threshold() == 0.0f && dflt.quantizer().low() == 0 && dflt.quantizer().high() == 1);
    vq::IVFBinaryIndex ix(coarse.data(), 4, 37, bq);
    const std::uint32_t lists[3] = {0, 3, 3}, bad_lists[3] = {0, 4, 1};
    const std::uint32_t words[6] = {5u, 1u << 4, 0xFFFFFFFFu, 31u, 0u, 0u}, padded[6] = {5u, 1u << 4, 0u, 1u << 5, 0u, 0u};
    std::vector<std::uint8_t> codes(3 * 37);
    for (std::size_t e = 0; e < codes.size(); ++e) codes[e] = (std::uint8_t)(140 + e);  // on both sides of high = 200
    const std::vector<float> rows(3 * 37, 1.0f);
    EXPECT(kind_of([&] { ix.add_packed(bad_lists, words, 3); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.add_codes(bad_lists, codes.data(), 3); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.add_rows(bad_lists, rows.data(), 3); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.add_packed(lists, padded, 3); }) == K::InvalidParameter);
    EXPECT(ix.size() == 0);
    EXPECT(ix.add_packed(lists, words, 3) == 0 && ix.add_codes(lists, codes.data(), 3) == 3 && ix.size() == 6);
    EXPECT(ix.add_rows(lists, rows.data(), 0) == 6);
    const std::vector<std::uint64_t> sizes = ix.list_sizes();
    EXPECT(sizes.size() == 4 && sizes[0] == 2 && sizes[1] == 0 && sizes[2] == 0 && sizes[3] == 4);
    const std::vector<std::uint32_t> back = ix.packed();
    EXPECT(back.size() == 6 * 2 && !std::memcmp(back.data(), words, 24));
    for (std::size_t i = 0; i < 3; ++i) {  // add_codes: bit = code >= high
        std::uint32_t w[2] = {0, 0};
        for (std::size_t t = 0; t < 37; ++t)
            if (codes[i * 37 + t] >= 200) w[t / 32] |= 1u << (t % 32);
        EXPECT(back[6 + 2 * i] == w[0] && back[6 + 2 * i + 1] == w[1]);
    }
    EXPECT(ix.nlist() == 4 && ix.dim() == 37 && ix.words_per_row() == 2 && ix.quantizer().high() == 200);
    const std::vector<float> q(37, 0.0f);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 1, 0); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 1, 5); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 7, 1); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 0, 1); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.probe(q.data(), 1, 5); }) == K::InvalidParameter);
    EXPECT(ix.search(q.data(), 0, 2, 2).idx.empty() && ix.probe(q.data(), 0, 2).empty());
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[6];
    float thr;
    std::uint32_t lh[2];
    if (std::fread(h, 8, 6, in) != 6 || std::fread(&thr, 4, 1, in) != 1 || std::fread(lh, 4, 2, in) != 2) return 2;
    const std::size_t nlist = h[0], dim = h[1], n = h[2], nq = h[3], topk = h[4], nprobe = h[5], W = (dim + 31) / 32;
    std::vector<float> coarse(nlist * dim), rows(n * dim), queries(nq * dim);
    std::vector<std::uint32_t> lists(n), words(n * W);
    std::vector<std::uint8_t> codes(n * dim);
    if (std::fread(coarse.data(), 4, coarse.size(), in) != coarse.size() || std::fread(lists.data(), 4, n, in) != n ||
        std::fread(words.data(), 4, words.size(), in) != words.size() || std::fread(codes.data(), 1, codes.size(), in) != codes.size() ||
        std::fread(rows.data(), 4, rows.size(), in) != rows.size() || std::fread(queries.data(), 4, queries.size(), in) != queries.size())
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const vq::BinaryQuantizer bq(thr, (std::uint8_t)lh[0], (std::uint8_t)lh[1]);
    const vq::Distance::Kind metrics[] = {vq::Distance::SquaredEuclidean, vq::Distance::Euclidean, vq::Distance::Manhattan};
    const vq::Distance::Kind probes[] = {vq::Distance::Euclidean, vq::Distance::Manhattan, vq::Distance::CosineDistance};
    const std::size_t a = n / 3, b = 2 * (n / 3);
    for (int m = 0; m < 3; ++m) {
        vq::IVFBinaryIndex ix(coarse.data(), nlist, dim, bq, vq::Distance(metrics[m]), vq::Distance(probes[m]));
        ix.add_packed(lists.data(), words.data(), a);
        ix.add_codes(lists.data() + a, codes.data() + a * dim, b - a);
        ix.add_rows(lists.data() + b, rows.data() + b * dim, n - b);
        EXPECT(ix.size() == n && ix.nlist() == nlist && ix.dim() == dim);
        if (m == 0) {
            const std::vector<std::uint32_t> w = ix.packed();
            std::fwrite(w.data(), 4, w.size(), out);
        }
        const std::vector<std::uint32_t> p = ix.probe(queries.data(), nq, nprobe);
        const vq::IVFBinaryIndex::Result r = ix.search(queries.data(), nq, topk, nprobe);
        std::fwrite(p.data(), 4, p.size(), out);
        std::fwrite(r.idx.data(), 4, r.idx.size(), out);
        std::fwrite(r.dist.data(), 4, r.dist.size(), out);
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
