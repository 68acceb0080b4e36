// The filtered forms of vq::BinaryIndex and vq::IVFBinaryIndex of include/vq.hpp (search and hamming_range_search under a
// row mask): `validate` checks the argument errors of the wrapper and of the C ABI (no device needed -- they come before
// any device work); `run in out` searches the rows of `in` under its mask and writes the results for the driver
// (tests/test_cpp_binary_filter.py) to compare with the numpy statement (tests/ref_binary_filter.py).
//   in : u64 n, u64 d, u64 nq, u64 topk, u64 nlist, u64 nprobe, f32 threshold, u32 low, u32 high, f32 rows [n][d],
//        f32 queries [nq][d], u8 allowed [n], u32 radii [nq], f32 coarse [nlist][d], u32 lists [n]
//   out: for each of the three metrics, BinaryIndex then IVFBinaryIndex: u32 idx [nq][topk], f32 dist [nq][topk],
//        u64 lims [nq + 1], u32 idx [total], f32 dist [total]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
static int kind_of(Fn fn) {
    try {
        fn();
    } catch (const vq::VqError &e) {
        return (int)e.kind;
    }
    return -1;  // no error
}

static int validate() {
    using K = vq::VqError::Kind;
    // the C ABI: the pointers (the mask among them) come before the index handle, a device mask's alignment too
    const std::vector<std::uint32_t> three(3, ~0u);
    const std::vector<float> q(8, 0.0f);
    const std::uint32_t good[2] = {1u, 0xFFFFFFFFu};
    std::uint32_t idx[2];
    float dist[2];
    vqhip_binary *fb = reinterpret_cast<vqhip_binary *>(8);  // never dereferenced: a NULL pointer is found first
    vqhip_ivfbin *fi = reinterpret_cast<vqhip_ivfbin *>(8);
    const std::uint32_t *odd = reinterpret_cast<const std::uint32_t *>(reinterpret_cast<const char *>(three.data()) + 1);
    EXPECT(vqhip_binary_search_masked(nullptr, q.data(), 2, 1, three.data(), idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_search_masked(fb, q.data(), 2, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfbin_search_masked(nullptr, q.data(), 2, 1, 1, three.data(), idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfbin_search_masked(fi, q.data(), 2, 1, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_search_masked_device(fb, q.data(), 2, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfbin_search_masked_device(fi, q.data(), 2, 1, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_search_masked_device(nullptr, q.data(), 2, 1, odd, idx, dist) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(std::strstr(vqhip_last_error(), "row mask is not 4-byte aligned") != nullptr);
    EXPECT(vqhip_ivfbin_search_masked_device(nullptr, q.data(), 2, 1, 1, odd, idx, dist) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_binary_search_masked_device(nullptr, q.data(), 2, 1, three.data(), idx, dist) == VQHIP_ERR_NULL_PTR);
    vqhip_range *r = reinterpret_cast<vqhip_range *>(1);
    EXPECT(vqhip_binary_range_search_masked(nullptr, q.data(), 2, good, 10, three.data(), nullptr) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_range_search_masked(fb, q.data(), 2, good, 10, nullptr, &r) == VQHIP_ERR_NULL_PTR && r == nullptr);
    EXPECT(vqhip_ivfbin_range_search_masked(fi, q.data(), 2, 1, good, 10, nullptr, &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_range_search_masked(nullptr, q.data(), 2, good, 0, three.data(), &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_ivfbin_range_search_masked(nullptr, q.data(), 2, 1, good, 10, three.data(), &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_range_search_masked_device(fb, q.data(), 2, good, 10, nullptr, &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_range_search_masked_device(nullptr, q.data(), 2, good, 10, odd, &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_ivfbin_range_search_masked_device(nullptr, q.data(), 2, 1, good, 10, odd, &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_ivfbin_range_search_masked_device(nullptr, q.data(), 2, 1, good, 10, three.data(), &r) == VQHIP_ERR_NULL_PTR);
    // the inverted file's wrapper needs no device until it searches: its argument errors
    const std::vector<float> coarse(2 * 4, 0.0f);
    vq::IVFBinaryIndex ix(coarse.data(), 2, 4);
    const std::uint32_t lists[3] = {0, 1, 1}, words[3] = {1, 2, 3};
    ix.add_packed(lists, words, 3);
    const std::vector<std::uint32_t> one(1, ~0u);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 1, 1, nullptr); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 0, 1, one.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 4, 1, one.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 1, 3, one.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q, 1, 1, std::vector<std::uint32_t>(2)); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([&] { ix.hamming_range_search(q.data(), 2, good, 1, 10, nullptr); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.hamming_range_search(q.data(), 2, good, 1, 0, one.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.hamming_range_search(q.data(), 2, good, 0, 10, one.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.hamming_range_search(q, std::vector<std::uint32_t>(3), 1, 10, one); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([&] { ix.hamming_range_search(q, std::vector<std::uint32_t>(2), 1, 10, three); }) == (int)K::DimensionMismatch);
    EXPECT(ix.hamming_range_search(q.data(), 0, good, 1, 10, one.data()).lims.size() == 1);
    EXPECT(ix.search(q.data(), 0, 1, 1, one.data()).idx.empty());
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

template <class Result>
static void write(FILE *out, const Result &s, const vq::RangeResult &r) {
    std::fwrite(s.idx.data(), 4, s.idx.size(), out);
    std::fwrite(s.dist.data(), 4, s.dist.size(), out);
    std::fwrite(r.lims.data(), 8, r.lims.size(), out);
    std::fwrite(r.idx.data(), 4, r.idx.size(), out);
    std::fwrite(r.dist.data(), 4, r.dist.size(), out);
}

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[6];
    float thr;
    std::uint32_t lh[2];
    if (std::fread(h, 8, 6, in) != 6 || std::fread(&thr, 4, 1, in) != 1 || std::fread(lh, 4, 2, in) != 2) return 2;
    const std::size_t n = h[0], d = h[1], nq = h[2], topk = h[3], nlist = h[4], nprobe = h[5];
    std::vector<float> rows(n * d), queries(nq * d), coarse(nlist * d);
    std::vector<std::uint8_t> bytes(n);
    std::vector<std::uint32_t> radii(nq), lists(n);
    if (std::fread(rows.data(), 4, rows.size(), in) != rows.size() || std::fread(queries.data(), 4, queries.size(), in) != queries.size() ||
        std::fread(bytes.data(), 1, n, in) != n || std::fread(radii.data(), 4, nq, in) != nq ||
        std::fread(coarse.data(), 4, coarse.size(), in) != coarse.size() || std::fread(lists.data(), 4, n, in) != n)
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    std::vector<bool> allowed(n);
    for (std::size_t i = 0; i < n; ++i) allowed[i] = bytes[i] != 0;
    const std::vector<std::uint32_t> mask = vq::pack_row_mask(allowed);
    const std::vector<std::uint32_t> ones(mask.size(), ~0u), zeros(mask.size(), 0u);
    const vq::Distance::Kind metrics[] = {vq::Distance::SquaredEuclidean, vq::Distance::Euclidean, vq::Distance::Manhattan};
    const vq::BinaryQuantizer bq(thr, (std::uint8_t)lh[0], (std::uint8_t)lh[1]);
    const std::uint64_t cap = std::uint64_t(1) << 28;
    using E = vq::VqError::Kind;
    for (std::size_t mi = 0; mi < 3; ++mi) {
        vq::BinaryIndex b(rows.data(), n, d, bq, vq::Distance(metrics[mi]));
        vq::IVFBinaryIndex v(coarse.data(), nlist, d, bq, vq::Distance(metrics[mi]));
        v.add_rows(lists.data(), rows.data(), n);
        const auto ba = b.search(queries.data(), nq, topk, mask.data());
        const auto va = v.search(queries, topk, nprobe, mask);  // the vector overloads
        const vq::RangeResult br = b.hamming_range_search(queries, radii, cap, mask);
        const vq::RangeResult vr = v.hamming_range_search(queries.data(), nq, radii.data(), nprobe, cap, mask.data());
        EXPECT(br.lims.size() == nq + 1 && br.lims[0] == 0 && br.lims[nq] == br.idx.size() && br.idx.size() == br.dist.size());
        // all ones: the unmasked call, bit for bit; all zeros: padding, and no hits
        const auto plain = b.search(queries.data(), nq, topk), full = b.search(queries.data(), nq, topk, ones.data());
        EXPECT(plain.idx == full.idx && !std::memcmp(plain.dist.data(), full.dist.data(), plain.dist.size() * 4));
        const auto vplain = v.search(queries.data(), nq, topk, nprobe), vfull = v.search(queries.data(), nq, topk, nprobe, ones.data());
        EXPECT(vplain.idx == vfull.idx && !std::memcmp(vplain.dist.data(), vfull.dist.data(), vplain.dist.size() * 4));
        const auto none = v.search(queries.data(), nq, topk, nprobe, zeros.data());
        for (std::size_t e = 0; e < none.idx.size(); ++e) EXPECT(none.idx[e] == 0xFFFFFFFFu && none.dist[e] == std::numeric_limits<float>::infinity());
        EXPECT(b.hamming_range_search(queries.data(), nq, radii.data(), 10, zeros.data()).idx.empty());
        // nprobe == nlist: the filtered BinaryIndex
        const auto vall = v.search(queries.data(), nq, topk, nlist, mask.data());
        EXPECT(vall.idx == ba.idx && !std::memcmp(vall.dist.data(), ba.dist.data(), ba.dist.size() * 4));
        // argument errors, without a call into the library
        EXPECT(kind_of([&] { b.search(queries.data(), nq, topk, nullptr); }) == (int)E::InvalidParameter);
        EXPECT(kind_of([&] { b.search(queries, topk, std::vector<std::uint32_t>(mask.size() + 1)); }) == (int)E::DimensionMismatch);
        EXPECT(kind_of([&] { b.search(queries.data(), nq, 0, mask.data()); }) == (int)E::InvalidParameter);
        EXPECT(kind_of([&] { b.hamming_range_search(queries.data(), nq, radii.data(), 10, nullptr); }) == (int)E::InvalidParameter);
        EXPECT(kind_of([&] { b.hamming_range_search(queries, radii, 10, std::vector<std::uint32_t>()); }) == (int)E::DimensionMismatch);
        EXPECT(kind_of([&] { b.hamming_range_search(queries.data(), nq, radii.data(), 0, mask.data()); }) == (int)E::InvalidParameter);
        if (br.idx.size() > 1)  // one hit fewer than there are: the cap
            EXPECT(kind_of([&] { b.hamming_range_search(queries.data(), nq, radii.data(), br.idx.size() - 1, mask.data()); }) == (int)E::FfiError);
        EXPECT(b.hamming_range_search(queries.data(), 0, radii.data(), 10, mask.data()).lims.size() == 1);
        write(out, ba, br);
        write(out, va, vr);
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
