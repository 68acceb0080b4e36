// The filtered forms of vq::FlatIndex and vq::ScalarIndex of include/vq.hpp (search and range_search under a row mask)
// and vq::pack_row_mask: `validate` checks the argument errors of the wrapper and of the C ABI (no device needed -- they
// come before any device work); `run in out` searches the rows of `in` under its mask and writes the results for the
// driver (tests/test_cpp_filter.py) to compare with the numpy statement (tests/ref_filter.py).
//   in : u64 n, u64 d, u64 nq, u64 topk, f32 sq_min, f32 sq_max, u64 levels, f32 rows [n][d], f32 queries [nq][d],
//        u8 allowed [n], then for each of the four metrics f32 radii [nq] (flat) and f32 radii [nq] (scalar)
//   out: for each metric, flat then scalar: u32 idx [nq][topk], f32 dist [nq][topk], u64 lims [nq + 1], u32 idx [total],
//        f32 dist [total]
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
    // pack_row_mask: row i is bit i & 31 of word i >> 5, the pad bits zero
    EXPECT(vq::pack_row_mask(std::vector<bool>()).empty());
    for (std::size_t n : {1u, 31u, 32u, 33u, 64u, 65u, 1037u}) {
        std::vector<bool> m(n);
        for (std::size_t i = 0; i < n; ++i) m[i] = (i * 7 + n) % 3 == 0 || i == n - 1;
        const std::vector<std::uint32_t> w = vq::pack_row_mask(m);
        EXPECT(w.size() == (n + 31) / 32);
        for (std::size_t i = 0; i < w.size() * 32; ++i) EXPECT(((w[i >> 5] >> (i & 31)) & 1u) == (i < n && m[i] ? 1u : 0u));
    }
    // the wrapper's own checks
    const std::vector<std::uint32_t> three(3, ~0u);
    EXPECT(kind_of([&] { vq::detail::check_row_mask(nullptr); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { vq::detail::check_row_mask(three.data()); }) == -1);
    EXPECT(kind_of([&] { vq::detail::check_row_mask(three, 65); }) == -1);
    EXPECT(kind_of([&] { vq::detail::check_row_mask(three, 96); }) == -1);
    EXPECT(kind_of([&] { vq::detail::check_row_mask(three, 64); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([&] { vq::detail::check_row_mask(three, 97); }) == (int)K::DimensionMismatch);
    // the C ABI: the pointers (the mask among them) come before the index handle, a device mask's alignment too
    const std::vector<float> q(8, 0.0f);
    const float good[2] = {1.0f, std::numeric_limits<float>::infinity()};
    std::uint32_t idx[2];
    float dist[2];
    vqhip_flat *ff = reinterpret_cast<vqhip_flat *>(8);        // never dereferenced: a NULL pointer is found first
    vqhip_sqindex *fs = reinterpret_cast<vqhip_sqindex *>(8);
    const std::uint32_t *odd = reinterpret_cast<const std::uint32_t *>(reinterpret_cast<const char *>(three.data()) + 1);
    EXPECT(vqhip_flat_search_masked(nullptr, q.data(), 2, 1, three.data(), idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_flat_search_masked(ff, q.data(), 2, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_sqindex_search_masked(nullptr, q.data(), 2, 1, three.data(), idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_sqindex_search_masked(fs, q.data(), 2, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_flat_search_masked_device(ff, q.data(), 2, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_sqindex_search_masked_device(fs, q.data(), 2, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_flat_search_masked_device(nullptr, q.data(), 2, 1, odd, idx, dist) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(std::strstr(vqhip_last_error(), "row mask is not 4-byte aligned") != nullptr);
    EXPECT(vqhip_sqindex_search_masked_device(nullptr, q.data(), 2, 1, odd, idx, dist) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_flat_search_masked_device(nullptr, q.data(), 2, 1, three.data(), idx, dist) == VQHIP_ERR_NULL_PTR);
    vqhip_range *r = reinterpret_cast<vqhip_range *>(1);
    EXPECT(vqhip_flat_range_search_masked(nullptr, q.data(), 2, good, 10, three.data(), nullptr) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_flat_range_search_masked(ff, q.data(), 2, good, 10, nullptr, &r) == VQHIP_ERR_NULL_PTR && r == nullptr);
    EXPECT(vqhip_sqindex_range_search_masked(fs, q.data(), 2, good, 10, nullptr, &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_flat_range_search_masked(nullptr, q.data(), 2, good, 0, three.data(), &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_sqindex_range_search_masked(nullptr, q.data(), 2, good, 10, three.data(), &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_flat_range_search_masked_device(ff, q.data(), 2, good, 10, nullptr, &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_flat_range_search_masked_device(nullptr, q.data(), 2, good, 10, odd, &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_sqindex_range_search_masked_device(nullptr, q.data(), 2, good, 10, odd, &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_sqindex_range_search_masked_device(nullptr, q.data(), 2, good, 10, three.data(), &r) == VQHIP_ERR_NULL_PTR);
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
    std::uint64_t h[4], levels;
    float mm[2];
    if (std::fread(h, 8, 4, in) != 4 || std::fread(mm, 4, 2, in) != 2 || std::fread(&levels, 8, 1, in) != 1) return 2;
    const std::size_t n = h[0], d = h[1], nq = h[2], topk = h[3];
    std::vector<float> rows(n * d), queries(nq * d), radii(2 * 4 * nq);
    std::vector<std::uint8_t> bytes(n);
    if (std::fread(rows.data(), 4, rows.size(), in) != rows.size() || std::fread(queries.data(), 4, queries.size(), in) != queries.size() ||
        std::fread(bytes.data(), 1, n, in) != n || std::fread(radii.data(), 4, radii.size(), in) != radii.size())
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    std::vector<bool> allowed(n);
    for (std::size_t i = 0; i < n; ++i) allowed[i] = bytes[i] != 0;
    const std::vector<std::uint32_t> mask = vq::pack_row_mask(allowed);
    const std::vector<std::uint32_t> ones(mask.size(), ~0u), zeros(mask.size(), 0u);
    const vq::Distance::Kind metrics[] = {vq::Distance::SquaredEuclidean, vq::Distance::Euclidean, vq::Distance::Manhattan,
                                          vq::Distance::CosineDistance};
    const vq::ScalarQuantizer sq(mm[0], mm[1], (std::size_t)levels);
    using E = vq::VqError::Kind;
    for (std::size_t mi = 0; mi < 4; ++mi) {
        const float *rf = radii.data() + (2 * mi) * nq, *rs = rf + nq;
        vq::FlatIndex f(rows.data(), n, d, vq::Distance(metrics[mi]));
        vq::ScalarIndex s(rows.data(), n, d, sq, vq::Distance(metrics[mi]));
        const auto fa = f.search(queries.data(), nq, topk, mask.data());
        const auto sa = s.search(queries, topk, mask);  // the vector overloads
        const vq::RangeResult fr = f.range_search(queries.data(), nq, rf, std::uint64_t(1) << 28, mask.data());
        const vq::RangeResult sr = s.range_search(queries, std::vector<float>(rs, rs + nq), std::uint64_t(1) << 28, mask);
        EXPECT(fr.lims.size() == nq + 1 && fr.lims[0] == 0 && fr.lims[nq] == fr.idx.size() && fr.idx.size() == fr.dist.size());
        // all ones: the unmasked call, bit for bit; all zeros: padding, and no hits
        const auto plain = f.search(queries.data(), nq, topk), full = f.search(queries.data(), nq, topk, ones.data());
        EXPECT(plain.idx == full.idx && !std::memcmp(plain.dist.data(), full.dist.data(), plain.dist.size() * 4));
        const auto none = s.search(queries.data(), nq, topk, zeros.data());
        for (std::size_t e = 0; e < none.idx.size(); ++e) EXPECT(none.idx[e] == 0xFFFFFFFFu && none.dist[e] == std::numeric_limits<float>::infinity());
        EXPECT(f.range_search(queries.data(), nq, rf, 10, zeros.data()).idx.empty());
        // argument errors, without a call into the library
        EXPECT(kind_of([&] { f.search(queries.data(), nq, topk, nullptr); }) == (int)E::InvalidParameter);
        EXPECT(kind_of([&] { s.search(queries, topk, std::vector<std::uint32_t>(mask.size() + 1)); }) == (int)E::DimensionMismatch);
        EXPECT(kind_of([&] { f.search(queries.data(), nq, 0, mask.data()); }) == (int)E::InvalidParameter);
        EXPECT(kind_of([&] { s.range_search(queries.data(), nq, rs, 10, nullptr); }) == (int)E::InvalidParameter);
        EXPECT(kind_of([&] { f.range_search(queries, std::vector<float>(rf, rf + nq), 10, std::vector<std::uint32_t>()); }) ==
               (int)E::DimensionMismatch);
        EXPECT(kind_of([&] { f.range_search(queries.data(), nq, rf, 0, mask.data()); }) == (int)E::InvalidParameter);
        if (fr.idx.size() > 1)  // one hit fewer than there are: the cap
            EXPECT(kind_of([&] { f.range_search(queries.data(), nq, rf, fr.idx.size() - 1, mask.data()); }) == (int)E::FfiError);
        EXPECT(s.range_search(queries.data(), 0, rs, 10, mask.data()).lims.size() == 1);
        write(out, fa, fr);
        write(out, sa, sr);
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
