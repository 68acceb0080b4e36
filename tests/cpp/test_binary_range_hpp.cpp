// vq::BinaryIndex::hamming_range_search and vq::IVFBinaryIndex::hamming_range_search of include/vq.hpp: `validate` checks
// the argument errors of the wrappers and of the C ABI (no device needed -- they come before any device work); `run in
// out` searches the rows of `in` and writes the results for the driver (tests/test_cpp_binary_range.py) to compare with
// the numpy statement.
//   in : u64 n, u64 d, u64 nq, u64 nlist, u64 nprobe, f32 threshold, u32 low, u32 high, f32 rows [n][d],
//        f32 queries [nq][d], f32 coarse [nlist][d], u32 lists [n], u32 radii [nq]
//   out: for each of the three metrics, dense then inverted-file at nprobe then inverted-file at nlist:
//        u64 lims [nq + 1], u32 idx [total], f32 dist [total]
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
    const std::vector<float> q(8, 0.0f);
    const std::uint32_t radii[2] = {0u, 0xFFFFFFFFu};
    // the C ABI: out, pointers and max_results come before the index handle; every u32 is a radius
    vqhip_range *r = reinterpret_cast<vqhip_range *>(1);
    EXPECT(vqhip_binary_range_search(nullptr, q.data(), 2, radii, 10, nullptr) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_range_search(nullptr, nullptr, 2, radii, 10, &r) == VQHIP_ERR_NULL_PTR && r == nullptr);
    EXPECT(vqhip_binary_range_search_device(nullptr, q.data(), 2, nullptr, 10, &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_range_search(nullptr, q.data(), 2, radii, 0, &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(std::strstr(vqhip_last_error(), "max_results") != nullptr);
    EXPECT(vqhip_binary_range_search_device(nullptr, q.data(), 2, radii, 10, &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfbin_range_search(nullptr, q.data(), 2, 1, radii, 10, nullptr) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfbin_range_search(nullptr, q.data(), 2, 1, nullptr, 10, &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfbin_range_search_device(nullptr, q.data(), 2, 1, radii, 0, &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_ivfbin_range_search(nullptr, q.data(), 2, 1, radii, 10, &r) == VQHIP_ERR_NULL_PTR && r == nullptr);
    // the inverted-file wrapper needs no device until it searches
    const std::vector<float> coarse(3 * 4, 0.5f);
    vq::IVFBinaryIndex ix(coarse.data(), 3, 4);
    EXPECT(kind_of([&] { ix.hamming_range_search(q.data(), 2, radii, 0); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.hamming_range_search(q.data(), 2, radii, 4); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.hamming_range_search(q.data(), 2, radii, 1, 0); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { EXPECT(ix.hamming_range_search(q.data(), 0, radii, 1).lims.size() == 1); }) == -1);
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

static void write(FILE *out, const vq::RangeResult &r) {
    std::fwrite(r.lims.data(), 8, r.lims.size(), out);
    std::fwrite(r.idx.data(), 4, r.idx.size(), out);
    std::fwrite(r.dist.data(), 4, r.dist.size(), out);
}

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[5];
    float thr;
    std::uint32_t lh[2];
    if (std::fread(h, 8, 5, in) != 5 || std::fread(&thr, 4, 1, in) != 1 || std::fread(lh, 4, 2, in) != 2) return 2;
    const std::size_t n = h[0], d = h[1], nq = h[2], nlist = h[3], nprobe = h[4];
    std::vector<float> rows(n * d), queries(nq * d), coarse(nlist * d);
    std::vector<std::uint32_t> lists(n), radii(nq);
    if (std::fread(rows.data(), 4, rows.size(), in) != rows.size() || std::fread(queries.data(), 4, queries.size(), in) != queries.size() ||
        std::fread(coarse.data(), 4, coarse.size(), in) != coarse.size() || std::fread(lists.data(), 4, n, in) != n ||
        std::fread(radii.data(), 4, nq, in) != nq)
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const vq::Distance::Kind metrics[] = {vq::Distance::SquaredEuclidean, vq::Distance::Euclidean, vq::Distance::Manhattan};
    const vq::BinaryQuantizer bq(thr, (std::uint8_t)lh[0], (std::uint8_t)lh[1]);
    for (std::size_t mi = 0; mi < 3; ++mi) {
        vq::BinaryIndex b(rows.data(), n, d, bq, vq::Distance(metrics[mi]));
        vq::IVFBinaryIndex ix(coarse.data(), nlist, d, bq, vq::Distance(metrics[mi]));
        ix.add_rows(lists.data(), rows.data(), n);
        const vq::RangeResult a = b.hamming_range_search(queries.data(), nq, radii.data());
        const vq::RangeResult a2 = b.hamming_range_search(queries, radii);  // the vector overload
        const vq::RangeResult p = ix.hamming_range_search(queries.data(), nq, radii.data(), nprobe);
        const vq::RangeResult f = ix.hamming_range_search(queries.data(), nq, radii.data(), nlist);
        EXPECT(a.lims.size() == nq + 1 && a.lims[0] == 0 && a.lims[nq] == a.idx.size() && a.idx.size() == a.dist.size());
        EXPECT(a.lims == a2.lims && a.idx == a2.idx && std::memcmp(a.dist.data(), a2.dist.data(), 4 * a.dist.size()) == 0);
        EXPECT(f.lims == a.lims && f.idx == a.idx && std::memcmp(f.dist.data(), a.dist.data(), 4 * a.dist.size()) == 0);  // the identity
        EXPECT(p.idx.size() <= f.idx.size());
        EXPECT(kind_of([&] { b.hamming_range_search(queries.data(), nq, radii.data(), 0); }) == (int)vq::VqError::Kind::InvalidParameter);
        EXPECT(kind_of([&] { b.hamming_range_search(queries, std::vector<std::uint32_t>(nq + 1, 1u)); }) ==
               (int)vq::VqError::Kind::DimensionMismatch);
        if (a.idx.size() > 1) {  // one hit fewer than there are: the cap
            EXPECT(kind_of([&] { b.hamming_range_search(queries.data(), nq, radii.data(), a.idx.size() - 1); }) == (int)vq::VqError::Kind::FfiError);
            EXPECT(kind_of([&] { ix.hamming_range_search(queries.data(), nq, radii.data(), nlist, a.idx.size() - 1); }) ==
                   (int)vq::VqError::Kind::FfiError);
        }
        EXPECT(b.hamming_range_search(queries.data(), 0, radii.data()).lims.size() == 1);
        write(out, a);
        write(out, p);
        write(out, f);
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
