// vq::IVFFlatIndex::range_search and vq::IVFScalarIndex::range_search of include/vq.hpp: `validate` checks the argument
// errors of the wrapper and of the C ABI (no device needed -- they come before any device work); `run in out` searches
// the rows of `in` and writes the results for the driver (tests/test_cpp_ivf_range.py) to compare with the numpy
// statement.
//   in : u64 n, u64 d, u64 nq, u64 nlist, u64 nprobe, f32 sq_min, f32 sq_max, u64 levels, f32 coarse [nlist][d],
//        u32 lists [n], f32 rows [n][d], f32 queries [nq][d], then for each of the four metrics f32 radii [nq] (flat) and
//        f32 radii [nq] (scalar)
//   out: for each metric, flat then scalar: u64 lims [nq + 1], u32 idx [total], f32 dist [total]
#include <cmath>
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
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const std::vector<float> q(8, 0.0f), coarse(12, 0.5f);
    const float good[2] = {1.0f, std::numeric_limits<float>::infinity()}, bad[2] = {1.0f, nan};
    // the wrapper's own checks, none of which needs a device: radii, max_results, nprobe
    vq::IVFFlatIndex f(coarse.data(), 3, 4);
    vq::IVFScalarIndex s(coarse.data(), 3, 4, vq::ScalarQuantizer(-1.0f, 1.0f, 256));
    EXPECT(kind_of([&] { f.range_search(q.data(), 2, bad, 1); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { s.range_search(q.data(), 2, bad, 1); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { f.range_search(q.data(), 2, good, 1, 0); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { f.range_search(q.data(), 2, good, 0); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { f.range_search(q.data(), 2, good, 4); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { s.range_search(q.data(), 2, good, 0); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { s.range_search(q.data(), 2, good, 1025); }) == (int)K::InvalidParameter);
    EXPECT(f.range_search(q.data(), 0, nullptr, 3).lims == std::vector<std::uint64_t>(1, 0));  // no queries: no device
    EXPECT(s.range_search(q.data(), 0, nullptr, 1).idx.empty());
    // the C ABI: out, pointers, max_results and the radii come before the index handle
    vqhip_range *r = reinterpret_cast<vqhip_range *>(1);
    EXPECT(vqhip_ivfflat_range_search(nullptr, q.data(), 2, 1, good, 10, nullptr) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_range_search(nullptr, nullptr, 2, 1, good, 10, &r) == VQHIP_ERR_NULL_PTR && r == nullptr);
    EXPECT(vqhip_ivfsq_range_search(nullptr, q.data(), 2, 1, nullptr, 10, &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_range_search(nullptr, q.data(), 2, 1, good, 0, &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_ivfsq_range_search(nullptr, q.data(), 2, 1, bad, 10, &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(std::strstr(vqhip_last_error(), "NaN") != nullptr);
    EXPECT(vqhip_ivfflat_range_search_device(nullptr, q.data(), 2, 1, bad, 10, &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_ivfsq_range_search_device(nullptr, q.data(), 2, 1, good, 10, &r) == VQHIP_ERR_NULL_PTR);
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
    std::uint64_t h[5], levels;
    float mm[2];
    if (std::fread(h, 8, 5, in) != 5 || std::fread(mm, 4, 2, in) != 2 || std::fread(&levels, 8, 1, in) != 1) return 2;
    const std::size_t n = h[0], d = h[1], nq = h[2], nlist = h[3], nprobe = h[4];
    std::vector<float> coarse(nlist * d), rows(n * d), queries(nq * d), radii(2 * 4 * nq);
    std::vector<std::uint32_t> lists(n);
    if (std::fread(coarse.data(), 4, coarse.size(), in) != coarse.size() || std::fread(lists.data(), 4, n, in) != n ||
        std::fread(rows.data(), 4, rows.size(), in) != rows.size() || std::fread(queries.data(), 4, queries.size(), in) != queries.size() ||
        std::fread(radii.data(), 4, radii.size(), in) != radii.size())
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const vq::Distance::Kind metrics[] = {vq::Distance::SquaredEuclidean, vq::Distance::Euclidean, vq::Distance::Manhattan,
                                          vq::Distance::CosineDistance};
    const vq::ScalarQuantizer sq(mm[0], mm[1], (std::size_t)levels);
    for (std::size_t mi = 0; mi < 4; ++mi) {
        const float *rf = radii.data() + (2 * mi) * nq, *rs = rf + nq;
        vq::IVFFlatIndex f(coarse.data(), nlist, d, vq::Distance(metrics[mi]));
        vq::IVFScalarIndex s(coarse.data(), nlist, d, sq, vq::Distance(metrics[mi]));
        EXPECT(f.range_search(queries.data(), nq, rf, nprobe).lims == std::vector<std::uint64_t>(nq + 1, 0));  // no rows yet
        f.add(lists.data(), rows.data(), n / 2);  // two adds
        f.add(lists.data() + n / 2, rows.data() + (n / 2) * d, n - n / 2);
        s.add_rows(lists.data(), rows.data(), n);
        const vq::RangeResult a = f.range_search(queries.data(), nq, rf, nprobe);
        const vq::RangeResult b = s.range_search(queries.data(), nq, rs, nprobe);
        EXPECT(a.lims.size() == nq + 1 && a.lims[0] == 0 && a.lims[nq] == a.idx.size() && a.idx.size() == a.dist.size());
        EXPECT(b.lims.size() == nq + 1 && b.lims[nq] == b.idx.size());
        if (a.idx.size() > 1) {  // one hit fewer than there are: the cap; exactly as many: the same result
            EXPECT(kind_of([&] { f.range_search(queries.data(), nq, rf, nprobe, a.idx.size() - 1); }) == (int)vq::VqError::Kind::FfiError);
            EXPECT(f.range_search(queries.data(), nq, rf, nprobe, a.idx.size()).idx == a.idx);
        }
        write(out, a);
        write(out, b);
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
