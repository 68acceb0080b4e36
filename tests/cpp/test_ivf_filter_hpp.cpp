// The filtered forms of vq::IVFFlatIndex and vq::IVFScalarIndex of include/vq.hpp (search and range_search under a row
// mask): `validate` checks the argument errors of the wrapper and of the C ABI (no device needed -- they come before any
// device work); `run in out` searches the rows of `in` under its mask and writes the results for the driver
// (tests/test_cpp_ivf_filter.py) to compare with the numpy statement (tests/ref_ivf_filter.py).
//   in : u64 n, u64 d, u64 nq, u64 topk, u64 nlist, u64 nprobe, f32 sq_min, f32 sq_max, u64 levels, f32 coarse [nlist][d],
//        u32 lists [n], f32 rows [n][d], u8 codes [n][d], f32 queries [nq][d], u8 allowed [n], then for each of the four
//        metrics f32 radii [nq] (flat) and f32 radii [nq] (scalar)
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

// the wrapper's checks on an index of 70 rows (3 mask words) in 4 lists, dim 3: none of them reaches the device
template <class Index>
static void validate_index(Index &ix) {
    using K = vq::VqError::Kind;
    const std::vector<float> q(6, 0.0f), radii(2, 1.0f), nan_radii{1.0f, std::numeric_limits<float>::quiet_NaN()};
    const std::vector<std::uint32_t> three(3, ~0u), four(4, ~0u);
    const std::uint64_t cap = 100;
    EXPECT(ix.size() == 70);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 5, 2, nullptr); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q, 5, 2, four); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([&] { ix.search(q, 5, 2, std::vector<std::uint32_t>()); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([&] { ix.search(std::vector<float>(5, 0.0f), 5, 2, three); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 0, 2, three.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 71, 2, three.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 5, 0, three.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 5, 5, three.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.range_search(q.data(), 2, radii.data(), 2, cap, nullptr); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.range_search(q, radii, 2, cap, four); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([&] { ix.range_search(q, std::vector<float>(3, 1.0f), 2, cap, three); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([&] { ix.range_search(q.data(), 2, radii.data(), 2, 0, three.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.range_search(q.data(), 2, nan_radii.data(), 2, cap, three.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.range_search(q.data(), 2, radii.data(), 0, cap, three.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.range_search(q.data(), 2, radii.data(), 5, cap, three.data()); }) == (int)K::InvalidParameter);
    // no queries: the empty results, without a device
    EXPECT(ix.search(q.data(), 0, 5, 2, three.data()).idx.empty());
    const vq::RangeResult e = ix.range_search(q.data(), 0, radii.data(), 2, cap, three.data());
    EXPECT(e.lims.size() == 1 && e.lims[0] == 0 && e.idx.empty());
}

static int validate() {
    const std::size_t n = 70, d = 3, nlist = 4;
    std::vector<float> coarse(nlist * d);
    for (std::size_t e = 0; e < coarse.size(); ++e) coarse[e] = (float)e;
    std::vector<std::uint32_t> lists(n);
    for (std::size_t i = 0; i < n; ++i) lists[i] = (std::uint32_t)(i % nlist);
    const std::vector<float> rows(n * d, 0.0f);
    const std::vector<std::uint8_t> codes(n * d, 0);
    vq::IVFFlatIndex flat(coarse.data(), nlist, d);
    flat.add(lists.data(), rows.data(), n);
    validate_index(flat);
    vq::IVFScalarIndex sq(coarse.data(), nlist, d, vq::ScalarQuantizer(-1.0f, 1.0f, 256));
    sq.add_codes(lists.data(), codes.data(), n);
    validate_index(sq);
    // the mask follows the rows: after an add of 30, 100 rows are 4 words
    using K = vq::VqError::Kind;
    flat.add(lists.data(), rows.data(), 30);
    const std::vector<float> q(6, 0.0f);
    EXPECT(kind_of([&] { flat.search(q, 5, 2, std::vector<std::uint32_t>(3, ~0u)); }) == (int)K::DimensionMismatch);
    EXPECT(flat.search(q.data(), 0, 5, 2, std::vector<std::uint32_t>(4, ~0u).data()).idx.empty());
    // the C ABI: the pointers (the mask among them) come before the index handle, a device mask's alignment too
    const std::vector<std::uint32_t> three(3, ~0u);
    const float good[2] = {1.0f, std::numeric_limits<float>::infinity()};
    std::uint32_t idx[2];
    float dist[2];
    vqhip_ivfflat *ff = reinterpret_cast<vqhip_ivfflat *>(8);  // never dereferenced: a NULL pointer is found first
    vqhip_ivfsq *fs = reinterpret_cast<vqhip_ivfsq *>(8);
    const std::uint32_t *odd = reinterpret_cast<const std::uint32_t *>(reinterpret_cast<const char *>(three.data()) + 1);
    EXPECT(vqhip_ivfflat_search_masked(nullptr, q.data(), 2, 1, 1, three.data(), idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_search_masked(ff, q.data(), 2, 1, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfsq_search_masked(nullptr, q.data(), 2, 1, 1, three.data(), idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfsq_search_masked(fs, q.data(), 2, 1, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_search_masked_device(ff, q.data(), 2, 1, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfsq_search_masked_device(fs, q.data(), 2, 1, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_search_masked_device(nullptr, q.data(), 2, 1, 1, odd, idx, dist) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(std::strstr(vqhip_last_error(), "row mask is not 4-byte aligned") != nullptr);
    EXPECT(vqhip_ivfsq_search_masked_device(nullptr, q.data(), 2, 1, 1, odd, idx, dist) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_ivfflat_search_masked_device(nullptr, q.data(), 2, 1, 1, three.data(), idx, dist) == VQHIP_ERR_NULL_PTR);
    vqhip_range *r = reinterpret_cast<vqhip_range *>(1);
    EXPECT(vqhip_ivfflat_range_search_masked(nullptr, q.data(), 2, 1, good, 10, three.data(), nullptr) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_range_search_masked(ff, q.data(), 2, 1, good, 10, nullptr, &r) == VQHIP_ERR_NULL_PTR && r == nullptr);
    EXPECT(vqhip_ivfsq_range_search_masked(fs, q.data(), 2, 1, good, 10, nullptr, &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_range_search_masked(nullptr, q.data(), 2, 1, good, 0, three.data(), &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_ivfsq_range_search_masked(nullptr, q.data(), 2, 1, good, 10, three.data(), &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_range_search_masked_device(ff, q.data(), 2, 1, good, 10, nullptr, &r) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_range_search_masked_device(nullptr, q.data(), 2, 1, good, 10, odd, &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_ivfsq_range_search_masked_device(nullptr, q.data(), 2, 1, good, 10, odd, &r) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(vqhip_ivfsq_range_search_masked_device(nullptr, q.data(), 2, 1, good, 10, three.data(), &r) == VQHIP_ERR_NULL_PTR);
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

template <class T>
static bool take(FILE *in, std::vector<T> &v) {
    return std::fread(v.data(), sizeof(T), v.size(), in) == v.size();
}

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[6], levels;
    float mm[2];
    if (std::fread(h, 8, 6, in) != 6 || std::fread(mm, 4, 2, in) != 2 || std::fread(&levels, 8, 1, in) != 1) return 2;
    const std::size_t n = h[0], d = h[1], nq = h[2], topk = h[3], nlist = h[4], nprobe = h[5];
    std::vector<float> coarse(nlist * d), rows(n * d), queries(nq * d), radii(2 * 4 * nq);
    std::vector<std::uint32_t> lists(n);
    std::vector<std::uint8_t> codes(n * d), bytes(n);
    if (!take(in, coarse) || !take(in, lists) || !take(in, rows) || !take(in, codes) || !take(in, queries) || !take(in, bytes) ||
        !take(in, radii))
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
    const std::uint64_t cap = std::uint64_t(1) << 28;
    using E = vq::VqError::Kind;
    for (std::size_t mi = 0; mi < 4; ++mi) {
        const float *rf = radii.data() + (2 * mi) * nq, *rs = rf + nq;
        vq::IVFFlatIndex f(coarse.data(), nlist, d, vq::Distance(metrics[mi]));
        f.add(lists.data(), rows.data(), n);
        vq::IVFScalarIndex s(coarse.data(), nlist, d, sq, vq::Distance(metrics[mi]));
        s.add_codes(lists.data(), codes.data(), n);
        const auto fa = f.search(queries.data(), nq, topk, nprobe, mask.data());
        const auto sa = s.search(queries, topk, nprobe, mask);  // the vector overloads
        const vq::RangeResult fr = f.range_search(queries.data(), nq, rf, nprobe, cap, mask.data());
        const vq::RangeResult sr = s.range_search(queries, std::vector<float>(rs, rs + nq), nprobe, cap, mask);
        EXPECT(fr.lims.size() == nq + 1 && fr.lims[0] == 0 && fr.lims[nq] == fr.idx.size() && fr.idx.size() == fr.dist.size());
        // all ones: the unmasked call, bit for bit; all zeros: padding, and no hits
        const auto plain = f.search(queries.data(), nq, topk, nprobe), full = f.search(queries.data(), nq, topk, nprobe, ones.data());
        EXPECT(plain.idx == full.idx && !std::memcmp(plain.dist.data(), full.dist.data(), plain.dist.size() * 4));
        const vq::RangeResult pr = s.range_search(queries.data(), nq, rs, nprobe), fu = s.range_search(queries.data(), nq, rs, nprobe, cap, ones.data());
        EXPECT(pr.lims == fu.lims && pr.idx == fu.idx && !std::memcmp(pr.dist.data(), fu.dist.data(), pr.dist.size() * 4));
        const auto none = s.search(queries.data(), nq, topk, nprobe, zeros.data());
        for (std::size_t e = 0; e < none.idx.size(); ++e) EXPECT(none.idx[e] == 0xFFFFFFFFu && none.dist[e] == std::numeric_limits<float>::infinity());
        EXPECT(f.range_search(queries.data(), nq, rf, nprobe, 10, zeros.data()).idx.empty());
        if (fr.idx.size() > 1)  // one hit fewer than there are: the cap
            EXPECT(kind_of([&] { f.range_search(queries.data(), nq, rf, nprobe, fr.idx.size() - 1, mask.data()); }) == (int)E::FfiError);
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
