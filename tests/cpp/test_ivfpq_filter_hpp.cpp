// The filtered form of vq::IVFPQIndex of include/vq.hpp (search under a row mask), plain and residual lists: `validate`
// checks the argument errors of the wrapper and of the C ABI (no device needed -- they come before any device work);
// `run in out` searches the codes of `in` under its mask and writes the results for the driver
// (tests/test_cpp_ivfpq_filter.py) to compare with the numpy statement (tests/ref_pq_filter.py).
//   in : u64 n, u64 m, u64 k, u64 sd, u64 nq, u64 topk, u64 nlist, u64 nprobe, f32 coarse [nlist][m sd], f32 codebooks
//        [m][k][sd], u32 lists [n], u8 codes [n][m], f32 queries [nq][m sd], u8 allowed [n]
//   out: for each of the three metrics, plain then residual: u32 idx [nq][topk], f32 dist [nq][topk]
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

// the wrapper's checks on an index of 70 rows (3 mask words) in 4 lists, dim 4: none of them reaches the device
static void validate_index(bool residual) {
    using K = vq::VqError::Kind;
    const std::size_t n = 70, m = 2, k = 4, sd = 2, nlist = 4;
    std::vector<float> coarse(nlist * m * sd);
    for (std::size_t e = 0; e < coarse.size(); ++e) coarse[e] = (float)e;
    const std::vector<float> cb(m * k * sd, 0.0f);
    std::vector<std::uint32_t> lists(n);
    for (std::size_t i = 0; i < n; ++i) lists[i] = (std::uint32_t)(i % nlist);
    const std::vector<std::uint8_t> codes(n * m, 0);
    vq::IVFPQIndex ix(coarse.data(), nlist, cb.data(), m, k, sd, vq::Distance(), residual);
    ix.add(lists.data(), codes.data(), n);
    const std::vector<float> q(8, 0.0f);
    const std::vector<std::uint32_t> three(3, ~0u), four(4, ~0u);
    EXPECT(ix.size() == 70 && ix.residual() == residual);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 5, 2, nullptr); }) == (int)K::InvalidParameter);  // a NULL mask
    EXPECT(kind_of([&] { ix.search(q, 5, 2, four); }) == (int)K::DimensionMismatch);              // a wrong-size mask
    EXPECT(kind_of([&] { ix.search(q, 5, 2, std::vector<std::uint32_t>()); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([&] { ix.search(std::vector<float>(7, 0.0f), 5, 2, three); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 0, 2, three.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 71, 2, three.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 5, 0, three.data()); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 2, 5, 5, three.data()); }) == (int)K::InvalidParameter);
    EXPECT(ix.search(q.data(), 0, 5, 2, three.data()).idx.empty());  // no queries: the empty result, without a device
    // the mask follows the rows: after an add of 30, 100 rows are 4 words
    ix.add(lists.data(), codes.data(), 30);
    EXPECT(kind_of([&] { ix.search(q, 5, 2, three); }) == (int)K::DimensionMismatch);
    EXPECT(ix.search(q.data(), 0, 5, 2, four.data()).idx.empty());
}

static int validate() {
    validate_index(false);
    validate_index(true);
    // the C ABI: the pointers (the mask among them) come before the index handle, a device mask's alignment too
    const std::vector<float> q(8, 0.0f);
    const std::vector<std::uint32_t> three(3, ~0u);
    std::uint32_t idx[2];
    float dist[2];
    vqhip_ivfpq *fp = reinterpret_cast<vqhip_ivfpq *>(8);  // never dereferenced: a NULL pointer is found first
    const std::uint32_t *odd = reinterpret_cast<const std::uint32_t *>(reinterpret_cast<const char *>(three.data()) + 1);
    EXPECT(vqhip_ivfpq_search_masked(nullptr, q.data(), 2, 1, 1, three.data(), idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfpq_search_masked(fp, q.data(), 2, 1, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfpq_search_masked_device(fp, q.data(), 2, 1, 1, nullptr, idx, dist) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfpq_search_masked_device(nullptr, q.data(), 2, 1, 1, odd, idx, dist) == VQHIP_ERR_INVALID_INPUT);
    EXPECT(std::strstr(vqhip_last_error(), "row mask is not 4-byte aligned") != nullptr);
    EXPECT(vqhip_ivfpq_search_masked_device(nullptr, q.data(), 2, 1, 1, three.data(), idx, dist) == VQHIP_ERR_NULL_PTR);
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

template <class T>
static bool take(FILE *in, std::vector<T> &v) {
    return std::fread(v.data(), sizeof(T), v.size(), in) == v.size();
}

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[8];
    if (std::fread(h, 8, 8, in) != 8) return 2;
    const std::size_t n = h[0], m = h[1], k = h[2], sd = h[3], nq = h[4], topk = h[5], nlist = h[6], nprobe = h[7], d = m * sd;
    std::vector<float> coarse(nlist * d), cb(m * k * sd), queries(nq * d);
    std::vector<std::uint32_t> lists(n);
    std::vector<std::uint8_t> codes(n * m), bytes(n);
    if (!take(in, coarse) || !take(in, cb) || !take(in, lists) || !take(in, codes) || !take(in, queries) || !take(in, bytes)) return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    std::vector<bool> allowed(n);
    for (std::size_t i = 0; i < n; ++i) allowed[i] = bytes[i] != 0;
    const std::vector<std::uint32_t> mask = vq::pack_row_mask(allowed);
    const std::vector<std::uint32_t> ones(mask.size(), ~0u), zeros(mask.size(), 0u);
    const vq::Distance::Kind metrics[] = {vq::Distance::SquaredEuclidean, vq::Distance::Euclidean, vq::Distance::Manhattan};
    for (std::size_t mi = 0; mi < 3; ++mi)
        for (int residual = 0; residual < 2; ++residual) {
            vq::IVFPQIndex ix(coarse.data(), nlist, cb.data(), m, k, sd, vq::Distance(metrics[mi]), residual != 0);
            ix.add(lists.data(), codes.data(), n);
            const auto a = ix.search(queries.data(), nq, topk, nprobe, mask.data());
            const auto v = ix.search(queries, topk, nprobe, mask);  // the vector overload
            EXPECT(a.idx == v.idx && !std::memcmp(a.dist.data(), v.dist.data(), a.dist.size() * 4));
            // all ones: the unmasked call, bit for bit; all zeros: padding
            const auto plain = ix.search(queries.data(), nq, topk, nprobe), full = ix.search(queries.data(), nq, topk, nprobe, ones.data());
            EXPECT(plain.idx == full.idx && !std::memcmp(plain.dist.data(), full.dist.data(), plain.dist.size() * 4));
            const auto none = ix.search(queries.data(), nq, topk, nprobe, zeros.data());
            for (std::size_t e = 0; e < none.idx.size(); ++e)
                EXPECT(none.idx[e] == 0xFFFFFFFFu && none.dist[e] == std::numeric_limits<float>::infinity());
            std::fwrite(a.idx.data(), 4, a.idx.size(), out);
            std::fwrite(a.dist.data(), 4, a.dist.size(), out);
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
