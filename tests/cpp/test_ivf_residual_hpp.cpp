// vq::IVFPQIndex of include/vq.hpp with residual lists: `validate` checks the flag and the host-only calls (no device
// needed); `run in out` searches the residual index of `in` and writes the results for the driver
// (tests/test_cpp_ivf_residual.py) to compare with the numpy statement (tests/ref_ivf_residual.py).
//   in : u64 nlist, u64 m, u64 k, u64 sd, u64 n, u64 nq, u64 topk, u64 nprobe, f32 coarse [nlist][m sd],
//        f32 codebooks [m][k][sd], u32 list ids [n], u8 codes [n][m], f32 queries [nq][m sd]
//   out: for each metric (squared Euclidean, Euclidean, Manhattan): u32 probe [nq][nprobe], u32 idx [nq][topk],
//        f32 dist [nq][topk]
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
    const std::vector<float> coarse(4 * 6, 0.0f), cb(2 * 16 * 3, 0.0f);
    EXPECT(kind_of([&] { vq::IVFPQIndex ix(coarse.data(), 0, cb.data(), 2, 16, 3, vq::Distance(), true); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::IVFPQIndex ix(coarse.data(), 4, cb.data(), 2, 16, 3, vq::Distance(vq::Distance::CosineDistance), true); }) ==
           K::InvalidParameter);
    vq::IVFPQIndex plain(coarse.data(), 4, cb.data(), 2, 16, 3);
    EXPECT(!plain.residual());
    vq::IVFPQIndex ix(coarse.data(), 4, cb.data(), 2, 16, 3, vq::Distance(vq::Distance::Manhattan), true);
    EXPECT(ix.residual());
    std::uint32_t flags = 7;
    const std::uint32_t lists[3] = {0, 3, 3}, bad_lists[3] = {0, 4, 1};
    const std::uint8_t codes[6] = {1, 2, 3, 4, 15, 0};
    EXPECT(kind_of([&] { ix.add(bad_lists, codes, 3); }) == K::InvalidParameter);
    EXPECT(ix.add(lists, codes, 3) == 0 && ix.size() == 3);
    const std::vector<std::uint64_t> sizes = ix.list_sizes();
    EXPECT(sizes.size() == 4 && sizes[0] == 1 && sizes[3] == 2);
    const std::vector<float> q(6, 0.0f);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 1, 5); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 4, 1); }) == K::InvalidParameter);
    // the C ABI under the class: the flag as given, unknown bits refused
    vqhip_ivfpq *h = nullptr;
    EXPECT(vqhip_ivfpq_create_ex(coarse.data(), 4, cb.data(), 2, 16, 3, 1, 2u, &h) == VQHIP_ERR_INVALID_INPUT && !h);
    EXPECT(vqhip_ivfpq_create_ex(coarse.data(), 4, cb.data(), 2, 16, 3, 1, VQHIP_IVF_RESIDUAL, &h) == VQHIP_OK && h);
    EXPECT(vqhip_ivfpq_flags(h, &flags) == VQHIP_OK && flags == VQHIP_IVF_RESIDUAL);
    vqhip_ivfpq_destroy(h);
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[8];
    if (std::fread(h, 8, 8, in) != 8) return 2;
    const std::size_t nlist = h[0], m = h[1], k = h[2], sd = h[3], n = h[4], nq = h[5], topk = h[6], nprobe = h[7];
    std::vector<float> coarse(nlist * m * sd), cb(m * k * sd), queries(nq * m * sd);
    std::vector<std::uint32_t> lists(n);
    std::vector<std::uint8_t> codes(n * m);
    if (std::fread(coarse.data(), 4, coarse.size(), in) != coarse.size() || std::fread(cb.data(), 4, cb.size(), in) != cb.size() ||
        std::fread(lists.data(), 4, n, in) != n || std::fread(codes.data(), 1, codes.size(), in) != codes.size() ||
        std::fread(queries.data(), 4, queries.size(), in) != queries.size())
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const vq::Distance::Kind metrics[] = {vq::Distance::SquaredEuclidean, vq::Distance::Euclidean, vq::Distance::Manhattan};
    for (vq::Distance::Kind mt : metrics) {
        vq::IVFPQIndex ix(coarse.data(), nlist, cb.data(), m, k, sd, vq::Distance(mt), true);
        ix.add(lists.data(), codes.data(), n / 2);
        ix.add(lists.data() + n / 2, codes.data() + (n / 2) * m, n - n / 2);
        EXPECT(ix.residual() && ix.size() == n && ix.nlist() == nlist && ix.dim() == m * sd);
        const std::vector<std::uint32_t> p = ix.probe(queries.data(), nq, nprobe);
        const vq::IVFPQIndex::Result r = ix.search(queries.data(), nq, topk, nprobe);
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
