// vq::IVFScalarIndex of include/vq.hpp: `validate` checks the argument errors and the host-only calls (construction,
// add_codes, codes, list sizes: no device needed); `run in out` searches the index of `in` and writes the results for the
// driver (tests/test_cpp_ivfsq.py) to compare with the numpy statement.
//   in : u64 nlist, u64 dim, u64 n, u64 nq, u64 topk, u64 nprobe, f32 min, f32 max, u64 levels, f32 coarse [nlist][dim],
//        u32 list ids [n], u8 codes [n][dim], f32 rows [n][dim], f32 queries [nq][dim]; the first n / 2 rows are added as
//        codes, the others as rows
//   out: u8 codes [n][dim] of the index, then for each metric of vq::Distance (squared Euclidean, Euclidean, Manhattan,
//        cosine): u32 probe [nq][nprobe], u32 idx [nq][topk], f32 dist [nq][topk]
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
    const std::vector<float> coarse(4 * 6, 0.0f);
    const vq::ScalarQuantizer sq(-3.0f, 5.0f, 17);
    EXPECT(kind_of([&] { vq::IVFScalarIndex ix(coarse.data(), 0, 6, sq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::IVFScalarIndex ix(coarse.data(), 65537, 6, sq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::IVFScalarIndex ix(coarse.data(), 4, 0, sq); }) == K::InvalidParameter);
    vq::IVFScalarIndex cosine(coarse.data(), 4, 6, vq::ScalarQuantizer(-3e38f, 3e38f, 2), vq::Distance(vq::Distance::CosineDistance));
    EXPECT(cosine.size() == 0 && cosine.quantizer().levels() == 2 && cosine.codes().empty());
    vq::IVFScalarIndex ix(coarse.data(), 4, 6, sq);
    const std::uint32_t lists[3] = {0, 3, 3}, bad_lists[3] = {0, 4, 1};
    std::vector<std::uint8_t> codes(3 * 6);
    for (std::size_t e = 0; e < codes.size(); ++e) codes[e] = (std::uint8_t)(240 + e);  // codes >= levels are legal
    const std::vector<float> rows(3 * 6, 1.0f);
    EXPECT(kind_of([&] { ix.add_codes(bad_lists, codes.data(), 3); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.add_rows(bad_lists, rows.data(), 3); }) == K::InvalidParameter);
    EXPECT(ix.add_codes(lists, codes.data(), 3) == 0 && ix.add_codes(lists, codes.data(), 1) == 3 && ix.size() == 4);
    EXPECT(ix.add_rows(lists, rows.data(), 0) == 4);
    const std::vector<std::uint64_t> sizes = ix.list_sizes();
    EXPECT(sizes.size() == 4 && sizes[0] == 2 && sizes[1] == 0 && sizes[2] == 0 && sizes[3] == 2);
    const std::vector<std::uint8_t> back = ix.codes();
    EXPECT(back.size() == 4 * 6 && !std::memcmp(back.data(), codes.data(), 18) && !std::memcmp(back.data() + 18, codes.data(), 6));
    EXPECT(ix.nlist() == 4 && ix.dim() == 6 && ix.quantizer().levels() == 17);
    const std::vector<float> q(6, 0.0f);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 1, 0); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 1, 5); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 5, 1); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 0, 1); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.probe(q.data(), 1, 5); }) == K::InvalidParameter);
    EXPECT(ix.search(q.data(), 0, 2, 2).idx.empty() && ix.probe(q.data(), 0, 2).empty());
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

static int run(const char *in_path, const char *out_path) {
    FILE *in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::uint64_t h[6], levels;
    float mm[2];
    if (std::fread(h, 8, 6, in) != 6 || std::fread(mm, 4, 2, in) != 2 || std::fread(&levels, 8, 1, in) != 1) return 2;
    const std::size_t nlist = h[0], dim = h[1], n = h[2], nq = h[3], topk = h[4], nprobe = h[5];
    std::vector<float> coarse(nlist * dim), rows(n * dim), queries(nq * dim);
    std::vector<std::uint32_t> lists(n);
    std::vector<std::uint8_t> codes(n * dim);
    if (std::fread(coarse.data(), 4, coarse.size(), in) != coarse.size() || std::fread(lists.data(), 4, n, in) != n ||
        std::fread(codes.data(), 1, codes.size(), in) != codes.size() || std::fread(rows.data(), 4, rows.size(), in) != rows.size() ||
        std::fread(queries.data(), 4, queries.size(), in) != queries.size())
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const vq::ScalarQuantizer sq(mm[0], mm[1], (std::size_t)levels);
    const vq::Distance::Kind metrics[] = {vq::Distance::SquaredEuclidean, vq::Distance::Euclidean, vq::Distance::Manhattan,
                                          vq::Distance::CosineDistance};
    bool first = true;
    for (vq::Distance::Kind mt : metrics) {
        vq::IVFScalarIndex ix(coarse.data(), nlist, dim, sq, vq::Distance(mt));
        ix.add_codes(lists.data(), codes.data(), n / 2);
        ix.add_rows(lists.data() + n / 2, rows.data() + (n / 2) * dim, n - n / 2);
        EXPECT(ix.size() == n && ix.nlist() == nlist && ix.dim() == dim);
        if (first) {
            const std::vector<std::uint8_t> c = ix.codes();
            std::fwrite(c.data(), 1, c.size(), out);
            first = false;
        }
        const std::vector<std::uint32_t> p = ix.probe(queries.data(), nq, nprobe);
        const vq::IVFScalarIndex::Result r = ix.search(queries.data(), nq, topk, nprobe);
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
