// vq::IVFScalar4Index of include/vq.hpp.
//   validate    the argument errors and the host-only calls (construction, add_codes, add_packed, codes, packed, list
//               sizes, a removal without a device state: no device needed)
//   offsets     nib_word_offset (vq_amd/csrc/nibble_decode.hpp) at the rows the inverted-file kernels hand it -- row
//               off[l] + r of a list's run, row pick[j] of a filtered view -- on both sides of byte 2^31 and 2^32 of the
//               words; stands in for a GPU test over 4 GB of words
//   run in out  create, add, search, remove, search on the GPU; the results go to the driver (tests/test_cpp_ivfsq4.py) to
//               compare with the numpy statement, and are compared here with vq::IVFScalarIndex over the same codes
//   in : u64 nlist, u64 dim, u64 n, u64 nq, u64 topk, u64 nprobe, f32 min, f32 max, u64 levels, f32 coarse [nlist][dim],
//        u32 list ids [n], u8 codes [n][dim], f32 rows [n][dim], f32 queries [nq][dim], u8 remove [n]; the first third of
//        the rows is added as codes, the second as packed words, the last as f32 rows
//   out: u8 codes [n][dim] of the index, then for each metric of vq::Distance (squared Euclidean, Euclidean, Manhattan,
//        cosine): u32 probe [nq][nprobe], u32 idx [nq][topk], f32 dist [nq][topk], and after the removal u32 idx, f32 dist
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nibble_decode.hpp"
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

static std::vector<std::uint32_t> pack4(const std::uint8_t *codes, std::size_t n, std::size_t dim) {
    const std::size_t W = (dim + 7) / 8;
    std::vector<std::uint32_t> w(n * W, 0u);
    for (std::size_t i = 0; i < n; ++i)
        for (std::size_t t = 0; t < dim; ++t) w[i * W + t / 8] |= (std::uint32_t)codes[i * dim + t] << (4 * (t % 8));
    return w;
}

static int validate() {
    using K = vq::VqError::Kind;
    const std::vector<float> coarse(4 * 6, 0.0f);
    const vq::ScalarQuantizer sq(-3.5f, 200.0f, 5);
    EXPECT(kind_of([&] { vq::IVFScalar4Index ix(coarse.data(), 0, 6, sq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::IVFScalar4Index ix(coarse.data(), 65537, 6, sq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::IVFScalar4Index ix(coarse.data(), 4, 0, sq); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::IVFScalar4Index ix(coarse.data(), 4, 6, vq::ScalarQuantizer(0.0f, 1.0f, 17)); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { vq::IVFScalar4Index ix(coarse.data(), 4, 6, vq::ScalarQuantizer(0.0f, 1.0f, 256)); }) == K::InvalidParameter);
    vq::IVFScalar4Index two(coarse.data(), 4, 6, vq::ScalarQuantizer(0.0f, 1.0f, 2)), sixteen(coarse.data(), 4, 6, vq::ScalarQuantizer(0.0f, 1.0f, 16));
    EXPECT(two.quantizer().levels() == 2 && sixteen.quantizer().levels() == 16);
    vq::IVFScalar4Index cosine(coarse.data(), 4, 6, vq::ScalarQuantizer(-3e38f, 3e38f, 2), vq::Distance(vq::Distance::CosineDistance));
    EXPECT(cosine.size() == 0 && cosine.codes().empty() && cosine.packed().empty() && cosine.words() == 1);
    vq::IVFScalar4Index ix(coarse.data(), 4, 6, sq);
    const std::uint32_t lists[3] = {0, 3, 3}, bad_lists[3] = {0, 4, 1};
    std::vector<std::uint8_t> codes(3 * 6);
    for (std::size_t e = 0; e < codes.size(); ++e) codes[e] = (std::uint8_t)((e + 3) % 16);  // codes >= levels are legal
    const std::vector<std::uint32_t> words = pack4(codes.data(), 3, 6);
    const std::vector<float> rows(3 * 6, 1.0f);
    EXPECT(kind_of([&] { ix.add_codes(bad_lists, codes.data(), 3); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.add_packed(bad_lists, words.data(), 3); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.add_rows(bad_lists, rows.data(), 3); }) == K::InvalidParameter);
    std::vector<std::uint8_t> c16 = codes;
    c16[17] = 16;
    EXPECT(kind_of([&] { ix.add_codes(lists, c16.data(), 3); }) == K::InvalidParameter);
    std::vector<std::uint32_t> wpad = words;
    wpad[1] |= 1u << 24;  // dimension 6 of a row of 6
    EXPECT(kind_of([&] { ix.add_packed(lists, wpad.data(), 3); }) == K::InvalidParameter);
    EXPECT(ix.size() == 0);  // the refused adds left the index as it was
    EXPECT(ix.add_codes(lists, codes.data(), 3) == 0 && ix.add_packed(lists, words.data(), 1) == 3 && ix.size() == 4);
    EXPECT(ix.add_rows(lists, rows.data(), 0) == 4);
    std::vector<std::uint64_t> sizes = ix.list_sizes();
    EXPECT(sizes.size() == 4 && sizes[0] == 2 && sizes[1] == 0 && sizes[2] == 0 && sizes[3] == 2);
    const std::vector<std::uint8_t> back = ix.codes();
    EXPECT(back.size() == 4 * 6 && !std::memcmp(back.data(), codes.data(), 18) && !std::memcmp(back.data() + 18, codes.data(), 6));
    const std::vector<std::uint32_t> wback = ix.packed();
    EXPECT(wback.size() == 4 && !std::memcmp(wback.data(), words.data(), 12) && wback[3] == words[0]);
    EXPECT(ix.nlist() == 4 && ix.dim() == 6 && ix.words() == 1 && ix.quantizer().levels() == 5);
    const std::vector<float> q(6, 0.0f);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 1, 0); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 1, 5); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 5, 1); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.search(q.data(), 1, 0, 1); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.probe(q.data(), 1, 5); }) == K::InvalidParameter);
    EXPECT(kind_of([&] { ix.range_search(q.data(), 1, q.data(), 5); }) == K::InvalidParameter);
    EXPECT(ix.search(q.data(), 0, 2, 2).idx.empty() && ix.probe(q.data(), 0, 2).empty());
    // a removal without a device state is the host's
    const std::vector<std::uint32_t> kept = ix.remove_rows(std::vector<bool>{false, true, false, true});
    EXPECT(kept.size() == 2 && kept[0] == 0 && kept[1] == 2 && ix.size() == 2 && ix.uploads() == 0);
    sizes = ix.list_sizes();
    EXPECT(sizes[0] == 1 && sizes[3] == 1);
    const std::vector<std::uint32_t> wkept = ix.packed();
    EXPECT(wkept.size() == 2 && wkept[0] == words[0] && wkept[1] == words[2]);
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

// The word offsets of the two kernels' row numbers.  The tile kernel fills from row (uint64_t)row0 + r0 + r, the scan kernel
// walks row (uint64_t)seg[slot] + (pos - pref[slot]): both off[l] plus a row of the list, the sum taken in 64 bits; a
// filtered view hands (uint64_t)pick[j].  W words a row, so the byte of a row's first word is 4 W row.
static int offsets() {
    const std::uint64_t two31 = std::uint64_t(1) << 31, two32 = std::uint64_t(1) << 32;
    for (std::uint32_t dim : {8u, 100u, 1024u, 1100u}) {
        const std::uint32_t W = vqhip::nib_row_words(dim);
        EXPECT(W == (dim + 7) / 8);
        for (std::uint64_t edge : {two31, two32}) {
            const std::uint64_t first_past = (edge + 4ull * W - 1) / (4ull * W);  // the first row that starts at or past the edge
            for (std::int64_t delta = -2; delta <= 2; ++delta) {
                const std::uint64_t row = first_past + (std::uint64_t)delta;
                if (row >= two32) continue;  // (n < 2^32)
                // the row as the r-th of a list that starts 1000 rows (or as many as there are) before it
                const std::uint32_t r = (std::uint32_t)(row < 1000 ? row : 1000), off_l = (std::uint32_t)(row - r);
                for (std::uint32_t t0 : {0u, 32u, 1024u}) {
                    if (t0 >= dim) continue;
                    const std::uint64_t got = vqhip::nib_word_offset((std::uint64_t)off_l + r, W, t0);
                    EXPECT(got == row * W + t0 / 8);
                    const std::uint64_t row_byte = 4 * (got - t0 / 8);  // rows on both sides of the edge
                    EXPECT(delta < 0 ? row_byte < edge : row_byte >= edge);
                    const std::uint32_t pick_j = (std::uint32_t)row;  // the same row through a view
                    EXPECT(vqhip::nib_word_offset((std::uint64_t)pick_j, W, t0) == got);
                    // a 32-bit product would have wrapped here: the test is sharp
                    if (got > 0xFFFFFFFFull) EXPECT((std::uint64_t)(std::uint32_t)((std::uint32_t)row * W + t0 / 8) != got);
                }
            }
        }
        // the last row an index can hold: the sum off[l] + r itself needs no more than 32 bits, its product with W does
        const std::uint64_t last = two32 - 2;
        EXPECT(vqhip::nib_word_offset((std::uint64_t)0xFFFFFF00u + 0xFEu, W, 0) == last * W);
    }
    std::printf("OFFSETS_%s\n", fails ? "FAILED" : "OK");
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
    std::vector<std::uint8_t> codes(n * dim), remove(n);
    if (std::fread(coarse.data(), 4, coarse.size(), in) != coarse.size() || std::fread(lists.data(), 4, n, in) != n ||
        std::fread(codes.data(), 1, codes.size(), in) != codes.size() || std::fread(rows.data(), 4, rows.size(), in) != rows.size() ||
        std::fread(queries.data(), 4, queries.size(), in) != queries.size() || std::fread(remove.data(), 1, n, in) != n)
        return 2;
    std::fclose(in);
    FILE *out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const vq::ScalarQuantizer sq(mm[0], mm[1], (std::size_t)levels);
    const vq::Distance::Kind metrics[] = {vq::Distance::SquaredEuclidean, vq::Distance::Euclidean, vq::Distance::Manhattan,
                                          vq::Distance::CosineDistance};
    const std::size_t a = n / 3, b = 2 * n / 3;
    const std::vector<std::uint32_t> words = pack4(codes.data() + a * dim, b - a, dim);
    const std::vector<bool> gone(remove.begin(), remove.end());
    bool first = true;
    for (vq::Distance::Kind mt : metrics) {
        vq::IVFScalar4Index ix(coarse.data(), nlist, dim, sq, vq::Distance(mt));
        ix.add_codes(lists.data(), codes.data(), a);
        ix.add_packed(lists.data() + a, words.data(), b - a);
        ix.add_rows(lists.data() + b, rows.data() + b * dim, n - b);
        EXPECT(ix.size() == n && ix.nlist() == nlist && ix.dim() == dim);
        const std::vector<std::uint8_t> c = ix.codes();
        if (first) {
            std::fwrite(c.data(), 1, c.size(), out);
            first = false;
        }
        vq::IVFScalarIndex ref(coarse.data(), nlist, dim, sq, vq::Distance(mt));  // the same codes, one byte each
        ref.add_codes(lists.data(), c.data(), n);
        const std::vector<std::uint32_t> p = ix.probe(queries.data(), nq, nprobe);
        vq::IVFScalar4Index::Result r = ix.search(queries.data(), nq, topk, nprobe);
        vq::IVFScalarIndex::Result w = ref.search(queries.data(), nq, topk, nprobe);
        EXPECT(p == ref.probe(queries.data(), nq, nprobe) && r.idx == w.idx);
        EXPECT(!std::memcmp(r.dist.data(), w.dist.data(), 4 * r.dist.size()));
        std::fwrite(p.data(), 4, p.size(), out);
        std::fwrite(r.idx.data(), 4, r.idx.size(), out);
        std::fwrite(r.dist.data(), 4, r.dist.size(), out);
        const std::uint64_t uploads = ix.uploads();
        const std::vector<std::uint32_t> kept = ix.remove_rows(gone);
        EXPECT(kept == ref.remove_rows(gone) && ix.size() == kept.size() && ix.uploads() == uploads && uploads == 1);
        r = ix.search(queries.data(), nq, topk, nprobe);
        w = ref.search(queries.data(), nq, topk, nprobe);
        EXPECT(r.idx == w.idx && !std::memcmp(r.dist.data(), w.dist.data(), 4 * r.dist.size()) && ix.uploads() == uploads);
        std::fwrite(r.idx.data(), 4, r.idx.size(), out);
        std::fwrite(r.dist.data(), 4, r.dist.size(), out);
    }
    std::fclose(out);
    std::printf("RUN_%s backend=%s\n", fails ? "FAILED" : "OK", vq::get_simd_backend().c_str());
    return fails ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "validate")) return validate();
    if (argc >= 2 && !std::strcmp(argv[1], "offsets")) return offsets();
    if (argc >= 4 && !std::strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    std::fprintf(stderr, "usage: %s validate | offsets | run in out\n", argv[0]);
    return 2;
}
