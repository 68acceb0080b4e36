// Removing rows through include/vq.hpp (vq::IVFPQIndex, vq::IVFFlatIndex, vq::IVFScalarIndex, vq::IVFBinaryIndex):
// `validate` needs no device -- the argument errors of the wrapper and of the C ABI, and removals from indexes that were
// never searched (the host path): size, list sizes, codes / packed and the returned ids against the obvious loop; `run in
// out` adds the rows of `in`, searches (so that the device state exists), removes the rows of its mask and writes what
// each index then answers for the driver (tests/test_cpp_ivf_mutate.py) to compare with fresh indexes over the
// remaining rows.
//   in : u64 n, u64 d, u64 nlist, u64 nq, u64 topk, f32 coarse [nlist][d], u32 lists [n], f32 rows [n][d], u8 remove [n],
//        f32 queries [nq][d]
//   out: for flat, scalar, binary: u64 size, u64 uploads, u32 kept [size], u32 idx [nq][topk], f32 dist [nq][topk]
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

constexpr std::size_t N = 200, NLIST = 5, D = 8;

static std::vector<std::uint32_t> lists_of(std::size_t n) {
    std::vector<std::uint32_t> l(n);
    for (std::size_t i = 0; i < n; ++i) l[i] = (std::uint32_t)((i * 7 + i / 3) % 4);  // list 4 stays empty
    return l;
}
static std::vector<bool> mask_of(std::size_t n) {
    std::vector<bool> m(n, false);
    for (std::size_t i = 0; i < n; ++i) m[i] = (i % 3 == 0) || (i >= 64 && i < 130) || i + 1 == n;
    return m;
}

// a removal on an index that was never searched: the host path.  `holds(ix, kept)` compares what the index stores.
template <class Index, class Holds>
static void host_removals(Index &ix, Holds &&holds) {
    using K = vq::VqError::Kind;
    const std::vector<std::uint32_t> lists = lists_of(N);
    EXPECT(ix.size() == N);
    EXPECT(ix.remove_rows(std::vector<bool>(N, false)).size() == N && ix.size() == N);
    EXPECT(ix.remove_rows(std::vector<std::uint32_t>{}).size() == N && ix.size() == N);
    EXPECT(kind_of([&] { ix.remove_rows(std::vector<bool>(N + 1, false)); }) == (int)K::DimensionMismatch && ix.size() == N);
    EXPECT(kind_of([&] { ix.remove_rows(std::vector<std::uint32_t>{(std::uint32_t)N}); }) == (int)K::InvalidParameter && ix.size() == N);
    const std::vector<bool> m = mask_of(N);
    std::vector<std::uint32_t> want;
    std::vector<std::uint64_t> sizes(NLIST, 0);
    for (std::size_t i = 0; i < N; ++i)
        if (!m[i]) {
            want.push_back((std::uint32_t)i);
            ++sizes[lists[i]];
        }
    const std::vector<std::uint32_t> kept = ix.remove_rows(m);
    EXPECT(kept == want && ix.size() == want.size());
    EXPECT(ix.list_sizes() == sizes);
    holds(ix, kept);
    // by ids, in any order, repeats welcome: rows 1 and 0 of what is left
    const std::vector<std::uint32_t> kept2 = ix.remove_rows(std::vector<std::uint32_t>{1, 0, 1});
    EXPECT(kept2.size() == want.size() - 2 && kept2[0] == 2 && ix.size() == want.size() - 2);
    // every row: allowed on an inverted file, which is then as empty as a created one
    EXPECT(ix.remove_rows(std::vector<bool>(ix.size(), true)).empty() && ix.size() == 0);
    EXPECT(ix.list_sizes() == std::vector<std::uint64_t>(NLIST, 0));
    EXPECT(ix.remove_rows(std::vector<bool>()).empty());
    EXPECT(kind_of([&] { ix.remove_rows(std::vector<std::uint32_t>{0}); }) == (int)K::InvalidParameter);
}

static int validate() {
    std::vector<float> coarse(NLIST * D);
    for (std::size_t i = 0; i < coarse.size(); ++i) coarse[i] = (float)((i * 37) % 11) - 5.0f;
    const std::vector<std::uint32_t> lists = lists_of(N);
    {
        std::vector<float> rows(N * D);
        for (std::size_t i = 0; i < rows.size(); ++i) rows[i] = (float)(i % 97) * 0.25f;
        vq::IVFFlatIndex ix(coarse.data(), NLIST, D);
        EXPECT(ix.add(lists.data(), rows.data(), N) == 0);
        host_removals(ix, [](vq::IVFFlatIndex &, const std::vector<std::uint32_t> &) {});
        EXPECT(ix.add(lists.data(), rows.data(), 40) == 0 && ix.size() == 40);  // later adds work
    }
    {
        std::vector<std::uint8_t> codes(N * D);
        for (std::size_t i = 0; i < codes.size(); ++i) codes[i] = (std::uint8_t)(i * 13);
        vq::IVFScalarIndex ix(coarse.data(), NLIST, D, vq::ScalarQuantizer(-3.0f, 3.0f, 256));
        EXPECT(ix.add_codes(lists.data(), codes.data(), N) == 0);
        host_removals(ix, [&](vq::IVFScalarIndex &x, const std::vector<std::uint32_t> &kept) {
            std::vector<std::uint8_t> want;
            for (std::uint32_t i : kept) want.insert(want.end(), codes.begin() + i * D, codes.begin() + (i + 1) * D);
            EXPECT(x.codes() == want);
        });
        EXPECT(ix.add_codes(lists.data(), codes.data(), 40) == 0 && ix.size() == 40);
        EXPECT(ix.codes() == std::vector<std::uint8_t>(codes.begin(), codes.begin() + 40 * D));
    }
    {
        std::vector<std::uint32_t> words(N);  // D = 8 bits: one word a row, the pad bits zero
        for (std::size_t i = 0; i < N; ++i) words[i] = (std::uint32_t)(i * 29) & 0xFFu;
        vq::IVFBinaryIndex ix(coarse.data(), NLIST, D);
        EXPECT(ix.add_packed(lists.data(), words.data(), N) == 0);
        host_removals(ix, [&](vq::IVFBinaryIndex &x, const std::vector<std::uint32_t> &kept) {
            std::vector<std::uint32_t> want;
            for (std::uint32_t i : kept) want.push_back(words[i]);
            EXPECT(x.packed() == want);
        });
        EXPECT(ix.add_packed(lists.data(), words.data(), 40) == 0 && ix.size() == 40);
    }
    for (int residual = 0; residual < 2; ++residual) {
        const std::size_t m = 2, k = 16, sd = D / m;
        std::vector<float> cb(m * k * sd);
        for (std::size_t i = 0; i < cb.size(); ++i) cb[i] = (float)(i % 19) - 9.0f;
        std::vector<std::uint8_t> codes(N * m);
        for (std::size_t i = 0; i < codes.size(); ++i) codes[i] = (std::uint8_t)((i * 5) % k);
        vq::IVFPQIndex ix(coarse.data(), NLIST, cb.data(), m, k, sd, vq::Distance(), residual != 0);
        EXPECT(ix.add(lists.data(), codes.data(), N) == 0);
        host_removals(ix, [](vq::IVFPQIndex &, const std::vector<std::uint32_t> &) {});
        EXPECT(ix.add(lists.data(), codes.data(), 40) == 0 && ix.size() == 40);
    }
    // the C ABI: NULL arguments before anything else
    const std::vector<std::uint32_t> words(2, 0u);
    std::uint64_t out = 7;
    EXPECT(vqhip_ivfpq_remove(nullptr, words.data(), &out) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_remove(nullptr, words.data(), &out) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfsq_remove(nullptr, words.data(), &out) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfbin_remove(nullptr, words.data(), &out) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfpq_uploads(nullptr, &out) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_uploads(nullptr, &out) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfsq_uploads(nullptr, &out) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfbin_uploads(nullptr, &out) == VQHIP_ERR_NULL_PTR);
    vqhip_ivfflat *raw = nullptr;
    EXPECT(vqhip_ivfflat_create(coarse.data(), NLIST, D, 0, VQHIP_EUCLIDEAN, &raw) == VQHIP_OK);
    EXPECT(vqhip_ivfflat_remove(raw, nullptr, &out) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_remove(raw, words.data(), nullptr) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_uploads(raw, nullptr) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_ivfflat_uploads(raw, &out) == VQHIP_OK && out == 0);
    EXPECT(vqhip_ivfflat_destroy(raw) == VQHIP_OK);
    std::printf("VALIDATE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

template <class T>
static std::vector<T> take(std::FILE *f, std::size_t count) {
    std::vector<T> v(count);
    if (count && std::fread(v.data(), sizeof(T), count, f) != count) {
        std::fprintf(stderr, "short input\n");
        std::exit(2);
    }
    return v;
}
template <class T>
static void put(std::FILE *f, const std::vector<T> &v) {
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

// search (the device state is built), remove on the device, then what the index answers
template <class Index, class Uploads>
static void mutate(Index &ix, Uploads &&uploads, const std::vector<bool> &remove, const std::vector<float> &queries, std::size_t nq,
                   std::size_t topk, std::FILE *out) {
    using K = vq::VqError::Kind;
    (void)ix.search(queries.data(), nq, topk, ix.nlist());
    EXPECT(uploads() == 1);
    const std::vector<std::uint32_t> kept = ix.remove_rows(remove);
    EXPECT(ix.size() == kept.size());
    EXPECT(kind_of([&] { ix.search(queries.data(), nq, ix.size() + 1, 1); }) == (int)K::InvalidParameter || ix.size() >= 1024);
    const auto r = ix.search(queries.data(), nq, topk, ix.nlist());
    const std::vector<std::uint64_t> head{ix.size(), uploads()};
    put(out, head);
    put(out, kept);
    put(out, r.idx);
    put(out, r.dist);
}

static int run(const char *in_path, const char *out_path) {
    std::FILE *in = std::fopen(in_path, "rb"), *out = std::fopen(out_path, "wb");
    if (!in || !out) return 2;
    const std::vector<std::uint64_t> head = take<std::uint64_t>(in, 5);
    const std::size_t n = head[0], d = head[1], nlist = head[2], nq = head[3], topk = head[4];
    const std::vector<float> coarse = take<float>(in, nlist * d);
    const std::vector<std::uint32_t> lists = take<std::uint32_t>(in, n);
    const std::vector<float> rows = take<float>(in, n * d);
    const std::vector<std::uint8_t> rm = take<std::uint8_t>(in, n);
    const std::vector<float> queries = take<float>(in, nq * d);
    std::fclose(in);
    const std::vector<bool> remove(rm.begin(), rm.end());
    vq::IVFFlatIndex flat(coarse.data(), nlist, d, vq::Distance(vq::Distance::CosineDistance));
    flat.add(lists.data(), rows.data(), n);
    mutate(flat, [&] { return flat.uploads(); }, remove, queries, nq, topk, out);
    vq::IVFScalarIndex scalar(coarse.data(), nlist, d, vq::ScalarQuantizer(-3.0f, 3.0f, 256));
    scalar.add_rows(lists.data(), rows.data(), n);
    mutate(scalar, [&] { return scalar.uploads(); }, remove, queries, nq, topk, out);
    vq::IVFBinaryIndex binary(coarse.data(), nlist, d);
    binary.add_rows(lists.data(), rows.data(), n);
    mutate(binary, [&] { return binary.uploads(); }, remove, queries, nq, topk, out);
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
