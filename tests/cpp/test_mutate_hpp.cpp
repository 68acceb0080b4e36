// Adding and removing rows through include/vq.hpp (vq::FlatIndex, vq::ScalarIndex, vq::BinaryIndex): `validate` checks
// the argument errors of the wrapper and of the C ABI (no device needed -- they come before any device work); `run in
// out` builds each index over the rows of `in`, adds its second block, removes the rows of its mask, and writes what the
// index then holds and answers for the driver (tests/test_cpp_mutate.py) to compare with fresh indexes over
// tests/ref_mutate.py's rows.
//   in : u64 n, u64 b, u64 d, u64 nq, u64 topk, f32 sq_min, f32 sq_max, u64 levels, f32 rows [n][d], f32 added [b][d],
//        u8 remove [n + b], f32 queries [nq][d]
//   out: for flat, scalar, binary: u64 size, u32 ids [b], u32 kept [size], u32 idx [nq][topk], f32 dist [nq][topk]; then
//        the scalar index's codes u8 [size][d] and the binary index's words u32 [size][W]
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
    // remove_mask: ids in any order, repeats welcome; an id at or past n is refused
    const std::vector<bool> m = vq::remove_mask({4, 1, 1}, 6);
    EXPECT(m == std::vector<bool>({false, true, false, false, true, false}));
    EXPECT(vq::remove_mask({}, 3) == std::vector<bool>(3, false));
    EXPECT(kind_of([] { vq::remove_mask({6}, 6); }) == (int)K::InvalidParameter);
    // kept_rows: the mask has n entries and leaves a row; the old ids of the rest, ascending
    EXPECT(vq::detail::kept_rows(m, 6) == std::vector<std::uint32_t>({0, 2, 3, 5}));
    EXPECT(vq::detail::kept_rows(std::vector<bool>(3, false), 3) == std::vector<std::uint32_t>({0, 1, 2}));
    EXPECT(kind_of([&] { vq::detail::kept_rows(m, 5); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([&] { vq::detail::kept_rows(m, 7); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([] { vq::detail::kept_rows(std::vector<bool>(4, true), 4); }) == (int)K::InvalidParameter);
    // check_room: n + b stays below 2^32
    EXPECT(kind_of([] { vq::detail::check_room(10, 0); }) == -1);
    EXPECT(kind_of([] { vq::detail::check_room(10, (std::size_t(1) << 32) - 11); }) == -1);
    EXPECT(kind_of([] { vq::detail::check_room(10, (std::size_t(1) << 32) - 10); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([] { vq::detail::check_room(1, std::size_t(1) << 32); }) == (int)K::InvalidParameter);
    // the C ABI: the handle comes first (before n_add == 0 too), then the other pointers, a device mask's alignment
    const std::vector<float> rows(8, 0.0f);
    const std::vector<std::uint32_t> words(2, 0u);
    const std::uint32_t *odd = reinterpret_cast<const std::uint32_t *>(reinterpret_cast<const char *>(words.data()) + 1);
    std::uint64_t gone = 7;
    EXPECT(vqhip_flat_add(nullptr, rows.data(), 1) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_flat_add(nullptr, rows.data(), 0) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_flat_add_device(nullptr, rows.data(), 1) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_sqindex_add_rows(nullptr, rows.data(), 1) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_sqindex_add_rows_device(nullptr, rows.data(), 1) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_sqindex_add_codes(nullptr, reinterpret_cast<const std::uint8_t *>(rows.data()), 1) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_sqindex_add_codes_device(nullptr, rows.data(), 1) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_add(nullptr, rows.data(), VQHIP_BINARY_F32, 1) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_add_device(nullptr, rows.data(), VQHIP_BINARY_F32, 1) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_flat_remove(nullptr, words.data(), &gone) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_flat_remove_device(nullptr, words.data(), &gone) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_sqindex_remove(nullptr, words.data(), &gone) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_sqindex_remove_device(nullptr, words.data(), &gone) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_remove(nullptr, words.data(), &gone) == VQHIP_ERR_NULL_PTR);
    EXPECT(vqhip_binary_remove_device(nullptr, odd, &gone) == VQHIP_ERR_NULL_PTR);
    // without a device an index cannot be built, so its methods have nothing to refuse: the constructor says so
    if (vq::get_simd_backend().find("gfx950") == std::string::npos)
        EXPECT(kind_of([&] { vq::FlatIndex f(rows.data(), 2, 4); }) == (int)K::FfiError);
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

// add, remove, then what the index holds and answers
template <class Index>
static void mutate(Index &ix, const std::vector<float> &added, std::size_t b, const std::vector<bool> &remove,
                   const std::vector<float> &queries, std::size_t topk, std::FILE *out) {
    using K = vq::VqError::Kind;
    const std::size_t n = ix.size();
    EXPECT(ix.add(added.data(), 0).empty() && ix.size() == n);
    EXPECT(ix.remove_rows(std::vector<bool>(n, false)).size() == n && ix.size() == n);
    EXPECT(kind_of([&] { ix.remove_rows(std::vector<bool>(n, true)); }) == (int)K::InvalidParameter && ix.size() == n);
    EXPECT(kind_of([&] { ix.remove_rows(std::vector<bool>(n + 1, false)); }) == (int)K::DimensionMismatch);
    EXPECT(kind_of([&] { ix.remove_rows(std::vector<std::uint32_t>{(std::uint32_t)n}); }) == (int)K::InvalidParameter);
    EXPECT(kind_of([&] { ix.add(static_cast<const float *>(nullptr), 1); }) == (int)K::InvalidParameter && ix.size() == n);
    const std::vector<std::uint32_t> ids = ix.add(added.data(), b);
    EXPECT(ix.size() == n + b);
    const std::vector<std::uint32_t> kept = ix.remove_rows(remove);
    EXPECT(ix.size() == kept.size());
    EXPECT(kind_of([&] { ix.search(queries, ix.size() + 1); }) == (int)K::InvalidParameter || ix.size() >= 1024);
    const auto r = ix.search(queries, topk);
    const std::vector<std::uint64_t> size(1, ix.size());
    put(out, size);
    put(out, ids);
    put(out, kept);
    put(out, r.idx);
    put(out, r.dist);
}

static int run(const char *in_path, const char *out_path) {
    std::FILE *in = std::fopen(in_path, "rb"), *out = std::fopen(out_path, "wb");
    if (!in || !out) return 2;
    const std::vector<std::uint64_t> head = take<std::uint64_t>(in, 5);
    const std::size_t n = head[0], b = head[1], d = head[2], nq = head[3], topk = head[4];
    const std::vector<float> sq = take<float>(in, 2);
    const std::size_t levels = take<std::uint64_t>(in, 1)[0];
    const std::vector<float> rows = take<float>(in, n * d), added = take<float>(in, b * d);
    const std::vector<std::uint8_t> rm = take<std::uint8_t>(in, n + b);
    const std::vector<float> queries = take<float>(in, nq * d);
    std::fclose(in);
    const std::vector<bool> remove(rm.begin(), rm.end());
    vq::FlatIndex flat(rows.data(), n, d, vq::Distance(vq::Distance::CosineDistance));
    mutate(flat, added, b, remove, queries, topk, out);
    vq::ScalarIndex scalar(rows.data(), n, d, vq::ScalarQuantizer(sq[0], sq[1], levels));
    mutate(scalar, added, b, remove, queries, topk, out);
    vq::BinaryIndex binary(rows.data(), n, d);
    mutate(binary, added, b, remove, queries, topk, out);
    put(out, scalar.codes());
    put(out, binary.packed());
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
