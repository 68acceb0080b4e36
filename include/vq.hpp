// vq.hpp -- C++ host mirror of the reference's public interface for the hot path, over libvqhip.
//
// The reference is a Rust crate (no Rust toolchain in this image), so the compiled-language host
// side above the C ABI (include/vqhip.h) is this header: same type and method names, argument
// meaning, defaults and error behaviour as
//   vq::Distance           src/core/distance.rs:8-64
//   vq::VqError            src/core/error.rs:4-28   (what() == the Rust Display text)
//   vq::ProductQuantizer   src/pq.rs:83-210         (new / getters / Quantizer::quantize / dequantize)
//   vq::TSVQ               src/tsvq.rs:195-266
//   vq::ScalarQuantizer    src/sq.rs                (new / getters / quantize / dequantize)
//   vq::BinaryQuantizer    src/bq.rs
//   vq::lbg_quantize       src/core/vector.rs:390-461
// Validation happens before anything touches the device (same order and messages as the
// reference); the bodies run on the MI355X.  Random draws (src/core/vector.rs:412-413, 448-452) come
// from the documented SplitMix64 sampler also used by the Python mirror (vq_amd/rng.py) -- rand's
// StdRng stream is not reproducible outside Rust -- or from the caller (`init_rows`).
//
// Header-only, C++17; link with -lvqhip.  Thread-safe per object like the reference's plain-data types (`Send + Sync`,
// src/pq.rs:39-45): the `const` methods (`quantize`, `dequantize`, the getters) may be called on one object from any
// number of threads at once -- every libvqhip handle carries its own lock and hands its stream's tail over between
// threads (include/vqhip.h "Threads"; held by tests/cpp/test_vq_hpp.cpp's std::thread case).
#ifndef VQ_HPP
#define VQ_HPP

#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "vqhip.h"

namespace vq {

// ---------------------------------------------------------------------------- errors ----
class VqError : public std::runtime_error {
   public:
    enum class Kind { DimensionMismatch, EmptyInput, InvalidParameter, InvalidData, FfiError };
    Kind kind;
    std::size_t expected = 0, found = 0;  // DimensionMismatch
    std::string parameter, reason;        // InvalidParameter

    static VqError DimensionMismatch(std::size_t expected, std::size_t found) {
        VqError e(Kind::DimensionMismatch, "Dimension mismatch: expected " + std::to_string(expected) + ", found " +
                                               std::to_string(found));
        e.expected = expected;
        e.found = found;
        return e;
    }
    static VqError EmptyInput() { return VqError(Kind::EmptyInput, "Empty input: at least one vector is required"); }
    static VqError InvalidParameter(const std::string &parameter, const std::string &reason) {
        VqError e(Kind::InvalidParameter, "Invalid parameter '" + parameter + "': " + reason);
        e.parameter = parameter;
        e.reason = reason;
        return e;
    }
    static VqError InvalidData(const std::string &what) { return VqError(Kind::InvalidData, "Invalid data: " + what); }
    static VqError FfiError(const std::string &what) { return VqError(Kind::FfiError, "FFI error: " + what); }

   private:
    VqError(Kind k, const std::string &msg) : std::runtime_error(msg), kind(k) {}
};

namespace detail {
inline void check(int status) {
    if (status != VQHIP_OK) throw VqError::FfiError(vqhip_last_error());
}
}  // namespace detail

// ------------------------------------------------------------------------------- f16 ----
// `half::f16` stand-in: the bits the device wrote (IEEE binary16, round-to-nearest-even)
struct f16 {
    std::uint16_t bits = 0;
    float to_f32() const {
        const std::uint32_t s = (std::uint32_t)(bits & 0x8000u) << 16, e = (bits >> 10) & 0x1Fu, m = bits & 0x3FFu;
        std::uint32_t u;
        if (e == 0) {
            if (m == 0) {
                u = s;
            } else {  // subnormal: normalise
                int sh = 0;
                std::uint32_t mm = m;
                while (!(mm & 0x400u)) {
                    mm <<= 1;
                    ++sh;
                }
                u = s | ((std::uint32_t)(127 - 15 - sh + 1) << 23) | ((mm & 0x3FFu) << 13);
            }
        } else if (e == 31) {
            u = s | 0x7F800000u | (m << 13);
        } else {
            u = s | ((e + 112u) << 23) | (m << 13);
        }
        float f;
        std::memcpy(&f, &u, 4);
        return f;
    }
    bool operator==(const f16 &o) const { return bits == o.bits; }
};

// -------------------------------------------------------------------------- Distance ----
class Distance {
   public:
    enum Kind : int {
        SquaredEuclidean = VQHIP_SQUARED_EUCLIDEAN,
        Euclidean = VQHIP_EUCLIDEAN,
        Manhattan = VQHIP_MANHATTAN,
        CosineDistance = VQHIP_COSINE,
    };
    constexpr Distance(Kind k = Euclidean) : kind_(k) {}
    constexpr Kind kind() const { return kind_; }
    constexpr bool operator==(const Distance &o) const { return kind_ == o.kind_; }
    // src/core/distance.rs:22-29
    const char *name() const {
        switch (kind_) {
            case SquaredEuclidean: return "squared_euclidean";
            case Euclidean: return "euclidean";
            case Manhattan: return "manhattan";
            default: return "cosine";
        }
    }
    // src/core/distance.rs:48-64 (scalar kernels; one pair per call, evaluated on the device)
    float compute(const float *a, std::size_t a_len, const float *b, std::size_t b_len) const {
        if (a_len != b_len) throw VqError::DimensionMismatch(a_len, b_len);
        float out = 0.0f;
        if (a_len == 0) return kind_ == CosineDistance ? 1.0f : 0.0f;
        detail::check(vqhip_distance_batch((int)kind_, a, b, 1, (std::uint32_t)a_len, &out));
        return out;
    }
    float compute(const std::vector<float> &a, const std::vector<float> &b) const {
        return compute(a.data(), a.size(), b.data(), b.size());
    }

   private:
    Kind kind_;
};

// ------------------------------------------------------------------------------- rng ----
// vq_amd/rng.py in C++: SplitMix64, Lemire's bounded integers, Floyd's sampling
class HostRng {
   public:
    explicit HostRng(std::uint64_t seed) : state_(seed) {}
    std::uint64_t next_u64() {
        state_ += 0x9E3779B97F4A7C15ull;
        std::uint64_t z = state_;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    std::uint64_t below(std::uint64_t n) {
        const std::uint64_t threshold = (0 - n) % n;
        for (;;) {
            const unsigned __int128 m = (unsigned __int128)next_u64() * n;
            if ((std::uint64_t)m >= threshold) return (std::uint64_t)(m >> 64);
        }
    }
    std::uint64_t choose(std::uint64_t n) { return below(n); }
    std::vector<std::uint64_t> choose_multiple(std::uint64_t n, std::uint64_t k) {
        std::unordered_set<std::uint64_t> chosen;
        std::vector<std::uint64_t> out;
        out.reserve(k);
        for (std::uint64_t j = n - k; j < n; ++j) {
            const std::uint64_t t = below(j + 1), pick = chosen.count(t) ? j : t;
            chosen.insert(pick);
            out.push_back(pick);
        }
        return out;
    }

   private:
    std::uint64_t state_;
};

namespace detail {

struct DatasetDel {
    void operator()(vqhip_dataset *p) const { vqhip_dataset_destroy(p); }
};
struct KMeansDel {
    void operator()(vqhip_kmeans *p) const { vqhip_kmeans_destroy(p); }
};
struct EncoderDel {
    void operator()(vqhip_pq_encoder *p) const { vqhip_pq_encoder_destroy(p); }
};
struct TsvqDel {
    void operator()(vqhip_tsvq *p) const { vqhip_tsvq_destroy(p); }
};
struct MTsvqDel {
    void operator()(vqhip_mtsvq *p) const { (void)vqhip_mtsvq_destroy(p); }
};

// `&[&[f32]]` -> contiguous [n][dim] with the reference's checks (src/pq.rs:91-104, src/tsvq.rs:196-210)
inline std::vector<float> flatten(const std::vector<std::vector<float>> &rows, std::size_t *dim) {
    if (rows.empty()) throw VqError::EmptyInput();
    *dim = rows[0].size();
    for (const auto &r : rows)
        if (r.size() != *dim) throw VqError::DimensionMismatch(*dim, r.size());
    std::vector<float> flat(rows.size() * *dim);
    for (std::size_t i = 0; i < rows.size(); ++i)
        if (*dim) std::memcpy(flat.data() + i * *dim, rows[i].data(), *dim * sizeof(float));
    return flat;
}

// src/core/vector.rs:396-410
inline void check_lbg_params(std::size_t n, std::size_t k) {
    if (n == 0) throw VqError::EmptyInput();
    if (k == 0) throw VqError::InvalidParameter("k", "must be greater than 0");
    if (n < k)
        throw VqError::InvalidParameter(
            "k", "not enough data points (" + std::to_string(n) + ") for " + std::to_string(k) + " clusters");
}

// control flow of lbg_quantize (src/core/vector.rs:412-460) for all m subspaces of a resident
// data set; the device does each Lloyd iteration, the host keeps the RNG (seed + s per subspace,
// src/pq.rs:130) and the convergence / empty-cluster logic
inline std::vector<float> fit_codebooks(vqhip_dataset *ds, std::uint64_t n, std::uint32_t dim, std::uint32_t m,
                                        std::uint32_t k, std::size_t max_iters, std::uint64_t seed,
                                        const std::uint64_t *init_rows = nullptr) {
    std::vector<HostRng> rngs;
    for (std::uint32_t s = 0; s < m; ++s) rngs.emplace_back(seed + s);
    std::vector<std::uint64_t> init((std::size_t)m * k);
    if (init_rows) {
        std::memcpy(init.data(), init_rows, init.size() * 8);
    } else {
        for (std::uint32_t s = 0; s < m; ++s) {
            const auto rows = rngs[s].choose_multiple(n, k);
            std::memcpy(init.data() + (std::size_t)s * k, rows.data(), (std::size_t)k * 8);
        }
    }
    vqhip_kmeans *raw = nullptr;
    check(vqhip_kmeans_create(ds, m, k, &raw));
    std::unique_ptr<vqhip_kmeans, KMeansDel> km(raw);
    check(vqhip_kmeans_init_from_rows(km.get(), init.data()));
    std::vector<std::uint8_t> active(m, 1), changed(m, 0);
    std::vector<std::uint32_t> counts((std::size_t)m * k);
    for (std::size_t it = 0; it < max_iters; ++it) {
        bool any = false;
        for (auto a : active) any = any || a;
        if (!any) break;
        check(vqhip_kmeans_step(km.get(), counts.data(), changed.data()));
        for (std::uint32_t s = 0; s < m; ++s) {
            if (!active[s]) continue;
            for (std::uint32_t j = 0; j < k; ++j)  // empty clusters in ascending j, vector.rs:448-452
                if (counts[(std::size_t)s * k + j] == 0)
                    check(vqhip_kmeans_patch_from_row(km.get(), s, j, rngs[s].choose(n)));
            if (!changed[s]) active[s] = 0;  // vector.rs:455-457
        }
        check(vqhip_kmeans_set_active(km.get(), active.data()));
    }
    std::vector<float> cb((std::size_t)m * k * (dim / m));
    check(vqhip_kmeans_get_centroids(km.get(), cb.data()));
    return cb;
}

struct MDatasetDel {
    void operator()(vqhip_mdataset *p) const { (void)vqhip_mdataset_destroy(p); }
};
struct MKMeansDel {
    void operator()(vqhip_mkmeans *p) const { (void)vqhip_mkmeans_destroy(p); }
};
struct MEncoderDel {
    void operator()(vqhip_mpq_encoder *p) const { (void)vqhip_mpq_encoder_destroy(p); }
};

// the same control flow with the training batch partitioned over several GPUs of THIS process (include/vqhip.h "one
// call, one process, several GPUs": the ranks of the row-sharded fit are worker threads inside the library; each Lloyd
// iteration all-reduces the per-cluster sums).  The loop's decisions are taken on the device (vqhip_mkmeans_run): it
// comes back when the iterations are used up, when every subspace has converged, or paused behind an iteration that
// left a cluster empty -- the reseed row is this side's draw (vector.rs:448-452), named by its global row id.
inline std::vector<float> fit_codebooks_multi(vqhip_mdataset *ds, std::uint64_t n, std::uint32_t dim, std::uint32_t m,
                                              std::uint32_t k, std::size_t max_iters, std::uint64_t seed,
                                              const std::uint64_t *init_rows = nullptr) {
    std::vector<HostRng> rngs;
    for (std::uint32_t s = 0; s < m; ++s) rngs.emplace_back(seed + s);
    std::vector<std::uint64_t> init((std::size_t)m * k);
    if (init_rows) {
        std::memcpy(init.data(), init_rows, init.size() * 8);
    } else {
        for (std::uint32_t s = 0; s < m; ++s) {
            const auto rows = rngs[s].choose_multiple(n, k);
            std::memcpy(init.data() + (std::size_t)s * k, rows.data(), (std::size_t)k * 8);
        }
    }
    vqhip_mkmeans *raw = nullptr;
    check(vqhip_mkmeans_create(ds, m, k, &raw));
    std::unique_ptr<vqhip_mkmeans, MKMeansDel> km(raw);
    check(vqhip_mkmeans_init_from_rows(km.get(), init.data()));
    std::vector<std::uint8_t> active(m, 1), changed(m, 0);
    std::vector<std::uint32_t> counts((std::size_t)m * k), iters(m);
    std::size_t done = 0;
    for (;;) {
        bool any = false;
        for (auto a : active) any = any || a;
        if (!any || done >= max_iters) break;
        int paused = 0;
        check(vqhip_mkmeans_run(km.get(), (std::uint32_t)(max_iters - done), iters.data(), counts.data(), changed.data(), &paused));
        std::uint32_t most = 1;
        for (auto x : iters) most = x > most ? x : most;
        done += most;
        check(vqhip_mkmeans_get_active(km.get(), active.data()));  // subspaces that converged inside the call are retired
        if (!paused) continue;
        for (std::uint32_t s = 0; s < m; ++s) {
            if (!active[s]) continue;
            for (std::uint32_t j = 0; j < k; ++j)  // empty clusters in ascending j, vector.rs:448-452
                if (counts[(std::size_t)s * k + j] == 0)
                    check(vqhip_mkmeans_patch_from_row(km.get(), s, j, rngs[s].choose(n)));
            if (!changed[s]) active[s] = 0;  // vector.rs:455-457
        }
        check(vqhip_mkmeans_set_active(km.get(), active.data()));
    }
    std::vector<float> cb((std::size_t)m * k * (dim / m));
    check(vqhip_mkmeans_get_centroids(km.get(), cb.data()));
    return cb;
}

}  // namespace detail

// ------------------------------------------------------------------ ProductQuantizer ----
class ProductQuantizer {
   public:
    // ProductQuantizer::new, src/pq.rs:83-141
    ProductQuantizer(const std::vector<std::vector<float>> &training_data, std::size_t m, std::size_t k,
                     std::size_t max_iters, Distance distance, std::uint64_t seed) {
        std::size_t dim = 0;
        const std::vector<float> flat = detail::flatten(training_data, &dim);
        init(flat.data(), training_data.size(), dim, m, k, max_iters, distance, seed);
    }
    // same, training rows already contiguous [n][dim]
    ProductQuantizer(const float *rows, std::size_t n, std::size_t dim, std::size_t m, std::size_t k,
                     std::size_t max_iters, Distance distance, std::uint64_t seed) {
        if (n == 0) throw VqError::EmptyInput();
        init(rows, n, dim, m, k, max_iters, distance, seed);
    }
    // same call, the training batch partitioned over `devices` (ids of visible GPUs; all_devices() names them all):
    // still ONE call in ONE process -- the ranks are worker threads inside libvqhip (not in the reference: src/pq.rs:83-141
    // has no device argument; the Rust shim passes the visible devices itself)
    ProductQuantizer(const float *rows, std::size_t n, std::size_t dim, std::size_t m, std::size_t k,
                     std::size_t max_iters, Distance distance, std::uint64_t seed, const std::vector<int> &devices) {
        if (n == 0) throw VqError::EmptyInput();
        init(rows, n, dim, m, k, max_iters, distance, seed, devices);
    }
    static std::vector<int> all_devices() {
        std::vector<int> v;
        for (int i = 0; i < vqhip_device_count(); ++i) v.push_back(i);
        return v;
    }

    std::size_t num_subspaces() const { return m_; }
    std::size_t sub_dim() const { return sub_dim_; }
    std::size_t dim() const { return dim_; }
    const char *distance_metric() const { return distance_.name(); }
    const std::vector<float> &codebooks() const { return codebooks_; }  // [m][k][sub_dim]
    std::size_t num_centroids() const { return k_; }

    // Quantizer::quantize, src/pq.rs:167-199
    std::vector<f16> quantize(const float *vector, std::size_t len) const {
        if (len != dim_) throw VqError::DimensionMismatch(dim_, len);
        std::vector<f16> out(dim_);
        detail::check(vqhip_pq_encode(enc_.get(), vector, 1, nullptr, reinterpret_cast<std::uint16_t *>(out.data())));
        return out;
    }
    std::vector<f16> quantize(const std::vector<float> &vector) const { return quantize(vector.data(), vector.size()); }
    // Quantizer::dequantize, src/pq.rs:201-209
    std::vector<float> dequantize(const std::vector<f16> &quantized) const {
        if (quantized.size() != dim_) throw VqError::DimensionMismatch(dim_, quantized.size());
        std::vector<float> out(dim_);
        for (std::size_t i = 0; i < dim_; ++i) out[i] = quantized[i].to_f32();
        return out;
    }

    // batch forms (ROADMAP.md:30 "batch quantization" is open upstream): rows [n][dim]
    std::vector<f16> quantize_batch(const float *rows, std::size_t n) const {
        std::vector<f16> out(n * dim_);
        if (n) detail::check(encode_raw(rows, n, nullptr, reinterpret_cast<std::uint16_t *>(out.data())));
        return out;
    }
    std::vector<std::uint8_t> encode(const float *rows, std::size_t n) const {  // best_idx per subspace, k <= 256
        if (k_ > 256) throw VqError::InvalidParameter("k", "one-byte codes need k <= 256: use encode_wide");
        std::vector<std::uint8_t> codes(n * m_);
        if (n) detail::check(encode_raw(rows, n, codes.data(), nullptr));
        return codes;
    }
    // any k: the library's one- or two-byte codes (vqhip.h "code width") widened to 32 bits
    std::vector<std::uint32_t> encode_wide(const float *rows, std::size_t n) const {
        std::vector<std::uint32_t> out(n * m_);
        if (!n) return out;
        if (vqhip_code_bytes((std::uint32_t)k_) == 1) {
            std::vector<std::uint8_t> c(n * m_);
            detail::check(vqhip_pq_encode(enc_.get(), rows, n, c.data(), nullptr));
            for (std::size_t i = 0; i < c.size(); ++i) out[i] = c[i];
        } else {
            std::vector<std::uint16_t> c(n * m_);
            detail::check(vqhip_pq_encode(enc_.get(), rows, n, reinterpret_cast<std::uint8_t *>(c.data()), nullptr));
            for (std::size_t i = 0; i < c.size(); ++i) out[i] = c[i];
        }
        return out;
    }

    // reconstruction from one-byte codes [n][m] -> [n][dim] f32 (un-rounded centroids), and the batch form of dequantize
    // (src/pq.rs:201-209): row blocks over the quantizer's devices when it was trained over several
    std::vector<float> decode(const std::uint8_t *codes, std::size_t n) const {
        if (k_ > 256) throw VqError::InvalidParameter("k", "one-byte codes need k <= 256");
        std::vector<float> out(n * dim_);
        if (!n) return out;
        detail::check(menc_ && n >= 65536 ? vqhip_mpq_decode(menc_.get(), codes, n, out.data())
                                          : vqhip_pq_decode(enc_.get(), codes, n, out.data()));
        return out;
    }
    std::vector<float> dequantize_batch(const f16 *quantized, std::size_t n) const {
        std::vector<float> out(n * dim_);
        if (!n) return out;
        const std::uint16_t *bits = reinterpret_cast<const std::uint16_t *>(quantized);
        detail::check(menc_ && n >= 65536 ? vqhip_mpq_dequantize_f16(menc_.get(), bits, n * dim_, out.data())
                                          : vqhip_dequantize_f16(bits, n * dim_, out.data()));
        return out;
    }

   private:
    // large batches of a quantizer trained over several devices: row blocks over the same devices
    int encode_raw(const float *rows, std::size_t n, std::uint8_t *codes, std::uint16_t *f16_out) const {
        if (menc_ && n >= 65536) return vqhip_mpq_encode(menc_.get(), rows, n, codes, f16_out);
        return vqhip_pq_encode(enc_.get(), rows, n, codes, f16_out);
    }
    void init(const float *rows, std::size_t n, std::size_t dim, std::size_t m, std::size_t k, std::size_t max_iters,
              Distance distance, std::uint64_t seed, const std::vector<int> &devices = {}) {
        if (m == 0) throw VqError::InvalidParameter("m", "must be greater than 0");
        if (dim < m) throw VqError::InvalidParameter("m", "must be at most the data dimension (" + std::to_string(dim) + ")");
        if (dim % m != 0)
            throw VqError::InvalidParameter("m", "dimension (" + std::to_string(dim) + ") must be divisible by m");
        detail::check_lbg_params(n, k);
        if (k > 65536) throw VqError::InvalidParameter("k", "codes are at most two bytes (k <= 65536)");
        m_ = m;
        k_ = k;
        dim_ = dim;
        sub_dim_ = dim / m;
        distance_ = distance;
        if (devices.size() > 1) {
            vqhip_mdataset *raw = nullptr;
            detail::check(vqhip_mdataset_from_host(rows, n, (std::uint32_t)dim, devices.data(), (int)devices.size(), &raw));
            std::unique_ptr<vqhip_mdataset, detail::MDatasetDel> ds(raw);
            codebooks_ = detail::fit_codebooks_multi(ds.get(), n, (std::uint32_t)dim, (std::uint32_t)m, (std::uint32_t)k, max_iters, seed);
            vqhip_mpq_encoder *me = nullptr;
            detail::check(vqhip_mpq_encoder_create(codebooks_.data(), (std::uint32_t)m, (std::uint32_t)k, (std::uint32_t)sub_dim_,
                                                   (int)distance.kind(), devices.data(), (int)devices.size(), &me));
            menc_.reset(me);
        } else {
            if (devices.size() == 1) detail::check(vqhip_set_device(devices[0]));
            vqhip_dataset *raw = nullptr;
            detail::check(vqhip_dataset_from_host(rows, n, (std::uint32_t)dim, &raw));
            std::unique_ptr<vqhip_dataset, detail::DatasetDel> ds(raw);
            codebooks_ = detail::fit_codebooks(ds.get(), n, (std::uint32_t)dim, (std::uint32_t)m, (std::uint32_t)k,
                                               max_iters, seed);
        }
        vqhip_pq_encoder *e = nullptr;
        detail::check(vqhip_pq_encoder_create(codebooks_.data(), (std::uint32_t)m, (std::uint32_t)k,
                                              (std::uint32_t)sub_dim_, (int)distance.kind(), &e));
        enc_.reset(e);
    }
    std::size_t m_ = 0, k_ = 0, dim_ = 0, sub_dim_ = 0;
    Distance distance_;
    std::vector<float> codebooks_;
    std::unique_ptr<vqhip_pq_encoder, detail::EncoderDel> enc_;
    std::unique_ptr<vqhip_mpq_encoder, detail::MEncoderDel> menc_;
};

// ------------------------------------------------------------------------------ TSVQ ----
class TSVQ {
   public:
    // TSVQ::new, src/tsvq.rs:195-223
    TSVQ(const std::vector<std::vector<float>> &training_data, std::size_t max_depth, Distance distance) {
        std::size_t dim = 0;
        const std::vector<float> flat = detail::flatten(training_data, &dim);
        init(flat.data(), training_data.size(), dim, max_depth, distance);
    }
    TSVQ(const float *rows, std::size_t n, std::size_t dim, std::size_t max_depth, Distance distance) {
        if (n == 0) throw VqError::EmptyInput();
        init(rows, n, dim, max_depth, distance);
    }
    // same, batch encodes in row blocks over `devices` (the build runs on devices[0]: SURVEY.md 8(e), "replicas only";
    // the tree is replicated, each device descends its own rows)
    TSVQ(const float *rows, std::size_t n, std::size_t dim, std::size_t max_depth, Distance distance, const std::vector<int> &devices) {
        if (n == 0) throw VqError::EmptyInput();
        if (!devices.empty()) detail::check(vqhip_set_device(devices[0]));
        init(rows, n, dim, max_depth, distance);
        if (devices.size() > 1) {
            vqhip_mtsvq *mt = nullptr;
            detail::check(vqhip_mtsvq_create(centroids_.data(), left_.data(), right_.data(), (std::uint32_t)left_.size(), (std::uint32_t)dim,
                                             (int)distance.kind(), devices.data(), (int)devices.size(), &mt));
            menc_.reset(mt);
        }
    }
    std::size_t dim() const { return dim_; }
    const char *distance_metric() const { return distance_.name(); }
    std::size_t num_nodes() const { return left_.size(); }
    const std::vector<float> &centroids() const { return centroids_; }  // [nodes][dim], pre-order
    const std::vector<std::int32_t> &left() const { return left_; }
    const std::vector<std::int32_t> &right() const { return right_; }

    // Quantizer::quantize, src/tsvq.rs:239-255
    std::vector<f16> quantize(const float *vector, std::size_t len) const {
        if (len != dim_) throw VqError::DimensionMismatch(dim_, len);
        std::vector<f16> out(dim_);
        detail::check(vqhip_tsvq_encode(enc_.get(), vector, 1, nullptr, reinterpret_cast<std::uint16_t *>(out.data())));
        return out;
    }
    std::vector<f16> quantize(const std::vector<float> &vector) const { return quantize(vector.data(), vector.size()); }
    // src/tsvq.rs:257-265
    std::vector<float> dequantize(const std::vector<f16> &quantized) const {
        if (quantized.size() != dim_) throw VqError::DimensionMismatch(dim_, quantized.size());
        std::vector<float> out(dim_);
        for (std::size_t i = 0; i < dim_; ++i) out[i] = quantized[i].to_f32();
        return out;
    }
    std::vector<std::int32_t> leaf_ids(const float *rows, std::size_t n) const {
        std::vector<std::int32_t> leaf(n);
        if (n) detail::check(encode_raw(rows, n, leaf.data(), nullptr));
        return leaf;
    }
    // batch forms: rows [n][dim] -> the leaf centroids as f16 (row i == quantize(rows[i])), and f16 -> f32
    std::vector<f16> quantize_batch(const float *rows, std::size_t n) const {
        std::vector<f16> out(n * dim_);
        if (n) detail::check(encode_raw(rows, n, nullptr, reinterpret_cast<std::uint16_t *>(out.data())));
        return out;
    }
    std::vector<float> dequantize_batch(const f16 *quantized, std::size_t n) const {
        std::vector<float> out(n * dim_);
        if (!n) return out;
        const std::uint16_t *bits = reinterpret_cast<const std::uint16_t *>(quantized);
        detail::check(menc_ && n >= 65536 ? vqhip_mtsvq_dequantize_f16(menc_.get(), bits, n * dim_, out.data())
                                          : vqhip_dequantize_f16(bits, n * dim_, out.data()));
        return out;
    }

   private:
    int encode_raw(const float *rows, std::size_t n, std::int32_t *leaf, std::uint16_t *f16_out) const {
        if (menc_ && n >= 65536) return vqhip_mtsvq_encode(menc_.get(), rows, n, leaf, f16_out);
        return vqhip_tsvq_encode(enc_.get(), rows, n, leaf, f16_out);
    }
    void init(const float *rows, std::size_t n, std::size_t dim, std::size_t max_depth, Distance distance) {
        dim_ = dim;
        distance_ = distance;
        vqhip_dataset *raw = nullptr;
        detail::check(vqhip_dataset_from_host(rows, n, (std::uint32_t)dim, &raw));
        std::unique_ptr<vqhip_dataset, detail::DatasetDel> ds(raw);
        const std::uint64_t by_rows = 2 * (std::uint64_t)n - 1;
        std::uint64_t cap = by_rows;
        if (max_depth < 40 && ((1ull << (max_depth + 1)) - 1) < cap) cap = (1ull << (max_depth + 1)) - 1;
        centroids_.assign((std::size_t)cap * dim, 0.0f);
        left_.assign(cap, -1);
        right_.assign(cap, -1);
        std::int32_t nodes = 0;
        detail::check(vqhip_tsvq_build(ds.get(), (std::uint32_t)max_depth, (std::uint32_t)cap, centroids_.data(),
                                       left_.data(), right_.data(), &nodes));
        centroids_.resize((std::size_t)nodes * dim);
        left_.resize(nodes);
        right_.resize(nodes);
        vqhip_tsvq *t = nullptr;
        detail::check(vqhip_tsvq_create(centroids_.data(), left_.data(), right_.data(), (std::uint32_t)nodes,
                                        (std::uint32_t)dim, (int)distance.kind(), &t));
        enc_.reset(t);
    }
    std::size_t dim_ = 0;
    Distance distance_;
    std::vector<float> centroids_;
    std::vector<std::int32_t> left_, right_;
    std::unique_ptr<vqhip_tsvq, detail::TsvqDel> enc_;
    std::unique_ptr<vqhip_mtsvq, detail::MTsvqDel> menc_;
};

// ----------------------------------------------------------- ScalarQuantizer / BinaryQuantizer ----
namespace detail {
// a *_check status -> VqError::InvalidParameter from the library's `Display` text ("Invalid parameter 'p': reason")
inline void check_param(int status) {
    if (status == VQHIP_OK) return;
    const std::string msg = vqhip_last_error(), head = "Invalid parameter '";
    const std::size_t q = msg.find("': ", head.size());
    if (status == VQHIP_ERR_INVALID_INPUT && msg.compare(0, head.size(), head) == 0 && q != std::string::npos)
        throw VqError::InvalidParameter(msg.substr(head.size(), q - head.size()), msg.substr(q + 3));
    throw VqError::FfiError(msg);
}
}  // namespace detail

// src/sq.rs: [min, max] into `levels` codes; bit-identical codes and values, on the device (vqhip_sq_*)
class ScalarQuantizer {
   public:
    ScalarQuantizer(float min, float max, std::size_t levels) : min_(min), max_(max), levels_(levels) {
        // levels beyond u32 fail the same "no more than 256" check as any value above 256
        detail::check_param(vqhip_sq_check(min, max, levels > 0xFFFFFFFFu ? 0xFFFFFFFFu : (std::uint32_t)levels, &step_));
    }
    float min() const { return min_; }
    float max() const { return max_; }
    std::size_t levels() const { return levels_; }
    float step() const { return step_; }

    std::vector<std::uint8_t> quantize(const float *x, std::size_t count) const {
        std::vector<std::uint8_t> out(count);
        detail::check(vqhip_sq_encode(min_, max_, (std::uint32_t)levels_, x, count, out.data()));
        return out;
    }
    std::vector<std::uint8_t> quantize(const std::vector<float> &vector) const { return quantize(vector.data(), vector.size()); }
    std::vector<float> dequantize(const std::vector<std::uint8_t> &codes) const {
        std::vector<float> out(codes.size());
        detail::check(vqhip_sq_decode(min_, max_, (std::uint32_t)levels_, codes.data(), codes.size(), out.data()));
        return out;
    }

   private:
    float min_, max_;
    std::size_t levels_;
    float step_ = 0;
};

// src/bq.rs: x >= threshold -> high, else low; a code >= high decodes to high, any other to low (vqhip_bq_*)
class BinaryQuantizer {
   public:
    BinaryQuantizer(float threshold, std::uint8_t low, std::uint8_t high) : threshold_(threshold), low_(low), high_(high) {
        detail::check_param(vqhip_bq_check(threshold, low, high));
    }
    float threshold() const { return threshold_; }
    std::uint8_t low() const { return low_; }
    std::uint8_t high() const { return high_; }

    std::vector<std::uint8_t> quantize(const float *x, std::size_t count) const {
        std::vector<std::uint8_t> out(count);
        detail::check(vqhip_bq_encode(threshold_, low_, high_, x, count, out.data()));
        return out;
    }
    std::vector<std::uint8_t> quantize(const std::vector<float> &vector) const { return quantize(vector.data(), vector.size()); }
    std::vector<float> dequantize(const std::vector<std::uint8_t> &codes) const {
        std::vector<float> out(codes.size());
        detail::check(vqhip_bq_decode(threshold_, low_, high_, codes.data(), codes.size(), out.data()));
        return out;
    }

   private:
    float threshold_;
    std::uint8_t low_, high_;
};

// ---------------------------------------------------------------------- lbg_quantize ----
// src/core/vector.rs:390-461: k centroids of `data` (n vectors of equal length)
inline std::vector<std::vector<float>> lbg_quantize(const std::vector<std::vector<float>> &data, std::size_t k,
                                                    std::size_t max_iters, std::uint64_t seed) {
    if (data.empty()) throw VqError::EmptyInput();  // vector.rs:396-398
    if (k == 0) throw VqError::InvalidParameter("k", "must be greater than 0");
    if (data.size() < k)
        throw VqError::InvalidParameter("k", "not enough data points (" + std::to_string(data.size()) + ") for " +
                                                 std::to_string(k) + " clusters");
    if (k > 65536) throw VqError::InvalidParameter("k", "codes are at most two bytes (k <= 65536)");
    std::size_t dim = 0;
    const std::vector<float> flat = detail::flatten(data, &dim);
    vqhip_dataset *raw = nullptr;
    detail::check(vqhip_dataset_from_host(flat.data(), data.size(), (std::uint32_t)dim, &raw));
    std::unique_ptr<vqhip_dataset, detail::DatasetDel> ds(raw);
    const std::vector<float> cb =
        detail::fit_codebooks(ds.get(), data.size(), (std::uint32_t)dim, 1, (std::uint32_t)k, max_iters, seed);
    std::vector<std::vector<float>> out(k, std::vector<float>(dim));
    for (std::size_t j = 0; j < k; ++j) std::memcpy(out[j].data(), cb.data() + j * dim, dim * sizeof(float));
    return out;
}

// The result of a range search (include/vqhip.h, vqhip_*_range_search), CSR: the hits of query q are idx / dist
// [lims[q], lims[q + 1]) -- the rows with D(q, row) <= radius[q] (the binary indexes: H(q, row) <= radius[q] bits), in
// ascending row id -- and lims[0] = 0.
struct RangeResult {
    std::vector<std::uint64_t> lims;  // [nq + 1]
    std::vector<std::uint32_t> idx;   // [total]
    std::vector<float> dist;          // [total]
};

// The row mask of a filtered call (include/vqhip.h): ceil(n / 32) words, row i allowed iff bit i & 31 of word i >> 5 is set.
inline std::vector<std::uint32_t> pack_row_mask(const std::vector<bool> &allowed) {
    std::vector<std::uint32_t> w((allowed.size() + 31) / 32, 0u);
    for (std::size_t i = 0; i < allowed.size(); ++i)
        if (allowed[i]) w[i >> 5] |= 1u << (i & 31);
    return w;
}

// Removing rows (include/vqhip.h, "adding and removing rows"): the mask of a removal from row ids in [0, n), in any order,
// repeats welcome -- true: the row is removed.
inline std::vector<bool> remove_mask(const std::vector<std::uint32_t> &ids, std::size_t n) {
    std::vector<bool> m(n, false);
    for (std::uint32_t i : ids) {
        if (i >= n) throw VqError::InvalidParameter("ids", "row id " + std::to_string(i) + " is outside [0, n)");
        m[i] = true;
    }
    return m;
}

namespace detail {
// the argument checks of an add and of a removal, before the library is called: the rows in all stay below 2^32; the
// mask has n entries and leaves a row -- returns the old ids of the rows it leaves, in their new order
inline void check_room(std::size_t n, std::size_t b) {
    if (b >= (std::size_t(1) << 32) || n + b >= (std::size_t(1) << 32))
        throw VqError::InvalidParameter("rows", "at most 2^32 - 1 rows in all");
}
inline std::vector<std::uint32_t> kept_rows(const std::vector<bool> &remove, std::size_t n) {
    if (remove.size() != n) throw VqError::DimensionMismatch(n, remove.size());
    std::vector<std::uint32_t> kept;
    for (std::size_t i = 0; i < n; ++i)
        if (!remove[i]) kept.push_back((std::uint32_t)i);
    if (kept.empty()) throw VqError::InvalidParameter("remove", "would leave no row; an index holds at least one");
    return kept;
}
// the argument checks of a filtered call, before the library is called: the mask's pointer; its length as a vector
inline void check_row_mask(const std::uint32_t *allowed) {
    if (!allowed) throw VqError::InvalidParameter("allowed", "the row mask is null");
}
inline void check_row_mask(const std::vector<std::uint32_t> &allowed, std::size_t n) {
    if (allowed.size() != (n + 31) / 32) throw VqError::DimensionMismatch((n + 31) / 32, allowed.size());
}
struct RangeDel {
    void operator()(vqhip_range *p) const { (void)vqhip_range_destroy(p); }
};
// the argument checks of a range search, before the library is called
inline void check_range_args(const float *radii, std::size_t nq, std::uint64_t max_results) {
    if (nq >= (std::size_t(1) << 32)) throw VqError::InvalidParameter("queries", "at most 2^32 - 1 per call");
    if (max_results == 0) throw VqError::InvalidParameter("max_results", "must be at least 1");
    for (std::size_t q = 0; q < nq; ++q)
        if (radii[q] != radii[q]) throw VqError::InvalidParameter("radius", "is NaN for query " + std::to_string(q));
}
// a finished device result to host vectors
inline RangeResult read_range(vqhip_range *raw) {
    std::unique_ptr<vqhip_range, RangeDel> r(raw);
    std::uint32_t nq = 0;
    std::uint64_t total = 0;
    check(vqhip_range_info(r.get(), &nq, &total));
    RangeResult out{std::vector<std::uint64_t>((std::size_t)nq + 1), std::vector<std::uint32_t>(total), std::vector<float>(total)};
    check(vqhip_range_read(r.get(), out.lims.data(), out.idx.data(), out.dist.data()));
    return out;
}
}  // namespace detail

namespace detail {
// What the resident indexes share over their C handles (H and its destroy / search): the shape, the handle, and a search,
// whose arguments are the same for every kind of row.  The arguments are checked before the device is touched.
template <class H, int (*Destroy)(H *), int (*Search)(H *, const float *, std::uint32_t, std::uint32_t, std::uint32_t *, float *),
          int (*Remove)(H *, const std::uint32_t *, std::uint64_t *), int (*RemoveDevice)(H *, const std::uint32_t *, std::uint64_t *)>
class ResidentIndex {
   public:
    std::size_t size() const { return n_; }
    std::size_t dim() const { return dim_; }
    const char *distance_metric() const { return distance_.name(); }

    struct Result {
        std::vector<std::uint32_t> idx;  // [nq][topk]
        std::vector<float> dist;         // [nq][topk]
    };
    // queries [nq][dim] f32
    Result search(const float *queries, std::size_t nq, std::size_t topk) const {
        if (topk == 0 || topk > 1024 || topk > n_)
            throw VqError::InvalidParameter("topk", "must be between 1 and min(n, 1024)");
        if (nq >= (std::size_t(1) << 32)) throw VqError::InvalidParameter("queries", "at most 2^32 - 1 per call");
        Result r{std::vector<std::uint32_t>(nq * topk), std::vector<float>(nq * topk)};
        if (nq) check(Search(ix_.get(), queries, (std::uint32_t)nq, (std::uint32_t)topk, r.idx.data(), r.dist.data()));
        return r;
    }
    Result search(const std::vector<float> &queries, std::size_t topk) const {
        if (queries.size() % dim_) throw VqError::DimensionMismatch(dim_, queries.size() % dim_);
        return search(queries.data(), queries.size() / dim_, topk);
    }

    // Adding and removing rows (include/vqhip.h, "adding and removing rows"): after any sequence of them every call
    // returns bit for bit what a fresh index over the remaining rows returns.  The arguments are checked before the device
    // is touched; adding no rows and removing none do not touch it.  Each class has its own add forms.
    // remove_rows: `remove` [n], true: the row goes (or row ids, through remove_mask).  The other rows keep their order and
    // move up; returns the old ids of the remaining rows in their new order.  Removing every row is refused.
    std::vector<std::uint32_t> remove_rows(const std::vector<bool> &remove) {
        std::vector<std::uint32_t> kept = kept_rows(remove, n_);
        if (kept.size() == n_) return kept;
        const std::vector<std::uint32_t> words = pack_row_mask(remove);
        std::uint64_t gone = 0;
        check(Remove(ix_.get(), words.data(), &gone));
        n_ = kept.size();
        return kept;
    }
    std::vector<std::uint32_t> remove_rows(const std::vector<std::uint32_t> &ids) { return remove_rows(remove_mask(ids, n_)); }
    // the mask's ceil(n / 32) words at a device pointer (4-byte aligned; bit set: remove); returns the rows removed
    std::size_t remove_rows_device(const std::uint32_t *dev_remove_words) {
        if (!dev_remove_words) throw VqError::InvalidParameter("remove", "the mask is null");
        std::uint64_t gone = 0;
        check(RemoveDevice(ix_.get(), dev_remove_words, &gone));
        n_ -= (std::size_t)gone;
        return (std::size_t)gone;
    }

   protected:
    ResidentIndex() = default;
    // b rows through call(handle): their ids n .. n + b - 1
    template <class F>
    std::vector<std::uint32_t> append(const void *src, std::size_t b, F &&call) {
        check_room(n_, b);
        std::vector<std::uint32_t> ids(b);
        if (b == 0) return ids;
        if (!src) throw VqError::InvalidParameter("rows", "the source is null");
        check(call(ix_.get()));
        for (std::size_t i = 0; i < b; ++i) ids[i] = (std::uint32_t)(n_ + i);
        n_ += b;
        return ids;
    }
    // the shape checks of an index of any dimension (BinaryIndex has a bound on it, and its own)
    static void check_shape(std::size_t n, std::size_t dim) {
        if (n == 0) throw VqError::EmptyInput();
        if (dim == 0) throw VqError::InvalidParameter("dim", "must be at least 1");
        if (n >= (std::size_t(1) << 32) || dim > 0xFFFFFFFFu) throw VqError::InvalidParameter("rows", "at most 2^32 - 1 rows of 2^32 - 1 dimensions");
    }
    // a created handle and its shape
    void adopt(H *h, std::size_t n, std::size_t dim, Distance distance) {
        ix_.reset(h);
        n_ = n;
        dim_ = dim;
        distance_ = distance;
    }
    struct Del {
        void operator()(H *p) const { (void)Destroy(p); }
    };
    std::unique_ptr<H, Del> ix_;
    std::size_t n_ = 0, dim_ = 0;
    Distance distance_;
};

// The two indexes of exact distances (FlatIndex, ScalarIndex) also answer range queries and rerank a caller's candidates.
template <class H, int (*Destroy)(H *), int (*Search)(H *, const float *, std::uint32_t, std::uint32_t, std::uint32_t *, float *),
          int (*Range)(H *, const float *, std::uint32_t, const float *, std::uint64_t, vqhip_range **),
          int (*Rerank)(H *, const float *, std::uint32_t, const std::uint32_t *, std::uint32_t, std::uint32_t, std::uint32_t *, float *),
          int (*SearchMasked)(H *, const float *, std::uint32_t, std::uint32_t, const std::uint32_t *, std::uint32_t *, float *),
          int (*RangeMasked)(H *, const float *, std::uint32_t, const float *, std::uint64_t, const std::uint32_t *, vqhip_range **),
          int (*Remove)(H *, const std::uint32_t *, std::uint64_t *), int (*RemoveDevice)(H *, const std::uint32_t *, std::uint64_t *)>
class ExactResidentIndex : public ResidentIndex<H, Destroy, Search, Remove, RemoveDevice> {
    using Base = ResidentIndex<H, Destroy, Search, Remove, RemoveDevice>;

   public:
    using Result = typename Base::Result;
    using Base::search;
    // The filtered forms: `allowed` is the row mask of the call, ceil(n / 32) words (pack_row_mask).  search: the nearest
    // among the allowed rows; a query with fewer than topk of them has idx 0xFFFFFFFF / dist +inf behind them.
    Result search(const float *queries, std::size_t nq, std::size_t topk, const std::uint32_t *allowed) const {
        check_row_mask(allowed);
        if (topk == 0 || topk > 1024 || topk > this->n_)
            throw VqError::InvalidParameter("topk", "must be between 1 and min(n, 1024)");
        if (nq >= (std::size_t(1) << 32)) throw VqError::InvalidParameter("queries", "at most 2^32 - 1 per call");
        Result r{std::vector<std::uint32_t>(nq * topk), std::vector<float>(nq * topk)};
        if (nq)
            check(SearchMasked(this->ix_.get(), queries, (std::uint32_t)nq, (std::uint32_t)topk, allowed, r.idx.data(), r.dist.data()));
        return r;
    }
    Result search(const std::vector<float> &queries, std::size_t topk, const std::vector<std::uint32_t> &allowed) const {
        check_row_mask(allowed, this->n_);
        if (queries.size() % this->dim_) throw VqError::DimensionMismatch(this->dim_, queries.size() % this->dim_);
        return search(queries.data(), queries.size() / this->dim_, topk, allowed.data());
    }
    // range_search over the allowed rows only (the mask comes last: max_results has no default here, so that a literal 0
    // in its place never reads as a null mask)
    RangeResult range_search(const float *queries, std::size_t nq, const float *radii, std::uint64_t max_results,
                             const std::uint32_t *allowed) const {
        check_row_mask(allowed);
        check_range_args(radii, nq, max_results);
        if (nq == 0) return RangeResult{std::vector<std::uint64_t>(1, 0), {}, {}};
        vqhip_range *r = nullptr;
        check(RangeMasked(this->ix_.get(), queries, (std::uint32_t)nq, radii, max_results, allowed, &r));
        return read_range(r);
    }
    RangeResult range_search(const std::vector<float> &queries, const std::vector<float> &radii, std::uint64_t max_results,
                             const std::vector<std::uint32_t> &allowed) const {
        const std::size_t dim = this->dim_;
        check_row_mask(allowed, this->n_);
        if (queries.size() % dim) throw VqError::DimensionMismatch(dim, queries.size() % dim);
        if (radii.size() != queries.size() / dim) throw VqError::DimensionMismatch(queries.size() / dim, radii.size());
        return range_search(queries.data(), queries.size() / dim, radii.data(), max_results, allowed.data());
    }
    // every row within radii[q] of query q (radii [nq], none NaN), at most max_results hits in all (more: FfiError)
    RangeResult range_search(const float *queries, std::size_t nq, const float *radii, std::uint64_t max_results = std::uint64_t(1) << 28) const {
        check_range_args(radii, nq, max_results);
        if (nq == 0) return RangeResult{std::vector<std::uint64_t>(1, 0), {}, {}};
        vqhip_range *r = nullptr;
        check(Range(this->ix_.get(), queries, (std::uint32_t)nq, radii, max_results, &r));
        return read_range(r);
    }
    RangeResult range_search(const std::vector<float> &queries, const std::vector<float> &radii,
                             std::uint64_t max_results = std::uint64_t(1) << 28) const {
        const std::size_t dim = this->dim_;
        if (queries.size() % dim) throw VqError::DimensionMismatch(dim, queries.size() % dim);
        if (radii.size() != queries.size() / dim) throw VqError::DimensionMismatch(queries.size() / dim, radii.size());
        return range_search(queries.data(), queries.size() / dim, radii.data(), max_results);
    }
    // per query the topk nearest of its c candidate row ids cand [nq][c] (distinct within a query, each < n)
    Result rerank(const float *queries, std::size_t nq, const std::uint32_t *cand, std::size_t c, std::size_t topk) const {
        if (c == 0 || c > 4096) throw VqError::InvalidParameter("candidates", "between 1 and 4096 per query");
        if (topk == 0 || topk > c) throw VqError::InvalidParameter("topk", "must be between 1 and the number of candidates");
        if (nq >= (std::size_t(1) << 32)) throw VqError::InvalidParameter("queries", "at most 2^32 - 1 per call");
        for (std::size_t e = 0; e < nq * c; ++e)
            if (cand[e] >= this->n_) throw VqError::InvalidParameter("candidates", "a row id is outside [0, n)");
        Result r{std::vector<std::uint32_t>(nq * topk), std::vector<float>(nq * topk)};
        if (nq)
            check(Rerank(this->ix_.get(), queries, (std::uint32_t)nq, cand, (std::uint32_t)c, (std::uint32_t)topk, r.idx.data(),
                         r.dist.data()));
        return r;
    }
};
}  // namespace detail

// Exact k-NN search over rows kept on the device (include/vqhip.h, vqhip_flat_*): rows [n][dim] f32 or f16, uploaded once
// by the constructor; search / rerank give (row index, distance) pairs [nq][topk], nearest first, NaN last, ties to the
// lower row.  The arguments are checked before the device is touched.
class FlatIndex : public detail::ExactResidentIndex<vqhip_flat, vqhip_flat_destroy, vqhip_flat_search, vqhip_flat_range_search, vqhip_flat_rerank,
                                                    vqhip_flat_search_masked, vqhip_flat_range_search_masked, vqhip_flat_remove,
                                                    vqhip_flat_remove_device> {
   public:
    FlatIndex(const float *rows, std::size_t n, std::size_t dim, Distance distance = Distance()) {
        init(rows, 0, n, dim, distance);
    }
    FlatIndex(const f16 *rows, std::size_t n, std::size_t dim, Distance distance = Distance()) {
        init(rows, 1, n, dim, distance);
    }
    bool half() const { return dtype_ == 1; }
    // append b rows [b][dim] in the index's own element type (the other one is refused); returns their ids n .. n + b - 1
    std::vector<std::uint32_t> add(const float *rows, std::size_t b) { return add_as(rows, 0, b); }
    std::vector<std::uint32_t> add(const f16 *rows, std::size_t b) { return add_as(rows, 1, b); }
    // the same from a device pointer to rows of the index's element type
    std::vector<std::uint32_t> add_device(const void *dev_rows, std::size_t b) {
        return append(dev_rows, b, [&](vqhip_flat *f) { return vqhip_flat_add_device(f, dev_rows, b); });
    }

   private:
    std::vector<std::uint32_t> add_as(const void *rows, int dtype, std::size_t b) {
        if (dtype != dtype_) throw VqError::InvalidParameter("rows", dtype_ ? "the index holds f16 rows" : "the index holds f32 rows");
        return append(rows, b, [&](vqhip_flat *f) { return vqhip_flat_add(f, rows, b); });
    }
    int dtype_ = 0;
    void init(const void *rows, int dtype, std::size_t n, std::size_t dim, Distance distance) {
        check_shape(n, dim);
        dtype_ = dtype;
        vqhip_flat *f = nullptr;
        detail::check(vqhip_flat_create(rows, n, (std::uint32_t)dim, dtype, (int)distance.kind(), &f));
        adopt(f, n, dim, distance);
    }
};

namespace detail {
// packed rows [n][ceil(dim / 32)] of the two binary indexes: no bit at or past dim may be set
inline void check_pad_bits(const std::uint32_t *words, std::size_t n, std::size_t dim) {
    if (dim % 32 == 0) return;
    const std::size_t w = (dim + 31) / 32;
    const std::uint32_t mask = (1u << (dim % 32)) - 1u;
    for (std::size_t i = 0; i < n; ++i)
        if (words[i * w + w - 1] & ~mask) throw VqError::InvalidParameter("words", "a row has a pad bit set");
}
}  // namespace detail

// Hamming index over packed BQ codes (include/vqhip.h, vqhip_binary_*): rows binarised by a BinaryQuantizer (f32 rows,
// u8 codes or packed words [n][ceil(dim / 32)]), searched under squared Euclidean, Euclidean or Manhattan on the
// dequantized vectors; (row id, distance) pairs [nq][topk], nearest first, ties to the lower row.  The queries are
// binarised by the index's quantizer on the device.  Cosine and every other bad argument are refused before the device
// is touched.
class BinaryIndex : public detail::ResidentIndex<vqhip_binary, vqhip_binary_destroy, vqhip_binary_search, vqhip_binary_remove,
                                                 vqhip_binary_remove_device> {
   public:
    enum class Source { Rows = VQHIP_BINARY_F32, Codes = VQHIP_BINARY_U8, Packed = VQHIP_BINARY_PACKED };
    BinaryIndex(const float *rows, std::size_t n, std::size_t dim, BinaryQuantizer quantizer = BinaryQuantizer(0.0f, 0, 1),
                Distance distance = Distance(Distance::Manhattan))
        : quantizer_(quantizer) {
        init(rows, Source::Rows, n, dim, distance);
    }
    BinaryIndex(const std::uint8_t *codes, std::size_t n, std::size_t dim, BinaryQuantizer quantizer,
                Distance distance = Distance(Distance::Manhattan))
        : quantizer_(quantizer) {
        init(codes, Source::Codes, n, dim, distance);
    }
    BinaryIndex(const std::uint32_t *words, std::size_t n, std::size_t dim, BinaryQuantizer quantizer,
                Distance distance = Distance(Distance::Manhattan))
        : quantizer_(quantizer) {
        init(words, Source::Packed, n, dim, distance);
    }
    std::size_t words_per_row() const { return (dim_ + 31) / 32; }
    const BinaryQuantizer &quantizer() const { return quantizer_; }
    // every row within radii[q] bits of query q: H(q, row) <= radii[q], H the Hamming distance search selects on (radii
    // [nq], any value: >= dim returns every row, 0 the exact bit matches); CSR and in ascending row id, dist the distance
    // search reports for the row.  At most max_results hits in all (more: FfiError).
    RangeResult hamming_range_search(const float *queries, std::size_t nq, const std::uint32_t *radii,
                                     std::uint64_t max_results = std::uint64_t(1) << 28) const {
        if (nq >= (std::size_t(1) << 32)) throw VqError::InvalidParameter("queries", "at most 2^32 - 1 per call");
        if (max_results == 0) throw VqError::InvalidParameter("max_results", "must be at least 1");
        if (nq == 0) return RangeResult{std::vector<std::uint64_t>(1, 0), {}, {}};
        vqhip_range *r = nullptr;
        detail::check(vqhip_binary_range_search(ix_.get(), queries, (std::uint32_t)nq, radii, max_results, &r));
        return detail::read_range(r);
    }
    RangeResult hamming_range_search(const std::vector<float> &queries, const std::vector<std::uint32_t> &radii,
                                     std::uint64_t max_results = std::uint64_t(1) << 28) const {
        if (queries.size() % dim_) throw VqError::DimensionMismatch(dim_, queries.size() % dim_);
        if (radii.size() != queries.size() / dim_) throw VqError::DimensionMismatch(queries.size() / dim_, radii.size());
        return hamming_range_search(queries.data(), queries.size() / dim_, radii.data(), max_results);
    }
    // The filtered forms (include/vqhip.h, vqhip_binary_search_masked / _range_search_masked): `allowed` is the row mask of
    // the call, ceil(n / 32) words (pack_row_mask).  search: the nearest among the allowed rows by (H, row id); a query with
    // fewer than topk of them has idx 0xFFFFFFFF / dist +inf behind them.  hamming_range_search: only allowed rows hit.  The
    // mask comes last, and max_results has no default beside it, so that a literal 0 never reads as a null mask.
    using ResidentIndex::search;
    Result search(const float *queries, std::size_t nq, std::size_t topk, const std::uint32_t *allowed) const {
        detail::check_row_mask(allowed);
        if (topk == 0 || topk > 1024 || topk > n_) throw VqError::InvalidParameter("topk", "must be between 1 and min(n, 1024)");
        if (nq >= (std::size_t(1) << 32)) throw VqError::InvalidParameter("queries", "at most 2^32 - 1 per call");
        Result r{std::vector<std::uint32_t>(nq * topk), std::vector<float>(nq * topk)};
        if (nq)
            detail::check(vqhip_binary_search_masked(ix_.get(), queries, (std::uint32_t)nq, (std::uint32_t)topk, allowed, r.idx.data(),
                                                     r.dist.data()));
        return r;
    }
    Result search(const std::vector<float> &queries, std::size_t topk, const std::vector<std::uint32_t> &allowed) const {
        detail::check_row_mask(allowed, n_);
        if (queries.size() % dim_) throw VqError::DimensionMismatch(dim_, queries.size() % dim_);
        return search(queries.data(), queries.size() / dim_, topk, allowed.data());
    }
    RangeResult hamming_range_search(const float *queries, std::size_t nq, const std::uint32_t *radii, std::uint64_t max_results,
                                     const std::uint32_t *allowed) const {
        detail::check_row_mask(allowed);
        if (nq >= (std::size_t(1) << 32)) throw VqError::InvalidParameter("queries", "at most 2^32 - 1 per call");
        if (max_results == 0) throw VqError::InvalidParameter("max_results", "must be at least 1");
        if (nq == 0) return RangeResult{std::vector<std::uint64_t>(1, 0), {}, {}};
        vqhip_range *r = nullptr;
        detail::check(vqhip_binary_range_search_masked(ix_.get(), queries, (std::uint32_t)nq, radii, max_results, allowed, &r));
        return detail::read_range(r);
    }
    RangeResult hamming_range_search(const std::vector<float> &queries, const std::vector<std::uint32_t> &radii,
                                     std::uint64_t max_results, const std::vector<std::uint32_t> &allowed) const {
        detail::check_row_mask(allowed, n_);
        if (queries.size() % dim_) throw VqError::DimensionMismatch(dim_, queries.size() % dim_);
        if (radii.size() != queries.size() / dim_) throw VqError::DimensionMismatch(queries.size() / dim_, radii.size());
        return hamming_range_search(queries.data(), queries.size() / dim_, radii.data(), max_results, allowed.data());
    }
    // the packed rows [n][words_per_row()]
    std::vector<std::uint32_t> packed() const {
        std::vector<std::uint32_t> out(n_ * words_per_row());
        detail::check(vqhip_binary_packed(ix_.get(), out.data()));
        return out;
    }
    // append b rows in one of the constructors' three forms -- f32 rows [b][dim], u8 codes [b][dim], packed words
    // [b][words_per_row()] with the pad bits zero -- from host memory, or from a device pointer (f32 rows and words 4-byte
    // aligned; a pad bit set there is an FfiError that leaves the index as it was); returns their ids n .. n + b - 1
    std::vector<std::uint32_t> add(const float *rows, std::size_t b) { return add_from(rows, Source::Rows, b, false); }
    std::vector<std::uint32_t> add_codes(const std::uint8_t *codes, std::size_t b) { return add_from(codes, Source::Codes, b, false); }
    std::vector<std::uint32_t> add_packed(const std::uint32_t *words, std::size_t b) {
        if (words) check_pad(words, b, dim_);
        return add_from(words, Source::Packed, b, false);
    }
    std::vector<std::uint32_t> add_device(const void *dev_src, Source kind, std::size_t b) { return add_from(dev_src, kind, b, true); }

   private:
    static void check_pad(const std::uint32_t *words, std::size_t n, std::size_t dim) { detail::check_pad_bits(words, n, dim); }
    std::vector<std::uint32_t> add_from(const void *src, Source kind, std::size_t b, bool device) {
        return append(src, b, [&](vqhip_binary *h) {
            return device ? vqhip_binary_add_device(h, src, (int)kind, b) : vqhip_binary_add(h, src, (int)kind, b);
        });
    }
    void init(const void *src, Source kind, std::size_t n, std::size_t dim, Distance distance) {
        if (n == 0) throw VqError::EmptyInput();
        if (dim == 0 || dim > VQHIP_BINARY_MAX_DIM) throw VqError::InvalidParameter("dim", "must be between 1 and 8192");
        if (n >= (std::size_t(1) << 32)) throw VqError::InvalidParameter("rows", "at most 2^32 - 1 rows");
        if (distance.kind() != Distance::SquaredEuclidean && distance.kind() != Distance::Euclidean &&
            distance.kind() != Distance::Manhattan)
            throw VqError::InvalidParameter("distance", "must be squared_euclidean, euclidean or manhattan");
        if (kind == Source::Packed) check_pad(static_cast<const std::uint32_t *>(src), n, dim);
        vqhip_binary *b = nullptr;
        detail::check(vqhip_binary_create(src, (int)kind, n, (std::uint32_t)dim, quantizer_.threshold(), quantizer_.low(),
                                          quantizer_.high(), (int)distance.kind(), &b));
        adopt(b, n, dim, distance);
    }
    BinaryQuantizer quantizer_;
};

// Exact index over SQ codes kept on the device, one byte per dimension (include/vqhip.h, vqhip_sqindex_*): built from f32
// rows (encoded on the device; only the codes stay) or from u8 codes, searched with f32 queries (never quantized) under
// any metric.  Every result equals FlatIndex over quantizer.dequantize(codes): (row index, distance) pairs [nq][topk],
// nearest first, NaN last, ties to the lower row.  The arguments are checked before the device is touched.
class ScalarIndex
    : public detail::ExactResidentIndex<vqhip_sqindex, vqhip_sqindex_destroy, vqhip_sqindex_search, vqhip_sqindex_range_search, vqhip_sqindex_rerank,
                                        vqhip_sqindex_search_masked, vqhip_sqindex_range_search_masked, vqhip_sqindex_remove,
                                        vqhip_sqindex_remove_device> {
   public:
    ScalarIndex(const float *rows, std::size_t n, std::size_t dim, ScalarQuantizer quantizer, Distance distance = Distance())
        : quantizer_(quantizer) {
        init(rows, true, n, dim, distance);
    }
    ScalarIndex(const std::uint8_t *codes, std::size_t n, std::size_t dim, ScalarQuantizer quantizer, Distance distance = Distance())
        : quantizer_(quantizer) {
        init(codes, false, n, dim, distance);
    }
    const ScalarQuantizer &quantizer() const { return quantizer_; }
    // the codes [n][dim]
    std::vector<std::uint8_t> codes() const {
        std::vector<std::uint8_t> out(n_ * dim_);
        detail::check(vqhip_sqindex_codes(ix_.get(), out.data()));
        return out;
    }
    // append b rows: f32 rows [b][dim], encoded on the device as the constructor encodes them, or u8 codes [b][dim] as they
    // are; from host memory or a device pointer (f32 rows 4-byte aligned).  Returns their ids n .. n + b - 1.
    std::vector<std::uint32_t> add(const float *rows, std::size_t b) {
        return append(rows, b, [&](vqhip_sqindex *x) { return vqhip_sqindex_add_rows(x, rows, b); });
    }
    std::vector<std::uint32_t> add_device(const void *dev_rows, std::size_t b) {
        return append(dev_rows, b, [&](vqhip_sqindex *x) { return vqhip_sqindex_add_rows_device(x, dev_rows, b); });
    }
    std::vector<std::uint32_t> add_codes(const std::uint8_t *codes, std::size_t b) {
        return append(codes, b, [&](vqhip_sqindex *x) { return vqhip_sqindex_add_codes(x, codes, b); });
    }
    std::vector<std::uint32_t> add_codes_device(const void *dev_codes, std::size_t b) {
        return append(dev_codes, b, [&](vqhip_sqindex *x) { return vqhip_sqindex_add_codes_device(x, dev_codes, b); });
    }

   private:
    void init(const void *src, bool rows, std::size_t n, std::size_t dim, Distance distance) {
        check_shape(n, dim);
        vqhip_sqindex *x = nullptr;
        const std::uint32_t levels = (std::uint32_t)quantizer_.levels();
        if (rows)
            detail::check(vqhip_sqindex_create_rows(quantizer_.min(), quantizer_.max(), levels, static_cast<const float *>(src), n,
                                                    (std::uint32_t)dim, (int)distance.kind(), &x));
        else
            detail::check(vqhip_sqindex_create(quantizer_.min(), quantizer_.max(), levels, static_cast<const std::uint8_t *>(src), n,
                                               (std::uint32_t)dim, (int)distance.kind(), &x));
        adopt(x, n, dim, distance);
    }
    ScalarQuantizer quantizer_;
};

// Exact index of f32 queries (never quantized) over BQ bits packed 32 to a word on the device (include/vqhip.h,
// vqhip_abin_*): BinaryIndex's rows and word layout, but the distance is Distance::compute(q, v(bits)) with v(bit) = bit ?
// high : low, under any metric, cosine included.  Every result equals FlatIndex over the dequantized rows and ScalarIndex
// over the bits as 0/1 bytes under ScalarQuantizer(low, high, 2): (row index, distance) pairs [nq][topk], nearest first,
// NaN last, ties to the lower row.  Built from f32 rows, u8 codes or packed words [n][ceil(dim / 32)] (pad bits zero); the
// twin of a BinaryIndex b is AsymmetricBinaryIndex(b.packed().data(), b.size(), b.dim(), b.quantizer(), distance).  The
// arguments are checked before the device is touched.
class AsymmetricBinaryIndex
    : public detail::ExactResidentIndex<vqhip_abin, vqhip_abin_destroy, vqhip_abin_search, vqhip_abin_range_search, vqhip_abin_rerank,
                                        vqhip_abin_search_masked, vqhip_abin_range_search_masked, vqhip_abin_remove,
                                        vqhip_abin_remove_device> {
   public:
    using Source = BinaryIndex::Source;
    AsymmetricBinaryIndex(const float *rows, std::size_t n, std::size_t dim, BinaryQuantizer quantizer = BinaryQuantizer(0.0f, 0, 1),
                          Distance distance = Distance())
        : quantizer_(quantizer) {
        init(rows, Source::Rows, n, dim, distance);
    }
    AsymmetricBinaryIndex(const std::uint8_t *codes, std::size_t n, std::size_t dim, BinaryQuantizer quantizer, Distance distance = Distance())
        : quantizer_(quantizer) {
        init(codes, Source::Codes, n, dim, distance);
    }
    AsymmetricBinaryIndex(const std::uint32_t *words, std::size_t n, std::size_t dim, BinaryQuantizer quantizer, Distance distance = Distance())
        : quantizer_(quantizer) {
        init(words, Source::Packed, n, dim, distance);
    }
    std::size_t words_per_row() const { return (dim_ + 31) / 32; }
    const BinaryQuantizer &quantizer() const { return quantizer_; }
    // the packed rows [n][words_per_row()]
    std::vector<std::uint32_t> packed() const {
        std::vector<std::uint32_t> out(n_ * words_per_row());
        detail::check(vqhip_abin_packed(ix_.get(), out.data()));
        return out;
    }
    // append b rows in one of the constructors' three forms, from host memory or from a device pointer (f32 rows and words
    // 4-byte aligned; a pad bit set there is an FfiError that leaves the index as it was); returns their ids n .. n + b - 1
    std::vector<std::uint32_t> add(const float *rows, std::size_t b) { return add_from(rows, Source::Rows, b, false); }
    std::vector<std::uint32_t> add_codes(const std::uint8_t *codes, std::size_t b) { return add_from(codes, Source::Codes, b, false); }
    std::vector<std::uint32_t> add_packed(const std::uint32_t *words, std::size_t b) {
        if (words) detail::check_pad_bits(words, b, dim_);
        return add_from(words, Source::Packed, b, false);
    }
    std::vector<std::uint32_t> add_device(const void *dev_src, Source kind, std::size_t b) { return add_from(dev_src, kind, b, true); }

   private:
    std::vector<std::uint32_t> add_from(const void *src, Source kind, std::size_t b, bool device) {
        return append(src, b, [&](vqhip_abin *h) {
            return device ? vqhip_abin_add_device(h, src, (int)kind, b) : vqhip_abin_add(h, src, (int)kind, b);
        });
    }
    void init(const void *src, Source kind, std::size_t n, std::size_t dim, Distance distance) {
        if (n == 0) throw VqError::EmptyInput();
        if (dim == 0 || dim > VQHIP_BINARY_MAX_DIM) throw VqError::InvalidParameter("dim", "must be between 1 and 8192");
        if (n >= (std::size_t(1) << 32)) throw VqError::InvalidParameter("rows", "at most 2^32 - 1 rows");
        if (kind == Source::Packed && src) detail::check_pad_bits(static_cast<const std::uint32_t *>(src), n, dim);
        vqhip_abin *x = nullptr;
        detail::check(vqhip_abin_create(src, (int)kind, n, (std::uint32_t)dim, quantizer_.threshold(), quantizer_.low(), quantizer_.high(),
                                        (int)distance.kind(), &x));
        adopt(x, n, dim, distance);
    }
    BinaryQuantizer quantizer_;
};

// Exact index of f32 queries (never quantized) over SQ codes of at most 16 levels kept on the device at four bits a
// dimension (include/vqhip.h, vqhip_sq4index_*): dimension t of a row in bits 4 (t % 8) .. + 3 of its word t / 8, pad
// nibbles zero.  Distance::compute(q, v(codes)) with v(c) = min + (float)c * step for every nibble value, under any metric,
// cosine included.  Every result equals ScalarIndex over the same codes as bytes and FlatIndex over the dequantized rows:
// (row index, distance) pairs [nq][topk], nearest first, NaN last, ties to the lower row.  Built from f32 rows (encoded and
// packed on the device), u8 codes (each <= 15) or packed words [n][ceil(dim / 8)].  The arguments are checked before the
// device is touched.
class Scalar4Index
    : public detail::ExactResidentIndex<vqhip_sq4index, vqhip_sq4index_destroy, vqhip_sq4index_search, vqhip_sq4index_range_search,
                                        vqhip_sq4index_rerank, vqhip_sq4index_search_masked, vqhip_sq4index_range_search_masked,
                                        vqhip_sq4index_remove, vqhip_sq4index_remove_device> {
   public:
    enum class Source { Rows = VQHIP_SQ4_F32, Codes = VQHIP_SQ4_U8, Packed = VQHIP_SQ4_PACKED };
    Scalar4Index(const float *rows, std::size_t n, std::size_t dim, ScalarQuantizer quantizer, Distance distance = Distance())
        : quantizer_(quantizer) {
        init(rows, Source::Rows, n, dim, distance);
    }
    Scalar4Index(const std::uint8_t *codes, std::size_t n, std::size_t dim, ScalarQuantizer quantizer, Distance distance = Distance())
        : quantizer_(quantizer) {
        init(codes, Source::Codes, n, dim, distance);
    }
    Scalar4Index(const std::uint32_t *words, std::size_t n, std::size_t dim, ScalarQuantizer quantizer, Distance distance = Distance())
        : quantizer_(quantizer) {
        init(words, Source::Packed, n, dim, distance);
    }
    std::size_t words_per_row() const { return (dim_ + 7) / 8; }
    const ScalarQuantizer &quantizer() const { return quantizer_; }
    // the packed rows [n][words_per_row()]
    std::vector<std::uint32_t> packed() const {
        std::vector<std::uint32_t> out(n_ * words_per_row());
        detail::check(vqhip_sq4index_packed(ix_.get(), out.data()));
        return out;
    }
    // the codes unpacked [n][dim]
    std::vector<std::uint8_t> codes() const {
        const std::vector<std::uint32_t> words = packed();
        const std::size_t W = words_per_row();
        std::vector<std::uint8_t> out(n_ * dim_);
        for (std::size_t i = 0; i < n_; ++i)
            for (std::size_t t = 0; t < dim_; ++t) out[i * dim_ + t] = (std::uint8_t)((words[i * W + t / 8] >> (4 * (t % 8))) & 15u);
        return out;
    }
    // append b rows in one of the constructors' three forms, from host memory or from a device pointer (f32 rows and words
    // 4-byte aligned; a code above 15 or a pad nibble set there is an FfiError that leaves the index as it was); returns
    // their ids n .. n + b - 1
    std::vector<std::uint32_t> add(const float *rows, std::size_t b) { return add_from(rows, Source::Rows, b, false); }
    std::vector<std::uint32_t> add_codes(const std::uint8_t *codes, std::size_t b) {
        if (codes) check_codes(codes, b, dim_);
        return add_from(codes, Source::Codes, b, false);
    }
    std::vector<std::uint32_t> add_packed(const std::uint32_t *words, std::size_t b) {
        if (words) check_pad_nibbles(words, b, dim_);
        return add_from(words, Source::Packed, b, false);
    }
    std::vector<std::uint32_t> add_device(const void *dev_src, Source kind, std::size_t b) { return add_from(dev_src, kind, b, true); }

   private:
    static void check_codes(const std::uint8_t *codes, std::size_t n, std::size_t dim) {
        for (std::size_t i = 0; i < n * dim; ++i)
            if (codes[i] > 15) throw VqError::InvalidParameter("codes", "a 4-bit code is at most 15");
    }
    static void check_pad_nibbles(const std::uint32_t *words, std::size_t n, std::size_t dim) {
        if (dim % 8 == 0) return;
        const std::size_t W = (dim + 7) / 8;
        const std::uint32_t keep = (1u << (4 * (dim % 8))) - 1u;
        for (std::size_t i = 0; i < n; ++i)
            if (words[i * W + W - 1] & ~keep) throw VqError::InvalidParameter("words", "a row has a pad nibble set");
    }
    std::vector<std::uint32_t> add_from(const void *src, Source kind, std::size_t b, bool device) {
        return append(src, b, [&](vqhip_sq4index *h) {
            return device ? vqhip_sq4index_add_device(h, src, (int)kind, b) : vqhip_sq4index_add(h, src, (int)kind, b);
        });
    }
    void init(const void *src, Source kind, std::size_t n, std::size_t dim, Distance distance) {
        check_shape(n, dim);
        if (quantizer_.levels() > 16) throw VqError::InvalidParameter("quantizer", "a 4-bit index holds at most 16 levels");
        if (kind == Source::Codes && src) check_codes(static_cast<const std::uint8_t *>(src), n, dim);
        if (kind == Source::Packed && src) check_pad_nibbles(static_cast<const std::uint32_t *>(src), n, dim);
        vqhip_sq4index *x = nullptr;
        detail::check(vqhip_sq4index_create(quantizer_.min(), quantizer_.max(), (std::uint32_t)quantizer_.levels(), src, (int)kind, n,
                                            (std::uint32_t)dim, (int)distance.kind(), &x));
        adopt(x, n, dim, distance);
    }
    ScalarQuantizer quantizer_;
};

namespace detail {
// What the inverted-file indexes share over their C handles (H and its destroy / list_sizes / probe / search):
// the shape, the add-side and probe-side checks, and the calls whose arguments are the same for every payload.
template <class H, int (*Destroy)(H *), int (*ListSizes)(H *, std::uint64_t *),
          int (*Probe)(H *, const float *, std::uint32_t, std::uint32_t, std::uint32_t *),
          int (*Search)(H *, const float *, std::uint32_t, std::uint32_t, std::uint32_t, std::uint32_t *, float *),
          int (*Remove)(H *, const std::uint32_t *, std::uint64_t *), int (*Uploads)(const H *, std::uint64_t *)>
class IvfIndex {
   public:
    std::size_t size() const { return n_; }
    std::size_t nlist() const { return nlist_; }
    std::size_t dim() const { return dim_; }
    const char *distance_metric() const { return distance_.name(); }
    std::vector<std::uint64_t> list_sizes() const {
        std::vector<std::uint64_t> s(nlist_);
        check(ListSizes(ix_.get(), s.data()));
        return s;
    }

    struct Result {
        std::vector<std::uint32_t> idx;  // [nq][topk]
        std::vector<float> dist;         // [nq][topk]
    };
    // queries [nq][dim] -> the lists each query scans [nq][nprobe], nearest first
    std::vector<std::uint32_t> probe(const float *queries, std::size_t nq, std::size_t nprobe) const {
        check_probe(nprobe, nq);
        std::vector<std::uint32_t> out(nq * nprobe);
        if (nq) check(Probe(ix_.get(), queries, (std::uint32_t)nq, (std::uint32_t)nprobe, out.data()));
        return out;
    }
    Result search(const float *queries, std::size_t nq, std::size_t topk, std::size_t nprobe) const {
        check_probe(nprobe, nq);
        if (topk == 0 || topk > 1024 || topk > n_) throw VqError::InvalidParameter("topk", "must be between 1 and min(n, 1024)");
        Result r{std::vector<std::uint32_t>(nq * topk), std::vector<float>(nq * topk)};
        if (nq)
            check(Search(ix_.get(), queries, (std::uint32_t)nq, (std::uint32_t)nprobe, (std::uint32_t)topk, r.idx.data(), r.dist.data()));
        return r;
    }

    // Removing rows (include/vqhip.h, "removing rows from an inverted file"): `remove` [n], true: the row goes (or row ids,
    // through remove_mask).  The other rows keep their order and their lists and move up; returns the old ids of the
    // remaining rows in their new order.  Removing every row is allowed: the index is then empty, and adds work.  After any
    // sequence of adds and removals every call returns bit for bit what a fresh index given the remaining rows in one add
    // returns.  A device state that is current stays current; without one no device is touched.
    std::vector<std::uint32_t> remove_rows(const std::vector<bool> &remove) {
        if (remove.size() != n_) throw VqError::DimensionMismatch(n_, remove.size());
        std::vector<std::uint32_t> kept;
        for (std::size_t i = 0; i < n_; ++i)
            if (!remove[i]) kept.push_back((std::uint32_t)i);
        if (kept.size() == n_) return kept;
        const std::vector<std::uint32_t> words = pack_row_mask(remove);
        std::uint64_t gone = 0;
        check(Remove(ix_.get(), words.data(), &gone));
        n_ = kept.size();
        return kept;
    }
    std::vector<std::uint32_t> remove_rows(const std::vector<std::uint32_t> &ids) { return remove_rows(remove_mask(ids, n_)); }
    // how many times the device state has been built from the host rows (by the first probe or search, and by the first
    // one after an add): a removal does not move it
    std::uint64_t uploads() const {
        std::uint64_t u = 0;
        check(Uploads(ix_.get(), &u));
        return u;
    }

   protected:
    static void check_nlist(std::size_t nlist) {
        if (nlist == 0 || nlist > 65536) throw VqError::InvalidParameter("nlist", "must be between 1 and 65536");
    }
    static void check_dim(std::size_t dim) {
        if (dim == 0 || dim > 0xFFFFFFFFu) throw VqError::InvalidParameter("dim", "must be between 1 and 2^32 - 1");
    }
    void adopt(H *ix, std::size_t nlist, std::size_t dim, Distance distance) {
        ix_.reset(ix);
        nlist_ = nlist;
        dim_ = dim;
        distance_ = distance;
    }
    void check_add(const std::uint32_t *list_ids, std::size_t n, const char *what) const {
        if (n >= (std::size_t(1) << 32) - n_) throw VqError::InvalidParameter(what, "an index holds at most 2^32 - 1 rows");
        for (std::size_t i = 0; i < n; ++i)
            if (list_ids[i] >= nlist_) throw VqError::InvalidParameter("list_ids", "a list id is outside [0, nlist)");
    }
    // n rows are in (rc: the C add's result, VQHIP_OK when n == 0 and it was not called); the first new row id
    std::size_t added(std::size_t n, int rc) {
        check(rc);
        const std::size_t first = n_;
        n_ += n;
        return first;
    }
    void check_probe(std::size_t nprobe, std::size_t nq) const {
        if (nprobe == 0 || nprobe > 1024 || nprobe > nlist_)
            throw VqError::InvalidParameter("nprobe", "must be between 1 and min(nlist, 1024)");
        if (nq >= (std::size_t(1) << 32)) throw VqError::InvalidParameter("queries", "at most 2^32 - 1 per call");
    }
    struct Del {
        void operator()(H *p) const { (void)Destroy(p); }
    };
    std::unique_ptr<H, Del> ix_;
    std::size_t n_ = 0, nlist_ = 0, dim_ = 0;
    Distance distance_;

    // the range search of the two indexes of exact distances (IVFFlatIndex, IVFScalarIndex; not IVFPQIndex, whose
    // distances are approximations)
    template <int (*Range)(H *, const float *, std::uint32_t, std::uint32_t, const float *, std::uint64_t, vqhip_range **)>
    RangeResult range(const float *queries, std::size_t nq, const float *radii, std::size_t nprobe, std::uint64_t max_results) const {
        check_range_args(radii, nq, max_results);
        check_probe(nprobe, nq);
        if (nq == 0) return RangeResult{std::vector<std::uint64_t>(1, 0), {}, {}};
        vqhip_range *r = nullptr;
        check(Range(ix_.get(), queries, (std::uint32_t)nq, (std::uint32_t)nprobe, radii, max_results, &r));
        return read_range(r);
    }
    // The filtered forms of the same two indexes: `allowed` is the row mask of the call, ceil(n / 32) words for the n rows
    // the index holds now (pack_row_mask).  Probing takes no mask; the searched set is the allowed rows of the probed lists.
    template <int (*SearchMasked)(H *, const float *, std::uint32_t, std::uint32_t, std::uint32_t, const std::uint32_t *, std::uint32_t *,
                                  float *)>
    Result masked(const float *queries, std::size_t nq, std::size_t topk, std::size_t nprobe, const std::uint32_t *allowed) const {
        check_row_mask(allowed);
        check_probe(nprobe, nq);
        if (topk == 0 || topk > 1024 || topk > n_) throw VqError::InvalidParameter("topk", "must be between 1 and min(n, 1024)");
        Result r{std::vector<std::uint32_t>(nq * topk), std::vector<float>(nq * topk)};
        if (nq)
            check(SearchMasked(ix_.get(), queries, (std::uint32_t)nq, (std::uint32_t)nprobe, (std::uint32_t)topk, allowed, r.idx.data(),
                               r.dist.data()));
        return r;
    }
    template <int (*RangeMasked)(H *, const float *, std::uint32_t, std::uint32_t, const float *, std::uint64_t, const std::uint32_t *,
                                 vqhip_range **)>
    RangeResult range_masked(const float *queries, std::size_t nq, const float *radii, std::size_t nprobe, std::uint64_t max_results,
                             const std::uint32_t *allowed) const {
        check_row_mask(allowed);
        check_range_args(radii, nq, max_results);
        check_probe(nprobe, nq);
        if (nq == 0) return RangeResult{std::vector<std::uint64_t>(1, 0), {}, {}};
        vqhip_range *r = nullptr;
        check(RangeMasked(ix_.get(), queries, (std::uint32_t)nq, (std::uint32_t)nprobe, radii, max_results, allowed, &r));
        return read_range(r);
    }
    // the vector forms' checks: the mask's length against the rows the index holds, whole queries, one radius per query
    std::size_t check_masked_vectors(const std::vector<float> &queries, const std::vector<std::uint32_t> &allowed,
                                     const std::vector<float> *radii) const {
        check_row_mask(allowed, n_);
        if (queries.size() % dim_) throw VqError::DimensionMismatch(dim_, queries.size() % dim_);
        const std::size_t nq = queries.size() / dim_;
        if (radii && radii->size() != nq) throw VqError::DimensionMismatch(nq, radii->size());
        return nq;
    }
};
}  // namespace detail

// Inverted-file index over PQ codes (include/vqhip.h, vqhip_ivfpq_*): coarse centroids [nlist][dim], codebooks
// [m][k][sub_dim], rows added as (list id, codes).  search scans only the nprobe lists nearest to a query and gives
// (row id, ADC distance) pairs [nq][topk], nearest first; slots past the probed rows hold (0xFFFFFFFF, +inf).  The
// constructor, add and list_sizes need no device; the arguments are checked before the device is touched.
class IVFPQIndex
    : public detail::IvfIndex<vqhip_ivfpq, vqhip_ivfpq_destroy, vqhip_ivfpq_list_sizes, vqhip_ivfpq_probe, vqhip_ivfpq_search,
                              vqhip_ivfpq_remove, vqhip_ivfpq_uploads> {
   public:
    // residual: the codes of a row in list l quantise x - C[l] (include/vqhip.h, VQHIP_IVF_RESIDUAL)
    IVFPQIndex(const float *coarse, std::size_t nlist, const float *codebooks, std::size_t m, std::size_t k, std::size_t sub_dim,
               Distance distance = Distance(), bool residual = false) {
        check_nlist(nlist);
        if (m == 0 || k == 0 || sub_dim == 0) throw VqError::InvalidParameter("codebooks", "m, k and sub_dim must be positive");
        if (k > 65536 || m * k > 38400) throw VqError::InvalidParameter("codebooks", "m * k must be at most 38400");
        if (m * sub_dim > 0xFFFFFFFFu) throw VqError::InvalidParameter("codebooks", "dim must be below 2^32");
        if (distance.kind() == Distance::CosineDistance)
            throw VqError::InvalidParameter("distance", "cosine distance is not a sum over subspaces: no ADC form");
        vqhip_ivfpq *ix = nullptr;
        detail::check(vqhip_ivfpq_create_ex(coarse, (std::uint32_t)nlist, codebooks, (std::uint32_t)m, (std::uint32_t)k,
                                            (std::uint32_t)sub_dim, (int)distance.kind(), residual ? VQHIP_IVF_RESIDUAL : 0u, &ix));
        adopt(ix, nlist, m * sub_dim, distance);
        m_ = m;
        k_ = k;
        residual_ = residual;
    }
    bool residual() const { return residual_; }

    // rows appended in order: list_ids [n] < nlist, codes [n][m] < k (one byte per code up to k = 256, u16 above: the
    // library's code width); returns the first new row id
    std::size_t add(const std::uint32_t *list_ids, const void *codes, std::size_t n) {
        check_add(list_ids, n, "codes");
        for (std::size_t e = 0; e < n * m_; ++e) {
            const std::uint32_t c = k_ <= 256 ? static_cast<const std::uint8_t *>(codes)[e] : static_cast<const std::uint16_t *>(codes)[e];
            if (c >= k_) throw VqError::InvalidParameter("codes", "a code is outside [0, k)");
        }
        return added(n, n ? vqhip_ivfpq_add(ix_.get(), list_ids, codes, n) : VQHIP_OK);
    }

    // The filtered form (include/vqhip.h, vqhip_ivfpq_search_masked), plain and residual alike: the nearest among the
    // allowed rows of the probed lists by ADC distance, padded with (0xFFFFFFFF, +inf) behind fewer than topk of them.
    // `allowed` is the row mask of the call, ceil(n / 32) words for the n rows the index holds now (pack_row_mask).
    using IvfIndex::search;
    Result search(const float *queries, std::size_t nq, std::size_t topk, std::size_t nprobe, const std::uint32_t *allowed) const {
        return masked<vqhip_ivfpq_search_masked>(queries, nq, topk, nprobe, allowed);
    }
    Result search(const std::vector<float> &queries, std::size_t topk, std::size_t nprobe, const std::vector<std::uint32_t> &allowed) const {
        const std::size_t nq = check_masked_vectors(queries, allowed, nullptr);
        return search(queries.data(), nq, topk, nprobe, allowed.data());
    }

   private:
    std::size_t m_ = 0, k_ = 0;
    bool residual_ = false;
};

// Inverted-file index over the rows themselves (include/vqhip.h, vqhip_ivfflat_*): coarse centroids [nlist][dim], rows added
// as (list id, row) in f32 or as the f16 bits quantize returns.  search computes the exact distance (FlatIndex's, any
// metric) to the rows of the nprobe lists nearest to a query and gives (row id, distance) pairs [nq][topk], nearest
// first; slots past the probed rows hold (0xFFFFFFFF, +inf); with nprobe == nlist it is FlatIndex's search.  The
// constructor, add and list_sizes need no device; the arguments are checked before the device is touched.
class IVFFlatIndex : public detail::IvfIndex<vqhip_ivfflat, vqhip_ivfflat_destroy, vqhip_ivfflat_list_sizes, vqhip_ivfflat_probe,
                                             vqhip_ivfflat_search, vqhip_ivfflat_remove, vqhip_ivfflat_uploads> {
   public:
    enum class Rows { F32 = 0, F16 = 1 };
    IVFFlatIndex(const float *coarse, std::size_t nlist, std::size_t dim, Distance distance = Distance(), Rows rows = Rows::F32) {
        check_nlist(nlist);
        check_dim(dim);
        vqhip_ivfflat *ix = nullptr;
        detail::check(vqhip_ivfflat_create(coarse, (std::uint32_t)nlist, (std::uint32_t)dim, (int)rows, (int)distance.kind(), &ix));
        adopt(ix, nlist, dim, distance);
        rows_ = rows;
    }
    Rows rows() const { return rows_; }

    // every row of the nprobe nearest lists within radii[q] of query q (D <= radius as a float comparison; NaN never
    // hits), CSR and in ascending row id; with nprobe == nlist it is FlatIndex's range_search.  More than max_results
    // hits: VqError (UNSUPPORTED)
    RangeResult range_search(const float *queries, std::size_t nq, const float *radii, std::size_t nprobe,
                             std::uint64_t max_results = std::uint64_t(1) << 28) const {
        return range<vqhip_ivfflat_range_search>(queries, nq, radii, nprobe, max_results);
    }

    // The filtered forms (include/vqhip.h, vqhip_ivfflat_search_masked / _range_search_masked): the nearest among the allowed
    // rows of the probed lists, padded with (0xFFFFFFFF, +inf) behind fewer than topk of them; only allowed rows hit a range
    // query.  With nprobe == nlist they are FlatIndex's filtered search and range_search.  The mask comes last, and
    // max_results has no default beside it, so that a literal 0 never reads as a null mask.
    using IvfIndex::search;
    Result search(const float *queries, std::size_t nq, std::size_t topk, std::size_t nprobe, const std::uint32_t *allowed) const {
        return masked<vqhip_ivfflat_search_masked>(queries, nq, topk, nprobe, allowed);
    }
    Result search(const std::vector<float> &queries, std::size_t topk, std::size_t nprobe, const std::vector<std::uint32_t> &allowed) const {
        const std::size_t nq = check_masked_vectors(queries, allowed, nullptr);
        return search(queries.data(), nq, topk, nprobe, allowed.data());
    }
    RangeResult range_search(const float *queries, std::size_t nq, const float *radii, std::size_t nprobe, std::uint64_t max_results,
                             const std::uint32_t *allowed) const {
        return range_masked<vqhip_ivfflat_range_search_masked>(queries, nq, radii, nprobe, max_results, allowed);
    }
    RangeResult range_search(const std::vector<float> &queries, const std::vector<float> &radii, std::size_t nprobe,
                             std::uint64_t max_results, const std::vector<std::uint32_t> &allowed) const {
        const std::size_t nq = check_masked_vectors(queries, allowed, &radii);
        return range_search(queries.data(), nq, radii.data(), nprobe, max_results, allowed.data());
    }

    // rows appended in order: list_ids [n] < nlist, rows [n][dim] in the index's row type; returns the first new row id
    std::size_t add(const std::uint32_t *list_ids, const void *rows, std::size_t n) {
        check_add(list_ids, n, "rows");
        return added(n, n ? vqhip_ivfflat_add(ix_.get(), list_ids, rows, n) : VQHIP_OK);
    }

   private:
    Rows rows_ = Rows::F32;
};

// Inverted-file index over SQ codes (include/vqhip.h, vqhip_ivfsq_*): coarse centroids [nlist][dim], a ScalarQuantizer, rows
// added as (list id, u8 codes) or as (list id, f32 row) encoded on the device.  search computes the exact distance
// (FlatIndex's, any metric) to the dequantized rows of the nprobe lists nearest to a query and gives (row id, distance)
// pairs [nq][topk], nearest first; slots past the probed rows hold (0xFFFFFFFF, +inf).  Every result equals IVFFlatIndex
// over quantizer.dequantize(codes) in the same lists; with nprobe == nlist it is ScalarIndex's search.  The constructor,
// add_codes, codes and list_sizes need no device; the arguments are checked before the device is touched.
class IVFScalarIndex
    : public detail::IvfIndex<vqhip_ivfsq, vqhip_ivfsq_destroy, vqhip_ivfsq_list_sizes, vqhip_ivfsq_probe, vqhip_ivfsq_search,
                              vqhip_ivfsq_remove, vqhip_ivfsq_uploads> {
   public:
    IVFScalarIndex(const float *coarse, std::size_t nlist, std::size_t dim, ScalarQuantizer quantizer, Distance distance = Distance())
        : quantizer_(quantizer) {
        check_nlist(nlist);
        check_dim(dim);
        vqhip_ivfsq *ix = nullptr;
        detail::check(vqhip_ivfsq_create(quantizer_.min(), quantizer_.max(), (std::uint32_t)quantizer_.levels(), coarse,
                                         (std::uint32_t)nlist, (std::uint32_t)dim, (int)distance.kind(), &ix));
        adopt(ix, nlist, dim, distance);
    }
    const ScalarQuantizer &quantizer() const { return quantizer_; }

    // IVFFlatIndex's range_search over the dequantized rows; with nprobe == nlist it is ScalarIndex's range_search
    RangeResult range_search(const float *queries, std::size_t nq, const float *radii, std::size_t nprobe,
                             std::uint64_t max_results = std::uint64_t(1) << 28) const {
        return range<vqhip_ivfsq_range_search>(queries, nq, radii, nprobe, max_results);
    }

    // The filtered forms (include/vqhip.h, vqhip_ivfsq_search_masked / _range_search_masked): the nearest among the allowed
    // rows of the probed lists, padded with (0xFFFFFFFF, +inf) behind fewer than topk of them; only allowed rows hit a range
    // query.  With nprobe == nlist they are ScalarIndex's filtered search and range_search.  The mask comes last, and
    // max_results has no default beside it, so that a literal 0 never reads as a null mask.
    using IvfIndex::search;
    Result search(const float *queries, std::size_t nq, std::size_t topk, std::size_t nprobe, const std::uint32_t *allowed) const {
        return masked<vqhip_ivfsq_search_masked>(queries, nq, topk, nprobe, allowed);
    }
    Result search(const std::vector<float> &queries, std::size_t topk, std::size_t nprobe, const std::vector<std::uint32_t> &allowed) const {
        const std::size_t nq = check_masked_vectors(queries, allowed, nullptr);
        return search(queries.data(), nq, topk, nprobe, allowed.data());
    }
    RangeResult range_search(const float *queries, std::size_t nq, const float *radii, std::size_t nprobe, std::uint64_t max_results,
                             const std::uint32_t *allowed) const {
        return range_masked<vqhip_ivfsq_range_search_masked>(queries, nq, radii, nprobe, max_results, allowed);
    }
    RangeResult range_search(const std::vector<float> &queries, const std::vector<float> &radii, std::size_t nprobe,
                             std::uint64_t max_results, const std::vector<std::uint32_t> &allowed) const {
        const std::size_t nq = check_masked_vectors(queries, allowed, &radii);
        return range_search(queries.data(), nq, radii.data(), nprobe, max_results, allowed.data());
    }

    // rows appended in order: list_ids [n] < nlist, codes [n][dim] (every byte value is legal); returns the first new row id
    std::size_t add_codes(const std::uint32_t *list_ids, const std::uint8_t *codes, std::size_t n) {
        check_add(list_ids, n, "codes");
        return added(n, n ? vqhip_ivfsq_add_codes(ix_.get(), list_ids, codes, n) : VQHIP_OK);
    }
    // rows [n][dim] f32, encoded on the device (the quantizer's codes); only the codes are kept
    std::size_t add_rows(const std::uint32_t *list_ids, const float *rows, std::size_t n) {
        check_add(list_ids, n, "rows");
        return added(n, n ? vqhip_ivfsq_add_rows(ix_.get(), list_ids, rows, n) : VQHIP_OK);
    }
    // the codes [n][dim], in add order
    std::vector<std::uint8_t> codes() const {
        std::vector<std::uint8_t> out(n_ * dim_);
        detail::check(vqhip_ivfsq_codes(ix_.get(), out.data()));
        return out;
    }

   private:
    ScalarQuantizer quantizer_;
};

// Inverted-file index over 4-bit SQ codes (include/vqhip.h, vqhip_ivfsq4_*): IVFScalarIndex for a ScalarQuantizer of at most
// 16 levels, each row kept at four bits a dimension, eight dimensions a u32 word (Scalar4Index's layout, pad nibbles zero).
// Rows are added as (list id, u8 codes <= 15) or (list id, packed words), both on the host, or as (list id, f32 row) encoded
// and packed on the device.  Every result equals IVFScalarIndex over the same codes in the same lists, bit for bit; with
// nprobe == nlist it is Scalar4Index's search.  The constructor, add_codes, add_packed, codes, packed and list_sizes need
// no device; the arguments are checked before the device is touched.
class IVFScalar4Index
    : public detail::IvfIndex<vqhip_ivfsq4, vqhip_ivfsq4_destroy, vqhip_ivfsq4_list_sizes, vqhip_ivfsq4_probe, vqhip_ivfsq4_search,
                              vqhip_ivfsq4_remove, vqhip_ivfsq4_uploads> {
   public:
    IVFScalar4Index(const float *coarse, std::size_t nlist, std::size_t dim, ScalarQuantizer quantizer, Distance distance = Distance())
        : quantizer_(quantizer) {
        check_nlist(nlist);
        check_dim(dim);
        if (quantizer_.levels() > 16) throw VqError::InvalidParameter("quantizer", "a 4-bit index holds at most 16 levels");
        vqhip_ivfsq4 *ix = nullptr;
        detail::check(vqhip_ivfsq4_create(quantizer_.min(), quantizer_.max(), (std::uint32_t)quantizer_.levels(), coarse,
                                          (std::uint32_t)nlist, (std::uint32_t)dim, (int)distance.kind(), &ix));
        adopt(ix, nlist, dim, distance);
    }
    const ScalarQuantizer &quantizer() const { return quantizer_; }
    std::size_t words() const { return (dim_ + 7) / 8; }  // u32 words of a row

    // IVFFlatIndex's range_search over the dequantized rows; with nprobe == nlist it is Scalar4Index's range_search
    RangeResult range_search(const float *queries, std::size_t nq, const float *radii, std::size_t nprobe,
                             std::uint64_t max_results = std::uint64_t(1) << 28) const {
        return range<vqhip_ivfsq4_range_search>(queries, nq, radii, nprobe, max_results);
    }

    // The filtered forms (include/vqhip.h, vqhip_ivfsq4_search_masked / _range_search_masked), as IVFScalarIndex's
    using IvfIndex::search;
    Result search(const float *queries, std::size_t nq, std::size_t topk, std::size_t nprobe, const std::uint32_t *allowed) const {
        return masked<vqhip_ivfsq4_search_masked>(queries, nq, topk, nprobe, allowed);
    }
    Result search(const std::vector<float> &queries, std::size_t topk, std::size_t nprobe, const std::vector<std::uint32_t> &allowed) const {
        const std::size_t nq = check_masked_vectors(queries, allowed, nullptr);
        return search(queries.data(), nq, topk, nprobe, allowed.data());
    }
    RangeResult range_search(const float *queries, std::size_t nq, const float *radii, std::size_t nprobe, std::uint64_t max_results,
                             const std::uint32_t *allowed) const {
        return range_masked<vqhip_ivfsq4_range_search_masked>(queries, nq, radii, nprobe, max_results, allowed);
    }
    RangeResult range_search(const std::vector<float> &queries, const std::vector<float> &radii, std::size_t nprobe,
                             std::uint64_t max_results, const std::vector<std::uint32_t> &allowed) const {
        const std::size_t nq = check_masked_vectors(queries, allowed, &radii);
        return range_search(queries.data(), nq, radii.data(), nprobe, max_results, allowed.data());
    }

    // rows appended in order: list_ids [n] < nlist, codes [n][dim], each <= 15 (codes >= levels are legal); returns the
    // first new row id.  A refused add leaves the index as it was.
    std::size_t add_codes(const std::uint32_t *list_ids, const std::uint8_t *codes, std::size_t n) {
        check_add(list_ids, n, "codes");
        for (std::size_t e = 0; e < n * dim_; ++e)
            if (codes[e] > 15) throw VqError::InvalidParameter("codes", "a 4-bit code is at most 15");
        return added(n, n ? vqhip_ivfsq4_add_codes(ix_.get(), list_ids, codes, n) : VQHIP_OK);
    }
    // words [n][words()] in the index layout, pad nibbles zero
    std::size_t add_packed(const std::uint32_t *list_ids, const std::uint32_t *packed, std::size_t n) {
        check_add(list_ids, n, "words");
        if (dim_ % 8) {
            const std::uint32_t keep = (std::uint32_t(1) << (4 * (dim_ % 8))) - 1u;
            for (std::size_t i = 0; i < n; ++i)
                if (packed[i * words() + words() - 1] & ~keep) throw VqError::InvalidParameter("words", "a row has a pad nibble set");
        }
        return added(n, n ? vqhip_ivfsq4_add_packed(ix_.get(), list_ids, packed, n) : VQHIP_OK);
    }
    // rows [n][dim] f32, encoded and packed on the device (the quantizer's codes); only the words are kept
    std::size_t add_rows(const std::uint32_t *list_ids, const float *rows, std::size_t n) {
        check_add(list_ids, n, "rows");
        return added(n, n ? vqhip_ivfsq4_add_rows(ix_.get(), list_ids, rows, n) : VQHIP_OK);
    }
    // the codes unpacked [n][dim] and the words [n][words()], in add order
    std::vector<std::uint8_t> codes() const {
        std::vector<std::uint8_t> out(n_ * dim_);
        detail::check(vqhip_ivfsq4_codes(ix_.get(), out.data()));
        return out;
    }
    std::vector<std::uint32_t> packed() const {
        std::vector<std::uint32_t> out(n_ * words());
        detail::check(vqhip_ivfsq4_packed(ix_.get(), out.data()));
        return out;
    }

   private:
    ScalarQuantizer quantizer_;
};

// Inverted-file index over packed BQ bits (include/vqhip.h, vqhip_ivfbin_*): coarse centroids [nlist][dim], a BinaryQuantizer,
// rows added as (list id, packed words [ceil(dim / 32)]), as (list id, u8 codes) packed on the host, or as (list id, f32
// row) packed on the device.  search computes the Hamming distance to the rows of the nprobe lists nearest to the f32
// query under coarse_distance and reports BinaryIndex's distance for it under `distance` (squared Euclidean, Euclidean or
// Manhattan; cosine is refused); (row id, distance) pairs [nq][topk], nearest first, ties to the lower row; slots past the
// probed rows hold (0xFFFFFFFF, +inf); with nprobe == nlist it is BinaryIndex's search.  The constructor, add_packed,
// add_codes, packed and list_sizes need no device; the arguments are checked before the device is touched.
class IVFBinaryIndex
    : public detail::IvfIndex<vqhip_ivfbin, vqhip_ivfbin_destroy, vqhip_ivfbin_list_sizes, vqhip_ivfbin_probe, vqhip_ivfbin_search,
                              vqhip_ivfbin_remove, vqhip_ivfbin_uploads> {
   public:
    IVFBinaryIndex(const float *coarse, std::size_t nlist, std::size_t dim, BinaryQuantizer quantizer = BinaryQuantizer(0.0f, 0, 1),
                   Distance distance = Distance(Distance::Manhattan), Distance coarse_distance = Distance())
        : quantizer_(quantizer), coarse_distance_(coarse_distance) {
        check_nlist(nlist);
        if (dim == 0 || dim > VQHIP_BINARY_MAX_DIM) throw VqError::InvalidParameter("dim", "must be between 1 and 8192");
        if (distance.kind() == Distance::CosineDistance)
            throw VqError::InvalidParameter("distance", "cosine is not a function of the Hamming distance alone");
        vqhip_ivfbin *ix = nullptr;
        detail::check(vqhip_ivfbin_create(quantizer_.threshold(), quantizer_.low(), quantizer_.high(), coarse, (std::uint32_t)nlist,
                                          (std::uint32_t)dim, (int)distance.kind(), (int)coarse_distance.kind(), &ix));
        adopt(ix, nlist, dim, distance);
    }
    const BinaryQuantizer &quantizer() const { return quantizer_; }
    const char *coarse_distance_metric() const { return coarse_distance_.name(); }
    std::size_t words_per_row() const { return (dim_ + 31) / 32; }

    // every row of the nprobe nearest lists within radii[q] bits of query q (BinaryIndex::hamming_range_search's rule
    // and radii), CSR and in ascending row id; with nprobe == nlist it is BinaryIndex's hamming_range_search.  More than
    // max_results hits in all: FfiError.
    RangeResult hamming_range_search(const float *queries, std::size_t nq, const std::uint32_t *radii, std::size_t nprobe,
                                     std::uint64_t max_results = std::uint64_t(1) << 28) const {
        if (max_results == 0) throw VqError::InvalidParameter("max_results", "must be at least 1");
        check_probe(nprobe, nq);
        if (nq == 0) return RangeResult{std::vector<std::uint64_t>(1, 0), {}, {}};
        vqhip_range *r = nullptr;
        detail::check(vqhip_ivfbin_range_search(ix_.get(), queries, (std::uint32_t)nq, (std::uint32_t)nprobe, radii, max_results, &r));
        return detail::read_range(r);
    }

    // The filtered forms (include/vqhip.h, vqhip_ivfbin_search_masked / _range_search_masked): the nearest among the allowed
    // rows of the probed lists, padded with (0xFFFFFFFF, +inf) behind fewer than topk of them; only allowed rows hit a range
    // query.  `allowed`: ceil(n / 32) words for the n rows the index holds now.  With nprobe == nlist they are BinaryIndex's
    // filtered forms.  The mask comes last, and max_results has no default beside it.
    using IvfIndex::search;
    Result search(const float *queries, std::size_t nq, std::size_t topk, std::size_t nprobe, const std::uint32_t *allowed) const {
        return masked<vqhip_ivfbin_search_masked>(queries, nq, topk, nprobe, allowed);
    }
    Result search(const std::vector<float> &queries, std::size_t topk, std::size_t nprobe, const std::vector<std::uint32_t> &allowed) const {
        const std::size_t nq = check_masked_vectors(queries, allowed, nullptr);
        return search(queries.data(), nq, topk, nprobe, allowed.data());
    }
    RangeResult hamming_range_search(const float *queries, std::size_t nq, const std::uint32_t *radii, std::size_t nprobe,
                                     std::uint64_t max_results, const std::uint32_t *allowed) const {
        detail::check_row_mask(allowed);
        if (max_results == 0) throw VqError::InvalidParameter("max_results", "must be at least 1");
        check_probe(nprobe, nq);
        if (nq == 0) return RangeResult{std::vector<std::uint64_t>(1, 0), {}, {}};
        vqhip_range *r = nullptr;
        detail::check(vqhip_ivfbin_range_search_masked(ix_.get(), queries, (std::uint32_t)nq, (std::uint32_t)nprobe, radii, max_results,
                                                       allowed, &r));
        return detail::read_range(r);
    }
    RangeResult hamming_range_search(const std::vector<float> &queries, const std::vector<std::uint32_t> &radii, std::size_t nprobe,
                                     std::uint64_t max_results, const std::vector<std::uint32_t> &allowed) const {
        const std::size_t nq = check_masked_vectors(queries, allowed, nullptr);
        if (radii.size() != nq) throw VqError::DimensionMismatch(nq, radii.size());
        return hamming_range_search(queries.data(), nq, radii.data(), nprobe, max_results, allowed.data());
    }

    // rows appended in order: list_ids [n] < nlist, words [n][words_per_row()], pad bits zero; returns the first new row id
    std::size_t add_packed(const std::uint32_t *list_ids, const std::uint32_t *words, std::size_t n) {
        check_add(list_ids, n, "words");
        if (dim_ % 32) {
            const std::uint32_t mask = (1u << (dim_ % 32)) - 1u;
            const std::size_t w = words_per_row();
            for (std::size_t i = 0; i < n; ++i)
                if (words[i * w + w - 1] & ~mask) throw VqError::InvalidParameter("words", "a row has a pad bit set");
        }
        return added(n, n ? vqhip_ivfbin_add_packed(ix_.get(), list_ids, words, n) : VQHIP_OK);
    }
    // codes [n][dim] u8, packed on the host: bit = code >= high
    std::size_t add_codes(const std::uint32_t *list_ids, const std::uint8_t *codes, std::size_t n) {
        check_add(list_ids, n, "codes");
        return added(n, n ? vqhip_ivfbin_add_codes(ix_.get(), list_ids, codes, n) : VQHIP_OK);
    }
    // rows [n][dim] f32, packed on the device: bit = x >= threshold; only the words are kept
    std::size_t add_rows(const std::uint32_t *list_ids, const float *rows, std::size_t n) {
        check_add(list_ids, n, "rows");
        return added(n, n ? vqhip_ivfbin_add_rows(ix_.get(), list_ids, rows, n) : VQHIP_OK);
    }
    // the words [n][words_per_row()], in add order
    std::vector<std::uint32_t> packed() const {
        std::vector<std::uint32_t> out(n_ * words_per_row());
        detail::check(vqhip_ivfbin_packed(ix_.get(), out.data()));
        return out;
    }

   private:
    BinaryQuantizer quantizer_;
    Distance coarse_distance_;
};

// analogue of vq::get_simd_backend (src/lib.rs): names the device backend
inline std::string get_simd_backend() { return vqhip_backend(); }

}  // namespace vq
#endif  // VQ_HPP
