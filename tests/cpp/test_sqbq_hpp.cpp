// Exercises vq::ScalarQuantizer / vq::BinaryQuantizer of include/vq.hpp (tests/test_cpp_sqbq.py drives it).
//   test_sqbq_hpp validate         -- constructor checks: order, parameter names and texts (no device needed)
//   test_sqbq_hpp run <in> <out>   -- <in>: u64 count, then count f32; <out>: SQ(-1, 1, 256) codes, their
//                                     dequantize, BQ(0, 0, 1) codes, their dequantize (on the GPU)
#include <cmath>
#include <cstdio>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "vq.hpp"

using vq::VqError;

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                \
        }                                                              \
    } while (0)

template <class F>
static void expect_param(F f, const char *parameter, const char *what) {
    try {
        f();
        std::printf("FAIL no error, expected %s\n", what);
        ++failures;
    } catch (const VqError &e) {
        if (e.kind != VqError::Kind::InvalidParameter || e.parameter != parameter || std::string(e.what()) != what) {
            std::printf("FAIL got '%s' (parameter '%s'), expected '%s'\n", e.what(), e.parameter.c_str(), what);
            ++failures;
        }
    }
}

static int validate() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // src/sq.rs ScalarQuantizer::new, checks in order (a NaN min wins over a bad max or levels)
    expect_param([&] { vq::ScalarQuantizer(nan, nan, 0); }, "min", "Invalid parameter 'min': must be finite (not NaN or infinite)");
    expect_param([&] { vq::ScalarQuantizer(-inf, 1, 256); }, "min", "Invalid parameter 'min': must be finite (not NaN or infinite)");
    expect_param([&] { vq::ScalarQuantizer(0, inf, 0); }, "max", "Invalid parameter 'max': must be finite (not NaN or infinite)");
    expect_param([&] { vq::ScalarQuantizer(1, 1, 0); }, "max", "Invalid parameter 'max': must be greater than min");
    expect_param([&] { vq::ScalarQuantizer(10, 5, 256); }, "max", "Invalid parameter 'max': must be greater than min");
    expect_param([&] { vq::ScalarQuantizer(0, 1, 1); }, "levels", "Invalid parameter 'levels': must be at least 2");
    expect_param([&] { vq::ScalarQuantizer(0, 1, 300); }, "levels", "Invalid parameter 'levels': must be no more than 256 to fit in u8");
    expect_param([&] { vq::ScalarQuantizer(0, 1, (std::size_t)1 << 40); }, "levels", "Invalid parameter 'levels': must be no more than 256 to fit in u8");
    // src/bq.rs BinaryQuantizer::new
    expect_param([&] { vq::BinaryQuantizer(nan, 1, 0); }, "threshold", "Invalid parameter 'threshold': must be finite (not NaN or infinite)");
    expect_param([&] { vq::BinaryQuantizer(0, 5, 5); }, "low/high", "Invalid parameter 'low/high': low must be less than high");
    expect_param([&] { vq::BinaryQuantizer(0, 10, 5); }, "low/high", "Invalid parameter 'low/high': low must be less than high");
    // valid ones construct without a device; getters (src/bq.rs test_getters)
    const vq::ScalarQuantizer sq(-1, 1, 256);
    EXPECT(sq.min() == -1.0f && sq.max() == 1.0f && sq.levels() == 256 && sq.step() == 2.0f / 255.0f);
    const vq::ScalarQuantizer sq_inf(-3e38f, 3e38f, 256);
    EXPECT(std::isinf(sq_inf.step()));
    const vq::BinaryQuantizer bq(0.5f, 10, 20);
    EXPECT(bq.threshold() == 0.5f && bq.low() == 10 && bq.high() == 20);
    // empty input: empty output, no device needed
    EXPECT(sq.quantize(std::vector<float>{}).empty() && bq.dequantize(std::vector<std::uint8_t>{}).empty());
    std::printf(failures ? "VALIDATE_FAILED\n" : "VALIDATE_OK\n");
    return failures ? 1 : 0;
}

static int run(const char *in_path, const char *out_path) {
    std::ifstream in(in_path, std::ios::binary);
    std::uint64_t n = 0;
    in.read(reinterpret_cast<char *>(&n), 8);
    std::vector<float> x(n);
    in.read(reinterpret_cast<char *>(x.data()), (std::streamsize)(n * 4));
    const vq::ScalarQuantizer sq(-1, 1, 256);
    const vq::BinaryQuantizer bq(0, 0, 1);
    const std::vector<std::uint8_t> sc = sq.quantize(x), bc = bq.quantize(x);
    const std::vector<float> sd = sq.dequantize(sc), bd = bq.dequantize(bc);
    std::ofstream out(out_path, std::ios::binary);
    out.write(reinterpret_cast<const char *>(sc.data()), (std::streamsize)n);
    out.write(reinterpret_cast<const char *>(sd.data()), (std::streamsize)(n * 4));
    out.write(reinterpret_cast<const char *>(bc.data()), (std::streamsize)n);
    out.write(reinterpret_cast<const char *>(bd.data()), (std::streamsize)(n * 4));
    std::printf("RUN_OK %s\n", vq::get_simd_backend().c_str());
    return 0;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    try {
        if (mode == "validate") return validate();
        if (mode == "run" && argc == 4) return run(argv[2], argv[3]);
    } catch (const std::exception &e) {
        std::printf("EXCEPTION %s\n", e.what());
        return 2;
    }
    std::printf("usage: test_sqbq_hpp validate | run <in> <out>\n");
    return 2;
}
