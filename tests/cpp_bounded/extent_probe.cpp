// extent_probe.cpp — the bounded decode's extent predicate
// (onc-rpc_amd/csrc/extent.h) at the extremes of its 64-bit arguments, on the
// CPU: compiled with the host compiler (and -fsanitize=undefined where the
// toolchain has it) and run by tests/test_bounded_host.py. The kernels call
// the same functions; extreme offsets are never handed to the GPU.
#include <cstdint>
#include <cstdio>

#include "extent.h"

static int g_fail = 0;
#define EXPECT(expr, want)                                                                        \
    do {                                                                                          \
        const uint32_t got_ = (expr);                                                             \
        if (got_ != uint32_t(want)) {                                                             \
            std::printf("FAIL line %d: %s = %u, want %u\n", __LINE__, #expr, got_, uint32_t(want)); \
            ++g_fail;                                                                             \
        }                                                                                         \
    } while (0)

int main() {
    using namespace onc;
    const uint64_t kMax = ~uint64_t(0);
    const uint64_t W = 1000;
    // inside, and the legal empty slice at the end
    EXPECT(extent_reason(0, 0, W), kExtentOk);
    EXPECT(extent_reason(0, W, W), kExtentOk);
    EXPECT(extent_reason(W - 1, 1, W), kExtentOk);
    EXPECT(extent_reason(W, 0, W), kExtentOk);
    // one byte too many, a start past the end (an empty record there too)
    EXPECT(extent_reason(W, 1, W), kExtentEnd);
    EXPECT(extent_reason(0, W + 1, W), kExtentEnd);
    EXPECT(extent_reason(W + 1, 0, W), kExtentStart);
    EXPECT(extent_reason(W + 1, 5, W), kExtentStart);
    // b + L wraps to 8: still a start past the wire
    EXPECT(extent_reason(kMax - 7, 16, uint64_t(1) << 40), kExtentStart);
    EXPECT(extent_reason(8, kMax - 3, uint64_t(1) << 40), kExtentEnd);
    EXPECT(extent_reason(kMax, kMax, kMax), kExtentEnd);
    EXPECT(extent_reason(kMax, 0, kMax), kExtentOk);
    EXPECT(extent_reason(0, kMax, kMax), kExtentOk);
    // an empty wire holds exactly the empty record at 0
    EXPECT(extent_reason(0, 0, 0), kExtentOk);
    EXPECT(extent_reason(0, 1, 0), kExtentEnd);
    EXPECT(extent_reason(1, 0, 0), kExtentStart);
    // offsets form: order first, then start, then end
    EXPECT(extent_reason_off(100, 50, W), kExtentOrder);
    EXPECT(extent_reason_off(W + 100, W + 50, W), kExtentOrder);
    EXPECT(extent_reason_off(100, 100, W), kExtentOk);
    EXPECT(extent_reason_off(W, W, W), kExtentOk);
    EXPECT(extent_reason_off(W - 1, W + 1, W), kExtentEnd);
    EXPECT(extent_reason_off(W + 1, W + 1, W), kExtentStart);
    EXPECT(extent_reason_off(W + 1, kMax, W), kExtentStart);
    EXPECT(extent_reason_off(kMax, 0, W), kExtentOrder);
    EXPECT(extent_reason_off(0, kMax, kMax), kExtentOk);
    EXPECT(extent_reason_off(0, 0, 0), kExtentOk);
    EXPECT(extent_reason_off(0, 1, 0), kExtentEnd);
    // lengths form: a prefix sum that wrapped came out below base
    EXPECT(extent_reason_len(7, 7, 10, W), kExtentOk);
    EXPECT(extent_reason_len(7, W, 0, W), kExtentOk);
    EXPECT(extent_reason_len(7, W, 1, W), kExtentEnd);
    EXPECT(extent_reason_len(7, W + 1, 0, W), kExtentStart);
    EXPECT(extent_reason_len(kMax - 7, 8, 16, uint64_t(1) << 40), kExtentStart);
    EXPECT(extent_reason_len(kMax - 7, 8, 0, kMax), kExtentStart);
    EXPECT(extent_reason_len(0, 0, 0, 0), kExtentOk);
    if (g_fail) return 1;
    std::printf("extent ok\n");
    return 0;
}
