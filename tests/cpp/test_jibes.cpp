// C++ host-mirror test of the JIBES tag caller (include/crgpu.hpp): the latent states and the prior on the host (the 970 states of
// 16 tags, the -inf priors of a limited model with k <= 3), the expected-cells root, and a small two-tag fit on the device: the
// refusals, n == 0, a seeded well whose two runs agree bit for bit and whose calls are the planted ones.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_jibes.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_jibes_cpp.py)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crgpu.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                      \
        }                                                                  \
    } while (0)

static void test_host_functions() {
    const double est = crgpu::jibes_expected_cells(400, 2000);
    CHECK(est > 400.0 && est < 600.0);
    double c = 0.0;  // it is the root: the expected barcodes of est cells are 400 again
    CHECK(crgpu_jibes_expected_cells(400, 2000, &c) == CRGPU_OK && c == est);
    bool raised = false;
    try {
        crgpu::jibes_expected_cells(70000, 95000);
    } catch (const crgpu::Error &e) {
        raised = e.code == CRGPU_JIBES_CANT_CONVERGE;
    }
    CHECK(raised);
    const auto l3 = crgpu::jibes_latent_states(400, 3, 2000, est);
    CHECK(l3.setup.n_states == 21 && l3.setup.k_let_limited == 1 && l3.setup.max_multiplets == 3 && l3.setup.max_modeled_k_let == 3);
    CHECK(l3.states[0] == 0 && l3.states[1] == 0 && l3.states[2] == 0);                    // the blank state first
    CHECK(l3.states[3] == 0 && l3.states[4] == 0 && l3.states[5] == 1);                    // then [0, 0, 1]: generate_solutions order
    CHECK(l3.states[20 * 3] == 1 && l3.states[20 * 3 + 1] == 1 && l3.states[20 * 3 + 2] == 1);  // the unit vector appended
    int ninf = 0;
    for (double p : l3.prior) ninf += std::isinf(p) && p < 0;
    CHECK(ninf == 11 && l3.prior[0] == std::log(0.04));  // the quirk: the 3-lets (and the unit vector) of a limited model with k <= 3
    CHECK(crgpu::jibes_latent_states(130, 16, 300, crgpu::jibes_expected_cells(130, 300)).setup.n_states == CRGPU_JIBES_MAX_STATES);
    CHECK(crgpu::jibes_latent_states(1000, 12, 4000, crgpu::jibes_expected_cells(1000, 4000)).setup.n_states == 456);
    bool range = false;
    try {
        crgpu::jibes_latent_states(100, 17, 2000, 100.0);
    } catch (const crgpu::Error &e) {
        range = e.code == CRGPU_ERANGE;
    }
    CHECK(range);
}

static void test_fit() {
    crgpu::Context ctx(0);
    // 90 barcodes: 40 carry tag 0, 40 tag 1, 10 both; log10 counts 1.0 (background) / 2.5 (foreground) with a small seeded jitter
    const uint32_t n = 90, k = 2;
    std::vector<double> y(n * k);
    uint64_t s = 12345;
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t t = 0; t < k; t++) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            const double jitter = ((double)(s >> 40) / (double)(1 << 24) - 0.5) * 0.2;
            const bool on = i < 40 ? t == 0 : i < 80 ? t == 1 : true;
            y[i * k + t] = (on ? 2.5 : 1.0) + jitter;
        }
    const double est = crgpu::jibes_expected_cells(n, 2000);
    const std::vector<double> bg = {1.2, 1.2}, fg = {1.0, 1.0}, sd = {0.4, 0.4};
    const auto a = crgpu::jibes_fit(ctx, y, k, bg, fg, sd, 2000, est, 0.1);
    const auto b = crgpu::jibes_fit(ctx, y, k, bg, fg, sd, 2000, est, 0.1);
    CHECK(a.result.converged == 1 && a.result.iterations >= 2 && a.result.n_states == 6 && a.result.k_let_limited == 0);
    CHECK(std::memcmp(&a.result, &b.result, offsetof(crgpu_jibes_fit_result, fit_ms)) == 0 && a.result.iterations == b.result.iterations);
    CHECK(a.probs == b.probs && a.assignment == b.assignment && a.assignment_prob == b.assignment_prob && a.ml_state == b.ml_state);
    CHECK(std::fabs(a.result.bg[0] - 1.0) < 0.05 && std::fabs(a.result.fg[0] - 1.5) < 0.05 && a.result.sd[0] < 0.1);
    uint32_t right = 0;
    for (uint32_t i = 0; i < n; i++) {
        const int32_t want = i < 40 ? 0 : i < 80 ? 1 : 2;  // k = Multiplet
        right += a.assignment[i] == want;
        double sum = 0.0;
        for (uint32_t c2 = 0; c2 < k + 2; c2++) sum += a.probs[i * (k + 2) + c2];
        CHECK(std::fabs(sum - 1.0) < 1e-12);
        if (want == 2) CHECK(a.ml_state[i] == 4);  // states: blank, 01, 10, 02, 11, 20
    }
    CHECK(right == n);
    // refusals and the empty input
    int code = 0;
    try {
        crgpu::jibes_fit(ctx, y, k, bg, {1.0, 0.009}, sd, 2000, est);
    } catch (const crgpu::Error &e) {
        code = e.code;
    }
    CHECK(code == CRGPU_EINVAL);
    code = 0;
    try {
        crgpu::jibes_fit(ctx, std::vector<double>(17 * 3, 1.0), 17, std::vector<double>(17, 1.0), std::vector<double>(17, 1.0), std::vector<double>(17, 0.3), 2000, 3.0);
    } catch (const crgpu::Error &e) {
        code = e.code;
    }
    CHECK(code == CRGPU_ERANGE);
    const auto e0 = crgpu::jibes_fit(ctx, {}, k, bg, fg, sd, 2000, 0.0);
    CHECK(e0.result.ll == 0.0 && e0.result.converged == 1 && e0.result.iterations == 0 && e0.result.fg[0] == 0.0 && e0.result.bg[0] == 1.2);
}

int main(int argc, char **argv) {
    test_host_functions();
    if (argc < 2 || std::strcmp(argv[1], "--host-only") != 0) test_fit();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("all tests passed\n");
    return 0;
}
