// noise_ar1_ab.hip -- which lane width and block depth should ppo_noise_ar1 run at?  The kernel of csrc/noise_ar1.hip itself
// (this file includes it), instantiated at 16-, 8- and 4-byte lanes and at 4, 8 and 16 steps per block of loads, on the noise buffer
// of a rollout: T x C floats filtered in place.  The yardstick is one device copy of the same bytes between two buffers (T x C
// floats read, T x C written).  All forms and the copy alternate in one process; every form runs on the same buffer, which a
// second buffer of the same size separates from its previous pass (2 x 47 MB at 8192 envs: nothing is read back from L2).
// Also: the reference's 16-env shape (T = 40 960, C = 288), where the launch is one dependent chain of T steps on two waves.
// Prints one line per form: median / min / max microseconds over the rounds, and bytes moved per second at the median.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -I include -I fly_bproject_amd/csrc -o noise_ar1_ab tools/noise_ar1_ab.hip
//   ./noise_ar1_ab [N envs (8192)] [rounds (30)]
#include "../fly_bproject_amd/csrc/noise_ar1.hip"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                                     \
    do {                                                                                             \
        hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) {                                                                      \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));               \
            exit(1);                                                                                 \
        }                                                                                            \
    } while (0)

namespace {

struct Form {
    const char* name;
    hipError_t (*run)(float* eps, float* carry, long T, long C, float* other);
    std::vector<float> us;
};

template <int W, int U>
hipError_t run_form(float* eps, float* carry, long T, long C, float*)
{
    const long lanes = C / W;
    return launch_kernel<noise_ar1_kernel<W, U>>(dim3((unsigned)((lanes + AR1_BLOCK - 1) / AR1_BLOCK)), AR1_BLOCK, 0, nullptr, eps,
                                                 carry, T, C, 0.5f, 0.8660254f);
}

hipError_t run_copy(float* eps, float*, long T, long C, float* other)
{
    return hipMemcpyAsync(other, eps, (size_t)T * C * sizeof(float), hipMemcpyDeviceToDevice, nullptr);
}

hipError_t run_entry(float* eps, float* carry, long T, long C, float*)      // what the library launches
{
    return flyhip_launch_noise_ar1(eps, carry, T, C, 0.5f, nullptr);
}

void measure(const char* title, long T, long C, int rounds, std::vector<Form> forms)
{
    const size_t n = (size_t)T * C;
    float *eps, *other, *carry;
    CHECK(hipMalloc(&eps, n * sizeof(float)));
    CHECK(hipMalloc(&other, n * sizeof(float)));
    CHECK(hipMalloc(&carry, C * sizeof(float)));
    std::vector<float> host(n);
    unsigned x = 12345u;
    for (size_t i = 0; i < n; ++i) {                        // finite values of either sign (the timing does not depend on them)
        x = x * 1664525u + 1013904223u;
        host[i] = (float)(int)(x >> 8) * (1.0f / 8388608.0f) - 1.0f;
    }
    CHECK(hipMemcpy(eps, host.data(), n * sizeof(float), hipMemcpyHostToDevice));
    CHECK(hipMemset(other, 0, n * sizeof(float)));
    CHECK(hipMemset(carry, 0, C * sizeof(float)));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    for (int r = 0; r < rounds + 2; ++r) {                  // the first two rounds are the warm-up
        for (size_t f = 0; f < forms.size(); ++f) {
            Form& fm = forms[(f + r) % forms.size()];       // the order rotates from round to round
            CHECK(hipMemsetAsync(other, 0, n * sizeof(float), nullptr));    // the form's buffer leaves the caches
            CHECK(hipEventRecord(a, nullptr));
            CHECK(fm.run(eps, carry, T, C, other));
            CHECK(hipEventRecord(b, nullptr));
            CHECK(hipEventSynchronize(b));
            float ms = 0.0f;
            CHECK(hipEventElapsedTime(&ms, a, b));
            if (r >= 2) fm.us.push_back(1e3f * ms);
        }
    }
    printf("%s: T = %ld, C = %ld, %.1f MB read + %.1f MB written per launch, %d rounds\n", title, T, C, n * 4e-6, n * 4e-6, rounds);
    for (Form& fm : forms) {
        std::sort(fm.us.begin(), fm.us.end());
        const float med = fm.us[fm.us.size() / 2];
        printf("  %-28s median %9.2f us  min %9.2f  max %9.2f   %7.1f GB/s read + write\n", fm.name, med, fm.us.front(), fm.us.back(),
               2.0 * n * 4.0 / (med * 1e3));
    }
    fflush(stdout);
    CHECK(hipFree(eps));
    CHECK(hipFree(other));
    CHECK(hipFree(carry));
}

}  // namespace

int main(int argc, char** argv)
{
    const long N = argc > 1 ? atol(argv[1]) : 8192;
    const int rounds = argc > 2 ? atoi(argv[2]) : 30;
    if (N < 1 || N > 40960 || rounds < 1) {
        fprintf(stderr, "usage: noise_ar1_ab [N envs, 1..40960 (8192)] [rounds (30)]\n");
        return 2;
    }
    const long T = 16 * (40960 / N), C = 18 * N;            // ppo.py:118-122: rollout_size = 16 * (40960 // N)
    std::vector<Form> wide = {{"device copy, same bytes", run_copy, {}},
                              {"ppo_noise_ar1 (as launched)", run_entry, {}},
                              {"16-byte lanes, 8 steps", run_form<4, 8>, {}},
                              {"16-byte lanes, 4 steps", run_form<4, 4>, {}},
                              {"16-byte lanes, 16 steps", run_form<4, 16>, {}},
                              {"8-byte lanes, 8 steps", run_form<2, 8>, {}},
                              {"8-byte lanes, 16 steps", run_form<2, 16>, {}},
                              {"4-byte lanes, 8 steps", run_form<1, 8>, {}},
                              {"4-byte lanes, 16 steps", run_form<1, 16>, {}}};
    if (C % 4) wide.erase(wide.begin() + 2, wide.begin() + 5);
    measure("rollout noise buffer", T, C, rounds, wide);
    // the reference's own configuration: 16 envs, one chain of 40 960 dependent steps on ceil(288 / 4 / 64) = 2 waves
    std::vector<Form> chain = {{"device copy, same bytes", run_copy, {}},
                               {"ppo_noise_ar1 (as launched)", run_entry, {}},
                               {"16-byte lanes, 8 steps", run_form<4, 8>, {}},
                               {"16-byte lanes, 16 steps", run_form<4, 16>, {}},
                               {"4-byte lanes, 8 steps", run_form<1, 8>, {}},
                               {"4-byte lanes, 16 steps", run_form<1, 16>, {}}};
    measure("16-env shape", 16 * (40960 / 16), 18 * 16, rounds < 10 ? rounds : 10, chain);
    return 0;
}
