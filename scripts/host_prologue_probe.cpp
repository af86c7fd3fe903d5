// Host prologue of local_laplacian without Python: every argument check up to the device acquisition, which fails (-29) on a box
// without a GPU.  g++ -O2 -std=c++17 -Iinclude scripts/host_prologue_probe.cpp -o /tmp/prologue -ldl -lpthread && /tmp/prologue halide_amd/lib/libhlmi.so
#include <chrono>
#include <cstdio>
#include <dlfcn.h>
#include <thread>
#include <vector>
#include <algorithm>
#include "hlmi_abi.h"
typedef int (*ll_t)(halide_buffer_t *, int32_t, float, float, halide_buffer_t *);
typedef void (*handler_t)(void *, const char *);
static void quiet(void *, const char *) {}
int main(int argc, char **argv) {
    void *h = dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL);
    if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
    ((handler_t (*)(handler_t))dlsym(h, "halide_set_error_handler"))(quiet);
    ll_t ll = (ll_t)dlsym(h, "local_laplacian");
    const int N = 200000;
    for (int nt : {1, 4}) {
        std::vector<double> best;
        for (int rep = 0; rep < 5; rep++) {
            auto t0 = std::chrono::steady_clock::now();
            std::vector<std::thread> th;
            for (int t = 0; t < nt; t++) th.emplace_back([&] {
                static thread_local uint16_t a[64 * 48 * 3], o[64 * 48 * 3];
                halide_dimension_t d[3] = {{0, 64, 1, 0}, {0, 48, 64, 0}, {0, 3, 64 * 48, 0}};
                halide_buffer_t in = {0, nullptr, (uint8_t *)a, 1, {1, 16, 0}, 3, d, nullptr}, out = {0, nullptr, (uint8_t *)o, 0, {1, 16, 0}, 3, d, nullptr};
                int r = 0;
                for (int i = 0; i < N; i++) r += ll(&in, 8, 0.14f, 1.0f, &out);
                if (r != -29 * N) fprintf(stderr, "unexpected %d\n", r / N);
            });
            for (auto &t : th) t.join();
            best.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / N * 1e9);
        }
        std::sort(best.begin(), best.end());
        printf("%d thread(s): %.0f ns per call (min of 5; max %.0f)\n", nt, best[0], best[4]);
    }
}
