// CPU test build only (tests/optim_cases.py build_driver): a program of its own around the optimizer's host code and the one-lane build of its
// kernels (csrc/optim.hpp), so that gaz_optim_* runs under -fsanitize=address,undefined with caller buffers that are exactly as large as the
// header says they must be — a library loaded into Python cannot.  It steps the size list of tests/optim_cases.py (tails of 1 .. 3, pads behind odd
// sizes, one chunk - 1 / exactly / + 1, three chunks + 5) under every combination of kind, orthograd, grokfast and decay, reads and writes whole
// arenas and ranges that end at the arena's last element, and uses the refusals.  Checked here: pads stay zero, the grads are zero after
// zero_grads, every result is finite, a second object given the same inputs gives the same bytes.
//   optim_asan       exit status 0 = every check held, 2 = anything else.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/gaz_engine.h"

static gaz_optim* h = nullptr;
static int fail(const char* what) { fprintf(stderr, "%s: %s\n", what, gaz_optim_last_error(h)); return 2; }
static unsigned rng = 12345u;
static float unit() { rng = rng * 1664525u + 1013904223u; return (float)((rng >> 8) & 0xFFFF) / 65536.0f - 0.5f; }

int main() {
    const int CH = 2048;
    const int64_t sizes_[] = {1, 3, 5, 7, 63, 65, 255, 257, CH - 1, CH + 1, 3 * CH + 5, 4, 64, 256, CH};
    const int T = (int)(sizeof(sizes_) / sizeof(sizes_[0]));
    int64_t* sizes = new int64_t[T];                                            // exactly n_tensors entries
    memcpy(sizes, sizes_, sizeof(sizes_));

    for (int combo = 0; combo < 16; ++combo) {
        gaz_optim_config c;
        memset(&c, 0, sizeof(c));
        c.struct_size = sizeof(c); c.n_tensors = T; c.sizes = sizes; c.kind = combo & 1; c.orthograd = (combo >> 1) & 1; c.grokfast = (combo >> 2) & 1;
        c.weight_decay = (combo >> 3) & 1 ? 0.004 : 0.0; c.beta_1 = 0.9; c.beta_2 = 0.999; c.epsilon = 1e-7; c.alpha = 0.99; c.lamb = 2.0;
        gaz_optim* pair[2] = {nullptr, nullptr};
        std::vector<float> result[2];
        for (int rep = 0; rep < 2; ++rep) {
            rng = 777u + (unsigned)combo;
            h = nullptr;
            if (gaz_optim_create(&c, &h)) return fail("create");
            pair[rep] = h;
            int64_t* offs = new int64_t[T];
            int64_t* info = new int64_t[5];
            if (gaz_optim_layout(h, offs, info)) return fail("layout");
            const int64_t total = info[0];
            if (info[2] != CH || info[3] != (c.orthograd ? 3 : 1) || info[4] != 1 || offs[0] != 0) { fprintf(stderr, "layout: info\n"); return 2; }
            for (int k = 0; k + 1 < T; ++k) if (offs[k + 1] != offs[k] + (sizes[k] + 3) / 4 * 4) { fprintf(stderr, "layout: offsets\n"); return 2; }
            if (total != offs[T - 1] + (sizes[T - 1] + 3) / 4 * 4) { fprintf(stderr, "layout: total\n"); return 2; }
            void* ptrs[5];
            if (gaz_optim_ptrs(h, &ptrs[0], &ptrs[1], &ptrs[2], &ptrs[3], &ptrs[4]) || !ptrs[0] || !ptrs[3] || (ptrs[4] != nullptr) != (c.grokfast != 0)) return fail("ptrs");
            float* w = new float[total];                                        // a whole arena, pads included: write zeroes them
            for (int64_t i = 0; i < total; ++i) w[i] = unit() * 0.2f;
            if (gaz_optim_write(h, 0, 0, total, w)) return fail("write params");
            const int64_t steps_t[] = {1, 2, 3, 1000};
            for (int s = 0; s < 4; ++s) {
                for (int k = 0; k < T; ++k) {                                   // a tensor at a time, buffers of exactly sizes[k] floats
                    float* g = new float[sizes[k]];
                    for (int64_t i = 0; i < sizes[k]; ++i) g[i] = unit();
                    if (gaz_optim_write(h, 1, offs[k], sizes[k], g)) return fail("write grads");
                    delete[] g;
                }
                if (gaz_optim_step(h, 2e-3, steps_t[s], s != 1)) return fail("step");
                double* norms = new double[(size_t)T * 4];
                if (gaz_optim_read_norms(h, norms)) return fail("read_norms");
                for (int i = 0; i < T * 4; ++i)                                 // (w.g has either sign; the other three are sums of squares)
                    if (!std::isfinite(norms[i]) || (!c.orthograd && norms[i] != 0.0) || (i % 4 != 0 && norms[i] < 0.0)) { fprintf(stderr, "norms[%d] = %g\n", i, norms[i]); return 2; }
                delete[] norms;
                for (int arena = 0; arena < (c.grokfast ? 5 : 4); ++arena) {
                    float* a = new float[total];
                    if (gaz_optim_read(h, arena, 0, total, a)) return fail("read");
                    for (int k = 0; k < T; ++k) {
                        for (int64_t i = 0; i < sizes[k]; ++i) {
                            const float x = a[offs[k] + i];
                            if (!std::isfinite(x) || (arena == 1 && s != 1 && x != 0.f)) { fprintf(stderr, "arena %d tensor %d element %lld = %g\n", arena, k, (long long)i, x); return 2; }
                        }
                        const int64_t end = k + 1 < T ? offs[k + 1] : total;
                        for (int64_t i = offs[k] + sizes[k]; i < end; ++i) if (a[i] != 0.f) { fprintf(stderr, "arena %d: a pad behind tensor %d is not zero\n", arena, k); return 2; }
                    }
                    if (s == 3 && arena == 0) result[rep].assign(a, a + total);
                    delete[] a;
                }
            }
            float* last = new float[3];                                         // a range that ends at the arena's last element
            if (gaz_optim_read(h, 3, total - 3, 3, last)) return fail("read the last elements");
            delete[] last;
            double ms = -1.0;
            if (gaz_optim_step_timed(h, 1e-3, 5, 1, 2, &ms) || ms < 0.0) return fail("step_timed");
            if (gaz_optim_synchronize(h)) return fail("synchronize");
            // the refusals at the limits
            float one = 0.f;
            if (gaz_optim_read(h, 0, total, 1, &one) == 0 || !strstr(gaz_optim_last_error(h), "of an arena of")) return fail("a read past the arena was accepted");
            if (gaz_optim_write(h, 0, total - 1, 2, &one) == 0) return fail("a write past the arena was accepted");
            if (gaz_optim_read(h, 5, 0, 1, &one) == 0 || !strstr(gaz_optim_last_error(h), "arena must be")) return fail("arena 5 was accepted");
            if (!c.grokfast && (gaz_optim_read(h, 4, 0, 1, &one) == 0 || !strstr(gaz_optim_last_error(h), "no ema arena"))) return fail("the missing ema arena was read");
            if (gaz_optim_step(h, 1e-3, 0, 1) == 0 || !strstr(gaz_optim_last_error(h), "t must be at least 1")) return fail("t = 0 was accepted");
            if (gaz_optim_step(h, NAN, 1, 1) == 0 || !strstr(gaz_optim_last_error(h), "lr must be finite")) return fail("lr = NaN was accepted");
            delete[] w; delete[] offs; delete[] info;
        }
        if (result[0].size() != result[1].size() || memcmp(result[0].data(), result[1].data(), result[0].size() * 4) != 0) { fprintf(stderr, "combo %d: two runs differ\n", combo); return 2; }
        gaz_optim_destroy(pair[0]); gaz_optim_destroy(pair[1]);
    }
    h = nullptr;
    // create's refusals
    gaz_optim_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c); c.n_tensors = T; c.sizes = sizes; c.kind = 1; c.beta_1 = 0.9; c.beta_2 = 0.999; c.epsilon = 1e-7;
    gaz_optim* o = nullptr;
    gaz_optim_config bad = c; bad.struct_size -= 8;
    if (gaz_optim_create(&bad, &o) == 0 || !strstr(gaz_optim_last_error(nullptr), "struct_size")) return fail("a stale struct_size was accepted");
    bad = c; bad.n_tensors = 0;
    if (gaz_optim_create(&bad, &o) == 0 || !strstr(gaz_optim_last_error(nullptr), "n_tensors must be at least 1")) return fail("n_tensors 0 was accepted");
    bad = c; bad.kind = 2;
    if (gaz_optim_create(&bad, &o) == 0 || !strstr(gaz_optim_last_error(nullptr), "kind must be 0")) return fail("kind 2 was accepted");
    bad = c; bad.beta_2 = 1.0;
    if (gaz_optim_create(&bad, &o) == 0 || !strstr(gaz_optim_last_error(nullptr), "beta_2 must be in [0, 1)")) return fail("beta_2 = 1 was accepted");
    sizes[T - 1] = 0;
    if (gaz_optim_create(&c, &o) == 0 || !strstr(gaz_optim_last_error(nullptr), "must be at least 1, not 0")) return fail("a size of 0 was accepted");
    delete[] sizes;
    printf("ok\n");
    return 0;
}
