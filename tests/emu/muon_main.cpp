// CPU test build only (tests/muon_cases.py build_driver): a program of its own around the optimizer's host code and the one-lane build of the Muon
// kernels (csrc/muon.hpp), so that gaz_muon_* runs under -fsanitize=address,undefined with caller buffers that are exactly as large as the header
// says they must be — a library loaded into Python cannot.  It steps the tensor list of tests/muon_cases.py (Adam and Muon tensors interleaved
// behind pads; general matrices with partial tiles in both orientations; thin ones of 1, 3 and 4 rows, three chunks of columns with a tail, the
// N x 1 Dense) under six combinations of the switches, reads every debug buffer into a buffer of exactly its size, and uses the refusals.  Checked
// here: pads stay zero, every result is finite, X0 and X are bf16 values, A and B are symmetric, a second object given the same inputs gives
// the same bytes.
//   muon_asan       exit status 0 = every check held, 2 = anything else.
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
static bool is_bf16(float x) { unsigned u; memcpy(&u, &x, 4); return (u & 0xFFFFu) == 0; }

int main() {
    const int T = 16;
    const int rows_[T] = {0, 5, 1, 0, 3, 17, 65, 0, 16, 64, 33, 70, 3, 130, 4, 0};
    const int cols_[T] = {0, 7, 18, 0, 18, 33, 33, 0, 48, 64, 130, 257, 6147, 1, 9, 0};
    const int64_t adam_sizes[T] = {7, 0, 0, 3, 0, 0, 0, 30, 0, 0, 0, 0, 0, 0, 0, 33};
    int64_t* sizes = new int64_t[T];
    int32_t* rows = new int32_t[T];
    int32_t* cols = new int32_t[T];
    float* scale = new float[T];
    for (int k = 0; k < T; ++k) { rows[k] = rows_[k]; cols[k] = cols_[k]; sizes[k] = rows_[k] ? (int64_t)rows_[k] * cols_[k] : adam_sizes[k]; scale[k] = 0.2f + 0.01f * k; }

    for (int combo = 0; combo < 6; ++combo) {
        gaz_optim_config c;
        memset(&c, 0, sizeof(c));
        c.struct_size = sizeof(c); c.n_tensors = T; c.sizes = sizes; c.kind = combo & 1; c.orthograd = combo % 3 == 0; c.grokfast = combo % 2 == 0;
        c.weight_decay = combo < 3 ? 0.004 : 0.0; c.beta_1 = 0.9; c.beta_2 = 0.995; c.epsilon = 1e-8; c.alpha = 0.99; c.lamb = 2.0;
        gaz_muon_config m;
        memset(&m, 0, sizeof(m));
        m.struct_size = sizeof(m); m.n_tensors = T; m.rows = rows; m.cols = cols; m.scale = scale; m.muon_beta = 0.95; m.nesterov = combo & 1;
        m.ns_steps = combo < 2 ? 5 : combo < 4 ? 1 : 0; m.muon_a = 3.4445; m.muon_b = -4.775; m.muon_c = 2.0315; m.adam_lr_ratio = combo & 1 ? 0.5 : 1.0;
        gaz_optim* pair[2] = {nullptr, nullptr};
        std::vector<float> result[2];
        for (int rep = 0; rep < 2; ++rep) {
            rng = 999u + (unsigned)combo;
            h = nullptr;
            if (gaz_optim_create(&c, &h)) return fail("create");
            pair[rep] = h;
            if (gaz_muon_set(h, &m)) return fail("muon_set");
            if (gaz_muon_set(h, &m) == 0 || !strstr(gaz_optim_last_error(h), "in Muon mode already")) return fail("a second muon_set was accepted");
            int64_t* offs = new int64_t[T];
            int64_t* info = new int64_t[5];
            if (gaz_optim_layout(h, offs, info)) return fail("layout");
            const int64_t total = info[0];
            if (info[3] != (c.orthograd ? 3 : 1) + 2 + 3 * m.ns_steps || info[4] != 1) { fprintf(stderr, "layout: launches %lld\n", (long long)info[3]); return 2; }
            float* w = new float[total];
            for (int64_t i = 0; i < total; ++i) w[i] = unit() * 0.2f;
            if (gaz_optim_write(h, 0, 0, total, w)) return fail("write params");
            const int64_t steps_t[] = {1, 2, 1000};
            for (int s = 0; s < 3; ++s) {
                for (int k = 0; k < T; ++k) {
                    float* g = new float[sizes[k]];
                    for (int64_t i = 0; i < sizes[k]; ++i) g[i] = unit();
                    if (gaz_optim_write(h, 1, offs[k], sizes[k], g)) return fail("write grads");
                    delete[] g;
                }
                if (gaz_optim_step(h, 2e-3, steps_t[s], s != 1)) return fail("step");
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
                    if (s == 2 && arena == 0) result[rep].assign(a, a + total);
                    delete[] a;
                }
                for (int k = 0; k < T; ++k) {
                    if (!rows[k]) continue;
                    const int P = rows[k] < cols[k] ? rows[k] : cols[k];
                    for (int what = 0; what < 5; ++what) {                       // buffers of exactly the documented sizes
                        const int64_t n = what == 1 ? 1 : what == 0 || what == 2 ? sizes[k] : (int64_t)P * P;
                        float* b = new float[n];
                        if (gaz_muon_read(h, k, what, b)) return fail("muon_read");
                        for (int64_t i = 0; i < n; ++i)
                            if (!std::isfinite(b[i]) || (what != 1 && !is_bf16(b[i]))) { fprintf(stderr, "tensor %d what %d element %lld = %g\n", k, what, (long long)i, b[i]); return 2; }
                        if (what == 1 && !(b[0] > 0.f)) { fprintf(stderr, "tensor %d: n = %g\n", k, b[0]); return 2; }
                        if (what >= 3)
                            for (int i = 0; i < P; ++i) for (int j = 0; j < P; ++j)
                                if (b[i * P + j] != b[j * P + i] || (m.ns_steps == 0 && b[i * P + j] != 0.f)) { fprintf(stderr, "tensor %d what %d is not symmetric\n", k, what); return 2; }
                        delete[] b;
                    }
                }
            }
            double ms = -1.0;
            if (gaz_optim_step_timed(h, 1e-3, 5, 1, 2, &ms) || ms < 0.0) return fail("step_timed");
            float one = 0.f;
            if (gaz_muon_read(h, 0, 0, &one) == 0 || !strstr(gaz_optim_last_error(h), "is an Adam tensor")) return fail("muon_read of an Adam tensor was accepted");
            if (gaz_muon_read(h, T, 0, &one) == 0 || gaz_muon_read(h, -1, 0, &one) == 0) return fail("muon_read of tensor T was accepted");
            if (gaz_muon_read(h, 1, 5, &one) == 0 || !strstr(gaz_optim_last_error(h), "what must be")) return fail("what = 5 was accepted");
            delete[] w; delete[] offs; delete[] info;
        }
        if (result[0].size() != result[1].size() || memcmp(result[0].data(), result[1].data(), result[0].size() * 4) != 0) { fprintf(stderr, "combo %d: two runs differ\n", combo); return 2; }
        gaz_optim_destroy(pair[0]); gaz_optim_destroy(pair[1]);
    }
    // muon_set's refusals
    gaz_optim_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c); c.n_tensors = T; c.sizes = sizes; c.kind = 1; c.beta_1 = 0.9; c.beta_2 = 0.995; c.epsilon = 1e-8;
    h = nullptr;
    if (gaz_optim_create(&c, &h)) return fail("create");
    gaz_muon_config m;
    memset(&m, 0, sizeof(m));
    m.struct_size = sizeof(m); m.n_tensors = T; m.rows = rows; m.cols = cols; m.scale = scale; m.muon_beta = 0.95; m.nesterov = 1; m.ns_steps = 5; m.muon_a = 3.4445; m.muon_b = -4.775;
    m.muon_c = 2.0315; m.adam_lr_ratio = 1.0;
    float one = 0.f;
    if (gaz_muon_read(h, 1, 0, &one) == 0 || !strstr(gaz_optim_last_error(h), "not in Muon mode")) return fail("muon_read without Muon was accepted");
    gaz_muon_config bad = m; bad.struct_size -= 8;
    if (gaz_muon_set(h, &bad) == 0 || !strstr(gaz_optim_last_error(h), "struct_size")) return fail("a stale struct_size was accepted");
    bad = m; bad.ns_steps = 17;
    if (gaz_muon_set(h, &bad) == 0 || !strstr(gaz_optim_last_error(h), "ns_steps must be in 0 .. 16")) return fail("ns_steps 17 was accepted");
    bad = m; bad.muon_c = NAN;
    if (gaz_muon_set(h, &bad) == 0 || !strstr(gaz_optim_last_error(h), "must be finite")) return fail("muon_c = NaN was accepted");
    bad = m; bad.muon_beta = 1.0;
    if (gaz_muon_set(h, &bad) == 0 || !strstr(gaz_optim_last_error(h), "muon_beta must be in [0, 1)")) return fail("muon_beta = 1 was accepted");
    bad = m; bad.n_tensors = T - 1;
    if (gaz_muon_set(h, &bad) == 0 || !strstr(gaz_optim_last_error(h), "n_tensors is")) return fail("n_tensors T - 1 was accepted");
    cols[5] = 34;
    if (gaz_muon_set(h, &m) == 0 || !strstr(gaz_optim_last_error(h), "is not its size")) return fail("rows * cols != size was accepted");
    cols[5] = 33;
    if (gaz_optim_step(h, 1e-3, 1, 1)) return fail("step");
    if (gaz_muon_set(h, &m) == 0 || !strstr(gaz_optim_last_error(h), "before the first step")) return fail("muon_set after a step was accepted");
    gaz_optim_destroy(h);
    delete[] sizes; delete[] rows; delete[] cols; delete[] scale;
    printf("ok\n");
    return 0;
}
