// Host-only check of the evaluation-scratch layout of csrc/engine.h (EvalScratch, eval_scratch_carve, eval_scratch_floats / _ints; built
// with g++ by tests/host_check.py; opens no device).  Prints one "N E C R -> ok" line per case and exits 1 at the first failure.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define VLSAT_EVAL_SCRATCH_ONLY
#include "engine.h"

using namespace vlsat;

static void check(bool ok, const char* what, long long a = 0, long long b = 0) {
    if (ok) return;
    printf("%s -> FAILED (%lld, %lld)\n", what, a, b);
    exit(1);
}

// regions in the order they must lie in; each starts where the one before it ends, the last ends at or before `total`
template <class T>
struct Region { const char* name; T* p; size_t n; };

template <class T, size_t K>
static void check_regions(const Region<T> (&r)[K], T* base, size_t total) {
    T* at = base;
    for (size_t k = 0; k < K; ++k) {
        check(r[k].p == at, r[k].name, (long long)(r[k].p - base), (long long)(at - base));     // in order, disjoint, no gap
        for (size_t j = 0; j < r[k].n; ++j) r[k].p[j] = (T)k;                                   // (out of bounds: the sanitizer's)
        at += r[k].n;
    }
    check((size_t)(at - base) <= total, "end <= size", (long long)(at - base), (long long)total);
    at = base;
    for (size_t k = 0; k < K; ++k)
        for (size_t j = 0; j < r[k].n; ++j) check(*at++ == (T)k, "region overwritten by a later one", (long long)k, (long long)j);
}

static void check_case(size_t N, size_t E, size_t C, size_t R) {
    const size_t Es = E > 0 ? E : 1;                     // plan_graph.h: Ns = N, Es = max(E, 1)
    const size_t nf = eval_scratch_floats(N, E, C, R), ni = eval_scratch_ints(N, E, R);
    check(nf == 4 * N * C + 2 * Es * R + N * C, "floats", (long long)nf);
    check(ni == 2 * N + 4 * Es * R + 2 * Es, "ints", (long long)ni);
    std::vector<float> f(nf);
    std::vector<int32_t> i(ni);
    const EvalScratch v = eval_scratch_carve(f.data(), i.data(), N, E, C, R);
    const Region<float> rf[] = {{"obj3", v.obj3, N * C}, {"obj2", v.obj2, N * C}, {"prob3", v.prob3, N * C}, {"prob2", v.prob2, N * C},
                                {"rel3", v.rel3, Es * R}, {"rel2", v.rel2, Es * R}, {"sorted", v.sorted, N * C}};
    const Region<int32_t> ri[] = {{"or3", v.or3, N}, {"or2", v.or2, N}, {"rr3", v.rr3, Es * R}, {"rr2", v.rr2, Es * R},
                                  {"tr3", v.tr3, Es * R}, {"tr2", v.tr2, Es * R}, {"cn3", v.cn3, Es}, {"cn2", v.cn2, Es}};
    check_regions(rf, f.data(), nf);
    check_regions(ri, i.data(), ni);
    printf("%zu %zu %zu %zu -> ok\n", N, E, C, R);
}

int main() {
    check_case(1, 0, 160, 26);
    check_case(2, 2, 160, 26);
    check_case(64, 4032, 160, 26);
    check_case(3, 6, 20, 8);
    return 0;
}
