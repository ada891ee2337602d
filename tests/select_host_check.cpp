// Host-only check of the integer helpers of csrc/select_core.h (built with g++ by tests/host_check.py; opens no device).
// Prints one "name -> ok" line per check and exits 1 at the first failure.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "select_core.h"

using namespace vlsat;

static void check(bool ok, const char* what, long long a = 0, long long b = 0) {
    if (ok) return;
    printf("%s -> FAILED (%lld, %lld)\n", what, a, b);
    exit(1);
}

// the formula proximity.hip and label_transfer.hip carried before they took fkey
static uint32_t old_f32_code(float x) {
    const uint32_t u = f32_bits(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

static void check_keys() {
    const float den = bits_f32(1u);                                    // the smallest denormal
    const float xs[] = {-INFINITY, -FLT_MAX, -1.0f, -FLT_MIN, -den, -0.0f, 0.0f, den, FLT_MIN, 1.0f, FLT_MAX, INFINITY};     // ascending
    const int n = (int)(sizeof xs / sizeof xs[0]);
    for (int i = 0; i < n; ++i) {
        const uint32_t k = fkey(xs[i]);
        check(f32_bits(unkey(k)) == f32_bits(xs[i]), "unkey(fkey(x)) bits", i);
        check(k > 0, "key > 0", i);
        check(k == old_f32_code(xs[i]), "fkey == old f32_code", i);
        if (i > 0) check(fkey(xs[i - 1]) < k, "fkey strictly monotone", i);
    }
    printf("keys -> ok\n");
}

static void check_count_ge() {
    const int lens[] = {0, 1, 2, 31, 32, 33};
    int cases = 0;
    for (int len : lens) {
        std::vector<uint32_t> p(len + 1, 0xDEADBEEFu);                  // (one entry past the list: never read)
        for (int i = 0; i < len; ++i) p[i] = 1000u - 10u * (uint32_t)(i / 3);      // descending, every value three times
        std::vector<uint32_t> ts = {0u, 1u, 0xFFFFFFFFu};
        for (int i = 0; i < len; ++i) {                                  // equal to, just above and just below every entry
            ts.push_back(p[i]);
            ts.push_back(p[i] + 1);
            ts.push_back(p[i] - 1);
            ts.push_back(p[i] - 5);                                      // between two values
        }
        for (uint32_t t : ts) {
            int want = 0;
            for (int i = 0; i < len; ++i) want += p[i] >= t;
            check(count_ge(p.data(), len, t) == want, "count_ge", len, t);
            ++cases;
        }
    }
    printf("count_ge -> ok %d\n", cases);
}

static void check_triples() {
    static constexpr TriTable<100, 32> tab = make_tri<100, 32>();
    check(tab.N == 1365, "1365 triples", tab.N);
    std::set<uint32_t> seen(tab.v, tab.v + tab.N);
    check((int)seen.size() == tab.N, "triples distinct", (long long)seen.size());
    int want = 0;
    for (int a = 1; a <= 100; ++a)
        for (int b = 1; b <= 100; ++b)
            for (int c = 1; c <= 32; ++c) {
                const bool in = a * b * c <= 100;
                want += in;
                check(seen.count((uint32_t)((a - 1) | ((b - 1) << 8) | ((c - 1) << 16))) == (in ? 1u : 0u), "triple present", a * 10000 + b * 100 + c);
            }
    check(want == tab.N, "no other triples", want);
    printf("triples -> ok %d\n", tab.N);
}

int main() {
    check_keys();
    check_count_ge();
    check_triples();
    check(clampi(-5, 0, 9) == 0 && clampi(12, 0, 9) == 9 && clampi(4, 0, 9) == 4 && clampi((int64_t)1 << 40, 0, 9) == 9, "clampi");
    printf("clampi -> ok\n");
    return 0;
}
