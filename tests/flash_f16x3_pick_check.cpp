// Host-only check of the split-fp16 part of csrc/flash_pick.h (built with g++ by tests/host_check.py; opens no device):
// flash_f16x3_pick over its whole input space.  The form exists for fp32 tensors at head dim 64 with 128-query tiles, 32 queries per
// wave and no timing ablation, with the transpose read on or off; every such call must name the row of kFlashF16x3Variants with that
// (tr, d), every other call must be an error with a text and never another kernel, and every row must be reached.
// Prints one "name -> ok ..." line per check and exits 1 at the first failure.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>

#include "flash_pick.h"

using namespace vlsat;

namespace {

struct In { int d, use_tr, io, bq, qg, ablate; };

void die(const char* what, const In& in, const char* detail = "") {
    printf("%s -> FAILED at d %d use_tr %d io %d bq %d qg %d ablate %d %s\n", what, in.d, in.use_tr, in.io, in.bq, in.qg, in.ablate, detail);
    exit(1);
}

}  // namespace

int main() {
    std::set<int> reached;
    int cases = 0, launches = 0, errors = 0;
    for (int d : {0, 32, 48, 64, 128}) for (int use_tr = -1; use_tr <= 4; ++use_tr) for (int io = 0; io <= 3; ++io)
    for (int bq : {64, 128, 256}) for (int qg : {0, 1, 2}) for (int ablate : {0, 1, 4, 64}) {
        const In in{d, use_tr, io, bq, qg, ablate};
        const bool listed = d == 64 && (use_tr == 0 || use_tr == 1) && io == 0 && bq == FLASH_BQ && qg == 0 && ablate == 0;
        const FlashPick got = flash_f16x3_pick(d, use_tr, io, bq, qg, ablate);
        ++cases;
        if (!listed) {
            if (got.index != -1) die("unlisted", in, "(picked a kernel)");
            if (!got.error || !strlen(got.error) || strncmp(got.error, "flash_attn_f16x3: ", 18)) die("unlisted", in, "(no error text)");
            ++errors;
            continue;
        }
        if (got.index < 0 || got.index >= kFlashF16x3VariantCount || got.error) die("listed", in, got.error ? got.error : "(bad index)");
        const FlashF16x3Variant& v = kFlashF16x3Variants[got.index];
        if (v.tr != (use_tr == 1) || v.d != d) die("listed", in, "(another kernel)");
        reached.insert(got.index);
        ++launches;
    }
    printf("listed -> ok %d cases, %d launches\n", cases, launches);
    printf("unlisted -> ok %d errors\n", errors);

    if ((int)reached.size() != kFlashF16x3VariantCount) { printf("reachable -> FAILED (%d of %d)\n", (int)reached.size(), kFlashF16x3VariantCount); return 1; }
    printf("reachable -> ok %d\n", kFlashF16x3VariantCount);

    // the defaults are the engine's call: fp32 tensors, 128-query tiles, 32 queries per wave
    for (int d : {32, 48, 64, 128}) for (int use_tr : {0, 1})
        if (flash_f16x3_supports(d, use_tr) != (flash_f16x3_pick(d, use_tr).index >= 0) || flash_f16x3_supports(d, use_tr) != (d == 64))
            die("supports", In{d, use_tr, 0, FLASH_BQ, 0, 0});
    printf("supports -> ok\n");

    for (int i = 0; i < kFlashF16x3VariantCount; ++i)
        for (int j = 0; j < i; ++j)
            if (kFlashF16x3Variants[i] == kFlashF16x3Variants[j]) { printf("rows -> FAILED (row %d is listed twice)\n", i); return 1; }
    printf("rows -> ok %d\n", kFlashF16x3VariantCount);
    return 0;
}
