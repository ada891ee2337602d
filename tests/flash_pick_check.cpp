// Host-only check of csrc/flash_pick.h (built with g++ by tests/host_check.py; opens no device): flash_bf16_pick against the
// if-cascade launch_flash_attn_bf16 had before the selector existed, over the whole input space.
// Prints one "name -> ok ..." line per check and exits 1 at the first failure.
// With -DVLSAT_EXPERIMENTS the list has the lab rows as well, and the ablation values are enumerated too.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>

#include "flash_pick.h"

using namespace vlsat;

namespace {

struct int4 { int x, y, z, w; };
struct FlashSplit {                 // the fields of kernels.h's FlashSplit
    int parts = 1;
    const int4* krange = nullptr;
    float* o_part = nullptr; float* m_part = nullptr; float* l_part = nullptr;
    size_t part_stride = 0;
    int rows = 0, heads = 0;
    int ablate = 0;
    int qg = 0;
    int bq = 128;
};

struct Launched {                   // what the cascade did: one launch (template arguments, block size) or one error text
    bool launched = false;
    FlashVariant v{};
    int block = 0;
    const char* error = nullptr;
};

// ---- the frozen oracle: launch_flash_attn_bf16 of commit f5918ff, lines 596-678, word for word.  A "kernel" here returns its own
//      template arguments, a "launch" records them with the block size, fail() records the text. ----
template <int TERMS, bool TR, int IO, int PVT = 3, int FB_D = 64, int RING = 0, int BQW = 4, int ABL = 0, int QG = 1, int ORD = 0>
FlashVariant flash_attn_bf16_kernel() { return {TERMS, TR, IO, PVT, FB_D, RING, BQW, ABL, QG, ORD}; }
int dim3(int x) { return x; }
#define hipLaunchKernelGGL(kernel, grid, blk, ...) (out.launched = true, out.v = (kernel)(), out.block = blk)
#define fail(code, text) (out.error = text, code)

bool legacy_supports(int head_dim, int terms, int use_tr, int io_split) {
    if (head_dim == 64) return true;
    if (head_dim != 32 && head_dim != 128) return false;
    if (!use_tr || !io_split) return false;
    if (io_split >= 2 && terms != 1) return false;
    return head_dim == 32 || terms == 1;
}

int legacy_launch(Launched& out, int ldq, int ldkv, int ldo, int terms, int use_tr, int io_split, const FlashSplit* split, int pv_terms, int head_dim) {
    const int FB_D = head_dim;
    if (!legacy_supports(head_dim, terms, use_tr, io_split)) return fail(-1, "flash_attn_bf16: head dim / format combination not built");
    if ((ldq | ldkv | ldo) & 3) return fail(-1, "flash_attn: leading dims must be multiples of 4");
    if (terms != 1 && terms != 3) return fail(-1, "flash_attn_bf16: terms must be 1 or 3");
    if (io_split == 3 && !(split && split->rows > 0 && (size_t)split->rows * (size_t)ldkv * 4 < (1ull << 32)))
        return fail(-1, "flash_attn_bf16: fp16 half rows are built for scenes addressable with 32-bit offsets (the LDS-direct kernel)");
    FlashSplit sp{};
    if (split && split->parts > 1) {
        sp = *split;
        if (!sp.krange || !sp.o_part || !sp.m_part || !sp.l_part || sp.heads * FB_D > ldo)
            return fail(-1, "flash_attn: incomplete split-key workspace");
    }
    if (split) { sp.ablate = split->ablate; sp.bq = split->bq; sp.rows = split->rows; sp.qg = split->qg; }
    if (sp.bq != FLASH_BQ && !(sp.bq == FLASH_BQ_BIG && FB_D == 64 && io_split >= 2 && use_tr == 1 && sp.parts <= 1 && sp.rows > 0 &&
                               (size_t)sp.rows * (size_t)ldkv * 4 < (1ull << 32)))
        return fail(-1, "flash_attn_bf16: 256-query tiles are built for half rows, head dim 64, the LDS-direct kernel, no key split");
    if (io_split == 2 && use_tr && use_tr != 2 && !(split && split->rows > 0 && (size_t)split->rows * (size_t)ldkv * 4 < (1ull << 32))) use_tr = 2;
#define VLSAT_FA(T, R, S) hipLaunchKernelGGL((flash_attn_bf16_kernel<T, R, S>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp)
#define VLSAT_FAD(T, S, P, D) hipLaunchKernelGGL((flash_attn_bf16_kernel<T, true, S, P, D>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp)
    if (FB_D != 64) {          // 16 / 4 heads: the formats the forward uses (the transpose-read path; split-bf16 only at 32)
        if (io_split == 3) {                         // fp16 half rows
            if (use_tr == 2 || !use_tr || terms != 1) return fail(-1, "flash_attn_bf16: fp16 half rows are built for the LDS-direct single-rounding kernel only");
            if (FB_D == 32) hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 3, 3, 32, 2>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
            else hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 3, 3, 128, 2>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
        } else
        if (io_split == 2 && use_tr != 2) {          // half rows: LDS-direct K/V staging, one tile ahead
            if (FB_D == 32) hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 2, 3, 32, 2>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
            else hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 2, 3, 128, 2>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
        } else if (FB_D == 32) {
            if (io_split == 2) VLSAT_FAD(1, 2, 3, 32);
            else if (terms == 3 && pv_terms == 2) VLSAT_FAD(3, 1, 2, 32);
            else if (terms == 3) VLSAT_FAD(3, 1, 3, 32);
            else VLSAT_FAD(1, 1, 3, 32);
        } else {
            if (io_split == 2) VLSAT_FAD(1, 2, 3, 128); else VLSAT_FAD(1, 1, 3, 128);
        }
    } else
    if (io_split == 3) {                 // fp16 half rows (precision mode fp16_mixed): the two shipped forms of the LDS-direct kernel
        if (!use_tr || terms != 1 || use_tr == 2 || use_tr >= 3) return fail(-1, "flash_attn_bf16: fp16 half rows are built for the LDS-direct single-rounding kernel only");
        if (sp.bq == FLASH_BQ_BIG)
            hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 3, 3, 64, 2, 8>), dim3(n_tiles), dim3(512), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
        else
            hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 3, 3, 64, 2>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
    } else
    if (io_split == 2) {
        if (!use_tr || terms != 1) return fail(-1, "flash_attn_bf16: half-row tensors need terms = 1 and the transpose-read path");
        if (use_tr == 3)            // (experiments: vlsat_debug_option "flash_dma" 3 | 4 = rings of three / four buffers)
            hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 2, 3, 64, 3>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
        else if (use_tr == 4)
            hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 2, 3, 64, 4>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
#ifdef VLSAT_EXPERIMENTS
#define VLSAT_FA_ABL(A) else if (use_tr != 2 && sp.bq == FLASH_BQ_BIG && (sp.ablate & ~3) == (A)) \
            hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 2, 3, 64, 2, 8, A>), dim3(n_tiles), dim3(512), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
        VLSAT_FA_ABL(4) VLSAT_FA_ABL(8) VLSAT_FA_ABL(16) VLSAT_FA_ABL(28) VLSAT_FA_ABL(32) VLSAT_FA_ABL(64) VLSAT_FA_ABL(96) VLSAT_FA_ABL(256) VLSAT_FA_ABL(124) VLSAT_FA_ABL(380)
#undef VLSAT_FA_ABL
#endif
        else if (use_tr != 2 && sp.bq == FLASH_BQ_BIG && sp.qg == 1)
            hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 2, 3, 64, 2, 4, 0, 2, 0>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
        else if (use_tr != 2 && sp.bq == FLASH_BQ_BIG && sp.qg == 2)
            hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 2, 3, 64, 2, 4, 0, 2, 1>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
        else if (use_tr != 2 && sp.qg == 1 && sp.parts <= 1)
            hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 2, 3, 64, 2, 2, 0, 2, 0>), dim3(n_tiles), dim3(128), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
        else if (use_tr != 2 && sp.qg == 2 && sp.parts <= 1)
            hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 2, 3, 64, 2, 2, 0, 2, 1>), dim3(n_tiles), dim3(128), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
        else if (use_tr != 2 && sp.bq == FLASH_BQ_BIG)
            hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 2, 3, 64, 2, 8>), dim3(n_tiles), dim3(512), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
        else if (use_tr != 2)       // (use_tr = 2: the register-staged kernel of round 3, for A/B -- "flash_dma" 0)
            hipLaunchKernelGGL((flash_attn_bf16_kernel<1, true, 2, 3, 64, 2>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
        else
            VLSAT_FA(1, true, 2);
    } else if (io_split) {
        if (!use_tr) return fail(-1, "flash_attn_bf16: the split-pair format is built for the transpose-read path only");
        if (terms == 3 && pv_terms == 2)
            hipLaunchKernelGGL((flash_attn_bf16_kernel<3, true, 1, 2>), dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
        else if (terms == 3) VLSAT_FA(3, true, 1); else VLSAT_FA(1, true, 1);
    } else if (terms == 3) { if (use_tr) VLSAT_FA(3, true, 0); else VLSAT_FA(3, false, 0); }
    else                   { if (use_tr) VLSAT_FA(1, true, 0); else VLSAT_FA(1, false, 0); }
#undef VLSAT_FA
#undef VLSAT_FAD
    return 0;
}
#undef hipLaunchKernelGGL
#undef fail
// ---- end of the oracle ----

struct In { int d, terms, use_tr, io, pv, bq, qg, parts; bool fit; int ablate; };

// the cascade on a call that states `in`: leading dims of 1024 floats; rows that fit = 1000, rows that do not = 2^21 (8 GiB of K|V rows)
Launched legacy_pick(const In& in) {
    static const int4 kr{};
    static float ws;
    FlashSplit sp;
    sp.parts = in.parts; sp.krange = &kr; sp.o_part = sp.m_part = sp.l_part = &ws; sp.heads = 8;
    sp.rows = in.fit ? 1000 : 1 << 21; sp.ablate = in.ablate; sp.qg = in.qg; sp.bq = in.bq;
    Launched out;
    legacy_launch(out, 1024, 1024, 1024, in.terms, in.use_tr, in.io, &sp, in.pv, in.d);
    return out;
}

void die(const char* what, const In& in, const char* detail = "") {
    printf("%s -> FAILED at d %d terms %d use_tr %d io %d pv %d bq %d qg %d parts %d fit %d ablate %d %s\n", what, in.d, in.terms, in.use_tr, in.io,
           in.pv, in.bq, in.qg, in.parts, (int)in.fit, in.ablate, detail);
    exit(1);
}

}  // namespace

int main() {
#ifdef VLSAT_EXPERIMENTS
    const int ablates[] = {0, 4, 8, 16, 28, 32, 64, 96, 124, 256, 380, 5 /* 4 with bit 0 */, 12 /* no such kernel */};
#else
    const int ablates[] = {0};
#endif
    std::set<int> reached;
    int cases = 0, launches = 0, ring2_for_ring34 = 0;
    for (int d : {32, 48, 64, 128}) for (int terms : {1, 2, 3}) for (int use_tr = 0; use_tr <= 4; ++use_tr) for (int io = 0; io <= 3; ++io)
    for (int pv : {2, 3}) for (int bq : {128, 256}) for (int qg : {0, 1, 2}) for (int parts : {1, 2}) for (bool fit : {false, true})
    for (int ablate : ablates) {
        const In in{d, terms, use_tr, io, pv, bq, qg, parts, fit, ablate};
        Launched want = legacy_pick(in);
        // THE ONE PERMITTED DIFFERENCE: rings of 3 / 4 buffers are kernels of the experiments build.  The release selector answers
        // use_tr 3 | 4 (bf16 half rows, head dim 64) like use_tr 1, the LDS-direct kernel with its ring of 2, as the cascade
        // already did at head dims 32 / 128.
        if (!kFlashLab && want.launched && want.v.ring >= 3) {
            In as1 = in;
            as1.use_tr = 1;
            want = legacy_pick(as1);
            if (!want.launched || want.v.ring != 2) die("legacy", in, "(use_tr 1 is not a ring of 2)");
            ++ring2_for_ring34;
        }
        const FlashPick got = flash_bf16_pick(d, terms, use_tr, io, pv, bq, qg, parts, fit, ablate);
        ++cases;
        if (!want.launched) {
            if (got.index >= 0 || !got.error || strcmp(got.error, want.error)) die("legacy", in, got.error ? got.error : "(picked a kernel)");
            continue;
        }
        if (got.index < 0 || got.index >= kFlashVariantCount || got.error) die("legacy", in, got.error ? got.error : "(bad index)");
        const FlashVariant& v = kFlashVariants[got.index];
        if (!(v == want.v) || 64 * v.bqw != want.block) die("legacy", in, "(another kernel or block size)");
        reached.insert(got.index);
        ++launches;
    }
    printf("legacy -> ok %d cases, %d launches, %d ring-of-2 for ring-of-3/4\n", cases, launches, ring2_for_ring34);

    if ((int)reached.size() != kFlashVariantCount) { printf("reachable -> FAILED (%d of %d)\n", (int)reached.size(), kFlashVariantCount); return 1; }
    printf("reachable -> ok %d\n", kFlashVariantCount);

    // flash_attn_bf16_supports: the pick with the defaults; and over what the engine asks it (edge_attn_fmt: head dims other than 64,
    // terms 1 | 3, use_tr 0 | 1, split pairs | half rows) it answers what the hand-written rule answered
    for (int d : {32, 128}) for (int terms : {1, 2, 3}) for (int use_tr = 0; use_tr <= 4; ++use_tr) for (int io = 0; io <= 3; ++io) {
        const In in{d, terms, use_tr, io, 3, 128, 0, 1, true, 0};
        if (flash_attn_bf16_supports(d, terms, use_tr, io) != legacy_pick(in).launched) die("supports", in, "(not the pick with the defaults)");
    }
    for (int d : {32, 48, 128}) for (int terms : {1, 3}) for (int use_tr : {0, 1}) for (int io : {1, 2})
        if (flash_attn_bf16_supports(d, terms, use_tr, io) != legacy_supports(d, terms, use_tr, io)) die("supports", In{d, terms, use_tr, io, 3, 128, 0, 1, true, 0}, "(engine)");
    printf("supports -> ok\n");

    int release_rows = 0;
    for (int i = 0; i < kFlashVariantCount; ++i) {
        const FlashVariant& v = kFlashVariants[i];
        if (v.bqw != 2 && v.bqw != 4 && v.bqw != 8) { printf("block -> FAILED (row %d: %d waves)\n", i, v.bqw); return 1; }      // blocks of 128 | 256 | 512
        if (flash_bf16_find(v) != i) { printf("block -> FAILED (row %d is listed twice)\n", i); return 1; }
        release_rows += v.abl == 0 && v.ring <= 2;
    }
    printf("block -> ok %d rows, %d without ABL or a ring above 2\n", kFlashVariantCount, release_rows);
    return 0;
}
