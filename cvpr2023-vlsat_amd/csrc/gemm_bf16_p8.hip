// bf16 GEMM of the single-rounding modes for the large edge-row launches (BASELINE configs[2]) -- same contract as
// gemm_f32.hip / gemm_bf16_ring.hip,
//     C[M,N] = act((A[M,K] . W[N,K]^T) + bias + resid_scale*resid + g0[gi0] + g1[gi1]) * c_scale,
// for A stored as HALF ROWS (bf16 at byte 2 k of an fp32-pitched row) and one bf16 weight plane.  Every nn.Linear on edge
// rows goes through it in the bf16_mixed / bf16 modes (reference network_MMG.py:59-79,93-98; attention.py:54-58,77;
// network_PointNet.py:328-341).
//
// Structure (cdna_hip_programming.md "The 256^2 8-phase template", rebuilt for this library's operand formats):
//   * ONE persistent block of 8 waves per CU, block tile 256 x 256, waves 2 (M) x 4 (N), wave tile 128 x 64 =
//     4 x 2 tiles of v_mfma_f32_32x32x16_bf16 (transposed product: a lane owns one output ROW, gemm_core.h).
//   * K in tiles of 64; LDS holds two K-tiles (2 x 64 KB), each as four HALF-TILES of 128 rows x 128 bytes:
//       A_h = rows {wr*128 + h*64 + i} of the block's A panel,  W_h = rows {wc*64 + h*32 + j} of its weight panel,
//     i.e. half-tile h is what quadrant h of EVERY wave reads.  Rows are 128 bytes, 16-byte chunks XOR-swizzled with
//     (row >> 1) & 7 on the global side of the LDS-direct loads and on the fragment reads (0 bank conflicts in the K loop;
//     the epilogue's transposition buffer has its own swizzle, see epi_t).
//   * A K-tile is FOUR PHASES, one per quadrant of the wave tile, in the order (a0,w0) (a0,w1) (a1,w1) (a1,w0); a phase is
//         ds_read the operands the quadrant does not hold yet (12 / 4 / 8 / 0 ds_read_b128)
//         issue ONE half-tile of LDS-direct loads (2 x buffer_load_dwordx4 ... lds per lane)
//         s_waitcnt vmcnt(8 + e) ; s_barrier ; s_waitcnt lgkmcnt(0) ; 8 MFMAs under s_setprio 1 ; s_barrier
//     and the two wave rows run one barrier apart, so on every SIMD one wave is in its MFMA cluster while its partner
//     reads LDS and issues loads.
//   * Loads are never drained: phase q of K-tile g stages  W_1(g+1), A_1(g+1), A_0(g+2), W_0(g+2)  for q = 1..4 -- each
//     into the buffer half its previous tenant's last ds_read left >= 2 phases earlier -- and every wait is counted:
//     "everything but the four half-tiles issued last (and the e epilogue stores issued since) has landed", which is
//     exactly what the next phase reads.  The sequence of K-tiles runs on across output tiles (the staging cursor is two
//     K-tiles ahead, in the next tile if need be).
//   * The epilogue is spread over the phases around a tile boundary, one 32-row strip of the wave tile per phase: strips
//     0 / 1 (final after quadrant (a0,w1)) in phases 3 / 4 of the tile's last K-tile, strips 2 / 3 in phases 1 / 2 of the
//     NEXT tile's first K-tile -- under the partner wave's MFMAs.  A strip goes bias -> activation -> bf16 -> a wave-private
//     4 KB LDS transposition -> buffer_store_dwordx4 of 8 full 128-byte rows per instruction (row-per-lane 8-byte stores
//     touch 32 lines per instruction and made the epilogue 40 % of the launch).
// Results equal the 128 x 128 kernel's up to the place of the bias in the fp32 summation (first instead of last).
// Roofline: bf16 MFMA (2.5 PF dense); per K-tile a block moves 64 KB from L2 for 8.4 MFLOP.
#include <type_traits>

#include "gemm_core.h"
#include "kernels.h"

namespace vlsat {

namespace {

template <int N> __device__ __forceinline__ void p8_wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void p8_barrier() { asm volatile("s_barrier" ::: "memory"); }
__device__ __forceinline__ void p8_wait_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

constexpr int P8_BM = 256, P8_BN = 256, P8_BK = 64;
constexpr int P8_HALF = 128 * 128;            // bytes of a half-tile
constexpr int P8_WBASE = 4 * P8_HALF;         // weight half-tiles start after the four A half-tiles (2 buffers x 2 halves)
constexpr int P8_TBASE = 8 * P8_HALF;         // wave-private transposition buffers of the epilogue (8 x 4 KB)

// (ABL bit 4: no barrier after the MFMA clusters, bit 5: no barrier in the K loop at all -- timing experiments)
enum { P8_MID = 0, P8_LAST = 1, P8_FIRST = 2, P8_SECOND = 3, P8_FIRST0 = 4 };   // FIRST0: first K-tile of a tile without strips of a previous one

#define VLSAT_P8_NAME gemm_p8_kernel
#define VLSAT_P8_FS false
#include "gemm_p8_kernel.h"
#undef VLSAT_P8_NAME
#undef VLSAT_P8_FS
// the split-fp16 siblings of the exact-fp32 rows: gemm_p8s_kernel<2, ADD, RELU, 0> (FS in gemm_p8_kernel.h)
#define VLSAT_P8_NAME gemm_p8s_kernel
#define VLSAT_P8_FS true
#include "gemm_p8_kernel.h"
#undef VLSAT_P8_NAME
#undef VLSAT_P8_FS

}  // namespace

// one kernel pointer per row of the variant list (gemm_plan.h), in its order: taking the address is what instantiates a row
typedef void (*P8Kernel)(GemmArgs, int, int);
#define VLSAT_P8_KERNEL(...) gemm_p8_kernel<__VA_ARGS__>,
constexpr P8Kernel kP8Kernels[] = {VLSAT_GEMM_P8_VARIANTS(VLSAT_P8_KERNEL)};
#undef VLSAT_P8_KERNEL
static_assert(sizeof kP8Kernels / sizeof kP8Kernels[0] == kGemmP8Count, "one kernel per row of the variant list");
#define VLSAT_P8S_KERNEL(...) gemm_p8s_kernel<2, __VA_ARGS__, 0>,
constexpr P8Kernel kP8sKernels[] = {VLSAT_GEMM_P8S_VARIANTS(VLSAT_P8S_KERNEL)};
#undef VLSAT_P8S_KERNEL
static_assert(sizeof kP8sKernels / sizeof kP8sKernels[0] == kGemmP8sCount, "one kernel per row of the sibling list");
#define VLSAT_P8S_PAIR_KERNEL(...) gemm_p8s_kernel<2, __VA_ARGS__>,
constexpr P8Kernel kP8sPairKernels[] = {VLSAT_GEMM_P8S_PAIR_VARIANTS(VLSAT_P8S_PAIR_KERNEL)};
#undef VLSAT_P8S_PAIR_KERNEL
static_assert(sizeof kP8sPairKernels / sizeof kP8sPairKernels[0] == kGemmP8sPairCount, "one kernel per row of the pair-word list");

// full rounds of a large-M launch on 256 x 256 tiles: half-row bf16 / fp16 operands (prec 1), exact fp32 (prec 0) or split-bf16
// on split-pair operands (prec 3).  Which launches come here, and as which row, is plan_gemm with gemm_p8_pick.
// (round 4, measured and dropped: loading the accumulator inits of the wave tile's second row half one phase later, under
//  the MFMAs of phases 1 / 2 -- fp32 nn_edge.0 + gathered rows 923 vs 917 us, out-projection + residual 480 vs 483: the
//  cost of additive operands is not latency at the start of a tile; it is consistent with every CU pulling its 256-512 KB at the same
//  moment: 64-128 MB per round of tiles at what the memory system delivers)
int launch_gemm_p8(const GemmArgs& a, const GemmPlan& p, hipStream_t s) {
    // (GemmArgs::f16s: the split-fp16 sibling of an exact-fp32 row takes the launch as planned -- gemm_p8s_pick)
    const int sib = gemm_p8s_pick(a, p.variant);
    P8Kernel k = sib >= 0 ? kP8sKernels[sib] : kP8Kernels[p.variant];
    if (a.a_pair || a.c_pair) {                  // GEMM pair words: only the sibling's pair forms read and write them
        const int pr = gemm_p8s_pair_pick(a, p.variant);
        if (pr < 0) return fail(-1, "gemm_p8: pair words (a_pair / c_pair) on a launch without a split-fp16 pair form");
        k = kP8sPairKernels[pr];
    }
    hipLaunchKernelGGL(k, dim3(p.grid), dim3(512), 0, s, a, p.n_tiles, a.N / P8_BN);
    if (a.launches) ++*a.launches;
    VLSAT_LAUNCH_CHECK("gemm_p8");
    return 0;
}

}  // namespace vlsat
