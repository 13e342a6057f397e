// What the three tiled-GEMM translation units share (gemm.hip: the 128-row tile family, gemm256.hip: 256 x 256 plain NT,
// gemm256_tn.hip: 256 x 256 TN weight gradient).  Included by those three only.
//   * the K range of a split -- every split-K launch of the family feeds gemm.hip's splitk_reduce_kernel, so there is ONE rule
//   * the LDS-direct buffer load, the barrier with compiler fences, the vector / LDS typedefs, the transpose fragment read
//   * the two source-side LDS swizzles, each with the one explanation of why it is conflict-free
//   * the pieces of the 256-tile kernels' body that do not differ between them: stage selectors, accumulator clear, the
//     bf16 MFMA quadrant (their 4-phase main loops deliberately stay two copies: they differ in where phase 1 splits its
//     reads, how an item ends and whether the epilogue un-staggers the wave rows)
#pragma once
#include "common_hip.h"
#include <type_traits>
#include "../../include/mammoclip_hip.h"

namespace gt {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((ext_vector_type(4))) short s4_t;
typedef __attribute__((ext_vector_type(8))) short s8_t;
typedef __attribute__((address_space(3))) s4_t lds_s4_t;
typedef __attribute__((address_space(3))) unsigned int lds_u32_t;

// ---- K range [kbeg, kend) of one split, in rows of the reduction index (empty when kbeg >= kend).
// Plain form: the K tiles are dealt to the splits in equal runs.  Grouped form (split_group_rows > 0): the reduction
// index is cut at group (= image) boundaries, split_sub splits per group, so that a per-(group, column) factor can be
// applied when the partials are combined (see splitk_reduce_kernel).
struct KRange { long long kbeg, kend; };
__host__ __device__ __forceinline__ KRange split_k_range(const mc_gemm_args& p, int split, int BK) {
    const long long ktiles = (p.K + BK - 1) / BK;
    const long long tps = (ktiles + p.splits - 1) / p.splits;
    KRange r;
    r.kbeg = (long long)split * tps * BK;
    r.kend = r.kbeg + tps * BK;
    if (p.split_group_rows > 0) {
        const long long grp = split / p.split_sub, j = split % p.split_sub;
        const long long chunk = (p.split_group_rows + p.split_sub - 1) / p.split_sub;
        r.kbeg = grp * p.split_group_rows + j * chunk;
        r.kend = r.kbeg + chunk;
        if (r.kend > (grp + 1) * p.split_group_rows) r.kend = (grp + 1) * p.split_group_rows;
    }
    if (r.kend > p.K) r.kend = p.K;
    return r;
}

// ---- LDS-direct buffer load of 16 bytes per lane: lane l's bytes land at M0 + 16 l.  voff = per-lane byte offset from the
// descriptor's base (range-checked against num_records: out-of-range lanes deliver zeros).  Inline assembly: the compiler
// keeps no book on it (the kernel counts vmcnt itself); M0 is written in the statement that uses it.
__device__ __forceinline__ void dma16(unsigned voff, u32x4 srd, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds"
                 :: "v"(voff), "s"(srd), "s"(lds_dst) : "memory");
}

// workgroup barrier that neither the compiler's memory accesses nor its instruction scheduler move across
#define GT_BAR()                                     \
    do {                                             \
        asm volatile("" ::: "memory");               \
        __builtin_amdgcn_s_barrier();                \
        asm volatile("" ::: "memory");               \
        __builtin_amdgcn_sched_barrier(0);           \
    } while (0)

// ---- MFMA fragment of a k-major operand that lies ROW-MAJOR in LDS ([k][x]): gfx950's LDS transpose-read.  Within a
// 16-lane group lane i supplies the address of row i/4, cols (i%4)*4..+3 of a 4 (k) x 16 (x) block and lane c receives
// column c, rows 0..3 (verified on hardware); `lo` addresses k rows 0-3 of the lane group's 8, `hi` rows 4-7.
__device__ __forceinline__ bf16x8_t tr_read(const unsigned char* lo_addr, const unsigned char* hi_addr) {
    const s4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(lo_addr));
    const s4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(hi_addr));
    const s8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, v);
}

// ---- source-side swizzles.  The DMA writes a wave-instruction's 64 x 16 bytes lane-linearly, so the LDS image is plain
// rows and the bank-conflict swizzle sits on the SOURCE address: the lane that fills 16-byte slot s of LDS row r fetches
// chunk s ^ x(r) of that row (still the same line), and a fragment read of chunk c addresses slot c ^ x(r).
//
// k-contiguous rows ([x][64 k] bf16, 128 bytes = 8 chunks per row), x(r) = swz_kc(r): ds_read_b128 serves 16 lanes at a
// time, rows r .. r+15 of ONE chunk; the 8 row pairs land in 8 different slots, and the two rows of a pair are 128 bytes =
// half the 64 banks apart -- 16 rows x 16 bytes cover all 64 banks exactly once.
__host__ __device__ __forceinline__ constexpr int swz_kc(int r) { return (r >> 1) & 7; }
// k-major rows ([64 k][128 x] bf16, 256 bytes = 16 chunks per row, read by tr_read), x(r) = 2 swz_km(r): swz_km is the XOR
// on the index of a 32-BYTE chunk pair, which keeps the pairs a transpose-read needs together; the 8 k rows {8g .. 8g+3} U
// {8g+8 .. 8g+11} a 32-lane bank group touches land in 8 different 32-byte columns.  (It looks at bits 0, 1 and 3 of r.)
__host__ __device__ __forceinline__ constexpr int swz_km(int r) { return (r & 3) | ((r >> 1) & 4); }

// acc[..][..] = 0 for an accumulator array of f32x4_t.  A macro, not a function: through a function the compiler orders the
// accumulator registers of the 256 x 256 kernels differently, and their register allocation is part of what was tuned.
#define GT_CLEAR_ACC(acc)                                                                 \
    do {                                                                                  \
        _Pragma("unroll") for (auto& row_ : acc)                                          \
            _Pragma("unroll") for (auto& a_ : row_) a_ = (f32x4_t){0.f, 0.f, 0.f, 0.f};   \
    } while (0)

// ---- shared body of the two 256 x 256 kernels (8 waves = 2 (M) x 4 (N), wave tile 128 x 64, quadrants of 64 x 32)
// half-tile selectors of a stage [A0 | A1 | B0 | B1], and quadrant indices
using C0 = std::integral_constant<int, 0>; using C1 = std::integral_constant<int, 1>;
using C2 = std::integral_constant<int, 2>; using C3 = std::integral_constant<int, 3>;

// one C quadrant (ih, jh) of a K tile: 2 x 4 x 2 MFMAs.  Operands swapped (D = Bfrag . Afrag^T): a lane holds 4
// consecutive output COLUMNS of one output row
//   acc[i8][j4][r]: row = wm*128 + i8*16 + (lane & 15), column = wn*64 + j4*16 + (lane >> 4)*4 + r
template <int ih, int jh>
__device__ __forceinline__ void mma_quad(f32x4_t (&acc)[8][4], const bf16x8_t (&af)[4][2], const bf16x8_t (&bf)[2][2]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[ih * 4 + i][jh * 2 + j] = MC_MFMA_16x16x32(bf[j][kk], af[i][kk], acc[ih * 4 + i][jh * 2 + j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
}

}  // namespace gt
