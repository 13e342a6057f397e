// Evaluation metrics on the device: image-to-report retrieval ranks, top-k retrieval, the zero-shot softmax and the pair
// counts behind AUROC; per-sample rank counts and the record of binary-classification metrics (pF1, PR-AUC, AP, threshold
// scores) reduced from them, and the same record for every bootstrap replicate of the samples.  All
// fp32 (embeddings are fp32 in both storage builds).
// [ref: breastclip/evaluator.py:146-252 (eval_zeroshot, eval_img_text_retrieval), 255-346 (classification scores)]
//
// The similarity product a[N,D] . b[M,D]^T is STREAMED: a workgroup owns 64 image rows and a chunk of the M texts, walks the
// chunk in tiles of 128 texts staged through LDS, and reduces every 64 x 128 tile of scores to what the caller wants (a count
// per row, or a running top-k list per row) before the next tile overwrites it.  The N x M matrix never exists in memory.
// Products run on the f32-input MFMA (v_mfma_f32_32x32x2_f32): exact f32, one rounding per product, the same value as an fmaf
// chain in the same k order -- bf16 / f16 operands would reorder ranks.
#include "common_hip.h"
#include "../../include/mammoclip_hip.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef unsigned long long u64;

constexpr int BM = 64;          // image rows of a workgroup
constexpr int BN = 128;         // texts of one tile
constexpr int KT = 32;          // k extent of one LDS stage
constexpr int LDK = KT + 1;     // LDS row stride of a staged operand (odd: the 32 rows a wave reads spread over the banks)
constexpr int LDS_S = BN + 1;   // LDS row stride of a stored score tile
constexpr int KMAX = 32;        // largest k of mc_sim_topk
constexpr int MAX_SPLITS = 64;

// rows x KT floats of src[., D] into dst[rows][LDK]; row r is src row gather[r] (gather != null) or row0 + r; rows outside
// [0, nrows_total) and k >= D are zeros (a zero product leaves an accumulator unchanged, so padding never alters a score)
template <int ROWS>
__device__ __forceinline__ void stage_rows(float* __restrict__ dst, const float* __restrict__ src, int nrows_total, int row0,
                                           const int* gather, int k0, int D, bool vec) {
    if (vec) {
        for (int e = threadIdx.x; e < ROWS * (KT / 4); e += 256) {
            const int r = e >> 3, c = (e & 7) * 4;
            const int gr = gather ? gather[r] : row0 + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gr >= 0 && gr < nrows_total && k0 + c < D) v = *reinterpret_cast<const float4*>(src + (long long)gr * D + k0 + c);
            float* d = dst + r * LDK + c;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    } else {
        for (int e = threadIdx.x; e < ROWS * KT; e += 256) {
            const int r = e >> 5, c = e & 31;
            const int gr = gather ? gather[r] : row0 + r;
            dst[r * LDK + c] = (gr >= 0 && gr < nrows_total && k0 + c < D) ? src[(long long)gr * D + k0 + c] : 0.f;
        }
    }
}

// row of accumulator register `reg` inside a wave's 32 x 32 tile (the column is lane & 31)
__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// order-preserving key of (score, index): a larger key is a better match -- higher score first, lower index on equal scores.
// 0 is "no entry" (never produced by a real pair: the high word of a real key has bit 31 or some bit below it set).
__device__ __forceinline__ u64 make_key(float v, int idx) {
    uint32_t u = __float_as_uint(v + 0.f);                      // -0 -> +0: equal scores get equal high words
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u64)u << 32) | (u64)(0xffffffffu - (uint32_t)idx);
}
__device__ __forceinline__ float key_score(u64 k) {
    uint32_t u = (uint32_t)(k >> 32);
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}
__device__ __forceinline__ int key_index(u64 k) { return (int)(0xffffffffu - (uint32_t)k); }
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        const u64 w = ((u64)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}
// the k best of {c0, c1, c2 of every lane} in order, entry j returned in lane j (k <= 32 <= 64); keys of real entries are
// distinct (distinct indices), so exactly one lane retires the winner of a round
__device__ __forceinline__ u64 wave_select_k(u64 c0, u64 c1, u64 c2, int k, int lane) {
    u64 mine = 0;
    for (int r = 0; r < k; ++r) {
        u64 best = c0 > c1 ? c0 : c1;
        best = best > c2 ? best : c2;
        best = wave_max_u64(best);
        if (best == 0) break;                                   // fewer than k entries (wave-uniform)
        if (c0 == best) c0 = 0; else if (c1 == best) c1 = 0; else if (c2 == best) c2 = 0;
        if (lane == r) mine = best;
    }
    return mine;
}

// MODE 0: rank[i] += #{ j in chunk : <a_i, b_j> > <a_i, b_label[i]> }   (rank pre-set to 1, or -1 for a label out of range)
// MODE 1: ws[i][split][0..k) = keys of the k best texts of the chunk, best first
template <int MODE>
__global__ __launch_bounds__(256) void sim_stream_k(const float* __restrict__ a, const float* __restrict__ b,
                                                    const int* __restrict__ label, int* __restrict__ rank,
                                                    u64* __restrict__ ws, int N, int M, int D, int chunk, int k, int vec) {
    constexpr int STAGE = (BM + BN) * LDK, SCORES = BM * LDS_S;
    __shared__ float smem[MODE == 1 ? (SCORES > STAGE ? SCORES : STAGE) : STAGE];
    __shared__ u64 s_top[MODE == 1 ? BM * KMAX : 1];
    __shared__ float s_pair[BM];
    __shared__ int s_lab[BM], s_cnt[BM];
    float* sa = smem;
    float* sb = smem + BM * LDK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave & 1, wc = wave >> 1;                    // wave tile: rows 32 wr .., columns 64 wc .. of the 64 x 128 tile
    const int l31 = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * BM;
    const int m_begin = blockIdx.y * chunk, m_end = min(M, m_begin + chunk);
    const f32x16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    float pair[16];
    int cnt[16];
    if (MODE == 0) {
        // The paired similarity <a_i, b_label[i]> comes out of the SAME instruction sequence as the streamed ones: the paired
        // texts are staged as a 64-row operand and the diagonal of the wave's 32 x 32 product is kept.  A text therefore never
        // outranks itself, and an exact duplicate of it ties.
        if (threadIdx.x < BM) {
            const int i = row0 + threadIdx.x;
            const int lb = i < N ? label[i] : -1;
            s_lab[threadIdx.x] = (lb >= 0 && lb < M) ? lb : -1;
            s_cnt[threadIdx.x] = 0;
        }
        __syncthreads();
        f32x16_t acc = zero16;
        for (int k0 = 0; k0 < D; k0 += KT) {
            stage_rows<BM>(sa, a, N, row0, nullptr, k0, D, vec);
            stage_rows<BM>(sb, b, M, 0, s_lab, k0, D, vec);
            __syncthreads();
            if (wc == 0) {
#pragma unroll
                for (int ks = 0; ks < KT; ks += 2)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[(wr * 32 + l31) * LDK + ks + h], sb[(wr * 32 + l31) * LDK + ks + h],
                                                               acc, 0, 0, 0);
            }
            __syncthreads();
        }
        if (wc == 0) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                if (acc_row(reg, lane) == l31)                  // diagonal element: row == column
                    s_pair[wr * 32 + l31] = s_lab[wr * 32 + l31] >= 0 ? acc[reg] : __builtin_inff();
        }
        __syncthreads();
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) { pair[reg] = s_pair[wr * 32 + acc_row(reg, lane)]; cnt[reg] = 0; }
    } else {
        for (int e = threadIdx.x; e < BM * KMAX; e += 256) s_top[e] = 0;
        __syncthreads();
    }

    for (int t0 = m_begin; t0 < m_end; t0 += BN) {
        f32x16_t acc0 = zero16, acc1 = zero16;
        for (int k0 = 0; k0 < D; k0 += KT) {
            stage_rows<BM>(sa, a, N, row0, nullptr, k0, D, vec);
            stage_rows<BN>(sb, b, m_end, t0, nullptr, k0, D, vec);
            __syncthreads();
            const float* pa = sa + (wr * 32 + l31) * LDK + h;
            const float* pb = sb + (wc * 64 + l31) * LDK + h;
#pragma unroll
            for (int ks = 0; ks < KT; ks += 2) {
                const float av = pa[ks];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, pb[ks], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, pb[32 * LDK + ks], acc1, 0, 0, 0);
            }
            __syncthreads();
        }
        const int c0 = t0 + wc * 64 + l31, c1 = c0 + 32;        // this lane's two texts
        if (MODE == 0) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                cnt[reg] += (int)(c0 < m_end && acc0[reg] > pair[reg]) + (int)(c1 < m_end && acc1[reg] > pair[reg]);
        } else {
            // (the stage buffers are free: the k loop ended on a barrier)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                float* srow = smem + (wr * 32 + acc_row(reg, lane)) * LDS_S + wc * 64 + l31;
                srow[0] = acc0[reg];
                srow[32] = acc1[reg];
            }
            __syncthreads();
            for (int r = wave * 16; r < wave * 16 + 16; ++r) {  // one wave merges the tile into the lists of 16 rows
                if (row0 + r >= N) break;
                const int j0 = t0 + lane, j1 = t0 + 64 + lane;
                u64 n0 = j0 < m_end ? make_key(smem[r * LDS_S + lane], j0) : 0;
                u64 n1 = j1 < m_end ? make_key(smem[r * LDS_S + 64 + lane], j1) : 0;
                const u64 thr = s_top[r * KMAX + k - 1];        // the k-th best so far (0 while the list is short)
                if (n0 <= thr) n0 = 0;
                if (n1 <= thr) n1 = 0;
                if (!__any((n0 | n1) != 0)) continue;
                const u64 old = lane < k ? s_top[r * KMAX + lane] : 0;
                const u64 mine = wave_select_k(n0, n1, old, k, lane);
                if (lane < k) s_top[r * KMAX + lane] = mine;
            }
            __syncthreads();
        }
    }

    if (MODE == 0) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
            if (cnt[reg]) atomicAdd(&s_cnt[wr * 32 + acc_row(reg, lane)], cnt[reg]);
        __syncthreads();
        // integer adds: the result does not depend on the order in which the chunks' workgroups finish
        if (threadIdx.x < BM && row0 + threadIdx.x < N && s_lab[threadIdx.x] >= 0 && s_cnt[threadIdx.x])
            atomicAdd(&rank[row0 + threadIdx.x], s_cnt[threadIdx.x]);
    } else {
        for (int e = threadIdx.x; e < BM * k; e += 256) {
            const int r = e / k, j = e % k;
            if (row0 + r < N) ws[((long long)(row0 + r) * gridDim.y + blockIdx.y) * k + j] = s_top[r * KMAX + j];
        }
    }
}

__global__ void rank_init_k(const int* __restrict__ label, int* __restrict__ rank, int N, int M) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) rank[i] = (label[i] >= 0 && label[i] < M) ? 1 : -1;
}

// one wave per row: the k best of the row's splits * k candidates under the same total order, so the result does not depend
// on how M was split
__global__ void topk_merge_k(const u64* __restrict__ ws, int N, int splits, int k, float* __restrict__ vals, int* __restrict__ idx) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const u64* c = ws + (long long)row * splits * k;
    const int n = splits * k;
    u64 mine = 0;
    for (int e0 = 0; e0 < n; e0 += 64) mine = wave_select_k(e0 + lane < n ? c[e0 + lane] : 0, 0, mine, k, lane);
    if (lane < k) {
        vals[(long long)row * k + lane] = mine ? key_score(mine) : -__builtin_inff();
        idx[(long long)row * k + lane] = mine ? key_index(mine) : -1;
    }
}

// one wave per image: similarities to the M prompts, then the softmax over them (scores parked in p between the two passes)
__global__ __launch_bounds__(64) void sim_softmax_k(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ p,
                                                    int M, int D) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const float* ar = a + (long long)row * D;
    float* pr = p + (long long)row * M;
    float mx = -__builtin_inff();
    for (int j = 0; j < M; ++j) {
        const float* br = b + (long long)j * D;
        float s = 0.f;
        for (int i = lane; i < D; i += 64) s = fmaf(ar[i], br[i], s);
        s = wave_sum(s);
        mx = fmaxf(mx, s);
        if (lane == 0) pr[j] = s;
    }
    __syncthreads();
    float den = 0.f;
    for (int j = lane; j < M; j += 64) den += expf(pr[j] - mx);
    den = wave_sum(den);
    for (int j = lane; j < M; j += 64) pr[j] = expf(pr[j] - mx) / den;
}

constexpr int AUC_J = 2048;     // scores of one workgroup's comparison partners
// counts[0] += #{(p, n) : s_p > s_n}, counts[1] += #{s_p == s_n}, counts[2] = positives, counts[3] = negatives.
// A score takes part on one side only: the other side sees NaN, which compares false both ways (so does a NaN score).
__global__ __launch_bounds__(256) void auroc_counts_k(const float* __restrict__ score, const int* __restrict__ label,
                                                      u64* __restrict__ counts, int N) {
    __shared__ float s_neg[AUC_J];
    __shared__ u64 s_red[4];
    const float nan = __uint_as_float(0x7fc00000u);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j0 = blockIdx.y * AUC_J, jn = min(AUC_J, N - j0);
    if (threadIdx.x < 4) s_red[threadIdx.x] = 0;
    for (int e = threadIdx.x; e < jn; e += 256) s_neg[e] = label[j0 + e] == 0 ? score[j0 + e] : nan;
    __syncthreads();
    const bool pos = i < N && label[i] != 0;
    const float sp = pos ? score[i] : nan;
    int gt = 0, eq = 0;
    for (int e = 0; e < jn; ++e) {
        const float sn = s_neg[e];
        gt += (int)(sp > sn);
        eq += (int)(sp == sn);
    }
    u64 v[4] = {(u64)gt, (u64)eq, 0, 0};
    if (blockIdx.y == 0 && i < N) { v[2] = pos ? 1 : 0; v[3] = pos ? 0 : 1; }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t w = (uint32_t)v[q];                            // per-thread counts fit 32 bits (<= AUC_J)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(&s_red[q], (u64)w);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_red[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_red[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Binary-classification metrics (pF1, PR-AUC, AP, threshold scores) from per-sample rank counts: the same all-pairs sweep as
// auroc_counts_k gives every point of the ROC and PR curves as exact integers, without a sort.
constexpr int RC_I = 256;       // samples of one workgroup (one per thread)
constexpr int RC_J = 2048;      // comparison partners of one workgroup
constexpr int RC_COLS = 5;      // pos_ge, neg_ge, pos_gt, neg_gt, earlier_eq

// counts[i][0..3] += positives / negatives j of the tile with s_j >= s_i, then with s_j > s_i (i itself is a partner);
// counts[i][4] += #{j < i in the tile : s_j == s_i}.  A NaN score compares false both ways and counts nowhere.
__global__ __launch_bounds__(RC_I) void rank_counts_k(const float* __restrict__ score, const int* __restrict__ label,
                                                      uint32_t* __restrict__ counts, int N) {
    __shared__ float s_s[RC_J];
    __shared__ int s_pos[RC_J];
    const int i = blockIdx.x * RC_I + threadIdx.x;
    const int j0 = blockIdx.y * RC_J, jn = min(RC_J, N - j0);
    for (int e = threadIdx.x; e < jn; e += RC_I) {
        s_s[e] = score[j0 + e];
        s_pos[e] = label[j0 + e] != 0 ? 1 : 0;
    }
    __syncthreads();
    if (i >= N) return;
    const float si = score[i];
    int ge = 0, gt = 0, pge = 0, pgt = 0, early = 0;
    const int ne = min(jn, i - j0);                             // partners [0, ne) of the tile come before i (ne may be <= 0)
    for (int e = 0; e < jn; ++e) {
        const float sj = s_s[e];
        const int p = s_pos[e];
        const int a = (int)(sj >= si), b = (int)(sj > si);
        ge += a;
        gt += b;
        pge += a & p;
        pgt += b & p;
        early += (int)(e < ne) & (a ^ b);                       // s_j == s_i  <=>  >= and not >
    }
    uint32_t* c = counts + (long long)i * RC_COLS;
    // integer adds: the result does not depend on the order in which the partner tiles' workgroups finish
    if (pge) atomicAdd(c + 0, (uint32_t)pge);
    if (ge - pge) atomicAdd(c + 1, (uint32_t)(ge - pge));
    if (pgt) atomicAdd(c + 2, (uint32_t)pgt);
    if (gt - pgt) atomicAdd(c + 3, (uint32_t)(gt - pgt));
    if (early) atomicAdd(c + 4, (uint32_t)early);
}

// pos[i] += #{representatives j of the tile : s_j < s_i} for every representative i (earlier_eq == 0: the first sample of its
// distinct score): the index of i's threshold among the distinct thresholds in ascending order
__global__ __launch_bounds__(RC_I) void rep_rank_k(const float* __restrict__ score, const uint32_t* __restrict__ counts,
                                                   uint32_t* __restrict__ pos, int N) {
    __shared__ float s_s[RC_J];
    const float nan = __uint_as_float(0x7fc00000u);
    const int i = blockIdx.x * RC_I + threadIdx.x;
    const int j0 = blockIdx.y * RC_J, jn = min(RC_J, N - j0);
    for (int e = threadIdx.x; e < jn; e += RC_I) s_s[e] = counts[(long long)(j0 + e) * RC_COLS + 4] == 0 ? score[j0 + e] : nan;
    __syncthreads();
    if (i >= N || counts[(long long)i * RC_COLS + 4] != 0) return;
    const float si = score[i];
    int lt = 0;
    for (int e = 0; e < jn; ++e) lt += (int)(s_s[e] < si);
    if (lt) atomicAdd(pos + i, (uint32_t)lt);
}
__global__ void curve_scatter_k(const float* __restrict__ score, const uint32_t* __restrict__ counts,
                                const uint32_t* __restrict__ pos, int N, int K, int* __restrict__ tp, int* __restrict__ fp,
                                float* __restrict__ thr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N || counts[(long long)i * RC_COLS + 4] != 0) return;
    const uint32_t p = pos[i];
    if (p >= (uint32_t)K) return;                               // (a K that is not the record's: no write out of bounds)
    tp[p] = (int)counts[(long long)i * RC_COLS + 0];
    fp[p] = (int)counts[(long long)i * RC_COLS + 1];
    thr[p] = score[i];
}

constexpr int CR_MAX_BLOCKS = 1024;     // workgroups of the two partial passes (a function of N only: the sums' order is fixed)
constexpr int CR_INTS = 11;             // integer partials of a workgroup (CI_*)
constexpr int CR_F64 = 4;               // fp64 partials of a workgroup
constexpr int CR_WS_ROW = CR_INTS + CR_F64 + 3;   // + the workgroup's best-pF1 candidate (tp, fp, score bits)
enum { CI_NPOS, CI_NNEG, CI_SUM_NEG_GE, CI_SUM_NEG_GT, CI_TP, CI_FP, CI_TN, CI_FN, CI_K, CI_NAN, CI_BADLABEL, CI_COUNT };
static_assert(CI_COUNT == CR_INTS, "one partial per CI_* index");
enum { REC_NPOS, REC_NNEG, REC_GT, REC_EQ, REC_BEST_TP, REC_BEST_FP, REC_BEST_THR, REC_TP, REC_FP, REC_TN, REC_FN, REC_K,
       REC_NAN, REC_BADLABEL, REC_SPARE0, REC_SPARE1, REC_PRAUC, REC_AP, REC_CLIP_POS, REC_CLIP_NEG, REC_SLOTS };
static_assert(REC_SLOTS == 20 && REC_PRAUC == 16, "record layout of include/mammoclip_hip.h");

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}
// xor butterfly: every lane adds the same pairs in the same order on every call, so the sum's bits are fixed
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sums of the 256 threads' values in thread 0 (waves combined in wave order through LDS)
__device__ __forceinline__ u64 block_sum_u64(u64 v, u64* s4) {
    v = wave_sum_u64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return s4[0] + s4[1] + s4[2] + s4[3];
}
__device__ __forceinline__ double block_sum_f64(double v, double* s4) {
    v = wave_sum_f64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// best-pF1 candidate: 2 tp / (tp + fp + n_pos) compared as a cross product in 64-bit integers (tp, fp, n_pos <= 2^24: below
// 2^50), the higher threshold on equal value.  (0, 0, -inf) is "none" and loses against every real candidate (tp >= 1).
struct Best { uint32_t tp, fp; float thr; };
__device__ __forceinline__ bool best_better(const Best& a, const Best& b, u64 npos) {
    const u64 l = (u64)a.tp * ((u64)b.tp + b.fp + npos), r = (u64)b.tp * ((u64)a.tp + a.fp + npos);
    return l > r || (l == r && a.thr > b.thr);
}
__device__ __forceinline__ Best best_shfl_xor(const Best& a, int o) {
    Best b;
    b.tp = __shfl_xor(a.tp, o, 64);
    b.fp = __shfl_xor(a.fp, o, 64);
    b.thr = __shfl_xor(a.thr, o, 64);
    return b;
}

// pass 1: the workgroup's integer partials -> ws[block][0 .. CR_INTS).  counts may be null (the count columns read as 0).
__global__ __launch_bounds__(256) void cls_partial_int_k(const float* __restrict__ score, const int* __restrict__ label,
                                                         const uint32_t* __restrict__ counts, int N, double threshold,
                                                         u64* __restrict__ ws) {
    __shared__ u64 s4[4];
    u64 v[CR_INTS];
#pragma unroll
    for (int q = 0; q < CR_INTS; ++q) v[q] = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        const float s = score[i];
        const int lb = label[i];
        const bool pos = lb != 0, pred = (double)s >= threshold;
        v[CI_NPOS] += (u64)pos;
        v[CI_NNEG] += (u64)!pos;
        v[CI_TP] += (u64)(pos && pred);
        v[CI_FN] += (u64)(pos && !pred);
        v[CI_FP] += (u64)(!pos && pred);
        v[CI_TN] += (u64)(!pos && !pred);
        v[CI_NAN] += (u64)(s != s);
        v[CI_BADLABEL] += (u64)(lb != 0 && lb != 1);
        if (counts) {
            const uint32_t* c = counts + i * RC_COLS;
            if (pos) { v[CI_SUM_NEG_GE] += c[1]; v[CI_SUM_NEG_GT] += c[3]; }
            v[CI_K] += (u64)(c[4] == 0);
        }
    }
#pragma unroll
    for (int q = 0; q < CR_INTS; ++q) {
        const u64 t = block_sum_u64(v[q], s4);
        if (threadIdx.x == 0) ws[(long long)blockIdx.x * CR_WS_ROW + q] = t;
    }
}

// pass 2: n_pos from pass 1's partials, then the workgroup's fp64 partials (samples in a fixed order per thread, threads in a
// fixed tree) and its best-pF1 candidate -> ws[block][CR_INTS ..)
__global__ __launch_bounds__(256) void cls_partial_f64_k(const float* __restrict__ score, const int* __restrict__ label,
                                                         const uint32_t* __restrict__ counts, int N, u64* __restrict__ ws) {
    __shared__ u64 s4[4];
    __shared__ double d4[4];
    __shared__ Best b4[4];
    u64 np = 0;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += 256) np += ws[(long long)b * CR_WS_ROW + CI_NPOS];
    const u64 npos = block_sum_u64(np, s4);
    const double dn = (double)npos;
    double f[CR_F64] = {0.0, 0.0, 0.0, 0.0};                    // PR-AUC, AP, sum of clipped scores over positives, negatives
    Best best = {0u, 0u, -__builtin_inff()};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        const float s = score[i];
        const bool pos = label[i] != 0;
        const double cs = (double)fminf(fmaxf(s, 0.f), 1.f);
        f[2] += pos ? cs : 0.0;                                 // (+ 0.0 leaves a sum's bits as they are)
        f[3] += pos ? 0.0 : cs;
        if (!counts) continue;
        const uint32_t* c = counts + i * RC_COLS;
        const uint32_t tp1 = c[0], fp1 = c[1], tp0 = c[2], fp0 = c[3];
        if (pos) {
            const Best cand = {tp1, fp1, s};
            if (best_better(cand, best, npos)) best = cand;
        }
        if (c[4] == 0 && npos && tp1 + fp1) {                   // the representative of its threshold (tp1 + fp1 == 0: NaN)
            const double p1 = (double)tp1 / (double)(tp1 + fp1);
            const double p0 = tp0 + fp0 ? (double)tp0 / (double)(tp0 + fp0) : 1.0;      // the curve's start: precision 1
            const double dr = (double)tp1 / dn - (double)tp0 / dn;
            f[0] += dr * (p1 + p0) / 2.0;
            f[1] += dr * p1;
        }
    }
    u64* row = ws + (long long)blockIdx.x * CR_WS_ROW + CR_INTS;
#pragma unroll
    for (int q = 0; q < CR_F64; ++q) {
        const double t = block_sum_f64(f[q], d4);
        if (threadIdx.x == 0) row[q] = (u64)__double_as_longlong(t);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const Best other = best_shfl_xor(best, o);
        if (best_better(other, best, npos)) best = other;
    }
    if ((threadIdx.x & 63) == 0) b4[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (best_better(b4[w], best, npos)) best = b4[w];
        row[CR_F64 + 0] = best.tp;
        row[CR_F64 + 1] = best.fp;
        row[CR_F64 + 2] = __float_as_uint(best.thr);
    }
}

// pass 3, one workgroup: the partial rows in row order -> the record
__global__ __launch_bounds__(256) void cls_final_k(const u64* __restrict__ ws, int blocks, int have_counts,
                                                   u64* __restrict__ rec) {
    __shared__ u64 s4[4];
    __shared__ double d4[4];
    __shared__ Best b4[4];
    u64 tot[CR_INTS];
#pragma unroll
    for (int q = 0; q < CR_INTS; ++q) {
        u64 v = 0;
        for (int b = threadIdx.x; b < blocks; b += 256) v += ws[(long long)b * CR_WS_ROW + q];
        tot[q] = block_sum_u64(v, s4);
    }
    double ftot[CR_F64];
#pragma unroll
    for (int q = 0; q < CR_F64; ++q) {
        double v = 0.0;
        for (int b = threadIdx.x; b < blocks; b += 256)
            v += __longlong_as_double((long long)ws[(long long)b * CR_WS_ROW + CR_INTS + q]);
        ftot[q] = block_sum_f64(v, d4);
    }
    const u64 npos = tot[CI_NPOS], nneg = tot[CI_NNEG];
    Best best = {0u, 0u, -__builtin_inff()};
    for (int b = threadIdx.x; b < blocks; b += 256) {
        const u64* row = ws + (long long)b * CR_WS_ROW + CR_INTS + CR_F64;
        const Best cand = {(uint32_t)row[0], (uint32_t)row[1], __uint_as_float((uint32_t)row[2])};
        if (best_better(cand, best, npos)) best = cand;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const Best other = best_shfl_xor(best, o);
        if (best_better(other, best, npos)) best = other;
    }
    if ((threadIdx.x & 63) == 0) b4[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w)
        if (best_better(b4[w], best, npos)) best = b4[w];
    const bool curve = have_counts && npos;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    rec[REC_NPOS] = npos;
    rec[REC_NNEG] = nneg;
    rec[REC_GT] = have_counts ? npos * nneg - tot[CI_SUM_NEG_GE] : 0;          // sum over positives of (n_neg - neg_ge)
    rec[REC_EQ] = have_counts ? tot[CI_SUM_NEG_GE] - tot[CI_SUM_NEG_GT] : 0;    // sum over positives of (neg_ge - neg_gt)
    rec[REC_BEST_TP] = best.tp;
    rec[REC_BEST_FP] = best.fp;
    rec[REC_BEST_THR] = __float_as_uint(best.thr);
    rec[REC_TP] = tot[CI_TP];
    rec[REC_FP] = tot[CI_FP];
    rec[REC_TN] = tot[CI_TN];
    rec[REC_FN] = tot[CI_FN];
    rec[REC_K] = tot[CI_K];
    rec[REC_NAN] = tot[CI_NAN];
    rec[REC_BADLABEL] = tot[CI_BADLABEL];
    rec[REC_SPARE0] = 0;
    rec[REC_SPARE1] = 0;
    rec[REC_PRAUC] = (u64)__double_as_longlong(curve ? ftot[0] : nan);
    rec[REC_AP] = (u64)__double_as_longlong(curve ? ftot[1] : nan);
    rec[REC_CLIP_POS] = (u64)__double_as_longlong(ftot[2]);
    rec[REC_CLIP_NEG] = (u64)__double_as_longlong(ftot[3]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Bootstrap replicates of the record.  bin(i) = N - pos_ge_i - neg_ge_i = the number of samples with a
// strictly smaller score: equal for tied samples, monotone in the score, so the N bins (empty ones where scores tie) are the
// thresholds in ascending order and a replicate is a histogram hist[bin][class] of its N draws -- no sort, no second sweep.
constexpr uint32_t BOOT_STREAM = 0x626f6f74u;   // counter word 2 of every draw ("boot")
constexpr int BOOT_TILE = 1024;                 // bins of one scan step: 256 threads x 4
constexpr long long BOOT_HIST_CAP = 64ll << 20; // bytes of histogram of one chunk of replicates (chosen chunk; at least 1)
constexpr int BOOT_MAX_B = 1 << 20;
constexpr int BOOT_MAX_CHUNK = 65535;           // replicates of a chunk = gridDim.y of the histogram kernel

// exclusive prefix of v over the 256 threads (lane order, then wave order) and the block's total; s_w: 4 words of LDS
__device__ __forceinline__ u64 block_excl_scan_u64(u64 v, u64* s_w, u64* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lo = __shfl_up((uint32_t)incl, o, 64), hi = __shfl_up((uint32_t)(incl >> 32), o, 64);
        if (lane >= o) incl += ((u64)hi << 32) | lo;
    }
    __syncthreads();                                            // (the previous step's reads of s_w are done)
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    u64 off = 0;
    for (int w = 0; w < wave; ++w) off += s_w[w];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return off + incl - v;
}

// table[i] = bin(i) | class(i) << 31, bin_score[bin(i)] = s_i (tied samples store the same value).  A sample the counts do
// not place (a NaN score counts nowhere) goes to bin N - 1: whatever the input, every bin is inside [0, N).
__global__ __launch_bounds__(256) void boot_table_k(const float* __restrict__ score, const int* __restrict__ label,
                                                    const uint32_t* __restrict__ counts, int N, uint32_t* __restrict__ table,
                                                    float* __restrict__ bin_score) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint32_t ge = counts[(long long)i * RC_COLS + 0] + counts[(long long)i * RC_COLS + 1];
    const uint32_t bin = ge - 1u < (uint32_t)N ? (uint32_t)N - ge : (uint32_t)N - 1u;
    table[i] = bin | (label[i] != 0 ? 0x80000000u : 0u);
    bin_score[bin] = score[i];
}

// one workgroup: strat[0 .. n_pos) = the table entries of the positives in index order, strat[N .. N + n_neg) = those of the
// negatives; hdr = (n_pos, n_neg).  A tile of 1024 samples per step, block scan with a carried prefix.
__global__ __launch_bounds__(256) void boot_strat_k(const uint32_t* __restrict__ table, int N, uint32_t* __restrict__ strat,
                                                    uint32_t* __restrict__ hdr) {
    __shared__ u64 s_w[4];
    u64 carry = 0;                                              // positives so far << 32 | negatives so far
    for (int base = 0; base < N; base += BOOT_TILE) {
        const int i0 = base + 4 * (int)threadIdx.x;
        uint32_t e[4];
        u64 v = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            e[q] = i0 + q < N ? table[i0 + q] : 0u;
            if (i0 + q < N) v += e[q] >> 31 ? 1ull << 32 : 1ull;
        }
        u64 total;
        const u64 ex = block_excl_scan_u64(v, s_w, &total) + carry;
        uint32_t p = (uint32_t)(ex >> 32), n = (uint32_t)ex;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (i0 + q >= N) continue;
            if (e[q] >> 31) strat[p++] = e[q];
            else strat[(long long)N + n++] = e[q];
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        hdr[0] = (uint32_t)(carry >> 32);
        hdr[1] = (uint32_t)carry;
    }
}

// replicate r = r0 + blockIdx.y, draws t = 4 q .. 4 q + 3 of thread q: word t & 3 of philox4x32((t >> 2, r, BOOT_STREAM,
// 0x5bd1e995), seed).  Plain: entry (u N) >> 32 of `table` (index order).  Stratified (hdr != null, table = strat): draws
// t < n_pos take positive (u n_pos) >> 32, the others negative (u n_neg) >> 32.  hist[rl][bin][class] += 1, ctr[rl] += the
// replicate's positives: integer atomics, the result does not depend on their order.
__global__ __launch_bounds__(256) void boot_hist_k(const uint32_t* __restrict__ table, const uint32_t* __restrict__ hdr, int N,
                                                   int r0, uint32_t seed_lo, uint32_t seed_hi, uint32_t* __restrict__ hist,
                                                   uint32_t* __restrict__ ctr) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    const uint32_t np = hdr ? hdr[0] : (uint32_t)N, nn = hdr ? hdr[1] : 0u;
    const uint4 r4 = philox4x32(q, (uint32_t)(r0 + (int)blockIdx.y), BOOT_STREAM, 0x5bd1e995u, seed_lo, seed_hi);
    const uint32_t w[4] = {r4.x, r4.y, r4.z, r4.w};
    uint32_t* h = hist + (size_t)blockIdx.y * (size_t)N * 2;
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t t = 4u * q + k;
        if (t >= (uint32_t)N) continue;
        // t >= np only when stratified, and then nn = N - np >= 1: both forms stay inside the table
        const uint32_t j = t < np ? __umulhi(w[k], np) : (uint32_t)N + __umulhi(w[k], nn);
        const uint32_t e = table[j];
        atomicAdd(h + 2 * (size_t)(e & 0x7fffffffu) + (e >> 31), 1u);
        mine += e >> 31;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(ctr + blockIdx.y, mine);
}

// one workgroup per replicate: the bins in descending order, 1024 per step, cumulative (tp, fp) by a block scan with a
// carried prefix; every sum is per thread in step order, then over the threads in a fixed tree -- the bits are a function of
// (hist, N) alone.  The record's slots and their meaning are mc_cls_record's on the resampled multiset.
__global__ __launch_bounds__(256) void boot_record_k(const uint32_t* __restrict__ hist, const uint32_t* __restrict__ ctr,
                                                     const float* __restrict__ bin_score, int N, double threshold,
                                                     u64* __restrict__ records) {
    __shared__ u64 s_w[4];
    __shared__ u64 s4[4];
    __shared__ double d4[4];
    __shared__ Best b4[4];
    const uint32_t* h = hist + (size_t)blockIdx.x * (size_t)N * 2;
    const u64 npos = ctr[blockIdx.x], nneg = (u64)N - npos;
    const double dn = (double)npos;
    u64 carry = 0;                                              // tp << 32 | fp over the bins above this step
    u64 iv[7] = {0, 0, 0, 0, 0, 0, 0};                          // gt, eq, tp, fp, tn, fn, K
    double f[CR_F64] = {0.0, 0.0, 0.0, 0.0};
    Best best = {0u, 0u, -__builtin_inff()};
    for (int base = 0; base < N; base += BOOT_TILE) {
        const int p0 = base + 4 * (int)threadIdx.x;
        uint32_t cp[4], cn[4];
        u64 v = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cp[q] = cn[q] = 0;
            if (p0 + q < N) {
                const uint2 c = *reinterpret_cast<const uint2*>(h + 2 * (size_t)(N - 1 - (p0 + q)));
                cn[q] = c.x;
                cp[q] = c.y;
            }
            v += ((u64)cp[q] << 32) | cn[q];
        }
        u64 total;
        const u64 ex = block_excl_scan_u64(v, s_w, &total) + carry;
        uint32_t tp0 = (uint32_t)(ex >> 32), fp0 = (uint32_t)ex;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!(cp[q] | cn[q])) continue;                     // a score absent from the replicate is no threshold of it
            const float s = bin_score[N - 1 - (p0 + q)];
            const uint32_t tp1 = tp0 + cp[q], fp1 = fp0 + cn[q];
            iv[0] += (u64)cn[q] * tp0;                          // pairs won: the positives strictly above these negatives
            iv[1] += (u64)cp[q] * cn[q];
            const bool pred = (double)s >= threshold;
            iv[2] += pred ? cp[q] : 0u;
            iv[3] += pred ? cn[q] : 0u;
            iv[4] += pred ? 0u : cn[q];
            iv[5] += pred ? 0u : cp[q];
            iv[6] += 1;
            const double cs = (double)fminf(fmaxf(s, 0.f), 1.f);
            f[2] += cs * (double)cp[q];
            f[3] += cs * (double)cn[q];
            if (cp[q]) {
                const Best cand = {tp1, fp1, s};
                if (best_better(cand, best, npos)) best = cand;
            }
            if (npos) {
                const double p1 = (double)tp1 / (double)(tp1 + fp1);
                const double pp = tp0 + fp0 ? (double)tp0 / (double)(tp0 + fp0) : 1.0;    // the curve's start: precision 1
                const double dr = (double)tp1 / dn - (double)tp0 / dn;
                f[0] += dr * (p1 + pp) / 2.0;
                f[1] += dr * p1;
            }
            tp0 = tp1;
            fp0 = fp1;
        }
        carry += total;
    }
    u64 tot[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) tot[q] = block_sum_u64(iv[q], s4);
    double ftot[CR_F64];
#pragma unroll
    for (int q = 0; q < CR_F64; ++q) ftot[q] = block_sum_f64(f[q], d4);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const Best other = best_shfl_xor(best, o);
        if (best_better(other, best, npos)) best = other;
    }
    if ((threadIdx.x & 63) == 0) b4[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w)
        if (best_better(b4[w], best, npos)) best = b4[w];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    u64* rec = records + (size_t)blockIdx.x * REC_SLOTS;
    rec[REC_NPOS] = npos;
    rec[REC_NNEG] = nneg;
    rec[REC_GT] = tot[0];
    rec[REC_EQ] = tot[1];
    rec[REC_BEST_TP] = best.tp;
    rec[REC_BEST_FP] = best.fp;
    rec[REC_BEST_THR] = __float_as_uint(best.thr);
    rec[REC_TP] = tot[2];
    rec[REC_FP] = tot[3];
    rec[REC_TN] = tot[4];
    rec[REC_FN] = tot[5];
    rec[REC_K] = tot[6];
    rec[REC_NAN] = 0;
    rec[REC_BADLABEL] = 0;
    rec[REC_SPARE0] = 0;
    rec[REC_SPARE1] = 0;
    rec[REC_PRAUC] = (u64)__double_as_longlong(npos ? ftot[0] : nan);
    rec[REC_AP] = (u64)__double_as_longlong(npos ? ftot[1] : nan);
    rec[REC_CLIP_POS] = (u64)__double_as_longlong(ftot[2]);
    rec[REC_CLIP_NEG] = (u64)__double_as_longlong(ftot[3]);
}

constexpr int CLS_MAX_N = 1 << 24;      // counts fit 32 bits, count products fit fp64 (and 64-bit integers) exactly

int g_splits = 0;   // 0: chosen per call
int g_boot_chunk = 0;   // 0: chosen per call
int g_boot_stages = 3;

// workspace of mc_boot_records: 256-byte aligned sections
struct BootLayout { long long hdr, table, strat, bin_score, ctr, hist, bytes; int chunk; };
BootLayout boot_layout(int N, int B) {
    auto up = [](long long v) { return (v + 255) / 256 * 256; };
    BootLayout l;
    long long chunk = g_boot_chunk > 0 ? g_boot_chunk : BOOT_HIST_CAP / (8ll * N);
    if (chunk > BOOT_MAX_CHUNK) chunk = BOOT_MAX_CHUNK;
    if (chunk > B) chunk = B;
    if (chunk < 1) chunk = 1;
    l.chunk = (int)chunk;
    l.hdr = 0;
    l.table = 256;
    l.strat = l.table + up(4ll * N);
    l.bin_score = l.strat + up(8ll * N);
    l.ctr = l.bin_score + up(4ll * N);
    l.hist = l.ctr + up(4ll * chunk);                           // ctr and hist are adjacent: one memset clears both
    l.bytes = l.hist + up(8ll * N * chunk);
    return l;
}

}  // namespace

// texts per workgroup: whole tiles, enough workgroups for ~2 per CU when N alone gives too few row blocks
static int sim_chunk(int N, int M, int* splits_out) {
    const int row_blocks = mc_div_up(N, BM), tiles = mc_div_up(M, BN);
    int splits = g_splits > 0 ? g_splits : mc_div_up(512, row_blocks);
    if (splits > MAX_SPLITS) splits = MAX_SPLITS;
    if (splits > tiles) splits = tiles;
    const int chunk = mc_div_up(tiles, splits) * BN;
    *splits_out = mc_div_up(M, chunk);
    return chunk;
}
static bool sim_vec(const float* a, const float* b, int D) { return D % 4 == 0 && mc_aligned16(a) && mc_aligned16(b); }

extern "C" int mc_sim_set_splits(int splits) {
    MC_CHECK(splits >= 0 && splits <= MAX_SPLITS, "sim_set_splits: splits outside [0, 64]");
    g_splits = splits;
    return MC_OK;
}
extern "C" int mc_sim_rank(const float* a, const float* b, const int* label, int* rank, int N, int M, int D, void* stream) {
    MC_CHECK(a && b && label && rank && N > 0 && M > 0 && D > 0, "sim_rank: bad args");
    int splits;
    const int chunk = sim_chunk(N, M, &splits);
    hipLaunchKernelGGL(rank_init_k, dim3(mc_div_up(N, 256)), dim3(256), 0, (hipStream_t)stream, label, rank, N, M);
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(sim_stream_k<0>, dim3(mc_div_up(N, BM), splits), dim3(256), 0, (hipStream_t)stream, a, b, label, rank,
                       (u64*)nullptr, N, M, D, chunk, 0, (int)sim_vec(a, b, D));
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" long long mc_sim_topk_ws_bytes(int N, int M, int k) {
    if (N <= 0 || M <= 0 || k <= 0) return 0;
    int splits;
    sim_chunk(N, M, &splits);
    return (long long)N * splits * k * (long long)sizeof(u64);
}
extern "C" int mc_sim_topk(const float* a, const float* b, float* vals, int* idx, int N, int M, int D, int k, void* ws,
                           void* stream) {
    MC_CHECK(a && b && vals && idx && ws && N > 0 && M > 0 && D > 0, "sim_topk: bad args");
    MC_CHECK(k >= 1 && k <= KMAX, "sim_topk: k outside [1, 32]");
    MC_CHECK(k <= M, "sim_topk: k exceeds the number of texts");
    int splits;
    const int chunk = sim_chunk(N, M, &splits);
    hipLaunchKernelGGL(sim_stream_k<1>, dim3(mc_div_up(N, BM), splits), dim3(256), 0, (hipStream_t)stream, a, b,
                       (const int*)nullptr, (int*)nullptr, (u64*)ws, N, M, D, chunk, k, (int)sim_vec(a, b, D));
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(topk_merge_k, dim3(mc_div_up(N, 4)), dim3(256), 0, (hipStream_t)stream, (const u64*)ws, N, splits, k, vals,
                       idx);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_sim_softmax(const float* a, const float* b, float* p, int N, int M, int D, void* stream) {
    MC_CHECK(a && b && p && N > 0 && M > 0 && D > 0, "sim_softmax: bad args");
    hipLaunchKernelGGL(sim_softmax_k, dim3(N), dim3(64), 0, (hipStream_t)stream, a, b, p, M, D);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_auroc_counts(const float* score, const int* label, long long* counts, int N, void* stream) {
    MC_CHECK(score && label && counts && N > 0, "auroc_counts: bad args");
    if (hipMemsetAsync(counts, 0, 4 * sizeof(long long), (hipStream_t)stream) != hipSuccess) {
        mc_set_error("auroc_counts: hipMemsetAsync failed");
        return MC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(auroc_counts_k, dim3(mc_div_up(N, 256), mc_div_up(N, AUC_J)), dim3(256), 0, (hipStream_t)stream, score,
                       label, (u64*)counts, N);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_rank_counts(const float* score, const int* label, unsigned int* counts, int N, void* stream) {
    MC_CHECK(score && label && counts, "rank_counts: null pointer");
    MC_CHECK(N >= 1 && N <= CLS_MAX_N, "rank_counts: N outside [1, 2^24]");
    if (hipMemsetAsync(counts, 0, (size_t)N * RC_COLS * sizeof(uint32_t), (hipStream_t)stream) != hipSuccess) {
        mc_set_error("rank_counts: hipMemsetAsync failed");
        return MC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(rank_counts_k, dim3(mc_div_up(N, RC_I), mc_div_up(N, RC_J)), dim3(RC_I), 0, (hipStream_t)stream, score,
                       label, counts, N);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" long long mc_cls_record_ws_bytes(int N) {
    if (N < 1 || N > CLS_MAX_N) return 0;
    return (long long)min(mc_div_up(N, 256), CR_MAX_BLOCKS) * CR_WS_ROW * (long long)sizeof(u64);
}
extern "C" int mc_cls_record(const float* score, const int* label, const unsigned int* counts, int N, double threshold,
                             long long* record, void* ws, void* stream) {
    MC_CHECK(score && label && record && ws, "cls_record: null pointer");
    MC_CHECK(N >= 1 && N <= CLS_MAX_N, "cls_record: N outside [1, 2^24]");
    MC_CHECK(threshold == threshold, "cls_record: the threshold is NaN");
    const int blocks = min(mc_div_up(N, 256), CR_MAX_BLOCKS);
    hipLaunchKernelGGL(cls_partial_int_k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, score, label, counts, N, threshold,
                       (u64*)ws);
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(cls_partial_f64_k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, score, label, counts, N, (u64*)ws);
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(cls_final_k, dim3(1), dim3(256), 0, (hipStream_t)stream, (const u64*)ws, blocks, (int)(counts != nullptr),
                       (u64*)record);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_cls_curve(const float* score, const unsigned int* counts, int N, int K, unsigned int* pos_ws, int* tp, int* fp,
                            float* threshold, void* stream) {
    MC_CHECK(score && counts && pos_ws && tp && fp && threshold, "cls_curve: null pointer");
    MC_CHECK(N >= 1 && N <= CLS_MAX_N, "cls_curve: N outside [1, 2^24]");
    MC_CHECK(K >= 1 && K <= N, "cls_curve: K outside [1, N]");
    if (hipMemsetAsync(pos_ws, 0, (size_t)N * sizeof(uint32_t), (hipStream_t)stream) != hipSuccess) {
        mc_set_error("cls_curve: hipMemsetAsync failed");
        return MC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(rep_rank_k, dim3(mc_div_up(N, RC_I), mc_div_up(N, RC_J)), dim3(RC_I), 0, (hipStream_t)stream, score, counts,
                       pos_ws, N);
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(curve_scatter_k, dim3(mc_div_up(N, 256)), dim3(256), 0, (hipStream_t)stream, score, counts,
                       (const uint32_t*)pos_ws, N, K, tp, fp, threshold);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_boot_set_chunk(int chunk) {
    MC_CHECK(chunk >= 0 && chunk <= BOOT_MAX_CHUNK, "boot_set_chunk: chunk outside [0, 65535]");
    g_boot_chunk = chunk;
    return MC_OK;
}
extern "C" int mc_boot_set_stages(int mask) {
    MC_CHECK(mask >= 1 && mask <= 3, "boot_set_stages: mask outside [1, 3]");
    g_boot_stages = mask;
    return MC_OK;
}
extern "C" long long mc_boot_ws_bytes(int N, int B) {
    if (N < 1 || N > CLS_MAX_N || B < 1 || B > BOOT_MAX_B) return 0;
    return boot_layout(N, B).bytes;
}
extern "C" int mc_boot_records(const float* score, const int* label, const unsigned int* counts, int N, int B, double threshold,
                               unsigned long long seed, int stratified, long long* records, void* ws, long long ws_bytes,
                               void* stream) {
    MC_CHECK(score && label && counts && records && ws, "boot_records: null pointer");
    MC_CHECK(N >= 1 && N <= CLS_MAX_N, "boot_records: N outside [1, 2^24]");
    MC_CHECK(B >= 1 && B <= BOOT_MAX_B, "boot_records: B outside [1, 2^20]");
    MC_CHECK(threshold == threshold, "boot_records: the threshold is NaN");
    const BootLayout l = boot_layout(N, B);
    MC_CHECK(ws_bytes >= l.bytes, "boot_records: the workspace is smaller than mc_boot_ws_bytes(N, B)");
    MC_CHECK(mc_aligned16(ws), "boot_records: the workspace is not 16-byte aligned");
    char* base = (char*)ws;
    uint32_t* hdr = (uint32_t*)(base + l.hdr);
    uint32_t* table = (uint32_t*)(base + l.table);
    uint32_t* strat = (uint32_t*)(base + l.strat);
    float* bin_score = (float*)(base + l.bin_score);
    uint32_t* ctr = (uint32_t*)(base + l.ctr);
    uint32_t* hist = (uint32_t*)(base + l.hist);
    hipStream_t st = (hipStream_t)stream;
    if (g_boot_stages & 1) {
        hipLaunchKernelGGL(boot_table_k, dim3(mc_div_up(N, 256)), dim3(256), 0, st, score, label, counts, N, table, bin_score);
        MC_LAUNCH_CHECK();
        if (stratified) {
            hipLaunchKernelGGL(boot_strat_k, dim3(1), dim3(256), 0, st, (const uint32_t*)table, N, strat, hdr);
            MC_LAUNCH_CHECK();
        }
    }
    for (int r0 = 0; r0 < B; r0 += l.chunk) {
        const int nr = min(l.chunk, B - r0);
        if (g_boot_stages & 1) {
            if (hipMemsetAsync(ctr, 0, (size_t)(l.hist - l.ctr) + (size_t)nr * N * 8, st) != hipSuccess) {
                mc_set_error("boot_records: hipMemsetAsync failed");
                return MC_ERR_LAUNCH;
            }
            hipLaunchKernelGGL(boot_hist_k, dim3(mc_div_up(mc_div_up(N, 4), 256), nr), dim3(256), 0, st,
                               (const uint32_t*)(stratified ? strat : table), (const uint32_t*)(stratified ? hdr : nullptr), N, r0,
                               (uint32_t)seed, (uint32_t)(seed >> 32), hist, ctr);
            MC_LAUNCH_CHECK();
        }
        if (g_boot_stages & 2) {
            hipLaunchKernelGGL(boot_record_k, dim3(nr), dim3(256), 0, st, (const uint32_t*)hist, (const uint32_t*)ctr,
                               (const float*)bin_score, N, threshold, (u64*)records + (size_t)r0 * REC_SLOTS);
            MC_LAUNCH_CHECK();
        }
    }
    return MC_OK;
}
