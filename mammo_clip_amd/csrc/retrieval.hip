// Evaluation metrics on the device: image-to-report retrieval ranks, top-k retrieval, the zero-shot softmax and the pair
// counts behind AUROC.  All fp32 (embeddings are fp32 in both storage builds).
// [ref: breastclip/evaluator.py:146-252 (eval_zeroshot, eval_img_text_retrieval)]
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

int g_splits = 0;   // 0: chosen per call

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
