// Variable-length fused BERT self-attention for gfx950 on PACKED rows: the b reports of a call are concatenated into one
// [R, 3H] row matrix, sequence i owns rows cu_seqlens[i] .. cu_seqlens[i+1]-1, and per (sequence, head)
//     ctx = dropout(softmax(alpha * Q K^T)) V      over the sequence's own 1 <= len_i <= 256 tokens
// -- what attn.hip computes for a padded [b, T] batch whose mask is 1..10..0, without the padded rows.
// [ref: model/modules/text_encoder.py:47-49 -> transformers BertSelfAttention.forward; the reference pads every report to
//       max_length 256 (data/datasets/imagetext.py:217-222) and masks the padding, so the real tokens see exactly this]
//
// Same algorithm, LDS layout and MFMA fragment mapping as attn_fwd_k / attn_bwd_k (see attn.hip), one 8-wave workgroup
// per (sequence, head).  Differences:
//   * the key blocks nJ = ceil(len / 32) and the query-block loop are per-workgroup values; keys >= len of the last
//     block are masked in registers (score = finfo.min, probability exactly 0), there is no mask_bias array;
//   * staging never reads a row at or beyond cu_seqlens[i+1] (the next sequence's, or past the allocation): LDS rows
//     len .. 32*nJ-1 are filled with zeros; lanes of a partial query / key block read the sequence's LAST row instead
//     of their own and do not store;
//   * the dropout element index is the one the padded [b, T] layout uses -- ((i*nh + head)*T + query) * T/8 + key/8 with
//     the caller's padded T -- so one seed drops the same (query, key) pairs as mc_attn_fwd on the padded batch;
//   * lse is [R, nh, 2];
//   * the dynamic LDS is sized by the call's longest sequence (332 bytes per key in the backward: 21 KB at 64 tokens,
//     83 KB at 256), so batches of short reports get more workgroups per CU;
//   * the grid is issued in the order of ``order`` (sequence indices, longest first, optional): a workgroup costs
//     O(len^2), and the long ones should not start last;
//   * rows cu_seqlens[b] .. rows-1 (alignment rows that belong to no sequence) get zeros in ctx / dqkv from the first
//     workgroups of the grid: weight-gradient GEMMs and column sums read them.
// The backward is atomic-free and bit-reproducible like the padded one.
#include "common_hip.h"
#include "attn_frag.h"
#include "../../include/mammoclip_hip.h"

namespace {

struct vattn_args {
    const bf16_t* qkv;      // [rows, 3H]: Q | K | V
    const bf16_t* dctx;     // [rows, H] (backward)
    bf16_t* ctx;            // [rows, H] (forward)
    bf16_t* dqkv;           // [rows, 3H] (backward)
    float* lse;             // [rows, nh][2]: row max, 1 / row sum
    const int* cu;          // [nseq + 1]
    const int* order;       // [nseq] or null
    long long rows;
    int nseq, tl, tpad, nh; // tl: LDS rows (longest sequence rounded up to 32); tpad: T of the padded layout (dropout index)
    float alpha, p;
    unsigned long long seed;
    unsigned int sid;
};

constexpr float NEG_MAX = -3.4028234663852886e38f;

// rows [0, len) from global memory, rows [len, tpad) zero
__device__ __forceinline__ void stage_rows_z(unsigned char* dst, const bf16_t* src, long long ld, int len, int tpad, int tid) {
    for (int idx = tid; idx < tpad * 8; idx += 512) {
        const int row = idx >> 3, ch = idx & 7;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (row < len) v = *reinterpret_cast<const uint4*>(src + (long long)row * ld + ch * 8);
        *reinterpret_cast<uint4*>(dst + row * RS + ch * 16) = v;
    }
}
// zeros in columns [col0, col0 + 64) of rows [r_begin, r_end) of a row-major matrix with leading dimension ld
__device__ __forceinline__ void zero_tail_rows(bf16_t* m, long long ld, int col0, long long r_begin, long long r_end, int tid) {
    if (r_begin < 0) return;
    for (long long idx = tid; idx < (r_end - r_begin) * 8; idx += 512)
        *reinterpret_cast<uint4*>(m + (r_begin + (idx >> 3)) * ld + col0 + (idx & 7) * 8) = make_uint4(0u, 0u, 0u, 0u);
}

template <bool DROP>
__global__ __launch_bounds__(512) void attn_varlen_fwd_k(vattn_args a) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* const Ks = smem;
    unsigned char* const Vs = smem + a.tl * RS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const int nh = a.nh, H = nh * HD, ld = 3 * H;
    const int oi = blockIdx.x / nh, h = blockIdx.x % nh;
    if (oi == 0) zero_tail_rows(a.ctx, H, h * HD, a.cu[a.nseq], a.rows, tid);
    const int bi = a.order ? a.order[oi] : oi;
    if (bi < 0 || bi >= a.nseq) return;
    const int r0 = a.cu[bi], len = a.cu[bi + 1] - r0;
    if (len < 1 || len > a.tl || r0 < 0 || r0 + len > a.rows) return;      // malformed cu_seqlens: touch nothing
    const int tp = (len + 31) & ~31, nJ = tp >> 5;
    const bf16_t* const base = a.qkv + (long long)r0 * ld + h * HD;
    stage_rows_z(Ks, base + H, ld, len, tp, tid);
    stage_rows_z(Vs, base + 2 * H, ld, len, tp, tid);
    __syncthreads();
    for (int qb = wave; qb * 16 < len; qb += 8) {
        const int q = qb * 16 + li, qc = q < len ? q : len - 1;
        bf16x8_t qf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            qf[ks] = *reinterpret_cast<const bf16x8_t*>(base + (long long)qc * ld + ks * 32 + g * 8);
        float s[8][8];
        float mx = NEG_MAX;
#pragma unroll
        for (int J = 0; J < 8; ++J) {
            if (J < nJ) {
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks)
                        acc = MC_MFMA_16x16x32(perm_frag(Ks, 32 * J + 4 * tt, ks, lane), qf[ks], acc, 0, 0, 0);
                    const int key = 32 * J + g * 8 + 4 * tt;
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[J][tt * 4 + r] = key + r < len ? acc[r] * a.alpha : NEG_MAX;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) mx = fmaxf(mx, s[J][i]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int J = 0; J < 8; ++J)
            if (J < nJ)
#pragma unroll
                for (int i = 0; i < 8; ++i) { s[J][i] = __expf(s[J][i] - mx); sum += s[J][i]; }
        const float inv = 1.f / xor_sum16_32(sum);
        if (g == 0 && q < len) *reinterpret_cast<float2*>(a.lse + ((long long)(r0 + q) * nh + h) * 2) = make_float2(mx, inv);
        const long long prow = ((long long)bi * nh + h) * a.tpad + qc;      // row of the padded [b, nh, T, T] probabilities
        f32x4_t o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int J = 0; J < 8; ++J) {
            if (J < nJ) {
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = s[J][i] * inv;
                if (DROP) {
                    float ds[8];
                    dropout_scale8(a.seed, a.sid, (unsigned long long)prow * (a.tpad >> 3) + 4 * J + g, a.p, ds);
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] *= ds[i];
                }
                const bf16x8_t pf = as_frag(v);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    o[dt] = MC_MFMA_16x16x32(tr_frag(Vs, 32 * J, dt * 16, lane), pf, o[dt], 0, 0, 0);
            }
        }
        if (q < len) {
            bf16_t* const dst = a.ctx + (long long)(r0 + q) * H + h * HD + g * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<uint2*>(dst + dt * 16) = make_uint2(pack_bf2(o[dt][0], o[dt][1]), pack_bf2(o[dt][2], o[dt][3]));
        }
    }
}

template <bool DROP>
__global__ __launch_bounds__(512) void attn_varlen_bwd_k(vattn_args a) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* const Ks = smem;                    // phase A: K rows, phase B: Q rows
    unsigned char* const Vs = smem + a.tl * RS;        // phase A: V rows, phase B: dO rows
    float* const lse_s = reinterpret_cast<float*>(smem + 2 * a.tl * RS);           // [tl][2]
    float* const dot_s = lse_s + 2 * a.tl;                                          // [tl]
    unsigned char* const dmask = reinterpret_cast<unsigned char*>(dot_s + a.tl);    // [tl][32] keep bits, 8 keys per byte
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const int nh = a.nh, H = nh * HD, ld = 3 * H;
    const int oi = blockIdx.x / nh, h = blockIdx.x % nh;
    if (oi == 0) {
        const long long rend = a.cu[a.nseq];
#pragma unroll
        for (int part = 0; part < 3; ++part) zero_tail_rows(a.dqkv, ld, part * H + h * HD, rend, a.rows, tid);
    }
    const int bi = a.order ? a.order[oi] : oi;
    if (bi < 0 || bi >= a.nseq) return;
    const int r0 = a.cu[bi], len = a.cu[bi + 1] - r0;
    if (len < 1 || len > a.tl || r0 < 0 || r0 + len > a.rows) return;
    const int tp = (len + 31) & ~31, nJ = tp >> 5;
    const bf16_t* const base = a.qkv + (long long)r0 * ld + h * HD;
    const bf16_t* const dbase = a.dctx + (long long)r0 * H + h * HD;
    bf16_t* const gbase = a.dqkv + (long long)r0 * ld + h * HD;
    stage_rows_z(Ks, base + H, ld, len, tp, tid);
    stage_rows_z(Vs, base + 2 * H, ld, len, tp, tid);
    for (int k = tid; k < tp; k += 512) {
        float2 l2 = make_float2(0.f, 0.f);
        if (k < len) l2 = *reinterpret_cast<const float2*>(a.lse + ((long long)(r0 + k) * nh + h) * 2);
        *reinterpret_cast<float2*>(lse_s + 2 * k) = l2;
        dot_s[k] = 0.f;
    }
    __syncthreads();
    const float invkeep = 1.f / (1.f - a.p);
    // ---------------- phase A: a lane = one query x 8 consecutive keys per 32-key block
    for (int qb = wave; qb * 16 < len; qb += 8) {
        const int q = qb * 16 + li, qc = q < len ? q : len - 1;
        bf16x8_t qf[2], dof[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[ks] = *reinterpret_cast<const bf16x8_t*>(base + (long long)qc * ld + ks * 32 + g * 8);
            dof[ks] = *reinterpret_cast<const bf16x8_t*>(dbase + (long long)qc * H + ks * 32 + g * 8);
        }
        const float mx = lse_s[2 * qc], inv = lse_s[2 * qc + 1];
        const long long prow = ((long long)bi * nh + h) * a.tpad + qc;
        float pr[8][8], d[8][8];
        float dot = 0.f;
#pragma unroll
        for (int J = 0; J < 8; ++J) {
            if (J < nJ) {
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    f32x4_t acc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        acc = MC_MFMA_16x16x32(perm_frag(Ks, 32 * J + 4 * tt, ks, lane), qf[ks], acc, 0, 0, 0);
                        dacc = MC_MFMA_16x16x32(perm_frag(Vs, 32 * J + 4 * tt, ks, lane), dof[ks], dacc, 0, 0, 0);
                    }
                    const int key = 32 * J + g * 8 + 4 * tt;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = key + r < len ? __expf(acc[r] * a.alpha - mx) * inv : 0.f;
                        pr[J][tt * 4 + r] = bf2f(f2bf(v));
                        d[J][tt * 4 + r] = dacc[r];
                    }
                }
                if (DROP) {
                    float ds[8];
                    dropout_scale8(a.seed, a.sid, (unsigned long long)prow * (a.tpad >> 3) + 4 * J + g, a.p, ds);
                    unsigned int bits = 0;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        d[J][i] *= ds[i];
                        bits |= (ds[i] != 0.f ? 1u : 0u) << i;
                    }
                    if (q < len) dmask[q * 32 + 4 * J + g] = (unsigned char)bits;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) dot += pr[J][i] * d[J][i];
            }
        }
        dot = xor_sum16_32(dot);
        if (g == 0 && q < len) dot_s[q] = dot;
        f32x4_t dq[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int J = 0; J < 8; ++J) {
            if (J < nJ) {
                float dsv[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) dsv[i] = pr[J][i] * (d[J][i] - dot) * a.alpha;
                const bf16x8_t dsf = as_frag(dsv);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    dq[dt] = MC_MFMA_16x16x32(tr_frag(Ks, 32 * J, dt * 16, lane), dsf, dq[dt], 0, 0, 0);
            }
        }
        if (q < len) {
            bf16_t* const dst = gbase + (long long)q * ld + g * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<uint2*>(dst + dt * 16) = make_uint2(pack_bf2(dq[dt][0], dq[dt][1]), pack_bf2(dq[dt][2], dq[dt][3]));
        }
    }
    __syncthreads();
    // ---------------- phase B: a lane = one key x 8 consecutive queries per 32-query block; a wave owns 32 keys
    stage_rows_z(Ks, base, ld, len, tp, tid);          // Q rows
    stage_rows_z(Vs, dbase, H, len, tp, tid);          // dO rows
    __syncthreads();
    if (wave * 32 >= len) return;
    bf16x8_t kfr[2][2], vfr[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = wave * 32 + kt * 16 + li, kc = key < len ? key : len - 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kfr[kt][ks] = *reinterpret_cast<const bf16x8_t*>(base + H + (long long)kc * ld + ks * 32 + g * 8);
            vfr[kt][ks] = *reinterpret_cast<const bf16x8_t*>(base + 2 * H + (long long)kc * ld + ks * 32 + g * 8);
        }
    }
    f32x4_t dk[2][4], dv[2][4];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { dk[kt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; dv[kt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
    for (int I = 0; I < nJ; ++I) {
        float sv[2][8], dp[2][8];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            bf16x8_t qr[2], dor[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                qr[ks] = perm_frag(Ks, 32 * I + 4 * tt, ks, lane);
                dor[ks] = perm_frag(Vs, 32 * I + 4 * tt, ks, lane);
            }
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                f32x4_t acc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    acc = MC_MFMA_16x16x32(qr[ks], kfr[kt][ks], acc, 0, 0, 0);
                    dacc = MC_MFMA_16x16x32(dor[ks], vfr[kt][ks], dacc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) { sv[kt][tt * 4 + r] = acc[r]; dp[kt][tt * 4 + r] = dacc[r]; }
            }
        }
        const int q0 = 32 * I + g * 8;
        float ls[16], dots[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 l4 = *reinterpret_cast<const float4*>(lse_s + 2 * q0 + 4 * i);
            ls[4 * i] = l4.x; ls[4 * i + 1] = l4.y; ls[4 * i + 2] = l4.z; ls[4 * i + 3] = l4.w;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float4 d4 = *reinterpret_cast<const float4*>(dot_s + q0 + 4 * i);
            dots[4 * i] = d4.x; dots[4 * i + 1] = d4.y; dots[4 * i + 2] = d4.z; dots[4 * i + 3] = d4.w;
        }
        bf16x8_t dsf[2], pdf[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const int key = wave * 32 + kt * 16 + li;
            float pdv[8], dsv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                // a query row >= len (zero Q / dO rows in LDS) contributes nothing to dK / dV
                const float v = q0 + i < len ? __expf(sv[kt][i] * a.alpha - ls[2 * i]) * ls[2 * i + 1] : 0.f;
                const float prr = bf2f(f2bf(v));
                float dsc = 1.f;
                if (DROP) dsc = ((dmask[(q0 + i) * 32 + (key >> 3)] >> (key & 7)) & 1) ? invkeep : 0.f;
                pdv[i] = v * dsc;
                dsv[i] = prr * (dp[kt][i] * dsc - dots[i]) * a.alpha;
            }
            pdf[kt] = as_frag(pdv);
            dsf[kt] = as_frag(dsv);
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const bf16x8_t qt = tr_frag(Ks, 32 * I, dt * 16, lane);
            const bf16x8_t dot_f = tr_frag(Vs, 32 * I, dt * 16, lane);
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                dk[kt][dt] = MC_MFMA_16x16x32(qt, dsf[kt], dk[kt][dt], 0, 0, 0);
                dv[kt][dt] = MC_MFMA_16x16x32(dot_f, pdf[kt], dv[kt][dt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = wave * 32 + kt * 16 + li;
        if (key >= len) continue;                      // a column of the accumulators that belongs to no key
        bf16_t* const dst = gbase + (long long)key * ld + g * 4;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            *reinterpret_cast<uint2*>(dst + H + dt * 16) =
                make_uint2(pack_bf2(dk[kt][dt][0], dk[kt][dt][1]), pack_bf2(dk[kt][dt][2], dk[kt][dt][3]));
            *reinterpret_cast<uint2*>(dst + 2 * H + dt * 16) =
                make_uint2(pack_bf2(dv[kt][dt][0], dv[kt][dt][1]), pack_bf2(dv[kt][dt][2], dv[kt][dt][3]));
        }
    }
}

constexpr int fwd_lds(int tl) { return 2 * tl * RS; }
constexpr int bwd_lds(int tl) { return 2 * tl * RS + tl * 4 * 3 + tl * 32; }

int check_shape(int b, int max_len, int t_pad, long long rows, int nh, float p) {
    MC_CHECK(b > 0 && nh > 0 && max_len >= 1 && max_len <= TMAX, "attn_varlen: needs 1 <= max_len <= 256 (head size 64)");
    MC_CHECK(t_pad >= max_len && t_pad % 8 == 0, "attn_varlen: t_pad (the padded layout's T) must be >= max_len and a multiple of 8");
    MC_CHECK(rows >= b && rows <= 0x7fffffffLL, "attn_varlen: bad row count");
    MC_CHECK(p >= 0.f && p < 1.f, "attn_varlen: dropout p out of range");
    return MC_OK;
}

}  // namespace

extern "C" int mc_attn_varlen_supported(int max_len, int head_dim) { return head_dim == HD && max_len >= 1 && max_len <= TMAX; }

extern "C" int mc_attn_varlen_fwd(const mc_bf16* qkv, const int* cu_seqlens, const int* order, int b, int max_len, int t_pad,
                                  long long rows, int nh, float alpha, float p, unsigned long long seed,
                                  unsigned int stream_id, mc_bf16* ctx, float* lse, void* stream) {
    MC_CHECK(qkv && cu_seqlens && ctx && lse, "attn_varlen_fwd: null pointer");
    if (int e = check_shape(b, max_len, t_pad, rows, nh, p)) return e;
    vattn_args a{};
    a.qkv = (const bf16_t*)qkv; a.ctx = (bf16_t*)ctx; a.lse = lse; a.cu = cu_seqlens; a.order = order;
    a.rows = rows; a.nseq = b; a.tl = (max_len + 31) & ~31; a.tpad = t_pad; a.nh = nh;
    a.alpha = alpha; a.p = p; a.seed = seed; a.sid = stream_id;
    static unsigned long long done_t = 0, done_f = 0;
    MC_SET_MAX_LDS(done_t, attn_varlen_fwd_k<true>, fwd_lds(TMAX));
    MC_SET_MAX_LDS(done_f, attn_varlen_fwd_k<false>, fwd_lds(TMAX));
    const int lds = fwd_lds(a.tl);
    if (p > 0.f) hipLaunchKernelGGL(attn_varlen_fwd_k<true>, dim3(b * nh), dim3(512), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(attn_varlen_fwd_k<false>, dim3(b * nh), dim3(512), lds, (hipStream_t)stream, a);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

extern "C" int mc_attn_varlen_bwd(const mc_bf16* qkv, const int* cu_seqlens, const int* order, const mc_bf16* dctx,
                                  const float* lse, int b, int max_len, int t_pad, long long rows, int nh, float alpha,
                                  float p, unsigned long long seed, unsigned int stream_id, mc_bf16* dqkv, void* stream) {
    MC_CHECK(qkv && cu_seqlens && dctx && lse && dqkv, "attn_varlen_bwd: null pointer");
    if (int e = check_shape(b, max_len, t_pad, rows, nh, p)) return e;
    vattn_args a{};
    a.qkv = (const bf16_t*)qkv; a.dctx = (const bf16_t*)dctx; a.dqkv = (bf16_t*)dqkv; a.lse = const_cast<float*>(lse);
    a.cu = cu_seqlens; a.order = order;
    a.rows = rows; a.nseq = b; a.tl = (max_len + 31) & ~31; a.tpad = t_pad; a.nh = nh;
    a.alpha = alpha; a.p = p; a.seed = seed; a.sid = stream_id;
    static unsigned long long done_t = 0, done_f = 0;
    MC_SET_MAX_LDS(done_t, attn_varlen_bwd_k<true>, bwd_lds(TMAX));
    MC_SET_MAX_LDS(done_f, attn_varlen_bwd_k<false>, bwd_lds(TMAX));
    const int lds = bwd_lds(a.tl);
    if (p > 0.f) hipLaunchKernelGGL(attn_varlen_bwd_k<true>, dim3(b * nh), dim3(512), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(attn_varlen_bwd_k<false>, dim3(b * nh), dim3(512), lds, (hipStream_t)stream, a);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
