// Fused BERT self-attention core for gfx950: per (sequence, head)
//     ctx = dropout(softmax(alpha * Q K^T + mask_bias)) V
// forward and backward in one kernel each -- the [b, heads, T, T] score / probability tensors never reach HBM.
// [ref: model/modules/text_encoder.py:47-49 -> transformers BertSelfAttention.forward (scores, mask, softmax, dropout,
//       context); head size 64 (BERT-base)]
// Two pairs of kernels: the RESIDENT pair below for T <= 256 (the reference tokenises to max_length 256) and the LONG pair
// at the end of the file for up to 512 keys (BERT's position table); same contract, views, lse layout and dropout masks.
//
// Resident kernels:
// One 8-wave workgroup per (sequence, head); K and V rows (forward) live in LDS, row-major with a 144-byte stride.
// A wave owns 16 queries at a time and computes S^T = K Q^T on v_mfma_f32_16x16x32_bf16: with the A-operand ROWS of a
// tile pair mapped to keys 32J + (r>>2)*8 + (r&3) (+4), a lane ends up with 8 CONSECUTIVE keys of one query per 32-key
// block J -- exactly the k-slots an MFMA operand fragment holds -- so the probabilities feed P V (and dS feeds dS K)
// straight from registers, the row reductions are in-lane + two cross-lane steps, and one Philox draw covers a lane's
// 8 keys (same (seed, stream, element) function as the unfused softmax kernel: identical dropout masks).
// V^T / K^T / Q^T / dO^T fragments come from the row-major tiles through ds_read_b64_tr_b16.
// Backward: phase A = per-query work in the same layout (recompute P from the saved row max / 1/sum, dP = dO V^T,
// row dots, dQ = dS K; the keep-mask bits and the row dots are parked in LDS); phase B = per-key work in the
// transposed layout (a lane holds 8 consecutive queries of one key): dK = dS^T Q, dV = Pd^T dO with fp32 accumulators
// held by the wave that owns the 32 keys -- no atomics, bit-reproducible.
//
// The kernels are written once and instantiated for two views of the batch, which are also their argument structs:
//   padded_view (mc_attn_*): a [b, T] batch, T % 32 == 0, every sequence owns T rows; the additive key bias of an
//     arbitrary mask is staged in LDS; lse is [b*nh*T][2]; LDS offsets are fixed (TMAX rows).  Every `in_seq` test
//     below is the constant true here.
//   packed_view (mc_attn_varlen_*): the b reports of a call are concatenated into one [R, 3H] row matrix, sequence i
//     owns rows cu_seqlens[i] .. cu_seqlens[i+1]-1 (1 <= len_i <= 256) -- what the padded view computes for a mask
//     1..10..0, without the padded rows [the reference pads every report to max_length 256
//     (data/datasets/imagetext.py:217-222) and masks the padding, so the real tokens see exactly this]:
//   * the key blocks ceil(len / 32) and the query-block loop are per-workgroup values; keys >= len of the last
//     block are masked in registers (score = finfo.min, probability exactly 0), there is no mask_bias array;
//   * staging never reads a row at or beyond cu_seqlens[i+1] (the next sequence's, or past the allocation): LDS rows
//     len .. 32*ceil(len/32)-1 are filled with zeros; lanes of a partial query / key block read the sequence's LAST
//     row instead of their own and do not store;
//   * the dropout element index is the one the padded [b, T] layout uses -- ((i*nh + head)*T + query) * T/8 + key/8 with
//     the caller's padded T -- so one seed drops the same (query, key) pairs as mc_attn_fwd on the padded batch;
//   * lse is [R, nh, 2];
//   * the dynamic LDS is sized by the call's longest sequence (332 bytes per key in the backward: 21 KB at 64 tokens,
//     83 KB at 256), so batches of short reports get more workgroups per CU;
//   * the grid is issued in the order of ``order`` (sequence indices, longest first, optional): a workgroup costs
//     O(len^2), and the long ones should not start last;
//   * rows cu_seqlens[b] .. rows-1 (alignment rows that belong to no sequence) get zeros in ctx / dqkv from the first
//     workgroups of the grid: weight-gradient GEMMs and column sums read them.
#include "common_hip.h"
#include "../../include/mammoclip_hip.h"

namespace {

constexpr int RS = 144;          // LDS row stride (bytes) of a 64-wide bf16 row: +16 B keeps ds_read_b64_tr_b16 conflict-free
constexpr int TMAX = 256;
constexpr int HD = 64;
constexpr float NEG_MAX = -3.4028234663852886e38f;

typedef __attribute__((ext_vector_type(4))) short s4_t;
typedef __attribute__((ext_vector_type(8))) short s8_t;
typedef __attribute__((address_space(3))) s4_t lds_s4_t;

// fragment (index n = col0 + (lane & 15), k = row0 + (lane >> 4) * 8 .. +8) of a row-major [k][n] LDS tile
__device__ __forceinline__ bf16x8_t tr_frag(const unsigned char* tile, int row0, int col0, int lane) {
    const int g = lane >> 4, i = lane & 15;
    const unsigned char* a = tile + (row0 + g * 8 + (i >> 2)) * RS + (col0 + (i & 3) * 4) * 2;
    s4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(a));
    s4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(a + 4 * RS));
    s8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, v);
}
// fragment of the row-major tile whose MFMA row r is tile row base + (r>>2)*8 + (r&3): lanes of a 16-row group end up
// owning rows base + g*8 + (0..3); the caller adds 4 rows for the second tile of the pair
__device__ __forceinline__ bf16x8_t perm_frag(const unsigned char* tile, int base, int ks, int lane) {
    const int g = lane >> 4, i = lane & 15;
    return *reinterpret_cast<const bf16x8_t*>(tile + (base + (i >> 2) * 8 + (i & 3)) * RS + (ks * 32 + g * 8) * 2);
}
__device__ __forceinline__ bf16x8_t as_frag(const float* f) {
    uint4 v = pack8(f);
    return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ float xor_sum16_32(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
// rows [0, len) from global memory; PARTIAL: rows [len, tp) zero (otherwise len == tp)
template <bool PARTIAL>
__device__ __forceinline__ void stage_rows(unsigned char* dst, const bf16_t* src, long long ld, int len, int tp, int tid) {
    for (int idx = tid; idx < tp * 8; idx += 512) {
        const int row = idx >> 3, ch = idx & 7;
        const uint4* const s = reinterpret_cast<const uint4*>(src + (long long)row * ld + ch * 8);
        uint4* const d = reinterpret_cast<uint4*>(dst + row * RS + ch * 16);
        if (!PARTIAL || row < len) *d = *s;
        else *d = make_uint4(0u, 0u, 0u, 0u);
    }
}

// what a workgroup works on: sequence bi, head h (bh = bi*nh + h), rows r0 .. r0+len-1 of the row matrices, tp = len
// rounded up to 32 (the rows the LDS tiles hold)
struct seq_t {
    int bi, h, bh, len, tp;
    long long r0;
};

// A view = the kernels' argument struct + what differs between the two layouts: lds_rows (rows of an LDS tile),
// zero_tail (alignment rows), open (the sequence this workgroup takes; false: nothing to do), stage_bias / bias4 / bias /
// score (the additive key bias and the score it enters), lse_at (row of lse), PARTIAL (a sequence may end inside a
// 32-row block: the kernels then clamp rows, mask keys and predicate stores with `in_seq`).
struct padded_view {
    const bf16_t* qkv;      // [b*t, 3H]: Q | K | V
    const float* maskb;     // [b, t] additive key bias
    const bf16_t* dctx;     // [b*t, H] (backward)
    bf16_t* ctx;            // [b*t, H] (forward)
    bf16_t* dqkv;           // [b*t, 3H] (backward)
    float* lse;             // [b*nh*t][2]: row max, 1 / row sum
    int t, nh;
    float alpha, p;
    unsigned long long seed;
    unsigned int sid;

    static constexpr bool PARTIAL = false;      // a sequence never ends inside a 32-row block
    static constexpr int BIAS_ROWS = TMAX;      // floats of LDS for the key bias
    __host__ __device__ int lds_rows() const { return TMAX; }
    __device__ void zero_tail(bf16_t*, int, int) const {}
    __device__ bool open(seq_t& s) const {
        s.bh = blockIdx.x;
        s.bi = s.bh / nh; s.h = s.bh % nh; s.len = s.tp = t;
        s.r0 = (long long)s.bi * t;
        return true;
    }
    __device__ void stage_bias(float* mb, const seq_t& s, int k) const { mb[k] = maskb[s.r0 + k]; }
    __device__ float4 bias4(const float* mb, int key0) const { return *reinterpret_cast<const float4*>(mb + key0); }
    __device__ float bias(const float* mb, int key) const { return mb[key]; }
    __device__ float score(float qk, float bias) const { return qk * alpha + bias; }
    __device__ float* lse_at(const seq_t& s, int q) const { return lse + ((long long)s.bh * t + q) * 2; }
};

struct packed_view {
    const bf16_t* qkv;      // [rows, 3H]: Q | K | V
    const bf16_t* dctx;     // [rows, H] (backward)
    bf16_t* ctx;            // [rows, H] (forward)
    bf16_t* dqkv;           // [rows, 3H] (backward)
    float* lse;             // [rows, nh][2]: row max, 1 / row sum
    const int* cu;          // [nseq + 1]
    const int* order;       // [nseq] or null
    long long rows;
    int nseq, tl, t, nh;    // tl: LDS rows (longest sequence rounded up to 32); t: T of the padded layout (dropout index)
    float alpha, p;
    unsigned long long seed;
    unsigned int sid;

    static constexpr bool PARTIAL = true;
    static constexpr int BIAS_ROWS = 0;
    __host__ __device__ int lds_rows() const { return tl; }
    // the first nh workgroups of the grid (one per head): zeros in the head's 64 columns of the alignment rows of m
    // (leading dimension ld)
    __device__ void zero_tail(bf16_t* m, int ld, int tid) const {
        if (blockIdx.x >= (unsigned)nh) return;
        const long long r_begin = cu[nseq];
        if (r_begin < 0) return;
        for (long long idx = tid; idx < (rows - r_begin) * 8; idx += 512)
            *reinterpret_cast<uint4*>(m + (r_begin + (idx >> 3)) * (long long)ld + blockIdx.x * HD + (idx & 7) * 8) = make_uint4(0u, 0u, 0u, 0u);
    }
    __device__ bool open(seq_t& s) const {
        const int oi = blockIdx.x / nh;
        s.h = blockIdx.x % nh;
        s.bi = order ? order[oi] : oi;
        if (s.bi < 0 || s.bi >= nseq) return false;
        const int r0 = cu[s.bi];
        s.len = cu[s.bi + 1] - r0;
        if (s.len < 1 || s.len > tl || r0 < 0 || r0 + s.len > rows) return false;      // malformed cu_seqlens: touch nothing
        s.tp = (s.len + 31) & ~31;
        s.r0 = r0; s.bh = s.bi * nh + s.h;
        return true;
    }
    __device__ void stage_bias(float*, const seq_t&, int) const {}
    __device__ float4 bias4(const float*, int) const { return make_float4(0.f, 0.f, 0.f, 0.f); }
    __device__ float bias(const float*, int) const { return 0.f; }
    __device__ float score(float qk, float) const { return qk * alpha; }
    __device__ float* lse_at(const seq_t& s, int q) const { return lse + ((s.r0 + q) * nh + s.h) * 2; }
};

template <class V, bool DROP>
__global__ __launch_bounds__(512) void attn_fwd_k(V a) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* const Ks = smem;
    unsigned char* const Vs = smem + a.lds_rows() * RS;
    float* const mb = reinterpret_cast<float*>(smem + 2 * a.lds_rows() * RS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const int nh = a.nh, H = nh * HD, ld = 3 * H;
    a.zero_tail(a.ctx, H, tid);
    seq_t sq;
    if (!a.open(sq)) return;
    const int h = sq.h, len = sq.len;
    const auto in_seq = [len](int r) { return !V::PARTIAL || r < len; };
    const bf16_t* const base = a.qkv + sq.r0 * ld + h * HD;
    stage_rows<V::PARTIAL>(Ks, base + H, ld, len, sq.tp, tid);
    stage_rows<V::PARTIAL>(Vs, base + 2 * H, ld, len, sq.tp, tid);
    for (int k = tid; k < sq.tp; k += 512) a.stage_bias(mb, sq, k);
    __syncthreads();
    const int nJ = sq.tp >> 5;
    for (int qb = wave; qb * 16 < len; qb += 8) {
        const int q = qb * 16 + li, qc = in_seq(q) ? q : len - 1;
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
                    const float4 bv = a.bias4(mb, key);
                    s[J][tt * 4 + 0] = in_seq(key + 0) ? a.score(acc[0], bv.x) : NEG_MAX;
                    s[J][tt * 4 + 1] = in_seq(key + 1) ? a.score(acc[1], bv.y) : NEG_MAX;
                    s[J][tt * 4 + 2] = in_seq(key + 2) ? a.score(acc[2], bv.z) : NEG_MAX;
                    s[J][tt * 4 + 3] = in_seq(key + 3) ? a.score(acc[3], bv.w) : NEG_MAX;
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
        const long long prow = (long long)sq.bh * a.t + qc;      // row of the padded [b, nh, T, T] probabilities
        if (g == 0 && in_seq(q)) *reinterpret_cast<float2*>(a.lse_at(sq, q)) = make_float2(mx, inv);
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
                    dropout_scale8(a.seed, a.sid, (unsigned long long)prow * (a.t >> 3) + 4 * J + g, a.p, ds);
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] *= ds[i];
                }
                const bf16x8_t pf = as_frag(v);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    o[dt] = MC_MFMA_16x16x32(tr_frag(Vs, 32 * J, dt * 16, lane), pf, o[dt], 0, 0, 0);
            }
        }
        if (in_seq(q)) {
            bf16_t* const dst = a.ctx + (sq.r0 + q) * H + h * HD + g * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<uint2*>(dst + dt * 16) = make_uint2(pack_bf2(o[dt][0], o[dt][1]), pack_bf2(o[dt][2], o[dt][3]));
        }
    }
}

template <class V, bool DROP>
__global__ __launch_bounds__(512) void attn_bwd_k(V a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tl = a.lds_rows();
    unsigned char* const Ks = smem;                    // phase A: K rows, phase B: Q rows
    unsigned char* const Vs = smem + tl * RS;          // phase A: V rows, phase B: dO rows
    float* const mb = reinterpret_cast<float*>(smem + 2 * tl * RS);
    float* const lse_s = mb + V::BIAS_ROWS;            // [tl][2]
    float* const dot_s = lse_s + 2 * tl;               // [tl]
    unsigned char* const dmask = reinterpret_cast<unsigned char*>(dot_s + tl);     // [tl][32] keep bits, 8 keys per byte
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const int nh = a.nh, H = nh * HD, ld = 3 * H;
#pragma unroll
    for (int part = 0; part < 3; ++part) a.zero_tail(a.dqkv + part * H, ld, tid);
    seq_t sq;
    if (!a.open(sq)) return;
    const int h = sq.h, len = sq.len;
    const auto in_seq = [len](int r) { return !V::PARTIAL || r < len; };
    const bf16_t* const base = a.qkv + sq.r0 * ld + h * HD;
    const bf16_t* const dbase = a.dctx + sq.r0 * H + h * HD;
    bf16_t* const gbase = a.dqkv + sq.r0 * ld + h * HD;
    stage_rows<V::PARTIAL>(Ks, base + H, ld, len, sq.tp, tid);
    stage_rows<V::PARTIAL>(Vs, base + 2 * H, ld, len, sq.tp, tid);
    for (int k = tid; k < sq.tp; k += 512) {
        a.stage_bias(mb, sq, k);
        float2 l2 = make_float2(0.f, 0.f);
        if (in_seq(k)) l2 = *reinterpret_cast<const float2*>(a.lse_at(sq, k));
        *reinterpret_cast<float2*>(lse_s + 2 * k) = l2;
        if (V::PARTIAL) dot_s[k] = 0.f;                // phase A writes only the rows < len
    }
    __syncthreads();
    const int nJ = sq.tp >> 5;
    const float invkeep = 1.f / (1.f - a.p);
    // ---------------- phase A: a lane = one query x 8 consecutive keys per 32-key block
    for (int qb = wave; qb * 16 < len; qb += 8) {
        const int q = qb * 16 + li, qc = in_seq(q) ? q : len - 1;
        bf16x8_t qf[2], dof[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[ks] = *reinterpret_cast<const bf16x8_t*>(base + (long long)qc * ld + ks * 32 + g * 8);
            dof[ks] = *reinterpret_cast<const bf16x8_t*>(dbase + (long long)qc * H + ks * 32 + g * 8);
        }
        const float mx = lse_s[2 * qc], inv = lse_s[2 * qc + 1];
        const long long prow = (long long)sq.bh * a.t + qc;      // row of the padded [b, nh, T, T] probabilities
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
                    const float4 bv = a.bias4(mb, key);
                    const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = in_seq(key + r) ? __expf(a.score(acc[r], bb[r]) - mx) * inv : 0.f;
                        pr[J][tt * 4 + r] = bf2f(f2bf(v));
                        d[J][tt * 4 + r] = dacc[r];
                    }
                }
                if (DROP) {
                    float ds[8];
                    dropout_scale8(a.seed, a.sid, (unsigned long long)prow * (a.t >> 3) + 4 * J + g, a.p, ds);
                    unsigned int bits = 0;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        d[J][i] *= ds[i];
                        bits |= (ds[i] != 0.f ? 1u : 0u) << i;
                    }
                    if (in_seq(q)) dmask[q * 32 + 4 * J + g] = (unsigned char)bits;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) dot += pr[J][i] * d[J][i];
            }
        }
        dot = xor_sum16_32(dot);
        if (g == 0 && in_seq(q)) dot_s[q] = dot;
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
        if (in_seq(q)) {
            bf16_t* const dst = gbase + (long long)q * ld + g * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<uint2*>(dst + dt * 16) = make_uint2(pack_bf2(dq[dt][0], dq[dt][1]), pack_bf2(dq[dt][2], dq[dt][3]));
        }
    }
    __syncthreads();
    // ---------------- phase B: a lane = one key x 8 consecutive queries per 32-query block; a wave owns 32 keys
    stage_rows<V::PARTIAL>(Ks, base, ld, len, sq.tp, tid);          // Q rows
    stage_rows<V::PARTIAL>(Vs, dbase, H, len, sq.tp, tid);          // dO rows
    __syncthreads();
    if (wave * 32 >= len) return;
    bf16x8_t kfr[2][2], vfr[2][2];
    float mbk[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = wave * 32 + kt * 16 + li, kc = in_seq(key) ? key : len - 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kfr[kt][ks] = *reinterpret_cast<const bf16x8_t*>(base + H + (long long)kc * ld + ks * 32 + g * 8);
            vfr[kt][ks] = *reinterpret_cast<const bf16x8_t*>(base + 2 * H + (long long)kc * ld + ks * 32 + g * 8);
        }
        mbk[kt] = a.bias(mb, key);
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
                const float v = in_seq(q0 + i) ? __expf(a.score(sv[kt][i], mbk[kt]) - ls[2 * i]) * ls[2 * i + 1] : 0.f;
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
        if (!in_seq(key)) continue;                    // a column of the accumulators that belongs to no key
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

// dynamic LDS of a workgroup whose tiles hold tl rows: K/V tiles, the view's key bias, backward: lse, row dots, keep bits
template <class V, bool BWD>
constexpr int lds_bytes(int tl) { return 2 * tl * RS + V::BIAS_ROWS * 4 + (BWD ? tl * 4 * 3 + tl * 32 : 0); }

// one workgroup per (sequence, head), with or without dropout
template <class V, bool BWD>
int launch(const V& a, int nseq, void* stream) {
    constexpr auto drop = BWD ? attn_bwd_k<V, true> : attn_fwd_k<V, true>;
    constexpr auto nodrop = BWD ? attn_bwd_k<V, false> : attn_fwd_k<V, false>;
    static unsigned long long done_t = 0, done_f = 0;
    MC_SET_MAX_LDS(done_t, drop, (lds_bytes<V, BWD>(TMAX)));
    MC_SET_MAX_LDS(done_f, nodrop, (lds_bytes<V, BWD>(TMAX)));
    hipLaunchKernelGGL(a.p > 0.f ? drop : nodrop, dim3(nseq * a.nh), dim3(512), (lds_bytes<V, BWD>(a.lds_rows())), (hipStream_t)stream, a);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int check_shape(int b, int t, int nh, float p) {
    MC_CHECK(b > 0 && nh > 0 && t >= 32 && t <= TMAX && t % 32 == 0, "attn: needs 32 <= t <= 256, t % 32 == 0 (head size 64)");
    MC_CHECK(p >= 0.f && p < 1.f, "attn: dropout p out of range");
    return MC_OK;
}

int check_shape_varlen(int b, int max_len, int t_pad, long long rows, int nh, float p) {
    MC_CHECK(b > 0 && nh > 0 && max_len >= 1 && max_len <= TMAX, "attn_varlen: needs 1 <= max_len <= 256 (head size 64)");
    MC_CHECK(t_pad >= max_len && t_pad % 8 == 0, "attn_varlen: t_pad (the padded layout's T) must be >= max_len and a multiple of 8");
    MC_CHECK(rows >= b && rows <= 0x7fffffffLL, "attn_varlen: bad row count");
    MC_CHECK(p >= 0.f && p < 1.f, "attn_varlen: dropout p out of range");
    return MC_OK;
}

}  // namespace

extern "C" int mc_attn_supported(int t, int head_dim) { return head_dim == HD && t >= 32 && t <= TMAX && t % 32 == 0; }

extern "C" int mc_attn_fwd(const mc_bf16* qkv, const float* mask_bias, int b, int t, int nh, float alpha, float p,
                           unsigned long long seed, unsigned int stream_id, mc_bf16* ctx, float* lse, void* stream) {
    MC_CHECK(qkv && mask_bias && ctx && lse, "attn_fwd: null pointer");
    if (int e = check_shape(b, t, nh, p)) return e;
    padded_view a{};
    a.qkv = (const bf16_t*)qkv; a.maskb = mask_bias; a.ctx = (bf16_t*)ctx; a.lse = lse;
    a.t = t; a.nh = nh; a.alpha = alpha; a.p = p; a.seed = seed; a.sid = stream_id;
    return launch<padded_view, false>(a, b, stream);
}

extern "C" int mc_attn_bwd(const mc_bf16* qkv, const float* mask_bias, const mc_bf16* dctx, const float* lse, int b, int t,
                           int nh, float alpha, float p, unsigned long long seed, unsigned int stream_id, mc_bf16* dqkv,
                           void* stream) {
    MC_CHECK(qkv && mask_bias && dctx && lse && dqkv, "attn_bwd: null pointer");
    if (int e = check_shape(b, t, nh, p)) return e;
    padded_view a{};
    a.qkv = (const bf16_t*)qkv; a.maskb = mask_bias; a.dctx = (const bf16_t*)dctx; a.dqkv = (bf16_t*)dqkv;
    a.lse = const_cast<float*>(lse);
    a.t = t; a.nh = nh; a.alpha = alpha; a.p = p; a.seed = seed; a.sid = stream_id;
    return launch<padded_view, true>(a, b, stream);
}

extern "C" int mc_attn_varlen_supported(int max_len, int head_dim) { return head_dim == HD && max_len >= 1 && max_len <= TMAX; }

extern "C" int mc_attn_varlen_fwd(const mc_bf16* qkv, const int* cu_seqlens, const int* order, int b, int max_len, int t_pad,
                                  long long rows, int nh, float alpha, float p, unsigned long long seed,
                                  unsigned int stream_id, mc_bf16* ctx, float* lse, void* stream) {
    MC_CHECK(qkv && cu_seqlens && ctx && lse, "attn_varlen_fwd: null pointer");
    if (int e = check_shape_varlen(b, max_len, t_pad, rows, nh, p)) return e;
    packed_view a{};
    a.qkv = (const bf16_t*)qkv; a.ctx = (bf16_t*)ctx; a.lse = lse; a.cu = cu_seqlens; a.order = order;
    a.rows = rows; a.nseq = b; a.tl = (max_len + 31) & ~31; a.t = t_pad; a.nh = nh;
    a.alpha = alpha; a.p = p; a.seed = seed; a.sid = stream_id;
    return launch<packed_view, false>(a, b, stream);
}

extern "C" int mc_attn_varlen_bwd(const mc_bf16* qkv, const int* cu_seqlens, const int* order, const mc_bf16* dctx,
                                  const float* lse, int b, int max_len, int t_pad, long long rows, int nh, float alpha,
                                  float p, unsigned long long seed, unsigned int stream_id, mc_bf16* dqkv, void* stream) {
    MC_CHECK(qkv && cu_seqlens && dctx && lse && dqkv, "attn_varlen_bwd: null pointer");
    if (int e = check_shape_varlen(b, max_len, t_pad, rows, nh, p)) return e;
    packed_view a{};
    a.qkv = (const bf16_t*)qkv; a.dctx = (const bf16_t*)dctx; a.dqkv = (bf16_t*)dqkv; a.lse = const_cast<float*>(lse);
    a.cu = cu_seqlens; a.order = order;
    a.rows = rows; a.nseq = b; a.tl = (max_len + 31) & ~31; a.t = t_pad; a.nh = nh;
    a.alpha = alpha; a.p = p; a.seed = seed; a.sid = stream_id;
    return launch<packed_view, true>(a, b, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Long kernels (mc_attn_long_* / mc_attn_varlen_long_*): the same contract for up to 512 keys, on the same two views.
// The resident bodies above keep a query block's scores of ALL keys in registers (8 blocks x 8 floats), their backward
// keeps both 256-row tiles next to [T][32] keep bits (188 KB at 512 rows) and gives each of the 8 waves 32 keys; here
//   forward:  K and V are whole in LDS (2 * 512 * 144 B + bias = 149,504 B), 16 key blocks of scores per lane (one
//     workgroup per CU = two waves per SIMD, 256 VGPRs each); otherwise the resident forward, statement for statement;
//   backward: the small per-row arrays are full length (bias, lse, row dots, keep bits at T/8 bytes per query), the two
//     tiles hold 256 rows and are restaged per 256-row chunk of the other dimension (114,688 B at 512 rows).
//     dS needs a query's row dot sum_j P_ij dPd_ij BEFORE its first key, so phase A sweeps the key chunks twice (row
//     dots and dropout bits, then dS and dQ) and stores no scores: a wave keeps the dQ accumulators of its (up to 4)
//     query blocks across the key chunks and consumes a 32-key block at once.  [dO_i . ctx_i is the same dot up to the
//     16-bit rounding of ctx and would save the first sweep, but moves dS by an ulp in ~10 % of its elements: measured
//     against the resident kernels, dQ / dK then differ by one 16-bit ulp near max|dQ|, 6.3e-3 .. 7.4e-3 of it.]
//     Phase B does the 256-key halves in turn (a wave owns 32 keys of the half), sweeping the query chunks for each.
// lds_rows() of a view describes the resident layout and is not used here: tiles and per-row arrays are sized by
// long_rows(); BIAS_ROWS only tells whether the view stages a key bias.
namespace {

constexpr int TLONG = 512;
constexpr int CH = 256;          // rows of a restaged backward tile
constexpr int NJL = TLONG / 32;  // key blocks of the forward

__host__ __device__ inline int long_rows(const padded_view& a) { return a.t; }
__host__ __device__ inline int long_rows(const packed_view& a) { return a.tl; }
template <class V> constexpr bool has_bias() { return V::BIAS_ROWS != 0; }

template <class V, bool DROP>
__global__ __launch_bounds__(512) void attn_long_fwd_k(V a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tl = long_rows(a);
    unsigned char* const Ks = smem;
    unsigned char* const Vs = smem + tl * RS;
    float* const mb = reinterpret_cast<float*>(smem + 2 * tl * RS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const int nh = a.nh, H = nh * HD, ld = 3 * H;
    a.zero_tail(a.ctx, H, tid);
    seq_t sq;
    if (!a.open(sq)) return;
    const int h = sq.h, len = sq.len;
    const auto in_seq = [len](int r) { return !V::PARTIAL || r < len; };
    const bf16_t* const base = a.qkv + sq.r0 * ld + h * HD;
    stage_rows<V::PARTIAL>(Ks, base + H, ld, len, sq.tp, tid);
    stage_rows<V::PARTIAL>(Vs, base + 2 * H, ld, len, sq.tp, tid);
    for (int k = tid; k < sq.tp; k += 512) a.stage_bias(mb, sq, k);
    __syncthreads();
    const int nJ = sq.tp >> 5;
    for (int qb = wave; qb * 16 < len; qb += 8) {
        const int q = qb * 16 + li, qc = in_seq(q) ? q : len - 1;
        bf16x8_t qf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            qf[ks] = *reinterpret_cast<const bf16x8_t*>(base + (long long)qc * ld + ks * 32 + g * 8);
        float s[NJL][8];
        float mx = NEG_MAX;
#pragma unroll
        for (int J = 0; J < NJL; ++J) {
            if (J < nJ) {
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks)
                        acc = MC_MFMA_16x16x32(perm_frag(Ks, 32 * J + 4 * tt, ks, lane), qf[ks], acc, 0, 0, 0);
                    const int key = 32 * J + g * 8 + 4 * tt;
                    const float4 bv = a.bias4(mb, key);
                    s[J][tt * 4 + 0] = in_seq(key + 0) ? a.score(acc[0], bv.x) : NEG_MAX;
                    s[J][tt * 4 + 1] = in_seq(key + 1) ? a.score(acc[1], bv.y) : NEG_MAX;
                    s[J][tt * 4 + 2] = in_seq(key + 2) ? a.score(acc[2], bv.z) : NEG_MAX;
                    s[J][tt * 4 + 3] = in_seq(key + 3) ? a.score(acc[3], bv.w) : NEG_MAX;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) mx = fmaxf(mx, s[J][i]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int J = 0; J < NJL; ++J)
            if (J < nJ)
#pragma unroll
                for (int i = 0; i < 8; ++i) { s[J][i] = __expf(s[J][i] - mx); sum += s[J][i]; }
        const float inv = 1.f / xor_sum16_32(sum);
        const long long prow = (long long)sq.bh * a.t + qc;      // row of the padded [b, nh, T, T] probabilities
        if (g == 0 && in_seq(q)) *reinterpret_cast<float2*>(a.lse_at(sq, q)) = make_float2(mx, inv);
        f32x4_t o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int J = 0; J < NJL; ++J) {
            if (J < nJ) {
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = s[J][i] * inv;
                if (DROP) {
                    float ds[8];
                    dropout_scale8(a.seed, a.sid, (unsigned long long)prow * (a.t >> 3) + 4 * J + g, a.p, ds);
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] *= ds[i];
                }
                const bf16x8_t pf = as_frag(v);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    o[dt] = MC_MFMA_16x16x32(tr_frag(Vs, 32 * J, dt * 16, lane), pf, o[dt], 0, 0, 0);
            }
        }
        if (in_seq(q)) {
            bf16_t* const dst = a.ctx + (sq.r0 + q) * H + h * HD + g * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<uint2*>(dst + dt * 16) = make_uint2(pack_bf2(o[dt][0], o[dt][1]), pack_bf2(o[dt][2], o[dt][3]));
        }
    }
}

template <class V, bool DROP>
__global__ __launch_bounds__(512) void attn_long_bwd_k(V a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tl = long_rows(a), tr = tl < CH ? tl : CH;        // rows of the per-row arrays / of a tile
    unsigned char* const Ks = smem;                    // phase A: a K chunk, phase B: a Q chunk
    unsigned char* const Vs = smem + tr * RS;          // phase A: a V chunk, phase B: a dO chunk
    float* const mb = reinterpret_cast<float*>(smem + 2 * tr * RS);        // [tl] (padded view)
    float* const lse_s = mb + (has_bias<V>() ? tl : 0);                    // [tl][2]
    float* const dot_s = lse_s + 2 * tl;                                   // [tl]
    unsigned char* const dmask = reinterpret_cast<unsigned char*>(dot_s + tl);     // [tl][tl/8] keep bits, 8 keys per byte
    const int ms = tl >> 3;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const int nh = a.nh, H = nh * HD, ld = 3 * H;
#pragma unroll
    for (int part = 0; part < 3; ++part) a.zero_tail(a.dqkv + part * H, ld, tid);
    seq_t sq;
    if (!a.open(sq)) return;
    const int h = sq.h, len = sq.len;
    const auto in_seq = [len](int r) { return !V::PARTIAL || r < len; };
    const bf16_t* const base = a.qkv + sq.r0 * ld + h * HD;
    const bf16_t* const dbase = a.dctx + sq.r0 * H + h * HD;
    bf16_t* const gbase = a.dqkv + sq.r0 * ld + h * HD;
    for (int k = tid; k < sq.tp; k += 512) {
        a.stage_bias(mb, sq, k);
        float2 l2 = make_float2(0.f, 0.f);
        if (in_seq(k)) l2 = *reinterpret_cast<const float2*>(a.lse_at(sq, k));
        *reinterpret_cast<float2*>(lse_s + 2 * k) = l2;
        if (V::PARTIAL) dot_s[k] = 0.f;                // phase A writes only the rows < len
    }
    const int nC = (sq.tp + CH - 1) / CH;              // 256-row chunks of the sequence
    const float invkeep = 1.f / (1.f - a.p);
    // ---------------- phase A: a lane = one query x 8 consecutive keys of a 32-key block; a wave owns query blocks
    // wave, wave + 8, wave + 16, wave + 24.  Two sweeps over the key chunks: the first draws the dropout bits and sums the row
    // dots sum_j P_ij dPd_ij (the resident kernel's expression, in its order), the second forms dS and keeps dQ over the
    // chunks.  The second sweep walks the chunks backwards: the last chunk of the first sweep is still staged.
    float dot[4] = {0.f, 0.f, 0.f, 0.f};
    f32x4_t dq[4][4];
#pragma unroll
    for (int qi = 0; qi < 4; ++qi)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[qi][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int step = 0; step < 2 * nC; ++step) {
        const bool second = step >= nC;
        const int c = second ? 2 * nC - 1 - step : step;
        const int rows_c = sq.tp - c * CH < CH ? sq.tp - c * CH : CH;
        if (step != nC) {                              // (the first chunk of the second sweep is the staged one)
            if (step) __syncthreads();                 // every wave is done with the previous chunk
            stage_rows<V::PARTIAL>(Ks, base + H + (long long)c * CH * ld, ld, len - c * CH, rows_c, tid);
            stage_rows<V::PARTIAL>(Vs, base + 2 * H + (long long)c * CH * ld, ld, len - c * CH, rows_c, tid);
            __syncthreads();
        } else {
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) {
                const int q = (wave + 8 * qi) * 16 + li;
                dot[qi] = xor_sum16_32(dot[qi]);
                if (g == 0 && q < len) dot_s[q] = dot[qi];
            }
        }
        const int nJc = rows_c >> 5;
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) {
            const int qb = wave + 8 * qi;
            if (qb * 16 < len) {
                const int q = qb * 16 + li, qc = in_seq(q) ? q : len - 1;
                bf16x8_t qf[2], dof[2];
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    qf[ks] = *reinterpret_cast<const bf16x8_t*>(base + (long long)qc * ld + ks * 32 + g * 8);
                    dof[ks] = *reinterpret_cast<const bf16x8_t*>(dbase + (long long)qc * H + ks * 32 + g * 8);
                }
                const float mx = lse_s[2 * qc], inv = lse_s[2 * qc + 1];
                const long long prow = (long long)sq.bh * a.t + qc;      // row of the padded [b, nh, T, T] probabilities
                for (int Jl = 0; Jl < nJc; ++Jl) {
                    const int J = c * (CH / 32) + Jl;
                    float pr[8], d[8];
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) {
                        f32x4_t acc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks) {
                            acc = MC_MFMA_16x16x32(perm_frag(Ks, 32 * Jl + 4 * tt, ks, lane), qf[ks], acc, 0, 0, 0);
                            dacc = MC_MFMA_16x16x32(perm_frag(Vs, 32 * Jl + 4 * tt, ks, lane), dof[ks], dacc, 0, 0, 0);
                        }
                        const int key = 32 * J + g * 8 + 4 * tt;
                        const float4 bv = a.bias4(mb, key);
                        const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float v = in_seq(key + r) ? __expf(a.score(acc[r], bb[r]) - mx) * inv : 0.f;
                            pr[tt * 4 + r] = bf2f(f2bf(v));
                            d[tt * 4 + r] = dacc[r];
                        }
                    }
                    if (!second) {
                        if (DROP) {
                            float ds[8];
                            dropout_scale8(a.seed, a.sid, (unsigned long long)prow * (a.t >> 3) + 4 * J + g, a.p, ds);
                            unsigned int bits = 0;
#pragma unroll
                            for (int i = 0; i < 8; ++i) {
                                d[i] *= ds[i];
                                bits |= (ds[i] != 0.f ? 1u : 0u) << i;
                            }
                            if (in_seq(q)) dmask[q * ms + 4 * J + g] = (unsigned char)bits;
                        }
#pragma unroll
                        for (int i = 0; i < 8; ++i) dot[qi] += pr[i] * d[i];
                    } else {
                        if (DROP) {
                            const unsigned int bits = dmask[qc * ms + 4 * J + g];  // written by this wave in the first sweep
#pragma unroll
                            for (int i = 0; i < 8; ++i) d[i] *= ((bits >> i) & 1) ? invkeep : 0.f;
                        }
                        float dsv[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i) dsv[i] = pr[i] * (d[i] - dot[qi]) * a.alpha;
                        const bf16x8_t dsf = as_frag(dsv);
#pragma unroll
                        for (int dt = 0; dt < 4; ++dt)
                            dq[qi][dt] = MC_MFMA_16x16x32(tr_frag(Ks, 32 * Jl, dt * 16, lane), dsf, dq[qi][dt], 0, 0, 0);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
        const int q = (wave + 8 * qi) * 16 + li;
        if (q < len) {
            bf16_t* const dst = gbase + (long long)q * ld + g * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<uint2*>(dst + dt * 16) =
                    make_uint2(pack_bf2(dq[qi][dt][0], dq[qi][dt][1]), pack_bf2(dq[qi][dt][2], dq[qi][dt][3]));
        }
    }
    // ---------------- phase B: a lane = one key x 8 consecutive queries per 32-query block; the 256-key halves in turn,
    // a wave owns 32 keys of the half and sweeps the query chunks
    for (int kh = 0; kh < nC; ++kh) {
        const int k0 = kh * CH + wave * 32;
        const bool act = k0 < len;                     // wave-uniform; the barriers below are outside of it
        bf16x8_t kfr[2][2] = {}, vfr[2][2] = {};
        float mbk[2] = {0.f, 0.f};
        if (act) {
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                const int key = k0 + kt * 16 + li, kc = in_seq(key) ? key : len - 1;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    kfr[kt][ks] = *reinterpret_cast<const bf16x8_t*>(base + H + (long long)kc * ld + ks * 32 + g * 8);
                    vfr[kt][ks] = *reinterpret_cast<const bf16x8_t*>(base + 2 * H + (long long)kc * ld + ks * 32 + g * 8);
                }
                mbk[kt] = a.bias(mb, key);
            }
        }
        f32x4_t dk[2][4], dv[2][4];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) { dk[kt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; dv[kt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
        for (int c = 0; c < nC; ++c) {
            const int rows_c = sq.tp - c * CH < CH ? sq.tp - c * CH : CH;
            __syncthreads();                           // every wave is done with the tiles (phase A, or the previous chunk)
            stage_rows<V::PARTIAL>(Ks, base + (long long)c * CH * ld, ld, len - c * CH, rows_c, tid);       // Q rows
            stage_rows<V::PARTIAL>(Vs, dbase + (long long)c * CH * H, H, len - c * CH, rows_c, tid);        // dO rows
            __syncthreads();
            if (!act) continue;
            for (int Il = 0; Il < (rows_c >> 5); ++Il) {
                float sv[2][8], dp[2][8];
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    bf16x8_t qr[2], dor[2];
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        qr[ks] = perm_frag(Ks, 32 * Il + 4 * tt, ks, lane);
                        dor[ks] = perm_frag(Vs, 32 * Il + 4 * tt, ks, lane);
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
                const int q0 = c * CH + 32 * Il + g * 8;
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
                    const int key = k0 + kt * 16 + li;
                    float pdv[8], dsv[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        // a query row >= len (zero Q / dO rows in LDS) contributes nothing to dK / dV
                        const float v = in_seq(q0 + i) ? __expf(a.score(sv[kt][i], mbk[kt]) - ls[2 * i]) * ls[2 * i + 1] : 0.f;
                        const float prr = bf2f(f2bf(v));
                        float dsc = 1.f;
                        if (DROP) dsc = ((dmask[(q0 + i) * ms + (key >> 3)] >> (key & 7)) & 1) ? invkeep : 0.f;
                        pdv[i] = v * dsc;
                        dsv[i] = prr * (dp[kt][i] * dsc - dots[i]) * a.alpha;
                    }
                    pdf[kt] = as_frag(pdv);
                    dsf[kt] = as_frag(dsv);
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const bf16x8_t qt = tr_frag(Ks, 32 * Il, dt * 16, lane);
                    const bf16x8_t dot_f = tr_frag(Vs, 32 * Il, dt * 16, lane);
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt) {
                        dk[kt][dt] = MC_MFMA_16x16x32(qt, dsf[kt], dk[kt][dt], 0, 0, 0);
                        dv[kt][dt] = MC_MFMA_16x16x32(dot_f, pdf[kt], dv[kt][dt], 0, 0, 0);
                    }
                }
            }
        }
        if (!act) continue;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const int key = k0 + kt * 16 + li;
            if (!in_seq(key)) continue;                // a column of the accumulators that belongs to no key
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
}

// dynamic LDS of a long workgroup whose sequences have up to tl rows (a multiple of 32)
template <class V, bool BWD>
constexpr int lds_long_bytes(int tl) {
    const int bias = has_bias<V>() ? tl * 4 : 0;
    return BWD ? 2 * (tl < CH ? tl : CH) * RS + bias + tl * 4 * 3 + tl * (tl >> 3) : 2 * tl * RS + bias;
}
static_assert(lds_long_bytes<padded_view, false>(TLONG) <= 163840 && lds_long_bytes<padded_view, true>(TLONG) <= 163840,
              "long attention: a workgroup's LDS must fit the CU's 160 KB");

template <class V, bool BWD>
int launch_long(const V& a, int nseq, void* stream) {
    constexpr auto drop = BWD ? attn_long_bwd_k<V, true> : attn_long_fwd_k<V, true>;
    constexpr auto nodrop = BWD ? attn_long_bwd_k<V, false> : attn_long_fwd_k<V, false>;
    static unsigned long long done_t = 0, done_f = 0;
    MC_SET_MAX_LDS(done_t, drop, (lds_long_bytes<V, BWD>(TLONG)));
    MC_SET_MAX_LDS(done_f, nodrop, (lds_long_bytes<V, BWD>(TLONG)));
    hipLaunchKernelGGL(a.p > 0.f ? drop : nodrop, dim3(nseq * a.nh), dim3(512), (lds_long_bytes<V, BWD>(long_rows(a))),
                       (hipStream_t)stream, a);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int check_shape_long(int b, int t, int nh, float p) {
    MC_CHECK(b > 0 && nh > 0 && t >= 32 && t <= TLONG && t % 32 == 0, "attn_long: needs 32 <= t <= 512, t % 32 == 0 (head size 64)");
    MC_CHECK(p >= 0.f && p < 1.f, "attn_long: dropout p out of range");
    return MC_OK;
}

int check_shape_varlen_long(int b, int max_len, int t_pad, long long rows, int nh, float p) {
    MC_CHECK(b > 0 && nh > 0 && max_len >= 1 && max_len <= TLONG, "attn_varlen_long: needs 1 <= max_len <= 512 (head size 64)");
    MC_CHECK(t_pad >= max_len && t_pad % 8 == 0, "attn_varlen_long: t_pad (the padded layout's T) must be >= max_len and a multiple of 8");
    MC_CHECK(rows >= b && rows <= 0x7fffffffLL, "attn_varlen_long: bad row count");
    MC_CHECK(p >= 0.f && p < 1.f, "attn_varlen_long: dropout p out of range");
    return MC_OK;
}

}  // namespace

extern "C" int mc_attn_long_supported(int t, int head_dim) { return head_dim == HD && t >= 32 && t <= TLONG && t % 32 == 0; }

extern "C" int mc_attn_long_fwd(const mc_bf16* qkv, const float* mask_bias, int b, int t, int nh, float alpha, float p,
                                unsigned long long seed, unsigned int stream_id, mc_bf16* ctx, float* lse, void* stream) {
    MC_CHECK(qkv && mask_bias && ctx && lse, "attn_long_fwd: null pointer");
    if (int e = check_shape_long(b, t, nh, p)) return e;
    padded_view a{};
    a.qkv = (const bf16_t*)qkv; a.maskb = mask_bias; a.ctx = (bf16_t*)ctx; a.lse = lse;
    a.t = t; a.nh = nh; a.alpha = alpha; a.p = p; a.seed = seed; a.sid = stream_id;
    return launch_long<padded_view, false>(a, b, stream);
}

extern "C" int mc_attn_long_bwd(const mc_bf16* qkv, const float* mask_bias, const mc_bf16* dctx, const float* lse, int b,
                                int t, int nh, float alpha, float p, unsigned long long seed, unsigned int stream_id,
                                mc_bf16* dqkv, void* stream) {
    MC_CHECK(qkv && mask_bias && dctx && lse && dqkv, "attn_long_bwd: null pointer");
    if (int e = check_shape_long(b, t, nh, p)) return e;
    padded_view a{};
    a.qkv = (const bf16_t*)qkv; a.maskb = mask_bias; a.dctx = (const bf16_t*)dctx; a.dqkv = (bf16_t*)dqkv;
    a.lse = const_cast<float*>(lse);
    a.t = t; a.nh = nh; a.alpha = alpha; a.p = p; a.seed = seed; a.sid = stream_id;
    return launch_long<padded_view, true>(a, b, stream);
}

extern "C" int mc_attn_varlen_long_supported(int max_len, int head_dim) { return head_dim == HD && max_len >= 1 && max_len <= TLONG; }

extern "C" int mc_attn_varlen_long_fwd(const mc_bf16* qkv, const int* cu_seqlens, const int* order, int b, int max_len,
                                       int t_pad, long long rows, int nh, float alpha, float p, unsigned long long seed,
                                       unsigned int stream_id, mc_bf16* ctx, float* lse, void* stream) {
    MC_CHECK(qkv && cu_seqlens && ctx && lse, "attn_varlen_long_fwd: null pointer");
    if (int e = check_shape_varlen_long(b, max_len, t_pad, rows, nh, p)) return e;
    packed_view a{};
    a.qkv = (const bf16_t*)qkv; a.ctx = (bf16_t*)ctx; a.lse = lse; a.cu = cu_seqlens; a.order = order;
    a.rows = rows; a.nseq = b; a.tl = (max_len + 31) & ~31; a.t = t_pad; a.nh = nh;
    a.alpha = alpha; a.p = p; a.seed = seed; a.sid = stream_id;
    return launch_long<packed_view, false>(a, b, stream);
}

extern "C" int mc_attn_varlen_long_bwd(const mc_bf16* qkv, const int* cu_seqlens, const int* order, const mc_bf16* dctx,
                                       const float* lse, int b, int max_len, int t_pad, long long rows, int nh, float alpha,
                                       float p, unsigned long long seed, unsigned int stream_id, mc_bf16* dqkv,
                                       void* stream) {
    MC_CHECK(qkv && cu_seqlens && dctx && lse && dqkv, "attn_varlen_long_bwd: null pointer");
    if (int e = check_shape_varlen_long(b, max_len, t_pad, rows, nh, p)) return e;
    packed_view a{};
    a.qkv = (const bf16_t*)qkv; a.dctx = (const bf16_t*)dctx; a.dqkv = (bf16_t*)dqkv;
    a.lse = const_cast<float*>(lse);
    a.cu = cu_seqlens; a.order = order;
    a.rows = rows; a.nseq = b; a.tl = (max_len + 31) & ~31; a.t = t_pad; a.nh = nh;
    a.alpha = alpha; a.p = p; a.seed = seed; a.sid = stream_id;
    return launch_long<packed_view, true>(a, b, stream);
}
