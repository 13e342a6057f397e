// BERT (BioClinicalBERT = BERT-base shape) non-GEMM pieces for gfx950: embeddings + LayerNorm, residual +
// dropout + LayerNorm, masked softmax with dropout, erf-GELU, eos pooling -- forward and backward.
// [ref: model/modules/text_encoder.py:47-49 -> transformers BertModel (BertEmbeddings, BertSelfAttention,
//       BertSelfOutput, BertIntermediate, BertOutput); model/clip.py:65-68 (eos pooling)]
// One 64-lane wave owns one row (hidden <= 1024, keys <= 512); row reductions are wavefront shuffles;
// dropout masks are Philox functions of (seed, stream id, element index) and are regenerated in backward.
#include "common_hip.h"
#include "../../include/mammoclip_hip.h"

namespace {

constexpr int MAXV = 2;    // 8-element vectors per lane: hidden <= 64*8*2 = 1024

__device__ __forceinline__ void ln_stats(const float (*x)[8], int nvec, int lane, int h, float eps, float* mean,
                                         float* rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (lane + i * 64 < nvec)
#pragma unroll
            for (int q = 0; q < 8; ++q) s += x[i][q];
    float m = wave_sum(s) / (float)h;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (lane + i * 64 < nvec)
#pragma unroll
            for (int q = 0; q < 8; ++q) { float d = x[i][q] - m; v += d * d; }
    v = wave_sum(v) / (float)h;
    *mean = m;
    *rstd = rsqrtf(v + eps);
}

// MAP: packed rows -- ids / tt are in packed order, the position comes from pos_ids[row] and the dropout element index from
// row_map[row] (the row of the padded [b, t] layout); a row with row_map < 0 belongs to no sequence and gets zeros
template <bool MAP>
__global__ __launch_bounds__(256) void embed_fwd_k(const long long* __restrict__ ids, const long long* __restrict__ tt,
                                                   const int* __restrict__ pos_ids, const int* __restrict__ row_map,
                                                   const float* __restrict__ word, const float* __restrict__ pos,
                                                   const float* __restrict__ type, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float eps, long long rows, int t,
                                                   int h, float p, unsigned long long seed, unsigned int sid,
                                                   bf16_t* __restrict__ y, float* __restrict__ mean,
                                                   float* __restrict__ rstd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nvec = h / 8;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += (long long)gridDim.x * 4) {
        const long long drow = MAP ? (long long)row_map[row] : row;
        if (MAP && drow < 0) {
            if (lane == 0) { mean[row] = 0.f; rstd[row] = 0.f; }
            for (int v = lane; v < nvec; v += 64) *reinterpret_cast<uint4*>(y + row * h + v * 8) = make_uint4(0u, 0u, 0u, 0u);
            continue;
        }
        const long long id = ids[row];
        const long long ty = tt ? tt[row] : 0;
        const int tp = MAP ? pos_ids[row] : (int)(row % t);
        float x[MAXV][8];
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            int v = lane + i * 64;
            if (v < nvec) {
                float a[8], b[8], c[8];
                load8f(word + id * h + v * 8, a);
                load8f(pos + (long long)tp * h + v * 8, b);
                load8f(type + ty * h + v * 8, c);
#pragma unroll
                for (int q = 0; q < 8; ++q) x[i][q] = a[q] + c[q] + b[q];
            }
        }
        float m, rs;
        ln_stats(x, nvec, lane, h, eps, &m, &rs);
        if (lane == 0) { mean[row] = m; rstd[row] = rs; }
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            int v = lane + i * 64;
            if (v < nvec) {
                float g[8], b[8], o[8], ds[8];
                load8f(gamma + v * 8, g);
                load8f(beta + v * 8, b);
#pragma unroll
                for (int q = 0; q < 8; ++q) o[q] = (x[i][q] - m) * rs * g[q] + b[q];
                if (p > 0.f) {
                    dropout_scale8(seed, sid, (unsigned long long)(drow * nvec + v), p, ds);
#pragma unroll
                    for (int q = 0; q < 8; ++q) o[q] *= ds[q];
                }
                *reinterpret_cast<uint4*>(y + row * h + v * 8) = pack8(o);
            }
        }
    }
}

// wave w owns position tp = w % t and batch rows bi = w / t, w / t + nbw, ...
// MAP: packed rows -- sequence bi owns rows cu[bi] .. cu[bi+1]-1 of dy / ids / tt / mean / rstd, t is the longest
// sequence and tdrop the T of the padded layout (dropout element index)
// DET (the store-and-sum ending, no float atomics): the wave stores each token row's dx to dxrows [rows][h] (summed per
// vocabulary row by embed_dword_sum_k), its position sums to ws_pos [nbw][t][h], and the workgroup its gamma / beta / type-0 /
// type-1 sums (4 waves combined through LDS in wave order) to ws_gb [gridDim.x][4][h]; mc_ordered_sum finishes the last two
template <bool MAP, bool DET>
__device__ __forceinline__ void embed_bwd_body(const bf16_t* __restrict__ dy, const long long* __restrict__ ids,
                                               const int* __restrict__ cu, int tdrop,
                                               const long long* __restrict__ tt, const float* __restrict__ word,
                                               const float* __restrict__ pos, const float* __restrict__ type,
                                               const float* __restrict__ gamma, const float* __restrict__ mean,
                                               const float* __restrict__ rstd, int b, int t, int h, int nbw, float p,
                                               unsigned long long seed, unsigned int sid, float* __restrict__ dword,
                                               float* __restrict__ dpos, float* __restrict__ dtype,
                                               float* __restrict__ dgamma, float* __restrict__ dbeta,
                                               float* __restrict__ dxrows, float* __restrict__ ws_pos,
                                               float* __restrict__ ws_gb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nvec = h / 8;
    const long long gw = (long long)blockIdx.x * 4 + wave;
    const bool live = gw < (long long)t * nbw;
    if (!DET && !live) return;                 // (DET: the waves past the last position take part in the LDS combine with zeros)
    const int tp = (int)(gw % t);
    const int bg = live ? (int)(gw / t) : b;
    float aps[MAXV][8], agm[MAXV][8], abt[MAXV][8], at0[MAXV][8], at1[MAXV][8], g[MAXV][8];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
#pragma unroll
        for (int q = 0; q < 8; ++q) { aps[i][q] = agm[i][q] = abt[i][q] = at0[i][q] = at1[i][q] = 0.f; g[i][q] = 0.f; }
        int v = lane + i * 64;
        if (v < nvec) load8f(gamma + v * 8, g[i]);
    }
    for (int bi = bg; bi < b; bi += nbw) {
        if (MAP && tp >= cu[bi + 1] - cu[bi]) continue;
        const long long row = MAP ? (long long)cu[bi] + tp : (long long)bi * t + tp;
        const long long drow = MAP ? (long long)bi * tdrop + tp : row;
        const long long id = ids[row];
        const long long ty = tt ? tt[row] : 0;
        const float m = mean[row], rs = rstd[row];
        float xh[MAXV][8], dg[MAXV][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            int v = lane + i * 64;
            if (v < nvec) {
                float a[8], bb[8], c[8], d[8];
                load8f(word + id * h + v * 8, a);
                load8f(pos + (long long)tp * h + v * 8, bb);
                load8f(type + ty * h + v * 8, c);
                unpack8(*reinterpret_cast<const uint4*>(dy + row * h + v * 8), d);
                if (p > 0.f) {
                    float ds[8];
                    dropout_scale8(seed, sid, (unsigned long long)(drow * nvec + v), p, ds);
#pragma unroll
                    for (int q = 0; q < 8; ++q) d[q] *= ds[q];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    float xv = (a[q] + c[q] + bb[q] - m) * rs;
                    xh[i][q] = xv;
                    agm[i][q] += d[q] * xv;
                    abt[i][q] += d[q];
                    float dgv = d[q] * g[i][q];
                    dg[i][q] = dgv;
                    s1 += dgv;
                    s2 += dgv * xv;
                }
            }
        }
        s1 = wave_sum(s1) / (float)h;
        s2 = wave_sum(s2) / (float)h;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            int v = lane + i * 64;
            if (v < nvec) {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    float dx = rs * (dg[i][q] - s1 - xh[i][q] * s2);
                    aps[i][q] += dx;
                    if (ty == 0) at0[i][q] += dx; else at1[i][q] += dx;
                    if constexpr (DET) dxrows[row * h + v * 8 + q] = dx;
                    else atomicAdd(dword + id * h + v * 8 + q, dx);
                }
            }
        }
    }
    if constexpr (DET) {
        __shared__ float red[4][MAXV * 64 * 16];
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {                  // 0: gamma | beta, 1: type 0 | type 1
            if (pass) __syncthreads();
#pragma unroll
            for (int i = 0; i < MAXV; ++i)
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    red[wave][((i * 64 + lane) * 16) + q] = pass ? at0[i][q] : agm[i][q];
                    red[wave][((i * 64 + lane) * 16) + 8 + q] = pass ? at1[i][q] : abt[i][q];
                    if (pass == 0 && live && lane + i * 64 < nvec) ws_pos[((long long)bg * t + tp) * h + (lane + i * 64) * 8 + q] = aps[i][q];
                }
            __syncthreads();
            for (int e = threadIdx.x; e < nvec * 16; e += 256) {
                int v = e / 16, q = e % 16;
                int i = v / 64, ln = v % 64;
                float sv = 0.f;
                for (int w = 0; w < 4; ++w) sv += red[w][((i * 64 + ln) * 16) + q];
                ws_gb[((long long)blockIdx.x * 4 + pass * 2 + q / 8) * h + v * 8 + q % 8] = sv;
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int v = lane + i * 64;
        if (v < nvec) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                atomicAdd(dpos + (long long)tp * h + v * 8 + q, aps[i][q]);
                atomicAdd(dgamma + v * 8 + q, agm[i][q]);
                atomicAdd(dbeta + v * 8 + q, abt[i][q]);
                atomicAdd(dtype + v * 8 + q, at0[i][q]);
                if (at1[i][q] != 0.f) atomicAdd(dtype + h + v * 8 + q, at1[i][q]);
            }
        }
    }
}
template <bool MAP>
__global__ __launch_bounds__(256) void embed_bwd_k(const bf16_t* __restrict__ dy, const long long* __restrict__ ids,
                                                   const int* __restrict__ cu, int tdrop,
                                                   const long long* __restrict__ tt, const float* __restrict__ word,
                                                   const float* __restrict__ pos, const float* __restrict__ type,
                                                   const float* __restrict__ gamma, const float* __restrict__ mean,
                                                   const float* __restrict__ rstd, int b, int t, int h, int nbw, float p,
                                                   unsigned long long seed, unsigned int sid, float* __restrict__ dword,
                                                   float* __restrict__ dpos, float* __restrict__ dtype,
                                                   float* __restrict__ dgamma, float* __restrict__ dbeta) {
    embed_bwd_body<MAP, false>(dy, ids, cu, tdrop, tt, word, pos, type, gamma, mean, rstd, b, t, h, nbw, p, seed, sid, dword, dpos,
                               dtype, dgamma, dbeta, nullptr, nullptr, nullptr);
}
template <bool MAP>
__global__ __launch_bounds__(256) void embed_bwd_ws_k(const bf16_t* __restrict__ dy, const long long* __restrict__ ids,
                                                      const int* __restrict__ cu, int tdrop,
                                                      const long long* __restrict__ tt, const float* __restrict__ word,
                                                      const float* __restrict__ pos, const float* __restrict__ type,
                                                      const float* __restrict__ gamma, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, int b, int t, int h, int nbw, float p,
                                                      unsigned long long seed, unsigned int sid, float* __restrict__ dxrows,
                                                      float* __restrict__ ws_pos, float* __restrict__ ws_gb) {
    embed_bwd_body<MAP, true>(dy, ids, cu, tdrop, tt, word, pos, type, gamma, mean, rstd, b, t, h, nbw, p, seed, sid, nullptr, nullptr,
                              nullptr, nullptr, nullptr, dxrows, ws_pos, ws_gb);
}
// dword[id] += (float) sum (double) dxrows[row] over the token rows that name id, in ascending row order.  sorted_ids / order:
// the n token ids sorted ascending (stable) and the token row of each; the wave at the FIRST sorted position of an id owns
// that vocabulary row, the others leave -- ids that no token names are not touched
__global__ __launch_bounds__(256) void embed_dword_sum_k(const long long* __restrict__ sorted_ids,
                                                         const long long* __restrict__ order, long long n,
                                                         const float* __restrict__ dxrows, int h, float* __restrict__ dword) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nvec = h / 8;
    const long long j0 = (long long)blockIdx.x * 4 + wave;
    if (j0 >= n) return;
    const long long id = sorted_ids[j0];
    if (j0 > 0 && sorted_ids[j0 - 1] == id) return;
    double acc[MAXV][8];
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[i][q] = 0.0;
    for (long long j = j0; j < n && sorted_ids[j] == id; ++j) {
        const float* src = dxrows + order[j] * h;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            int v = lane + i * 64;
            if (v < nvec) {
                float d[8];
                load8f(src + v * 8, d);
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[i][q] += (double)d[q];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int v = lane + i * 64;
        if (v < nvec)
#pragma unroll
            for (int q = 0; q < 8; ++q) dword[id * h + v * 8 + q] += (float)acc[i][q];
    }
}

// MAP (add_ln_fwd_k / add_ln_bwd_k): packed rows -- the dropout element index comes from row_map[row], the row of the
// padded [b, t] layout; a row with row_map < 0 belongs to no sequence and is not dropped
template <bool MAP>
__global__ __launch_bounds__(256) void add_ln_fwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ res,
                                                    const int* __restrict__ row_map,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float eps, long long rows, int h, float p, unsigned long long seed,
                                                    unsigned int sid, bf16_t* __restrict__ y, float* __restrict__ mean,
                                                    float* __restrict__ rstd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nvec = h / 8;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += (long long)gridDim.x * 4) {
        const long long drow = MAP ? (long long)row_map[row] : row;
        float s[MAXV][8];
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            int v = lane + i * 64;
            if (v < nvec) {
                float a[8], r[8];
                unpack8(*reinterpret_cast<const uint4*>(x + row * h + v * 8), a);
                unpack8(*reinterpret_cast<const uint4*>(res + row * h + v * 8), r);
                if (p > 0.f && drow >= 0) {
                    float ds[8];
                    dropout_scale8(seed, sid, (unsigned long long)(drow * nvec + v), p, ds);
#pragma unroll
                    for (int q = 0; q < 8; ++q) a[q] *= ds[q];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) s[i][q] = a[q] + r[q];
            }
        }
        float m, rs;
        ln_stats(s, nvec, lane, h, eps, &m, &rs);
        if (lane == 0) { mean[row] = m; rstd[row] = rs; }
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            int v = lane + i * 64;
            if (v < nvec) {
                float g[8], b[8], o[8];
                load8f(gamma + v * 8, g);
                load8f(beta + v * 8, b);
#pragma unroll
                for (int q = 0; q < 8; ++q) o[q] = (s[i][q] - m) * rs * g[q] + b[q];
                *reinterpret_cast<uint4*>(y + row * h + v * 8) = pack8(o);
            }
        }
    }
}

template <bool MAP>
__global__ __launch_bounds__(256) void add_ln_bwd_k(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                    const bf16_t* __restrict__ res, const int* __restrict__ row_map,
                                                    const float* __restrict__ gamma,
                                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                                    long long rows, int h, float p, unsigned long long seed,
                                                    unsigned int sid, bf16_t* __restrict__ dx, bf16_t* __restrict__ dres,
                                                    float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                    float* __restrict__ ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nvec = h / 8;
    float agm[MAXV][8], abt[MAXV][8], g[MAXV][8];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
#pragma unroll
        for (int q = 0; q < 8; ++q) { agm[i][q] = abt[i][q] = 0.f; g[i][q] = 0.f; }
        int v = lane + i * 64;
        if (v < nvec) load8f(gamma + v * 8, g[i]);
    }
    for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += (long long)gridDim.x * 4) {
        const float m = mean[row], rs = rstd[row];
        const long long drow = MAP ? (long long)row_map[row] : row;
        float xh[MAXV][8], dg[MAXV][8], ds[MAXV][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            int v = lane + i * 64;
#pragma unroll
            for (int q = 0; q < 8; ++q) ds[i][q] = 1.f;
            if (v < nvec) {
                float a[8], r[8], d[8];
                unpack8(*reinterpret_cast<const uint4*>(x + row * h + v * 8), a);
                unpack8(*reinterpret_cast<const uint4*>(res + row * h + v * 8), r);
                unpack8(*reinterpret_cast<const uint4*>(dy + row * h + v * 8), d);
                if (p > 0.f && drow >= 0) dropout_scale8(seed, sid, (unsigned long long)(drow * nvec + v), p, ds[i]);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    float xv = (a[q] * ds[i][q] + r[q] - m) * rs;
                    xh[i][q] = xv;
                    agm[i][q] += d[q] * xv;
                    abt[i][q] += d[q];
                    float dgv = d[q] * g[i][q];
                    dg[i][q] = dgv;
                    s1 += dgv;
                    s2 += dgv * xv;
                }
            }
        }
        s1 = wave_sum(s1) / (float)h;
        s2 = wave_sum(s2) / (float)h;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            int v = lane + i * 64;
            if (v < nvec) {
                float o[8], o2[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    o[q] = rs * (dg[i][q] - s1 - xh[i][q] * s2);
                    o2[q] = o[q] * ds[i][q];
                }
                *reinterpret_cast<uint4*>(dres + row * h + v * 8) = pack8(o);
                *reinterpret_cast<uint4*>(dx + row * h + v * 8) = pack8(o2);
            }
        }
    }
    // block reduce of dgamma / dbeta over the 4 waves, then one atomic per element per workgroup
    // (ws != NULL: a plain store into the workgroup's row of ws [gridDim.x][2][h] instead; mc_ordered_sum finishes)
    __shared__ float red[4][MAXV * 64 * 16];
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            red[wave][((i * 64 + lane) * 16) + q] = agm[i][q];
            red[wave][((i * 64 + lane) * 16) + 8 + q] = abt[i][q];
        }
    __syncthreads();
    for (int e = threadIdx.x; e < nvec * 16; e += 256) {
        int v = e / 16, q = e % 16;
        int i = v / 64, ln = v % 64;
        float s = 0.f;
        for (int w = 0; w < 4; ++w) s += red[w][((i * 64 + ln) * 16) + q];
        if (ws) ws[((long long)blockIdx.x * 2 + q / 8) * h + v * 8 + q % 8] = s;
        else if (q < 8) atomicAdd(dgamma + v * 8 + q, s);
        else atomicAdd(dbeta + v * 8 + (q - 8), s);
    }
}

constexpr int MAXT = 8;     // keys per lane: t <= 512

__global__ __launch_bounds__(256) void softmax_fwd_k(const float* __restrict__ sc, long long rows, int t, float p,
                                                     unsigned long long seed, unsigned int sid,
                                                     bf16_t* __restrict__ probs, bf16_t* __restrict__ pd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += (long long)gridDim.x * 4) {
        float v[MAXT];
        // the start of the maximum and the filler of the slots past t lie under every finite score: a row whose keys all carry
        // mc_mask_bias's -FLT_MAX keeps its own maximum and comes out uniform (1/t), as from torch and softmax_fwd_v8_k
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            int k = lane + i * 64;
            v[i] = (k < t) ? sc[row * t + k] : -INFINITY;
            mx = fmaxf(mx, v[i]);
        }
        mx = wave_max(mx);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            int k = lane + i * 64;
            v[i] = (k < t) ? __expf(v[i] - mx) : 0.f;
            s += v[i];
        }
        s = 1.f / wave_sum(s);
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            int k = lane + i * 64;
            if (k < t) {
                float pr = v[i] * s;
                long long e = row * t + k;
                probs[e] = f2bf(pr);
                if (p > 0.f) {
                    float ds[8];
                    dropout_scale8(seed, sid, (unsigned long long)(e >> 3), p, ds);
                    pd[e] = f2bf(pr * ds[e & 7]);
                } else if (pd != probs) {
                    pd[e] = f2bf(pr);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void softmax_bwd_k(const bf16_t* __restrict__ probs, const float* __restrict__ dpd,
                                                     long long rows, int t, float p, unsigned long long seed,
                                                     unsigned int sid, float alpha, bf16_t* __restrict__ ds_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += (long long)gridDim.x * 4) {
        float pr[MAXT], dp[MAXT];
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            int k = lane + i * 64;
            pr[i] = 0.f; dp[i] = 0.f;
            if (k < t) {
                long long e = row * t + k;
                pr[i] = bf2f(probs[e]);
                float d = dpd[e];
                if (p > 0.f) {
                    float dsc[8];
                    dropout_scale8(seed, sid, (unsigned long long)(e >> 3), p, dsc);
                    d *= dsc[e & 7];
                }
                dp[i] = d;
                dot += pr[i] * d;
            }
        }
        dot = wave_sum(dot);
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            int k = lane + i * 64;
            if (k < t) ds_out[row * t + k] = f2bf(pr[i] * (dp[i] - dot) * alpha);
        }
    }
}

// 8 keys per lane (t % 8 == 0, t / 8 a power of two <= 64): a row is G = t/8 adjacent lanes, a wave holds 64/G rows.
// 32-byte score loads, 16-byte probability stores, ONE dropout draw (8 factors) per lane instead of one per element.
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
template <int G>
__global__ __launch_bounds__(256) void softmax_fwd_v8_k(const float* __restrict__ sc, long long rows, float p,
                                                        unsigned long long seed, unsigned int sid,
                                                        bf16_t* __restrict__ probs, bf16_t* __restrict__ pd) {
    constexpr int RPW = 64 / G;                                  // rows per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / G, gl = lane % G;
    for (long long row0 = ((long long)blockIdx.x * 4 + wave) * RPW; row0 < rows; row0 += (long long)gridDim.x * 4 * RPW) {
        const long long row = row0 + sub;
        const bool ok = row < rows;
        const long long e8 = (ok ? row : 0) * G + gl;            // index of this lane's 8-element group
        float v[8];
        load8f(sc + e8 * 8, v);
        float mx = v[0];
#pragma unroll
        for (int q = 1; q < 8; ++q) mx = fmaxf(mx, v[q]);
        mx = group_max<G>(mx);
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) { v[q] = __expf(v[q] - mx); s += v[q]; }
        s = 1.f / group_sum<G>(s);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] *= s;
        if (!ok) continue;
        *reinterpret_cast<uint4*>(probs + e8 * 8) = pack8(v);
        if (p > 0.f) {
            float ds[8];
            dropout_scale8(seed, sid, (unsigned long long)e8, p, ds);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] *= ds[q];
            *reinterpret_cast<uint4*>(pd + e8 * 8) = pack8(v);
        } else if (pd != probs) {
            *reinterpret_cast<uint4*>(pd + e8 * 8) = pack8(v);
        }
    }
}
template <int G>
__global__ __launch_bounds__(256) void softmax_bwd_v8_k(const bf16_t* __restrict__ probs, const float* __restrict__ dpd,
                                                        long long rows, float p, unsigned long long seed,
                                                        unsigned int sid, float alpha, bf16_t* __restrict__ ds_out) {
    constexpr int RPW = 64 / G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / G, gl = lane % G;
    for (long long row0 = ((long long)blockIdx.x * 4 + wave) * RPW; row0 < rows; row0 += (long long)gridDim.x * 4 * RPW) {
        const long long row = row0 + sub;
        const bool ok = row < rows;
        const long long e8 = (ok ? row : 0) * G + gl;
        float pr[8], d[8];
        unpack8(*reinterpret_cast<const uint4*>(probs + e8 * 8), pr);
        load8f(dpd + e8 * 8, d);
        if (p > 0.f) {
            float dsc[8];
            dropout_scale8(seed, sid, (unsigned long long)e8, p, dsc);
#pragma unroll
            for (int q = 0; q < 8; ++q) d[q] *= dsc[q];
        }
        float dot = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) dot += pr[q] * d[q];
        dot = group_sum<G>(dot);
        if (!ok) continue;
#pragma unroll
        for (int q = 0; q < 8; ++q) d[q] = pr[q] * (d[q] - dot) * alpha;
        *reinterpret_cast<uint4*>(ds_out + e8 * 8) = pack8(d);
    }
}

__global__ void gelu_fwd_k(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, long long n8) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(x + i * 8), f);
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = gelu_f(f[q]);
        *reinterpret_cast<uint4*>(y + i * 8) = pack8(f);
    }
}
__global__ void gelu_bwd_k(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, bf16_t* __restrict__ dx, long long n8) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        float f[8], g[8];
        unpack8(*reinterpret_cast<const uint4*>(x + i * 8), f);
        unpack8(*reinterpret_cast<const uint4*>(dy + i * 8), g);
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = g[q] * gelu_grad_f(f[q]);
        *reinterpret_cast<uint4*>(dx + i * 8) = pack8(f);
    }
}
__global__ void mask_bias_k(const long long* __restrict__ mask, float* __restrict__ out, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = mask[i] ? 0.f : -3.4028234663852886e38f;
}
__global__ void eos_gather_k(const bf16_t* __restrict__ hid, const long long* __restrict__ mask, int t, int h,
                             float* __restrict__ out) {
    const int bi = blockIdx.x;
    __shared__ int idx;
    if (threadIdx.x == 0) {
        long long s = 0;
        for (int k = 0; k < t; ++k) s += mask[(long long)bi * t + k];
        int e = (int)s - 1;
        if (e < 0) e += t;                       // python negative index semantics of clip.py:67-68
        idx = e;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < h; i += blockDim.x) out[(long long)bi * h + i] = bf2f(hid[((long long)bi * t + idx) * h + i]);
}
__global__ void eos_scatter_k(const float* __restrict__ dout, const long long* __restrict__ mask, int t, int h,
                              bf16_t* __restrict__ dhid) {
    const int bi = blockIdx.x;
    __shared__ int idx;
    if (threadIdx.x == 0) {
        long long s = 0;
        for (int k = 0; k < t; ++k) s += mask[(long long)bi * t + k];
        int e = (int)s - 1;
        if (e < 0) e += t;
        idx = e;
    }
    __syncthreads();
    for (long long i = threadIdx.x; i < (long long)t * h; i += blockDim.x) {
        int k = (int)(i / h), c = (int)(i % h);
        dhid[(long long)bi * t * h + i] = (k == idx) ? f2bf(dout[(long long)bi * h + c]) : (bf16_t)0;
    }
}

int row_blocks(long long rows) {
    long long b = (rows + 3) / 4;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}

// work split of the embedding backward: batch groups per position, workgroups
int embed_bwd_nbw(int b, int t) {
    int nbw = 2048 / t;
    if (nbw < 1) nbw = 1;
    if (nbw > b) nbw = b;
    return nbw;
}
// the store-and-sum form (no float atomics): ws = dxrows [rows][h] | ws_pos [nbw][t][h] | ws_gb [workgroups][4][h]; `rows` token
// rows (padded: b * t), sorted_ids / order: their ids sorted ascending (stable) and the row of each
int launch_embed_bwd_ws(const mc_bf16* dy, const long long* ids, const long long* tt, const int* cu_seqlens, const float* word,
                        const float* pos, const float* type, const float* gamma, const float* mean, const float* rstd, int b, int t,
                        int t_pad, int h, long long rows, float p, unsigned long long seed, unsigned int stream_id, float* dword,
                        float* dpos, float* dtype, float* dgamma, float* dbeta, const long long* sorted_ids, const long long* order,
                        float* ws, long long ws_floats, void* stream) {
    int plan[2];
    MC_CHECK(ws_floats == mc_bert_embed_bwd_ws_floats(b, t, h, rows, plan), "embed_bwd_ws: ws was sized for another shape");
    const int nbw = plan[0], groups = plan[1];
    float* dxrows = ws;
    float* ws_pos = dxrows + rows * h;
    float* ws_gb = ws_pos + (long long)nbw * t * h;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cu_seqlens ? embed_bwd_ws_k<true> : embed_bwd_ws_k<false>, dim3(groups), dim3(256), 0, st, dy, ids, cu_seqlens,
                       t_pad, tt, word, pos, type, gamma, mean, rstd, b, t, h, nbw, p, seed, stream_id, dxrows, ws_pos, ws_gb);
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(embed_dword_sum_k, dim3(mc_div_up(rows, 4)), dim3(256), 0, st, sorted_ids, order, rows, dxrows, h, dword);
    MC_LAUNCH_CHECK();
    if (int e = mc_ordered_sum(ws_pos, nbw, (long long)t * h, (long long)t * h, dpos, 1, stream)) return e;
    if (int e = mc_ordered_sum(ws_gb, groups, 4ll * h, h, dgamma, 1, stream)) return e;
    if (int e = mc_ordered_sum(ws_gb + h, groups, 4ll * h, h, dbeta, 1, stream)) return e;
    return mc_ordered_sum(ws_gb + 2 * h, groups, 4ll * h, 2ll * h, dtype, 1, stream);
}
// embedding backward over t positions of b sequences; cu_seqlens set: packed rows, dropout indices of the [b, t_pad] layout
int launch_embed_bwd(const mc_bf16* dy, const long long* ids, const long long* tt, const int* cu_seqlens, const float* word,
                     const float* pos, const float* type, const float* gamma, const float* mean, const float* rstd, int b, int t,
                     int t_pad, int h, float p, unsigned long long seed, unsigned int stream_id, float* dword, float* dpos,
                     float* dtype, float* dgamma, float* dbeta, void* stream) {
    const int nbw = embed_bwd_nbw(b, t);
    long long waves = (long long)t * nbw;
    hipLaunchKernelGGL(cu_seqlens ? embed_bwd_k<true> : embed_bwd_k<false>, dim3(mc_div_up(waves, 4)), dim3(256), 0, (hipStream_t)stream,
                       dy, ids, cu_seqlens, t_pad, tt, word, pos, type, gamma, mean, rstd, b, t, h, nbw, p, seed, stream_id, dword, dpos,
                       dtype, dgamma, dbeta);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
// the two add+LayerNorm entry points (padded rows / row_map of the packed layout) differ in row_map only
int launch_add_ln_fwd(const char* shape_msg, const mc_bf16* x, const mc_bf16* res, const int* row_map, const float* gamma,
                      const float* beta, float eps, long long rows, int h, float p, unsigned long long seed,
                      unsigned int stream_id, mc_bf16* y, float* mean, float* rstd, void* stream) {
    MC_CHECK(rows > 0 && h > 0 && h % 8 == 0 && h <= 1024, shape_msg);
    hipLaunchKernelGGL(row_map ? add_ln_fwd_k<true> : add_ln_fwd_k<false>, dim3(row_blocks(rows)), dim3(256), 0, (hipStream_t)stream,
                       x, res, row_map, gamma, beta, eps, rows, h, p, seed, stream_id, y, mean, rstd);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
int launch_add_ln_bwd(const char* shape_msg, const mc_bf16* dy, const mc_bf16* x, const mc_bf16* res, const int* row_map,
                      const float* gamma, const float* mean, const float* rstd, long long rows, int h, float p,
                      unsigned long long seed, unsigned int stream_id, mc_bf16* dx, mc_bf16* dres, float* dgamma,
                      float* dbeta, float* ws, int ws_rows, void* stream) {
    MC_CHECK(rows > 0 && h > 0 && h % 8 == 0 && h <= 1024, shape_msg);
    const int blocks = mc_add_ln_bwd_ws_rows(rows);
    MC_CHECK(!ws || ws_rows == blocks, "add_ln_bwd_ws: ws was sized for another row count (ws_rows != mc_add_ln_bwd_ws_rows)");
    hipLaunchKernelGGL(row_map ? add_ln_bwd_k<true> : add_ln_bwd_k<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy,
                       x, res, row_map, gamma, mean, rstd, rows, h, p, seed, stream_id, dx, dres, dgamma, dbeta, ws);
    MC_LAUNCH_CHECK();
    if (!ws) return MC_OK;
    if (int e = mc_ordered_sum(ws, blocks, 2ll * h, h, dgamma, 1, stream)) return e;
    return mc_ordered_sum(ws + h, blocks, 2ll * h, h, dbeta, 1, stream);
}

}  // namespace

extern "C" int mc_bert_embed_fwd(const long long* ids, const long long* tt, const float* word, const float* pos,
                                 const float* type, const float* gamma, const float* beta, float eps, int b, int t, int h,
                                 float p, unsigned long long seed, unsigned int stream_id, mc_bf16* y, float* mean,
                                 float* rstd, void* stream) {
    MC_CHECK(ids && word && pos && type && gamma && beta && y && mean && rstd, "embed_fwd: null arg");
    MC_CHECK(b > 0 && t > 0 && h > 0 && h % 8 == 0 && h <= 1024, "embed_fwd: hidden must be a multiple of 8 and <= 1024");
    long long rows = (long long)b * t;
    hipLaunchKernelGGL(embed_fwd_k<false>, dim3(row_blocks(rows)), dim3(256), 0, (hipStream_t)stream, ids, tt, nullptr, nullptr,
                       word, pos, type, gamma, beta, eps, rows, t, h, p, seed, stream_id, y, mean, rstd);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_bert_embed_bwd(const mc_bf16* dy, const long long* ids, const long long* tt, const float* word,
                                 const float* pos, const float* type, const float* gamma, const float* mean,
                                 const float* rstd, int b, int t, int h, float p, unsigned long long seed,
                                 unsigned int stream_id, float* dword, float* dpos, float* dtype, float* dgamma,
                                 float* dbeta, void* stream) {
    MC_CHECK(dy && ids && word && pos && type && gamma && mean && rstd && dword && dpos && dtype && dgamma && dbeta, "embed_bwd: null arg");
    MC_CHECK(b > 0 && t > 0 && h > 0 && h % 8 == 0 && h <= 1024, "embed_bwd: bad shape");
    return launch_embed_bwd(dy, ids, tt, nullptr, word, pos, type, gamma, mean, rstd, b, t, t, h, p, seed, stream_id, dword, dpos, dtype,
                            dgamma, dbeta, stream);
}
extern "C" int mc_add_ln_fwd(const mc_bf16* x, const mc_bf16* res, const float* gamma, const float* beta, float eps,
                             long long rows, int h, float p, unsigned long long seed, unsigned int stream_id, mc_bf16* y,
                             float* mean, float* rstd, void* stream) {
    MC_CHECK(x && res && gamma && beta && y && mean && rstd, "add_ln_fwd: null arg");
    return launch_add_ln_fwd("add_ln_fwd: bad shape", x, res, nullptr, gamma, beta, eps, rows, h, p, seed, stream_id, y, mean, rstd, stream);
}
extern "C" int mc_add_ln_bwd(const mc_bf16* dy, const mc_bf16* x, const mc_bf16* res, const float* gamma,
                             const float* mean, const float* rstd, long long rows, int h, float p,
                             unsigned long long seed, unsigned int stream_id, mc_bf16* dx, mc_bf16* dres, float* dgamma,
                             float* dbeta, void* stream) {
    MC_CHECK(dy && x && res && gamma && mean && rstd && dx && dres && dgamma && dbeta, "add_ln_bwd: null arg");
    return launch_add_ln_bwd("add_ln_bwd: bad shape", dy, x, res, nullptr, gamma, mean, rstd, rows, h, p, seed, stream_id, dx, dres, dgamma,
                             dbeta, nullptr, 0, stream);
}
extern "C" int mc_add_ln_bwd_ws_rows(long long rows) {
    long long blocks = (rows + 3) / 4;
    if (blocks > 512) blocks = 512;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}
extern "C" int mc_add_ln_bwd_ws(const mc_bf16* dy, const mc_bf16* x, const mc_bf16* res, const float* gamma,
                                const float* mean, const float* rstd, long long rows, int h, float p,
                                unsigned long long seed, unsigned int stream_id, mc_bf16* dx, mc_bf16* dres, float* dgamma,
                                float* dbeta, float* ws, int ws_rows, void* stream) {
    MC_CHECK(dy && x && res && gamma && mean && rstd && dx && dres && dgamma && dbeta && ws, "add_ln_bwd_ws: null arg");
    return launch_add_ln_bwd("add_ln_bwd_ws: bad shape", dy, x, res, nullptr, gamma, mean, rstd, rows, h, p, seed, stream_id, dx, dres,
                             dgamma, dbeta, ws, ws_rows, stream);
}
extern "C" long long mc_bert_embed_bwd_ws_floats(int b, int t, int h, long long rows, int* plan) {
    if (b <= 0 || t <= 0 || h <= 0 || rows <= 0) return 0;
    const int nbw = embed_bwd_nbw(b, t), groups = mc_div_up((long long)t * nbw, 4);
    if (plan) { plan[0] = nbw; plan[1] = groups; }
    return (rows + (long long)nbw * t + 4ll * groups) * h;
}
extern "C" int mc_bert_embed_bwd_ws(const mc_bf16* dy, const long long* ids, const long long* tt, const float* word,
                                    const float* pos, const float* type, const float* gamma, const float* mean,
                                    const float* rstd, int b, int t, int h, float p, unsigned long long seed,
                                    unsigned int stream_id, float* dword, float* dpos, float* dtype, float* dgamma,
                                    float* dbeta, const long long* sorted_ids, const long long* order, float* ws,
                                    long long ws_floats, void* stream) {
    MC_CHECK(dy && ids && word && pos && type && gamma && mean && rstd && dword && dpos && dtype && dgamma && dbeta && sorted_ids &&
             order && ws, "embed_bwd_ws: null arg");
    MC_CHECK(b > 0 && t > 0 && h > 0 && h % 8 == 0 && h <= 1024, "embed_bwd_ws: bad shape");
    return launch_embed_bwd_ws(dy, ids, tt, nullptr, word, pos, type, gamma, mean, rstd, b, t, t, h, (long long)b * t, p, seed, stream_id,
                               dword, dpos, dtype, dgamma, dbeta, sorted_ids, order, ws, ws_floats, stream);
}
extern "C" int mc_softmax_fwd(const float* scores, long long rows, int t, float p, unsigned long long seed,
                              unsigned int stream_id, mc_bf16* probs, mc_bf16* probs_drop, void* stream) {
    MC_CHECK(scores && probs && probs_drop && rows > 0 && t > 0 && t <= 512, "softmax_fwd: bad args (t <= 512)");
    MC_CHECK(p == 0.f || t % 8 == 0, "softmax_fwd: dropout needs t % 8 == 0");
    const int g = t / 8;
    const bool v8 = t % 8 == 0 && g >= 2 && g <= 64 && (g & (g - 1)) == 0 && mc_aligned16(scores) && mc_aligned16(probs) && mc_aligned16(probs_drop);
    if (v8) {
        const int blocks = row_blocks(mc_div_up(rows, 64 / g)) * 2;
#define SM_FWD(G) hipLaunchKernelGGL(softmax_fwd_v8_k<G>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, scores, rows, p, seed, stream_id, probs, probs_drop)
        switch (g) { case 2: SM_FWD(2); break; case 4: SM_FWD(4); break; case 8: SM_FWD(8); break; case 16: SM_FWD(16); break;
                     case 32: SM_FWD(32); break; default: SM_FWD(64); break; }
#undef SM_FWD
    } else {
        hipLaunchKernelGGL(softmax_fwd_k, dim3(row_blocks(rows) * 2), dim3(256), 0, (hipStream_t)stream, scores, rows, t, p, seed,
                           stream_id, probs, probs_drop);
    }
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_softmax_bwd(const mc_bf16* probs, const float* dprobs_drop, long long rows, int t, float p,
                              unsigned long long seed, unsigned int stream_id, float alpha, mc_bf16* dscores,
                              void* stream) {
    MC_CHECK(probs && dprobs_drop && dscores && rows > 0 && t > 0 && t <= 512, "softmax_bwd: bad args (t <= 512)");
    const int g = t / 8;
    const bool v8 = t % 8 == 0 && g >= 2 && g <= 64 && (g & (g - 1)) == 0 && mc_aligned16(probs) && mc_aligned16(dprobs_drop) && mc_aligned16(dscores);
    if (v8) {
        const int blocks = row_blocks(mc_div_up(rows, 64 / g)) * 2;
#define SM_BWD(G) hipLaunchKernelGGL(softmax_bwd_v8_k<G>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, probs, dprobs_drop, rows, p, seed, stream_id, alpha, dscores)
        switch (g) { case 2: SM_BWD(2); break; case 4: SM_BWD(4); break; case 8: SM_BWD(8); break; case 16: SM_BWD(16); break;
                     case 32: SM_BWD(32); break; default: SM_BWD(64); break; }
#undef SM_BWD
    } else {
        hipLaunchKernelGGL(softmax_bwd_k, dim3(row_blocks(rows) * 2), dim3(256), 0, (hipStream_t)stream, probs, dprobs_drop, rows,
                           t, p, seed, stream_id, alpha, dscores);
    }
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_gelu_fwd(const mc_bf16* x, mc_bf16* y, long long n, void* stream) {
    MC_CHECK(x && y && n > 0 && n % 8 == 0, "gelu_fwd: n must be a positive multiple of 8");
    long long n8 = n / 8;
    int blocks = mc_div_up(n8, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(gelu_fwd_k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, n8);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_gelu_bwd(const mc_bf16* dy, const mc_bf16* x, mc_bf16* dx, long long n, void* stream) {
    MC_CHECK(dy && x && dx && n > 0 && n % 8 == 0, "gelu_bwd: n must be a positive multiple of 8");
    long long n8 = n / 8;
    int blocks = mc_div_up(n8, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(gelu_bwd_k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy, x, dx, n8);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_mask_bias(const long long* mask, float* out, long long n, void* stream) {
    MC_CHECK(mask && out && n > 0, "mask_bias: bad args");
    hipLaunchKernelGGL(mask_bias_k, dim3(mc_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, mask, out, n);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_eos_gather(const mc_bf16* hid, const long long* mask, int b, int t, int h, float* out, void* stream) {
    MC_CHECK(hid && mask && out && b > 0 && t > 0 && h > 0, "eos_gather: bad args");
    hipLaunchKernelGGL(eos_gather_k, dim3(b), dim3(256), 0, (hipStream_t)stream, hid, mask, t, h, out);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_eos_scatter(const float* dout, const long long* mask, int b, int t, int h, mc_bf16* dhid, void* stream) {
    MC_CHECK(dout && mask && dhid && b > 0 && t > 0 && h > 0, "eos_scatter: bad args");
    hipLaunchKernelGGL(eos_scatter_k, dim3(b), dim3(256), 0, (hipStream_t)stream, dout, mask, t, h, dhid);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

// ------------------------------------------------------------------------------------------------ packed rows
// The packed text encoder (BertModelHIP.set_packed) keeps only the real tokens of a [b, t] batch: sequence i owns rows
// cu_seqlens[i] .. cu_seqlens[i+1]-1 of an [R, h] matrix, row_map[r] is the padded row i*t + position of packed row r
// (-1 for the alignment rows behind the last sequence).  [ref: model/modules/text_encoder.py:47-49; model/clip.py:65-75]
namespace {

// out[i, :] = float(src[idx[i], :])
__global__ void rows_gather_k(const bf16_t* __restrict__ src, const int* __restrict__ idx, int h, float* __restrict__ out) {
    const long long r = idx[blockIdx.x];
    for (int c = threadIdx.x; c < h; c += blockDim.x) out[(long long)blockIdx.x * h + c] = bf2f(src[r * h + c]);
}
// dsrc[idx[i], :] = dout[i, :]   (dsrc zero-filled by the caller; idx has no duplicates)
__global__ void rows_scatter_k(const float* __restrict__ dout, const int* __restrict__ idx, int h, bf16_t* __restrict__ dsrc) {
    const long long r = idx[blockIdx.x];
    for (int c = threadIdx.x; c < h; c += blockDim.x) dsrc[r * h + c] = f2bf(dout[(long long)blockIdx.x * h + c]);
}
__global__ void segment_mean_fwd_k(const bf16_t* __restrict__ src, const int* __restrict__ cu, int h, float* __restrict__ out) {
    const int r0 = cu[blockIdx.x], r1 = cu[blockIdx.x + 1];
    const float n = fmaxf((float)(r1 - r0), 1e-9f);             // [ref: model/clip.py:73 torch.clamp(sum_mask, min=1e-9)]
    for (int c = threadIdx.x; c < h; c += blockDim.x) {
        float s = 0.f;
        for (long long r = r0; r < r1; ++r) s += bf2f(src[r * h + c]);
        out[(long long)blockIdx.x * h + c] = s / n;
    }
}
// one workgroup per packed row: dsrc[r, :] = dout[seq(r), :] / len, zeros in the alignment rows
__global__ void segment_mean_bwd_k(const float* __restrict__ dout, const int* __restrict__ cu, const int* __restrict__ row_map,
                                   int t, int h, bf16_t* __restrict__ dsrc) {
    const long long r = blockIdx.x;
    const int pr = row_map[r];
    const int i = pr < 0 ? 0 : pr / t;
    const float n = fmaxf((float)(cu[i + 1] - cu[i]), 1e-9f);
    for (int c = threadIdx.x; c < h; c += blockDim.x) dsrc[r * h + c] = pr < 0 ? (bf16_t)0 : f2bf(dout[(long long)i * h + c] / n);
}
// one workgroup per padded row: dst[i*t + pos, :] = pos < len_i ? src[cu[i] + pos, :] : 0     (16-byte chunks)
__global__ void unpack_rows_k(const bf16_t* __restrict__ src, const int* __restrict__ cu, int t, int h, bf16_t* __restrict__ dst) {
    const long long pr = blockIdx.x;
    const int i = (int)(pr / t), pos = (int)(pr % t);
    const bool real = pos < cu[i + 1] - cu[i];
    const long long r = (long long)cu[i] + pos;
    for (int v = threadIdx.x; v < h / 8; v += blockDim.x)
        *reinterpret_cast<uint4*>(dst + pr * h + v * 8) = real ? *reinterpret_cast<const uint4*>(src + r * h + v * 8) : make_uint4(0u, 0u, 0u, 0u);
}
// one workgroup per packed row: dst[r, :] = row_map[r] >= 0 ? src[row_map[r], :] : 0
__global__ void pack_rows_k(const bf16_t* __restrict__ src, const int* __restrict__ row_map, int h, bf16_t* __restrict__ dst) {
    const long long r = blockIdx.x;
    const long long pr = row_map[r];
    for (int v = threadIdx.x; v < h / 8; v += blockDim.x)
        *reinterpret_cast<uint4*>(dst + r * h + v * 8) = pr >= 0 ? *reinterpret_cast<const uint4*>(src + pr * h + v * 8) : make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

extern "C" int mc_bert_embed_rows_fwd(const long long* ids, const long long* tt, const int* pos_ids, const int* row_map,
                                      const float* word, const float* pos, const float* type, const float* gamma,
                                      const float* beta, float eps, long long rows, int h, float p, unsigned long long seed,
                                      unsigned int stream_id, mc_bf16* y, float* mean, float* rstd, void* stream) {
    MC_CHECK(ids && pos_ids && row_map && word && pos && type && gamma && beta && y && mean && rstd, "embed_rows_fwd: null arg");
    MC_CHECK(rows > 0 && h > 0 && h % 8 == 0 && h <= 1024, "embed_rows_fwd: hidden must be a multiple of 8 and <= 1024");
    hipLaunchKernelGGL(embed_fwd_k<true>, dim3(row_blocks(rows)), dim3(256), 0, (hipStream_t)stream, ids, tt, pos_ids, row_map,
                       word, pos, type, gamma, beta, eps, rows, 1, h, p, seed, stream_id, y, mean, rstd);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_bert_embed_rows_bwd(const mc_bf16* dy, const long long* ids, const long long* tt, const int* cu_seqlens,
                                      const float* word, const float* pos, const float* type, const float* gamma,
                                      const float* mean, const float* rstd, int b, int max_len, int t_pad, int h, float p,
                                      unsigned long long seed, unsigned int stream_id, float* dword, float* dpos,
                                      float* dtype, float* dgamma, float* dbeta, void* stream) {
    MC_CHECK(dy && ids && cu_seqlens && word && pos && type && gamma && mean && rstd && dword && dpos && dtype && dgamma && dbeta,
             "embed_rows_bwd: null arg");
    MC_CHECK(b > 0 && max_len > 0 && t_pad >= max_len && h > 0 && h % 8 == 0 && h <= 1024, "embed_rows_bwd: bad shape");
    return launch_embed_bwd(dy, ids, tt, cu_seqlens, word, pos, type, gamma, mean, rstd, b, max_len, t_pad, h, p, seed, stream_id, dword,
                            dpos, dtype, dgamma, dbeta, stream);
}
extern "C" int mc_bert_embed_rows_bwd_ws(const mc_bf16* dy, const long long* ids, const long long* tt, const int* cu_seqlens,
                                         const float* word, const float* pos, const float* type, const float* gamma,
                                         const float* mean, const float* rstd, int b, int max_len, int t_pad, int h,
                                         long long real_rows, float p, unsigned long long seed, unsigned int stream_id,
                                         float* dword, float* dpos, float* dtype, float* dgamma, float* dbeta,
                                         const long long* sorted_ids, const long long* order, float* ws, long long ws_floats,
                                         void* stream) {
    MC_CHECK(dy && ids && cu_seqlens && word && pos && type && gamma && mean && rstd && dword && dpos && dtype && dgamma && dbeta &&
             sorted_ids && order && ws, "embed_rows_bwd_ws: null arg");
    MC_CHECK(b > 0 && max_len > 0 && t_pad >= max_len && h > 0 && h % 8 == 0 && h <= 1024 && real_rows >= b &&
             real_rows <= (long long)b * max_len, "embed_rows_bwd_ws: bad shape");
    return launch_embed_bwd_ws(dy, ids, tt, cu_seqlens, word, pos, type, gamma, mean, rstd, b, max_len, t_pad, h, real_rows, p, seed,
                               stream_id, dword, dpos, dtype, dgamma, dbeta, sorted_ids, order, ws, ws_floats, stream);
}
extern "C" int mc_add_ln_rows_fwd(const mc_bf16* x, const mc_bf16* res, const int* row_map, const float* gamma,
                                  const float* beta, float eps, long long rows, int h, float p, unsigned long long seed,
                                  unsigned int stream_id, mc_bf16* y, float* mean, float* rstd, void* stream) {
    MC_CHECK(x && res && row_map && gamma && beta && y && mean && rstd, "add_ln_rows_fwd: null arg");
    return launch_add_ln_fwd("add_ln_rows_fwd: bad shape", x, res, row_map, gamma, beta, eps, rows, h, p, seed, stream_id, y, mean, rstd,
                             stream);
}
extern "C" int mc_add_ln_rows_bwd(const mc_bf16* dy, const mc_bf16* x, const mc_bf16* res, const int* row_map,
                                  const float* gamma, const float* mean, const float* rstd, long long rows, int h, float p,
                                  unsigned long long seed, unsigned int stream_id, mc_bf16* dx, mc_bf16* dres,
                                  float* dgamma, float* dbeta, void* stream) {
    MC_CHECK(dy && x && res && row_map && gamma && mean && rstd && dx && dres && dgamma && dbeta, "add_ln_rows_bwd: null arg");
    return launch_add_ln_bwd("add_ln_rows_bwd: bad shape", dy, x, res, row_map, gamma, mean, rstd, rows, h, p, seed, stream_id, dx, dres,
                             dgamma, dbeta, nullptr, 0, stream);
}
extern "C" int mc_add_ln_rows_bwd_ws(const mc_bf16* dy, const mc_bf16* x, const mc_bf16* res, const int* row_map,
                                     const float* gamma, const float* mean, const float* rstd, long long rows, int h, float p,
                                     unsigned long long seed, unsigned int stream_id, mc_bf16* dx, mc_bf16* dres,
                                     float* dgamma, float* dbeta, float* ws, int ws_rows, void* stream) {
    MC_CHECK(dy && x && res && row_map && gamma && mean && rstd && dx && dres && dgamma && dbeta && ws, "add_ln_rows_bwd_ws: null arg");
    return launch_add_ln_bwd("add_ln_rows_bwd_ws: bad shape", dy, x, res, row_map, gamma, mean, rstd, rows, h, p, seed, stream_id, dx,
                             dres, dgamma, dbeta, ws, ws_rows, stream);
}
extern "C" int mc_rows_gather(const mc_bf16* src, const int* idx, int n, int h, float* out, void* stream) {
    MC_CHECK(src && idx && out && n > 0 && h > 0, "rows_gather: bad args");
    hipLaunchKernelGGL(rows_gather_k, dim3(n), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, idx, h, out);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_rows_scatter(const float* dout, const int* idx, int n, int h, mc_bf16* dsrc, void* stream) {
    MC_CHECK(dout && idx && dsrc && n > 0 && h > 0, "rows_scatter: bad args");
    hipLaunchKernelGGL(rows_scatter_k, dim3(n), dim3(256), 0, (hipStream_t)stream, dout, idx, h, (bf16_t*)dsrc);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_segment_mean_fwd(const mc_bf16* src, const int* cu_seqlens, int b, int h, float* out, void* stream) {
    MC_CHECK(src && cu_seqlens && out && b > 0 && h > 0, "segment_mean_fwd: bad args");
    hipLaunchKernelGGL(segment_mean_fwd_k, dim3(b), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, cu_seqlens, h, out);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_segment_mean_bwd(const float* dout, const int* cu_seqlens, const int* row_map, long long rows, int t, int h,
                                   mc_bf16* dsrc, void* stream) {
    MC_CHECK(dout && cu_seqlens && row_map && dsrc && rows > 0 && t > 0 && h > 0, "segment_mean_bwd: bad args");
    hipLaunchKernelGGL(segment_mean_bwd_k, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, dout, cu_seqlens, row_map, t, h,
                       (bf16_t*)dsrc);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_unpack_rows(const mc_bf16* src, const int* cu_seqlens, int b, int t, int h, mc_bf16* dst, void* stream) {
    MC_CHECK(src && cu_seqlens && dst && b > 0 && t > 0 && h > 0 && h % 8 == 0, "unpack_rows: bad args (h % 8 == 0)");
    hipLaunchKernelGGL(unpack_rows_k, dim3((unsigned)((long long)b * t)), dim3(128), 0, (hipStream_t)stream, (const bf16_t*)src,
                       cu_seqlens, t, h, (bf16_t*)dst);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_pack_rows(const mc_bf16* src, const int* row_map, long long rows, int h, mc_bf16* dst, void* stream) {
    MC_CHECK(src && row_map && dst && rows > 0 && h > 0 && h % 8 == 0, "pack_rows: bad args (h % 8 == 0)");
    hipLaunchKernelGGL(pack_rows_k, dim3((unsigned)rows), dim3(128), 0, (hipStream_t)stream, (const bf16_t*)src, row_map, h,
                       (bf16_t*)dst);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
