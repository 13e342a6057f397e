// Projection heads, L2 normalisation and the InfoNCE cross-entropy, all fp32 (the reference keeps
// embeddings / logits / loss in fp32 even under autocast).
// [ref: model/modules/projection.py:23-29, model/clip.py:86-91, loss/breast_clip.py:46-100]
// These are tiny (b x 512 x W*b); a simple LDS-tiled VALU kernel with arbitrary strides serves every layout.
#include "common_hip.h"
#include "../../include/mammoclip_hip.h"

namespace {

constexpr int TS = 32;

__global__ __launch_bounds__(256) void sgemm_k(const float* __restrict__ a, long long ars, long long acs,
                                               const float* __restrict__ b, long long brs, long long bcs,
                                               float* __restrict__ c, long long ldc, int m, int n, int k, float alpha,
                                               float beta, const float* __restrict__ bias,
                                               const float* __restrict__ alpha_dev, float* __restrict__ ws) {
    if (alpha_dev) alpha *= alpha_dev[0];
    __shared__ float sa[TS][TS + 1], sb[TS][TS + 1];
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;       // 16 x 16 threads, 2 x 2 outputs each
    const int m0 = blockIdx.y * TS, n0 = blockIdx.x * TS;
    float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    // split-K (gridDim.z > 1): this workgroup reduces k in [kb, ke) and leaves its partial in ws[z][m][n]
    const int kper = ((k + (int)gridDim.z - 1) / (int)gridDim.z + TS - 1) / TS * TS;
    const int kb = blockIdx.z * kper, ke = kb + kper < k ? kb + kper : k;
    for (int k0 = kb; k0 < ke; k0 += TS) {
        for (int e = threadIdx.x; e < TS * TS; e += 256) {
            int r = e / TS, cc = e % TS;
            // choose the faster-varying index by stride to keep loads coalesced where possible
            int mi = m0 + r, ki = k0 + cc;
            sa[r][cc] = (mi < m && ki < ke) ? a[mi * ars + ki * acs] : 0.f;
            int kj = k0 + r, nj = n0 + cc;
            sb[r][cc] = (kj < ke && nj < n) ? b[kj * brs + nj * bcs] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < TS; ++kk) {
            float a0 = sa[ty][kk], a1 = sa[ty + 16][kk];
            float b0 = sb[kk][tx], b1 = sb[kk][tx + 16];
            acc[0][0] = fmaf(a0, b0, acc[0][0]); acc[0][1] = fmaf(a0, b1, acc[0][1]);
            acc[1][0] = fmaf(a1, b0, acc[1][0]); acc[1][1] = fmaf(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int mi = m0 + ty + i * 16, nj = n0 + tx + j * 16;
            if (mi < m && nj < n) {
                if (gridDim.z > 1) { ws[((long long)blockIdx.z * m + mi) * n + nj] = acc[i][j]; continue; }
                float v = alpha * acc[i][j];
                if (bias) v += bias[nj];
                if (beta != 0.f) v += beta * c[mi * ldc + nj];
                c[mi * ldc + nj] = v;
            }
        }
}
// combine the split-K partials in split order (deterministic) and apply the epilogue
__global__ __launch_bounds__(256) void sgemm_splitk_finish_k(const float* __restrict__ ws, int splits, float* __restrict__ c,
                                                             long long ldc, int m, int n, float alpha, float beta,
                                                             const float* __restrict__ bias, const float* __restrict__ alpha_dev) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)m * n) return;
    if (alpha_dev) alpha *= alpha_dev[0];
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += ws[(long long)z * m * n + i];
    const int mi = (int)(i / n), nj = (int)(i % n);
    float v = alpha * s;
    if (bias) v += bias[nj];
    if (beta != 0.f) v += beta * c[mi * ldc + nj];
    c[mi * ldc + nj] = v;
}

__global__ void l2norm_fwd_k(const float* __restrict__ x, int rows, int d, float* __restrict__ y, float* __restrict__ norm) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f;
    for (int i = lane; i < d; i += 64) { float v = x[(long long)row * d + i]; s += v * v; }
    s = sqrtf(wave_sum(s));
    if (lane == 0) norm[row] = s;
    for (int i = lane; i < d; i += 64) y[(long long)row * d + i] = x[(long long)row * d + i] / s;
}
__global__ void l2norm_bwd_k(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ norm,
                             int rows, int d, float* __restrict__ dx) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f;
    for (int i = lane; i < d; i += 64) s += dy[(long long)row * d + i] * y[(long long)row * d + i];
    s = wave_sum(s);
    float inv = 1.f / norm[row];
    for (int i = lane; i < d; i += 64)
        dx[(long long)row * d + i] = (dy[(long long)row * d + i] - y[(long long)row * d + i] * s) * inv;
}

// ---- MLP projection head: the pointwise and row kernels around its two mc_sgemm calls (all fp32) ----
constexpr int MLP_MAX_N = 2048;        // four 8-float vectors per lane: the row kernels hold a row in registers
constexpr int MLP_BWD_MAX_WG = 256;    // the backward's grid cap (one workgroup per CU); each keeps a row of ws

// four elements per thread: one 16-byte access when the whole quad is inside, scalar at the tail
__global__ __launch_bounds__(256) void gelu_f32_fwd_k(const float* __restrict__ x, float* __restrict__ y, long long count) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < count) {
        const float4 v = *reinterpret_cast<const float4*>(x + i);
        *reinterpret_cast<float4*>(y + i) = make_float4(gelu_f(v.x), gelu_f(v.y), gelu_f(v.z), gelu_f(v.w));
    } else {
        for (long long j = i; j < count; ++j) y[j] = gelu_f(x[j]);
    }
}
// dx, dg and add may alias: a thread reads its quad before it writes it
__global__ __launch_bounds__(256) void gelu_f32_bwd_add_k(const float* dg, const float* __restrict__ x, const float* add,
                                                          float* dx, long long count) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < count) {
        const float4 g = *reinterpret_cast<const float4*>(dg + i), v = *reinterpret_cast<const float4*>(x + i);
        const float4 a = *reinterpret_cast<const float4*>(add + i);
        *reinterpret_cast<float4*>(dx + i) = make_float4(fmaf(g.x, gelu_grad_f(v.x), a.x), fmaf(g.y, gelu_grad_f(v.y), a.y),
                                                         fmaf(g.z, gelu_grad_f(v.z), a.z), fmaf(g.w, gelu_grad_f(v.w), a.w));
    } else {
        for (long long j = i; j < count; ++j) dx[j] = fmaf(dg[j], gelu_grad_f(x[j]), add[j]);
    }
}

// One wave per row, NV 8-float vectors per lane (vector v of lane l covers columns (l + 64 v) * 8 .. + 7): the row stays in
// registers between the mean pass, the variance pass and the store.  Lanes past the row's end carry zeros and are kept out
// of the variance.  The dropout factor of element row * n + col is half col % 8 of Philox draw (row * n + col) / 8.
template <int NV>
__global__ __launch_bounds__(256) void mlp_head_ln_fwd_k(const float* __restrict__ f, const float* __restrict__ res,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float eps, int rows, int n, float p, unsigned long long seed,
                                                         unsigned int sid, float* __restrict__ y, float* __restrict__ xhat,
                                                         float* __restrict__ rstd) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int nv = n / 8;
    const long long base = (long long)row * n;
    float z[NV][8];
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c8 = lane + 64 * v;
#pragma unroll
        for (int q = 0; q < 8; ++q) z[v][q] = 0.f;
        if (c8 < nv) {
            float a[8], r[8];
            load8f(f + base + c8 * 8, a);
            load8f(res + base + c8 * 8, r);
            if (p > 0.f) {
                float k[8];
                dropout_scale8(seed, sid, (unsigned long long)(base / 8 + c8), p, k);
#pragma unroll
                for (int q = 0; q < 8; ++q) z[v][q] = a[q] * k[q] + r[q];
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) z[v][q] = a[q] + r[q];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) s += z[v][q];
        }
    }
    const float mean = wave_sum(s) / (float)n;
    float ss = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v)
        if (lane + 64 * v < nv) {
#pragma unroll
            for (int q = 0; q < 8; ++q) { z[v][q] -= mean; ss += z[v][q] * z[v][q]; }
        }
    const float rs = 1.0f / sqrtf(wave_sum(ss) / (float)n + eps);
    if (lane == 0) rstd[row] = rs;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c8 = lane + 64 * v;
        if (c8 < nv) {
            float g[8], b[8], xh[8], o[8];
            load8f(gamma + c8 * 8, g);
            load8f(beta + c8 * 8, b);
#pragma unroll
            for (int q = 0; q < 8; ++q) { xh[q] = z[v][q] * rs; o[q] = xh[q] * g[q] + b[q]; }
            float* xo = xhat + base + c8 * 8;
            float* yo = y + base + c8 * 8;
            *reinterpret_cast<float4*>(xo) = make_float4(xh[0], xh[1], xh[2], xh[3]);
            *reinterpret_cast<float4*>(xo + 4) = make_float4(xh[4], xh[5], xh[6], xh[7]);
            *reinterpret_cast<float4*>(yo) = make_float4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<float4*>(yo + 4) = make_float4(o[4], o[5], o[6], o[7]);
        }
    }
}

// Workgroup b owns rows 4 b + w + 4 gridDim.x i (w = its wave, i = 0, 1, ..): a wave walks its rows in ascending order with
// the three column sums of its columns in registers, then the four waves add theirs in wave order through LDS
// (cs[3][n], dynamic) and the workgroup stores the result to its row of ws[gridDim.x][3][n] -- a fixed order, no atomics.
template <int NV>
__global__ __launch_bounds__(256) void mlp_head_ln_bwd_k(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                         const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                         int rows, int n, float p, unsigned long long seed, unsigned int sid,
                                                         float* __restrict__ df, float* __restrict__ dz,
                                                         float* __restrict__ ws) {
    extern __shared__ float cs[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nv = n / 8;
    const float inv_n = 1.0f / (float)n;
    float sg[NV][8], sb[NV][8], sf[NV][8], gm[NV][8];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
#pragma unroll
        for (int q = 0; q < 8; ++q) sg[v][q] = sb[v][q] = sf[v][q] = gm[v][q] = 0.f;
        if (lane + 64 * v < nv) load8f(gamma + (lane + 64 * v) * 8, gm[v]);
    }
    for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += 4ll * gridDim.x) {
        const long long base = row * n;
        float d[NV][8], xh[NV][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c8 = lane + 64 * v;
#pragma unroll
            for (int q = 0; q < 8; ++q) d[v][q] = xh[v][q] = 0.f;
            if (c8 < nv) {
                load8f(dy + base + c8 * 8, d[v]);
                load8f(xhat + base + c8 * 8, xh[v]);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    sg[v][q] += d[v][q] * xh[v][q];
                    sb[v][q] += d[v][q];
                    d[v][q] *= gm[v][q];                 // from here on: dy * gamma
                    s1 += d[v][q];
                    s2 += d[v][q] * xh[v][q];
                }
            }
        }
        const float m1 = wave_sum(s1) * inv_n, m2 = wave_sum(s2) * inv_n;
        const float rs = rstd[row];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c8 = lane + 64 * v;
            if (c8 < nv) {
                float o[8], k[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) o[q] = rs * (d[v][q] - m1 - xh[v][q] * m2);
                float* zo = dz + base + c8 * 8;
                *reinterpret_cast<float4*>(zo) = make_float4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<float4*>(zo + 4) = make_float4(o[4], o[5], o[6], o[7]);
                if (p > 0.f) {
                    dropout_scale8(seed, sid, (unsigned long long)(base / 8 + c8), p, k);
#pragma unroll
                    for (int q = 0; q < 8; ++q) o[q] *= k[q];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) sf[v][q] += o[q];
                float* fo = df + base + c8 * 8;
                *reinterpret_cast<float4*>(fo) = make_float4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<float4*>(fo + 4) = make_float4(o[4], o[5], o[6], o[7]);
            }
        }
    }
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int c8 = lane + 64 * v;
                if (c8 < nv) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int c = c8 * 8 + q;
                        if (w == 0) { cs[c] = sg[v][q]; cs[n + c] = sb[v][q]; cs[2 * n + c] = sf[v][q]; }
                        else { cs[c] += sg[v][q]; cs[n + c] += sb[v][q]; cs[2 * n + c] += sf[v][q]; }
                    }
                }
            }
        }
        __syncthreads();
    }
    float* wr = ws + (long long)blockIdx.x * 3 * n;
    for (int i = threadIdx.x; i < 3 * n; i += 256) wr[i] = cs[i];
}

// one wave per row: lse, per-row loss contribution (into row_loss), dlogits in place.
// labels: optional int64 class index per row (the `labels` the loss was called with, loss/breast_clip.py:43-44);
// the target of row r is labels[r] + label_offset (null: r + label_offset).
__global__ void ce_fwd_bwd_k(float* __restrict__ logits, int rows, int n, const long long* __restrict__ labels,
                             int label_offset, float w, float eps, float* __restrict__ row_loss) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float* lr = logits + (long long)row * n;
    float mx = -3.4e38f;
    for (int i = lane; i < n; i += 64) mx = fmaxf(mx, lr[i]);
    mx = wave_max(mx);
    float s = 0.f, sx = 0.f;
    for (int i = lane; i < n; i += 64) { s += __expf(lr[i] - mx); sx += lr[i]; }
    s = wave_sum(s);
    sx = wave_sum(sx);
    const float lse = mx + __logf(s);
    const int label = (labels ? (int)labels[row] : row) + label_offset;
    const float scale = w / (float)rows;
    // caller-supplied labels are validated here (the host can only range-check the arange form): an out-of-range label
    // makes the row's loss -- and with it the step's loss -- NaN instead of reading beside the row
    const bool ok = label >= 0 && label < n;
    // label smoothing eps: target = (1-eps) * onehot + eps / n   (torch F.cross_entropy semantics)
    if (lane == 0)
        row_loss[row] = ok ? ((1.f - eps) * (lse - lr[label]) + eps * (lse - sx / (float)n)) * scale : __uint_as_float(0x7fc00000u);
    const float inv = 1.f / s;
    const float un = eps / (float)n;
    for (int i = lane; i < n; i += 64) {
        float pr = __expf(lr[i] - mx) * inv;
        lr[i] = (pr - (i == label ? 1.f - eps : 0.f) - un) * scale;
    }
}
// loss_out[0] += sum_r row_loss[r], in a fixed order (bit-reproducible: no float atomics)
__global__ void ce_sum_rows_k(const float* __restrict__ row_loss, int rows, float* __restrict__ loss_out) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < rows; i += 256) s += row_loss[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_out[0] += red[0];
}

}  // namespace

static int sgemm_splits(int m, int n, int k) {
    const long long tiles = (long long)mc_div_up(n, TS) * mc_div_up(m, TS);
    long long s = 512 / tiles;                      // aim at ~2 workgroups per CU
    const long long kmax = k / (4 * TS);            // at least 4 k-tiles per split
    if (s > kmax) s = kmax;
    if (s > 32) s = 32;
    return s < 2 ? 1 : (int)s;
}
extern "C" long long mc_sgemm_ws_floats(int m, int n, int k) {
    const int s = sgemm_splits(m, n, k);
    return s > 1 ? (long long)s * m * n : 0;
}
extern "C" int mc_sgemm(const float* a, long long ars, long long acs, const float* b, long long brs, long long bcs,
                        float* c, long long ldc, int m, int n, int k, float alpha, float beta, const float* bias,
                        const float* alpha_dev, float* ws, void* stream) {
    MC_CHECK(a && b && c && m > 0 && n > 0 && k > 0, "sgemm: bad args");
    const int splits = ws ? sgemm_splits(m, n, k) : 1;
    dim3 grid(mc_div_up(n, TS), mc_div_up(m, TS), splits);
    hipLaunchKernelGGL(sgemm_k, grid, dim3(256), 0, (hipStream_t)stream, a, ars, acs, b, brs, bcs, c, ldc, m, n, k, alpha,
                       beta, bias, alpha_dev, ws);
    MC_LAUNCH_CHECK();
    if (splits > 1) {
        hipLaunchKernelGGL(sgemm_splitk_finish_k, dim3(mc_div_up((long long)m * n, 256)), dim3(256), 0, (hipStream_t)stream, ws,
                           splits, c, ldc, m, n, alpha, beta, bias, alpha_dev);
        MC_LAUNCH_CHECK();
    }
    return MC_OK;
}
__global__ void scale_f32_k(const float* __restrict__ x, const float* __restrict__ sd, float alpha, float* __restrict__ y,
                            long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float s = alpha * (sd ? sd[0] : 1.f);
    if (i < n) y[i] = x[i] * s;
}
extern "C" int mc_scale_f32(const float* x, const float* scalar_dev, float alpha, float* y, long long n, void* stream) {
    MC_CHECK(x && y && n > 0, "scale: bad args");
    hipLaunchKernelGGL(scale_f32_k, dim3(mc_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, x, scalar_dev, alpha, y, n);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_l2norm_fwd(const float* x, int rows, int d, float* y, float* norm, void* stream) {
    MC_CHECK(x && y && norm && rows > 0 && d > 0, "l2norm_fwd: bad args");
    hipLaunchKernelGGL(l2norm_fwd_k, dim3(mc_div_up(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, rows, d, y, norm);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_l2norm_bwd(const float* dy, const float* y, const float* norm, int rows, int d, float* dx, void* stream) {
    MC_CHECK(dy && y && norm && dx && rows > 0 && d > 0, "l2norm_bwd: bad args");
    hipLaunchKernelGGL(l2norm_bwd_k, dim3(mc_div_up(rows, 4)), dim3(256), 0, (hipStream_t)stream, dy, y, norm, rows, d, dx);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_mlp_head_max_n(void) { return MLP_MAX_N; }
extern "C" int mc_mlp_head_supported(int n) { return n >= 8 && n <= MLP_MAX_N && n % 8 == 0; }
extern "C" int mc_gelu_f32_fwd(const float* x, float* y, long long count, void* stream) {
    MC_CHECK(x && y, "gelu_f32_fwd: null pointer");
    MC_CHECK(count > 0 && count <= (1ll << 40), "gelu_f32_fwd: bad count");
    MC_CHECK(mc_aligned16(x) && mc_aligned16(y), "gelu_f32_fwd: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(gelu_f32_fwd_k, dim3(mc_div_up(count, 1024)), dim3(256), 0, (hipStream_t)stream, x, y, count);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_gelu_f32_bwd_add(const float* dg, const float* x, const float* add, float* dx, long long count,
                                   void* stream) {
    MC_CHECK(dg && x && add && dx, "gelu_f32_bwd_add: null pointer");
    MC_CHECK(count > 0 && count <= (1ll << 40), "gelu_f32_bwd_add: bad count");
    MC_CHECK(mc_aligned16(dg) && mc_aligned16(x) && mc_aligned16(add) && mc_aligned16(dx),
             "gelu_f32_bwd_add: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(gelu_f32_bwd_add_k, dim3(mc_div_up(count, 1024)), dim3(256), 0, (hipStream_t)stream, dg, x, add, dx,
                       count);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_mlp_head_ln_fwd(const float* f, const float* res, const float* gamma, const float* beta, float eps,
                                  int rows, int n, float p, unsigned long long seed, unsigned int stream_id, float* y,
                                  float* xhat, float* rstd, void* stream) {
    MC_CHECK(f && res && gamma && beta && y && xhat && rstd, "mlp_head_ln_fwd: null pointer");
    MC_CHECK(mc_mlp_head_supported(n), "mlp_head_ln_fwd: n must be a multiple of 8 in [8, 2048] (mc_mlp_head_supported)");
    MC_CHECK(rows > 0 && p >= 0.f && p < 1.f && eps >= 0.f, "mlp_head_ln_fwd: bad args (rows > 0, 0 <= p < 1, eps >= 0)");
    MC_CHECK(mc_aligned16(f) && mc_aligned16(res) && mc_aligned16(gamma) && mc_aligned16(beta) && mc_aligned16(y) &&
                 mc_aligned16(xhat), "mlp_head_ln_fwd: pointers must be 16-byte aligned");
    const dim3 grid(mc_div_up(rows, 4)), block(256);
    if (n <= 512)
        hipLaunchKernelGGL(mlp_head_ln_fwd_k<1>, grid, block, 0, (hipStream_t)stream, f, res, gamma, beta, eps, rows, n, p, seed,
                           stream_id, y, xhat, rstd);
    else if (n <= 1024)
        hipLaunchKernelGGL(mlp_head_ln_fwd_k<2>, grid, block, 0, (hipStream_t)stream, f, res, gamma, beta, eps, rows, n, p, seed,
                           stream_id, y, xhat, rstd);
    else
        hipLaunchKernelGGL(mlp_head_ln_fwd_k<4>, grid, block, 0, (hipStream_t)stream, f, res, gamma, beta, eps, rows, n, p, seed,
                           stream_id, y, xhat, rstd);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_mlp_head_ln_bwd_ws_rows(int rows) {
    if (rows <= 0) return 0;
    const int wg = mc_div_up(rows, 4);
    return wg < MLP_BWD_MAX_WG ? wg : MLP_BWD_MAX_WG;
}
extern "C" int mc_mlp_head_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, int rows, int n,
                                  float p, unsigned long long seed, unsigned int stream_id, float* df, float* dz, float* ws,
                                  int ws_rows, void* stream) {
    MC_CHECK(dy && xhat && rstd && gamma && df && dz && ws, "mlp_head_ln_bwd: null pointer");
    MC_CHECK(mc_mlp_head_supported(n), "mlp_head_ln_bwd: n must be a multiple of 8 in [8, 2048] (mc_mlp_head_supported)");
    MC_CHECK(rows > 0 && p >= 0.f && p < 1.f, "mlp_head_ln_bwd: bad args (rows > 0, 0 <= p < 1)");
    MC_CHECK(ws_rows == mc_mlp_head_ln_bwd_ws_rows(rows), "mlp_head_ln_bwd: ws_rows must be mc_mlp_head_ln_bwd_ws_rows(rows)");
    MC_CHECK(mc_aligned16(dy) && mc_aligned16(xhat) && mc_aligned16(gamma) && mc_aligned16(df) && mc_aligned16(dz),
             "mlp_head_ln_bwd: pointers must be 16-byte aligned");
    const dim3 grid(ws_rows), block(256);
    const size_t lds = 3 * (size_t)n * sizeof(float);
    if (n <= 512)
        hipLaunchKernelGGL(mlp_head_ln_bwd_k<1>, grid, block, lds, (hipStream_t)stream, dy, xhat, rstd, gamma, rows, n, p, seed,
                           stream_id, df, dz, ws);
    else if (n <= 1024)
        hipLaunchKernelGGL(mlp_head_ln_bwd_k<2>, grid, block, lds, (hipStream_t)stream, dy, xhat, rstd, gamma, rows, n, p, seed,
                           stream_id, df, dz, ws);
    else
        hipLaunchKernelGGL(mlp_head_ln_bwd_k<4>, grid, block, lds, (hipStream_t)stream, dy, xhat, rstd, gamma, rows, n, p, seed,
                           stream_id, df, dz, ws);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
extern "C" int mc_ce_fwd_bwd(float* logits, int rows, int n, const long long* labels, int label_offset, float w,
                             float smoothing, float* loss_out, float* row_ws, void* stream) {
    MC_CHECK(logits && loss_out && row_ws && rows > 0 && n > 0, "ce: bad args");
    MC_CHECK(label_offset >= 0 && (labels || label_offset + rows <= n), "ce: labels out of range");
    hipLaunchKernelGGL(ce_fwd_bwd_k, dim3(mc_div_up(rows, 4)), dim3(256), 0, (hipStream_t)stream, logits, rows, n, labels,
                       label_offset, w, smoothing, row_ws);
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(ce_sum_rows_k, dim3(1), dim3(256), 0, (hipStream_t)stream, row_ws, rows, loss_out);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
