// Multi-tensor AdamW update for the hot loop's optimizer step [ref: breastclip/optimizer/__init__.py:28-29 builds
// torch.optim.AdamW over ALL parameters; trainer_ddp.py:300-303 steps it once per iteration].
// HBM-bound: 16 B read + 12 B written per element (param, grad, exp_avg, exp_avg_sq), ~3.9 GB for the 138 M-parameter
// B5 + BERT model; a parameter that is consumed as a bf16 matrix gets its bf16 image rewritten by the same pass (+2 B)
// instead of by a cast kernel of its own in the next forward.  The packing of a tensor list into launches, the lookup of a
// workgroup's chunk and the pieces shared with the SGD step are multi_tensor.h's.
// mc_adamw_step_ema folds an exponential moving average of the weights into the same pass: the shadow of every updated
// element is read and written while the parameter is still in registers (+8 B per element, no second read of the parameter);
// mc_ema_update is the stand-alone form for tensors the optimizer pass does not cover (12 B per element).
// The file also holds the gradient passes of the loss-scaled and the clipped step (unscale, non-finite flag, norm) and the
// loss-scale update.  Kernels and host helpers first, the extern "C" entry points together at the end.
#include <cfloat>
#include <type_traits>
#include "multi_tensor.h"
#include "../../include/mammoclip_hip.h"

namespace {

// ---- AdamW
struct AdamPack {
    bf16_t* img[PACK];               // optional bf16 image of the updated parameter (nullptr: none)
    float* p[PACK];
    const float* g[PACK];
    float* m[PACK];
    float* v[PACK];
    PackIndex ix;
};

struct AdamScalars {
    float lr_wd;        // lr * weight_decay
    float beta1, beta2;
    float one_m_beta1, one_m_beta2;
    float step_size;    // lr / (1 - beta1^t)
    float inv_bc2_sqrt; // 1 / sqrt(1 - beta2^t)
    float eps;
};

// FORM: which of the two products of the second moment, beta2 v + ((1 - beta2) g) g, is rounded before the fused multiply-add
// takes the other.  1: fma(beta2, v, ((1 - beta2) g) g); 2: fma((1 - beta2) g, g, beta2 v).  The two differ in the last bit, so
// the form is part of the kernel's arithmetic and is written out; the kernel says which body uses which.  Every other
// expression has one product per sum, which -ffp-contract=fast fuses in one way only.
template <int FORM>
__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const AdamScalars& s) {
    static_assert(FORM == 1 || FORM == 2, "the second-moment form is always stated");
    // same operation order as torch's AdamW: decoupled decay first, moments, then the bias-corrected step
    p -= s.lr_wd * p;
    m = m + s.one_m_beta1 * (g - m);
    if (FORM == 1) v = __builtin_fmaf(s.beta2, v, (s.one_m_beta2 * g) * g);
    else v = __builtin_fmaf(s.one_m_beta2 * g, g, s.beta2 * v);
    const float denom = sqrtf(v) * s.inv_bc2_sqrt + s.eps;
    p -= s.step_size * (m / denom);
}

// Loss-scaled step without a host sync (f16 storage build): the non-finite flag of the gradient unscale and the count of
// steps skipped so far stay on the device.  A set flag makes the launch a no-op (GradScaler.step() skips optimizer.step());
// the bias corrections use the number of APPLIED steps, host step - skipped, like an optimizer that was never called.
struct AdamLs {
    const float* found_inf;    // nullptr: plain step with the host-derived scalars
    const float* skipped;      // steps skipped so far (float counter)
    double lr, beta1, beta2;
    long long step;
    const float* grad_coef;    // CLIP only: the clip coefficient of mc_grad_norm, a device scalar
};

struct NoEma {};
struct AdamEma {                     // the weight EMA of multi_tensor.h, for the tensors of the pack
    float* e[PACK];                  // shadow of pk.p[t]
    const long long* count;
    double decay;
    int warmup;
};

// CLIP: every gradient is multiplied by *ls.grad_coef as it is loaded (gradient-norm clipping without rewriting the
// gradients in memory; mul_rn_u: under -ffp-contract=fast a C++ product would be fused into the (g - m) and g * g that consume
// it, which is another rounding); CLIP = false is the kernel as it was.  EMA: the shadow em.e[t] of every updated element
// follows in the same pass (a skipped step returns before it, like before everything else); EMA = false is the kernel as it was.
template <bool CLIP, bool EMA>
__global__ void __launch_bounds__(256) adamw_multi_k(AdamPack pk, int count, AdamScalars s, AdamLs ls,
                                                     std::conditional_t<EMA, AdamEma, NoEma> em) {
    if (ls.found_inf) {
        if (*ls.found_inf != 0.f) return;                              // (uniform: the whole grid leaves)
        __shared__ float s_dev[2];
        if (threadIdx.x == 0) {
            long long te = ls.step - (long long)(*ls.skipped);
            if (te < 1) te = 1;
            s_dev[0] = (float)(ls.lr / (1.0 - pow(ls.beta1, (double)te)));
            s_dev[1] = (float)(1.0 / sqrt(1.0 - pow(ls.beta2, (double)te)));
        }
        __syncthreads();
        s.step_size = s_dev[0];
        s.inv_bc2_sqrt = s_dev[1];
    }
    const float c = CLIP ? *ls.grad_coef : 1.f;
    // Second-moment form (adamw1) of each body, with and without EMA: the float4 bodies of the kernel without clip use form 2;
    // its ragged tail and scalar body, and every body of the clip kernel, use form 1.  tests/test_adamw_bits_gpu.py holds the
    // bits of every body to recorded ones, tests/test_ema_gpu.py those of the EMA instantiations to the plain ones.
    constexpr int FV = CLIP ? 1 : 2, FS = 1;
    float w = 0.f;
    if constexpr (EMA) w = ema_weight(em.count, em.decay, em.warmup);
    const ChunkRef ck = chunk_of_block(pk.ix, count);
    const long long t = ck.t;
    float* __restrict__ p = pk.p[t] + ck.base;
    const float* __restrict__ g = pk.g[t] + ck.base;
    float* __restrict__ m = pk.m[t] + ck.base;
    float* __restrict__ v = pk.v[t] + ck.base;
    bf16_t* __restrict__ img = pk.img[t] ? pk.img[t] + ck.base : nullptr;
    const int len = ck.len();
    float* __restrict__ e = nullptr;
    if constexpr (EMA) e = em.e[t] + ck.base;
    const bool vec = (addr_bits(p, g, m, v, e) & 15) == 0 && (addr_bits(img) & 7) == 0;
    int i = threadIdx.x * 4;
    if (vec) {
        // 2 float4 per array in flight per lane (8 loads) before the first use
        for (; i + 1024 + 3 < len; i += 2048) {
            float4 P0 = *(const float4*)(p + i), P1 = *(const float4*)(p + i + 1024);
            float4 G0 = *(const float4*)(g + i), G1 = *(const float4*)(g + i + 1024);
            float4 M0 = *(const float4*)(m + i), M1 = *(const float4*)(m + i + 1024);
            float4 V0 = *(const float4*)(v + i), V1 = *(const float4*)(v + i + 1024);
            float4 E0, E1;
            if constexpr (EMA) { E0 = *(const float4*)(e + i); E1 = *(const float4*)(e + i + 1024); }
            if (CLIP) { mul_rn4_u(G0, c); mul_rn4_u(G1, c); }
            adamw1<FV>(P0.x, G0.x, M0.x, V0.x, s); adamw1<FV>(P0.y, G0.y, M0.y, V0.y, s);
            adamw1<FV>(P0.z, G0.z, M0.z, V0.z, s); adamw1<FV>(P0.w, G0.w, M0.w, V0.w, s);
            adamw1<FV>(P1.x, G1.x, M1.x, V1.x, s); adamw1<FV>(P1.y, G1.y, M1.y, V1.y, s);
            adamw1<FV>(P1.z, G1.z, M1.z, V1.z, s); adamw1<FV>(P1.w, G1.w, M1.w, V1.w, s);
            *(float4*)(p + i) = P0; *(float4*)(p + i + 1024) = P1;
            *(float4*)(m + i) = M0; *(float4*)(m + i + 1024) = M1;
            *(float4*)(v + i) = V0; *(float4*)(v + i + 1024) = V1;
            if constexpr (EMA) {
                ema4(E0, P0, w); ema4(E1, P1, w);
                *(float4*)(e + i) = E0; *(float4*)(e + i + 1024) = E1;
            }
            if (img) { store_image4(img + i, P0); store_image4(img + i + 1024, P1); }
        }
        for (; i + 3 < len; i += 1024) {
            float4 P0 = *(const float4*)(p + i), G0 = *(const float4*)(g + i);
            float4 M0 = *(const float4*)(m + i), V0 = *(const float4*)(v + i);
            float4 E0;
            if constexpr (EMA) E0 = *(const float4*)(e + i);
            if (CLIP) mul_rn4_u(G0, c);
            adamw1<FV>(P0.x, G0.x, M0.x, V0.x, s); adamw1<FV>(P0.y, G0.y, M0.y, V0.y, s);
            adamw1<FV>(P0.z, G0.z, M0.z, V0.z, s); adamw1<FV>(P0.w, G0.w, M0.w, V0.w, s);
            *(float4*)(p + i) = P0; *(float4*)(m + i) = M0; *(float4*)(v + i) = V0;
            if constexpr (EMA) { ema4(E0, P0, w); *(float4*)(e + i) = E0; }
            if (img) store_image4(img + i, P0);
        }
        // ragged tail of the chunk: the (< 4) elements after the last whole float4
        const int done = len & ~3;
        const int j = done + threadIdx.x;
        if (j < len) {
            float P = p[j], M = m[j], V = v[j];
            adamw1<FS>(P, CLIP ? mul_rn_u(g[j], c) : g[j], M, V, s);
            p[j] = P; m[j] = M; v[j] = V;
            if constexpr (EMA) { float E = e[j]; ema1(E, P, w); e[j] = E; }
            if (img) store_image1(img + j, P);
        }
    } else {
        for (int j = threadIdx.x; j < len; j += 256) {
            float P = p[j], M = m[j], V = v[j];
            adamw1<FS>(P, CLIP ? mul_rn_u(g[j], c) : g[j], M, V, s);
            p[j] = P; m[j] = M; v[j] = V;
            if constexpr (EMA) { float E = e[j]; ema1(E, P, w); e[j] = E; }
            if (img) store_image1(img + j, P);
        }
    }
}

// shadows == nullptr: no EMA (decay, warmup and count are not looked at).  The entry points have checked what is theirs alone.
int adamw_impl(const mc_adamw_tensor* tensors, int n_tensors, double lr, double beta1, double beta2, double eps, double weight_decay,
               long long step, const float* grad_coef, const float* found_inf, const float* skipped, float* const* shadows,
               double decay, int warmup, const long long* count, void* stream) {
    MC_CHECK(n_tensors >= 0 && (tensors || n_tensors == 0), "adamw: bad tensor list");
    MC_CHECK(step >= 1 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, "adamw: bad hyper-parameters");
    for (int i = 0; i < n_tensors; ++i) {                       // every argument is checked before the first launch
        const mc_adamw_tensor& t = tensors[i];
        MC_CHECK(t.numel == 0 || (t.param && t.grad && t.exp_avg && t.exp_avg_sq && t.numel > 0), "adamw: null tensor pointer");
    }
    // scalars are derived in double like torch does on the host (1 - 0.999 in fp32 is already 1.3e-5 off)
    AdamScalars s;
    s.lr_wd = (float)(lr * weight_decay);
    s.beta1 = (float)beta1; s.beta2 = (float)beta2;
    s.one_m_beta1 = (float)(1.0 - beta1); s.one_m_beta2 = (float)(1.0 - beta2);
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    s.step_size = (float)(lr / bc1);
    s.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    s.eps = (float)eps;
    AdamLs ls;
    ls.found_inf = found_inf; ls.skipped = skipped; ls.lr = lr; ls.beta1 = beta1; ls.beta2 = beta2; ls.step = step;
    ls.grad_coef = grad_coef;
    AdamEma em;
    em.count = count; em.decay = decay; em.warmup = warmup;
    return multi_tensor_launch<AdamPack>(
        n_tensors, "adamw: tensor too large", [&](int i) { return tensors[i].numel; },
        [&](AdamPack& pk, int slot, int i) {
            const mc_adamw_tensor& t = tensors[i];
            pk.p[slot] = t.param; pk.g[slot] = t.grad; pk.m[slot] = t.exp_avg; pk.v[slot] = t.exp_avg_sq;
            pk.img[slot] = t.bf16_image;
            if (shadows) em.e[slot] = shadows[i];
        },
        [&](const AdamPack& pk, int cnt, int chunks, long long) {
            if (shadows)
                hipLaunchKernelGGL((grad_coef ? adamw_multi_k<true, true> : adamw_multi_k<false, true>), dim3(chunks), dim3(256), 0,
                                   (hipStream_t)stream, pk, cnt, s, ls, em);
            else
                hipLaunchKernelGGL((grad_coef ? adamw_multi_k<true, false> : adamw_multi_k<false, false>), dim3(chunks), dim3(256), 0,
                                   (hipStream_t)stream, pk, cnt, s, ls, NoEma{});
        });
}

// ---- stand-alone weight EMA: shadow <- shadow + w * (source - shadow) for a list of tensors (buffers, parameters the optimizer
// pass did not cover, loops under another optimizer).  Same packing; 8 B read + 4 B written per element.  A set non-finite
// flag makes the launch a no-op, like the optimizer step it follows.
struct EmaPack {
    float* e[PACK];
    const float* p[PACK];
    PackIndex ix;
};

__global__ void __launch_bounds__(256) ema_multi_k(EmaPack pk, int count, const long long* __restrict__ applied, double decay,
                                                   int warmup, const float* __restrict__ found_inf) {
    if (found_inf && *found_inf != 0.f) return;                        // (uniform: the whole grid leaves)
    const float w = ema_weight(applied, decay, warmup);
    const ChunkRef ck = chunk_of_block(pk.ix, count);
    float* __restrict__ e = pk.e[ck.t] + ck.base;
    const float* __restrict__ p = pk.p[ck.t] + ck.base;
    const int len = ck.len();
    int i = threadIdx.x * 4;
    if ((addr_bits(e, p) & 15) == 0) {
        // 4 float4 per array in flight per lane (8 loads) before the first use, like the optimizer pass
        for (; i + 3 * 1024 + 3 < len; i += 4096) {
            float4 E[4], P[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { E[u] = *(const float4*)(e + i + u * 1024); P[u] = *(const float4*)(p + i + u * 1024); }
#pragma unroll
            for (int u = 0; u < 4; ++u) { ema4(E[u], P[u], w); *(float4*)(e + i + u * 1024) = E[u]; }
        }
        for (; i + 3 < len; i += 1024) {
            float4 E0 = *(const float4*)(e + i);
            const float4 P0 = *(const float4*)(p + i);
            ema4(E0, P0, w);
            *(float4*)(e + i) = E0;
        }
        const int j = (len & ~3) + threadIdx.x;
        if (j < len) { float E0 = e[j]; ema1(E0, p[j], w); e[j] = E0; }
    } else {
        for (int j = threadIdx.x; j < len; j += 256) { float E0 = e[j]; ema1(E0, p[j], w); e[j] = E0; }
    }
}

// the count of applied updates moves on unless the step was skipped (one thread; before mc_loss_scale_update clears the flag)
__global__ void ema_tick_k(long long* __restrict__ applied, const float* __restrict__ found_inf) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (found_inf && *found_inf != 0.f) return;
    *applied += 1;
}

inline bool ema_decay_ok(double decay) { return decay > 0.0 && decay < 1.0; }            // (false for nan)

// ---- gradient unscale + non-finite check of the loss-scaled (f16 storage) step [ref: trainer.py:271-278 runs the backward
// under torch.cuda.amp.GradScaler: scaler.step() = unscale the gradients, skip the update if any is inf / nan].
// Same packing as the update kernel: a workgroup owns one CHUNK of one gradient tensor.
struct UnscalePack {
    float* g[PACK];
    PackIndex ix;
};

// torch.isfinite's answer: +-FLT_MAX is a finite gradient, inf and nan (every compare with nan is false) are not
__device__ __forceinline__ bool nonfinite(float v) { return !(fabsf(v) <= FLT_MAX); }

// One pass of a workgroup over its chunk, shared by every gradient kernel below.  STORE: g = g * mul in place, `bad` set on
// a non-finite product.  NORM: returns this lane's sum of v * v over the values it kept (the stored ones under STORE), in
// fp64 -- the product of two fp32 values is exact there, 1e-25 and 1e25 neither underflow nor overflow, and the lane adds
// its terms in index order, so the sum depends on the chunk's address and length alone (never on the kernel around it).
template <bool STORE, bool NORM>
__device__ __forceinline__ float pass1(float v, float mul, bool& bad, double& acc) {
    if (STORE) { v *= mul; bad |= nonfinite(v); }
    if (NORM) acc += (double)v * (double)v;
    return v;
}

template <bool STORE, bool NORM>
__device__ __forceinline__ double chunk_pass(float* __restrict__ g, int len, float mul, bool& bad) {
    double acc = 0.0;
    int i = threadIdx.x * 4;
    if ((addr_bits(g) & 15) == 0) {
        // 4 float4 in flight per lane before the first use (one load at a time leaves the pass latency-bound at less than
        // half of the HBM rate); the values are consumed in index order either way, so the lane's sum does not change
        for (; i + 3 * 1024 + 3 < len; i += 4096) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *(const float4*)(g + i + u * 1024);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u].x = pass1<STORE, NORM>(v[u].x, mul, bad, acc); v[u].y = pass1<STORE, NORM>(v[u].y, mul, bad, acc);
                v[u].z = pass1<STORE, NORM>(v[u].z, mul, bad, acc); v[u].w = pass1<STORE, NORM>(v[u].w, mul, bad, acc);
                if (STORE) *(float4*)(g + i + u * 1024) = v[u];
            }
        }
        for (; i + 3 < len; i += 1024) {
            float4 v = *(const float4*)(g + i);
            v.x = pass1<STORE, NORM>(v.x, mul, bad, acc); v.y = pass1<STORE, NORM>(v.y, mul, bad, acc);
            v.z = pass1<STORE, NORM>(v.z, mul, bad, acc); v.w = pass1<STORE, NORM>(v.w, mul, bad, acc);
            if (STORE) *(float4*)(g + i) = v;
        }
        const int j = (len & ~3) + threadIdx.x;
        if (j < len) { const float v = pass1<STORE, NORM>(g[j], mul, bad, acc); if (STORE) g[j] = v; }
    } else {
        for (int j = threadIdx.x; j < len; j += 256) { const float v = pass1<STORE, NORM>(g[j], mul, bad, acc); if (STORE) g[j] = v; }
    }
    return acc;
}

// sum over the 256 lanes of a workgroup in a fixed order (a tree over LDS: no atomics, no dependence on wave timing)
__device__ __forceinline__ double block_sum256(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// <STORE, NORM> = <1, 0>: the unscale (mul = inv_scale or 1 / *scale_dev) and the in-place clip (mul = *mul_dev, a plain
// product, no flag); <1, 1>: the unscale that also writes its chunk's sum of squares; <0, 1>: the sum of squares alone.
// partials: one double per workgroup, at this launch's running chunk offset of the whole call.
template <bool STORE, bool NORM>
__global__ void __launch_bounds__(256) grads_pass_k(UnscalePack pk, int count, float mul, const float* __restrict__ scale_dev,
                                                    const float* __restrict__ mul_dev, float* __restrict__ found_inf,
                                                    double* __restrict__ partials) {
    if (STORE) {
        if (scale_dev) mul = 1.0f / *scale_dev;                         // the dynamic scale lives on the device (no host sync)
        else if (mul_dev) mul = *mul_dev;
    }
    const ChunkRef ck = chunk_of_block(pk.ix, count);
    float* __restrict__ g = pk.g[ck.t] + ck.base;
    bool bad = false;
    const double acc = chunk_pass<STORE, NORM>(g, ck.len(), mul, bad);
    if (STORE && bad && found_inf) *found_inf = 1.0f;          // (every writer stores the same value)
    if (NORM) {
        __shared__ double sh[256];
        const double tot = block_sum256(acc, sh);
        if (threadIdx.x == 0) partials[blockIdx.x] = tot;
    }
}

// total norm and clip coefficient from the per-chunk sums: one workgroup, thread-strided pass then the fixed tree.
// out[0] = (float)sqrt(sum); out[1] = min(1, max_norm / (out[0] + 1e-6)) in fp32 from the ROUNDED norm, with the quotient
// formed the way torch forms `max_norm / tensor` (Tensor.__rtruediv__): the correctly rounded reciprocal times max_norm,
// two roundings.  (float)(1.0 / (double)d) IS the correctly rounded fp32 reciprocal: 53 >= 2 * 24 + 2 bits.  A nan norm
// gives a nan coefficient (every compare with nan is false), an infinite max_norm gives 1.
__global__ void __launch_bounds__(256) grad_norm_finish_k(const double* __restrict__ partials, long long n, float max_norm,
                                                          float* __restrict__ out) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) acc += partials[i];
    const double tot = block_sum256(acc, sh);
    if (threadIdx.x == 0) {
        const float nrm = (float)sqrt(tot);
        const float c = mul_rn_u((float)(1.0 / (double)(nrm + 1e-6f)), max_norm);
        out[0] = nrm;
        out[1] = c > 1.0f ? 1.0f : c;
    }
}

// GradScaler.update() on the device [ref: trainer_ddp.py:303]: state = {scale, clean steps in a row, found_inf flag of the
// step, steps skipped (this scaler), _}.  Consumes and clears the flag; the optimizer's own skipped-step counter follows.
// The arithmetic is torch's (amp_update_scale_cuda_kernel): the fp32 scale times the DOUBLE factor, rounded once -- with a
// factor like 0.3 an fp32 multiply by 0.3f lands on other scales after two steps -- and a scale that growth would take
// past the fp32 range stays where it is (an inf scale never comes back: inf * backoff = inf, every later step skipped).
__global__ void loss_scale_update_k(float* __restrict__ st, float* __restrict__ opt_skipped, double growth, double backoff, int interval, int dynamic) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool bad = st[2] != 0.f;
    if (bad) { st[3] += 1.f; if (opt_skipped) *opt_skipped += 1.f; }
    if (dynamic) {
        if (bad) { st[0] = (float)((double)st[0] * backoff); st[1] = 0.f; }
        else {
            st[1] += 1.f;
            if (st[1] >= (float)interval) {
                const float grown = (float)((double)st[0] * growth);
                if (!nonfinite(grown)) st[0] = grown;
                st[1] = 0.f;
            }
        }
    }
    st[4] = bad ? 1.f : 0.f;        // what happened to the step just finished (for whoever looks, later)
    st[2] = 0.f;
}

// chunks (= doubles of norm workspace) of a gradient list, -1 on a bad one; need_grad: every non-empty tensor has a pointer
long long list_chunks(const mc_adamw_tensor* tensors, int n_tensors, bool need_grad) {
    if (n_tensors < 0 || (!tensors && n_tensors > 0)) return -1;
    long long tot = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (tensors[i].numel < 0 || (need_grad && tensors[i].numel > 0 && !tensors[i].grad)) return -1;
        tot += (tensors[i].numel + CHUNK - 1) / CHUNK;
    }
    return tot;
}

enum GradPass { GP_UNSCALE, GP_UNSCALE_NORM, GP_NORM };
int grads_pass_impl(GradPass mode, const mc_adamw_tensor* tensors, int n_tensors, float mul, const float* scale_dev,
                    const float* mul_dev, float* found_inf, double* partials, void* stream) {
    for (int i = 0; i < n_tensors; ++i)                         // every argument is checked before the first launch
        MC_CHECK(tensors[i].numel == 0 || (tensors[i].grad && tensors[i].numel > 0), "grads_unscale: null gradient pointer");
    auto k = mode == GP_UNSCALE ? grads_pass_k<true, false> : mode == GP_UNSCALE_NORM ? grads_pass_k<true, true> : grads_pass_k<false, true>;
    return multi_tensor_launch<UnscalePack>(
        n_tensors, "grads_unscale: tensor too large", [&](int i) { return tensors[i].numel; },
        [&](UnscalePack& pk, int slot, int i) { pk.g[slot] = const_cast<float*>(tensors[i].grad); },
        [&](const UnscalePack& pk, int cnt, int chunks, long long chunk_base) {
            hipLaunchKernelGGL(k, dim3(chunks), dim3(256), 0, (hipStream_t)stream, pk, cnt, mul, scale_dev, mul_dev, found_inf,
                               partials ? partials + chunk_base : nullptr);
        });
}

int grad_norm_finish(const double* partials, long long n, float max_norm, float* out2, void* stream) {
    hipLaunchKernelGGL(grad_norm_finish_k, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n, max_norm, out2);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

}  // namespace

// ---- entry points (include/mammoclip_hip.h)
extern "C" int mc_adamw_step(const mc_adamw_tensor* tensors, int n_tensors, double lr, double beta1, double beta2,
                             double eps, double weight_decay, long long step, void* stream) {
    return adamw_impl(tensors, n_tensors, lr, beta1, beta2, eps, weight_decay, step, nullptr, nullptr, nullptr, nullptr, 0.0, 0, nullptr,
                      stream);
}

extern "C" int mc_adamw_step_ls(const mc_adamw_tensor* tensors, int n_tensors, double lr, double beta1, double beta2,
                                double eps, double weight_decay, long long step, const float* found_inf, const float* skipped,
                                void* stream) {
    MC_CHECK(found_inf && skipped, "adamw_step_ls: null loss-scale state");
    return adamw_impl(tensors, n_tensors, lr, beta1, beta2, eps, weight_decay, step, nullptr, found_inf, skipped, nullptr, 0.0, 0, nullptr,
                      stream);
}

extern "C" int mc_adamw_step_clip(const mc_adamw_tensor* tensors, int n_tensors, double lr, double beta1, double beta2,
                                  double eps, double weight_decay, long long step, const float* grad_coef, const float* found_inf,
                                  const float* skipped, void* stream) {
    MC_CHECK(grad_coef, "adamw_step_clip: null grad_coef");
    MC_CHECK((found_inf == nullptr) == (skipped == nullptr), "adamw_step_clip: found_inf and skipped are both null or both set");
    return adamw_impl(tensors, n_tensors, lr, beta1, beta2, eps, weight_decay, step, grad_coef, found_inf, skipped, nullptr, 0.0, 0, nullptr,
                      stream);
}

extern "C" int mc_adamw_step_ema(const mc_adamw_tensor* tensors, float* const* shadows, int n_tensors, double lr, double beta1,
                                 double beta2, double eps, double weight_decay, long long step, double decay, int warmup,
                                 const long long* count, const float* grad_coef, const float* found_inf, const float* skipped,
                                 void* stream) {
    MC_CHECK(n_tensors >= 0 && ((tensors && shadows) || n_tensors == 0), "adamw_step_ema: bad tensor or shadow list");
    MC_CHECK(ema_decay_ok(decay), "adamw_step_ema: decay must lie strictly between 0 and 1");
    MC_CHECK(count, "adamw_step_ema: null update count");
    MC_CHECK((found_inf == nullptr) == (skipped == nullptr), "adamw_step_ema: found_inf and skipped are both null or both set");
    for (int i = 0; i < n_tensors; ++i) {
        MC_CHECK(tensors[i].numel >= 0, "adamw_step_ema: negative size");
        MC_CHECK(tensors[i].numel == 0 || shadows[i], "adamw_step_ema: null shadow pointer");
    }
    return adamw_impl(tensors, n_tensors, lr, beta1, beta2, eps, weight_decay, step, grad_coef, found_inf, skipped, shadows, decay,
                      warmup != 0, count, stream);
}

extern "C" int mc_ema_update(float* const* shadows, const float* const* sources, const long long* numel, int n_tensors, double decay,
                             int warmup, const long long* count, const float* found_inf, void* stream) {
    MC_CHECK(n_tensors >= 0 && ((shadows && sources && numel) || n_tensors == 0), "ema_update: bad tensor lists");
    MC_CHECK(ema_decay_ok(decay), "ema_update: decay must lie strictly between 0 and 1");
    MC_CHECK(count, "ema_update: null update count");
    for (int i = 0; i < n_tensors; ++i) {                       // every argument is checked before the first launch
        MC_CHECK(numel[i] >= 0, "ema_update: negative size");
        MC_CHECK(numel[i] == 0 || (shadows[i] && sources[i]), "ema_update: null tensor pointer");
    }
    return multi_tensor_launch<EmaPack>(
        n_tensors, "ema_update: tensor too large", [&](int i) { return numel[i]; },
        [&](EmaPack& pk, int slot, int i) { pk.e[slot] = shadows[i]; pk.p[slot] = sources[i]; },
        [&](const EmaPack& pk, int cnt, int chunks, long long) {
            hipLaunchKernelGGL(ema_multi_k, dim3(chunks), dim3(256), 0, (hipStream_t)stream, pk, cnt, count, decay, warmup != 0, found_inf);
        });
}

extern "C" int mc_ema_tick(long long* count, const float* found_inf, void* stream) {
    MC_CHECK(count, "ema_tick: null update count");
    hipLaunchKernelGGL(ema_tick_k, dim3(1), dim3(64), 0, (hipStream_t)stream, count, found_inf);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

extern "C" int mc_grads_unscale(const mc_adamw_tensor* tensors, int n_tensors, float inv_scale, float* found_inf, void* stream) {
    MC_CHECK(n_tensors >= 0 && (tensors || n_tensors == 0) && found_inf, "grads_unscale: bad arguments");
    return grads_pass_impl(GP_UNSCALE, tensors, n_tensors, inv_scale, nullptr, nullptr, found_inf, nullptr, stream);
}

extern "C" int mc_grads_unscale_dev(const mc_adamw_tensor* tensors, int n_tensors, const float* scale_dev, float* found_inf, void* stream) {
    MC_CHECK(scale_dev, "grads_unscale_dev: null scale");
    MC_CHECK(n_tensors >= 0 && (tensors || n_tensors == 0) && found_inf, "grads_unscale: bad arguments");
    return grads_pass_impl(GP_UNSCALE, tensors, n_tensors, 1.0f, scale_dev, nullptr, found_inf, nullptr, stream);
}

extern "C" long long mc_grad_norm_partials(const mc_adamw_tensor* tensors, int n_tensors) {
    const long long need = list_chunks(tensors, n_tensors, false);
    if (need < 0) mc_set_error("grad_norm_partials: bad tensor list");
    return need;
}

extern "C" int mc_grad_norm(const mc_adamw_tensor* tensors, int n_tensors, double* partials, long long n_partials, float max_norm,
                            float* out2, void* stream) {
    const long long need = list_chunks(tensors, n_tensors, true);
    MC_CHECK(need >= 0, "grad_norm: bad tensor list");
    MC_CHECK(out2, "grad_norm: null output");
    MC_CHECK(max_norm > 0.f, "grad_norm: max_norm must be positive (inf: the norm alone)");         // (false for nan)
    MC_CHECK(n_partials >= need && (partials || need == 0), "grad_norm: partials workspace too small");
    int r = grads_pass_impl(GP_NORM, tensors, n_tensors, 1.0f, nullptr, nullptr, nullptr, partials, stream);
    if (r != MC_OK) return r;
    return grad_norm_finish(partials, need, max_norm, out2, stream);
}

extern "C" int mc_grads_unscale_norm_dev(const mc_adamw_tensor* tensors, int n_tensors, const float* scale_dev, float* found_inf,
                                         double* partials, long long n_partials, float max_norm, float* out2, void* stream) {
    const long long need = list_chunks(tensors, n_tensors, true);
    MC_CHECK(need >= 0, "grads_unscale_norm_dev: bad tensor list");
    MC_CHECK(scale_dev && found_inf && out2, "grads_unscale_norm_dev: null scale, flag or output");
    MC_CHECK(max_norm > 0.f, "grads_unscale_norm_dev: max_norm must be positive (inf: the norm alone)");
    MC_CHECK(n_partials >= need && (partials || need == 0), "grads_unscale_norm_dev: partials workspace too small");
    int r = grads_pass_impl(GP_UNSCALE_NORM, tensors, n_tensors, 1.0f, scale_dev, nullptr, found_inf, partials, stream);
    if (r != MC_OK) return r;
    return grad_norm_finish(partials, need, max_norm, out2, stream);
}

extern "C" int mc_grads_scale_dev(const mc_adamw_tensor* tensors, int n_tensors, const float* coef, void* stream) {
    MC_CHECK(list_chunks(tensors, n_tensors, true) >= 0, "grads_scale_dev: bad tensor list");
    MC_CHECK(coef, "grads_scale_dev: null coefficient");
    return grads_pass_impl(GP_UNSCALE, tensors, n_tensors, 1.0f, nullptr, coef, nullptr, nullptr, stream);
}

extern "C" int mc_loss_scale_update(float* state, float* opt_skipped, double growth_factor, double backoff_factor, int growth_interval,
                                    int dynamic, void* stream) {
    MC_CHECK(state && growth_factor > 0.0 && backoff_factor > 0.0 && growth_interval >= 1, "loss_scale_update: bad arguments");
    hipLaunchKernelGGL(loss_scale_update_k, dim3(1), dim3(64), 0, (hipStream_t)stream, state, opt_skipped, growth_factor, backoff_factor,
                       growth_interval, dynamic);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
