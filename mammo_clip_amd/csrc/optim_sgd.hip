// Multi-tensor SGD with momentum for the hot loop's optimizer step [ref: breastclip/optimizer/__init__.py:26-27 builds
// torch.optim.SGD over ALL parameters; trainer_ddp.py:300-303 steps it once per iteration].
// HBM-bound: 12 B read + 8 B written per element with momentum (param, grad, buffer), 8 + 4 without; +2 B for a bf16 image the
// pass rewrites from the updated parameter, +8 B for an EMA shadow that follows while the parameter is still in registers.
// The packing of the tensor list into launches (a workgroup owns one CHUNK of one tensor) and the product, EMA and image
// pieces are multi_tensor.h's.  The tensor table is mc_adamw_tensor: exp_avg carries the momentum buffer, exp_avg_sq is not read.
//
// Every operation of the rule (include/mammoclip_hip.h) is rounded to fp32 on its own, which is what the separate tensor
// operations of torch give on any IEEE host.  The library is built with -ffp-contract=fast, so every product is written as
// the instruction (mul_rn of multi_tensor.h): a product the compiler cannot see cannot be fused into the sum that consumes it.
// tests/test_sgd_gpu.py compares the bits on every body.
#pragma clang fp contract(off)
#include "multi_tensor.h"
#include "../../include/mammoclip_hip.h"

namespace {

struct SgdPack {
    bf16_t* img[PACK];               // optional bf16 image of the updated parameter (nullptr: none)
    float* p[PACK];
    const float* g[PACK];
    float* b[PACK];                  // momentum buffer (MOM only)
    float* e[PACK];                  // EMA shadow (EMA only)
    PackIndex ix;
};

struct SgdScalars {
    float lr, mu, one_m_damp, wd;    // each rounded from the double once, on the host
    unsigned sign;                   // maximize: 0x80000000 (the gradient's sign bit is flipped: an exact negation), else 0
    int nesterov;
    int has_wd;
    long long step;                  // host count of this launch set, >= 1; the first APPLIED step sets buf = g'
    const float* grad_coef;          // nullptr: no clip
    const float* found_inf;          // nullptr: no loss scale (then skipped is nullptr too)
    const float* skipped;
    const long long* ema_count;      // EMA only
    double ema_decay;
    int ema_warmup;
};

struct SgdUniform {                  // what a workgroup derives once
    float c, w;
    bool clip, first;
};

template <bool MOM>
__device__ __forceinline__ void sgd1(float& p, float g, float& b, const SgdScalars& s, const SgdUniform& u) {
    g = __uint_as_float(__float_as_uint(g) ^ s.sign);
    if (u.clip) g = mul_rn(g, u.c);
    if (s.has_wd) g = g + mul_rn(p, s.wd);
    float d = g;
    if (MOM) {
        if (u.first) b = g;
        else b = mul_rn(b, s.mu) + mul_rn(g, s.one_m_damp);
        d = s.nesterov ? g + mul_rn(b, s.mu) : b;
    }
    p = p - mul_rn(d, s.lr);
}
template <bool MOM>
__device__ __forceinline__ void sgd4(float4& p, const float4& g, float4& b, const SgdScalars& s, const SgdUniform& u) {
    sgd1<MOM>(p.x, g.x, b.x, s, u); sgd1<MOM>(p.y, g.y, b.y, s, u); sgd1<MOM>(p.z, g.z, b.z, s, u); sgd1<MOM>(p.w, g.w, b.w, s, u);
}

// MOM: the momentum buffer is read (not on a first step) and written; EMA: the shadow follows.  Everything else is a uniform
// branch on a kernel argument.  Body layout as adamw_multi_k: two float4 per array in flight, one float4, the ragged tail,
// and the scalar body for pointers that are not 16-byte aligned (8 bytes for the image).
template <bool MOM, bool EMA>
__global__ void __launch_bounds__(256) sgd_multi_k(SgdPack pk, int count, SgdScalars s) {
    SgdUniform u;
    u.first = s.step == 1;
    if (s.found_inf) {
        if (*s.found_inf != 0.f) return;                               // (uniform: the whole grid leaves)
        long long te = s.step - (long long)(*s.skipped);               // applied steps, this one included
        u.first = te <= 1;
    }
    u.clip = s.grad_coef != nullptr;
    u.c = u.clip ? *s.grad_coef : 1.f;
    u.w = 0.f;
    if constexpr (EMA) u.w = ema_weight(s.ema_count, s.ema_decay, s.ema_warmup);
    // chunk_of_block of multi_tensor.h, written out: through the function the <MOM, EMA> = <true, true> instance waits for its
    // loads at another place in the two-deep loop (profiles/optim_family_ab.md)
    int t = 0;
    const int blk = blockIdx.x;
    while (t + 1 < count && pk.ix.first_chunk[t + 1] <= blk) ++t;
    const long long base = (long long)(blk - pk.ix.first_chunk[t]) * CHUNK;
    float* __restrict__ p = pk.p[t] + base;
    const float* __restrict__ g = pk.g[t] + base;
    float* __restrict__ b = MOM ? pk.b[t] + base : nullptr;
    float* __restrict__ e = EMA ? pk.e[t] + base : nullptr;
    bf16_t* __restrict__ img = pk.img[t] ? pk.img[t] + base : nullptr;      // base is a multiple of 16384: alignment kept
    const long long left = pk.ix.n[t] - base;
    const int len = left < CHUNK ? (int)left : CHUNK;
    const bool vec = (addr_bits(p, g, b, e) & 15) == 0 && (addr_bits(img) & 7) == 0;
    const bool load_b = MOM && !u.first;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    int i = threadIdx.x * 4;
    if (vec) {
        for (; i + 1024 + 3 < len; i += 2048) {
            float4 P0 = *(const float4*)(p + i), P1 = *(const float4*)(p + i + 1024);
            const float4 G0 = *(const float4*)(g + i), G1 = *(const float4*)(g + i + 1024);
            float4 B0 = z4, B1 = z4, E0, E1;
            if (load_b) { B0 = *(const float4*)(b + i); B1 = *(const float4*)(b + i + 1024); }
            if constexpr (EMA) { E0 = *(const float4*)(e + i); E1 = *(const float4*)(e + i + 1024); }
            sgd4<MOM>(P0, G0, B0, s, u); sgd4<MOM>(P1, G1, B1, s, u);
            *(float4*)(p + i) = P0; *(float4*)(p + i + 1024) = P1;
            if constexpr (MOM) { *(float4*)(b + i) = B0; *(float4*)(b + i + 1024) = B1; }
            if constexpr (EMA) {
                ema4(E0, P0, u.w); ema4(E1, P1, u.w);
                *(float4*)(e + i) = E0; *(float4*)(e + i + 1024) = E1;
            }
            if (img) { store_image4(img + i, P0); store_image4(img + i + 1024, P1); }
        }
        for (; i + 3 < len; i += 1024) {
            float4 P0 = *(const float4*)(p + i);
            const float4 G0 = *(const float4*)(g + i);
            float4 B0 = z4, E0;
            if (load_b) B0 = *(const float4*)(b + i);
            if constexpr (EMA) E0 = *(const float4*)(e + i);
            sgd4<MOM>(P0, G0, B0, s, u);
            *(float4*)(p + i) = P0;
            if constexpr (MOM) *(float4*)(b + i) = B0;
            if constexpr (EMA) { ema4(E0, P0, u.w); *(float4*)(e + i) = E0; }
            if (img) store_image4(img + i, P0);
        }
    }
    // vector path: the (< 4) elements after the last whole float4, one per lane; otherwise the whole chunk, lane-strided
    for (int j = vec ? (len & ~3) + threadIdx.x : threadIdx.x; j < len; j += 256) {
        float P = p[j], B = load_b ? b[j] : 0.f;
        sgd1<MOM>(P, g[j], B, s, u);
        p[j] = P;
        if constexpr (MOM) b[j] = B;
        if constexpr (EMA) { float E = e[j]; ema1(E, P, u.w); e[j] = E; }
        if (img) store_image1(img + j, P);
    }
}

}  // namespace

extern "C" int mc_sgd_step(const mc_adamw_tensor* tensors, float* const* shadows, int n_tensors, double lr, double momentum,
                           double dampening, double weight_decay, int nesterov, int maximize, long long step, double decay,
                           int warmup, const long long* count, const float* grad_coef, const float* found_inf,
                           const float* skipped, void* stream) {
    MC_CHECK(n_tensors >= 0 && (tensors || n_tensors == 0), "sgd_step: bad tensor list");
    MC_CHECK(lr >= 0.0, "sgd_step: negative or nan lr");                                        // (false for nan)
    MC_CHECK(momentum >= 0.0, "sgd_step: negative or nan momentum");
    MC_CHECK(weight_decay >= 0.0, "sgd_step: negative or nan weight_decay");
    MC_CHECK(dampening == dampening, "sgd_step: nan dampening");
    MC_CHECK(!nesterov || (momentum > 0.0 && dampening == 0.0), "sgd_step: nesterov requires a momentum and zero dampening");
    MC_CHECK(step >= 1, "sgd_step: step counts from 1");
    MC_CHECK((found_inf == nullptr) == (skipped == nullptr), "sgd_step: found_inf and skipped are both null or both set");
    if (shadows) {
        MC_CHECK(decay > 0.0 && decay < 1.0, "sgd_step: decay must lie strictly between 0 and 1");
        MC_CHECK(count, "sgd_step: null update count");
    }
    const bool mom = momentum != 0.0;
    for (int i = 0; i < n_tensors; ++i) {                       // every argument is checked before the first launch
        const mc_adamw_tensor& t = tensors[i];
        MC_CHECK(t.numel >= 0, "sgd_step: negative size");
        if (t.numel == 0) continue;
        MC_CHECK(t.param && t.grad && (t.exp_avg || !mom), "sgd_step: null tensor pointer");
        MC_CHECK(!shadows || shadows[i], "sgd_step: null shadow pointer");
    }
    SgdScalars s;
    s.lr = (float)lr; s.mu = (float)momentum; s.one_m_damp = (float)(1.0 - dampening); s.wd = (float)weight_decay;
    s.sign = maximize ? 0x80000000u : 0u;
    s.nesterov = nesterov != 0;
    s.has_wd = weight_decay != 0.0;
    s.step = step;
    s.grad_coef = grad_coef; s.found_inf = found_inf; s.skipped = skipped;
    s.ema_count = shadows ? count : nullptr; s.ema_decay = decay; s.ema_warmup = warmup != 0;
    auto k = mom ? (shadows ? sgd_multi_k<true, true> : sgd_multi_k<true, false>)
                 : (shadows ? sgd_multi_k<false, true> : sgd_multi_k<false, false>);
    return multi_tensor_launch<SgdPack>(
        n_tensors, "sgd_step: tensor too large", [&](int i) { return tensors[i].numel; },
        [&](SgdPack& pk, int slot, int i) {
            const mc_adamw_tensor& t = tensors[i];
            pk.p[slot] = t.param; pk.g[slot] = t.grad; pk.b[slot] = mom ? t.exp_avg : nullptr;
            pk.e[slot] = shadows ? shadows[i] : nullptr;
            pk.img[slot] = t.bf16_image;
        },
        [&](const SgdPack& pk, int cnt, int chunks, long long) {
            hipLaunchKernelGGL(k, dim3(chunks), dim3(256), 0, (hipStream_t)stream, pk, cnt, s);
        });
}
