// Multi-tensor launches of the optimizer kernels (optim.hip, optim_sgd.hip): the packing of a tensor list into launches, the
// device-side lookup of a workgroup's chunk, and the arithmetic pieces the update kernels share.
// Up to PACK tensors go into one launch (their pointers travel as kernel arguments, no device table to keep in sync); a
// workgroup owns one CHUNK of one tensor, found by a scan over the pack's chunk prefix.
#pragma once
#include "common_hip.h"

constexpr int PACK = 40;             // tensors per launch: 40 * 44 B + scalars stays far below the 4 KB argument limit
constexpr int CHUNK = 16384;         // elements per workgroup: 64 KB per stream in flight across its 256 lanes

// the index part of every pack struct (its last member, `ix`, after the pointer arrays of the kernel)
struct PackIndex {
    int first_chunk[PACK + 1];       // prefix of chunk counts
    long long n[PACK];
};

// the chunk of workgroup blockIdx.x: tensor slot t, len() (<= CHUNK) elements from element `base` of it.  base is a multiple
// of 16384, so a pointer advanced by it keeps its alignment.  (t is 64 bits wide because that is how the compiler indexes the
// pointer arrays with it: an int here is truncated and extended again in front of every use.)
struct ChunkRef {
    long long t, base, left;         // left: elements of the tensor from base on
    __device__ __forceinline__ int len() const { return left < CHUNK ? (int)left : CHUNK; }
};
__device__ __forceinline__ ChunkRef chunk_of_block(const PackIndex& ix, int count) {
    long long t = 0;
    const int blk = blockIdx.x;
    while (t + 1 < count && ix.first_chunk[t + 1] <= blk) ++t;       // uniform scan, <= PACK scalar compares
    const long long base = (long long)(blk - ix.first_chunk[t]) * CHUNK;
    return {t, base, ix.n[t] - base};
}

// the low address bits of several pointers at once: (addr_bits(p, g) & 15) == 0 is the float4 test of both
template <class... P>
__device__ __forceinline__ uintptr_t addr_bits(const P*... p) { return (... | (uintptr_t)p); }

// Walks a list of n_tensors tensors and launches over it in packs.  numel(i): elements of tensor i (0: skipped);
// fill(pack, slot, i): writes tensor i's pointers into the slot; launch(pack, count, chunks, chunk_base): one launch of
// `chunks` workgroups over `count` slots, chunk_base = the chunks of the launches before it (where a per-chunk output of the
// whole call continues).  A pack is flushed at PACK tensors or 2^30 chunks.  The whole list is checked against `too_large`
// before the first launch; the caller has checked its pointers by then.
template <class Pack, class Numel, class Fill, class Launch>
int multi_tensor_launch(int n_tensors, const char* too_large, Numel numel, Fill fill, Launch launch) {
    constexpr long long MAX_CHUNKS = 1ll << 30;
    auto chunks_of = [&](int i) { return (numel(i) + CHUNK - 1) / CHUNK; };
    for (int i = 0; i < n_tensors; ++i) MC_CHECK(chunks_of(i) < MAX_CHUNKS, too_large);
    Pack pk;
    int cnt = 0, chunks = 0;
    long long chunk_base = 0;
    auto flush = [&]() -> int {
        if (cnt == 0) return MC_OK;
        pk.ix.first_chunk[cnt] = chunks;
        launch(pk, cnt, chunks, chunk_base);
        MC_LAUNCH_CHECK();
        chunk_base += chunks;
        cnt = 0; chunks = 0;
        return MC_OK;
    };
    for (int i = 0; i < n_tensors; ++i) {
        if (numel(i) == 0) continue;
        const long long nch = chunks_of(i);
        if (cnt == PACK || chunks + nch > MAX_CHUNKS) {
            int r = flush();
            if (r != MC_OK) return r;
        }
        fill(pk, cnt, i);
        pk.ix.n[cnt] = numel(i); pk.ix.first_chunk[cnt] = chunks;
        chunks += (int)nch;
        ++cnt;
    }
    return flush();
}

// ---- shared arithmetic.  optim.hip is compiled under -ffp-contract=fast, optim_sgd.hip under `#pragma clang fp contract(off)`;
// every function below gives the same value under both: each product is written as the instruction, which the compiler cannot
// fuse into the sum that consumes it, and no function holds a C++ product next to a sum.

// a * b rounded once to fp32, the value torch.Tensor.mul_ would have stored; the product replaces a in place.
// mul_rn_u: b is uniform and sits in a scalar register (a kernel argument, a value loaded through a uniform pointer).
__device__ __forceinline__ float mul_rn(float a, float b) {
    asm("v_mul_f32 %0, %1, %0" : "+v"(a) : "v"(b));
    return a;
}
__device__ __forceinline__ float mul_rn_u(float a, float b) {
    asm("v_mul_f32 %0, %1, %0" : "+v"(a) : "s"(b));
    return a;
}
__device__ __forceinline__ void mul_rn4_u(float4& g, float c) {
    g.x = mul_rn_u(g.x, c); g.y = mul_rn_u(g.y, c); g.z = mul_rn_u(g.z, c); g.w = mul_rn_u(g.w, c);
}

// Weight EMA: e <- e + w * (p - e) as three separately rounded fp32 operations (sub, mul, add: what three tensor operations of
// torch give on any IEEE host).  w = (float)(1 - d_k), d_k = min(decay, (1 + k) / (10 + k)) with warm-up, decay without, in
// double; k = *count + 1: the applied updates so far, a device integer, plus this one.  Every launch of one update reads the
// same count; mc_ema_tick advances it afterwards.
__device__ __forceinline__ float ema_weight(const long long* __restrict__ count, double decay, int warmup) {
    double d = decay;
    if (warmup) {
        const double k = (double)(*count + 1);
        const double r = (1.0 + k) / (10.0 + k);
        if (r < d) d = r;
    }
    return (float)(1.0 - d);
}
__device__ __forceinline__ void ema1(float& e, float p, float w) { e = e + mul_rn(p - e, w); }     // (w comes out of fp64 arithmetic: a vector register)
__device__ __forceinline__ void ema4(float4& e, const float4& p, float w) {
    ema1(e.x, p.x, w); ema1(e.y, p.y, w); ema1(e.z, p.z, w); ema1(e.w, p.w, w);
}

// the 16-bit image of an updated parameter: four elements (img 8-byte aligned) or one.  (The float4 travels by value: by
// reference adamw_multi_k came out with more registers and one wave less per SIMD.)
__device__ __forceinline__ void store_image4(bf16_t* img, float4 p) {
    *(uint2*)img = make_uint2(pack_bf2(p.x, p.y), pack_bf2(p.z, p.w));
}
__device__ __forceinline__ void store_image1(bf16_t* img, float p) { *img = f2bf(p); }
