// Shared pieces of the fused attention kernels (attn.hip: padded [b, t] batches, attn_varlen.hip: packed rows): LDS row
// layout, MFMA operand fragments read from the row-major LDS tiles, the two-step cross-lane row reduction.
#pragma once
#include "common_hip.h"

namespace {

constexpr int RS = 144;          // LDS row stride (bytes) of a 64-wide bf16 row: +16 B keeps ds_read_b64_tr_b16 conflict-free
constexpr int TMAX = 256;
constexpr int HD = 64;

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
__device__ __forceinline__ void stage_rows(unsigned char* dst, const bf16_t* src, long long ld, int t, int tid) {
    for (int idx = tid; idx < t * 8; idx += 512) {
        const int row = idx >> 3, ch = idx & 7;
        *reinterpret_cast<uint4*>(dst + row * RS + ch * 16) = *reinterpret_cast<const uint4*>(src + (long long)row * ld + ch * 8);
    }
}

}  // namespace
