// Direct stem convolution (3x3, stride 2, 3 input channels, static "same" padding) straight from a channels-last image:
//     e[n*oh*ow, c0] (bf16) = patches(x)[., 32] . Wb[c0, 32]^T          (+ BatchNorm column-statistic partials of e)
//     dW[c0, 32]    (fp32)  = de[n*oh*ow, c0]^T . patches(x)[., 32]
// [ref: efficientnet_custom.py:273 (_conv_stem), efficient_net_custom_utils.py:248-276 (static same padding)]
//
// The [n*oh*ow, 32] patch matrix of mc_stem_im2col (1.33x the bytes of the image, written and read once per forward and once
// more per backward) is never formed: a workgroup stages the (2 SR + 1) x (2 TW + 1) input pixels under a tile of SR output
// rows x TW output pixels into LDS -- rounded ONCE to bf16, planar per channel, zero where the static padding is -- and every
// wave builds the MFMA operand fragments of its output row from that tile with the patch index of the im2col path,
// k = cin*9 + kh*3 + kw (k = 27..31 zero).  The whole reduction is one 16x16x32 MFMA K-step against the [c0, 32] weight image of
// mc_stem_weight_prep, so the forward gives the bits of mc_stem_im2col + mc_gemm_rows_bf16.
//
// Planar bf16 tile: the 16 pixels of a fragment are 16 consecutive 32-bit LDS words per (channel, kernel row, kernel column)
// -- a row-interleaved fp32 tile (9-float pitch per output pixel) would put them on a stride-6 bank pattern.
//
// Persistent workgroups walk the tiles cyclically (the chip sweeps the image as one moving window); the next tile's pixels
// travel in registers while the current tile is computed.
#include "common_hip.h"
#include "../../include/mammoclip_hip.h"

namespace {

constexpr int TW = 64;                      // output pixels of one tile row (a wave's row: 4 fragments of 16 pixels)
constexpr int SR = 4;                       // output rows of a tile = waves of a workgroup
constexpr int NR = 2 * SR + 1;              // input rows under a tile
constexpr int NPX = 2 * TW + 1;             // input pixels under a tile row
constexpr int RSI = NPX + 3;                // tile row pitch in bf16 elements (264 bytes)
constexpr int PSI = NR * RSI * 2;           // plane pitch in bytes
constexpr int ZOFF = 3 * PSI;               // a row of zeros behind the planes: where k = 27..31 reads
constexpr int IMG_BYTES = ZOFF + RSI * 2;
constexpr int CPRW = (3 * NPX + 3) / 4;     // 4-element chunks of one input tile row
constexpr int NCHUNK = NR * CPRW;
constexpr int ISLOTS = (NCHUNK + 255) / 256;    // chunks per thread and tile

typedef __attribute__((ext_vector_type(4))) short s4_t;
typedef __attribute__((address_space(3))) s4_t lds_s4_t;

struct stem_geo {
    const void* x; long long sn, sh;        // channels-last image: element (img, y, x, c) at img*sn + y*sh + x*3 + c
    const unsigned int* mm; float mean, stdv;   // SRC = unsigned char: per-image {min}[n], {max}[n] and the dataset's mean / std
    int n, h, w, pad_l, pad_t, oh, ow;
    int tx, ty;                             // tiles per output row / column of one image
    long long tiles;
    int vec;                                // every 4-element chunk inside a row is one aligned vector load
};

// per-thread chunk of the input tile, constant over the tiles: LDS byte offset of its first element | channel of that element
// << 16 | tile row << 18 | chunk << 22 (0xffffffff: no chunk)
__device__ __forceinline__ void img_meta(int tid, unsigned (&meta)[ISLOTS]) {
#pragma unroll
    for (int s = 0; s < ISLOTS; ++s) {
        const int ci = tid + s * 256;
        meta[s] = 0xffffffffu;
        if (ci < NCHUNK) {
            const int r = ci / CPRW, q = ci - r * CPRW;
            const int px0 = (4 * q) / 3, c0 = 4 * q - 3 * px0;
            meta[s] = (unsigned)((r * RSI + px0) * 2) | ((unsigned)c0 << 16) | ((unsigned)r << 18) | ((unsigned)q << 22);
        }
    }
}

__device__ __forceinline__ void tile_origin(const stem_geo& g, long long t, int& img, int& oy0, int& ox0) {
    const int txi = (int)(t % g.tx);
    const long long u = t / g.tx;
    oy0 = (int)(u % g.ty) * SR;
    img = (int)(u / g.ty);
    ox0 = txi * TW;
}

// the tile's pixels -> registers, raw (fp32 bits / 4 bytes per chunk); elements outside the image load as zero
template <typename SRC>
__device__ __forceinline__ void img_load(const stem_geo& g, long long t, const unsigned (&meta)[ISLOTS],
                                         uint4 (&raw)[ISLOTS]) {
    int img, oy0, ox0;
    tile_origin(g, t, img, oy0, ox0);
    const int y0 = 2 * oy0 - g.pad_t, a00 = 3 * (2 * ox0 - g.pad_l), w3 = 3 * g.w;
    const SRC* base = reinterpret_cast<const SRC*>(g.x) + (long long)img * g.sn;
#pragma unroll
    for (int s = 0; s < ISLOTS; ++s) {
        raw[s] = make_uint4(0u, 0u, 0u, 0u);
        if (meta[s] == 0xffffffffu) continue;
        const int r = (int)((meta[s] >> 18) & 15u), q = (int)(meta[s] >> 22);
        const int y = y0 + r, a0 = a00 + 4 * q;
        if (y < 0 || y >= g.h) continue;
        const SRC* row = base + (long long)y * g.sh;
        if (g.vec && a0 >= 0 && a0 + 3 < w3) {
            if constexpr (sizeof(SRC) == 1) raw[s].x = *reinterpret_cast<const unsigned int*>(row + a0);
            else raw[s] = *reinterpret_cast<const uint4*>(row + a0);
        } else {
            unsigned v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int a = a0 + i;
                if (a >= 0 && a < w3) {
                    if constexpr (sizeof(SRC) == 1) v[i] = row[a];
                    else v[i] = __float_as_uint(row[a]);
                }
            }
            if constexpr (sizeof(SRC) == 1) raw[s].x = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            else raw[s] = make_uint4(v[0], v[1], v[2], v[3]);
        }
    }
}

// registers -> the planar bf16 tile.  SRC = unsigned char: the dataset's normalisation exactly as stem_im2col_k applies it
// (same operation order and roundings); padding stays zero
template <typename SRC>
__device__ __forceinline__ void img_store(const stem_geo& g, long long t, const unsigned (&meta)[ISLOTS],
                                          const uint4 (&raw)[ISLOTS], unsigned char* sImg) {
    int img, oy0, ox0;
    tile_origin(g, t, img, oy0, ox0);
    float lo = 0.f, range = 1.f;
    if constexpr (sizeof(SRC) == 1) {
        lo = (float)g.mm[img];
        range = (float)g.mm[g.n + img] - lo;
    }
    const int y0 = 2 * oy0 - g.pad_t, a00 = 3 * (2 * ox0 - g.pad_l), w3 = 3 * g.w;
#pragma unroll
    for (int s = 0; s < ISLOTS; ++s) {
        if (meta[s] == 0xffffffffu) continue;
        const unsigned lbase = meta[s] & 0xffffu;
        const int c0 = (int)((meta[s] >> 16) & 3u);
        float v[4];
        if constexpr (sizeof(SRC) == 1) {
            const int r = (int)((meta[s] >> 18) & 15u), q = (int)(meta[s] >> 22);
            const int y = y0 + r, a0 = a00 + 4 * q;
            const bool yok = y >= 0 && y < g.h;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float tv = (float)((raw[s].x >> (8 * i)) & 0xffu) - lo;
                tv = __fdiv_rn(tv, range);
                tv = __fdiv_rn(__fsub_rn(tv, g.mean), g.stdv);
                v[i] = (yok && a0 + i >= 0 && a0 + i < w3) ? tv : 0.f;
            }
        } else {
            v[0] = __uint_as_float(raw[s].x); v[1] = __uint_as_float(raw[s].y);
            v[2] = __uint_as_float(raw[s].z); v[3] = __uint_as_float(raw[s].w);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cc = c0 + i, wrap = cc >= 3 ? 1 : 0;              // (c0 <= 2, i <= 3: the pixel changes at most once)
            const unsigned addr = lbase + (unsigned)((cc - 3 * wrap) * PSI + wrap * 2);
            *reinterpret_cast<bf16_t*>(sImg + addr) = f2bf(v[i]);
        }
    }
}

// byte offset in the tile of patch element k of output pixel 0 of tile row `trow` (k >= 27: the row of zeros)
__device__ __forceinline__ unsigned patch_off(int k, int trow) {
    if (k >= 27) return (unsigned)ZOFF;
    const int c = k / 9, kh = (k - c * 9) / 3, kw = k - c * 9 - kh * 3;
    return (unsigned)(c * PSI + ((2 * trow + kh) * RSI + kw) * 2);
}

__device__ __forceinline__ bf16x8_t gather8(const unsigned char* p0, const unsigned char* p1, const unsigned char* p2,
                                            const unsigned char* p3, const unsigned char* p4, const unsigned char* p5,
                                            const unsigned char* p6, const unsigned char* p7) {
    uint4 v;
    v.x = (unsigned)*reinterpret_cast<const bf16_t*>(p0) | ((unsigned)*reinterpret_cast<const bf16_t*>(p1) << 16);
    v.y = (unsigned)*reinterpret_cast<const bf16_t*>(p2) | ((unsigned)*reinterpret_cast<const bf16_t*>(p3) << 16);
    v.z = (unsigned)*reinterpret_cast<const bf16_t*>(p4) | ((unsigned)*reinterpret_cast<const bf16_t*>(p5) << 16);
    v.w = (unsigned)*reinterpret_cast<const bf16_t*>(p6) | ((unsigned)*reinterpret_cast<const bf16_t*>(p7) << 16);
    return __builtin_bit_cast(bf16x8_t, v);
}

// ---------------------------------------------------------------------------------------------------------------- forward
// C8 = c0 / 8 (16-byte chunks of an output row).  D = W_frag . X_frag^T as in gemm_rows_kernel: a lane ends with 4 consecutive
// output channels of one pixel; the 16 x c0 result leaves through a per-wave LDS tile as whole 16-byte chunks, and a lane
// always stores the same 8 channels, whose BatchNorm statistics it accumulates (of the ROUNDED values, like gemm_rows_kernel).
template <typename SRC, int C8>
__global__ __launch_bounds__(256) void stem_conv_fwd_k(const stem_geo g, const bf16_t* __restrict__ wb, bf16_t* __restrict__ e,
                                                       float* __restrict__ stat_partials) {
    constexpr int FN = (C8 + 1) / 2, NP = FN * 16, C0 = C8 * 8;
    constexpr int CROW = (NP + 8) * 2;
    constexpr int SC_BYTES = (4 * 16 * CROW > 4 * 64 * 16 * 4) ? 4 * 16 * CROW : 4 * 64 * 16 * 4;
    __shared__ __attribute__((aligned(16))) unsigned char sImg[IMG_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char sC[SC_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kg = lane >> 4;

    for (int i = tid; i < RSI / 2; i += 256) reinterpret_cast<unsigned int*>(sImg + ZOFF)[i] = 0u;
    bf16x8_t wf[FN];
#pragma unroll
    for (int f = 0; f < FN; ++f) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (f * 16 + j < C0) v = *reinterpret_cast<const uint4*>(wb + (f * 16 + j) * 32 + kg * 8);
        wf[f] = __builtin_bit_cast(bf16x8_t, v);
    }
    unsigned meta[ISLOTS];
    img_meta(tid, meta);
    unsigned off[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) off[q] = patch_off(kg * 8 + q, wave) + (unsigned)(j * 4);

    constexpr int slots = 64 / C8;                  // rows written concurrently by one wave
    const int c8 = lane % C8, rs = lane / C8;
    const bool ep_active = rs < slots;
    float ssum[8], ssq[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { ssum[q] = 0.f; ssq[q] = 0.f; }
    unsigned char* myC = sC + wave * 16 * CROW;

    uint4 raw[ISLOTS];
    long long t = blockIdx.x;
    if (t < g.tiles) img_load<SRC>(g, t, meta, raw);
    for (; t < g.tiles; t += gridDim.x) {
        __syncthreads();                            // the previous tile's fragment reads are done
        img_store<SRC>(g, t, meta, raw, sImg);
        __syncthreads();
        if (t + gridDim.x < g.tiles) img_load<SRC>(g, t + gridDim.x, meta, raw);
        int img, oy0, ox0;
        tile_origin(g, t, img, oy0, ox0);
        const int oy = oy0 + wave;
        if (oy >= g.oh) continue;
        const long long mrow0 = ((long long)img * g.oh + oy) * g.ow;
#pragma unroll 1
        for (int gq = 0; gq < TW / 16; ++gq) {
            const int oxg = ox0 + gq * 16;
            if (oxg >= g.ow) break;
            const unsigned char* pb = sImg + gq * 64;
            const bf16x8_t xf = gather8(pb + off[0], pb + off[1], pb + off[2], pb + off[3], pb + off[4], pb + off[5],
                                        pb + off[6], pb + off[7]);
#pragma unroll
            for (int f = 0; f < FN; ++f) {
                const f32x4_t acc = MC_MFMA_16x16x32(wf[f], xf, ((f32x4_t){0.f, 0.f, 0.f, 0.f}), 0, 0, 0);
                const uint2 pk = make_uint2(pack_bf2(acc[0], acc[1]), pack_bf2(acc[2], acc[3]));
                *reinterpret_cast<uint2*>(myC + j * CROW + (f * 16 + kg * 4) * 2) = pk;
            }
            __builtin_amdgcn_wave_barrier();
            if (ep_active) {
                for (int row = rs; row < 16; row += slots) {
                    if (oxg + row < g.ow) {
                        const uint4 v = *reinterpret_cast<const uint4*>(myC + row * CROW + c8 * 16);
                        if (stat_partials) {
                            float a[8];
                            unpack8(v, a);
#pragma unroll
                            for (int q = 0; q < 8; ++q) { ssum[q] += a[q]; ssq[q] += a[q] * a[q]; }
                        }
                        *reinterpret_cast<uint4*>(e + (mrow0 + oxg + row) * C0 + c8 * 8) = v;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (stat_partials) {
        __syncthreads();
        float* red = reinterpret_cast<float*>(sC);          // [4 waves][64 lanes][16]
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            red[(wave * 64 + lane) * 16 + q] = ep_active ? ssum[q] : 0.f;
            red[(wave * 64 + lane) * 16 + 8 + q] = ep_active ? ssq[q] : 0.f;
        }
        __syncthreads();
        for (int c = tid; c < C0; c += 256) {
            float s = 0.f, s2 = 0.f;
            for (int w = 0; w < 4; ++w)
                for (int r = 0; r < slots; ++r) {
                    const float* p = red + (w * 64 + r * C8 + (c >> 3)) * 16 + (c & 7);
                    s += p[0]; s2 += p[8];
                }
            float* dst = stat_partials + (long long)blockIdx.x * 2 * C0;
            dst[c] = s;
            dst[C0 + c] = s2;
        }
    }
}

// --------------------------------------------------------------------------------------------------------- weight gradient
// 16x16x32 MFMA operand fragment of a row-major bf16 LDS tile, read transposed (gemm_wgrad_rows.hip: tr_frag): lane
// (i = l&15, g = l>>4) receives rows row0 + g*8 + 0..7 of column col0 + i
__device__ __forceinline__ bf16x8_t tr_frag(const unsigned char* tile, int rs, int row0, int col0, int lane) {
    const int g = lane >> 4, i = lane & 15;
    const unsigned char* a = tile + (size_t)(row0 + g * 8 + (i >> 2)) * rs + (col0 + (i & 3) * 4) * 2;
    s4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(a));
    s4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(a + 4 * rs));
    typedef __attribute__((ext_vector_type(8))) short s8_t;
    s8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, v);
}

// The reduction runs over the pixels.  de rows of the tile are staged row-major ([SR * TW pixels][NP channels], channels past
// c0 and pixels outside the map zero) and read transposed as the A operand; the B operand of patch column k is 8 consecutive
// output pixels of one (channel, kernel row, kernel column) of the image tile.  Every wave keeps a [NP x 32] partial of its tile
// rows in accumulators; the four are summed in wave order when the workgroup is done and its partial goes to ws[block], which
// stem_wgrad_reduce_k sums in block order: no atomics, the same bits every run.
// BN: `de` is dZ0 = dL/d bn0(e) and the BatchNorm0 backward apply, de = coef[0]*dZ0 + coef[1]*e + coef[2] (mc_bnact_bwd_apply
// without activation or factors: bnact_bwd_k<true, false, false>), is formed while the tile is staged -- in fp32, rounded to
// 16 bits where that kernel rounds its output, so the MFMA sees the operand the separate pass would have written.
template <typename SRC, int C8, bool BN>
__global__ __launch_bounds__(256) void stem_conv_wgrad_k(const stem_geo g, const bf16_t* __restrict__ de, const bf16_t* __restrict__ e,
                                                         const float* __restrict__ coef, float* __restrict__ ws) {
    constexpr int FN = (C8 + 1) / 2, NP = FN * 16, C0 = C8 * 8;
    constexpr int RSY = NP * 2;                             // de tile row pitch in bytes
    constexpr int NPIX = SR * TW;
    constexpr int Y_BYTES = (NPIX * RSY > 4 * NP * 32 * 4) ? NPIX * RSY : 4 * NP * 32 * 4;
    constexpr int YSLOTS = (NPIX * C8 + 255) / 256;
    __shared__ __attribute__((aligned(16))) unsigned char sImg[IMG_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char sY[Y_BYTES];
    __shared__ __attribute__((aligned(16))) float sCoef[BN ? 3 * C0 : 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kg = lane >> 4;

    for (int i = tid; i < RSI / 2; i += 256) reinterpret_cast<unsigned int*>(sImg + ZOFF)[i] = 0u;
    if constexpr (BN)
        for (int i = tid; i < 3 * C0; i += 256) sCoef[i] = coef[i];
    for (int i = tid; i < NPIX * RSY / 16; i += 256) reinterpret_cast<uint4*>(sY)[i] = make_uint4(0u, 0u, 0u, 0u);   // (channels c0 .. NP-1 stay zero)
    unsigned meta[ISLOTS];
    img_meta(tid, meta);
    unsigned off[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) off[kt] = patch_off(kt * 16 + j, wave) + (unsigned)(kg * 32);
    f32x4_t acc[FN][2];
#pragma unroll
    for (int f = 0; f < FN; ++f)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) acc[f][kt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    uint4 raw[ISLOTS], yraw[YSLOTS], eraw[BN ? YSLOTS : 1];
    auto y_load = [&](long long t) {
        int img, oy0, ox0;
        tile_origin(g, t, img, oy0, ox0);
#pragma unroll
        for (int s = 0; s < YSLOTS; ++s) {
            const int ci = tid + s * 256;
            const int pl = ci / C8, ch = ci - pl * C8;
            const int oy = oy0 + (pl / TW), ox = ox0 + (pl % TW);
            yraw[s] = make_uint4(0u, 0u, 0u, 0u);
            if constexpr (BN) eraw[s] = make_uint4(0u, 0u, 0u, 0u);
            if (pl < NPIX && oy < g.oh && ox < g.ow) {
                const long long o = (((long long)img * g.oh + oy) * g.ow + ox) * C0 + ch * 8;
                yraw[s] = *reinterpret_cast<const uint4*>(de + o);
                if constexpr (BN) eraw[s] = *reinterpret_cast<const uint4*>(e + o);
            }
        }
    };
    auto y_store = [&](long long t) {
        int img, oy0, ox0;
        tile_origin(g, t, img, oy0, ox0);
#pragma unroll
        for (int s = 0; s < YSLOTS; ++s) {
            const int ci = tid + s * 256;
            const int pl = ci / C8, ch = ci - pl * C8;
            if (pl >= NPIX) continue;
            uint4 v = yraw[s];
            if constexpr (BN) {
                if (oy0 + (pl / TW) < g.oh && ox0 + (pl % TW) < g.ow) {        // (pixels outside the map stay zero)
                    float dz[8], x[8], k0[8], k1[8], k2[8];
                    unpack8(yraw[s], dz);
                    unpack8(eraw[s], x);
                    load8f(sCoef + ch * 8, k0); load8f(sCoef + C0 + ch * 8, k1); load8f(sCoef + 2 * C0 + ch * 8, k2);
#pragma unroll
                    for (int q = 0; q < 8; ++q) dz[q] = k0[q] * dz[q] + k1[q] * x[q] + k2[q];
                    v = pack8(dz);
                }
            }
            *reinterpret_cast<uint4*>(sY + pl * RSY + ch * 16) = v;
        }
    };

    long long t = blockIdx.x;
    if (t < g.tiles) { img_load<SRC>(g, t, meta, raw); y_load(t); }
    for (; t < g.tiles; t += gridDim.x) {
        __syncthreads();
        img_store<SRC>(g, t, meta, raw, sImg);
        y_store(t);
        __syncthreads();
        if (t + gridDim.x < g.tiles) { img_load<SRC>(g, t + gridDim.x, meta, raw); y_load(t + gridDim.x); }
#pragma unroll
        for (int ks = 0; ks < TW / 32; ++ks) {
            bf16x8_t b[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                const unsigned char* pb = sImg + off[kt] + ks * 128;
                b[kt] = gather8(pb, pb + 4, pb + 8, pb + 12, pb + 16, pb + 20, pb + 24, pb + 28);
            }
#pragma unroll
            for (int f = 0; f < FN; ++f) {
                const bf16x8_t a = tr_frag(sY, RSY, wave * TW + ks * 32, f * 16, lane);
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) acc[f][kt] = MC_MFMA_16x16x32(a, b[kt], acc[f][kt], 0, 0, 0);
            }
        }
    }
    // D[i][j]: i = output channel (A operand), j = patch column (B operand)
    __syncthreads();
    float* red = reinterpret_cast<float*>(sY);              // [4 waves][NP][32]
#pragma unroll
    for (int f = 0; f < FN; ++f)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[(wave * NP + f * 16 + kg * 4 + r) * 32 + kt * 16 + j] = acc[f][kt][r];
    __syncthreads();
    float* dst = ws + (long long)blockIdx.x * C0 * 32;
    for (int i = tid; i < C0 * 32; i += 256)
        dst[i] = ((red[i] + red[NP * 32 + i]) + red[2 * NP * 32 + i]) + red[3 * NP * 32 + i];
}

// dW[i] = sum over the workgroup partials, in block order
__global__ __launch_bounds__(256) void stem_wgrad_reduce_k(const float* __restrict__ ws, int parts, int nk, float* __restrict__ dw) {
    __shared__ float sh[16][17];
    const int el = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + el;
    float s = 0.f;
    if (i < nk) {
        int k = pl;
        for (; k + 48 < parts; k += 64) {                     // four independent loads in flight, summed in part order
            const float a = ws[(long long)k * nk + i], b = ws[(long long)(k + 16) * nk + i];
            const float c = ws[(long long)(k + 32) * nk + i], d = ws[(long long)(k + 48) * nk + i];
            s += a; s += b; s += c; s += d;
        }
        for (; k < parts; k += 16) s += ws[(long long)k * nk + i];
    }
    sh[pl][el] = s;
    __syncthreads();
    if (pl != 0 || i >= nk) return;
    s = 0.f;
    for (int k = 0; k < 16; ++k) s += sh[k][el];
    dw[i] = s;
}

int make_geo(stem_geo& g, const void* x, int elem, long long sn, long long sh, const unsigned int* mm, float mean, float stdv, int n,
             int h, int w, int pad_l, int pad_t, int oh, int ow) {
    g.x = x; g.sn = sn; g.sh = sh; g.mm = mm; g.mean = mean; g.stdv = stdv;
    g.n = n; g.h = h; g.w = w; g.pad_l = pad_l; g.pad_t = pad_t; g.oh = oh; g.ow = ow;
    g.tx = (ow + TW - 1) / TW; g.ty = (oh + SR - 1) / SR;
    g.tiles = (long long)n * g.tx * g.ty;
    // one vector load per chunk (16 bytes of fp32 / 4 bytes of uint8: 4 elements), aligned in every row of every image
    g.vec = (((uintptr_t)x) % (size_t)(4 * elem) == 0 && sn % 4 == 0 && sh % 4 == 0 && pad_l == 0) ? 1 : 0;
    return MC_OK;
}

int check_geo(const void* x, long long sn, long long sh, int n, int h, int w, int pad_l, int pad_t, int oh, int ow, int c0) {
    MC_CHECK(x && n > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "stem_conv: bad args");
    MC_CHECK(c0 >= 32 && c0 <= 64 && c0 % 8 == 0, "stem_conv: 32 <= c0 <= 64 output channels, a multiple of 8");
    MC_CHECK(pad_l >= 0 && pad_l <= 2 && pad_t >= 0 && pad_t <= 2, "stem_conv: left / top padding of 0 .. 2");
    // (taps outside the image are the zero padding, whatever oh / ow ask for; the strides of a size-1 extent mean nothing)
    MC_CHECK((h == 1 || sh >= 3LL * w) && (n == 1 || sn >= sh * (long long)(h - 1) + 3LL * w), "stem_conv: strides of a channels-last image");
    return MC_OK;
}

}  // namespace

// workgroups of the launches below for n images of oh x ow outputs = rows of stat_partials (kind 1: forward) / of the
// weight-gradient workspace (kind 0; kind 2: its BatchNorm0 form).  At most what is resident at once: 4 / 3 / 2 workgroups on
// each of the 256 CUs (115 / 136 / 168 registers)
extern "C" int mc_stem_conv_blocks(int n, int oh, int ow, int kind) {
    if (n <= 0 || oh <= 0 || ow <= 0 || kind < 0 || kind > 2) return 0;
    const long long tiles = (long long)n * ((ow + TW - 1) / TW) * ((oh + SR - 1) / SR);
    const long long cap = kind == 1 ? 1024 : (kind == 0 ? 768 : 512);
    return (int)(tiles < cap ? tiles : cap);
}

#define STEM_C8_SWITCH(KERNEL, TARGS, ...)                                                                                 \
    switch (c0 / 8) {                                                                                                      \
        case 4: hipLaunchKernelGGL((KERNEL<TARGS(4)>), dim3(blocks), dim3(256), 0, st, __VA_ARGS__); break;                \
        case 5: hipLaunchKernelGGL((KERNEL<TARGS(5)>), dim3(blocks), dim3(256), 0, st, __VA_ARGS__); break;                \
        case 6: hipLaunchKernelGGL((KERNEL<TARGS(6)>), dim3(blocks), dim3(256), 0, st, __VA_ARGS__); break;                \
        case 7: hipLaunchKernelGGL((KERNEL<TARGS(7)>), dim3(blocks), dim3(256), 0, st, __VA_ARGS__); break;                \
        default: hipLaunchKernelGGL((KERNEL<TARGS(8)>), dim3(blocks), dim3(256), 0, st, __VA_ARGS__); break;        \
    }
#define T_F32(c8) float, c8
#define T_U8(c8) unsigned char, c8
#define T_F32_W(c8) float, c8, false
#define T_U8_W(c8) unsigned char, c8, false
#define T_F32_WBN(c8) float, c8, true
#define T_U8_WBN(c8) unsigned char, c8, true

static int stem_fwd(const void* x, bool u8, long long sn, long long sh, const unsigned int* mm, float mean, float stdv, int n, int h,
                    int w, int pad_l, int pad_t, int oh, int ow, const mc_bf16* wb, int c0, mc_bf16* e, float* stat_partials,
                    void* stream) {
    if (int rc = check_geo(x, sn, sh, n, h, w, pad_l, pad_t, oh, ow, c0)) return rc;
    MC_CHECK(wb && e && mc_aligned16(wb) && mc_aligned16(e), "stem_conv_fwd: weight image and output must be 16-byte aligned");
    stem_geo g;
    make_geo(g, x, u8 ? 1 : 4, sn, sh, mm, mean, stdv, n, h, w, pad_l, pad_t, oh, ow);
    const int blocks = mc_stem_conv_blocks(n, oh, ow, 1);
    hipStream_t st = (hipStream_t)stream;
    if (u8) { STEM_C8_SWITCH(stem_conv_fwd_k, T_U8, g, wb, e, stat_partials) }
    else { STEM_C8_SWITCH(stem_conv_fwd_k, T_F32, g, wb, e, stat_partials) }
    MC_LAUNCH_CHECK();
    return MC_OK;
}

extern "C" int mc_stem_conv_fwd(const float* x, long long sn, long long sh, int n, int h, int w, int pad_l, int pad_t, int oh,
                                int ow, const mc_bf16* wb, int c0, mc_bf16* e, float* stat_partials, void* stream) {
    return stem_fwd(x, false, sn, sh, nullptr, 0.f, 1.f, n, h, w, pad_l, pad_t, oh, ow, wb, c0, e, stat_partials, stream);
}

extern "C" int mc_stem_conv_fwd_u8(const unsigned char* x, long long sn, long long sh, const unsigned int* minmax, float mean,
                                   float std, int n, int h, int w, int pad_l, int pad_t, int oh, int ow, const mc_bf16* wb, int c0,
                                   mc_bf16* e, float* stat_partials, void* stream) {
    MC_CHECK(minmax && std != 0.f, "stem_conv_fwd_u8: bad args");
    return stem_fwd(x, true, sn, sh, minmax, mean, std, n, h, w, pad_l, pad_t, oh, ow, wb, c0, e, stat_partials, stream);
}

extern "C" int mc_stem_conv_wgrad(const void* x, int is_u8, long long sn, long long sh, const unsigned int* minmax, float mean,
                                  float std, int n, int h, int w, int pad_l, int pad_t, int oh, int ow, const mc_bf16* de, int c0,
                                  const mc_bf16* bn_e, const float* bn_coef, float* ws, float* dw, void* stream) {
    if (int rc = check_geo(x, sn, sh, n, h, w, pad_l, pad_t, oh, ow, c0)) return rc;
    MC_CHECK(de && ws && dw && mc_aligned16(de), "stem_conv_wgrad: bad args");
    MC_CHECK((bn_e == nullptr) == (bn_coef == nullptr) && mc_aligned16(bn_e), "stem_conv_wgrad: the BatchNorm form needs e (16-byte aligned) and coef");
    MC_CHECK(!is_u8 || (minmax && std != 0.f), "stem_conv_wgrad: uint8 source needs minmax and std");
    stem_geo g;
    make_geo(g, x, is_u8 ? 1 : 4, sn, sh, minmax, mean, is_u8 ? std : 1.f, n, h, w, pad_l, pad_t, oh, ow);
    const int blocks = mc_stem_conv_blocks(n, oh, ow, bn_e ? 2 : 0);
    hipStream_t st = (hipStream_t)stream;
    const bf16_t* e = bn_e;
    if (bn_e) {
        if (is_u8) { STEM_C8_SWITCH(stem_conv_wgrad_k, T_U8_WBN, g, de, e, bn_coef, ws) }
        else { STEM_C8_SWITCH(stem_conv_wgrad_k, T_F32_WBN, g, de, e, bn_coef, ws) }
    } else {
        if (is_u8) { STEM_C8_SWITCH(stem_conv_wgrad_k, T_U8_W, g, de, e, bn_coef, ws) }
        else { STEM_C8_SWITCH(stem_conv_wgrad_k, T_F32_W, g, de, e, bn_coef, ws) }
    }
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(stem_wgrad_reduce_k, dim3(mc_div_up(c0 * 32, 16)), dim3(256), 0, st, ws, blocks, c0 * 32, dw);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
