// Training augmentation on the device: flips, affine and elastic warp of the reference's train transform as ONE gather per
// output pixel, both views of a pair from one uint8 grayscale plane.  All integer: the specification is the docstring of
// mammo_clip_amd/augment.py, whose numpy path these kernels reproduce byte for byte.
// [ref: breastclip/data/data_utils.py:25-62 (Compose([HorizontalFlip, VerticalFlip, Affine, ElasticTransform], p));
//  data/datasets/imagetext.py:126-160 (applied twice per sample)]
//
// Two kernels per chunk of output images, both skipped (per workgroup, uniformly) for an image whose elastic bit is clear:
//   aug_hpass_k   one row segment of one displacement component: Philox noise of the segment plus its halo into LDS (eight
//                 16-bit values per Philox call), the horizontal taps from LDS, h as int16 to the workspace.
//   aug_warp_k    a 64 x 64 output tile: the (rows + 2R) x 64 column tile of h staged in LDS as pairs of rows, the vertical
//                 taps, the map, the four source taps and the three output planes.
// The tap loops hold 16-bit operands and taps below 2^15: both passes run on the packed 16-bit dot product (v_dot2c_i32_i16,
// two multiply-adds per instruction) against tap PAIRS (G(k), G(k+1)) kept for every k, so that a thread's 8 (16) consecutive
// outputs share each loaded pair of values.  The quarter-rate 32-bit multiply appears only in Philox and in the per-pixel
// 64-bit products of the map and the source address.
#include "common_hip.h"
#include "../../include/mammoclip_hip.h"

namespace {

typedef short s16x2_t __attribute__((ext_vector_type(2)));

constexpr int MAX_R = 128;          // largest tap radius
constexpr int MAX_EXT = 16384;      // largest extent: ((extent - 1) << 16) + displacement stays inside int32
constexpr int ROWLEN = 16;          // int32 values of a parameter row

constexpr int HT = 128;             // threads of an h-pass workgroup
constexpr int HPX = 8;              // consecutive outputs of a thread
constexpr int SEG = HT * HPX;       // outputs of a workgroup: one whole row of a 912-wide image
constexpr int HC_MAX = (2 * MAX_R + 15) / 8;    // 8-value chunks of a thread's window, at most

constexpr int TW = 64, TH = 64;     // output tile of the warp kernel
constexpr int VPX = 16;             // consecutive rows of a thread (256 threads: 64 columns x 4 row groups)

__device__ __forceinline__ long long rs64(long long a, int s) { return (a + (1LL << (s - 1))) >> s; }
__device__ __forceinline__ int refl(int i, int n) {     // reflect-101, single fold
    i = i < 0 ? -i : i;
    return i > n - 1 ? 2 * (n - 1) - i : i;
}

__global__ __launch_bounds__(HT) void aug_hpass_k(const int* __restrict__ params, const int* __restrict__ taps, int R, int H,
                                                  int W, int img0, short* __restrict__ hbuf, long long plane, int segs,
                                                  int vec) {
    __shared__ __attribute__((aligned(16))) short s_n[SEG + 2 * MAX_R + 16];
    __shared__ __attribute__((aligned(16))) int s_pt[8 * HC_MAX + 16];
    const int img = blockIdx.y >> 1, comp = blockIdx.y & 1;
    const int* pr = params + (long long)(img0 + img) * ROWLEN;
    if (!(pr[1] & 4)) return;                                   // no elastic on this image (uniform)
    const uint32_t seed_lo = (uint32_t)pr[9], seed_hi = (uint32_t)pr[10];
    const int y = blockIdx.x / segs, x0 = (blockIdx.x - y * segs) * SEG;
    const int tid = threadIdx.x;
    const int NC = (2 * R + 15) >> 3;                           // chunks that cover the 2R + 8 values of a thread's window

    // packed tap pairs: s_pt[q] = (G(q - 8), G(q - 7)), G(k) = taps[k] inside [0, 2R] and 0 outside
    for (int q = tid; q < 8 * NC + 8; q += HT) {
        const int k0 = q - 8, k1 = q - 7;
        const int g0 = (k0 >= 0 && k0 <= 2 * R) ? taps[k0] : 0;
        const int g1 = (k1 >= 0 && k1 <= 2 * R) ? taps[k1] : 0;
        s_pt[q] = (g0 & 0xffff) | (g1 << 16);
    }

    // noise of columns [lo, hi] of row y at LDS position x - xa
    const int xa = x0 - R, xb = min(x0 + SEG, W) - 1 + R;
    const int lo = max(xa, 0), hi = min(xb, W - 1);
    const int rowbase = y * W;                                  // H * W <= 2^28
    const int ga = (rowbase + lo) >> 3, gb = (rowbase + hi) >> 3;
    for (int gi = ga + tid; gi <= gb; gi += HT) {
        const uint4 r = philox4x32((uint32_t)gi, 0u, (uint32_t)comp, 0x5bd1e995u, seed_lo, seed_hi);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int x = gi * 8 + e - rowbase;
            const uint32_t half = (e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu);
            if (x >= lo && x <= hi) s_n[x - xa] = (short)(half ^ 0x8000u);      // half - 32768
        }
    }
    __syncthreads();
    // halo outside the row: reflect-101 (reads generated positions only, writes positions outside [lo, hi] only)
    for (int p = tid; p <= xb - xa; p += HT) {
        const int x = xa + p;
        if (x < 0 || x > W - 1) s_n[p] = s_n[refl(x, W) - xa];
    }
    __syncthreads();

    int acc[HPX];
#pragma unroll
    for (int o = 0; o < HPX; ++o) acc[o] = 0;
    const uint4* np = reinterpret_cast<const uint4*>(s_n + HPX * tid);
    for (int c = 0; c < NC; ++c) {
        const uint4 d = np[c];
        const uint32_t dd[4] = {d.x, d.y, d.z, d.w};
        uint32_t pt[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 t = *reinterpret_cast<const uint4*>(s_pt + 8 * c + 4 * q);
            pt[4 * q] = t.x; pt[4 * q + 1] = t.y; pt[4 * q + 2] = t.z; pt[4 * q + 3] = t.w;
        }
        // value j = 8c + 2p (+1) of the window meets output o with tap G(j - o): pair index 8c + 2p - o + 8
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int o = 0; o < HPX; ++o)
                acc[o] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2_t, dd[p]), __builtin_bit_cast(s16x2_t, pt[2 * p - o + 8]),
                                                acc[o], false);
    }

    const int x = x0 + HPX * tid;
    if (x >= W) return;
    short* out = hbuf + ((long long)img * 2 + comp) * plane + rowbase + x;
    if (vec) {                                                  // W % 8 == 0: all eight are inside, 16-byte aligned
        uint4 v;
        v.x = (uint32_t)((acc[0] + 16384) >> 15 & 0xffff) | ((uint32_t)((acc[1] + 16384) >> 15) << 16);
        v.y = (uint32_t)((acc[2] + 16384) >> 15 & 0xffff) | ((uint32_t)((acc[3] + 16384) >> 15) << 16);
        v.z = (uint32_t)((acc[4] + 16384) >> 15 & 0xffff) | ((uint32_t)((acc[5] + 16384) >> 15) << 16);
        v.w = (uint32_t)((acc[6] + 16384) >> 15 & 0xffff) | ((uint32_t)((acc[7] + 16384) >> 15) << 16);
        *reinterpret_cast<uint4*>(out) = v;
    } else {
#pragma unroll
        for (int o = 0; o < HPX; ++o)
            if (x + o < W) out[o] = (short)((acc[o] + 16384) >> 15);
    }
}

// v of 16 consecutive rows of one column for one component: the column tile of h is staged (rows y0 - R .. of the tile,
// reflected at the image border) as PAIRS of rows, one dword per column, then every staged pair meets the 16 outputs it belongs
// to in one packed dot product each
__device__ __forceinline__ void vpass(const short* __restrict__ hsrc, uint32_t* s_h, const uint32_t* s_pt, int LR2, int NCV,
                                      int R, int H, int W, int x0, int y0, int col, int rg, int tid, int* v) {
    __syncthreads();                                            // the previous component's readers are done
    for (int e = tid; e < LR2 * TW; e += 256) {
        const int pr = e >> 6, cx = e & 63;
        // rows past the last needed one: any valid row
        const int ya = min(max(refl(y0 - R + 2 * pr, H), 0), H - 1), yb = min(max(refl(y0 - R + 2 * pr + 1, H), 0), H - 1);
        uint32_t pair = 0;
        if (x0 + cx < W)
            pair = (uint32_t)(unsigned short)hsrc[(long long)ya * W + x0 + cx] |
                   ((uint32_t)(unsigned short)hsrc[(long long)yb * W + x0 + cx] << 16);
        s_h[e] = pair;
    }
    __syncthreads();
#pragma unroll
    for (int o = 0; o < VPX; ++o) v[o] = 0;
    const uint32_t* hp = s_h + (rg * (VPX / 2)) * TW + col;
    for (int c = 0; c < NCV; ++c) {
        uint32_t pt[24];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const uint4 t = *reinterpret_cast<const uint4*>(s_pt + 8 * c + 4 * q);
            pt[4 * q] = t.x; pt[4 * q + 1] = t.y; pt[4 * q + 2] = t.z; pt[4 * q + 3] = t.w;
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const uint32_t hv = hp[(4 * c + p) * TW];
            // staged rows j = 8c + 2p (+1) of the thread's window meet output o with taps G(j - o), G(j + 1 - o): pair 8c + 2p - o + 16
#pragma unroll
            for (int o = 0; o < VPX; ++o)
                v[o] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2_t, hv), __builtin_bit_cast(s16x2_t, pt[2 * p - o + 16]), v[o],
                                              false);
        }
    }
}

__global__ __launch_bounds__(256) void aug_warp_k(const unsigned char* __restrict__ src, long long sn, long long sh, long long sw,
                                                  int n_src, const int* __restrict__ params, const int* __restrict__ taps, int R,
                                                  int H, int W, int img0, const short* __restrict__ hbuf, long long plane,
                                                  unsigned char* __restrict__ dst, int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NCV = (2 * R + 23) >> 3;                          // chunks that cover the 2R + 16 rows of a thread's window
    const int LR = (TH - VPX) + 8 * NCV;                        // staged rows (>= TH + 2R)
    uint32_t* s_pt = reinterpret_cast<uint32_t*>(smem);          // tap pairs (G(q - 16), G(q - 15)), q in [0, 8 NCV + 16)
    uint32_t* s_h = s_pt + 8 * NCV + 16;                        // LR / 2 row pairs x 64 columns
    const int img = blockIdx.y, tid = threadIdx.x;
    const int col = tid & 63, rg = tid >> 6;
    const int ty = blockIdx.x / tiles_x, y0 = ty * TH, x0 = (blockIdx.x - ty * tiles_x) * TW;
    const int* pr = params + (long long)(img0 + img) * ROWLEN;
    const int sidx = pr[0], flags = pr[1];
    const int m00 = pr[2], m01 = pr[3], m10 = pr[4], m11 = pr[5], b0 = pr[6], b1 = pr[7], alpha = pr[8];
    const bool elastic = (flags & 4) != 0;                      // uniform per workgroup

    int v0[VPX], v1[VPX];
    if (elastic) {
        for (int q = tid; q < 8 * NCV + 16; q += 256) {
            const int k0 = q - 16, k1 = q - 15;
            const int g0 = (k0 >= 0 && k0 <= 2 * R) ? taps[k0] : 0;
            const int g1 = (k1 >= 0 && k1 <= 2 * R) ? taps[k1] : 0;
            s_pt[q] = (uint32_t)(g0 & 0xffff) | ((uint32_t)g1 << 16);
        }
        const short* h0 = hbuf + (long long)img * 2 * plane;
        vpass(h0, s_h, s_pt, LR / 2, NCV, R, H, W, x0, y0, col, rg, tid, v0);
        vpass(h0 + plane, s_h, s_pt, LR / 2, NCV, R, H, W, x0, y0, col, rg, tid, v1);
    }

    const int x = x0 + col;
    if (x >= W) return;
    const bool src_ok = sidx >= 0 && sidx < n_src;              // ops rejects such a row; never read outside the source
    const unsigned char* sp = src + (long long)sidx * sn;
    const long long hw = (long long)H * W;
    unsigned char* dp = dst + (long long)(img0 + img) * 3 * hw;
#pragma unroll
    for (int o = 0; o < VPX; ++o) {
        const int y = y0 + rg * VPX + o;
        if (y >= H) break;
        int qx = x << 16, qy = y << 16;
        if (elastic) {
            const int lx = (W - 1) << 16, ly = (H - 1) << 16;
            qx += (int)rs64((long long)alpha * v0[o], 22);
            qy += (int)rs64((long long)alpha * v1[o], 22);
            qx = qx < 0 ? -qx : qx; qx = qx > lx ? 2 * lx - qx : qx; qx = min(max(qx, 0), lx);
            qy = qy < 0 ? -qy : qy; qy = qy > ly ? 2 * ly - qy : qy; qy = min(max(qy, 0), ly);
        }
        long long sx = rs64(rs64((long long)m00 * qx + (long long)m01 * qy, 16) + b0, 8);
        long long sy = rs64(rs64((long long)m10 * qx + (long long)m11 * qy, 16) + b1, 8);
        if (flags & 1) sx = ((long long)(W - 1) << 8) - sx;
        if (flags & 2) sy = ((long long)(H - 1) << 8) - sy;
        const long long ixl = sx >> 8, iyl = sy >> 8;
        unsigned char res = 0;
        if (src_ok && ixl >= -1 && ixl <= W - 1 && iyl >= -1 && iyl <= H - 1) {
            const int ix = (int)ixl, iy = (int)iyl, fx = (int)(sx & 255), fy = (int)(sy & 255);
            const bool xl = ix >= 0, xr = ix + 1 < W, yt = iy >= 0, yb = iy + 1 < H;
            const unsigned char* p = sp + (long long)iy * sh + (long long)ix * sw;
            const int a = (yt && xl) ? p[0] : 0, b = (yt && xr) ? p[sw] : 0;
            const int c = (yb && xl) ? p[sh] : 0, d = (yb && xr) ? p[sh + sw] : 0;
            const int sum = (256 - fx) * (256 - fy) * a + fx * (256 - fy) * b + (256 - fx) * fy * c + fx * fy * d;
            res = (unsigned char)((sum + 32768) >> 16);
        }
        const long long off = (long long)y * W + x;
        dp[off] = res; dp[off + hw] = res; dp[off + 2 * hw] = res;
    }
}

// shorts of one displacement component of one image in the workspace (a multiple of 8: 16-byte aligned planes)
long long aug_plane(int h, int w) { return (((long long)h * w) + 7) & ~7LL; }

int g_stages = 3;   // bit 0: aug_hpass_k, bit 1: aug_warp_k

}  // namespace

extern "C" long long mc_augment_ws_bytes(int n_out, int h, int w) {
    if (n_out <= 0 || h <= 0 || w <= 0 || h > MAX_EXT || w > MAX_EXT) return 0;
    return (long long)n_out * 2 * aug_plane(h, w) * (long long)sizeof(short);
}

extern "C" int mc_augment_set_stages(int mask) {
    MC_CHECK(mask >= 1 && mask <= 3, "augment_set_stages: mask outside [1, 3]");
    g_stages = mask;
    return MC_OK;
}

extern "C" int mc_augment_u8(const unsigned char* src, long long sn, long long sh, long long sw, int n_src, const int* params,
                             int n_out, const int* taps, int radius, int h, int w, unsigned char* dst, void* ws,
                             long long ws_bytes, void* stream) {
    MC_CHECK(src && params && taps && dst && ws, "augment_u8: null pointer");
    MC_CHECK(n_src > 0 && n_out > 0, "augment_u8: no images");
    MC_CHECK(h >= 1 && w >= 1 && h <= MAX_EXT && w <= MAX_EXT, "augment_u8: extents outside [1, 16384]");
    MC_CHECK(radius >= 1 && radius <= MAX_R && radius <= (h < w ? h : w) - 1, "augment_u8: radius outside [1, min(128, min(h, w) - 1)]");
    const long long per_img = mc_augment_ws_bytes(1, h, w), plane = aug_plane(h, w);
    MC_CHECK(ws_bytes >= per_img, "augment_u8: ws_bytes below mc_augment_ws_bytes(1, h, w)");
    MC_CHECK((((uintptr_t)ws) & 1u) == 0, "augment_u8: ws must be 2-byte aligned");
    long long fit = ws_bytes / per_img;
    const int chunk = (int)(fit < 32767 ? fit : 32767);
    const int segs = mc_div_up(w, SEG), tiles_x = mc_div_up(w, TW), tiles_y = mc_div_up(h, TH);
    const int vec = (w % 8 == 0) && mc_aligned16(ws);
    const int ncv = (2 * radius + 23) >> 3;
    const size_t lds = (size_t)(8 * ncv + 16) * sizeof(int) + (size_t)((TH - VPX) + 8 * ncv) * TW * sizeof(short);
    for (int i0 = 0; i0 < n_out; i0 += chunk) {
        const int nc = n_out - i0 < chunk ? n_out - i0 : chunk;
        if (g_stages & 1) {
            hipLaunchKernelGGL(aug_hpass_k, dim3(segs * h, nc * 2), dim3(HT), 0, (hipStream_t)stream, params, taps, radius, h, w,
                               i0, (short*)ws, plane, segs, vec);
            MC_LAUNCH_CHECK();
        }
        if (g_stages & 2) {
            hipLaunchKernelGGL(aug_warp_k, dim3(tiles_x * tiles_y, nc), dim3(256), lds, (hipStream_t)stream, src, sn, sh, sw,
                               n_src, params, taps, radius, h, w, i0, (const short*)ws, plane, dst, tiles_x);
            MC_LAUNCH_CHECK();
        }
    }
    return MC_OK;
}
