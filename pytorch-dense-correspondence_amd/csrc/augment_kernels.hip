// Training-image augmentation on the device: the two steps every within-scene sample of the reference goes through
// (dense_correspondence/dataset/spartan_dataset_masked.py:667-680) and the ToTensor + Normalize that follows (:297-304), for
// device-resident images.  Mirrors dense_correspondence/correspondence_tools/correspondence_augmentation.py:
//   random_domain_randomize_background (:86-94) / domain_randomize_background (:96-123): rgb*m + (1-m)*bg in uint8
//       arithmetic, bg from get_random_image (:125-146): a solid colour (get_random_rgb, :148-153: uint8(U*255), 0..254) or
//       get_gradient_image (:180-199: uint8(rgb2*p + rgb1*(1.0-p)) in float64, p = numpy.linspace(0, 1, n) along rows if
//       `vertical`, along columns otherwise), then add_noise (:201-215): bg + n1 - n2 mod 256, n1, n2 = uint8(U*50)
//   random_image_and_indices_mutation (:19-56) = flip_vertical (:59-69) then flip_horizontal (:72-83): a 180-degree rotation
//       of every image of the list, and (u, v) -> ((W-1) - u, (H-1) - v)
// Background randomization runs on the UNROTATED image, so the gradient position and the noise index of an output pixel are
// those of its SOURCE pixel.
//
//   augment_kernel      one pass over a batch: uint8 HWC RGB + uint8 mask in; float NCHW network input, uint8 HWC RGB and
//                       float 0/1 mask out (each optional).  20 bytes per pixel with the network input and the float mask:
//                       HBM bound -- two groups of 4 output pixels per work-item (12-byte RGB / 4-byte mask loads, all
//                       issued up front; 16-byte stores), the (c, x) -> (x / 255 - mean_c) / std_c table (IEEE divisions,
//                       as torch) built once per workgroup while those loads are in flight.
//   flip_planes_kernel  vertical / horizontal flip of [planes][h][w] pixels of any size (uint8 RGB, masks, 16-bit depth ...)
//   flip_uv_kernel      (u, v) -> ((W-1) - u, (H-1) - v), int64 or float32, per image of a concatenated list
//
// Noise of the batched path comes from a counter-based hash of (seed, image, source pixel, channel): launch geometry does
// not change it and the same record gives the same bits.  The mirror path passes the reference's own host-drawn noise
// instead, as one (n1 - n2) mod 256 plane.
#include "dcn_common.h"
#include "image_norm.h"

#pragma clang fp contract(off)   // (the build passes -ffp-contract=off as well; the gradient must not fuse into an FMA)

namespace {

constexpr int kAugThreads = 256;
constexpr int kAugPix = 4;      // output pixels per group
constexpr int kAugGroups = 2;   // groups per work-item

struct AugArgs {
    const unsigned char* rgb[2];     // side a, side b: [n][h][w][3]
    const unsigned char* mask[2];    // [n][h][w]
    float* net[2];                   // [n][3][h][w] or null
    unsigned char* rgb_out[2];       // [n][h][w][3] or null
    float* mask_out[2];              // [n][h][w] or null
    const int32_t* params;           // [sides * n][DCN_AUG_PARAM_WORDS]
    const unsigned char* noise;      // [sides * n][h][w][3] (n1 - n2) mod 256, or null: the hash
    float mean[3], std[3];
    double step_v, step_h;           // 1 / (h - 1), 1 / (w - 1) (0 for a single row / column), as numpy.linspace
    int n, h, w, vec;
};

__device__ __forceinline__ uint32_t mix32(uint32_t x) {   // a 32-bit integer finaliser (bijective)
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}

struct NoiseKey {
    uint32_t k0, k1;
};

__device__ __forceinline__ NoiseKey noise_key(uint32_t seed_lo, uint32_t seed_hi, uint32_t image) {
    NoiseKey k;
    k.k0 = mix32(seed_lo ^ mix32(image * 0x9E3779B9U + 0x7F4A7C15U));
    k.k1 = mix32(seed_hi ^ k.k0);
    return k;
}

// (n1 - n2) mod 256 of element e = 3 * source pixel + channel: n1, n2 = (16-bit field * 50) >> 16, uniform on 0..49 (each
// value has probability 1310 / 65536 or 1311 / 65536)
__device__ __forceinline__ uint32_t noise_diff(NoiseKey k, uint32_t e) {
    const uint32_t r = mix32(mix32(e ^ k.k0) ^ k.k1);
    return (((r >> 16) * 50U) >> 16) - (((r & 0xffffU) * 50U) >> 16);
}

struct Record {
    bool fv, fh, rnd, grad, vert, noise;
    uint32_t c1[3], c2[3];
    NoiseKey key;
};

__device__ __forceinline__ Record load_record(const int32_t* p, uint32_t image) {
    Record r;
    const uint32_t f = (uint32_t)p[0];
    r.fv = f & DCN_AUG_FLIP_V;
    r.fh = f & DCN_AUG_FLIP_H;
    r.rnd = f & DCN_AUG_RANDOMIZE;
    r.grad = f & DCN_AUG_GRADIENT;
    r.vert = f & DCN_AUG_VERTICAL;
    r.noise = f & DCN_AUG_NOISE;
    for (int c = 0; c < 3; ++c) {
        r.c1[c] = (uint32_t)p[1 + c] & 0xffU;
        r.c2[c] = (uint32_t)p[4 + c] & 0xffU;
    }
    r.key = noise_key((uint32_t)p[8], (uint32_t)p[9], image);
    return r;
}

// The background colour of source pixel (sy, sx) before noise.
__device__ __forceinline__ void background(const Record& r, const AugArgs& a, int sy, int sx, uint32_t bg[3]) {
    if (!r.grad) {
        for (int c = 0; c < 3; ++c) bg[c] = r.c1[c];
        return;
    }
    const int t = r.vert ? sy : sx, len = r.vert ? a.h : a.w;
    const double p = (len > 1 && t == len - 1) ? 1.0 : (double)t * (r.vert ? a.step_v : a.step_h);
    const double q = 1.0 - p;
    for (int c = 0; c < 3; ++c) bg[c] = (uint32_t)((double)r.c2[c] * p + (double)r.c1[c] * q);   // truncation, as numpy
}

// Output RGB of one pixel: src, mask byte m, source coordinates; noise (when set) from `nz` (mem_noise: read from memory)
// or the hash.
__device__ __forceinline__ void blend(const Record& r, const AugArgs& a, int sy, int sx, const uint32_t src[3], uint32_t m,
                                      bool mem_noise, const uint32_t nz[3], uint32_t out[3]) {
    if (!r.rnd) {
        for (int c = 0; c < 3; ++c) out[c] = src[c];
        return;
    }
    uint32_t bg[3];
    background(r, a, sy, sx, bg);
    if (r.noise) {
        const uint32_t e = 3U * ((uint32_t)sy * (uint32_t)a.w + (uint32_t)sx);
        for (int c = 0; c < 3; ++c) bg[c] += mem_noise ? nz[c] : noise_diff(r.key, e + c);
    }
    const uint32_t mc = (1U - m) & 0xffU;
    for (int c = 0; c < 3; ++c) out[c] = (src[c] * m + mc * (bg[c] & 0xffU)) & 0xffU;   // uint8 arithmetic, as numpy
}

// Work-item t of workgroup x owns the 4-pixel groups x * kAugThreads * kAugGroups + t + j * kAugThreads, j < kAugGroups.  All
// loads are issued before the table is built (its divisions and barrier hide under their latency).
__global__ void __launch_bounds__(kAugThreads) augment_kernel(AugArgs a) {
    __shared__ float lut[3][256];
    const int img = blockIdx.y;
    const int side = img >= a.n ? 1 : 0, i = img - side * a.n;
    const Record r = load_record(a.params + (size_t)img * DCN_AUG_PARAM_WORDS, (uint32_t)img);
    const int64_t hw = (int64_t)a.h * a.w;
    const int w = a.w, h = a.h;
    const unsigned char* rgb = a.rgb[side] + (size_t)i * hw * 3;
    const unsigned char* msk = a.mask[side] + (size_t)i * hw;
    const unsigned char* noise = (r.rnd && r.noise && a.noise) ? a.noise + (size_t)img * hw * 3 : nullptr;
    unsigned char* rgb_out = a.rgb_out[side] ? a.rgb_out[side] + (size_t)i * hw * 3 : nullptr;
    float* mask_out = a.mask_out[side] ? a.mask_out[side] + (size_t)i * hw : nullptr;
    float* net = a.net[side] ? a.net[side] + (size_t)i * 3 * hw : nullptr;
    const int64_t g0 = (int64_t)blockIdx.x * kAugThreads * kAugGroups + threadIdx.x;
    if (!a.vec) {   // any width / alignment: pixel by pixel
        if (net) dcn::build_norm_table<kAugThreads>(lut, a.mean, a.std);
        for (int g = 0; g < kAugGroups; ++g) {
            for (int j = 0; j < kAugPix; ++j) {
                const int64_t p = (g0 + (int64_t)g * kAugThreads) * kAugPix + j;
                if (p >= hw) break;
                const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
                const int sy = r.fv ? h - 1 - y : y, sx = r.fh ? w - 1 - x : x;
                const int64_t sp = (int64_t)sy * w + sx;
                const uint32_t src[3] = {rgb[sp * 3], rgb[sp * 3 + 1], rgb[sp * 3 + 2]};
                const uint32_t m = msk[sp];
                uint32_t nz[3] = {0u, 0u, 0u}, px[3];
                if (noise)
                    for (int c = 0; c < 3; ++c) nz[c] = noise[sp * 3 + c];
                blend(r, a, sy, sx, src, m, noise != nullptr, nz, px);
                dcn::store_pixel(lut, p, hw, px, (float)m, net, rgb_out, mask_out);
            }
        }
        return;
    }
    // w % 4 == 0, aligned pointers: a group's 4 pixels share a row, and so do their 4 (aligned) source pixels
    uint32_t s[kAugGroups][3], nzw[kAugGroups][3], mw[kAugGroups];
    int ys[kAugGroups], x0s[kAugGroups];
#pragma unroll
    for (int g = 0; g < kAugGroups; ++g) {
        const int64_t p0 = (g0 + (int64_t)g * kAugThreads) * kAugPix;
        ys[g] = -1;
        x0s[g] = 0;
        mw[g] = 0u;
        for (int k = 0; k < 3; ++k) s[g][k] = nzw[g][k] = 0u;
        if (p0 < hw) {
            const int y = (int)(p0 / w), x0 = (int)(p0 - (int64_t)y * w);
            const int sy = r.fv ? h - 1 - y : y, sx0 = r.fh ? w - kAugPix - x0 : x0;
            const int64_t sp = (int64_t)sy * w + sx0;
            const uint32_t* s32 = reinterpret_cast<const uint32_t*>(rgb + sp * 3);
            s[g][0] = s32[0];
            s[g][1] = s32[1];
            s[g][2] = s32[2];
            mw[g] = *reinterpret_cast<const uint32_t*>(msk + sp);
            if (noise) {
                const uint32_t* n32 = reinterpret_cast<const uint32_t*>(noise + sp * 3);
                nzw[g][0] = n32[0];
                nzw[g][1] = n32[1];
                nzw[g][2] = n32[2];
            }
            ys[g] = y;
            x0s[g] = x0;
        }
    }
    if (net) dcn::build_norm_table<kAugThreads>(lut, a.mean, a.std);
#pragma unroll
    for (int g = 0; g < kAugGroups; ++g) {
        if (ys[g] < 0) continue;
        const int y = ys[g], x0 = x0s[g];
        const int sy = r.fv ? h - 1 - y : y, sx0 = r.fh ? w - kAugPix - x0 : x0;
        uint32_t sv[kAugPix][3], nv3[kAugPix][3], ms[kAugPix];   // unpacked in source order (static indices: no scratch)
#pragma unroll
        for (int q = 0; q < kAugPix; ++q) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int b = 3 * q + c;
                sv[q][c] = (s[g][b >> 2] >> (8 * (b & 3))) & 0xffU;
                nv3[q][c] = (nzw[g][b >> 2] >> (8 * (b & 3))) & 0xffU;
            }
            ms[q] = (mw[g] >> (8 * q)) & 0xffU;
        }
        uint32_t px[kAugPix][3];
        float mv[kAugPix];
#pragma unroll
        for (int j = 0; j < kAugPix; ++j) {
            const int qf = kAugPix - 1 - j;                      // output pixel j's source within the group: qf if fh, else j
            uint32_t src[3], nz[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                src[c] = r.fh ? sv[qf][c] : sv[j][c];
                nz[c] = r.fh ? nv3[qf][c] : nv3[j][c];
            }
            const uint32_t m = r.fh ? ms[qf] : ms[j];
            blend(r, a, sy, sx0 + (r.fh ? qf : j), src, m, noise != nullptr, nz, px[j]);
            mv[j] = (float)m;
        }
        dcn::store_pixels4(lut, (int64_t)y * w + x0, hw, px, mv, net, rgb_out, mask_out);
    }
}

// out[plane][y][x] = in[plane][fv ? h-1-y : y][fh ? w-1-x : x], pixels of `upp` units of T
template <class T>
__global__ void __launch_bounds__(256)
flip_planes_kernel(const T* __restrict__ in, T* __restrict__ out, int h, int w, int upp, int fv, int fh) {
    const int64_t per_plane = (int64_t)h * w * upp;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= per_plane) return;
    const int64_t base = (int64_t)blockIdx.y * per_plane;
    const int64_t pix = k / upp;
    const int u = (int)(k - pix * upp);
    const int y = (int)(pix / w), x = (int)(pix - (int64_t)y * w);
    const int sy = fv ? h - 1 - y : y, sx = fh ? w - 1 - x : x;
    out[base + k] = in[base + ((int64_t)sy * w + sx) * upp + u];
}

// Entry i of a list concatenated over n images (image b owns [offsets[b], offsets[b+1]); offsets == null: all of image 0)
// takes the flips of its image's record (params) or `flags` (params == null).  (W-1) - u in the list's type: for float32
// that is torch's `(W-1) - t`, one rounding.  Entries outside [offsets[0], offsets[n]) are copied unchanged.
template <class T>
__global__ void __launch_bounds__(256)
flip_uv_kernel(const T* __restrict__ u_in, const T* __restrict__ v_in, T* u_out, T* v_out, int64_t count,
               const int64_t* __restrict__ offsets, int n, const int32_t* __restrict__ params, int flags, int h, int w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    int img = 0;
    if (offsets) {
        if (i < offsets[0] || i >= offsets[n]) {
            img = -1;
        } else {
            int lo = 0, hi = n - 1;   // largest b with offsets[b] <= i
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (offsets[mid] <= i) lo = mid; else hi = mid - 1;
            }
            img = lo;
        }
    }
    const uint32_t f = img < 0 ? 0U : (uint32_t)(params ? params[(size_t)img * DCN_AUG_PARAM_WORDS] : flags);
    const T u = u_in[i], v = v_in[i];
    u_out[i] = (f & DCN_AUG_FLIP_H) ? (T)(w - 1) - u : u;
    v_out[i] = (f & DCN_AUG_FLIP_V) ? (T)(h - 1) - v : v;
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int dcn_augment_images(int n, int h, int w, const uint8_t* rgb_a, const uint8_t* rgb_b, const uint8_t* mask_a,
                                  const uint8_t* mask_b, const int32_t* params, const uint8_t* noise, const float* mean,
                                  const float* std, float* net_a, float* net_b, uint8_t* rgb_out_a, uint8_t* rgb_out_b,
                                  float* mask_out_a, float* mask_out_b, void* stream) {
    const int sides = rgb_b ? 2 : 1;
    if (n < 1 || h < 1 || w < 1 || (int64_t)h * w > (1LL << 30) || (int64_t)sides * n > 65535 || !rgb_a || !mask_a ||
        !params || !mean || !std || ((rgb_b == nullptr) != (mask_b == nullptr)) ||
        (sides == 1 && (net_b || rgb_out_b || mask_out_b)))
        return DCN_E_INVALID;
    AugArgs a;
    a.rgb[0] = rgb_a;
    a.rgb[1] = rgb_b;
    a.mask[0] = mask_a;
    a.mask[1] = mask_b;
    a.net[0] = net_a;
    a.net[1] = net_b;
    a.rgb_out[0] = rgb_out_a;
    a.rgb_out[1] = rgb_out_b;
    a.mask_out[0] = mask_out_a;
    a.mask_out[1] = mask_out_b;
    a.params = params;
    a.noise = noise;
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = mean[c];
        a.std[c] = std[c];
    }
    a.step_v = h > 1 ? 1.0 / (double)(h - 1) : 0.0;   // numpy.linspace(0, 1, n): i * (1.0 / (n - 1)), last = 1.0
    a.step_h = w > 1 ? 1.0 / (double)(w - 1) : 0.0;
    a.n = n;
    a.h = h;
    a.w = w;
    bool vec = (w % kAugPix) == 0;
    const void* p16[] = {net_a, net_b, mask_out_a, mask_out_b};
    const void* p4[] = {rgb_a, rgb_b, mask_a, mask_b, noise, rgb_out_a, rgb_out_b};
    for (const void* p : p16) vec = vec && aligned(p, 16);
    for (const void* p : p4) vec = vec && aligned(p, 4);
    a.vec = vec ? 1 : 0;
    const int64_t groups = dcn::ceil_div64((int64_t)h * w, kAugPix);
    const dim3 grid((unsigned)dcn::ceil_div64(groups, kAugThreads * kAugGroups), (unsigned)(sides * n));
    hipLaunchKernelGGL(augment_kernel, grid, dim3(kAugThreads), 0, (hipStream_t)stream, a);
    return dcn::check_launch();
}

extern "C" int dcn_flip_planes(const void* in, void* out, int64_t planes, int h, int w, int bytes_per_pixel, int flip_v,
                               int flip_h, void* stream) {
    if (!in || !out || in == out || planes < 1 || planes > 65535 || h < 1 || w < 1 || bytes_per_pixel < 1 ||
        bytes_per_pixel > 64 || (int64_t)h * w * bytes_per_pixel > (1LL << 40))
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)h * w;
    const int fv = flip_v ? 1 : 0, fh = flip_h ? 1 : 0;
    if (bytes_per_pixel % 4 == 0 && aligned(in, 4) && aligned(out, 4)) {
        const int upp = bytes_per_pixel / 4;
        hipLaunchKernelGGL(flip_planes_kernel<uint32_t>, dim3((unsigned)dcn::ceil_div64(hw * upp, 256), (unsigned)planes),
                           dim3(256), 0, st, (const uint32_t*)in, (uint32_t*)out, h, w, upp, fv, fh);
    } else if (bytes_per_pixel % 2 == 0 && aligned(in, 2) && aligned(out, 2)) {
        const int upp = bytes_per_pixel / 2;
        hipLaunchKernelGGL(flip_planes_kernel<uint16_t>, dim3((unsigned)dcn::ceil_div64(hw * upp, 256), (unsigned)planes),
                           dim3(256), 0, st, (const uint16_t*)in, (uint16_t*)out, h, w, upp, fv, fh);
    } else {
        hipLaunchKernelGGL(flip_planes_kernel<uint8_t>,
                           dim3((unsigned)dcn::ceil_div64(hw * bytes_per_pixel, 256), (unsigned)planes), dim3(256), 0, st,
                           (const uint8_t*)in, (uint8_t*)out, h, w, bytes_per_pixel, fv, fh);
    }
    return dcn::check_launch();
}

extern "C" int dcn_flip_uv(int uv_dtype, const void* u_in, const void* v_in, void* u_out, void* v_out, int64_t count,
                           int n_images, const int64_t* offsets, const int32_t* params, int flags, int h, int w,
                           void* stream) {
    if (!u_in || !v_in || !u_out || !v_out || count < 0 || n_images < 1 || h < 1 || w < 1 ||
        (uv_dtype != DCN_UV_INT64 && uv_dtype != DCN_UV_FLOAT32) || (offsets == nullptr && n_images != 1))
        return DCN_E_INVALID;
    if (count == 0) return DCN_OK;
    const dim3 grid((unsigned)dcn::ceil_div64(count, 256));
    hipStream_t st = (hipStream_t)stream;
    if (uv_dtype == DCN_UV_INT64)
        hipLaunchKernelGGL(flip_uv_kernel<int64_t>, grid, dim3(256), 0, st, (const int64_t*)u_in, (const int64_t*)v_in,
                           (int64_t*)u_out, (int64_t*)v_out, count, offsets, n_images, params, flags, h, w);
    else
        hipLaunchKernelGGL(flip_uv_kernel<float>, grid, dim3(256), 0, st, (const float*)u_in, (const float*)v_in,
                           (float*)u_out, (float*)v_out, count, offsets, n_images, params, flags, h, w);
    return dcn::check_launch();
}
