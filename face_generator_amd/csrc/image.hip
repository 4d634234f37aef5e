// The device data path for gfx950 (wave = 64): image.scale, the warps of an HBM-resident image set (fg_warp_images, fg_warp_c2f,
// fg_warp_faces; their _u8 siblings on a set of 8-bit pixels and the _u8_y ones, luma of R, G, B bytes, are instances of the same
// kernels) and the draw of their transforms (fg_draw_transforms).  One kernel name per entry.  The gather (fg_gather_images)
// is in pointwise.hip: it shares its tile code with the layout kernels of the step path.
// Reference semantics: include/facegen_hip.h (dataset_c2f.lua:53-61, dataset.lua:95, generate_dataset.py).
#include "fg_internal.h"

// ---------------------------------------------------------------------------------------------------------------------------------
// image.scale(src, width, height) of the Torch7 `image` package, default mode 'bilinear' (dataset_c2f.lua:53-56): the width pass
// of image_(Main_scaleLinear_rowcol) over every row, then its height pass over every column of the (float) intermediate.  Per axis:
// up-scaling interpolates linearly with scale = (src - 1) / (dst - 1) (end points onto end points), down-scaling is a box mean with
// fractional coverage of the two end pixels (scale = src / dst), equal lengths copy.  One thread per output element; every product,
// sum and quotient is rounded on its own, in the reference's order (no FMA contraction) -- bit-for-bit the C loop (provenance of the
// algorithm: include/facegen_hip.h fg_scale_bilinear).  sub_from (optional): also writes diff = sub_from - result (dataset_c2f.lua:59-61).
// ---------------------------------------------------------------------------------------------------------------------------------
struct ScaleTerm { int i0, i1; float w0, w1, n; int has_last, div; };
__device__ __forceinline__ ScaleTerm fg_scale_plan(int src_len, int dst_len, int di) {
#pragma clang fp contract(off)
    ScaleTerm t;
    t.w0 = 1.f; t.w1 = 0.f; t.n = 1.f; t.has_last = 0; t.div = 0;
    if (dst_len > src_len) {
        if (src_len == 1 || di == dst_len - 1) { t.i0 = src_len - 1; t.i1 = t.i0 + 1; return t; }
        const float scale = (float)(src_len - 1) / (float)(dst_len - 1);
        float f = (float)di * scale;
        const int i = (int)f;
        f = f - (float)i;
        t.i0 = i; t.i1 = i + 1; t.w0 = 1.f - f; t.w1 = f; t.has_last = 1;
        return t;
    }
    if (dst_len < src_len) {
        const float scale = (float)src_len / (float)dst_len;
        const float s0 = (float)di * scale, s1 = (float)(di + 1) * scale;
        t.i0 = (int)s0; t.i1 = (int)s1;
        const float f0 = s0 - (float)t.i0, f1 = s1 - (float)t.i1;
        t.w0 = 1.f - f0;
        float n = t.w0;
        for (int si = t.i0 + 1; si < t.i1; ++si) n = n + 1.f;
        t.has_last = t.i1 < src_len;
        t.w1 = f1;
        if (t.has_last) n = n + f1;
        t.n = n; t.div = 1;
        return t;
    }
    t.i0 = di; t.i1 = di + 1;
    return t;
}
template <typename F>
__device__ __forceinline__ float fg_scale_eval(const ScaleTerm& t, F fetch) {
#pragma clang fp contract(off)
    float acc = t.w0 * fetch(t.i0);
    for (int si = t.i0 + 1; si < t.i1; ++si) acc = acc + fetch(si);
    if (t.has_last) { const float v = t.w1 * fetch(t.i1); acc = acc + v; }
    if (t.div) acc = acc / t.n;
    return acc;
}
// fg_scale_eval for a plan of dst_len >= src_len (no box: i1 == i0 + 1, no division), with both taps read before either is used
// -- a tap the plan does not have reads tap i0 once more and is dropped.  The same product(s) and the same sum: the same bits
template <typename F>
__device__ __forceinline__ float fg_scale_eval_up(const ScaleTerm& t, F fetch) {
#pragma clang fp contract(off)
    const float a = fetch(t.i0), b = fetch(t.has_last ? t.i1 : t.i0);
    const float acc = t.w0 * a, v = t.w1 * b;
    return t.has_last ? acc + v : acc;
}
__global__ __launch_bounds__(256) void scale_bilinear_kernel(const float* __restrict__ src, float* __restrict__ dst, long long total, int C, int Hs,
                                                             int Ws, int Hd, int Wd, int nchw, const float* __restrict__ sub_from,
                                                             float* __restrict__ diff) {
#pragma clang fp contract(off)
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        long long r = idx;
        int c, x, y;
        if (nchw) { x = (int)(r % Wd); r /= Wd; y = (int)(r % Hd); r /= Hd; c = (int)(r % C); r /= C; }
        else { c = (int)(r % C); r /= C; x = (int)(r % Wd); r /= Wd; y = (int)(r % Hd); r /= Hd; }
        const long long n = r;
        const long long sy = nchw ? Ws : (long long)Ws * C, sx = nchw ? 1 : C;
        const float* img = src + (nchw ? (n * C + c) * (long long)Hs * Ws : n * (long long)Hs * Ws * C + c);
        const ScaleTerm th = fg_scale_plan(Ws, Wd, x), tv = fg_scale_plan(Hs, Hd, y);
        const float v = fg_scale_eval(tv, [&](int j) {
            const float* row = img + j * sy;
            return fg_scale_eval(th, [&](int i) { return row[i * sx]; });
        });
        dst[idx] = v;
        if (diff) diff[idx] = sub_from[idx] - v;
    }
}
int fg_launch_scale_bilinear(fg_ctx* ctx, const float* src, float* dst, int N, int C, int Hs, int Ws, int Hd, int Wd, int nchw,
                             const float* sub_from, float* diff) {
    const long long total = (long long)N * C * Hd * Wd;
    if (total == 0) return FG_OK;
    hipLaunchKernelGGL(scale_bilinear_kernel, FG_GRID(total, 256), dim3(256), 0, ctx->stream, src, dst, total, C, Hs, Ws, Hd, Wd, nchw,
                       sub_from, diff);
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The warps: one block of 256 threads per output image, the exact count (no kernel walks a grid), an instance per pair of layouts
// (SET_NCHW: the set is channel-major, OUT_NCHW: the batch is).  What the three kernels share:
// ---------------------------------------------------------------------------------------------------------------------------------
// the pixels p = tid, tid + 256, .. < n of an image w wide: f(p, y, x) with p = y * w + x.  (y, x) advance by the quotient and
// remainder of 256 by w, taken once, with one carry: no division in the loop
template <typename F>
__device__ __forceinline__ void img_walk(int tid, int n, int w, F f) {
    int y = tid / w, x = tid - y * w;
    const int qy = 256 / w, rx = 256 - qy * w;
    for (int p = tid; p < n; p += 256) {
        f(p, y, x);
        x += rx; y += qy;
        if (x >= w) { x -= w; ++y; }
    }
}
// the instance of a pair of layouts: LAUNCH(SN, ON) with literal template arguments, which the launch log then shows
#define FG_BY_LAYOUT(set_nchw, out_nchw, LAUNCH)                                                                                \
    if (set_nchw) {                                                                                                             \
        if (out_nchw) { LAUNCH(true, true); } else { LAUNCH(true, false); }                                                     \
    } else {                                                                                                                    \
        if (out_nchw) { LAUNCH(false, true); } else { LAUNCH(false, false); }                                                   \
    }
// the copy of one source image of E floats into LDS, as it lies in the set (warp_images_kernel, warp_c2f_kernel)
__device__ __forceinline__ void wi_load(const float* __restrict__ s, float* __restrict__ img, int E, int vec, int tid) {
    if (vec) {                                                              // E % 4 == 0 and a 16-byte aligned set
        // four loads per lane issued before the first is used.  No branch: a slot past the end of the image (the last round
        // only) moves the lane's first slot once more, from the same source to the same place
        for (int e0 = tid * 4; e0 < E; e0 += 4096) {
            const int e1 = e0 + 1024 < E ? e0 + 1024 : e0, e2 = e0 + 2048 < E ? e0 + 2048 : e0, e3 = e0 + 3072 < E ? e0 + 3072 : e0;
            const float4 v0 = *reinterpret_cast<const float4*>(s + e0), v1 = *reinterpret_cast<const float4*>(s + e1);
            const float4 v2 = *reinterpret_cast<const float4*>(s + e2), v3 = *reinterpret_cast<const float4*>(s + e3);
            *reinterpret_cast<float4*>(img + e0) = v0;
            *reinterpret_cast<float4*>(img + e1) = v1;
            *reinterpret_cast<float4*>(img + e2) = v2;
            *reinterpret_cast<float4*>(img + e3) = v3;
        }
    } else {
        for (int e0 = tid; e0 < E; e0 += 1024) {
            const int e1 = e0 + 256 < E ? e0 + 256 : e0, e2 = e0 + 512 < E ? e0 + 512 : e0, e3 = e0 + 768 < E ? e0 + 768 : e0;
            const float v0 = s[e0], v1 = s[e1], v2 = s[e2], v3 = s[e3];
            img[e0] = v0;
            img[e1] = v1;
            img[e2] = v2;
            img[e3] = v3;
        }
    }
}
// A set held as 8-bit pixels (the _u8 entries, PIX = uint8_t): the value of a byte b is b / 255 by a true division, the correctly
// rounded fp32 quotient the host loaders produce (b * (1 / 255) gives another float for 126 of the 256 bytes).  A pixel is decoded
// where it leaves global memory and nowhere else, so everything behind the decode is the fp32 code on the same floats
__device__ __forceinline__ float wi_pix(float v) { return v; }
__device__ __forceinline__ float wi_pix(uint8_t b) { return (float)b / 255.0f; }
__device__ __forceinline__ float wi_pix(uint32_t b) { return (float)b / 255.0f; }       // a byte in a register of its own
// The four taps of a channel read straight from global memory (wi_warp<.., LDS_IMG = false>): wi_raw is a tap as it is read, a float
// or a byte widened to a word, and wi_taps_read stands between the four reads and their decode.  For bytes it pins the words in
// registers: without it the compiler moves each tap's conversion up under that tap's condition, next to its load, and waits there --
// four memory latencies per channel in turn where the fp32 instance has its four reads in flight together (measured: 131 us against
// 75 us for 64 faces of 84 -> 32, profiles/r18_u8_sets.md).  For floats it is nothing
__device__ __forceinline__ float wi_raw(float v) { return v; }
__device__ __forceinline__ uint32_t wi_raw(uint8_t b) { return b; }
__device__ __forceinline__ void wi_taps_read(float&, float&, float&, float&) {}
__device__ __forceinline__ void wi_taps_read(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }
// (a luma set: the twelve words of four taps from planes, or of the four slots of wi_load_luma, W = uint32_t or four words; the
// eight words of four taps from triples.  One statement each, over the words as they are loaded: nothing is taken out of a word,
// and so nothing waits for one, before all are read)
typedef uint32_t wi_u32x4 __attribute__((ext_vector_type(4)));
template <typename W>
__device__ __forceinline__ void wi_taps_read(W& a0, W& a1, W& a2, W& b0, W& b1, W& b2, W& c0, W& c1, W& c2, W& d0, W& d1, W& d2) {
    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(b0), "+v"(b1), "+v"(b2), "+v"(c0), "+v"(c1), "+v"(c2), "+v"(d0), "+v"(d1), "+v"(d2));
}
__device__ __forceinline__ void wi_taps_read(uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1, uint32_t& c0, uint32_t& c1, uint32_t& d0,
                                             uint32_t& d1) {
    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(b0), "+v"(b1), "+v"(c0), "+v"(c1), "+v"(d0), "+v"(d1));
}
// four pixels of a little-endian word, in address order
__device__ __forceinline__ float4 wi_pix4(uint32_t w) {
    return make_float4(wi_pix((uint8_t)(w & 255u)), wi_pix((uint8_t)((w >> 8) & 255u)), wi_pix((uint8_t)((w >> 16) & 255u)), wi_pix((uint8_t)(w >> 24)));
}
// the same copy of a source image of E bytes, decoded into E floats of LDS.  wide 16: a 16-byte aligned set of images of E % 16 == 0
// bytes, sixteen pixels per lane and load, stored as four 16-byte rows (the widest LDS store: a lane's pixels are 64 contiguous
// bytes of LDS whatever the store, and the wide one has the fewest lanes per pass on the same banks); wide 4: a 4-byte aligned set
// of images of E % 4 == 0 bytes, a word per lane and load, lanes side by side in LDS; otherwise bytes.  As above, four loads per
// lane are issued before the first is used, and a slot past the end of the image moves the lane's first slot once more.  No load
// reaches past byte E - 1 of the image
__device__ __forceinline__ void wi_load(const uint8_t* __restrict__ s, float* __restrict__ img, int E, int wide, int tid) {
    if (wide == 16) {
        for (int e0 = tid * 16; e0 < E; e0 += 16384) {
            const int e1 = e0 + 4096 < E ? e0 + 4096 : e0, e2 = e0 + 8192 < E ? e0 + 8192 : e0, e3 = e0 + 12288 < E ? e0 + 12288 : e0;
            const uint4 v0 = *reinterpret_cast<const uint4*>(s + e0), v1 = *reinterpret_cast<const uint4*>(s + e1);
            const uint4 v2 = *reinterpret_cast<const uint4*>(s + e2), v3 = *reinterpret_cast<const uint4*>(s + e3);
            auto put = [&](int e, const uint4& v) {
                float4* d = reinterpret_cast<float4*>(img + e);
                d[0] = wi_pix4(v.x); d[1] = wi_pix4(v.y); d[2] = wi_pix4(v.z); d[3] = wi_pix4(v.w);
            };
            put(e0, v0);
            put(e1, v1);
            put(e2, v2);
            put(e3, v3);
        }
    } else if (wide == 4) {
        for (int e0 = tid * 4; e0 < E; e0 += 4096) {
            const int e1 = e0 + 1024 < E ? e0 + 1024 : e0, e2 = e0 + 2048 < E ? e0 + 2048 : e0, e3 = e0 + 3072 < E ? e0 + 3072 : e0;
            const uint32_t v0 = *reinterpret_cast<const uint32_t*>(s + e0), v1 = *reinterpret_cast<const uint32_t*>(s + e1);
            const uint32_t v2 = *reinterpret_cast<const uint32_t*>(s + e2), v3 = *reinterpret_cast<const uint32_t*>(s + e3);
            *reinterpret_cast<float4*>(img + e0) = wi_pix4(v0);
            *reinterpret_cast<float4*>(img + e1) = wi_pix4(v1);
            *reinterpret_cast<float4*>(img + e2) = wi_pix4(v2);
            *reinterpret_cast<float4*>(img + e3) = wi_pix4(v3);
        }
    } else {
        for (int e0 = tid; e0 < E; e0 += 1024) {
            const int e1 = e0 + 256 < E ? e0 + 256 : e0, e2 = e0 + 512 < E ? e0 + 512 : e0, e3 = e0 + 768 < E ? e0 + 768 : e0;
            const uint8_t v0 = s[e0], v1 = s[e1], v2 = s[e2], v3 = s[e3];
            img[e0] = wi_pix(v0);
            img[e1] = wi_pix(v1);
            img[e2] = wi_pix(v2);
            img[e3] = wi_pix(v3);
        }
    }
}
// the widest load wi_load may use on a byte set: every image base is then aligned to it and no load crosses the end of an image
static int wi_wide_u8(const uint8_t* set, int E) {
    return ((size_t)set & 15) == 0 && E % 16 == 0 ? 16 : ((size_t)set & 3) == 0 && E % 4 == 0 ? 4 : 1;
}
// A set of R, G, B bytes read as luma (the _u8_y entries, PIX = wi_y8, a tag: a set of wi_y8 is three bytes per pixel and the kernels
// run at c == 1).  The value of a pixel is Torch7's image.rgb2y on the floats p(b) = b / 255,
//     Y = ((0.299f * p(r)) + (0.587f * p(g))) + (0.114f * p(b)),
// every product and sum rounded on its own in this order (no FMA contraction; the constants are the floats nearest to the decimals).
// As with the bytes it is formed where the pixel leaves global memory, so everything behind it is the fp32 code at c == 1
struct wi_y8 { uint8_t b; };
template <typename PIX> struct wi_is_luma { static constexpr bool value = false; };
template <> struct wi_is_luma<wi_y8> { static constexpr bool value = true; };
__device__ __forceinline__ float wi_luma(uint32_t r, uint32_t g, uint32_t b) {
#pragma clang fp contract(off)
    const float yr = 0x1.322d0ep-2f * wi_pix(r), yg = 0x1.2c8b44p-1f * wi_pix(g), yb = 0x1.d2f1aap-4f * wi_pix(b);
    return (yr + yg) + yb;
}
// byte k (address order) of the little-endian words w[]
__device__ __forceinline__ uint32_t wi_byte(const uint32_t* w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }
// the words of a load as it sits in registers, R = wi_u32x4 (16 bytes in address order) / uint32_t (a word, or a byte widened)
__device__ __forceinline__ void wi_words(const wi_u32x4& v, uint32_t* w) { w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
__device__ __forceinline__ void wi_words(const uint32_t& v, uint32_t* w) { w[0] = v; }
// wi_load for a luma set: the image at `s` is 3 P bytes (PLANES: the planes R, G, B of P bytes each; otherwise P triples R, G, B),
// LDS takes its P luma floats.  A slot is W = sizeof(V) pixels of a lane: three loads of W bytes, one from each plane at the same
// offset, or the 3 W contiguous bytes of the W triples.  wide 16 / 4 (V = wi_u32x4 / uint32_t): `set` is aligned to W and
// P % W == 0, so the image's base 3 P i, the plane offsets P and 2 P and the slots 3 W k are aligned to W and no slot straddles the
// end of a plane or of the image; otherwise single bytes.  wi_load's shape: the loads of four slots per lane (twelve) are issued
// before the first is used, and a slot past the end moves the lane's first slot once more.  The twelve loaded registers (48 words
// at the 16-byte width) are pinned between the loads and the decode (wi_taps_read): left alone, the compiler decodes the 16-byte
// slots one at a time, each behind a wait of its own.  No load reaches past byte 3 P - 1 of the image
template <bool PLANES, typename V>
__device__ __forceinline__ void wi_load_luma_as(const uint8_t* __restrict__ s, float* __restrict__ img, int P, int tid) {
    constexpr int W = (int)sizeof(V), NW = W < 4 ? 1 : W / 4;
    using R = decltype(V() + 0u);                                           // uint8_t widens to a word
    struct Slot { R a, b, c; };
    auto get = [&](int e) {
        const uint8_t* q = PLANES ? s + e : s + 3 * e;
        const int step = PLANES ? P : W;
        Slot t;
        t.a = *reinterpret_cast<const V*>(q); t.b = *reinterpret_cast<const V*>(q + step); t.c = *reinterpret_cast<const V*>(q + 2 * step);
        return t;
    };
    auto put = [&](int e, const Slot& t) {
        uint32_t w[3 * NW];
        wi_words(t.a, w); wi_words(t.b, w + NW); wi_words(t.c, w + 2 * NW);
        float y[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            if (W == 1) y[k] = wi_luma(w[0], w[1], w[2]);
            else if (PLANES) y[k] = wi_luma(wi_byte(w, k), wi_byte(w + NW, k), wi_byte(w + 2 * NW, k));
            else y[k] = wi_luma(wi_byte(w, 3 * k), wi_byte(w, 3 * k + 1), wi_byte(w, 3 * k + 2));
        }
        if (W == 1) img[e] = y[0];
        else {
#pragma unroll
            for (int k = 0; k < W; k += 4) *reinterpret_cast<float4*>(img + e + k) = make_float4(y[k], y[k + 1], y[k + 2], y[k + 3]);
        }
    };
    for (int e0 = tid * W; e0 < P; e0 += 1024 * W) {
        const int e1 = e0 + 256 * W < P ? e0 + 256 * W : e0, e2 = e0 + 512 * W < P ? e0 + 512 * W : e0, e3 = e0 + 768 * W < P ? e0 + 768 * W : e0;
        Slot t0 = get(e0), t1 = get(e1), t2 = get(e2), t3 = get(e3);
        wi_taps_read(t0.a, t0.b, t0.c, t1.a, t1.b, t1.c, t2.a, t2.b, t2.c, t3.a, t3.b, t3.c);
        put(e0, t0);
        put(e1, t1);
        put(e2, t2);
        put(e3, t3);
    }
}
template <bool PLANES>
__device__ __forceinline__ void wi_load_luma(const uint8_t* __restrict__ s, float* __restrict__ img, int P, int wide, int tid) {
    if (wide == 16) wi_load_luma_as<PLANES, wi_u32x4>(s, img, P, tid);
    else if (wide == 4) wi_load_luma_as<PLANES, uint32_t>(s, img, P, tid);
    else wi_load_luma_as<PLANES, uint8_t>(s, img, P, tid);
}
// the widest load wi_load_luma may use, in either layout: with `set` aligned to it and P % width == 0 every image base, plane and
// slot is aligned to it and no load crosses the end of a plane or of an image (3 P % 16 == 0 is P % 16 == 0)
static int wi_wide_u8_y(const uint8_t* set, int P) {
    return ((size_t)set & 15) == 0 && P % 16 == 0 ? 16 : ((size_t)set & 3) == 0 && P % 4 == 0 ? 4 : 1;
}
// fg_warp_images (include/facegen_hip.h): out[j] = clamp01(gains[j] * bilinear(set[idx[j]], affine map mats[j])).
//   - the source image (c * hs * ws <= 16384 floats) goes to LDS as it lies in the set, 16 bytes per lane where `vec` allows;
//   - a thread owns output pixels p = tid, tid + 256, ..: the source coordinates, the range test and the four tap offsets are
//     taken once per pixel, then every channel reads its four taps from LDS (lanes on neighbouring pixels: stride 1 in a
//     channel-major image, stride c in a pixel-major one -- c = 3 keeps a 32-lane group on 32 banks) and writes one float:
//     an NCHW batch gets 256 contiguous bytes per wave and channel, an NHWC one the c floats of each pixel, the wave's
//     pixels side by side;
//   - indices are 32-bit inside an image, the image's base 64-bit.
// Every product, sum and difference is rounded on its own, in the order the header states (no FMA contraction): a numpy fp32
// restatement matches bit for bit.  Out of the image: a tap is 0 (fill 0: the lane reads the LDS copy of pixel 0 instead and
// drops it, so that the four reads of a channel are in flight together); coordinates are clamped in float before the floor
// (fill 1); the range test comes before any float-to-int conversion, so NaN, inf and huge coordinates address nothing.  Global
// memory is read only by the copy of the image into LDS.
//
// wi_warp, the warp of the image `img` under mats[j] / gains[j]: store(p, ch, v) takes channel ch of output pixel p = y * wo + x.
// HOLDS A BARRIER: one __syncthreads() in front of the first tap, which every thread of the block reaches -- what the block wrote
// to LDS before the call (wi_load's copy of the image, the scale plans) is visible to the taps and to everything behind the call.
// LDS_IMG: `img` is the block's LDS copy, and a tap outside the image reads pixel 0 and drops it; otherwise `img` is the image
// where it lies in the set (warp_faces_kernel: a photo of any size, taps straight from global memory) and such a tap addresses
// nothing.  PIX: what `img` holds, floats or, where it is a photo of a byte set, bytes that the tap read decodes (wi_pix).  The
// arithmetic is one
template <bool SET_NCHW, bool LDS_IMG = true, typename PIX, typename Store>
__device__ __forceinline__ void wi_warp(const PIX* __restrict__ img, const float* __restrict__ mats, const float* __restrict__ gains, int j,
                                        int c, int hs, int ws, int ho, int wo, int edge, int tid, Store store) {
#pragma clang fp contract(off)
    const int Ps = hs * ws;
    float m0 = 1.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 1.f, m5 = 0.f;
    if (mats) { const float* m = mats + 6 * (long long)j; m0 = m[0]; m1 = m[1]; m2 = m[2]; m3 = m[3]; m4 = m[4]; m5 = m[5]; }
    const float g = gains ? gains[j] : 1.f;
    const float wsf = (float)ws, hsf = (float)hs, xmax = (float)(ws - 1), ymax = (float)(hs - 1);
    // img_walk, written out: handed to img_walk as a functor this loop compiles to other control flow around the range test and
    // to another order of the LDS reads, and the warps measured 1 to 3 % slower at 64 x 64 (profiles/r17_image_split.md)
    const int Po = ho * wo;
    int y = tid / wo, x = tid - y * wo;
    const int qy = 256 / wo, rx = 256 - qy * wo;
    __syncthreads();
    for (int p = tid; p < Po; p += 256) {
        const float xf = (float)x, yf = (float)y;
        float sx = (m0 * xf + m1 * yf) + m2;
        float sy = (m3 * xf + m4 * yf) + m5;
        bool inside = true;
        if (edge) {
            sx = fminf(fmaxf(sx, 0.f), xmax);
            sy = fminf(fmaxf(sy, 0.f), ymax);
        } else
            inside = sx > -1.f && sx < wsf && sy > -1.f && sy < hsf;
        int oa = -1, ob = -1, oc = -1, od = -1;                             // pixel offsets of the four taps, -1: outside
        float fx = 0.f, fy = 0.f;
        if (inside) {
            const float x0f = floorf(sx), y0f = floorf(sy);
            fx = sx - x0f; fy = sy - y0f;
            const int x0 = (int)x0f, y0 = (int)y0f;                         // -1 .. ws - 1, -1 .. hs - 1
            const bool xl = x0 >= 0, xr = x0 + 1 < ws, yt = y0 >= 0, yb = y0 + 1 < hs;
            const int at = y0 * ws + x0;
            if (yt && xl) oa = at;
            if (yt && xr) ob = at + 1;
            if (yb && xl) oc = at + ws;
            if (yb && xr) od = at + ws + 1;
        }
        const int ts = SET_NCHW ? 1 : c, cs = SET_NCHW ? Ps : 1;            // strides of a pixel and of a channel in the LDS image
        // (a tap outside an LDS image reads the copy of pixel 0 and drops it: four reads in flight per channel, no branch)
        const int ia = (oa < 0 ? 0 : oa) * ts, ib = (ob < 0 ? 0 : ob) * ts, ic = (oc < 0 ? 0 : oc) * ts, id = (od < 0 ? 0 : od) * ts;
        for (int ch = 0; ch < c; ++ch) {
            float ra, rb, rc, rd;
            if constexpr (wi_is_luma<PIX>::value) {
                // a photo of a luma set (c == 1, never an LDS image): the R, G, B bytes of the four taps, all read in front of the
                // first decode (wi_taps_read).  Planes: byte o of each plane, twelve reads.  Triples: the triple at 3 o as its
                // first two bytes in one 2-byte read (at any address) and its third, eight reads -- what the compiler makes of
                // three byte reads too, but then it takes R and G apart next to their read and waits there, tap after tap
                const uint8_t* ph = &img->b;
                if constexpr (SET_NCHW) {
                    uint32_t a0 = oa >= 0 ? ph[oa] : 0u, a1 = oa >= 0 ? ph[oa + Ps] : 0u, a2 = oa >= 0 ? ph[oa + 2 * Ps] : 0u;
                    uint32_t b0 = ob >= 0 ? ph[ob] : 0u, b1 = ob >= 0 ? ph[ob + Ps] : 0u, b2 = ob >= 0 ? ph[ob + 2 * Ps] : 0u;
                    uint32_t c0 = oc >= 0 ? ph[oc] : 0u, c1 = oc >= 0 ? ph[oc + Ps] : 0u, c2 = oc >= 0 ? ph[oc + 2 * Ps] : 0u;
                    uint32_t d0 = od >= 0 ? ph[od] : 0u, d1 = od >= 0 ? ph[od + Ps] : 0u, d2 = od >= 0 ? ph[od + 2 * Ps] : 0u;
                    wi_taps_read(a0, a1, a2, b0, b1, b2, c0, c1, c2, d0, d1, d2);
                    ra = wi_luma(a0, a1, a2); rb = wi_luma(b0, b1, b2); rc = wi_luma(c0, c1, c2); rd = wi_luma(d0, d1, d2);
                } else {
                    typedef uint16_t __attribute__((aligned(1))) rg_t;          // R, G of a triple, little-endian: G in the high byte
                    auto rg = [&](int o) -> uint32_t { return *reinterpret_cast<const rg_t*>(ph + 3 * o); };
                    uint32_t a0 = oa >= 0 ? rg(oa) : 0u, a2 = oa >= 0 ? ph[3 * oa + 2] : 0u;
                    uint32_t b0 = ob >= 0 ? rg(ob) : 0u, b2 = ob >= 0 ? ph[3 * ob + 2] : 0u;
                    uint32_t c0 = oc >= 0 ? rg(oc) : 0u, c2 = oc >= 0 ? ph[3 * oc + 2] : 0u;
                    uint32_t d0 = od >= 0 ? rg(od) : 0u, d2 = od >= 0 ? ph[3 * od + 2] : 0u;
                    wi_taps_read(a0, a2, b0, b2, c0, c2, d0, d2);
                    ra = wi_luma(a0 & 255u, a0 >> 8, a2); rb = wi_luma(b0 & 255u, b0 >> 8, b2);
                    rc = wi_luma(c0 & 255u, c0 >> 8, c2); rd = wi_luma(d0 & 255u, d0 >> 8, d2);
                }
            } else {
                const PIX* pl = img + ch * cs;
                // (the four reads, then the decode of a byte set's taps: wi_taps_read)
                using RAW = decltype(wi_raw(pl[0]));
                RAW qa = LDS_IMG || oa >= 0 ? wi_raw(pl[ia]) : RAW(0), qb = LDS_IMG || ob >= 0 ? wi_raw(pl[ib]) : RAW(0);
                RAW qc = LDS_IMG || oc >= 0 ? wi_raw(pl[ic]) : RAW(0), qd = LDS_IMG || od >= 0 ? wi_raw(pl[id]) : RAW(0);
                wi_taps_read(qa, qb, qc, qd);
                ra = wi_pix(qa); rb = wi_pix(qb); rc = wi_pix(qc); rd = wi_pix(qd);
            }
            const float a = oa >= 0 ? ra : 0.f, b = ob >= 0 ? rb : 0.f, cc = oc >= 0 ? rc : 0.f, d = od >= 0 ? rd : 0.f;
            const float top = a + (b - a) * fx, bot = cc + (d - cc) * fx;
            float v = top + (bot - top) * fy;
            if (gains) v = fminf(fmaxf(v * g, 0.f), 1.f);
            store(p, ch, v);
        }
        x += rx; y += qy;
        if (x >= wo) { x -= wo; ++y; }
    }
}
template <bool SET_NCHW, bool OUT_NCHW, typename PIX = float>
__global__ __launch_bounds__(256) void warp_images_kernel(const PIX* __restrict__ set, long long n_set, const int* __restrict__ idx,
                                                          const float* __restrict__ mats, const float* __restrict__ gains, int c, int hs,
                                                          int ws, int ho, int wo, float* __restrict__ out, int edge, int vec) {
    extern __shared__ float4 wi_lds[];                                      // c * hs * ws floats
    float* img = reinterpret_cast<float*>(wi_lds);
    const int tid = (int)threadIdx.x, j = (int)blockIdx.x;
    const int Po = ho * wo, E = c * hs * ws, Eo = c * Po;
    float* __restrict__ o = out + (long long)j * Eo;
    const int i = idx[j];
    if (i < 0 || (long long)i >= n_set) {                                   // outside the set: nothing is read, the image is NaN
        for (int e = tid; e < Eo; e += 256) o[e] = gi_nan();
        return;
    }
    if constexpr (wi_is_luma<PIX>::value) wi_load_luma<SET_NCHW>(&set->b + 3 * ((long long)i * E), img, E, vec, tid);     // (c == 1: E pixels)
    else wi_load(set + (long long)i * E, img, E, vec, tid);
    // (the barrier inside wi_warp: the image is complete before the first tap)
    wi_warp<SET_NCHW>(img, mats, gains, j, c, hs, ws, ho, wo, edge, tid,
                      [&](int p, int ch, float v) { o[OUT_NCHW ? ch * Po + p : p * c + ch] = v; });
}
// fg_warp_images: c * hs * ws <= FG_WARP_MAX_FLOATS, checked by the entry.  One channel: the two layouts are one order, and the
// NCHW instance serves all four pairs
int fg_launch_warp_images(fg_ctx* ctx, const float* set, long long n_set, int c, int hs, int ws, int set_nchw, const int* idx,
                          const float* mats, const float* gains, int n, float* out, int ho, int wo, int out_nchw, int edge) {
    const int E = c * hs * ws;
    const size_t lds = ((size_t)E * sizeof(float) + 15) & ~(size_t)15;
    const int vec = ((size_t)set & 15) == 0 && E % 4 == 0;
    const dim3 images((unsigned)n);
    if (c == 1) set_nchw = out_nchw = 1;
#define IMAGES(SN, ON)                                                                                                           \
    hipLaunchKernelGGL((warp_images_kernel<SN, ON>), images, dim3(256), lds, ctx->stream, set, n_set, idx, mats, gains, c, hs, ws, ho, wo, \
                       out, edge, vec)
    FG_BY_LAYOUT(set_nchw, out_nchw, IMAGES)
#undef IMAGES
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}
// fg_warp_images_u8: the same grid, block and LDS (the block's copy holds decoded floats); `vec` carries wi_wide_u8
int fg_launch_warp_images_u8(fg_ctx* ctx, const uint8_t* set, long long n_set, int c, int hs, int ws, int set_nchw, const int* idx,
                             const float* mats, const float* gains, int n, float* out, int ho, int wo, int out_nchw, int edge) {
    const int E = c * hs * ws;
    const size_t lds = ((size_t)E * sizeof(float) + 15) & ~(size_t)15;
    const int vec = wi_wide_u8(set, E);
    const dim3 images((unsigned)n);
    if (c == 1) set_nchw = out_nchw = 1;
#define IMAGES_U8(SN, ON)                                                                                                        \
    hipLaunchKernelGGL((warp_images_kernel<SN, ON, uint8_t>), images, dim3(256), lds, ctx->stream, set, n_set, idx, mats, gains, c, hs, ws, \
                       ho, wo, out, edge, vec)
    FG_BY_LAYOUT(set_nchw, out_nchw, IMAGES_U8)
#undef IMAGES_U8
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}
// fg_warp_images_u8_y: a set of R, G, B bytes read as luma, one channel out: fg_launch_warp_images' grid, block and LDS at c == 1
// (the block's copy holds the hs * ws luma floats).  An instance per set layout (the batch's two layouts are one order); `vec`
// carries wi_wide_u8_y
int fg_launch_warp_images_u8_y(fg_ctx* ctx, const uint8_t* set, long long n_set, int hs, int ws, int set_nchw, const int* idx, const float* mats,
                               const float* gains, int n, float* out, int ho, int wo, int edge) {
    const int P = hs * ws;
    const size_t lds = ((size_t)P * sizeof(float) + 15) & ~(size_t)15;
    const int vec = wi_wide_u8_y(set, P);
    const dim3 images((unsigned)n);
    const wi_y8* luma = reinterpret_cast<const wi_y8*>(set);
#define IMAGES_Y(SN, ON)                                                                                                         \
    hipLaunchKernelGGL((warp_images_kernel<SN, ON, wi_y8>), images, dim3(256), lds, ctx->stream, luma, n_set, idx, mats, gains, 1, hs, ws, \
                       ho, wo, out, edge, vec)
    if (set_nchw) { IMAGES_Y(true, true); } else { IMAGES_Y(false, true); }
#undef IMAGES_Y
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The coarse-to-fine fields of one image inside its block, shared by warp_c2f_kernel and warp_faces_kernel.  LDS holds B, the fine
// image at s x s (channel-major), a region A that is free once B is complete, and the scale plans T, one per coordinate and
// direction (the images are square), taken once per block: T[0 .. s): cs -> s, T[s .. s + cs): s -> cs.  Both scale passes are the
// nested width-then-height evaluation of scale_bilinear_kernel (fg_scale_plan / fg_scale_eval per output element), so every float
// is the one fg_scale_bilinear and fg_c2f_coarse_diff give through HBM.  A block is alone on its CU with one wave per SIMD, so
// nothing hides an LDS round trip: the last pass, the longest, reads its four taps together (fg_scale_eval_up).  Lanes walk
// neighbouring pixels of one channel plane: stride 1 in the last pass, stride s / cs (2 at 64 -> 32: two lanes per bank) in the
// down pass.
// ---------------------------------------------------------------------------------------------------------------------------------
// an index outside the set: nothing is read, every requested image (Eo floats) is NaN
__device__ __forceinline__ void c2f_fill_nan(float* __restrict__ fine, float* __restrict__ coarse, float* __restrict__ diff, int Eo, int tid) {
    for (int e = tid; e < Eo; e += 256) {
        if (fine) fine[e] = gi_nan();
        if (coarse) coarse[e] = gi_nan();
        if (diff) diff[e] = gi_nan();
    }
}
// A = scale(B, cs, cs), through T[s .. s + cs)
__device__ __forceinline__ void c2f_down(const float* B, float* A, const ScaleTerm* T, int c, int s, int cs, int tid) {
#pragma clang fp contract(off)
    const int Po = s * s, Pc = cs * cs;
    img_walk(tid, Pc, cs, [&](int p, int y, int x) {
        const ScaleTerm th = T[s + x], tv = T[s + y];
        for (int ch = 0; ch < c; ++ch) {
            const float* plane = B + ch * Po;
            A[ch * Pc + p] = fg_scale_eval(tv, [&](int r) {
                const float* row = plane + r * s;
                return fg_scale_eval(th, [&](int q) { return row[q]; });
            });
        }
    });
}
// coarse = scale(A, s, s) through T[0 .. s), diff = B - coarse, fine = B: each requested field to its place in the batch
template <bool OUT_NCHW>
__device__ __forceinline__ void c2f_up_write(const float* A, const float* B, const ScaleTerm* T, int c, int s, int cs, float* __restrict__ fine,
                                             float* __restrict__ coarse, float* __restrict__ diff, int tid) {
#pragma clang fp contract(off)
    const int Po = s * s, Pc = cs * cs;
    img_walk(tid, Po, s, [&](int p, int y, int x) {
        const ScaleTerm th = T[x], tv = T[y];
        for (int ch = 0; ch < c; ++ch) {
            const float* plane = A + ch * Pc;
            const float v = fg_scale_eval_up(tv, [&](int r) {
                const float* row = plane + r * cs;
                return fg_scale_eval_up(th, [&](int q) { return row[q]; });
            });
            const float f = B[ch * Po + p];
            const int o = OUT_NCHW ? ch * Po + p : p * c + ch;
            if (coarse) coarse[o] = v;
            if (diff) diff[o] = f - v;
            if (fine) fine[o] = f;
        }
    });
}
// fg_warp_c2f (include/facegen_hip.h): fg_warp_images at s x s followed by fg_c2f_coarse_diff, nothing but the requested outputs
// leaves the block.  A is the source image (wi_load), B takes the warp's stores (stride 1 per channel plane).  The source is dead
// after the warp: A then takes the cs x cs image.  Up to 135 KB of LDS.
template <bool SET_NCHW, bool OUT_NCHW, typename PIX = float>
__global__ __launch_bounds__(256) void warp_c2f_kernel(const PIX* __restrict__ set, long long n_set, const int* __restrict__ idx,
                                                       const float* __restrict__ mats, const float* __restrict__ gains, int c, int hs, int ws,
                                                       int s, int cs, float* __restrict__ fine, float* __restrict__ coarse,
                                                       float* __restrict__ diff, int edge, int vec) {
#pragma clang fp contract(off)
    extern __shared__ float4 wi_lds[];                                      // A: max(c * hs * ws, c * cs * cs) floats, B: c * s * s, T
    const int tid = (int)threadIdx.x, j = (int)blockIdx.x;
    const int Po = s * s, E = c * hs * ws, Eo = c * Po, Ec = c * cs * cs;
    float* A = reinterpret_cast<float*>(wi_lds);
    float* B = A + (((E > Ec ? E : Ec) + 3) & ~3);
    ScaleTerm* T = reinterpret_cast<ScaleTerm*>(B + Eo);                    // s plans of cs -> s, then cs plans of s -> cs
    const long long base = (long long)j * Eo;
    if (fine) fine += base;
    if (coarse) coarse += base;
    if (diff) diff += base;
    const int i = idx[j];
    if (i < 0 || (long long)i >= n_set) { c2f_fill_nan(fine, coarse, diff, Eo, tid); return; }
    if constexpr (wi_is_luma<PIX>::value) wi_load_luma<SET_NCHW>(&set->b + 3 * ((long long)i * E), A, E, vec, tid);       // (c == 1: E pixels)
    else wi_load(set + (long long)i * E, A, E, vec, tid);
    for (int k = tid; k < s + cs; k += 256) T[k] = k < s ? fg_scale_plan(cs, s, k) : fg_scale_plan(s, cs, k - s);
    // (the barrier inside wi_warp: the image is complete before the first tap, and the plans before the passes below)
    wi_warp<SET_NCHW>(A, mats, gains, j, c, hs, ws, s, s, edge, tid, [&](int p, int ch, float v) { B[ch * Po + p] = v; });
    __syncthreads();                                                        // B is complete, A is free
    c2f_down(B, A, T, c, s, cs, tid);
    __syncthreads();
    c2f_up_write<OUT_NCHW>(A, B, T, c, s, cs, fine, coarse, diff, tid);
}
// fg_warp_c2f: LDS: the source image (or the cs x cs one where that is larger), the fine image and the s + cs scale plans: up to
// 2 * FG_WARP_MAX_FLOATS floats and 2 * 128 plans (c * s * s <= 16384: s <= 128) = 135 KB of the CU's 160 KB: the limit of each
// instance is raised once per context
int fg_launch_warp_c2f(fg_ctx* ctx, const float* set, long long n_set, int c, int hs, int ws, int set_nchw, const int* idx, const float* mats,
                       const float* gains, int n, int s, int cs, float* fine, float* coarse, float* diff, int out_nchw, int edge) {
    const int E = c * hs * ws, Ec = c * cs * cs;
    const size_t lds = (((size_t)(((E > Ec ? E : Ec) + 3) & ~3) + (size_t)c * s * s) * sizeof(float) + (size_t)(s + cs) * sizeof(ScaleTerm) + 15) & ~(size_t)15;
    const int vec = ((size_t)set & 15) == 0 && E % 4 == 0;
    const dim3 images((unsigned)n);
    if (c == 1) set_nchw = out_nchw = 1;
#define C2F(SN, ON)                                                                                                              \
    static char attr_key;                                                                                                        \
    if (fg_attr_first(ctx, &attr_key))                                                                                           \
        FG_HIP(ctx, hipFuncSetAttribute((const void*)warp_c2f_kernel<SN, ON>, hipFuncAttributeMaxDynamicSharedMemorySize,        \
                                        (int)(2 * FG_WARP_MAX_FLOATS * sizeof(float) + 2 * 128 * sizeof(ScaleTerm))));           \
    hipLaunchKernelGGL((warp_c2f_kernel<SN, ON>), images, dim3(256), lds, ctx->stream, set, n_set, idx, mats, gains, c, hs, ws, s, cs, \
                       fine, coarse, diff, edge, vec)
    FG_BY_LAYOUT(set_nchw, out_nchw, C2F)
#undef C2F
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}
// fg_warp_c2f_u8: the same grid, block and LDS.  The byte instances are functions of their own: each has its limit raised behind
// its own key
int fg_launch_warp_c2f_u8(fg_ctx* ctx, const uint8_t* set, long long n_set, int c, int hs, int ws, int set_nchw, const int* idx,
                          const float* mats, const float* gains, int n, int s, int cs, float* fine, float* coarse, float* diff, int out_nchw,
                          int edge) {
    const int E = c * hs * ws, Ec = c * cs * cs;
    const size_t lds = (((size_t)(((E > Ec ? E : Ec) + 3) & ~3) + (size_t)c * s * s) * sizeof(float) + (size_t)(s + cs) * sizeof(ScaleTerm) + 15) & ~(size_t)15;
    const int vec = wi_wide_u8(set, E);
    const dim3 images((unsigned)n);
    if (c == 1) set_nchw = out_nchw = 1;
#define C2F_U8(SN, ON)                                                                                                           \
    static char attr_key;                                                                                                        \
    if (fg_attr_first(ctx, &attr_key))                                                                                           \
        FG_HIP(ctx, hipFuncSetAttribute((const void*)warp_c2f_kernel<SN, ON, uint8_t>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                        (int)(2 * FG_WARP_MAX_FLOATS * sizeof(float) + 2 * 128 * sizeof(ScaleTerm))));           \
    hipLaunchKernelGGL((warp_c2f_kernel<SN, ON, uint8_t>), images, dim3(256), lds, ctx->stream, set, n_set, idx, mats, gains, c, hs, ws, s, \
                       cs, fine, coarse, diff, edge, vec)
    FG_BY_LAYOUT(set_nchw, out_nchw, C2F_U8)
#undef C2F_U8
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}
// fg_warp_c2f_u8_y: fg_launch_warp_c2f's grid, block and LDS at c == 1; the two luma instances have their limit raised behind
// their own keys
int fg_launch_warp_c2f_u8_y(fg_ctx* ctx, const uint8_t* set, long long n_set, int hs, int ws, int set_nchw, const int* idx, const float* mats,
                            const float* gains, int n, int s, int cs, float* fine, float* coarse, float* diff, int edge) {
    const int P = hs * ws, Pc = cs * cs;
    const size_t lds = (((size_t)(((P > Pc ? P : Pc) + 3) & ~3) + (size_t)s * s) * sizeof(float) + (size_t)(s + cs) * sizeof(ScaleTerm) + 15) & ~(size_t)15;
    const int vec = wi_wide_u8_y(set, P);
    const dim3 images((unsigned)n);
    const wi_y8* luma = reinterpret_cast<const wi_y8*>(set);
#define C2F_Y(SN, ON)                                                                                                            \
    static char attr_key;                                                                                                        \
    if (fg_attr_first(ctx, &attr_key))                                                                                           \
        FG_HIP(ctx, hipFuncSetAttribute((const void*)warp_c2f_kernel<SN, ON, wi_y8>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                        (int)(2 * FG_WARP_MAX_FLOATS * sizeof(float) + 2 * 128 * sizeof(ScaleTerm))));           \
    hipLaunchKernelGGL((warp_c2f_kernel<SN, ON, wi_y8>), images, dim3(256), lds, ctx->stream, luma, n_set, idx, mats, gains, 1, hs, ws, s, \
                       cs, fine, coarse, diff, edge, vec)
    if (set_nchw) { C2F_Y(true, true); } else { C2F_Y(false, true); }
#undef C2F_Y
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}
// fg_warp_faces (include/facegen_hip.h): the reference's pipeline on a photo of any size.  The photo stays in global memory: wi_warp
// takes the four taps of every channel of a window pixel straight from it (lanes on neighbouring window pixels read neighbouring
// addresses of a channel-major photo; a pixel's c floats are adjacent in a pixel-major one) and stores the hw x ww window into A,
// channel-major.  Stage 2 scales the window to the s x s face in B: scale_bilinear_kernel's body per face element (width pass
// nested in height pass), through two more runs of plans, T[s + cs .. 2s + cs): ww -> s (columns), T[2s + cs .. 3s + cs): hw -> s
// (rows); with hw == ww == s the warp writes the face itself.  With cs == 0 the face goes straight to `fine` and nothing follows.
template <bool SET_NCHW, bool OUT_NCHW, typename PIX = float>
__global__ __launch_bounds__(256) void warp_faces_kernel(const PIX* __restrict__ set, long long n_set, const int* __restrict__ idx,
                                                         const float* __restrict__ mats, const float* __restrict__ gains, int c, int hs,
                                                         int ws, int hw, int ww, int s, int cs, float* __restrict__ fine,
                                                         float* __restrict__ coarse, float* __restrict__ diff, int edge) {
#pragma clang fp contract(off)
    extern __shared__ float4 wi_lds[];
    const int tid = (int)threadIdx.x, j = (int)blockIdx.x;
    const int Pw = hw * ww, Po = s * s, Ew = c * Pw, Eo = c * Po, Ec = c * cs * cs;
    float* A = reinterpret_cast<float*>(wi_lds);
    float* B = A + (((Ew > Ec ? Ew : Ec) + 3) & ~3);
    ScaleTerm* T = reinterpret_cast<ScaleTerm*>(B + Eo);
    const long long base = (long long)j * Eo;
    if (fine) fine += base;
    if (coarse) coarse += base;
    if (diff) diff += base;
    const int i = idx[j];
    if (i < 0 || (long long)i >= n_set) { c2f_fill_nan(fine, coarse, diff, Eo, tid); return; }
    const PIX* photo = set + (long long)i * ((long long)(wi_is_luma<PIX>::value ? 3 : c) * hs * ws);       // (a luma set: c == 1 of 3 bytes)
    for (int k = tid; k < 3 * s + cs; k += 256)
        T[k] = k < s ? fg_scale_plan(cs, s, k) : k < s + cs ? fg_scale_plan(s, cs, k - s)
             : k < 2 * s + cs ? fg_scale_plan(ww, s, k - s - cs) : fg_scale_plan(hw, s, k - 2 * s - cs);
    // an element of the face: into B, or, without the coarse-to-fine fields, to its place in `fine`
    auto face = [&](int p, int ch, float v) {
        if (cs) B[ch * Po + p] = v;
        else fine[OUT_NCHW ? ch * Po + p : p * c + ch] = v;
    };
    // (the barrier inside wi_warp: the plans are complete before the passes below)
    if (hw == s && ww == s) wi_warp<SET_NCHW, false>(photo, mats, gains, j, c, hs, ws, s, s, edge, tid, face);
    else {
        wi_warp<SET_NCHW, false>(photo, mats, gains, j, c, hs, ws, hw, ww, edge, tid, [&](int p, int ch, float v) { A[ch * Pw + p] = v; });
        __syncthreads();                                                    // the window is complete
        img_walk(tid, Po, s, [&](int p, int y, int x) {
            const ScaleTerm th = T[s + cs + x], tv = T[2 * s + cs + y];
            for (int ch = 0; ch < c; ++ch) {
                const float* plane = A + ch * Pw;
                face(p, ch, fg_scale_eval(tv, [&](int r) {
                    const float* row = plane + r * ww;
                    return fg_scale_eval(th, [&](int q) { return row[q]; });
                }));
            }
        });
    }
    if (!cs) return;
    __syncthreads();                                                        // B is complete, A is free
    c2f_down(B, A, T, c, s, cs, tid);
    __syncthreads();
    c2f_up_write<OUT_NCHW>(A, B, T, c, s, cs, fine, coarse, diff, tid);
}
// fg_warp_faces: LDS: fg_warp_faces_lds_bytes (<= FG_FACES_MAX_LDS, checked by the entry); the limit of each instance is raised
// once per context
size_t fg_warp_faces_lds_bytes(int c, int hw, int ww, int s, int cs) {
    const size_t Ew = (size_t)c * hw * ww, Ec = (size_t)c * cs * cs;
    return (((((Ew > Ec ? Ew : Ec) + 3) & ~(size_t)3) + (size_t)c * s * s) * sizeof(float) + ((size_t)3 * s + cs) * sizeof(ScaleTerm) + 15) & ~(size_t)15;
}
int fg_launch_warp_faces(fg_ctx* ctx, const float* set, long long n_set, int c, int hs, int ws, int set_nchw, const int* idx, const float* mats,
                         const float* gains, int n, int hw, int ww, int s, int cs, float* fine, float* coarse, float* diff, int out_nchw,
                         int edge) {
    static_assert(sizeof(ScaleTerm) == FG_SCALE_PLAN_BYTES, "the header of fg_warp_faces states the size of a scale plan");
    const size_t lds = fg_warp_faces_lds_bytes(c, hw, ww, s, cs);
    const dim3 images((unsigned)n);
    if (c == 1) set_nchw = out_nchw = 1;
#define FACES(SN, ON)                                                                                                            \
    static char attr_key;                                                                                                        \
    if (fg_attr_first(ctx, &attr_key))                                                                                           \
        FG_HIP(ctx, hipFuncSetAttribute((const void*)warp_faces_kernel<SN, ON>, hipFuncAttributeMaxDynamicSharedMemorySize,      \
                                        (int)FG_FACES_MAX_LDS));                                                                 \
    hipLaunchKernelGGL((warp_faces_kernel<SN, ON>), images, dim3(256), lds, ctx->stream, set, n_set, idx, mats, gains, c, hs, ws, hw, ww, \
                       s, cs, fine, coarse, diff, edge)
    FG_BY_LAYOUT(set_nchw, out_nchw, FACES)
#undef FACES
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}
// fg_warp_faces_u8: the same grid, block and LDS; the taps read single bytes, so any base will do
int fg_launch_warp_faces_u8(fg_ctx* ctx, const uint8_t* set, long long n_set, int c, int hs, int ws, int set_nchw, const int* idx,
                            const float* mats, const float* gains, int n, int hw, int ww, int s, int cs, float* fine, float* coarse,
                            float* diff, int out_nchw, int edge) {
    const size_t lds = fg_warp_faces_lds_bytes(c, hw, ww, s, cs);
    const dim3 images((unsigned)n);
    if (c == 1) set_nchw = out_nchw = 1;
#define FACES_U8(SN, ON)                                                                                                         \
    static char attr_key;                                                                                                        \
    if (fg_attr_first(ctx, &attr_key))                                                                                           \
        FG_HIP(ctx, hipFuncSetAttribute((const void*)warp_faces_kernel<SN, ON, uint8_t>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                        (int)FG_FACES_MAX_LDS));                                                                 \
    hipLaunchKernelGGL((warp_faces_kernel<SN, ON, uint8_t>), images, dim3(256), lds, ctx->stream, set, n_set, idx, mats, gains, c, hs, ws, \
                       hw, ww, s, cs, fine, coarse, diff, edge)
    FG_BY_LAYOUT(set_nchw, out_nchw, FACES_U8)
#undef FACES_U8
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}
// fg_warp_faces_u8_y: fg_launch_warp_faces' grid, block and LDS at c == 1; the taps read the R, G, B bytes of a pixel one by one, so
// any base will do
int fg_launch_warp_faces_u8_y(fg_ctx* ctx, const uint8_t* set, long long n_set, int hs, int ws, int set_nchw, const int* idx, const float* mats,
                              const float* gains, int n, int hw, int ww, int s, int cs, float* fine, float* coarse, float* diff, int edge) {
    const size_t lds = fg_warp_faces_lds_bytes(1, hw, ww, s, cs);
    const dim3 images((unsigned)n);
    const wi_y8* luma = reinterpret_cast<const wi_y8*>(set);
#define FACES_Y(SN, ON)                                                                                                          \
    static char attr_key;                                                                                                        \
    if (fg_attr_first(ctx, &attr_key))                                                                                           \
        FG_HIP(ctx, hipFuncSetAttribute((const void*)warp_faces_kernel<SN, ON, wi_y8>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                        (int)FG_FACES_MAX_LDS));                                                                 \
    hipLaunchKernelGGL((warp_faces_kernel<SN, ON, wi_y8>), images, dim3(256), lds, ctx->stream, luma, n_set, idx, mats, gains, 1, hs, ws, \
                       hw, ww, s, cs, fine, coarse, diff, edge)
    if (set_nchw) { FACES_Y(true, true); } else { FACES_Y(false, true); }
#undef FACES_Y
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// fg_draw_transforms (include/facegen_hip.h): the random transforms of n images, drawn from the Philox stream and assembled into the
// mats / gains of fg_warp_images on the device.  One thread per image: three quads (twelve words, a fixed word per pick), the picks,
// sin / cos of whole degrees by the header's polynomial, the closed-form inverse of runtime.Augmenter.matrix, six + one 4-byte stores.
// All arithmetic is fp64 with every operation rounded on its own, in the header's order (no FMA contraction): a numpy float64
// restatement matches bit for bit.  No LDS, no scratch; nothing on the device is read.
// ---------------------------------------------------------------------------------------------------------------------------------
// sin(x) = x * P(x*x), cos(x) = Q(x*x) for |x| <= pi/4: the Taylor coefficients (-1)^i / (2i+1)!, i = 8 .. 0, and (-1)^i / (2i)!,
// i = 9 .. 0, each the double nearest to the quotient (the factorials are exact in fp64, the division is rounded once at compile time)
__device__ __forceinline__ double fg_deg_sin_poly(double x) {
#pragma clang fp contract(off)
    constexpr double c[9] = {1.0, -1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0, 1.0 / 6227020800.0,
                             -1.0 / 1307674368000.0, 1.0 / 355687428096000.0};
    const double z = x * x;
    double p = c[8];
#pragma unroll
    for (int i = 7; i >= 0; --i) p = p * z + c[i];
    return x * p;
}
__device__ __forceinline__ double fg_deg_cos_poly(double x) {
#pragma clang fp contract(off)
    constexpr double c[10] = {1.0, -1.0 / 2.0, 1.0 / 24.0, -1.0 / 720.0, 1.0 / 40320.0, -1.0 / 3628800.0, 1.0 / 479001600.0,
                              -1.0 / 87178291200.0, 1.0 / 20922789888000.0, -1.0 / 6402373705728000.0};
    const double z = x * x;
    double p = c[9];
#pragma unroll
    for (int i = 8; i >= 0; --i) p = p * z + c[i];
    return p;
}
// sin and cos of k whole degrees: k to [0, 360), the quadrant q and r in [0, 90); the polynomial's argument never exceeds 45 degrees
__device__ __forceinline__ void fg_deg_sincos(long long k, double& s, double& c) {
#pragma clang fp contract(off)
    int m = (int)(k % 360);
    if (m < 0) m += 360;
    const int q = m / 90, r = m % 90;
    const double D = 0x1.1df46a2529d39p-6;
    double s0, c0;
    if (r <= 45) { const double x = (double)r * D; s0 = fg_deg_sin_poly(x); c0 = fg_deg_cos_poly(x); }
    else { const double x = (double)(90 - r) * D; s0 = fg_deg_cos_poly(x); c0 = fg_deg_sin_poly(x); }
    if (q == 0) { s = s0; c = c0; }
    else if (q == 1) { s = c0; c = 0.0 - s0; }
    else if (q == 2) { s = 0.0 - s0; c = 0.0 - c0; }
    else { s = 0.0 - c0; c = s0; }
}
__device__ __forceinline__ long long fg_draw_int(uint32_t w, int lo, int hi) {
    return (long long)lo + (long long)(((uint64_t)w * (uint64_t)((long long)hi - lo + 1)) >> 32);
}
__global__ __launch_bounds__(256) void draw_transforms_kernel(const fg_augment_spec sp, uint64_t seed, uint64_t offset, int n, int hs, int ws,
                                                              int ho, int wo, float* __restrict__ mats, float* __restrict__ gains) {
#pragma clang fp contract(off)
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x) {
        uint32_t w[12];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const uint64_t ctr = offset + 3ull * (uint64_t)j + (uint64_t)t;
            philox4x32((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w + 4 * t);
        }
        const bool hf = sp.hflip && (w[0] >> 31), vf = sp.vflip && (w[1] >> 31);
        const double U = 1.0 / 16777216.0;
        const double zx = sp.zoom_lo + ((double)(w[2] >> 8) * U) * (sp.zoom_hi - sp.zoom_lo);
        const double zy = sp.zoom_equal ? zx : sp.zoom_lo + ((double)(w[3] >> 8) * U) * (sp.zoom_hi - sp.zoom_lo);
        const long long rot = fg_draw_int(w[4], sp.rot_lo, sp.rot_hi), sh = fg_draw_int(w[5], sp.shear_lo, sp.shear_hi);
        const long long tx = fg_draw_int(w[6], sp.tx_lo, sp.tx_hi), ty = fg_draw_int(w[7], sp.ty_lo, sp.ty_hi);
        const double gain = sp.gain_lo + ((double)(w[8] >> 8) * U) * (sp.gain_hi - sp.gain_lo);
        double sr, cr, srs, crs;
        fg_deg_sincos(rot, sr, cr);
        fg_deg_sincos(rot + sh, srs, crs);
        const double a = zx * cr, b = 0.0 - zy * srs, c = zx * sr, d = zy * crs;
        const double det = a * d - b * c;
        const double ia = d / det, ib = (0.0 - b) / det, ic = (0.0 - c) / det, id = a / det;
        const int cx = wo / 2, cy = ho / 2;
        const double qx = (double)((long long)cx + tx), qy = (double)((long long)cy + ty);
        double m0 = ia + 0.0, m1 = ib + 0.0, m2 = ((double)cx - (ia * qx + ib * qy)) + (double)(ws - wo) / 2.0;
        double m3 = ic + 0.0, m4 = id + 0.0, m5 = ((double)cy - (ic * qx + id * qy)) + (double)(hs - ho) / 2.0;
        if (hf) { m0 = 0.0 - m0; m1 = 0.0 - m1; m2 = (double)(ws - 1) - m2; }
        if (vf) { m3 = 0.0 - m3; m4 = 0.0 - m4; m5 = (double)(hs - 1) - m5; }
        float* o = mats + 6 * j;
        o[0] = (float)m0; o[1] = (float)m1; o[2] = (float)m2; o[3] = (float)m3; o[4] = (float)m4; o[5] = (float)m5;
        if (gains) gains[j] = (float)gain;
    }
}
int fg_launch_draw_transforms(fg_ctx* ctx, const fg_augment_spec& spec, uint64_t seed, uint64_t offset, int n, int hs, int ws, int ho, int wo,
                              float* mats, float* gains) {
    if (n == 0) return FG_OK;
    hipLaunchKernelGGL(draw_transforms_kernel, FG_GRID((long long)n, 256), dim3(256), 0, ctx->stream, spec, seed, offset, n, hs, ws, ho, wo, mats, gains);
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}
