// Sampler level of libfacegen_hip.so: sample.lua:69-90 / NN_UTILS.visualizeProgress (nn_utils.lua:131-204) on the device.
//   fg_rank_scores  = the sort of sortImagesByPrediction (nn_utils.lua:99-106) with a fixed tie rule,
//   fg_image_grid   = image.toDisplayTensor{input, nrow, padding} over a (ranked) selection of a batch,
//   fg_sampler      = createNoiseInputs + createImagesFromNoise + the prediction loop + both rankings behind one object.
#include "fg_internal.h"
#include "../../include/facegen_hip.h"

// ---------------------------------------------------------------------------------------------------------------------
// Ranking.  Every image gets the 64-bit key (order-preserving transform of its score | its index); keys are distinct, so
// rank[i] = #{j : key[j] < key[i]} is a permutation and order[rank[i]] = i needs neither a sort network nor an atomic.
// n^2 / 2^32 compares of 64-bit integers: 1024 scores are 4 blocks, 65536 scores 256 blocks of ~16 k LDS reads per lane.
// ---------------------------------------------------------------------------------------------------------------------
#define FG_RANK_MAX_N (1 << 20)
#define RK_TILE 2048              // keys staged per pass (16 KB of LDS)
#define RK_IPT 4                  // scores ranked per lane: one LDS read serves four compares

struct RankArgs {
    const float* scores;
    int n, ndir;
    int asc[2];
    int* order[2];
};

// high word of the key: ascending in the wanted direction, -0 == +0, NaN behind everything (also behind +-inf) both ways
__device__ __forceinline__ unsigned long long rank_key(float s, int i, int ascending) {
    unsigned u = 0xFFFFFFFFu;
    if (s == s) {
        unsigned b = __float_as_uint(s);
        if ((b << 1) == 0u) b = 0u;                                       // -0.0f ties with +0.0f
        u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);                   // unsigned order == float order, in [0x007FFFFF, 0xFF800000]
        if (!ascending) u = ~u;                                           // same interval, reversed: never 0xFFFFFFFF
    }
    return ((unsigned long long)u << 32) | (unsigned)i;
}

// block = 256 scores (4 per lane) x 4 waves, each wave counting over its quarter of every staged tile
__global__ __launch_bounds__(256) void rank_count_kernel(RankArgs a) {
    __shared__ unsigned long long tile[RK_TILE];
    __shared__ int part[4][64 * RK_IPT];
    const int d = blockIdx.y, n = a.n, asc = a.asc[d];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.x * (64 * RK_IPT);
    unsigned long long mine[RK_IPT];
    int cnt[RK_IPT];
#pragma unroll
    for (int e = 0; e < RK_IPT; ++e) {
        const int i = i0 + e * 64 + lane;
        mine[e] = i < n ? rank_key(a.scores[i], i, asc) : 0ull;
        cnt[e] = 0;
    }
    for (int j0 = 0; j0 < n; j0 += RK_TILE) {
        for (int t = threadIdx.x; t < RK_TILE; t += 256) {
            const int j = j0 + t;
            tile[t] = j < n ? rank_key(a.scores[j], j, asc) : ~0ull;      // the filler is below no key
        }
        __syncthreads();
        const unsigned long long* tw = tile + wave * (RK_TILE / 4);
#pragma unroll 8
        for (int t = 0; t < RK_TILE / 4; ++t) {
            const unsigned long long k = tw[t];
#pragma unroll
            for (int e = 0; e < RK_IPT; ++e) cnt[e] += (k < mine[e]) ? 1 : 0;
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < RK_IPT; ++e) part[wave][e * 64 + lane] = cnt[e];
    __syncthreads();
    const int l = threadIdx.x, i = i0 + l;
    if (i < n) a.order[d][part[0][l] + part[1][l] + part[2][l] + part[3][l]] = i;     // a rank below n: n distinct keys
}

static int launch_rank(fg_ctx* ctx, const RankArgs& a) {
    hipLaunchKernelGGL(rank_count_kernel, dim3(fg_cdiv(a.n, 64 * RK_IPT), a.ndir), dim3(256), 0, ctx->stream, a);
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Display grid.  Pass 1: up to GRID_NB blocks leave the min / max of their images (fixed image -> block assignment, fixed
// tree); pass 2: every block folds those partials (same order in every block) and writes its share of the CHW grid.
// ---------------------------------------------------------------------------------------------------------------------
#define GRID_NB (FG_GRID_PART_FLOATS / 2)

__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* sh) {
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { sh[(threadIdx.x >> 6) * 2] = mn; sh[(threadIdx.x >> 6) * 2 + 1] = mx; }
    __syncthreads();
    mn = fminf(fminf(sh[0], sh[2]), fminf(sh[4], sh[6]));
    mx = fmaxf(fmaxf(sh[1], sh[3]), fmaxf(sh[5], sh[7]));
}

__global__ __launch_bounds__(256) void grid_minmax_kernel(const float* __restrict__ img, const int* __restrict__ order, int k,
                                                          long long per, float* __restrict__ part) {
    __shared__ float sh[8];
    float mn = INFINITY, mx = -INFINITY;
    for (int j = blockIdx.x; j < k; j += gridDim.x) {
        const float* p = img + (long long)(order ? order[j] : j) * per;
        for (long long e = threadIdx.x; e < per; e += 256) {
            const float v = p[e];
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    }
    block_minmax(mn, mx, sh);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = mn; part[2 * blockIdx.x + 1] = mx; }
}

struct GridArgs {
    const float* img; const int* order; const float* part; float* grid; float* minmax_out;
    int nb, k, c, h, w, xmaps, padding, normalize, GH, GW;
};

__global__ __launch_bounds__(256) void grid_fill_kernel(GridArgs a) {
    __shared__ float sh[8];
    float mn = INFINITY, mx = -INFINITY;
    if ((int)threadIdx.x < a.nb) { mn = a.part[2 * threadIdx.x]; mx = a.part[2 * threadIdx.x + 1]; }
    block_minmax(mn, mx, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.minmax_out) { a.minmax_out[0] = mn; a.minmax_out[1] = mx; }
    const long long total = (long long)a.c * a.GH * a.GW;
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int X = (int)(o % a.GW), Y = (int)((o / a.GW) % a.GH), ch = (int)(o / ((long long)a.GW * a.GH));
    const int ch_h = a.h + a.padding, ch_w = a.w + a.padding;
    const int row = Y / ch_h, col = X / ch_w;
    const int y = Y - row * ch_h - a.padding / 2, x = X - col * ch_w - a.padding / 2;
    const int j = row * a.xmaps + col;
    float v = mx;                                                          // padding and the cells behind image k - 1
    if (j < a.k && y >= 0 && y < a.h && x >= 0 && x < a.w) {
        const long long src = a.order ? a.order[j] : j;
        v = a.img[((src * a.h + y) * a.w + x) * a.c + ch];
    }
    if (a.normalize) v = (mx == mn) ? 0.f : (v - mn) / (mx - mn);
    a.grid[o] = v;
}

// scratch: 2 * GRID_NB floats (FG_GRID_PART_FLOATS of the context)
static int launch_image_grid(fg_ctx* ctx, const float* img, const int* order, int k, int c, int h, int w, int nrow, int padding,
                             int normalize, float* grid, float* minmax_out, float* scratch) {
    GridArgs a;
    a.img = img; a.order = order; a.part = scratch; a.grid = grid; a.minmax_out = minmax_out;
    a.nb = k < GRID_NB ? k : GRID_NB; a.k = k; a.c = c; a.h = h; a.w = w; a.padding = padding; a.normalize = normalize;
    a.xmaps = nrow < k ? nrow : k;
    const int ymaps = (k + a.xmaps - 1) / a.xmaps;
    a.GH = ymaps * (h + padding); a.GW = a.xmaps * (w + padding);
    hipLaunchKernelGGL(grid_minmax_kernel, dim3(a.nb), dim3(256), 0, ctx->stream, img, order, k, (long long)h * w * c, scratch);
    FG_CHECK_LAUNCH(ctx);
    const long long total = (long long)c * a.GH * a.GW;
    hipLaunchKernelGGL(grid_fill_kernel, dim3(fg_cdiv(total, 256)), dim3(256), 0, ctx->stream, a);
    FG_CHECK_LAUNCH(ctx);
    return FG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// fg_sampler
// ---------------------------------------------------------------------------------------------------------------------
struct fg_sampler {
    fg_ctx* ctx = nullptr;
    fg_net *G = nullptr, *D = nullptr;
    int maxN = 0, chunk = 0;
    float *ws = nullptr, *wsG = nullptr, *wsD = nullptr;
    size_t wsG_bytes = 0, wsD_bytes = 0;
    long long gin = 0, img = 0;                                   // floats per noise vector / per image
    int ic = 0, ih = 0, iw = 0;
    long long o_noise = 0, o_images = 0, o_preds = 0, o_desc = 0, o_asc = 0, total = 0;
    uint64_t seed = 1, offset = 0;
};

static inline long long sal64(long long v) { return (v + 63) / 64 * 64; }

static void sampler_layout(fg_sampler* s) {
    long long off = 0;
    auto take = [&](long long n) { const long long o = off; off += sal64(n); return o; };
    const long long N = s->maxN;
    s->o_noise = take(N * s->gin);
    s->o_images = take(N * s->img);
    s->o_preds = take(N);
    s->o_desc = take(N);
    s->o_asc = take(N);
    s->total = off;
}

static void sampler_dims(fg_sampler* s) {
    int c = 0, h = 0, w = 0;
    fg_net_in_dims(s->G, &c, &h, &w);
    s->gin = (long long)c * h * w;
    fg_net_in_dims(s->D, &s->ic, &s->ih, &s->iw);
    s->img = (long long)s->ic * s->ih * s->iw;
}

static int sampler_check(fg_sampler* s, int n, const char* who) {
    if (!s) return FG_ERR_INVALID;
    if (!s->wsG || !s->wsD) return fg_set_err(s->ctx, FG_ERR_INVALID, "%s: fg_sampler_bind_workspaces first", who);
    if (n < 1 || n > s->maxN) return fg_set_err(s->ctx, FG_ERR_INVALID, "%s: %d images (1..%d, the max_images of fg_sampler_create)", who, n, s->maxN);
    return FG_OK;
}

static int sampler_rank(fg_sampler* s, int n) {
    RankArgs a;
    a.scores = s->ws + s->o_preds; a.n = n; a.ndir = 2;
    a.asc[0] = 0; a.order[0] = (int*)(s->ws + s->o_desc);
    a.asc[1] = 1; a.order[1] = (int*)(s->ws + s->o_asc);
    return launch_rank(s->ctx, a);
}

extern "C" {
#pragma GCC visibility push(default)

size_t fg_rank_scores_workspace_bytes(int n) { (void)n; return 0; }

int fg_rank_scores(fg_ctx* ctx, const float* scores, int n, int ascending, int* order_out, void* scratch, size_t scratch_bytes) {
    (void)scratch; (void)scratch_bytes;
    if (!ctx || !scores || !order_out || n < 1) return fg_set_err(ctx, FG_ERR_INVALID, "fg_rank_scores: bad argument");
    if (n > FG_RANK_MAX_N) return fg_set_err(ctx, FG_ERR_UNSUPPORTED, "fg_rank_scores: n = %d exceeds the %d scores one call ranks", n, FG_RANK_MAX_N);
    RankArgs a;
    a.scores = scores; a.n = n; a.ndir = 1;
    a.asc[0] = a.asc[1] = ascending ? 1 : 0; a.order[0] = a.order[1] = order_out;
    return launch_rank(ctx, a);
}

int fg_image_grid(fg_ctx* ctx, const float* images_nhwc, const int* order, int k, int c, int h, int w, int nrow, int padding,
                  int normalize, float* grid_chw, float* minmax_out) {
    if (!ctx || !images_nhwc || !grid_chw || k < 1 || c < 1 || h < 1 || w < 1 || nrow < 1 || padding < 0)
        return fg_set_err(ctx, FG_ERR_INVALID, "fg_image_grid: bad argument");
    return launch_image_grid(ctx, images_nhwc, order, k, c, h, w, nrow, padding, normalize ? 1 : 0, grid_chw, minmax_out, ctx->grid_part);
}

size_t fg_sampler_workspace_bytes(const fg_net* G, const fg_net* D, int max_images) {
    if (!G || !D || max_images < 1) return 0;
    fg_sampler t;
    t.G = (fg_net*)G; t.D = (fg_net*)D; t.maxN = max_images;
    sampler_dims(&t);
    sampler_layout(&t);
    return (size_t)t.total * sizeof(float);
}

int fg_sampler_create(fg_ctx* ctx, fg_net* G, fg_net* D, int max_images, int chunk, void* ws, size_t ws_bytes, fg_sampler** out) {
    if (!ctx || !G || !D || !ws || !out || max_images < 1 || chunk < 1) return fg_set_err(ctx, FG_ERR_INVALID, "fg_sampler_create: bad argument");
    if ((uintptr_t)ws & 255) return fg_set_err(ctx, FG_ERR_INVALID, "fg_sampler_create: workspace must be 256-byte aligned");
    if (max_images > FG_RANK_MAX_N) return fg_set_err(ctx, FG_ERR_UNSUPPORTED, "fg_sampler_create: max_images = %d exceeds the %d scores one ranking takes", max_images, FG_RANK_MAX_N);
    fg_sampler* s = new fg_sampler();
    s->ctx = ctx; s->G = G; s->D = D; s->maxN = max_images; s->chunk = chunk; s->ws = (float*)ws;
    sampler_dims(s);
    int gc = 0, gh = 0, gw = 0, oc = 0, oh = 0, ow = 0, rc = FG_OK;
    fg_net_in_dims(G, &gc, &gh, &gw);
    fg_net_out_dims(G, &oc, &oh, &ow);
    if (gh * gw != 1)   // the c2f pair: G{noise[S][S][1], cond[S][S][C]} -> JoinTable, D{x, cond} -> CAddTable (fg_gan table_inputs = 1)
        rc = fg_set_err(ctx, FG_ERR_UNSUPPORTED, "fg_sampler_create: table-input nets are not sampled (G takes a %dx%dx%d map, not a noise vector)", gc, gh, gw);
    if (!rc && (long long)oc * oh * ow != s->img) rc = fg_set_err(ctx, FG_ERR_INVALID, "fg_sampler_create: G produces %dx%dx%d, D takes %dx%dx%d", oc, oh, ow, s->ic, s->ih, s->iw);
    fg_net_out_dims(D, &oc, &oh, &ow);
    if (!rc && oc * oh * ow != 1) rc = fg_set_err(ctx, FG_ERR_INVALID, "fg_sampler_create: D must end in one probability");
    // fg_net_forward_to wants 16-byte aligned inputs and outputs: chunk i of the noise / image buffers starts at i * chunk samples
    if (!rc && ((chunk * s->gin) % 4 || (chunk * s->img) % 4))
        rc = fg_set_err(ctx, FG_ERR_UNSUPPORTED, "fg_sampler_create: chunk %d of %lld-float noise vectors / %lld-float images does not start every chunk on 16 bytes", chunk, s->gin, s->img);
    if (!rc) {
        sampler_layout(s);
        if ((size_t)s->total * sizeof(float) > ws_bytes) rc = fg_set_err(ctx, FG_ERR_WORKSPACE, "fg_sampler_create: workspace %zu < %lld bytes", ws_bytes, s->total * 4LL);
    }
    if (rc) { delete s; return rc; }
    *out = s;
    return FG_OK;
}

int fg_sampler_destroy(fg_sampler* s) { delete s; return FG_OK; }

int fg_sampler_bind_workspaces(fg_sampler* s, void* wsG, size_t wsG_bytes, void* wsD, size_t wsD_bytes) {
    if (!s || !wsG || !wsD) return fg_set_err(s ? s->ctx : nullptr, FG_ERR_INVALID, "fg_sampler_bind_workspaces: null argument");
    const size_t needG = fg_net_workspace_bytes(s->G, s->chunk), needD = fg_net_workspace_bytes(s->D, s->chunk);
    if (wsG_bytes < needG || wsD_bytes < needD)
        return fg_set_err(s->ctx, FG_ERR_WORKSPACE, "fg_sampler_bind_workspaces: chunk %d needs %zu / %zu bytes (G / D), bound %zu / %zu", s->chunk, needG, needD, wsG_bytes, wsD_bytes);
    s->wsG = (float*)wsG; s->wsG_bytes = wsG_bytes; s->wsD = (float*)wsD; s->wsD_bytes = wsD_bytes;
    return FG_OK;
}

int fg_sampler_set_seed(fg_sampler* s, uint64_t seed, uint64_t offset) {
    if (!s) return FG_ERR_INVALID;
    s->seed = seed; s->offset = offset;
    return FG_OK;
}

int fg_sampler_buffer(const fg_sampler* s, int what, long long* offset_floats, long long* count) {
    if (!s) return FG_ERR_INVALID;
    long long o = -1, c = 0;
    switch (what) {
        case FG_SAMPLER_NOISE: o = s->o_noise; c = s->maxN * s->gin; break;
        case FG_SAMPLER_IMAGES: o = s->o_images; c = s->maxN * s->img; break;
        case FG_SAMPLER_PREDS: o = s->o_preds; c = s->maxN; break;
        case FG_SAMPLER_ORDER_DESC: o = s->o_desc; c = s->maxN; break;
        case FG_SAMPLER_ORDER_ASC: o = s->o_asc; c = s->maxN; break;
        default: return fg_set_err(s->ctx, FG_ERR_INVALID, "fg_sampler_buffer: unknown buffer %d", what);
    }
    if (offset_floats) *offset_floats = o;
    if (count) *count = c;
    return FG_OK;
}

int fg_sample_generate(fg_sampler* s, int n, const float* noise) {
    int rc = sampler_check(s, n, "fg_sample_generate");
    if (rc) return rc;
    const float* nz = noise;
    if (!nz) {          // NN_UTILS.createNoiseInputs: uniform(-1, 1) (nn_utils.lua:37), all n vectors from one launch
        const long long cnt = (long long)n * s->gin;
        if ((rc = fg_launch_rng_uniform(s->ctx, s->seed, s->offset, s->ws + s->o_noise, cnt, -1.f, 1.f))) return rc;
        s->offset += (uint64_t)((cnt + 3) / 4);
        nz = s->ws + s->o_noise;
    }
    float* images = s->ws + s->o_images;
    for (int i = 0; i < n; i += s->chunk) {
        const int b = n - i < s->chunk ? n - i : s->chunk;
        long long off = 0;
        rc = fg_net_forward_to(s->G, b, nz + (long long)i * s->gin, s->wsG, s->wsG_bytes, 0, nullptr, 0, &off, images + (long long)i * s->img);
        if (rc == FG_PAUSED_SYNC) return fg_set_err(s->ctx, FG_ERR_UNSUPPORTED, "fg_sample_generate: G paused for a sync-BN exchange in evaluate mode");
        if (rc) return rc;
    }
    return FG_OK;
}

int fg_sample_score(fg_sampler* s, int n, const float* images) {
    int rc = sampler_check(s, n, "fg_sample_score");
    if (rc) return rc;
    const float* im = images ? images : s->ws + s->o_images;
    float* preds = s->ws + s->o_preds;
    const bool direct = (s->chunk & 3) == 0;          // every chunk's slice of PREDS starts on 16 bytes
    for (int i = 0; i < n; i += s->chunk) {
        const int b = n - i < s->chunk ? n - i : s->chunk;
        long long off = 0;
        rc = fg_net_forward_to(s->D, b, im + (long long)i * s->img, s->wsD, s->wsD_bytes, 0, nullptr, 0, &off, direct ? preds + i : nullptr);
        if (rc == FG_PAUSED_SYNC) return fg_set_err(s->ctx, FG_ERR_UNSUPPORTED, "fg_sample_score: D paused for a sync-BN exchange in evaluate mode");
        if (rc) return rc;
        if (!direct && (rc = fg_launch_copy(s->ctx, s->wsD + off, preds + i, b))) return rc;
    }
    return FG_OK;
}

int fg_sample(fg_sampler* s, int n, const float* noise) {
    int rc = fg_sample_generate(s, n, noise);
    if (rc) return rc;
    if ((rc = fg_sample_score(s, n, nullptr))) return rc;          // once: evaluate mode is deterministic, "best" and "worst" share it
    return sampler_rank(s, n);
}

#pragma GCC visibility pop
}  // extern "C"
