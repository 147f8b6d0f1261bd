// Whole volumes from blended windows (PHISeg3D.predict_volume, models/phiseg3D.py): the four kernels around the two plans of
// predict() when they run on a window of a volume that is larger than - or not shaped like - what the net was trained at.
//   - uz_vol_window_gather: the window of the source volume, zero beyond its faces, into the trunk plan's input;
//   - uz_vol_window_noise: the window's crop of one latent level's noise field into the draw plan's noise operand;
//   - uz_vol_window_accum: one sample of one window - the level logits read as uz_vol_sample_accum reads them, the sample's
//     probabilities times the voxel's blend weight added to that sample's fp64 accumulator over the WHOLE volume;
//   - uz_vol_window_finish: once per call, all S accumulators divided by the weight sum -> labels, probabilities, their mean, its
//     argmax and entropy.
// No atomics: a voxel is owned by one thread of a launch, and the launches of the overlapping windows are serialised by the
// stream, so the adds to a voxel happen in the order of the window grid and a repeated call is bit-equal.
// All four are streaming kernels, one element per thread, consecutive lanes on consecutive W: the finest level, the accumulators
// and every output are coalesced; the coarser levels repeat an element over f lanes and come out of cache.  The per-voxel
// arithmetic behind the fp32 sum of the logits is uz::sample_softmax (uz_common.h), the one predict.hip uses.
// Mirrored passes (the _ex entry points and uz_vol_window_noise; flip bit 0, 1, 2 = D, H, W): the window is mirrored within itself,
// net-frame voxel (z, y, x) is window voxel (z', y', x') with z' = wd - 1 - z where bit 0 is set.  A mirrored W reverses the lane
// order of one side of every kernel.  The accumulate numbers its threads by the WINDOW voxel, so the fp64 read-modify-write of acc and
// wsum ascends across a wave exactly as without a mirror and the fp32 level reads run backwards; gather and noise number theirs by the
// element they store and read backwards.  A reversed wave touches the same cache lines as an ascending one, only in the other lane
// order - it is put on the side that is read once, fp32, and where a line costs half of what it costs in fp64.
#include "uz_common.h"

namespace {

// dst is the C-channel slice of a plan volume [wd][Ctot][wh][ww]; element e = ((z * C + c) * wh + y) * ww + x of the slice.
__global__ __launch_bounds__(256) void vol_window_gather_k(const float* __restrict__ src, int C, int D, int H, int W, int oz, int oy, int ox,
                                                            float* __restrict__ dst, int Ctot, int wd, int wh, int ww, int n, int flip) {
    const long long e64 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e64 >= n) return;
    int e = (int)e64;
    const int x = e % ww; e /= ww;
    const int y = e % wh; e /= wh;
    const int c = e % C, z = e / C;
    const int gz = oz + (flip & 1 ? wd - 1 - z : z), gy = oy + (flip & 2 ? wh - 1 - y : y), gx = ox + (flip & 4 ? ww - 1 - x : x);
    float v = 0.f;
    if (gz < D && gy < H && gx < W) v = src[(((size_t)c * D + gz) * H + gy) * W + gx];     // (origins are >= 0)
    dst[(((size_t)z * Ctot + c) * wh + y) * ww + x] = v;
}

// field: one sample's row of a level's noise (C2, d, h, w), dense; dst: the C2-channel slice of a plan volume [cd][Ctot][ch][cw], element
// e as in the gather.  The crop lies inside the field (the host part checks), so every element has a source.
__global__ __launch_bounds__(256) void vol_window_noise_k(const float* __restrict__ field, int C2, int d, int h, int w, int oz, int oy, int ox,
                                                           float* __restrict__ dst, int Ctot, int cd, int ch, int cw, int n, int flip) {
    const long long e64 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e64 >= n) return;
    int e = (int)e64;
    const int x = e % cw; e /= cw;
    const int y = e % ch; e /= ch;
    const int c = e % C2, z = e / C2;
    const int gz = oz + (flip & 1 ? cd - 1 - z : z), gy = oy + (flip & 2 ? ch - 1 - y : y), gx = ox + (flip & 4 ? cw - 1 - x : x);
    dst[(((size_t)z * Ctot + c) * ch + y) * cw + x] = field[(((size_t)c * d + gz) * h + gy) * w + gx];
}

struct Window {
    int wd, wh, ww, oz, oy, ox, flip;
};

// One window voxel (z, y, x) per thread - the voxel it adds to, whatever the mirror; the net-frame voxel (nz, ny, nx) it reads the levels
// at is its mirror image.  acc: this sample's (K, D, H, W) accumulator, wsum: (D, H, W) or null (not the window's first sample).
// weight * p_k and the add are two roundings (no fused multiply-add), as the numpy twin of the tests evaluates them.
template <int K>
__global__ __launch_bounds__(256) void vol_window_accum_k(uz::VolLevels lv, int L, Window w, int D, int H, int W, const double* __restrict__ tz,
                                                           const double* __restrict__ ty, const double* __restrict__ tx, double* __restrict__ acc,
                                                           double* __restrict__ wsum) {
    const int hw = w.wh * w.ww;
    const long long q64 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q64 >= (long long)w.wd * hw) return;
    const int q = (int)q64, z = q / hw, r = q - z * hw, y = r / w.ww, x = r - y * w.ww;
    const int gz = w.oz + z, gy = w.oy + y, gx = w.ox + x;
    if (gz >= D || gy >= H || gx >= W) return;                                          // the overhang: read as zeros by the gather, never written
    const int nz = w.flip & 1 ? w.wd - 1 - z : z, ny = w.flip & 2 ? w.wh - 1 - y : y, nx = w.flip & 4 ? w.ww - 1 - x : x;
    float a[K];
    for (int j = 0; j < L; ++j) {
        const int l = j == 0 ? L - 1 : j - 1;                                           // last level first, then 0 .. L-2: the order of vol_sample_accum_k
        const int f = lv.f[l], Hl = w.wh / f, Wl = w.ww / f;
        const float* s = lv.p[l] + ((size_t)(nz / lv.fz[l]) * lv.ctot[l]) * Hl * Wl + (size_t)(ny / f) * Wl + nx / f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float v = s[(size_t)k * Hl * Wl];
            a[k] = j == 0 ? v : a[k] + v;
        }
    }
    double sv[K];
    uz::sample_softmax<K>(a, sv);
    const double wt = __dmul_rn(__dmul_rn(tz[z], ty[y]), tx[x]);
    const size_t n = (size_t)D * H * W, g = ((size_t)gz * H + gy) * W + gx;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const size_t o = (size_t)k * n + g;
        acc[o] = __dadd_rn(acc[o], __dmul_rn(wt, sv[k]));
    }
    if (wsum) wsum[g] = __dadd_rn(wsum[g], wt);
}

// One voxel per thread, all S accumulators in order: every accumulator is read once.  A voxel no window reached (wsum == 0, which the
// window grid of predict_volume excludes) gets label 0, probabilities 0 and entropy 0 instead of NaN.
template <int K>
__global__ __launch_bounds__(256) void vol_window_finish_k(const double* __restrict__ acc, const double* __restrict__ wsum, int S, int n,
                                                            uint8_t* __restrict__ labels, float* __restrict__ soft, float* __restrict__ mean_soft,
                                                            uint8_t* __restrict__ mean_label, float* __restrict__ entropy) {
    const long long q64 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q64 >= n) return;
    const int q = (int)q64;
    const double ws = wsum[q];
    double m[K];
#pragma unroll
    for (int k = 0; k < K; ++k) m[k] = 0.0;
    for (int s = 0; s < S; ++s) {
        const double* a = acc + (size_t)s * K * n + q;
        int best = 0;
        double bv = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double v = a[(size_t)k * n];
            if (k == 0 || v > bv) { bv = v; best = k; }                                 // first maximum of the unnormalised blend
            const double p = ws != 0.0 ? v / ws : 0.0;
            if (soft) soft[((size_t)s * K + k) * n + q] = (float)p;
            m[k] += p;                                                                  // ordered: s = 0 .. S-1
        }
        labels[(size_t)s * n + q] = (uint8_t)best;
    }
    double p[K], h;
    const int best = uz::mean_stats<K>(m, S, p, h);
#pragma unroll
    for (int k = 0; k < K; ++k) mean_soft[(size_t)k * n + q] = (float)p[k];
    if (mean_label) mean_label[q] = (uint8_t)best;
    if (entropy) entropy[q] = (float)h;
}

template <int K>
void launch_accum(int groups, hipStream_t st, const uz::VolLevels& lv, int L, const Window& w, int D, int H, int W, const double* tz, const double* ty,
                  const double* tx, double* acc, double* wsum) {
    hipLaunchKernelGGL(vol_window_accum_k<K>, dim3(groups), dim3(256), 0, st, lv, L, w, D, H, W, tz, ty, tx, acc, wsum);
}
template <int K>
void launch_finish(int groups, hipStream_t st, const double* acc, const double* wsum, int S, int n, uint8_t* labels, float* soft, float* mean_soft,
                   uint8_t* mean_label, float* entropy) {
    hipLaunchKernelGGL(vol_window_finish_k<K>, dim3(groups), dim3(256), 0, st, acc, wsum, S, n, labels, soft, mean_soft, mean_label, entropy);
}

}  // namespace

extern "C" int uz_vol_window_gather_ex(const float* src, int C, int D, int H, int W, int oz, int oy, int ox, float* dst, int Ctot,
                                       int wd, int wh, int ww, int flip, void* stream) {
    UZ_REQUIRE(flip >= 0 && flip <= 7, "vol_window_gather: flip mask %d outside 0..7", flip);
    UZ_REQUIRE(src && dst, "vol_window_gather: null pointer");
    UZ_REQUIRE(C >= 1 && Ctot >= C, "vol_window_gather: a slice of %d channels in a buffer of %d", C, Ctot);
    UZ_REQUIRE(D > 0 && H > 0 && W > 0 && wd > 0 && wh > 0 && ww > 0, "vol_window_gather: an empty volume or window");
    UZ_REQUIRE(oz >= 0 && oy >= 0 && ox >= 0, "vol_window_gather: origin below 0");
    const long long n = (long long)wd * C * wh * ww, ns = (long long)C * D * H * W;
    UZ_REQUIRE(n < (1ll << 31) && ns < (1ll << 31), "vol_window_gather: window or volume too large");
    hipLaunchKernelGGL(vol_window_gather_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, uz::S(stream), src, C, D, H, W, oz, oy, ox, dst, Ctot,
                       wd, wh, ww, (int)n, flip);
    return uz::check_launch("vol_window_gather_k");
}

extern "C" int uz_vol_window_gather(const float* src, int C, int D, int H, int W, int oz, int oy, int ox, float* dst, int Ctot,
                                    int wd, int wh, int ww, void* stream) {
    return uz_vol_window_gather_ex(src, C, D, H, W, oz, oy, ox, dst, Ctot, wd, wh, ww, 0, stream);
}

extern "C" int uz_vol_window_noise(const float* field, int C2, int d, int h, int w, int oz, int oy, int ox, int cd, int ch, int cw, int flip,
                                   float* dst, int Ctot, void* stream) {
    UZ_REQUIRE(flip >= 0 && flip <= 7, "vol_window_noise: flip mask %d outside 0..7", flip);
    UZ_REQUIRE(field && dst, "vol_window_noise: null pointer");
    UZ_REQUIRE(C2 >= 1 && Ctot >= C2, "vol_window_noise: a slice of %d channels in a buffer of %d", C2, Ctot);
    UZ_REQUIRE(d > 0 && h > 0 && w > 0 && cd > 0 && ch > 0 && cw > 0, "vol_window_noise: an empty field or crop");
    UZ_REQUIRE(oz >= 0 && oy >= 0 && ox >= 0 && cd <= d - oz && ch <= h - oy && cw <= w - ox,
               "vol_window_noise: the crop %d x %d x %d at (%d, %d, %d) leaves its field %d x %d x %d", cd, ch, cw, oz, oy, ox, d, h, w);
    const long long n = (long long)cd * C2 * ch * cw, nf = (long long)C2 * d * h * w;
    UZ_REQUIRE(n < (1ll << 31) && nf < (1ll << 31), "vol_window_noise: crop or field too large");
    hipLaunchKernelGGL(vol_window_noise_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, uz::S(stream), field, C2, d, h, w, oz, oy, ox, dst, Ctot,
                       cd, ch, cw, (int)n, flip);
    return uz::check_launch("vol_window_noise_k");
}

extern "C" int uz_vol_window_accum_ex(const float* const* s_ptrs, const int* ctot, const int* f, const int* fz, int L, int K, int wd, int wh, int ww,
                                      int oz, int oy, int ox, int D, int H, int W, const double* tz, const double* ty, const double* tx,
                                      double* acc, double* wsum, int add_weight, int flip, void* stream) {
    UZ_REQUIRE(flip >= 0 && flip <= 7, "vol_window_accum: flip mask %d outside 0..7", flip);
    UZ_REQUIRE(K >= 1 && K <= 8, "vol_window_accum: 1..8 classes supported (got %d)", K);
    UZ_REQUIRE(L >= 1 && L <= uz::VOL_LEVELS_MAX, "vol_window_accum: 1..8 levels supported (got %d)", L);
    UZ_REQUIRE(s_ptrs && ctot && f && fz && tz && ty && tx && acc && wsum, "vol_window_accum: null pointer");
    UZ_REQUIRE(D > 0 && H > 0 && W > 0 && wd > 0 && wh > 0 && ww > 0, "vol_window_accum: an empty volume or window");
    UZ_REQUIRE(oz >= 0 && oy >= 0 && ox >= 0, "vol_window_accum: origin below 0");
    const long long n = (long long)D * H * W, nw = (long long)wd * wh * ww;
    UZ_REQUIRE(n < (1ll << 31) && nw < (1ll << 31), "vol_window_accum: window or volume too large");
    uz::VolLevels lv = {};
    for (int l = 0; l < L; ++l) {
        UZ_REQUIRE(s_ptrs[l], "vol_window_accum: level %d is a null pointer", l);
        UZ_REQUIRE(f[l] >= 1 && fz[l] >= 1 && ctot[l] >= K, "vol_window_accum: level %d: factors below 1 or fewer channels than classes", l);
        UZ_REQUIRE(wd % fz[l] == 0 && wh % f[l] == 0 && ww % f[l] == 0, "vol_window_accum: level %d: the window is not level size x factor", l);
        lv.p[l] = s_ptrs[l]; lv.ctot[l] = ctot[l]; lv.f[l] = f[l]; lv.fz[l] = fz[l];
    }
    const Window w = {wd, wh, ww, oz, oy, ox, flip};
    const int r = (int)((nw + 255) / 256);
    double* ws = add_weight ? wsum : nullptr;
    hipStream_t st = uz::S(stream);
    switch (K) {
        case 1: launch_accum<1>(r, st, lv, L, w, D, H, W, tz, ty, tx, acc, ws); break;
        case 2: launch_accum<2>(r, st, lv, L, w, D, H, W, tz, ty, tx, acc, ws); break;
        case 3: launch_accum<3>(r, st, lv, L, w, D, H, W, tz, ty, tx, acc, ws); break;
        case 4: launch_accum<4>(r, st, lv, L, w, D, H, W, tz, ty, tx, acc, ws); break;
        case 5: launch_accum<5>(r, st, lv, L, w, D, H, W, tz, ty, tx, acc, ws); break;
        case 6: launch_accum<6>(r, st, lv, L, w, D, H, W, tz, ty, tx, acc, ws); break;
        case 7: launch_accum<7>(r, st, lv, L, w, D, H, W, tz, ty, tx, acc, ws); break;
        default: launch_accum<8>(r, st, lv, L, w, D, H, W, tz, ty, tx, acc, ws); break;
    }
    return uz::check_launch("vol_window_accum_k");
}

extern "C" int uz_vol_window_accum(const float* const* s_ptrs, const int* ctot, const int* f, const int* fz, int L, int K, int wd, int wh, int ww,
                                   int oz, int oy, int ox, int D, int H, int W, const double* tz, const double* ty, const double* tx,
                                   double* acc, double* wsum, int add_weight, void* stream) {
    return uz_vol_window_accum_ex(s_ptrs, ctot, f, fz, L, K, wd, wh, ww, oz, oy, ox, D, H, W, tz, ty, tx, acc, wsum, add_weight, 0, stream);
}

extern "C" int uz_vol_window_finish(const double* acc, const double* wsum, int K, int S, int D, int H, int W, uint8_t* labels, float* soft,
                                    float* mean_soft, uint8_t* mean_label, float* entropy, void* stream) {
    UZ_REQUIRE(K >= 1 && K <= 8, "vol_window_finish: 1..8 classes supported (got %d)", K);
    UZ_REQUIRE(acc && wsum && labels && mean_soft, "vol_window_finish: null pointer");
    UZ_REQUIRE(S > 0 && D > 0 && H > 0 && W > 0, "vol_window_finish: no samples or an empty volume");
    const long long n = (long long)D * H * W;
    UZ_REQUIRE(n < (1ll << 31), "vol_window_finish: volume too large");
    const int r = (int)((n + 255) / 256);
    hipStream_t st = uz::S(stream);
    switch (K) {
        case 1: launch_finish<1>(r, st, acc, wsum, S, (int)n, labels, soft, mean_soft, mean_label, entropy); break;
        case 2: launch_finish<2>(r, st, acc, wsum, S, (int)n, labels, soft, mean_soft, mean_label, entropy); break;
        case 3: launch_finish<3>(r, st, acc, wsum, S, (int)n, labels, soft, mean_soft, mean_label, entropy); break;
        case 4: launch_finish<4>(r, st, acc, wsum, S, (int)n, labels, soft, mean_soft, mean_label, entropy); break;
        case 5: launch_finish<5>(r, st, acc, wsum, S, (int)n, labels, soft, mean_soft, mean_label, entropy); break;
        case 6: launch_finish<6>(r, st, acc, wsum, S, (int)n, labels, soft, mean_soft, mean_label, entropy); break;
        case 7: launch_finish<7>(r, st, acc, wsum, S, (int)n, labels, soft, mean_soft, mean_label, entropy); break;
        default: launch_finish<8>(r, st, acc, wsum, S, (int)n, labels, soft, mean_soft, mean_label, entropy); break;
    }
    return uz::check_launch("vol_window_finish_k");
}
