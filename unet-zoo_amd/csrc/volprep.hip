// Raw BraTS cases onto the fixed extent, and maps back into native space (uz_api.h "volume preparation").
//
// uz_vol_prepare: crop_volume_allDim + crop_or_pad_slice_to_size + normalise_image of the reference's loaders, seven launches on
// the caller's stream; the box never visits the host.
//   bounds       one read of raw: a voxel with ANY channel > 0 widens its thread's box; wave shuffle, LDS, then the workgroup's own slice
//   fold bounds  one workgroup folds the slices in a fixed order, forms the per-axis descriptor {n, t, e} and writes info[16]
//   sums         over the placed block: per channel the sum (fp64) and the count of values != 0 -> slices;  fold -> count, mean
//   squares      over the placed block: per channel sum((x - mean)^2) in fp64 with the unrounded mean -> slices;  fold -> std
//   store        every target voxel: (x - f32(mean)) / f32(std) where x != 0 inside the block, 0 elsewhere; the mask travels along
// The three passes behind the descriptor walk the TARGET volume (its extent is known on the host, the box is not): a target voxel
// outside the placed block costs a thread no memory traffic.  A voxel's coordinates come from its linear index by multiplications
// (FastDiv); the divisors are host constants.
// Wide form (C == 4, raw and image 16-byte aligned): a voxel is one 16-byte load / store.  Scalar form: any C in 1 .. 8.
// The folds are launches of their own: folded in the prologue of the next pass, every workgroup would read every slice.
//
// uz_vol_restore: one thread per native element, or per 4 (fp32, uint8) or 16 (uint8) of them where out is aligned for the one store;
// the source is read element by element - the rows' Z is odd in real cases.  `place` is device data: clipped per voxel.
#include "uz_common.h"
#include <algorithm>
#include <climits>
#include <cstring>

namespace {

constexpr int TB = 256;             // threads of every pass
constexpr int CAP = 2048;           // workgroups of a pass at the most: eight per CU; the grid-stride loop covers the rest
constexpr int MAXC = UZ_VOL_PREP_MAX_CHANNELS;
constexpr int BSL = 8;              // int32 per bounds slice: {lo x, y, z, hi x, y, z, -, -}

typedef unsigned long long u64;

// n / d for 0 <= n < 2^31 and 1 <= d < 2^31 as one multiplication: k = 31 + ceil(log2 d), m = ceil(2^k / d) <= 2^32.  With
// e = m d - 2^k in [0, d): n m / 2^k = n / d + n e / (d 2^k), and n e < 2^31 d <= 2^k, so the excess stays below 1 / d: the floor is n / d.
struct FastDiv { u64 m; int k; };
FastDiv make_div(int d) {
    int l = 0;
    while ((1LL << l) < (long long)d) ++l;
    FastDiv f;
    f.k = 31 + l;
    f.m = ((1ULL << f.k) + (u64)d - 1ULL) / (u64)d;
    return f;
}
__device__ __forceinline__ unsigned fdiv(unsigned n, const FastDiv& f) { return (unsigned)(((u64)n * f.m) >> f.k); }

struct Geo {
    int C, X, Y, Z, Xt, Yt, Zt;
    FastDiv dZ, dY, dZt, dYt;
};

// ------------------------------------------------------------------------------------------------ bounds
template <bool WIDE>
__device__ __forceinline__ bool any_positive(const float* __restrict__ raw, unsigned v, int C) {
    if constexpr (WIDE) {
        const float4 a = reinterpret_cast<const float4*>(raw)[v];
        return a.x > 0.f || a.y > 0.f || a.z > 0.f || a.w > 0.f;
    } else {
        const float* q = raw + (size_t)v * C;
        bool p = false;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) p |= q[c] > 0.f;
        return p;
    }
}

// lo[3] (minimum) and hi[3] (maximum + 1, 0 = none) of a workgroup into thread 0
__device__ __forceinline__ void block_box(int (&lo)[3], int (&hi)[3], int (*sm)[6]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = uz::wave_min(lo[a]); hi[a] = uz::wave_max(hi[a]); }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { sm[wave][a] = lo[a]; sm[wave][3 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = min(min(sm[0][a], sm[1][a]), min(sm[2][a], sm[3][a]));
            hi[a] = max(max(sm[0][3 + a], sm[1][3 + a]), max(sm[2][3 + a], sm[3][3 + a]));
        }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(TB) void prep_bounds_k(const float* __restrict__ raw, Geo g, unsigned P, int* __restrict__ slices) {
    __shared__ int sm[4][6];
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {0, 0, 0};
    const unsigned stride = gridDim.x * TB;
    for (unsigned v = blockIdx.x * TB + threadIdx.x; v < P; v += stride) {
        if (any_positive<WIDE>(raw, v, g.C)) {
            const unsigned xy = fdiv(v, g.dZ), x = fdiv(xy, g.dY);
            const int c[3] = {(int)x, (int)(xy - x * (unsigned)g.Y), (int)(v - xy * (unsigned)g.Z)};
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], c[a]); hi[a] = max(hi[a], c[a] + 1); }
        }
    }
    block_box(lo, hi, sm);
    if (threadIdx.x == 0) {
        int* mine = slices + (size_t)blockIdx.x * BSL;
#pragma unroll
        for (int a = 0; a < 3; ++a) { mine[a] = lo[a]; mine[3 + a] = hi[a]; }
    }
}

// one workgroup: the slices in a fixed order, then the descriptor
__global__ __launch_bounds__(TB) void prep_fold_bounds_k(const int* __restrict__ slices, int G, int X, int Y, int Z, int Xt, int Yt, int Zt,
                                                          int placement, int* __restrict__ info) {
    __shared__ int sm[4][6];
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {0, 0, 0};
    for (int s = threadIdx.x; s < G; s += TB) {
        const int* sl = slices + (size_t)s * BSL;
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], sl[a]); hi[a] = max(hi[a], sl[3 + a]); }
    }
    block_box(lo, hi, sm);
    if (threadIdx.x == 0) {
        if (hi[0] == 0) {                                                   // no voxel > 0: every entry 0, flag bit 0
            for (int k = 0; k < 15; ++k) info[k] = 0;
            info[15] = 1;
            return;
        }
        const int T[3] = {Xt, Yt, Zt};
        int lost = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int s = hi[a] - lo[a], d = (T[a] < s ? s - T[a] : T[a] - s) / 2;
            int n = lo[a], t = 0, e = s;
            if (T[a] < s) { e = T[a]; lost = 2; if (placement == 0) n += d; }
            else if (placement == 0) t = d;
            info[a] = lo[a]; info[3 + a] = hi[a]; info[6 + a] = n; info[9 + a] = t; info[12 + a] = e;
        }
        info[15] = lost;
    }
}

// ------------------------------------------------------------------------------------------------ the placed block
// target voxel q -> the native voxel it shows, or false outside the placed block.  The descriptor is this call's own: n + e <= box end.
__device__ __forceinline__ bool placed(unsigned q, const Geo& g, const int* __restrict__ info, unsigned& nv) {
    const unsigned xy = fdiv(q, g.dZt), x = fdiv(xy, g.dYt);
    const int ix = (int)x - info[9], iy = (int)(xy - x * (unsigned)g.Yt) - info[10], iz = (int)(q - xy * (unsigned)g.Zt) - info[11];
    if ((unsigned)ix >= (unsigned)info[12] || (unsigned)iy >= (unsigned)info[13] || (unsigned)iz >= (unsigned)info[14]) return false;
    nv = ((unsigned)(info[6] + ix) * (unsigned)g.Y + (unsigned)(info[7] + iy)) * (unsigned)g.Z + (unsigned)(info[8] + iz);
    return true;
}

template <bool WIDE>
__device__ __forceinline__ void load_voxel(const float* __restrict__ raw, unsigned nv, int C, float (&x)[MAXC]) {
    if constexpr (WIDE) {
        const float4 a = reinterpret_cast<const float4*>(raw)[nv];
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
#pragma unroll
        for (int c = 4; c < MAXC; ++c) x[c] = 0.f;
    } else {
        const float* p = raw + (size_t)nv * C;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) x[c] = c < C ? p[c] : 0.f;
    }
}

// a slice of the sums: MAXC doubles, then MAXC counts
struct SumSlice { double s[MAXC]; long long n[MAXC]; };

// SQ = false: sum and count of the values != 0;  SQ = true: sum of (x - mean)^2 over them, mean = stats[c][1]
template <bool WIDE, bool SQ>
__global__ __launch_bounds__(TB) void prep_sums_k(const float* __restrict__ raw, Geo g, unsigned Pt, const int* __restrict__ info,
                                                  const double* __restrict__ stats, SumSlice* __restrict__ slices) {
    __shared__ double smd[4][MAXC];
    __shared__ int smn[4][MAXC];
    constexpr int NC = WIDE ? 4 : MAXC;
    double acc[NC], mean[NC];
    int cnt[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        acc[c] = 0.0; cnt[c] = 0;
        mean[c] = (SQ && c < g.C) ? stats[c * 3 + 1] : 0.0;
    }
    const unsigned stride = gridDim.x * TB;
    for (unsigned q = blockIdx.x * TB + threadIdx.x; q < Pt; q += stride) {
        unsigned nv;
        if (!placed(q, g, info, nv)) continue;
        float x[MAXC];
        load_voxel<WIDE>(raw, nv, g.C, x);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (x[c] != 0.f) {                                              // a channel beyond C reads as 0
                if constexpr (SQ) { const double d = (double)x[c] - mean[c]; acc[c] += d * d; }
                else { acc[c] += (double)x[c]; ++cnt[c]; }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        acc[c] = uz::wave_sum_d(acc[c]);
        const int n = uz::wave_sum(cnt[c]);
        if (lane == 0) { smd[wave][c] = acc[c]; smn[wave][c] = n; }
    }
    __syncthreads();
    if ((int)threadIdx.x < g.C) {
        const int c = threadIdx.x;
        SumSlice& mine = slices[blockIdx.x];
        mine.s[c] = ((smd[0][c] + smd[1][c]) + smd[2][c]) + smd[3][c];
        if constexpr (!SQ) mine.n[c] = (long long)smn[0][c] + smn[1][c] + smn[2][c] + smn[3][c];
    }
}

// workgroup = channel.  Thread t adds the slices t, t + 256, ... in that order; then the shuffle tree, then the four waves in order.
// phase 0: stats[c] = {count, mean, 0};  phase 1: stats[c][2] = sqrt(sum / count).  A channel without a value != 0: {0, 0, 0}.
__global__ __launch_bounds__(TB) void prep_fold_stats_k(const SumSlice* __restrict__ slices, int G, int phase, double* __restrict__ stats) {
    __shared__ double smd[4];
    __shared__ long long smn[4];
    const int c = blockIdx.x;
    double s = 0.0;
    long long n = 0;
    for (int k = threadIdx.x; k < G; k += TB) {
        s += slices[k].s[c];
        if (phase == 0) n += slices[k].n[c];
    }
    s = uz::wave_sum_d(s);
    n = uz::wave_sum(n);
    if ((threadIdx.x & 63) == 0) { smd[threadIdx.x >> 6] = s; smn[threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        s = ((smd[0] + smd[1]) + smd[2]) + smd[3];
        if (phase == 0) {
            n = smn[0] + smn[1] + smn[2] + smn[3];
            stats[c * 3] = (double)n;
            stats[c * 3 + 1] = n > 0 ? s / (double)n : 0.0;
            stats[c * 3 + 2] = 0.0;
        } else {
            const double cnt = stats[c * 3];
            stats[c * 3 + 2] = cnt > 0.0 ? sqrt(s / cnt) : 0.0;
        }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(TB) void prep_store_k(const float* __restrict__ raw, const uint8_t* __restrict__ mask, Geo g, unsigned Pt,
                                                   const int* __restrict__ info, const double* __restrict__ stats,
                                                   float* __restrict__ image, uint8_t* __restrict__ mask_out) {
    constexpr int NC = WIDE ? 4 : MAXC;
    float m[NC], s[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        m[c] = c < g.C ? (float)stats[c * 3 + 1] : 0.f;
        s[c] = c < g.C ? (float)stats[c * 3 + 2] : 1.f;
    }
    const unsigned stride = gridDim.x * TB;
    for (unsigned q = blockIdx.x * TB + threadIdx.x; q < Pt; q += stride) {
        float y[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) y[c] = 0.f;
        uint8_t mk = 0;
        unsigned nv;
        if (placed(q, g, info, nv)) {
            float x[MAXC];
            load_voxel<WIDE>(raw, nv, g.C, x);
#pragma unroll
            for (int c = 0; c < NC; ++c) y[c] = x[c] == 0.f ? 0.f : (x[c] - m[c]) / s[c];      // one subtraction, one IEEE division
            if (mask) mk = mask[nv];
        }
        if constexpr (WIDE) reinterpret_cast<float4*>(image)[q] = make_float4(y[0], y[1], y[2], y[3]);
        else {
            float* p = image + (size_t)q * g.C;
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < g.C) p[c] = y[c];
        }
        if (mask_out) mask_out[q] = mk;
    }
}

// ------------------------------------------------------------------------------------------------ restore
struct Lut { uint32_t w[64]; };
struct RGeo {
    int X, Y, Z, Xt, Yt, Zt;
    FastDiv dZ, dY, dX;
};

// The native voxels of one axis that show a target voxel: [lo, hi), and the shift from native to target coordinate.  `place` is
// data - any int32 -, so the intersection of [n, n + e), [n - t, n - t + T) and [0, dim) is formed in 64 bits; it is the same for
// every thread (scalar arithmetic).  For lo <= v < hi the 32-bit v + sh is exact: it lies in [0, T).
struct Clip { int lo, hi, sh; };
__device__ __forceinline__ Clip clip_axis(int n, int t, int e, int T, int dim) {
    const long long lo = max(max((long long)n, (long long)n - t), 0LL), hi = min(min((long long)n + e, (long long)n - t + T), (long long)dim);
    Clip c;
    c.lo = hi > lo ? (int)lo : 0;
    c.hi = hi > lo ? (int)hi : 0;
    c.sh = (int)((unsigned)t - (unsigned)n);
    return c;
}

// W elements a thread: thread u < total / W writes the elements W u .. W u + W - 1 with one store (4 or 16 bytes); the total % W
// elements behind them go one per thread.  The source row of a voxel is found once per (n, x, y) and kept while z runs.
template <typename T, int W>
__global__ __launch_bounds__(TB) void restore_k(const T* __restrict__ rows, const int* __restrict__ place, Lut lut, int has_lut, T fill,
                                                T* __restrict__ out, RGeo g, unsigned total) {
    __shared__ uint32_t slut[64];
    const uint8_t* lp = nullptr;
    if constexpr (sizeof(T) == 1) {
        if (has_lut) {
            if (threadIdx.x < 64) slut[threadIdx.x] = lut.w[threadIdx.x];
            __syncthreads();
            lp = reinterpret_cast<const uint8_t*>(slut);
        }
    }
    const Clip cx = clip_axis(place[0], place[3], place[6], g.Xt, g.X), cy = clip_axis(place[1], place[4], place[7], g.Yt, g.Y),
               cz = clip_axis(place[2], place[5], place[8], g.Zt, g.Z);
    const unsigned u = blockIdx.x * TB + threadIdx.x;
    const unsigned units = W > 1 ? total / W : 0;
    unsigned o;
    int cnt;
    if (W > 1 && u < units) { o = W * u; cnt = W; }
    else { o = W * units + (u - units); cnt = 1; if (o >= total) return; }
    const unsigned r = fdiv(o, g.dZ), r2 = fdiv(r, g.dY), n0 = fdiv(r2, g.dX);
    int n = (int)n0, x = (int)(r2 - n0 * (unsigned)g.X), y = (int)(r - r2 * (unsigned)g.Y), z = (int)(o - r * (unsigned)g.Z);
    bool row_ok;
    size_t base;
    auto find_row = [&]() {
        row_ok = x >= cx.lo && x < cx.hi && y >= cy.lo && y < cy.hi;
        base = row_ok ? (((size_t)n * g.Xt + (size_t)(x + cx.sh)) * g.Yt + (size_t)(y + cy.sh)) * g.Zt : 0;
    };
    auto fetch = [&]() -> T {
        if (!row_ok || z < cz.lo || z >= cz.hi) return fill;
        const T v = rows[base + (size_t)(z + cz.sh)];
        if constexpr (sizeof(T) == 1) return lp ? lp[v] : v;
        else return v;
    };
    find_row();
    if (cnt == 1) { out[o] = fetch(); return; }
    if constexpr (W > 1) {
    T v[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        v[k] = fetch();
        if (++z == g.Z) {
            z = 0;
            if (++y == g.Y) { y = 0; if (++x == g.X) { x = 0; ++n; } }
            find_row();
        }
    }
    if constexpr (sizeof(T) == 1) {
        uint32_t w[W / 4];
#pragma unroll
        for (int k = 0; k < W / 4; ++k) w[k] = (uint32_t)v[4 * k] | ((uint32_t)v[4 * k + 1] << 8) | ((uint32_t)v[4 * k + 2] << 16) | ((uint32_t)v[4 * k + 3] << 24);
        if constexpr (W == 16) *reinterpret_cast<uint4*>(out + o) = make_uint4(w[0], w[1], w[2], w[3]);
        else *reinterpret_cast<uint32_t*>(out + o) = w[0];
    } else {
        *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
    }
    }
}

// ------------------------------------------------------------------------------------------------ host
const char* prep_sizes_bad(int C, int X, int Y, int Z, int Xt, int Yt, int Zt) {
    if (C < 1 || C > MAXC) return "1 <= C <= 8 channels";
    if (X < 1 || Y < 1 || Z < 1 || Xt < 1 || Yt < 1 || Zt < 1) return "empty axis";
    const long long lim = 1LL << 31, a = (long long)X * Y, b = (long long)Xt * Yt;            // the products in steps, each below 2^31 * 2^31
    if (a >= lim || a * Z >= lim || a * Z * C >= lim) return "X*Y*Z*C must stay below 2^31";
    if (b >= lim || b * Zt >= lim || b * Zt * C >= lim) return "Xt*Yt*Zt*C must stay below 2^31";
    return nullptr;
}
inline int sweep_wg(long long P) { return uz::sweep_grid(P, TB); }                                // workgroups that would cover P in one sweep
inline int pass_grid(long long P) { return uz::sweep_grid(P, TB, CAP); }
inline bool prep_wide(int C, uintptr_t raw, uintptr_t image) { return C == 4 && raw % 16 == 0 && image % 16 == 0; }
inline Geo make_geo(int C, int X, int Y, int Z, int Xt, int Yt, int Zt) {
    Geo g;
    g.C = C; g.X = X; g.Y = Y; g.Z = Z; g.Xt = Xt; g.Yt = Yt; g.Zt = Zt;
    g.dZ = make_div(Z); g.dY = make_div(Y); g.dZt = make_div(Zt); g.dYt = make_div(Yt);
    return g;
}

template <bool WIDE>
int launch_prepare(const float* raw, const uint8_t* mask, const Geo& g, int placement, void* workspace, float* image, uint8_t* mask_out,
                   int32_t* info, double* stats, hipStream_t st) {
    const unsigned P = (unsigned)g.X * g.Y * g.Z, Pt = (unsigned)g.Xt * g.Yt * g.Zt;
    const int Gb = pass_grid(P), Gt = pass_grid(Pt);
    int* bsl = static_cast<int*>(workspace);
    SumSlice* ssl = reinterpret_cast<SumSlice*>(static_cast<char*>(workspace) + uz::up16((size_t)Gb * BSL * sizeof(int)));
    hipLaunchKernelGGL(prep_bounds_k<WIDE>, dim3(Gb), dim3(TB), 0, st, raw, g, P, bsl);
    if (int rc = uz::check_launch("prep_bounds_k")) return rc;
    hipLaunchKernelGGL(prep_fold_bounds_k, dim3(1), dim3(TB), 0, st, bsl, Gb, g.X, g.Y, g.Z, g.Xt, g.Yt, g.Zt, placement, info);
    if (int rc = uz::check_launch("prep_fold_bounds_k")) return rc;
    hipLaunchKernelGGL((prep_sums_k<WIDE, false>), dim3(Gt), dim3(TB), 0, st, raw, g, Pt, info, stats, ssl);
    if (int rc = uz::check_launch("prep_sums_k")) return rc;
    hipLaunchKernelGGL(prep_fold_stats_k, dim3(g.C), dim3(TB), 0, st, ssl, Gt, 0, stats);
    if (int rc = uz::check_launch("prep_fold_stats_k")) return rc;
    hipLaunchKernelGGL((prep_sums_k<WIDE, true>), dim3(Gt), dim3(TB), 0, st, raw, g, Pt, info, stats, ssl);
    if (int rc = uz::check_launch("prep_sums_k (squares)")) return rc;
    hipLaunchKernelGGL(prep_fold_stats_k, dim3(g.C), dim3(TB), 0, st, ssl, Gt, 1, stats);
    if (int rc = uz::check_launch("prep_fold_stats_k (squares)")) return rc;
    hipLaunchKernelGGL(prep_store_k<WIDE>, dim3(Gt), dim3(TB), 0, st, raw, mask, g, Pt, info, stats, image, mask_out);
    return uz::check_launch("prep_store_k");
}

const char* restore_sizes_bad(int elem, int N, int Xt, int Yt, int Zt, int X, int Y, int Z) {
    if (elem != 1 && elem != 4) return "elem is 1 (uint8) or 4 (fp32)";
    if (N < 1 || X < 1 || Y < 1 || Z < 1 || Xt < 1 || Yt < 1 || Zt < 1) return "empty axis";
    const long long lim = 1LL << 31, a = (long long)X * Y, b = (long long)Xt * Yt;
    if (a >= lim || a * Z >= lim || a * Z * N >= lim) return "N*X*Y*Z must stay below 2^31";
    if (b >= lim || b * Zt >= lim || b * Zt * N >= lim) return "N*Xt*Yt*Zt must stay below 2^31";
    return nullptr;
}
// elements a thread: uint8 16 or 4, fp32 4, where `out` is aligned for the one store; else 1
inline int restore_width(int elem, uintptr_t out, long long total) {
    if (elem == 1) return total >= 16 && out % 16 == 0 ? 16 : total >= 4 && out % 4 == 0 ? 4 : 1;
    return total >= 4 && out % 16 == 0 ? 4 : 1;
}
inline long long restore_threads(int w, long long total) { return total / w + total % w; }

template <typename T, int W>
int launch_restore(const void* rows, const int32_t* place, const Lut& lut, int has_lut, T fill, void* out, const RGeo& g, unsigned total, hipStream_t st) {
    const int G = sweep_wg(restore_threads(W, total));
    hipLaunchKernelGGL((restore_k<T, W>), dim3(G), dim3(TB), 0, st, static_cast<const T*>(rows), place, lut, has_lut, fill, static_cast<T*>(out), g, total);
    return uz::check_launch("restore_k");
}

}  // namespace

extern "C" size_t uz_vol_prepare_workspace(int C, int X, int Y, int Z, int Xt, int Yt, int Zt) {
    if (prep_sizes_bad(C, X, Y, Z, Xt, Yt, Zt)) return 0;
    return uz::up16((size_t)pass_grid((long long)X * Y * Z) * BSL * sizeof(int)) + (size_t)pass_grid((long long)Xt * Yt * Zt) * sizeof(SumSlice);
}

extern "C" int uz_vol_prepare_route(int C, int X, int Y, int Z, int Xt, int Yt, int Zt, int align, int* out3) {
    UZ_REQUIRE(out3, "vol_prepare_route: three ints to answer into");
    const char* bad = prep_sizes_bad(C, X, Y, Z, Xt, Yt, Zt);
    UZ_REQUIRE(!bad, "vol_prepare_route: %s", bad);
    UZ_REQUIRE(align == 4 || align == 8 || align == 16, "vol_prepare_route: align is 4, 8 or 16");
    const long long P = std::max((long long)X * Y * Z, (long long)Xt * Yt * Zt);
    out3[0] = prep_wide(C, (uintptr_t)align, (uintptr_t)align) ? 1 : 0;
    out3[1] = pass_grid(P);
    out3[2] = sweep_wg(P) > CAP ? 1 : 0;
    return 0;
}

extern "C" int uz_vol_prepare(const float* raw, const uint8_t* mask, int C, int X, int Y, int Z, int Xt, int Yt, int Zt, int placement,
                              void* workspace, float* image, uint8_t* mask_out, int32_t* info, double* stats, void* stream) {
    UZ_REQUIRE(raw && workspace && image && info && stats, "vol_prepare: null argument (raw, workspace, image, info, stats)");
    UZ_REQUIRE((mask == nullptr) == (mask_out == nullptr), "vol_prepare: mask and mask_out go together, both or neither");
    const char* bad = prep_sizes_bad(C, X, Y, Z, Xt, Yt, Zt);
    UZ_REQUIRE(!bad, "vol_prepare: %s", bad);
    UZ_REQUIRE(placement == 0 || placement == 1, "vol_prepare: placement is 0 (centre) or 1 (corner)");
    UZ_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "vol_prepare: workspace must be 16-byte aligned");
    UZ_REQUIRE(reinterpret_cast<uintptr_t>(info) % 4 == 0, "vol_prepare: info must be 4-byte aligned");
    UZ_REQUIRE(reinterpret_cast<uintptr_t>(stats) % 8 == 0, "vol_prepare: stats must be 8-byte aligned");
    const Geo g = make_geo(C, X, Y, Z, Xt, Yt, Zt);
    hipStream_t st = uz::S(stream);
    return prep_wide(C, reinterpret_cast<uintptr_t>(raw), reinterpret_cast<uintptr_t>(image))
               ? launch_prepare<true>(raw, mask, g, placement, workspace, image, mask_out, info, stats, st)
               : launch_prepare<false>(raw, mask, g, placement, workspace, image, mask_out, info, stats, st);
}

extern "C" int uz_vol_restore_route(int elem, int N, int X, int Y, int Z, int align, int* out3) {
    UZ_REQUIRE(out3, "vol_restore_route: three ints to answer into");
    const char* bad = restore_sizes_bad(elem, N, 1, 1, 1, X, Y, Z);
    UZ_REQUIRE(!bad, "vol_restore_route: %s", bad);
    UZ_REQUIRE(align == 1 || align == 2 || align == 4 || align == 8 || align == 16, "vol_restore_route: align is 1, 2, 4, 8 or 16");
    UZ_REQUIRE(elem == 1 || align >= 4, "vol_restore_route: fp32 elements are 4-byte aligned at the least");
    const long long total = (long long)N * X * Y * Z;
    const int w = restore_width(elem, (uintptr_t)align, total);
    out3[0] = w;
    out3[1] = sweep_wg(restore_threads(w, total));
    out3[2] = 0;                                                            // one sweep, always
    return 0;
}

extern "C" int uz_vol_restore(const void* rows, int elem, int N, int Xt, int Yt, int Zt, const int32_t* place, const uint8_t* lut,
                              const void* fill, void* out, int X, int Y, int Z, void* stream) {
    UZ_REQUIRE(rows && place && fill && out, "vol_restore: null argument (rows, place, fill, out)");
    const char* bad = restore_sizes_bad(elem, N, Xt, Yt, Zt, X, Y, Z);
    UZ_REQUIRE(!bad, "vol_restore: %s", bad);
    UZ_REQUIRE(!(lut && elem == 4), "vol_restore: the lut maps uint8 rows only, not fp32");
    const uintptr_t r0 = reinterpret_cast<uintptr_t>(rows), o0 = reinterpret_cast<uintptr_t>(out);
    UZ_REQUIRE(elem == 1 || ((r0 | o0) & 3) == 0, "vol_restore: fp32 rows and out must be 4-byte aligned");
    UZ_REQUIRE((reinterpret_cast<uintptr_t>(place) & 3) == 0, "vol_restore: place must be 4-byte aligned");
    const size_t total = (size_t)N * X * Y * Z, rbytes = (size_t)N * Xt * Yt * Zt * elem, obytes = total * elem;
    UZ_REQUIRE(r0 + rbytes <= o0 || o0 + obytes <= r0, "vol_restore: out may not overlap rows");
    RGeo g;
    g.X = X; g.Y = Y; g.Z = Z; g.Xt = Xt; g.Yt = Yt; g.Zt = Zt;
    g.dZ = make_div(Z); g.dY = make_div(Y); g.dX = make_div(X);
    Lut l = {};
    if (lut) {
        for (int k = 0; k < 256; ++k) l.w[k >> 2] |= (uint32_t)lut[k] << (8 * (k & 3));
    }
    hipStream_t st = uz::S(stream);
    const int w = restore_width(elem, o0, (long long)total);
    if (elem == 1) {
        const uint8_t f = *static_cast<const uint8_t*>(fill);
        const int hl = lut ? 1 : 0;
        return w == 16 ? launch_restore<uint8_t, 16>(rows, place, l, hl, f, out, g, (unsigned)total, st)
             : w == 4  ? launch_restore<uint8_t, 4>(rows, place, l, hl, f, out, g, (unsigned)total, st)
                       : launch_restore<uint8_t, 1>(rows, place, l, hl, f, out, g, (unsigned)total, st);
    }
    float f;
    memcpy(&f, fill, sizeof f);
    return w == 4 ? launch_restore<float, 4>(rows, place, l, 0, f, out, g, (unsigned)total, st)
                  : launch_restore<float, 1>(rows, place, l, 0, f, out, g, (unsigned)total, st);
}
