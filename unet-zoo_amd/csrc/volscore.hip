// BraTS region scores of label volumes on the device (uz_api.h "volume scores"): an exact squared Euclidean distance transform in three
// separable integer passes, and Dice / sensitivity / specificity / HD95 of N label volumes against one reference for R regions given
// as sets of label values.  Replaces data/bratsUtils.py:6-24,57-84 (dice, sensitivity, specificity, getHd95 with MedPy 0.4.0's
// __surface_distances: binary_erosion, distance_transform_edt and a gather per direction, per region, per sample, on the host).
//
// Transform of a seed volume (D, H, W), W fastest:
//   W pass  one wave per row: the nearest seed to the left by a max-scan over the lanes, to the right by a min-scan, g = min(.)^2 or INF;
//   H, D    out[i] = min_j (g[j] + (i - j)^2) by direct evaluation: a tile of 64 neighbouring columns x up to 128 positions of the axis
//           lives in LDS (lane = the contiguous index, so every global access is a 256-byte row), each wave keeps eight outputs in
//           registers per LDS read.  An axis longer than 128 is walked in chunks of 128 j, the running minimum kept in the output.
// Everything is unsigned integer arithmetic: g <= INF = 2^30 and (i - j)^2 < 2^30 (D^2 + H^2 + W^2 <= 2^30), so no sum reaches 2^32, and
// each pass clamps what it stores to INF, so the sentinel never grows; the last pass turns INF into INT32_MAX.
#include "uz_common.h"
#include <limits.h>
#include <algorithm>

namespace {

constexpr unsigned INF = 1u << 30;
constexpr int TW = 64;            // columns of one LDS tile = lanes of a wave
constexpr int CH = 128;           // axis positions of one LDS tile (32 KB: five workgroups per CU hide the LDS reads)
constexpr int IB = 8;             // outputs a thread keeps per LDS read
constexpr int LB = 1024;          // bins of the histogram's per-workgroup LDS part
constexpr int WALK_T = 1024;      // threads of the prefix walk, four bins each
constexpr int WALK_BINS = WALK_T * 4;
constexpr long long EDT_MAX_SQ = 1LL << 30;
constexpr long long HD_MAX_SQ = UZ_VOL_HD95_MAX_SQ;

__device__ __forceinline__ bool member(const uint8_t* __restrict__ lab, size_t idx, uint32_t set) { return uz::in_set(lab[idx], set); }
// border of the mask {label in set}: a voxel of the mask with a face neighbour outside the mask or outside the volume
// (scipy.ndimage.binary_erosion, connectivity 1, border_value 0: mask ^ erosion)
__device__ __forceinline__ bool border_at(const uint8_t* __restrict__ lab, uint32_t set, int d, int h, int w, int D, int H, int W) {
    const size_t hw = (size_t)H * W, idx = (size_t)d * hw + (size_t)h * W + w;
    if (!member(lab, idx, set)) return false;
    if (d == 0 || d == D - 1 || h == 0 || h == H - 1 || w == 0 || w == W - 1) return true;
    return !(member(lab, idx - hw, set) && member(lab, idx + hw, set) && member(lab, idx - W, set) && member(lab, idx + W, set) &&
             member(lab, idx - 1, set) && member(lab, idx + 1, set));
}

// ------------------------------------------------------------------------------------------------ W pass
// BORDER: the seeds are the border of {src in set}; else src != 0.  The left scan parks the index of the nearest seed at or before i
// (-1: none) in dst, the right scan reads it back (the same lane wrote it) and knows a seed by L == i.
template <bool BORDER>
__global__ __launch_bounds__(256) void edt_w_k(const uint8_t* __restrict__ src, uint32_t set, int D, int H, int W, int* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int rows = D * H, nchunk = (W + 63) >> 6;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4) {
        const int d = row / H, h = row - d * H;
        const size_t base = (size_t)row * W;
        int carry = -1;
        for (int c = 0; c < nchunk; ++c) {
            const int i = (c << 6) + lane;
            bool seed = false;
            if (i < W) seed = BORDER ? border_at(src, set, d, h, i, D, H, W) : src[base + i] != 0;
            int v = seed ? i : -1;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if (lane >= o) v = max(v, u); }
            v = max(v, carry);
            carry = __shfl(v, 63, 64);
            if (i < W) dst[base + i] = v;
        }
        carry = INT_MAX;
        for (int c = nchunk - 1; c >= 0; --c) {
            const int i = (c << 6) + lane;
            const int L = i < W ? dst[base + i] : -1;
            int v = (i < W && L == i) ? i : INT_MAX;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_down(v, o, 64); if (lane + o < 64) v = min(v, u); }
            v = min(v, carry);
            carry = __shfl(v, 0, 64);
            if (i < W) {
                const unsigned dl = L < 0 ? INF : (unsigned)(i - L), dr = v == INT_MAX ? INF : (unsigned)(v - i);
                const unsigned m = min(dl, dr);                                     // < 2^15 when there is a seed in the row
                dst[base + i] = (int)(m >= INF ? INF : m * m);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ H and D passes
// The volume as (outer, L, inner): workgroup = one tile of 64 inner indices of one outer index, the whole axis.  src != dst.
__global__ __launch_bounds__(256) void edt_axis_k(const int* __restrict__ src, int* __restrict__ dst, int L, int inner, int tiles, int fin) {
    extern __shared__ unsigned g[];                                    // [min(L, CH)][TW]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = blockIdx.x / tiles, t = blockIdx.x - o * tiles;
    const int col = t * TW + lane;
    const bool live = col < inner;
    const size_t base = (size_t)o * L * inner + col;
    for (int j0 = 0; j0 < L; j0 += CH) {
        const int nj = min(CH, L - j0);
        if (j0) __syncthreads();
        for (int j = wv; j < nj; j += 4) g[j * TW + lane] = live ? (unsigned)src[base + (size_t)(j0 + j) * inner] : INF;
        __syncthreads();
        const bool first = j0 == 0, last = j0 + CH >= L;
        for (int i0 = wv * IB; i0 < L; i0 += 4 * IB) {
            unsigned m[IB];
            int dd[IB];
#pragma unroll
            for (int b = 0; b < IB; ++b) { m[b] = 0xffffffffu; dd[b] = i0 + b - j0; }
#pragma unroll 4
            for (int j = 0; j < nj; ++j) {
                const unsigned v = g[j * TW + lane];
#pragma unroll
                for (int b = 0; b < IB; ++b) { m[b] = min(m[b], (unsigned)__mul24(dd[b], dd[b]) + v); dd[b] -= 1; }
            }
#pragma unroll
            for (int b = 0; b < IB; ++b) {
                const int i = i0 + b;
                if (i < L && live) {
                    const size_t a = base + (size_t)i * inner;
                    unsigned r = m[b];
                    if (!first) r = min(r, (unsigned)dst[a]);
                    if (last) r = r >= INF ? (fin ? (unsigned)INT_MAX : INF) : r;
                    dst[a] = (int)r;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ counts
// counts[n][r] = {tp, |pred|, |ref|, .}: per-thread integer counters, wave sums, one LDS sum per workgroup, then integer atomics.
__device__ __forceinline__ void count_voxel(unsigned a, unsigned b, const uz::RegionSets& s, unsigned (&tp)[UZ_VOL_MAX_REGIONS],
                                            unsigned (&cp)[UZ_VOL_MAX_REGIONS], unsigned (&cr)[UZ_VOL_MAX_REGIONS]) {
    const uint32_t ma = a < 32u ? 1u << a : 0u, mb = b < 32u ? 1u << b : 0u;
#pragma unroll
    for (int r = 0; r < UZ_VOL_MAX_REGIONS; ++r) {                      // sets beyond R are empty
        const unsigned ip = (s.p[r] & ma) != 0u, ir = (s.r[r] & mb) != 0u;
        tp[r] += ip & ir; cp[r] += ip; cr[r] += ir;
    }
}
__global__ __launch_bounds__(256) void count_k(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ ref, uz::RegionSets s, int R, int P, int vec,
                                               unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long acc[3 * UZ_VOL_MAX_REGIONS];
    const int n = blockIdx.y;
    const uint8_t* p = pred + (size_t)n * P;
    unsigned tp[UZ_VOL_MAX_REGIONS] = {}, cp[UZ_VOL_MAX_REGIONS] = {}, cr[UZ_VOL_MAX_REGIONS] = {};
    if (threadIdx.x < 3 * UZ_VOL_MAX_REGIONS) acc[threadIdx.x] = 0ull;
    __syncthreads();
    if (vec) {
        const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p);
        const uint32_t* r4 = reinterpret_cast<const uint32_t*>(ref);
        for (int q = blockIdx.x * 256 + threadIdx.x; q < (P >> 2); q += gridDim.x * 256) {
            const uint32_t a = p4[q], b = r4[q];
#pragma unroll
            for (int k = 0; k < 4; ++k) count_voxel((a >> (8 * k)) & 255u, (b >> (8 * k)) & 255u, s, tp, cp, cr);
        }
    } else {
        for (int q = blockIdx.x * 256 + threadIdx.x; q < P; q += gridDim.x * 256) count_voxel(p[q], ref[q], s, tp, cp, cr);
    }
#pragma unroll
    for (int r = 0; r < UZ_VOL_MAX_REGIONS; ++r) {
        const unsigned a = uz::wave_sum(tp[r]), b = uz::wave_sum(cp[r]), c = uz::wave_sum(cr[r]);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&acc[3 * r], (unsigned long long)a); atomicAdd(&acc[3 * r + 1], (unsigned long long)b); atomicAdd(&acc[3 * r + 2], (unsigned long long)c);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * R) {
        const int r = threadIdx.x / 3, k = threadIdx.x - 3 * r;
        atomicAdd(&counts[((size_t)n * R + r) * 4 + k], acc[threadIdx.x]);
    }
}

// scores from the integer counts, one fp64 division each (bratsUtils.py:15,19-21,57-72)
__global__ void finish_k(long long* __restrict__ counts, double* __restrict__ scores, int NR, int P, int want_hd95) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= NR) return;
    const long long tp = counts[4 * q], cp = counts[4 * q + 1], cr = counts[4 * q + 2];
    counts[4 * q + 3] = P;
    scores[4 * q] = cp + cr == 0 ? 1.0 : (double)(2 * tp) / (double)(cp + cr);
    scores[4 * q + 1] = cr == 0 ? 1.0 : (double)tp / (double)cr;
    scores[4 * q + 2] = (double)(P - cp - cr + tp) / (double)(P - cr);           // 0 / 0 = NaN when the reference region is the whole volume
    if (!want_hd95) scores[4 * q + 3] = __longlong_as_double(0x7ff8000000000000ll);
}

// ------------------------------------------------------------------------------------------------ HD95
// Both directions of one (row, region) in one launch: blockIdx.y = 0 the pred border against the reference border's transform, 1 the
// reference border against the pred border's.  Squared distances below LB are counted in LDS first (the hot bins of overlapping masks),
// the others straight in the global histogram; integer atomics only, so the result does not depend on the order.
__global__ __launch_bounds__(256) void gather_k(const uint8_t* __restrict__ pred, uint32_t pset, const int* __restrict__ t_ref,
                                                const uint8_t* __restrict__ ref, uint32_t rset, const int* __restrict__ t_pred,
                                                int D, int H, int W, int nbins, unsigned* __restrict__ hist) {
    __shared__ unsigned lh[LB];
    for (int k = threadIdx.x; k < LB; k += 256) lh[k] = 0u;
    __syncthreads();
    const uint8_t* lab = blockIdx.y ? ref : pred;
    const uint32_t set = blockIdx.y ? rset : pset;
    const int* t = blockIdx.y ? t_pred : t_ref;
    const int P = D * H * W, HW = H * W;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < P; q += gridDim.x * 256) {
        const int d = q / HW, rem = q - d * HW, h = rem / W, w = rem - h * W;
        if (border_at(lab, set, d, h, w, D, H, W)) {
            const int v = t[q];
            if (v < LB) atomicAdd(&lh[v], 1u);
            else if (v < nbins) atomicAdd(&hist[v], 1u);                  // INT32_MAX (the other mask is empty) is no distance
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < LB && k < nbins; k += 256)
        if (lh[k]) atomicAdd(&hist[k], lh[k]);
}

__device__ __forceinline__ unsigned long long block_excl_scan(unsigned long long v, unsigned long long* wsum, unsigned long long& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
    __syncthreads();
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned long long before = 0ull, all = 0ull;
    for (int k = 0; k < WALK_T / 64; ++k) { const unsigned long long s = wsum[k]; if (k < wv) before += s; all += s; }
    total = all;
    return before + inc - v;
}
// numpy.percentile(., 95), linear rule, of the multiset the histogram holds: n from the bins, the two order statistics by a prefix
// walk (exact: the bins are the integer squared distances), then one interpolation in fp64.  Leaves the histogram zeroed for the next pair.
__global__ __launch_bounds__(WALK_T) void walk_k(unsigned* __restrict__ hist, int nbins_pad, const long long* __restrict__ cnt, double* __restrict__ out) {
    __shared__ unsigned long long wsum[WALK_T / 64];
    __shared__ unsigned long long tot;
    __shared__ int res[2];
    if (cnt[1] == 0 || cnt[2] == 0) {                                    // an empty mask: nothing was counted (bratsUtils.py:82-84)
        if (threadIdx.x == 0) *out = -1.0;
        return;
    }
    if (threadIdx.x == 0) { tot = 0ull; res[0] = res[1] = 0; }
    __syncthreads();
    uint4* h4 = reinterpret_cast<uint4*>(hist);
    unsigned long long mine = 0ull;
    for (int q = threadIdx.x; q < nbins_pad / 4; q += WALK_T) { const uint4 c = h4[q]; mine += (unsigned long long)c.x + c.y + c.z + c.w; }
    mine = uz::wave_sum(mine);
    if ((threadIdx.x & 63) == 0) atomicAdd(&tot, mine);
    __syncthreads();
    const unsigned long long n = tot;
    const double hq = 0.95 * (double)(n - 1);
    const unsigned long long k0 = (unsigned long long)floor(hq), k1 = k0 + 1 < n ? k0 + 1 : n - 1;
    unsigned long long base = 0ull;
    for (int q0 = 0; q0 < nbins_pad / 4; q0 += WALK_T) {
        const int q = q0 + threadIdx.x;
        const uint4 c = h4[q];
        h4[q] = make_uint4(0u, 0u, 0u, 0u);
        unsigned long long all;
        unsigned long long p = base + block_excl_scan((unsigned long long)c.x + c.y + c.z + c.w, wsum, all);
        const unsigned cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (p <= k0 && k0 < p + cc[k]) res[0] = 4 * q + k;
            if (p <= k1 && k1 < p + cc[k]) res[1] = 4 * q + k;
            p += cc[k];
        }
        base += all;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double lo = sqrt((double)res[0]), hi = sqrt((double)res[1]);
        *out = lo + (hq - (double)k0) * (hi - lo);
    }
}

// ------------------------------------------------------------------------------------------------ host
const char* sizes_bad(int D, int H, int W, long long max_sq) {
    if (D < 1 || H < 1 || W < 1) return "empty axis";
    if ((long long)D * H * W >= (1LL << 31)) return "D*H*W must stay below 2^31";
    if ((long long)D * D + (long long)H * H + (long long)W * W > max_sq)
        return max_sq == EDT_MAX_SQ ? "D^2 + H^2 + W^2 beyond 2^30" : "D^2 + H^2 + W^2 beyond 2^22 (the HD95 histogram)";
    return nullptr;
}
inline int w_grid(int D, int H) { return uz::sweep_grid((long long)D * H, 4, 65536); }
inline int axis_form(int L) { return L > CH ? 1 : 0; }                  // 0 the whole axis in one LDS tile, 1 chunks of CH
inline int axis_grid(long long outer, long long inner) { return (int)(outer * ((inner + TW - 1) / TW)); }
inline int count_grid(int P, bool vec) { return uz::sweep_grid(vec ? P / 4 : P, 256, 256); }
inline int gather_grid(int P) { return uz::sweep_grid(P, 256, 2048); }
inline bool count_vec(int P, const void* a, const void* b) { return P % 4 == 0 && (reinterpret_cast<uintptr_t>(a) & 3) == 0 && (reinterpret_cast<uintptr_t>(b) & 3) == 0; }
inline int hist_bins(int D, int H, int W) { return (D - 1) * (D - 1) + (H - 1) * (H - 1) + (W - 1) * (W - 1) + 1; }
inline int hist_bins_pad(int D, int H, int W) { return uz::ceil_div(hist_bins(D, H, W), WALK_BINS) * WALK_BINS; }

int launch_axis(const int* src, int* dst, long long outer, int L, long long inner, int fin, hipStream_t st) {
    const int tiles = (int)((inner + TW - 1) / TW);
    hipLaunchKernelGGL(edt_axis_k, dim3(axis_grid(outer, inner)), dim3(256), (size_t)std::min(L, CH) * TW * 4, st, src, dst, L, (int)inner, tiles, fin);
    return uz::check_launch("edt_axis_k");
}
// src -> d2 through tmp: W pass into d2, H pass d2 -> tmp, D pass tmp -> d2
int transform(const uint8_t* src, bool border, uint32_t set, int D, int H, int W, int* d2, int* tmp, hipStream_t st) {
    if (border) hipLaunchKernelGGL(edt_w_k<true>, dim3(w_grid(D, H)), dim3(256), 0, st, src, set, D, H, W, d2);
    else hipLaunchKernelGGL(edt_w_k<false>, dim3(w_grid(D, H)), dim3(256), 0, st, src, set, D, H, W, d2);
    if (int rc = uz::check_launch("edt_w_k")) return rc;
    if (int rc = launch_axis(d2, tmp, D, H, W, 0, st)) return rc;
    return launch_axis(tmp, d2, 1, D, (long long)H * W, 1, st);
}

}  // namespace

extern "C" size_t uz_vol_edt_sq_workspace(int D, int H, int W) {
    if (sizes_bad(D, H, W, EDT_MAX_SQ)) return 0;
    return uz::up16((size_t)D * H * W * 4);
}

extern "C" int uz_vol_edt_sq(const uint8_t* seeds, int D, int H, int W, int32_t* d2, void* workspace, void* stream) {
    UZ_REQUIRE(seeds && d2 && workspace, "vol_edt_sq: null argument (seeds, d2, workspace)");
    const char* bad = sizes_bad(D, H, W, EDT_MAX_SQ);
    UZ_REQUIRE(!bad, "vol_edt_sq: %s", bad);
    UZ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0 && (reinterpret_cast<uintptr_t>(d2) & 3) == 0, "vol_edt_sq: d2 and workspace must be 4-byte aligned");
    return transform(seeds, false, 0u, D, H, W, d2, static_cast<int*>(workspace), uz::S(stream));
}

extern "C" size_t uz_vol_region_scores_workspace(int N, int R, int D, int H, int W, int want_hd95) {
    if (N < 1 || N > UZ_VOL_MAX_ROWS || R < 1 || R > UZ_VOL_MAX_REGIONS || sizes_bad(D, H, W, want_hd95 ? HD_MAX_SQ : EDT_MAX_SQ)) return 0;
    if (!want_hd95) return 16;
    return 3 * uz::up16((size_t)D * H * W * 4) + (size_t)hist_bins_pad(D, H, W) * 4;
}

extern "C" int uz_vol_region_scores_route(int N, int R, int D, int H, int W, int want_hd95, int* out4) {
    UZ_REQUIRE(out4, "vol_region_scores_route: four ints to answer into");
    UZ_REQUIRE(N >= 1 && N <= UZ_VOL_MAX_ROWS, "vol_region_scores_route: 1 <= N <= %d", UZ_VOL_MAX_ROWS);
    UZ_REQUIRE(R >= 1 && R <= UZ_VOL_MAX_REGIONS, "vol_region_scores_route: 1 <= R <= %d", UZ_VOL_MAX_REGIONS);
    const char* bad = sizes_bad(D, H, W, want_hd95 ? HD_MAX_SQ : EDT_MAX_SQ);
    UZ_REQUIRE(!bad, "vol_region_scores_route: %s", bad);
    const int P = D * H * W;
    long long widest = (long long)count_grid(P, P % 4 == 0) * N;
    if (want_hd95) {
        widest = std::max<long long>(widest, w_grid(D, H));
        widest = std::max<long long>(widest, axis_grid(D, W));
        widest = std::max<long long>(widest, axis_grid(1, (long long)H * W));
        widest = std::max<long long>(widest, 2LL * gather_grid(P));
    }
    out4[0] = axis_form(H); out4[1] = axis_form(D);
    out4[2] = (int)widest;
    out4[3] = want_hd95 ? R * (N + 1) : 0;
    return 0;
}

extern "C" int uz_vol_region_scores(const uint8_t* pred, int N, const uint32_t* pred_sets, const uint8_t* ref, const uint32_t* ref_sets, int R,
                                    int D, int H, int W, int want_hd95, void* workspace, int64_t* counts, double* scores, void* stream) {
    UZ_REQUIRE(pred && pred_sets && ref && ref_sets && workspace && counts && scores,
               "vol_region_scores: null argument (pred, pred_sets, ref, ref_sets, workspace, counts, scores)");
    UZ_REQUIRE(N >= 1, "vol_region_scores: N >= 1 label volumes");
    UZ_REQUIRE(R >= 1 && R <= UZ_VOL_MAX_REGIONS, "vol_region_scores: 1 <= R <= %d regions", UZ_VOL_MAX_REGIONS);
    const char* bad = sizes_bad(D, H, W, want_hd95 ? HD_MAX_SQ : EDT_MAX_SQ);
    UZ_REQUIRE(!bad, "vol_region_scores: %s", bad);
    UZ_REQUIRE(N <= UZ_VOL_MAX_ROWS, "vol_region_scores: N beyond %d label volumes", UZ_VOL_MAX_ROWS);
    UZ_REQUIRE(uz::align_of(workspace) == 16, "vol_region_scores: workspace must be 16-byte aligned");
    UZ_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0 && (reinterpret_cast<uintptr_t>(scores) & 7) == 0, "vol_region_scores: counts and scores must be 8-byte aligned");
    hipStream_t st = uz::S(stream);
    const int P = D * H * W;
    const uz::RegionSets s = uz::region_sets(pred_sets, ref_sets, R);

    if (hipMemsetAsync(counts, 0, (size_t)N * R * 4 * sizeof(int64_t), st) != hipSuccess) return uz::fail("vol_region_scores: clearing counts failed");
    const bool vec = count_vec(P, pred, ref);
    hipLaunchKernelGGL(count_k, dim3(count_grid(P, vec), N), dim3(256), 0, st, pred, ref, s, R, P, vec ? 1 : 0, reinterpret_cast<unsigned long long*>(counts));
    if (int rc = uz::check_launch("count_k")) return rc;
    hipLaunchKernelGGL(finish_k, dim3(uz::ceil_div(N * R, 256)), dim3(256), 0, st, reinterpret_cast<long long*>(counts), scores, N * R, P, want_hd95);
    if (int rc = uz::check_launch("finish_k")) return rc;
    if (!want_hd95) return 0;

    char* base = static_cast<char*>(workspace);
    const size_t vol = uz::up16((size_t)P * 4);
    int* t_ref = reinterpret_cast<int*>(base);
    int* t_pred = reinterpret_cast<int*>(base + vol);
    int* tmp = reinterpret_cast<int*>(base + 2 * vol);
    unsigned* hist = reinterpret_cast<unsigned*>(base + 3 * vol);
    const int nbins = hist_bins(D, H, W), nbins_pad = hist_bins_pad(D, H, W);
    if (hipMemsetAsync(hist, 0, (size_t)nbins_pad * 4, st) != hipSuccess) return uz::fail("vol_region_scores: clearing the histogram failed");
    for (int r = 0; r < R; ++r) {
        if (int rc = transform(ref, true, s.r[r], D, H, W, t_ref, tmp, st)) return rc;      // once per region, shared by the N rows
        for (int n = 0; n < N; ++n) {
            const uint8_t* p = pred + (size_t)n * P;
            if (int rc = transform(p, true, s.p[r], D, H, W, t_pred, tmp, st)) return rc;
            hipLaunchKernelGGL(gather_k, dim3(gather_grid(P), 2), dim3(256), 0, st, p, s.p[r], t_ref, ref, s.r[r], t_pred, D, H, W, nbins, hist);
            if (int rc = uz::check_launch("gather_k")) return rc;
            const size_t q = (size_t)n * R + r;
            hipLaunchKernelGGL(walk_k, dim3(1), dim3(WALK_T), 0, st, hist, nbins_pad, reinterpret_cast<const long long*>(counts) + 4 * q, scores + 4 * q + 3);
            if (int rc = uz::check_launch("walk_k")) return rc;
        }
    }
    return 0;
}
