// Scoring S prior samples of B images against A annotators on the device (uz_score_samples): GED, NCC and per-label Dice of the
// reference's evaluation loop (train_model.py:186-230) for all B images in five launches, with no host round trip.
//   1 score_planes_k    every label map (S*B samples, B*A annotators, B mean labels) -> K bit planes of ceil(P/64) words: one read
//                       of a map serves all K labels, the word is the wave's ballot of (pixel == k)
//   2 score_pairs_k     one wave per (image, label, pair): popcount(x & y), popcount(x), popcount(y) over two planes -> `counts` in
//                       the layout of uz_label_pair_counts; behind them one wave per (image, annotator, label) -> Dice
//   3 score_ncc_maps_k  the cross-entropy maps of variance_ncc_dist per image (uz::ncc_maps_px, shared with metrics.hip)
//   4 score_ncc_k       their correlations (uz::ncc_sums / uz::ncc_of_sums, shared with metrics.hip)
//   5 score_final_k     one workgroup per image: GED in fp64 from the counts, the mean of the image's NCCs
// Integer counts, no atomics, every output written once by its owner: a repeated call is bit-equal.
#include "uz_common.h"

namespace {

typedef unsigned long long u64;

struct ScoreLayout {          // byte offsets into the workspace; total == 0: sizes refused
    size_t planes = 0, counts = 0, ess = 0, esy = 0, total = 0;
    long long maps = 0, pairs = 0;
    int W64 = 0;
};

ScoreLayout score_layout(int B, int S, int A, int K, int P) {
    ScoreLayout l;
    if (K < 2 || K > 8 || B < 1 || S < 1 || A < 1 || P < 1) return l;
    const long long lim = INT32_MAX, b = B, s = S, a = A, k = K, p = P, w64 = (p + 63) / 64;
    // every factor is an int, so a product of two fits 64 bits; each check keeps the next product inside them
    if (s * b > lim || b * a > lim || s * a > lim || s * s > lim || a * a > lim) return l;
    const long long maps = s * b + b * a + b, pairs = s * a + s * s + a * a;
    if (s * b * p > lim || b * a * p > lim || s * b * p * k > lim || maps * (k * w64) > lim || pairs > lim || b * pairs > lim || b * pairs * k > lim / 3) return l;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    l.maps = maps; l.pairs = pairs; l.W64 = (int)w64;
    l.planes = 0;
    l.counts = up((size_t)(maps * k * w64) * 8);
    l.ess = l.counts + up((size_t)(b * k * pairs * 3) * 4);
    l.esy = l.ess + up((size_t)(b * p) * 4);
    l.total = l.esy + up((size_t)(b * a * p) * 4);
    return l;
}

// planes[(map * K + k) * W64 + w]: bit (q % 64) of word q / 64 = (pixel q of the map == k).  Lanes past P compare 255 (>= K): no bit.
__global__ __launch_bounds__(256) void score_planes_k(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ ann,
                                                       const uint8_t* __restrict__ mean_label, int nS, int nA, int K, int P, int W64,
                                                       u64* __restrict__ planes) {
    const int map = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t* src = map < nS ? labels + (size_t)map * P : map < nS + nA ? ann + (size_t)(map - nS) * P : mean_label + (size_t)(map - nS - nA) * P;
    u64* dst = planes + (size_t)map * K * W64;
    for (int w = blockIdx.y * 4 + wave; w < W64; w += gridDim.y * 4) {
        const long long q = (long long)w * 64 + lane;
        const int v = q < P ? src[q] : 255;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < K) {
                const u64 m = __ballot(v == k);
                if (lane == k) dst[(size_t)k * W64 + w] = m;
            }
        }
    }
}

// One wave per item.  Items 0 .. B*K*NP-1 (NP = S*A + S*S + A*A): item = (b*K + k)*NP + t, t walks [S][A], [S][S], [A][A] row-major
// -> counts[item*3 + 0..2].  Items behind them: d = (b*A + j)*K + k -> dice[d] of mean_label[b] against annotator j.
__global__ __launch_bounds__(256) void score_pairs_k(const u64* __restrict__ planes, int B, int S, int A, int K, int W64, long long NP,
                                                      int* __restrict__ counts, double* __restrict__ dice) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long nG = (long long)B * K * NP, nD = (long long)B * A * K;
    if (g >= nG + nD) return;
    const long long nS = (long long)S * B, nA = (long long)B * A;
    long long mx, my;
    int k;
    if (g < nG) {
        const long long bk = g / NP, t = g % NP, sa = (long long)S * A, ss = (long long)S * S;
        const int b = (int)(bk / K);
        k = (int)(bk % K);
        if (t < sa)           { mx = (t / A) * B + b;                my = nS + (long long)b * A + t % A; }
        else if (t < sa + ss) { mx = ((t - sa) / S) * B + b;         my = ((t - sa) % S) * B + b; }
        else                  { mx = nS + (long long)b * A + (t - sa - ss) / A; my = nS + (long long)b * A + (t - sa - ss) % A; }
    } else {
        const long long d = g - nG;
        k = (int)(d % K);
        const long long bj = d / K;                      // b*A + j
        mx = nS + nA + bj / A;
        my = nS + bj;
    }
    const u64* x = planes + (size_t)(mx * K + k) * W64;
    const u64* y = planes + (size_t)(my * K + k) * W64;
    int inter = 0, ca = 0, cb = 0;
    for (int w = lane; w < W64; w += 64) {
        const u64 xv = x[w], yv = y[w];
        inter += __popcll(xv & yv); ca += __popcll(xv); cb += __popcll(yv);
    }
    inter = uz::wave_sum(inter); ca = uz::wave_sum(ca); cb = uz::wave_sum(cb);
    if (lane != 0) return;
    if (g < nG) {
        int* out = counts + g * 3;
        out[0] = inter; out[1] = ca; out[2] = cb;
    } else {
        dice[g - nG] = (ca == 0 && cb == 0) ? 1.0 : (ca == 0 || cb == 0) ? 0.0 : 2.0 * inter / (double)(ca + cb);
    }
}

__global__ __launch_bounds__(256) void score_ncc_maps_k(const float* __restrict__ soft, const uint8_t* __restrict__ ann, int B, int S, int A, int K,
                                                         int P, int nb, float* __restrict__ Ess, float* __restrict__ Esy) {
    const int b = blockIdx.x / nb, q = (blockIdx.x % nb) * 256 + threadIdx.x;
    if (q >= P) return;
    uz::ncc_maps_px(soft + (size_t)b * K * P, B * K, S, A, K, P, q, ann + (size_t)b * A * P, Ess + (size_t)b * P, Esy + (size_t)b * A * P);
}

__global__ __launch_bounds__(256) void score_ncc_k(const float* __restrict__ Ess, const float* __restrict__ Esy, int A, int P, float* __restrict__ out) {
    __shared__ double sm[4 * 5];
    const int bj = blockIdx.x;
    double s[5];
    uz::ncc_sums(Ess + (size_t)(bj / A) * P, Esy + (size_t)bj * P, P, s, sm);
    if (threadIdx.x == 0) out[bj] = uz::ncc_of_sums(s, P);
}

// metrics._iou_dist_sum's conventions on one pair and one label
__device__ __forceinline__ double iou_of(const int* __restrict__ c) {
    const int inter = c[0], ca = c[1], cb = c[2];
    return (ca == 0 && cb == 0) ? 1.0 : (ca == 0 || cb == 0) ? 0.0 : (double)inter / (double)(ca + cb - inter);
}

__global__ __launch_bounds__(256) void score_final_k(const int* __restrict__ counts, int S, int A, int K, long long NP, const float* __restrict__ ncc_pairs,
                                                      double* __restrict__ ged, double* __restrict__ ncc) {
    __shared__ double sm[4 * 3];
    const int b = blockIdx.x;
    const int* base = counts + (size_t)b * K * NP * 3;
    const long long n[3] = {(long long)S * A, (long long)S * S, (long long)A * A};
    double s[3] = {0.0, 0.0, 0.0};
    long long off = 0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        for (long long t = threadIdx.x; t < n[m]; t += 256) {
            double tot = 0.0;
            for (int l = 1; l < K; ++l) tot += iou_of(base + ((size_t)l * NP + off + t) * 3);
            s[m] += 1.0 - tot / (double)(K - 1);
        }
        off += n[m];
    }
    uz::block_sum_d<3>(s, sm);
    if (threadIdx.x == 0) {
        ged[b] = (2.0 / ((double)S * A)) * s[0] - (1.0 / ((double)S * S)) * s[1] - (1.0 / ((double)A * A)) * s[2];
        if (ncc_pairs) {
            double acc = 0.0;
            for (int j = 0; j < A; ++j) acc += (double)ncc_pairs[(size_t)b * A + j];
            ncc[b] = acc / A;
        }
    }
}

}  // namespace

extern "C" size_t uz_score_workspace(int B, int S, int A, int K, int P) { return score_layout(B, S, A, K, P).total; }

extern "C" int uz_score_samples(const uint8_t* labels, const uint8_t* ann, const uint8_t* mean_label, const float* soft,
                                int B, int S, int A, int K, int P, void* workspace,
                                int32_t* counts, double* ged, float* ncc_pairs, double* ncc, double* dice, void* stream) {
    UZ_REQUIRE(K >= 2 && K <= 8, "score_samples: K = %d outside 2 .. 8", K);
    UZ_REQUIRE(B >= 1 && S >= 1 && A >= 1 && P >= 1, "score_samples: bad sizes B %d S %d A %d P %d", B, S, A, P);
    const ScoreLayout l = score_layout(B, S, A, K, P);
    UZ_REQUIRE(l.total != 0, "score_samples: an element count does not fit int32 (B %d S %d A %d K %d P %d)", B, S, A, K, P);
    UZ_REQUIRE(labels && ann && mean_label && workspace && ged && dice, "score_samples: null operand");
    UZ_REQUIRE(!soft || (ncc_pairs && ncc), "score_samples: soft without ncc / ncc_pairs");
    UZ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "score_samples: workspace not 256-byte aligned");
    char* ws = static_cast<char*>(workspace);
    u64* planes = reinterpret_cast<u64*>(ws + l.planes);
    int* cnt = counts ? counts : reinterpret_cast<int*>(ws + l.counts);
    float* ess = reinterpret_cast<float*>(ws + l.ess);
    float* esy = reinterpret_cast<float*>(ws + l.esy);
    hipStream_t st = uz::S(stream);
    const int wblocks = uz::ceil_div(l.W64, 4);
    hipLaunchKernelGGL(score_planes_k, dim3((unsigned)l.maps, wblocks < 1024 ? wblocks : 1024), dim3(256), 0, st,
                       labels, ann, mean_label, S * B, B * A, K, P, l.W64, planes);
    if (int rc = uz::check_launch("score_planes_k")) return rc;
    const long long items = (long long)B * K * l.pairs + (long long)B * A * K;
    hipLaunchKernelGGL(score_pairs_k, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, planes, B, S, A, K, l.W64, l.pairs, cnt, dice);
    if (int rc = uz::check_launch("score_pairs_k")) return rc;
    if (soft) {
        const int nb = uz::ceil_div(P, 256);
        hipLaunchKernelGGL(score_ncc_maps_k, dim3((unsigned)((long long)nb * B)), dim3(256), 0, st, soft, ann, B, S, A, K, P, nb, ess, esy);
        if (int rc = uz::check_launch("score_ncc_maps_k")) return rc;
        hipLaunchKernelGGL(score_ncc_k, dim3((unsigned)(B * A)), dim3(256), 0, st, ess, esy, A, P, ncc_pairs);
        if (int rc = uz::check_launch("score_ncc_k")) return rc;
    }
    hipLaunchKernelGGL(score_final_k, dim3(B), dim3(256), 0, st, cnt, S, A, K, l.pairs, soft ? ncc_pairs : nullptr, ged, ncc);
    return uz::check_launch("score_final_k");
}
