// Mask-free inference (PHISeg.predict, models/phiseg.py): the two kernels between and behind its two plans.
//   - uz_batch_repeat_fwd: patch.repeat(S, 1, 1, 1) of a channel slice - the prior trunk's feature maps, computed once per image, into
//     the S*B rows of the plan that draws the samples;
//   - uz_sample_stats: what a user wants from S samples - label maps, mean class probabilities, their argmax and the predictive
//     entropy - from ONE read of the level logits.
// Both are streaming kernels on tensors of a few MB at most: what bounds them is how many loads the chip has in flight, so the
// workgroups are single waves (a 128 x 128 image is 256 of them: one per CU) and nothing is staged, reduced or synchronised.
#include "uz_common.h"

namespace {

// One thread moves VEC consecutive floats of image b's slice (its C planes are contiguous: n = C * HW floats) to the S rows
// s * B + b of y: read once, written S times.
template <typename T>
__global__ __launch_bounds__(256) void batch_repeat_k(const float* __restrict__ x, float* __restrict__ y, int n, size_t strideX, size_t strideY,
                                                       int B, int S) {
    constexpr int VEC = sizeof(T) / 4;
    const int e = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (e >= n / VEC) return;
    const T v = *reinterpret_cast<const T*>(x + (size_t)b * strideX + (size_t)e * VEC);
    float* d = y + (size_t)b * strideY + (size_t)e * VEC;
    for (int s = 0; s < S; ++s) *reinterpret_cast<T*>(d + (size_t)s * B * strideY) = v;
}

// One thread owns pixel q of image b and walks its S samples in order: consecutive lanes read consecutive floats of every
// (level, sample, class) plane, the running mean stays in registers, every output is written once.
// The logits are summed in fp32 like acc_softmax_argmax_k (pointwise.hip); everything behind the sum is fp64 and rounded once on
// the way out.  In fp32 a sample that saturates (p = 1 - 1e-10) rounds to exactly 1, and a pixel whose samples saturate in opposite
// directions ends in an exact tie of its mean probabilities that is none: the mean label would be a coin the first class always
// wins.  The kernel waits on its loads, K exponentials per sample do not show.
template <int K>
__global__ __launch_bounds__(64) void sample_stats_k(const float* const* __restrict__ sp, int L, int B, int S, int HW,
                                                      float* __restrict__ soft, uint8_t* __restrict__ labels, float* __restrict__ mean_soft,
                                                      uint8_t* __restrict__ mean_label, float* __restrict__ entropy) {
    const int q = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    if (q >= HW) return;
    double m[K];
#pragma unroll
    for (int k = 0; k < K; ++k) m[k] = 0.0;
#pragma unroll 2
    for (int s = 0; s < S; ++s) {
        const size_t row = (size_t)s * B + b, base = row * K * HW + q;
        float a[K];
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = sp[L - 1][base + (size_t)k * HW];        // the level order of acc_softmax_argmax_k
        for (int l = 0; l < L - 1; ++l)
#pragma unroll
            for (int k = 0; k < K; ++k) a[k] += sp[l][base + (size_t)k * HW];
        float mx = a[0];
        int best = 0;
#pragma unroll
        for (int k = 1; k < K; ++k) {
            if (a[k] > mx) { mx = a[k]; best = k; }                                 // first maximum wins
        }
        double e[K], se = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) { e[k] = exp((double)a[k] - (double)mx); se += e[k]; }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double sv = e[k] / se;
            m[k] += sv;                                                             // ordered: s = 0 .. S-1, bit-repeatable
            if (soft) soft[base + (size_t)k * HW] = (float)sv;
        }
        if (labels) labels[row * HW + q] = (uint8_t)best;
    }
    int best = 0;
    double h = 0.0, bv = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double p = m[k] / (double)S;
        mean_soft[((size_t)b * K + k) * HW + q] = (float)p;
        if (k == 0 || p > bv) { bv = p; best = k; }
        if (p > 0.0) h -= p * log(p);                                              // a class no sample gave any weight adds nothing
    }
    if (mean_label) mean_label[(size_t)b * HW + q] = (uint8_t)best;
    if (entropy) entropy[(size_t)b * HW + q] = (float)h;
}

template <int K>
void launch_stats(dim3 grid, hipStream_t st, const float* const* sp, int L, int B, int S, int HW, float* soft, uint8_t* labels, float* mean_soft,
                  uint8_t* mean_label, float* entropy) {
    hipLaunchKernelGGL(sample_stats_k<K>, grid, dim3(64), 0, st, sp, L, B, S, HW, soft, labels, mean_soft, mean_label, entropy);
}

}  // namespace

extern "C" int uz_batch_repeat_fwd(const float* x, int C, int CtotX, float* y, int CtotY, int B, int S, int H, int W, void* stream) {
    UZ_REQUIRE(x && y && C > 0 && CtotX >= C && CtotY >= C && B > 0 && B <= 65535 && S > 0 && H > 0 && W > 0, "batch_repeat_fwd: bad arguments");
    const long long HW = (long long)H * W, n = HW * C;
    UZ_REQUIRE(n < (1ll << 31), "batch_repeat_fwd: slice too large");
    const size_t sx = (size_t)CtotX * HW, sy = (size_t)CtotY * HW;
    hipStream_t st = uz::S(stream);
    // whole float4 of every plane and 16-byte slice origins: every image's slice then starts on a 16-byte boundary too
    if (HW % 4 == 0 && uz::align_of(x) == 16 && uz::align_of(y) == 16)
        hipLaunchKernelGGL(batch_repeat_k<float4>, dim3(uz::ceil_div((int)(n / 4), 256), B), dim3(256), 0, st, x, y, (int)n, sx, sy, B, S);
    else
        hipLaunchKernelGGL(batch_repeat_k<float>, dim3(uz::ceil_div((int)n, 256), B), dim3(256), 0, st, x, y, (int)n, sx, sy, B, S);
    return uz::check_launch("batch_repeat_k");
}

extern "C" int uz_sample_stats(const float* const* s_ptrs, int L, int K, int B, int S, int H, int W, float* soft, uint8_t* labels,
                               float* mean_soft, uint8_t* mean_label, float* entropy, void* stream) {
    UZ_REQUIRE(K >= 1 && K <= 8, "sample_stats: 1..8 classes supported (got %d)", K);
    UZ_REQUIRE(s_ptrs && mean_soft && L >= 1 && B > 0 && B <= 65535 && S > 0 && H > 0 && W > 0, "sample_stats: bad arguments");
    const long long HW = (long long)H * W;
    UZ_REQUIRE(HW < (1ll << 31), "sample_stats: plane too large");
    const dim3 grid(uz::ceil_div((int)HW, 64), B);
    hipStream_t st = uz::S(stream);
    switch (K) {
        case 1: launch_stats<1>(grid, st, s_ptrs, L, B, S, (int)HW, soft, labels, mean_soft, mean_label, entropy); break;
        case 2: launch_stats<2>(grid, st, s_ptrs, L, B, S, (int)HW, soft, labels, mean_soft, mean_label, entropy); break;
        case 3: launch_stats<3>(grid, st, s_ptrs, L, B, S, (int)HW, soft, labels, mean_soft, mean_label, entropy); break;
        case 4: launch_stats<4>(grid, st, s_ptrs, L, B, S, (int)HW, soft, labels, mean_soft, mean_label, entropy); break;
        case 5: launch_stats<5>(grid, st, s_ptrs, L, B, S, (int)HW, soft, labels, mean_soft, mean_label, entropy); break;
        case 6: launch_stats<6>(grid, st, s_ptrs, L, B, S, (int)HW, soft, labels, mean_soft, mean_label, entropy); break;
        case 7: launch_stats<7>(grid, st, s_ptrs, L, B, S, (int)HW, soft, labels, mean_soft, mean_label, entropy); break;
        default: launch_stats<8>(grid, st, s_ptrs, L, B, S, (int)HW, soft, labels, mean_soft, mean_label, entropy); break;
    }
    return uz::check_launch("sample_stats_k");
}
