// Mask-free inference (PHISeg.predict, models/phiseg.py): the two kernels between and behind its two plans.
//   - uz_batch_repeat_fwd: patch.repeat(S, 1, 1, 1) of a channel slice - the prior trunk's feature maps, computed once per image, into
//     the S*B rows of the plan that draws the samples;
//   - uz_sample_stats: what a user wants from S samples - label maps, mean class probabilities, their argmax and the predictive
//     entropy - from ONE read of the level logits;
// and the two behind every sample of a volume (PHISeg3D.predict, models/phiseg3D.py), drawn one after another on a one-volume plan:
//   - uz_vol_sample_accum: one sample's labels, probabilities and its term of a running fp64 sum, read from the L level logits at
//     their OWN resolution (the nearest resize to the full volume is an index computation, never a tensor);
//   - uz_vol_sample_finish: mean probabilities, their argmax and the entropy from that sum.
// The per-voxel arithmetic of the three statistics kernels is ONE set of device functions (sample_softmax, mean_stats), so the
// streamed pair gives the bits uz_sample_stats gives on the materialised levels.
// All are streaming kernels on tensors of a few MB (a 128 x 128 x 64 volume: 1 M voxels, a running sum of 25 MB): what bounds them is
// how many loads the chip has in flight, so the workgroups are single waves (a 128 x 128 image is 256 of them: one per CU; the
// volume 16 384) and nothing is staged, reduced or synchronised.
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
// The kernel waits on its loads, K exponentials per sample do not show.
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
        double sv[K];
        const int best = uz::sample_softmax<K>(a, sv);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            m[k] += sv[k];                                                          // ordered: s = 0 .. S-1, bit-repeatable
            if (soft) soft[base + (size_t)k * HW] = (float)sv[k];
        }
        if (labels) labels[row * HW + q] = (uint8_t)best;
    }
    double p[K], h;
    const int best = uz::mean_stats<K>(m, S, p, h);
#pragma unroll
    for (int k = 0; k < K; ++k) mean_soft[((size_t)b * K + k) * HW + q] = (float)p[k];
    if (mean_label) mean_label[(size_t)b * HW + q] = (uint8_t)best;
    if (entropy) entropy[(size_t)b * HW + q] = (float)h;
}

// ---- volumes.  A level is [D_l][Ctot_l][H_l][W_l] (Plan.vol: the pointer addresses real slice 0); voxel (od, oy, ox) of the full volume
// reads its element (od / fz, oy / f, ox / f), the index of nearest3d_fwd_k (vol.hip).  The table travels as a kernel argument.
// (uz::VolLevels, sample_softmax, mean_stats: uz_common.h - shared with volwindow.hip)

// One voxel per thread, consecutive lanes consecutive voxels of a row: the finest level, the label store and the running sum are
// coalesced; the coarser levels repeat an element over f lanes and come out of cache.  The outputs are dense (K, D, H, W) / (D, H, W).
// (A form with four voxels per thread - float4 loads, one 4-byte label store, double2 traffic of the sum - was built and measured:
// 20.0 against 21.5 us for a 128 x 128 x 64 volume, and no gain in the finish kernel, beside 8.4 ms of plan per sample; it was dropped.)
template <int K>
__global__ __launch_bounds__(64) void vol_sample_accum_k(uz::VolLevels lv, int L, int D, int H, int W, uint8_t* __restrict__ labels,
                                                          float* __restrict__ soft, double* __restrict__ acc, int first) {
    const int HW = H * W, n = D * HW;
    const long long q64 = (long long)blockIdx.x * 64 + threadIdx.x;                // (the last workgroup of a 2^31 - 1 voxel volume)
    if (q64 >= n) return;
    const int q = (int)q64, od = q / HW, r = q - od * HW, oy = r / W, ox = r - oy * W;
    float a[K];
    for (int j = 0; j < L; ++j) {
        const int l = j == 0 ? L - 1 : j - 1;                                       // last level first, then 0 .. L-2: the order of sample_stats_k
        const int f = lv.f[l], Hl = H / f, Wl = W / f;
        const float* s = lv.p[l] + ((size_t)(od / lv.fz[l]) * lv.ctot[l]) * Hl * Wl + (size_t)(oy / f) * Wl + ox / f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float x = s[(size_t)k * Hl * Wl];
            a[k] = j == 0 ? x : a[k] + x;
        }
    }
    double sv[K];
    labels[q] = (uint8_t)uz::sample_softmax<K>(a, sv);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const size_t o = (size_t)k * n + q;
        if (soft) soft[o] = (float)sv[k];
        acc[o] = first ? sv[k] : acc[o] + sv[k];                                    // the samples arrive in order: bit-repeatable
    }
}

template <int K>
__global__ __launch_bounds__(64) void vol_sample_finish_k(const double* __restrict__ acc, int S, int n, float* __restrict__ mean_soft,
                                                           uint8_t* __restrict__ mean_label, float* __restrict__ entropy) {
    const long long q64 = (long long)blockIdx.x * 64 + threadIdx.x;
    if (q64 >= n) return;
    const int q = (int)q64;
    double m[K], p[K], h;
#pragma unroll
    for (int k = 0; k < K; ++k) m[k] = acc[(size_t)k * n + q];
    const int best = uz::mean_stats<K>(m, S, p, h);
#pragma unroll
    for (int k = 0; k < K; ++k) mean_soft[(size_t)k * n + q] = (float)p[k];
    if (mean_label) mean_label[q] = (uint8_t)best;
    if (entropy) entropy[q] = (float)h;
}

template <int K>
void launch_stats(dim3 grid, hipStream_t st, const float* const* sp, int L, int B, int S, int HW, float* soft, uint8_t* labels, float* mean_soft,
                  uint8_t* mean_label, float* entropy) {
    hipLaunchKernelGGL(sample_stats_k<K>, grid, dim3(64), 0, st, sp, L, B, S, HW, soft, labels, mean_soft, mean_label, entropy);
}

template <int K>
void launch_vol_accum(int groups, hipStream_t st, const uz::VolLevels& lv, int L, int D, int H, int W, uint8_t* labels, float* soft, double* acc, int first) {
    hipLaunchKernelGGL(vol_sample_accum_k<K>, dim3(groups), dim3(64), 0, st, lv, L, D, H, W, labels, soft, acc, first);
}
template <int K>
void launch_vol_finish(int groups, hipStream_t st, const double* acc, int S, int n, float* mean_soft, uint8_t* mean_label, float* entropy) {
    hipLaunchKernelGGL(vol_sample_finish_k<K>, dim3(groups), dim3(64), 0, st, acc, S, n, mean_soft, mean_label, entropy);
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

extern "C" int uz_vol_sample_accum(const float* const* s_ptrs, const int* ctot, const int* f, const int* fz, int L, int K, int D, int H, int W,
                                   uint8_t* labels, float* soft, double* acc, int first, void* stream) {
    UZ_REQUIRE(K >= 1 && K <= 8, "vol_sample_accum: 1..8 classes supported (got %d)", K);
    UZ_REQUIRE(L >= 1 && L <= uz::VOL_LEVELS_MAX, "vol_sample_accum: 1..8 levels supported (got %d)", L);
    UZ_REQUIRE(s_ptrs && ctot && f && fz && labels && acc && D > 0 && H > 0 && W > 0, "vol_sample_accum: bad arguments");
    const long long n = (long long)D * H * W;
    UZ_REQUIRE(n < (1ll << 31), "vol_sample_accum: volume too large");
    uz::VolLevels lv = {};
    for (int l = 0; l < L; ++l) {
        UZ_REQUIRE(s_ptrs[l], "vol_sample_accum: level %d is a null pointer", l);
        UZ_REQUIRE(f[l] >= 1 && fz[l] >= 1 && ctot[l] >= K, "vol_sample_accum: level %d: factors below 1 or fewer channels than classes", l);
        UZ_REQUIRE(D % fz[l] == 0 && H % f[l] == 0 && W % f[l] == 0, "vol_sample_accum: level %d: the volume is not level size x factor", l);
        lv.p[l] = s_ptrs[l]; lv.ctot[l] = ctot[l]; lv.f[l] = f[l]; lv.fz[l] = fz[l];
    }
    const int r = (int)((n + 63) / 64);
    hipStream_t st = uz::S(stream);
    switch (K) {
        case 1: launch_vol_accum<1>(r, st, lv, L, D, H, W, labels, soft, acc, first); break;
        case 2: launch_vol_accum<2>(r, st, lv, L, D, H, W, labels, soft, acc, first); break;
        case 3: launch_vol_accum<3>(r, st, lv, L, D, H, W, labels, soft, acc, first); break;
        case 4: launch_vol_accum<4>(r, st, lv, L, D, H, W, labels, soft, acc, first); break;
        case 5: launch_vol_accum<5>(r, st, lv, L, D, H, W, labels, soft, acc, first); break;
        case 6: launch_vol_accum<6>(r, st, lv, L, D, H, W, labels, soft, acc, first); break;
        case 7: launch_vol_accum<7>(r, st, lv, L, D, H, W, labels, soft, acc, first); break;
        default: launch_vol_accum<8>(r, st, lv, L, D, H, W, labels, soft, acc, first); break;
    }
    return uz::check_launch("vol_sample_accum_k");
}

extern "C" int uz_vol_sample_finish(const double* acc, int K, int S, int D, int H, int W, float* mean_soft, uint8_t* mean_label, float* entropy,
                                    void* stream) {
    UZ_REQUIRE(K >= 1 && K <= 8, "vol_sample_finish: 1..8 classes supported (got %d)", K);
    UZ_REQUIRE(acc && mean_soft && S > 0 && D > 0 && H > 0 && W > 0, "vol_sample_finish: bad arguments");
    const long long n = (long long)D * H * W;
    UZ_REQUIRE(n < (1ll << 31), "vol_sample_finish: volume too large");
    const int r = (int)((n + 63) / 64);
    hipStream_t st = uz::S(stream);
    switch (K) {
        case 1: launch_vol_finish<1>(r, st, acc, S, (int)n, mean_soft, mean_label, entropy); break;
        case 2: launch_vol_finish<2>(r, st, acc, S, (int)n, mean_soft, mean_label, entropy); break;
        case 3: launch_vol_finish<3>(r, st, acc, S, (int)n, mean_soft, mean_label, entropy); break;
        case 4: launch_vol_finish<4>(r, st, acc, S, (int)n, mean_soft, mean_label, entropy); break;
        case 5: launch_vol_finish<5>(r, st, acc, S, (int)n, mean_soft, mean_label, entropy); break;
        case 6: launch_vol_finish<6>(r, st, acc, S, (int)n, mean_soft, mean_label, entropy); break;
        case 7: launch_vol_finish<7>(r, st, acc, S, (int)n, mean_soft, mean_label, entropy); break;
        default: launch_vol_finish<8>(r, st, acc, S, (int)n, mean_soft, mean_label, entropy); break;
    }
    return uz::check_launch("vol_sample_finish_k");
}
