// Validation metrics of the reference harness on the device (train_model.py:186-230):
//   - pair counts |A == l and B == l|, |A == l|, |B == l| for every (sample, ground truth) pair of integer
//     label maps: the integer core of generalised_energy_distance (utils.py:148-200, IoU via medpy jc) and of the
//     per-label Dice (train_model.py:212-224, medpy dc).  Exact integer arithmetic -> bit-exact parity.
//   - the two pixel-wise cross-entropy maps of variance_ncc_dist (utils.py:202-247) and the normalised
//     cross-correlation of a map pair (utils.py:130-145).
#include "uz_common.h"

namespace {

__global__ __launch_bounds__(256) void pair_counts_k(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int HW, int label,
                                                      int* __restrict__ out) {
    __shared__ int sm[3][4];
    const int i = blockIdx.x, j = blockIdx.y, nb = gridDim.y;
    const uint8_t* pa = a + (size_t)i * HW;
    const uint8_t* pb = b + (size_t)j * HW;
    int inter = 0, ca = 0, cb = 0;
    for (int q = threadIdx.x; q < HW; q += 256) {
        const int x = pa[q] == label, y = pb[q] == label;
        inter += x & y; ca += x; cb += y;
    }
    inter = uz::wave_sum(inter); ca = uz::wave_sum(ca); cb = uz::wave_sum(cb);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sm[0][w] = inter; sm[1][w] = ca; sm[2][w] = cb; }
    __syncthreads();
    if (threadIdx.x < 3) out[((size_t)i * nb + j) * 3 + threadIdx.x] = sm[threadIdx.x][0] + sm[threadIdx.x][1] + sm[threadIdx.x][2] + sm[threadIdx.x][3];
}

// E_ss[p] = mean_i( -sum_k mean_seg[k,p] * log(s_i[k,p] + eps) ),  E_sy[j,p] = mean_i( -sum_k gt_j[k,p] * log(s_i[k,p] + eps) ): uz::ncc_maps_px
__global__ __launch_bounds__(256) void ncc_maps_k(const float* __restrict__ soft, const float* __restrict__ gt, int N, int M, int K, int HW,
                                                   float* __restrict__ Ess, float* __restrict__ Esy) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= HW) return;
    uz::ncc_maps_px(soft, K, N, M, K, HW, q, gt, Ess, Esy);
}

// ncc(a, v) with zero_norm=True (utils.py:130-145) = Pearson correlation of the two maps: uz::ncc_sums, uz::ncc_of_sums
__global__ __launch_bounds__(256) void ncc_k(const float* __restrict__ a, const float* __restrict__ v, int HW, float* __restrict__ out) {
    __shared__ double sm[4 * 5];
    double s[5];
    uz::ncc_sums(a, v + (size_t)blockIdx.x * HW, HW, s, sm);
    if (threadIdx.x == 0) out[blockIdx.x] = uz::ncc_of_sums(s, HW);
}

}  // namespace

extern "C" int uz_label_pair_counts(const uint8_t* a, int Na, const uint8_t* b, int Nb, int HW, int label, int32_t* out, void* stream) {
    UZ_REQUIRE(Na > 0 && Nb > 0 && HW > 0 && Nb <= 65535, "label_pair_counts: bad sizes");
    hipLaunchKernelGGL(pair_counts_k, dim3(Na, Nb), dim3(256), 0, uz::S(stream), a, b, HW, label, out);
    return uz::check_launch("pair_counts_k");
}
extern "C" int uz_ncc_maps(const float* soft, const float* gt_onehot, int N, int M, int K, int HW, float* E_ss, float* E_sy, void* stream) {
    UZ_REQUIRE(N > 0 && M > 0 && K > 0 && HW > 0, "ncc_maps: bad sizes");
    hipLaunchKernelGGL(ncc_maps_k, dim3(uz::ceil_div(HW, 256)), dim3(256), 0, uz::S(stream), soft, gt_onehot, N, M, K, HW, E_ss, E_sy);
    return uz::check_launch("ncc_maps_k");
}
extern "C" int uz_ncc(const float* a, const float* v, int M, int HW, float* out, void* stream) {
    UZ_REQUIRE(M > 0 && HW > 0, "ncc: bad sizes");
    hipLaunchKernelGGL(ncc_k, dim3(M), dim3(256), 0, uz::S(stream), a, v, HW, out);
    return uz::check_launch("ncc_k");
}
