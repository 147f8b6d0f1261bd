// ProbabilisticUnet.predict (models/probabilistic_unet.py): Fcomb - the per-pixel MLP behind the U-Net features - in eval mode for S
// latent draws per image in ONE launch.  Only the z term of the first layer differs between the samples of an image, and it is a
// per-(sample, image) vector, not a plane: a thread loads the 32 features of its pixel(s) once, computes base = W0[:, :32] f + b0
// once, and then walks its samples with every activation in registers - per sample 32 adds of the z term, the eval BatchNorm + ReLU,
// the 32 x 32 units and the K-row head; only the logits go to memory.  fp32 FMAs in a fixed order, no atomics: bit-repeatable.
//   * Weights are indexed uniformly across the wave.  They are reached through a pointer table in device memory, so the compiler
//     cannot prove them unwritten; reading them through the constant address space (they ARE constant for the launch) makes every
//     weight a scalar load and an SGPR operand of the multiply-add instead of a vector load per lane.
//   * PX = 2 pixels per thread (256 apart: plane-coalesced dword accesses whatever the alignment) puts the multiply-adds on
//     v_pk_fma_f32; PX = 1 has twice the workgroups where the plane is too small to fill the chip with pairs.
//   * The samples of an image are split over grid.z (fcomb_route): at B = 1, 128 x 128 the pixels alone are 64 workgroups.
//   * Per chunk of 8 samples the 256 threads compute the 8 x 32 z terms W0[:, 32:] z once into LDS; the workgroups of pixel block 0
//     also write z.  Of the BatchNorm constants only rstd is computed (once per workgroup, into LDS); running_mean, gamma and beta
//     are scalar operands like the weights.  A float4 table in LDS cost 128 more live registers (the scheduler hoists the reads)
//     and spilled under the occupancy bounds below; the scheduling barrier behind every fourth output channel keeps it from
//     hoisting the rest (118 VGPRs at one pixel per thread, 212 at two, no scratch).
#include <stdlib.h>
#include "uz_common.h"

namespace {

constexpr int FC = 32;             // channels of the features and of every hidden layer (probabilistic_unet.py:244)
constexpr int FCOMB_MAXU = 8, FCOMB_MAXL = 8, FCOMB_MAXK = 8;
constexpr int ZCH = 8;             // samples per z-term chunk: ZCH * FC = 256 = one entry per thread
constexpr int FCOMB_WG_TARGET = 512;   // workgroups wanted before the samples stop being split: two per CU
constexpr int FCOMB_SPW_MIN = 4;       // ... but every workgroup recomputes base (one layer's worth of work): at least 4 samples each

typedef float float2_t __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) float* cptr_t;      // constant address space: uniform reads become scalar loads
__device__ __forceinline__ cptr_t as_const(const float* p) { return (cptr_t)(uintptr_t)p; }

template <int PX> struct PV;
template <> struct PV<1> {
    typedef float T;
    static __device__ __forceinline__ T load(const float* p, int q0, int) { return p[q0]; }
    static __device__ __forceinline__ void store(float* p, int q0, int, bool ok0, bool, T v) { if (ok0) p[q0] = v; }
    static __device__ __forceinline__ T relu(T v) { return fmaxf(v, 0.f); }
};
template <> struct PV<2> {
    typedef float2_t T;
    static __device__ __forceinline__ T load(const float* p, int q0, int q1) { T v; v.x = p[q0]; v.y = p[q1]; return v; }
    static __device__ __forceinline__ void store(float* p, int q0, int q1, bool ok0, bool ok1, T v) { if (ok0) p[q0] = v.x; if (ok1) p[q1] = v.y; }
    static __device__ __forceinline__ T relu(T v) { T r; r.x = fmaxf(v.x, 0.f); r.y = fmaxf(v.y, 0.f); return r; }
};

struct FcombRoute { int px, spw, gx, gy, gz; };

// The one predicate: the launch below and uz_fcomb_sample_route both answer from it.
inline void fcomb_route(int B, int S, long long HW, FcombRoute& r) {
    const char* env = getenv("UZ_FCOMB_PX");                         // experiments: force 1 or 2 pixels per thread
    const int forced = env ? atoi(env) : 0;
    for (int px = 2; px >= 1; --px) {
        const long long nb = ((HW + 256 * px - 1) / (256 * px)) * B;   // pixel workgroups
        const long long zt = nb >= FCOMB_WG_TARGET ? 1 : FCOMB_WG_TARGET / nb;
        long long spw = (S + zt - 1) / zt;
        const int lo = S < FCOMB_SPW_MIN ? S : FCOMB_SPW_MIN;
        if (spw < lo) spw = lo;
        r.px = px; r.spw = (int)spw; r.gx = (int)(nb / B); r.gy = B; r.gz = (int)((S + spw - 1) / spw);
        if (forced == px) return;
        if (forced != 1 && forced != 2 && nb * r.gz >= 256) return;   // pairs only where they still give every CU a workgroup
    }
}

// y -> (y - rm) * rstd * gamma + beta, the order of bn.hip's eval kernels
struct BnTab { cptr_t gamma, beta, rm; };
__device__ __forceinline__ BnTab bn_tab(const float* const* params, int u) {
    return BnTab{as_const(params[6 * u + 2]), as_const(params[6 * u + 3]), as_const(params[6 * u + 4])};
}
template <typename T>
__device__ __forceinline__ T bn_apply(T y, const BnTab& t, float rs, int o) { return (y - t.rm[o]) * rs * t.gamma[o] + t.beta[o]; }

template <int PX>
__global__ __launch_bounds__(256, PX == 1 ? 4 : 2) void fcomb_sample_k(const float* __restrict__ feat, size_t strideF, const float* __restrict__ mu,
                                                       const float* __restrict__ sigma, const float* __restrict__ eps,
                                                       const float* const* __restrict__ params, int n_units, float bn_eps, int L, int K, int B,
                                                       int S, int spw, int HW, float* __restrict__ z, float* __restrict__ logits) {
    typedef PV<PX> V;
    typedef typename V::T T;
    __shared__ float rstd[FCOMB_MAXU][FC];
    __shared__ float zs[ZCH][FC];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int p0 = blockIdx.x * (256 * PX) + tid, p1 = p0 + 256;
    const bool ok0 = p0 < HW, ok1 = PX == 2 && p1 < HW;
    const int q0 = ok0 ? p0 : HW - 1, q1 = ok1 ? p1 : HW - 1;          // a thread past the plane reads its last pixel and stores nothing
    const int s_begin = blockIdx.z * spw, s_end = min(S, s_begin + spw);

    for (int e = tid; e < n_units * FC; e += 256) {
        const int u = e >> 5, o = e & 31;
        rstd[u][o] = 1.f / sqrtf(params[6 * u + 5][o] + bn_eps);
    }

    // ---- once per workgroup: base = W0[:, :32] f + b0
    const int ld0 = FC + L;
    const cptr_t w0 = as_const(params[0]), b0 = as_const(params[1]);
    T base[FC];
    {
        T f[FC];
        const float* fp = feat + (size_t)b * strideF;
#pragma unroll
        for (int c = 0; c < FC; ++c) f[c] = V::load(fp + (size_t)c * HW, q0, q1);
#pragma unroll
        for (int o = 0; o < FC; ++o) {
            T a = T(b0[o]);
#pragma unroll
            for (int c = 0; c < FC; ++c) a += f[c] * w0[o * ld0 + c];
            base[o] = a;
        }
    }
    const BnTab bn0 = bn_tab(params, 0);
    const cptr_t wl = as_const(params[6 * n_units]), bl = as_const(params[6 * n_units + 1]);

    for (int sc = s_begin; sc < s_end; sc += ZCH) {
        __syncthreads();                                               // the previous chunk's z terms are read (first pass: rstd is written)
        {
            const int s = sc + (tid >> 5), o = tid & 31;
            if (s < s_end) {
                const size_t row = (size_t)s * B + b;
                float a = 0.f;
                for (int l = 0; l < L; ++l)
                    a = fmaf(params[0][o * ld0 + FC + l], fmaf(sigma[b * L + l], eps[row * L + l], mu[b * L + l]), a);
                zs[tid >> 5][o] = a;
                if (blockIdx.x == 0 && o < L) z[row * L + o] = fmaf(sigma[b * L + o], eps[row * L + o], mu[b * L + o]);
            }
        }
        __syncthreads();
        const int ns = min(ZCH, s_end - sc);
        for (int sl = 0; sl < ns; ++sl) {
            T h[FC];
#pragma unroll
            for (int o = 0; o < FC; ++o) h[o] = V::relu(bn_apply<T>(base[o] + zs[sl][o], bn0, rstd[0][o], o));
            for (int u = 1; u < n_units; ++u) {
                const cptr_t w = as_const(params[6 * u]), bias = as_const(params[6 * u + 1]);
                const BnTab bnu = bn_tab(params, u);
                T n[FC];
#pragma unroll
                for (int o = 0; o < FC; ++o) {
                    T a = T(bias[o]);
#pragma unroll
                    for (int c = 0; c < FC; ++c) a += h[c] * w[o * FC + c];
                    n[o] = V::relu(bn_apply<T>(a, bnu, rstd[u][o], o));
                    if (o % 4 == 3) __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int o = 0; o < FC; ++o) h[o] = n[o];
            }
            float* out = logits + ((size_t)(sc + sl) * B + b) * K * HW;
            for (int k = 0; k < K; ++k) {
                T a = T(bl[k]);
#pragma unroll
                for (int c = 0; c < FC; ++c) a += h[c] * wl[k * FC + c];
                V::store(out + (size_t)k * HW, p0, p1, ok0, ok1, a);
            }
        }
    }
}

int fcomb_check(int C, int L, int K, int n_units, int B, int S, int H, int W) {
    UZ_REQUIRE(C == FC, "fcomb_sample: %d feature channels, the model fixes them at 32 (probabilistic_unet.py:244)", C);
    UZ_REQUIRE(L >= 1 && L <= FCOMB_MAXL, "fcomb_sample: 1..8 latent dimensions supported (got %d)", L);
    UZ_REQUIRE(K >= 1 && K <= FCOMB_MAXK, "fcomb_sample: 1..8 classes supported (got %d)", K);
    UZ_REQUIRE(n_units >= 1 && n_units <= FCOMB_MAXU, "fcomb_sample: 1..8 Conv-BN-ReLU units supported (got %d)", n_units);
    UZ_REQUIRE(B > 0 && B <= 65535 && S > 0 && H > 0 && W > 0, "fcomb_sample: bad sizes");
    UZ_REQUIRE((long long)H * W < (1ll << 31) - 512, "fcomb_sample: plane too large");
    return 0;
}

}  // namespace

extern "C" int uz_fcomb_sample_route(int L, int K, int n_units, int B, int S, int H, int W, int* out) {
    UZ_REQUIRE(out, "fcomb_sample_route: five ints to answer into");
    if (int rc = fcomb_check(FC, L, K, n_units, B, S, H, W)) return rc;
    FcombRoute r;
    fcomb_route(B, S, (long long)H * W, r);
    out[0] = 256 * r.px; out[1] = r.spw; out[2] = r.gx; out[3] = r.gy; out[4] = r.gz;
    return 0;
}

extern "C" int uz_fcomb_sample_fwd(const float* feat, int C, int CtotF, const float* mu, const float* sigma, const float* eps,
                                   const float* const* params, int n_units, float bn_eps, int L, int K, int B, int S, int H, int W,
                                   float* z, float* logits, void* stream) {
    if (int rc = fcomb_check(C, L, K, n_units, B, S, H, W)) return rc;
    UZ_REQUIRE(feat && mu && sigma && eps && params && z && logits && CtotF >= C, "fcomb_sample_fwd: bad arguments");
    const int HW = H * W;
    FcombRoute r;
    fcomb_route(B, S, HW, r);
    UZ_REQUIRE(r.gz <= 65535, "fcomb_sample_fwd: too many sample groups");
    const dim3 grid(r.gx, r.gy, r.gz);
    const size_t strideF = (size_t)CtotF * HW;
    hipStream_t st = uz::S(stream);
    if (r.px == 2)
        hipLaunchKernelGGL(fcomb_sample_k<2>, grid, dim3(256), 0, st, feat, strideF, mu, sigma, eps, params, n_units, bn_eps, L, K, B, S, r.spw, HW, z, logits);
    else
        hipLaunchKernelGGL(fcomb_sample_k<1>, grid, dim3(256), 0, st, feat, strideF, mu, sigma, eps, params, n_units, bn_eps, L, K, B, S, r.spw, HW, z, logits);
    return uz::check_launch("fcomb_sample_k");
}
