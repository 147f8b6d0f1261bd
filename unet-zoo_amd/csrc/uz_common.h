// Shared helpers for the libuz_hip.so kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <limits.h>
#include <algorithm>
#include <type_traits>
#include "uz_api.h"

namespace uz {

void set_error(const char* fmt, ...);
int  fail(const char* fmt, ...);          // set_error + return -1
int  check_launch(const char* what);      // hipGetLastError -> status
extern long long* debug_stamps;           // diagnostics: per-workgroup cycle stamps of the split kernels (uz_debug_stamps), normally null
int  conv_math_mode();                    // 0 fp32 MFMA only | 1 split-fp16 where it pays | 2 split-fp16 wherever eligible | 3 bf16 (one piece, one product) where 1 would split
int  conv_np();                           // operand planes of the split kernels under the current mode: 2 (fp16 split) or 1 (bf16)

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int pow2_ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }
static inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
// byte alignment of a float view as the streaming dispatch sees it: 16, 8 or 4 (NULL, an absent operand, constrains nothing: 16)
static inline int align_of(const void* p) { const uintptr_t a = reinterpret_cast<uintptr_t>(p); return (a & 15) == 0 ? 16 : (a & 7) == 0 ? 8 : 4; }

// The dispatcher deals consecutive workgroup ids round-robin over the 8 XCDs (each with a
// private L2).  Remap so that every XCD walks a contiguous chunk of the work list: blocks that
// share operand panels then hit the same L2.  Bijective for any nwg (cdna guide 5.5 T1).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, slot = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

// Reductions over the 64 lanes of a wave, a butterfly in the order o = 32 .. 1: every lane ends with the result.
template <class T> __device__ __forceinline__ T lane_xor(T v, int o) { return __shfl_xor(v, o, 64); }
template <> __device__ __forceinline__ unsigned long long lane_xor(unsigned long long v, int o) { return (unsigned long long)__shfl_xor((long long)v, o, 64); }
template <class T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += lane_xor(v, o);
    return v;
}
template <class T> __device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, lane_xor(v, o));
    return v;
}
template <class T> __device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, lane_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) { return wave_sum<double>(v); }

// Block-wide sum of NV doubles (blockDim.x == 256).  Result valid in thread 0.
template <int NV>
__device__ __forceinline__ void block_sum_d(double (&v)[NV], double* smem /* >= 4*NV */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum_d(v[i]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) smem[wave * NV + i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = smem[i] + smem[NV + i] + smem[2 * NV + i] + smem[3 * NV + i];
    }
}

// The arithmetic of variance_ncc_dist (utils.py:130-145,202-247), shared by metrics.hip (one image, materialised one-hot ground truths)
// and score.hip (B images, the one-hot read from uint8 labels): ONE statement of it, so the two agree bit for bit.
// ncc_maps_px, pixel q of one image: sample i, class k is soft[(i * R + k) * HW + q] (R maps of HW pixels per sample); gt holds the M ground truths, as one-hot
// floats (M, K, HW) or as uint8 label maps (M, HW) whose one-hot value is 1 where the label equals k (a product with 1.0f is exact).  E_ss[q] = mean_i( -sum_k mean_seg[k] * log(s_i[k] + eps) ), E_sy[j][q] = mean_i( -sum_k gt_j[k] * log(s_i[k] + eps) ):
// fp32 mean over the samples in the order i = 0 .. N-1, fp64 accumulation of fp32 products.
template <class GT>
__device__ __forceinline__ void ncc_maps_px(const float* soft, int R, int N, int M, int K, int HW, int q, const GT* gt, float* Ess, float* Esy) {
    double ess = 0.0;
    for (int k = 0; k < K; ++k) {
        float ms = 0.f;
        for (int i = 0; i < N; ++i) ms += soft[((size_t)i * R + k) * HW + q];
        ms /= (float)N;
        double acc = 0.0;
        for (int i = 0; i < N; ++i) acc += (double)(ms * logf(soft[((size_t)i * R + k) * HW + q] + 1e-8f));
        ess -= acc;
    }
    Ess[q] = (float)(ess / N);
    for (int j = 0; j < M; ++j) {
        double acc = 0.0;
        for (int k = 0; k < K; ++k) {
            float g;
            if constexpr (std::is_same<GT, float>::value) g = gt[((size_t)j * K + k) * HW + q];        // float: materialised one-hot (M, K, HW)
            else g = gt[(size_t)j * HW + q] == k ? 1.f : 0.f;                           // uint8_t: label maps (M, HW)
            if (g != 0.f)
                for (int i = 0; i < N; ++i) acc -= (double)(g * logf(soft[((size_t)i * R + k) * HW + q] + 1e-8f));
        }
        Esy[(size_t)j * HW + q] = (float)(acc / N);
    }
}
// ncc(a, v) with zero_norm=True (utils.py:130-145) = Pearson correlation of two maps of HW pixels, by one 256-thread workgroup:
// ncc_sums leaves the five fp64 sums in thread 0 (sm: >= 20 doubles of LDS), ncc_of_sums is what thread 0 makes of them.
__device__ __forceinline__ void ncc_sums(const float* __restrict__ a, const float* __restrict__ v, int HW, double (&s)[5], double* sm) {
    for (int i = 0; i < 5; ++i) s[i] = 0.0;
    for (int q = threadIdx.x; q < HW; q += 256) {
        const double x = a[q], y = v[q];
        s[0] += x; s[1] += x * x; s[2] += y; s[3] += y * y; s[4] += x * y;
    }
    block_sum_d<5>(s, sm);
}
__device__ __forceinline__ float ncc_of_sums(const double (&s)[5], int HW) {
    const double n = HW, ma = s[0] / n, mv = s[2] / n;
    const double sa = sqrt(fmax(s[1] / n - ma * ma, 0.0)), sv = sqrt(fmax(s[3] / n - mv * mv, 0.0));
    return (float)((s[4] / n - ma * mv) / (sa * sv));
}

// The per-voxel arithmetic every statistics kernel shares (predict.hip, volwindow.hip).  The logits are summed in fp32 like acc_softmax_argmax_k
// (pointwise.hip); everything behind the sum is fp64 and rounded once on the way out.  In fp32 a sample that saturates
// (p = 1 - 1e-10) rounds to exactly 1, and a pixel whose samples saturate in opposite directions ends in an exact tie of its mean
// probabilities that is none: the mean label would be a coin the first class always wins.
template <int K>
__device__ __forceinline__ int sample_softmax(const float (&a)[K], double (&sv)[K]) {
    float mx = a[0];
    int best = 0;
#pragma unroll
    for (int k = 1; k < K; ++k) {
        if (a[k] > mx) { mx = a[k]; best = k; }                                     // first maximum wins
    }
    double se = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) { sv[k] = exp((double)a[k] - (double)mx); se += sv[k]; }
#pragma unroll
    for (int k = 0; k < K; ++k) sv[k] = sv[k] / se;
    return best;
}
// m: the sum of S samples' probabilities.  p = m / S, its first maximum, its entropy (a class no sample gave any weight adds nothing)
template <int K>
__device__ __forceinline__ int mean_stats(const double (&m)[K], int S, double (&p)[K], double& h) {
    int best = 0;
    double bv = 0.0;
    h = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        p[k] = m[k] / (double)S;
        if (k == 0 || p[k] > bv) { bv = p[k]; best = k; }
        if (p[k] > 0.0) h -= p[k] * log(p[k]);
    }
    return best;
}

// The level table of the volume statistics kernels (predict.hip, volwindow.hip); it travels as a kernel argument.
constexpr int VOL_LEVELS_MAX = 8;
struct VolLevels {
    const float* p[VOL_LEVELS_MAX];
    int ctot[VOL_LEVELS_MAX], f[VOL_LEVELS_MAX], fz[VOL_LEVELS_MAX];
};

// What the volume post-processing files share (volscore.hip, volcomp.hip, voluncert.hip, volprep.hip).
// Regions as sets of label values, bit v = value v: of the prediction (p) and of the reference (r); it travels as a kernel argument.
struct RegionSets { uint32_t p[UZ_VOL_MAX_REGIONS], r[UZ_VOL_MAX_REGIONS]; };
static inline RegionSets region_sets(const uint32_t* p, const uint32_t* r, int R) {       // sets beyond R are empty
    RegionSets s = {};
    for (int i = 0; i < R; ++i) { s.p[i] = p[i]; s.r[i] = r[i]; }
    return s;
}
__host__ __device__ __forceinline__ bool in_set(unsigned v, uint32_t set) { return v < 32u && ((set >> (v & 31u)) & 1u); }
static inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }
// workgroups of `threads` that would cover work_items in one sweep (at least one), capped
static inline int sweep_grid(long long work_items, int threads, long long cap = INT_MAX) {
    return (int)std::min<long long>((std::max<long long>(work_items, 1) + threads - 1) / threads, cap);
}
// the reason a call on N volumes of D x H x W voxels is refused, or null (volcomp.hip, volmorph.hip, vollesion.hip)
static inline const char* vol_sizes_bad(int N, int D, int H, int W) {
    if (D < 1 || H < 1 || W < 1) return "empty axis";
    if (N < 1 || N > UZ_VOL_MAX_ROWS) return "1 <= N <= 65536 volumes";
    long long t = N;
    for (int f : {D, H, W}) { t *= f; if (t >= (1LL << 31)) return "N*D*H*W must stay below 2^31"; }
    return nullptr;
}
// two blocks of `bytes` bytes share a byte
static inline bool bytes_overlap(const void* a_, const void* b_, long long bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(a_), b = reinterpret_cast<uintptr_t>(b_);
    return !(a + (uintptr_t)bytes <= b || b + (uintptr_t)bytes <= a);
}

// ---- How a convolution call is routed, and the call itself.  Forward and data gradient: Kc contraction, Mc output channels.
enum { CONV_F32 = 0, CONV_SPLIT = 1, CONV_STREAM = 2, STREAM_HEAD = 1, STREAM_THIN = 2 };     // ConvRoute::family = what uz_conv_route returns; ::stream: 1x1 head | 1..4 input channels
struct Geom { int TW, TH, TB, PW, PSI, PS, tilesX, tilesY, tilesB; };       // fp32 kernel: pixel tile and its LDS patch
struct SplitGeom {                  // matrix-pipe kernel (conv_split.hip)
    int tw, cot;                    // tile width (16: 16 x 16 tiles, 256 threads; 32: 16 x 32 tiles, 512 threads), output channels per tile
    int nChunks, rows;              // chunks of the contraction, rows of the packed weight image
    size_t image_bytes, ws_bytes;   // ... its bytes (all above depend on Kc, Mc and W alone: split_image); workspace = bound slots + image + slabs
    int parts, cps, partials;       // workgroups one tile's chunk loop is shared out over (no empty parts), chunks per part; rows of per-channel partials a fused epilogue writes (0: split loop)
};
struct ConvRoute {
    int family = CONV_F32, stream = 0;
    SplitGeom s = {};               // CONV_SPLIT
    Geom g = {}; int msub = 0, jmax = 0, ksplit = 1, cps = 0;      // CONV_F32: tile, 32-channel sub-tiles per tile, pixel sub-tiles per wave, split of the chunk loop, chunks per part
    size_t smem = 0, ws_bytes = 0;  // workspace of the family (CONV_F32: the split-K slabs)
};
// streaming = false: the matrix kernels' route (a head with a ReLU epilogue, a thin-input layer with a pre-packed weight image, uz_conv_workspace).
// Pure: reads the math mode and the policy's getenv statics.  Any integers are safe; the entry points refuse empty shapes behind it.
ConvRoute conv_route(int dgrad, int Kc, int Mc, int N, int H, int W, int ks, bool streaming = true);
SplitGeom split_geom(int Kc, int Mc, int N, int H, int W);         // conv_split.hip
struct ConvCall {
    const float* x = nullptr; int Kc = 0, KcTot = 0;               // input view (dy for a data gradient)
    const float* w = nullptr; int wCi = 0; const float* bias = nullptr;     // PyTorch [Cout][Cin][ks][ks] parameter and its Cin
    float* y = nullptr; int Mc = 0, McTot = 0;                      // output view (dx)
    int N = 0, H = 0, W = 0, ks = 0, dgrad = 0, relu = 0, accumulate = 0;
    // x_amax / w_amax: device scalars bounding |x| and |w| (any upper bound within ~2^10 of the true maximum keeps full
    // accuracy); NULL = measure here (one extra pass over the tensor: the stand-alone C-ABI path, the model plans pass
    // bounds that the producing kernels maintain).  y_amax (nullable): atomic max of |y| for the next consumer.
    const float* x_amax = nullptr; const float* w_amax = nullptr; float* y_amax = nullptr;
    void* workspace = nullptr; size_t workspace_bytes = 0;
    const void* packed_w = nullptr;                                 // weight image packed once per step (uz_conv_pack_weights)
    float* bn_partials = nullptr;                                   // fused BatchNorm statistics / the folded epilogue's partial rows
    // slabs_only: stop after the split-K main kernel and leave the partial sums [ksplit][N][Mc][HW] in slabs_out, or at the start of
    // the workspace (the caller's BatchNorm adds them, uz_bn_relu_fwd_slabs / uz_bn_relu_bwd_ex); only legal where the fp32 route's ksplit > 1.
    float* slabs_out = nullptr; bool slabs_only = false; hipStream_t st = nullptr;
    // round-4 options of the split path
    int x_packed = 0;                       // the input operand (x, or dy for a data gradient) is split storage (split_f16.h)
    const float* x_amax2 = nullptr; int seg_channels = 0;      // ... whose channels from seg_channels on were scaled from this bound instead of x_amax
    int mk = 0;                             // epilogue: 0 plain, 1 ReLU mask of the producing unit (mask = its activation), 2 BatchNorm-backward reduction
    const float* mask = nullptr; int maskCtot = 0;
    const float* mk_save = nullptr; int mk_relu = 1;           // mk == 2: [4][C] {mean, rstd, alpha, beta'} of the producing unit (uz_bn_relu_fwd_ex)
    // bf16 STORAGE (single-piece bf16 mode only, unsplit chunk loops): the input operand / the output tensor hold 2-byte bf16 elements
    int x_b16 = 0, y_b16 = 0;
    // round 6: x is the pre-normalisation output of the Conv -> BatchNorm -> ReLU unit in front (fp32) and aff its [4][Kc] {mean, rstd, alpha, beta'} table:
    // the forward convolution's staging applies the unit's BatchNorm + ReLU itself (x_amax = the bound of the APPLIED activation)
    const float* aff = nullptr; int aff_relu = 0;
};
// conv_split.hip: 3x3 forward / data gradient on the fp16 matrix pipe with two-piece split operands (fp32-accurate)
bool conv_split_ok(int Kc, int Mc, int N, int H, int W, int ks, int dgrad);
int conv_split(const ConvCall& c, const ConvRoute& r);
int splitk_reduce(const float* slab, int ksplit, const float* bias, float* y, int Mc, int McTot, int N, int HW, int relu, int accumulate,
                  float* y_amax, hipStream_t st);      // conv_mfma.hip

// ---- weight gradient
enum { WG_HEAD, WG_THIN, WG_SPLIT, WG_FAST, WG_GENERIC };   // streaming 1x1 head | 1..4 input channels | matrix pipe | fp32, one buffer resource | fp32, 64-bit pointers
struct WGeom { int TW, TH, TB, PW, PSI, PS, tilesX, tilesY, tilesB, T, S, nCoT, nCiT, WM, WN, WK, pf, fast, SW; };   // SW: slabs per pixel split
struct WgradRoute {
    int family = WG_GENERIC;
    int slabs = 0, view_slabs = 0;  // partial-sum slabs [ks*ks][Cout][Cin] the call writes before its reduction (0: WG_HEAD) | ... a call on a buffer of the view's size would
    size_t ws_bytes = 0;            // uz_conv_bwd_weight_workspace: enough for every family the shape is eligible for, and the bias gradient
    WGeom g = {}; size_t f32_bytes = 0;     // the fp32 geometry, of every shape: its slab bytes enter ws_bytes, and the entry point asks every call for them
    int per_wg = 0;                 // WG_THIN: row pairs per workgroup
    bool split_eligible = false, huge = false;      // wgrad_split_ok | the BUFFER has 2^30 elements or more: such a call leaves the matrix pipe
    int tw = 0, ct = 0;             // split_eligible: tile width, channel tile (conv_wgrad_split.hip)
};
// Cin, Cout: the views' channels; CinTot, CoutTot: the buffers' (a query passes the views' for both).  Pure, like conv_route().
WgradRoute wgrad_route(int Cin, int Cout, int CinTot, int CoutTot, int N, int H, int W, int ks);
struct WgradCall {
    const float* x = nullptr; int Cin = 0, CinTot = 0; const float* dy = nullptr; int Cout = 0, CoutTot = 0;
    float* dw = nullptr; float* db = nullptr; int N = 0, H = 0, W = 0, ks = 0;
    const float* x_amax = nullptr; const float* dy_amax = nullptr;
    void* workspace = nullptr; size_t workspace_bytes = 0;
    int x_packed = 0; const float* x_amax2 = nullptr; int seg_channels = 0; int dy_packed = 0;      // *_packed: operand in split storage
    int x_b16 = 0, dy_b16 = 0;                                                                        // *_b16: operand stored as bf16 (single-piece mode)
    float* slabs_out = nullptr; hipStream_t st = nullptr;
};
// conv_wgrad_split.hip: 3x3 weight gradient on the fp16 matrix pipe with two-piece split operands; r.slabs slabs into `slab`
bool wgrad_split_ok(int Cin, int Cout, int N, int H, int W, int ks);
int wgrad_split_splits(int Cin, int Cout, int N, int H, int W, int& tw, int& ct);       // ... and the tile width and channel tile
int wgrad_split(const WgradCall& c, const WgradRoute& r, float* slab, const float* x_amax, const float* dy_amax);

// conv1x1_small.hip: streaming VALU kernels for 1x1 convolutions with 1, 2, 3, 4, 6 or 8 outputs (conv1x1_small_ok says exactly which
// shapes; -2 = output count not instantiated, unreachable behind that check)
bool conv1x1_small_ok(int Cin, int Cout);
int conv1x1_small_fwd(const float* x, int Cin, int CinTot, const float* w, const float* bias, float* y, int Cout, int CoutTot,
                      int N, int H, int W, hipStream_t st, int x_b16 = 0);
int conv1x1_small_bwd_data(const float* dy, int Cout, int CoutTot, const float* w, float* dx, int Cin, int CinTot,
                           int N, int H, int W, int accumulate, hipStream_t st, int dx_b16 = 0);
size_t conv1x1_small_bwd_weight_ws(int Cin, int Cout, int N, int H, int W);
int conv1x1_small_bwd_weight(const float* x, int Cin, int CinTot, const float* dy, int Cout, int CoutTot, float* dw, float* db,
                             int N, int H, int W, void* ws, hipStream_t st, int x_b16 = 0);

// pointwise.hip: what uz_stream_route answers for uz_add_views (op 5), from the file-local predicate uz_add_views dispatches with
int add_views_stream_route(int H, int W, int al_a, int al_y, int al_b);

}  // namespace uz

#define UZ_REQUIRE(cond, ...) do { if (!(cond)) return uz::fail(__VA_ARGS__); } while (0)
