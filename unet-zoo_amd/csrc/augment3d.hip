// Volume augmentation on the device: the work of BratsDataset.__getitem__ (data/bratsDataset.py:34-96) + augment3DImage
// (data/BratsProcessing/augmentation.py:12-104) on ONE volume that is resident in HBM as the HDF5 file stores it, channels last
// [X][Y][Z][C] fp32 with a [X][Y][Z] uint8 label.  The reference makes five passes, four of them a Python loop over the Z slices
// through OpenCV; here every geometric stage that is switched on is one launch, in the reference's order
//   rotate (:44-48)  ->  scale + pad / crop (:51-62)  ->  elastic warp (:65-79)
// and each stage reads the RESULT of the stage before it (the reference resamples a resampled volume: composing the transforms
// would give another image), ping-ponging through two channels-last images in the workspace.  The LAST stage that is on (a plain
// copy when none is) stores straight into the outputs and does there what needs no pass of its own: intensity shift (:82-84),
// flips (:87-91), the random crop (bratsDataset.py:80-86), _toEvaluationOneHot (:125-131) and channels-last -> planar (:88-89).
// All in-plane geometry acts on the plane [X][Y] of one z (rows = X, columns = Y), identically for every z and channel.
//
// One thread per voxel, z fastest: with C == 4 and a 16-byte aligned image a tap is ONE float4, neighbouring threads read
// neighbouring 16 bytes and write neighbouring dwords of every output plane; any other C or alignment takes a scalar path
// (use_vec below is the only predicate; uz_augment_volume_route answers from it).  No atomics: every output element is written
// once by its owner.  OpenCV itself is not in this image: its published rules are restated (tests/_augment3d.py holds the numpy
// twin, DESIGN.md 2b the rules); unlike csrc/augment.hip the elastic stage DOES reproduce the 1/32-pixel quantisation of
// convertMaps(CV_16SC2), from a displacement field that is evaluated in fp64 so that the fp32 cast and the rint decide as numpy's.
//
// Contraction is off for the whole file: every product and sum below rounds as the same expression does in numpy, so the twin's
// fp32 arithmetic is this file's arithmetic and the fp64 field is numpy's bit for bit.  The kernels are bound by memory.
#include "uz_common.h"
#include <math.h>
#pragma clang fp contract(off)

namespace {

enum { ST_COPY = 0, ST_ROT = 1, ST_SCALE = 2, ST_ELASTIC = 3 };

struct VolP {
    const float* src; const uint8_t* lsrc;      // what the stage reads: channels-last image, label (null without masks)
    float* dst; uint8_t* ldst;                  // what a stage that is not the last writes: channels-last image, label
    float* xo; float* ye; uint8_t* yr;          // what the last stage writes: (C, Xc, Yc, Zc) image, (3, Xc, Yc, Zc) maps, (Xc, Yc, Zc) label
    const float* mapx; const float* mapy;       // elastic: fp32 maps [X][Y] (field_k)
    int C, X, Y, Z;
    int Xc, Yc, Zc, ox, oy, oz, flips;
    float cs, sn;                               // rotate
    int sX, sY;                                 // scale: size of the resized plane
    float shift[8];                             // per channel, 0 where the shift is off
};

// where one voxel of a stage's result comes from in the plane it reads: bilinear taps (i0 | i1) x (j0 | j1) with weights fi, fj for
// the image, the single voxel (li, lj) for the label; fill = outside the padded plane of a down-scale
struct Geo { int i0, i1, j0, j1; float fi, fj; int li, lj; bool fill; };

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }
// BORDER_REFLECT fedcba|abcdefgh|hgfedcb: period 2 n, any distance outside
__device__ __forceinline__ int reflecti(int v, int n) {
    const int n2 = 2 * n;
    int m = v % n2;
    if (m < 0) m += n2;
    return m < n ? m : n2 - 1 - m;
}

// rows = X, columns = Y: (x, y) of csrc/augment.hip's rot_coords = (j, i), centre (Y / 2, X / 2)
__device__ __forceinline__ Geo geo_rot(const VolP& p, int i, int j) {
    const float cx = p.Y * 0.5f, cy = p.X * 0.5f, dx = j - cx, dy = i - cy;
    const float sx = p.cs * dx - p.sn * dy + cx;
    const float sy = p.sn * dx + p.cs * dy + cy;
    const float x0 = floorf(sx), y0 = floorf(sy);
    Geo g;
    g.fj = sx - x0; g.fi = sy - y0;
    g.j0 = clampi((int)x0, p.Y); g.j1 = clampi((int)x0 + 1, p.Y);                 // BORDER_REPLICATE
    g.i0 = clampi((int)y0, p.X); g.i1 = clampi((int)y0 + 1, p.X);
    g.lj = clampi((int)floorf(sx + 0.5f), p.Y); g.li = clampi((int)floorf(sy + 0.5f), p.X);
    g.fill = false;
    return g;
}

// one axis of resize(plane, (sX, sY)) + padToSize / cropToSize: o = index in the n-wide result, s = the resized size
__device__ __forceinline__ bool scale_axis(int o, int n, int s, int& t0, int& t1, float& w, int& l) {
    const int u = s < n ? o - (n - s) / 2 : o + (s - n) / 2;
    if (u < 0 || u >= s) { t0 = t1 = l = 0; w = 0.f; return true; }
    const float f = ((float)u + 0.5f) * ((float)n / (float)s) - 0.5f;                // INTER_LINEAR: oracle.augment.resize_image
    const float f0 = floorf(f);
    w = f0 < 0.f ? 0.f : f - f0;
    t0 = clampi((int)f0, n); t1 = clampi(t0 + 1, n);
    const int q = (int)floor((double)u * ((double)n / (double)s));                  // INTER_NEAREST, decided in fp64
    l = q < n - 1 ? q : n - 1;
    return false;
}
__device__ __forceinline__ Geo geo_scale(const VolP& p, int i, int j) {
    Geo g;
    const bool fi = scale_axis(i, p.X, p.sX, g.i0, g.i1, g.fi, g.li);
    const bool fj = scale_axis(j, p.Y, p.sY, g.j0, g.j1, g.fj, g.lj);
    g.fill = fi || fj;
    if (g.fill) g.fi = g.fj = 0.f;              // the fill value itself, whatever the other axis would weigh
    return g;
}

__device__ __forceinline__ Geo geo_elastic(const VolP& p, int i, int j) {
    const float mx = p.mapx[i * p.Y + j], my = p.mapy[i * p.Y + j];
    const int qx = (int)rintf(mx * 32.f), qy = (int)rintf(my * 32.f);                // convertMaps(CV_16SC2): 1/32 pixel, half to even
    Geo g;
    g.j0 = reflecti(qx >> 5, p.Y); g.j1 = reflecti((qx >> 5) + 1, p.Y); g.fj = (float)(qx & 31) * 0.03125f;
    g.i0 = reflecti(qy >> 5, p.X); g.i1 = reflecti((qy >> 5) + 1, p.X); g.fi = (float)(qy & 31) * 0.03125f;
    g.lj = reflecti((int)rintf(mx), p.Y); g.li = reflecti((int)rintf(my), p.X);
    g.fill = false;
    return g;
}

__device__ __forceinline__ float blend(const Geo& g, float v00, float v01, float v10, float v11) {
    return (1.f - g.fi) * ((1.f - g.fj) * v00 + g.fj * v01) + g.fi * ((1.f - g.fj) * v10 + g.fj * v11);
}

template <int STAGE, bool VEC, bool FINAL>
__global__ __launch_bounds__(256) void vol_stage_k(const VolP p) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    int i, j, k, n;
    if (FINAL) {
        n = p.Xc * p.Yc * p.Zc;
        if (o >= n) return;
        const int xy = o / p.Zc;
        k = o - xy * p.Zc + p.oz; i = xy / p.Yc; j = xy - i * p.Yc + p.oy; i += p.ox;        // the crop of the flipped volume
        if (p.flips & 1) i = p.X - 1 - i;
        if (p.flips & 2) j = p.Y - 1 - j;
        if (p.flips & 4) k = p.Z - 1 - k;
    } else {
        n = p.X * p.Y * p.Z;
        if (o >= n) return;
        const int xy = o / p.Z;
        k = o - xy * p.Z; i = xy / p.Y; j = xy - i * p.Y;
    }
    Geo g;
    if (STAGE == ST_ROT) g = geo_rot(p, i, j);
    else if (STAGE == ST_SCALE) g = geo_scale(p, i, j);
    else if (STAGE == ST_ELASTIC) g = geo_elastic(p, i, j);
    else { g.i0 = g.i1 = g.li = i; g.j0 = g.j1 = g.lj = j; g.fi = g.fj = 0.f; g.fill = false; }
    // voxel index (without the channel) of the four taps; a filled voxel reads [0,0,0,:] of the volume as it enters the stage
    const int t00 = g.fill ? 0 : (g.i0 * p.Y + g.j0) * p.Z + k, t01 = g.fill ? 0 : (g.i0 * p.Y + g.j1) * p.Z + k;
    const int t10 = g.fill ? 0 : (g.i1 * p.Y + g.j0) * p.Z + k, t11 = g.fill ? 0 : (g.i1 * p.Y + g.j1) * p.Z + k;
    if (VEC) {
        const float4* s4 = reinterpret_cast<const float4*>(p.src);
        float4 v;
        if (STAGE == ST_COPY) v = s4[t00];
        else {
            const float4 a = s4[t00], b = s4[t01], c = s4[t10], d = s4[t11];
            v.x = blend(g, a.x, b.x, c.x, d.x); v.y = blend(g, a.y, b.y, c.y, d.y);
            v.z = blend(g, a.z, b.z, c.z, d.z); v.w = blend(g, a.w, b.w, c.w, d.w);
        }
        if (FINAL) {
            p.xo[o] = v.x + p.shift[0]; p.xo[n + o] = v.y + p.shift[1];
            p.xo[2 * n + o] = v.z + p.shift[2]; p.xo[3 * n + o] = v.w + p.shift[3];
        } else reinterpret_cast<float4*>(p.dst)[o] = v;
    } else {
        for (int c = 0; c < p.C; ++c) {
            float v;
            if (STAGE == ST_COPY) v = p.src[t00 * p.C + c];
            else v = blend(g, p.src[t00 * p.C + c], p.src[t01 * p.C + c], p.src[t10 * p.C + c], p.src[t11 * p.C + c]);
            if (FINAL) p.xo[c * n + o] = v + p.shift[c];
            else p.dst[o * p.C + c] = v;
        }
    }
    if (p.lsrc) {
        const int l = g.fill ? 0 : (int)p.lsrc[(g.li * p.Y + g.lj) * p.Z + k];
        if (FINAL) {
            if (p.yr) p.yr[o] = (uint8_t)l;
            if (p.ye) {                                                              // _toEvaluationOneHot: three nested maps
                p.ye[o] = l != 0 ? 1.f : 0.f;
                p.ye[n + o] = (l != 0 && l != 2) ? 1.f : 0.f;
                p.ye[2 * n + o] = l == 4 ? 1.f : 0.f;
            }
        } else p.ldst[o] = (uint8_t)l;
    }
}

// ---- the elastic field: resize(3 x 3, (X, Y), INTER_CUBIC) of dx and dy in fp64, then deformation_to_transformation's fp32 cast
struct FieldP { double dx[9], dy[9]; float* mapx; float* mapy; int X, Y; };

__device__ __forceinline__ double sel3(double a, double b, double c, int t) { return t <= 0 ? a : (t == 1 ? b : c); }   // tap clamped to 0..2
__device__ __forceinline__ void cubic_w(double x, double (&w)[4]) {               // A = -0.75
    w[0] = ((-0.75 * (x + 1.0) + 3.75) * (x + 1.0) - 6.0) * (x + 1.0) + 3.0;
    w[1] = ((1.25 * x - 2.25) * x) * x + 1.0;
    w[2] = ((1.25 * (1.0 - x) - 2.25) * (1.0 - x)) * (1.0 - x) + 1.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
}
__device__ __forceinline__ double cubic3(const double (&m)[9], const double (&wi)[4], int fi, const double (&wj)[4], int fj) {
    double h[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        h[r] = ((wj[0] * sel3(m[3 * r], m[3 * r + 1], m[3 * r + 2], fj - 1) + wj[1] * sel3(m[3 * r], m[3 * r + 1], m[3 * r + 2], fj)) +
                wj[2] * sel3(m[3 * r], m[3 * r + 1], m[3 * r + 2], fj + 1)) + wj[3] * sel3(m[3 * r], m[3 * r + 1], m[3 * r + 2], fj + 2 > 2 ? 2 : fj + 2);
    return ((wi[0] * sel3(h[0], h[1], h[2], fi - 1) + wi[1] * sel3(h[0], h[1], h[2], fi)) + wi[2] * sel3(h[0], h[1], h[2], fi + 1)) +
           wi[3] * sel3(h[0], h[1], h[2], fi + 2 > 2 ? 2 : fi + 2);
}
__global__ __launch_bounds__(256) void field_k(const FieldP p) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= p.X * p.Y) return;
    const int i = o / p.Y, j = o - i * p.Y;
    const double ci = ((double)i + 0.5) * (3.0 / (double)p.X) - 0.5, cj = ((double)j + 0.5) * (3.0 / (double)p.Y) - 0.5;
    const double fi = floor(ci), fj = floor(cj);
    double wi[4], wj[4];
    cubic_w(ci - fi, wi);
    cubic_w(cj - fj, wj);
    p.mapx[o] = (float)((double)j + cubic3(p.dx, wi, (int)fi, wj, (int)fj));
    p.mapy[o] = (float)((double)i + cubic3(p.dy, wi, (int)fi, wj, (int)fj));
}

// ---- kernel choice and workspace.  uz_augment_volume and the host-side query uz_augment_volume_route decide through these.
inline bool use_vec(int C, int align_img) { return C == 4 && align_img == 16; }
inline int stage_grid(int nvox) { return uz::ceil_div(nvox, 256); }
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
struct Ws { size_t imgA, imgB, lblA, lblB, mapx, mapy, total; };
inline Ws ws_layout(int C, int X, int Y, int Z) {
    const size_t nv = (size_t)X * Y * Z, img = up256(nv * C * sizeof(float)), lbl = up256(nv), map = up256((size_t)X * Y * sizeof(float));
    Ws w;
    w.imgA = 0; w.imgB = img; w.lblA = 2 * img; w.lblB = 2 * img + lbl; w.mapx = 2 * img + 2 * lbl; w.mapy = w.mapx + map; w.total = w.mapy + map;
    return w;
}
inline const char* sizes_bad(int C, int X, int Y, int Z) {
    if (C < 1 || C > 8) return "1 <= C <= 8";
    if (X < 1 || Y < 1 || Z < 1) return "empty volume";
    if ((double)X * Y * Z * C >= 2147483648.0) return "element count beyond int32";
    return nullptr;
}

template <int STAGE>
int launch_stage(const VolP& p, bool vec, bool final, hipStream_t st) {
    const int g = stage_grid(final ? p.Xc * p.Yc * p.Zc : p.X * p.Y * p.Z);
    if (vec) {
        if (final) hipLaunchKernelGGL((vol_stage_k<STAGE, true, true>), dim3(g), dim3(256), 0, st, p);
        else hipLaunchKernelGGL((vol_stage_k<STAGE, true, false>), dim3(g), dim3(256), 0, st, p);
    } else {
        if (final) hipLaunchKernelGGL((vol_stage_k<STAGE, false, true>), dim3(g), dim3(256), 0, st, p);
        else hipLaunchKernelGGL((vol_stage_k<STAGE, false, false>), dim3(g), dim3(256), 0, st, p);
    }
    return uz::check_launch("vol_stage_k");
}

}  // namespace

extern "C" size_t uz_augment_volume_workspace(int C, int X, int Y, int Z) {
    if (sizes_bad(C, X, Y, Z)) return 0;
    return ws_layout(C, X, Y, Z).total;
}

extern "C" int uz_augment_volume_route(int C, int X, int Y, int Z, int align_img, int* out2) {
    UZ_REQUIRE(out2, "augment_volume_route: two ints to answer into");
    const char* bad = sizes_bad(C, X, Y, Z);
    UZ_REQUIRE(!bad, "augment_volume_route: %s", bad);
    UZ_REQUIRE(align_img == 16 || align_img == 8 || align_img == 4, "augment_volume_route: alignment 16, 8 or 4");
    out2[0] = use_vec(C, align_img) ? 1 : 0;
    out2[1] = stage_grid(X * Y * Z);
    return 0;
}

extern "C" int uz_augment_volume(const float* img, const uint8_t* lbl, int C, int X, int Y, int Z, const double* prm,
                                 int Xc, int Yc, int Zc, void* workspace, float* x_out, float* y_eval, uint8_t* y_raw, void* stream) {
    UZ_REQUIRE(img && prm && workspace && x_out, "augment_volume: null argument (img, prm, workspace, x_out)");
    UZ_REQUIRE(lbl || (!y_eval && !y_raw), "augment_volume: label outputs without a label (lbl null: y_eval and y_raw must be null)");
    const char* bad = sizes_bad(C, X, Y, Z);
    UZ_REQUIRE(!bad, "augment_volume: %s", bad);
    UZ_REQUIRE(uz::align_of(workspace) == 16, "augment_volume: workspace must be 16-byte aligned");
    for (int q = 0; q < UZ_AUG3_NPRM; ++q) UZ_REQUIRE(isfinite(prm[q]) && fabs(prm[q]) <= 1e6, "augment_volume: parameter %d is not a finite value of at most 1e6", q);
    const bool do_rot = prm[0] != 0.0, do_scale = prm[3] != 0.0, do_el = prm[6] != 0.0, do_shift = prm[25] != 0.0;
    const int ox = (int)prm[31], oy = (int)prm[32], oz = (int)prm[33], flips = (int)prm[30];
    UZ_REQUIRE(Xc >= 1 && Yc >= 1 && Zc >= 1 && ox >= 0 && oy >= 0 && oz >= 0 && ox + Xc <= X && oy + Yc <= Y && oz + Zc <= Z,
               "augment_volume: the crop (%d, %d, %d) at (%d, %d, %d) leaves the volume (%d, %d, %d)", Xc, Yc, Zc, ox, oy, oz, X, Y, Z);
    UZ_REQUIRE(flips >= 0 && flips <= 7, "augment_volume: flips is a mask of three bits");
    UZ_REQUIRE(!do_rot || (fabs(prm[1]) <= 1.0 && fabs(prm[2]) <= 1.0), "augment_volume: cos / sin beyond 1");
    UZ_REQUIRE(!do_scale || (prm[4] >= 1.0 && prm[5] >= 1.0), "augment_volume: the scaled size must be at least 1 x 1");
    UZ_REQUIRE(!do_shift || C >= 4, "augment_volume: the intensity shift acts on channels 0..3 (augmentation.py:83), C = %d", C);

    const Ws w = ws_layout(C, X, Y, Z);
    char* base = static_cast<char*>(workspace);
    float* ibuf[2] = {reinterpret_cast<float*>(base + w.imgA), reinterpret_cast<float*>(base + w.imgB)};
    uint8_t* lbuf[2] = {reinterpret_cast<uint8_t*>(base + w.lblA), reinterpret_cast<uint8_t*>(base + w.lblB)};
    hipStream_t st = uz::S(stream);
    const bool vec = use_vec(C, uz::align_of(img));

    VolP p = {};
    p.src = img; p.lsrc = lbl;
    p.xo = x_out; p.ye = y_eval; p.yr = y_raw;
    p.mapx = reinterpret_cast<float*>(base + w.mapx); p.mapy = reinterpret_cast<float*>(base + w.mapy);
    p.C = C; p.X = X; p.Y = Y; p.Z = Z;
    p.Xc = Xc; p.Yc = Yc; p.Zc = Zc; p.ox = ox; p.oy = oy; p.oz = oz; p.flips = flips;
    p.cs = (float)prm[1]; p.sn = (float)prm[2];
    p.sX = (int)prm[4]; p.sY = (int)prm[5];
    for (int c = 0; c < 4; ++c) p.shift[c] = do_shift ? (float)prm[26 + c] : 0.f;

    if (do_el) {
        FieldP f;
        for (int q = 0; q < 9; ++q) { f.dx[q] = prm[7 + q]; f.dy[q] = prm[16 + q]; }
        f.mapx = reinterpret_cast<float*>(base + w.mapx); f.mapy = reinterpret_cast<float*>(base + w.mapy); f.X = X; f.Y = Y;
        hipLaunchKernelGGL(field_k, dim3(uz::ceil_div(X * Y, 256)), dim3(256), 0, st, f);
        if (int rc = uz::check_launch("field_k")) return rc;
    }
    const int stages[3] = {do_rot ? ST_ROT : -1, do_scale ? ST_SCALE : -1, do_el ? ST_ELASTIC : -1};
    int last = -1, nb = 0;
    for (int s = 0; s < 3; ++s) if (stages[s] >= 0) last = s;
    if (last < 0) return launch_stage<ST_COPY>(p, vec, true, st);
    for (int s = 0; s <= last; ++s) {
        if (stages[s] < 0) continue;
        const bool final = s == last;
        p.dst = ibuf[nb]; p.ldst = lbuf[nb];
        int rc;                                     // one path for every stage of a call (the workspace images are 256-byte aligned)
        if (stages[s] == ST_ROT) rc = launch_stage<ST_ROT>(p, vec, final, st);
        else if (stages[s] == ST_SCALE) rc = launch_stage<ST_SCALE>(p, vec, final, st);
        else rc = launch_stage<ST_ELASTIC>(p, vec, final, st);
        if (rc) return rc;
        p.src = ibuf[nb]; if (lbl) p.lsrc = lbuf[nb];
        nb ^= 1;
    }
    return 0;
}
