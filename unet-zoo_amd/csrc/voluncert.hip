// Sample uncertainty of label volumes on the device (uz_api.h "volume uncertainty"): the vote table T[r][c][d][t] of S sampled label
// volumes, a decision volume and a reference, and from it the filtered Dice / filtered true-positive / true-negative curves of the BraTS
// uncertainty task, their areas, and ECE / MCE / Brier with one bin per vote count.
//
// Table pass: one streaming pass over S + 2 bytes per voxel (+ R bytes with votes).
//   membership  two 256-entry tables in LDS, built per workgroup: byte r of lutP[v] is 1 when the value v is in pred_sets[r] (lutR: ref_sets).
//               A voxel's votes for all R regions are then ONE 64-bit sum of S table entries, byte r = c (S <= 255: no byte overflows).
//   background  a 32-bit word of four voxels that is 0 adds nothing when no set holds the value 0, so it is skipped without a table
//               read; a voxel with c = d = t = 0 in every region is counted in a register.  A wave of background touches LDS only for
//               its R adds behind the loop.
//   histogram   uint32 region tables in LDS, LDS atomics; the bin (0, 0, 0) of a region never goes through them.
//   output      every workgroup stores its whole table, zeros included, to its own slice: no global atomics, no cleared memory.
// VB = bytes (= voxels) a thread reads per row and step: 16, 4 (the wide forms) or 1 (the scalar form, any address).  The P % VB voxels
// behind the last whole step are taken by workgroup 0, one voxel per thread.
// Finish: one workgroup per region sums the slices (int64), then a few threads form levels, curves, areas and calibration.
#include "uz_common.h"
#include <algorithm>

namespace {

constexpr int TB = 256;             // threads of the table pass
constexpr int CAP = 1024;           // workgroups of the table pass at the most: four per CU; the grid-stride loop covers the rest
constexpr int FT = 1024;            // threads of the finish
constexpr int MAXB = (UZ_VOL_UNC_MAX_SAMPLES + 1) * 4;       // bins of one region at the most

typedef unsigned long long u64;

// the VB bytes at p as VB / 4 words (VB = 1: the byte in the low bits of one word)
template <int VB>
__device__ __forceinline__ void load_row(const uint8_t* __restrict__ p, uint32_t (&w)[(VB + 3) / 4]) {
    if constexpr (VB == 16) { const uint4 v = *reinterpret_cast<const uint4*>(p); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
    else if constexpr (VB == 4) w[0] = *reinterpret_cast<const uint32_t*>(p);
    else w[0] = *p;
}
template <int VB>
__device__ __forceinline__ void store_row(uint8_t* __restrict__ p, const uint32_t (&w)[(VB + 3) / 4]) {
    if constexpr (VB == 16) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    else if constexpr (VB == 4) *reinterpret_cast<uint32_t*>(p) = w[0];
    else *p = (uint8_t)w[0];
}

// acc[k] += lut[byte k of the words]; a zero word is skipped when the value 0 is in no set (zero_in = false)
template <int VB>
__device__ __forceinline__ void add_row(const uint32_t (&w)[(VB + 3) / 4], const u64* __restrict__ lut, bool zero_in, u64 (&acc)[VB]) {
#pragma unroll
    for (int i = 0; i < (VB + 3) / 4; ++i) {
        if (w[i] != 0u || zero_in) {
#pragma unroll
            for (int k = 0; k < (VB < 4 ? VB : 4); ++k) acc[4 * i + k] += lut[(w[i] >> (8 * k)) & 255u];
        }
    }
}

// one voxel with its votes c, decision bits d and reference bits t (byte r = region r) into the tables
__device__ __forceinline__ void bin_voxel(u64 c, u64 d, u64 t, int R, int nb, unsigned* __restrict__ tab, unsigned& bg, unsigned (&z)[UZ_VOL_MAX_REGIONS]) {
    if ((c | d | t) == 0ull) { ++bg; return; }
#pragma unroll
    for (int r = 0; r < UZ_VOL_MAX_REGIONS; ++r) {
        if (r < R) {
            const unsigned cr = (unsigned)(c >> (8 * r)) & 255u, dr = (unsigned)(d >> (8 * r)) & 1u, tr = (unsigned)(t >> (8 * r)) & 1u;
            if ((cr | dr | tr) == 0u) ++z[r];
            else atomicAdd(&tab[r * nb + (int)(cr * 4u + dr * 2u + tr)], 1u);
        }
    }
}

template <int VB>
__device__ __forceinline__ void step(const uint8_t* __restrict__ samples, int S, const uint8_t* __restrict__ decision, const uint8_t* __restrict__ ref,
                                     int R, size_t P, size_t base, const u64* __restrict__ lutP, const u64* __restrict__ lutR, bool zp, bool zr,
                                     int nb, unsigned* __restrict__ tab, unsigned& bg, unsigned (&z)[UZ_VOL_MAX_REGIONS], uint8_t* __restrict__ votes) {
    constexpr int NW = (VB + 3) / 4;
    u64 c[VB], d[VB], t[VB];
#pragma unroll
    for (int k = 0; k < VB; ++k) c[k] = d[k] = t[k] = 0ull;
    uint32_t wd[NW], wt[NW];
    load_row<VB>(decision + base, wd);
    load_row<VB>(ref + base, wt);
#pragma unroll 4
    for (int s = 0; s < S; ++s) {
        uint32_t w[NW];
        load_row<VB>(samples + (size_t)s * P + base, w);
        add_row<VB>(w, lutP, zp, c);
    }
    add_row<VB>(wd, lutP, zp, d);
    add_row<VB>(wt, lutR, zr, t);
#pragma unroll
    for (int k = 0; k < VB; ++k) bin_voxel(c[k], d[k], t[k], R, nb, tab, bg, z);
    if (votes) {
#pragma unroll
        for (int r = 0; r < UZ_VOL_MAX_REGIONS; ++r) {
            if (r < R) {
                uint32_t w[NW];
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    w[i] = 0u;
#pragma unroll
                    for (int k = 0; k < (VB < 4 ? VB : 4); ++k) w[i] |= ((uint32_t)(c[4 * i + k] >> (8 * r)) & 255u) << (8 * k);
                }
                store_row<VB>(votes + (size_t)r * P + base, w);
            }
        }
    }
}

template <int VB>
__global__ __launch_bounds__(TB) void table_k(const uint8_t* __restrict__ samples, int S, const uint8_t* __restrict__ decision,
                                              const uint8_t* __restrict__ ref, uz::RegionSets sets, int R, int P_, uint32_t* __restrict__ slices,
                                              uint8_t* __restrict__ votes) {
    extern __shared__ __align__(16) u64 lds[];                          // [256] lutP, [256] lutR, then R * nb uint32
    u64* lutP = lds;
    u64* lutR = lds + 256;
    unsigned* tab = reinterpret_cast<unsigned*>(lds + 512);
    const int nb = (S + 1) * 4, nbr = R * nb;
    const size_t P = (size_t)P_;
    {
        const unsigned v = threadIdx.x;                                  // TB == 256: one value per thread
        u64 a = 0ull, b = 0ull;
        if (v < 32u) {
            for (int r = 0; r < R; ++r) {
                a |= (u64)((sets.p[r] >> v) & 1u) << (8 * r);
                b |= (u64)((sets.r[r] >> v) & 1u) << (8 * r);
            }
        }
        lutP[v] = a; lutR[v] = b;
    }
    for (int k = threadIdx.x; k < nbr; k += TB) tab[k] = 0u;
    __syncthreads();
    const bool zp = lutP[0] != 0ull, zr = lutR[0] != 0ull;               // the value 0 is in some set: a zero word counts
    unsigned bg = 0u, z[UZ_VOL_MAX_REGIONS];
#pragma unroll
    for (int r = 0; r < UZ_VOL_MAX_REGIONS; ++r) z[r] = 0u;
    const size_t units = P / VB;
    for (size_t u = (size_t)blockIdx.x * TB + threadIdx.x; u < units; u += (size_t)gridDim.x * TB)
        step<VB>(samples, S, decision, ref, R, P, u * VB, lutP, lutR, zp, zr, nb, tab, bg, z, votes);
    if constexpr (VB > 1) {                                              // the tail: fewer than VB voxels, one per thread
        const size_t q = units * VB + threadIdx.x;
        if (blockIdx.x == 0 && q < P) step<1>(samples, S, decision, ref, R, P, q, lutP, lutR, zp, zr, nb, tab, bg, z, votes);
    }
#pragma unroll
    for (int r = 0; r < UZ_VOL_MAX_REGIONS; ++r) {
        if (r < R) {
            const unsigned v = uz::wave_sum(z[r] + bg);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(&tab[r * nb], v);
        }
    }
    __syncthreads();
    uint32_t* mine = slices + (size_t)blockIdx.x * nbr;
    for (int k = threadIdx.x; k < nbr; k += TB) mine[k] = tab[k];
}

// ------------------------------------------------------------------------------------------------ finish
// workgroup = region.  Everything behind the sum is a few hundred operations: single threads walk the S + 1 levels.
__global__ __launch_bounds__(FT) void unc_finish_k(const uint32_t* __restrict__ slices, int G, int R, int S, long long P,
                                                   long long* __restrict__ table, long long* __restrict__ levels, double* __restrict__ curves,
                                                   double* __restrict__ auc, double* __restrict__ calibration) {
    __shared__ u64 tab[MAXB];
    __shared__ long long lev[MAXB];
    __shared__ double cur[3][UZ_VOL_UNC_MAX_SAMPLES + 1];
    __shared__ double area[3];
    const int r = blockIdx.x, nb = (S + 1) * 4, tid = threadIdx.x;
    for (int k = tid; k < nb; k += FT) tab[k] = 0ull;
    __syncthreads();
    {
        // the four bins (d, t) of one vote count are one 16-byte load (a slice is R * nb * 4 bytes, a multiple of 16, on a 16-byte
        // aligned workspace); S + 1 <= 256 such quads, FT / (S + 1) >= 4 threads share the slices of each
        const int nq = S + 1, stripes = FT / nq;
        if (tid < stripes * nq) {
            const int q = tid % nq;
            const uint4* src = reinterpret_cast<const uint4*>(slices + (size_t)r * nb) + q;
            const size_t pitch = (size_t)R * nq;                         // uint4s from one slice to the next
            u64 a0 = 0ull, a1 = 0ull, a2 = 0ull, a3 = 0ull;
#pragma unroll 8
            for (int sl = tid / nq; sl < G; sl += stripes) {
                const uint4 v = src[(size_t)sl * pitch];
                a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
            }
            atomicAdd(&tab[4 * q], a0); atomicAdd(&tab[4 * q + 1], a1); atomicAdd(&tab[4 * q + 2], a2); atomicAdd(&tab[4 * q + 3], a3);
        }
    }
    __syncthreads();
    if (tid < nb) table[(size_t)r * nb + tid] = (long long)tab[tid];
    if (tid < 4) {                                                       // 0 tp, 1 fp: c from S down; 2 fn, 3 tn: c from 0 up
        const int dt = tid == 0 ? 3 : tid == 1 ? 2 : tid == 2 ? 1 : 0;
        long long run = 0;
        for (int j = 0; j <= S; ++j) {
            run += (long long)tab[(tid < 2 ? S - j : j) * 4 + dt];
            lev[j * 4 + tid] = run;
        }
    }
    __syncthreads();
    if (tid < nb) levels[(size_t)r * nb + tid] = lev[tid];
    if (tid <= S) {
        const long long tp = lev[tid * 4], fp = lev[tid * 4 + 1], fn = lev[tid * 4 + 2], tn = lev[tid * 4 + 3];
        const long long tpS = lev[S * 4], tnS = lev[S * 4 + 3], den = 2 * tp + fp + fn;
        const double dice = den == 0 ? 1.0 : (double)(2 * tp) / (double)den;
        const double ftp = tpS == 0 ? 0.0 : (double)(tpS - tp) / (double)tpS;
        const double ftn = tnS == 0 ? 0.0 : (double)(tnS - tn) / (double)tnS;
        double* o = curves + ((size_t)r * (S + 1) + tid) * 3;
        o[0] = dice; o[1] = ftp; o[2] = ftn;
        cur[0][tid] = dice; cur[1][tid] = ftp; cur[2][tid] = ftn;
    }
    __syncthreads();
    if (tid < 3) {                                                       // trapezoids on the grid j / S, in the order of j
        double a = 0.0;
        for (int j = 0; j < S; ++j) a += (cur[tid][j] + cur[tid][j + 1]) * 0.5;
        a /= (double)S;
        area[tid] = a;
        auc[r * 4 + tid] = a;
    }
    if (tid == 64) {                                                     // another wave: reliability with one bin per vote count
        long long ece = 0, brier = 0;
        double mce = 0.0;
        for (int c = 0; c <= S; ++c) {
            const long long pos = (long long)(tab[c * 4 + 1] + tab[c * 4 + 3]), n = pos + (long long)(tab[c * 4] + tab[c * 4 + 2]);
            long long gap = (long long)S * pos - (long long)c * n;
            gap = gap < 0 ? -gap : gap;
            ece += gap;
            brier += pos * (long long)((S - c) * (S - c)) + (n - pos) * (long long)(c * c);
            if (n > 0) mce = fmax(mce, (double)gap / (double)((long long)S * n));
        }
        calibration[r * 3] = (double)ece / (double)((long long)S * P);
        calibration[r * 3 + 1] = mce;
        calibration[r * 3 + 2] = (double)brier / (double)((long long)S * S * P);
    }
    __syncthreads();
    if (tid == 0) auc[r * 4 + 3] = (area[0] + (1.0 - area[1]) + (1.0 - area[2])) / 3.0;
}

// ------------------------------------------------------------------------------------------------ host
const char* sizes_bad(int S, int R, int D, int H, int W) {
    if (S < 1 || S > UZ_VOL_UNC_MAX_SAMPLES) return "1 <= S <= 255 samples";
    if (R < 1 || R > UZ_VOL_MAX_REGIONS) return "1 <= R <= 8 regions";
    if (D < 1 || H < 1 || W < 1) return "empty axis";
    // the product in steps, each below 2^31 * 2^31
    const long long dh = (long long)D * H;
    if (dh >= (1LL << 31) || dh * W >= (1LL << 31) || dh * W * S >= (1LL << 31)) return "S*D*H*W must stay below 2^31";
    return nullptr;
}
inline int bins(int S, int R) { return R * (S + 1) * 4; }
// n rows of P bytes from address a on, every one aligned to vb bytes
inline bool rows_aligned(uintptr_t a, int n, long long P, int vb) { return a % vb == 0 && (n == 1 || P % vb == 0); }
// bytes per thread and row: 16 or 4 the wide forms, 1 the scalar form.  votes = 0: none (constrains nothing)
inline int vec_bytes(uintptr_t samples, int S, uintptr_t decision, uintptr_t ref, uintptr_t votes, int R, long long P) {
    for (int vb = 16; vb > 1; vb >>= 2)
        if (P >= vb && rows_aligned(samples, S, P, vb) && rows_aligned(decision, 1, P, vb) && rows_aligned(ref, 1, P, vb) && (votes == 0 || rows_aligned(votes, R, P, vb))) return vb;
    return 1;
}
inline int sweeps_wg(long long P, int vb) { return uz::sweep_grid(P / vb, TB); }               // workgroups that would cover P in one sweep
inline int table_grid(long long P, int vb) { return uz::sweep_grid(P / vb, TB, CAP); }

template <int VB>
int launch_table(const uint8_t* samples, int S, const uint8_t* decision, const uint8_t* ref, const uz::RegionSets& s, int R, int P, int G, uint32_t* slices,
                 uint8_t* votes, hipStream_t st) {
    const size_t lds = 512 * sizeof(u64) + (size_t)bins(S, R) * sizeof(uint32_t);
    hipLaunchKernelGGL(table_k<VB>, dim3(G), dim3(TB), lds, st, samples, S, decision, ref, s, R, P, slices, votes);
    return uz::check_launch("table_k");
}

}  // namespace

extern "C" size_t uz_vol_uncertainty_workspace(int S, int R, int D, int H, int W) {
    if (sizes_bad(S, R, D, H, W)) return 0;
    return uz::up16((size_t)table_grid((long long)D * H * W, 1) * bins(S, R) * sizeof(uint32_t));       // the scalar form's grid is the largest
}

extern "C" int uz_vol_uncertainty_route(int S, int R, int D, int H, int W, int align, int* out3) {
    UZ_REQUIRE(out3, "vol_uncertainty_route: three ints to answer into");
    const char* bad = sizes_bad(S, R, D, H, W);
    UZ_REQUIRE(!bad, "vol_uncertainty_route: %s", bad);
    UZ_REQUIRE(align == 1 || align == 2 || align == 4 || align == 8 || align == 16, "vol_uncertainty_route: align is 1, 2, 4, 8 or 16");
    const long long P = (long long)D * H * W;
    const uintptr_t a = (uintptr_t)align;                               // an address with exactly this alignment
    const int vb = vec_bytes(a, S, a, a, a, R, P);
    out3[0] = vb > 1 ? 1 : 0;
    out3[1] = table_grid(P, vb);
    out3[2] = sweeps_wg(P, vb) > CAP ? 1 : 0;
    return 0;
}

extern "C" int uz_vol_uncertainty(const uint8_t* samples, int S, const uint8_t* decision, const uint32_t* pred_sets,
                                  const uint8_t* ref, const uint32_t* ref_sets, int R, int D, int H, int W,
                                  void* workspace, int64_t* table, int64_t* levels, double* curves, double* auc,
                                  double* calibration, uint8_t* votes, void* stream) {
    UZ_REQUIRE(samples && decision && pred_sets && ref && ref_sets && workspace && table && levels && curves && auc && calibration,
               "vol_uncertainty: null argument (samples, decision, pred_sets, ref, ref_sets, workspace, table, levels, curves, auc, calibration)");
    const char* bad = sizes_bad(S, R, D, H, W);
    UZ_REQUIRE(!bad, "vol_uncertainty: %s", bad);
    UZ_REQUIRE(uz::align_of(workspace) == 16, "vol_uncertainty: workspace must be 16-byte aligned");
    UZ_REQUIRE(((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(levels) | reinterpret_cast<uintptr_t>(curves) |
                 reinterpret_cast<uintptr_t>(auc) | reinterpret_cast<uintptr_t>(calibration)) & 7) == 0,
               "vol_uncertainty: table, levels, curves, auc and calibration must be 8-byte aligned");
    hipStream_t st = uz::S(stream);
    const int P = D * H * W;
    const uz::RegionSets s = uz::region_sets(pred_sets, ref_sets, R);
    const int vb = vec_bytes(reinterpret_cast<uintptr_t>(samples), S, reinterpret_cast<uintptr_t>(decision), reinterpret_cast<uintptr_t>(ref),
                             reinterpret_cast<uintptr_t>(votes), R, P);
    const int G = table_grid(P, vb);                                     // <= the scalar form's grid, which sized the workspace
    uint32_t* slices = static_cast<uint32_t*>(workspace);
    int rc = vb == 16 ? launch_table<16>(samples, S, decision, ref, s, R, P, G, slices, votes, st)
           : vb == 4  ? launch_table<4>(samples, S, decision, ref, s, R, P, G, slices, votes, st)
                      : launch_table<1>(samples, S, decision, ref, s, R, P, G, slices, votes, st);
    if (rc) return rc;
    hipLaunchKernelGGL(unc_finish_k, dim3(R), dim3(FT), 0, st, slices, G, R, S, (long long)P, reinterpret_cast<long long*>(table),
                       reinterpret_cast<long long*>(levels), curves, auc, calibration);
    return uz::check_launch("unc_finish_k");
}
