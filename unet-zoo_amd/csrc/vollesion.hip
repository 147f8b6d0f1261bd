// Lesion-wise scores of label volumes on the device (uz_api.h "lesion-wise scores"): reference lesions are the 26-connected components
// of the reference region dilated `dilation` times with the 18-neighbour structure, each is matched to the predicted 26-connected
// components that reach it, and every missed lesion and every false-positive component enters the mean Dice as a 0.
//
// Per region r, the regions one after the other through one workspace (as uz_vol_keep_components runs its sets):
//   reference side, once (it does not depend on the row)
//     dilate   uz_vol_morph(ref, set, connectivity 2, dilation) -> dk, a 0 / 1 volume                                  (volmorph.hip)
//     label    uz_vol_label_components_ex(dk, connectivity 3) -> lg, canonical labels: a root voxel v carries lg[v] == v + 1 (volcomp.hip)
//     rank     compact lesion indices in the order of the root voxels, which is the order of the canonical labels: a count of the roots
//              per 256 voxels, one workgroup that turns the counts into offsets, and a pass that gives every root offset + its rank
//              among the roots of its 256 (a ballot per wave, the waves in order); the rank is parked at the root, in the sizes volume
//     index    lg[v] = 1 + min(rank of v's root, max_lesions), 0 outside dk; a voxel of G adds 1 to gt_vol[index]   (integer atomics)
//   prediction side, all N rows per launch
//     label    uz_vol_label_components_ex(pred, connectivity 3) -> lp, sp: canonical labels and component sizes
//     links    max_links rounds.  offer: every voxel with lp > 0 and lg > 0 offers its lesion index to its component's root with an
//              integer fetch_min, if the index is greater than the one the root settled in the round before.  settle: the root's own
//              thread adds the component's size to pred_vol[link], remembers the link and clears the offer.  The first offer pass
//              also counts inter (a predicted voxel inside G); the first settle pass counts the components, and those without any
//              offer - no voxel in dk - of at least min_pred_voxels voxels as false positives.  One more offer pass, and the roots
//              that would still take a link are counted: links beyond max_links.
//              The index max_lesions stands for every lesion beyond the table: it is a link like any other and adds to no sum.
//   finish     one workgroup per row: the counts, the per-lesion table, and the four scores, the Dice sum serially in ascending g in fp64.
// Integer atomics only, and every sum is of integers: exact, independent of order, bit-equal on repetition.
#include "uz_common.h"
#include <float.h>

namespace {

constexpr int VOX_GRID_MAX = 1 << 18;
#define UZ_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
constexpr int NO_LINK = INT_MAX;

// ------------------------------------------------------------------------------------------------ rank of the roots
__global__ __launch_bounds__(256) void les_count_k(const int* __restrict__ lg, int P, int* __restrict__ blk) {
    __shared__ int sm[4];
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool root = v < P && lg[v] == (int)v + 1;
    const unsigned long long m = __ballot(root);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

// blk[0 .. nb) -> exclusive offsets in place, blk[nb] = the total: one workgroup, every thread a contiguous stretch
__global__ __launch_bounds__(256) void les_scan_k(int* __restrict__ blk, int nb) {
    __shared__ int sm[256];
    const int per = (nb + 255) / 256;
    const int lo = min(threadIdx.x * per, nb), hi = min(lo + per, nb);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += blk[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int t = sm[i]; sm[i] = run; run += t; }
        blk[nb] = run;
    }
    __syncthreads();
    int run = sm[threadIdx.x];
    for (int i = lo; i < hi; ++i) { const int t = blk[i]; blk[i] = run; run += t; }
}

__global__ __launch_bounds__(256) void les_rank_k(const int* __restrict__ lg, int P, const int* __restrict__ blk, int* __restrict__ rank) {
    __shared__ int sm[4];
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool root = v < P && lg[v] == (int)v + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(root);
    if (lane == 0) sm[wave] = __popcll(m);
    __syncthreads();
    if (root) {
        int before = blk[blockIdx.x];
        for (int w = 0; w < wave; ++w) before += sm[w];
        rank[v] = before + __popcll(m & ((1ull << lane) - 1ull));
    }
}

// lg: canonical label -> 1 + compact index (capped at max_lesions); gt_vol from the voxels of G
__global__ __launch_bounds__(256) void les_index_k(const uint8_t* __restrict__ ref, uint32_t rset, int P, int max_lesions, int* __restrict__ lg,
                                                   const int* __restrict__ rank, int* __restrict__ gt) {
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < P; v += (long long)gridDim.x * 256) {
        const int l = lg[v];
        if (!l) continue;
        const int g = min(rank[l - 1], max_lesions);
        lg[v] = g + 1;                                                     // nobody reads lg of another voxel here: rank[] holds what they need
        if (g < max_lesions && uz::in_set(ref[v], rset)) atomicAdd(&gt[g], 1);
    }
}

// ------------------------------------------------------------------------------------------------ links
__global__ __launch_bounds__(256) void les_init_k(long long T, int* __restrict__ settled, int* __restrict__ cur) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < T; q += (long long)gridDim.x * 256) { settled[q] = -1; cur[q] = NO_LINK; }
}

template <bool FIRST> __global__ __launch_bounds__(256) void les_offer_k(const int* __restrict__ lp, const int* __restrict__ lg, const uint8_t* __restrict__ ref, uint32_t rset,
                                                                         long long T, int P, int max_lesions, const int* __restrict__ settled, int* __restrict__ cur,
                                                                         int* __restrict__ inter) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < T; q += (long long)gridDim.x * 256) {
        const int l = lp[q];
        if (!l) continue;
        const int n = (int)(q / P);
        const int v = (int)(q - (long long)n * P);
        const int gi = lg[v];
        if (!gi) continue;
        const int g = gi - 1;
        const long long root = (long long)n * P + (l - 1);
        if (g > settled[root] && __hip_atomic_load(&cur[root], UZ_RLX_AGENT) > g) __hip_atomic_fetch_min(&cur[root], g, UZ_RLX_AGENT);
        if (FIRST && g < max_lesions && uz::in_set(ref[v], rset)) atomicAdd(&inter[(long long)n * max_lesions + g], 1);
    }
}

// ctr (N, 4) = {components, false positives, roots that would take another link, unused}
template <bool FIRST> __global__ __launch_bounds__(256) void les_settle_k(const int* __restrict__ lp, const int* __restrict__ sp, long long T, int P, int max_lesions,
                                                                          int min_pred_voxels, int* __restrict__ settled, int* __restrict__ cur,
                                                                          int* __restrict__ pred_vol, int* __restrict__ ctr) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < T; q += (long long)gridDim.x * 256) {
        const int n = (int)(q / P);
        if (lp[q] != (int)(q - (long long)n * P) + 1) continue;            // roots only
        const int c = cur[q], size = sp[q];
        if (FIRST) {
            atomicAdd(&ctr[n * 4 + 0], 1);
            if (c == NO_LINK && size >= min_pred_voxels) atomicAdd(&ctr[n * 4 + 1], 1);
        }
        if (c == NO_LINK) continue;
        if (c < max_lesions) atomicAdd(&pred_vol[(long long)n * max_lesions + c], size);
        settled[q] = c;
        cur[q] = NO_LINK;
    }
}

__global__ __launch_bounds__(256) void les_left_k(const int* __restrict__ lp, long long T, int P, const int* __restrict__ cur, int* __restrict__ ctr) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < T; q += (long long)gridDim.x * 256) {
        const int n = (int)(q / P);
        if (lp[q] == (int)(q - (long long)n * P) + 1 && cur[q] != NO_LINK) atomicAdd(&ctr[n * 4 + 2], 1);
    }
}

// ------------------------------------------------------------------------------------------------ finish
__global__ __launch_bounds__(256) void les_finish_k(const int* __restrict__ n_ref_p, const int* __restrict__ gt, const int* __restrict__ inter, const int* __restrict__ pred_vol,
                                                    const int* __restrict__ ctr, int r, int R, int max_lesions, int min_ref_voxels,
                                                    int64_t* __restrict__ counts, int64_t* __restrict__ lesions, double* __restrict__ scores) {
    const int n = blockIdx.x;
    const int n_ref = *n_ref_p, n_tab = min(n_ref, max_lesions);
    const int* in = inter + (long long)n * max_lesions;
    const int* pv = pred_vol + (long long)n * max_lesions;
    if (lesions) {
        int64_t* les = lesions + ((long long)n * R + r) * max_lesions * 3;
        for (int g = threadIdx.x; g < max_lesions; g += 256) {
            const bool has = g < n_tab;
            les[g * 3 + 0] = has ? gt[g] : 0;
            les[g * 3 + 1] = has ? in[g] : 0;
            les[g * 3 + 2] = has ? pv[g] : 0;
        }
    }
    if (threadIdx.x != 0) return;
    long long n_kept = 0, n_tp = 0;
    double sum = 0.0;
    for (int g = 0; g < n_tab; ++g) {                                      // ascending g, serially: the order is part of the contract
        if (gt[g] < min_ref_voxels) continue;
        ++n_kept;
        if (pv[g] == 0) continue;                                          // a missed lesion: Dice 0
        ++n_tp;
        sum += (double)(2LL * in[g]) / (double)((long long)gt[g] + pv[g]);
    }
    const long long n_fn = n_kept - n_tp, n_pred = ctr[n * 4 + 0], n_fp = ctr[n * 4 + 1], over_links = ctr[n * 4 + 2];
    const long long over_lesions = n_ref - n_tab;
    int64_t* c = counts + ((long long)n * R + r) * 8;
    c[0] = n_ref; c[1] = n_kept; c[2] = n_tp; c[3] = n_fn; c[4] = n_fp; c[5] = n_pred; c[6] = over_lesions; c[7] = over_links;
    double* s = scores + ((long long)n * R + r) * 4;
    if (over_lesions || over_links) {
        const double nan = __longlong_as_double(0x7FF8000000000000LL);
        s[0] = s[1] = s[2] = s[3] = nan;
        return;
    }
    s[0] = n_kept + n_fp ? sum / (double)(n_kept + n_fp) : 1.0;
    s[1] = n_kept ? (double)n_tp / (double)n_kept : 1.0;
    s[2] = n_tp + n_fp ? (double)n_tp / (double)(n_tp + n_fp) : 1.0;
    s[3] = 2 * n_tp + n_fn + n_fp ? (double)(2 * n_tp) / (double)(2 * n_tp + n_fn + n_fp) : 1.0;
}

// ------------------------------------------------------------------------------------------------ lesion-wise HD95 (uz_api.h rule 6)
// Lists of at most MB = max_border entries: refA, the border voxels of G grouped by lesion (seg[g] .. seg[g + 1], seg[ML] the total);
// per row ent, the (border voxel of P, lesion) entries as the link rounds append them, sq, the same sorted by lesion (eo[n][g] ..
// eo[n][g + 1]), dB, the squared distance of every sorted entry to its lesion's border, and dminA, the squared distance of every
// voxel of refA to the row's entries of its lesion.  Everything an overflowing list would have held is counted and dropped.
constexpr int HD_Q = 256;         // queries of one workgroup of the pair kernel, one per thread
constexpr int HD_T = 512;         // seeds of one LDS tile
constexpr int HD_NONE = INT_MAX;  // no distance yet

// the rule of volscore.hip's border_at: a voxel of {label in set} with a face neighbour outside the set or outside the volume
__device__ __forceinline__ bool hd_border_at(const uint8_t* __restrict__ lab, uint32_t set, int v, int D, int H, int W) {
    if (!uz::in_set(lab[v], set)) return false;
    const int hw = H * W, d = v / hw, rem = v - d * hw, h = rem / W, w = rem - h * W;
    if (d == 0 || d == D - 1 || h == 0 || h == H - 1 || w == 0 || w == W - 1) return true;
    return !(uz::in_set(lab[v - hw], set) && uz::in_set(lab[v + hw], set) && uz::in_set(lab[v - W], set) && uz::in_set(lab[v + W], set) &&
             uz::in_set(lab[v - 1], set) && uz::in_set(lab[v + 1], set));
}
__device__ __forceinline__ int4 hd_coords(int v, int H, int W) {
    const int hw = H * W, d = v / hw, rem = v - d * hw, h = rem / W;
    return make_int4(rem - h * W, h, d, 0);
}
// coordinates are below 2^15 (D^2 + H^2 + W^2 <= 2^30), so every difference fits the 24-bit multiplier
__device__ __forceinline__ int hd_dist(const int4 a, const int4 b) {
    const int dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return __mul24(dx, dx) + __mul24(dy, dy) + __mul24(dz, dz);
}

__global__ __launch_bounds__(256) void hd_fill_k(long long n, int* __restrict__ p) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) p[i] = HD_NONE;
}

// SCATTER = false: seg[g] += 1 per border voxel of lesion g (les_scan_k then turns the counts into offsets); true: the voxel goes into its segment
template <bool SCATTER> __global__ __launch_bounds__(256) void hd_ref_k(const uint8_t* __restrict__ ref, uint32_t rset, const int* __restrict__ lg, int P, int D, int H, int W,
                                                                      int max_lesions, int max_border, int* __restrict__ seg, int* __restrict__ fill, int* __restrict__ refA) {
    for (long long vv = (long long)blockIdx.x * 256 + threadIdx.x; vv < P; vv += (long long)gridDim.x * 256) {
        const int v = (int)vv, gi = lg[v];
        if (!gi || gi > max_lesions || !hd_border_at(ref, rset, v, D, H, W)) continue;
        if (!SCATTER) { atomicAdd(&seg[gi - 1], 1); continue; }
        const int pos = seg[gi - 1] + atomicAdd(&fill[gi - 1], 1);
        if (pos < max_border) refA[pos] = v;
    }
}

// between offer k and settle k: cur[root] is the link the component settles in this round
__global__ __launch_bounds__(256) void hd_entries_k(const uint8_t* __restrict__ pred, uint32_t pset, const int* __restrict__ lp, const int* __restrict__ cur, long long T, int P,
                                                    int D, int H, int W, int max_lesions, int max_border, unsigned long long* __restrict__ ecur, int2* __restrict__ ent) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < T; q += (long long)gridDim.x * 256) {
        const int l = lp[q];
        if (!l) continue;
        const int n = (int)(q / P);
        const int v = (int)(q - (long long)n * P);
        const int g = cur[(long long)n * P + (l - 1)];
        if (g >= max_lesions || !hd_border_at(pred + (long long)n * P, pset, v, D, H, W)) continue;        // NO_LINK, and the lesions beyond the table
        const unsigned long long pos = atomicAdd(&ecur[n], 1ull);
        if (pos < (unsigned long long)max_border) ent[(long long)n * max_border + (long long)pos] = make_int2(v, g);
    }
}

// bpr workgroups per row.  SCATTER = false: eo[n][g] += 1 per stored entry; true: the entry's voxel goes into its lesion's stretch of sq
template <bool SCATTER> __global__ __launch_bounds__(256) void hd_sort_k(const int2* __restrict__ ent, const unsigned long long* __restrict__ ecur, int bpr, int max_lesions,
                                                                       int max_border, int* __restrict__ eo, int* __restrict__ fill, int* __restrict__ sq) {
    const int n = blockIdx.x / bpr, b = blockIdx.x - n * bpr;
    const int cnt = (int)min(ecur[n], (unsigned long long)max_border);
    for (long long i = (long long)b * 256 + threadIdx.x; i < cnt; i += (long long)bpr * 256) {
        const int2 e = ent[(long long)n * max_border + i];
        if (!SCATTER) { atomicAdd(&eo[(long long)n * (max_lesions + 1) + e.y], 1); continue; }
        const int pos = eo[(long long)n * (max_lesions + 1) + e.y] + atomicAdd(&fill[(long long)n * max_lesions + e.y], 1);
        sq[(long long)n * max_border + pos] = e.x;                         // pos < cnt <= max_border: only stored entries were counted
    }
}

// one workgroup per row: eo[n][0 .. ML) counts -> exclusive offsets, eo[n][ML] the total; co[n][g] = the pair kernel's workgroups before lesion g
__global__ __launch_bounds__(256) void hd_scan_k(int* __restrict__ eo, int* __restrict__ co, int max_lesions) {
    __shared__ int se[256], sc[256];
    int* e = eo + (long long)blockIdx.x * (max_lesions + 1);
    int* c = co + (long long)blockIdx.x * (max_lesions + 1);
    const int per = (max_lesions + 255) / 256;
    const int lo = min((int)threadIdx.x * per, max_lesions), hi = min(lo + per, max_lesions);
    int s = 0, t = 0;
    for (int i = lo; i < hi; ++i) { s += e[i]; t += (e[i] + HD_Q - 1) / HD_Q; }
    se[threadIdx.x] = s; sc[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        int rs = 0, rc = 0;
        for (int i = 0; i < 256; ++i) { const int a = se[i], b = sc[i]; se[i] = rs; sc[i] = rc; rs += a; rc += b; }
        e[max_lesions] = rs; c[max_lesions] = rc;
    }
    __syncthreads();
    int rs = se[threadIdx.x], rc = sc[threadIdx.x];
    for (int i = lo; i < hi; ++i) { const int a = e[i]; e[i] = rs; c[i] = rc; rs += a; rc += (a + HD_Q - 1) / HD_Q; }
}

// bpr workgroups per row; workgroup b of row n takes HD_Q queries of the lesion g with co[n][g] <= b < co[n][g + 1]
__global__ __launch_bounds__(256) void hd_pair_k(const int* __restrict__ sq, const int* __restrict__ refA, const int* __restrict__ seg, const int* __restrict__ eo,
                                                 const int* __restrict__ co, int bpr, int max_lesions, int max_border, int H, int W,
                                                 int* __restrict__ dB, int* __restrict__ dminA) {
    __shared__ int4 qs[HD_Q], ss[HD_T];
    const int n = blockIdx.x / bpr, b = blockIdx.x - n * bpr;
    const int* c = co + (long long)n * (max_lesions + 1);
    if (b >= c[max_lesions]) return;
    int g = 0, hi = max_lesions;
    while (hi - g > 1) { const int mid = (g + hi) >> 1; if (c[mid] <= b) g = mid; else hi = mid; }
    const int* e = eo + (long long)n * (max_lesions + 1);
    const int e0 = e[g] + (b - c[g]) * HD_Q, nq = min(HD_Q, e[g + 1] - e0);
    const int s0 = min(seg[g], max_border), s1 = min(seg[g + 1], max_border);
    const long long row = (long long)n * max_border;
    const int tid = threadIdx.x;
    const bool valid = tid < nq;
    int4 me = make_int4(0, 0, 0, 0);
    if (valid) { me = hd_coords(sq[row + e0 + tid], H, W); qs[tid] = me; }
    int best = HD_NONE;
    for (int t0 = s0; t0 < s1; t0 += HD_T) {
        const int nt = min(HD_T, s1 - t0);
        __syncthreads();                                                   // the tile before is read out (and qs is written)
        for (int j = tid; j < nt; j += 256) ss[j] = hd_coords(refA[t0 + j], H, W);
        __syncthreads();
        if (valid)
            for (int j = 0; j < nt; ++j) best = min(best, hd_dist(me, ss[j]));
        for (int j = tid; j < nt; j += 256) {                              // the roles swapped: this workgroup's queries, seen from seed j
            const int4 s = ss[j];
            int m = HD_NONE;
            for (int i = 0; i < nq; ++i) m = min(m, hd_dist(s, qs[i]));
            __hip_atomic_fetch_min(&dminA[row + t0 + j], m, UZ_RLX_AGENT);
        }
    }
    if (valid) dB[row + e0 + tid] = best;
}

// one workgroup per (row, lesion): s[k0], s[k1] of the lesion's stretch of dminA and of dB together, by a radix select of 8 bits a pass
__global__ __launch_bounds__(256) void hd_select_k(const int* __restrict__ dminA, const int* __restrict__ dB, const int* __restrict__ seg, const int* __restrict__ eo,
                                                   const unsigned long long* __restrict__ ecur, const int* __restrict__ n_ref_p, int r, int R, int max_lesions, int max_border,
                                                   int64_t* __restrict__ hd_lesions, double* __restrict__ hdg) {
    __shared__ unsigned hist[256];
    __shared__ unsigned pick[3];                                          // the bin, the rank left inside it, its count
    __shared__ unsigned next_up;
    const int n = blockIdx.x / max_lesions, g = blockIdx.x - n * max_lesions;
    const int* e = eo + (long long)n * (max_lesions + 1);
    const bool over = seg[max_lesions] > max_border || ecur[n] > (unsigned long long)max_border;
    const int nb = e[g + 1] - e[g];
    int64_t* out = hd_lesions ? hd_lesions + (((long long)n * R + r) * max_lesions + g) * 3 : nullptr;
    if (over || g >= min(*n_ref_p, max_lesions) || nb == 0) {             // an overflow, no such lesion, or no match
        if (threadIdx.x == 0) {
            hdg[(long long)n * max_lesions + g] = 0.0;
            if (out) out[0] = out[1] = out[2] = 0;
        }
        return;
    }
    const int na = seg[g + 1] - seg[g];
    const int* pa = dminA + (long long)n * max_border + seg[g];
    const int* pb = dB + (long long)n * max_border + e[g];
    const unsigned m = (unsigned)na + (unsigned)nb;
    const double hq = 0.95 * (double)(m - 1);
    const unsigned k0 = (unsigned)floor(hq), k1 = k0 + 1 < m ? k0 + 1 : m - 1;
    unsigned prefix = 0, k = k0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        if (threadIdx.x == 0) next_up = 0xFFFFFFFFu;
        __syncthreads();
        for (unsigned i = threadIdx.x; i < m; i += 256) {
            const unsigned key = (unsigned)(i < (unsigned)na ? pa[i] : pb[i - na]);
            if (((unsigned long long)(key ^ prefix) >> (shift + 8)) == 0) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned before = 0, bin = 0;
            while (bin < 255 && before + hist[bin] <= k) before += hist[bin++];
            pick[0] = bin; pick[1] = k - before; pick[2] = hist[bin];
        }
        __syncthreads();
        prefix |= pick[0] << shift;
        k = pick[1];
        __syncthreads();
    }
    const unsigned lo = prefix;                                           // s[k0]; k of its pick[2] copies lie before position k0
    unsigned up = lo;
    if (k1 != k0 && k + 1 >= pick[2]) {                                   // position k0 is the last copy: s[k1] is the next greater value
        unsigned mine = 0xFFFFFFFFu;
        for (unsigned i = threadIdx.x; i < m; i += 256) {
            const unsigned key = (unsigned)(i < (unsigned)na ? pa[i] : pb[i - na]);
            if (key > lo) mine = min(mine, key);
        }
        atomicMin(&next_up, mine);
        __syncthreads();
        up = next_up;
    }
    if (threadIdx.x == 0) {
        const double a = sqrt((double)lo), b = sqrt((double)up);
        hdg[(long long)n * max_lesions + g] = a + (hq - (double)k0) * (b - a);
        if (out) { out[0] = m; out[1] = lo; out[2] = up; }
    }
}

// one thread per row: the mean in the order of the contract
__global__ __launch_bounds__(64) void hd_mean_k(const int* __restrict__ n_ref_p, const int* __restrict__ gt, const int* __restrict__ pred_vol, const int* __restrict__ ctr,
                                                const int* __restrict__ seg, const unsigned long long* __restrict__ ecur, const double* __restrict__ hdg, int N, int r, int R,
                                                int max_lesions, int max_border, int min_ref_voxels, double penalty, int64_t* __restrict__ hd_counts, double* __restrict__ hd95) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const int n_ref = *n_ref_p, n_tab = min(n_ref, max_lesions);
    const int* pv = pred_vol + (long long)n * max_lesions;
    long long n_kept = 0;
    double sum = 0.0;
    for (int g = 0; g < n_tab; ++g) {                                      // ascending g, serially: the order is part of the contract
        if (gt[g] < min_ref_voxels) continue;
        ++n_kept;
        sum += pv[g] ? hdg[(long long)n * max_lesions + g] : penalty;
    }
    const long long n_fp = ctr[n * 4 + 1];
    sum += penalty * (double)n_fp;
    const long long over_a = max((long long)seg[max_lesions] - max_border, 0LL);
    const long long over_b = ecur[n] > (unsigned long long)max_border ? (long long)(ecur[n] - (unsigned long long)max_border) : 0LL;
    int64_t* c = hd_counts + ((long long)n * R + r) * 2;
    c[0] = over_a; c[1] = over_b;
    double v = n_kept + n_fp ? sum / (double)(n_kept + n_fp) : 0.0;
    if (over_a || over_b || n_ref > n_tab || ctr[n * 4 + 2]) v = __longlong_as_double(0x7FF8000000000000LL);
    hd95[(long long)n * R + r] = v;
}

// ------------------------------------------------------------------------------------------------ host
inline int vox_grid(long long T) { return uz::sweep_grid(T, 256, VOX_GRID_MAX); }
inline int rank_blocks(int P) { return (int)(((long long)P + 255) / 256); }

struct Ws {
    void* comp; void* morph; uint8_t* dk; int* lg; int* rank; int* lp; int* sp; int* blk; int* tab;
    size_t tab_bytes, total;
};
// tab: gt (max_lesions), inter (N, max_lesions), pred_vol (N, max_lesions), ctr (N, 4)
inline Ws carve(void* workspace, int N, int D, int H, int W, int max_lesions) {
    const size_t P = (size_t)D * H * W, T = (size_t)N * P;
    char* b = static_cast<char*>(workspace);
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = b ? b + o : nullptr; o += uz::up16(bytes); return p; };
    Ws w;
    w.comp = take(uz_vol_components_workspace(N, D, H, W));               // the labelling's; behind the labelling, the link words: 2 int32 a voxel
    w.morph = take(uz_vol_morph_workspace(1, D, H, W));
    w.dk = reinterpret_cast<uint8_t*>(take(P));
    w.lg = reinterpret_cast<int*>(take(P * 4));
    w.rank = reinterpret_cast<int*>(take(P * 4));
    w.lp = reinterpret_cast<int*>(take(T * 4));
    w.sp = reinterpret_cast<int*>(take(T * 4));
    w.blk = reinterpret_cast<int*>(take(((size_t)rank_blocks((int)P) + 1) * 4));
    w.tab_bytes = ((size_t)max_lesions * (1 + 2 * (size_t)N) + 4 * (size_t)N) * 4;
    w.tab = reinterpret_cast<int*>(take(w.tab_bytes));
    w.total = o;
    return w;
}

const char* limits_bad(int N, int R, int D, int H, int W) {
    if (const char* bad = uz::vol_sizes_bad(N, D, H, W)) return bad;
    if (R < 1 || R > UZ_VOL_MAX_REGIONS) return "1 <= R <= 8 regions";
    return nullptr;
}

// the lists of rule 6, behind the workspace of the scores.  zero .. zero + zero_bytes is cleared per region: ecur (N), seg (ML + 1), fill_a (ML),
// eo (N, ML + 1), fill_e (N, ML)
struct HdWs {
    int* refA; int* dminA; int2* ent; int* sq; int* dB; int* co; double* hdg;
    unsigned long long* ecur; int* seg; int* fill_a; int* eo; int* fill_e;
    char* zero; size_t zero_bytes, total;
};
inline HdWs carve_hd(void* workspace, size_t at, int N, int max_lesions, int max_border) {
    const size_t MB = (size_t)max_border, ML = (size_t)max_lesions, n = (size_t)N;
    char* b = static_cast<char*>(workspace);
    size_t o = at;
    auto take = [&](size_t bytes) { char* p = b ? b + o : nullptr; o += uz::up16(bytes); return p; };
    HdWs h;
    h.refA = reinterpret_cast<int*>(take(MB * 4));
    h.dminA = reinterpret_cast<int*>(take(n * MB * 4));
    h.ent = reinterpret_cast<int2*>(take(n * MB * 8));
    h.sq = reinterpret_cast<int*>(take(n * MB * 4));
    h.dB = reinterpret_cast<int*>(take(n * MB * 4));
    h.co = reinterpret_cast<int*>(take(n * (ML + 1) * 4));
    h.hdg = reinterpret_cast<double*>(take(n * ML * 8));
    h.zero_bytes = n * 8 + ((ML + 1) + ML + n * (ML + 1) + n * ML) * 4;
    h.zero = take(h.zero_bytes);
    h.ecur = reinterpret_cast<unsigned long long*>(h.zero);
    h.seg = reinterpret_cast<int*>(h.zero ? h.zero + n * 8 : nullptr);
    h.fill_a = h.seg + (ML + 1);
    h.eo = h.fill_a + ML;
    h.fill_e = h.eo + n * (ML + 1);
    h.total = o;
    return h;
}
inline int hd_row_blocks(int max_border) { return (max_border + 255) / 256; }                          // workgroups per row of the two sort passes
inline int hd_pair_blocks(int max_border, int max_lesions) { return (max_border + HD_Q - 1) / HD_Q + max_lesions; }   // per row: every lesion may leave one part-filled workgroup
const char* hd_bad(int D, int H, int W, int max_border) {
    if ((long long)D * D + (long long)H * H + (long long)W * W > (1LL << 30)) return "D^2 + H^2 + W^2 beyond 2^30 (the squared distances)";
    if (max_border < 1 || max_border > (long long)D * H * W) return "1 <= max_border <= D*H*W";
    return nullptr;
}

}  // namespace

extern "C" size_t uz_vol_lesion_scores_workspace_ex(int N, int R, int D, int H, int W, int max_lesions, int want_hd95, int max_border) {
    if (limits_bad(N, R, D, H, W) || max_lesions < 1 || max_lesions > UZ_VOL_MAX_LESIONS) return 0;
    const size_t base = carve(nullptr, N, D, H, W, max_lesions).total;
    if (!want_hd95) return base;
    if (hd_bad(D, H, W, max_border)) return 0;
    return carve_hd(nullptr, base, N, max_lesions, max_border).total;
}

extern "C" size_t uz_vol_lesion_scores_workspace(int N, int R, int D, int H, int W, int max_lesions) {
    return uz_vol_lesion_scores_workspace_ex(N, R, D, H, W, max_lesions, 0, 0);
}

static int route_ex(const char* who, int N, int R, int D, int H, int W, int want_hd95, int* out, int n_out) {
    UZ_REQUIRE(out, "%s: %s ints to answer into", who, n_out == 2 ? "two" : "four");
    const char* bad = limits_bad(N, R, D, H, W);
    UZ_REQUIRE(!bad, "%s: %s", who, bad);
    int comp[2], morph[2];
    if (int rc = uz_vol_components_route_ex(N, D, H, W, 3, comp)) return rc;
    if (int rc = uz_vol_morph_route(1, D, H, W, morph)) return rc;
    out[0] = comp[0];                                                      // both labelling sweeps take this merge instance
    out[1] = std::max(std::max(comp[1], morph[1]), std::max(vox_grid((long long)N * D * H * W), rank_blocks(D * H * W)));
    if (n_out == 4) { out[2] = want_hd95 ? HD_Q : 0; out[3] = want_hd95 ? HD_T : 0; }
    return 0;
}

extern "C" int uz_vol_lesion_scores_route(int N, int R, int D, int H, int W, int* out2) {
    return route_ex("vol_lesion_scores_route", N, R, D, H, W, 0, out2, 2);
}

extern "C" int uz_vol_lesion_scores_route_ex(int N, int R, int D, int H, int W, int want_hd95, int* out4) {
    return route_ex("vol_lesion_scores_route_ex", N, R, D, H, W, want_hd95, out4, 4);
}

extern "C" int uz_vol_lesion_scores_ex(const uint8_t* pred, int N, const uint32_t* pred_sets, const uint8_t* ref, const uint32_t* ref_sets, int R,
                                       int D, int H, int W, int dilation, int min_ref_voxels, int min_pred_voxels, int max_lesions, int max_links,
                                       int want_hd95, const double* hd95_penalty, int max_border,
                                       void* workspace, int64_t* counts, int64_t* lesions, double* scores,
                                       int64_t* hd_counts, int64_t* hd_lesions, double* hd95, void* stream) {
    UZ_REQUIRE(pred && pred_sets && ref && ref_sets && workspace && counts && scores,
               "vol_lesion_scores: null argument (pred, pred_sets, ref, ref_sets, workspace, counts, scores)");
    const char* bad = limits_bad(N, R, D, H, W);
    UZ_REQUIRE(!bad, "vol_lesion_scores: %s", bad);
    UZ_REQUIRE(dilation >= 0 && dilation <= UZ_VOL_MAX_DILATION, "vol_lesion_scores: 0 <= dilation <= %d, not %d", UZ_VOL_MAX_DILATION, dilation);
    UZ_REQUIRE(min_ref_voxels >= 0 && min_pred_voxels >= 0, "vol_lesion_scores: min_ref_voxels %d, min_pred_voxels %d: a threshold is a voxel count >= 0",
               min_ref_voxels, min_pred_voxels);
    UZ_REQUIRE(max_lesions >= 1 && max_lesions <= UZ_VOL_MAX_LESIONS, "vol_lesion_scores: 1 <= max_lesions <= %d, not %d", UZ_VOL_MAX_LESIONS, max_lesions);
    UZ_REQUIRE(max_links >= 1 && max_links <= UZ_VOL_MAX_LINKS, "vol_lesion_scores: 1 <= max_links <= %d, not %d", UZ_VOL_MAX_LINKS, max_links);
    UZ_REQUIRE(uz::align_of(workspace) == 16, "vol_lesion_scores: workspace must be 16-byte aligned");
    UZ_REQUIRE(((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(lesions) | reinterpret_cast<uintptr_t>(scores)) & 7) == 0,
               "vol_lesion_scores: counts, lesions and scores must be 8-byte aligned");
    double penalty = 0.0;
    if (want_hd95) {
        UZ_REQUIRE(hd_counts && hd95 && hd95_penalty, "vol_lesion_scores: null argument (hd_counts, hd95, hd95_penalty) with want_hd95");
        const char* hbad = hd_bad(D, H, W, max_border);
        UZ_REQUIRE(!hbad, "vol_lesion_scores: %s (max_border %d)", hbad, max_border);
        penalty = *hd95_penalty;
        UZ_REQUIRE(penalty >= 0.0 && penalty <= DBL_MAX, "vol_lesion_scores: hd95_penalty %g: a finite distance >= 0", penalty);
        UZ_REQUIRE(((reinterpret_cast<uintptr_t>(hd_counts) | reinterpret_cast<uintptr_t>(hd_lesions) | reinterpret_cast<uintptr_t>(hd95)) & 7) == 0,
                   "vol_lesion_scores: hd_counts, hd_lesions and hd95 must be 8-byte aligned");
    }
    hipStream_t st = uz::S(stream);
    const int P = D * H * W;
    const long long T = (long long)N * P;
    const Ws w = carve(workspace, N, D, H, W, max_lesions);
    const HdWs h = want_hd95 ? carve_hd(workspace, w.total, N, max_lesions, max_border) : HdWs();
    const dim3 g_sort(want_hd95 ? N * hd_row_blocks(max_border) : 1), g_pair(want_hd95 ? N * hd_pair_blocks(max_border, max_lesions) : 1);
    int* settled = static_cast<int*>(w.comp);                              // 2 T int32 <= uz_vol_components_workspace(N, ...)
    int* cur = settled + T;
    int* gt = w.tab;
    int* inter = gt + max_lesions;
    int* pred_vol = inter + (long long)N * max_lesions;
    int* ctr = pred_vol + (long long)N * max_lesions;
    const int nb = rank_blocks(P);
    const dim3 blk256(256), gp(vox_grid(P)), gt_(vox_grid(T));
    for (int r = 0; r < R; ++r) {
        if (hipMemsetAsync(w.tab, 0, w.tab_bytes, st) != hipSuccess) return uz::fail("vol_lesion_scores: clearing the tables failed");
        // the reference side
        if (int rc = uz_vol_morph(ref, 1, D, H, W, ref_sets[r], 2, dilation, 0, w.dk, w.morph, stream)) return rc;
        if (int rc = uz_vol_label_components_ex(w.dk, 1, D, H, W, 2u, 3, w.lg, nullptr, w.comp, stream)) return rc;
        hipLaunchKernelGGL(les_count_k, dim3(nb), blk256, 0, st, w.lg, P, w.blk);
        if (int rc = uz::check_launch("les_count_k")) return rc;
        hipLaunchKernelGGL(les_scan_k, dim3(1), blk256, 0, st, w.blk, nb);
        if (int rc = uz::check_launch("les_scan_k")) return rc;
        hipLaunchKernelGGL(les_rank_k, dim3(nb), blk256, 0, st, w.lg, P, w.blk, w.rank);
        if (int rc = uz::check_launch("les_rank_k")) return rc;
        hipLaunchKernelGGL(les_index_k, gp, blk256, 0, st, ref, ref_sets[r], P, max_lesions, w.lg, w.rank, gt);
        if (int rc = uz::check_launch("les_index_k")) return rc;
        if (want_hd95) {                                                    // the border of G, grouped by lesion
            if (hipMemsetAsync(h.zero, 0, h.zero_bytes, st) != hipSuccess) return uz::fail("vol_lesion_scores: clearing the border tables failed");
            hipLaunchKernelGGL(hd_fill_k, dim3(vox_grid((long long)N * max_border)), blk256, 0, st, (long long)N * max_border, h.dminA);
            if (int rc = uz::check_launch("hd_fill_k")) return rc;
            hipLaunchKernelGGL(hd_ref_k<false>, gp, blk256, 0, st, ref, ref_sets[r], w.lg, P, D, H, W, max_lesions, max_border, h.seg, h.fill_a, h.refA);
            if (int rc = uz::check_launch("hd_ref_k")) return rc;
            hipLaunchKernelGGL(les_scan_k, dim3(1), blk256, 0, st, h.seg, max_lesions);
            if (int rc = uz::check_launch("les_scan_k")) return rc;
            hipLaunchKernelGGL(hd_ref_k<true>, gp, blk256, 0, st, ref, ref_sets[r], w.lg, P, D, H, W, max_lesions, max_border, h.seg, h.fill_a, h.refA);
            if (int rc = uz::check_launch("hd_ref_k")) return rc;
        }
        // the prediction side
        if (int rc = uz_vol_label_components_ex(pred, N, D, H, W, pred_sets[r], 3, w.lp, w.sp, w.comp, stream)) return rc;
        hipLaunchKernelGGL(les_init_k, gt_, blk256, 0, st, T, settled, cur);
        if (int rc = uz::check_launch("les_init_k")) return rc;
        for (int k = 0; k <= max_links; ++k) {
            if (k == 0) hipLaunchKernelGGL(les_offer_k<true>, gt_, blk256, 0, st, w.lp, w.lg, ref, ref_sets[r], T, P, max_lesions, settled, cur, inter);
            else hipLaunchKernelGGL(les_offer_k<false>, gt_, blk256, 0, st, w.lp, w.lg, ref, ref_sets[r], T, P, max_lesions, settled, cur, inter);
            if (int rc = uz::check_launch("les_offer_k")) return rc;
            if (k == max_links) break;                                      // the last offer is only counted
            if (want_hd95) {                                                // the border of the components that settle a link in this round
                hipLaunchKernelGGL(hd_entries_k, gt_, blk256, 0, st, pred, pred_sets[r], w.lp, cur, T, P, D, H, W, max_lesions, max_border, h.ecur, h.ent);
                if (int rc = uz::check_launch("hd_entries_k")) return rc;
            }
            if (k == 0) hipLaunchKernelGGL(les_settle_k<true>, gt_, blk256, 0, st, w.lp, w.sp, T, P, max_lesions, min_pred_voxels, settled, cur, pred_vol, ctr);
            else hipLaunchKernelGGL(les_settle_k<false>, gt_, blk256, 0, st, w.lp, w.sp, T, P, max_lesions, min_pred_voxels, settled, cur, pred_vol, ctr);
            if (int rc = uz::check_launch("les_settle_k")) return rc;
        }
        hipLaunchKernelGGL(les_left_k, gt_, blk256, 0, st, w.lp, T, P, cur, ctr);
        if (int rc = uz::check_launch("les_left_k")) return rc;
        hipLaunchKernelGGL(les_finish_k, dim3(N), blk256, 0, st, w.blk + nb, gt, inter, pred_vol, ctr, r, R, max_lesions, min_ref_voxels, counts, lesions, scores);
        if (int rc = uz::check_launch("les_finish_k")) return rc;
        if (!want_hd95) continue;
        hipLaunchKernelGGL(hd_sort_k<false>, g_sort, blk256, 0, st, h.ent, h.ecur, hd_row_blocks(max_border), max_lesions, max_border, h.eo, h.fill_e, h.sq);
        if (int rc = uz::check_launch("hd_sort_k")) return rc;
        hipLaunchKernelGGL(hd_scan_k, dim3(N), blk256, 0, st, h.eo, h.co, max_lesions);
        if (int rc = uz::check_launch("hd_scan_k")) return rc;
        hipLaunchKernelGGL(hd_sort_k<true>, g_sort, blk256, 0, st, h.ent, h.ecur, hd_row_blocks(max_border), max_lesions, max_border, h.eo, h.fill_e, h.sq);
        if (int rc = uz::check_launch("hd_sort_k")) return rc;
        hipLaunchKernelGGL(hd_pair_k, g_pair, blk256, 0, st, h.sq, h.refA, h.seg, h.eo, h.co, hd_pair_blocks(max_border, max_lesions), max_lesions, max_border, H, W, h.dB, h.dminA);
        if (int rc = uz::check_launch("hd_pair_k")) return rc;
        hipLaunchKernelGGL(hd_select_k, dim3(N * max_lesions), blk256, 0, st, h.dminA, h.dB, h.seg, h.eo, h.ecur, w.blk + nb, r, R, max_lesions, max_border, hd_lesions, h.hdg);
        if (int rc = uz::check_launch("hd_select_k")) return rc;
        hipLaunchKernelGGL(hd_mean_k, dim3((N + 63) / 64), dim3(64), 0, st, w.blk + nb, gt, pred_vol, ctr, h.seg, h.ecur, h.hdg, N, r, R, max_lesions, max_border,
                           min_ref_voxels, penalty, hd_counts, hd95);
        if (int rc = uz::check_launch("hd_mean_k")) return rc;
    }
    return 0;
}

extern "C" int uz_vol_lesion_scores(const uint8_t* pred, int N, const uint32_t* pred_sets, const uint8_t* ref, const uint32_t* ref_sets, int R,
                                    int D, int H, int W, int dilation, int min_ref_voxels, int min_pred_voxels, int max_lesions, int max_links,
                                    void* workspace, int64_t* counts, int64_t* lesions, double* scores, void* stream) {
    return uz_vol_lesion_scores_ex(pred, N, pred_sets, ref, ref_sets, R, D, H, W, dilation, min_ref_voxels, min_pred_voxels, max_lesions, max_links, 0, nullptr, 0,
                                   workspace, counts, lesions, scores, nullptr, nullptr, nullptr, stream);
}
