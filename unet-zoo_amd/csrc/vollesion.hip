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

}  // namespace

extern "C" size_t uz_vol_lesion_scores_workspace(int N, int R, int D, int H, int W, int max_lesions) {
    if (limits_bad(N, R, D, H, W) || max_lesions < 1 || max_lesions > UZ_VOL_MAX_LESIONS) return 0;
    return carve(nullptr, N, D, H, W, max_lesions).total;
}

extern "C" int uz_vol_lesion_scores_route(int N, int R, int D, int H, int W, int* out2) {
    UZ_REQUIRE(out2, "vol_lesion_scores_route: two ints to answer into");
    const char* bad = limits_bad(N, R, D, H, W);
    UZ_REQUIRE(!bad, "vol_lesion_scores_route: %s", bad);
    int comp[2], morph[2];
    if (int rc = uz_vol_components_route_ex(N, D, H, W, 3, comp)) return rc;
    if (int rc = uz_vol_morph_route(1, D, H, W, morph)) return rc;
    out2[0] = comp[0];                                                     // both labelling sweeps take this merge instance
    out2[1] = std::max(std::max(comp[1], morph[1]), std::max(vox_grid((long long)N * D * H * W), rank_blocks(D * H * W)));
    return 0;
}

extern "C" int uz_vol_lesion_scores(const uint8_t* pred, int N, const uint32_t* pred_sets, const uint8_t* ref, const uint32_t* ref_sets, int R,
                                    int D, int H, int W, int dilation, int min_ref_voxels, int min_pred_voxels, int max_lesions, int max_links,
                                    void* workspace, int64_t* counts, int64_t* lesions, double* scores, void* stream) {
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
    hipStream_t st = uz::S(stream);
    const int P = D * H * W;
    const long long T = (long long)N * P;
    const Ws w = carve(workspace, N, D, H, W, max_lesions);
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
        // the prediction side
        if (int rc = uz_vol_label_components_ex(pred, N, D, H, W, pred_sets[r], 3, w.lp, w.sp, w.comp, stream)) return rc;
        hipLaunchKernelGGL(les_init_k, gt_, blk256, 0, st, T, settled, cur);
        if (int rc = uz::check_launch("les_init_k")) return rc;
        for (int k = 0; k <= max_links; ++k) {
            if (k == 0) hipLaunchKernelGGL(les_offer_k<true>, gt_, blk256, 0, st, w.lp, w.lg, ref, ref_sets[r], T, P, max_lesions, settled, cur, inter);
            else hipLaunchKernelGGL(les_offer_k<false>, gt_, blk256, 0, st, w.lp, w.lg, ref, ref_sets[r], T, P, max_lesions, settled, cur, inter);
            if (int rc = uz::check_launch("les_offer_k")) return rc;
            if (k == max_links) break;                                      // the last offer is only counted
            if (k == 0) hipLaunchKernelGGL(les_settle_k<true>, gt_, blk256, 0, st, w.lp, w.sp, T, P, max_lesions, min_pred_voxels, settled, cur, pred_vol, ctr);
            else hipLaunchKernelGGL(les_settle_k<false>, gt_, blk256, 0, st, w.lp, w.sp, T, P, max_lesions, min_pred_voxels, settled, cur, pred_vol, ctr);
            if (int rc = uz::check_launch("les_settle_k")) return rc;
        }
        hipLaunchKernelGGL(les_left_k, gt_, blk256, 0, st, w.lp, T, P, cur, ctr);
        if (int rc = uz::check_launch("les_left_k")) return rc;
        hipLaunchKernelGGL(les_finish_k, dim3(N), blk256, 0, st, w.blk + nb, gt, inter, pred_vol, ctr, r, R, max_lesions, min_ref_voxels, counts, lesions, scores);
        if (int rc = uz::check_launch("les_finish_k")) return rc;
    }
    return 0;
}
