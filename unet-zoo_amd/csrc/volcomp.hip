// Connected components of label volumes on the device (uz_api.h "volume components"): a canonical labelling of the components of
// {label in set} at 6-, 18- or 26-connectivity, their sizes, the filter that keeps the largest (or the large enough) component of every
// set and erases or relabels the rest, and hole filling: the components of a set's COMPLEMENT that do not reach the volume's border.
// Replaces data/BratsProcessing/utils.py:228-251 (keep_largest_connected_components: skimage.measure.label(connectivity=1), regionprops
// and an argmax over the areas, per label, on the host).
//
// A union-find over the voxels' GLOBAL linear indices g = n*P + local (all N volumes in one index space, N*P < 2^31), the parent of a
// voxel always an index <= its own, so the root of a tree is the smallest index of its component and the labelling is canonical by
// construction: no scan order and no arrival order of an atomic can change it.
//   runs     one wave per row, 64 voxels a step, no atomics: a ballot gives every voxel the first voxel of its x-run as parent (a run
//            that crosses a 64-voxel step is carried in wave-uniform registers), and the run's length is parked in cnt[] at its first voxel;
//   merge    one union per OVERLAP of two runs in neighbouring rows (y-1) and slices (z-1): the thread of the overlap's first voxel unites;
//            at connectivity 2 and 3 the overlap is that of the run with the other run widened by one voxel, and the rows (z-1, y-1) and
//            (z-1, y+1) join in: the first voxel of my run whose window touches the other run unites (comp_merge_k);
//   flatten  every run's first voxel looks its root up, points at it, and adds its run length to cnt[root]: one integer add per run;
//   select   roots offer (size << 32) | (0xFFFFFFFF - local index) to a 64-bit maximum per volume, reduced per wave first;
//   apply    one pass over the voxels: parent[parent[v]] is the root (a voxel that is not first in its run never changed its parent).
//   border   (hole filling only, INV = the complement is the foreground) a complement voxel on the volume's border sets bit 31 of
//            cnt[root] with an integer OR - idempotent, and free: a size stays below 2^31; the fill pass reads size and bit in one word.
// Rows never join across their end because a run lives in one row and a window is cut at x = 0 and x = W-1; slices and volumes never
// join because merge looks at y-1 and y+1 only within the slice and at z-1 only within the volume: a neighbour outside the volume is
// never read.
#include "uz_common.h"
#include <algorithm>

namespace {

constexpr int VOX_GRID_MAX = 1 << 18;   // workgroups of a launch over the voxels (256 voxels each; a grid-stride loop covers the rest)
constexpr int ROW_GRID_MAX = 1 << 16;   // workgroups of the run kernel (four rows each)
constexpr int SEL_VOX = 4096;           // voxels of one volume a workgroup of the select kernel looks at per step

#define UZ_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// INV: the foreground is the set's complement (hole filling); a value of 32 or more is in no set and therefore in every complement
template <bool INV = false> __device__ __forceinline__ bool member(const uint8_t* __restrict__ lab, long long idx, uint32_t set) {
    return uz::in_set(lab[idx], set) != INV;
}

// ------------------------------------------------------------------------------------------------ runs
template <bool INV> __global__ __launch_bounds__(256) void comp_runs_k(const uint8_t* __restrict__ vol, uint32_t set, long long rows, int W, int N,
                                                   int* __restrict__ parent, int* __restrict__ cnt, unsigned long long* __restrict__ best) {
    if (blockIdx.x == 0)
        for (int n = threadIdx.x; n < N; n += 256) best[n] = 0ull;
    const int lane = threadIdx.x & 63;
    const int nchunk = (int)(((long long)W + 63) >> 6);                // W may be just below 2^31: positions along the row are 64-bit
    const unsigned long long below_me = (1ull << lane) - 1ull, me_and_below = lane == 63 ? ~0ull : (2ull << lane) - 1ull;
    for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * 4) {
        const long long base = row * W;                                   // < 2^31
        int open_start = -1, open_len = 0;                                // wave-uniform: the run that reached the end of the last step
        for (int c = 0; c < nchunk; ++c) {
            const long long x0 = (long long)c << 6, x = x0 + lane;
            const bool fg = x < W && member<INV>(vol, base + x, set);
            const unsigned long long m = __ballot(fg);
            const unsigned long long bg_below = ~m & below_me;
            // first lane of my run inside this step, or -1: it began in an earlier step
            const int st = bg_below ? 64 - __clzll((long long)bg_below) : (open_start >= 0 ? -1 : 0);
            if (x < W) parent[base + x] = fg ? (st < 0 ? open_start : (int)(base + x0 + st)) : -1;
            if (fg && st == lane) {                                       // a run begins here: park its length, unless it goes on into the next step
                const unsigned long long bg_above = ~m & ~me_and_below;
                if (bg_above) cnt[base + x] = __ffsll((long long)bg_above) - 1 - lane;
            }
            const int lead = ~m ? __ffsll((long long)~m) - 1 : 64;        // voxels of the run at the start of the step
            if (open_start >= 0) {
                if (lead == 64) open_len += 64;
                else { if (lane == 0) cnt[open_start] = open_len + lead; open_start = -1; }
            }
            if (open_start < 0 && (m >> 63)) {
                const int trail = ~m ? __clzll((long long)~m) : 64;       // voxels of the run at the end of the step
                open_start = (int)(base + x0 + 64 - trail); open_len = trail;
            }
        }
        if (open_start >= 0 && lane == 0) cnt[open_start] = open_len;     // W a multiple of 64 and the row ends inside a run
    }
}

// ------------------------------------------------------------------------------------------------ union-find
// The root of a's tree.  Terminates by construction: a parent is never larger than its index, so every round moves to a strictly
// smaller index or stops; nothing here waits for another thread.  A stale value is an older ancestor of the same tree: it costs a round.
__device__ __forceinline__ int find_root(int* parent, int a) {
    for (;;) {
        const int p = __hip_atomic_load(&parent[a], UZ_RLX_AGENT);
        if ((unsigned)p >= (unsigned)a) return a;                          // p == a: a root (anything else cannot be there, and is not followed)
        a = p;
    }
}
// Terminates by construction: every round either stops or goes on with two indices that are both smaller than this round's hi, and
// find_root only ever moves down.  No thread waits for another one's progress: fetch_min decides, and whoever finds that hi already
// had a parent takes over the duty to unite that parent with lo.  Correctness does not depend on how fresh a loaded parent is.
__device__ __forceinline__ void unite(int* parent, int a, int b) {
    for (;;) {
        a = find_root(parent, a); b = find_root(parent, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = __hip_atomic_fetch_min(&parent[hi], lo, UZ_RLX_AGENT);
        if (old == hi) return;                                             // hi was a root and now hangs below lo
        a = old; b = lo;                                                   // hi hung below old already: old and lo are to be united, both < hi
    }
}

// One earlier row at connectivity >= 2, `d` the (negative) index offset from voxel q at x to the other row's voxel at x; WIDE: the window
// is x-1 .. x+1, cut at the row's ends (never read beyond them), else x alone.  prev = my run goes on to the left of q.  "The first voxel
// of my run whose window touches that run" unites: with the voxel straight across foreground the window touches ONE run (x-1, x, x+1
// are contiguous) and my left neighbour's window, which reaches x, touched it already; with it background the window can touch TWO
// different runs - one that ends at x-1, which my left neighbour's window also touched, and one that begins at x+1, which no earlier
// voxel of my run can have touched (their windows end at x or before, and x is background).  Both are united.
template <bool INV, bool WIDE> __device__ __forceinline__ void merge_row(const uint8_t* __restrict__ vol, uint32_t set, int* parent, long long q, long long d,
                                                                         int x, int W, bool prev) {
    if (member<INV>(vol, q + d, set)) {
        if (!prev || (!WIDE && !member<INV>(vol, q + d - 1, set))) unite(parent, (int)q, (int)(q + d));
    } else if (WIDE) {
        if (!prev && x > 0 && member<INV>(vol, q + d - 1, set)) unite(parent, (int)q, (int)(q + d - 1));
        if (x < W - 1 && member<INV>(vol, q + d + 1, set)) unite(parent, (int)q, (int)(q + d + 1));
    }
}

// CONN 1: the rows (z, y-1) and (z-1, y) at x.  CONN 2: the same rows at x-1 .. x+1, and (z-1, y-1) and (z-1, y+1) at x.  CONN 3: all four
// rows at x-1 .. x+1.  The four are the 13 earlier neighbours of the 26 less x-1, which the run kernel resolved; the 13 later ones look
// back at this voxel.  (z-1, y+1) exists only for y < H-1: at y = H-1 the same arithmetic lands in row 0 of the voxel's OWN slice.
// What DESIGN.md 2e states holds at every new loop, because the only writes are still unite()'s: a parent is never larger than its
// index (fetch_min with lo < hi), every loop moves to a strictly smaller index or stops, no thread waits for another, and parent[] is
// touched by agent-scope relaxed atomics only.  A union that the predicate fails to drop is harmless: unite returns at a == b.
template <int CONN, bool INV> __global__ __launch_bounds__(256) void comp_merge_k(const uint8_t* __restrict__ vol, uint32_t set, long long T, int D, int H, int W, int* parent) {
    const int HW = H * W;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < T; q += (long long)gridDim.x * 256) {
        if (!member<INV>(vol, q, set)) continue;
        const long long t = q / W;
        const int x = (int)(q - t * W);
        const long long t2 = t / H;
        const int y = (int)(t - t2 * H), z = (int)(t2 % D);
        if constexpr (CONN == 1) {
            // the first voxel of the overlap of my run with the run above: not both left neighbours are foreground
            if (y > 0 && member<INV>(vol, q - W, set) && (x == 0 || !(member<INV>(vol, q - 1, set) && member<INV>(vol, q - 1 - W, set)))) unite(parent, (int)q, (int)(q - W));
            if (z > 0 && member<INV>(vol, q - HW, set) && (x == 0 || !(member<INV>(vol, q - 1, set) && member<INV>(vol, q - 1 - HW, set)))) unite(parent, (int)q, (int)(q - HW));
        } else {
            const bool prev = x > 0 && member<INV>(vol, q - 1, set);
            if (y > 0) merge_row<INV, true>(vol, set, parent, q, -(long long)W, x, W, prev);
            if (z > 0) {
                merge_row<INV, true>(vol, set, parent, q, -(long long)HW, x, W, prev);
                if (y > 0) merge_row<INV, CONN == 3>(vol, set, parent, q, -(long long)HW - W, x, W, prev);
                if (y < H - 1) merge_row<INV, CONN == 3>(vol, set, parent, q, -(long long)HW + W, x, W, prev);
            }
        }
    }
}

// Behind the kernel boundary the forest is final.  The first voxel of every run points at its root and hands its run length over.
// Another thread may walk through parent[q] while it is rewritten: it reads the old ancestor or the root, both in its tree.
template <bool INV> __global__ __launch_bounds__(256) void comp_flatten_k(const uint8_t* __restrict__ vol, uint32_t set, long long T, int W, int* parent, int* cnt) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < T; q += (long long)gridDim.x * 256) {
        if (!member<INV>(vol, q, set)) continue;
        if (q % W != 0 && member<INV>(vol, q - 1, set)) continue;
        const int r = find_root(parent, (int)q);
        if (r != (int)q) {
            __hip_atomic_store(&parent[q], r, UZ_RLX_AGENT);
            atomicAdd(&cnt[r], cnt[q]);                                    // cnt[q] of a run that is no root is never added to
        }
    }
}

// ------------------------------------------------------------------------------------------------ border (hole filling)
// A component of the complement that reaches the volume's border is no hole: bit 31 of cnt[root] says so.  The border is the six faces,
// and for D == 1, an image, the four edges (zface = 0).  One voxel per run speaks for a face row (the run's first), and the voxels at
// x = 0 and x = W-1 for the other rows.  An OR of one bit is idempotent: neither the order nor the number of arrivals shows.
__global__ __launch_bounds__(256) void comp_border_k(const uint8_t* __restrict__ vol, uint32_t set, long long T, int D, int H, int W, int zface,
                                                     const int* __restrict__ parent, int* cnt) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < T; q += (long long)gridDim.x * 256) {
        if (!member<true>(vol, q, set)) continue;
        const long long t = q / W;
        const int x = (int)(q - t * W);
        const long long t2 = t / H;
        const int y = (int)(t - t2 * H), z = (int)(t2 % D);
        const bool face_row = y == 0 || y == H - 1 || (zface && (z == 0 || z == D - 1));
        if (!(x == 0 || x == W - 1 || (face_row && !member<true>(vol, q - 1, set)))) continue;
        const int r = parent[parent[q]];
        if (__hip_atomic_load(&cnt[r], UZ_RLX_AGENT) >= 0) __hip_atomic_fetch_or(&cnt[r], (int)0x80000000u, UZ_RLX_AGENT);
    }
}

// ------------------------------------------------------------------------------------------------ select
__global__ __launch_bounds__(256) void comp_select_k(const int* __restrict__ parent, const int* __restrict__ cnt, int P, int per_vol, long long items,
                                                     unsigned long long* __restrict__ best) {
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int n = (int)(it / per_vol);
        const int v0 = (int)(it - (long long)n * per_vol) * SEL_VOX;
        const long long off = (long long)n * P;
        unsigned long long mine = 0ull;
        const long long vend = min((long long)v0 + SEL_VOX, (long long)P);
        for (long long v = v0 + threadIdx.x; v < vend; v += 256) {
            const long long g = off + v;
            if (parent[g] == (int)g) mine = max(mine, ((unsigned long long)(unsigned)cnt[g] << 32) | (0xFFFFFFFFull - (unsigned)v));
        }
        mine = uz::wave_max(mine);
        if ((threadIdx.x & 63) == 0 && mine) atomicMax(&best[n], mine);
    }
}

// ------------------------------------------------------------------------------------------------ outputs
__global__ __launch_bounds__(256) void comp_labels_k(const uint8_t* __restrict__ vol, uint32_t set, long long T, int P, const int* __restrict__ parent,
                                                     const int* __restrict__ cnt, int* __restrict__ labels, int* __restrict__ sizes) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < T; q += (long long)gridDim.x * 256) {
        int l = 0, s = 0;
        if (member(vol, q, set)) {
            const int r = parent[parent[q]];
            l = r - (int)(q / P) * P + 1;                                  // (q / P) * P < 2^31
            s = cnt[r];
        }
        labels[q] = l;
        if (sizes) sizes[q] = s;
    }
}

// first: out = vol where the label is listed (or unlisted labels are kept), 0 elsewhere; then every set writes `removed` (0, or the value
// it relabels to) over what it does not keep, and nothing over what it keeps: the last set that removes a voxel decides its value
__global__ __launch_bounds__(256) void comp_apply_k(const uint8_t* __restrict__ vol, uint32_t set, uint32_t listed, int keep_unlisted, int first,
                                                    int min_voxels, int removed, long long T, int P, const int* __restrict__ parent, const int* __restrict__ cnt,
                                                    const unsigned long long* __restrict__ best, uint8_t* __restrict__ out) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < T; q += (long long)gridDim.x * 256) {
        const unsigned l = vol[q];
        const bool in_set = l < 32u && ((set >> l) & 1u);
        bool kept = true;
        if (in_set) {
            const int r = parent[parent[q]];
            const unsigned sz = (unsigned)cnt[r];
            if (min_voxels > 0) kept = sz >= (unsigned)min_voxels;
            else {
                const int n = (int)(q / P);
                kept = best[n] == (((unsigned long long)sz << 32) | (0xFFFFFFFFull - (unsigned)(r - n * P)));
            }
        }
        if (!kept) out[q] = (uint8_t)removed;
        else if (first) out[q] = (keep_unlisted || (l < 32u && ((listed >> l) & 1u))) ? (uint8_t)l : (uint8_t)0;
    }
}

// first: out = vol; then every set writes its value into its holes: the components of its complement without the border bit, of at
// most max_voxels voxels (0: of any size).  The sets all see vol; a later set overwrites an earlier one
__global__ __launch_bounds__(256) void comp_fill_k(const uint8_t* __restrict__ vol, uint32_t set, int first, int max_voxels, int value, long long T,
                                                   const int* __restrict__ parent, const int* __restrict__ cnt, uint8_t* __restrict__ out) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < T; q += (long long)gridDim.x * 256) {
        const unsigned l = vol[q];
        bool fill = false;
        if (!uz::in_set(l, set)) {
            const int c = cnt[parent[parent[q]]];                          // negative: the component reaches the border
            fill = c >= 0 && (max_voxels == 0 || c <= max_voxels);
        }
        if (fill) out[q] = (uint8_t)value;
        else if (first) out[q] = (uint8_t)l;
    }
}

// ------------------------------------------------------------------------------------------------ host
inline const char* sizes_bad(int N, int D, int H, int W) { return uz::vol_sizes_bad(N, D, H, W); }
inline int vox_grid(long long T) { return uz::sweep_grid(T, 256, VOX_GRID_MAX); }
inline int row_grid(long long rows) { return uz::sweep_grid(rows, 4, ROW_GRID_MAX); }
inline int sel_per_vol(int P) { return (int)(((long long)P + SEL_VOX - 1) / SEL_VOX); }
inline int sel_grid(int N, int P) { return (int)std::min<long long>((long long)N * sel_per_vol(P), VOX_GRID_MAX); }

struct Ws { unsigned long long* best; int* parent; int* cnt; };
inline Ws carve(void* workspace, int N, long long T) {
    char* b = static_cast<char*>(workspace);
    Ws w;
    w.best = reinterpret_cast<unsigned long long*>(b);
    w.parent = reinterpret_cast<int*>(b + uz::up16((size_t)N * 8));
    w.cnt = reinterpret_cast<int*>(b + uz::up16((size_t)N * 8) + uz::up16((size_t)T * 4));
    return w;
}

// runs, merge, flatten of one set: afterwards parent[parent[v]] is the root of v and cnt[root] the size of its component
template <int CONN, bool INV> int label_set_as(const uint8_t* vol, uint32_t set, int N, int D, int H, int W, const Ws& w, hipStream_t st) {
    const long long rows = (long long)N * D * H, T = rows * W;
    hipLaunchKernelGGL(comp_runs_k<INV>, dim3(row_grid(rows)), dim3(256), 0, st, vol, set, rows, W, N, w.parent, w.cnt, w.best);
    if (int rc = uz::check_launch("comp_runs_k")) return rc;
    hipLaunchKernelGGL((comp_merge_k<CONN, INV>), dim3(vox_grid(T)), dim3(256), 0, st, vol, set, T, D, H, W, w.parent);
    if (int rc = uz::check_launch("comp_merge_k")) return rc;
    hipLaunchKernelGGL(comp_flatten_k<INV>, dim3(vox_grid(T)), dim3(256), 0, st, vol, set, T, W, w.parent, w.cnt);
    return uz::check_launch("comp_flatten_k");
}
// the merge instance of a connectivity, 0 for one that is refused: what the launches and uz_vol_components_route_ex both go by
inline int merge_form(int connectivity) { return connectivity >= 1 && connectivity <= 3 ? connectivity : 0; }
template <bool INV> int label_set(const uint8_t* vol, uint32_t set, int connectivity, int N, int D, int H, int W, const Ws& w, hipStream_t st) {
    switch (merge_form(connectivity)) {
        case 1: return label_set_as<1, INV>(vol, set, N, D, H, W, w, st);
        case 2: return label_set_as<2, INV>(vol, set, N, D, H, W, w, st);
        case 3: return label_set_as<3, INV>(vol, set, N, D, H, W, w, st);
    }
    return uz::fail("vol components: connectivity %d", connectivity);
}
inline bool overlap(const void* vol, const void* out, long long T) { return uz::bytes_overlap(vol, out, T); }

// uz_vol_label_components and uz_vol_label_components_ex: `who` names the caller in a refusal
int label_call(const char* who, const uint8_t* vol, int N, int D, int H, int W, uint32_t set, int connectivity, int32_t* labels, int32_t* sizes,
               void* workspace, void* stream) {
    UZ_REQUIRE(vol && labels && workspace, "%s: null argument (vol, labels, workspace)", who);
    const char* bad = sizes_bad(N, D, H, W);
    UZ_REQUIRE(!bad, "%s: %s", who, bad);
    UZ_REQUIRE(merge_form(connectivity), "%s: connectivity %d is not 1, 2 or 3", who, connectivity);
    UZ_REQUIRE(uz::align_of(workspace) == 16, "%s: workspace must be 16-byte aligned", who);
    UZ_REQUIRE((reinterpret_cast<uintptr_t>(labels) & 3) == 0 && (reinterpret_cast<uintptr_t>(sizes) & 3) == 0, "%s: labels and sizes must be 4-byte aligned", who);
    hipStream_t st = uz::S(stream);
    const int P = D * H * W;
    const long long T = (long long)N * P;
    const Ws w = carve(workspace, N, T);
    if (int rc = label_set<false>(vol, set, connectivity, N, D, H, W, w, st)) return rc;
    hipLaunchKernelGGL(comp_labels_k, dim3(vox_grid(T)), dim3(256), 0, st, vol, set, T, P, w.parent, w.cnt, labels, sizes);
    return uz::check_launch("comp_labels_k");
}

// uz_vol_keep_components (relabel == nullptr: every removed voxel becomes 0) and uz_vol_keep_components_ex
int keep_call(const char* who, const uint8_t* vol, int N, int D, int H, int W, const uint32_t* sets, const int32_t* min_voxels, const int32_t* relabel, int R,
              int connectivity, int keep_unlisted, uint8_t* out, void* workspace, void* stream) {
    const char* bad = sizes_bad(N, D, H, W);
    UZ_REQUIRE(!bad, "%s: %s", who, bad);
    UZ_REQUIRE(R >= 1 && R <= UZ_VOL_MAX_REGIONS, "%s: 1 <= R <= %d sets", who, UZ_VOL_MAX_REGIONS);
    for (int r = 0; r < R; ++r) UZ_REQUIRE(min_voxels[r] >= 0, "%s: min_voxels[%d] is negative", who, r);
    for (int r = 0; relabel && r < R; ++r) UZ_REQUIRE(relabel[r] >= -1 && relabel[r] <= 255, "%s: relabel[%d] = %d is neither -1 nor a value 0 .. 255", who, r, relabel[r]);
    UZ_REQUIRE(merge_form(connectivity), "%s: connectivity %d is not 1, 2 or 3", who, connectivity);
    UZ_REQUIRE(uz::align_of(workspace) == 16, "%s: workspace must be 16-byte aligned", who);
    const int P = D * H * W;
    const long long T = (long long)N * P;
    UZ_REQUIRE(!overlap(vol, out, T), "%s: out overlaps vol (later sets must see the unfiltered input)", who);
    hipStream_t st = uz::S(stream);
    const Ws w = carve(workspace, N, T);
    uint32_t listed = 0u;
    for (int r = 0; r < R; ++r) listed |= sets[r];
    for (int r = 0; r < R; ++r) {                                          // all N volumes of one set per launch, the sets one after the other
        if (int rc = label_set<false>(vol, sets[r], connectivity, N, D, H, W, w, st)) return rc;
        if (min_voxels[r] == 0) {
            hipLaunchKernelGGL(comp_select_k, dim3(sel_grid(N, P)), dim3(256), 0, st, w.parent, w.cnt, P, sel_per_vol(P), (long long)N * sel_per_vol(P), w.best);
            if (int rc = uz::check_launch("comp_select_k")) return rc;
        }
        hipLaunchKernelGGL(comp_apply_k, dim3(vox_grid(T)), dim3(256), 0, st, vol, sets[r], listed, keep_unlisted ? 1 : 0, r == 0 ? 1 : 0, min_voxels[r],
                           relabel && relabel[r] >= 0 ? relabel[r] : 0, T, P, w.parent, w.cnt, w.best, out);
        if (int rc = uz::check_launch("comp_apply_k")) return rc;
    }
    return 0;
}

int route_call(const char* who, int N, int D, int H, int W, int form, int* out2) {
    UZ_REQUIRE(out2, "%s: two ints to answer into", who);
    const char* bad = sizes_bad(N, D, H, W);
    UZ_REQUIRE(!bad, "%s: %s", who, bad);
    const long long rows = (long long)N * D * H, T = rows * W;
    out2[0] = form;
    out2[1] = std::max(std::max(row_grid(rows), vox_grid(T)), sel_grid(N, D * H * W));
    return 0;
}

}  // namespace

extern "C" size_t uz_vol_components_workspace(int N, int D, int H, int W) {
    if (sizes_bad(N, D, H, W)) return 0;
    return uz::up16((size_t)N * 8) + 2 * uz::up16((size_t)N * D * H * W * 4);
}

extern "C" int uz_vol_components_route(int N, int D, int H, int W, int* out2) {
    return route_call("vol_components_route", N, D, H, W, 0, out2);       // one form
}

extern "C" int uz_vol_components_route_ex(int N, int D, int H, int W, int connectivity, int* out2) {
    UZ_REQUIRE(merge_form(connectivity), "vol_components_route_ex: connectivity %d is not 1, 2 or 3", connectivity);
    return route_call("vol_components_route_ex", N, D, H, W, merge_form(connectivity), out2);
}

extern "C" int uz_vol_label_components(const uint8_t* vol, int N, int D, int H, int W, uint32_t set, int32_t* labels, int32_t* sizes,
                                       void* workspace, void* stream) {
    return label_call("vol_label_components", vol, N, D, H, W, set, 1, labels, sizes, workspace, stream);
}

extern "C" int uz_vol_label_components_ex(const uint8_t* vol, int N, int D, int H, int W, uint32_t set, int connectivity, int32_t* labels, int32_t* sizes,
                                          void* workspace, void* stream) {
    return label_call("vol_label_components_ex", vol, N, D, H, W, set, connectivity, labels, sizes, workspace, stream);
}

extern "C" int uz_vol_keep_components(const uint8_t* vol, int N, int D, int H, int W, const uint32_t* sets, const int32_t* min_voxels, int R,
                                      int keep_unlisted, uint8_t* out, void* workspace, void* stream) {
    UZ_REQUIRE(vol && sets && min_voxels && out && workspace, "vol_keep_components: null argument (vol, sets, min_voxels, out, workspace)");
    return keep_call("vol_keep_components", vol, N, D, H, W, sets, min_voxels, nullptr, R, 1, keep_unlisted, out, workspace, stream);
}

extern "C" int uz_vol_keep_components_ex(const uint8_t* vol, int N, int D, int H, int W, const uint32_t* sets, const int32_t* min_voxels, const int32_t* relabel,
                                         int R, int connectivity, int keep_unlisted, uint8_t* out, void* workspace, void* stream) {
    UZ_REQUIRE(vol && sets && min_voxels && relabel && out && workspace, "vol_keep_components_ex: null argument (vol, sets, min_voxels, relabel, out, workspace)");
    return keep_call("vol_keep_components_ex", vol, N, D, H, W, sets, min_voxels, relabel, R, connectivity, keep_unlisted, out, workspace, stream);
}

extern "C" int uz_vol_fill_holes(const uint8_t* vol, int N, int D, int H, int W, const uint32_t* sets, const int32_t* fill_values, const int32_t* max_voxels, int R,
                                 int connectivity, uint8_t* out, void* workspace, void* stream) {
    UZ_REQUIRE(vol && sets && fill_values && max_voxels && out && workspace, "vol_fill_holes: null argument (vol, sets, fill_values, max_voxels, out, workspace)");
    const char* bad = sizes_bad(N, D, H, W);
    UZ_REQUIRE(!bad, "vol_fill_holes: %s", bad);
    UZ_REQUIRE(R >= 1 && R <= UZ_VOL_MAX_REGIONS, "vol_fill_holes: 1 <= R <= %d sets", UZ_VOL_MAX_REGIONS);
    for (int r = 0; r < R; ++r) {
        UZ_REQUIRE(fill_values[r] >= 0 && uz::in_set((unsigned)fill_values[r], sets[r]), "vol_fill_holes: fill_values[%d] = %d is no member of its set", r, fill_values[r]);
        UZ_REQUIRE(max_voxels[r] >= 0, "vol_fill_holes: max_voxels[%d] is negative", r);
    }
    UZ_REQUIRE(merge_form(connectivity), "vol_fill_holes: connectivity %d is not 1, 2 or 3", connectivity);
    UZ_REQUIRE(uz::align_of(workspace) == 16, "vol_fill_holes: workspace must be 16-byte aligned");
    const long long T = (long long)N * D * H * W;
    UZ_REQUIRE(!overlap(vol, out, T), "vol_fill_holes: out overlaps vol (later sets must see the unfilled input)");
    hipStream_t st = uz::S(stream);
    const Ws w = carve(workspace, N, T);
    for (int r = 0; r < R; ++r) {                                          // the complement of one set in all N volumes per launch
        if (int rc = label_set<true>(vol, sets[r], connectivity, N, D, H, W, w, st)) return rc;
        hipLaunchKernelGGL(comp_border_k, dim3(vox_grid(T)), dim3(256), 0, st, vol, sets[r], T, D, H, W, D > 1 ? 1 : 0, w.parent, w.cnt);
        if (int rc = uz::check_launch("comp_border_k")) return rc;
        hipLaunchKernelGGL(comp_fill_k, dim3(vox_grid(T)), dim3(256), 0, st, vol, sets[r], r == 0 ? 1 : 0, max_voxels[r], fill_values[r], T, w.parent, w.cnt, out);
        if (int rc = uz::check_launch("comp_fill_k")) return rc;
    }
    return 0;
}
