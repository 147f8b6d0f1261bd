// Binary dilation and erosion of label volumes on the device (uz_api.h "volume morphology"): scipy.ndimage.binary_dilation /
// binary_erosion with structure = generate_binary_structure(3, connectivity), `iterations` passes, border_value = 0.
//
// Bit planes.  The membership mask {label in set} is packed once, one 64-bit word per __ballot of a wave, rows padded to whole words
// (WW = ceil(W / 64) words a row); every pass works on words and the result is unpacked once: one byte read and one byte written per
// voxel, the passes in between move a 64th of that.
//   pack     one wave per row, 64 voxels a step: lane 0 stores the ballot.  A lane beyond W votes 0, so pad bits start cleared.
//   pass     one thread per word.  xs(row) = the row's word combined with itself shifted one voxel left and right, the carry bit
//            taken from the neighbouring word of the SAME row (0 at the row's ends: rows never wrap); the new word is the
//            combination of xs of the voxel's own row with, of the eight neighbouring rows (dz, dy),
//              connectivity 1: the plain word of the four with |dz| + |dy| == 1,
//              connectivity 2: xs of those four and the plain word of the four with |dz| + |dy| == 2,
//              connectivity 3: xs of all eight.
//            "Combined" is OR for a dilation and AND for an erosion.  A row outside 0 <= y < H, 0 <= z < D of the voxel's own volume
//            is never read: it adds nothing to an OR and makes an AND 0 (border_value = 0: an erosion eats inward from the faces).
//            With D == 1 the stencil is the 2-D one: the rows dz != 0 are not part of it, for either operation.
//            The pad bits of a row's last word are "outside", which reads as 0: the pack leaves them 0 and every pass clears them on
//            the way out (a dilation sets the first of them whenever the row's last voxel is set), so a plane is canonical after
//            every pass and an erosion never sees a 1 beyond the row's end.
//   unpack   one thread per voxel.
// Two planes, ping-pong; every pass is one launch (the passes depend on each other across the whole volume).
#include "uz_common.h"

namespace {

constexpr int WORD_GRID_MAX = 1 << 18;
constexpr int VOX_GRID_MAX = 1 << 18;
constexpr int ROW_GRID_MAX = 1 << 16;
typedef unsigned long long u64;

__global__ __launch_bounds__(256) void morph_pack_k(const uint8_t* __restrict__ vol, uint32_t set, long long rows, int W, int WW, u64* __restrict__ plane) {
    const int lane = threadIdx.x & 63;
    for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * 4) {
        const long long base = row * W;
        for (int c = 0; c < WW; ++c) {
            const long long x = ((long long)c << 6) + lane;
            const u64 m = __ballot(x < W && uz::in_set(vol[base + (x < W ? x : 0)], set));
            if (lane == 0) plane[row * WW + c] = m;
        }
    }
}

// the word c of row `r` with its two x neighbours folded in; `src` points at the row's first word
template <bool ERODE> __device__ __forceinline__ u64 x_step(const u64* __restrict__ src, int c, int WW) {
    const u64 w = src[c];
    const u64 lo = c > 0 ? src[c - 1] >> 63 : 0ull;                      // voxel x-1 of bit 0
    const u64 hi = c < WW - 1 ? src[c + 1] << 63 : 0ull;                 // voxel x+1 of bit 63
    const u64 l = (w << 1) | lo, r = (w >> 1) | hi;
    return ERODE ? (w & l & r) : (w | l | r);
}

template <int CONN, bool ERODE> __global__ __launch_bounds__(256) void morph_pass_k(const u64* __restrict__ src, u64* __restrict__ dst, long long words, int D, int H,
                                                                                  int WW, u64 last_mask) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < words; i += (long long)gridDim.x * 256) {
        const long long row = i / WW;
        const int c = (int)(i - row * WW);
        const long long t2 = row / H;
        const int y = (int)(row - t2 * H), z = (int)(t2 % D);
        u64 acc = x_step<ERODE>(src + row * WW, c, WW);
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz) {
            if (D == 1 && dz != 0) continue;                              // an image: the 2-D stencil
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int k = (dz != 0) + (dy != 0);                      // coordinates that differ, x aside
                if (k == 0 || k > CONN) continue;
                const bool wide = k < CONN;                               // one more coordinate may differ: x
                const bool inside = z + dz >= 0 && z + dz < D && y + dy >= 0 && y + dy < H;
                u64 v = 0ull;
                if (inside) {
                    const u64* r = src + (row + (long long)dz * H + dy) * WW;
                    v = wide ? x_step<ERODE>(r, c, WW) : r[c];
                }
                acc = ERODE ? (acc & v) : (acc | v);
            }
        }
        dst[i] = c == WW - 1 ? (acc & last_mask) : acc;
    }
}

__global__ __launch_bounds__(256) void morph_unpack_k(const u64* __restrict__ plane, long long T, int W, int WW, uint8_t* __restrict__ out) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < T; q += (long long)gridDim.x * 256) {
        const long long row = q / W;
        const int x = (int)(q - row * W);
        out[q] = (uint8_t)((plane[row * WW + (x >> 6)] >> (x & 63)) & 1ull);
    }
}

inline int words_per_row(int W) { return (int)(((long long)W + 63) >> 6); }
inline size_t plane_bytes(int N, int D, int H, int W) { return uz::up16((size_t)N * D * H * words_per_row(W) * 8); }

template <int CONN> int launch_pass(int erode, const u64* src, u64* dst, long long words, int D, int H, int WW, u64 last_mask, hipStream_t st) {
    const dim3 grid(uz::sweep_grid(words, 256, WORD_GRID_MAX));
    if (erode) hipLaunchKernelGGL((morph_pass_k<CONN, true>), grid, dim3(256), 0, st, src, dst, words, D, H, WW, last_mask);
    else hipLaunchKernelGGL((morph_pass_k<CONN, false>), grid, dim3(256), 0, st, src, dst, words, D, H, WW, last_mask);
    return uz::check_launch("morph_pass_k");
}

}  // namespace

extern "C" size_t uz_vol_morph_workspace(int N, int D, int H, int W) {
    if (uz::vol_sizes_bad(N, D, H, W)) return 0;
    return 2 * plane_bytes(N, D, H, W);
}

extern "C" int uz_vol_morph_route(int N, int D, int H, int W, int* out2) {
    UZ_REQUIRE(out2, "vol_morph_route: two ints to answer into");
    const char* bad = uz::vol_sizes_bad(N, D, H, W);
    UZ_REQUIRE(!bad, "vol_morph_route: %s", bad);
    const long long rows = (long long)N * D * H;
    const int WW = words_per_row(W);
    out2[0] = WW;
    out2[1] = std::max(std::max(uz::sweep_grid(rows, 4, ROW_GRID_MAX), uz::sweep_grid(rows * WW, 256, WORD_GRID_MAX)), uz::sweep_grid(rows * W, 256, VOX_GRID_MAX));
    return 0;
}

extern "C" int uz_vol_morph(const uint8_t* vol, int N, int D, int H, int W, uint32_t set, int connectivity, int iterations, int erode, uint8_t* out,
                            void* workspace, void* stream) {
    UZ_REQUIRE(vol && out && workspace, "vol_morph: null argument (vol, out, workspace)");
    const char* bad = uz::vol_sizes_bad(N, D, H, W);
    UZ_REQUIRE(!bad, "vol_morph: %s", bad);
    UZ_REQUIRE(connectivity >= 1 && connectivity <= 3, "vol_morph: connectivity %d is not 1, 2 or 3", connectivity);
    UZ_REQUIRE(iterations >= 0, "vol_morph: iterations %d is negative", iterations);
    UZ_REQUIRE(erode == 0 || erode == 1, "vol_morph: erode %d is neither 0 nor 1", erode);
    UZ_REQUIRE(uz::align_of(workspace) == 16, "vol_morph: workspace must be 16-byte aligned");
    const long long rows = (long long)N * D * H, T = rows * W;
    UZ_REQUIRE(!uz::bytes_overlap(vol, out, T), "vol_morph: out overlaps vol");
    hipStream_t st = uz::S(stream);
    const int WW = words_per_row(W);
    const long long words = rows * WW;
    u64* a = static_cast<u64*>(workspace);
    u64* b = reinterpret_cast<u64*>(static_cast<char*>(workspace) + plane_bytes(N, D, H, W));
    const u64 last_mask = (W & 63) ? (1ull << (W & 63)) - 1ull : ~0ull;
    hipLaunchKernelGGL(morph_pack_k, dim3(uz::sweep_grid(rows, 4, ROW_GRID_MAX)), dim3(256), 0, st, vol, set, rows, W, WW, a);
    if (int rc = uz::check_launch("morph_pack_k")) return rc;
    for (int it = 0; it < iterations; ++it) {
        int rc = connectivity == 1 ? launch_pass<1>(erode, a, b, words, D, H, WW, last_mask, st)
               : connectivity == 2 ? launch_pass<2>(erode, a, b, words, D, H, WW, last_mask, st)
                                   : launch_pass<3>(erode, a, b, words, D, H, WW, last_mask, st);
        if (rc) return rc;
        std::swap(a, b);
    }
    hipLaunchKernelGGL(morph_unpack_k, dim3(uz::sweep_grid(T, 256, VOX_GRID_MAX)), dim3(256), 0, st, a, T, W, WW, out);
    return uz::check_launch("morph_unpack_k");
}
