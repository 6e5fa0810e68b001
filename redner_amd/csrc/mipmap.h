// mipmap.h -- the mip pyramid of an image texture and its adjoint (rdr_mip_pyramid / rdr_mip_pyramid_backward).
//
// The meaning is that of pyredner/texture.py:34-69 (Texture.generate_mipmap).  For texels [H, W, C] fp32:
//   * num_levels = min(ceil(log2(max(H, W))) + 1, 8); level 0 is the input.  A side that is not a power of two reaches 1 early
//     and the last levels repeat at 1 x 1; they are kept (the renderer's level selection depends on the count).
//   * level l + 1 (Ho x Wo = max(Hp / 2, 1) x max(Wp / 2, 1)) from level l (P, Hp x Wp):
//       B[r, c]   = ((P[r, c] + P[r, c+1]) + (P[r+1, c] + P[r+1, c+1])) * 0.25        indices WRAP (circular padding + 2 x 2 box)
//       out[i, j] = (sum of B over rows [floor(i Hp / Ho), ceil((i+1) Hp / Ho)) and the like columns, row-major) / count
//     (interpolate(mode='area')).  An even side gives the wrapping [1 2 1] / 4 filter at stride 2, an odd side windows of 3
//     that overlap, a side of 1 the identity.
//   * the adjoint is the transpose of that linear map summed down the chain: acc_l = g_l + A_{l+1}^T acc_{l+1}, d_texels = acc_0,
//     where g_l is the upstream gradient of level l (absent = zero).  It is a GATHER: a fine texel (r, c) adds, in ascending
//     (i, j), (acc[i, j] / count(i, j)) * (0.25 * m_r * m_c) of the coarse texels whose windows hold row r or r - 1 (m_r says
//     how many of the two) and column c or c - 1.  No atomics: bitwise reproducible from run to run.
//
// INDICES ARE "UNWRAPPED".  Wrapping makes the texels a tile needs non-contiguous at the right / bottom (forward) and left /
// top (adjoint) border.  Every function below therefore takes indices that may lie outside [0, n): index x of a level with n
// rows stands for row x mod n, and the window of coarse index i = q no + m is the window of m shifted by q np.  With that, what
// a range of coarse texels needs of the finer level (and the other way round in the adjoint) is ONE contiguous range, the same
// closed forms serve every tile, and a side of 1 or 2, where the wrapped neighbour is the texel itself or falls into the same
// window, needs no special case: the coincidences are counted with their multiplicity because they are separate unwrapped
// indices.
//
// Every level after the first has no = max(np / 2, 1) rows, so np is 1, 2 no or 2 no + 1 and the floor / ceil of the window rule
// reduce to shifts: the window of row m is [2 m, 2 m + 2 + (np & 1)), or [0, 1) when np == 1 (window(), covering()).
//
// The per-texel bodies (down_texel, up_texel) are shared by the kernels at the end of this header and by the plain loops of the
// CPU debugging harness.  A texel's value depends only on the values of the level before it and is computed by the same
// function in the same order wherever it is computed (from global memory, or from a tile in LDS), so the harness and the
// kernels agree bit for bit.  fp32 throughout, no contraction.
#pragma once
#include "../../include/redner_amd.h"
#include "arena.h"
#include <stdexcept>
#include <string>

namespace rdr {
namespace mip {

constexpr int kMaxLevels = 8;
constexpr int kChunk = 4;            // channels a lane holds at a time

RDR_FN int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
RDR_FN int wrap(int x, int n) { return (x >= 0 && x < n) ? x : x - floor_div(x, n) * n; }

struct Range { int lo, hi; };        // [lo, hi)
RDR_FN bool inside(Range r, int x) { return r.lo <= x && x < r.hi; }
RDR_FN int len(Range r) { return r.hi - r.lo; }

// rows of the finer level (np of them) that coarse row i (of no = max(np / 2, 1)) averages: B rows [lo, hi), i.e. P rows [lo, hi]
RDR_FN Range window(int i, int np, int no) {
    int q = 0, m = i;
    if (i < 0 || i >= no) { q = floor_div(i, no); m = i - q * no; }
    const int lo = q * np + (np == 1 ? 0 : 2 * m);
    return Range{lo, lo + (np == 1 ? 1 : 2 + (np & 1))};
}
// coarse rows whose window holds fine row x: [lo, hi)
RDR_FN Range covering(int x, int np, int no) {
    int q = 0, m = x;
    if (x < 0 || x >= np) { q = floor_div(x, np); m = x - q * np; }
    if (np == 1) return Range{q * no, q * no + 1};
    const int first = (np & 1) ? (m > 0 ? (m - 1) >> 1 : 0) : m >> 1, last = (m >> 1) < no - 1 ? m >> 1 : no - 1;
    return Range{q * no + first, q * no + last + 1};
}
// forward: the fine rows that the coarse rows [c.lo, c.hi) read (the + 1 row of B included)
RDR_FN Range fine_needed(Range c, int np, int no) { return Range{window(c.lo, np, no).lo, window(c.hi - 1, np, no).hi + 1}; }
// adjoint: the coarse rows that the fine rows [f.lo, f.hi) gather from
RDR_FN Range coarse_needed(Range f, int np, int no) { return Range{covering(f.lo - 1, np, no).lo, covering(f.hi - 1, np, no).hi}; }

// The sizes of every level and the tensors' channel count: what a launch knows about the pyramid.
struct Shape {
    int h[kMaxLevels], w[kMaxLevels];
    int channels, num_levels;
};
struct Levels { float *p[kMaxLevels]; };
struct ConstLevels { const float *p[kMaxLevels]; };

inline int num_levels(int height, int width) {
    const int side = height > width ? height : width;
    int bits = 0;                                  // (side - 1).bit_length()
    for (int v = side - 1; v > 0; v >>= 1) ++bits;
    return bits + 1 < kMaxLevels ? bits + 1 : kMaxLevels;
}

// The channels [ch0, ch0 + ...) of one level in global (or host) memory, read at unwrapped indices; a null level reads as zeros.
struct GlobalTexels {
    const float *p;
    int h, w, channels, ch0;
    RDR_FN float operator()(int r, int c, int k) const {
        return p ? p[((size_t)wrap(r, h) * w + wrap(c, w)) * channels + ch0 + k] : 0.f;
    }
};
// A tile [r0, ...) x [c0, c0 + ncols) x cc of unwrapped indices (LDS)
struct TileTexels {
    const float *p;
    int r0, c0, ncols, cc;
    RDR_FN float operator()(int r, int c, int k) const { return p[((r - r0) * ncols + (c - c0)) * cc + k]; }
};

// out[k] = texel (i, j), channel k < n <= kChunk of P's chunk, of the level of size ho x wo from the level P of size hp x wp
template <class F>
RDR_FN void down_texel(const F &P, int hp, int wp, int ho, int wo, int i, int j, int n, float *out) {
    const Range rw = window(i, hp, ho), cw = window(j, wp, wo);
    float sum[kChunk] = {0.f, 0.f, 0.f, 0.f};
    for (int r = rw.lo; r < rw.hi; ++r)
        for (int c = cw.lo; c < cw.hi; ++c)
            for (int k = 0; k < kChunk; ++k)
                if (k < n) sum[k] += ((P(r, c, k) + P(r, c + 1, k)) + (P(r + 1, c, k) + P(r + 1, c + 1, k))) * 0.25f;
    const float count = (float)(len(rw) * len(cw));
    for (int k = 0; k < kChunk; ++k)
        if (k < n) out[k] = sum[k] / count;
}

// out[k] = what fine texel (r, c) of the level of size hp x wp gathers from the coarse level's ACC (ho x wo): (A^T acc)[r, c]
template <class F>
RDR_FN void up_texel(const F &ACC, int hp, int wp, int ho, int wo, int r, int c, int n, float *out) {
    const Range ri = coarse_needed(Range{r, r + 1}, hp, ho), ci = coarse_needed(Range{c, c + 1}, wp, wo);
    float sum[kChunk] = {0.f, 0.f, 0.f, 0.f};
    for (int i = ri.lo; i < ri.hi; ++i) {
        const Range rw = window(i, hp, ho);
        const int mr = (int)inside(rw, r - 1) + (int)inside(rw, r);
        for (int j = ci.lo; j < ci.hi; ++j) {
            const Range cw = window(j, wp, wo);
            const int mc = (int)inside(cw, c - 1) + (int)inside(cw, c);
            const float count = (float)(len(rw) * len(cw)), weight = 0.25f * (float)(mr * mc);
            for (int k = 0; k < kChunk; ++k)
                if (k < n) sum[k] += (ACC(i, j, k) / count) * weight;
        }
    }
    for (int k = 0; k < kChunk; ++k)
        if (k < n) out[k] = sum[k];
}

// ---- tiles ---------------------------------------------------------------------------------------------------------------
// A tiled launch does three levels: b + 1 .. b + 3 from level b (forward), acc_b from acc_{b+3} (adjoint).  A forward workgroup
// owns kTile x kTile texels of level b + 3; the texels of the levels b + 2 and b + 1 those need (halo included) are computed
// into LDS, and the part of them the tile OWNS (a level is partitioned by the first row of each window) is also written out.
// An adjoint workgroup owns kFineTile x kFineTile texels of level b and computes the acc_{b+2} and acc_{b+1} texels they gather
// from into LDS.  A lane computes one texel at a time, kChunk channels of it (blockIdx.z: which); a chunk of an rgb texture is
// the whole texel.
constexpr int kTile = 4, kFineTile = 32;
// LDS capacities per side: a tile's range at the next level has fewer than n Hp / Ho + 3 (forward; n <= Ho + 2, Hp <= 2 Ho + 1)
// resp. (n + 1) Ho / Hp + 2 (adjoint) entries.  check_tiles() checks the actual ranges of every tile against these before a launch.
constexpr int kDown2 = 2 * kTile + 4, kDown1 = 2 * kDown2 + 6;          // 12, 30
constexpr int kUp1 = kFineTile / 2 + 3, kUp2 = kUp1 / 2 + 3;            // 19, 12
// A level of at most this many floats is finished by ONE workgroup (the chain kernels): the whole pyramid when level 0 is that
// small.  Above it a tiled launch does three levels at a time for all the texels in parallel.
constexpr int kSmall = 64 * 64 * 3;
constexpr int kChainThreads = 1024;

struct Tile { Range r3, c3, r2, c2, r1, c1, own2r, own2c, own1r, own1c; };
// the forward tile (ty, tx) over level b: ranges it computes at levels b + 3, b + 2, b + 1 and the part of b + 2, b + 1 it writes
RDR_FN Tile forward_tile(const Shape &s, int b, int ty, int tx) {
    const int *h = s.h + b, *w = s.w + b;
    Tile t;
    t.r3 = Range{ty * kTile, ty * kTile + kTile < h[3] ? ty * kTile + kTile : h[3]};
    t.c3 = Range{tx * kTile, tx * kTile + kTile < w[3] ? tx * kTile + kTile : w[3]};
    t.r2 = fine_needed(t.r3, h[2], h[3]);
    t.c2 = fine_needed(t.c3, w[2], w[3]);
    t.r1 = fine_needed(t.r2, h[1], h[2]);
    t.c1 = fine_needed(t.c2, w[1], w[2]);
    t.own2r = Range{window(t.r3.lo, h[2], h[3]).lo, t.r3.hi == h[3] ? h[2] : window(t.r3.hi, h[2], h[3]).lo};
    t.own2c = Range{window(t.c3.lo, w[2], w[3]).lo, t.c3.hi == w[3] ? w[2] : window(t.c3.hi, w[2], w[3]).lo};
    t.own1r = Range{window(t.own2r.lo, h[1], h[2]).lo, t.own2r.hi == h[2] ? h[1] : window(t.own2r.hi, h[1], h[2]).lo};
    t.own1c = Range{window(t.own2c.lo, w[1], w[2]).lo, t.own2c.hi == w[2] ? w[1] : window(t.own2c.hi, w[1], w[2]).lo};
    return t;
}
struct FineTile { Range r0, c0, r1, c1, r2, c2; };
RDR_FN FineTile adjoint_tile(const Shape &s, int b, int ty, int tx) {
    const int *h = s.h + b, *w = s.w + b;
    FineTile t;
    t.r0 = Range{ty * kFineTile, ty * kFineTile + kFineTile < h[0] ? ty * kFineTile + kFineTile : h[0]};
    t.c0 = Range{tx * kFineTile, tx * kFineTile + kFineTile < w[0] ? tx * kFineTile + kFineTile : w[0]};
    t.r1 = coarse_needed(t.r0, h[0], h[1]);
    t.c1 = coarse_needed(t.c0, w[0], w[1]);
    t.r2 = coarse_needed(t.r1, h[1], h[2]);
    t.c2 = coarse_needed(t.c1, w[1], w[2]);
    return t;
}

#if !defined(RDR_HOSTSIM)
// ---- gfx950 kernels --------------------------------------------------------------------------------------------------------
// Levels [first, last] by ONE workgroup, each from the level before it in global memory (written by this workgroup: the barrier
// between two levels orders the stores of one before the loads of the next).  A lane takes a texel, chunk by chunk of channels.
__global__ void __launch_bounds__(kChainThreads) mip_chain_kernel(Levels lv, Shape s, int first, int last) {
    const int C = s.channels;
    for (int l = first; l <= last; ++l) {
        const int texels = s.h[l] * s.w[l];
        for (int e = threadIdx.x; e < texels; e += kChainThreads) {
            const int i = e / s.w[l], j = e - i * s.w[l];
            for (int ch0 = 0; ch0 < C; ch0 += kChunk) {
                const int n = C - ch0 < kChunk ? C - ch0 : kChunk;
                float v[kChunk];
                down_texel(GlobalTexels{lv.p[l - 1], s.h[l - 1], s.w[l - 1], C, ch0}, s.h[l - 1], s.w[l - 1], s.h[l], s.w[l], i, j, n, v);
                for (int k = 0; k < kChunk; ++k)
                    if (k < n) lv.p[l][(size_t)e * C + ch0 + k] = v[k];
            }
        }
        __syncthreads();
    }
}

// acc_l = g_l + A_{l+1}^T acc_{l+1} for l = first down to last, by one workgroup.  acc.p[l] is where acc_l is written (scratch, or
// d_texels for l = 0) and where the level below reads it; acc.p[first + 1] is what the chain starts from (may be null = zeros).
__global__ void __launch_bounds__(kChainThreads) mip_chain_adjoint_kernel(ConstLevels g, Levels acc, Shape s, int first, int last) {
    const int C = s.channels;
    for (int l = first; l >= last; --l) {
        const int texels = s.h[l] * s.w[l];
        for (int e = threadIdx.x; e < texels; e += kChainThreads) {
            const int r = e / s.w[l], c = e - r * s.w[l];
            for (int ch0 = 0; ch0 < C; ch0 += kChunk) {
                const int n = C - ch0 < kChunk ? C - ch0 : kChunk;
                float v[kChunk];
                up_texel(GlobalTexels{acc.p[l + 1], s.h[l + 1], s.w[l + 1], C, ch0}, s.h[l], s.w[l], s.h[l + 1], s.w[l + 1], r, c, n, v);
                for (int k = 0; k < kChunk; ++k)
                    if (k < n) acc.p[l][(size_t)e * C + ch0 + k] = (g.p[l] ? g.p[l][(size_t)e * C + ch0 + k] : 0.f) + v[k];
            }
        }
        __syncthreads();
    }
}

// CC: channels per chunk known at compile time (1, 3), or 0 = up to kChunk of them, decided per workgroup
template <int CC>
__global__ void __launch_bounds__(256) mip_tile_kernel(Levels lv, Shape s, int b) {
    __shared__ float t1[kDown1 * kDown1 * kChunk], t2[kDown2 * kDown2 * kChunk];
    const int C = s.channels, ch0 = blockIdx.z * (CC ? CC : kChunk);
    const int cc = CC ? CC : (C - ch0 < kChunk ? C - ch0 : kChunk);
    const Tile t = forward_tile(s, b, blockIdx.y, blockIdx.x);
    const int *h = s.h + b, *w = s.w + b;
    float v[kChunk];
    {   // level b + 1 from level b (global)
        const int ncols = len(t.c1), n = len(t.r1) * ncols;
        const GlobalTexels P{lv.p[b], h[0], w[0], C, ch0};
        for (int e = threadIdx.x; e < n; e += 256) {
            const int y = e / ncols, i = t.r1.lo + y, j = t.c1.lo + (e - y * ncols);
            down_texel(P, h[0], w[0], h[1], w[1], i, j, cc, v);
            const bool own = inside(t.own1r, i) && inside(t.own1c, j);
            for (int k = 0; k < kChunk; ++k)
                if (k < cc) {
                    t1[e * cc + k] = v[k];
                    if (own) lv.p[b + 1][((size_t)i * w[1] + j) * C + ch0 + k] = v[k];
                }
        }
    }
    __syncthreads();
    {   // level b + 2 from the tile of level b + 1
        const int ncols = len(t.c2), n = len(t.r2) * ncols;
        const TileTexels P{t1, t.r1.lo, t.c1.lo, len(t.c1), cc};
        for (int e = threadIdx.x; e < n; e += 256) {
            const int y = e / ncols, i = t.r2.lo + y, j = t.c2.lo + (e - y * ncols);
            down_texel(P, h[1], w[1], h[2], w[2], i, j, cc, v);
            const bool own = inside(t.own2r, i) && inside(t.own2c, j);
            for (int k = 0; k < kChunk; ++k)
                if (k < cc) {
                    t2[e * cc + k] = v[k];
                    if (own) lv.p[b + 2][((size_t)i * w[2] + j) * C + ch0 + k] = v[k];
                }
        }
    }
    __syncthreads();
    {   // level b + 3 from the tile of level b + 2
        const int ncols = len(t.c3), n = len(t.r3) * ncols;
        const TileTexels P{t2, t.r2.lo, t.c2.lo, len(t.c2), cc};
        for (int e = threadIdx.x; e < n; e += 256) {
            const int y = e / ncols, i = t.r3.lo + y, j = t.c3.lo + (e - y * ncols);
            down_texel(P, h[2], w[2], h[3], w[3], i, j, cc, v);
            for (int k = 0; k < kChunk; ++k)
                if (k < cc) lv.p[b + 3][((size_t)i * w[3] + j) * C + ch0 + k] = v[k];
        }
    }
}

// acc_b (written to `out`: scratch, or d_texels for b = 0) of a kFineTile x kFineTile tile of level b, from acc_{b+3} in global
// memory (`top`; null = zeros): acc_{b+2} and acc_{b+1} over the tile's ranges in LDS
template <int CC>
__global__ void __launch_bounds__(256) mip_tile_adjoint_kernel(ConstLevels g, const float *top, float *out, Shape s, int b) {
    __shared__ float a1[kUp1 * kUp1 * kChunk], a2[kUp2 * kUp2 * kChunk];
    const int C = s.channels, ch0 = blockIdx.z * (CC ? CC : kChunk);
    const int cc = CC ? CC : (C - ch0 < kChunk ? C - ch0 : kChunk);
    const FineTile t = adjoint_tile(s, b, blockIdx.y, blockIdx.x);
    const int *h = s.h + b, *w = s.w + b;
    float v[kChunk];
    {   // acc_{b+2} over the tile's range of that level
        const int ncols = len(t.c2), n = len(t.r2) * ncols;
        const GlobalTexels A{top, h[3], w[3], C, ch0}, G{g.p[b + 2], h[2], w[2], C, ch0};
        for (int e = threadIdx.x; e < n; e += 256) {
            const int y = e / ncols, r = t.r2.lo + y, c = t.c2.lo + (e - y * ncols);
            up_texel(A, h[2], w[2], h[3], w[3], r, c, cc, v);
            for (int k = 0; k < kChunk; ++k)
                if (k < cc) a2[e * cc + k] = G(r, c, k) + v[k];
        }
    }
    __syncthreads();
    {   // acc_{b+1}
        const int ncols = len(t.c1), n = len(t.r1) * ncols;
        const TileTexels A{a2, t.r2.lo, t.c2.lo, len(t.c2), cc};
        const GlobalTexels G{g.p[b + 1], h[1], w[1], C, ch0};
        for (int e = threadIdx.x; e < n; e += 256) {
            const int y = e / ncols, r = t.r1.lo + y, c = t.c1.lo + (e - y * ncols);
            up_texel(A, h[1], w[1], h[2], w[2], r, c, cc, v);
            for (int k = 0; k < kChunk; ++k)
                if (k < cc) a1[e * cc + k] = G(r, c, k) + v[k];
        }
    }
    __syncthreads();
    {   // acc_b
        const int ncols = len(t.c0), n = len(t.r0) * ncols;
        const TileTexels A{a1, t.r1.lo, t.c1.lo, len(t.c1), cc};
        for (int e = threadIdx.x; e < n; e += 256) {
            const int y = e / ncols, r = t.r0.lo + y, c = t.c0.lo + (e - y * ncols);
            up_texel(A, h[0], w[0], h[1], w[1], r, c, cc, v);
            const size_t at = ((size_t)r * w[0] + c) * C + ch0;
            for (int k = 0; k < kChunk; ++k)
                if (k < cc) out[at + k] = (g.p[b] ? g.p[b][at + k] : 0.f) + v[k];
        }
    }
}
#endif

// ---- host side -------------------------------------------------------------------------------------------------------------
inline Shape make_shape(int height, int width, int channels, int levels, const char *who) {
    auto fail = [&](const std::string &what) { throw std::runtime_error(std::string(who) + ": " + what); };
    if (height <= 0 || width <= 0 || channels <= 0) fail("height, width and channels must be positive");
    if (height > 32768 || width > 32768 || (long long)height * width * channels > (long long)1 << 30)
        fail("a side of more than 32768 texels or an image of more than 2^30 floats");
    if (levels != num_levels(height, width))
        fail("num_levels is " + std::to_string(levels) + ", a " + std::to_string(height) + " x " + std::to_string(width) +
             " image has " + std::to_string(num_levels(height, width)));
    Shape s{};
    s.channels = channels;
    s.num_levels = levels;
    s.h[0] = height;
    s.w[0] = width;
    for (int l = 1; l < levels; ++l) {
        s.h[l] = s.h[l - 1] / 2 > 1 ? s.h[l - 1] / 2 : 1;
        s.w[l] = s.w[l - 1] / 2 > 1 ? s.w[l - 1] / 2 : 1;
    }
    return s;
}

// How many tiled launches (three levels each, from level 0) before one workgroup finishes the rest: a tiled launch as long as
// the level it would start from is large and three more levels exist.  0 = one chain workgroup does everything.
inline int tiled_stages(const Shape &s) {
    int stages = 0;
    while (3 * stages + 3 < s.num_levels && (long long)s.h[3 * stages] * s.w[3 * stages] * s.channels > (long long)kSmall) ++stages;
    return stages;
}
inline int chunks(const Shape &s) { return s.channels == 1 || s.channels == 3 ? 1 : (s.channels + kChunk - 1) / kChunk; }

// Every tile's ranges fit the LDS arrays (they do by the bounds above; a shape that broke them must not reach a launch).
// The ranges of rows and of columns are independent, so the tiles of one column and of one row are looked at.
inline void check_tiles(const Shape &s, int b, bool adjoint) {
    bool ok = true;
    if (!adjoint) {
        const int ty = (s.h[b + 3] + kTile - 1) / kTile, tx = (s.w[b + 3] + kTile - 1) / kTile;
        for (int y = 0; y < ty; ++y) { const Tile t = forward_tile(s, b, y, 0); ok = ok && len(t.r2) <= kDown2 && len(t.r1) <= kDown1; }
        for (int x = 0; x < tx; ++x) { const Tile t = forward_tile(s, b, 0, x); ok = ok && len(t.c2) <= kDown2 && len(t.c1) <= kDown1; }
    } else {
        const int ty = (s.h[b] + kFineTile - 1) / kFineTile, tx = (s.w[b] + kFineTile - 1) / kFineTile;
        for (int y = 0; y < ty; ++y) { const FineTile t = adjoint_tile(s, b, y, 0); ok = ok && len(t.r1) <= kUp1 && len(t.r2) <= kUp2; }
        for (int x = 0; x < tx; ++x) { const FineTile t = adjoint_tile(s, b, 0, x); ok = ok && len(t.c1) <= kUp1 && len(t.c2) <= kUp2; }
    }
    if (!ok) throw std::runtime_error("mip pyramid: a tile exceeds its LDS range (internal error)");
}

// floats of scratch rdr_mip_pyramid_backward needs: acc_l of the levels 1 .. num_levels - 2, each padded to 64 floats
inline size_t padded(const Shape &s, int l) { return (((size_t)s.h[l] * s.w[l] * s.channels) + 63) & ~(size_t)63; }
inline size_t scratch_floats(const Shape &s) {
    size_t n = 0;
    for (int l = 1; l + 1 < s.num_levels; ++l) n += padded(s, l);
    return n;
}

// rdr_mip_pyramid: levels[0] is read, levels[1 ..) are written; stream-ordered, not synchronised
inline void pyramid(int height, int width, int channels, int levels, float *const *level_ptrs) {
    const Shape s = make_shape(height, width, channels, levels, "rdr_mip_pyramid");
    if (!level_ptrs) throw std::runtime_error("rdr_mip_pyramid: levels is required");
    Levels lv{};
    for (int l = 0; l < levels; ++l) {
        if (!level_ptrs[l]) throw std::runtime_error("rdr_mip_pyramid: level " + std::to_string(l) + " is null");
        lv.p[l] = level_ptrs[l];
    }
    if (levels == 1) return;
#if !defined(RDR_HOSTSIM)
    hipStream_t stream = exec::ctx().stream;
    const int stages = tiled_stages(s);
    for (int b = 0; b < 3 * stages; b += 3) {
        check_tiles(s, b, false);
        const dim3 grid((s.w[b + 3] + kTile - 1) / kTile, (s.h[b + 3] + kTile - 1) / kTile, chunks(s));
        if (channels == 1) hipLaunchKernelGGL(mip_tile_kernel<1>, grid, dim3(256), 0, stream, lv, s, b);
        else if (channels == 3) hipLaunchKernelGGL(mip_tile_kernel<3>, grid, dim3(256), 0, stream, lv, s, b);
        else hipLaunchKernelGGL(mip_tile_kernel<0>, grid, dim3(256), 0, stream, lv, s, b);
        exec::check(hipGetLastError(), "mip_tile launch");
    }
    if (3 * stages + 1 < levels) {
        hipLaunchKernelGGL(mip_chain_kernel, dim3(1), dim3(kChainThreads), 0, stream, lv, s, 3 * stages + 1, levels - 1);
        exec::check(hipGetLastError(), "mip_chain launch");
    }
#else
    for (int l = 1; l < levels; ++l)
        for (int i = 0; i < s.h[l]; ++i)
            for (int j = 0; j < s.w[l]; ++j)
                for (int ch0 = 0; ch0 < channels; ch0 += kChunk) {
                    const int n = channels - ch0 < kChunk ? channels - ch0 : kChunk;
                    float v[kChunk];
                    down_texel(GlobalTexels{lv.p[l - 1], s.h[l - 1], s.w[l - 1], channels, ch0}, s.h[l - 1], s.w[l - 1], s.h[l], s.w[l],
                               i, j, n, v);
                    for (int k = 0; k < n; ++k) lv.p[l][((size_t)i * s.w[l] + j) * channels + ch0 + k] = v[k];
                }
#endif
}

// rdr_mip_pyramid_backward: writes every element of d_texels; d_levels[l] may be null; stream-ordered, not synchronised
inline void pyramid_backward(int height, int width, int channels, int levels, const float *const *d_levels, float *d_texels,
                             float *scratch, size_t scratch_count) {
    const Shape s = make_shape(height, width, channels, levels, "rdr_mip_pyramid_backward");
    if (!d_levels || !d_texels) throw std::runtime_error("rdr_mip_pyramid_backward: d_levels and d_texels are required");
    need_scratch("rdr_mip_pyramid_backward", scratch_floats(s), scratch, scratch_count);
    ConstLevels g{};
    Levels acc{};
    for (int l = 0; l < levels; ++l) g.p[l] = d_levels[l];
    acc.p[0] = d_texels;
    float *next = scratch;
    for (int l = 1; l + 1 < levels; ++l) { acc.p[l] = next; next += padded(s, l); }
    // the chain starts from the last level's upstream gradient itself (read only)
    if (levels > 1) acc.p[levels - 1] = const_cast<float *>(d_levels[levels - 1]);
#if !defined(RDR_HOSTSIM)
    hipStream_t stream = exec::ctx().stream;
    if (levels == 1) {
        // d_texels = g_0 (or zeros): the chain kernel with nothing above level 0
        Shape one = s;
        one.h[1] = one.w[1] = 1;
        acc.p[1] = nullptr;
        hipLaunchKernelGGL(mip_chain_adjoint_kernel, dim3(1), dim3(kChainThreads), 0, stream, g, acc, one, 0, 0);
        exec::check(hipGetLastError(), "mip_chain_adjoint launch");
        return;
    }
    // mirrored: one workgroup takes the chain down to the level the last tiled launch of the forward pass wrote, then the tiles
    const int stages = tiled_stages(s);
    if (3 * stages <= levels - 2) {
        hipLaunchKernelGGL(mip_chain_adjoint_kernel, dim3(1), dim3(kChainThreads), 0, stream, g, acc, s, levels - 2, 3 * stages);
        exec::check(hipGetLastError(), "mip_chain_adjoint launch");
    }
    for (int b = 3 * stages - 3; b >= 0; b -= 3) {
        check_tiles(s, b, true);
        const dim3 grid((s.w[b] + kFineTile - 1) / kFineTile, (s.h[b] + kFineTile - 1) / kFineTile, chunks(s));
        const float *top = acc.p[b + 3];
        if (channels == 1) hipLaunchKernelGGL(mip_tile_adjoint_kernel<1>, grid, dim3(256), 0, stream, g, top, acc.p[b], s, b);
        else if (channels == 3) hipLaunchKernelGGL(mip_tile_adjoint_kernel<3>, grid, dim3(256), 0, stream, g, top, acc.p[b], s, b);
        else hipLaunchKernelGGL(mip_tile_adjoint_kernel<0>, grid, dim3(256), 0, stream, g, top, acc.p[b], s, b);
        exec::check(hipGetLastError(), "mip_tile_adjoint launch");
    }
#else
    for (int l = levels - 2; l >= 0; --l)
        for (int r = 0; r < s.h[l]; ++r)
            for (int c = 0; c < s.w[l]; ++c)
                for (int ch0 = 0; ch0 < channels; ch0 += kChunk) {
                    const int n = channels - ch0 < kChunk ? channels - ch0 : kChunk;
                    float v[kChunk];
                    up_texel(GlobalTexels{acc.p[l + 1], s.h[l + 1], s.w[l + 1], channels, ch0}, s.h[l], s.w[l], s.h[l + 1], s.w[l + 1],
                             r, c, n, v);
                    const size_t at = ((size_t)r * s.w[l] + c) * channels + ch0;
                    for (int k = 0; k < n; ++k) acc.p[l][at + k] = (g.p[l] ? g.p[l][at + k] : 0.f) + v[k];
                }
    if (levels == 1)
        for (size_t at = 0; at < (size_t)height * width * channels; ++at) d_texels[at] = g.p[0] ? g.p[0][at] : 0.f;
#endif
}

} // namespace mip
} // namespace rdr
