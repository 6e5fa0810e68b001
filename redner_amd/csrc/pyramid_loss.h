// pyramid_loss.h -- the Gaussian image pyramid loss of the reference's optimisation scripts and its gradient
// (rdr_pyramid_loss / rdr_pyramid_loss_backward).
//
// THE MEANING.  image, target [N, H, W, C] fp32, L = num_levels >= 1, min(H, W) >> (L - 1) >= 1:
//   D_0 = image - target, each element clamped to [-c, c] when clamp = c > 0 (the derivative is 1 on the closed interval);
//   level l + 1 is floor(H_l / 2) x floor(W_l / 2):  G = D_l filtered with the 7 x 7 kernel a (x) a at ZERO padding 3,
//       D_{l+1}[y, x] = mean of G over rows 2 y, 2 y + 1 and columns 2 x, 2 x + 1     (an odd side drops the last row / column of G);
//   a = [w3 + w4, w2, w1, w0, w1, w2, w3 + w4], w_k = exp(-k^2 / 2) / sum_{k = -4 .. 4} exp(-k^2 / 2), each rounded to fp32: the
//       unit Gaussian truncated at 4 sigma, whose ninth tap a 7-tap window reflects into its ends;
//   loss = sum_l weight_l * sum_n sum(D_l^2) / ((H / 2^l) * (W / 2^l))          (true division of the level-0 sizes).
//
// THE ARITHMETIC.  The filter and the 2 x 2 mean fold into ONE 8 x 8 kernel b (x) b at stride 2, b[t] = (a[t] + a[t-1]) / 2
// (a[-1] = a[7] = 0; computed in double from the fp32 a and rounded to fp32 once, make_plan).  A coarse texel is (down_texel)
//       row_i = sum over j = 0 .. 7, ascending from 0.f, of b[j] * D_l[2 y - 3 + i, 2 x - 3 + j]     (an index outside reads 0.f)
//       D_{l+1}[y, x] = sum over i = 0 .. 7, ascending from 0.f, of b[i] * row_i
// in fp32 without contraction: 18 roundings on the path of one term (a tap, a product, eight additions, twice) beside the
// rounding of b.  The adjoint is a GATHER (up_texel): a fine texel (y, x) takes the at most 4 x 4 coarse texels (i, j),
// ceil((y - 4) / 2) <= i <= floor((y + 3) / 2) inside the level, whose footprint covers it,
//       row_i = sum over j ascending of b[x - 2 j + 3] * acc[i, j],    (A^T acc)[y, x] = sum over i ascending of b[y - 2 i + 3] * row_i
// and acc_l = coef_l * D_l + A^T acc_{l+1} with coef_l = fp32(2 weight_l / ((H / 2^l) (W / 2^l))) (double, rounded once);
// d_image = upstream * acc_0 where the clamp passes and 0 elsewhere, d_target = -d_image.  No atomics anywhere.
//
// THE SUMS OF SQUARES.  Every level is cut into kTile x kTile tiles (a function of the level's size only).  A ROW of a tile is
// summed in fp64 (each square is exact there) in ascending (column, channel) order -- chunk of kChunk channels by chunk when
// C > kChunk -- the rows of a tile are added in ascending order, the tiles of a level in ascending (image, tile row, tile
// column) order, the term of the level is double(weight_l) * sum / ((H / 2^l) (W / 2^l)) in fp64, the terms are added in
// ascending l and the total is rounded to fp32 ONCE.  Bitwise reproducible from run to run; the harness adds in the same order.
//
// THE LAUNCH PLAN.  T = tiled_levels(plan) >= 1 leading levels are "large": level 0 always, level l >= 1 while it has more than
// kSmall floats per image and the levels before it are large.
//   forward    T launches of level_kernel (level l < T: a workgroup of kThreads lanes owns a kTile x kTile tile of D_l of one
//              image; it stages the tile with its halo of 3, (kTile + 6)^2 x kChunk floats = 23 KB of LDS, forms D_0 there from
//              image and target -- each is read once plus the halo, D_0 never goes to memory --, adds the tile's squares and
//              writes its (kTile / 2)^2 texels of D_{l+1}); then, if T < L, ONE launch of chain_kernel (a workgroup of
//              kChainThreads lanes per image does the levels T .. L - 1 from memory it wrote itself, a barrier between two
//              levels); then finish_kernel (one workgroup: the L sums, the terms, the loss).  256^2 x 3, L = 5: 4 launches.
//   backward   mirrored: if T < L one launch of chain_adjoint_kernel (acc_{L-1} .. acc_T, a workgroup per image), then T
//              launches of level_adjoint_kernel, level T - 1 down to level 0: a workgroup owns a kTile x kTile tile of level l
//              and stages the (kTile / 2 + 4)^2 texels of acc_{l+1} it gathers from in LDS (6 KB); level 0 forms D_0 and the
//              clamp's mask again from image and target and writes d_image (and d_target).  `upstream` is read from device
//              memory by that last launch: nothing is synchronised.  256^2 x 3, L = 5: 3 launches.
// Scratch is the caller's: the forward call keeps D_1 .. D_{L-1} (each level [N, H_l, W_l, C], padded to 64 floats), then the
// fp64 tile sums and row sums; the backward call reads the levels from there (`saved`) and keeps acc_1 .. acc_{L-1} in the same
// layout.
//
// The per-texel bodies (difference, down_texel, up_texel, row_squares) are shared by the kernels at the end of this header and
// by the plain loops of the CPU debugging harness; a value depends only on the level before it and is computed by the same
// function in the same order wherever it is computed (global memory or an LDS tile), so harness and kernels agree bit for bit.
#pragma once
#include "../../include/redner_amd_image.h"
#include "arena.h"
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

namespace rdr {
namespace pyl {

constexpr int kMaxLevels = 16;
constexpr int kChunk = 4;                       // channels a lane holds at a time
constexpr int kTile = 32;                       // texels of level l a workgroup owns, per side
constexpr int kHalo = 3;
constexpr int kIn = kTile + 2 * kHalo;          // 38: the staged tile of D_l, per side
constexpr int kCoarse = kTile / 2 + 4;          // 20: the coarse texels 32 fine ones gather from, per side
constexpr int kThreads = 256, kChainThreads = 1024;
constexpr int kSmall = 64 * 64 * 3;             // floats per image: a level of at most this many is left to the chain workgroup

struct Plan {
    int batch, channels, num_levels, tiled;
    int h[kMaxLevels], w[kMaxLevels];
    float weight[kMaxLevels], coef[kMaxLevels];
    double count[kMaxLevels];                   // (H / 2^l) * (W / 2^l)
    long long level_off[kMaxLevels];            // floats from the start of the levels' block; [0] unused
    long long partial_off[kMaxLevels + 1];      // doubles from the start of the tile sums
    long long row_stride;                       // doubles of row sums per image (chain levels)
    float clamp;                                // 0 = none
    float b[8];
};

RDR_FN int tiles_x(const Plan &p, int l) { return (p.w[l] + kTile - 1) / kTile; }
RDR_FN int tiles_y(const Plan &p, int l) { return (p.h[l] + kTile - 1) / kTile; }
RDR_FN int tiles(const Plan &p, int l) { return tiles_x(p, l) * tiles_y(p, l); }
RDR_FN long long level_floats(const Plan &p, int l) { return (long long)p.batch * p.h[l] * p.w[l] * p.channels; }
RDR_FN long long image_floats(const Plan &p, int l) { return (long long)p.h[l] * p.w[l] * p.channels; }

RDR_FN float difference(float a, float b, float clamp) {
    float d = a - b;
    if (clamp > 0.f) d = d < -clamp ? -clamp : (d > clamp ? clamp : d);
    return d;
}
RDR_FN bool passes(float a, float b, float clamp) {
    const float d = a - b;
    return !(clamp > 0.f) || (d >= -clamp && d <= clamp);
}

// One level of one image, channels [ch0, ...): texels(r, c, k); an index outside the level reads 0.f.
struct GlobalTexels {
    const float *p;
    int h, w, channels, ch0;
    RDR_FN float operator()(int r, int c, int k) const {
        return (r >= 0 && r < h && c >= 0 && c < w) ? p[((size_t)r * w + c) * channels + ch0 + k] : 0.f;
    }
};
// D_0 of one image, formed where it is read
struct DiffTexels {
    const float *image, *target;
    int h, w, channels, ch0;
    float clamp;
    RDR_FN float operator()(int r, int c, int k) const {
        if (!(r >= 0 && r < h && c >= 0 && c < w)) return 0.f;
        const size_t at = ((size_t)r * w + c) * channels + ch0 + k;
        return difference(image[at], target[at], clamp);
    }
};
// A staged tile [r0, ...) x [c0, c0 + ncols) x cc (LDS); what lies outside the level was staged as 0.f
struct TileTexels {
    const float *p;
    int r0, c0, ncols, cc;
    RDR_FN float operator()(int r, int c, int k) const { return p[((r - r0) * ncols + (c - c0)) * cc + k]; }
};

// out[k] = D_{l+1}[y, x], channel k < n <= kChunk of P's chunk, from the level P
template <class F>
RDR_FN void down_texel(const F &P, const float *b, int y, int x, int n, float *out) {
    float acc[kChunk] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 8; ++i) {
        float row[kChunk] = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < 8; ++j)
            for (int k = 0; k < kChunk; ++k)
                if (k < n) row[k] = row[k] + b[j] * P(2 * y - 3 + i, 2 * x - 3 + j, k);
        for (int k = 0; k < kChunk; ++k)
            if (k < n) acc[k] = acc[k] + b[i] * row[k];
    }
    for (int k = 0; k < kChunk; ++k)
        if (k < n) out[k] = acc[k];
}

// out[k] = (A^T acc)[y, x]: what the fine texel (y, x) gathers from the coarse level ACC of size hc x wc
template <class F>
RDR_FN void up_texel(const F &ACC, const float *b, int hc, int wc, int y, int x, int n, float *out) {
    int i0 = (y - 3) >> 1, i1 = (y + 3) >> 1, j0 = (x - 3) >> 1, j1 = (x + 3) >> 1;     // ceil((y - 4) / 2) .. floor((y + 3) / 2)
    if (i0 < 0) i0 = 0;
    if (j0 < 0) j0 = 0;
    if (i1 > hc - 1) i1 = hc - 1;
    if (j1 > wc - 1) j1 = wc - 1;
    float acc[kChunk] = {0.f, 0.f, 0.f, 0.f};
    for (int i = i0; i <= i1; ++i) {
        float row[kChunk] = {0.f, 0.f, 0.f, 0.f};
        for (int j = j0; j <= j1; ++j)
            for (int k = 0; k < kChunk; ++k)
                if (k < n) row[k] = row[k] + b[x - 2 * j + 3] * ACC(i, j, k);
        for (int k = 0; k < kChunk; ++k)
            if (k < n) acc[k] = acc[k] + b[y - 2 * i + 3] * row[k];
    }
    for (int k = 0; k < kChunk; ++k)
        if (k < n) out[k] = acc[k];
}

// acc += the squares of row r, columns [c0, c1), the n channels of P's chunk
template <class F>
RDR_FN void row_squares(const F &P, int r, int c0, int c1, int n, double &acc) {
    for (int c = c0; c < c1; ++c)
        for (int k = 0; k < kChunk; ++k)
            if (k < n) {
                const double d = (double)P(r, c, k);
                acc += d * d;
            }
}

// what the finish does with the tile sums (partial): sums[l], the terms and the loss
RDR_FN double level_sum(const Plan &p, const double *partial, int l) {
    const long long n = p.partial_off[l + 1] - p.partial_off[l];
    double s = 0.0;
    for (long long q = 0; q < n; ++q) s += partial[p.partial_off[l] + q];
    return s;
}
RDR_FN double level_term(const Plan &p, int l, double sum) { return (double)p.weight[l] * sum / p.count[l]; }

#if !defined(RDR_HOSTSIM)
// ---- gfx950 kernels --------------------------------------------------------------------------------------------------------
// Level l < tiled of image blockIdx.z, tile (blockIdx.y, blockIdx.x): the tile's sum of squares, and its texels of D_{l+1}.
// FIRST: level 0, formed from image and target.
template <bool FIRST>
__global__ void __launch_bounds__(kThreads) level_kernel(Plan p, int l, const float *image, const float *target, float *levels,
                                                         double *partial) {
    __shared__ float tile[kIn * kIn * kChunk];
    __shared__ double rows[kTile];
    const int t = threadIdx.x, n = blockIdx.z, C = p.channels, h = p.h[l], w = p.w[l];
    const int r0 = blockIdx.y * kTile, c0 = blockIdx.x * kTile;
    const int nrows = h - r0 < kTile ? h - r0 : kTile, ncols = w - c0 < kTile ? w - c0 : kTile;
    const bool next = l + 1 < p.num_levels;
    const int h1 = next ? p.h[l + 1] : 0, w1 = next ? p.w[l + 1] : 0;
    const int y = r0 / 2 + t / (kTile / 2), x = c0 / 2 + t % (kTile / 2);           // this lane's texel of D_{l+1}
    const size_t image_at = (size_t)n * image_floats(p, l);
    const float *src = FIRST ? nullptr : levels + p.level_off[l] + image_at;
    float *dst = next ? levels + p.level_off[l + 1] + (size_t)n * image_floats(p, l + 1) : nullptr;
    double acc = 0.0;                                                               // lanes 0 .. nrows - 1: the sum of row r0 + t
    for (int ch0 = 0; ch0 < C; ch0 += kChunk) {
        const int cc = C - ch0 < kChunk ? C - ch0 : kChunk;
        for (int e = t; e < kIn * kIn * cc; e += kThreads) {
            const int px = e / cc, k = e - px * cc, yy = px / kIn, xx = px - yy * kIn;
            const int r = r0 - kHalo + yy, c = c0 - kHalo + xx;
            float v = 0.f;
            if (r >= 0 && r < h && c >= 0 && c < w) {
                const size_t at = ((size_t)r * w + c) * C + ch0 + k;
                v = FIRST ? difference(image[image_at + at], target[image_at + at], p.clamp) : src[at];
            }
            tile[e] = v;
        }
        __syncthreads();
        const TileTexels P{tile, r0 - kHalo, c0 - kHalo, kIn, cc};
        if (t < nrows) row_squares(P, r0 + t, c0, c0 + ncols, cc, acc);
        if (next && y < h1 && x < w1) {
            float v[kChunk];
            down_texel(P, p.b, y, x, cc, v);
            for (int k = 0; k < kChunk; ++k)
                if (k < cc) dst[((size_t)y * w1 + x) * C + ch0 + k] = v[k];
        }
        __syncthreads();
    }
    if (t < kTile) rows[t] = t < nrows ? acc : 0.0;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int r = 0; r < nrows; ++r) s += rows[r];
        partial[p.partial_off[l] + (size_t)n * tiles(p, l) + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// Levels tiled .. L - 1 of image blockIdx.x by ONE workgroup: the row sums and tile sums of each and the level after it, each
// from memory this workgroup wrote (or, for level `tiled`, the launch before it): a barrier orders the stores before the loads.
__global__ void __launch_bounds__(kChainThreads) chain_kernel(Plan p, float *levels, double *partial, double *rowsum) {
    const int t = threadIdx.x, n = blockIdx.x, C = p.channels;
    double *rs = rowsum + (size_t)n * p.row_stride;
    for (int l = p.tiled; l < p.num_levels; ++l) {
        const int h = p.h[l], w = p.w[l], tx = tiles_x(p, l);
        const float *src = levels + p.level_off[l] + (size_t)n * image_floats(p, l);
        for (int e = t; e < h * tx; e += kChainThreads) {
            const int r = e / tx, c0 = (e - r * tx) * kTile, c1 = c0 + kTile < w ? c0 + kTile : w;
            double acc = 0.0;
            for (int ch0 = 0; ch0 < C; ch0 += kChunk)
                row_squares(GlobalTexels{src, h, w, C, ch0}, r, c0, c1, C - ch0 < kChunk ? C - ch0 : kChunk, acc);
            rs[e] = acc;
        }
        if (l + 1 < p.num_levels) {
            const int h1 = p.h[l + 1], w1 = p.w[l + 1];
            float *dst = levels + p.level_off[l + 1] + (size_t)n * image_floats(p, l + 1);
            for (int e = t; e < h1 * w1; e += kChainThreads) {
                const int y = e / w1, x = e - y * w1;
                for (int ch0 = 0; ch0 < C; ch0 += kChunk) {
                    const int cc = C - ch0 < kChunk ? C - ch0 : kChunk;
                    float v[kChunk];
                    down_texel(GlobalTexels{src, h, w, C, ch0}, p.b, y, x, cc, v);
                    for (int k = 0; k < kChunk; ++k)
                        if (k < cc) dst[(size_t)e * C + ch0 + k] = v[k];
                }
            }
        }
        __syncthreads();
        for (int e = t; e < tiles(p, l); e += kChainThreads) {
            const int ty = e / tx, r1 = (ty + 1) * kTile < h ? (ty + 1) * kTile : h;
            double s = 0.0;
            for (int r = ty * kTile; r < r1; ++r) s += rs[(size_t)r * tx + (e - ty * tx)];
            partial[p.partial_off[l] + (size_t)n * tiles(p, l) + e] = s;
        }
        __syncthreads();
    }
}

// loss[0] (fp32) and, when not null, terms[L] (fp64) from the tile sums: lane l adds the sums of level l in ascending order
__global__ void __launch_bounds__(64) finish_kernel(Plan p, const double *partial, float *loss, double *terms) {
    __shared__ double term[kMaxLevels];
    const int l = threadIdx.x;
    if (l < p.num_levels) term[l] = level_term(p, l, level_sum(p, partial, l));
    __syncthreads();
    if (l == 0) {
        double total = 0.0;
        for (int q = 0; q < p.num_levels; ++q) {
            total += term[q];
            if (terms) terms[q] = term[q];
        }
        loss[0] = (float)total;
    }
}

// acc_l = coef_l * D_l + A^T acc_{l+1} for l = L - 1 down to max(tiled, 1), image blockIdx.x, by one workgroup
__global__ void __launch_bounds__(kChainThreads) chain_adjoint_kernel(Plan p, const float *levels, float *acc) {
    const int t = threadIdx.x, n = blockIdx.x, C = p.channels, last = p.tiled > 1 ? p.tiled : 1;
    for (int l = p.num_levels - 1; l >= last; --l) {
        const int h = p.h[l], w = p.w[l];
        const bool top = l + 1 == p.num_levels;
        const int hc = top ? 0 : p.h[l + 1], wc = top ? 0 : p.w[l + 1];
        const size_t at0 = p.level_off[l] + (size_t)n * image_floats(p, l);
        const float *coarse = top ? nullptr : acc + p.level_off[l + 1] + (size_t)n * image_floats(p, l + 1);
        for (int e = t; e < h * w; e += kChainThreads) {
            const int y = e / w, x = e - y * w;
            for (int ch0 = 0; ch0 < C; ch0 += kChunk) {
                const int cc = C - ch0 < kChunk ? C - ch0 : kChunk;
                float v[kChunk] = {0.f, 0.f, 0.f, 0.f};
                if (!top) up_texel(GlobalTexels{coarse, hc, wc, C, ch0}, p.b, hc, wc, y, x, cc, v);
                for (int k = 0; k < kChunk; ++k)
                    if (k < cc) acc[at0 + (size_t)e * C + ch0 + k] = p.coef[l] * levels[at0 + (size_t)e * C + ch0 + k] + v[k];
            }
        }
        __syncthreads();
    }
}

// acc_l of a kTile x kTile tile of level l < tiled of image blockIdx.z; FIRST: level 0, written as d_image (and d_target)
template <bool FIRST>
__global__ void __launch_bounds__(kThreads) level_adjoint_kernel(Plan p, int l, const float *image, const float *target,
                                                                 const float *levels, float *acc, const float *upstream,
                                                                 float *d_image, float *d_target) {
    __shared__ float tile[kCoarse * kCoarse * kChunk];
    const int t = threadIdx.x, n = blockIdx.z, C = p.channels, h = p.h[l], w = p.w[l];
    const int r0 = blockIdx.y * kTile, c0 = blockIdx.x * kTile;
    const int nrows = h - r0 < kTile ? h - r0 : kTile, ncols = w - c0 < kTile ? w - c0 : kTile;
    const bool top = l + 1 == p.num_levels;
    const int hc = top ? 0 : p.h[l + 1], wc = top ? 0 : p.w[l + 1];
    const int i0 = r0 / 2 - 2, j0 = c0 / 2 - 2;                                     // the staged coarse texels start here
    const float *coarse = top ? nullptr : acc + p.level_off[l + 1] + (size_t)n * image_floats(p, l + 1);
    const size_t at0 = (FIRST ? 0 : p.level_off[l]) + (size_t)n * image_floats(p, l);
    const float up = FIRST ? upstream[0] : 0.f;
    for (int ch0 = 0; ch0 < C; ch0 += kChunk) {
        const int cc = C - ch0 < kChunk ? C - ch0 : kChunk;
        if (!top)
            for (int e = t; e < kCoarse * kCoarse * cc; e += kThreads) {
                const int px = e / cc, k = e - px * cc, yy = px / kCoarse, xx = px - yy * kCoarse;
                const int i = i0 + yy, j = j0 + xx;
                tile[e] = (i >= 0 && i < hc && j >= 0 && j < wc) ? coarse[((size_t)i * wc + j) * C + ch0 + k] : 0.f;
            }
        __syncthreads();
        const TileTexels A{tile, i0, j0, kCoarse, cc};
        for (int e = t; e < nrows * ncols; e += kThreads) {
            const int yy = e / ncols, y = r0 + yy, x = c0 + (e - yy * ncols);
            float v[kChunk] = {0.f, 0.f, 0.f, 0.f};
            if (!top) up_texel(A, p.b, hc, wc, y, x, cc, v);
            const size_t at = at0 + ((size_t)y * w + x) * C + ch0;
            for (int k = 0; k < kChunk; ++k)
                if (k < cc) {
                    if (FIRST) {
                        const float a = image[at + k], b = target[at + k];
                        const float g = passes(a, b, p.clamp) ? up * (p.coef[0] * difference(a, b, p.clamp) + v[k]) : 0.f;
                        d_image[at + k] = g;
                        if (d_target) d_target[at + k] = -g;
                    } else {
                        acc[at + k] = p.coef[l] * levels[at + k] + v[k];
                    }
                }
        }
        __syncthreads();
    }
}
#endif

// ---- host side -------------------------------------------------------------------------------------------------------------
inline long long padded(long long floats) { return (floats + 63) & ~(long long)63; }

// how many leading levels the tiled kernels do: level 0, and every level after it that is large while the ones before it are
inline int tiled_levels(const Plan &p) {
    int t = 1;
    while (t < p.num_levels && image_floats(p, t) > (long long)kSmall) ++t;
    return t;
}

inline Plan make_plan(int batch, int height, int width, int channels, int levels, const float *weights, float clamp, const char *who) {
    auto fail = [&](const std::string &what) { throw std::runtime_error(std::string(who) + ": " + what); };
    if (batch <= 0 || height <= 0 || width <= 0 || channels <= 0) fail("batch, height, width and channels must be positive");
    if (height > 32768 || width > 32768 || batch > 65535 || (long long)batch * height * width * channels > (long long)1 << 30)
        fail("a side of more than 32768 pixels, more than 65535 images or more than 2^30 floats");
    if (levels < 1) fail("num_levels must be at least 1");
    if (levels > kMaxLevels || ((height < width ? height : width) >> (levels - 1)) < 1)
        fail("too many levels: " + std::to_string(levels) + " for " + std::to_string(height) + " x " + std::to_string(width) +
             " (the smaller side must stay at least 1 texel)");
    if (!(clamp >= 0.f)) fail("clamp must be positive (0 = none)");
    Plan p{};
    p.batch = batch; p.channels = channels; p.num_levels = levels; p.clamp = clamp;
    long long off = 0, poff = 0;
    for (int l = 0; l < levels; ++l) {
        p.h[l] = l ? p.h[l - 1] / 2 : height;
        p.w[l] = l ? p.w[l - 1] / 2 : width;
        p.count[l] = ((double)height / (double)(1 << l)) * ((double)width / (double)(1 << l));
        p.weight[l] = weights ? weights[l] : 1.f;
        p.coef[l] = (float)(2.0 * (double)p.weight[l] / p.count[l]);
        if (l) { p.level_off[l] = off; off += padded(level_floats(p, l)); }
        p.partial_off[l] = poff;
        poff += (long long)batch * tiles(p, l);
    }
    p.partial_off[levels] = poff;
    p.tiled = tiled_levels(p);
    p.row_stride = p.tiled < levels ? (long long)p.h[p.tiled] * tiles_x(p, p.tiled) : 0;
    // the taps: the unit Gaussian truncated at 4 sigma and reflected into a window of 7, then folded with the 2 x 2 mean
    double wk[5], sum = 0.0;
    for (int k = 0; k <= 4; ++k) { wk[k] = std::exp(-0.5 * k * k); sum += (k ? 2.0 : 1.0) * wk[k]; }
    const float a[7] = {(float)((wk[3] + wk[4]) / sum), (float)(wk[2] / sum), (float)(wk[1] / sum), (float)(wk[0] / sum),
                        (float)(wk[1] / sum), (float)(wk[2] / sum), (float)((wk[3] + wk[4]) / sum)};
    for (int t = 0; t < 8; ++t) p.b[t] = (float)(0.5 * ((t < 7 ? (double)a[t] : 0.0) + (t > 0 ? (double)a[t - 1] : 0.0)));
    return p;
}

// floats of the levels' block: D_1 .. D_{L-1} (forward scratch, `saved`) or acc_1 .. acc_{L-1} (backward scratch)
inline long long levels_floats(const Plan &p) {
    return p.num_levels > 1 ? p.level_off[p.num_levels - 1] + padded(level_floats(p, p.num_levels - 1)) : 0;
}
// floats of scratch of the forward call: the levels, the fp64 tile sums, the fp64 row sums of the chain levels
inline long long forward_floats(const Plan &p) {
    return levels_floats(p) + 2 * (p.partial_off[p.num_levels] + (long long)p.batch * p.row_stride);
}
inline long long backward_floats(const Plan &p) { return levels_floats(p); }

// rdr_pyramid_loss: writes loss[0], terms[L] (when not null) and the levels at the start of scratch; stream-ordered, not synchronised
inline void forward(const Plan &p, const float *image, const float *target, float *loss, double *terms, float *scratch,
                    size_t scratch_count) {
    if (!image || !target || !loss) throw std::runtime_error("rdr_pyramid_loss: image, target and loss are required");
    need_scratch("rdr_pyramid_loss", (size_t)forward_floats(p), scratch, scratch_count, true);
    float *levels = scratch;
    double *partial = reinterpret_cast<double *>(scratch + levels_floats(p));
    double *rowsum = partial + p.partial_off[p.num_levels];
    const int L = p.num_levels;
#if !defined(RDR_HOSTSIM)
    hipStream_t stream = exec::ctx().stream;
    for (int l = 0; l < p.tiled; ++l) {
        const dim3 grid(tiles_x(p, l), tiles_y(p, l), p.batch);
        if (l == 0) hipLaunchKernelGGL(level_kernel<true>, grid, dim3(kThreads), 0, stream, p, l, image, target, levels, partial);
        else hipLaunchKernelGGL(level_kernel<false>, grid, dim3(kThreads), 0, stream, p, l, image, target, levels, partial);
        exec::check(hipGetLastError(), "pyramid_loss level launch");
    }
    if (p.tiled < L) {
        hipLaunchKernelGGL(chain_kernel, dim3(p.batch), dim3(kChainThreads), 0, stream, p, levels, partial, rowsum);
        exec::check(hipGetLastError(), "pyramid_loss chain launch");
    }
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(64), 0, stream, p, (const double *)partial, loss, terms);
    exec::check(hipGetLastError(), "pyramid_loss finish launch");
#else
    (void)rowsum;
    const int C = p.channels;
    for (int l = 0; l < L; ++l)
        for (int n = 0; n < p.batch; ++n) {
            const int h = p.h[l], w = p.w[l];
            const size_t at0 = (size_t)n * image_floats(p, l);
            const float *src = l ? levels + p.level_off[l] + at0 : nullptr;
            // a texel of this level by the accessor its kernel uses (the values are the same through either)
            auto each_chunk = [&](auto &&body) {
                for (int ch0 = 0; ch0 < C; ch0 += kChunk) {
                    const int cc = C - ch0 < kChunk ? C - ch0 : kChunk;
                    if (l == 0) body(DiffTexels{image + at0, target + at0, h, w, C, ch0, p.clamp}, ch0, cc);
                    else body(GlobalTexels{src, h, w, C, ch0}, ch0, cc);
                }
            };
            for (int ty = 0; ty < tiles_y(p, l); ++ty)
                for (int tx = 0; tx < tiles_x(p, l); ++tx) {
                    const int r1 = (ty + 1) * kTile < h ? (ty + 1) * kTile : h, c1 = (tx + 1) * kTile < w ? (tx + 1) * kTile : w;
                    double s = 0.0;
                    for (int r = ty * kTile; r < r1; ++r) {
                        double acc = 0.0;
                        each_chunk([&](const auto &P, int, int cc) { row_squares(P, r, tx * kTile, c1, cc, acc); });
                        s += acc;
                    }
                    partial[p.partial_off[l] + (size_t)n * tiles(p, l) + (size_t)ty * tiles_x(p, l) + tx] = s;
                }
            if (l + 1 < L) {
                const int h1 = p.h[l + 1], w1 = p.w[l + 1];
                float *dst = levels + p.level_off[l + 1] + (size_t)n * image_floats(p, l + 1);
                for (int y = 0; y < h1; ++y)
                    for (int x = 0; x < w1; ++x)
                        each_chunk([&](const auto &P, int ch0, int cc) {
                            float v[kChunk];
                            down_texel(P, p.b, y, x, cc, v);
                            for (int k = 0; k < cc; ++k) dst[((size_t)y * w1 + x) * C + ch0 + k] = v[k];
                        });
            }
        }
    double total = 0.0;
    for (int l = 0; l < L; ++l) {
        const double term = level_term(p, l, level_sum(p, partial, l));
        total += term;
        if (terms) terms[l] = term;
    }
    loss[0] = (float)total;
#endif
}

// rdr_pyramid_loss_backward: writes every element of d_image and (when not null) d_target; stream-ordered, not synchronised
inline void backward(const Plan &p, const float *image, const float *target, const float *saved, size_t saved_count,
                     const float *upstream, float *d_image, float *d_target, float *scratch, size_t scratch_count) {
    if (!image || !target || !upstream || !d_image)
        throw std::runtime_error("rdr_pyramid_loss_backward: image, target, upstream and d_image are required");
    if (levels_floats(p) > 0 && (!saved || saved_count < (size_t)levels_floats(p)))
        throw std::runtime_error("rdr_pyramid_loss_backward: saved must hold the " + std::to_string(levels_floats(p)) +
                                 " floats of levels the forward call left at the start of its scratch");
    need_scratch("rdr_pyramid_loss_backward", (size_t)backward_floats(p), scratch, scratch_count);
    const int L = p.num_levels;
#if !defined(RDR_HOSTSIM)
    hipStream_t stream = exec::ctx().stream;
    if (L > 1 && p.tiled < L) {
        hipLaunchKernelGGL(chain_adjoint_kernel, dim3(p.batch), dim3(kChainThreads), 0, stream, p, saved, scratch);
        exec::check(hipGetLastError(), "pyramid_loss chain adjoint launch");
    }
    for (int l = p.tiled - 1; l >= 0; --l) {
        const dim3 grid(tiles_x(p, l), tiles_y(p, l), p.batch);
        if (l == 0)
            hipLaunchKernelGGL(level_adjoint_kernel<true>, grid, dim3(kThreads), 0, stream, p, l, image, target, saved, scratch, upstream,
                               d_image, d_target);
        else
            hipLaunchKernelGGL(level_adjoint_kernel<false>, grid, dim3(kThreads), 0, stream, p, l, image, target, saved, scratch, upstream,
                               d_image, d_target);
        exec::check(hipGetLastError(), "pyramid_loss level adjoint launch");
    }
#else
    const int C = p.channels;
    const float up = upstream[0];
    for (int l = L - 1; l >= 0; --l)
        for (int n = 0; n < p.batch; ++n) {
            const int h = p.h[l], w = p.w[l];
            const bool top = l + 1 == L;
            const int hc = top ? 0 : p.h[l + 1], wc = top ? 0 : p.w[l + 1];
            const float *coarse = top ? nullptr : scratch + p.level_off[l + 1] + (size_t)n * image_floats(p, l + 1);
            const size_t at0 = (l ? p.level_off[l] : 0) + (size_t)n * image_floats(p, l);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x)
                    for (int ch0 = 0; ch0 < C; ch0 += kChunk) {
                        const int cc = C - ch0 < kChunk ? C - ch0 : kChunk;
                        float v[kChunk] = {0.f, 0.f, 0.f, 0.f};
                        if (!top) up_texel(GlobalTexels{coarse, hc, wc, C, ch0}, p.b, hc, wc, y, x, cc, v);
                        const size_t at = at0 + ((size_t)y * w + x) * C + ch0;
                        for (int k = 0; k < cc; ++k) {
                            if (l == 0) {
                                const float a = image[at + k], b = target[at + k];
                                const float g = passes(a, b, p.clamp) ? up * (p.coef[0] * difference(a, b, p.clamp) + v[k]) : 0.f;
                                d_image[at + k] = g;
                                if (d_target) d_target[at + k] = -g;
                            } else {
                                scratch[at + k] = p.coef[l] * saved[at + k] + v[k];
                            }
                        }
                    }
        }
#endif
}

} // namespace pyl
} // namespace rdr
