// sh_envmap.h -- an environment map from spherical-harmonic coefficients, its adjoint, and the sampling tables of an environment
// map (rdr_sh_reconstruct / rdr_sh_reconstruct_backward / rdr_envmap_tables).
//
// (a) SH reconstruction.  The meaning is that of pyredner/utils.py:10-60 (SH_reconstruct), operation by operation in the same
// fp32 order.  coeffs [C, N] fp32, an image of H x W, L = int(sqrt(N)) bands, 1 <= L <= 8; the columns >= L * L are not read.
//   theta_r = fp32(pi / H) * (r + 0.5f),  phi_c = fp32(2 pi / W) * (c + 0.5f),  x_r = cos(theta_r)
//   P_l^m(x), 0 <= m <= l, by the reference's recurrence (every scalar an fp32 constant):
//       somx2 = sqrt((1 - x) * (1 + x));   P_m^m: pmm = 1, then m times pmm = (pmm * -(2 k - 1)) * somx2, k = 1 .. m
//       P_{m+1}^m = (x * (2 m + 1)) * P_m^m;   P_ll^m = ((((2 ll - 1) * x) * P_{ll-1}^m) - ((ll + m - 1) * P_{ll-2}^m)) / (ll - m)
//   K_l^m = sqrt((2 l + 1) (l - m)! / (4 pi (l + m)!)) and sqrt(2) K_l^m in double on the host, rounded to fp32 ONCE (make_plan)
//   Y_i, i = l * l + l + m:   K * P_l^0 (m = 0),   (K' * cos(fp32(m) * phi)) * P_l^m (m > 0),   (K' * sin(fp32(-m) * phi)) * P_l^-m (m < 0)
//   acc = 0; acc = acc + Y_i * coeffs[ch, i] in ascending i;   out[r, c, ch] = max(acc, 0)
// The basis is a product of a ROW factor (P_l^|m|(x_r): L * L values per row, row_factors) and a COLUMN factor (cos / sin of
// |m| phi_c: 2 L - 1 values per column, col_factors); a workgroup computes the factors of its tile's rows and columns once into
// LDS, after which a pixel costs L * L * (2 + 2 C) multiplications and additions (basis()).  cos and sin are the fp64 routines of
// libm_exact.h rounded to fp32 (as in vertex_normal.h): they are only evaluated for the factors, and every build and the CPU
// harness compute the same bits.
//
// (b) Its adjoint.  d_coeffs[ch, i] = sum over the pixels of Y_i(r, c) * (g[r, c, ch] * w(r, c, ch)); w is the derivative of the
// clamp as torch.max(a, 0) has it: 1 where the unclamped sum is > 0, 0 where it is < 0 and 0.5 at a tie (all-zero coefficients:
// every pixel).  The forward call saves w as one byte per element (2 w).  A REDUCTION in a fixed order, no float atomics: the
// image is cut into kTile x kTile tiles (a function of H and W only); per tile and (i, ch) the terms double(Y_i) * double(g * w)
// -- each exact in fp64 -- are added in row-major order of the tile's pixels into an fp64 partial sum, the partials go to scratch
// [tiles][C][L * L], and a second kernel adds them in ascending tile id and rounds to fp32 once.  Columns >= L * L get 0.
// Bitwise reproducible from run to run; the harness adds in the same order and computes the same bits.
//
// (c) Sampling tables.  The meaning is that of pyredner/envmap.py:36-60 with its cumsum as torch computes it on the CPU: a
// sequential fp64 accumulator rounded to fp32 at every output.  texels [H, W, 3] fp32, y_weight [H] fp32 (the caller's):
//   lum = (0.212671f * r + 0.715160f * g) + 0.072169f * b
//   cx_[y, x] = fp32(double accumulator over lum[y, 0 .. x]);   cy_[y] = fp32(double accumulator over fp32(cx_[y, W-1] * y_weight[y]))
//   sample_cdf_xs = (cx_ - cx_[:, 0]) / max(cx_[:, W-1], 1e-8f);   sample_cdf_ys = (cy_ - cy_[0]) / max(cy_[H-1], 1e-8f)
// and cy_[H-1] goes back to the host (pdf_norm).  THE SUMMATION ORDER IS THE DEFINITION (a table entry that differs in its last
// bit moves an importance sample into the neighbouring texel), so there is no parallel scan: one lane carries a row's
// accumulator while its workgroup stages kScanCols-column tiles of kScanRows rows through LDS (coalesced reads and writes), and
// the column pass is one lane's walk over H values in a second launch.
#pragma once
#include "../../include/redner_amd.h"
#include "arena.h"
#include "vecmath.h"
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

namespace rdr {
namespace shenv {

constexpr int kMaxBands = 8, kMaxBasis = kMaxBands * kMaxBands, kMaxTrig = 2 * kMaxBands - 1;
constexpr int kChunk = 4;            // channels a lane holds at a time
constexpr int kTile = 32;            // a workgroup's pixels: kTile x kTile
constexpr int kThreads = 256;
constexpr int kScanRows = 16, kScanCols = 64;

// What a launch knows: sizes, the two angle steps and the normalisation constants (k[i]: K for m = 0, sqrt(2) K otherwise).
struct Plan {
    int height, width, channels, num_coeffs, bands;
    float theta_step, phi_step;
    float k[kMaxBasis];
};

RDR_FN int basis_count(const Plan &p) { return p.bands * p.bands; }
RDR_FN int tiles_x(const Plan &p) { return (p.width + kTile - 1) / kTile; }
RDR_FN int tiles_y(const Plan &p) { return (p.height + kTile - 1) / kTile; }

// out[l * l + l + m] = out[l * l + l - m] = P_l^m(cos(theta_r)), 0 <= m <= l < bands
RDR_FN void row_factors(const Plan &p, int r, float *out) {
    const float theta = p.theta_step * ((float)r + 0.5f);
    const float x = (float)gm::cos((double)theta);
    const float somx2 = sqrtf((1.f - x) * (1.f + x));
    float pmm = 1.f;
    for (int m = 0; m < p.bands; ++m) {
        if (m > 0) pmm = (pmm * -(float)(2 * m - 1)) * somx2;
        float below = pmm, at = pmm;                     // P_{l-1}^m (for l > m) and P_l^m
        for (int l = m; l < p.bands; ++l) {
            if (l == m + 1) at = (x * (float)(2 * m + 1)) * pmm;
            else if (l > m + 1) {
                const float pll = ((((float)(2 * l - 1) * x) * at) - ((float)(l + m - 1) * below)) / (float)(l - m);
                below = at;
                at = pll;
            }
            out[l * l + l + m] = at;
            out[l * l + l - m] = at;
        }
    }
}

// the column factor of order m, -bands < m < bands, kept at [bands - 1 + m]: cos(fp32(m) * phi_c) for m > 0, sin(fp32(-m) * phi_c) for m < 0
RDR_FN float col_factor(const Plan &p, int c, int m) {
    const float phi = p.phi_step * ((float)c + 0.5f);
    if (m == 0) return 1.f;
    return m > 0 ? (float)gm::cos((double)((float)m * phi)) : (float)gm::sin((double)((float)(-m) * phi));
}

// Y_i from the factors of the pixel's row (P) and column (T)
RDR_FN float basis(const Plan &p, const float *P, const float *T, int i, int m) {
    return m == 0 ? p.k[i] * P[i] : (p.k[i] * T[p.bands - 1 + m]) * P[i];
}

// One pixel, the channels [ch0, ch0 + n), n <= kChunk: out[k] = max(acc, 0), weight[k] = 2 * d max(acc, 0) / d acc.
// coeffs(k, i): the coefficient of channel ch0 + k.
template <class F>
RDR_FN void pixel(const Plan &p, const float *P, const float *T, const F &coeffs, int n, float *out, uint8_t *weight) {
    float acc[kChunk] = {0.f, 0.f, 0.f, 0.f};
    int i = 0;
    for (int l = 0; l < p.bands; ++l)
        for (int m = -l; m <= l; ++m, ++i) {
            const float y = basis(p, P, T, i, m);
            for (int k = 0; k < kChunk; ++k)
                if (k < n) acc[k] = acc[k] + y * coeffs(k, i);
        }
    for (int k = 0; k < kChunk; ++k)
        if (k < n) {
            out[k] = acc[k] > 0.f ? acc[k] : (acc[k] != acc[k] ? acc[k] : 0.f);
            weight[k] = acc[k] > 0.f ? 2 : (acc[k] == 0.f ? 1 : 0);
        }
}
RDR_FN float clamp_weight(uint8_t w) { return 0.5f * (float)w; }

struct GlobalCoeffs {
    const float *p; int stride, ch0;
    RDR_FN float operator()(int k, int i) const { return p[(size_t)(ch0 + k) * stride + i]; }
};
struct TileCoeffs {
    const float *p; int count;
    RDR_FN float operator()(int k, int i) const { return p[k * count + i]; }
};

RDR_FN float luminance(const float *t) { return (0.212671f * t[0] + 0.715160f * t[1]) + 0.072169f * t[2]; }
RDR_FN float normalised(float v, float first, float last) { return (v - first) / (last > 1e-8f ? last : 1e-8f); }

#if !defined(RDR_HOSTSIM)
// ---- gfx950 kernels --------------------------------------------------------------------------------------------------------
// The factors of the tile (blockIdx.y, blockIdx.x) into LDS: rows[y * nb + i], cols[x * (2 bands - 1) + j].  Returns after a barrier.
__device__ inline void tile_factors(const Plan &p, int r0, int nrows, int c0, int ncols, float *rows, float *cols) {
    const int nb = basis_count(p), nt = 2 * p.bands - 1;
    for (int e = threadIdx.x; e < nrows + ncols * nt; e += kThreads) {
        if (e < nrows) row_factors(p, r0 + e, rows + e * nb);
        else {
            const int x = (e - nrows) / nt, j = (e - nrows) - x * nt;
            cols[x * nt + j] = col_factor(p, c0 + x, j - (p.bands - 1));
        }
    }
    __syncthreads();
}

// image [H, W, C] and (when `weight` is not null) the clamp's derivative, a tile and a chunk of channels (blockIdx.z) per workgroup
__global__ void __launch_bounds__(kThreads) sh_forward_kernel(Plan p, const float *coeffs, float *image, uint8_t *weight) {
    __shared__ float rows[kTile * kMaxBasis], cols[kTile * kMaxTrig], cf[kChunk * kMaxBasis];
    const int nb = basis_count(p), nt = 2 * p.bands - 1, C = p.channels;
    const int ch0 = blockIdx.z * kChunk, cc = C - ch0 < kChunk ? C - ch0 : kChunk;
    const int r0 = blockIdx.y * kTile, c0 = blockIdx.x * kTile;
    const int nrows = p.height - r0 < kTile ? p.height - r0 : kTile, ncols = p.width - c0 < kTile ? p.width - c0 : kTile;
    for (int e = threadIdx.x; e < cc * nb; e += kThreads) {
        const int k = e / nb;
        cf[e] = coeffs[(size_t)(ch0 + k) * p.num_coeffs + (e - k * nb)];
    }
    tile_factors(p, r0, nrows, c0, ncols, rows, cols);
    const TileCoeffs tc{cf, nb};
    for (int e = threadIdx.x; e < nrows * ncols; e += kThreads) {
        const int y = e / ncols, x = e - y * ncols;
        float v[kChunk];
        uint8_t w[kChunk];
        pixel(p, rows + y * nb, cols + x * nt, tc, cc, v, w);
        const size_t at = ((size_t)(r0 + y) * p.width + (c0 + x)) * C + ch0;
        for (int k = 0; k < kChunk; ++k)
            if (k < cc) {
                image[at + k] = v[k];
                if (weight) weight[at + k] = w[k];
            }
    }
}

// partial[tile][ch][i] (fp64) = sum over the tile's pixels, row-major, of double(Y_i) * double(g * w): a lane per (i, channel of the chunk)
__global__ void __launch_bounds__(kThreads) sh_backward_tile_kernel(Plan p, const uint8_t *weight, const float *d_image, double *partial) {
    __shared__ float rows[kTile * kMaxBasis], cols[kTile * kMaxTrig], gw[kTile * kTile * kChunk];
    const int nb = basis_count(p), nt = 2 * p.bands - 1, C = p.channels;
    const int ch0 = blockIdx.z * kChunk, cc = C - ch0 < kChunk ? C - ch0 : kChunk;
    const int r0 = blockIdx.y * kTile, c0 = blockIdx.x * kTile;
    const int nrows = p.height - r0 < kTile ? p.height - r0 : kTile, ncols = p.width - c0 < kTile ? p.width - c0 : kTile;
    for (int e = threadIdx.x; e < nrows * ncols * cc; e += kThreads) {
        const int px = e / cc, k = e - px * cc, y = px / ncols, x = px - y * ncols;
        const size_t at = ((size_t)(r0 + y) * p.width + (c0 + x)) * C + ch0 + k;
        gw[e] = d_image[at] * clamp_weight(weight[at]);
    }
    tile_factors(p, r0, nrows, c0, ncols, rows, cols);          // (its barrier also covers gw)
    const int t = threadIdx.x;
    if (t >= nb * cc) return;
    const int i = t / cc, k = t - i * cc;
    int l = 0;
    while ((l + 1) * (l + 1) <= i) ++l;
    const int m = i - l * l - l;
    double sum = 0.0;
    for (int y = 0; y < nrows; ++y)
        for (int x = 0; x < ncols; ++x)
            sum += (double)basis(p, rows + y * nb, cols + x * nt, i, m) * (double)gw[(y * ncols + x) * cc + k];
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    partial[(tile * C + ch0 + k) * nb + i] = sum;
}

// d_coeffs[ch, i] = fp32(sum of the tiles' partials in ascending tile id); 0 for the columns the reconstruction does not read
__global__ void __launch_bounds__(kThreads) sh_backward_sum_kernel(Plan p, const double *partial, int tiles, float *d_coeffs) {
    const int e = blockIdx.x * kThreads + threadIdx.x, nb = basis_count(p);
    if (e >= p.channels * p.num_coeffs) return;
    const int ch = e / p.num_coeffs, i = e - ch * p.num_coeffs;
    double sum = 0.0;
    if (i < nb) {
#pragma unroll 8
        for (int t = 0; t < tiles; ++t) sum += partial[((size_t)t * p.channels + ch) * nb + i];
    }
    d_coeffs[e] = (float)sum;
}

// Rows [blockIdx.x * kScanRows, ...): the raw running sums of every row into cdf_xs, the row's weighted total into row_total,
// then the row's entries normalised in place (the workgroup reads back what it wrote itself, after a barrier).
__global__ void __launch_bounds__(kThreads) envmap_rows_kernel(const float *texels, const float *y_weight, int height, int width,
                                                               float *cdf_xs, float *row_total) {
    __shared__ float tile[kScanRows][kScanCols + 1];
    __shared__ float first[kScanRows], last[kScanRows];
    const int r0 = blockIdx.x * kScanRows, nrows = height - r0 < kScanRows ? height - r0 : kScanRows;
    const int t = threadIdx.x;
    double acc = 0.0;                                   // lanes 0 .. nrows - 1: the accumulator of row r0 + t
    for (int c0 = 0; c0 < width; c0 += kScanCols) {
        const int ncols = width - c0 < kScanCols ? width - c0 : kScanCols;
        for (int e = t; e < nrows * kScanCols; e += kThreads) {
            const int y = e / kScanCols, x = e - y * kScanCols;
            if (x < ncols) tile[y][x] = luminance(texels + ((size_t)(r0 + y) * width + (c0 + x)) * 3);
        }
        __syncthreads();
        if (t < nrows) {
            for (int x = 0; x < ncols; ++x) {
                acc += (double)tile[t][x];
                tile[t][x] = (float)acc;
            }
            if (c0 == 0) first[t] = tile[t][0];
        }
        __syncthreads();
        for (int e = t; e < nrows * kScanCols; e += kThreads) {
            const int y = e / kScanCols, x = e - y * kScanCols;
            if (x < ncols) cdf_xs[(size_t)(r0 + y) * width + (c0 + x)] = tile[y][x];
        }
        __syncthreads();
    }
    if (t < nrows) {
        last[t] = (float)acc;
        row_total[r0 + t] = (float)acc * y_weight[r0 + t];
    }
    __syncthreads();
    for (int y = 0; y < nrows; ++y)
        for (int x = t; x < width; x += kThreads) {
            const size_t at = (size_t)(r0 + y) * width + x;
            cdf_xs[at] = normalised(cdf_xs[at], first[y], last[y]);
        }
}

// cdf_ys holds the rows' weighted totals on entry: one lane's walk, then every lane normalises; total[0] = cy_[H - 1]
__global__ void __launch_bounds__(kThreads) envmap_column_kernel(int height, float *cdf_ys, float *total) {
    __shared__ float ends[2];
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int y = 0; y < height; ++y) {
            acc += (double)cdf_ys[y];
            cdf_ys[y] = (float)acc;
            if (y == 0) ends[0] = (float)acc;
        }
        ends[1] = (float)acc;
        total[0] = (float)acc;
    }
    __syncthreads();
    for (int y = threadIdx.x; y < height; y += kThreads) cdf_ys[y] = normalised(cdf_ys[y], ends[0], ends[1]);
}
#endif

// ---- host side -------------------------------------------------------------------------------------------------------------
inline double factorial(int n) { double f = 1.0; for (int k = 2; k <= n; ++k) f *= (double)k; return f; }

inline Plan make_plan(int height, int width, int channels, int num_coeffs, const char *who) {
    auto fail = [&](const std::string &what) { throw std::runtime_error(std::string(who) + ": " + what); };
    if (height <= 0 || width <= 0 || channels <= 0 || num_coeffs <= 0) fail("height, width, channels and the number of coefficients must be positive");
    if (height > 32768 || width > 32768 || (long long)height * width * channels > (long long)1 << 30)
        fail("a side of more than 32768 pixels or an image of more than 2^30 floats");
    if (channels > 65535 * kChunk) fail("too many channels");
    const int bands = (int)std::sqrt((double)num_coeffs);
    if (bands > kMaxBands)
        fail(std::to_string(num_coeffs) + " coefficients are " + std::to_string(bands) + " bands; at most " + std::to_string(kMaxBands) + " are supported");
    const double pi = 3.141592653589793;
    Plan p{};
    p.height = height; p.width = width; p.channels = channels; p.num_coeffs = num_coeffs; p.bands = bands;
    p.theta_step = (float)(pi / (double)height);
    p.phi_step = (float)(2.0 * pi / (double)width);
    for (int l = 0; l < bands; ++l)
        for (int m = -l; m <= l; ++m) {
            const int a = m < 0 ? -m : m;
            const double k = std::sqrt((2.0 * l + 1.0) * factorial(l - a) / (4.0 * pi * factorial(l + a)));
            p.k[l * l + l + m] = (float)(m == 0 ? k : std::sqrt(2.0) * k);
        }
    return p;
}

// floats of scratch rdr_sh_reconstruct_backward needs: the fp64 partial sums [tiles][C][L * L], two floats each
inline size_t scratch_floats(const Plan &p) { return 2 * (size_t)tiles_x(p) * tiles_y(p) * p.channels * basis_count(p); }

// rdr_sh_reconstruct: writes every element of image [H, W, C] and, when not null, of clamp [H, W, C]; stream-ordered, not synchronised
inline void reconstruct(int height, int width, int channels, int num_coeffs, const float *coeffs, float *image, uint8_t *clamp) {
    const Plan p = make_plan(height, width, channels, num_coeffs, "rdr_sh_reconstruct");
    if (!coeffs || !image) throw std::runtime_error("rdr_sh_reconstruct: coeffs and image are required");
#if !defined(RDR_HOSTSIM)
    const dim3 grid(tiles_x(p), tiles_y(p), (channels + kChunk - 1) / kChunk);
    hipLaunchKernelGGL(sh_forward_kernel, grid, dim3(kThreads), 0, exec::ctx().stream, p, coeffs, image, clamp);
    exec::check(hipGetLastError(), "sh_forward launch");
#else
    const int nb = basis_count(p), nt = 2 * p.bands - 1;
    std::vector<float> rows((size_t)height * nb), cols((size_t)width * nt);
    for (int r = 0; r < height; ++r) row_factors(p, r, rows.data() + (size_t)r * nb);
    for (int c = 0; c < width; ++c)
        for (int j = 0; j < nt; ++j) cols[(size_t)c * nt + j] = col_factor(p, c, j - (p.bands - 1));
    for (int r = 0; r < height; ++r)
        for (int c = 0; c < width; ++c)
            for (int ch0 = 0; ch0 < channels; ch0 += kChunk) {
                const int n = channels - ch0 < kChunk ? channels - ch0 : kChunk;
                float v[kChunk];
                uint8_t w[kChunk];
                pixel(p, rows.data() + (size_t)r * nb, cols.data() + (size_t)c * nt, GlobalCoeffs{coeffs, num_coeffs, ch0}, n, v, w);
                const size_t at = ((size_t)r * width + c) * channels + ch0;
                for (int k = 0; k < n; ++k) { image[at + k] = v[k]; if (clamp) clamp[at + k] = w[k]; }
            }
#endif
}

// rdr_sh_reconstruct_backward: writes every element of d_coeffs [C, N]; stream-ordered, not synchronised
inline void reconstruct_backward(int height, int width, int channels, int num_coeffs, const uint8_t *clamp, const float *d_image,
                                 float *d_coeffs, float *scratch, size_t scratch_count) {
    const Plan p = make_plan(height, width, channels, num_coeffs, "rdr_sh_reconstruct_backward");
    if (!clamp || !d_image || !d_coeffs) throw std::runtime_error("rdr_sh_reconstruct_backward: clamp, d_image and d_coeffs are required");
    need_scratch("rdr_sh_reconstruct_backward", scratch_floats(p), scratch, scratch_count, true);
    double *partial = reinterpret_cast<double *>(scratch);
    const int tiles = tiles_x(p) * tiles_y(p);
#if !defined(RDR_HOSTSIM)
    hipStream_t stream = exec::ctx().stream;
    const dim3 grid(tiles_x(p), tiles_y(p), (channels + kChunk - 1) / kChunk);
    hipLaunchKernelGGL(sh_backward_tile_kernel, grid, dim3(kThreads), 0, stream, p, clamp, d_image, partial);
    exec::check(hipGetLastError(), "sh_backward_tile launch");
    hipLaunchKernelGGL(sh_backward_sum_kernel, dim3((channels * num_coeffs + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, p,
                       (const double *)partial, tiles, d_coeffs);
    exec::check(hipGetLastError(), "sh_backward_sum launch");
#else
    const int nb = basis_count(p), nt = 2 * p.bands - 1;
    std::vector<float> rows((size_t)height * nb), cols((size_t)width * nt);
    for (int r = 0; r < height; ++r) row_factors(p, r, rows.data() + (size_t)r * nb);
    for (int c = 0; c < width; ++c)
        for (int j = 0; j < nt; ++j) cols[(size_t)c * nt + j] = col_factor(p, c, j - (p.bands - 1));
    for (int ty = 0; ty < tiles_y(p); ++ty)
        for (int tx = 0; tx < tiles_x(p); ++tx) {
            const int r1 = (ty + 1) * kTile < height ? (ty + 1) * kTile : height, c1 = (tx + 1) * kTile < width ? (tx + 1) * kTile : width;
            const size_t tile = (size_t)ty * tiles_x(p) + tx;
            for (int ch = 0; ch < channels; ++ch) {
                int i = 0;
                for (int l = 0; l < p.bands; ++l)
                    for (int m = -l; m <= l; ++m, ++i) {
                        double sum = 0.0;
                        for (int r = ty * kTile; r < r1; ++r)
                            for (int c = tx * kTile; c < c1; ++c) {
                                const size_t at = ((size_t)r * width + c) * channels + ch;
                                const float gw = d_image[at] * clamp_weight(clamp[at]);
                                sum += (double)basis(p, rows.data() + (size_t)r * nb, cols.data() + (size_t)c * nt, i, m) * (double)gw;
                            }
                        partial[(tile * channels + ch) * nb + i] = sum;
                    }
            }
        }
    for (int ch = 0; ch < channels; ++ch)
        for (int i = 0; i < num_coeffs; ++i) {
            double sum = 0.0;
            if (i < nb)
                for (int t = 0; t < tiles; ++t) sum += partial[((size_t)t * channels + ch) * nb + i];
            d_coeffs[(size_t)ch * num_coeffs + i] = (float)sum;
        }
#endif
}

// rdr_envmap_tables: writes every element of sample_cdf_ys [H] and sample_cdf_xs [H, W] and *total (HOST) = cy_[H - 1];
// synchronises once (the read-back)
inline void tables(int height, int width, const float *texels, const float *y_weight, float *cdf_ys, float *cdf_xs, float *total) {
    if (height <= 0 || width <= 0) throw std::runtime_error("rdr_envmap_tables: height and width must be positive");
    if (height > 32768 || width > 32768 || (long long)height * width * 3 > (long long)1 << 30)
        throw std::runtime_error("rdr_envmap_tables: a side of more than 32768 texels or an image of more than 2^30 floats");
    if (!texels || !y_weight || !cdf_ys || !cdf_xs || !total)
        throw std::runtime_error("rdr_envmap_tables: texels, y_weight, sample_cdf_ys, sample_cdf_xs and total are required");
#if !defined(RDR_HOSTSIM)
    hipStream_t stream = exec::ctx().stream;
    Arena arena;
    float *sum = arena.get<float>(1);
    hipLaunchKernelGGL(envmap_rows_kernel, dim3((height + kScanRows - 1) / kScanRows), dim3(kThreads), 0, stream, texels, y_weight,
                       height, width, cdf_xs, cdf_ys);
    exec::check(hipGetLastError(), "envmap_rows launch");
    hipLaunchKernelGGL(envmap_column_kernel, dim3(1), dim3(kThreads), 0, stream, height, cdf_ys, sum);
    exec::check(hipGetLastError(), "envmap_column launch");
    exec::download(total, sum, sizeof(float));          // both kernels have finished: `arena` may go back to the pool
#else
    std::vector<float> row(width);
    for (int y = 0; y < height; ++y) {
        double acc = 0.0;
        for (int x = 0; x < width; ++x) {
            acc += (double)luminance(texels + ((size_t)y * width + x) * 3);
            row[x] = (float)acc;
        }
        cdf_ys[y] = row[width - 1] * y_weight[y];
        for (int x = 0; x < width; ++x) cdf_xs[(size_t)y * width + x] = normalised(row[x], row[0], row[width - 1]);
    }
    double acc = 0.0;
    float first = 0.f;
    for (int y = 0; y < height; ++y) {
        acc += (double)cdf_ys[y];
        cdf_ys[y] = (float)acc;
        if (y == 0) first = (float)acc;
    }
    *total = (float)acc;
    for (int y = 0; y < height; ++y) cdf_ys[y] = normalised(cdf_ys[y], first, *total);
#endif
}

} // namespace shenv
} // namespace rdr
