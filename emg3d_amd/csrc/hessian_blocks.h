// The n x n blocks of the Gauss-Newton Hessian that couple the conductivity components of ONE cell,
// from the kept fields and in the notation of hessian.h: with Z_p = sum_{d: row[d] = p} Z_{s,r,d}(c),
//     h[(p,q), c] += scale (V_c / 4)^2 sum_{s,r} w[s, r] Re( conj(Z_p) Z_q ),   p <= q < n,   n = max(row) + 1
// (real fields: Z_p Z_q). Packed rows of h: the diagonal (0,0) .. (n-1,n-1) first -- the rows that
// k_hessian_diagonal adds --, then (0,1) and, for n = 3, (0,2), (1,2).
// The patch, the staging and the orders are those of k_hessian_diagonal; the difference: a direction is staged ONCE
// per tile and added into the pair sums of its row, so all NROWS sets of pair sums are live at the end of a tile,
// where the n (n + 1) / 2 weighted products go to per-tile sums and from there to the thread's row accumulators, kept
// over all tiles. The pair sums are the register budget: 4 x 4 complex sums x 2 rows are 128 VGPRs, which fit beside
// the operands; three rows take a tile of 4 sources x 2 receivers (96 VGPRs). Per row the operations and
// their order are those of k_hessian_diagonal for the same tile: directions x, y, z, the edges in edges_to_cell's
// order, pairs s outer, the tile's sum added to the row's accumulator.
// Plain fp64, no atomics; every order depends on the sizes alone. Fields of a ragged tile are not read; pairs with
// weight 0 are skipped.
// Included at the end of kernels.hip (one translation unit), after hessian.h.
#pragma once

namespace {

template <int NROWS> struct HbTile {
    static constexpr int TS = HD_TS, TR = NROWS == 3 ? 2 : HD_TR;
    static constexpr int NPACK = NROWS * (NROWS + 1) / 2;
};
template <class S, int NROWS> constexpr size_t hessian_blocks_lds_bytes()
{
    return (size_t)(HbTile<NROWS>::TS + HbTile<NROWS>::TR) * HD_EDGES * sizeof(S);
}

EMG_HD double hb_re_conj_product(emg::cplx a, emg::cplx b) { return __builtin_fma(a.re, b.re, a.im * b.im); }
EMG_HD double hb_re_conj_product(double a, double b) { return a * b; }

// the four d-edges of the thread's cell (from `src`, strides o1 and o2) into the TS x TR pair sums of one row
template <class T, class S, int TS, int TR>
__device__ __forceinline__ void hb_add_direction(const S *src, int o1, int o2, T (&acc)[TS][TR])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const S *const q = src + ((k & 1) * o1 + (k >> 1) * o2);
        T ev[TS], xv[TR];
#pragma unroll
        for (int i = 0; i < TS; ++i) ev[i] = emg::widen(q[i * HD_EDGES]);
#pragma unroll
        for (int j = 0; j < TR; ++j) xv[j] = emg::widen(q[(TS + j) * HD_EDGES]);
#pragma unroll
        for (int i = 0; i < TS; ++i)
#pragma unroll
            for (int j = 0; j < TR; ++j) acc[i][j] = emg::mad(ev[i], xv[j], acc[i][j]);
    }
}

template <class T, class S, int NROWS>
__global__ __launch_bounds__(HD_THREADS) void k_hessian_cell_blocks(int nx, int ny, int nz, const S *__restrict__ e,
                                                                    size_t es, int ns, const S *__restrict__ x, size_t xs,
                                                                    int nr, const double *__restrict__ wt, int row_x,
                                                                    int row_y, int row_z, double scale,
                                                                    const double *__restrict__ vol, double *__restrict__ h,
                                                                    size_t hs)
{
    constexpr int TS = HbTile<NROWS>::TS, TR = HbTile<NROWS>::TR, NPACK = HbTile<NROWS>::NPACK;
    extern __shared__ double2 hd_smem[];
    S *const lds = reinterpret_cast<S *>(hd_smem);          // [TS + TR][HD_EDGES]
    const int t = threadIdx.x;
    const int tx = t % HD_PX, trow = t / HD_PX;             // staging: thread tx of row trow
    const int ty = trow % HD_PY, tz = trow / HD_PY;         // the thread's cell in the patch
    const int x0 = blockIdx.x * HD_PX, y0 = blockIdx.y * HD_PY, z0 = blockIdx.z * HD_PZ;
    const size_t n_x = (size_t)nx * (ny + 1) * (nz + 1), n_y = (size_t)(nx + 1) * ny * (nz + 1);
    double hacc[NPACK];
#pragma unroll
    for (int m = 0; m < NPACK; ++m) hacc[m] = 0.0;

    for (int s0 = 0; s0 < ns; s0 += TS) {
        for (int r0 = 0; r0 < nr; r0 += TR) {
            T acc[NROWS][TS][TR];
#pragma unroll
            for (int p = 0; p < NROWS; ++p)
#pragma unroll
                for (int i = 0; i < TS; ++i)
#pragma unroll
                    for (int j = 0; j < TR; ++j) acc[p][i][j] = emg::zero<T>();
#pragma unroll 1
            for (int d = 0; d < 3; ++d) {
                const int rd = d == 0 ? row_x : d == 1 ? row_y : row_z;
                // the d-edges: (gnx, gny, gnz) of them on the grid, (lx, ly, lz) on the patch
                const int gnx = nx + (d != 0), gny = ny + (d != 1), gnz = nz + (d != 2);
                const int lx = HD_PX + (d != 0), ly = HD_PY + (d != 1), lz = HD_PZ + (d != 2);
                const size_t goff = d == 0 ? 0 : d == 1 ? n_x : n_x + n_y;
                __syncthreads();                            // the previous stage has been used up
                for (int row = trow; row < ly * lz; row += HD_THREADS / HD_PX) {
                    const int gj = y0 + row % ly, gk = z0 + row / ly;
                    for (int li = tx; li < lx; li += HD_PX) {
                        const int gi = x0 + li;
                        const bool in = gi < gnx && gj < gny && gk < gnz;
                        const size_t g = goff + gi + (size_t)gnx * (gj + (size_t)gny * gk);
                        S *const dst = lds + (li + lx * row);
#pragma unroll
                        for (int i = 0; i < TS; ++i)
                            dst[i * HD_EDGES] =
                                in && s0 + i < ns ? e[(size_t)(s0 + i) * es + g] : emg::narrow<S>(emg::zero<T>());
#pragma unroll
                        for (int j = 0; j < TR; ++j)
                            dst[(TS + j) * HD_EDGES] =
                                in && r0 + j < nr ? x[(size_t)(r0 + j) * xs + g] : emg::narrow<S>(emg::zero<T>());
                    }
                }
                __syncthreads();
                // the four d-edges of the cell in the order of edges_to_cell: x: y inner, z outer; y: x, z; z: x, y
                const int o1 = d == 0 ? lx : 1, o2 = d == 2 ? lx : lx * ly;
                const S *const src = lds + (tx + lx * (ty + ly * tz));
#pragma unroll
                for (int p = 0; p < NROWS; ++p)             // rd is uniform: one of the NROWS copies runs
                    if (rd == p) hb_add_direction<T, S, TS, TR>(src, o1, o2, acc[p]);
            }
            double sum[NPACK];
#pragma unroll
            for (int m = 0; m < NPACK; ++m) sum[m] = 0.0;
#pragma unroll
            for (int i = 0; i < TS; ++i)
#pragma unroll
                for (int j = 0; j < TR; ++j)
                    if (s0 + i < ns && r0 + j < nr) {
                        const double w = wt[(size_t)(s0 + i) * nr + (r0 + j)];
                        if (w != 0.0) {
#pragma unroll
                            for (int p = 0; p < NROWS; ++p) sum[p] = __builtin_fma(w, emg::abs2(acc[p][i][j]), sum[p]);
                            int m = NROWS;
#pragma unroll
                            for (int q = 1; q < NROWS; ++q)
#pragma unroll
                                for (int p = 0; p < q; ++p, ++m)
                                    sum[m] = __builtin_fma(w, hb_re_conj_product(acc[p][i][j], acc[q][i][j]), sum[m]);
                        }
                    }
#pragma unroll
            for (int m = 0; m < NPACK; ++m) hacc[m] += sum[m];
        }
    }
    const int ix = x0 + tx, iy = y0 + ty, iz = z0 + tz;
    if (ix >= nx || iy >= ny || iz >= nz) return;
    const size_t c = (size_t)ix + (size_t)nx * (iy + (size_t)ny * iz);
    const double q = vol[c] / 4;
    const double f = scale * (q * q);
#pragma unroll
    for (int m = 0; m < NPACK; ++m) h[(size_t)m * hs + c] += f * hacc[m];
}

template <class T, class S, int NROWS>
int launch_hessian_cell_blocks(int nx, int ny, int nz, const void *e, size_t es, int ns, const void *x, size_t xs, int nr,
                               const double *wt, int row_x, int row_y, int row_z, double scale, const double *vol, double *h,
                               size_t hs, hipStream_t st)
{
    constexpr size_t smem = hessian_blocks_lds_bytes<S, NROWS>();
    if (smem > (size_t)64 * 1024) HIP_TRY(allow_lds((const void *)&k_hessian_cell_blocks<T, S, NROWS>, smem));
    const dim3 grid(cdiv(nx, HD_PX), cdiv(ny, HD_PY), cdiv(nz, HD_PZ));
    hipLaunchKernelGGL((k_hessian_cell_blocks<T, S, NROWS>), grid, dim3(HD_THREADS), smem, st, nx, ny, nz, (const S *)e, es, ns,
                       (const S *)x, xs, nr, wt, row_x, row_y, row_z, scale, vol, h, hs);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The checks of emg3d_dev_hessian_cell_blocks and of its _sp sibling (SP: stacks in single precision): those of
// hessian_diagonal, and every row below n must have a direction.
template <bool SP>
int hessian_cell_blocks(int nx, int ny, int nz, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                        size_t x_stride, int nr, const double *weights, int row_x, int row_y, int row_z, double scale,
                        const double *volumes, double *h, size_t h_stride, void *stream)
{
    if (nx < 1 || ny < 1 || nz < 1 || ns < 1 || nr < 1 || !e || !x || !weights || !volumes || !h)
        return fail(EMG3D_ERR_BADARG, "hessian_cell_blocks: bad argument");
    if (row_x < 0 || row_x > 2 || row_y < 0 || row_y > 2 || row_z < 0 || row_z > 2)
        return fail(EMG3D_ERR_BADARG, "hessian_cell_blocks: a row index is outside 0..2");
    const int n = std::max(row_x, std::max(row_y, row_z)) + 1;
    for (int p = 0; p < n; ++p)
        if (row_x != p && row_y != p && row_z != p)
            return fail(EMG3D_ERR_BADARG, "hessian_cell_blocks: a row below the largest has no direction");
    const size_t n_edges = (size_t)nx * (ny + 1) * (nz + 1) + (size_t)(nx + 1) * ny * (nz + 1) +
                           (size_t)(nx + 1) * (ny + 1) * nz;
    if (e_stride < n_edges || x_stride < n_edges || h_stride < (size_t)nx * ny * nz)
        return fail(EMG3D_ERR_BADARG, "hessian_cell_blocks: a stride is smaller than its row");
    if (cdiv(ny, HD_PY) > 65535 || cdiv(nz, HD_PZ) > 65535)
        return fail(EMG3D_ERR_BADARG, "hessian_cell_blocks: too large for one launch");
    using C = std::conditional_t<SP, emg::cplxf, cplx>;
    using R = std::conditional_t<SP, float, double>;
    const hipStream_t st = (hipStream_t)stream;
#define EMG_HB_LAUNCH(N)                                                                                                       \
    (is_complex ? launch_hessian_cell_blocks<cplx, C, N>(nx, ny, nz, e, e_stride, ns, x, x_stride, nr, weights, row_x, row_y,    \
                                                         row_z, scale, volumes, h, h_stride, st)                                 \
                : launch_hessian_cell_blocks<double, R, N>(nx, ny, nz, e, e_stride, ns, x, x_stride, nr, weights, row_x, row_y,  \
                                                           row_z, scale, volumes, h, h_stride, st))
    const int err = n == 1 ? EMG_HB_LAUNCH(1) : n == 2 ? EMG_HB_LAUNCH(2) : EMG_HB_LAUNCH(3);
#undef EMG_HB_LAUNCH
    return err;
}

}  // namespace

extern "C" {

int emg3d_dev_hessian_cell_blocks(int nx, int ny, int nz, int is_complex, const void *e, size_t e_stride, int ns,
                                  const void *x, size_t x_stride, int nr, const double *weights, int row_x, int row_y,
                                  int row_z, double scale, const double *volumes, double *h, size_t h_stride, void *stream)
{
    return hessian_cell_blocks<false>(nx, ny, nz, is_complex, e, e_stride, ns, x, x_stride, nr, weights, row_x, row_y, row_z,
                                      scale, volumes, h, h_stride, stream);
}

int emg3d_dev_hessian_cell_blocks_sp(int nx, int ny, int nz, int is_complex, const void *e, size_t e_stride, int ns,
                                     const void *x, size_t x_stride, int nr, const double *weights, int row_x, int row_y,
                                     int row_z, double scale, const double *volumes, double *h, size_t h_stride,
                                     void *stream)
{
    return hessian_cell_blocks<true>(nx, ny, nz, is_complex, e, e_stride, ns, x, x_stride, nr, weights, row_x, row_y, row_z,
                                     scale, volumes, h, h_stride, stream);
}

}  // extern "C"
