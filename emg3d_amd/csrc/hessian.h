// Diagonal of the Gauss-Newton Hessian from the kept fields of reciprocal.h: the Jacobian row of
// datum (s, r) with respect to the conductivity component d of cell c is  s mu0 V_c / 4 Z_{s,r,d}(c),
//     Z_{s,r,d}(c) = sum over the four d-edges k of c (those of edges_to_cell, adjoint.h, in its order) of e_s[k] x_r[k],
// so with the components that the model does not distinguish added BEFORE the modulus (row[d]: d -> row of h)
//     h[p, c] += scale (V_c / 4)^2 sum_{s,r} w[s, r] | sum_{d: row[d] = p} Z_{s,r,d}(c) |^2 .
// One pass over the two stacks, arithmetic ~ ns nr per cell. A workgroup owns a patch of HD_PX x HD_PY x HD_PZ cells,
// one per thread. Per tile of HD_TS sources x HD_TR receivers and per direction it stages the edges of the patch
// (with the upper halo) of those fields in LDS -- 16-byte loads for complex fields, rows of HD_PX consecutive
// edges --, and every thread adds its four edges into HD_TS x HD_TR accumulators in registers; after the directions
// of a row the weighted squared moduli go into the row's accumulator, kept in a register over all tiles. Every edge
// value is fetched once per workgroup and partner tile and used 4 (cells) x HD_TR or HD_TS (partners) times from
// LDS. Plain fp64, no atomics; the order of every sum (edges: x, y, z and edges_to_cell's within; pairs: tile by
// tile, s outer) depends on the sizes alone. Fields of a ragged tile are not read (zeros in LDS, their pairs are
// skipped); the weights are uniform over the wave and arrive by scalar loads.
// Included at the end of kernels.hip (one translation unit), after reciprocal.h.
#pragma once

namespace {

constexpr int HD_PX = 16, HD_PY = 4, HD_PZ = 4;             // the patch; HD_PX complex values = 256 B per row
constexpr int HD_THREADS = HD_PX * HD_PY * HD_PZ;
constexpr int HD_TS = 4, HD_TR = 4;                          // the tile of (s, r): 16 accumulators per thread
constexpr int HD_EDGES = HD_PX * (HD_PY + 1) * (HD_PZ + 1); // x-edges of a patch, the most of the three directions
static_assert((HD_PX + 1) * HD_PY * (HD_PZ + 1) <= HD_EDGES && (HD_PX + 1) * (HD_PY + 1) * HD_PZ <= HD_EDGES, "LDS tile");
static_assert(HD_THREADS == 256 && HD_THREADS % HD_PX == 0, "one cell per thread, rows of HD_PX threads");

// S: the type the stacks are stored in (T, or its single-precision partner). The edges are staged in LDS AS STORED and
// widened when a thread reads them for its pair sums: the narrow instantiations ask for half the LDS; every operation
// is T's.
template <class S> constexpr size_t hessian_lds_bytes() { return (size_t)(HD_TS + HD_TR) * HD_EDGES * sizeof(S); }

template <class T, class S>
__global__ __launch_bounds__(HD_THREADS) void k_hessian_diagonal(int nx, int ny, int nz, const S *__restrict__ e, size_t es,
                                                                 int ns, const S *__restrict__ x, size_t xs, int nr,
                                                                 const double *__restrict__ wt, int row_x, int row_y,
                                                                 int row_z, double scale, const double *__restrict__ vol,
                                                                 double *__restrict__ h, size_t hs)
{
    extern __shared__ double2 hd_smem[];
    S *const lds = reinterpret_cast<S *>(hd_smem);          // [HD_TS + HD_TR][HD_EDGES]
    const int t = threadIdx.x;
    const int tx = t % HD_PX, trow = t / HD_PX;             // staging: thread tx of row trow
    const int ty = trow % HD_PY, tz = trow / HD_PY;         // the thread's cell in the patch
    const int x0 = blockIdx.x * HD_PX, y0 = blockIdx.y * HD_PY, z0 = blockIdx.z * HD_PZ;
    const size_t n_x = (size_t)nx * (ny + 1) * (nz + 1), n_y = (size_t)(nx + 1) * ny * (nz + 1);
    double h0 = 0.0, h1 = 0.0, h2 = 0.0;

    for (int s0 = 0; s0 < ns; s0 += HD_TS) {
        for (int r0 = 0; r0 < nr; r0 += HD_TR) {
#pragma unroll 1
            for (int p = 0; p < 3; ++p) {
                if (row_x != p && row_y != p && row_z != p) continue;
                T acc[HD_TS][HD_TR];
#pragma unroll
                for (int i = 0; i < HD_TS; ++i)
#pragma unroll
                    for (int j = 0; j < HD_TR; ++j) acc[i][j] = emg::zero<T>();
#pragma unroll 1
                for (int d = 0; d < 3; ++d) {
                    if ((d == 0 ? row_x : d == 1 ? row_y : row_z) != p) continue;
                    // the d-edges: (gnx, gny, gnz) of them on the grid, (lx, ly, lz) on the patch
                    const int gnx = nx + (d != 0), gny = ny + (d != 1), gnz = nz + (d != 2);
                    const int lx = HD_PX + (d != 0), ly = HD_PY + (d != 1), lz = HD_PZ + (d != 2);
                    const size_t goff = d == 0 ? 0 : d == 1 ? n_x : n_x + n_y;
                    __syncthreads();                        // the previous stage has been used up
                    for (int row = trow; row < ly * lz; row += HD_THREADS / HD_PX) {
                        const int gj = y0 + row % ly, gk = z0 + row / ly;
                        for (int li = tx; li < lx; li += HD_PX) {
                            const int gi = x0 + li;
                            const bool in = gi < gnx && gj < gny && gk < gnz;
                            const size_t g = goff + gi + (size_t)gnx * (gj + (size_t)gny * gk);
                            S *const dst = lds + (li + lx * row);
#pragma unroll
                            for (int i = 0; i < HD_TS; ++i)
                                dst[i * HD_EDGES] =
                                    in && s0 + i < ns ? e[(size_t)(s0 + i) * es + g] : emg::narrow<S>(emg::zero<T>());
#pragma unroll
                            for (int j = 0; j < HD_TR; ++j)
                                dst[(HD_TS + j) * HD_EDGES] =
                                    in && r0 + j < nr ? x[(size_t)(r0 + j) * xs + g] : emg::narrow<S>(emg::zero<T>());
                        }
                    }
                    __syncthreads();
                    // the four d-edges of the cell in the order of edges_to_cell: x: y inner, z outer; y: x, z; z: x, y
                    const int o1 = d == 0 ? lx : 1, o2 = d == 2 ? lx : lx * ly;
                    const S *const src = lds + (tx + lx * (ty + ly * tz));
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const S *const q = src + ((k & 1) * o1 + (k >> 1) * o2);
                        T ev[HD_TS], xv[HD_TR];
#pragma unroll
                        for (int i = 0; i < HD_TS; ++i) ev[i] = emg::widen(q[i * HD_EDGES]);
#pragma unroll
                        for (int j = 0; j < HD_TR; ++j) xv[j] = emg::widen(q[(HD_TS + j) * HD_EDGES]);
#pragma unroll
                        for (int i = 0; i < HD_TS; ++i)
#pragma unroll
                            for (int j = 0; j < HD_TR; ++j) acc[i][j] = emg::mad(ev[i], xv[j], acc[i][j]);
                    }
                }
                double sum = 0.0;
#pragma unroll
                for (int i = 0; i < HD_TS; ++i)
#pragma unroll
                    for (int j = 0; j < HD_TR; ++j)
                        if (s0 + i < ns && r0 + j < nr) {
                            const double w = wt[(size_t)(s0 + i) * nr + (r0 + j)];
                            if (w != 0.0) sum = __builtin_fma(w, emg::abs2(acc[i][j]), sum);
                        }
                if (p == 0) h0 += sum;
                else if (p == 1) h1 += sum;
                else h2 += sum;
            }
        }
    }
    const int ix = x0 + tx, iy = y0 + ty, iz = z0 + tz;
    if (ix >= nx || iy >= ny || iz >= nz) return;
    const size_t c = (size_t)ix + (size_t)nx * (iy + (size_t)ny * iz);
    const double q = vol[c] / 4;
    const double f = scale * (q * q);
    if (row_x == 0 || row_y == 0 || row_z == 0) h[c] += f * h0;
    if (row_x == 1 || row_y == 1 || row_z == 1) h[hs + c] += f * h1;
    if (row_x == 2 || row_y == 2 || row_z == 2) h[2 * hs + c] += f * h2;
}

template <class T, class S>
int launch_hessian_diagonal(int nx, int ny, int nz, const void *e, size_t es, int ns, const void *x, size_t xs, int nr,
                            const double *wt, int row_x, int row_y, int row_z, double scale, const double *vol, double *h,
                            size_t hs, hipStream_t st)
{
    constexpr size_t smem = hessian_lds_bytes<S>();
    if (smem > (size_t)64 * 1024) HIP_TRY(allow_lds((const void *)&k_hessian_diagonal<T, S>, smem));
    const dim3 grid(cdiv(nx, HD_PX), cdiv(ny, HD_PY), cdiv(nz, HD_PZ));
    hipLaunchKernelGGL((k_hessian_diagonal<T, S>), grid, dim3(HD_THREADS), smem, st, nx, ny, nz, (const S *)e, es, ns,
                       (const S *)x, xs, nr, wt, row_x, row_y, row_z, scale, vol, h, hs);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The checks of emg3d_dev_hessian_diagonal and of its _sp sibling (SP: stacks in single precision).
template <bool SP>
int hessian_diagonal(int nx, int ny, int nz, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                     size_t x_stride, int nr, const double *weights, int row_x, int row_y, int row_z, double scale,
                     const double *volumes, double *h, size_t h_stride, void *stream)
{
    if (nx < 1 || ny < 1 || nz < 1 || ns < 1 || nr < 1 || !e || !x || !weights || !volumes || !h)
        return fail(EMG3D_ERR_BADARG, "hessian_diagonal: bad argument");
    if (row_x < 0 || row_x > 2 || row_y < 0 || row_y > 2 || row_z < 0 || row_z > 2)
        return fail(EMG3D_ERR_BADARG, "hessian_diagonal: a row index is outside 0..2");
    const size_t n_edges = (size_t)nx * (ny + 1) * (nz + 1) + (size_t)(nx + 1) * ny * (nz + 1) +
                           (size_t)(nx + 1) * (ny + 1) * nz;
    if (e_stride < n_edges || x_stride < n_edges || h_stride < (size_t)nx * ny * nz)
        return fail(EMG3D_ERR_BADARG, "hessian_diagonal: a stride is smaller than its row");
    if (cdiv(ny, HD_PY) > 65535 || cdiv(nz, HD_PZ) > 65535)
        return fail(EMG3D_ERR_BADARG, "hessian_diagonal: too large for one launch");
    using C = std::conditional_t<SP, emg::cplxf, cplx>;
    using R = std::conditional_t<SP, float, double>;
    return is_complex ? launch_hessian_diagonal<cplx, C>(nx, ny, nz, e, e_stride, ns, x, x_stride, nr, weights, row_x, row_y,
                                                         row_z, scale, volumes, h, h_stride, (hipStream_t)stream)
                      : launch_hessian_diagonal<double, R>(nx, ny, nz, e, e_stride, ns, x, x_stride, nr, weights, row_x, row_y,
                                                           row_z, scale, volumes, h, h_stride, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int emg3d_dev_hessian_diagonal(int nx, int ny, int nz, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                               size_t x_stride, int nr, const double *weights, int row_x, int row_y, int row_z, double scale,
                               const double *volumes, double *h, size_t h_stride, void *stream)
{
    return hessian_diagonal<false>(nx, ny, nz, is_complex, e, e_stride, ns, x, x_stride, nr, weights, row_x, row_y, row_z, scale,
                                   volumes, h, h_stride, stream);
}

int emg3d_dev_hessian_diagonal_sp(int nx, int ny, int nz, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                                  size_t x_stride, int nr, const double *weights, int row_x, int row_y, int row_z, double scale,
                                  const double *volumes, double *h, size_t h_stride, void *stream)
{
    return hessian_diagonal<true>(nx, ny, nz, is_complex, e, e_stride, ns, x, x_stride, nr, weights, row_x, row_y, row_z, scale,
                                  volumes, h, h_stride, stream);
}

}  // extern "C"
