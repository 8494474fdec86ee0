// Block-Jacobi for the block PCG of regularise.h: k_pcg_update and k_pcg_direction with the
// preconditioner z_c = (B_c + lambda diag(rd_c))^-1 r_c per cell c, B_c the n x n block of the Gauss-Newton Hessian that
// couples the n = vec_per_col components of the cell (hessian_blocks.h; packed rows, hblocks_stride apart: the diagonal
// (0,0) .. (n-1,n-1) first, then (0,1) and, for n = 3, (0,2), (1,2)) and rd_c the diagonal of R (rdiag_stride 0: one
// row for all components; otherwise one row per component).
// A thread takes a cell and ALL its components (cells grid-stride, components inner): it forms the symmetric A,
// factorises it by Cholesky in registers in a fixed order (column by column, A = L L^T) and solves by the two
// substitutions -- if every pivot is finite and > 0. Otherwise the cell falls back to pcg_precondition component by
// component: Jacobi on the diagonal rows, the identity where that sum is not positive. Inactive cells: r = z = 0.
// alpha, beta, the frozen columns, the table, the two partial sums per workgroup in the ws layout that k_pcg_scalar
// reads, and z formed again in the direction kernel are those of k_pcg_update / k_pcg_direction. Plain fp64, no
// atomics, every order fixed by the sizes.
// Included at the end of kernels.hip (one translation unit), after regularise.h.
#pragma once

namespace {

__device__ __forceinline__ bool pcg_pivot_ok(double d) { return d > 0.0 && d <= 1.7976931348623157e308; }

// z = M r for the N components of cell c of a column with damping lam
template <int N>
__device__ __forceinline__ void pcg_block_precondition(const double (&r)[N], bool act, const double *__restrict__ hb,
                                                       size_t hbs, const double *__restrict__ rdiag, size_t rds, size_t c,
                                                       double lam, double (&z)[N])
{
    if (!act) {
#pragma unroll
        for (int k = 0; k < N; ++k) z[k] = 0.0;
        return;
    }
    double hd[N], rd[N], L[N][N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        hd[k] = hb[(size_t)k * hbs + c];
        rd[k] = rdiag[(size_t)k * rds + c];
        L[k][k] = hd[k] + lam * rd[k];
    }
    {
        int m = N;                                          // the packed rows behind the diagonal: (0,1), (0,2), (1,2)
#pragma unroll
        for (int q = 1; q < N; ++q)
#pragma unroll
            for (int p = 0; p < q; ++p, ++m) L[q][p] = hb[(size_t)m * hbs + c];
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {                           // column j of L
        double d = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        ok = ok && pcg_pivot_ok(d);
        const double l = sqrt(d);
        L[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double s = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            L[i][j] = s / l;
        }
    }
    if (ok) {
        double y[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {                       // L y = r
            double s = r[i];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
            y[i] = s / L[i][i];
        }
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {                  // L^T z = y
            double s = y[i];
#pragma unroll
            for (int k = i + 1; k < N; ++k) s -= L[k][i] * z[k];
            z[i] = s / L[i][i];
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) z[k] = pcg_precondition(r[k], true, true, hd[k], rd[k], lam);
    }
}

template <int N>
__global__ __launch_bounds__(PCG_BLOCK) void k_pcg_update_blk(size_t ncell, int first, double *x, double *r,
                                                              const double *__restrict__ p, const double *__restrict__ q,
                                                              const double *__restrict__ hb, size_t hbs,
                                                              const double *__restrict__ rdiag, size_t rds,
                                                              const unsigned char *__restrict__ mask, const double *table,
                                                              const double *pq, double *ws)
{
    const int col = blockIdx.y;
    const double *row = table + (size_t)col * PCG_ROW;
    const double lam = row[PCG_LAM];
    const bool run = row[PCG_STATE] == 0.0 && (first || pcg_pq_ok(pq[col]));
    const double alpha = (run && !first) ? row[PCG_RZ] / pq[col] : 0.0;
    double arz = 0.0, arr = 0.0;
    if (run) {
        const size_t base = (size_t)col * N * ncell;
        for (size_t c = (size_t)blockIdx.x * PCG_BLOCK + threadIdx.x; c < ncell; c += (size_t)gridDim.x * PCG_BLOCK) {
            const bool act = !mask || mask[c];
            double rn[N], z[N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const size_t i = base + (size_t)k * ncell + c;
                rn[k] = r[i];
                if (!first) {
                    x[i] += alpha * p[i];
                    rn[k] -= alpha * q[i];
                }
                rn[k] = act ? rn[k] : 0.0;
                r[i] = rn[k];
            }
            pcg_block_precondition<N>(rn, act, hb, hbs, rdiag, rds, c, lam, z);
#pragma unroll
            for (int k = 0; k < N; ++k) {
                arz += rn[k] * z[k];
                arr += rn[k] * rn[k];
            }
        }
    }
    __shared__ double sm[PCG_BLOCK / 64][2];
    arz = wave_sum(arz);
    arr = wave_sum(arr);
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = arz; sm[threadIdx.x >> 6][1] = arr; }
    __syncthreads();
    if (threadIdx.x < 2)
        ws[((size_t)col * gridDim.x + blockIdx.x) * 2 + threadIdx.x] =
            (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
}

template <int N>
__global__ __launch_bounds__(PCG_BLOCK) void k_pcg_direction_blk(size_t ncell, int first, double *p,
                                                                 const double *__restrict__ r, const double *__restrict__ hb,
                                                                 size_t hbs, const double *__restrict__ rdiag, size_t rds,
                                                                 const unsigned char *__restrict__ mask, const double *table)
{
    const int col = blockIdx.y;
    const double *row = table + (size_t)col * PCG_ROW;
    if (row[PCG_STATE] != 0.0) return;
    const double lam = row[PCG_LAM];
    const double beta = first ? 0.0 : row[PCG_RZ] / row[PCG_RZ_OLD];
    const size_t base = (size_t)col * N * ncell;
    for (size_t c = (size_t)blockIdx.x * PCG_BLOCK + threadIdx.x; c < ncell; c += (size_t)gridDim.x * PCG_BLOCK) {
        const bool act = !mask || mask[c];
        double rn[N], z[N];
#pragma unroll
        for (int k = 0; k < N; ++k) rn[k] = r[base + (size_t)k * ncell + c];
        pcg_block_precondition<N>(rn, act, hb, hbs, rdiag, rds, c, lam, z);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const size_t i = base + (size_t)k * ncell + c;
            p[i] = first ? z[k] : z[k] + beta * p[i];
        }
    }
}

inline bool pcg_blk_args_ok(size_t n_cells, int vec_per_col, int ncol, const double *hblocks, size_t hblocks_stride,
                            const double *rdiag, size_t rdiag_stride)
{
    return n_cells >= 1 && (vec_per_col == 2 || vec_per_col == 3) && ncol >= 1 && ncol <= 65535 && hblocks && rdiag &&
           hblocks_stride >= n_cells && (rdiag_stride == 0 || rdiag_stride >= n_cells);
}

}  // namespace

extern "C" {

int emg3d_dev_pcg_update_blk(size_t n_cells, int vec_per_col, int ncol, int first, double *x, double *r, const double *p,
                             const double *q, const double *hblocks, size_t hblocks_stride, const double *rdiag,
                             size_t rdiag_stride, const unsigned char *mask, const double *table, const double *pq, double *ws,
                             size_t ws_len, void *stream)
{
    if (!pcg_blk_args_ok(n_cells, vec_per_col, ncol, hblocks, hblocks_stride, rdiag, rdiag_stride) || !r || !table || !ws ||
        (!first && (!x || !p || !q || !pq)))
        return fail(EMG3D_ERR_BADARG, "pcg_update_blk: bad argument");
    if (ws_len < emg3d_pcg_ws_len(n_cells, ncol))
        return fail(EMG3D_ERR_SCRATCH, "pcg_update_blk: workspace too small (emg3d_pcg_ws_len)");
    const dim3 grid(pcg_blocks(n_cells), ncol);
    if (vec_per_col == 2)
        hipLaunchKernelGGL(k_pcg_update_blk<2>, grid, dim3(PCG_BLOCK), 0, (hipStream_t)stream, n_cells, first ? 1 : 0, x, r, p, q,
                           hblocks, hblocks_stride, rdiag, rdiag_stride, mask, table, pq, ws);
    else
        hipLaunchKernelGGL(k_pcg_update_blk<3>, grid, dim3(PCG_BLOCK), 0, (hipStream_t)stream, n_cells, first ? 1 : 0, x, r, p, q,
                           hblocks, hblocks_stride, rdiag, rdiag_stride, mask, table, pq, ws);
    HIP_TRY(hipGetLastError());
    return 0;
}

int emg3d_dev_pcg_direction_blk(size_t n_cells, int vec_per_col, int ncol, int first, double *p, const double *r,
                                const double *hblocks, size_t hblocks_stride, const double *rdiag, size_t rdiag_stride,
                                const unsigned char *mask, const double *table, void *stream)
{
    if (!pcg_blk_args_ok(n_cells, vec_per_col, ncol, hblocks, hblocks_stride, rdiag, rdiag_stride) || !p || !r || !table)
        return fail(EMG3D_ERR_BADARG, "pcg_direction_blk: bad argument");
    const dim3 grid(pcg_blocks(n_cells), ncol);
    if (vec_per_col == 2)
        hipLaunchKernelGGL(k_pcg_direction_blk<2>, grid, dim3(PCG_BLOCK), 0, (hipStream_t)stream, n_cells, first ? 1 : 0, p, r,
                           hblocks, hblocks_stride, rdiag, rdiag_stride, mask, table);
    else
        hipLaunchKernelGGL(k_pcg_direction_blk<3>, grid, dim3(PCG_BLOCK), 0, (hipStream_t)stream, n_cells, first ? 1 : 0, p, r,
                           hblocks, hblocks_stride, rdiag, rdiag_stride, mask, table);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
