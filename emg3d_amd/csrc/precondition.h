// The data-space (Woodbury) preconditioner of the block PCG of regularise.h. H = J^T W J has rank
// at most M (the real data), so with D_k = lambda_k diag R, B = diag(s) (J^ diag(dinv) J^T) diag(s) = Q L Q^T, s = sqrt(W)
// and dinv = 1 / diag R (1 where that is not positive, 0 on inactive cells)
//
//     z = (D_k + J^T diag(s) Q_rho Q_rho^T diag(s) J^)^-1 r = u - dinv o J^T y / lambda_k,      u = dinv o r / lambda_k,
//     y = diag(s) Q_rho diag(phi_k) Q_rho^T diag(s) J^ u,      phi_k,j = lambda_k / (lambda_k + L_j)
//
// -- exactly, for every rank rho <= M kept, and with all of them the inverse of D_k + H itself. J^ u and J^T y are the
// two halves of a block pass over the kept fields (block.h); here are the four kernels around them. Everything is
// plain fp64, there are no floating-point atomics and every sum runs in an order fixed by the sizes alone: the same
// call gives the same bits. Columns, the table and its states: as in regularise.h; a column whose state is not 0, or
// whose <p,q> k_pcg_update has refused, is skipped by the three vector kernels: u, z and p keep their bits.
//
//   k_pcg_scale         grid (blocks, K): u = dinv o r / lambda_k. dinv_stride: doubles between the rows of dinv of two
//                       components (0: one row for all), as rdiag_stride.
//   k_data_filter_down  t[k, j] = phi_k,j sum_i Q[i, j] s[i] d[k, i]: workgroup (64, 4) for 64 columns j of Q (row-major
//                       M x rho: a wave reads 512 B of one row), wave w adds the rows of its quarter of 0 .. M - 1 in
//                       ascending order, the four partial sums meet in LDS and are added as (0 + 1) + (2 + 3).
//   k_data_filter_up    y[k, i] = s[i] sum_j Q[i, j] t[k, j]: one wave per row i, lane l adds j = l, l + 64, ... in
//                       ascending order, then the shuffle tree of wave_sum. A frozen column: phi = 0 and y = 0, written.
//                       Both stages keep FILTER_COLS = 8 columns in registers, so Q is read once per stage for every
//                       eight columns.
//   k_pcg_finish        grid (blocks, K): z = u - dinv o g / lambda_k (0 on inactive cells) and the workgroup's share of
//                       <r, z> and <r, r> in the layout of k_pcg_update, ws[(k * blocks + block) * 2 + {0, 1}]:
//                       k_pcg_scalar and the table are those of the Jacobi route.
//   k_pcg_direction_z   p = z + beta p from the stored z, beta = <r,z> / <r,z>_old (first: p = z).
// Included at the end of kernels.hip (one translation unit), after regularise.h.
#pragma once

namespace {

constexpr int FILTER_COLS = 8;

__device__ __forceinline__ bool pcg_column_runs(const double *row, int first, const double *pq, int col)
{
    return row[PCG_STATE] == 0.0 && (first || pcg_pq_ok(pq[col]));
}

__global__ __launch_bounds__(PCG_BLOCK) void k_pcg_scale(size_t ncell, int vpc, int first, double *__restrict__ u,
                                                         const double *__restrict__ r, const double *__restrict__ dinv,
                                                         size_t dinv_stride, const double *table, const double *pq)
{
    const int col = blockIdx.y;
    const double *row = table + (size_t)col * PCG_ROW;
    if (!pcg_column_runs(row, first, pq, col)) return;
    const double lam = row[PCG_LAM];
    for (int k = 0; k < vpc; ++k) {
        const size_t dcomp = (size_t)k * dinv_stride, base = ((size_t)col * vpc + k) * ncell;
        for (size_t c = (size_t)blockIdx.x * PCG_BLOCK + threadIdx.x; c < ncell; c += (size_t)gridDim.x * PCG_BLOCK)
            u[base + c] = dinv[dcomp + c] * r[base + c] / lam;
    }
}

__global__ __launch_bounds__(PCG_BLOCK) void k_pcg_finish(size_t ncell, int vpc, int first, double *__restrict__ z,
                                                          const double *__restrict__ u, const double *__restrict__ g,
                                                          const double *__restrict__ r, const double *__restrict__ dinv,
                                                          size_t dinv_stride, const unsigned char *__restrict__ mask,
                                                          const double *table, const double *pq, double *ws)
{
    const int col = blockIdx.y;
    const double *row = table + (size_t)col * PCG_ROW;
    const double lam = row[PCG_LAM];
    double arz = 0.0, arr = 0.0;
    if (pcg_column_runs(row, first, pq, col)) {
        for (int k = 0; k < vpc; ++k) {
            const size_t dcomp = (size_t)k * dinv_stride, base = ((size_t)col * vpc + k) * ncell;
            for (size_t c = (size_t)blockIdx.x * PCG_BLOCK + threadIdx.x; c < ncell; c += (size_t)gridDim.x * PCG_BLOCK) {
                const bool act = !mask || mask[c];
                const double rn = r[base + c];
                const double zn = act ? u[base + c] - dinv[dcomp + c] * g[base + c] / lam : 0.0;
                z[base + c] = zn;
                arz += rn * zn;
                arr += rn * rn;
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

__global__ __launch_bounds__(PCG_BLOCK) void k_pcg_direction_z(size_t ncell, int vpc, int first, double *__restrict__ p,
                                                               const double *__restrict__ z, const double *table)
{
    const int col = blockIdx.y;
    const double *row = table + (size_t)col * PCG_ROW;
    if (row[PCG_STATE] != 0.0) return;
    const double beta = first ? 0.0 : row[PCG_RZ] / row[PCG_RZ_OLD];
    const size_t n = (size_t)vpc * ncell, base = (size_t)col * n;
    for (size_t c = (size_t)blockIdx.x * PCG_BLOCK + threadIdx.x; c < n; c += (size_t)gridDim.x * PCG_BLOCK)
        p[base + c] = first ? z[base + c] : z[base + c] + beta * p[base + c];
}

// t[(k0 + k) * rho + j], k < kn <= FILTER_COLS: workgroup (64, 4), j = 64 blockIdx.x + threadIdx.x
__global__ __launch_bounds__(256) void k_data_filter_down(int m, int rho, int k0, int kn, const double *__restrict__ Q,
                                                          const double *__restrict__ eig, const double *__restrict__ s,
                                                          const double *__restrict__ d, const double *table,
                                                          double *__restrict__ t)
{
    const int j = blockIdx.x * 64 + threadIdx.x, w = threadIdx.y;
    const int per = (m + 3) / 4, i0 = w * per, i1 = min(m, i0 + per);
    double acc[FILTER_COLS];
#pragma unroll
    for (int k = 0; k < FILTER_COLS; ++k) acc[k] = 0.0;
    if (j < rho) {
        for (int i = i0; i < i1; ++i) {
            const double qij = Q[(size_t)i * rho + j], si = s[i];
#pragma unroll
            for (int k = 0; k < FILTER_COLS; ++k)
                if (k < kn) acc[k] += qij * (si * d[(size_t)(k0 + k) * m + i]);
        }
    }
    __shared__ double sm[4][FILTER_COLS][64];
#pragma unroll
    for (int k = 0; k < FILTER_COLS; ++k) sm[w][k][threadIdx.x] = acc[k];
    __syncthreads();
    if (w != 0 || j >= rho) return;
    const double lj = eig[j];
    for (int k = 0; k < kn; ++k) {
        const double *row = table + (size_t)(k0 + k) * PCG_ROW;
        const double lam = row[PCG_LAM];
        const double phi = row[PCG_STATE] == 0.0 ? lam / (lam + lj) : 0.0;
        const double sum = (sm[0][k][threadIdx.x] + sm[1][k][threadIdx.x]) + (sm[2][k][threadIdx.x] + sm[3][k][threadIdx.x]);
        t[(size_t)(k0 + k) * rho + j] = phi * sum;
    }
}

// y[(k0 + k) * m + i], k < kn <= FILTER_COLS: one wave per row i = 4 blockIdx.x + wave
__global__ __launch_bounds__(256) void k_data_filter_up(int m, int rho, int k0, int kn, const double *__restrict__ Q,
                                                        const double *__restrict__ s, const double *__restrict__ t,
                                                        const double *table, double *__restrict__ y)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;                                  // (a whole wave: no shuffle partner is lost)
    double acc[FILTER_COLS];
#pragma unroll
    for (int k = 0; k < FILTER_COLS; ++k) acc[k] = 0.0;
    for (int j = lane; j < rho; j += 64) {
        const double qij = Q[(size_t)i * rho + j];
#pragma unroll
        for (int k = 0; k < FILTER_COLS; ++k)
            if (k < kn) acc[k] += qij * t[(size_t)(k0 + k) * rho + j];
    }
    const double si = s[i];
#pragma unroll
    for (int k = 0; k < FILTER_COLS; ++k) {
        const double sum = wave_sum(acc[k]);
        if (lane == 0 && k < kn)
            y[(size_t)(k0 + k) * m + i] = table[(size_t)(k0 + k) * PCG_ROW + PCG_STATE] == 0.0 ? si * sum : 0.0;
    }
}

}  // namespace

extern "C" {

int emg3d_dev_pcg_scale(size_t n_cells, int vec_per_col, int ncol, int first, double *u, const double *r, const double *dinv,
                        size_t dinv_stride, const double *table, const double *pq, void *stream)
{
    if (n_cells < 1 || vec_per_col < 1 || ncol < 1 || ncol > 65535 || !u || !r || u == r || !dinv || !table ||
        (dinv_stride != 0 && dinv_stride < n_cells) || (!first && !pq))
        return fail(EMG3D_ERR_BADARG, "pcg_scale: bad argument");
    hipLaunchKernelGGL(k_pcg_scale, dim3(pcg_blocks(n_cells), ncol), dim3(PCG_BLOCK), 0, (hipStream_t)stream, n_cells,
                       vec_per_col, first ? 1 : 0, u, r, dinv, dinv_stride, table, pq);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t emg3d_data_space_filter_ws_len(int rank, int ncol)
{
    return rank < 1 || ncol < 1 ? 0 : (size_t)rank * ncol;
}

int emg3d_dev_data_space_filter(int n_data, int rank, int ncol, const double *q, const double *eigenvalues,
                                const double *s, const double *d, double *y, const double *table, double *ws, size_t ws_len,
                                void *stream)
{
    if (n_data < 1 || rank < 1 || rank > n_data || ncol < 1 || !q || !eigenvalues || !s || !d || !y || d == y || !table ||
        (long long)n_data * rank >= (1LL << 40))
        return fail(EMG3D_ERR_BADARG, "data_space_filter: bad argument");
    if (!ws || ws_len < emg3d_data_space_filter_ws_len(rank, ncol))
        return fail(EMG3D_ERR_SCRATCH, "data_space_filter: workspace too small (emg3d_data_space_filter_ws_len)");
    const hipStream_t st = (hipStream_t)stream;
    for (int k0 = 0; k0 < ncol; k0 += FILTER_COLS) {
        const int kn = ncol - k0 < FILTER_COLS ? ncol - k0 : FILTER_COLS;
        hipLaunchKernelGGL(k_data_filter_down, dim3((rank + 63) / 64), dim3(64, 4, 1), 0, st, n_data, rank, k0, kn, q,
                           eigenvalues, s, d, table, ws);
        hipLaunchKernelGGL(k_data_filter_up, dim3((n_data + 3) / 4), dim3(256), 0, st, n_data, rank, k0, kn, q, s,
                           (const double *)ws, table, y);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int emg3d_dev_pcg_finish(size_t n_cells, int vec_per_col, int ncol, int first, double *z, const double *u, const double *g,
                         const double *r, const double *dinv, size_t dinv_stride, const unsigned char *mask,
                         const double *table, const double *pq, double *ws, size_t ws_len, void *stream)
{
    if (n_cells < 1 || vec_per_col < 1 || ncol < 1 || ncol > 65535 || !z || !u || !g || !r || z == u || z == g || z == r ||
        !dinv || !table || !ws || (dinv_stride != 0 && dinv_stride < n_cells) || (!first && !pq))
        return fail(EMG3D_ERR_BADARG, "pcg_finish: bad argument");
    if (ws_len < emg3d_pcg_ws_len(n_cells, ncol))
        return fail(EMG3D_ERR_SCRATCH, "pcg_finish: workspace too small (emg3d_pcg_ws_len)");
    hipLaunchKernelGGL(k_pcg_finish, dim3(pcg_blocks(n_cells), ncol), dim3(PCG_BLOCK), 0, (hipStream_t)stream, n_cells,
                       vec_per_col, first ? 1 : 0, z, u, g, r, dinv, dinv_stride, mask, table, pq, ws);
    HIP_TRY(hipGetLastError());
    return 0;
}

int emg3d_dev_pcg_direction_z(size_t n_cells, int vec_per_col, int ncol, int first, double *p, const double *z,
                              const double *table, void *stream)
{
    if (n_cells < 1 || vec_per_col < 1 || ncol < 1 || ncol > 65535 || !p || !z || p == z || !table)
        return fail(EMG3D_ERR_BADARG, "pcg_direction_z: bad argument");
    hipLaunchKernelGGL(k_pcg_direction_z, dim3(pcg_blocks(n_cells), ncol), dim3(PCG_BLOCK), 0, (hipStream_t)stream, n_cells,
                       vec_per_col, first ? 1 : 0, p, z, table);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
