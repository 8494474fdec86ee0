// The two primitives of subspace methods on device blocks. A block is ncol rows of n doubles, stride
// doubles apart (the model blocks of ReciprocalSensitivity.to_device: n = components x cells).
//     block_gram:    G[i, j]   = sum_k Y_i[k] Y_j[k]            ncol x ncol doubles, symmetric bit for bit
//     block_rotate:  out_j[k]  = sum_i Y_i[k] T[i, j]           T: ncol_in x ncol_out, row-major; out of place
// block_gram has the shape of dots_block (block.h): a wave owns one BG_T x BG_T tile of column pairs (ti <= tj only),
// streams a chunk of BG_CHUNK elements for it with the accumulators in registers and reduces by shuffles; the (up to
// BG_WAVES) waves of a workgroup take different tiles of the SAME chunk, so a value comes from HBM once and from the
// caches for the other tiles. No LDS, no barrier. Stage 2, k_block_gram_final, adds the chunks' partials of an entry
// i <= j in the order of k_pcg_scalar (thread t of 256: t, t + 256, ..., then a binary tree) and writes it to [i, j] AND
// [j, i]. block_rotate: a thread takes V consecutive k and RT_T outputs; the RT_T columns of T of its workgroup lie in
// LDS (every lane reads the same word: a broadcast), Y_i[k] is loaded once per thread and the sum runs over i ascending.
// V = 2 (16-byte loads and stores, reciprocal.h's packs) where every row starts on a 16-byte boundary, V = 1 otherwise.
// Plain fp64, no atomics, every sum in an order fixed by the sizes and that one bit; nothing behind n is read in any
// row, nothing between the rows of out is written.
// Included at the end of kernels.hip (one translation unit), after reciprocal.h and regularise.h (Pack, wave_sum).
#pragma once

namespace {

constexpr int BG_T = 4, BG_WAVES = 8, BG_UNROLL = 2, BG_FINAL = 256;
constexpr int BLOCK_MAX_COLS = 64;
constexpr size_t BG_CHUNK = 4096;           // elements of k per wave: 64 per lane, as DB_CHUNK

inline unsigned block_gram_tiles(int ncol)
{
    const unsigned nt = ((unsigned)ncol + BG_T - 1) / BG_T;
    return nt * (nt + 1) / 2;
}
inline size_t block_gram_chunks(size_t n) { return (n + BG_CHUNK - 1) / BG_CHUNK; }
inline bool block_rows_on_16(const double *p, size_t stride) { return (uintptr_t)p % 16 == 0 && stride % 2 == 0; }

// One k of the tile, element-wise loads.
__device__ __forceinline__ void block_gram_step(size_t k, const double *const *ap, const double *const *bp,
                                                double (&acc)[BG_T][BG_T])
{
    double a[BG_T], b[BG_T];
#pragma unroll
    for (int i = 0; i < BG_T; ++i) a[i] = ap[i][k];
#pragma unroll
    for (int j = 0; j < BG_T; ++j) b[j] = bp[j][k];
#pragma unroll
    for (int i = 0; i < BG_T; ++i)
#pragma unroll
        for (int j = 0; j < BG_T; ++j) acc[i][j] = __builtin_fma(a[i], b[j], acc[i][j]);
}

// Workgroup (chunk, group of blockDim.x / 64 tiles); partial[(i * ncol + j) * nchunk + chunk] for i <= j. Rows of a
// ragged tile repeat the last column (cache hits) and are not stored.
template <int V>
__global__ __launch_bounds__(BG_WAVES * 64) void k_block_gram(size_t n, int ncol, const double *__restrict__ y, size_t ys,
                                                              size_t nchunk, double *__restrict__ partial)
{
    const unsigned nt = ((unsigned)ncol + BG_T - 1) / BG_T, ntile = nt * (nt + 1) / 2;
    const unsigned waves = blockDim.x >> 6, ngroup = (ntile + waves - 1) / waves;
    const int lane = threadIdx.x & 63;
    const unsigned tile = (blockIdx.x % ngroup) * waves + (threadIdx.x >> 6);
    const size_t chunk = blockIdx.x / ngroup;
    if (tile >= ntile) return;                       // (a whole wave: there is no barrier below)
    unsigned ti = 0, rest = tile;                    // row ti of the upper triangle holds the nt - ti tiles tj >= ti
    while (rest >= nt - ti) {
        rest -= nt - ti;
        ++ti;
    }
    const int i0 = (int)ti * BG_T, j0 = (int)(ti + rest) * BG_T;
    const double *ap[BG_T], *bp[BG_T];
#pragma unroll
    for (int i = 0; i < BG_T; ++i) {
        ap[i] = y + (size_t)min(i0 + i, ncol - 1) * ys;
        bp[i] = y + (size_t)min(j0 + i, ncol - 1) * ys;
    }
    double acc[BG_T][BG_T];
#pragma unroll
    for (int i = 0; i < BG_T; ++i)
#pragma unroll
        for (int j = 0; j < BG_T; ++j) acc[i][j] = 0.0;
    const size_t k0 = chunk * BG_CHUNK;
    const size_t k1 = k0 + BG_CHUNK < n ? k0 + BG_CHUNK : n;
    if constexpr (V == 1) {
        for (size_t kb = k0 + lane; kb < k1; kb += (size_t)64 * BG_UNROLL) {
#pragma unroll
            for (int u = 0; u < BG_UNROLL; ++u) {
                const size_t k = kb + (size_t)u * 64;
                if (k < k1) block_gram_step(k, ap, bp, acc);
            }
        }
    } else {
        static_assert(BG_CHUNK % V == 0 && sizeof(double) * V == 16, "a chunk starts on a 16-byte boundary of every row");
        for (size_t k = k0 + (size_t)lane * V; k < k1; k += (size_t)64 * V) {
            if (k + V <= k1) {
                Pack<double, V> a[BG_T], b[BG_T];
#pragma unroll
                for (int i = 0; i < BG_T; ++i) a[i] = load_pack<double, V>(ap[i] + k);
#pragma unroll
                for (int j = 0; j < BG_T; ++j) b[j] = load_pack<double, V>(bp[j] + k);
#pragma unroll
                for (int m = 0; m < V; ++m)
#pragma unroll
                    for (int i = 0; i < BG_T; ++i)
#pragma unroll
                        for (int j = 0; j < BG_T; ++j) acc[i][j] = __builtin_fma(a[i].v[m], b[j].v[m], acc[i][j]);
            } else {
                for (size_t kk = k; kk < k1; ++kk) block_gram_step(kk, ap, bp, acc);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < BG_T; ++i)
#pragma unroll
        for (int j = 0; j < BG_T; ++j) {
            const double a = wave_sum(acc[i][j]);
            if (lane == 0 && i0 + i <= j0 + j && j0 + j < ncol)
                partial[((size_t)(i0 + i) * ncol + (j0 + j)) * nchunk + chunk] = a;
        }
}

// One workgroup per entry (i = blockIdx.y, j = blockIdx.x), i <= j: the sum of its nchunk partials, mirrored.
__global__ __launch_bounds__(BG_FINAL) void k_block_gram_final(int ncol, size_t nchunk, const double *__restrict__ partial,
                                                               double *__restrict__ g)
{
    const int i = blockIdx.y, j = blockIdx.x;
    if (i > j) return;                               // (the whole workgroup)
    __shared__ double sm[BG_FINAL];
    const double *src = partial + ((size_t)i * ncol + j) * nchunk;
    double a = 0.0;
    for (size_t b = threadIdx.x; b < nchunk; b += BG_FINAL) a += src[b];
    sm[threadIdx.x] = a;
    __syncthreads();
    for (int s = BG_FINAL / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) g[(size_t)i * ncol + j] = g[(size_t)j * ncol + i] = sm[0];
}

constexpr int RT_T = 16, RT_BLOCK = 256;

// Workgroup (RT_BLOCK x V consecutive k, tile of RT_T outputs). Outputs of a ragged tile are computed with T = 0 and not
// stored; the thread of an odd n's last element (V = 2) takes that one alone.
template <int V>
__global__ __launch_bounds__(RT_BLOCK) void k_block_rotate(size_t n, int nin, int nout, const double *__restrict__ y, size_t ys,
                                                           const double *__restrict__ t, double *__restrict__ out, size_t os)
{
    __shared__ double tl[BLOCK_MAX_COLS * RT_T];
    const int j0 = blockIdx.y * RT_T;
    for (int e = threadIdx.x; e < nin * RT_T; e += RT_BLOCK) {
        const int i = e / RT_T, j = j0 + e % RT_T;
        tl[e] = j < nout ? t[(size_t)i * nout + j] : 0.0;
    }
    __syncthreads();
    const size_t k = ((size_t)blockIdx.x * RT_BLOCK + threadIdx.x) * V;
    if (k >= n) return;                              // (behind the only barrier)
    const bool full = k + V <= n;
    double acc[V][RT_T];
#pragma unroll
    for (int m = 0; m < V; ++m)
#pragma unroll
        for (int j = 0; j < RT_T; ++j) acc[m][j] = 0.0;
    const double *src = y + k;
#pragma unroll 2
    for (int i = 0; i < nin; ++i) {
        double v[V];
        if constexpr (V == 1) {
            v[0] = src[(size_t)i * ys];
        } else {
            if (full) {
                const Pack<double, V> p = load_pack<double, V>(src + (size_t)i * ys);
#pragma unroll
                for (int m = 0; m < V; ++m) v[m] = p.v[m];
            } else {
                v[0] = src[(size_t)i * ys];
#pragma unroll
                for (int m = 1; m < V; ++m) v[m] = 0.0;
            }
        }
#pragma unroll
        for (int m = 0; m < V; ++m)
#pragma unroll
            for (int j = 0; j < RT_T; ++j) acc[m][j] = __builtin_fma(v[m], tl[i * RT_T + j], acc[m][j]);
    }
#pragma unroll
    for (int j = 0; j < RT_T; ++j) {
        if (j0 + j >= nout) continue;
        double *dst = out + (size_t)(j0 + j) * os + k;
        if constexpr (V == 1) {
            *dst = acc[0][j];
        } else {
            if (full) {
                Pack<double, V> p;
#pragma unroll
                for (int m = 0; m < V; ++m) p.v[m] = acc[m][j];
                *reinterpret_cast<Pack<double, V> *>(dst) = p;
            } else {
                *dst = acc[0][j];
            }
        }
    }
}

}  // namespace

extern "C" {

size_t emg3d_block_gram_ws_len(size_t n, int ncol)
{
    if (n < 1 || ncol < 1 || ncol > BLOCK_MAX_COLS) return 0;
    return (size_t)ncol * ncol * block_gram_chunks(n);
}

int emg3d_dev_block_gram(size_t n, int ncol, const double *y, size_t stride, double *g, double *ws, void *stream)
{
    if (!y || !g || !ws) return fail(EMG3D_ERR_BADARG, "block_gram: null pointer");
    if (n < 1 || ncol < 1 || ncol > BLOCK_MAX_COLS)
        return fail(EMG3D_ERR_BADARG, "block_gram: n < 1, or ncol outside 1..64");
    if (stride < n) return fail(EMG3D_ERR_BADARG, "block_gram: the stride is smaller than a row");
    const size_t nchunk = block_gram_chunks(n);
    const unsigned ntile = block_gram_tiles(ncol);
    const unsigned waves = ntile < (unsigned)BG_WAVES ? ntile : (unsigned)BG_WAVES, ngroup = (ntile + waves - 1) / waves;
    if (nchunk * ngroup > (size_t)INT_MAX) return fail(EMG3D_ERR_BADARG, "block_gram: too large for one launch");
    const dim3 grid((unsigned)(nchunk * ngroup)), block(waves * 64);
    if (block_rows_on_16(y, stride))
        hipLaunchKernelGGL(k_block_gram<2>, grid, block, 0, (hipStream_t)stream, n, ncol, y, stride, nchunk, ws);
    else
        hipLaunchKernelGGL(k_block_gram<1>, grid, block, 0, (hipStream_t)stream, n, ncol, y, stride, nchunk, ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_block_gram_final, dim3(ncol, ncol), dim3(BG_FINAL), 0, (hipStream_t)stream, ncol, nchunk, ws, g);
    HIP_TRY(hipGetLastError());
    return 0;
}

int emg3d_dev_block_rotate(size_t n, int ncol_in, int ncol_out, const double *y, size_t stride, const double *t, double *out,
                           size_t out_stride, void *stream)
{
    if (!y || !t || !out) return fail(EMG3D_ERR_BADARG, "block_rotate: null pointer");
    if (n < 1 || ncol_out < 1 || ncol_out > ncol_in || ncol_in > BLOCK_MAX_COLS)
        return fail(EMG3D_ERR_BADARG, "block_rotate: n < 1, or not 1 <= ncol_out <= ncol_in <= 64");
    if (stride < n || out_stride < n) return fail(EMG3D_ERR_BADARG, "block_rotate: a stride is smaller than a row");
    const double *const y_end = y + (size_t)(ncol_in - 1) * stride + n, *const o_end = out + (size_t)(ncol_out - 1) * out_stride + n;
    if ((const double *)out < y_end && y < o_end) return fail(EMG3D_ERR_BADARG, "block_rotate: y and out overlap");
    const int V = block_rows_on_16(y, stride) && block_rows_on_16(out, out_stride) ? 2 : 1;
    const size_t nblock = (n + (size_t)RT_BLOCK * V - 1) / ((size_t)RT_BLOCK * V);
    if (nblock > (size_t)INT_MAX) return fail(EMG3D_ERR_BADARG, "block_rotate: too large for one launch");
    const dim3 grid((unsigned)nblock, cdiv(ncol_out, RT_T));
    if (V == 2)
        hipLaunchKernelGGL(k_block_rotate<2>, grid, dim3(RT_BLOCK), 0, (hipStream_t)stream, n, ncol_in, ncol_out, y, stride, t, out,
                           out_stride);
    else
        hipLaunchKernelGGL(k_block_rotate<1>, grid, dim3(RT_BLOCK), 0, (hipStream_t)stream, n, ncol_in, ncol_out, y, stride, t, out,
                           out_stride);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
