// Solve-free sensitivity products: with one kept field per source, e_s, and one per
// receiver, x_r = A^-1 (unit residual source of receiver r), the system matrix being complex symmetric,
//     jvec(v)_{s,r} = c sum_k w_k e_s[k] x_r[k]                 w = cells_to_edges(volume * v), real
//     jtvec(y)      = cells( real(s mu0 t) ),   t[k] = sum_s e_s[k] sum_r conj(y_{s,r}) x_r[k]
// are reductions over the kept fields: no solve. Four kernels, plain fp64, no atomics, every sum in a fixed
// order that depends on the sizes only. Fields of one kind are stacked: field i starts i * stride elements
// behind field 0 (stride >= n; what lies between n and stride is never read).
// Included at the end of kernels.hip (one translation unit), after adjoint.h, whose gathers it shares.
#pragma once

namespace {

// ---- w(v): k_sensitivity_source without the field
struct WeightEdges {
    double *wx, *wy, *wz;
    __device__ __forceinline__ void x(size_t i, double q) const { wx[i] = q; }
    __device__ __forceinline__ void y(size_t i, double q) const { wy[i] = q; }
    __device__ __forceinline__ void z(size_t i, double q) const { wz[i] = q; }
};

__global__ __launch_bounds__(256) void k_edge_weights(int nx, int ny, int nz, const double *vol, const double *vx,
                                                      const double *vy, const double *vz, double *wx, double *wy, double *wz)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x, iy = blockIdx.y * blockDim.y + threadIdx.y, iz = blockIdx.z;
    if (ix > nx || iy > ny || iz > nz) return;
    cells_to_edges(nx, ny, nz, ix, iy, iz, vol, vx, vy, vz, WeightEdges{wx, wy, wz});
}

// ---- cells(real(s mu0 t)): k_gradient_accumulate with the product b e already formed
__device__ __forceinline__ double real_scaled(cplx smu0, cplx t) { return smu0.re * t.re - smu0.im * t.im; }
__device__ __forceinline__ double real_scaled(double smu0, double t) { return smu0 * t; }

template <class T> struct ProductEdges {
    const T *tx, *ty, *tz;
    T smu0;
    __device__ __forceinline__ double x(size_t i) const { return real_scaled(smu0, tx[i]); }
    __device__ __forceinline__ double y(size_t i) const { return real_scaled(smu0, ty[i]); }
    __device__ __forceinline__ double z(size_t i) const { return real_scaled(smu0, tz[i]); }
};

template <class T>
__global__ __launch_bounds__(256) void k_edges_to_cells(int nx, int ny, int nz, const T *tx, const T *ty, const T *tz, T smu0,
                                                        const double *vol, double *gx, double *gy, double *gz)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x, iy = blockIdx.y * blockDim.y + threadIdx.y, iz = blockIdx.z;
    if (ix >= nx || iy >= ny) return;
    edges_to_cell(nx, ny, ix, iy, iz, ProductEdges<T>{tx, ty, tz, smu0}, vol, gx, gy, gz);
}

// ---- dots: out[s, r] = scale sum_k w[k] e_s[k] x_r[k], a tall-skinny GEMM with K = n that is bound by HBM.
// Stage 1: workgroup (chunk, tile) streams DOT_CHUNK consecutive k (16-byte loads for complex fields, one element
// each, coalesced) for a DOT_TS x DOT_TR tile of (s, r), every thread with DOT_TS * DOT_TR accumulators in
// registers (64 VGPRs for complex); then wave shuffles, the four waves through LDS in the order 0..3, and one
// partial per (s, r, chunk) into ws. Stage 2: one workgroup per (s, r) adds the partials of the chunks in a fixed
// order and scales. A tile's rows / columns past ns / nr repeat the last field (cache hits) and are not stored.
constexpr int DOT_TS = 4, DOT_TR = 4, DOT_THREADS = 256, DOT_UNROLL = 2;
constexpr size_t DOT_CHUNK = 8192;          // elements of k per workgroup: 32 per thread

__device__ __forceinline__ double shfl_down_t(double a, int off) { return __shfl_down(a, off, 64); }
__device__ __forceinline__ cplx shfl_down_t(cplx a, int off)
{
    return cplx(__shfl_down(a.re, off, 64), __shfl_down(a.im, off, 64));
}

template <class T>
__global__ __launch_bounds__(DOT_THREADS) void k_sensitivity_dots(size_t n, const T *e, size_t es, int ns, const T *x,
                                                                  size_t xs, int nr, const double *w, size_t nchunk,
                                                                  T *partial)
{
    const int s0 = blockIdx.y * DOT_TS, r0 = blockIdx.z * DOT_TR;
    const T *ep[DOT_TS], *xp[DOT_TR];
#pragma unroll
    for (int i = 0; i < DOT_TS; ++i) ep[i] = e + (size_t)min(s0 + i, ns - 1) * es;
#pragma unroll
    for (int j = 0; j < DOT_TR; ++j) xp[j] = x + (size_t)min(r0 + j, nr - 1) * xs;
    T acc[DOT_TS][DOT_TR];
#pragma unroll
    for (int i = 0; i < DOT_TS; ++i)
#pragma unroll
        for (int j = 0; j < DOT_TR; ++j) acc[i][j] = emg::zero<T>();
    const size_t k0 = (size_t)blockIdx.x * DOT_CHUNK;
    const size_t k1 = k0 + DOT_CHUNK < n ? k0 + DOT_CHUNK : n;
    for (size_t kb = k0 + threadIdx.x; kb < k1; kb += (size_t)DOT_THREADS * DOT_UNROLL) {
#pragma unroll
        for (int u = 0; u < DOT_UNROLL; ++u) {
            const size_t k = kb + (size_t)u * DOT_THREADS;
            if (k < k1) {
                const double wk = w[k];
                T xv[DOT_TR];
#pragma unroll
                for (int j = 0; j < DOT_TR; ++j) xv[j] = xp[j][k];
#pragma unroll
                for (int i = 0; i < DOT_TS; ++i) {
                    const T we = wk * ep[i][k];
#pragma unroll
                    for (int j = 0; j < DOT_TR; ++j) acc[i][j] = emg::mad(we, xv[j], acc[i][j]);
                }
            }
        }
    }
    __shared__ T wsum[DOT_THREADS / 64][DOT_TS * DOT_TR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < DOT_TS; ++i)
#pragma unroll
        for (int j = 0; j < DOT_TR; ++j) {
            T a = acc[i][j];
            for (int off = 32; off > 0; off >>= 1) a += shfl_down_t(a, off);
            if (lane == 0) wsum[wave][i * DOT_TR + j] = a;
        }
    __syncthreads();
    if (threadIdx.x < DOT_TS * DOT_TR) {
        const int s = s0 + (int)threadIdx.x / DOT_TR, r = r0 + (int)threadIdx.x % DOT_TR;
        if (s < ns && r < nr)
            partial[((size_t)s * nr + r) * nchunk + blockIdx.x] =
                (wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + (wsum[2][threadIdx.x] + wsum[3][threadIdx.x]);
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_sensitivity_dots_final(const T *partial, size_t nchunk, T scale, T *out)
{
    partial += (size_t)blockIdx.x * nchunk;          // one workgroup per (s, r)
    __shared__ T sm[256];
    T acc = emg::zero<T>();
    for (size_t i = threadIdx.x; i < nchunk; i += 256) acc += partial[i];
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = scale * sm[0];
}

// ---- combine: t[k] = sum_s e_s[k] (sum_r coef[s, r] x_r[k]), r first, then s, both ascending. One thread per k;
// the first CMB_XR receiver values of its k stay in registers over the loop on s (a survey's receivers: every field
// is read once), further ones are read again per source (cache hits). The coefficients are uniform over the wave:
// the compiler fetches them with scalar loads.
constexpr int CMB_XR = 8;

template <class T>
__global__ __launch_bounds__(256) void k_sensitivity_combine(size_t n, const T *__restrict__ e, size_t es, int ns,
                                                             const T *__restrict__ x, size_t xs, int nr,
                                                             const T *__restrict__ coef, T *__restrict__ t)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    T xv[CMB_XR];
#pragma unroll
    for (int j = 0; j < CMB_XR; ++j) xv[j] = x[(size_t)min(j, nr - 1) * xs + k];
    T sum = emg::zero<T>();
    for (int s = 0; s < ns; ++s) {
        const T *c = coef + (size_t)s * nr;
        T u = emg::zero<T>();
#pragma unroll
        for (int j = 0; j < CMB_XR; ++j)
            if (j < nr) u = emg::mad(c[j], xv[j], u);
        for (int r = CMB_XR; r < nr; ++r) u = emg::mad(c[r], x[(size_t)r * xs + k], u);
        sum = emg::mad(e[(size_t)s * es + k], u, sum);
    }
    t[k] = sum;
}

inline size_t dots_chunks(size_t n) { return (n + DOT_CHUNK - 1) / DOT_CHUNK; }

template <class T>
int launch_dots(size_t n, const void *e, size_t es, int ns, const void *x, size_t xs, int nr, const double *w, T scale,
                void *out, double *ws, hipStream_t st)
{
    const size_t nchunk = dots_chunks(n);
    const dim3 grid((unsigned)nchunk, cdiv(ns, DOT_TS), cdiv(nr, DOT_TR));
    hipLaunchKernelGGL(k_sensitivity_dots<T>, grid, dim3(DOT_THREADS), 0, st, n, (const T *)e, es, ns, (const T *)x, xs, nr, w,
                       nchunk, (T *)ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sensitivity_dots_final<T>, dim3((unsigned)(ns * nr)), dim3(256), 0, st, (const T *)ws, nchunk, scale,
                       (T *)out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int emg3d_dev_edge_weights(int nx, int ny, int nz, const double *volumes, const double *vx, const double *vy,
                           const double *vz, double *wx, double *wy, double *wz, void *stream)
{
    if (nx < 1 || ny < 1 || nz < 1 || !volumes || !vx || !vy || !vz || !wx || !wy || !wz)
        return fail(EMG3D_ERR_BADARG, "edge_weights: bad argument");
    const dim3 block(64, 4, 1), grid(cdiv(nx + 1, 64), cdiv(ny + 1, 4), nz + 1);
    hipLaunchKernelGGL(k_edge_weights, grid, block, 0, (hipStream_t)stream, nx, ny, nz, volumes, vx, vy, vz, wx, wy, wz);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t emg3d_sensitivity_dots_ws_len(int ns, int nr, size_t n)
{
    if (ns < 1 || nr < 1 || n < 1) return 0;
    return 2 * (size_t)ns * (size_t)nr * dots_chunks(n);
}

int emg3d_dev_sensitivity_dots(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                               size_t x_stride, int nr, const double *w, double scale_re, double scale_im, void *out,
                               double *ws, size_t ws_len, void *stream)
{
    if (n < 1 || ns < 1 || nr < 1 || !e || !x || !w || !out || !ws || e_stride < n || x_stride < n)
        return fail(EMG3D_ERR_BADARG, "sensitivity_dots: bad argument");
    if (dots_chunks(n) > 0x7fffffffu || (size_t)ns * (size_t)nr > 0x7fffffffu || cdiv(ns, DOT_TS) > 65535 ||
        cdiv(nr, DOT_TR) > 65535)
        return fail(EMG3D_ERR_BADARG, "sensitivity_dots: too large for one launch");
    if (ws_len < emg3d_sensitivity_dots_ws_len(ns, nr, n))
        return fail(EMG3D_ERR_BADARG, "sensitivity_dots: workspace too small (emg3d_sensitivity_dots_ws_len)");
    return is_complex ? launch_dots<cplx>(n, e, e_stride, ns, x, x_stride, nr, w, cplx(scale_re, scale_im), out, ws,
                                          (hipStream_t)stream)
                      : launch_dots<double>(n, e, e_stride, ns, x, x_stride, nr, w, scale_re, out, ws, (hipStream_t)stream);
}

int emg3d_dev_sensitivity_combine(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                                  size_t x_stride, int nr, const void *coef, void *t, void *stream)
{
    if (n < 1 || ns < 1 || nr < 1 || !e || !x || !coef || !t || e_stride < n || x_stride < n)
        return fail(EMG3D_ERR_BADARG, "sensitivity_combine: bad argument");
    const size_t nblk = (n + 255) / 256;
    if (nblk > 0x7fffffffu) return fail(EMG3D_ERR_BADARG, "sensitivity_combine: too large for one launch");
    const dim3 grid((unsigned)nblk), block(256);
    if (is_complex)
        hipLaunchKernelGGL(k_sensitivity_combine<cplx>, grid, block, 0, (hipStream_t)stream, n, (const cplx *)e, e_stride, ns,
                           (const cplx *)x, x_stride, nr, (const cplx *)coef, (cplx *)t);
    else
        hipLaunchKernelGGL(k_sensitivity_combine<double>, grid, block, 0, (hipStream_t)stream, n, (const double *)e, e_stride,
                           ns, (const double *)x, x_stride, nr, (const double *)coef, (double *)t);
    HIP_TRY(hipGetLastError());
    return 0;
}

int emg3d_dev_edges_to_cells(int nx, int ny, int nz, int is_complex, const void *tx, const void *ty, const void *tz,
                             double smu0_re, double smu0_im, const double *volumes, double *gx, double *gy, double *gz,
                             void *stream)
{
    if (nx < 1 || ny < 1 || nz < 1 || !tx || !ty || !tz || !volumes || !gx || !gy || !gz)
        return fail(EMG3D_ERR_BADARG, "edges_to_cells: bad argument");
    const dim3 block(64, 4, 1), grid(cdiv(nx, 64), cdiv(ny, 4), nz);
    if (is_complex)
        hipLaunchKernelGGL(k_edges_to_cells<cplx>, grid, block, 0, (hipStream_t)stream, nx, ny, nz, (const cplx *)tx,
                           (const cplx *)ty, (const cplx *)tz, cplx(smu0_re, smu0_im), volumes, gx, gy, gz);
    else
        hipLaunchKernelGGL(k_edges_to_cells<double>, grid, block, 0, (hipStream_t)stream, nx, ny, nz, (const double *)tx,
                           (const double *)ty, (const double *)tz, smu0_re, volumes, gx, gy, gz);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
