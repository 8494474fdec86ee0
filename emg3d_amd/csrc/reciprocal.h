// Solve-free sensitivity products: with one kept field per source, e_s, and one per
// receiver, x_r = A^-1 (unit residual source of receiver r), the system matrix being complex symmetric,
//     jvec(v)_{s,r} = c sum_k w_k e_s[k] x_r[k]                 w = cells_to_edges(volume * v), real
//     jtvec(y)      = cells( real(s mu0 t) ),   t[k] = sum_s e_s[k] sum_r conj(y_{s,r}) x_r[k]
// are reductions over the kept fields: no solve. Four kernels, plain fp64, no atomics, every sum in a fixed
// order that depends on the sizes only. Fields of one kind are stacked: field i starts i * stride elements
// behind field 0 (stride >= n; what lies between n and stride is never read).
// The two reductions over the stacks, dots and combine, separate the type S the stacks are STORED in from the type T
// of the arithmetic: S = T, or T's single-precision partner of cplx.h, widened as it is loaded.
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

// One k of the tile: acc[i][j] += (w[k] e_i[k]) x_j[k], the fields widened as they arrive.
template <class T, class S>
__device__ __forceinline__ void dots_step(size_t k, const double *w, const S *const *ep, const S *const *xp,
                                          T (&acc)[DOT_TS][DOT_TR])
{
    const double wk = w[k];
    T xv[DOT_TR];
#pragma unroll
    for (int j = 0; j < DOT_TR; ++j) xv[j] = emg::widen(xp[j][k]);
#pragma unroll
    for (int i = 0; i < DOT_TS; ++i) {
        const T we = wk * emg::widen(ep[i][k]);
#pragma unroll
        for (int j = 0; j < DOT_TR; ++j) acc[i][j] = emg::mad(we, xv[j], acc[i][j]);
    }
}

// V consecutive values of a stack, fetched with 16-byte loads: the address must be a multiple of 16.
template <class S, int V> struct alignas(16) Pack { S v[V]; };
template <class S, int V> __device__ __forceinline__ Pack<S, V> load_pack(const S *p)
{
    return *reinterpret_cast<const Pack<S, V> *>(p);
}

// S: the type the stacks are stored in (T, or its single-precision partner: values are widened when they are loaded,
// every operation is T's). V: consecutive k per lane. V = 1: element-wise loads -- 16 bytes each for S = cplx. V > 1
// (S narrower than T only): a lane takes V consecutive k with ONE 16-byte load per field (V = 2 for cplxf, 4 for
// float), which needs every row of both stacks and w on a 16-byte boundary: launch_dots decides. The last lane of a
// row that is no multiple of V long goes element by element, so nothing behind n is read.
template <class T, class S, int V>
__global__ __launch_bounds__(DOT_THREADS) void k_sensitivity_dots(size_t n, const S *e, size_t es, int ns, const S *x,
                                                                  size_t xs, int nr, const double *w, size_t nchunk,
                                                                  T *partial)
{
    const int s0 = blockIdx.y * DOT_TS, r0 = blockIdx.z * DOT_TR;
    const S *ep[DOT_TS], *xp[DOT_TR];
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
    if constexpr (V == 1) {
        for (size_t kb = k0 + threadIdx.x; kb < k1; kb += (size_t)DOT_THREADS * DOT_UNROLL) {
#pragma unroll
            for (int u = 0; u < DOT_UNROLL; ++u) {
                const size_t k = kb + (size_t)u * DOT_THREADS;
                if (k < k1) dots_step<T, S>(k, w, ep, xp, acc);
            }
        }
    } else {
        static_assert(DOT_CHUNK % V == 0 && sizeof(S) * V == 16, "a chunk starts on a 16-byte boundary of every row");
        for (size_t kb = k0 + (size_t)threadIdx.x * V; kb < k1; kb += (size_t)DOT_THREADS * DOT_UNROLL * V) {
#pragma unroll
            for (int u = 0; u < DOT_UNROLL; ++u) {
                const size_t k = kb + (size_t)u * DOT_THREADS * V;
                if (k + V <= k1) {
                    const Pack<double, V> wk = load_pack<double, V>(w + k);
                    Pack<S, V> xv[DOT_TR];
#pragma unroll
                    for (int j = 0; j < DOT_TR; ++j) xv[j] = load_pack<S, V>(xp[j] + k);
#pragma unroll
                    for (int i = 0; i < DOT_TS; ++i) {
                        const Pack<S, V> ev = load_pack<S, V>(ep[i] + k);
#pragma unroll
                        for (int m = 0; m < V; ++m) {
                            const T we = wk.v[m] * emg::widen(ev.v[m]);
#pragma unroll
                            for (int j = 0; j < DOT_TR; ++j) acc[i][j] = emg::mad(we, emg::widen(xv[j].v[m]), acc[i][j]);
                        }
                    }
                } else {
                    for (size_t kk = k; kk < k1; ++kk) dots_step<T, S>(kk, w, ep, xp, acc);
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

template <class T, class S>
__device__ __forceinline__ T combine_one(size_t k, const S *__restrict__ e, size_t es, int ns, const S *__restrict__ x,
                                         size_t xs, int nr, const T *__restrict__ coef)
{
    T xv[CMB_XR];
#pragma unroll
    for (int j = 0; j < CMB_XR; ++j) xv[j] = emg::widen(x[(size_t)min(j, nr - 1) * xs + k]);
    T sum = emg::zero<T>();
    for (int s = 0; s < ns; ++s) {
        const T *c = coef + (size_t)s * nr;
        T u = emg::zero<T>();
#pragma unroll
        for (int j = 0; j < CMB_XR; ++j)
            if (j < nr) u = emg::mad(c[j], xv[j], u);
        for (int r = CMB_XR; r < nr; ++r) u = emg::mad(c[r], emg::widen(x[(size_t)r * xs + k]), u);
        sum = emg::mad(emg::widen(e[(size_t)s * es + k]), u, sum);
    }
    return sum;
}

// S, V: as in k_sensitivity_dots. V > 1: one thread per V consecutive k, a 16-byte load per field and 16-byte stores of
// t (every row of both stacks and t on a 16-byte boundary: the launcher decides); each of the V sums is combine_one's,
// term by term, so t does not depend on V. The last thread of an n that is no multiple of V goes element by element.
template <class T, class S, int V>
__global__ __launch_bounds__(256) void k_sensitivity_combine(size_t n, const S *__restrict__ e, size_t es, int ns,
                                                             const S *__restrict__ x, size_t xs, int nr,
                                                             const T *__restrict__ coef, T *__restrict__ t)
{
    const size_t k = ((size_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (k >= n) return;
    if constexpr (V == 1) {
        t[k] = combine_one<T, S>(k, e, es, ns, x, xs, nr, coef);
    } else {
        static_assert(sizeof(S) * V == 16, "one 16-byte load per field");
        if (k + V > n) {
            for (size_t kk = k; kk < n; ++kk) t[kk] = combine_one<T, S>(kk, e, es, ns, x, xs, nr, coef);
            return;
        }
        Pack<S, V> xv[CMB_XR];
#pragma unroll
        for (int j = 0; j < CMB_XR; ++j) xv[j] = load_pack<S, V>(x + (size_t)min(j, nr - 1) * xs + k);
        Pack<T, V> sum;
#pragma unroll
        for (int m = 0; m < V; ++m) sum.v[m] = emg::zero<T>();
        for (int s = 0; s < ns; ++s) {
            const T *c = coef + (size_t)s * nr;
            T u[V];
#pragma unroll
            for (int m = 0; m < V; ++m) u[m] = emg::zero<T>();
#pragma unroll
            for (int j = 0; j < CMB_XR; ++j)
                if (j < nr) {
#pragma unroll
                    for (int m = 0; m < V; ++m) u[m] = emg::mad(c[j], emg::widen(xv[j].v[m]), u[m]);
                }
            for (int r = CMB_XR; r < nr; ++r) {
                const Pack<S, V> xr = load_pack<S, V>(x + (size_t)r * xs + k);
#pragma unroll
                for (int m = 0; m < V; ++m) u[m] = emg::mad(c[r], emg::widen(xr.v[m]), u[m]);
            }
            const Pack<S, V> ev = load_pack<S, V>(e + (size_t)s * es + k);
#pragma unroll
            for (int m = 0; m < V; ++m) sum.v[m] = emg::mad(emg::widen(ev.v[m]), u[m], sum.v[m]);
        }
        *reinterpret_cast<Pack<T, V> *>(t + k) = sum;
    }
}

inline size_t dots_chunks(size_t n) { return (n + DOT_CHUNK - 1) / DOT_CHUNK; }

// Every row of a stack of S starts on a 16-byte boundary: the base does, and the stride is a whole number of them.
template <class S> inline bool rows_on_16_bytes(const void *base, size_t stride)
{
    return (uintptr_t)base % 16 == 0 && stride * sizeof(S) % 16 == 0;
}

template <class T, class S, int V>
int launch_dots_as(size_t n, const void *e, size_t es, int ns, const void *x, size_t xs, int nr, const double *w, T scale,
                   void *out, double *ws, hipStream_t st)
{
    const size_t nchunk = dots_chunks(n);
    const dim3 grid((unsigned)nchunk, cdiv(ns, DOT_TS), cdiv(nr, DOT_TR));
    hipLaunchKernelGGL((k_sensitivity_dots<T, S, V>), grid, dim3(DOT_THREADS), 0, st, n, (const S *)e, es, ns, (const S *)x, xs,
                       nr, w, nchunk, (T *)ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sensitivity_dots_final<T>, dim3((unsigned)(ns * nr)), dim3(256), 0, st, (const T *)ws, nchunk, scale,
                       (T *)out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Stacks stored as S. Narrow stacks: 16-byte loads (V = 16 / sizeof(S) consecutive k per lane) where every row of
// both stacks and w allow them, element-wise loads otherwise -- decided here, from the addresses and strides alone.
template <class T, class S>
int launch_dots(size_t n, const void *e, size_t es, int ns, const void *x, size_t xs, int nr, const double *w, T scale,
                void *out, double *ws, hipStream_t st)
{
    if constexpr (sizeof(S) < sizeof(T)) {
        if (rows_on_16_bytes<S>(e, es) && rows_on_16_bytes<S>(x, xs) && (uintptr_t)w % 16 == 0)
            return launch_dots_as<T, S, (int)(16 / sizeof(S))>(n, e, es, ns, x, xs, nr, w, scale, out, ws, st);
    }
    return launch_dots_as<T, S, 1>(n, e, es, ns, x, xs, nr, w, scale, out, ws, st);
}

template <class T, class S>
int launch_combine(size_t n, const void *e, size_t es, int ns, const void *x, size_t xs, int nr, const void *coef, void *t,
                   hipStream_t st)
{
    if constexpr (sizeof(S) < sizeof(T)) {
        if (rows_on_16_bytes<S>(e, es) && rows_on_16_bytes<S>(x, xs) && (uintptr_t)t % 16 == 0) {
            constexpr int V = (int)(16 / sizeof(S));
            const size_t nblk = ((n + V - 1) / V + 255) / 256;
            hipLaunchKernelGGL((k_sensitivity_combine<T, S, V>), dim3((unsigned)nblk), dim3(256), 0, st, n, (const S *)e, es, ns,
                               (const S *)x, xs, nr, (const T *)coef, (T *)t);
            HIP_TRY(hipGetLastError());
            return 0;
        }
    }
    hipLaunchKernelGGL((k_sensitivity_combine<T, S, 1>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (const S *)e, es,
                       ns, (const S *)x, xs, nr, (const T *)coef, (T *)t);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The checks of emg3d_dev_sensitivity_dots / _combine and of their _sp siblings (SP: stacks in single precision).
template <bool SP>
int sensitivity_dots(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x, size_t x_stride, int nr,
                     const double *w, double scale_re, double scale_im, void *out, double *ws, size_t ws_len, void *stream)
{
    if (n < 1 || ns < 1 || nr < 1 || !e || !x || !w || !out || !ws || e_stride < n || x_stride < n)
        return fail(EMG3D_ERR_BADARG, "sensitivity_dots: bad argument");
    if (dots_chunks(n) > 0x7fffffffu || (size_t)ns * (size_t)nr > 0x7fffffffu || cdiv(ns, DOT_TS) > 65535 ||
        cdiv(nr, DOT_TR) > 65535)
        return fail(EMG3D_ERR_BADARG, "sensitivity_dots: too large for one launch");
    if (ws_len < 2 * (size_t)ns * (size_t)nr * dots_chunks(n))
        return fail(EMG3D_ERR_BADARG, "sensitivity_dots: workspace too small (emg3d_sensitivity_dots_ws_len)");
    using C = std::conditional_t<SP, emg::cplxf, cplx>;
    using R = std::conditional_t<SP, float, double>;
    return is_complex ? launch_dots<cplx, C>(n, e, e_stride, ns, x, x_stride, nr, w, cplx(scale_re, scale_im), out, ws,
                                             (hipStream_t)stream)
                      : launch_dots<double, R>(n, e, e_stride, ns, x, x_stride, nr, w, scale_re, out, ws, (hipStream_t)stream);
}

template <bool SP>
int sensitivity_combine(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x, size_t x_stride,
                        int nr, const void *coef, void *t, void *stream)
{
    if (n < 1 || ns < 1 || nr < 1 || !e || !x || !coef || !t || e_stride < n || x_stride < n)
        return fail(EMG3D_ERR_BADARG, "sensitivity_combine: bad argument");
    if ((n + 255) / 256 > 0x7fffffffu) return fail(EMG3D_ERR_BADARG, "sensitivity_combine: too large for one launch");
    using C = std::conditional_t<SP, emg::cplxf, cplx>;
    using R = std::conditional_t<SP, float, double>;
    return is_complex ? launch_combine<cplx, C>(n, e, e_stride, ns, x, x_stride, nr, coef, t, (hipStream_t)stream)
                      : launch_combine<double, R>(n, e, e_stride, ns, x, x_stride, nr, coef, t, (hipStream_t)stream);
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
    return sensitivity_dots<false>(n, is_complex, e, e_stride, ns, x, x_stride, nr, w, scale_re, scale_im, out, ws, ws_len,
                                   stream);
}

int emg3d_dev_sensitivity_dots_sp(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                                  size_t x_stride, int nr, const double *w, double scale_re, double scale_im, void *out,
                                  double *ws, size_t ws_len, void *stream)
{
    return sensitivity_dots<true>(n, is_complex, e, e_stride, ns, x, x_stride, nr, w, scale_re, scale_im, out, ws, ws_len,
                                  stream);
}

int emg3d_dev_sensitivity_combine(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                                  size_t x_stride, int nr, const void *coef, void *t, void *stream)
{
    return sensitivity_combine<false>(n, is_complex, e, e_stride, ns, x, x_stride, nr, coef, t, stream);
}

int emg3d_dev_sensitivity_combine_sp(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                                     size_t x_stride, int nr, const void *coef, void *t, void *stream)
{
    return sensitivity_combine<true>(n, is_complex, e, e_stride, ns, x, x_stride, nr, coef, t, stream);
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
