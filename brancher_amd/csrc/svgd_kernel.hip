// svgd_kernel.hip — the step of Stein variational gradient descent that couples the particles (`inference.py:277-327` of the
// reference, Liu & Wang 2016) behind the C ABI: bsvi_svgd_direction (include/bsvi.h).
//
//   d_ij = |theta_i - theta_j|^2,  bw = 2 median_{i != j}(sqrt d_ij)^2 / log N (or the caller's),  K_ij = exp(-d_ij / (2 bw)),
//   out_i = sum_j K_ij grad_j - (1 / bw) (theta_i sum_j K_ij - sum_j K_ij theta_j)
//
// Three launches, no float atomics, every sum in a fixed order (two calls on the same inputs give the same bits):
//
//   svgd_gram      grid (splits, row tiles).  A workgroup walks its stretch of D in chunks of 32 columns: the chunk of ALL particles goes
//                  through LDS once, k-major (X[k][i]), is centred there (the column mean is local to a chunk: d_ij = S_ii + S_jj - 2 S_ij
//                  cancels badly for a cloud far from the origin, the centred one does not), and serves v_mfma_f32_32x32x2_f32 as the A
//                  operand (the workgroup's 32 rows) AND as the transposed B operand (the column tiles at and right of the diagonal, two
//                  per wave).  S is symmetric: only tiles tj >= ti are computed.  Partials [splits][NP][NP], NP = N padded to 32.
//   svgd_kernel    ONE workgroup of 1024: adds the partials in split order, d_ij = max(S_ii + S_jj - 2 S_ij, 0) for i < j, the exact
//                  median of the triangle by a radix select on the float bit patterns (four 8-bit passes, integer LDS histograms; the two
//                  middle values when the count is even), bw, K (exactly symmetric, zero in the padding) and its row sums.
//   svgd_product   grid over tiles of 64 columns of D.  out^T = [grad | theta]^T K: the workgroup walks the particles j in steps of 16,
//                  stages rows j of K (K is symmetric: row j is column j) and of its 64 columns of grad and theta in LDS — each element
//                  of grad and theta is read once, 16 bytes per lane where the alignment allows — and runs the f32-input MFMA with the
//                  DATA as the A operand, so that a lane of the accumulator holds 4 consecutive columns of one particle: the epilogue
//                  combines the two accumulators in registers and stores 16 bytes per lane.  A workgroup reads every row of its columns
//                  of grad before it writes any of out, and nobody else touches those columns: out may alias grad.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "bsvi.h"
#include "bsvi_internal.h"

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kMaxParticles = 256;
constexpr int kChunk = 32;                  // columns of D per Gram step
constexpr int kMaxSplits = 64;
constexpr int kColTile = 64;                // columns of D per workgroup of the product
constexpr int kStep = 16;                   // particles per step of the product
constexpr size_t kHeaderBytes = 256;        // {bw, 1 / bw} and padding

struct Plan {
    int np, nt, n_chunks, splits, chunks_per_split;
    size_t off_s, off_k, off_ksum, off_mean, off_part, bytes;
};

Plan plan_for(int n, int dim) {
    Plan p;
    p.nt = (n + 31) / 32;
    p.np = p.nt * 32;
    p.n_chunks = (dim + kChunk - 1) / kChunk;
    int max_splits = (1 << 20) / (p.np * p.np);                 // at most 4 MiB of partials for the one workgroup that adds them
    if (max_splits > kMaxSplits) max_splits = kMaxSplits;
    p.splits = p.n_chunks < max_splits ? p.n_chunks : max_splits;
    p.chunks_per_split = (p.n_chunks + p.splits - 1) / p.splits;
    p.splits = (p.n_chunks + p.chunks_per_split - 1) / p.chunks_per_split;      // no empty split
    const size_t mat = (size_t)p.np * p.np * sizeof(float);
    p.off_s = kHeaderBytes;
    p.off_k = p.off_s + mat;
    p.off_ksum = p.off_k + mat;
    p.off_mean = p.off_ksum + (size_t)kMaxParticles * sizeof(float);
    p.off_part = p.off_mean + (size_t)p.n_chunks * kChunk * sizeof(float);
    p.bytes = p.off_part + (size_t)p.splits * mat;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------
//  1. partial Gram matrices of the centred particles
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void svgd_gram(const float* __restrict__ theta, float* __restrict__ part, float* __restrict__ means, int N, int D, long ld,
                                                 int NP, int NT, int chunks_per_split, int n_chunks) {
    __shared__ float X[kChunk][kMaxParticles + 1];
    __shared__ float red[8][kChunk];
    const int t = threadIdx.x, c = t & 31, g = t >> 5;          // g: the wave-half 0..7 — rows g, g + 8, ... of column c
    const int w = t >> 6, lane = t & 63, lm = lane & 31, lk = lane >> 5;
    const int split = blockIdx.x, ti = blockIdx.y;
    const int first = split * chunks_per_split, last = min(first + chunks_per_split, n_chunks);
    const int rows_per_thread = NP / 8;                          // 4 .. 32
    const float inv_n = 1.0f / (float)N;

    floatx16 acc[2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;

    float pre[kMaxParticles / 8];
    auto fetch = [&](int chunk) {
        const int k = chunk * kChunk + c;
#pragma unroll
        for (int m = 0; m < kMaxParticles / 8; ++m) {
            const int i = g + 8 * m;
            pre[m] = (m < rows_per_thread && i < N && k < D) ? theta[(long)i * ld + k] : 0.0f;
        }
    };
    fetch(first);
    for (int chunk = first; chunk < last; ++chunk) {
        __syncthreads();                                         // the products of the previous chunk are done with X
        float s = 0.0f;
#pragma unroll
        for (int m = 0; m < kMaxParticles / 8; ++m)
            if (m < rows_per_thread) { X[c][g + 8 * m] = pre[m]; s += pre[m]; }
        red[g][c] = s;
        __syncthreads();
        if (chunk + 1 < last) fetch(chunk + 1);                  // in flight behind the centring and the products
        float mean = 0.0f;
#pragma unroll
        for (int q = 0; q < 8; ++q) mean += red[q][c];
        mean *= inv_n;
        if (ti == 0 && g == 0) means[chunk * kChunk + c] = mean;     // (the product launch centres theta with the same numbers)
        for (int m = 0; m < rows_per_thread; ++m) {
            const int i = g + 8 * m;
            if (i < N) X[c][i] -= mean;                           // (rows past N stay zero)
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kChunk / 2; ++kk) {
            const float a = X[2 * kk + lk][ti * 32 + lm];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int tj = ti + w + 4 * q;
                if (tj < NT) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, X[2 * kk + lk][tj * 32 + lm], acc[q], 0, 0, 0);
            }
        }
    }
    // acc[q][r] is S[32 ti + 8 (r >> 2) + 4 lk + (r & 3)][32 tj + lm] of this split
    float* out = part + (size_t)split * NP * NP;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int tj = ti + w + 4 * q;
        if (tj >= NT) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 32 * ti + 8 * (r >> 2) + 4 * lk + (r & 3);
            out[(size_t)i * NP + 32 * tj + lm] = acc[q][r];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
//  2. distances, bandwidth, kernel matrix, row sums: one workgroup
// ---------------------------------------------------------------------------------------------------------------------
// the value of rank `rank` (0-based, ascending) among the bit patterns of d_ij, i < j: non-negative floats order like their bits
__device__ uint32_t svgd_select(const float* S, int N, int NP, uint32_t rank, uint32_t* hist, uint32_t* pick) {
    const int t = threadIdx.x;
    uint32_t prefix = 0u, mask = 0u;
    for (int pass = 3; pass >= 0; --pass) {
        const int shift = 8 * pass;
        if (t < 256) hist[t] = 0u;
        __syncthreads();
        for (int e = t; e < N * N; e += 1024) {
            const int i = e / N, j = e - i * N;
            if (j <= i) continue;
            const uint32_t bits = __float_as_uint(S[(size_t)i * NP + j]);
            if ((bits & mask) == prefix) atomicAdd(&hist[(bits >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (t == 0) {
            uint32_t before = 0u, bin = 0u;
            for (; bin < 255u; ++bin) {
                if (before + hist[bin] > rank) break;
                before += hist[bin];
            }
            pick[0] = bin;
            pick[1] = rank - before;
        }
        __syncthreads();
        prefix |= pick[0] << shift;
        mask |= 255u << shift;
        rank = pick[1];
        __syncthreads();
    }
    return prefix;
}

__global__ __launch_bounds__(1024) void svgd_kernel(const float* __restrict__ part, float* __restrict__ S, float* __restrict__ K,
                                                    float* __restrict__ ksum, float* __restrict__ header, float* __restrict__ bw_out,
                                                    int N, int NP, int NT, int splits, float fixed_bw) {
    __shared__ float diag[kMaxParticles];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t pick[2];
    const int t = threadIdx.x;
    // S = the partials added in split order (tiles at and right of the diagonal: the others were never written)
    for (int e = t; e < NP * NP; e += 1024) {
        const int i = e / NP, j = e - i * NP;
        if ((j >> 5) < (i >> 5)) continue;
        float s = 0.0f;
        for (int q = 0; q < splits; ++q) s += part[(size_t)q * NP * NP + e];
        S[e] = s;
    }
    __syncthreads();
    if (t < N) diag[t] = S[(size_t)t * NP + t];
    __syncthreads();
    // d_ij over the strict upper triangle, in place
    for (int e = t; e < N * N; e += 1024) {
        const int i = e / N, j = e - i * N;
        if (j <= i) continue;
        float* s = S + (size_t)i * NP + j;
        *s = fmaxf(diag[i] + diag[j] - 2.0f * *s, 0.0f);
    }
    __syncthreads();
    float bw = fixed_bw;
    if (!(bw > 0.0f)) {
        const uint32_t m = (uint32_t)N * (uint32_t)(N - 1) / 2u;
        const uint32_t lo = svgd_select(S, N, NP, (m - 1u) / 2u, hist, pick);
        const uint32_t hi = (m & 1u) ? lo : svgd_select(S, N, NP, m / 2u, hist, pick);
        const float med = 0.5f * (sqrtf(__uint_as_float(lo)) + sqrtf(__uint_as_float(hi)));
        bw = 2.0f * med * med / logf((float)N);
    }
    const bool good = bw > 0.0f && bw < __int_as_float(0x7f800000);
    if (t == 0) {
        header[0] = good ? bw : 0.0f;                            // 0: degenerate — the product launch writes nothing
        header[1] = good ? 1.0f / bw : 0.0f;
        if (bw_out) *bw_out = good ? bw : 0.0f;
    }
    const float scale = good ? -0.5f / bw : 0.0f;
    for (int e = t; e < NP * NP; e += 1024) {
        const int i = e / NP, j = e - i * NP;
        float k = 0.0f;
        if (i < N && j < N) k = i == j ? 1.0f : expf(scale * S[(size_t)min(i, j) * NP + max(i, j)]);
        K[e] = k;
    }
    __syncthreads();
    // row sums: a wave per row, lanes over the columns, then a fixed butterfly
    const int w = t >> 6, lane = t & 63;
    for (int i = w; i < N; i += 16) {
        float s = 0.0f;
        for (int j = lane; j < NP; j += 64) s += K[(size_t)i * NP + j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) ksum[i] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
//  3. out = K grad - (1 / bw) (diag(k) theta - K theta)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ floatx4 svgd_load4(const float* row, int c, int D, bool vec) {
    if (vec && c + 3 < D) return *reinterpret_cast<const floatx4*>(row + c);
    floatx4 v;
    v.x = c < D ? row[c] : 0.0f;
    v.y = c + 1 < D ? row[c + 1] : 0.0f;
    v.z = c + 2 < D ? row[c + 2] : 0.0f;
    v.w = c + 3 < D ? row[c + 3] : 0.0f;
    return v;
}

__global__ __launch_bounds__(256) void svgd_product(const float* __restrict__ theta, const float* grad, float* out,
                                                    const float* __restrict__ K, const float* __restrict__ ksum, const float* __restrict__ means,
                                                    const float* __restrict__ header, int N, int D, long ld, int NP, int NT, int vec) {
    __shared__ __attribute__((aligned(16))) float Ks[kStep][kMaxParticles + 4];
    __shared__ __attribute__((aligned(16))) float Gs[kStep][kColTile + 4];
    __shared__ __attribute__((aligned(16))) float Ts[kStep][kColTile + 4];
    const float bw = header[0], inv_bw = header[1];
    if (!(bw > 0.0f)) return;                                    // degenerate bandwidth: the host reports it, nothing is written
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, lm = lane & 31, lk = lane >> 5;
    const int c0 = blockIdx.x * kColTile;
    const int ct = w & 1;                                        // the wave's 32 columns; its row tiles: (w >> 1) + 2 q
    const int srow = t >> 4, scol = (t & 15) * 4;                // staging: one floatx4 of grad and of theta per thread and step
    const int kquads = NP / 4;                                   // floatx4s per row of K

    floatx16 ag[4], at[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) { ag[q][r] = 0.0f; at[q][r] = 0.0f; }

    // theta enters centred (theta_i k_i - sum_j K_ij theta_j does not see a common shift, its rounding does): this thread's four means
    const floatx4 mu = svgd_load4(means, c0 + scol, D, true);
    floatx4 pg, pt, pk[4];
    auto fetch = [&](int j0) {
        const int j = j0 + srow;
        const floatx4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
        pg = j < N ? svgd_load4(grad + (long)j * ld, c0 + scol, D, vec != 0) : zero;
        pt = j < N ? svgd_load4(theta + (long)j * ld, c0 + scol, D, vec != 0) - mu : zero;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int e = t + 256 * m, jj = e / kquads, quad = e - jj * kquads;
            pk[m] = jj < kStep ? *reinterpret_cast<const floatx4*>(K + (size_t)(j0 + jj) * NP + 4 * quad) : zero;
        }
    };
    fetch(0);
    for (int j0 = 0; j0 < NP; j0 += kStep) {
        __syncthreads();
        *reinterpret_cast<floatx4*>(&Gs[srow][scol]) = pg;
        *reinterpret_cast<floatx4*>(&Ts[srow][scol]) = pt;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int e = t + 256 * m, jj = e / kquads, quad = e - jj * kquads;
            if (jj < kStep) *reinterpret_cast<floatx4*>(&Ks[jj][4 * quad]) = pk[m];
        }
        __syncthreads();
        if (j0 + kStep < NP) fetch(j0 + kStep);
#pragma unroll
        for (int kk = 0; kk < kStep / 2; ++kk) {
            const float g = Gs[2 * kk + lk][32 * ct + lm], th = Ts[2 * kk + lk][32 * ct + lm];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int rt = (w >> 1) + 2 * q;
                if (rt < NT) {
                    const float k = Ks[2 * kk + lk][32 * rt + lm];
                    ag[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(g, k, ag[q], 0, 0, 0);
                    at[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(th, k, at[q], 0, 0, 0);
                }
            }
        }
    }
    // ag[q][r] is (K grad)[particle 32 rt + lm][column c0 + 32 ct + 8 (r >> 2) + 4 lk + (r & 3)]: four consecutive columns per lane
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int rt = (w >> 1) + 2 * q, i = 32 * rt + lm;
        if (rt >= NT || i >= N) continue;
        const float ki = ksum[i];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int c = c0 + 32 * ct + 8 * b + 4 * lk;
            if (c >= D) continue;
            const floatx4 th = svgd_load4(theta + (long)i * ld, c, D, vec != 0) - svgd_load4(means, c, D, true);
            floatx4 o;
            o.x = ag[q][4 * b + 0] - inv_bw * (ki * th.x - at[q][4 * b + 0]);
            o.y = ag[q][4 * b + 1] - inv_bw * (ki * th.y - at[q][4 * b + 1]);
            o.z = ag[q][4 * b + 2] - inv_bw * (ki * th.z - at[q][4 * b + 2]);
            o.w = ag[q][4 * b + 3] - inv_bw * (ki * th.w - at[q][4 * b + 3]);
            float* dst = out + (long)i * ld + c;
            if (vec && c + 3 < D) {
                *reinterpret_cast<floatx4*>(dst) = o;
            } else {
                dst[0] = o.x;
                if (c + 1 < D) dst[1] = o.y;
                if (c + 2 < D) dst[2] = o.z;
                if (c + 3 < D) dst[3] = o.w;
            }
        }
    }
}

int svgd_check_shape(const char* who, uint32_t n, uint64_t dim, uint64_t ld) {
    if (n < 2 || n > (uint32_t)kMaxParticles)
        return bsvi_fail(BSVI_ERR_INVALID, std::string(who) + ": " + std::to_string(n) + " particles, the kernels serve 2 .. 256");
    if (dim < 1 || ld < dim)
        return bsvi_fail(BSVI_ERR_INVALID, std::string(who) + ": dim " + std::to_string(dim) + ", ld " + std::to_string(ld) + " (1 <= dim <= ld)");
    if ((uint64_t)n * ld >= (1ull << 31))
        return bsvi_fail(BSVI_ERR_INVALID, std::string(who) + ": n_particles * ld = " + std::to_string((uint64_t)n * ld) + ", the limit is 2^31 - 1 elements");
    return BSVI_OK;
}

}  // namespace

extern "C" size_t bsvi_svgd_workspace_bytes(uint32_t n_particles, uint64_t dim) {
    if (svgd_check_shape("bsvi_svgd_workspace_bytes", n_particles, dim, dim) != BSVI_OK) return 0;
    return plan_for((int)n_particles, (int)dim).bytes;
}

extern "C" int bsvi_svgd_direction(const float* theta_dev, const float* grad_dev, float* out_dev, uint32_t n_particles, uint64_t dim,
                                   uint64_t ld, float bandwidth, float* bandwidth_out_dev, void* workspace_dev, void* stream) {
    if (!theta_dev || !grad_dev || !out_dev || !workspace_dev) return bsvi_fail(BSVI_ERR_INVALID, "bsvi_svgd_direction: null argument");
    const int rc = svgd_check_shape("bsvi_svgd_direction", n_particles, dim, ld);
    if (rc) return rc;
    if (bandwidth != bandwidth || bandwidth > 3.0e38f) return bsvi_fail(BSVI_ERR_INVALID, "bsvi_svgd_direction: the bandwidth is not finite");
    if (((uintptr_t)workspace_dev & 15u) != 0) return bsvi_fail(BSVI_ERR_INVALID, "bsvi_svgd_direction: the workspace is not 16-byte aligned");
    const int N = (int)n_particles, D = (int)dim;
    const Plan p = plan_for(N, D);
    char* ws = (char*)workspace_dev;
    float* header = (float*)ws;
    float* S = (float*)(ws + p.off_s);
    float* K = (float*)(ws + p.off_k);
    float* ksum = (float*)(ws + p.off_ksum);
    float* means = (float*)(ws + p.off_mean);
    float* part = (float*)(ws + p.off_part);
    hipStream_t s = (hipStream_t)stream;
    const int vec = (ld % 4 == 0 && (((uintptr_t)theta_dev | (uintptr_t)grad_dev | (uintptr_t)out_dev) & 15u) == 0) ? 1 : 0;

    hipLaunchKernelGGL(svgd_gram, dim3(p.splits, p.nt), dim3(256), 0, s, theta_dev, part, means, N, D, (long)ld, p.np, p.nt, p.chunks_per_split, p.n_chunks);
    hipLaunchKernelGGL(svgd_kernel, dim3(1), dim3(1024), 0, s, part, S, K, ksum, header, bandwidth_out_dev, N, p.np, p.nt, p.splits,
                       bandwidth > 0.0f ? bandwidth : 0.0f);
    hipLaunchKernelGGL(svgd_product, dim3((D + kColTile - 1) / kColTile), dim3(256), 0, s, theta_dev, grad_dev, out_dev, K, ksum, means, header,
                       N, D, (long)ld, p.np, p.nt, vec);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bsvi_fail(BSVI_ERR_HIP, std::string("bsvi_svgd_direction launch: ") + hipGetErrorString(e));
    if (!(bandwidth > 0.0f)) {
        // the median rule can fail (every particle in one place): the one word that says so is read back, which waits for the stream
        float bw = 0.0f;
        e = hipMemcpyAsync(&bw, header, sizeof bw, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return bsvi_fail(BSVI_ERR_HIP, std::string("bsvi_svgd_direction: ") + hipGetErrorString(e));
        if (!(bw > 0.0f))
            return bsvi_fail(BSVI_ERR_INVALID, "bsvi_svgd_direction: the median rule gives bandwidth 0 — all particles coincide; "
                                               "nothing was written, pass a bandwidth > 0 or start the particles apart");
    }
    return BSVI_OK;
}
