// Classifier-free guidance (hd_guide_combine / hd_sample_path_guided; no reference counterpart).  Included through kernels.hpp.
//   k_guide_combine   out = eps_u + w_b (eps_c - eps_u) per molecule, optionally rescaled towards the spread of eps_c (the
//                     noise-prediction form of "CFG rescale").
// One workgroup (256 threads) per molecule as k_slerp: sums over a molecule's valid entries accumulate in double, strided per thread,
// then an xor butterfly, then the four wave partials in a fixed tree; no atomics; exact fp32 outputs.  Draws nothing.
#pragma once
#include "common.hpp"

struct GuideArgs {
    const float* eps_c;   // [B][N][D] network output under the context
    const float* eps_u;   // [B][N][D] network output under the null context
    const float* w;       // [w_rows] guidance scale, w_rows = 1 (shared) or B
    const uint8_t* nm;    // [B*N] node mask bytes
    float* out;           // [B][N][D]; may be eps_c itself (every thread reads the entries it writes, behind the last reduction)
    float rescale;        // phi in [0, 1]; 0: no reduction runs
    int w_rows, B, N, D;
};

// sums of K doubles over the workgroup, result in every thread; `red` is 4 * K doubles of LDS scratch
template <int K>
HD_DEVINL void guide_block_sum(double (&v)[K], double* red, int tid) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    __syncthreads();                               // previous use of `red` is over
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[(tid >> 6) * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (red[k] + red[K + k]) + (red[2 * K + k] + red[3 * K + k]);
}

// w_b == 1 copies eps_c and w_b == 0 copies eps_u (bit for bit, phi ignored); otherwise g = fmaf(w_b, ec - eu, eu) and, with
// phi > 0, out = f g with f = fp32(phi sqrt(S_c / S_g) + (1 - phi)), S_c / S_g the sums of squared deviations of eps_c / g from their
// means over the molecule's valid entries (all D columns); S_g == 0 or a non-finite quotient: f = 1.  Masked entries are exactly 0.
__global__ __launch_bounds__(256) void k_guide_combine(GuideArgs a) {
    __shared__ double red[4 * 3];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = a.N, D = a.D, total = N * D;
    const size_t base = (size_t)b * total;
    const float w = a.w[a.w_rows == 1 ? 0 : b];
    const float* ec = a.eps_c + base;
    const float* eu = a.eps_u + base;
    float* out = a.out + base;
    const uint8_t* nm = a.nm + (size_t)b * N;
    if (w == 1.f || w == 0.f) {                    // uniform over the workgroup
        const float* src = w == 1.f ? ec : eu;
        for (int e = tid; e < total; e += 256) out[e] = nm[e / D] ? src[e] : 0.f;
        return;
    }
    if (a.rescale == 0.f) {                        // uniform over the grid
        for (int e = tid; e < total; e += 256) {
            const float c = ec[e], u = eu[e];
            out[e] = nm[e / D] ? __builtin_fmaf(w, c - u, u) : 0.f;
        }
        return;
    }
    double s[3] = {0.0, 0.0, 0.0};                 // sum eps_c, sum g, valid entries
    for (int e = tid; e < total; e += 256) {
        if (!nm[e / D]) continue;
        const float c = ec[e], u = eu[e];
        s[0] += (double)c; s[1] += (double)__builtin_fmaf(w, c - u, u); s[2] += 1.0;
    }
    guide_block_sum<3>(s, red, tid);
    const double mc = s[2] > 0.0 ? s[0] / s[2] : 0.0, mg = s[2] > 0.0 ? s[1] / s[2] : 0.0;
    double q[2] = {0.0, 0.0};                      // S_c, S_g
    for (int e = tid; e < total; e += 256) {
        if (!nm[e / D]) continue;
        const float c = ec[e], u = eu[e];
        const double dc = (double)c - mc, dg = (double)__builtin_fmaf(w, c - u, u) - mg;
        q[0] += dc * dc; q[1] += dg * dg;
    }
    guide_block_sum<2>(q, red, tid);               // every thread holds the same sums: f needs no broadcast
    double r = 1.0;
    if (q[1] > 0.0) {
        const double t = sqrt(q[0] / q[1]);
        if (t - t == 0.0) r = t;                   // finite
    }
    const float f = (float)((double)a.rescale * r + (1.0 - (double)a.rescale));
    for (int e = tid; e < total; e += 256) {
        const float c = ec[e], u = eu[e];
        out[e] = nm[e / D] ? f * __builtin_fmaf(w, c - u, u) : 0.f;
    }
}
